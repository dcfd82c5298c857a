# coding=utf-8
"""GPU: the last stage of a training step on gradients the reference knows.

csrc/engine_train.h train_apply -- train_learning_rate, the scale, the element-wise clip, one of
adadelta / momentum / adam / rmsprop_kernel (csrc/train_kernels.h), Adam's beta powers,
train_pack_all, global_step -- is otherwise reached only at the end of whole training steps, where
its input is the GPU's own gradient and the assertions have to absorb that gradient's summation
noise (Adam parameters: the whole step).  Here one train_forward_backward of the batch-2,
hidden-128 engine makes the gradient buffer live, the buffer is OVERWRITTEN through
parallel.engine_grad_tensor with known values, and train_apply is compared with
oracle.apply_optimizer / oracle.learning_rate in float64 (tests/optimizer_cases.py).

Bound (parts 1, 2).  Every element of every parameter: |gpu - ref64| <= c_p 2^-24 path, path =
|w0| + sum over the applies of |dw_ref64|; every slot element: |gpu - ref64| <= c_s 2^-24 |ref64|
(1e-30 absolute where |ref64| <= 1e-30).  c_p, c_s are 4 x the constants the float32 oracle run
has on the same inputs (printed beside the GPU's), and the oracle's own must stay <= 16.

Measured on an MI355X, max over the three (grad_scale, clip) pairs and three applies (23
parameters, 4.49 M elements; the kernels are built with -ffp-contract=off and their sqrt and
division are correctly rounded, so the GPU's constants came out equal to the float32 oracle's in
every one of the 36 applies):

  optimizer   fp32 oracle c_p   c_s      MI355X c_p   c_s
  adadelta        4.97          8.89        4.97      8.89
  momentum        3.61          5.07        3.61      5.07
  adam            4.27          5.34        4.27      5.34
  rmsprop         3.29          4.24        3.29      4.24

The corners came out within 1.5 x 2^-24 path, Adam's alpha within 1.4; the schedules are bit-equal
to np.float32(oracle.learning_rate) except 1 ulp at cosine step 3 and staircase step 70
(init_lr reaches the engine as a float32 field).

Part 3: exact corners on one bias (zero gradient and zero slots, the clip boundary, clip after
scale, clip off, +-inf, NaN: a NaN gradient reaches the parameter and the slots, as np.clip in
oracle.train_step keeps it).  Part 4: the learning-rate schedules read back bit for bit through a
momentum step of gradient 1.0 from zero, cosine at and past max_steps, the staircase past several
boundaries, emb_lr, world 4; Adam's alpha at the first and a late step.  Part 5: the derived
weight forms after an apply, per compute mode.  Part 6: Saver.save / Saver.restore resume equals
the uninterrupted run, bit for bit, per optimizer.
"""
import copy

import numpy as np
import pytest
import torch

from multiverse_amd import parallel, pred_models, pred_utils, synth
from oracle import multiverse_oracle as oracle

import optimizer_cases as oc

pytestmark = pytest.mark.gpu
_SC_IDS = ["scale1_clip10", "scale_third_clip10", "scale_eighth_noclip"]


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _b1(x):
  return int(np.float32(x).view(np.uint32))


def _same_bits(a, b):
  return np.array_equal(_bits(a), _bits(b))


class _Rig(object):
  """One engine whose gradient buffer is live (one train_forward_backward) and is then written
  by the tests; train_init with another config re-targets the optimizer and the schedule."""

  def __init__(self, lib):
    self.cfg = oc.base_config(single_decoder=True)
    params = synth.make_params(self.cfg, seed=synth.SEED_BASE + 3, recurrent_gain=2.0,
                               bias_scale=0.1)
    feed = synth.make_feed(self.cfg, seed=synth.SEED_BASE + 53)
    self.eng = lib.Engine(self.cfg, device=0)
    self.eng.set_params(params)
    self.eng.train_init()
    self.eng.train_forward_backward(feed)
    self.specs = self.eng.param_specs()
    self.layout, self.total = oc.layout(self.specs)
    self.no_grad = tuple(n for n, _ in self.specs if oc.is_no_grad(self.cfg, n))
    self.grad = parallel.engine_grad_tensor(self.eng, 0)
    assert self.grad.numel() == self.total and self.grad.dtype == torch.float32

  def init(self, cfg, world=1, step=0, powers=None):
    self.eng.train_init(cfg, world=world)
    if powers is not None:
      self.eng.set_opt_scalars(float(powers[0]), float(powers[1]))
    self.eng.global_step = step

  def load(self, inputs):
    for n, (w, _, s0, s1) in inputs.items():
      self.eng.set_param(n, w)
      self.eng.set_opt_slot(n, 0, s0)
      self.eng.set_opt_slot(n, 1, s1)

  def write_grads(self, grads):
    """grads: {name: array}; parameters not named get zeros, pad elements the sentinel."""
    full = {n: grads.get(n, np.zeros(s, np.float32)) for n, s in self.specs}
    flat = oc.flat_gradients(self.specs, full)
    self.grad.copy_(torch.from_numpy(flat))
    torch.cuda.synchronize()
    return flat

  def read_grads(self):
    torch.cuda.synchronize()
    return self.grad.cpu().numpy()

  def state(self, names, nslots):
    return ({n: self.eng.get_param(n) for n in names},
            {n: tuple(self.eng.get_opt_slot(n, i) for i in range(nslots)) for n in names})


@pytest.fixture(scope="module")
def rig(built_lib):
  r = _Rig(built_lib)
  yield r
  r.eng.close()


def test_layout_has_the_sizes_the_kernels_can_get_wrong(rig):
  sizes = [size for _, _, _, size in rig.layout]
  assert any(s % 64 for s in sizes)                          # ends inside the layout's pad
  assert any(s % 256 and not s % 64 for s in sizes)          # a partial last block, no pad
  assert any(s > 256 and s % 256 == 0 for s in sizes)        # whole blocks
  assert len(rig.no_grad) == 4                               # regression encoders, both grids


# ------------------------------------------------------------ parts 1 and 2
@pytest.mark.parametrize("scale,clip", oc.SCALE_CLIP, ids=_SC_IDS)
@pytest.mark.parametrize("optimizer", oc.OPTIMIZERS)
def test_apply_matches_the_fp64_reference(rig, optimizer, scale, clip):
  cfg = oc.optimizer_config(rig.cfg, optimizer, clip=clip)
  nsl = oc.NUM_SLOTS[optimizer]
  inputs = oc.make_inputs(rig.specs, optimizer)
  for n in rig.no_grad:          # large finite gradients: an update of these would show
    w, g, s0, s1 = inputs[n]
    inputs[n] = (w, (np.sign(g) * (np.float32(1e3) + np.abs(g))).astype(np.float32), s0, s1)
  powers = oc.ADAM_START_POWERS if optimizer == "adam" else (np.float32(0.5), np.float32(0.25))
  rig.init(cfg, powers=powers)
  rig.load(inputs)
  flat = rig.write_grads({n: v[1] for n, v in inputs.items()})
  names = [n for n, _ in rig.specs]
  adam_powers = powers if optimizer == "adam" else None
  ref64 = oc.reference_run(cfg, inputs, scale, 3, np.float64, powers=adam_powers,
                           skip=rig.no_grad)
  ref32 = oc.reference_run(cfg, inputs, scale, 3, np.float32, powers=adam_powers,
                           skip=rig.no_grad)
  path = oc.paths(inputs, ref64)
  bad = []
  for k in range(3):
    rig.eng.train_apply(scale)
    gp, gs = rig.state(names, 2)
    c_gpu = oc.error_constants(gp, gs, ref64[k], path[k], nsl, skip=rig.no_grad)
    c_32 = oc.error_constants(ref32[k]["params"], ref32[k]["slots"], ref64[k], path[k], nsl,
                              skip=rig.no_grad)
    print("%-8s scale %.3g clip %s apply %d (lr %.6g): fp32 oracle c_p %.2f c_s %.2f | gpu "
          "c_p %.2f c_s %.2f tiny-slot abs %.1e" % (optimizer, scale, clip, k, ref64[k]["lr"],
                                                    c_32[0], c_32[1], c_gpu[0], c_gpu[1],
                                                    c_gpu[2]))
    assert c_32[0] <= oc.ORACLE_CEILING and c_32[1] <= oc.ORACLE_CEILING, "ill-conditioned input"
    if not oc.within_bounds(c_gpu, c_32):
      bad.append((k, c_gpu, c_32))
    # scalars: Adam's powers are the float32 products, bit for bit; the others' do not move
    want = ref64[k]["powers"] if optimizer == "adam" else powers
    assert rig.eng.opt_scalars() == (float(want[0]), float(want[1]))
    assert rig.eng.global_step == k + 1
    # part 2: no_grad parameters and both of their slots, and the whole gradient buffer
    for n in rig.no_grad:
      assert _same_bits(gp[n], inputs[n][0]), n
      assert _same_bits(gs[n][0], inputs[n][2]) and _same_bits(gs[n][1], inputs[n][3]), n
    assert _same_bits(rig.read_grads(), flat), "train_apply wrote the gradient buffer"
  if optimizer == "momentum":       # the slot the optimizer does not have stays as it was set
    for n in names:
      assert _same_bits(gs[n][1], inputs[n][3]), n
  assert not bad, bad


# ------------------------------------------------------------ part 3
def _corner_param(rig):
  name, shape = next((n, s) for n, s in rig.specs if n.endswith("grid_emb/b"))
  assert shape == (32,)
  return name, 32


@pytest.mark.parametrize("optimizer", oc.OPTIMIZERS)
def test_exact_corners(rig, optimizer):
  name, size = _corner_param(rig)
  nsl = oc.NUM_SLOTS[optimizer]
  bad = []
  for case in sorted(oc.CORNER_CASES):
    scale, clip, vals = oc.CORNER_CASES[case]
    cfg = oc.optimizer_config(rig.cfg, optimizer, clip=clip, init_lr=oc.CORNER_LR,
                              learning_rate_decay=None)
    inputs = oc.corner_inputs(optimizer, name, size, case)
    w0, g = inputs[name][0], inputs[name][1]
    first = (np.float32(0.9), np.float32(0.999))     # Adam's powers at step 0 (the engine keeps
    rig.init(cfg, powers=first)                      # them across train_init of one optimizer)
    rig.load(inputs)
    rig.write_grads({name: g})
    rig.eng.train_apply(scale)
    gp, gs = rig.state([name], nsl)
    ref = oc.reference_run(cfg, inputs, scale, 1, np.float64, powers=first)[0]
    model = oc.device_model_run(cfg, inputs, scale, 1, powers=first)[0]
    nan = np.isnan(g)
    fin = ~nan
    # NaN in: NaN in the parameter and in every slot the optimizer has
    if nan.any():
      assert np.isnan(ref["params"][name][nan]).all()
      for what, a in [("param", gp[name])] + [("slot %d" % i, gs[name][i]) for i in range(nsl)]:
        if not np.isnan(a[nan]).all():
          bad.append((case, what, "NaN gradient applied as", a[nan].tolist()))
    # everything else (+-clip, one float beyond / inside, +-inf, clip order, clip off, the
    # neighbours): finite and at the fp64 value
    d = np.abs(ref["params"][name] - w0.astype(np.float64))
    pth = np.abs(w0.astype(np.float64)) + d
    err = np.abs(gp[name].astype(np.float64) - ref["params"][name])
    print("%-8s %-11s param max err %.2f x 2^-24 path" % (
        optimizer, case, float(np.max(err[fin] / (oc.U * pth[fin])))))
    if not (np.isfinite(gp[name][fin]).all() and (err[fin] <= oc.CORNER_C * oc.U * pth[fin]).all()):
      bad.append((case, "param", gp[name].tolist(), ref["params"][name].tolist()))
    for i in range(nsl):
      r = ref["slots"][name][i]
      e = np.abs(gs[name][i].astype(np.float64) - r)
      tol = np.where(np.abs(r) > oc.TINY, oc.CORNER_C * oc.U * np.abs(r), oc.TINY)
      if not (e[fin] <= tol[fin]).all():
        bad.append((case, "slot %d" % i, gs[name][i].tolist(), r.tolist()))
    # zero gradient (+0 and -0) from zero slots: bitwise unchanged
    zero = g == 0
    assert zero.sum() >= (2 if case in ("boundary", "clip_off") else 0)
    if not _same_bits(gp[name][zero], w0[zero]):
      bad.append((case, "zero gradient moved the parameter", gp[name][zero].tolist()))
    if optimizer != "rmsprop" and not _same_bits(gs[name][0][zero], np.zeros(int(zero.sum()))):
      bad.append((case, "zero gradient moved slot 0", gs[name][0][zero].tolist()))
    # momentum from a zero accumulator with a power-of-two lr: w - lr g_clipped has one
    # rounding, the float32 answer is exact
    if optimizer == "momentum":
      if not _same_bits(gp[name][fin], model["params"][name][fin]):
        bad.append((case, "momentum not bitwise", gp[name].tolist(),
                    model["params"][name].tolist()))
      if not _same_bits(gs[name][0][fin], model["slots"][name][0][fin]):
        bad.append((case, "momentum accumulator not bitwise", gs[name][0].tolist()))
  z = np.zeros(size, np.float32)          # leave no NaN behind in the shared engine
  rig.load({name: (z, z, z, z)})
  assert not bad, bad


# ------------------------------------------------------------ part 4
_PROBE = "person_pred/scene_conv1/b"


def _schedule_cfg(rig, schedule, emb_lr, world):
  """max_steps 7 (odd) and decay_steps 14 at this world: train_num_examples scales with it."""
  return oc.optimizer_config(
      rig.cfg, "momentum", clip=10.0, emb_lr=emb_lr, use_cosine_lr=(schedule == "cosine"),
      learning_rate_decay=(None if schedule == "constant" else 0.95),
      train_num_examples=14 * world, num_epochs=1, num_epoch_per_decay=2.0)


def _probe_rate(rig, step):
  """-(parameter) after one momentum apply of gradient 1.0 from w = 0, accumulator 0 at `step`:
  the float32 learning rate itself."""
  z = np.zeros(64, np.float32)
  rig.eng.set_param(_PROBE, z)
  rig.eng.set_opt_slot(_PROBE, 0, z)
  rig.eng.global_step = step
  rig.eng.train_apply(1.0)
  assert rig.eng.global_step == step + 1
  got = rig.eng.get_param(_PROBE)
  assert (_bits(got) == _bits(got)[0]).all()
  return got[0]


@pytest.mark.parametrize("schedule,emb_lr,world", [
    ("cosine", 1.0, 1), ("staircase", 1.0, 1), ("cosine", 0.5, 1), ("staircase", 0.5, 1),
    ("cosine", 1.0, 4), ("staircase", 1.0, 4), ("constant", 1.0, 1)])
def test_learning_rate_schedule_read_back(rig, schedule, emb_lr, world):
  assert dict(rig.specs)[_PROBE] == (64,)
  cfg = _schedule_cfg(rig, schedule, emb_lr, world)
  ref_cfg = copy.copy(cfg)
  ref_cfg.batch_size = cfg.batch_size * world      # the schedules count global-batch steps
  if schedule == "cosine":
    max_steps = 7
    assert int(ref_cfg.train_num_examples / ref_cfg.batch_size * ref_cfg.num_epochs) == max_steps
    steps = [0, 1, max_steps // 2, max_steps - 1, max_steps, max_steps + 5]
  elif schedule == "staircase":
    ds = 14
    assert int(ref_cfg.train_num_examples / ref_cfg.batch_size * ref_cfg.num_epoch_per_decay) == ds
    steps = [ds - 1, ds, 2 * ds - 1, 2 * ds, 5 * ds]
  else:
    steps = [10 ** 6]
  want = [np.float32(oracle.learning_rate(ref_cfg, s)) for s in steps]
  if world > 1:       # the boundaries did move: a world-blind schedule reads differently
    assert [np.float32(oracle.learning_rate(cfg, s)) for s in steps] != want
  rig.init(cfg, world=world)
  rig.write_grads({_PROBE: np.ones(64, np.float32)})
  bad = []
  for s, w in zip(steps, want):
    got = _probe_rate(rig, s)
    if w == 0:          # at and past max_steps: the parameter is bitwise unchanged (+0.0)
      ok = _b1(got) == 0
    else:
      ok = abs(_b1(-got) - _b1(w)) <= 1
    if (_b1(got) != 0) if w == 0 else (_b1(-got) != _b1(w)):
      print("%s emb_lr %g world %d step %d: engine %.9g oracle %.9g" % (
          schedule, emb_lr, world, s, -got, w))
    if not ok:
      bad.append((s, float(-got), float(w)))
  rig.init(cfg, world=1)
  assert not bad, bad


@pytest.mark.parametrize("k", [1, 1000])
def test_adam_alpha_at_the_first_and_a_late_step(rig, k):
  """alpha = lr sqrt(1 - beta2_power) / (1 - beta1_power): at powers (0.9, 0.999) 1 - beta2_power
  is a difference of near-equal float32 numbers; at step 1000 beta1_power has underflowed."""
  cfg = oc.optimizer_config(rig.cfg, "adam", learning_rate_decay=None)
  powers = (np.float32(0.9 ** k), np.float32(0.999 ** k))
  z = np.zeros(64, np.float32)
  inputs = {_PROBE: (z, np.ones(64, np.float32), z.copy(), z.copy())}
  rig.init(cfg, powers=powers)
  rig.load(inputs)
  rig.write_grads({_PROBE: inputs[_PROBE][1]})
  rig.eng.train_apply(1.0)
  gp, gs = rig.state([_PROBE], 2)
  ref = oc.reference_run(cfg, inputs, 1.0, 1, np.float64, powers=powers)[0]
  want = ref["params"][_PROBE]
  err = np.abs(gp[_PROBE].astype(np.float64) - want)
  print("adam alpha at step %d: parameter %.9g oracle %.9g (%.2f x 2^-24)" % (
      k, gp[_PROBE][0], want[0], float(np.max(err / (oc.U * np.abs(want))))))
  assert (want < 0).all() and (err <= oc.CORNER_C * oc.U * np.abs(want)).all()
  for i in range(2):
    r = ref["slots"][_PROBE][i]
    assert (np.abs(gs[_PROBE][i] - r) <= oc.CORNER_C * oc.U * np.abs(r)).all()
  b1, b2 = rig.eng.opt_scalars()
  assert (b1, b2) == (float(powers[0] * np.float32(0.9)), float(powers[1] * np.float32(0.999)))


# ------------------------------------------------------------ part 5
def _forward_and_grads(eng, feed):
  cls, reg = eng.forward_greedy(feed)
  loss = eng.train_forward_backward(feed)
  return cls, reg, loss, {n: eng.get_grad(n) for n, _ in eng.param_specs()}


@pytest.mark.parametrize("mode", ["f32", "f16x3", "bf16"])
def test_derived_weight_forms_follow_an_apply(built_lib, mode):
  """train_apply re-packs every derived form of the weights (train_pack_all) and invalidates the
  inference forms: the greedy forward and the next gradients of the engine that stepped are
  bitwise those of a fresh engine handed its parameters."""
  cfg = oc.optimizer_config(oc.base_config(), "momentum", learning_rate_decay=None)
  params = synth.make_params(cfg, seed=synth.SEED_BASE + 4, recurrent_gain=2.0, bias_scale=0.1)
  feed = synth.make_feed(cfg, seed=synth.SEED_BASE + 54)
  eng = built_lib.Engine(cfg, device=0)
  eng.set_params(params)
  eng.set_compute_mode(mode)
  eng.train_init(cfg)
  eng.train_forward_backward(feed)
  specs = eng.param_specs()
  grads = {}
  for i, (n, s) in enumerate(specs):       # N(0,1): every weight moves by about lr = 0.01
    grads[n] = np.random.default_rng([oc.SEED, 5, i]).normal(0.0, 1.0, s).astype(np.float32)
  t = parallel.engine_grad_tensor(eng, 0)
  t.copy_(torch.from_numpy(oc.flat_gradients(specs, grads, fill=0.0)))
  torch.cuda.synchronize()
  eng.train_apply(1.0)
  stepped = {n: eng.get_param(n) for n, _ in specs}
  for n, s in specs:
    if n.endswith("/kernel"):
      assert (stepped[n] != params[n]).mean() > 0.99, n
      assert np.abs(256.0 * stepped[n]).max() < 60000.0
  a = _forward_and_grads(eng, feed)
  eng.close()
  fresh = built_lib.Engine(cfg, device=0)
  fresh.set_params(stepped)
  fresh.set_compute_mode(mode)
  fresh.train_init(cfg)
  b = _forward_and_grads(fresh, feed)
  fresh.close()
  for s in range(2):
    K = cfg.scene_grids[s][0] * cfg.scene_grids[s][1]
    assert np.isfinite(a[0][s]).all() and np.isfinite(a[1][s]).all()
    assert _same_bits(a[0][s], b[0][s]) and _same_bits(a[1][s], b[1][s]), (mode, s)
    assert (a[0][s].reshape(2, -1, K).argmax(-1) == b[0][s].reshape(2, -1, K).argmax(-1)).all()
  assert a[2] == b[2] and np.isfinite(a[2][0])
  for n in a[3]:
    assert _same_bits(a[3][n], b[3][n]), (mode, n)


# ------------------------------------------------------------ part 6
def _engine_state(model, nslots):
  eng = model.engine
  names = [n for n, _ in eng.param_specs()]
  return {"params": {n: eng.get_param(n) for n in names},
          "slots": {n: [eng.get_opt_slot(n, i) for i in range(nslots)] for n in names},
          "scalars": eng.opt_scalars(), "step": eng.global_step}


@pytest.mark.parametrize("optimizer", oc.OPTIMIZERS)
def test_resume_equals_the_uninterrupted_run(built_lib, tmp_path, optimizer):
  """2 steps, Saver.save, a new model, Saver.restore, 2 more steps == 4 steps.  decay_steps 2:
  the staircase moves right after the resume, so a lost global_step shows; a lost beta power
  shows for Adam; the checkpoint stores float32, so everything is bitwise."""
  cfg = oc.optimizer_config(oc.base_config(), optimizer)
  assert cfg.keep_prob == 1.0 and oracle.learning_rate(cfg, 1) != oracle.learning_rate(cfg, 2)
  nsl = oc.NUM_SLOTS[optimizer]
  data = synth.make_npz_data(cfg, 8, seed=13)
  ds = pred_utils.dataset_from_npz_dict(data, "train", cfg)
  batches = list(ds.get_batches(2, full=True, shuffle=False))
  assert len(batches) == 4
  params = synth.make_params(cfg, seed=synth.SEED_BASE + 6, recurrent_gain=2.0, bias_scale=0.1)

  def train(model, bts):
    trainer = pred_models.Trainer(model, cfg)
    return [trainer.step(None, bt) for bt in bts]

  whole = pred_models.get_model(cfg, 0)
  whole.load_params(params)
  l_whole = train(whole, batches)
  want = _engine_state(whole, nsl)
  whole.close()

  first = pred_models.get_model(cfg, 0)
  first.load_params(params)
  l_first = train(first, batches[:2])
  path = pred_utils.Saver().save(first, str(tmp_path / "save"), global_step=first.engine.global_step)
  first.close()
  second = pred_models.get_model(cfg, 0)
  pred_utils.Saver().restore(second, path)
  assert second.engine.global_step == 2
  l_second = train(second, batches[2:])
  got = _engine_state(second, nsl)
  second.close()

  def flat(ls):
    return [float(l[0]) for l in ls] + [float(l[2]) for l in ls] + \
        [float(x) for l in ls for x in l[3]]

  assert np.isfinite(flat(l_whole)).all()
  assert flat(l_first + l_second) == flat(l_whole)
  assert got["step"] == want["step"] == 4
  if optimizer == "adam":
    assert got["scalars"] == want["scalars"]
    assert got["scalars"][0] == float(np.float32(0.9) * np.float32(0.9) * np.float32(0.9)
                                      * np.float32(0.9) * np.float32(0.9))
  for n in want["params"]:
    assert _same_bits(got["params"][n], want["params"][n]), n
    for i in range(nsl):
      assert _same_bits(got["slots"][n][i], want["slots"][n][i]), (n, i)
