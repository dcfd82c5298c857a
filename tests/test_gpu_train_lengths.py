# coding=utf-8
"""GPU: one training step over rows of different history and horizon
(include/multiverse_hip.h mv_set_train_lengths) against the composition of uniform oracle runs
(tests/train_lengths_oracle.py), and the identities that keep the uniform step what it was.

Shapes: obs_len 4, pred_len 3, batch 5 -- the smallest at which a row joins the encoders late, a
row finishes early, a padding row sits inside a prefix and the order is not sorted.
  case A  coarse scale, unsorted   Lo = [4, 2, 4, 1, 3]   L = [3, 3, 0, 2, 1]
  case B  both scales, sorted      Lo = [4, 3, 3, 2, 4]   L = [3, 3, 2, 1, 0]
Bars: those of tests/test_gpu_train.py::test_gradients_match_oracle -- loss parts rtol 1e-4 /
atol 1e-5 against the fp32 composition, every gradient tensor within 2e-3 of its max against
the fp64 composition (the fp32 composition's own error is printed beside it)."""
import copy

import numpy as np
import pytest
import torch

from multiverse_amd import synth
from oracle import multiverse_oracle as oracle

import train_lengths_oracle as tlo

pytestmark = pytest.mark.gpu

TO, TP, N = 4, 3, 5
CASES = {"A": ((0, 1), [4, 2, 4, 1, 3], [3, 3, 0, 2, 1]),
         "B": ((1, 1), [4, 3, 3, 2, 4], [3, 3, 2, 1, 0])}


def _rel(a, b):
  a = np.asarray(a, dtype=np.float64)
  b = np.asarray(b, dtype=np.float64)
  return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _case(name, gnn=True, seed=1, **over):
  use_grids, lo, lp = CASES[name]
  cfg = synth.default_config(batch_size=N, use_grids=use_grids, is_train=True, obs_len=TO,
                             pred_len=TP, use_gnn=gnn, **over)
  params = synth.make_params(cfg, seed=synth.SEED_BASE + seed, recurrent_gain=2.0,
                             bias_scale=0.1)
  feed = synth.make_feed(cfg, seed=synth.SEED_BASE + 50 + seed)
  if cfg.use_soft_grid_class:
    feed["grid_pred_soft"] = [oracle.soft_grid_labels(feed["grid_pred_labels"][s], h, w,
                                                      cfg.soft_grid)
                              for s, (h, w) in enumerate(cfg.scene_grids)]
  return cfg, params, feed, lo, lp


def _engine(built_lib, cfg, params, mode="f32"):
  eng = built_lib.Engine(cfg, device=0)
  eng.set_params(params)
  eng.set_compute_mode(mode)
  eng.train_init()
  return eng


def _grads(eng):
  return {n: eng.get_grad(n) for n, _ in eng.param_specs()}


def _params(eng):
  return {n: eng.get_param(n) for n, _ in eng.param_specs()}


def _same(a, b):
  """bitwise: the same bytes (a zero's sign included)"""
  return all(np.array_equal(a[n].view(np.uint32), b[n].view(np.uint32)) for n in a)


def _check_against_composition(eng, cfg, params, feed, lo, lp, key, tag):
  loss, wd, pgl = eng.train_forward_backward(
      dict(feed, train_obs_lengths=lo, train_pred_lengths=lp))
  o32 = tlo.loss_and_grads(params, cfg, feed, lo, lp, cache_key=key)
  o64 = tlo.loss_and_grads(params, cfg, feed, lo, lp, dtype=torch.float64, cache_key=key)
  print("%s: loss gpu %.6f composition %.6f | wd %.6g / %.6g | parts %s / %s"
        % (tag, loss, o32[0], wd, o32[1], pgl, o32[2]))
  assert abs(loss - o32[0]) < 1e-4 * max(1.0, abs(o32[0]))
  assert abs(wd - o32[1]) < 1e-5 * max(1.0, abs(o32[1]))
  assert np.allclose(pgl, o32[2], rtol=1e-4, atol=1e-5)
  worst = 0.0
  for name, _ in eng.param_specs():
    g = eng.get_grad(name)
    assert np.isfinite(g).all(), name
    e_gpu, e_cpu = _rel(g, o64[3][name]), _rel(o32[3][name], o64[3][name])
    worst = max(worst, e_gpu)
    print("%-78s rel err gpu %.2e (fp32 composition %.2e) max|g| %.3g"
          % (name, e_gpu, e_cpu, np.abs(o64[3][name]).max()))
  assert worst < 2e-3
  return loss, wd, pgl


# ------------------------------------------------------------ 1. parity with the composition

@pytest.mark.parametrize("case,gnn,mode", [("A", True, "f32"), ("A", True, "f16x3"),
                                           ("A", False, "f32"), ("A", False, "f16x3"),
                                           ("B", True, "f16x3")])
def test_gradients_match_the_composition(built_lib, case, gnn, mode):
  """Loss parts and every parameter's gradient (wd = 0.001: the wd * W term and wd_loss ride
  in every case)."""
  cfg, params, feed, lo, lp = _case(case, gnn)
  assert cfg.wd > 0
  eng = _engine(built_lib, cfg, params, mode)
  _, wd, _ = _check_against_composition(eng, cfg, params, feed, lo, lp, (case, gnn),
                                        "case %s gnn %s %s" % (case, gnn, mode))
  assert wd > 0
  eng.close()


@pytest.mark.parametrize("name,over", [
    ("soft", dict(use_soft_grid_class=True, soft_grid=4)),
    ("mask", dict(mask_grid_regression=True)),
    ("dense_feedback", dict(train_w_onehot=False)),                # class_feedback 1
    ("teacher", dict(use_teacher_forcing=True))])                  # class_feedback 2 + reg tf
def test_loss_and_input_switches_match_the_composition(built_lib, name, over):
  cfg, params, feed, lo, lp = _case("A", True, **over)
  eng = _engine(built_lib, cfg, params, "f32")
  _check_against_composition(eng, cfg, params, feed, lo, lp, ("A", name), "case A " + name)
  eng.close()


# ------------------------------------------------------------ 2. all lengths full

@pytest.mark.parametrize("mode,keep_prob", [("f16x3", 1.0), ("f32", 1.0), ("f16x3", 0.7)])
def test_full_lengths_are_the_uniform_step_bitwise(built_lib, mode, keep_prob):
  cfg, params, feed, _, _ = _case("B", True, keep_prob=keep_prob)
  out = []
  for with_lengths in (False, True):
    eng = _engine(built_lib, cfg, params, mode)
    eng.set_dropout_seed(4242)
    fd = dict(feed, train_obs_lengths=[TO] * N, train_pred_lengths=[TP] * N) \
        if with_lengths else feed
    losses = eng.train_forward_backward(fd)
    grads = _grads(eng)
    rows = eng.last_train_gate_rows()
    eng.set_dropout_seed(4242)
    losses2 = eng.train_step(fd)
    out.append((losses, grads, rows, losses2, _params(eng)))
    eng.close()
  assert out[0][0] == out[1][0] and out[0][3] == out[1][3]
  assert _same(out[0][1], out[1][1])
  assert out[0][2] == out[1][2]
  assert _same(out[0][4], out[1][4])


# ------------------------------------------------------------ 3. ignored content

def _scribbled(cfg, feed, lo, lp):
  """The same batch with everything the lengths ignore replaced: the observation columns in
  front of each row's window, the target columns from L[n] on, the whole padding row --
  in-range labels and frame indices, finite floats."""
  other = synth.make_feed(cfg, seed=synth.SEED_BASE + 977)
  out = copy.deepcopy(feed)
  for n in range(N):
    first = 0 if lp[n] == 0 else TO - lo[n]     # padding row: every observation column
    cut = TO if lp[n] == 0 else first
    out["obs_scene"][n, :cut] = 1 - out["obs_scene"][n, :cut]          # (two frames: 0 / 1)
    for s, use in enumerate(cfg.use_grids):
      if not use:
        continue
      out["grid_obs_labels"][s][n, :cut] = other["grid_obs_labels"][s][n, :cut]
      out["grid_obs_regress"][s][n, :cut] = other["grid_obs_regress"][s][n, :cut] * 1.5
      out["grid_pred_labels"][s][n, lp[n]:] = other["grid_pred_labels"][s][n, lp[n]:]
      out["grid_pred_regress"][s][n, lp[n]:] = other["grid_pred_regress"][s][n, lp[n]:] - 3.0
  assert int(out["obs_scene"].max()) <= 1 and int(out["obs_scene"].min()) >= 0
  return out


@pytest.mark.parametrize("case,mode,keep_prob,over", [
    ("A", "f16x3", 1.0, {}), ("A", "f32", 1.0, {}), ("B", "f16x3", 1.0, {}),
    ("A", "f16x3", 0.7, {}), ("A", "f32", 0.7, {}),
    ("A", "f32", 1.0, dict(use_soft_grid_class=True, soft_grid=4, mask_grid_regression=True)),
    ("A", "f32", 1.0, dict(use_teacher_forcing=True))])
def test_ignored_content_changes_no_bit(built_lib, case, mode, keep_prob, over):
  cfg, params, feed, lo, lp = _case(case, True, keep_prob=keep_prob, **over)
  scribbled = _scribbled(cfg, feed, lo, lp)
  changed = sum(int((np.asarray(feed[k][s]) != np.asarray(scribbled[k][s])).sum())
                for k in ("grid_obs_labels", "grid_pred_regress")
                for s, use in enumerate(cfg.use_grids) if use)
  assert changed > 0
  eng = _engine(built_lib, cfg, params, mode)
  out = []
  for fd in (feed, scribbled):
    eng.set_dropout_seed(99)
    losses = eng.train_forward_backward(
        dict(fd, train_obs_lengths=lo, train_pred_lengths=lp))
    out.append((losses, _grads(eng)))
  eng.close()
  assert np.isfinite(out[0][0][0])
  assert out[0][0] == out[1][0]
  assert _same(out[0][1], out[1][1])


# ------------------------------------------------------------ 4. determinism, the split form

@pytest.mark.parametrize("mode", ["f32", "f16x3"])
def test_deterministic_and_split_apply_equals_step(built_lib, mode):
  cfg, params, feed, lo, lp = _case("A", True, seed=3)
  fd = dict(feed, train_obs_lengths=lo, train_pred_lengths=lp)
  outs = []
  for how in ("step", "split", "split"):
    eng = _engine(built_lib, cfg, params, mode)
    if how == "step":
      eng.train_step(fd)
    else:
      eng.train_forward_backward(fd)
      eng.train_apply(1.0)
    outs.append((_grads(eng), _params(eng)))
    eng.close()
  for other in outs[1:]:
    assert _same(outs[0][0], other[0])
    assert _same(outs[0][1], other[1])
  assert not _same(outs[0][1], {n: params[n] for n in outs[0][1]})     # the step moved them


# ------------------------------------------------------------ 5. only live rows are launched

def _plan_rows(lo, lp):
  """Rows per encoder / decoder step, from the definition of the two prefixes."""
  enc = []
  for t in range(TO):
    live = [n for n in range(N) if lp[n] > 0 and lo[n] >= TO - t]
    enc.append(1 + max(live) if live else 0)
  dec = []
  for t in range(TP):
    live = [n for n in range(N) if lp[n] > t]
    dec.append(1 + max(live) if live else 0)
  return enc, dec


def _expected_gate_rows(enc, dec, scales):
  # forward: two chains per used scale at every step.  dgrad: both decoder chains at every
  # step; the class encoder at every step (d x), the regression encoder from step 1 on (its
  # step 0 needs neither d h nor d x: no dgrad problem, as in the uniform step)
  fwd = scales * 2 * (sum(enc) + sum(dec))
  dgrad = scales * (2 * sum(dec) + sum(enc) + sum(enc[1:]))
  return fwd, dgrad


@pytest.mark.parametrize("mode", ["f32", "f16x3"])
def test_only_live_rows_are_launched(built_lib, mode):
  for case in ("B", "A"):
    cfg, params, feed, lo, lp = _case(case, True)
    scales = sum(cfg.use_grids)
    eng = _engine(built_lib, cfg, params, mode)
    eng.train_forward_backward(feed)                    # nothing set: the uniform counts
    assert eng.last_train_gate_rows() == _expected_gate_rows([N] * TO, [N] * TP, scales)
    eng.train_forward_backward(dict(feed, train_obs_lengths=lo, train_pred_lengths=lp))
    enc, dec = _plan_rows(lo, lp)
    got = eng.last_train_gate_rows()
    print("case %s %s: rows per encoder step %s, per decoder step %s -> %s" %
          (case, mode, enc, dec, got))
    assert got == _expected_gate_rows(enc, dec, scales)
    if case == "B":      # sorted: per scale and chain, sum of Lo over the live rows and sum of L
      assert sum(enc) == sum(a for a, b in zip(lo, lp) if b > 0) and sum(dec) == sum(lp)
    eng.train_forward_backward(feed)                    # a feed without the keys clears them
    assert eng.last_train_gate_rows() == _expected_gate_rows([N] * TO, [N] * TP, scales)
    eng.close()


# ------------------------------------------------------------ 6. training's alone

def test_setting_is_read_by_training_alone(built_lib):
  cfg, params, feed, lo, lp = _case("A", True)
  ref = _engine(built_lib, cfg, params, "f16x3")        # never had lengths
  ref_losses = ref.train_step(feed)
  ref_params = _params(ref)
  ref.close()
  eng = _engine(built_lib, cfg, params, "f16x3")
  cls0, reg0 = eng.forward_greedy(feed)
  eng.set_train_lengths(lo, lp)
  cls1, reg1 = eng.forward_greedy(feed)
  for s, use in enumerate(cfg.use_grids):
    if use:
      assert np.array_equal(cls0[s].view(np.uint32), cls1[s].view(np.uint32))
      assert np.array_equal(reg0[s].view(np.uint32), reg1[s].view(np.uint32))
  eng.set_train_lengths(None, None)
  assert eng.train_step(feed) == ref_losses
  assert _same(_params(eng), ref_params)
  eng.close()


# ------------------------------------------------------------ 7. three optimiser steps

def test_three_steps_follow_the_composition(built_lib):
  """test_train_steps_match_oracle's bars: losses 2e-4 relative, parameters within 5e-3 of
  the update, the first Adadelta slot to 5e-3."""
  cfg, params, _, lo, lp = _case("A", True, seed=2)
  cfg.train_num_examples = 5      # decay_steps = 2 -> the staircase LR moves at step 2
  eng = _engine(built_lib, cfg, params, "f16x3")
  p, st = dict(params), oracle.adadelta_init(params)
  feeds = [synth.make_feed(cfg, seed=synth.SEED_BASE + 70 + i) for i in range(3)]
  eng.set_train_lengths(lo, lp)                         # sticky over the three feeds
  for step, fd in enumerate(feeds):
    loss, _, _ = eng.train_step(fd)
    oloss, _, _, p, st, _ = tlo.train_step(p, st, step, cfg, fd, lo, lp)
    print("step %d loss gpu %.6f composition %.6f" % (step, loss, oloss))
    assert np.isfinite(loss)
    assert abs(loss - oloss) < 2e-4 * max(1.0, abs(oloss))
    assert eng.global_step == step + 1
  worst = 0.0
  for name, _ in eng.param_specs():
    d = np.abs(eng.get_param(name) - p[name]).max()
    upd = np.abs(p[name] - params[name]).max()
    worst = max(worst, d / max(upd, 1e-12))
    print("%-78s |gpu-composition| %.2e of update %.2e" % (name, d, upd))
    assert _rel(eng.get_opt_slot(name, 0), st[name][0]) < 5e-3
  assert worst < 5e-3
  eng.close()


# ------------------------------------------------------------ 8. refusals and range errors

@pytest.mark.parametrize("call", ["train_step", "train_forward_backward"])
def test_range_errors_name_the_call_the_row_and_the_value(built_lib, call):
  cfg, params, feed, lo, lp = _case("A", True)
  eng = _engine(built_lib, cfg, params)
  bad = [(dict(train_obs_lengths=[4, 2, 0, 1, 3]), r"observation length of row 2 is 0"),
         (dict(train_obs_lengths=[4, 2, 4, 5, 3]), r"observation length of row 3 is 5"),
         (dict(train_pred_lengths=[3, -1, 0, 2, 1]), r"prediction length of row 1 is -1"),
         (dict(train_pred_lengths=[3, 3, 0, 2, 4]), r"prediction length of row 4 is 4"),
         (dict(train_obs_lengths=lo, train_pred_lengths=[0] * N),
          r"every training prediction length is 0")]
  for keys, reason in bad:
    with pytest.raises(built_lib.MvError, match=r"mv_%s: .*%s" % (call, reason)):
      getattr(eng, call)(dict(feed, **keys))
  with pytest.raises(built_lib.MvError, match="train_pred_lengths: 4 values for batch_size 5"):
    getattr(eng, call)(dict(feed, train_pred_lengths=[1, 1, 1, 1]))
  # and the engine still trains
  getattr(eng, call)(dict(feed, train_obs_lengths=lo, train_pred_lengths=lp))
  eng.close()


def test_unsupported_models_and_modes_are_refused_at_the_step(built_lib):
  lengths = dict(train_obs_lengths=CASES["A"][1], train_pred_lengths=CASES["A"][2])

  def refused(cfg_over, reason, mode="f32", before=None):
    cfg, params, feed, _, _ = _case("A", True, **cfg_over)
    eng = _engine(built_lib, cfg, params, mode)
    if before:
      before(eng, feed)
    with pytest.raises(built_lib.MvError, match=r"mv_train_step: .*" + reason):
      eng.train_step(dict(feed, **lengths))
    eng.close()

  refused({}, "bf16 compute mode", mode="bf16")
  refused(dict(use_single_decoder=True), "use_single_decoder")
  refused(dict(use_scene_enc=False), "without the scene encoder")
  refused(dict(convlstm_kernel=5), "convlstm_kernel 5")

  def mixup(eng, feed):
    eng.upload(feed)
    eng.set_label_mixup(feed["grid_obs_labels"], feed["grid_pred_labels"], 0.7)
  refused({}, "label mixup", before=mixup)

  # the attacks: refused while training lengths are set at all
  cfg, params, feed, lo, lp = _case("A", True)
  eng = _engine(built_lib, cfg, params)
  eng.upload(feed)
  eng.set_train_lengths(lo, lp)
  with pytest.raises(built_lib.MvError, match=r"mv_attack_begin: .*mv_set_train_lengths"):
    eng.attack_begin()
  with pytest.raises(built_lib.MvError, match=r"mv_attack_step: .*mv_set_train_lengths"):
    eng.attack_step(0.1, 0.05)
  eng.set_train_lengths(None, None)
  eng.attack_begin()                                    # cleared: the attack pass opens
  with pytest.raises(built_lib.MvError,
                     match=r"mv_train_forward_backward: .*inside an attack pass"):
    eng.train_forward_backward(dict(feed, **lengths))
  eng.attack_end()
  eng.close()
