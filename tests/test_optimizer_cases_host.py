# coding=utf-8
"""Host half of the optimizer-apply parity tests (tests/optimizer_cases.py; the GPU half is
test_gpu_optimizer_apply.py).

1. The bound sees what it is for.  The fp64 reference and the fp32 oracle of optimizer_cases run
   on 70 001 elements; a float32 restatement of the kernels (device_model_run) must pass the
   acceptance rule the GPU is held to, and the same model made wrong in each of four ways -- Adam's
   epsilon 1e-7 instead of 1e-8, the clip before the scale, a beta power one step stale, the two
   slots swapped -- must fail it.  The clip that drops a NaN (fminf(fmaxf())) fails the NaN corner.
2. Saver.save -> tf_checkpoint.load_checkpoint(skip_optimizer_slots=False) -> Saver.restore round-
   trips the slot names of OPT_SLOT_NAMES, Adam's beta powers and global_step for a fake engine,
   and restore creates the training state of a model that has none yet.
"""
import argparse

import numpy as np
import pytest

from multiverse_amd import pred_utils, tf_checkpoint

import optimizer_cases as oc

SPECS = [("person_pred/probe/W", (70001,))]
_RUNS = {}


def _case(optimizer, scale, clip):
  """(cfg, inputs, ref64, per-step paths, per-step fp32 oracle constants), computed once."""
  key = (optimizer, scale, clip)
  if key not in _RUNS:
    cfg = oc.optimizer_config(oc.base_config(), optimizer, clip=clip)
    inputs = oc.make_inputs(SPECS, optimizer)
    powers = oc.ADAM_START_POWERS if optimizer == "adam" else None
    ref64 = oc.reference_run(cfg, inputs, scale, 3, np.float64, powers=powers)
    ref32 = oc.reference_run(cfg, inputs, scale, 3, np.float32, powers=powers)
    path = oc.paths(inputs, ref64)
    nsl = oc.NUM_SLOTS[optimizer]
    c32 = [oc.error_constants(ref32[k]["params"], ref32[k]["slots"], ref64[k], path[k], nsl)
           for k in range(3)]
    _RUNS[key] = (cfg, inputs, powers, ref64, path, c32)
  return _RUNS[key]


def _model_constants(optimizer, scale, clip, fault=None):
  cfg, inputs, powers, ref64, path, c32 = _case(optimizer, scale, clip)
  got = oc.device_model_run(cfg, inputs, scale, 3, powers=powers, fault=fault)
  nsl = oc.NUM_SLOTS[optimizer]
  cs = [oc.error_constants(got[k]["params"], got[k]["slots"], ref64[k], path[k], nsl)
        for k in range(3)]
  return cs, c32, got


@pytest.mark.parametrize("scale,clip", oc.SCALE_CLIP)
@pytest.mark.parametrize("optimizer", oc.OPTIMIZERS)
def test_right_model_passes_the_bound(optimizer, scale, clip):
  cs, c32, got = _model_constants(optimizer, scale, clip)
  for k in range(3):
    print("%-8s scale %.3g clip %s apply %d: fp32 oracle c_p %.2f c_s %.2f | kernel model "
          "c_p %.2f c_s %.2f" % (optimizer, scale, clip, k, c32[k][0], c32[k][1], cs[k][0],
                                 cs[k][1]))
    assert c32[k][0] <= oc.ORACLE_CEILING and c32[k][1] <= oc.ORACLE_CEILING
    assert oc.within_bounds(cs[k], c32[k]), (k, cs[k], c32[k])
    assert got[k]["step"] == k + 1


def _applies(fault, optimizer, scale, clip):
  if fault in ("adam_eps_1e-7", "stale_beta_power"):
    return optimizer == "adam"
  if fault == "clip_before_scale":
    return clip is not None and scale != 1.0
  return oc.NUM_SLOTS[optimizer] == 2          # slots_swapped


@pytest.mark.parametrize("fault", oc.FAULTS)
def test_each_wrong_model_fails_the_bound(fault):
  tried = 0
  for optimizer in oc.OPTIMIZERS:
    for scale, clip in oc.SCALE_CLIP:
      if not _applies(fault, optimizer, scale, clip):
        continue
      cs, c32, _ = _model_constants(optimizer, scale, clip, fault=fault)
      passed = [oc.within_bounds(cs[k], c32[k]) for k in range(3)]
      print("%-18s %-8s scale %.3g clip %s: c_p %s c_s %s" % (
          fault, optimizer, scale, clip, ["%.3g" % c[0] for c in cs], ["%.3g" % c[1] for c in cs]))
      assert not all(passed), (fault, optimizer, scale, clip)
      tried += 1
  assert tried > 0


def test_stale_beta_power_also_fails_the_scalar_check():
  """The powers the engine reports are compared bit for bit with float32 products."""
  b1, b2 = oc.ADAM_START_POWERS
  for _ in range(3):
    b1, b2 = oc._powers_after((b1, b2))      # pylint: disable=protected-access
  assert b1 == np.float32(0.9 ** 5) * np.float32(0.9) * np.float32(0.9) * np.float32(0.9)
  assert b1 != oc._powers_after((b1, b2))[0]  # pylint: disable=protected-access


@pytest.mark.parametrize("optimizer", oc.OPTIMIZERS)
def test_nan_dropping_clip_fails_the_nan_corner(optimizer):
  """np.clip (oracle.train_step) keeps a NaN gradient: the parameter and the slots become NaN.
  The comparison clip of the kernels does the same; fminf(fmaxf(g, -clip), clip) applied -clip."""
  name = "person_pred/probe/b"
  inputs = oc.corner_inputs(optimizer, name, 64, "boundary")
  scale, clip, vals = oc.CORNER_CASES["boundary"]
  cfg = oc.optimizer_config(oc.base_config(), optimizer, clip=clip, init_lr=oc.CORNER_LR,
                            learning_rate_decay=None)
  ref = oc.reference_run(cfg, inputs, scale, 1, np.float64)[0]
  at = [i for i, v in enumerate(vals) if np.isnan(v)]
  assert at and np.isnan(ref["params"][name][at]).all()
  assert all(np.isnan(s[at]).all() for s in ref["slots"][name])
  keep = oc.device_model_run(cfg, inputs, scale, 1)[0]
  drop = oc.device_model_run(cfg, inputs, scale, 1, nan_dropping_clip=True)[0]
  assert np.isnan(keep["params"][name][at]).all()
  assert all(np.isnan(s[at]).all() for s in keep["slots"][name])
  assert np.isfinite(drop["params"][name][at]).all()
  rest = np.ones(64, bool)
  rest[at] = False
  assert np.isfinite(keep["params"][name][rest]).all()


# ---------------------------------------------------------------- Saver round trip
class _FakeEngine(object):
  """The optimizer-state surface of _lib.Engine, on the host."""

  def __init__(self, specs, trained=True):
    self.specs = specs
    self.trained = trained
    self.slots = {(n, i): np.zeros(s, "f4") for n, s in specs for i in (0, 1)}
    self.scalars = (0.9, 0.999)
    self._step = 0
    self.inits = []

  def _need(self):
    if not self.trained:
      from multiverse_amd import _lib
      raise _lib.MvError("mv_train_init has not been called")

  def param_specs(self):
    return list(self.specs)

  def train_init(self, cfg=None, world=None):
    self.inits.append((cfg, world))
    self.trained = True

  def get_opt_slot(self, name, slot):
    self._need()
    return self.slots[(name, slot)].copy()

  def set_opt_slot(self, name, slot, value):
    self._need()
    assert value.shape == self.slots[(name, slot)].shape
    self.slots[(name, slot)] = np.asarray(value, "f4").copy()

  def opt_scalars(self):
    self._need()
    return self.scalars

  def set_opt_scalars(self, b1p, b2p):
    self._need()
    self.scalars = (float(b1p), float(b2p))

  @property
  def global_step(self):
    self._need()
    return self._step

  @global_step.setter
  def global_step(self, step):
    self._need()
    self._step = int(step)


class _FakeModel(object):
  def __init__(self, optimizer, specs, trained=True, is_train=True):
    self.config = argparse.Namespace(optimizer=optimizer, is_train=is_train)
    self.engine = _FakeEngine(specs, trained)
    self.params = {n: np.zeros(s, "f4") for n, s in specs}

  def get_params(self):
    return {n: v.copy() for n, v in self.params.items()}

  def load_params(self, params):
    assert sorted(params) == sorted(self.params)
    self.params = {n: np.asarray(v, "f4").copy() for n, v in params.items()}


@pytest.mark.parametrize("optimizer", oc.OPTIMIZERS)
def test_saver_round_trips_slots_powers_and_step(tmp_path, optimizer):
  specs = [("person_pred/scene_conv1/W", (3, 3, 11, 4)), ("person_pred/scene_conv1/b", (4,))]
  rng = np.random.default_rng(3)
  src = _FakeModel(optimizer, specs)
  nsl = oc.NUM_SLOTS[optimizer]
  for n, s in specs:
    src.params[n] = rng.normal(0, 1, s).astype("f4")
    for i in range(nsl):
      src.engine.slots[(n, i)] = rng.normal(0, 1, s).astype("f4")
  src.engine.scalars = (float(np.float32(0.9 ** 7)), float(np.float32(0.999 ** 7)))
  src.engine.global_step = 12345
  path = pred_utils.Saver().save(src, str(tmp_path / "save"), global_step=12345)
  allv = tf_checkpoint.load_checkpoint(path, skip_optimizer_slots=False)
  suffixes = pred_utils.OPT_SLOT_NAMES[optimizer]
  assert len(suffixes) == nsl
  want = set(n for n, _ in specs) | {"global_step"}
  want |= {n + "/" + sfx for n, _ in specs for sfx in suffixes}
  if optimizer == "adam":
    want |= {"beta1_power", "beta2_power"}
  assert set(allv) == want
  assert int(allv["global_step"]) == 12345
  for n, _ in specs:
    assert (allv[n] == src.params[n]).all()
    for i, sfx in enumerate(suffixes):
      assert allv[n + "/" + sfx].dtype == np.float32
      assert (allv[n + "/" + sfx] == src.engine.slots[(n, i)]).all()
  # the weights-only reader drops all of it
  assert set(tf_checkpoint.load_checkpoint(path)) == set(n for n, _ in specs)
  # restore into a model whose engine has no training state yet: restore creates it
  dst = _FakeModel(optimizer, specs, trained=False)
  pred_utils.Saver().restore(dst, path)
  assert len(dst.engine.inits) == 1 and dst.engine.inits[0][0] is dst.config
  assert dst.engine.global_step == 12345
  for n, _ in specs:
    assert (dst.params[n] == src.params[n]).all()
    for i in range(nsl):
      assert (dst.engine.slots[(n, i)] == src.engine.slots[(n, i)]).all()
  if optimizer == "adam":
    assert dst.engine.scalars == src.engine.scalars
  # weights only: an inference model, and with_optimizer=False
  inf = _FakeModel(optimizer, specs, trained=False, is_train=False)
  pred_utils.Saver().restore(inf, path)
  assert not inf.engine.inits and not inf.engine.trained
  assert (inf.params[specs[0][0]] == src.params[specs[0][0]]).all()
  cold = _FakeModel(optimizer, specs, trained=False)
  pred_utils.Saver().restore(cold, path, with_optimizer=False)
  assert not cold.engine.inits
