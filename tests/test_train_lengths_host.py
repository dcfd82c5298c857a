# coding=utf-8
"""CPU: the layers around per-row TRAINING lengths (include/multiverse_hip.h
mv_set_train_lengths) -- the two C-ABI symbols, the reference composition
(tests/train_lengths_oracle.py) against the whole-batch oracle, the row order
(`multifuture.order_train_rows`) and the feed-key rule of `Engine._targets`."""
import ctypes
import itertools
import os
import re

import numpy as np
import torch

from multiverse_amd import multifuture as mf, pred_models, synth
from oracle import multiverse_oracle as oracle

import train_lengths_oracle as tlo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = {"mv_set_train_lengths": ["mv_handle h", "const int32_t* obs_lengths",
                                "const int32_t* pred_lengths"],
       "mv_last_train_gate_rows": ["mv_handle h", "int64_t* forward_rows",
                                   "int64_t* dgrad_rows"]}


def test_library_exports_the_train_length_entry_points(built_lib):
  text = open(os.path.join(ROOT, "include", "multiverse_hip.h")).read()
  text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
  protos = dict(re.findall(r"\bint\s+(mv_\w+)\s*\(([^;{]*?)\)\s*;", text))
  raw = ctypes.CDLL(built_lib.LIB_PATH)
  lib = built_lib.load()
  for name, want in NEW.items():
    assert hasattr(raw, name), "libmultiverse_hip.so does not export %s" % name
    assert name in built_lib.EXPORTED_SYMBOLS
    assert [" ".join(p.split()) for p in protos[name].split(",")] == want
    fn = getattr(lib, name)
    assert len(fn.argtypes) == len(want)
  assert lib.mv_set_train_lengths.argtypes[1]._type_ is ctypes.c_int32
  assert lib.mv_set_train_lengths.argtypes[2]._type_ is ctypes.c_int32
  assert lib.mv_last_train_gate_rows.argtypes[1]._type_ is ctypes.c_int64
  assert lib.mv_last_train_gate_rows.argtypes[2]._type_ is ctypes.c_int64
  assert lib.mv_abi_version() == 5              # new symbols only
  # a NULL handle is an error code, not a crash
  assert lib.mv_set_train_lengths(None, None, None) != 0
  assert lib.mv_last_train_gate_rows(None, None, None) != 0


# ------------------------------------------------------------ the composition

def _rel(a, b):
  a = np.asarray(a, dtype=np.float64)
  b = np.asarray(b, dtype=np.float64)
  return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _small_case(N):
  # one coarse scale, short tracks: ~1 s of fp64 autograd per run
  cfg = synth.default_config(batch_size=N, use_grids=(0, 1), is_train=True, obs_len=3,
                             pred_len=2)
  params = synth.make_params(cfg, seed=synth.SEED_BASE + 3, recurrent_gain=2.0, bias_scale=0.1)
  feed = synth.make_feed(cfg, seed=synth.SEED_BASE + 53)
  return cfg, params, feed


def test_composition_reproduces_the_uniform_oracle():
  """ONE group (every row full length), and a uniform batch split into two groups by giving
  the composition the rows in two calls' worth of groups, against oracle.loss_and_grads of the
  whole batch in fp64: relative 1e-12 (measured 0 and 4e-15)."""
  cfg, params, feed = _small_case(4)
  whole = oracle.loss_and_grads(params, cfg, feed, dtype=torch.float64)
  # one group
  one = tlo.loss_and_grads(params, cfg, feed, [3] * 4, [2] * 4, dtype=torch.float64)
  # two groups of the SAME lengths: rows {0, 2} and {1, 3} (the grouping is by pair, so the
  # split goes through the group runner directly)
  pgl, grads = None, None
  for rows in ([0, 2], [1, 3]):
    sub, sfeed = tlo.slice_feed(cfg, feed, rows, 3, 2)
    sub.grid_loss_weight = cfg.grid_loss_weight * 0.5
    sub.grid_reg_loss_weight = cfg.grid_reg_loss_weight * 0.5
    _, _, gp, gg = oracle.loss_and_grads(params, sub, sfeed, dtype=torch.float64)
    pgl = gp if pgl is None else [a + b for a, b in zip(pgl, gp)]
    grads = gg if grads is None else {n: grads[n] + gg[n] for n in gg}
  wd_loss = 0.0
  for n in sorted(params):
    if n.endswith("/W"):
      w = params[n].astype(np.float64)
      grads[n] = grads[n] + cfg.wd * w
      wd_loss += cfg.wd * 0.5 * (w * w).sum()
  two = (sum(pgl) + wd_loss, wd_loss, pgl, grads)
  for what, got in (("one group", one), ("two groups", two)):
    worst = max(_rel(got[3][n], whole[3][n]) for n in whole[3])
    print("%s: loss %.15g / %.15g, worst gradient rel %.2e" % (what, got[0], whole[0], worst))
    assert abs(got[0] - whole[0]) <= 1e-12 * abs(whole[0])
    assert abs(got[1] - whole[1]) <= 1e-12 * abs(whole[1])
    assert np.allclose(got[2], whole[2], rtol=1e-12, atol=0)
    assert worst < 1e-12


def test_slicer_takes_right_aligned_observations_and_left_aligned_targets():
  cfg, _, feed = _small_case(3)
  sub, sf = tlo.slice_feed(cfg, feed, [2, 0], 2, 1)
  assert (sub.batch_size, sub.obs_len, sub.pred_len, sub.wd) == (2, 2, 1, 0.0)
  assert sf["pred_length"] == 1
  assert (sf["obs_scene"] == np.asarray(feed["obs_scene"])[[2, 0]][:, 1:]).all()
  lab = np.asarray(feed["grid_obs_labels"][1])
  assert (sf["grid_obs_labels"][1] == lab[[2, 0]][:, 1:]).all()
  reg = np.asarray(feed["grid_pred_regress"][1])
  assert (sf["grid_pred_regress"][1] == reg[[2, 0]][:, :1]).all()
  assert cfg.batch_size == 3 and cfg.wd != 0.0      # the caller's config is untouched
  assert tlo.groups_of([3, 2, 3, 1], [2, 2, 0, 2]) == {(3, 2): [0], (2, 2): [1], (1, 2): [3]}


# ------------------------------------------------------------ the row order

def _prefix_rows(lo, lp, obs_len):
  """(encoder, decoder) rows of one chain, from the definition of the two prefixes."""
  enc = 0
  for t in range(obs_len):
    live = [n for n in range(len(lo)) if lp[n] > 0 and lo[n] >= obs_len - t]
    enc += 1 + max(live) if live else 0
  dec = 0
  for t in range(max(lp) if lp else 0):
    dec += 1 + max(n for n in range(len(lp)) if lp[n] > t)
  return enc, dec


def test_order_train_rows_against_a_brute_force_sort():
  rng = np.random.default_rng(7)
  for trial in range(40):
    n = int(rng.integers(1, 9))
    obs_len, pred_len = 5, 4
    lo = [int(v) for v in rng.integers(1, obs_len + 1, n)]
    lp = [int(v) for v in rng.integers(0, pred_len + 1, n)]
    plan = mf.order_train_rows(lo, lp, obs_len=obs_len)
    # brute force: the permutation whose key sequence is the sorted one, stable by index
    keys = [(-lp[i], -lo[i], i) for i in range(n)]
    best = min(itertools.permutations(range(n)), key=lambda p: [keys[i] for i in p]) \
        if n <= 6 else tuple(sorted(range(n), key=lambda i: keys[i]))
    assert tuple(plan.order) == tuple(best)
    slo, slp = [lo[i] for i in plan.order], [lp[i] for i in plan.order]
    assert (plan.enc_rows, plan.dec_rows) == _prefix_rows(slo, slp, obs_len)
    assert (plan.enc_rows_unsorted, plan.dec_rows_unsorted) == _prefix_rows(lo, lp, obs_len)
    # sorted: the decoders launch no finished and no padding row; the encoders launch an
    # unstarted row only in front of a row of the same run with a longer history
    assert plan.dec_rows == sum(lp)
    assert plan.enc_rows >= sum(a for a, b in zip(lo, lp) if b > 0)
    if all(a >= b for a, b in zip(slo, slo[1:])):
      assert plan.enc_rows == sum(a for a, b in zip(lo, lp) if b > 0)
    assert plan.dec_rows <= plan.dec_rows_unsorted


# ------------------------------------------------------------ the feed keys

class _StubLib(object):
  def __init__(self):
    self.calls = []

  def mv_set_train_lengths(self, handle, obs, pred):
    def arr(p, n=3):
      return None if not p else [p[i] for i in range(n)]
    self.calls.append((arr(obs), arr(pred)))
    return 0


def _stub_engine(built_lib):
  cfg = synth.default_config(batch_size=3, use_grids=(0, 1), is_train=True, obs_len=3,
                             pred_len=2)
  eng = object.__new__(built_lib.Engine)
  eng.cfg, eng.lib, eng.handle = cfg, _StubLib(), None
  return eng, cfg, synth.make_feed(cfg, seed=synth.SEED_BASE + 1)


def test_feed_keys_are_set_kept_and_cleared(built_lib):
  eng, cfg, feed = _stub_engine(built_lib)
  eng._targets(feed)                                   # nothing set: nothing to clear
  assert eng.lib.calls == []
  eng._targets(dict(feed, train_obs_lengths=[3, 1, 2], train_pred_lengths=[2, 0, 1]))
  assert eng.lib.calls == [([3, 1, 2], [2, 0, 1])]
  eng._targets(dict(feed, train_pred_lengths=np.array([1, 2, 2])))   # one side: the other uniform
  assert eng.lib.calls[-1] == (None, [1, 2, 2])
  eng._targets(feed)                                   # a feed without them clears
  assert eng.lib.calls[-1] == (None, None) and len(eng.lib.calls) == 3
  eng._targets(feed)                                   # ... once
  assert len(eng.lib.calls) == 3
  # set through the call: a feed without the keys leaves it alone (sticky until cleared)
  eng.set_train_lengths([1, 1, 1], None)
  eng._targets(feed)
  assert eng.lib.calls[-1] == ([1, 1, 1], None) and len(eng.lib.calls) == 4
  for key in ("train_obs_lengths", "train_pred_lengths"):
    try:
      eng._targets(dict(feed, **{key: [1, 1]}))
    except built_lib.MvError as err:
      assert key in str(err) and "batch_size 3" in str(err)
    else:
      raise AssertionError("a length array of the wrong size must raise MvError")
  assert len(eng.lib.calls) == 4


def test_trainer_mirror_hands_the_keys_through():
  class _Batch(object):
    pass
  data, feed = {"train_obs_lengths": [2, 1], "train_pred_lengths": np.array([1, 0])}, {}
  pred_models._hand_train_lengths(data, feed, True)
  assert feed["train_obs_lengths"] is data["train_obs_lengths"]
  assert feed["train_pred_lengths"] is data["train_pred_lengths"]
  feed = {}
  pred_models._hand_train_lengths(data, feed, False)     # inference feeds: not handed
  pred_models._hand_train_lengths({}, feed, True)
  assert feed == {}
