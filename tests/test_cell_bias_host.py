# coding=utf-8
"""CPU: the cell costs (mv_set_cell_bias) around the engine -- the new symbols and their
prototypes, `multifuture.cell_bias_from_scene` against a brute-force pixel loop, the "cell_bias"
key of `inference_feed`, the script's flag and its refusals -- and the restatement
(tests/cell_bias_oracle.py) against the restatements it stands on: a zero bias is the mask
restatement's result bit for bit, and a bias of -1e30 outside a set A with no mask gives the
masked restatement's ids, logprobs and proposal log-probabilities bit for bit."""
import argparse
import ctypes
import inspect
import os
import re
from glob import glob

import numpy as np
import pytest

from multiverse_amd import cli, multifuture as mf

import cell_bias_oracle as cb
import cell_mask_oracle as cm
import mf_fixture
from test_cell_mask_host import _mf_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = (("mv_op_beam_step", 3), ("mv_op_sbs_step", 5), ("mv_op_sample_step", 2))


# ------------------------------------------------------------ symbols

def test_library_exports_the_new_symbols(built_lib):
  text = open(os.path.join(ROOT, "include", "multiverse_hip.h")).read()
  text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
  protos = dict(re.findall(r"\bint\s+(mv_\w+)\s*\(([^;{]*?)\)\s*;", text))
  raw = ctypes.CDLL(built_lib.LIB_PATH)
  lib = built_lib.load()
  for name in ("mv_set_cell_bias", "mv_op_beam_step_biased", "mv_op_sbs_step_biased",
               "mv_op_sample_step_biased"):
    assert hasattr(raw, name), "libmultiverse_hip.so does not export " + name
    assert name in built_lib.EXPORTED_SYMBOLS and name in protos
  norm = lambda name: [" ".join(p.split()) for p in protos[name].split(",")]
  assert norm("mv_set_cell_bias") == ["mv_handle h", "const float* bias", "int32_t Tm"]
  assert lib.mv_set_cell_bias.argtypes[1:] == [ctypes.POINTER(ctypes.c_float), ctypes.c_int32]
  # each biased op is its masked op plus one pointer, directly behind `allowed`
  for name, at in OPS:
    want = norm(name + "_masked")
    assert want[at] == "const uint8_t* allowed"
    want.insert(at + 1, "const float* bias")
    assert norm(name + "_biased") == want, name
    masked, biased = getattr(lib, name + "_masked").argtypes, getattr(lib, name + "_biased").argtypes
    assert list(biased) == list(masked[:at + 1]) + [ctypes.POINTER(ctypes.c_float)] + \
        list(masked[at + 1:]), name
  assert lib.mv_abi_version() == 5 == built_lib.MV_ABI_VERSION    # new symbols only
  assert lib.mv_set_cell_bias(None, None, 1) != 0                 # NULL handle: an error code
  assert ctypes.sizeof(built_lib.mv_config) == 28 * 4             # the structs keep their layout
  assert hasattr(built_lib.Engine, "set_cell_bias")
  for op in (built_lib.op_beam_step, built_lib.op_sbs_step, built_lib.op_sample_step):
    assert inspect.signature(op).parameters["bias"].default is None


# ------------------------------------------------------------ cell_bias_from_scene

def _brute_force(onehot, h, w, costs):
  H, W = onehot.shape[:2]
  total = np.zeros((h, w))
  count = np.zeros((h, w, onehot.shape[2]))
  for i in range(H):
    for j in range(W):
      gi, gj = (i * h) // H, (j * w) // W
      total[gi, gj] += 1
      for c in range(onehot.shape[2]):
        if onehot[i, j, c]:
          count[gi, gj, c] += 1
  out = np.zeros((h, w))
  for gi in range(h):
    for gj in range(w):
      for c, cost in costs:
        out[gi, gj] += cost * count[gi, gj, c] / total[gi, gj]
  return out


@pytest.mark.parametrize("H,W,grids,use", [(36, 64, [(18, 32), (9, 16)], (1, 0)),
                                           (36, 64, [(18, 32), (9, 16)], (0, 1)),
                                           (72, 36, [(36, 18), (18, 9)], (1, 0))])
def test_cell_bias_from_scene_is_the_brute_force_loop(H, W, grids, use):
  rng = np.random.RandomState(9 + H)
  C = 11
  cls = rng.randint(0, C, size=(H, W))
  cls[: H // 3] = 4                       # a block of one costed class, a block of none
  cls[-H // 4:, : W // 2] = 0
  onehot = np.eye(C, dtype=np.uint8)[cls]
  args = argparse.Namespace(scene_grids=grids, use_grids=[bool(u) for u in use])
  h, w = grids[list(use).index(1)]
  for costs in ([(4, -2.0)], [(1, -2.0), (4, 0.5), (7, 3.25)]):
    got = mf.cell_bias_from_scene(args, onehot, costs)
    assert got.shape == (h, w) and got.dtype == np.float32
    want = _brute_force(onehot, h, w, costs)
    assert np.abs(got - want).max() <= 1e-6 * max(1.0, np.abs(want).max()), costs
    assert np.array_equal(got, mf.cell_bias_from_scene(args, onehot, dict(costs)))
    assert (got[: h // 3 - 1] == np.float32(dict(costs)[4])).all()   # the pure block: its cost
  assert (mf.cell_bias_from_scene(args, onehot, [(0, 0.0)]) == 0).all()
  # the pixel-to-cell map is cell_mask_from_scene's: a cell costs something iff it is allowed
  b = mf.cell_bias_from_scene(args, onehot, [(4, 1.0)])
  assert np.array_equal(b > 0, mf.cell_mask_from_scene(args, onehot, [4], 0.0))


# ------------------------------------------------------------ inference_feed

def test_inference_feed_carries_the_bias(tmp_path):
  ds = mf_fixture.make_dataset(str(tmp_path / "fp"), n_traj=4)
  files = sorted(glob(os.path.join(ds["traj_path"], "*.txt")))
  ids = [os.path.splitext(os.path.basename(f))[0] for f in files]
  gt = mf.load_gt(ds["multifuture_path"], ids)
  plain_args = _mf_args(ds)
  inputs = mf.get_inputs(plain_args, files, gt)
  idxs = [0, 2]
  T_pred = max(inputs["max_pred_lengths"][i] for i in idxs)
  plain, _ = mf.inference_feed(inputs, plain_args, idxs, batch_size=3, pred_length=T_pred)
  assert "cell_bias" not in plain
  costs = [(1, -2.0), (4, 0.5)]
  args = _mf_args(ds, class_costs=costs)
  feed, n_real = mf.inference_feed(inputs, args, idxs, batch_size=3, pred_length=T_pred)
  assert n_real == 2 and feed["cell_bias"].shape == (3, 144)
  assert feed["cell_bias"].dtype == np.float32 and "cell_mask" not in feed
  for r, i in enumerate(idxs):
    last = inputs["scene_feats"][int(inputs["obs_scene"][i][-1][0])]       # the LAST frame
    want = mf.cell_bias_from_scene(args, last, costs).reshape(-1)
    assert np.array_equal(feed["cell_bias"][r], want) and (want != 0).any()
  assert (feed["cell_bias"][2] == 0).all()                                  # the padding row
  for k in plain:                                                           # all else unchanged
    a, b = plain[k], feed[k]
    if isinstance(a, list):
      assert all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b)), k
    else:
      assert np.array_equal(a, b), k
  both = _mf_args(ds, class_costs=costs, allowed_classes=[1, 2, 3], allowed_min_share=0.25)
  feed2, _ = mf.inference_feed(inputs, both, idxs, batch_size=3, pred_length=T_pred)
  assert np.array_equal(feed2["cell_bias"], feed["cell_bias"]) and "cell_mask" in feed2


# ------------------------------------------------------------ flags

def test_script_flag_and_its_refusals():
  flags = {f: (t, d) for f, t, d in cli._MF_FLAGS}                # pylint: disable=protected-access
  assert flags["--class_costs"] == (str, None)
  p = cli.multifuture_inference_parser()
  base = ["traj", "mfut", "model", "out.p"]
  off = p.parse_args(base)
  assert off.class_costs is None
  cli.parse_class_costs(off)
  assert off.class_costs is None
  a = p.parse_args(base + ["--class_costs", "1:-2.0,4:0.5", "--allowed_classes", "1,4", "--sample"])
  cli.parse_allowed_classes(a)
  cli.parse_class_costs(a)
  assert a.class_costs == [(1, -2.0), (4, 0.5)] and a.allowed_classes == [1, 4]
  for extra, word in ((["--class_costs", "1:-2", "--greedy"], "--greedy"),
                      (["--class_costs", "1:-2", "--score_gt", "s.p"], "--score_gt"),
                      (["--class_costs", "1,4"], "id:cost"),
                      (["--class_costs", "1:x"], "id:cost"),
                      (["--class_costs", "1:2:3"], "id:cost"),
                      (["--class_costs", ","], "scene_class"),
                      (["--class_costs", "11:1.0"], "scene_class"),
                      (["--class_costs=-1:1.0"], "scene_class"),
                      (["--class_costs", "1:inf"], "finite"),
                      (["--class_costs", "1:nan"], "finite"),
                      (["--class_costs", "1:1.0,1:2.0"], "twice")):
    with pytest.raises(SystemExit) as err:
      cli.multifuture_inference_main(base + extra)
    assert word in str(err.value) and "--class_costs" in str(err.value), extra


# ------------------------------------------------------------ the restatement

R, S, K = 8, 2, 70
N, B = 2, 3
LIMITS = ((0, 1.0), (8, 0.9))


def _inputs(seed):
  rng = np.random.RandomState(seed)
  logits = (4.0 * rng.randn(R, K)).astype(np.float32)
  l3 = (2.0 * rng.randn(N, B, K)).astype(np.float32)
  phi, LP, G = (-rng.rand(N, B).astype(np.float32) for _ in range(3))
  return rng, logits, l3, phi, LP, G


def test_zero_bias_is_the_mask_restatement_bit_for_bit():
  rng, logits, l3, phi, LP, G = _inputs(5)
  for allowed in (np.ones((R // S, K), dtype=np.uint8), rng.rand(R // S, K) < 0.5):
    zero = np.zeros((R // S, K), dtype=np.float32)
    for temp in (1.0, 0.7):
      for limits in LIMITS:
        a = cb.sample_step(logits, S, 1, allowed, zero, temp, 9, limits[0], limits[1],
                           dtype=np.float32)
        b = cm.sample_step(logits, S, 1, allowed, temp, 9, limits[0], limits[1], dtype=np.float32)
        for k in ("keep", "tight", "wide", "ids", "q", "lp_id", "q_id", "compared"):
          assert a[k].tobytes() == b[k].tobytes(), (temp, limits, k)
  for am in (np.ones((N, K), dtype=bool), rng.rand(N, K) < 0.5):
    zero = np.zeros((N, K), dtype=np.float32)
    for t in (0, 1):
      a = cb.sbs_step(l3, phi, LP, G, t, am, zero, 0.8, 3)
      b = cm.sbs_step(l3, phi, LP, G, t, am, 0.8, 3)
      for k in ("new_phi", "new_lp", "new_g", "ids", "parents", "q"):
        assert a[k].tobytes() == b[k].tobytes(), (t, k)
    for time in (1, 2):
      for diverse in (False, True):
        a = cb.beam_step(l3, LP, am, zero, time, diverse, 0.01, 0)
        b = cm.beam_step(l3, LP, am, time, diverse, 0.01, 0)
        for k in ("new_lp", "ids", "parents", "cand"):
          assert a[k].tobytes() == b[k].tobytes(), (time, diverse, k)
  # allowed=None is all ones
  zero = np.zeros((R // S, K), dtype=np.float32)
  a = cb.sample_step(logits, S, 1, None, zero, 0.7, 9, 8, 0.9)
  b = cb.sample_step(logits, S, 1, np.ones((R // S, K)), zero, 0.7, 9, 8, 0.9)
  assert all(a[k].tobytes() == b[k].tobytes() for k in a)
  lg = rng.randn(N, B, 2, K).astype(np.float32)
  mask = (rng.rand(N, 2, K) < 0.5).astype(np.uint8)
  for dt in (np.float32, np.float64):
    assert cb.occupancy(lg, LP, mask, np.zeros((N, 1, K)), dtype=dt).tobytes() == \
        cm.occupancy(lg, LP, mask, dtype=dt).tobytes()


def test_minus_1e30_outside_a_set_is_the_mask_restatement():
  """The float32 restatement shows it bit for bit in the ids, the model's and the proposal's
  log-probabilities of the chosen cells and the carried scores: w = l / tau - 1e30 is -1e30, whose
  e is exactly 0, so the maximum and every sum are those over A.  (The kept SET differs outside A
  with the limits off: a cell of probability exactly 0 is 'kept' and never drawn.)"""
  rng, logits, l3, phi, LP, G = _inputs(6)
  allowed = rng.rand(R // S, K) < 0.5
  veto = np.where(allowed, 0.0, -1e30).astype(np.float32)
  rows = np.repeat(allowed, S, axis=0)
  for temp in (1.0, 0.7):
    for limits in LIMITS:
      a = cb.sample_step(logits, S, 1, None, veto, temp, 9, limits[0], limits[1], dtype=np.float32)
      b = cm.sample_step(logits, S, 1, allowed, temp, 9, limits[0], limits[1], dtype=np.float32)
      for k in ("ids", "lp_id", "q_id"):
        assert a[k].tobytes() == b[k].tobytes(), (temp, limits, k)
      assert (a["keep"] & rows).tobytes() == b["keep"].tobytes()
      assert a["q"][rows].tobytes() == b["q"][rows].tobytes()
  am = rng.rand(N, K) < 0.5
  veto = np.where(am, 0.0, -1e30).astype(np.float32)
  for t in (0, 1):
    a = cb.sbs_step(l3, phi, LP, G, t, None, veto, 0.8, 3)
    b = cm.sbs_step(l3, phi, LP, G, t, am, 0.8, 3)
    for k in ("new_phi", "new_lp", "new_g", "ids", "parents"):
      assert a[k].tobytes() == b[k].tobytes(), (t, k)
  for time in (1, 2):
    for diverse in (False, True):
      a = cb.beam_step(l3, LP, None, veto, time, diverse, 0.01, 0)
      b = cm.beam_step(l3, LP, am, time, diverse, 0.01, 0)
      for k in ("new_lp", "ids", "parents"):
        assert a[k].tobytes() == b[k].tobytes(), (time, diverse, k)


def test_a_bias_moves_the_choice_and_leaves_the_model():
  rng, logits, l3, phi, LP, G = _inputs(7)
  bias = (2.0 * rng.randn(R // S, K)).astype(np.float32)
  rows = np.arange(R)
  d = cb.sample_step(logits, S, 0, None, bias, 0.7, 9, dtype=np.float64)
  plain = cm.sample_step(logits, S, 0, np.ones((R // S, K)), 0.7, 9, dtype=np.float64)
  assert (d["ids"] != plain["ids"]).any()
  assert np.allclose(np.exp(d["q"]).sum(-1), 1.0)
  lp = cm.sbs.log_softmax(logits.astype(np.float64))
  assert np.array_equal(d["lp_id"], lp[rows, d["ids"]])                     # the model's
  w = logits.astype(np.float64) / float(np.float32(0.7)) + np.repeat(bias, S, 0)
  assert np.abs(d["q"] - cm.sbs.log_softmax(w)).max() < 1e-5                # softmax of l/tau + b
  # the limits order by w, not by l: a bias that reverses the top cells keeps other cells
  rev = np.zeros((R // S, K), dtype=np.float32)
  for n in range(R // S):
    top = np.argsort(-logits[n * S])[:16]
    rev[n, top] = -2.0 * (logits[n * S, top] - logits[n * S, top[-1]])
  by_w = cb.sample_step(logits, S, 0, None, rev, 1.0, 9, 8, 1.0)["keep"]
  by_l = cm.sample_step(logits, S, 0, np.ones((R // S, K)), 1.0, 9, 8, 1.0)["keep"]
  assert (by_w.sum(-1) == 8).all() and (by_l.sum(-1) == 8).all() and (by_w != by_l).any()
  w32 = cb.proposal_w(logits, np.repeat(rev, S, 0), 1.0)
  for r in range(R):
    assert set(np.nonzero(by_w[r])[0]) == set(np.argsort(-w32[r], kind="stable")[:8])
  # three exactly equal top values of l + b share a count: kept or dropped together
  tie_l, tie_b = logits.copy(), np.zeros((R // S, K), dtype=np.float32)
  base = np.float32(np.ceil(tie_l[0].max()))
  tie_l[0, [5, 17, 40]] = base + np.array([0.5, 1.0, 1.5], dtype=np.float32)
  tie_b[0, [5, 17, 40]] = np.array([1.5, 1.0, 0.5], dtype=np.float32)
  assert len(set(cb.proposal_w(tie_l, np.repeat(tie_b, S, 0), 1.0)[0, [5, 17, 40]])) == 1
  for top_k, n_kept in ((1, 3), (2, 3), (3, 3), (4, 4)):
    keep = cb.sample_step(tie_l, S, 0, None, tie_b, 1.0, 9, top_k, 1.0)["keep"][0]
    assert keep[[5, 17, 40]].all() and keep.sum() == n_kept, top_k
  # beam: the candidate is (prev + lp) + b, and rank 0 carries no penalty
  st = cb.beam_step(l3, LP, None, bias[:N], 2, True, 0.01, 0)
  best = ((LP[..., None] + cm.sbs.log_softmax(l3)) + bias[:N, None, :]).astype(np.float32).max(-1)
  assert np.array_equal(st["cand"].max(-1), best)
  # occupancy: the softmax of l + b
  lg = rng.randn(N, B, 2, K).astype(np.float32)
  occ = cb.occupancy(lg, LP, None, bias[:N, None, :])
  assert np.abs(occ.sum(-1) - 1).max() < 1e-12
  assert not np.allclose(occ, cm.occupancy(lg, LP, np.ones((N, 1, K))))
