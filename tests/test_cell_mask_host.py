# coding=utf-8
"""CPU: the constrained decode (mv_set_cell_mask) around the engine -- the new symbols and their
prototypes, `multifuture.cell_mask_from_scene` against a brute-force loop, the "cell_mask" key and
the fallback list of `inference_feed`, the script's flags -- and the restatement
(tests/cell_mask_oracle.py) against the restatements it stands on: all allowed is their result,
bit for bit."""
import argparse
import ctypes
import math
import os
import re
from glob import glob

import numpy as np
import pytest

from multiverse_amd import cli, multifuture as mf

import cell_mask_oracle as cm
import mf_fixture
import sbs_oracle as sbs
import truncation_oracle as to

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------ symbols

def test_library_exports_the_new_symbols(built_lib):
  text = open(os.path.join(ROOT, "include", "multiverse_hip.h")).read()
  text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
  protos = dict(re.findall(r"\bint\s+(mv_\w+)\s*\(([^;{]*?)\)\s*;", text))
  raw = ctypes.CDLL(built_lib.LIB_PATH)
  lib = built_lib.load()
  for name in ("mv_set_cell_mask", "mv_graph_captures", "mv_op_beam_step_masked",
               "mv_op_sbs_step_masked", "mv_op_sample_step_masked"):
    assert hasattr(raw, name), "libmultiverse_hip.so does not export " + name
    assert name in built_lib.EXPORTED_SYMBOLS and name in protos
  norm = lambda name: [" ".join(p.split()) for p in protos[name].split(",")]
  assert norm("mv_set_cell_mask") == ["mv_handle h", "const uint8_t* allowed", "int32_t Tm"]
  assert lib.mv_set_cell_mask.argtypes[1:] == [ctypes.POINTER(ctypes.c_uint8), ctypes.c_int32]
  # each masked op is its unmasked op plus the plane, behind the last input
  for name, at in (("mv_op_beam_step", 3), ("mv_op_sbs_step", 5), ("mv_op_sample_step", 2)):
    want = norm(name)
    want.insert(at, "const uint8_t* allowed")
    assert norm(name + "_masked") == want, name
    assert len(getattr(lib, name + "_masked").argtypes) == len(getattr(lib, name).argtypes) + 1
  assert lib.mv_abi_version() == 5 == built_lib.MV_ABI_VERSION    # new symbols only
  assert lib.mv_set_cell_mask(None, None, 1) != 0                 # NULL handle: an error code
  assert lib.mv_graph_captures(None, None) != 0
  assert ctypes.sizeof(built_lib.mv_config) == 28 * 4             # the structs keep their layout
  assert hasattr(built_lib.Engine, "set_cell_mask") and hasattr(built_lib.Engine, "graph_captures")
  import inspect
  for op in (built_lib.op_beam_step, built_lib.op_sbs_step, built_lib.op_sample_step):
    assert inspect.signature(op).parameters["allowed"].default is None


# ------------------------------------------------------------ cell_mask_from_scene

def _brute_force(onehot, h, w, classes, min_share):
  H, W = onehot.shape[:2]
  count = np.zeros((h, w), dtype=int)
  total = np.zeros((h, w), dtype=int)
  for i in range(H):
    for j in range(W):
      gi, gj = (i * h) // H, (j * w) // W
      total[gi, gj] += 1
      if any(onehot[i, j, c] for c in classes):
        count[gi, gj] += 1
  out = np.zeros((h, w), dtype=bool)
  for gi in range(h):
    for gj in range(w):
      out[gi, gj] = count[gi, gj] >= max(1, math.ceil(min_share * total[gi, gj]))
  return out


@pytest.mark.parametrize("H,W,grids,use", [(36, 64, [(18, 32), (9, 16)], (1, 0)),
                                           (36, 64, [(18, 32), (9, 16)], (0, 1)),
                                           (72, 36, [(36, 18), (18, 9)], (1, 0))])
def test_cell_mask_from_scene_is_the_brute_force_loop(H, W, grids, use):
  rng = np.random.RandomState(7 + H)
  C = 11
  cls = rng.randint(0, C, size=(H, W))
  cls[: H // 3] = 4                       # a block of one allowed class, a block of none
  cls[-H // 4:, : W // 2] = 0
  onehot = np.eye(C, dtype=np.uint8)[cls]
  args = argparse.Namespace(scene_grids=grids, use_grids=[bool(u) for u in use])
  h, w = grids[list(use).index(1)]
  seen = set()
  for share in (0.0, 0.5, 1.0):
    for classes in ([4], [1, 4, 7]):
      got = mf.cell_mask_from_scene(args, onehot, classes, share)
      assert got.shape == (h, w) and got.dtype == bool
      assert np.array_equal(got, _brute_force(onehot, h, w, classes, share)), (share, classes)
      seen.add(int(got.sum()))
  assert len(seen) >= 3 and 0 not in seen   # the cases differ, and the block of class 4 is allowed


# ------------------------------------------------------------ inference_feed

def _mf_args(ds, **over):
  a = argparse.Namespace(
      traj_path=ds["traj_path"], multifuture_path=ds["multifuture_path"],
      scene_feat_path=ds["scene_feat_path"], scene_id2name=ds["scene_id2name"],
      num_out=3, save_prob_file=None, greedy=False, center_only=False, obs_length=8,
      emb_size=32, enc_hidden_size=256, dec_hidden_size=256, grid_strides="2,4",
      use_grids="0,1", use_gnn=True, use_scene_enc=True, use_single_decoder=False,
      use_soft_grid_class=False, diverse_beam=True, diverse_gamma=0.01, fix_num_timestep=1,
      scene_h=36, scene_w=64, scene_class=11, convlstm_kernel=3, scene_conv_dim=64,
      scene_conv_kernel=3, video_h=1080, video_w=1920)
  for k, v in over.items():
    setattr(a, k, v)
  return mf.add_grid(a)


def test_inference_feed_carries_the_mask_and_the_fallback_list(tmp_path):
  ds = mf_fixture.make_dataset(str(tmp_path / "fp"), n_traj=4)
  files = sorted(glob(os.path.join(ds["traj_path"], "*.txt")))
  ids = [os.path.splitext(os.path.basename(f))[0] for f in files]
  gt = mf.load_gt(ds["multifuture_path"], ids)
  plain_args = _mf_args(ds)
  inputs = mf.get_inputs(plain_args, files, gt)
  idxs = [0, 2]
  T_pred = max(inputs["max_pred_lengths"][i] for i in idxs)
  plain, _ = mf.inference_feed(inputs, plain_args, idxs, batch_size=3, pred_length=T_pred)
  assert "cell_mask" not in plain and "cell_mask_fallback" not in plain
  # classes 1-3 on a quarter of a 4 x 4-pixel cell: about half of the 9 x 16 cells
  args = _mf_args(ds, allowed_classes=[1, 2, 3], allowed_min_share=0.25)
  feed, n_real = mf.inference_feed(inputs, args, idxs, batch_size=3, pred_length=T_pred)
  assert n_real == 2 and feed["cell_mask"].shape == (3, 144) and feed["cell_mask"].dtype == np.uint8
  assert feed["cell_mask_fallback"] == []
  for r, i in enumerate(idxs):
    last = inputs["scene_feats"][int(inputs["obs_scene"][i][-1][0])]       # the LAST frame
    want = mf.cell_mask_from_scene(args, last, [1, 2, 3], 0.25).reshape(-1)
    assert np.array_equal(feed["cell_mask"][r] != 0, want)
    assert 3 <= want.sum() < 144
    first = inputs["scene_feats"][int(inputs["obs_scene"][i][0][0])]
    assert not np.array_equal(want, mf.cell_mask_from_scene(args, first, [1, 2, 3], 0.25).reshape(-1))
  assert (feed["cell_mask"][2] == 1).all()                                  # the padding row
  for k in plain:                                                           # all else unchanged
    a, b = plain[k], feed[k]
    if isinstance(a, list):
      assert all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b)), k
    else:
      assert np.array_equal(a, b), k
  # one class on half of a cell's 16 pixels: no cell qualifies, every real row falls back
  none = _mf_args(ds, allowed_classes=[1], allowed_min_share=0.5)
  feed, _ = mf.inference_feed(inputs, none, idxs, batch_size=3, pred_length=T_pred)
  assert feed["cell_mask_fallback"] == [0, 1] and (feed["cell_mask"] == 1).all()
  none.unconstrained = []
  mf._note_unconstrained(none, feed, idxs, ids)          # pylint: disable=protected-access
  assert none.unconstrained == [ids[0], ids[2]]


# ------------------------------------------------------------ flags

def test_script_flags():
  flags = {f: (t, d) for f, t, d in cli._MF_FLAGS}                # pylint: disable=protected-access
  assert flags["--allowed_classes"] == (str, None) and flags["--allowed_min_share"] == (float, 0.0)
  p = cli.multifuture_inference_parser()
  base = ["traj", "mfut", "model", "out.p"]
  off = p.parse_args(base)
  assert off.allowed_classes is None and off.allowed_min_share == 0.0
  cli.parse_allowed_classes(off)
  assert off.allowed_classes is None and not hasattr(off, "unconstrained")
  a = p.parse_args(base + ["--allowed_classes", "1,4,7", "--allowed_min_share", "0.5", "--sample"])
  cli.parse_allowed_classes(a)
  assert a.allowed_classes == [1, 4, 7] and a.allowed_min_share == 0.5 and a.unconstrained == []
  for extra, word in ((["--allowed_classes", "1", "--greedy"], "--greedy"),
                      (["--allowed_classes", "1", "--score_gt", "s.p"], "--score_gt"),
                      (["--allowed_min_share", "0.5"], "--allowed_classes"),
                      (["--allowed_classes", "1,x"], "--allowed_classes"),
                      (["--allowed_classes", "11"], "scene_class"),
                      (["--allowed_classes", "1", "--allowed_min_share", "1.5"], "[0, 1]")):
    with pytest.raises(SystemExit) as err:
      cli.multifuture_inference_main(base + extra)
    assert word in str(err.value), extra


# ------------------------------------------------------------ the restatement

def test_all_allowed_is_the_unmasked_restatement_bit_for_bit():
  rng = np.random.RandomState(5)
  R, S, K = 8, 2, 70
  logits = (4.0 * rng.randn(R, K)).astype(np.float32)
  ones = np.ones((R // S, K), dtype=np.uint8)
  for temp in (1.0, 0.7):
    for limits in ((0, 1.0), (8, 0.9)):
      a = cm.sample_step(logits, S, 1, ones, temp, 9, limits[0], limits[1], dtype=np.float32)
      b = to.sample_step(logits, S, 1, temp, 9, limits[0], limits[1], dtype=np.float32)
      for k in ("keep", "ids", "q", "lp_id", "q_id", "compared"):
        assert a[k].tobytes() == b[k].tobytes(), (temp, limits, k)
  N, B = 2, 3
  l3 = (2.0 * rng.randn(N, B, K)).astype(np.float32)
  phi, LP, G = (-rng.rand(N, B).astype(np.float32) for _ in range(3))
  for t in (0, 1):
    a = cm.sbs_step(l3, phi, LP, G, t, np.ones((N, K)), 0.8, 3)
    b = sbs.step(l3, phi, LP, G, t, 0.8, 3)
    for k in ("new_phi", "new_lp", "new_g", "ids", "parents"):
      assert a[k].tobytes() == b[k].tobytes(), (t, k)


def test_a_mask_moves_the_proposal_and_leaves_the_model():
  rng = np.random.RandomState(6)
  R, S, K = 8, 2, 70
  logits = (4.0 * rng.randn(R, K)).astype(np.float32)
  allowed = rng.rand(R // S, K) < 0.5
  rows = np.repeat(allowed, S, axis=0)
  d = cm.sample_step(logits, S, 0, allowed, 0.7, 9, dtype=np.float64)
  assert not (d["keep"] & ~rows).any() and (d["keep"] == rows).all()        # no limit: keep == A
  assert rows[np.arange(R), d["ids"]].all()
  assert np.allclose(np.exp(d["q"]).sum(-1), 1.0) and (d["q"][~rows] == -np.inf).all()
  lp = sbs.log_softmax(logits.astype(np.float64))
  assert np.array_equal(d["lp_id"], lp[np.arange(R), d["ids"]])             # the model's, over all K
  # allowed logits 200 below the row maximum: the maximum over A keeps q~ finite
  low = logits.copy()
  low[:, :3] = low.max() + 200.0
  a = np.ones((R // S, K), dtype=bool)
  a[:, :3] = False
  q = cm.proposal(low, 1.0, np.repeat(a, S, 0), np.repeat(a, S, 0), np.float32)
  assert np.isfinite(q[:, 3:]).all() and np.allclose(np.exp(q.astype(np.float64)).sum(-1), 1.0)
  # beam: a masked cell is never selected, and ranks count allowed cells only
  N, B = 2, 3
  l3 = (2.0 * rng.randn(N, B, K)).astype(np.float32)
  prev = -rng.rand(N, B).astype(np.float32)
  am = rng.rand(N, K) < 0.5
  st = cm.beam_step(l3, prev, am, 2, True, 0.01, 0)
  assert am[np.arange(N)[:, None], st["ids"]].all()
  best = np.where(am[:, None, :], prev[..., None] + sbs.log_softmax(l3), -np.inf).max(-1)
  assert np.allclose(st["cand"].max(-1), best)                              # rank 0: no penalty
