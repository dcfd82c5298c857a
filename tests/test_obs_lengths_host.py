# coding=utf-8
"""CPU: the layers around per-row observation lengths -- the new C-ABI symbol, `get_inputs`
with and without `allow_short_obs`, the right alignment and padding of `inference_feed`, the
batch planners with observation lengths, the closed form of the encoder rows an obs-ragged
forward launches, and the command-line flag."""
import argparse
import ctypes
import os
import re
from glob import glob

import numpy as np
import pytest

from multiverse_amd import cli, multifuture as mf

import mf_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHORT = {1: 5, 2: 1, 4: 3}            # sample index -> observed frames (the others keep 8)


def test_library_exports_mv_set_obs_lengths(built_lib):
  text = open(os.path.join(ROOT, "include", "multiverse_hip.h")).read()
  text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
  protos = dict(re.findall(r"\bint\s+(mv_\w+)\s*\(([^;{]*?)\)\s*;", text))
  raw = ctypes.CDLL(built_lib.LIB_PATH)
  lib = built_lib.load()
  assert hasattr(raw, "mv_set_obs_lengths")
  assert "mv_set_obs_lengths" in built_lib.EXPORTED_SYMBOLS
  assert [" ".join(p.split()) for p in protos["mv_set_obs_lengths"].split(",")] == \
      ["mv_handle h", "const int32_t* lengths"]
  assert len(lib.mv_set_obs_lengths.argtypes) == 2
  assert lib.mv_set_obs_lengths.argtypes[1]._type_ is ctypes.c_int32
  assert lib.mv_abi_version() == 5              # a new symbol only
  assert lib.mv_set_obs_lengths(None, None) != 0     # a NULL handle is an error code


# ------------------------------------------------------------ get_inputs / inference_feed

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


def _short_dataset(tmp_path, n_traj=6):
  """The fixture dataset, and a copy of its trajectory files in which the samples of SHORT
  entered the scene late (two lines per frame: the agent and another one)."""
  ds = mf_fixture.make_dataset(str(tmp_path / "fp"), n_traj=n_traj)
  files = sorted(glob(os.path.join(ds["traj_path"], "*.txt")))
  ids = [os.path.splitext(os.path.basename(f))[0] for f in files]
  short_dir = str(tmp_path / "short")
  os.makedirs(short_dir)
  lengths = []
  for k, f in enumerate(files):
    lines = open(f).read().splitlines()
    L = SHORT.get(k, 8)
    lengths.append(L)
    with open(os.path.join(short_dir, os.path.basename(f)), "w") as out:
      out.write("\n".join(lines[2 * (8 - L):]) + "\n")
  short_files = sorted(glob(os.path.join(short_dir, "*.txt")))
  return ds, files, short_files, ids, mf.load_gt(ds["multifuture_path"], ids), lengths


def test_get_inputs_with_and_without_the_flag(tmp_path):
  ds, files, short_files, ids, gt, lengths = _short_dataset(tmp_path)
  full = mf.get_inputs(_mf_args(ds), files, gt)
  assert "obs_lengths" not in full                         # unchanged without the flag
  with pytest.raises(AssertionError):
    mf.get_inputs(_mf_args(ds), short_files, gt)           # ... and the assert stays
  flagged_full = mf.get_inputs(_mf_args(ds, allow_short_obs=True), files, gt)
  assert flagged_full["obs_lengths"] == [8] * len(files)
  for key in ("obs_traj", "obs_grid_class", "obs_scene"):
    for a, b in zip(full[key], flagged_full[key]):
      assert np.array_equal(a, b), key
  short = mf.get_inputs(_mf_args(ds, allow_short_obs=True), short_files, gt)
  assert short["obs_lengths"] == lengths
  assert short["max_pred_lengths"] == full["max_pred_lengths"]
  for i, L in enumerate(lengths):                          # the track's LAST L observations
    assert short["obs_traj"][i].shape == (L, 2)
    assert np.array_equal(short["obs_traj"][i], full["obs_traj"][i][-L:])
    assert np.array_equal(short["obs_grid_class"][i], full["obs_grid_class"][i][:, -L:])
    assert short["obs_scene"][i].shape == (L, 1)
    for s in range(2):
      assert np.array_equal(short["obs_grid_target"][i][s], full["obs_grid_target"][i][s][-L:])
  # more frames than obs_length, or none, is refused with the flag as well
  with pytest.raises(AssertionError):
    mf.get_inputs(_mf_args(ds, allow_short_obs=True, obs_length=4), files, gt)


def test_inference_feed_right_aligns_and_pads_short_tracks(tmp_path):
  ds, files, short_files, ids, gt, lengths = _short_dataset(tmp_path)
  args = _mf_args(ds, allow_short_obs=True)
  full = mf.get_inputs(_mf_args(ds), files, gt)
  short = mf.get_inputs(args, short_files, gt)
  idxs = [0, 1, 2, 4]
  T_pred = max(full["max_pred_lengths"][i] for i in idxs)
  feed, n_real = mf.inference_feed(short, args, idxs, batch_size=5, pred_length=T_pred)
  ref, _ = mf.inference_feed(full, _mf_args(ds), idxs, batch_size=5, pred_length=T_pred)
  assert n_real == 4
  assert feed["obs_lengths"].dtype == np.int32
  assert feed["obs_lengths"].tolist() == [lengths[i] for i in idxs] + [lengths[idxs[-1]]]
  assert "obs_lengths" not in ref
  for r, i in enumerate(idxs + [idxs[-1]]):
    L = lengths[i]
    for s in range(2):
      lab, want = feed["grid_obs_labels"][s][r], ref["grid_obs_labels"][s][r]
      assert lab.shape == (8,)
      assert np.array_equal(lab[8 - L:], want[8 - L:])               # right-aligned
      assert (lab[:8 - L] == want[8 - L]).all()                      # the first observation
    reg, want = feed["grid_obs_regress"][1][r], ref["grid_obs_regress"][1][r]
    assert reg.shape == want.shape and reg.dtype == np.float32 and np.isfinite(reg).all()
    assert np.array_equal(reg[8 - L:], want[8 - L:])
    assert all(np.array_equal(reg[t], want[8 - L]) for t in range(8 - L))
    assert feed["grid_obs_regress"][0] is None
    # scene frames: the same frames at the right-aligned columns, the first one in front
    got = feed["scene_feat"][feed["obs_scene"][r]]
    want = ref["scene_feat"][ref["obs_scene"][r]]
    assert np.array_equal(got[8 - L:], want[8 - L:])
    assert all(np.array_equal(got[t], want[8 - L]) for t in range(8 - L))
  assert 0 <= feed["obs_scene"].min() and feed["obs_scene"].max() < feed["scene_feat"].shape[0]
  # the scene table holds only the frames the batch really uses
  assert feed["scene_feat"].shape[0] == sum(lengths[i] for i in idxs)
  # a batch without a short row carries no lengths: the engine runs the uniform forward
  feed0, _ = mf.inference_feed(short, args, [0, 3], batch_size=2,
                               pred_length=max(full["max_pred_lengths"][i] for i in (0, 3)))
  ref0, _ = mf.inference_feed(full, _mf_args(ds), [0, 3], batch_size=2,
                              pred_length=feed0["pred_length"])
  assert "obs_lengths" not in feed0
  for key in ("obs_scene", "scene_feat"):
    assert np.array_equal(feed0[key], ref0[key])
  assert np.array_equal(feed0["grid_obs_regress"][1], ref0["grid_obs_regress"][1])


# ------------------------------------------------------------ planners

PRED = [25, 14, 14, 19, 22, 14, 25, 16, 14, 21, 19, 23, 14]
OBS = [3, 8, 2, 8, 1, 5, 8, 8, 8, 4, 6, 8, 2]


@pytest.mark.parametrize("N", [1, 3, 4, 16])
def test_plan_ragged_batches_orders_ties_by_observation_length(N):
  plain = mf.plan_ragged_batches(PRED, N)
  assert mf.plan_ragged_batches(PRED, N, obs_lengths=None) == plain       # unchanged without
  assert [i for idxs, _, _ in plain.batches for i in idxs] == \
      sorted(range(len(PRED)), key=lambda i: (-PRED[i], i))
  plan = mf.plan_ragged_batches(PRED, N, obs_lengths=OBS)
  seen = [i for idxs, _, _ in plan.batches for i in idxs]
  assert sorted(seen) == list(range(len(PRED)))
  assert [PRED[i] for i in seen] == sorted(PRED, reverse=True)           # as before
  assert seen == sorted(range(len(PRED)), key=lambda i: (-PRED[i], -OBS[i], i))
  for a, b in zip(seen, seen[1:]):
    if PRED[a] == PRED[b]:
      assert OBS[a] > OBS[b] or (OBS[a] == OBS[b] and a < b)
  assert [(r, T) for _, r, T in plan.batches] == [(r, T) for _, r, T in plain.batches]
  assert plan.ragged_row_steps == plain.ragged_row_steps
  assert plan.grouped_row_steps == plain.grouped_row_steps
  # all observation lengths equal: the plain plan
  assert mf.plan_ragged_batches(PRED, N, obs_lengths=[8] * len(PRED)) == plain


def test_plan_score_batches_orders_ties_by_observation_length():
  n_fut = [2, 1, 3, 1]
  lens = [[5, 3], [5], [2, 5, 1], [4]]
  plain = mf.plan_score_batches(n_fut, lens, 2, 2)
  assert mf.plan_score_batches(n_fut, lens, 2, 2, obs_lengths=None) == plain
  assert mf.plan_score_batches(n_fut, lens, 2, 2, obs_lengths=[8, 8, 8, 8]) == plain
  plan = mf.plan_score_batches(n_fut, lens, 2, 2, obs_lengths=[2, 8, 5, 8])
  rows = [row for batch, _ in plan for row in batch if row.sample is not None]
  assert [max(r.lengths) for r in rows] == sorted([max(r.lengths) for r in rows], reverse=True)
  assert [r.sample for r in rows] == [1, 2, 0, 3, 2]      # 5-ties: obs 8, 5, 2; then 4; then 1
  assert sorted((r.sample, tuple(r.futures)) for r in rows) == \
      sorted((r.sample, tuple(r.futures)) for b, _ in plain for r in b if r.sample is not None)


def test_inference_batches_group_rows_by_observation_length(tmp_path):
  inputs = {"max_pred_lengths": [12, 14, 12, 12, 14], "obs_lengths": [3, 8, 8, 5, 8]}
  args = argparse.Namespace(ragged_batches=False)
  assert mf._inference_batches(args, inputs, 5, 2) == [([2, 3], None), ([0], None), ([1, 4], None)]
  del inputs["obs_lengths"]
  assert mf._inference_batches(args, inputs, 5, 2) == [([0, 2], None), ([3], None), ([1, 4], None)]


# ------------------------------------------------------------ the launch contract

def _brute_force_rows(lo, T, live):
  total = 0
  for t in range(T):
    started = [n for n in range(live) if lo[n] >= T - t]
    total += (1 + max(started)) if started else 0
  return total


def test_sum_enc_prefix_rows_against_a_brute_force_count():
  rng = np.random.default_rng(5)
  for _ in range(300):
    T = int(rng.integers(1, 9))
    N = int(rng.integers(1, 12))
    lo = rng.integers(1, T + 1, size=N).tolist()
    live = int(rng.integers(0, N + 1))
    assert mf.sum_enc_prefix_rows(lo, T) == _brute_force_rows(lo, T, N)
    assert mf.sum_enc_prefix_rows(lo, T, live_rows=live) == _brute_force_rows(lo, T, live)
    srt = sorted(lo, reverse=True)
    assert mf.sum_enc_prefix_rows(srt, T) == sum(lo)               # sorted: no unstarted row
    assert mf.sum_enc_prefix_rows(lo, T) >= sum(lo)
    assert mf.sum_enc_prefix_rows([T] * N, T) == N * T             # the uniform forward
  with pytest.raises(AssertionError):
    mf.sum_enc_prefix_rows([0, 2], 4)
  with pytest.raises(AssertionError):
    mf.sum_enc_prefix_rows([5, 2], 4)


# ------------------------------------------------------------ command line

def test_cli_flag():
  p = cli.multifuture_inference_parser()
  base = ["traj", "mf", "model", "out.p"]
  assert p.parse_args(base).allow_short_obs is False
  assert p.parse_args(base + ["--allow_short_obs"]).allow_short_obs is True
  script = open(os.path.join(ROOT, "scripts", "multifuture_inference.py")).read()
  assert "cli.multifuture_inference_main()" in script      # the script takes the flag from cli
