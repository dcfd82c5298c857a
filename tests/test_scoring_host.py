# coding=utf-8
"""CPU: the layers around the scoring of given futures (mv_score_futures) -- the new C-ABI
symbols, the batch plan, the ground-truth futures as grid cells, the exact-NLL evaluation, the
script's flag, and the consistency of tests/scoring_oracle.py with itself."""
import argparse
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from multiverse_amd import cli, multifuture as mf, synth

import mf_fixture
import scoring_oracle as sco

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["mv_score_futures", "mv_upload_score_futures", "mv_run_score_resident",
           "mv_download_scores", "mv_time_score_resident"]


def test_library_exports_the_scoring_symbols(built_lib):
  text = open(os.path.join(ROOT, "include", "multiverse_hip.h")).read()
  text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
  protos = dict(re.findall(r"\bint\s+(mv_\w+)\s*\(([^;{]*?)\)\s*;", text))
  raw = ctypes.CDLL(built_lib.LIB_PATH)
  lib = built_lib.load()
  for name in SYMBOLS:
    assert hasattr(raw, name), "libmultiverse_hip.so does not export %s" % name
    assert name in built_lib.EXPORTED_SYMBOLS and name in protos
  args = lambda name: [" ".join(p.split()) for p in protos[name].split(",")]
  assert args("mv_score_futures") == ["mv_handle h", "const mv_inputs* in",
                                      "const mv_score_futures_in* fut", "mv_score_outputs* out"]
  assert args("mv_upload_score_futures") == ["mv_handle h", "const mv_score_futures_in* fut"]
  assert args("mv_time_score_resident") == ["mv_handle h", "int32_t iters", "float* ms_out"]
  assert lib.mv_abi_version() == 5 == built_lib.MV_ABI_VERSION    # new symbols only
  assert ctypes.sizeof(built_lib.mv_config) == 28 * 4             # the structs keep their layout
  assert [f[0] for f in built_lib.mv_score_futures_in._fields_] == ["ids", "lengths"]
  assert [f[0] for f in built_lib.mv_score_outputs._fields_] == \
      ["step_logprobs", "logprobs", "ranks"]
  assert lib.mv_run_score_resident(None) != 0                     # NULL handle: an error code
  for method in ("score_futures", "upload_score_futures", "run_score_resident", "scores",
                 "time_score_resident"):
    assert hasattr(built_lib.Engine, method)


def test_plan_seven_futures_at_three_per_row():
  """One sample of 7 futures at F = 3: three rows of the same sample, the last one padded."""
  lens = [[5, 2, 7, 1, 1, 3, 4]]
  plan = mf.plan_score_batches([7], lens, N=2, F=3)
  rows = [row for batch, _ in plan for row in batch]
  assert len(plan) == 2 and all(len(batch) == 2 for batch, _ in plan)
  real = [row for row in rows if row.sample is not None]
  assert [row.sample for row in real] == [0, 0, 0]
  assert sorted(j for row in real for j in row.futures) == list(range(7))
  for row in real:
    assert len(row.lengths) == 3
    assert row.lengths[:len(row.futures)] == [lens[0][j] for j in row.futures]
    assert row.lengths[len(row.futures):] == [0] * (3 - len(row.futures))
  assert [row.futures for row in real] == [[0, 1, 2], [6], [3, 4, 5]]   # L = 7, 4, 3
  assert [T for _, T in plan] == [7, 3]
  pad = rows[-1]
  assert pad.sample is None and pad.futures == [] and pad.lengths == [0, 0, 0]


def test_plan_orders_rows_and_covers_every_future_once():
  rng = np.random.default_rng(5)
  n_fut = [int(v) for v in rng.integers(1, 9, size=11)]
  lens = [[int(v) for v in rng.integers(1, 17, size=n)] for n in n_fut]
  for N, F in ((1, 3), (4, 3), (3, 20), (5, 1)):
    plan = mf.plan_score_batches(n_fut, lens, N, F)
    L = [max(row.lengths) for batch, _ in plan for row in batch]
    assert L == sorted(L, reverse=True)                    # descending over the whole plan
    seen = []
    for batch, T in plan:
      assert len(batch) == N and T == max(batch[0].lengths) >= 1
      for row in batch:
        assert len(row.lengths) == F
        if row.sample is None:
          assert row.lengths == [0] * F and row.futures == []
          continue
        assert 1 <= len(row.futures) <= F
        assert row.lengths == [lens[row.sample][j] for j in row.futures] + \
            [0] * (F - len(row.futures))
        seen += [(row.sample, j) for j in row.futures]
    assert sorted(seen) == [(i, j) for i in range(len(n_fut)) for j in range(n_fut[i])]
    # padding rows only at the end of the last batch
    samples = [row.sample for batch, _ in plan for row in batch]
    n_real = len([v for v in samples if v is not None])
    assert all(v is not None for v in samples[:n_real])
    assert len(samples) - n_real < N
  with pytest.raises(AssertionError):
    mf.plan_score_batches([2], [[3, 0]], 2, 3)


def _mf_args(use_grids="0,1"):
  return mf.add_grid(argparse.Namespace(grid_strides="2,4", use_grids=use_grids, scene_h=36,
                                        scene_w=64, video_h=1080, video_w=1920))


def test_futures_to_grid_ids_against_xy_to_grid_class(tmp_path):
  ds = mf_fixture.make_dataset(str(tmp_path / "fp"), n_traj=4)
  gt = mf.load_gt(ds["multifuture_path"], ds["traj_ids"])
  for use_grids, s in (("0,1", 1), ("1,0", 0)):
    args = _mf_args(use_grids)
    h, w = args.scene_grids[s]
    for traj_id in ds["traj_ids"]:
      ids, lengths = mf.futures_to_grid_ids(args, gt, traj_id, s)
      fids = list(gt[traj_id])
      assert ids.dtype == np.int32 and lengths.dtype == np.int32
      assert ids.shape == (len(fids), max(len(gt[traj_id][f]["x_agent_traj"]) for f in fids))
      for j, fid in enumerate(fids):
        tr = gt[traj_id][fid]["x_agent_traj"]
        assert lengths[j] == len(tr)
        for t, (_, _, x, y) in enumerate(tr):
          want = mf.xy_to_grid_class(np.asarray([[x, y]]), h, w, 1080, 1920)[0]
          assert ids[j, t] == want and 0 <= want < h * w
        assert (ids[j, len(tr):] == 0).all()


def test_eval_exact_nll_on_a_hand_made_dict():
  scores = {
      "a": {"f0": {"logprob": np.float32(-3.5),
                   "step_logprobs": np.asarray([-1.0, -2.0, -0.5], dtype=np.float32),
                   "ranks": np.asarray([0, 4, 7], dtype=np.int32)},
            "f1": {"logprob": np.float32(-3.0),
                   "step_logprobs": np.asarray([-3.0], dtype=np.float32),
                   "ranks": np.asarray([5], dtype=np.int32)}},
      "b": {"f0": {"logprob": np.float32(-0.75),
                   "step_logprobs": np.asarray([-0.5, -0.25], dtype=np.float32),
                   "ranks": np.asarray([0, 0], dtype=np.int32)}},
  }
  nll, counts, hits = mf.eval_exact_nll(scores)
  assert sorted(nll) == sorted(counts) == ["T=%d" % t for t in range(1, 6)]
  assert counts == {"T=1": 3, "T=2": 2, "T=3": 1, "T=4": 0, "T=5": 0}
  assert nll["T=1"] == pytest.approx((1.0 + 3.0 + 0.5) / 3)
  assert nll["T=2"] == pytest.approx((2.0 + 0.25) / 2)
  assert nll["T=3"] == pytest.approx(0.5)
  assert np.isnan(nll["T=4"]) and np.isnan(nll["T=5"])
  assert hits == {"top1": 3 / 6, "top5": 4 / 6, "steps": 6}
  # the shape of eval_grid_nll's result: (means by "T=k", counts by "T=k")
  nll2, counts2, _ = mf.eval_exact_nll(scores, time_list=(0, 2))
  assert sorted(nll2) == ["T=1", "T=3"] and counts2 == {"T=1": 3, "T=3": 1}


def test_script_flag():
  flags = {f: (t, d) for f, t, d in cli._MF_FLAGS}                # pylint: disable=protected-access
  assert flags["--score_gt"] == (str, None)
  p = cli.multifuture_inference_parser()
  base = ["traj", "mfut", "model", "out.p"]
  assert p.parse_args(base).score_gt is None
  assert p.parse_args(base + ["--score_gt", "scores.p", "--batch_size", "2"]).score_gt == \
      "scores.p"
  with pytest.raises(SystemExit) as err:
    cli.multifuture_inference_main(base + ["--score_gt", "scores.p", "--greedy"])
  assert "--score_gt" in str(err.value)


def test_oracle_is_consistent_with_itself_in_float64():
  """logprobs == the sum of step_logprobs over t < len; nothing past a future's length; the
  steps a shorter length shares with a longer one are the same steps."""
  cfg = synth.default_config(batch_size=2, use_grids=(0, 1), beam_size=3, enc_hidden_size=32,
                             dec_hidden_size=32, emb_size=16)
  cfg.max_pred_len = 4
  params = synth.make_params(cfg, recurrent_gain=3.0, bias_scale=0.1)
  feed = synth.make_feed(cfg, seed=synth.SEED_BASE + 91, pred_len=3)
  K = cfg.scene_grids[1][0] * cfg.scene_grids[1][1]
  ids = np.random.default_rng(3).integers(0, K, size=(2, 3, 3)).astype(np.int32)
  lens = np.asarray([[3, 1, 0], [2, 3, 3]])
  full = sco.forward(params, cfg, feed, ids, None, dtype=torch.float64)
  rag = sco.forward(params, cfg, feed, ids, lens, dtype=torch.float64)
  for out, ln in ((full, np.full((2, 3), 3)), (rag, lens)):
    assert out["logprobs"].dtype == np.float64
    for n in range(2):
      for f in range(3):
        L = int(ln[n, f])
        assert out["logprobs"][n, f] == pytest.approx(out["step_logprobs"][n, f, :L].sum(),
                                                      rel=1e-12, abs=1e-12)
        assert (out["step_logprobs"][n, f, L:] == 0).all()
        assert (out["ranks"][n, f, L:] == -1).all() and (out["logits"][n, f, L:] == 0).all()
        assert (out["ranks"][n, f, :L] >= 0).all() and (out["step_logprobs"][n, f, :L] < 0).all()
        for k in ("step_logprobs", "ranks", "logits"):
          assert (out[k][n, f, :L] == full[k][n, f, :L]).all()
  assert (rag["grid_reg"][0] == full["grid_reg"][0]).all()
  assert (rag["grid_reg"][1] == full["grid_reg"][1]).all()
  # garbage past the length is never read
  junk = ids.copy()
  junk[0, 1, 1:] = [-7, K + 5]
  junk[0, 2, :] = K + 5
  again = sco.forward(params, cfg, feed, junk, lens, dtype=torch.float64)
  assert all((again[k] == rag[k]).all() for k in rag)
  # the rank is the position in the descending stable order of the row
  lg = full["logits"][1, 2, 0]
  order = np.argsort(-lg, kind="stable")
  assert order[full["ranks"][1, 2, 0]] == ids[1, 2, 0]
