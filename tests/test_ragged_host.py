# coding=utf-8
"""CPU: the layers around per-row prediction lengths -- the two new C-ABI symbols, the
batch planner (`multifuture.plan_ragged_batches`) and `run_inference` /
`run_inference_device` with `ragged_batches` against the grouped schedule."""
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

NEW = {"mv_set_pred_lengths": ["mv_handle h", "const int32_t* lengths"],
       "mv_last_forward_gate_rows": ["mv_handle h", "int64_t* rows"]}


def test_library_exports_the_ragged_entry_points(built_lib):
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
    for p, t in zip(want, fn.argtypes):
      is_ptr = hasattr(t, "contents") or t is ctypes.c_void_p
      assert is_ptr == ("*" in p or p.startswith("mv_handle")), (name, p, t)
  assert lib.mv_set_pred_lengths.argtypes[1]._type_ is ctypes.c_int32
  assert lib.mv_last_forward_gate_rows.argtypes[1]._type_ is ctypes.c_int64
  assert lib.mv_abi_version() == 5              # new symbols only
  # a NULL handle is an error code, not a crash
  assert lib.mv_set_pred_lengths(None, None) != 0
  assert lib.mv_last_forward_gate_rows(None, None) != 0


# ------------------------------------------------------------ the planner

def _grouped_row_steps(lengths, N):
  out = 0
  for T in set(lengths):
    g = sum(1 for l in lengths if l == T)
    out += -(-g // N) * N * T
  return out


def _fixture_lengths(tmp_path, n_traj=7):
  ds = mf_fixture.make_dataset(str(tmp_path), n_traj=n_traj)
  files = sorted(glob(os.path.join(ds["traj_path"], "*.txt")))
  ids = [os.path.splitext(os.path.basename(f))[0] for f in files]
  gt = mf.load_gt(ds["multifuture_path"], ids)
  return ds, files, ids, gt


HAND = [25, 14, 14, 19, 22, 17, 25, 16, 14, 21, 19, 23, 15]      # 9 distinct lengths


@pytest.mark.parametrize("N", [1, 3, 4, 16])
def test_plan_ragged_batches(tmp_path, N):
  ds, files, ids, gt = _fixture_lengths(tmp_path)
  fixture = mf.get_inputs(_mf_args(ds), files, gt)["max_pred_lengths"]
  assert len(set(HAND)) >= 6 and len(set(fixture)) > 1
  for lengths in (fixture, HAND):
    plan = mf.plan_ragged_batches(lengths, N)
    seen = [i for idxs, _, _ in plan.batches for i in idxs]
    assert sorted(seen) == list(range(len(lengths)))            # every sample exactly once
    flat = [lengths[i] for i in seen]
    assert flat == sorted(lengths, reverse=True)                # descending over the run
    assert seen == sorted(range(len(lengths)), key=lambda i: (-lengths[i], i))   # ties by index
    for k, (idxs, row_lengths, pred_length) in enumerate(plan.batches):
      assert len(row_lengths) == N and 1 <= len(idxs) <= N
      assert row_lengths[:len(idxs)] == [lengths[i] for i in idxs]
      assert all(l == 0 for l in row_lengths[len(idxs):])       # the pad rows
      assert len(idxs) == N or k == len(plan.batches) - 1       # only the last batch is padded
      assert pred_length == max(row_lengths) == row_lengths[0]
    # decoder row-steps: a sorted batch launches exactly its unfinished rows at every step
    launched = sum(sum(1 for l in row_lengths if l > t)
                   for _, row_lengths, T in plan.batches for t in range(T))
    assert plan.ragged_row_steps == launched == sum(lengths)
    assert plan.grouped_row_steps == _grouped_row_steps(lengths, N)
    assert plan.ragged_row_steps <= plan.grouped_row_steps
  if N > 1:
    assert mf.plan_ragged_batches(HAND, N).ragged_row_steps < \
        mf.plan_ragged_batches(HAND, N).grouped_row_steps


# ------------------------------------------------------------ run_inference

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


class _RowModel(object):
  """A canned model whose row output is a function of that row's inputs and its length alone
  -- what the engine guarantees bit for bit on the GPU (tests/test_gpu_ragged.py) -- with the
  ragged forward's padding past a row's end: zeros, ids -1."""

  def __init__(self, cfg, args):
    self.config, self.args = cfg, args
    self.feeds = []

  def _arrays(self, feed):
    N, B, T = self.config.batch_size, self.args.num_out, int(feed["pred_length"])
    h, w = self.args.scene_grids[1]
    K = h * w
    lens = feed.get("pred_lengths")
    lens = [T] * N if lens is None else [int(l) for l in lens]
    assert len(lens) == N and max(lens) == T and min(lens) >= 0
    self.feeds.append((T, lens))
    ids = np.full((N, B, T), -1, "int32")
    logits = np.zeros((N, B, T, K), "f4")
    reg = np.zeros((N, T, h, w, 2), "f4")
    logprobs = np.zeros((N, B), "f4")
    for n, L in enumerate(lens):
      if L == 0:
        continue
      r = np.random.default_rng(int(feed["grid_obs_labels"][1][n].sum()) * 7 + L)
      ids[n, :, :L] = r.integers(0, K, size=(B, L))
      logits[n, :, :L] = r.normal(0, 2, size=(B, L, K))
      reg[n, :L] = r.normal(0, 20, size=(L, h, w, 2))
      logprobs[n] = -np.sort(r.uniform(0, 9, size=B))
    return ids, logits, reg, logprobs, lens

  def run_forward(self, feed):
    ids, logits, reg, logprobs, _ = self._arrays(feed)
    N, _, T, _ = logits.shape
    h, w = self.args.scene_grids[1]
    beam = None if self.args.greedy else [logits, ids, logprobs]
    return [[], logits[:, 0].reshape(N, T, h, w, 1)], [[], reg], beam

  def run_forward_decoded(self, feed, center_only=False, occupancy=False, grid_centers=None,
                          logits=False):
    ids, lg, reg, logprobs, lens = self._arrays(feed)
    N, B, T, K = lg.shape
    centers = np.asarray(grid_centers[1], dtype=np.float64).reshape(-1, 2)
    if self.args.greedy:
      ids = lg[:, :1].argmax(-1).astype("int32")
    trajs = np.zeros((N, ids.shape[1], T, 2), np.float64)
    occ = np.zeros((N, T, K), "f4")
    for n, L in enumerate(lens):
      for t in range(L):
        trajs[n, :, t] = centers[ids[n, :, t]]
        if not center_only:
          trajs[n, :, t] = trajs[n, :, t] + reg[n, t].reshape(K, 2)[ids[n, :, t]]
        occ[n, t] = (mf._softmax(lg[n, :, t], axis=-1) *
                     mf._softmax(logprobs[n], axis=-1)[:, None]).sum(0)
    out = {"trajs": trajs}
    if not self.args.greedy:
      out.update(ids=ids, logprobs=logprobs)
    if occupancy:
      out["occupancy"] = occ
    if logits:
      out["logits"] = lg
    return out


def _same(a, b):
  a, b = np.asarray(a), np.asarray(b)
  return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("device_decode", [False, True])
@pytest.mark.parametrize("N", [1, 4])
def test_run_inference_ragged_batches_equal_the_grouped_path(tmp_path, N, device_decode):
  ds, files, ids, gt = _fixture_lengths(tmp_path)
  for greedy in (False, True):
    over = dict(greedy=greedy, save_prob_file="x", device_decode=device_decode)
    if device_decode:
      over["save_occupancy_file"] = "y"
    args = _mf_args(ds, **over)
    inputs = mf.get_inputs(args, files, gt)
    lens = inputs["max_pred_lengths"]
    cfg = mf.model_config(args, batch_size=N, max_pred_len=max(lens))
    grouped_model = _RowModel(cfg, args)
    want = mf.run_inference(args, grouped_model, inputs, ids)
    assert all(set(l) == {T} for T, l in grouped_model.feeds)     # uniform feeds only
    args_r = _mf_args(ds, ragged_batches=True, **over)
    ragged_model = _RowModel(cfg, args_r)
    got = mf.run_inference(args_r, ragged_model, inputs, ids)
    plan = mf.plan_ragged_batches(lens, N)
    assert [(T, l) for _, l, T in plan.batches] == ragged_model.feeds
    assert len(ragged_model.feeds) <= len(grouped_model.feeds)
    assert len(got) == len(want) == (3 if device_decode else 2)
    assert list(got[0]) == list(want[0]) == ids
    for t in ids:
      assert len(got[0][t]) == len(want[0][t]) == args.num_out
      for a, b in zip(got[0][t], want[0][t]):
        assert len(a) == len(b) == lens[ids.index(t)]
        assert all(_same(p, q) for p, q in zip(a, b))
    if greedy:
      assert got[1] == want[1] == {}
      continue
    assert list(got[1]) == list(want[1]) == ids
    for t in ids:
      assert _same(got[1][t][0], want[1][t][0]) and got[1][t][0].ndim == 4
      assert _same(got[1][t][1], want[1][t][1])
    if device_decode:
      assert list(got[2]) == list(want[2]) == ids
      for t in ids:
        assert _same(got[2][t], want[2][t]) and got[2][t].shape == (lens[ids.index(t)], 144)


def test_inference_feed_carries_the_row_lengths(tmp_path):
  ds, files, ids, gt = _fixture_lengths(tmp_path)
  args = _mf_args(ds)
  inputs = mf.get_inputs(args, files, gt)
  lens = inputs["max_pred_lengths"]
  idxs, row_lengths, T = mf.plan_ragged_batches(lens, 4).batches[-1]
  assert 0 in row_lengths                                          # 7 samples in batches of 4
  feed, n_real = mf.inference_feed(inputs, args, idxs, batch_size=4, lengths=row_lengths)
  assert n_real == len(idxs) and feed["pred_length"] == T == max(row_lengths)
  assert feed["pred_lengths"].dtype == np.int32 and feed["pred_lengths"].tolist() == row_lengths
  assert feed["grid_obs_labels"][1].shape == (4, 8)               # pad rows carry valid inputs
  plain, _ = mf.inference_feed(inputs, args, [0], batch_size=2)
  assert "pred_lengths" not in plain


def test_ragged_batches_flag_is_on_the_multifuture_script_only():
  p = cli.multifuture_inference_parser()
  base = ["traj", "mf", "model", "out.p"]
  assert p.parse_args(base).ragged_batches is False
  assert p.parse_args(base + ["--ragged_batches"]).ragged_batches is True
  for parser in (cli.train_parser, cli.test_parser) if hasattr(cli, "train_parser") else ():
    flags = {s for a in parser()._actions for s in a.option_strings}
    assert "--ragged_batches" not in flags
