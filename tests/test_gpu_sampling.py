# coding=utf-8
"""GPU: the sampled multi-future decode (mv_set_sampling): S = beam_size futures per row drawn
by Gumbel-max from the model's own step distribution.  The reference has no sampler; the draw
is defined in include/multiverse_hip.h and restated by tests/sampling_oracle.py, so engine and
oracle agree draw for draw."""
import argparse
import functools
import os
import pickle

import numpy as np
import pytest

from multiverse_amd import cli, multifuture as mf, synth, tf_checkpoint

import mf_fixture
import sampling_oracle as so

pytestmark = pytest.mark.gpu

TOL = 1e-4            # the project's parity bar on logits and offsets
T_PRED = 3
TEMP, SEED = 0.8, 1234
LITERAL = dict(scene_h=72, scene_w=36, scene_grids=[(36, 18), (18, 9)])

# name -> (config overrides, used grid, S, feed seed).  The feed seeds were picked on the CPU
# with the oracle alone: at most a quarter of the (row, step) pairs fall behind a step whose
# top-1 / top-2 score margin is below 1e-4.
CASES = {
    "k144": (dict(), (0, 1), 3, synth.SEED_BASE + 81),     # 9 x 16: a partial third lane group
    "k576": (dict(), (1, 0), 3, synth.SEED_BASE + 82),     # 18 x 32: J = 9
    "k162": (LITERAL, (0, 1), 2, synth.SEED_BASE + 83),    # 18 x 9: K no multiple of 64
}


def _cfg(name, batch_size=2, S=None):
  over, grids, s_default, _ = CASES[name]
  cfg = synth.default_config(batch_size=batch_size, use_grids=grids,
                             beam_size=S or s_default, enc_hidden_size=128,
                             dec_hidden_size=128, **over)
  cfg.max_pred_len = 4
  return cfg


@functools.lru_cache(maxsize=None)
def _case(name):
  cfg = _cfg(name)
  params = synth.make_params(cfg, recurrent_gain=3.0, bias_scale=0.1)
  feed = synth.make_feed(cfg, seed=CASES[name][3], pred_len=T_PRED)
  return cfg, params, feed


@functools.lru_cache(maxsize=None)
def _oracle(name):
  cfg, params, feed = _case(name)
  return so.forward(params, cfg, feed, temperature=TEMP, seed=SEED)


def _centers(cfg):
  return mf.add_grid(argparse.Namespace(
      grid_strides="2,4", use_grids=[bool(u) for u in cfg.use_grids], scene_h=cfg.scene_h,
      scene_w=cfg.scene_w, video_h=1080, video_w=1920)).scene_grid_centers


def _engine(cfg, params, mode="f16x3", sampling=(TEMP, SEED)):
  import multiverse_amd._lib as lib
  eng = lib.Engine(cfg, device=0)
  eng.set_params(params)
  eng.set_compute_mode(mode)
  if sampling is not None:
    eng.set_sampling(*sampling)
  return eng


def _same(a, b):
  return all(a[k].tobytes() == b[k].tobytes() and a[k].shape == b[k].shape for k in a)


def _check_parity(name, mode):
  cfg, params, feed = _case(name)
  want = _oracle(name)
  eng = _engine(cfg, params, mode)
  arrs, s = eng.forward_beam(feed)
  eng.close()
  N, S, T = cfg.batch_size, cfg.beam_size, T_PRED
  K = cfg.scene_grids[s][0] * cfg.scene_grids[s][1]
  assert arrs["logits"].shape == (N, S, T, K) and arrs["ids"].shape == (N, S, T)
  assert arrs["logprobs"].shape == (N, S)
  assert (arrs["ids"] >= 0).all() and (arrs["ids"] < K).all()
  upto = so.compared_steps(want["margin"])                 # ids compared on steps [0, upto)
  cut = int((T - upto).sum())
  print("%s/%s: %d of %d (row, step) pairs behind a margin below 1e-4; smallest margin %.3g"
        % (name, mode, cut, N * S * T, want["margin"].min()))
  assert cut * 4 <= N * S * T
  for n in range(N):
    for j in range(S):
      u = int(upto[n, j])
      assert (arrs["ids"][n, j, :u] == want["ids"][n, j, :u]).all(), (n, j)
      lu = min(u + 1, T)                                   # the tied step's logits still hold
      d = float(np.abs(arrs["logits"][n, j, :lu] - want["logits"][n, j, :lu]).max())
      print("  row (%d, %d): %d steps, max|dlogits| %.3g" % (n, j, u, d))
      assert d < TOL
      if u == T:
        dl = abs(float(arrs["logprobs"][n, j]) - float(want["logprobs"][n, j]))
        assert dl < TOL * T, (n, j, dl)
  dr = float(np.abs(arrs["grid_reg"] - want["grid_reg"]).max())
  print("  max|dreg| %.3g" % dr)
  assert dr < TOL
  # best_beam is future 0
  assert (arrs["best_beam"].reshape(N, T, K) == arrs["logits"][:, 0]).all()


@pytest.mark.parametrize("mode", ["f32", "f16x3"])
@pytest.mark.parametrize("name", ["k144", "k576"])
def test_parity_with_the_oracle(built_lib, name, mode):
  _check_parity(name, mode)


def test_grid_of_162_cells(built_lib):
  """A literal 18 x 9 grid: K = 162 is no multiple of the wave (two full lane groups + 34)."""
  _check_parity("k162", "f16x3")


@functools.lru_cache(maxsize=None)
def _runs():
  """The forwards of the determinism / graph / decode tests, on ONE engine (9 x 16, N = 2)."""
  cfg, params, feed = _case("k144")
  eng = _engine(cfg, params)
  eng.set_grid_centers(_centers(cfg))
  runs = {}
  runs["a0"] = dict(eng.forward_beam(feed)[0])
  runs["trajs"] = {co: eng.decode_trajectories(center_only=co) for co in (False, True)}
  runs["occupancy"] = eng.beam_occupancy()
  runs["beam_ids"] = eng.beam_ids()
  runs["a1"] = dict(eng.forward_beam(feed)[0])
  eng.set_sampling(TEMP, SEED + 1)
  runs["b0"] = dict(eng.forward_beam(feed)[0])
  eng.set_graph_mode(True)
  for key, seed in (("ga", SEED), ("gb", SEED + 1), ("ga2", SEED)):
    eng.set_sampling(TEMP, seed)
    runs[key] = dict(eng.forward_beam(feed)[0])
  eng.set_sampling(2.0, SEED)                      # a replayed graph follows the temperature
  runs["g_hot"] = dict(eng.forward_beam(feed)[0])
  eng.set_graph_mode(False)
  runs["hot"] = dict(eng.forward_beam(feed)[0])
  eng.clear_sampling()
  runs["beam_after"] = dict(eng.forward_beam(feed)[0])
  eng.close()
  fresh = _engine(cfg, params, sampling=None)
  runs["beam_fresh"] = dict(fresh.forward_beam(feed)[0])
  fresh.close()
  return cfg, feed, runs


def test_determinism_and_seeds(built_lib):
  _, _, r = _runs()
  assert _same(r["a0"], r["a1"])
  assert not (r["a0"]["ids"] == r["b0"]["ids"]).all()
  assert not (r["a0"]["ids"] == r["hot"]["ids"]).all()
  # sampling cleared: the handle searches again, bit for bit what a fresh beam handle does
  assert _same(r["beam_after"], r["beam_fresh"])
  assert not (r["beam_after"]["ids"] == r["a0"]["ids"]).all()


def test_graph_mode_follows_seed_and_temperature(built_lib):
  _, _, r = _runs()
  assert _same(r["ga"], r["a0"]) and _same(r["gb"], r["b0"]) and _same(r["ga2"], r["a0"])
  assert _same(r["g_hot"], r["hot"])


def test_rows_do_not_depend_on_the_batch(built_lib):
  """Header: batch row n draws as row 0 of a forward seeded seed + n * 0x632BE5AB (mod 2^32),
  whatever the batch around it."""
  cfg3 = _cfg("k144", batch_size=3)
  params = synth.make_params(cfg3, recurrent_gain=3.0, bias_scale=0.1)
  feed3 = synth.make_feed(cfg3, seed=synth.SEED_BASE + 84, pred_len=T_PRED)
  eng = _engine(cfg3, params)
  a3, _ = eng.forward_beam(feed3)
  eng.close()
  cfg1 = _cfg("k144", batch_size=1)
  eng1 = _engine(cfg1, params)
  for n in range(3):
    feed1 = dict(feed3, obs_scene=feed3["obs_scene"][n:n + 1],
                 grid_obs_labels=[a[n:n + 1] for a in feed3["grid_obs_labels"]],
                 grid_obs_regress=[a[n:n + 1] for a in feed3["grid_obs_regress"]])
    eng1.set_sampling(TEMP, so.row_seed(SEED, n))
    a1, _ = eng1.forward_beam(feed1)
    for k in ("ids", "logits", "logprobs", "grid_reg", "best_beam"):
      assert a1[k][0].tobytes() == a3[k][n].tobytes(), (n, k)
  eng1.close()


def test_future_s_is_the_same_for_every_number_of_futures(built_lib):
  """Header: future s draws the same noise for every beam_size > s.  (S = 2 .. 4: a handle of
  beam_size 1 is a greedy handle, which does not sample.)"""
  _, params, feed = _case("k144")
  outs = {}
  for S in (2, 3, 4):
    cfg = _cfg("k144", S=S)
    eng = _engine(cfg, params)
    outs[S] = eng.forward_beam(feed)[0]
    eng.close()
  for S in (2, 3):
    for k in ("ids", "logits", "logprobs"):
      assert outs[S][k].tobytes() == np.ascontiguousarray(outs[4][k][:, :S]).tobytes(), (S, k)
    assert outs[S]["grid_reg"].tobytes() == outs[4]["grid_reg"].tobytes()


def test_ragged_rows_are_bitwise_their_uniform_forwards(built_lib):
  lens = [3, 0, 2]
  cfg = _cfg("k144", batch_size=3)
  params = synth.make_params(cfg, recurrent_gain=3.0, bias_scale=0.1)
  feed = synth.make_feed(cfg, seed=synth.SEED_BASE + 84, pred_len=T_PRED)
  eng = _engine(cfg, params)
  eng.set_grid_centers(_centers(cfg))
  rag = dict(eng.forward_beam(dict(feed, pred_lengths=lens))[0])
  rag_rows = eng.last_forward_gate_rows()
  rag_occ, rag_traj = eng.beam_occupancy(), eng.decode_trajectories()
  uni, uni_rows = {}, {}
  for L in (3, 2):
    uni[L] = dict(eng.forward_beam(dict(feed, pred_length=L))[0])
    uni_rows[L] = eng.last_forward_gate_rows()
    uni[L]["occupancy"], uni[L]["trajs"] = eng.beam_occupancy(), eng.decode_trajectories()
  eng.close()
  rag["occupancy"], rag["trajs"] = rag_occ, rag_traj
  axis = {"ids": 1, "logits": 1, "best_beam": 0, "grid_reg": 0, "occupancy": 0, "trajs": 1}
  for n, L in enumerate(lens):
    for k, ax in axis.items():
      a = np.moveaxis(rag[k][n], ax, 0)
      assert (a[L:] == (-1 if k == "ids" else 0)).all(), (n, k)
      if L:
        want = np.moveaxis(uni[L][k][n], ax, 0)
        assert a[:L].tobytes() == np.ascontiguousarray(want).tobytes(), (n, k)
    if L:
      assert rag["logprobs"][n].tobytes() == uni[L]["logprobs"][n].tobytes(), n
    else:
      assert (rag["logprobs"][n] == 0).all()
  print("gate rows: ragged %d, uniform %d" % (rag_rows, uni_rows[3]))
  assert rag_rows < uni_rows[3]


def test_decode_calls(built_lib):
  cfg, _, r = _runs()
  arrs = r["a0"]
  N, S = cfg.batch_size, cfg.beam_size
  s = list(cfg.use_grids).index(True)
  ids, lp = r["beam_ids"]
  assert (ids == arrs["ids"]).all() and (lp == arrs["logprobs"]).all()
  for center_only in (False, True):
    args = mf.add_grid(argparse.Namespace(
        grid_strides="2,4", use_grids=[bool(u) for u in cfg.use_grids], scene_h=36, scene_w=64,
        video_h=1080, video_w=1920, greedy=False, center_only=center_only, num_out=S))
    want = np.asarray([mf.decode_trajectories(
        args, None, arrs["grid_reg"][n], (arrs["logits"][n], arrs["ids"][n], arrs["logprobs"][n]),
        T_PRED, s) for n in range(N)])
    dev = r["trajs"][center_only]
    assert dev.dtype == np.float64 and dev.shape == want.shape == (N, S, T_PRED, 2)
    assert (dev == want).all()

  def mixture(dtype):        # (1 / S) * sum_s softmax_k(logits[n, s, t, :]), beams in order s
    x = arrs["logits"].astype(dtype)
    e = np.exp(x - x.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    w = dtype(1) / dtype(S)
    out = np.zeros_like(p[:, 0])
    for j in range(S):
      out = out + p[:, j] * w
    return out

  exact, ref32 = mixture(np.float64), mixture(np.float32)
  dev = r["occupancy"]
  assert dev.dtype == np.float32 == ref32.dtype and dev.shape == exact.shape
  d_ref = float((np.abs(ref32 - exact) / exact).max())
  d_dev = float((np.abs(dev - exact) / exact).max())
  rows = float(np.abs(dev.astype(np.float64).sum(-1) - 1).max())
  print("uniform mixture: host float32 vs fp64 %.3g, device vs fp64 %.3g (bar %.3g), rows sum "
        "to 1 within %.3g" % (d_ref, d_dev, 4 * d_ref, rows))
  # the bar of test_gpu_multifuture_decode.py for the beam's map against its host formula
  assert d_dev <= 4 * d_ref
  assert rows <= 1e-6


def test_script_sample_device_decode_equals_host_decode(built_lib, tmp_path):
  ds = mf_fixture.make_dataset(str(tmp_path / "fp"), n_traj=4)
  cfg = synth.default_config(batch_size=1, use_grids=(0, 1), beam_size=3)
  params = synth.make_params(cfg, seed=synth.SEED_BASE + 31, recurrent_gain=3.0,
                             bias_scale=0.1)
  model_dir = str(tmp_path / "model")
  tf_checkpoint.save_checkpoint(os.path.join(model_dir, "save-best"), params, global_step=100)
  files = [str(tmp_path / n) for n in ("host.p", "dev.p", "other.p", "beam.p")]
  tail = ["--num_out", "3", "--emb_size", "32", "--use_grids", "0,1", "--use_gnn",
          "--use_scene_enc", "--scene_feat_path", ds["scene_feat_path"],
          "--scene_id2name", ds["scene_id2name"], "--obs_length", "8", "--batch_size", "2"]
  head = [ds["traj_path"], ds["multifuture_path"], model_dir]
  sample = ["--sample", "--sample_temperature", "0.9", "--sample_seed", "5"]
  cli.multifuture_inference_main(head + [files[0]] + tail + sample)
  cli.multifuture_inference_main(head + [files[1]] + tail + sample + ["--device_decode"])
  cli.multifuture_inference_main(head + [files[2]] + tail + sample[:3] +
                                 ["--sample_seed", "6", "--device_decode"])
  cli.multifuture_inference_main(head + [files[3]] + tail)
  host, dev, other, beam = (pickle.load(open(f, "rb")) for f in files)
  assert list(host) == list(dev) and len(host) == 4
  differs = False
  for t in host:
    a, b = np.asarray(host[t]), np.asarray(dev[t])
    assert a.shape == b.shape and a.shape[0] == 3 and a.dtype == b.dtype == np.float64
    assert (a == b).all(), t
    differs = differs or not (a == np.asarray(other[t])).all()
  assert differs                                         # another seed, other futures
  assert any(not (np.asarray(host[t]) == np.asarray(beam[t])).all() for t in host)


def test_errors_name_their_cause(built_lib):
  lib = built_lib
  cfg, params, feed = _case("k144")
  greedy = synth.default_config(batch_size=2, use_grids=(0, 1), enc_hidden_size=128,
                                dec_hidden_size=128)
  geng = lib.Engine(greedy, device=0)
  with pytest.raises(lib.MvError) as err:
    geng.set_sampling(1.0, 0)
  assert "beam_size 1" in str(err.value)
  geng.clear_sampling()                                   # clearing is always allowed
  geng.close()
  single = _cfg("k144")
  single.use_single_decoder = True
  seng = lib.Engine(single, device=0)
  with pytest.raises(lib.MvError) as err:
    seng.set_sampling(1.0, 0)
  assert "use_single_decoder" in str(err.value)
  seng.close()
  eng = _engine(cfg, params, sampling=None)
  for temp in (0.0, -0.5, float("nan")):
    with pytest.raises(lib.MvError) as err:
      eng.set_sampling(temp, 0)
    assert "temperature" in str(err.value)
  eng.set_sampling(1.0, 0)
  for call in (eng.train_init, eng.train_step, eng.train_forward_backward, eng.train_apply):
    with pytest.raises(lib.MvError) as err:
      call()
    assert "sampling is on" in str(err.value), call
  eng.close()
