# coding=utf-8
"""GPU: scoring of GIVEN futures (mv_score_futures): the teacher-forced log-likelihood, per
step, of beam_size futures per row under the class decoder.  The reference has no such call;
it is defined in include/multiverse_hip.h and restated by tests/scoring_oracle.py."""
import argparse
import contextlib
import functools
import io
import os
import pickle

import numpy as np
import pytest

from multiverse_amd import cli, multifuture as mf, synth, tf_checkpoint

import mf_fixture
import scoring_oracle as sco

pytestmark = pytest.mark.gpu

TOL = 1e-4            # the project's parity bar on logits and offsets
T_PRED = 3
TEMP, SEED = 0.8, 1234
LITERAL = dict(scene_h=72, scene_w=36, scene_grids=[(36, 18), (18, 9)])

# name -> (config overrides, used grid, F, feed seed, id seed).  The id seeds were picked on the
# CPU with the oracle alone: at most a quarter of the (row, step) pairs have the given cell's
# logit within 1e-4 of another cell's (there the rank may differ from the oracle's): 0 of 18,
# 4 of 18 (the 576 logits of a row lie within ~1 of each other: about half of all random cells sit
# that close to a neighbour, and 856 is the first id seed that meets the condition) and 0 of 12.
CASES = {
    "k144": (dict(), (0, 1), 3, synth.SEED_BASE + 81, 3),     # 9 x 16: a partial third lane group
    "k576": (dict(), (1, 0), 3, synth.SEED_BASE + 82, 856),     # 18 x 32: J = 9
    "k162": (LITERAL, (0, 1), 2, synth.SEED_BASE + 83, 2),    # 18 x 9: K no multiple of 64
}


def _cfg(name, batch_size=2, F=None):
  over, grids, f_default = CASES[name][:3]
  cfg = synth.default_config(batch_size=batch_size, use_grids=grids,
                             beam_size=F or f_default, enc_hidden_size=128,
                             dec_hidden_size=128, **over)
  cfg.max_pred_len = 4
  return cfg


def _cells(cfg):
  s = list(cfg.use_grids).index(True)
  return cfg.scene_grids[s][0] * cfg.scene_grids[s][1]


def _random_ids(cfg, seed, T=T_PRED):
  return np.random.default_rng(seed).integers(
      0, _cells(cfg), size=(cfg.batch_size, cfg.beam_size, T)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _case(name):
  cfg = _cfg(name)
  params = synth.make_params(cfg, recurrent_gain=3.0, bias_scale=0.1)
  feed = synth.make_feed(cfg, seed=CASES[name][3], pred_len=T_PRED)
  return cfg, params, feed, _random_ids(cfg, CASES[name][4])


@functools.lru_cache(maxsize=None)
def _oracle(name):
  cfg, params, feed, ids = _case(name)
  return sco.forward(params, cfg, feed, ids)


def _centers(cfg):
  return mf.add_grid(argparse.Namespace(
      grid_strides="2,4", use_grids=[bool(u) for u in cfg.use_grids], scene_h=cfg.scene_h,
      scene_w=cfg.scene_w, video_h=1080, video_w=1920)).scene_grid_centers


def _engine(cfg, params, mode="f16x3"):
  import multiverse_amd._lib as lib
  eng = lib.Engine(cfg, device=0)
  eng.set_params(params)
  eng.set_compute_mode(mode)
  return eng


def _score(eng, feed, ids, lengths=None):
  """One scoring forward with everything it leaves behind: scores + the beam downloads."""
  out = dict(eng.score_futures(feed, ids, lengths))
  beam = eng.download_beam()[0]
  out["logits"], out["grid_reg"], out["ids"] = beam["logits"], beam["grid_reg"], beam["ids"]
  assert beam["logprobs"].tobytes() == out["logprobs"].tobytes()
  return out


def _same(a, b, keys=None):
  return all(a[k].tobytes() == b[k].tobytes() and a[k].shape == b[k].shape
             for k in (keys or a))


def _numpy_ranks(logits, ids):
  return sco.ranks_of(logits, ids)


def _check_parity(name, mode):
  cfg, params, feed, ids = _case(name)
  want = _oracle(name)
  eng = _engine(cfg, params, mode)
  got = _score(eng, feed, ids)
  eng.close()
  N, F, T, K = cfg.batch_size, cfg.beam_size, T_PRED, _cells(cfg)
  assert got["logits"].shape == (N, F, T, K)
  assert got["step_logprobs"].shape == got["ranks"].shape == (N, F, T)
  assert got["logprobs"].shape == (N, F) and got["ranks"].dtype == np.int32
  assert (got["ids"] == ids).all()                       # the given ids come back
  d_logits = float(np.abs(got["logits"] - want["logits"]).max())
  d_reg = float(np.abs(got["grid_reg"] - want["grid_reg"]).max())
  d_step = float(np.abs(got["step_logprobs"] - want["step_logprobs"]).max())
  d_lp = float(np.abs(got["logprobs"] - want["logprobs"]).max())
  print("%s/%s: max|dlogits| %.3g max|dreg| %.3g max|dstep_lp| %.3g max|dlogprob| %.3g"
        % (name, mode, d_logits, d_reg, d_step, d_lp))
  assert d_logits < TOL and d_reg < TOL
  assert d_step < TOL and d_lp < TOL * T
  # ranks: exact given the engine's own logits ...
  assert (got["ranks"] == _numpy_ranks(got["logits"], ids)).all()
  # ... and the oracle's wherever its logits separate the given cell by the parity bar
  close = want["gap"] < TOL
  print("  %d of %d (row, step) pairs with a logit gap below 1e-4; smallest gap %.3g"
        % (int(close.sum()), N * F * T, want["gap"].min()))
  assert int(close.sum()) * 4 <= N * F * T
  assert (got["ranks"][~close] == want["ranks"][~close]).all()


@pytest.mark.parametrize("mode", ["f32", "f16x3"])
@pytest.mark.parametrize("name", ["k144", "k576"])
def test_parity_with_the_oracle(built_lib, name, mode):
  _check_parity(name, mode)


def test_grid_of_162_cells(built_lib):
  """A literal 18 x 9 grid: K = 162 is no multiple of the wave (two full lane groups + 34)."""
  _check_parity("k162", "f16x3")


@functools.lru_cache(maxsize=None)
def _runs():
  """The forwards of the sampler / graph / resident tests, on ONE engine (9 x 16, N = 2)."""
  cfg, params, feed, ids_a = _case("k144")
  ids_b = _random_ids(cfg, 77)
  eng = _engine(cfg, params)
  eng.set_grid_centers(_centers(cfg))
  runs = {}
  eng.set_sampling(TEMP, SEED)
  runs["sampled0"] = dict(eng.forward_beam(feed)[0])
  runs["rescored"] = _score(eng, feed, runs["sampled0"]["ids"])   # sampling stays on, unused
  runs["sampled1"] = dict(eng.forward_beam(feed)[0])
  eng.clear_sampling()
  runs["a"] = _score(eng, feed, ids_a)
  runs["trajs"] = {co: eng.decode_trajectories(center_only=co) for co in (False, True)}
  runs["beam_ids"] = eng.beam_ids()
  runs["b"] = _score(eng, feed, ids_b)
  # the resident path
  eng.upload(feed)
  eng.upload_score_futures(ids_a)
  eng.run_score_resident()
  runs["resident"] = dict(eng.scores())
  lens = np.asarray([[3, 1, 0], [2, 2, 1]], dtype=np.int32)
  runs["ragged"] = _score(eng, feed, ids_a, lens)
  eng.set_graph_mode(True)
  for key, ids in (("ga", ids_a), ("gb", ids_b), ("ga2", ids_a)):
    runs[key] = _score(eng, feed, ids)
  runs["g_ragged"] = _score(eng, feed, ids_a, lens)
  runs["ga3"] = _score(eng, feed, ids_a)                  # the graph again after an eager run
  eng.set_graph_mode(False)
  eng.close()
  return cfg, feed, ids_a, runs


def test_scoring_the_sampler_s_ids_is_the_sampler_bitwise(built_lib):
  _, _, _, r = _runs()
  s0, sc = r["sampled0"], r["rescored"]
  assert (sc["ids"] == s0["ids"]).all()
  for k in ("logprobs", "logits", "grid_reg"):
    assert sc[k].tobytes() == s0[k].tobytes(), k
  acc = np.zeros_like(sc["logprobs"])
  for t in range(T_PRED):                                  # float32, in step order
    acc = (acc + sc["step_logprobs"][:, :, t]).astype(np.float32)
  assert acc.tobytes() == sc["logprobs"].tobytes()
  assert (sc["ranks"] == _numpy_ranks(sc["logits"], sc["ids"])).all()
  # scoring is not sticky and leaves the sampler alone
  assert _same(r["sampled1"], s0)


def test_graph_mode_scores_the_latest_upload(built_lib):
  _, _, _, r = _runs()
  assert not (r["a"]["step_logprobs"] == r["b"]["step_logprobs"]).all()
  assert _same(r["ga"], r["a"]) and _same(r["gb"], r["b"]) and _same(r["ga2"], r["a"])
  assert _same(r["g_ragged"], r["ragged"]) and _same(r["ga3"], r["a"])


def test_resident_path_and_decode_calls(built_lib):
  cfg, _, ids_a, r = _runs()
  a = r["a"]
  assert _same(r["resident"], a, keys=("step_logprobs", "logprobs", "ranks"))
  ids, lp = r["beam_ids"]
  assert (ids == ids_a).all() and lp.tobytes() == a["logprobs"].tobytes()
  N, F, K = cfg.batch_size, cfg.beam_size, _cells(cfg)
  s = list(cfg.use_grids).index(True)
  centers = np.asarray(_centers(cfg)[s], dtype=np.float64).reshape(K, 2)
  reg = a["grid_reg"].reshape(N, T_PRED, K, 2)
  for center_only in (False, True):
    want = np.zeros((N, F, T_PRED, 2), dtype=np.float64)
    for n in range(N):
      for f in range(F):
        for t in range(T_PRED):
          k = int(ids_a[n, f, t])
          want[n, f, t] = centers[k] if center_only else \
              centers[k] + reg[n, t, k].astype(np.float64)
    dev = r["trajs"][center_only]
    assert dev.dtype == np.float64 and dev.shape == want.shape
    assert (dev == want).all()


def test_per_future_lengths_are_bitwise_their_uniform_forwards(built_lib):
  lens = np.asarray([[3, 1, 0], [2, 2, 1], [0, 0, 0]], dtype=np.int32)
  cfg = _cfg("k144", batch_size=3)
  K = _cells(cfg)
  params = synth.make_params(cfg, recurrent_gain=3.0, bias_scale=0.1)
  feed = synth.make_feed(cfg, seed=synth.SEED_BASE + 84, pred_len=T_PRED)
  ids = _random_ids(cfg, 5)
  eng = _engine(cfg, params)
  eng.set_grid_centers(_centers(cfg))
  rag = _score(eng, feed, ids, lens)
  rag_rows = eng.last_forward_gate_rows()
  rag["trajs"] = eng.decode_trajectories()
  junk = ids.copy()                                        # garbage past the lengths
  for n in range(3):
    for f in range(3):
      junk[n, f, lens[n, f]:] = [-7, K + 5, -7][:T_PRED - lens[n, f]]
  rag_junk = _score(eng, feed, junk, lens)
  uni, uni_rows = {}, {}
  for L in (3, 2, 1):
    uni[L] = _score(eng, dict(feed, pred_length=L), np.ascontiguousarray(ids[:, :, :L]))
    uni_rows[L] = eng.last_forward_gate_rows()
    uni[L]["trajs"] = eng.decode_trajectories()
  eng.close()
  assert _same(rag_junk, {k: rag[k] for k in rag_junk})
  for n in range(3):
    Ln = int(lens[n].max())
    assert (rag["grid_reg"][n, Ln:] == 0).all()
    if Ln:
      assert rag["grid_reg"][n, :Ln].tobytes() == \
          np.ascontiguousarray(uni[Ln]["grid_reg"][n]).tobytes(), n
    for f in range(3):
      L = int(lens[n, f])
      assert (rag["step_logprobs"][n, f, L:] == 0).all() and (rag["ranks"][n, f, L:] == -1).all()
      assert (rag["logits"][n, f, L:] == 0).all() and (rag["ids"][n, f, L:] == -1).all()
      assert (rag["trajs"][n, f, L:] == 0).all()
      if not L:
        assert rag["logprobs"][n, f] == 0
        continue
      assert (rag["ids"][n, f, :L] == ids[n, f, :L]).all()
      for k in ("step_logprobs", "ranks", "logits", "trajs"):
        assert rag[k][n, f, :L].tobytes() == \
            np.ascontiguousarray(uni[L][k][n, f]).tobytes(), (n, f, k)
      assert rag["logprobs"][n, f].tobytes() == uni[L]["logprobs"][n, f].tobytes(), (n, f)
  print("gate rows: per-future lengths %d, uniform %d" % (rag_rows, uni_rows[3]))
  assert rag_rows < uni_rows[3]


def test_errors_name_their_cause(built_lib):
  lib = built_lib
  cfg, params, feed, ids = _case("k144")
  K = _cells(cfg)
  greedy = synth.default_config(batch_size=2, use_grids=(0, 1), enc_hidden_size=128,
                                dec_hidden_size=128)
  greedy.max_pred_len = 4
  geng = lib.Engine(greedy, device=0)
  geng.set_params(synth.make_params(greedy, recurrent_gain=3.0, bias_scale=0.1))
  with pytest.raises(lib.MvError) as err:
    geng.score_futures(feed, ids[:, :1])
  assert "beam_size 1" in str(err.value)
  geng.close()
  single = _cfg("k144")
  single.use_single_decoder = True
  seng = lib.Engine(single, device=0)
  seng.set_params(synth.make_params(single, recurrent_gain=3.0, bias_scale=0.1))
  with pytest.raises(lib.MvError) as err:
    seng.score_futures(feed, ids)
  assert "use_single_decoder" in str(err.value)
  seng.close()
  eng = _engine(cfg, params)
  with pytest.raises(lib.MvError) as err:
    eng.run_score_resident()
  assert "no inputs uploaded" in str(err.value)
  eng.upload(feed)
  with pytest.raises(lib.MvError) as err:
    eng.run_score_resident()
  assert "no futures uploaded" in str(err.value)
  bad = ids.copy()
  bad[1, 2, 1] = K
  with pytest.raises(lib.MvError) as err:
    eng.score_futures(feed, bad)
  assert "n=1, f=2, t=1" in str(err.value) and "out of range" in str(err.value)
  eng.score_futures(feed, bad, [[3, 3, 3], [3, 3, 1]])    # the same id past its length: unread
  with pytest.raises(lib.MvError) as err:
    eng.score_futures(feed, ids, [[3, 3, 3], [3, T_PRED + 1, 3]])
  assert "lengths[1, 1] = 4" in str(err.value)
  with pytest.raises(lib.MvError) as err:
    eng.score_futures(dict(feed, pred_lengths=[3, 2]), ids)
  assert "mv_set_pred_lengths" in str(err.value)
  eng.score_futures(feed, ids)                            # (the feed cleared the lengths)
  with pytest.raises(lib.MvError) as err:
    eng.beam_occupancy()
  assert "not a predictive mixture" in str(err.value)
  # another pred_len invalidates the uploaded futures
  eng.upload(dict(feed, pred_length=2))
  with pytest.raises(lib.MvError) as err:
    eng.run_score_resident()
  assert "upload the futures again" in str(err.value)
  # not sticky: the next beam forward and its occupancy map, and training, are unaffected
  eng.forward_beam(feed)
  eng.beam_occupancy()
  with pytest.raises(lib.MvError) as err:
    eng.scores()
  assert "not a scoring one" in str(err.value)
  eng.score_futures(feed, ids)
  with pytest.raises(lib.MvError) as err:                 # refused for its own reason only
    eng.train_step()
  assert "mv_train_init has not been called" in str(err.value)
  eng.close()


def test_script_score_gt(built_lib, tmp_path):
  ds = mf_fixture.make_dataset(str(tmp_path / "fp"), n_traj=4)
  cfg = synth.default_config(batch_size=1, use_grids=(0, 1), beam_size=2)
  params = synth.make_params(cfg, seed=synth.SEED_BASE + 31, recurrent_gain=3.0,
                             bias_scale=0.1)
  model_dir = str(tmp_path / "model")
  tf_checkpoint.save_checkpoint(os.path.join(model_dir, "save-best"), params, global_step=100)
  files = [str(tmp_path / n) for n in ("two.p", "one.p")]
  # num_out 2: the samples with three futures take two rows
  tail = ["--num_out", "2", "--emb_size", "32", "--use_grids", "0,1", "--use_gnn",
          "--use_scene_enc", "--scene_feat_path", ds["scene_feat_path"],
          "--scene_id2name", ds["scene_id2name"], "--obs_length", "8"]
  head = [ds["traj_path"], ds["multifuture_path"], model_dir, str(tmp_path / "unused.p")]
  printed = io.StringIO()
  with contextlib.redirect_stdout(printed):
    cli.multifuture_inference_main(head + tail + ["--batch_size", "2", "--score_gt", files[0]])
  cli.multifuture_inference_main(head + tail + ["--batch_size", "1", "--score_gt", files[1]])
  assert not os.path.exists(head[3])                      # scoring replaces the decode
  two, one = (pickle.load(open(f, "rb")) for f in files)
  gt = mf.load_gt(ds["multifuture_path"], ds["traj_ids"])
  assert sorted(two) == sorted(one) == sorted(ds["traj_ids"])
  args = mf.add_grid(argparse.Namespace(grid_strides="2,4", use_grids="0,1", scene_h=36,
                                        scene_w=64, video_h=1080, video_w=1920))
  for t in gt:
    assert list(two[t]) == list(one[t]) == list(gt[t])
    cells, lengths = mf.futures_to_grid_ids(args, gt, t, 1)
    for j, fid in enumerate(gt[t]):
      a, b = two[t][fid], one[t][fid]
      L = len(gt[t][fid]["x_agent_traj"])
      assert a["step_logprobs"].shape == a["ranks"].shape == (L,) and L == lengths[j]
      for k in ("logprob", "step_logprobs", "ranks"):
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (t, fid, k)
      assert (a["step_logprobs"] < 0).all() and (a["ranks"] >= 0).all()
      assert (a["ranks"] < 9 * 16).all()
  want = io.StringIO()
  with contextlib.redirect_stdout(want):
    cli.print_exact_nll(mf.eval_exact_nll(two))
  assert printed.getvalue().endswith(want.getvalue()) and "exact NLL:" in want.getvalue()
