# coding=utf-8
"""GPU: sampling WITHOUT replacement on beam handles (mv_set_sampling_mode 1): stochastic beam
search, B = beam_size DISTINCT futures per row that are still a sample of the model, each with
its exact log-probability and its perturbed score.  The reference has none; the step is defined
in include/multiverse_hip.h and restated by tests/sbs_oracle.py."""
import argparse
import functools
import os
import pickle

import numpy as np
import pytest

from multiverse_amd import cli, multifuture as mf, synth, tf_checkpoint

import mf_fixture
import sbs_oracle as sbs
from sampling_oracle import row_seed

pytestmark = pytest.mark.gpu

TOL = 1e-4            # the project's parity bar on logits and offsets
T_PRED = 3
TEMP, SEED = 0.7, 4321
LITERAL = dict(scene_h=72, scene_w=36, scene_grids=[(36, 18), (18, 9)])

# name -> (config overrides, used grid, feed seed).  N = 2, B = 3.  The feed seeds were picked
# on the CPU with the oracle alone: no (row, step) of these feeds has a gap below 1e-4 among the
# B + 1 largest perturbed scores of the float64 restatement (the cap is a quarter).
CASES = {
    "k144": (dict(), (0, 1), synth.SEED_BASE + 91),     # 9 x 16: a partial third lane group
    "k576": (dict(), (1, 0), synth.SEED_BASE + 92),     # 18 x 32: J = 9
    "k162": (LITERAL, (0, 1), synth.SEED_BASE + 93),    # 18 x 9: K no multiple of 64
}
B_DEFAULT = 3


def _cfg(name, batch_size=2, B=B_DEFAULT):
  over, grids, _ = CASES[name]
  cfg = synth.default_config(batch_size=batch_size, use_grids=grids, beam_size=B,
                             enc_hidden_size=128, dec_hidden_size=128, **over)
  cfg.max_pred_len = 4
  return cfg


@functools.lru_cache(maxsize=None)
def _case(name):
  cfg = _cfg(name)
  params = synth.make_params(cfg, recurrent_gain=3.0, bias_scale=0.1)
  feed = synth.make_feed(cfg, seed=CASES[name][2], pred_len=T_PRED)
  return cfg, params, feed


@functools.lru_cache(maxsize=None)
def _oracle(name):
  cfg, params, feed = _case(name)
  return sbs.forward(params, cfg, feed, temperature=TEMP, seed=SEED)


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
    eng.set_sampling(*sampling, without_replacement=True)
  return eng


def _same(a, b):
  return sorted(a) == sorted(b) and \
      all(a[k].tobytes() == b[k].tobytes() and a[k].shape == b[k].shape for k in a)


def _check_invariants(arrs, K):
  ids, g = arrs["ids"], arrs["gumbels"]
  N, B, _ = ids.shape
  assert (ids >= 0).all() and (ids < K).all()
  for n in range(N):
    assert len({tuple(ids[n, b]) for b in range(B)}) == B, (n, ids[n])
  assert (g[:, 0] == 0).all() and (np.diff(g, axis=1) <= 0).all()


# ---------------------------------------------------------------- 1. the step op

# (N, B, K): J = 3 / 9 / 16, partial lane groups, K no multiple of 64
STEP_SHAPES = [(3, 3, 70), (2, 4, 144), (2, 3, 162), (2, 3, 576), (1, 2, 792), (1, 2, 1024)]


def _step_inputs(shape, t, temp):
  """Random inputs of one step, prev_gumbel sorted and <= 0.  The generator seeds were checked
  on the CPU with the oracle alone: no row of these inputs has a gap below 1e-4, and no winner
  sits so close under its parent's maximum (d = g - Z of a few 1e-3 at |g| of 5 and more, where
  the float32 rounding of g alone moves log(-expm1(d)) by ulp(g) / |d|) that the float32
  restatement itself leaves the 1e-4 bar: 6.6e-6 over the table."""
  N, B, K = shape
  rng = np.random.RandomState(2000 + 7 * K + 3 * t + int(temp * 10))
  logits = (2.0 * rng.randn(N, B, K)).astype(np.float32)
  prev_g = (-np.sort(rng.rand(N, B) * 3, axis=1)).astype(np.float32)
  prev_phi = (-rng.rand(N, B) * 6).astype(np.float32)
  prev_lp = (-rng.rand(N, B) * 6).astype(np.float32)
  return logits, prev_phi, prev_lp, prev_g


STEP_SEED = 99


@functools.lru_cache(maxsize=None)
def _restatement_error():
  """The largest |float32 restatement - float64 restatement| of new_gumbel over the whole table
  of step cases (same inputs, same winners), computed once.  Per case it is a maximum over B
  winners only, and exactly 0 whenever every winner is its parent's best child (whose score is
  the parent's bit for bit), so one case alone does not measure the float32 error of the
  formula; the table as a whole does."""
  worst = 0.0
  for shape in STEP_SHAPES:
    for t in (0, 2):
      for temp in (1.0, 0.7):
        inputs = _step_inputs(shape, t, temp)
        a, b = (sbs.step(*inputs, t, temp, STEP_SEED, dtype=d) for d in (np.float32, np.float64))
        assert (a["ids"] == b["ids"]).all() and (a["parents"] == b["parents"]).all()
        worst = max(worst, float(np.abs(a["new_g"].astype(np.float64) - b["new_g"]).max()))
  return worst


@pytest.mark.parametrize("temp", [1.0, 0.7])
@pytest.mark.parametrize("t", [0, 2])
@pytest.mark.parametrize("shape", STEP_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_step_op_against_the_restatement(built_lib, shape, t, temp):
  N, B, K = shape
  seed = STEP_SEED
  inputs = _step_inputs(shape, t, temp)
  logits, prev_phi, prev_lp, prev_g = inputs
  phi, lp, g, ids, parents = built_lib.op_sbs_step(logits, prev_phi, prev_lp, prev_g, t, temp,
                                                   seed)
  want = sbs.step(logits, prev_phi, prev_lp, prev_g, t, temp, seed, dtype=np.float64)
  # device and numpy libm differ by a few ulp per transcendental, four of them are chained
  e32 = _restatement_error()
  tol = 4 * e32
  # new_gumbel[:, 0] is the largest parent score (the root's at t == 0), bit for bit
  top = prev_g[:, 0] if t == 0 else prev_g.max(axis=1)
  assert g[:, 0].tobytes() == top.tobytes()
  assert (np.diff(g, axis=1) <= 0).all()
  assert (parents >= 0).all() and (parents < (1 if t == 0 else B)).all()
  assert (ids >= 0).all() and (ids < K).all()
  pairs = parents.astype(np.int64) * K + ids
  assert all(len(set(row)) == B for row in pairs.tolist())
  tied = want["gap"] < sbs.GAP_BAR
  assert tied.sum() * 4 <= N
  rows = np.arange(N)[:, None]
  for n in np.nonzero(~tied)[0]:
    assert (ids[n] == want["ids"][n]).all() and (parents[n] == want["parents"][n]).all(), n
  dg = float(np.abs(g - want["new_g"])[~tied].max()) if (~tied).any() else 0.0
  # LP and phi of the device's own winners: prev[parent] + the restatement's lp / q
  w_lp = prev_lp.astype(np.float64)[rows, parents] + want["lp"][rows, parents, ids]
  w_phi = prev_phi.astype(np.float64)[rows, parents] + want["q"][rows, parents, ids]
  dlp, dphi = float(np.abs(lp - w_lp).max()), float(np.abs(phi - w_phi).max())
  print("%s t=%d tau=%.1f: float32 restatement vs float64 %.3g -> bar %.3g; device: gumbel "
        "%.3g, logprob %.3g, phi %.3g; smallest gap %.3g"
        % (shape, t, temp, e32, tol, dg, dlp, dphi, want["gap"].min()))
  assert tol < 1e-4
  assert dg <= tol and dlp <= tol and dphi <= tol


# ---------------------------------------------------------------- 2. forward parity

def _check_parity(name, mode):
  cfg, params, feed = _case(name)
  want = _oracle(name)
  eng = _engine(cfg, params, mode)
  arrs, s = eng.forward_beam(feed)
  eng.close()
  N, B, T = cfg.batch_size, cfg.beam_size, T_PRED
  K = cfg.scene_grids[s][0] * cfg.scene_grids[s][1]
  assert arrs["logits"].shape == (N, B, T, K) and arrs["ids"].shape == (N, B, T)
  assert arrs["logprobs"].shape == arrs["gumbels"].shape == (N, B)
  _check_invariants(arrs, K)
  upto = sbs.compared_steps(want["gap"])                   # row n: ids compared on steps [0, upto)
  cut = int((T - upto).sum())
  print("%s/%s: %d of %d (row, step) pairs behind a gap below 1e-4; smallest gap %.3g"
        % (name, mode, cut, N * T, want["gap"].min()))
  assert cut * 4 <= N * T
  for n in range(N):
    u = int(upto[n])
    if u == T:
      assert (arrs["ids"][n] == want["ids"][n]).all(), n
      d = float(np.abs(arrs["logits"][n] - want["logits"][n]).max())
      dl = float(np.abs(arrs["logprobs"][n] - want["logprobs"][n]).max())
      dg = float(np.abs(arrs["gumbels"][n] - want["gumbels"][n]).max())
      print("  row %d: max|dlogits| %.3g, |dlogprob| %.3g, |dgumbel| %.3g" % (n, d, dl, dg))
      assert d < TOL and dl < TOL * T and dg < TOL
      continue
    # behind a near tie the engine may keep another set: each of its futures must still
    # descend from a slot the oracle held after step u - 1, with that slot's logits
    paths = {} if u == 0 else {tuple(sbs.trace_back(want, n, j, u)[0]): j for j in range(B)}
    for b in range(B):
      j = 0 if u == 0 else paths.get(tuple(arrs["ids"][n, b, :u]))
      assert j is not None, (n, b)
      slots = sbs.trace_back(want, n, j, u)[1] if u else []
      for t in range(u):
        assert np.abs(arrs["logits"][n, b, t] - want["step_logits"][t][n, slots[t]]).max() < TOL
      assert np.abs(arrs["logits"][n, b, u] - want["step_logits"][u][n, j]).max() < TOL
  dr = float(np.abs(arrs["grid_reg"] - want["grid_reg"]).max())
  print("  max|dreg| %.3g" % dr)
  assert dr < TOL
  assert (arrs["best_beam"].reshape(N, T, K) == arrs["logits"][:, 0]).all()   # slot 0


@pytest.mark.parametrize("mode", ["f32", "f16x3"])
@pytest.mark.parametrize("name", ["k144", "k576"])
def test_parity_with_the_oracle(built_lib, name, mode):
  _check_parity(name, mode)


def test_grid_of_162_cells(built_lib):
  """A literal 18 x 9 grid: K = 162 is no multiple of the wave (two full lane groups + 34)."""
  _check_parity("k162", "f16x3")


# ---------------------------------------------------------------- 3. invariants and the scorer

@pytest.mark.parametrize("temp", [1.0, 0.7])
def test_invariants_and_the_scorer_returns_the_logprobs(built_lib, temp):
  """LP is untempered and accumulated in step order from the terms of step_row_log_softmax, as
  the scorer's: scoring the drawn ids returns the logprobs bit for bit at any temperature."""
  cfg, params, feed = _case("k144")
  eng = _engine(cfg, params, sampling=(temp, SEED))
  arrs = dict(eng.forward_beam(feed)[0])
  _check_invariants(arrs, 144)
  scored = eng.score_futures(feed, arrs["ids"])
  again = dict(eng.forward_beam(feed)[0])                  # scoring is not sticky
  eng.close()
  assert scored["logprobs"].tobytes() == arrs["logprobs"].tobytes()
  assert (scored["logprobs"] < 0).all()
  assert _same(arrs, again)


# ---------------------------------------------------------------- 4. determinism, graph mode

@functools.lru_cache(maxsize=None)
def _runs():
  """The forwards of the determinism / graph / decode tests, on ONE engine (9 x 16, N = 2)."""
  cfg, params, feed = _case("k144")
  eng = _engine(cfg, params)
  eng.set_grid_centers(_centers(cfg))
  fwd = lambda: dict(eng.forward_beam(feed)[0])
  runs = {}
  runs["a0"] = fwd()
  runs["trajs"] = {co: eng.decode_trajectories(center_only=co) for co in (False, True)}
  runs["occupancy"] = eng.beam_occupancy()
  runs["beam_ids"] = eng.beam_ids()
  runs["decoded"] = eng.forward_beam_decoded(feed)[0]
  runs["a1"] = fwd()
  eng.set_sampling(TEMP, SEED + 1, without_replacement=True)
  runs["b0"] = fwd()
  eng.set_sampling(2.0, SEED, without_replacement=True)
  runs["hot"] = fwd()
  eng.set_sampling(TEMP, SEED)                             # mode 0: independent draws
  runs["iid"] = fwd()
  eng.clear_sampling()
  runs["beam"] = fwd()
  eng.set_graph_mode(True)
  for key, seed in (("ga", SEED), ("gb", SEED + 1), ("ga2", SEED)):
    eng.set_sampling(TEMP, seed, without_replacement=True)
    runs[key] = fwd()
  eng.set_sampling(2.0, SEED, without_replacement=True)    # a replayed graph follows tau
  runs["g_hot"] = fwd()
  # mode 0 -> 1 -> sampling off (beam) -> 1 on ONE handle, every forward a graph of its kind
  eng.set_sampling(TEMP, SEED)
  runs["g_iid"] = fwd()
  eng.set_sampling(TEMP, SEED, without_replacement=True)
  runs["g_wor"] = fwd()
  eng.clear_sampling()
  runs["g_beam"] = fwd()
  eng.set_sampling(TEMP, SEED, without_replacement=True)
  runs["g_wor2"] = fwd()
  eng.close()
  return cfg, feed, runs


def test_determinism_and_seeds(built_lib):
  _, _, r = _runs()
  assert "gumbels" in r["a0"] and "gumbels" not in r["iid"] and "gumbels" not in r["beam"]
  assert _same(r["a0"], r["a1"])
  assert not (r["a0"]["ids"] == r["b0"]["ids"]).all()
  assert not (r["a0"]["ids"] == r["hot"]["ids"]).all()
  assert not (r["a0"]["ids"] == r["iid"]["ids"]).all()
  assert not (r["a0"]["ids"] == r["beam"]["ids"]).all()


def test_graph_mode_follows_seed_temperature_and_mode(built_lib):
  _, _, r = _runs()
  assert _same(r["ga"], r["a0"]) and _same(r["gb"], r["b0"]) and _same(r["ga2"], r["a0"])
  assert _same(r["g_hot"], r["hot"])
  assert _same(r["g_iid"], r["iid"]) and _same(r["g_wor"], r["a0"])
  assert _same(r["g_beam"], r["beam"]) and _same(r["g_wor2"], r["a0"])


# ---------------------------------------------------------------- 5. batch and width

def test_rows_do_not_depend_on_the_batch(built_lib):
  cfg3 = _cfg("k144", batch_size=3)
  params = synth.make_params(cfg3, recurrent_gain=3.0, bias_scale=0.1)
  feed3 = synth.make_feed(cfg3, seed=synth.SEED_BASE + 94, pred_len=T_PRED)
  eng = _engine(cfg3, params)
  a3, _ = eng.forward_beam(feed3)
  eng.close()
  eng1 = _engine(_cfg("k144", batch_size=1), params)
  for n in range(3):
    feed1 = dict(feed3, obs_scene=feed3["obs_scene"][n:n + 1],
                 grid_obs_labels=[a[n:n + 1] for a in feed3["grid_obs_labels"]],
                 grid_obs_regress=[a[n:n + 1] for a in feed3["grid_obs_regress"]])
    eng1.set_sampling(TEMP, row_seed(SEED, n), without_replacement=True)
    a1, _ = eng1.forward_beam(feed1)
    for k in ("ids", "logits", "logprobs", "gumbels", "grid_reg", "best_beam"):
      assert a1[k][0].tobytes() == a3[k][n].tobytes(), (n, k)
  eng1.close()


def test_a_narrower_handle_draws_the_first_futures_of_a_wider_one(built_lib):
  _, params, feed = _case("k144")
  outs = {}
  for B in (2, 3, 4):
    eng = _engine(_cfg("k144", B=B), params)
    outs[B] = eng.forward_beam(feed)[0]
    eng.close()
  for B in (2, 3):
    for k in ("ids", "logits", "logprobs", "gumbels"):
      assert outs[B][k].tobytes() == np.ascontiguousarray(outs[4][k][:, :B]).tobytes(), (B, k)
    assert outs[B]["grid_reg"].tobytes() == outs[4]["grid_reg"].tobytes()


# ---------------------------------------------------------------- 6. ragged lengths

@pytest.mark.parametrize("lens", [(3, 1, 0), (2, 3, 1)])
def test_ragged_rows_are_bitwise_their_uniform_forwards(built_lib, lens):
  cfg = _cfg("k144", batch_size=3)
  params = synth.make_params(cfg, recurrent_gain=3.0, bias_scale=0.1)
  feed = synth.make_feed(cfg, seed=synth.SEED_BASE + 94, pred_len=T_PRED)
  eng = _engine(cfg, params)
  rag = dict(eng.forward_beam(dict(feed, pred_lengths=list(lens)))[0])
  rag_rows = eng.last_forward_gate_rows()
  uni = {L: dict(eng.forward_beam(dict(feed, pred_length=L))[0]) for L in set(lens) if L}
  eng.clear_sampling()
  eng.forward_beam(dict(feed, pred_lengths=list(lens)))
  beam_rows = eng.last_forward_gate_rows()
  eng.close()
  axis = {"ids": 1, "logits": 1, "best_beam": 0, "grid_reg": 0}
  for n, L in enumerate(lens):
    for k, ax in axis.items():
      a = np.moveaxis(rag[k][n], ax, 0)
      assert (a[L:] == (-1 if k == "ids" else 0)).all(), (n, k)
      if L:
        want = np.moveaxis(uni[L][k][n], ax, 0)
        assert a[:L].tobytes() == np.ascontiguousarray(want).tobytes(), (n, k)
    for k in ("logprobs", "gumbels"):
      if L:
        assert rag[k][n].tobytes() == uni[L][k][n].tobytes(), (n, k)
      else:
        assert (rag[k][n] == 0).all(), (n, k)
    assert rag["gumbels"][n, 0] == 0
  assert rag_rows == beam_rows


# ---------------------------------------------------------------- 7. decode calls

def test_decode_calls(built_lib):
  cfg, _, r = _runs()
  arrs = r["a0"]
  N, B = cfg.batch_size, cfg.beam_size
  s = list(cfg.use_grids).index(True)
  ids, lp = r["beam_ids"]
  assert (ids == arrs["ids"]).all() and (lp == arrs["logprobs"]).all()
  dec = r["decoded"]
  assert dec["gumbels"].tobytes() == arrs["gumbels"].tobytes()
  assert (dec["ids"] == arrs["ids"]).all() and (dec["trajs"] == r["trajs"][False]).all()
  for center_only in (False, True):
    args = mf.add_grid(argparse.Namespace(
        grid_strides="2,4", use_grids=[bool(u) for u in cfg.use_grids], scene_h=36, scene_w=64,
        video_h=1080, video_w=1920, greedy=False, center_only=center_only, num_out=B))
    want = np.asarray([mf.decode_trajectories(
        args, None, arrs["grid_reg"][n], (arrs["logits"][n], arrs["ids"][n], arrs["logprobs"][n]),
        T_PRED, s) for n in range(N)])
    dev = r["trajs"][center_only]
    assert dev.dtype == np.float64 and dev.shape == want.shape == (N, B, T_PRED, 2)
    assert (dev == want).all()

  def mixture(dtype):        # sum_b softmax_b(logprobs)[b] * softmax_k(logits[n, b, t, :])
    x = arrs["logits"].astype(dtype)
    e = np.exp(x - x.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    l = arrs["logprobs"].astype(dtype)
    w = np.exp(l - l.max(-1, keepdims=True))
    w = w / w.sum(-1, keepdims=True)
    out = np.zeros_like(p[:, 0])
    for j in range(B):
      out = out + p[:, j] * w[:, j, None, None]
    return out

  exact, ref32 = mixture(np.float64), mixture(np.float32)
  dev = r["occupancy"]
  assert dev.dtype == np.float32 == ref32.dtype and dev.shape == exact.shape
  d_ref = float((np.abs(ref32 - exact) / exact).max())
  d_dev = float((np.abs(dev - exact) / exact).max())
  rows = float(np.abs(dev.astype(np.float64).sum(-1) - 1).max())
  print("beam-weighted mixture: host float32 vs fp64 %.3g, device vs fp64 %.3g (bar %.3g), "
        "rows sum to 1 within %.3g" % (d_ref, d_dev, 4 * d_ref, rows))
  # the bar of test_gpu_multifuture_decode.py for the beam's map against its host formula
  assert d_dev <= 4 * d_ref
  assert rows <= 1e-6
  # not the sampler's 1 / B
  x = arrs["logits"].astype(np.float64)
  e = np.exp(x - x.max(-1, keepdims=True))
  uniform = (e / e.sum(-1, keepdims=True)).mean(axis=1)
  assert np.abs(dev - uniform).max() > 100 * np.abs(dev - exact).max()


# ---------------------------------------------------------------- 8. errors

def test_errors_name_their_cause(built_lib):
  lib = built_lib
  cfg, params, feed = _case("k144")
  greedy = synth.default_config(batch_size=2, use_grids=(0, 1), enc_hidden_size=128,
                                dec_hidden_size=128)
  geng = lib.Engine(greedy, device=0)
  assert geng.lib.mv_set_sampling_mode(geng.handle, 1) != 0
  assert "beam_size 1" in geng.lib.mv_last_error(geng.handle).decode()
  geng.close()
  eng = _engine(cfg, params, sampling=None)
  assert eng.lib.mv_set_sampling_mode(eng.handle, 2) != 0
  assert "mode 2" in eng.lib.mv_last_error(eng.handle).decode()
  # stored while sampling is off: the handle still searches
  assert eng.lib.mv_set_sampling_mode(eng.handle, 1) == 0
  eng.forward_beam(feed)
  with pytest.raises(lib.MvError) as err:
    eng.beam_gumbels()
  assert "beam search" in str(err.value)
  assert eng.lib.mv_set_sampling_mode(eng.handle, 0) == 0
  eng.set_sampling(TEMP, SEED)
  eng.forward_beam(feed)
  with pytest.raises(lib.MvError) as err:
    eng.beam_gumbels()
  assert "independent samples" in str(err.value)
  eng.set_sampling(TEMP, SEED, without_replacement=True)
  for call in (eng.train_init, eng.train_step):
    with pytest.raises(lib.MvError) as err:
      call()
    assert "sampling is on" in str(err.value), call
  eng.close()
  single = _cfg("k144")
  single.use_single_decoder = True
  seng = lib.Engine(single, device=0)
  with pytest.raises(lib.MvError) as err:
    seng.set_sampling(1.0, 0, without_replacement=True)
  assert "use_single_decoder" in str(err.value)
  seng.close()
  # beam_size > K: a 2 x 2 grid cannot be built; the step op carries the same check
  z = np.zeros((1, 5), dtype=np.float32)
  with pytest.raises(lib.MvError) as err:
    lib.op_sbs_step(np.zeros((1, 5, 4), dtype=np.float32), z, z, z, 0)
  assert "beam_size 5 > K = 4" in str(err.value)


# ---------------------------------------------------------------- 9. the script

def test_script_device_decode_equals_host_decode(built_lib, tmp_path):
  ds = mf_fixture.make_dataset(str(tmp_path / "fp"), n_traj=4)
  cfg = synth.default_config(batch_size=1, use_grids=(0, 1), beam_size=3)
  params = synth.make_params(cfg, seed=synth.SEED_BASE + 31, recurrent_gain=3.0,
                             bias_scale=0.1)
  model_dir = str(tmp_path / "model")
  tf_checkpoint.save_checkpoint(os.path.join(model_dir, "save-best"), params, global_step=100)
  files = [str(tmp_path / n) for n in ("host.p", "dev.p", "iid.p")]
  tail = ["--num_out", "3", "--emb_size", "32", "--use_grids", "0,1", "--use_gnn",
          "--use_scene_enc", "--scene_feat_path", ds["scene_feat_path"],
          "--scene_id2name", ds["scene_id2name"], "--obs_length", "8", "--batch_size", "2"]
  head = [ds["traj_path"], ds["multifuture_path"], model_dir]
  sample = ["--sample", "--sample_temperature", "0.9", "--sample_seed", "5"]
  wor = sample + ["--sample_without_replacement"]
  cli.multifuture_inference_main(head + [files[0]] + tail + wor)
  cli.multifuture_inference_main(head + [files[1]] + tail + wor + ["--device_decode"])
  cli.multifuture_inference_main(head + [files[2]] + tail + sample)
  host, dev, iid = (pickle.load(open(f, "rb")) for f in files)
  assert list(host) == list(dev) and len(host) == 4
  for t in host:
    a, b = np.asarray(host[t]), np.asarray(dev[t])
    assert a.shape == b.shape and a.shape[0] == 3 and a.dtype == b.dtype == np.float64
    assert (a == b).all(), t
  assert any(not (np.asarray(host[t]) == np.asarray(iid[t])).all() for t in host)
