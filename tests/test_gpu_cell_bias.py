# coding=utf-8
"""GPU: the cell costs (mv_set_cell_bias): a per-row, per-step, per-cell additive log-potential for
the beam search, the independent sampler and the sampling without replacement, and the occupancy
map after them.  The reference has none; the definition is in include/multiverse_hip.h (DESIGN.md
8.12) and restated by tests/cell_bias_oracle.py on top of the existing restatements.

Shapes, cases, seeds and every bar are those of test_gpu_cell_mask.py (its TOL and its restatement
error); the biases come from the generator seeds below."""
import ctypes
import functools

import numpy as np
import pytest

from multiverse_amd import synth

import cell_bias_oracle as cb
import cell_mask_oracle as cm
import sampling_oracle as so
import sbs_oracle as sbs
import test_gpu_cell_mask as tm
from beam_compare import compare_beams

pytestmark = pytest.mark.gpu

TOL, T_PRED, TEMP, SEED, KINDS = tm.TOL, tm.T_PRED, tm.TEMP, tm.SEED, tm.KINDS
BIAS_SEED = 4300
_case, _cfg, _K, _engine, _same, _half_mask = (tm._case, tm._cfg, tm._K, tm._engine, tm._same,  # pylint: disable=protected-access
                                               tm._half_mask)                                 # pylint: disable=protected-access


def _bias(N, Tm, K, seed=BIAS_SEED, scale=2.0):
  """Costs of a few nats per (row, plane, cell); the planes of a row differ."""
  return (scale * np.random.RandomState(seed + K).randn(N, Tm, K)).astype(np.float32)


def _fwd(eng, feed, bias=None, mask=None):
  """One forward under `bias` / `mask` (None: none) -> its arrays, with the proposal's
  log-probability under "q" where the forward sampled."""
  f = dict(feed)
  if bias is not None:
    f["cell_bias"] = bias
  if mask is not None:
    f["cell_mask"] = mask
  arrs = dict(eng.forward_beam(f)[0])
  if getattr(eng, "_sampling_on", False):
    arrs["q"] = eng.beam_proposal_logprobs()
  return arrs


# ---------------------------------------------------------------- 1. the step ops

STEP_K = tm.STEP_K                            # 70, 144, 162, 576, 1024: J = 3 / 9 / 16
STEP_R, STEP_S, STEP_T, STEP_SEED = tm.STEP_R, tm.STEP_S, tm.STEP_T, tm.STEP_SEED
STEP_N, STEP_B = tm.STEP_N, tm.STEP_B
TIE = tm.TIE                                  # row 0: three exactly equal top values of l + b
BIASES = ("random", "tie", "reverse")
MASKS = (None, "half")
SAMPLE_LIMITS = tm.SAMPLE_LIMITS              # (0, 1.0) and (8, 0.9)
TEMPS = (1.0, 0.7)


def _step_inputs(K, kind, samples):
  """logits [STEP_R, K] and bias [samples, K] of the named kind.  "tie": the three cells of TIE
  have different logits and the same l + b, exactly, above the rest of row 0.  "reverse": the 16
  best cells of each sample's first row get a cost that reverses their order, so that the limits'
  kept set by w is not the one by l."""
  rng = np.random.RandomState(5200 + 7 * K)
  logits = (4.0 * rng.randn(STEP_R, K)).astype(np.float32)
  per = STEP_R // samples
  bias = np.zeros((samples, K), dtype=np.float32)
  if kind == "random":
    bias = (2.0 * rng.randn(samples, K)).astype(np.float32)
  elif kind == "tie":
    base = np.float32(np.ceil(logits[0].max()))
    logits[0, list(TIE)] = base + np.array([0.5, 1.0, 1.5], dtype=np.float32)
    bias[0, list(TIE)] = np.array([1.5, 1.0, 0.5], dtype=np.float32)
  elif kind == "reverse":
    for n in range(samples):
      top = np.argsort(-logits[n * per])[:16]
      bias[n, top] = -2.0 * (logits[n * per, top] - logits[n * per, top[-1]])
  return logits, bias


def _step_mask(K, mask, samples):
  return None if mask is None else tm._step_mask(K, mask, samples)   # pylint: disable=protected-access


def test_the_step_inputs_are_what_they_are_named():
  for K in STEP_K:
    logits, bias = _step_inputs(K, "tie", STEP_R // STEP_S)
    w = cb.proposal_w(logits, np.repeat(bias, STEP_S, 0), 1.0)
    assert len(set(w[0, list(TIE)])) == 1 and len(set(logits[0, list(TIE)])) == 3
    assert (np.sort(w[0])[-3:] == w[0, TIE[0]]).all() and np.sort(w[0])[-4] < w[0, TIE[0]]
    logits, bias = _step_inputs(K, "reverse", STEP_R // STEP_S)
    ones = np.ones((STEP_R // STEP_S, K))
    by_w = cb.sample_step(logits, STEP_S, STEP_T, None, bias, 1.0, STEP_SEED, 8, 1.0)["keep"]
    by_l = cm.sample_step(logits, STEP_S, STEP_T, ones, 1.0, STEP_SEED, 8, 1.0)["keep"]
    assert (by_w != by_l).any(), K


@pytest.mark.parametrize("K", STEP_K)
def test_sample_step_op_against_the_restatement(built_lib, K):
  e32 = tm._restatement_error()            # pylint: disable=protected-access
  tol = 4 * e32                            # the bar of test_gpu_cell_mask.py for this op
  assert tol < 1e-4
  rows = np.arange(STEP_R)
  samples = STEP_R // STEP_S
  worst_lp = worst_q = 0.0
  for kind in BIASES:
    logits, bias = _step_inputs(K, kind, samples)
    for mask in MASKS:
      allowed = _step_mask(K, mask, samples)
      arows = np.ones((STEP_R, K), dtype=bool) if allowed is None else \
          np.repeat(allowed != 0, STEP_S, axis=0)
      for limits in SAMPLE_LIMITS:
        for temp in TEMPS:
          what = (K, kind, mask, limits, temp)
          ids, lp, qlp, keep = built_lib.op_sample_step(logits, STEP_S, STEP_T, temp, STEP_SEED,
                                                        limits[0], limits[1], 1, allowed=allowed,
                                                        bias=bias)
          want = cb.sample_step(logits, STEP_S, STEP_T, allowed, bias, temp, STEP_SEED,
                                limits[0], limits[1], 1, dtype=np.float64)
          band = want["wide"] & ~want["tight"]
          assert (keep == want["tight"])[~band].all(), what
          assert not (keep & ~arows).any(), what             # keep is a subset of A
          assert keep[rows, ids].all(), what                 # the drawn cell is a kept cell
          if limits == (0, 1.0):
            assert (keep == arows).all(), what               # no limit: the kept set IS A
          if kind == "tie" and temp == 1.0 and mask is None:
            assert len(set(keep[0, list(TIE)])) == 1, what   # equal w: kept or dropped together
          cmp = want["compared"]
          assert (~cmp).sum() * 4 <= STEP_R, what
          assert (ids[cmp] == want["ids"][cmp]).all(), what
          lp64 = sbs.log_softmax(logits.astype(np.float64))  # the model's, over ALL cells
          dlp = float(np.abs(lp - lp64[rows, ids]).max())
          sure = ~band.any(-1)
          assert np.isfinite(qlp).all() and (qlp <= 0).all(), what
          dq = float(np.abs(qlp - want["q"][rows, ids])[sure].max()) if sure.any() else 0.0
          worst_lp, worst_q = max(worst_lp, dlp), max(worst_q, dq)
          assert dlp <= tol and dq <= tol, (what, dlp, dq, tol)
    # a zero bias is the masked / the plain op, bitwise
    zero = np.zeros_like(bias)
    for mask in MASKS:
      allowed = _step_mask(K, mask, samples)
      for limits in SAMPLE_LIMITS:
        for temp in TEMPS:
          got = built_lib.op_sample_step(logits, STEP_S, STEP_T, temp, STEP_SEED, limits[0],
                                         limits[1], 1, allowed=allowed, bias=zero)
          plain = built_lib.op_sample_step(logits, STEP_S, STEP_T, temp, STEP_SEED, limits[0],
                                           limits[1], 1, allowed=allowed)
          for a, b in zip(got, plain):
            assert a.tobytes() == b.tobytes(), (K, kind, mask, limits, temp)
  print("K=%d: float32 restatement vs float64 %.3g -> bar %.3g; device: logprob %.3g, "
        "proposal %.3g" % (K, e32, tol, worst_lp, worst_q))


def _beam_inputs(K, kind):
  logits, bias = _step_inputs(K, kind, STEP_N)
  prev = -np.random.RandomState(7000 + K).rand(STEP_N, STEP_B).astype(np.float32)
  return logits.reshape(STEP_N, STEP_B, K), prev, bias


@pytest.mark.parametrize("K", STEP_K)
def test_beam_step_op_against_the_restatement(built_lib, K):
  tol = 4 * tm._restatement_error()        # pylint: disable=protected-access
  for kind in BIASES:
    logits, prev, bias = _beam_inputs(K, kind)
    for mask in MASKS:
      allowed = _step_mask(K, mask, STEP_N)
      for time in (1, 2):
        for diverse in (False, True):
          what = (K, kind, mask, time, diverse)
          new_lp, ids, parents = built_lib.op_beam_step(logits, prev, time, diverse, 0.01, 0,
                                                        allowed=allowed, bias=bias)
          want = cb.beam_step(logits, prev, allowed, bias, time, diverse, 0.01, 0,
                              dtype=np.float64)
          if allowed is not None:
            assert (allowed[np.arange(STEP_N)[:, None], ids] != 0).all(), what
          assert np.isfinite(new_lp).all(), what
          cmp = want["gap"] >= cb.GAP_BAR
          assert (~cmp).sum() * 4 <= STEP_N, what
          assert (ids[cmp] == want["ids"][cmp]).all() and \
              (parents[cmp] == want["parents"][cmp]).all(), what
          d = float(np.abs(new_lp - want["new_lp"])[cmp].max()) if cmp.any() else 0.0
          assert d <= tol, (what, d, tol)
          zero = built_lib.op_beam_step(logits, prev, time, diverse, 0.01, 0, allowed=allowed,
                                        bias=np.zeros_like(bias))
          plain = built_lib.op_beam_step(logits, prev, time, diverse, 0.01, 0, allowed=allowed)
          for a, b in zip(zero, plain):
            assert a.tobytes() == b.tobytes(), what


@pytest.mark.parametrize("K", STEP_K)
def test_sbs_step_op_against_the_restatement(built_lib, K):
  tol = 4 * tm._restatement_error()        # pylint: disable=protected-access
  rng = np.random.RandomState(8000 + K)
  for kind in BIASES:
    logits, _, bias = _beam_inputs(K, kind)
    phi, LP, G = (-rng.rand(STEP_N, STEP_B).astype(np.float32) for _ in range(3))
    for mask in MASKS:
      allowed = _step_mask(K, mask, STEP_N)
      for t in (0, 1):
        for temp in TEMPS:
          what = (K, kind, mask, t, temp)
          got = built_lib.op_sbs_step(logits, phi, LP, G, t, temp, STEP_SEED, allowed=allowed,
                                      bias=bias)
          want = cb.sbs_step(logits, phi, LP, G, t, allowed, bias, temp, STEP_SEED,
                             dtype=np.float64)
          nphi, nlp, ng, ids, parents = got
          if allowed is not None:
            assert (allowed[np.arange(STEP_N)[:, None], ids] != 0).all(), what
          assert all(np.isfinite(a).all() for a in (nphi, nlp, ng)), what
          cmp = want["gap"] >= cb.GAP_BAR
          assert (~cmp).sum() * 4 <= STEP_N, what
          assert (ids[cmp] == want["ids"][cmp]).all() and \
              (parents[cmp] == want["parents"][cmp]).all(), what
          for a, key in ((nphi, "new_phi"), (nlp, "new_lp"), (ng, "new_g")):
            d = float(np.abs(a - want[key])[cmp].max()) if cmp.any() else 0.0
            assert d <= max(tol, 2e-5), (what, key, d, tol)   # the bar of the masked op
          zero = built_lib.op_sbs_step(logits, phi, LP, G, t, temp, STEP_SEED, allowed=allowed,
                                       bias=np.zeros_like(bias))
          plain = built_lib.op_sbs_step(logits, phi, LP, G, t, temp, STEP_SEED, allowed=allowed)
          for a, b in zip(zero, plain):
            assert a.tobytes() == b.tobytes(), what


# ---------------------------------------------------------------- zero bias, graph replay

@functools.lru_cache(maxsize=None)
def _runs(kind):
  """One handle: eager forwards under bias A, A2, B (a plane per step), zero and none, then the
  same in graph mode; and a handle that never had a bias."""
  cfg, params, feed = _case("k144")
  N, K = cfg.batch_size, _K(cfg)
  A, A2 = _bias(N, 1, K), _bias(N, 1, K, BIAS_SEED + 1)
  Bb = _bias(N, T_PRED, K, BIAS_SEED + 2)
  zero = np.zeros((N, 1, K), dtype=np.float32)
  eng = _engine(cfg, params, kind)
  r = {"biases": {"A": A, "A2": A2, "B": Bb}}
  for key, b in (("A", A), ("A2", A2), ("B", Bb), ("zero", zero), ("none", None)):
    r[key] = _fwd(eng, feed, b)
    if b is not None:
      r[key + "/occ"] = eng.beam_occupancy()
  eng.set_graph_mode(True)
  caps = [eng.graph_captures()]
  for key, b in (("gA", A), ("gA2", A2), ("gA3", A), ("gzero", zero), ("gnone", None), ("gB", Bb),
                 ("gA4", A)):
    r[key] = _fwd(eng, feed, b)
    caps.append(eng.graph_captures())
  r["captures"] = caps
  eng.close()
  fresh = _engine(cfg, params, kind)
  r["fresh"] = _fwd(fresh, feed)
  r["fresh/occ"] = fresh.beam_occupancy()
  fresh.set_graph_mode(True)
  fcaps = [fresh.graph_captures()]
  r["gfresh"] = _fwd(fresh, feed)
  r["gfresh2"] = _fwd(fresh, feed)
  fcaps.append(fresh.graph_captures())
  r["fresh_captures"] = fcaps
  fresh.close()
  return r


@pytest.mark.parametrize("kind", KINDS)
def test_zero_bias_is_bitwise_a_handle_that_never_had_one(built_lib, kind):
  r = _runs(kind)
  keys = sorted(r["fresh"])
  assert _same(r["zero"], r["fresh"], keys) and _same(r["none"], r["fresh"], keys)
  assert _same(r["gzero"], r["gfresh"], keys) and _same(r["gnone"], r["gfresh"], keys)
  assert _same(r["fresh"], r["gfresh"], keys) and _same(r["gfresh2"], r["gfresh"], keys)
  assert r["zero/occ"].tobytes() == r["fresh/occ"].tobytes()
  assert r["fresh_captures"] == [0, 1]     # no bias set: one graph, as ever
  if kind != "beam":                       # under a bias the forwards report the proposal as well
    assert "proposal_logprobs" in r["zero"] and "proposal_logprobs" not in r["none"]
    assert r["zero"]["proposal_logprobs"].tobytes() == r["zero"]["q"].tobytes()
  assert not (r["A"]["ids"] == r["none"]["ids"]).all()       # ... and a real bias bites
  # the logits outputs stay the model's: a first step's logits do not depend on the bias
  assert r["A"]["logits"][:, :, 0].tobytes() == r["none"]["logits"][:, :, 0].tobytes()


@pytest.mark.parametrize("kind", KINDS)
def test_a_replayed_graph_follows_the_bias_without_recapture(built_lib, kind):
  r = _runs(kind)
  for g, e in (("gA", "A"), ("gA2", "A2"), ("gA3", "A"), ("gB", "B"), ("gA4", "A")):
    assert _same(r[g], r[e]), (g, e)
  assert not (r["A"]["ids"] == r["A2"]["ids"]).all()
  # captures: gA one graph; A', A again and zero replay it; none is the unbiased graph; a plane
  # per step is a third; A again replays the first
  c = r["captures"]
  assert [b - a for a, b in zip(c[:-1], c[1:])] == [1, 0, 0, 0, 1, 1, 0], c


# ---------------------------------------------------------------- stickiness

@pytest.mark.parametrize("kind", KINDS)
def test_a_bias_set_on_the_engine_stays_through_feeds_without_the_key(built_lib, kind):
  cfg, params, feed = _case("k144")
  N, K = cfg.batch_size, _K(cfg)
  bias, other = _bias(N, 1, K), _bias(N, 1, K, BIAS_SEED + 1)
  eng = _engine(cfg, params, kind)
  by_feed = _fwd(eng, feed, bias)
  plain = _fwd(eng, feed)                  # a feed without the key clears what a FEED set
  eng.set_cell_bias(bias)
  first, second = _fwd(eng, feed), _fwd(eng, feed)         # ... and not what was set directly
  eng.upload(feed)
  eng.run_resident(True)
  resident = eng.download_beam()[0]
  third = _fwd(eng, feed, other)           # a feed's own bias replaces it, and then follows
  fourth = _fwd(eng, feed)                 # the feeds' rule
  eng.set_cell_bias(bias.reshape((N, 1) + tuple(cfg.scene_grids[list(cfg.use_grids).index(True)])))
  grid_shaped = _fwd(eng, feed)
  eng.set_cell_bias(None)
  fifth = _fwd(eng, feed)
  eng.close()
  assert _same(first, by_feed) and _same(second, by_feed) and _same(grid_shaped, by_feed)
  assert resident["ids"].tobytes() == by_feed["ids"].tobytes()
  assert not _same(third, by_feed)
  assert _same(fourth, plain) and _same(fifth, plain)
  assert not _same(plain, by_feed)


# ---------------------------------------------------------------- the -1e30 identity

@pytest.mark.parametrize("kind", KINDS)
def test_minus_1e30_outside_a_set_is_the_masked_handle(built_lib, kind):
  """As far as tests/test_cell_bias_host.py establishes it on the float32 restatement: the ids,
  the logprobs (the beam's carried score) and the proposal's log-probabilities, bit for bit."""
  cfg, params, feed = _case("k144")
  N, K = cfg.batch_size, _K(cfg)
  mask = _half_mask(N, T_PRED, K)
  veto = np.where(mask != 0, 0.0, -1e30).astype(np.float32)
  eng = _engine(cfg, params, kind)
  masked = _fwd(eng, feed, None, mask)
  biased = _fwd(eng, feed, veto)
  eng.close()
  keys = ["ids", "logprobs", "logits", "grid_reg", "best_beam"] + \
      ([] if kind == "beam" else ["q"]) + (["gumbels"] if kind == "without_replacement" else [])
  for k in keys:
    assert biased[k].tobytes() == masked[k].tobytes(), k


# ---------------------------------------------------------------- the scorer under a bias

@pytest.mark.parametrize("kind", ["independent", "without_replacement"])
def test_the_scorer_returns_the_logprobs_under_a_bias(built_lib, kind):
  cfg, params, feed = _case("k144")
  bias = _bias(cfg.batch_size, T_PRED, _K(cfg))
  eng = _engine(cfg, params, kind)
  arrs = _fwd(eng, feed, bias)
  # the bias is still set while scoring, through the feed or directly: it is neither read ...
  scored = eng.score_futures(dict(feed, cell_bias=bias), arrs["ids"])
  again = _fwd(eng, feed, bias)
  eng.set_cell_bias(bias)
  direct = eng.score_futures(feed, arrs["ids"])
  kept = _fwd(eng, feed)                   # ... nor cleared by a feed without the key
  eng.close()
  assert scored["logprobs"].tobytes() == arrs["logprobs"].tobytes()
  assert direct["logprobs"].tobytes() == arrs["logprobs"].tobytes()
  assert _same(again, arrs) and _same(kept, arrs)          # ... and not changed
  assert np.isfinite(arrs["q"]).all() and (arrs["q"] <= 0).all()
  assert not (arrs["q"] == arrs["logprobs"]).any()         # the proposal is not the model


# ---------------------------------------------------------------- forward parity

@functools.lru_cache(maxsize=None)
def _forward_planes(name, Tm, with_mask):
  cfg = _cfg(name)
  N, K = cfg.batch_size, _K(cfg)
  return _bias(N, Tm, K), (_half_mask(N, T_PRED, K) if with_mask else None)


def _check_sampled(name, mode, Tm, with_mask):
  cfg, params, feed = _case(name)
  bias, mask = _forward_planes(name, Tm, with_mask)
  want = cb.sampled_forward(params, cfg, feed, mask, bias, temperature=TEMP, seed=SEED)
  eng = _engine(cfg, params, "independent", mode)
  arrs = _fwd(eng, feed, bias, mask)
  eng.close()
  N, S, T = cfg.batch_size, cfg.beam_size, T_PRED
  if mask is not None:
    tm._in_mask(arrs["ids"], mask)         # pylint: disable=protected-access
  upto = cb.to.compared_steps(want["compared"])
  cut = int((T - upto).sum())
  print("%s/%s/Tm=%d: %d of %d (row, step) pairs behind a step that is not compared"
        % (name, mode, Tm, cut, N * S * T))
  assert cut * 4 <= N * S * T
  for n in range(N):
    for j in range(S):
      u = int(upto[n, j])
      assert (arrs["ids"][n, j, :u] == want["ids"][n, j, :u]).all(), (n, j)
      lu = min(u + 1, T)
      assert np.abs(arrs["logits"][n, j, :lu] - want["logits"][n, j, :lu]).max() < TOL
      if u == T:
        assert abs(float(arrs["logprobs"][n, j]) - float(want["logprobs"][n, j])) < TOL * T
        assert abs(float(arrs["q"][n, j]) - float(want["proposal_logprobs"][n, j])) < TOL * T
  assert np.abs(arrs["grid_reg"] - want["grid_reg"]).max() < TOL
  plain = so.forward(params, cfg, feed, temperature=TEMP, seed=SEED)
  assert (plain["ids"] != want["ids"]).any()               # the bias bites


def _beam_traced_logits(want, n, b, T):
  """The logits the engine returns for slot b of row n: the BEAM's back-trace
  (include/multiverse_hip.h: "outputs as the beam's"), which, as the reference's, takes step t's
  logits from the row with the index of the path's slot AT step t.  sbs_oracle's "logits" takes
  the row that slot read, its parent's; the two are the same row wherever a slot continues the
  parent of its own index, and this file's biases select paths where they are not."""
  out = np.zeros((T,) + want["step_logits"][0].shape[2:], dtype=np.float32)
  slot = b
  for t in range(T - 1, -1, -1):
    out[t] = want["step_logits"][t][n, slot]
    slot = int(want["step_parents"][t][n, slot])
  return out


def _check_sbs(name, mode, Tm, with_mask):
  cfg, params, feed = _case(name)
  bias, mask = _forward_planes(name, Tm, with_mask)
  want = cb.sbs_forward(params, cfg, feed, mask, bias, temperature=TEMP, seed=SEED)
  eng = _engine(cfg, params, "without_replacement", mode)
  arrs = _fwd(eng, feed, bias, mask)
  eng.close()
  N, B, T = cfg.batch_size, cfg.beam_size, T_PRED
  upto = sbs.compared_steps(want["gap"])
  cut = int((T - upto).sum())
  print("%s/%s/Tm=%d: %d of %d (row, step) pairs behind a gap below 1e-4"
        % (name, mode, Tm, cut, N * T))
  assert cut * 4 <= N * T
  for n in range(N):
    u = int(upto[n])
    if u == T:
      assert (arrs["ids"][n] == want["ids"][n]).all(), n
      for b in range(B):
        assert np.abs(arrs["logits"][n, b] - _beam_traced_logits(want, n, b, T)).max() < TOL
      assert np.abs(arrs["logprobs"][n] - want["logprobs"][n]).max() < TOL * T
      assert np.abs(arrs["gumbels"][n] - want["gumbels"][n]).max() < TOL
      continue
    paths = {} if u == 0 else {tuple(sbs.trace_back(want, n, j, u)[0]): j for j in range(B)}
    for b in range(B):
      j = 0 if u == 0 else paths.get(tuple(arrs["ids"][n, b, :u]))
      assert j is not None, (n, b)
  assert np.abs(arrs["grid_reg"] - want["grid_reg"]).max() < TOL


def _check_beam(name, mode, Tm, with_mask):
  cfg, params, feed = _case(name)
  bias, mask = _forward_planes(name, Tm, with_mask)
  oreg, (ologits, oids, olp), trace = cb.beam_forward(params, cfg, feed, mask, bias)
  s = list(cfg.use_grids).index(True)
  eng = _engine(cfg, params, "beam", mode)
  arrs = _fwd(eng, feed, bias, mask)
  eng.close()
  cut_gap = np.minimum(np.stack(trace["beam_step_cut_gap"], axis=1),
                       np.stack(trace["beam_step_rank_gap"], axis=1))
  compare_beams(arrs, oreg[s].numpy() if hasattr(oreg[s], "numpy") else oreg[s], ologits, oids,
                olp, np.stack(trace["beam_step_topvals"], axis=-1), trace["beam_trace"],
                cut_gap=cut_gap)
  assert compare_beams.unmatched * 4 <= oids.shape[0] * oids.shape[1]
  plain = cm.beam_forward(params, cfg, feed, np.ones((cfg.batch_size, 1, _K(cfg))))[1]
  assert (plain[1] != oids).any()                          # the bias bites


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,mode,Tm,with_mask", [
    ("k144", "f16x3", 1, False), ("k144", "f16x3", T_PRED, True), ("k144", "f32", T_PRED, False),
    ("k576", "f16x3", 1, True), ("k576", "f16x3", T_PRED, False)])
def test_parity_with_the_oracle(built_lib, name, mode, Tm, with_mask, kind):
  {"beam": _check_beam, "independent": _check_sampled, "without_replacement": _check_sbs}[kind](
      name, mode, Tm, with_mask)


# ---------------------------------------------------------------- batch, lengths, short tracks

@pytest.mark.parametrize("kind", KINDS)
def test_rows_are_their_own_uniform_forwards_under_their_bias_row(built_lib, kind):
  lens, obs = (3, 3, 2), (8, 5, 6)
  cfg3, params, feed3 = _case("k144", 3)
  bias = _bias(3, T_PRED, _K(cfg3))
  mask = _half_mask(3, T_PRED, _K(cfg3))
  eng = _engine(cfg3, params, kind)
  full = _fwd(eng, feed3, bias, mask)
  rag = _fwd(eng, dict(feed3, pred_lengths=list(lens), obs_lengths=list(obs)), bias, mask)
  eng.close()
  keys = ["ids", "logits", "logprobs", "grid_reg", "best_beam"] + \
      ([] if kind == "beam" else ["q"]) + (["gumbels"] if kind == "without_replacement" else [])
  eng1 = _engine(_cfg("k144", batch_size=1), params, kind)
  for n in range(3):
    feed1 = dict(feed3, obs_scene=feed3["obs_scene"][n:n + 1],
                 grid_obs_labels=[a[n:n + 1] for a in feed3["grid_obs_labels"]],
                 grid_obs_regress=[a[n:n + 1] for a in feed3["grid_obs_regress"]])
    if kind != "beam":
      eng1.set_sampling(TEMP, so.row_seed(SEED, n), without_replacement=kind == "without_replacement")
    a1 = _fwd(eng1, feed1, bias[n:n + 1], mask[n:n + 1])
    for k in keys:
      assert a1[k][0].tobytes() == full[k][n].tobytes(), (n, k)
    L = lens[n]
    u1 = _fwd(eng1, dict(feed1, pred_length=L, obs_lengths=[obs[n]]), bias[n:n + 1],
              mask[n:n + 1])
    for k, ax in {"ids": 1, "logits": 1, "best_beam": 0, "grid_reg": 0}.items():
      a = np.moveaxis(rag[k][n], ax, 0)
      assert (a[L:] == (-1 if k == "ids" else 0)).all(), (n, k)
      want = np.moveaxis(u1[k][0], ax, 0)
      assert np.ascontiguousarray(a[:L]).tobytes() == np.ascontiguousarray(want).tobytes(), (n, k)
    for k in [k for k in keys if k in ("logprobs", "q", "gumbels")]:
      assert rag[k][n].tobytes() == u1[k][0].tobytes(), (n, k)
  eng1.close()


# ---------------------------------------------------------------- occupancy

def _occupancy_bar(dev, arrs, mask, bias, uniform, what):
  """The bar of the masked occupancy test: 4 x the float32 restatement's own error."""
  N, T, K = dev.shape
  a = np.ones((N, T, K), dtype=bool) if mask is None else \
      np.stack([cm.plane(mask, t) for t in range(T)], axis=1)
  assert (dev[~a] == 0).all()                              # exactly 0 outside A
  assert np.abs(dev.astype(np.float64).sum(-1) - 1).max() <= 1e-5
  exact = cb.occupancy(arrs["logits"], arrs["logprobs"], mask, bias, uniform, np.float64)
  ref32 = cb.occupancy(arrs["logits"], arrs["logprobs"], mask, bias, uniform, np.float32)
  big = a & (exact > 1e-30)                                # (a relative error needs a value)
  d_ref = float((np.abs(ref32 - exact)[big] / exact[big]).max())
  d_dev = float((np.abs(dev - exact)[big] / exact[big]).max())
  print("%s: float32 restatement vs fp64 %.3g, device vs fp64 %.3g (bar %.3g)"
        % (what, d_ref, d_dev, 4 * d_ref))
  assert d_dev <= 4 * d_ref


@pytest.mark.parametrize("kind", KINDS)
def test_occupancy_is_the_biased_mixture(built_lib, kind):
  r = _runs(kind)
  for key in ("A", "B"):
    _occupancy_bar(r[key + "/occ"], r[key], None, r["biases"][key], kind == "independent",
                   "%s/%s" % (kind, key))
  assert r["A/occ"].tobytes() != r["fresh/occ"].tobytes()
  # with a mask as well, and the bias that is set when the map is asked for
  cfg, params, feed = _case("k144")
  N, K = cfg.batch_size, _K(cfg)
  mask, bias = _half_mask(N, T_PRED, K), _bias(N, T_PRED, K, BIAS_SEED + 3)
  eng = _engine(cfg, params, kind)
  arrs = _fwd(eng, feed, bias, mask)
  _occupancy_bar(eng.beam_occupancy(), arrs, mask, bias, kind == "independent", kind + "/masked")
  eng.set_cell_mask(None)
  eng.set_cell_bias(r["biases"]["A"])      # set AFTER the forward: the map reads this one
  _occupancy_bar(eng.beam_occupancy(), arrs, None, r["biases"]["A"], kind == "independent",
                 kind + "/later")
  eng.close()


def test_any_k_occupancy_and_the_widest_row_form(built_lib):
  """The literal 36 x 22 grid of test_gpu_cell_mask.py: K = 792 cells take the J = 16 form of the
  step kernels and the any-K form of the occupancy kernel."""
  cfg = synth.default_config(batch_size=2, use_grids=(1, 0), beam_size=3, scene_h=72, scene_w=44,
                             scene_grids=[(36, 22), (18, 11)])
  cfg.max_pred_len = T_PRED
  params = synth.make_params(cfg, seed=synth.SEED_BASE + 91, recurrent_gain=3.0, bias_scale=0.1)
  feed = synth.make_feed(cfg, seed=synth.SEED_BASE + 91, pred_len=T_PRED)
  bias = _bias(2, T_PRED, 792)
  for kind, mask in zip(KINDS, (None, _half_mask(2, T_PRED, 792), None)):
    eng = _engine(cfg, params, kind, "f32")
    plain = _fwd(eng, feed, None, mask)
    arrs = _fwd(eng, feed, bias, mask)
    dev = eng.beam_occupancy()
    eng.close()
    assert not (arrs["ids"] == plain["ids"]).all()
    if mask is not None:
      tm._in_mask(arrs["ids"], mask)       # pylint: disable=protected-access
    _occupancy_bar(dev, arrs, mask, bias, kind == "independent", "k792 " + kind)


# ---------------------------------------------------------------- errors

def test_errors_name_their_cause(built_lib):
  lib = built_lib
  cfg, params, feed = _case("k144")
  N, K = cfg.batch_size, _K(cfg)
  greedy = synth.default_config(batch_size=2, use_grids=(0, 1), enc_hidden_size=128,
                                dec_hidden_size=128)
  geng = lib.Engine(greedy, device=0)
  with pytest.raises(lib.MvError) as err:
    geng.set_cell_bias(np.zeros((N, K), dtype=np.float32))
  assert "mv_set_cell_bias" in str(err.value) and "beam_size 1" in str(err.value)
  geng.close()
  eng = _engine(cfg, params, "beam")
  zero = np.zeros((N, 1, K), dtype=np.float32)
  fp = zero.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
  for tm_ in (0, -2):
    assert eng.lib.mv_set_cell_bias(eng.handle, fp, tm_) != 0
    assert "Tm = %d" % tm_ in eng.lib.mv_last_error(eng.handle).decode()
  with pytest.raises(lib.MvError) as err:
    eng.set_cell_bias(np.zeros((N, K + 1), dtype=np.float32))
  assert "cell_bias" in str(err.value)
  # a value that is not finite: n, tm and k, when the bias is set
  for bad in (np.nan, np.inf, -np.inf):
    b = np.zeros((N, T_PRED, K), dtype=np.float32)
    b[1, 2, 7] = bad
    with pytest.raises(lib.MvError) as err:
      eng.set_cell_bias(b)
    msg = str(err.value)
    assert "mv_set_cell_bias" in msg and "n = 1" in msg and "tm = 2" in msg and "k = 7" in msg
    assert "finite" in msg, bad
  before = dict(eng.forward_beam(feed)[0])                 # a refused bias is not set
  # 1 < Tm < pred_len, at the forward
  with pytest.raises(lib.MvError) as err:
    eng.forward_beam(dict(feed, cell_bias=np.zeros((N, 2, K), dtype=np.float32)))
  assert "mv_set_cell_bias" in str(err.value)
  assert "Tm = 2" in str(err.value) and "pred_len = 3" in str(err.value)
  # ... and by the occupancy map for the bias that is set when it is called
  eng.forward_beam(feed)
  eng.set_cell_bias(np.zeros((N, 2, K), dtype=np.float32))
  with pytest.raises(lib.MvError) as err:
    eng.beam_occupancy()
  assert "mv_beam_occupancy" in str(err.value) and "Tm = 2" in str(err.value)
  eng.set_cell_bias(None)
  # training and the pipelined greedy forward while a bias is set: the message names the call
  eng.set_cell_bias(zero)
  for call, name in ((eng.train_init, "mv_train_init"), (eng.train_step, "mv_train_step"),
                     (eng.train_forward_backward, "mv_train_forward_backward"),
                     (eng.train_apply, "mv_train_apply")):
    with pytest.raises(lib.MvError) as err:
      call()
    assert name + ":" in str(err.value) and "cell bias" in str(err.value), name
  inp = eng._inputs(dict(feed, cell_bias=zero))            # pylint: disable=protected-access
  assert eng.lib.mv_submit_greedy(eng.handle, ctypes.byref(inp)) != 0
  msg = eng.lib.mv_last_error(eng.handle).decode()
  assert "mv_submit_greedy" in msg and "cell bias" in msg
  eng.set_cell_bias(None)
  assert _same(dict(eng.forward_beam(feed)[0]), before)
  eng.close()
  # a grid of more than 1024 cells, at the forward (refused before anything is launched)
  big = synth.default_config(batch_size=1, use_grids=(1, 0), beam_size=2, enc_hidden_size=128,
                             dec_hidden_size=128, scene_h=72, scene_w=64,
                             scene_grids=[(36, 32), (18, 16)])
  big.max_pred_len = T_PRED
  beng = lib.Engine(big, device=0)
  bfeed = synth.make_feed(big, seed=synth.SEED_BASE + 7, pred_len=T_PRED)
  with pytest.raises(lib.MvError) as err:
    beng.forward_beam(dict(bfeed, cell_bias=np.zeros((1, 1152), dtype=np.float32)))
  assert "1152 cells" in str(err.value) and "mv_set_cell_bias" in str(err.value)
  beng.close()
  for op, args in ((lib.op_beam_step, (np.zeros((1, 2, 1100), np.float32), np.zeros((1, 2), np.float32),
                                       2, False, 1.0, 0)),
                   (lib.op_sbs_step, (np.zeros((1, 2, 1100), np.float32),) +
                    (np.zeros((1, 2), np.float32),) * 3 + (1,)),
                   (lib.op_sample_step, (np.zeros((2, 1100), np.float32), 2, 0))):
    with pytest.raises(lib.MvError) as err:
      op(*args, bias=np.zeros((1, 1100), dtype=np.float32))
    assert "K = 1100" in str(err.value) and "mv_" + op.__name__ in str(err.value), op
    small = tuple(a[..., :70] if isinstance(a, np.ndarray) and a.shape[-1] == 1100 else a
                  for a in args)
    with pytest.raises(lib.MvError) as err:
      op(*small, bias=np.full((1, 70), np.nan, dtype=np.float32))
    assert "finite" in str(err.value), op
