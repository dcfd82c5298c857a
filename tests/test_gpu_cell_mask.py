# coding=utf-8
"""GPU: the constrained decode (mv_set_cell_mask): per-row allowed cells for the beam search, the
independent sampler and the sampling without replacement, and the occupancy map after them.  The
reference has none; the definition is in include/multiverse_hip.h and restated
by tests/cell_mask_oracle.py on top of the existing restatements.

The feed seeds are those of test_gpu_truncation.py and the masks come from the generator seeds
below; both were checked on the CPU, with the restatement alone, to keep the (row, step) pairs
that follow a near tie within a quarter of each forward case."""
import copy
import ctypes
import functools

import numpy as np
import pytest

from multiverse_amd import synth

import cell_mask_oracle as cm
import sampling_oracle as so
import sbs_oracle as sbs
from beam_compare import compare_beams

pytestmark = pytest.mark.gpu

TOL = 1e-4            # the project's parity bar on logits and offsets
T_PRED = 3
TEMP, SEED = 0.8, 1234
LITERAL = dict(scene_h=72, scene_w=36, scene_grids=[(36, 18), (18, 9)])
KINDS = ("beam", "independent", "without_replacement")

# name -> (config overrides, used grid, B or S, feed seed): the cases of test_gpu_truncation.py
CASES = {
    "k144": (dict(), (0, 1), 3, synth.SEED_BASE + 81),     # 9 x 16: a partial third lane group
    "k576": (dict(), (1, 0), 3, synth.SEED_BASE + 102),    # 18 x 32: J = 9
    "k162": (LITERAL, (0, 1), 2, synth.SEED_BASE + 101),   # 18 x 9: K no multiple of 64
}
MASK_SEED = 4100


def _cfg(name, batch_size=2, S=None, diverse=True):
  over, grids, s_default, _ = CASES[name]
  cfg = synth.default_config(batch_size=batch_size, use_grids=grids,
                             beam_size=S or s_default, enc_hidden_size=128,
                             dec_hidden_size=128, **over)
  cfg.max_pred_len = 4
  cfg.diverse_beam = bool(diverse)
  return cfg


def _K(cfg):
  h, w = cfg.scene_grids[list(cfg.use_grids).index(True)]
  return h * w


@functools.lru_cache(maxsize=None)
def _case(name, batch_size=2):
  cfg = _cfg(name, batch_size)
  params = synth.make_params(cfg, recurrent_gain=3.0, bias_scale=0.1)
  seed = CASES[name][3] if batch_size == 2 else synth.SEED_BASE + 84
  feed = synth.make_feed(cfg, seed=seed, pred_len=T_PRED)
  return cfg, params, feed


def _half_mask(N, Tm, K, seed=MASK_SEED):
  """A random half of the cells per (row, plane); the planes of a row differ."""
  m = (np.random.RandomState(seed + K).rand(N, Tm, K) < 0.5).astype(np.uint8)
  assert (m.sum(-1) >= 8).all()
  return m


def _engine(cfg, params, kind, mode="f16x3", temp=TEMP, seed=SEED):
  import multiverse_amd._lib as lib
  eng = lib.Engine(cfg, device=0)
  eng.set_params(params)
  eng.set_compute_mode(mode)
  if kind != "beam":
    eng.set_sampling(temp, seed, without_replacement=kind == "without_replacement")
  return eng


def _fwd(eng, feed, mask=None):
  """One forward under `mask` (None: none) -> its arrays, with the proposal's log-probability
  under "q" where the forward sampled."""
  arrs = dict(eng.forward_beam(dict(feed, cell_mask=mask) if mask is not None else feed)[0])
  if getattr(eng, "_sampling_on", False):
    arrs["q"] = eng.beam_proposal_logprobs()
  return arrs


def _same(a, b, keys=None):
  """Bitwise equal: every key of both (keys None), or the given keys."""
  if keys is None:
    keys = sorted(a)
    if keys != sorted(b):
      return False
  return all(a[k].tobytes() == b[k].tobytes() and a[k].shape == b[k].shape for k in keys)


def _in_mask(ids, mask, lens=None):
  """Every returned id at t < length lies in A(n, t)."""
  N, B, T = ids.shape
  for n in range(N):
    for t in range(T if lens is None else lens[n]):
      a = cm.plane(mask, t)[n]
      assert a[ids[n, :, t]].all(), (n, t, ids[n, :, t])


# ---------------------------------------------------------------- 1. the step ops

STEP_K = [70, 144, 162, 576, 1024]            # J = 3 / 9 / 16; 70 and 162 no multiple of 64
STEP_R, STEP_S, STEP_T, STEP_SEED = 8, 2, 2, 99
STEP_N, STEP_B = 4, 2                         # the beam and the without-replacement op: R = N * B
TIE = (5, 17, 40)                             # row 0: three exactly equal top logits
HOT = (1, 2, 3)                               # "low": disallowed cells 200 above the rest
MASKS = ("ones", "half", "no_tie", "exactly_b", "last_group", "low")


def _step_logits(K, mask):
  rng = np.random.RandomState(5000 + 7 * K)
  logits = (4.0 * rng.randn(STEP_R, K)).astype(np.float32)
  logits[0, list(TIE)] = logits[0].max() + np.float32(0.5)
  if mask == "low":
    logits[:, list(HOT)] = logits.max() + np.float32(200.0)
  return logits


def _step_mask(K, mask, samples):
  """allowed [samples, K] of the named kind (the same plane logic for every op)."""
  rng = np.random.RandomState(6000 + K)
  a = np.ones((samples, K), dtype=np.uint8)
  if mask == "half":
    a = (rng.rand(samples, K) < 0.5).astype(np.uint8)
  elif mask == "no_tie":
    a[:, list(TIE)] = 0
  elif mask == "exactly_b":
    a[:] = 0
    for n in range(samples):
      a[n, rng.choice(K, STEP_B, replace=False)] = 1
  elif mask == "last_group":
    a[:] = 0
    a[:, 64 * ((K - 1) // 64):] = 1
  elif mask == "low":
    a[:, list(HOT)] = 0
  return a


SAMPLE_LIMITS = [(0, 1.0), (8, 0.9)]


def _sample_table():
  for K in STEP_K:
    for mask in MASKS:
      for limits in SAMPLE_LIMITS:
        for temp in (1.0, 0.7):
          yield K, mask, limits, temp


@functools.lru_cache(maxsize=None)
def _sample_want(K, mask, limits, temp, dtype):
  return cm.sample_step(_step_logits(K, mask), STEP_S, STEP_T,
                        _step_mask(K, mask, STEP_R // STEP_S), temp, STEP_SEED, limits[0],
                        limits[1], 1, dtype=dtype)


@functools.lru_cache(maxsize=None)
def _restatement_error():
  """The largest |float32 restatement - float64 restatement| of lp[id] and q~[id] over the whole
  table of sampler step cases (same ids), computed once: the bar of test_gpu_truncation.py."""
  worst = 0.0
  for case in _sample_table():
    a, b = _sample_want(*case, np.float32), _sample_want(*case, np.float64)
    for key in ("lp_id", "q_id"):
      worst = max(worst, float(np.abs(a[key].astype(np.float64) - b[key]).max()))
  return worst


@pytest.mark.parametrize("K", STEP_K)
def test_sample_step_op_against_the_restatement(built_lib, K):
  e32 = _restatement_error()
  tol = 4 * e32        # device and numpy libm differ by a few ulp per transcendental
  assert tol < 1e-4
  rows = np.arange(STEP_R)
  worst_lp = worst_q = 0.0
  for mask in MASKS:
    logits = _step_logits(K, mask)
    allowed = _step_mask(K, mask, STEP_R // STEP_S)
    arows = np.repeat(allowed != 0, STEP_S, axis=0)
    for limits in SAMPLE_LIMITS:
      for temp in (1.0, 0.7):
        what = (K, mask, limits, temp)
        ids, lp, qlp, keep = built_lib.op_sample_step(logits, STEP_S, STEP_T, temp, STEP_SEED,
                                                      limits[0], limits[1], 1, allowed=allowed)
        want = _sample_want(K, mask, limits, temp, np.float64)
        band = want["wide"] & ~want["tight"]
        assert (keep == want["tight"])[~band].all(), what
        assert not (keep & ~arows).any(), what             # keep is a subset of A
        assert keep[rows, ids].all(), what                 # the drawn cell is a kept cell
        if limits == (0, 1.0):
          assert (keep == arows).all(), what               # no limit: the kept set IS A
        if mask == "no_tie":
          assert not keep[:, list(TIE)].any(), what
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
        if mask == "ones":                                 # all allowed: the unmasked op, bitwise
          plain = built_lib.op_sample_step(logits, STEP_S, STEP_T, temp, STEP_SEED, limits[0],
                                           limits[1], 1)
          for a, b in zip((ids, lp, qlp, keep), plain):
            assert a.tobytes() == b.tobytes(), what
  print("K=%d: float32 restatement vs float64 %.3g -> bar %.3g; device: logprob %.3g, "
        "proposal %.3g" % (K, e32, tol, worst_lp, worst_q))


def _beam_inputs(K, mask):
  logits = _step_logits(K, mask).reshape(STEP_N, STEP_B, K)
  prev = -np.random.RandomState(7000 + K).rand(STEP_N, STEP_B).astype(np.float32)
  return logits, prev, _step_mask(K, mask, STEP_N)


@pytest.mark.parametrize("K", STEP_K)
def test_beam_step_op_against_the_restatement(built_lib, K):
  tol = 4 * _restatement_error()
  for mask in MASKS:
    logits, prev, allowed = _beam_inputs(K, mask)
    for time in (1, 2):
      for diverse in (False, True):
        what = (K, mask, time, diverse)
        new_lp, ids, parents = built_lib.op_beam_step(logits, prev, time, diverse, 0.01, 0,
                                                      allowed=allowed)
        want = cm.beam_step(logits, prev, allowed, time, diverse, 0.01, 0, dtype=np.float64)
        assert (allowed[np.arange(STEP_N)[:, None], ids] != 0).all(), what
        assert np.isfinite(new_lp).all(), what
        cmp = want["gap"] >= cm.GAP_BAR
        assert (~cmp).sum() * 4 <= STEP_N, what
        assert (ids[cmp] == want["ids"][cmp]).all() and \
            (parents[cmp] == want["parents"][cmp]).all(), what
        d = float(np.abs(new_lp - want["new_lp"])[cmp].max()) if cmp.any() else 0.0
        assert d <= tol, (what, d, tol)
        if mask == "ones":
          plain = built_lib.op_beam_step(logits, prev, time, diverse, 0.01, 0)
          for a, b in zip((new_lp, ids, parents), plain):
            assert a.tobytes() == b.tobytes(), what


@pytest.mark.parametrize("K", STEP_K)
def test_sbs_step_op_against_the_restatement(built_lib, K):
  tol = 4 * _restatement_error()
  rng = np.random.RandomState(8000 + K)
  for mask in MASKS:
    logits, _, allowed = _beam_inputs(K, mask)
    phi, LP, G = (-rng.rand(STEP_N, STEP_B).astype(np.float32) for _ in range(3))
    for t in (0, 1):
      for temp in (1.0, 0.7):
        what = (K, mask, t, temp)
        got = built_lib.op_sbs_step(logits, phi, LP, G, t, temp, STEP_SEED, allowed=allowed)
        want = cm.sbs_step(logits, phi, LP, G, t, allowed, temp, STEP_SEED, dtype=np.float64)
        nphi, nlp, ng, ids, parents = got
        assert (allowed[np.arange(STEP_N)[:, None], ids] != 0).all(), what
        assert all(np.isfinite(a).all() for a in (nphi, nlp, ng)), what
        cmp = want["gap"] >= cm.GAP_BAR
        assert (~cmp).sum() * 4 <= STEP_N, what
        assert (ids[cmp] == want["ids"][cmp]).all() and \
            (parents[cmp] == want["parents"][cmp]).all(), what
        for a, key in ((nphi, "new_phi"), (nlp, "new_lp"), (ng, "new_g")):
          d = float(np.abs(a - want[key])[cmp].max()) if cmp.any() else 0.0
          assert d <= max(tol, 2e-5), (what, key, d, tol)   # G, phi: sums of three rounded terms
        if mask == "ones":
          plain = built_lib.op_sbs_step(logits, phi, LP, G, t, temp, STEP_SEED)
          for a, b in zip(got, plain):
            assert a.tobytes() == b.tobytes(), what


# ---------------------------------------------------------------- 2 / 8. identity, graph replay

@functools.lru_cache(maxsize=None)
def _runs(kind):
  """One handle: eager forwards under mask A, mask B (a plane per step), all ones and none, then
  the same in graph mode (A, A', ones, none; B, A again); and a handle that never had a mask."""
  cfg, params, feed = _case("k144")
  N, K = cfg.batch_size, _K(cfg)
  A, A2 = _half_mask(N, 1, K), _half_mask(N, 1, K, MASK_SEED + 1)
  Bm = _half_mask(N, T_PRED, K, MASK_SEED + 2)
  ones = np.ones((N, 1, K), dtype=np.uint8)
  eng = _engine(cfg, params, kind)
  r = {"masks": {"A": A, "A2": A2, "B": Bm}}
  for key, m in (("A", A), ("A2", A2), ("B", Bm), ("ones", ones), ("none", None)):
    r[key] = _fwd(eng, feed, m)
    if m is not None:
      r[key + "/occ"] = eng.beam_occupancy()
  eng.set_graph_mode(True)
  caps = [eng.graph_captures()]
  for key, m in (("gA", A), ("gA2", A2), ("gA3", A), ("gones", ones), ("gnone", None), ("gB", Bm),
                 ("gA4", A)):
    r[key] = _fwd(eng, feed, m)
    caps.append(eng.graph_captures())
  r["captures"] = caps
  eng.close()
  fresh = _engine(cfg, params, kind)
  r["fresh"] = _fwd(fresh, feed)
  fresh.set_graph_mode(True)
  r["gfresh"] = _fwd(fresh, feed)
  fresh.close()
  return r


@pytest.mark.parametrize("kind", KINDS)
def test_all_ones_is_bitwise_a_handle_that_never_had_a_mask(built_lib, kind):
  r = _runs(kind)
  keys = sorted(r["fresh"])
  assert _same(r["ones"], r["fresh"], keys) and _same(r["none"], r["fresh"], keys)
  assert _same(r["gones"], r["gfresh"], keys) and _same(r["gnone"], r["gfresh"], keys)
  assert _same(r["fresh"], r["gfresh"], keys)
  if kind != "beam":                     # under a mask the forwards report the proposal as well
    assert "proposal_logprobs" in r["ones"] and "proposal_logprobs" not in r["none"]
    assert r["ones"]["proposal_logprobs"].tobytes() == r["ones"]["q"].tobytes()
  assert not (r["A"]["ids"] == r["none"]["ids"]).all()     # ... and a real mask bites


@pytest.mark.parametrize("kind", KINDS)
def test_a_replayed_graph_follows_the_mask_without_recapture(built_lib, kind):
  r = _runs(kind)
  for g, e in (("gA", "A"), ("gA2", "A2"), ("gA3", "A"), ("gB", "B"), ("gA4", "A")):
    assert _same(r[g], r[e]), (g, e)
  assert not (r["A"]["ids"] == r["A2"]["ids"]).all()
  # captures: gA one graph; A', A again replay it; all ones replays it too; none is the unmasked
  # graph; a plane per step is a third; A again replays the first
  c = r["captures"]
  assert [b - a for a, b in zip(c[:-1], c[1:])] == [1, 0, 0, 0, 1, 1, 0], c


# ---------------------------------------------------------------- 3. ids stay inside the mask

@pytest.mark.parametrize("kind", KINDS)
def test_no_id_leaves_the_mask(built_lib, kind):
  r = _runs(kind)
  for key in ("A", "A2", "B", "gA", "gB"):
    _in_mask(r[key]["ids"], r["masks"][key.lstrip("g")])
  Bm = r["masks"]["B"]
  assert not (Bm[:, 0] == Bm[:, 1]).all()                  # the planes of B differ
  # the logits outputs are the model's: finite everywhere, masked cells included
  assert np.isfinite(r["A"]["logits"]).all()


# ---------------------------------------------------------------- 4. oracle-free

@pytest.mark.parametrize("kind,diverse", [("independent", True), ("beam", False)])
def test_masking_cells_no_future_chose_changes_nothing_but_the_proposal(built_lib, kind, diverse):
  cfg, params, feed = _case("k144")
  cfg = copy.copy(cfg)
  cfg.diverse_beam = diverse
  eng = _engine(cfg, params, kind)
  plain = _fwd(eng, feed)
  N, K = cfg.batch_size, _K(cfg)
  rng = np.random.RandomState(11)
  mask = (rng.rand(N, 1, K) < 0.5).astype(np.uint8)
  for n in range(N):                       # only cells no future of the row chose at any step
    mask[n, 0, np.unique(plain["ids"][n])] = 1
  if kind == "beam":
    # ... a hypothesis the search held for a step and dropped later chose cells too: the
    # restatement's per-step selections name them (the returned ids are the survivors' only)
    trace = cm.beam_forward(params, cfg, feed, np.ones((N, 1, K), dtype=np.uint8))[2]
    for step_ids in trace["beam_step_ids"]:
      for n in range(N):
        mask[n, 0, np.unique(step_ids[n])] = 1
  got = _fwd(eng, feed, mask)
  eng.close()
  assert (mask == 0).sum() > N * K // 4
  for k in ("ids", "logprobs", "logits", "best_beam", "grid_reg"):
    assert got[k].tobytes() == plain[k].tobytes(), k
  if kind == "independent":                # the proposal is renormalised over fewer cells
    assert (got["q"] >= plain["q"]).all() and (got["q"] > plain["q"]).any()


# ---------------------------------------------------------------- a mask set directly is sticky

@pytest.mark.parametrize("kind", KINDS)
def test_a_mask_set_on_the_engine_stays_through_feeds_without_the_key(built_lib, kind):
  cfg, params, feed = _case("k144")
  N, K = cfg.batch_size, _K(cfg)
  mask, other = _half_mask(N, 1, K), _half_mask(N, 1, K, MASK_SEED + 1)
  eng = _engine(cfg, params, kind)
  by_feed = _fwd(eng, feed, mask)
  plain = _fwd(eng, feed)                  # a feed without the key clears what a FEED set
  eng.set_cell_mask(mask)
  first, second = _fwd(eng, feed), _fwd(eng, feed)         # ... and not what was set directly
  eng.upload(feed)
  eng.run_resident(True)
  resident = eng.download_beam()[0]
  occ = eng.beam_occupancy()
  third = _fwd(eng, feed, other)           # a feed's own mask replaces it, and then follows
  fourth = _fwd(eng, feed)                 # the feeds' rule
  eng.set_cell_mask(mask)
  eng.set_cell_mask(None)
  fifth = _fwd(eng, feed)
  eng.close()
  assert _same(first, by_feed) and _same(second, by_feed)
  assert resident["ids"].tobytes() == by_feed["ids"].tobytes()
  assert (occ[~np.broadcast_to(mask != 0, occ.shape)] == 0).all()
  _in_mask(third["ids"], other)
  assert not _same(third, by_feed)
  assert _same(fourth, plain) and _same(fifth, plain)
  assert not _same(plain, by_feed)


# ---------------------------------------------------------------- 5. the scorer under a mask

@pytest.mark.parametrize("kind", ["independent", "without_replacement"])
def test_the_scorer_returns_the_logprobs_under_a_mask(built_lib, kind):
  cfg, params, feed = _case("k144")
  mask = _half_mask(cfg.batch_size, T_PRED, _K(cfg))
  eng = _engine(cfg, params, kind)
  arrs = _fwd(eng, feed, mask)
  # the mask is still set while scoring, through the feed or directly: it is neither read ...
  scored = eng.score_futures(dict(feed, cell_mask=mask), arrs["ids"])
  again = _fwd(eng, feed, mask)
  eng.set_cell_mask(mask)
  direct = eng.score_futures(feed, arrs["ids"])
  kept = _fwd(eng, feed)                   # ... nor cleared by a feed without the key
  eng.close()
  assert scored["logprobs"].tobytes() == arrs["logprobs"].tobytes()
  assert direct["logprobs"].tobytes() == arrs["logprobs"].tobytes()
  assert _same(again, arrs) and _same(kept, arrs)          # ... and not changed
  assert np.isfinite(arrs["q"]).all() and (arrs["q"] <= 0).all()
  assert not (arrs["q"] == arrs["logprobs"]).any()         # the proposal is not the model


# ---------------------------------------------------------------- 6. forward parity

@functools.lru_cache(maxsize=None)
def _forward_mask(name):
  cfg = _cfg(name)
  return _half_mask(cfg.batch_size, T_PRED, _K(cfg))


def _check_sampled(name, mode):
  cfg, params, feed = _case(name)
  mask = _forward_mask(name)
  want = cm.sampled_forward(params, cfg, feed, mask, temperature=TEMP, seed=SEED)
  eng = _engine(cfg, params, "independent", mode)
  arrs = _fwd(eng, feed, mask)
  eng.close()
  N, S, T = cfg.batch_size, cfg.beam_size, T_PRED
  _in_mask(arrs["ids"], mask)
  upto = cm.to.compared_steps(want["compared"])
  cut = int((T - upto).sum())
  print("%s/%s: %d of %d (row, step) pairs behind a step that is not compared"
        % (name, mode, cut, N * S * T))
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
  assert (plain["ids"] != want["ids"]).any()               # the mask bites


def _check_sbs(name, mode):
  cfg, params, feed = _case(name)
  mask = _forward_mask(name)
  want = cm.sbs_forward(params, cfg, feed, mask, temperature=TEMP, seed=SEED)
  eng = _engine(cfg, params, "without_replacement", mode)
  arrs = _fwd(eng, feed, mask)
  eng.close()
  N, B, T = cfg.batch_size, cfg.beam_size, T_PRED
  _in_mask(arrs["ids"], mask)
  upto = sbs.compared_steps(want["gap"])
  cut = int((T - upto).sum())
  print("%s/%s: %d of %d (row, step) pairs behind a gap below 1e-4" % (name, mode, cut, N * T))
  assert cut * 4 <= N * T
  for n in range(N):
    u = int(upto[n])
    if u == T:
      assert (arrs["ids"][n] == want["ids"][n]).all(), n
      assert np.abs(arrs["logits"][n] - want["logits"][n]).max() < TOL
      assert np.abs(arrs["logprobs"][n] - want["logprobs"][n]).max() < TOL * T
      assert np.abs(arrs["gumbels"][n] - want["gumbels"][n]).max() < TOL
      continue
    paths = {} if u == 0 else {tuple(sbs.trace_back(want, n, j, u)[0]): j for j in range(B)}
    for b in range(B):
      j = 0 if u == 0 else paths.get(tuple(arrs["ids"][n, b, :u]))
      assert j is not None, (n, b)
  assert np.abs(arrs["grid_reg"] - want["grid_reg"]).max() < TOL


def _check_beam(name, mode):
  cfg, params, feed = _case(name)
  mask = _forward_mask(name)
  oreg, (ologits, oids, olp), trace = cm.beam_forward(params, cfg, feed, mask)
  s = list(cfg.use_grids).index(True)
  eng = _engine(cfg, params, "beam", mode)
  arrs = _fwd(eng, feed, mask)
  eng.close()
  _in_mask(arrs["ids"], mask)
  _in_mask(oids, mask)
  cut_gap = np.minimum(np.stack(trace["beam_step_cut_gap"], axis=1),
                       np.stack(trace["beam_step_rank_gap"], axis=1))
  compare_beams(arrs, oreg[s].numpy() if hasattr(oreg[s], "numpy") else oreg[s], ologits, oids,
                olp, np.stack(trace["beam_step_topvals"], axis=-1), trace["beam_trace"],
                cut_gap=cut_gap)
  assert compare_beams.unmatched * 4 <= oids.shape[0] * oids.shape[1]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,mode", [("k144", "f16x3"), ("k144", "f32"), ("k576", "f16x3"),
                                       ("k162", "f16x3")])
def test_parity_with_the_oracle(built_lib, name, mode, kind):
  {"beam": _check_beam, "independent": _check_sampled, "without_replacement": _check_sbs}[kind](
      name, mode)


# ---------------------------------------------------------------- 7. batch, lengths, short tracks

@pytest.mark.parametrize("kind", KINDS)
def test_rows_are_their_own_uniform_forwards_under_their_mask_row(built_lib, kind):
  lens, obs = (3, 3, 2), (8, 5, 6)
  cfg3, params, feed3 = _case("k144", 3)
  mask = _half_mask(3, T_PRED, _K(cfg3))
  eng = _engine(cfg3, params, kind)
  full = _fwd(eng, feed3, mask)
  rag = _fwd(eng, dict(feed3, pred_lengths=list(lens), obs_lengths=list(obs)), mask)
  eng.close()
  _in_mask(rag["ids"], mask, lens)
  keys = ["ids", "logits", "logprobs", "grid_reg", "best_beam"] + \
      ([] if kind == "beam" else ["q"]) + (["gumbels"] if kind == "without_replacement" else [])
  eng1 = _engine(_cfg("k144", batch_size=1), params, kind)
  for n in range(3):
    feed1 = dict(feed3, obs_scene=feed3["obs_scene"][n:n + 1],
                 grid_obs_labels=[a[n:n + 1] for a in feed3["grid_obs_labels"]],
                 grid_obs_regress=[a[n:n + 1] for a in feed3["grid_obs_regress"]])
    if kind != "beam":
      eng1.set_sampling(TEMP, so.row_seed(SEED, n), without_replacement=kind == "without_replacement")
    a1 = _fwd(eng1, feed1, mask[n:n + 1])
    for k in keys:
      assert a1[k][0].tobytes() == full[k][n].tobytes(), (n, k)
    L = lens[n]
    u1 = _fwd(eng1, dict(feed1, pred_length=L, obs_lengths=[obs[n]]), mask[n:n + 1])
    for k, ax in {"ids": 1, "logits": 1, "best_beam": 0, "grid_reg": 0}.items():
      a = np.moveaxis(rag[k][n], ax, 0)
      assert (a[L:] == (-1 if k == "ids" else 0)).all(), (n, k)
      want = np.moveaxis(u1[k][0], ax, 0)
      assert np.ascontiguousarray(a[:L]).tobytes() == np.ascontiguousarray(want).tobytes(), (n, k)
    for k in [k for k in keys if k in ("logprobs", "q", "gumbels")]:
      assert rag[k][n].tobytes() == u1[k][0].tobytes(), (n, k)
  eng1.close()


# ---------------------------------------------------------------- 9. occupancy

@pytest.mark.parametrize("kind", KINDS)
def test_occupancy_is_the_masked_mixture(built_lib, kind):
  r = _runs(kind)
  for key in ("A", "B"):
    mask, arrs, dev = r["masks"][key], r[key], r[key + "/occ"]
    N, T, K = dev.shape
    a = np.stack([cm.plane(mask, t) for t in range(T)], axis=1)
    assert (dev[~a] == 0).all()                            # exactly 0 outside A
    assert np.abs(dev.astype(np.float64).sum(-1) - 1).max() <= 1e-5
    uniform = kind == "independent"
    exact = cm.occupancy(arrs["logits"], arrs["logprobs"], mask, uniform, np.float64)
    ref32 = cm.occupancy(arrs["logits"], arrs["logprobs"], mask, uniform, np.float32)
    d_ref = float((np.abs(ref32 - exact)[a] / exact[a]).max())
    d_dev = float((np.abs(dev - exact)[a] / exact[a]).max())
    print("%s/%s: float32 restatement vs fp64 %.3g, device vs fp64 %.3g (bar %.3g)"
          % (kind, key, d_ref, d_dev, 4 * d_ref))
    assert d_dev <= 4 * d_ref                              # the bar of the unmasked occupancy test
  # all ones: the unmasked map, bitwise
  cfg, params, feed = _case("k144")
  eng = _engine(cfg, params, kind)
  _fwd(eng, feed)
  plain = eng.beam_occupancy()
  _fwd(eng, feed, np.ones((cfg.batch_size, 1, _K(cfg)), dtype=np.uint8))
  ones = eng.beam_occupancy()
  eng.close()
  assert plain.tobytes() == ones.tobytes()


def test_any_k_occupancy_and_the_widest_row_form(built_lib):
  """The literal 36 x 22 grid of test_gpu_forward_kinds.py: K = 792 cells take the J = 16 form
  of the step kernels and the any-K form of the occupancy kernel."""
  cfg = synth.default_config(batch_size=2, use_grids=(1, 0), beam_size=3, scene_h=72, scene_w=44,
                             scene_grids=[(36, 22), (18, 11)])
  cfg.max_pred_len = T_PRED
  params = synth.make_params(cfg, seed=synth.SEED_BASE + 91, recurrent_gain=3.0, bias_scale=0.1)
  feed = synth.make_feed(cfg, seed=synth.SEED_BASE + 91, pred_len=T_PRED)
  mask = _half_mask(2, T_PRED, 792)
  for kind in KINDS:
    eng = _engine(cfg, params, kind, "f32")
    arrs = _fwd(eng, feed, mask)
    dev = eng.beam_occupancy()
    eng.close()
    _in_mask(arrs["ids"], mask)
    a = mask != 0
    assert (dev[~a] == 0).all() and np.abs(dev.astype(np.float64).sum(-1) - 1).max() <= 1e-5
    uniform = kind == "independent"
    exact = cm.occupancy(arrs["logits"], arrs["logprobs"], mask, uniform)
    ref32 = cm.occupancy(arrs["logits"], arrs["logprobs"], mask, uniform, np.float32)
    d_ref = float((np.abs(ref32 - exact)[a] / exact[a]).max())
    d_dev = float((np.abs(dev - exact)[a] / exact[a]).max())
    print("k792 %s: float32 restatement vs fp64 %.3g, device vs fp64 %.3g" % (kind, d_ref, d_dev))
    assert d_dev <= 4 * d_ref


# ---------------------------------------------------------------- 10. errors

def test_errors_name_their_cause(built_lib):
  lib = built_lib
  cfg, params, feed = _case("k144")
  N, K, B = cfg.batch_size, _K(cfg), cfg.beam_size
  greedy = synth.default_config(batch_size=2, use_grids=(0, 1), enc_hidden_size=128,
                                dec_hidden_size=128)
  geng = lib.Engine(greedy, device=0)
  with pytest.raises(lib.MvError) as err:
    geng.set_cell_mask(np.ones((N, K), dtype=np.uint8))
  assert "mv_set_cell_mask" in str(err.value) and "beam_size 1" in str(err.value)
  geng.close()
  eng = _engine(cfg, params, "beam")
  ones = np.ones((N, 1, K), dtype=np.uint8)
  u8 = ones.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
  for tm in (0, -2):
    assert eng.lib.mv_set_cell_mask(eng.handle, u8, tm) != 0
    assert "Tm = %d" % tm in eng.lib.mv_last_error(eng.handle).decode()
  with pytest.raises(lib.MvError) as err:
    eng.set_cell_mask(np.ones((N, K + 1), dtype=np.uint8))
  assert "cell_mask" in str(err.value)
  # 1 < Tm < pred_len, at the forward
  with pytest.raises(lib.MvError) as err:
    eng.forward_beam(dict(feed, cell_mask=np.ones((N, 2, K), dtype=np.uint8)))
  assert "Tm = 2" in str(err.value) and "pred_len = 3" in str(err.value)
  # a step without an allowed cell: n, t and the count
  m = np.ones((N, T_PRED, K), dtype=np.uint8)
  m[1, 2] = 0
  with pytest.raises(lib.MvError) as err:
    eng.forward_beam(dict(feed, cell_mask=m))
  assert "n = 1" in str(err.value) and "t = 2" in str(err.value) and "0 allowed" in str(err.value)
  # ... but not below a row's length, and not in a row that does not decode
  m2 = m.copy()
  m2[0] = 0
  arrs = eng.forward_beam(dict(feed, cell_mask=m2, pred_lengths=[0, 2]))[0]
  assert (arrs["ids"][0] == -1).all() and (arrs["ids"][1, :, :2] >= 0).all()
  # fewer than beam_size cells at step 0: the beam and the sampling without replacement
  few = np.ones((N, 1, K), dtype=np.uint8)
  few[0, 0, B - 1:] = 0
  for wor in (None, True, False):
    if wor is not None:
      eng.set_sampling(TEMP, SEED, without_replacement=wor)
    if wor is False:                       # the independent sampler needs one cell only
      _in_mask(eng.forward_beam(dict(feed, cell_mask=few))[0]["ids"], few)
      continue
    with pytest.raises(lib.MvError) as err:
      eng.forward_beam(dict(feed, cell_mask=few))
    assert "n = 0" in str(err.value) and "t = 0" in str(err.value), wor
    assert "%d allowed" % (B - 1) in str(err.value) and "beam_size = %d" % B in str(err.value)
  eng.clear_sampling()
  # the occupancy map under a mask set AFTER the forward: an empty plane at a live step is
  # refused (n, t and the count), below a row's length only
  eng.forward_beam(dict(feed, pred_lengths=[3, 2]))
  eng.set_cell_mask(m)                     # row 1 has no cell at step 2, past its length
  assert np.isfinite(eng.beam_occupancy()).all()
  with pytest.raises(lib.MvError) as err:  # (the direct mask stays: the full forward refuses it)
    eng.forward_beam(feed)
  assert "n = 1" in str(err.value)
  eng.set_cell_mask(None)
  eng.forward_beam(feed)
  eng.set_cell_mask(m)
  with pytest.raises(lib.MvError) as err:
    eng.beam_occupancy()
  msg = str(err.value)
  assert "mv_beam_occupancy" in msg and "n = 1" in msg and "t = 2" in msg and "0 allowed" in msg
  eng.set_cell_mask(None)
  # training and the pipelined greedy forward while a mask is set: the message names the call
  eng.set_cell_mask(ones)
  for call, name in ((eng.train_init, "mv_train_init"), (eng.train_step, "mv_train_step"),
                     (eng.train_forward_backward, "mv_train_forward_backward"),
                     (eng.train_apply, "mv_train_apply")):
    with pytest.raises(lib.MvError) as err:
      call()
    assert name + ":" in str(err.value) and "cell mask" in str(err.value), name
  inp = eng._inputs(dict(feed, cell_mask=ones))           # pylint: disable=protected-access
  assert eng.lib.mv_submit_greedy(eng.handle, ctypes.byref(inp)) != 0
  msg = eng.lib.mv_last_error(eng.handle).decode()
  assert "mv_submit_greedy" in msg and "cell mask" in msg
  eng.set_cell_mask(None)
  assert _same(dict(eng.forward_beam(feed)[0]), dict(eng.forward_beam(feed)[0]))
  eng.close()
  # a grid of more than 1024 cells, at the forward (refused before anything is launched)
  big = synth.default_config(batch_size=1, use_grids=(1, 0), beam_size=2, enc_hidden_size=128,
                             dec_hidden_size=128, scene_h=72, scene_w=64,
                             scene_grids=[(36, 32), (18, 16)])
  big.max_pred_len = T_PRED
  beng = lib.Engine(big, device=0)
  bfeed = synth.make_feed(big, seed=synth.SEED_BASE + 7, pred_len=T_PRED)
  with pytest.raises(lib.MvError) as err:
    beng.forward_beam(dict(bfeed, cell_mask=np.ones((1, 1152), dtype=np.uint8)))
  assert "1152 cells" in str(err.value) and "mv_set_cell_mask" in str(err.value)
  beng.close()
  for op, args in ((lib.op_beam_step, (np.zeros((1, 2, 1100), np.float32), np.zeros((1, 2), np.float32),
                                       2, False, 1.0, 0)),
                   (lib.op_sbs_step, (np.zeros((1, 2, 1100), np.float32),) +
                    (np.zeros((1, 2), np.float32),) * 3 + (1,)),
                   (lib.op_sample_step, (np.zeros((2, 1100), np.float32), 2, 0))):
    with pytest.raises(lib.MvError) as err:
      op(*args, allowed=np.ones((1, 1100), dtype=np.uint8))
    assert "K = 1100" in str(err.value) and "mv_" + op.__name__ in str(err.value), op
