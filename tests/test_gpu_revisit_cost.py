# coding=utf-8
"""GPU: the revisit cost (mv_set_revisit_cost): a per-row penalty for paths that return to a cell
they left, for the beam search, the independent sampler and the sampling without replacement --
the first cost that needs the WHOLE path beside each slot (a bit per cell, carried through the
beam's parent indirection by the step kernels themselves).  The reference has none; the
definition is in include/multiverse_hip.h and restated by
tests/revisit_cost_oracle.py on top of motion_cost_oracle.

Shapes, feed seeds, B and every bar are those of test_gpu_cell_mask.py (its TOL, its near-tie band
and its restatement error); the forwards decode pred_len = max_pred_len = 5 steps, so that a slot's
set passes through more than one parent permutation and a cost is paid with seed_observed off
(nothing can be before t = 2).  The costs of the forward-parity cases come from COST_SEED, the
first seed from 4400 upward for which the restatement ALONE (on the CPU, no device) keeps every
case's (row, step) pairs behind a near tie within a quarter of the case and leaves no beam row
with a tied cut; every beam case also shows, from the restatement alone, a step whose parents are
not the identity and ids that differ from the same forward without the cost.  REVISIT_SEED_COUNTS
lists what the seed leaves uncompared (`parity_cuts` recomputes it).  The bias of the combined
cases follows the cost seed; the feed seeds are test_gpu_cell_mask.py's, none had to move.

Seeds 4400 .. 4429 each fail one of the conditions in at least one of the twelve cases -- nearly
always a combined case (mask + bias + motion) whose beam returns the same ids with and without the
cost, which bites rarely once three other constraints shape the paths; 4400, 4401, 4403 and 4426
also leave a k576 row behind a rank gap of 2e-6.  Seed 4430 leaves nothing uncompared in any case:
0 of 30 (k162: 20) pairs of the independent sampler, 0 of 10 of the sampling without replacement,
no beam row with a tied cut; its beams permute their slots at 1 to 3 of the 4 later steps."""
import ctypes
import functools

import numpy as np
import pytest

from multiverse_amd import multifuture as mf, synth

import cell_bias_oracle as cb
import motion_cost_oracle as mo
import revisit_cost_oracle as ro
import sampling_oracle as so
import sbs_oracle as sbs
import test_gpu_cell_mask as tm
import test_gpu_motion_cost as tmo
from beam_compare import compare_beams, TIE_TOL

pytestmark = pytest.mark.gpu

TOL, TEMP, SEED, KINDS = tm.TOL, tm.TEMP, tm.SEED, tm.KINDS
_K, _engine, _same, _half_mask = tm._K, tm._engine, tm._same, tm._half_mask   # pylint: disable=protected-access
T5 = 5
COST_SEED = 4430
NEVER = mf.MOTION_LIMIT
# (case, compute mode) x seed_observed x (alone | with motion + bias + mask)
PARITY = [("k144", "f16x3"), ("k576", "f16x3"), ("k162", "f16x3"), ("k144", "f32")]
# COST_SEED's (row, step) pairs behind a near tie per (case, seed_observed, combined), from the
# restatement alone, as "independent / without replacement / beam rows with a tied cut" (caps: a
# quarter of N * S * T = 30 or 20, of N * T = 10, and no tied cut); then the beam's steps whose
# parents are not the identity, of T - 1 = 4
REVISIT_SEED_COUNTS = {
    ("k144", True, False): "0 / 0 / 0; 3", ("k144", True, True): "0 / 0 / 0; 2",
    ("k144", False, False): "0 / 0 / 0; 2", ("k144", False, True): "0 / 0 / 0; 2",
    ("k576", True, False): "0 / 0 / 0; 2", ("k576", True, True): "0 / 0 / 0; 3",
    ("k576", False, False): "0 / 0 / 0; 2", ("k576", False, True): "0 / 0 / 0; 3",
    ("k162", True, False): "0 / 0 / 0; 2", ("k162", True, True): "0 / 0 / 0; 1",
    ("k162", False, False): "0 / 0 / 0; 3", ("k162", False, True): "0 / 0 / 0; 2"}


def _grid(cfg):
  s = list(cfg.use_grids).index(True)
  return (s,) + tuple(cfg.scene_grids[s])


def _cfg5(name, batch_size=2, S=None, diverse=True):
  cfg = tm._cfg(name, batch_size, S, diverse)              # pylint: disable=protected-access
  cfg.max_pred_len = T5
  return cfg


@functools.lru_cache(maxsize=None)
def _case5(name, batch_size=2, S=None, feed_seed=None):
  cfg = _cfg5(name, batch_size, S)
  params = synth.make_params(cfg, recurrent_gain=3.0, bias_scale=0.1)
  seed = feed_seed if feed_seed is not None else \
      (tm.CASES[name][3] if batch_size == 2 else synth.SEED_BASE + 84)
  return cfg, params, synth.make_feed(cfg, seed=seed, pred_len=T5)


def _costs(N, seed=COST_SEED):
  """Per-row costs, all distinct and of both signs (a negative cost repels, a positive one
  attracts: either shows a set that is wrong)."""
  vals = np.linspace(-3.0, 3.0, 4 * N).astype(np.float32)
  assert len(set(vals.tolist())) == 4 * N and (vals != 0).all()
  return vals[np.random.RandomState(seed).permutation(4 * N)[:N]].copy()


def _fwd(eng, feed, revisit=None, motion=None, bias=None, mask=None):
  """One forward under the revisit cost ((cost, seed_observed) or None) / motion cost / bias /
  mask given -> its arrays, with the proposal's log-probability under "q" where it sampled."""
  f = dict(feed)
  if revisit is not None:
    f["revisit_cost"] = {"cost": revisit[0], "seed_observed": revisit[1]}
  if motion is not None:
    f["motion_cost"] = motion
  if bias is not None:
    f["cell_bias"] = bias
  if mask is not None:
    f["cell_mask"] = mask
  arrs = dict(eng.forward_beam(f)[0])
  if getattr(eng, "_sampling_on", False):
    arrs["q"] = eng.beam_proposal_logprobs()
  return arrs


# ---------------------------------------------------------------- 1. the step ops

STEP_KW = tmo.STEP_KW                         # (70, 10), (144, 16), (162, 9), (576, 32), (1024, 32)
STEP_R, STEP_S, STEP_T, STEP_SEED = tm.STEP_R, tm.STEP_S, tm.STEP_T, tm.STEP_SEED
STEP_N, STEP_B = tm.STEP_N, tm.STEP_B
SAMPLE_LIMITS = tm.SAMPLE_LIMITS              # (0, 1.0) and (8, 0.9)
TEMPS = (1.0, 0.7)
# (half mask, random bias, motion radius or None)
PLANES = ((False, False, None), (True, False, None), (False, True, None), (False, False, 4),
          (True, True, 1), (True, True, 4))
SETS = ("marked", "empty", "all_but")


def _marks(K):
  """The cells the sets must hold over the rows: the edges of the 32- and 64-cell groups, the
  last cell, and the last bit of the last full word (of 32 and of 64 cells)."""
  return [0, 31, 32, 63, 64, K - 1, 32 * (K // 32) - 1, 64 * (K // 64) - 1]


def _visited(K, W, kind, samples):
  """prev1 [STEP_R] (test_gpu_motion_cost's placements) and visited bool [STEP_R, K] or None.
  marked: row i holds mark i, a random tenth of the cells and prev1[i] itself; rows 0 and 1 hold
  every mark.  all_but: everything but STEP_B + 1 cells (and prev1 counts as visited too)."""
  p1 = tmo._prev(K, W, 0)[0]                               # pylint: disable=protected-access
  if kind == "empty":
    return p1, None
  rng = np.random.RandomState(9100 + K)
  if kind == "all_but":
    v = np.ones((STEP_R, K), dtype=bool)
    for r in range(STEP_R):
      free = rng.choice(np.setdiff1d(np.arange(K), [p1[r]]), STEP_B + 1, replace=False)
      v[r, free] = False
    return p1, v
  v = rng.rand(STEP_R, K) < 0.1
  marks = _marks(K)
  for r in range(STEP_R):
    v[r, marks[r]] = True
    v[r, p1[r]] = True
  v[:2, marks] = True
  return p1, v


def test_the_step_sets_are_what_they_are_named():
  for K, W in STEP_KW:
    p1, v = _visited(K, W, "marked", 4)
    for c in _marks(K):
      assert 0 <= c < K and v[:, c].any(), (K, c)
    assert v[np.arange(STEP_R), p1].all() and 0 < v.sum() < STEP_R * K // 4
    p1, v = _visited(K, W, "all_but", 4)
    assert ((~v).sum(-1) == STEP_B + 1).all() and v[np.arange(STEP_R), p1].all()
    assert _visited(K, W, "empty", 4)[1] is None
    # a cost on prev1 itself would show: rterm is 0 there, the cost elsewhere in the set
    r = ro.rterm(v.reshape(4, 2, K), p1.reshape(4, 2), _step_costs(4))
    assert (r.reshape(STEP_R, K)[np.arange(STEP_R), p1] == 0).all() and (r != 0).sum() > 0


def _step_costs(samples, never=False):
  if never:
    return np.full(samples, NEVER, dtype=np.float32)
  c = np.array([-1.5, 0.75, -3.25, 2.0, -0.5, 1.25, -2.0, 0.25][:samples], dtype=np.float32)
  assert len(set(c.tolist())) == samples
  return c


def _step_case(K, W, planes_on, sets, samples):
  """logits [STEP_R, K], allowed / bias [samples, K] or None, the motion and revisit arguments of
  the ops, and the restatement's per-row planes [STEP_R, K]."""
  mask_on, bias_on, radius = planes_on
  rng = np.random.RandomState(5400 + 7 * K + (radius or 0))
  logits = (4.0 * rng.randn(STEP_R, K)).astype(np.float32)
  allowed = tm._step_mask(K, "half", samples) if mask_on else None   # pylint: disable=protected-access
  bias = (2.0 * rng.randn(samples, K)).astype(np.float32) if bias_on else None
  p1, vis = _visited(K, W, sets, samples)
  p0 = tmo._prev(K, W, 1)[1]                               # pylint: disable=protected-access
  tables = tmo._tables(samples, radius, True, seed=tmo.TABLE_SEED + K) if radius else None   # pylint: disable=protected-access
  cost = _step_costs(samples, never=sets == "all_but")
  per = STEP_R // samples
  v3 = np.zeros((samples, per, K), dtype=bool) if vis is None else vis.reshape(samples, per, K)
  planes = ro.row_planes(p1.reshape(samples, per), p0.reshape(samples, per), v3, W, K, cost,
                         tables, bias)
  motion = dict(tables, W=W, prev1=p1, prev0=p0) if radius else None
  revisit = {"cost": cost, "prev1": p1, "visited": vis}
  stored = ro.stored(v3, p1.reshape(samples, per)).reshape(STEP_R, K)
  return logits, allowed, bias, motion, revisit, planes.reshape(STEP_R, K), stored


def _free(revisit, K):
  """bool [STEP_R, K]: the cells a row may enter under the limit: outside its set, or prev1."""
  f = ~revisit["visited"]
  f[np.arange(STEP_R), revisit["prev1"]] = True
  return f


@pytest.mark.parametrize("K,W", STEP_KW)
def test_sample_step_op_against_the_restatement(built_lib, K, W):
  e32 = tm._restatement_error()            # pylint: disable=protected-access
  tol = 4 * e32                            # the bar of test_gpu_cell_mask.py for this op
  assert tol < 1e-4
  rows = np.arange(STEP_R)
  samples = STEP_R // STEP_S
  worst_lp = worst_q = 0.0
  for planes_on in PLANES:
    for sets in SETS:
      logits, allowed, bias, motion, revisit, planes, stored = _step_case(K, W, planes_on, sets,
                                                                         samples)
      arows = np.ones((STEP_R, K), dtype=bool) if allowed is None else \
          np.repeat(allowed != 0, STEP_S, axis=0)
      for limits in SAMPLE_LIMITS:
        for temp in TEMPS:
          what = (K, planes_on, sets, limits, temp)
          ids, lp, qlp, keep, vout = built_lib.op_sample_step(
              logits, STEP_S, STEP_T, temp, STEP_SEED, limits[0], limits[1], 1, allowed=allowed,
              bias=bias, motion=motion, revisit=revisit)
          assert (vout == stored).all(), what                # visited | {prev1}, exactly
          assert not (keep & ~arows).any() and keep[rows, ids].all(), what
          lp64 = sbs.log_softmax(logits.astype(np.float64))  # the model's, over ALL cells
          dlp = float(np.abs(lp - lp64[rows, ids]).max())
          assert dlp <= tol, (what, dlp, tol)
          if sets == "all_but":
            # "never": no row enters a cell of its set while an allowed cell outside it exists
            can = (_free(revisit, K) & arows).any(-1)
            assert _free(revisit, K)[rows, ids][can].all(), what
            continue
          want = mo.sample_step(logits, STEP_S, STEP_T, allowed, planes, temp, STEP_SEED,
                                limits[0], limits[1], 1, dtype=np.float64)
          band = want["wide"] & ~want["tight"]
          assert (keep == want["tight"])[~band].all(), what
          if limits == (0, 1.0):
            assert (keep == arows).all(), what
          cmp = want["compared"]
          assert (~cmp).sum() * 4 <= STEP_R, what
          assert (ids[cmp] == want["ids"][cmp]).all(), what
          sure = ~band.any(-1)
          assert np.isfinite(qlp).all() and (qlp <= 0).all(), what
          dq = float(np.abs(qlp - want["q"][rows, ids])[sure].max()) if sure.any() else 0.0
          worst_lp, worst_q = max(worst_lp, dlp), max(worst_q, dq)
          assert dq <= tol, (what, dq, tol)
    # zero cost is the motion / the biased / the masked / the plain op, bitwise
    logits, allowed, bias, motion, revisit, _, stored = _step_case(K, W, planes_on, "marked",
                                                                   samples)
    zero = dict(revisit, cost=np.zeros(samples, dtype=np.float32))
    for limits in SAMPLE_LIMITS:
      for temp in TEMPS:
        got = built_lib.op_sample_step(logits, STEP_S, STEP_T, temp, STEP_SEED, limits[0],
                                       limits[1], 1, allowed=allowed, bias=bias, motion=motion,
                                       revisit=zero)
        base = built_lib.op_sample_step(logits, STEP_S, STEP_T, temp, STEP_SEED, limits[0],
                                        limits[1], 1, allowed=allowed, bias=bias, motion=motion)
        for name, a, b in zip(("ids", "lp", "qlp", "keep"), got, base):
          assert a.tobytes() == b.tobytes(), (K, planes_on, limits, temp, name)
        assert (got[4] == stored).all()
  print("K=%d: float32 restatement vs float64 %.3g -> bar %.3g; device: logprob %.3g, "
        "proposal %.3g" % (K, e32, tol, worst_lp, worst_q))


def _beam_case(K, W, planes_on, sets):
  logits, allowed, bias, motion, revisit, planes, stored = _step_case(K, W, planes_on, sets, STEP_N)
  prev = -np.random.RandomState(7000 + K).rand(STEP_N, STEP_B).astype(np.float32)
  return (logits.reshape(STEP_N, STEP_B, K), prev, allowed, bias, motion, revisit,
          planes.reshape(STEP_N, STEP_B, K), stored.reshape(STEP_N, STEP_B, K))


def _ran(stored, revisit, K, first):
  """The sets the op reports: a slot > 0 of a first step does not run and keeps its set as given."""
  if not first:
    return stored
  out = stored.copy()
  given = np.zeros_like(stored) if revisit["visited"] is None else \
      revisit["visited"].reshape(stored.shape)
  out[:, 1:] = given[:, 1:]
  return out


def _entered_free(ids, parents, revisit, allowed, K):
  """Under the limit every slot that could be filled from outside its parent's set was."""
  free = _free(revisit, K).reshape(STEP_N, STEP_B, K)
  return free[np.arange(STEP_N)[:, None], parents, ids].all()


@pytest.mark.parametrize("K,W", STEP_KW)
def test_beam_step_op_against_the_restatement(built_lib, K, W):
  tol = 4 * tm._restatement_error()        # pylint: disable=protected-access
  for planes_on in PLANES:
    for sets in SETS:
      logits, prev, allowed, bias, motion, revisit, planes, stored = _beam_case(K, W, planes_on, sets)
      for time in (1, 2):
        for diverse in (False, True):
          what = (K, planes_on, sets, time, diverse)
          new_lp, ids, parents, vout = built_lib.op_beam_step(
              logits, prev, time, diverse, 0.01, 0, allowed=allowed, bias=bias, motion=motion,
              revisit=revisit)
          assert (vout == _ran(stored, revisit, K, time <= 1)).all(), what
          want = mo.beam_step(logits, prev, allowed, planes, time, diverse, 0.01, 0,
                              dtype=np.float64)
          if allowed is not None:
            assert (allowed[np.arange(STEP_N)[:, None], ids] != 0).all(), what
          assert np.isfinite(new_lp).all(), what
          if sets == "all_but":
            # "never": with B + 1 cells outside every row's set no slot has to enter one (under
            # a mask as well a slot may have to: defined, and not compared here)
            if allowed is None:
              assert _entered_free(ids, parents, revisit, allowed, K), what
              assert np.abs(new_lp).max() < 1e29, what
            else:
              continue
          cmp = want["gap"] >= ro.GAP_BAR
          assert (~cmp).sum() * 4 <= STEP_N, what
          assert (ids[cmp] == want["ids"][cmp]).all() and \
              (parents[cmp] == want["parents"][cmp]).all(), what
          ok = cmp[:, None] & (np.abs(want["new_lp"]) < 1e29)   # (a forced -1e30 rounds in float32)
          d = float(np.abs(new_lp - want["new_lp"])[ok].max()) if ok.any() else 0.0
          assert d <= tol, (what, d, tol)
    logits, prev, allowed, bias, motion, revisit, _, stored = _beam_case(K, W, planes_on, "marked")
    zero = dict(revisit, cost=np.zeros(STEP_N, dtype=np.float32))
    for time in (1, 2):
      for diverse in (False, True):
        got = built_lib.op_beam_step(logits, prev, time, diverse, 0.01, 0, allowed=allowed,
                                     bias=bias, motion=motion, revisit=zero)
        base = built_lib.op_beam_step(logits, prev, time, diverse, 0.01, 0, allowed=allowed,
                                      bias=bias, motion=motion)
        for a, b in zip(got, base):
          assert a.tobytes() == b.tobytes(), (K, planes_on, time, diverse)


@pytest.mark.parametrize("K,W", STEP_KW)
def test_sbs_step_op_against_the_restatement(built_lib, K, W):
  tol = 4 * tm._restatement_error()        # pylint: disable=protected-access
  rng = np.random.RandomState(8000 + K)
  phi, LP, G = (-rng.rand(STEP_N, STEP_B).astype(np.float32) for _ in range(3))
  for planes_on in PLANES:
    for sets in SETS:
      logits, _, allowed, bias, motion, revisit, planes, stored = _beam_case(K, W, planes_on, sets)
      for t in (0, 1):
        for temp in TEMPS:
          what = (K, planes_on, sets, t, temp)
          got = built_lib.op_sbs_step(logits, phi, LP, G, t, temp, STEP_SEED, allowed=allowed,
                                      bias=bias, motion=motion, revisit=revisit)
          nphi, nlp, ng, ids, parents, vout = got
          assert (vout == _ran(stored, revisit, K, t == 0)).all(), what
          if allowed is not None:
            assert (allowed[np.arange(STEP_N)[:, None], ids] != 0).all(), what
          if sets == "all_but":
            # "never": exp of such a cell's proposal weight is exactly 0; with B + 1 cells outside
            # every row's set no slot has to take one (under a mask as well a slot may have to)
            if allowed is None:
              assert _entered_free(ids, parents, revisit, allowed, K), what
              assert all(np.isfinite(a).all() for a in (nlp, ng)), what
            continue
          assert all(np.isfinite(a).all() for a in (nlp, ng)), what
          assert np.isfinite(nphi).all(), what
          want = mo.sbs_step(logits, phi, LP, G, t, allowed, planes, temp, STEP_SEED,
                             dtype=np.float64)
          cmp = want["gap"] >= ro.GAP_BAR
          assert (~cmp).sum() * 4 <= STEP_N, what
          assert (ids[cmp] == want["ids"][cmp]).all() and \
              (parents[cmp] == want["parents"][cmp]).all(), what
          for a, key in ((nphi, "new_phi"), (nlp, "new_lp"), (ng, "new_g")):
            d = float(np.abs(a - want[key])[cmp].max()) if cmp.any() else 0.0
            assert d <= max(tol, 2e-5), (what, key, d, tol)   # the bar of the masked op
    logits, _, allowed, bias, motion, revisit, _, stored = _beam_case(K, W, planes_on, "marked")
    zero = dict(revisit, cost=np.zeros(STEP_N, dtype=np.float32))
    for t in (0, 1):
      for temp in TEMPS:
        got = built_lib.op_sbs_step(logits, phi, LP, G, t, temp, STEP_SEED, allowed=allowed,
                                    bias=bias, motion=motion, revisit=zero)
        base = built_lib.op_sbs_step(logits, phi, LP, G, t, temp, STEP_SEED, allowed=allowed,
                                     bias=bias, motion=motion)
        for a, b in zip(got, base):
          assert a.tobytes() == b.tobytes(), (K, planes_on, t, temp)


# ---------------------------------------------------------------- 2. forward parity

@functools.lru_cache(maxsize=None)
def _others(name, combined, seed=COST_SEED):
  """The motion tables, bias and mask of a combined case (None, None, None alone); the bias
  follows the cost seed."""
  if not combined:
    return None, None, None
  cfg = _cfg5(name)
  N, K = cfg.batch_size, _K(cfg)
  bias = (2.0 * np.random.RandomState(seed + 5).randn(N, T5, K)).astype(np.float32)
  return tmo._tables(N, 2, True), bias, _half_mask(N, T5, K)   # pylint: disable=protected-access


@functools.lru_cache(maxsize=None)
def _want(name, seed_observed, combined, kind, seed=COST_SEED, with_cost=True):
  """The restatement's forward of one case, computed once for every compute mode."""
  cfg, params, feed = _case5(name)
  cost = _costs(cfg.batch_size, seed) if with_cost else np.zeros(cfg.batch_size, np.float32)
  tables, bias, mask = _others(name, combined, seed)
  if kind == "independent":
    return ro.sampled_forward(params, cfg, feed, cost, seed_observed, tables, mask, bias,
                              temperature=TEMP, seed=SEED)
  if kind == "without_replacement":
    return ro.sbs_forward(params, cfg, feed, cost, seed_observed, tables, mask, bias,
                          temperature=TEMP, seed=SEED)
  return ro.beam_forward(params, cfg, feed, cost, seed_observed, tables, mask, bias)


def parity_cuts(name, seed_observed, combined, seed=COST_SEED):
  """What the restatement ALONE leaves uncompared in one case (no device) -> ((cut, of),
  (cut, of), (beam rows with a tied cut, of), beam steps whose parents are not the identity,
  whether the beam's ids differ from the forward without the cost).  This is what COST_SEED was
  picked by."""
  cfg = _cfg5(name)
  N, S, T = cfg.batch_size, cfg.beam_size, T5
  want = _want(name, seed_observed, combined, "independent", seed)
  ind = int((T - cb.to.compared_steps(want["compared"])).sum())
  want = _want(name, seed_observed, combined, "without_replacement", seed)
  wor = int((T - sbs.compared_steps(want["gap"])).sum())
  _, (_, oids, _), trace = _want(name, seed_observed, combined, "beam", seed)
  gap = np.minimum(np.stack(trace["beam_step_cut_gap"], axis=1),
                   np.stack(trace["beam_step_rank_gap"], axis=1))
  moved = sum(int((p != np.arange(S)[None]).any()) for p in trace["step_parents_np"][1:])
  plain = _want(name, seed_observed, combined, "beam", seed, False)[1][1]
  return ((ind, N * S * T), (wor, N * T), (int((gap < TIE_TOL).any(axis=1).sum()), N), moved,
          bool((np.asarray(plain) != np.asarray(oids)).any()))


def _check_sampled(name, mode, seed_observed, combined):
  cfg, params, feed = _case5(name)
  want = _want(name, seed_observed, combined, "independent")
  tables, bias, mask = _others(name, combined)
  eng = _engine(cfg, params, "independent", mode)
  arrs = _fwd(eng, feed, (_costs(cfg.batch_size), seed_observed), tables, bias, mask)
  eng.close()
  N, S, T = cfg.batch_size, cfg.beam_size, T5
  upto = cb.to.compared_steps(want["compared"])
  cut = int((T - upto).sum())
  print("%s/%s/seed=%s/combined=%s: %d of %d (row, step) pairs behind a step that is not compared"
        % (name, mode, seed_observed, combined, cut, N * S * T))
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


def _check_sbs(name, mode, seed_observed, combined):
  cfg, params, feed = _case5(name)
  want = _want(name, seed_observed, combined, "without_replacement")
  tables, bias, mask = _others(name, combined)
  eng = _engine(cfg, params, "without_replacement", mode)
  arrs = _fwd(eng, feed, (_costs(cfg.batch_size), seed_observed), tables, bias, mask)
  eng.close()
  N, B, T = cfg.batch_size, cfg.beam_size, T5
  upto = sbs.compared_steps(want["gap"])
  cut = int((T - upto).sum())
  print("%s/%s/seed=%s/combined=%s: %d of %d (row, step) pairs behind a gap below 1e-4"
        % (name, mode, seed_observed, combined, cut, N * T))
  assert cut * 4 <= N * T
  for n in range(N):
    u = int(upto[n])
    if u == T:
      assert (arrs["ids"][n] == want["ids"][n]).all(), n
      for b in range(B):
        assert np.abs(arrs["logits"][n, b] -
                      tmo._beam_traced_logits(want, n, b, T)).max() < TOL   # pylint: disable=protected-access
      assert np.abs(arrs["logprobs"][n] - want["logprobs"][n]).max() < TOL * T
      assert np.abs(arrs["gumbels"][n] - want["gumbels"][n]).max() < TOL
      continue
    paths = {} if u == 0 else {tuple(sbs.trace_back(want, n, j, u)[0]): j for j in range(B)}
    for b in range(B):
      j = 0 if u == 0 else paths.get(tuple(arrs["ids"][n, b, :u]))
      assert j is not None, (n, b)
  assert np.abs(arrs["grid_reg"] - want["grid_reg"]).max() < TOL


def _check_beam(name, mode, seed_observed, combined):
  cfg, params, feed = _case5(name)
  oreg, (ologits, oids, olp), trace = _want(name, seed_observed, combined, "beam")
  tables, bias, mask = _others(name, combined)
  s = list(cfg.use_grids).index(True)
  eng = _engine(cfg, params, "beam", mode)
  arrs = _fwd(eng, feed, (_costs(cfg.batch_size), seed_observed), tables, bias, mask)
  eng.close()
  cut_gap = np.minimum(np.stack(trace["beam_step_cut_gap"], axis=1),
                       np.stack(trace["beam_step_rank_gap"], axis=1))
  assert not (cut_gap < TIE_TOL).any()                     # what COST_SEED was picked by
  compare_beams(arrs, oreg[s].numpy() if hasattr(oreg[s], "numpy") else oreg[s], ologits, oids,
                olp, np.stack(trace["beam_step_topvals"], axis=-1), trace["beam_trace"],
                cut_gap=cut_gap)
  assert compare_beams.unmatched == 0
  # the set went through a parent permutation, and the cost bites
  assert any((p != np.arange(cfg.beam_size)[None]).any() for p in trace["step_parents_np"][1:])
  plain = _want(name, seed_observed, combined, "beam", COST_SEED, False)[1][1]
  assert (np.asarray(plain) != np.asarray(oids)).any()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("combined", [False, True])
@pytest.mark.parametrize("seed_observed", [True, False])
@pytest.mark.parametrize("name,mode", PARITY)
def test_parity_with_the_oracle(built_lib, name, mode, seed_observed, combined, kind):
  {"beam": _check_beam, "independent": _check_sampled, "without_replacement": _check_sbs}[kind](
      name, mode, seed_observed, combined)


# ---------------------------------------------------------------- 3. behaviour

# (case, feed seed; None: the case's own) whose plain beam of B = 4 re-enters a cell it left, from
# the oracle alone: the first tried
LOOP_CASE = ("k144", None)


@functools.lru_cache(maxsize=None)
def _loop_case():
  return _case5(LOOP_CASE[0], 2, 4, LOOP_CASE[1])


def loops_without_a_cost(name, feed_seed):
  """From the oracle alone (no device): does a path of the plain beam of B = 4 re-enter a cell
  it left?  This is what LOOP_CASE was picked by."""
  cfg, params, feed = _case5(name, 2, 4, feed_seed)
  s = _grid(cfg)[0]
  oids = ro.beam_forward(params, cfg, feed, np.zeros(cfg.batch_size, np.float32))[1][1]
  return bool(mf.path_revisit_cost(np.asarray(oids), feed["grid_obs_labels"][s], 1.0).any())


@pytest.mark.parametrize("kind", KINDS)
def test_never_holds_and_is_not_vacuous(built_lib, kind):
  cfg, params, feed = _loop_case()
  s = _grid(cfg)[0]
  labels = feed["grid_obs_labels"][s]
  eng = _engine(cfg, params, kind)
  held = _fwd(eng, feed, (NEVER, True))
  eng.set_revisit_cost(None)
  free = _fwd(eng, feed)
  eng.close()
  assert (mf.path_revisit_cost(held["ids"], labels, 1.0) == 0).all(), held["ids"]
  assert np.abs(held["logprobs"]).max() < 1e29             # no slot had to enter a visited cell
  if kind == "beam":                                       # once cleared, a path loops again
    assert mf.path_revisit_cost(free["ids"], labels, 1.0).any()


# ---------------------------------------------------------------- 4. zero cost, graph replay

@functools.lru_cache(maxsize=None)
def _runs(kind):
  """One handle: eager forwards under costs A, A2 (other values), A with seed_observed off, zero
  and none, then the same in graph mode; and a handle that never had a revisit cost."""
  cfg, params, feed = _case5("k144")
  N = cfg.batch_size
  A, A2 = _costs(N), _costs(N, COST_SEED + 1)
  assert not (A == A2).all()
  zero = np.zeros(N, dtype=np.float32)
  eng = _engine(cfg, params, kind)
  r = {}
  for key, c in (("A", (A, True)), ("A2", (A2, True)), ("Aoff", (A, False)), ("zero", (zero, True)),
                 ("zero_off", (zero, False))):
    r[key] = _fwd(eng, feed, c)
  r["none"] = _fwd(eng, feed)
  eng.set_graph_mode(True)
  caps = [eng.graph_captures()]
  for key, c in (("gA", (A, True)), ("gA2", (A2, True)), ("gA3", (A, True)), ("gzero", (zero, True)),
                 ("gnone", None), ("gAoff", (A, False)), ("gA5", (A, True))):
    r[key] = _fwd(eng, feed, c)
    caps.append(eng.graph_captures())
  r["captures"] = caps
  eng.close()
  fresh = _engine(cfg, params, kind)
  r["fresh"] = _fwd(fresh, feed)
  fresh.set_graph_mode(True)
  fcaps = [fresh.graph_captures()]
  r["gfresh"] = _fwd(fresh, feed)
  r["gfresh2"] = _fwd(fresh, feed)
  fcaps.append(fresh.graph_captures())
  r["fresh_captures"] = fcaps
  fresh.close()
  return r


@pytest.mark.parametrize("kind", KINDS)
def test_zero_cost_is_bitwise_a_handle_that_never_had_one(built_lib, kind):
  r = _runs(kind)
  keys = sorted(r["fresh"])
  assert _same(r["zero"], r["fresh"], keys) and _same(r["none"], r["fresh"], keys)
  assert _same(r["zero_off"], r["fresh"], keys)
  assert _same(r["gzero"], r["gfresh"], keys) and _same(r["gnone"], r["gfresh"], keys)
  assert _same(r["fresh"], r["gfresh"], keys) and _same(r["gfresh2"], r["gfresh"], keys)
  assert r["fresh_captures"] == [0, 1]     # no cost set: one graph, as ever
  if kind != "beam":                       # under a cost the forwards report the proposal as well
    assert "proposal_logprobs" in r["zero"] and "proposal_logprobs" not in r["none"]
    assert r["zero"]["proposal_logprobs"].tobytes() == r["zero"]["q"].tobytes()
  assert not (r["A"]["ids"] == r["none"]["ids"]).all()       # ... and a real cost bites
  assert r["A"]["logits"][:, :, 0].tobytes() == r["none"]["logits"][:, :, 0].tobytes()


@pytest.mark.parametrize("kind", KINDS)
def test_a_replayed_graph_follows_the_cost_without_recapture(built_lib, kind):
  r = _runs(kind)
  for g, e in (("gA", "A"), ("gA2", "A2"), ("gA3", "A"), ("gAoff", "Aoff"), ("gA5", "A")):
    assert _same(r[g], r[e]), (g, e)
  assert not (r["A"]["ids"] == r["A2"]["ids"]).all()
  assert not _same(r["A"], r["Aoff"])
  # captures: gA one graph; other VALUES, A again and zero replay it; none is the plain graph;
  # seed_observed off is a third; A again replays the first
  c = r["captures"]
  assert [b - a for a, b in zip(c[:-1], c[1:])] == [1, 0, 0, 0, 1, 1, 0], c


@pytest.mark.parametrize("kind", KINDS)
def test_a_cost_set_on_the_engine_stays_through_feeds_without_the_key(built_lib, kind):
  cfg, params, feed = _case5("k144")
  N = cfg.batch_size
  cost, other = _costs(N), _costs(N, COST_SEED + 1)
  eng = _engine(cfg, params, kind)
  by_feed = _fwd(eng, feed, (cost, True))
  plain = _fwd(eng, feed)                  # a feed without the key clears what a FEED set
  eng.set_revisit_cost(cost)               # (seed_observed defaults to True)
  first, second = _fwd(eng, feed), _fwd(eng, feed)         # ... and not what was set directly
  third = _fwd(eng, feed, (other, True))   # a feed's own cost replaces it, and then follows
  fourth = _fwd(eng, feed)                 # the feeds' rule
  eng.set_revisit_cost(float(cost[0]))     # a scalar is taken for every row
  broadcast = _fwd(eng, feed)
  eng.set_revisit_cost(None)
  fifth = _fwd(eng, feed)
  eng.close()
  assert _same(first, by_feed) and _same(second, by_feed)
  assert not _same(third, by_feed) and not _same(plain, by_feed)
  assert _same(fourth, plain) and _same(fifth, plain)
  assert broadcast["ids"][0].tobytes() == by_feed["ids"][0].tobytes()


# ---------------------------------------------------------------- 5. the scores

@pytest.mark.parametrize("combined", [False, True])
def test_the_beam_score_is_the_models_plus_what_the_path_paid(built_lib, combined):
  params, feed = _case5("k144")[1:]
  cfg = _cfg5("k144", diverse=False)
  s, _, W = _grid(cfg)
  N, B, T, K = cfg.batch_size, cfg.beam_size, T5, _K(cfg)
  cost = np.array([-2.5, 1.75], dtype=np.float32)
  tables, bias, _ = _others("k144", combined)
  labels = feed["grid_obs_labels"][s]
  eng = _engine(cfg, params, "beam")
  arrs = _fwd(eng, feed, (cost, True), tables, bias)
  ids = arrs["ids"]
  # the model's step log-probabilities along each returned path: the teacher-forced scorer
  model = eng.score_futures(feed, ids)["step_logprobs"].astype(np.float64)
  eng.close()
  paid = mf.path_revisit_cost(ids, labels, cost).astype(np.float64)
  assert np.abs(paid).max() > 0.5                          # a revisit was paid for
  if combined:
    paid += mf.path_motion_cost(ids, labels, W, tables).astype(np.float64)
    paid += np.take_along_axis(np.broadcast_to(bias[:, None], (N, B, T, K)).astype(np.float64),
                               ids[..., None].astype(np.int64), axis=-1)[..., 0]
  live = np.arange(T) >= cfg.fix_num_timestep
  got = arrs["logprobs"].astype(np.float64) - (paid * live).sum(-1)
  assert np.abs(got - (model * live).sum(-1)).max() < TOL * T


@pytest.mark.parametrize("kind", ["independent", "without_replacement"])
def test_the_scorer_returns_the_logprobs_under_a_cost(built_lib, kind):
  cfg, params, feed = _case5("k144")
  cost = (_costs(cfg.batch_size), True)
  key = {"revisit_cost": {"cost": cost[0], "seed_observed": True}}
  eng = _engine(cfg, params, kind)
  arrs = _fwd(eng, feed, cost)
  # the cost is still set while scoring, through the feed or directly: it is neither read ...
  scored = eng.score_futures(dict(feed, **key), arrs["ids"])
  again = _fwd(eng, feed, cost)
  eng.set_revisit_cost(*cost)
  direct = eng.score_futures(feed, arrs["ids"])
  kept = _fwd(eng, feed)                   # ... nor cleared by a feed without the key
  eng.close()
  assert scored["logprobs"].tobytes() == arrs["logprobs"].tobytes()
  assert direct["logprobs"].tobytes() == arrs["logprobs"].tobytes()
  assert _same(again, arrs) and _same(kept, arrs)          # ... and not changed
  assert np.isfinite(arrs["q"]).all() and (arrs["q"] <= 0).all()
  assert not (arrs["q"] == arrs["logprobs"]).all()         # the proposal is not the model


# ---------------------------------------------------------------- 6. batch, lengths, short tracks

@pytest.mark.parametrize("seed_observed", [True, False])
@pytest.mark.parametrize("kind", KINDS)
def test_rows_are_their_own_uniform_forwards_under_their_own_cost(built_lib, kind, seed_observed):
  """Row 1 is observed for ONE frame (its set starts from that cell alone) beside row 2 with
  two and row 0 with all eight."""
  lens, obs = (5, 4, 2), (8, 1, 2)
  cfg3, params, feed3 = _case5("k144", 3)
  K = _K(cfg3)
  cost = _costs(3)
  tables = tmo._tables(3, 2, True)                         # pylint: disable=protected-access
  bias = (2.0 * np.random.RandomState(COST_SEED + 6).randn(3, T5, K)).astype(np.float32)
  mask = _half_mask(3, T5, K)
  eng = _engine(cfg3, params, kind)
  full = _fwd(eng, feed3, (cost, seed_observed), tables, bias, mask)
  rag = _fwd(eng, dict(feed3, pred_lengths=list(lens), obs_lengths=list(obs)),
             (cost, seed_observed), tables, bias, mask)
  eng.close()
  keys = ["ids", "logits", "logprobs", "grid_reg", "best_beam"] + \
      ([] if kind == "beam" else ["q"]) + (["gumbels"] if kind == "without_replacement" else [])
  eng1 = _engine(_cfg5("k144", batch_size=1), params, kind)
  for n in range(3):
    feed1 = dict(feed3, obs_scene=feed3["obs_scene"][n:n + 1],
                 grid_obs_labels=[a[n:n + 1] for a in feed3["grid_obs_labels"]],
                 grid_obs_regress=[a[n:n + 1] for a in feed3["grid_obs_regress"]])
    t1 = {k: (v[n:n + 1] if isinstance(v, np.ndarray) else v) for k, v in tables.items()}
    c1 = (cost[n:n + 1], seed_observed)
    if kind != "beam":
      eng1.set_sampling(TEMP, so.row_seed(SEED, n), without_replacement=kind == "without_replacement")
    a1 = _fwd(eng1, feed1, c1, t1, bias[n:n + 1], mask[n:n + 1])
    for k in keys:
      assert a1[k][0].tobytes() == full[k][n].tobytes(), (n, k)
    L = lens[n]
    u1 = _fwd(eng1, dict(feed1, pred_length=L, obs_lengths=[obs[n]]), c1, t1, bias[n:n + 1],
              mask[n:n + 1])
    for k, ax in {"ids": 1, "logits": 1, "best_beam": 0, "grid_reg": 0}.items():
      a = np.moveaxis(rag[k][n], ax, 0)
      assert (a[L:] == (-1 if k == "ids" else 0)).all(), (n, k)
      want = np.moveaxis(u1[k][0], ax, 0)
      assert np.ascontiguousarray(a[:L]).tobytes() == np.ascontiguousarray(want).tobytes(), (n, k)
    for k in [k for k in keys if k in ("logprobs", "q", "gumbels")]:
      assert rag[k][n].tobytes() == u1[k][0].tobytes(), (n, k)
  eng1.close()


# ---------------------------------------------------------------- 7. errors

def test_errors_name_their_cause(built_lib):
  lib = built_lib
  cfg, params, feed = _case5("k144")
  N = cfg.batch_size
  good = _costs(N)
  greedy = synth.default_config(batch_size=2, use_grids=(0, 1), enc_hidden_size=128,
                                dec_hidden_size=128)
  geng = lib.Engine(greedy, device=0)
  with pytest.raises(lib.MvError) as err:
    geng.set_revisit_cost(good)
  assert "mv_set_revisit_cost" in str(err.value) and "beam_size 1" in str(err.value)
  geng.close()
  eng = _engine(cfg, params, "beam")
  before = dict(eng.forward_beam(feed)[0])
  # a value that is not finite: the message names n
  for n in range(N):
    for bad in (np.nan, np.inf, -np.inf):
      c = good.copy()
      c[n] = bad
      with pytest.raises(lib.MvError) as err:
        eng.set_revisit_cost(c)
      msg = str(err.value)
      assert "mv_set_revisit_cost" in msg and "cost[n = %d]" % n in msg and "finite" in msg
  with pytest.raises(lib.MvError) as err:
    eng.set_revisit_cost(np.zeros(N + 1, dtype=np.float32))
  assert "revisit_cost" in str(err.value) and "shape" in str(err.value)
  assert _same(dict(eng.forward_beam(feed)[0]), before)     # a refused cost is not set
  # training, the pipelined greedy forward and the occupancy map while a cost is set
  eng.set_revisit_cost(good)
  for call, name in ((eng.train_init, "mv_train_init"), (eng.train_step, "mv_train_step"),
                     (eng.train_forward_backward, "mv_train_forward_backward"),
                     (eng.train_apply, "mv_train_apply")):
    with pytest.raises(lib.MvError) as err:
      call()
    assert name + ":" in str(err.value) and "revisit cost" in str(err.value), name
  inp = eng._inputs(feed)                                  # pylint: disable=protected-access
  assert eng.lib.mv_submit_greedy(eng.handle, ctypes.byref(inp)) != 0
  msg = eng.lib.mv_last_error(eng.handle).decode()
  assert "mv_submit_greedy" in msg and "revisit cost" in msg
  eng.forward_beam(feed)
  with pytest.raises(lib.MvError) as err:
    eng.beam_occupancy()
  assert "mv_beam_occupancy" in str(err.value) and "revisit cost" in str(err.value)
  eng.set_revisit_cost(None)
  assert eng.beam_occupancy().shape[0] == N                # cleared: the map is back
  assert _same(dict(eng.forward_beam(feed)[0]), before)
  eng.close()
  # a grid of more than 1024 cells, at the forward (refused before anything is launched)
  wide = synth.default_config(batch_size=1, use_grids=(1, 0), beam_size=2, enc_hidden_size=128,
                              dec_hidden_size=128, scene_h=72, scene_w=64,
                              scene_grids=[(36, 32), (18, 16)])
  wide.max_pred_len = T5
  weng = lib.Engine(wide, device=0)
  wfeed = synth.make_feed(wide, seed=synth.SEED_BASE + 7, pred_len=T5)
  with pytest.raises(lib.MvError) as err:
    weng.forward_beam(dict(wfeed, revisit_cost={"cost": -1.0}))
  assert "1152 cells" in str(err.value) and "mv_set_revisit_cost" in str(err.value)
  weng.close()
  # the ops: K beyond a wave, a value that is not finite, a cell outside the grid
  rev = {"cost": np.zeros(1, np.float32), "prev1": np.zeros(2, np.int32)}
  for op, args in ((lib.op_beam_step, (np.zeros((1, 2, 1100), np.float32), np.zeros((1, 2), np.float32),
                                       2, False, 1.0, 0)),
                   (lib.op_sbs_step, (np.zeros((1, 2, 1100), np.float32),) +
                    (np.zeros((1, 2), np.float32),) * 3 + (1,)),
                   (lib.op_sample_step, (np.zeros((2, 1100), np.float32), 2, 0))):
    with pytest.raises(lib.MvError) as err:
      op(*args, revisit=rev)
    assert "K = 1100" in str(err.value) and "mv_" + op.__name__ + "_path" in str(err.value), op
    small = tuple(a[..., :70] if isinstance(a, np.ndarray) and a.shape[-1] == 1100 else a
                  for a in args)
    for change, word in ((dict(cost=np.full(1, np.nan, np.float32)), "cost[n = 0]"),
                         (dict(prev1=np.array([0, 70], np.int32)), "prev1[1] = 70"),
                         (dict(prev1=np.array([-1, 0], np.int32)), "prev1[0] = -1")):
      with pytest.raises(lib.MvError) as err:
        op(*small, revisit=dict(rev, **change))
      assert word in str(err.value), (op, word, str(err.value))
