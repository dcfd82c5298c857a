# coding=utf-8
"""GPU: the motion costs (mv_set_motion_cost): per-row speed and turn priors for the beam search,
the independent sampler and the sampling without replacement -- a cell bias whose plane each
wave derives from its own row's path.  The reference has none; the definition is in
include/multiverse_hip.h and restated by tests/motion_cost_oracle.py on top of
cell_bias_oracle.

Shapes, cases, feed seeds, B and every bar are those of test_gpu_cell_mask.py (its TOL, its
near-tie band and its restatement error).  The tables of the forward-parity cases come from
TABLE_SEED, the first seed from 4300 upward for which the restatement ALONE (on the CPU, no
device) keeps every case's (row, step) pairs behind a near tie within a quarter of the case;
MOTION_SEED_COUNTS lists what that seed leaves uncompared (`parity_cuts` recomputes it).

Seed 4300, the first tried, leaves nothing uncompared in any of the seven cases: 0 of 18 (k162: 12)
(row, step) pairs of the independent sampler, 0 of 6 of the sampling without replacement, and no
beam row with a cut or a rank gap below the tie bar."""
import ctypes
import functools

import numpy as np
import pytest

from multiverse_amd import multifuture as mf, synth

import cell_bias_oracle as cb
import motion_cost_oracle as mo
import sampling_oracle as so
import sbs_oracle as sbs
import test_gpu_cell_mask as tm
from beam_compare import compare_beams, TIE_TOL

pytestmark = pytest.mark.gpu

TOL, T_PRED, TEMP, SEED, KINDS = tm.TOL, tm.T_PRED, tm.TEMP, tm.SEED, tm.KINDS
_case, _cfg, _K, _engine, _same, _half_mask = (tm._case, tm._cfg, tm._K, tm._engine, tm._same,  # pylint: disable=protected-access
                                               tm._half_mask)                                 # pylint: disable=protected-access
TABLE_SEED = 4300
LIMIT = mf.motion_tables(2, max_step=1)       # "at most one cell per step", no other cost
# (case, compute mode, radius, acc) of the forward parity
PARITY = [("k144", "f16x3", 2, True), ("k144", "f16x3", 1, False), ("k144", "f32", 4, True),
          ("k576", "f16x3", 2, True), ("k576", "f16x3", 4, False), ("k162", "f16x3", 2, True),
          ("k162", "f16x3", 1, False)]
# TABLE_SEED's (row, step) pairs behind a near tie per case, from the restatement alone, as
# "independent / without replacement / beam rows with a tied cut" (caps: a quarter of
# N * S * T = 18 or 12, of N * T = 6, and no tied cut)
MOTION_SEED_COUNTS = {
    ("k144", 2, True): "0 / 0 / 0", ("k144", 1, False): "0 / 0 / 0", ("k144", 4, True): "0 / 0 / 0",
    ("k576", 2, True): "0 / 0 / 0", ("k576", 4, False): "0 / 0 / 0", ("k162", 2, True): "0 / 0 / 0",
    ("k162", 1, False): "0 / 0 / 0"}


def _grid(cfg):
  s = list(cfg.use_grids).index(True)
  return (s,) + tuple(cfg.scene_grids[s])


def _tables(N, radius, acc, seed=TABLE_SEED, scale=3.0):
  """Per-row tables whose entries are ALL distinct (a permutation of an even spacing over
  [-scale, scale]): a wrapped column, a transposed index or another row's table shows."""
  D = 2 * radius + 1
  count = N * (D * D + 1) * (2 if acc else 1)
  vals = np.linspace(-scale, scale, count).astype(np.float32)
  assert len(set(vals.tolist())) == count
  vals = vals[np.random.RandomState(seed + 10 * radius + int(acc)).permutation(count)]
  cut = [N * D * D, N * D * D + N, 2 * N * D * D + N]
  t = {"radius": radius, "vel": vals[:cut[0]].reshape(N, D, D).copy(),
       "vel_far": vals[cut[0]:cut[1]].copy(), "acc": None, "acc_far": None}
  if acc:
    t["acc"] = vals[cut[1]:cut[2]].reshape(N, D, D).copy()
    t["acc_far"] = vals[cut[2]:].copy()
  return t


def _zero_tables(N, radius, acc):
  D = 2 * radius + 1
  z = lambda *s: np.zeros(s, dtype=np.float32)
  return {"radius": radius, "vel": z(N, D, D), "vel_far": z(N),
          "acc": z(N, D, D) if acc else None, "acc_far": z(N) if acc else None}


def _fwd(eng, feed, motion=None, bias=None, mask=None):
  """One forward under the motion cost / bias / mask given (None: none) -> its arrays, with the
  proposal's log-probability under "q" where the forward sampled."""
  f = dict(feed)
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

STEP_KW = [(70, 10), (144, 16), (162, 9), (576, 32), (1024, 32)]   # J = 3 / 9 / 16
STEP_R, STEP_S, STEP_T, STEP_SEED = tm.STEP_R, tm.STEP_S, tm.STEP_T, tm.STEP_SEED
STEP_N, STEP_B = tm.STEP_N, tm.STEP_B
SAMPLE_LIMITS = tm.SAMPLE_LIMITS              # (0, 1.0) and (8, 0.9)
TEMPS = (1.0, 0.7)
RADII = (1, 4)
PREV0 = ("absent", "adjacent", "far")
PLANES = ((False, False), (True, True))       # (half mask, random bias): neither, both


def _prev(K, W, shift):
  """prev1 / prev0 of the STEP_R = 8 rows.  prev1: the four corners, the middle of the left
  edge, an interior cell, the middle of the top edge, another interior cell.  prev0 of row i is
  of kind PREV0[(i + shift) % 3]: absent (-1), the cell beside prev1, or the corner that puts
  2 p1 - p0 farthest outside the grid (from a corner: every cell takes acc_far)."""
  H = K // W
  cell = lambda y, x: y * W + x
  p1 = [cell(0, 0), cell(0, W - 1), cell(H - 1, 0), cell(H - 1, W - 1), cell(H // 2, 0),
        cell(H // 2, W // 2), cell(0, W // 2), cell(H // 3, W // 3 + 1)]
  p0 = []
  for i, p in enumerate(p1):
    kind = PREV0[(i + shift) % 3]
    y, x = p // W, p % W
    if kind == "absent":
      p0.append(-1)
    elif kind == "adjacent":
      p0.append(cell(y, x + 1 if x + 1 < W else x - 1))
    else:
      def outside(c):
        cy, cx = 2 * y - c // W, 2 * x - c % W
        return max(-cy, cy - (H - 1), -cx, cx - (W - 1))
      p0.append(max((cell(0, 0), cell(0, W - 1), cell(H - 1, 0), cell(H - 1, W - 1)), key=outside))
  return np.array(p1, dtype=np.int32), np.array(p0, dtype=np.int32)


def _step_case(K, W, radius, shift, samples, planes_on):
  """logits [STEP_R, K], the motion argument of the ops, allowed / bias [samples, K] or None, and
  the restatement's per-row planes [STEP_R, K]."""
  rng = np.random.RandomState(5300 + 7 * K + radius)
  logits = (4.0 * rng.randn(STEP_R, K)).astype(np.float32)
  tables = _tables(samples, radius, True, seed=TABLE_SEED + K)
  p1, p0 = _prev(K, W, shift)
  mask_on, bias_on = planes_on
  allowed = tm._step_mask(K, "half", samples) if mask_on else None   # pylint: disable=protected-access
  bias = (2.0 * rng.randn(samples, K)).astype(np.float32) if bias_on else None
  per = STEP_R // samples
  planes = mo.row_planes(p1.reshape(samples, per), p0.reshape(samples, per), W, K, tables, bias)
  motion = dict(tables, W=W, prev1=p1, prev0=p0)
  return logits, motion, allowed, bias, planes.reshape(STEP_R, K)


def test_the_step_cases_are_what_they_are_named():
  for K, W in STEP_KW:
    seen = set()
    for shift in range(3):
      p1, p0 = _prev(K, W, shift)
      assert len(set(p1.tolist())) == STEP_R and ((p1 >= 0) & (p1 < K)).all()
      assert ((p0 >= -1) & (p0 < K)).all()
      tables = mo.tables_for(_tables(4, 4, True), 4)
      for i in range(STEP_R):
        kind = PREV0[(i + shift) % 3]
        seen.add((i, kind))
        _, a = mo.terms(p1[i], p0[i], W, K, tables, i // 2)
        if kind == "absent":
          assert (a == 0).all()
        elif kind == "adjacent":
          assert abs(p1[i] - p0[i]) == 1 and len(set(a.tolist())) > 9
        elif i < 4:                            # from a corner: every cell beyond the window
          assert (a == tables["acc_far"][i // 2]).all(), (K, i)
    assert len(seen) == 3 * STEP_R             # every placement of prev1 meets every kind of prev0


@pytest.mark.parametrize("K,W", STEP_KW)
def test_sample_step_op_against_the_restatement(built_lib, K, W):
  e32 = tm._restatement_error()            # pylint: disable=protected-access
  tol = 4 * e32                            # the bar of test_gpu_cell_mask.py for this op
  assert tol < 1e-4
  rows = np.arange(STEP_R)
  samples = STEP_R // STEP_S
  worst_lp = worst_q = 0.0
  for radius in RADII:
    for shift in range(3):
      for planes_on in PLANES:
        logits, motion, allowed, bias, planes = _step_case(K, W, radius, shift, samples, planes_on)
        arows = np.ones((STEP_R, K), dtype=bool) if allowed is None else \
            np.repeat(allowed != 0, STEP_S, axis=0)
        for limits in SAMPLE_LIMITS:
          for temp in TEMPS:
            what = (K, radius, shift, planes_on, limits, temp)
            ids, lp, qlp, keep = built_lib.op_sample_step(
                logits, STEP_S, STEP_T, temp, STEP_SEED, limits[0], limits[1], 1, allowed=allowed,
                bias=bias, motion=motion)
            want = mo.sample_step(logits, STEP_S, STEP_T, allowed, planes, temp, STEP_SEED,
                                  limits[0], limits[1], 1, dtype=np.float64)
            band = want["wide"] & ~want["tight"]
            assert (keep == want["tight"])[~band].all(), what
            assert not (keep & ~arows).any() and keep[rows, ids].all(), what
            if limits == (0, 1.0):
              assert (keep == arows).all(), what
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
    # zero tables are the biased / the masked / the plain op, bitwise
    for mask_on in (False, True):
      for bias_on in (False, True):
        for acc in (False, True):
          logits, motion, allowed, bias, _ = _step_case(K, W, radius, 1, samples, (mask_on, True))
          allowed, bias = (allowed if mask_on else None), (bias if bias_on else None)
          zero = dict(_zero_tables(samples, radius, acc), W=W, prev1=motion["prev1"],
                      prev0=motion["prev0"])
          for limits in SAMPLE_LIMITS:
            for temp in TEMPS:
              got = built_lib.op_sample_step(logits, STEP_S, STEP_T, temp, STEP_SEED, limits[0],
                                             limits[1], 1, allowed=allowed, bias=bias, motion=zero)
              base = built_lib.op_sample_step(logits, STEP_S, STEP_T, temp, STEP_SEED, limits[0],
                                              limits[1], 1, allowed=allowed, bias=bias)
              for name, a, b in zip(("ids", "lp", "qlp", "keep"), got, base):
                assert a.tobytes() == b.tobytes(), (K, radius, mask_on, bias_on, acc, limits, temp,
                                                    name)
  print("K=%d: float32 restatement vs float64 %.3g -> bar %.3g; device: logprob %.3g, "
        "proposal %.3g" % (K, e32, tol, worst_lp, worst_q))


def _beam_case(K, W, radius, shift, planes_on):
  logits, motion, allowed, bias, planes = _step_case(K, W, radius, shift, STEP_N, planes_on)
  prev = -np.random.RandomState(7000 + K).rand(STEP_N, STEP_B).astype(np.float32)
  return (logits.reshape(STEP_N, STEP_B, K), prev, motion, allowed, bias,
          planes.reshape(STEP_N, STEP_B, K))


@pytest.mark.parametrize("K,W", STEP_KW)
def test_beam_step_op_against_the_restatement(built_lib, K, W):
  tol = 4 * tm._restatement_error()        # pylint: disable=protected-access
  for radius in RADII:
    for shift in range(3):
      for planes_on in PLANES:
        logits, prev, motion, allowed, bias, planes = _beam_case(K, W, radius, shift, planes_on)
        for time in (1, 2):
          for diverse in (False, True):
            what = (K, radius, shift, planes_on, time, diverse)
            new_lp, ids, parents = built_lib.op_beam_step(logits, prev, time, diverse, 0.01, 0,
                                                          allowed=allowed, bias=bias,
                                                          motion=motion)
            want = mo.beam_step(logits, prev, allowed, planes, time, diverse, 0.01, 0,
                                dtype=np.float64)
            if allowed is not None:
              assert (allowed[np.arange(STEP_N)[:, None], ids] != 0).all(), what
            assert np.isfinite(new_lp).all(), what
            cmp = want["gap"] >= mo.GAP_BAR
            assert (~cmp).sum() * 4 <= STEP_N, what
            assert (ids[cmp] == want["ids"][cmp]).all() and \
                (parents[cmp] == want["parents"][cmp]).all(), what
            d = float(np.abs(new_lp - want["new_lp"])[cmp].max()) if cmp.any() else 0.0
            assert d <= tol, (what, d, tol)
    for mask_on in (False, True):
      for bias_on in (False, True):
        for acc in (False, True):
          logits, prev, motion, allowed, bias, _ = _beam_case(K, W, radius, 1, (mask_on, True))
          allowed, bias = (allowed if mask_on else None), (bias if bias_on else None)
          zero = dict(_zero_tables(STEP_N, radius, acc), W=W, prev1=motion["prev1"],
                      prev0=motion["prev0"])
          for time in (1, 2):
            for diverse in (False, True):
              got = built_lib.op_beam_step(logits, prev, time, diverse, 0.01, 0, allowed=allowed,
                                           bias=bias, motion=zero)
              base = built_lib.op_beam_step(logits, prev, time, diverse, 0.01, 0, allowed=allowed,
                                            bias=bias)
              for a, b in zip(got, base):
                assert a.tobytes() == b.tobytes(), (K, radius, mask_on, bias_on, acc, time, diverse)


@pytest.mark.parametrize("K,W", STEP_KW)
def test_sbs_step_op_against_the_restatement(built_lib, K, W):
  tol = 4 * tm._restatement_error()        # pylint: disable=protected-access
  rng = np.random.RandomState(8000 + K)
  phi, LP, G = (-rng.rand(STEP_N, STEP_B).astype(np.float32) for _ in range(3))
  for radius in RADII:
    for shift in range(3):
      for planes_on in PLANES:
        logits, _, motion, allowed, bias, planes = _beam_case(K, W, radius, shift, planes_on)
        for t in (0, 1):
          for temp in TEMPS:
            what = (K, radius, shift, planes_on, t, temp)
            got = built_lib.op_sbs_step(logits, phi, LP, G, t, temp, STEP_SEED, allowed=allowed,
                                        bias=bias, motion=motion)
            want = mo.sbs_step(logits, phi, LP, G, t, allowed, planes, temp, STEP_SEED,
                               dtype=np.float64)
            nphi, nlp, ng, ids, parents = got
            if allowed is not None:
              assert (allowed[np.arange(STEP_N)[:, None], ids] != 0).all(), what
            assert all(np.isfinite(a).all() for a in (nphi, nlp, ng)), what
            cmp = want["gap"] >= mo.GAP_BAR
            assert (~cmp).sum() * 4 <= STEP_N, what
            assert (ids[cmp] == want["ids"][cmp]).all() and \
                (parents[cmp] == want["parents"][cmp]).all(), what
            for a, key in ((nphi, "new_phi"), (nlp, "new_lp"), (ng, "new_g")):
              d = float(np.abs(a - want[key])[cmp].max()) if cmp.any() else 0.0
              assert d <= max(tol, 2e-5), (what, key, d, tol)   # the bar of the masked op
    for mask_on in (False, True):
      for bias_on in (False, True):
        logits, _, motion, allowed, bias, _ = _beam_case(K, W, radius, 1, (mask_on, True))
        allowed, bias = (allowed if mask_on else None), (bias if bias_on else None)
        zero = dict(_zero_tables(STEP_N, radius, True), W=W, prev1=motion["prev1"],
                    prev0=motion["prev0"])
        for t in (0, 1):
          for temp in TEMPS:
            got = built_lib.op_sbs_step(logits, phi, LP, G, t, temp, STEP_SEED, allowed=allowed,
                                        bias=bias, motion=zero)
            base = built_lib.op_sbs_step(logits, phi, LP, G, t, temp, STEP_SEED, allowed=allowed,
                                         bias=bias)
            for a, b in zip(got, base):
              assert a.tobytes() == b.tobytes(), (K, radius, mask_on, bias_on, t, temp)


# ---------------------------------------------------------------- 2. forward parity

@functools.lru_cache(maxsize=None)
def _parity_tables(name, radius, acc, seed=TABLE_SEED):
  return _tables(_cfg(name).batch_size, radius, acc, seed)


def parity_cuts(name, radius, acc, seed=TABLE_SEED):
  """What the restatement ALONE leaves uncompared in one case (no device): the independent
  sampler's and the without-replacement sampler's (row, step) pairs behind a near tie, and the
  beam's rows with a tied cut -> ((cut, of), (cut, of), (rows, of)).  This is what TABLE_SEED was
  picked by."""
  cfg, params, feed = _case(name)
  tables = _parity_tables(name, radius, acc, seed)
  N, S, T = cfg.batch_size, cfg.beam_size, T_PRED
  want = mo.sampled_forward(params, cfg, feed, tables, temperature=TEMP, seed=SEED)
  ind = int((T - cb.to.compared_steps(want["compared"])).sum())
  want = mo.sbs_forward(params, cfg, feed, tables, temperature=TEMP, seed=SEED)
  wor = int((T - sbs.compared_steps(want["gap"])).sum())
  trace = mo.beam_forward(params, cfg, feed, tables)[2]
  gap = np.minimum(np.stack(trace["beam_step_cut_gap"], axis=1),
                   np.stack(trace["beam_step_rank_gap"], axis=1))
  return (ind, N * S * T), (wor, N * T), (int((gap < TIE_TOL).any(axis=1).sum()), N)


def _check_sampled(name, mode, radius, acc):
  cfg, params, feed = _case(name)
  tables = _parity_tables(name, radius, acc)
  want = mo.sampled_forward(params, cfg, feed, tables, temperature=TEMP, seed=SEED)
  eng = _engine(cfg, params, "independent", mode)
  arrs = _fwd(eng, feed, tables)
  eng.close()
  N, S, T = cfg.batch_size, cfg.beam_size, T_PRED
  upto = cb.to.compared_steps(want["compared"])
  cut = int((T - upto).sum())
  print("%s/%s/R=%d/acc=%s: %d of %d (row, step) pairs behind a step that is not compared"
        % (name, mode, radius, acc, cut, N * S * T))
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
  assert (plain["ids"] != want["ids"]).any()               # the cost bites


def _beam_traced_logits(want, n, b, T):
  """The logits the engine returns for slot b of row n: the engine's own back-trace, as
  test_gpu_cell_bias.py compares them."""
  out = np.zeros((T,) + want["step_logits"][0].shape[2:], dtype=np.float32)
  slot = b
  for t in range(T - 1, -1, -1):
    out[t] = want["step_logits"][t][n, slot]
    slot = int(want["step_parents"][t][n, slot])
  return out


def _check_sbs(name, mode, radius, acc):
  cfg, params, feed = _case(name)
  tables = _parity_tables(name, radius, acc)
  want = mo.sbs_forward(params, cfg, feed, tables, temperature=TEMP, seed=SEED)
  eng = _engine(cfg, params, "without_replacement", mode)
  arrs = _fwd(eng, feed, tables)
  eng.close()
  N, B, T = cfg.batch_size, cfg.beam_size, T_PRED
  upto = sbs.compared_steps(want["gap"])
  cut = int((T - upto).sum())
  print("%s/%s/R=%d/acc=%s: %d of %d (row, step) pairs behind a gap below 1e-4"
        % (name, mode, radius, acc, cut, N * T))
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


def _check_beam(name, mode, radius, acc):
  cfg, params, feed = _case(name)
  tables = _parity_tables(name, radius, acc)
  oreg, (ologits, oids, olp), trace = mo.beam_forward(params, cfg, feed, tables)
  s = list(cfg.use_grids).index(True)
  eng = _engine(cfg, params, "beam", mode)
  arrs = _fwd(eng, feed, tables)
  eng.close()
  cut_gap = np.minimum(np.stack(trace["beam_step_cut_gap"], axis=1),
                       np.stack(trace["beam_step_rank_gap"], axis=1))
  compare_beams(arrs, oreg[s].numpy() if hasattr(oreg[s], "numpy") else oreg[s], ologits, oids,
                olp, np.stack(trace["beam_step_topvals"], axis=-1), trace["beam_trace"],
                cut_gap=cut_gap)
  assert compare_beams.unmatched * 4 <= oids.shape[0] * oids.shape[1]
  plain = cb.beam_forward(params, cfg, feed, None,
                          np.zeros((cfg.batch_size, 1, _K(cfg)), dtype=np.float32))[1]
  assert (plain[1] != oids).any()                          # the cost bites


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,mode,radius,acc", PARITY)
def test_parity_with_the_oracle(built_lib, name, mode, radius, acc, kind):
  {"beam": _check_beam, "independent": _check_sampled, "without_replacement": _check_sbs}[kind](
      name, mode, radius, acc)


# ---------------------------------------------------------------- 3. the first step is the bias

def _labels_plane(cfg, feed, tables, obs_lengths=None):
  """b[n, k] = vterm + aterm of a first step, from the labels: [N, 1, K]."""
  s, _, W = _grid(cfg)
  N, K = cfg.batch_size, _K(cfg)
  path = mo.Path(feed["grid_obs_labels"][s], 1, obs_lengths)
  return mo.row_planes(path.p1, path.p0, W, K, tables)


@pytest.mark.parametrize("kind", KINDS)
def test_a_one_step_forward_is_the_bias_of_the_plane_built_from_the_labels(built_lib, kind):
  cfg, params, feed = _case("k144")
  feed = dict(feed, pred_length=1)
  keys = ["ids", "logits", "logprobs", "grid_reg", "best_beam"] + \
      ([] if kind == "beam" else ["q"]) + (["gumbels"] if kind == "without_replacement" else [])
  eng = _engine(cfg, params, kind)
  plain = _fwd(eng, feed)
  for acc in (False, True):
    tables = _tables(cfg.batch_size, 2, acc)
    moved = _fwd(eng, feed, tables)
    biased = _fwd(eng, feed, None, _labels_plane(cfg, feed, tables))
    for k in keys:
      assert moved[k].tobytes() == biased[k].tobytes(), (acc, k)
    assert not (moved["ids"] == plain["ids"]).all()
  eng.close()


# ---------------------------------------------------------------- 4. the limit

def _steps_in_cells(ids, labels, W):
  """Chebyshev length, in cells, of every step of every returned path: [N, B, T]."""
  ids = np.asarray(ids).astype(np.int64)
  N, B, T = ids.shape
  prev = np.concatenate([np.repeat(np.asarray(labels)[:, None, -1:], B, axis=1), ids[:, :, :-1]], 2)
  return np.maximum(np.abs(ids // W - prev // W), np.abs(ids % W - prev % W))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["k144", "k576"])
def test_the_limit_holds_and_is_not_vacuous(built_lib, name, kind):
  params, feed = _case(name)[1:]
  cfg = _cfg(name, S=4)
  s, H, W = _grid(cfg)
  labels = [None if a is None else np.array(a, copy=True) for a in feed["grid_obs_labels"]]
  labels[s][0, -1] = (H - 1) * W                           # row 0 ends in a corner
  feed = dict(feed, grid_obs_labels=labels)
  limit = LIMIT
  assert limit["vel"][0, 0] == np.float32(-1e30) and limit["vel"][1, 1] == 0 and limit["acc"] is None
  eng = _engine(cfg, params, kind)
  held = _fwd(eng, feed, limit)
  eng.set_motion_cost(None)
  free = _fwd(eng, feed)
  eng.close()
  steps = _steps_in_cells(held["ids"], labels[s], W)
  assert steps.max() <= 1, (steps, held["ids"])
  assert np.abs(held["logprobs"]).max() < 1e29             # no slot had to leave the windows
  assert _steps_in_cells(free["ids"], labels[s], W).max() > 1


# ---------------------------------------------------------------- 5. zero tables, graph replay

@functools.lru_cache(maxsize=None)
def _runs(kind):
  """One handle: eager forwards under tables A, A2 (other values), A4 (another radius, no acc),
  zero and none, then the same in graph mode; and a handle that never had a motion cost."""
  cfg, params, feed = _case("k144")
  N = cfg.batch_size
  A, A2 = _tables(N, 2, True), _tables(N, 2, True, TABLE_SEED + 1)
  A4 = _tables(N, 4, False, TABLE_SEED + 2)
  zero = _zero_tables(N, 2, True)
  eng = _engine(cfg, params, kind)
  r = {}
  for key, t in (("A", A), ("A2", A2), ("A4", A4), ("zero", zero)):
    r[key] = _fwd(eng, feed, t)
  r["none"] = _fwd(eng, feed)
  eng.set_graph_mode(True)
  caps = [eng.graph_captures()]
  for key, t in (("gA", A), ("gA2", A2), ("gA3", A), ("gzero", zero), ("gnone", None), ("gA4", A4),
                 ("gA5", A)):
    r[key] = _fwd(eng, feed, t)
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
def test_zero_tables_are_bitwise_a_handle_that_never_had_one(built_lib, kind):
  r = _runs(kind)
  keys = sorted(r["fresh"])
  assert _same(r["zero"], r["fresh"], keys) and _same(r["none"], r["fresh"], keys)
  assert _same(r["gzero"], r["gfresh"], keys) and _same(r["gnone"], r["gfresh"], keys)
  assert _same(r["fresh"], r["gfresh"], keys) and _same(r["gfresh2"], r["gfresh"], keys)
  assert r["fresh_captures"] == [0, 1]     # no cost set: one graph, as ever
  if kind != "beam":                       # under a cost the forwards report the proposal as well
    assert "proposal_logprobs" in r["zero"] and "proposal_logprobs" not in r["none"]
    assert r["zero"]["proposal_logprobs"].tobytes() == r["zero"]["q"].tobytes()
  assert not (r["A"]["ids"] == r["none"]["ids"]).all()       # ... and real tables bite
  assert r["A"]["logits"][:, :, 0].tobytes() == r["none"]["logits"][:, :, 0].tobytes()


@pytest.mark.parametrize("kind", KINDS)
def test_a_replayed_graph_follows_the_tables_without_recapture(built_lib, kind):
  r = _runs(kind)
  for g, e in (("gA", "A"), ("gA2", "A2"), ("gA3", "A"), ("gA4", "A4"), ("gA5", "A")):
    assert _same(r[g], r[e]), (g, e)
  assert not (r["A"]["ids"] == r["A2"]["ids"]).all()
  # captures: gA one graph; other VALUES, A again and zero replay it; none is the plain graph;
  # another radius without acc is a third; A again replays the first
  c = r["captures"]
  assert [b - a for a, b in zip(c[:-1], c[1:])] == [1, 0, 0, 0, 1, 1, 0], c


@pytest.mark.parametrize("kind", KINDS)
def test_a_cost_set_on_the_engine_stays_through_feeds_without_the_key(built_lib, kind):
  cfg, params, feed = _case("k144")
  N = cfg.batch_size
  tables, other = _tables(N, 2, True), _tables(N, 2, True, TABLE_SEED + 1)
  eng = _engine(cfg, params, kind)
  by_feed = _fwd(eng, feed, tables)
  plain = _fwd(eng, feed)                  # a feed without the key clears what a FEED set
  eng.set_motion_cost(**tables)
  first, second = _fwd(eng, feed), _fwd(eng, feed)         # ... and not what was set directly
  third = _fwd(eng, feed, other)           # a feed's own tables replace them, and then follow
  fourth = _fwd(eng, feed)                 # the feeds' rule
  one_row = {k: (v[0] if isinstance(v, np.ndarray) else v) for k, v in tables.items()}
  eng.set_motion_cost(**one_row)           # one row's tables are taken for every row
  broadcast = _fwd(eng, feed)
  eng.set_motion_cost(None)
  fifth = _fwd(eng, feed)
  eng.close()
  assert _same(first, by_feed) and _same(second, by_feed)
  assert not _same(third, by_feed) and not _same(plain, by_feed)
  assert _same(fourth, plain) and _same(fifth, plain)
  assert broadcast["ids"][0].tobytes() == by_feed["ids"][0].tobytes()


# ---------------------------------------------------------------- 6. the beam score

@pytest.mark.parametrize("with_bias", [False, True])
def test_the_beam_score_is_the_models_plus_what_the_path_paid(built_lib, with_bias):
  params, feed = _case("k144")[1:]
  cfg = _cfg("k144", diverse=False)
  s, _, W = _grid(cfg)
  N, B, T, K = cfg.batch_size, cfg.beam_size, T_PRED, _K(cfg)
  tables = _tables(N, 2, True)
  bias = (2.0 * np.random.RandomState(TABLE_SEED).randn(N, T, K)).astype(np.float32) \
      if with_bias else None
  eng = _engine(cfg, params, "beam")
  arrs = _fwd(eng, feed, tables, bias)
  ids = arrs["ids"]
  # the model's step log-probabilities along each returned path: the teacher-forced scorer (the
  # returned logits follow the reference's back-trace, which gathers by the NEW slot index)
  model = eng.score_futures(feed, ids)["step_logprobs"].astype(np.float64)
  eng.close()
  paid = mf.path_motion_cost(ids, feed["grid_obs_labels"][s], W, tables).astype(np.float64)
  if bias is not None:
    paid += np.take_along_axis(np.broadcast_to(bias[:, None], (N, B, T, K)).astype(np.float64),
                               ids[..., None].astype(np.int64), axis=-1)[..., 0]
  # the carried score starts after the first fix_num_timestep steps, as without a cost
  live = np.arange(T) >= cfg.fix_num_timestep
  got = arrs["logprobs"].astype(np.float64) - (paid * live).sum(-1)
  assert np.abs(got - (model * live).sum(-1)).max() < TOL * T
  assert np.abs(paid).max() > 0.5


# ---------------------------------------------------------------- 7. the scorer

@pytest.mark.parametrize("kind", ["independent", "without_replacement"])
def test_the_scorer_returns_the_logprobs_under_a_cost(built_lib, kind):
  cfg, params, feed = _case("k144")
  tables = _tables(cfg.batch_size, 2, True)
  eng = _engine(cfg, params, kind)
  arrs = _fwd(eng, feed, tables)
  # the cost is still set while scoring, through the feed or directly: it is neither read ...
  scored = eng.score_futures(dict(feed, motion_cost=tables), arrs["ids"])
  again = _fwd(eng, feed, tables)
  eng.set_motion_cost(**tables)
  direct = eng.score_futures(feed, arrs["ids"])
  kept = _fwd(eng, feed)                   # ... nor cleared by a feed without the key
  eng.close()
  assert scored["logprobs"].tobytes() == arrs["logprobs"].tobytes()
  assert direct["logprobs"].tobytes() == arrs["logprobs"].tobytes()
  assert _same(again, arrs) and _same(kept, arrs)          # ... and not changed
  assert np.isfinite(arrs["q"]).all() and (arrs["q"] <= 0).all()
  assert not (arrs["q"] == arrs["logprobs"]).any()         # the proposal is not the model


# ---------------------------------------------------------------- 8. batch, lengths, short tracks

@pytest.mark.parametrize("kind", KINDS)
def test_rows_are_their_own_uniform_forwards_under_their_own_tables(built_lib, kind):
  """Row 1 is observed for ONE frame (no turn term at its first step) beside row 2 with two."""
  lens, obs = (3, 3, 2), (8, 1, 2)
  cfg3, params, feed3 = _case("k144", 3)
  K = _K(cfg3)
  tables = _tables(3, 2, True)
  bias = (2.0 * np.random.RandomState(TABLE_SEED + 5).randn(3, T_PRED, K)).astype(np.float32)
  mask = _half_mask(3, T_PRED, K)
  eng = _engine(cfg3, params, kind)
  full = _fwd(eng, feed3, tables, bias, mask)
  rag = _fwd(eng, dict(feed3, pred_lengths=list(lens), obs_lengths=list(obs)), tables, bias, mask)
  eng.close()
  keys = ["ids", "logits", "logprobs", "grid_reg", "best_beam"] + \
      ([] if kind == "beam" else ["q"]) + (["gumbels"] if kind == "without_replacement" else [])
  eng1 = _engine(_cfg("k144", batch_size=1), params, kind)
  for n in range(3):
    feed1 = dict(feed3, obs_scene=feed3["obs_scene"][n:n + 1],
                 grid_obs_labels=[a[n:n + 1] for a in feed3["grid_obs_labels"]],
                 grid_obs_regress=[a[n:n + 1] for a in feed3["grid_obs_regress"]])
    t1 = {k: (v[n:n + 1] if isinstance(v, np.ndarray) else v) for k, v in tables.items()}
    if kind != "beam":
      eng1.set_sampling(TEMP, so.row_seed(SEED, n), without_replacement=kind == "without_replacement")
    a1 = _fwd(eng1, feed1, t1, bias[n:n + 1], mask[n:n + 1])
    for k in keys:
      assert a1[k][0].tobytes() == full[k][n].tobytes(), (n, k)
    L = lens[n]
    u1 = _fwd(eng1, dict(feed1, pred_length=L, obs_lengths=[obs[n]]), t1, bias[n:n + 1],
              mask[n:n + 1])
    for k, ax in {"ids": 1, "logits": 1, "best_beam": 0, "grid_reg": 0}.items():
      a = np.moveaxis(rag[k][n], ax, 0)
      assert (a[L:] == (-1 if k == "ids" else 0)).all(), (n, k)
      want = np.moveaxis(u1[k][0], ax, 0)
      assert np.ascontiguousarray(a[:L]).tobytes() == np.ascontiguousarray(want).tobytes(), (n, k)
    for k in [k for k in keys if k in ("logprobs", "q", "gumbels")]:
      assert rag[k][n].tobytes() == u1[k][0].tobytes(), (n, k)
    if obs[n] == 1:
      # no turn term at the first step: the same row under tables whose acc differs, cut to one step
      other = dict(t1, acc=t1["acc"] + np.float32(1.0))
      one = dict(feed1, pred_length=1, obs_lengths=[1])
      assert _fwd(eng1, one, other, bias[n:n + 1], mask[n:n + 1])["ids"].tobytes() == \
          _fwd(eng1, one, t1, bias[n:n + 1], mask[n:n + 1])["ids"].tobytes()
  eng1.close()


# ---------------------------------------------------------------- 9. errors

def test_errors_name_their_cause(built_lib):
  lib = built_lib
  cfg, params, feed = _case("k144")
  N = cfg.batch_size
  good = _tables(N, 2, True)
  greedy = synth.default_config(batch_size=2, use_grids=(0, 1), enc_hidden_size=128,
                                dec_hidden_size=128)
  geng = lib.Engine(greedy, device=0)
  with pytest.raises(lib.MvError) as err:
    geng.set_motion_cost(**_tables(2, 2, True))
  assert "mv_set_motion_cost" in str(err.value) and "beam_size 1" in str(err.value)
  geng.close()
  eng = _engine(cfg, params, "beam")
  fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
  big = np.zeros((N, 11, 11), dtype=np.float32)
  far = np.zeros(N, dtype=np.float32)
  for radius in (0, 5, -1):
    assert eng.lib.mv_set_motion_cost(eng.handle, radius, fp(big), fp(far), None, None) != 0
    assert "radius = %d" % radius in eng.lib.mv_last_error(eng.handle).decode()
  with pytest.raises(lib.MvError) as err:
    eng.set_motion_cost(5, big, far)
  assert "radius" in str(err.value)
  # acc / acc_far: both or neither
  assert eng.lib.mv_set_motion_cost(eng.handle, 2, fp(good["vel"]), fp(good["vel_far"]),
                                    fp(good["acc"]), None) != 0
  msg = eng.lib.mv_last_error(eng.handle).decode()
  assert "mv_set_motion_cost" in msg and "both or neither" in msg and "acc_far" in msg
  assert eng.lib.mv_set_motion_cost(eng.handle, 2, fp(good["vel"]), fp(good["vel_far"]), None,
                                    fp(good["acc_far"])) != 0
  assert "both or neither" in eng.lib.mv_last_error(eng.handle).decode()
  with pytest.raises(lib.MvError):
    eng.set_motion_cost(2, good["vel"], good["vel_far"], good["acc"])
  with pytest.raises(lib.MvError) as err:
    eng.set_motion_cost(2, np.zeros((N, 3, 3), dtype=np.float32), good["vel_far"])
  assert "motion_cost" in str(err.value) and "vel" in str(err.value)
  # a value that is not finite: the table, n and the entry
  for name, entry in (("vel", (1, 2, 3)), ("vel_far", (1,)), ("acc", (0, 4, 4)), ("acc_far", (0,))):
    for bad in (np.nan, np.inf, -np.inf):
      t = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in good.items()}
      t[name][entry] = bad
      with pytest.raises(lib.MvError) as err:
        eng.set_motion_cost(**t)
      msg = str(err.value)
      flat = 0 if len(entry) == 1 else entry[1] * 5 + entry[2]
      assert "mv_set_motion_cost" in msg and name + "[n = %d, entry %d]" % (entry[0], flat) in msg
      assert "finite" in msg, (name, bad)
  before = dict(eng.forward_beam(feed)[0])                 # a refused cost is not set
  # training, the pipelined greedy forward and the occupancy map while a cost is set
  eng.set_motion_cost(**good)
  for call, name in ((eng.train_init, "mv_train_init"), (eng.train_step, "mv_train_step"),
                     (eng.train_forward_backward, "mv_train_forward_backward"),
                     (eng.train_apply, "mv_train_apply")):
    with pytest.raises(lib.MvError) as err:
      call()
    assert name + ":" in str(err.value) and "motion cost" in str(err.value), name
  inp = eng._inputs(dict(feed, motion_cost=good))          # pylint: disable=protected-access
  assert eng.lib.mv_submit_greedy(eng.handle, ctypes.byref(inp)) != 0
  msg = eng.lib.mv_last_error(eng.handle).decode()
  assert "mv_submit_greedy" in msg and "motion cost" in msg
  eng.forward_beam(dict(feed, motion_cost=good))
  with pytest.raises(lib.MvError) as err:
    eng.beam_occupancy()
  assert "mv_beam_occupancy" in str(err.value) and "motion cost" in str(err.value)
  eng.set_motion_cost(None)
  assert eng.beam_occupancy().shape[0] == N                # cleared: the map is back
  assert _same(dict(eng.forward_beam(feed)[0]), before)
  eng.close()
  # a grid of more than 1024 cells, at the forward (refused before anything is launched)
  wide = synth.default_config(batch_size=1, use_grids=(1, 0), beam_size=2, enc_hidden_size=128,
                              dec_hidden_size=128, scene_h=72, scene_w=64,
                              scene_grids=[(36, 32), (18, 16)])
  wide.max_pred_len = T_PRED
  weng = lib.Engine(wide, device=0)
  wfeed = synth.make_feed(wide, seed=synth.SEED_BASE + 7, pred_len=T_PRED)
  with pytest.raises(lib.MvError) as err:
    weng.forward_beam(dict(wfeed, motion_cost=_tables(1, 2, False)))
  assert "1152 cells" in str(err.value) and "mv_set_motion_cost" in str(err.value)
  weng.close()
  # the ops: K beyond a wave, a value that is not finite, a cell outside the grid, W
  mot = dict(_tables(1, 1, True), W=10, prev1=np.zeros(2, np.int32), prev0=np.zeros(2, np.int32))
  for op, args in ((lib.op_beam_step, (np.zeros((1, 2, 1100), np.float32), np.zeros((1, 2), np.float32),
                                       2, False, 1.0, 0)),
                   (lib.op_sbs_step, (np.zeros((1, 2, 1100), np.float32),) +
                    (np.zeros((1, 2), np.float32),) * 3 + (1,)),
                   (lib.op_sample_step, (np.zeros((2, 1100), np.float32), 2, 0))):
    with pytest.raises(lib.MvError) as err:
      op(*args, motion=mot)
    assert "K = 1100" in str(err.value) and "mv_" + op.__name__ + "_motion" in str(err.value), op
    small = tuple(a[..., :70] if isinstance(a, np.ndarray) and a.shape[-1] == 1100 else a
                  for a in args)
    for change, word in ((dict(vel=np.full((1, 3, 3), np.nan, np.float32)), "finite"),
                         (dict(prev1=np.array([0, 70], np.int32)), "prev1[1] = 70"),
                         (dict(prev0=np.array([-2, 0], np.int32)), "prev0[0] = -2"),
                         (dict(W=9), "W = 9"), (dict(radius=5), "radius 5"),
                         (dict(acc_far=None), "both or neither")):
      with pytest.raises(lib.MvError) as err:
        op(*small, motion=dict(mot, **change))
      assert word in str(err.value), (op, word, str(err.value))
