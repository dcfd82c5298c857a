# coding=utf-8
"""Test-side restatement of the CONSTRAINED decode (mv_set_cell_mask: per-row allowed cells for
the beam search and both samplers; the reference has none, the definition is in
include/multiverse_hip.h), on top of the existing restatements -- beam_compare, sampling_oracle,
sbs_oracle, truncation_oracle and the oracle's beam decoder -- which it imports and does not
modify: the forwards below run THEIR loops with the one function that chooses cells swapped for
its masked form while the call lasts.

A = A(n, t) is the allowed set, l the step's logits:
  lp = log_softmax(l) over ALL cells, unchanged (logprobs and the logits outputs are the model's)
  beam:     lp + prev_lp is -inf outside A BEFORE the diversity ranks; all else as it is
  samplers: a cell outside A is absent from the proposal: w = l / tau, mxq = max of w over A,
            e, sum_e, c(k), m(k) and the floor over A, keep(k) = k in A and the limits' predicate,
            q~[k] = (w[k] - mxq) - log(sum of e over the kept cells), -inf elsewhere
  occupancy: every future's step map is the softmax over A, exactly 0 outside."""
import contextlib

import numpy as np

from oracle import multiverse_oracle as oracle
import beam_compare  # noqa: F401  pylint: disable=unused-import  (the comparator of beam_forward's users)
import sampling_oracle as so
import sbs_oracle as sbs
import truncation_oracle as to

GAP_BAR = sbs.GAP_BAR


def plane(mask, t):
  """mask [N, Tm, K] -> the planes [N, K] of decode step t (Tm == 1: the one plane)."""
  mask = np.asarray(mask) != 0
  return mask[:, 0 if mask.shape[1] == 1 else t]


def keep_sets(logits, allowed, temperature, top_k, top_p, floor=1):
  """truncation_oracle.keep_sets over the allowed cells of every row: logits, allowed [..., K] ->
  (keep, tight, wide) bool [..., K], all False outside `allowed`."""
  logits = np.asarray(logits, dtype=np.float32)
  allowed = np.broadcast_to(np.asarray(allowed) != 0, logits.shape)
  flat, fa = logits.reshape(-1, logits.shape[-1]), allowed.reshape(-1, logits.shape[-1])
  floors = np.broadcast_to(np.asarray(floor), logits.shape[:-1]).reshape(-1)
  out = np.zeros((3,) + flat.shape, dtype=bool)
  for r in range(flat.shape[0]):
    idx = np.nonzero(fa[r])[0]
    sets = to._keep_row(flat[r, idx], temperature, top_k, top_p, int(floors[r]))   # pylint: disable=protected-access
    for i in range(3):
      out[i, r, idx] = sets[i]
  return tuple(o.reshape(logits.shape) for o in out)


def proposal(logits, temperature, keep, allowed, dtype=np.float32):
  """q~ [..., K] in `dtype`: truncation_oracle.proposal with the maximum taken over `allowed` and
  the sum over `keep` (a subset of it); -inf elsewhere.  All allowed and kept: sbs_oracle's
  log_softmax of w, the same bits."""
  l = np.asarray(logits).astype(dtype)
  w = l if float(temperature) == 1.0 else (l / dtype(temperature)).astype(dtype)
  mx = np.where(allowed, w, -np.inf).max(axis=-1, keepdims=True)
  with np.errstate(over="ignore", invalid="ignore"):
    e = np.where(keep, np.exp(np.where(keep, w - mx, -np.inf)), dtype(0)).astype(dtype)
    lse = np.log(e.sum(axis=-1, keepdims=True, dtype=dtype))
    return np.where(keep, (w - mx) - lse, -np.inf).astype(dtype)


def draw(logits, lp, g, allowed, temperature, top_k=0, top_p=1.0, floor=1, dtype=np.float64):
  """truncation_oracle.draw under `allowed` [..., K] (broadcast over the futures of a sample)."""
  allowed = np.broadcast_to(np.asarray(allowed) != 0, np.asarray(logits).shape)
  keep, tight, wide = keep_sets(logits, allowed, temperature, top_k, top_p, floor)
  ids, _ = to.masked_ids(lp, temperature, g, keep)
  ids_t, _ = to.masked_ids(lp, temperature, g, tight)
  ids_w, margin = to.masked_ids(lp, temperature, g, wide)
  q = proposal(logits, temperature, keep, allowed, dtype)
  pick = lambda a: np.take_along_axis(a, ids[..., None].astype(np.int64), axis=-1)[..., 0]
  return {"keep": keep, "tight": tight, "wide": wide, "ids": ids,
          "compared": (ids_t == ids_w) & (ids == ids_w) & (margin >= GAP_BAR),
          "sure": (tight == wide).all(axis=-1),
          "lp_id": pick(np.asarray(lp, dtype=np.float32)), "q_id": pick(q), "q": q}


def sample_step(logits, S, t, allowed, temperature=1.0, seed=0, top_k=0, top_p=1.0, floor=1,
                dtype=np.float64):
  """mv_op_sample_step_masked: logits [R, K], allowed [R // S, K] -> draw() with lp_id in `dtype`."""
  logits = np.asarray(logits, dtype=np.float32)
  R, K = logits.shape
  g = so.step_noise(R // S, S, K, seed, t).reshape(R, K)
  rows = np.repeat(np.asarray(allowed).reshape(R // S, K) != 0, S, axis=0)
  out = draw(logits, sbs.log_softmax(logits), g, rows, temperature, top_k, top_p, floor, dtype)
  lpd = sbs.log_softmax(logits.astype(dtype))
  out["lp_id"] = np.take_along_axis(lpd, out["ids"][:, None].astype(np.int64), axis=-1)[:, 0]
  return out


def beam_step(logits, prev_lp, allowed, time, diverse, gamma, fix_num_timestep,
              dtype=np.float32):
  """mv_op_beam_step_masked on logits [N, B, K], prev_lp [N, B], allowed [N, K] -> dict of new_lp,
  ids, parents [N, B], cand (the candidates after the penalty) and gap [N]: the smallest adjacent
  gap among the B + 1 best candidates (and, diverse, among a parent's three best before the
  penalty: an ulp there trades a whole log(gamma))."""
  l = np.asarray(logits).astype(dtype)
  N, B, K = l.shape
  a = (np.asarray(allowed).reshape(N, 1, K) != 0)
  lp = (np.asarray(prev_lp).astype(dtype)[..., None] + sbs.log_softmax(l)).astype(dtype)
  lp = np.where(a, lp, -np.inf).astype(dtype)
  rank_gap = np.full(N, np.inf)
  if diverse:
    with np.errstate(invalid="ignore"):
      top3 = -np.sort(-lp.astype(np.float64), axis=-1)[..., :3]
      d = top3[..., :-1] - top3[..., 1:]
      rows = lp[:, :1] if time <= 1 else lp
      rank_gap = np.where(np.isfinite(d), d, np.inf)[:, :rows.shape[1]].reshape(N, -1).min(-1)
    order = np.argsort(-lp, axis=-1, kind="stable")
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.broadcast_to(np.arange(K), lp.shape).copy(), axis=-1)
    lp = (lp + dtype(np.log(np.float32(gamma))) * rank.astype(dtype)).astype(dtype)
  flat = lp.reshape(N, B * K) if time > 1 else lp[:, 0]
  order = np.argsort(-flat, axis=-1, kind="stable")
  top = order[:, :B]
  vals = np.take_along_axis(flat, top, axis=-1)
  best = np.take_along_axis(flat, order[:, :B + 1], axis=-1).astype(np.float64)
  with np.errstate(invalid="ignore"):
    gaps = best[:, :-1] - best[:, 1:]
  gaps = np.where(np.isnan(gaps), np.inf, gaps).min(axis=-1)
  return {"new_lp": vals if time > fix_num_timestep else np.zeros_like(vals),
          "ids": (top % K).astype("int32"), "parents": (top // K).astype("int32"), "cand": lp,
          "gap": np.minimum(gaps, rank_gap)}


def sbs_step(logits, prev_phi, prev_lp, prev_g, t, allowed, temperature=1.0, seed=0,
             dtype=np.float32, row_base=0, top_k=0, top_p=1.0):
  """sbs_oracle.step under `allowed` [N, K] (and the limits of the truncated sampling, floor B at
  t == 0): q is the masked proposal, a cell outside the kept set is the candidate -inf."""
  N, B, K = logits.shape
  l = np.asarray(logits).astype(dtype)
  phi, LP, G = (np.asarray(x).astype(dtype) for x in (prev_phi, prev_lp, prev_g))
  a = np.broadcast_to(np.asarray(allowed).reshape(N, 1, K) != 0, l.shape)
  lp = sbs.log_softmax(l)
  keep = keep_sets(logits, a, temperature, top_k, top_p, B if t == 0 else 1)[0]
  q = proposal(l, temperature, keep, a, dtype)
  u = sbs.step_uniform(N, B, K, seed, t, row_base)
  gum = (-np.log(-np.log(u.astype(dtype)))).astype(dtype)
  safe_q = np.where(keep, q, dtype(0))
  g = ((phi[..., None] + safe_q) + gum).astype(dtype)
  Z = np.where(keep, g, -np.inf).max(axis=-1, keepdims=True)
  Gt = np.where(keep, sbs.truncated(G[..., None], g, np.maximum(Z, g)), -np.inf).astype(dtype)
  cand = Gt[:, 0, :] if t == 0 else Gt.reshape(N, B * K)
  order = np.argsort(-cand, axis=-1, kind="stable")
  top = order[:, :B]
  par, k = top // K, top % K
  rows = np.arange(N)[:, None]
  best = np.take_along_axis(cand, order[:, :B + 1], axis=-1).astype(np.float64)
  with np.errstate(invalid="ignore"):
    gaps = best[:, :-1] - best[:, 1:]
  return {"new_phi": (phi[rows, par] + q[rows, par, k]).astype(dtype),
          "new_lp": (LP[rows, par] + lp[rows, par, k]).astype(dtype),
          "new_g": np.take_along_axis(cand, top, axis=-1),
          "ids": k.astype("int32"), "parents": par.astype("int32"), "lp": lp, "q": q,
          "gap": np.where(np.isnan(gaps), np.inf, gaps).min(axis=-1)}


def occupancy(logits, logprobs, mask, uniform=False, dtype=np.float64):
  """mv_beam_occupancy under a mask in `dtype`: logits [N, B, T, K], logprobs [N, B], mask
  [N, Tm, K] -> [N, T, K]; uniform: the independent sampler's 1 / B weights."""
  x = np.asarray(logits).astype(dtype)
  N, B, T, K = x.shape
  lp = np.zeros((N, B), dtype=dtype) if uniform else np.asarray(logprobs).astype(dtype)
  w = np.exp(lp - lp.max(-1, keepdims=True))
  w = (w / w.sum(-1, keepdims=True, dtype=dtype)).astype(dtype)
  out = np.zeros((N, T, K), dtype=dtype)
  for t in range(T):
    a = plane(mask, t)[:, None, :]
    xt = np.where(a, x[:, :, t], -np.inf).astype(dtype)
    e = np.exp(xt - xt.max(-1, keepdims=True)).astype(dtype)
    p = (e / e.sum(-1, keepdims=True, dtype=dtype)).astype(dtype)
    for b in range(B):                                     # the beams in order, each product rounded
      out[:, t] = (out[:, t] + (p[:, b] * w[:, b, None]).astype(dtype)).astype(dtype)
  return out


# ---- the forwards: the existing loops with the choosing function swapped while the call lasts

@contextlib.contextmanager
def _swapped(module, name, fn):
  old = getattr(module, name)
  setattr(module, name, fn)
  try:
    yield
  finally:
    setattr(module, name, old)


def sampled_forward(params, cfg, feed, mask, temperature=1.0, seed=0, top_k=0, top_p=1.0):
  """truncation_oracle.forward (independent sampler) under mask [N, Tm, K]."""
  step = [0]

  def masked_draw(logits, lp, g, temp, k, p):
    a = plane(mask, step[0])[:, None, :]
    step[0] += 1
    return draw(logits, lp, g, a, temp, k, p)

  with _swapped(to, "draw", masked_draw):
    return to.forward(params, cfg, feed, temperature=temperature, seed=seed, top_k=top_k,
                      top_p=top_p)


def sbs_forward(params, cfg, feed, mask, temperature=1.0, seed=0):
  """sbs_oracle.forward (sampling without replacement) under mask [N, Tm, K]."""
  def masked_step(logits, phi, LP, G, t, temp, sd, dtype=np.float32):
    return sbs_step(logits, phi, LP, G, t, plane(mask, t), temp, sd, dtype=dtype)

  with _swapped(sbs, "step", masked_step):
    return sbs.forward(params, cfg, feed, temperature=temperature, seed=seed)


def beam_forward(params, cfg, feed, mask):
  """The oracle's beam decoder under mask [N, Tm, K]: its log-softmax of step t is -inf outside
  A(n, t), which is what lp + prev_lp then is, before the ranks ->
  (oreg, (ologits, oids, olp), trace) as oracle.forward with a trace."""
  import torch
  plain = oracle.log_softmax_tf
  N, B = cfg.batch_size, cfg.beam_size
  step = [0]

  def masked_log_softmax(x):
    lp = plain(x)
    if x.dim() != 3 or tuple(x.shape[:2]) != (N, B):
      return lp
    a = torch.from_numpy(plane(mask, step[0])[:, None, :].copy())
    step[0] += 1
    return torch.where(a, lp, torch.full_like(lp, float("-inf")))

  trace = {}
  with _swapped(oracle, "log_softmax_tf", masked_log_softmax):
    _, oreg, obeam = oracle.forward(params, cfg, feed, trace=trace)
  assert step[0] == int(feed["pred_length"])
  return oreg, obeam, trace
