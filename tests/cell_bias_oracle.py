# coding=utf-8
"""Test-side restatement of the CELL COSTS (mv_set_cell_bias: a per-row, per-step, per-cell
additive log-potential for the beam search and both samplers; the reference has none, the
definition is in include/multiverse_hip.h), on top of cell_mask_oracle, truncation_oracle,
sbs_oracle and sampling_oracle, which it imports and does not modify.  The signatures are those of
cell_mask_oracle plus `bias`; `allowed` None means every cell.

b = b(n, t) is the row's bias plane, A the allowed set, l the step's logits:
  lp = log_softmax(l) over ALL cells, unchanged (logprobs and the logits outputs are the model's)
  beam:     the candidate is (prev_lp + lp) + b, -inf outside A, BEFORE the diversity ranks
  samplers: w = l / tau + b, -inf outside A; mxq, e, sum_e, c(k), m(k), the floor and q~ as under a
            mask, over this w; the ORDER of the limits is the order of the float32 w (not of l);
            the independent sampler's score is (lp / tau + b) + g
  occupancy: every future's step map is the softmax of l + b over A, exactly 0 outside."""
import numpy as np

from oracle import multiverse_oracle as oracle
import cell_mask_oracle as cm
import sampling_oracle as so
import sbs_oracle as sbs
import truncation_oracle as to

GAP_BAR = sbs.GAP_BAR
plane = cm.plane          # (a MASK's planes of step t; a bias's: bias_plane below)


def bias_plane(bias, t):
  """bias [N, Tm, K] -> float32 [N, K] of decode step t (Tm == 1: the one plane)."""
  bias = np.asarray(bias, dtype=np.float32)
  return bias[:, 0 if bias.shape[1] == 1 else t]


def _all(allowed, shape):
  if allowed is None:
    return np.ones(shape, dtype=bool)
  return np.broadcast_to(np.asarray(allowed) != 0, shape)


def proposal_w(logits, bias, temperature, dtype=np.float32):
  """w = l / tau + b in `dtype`, each operation rounded, as the kernels form it."""
  l = np.asarray(logits).astype(dtype)
  w = l if float(temperature) == 1.0 else (l / dtype(temperature)).astype(dtype)
  return (w + np.asarray(bias).astype(dtype)).astype(dtype)


def _keep_row(l, b, temperature, top_k, top_p, floor):
  """truncation_oracle._keep_row with the order taken of w: c(k) counts the cells whose FLOAT32 w
  is larger (the kernel's order, ties share a count); the masses are float64.  The band of the
  tight / wide sets is LOGIT_BAND on w in units of l, i.e. on w * tau."""
  w32 = proposal_w(l, b, temperature, np.float32)
  tau = float(np.float32(temperature))
  w = np.asarray(l, dtype=np.float32).astype(np.float64) / tau + \
      np.asarray(b, dtype=np.float32).astype(np.float64)
  e = np.exp(w - w.max())
  order = np.argsort(-w32, kind="stable")
  ws = w32[order]
  c = np.searchsorted(-ws, -w32, side="left")
  m = np.concatenate([[0.0], np.cumsum(e[order])])[c]
  total = e.sum()

  def keep_at(p, use_p):
    ok = np.ones(len(w), dtype=bool)
    if top_k > 0:
      ok &= c < top_k
    if use_p:
      ok &= m < p * total
    return ok | (c < floor)

  p = float(np.float32(top_p))
  use_p = p < 1.0
  keep = keep_at(p, use_p)
  lo, hi = keep_at(p - to.MASS_BAND, use_p), keep_at(p + to.MASS_BAND, use_p)
  wl = w * tau
  tight = lo.copy()
  if (~lo).any():
    tight &= wl > wl[~lo].max() + to.LOGIT_BAND
  wide = hi | (wl >= wl[hi].min() - to.LOGIT_BAND)
  return keep, tight, wide


def keep_sets(logits, bias, allowed, temperature, top_k, top_p, floor=1):
  """cell_mask_oracle.keep_sets under `bias` [..., K] (broadcast): -> (keep, tight, wide)."""
  logits = np.asarray(logits, dtype=np.float32)
  K = logits.shape[-1]
  fa = _all(allowed, logits.shape).reshape(-1, K)
  fb = np.broadcast_to(np.asarray(bias, dtype=np.float32), logits.shape).reshape(-1, K)
  flat = logits.reshape(-1, K)
  floors = np.broadcast_to(np.asarray(floor), logits.shape[:-1]).reshape(-1)
  out = np.zeros((3,) + flat.shape, dtype=bool)
  for r in range(flat.shape[0]):
    idx = np.nonzero(fa[r])[0]
    sets = _keep_row(flat[r, idx], fb[r, idx], temperature, top_k, top_p, int(floors[r]))
    for i in range(3):
      out[i, r, idx] = sets[i]
  return tuple(o.reshape(logits.shape) for o in out)


def proposal(logits, bias, temperature, keep, allowed, dtype=np.float32):
  """cell_mask_oracle.proposal over w = l / tau + b."""
  w = proposal_w(logits, np.broadcast_to(np.asarray(bias), np.asarray(logits).shape), temperature,
                 dtype)
  allowed = _all(allowed, w.shape)
  mx = np.where(allowed, w, -np.inf).max(axis=-1, keepdims=True)
  with np.errstate(over="ignore", invalid="ignore"):
    e = np.where(keep, np.exp(np.where(keep, w - mx, -np.inf)), dtype(0)).astype(dtype)
    lse = np.log(e.sum(axis=-1, keepdims=True, dtype=dtype))
    return np.where(keep, (w - mx) - lse, -np.inf).astype(dtype)


def biased_ids(lp, bias, temperature, g, mask):
  """truncation_oracle.masked_ids with the score (lp / tau + b) + g, float32."""
  score = ((np.asarray(lp, dtype=np.float32) / np.float32(temperature) +
            np.asarray(bias, dtype=np.float32)).astype(np.float32) +
           np.asarray(g, dtype=np.float32)).astype(np.float32)
  score = np.where(mask, score, -np.inf)
  top2 = np.sort(score, axis=-1)[..., -2:].astype(np.float64)
  ids = np.where(mask.any(axis=-1), np.argmax(score, axis=-1), -1).astype("int32")
  with np.errstate(invalid="ignore"):
    margin = np.where(np.isfinite(top2[..., 0]), top2[..., 1] - top2[..., 0], np.inf)
  return ids, margin


def draw(logits, lp, g, bias, allowed, temperature, top_k=0, top_p=1.0, floor=1,
         dtype=np.float64):
  """cell_mask_oracle.draw under `bias` [..., K] (broadcast over the futures of a sample)."""
  shape = np.asarray(logits).shape
  allowed = _all(allowed, shape)
  bias = np.broadcast_to(np.asarray(bias, dtype=np.float32), shape)
  keep, tight, wide = keep_sets(logits, bias, allowed, temperature, top_k, top_p, floor)
  ids, _ = biased_ids(lp, bias, temperature, g, keep)
  ids_t, _ = biased_ids(lp, bias, temperature, g, tight)
  ids_w, margin = biased_ids(lp, bias, temperature, g, wide)
  q = proposal(logits, bias, temperature, keep, allowed, dtype)
  pick = lambda a: np.take_along_axis(a, ids[..., None].astype(np.int64), axis=-1)[..., 0]
  return {"keep": keep, "tight": tight, "wide": wide, "ids": ids,
          "compared": (ids_t == ids_w) & (ids == ids_w) & (margin >= GAP_BAR),
          "sure": (tight == wide).all(axis=-1),
          "lp_id": pick(np.asarray(lp, dtype=np.float32)), "q_id": pick(q), "q": q}


def sample_step(logits, S, t, allowed, bias, temperature=1.0, seed=0, top_k=0, top_p=1.0,
                floor=1, dtype=np.float64):
  """mv_op_sample_step_biased: logits [R, K], allowed [R // S, K] or None, bias [R // S, K]."""
  logits = np.asarray(logits, dtype=np.float32)
  R, K = logits.shape
  g = so.step_noise(R // S, S, K, seed, t).reshape(R, K)
  arows = None if allowed is None else \
      np.repeat(np.asarray(allowed).reshape(R // S, K) != 0, S, axis=0)
  brows = np.repeat(np.asarray(bias, dtype=np.float32).reshape(R // S, K), S, axis=0)
  out = draw(logits, sbs.log_softmax(logits), g, brows, arows, temperature, top_k, top_p, floor,
             dtype)
  lpd = sbs.log_softmax(logits.astype(dtype))
  out["lp_id"] = np.take_along_axis(lpd, out["ids"][:, None].astype(np.int64), axis=-1)[:, 0]
  return out


def beam_step(logits, prev_lp, allowed, bias, time, diverse, gamma, fix_num_timestep,
              dtype=np.float32):
  """mv_op_beam_step_biased: cell_mask_oracle.beam_step with the candidate (prev_lp + lp) + b,
  bias [N, K], formed before the mask's -inf and the ranks."""
  l = np.asarray(logits).astype(dtype)
  N, B, K = l.shape
  a = _all(None if allowed is None else np.asarray(allowed).reshape(N, 1, K), (N, 1, K))
  lp = (np.asarray(prev_lp).astype(dtype)[..., None] + sbs.log_softmax(l)).astype(dtype)
  lp = (lp + np.asarray(bias).astype(dtype).reshape(N, 1, K)).astype(dtype)
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


def sbs_step(logits, prev_phi, prev_lp, prev_g, t, allowed, bias, temperature=1.0, seed=0,
             dtype=np.float32, row_base=0, top_k=0, top_p=1.0):
  """cell_mask_oracle.sbs_step with the proposal over w = l / tau + b, bias [N, K]."""
  N, B, K = logits.shape
  l = np.asarray(logits).astype(dtype)
  phi, LP, G = (np.asarray(x).astype(dtype) for x in (prev_phi, prev_lp, prev_g))
  a = _all(None if allowed is None else np.asarray(allowed).reshape(N, 1, K), l.shape)
  b = np.broadcast_to(np.asarray(bias, dtype=np.float32).reshape(N, 1, K), l.shape)
  lp = sbs.log_softmax(l)
  keep = keep_sets(logits, b, a, temperature, top_k, top_p, B if t == 0 else 1)[0]
  q = proposal(l, b, temperature, keep, a, dtype)
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


def occupancy(logits, logprobs, mask, bias, uniform=False, dtype=np.float64):
  """mv_beam_occupancy under bias [N, Tm, K] (and mask [N, Tm, K] or None) in `dtype`: the step
  maps are the softmax of l + b over A."""
  x = np.asarray(logits).astype(dtype)
  N, B, T, K = x.shape
  lp = np.zeros((N, B), dtype=dtype) if uniform else np.asarray(logprobs).astype(dtype)
  w = np.exp(lp - lp.max(-1, keepdims=True))
  w = (w / w.sum(-1, keepdims=True, dtype=dtype)).astype(dtype)
  out = np.zeros((N, T, K), dtype=dtype)
  for t in range(T):
    a = np.ones((N, 1, K), dtype=bool) if mask is None else cm.plane(mask, t)[:, None, :]
    xb = (x[:, :, t] + bias_plane(bias, t).astype(dtype)[:, None, :]).astype(dtype)
    xt = np.where(a, xb, -np.inf).astype(dtype)
    e = np.exp(xt - xt.max(-1, keepdims=True)).astype(dtype)
    p = (e / e.sum(-1, keepdims=True, dtype=dtype)).astype(dtype)
    for b in range(B):                                     # the beams in order, each product rounded
      out[:, t] = (out[:, t] + (p[:, b] * w[:, b, None]).astype(dtype)).astype(dtype)
  return out


# ---- the forwards: the existing loops with the choosing function swapped while the call lasts

def _mask_plane(mask, t):
  return None if mask is None else cm.plane(mask, t)[:, None, :]


def sampled_forward(params, cfg, feed, mask, bias, temperature=1.0, seed=0, top_k=0, top_p=1.0):
  """truncation_oracle.forward (independent sampler) under bias [N, Tm, K], mask or None."""
  step = [0]

  def biased_draw(logits, lp, g, temp, k, p):
    t = step[0]
    step[0] += 1
    return draw(logits, lp, g, bias_plane(bias, t)[:, None, :], _mask_plane(mask, t), temp, k, p)

  with cm._swapped(to, "draw", biased_draw):             # pylint: disable=protected-access
    return to.forward(params, cfg, feed, temperature=temperature, seed=seed, top_k=top_k,
                      top_p=top_p)


def sbs_forward(params, cfg, feed, mask, bias, temperature=1.0, seed=0):
  """sbs_oracle.forward (sampling without replacement) under bias [N, Tm, K], mask or None."""
  def biased_step(logits, phi, LP, G, t, temp, sd, dtype=np.float32):
    return sbs_step(logits, phi, LP, G, t, None if mask is None else cm.plane(mask, t),
                    bias_plane(bias, t), temp, sd, dtype=dtype)

  with cm._swapped(sbs, "step", biased_step):            # pylint: disable=protected-access
    return sbs.forward(params, cfg, feed, temperature=temperature, seed=seed)


def beam_forward(params, cfg, feed, mask, bias):
  """The oracle's beam decoder under bias [N, Tm, K], mask or None: its log-softmax of step t
  comes back as lp + b, -inf outside A(n, t), so that its candidate is prev_lp + (lp + b) -- the
  definition's (prev_lp + lp) + b but for the order of two float32 additions, which the beams'
  comparator takes within its bar -> (oreg, (ologits, oids, olp), trace)."""
  import torch
  plain = oracle.log_softmax_tf
  N, B = cfg.batch_size, cfg.beam_size
  step = [0]

  def biased_log_softmax(x):
    lp = plain(x)
    if x.dim() != 3 or tuple(x.shape[:2]) != (N, B):
      return lp
    t = step[0]
    step[0] += 1
    lp = lp + torch.from_numpy(bias_plane(bias, t)[:, None, :].copy()).to(lp.dtype)
    if mask is None:
      return lp
    a = torch.from_numpy(cm.plane(mask, t)[:, None, :].copy())
    return torch.where(a, lp, torch.full_like(lp, float("-inf")))

  trace = {}
  with cm._swapped(oracle, "log_softmax_tf", biased_log_softmax):   # pylint: disable=protected-access
    _, oreg, obeam = oracle.forward(params, cfg, feed, trace=trace)
  assert step[0] == int(feed["pred_length"])
  return oreg, obeam, trace
