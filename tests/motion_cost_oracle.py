# coding=utf-8
"""Test-side restatement of the MOTION COSTS (mv_set_motion_cost: per-row speed and turn priors
for the beam search and both samplers; the reference has none, the definition is in
include/multiverse_hip.h), on top of cell_bias_oracle, which it imports and does not modify.

A motion cost is a cell bias whose plane depends on the row's path, so everything here is
cell_bias_oracle with a plane per ROW [N, B, K] in place of the plane per sample [N, K]:
  b_eff[k] = (b[k] + vterm(k)) + aterm(k)   in float32, in this order
with p1 / p0 the row's last two cells, d = cell(k) - cell(p1), u = cell(p1) - cell(p0),
a = d - u, vterm = vel[n, d + R] inside the window else vel_far[n], aterm likewise of acc / acc_far
and exactly 0.0f when there is no acc table or p0 is absent (-1).  Tables: a dict with "radius",
"vel" [N, D, D], "vel_far" [N] and "acc" / "acc_far" (or None), per SAMPLE."""
import numpy as np

from oracle import multiverse_oracle as oracle
import cell_bias_oracle as cb
import cell_mask_oracle as cm
import sbs_oracle as sbs
import truncation_oracle as to

GAP_BAR = cb.GAP_BAR


def tables_for(tables, N):
  """The tables broadcast to N samples (one row's [D, D] and scalars are taken for every row)."""
  R = int(tables["radius"])
  D = 2 * R + 1
  out = {"radius": R,
         "vel": np.broadcast_to(np.asarray(tables["vel"], dtype=np.float32), (N, D, D)).copy(),
         "vel_far": np.broadcast_to(np.asarray(tables["vel_far"], dtype=np.float32), (N,)).copy(),
         "acc": None, "acc_far": None}
  if tables.get("acc") is not None:
    out["acc"] = np.broadcast_to(np.asarray(tables["acc"], dtype=np.float32), (N, D, D)).copy()
    out["acc_far"] = np.broadcast_to(np.asarray(tables["acc_far"], dtype=np.float32), (N,)).copy()
  return out


def terms(p1, p0, W, K, tables, n):
  """(vterm, aterm) float32 [K] of one row of sample n whose path ends in p0 -> p1 (p0 -1:
  absent), by the definition, cell by cell."""
  R = int(tables["radius"])
  v = np.empty(K, dtype=np.float32)
  a = np.zeros(K, dtype=np.float32)
  y1, x1 = int(p1) // W, int(p1) % W
  turn = tables.get("acc") is not None and int(p0) >= 0
  if turn:
    uy, ux = y1 - int(p0) // W, x1 - int(p0) % W
  for k in range(K):
    dy, dx = k // W - y1, k % W - x1
    v[k] = tables["vel"][n, dy + R, dx + R] if max(abs(dy), abs(dx)) <= R else tables["vel_far"][n]
    if turn:
      ay, ax = dy - uy, dx - ux
      a[k] = tables["acc"][n, ay + R, ax + R] if max(abs(ay), abs(ax)) <= R \
          else tables["acc_far"][n]
  return v, a


def row_planes(prev1, prev0, W, K, tables, bias=None):
  """b_eff float32 [N, B, K]: prev1 / prev0 int [N, B], bias [N, K] (the samples' cell-bias
  planes of the step) or None."""
  prev1, prev0 = np.asarray(prev1), np.asarray(prev0)
  N, B = prev1.shape
  tables = tables_for(tables, N)
  out = np.empty((N, B, K), dtype=np.float32)
  for n in range(N):
    b = np.zeros(K, dtype=np.float32) if bias is None else \
        np.asarray(bias, dtype=np.float32).reshape(N, K)[n]
    for s in range(B):
      v, a = terms(prev1[n, s], prev0[n, s], W, K, tables, n)
      out[n, s] = ((b + v).astype(np.float32) + a).astype(np.float32)
  return out


def _all(allowed, N, K):
  if allowed is None:
    return np.ones((N, 1, K), dtype=bool)
  return np.asarray(allowed).reshape(N, 1, K) != 0


# ---- the three steps: cell_bias_oracle's, with `planes` [N, B, K] per row for bias [N, K]

def sample_step(logits, S, t, allowed, planes, temperature=1.0, seed=0, top_k=0, top_p=1.0,
                floor=1, dtype=np.float64):
  """mv_op_sample_step_motion: logits [R, K], allowed [R // S, K] or None, planes [R, K]."""
  logits = np.asarray(logits, dtype=np.float32)
  R, K = logits.shape
  g = cb.so.step_noise(R // S, S, K, seed, t).reshape(R, K)
  arows = None if allowed is None else \
      np.repeat(np.asarray(allowed).reshape(R // S, K) != 0, S, axis=0)
  brows = np.asarray(planes, dtype=np.float32).reshape(R, K)
  out = cb.draw(logits, sbs.log_softmax(logits), g, brows, arows, temperature, top_k, top_p, floor,
                dtype)
  lpd = sbs.log_softmax(logits.astype(dtype))
  out["lp_id"] = np.take_along_axis(lpd, out["ids"][:, None].astype(np.int64), axis=-1)[:, 0]
  return out


def beam_step(logits, prev_lp, allowed, planes, time, diverse, gamma, fix_num_timestep,
              dtype=np.float32):
  """mv_op_beam_step_motion: cell_bias_oracle.beam_step with the candidate (prev_lp + lp) + b_eff,
  planes [N, B, K], formed before the mask's -inf and the ranks."""
  l = np.asarray(logits).astype(dtype)
  N, B, K = l.shape
  a = _all(allowed, N, K)
  lp = (np.asarray(prev_lp).astype(dtype)[..., None] + sbs.log_softmax(l)).astype(dtype)
  lp = (lp + np.asarray(planes).astype(dtype).reshape(N, B, K)).astype(dtype)
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


def sbs_step(logits, prev_phi, prev_lp, prev_g, t, allowed, planes, temperature=1.0, seed=0,
             dtype=np.float32, row_base=0, top_k=0, top_p=1.0):
  """cell_bias_oracle.sbs_step with the proposal over w = l / tau + b_eff, planes [N, B, K]."""
  N, B, K = logits.shape
  l = np.asarray(logits).astype(dtype)
  phi, LP, G = (np.asarray(x).astype(dtype) for x in (prev_phi, prev_lp, prev_g))
  a = np.broadcast_to(_all(allowed, N, K), l.shape)
  b = np.asarray(planes, dtype=np.float32).reshape(N, B, K)
  lp = sbs.log_softmax(l)
  keep = cb.keep_sets(logits, b, a, temperature, top_k, top_p, B if t == 0 else 1)[0]
  q = cb.proposal(l, b, temperature, keep, a, dtype)
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


# ---- the path state of a forward

class Path(object):
  """p1 / p0 [N, B] of every row or slot going INTO decode step t: the last two observed labels
  at t == 0 (p0 -1 for a row observed for one frame), then the cells chosen so far, a slot's
  path being its parent's."""

  def __init__(self, labels, B, obs_lengths=None):
    labels = np.asarray(labels)
    N, To = labels.shape
    self.p1 = np.repeat(labels[:, To - 1:To], B, axis=1).astype(np.int64)
    if To >= 2:
      self.p0 = np.repeat(labels[:, To - 2:To - 1], B, axis=1).astype(np.int64)
    else:
      self.p0 = np.full((N, B), -1, dtype=np.int64)
    if obs_lengths is not None:
      self.p0[np.asarray(obs_lengths) < 2] = -1

  def advance(self, ids, parents=None):
    ids = np.asarray(ids).astype(np.int64)
    rows = np.arange(ids.shape[0])[:, None]
    self.p0 = self.p1.copy() if parents is None else self.p1[rows, np.asarray(parents)]
    self.p1 = ids


def _grid(cfg):
  s = list(cfg.use_grids).index(True)
  H, W = cfg.scene_grids[s]
  return s, W, H * W


def _mask_plane(mask, t):
  return None if mask is None else cm.plane(mask, t)


def _bias_plane(bias, t):
  return None if bias is None else cb.bias_plane(bias, t)


# ---- the forwards: cell_bias_oracle's, with the plane of each step built from the path so far

def sampled_forward(params, cfg, feed, tables, mask=None, bias=None, temperature=1.0, seed=0,
                    top_k=0, top_p=1.0):
  """truncation_oracle.forward (independent sampler) under a motion cost."""
  s, W, K = _grid(cfg)
  path = Path(feed["grid_obs_labels"][s], cfg.beam_size, feed.get("obs_lengths"))
  step = [0]

  def draw(logits, lp, g, temp, k, p):
    t = step[0]
    step[0] += 1
    planes = row_planes(path.p1, path.p0, W, K, tables, _bias_plane(bias, t))
    m = _mask_plane(mask, t)
    out = cb.draw(logits, lp, g, planes, None if m is None else m[:, None, :], temp, k, p)
    path.advance(out["ids"])
    return out

  with cm._swapped(to, "draw", draw):                    # pylint: disable=protected-access
    return to.forward(params, cfg, feed, temperature=temperature, seed=seed, top_k=top_k,
                      top_p=top_p)


def sbs_forward(params, cfg, feed, tables, mask=None, bias=None, temperature=1.0, seed=0):
  """sbs_oracle.forward (sampling without replacement) under a motion cost."""
  s, W, K = _grid(cfg)
  path = Path(feed["grid_obs_labels"][s], cfg.beam_size, feed.get("obs_lengths"))

  def step(logits, phi, LP, G, t, temp, sd, dtype=np.float32):
    planes = row_planes(path.p1, path.p0, W, K, tables, _bias_plane(bias, t))
    out = sbs_step(logits, phi, LP, G, t, _mask_plane(mask, t), planes, temp, sd, dtype=dtype)
    path.advance(out["ids"], out["parents"])
    return out

  with cm._swapped(sbs, "step", step):                   # pylint: disable=protected-access
    return sbs.forward(params, cfg, feed, temperature=temperature, seed=seed)


def beam_forward(params, cfg, feed, tables, mask=None, bias=None):
  """The oracle's beam decoder under a motion cost, as cell_bias_oracle.beam_forward: its
  log-softmax of step t comes back as lp + b_eff, and the selection it makes from that (its
  top-B of the candidates) advances the paths -> (oreg, (ologits, oids, olp), trace)."""
  import torch
  plain, plain_topk = oracle.log_softmax_tf, oracle.topk_stable
  N, B = cfg.batch_size, cfg.beam_size
  s, W, K = _grid(cfg)
  path = Path(feed["grid_obs_labels"][s], B, feed.get("obs_lengths"))
  step = [0]

  def moved_log_softmax(x):
    lp = plain(x)
    if x.dim() != 3 or tuple(x.shape[:2]) != (N, B):
      return lp
    t = step[0]
    step[0] += 1
    planes = row_planes(path.p1, path.p0, W, K, tables, _bias_plane(bias, t))
    lp = lp + torch.from_numpy(planes).to(lp.dtype)
    if mask is None:
      return lp
    a = torch.from_numpy(cm.plane(mask, t)[:, None, :].copy())
    return torch.where(a, lp, torch.full_like(lp, float("-inf")))

  def watched_topk(x, k):
    vals, idx = plain_topk(x, k)
    if k == B and x.shape[-1] in (K, B * K) and x.shape[0] == N:   # the step's selection
      path.advance(idx % K, idx // K)
    return vals, idx

  trace = {}
  with cm._swapped(oracle, "log_softmax_tf", moved_log_softmax):   # pylint: disable=protected-access
    with cm._swapped(oracle, "topk_stable", watched_topk):         # pylint: disable=protected-access
      _, oreg, obeam = oracle.forward(params, cfg, feed, trace=trace)
  assert step[0] == int(feed["pred_length"])
  return oreg, obeam, trace
