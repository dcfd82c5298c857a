# coding=utf-8
"""Test-side restatement of the REVISIT COST (mv_set_revisit_cost: a per-row penalty for paths
that return to a cell they left; the reference has none, the definition is in
include/multiverse_hip.h), on top of motion_cost_oracle, which it imports and does not modify.

A revisit cost is a motion cost with one more term, so everything here is motion_cost_oracle with
the plane per ROW [N, B, K]
  b_eff[k] = b_m[k] + rterm(k)   in float32
where b_m is motion_cost_oracle's plane when a motion cost is set, else the bias plane or 0.0f, and
rterm(k) = cost[n] if k is in the row's visited set V and k != p1, else exactly 0.0f.  V holds the
row's observed cells (seed_observed; the last obs_lengths[n] of them) and the cells its path held
at the steps before, a slot's path being its parent's: the FULL set is carried beside each slot
here, as motion_cost_oracle.Path carries the last two cells."""
import numpy as np

from oracle import multiverse_oracle as oracle
import cell_bias_oracle as cb
import cell_mask_oracle as cm
import motion_cost_oracle as mo
import sbs_oracle as sbs
import truncation_oracle as to

GAP_BAR = mo.GAP_BAR
sample_step, beam_step, sbs_step = mo.sample_step, mo.beam_step, mo.sbs_step   # planes [N, B, K]


def rterm(visited, prev1, cost):
  """float32 [N, B, K]: visited bool [N, B, K] (the sets going INTO the step), prev1 int [N, B],
  cost [N] -- cell by cell, by the definition."""
  visited = np.asarray(visited) != 0
  N, B, K = visited.shape
  prev1 = np.asarray(prev1).reshape(N, B)
  cost = np.broadcast_to(np.asarray(cost, dtype=np.float32), (N,))
  out = np.zeros((N, B, K), dtype=np.float32)
  for n in range(N):
    for s in range(B):
      for k in range(K):
        if visited[n, s, k] and k != int(prev1[n, s]):
          out[n, s, k] = cost[n]
  return out


def row_planes(prev1, prev0, visited, W, K, cost, tables=None, bias=None):
  """b_eff float32 [N, B, K]: prev1 / prev0 int [N, B] (prev0 is read under a motion cost only),
  visited bool [N, B, K], cost [N], tables the dict of motion_cost_oracle or None, bias [N, K] (the
  samples' cell-bias planes of the step) or None."""
  prev1 = np.asarray(prev1)
  N, B = prev1.shape
  if tables is not None:
    bm = mo.row_planes(prev1, prev0, W, K, tables, bias)
  elif bias is not None:
    bm = np.repeat(np.asarray(bias, dtype=np.float32).reshape(N, 1, K), B, axis=1)
  else:
    bm = np.zeros((N, B, K), dtype=np.float32)
  return (bm.astype(np.float32) + rterm(visited, prev1, cost)).astype(np.float32)


def stored(visited, prev1):
  """The set a step kernel stores: visited | {prev1}, bool [N, B, K]."""
  out = np.array(np.asarray(visited) != 0, copy=True)
  N, B, _ = out.shape
  p1 = np.asarray(prev1).reshape(N, B)
  for n in range(N):
    for s in range(B):
      out[n, s, int(p1[n, s])] = True
  return out


class Path(mo.Path):
  """motion_cost_oracle.Path plus the visited set [N, B, K] of every row or slot going INTO
  decode step t: the observed cells (or nothing) at t == 0, then, with every step, the parent's
  set and the cell chosen."""

  def __init__(self, labels, B, K, obs_lengths=None, seed_observed=True):
    mo.Path.__init__(self, labels, B, obs_lengths)
    labels = np.asarray(labels)
    N, To = labels.shape
    self.visited = np.zeros((N, B, K), dtype=bool)
    if seed_observed:
      for n in range(N):
        lo = To if obs_lengths is None else int(obs_lengths[n])
        for c in labels[n, To - lo:]:
          self.visited[n, :, int(c)] = True

  def advance(self, ids, parents=None):
    ids = np.asarray(ids).astype(np.int64)
    N, B = ids.shape
    rows = np.arange(N)[:, None]
    v = self.visited if parents is None else self.visited[rows, np.asarray(parents)]
    v = np.array(v, copy=True)
    for n in range(N):
      for s in range(B):
        v[n, s, ids[n, s]] = True
    self.visited = v
    mo.Path.advance(self, ids, parents)


def _planes(path, W, K, cost, tables, bias, t):
  return row_planes(path.p1, path.p0, path.visited, W, K, cost, tables,
                    mo._bias_plane(bias, t))                 # pylint: disable=protected-access


def _path(cfg, feed, seed_observed):
  s, W, K = mo._grid(cfg)                                    # pylint: disable=protected-access
  return W, K, Path(feed["grid_obs_labels"][s], cfg.beam_size, K, feed.get("obs_lengths"),
                    seed_observed)


# ---- the forwards: motion_cost_oracle's, with the visited sets carried beside the last two cells

def sampled_forward(params, cfg, feed, cost, seed_observed=True, tables=None, mask=None, bias=None,
                    temperature=1.0, seed=0, top_k=0, top_p=1.0):
  """truncation_oracle.forward (independent sampler) under a revisit cost."""
  W, K, path = _path(cfg, feed, seed_observed)
  step = [0]

  def draw(logits, lp, g, temp, k, p):
    t = step[0]
    step[0] += 1
    planes = _planes(path, W, K, cost, tables, bias, t)
    m = mo._mask_plane(mask, t)                              # pylint: disable=protected-access
    out = cb.draw(logits, lp, g, planes, None if m is None else m[:, None, :], temp, k, p)
    path.advance(out["ids"])
    return out

  with cm._swapped(to, "draw", draw):                        # pylint: disable=protected-access
    return to.forward(params, cfg, feed, temperature=temperature, seed=seed, top_k=top_k,
                      top_p=top_p)


def sbs_forward(params, cfg, feed, cost, seed_observed=True, tables=None, mask=None, bias=None,
                temperature=1.0, seed=0):
  """sbs_oracle.forward (sampling without replacement) under a revisit cost."""
  W, K, path = _path(cfg, feed, seed_observed)

  def step(logits, phi, LP, G, t, temp, sd, dtype=np.float32):
    planes = _planes(path, W, K, cost, tables, bias, t)
    out = mo.sbs_step(logits, phi, LP, G, t, mo._mask_plane(mask, t), planes, temp, sd,  # pylint: disable=protected-access
                      dtype=dtype)
    path.advance(out["ids"], out["parents"])
    return out

  with cm._swapped(sbs, "step", step):                       # pylint: disable=protected-access
    return sbs.forward(params, cfg, feed, temperature=temperature, seed=seed)


def beam_forward(params, cfg, feed, cost, seed_observed=True, tables=None, mask=None, bias=None):
  """The oracle's beam decoder under a revisit cost, as motion_cost_oracle.beam_forward ->
  (oreg, (ologits, oids, olp), trace); trace["step_parents_np"]: the parents of every step."""
  import torch
  plain, plain_topk = oracle.log_softmax_tf, oracle.topk_stable
  N, B = cfg.batch_size, cfg.beam_size
  W, K, path = _path(cfg, feed, seed_observed)
  step = [0]
  parents = []

  def moved_log_softmax(x):
    lp = plain(x)
    if x.dim() != 3 or tuple(x.shape[:2]) != (N, B):
      return lp
    t = step[0]
    step[0] += 1
    planes = _planes(path, W, K, cost, tables, bias, t)
    lp = lp + torch.from_numpy(planes).to(lp.dtype)
    if mask is None:
      return lp
    a = torch.from_numpy(cm.plane(mask, t)[:, None, :].copy())
    return torch.where(a, lp, torch.full_like(lp, float("-inf")))

  def watched_topk(x, k):
    vals, idx = plain_topk(x, k)
    if k == B and x.shape[-1] in (K, B * K) and x.shape[0] == N:   # the step's selection
      idx_np = np.asarray(idx)
      path.advance(idx_np % K, idx_np // K)
      parents.append((idx_np // K).astype(np.int64))
    return vals, idx

  trace = {}
  with cm._swapped(oracle, "log_softmax_tf", moved_log_softmax):   # pylint: disable=protected-access
    with cm._swapped(oracle, "topk_stable", watched_topk):         # pylint: disable=protected-access
      _, oreg, obeam = oracle.forward(params, cfg, feed, trace=trace)
  assert step[0] == int(feed["pred_length"])
  trace["step_parents_np"] = parents
  return oreg, obeam, trace
