# coding=utf-8
"""Test-side restatement of the TRUNCATED sampling (mv_set_sampling_truncation: top-k and nucleus
limits on both samplers; the reference has none, the kept set is defined by
include/multiverse_hip.h), assembled from the blocks of sampling_oracle.py and sbs_oracle.py,
which it imports and does not modify.

Per row, l = the step's logits, w = l / temperature, e = exp(w - max w):
  c(k) = #{j : l[j] > l[k]};  m(k) = sum of e[j] over {j : l[j] > l[k]}
  keep(k) = c(k) < floor  or  ((top_k == 0 or c(k) < top_k) and (top_p >= 1 or m(k) < top_p * sum e))
  q~[k] = (w[k] - max w) - log(sum of e over the kept cells), -inf on dropped cells
The engine decides the kept set in float32 on ITS logits, which differ from the oracle's within
the project's logit bar, so every kept set comes twice: "tight" (certainly kept) and "wide"
(possibly kept).  A cell whose logit lies within LOGIT_BAND of the kept boundary, or whose
float64 m(k) / sum e lies within MASS_BAND of top_p, is in wide and not in tight.  A drawn id is
compared only where both sets give the same id with a score margin of GAP_BAR or more."""
import copy

import numpy as np
import torch

from oracle import multiverse_oracle as oracle
import sampling_oracle as so
import sbs_oracle as sbs

LOGIT_BAND = 2e-4     # 2 x the project's logit bar: two logits that far apart cannot swap
MASS_BAND = 1e-5      # ~10 x the rounding of a (J + 6)-deep float32 sum plus two ulps of expf
GAP_BAR = sbs.GAP_BAR


def _keep_row(l, temperature, top_k, top_p, floor):
  """float64 on one row of float32 logits -> (keep, tight, wide) bool [K]."""
  l = np.asarray(l, dtype=np.float32).astype(np.float64)
  w = l / float(np.float32(temperature))
  e = np.exp(w - w.max())
  order = np.argsort(-l, kind="stable")
  ls = l[order]
  c = np.searchsorted(-ls, -l, side="left")               # strictly better cells; ties share it
  m = np.concatenate([[0.0], np.cumsum(e[order])])[c]
  total = e.sum()

  def keep_at(p, use_p):
    ok = np.ones(len(l), dtype=bool)
    if top_k > 0:
      ok &= c < top_k
    if use_p:
      ok &= m < p * total
    return ok | (c < floor)

  p = float(np.float32(top_p))
  use_p = p < 1.0                                         # off means off: never evaluated
  keep = keep_at(p, use_p)
  lo, hi = keep_at(p - MASS_BAND, use_p), keep_at(p + MASS_BAND, use_p)
  tight = lo.copy()
  if (~lo).any():
    tight &= l > l[~lo].max() + LOGIT_BAND
  wide = hi | (l >= l[hi].min() - LOGIT_BAND)
  return keep, tight, wide


def keep_sets(logits, temperature, top_k, top_p, floor=1):
  """logits [..., K] -> (keep, tight, wide) bool [..., K]; floor an int or an array [...]."""
  logits = np.asarray(logits, dtype=np.float32)
  flat = logits.reshape(-1, logits.shape[-1])
  floors = np.broadcast_to(np.asarray(floor), logits.shape[:-1]).reshape(-1)
  rows = [_keep_row(r, temperature, top_k, top_p, int(f)) for r, f in zip(flat, floors)]
  return tuple(np.stack([r[i] for r in rows]).reshape(logits.shape) for i in range(3))


def proposal(logits, temperature, keep, dtype=np.float32):
  """q~ [..., K] in `dtype` over the kept set `keep`: the terms of sbs_oracle.log_softmax with the
  sum taken over the kept cells (all kept: the same bits), -inf on dropped cells."""
  l = np.asarray(logits).astype(dtype)
  w = l if float(temperature) == 1.0 else (l / dtype(temperature)).astype(dtype)
  mx = w.max(axis=-1, keepdims=True)
  e = np.where(keep, np.exp(w - mx), dtype(0)).astype(dtype)
  lse = np.log(e.sum(axis=-1, keepdims=True, dtype=dtype))
  return np.where(keep, (w - mx) - lse, -np.inf).astype(dtype)


def masked_ids(lp, temperature, g, mask):
  """sampling_oracle.sample_ids over the cells of `mask` -> (ids, top-1 / top-2 margin among
  them); id -1 where the mask is empty, margin inf where it has one cell."""
  score = (np.asarray(lp, dtype=np.float32) / np.float32(temperature) +
           np.asarray(g, dtype=np.float32)).astype(np.float32)
  score = np.where(mask, score, -np.inf)
  top2 = np.sort(score, axis=-1)[..., -2:].astype(np.float64)
  ids = np.where(mask.any(axis=-1), np.argmax(score, axis=-1), -1).astype("int32")
  with np.errstate(invalid="ignore"):
    margin = np.where(np.isfinite(top2[..., 0]), top2[..., 1] - top2[..., 0], np.inf)
  return ids, margin


def draw(logits, lp, g, temperature, top_k, top_p, floor=1, dtype=np.float64):
  """One truncated draw per row: logits, lp (float32 log-softmax), g (noise) [..., K] ->
  dict of keep / tight / wide, ids (from the exact kept set), compared (bool [...]: tight and wide
  give that same id with a margin of GAP_BAR or more), sure (bool [...]: no cell of the row lies
  in the band, so every kept set is the exact one), lp_id (float32, the model's), q_id (`dtype`,
  the proposal's) of the drawn ids, q [..., K]."""
  keep, tight, wide = keep_sets(logits, temperature, top_k, top_p, floor)
  ids, _ = masked_ids(lp, temperature, g, keep)
  ids_t, _ = masked_ids(lp, temperature, g, tight)
  ids_w, margin = masked_ids(lp, temperature, g, wide)
  q = proposal(logits, temperature, keep, dtype)
  pick = lambda a: np.take_along_axis(a, ids[..., None].astype(np.int64), axis=-1)[..., 0]
  return {"keep": keep, "tight": tight, "wide": wide, "ids": ids,
          "compared": (ids_t == ids_w) & (ids == ids_w) & (margin >= GAP_BAR),
          "sure": (tight == wide).all(axis=-1),
          "lp_id": pick(np.asarray(lp, dtype=np.float32)), "q_id": pick(q), "q": q}


def sample_step(logits, S, t, temperature=1.0, seed=0, top_k=0, top_p=1.0, floor=1,
                dtype=np.float64):
  """mv_op_sample_step: logits [R, K], row r = future r % S of sample r // S -> draw() with lp in
  `dtype` as well ("lp_id")."""
  logits = np.asarray(logits, dtype=np.float32)
  R, K = logits.shape
  g = so.step_noise(R // S, S, K, seed, t).reshape(R, K)
  lp32 = sbs.log_softmax(logits)
  out = draw(logits, lp32, g, temperature, top_k, top_p, floor, dtype)
  lpd = sbs.log_softmax(logits.astype(dtype))
  out["lp_id"] = np.take_along_axis(lpd, out["ids"][:, None].astype(np.int64), axis=-1)[:, 0]
  return out


def forward(params, cfg, feed, temperature=1.0, seed=0, top_k=0, top_p=1.0,
            dtype=torch.float32):
  """sampling_oracle.forward with the truncated draw (floor 1: independent mode) -> its dict plus
  "proposal_logprobs" [N, S] (float64 sum of the float64 q~ of the drawn ids) and "compared",
  "sure" [N, S, T] (draw()) in place of "margin"."""
  assert cfg.use_beam_search and sum(cfg.use_grids) == 1 and not cfg.use_single_decoder
  s = list(cfg.use_grids).index(True)
  H, W = cfg.scene_grids[s]
  K, S = H * W, cfg.beam_size
  T_pred = int(feed["pred_length"])
  gcfg = copy.copy(cfg)
  gcfg.use_beam_search, gcfg.beam_size = False, 1
  P = oracle.Params(params, dtype)
  trace = {}
  with torch.no_grad():
    _, reg_out, _ = oracle.forward_tensors(P, gcfg, feed, dtype, trace)
    c0 = torch.from_numpy(trace["enc_class_c_%d" % s]).to(dtype)
    h0 = torch.from_numpy(trace["enc_class_h_%d" % s]).to(dtype)
    sm0 = torch.from_numpy(trace["scene_mean_%d" % s]).to(dtype)
    N = h0.shape[0]
    labels = np.asarray(feed["grid_obs_labels"][s])
    first = oracle.one_hot_grid(labels, H, W, dtype)[:, -1]

    def tile(t):
      return t.unsqueeze(1).expand(-1, S, -1, -1, -1).reshape(N * S, H, W, -1)

    scope = "decoder_grid_class_%d" % s
    kernel = P["%s/decoder_rnn/dec_grid_%d/kernel" % (scope, s)]
    biases = P["%s/decoder_rnn/dec_grid_%d/biases" % (scope, s)]
    embW = P["%s/decoder_rnn/grid_emb/W" % scope]
    embb = P["%s/decoder_rnn/grid_emb/b" % scope]
    outW = P["hidden2grid_%s/out_dec_grid/W" % scope]
    c, h, sm, x_in = tile(c0), tile(h0), tile(sm0), tile(first)
    logprobs = np.zeros((N, S), dtype=np.float32)
    qlogprobs = np.zeros((N, S), dtype=np.float64)
    all_logits, all_ids, all_cmp, all_sure = [], [], [], []
    for t in range(T_pred):
      if cfg.use_gnn:
        h = h + oracle.gnn_dense(h, sm)
      x = oracle.conv_layer(x_in, embW, embb, act=oracle.activation_of(cfg))
      c, h = oracle.convlstm_cell(x, c, h, kernel, biases)
      logits = oracle.conv2d_same(h, outW).reshape(N, S, K)
      lp = oracle.log_softmax_tf(logits).to(torch.float32).numpy()
      d = draw(logits.to(torch.float32).numpy(), lp, so.step_noise(N, S, K, seed, t),
               temperature, top_k, top_p)
      logprobs = (logprobs + d["lp_id"]).astype(np.float32)
      qlogprobs = qlogprobs + d["q_id"]
      all_logits.append(logits.numpy())
      all_ids.append(d["ids"])
      all_cmp.append(d["compared"])
      all_sure.append(d["sure"])
      x_in = oracle.one_hot_grid(d["ids"].reshape(-1), H, W, dtype)
  return {"logits": np.stack(all_logits, axis=2), "ids": np.stack(all_ids, axis=2),
          "logprobs": logprobs, "proposal_logprobs": qlogprobs, "grid_reg": reg_out[s].numpy(),
          "compared": np.stack(all_cmp, axis=2), "sure": np.stack(all_sure, axis=2)}


def compared_steps(compared):
  """[N, S] number of leading steps whose ids are compared: up to the first step that is not
  (that step's logits are still compared, its id is not), as sampling_oracle.compared_steps."""
  N, S, T = compared.shape
  upto = np.full((N, S), T, dtype=np.int64)
  for n in range(N):
    for s in range(S):
      bad = np.nonzero(~compared[n, s])[0]
      if len(bad):
        upto[n, s] = int(bad[0])
  return upto


# ---- the definition as a sampler over a small tree (the CPU tests of the distribution)

def tree_draws(step_logits, B, temperature, seeds, top_k=0, top_p=1.0, dtype=np.float32):
  """sbs_oracle.tree_draws with the truncated proposal: floor B at the root, 1 below it ->
  its dict plus "phi" [S, B], the leaves' log-probability under the proposal."""
  root, kids = (np.asarray(a, dtype=dtype) for a in step_logits)
  K = root.shape[0]
  S = len(seeds)
  i = np.arange(B * K, dtype=np.uint64)
  sd = np.asarray(seeds, dtype=np.uint64)[:, None]
  noise = [(-np.log(-np.log(so.uniform(i[None, :], sd, t).astype(dtype)))).astype(dtype)
           .reshape(S, B, K) for t in (0, 1)]
  q0 = proposal(root, temperature, keep_sets(root, temperature, top_k, top_p, B)[0], dtype)
  lp0 = sbs.log_softmax(root)
  qk = proposal(kids, temperature, keep_sets(kids, temperature, top_k, top_p, 1)[0], dtype)
  lpk = sbs.log_softmax(kids)

  def scores(G, g):       # a dropped cell is the candidate -inf, explicitly
    finite = np.isfinite(g)
    safe = np.where(finite, g, dtype(0))
    Z = np.where(finite, g, -np.inf).max(-1, keepdims=True)
    return np.where(finite, sbs.truncated(G, safe, np.maximum(Z, safe)), -np.inf).astype(dtype)

  # step 0: the root's children
  g = (dtype(0) + q0)[None, :] + noise[0][:, 0]
  Gt = scores(dtype(0), g)
  best_equal = bool((Gt.max(-1) == 0).all())
  first = np.argsort(-Gt, axis=-1, kind="stable")[:, :B]
  G1 = np.take_along_axis(Gt, first, -1)
  phi1, lp1 = q0[first], lp0[first]
  # step 1
  g = (phi1[..., None] + qk[first]) + noise[1]
  Gt = scores(G1[..., None], g)
  best_equal = best_equal and bool((Gt.max(-1) == G1).all())
  flat = Gt.reshape(S, B * K)
  top = np.argsort(-flat, axis=-1, kind="stable")[:, :B]
  par, k = top // K, top % K
  rows = np.arange(S)[:, None]
  return {"leaves": first[rows, par] * K + k, "gumbels": np.take_along_axis(flat, top, -1),
          "logprobs": lp1[rows, par] + lpk[first][rows, par, k],
          "phi": phi1[rows, par] + qk[first][rows, par, k], "best_equal": best_equal}


def tree_leaf_probs(step_logits, temperature=1.0, top_k=0, top_p=1.0, B=1):
  """float64 [K*K] leaf probabilities of the tempered, truncated tree (floor B at the root)."""
  root, kids = (np.asarray(a, dtype=np.float32) for a in step_logits)
  q0 = proposal(root, temperature, keep_sets(root, temperature, top_k, top_p, B)[0], np.float64)
  qk = proposal(kids, temperature, keep_sets(kids, temperature, top_k, top_p, 1)[0], np.float64)
  return np.exp(q0[:, None] + qk).reshape(-1)
