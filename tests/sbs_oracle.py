# coding=utf-8
"""Test-side restatement of the sampling WITHOUT replacement (mv_set_sampling_mode 1: stochastic
beam search, Kool, van Hoof, Welling, ICML 2019; the reference has none, the step is defined by
include/multiverse_hip.h): the class decoder loop of sampling_oracle.forward with the parent
gather of (c, h) and the Gumbel-top-B step below, and the generator of the sampler.

Slot b of batch row n carries phi (tempered log-probability), LP (untempered, reported) and G
(perturbed score); one root per row with phi = LP = G = 0.  Decode step t, parent slot b:
  lp = log_softmax(l);  q = lp at temperature 1, else log_softmax(l / temperature)
  g[k] = (phi_b + q[k]) - log(-log(u(b*K + k, row_seed(seed, n), t)));  Z = max_k g;  d = g - Z
  v = (G_b - g[k]) + log(-expm1(d)) for d < 0, -inf for d == 0
  Gt[k] = (G_b - max(v, 0)) - log1p(exp(-|v|))
  new slots = the B largest Gt over (b, k), descending, ties to the lower b*K + k; slot j from
  (b, k): phi = phi_b + q[k], LP = LP_b + lp[k], G = Gt[k], parent b, id k."""
import copy

import numpy as np
import torch

from oracle import multiverse_oracle as oracle
from sampling_oracle import hash32, row_seed, uniform, gumbel   # noqa: F401  pylint: disable=unused-import

GAP_BAR = 1e-4        # the bar of sampling_oracle.compared_steps


def log_softmax(x):
  """(x - max) - log(sum(exp(x - max))) in x's dtype, the terms of step_row_log_softmax."""
  mx = x.max(axis=-1, keepdims=True)
  lse = np.log(np.exp(x - mx).sum(axis=-1, keepdims=True, dtype=x.dtype))
  return ((x - mx) - lse).astype(x.dtype)


def step_uniform(N, B, K, seed, t, row_base=0):
  """float32 u [N, B, K] of decode step t: element b*K + k of row n, b the PARENT's slot."""
  i = (np.arange(B, dtype=np.uint64)[:, None] * np.uint64(K) +
       np.arange(K, dtype=np.uint64)[None, :])
  return np.stack([uniform(i, row_seed(seed, row_base + n), t) for n in range(N)])


def truncated(G, g, Z, form="expm1"):
  """Gt of the definition, in the dtype of the operands (G, Z broadcast over g).  form "log1p" is
  the paper's v = (G - g) + log1p(-exp(d)), kept for the comparison of the two."""
  d = g - Z
  with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
    tail = np.log(-np.expm1(d)) if form == "expm1" else np.log1p(-np.exp(d))
    v = np.where(d < 0, (G - g) + tail, -np.inf).astype(g.dtype)
    return ((G - np.maximum(v, 0)) - np.log1p(np.exp(-np.abs(v)))).astype(g.dtype)


def step(logits, prev_phi, prev_lp, prev_g, t, temperature=1.0, seed=0, dtype=np.float32,
         row_base=0, u=None):
  """One step on logits [N, B, K], prev_* [N, B] -> dict of new_phi, new_lp, new_g, ids, parents
  [N, B], lp, q [N, B, K] and gap [N]: the smallest adjacent gap among the B + 1 largest Gt.
  Everything after the float32 uniforms is evaluated in `dtype`.  t == 0: only slot 0 of a row
  is a candidate row (the root)."""
  N, B, K = logits.shape
  l = np.asarray(logits).astype(dtype)
  phi, LP, G = (np.asarray(a).astype(dtype) for a in (prev_phi, prev_lp, prev_g))
  lp = log_softmax(l)
  q = lp if float(temperature) == 1.0 else log_softmax((l / dtype(temperature)).astype(dtype))
  if u is None:
    u = step_uniform(N, B, K, seed, t, row_base)
  gum = (-np.log(-np.log(u.astype(dtype)))).astype(dtype)
  g = ((phi[..., None] + q) + gum).astype(dtype)
  Gt = truncated(G[..., None], g, g.max(axis=-1, keepdims=True))
  cand = Gt[:, 0, :] if t == 0 else Gt.reshape(N, B * K)
  order = np.argsort(-cand, axis=-1, kind="stable")       # descending, ties to the lower index
  top = order[:, :B]
  par, k = top // K, top % K
  rows = np.arange(N)[:, None]
  best = np.take_along_axis(cand, order[:, :B + 1], axis=-1).astype(np.float64)
  return {"new_phi": (phi[rows, par] + q[rows, par, k]).astype(dtype),
          "new_lp": (LP[rows, par] + lp[rows, par, k]).astype(dtype),
          "new_g": np.take_along_axis(cand, top, axis=-1),
          "ids": k.astype("int32"), "parents": par.astype("int32"), "lp": lp, "q": q,
          "gap": (best[:, :-1] - best[:, 1:]).min(axis=-1)}


def forward(params, cfg, feed, temperature=1.0, seed=0, dtype=torch.float32):
  """The forward of a beam config (B = cfg.beam_size, one scale) that samples without
  replacement: the model in `dtype`, the step in float64 on its float32 logits ->
  {"logits" [N,B,T,K], "ids" [N,B,T] (back-traced), "logprobs", "gumbels" [N,B], "grid_reg",
   "gap" [N,T], and per step "step_logits" [T][N,B,K], "step_ids", "step_parents" [T][N,B]}."""
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
    phi = np.zeros((N, S)); LP = np.zeros((N, S)); G = np.zeros((N, S))
    out = {"step_logits": [], "step_ids": [], "step_parents": [], "gap": []}
    for t in range(T_pred):
      if cfg.use_gnn:
        h = h + oracle.gnn_dense(h, sm)
      x = oracle.conv_layer(x_in, embW, embb, act=oracle.activation_of(cfg))
      c, h = oracle.convlstm_cell(x, c, h, kernel, biases)
      logits = oracle.conv2d_same(h, outW).reshape(N, S, K).to(torch.float32).numpy()
      st = step(logits, phi, LP, G, t, temperature, seed, dtype=np.float64)
      phi, LP, G = st["new_phi"], st["new_lp"], st["new_g"]
      out["step_logits"].append(logits)
      out["step_ids"].append(st["ids"])
      out["step_parents"].append(st["parents"])
      out["gap"].append(st["gap"])
      # the parent gather of (c, h); the next input is the drawn cell
      src = torch.from_numpy((np.arange(N)[:, None] * S + st["parents"]).reshape(-1).astype(np.int64))
      c, h = c[src], h[src]
      x_in = oracle.one_hot_grid(st["ids"].reshape(-1), H, W, dtype)
  ids = np.zeros((N, S, T_pred), dtype="int32")
  logits = np.zeros((N, S, T_pred, K), dtype=np.float32)
  for n in range(N):
    for j in range(S):
      path_ids, slots = trace_back(out, n, j, T_pred)
      ids[n, j] = path_ids
      for t in range(T_pred):
        logits[n, j, t] = out["step_logits"][t][n, slots[t]]
  out.update(ids=ids, logits=logits, logprobs=LP.astype(np.float32),
             gumbels=G.astype(np.float32), grid_reg=reg_out[s].numpy(),
             gap=np.stack(out["gap"], axis=1))
  return out


def trace_back(out, n, slot, steps):
  """Slot `slot` of row n after `steps` steps -> (its ids [steps], the state row slots[t] whose
  logits it read at step t): slots[t] is its ancestor among the slots selected at step t - 1."""
  path = np.zeros(steps, dtype="int32")
  slots = np.zeros(steps, dtype="int32")
  b = slot
  for t in range(steps - 1, -1, -1):
    path[t] = out["step_ids"][t][n, b]
    b = int(out["step_parents"][t][n, b])
    slots[t] = b
  return path, slots


def compared_steps(gap, bar=GAP_BAR):
  """[N] number of leading steps whose ids are compared: up to the first step whose gap among the
  B + 1 largest Gt is below `bar` (that step's logits are still compared, its ids are not)."""
  N, T = gap.shape
  upto = np.full(N, T, dtype=np.int64)
  for n in range(N):
    tied = np.nonzero(gap[n] < bar)[0]
    if len(tied):
      upto[n] = int(tied[0])
  return upto


# ---- the definition as a sampler over a small tree (the CPU test of the distribution)

def tree_draws(step_logits, B, temperature, seeds, dtype=np.float32, form="expm1"):
  """Two-step tree with K children per node: step_logits = (root [K], children [K, K]), the
  logits of the root and of every first-step cell.  One draw per row seed through the definition
  (all seeds at once) -> leaves int [S, B] (first * K + second, in slot order), gumbels [S, B],
  logprobs [S, B] (untempered), and best_equal: whether every parent's best child got
  Gt == G_parent bit for bit at both steps."""
  root, kids = (np.asarray(a, dtype=dtype) for a in step_logits)
  K = root.shape[0]
  S = len(seeds)
  tq = lambda l: log_softmax(l) if float(temperature) == 1.0 else \
      log_softmax((l / dtype(temperature)).astype(dtype))
  i = np.arange(B * K, dtype=np.uint64)
  sd = np.asarray(seeds, dtype=np.uint64)[:, None]        # every row seed at once
  noise = [(-np.log(-np.log(uniform(i[None, :], sd, t).astype(dtype)))).astype(dtype)
           .reshape(S, B, K) for t in (0, 1)]
  # step 0: the root's children
  q0, lp0 = tq(root), log_softmax(root)
  g = (dtype(0) + q0)[None, :] + noise[0][:, 0]
  Gt = truncated(dtype(0), g, g.max(-1, keepdims=True), form)
  best_equal = bool((Gt.max(-1) == 0).all())
  first = np.argsort(-Gt, axis=-1, kind="stable")[:, :B]             # [S, B]
  G1 = np.take_along_axis(Gt, first, -1)
  phi1, lp1 = q0[first], lp0[first]
  # step 1
  q1, lpk = tq(kids)[first], log_softmax(kids)[first]                # [S, B, K]
  g = (phi1[..., None] + q1) + noise[1]
  Gt = truncated(G1[..., None], g, g.max(-1, keepdims=True), form)
  best_equal = best_equal and bool((Gt.max(-1) == G1).all())
  flat = Gt.reshape(S, B * K)
  top = np.argsort(-flat, axis=-1, kind="stable")[:, :B]
  par, k = top // K, top % K
  rows = np.arange(S)[:, None]
  return {"leaves": first[rows, par] * K + k, "gumbels": np.take_along_axis(flat, top, -1),
          "logprobs": lp1[rows, par] + lpk[rows, par, k], "best_equal": best_equal}


def tree_leaf_probs(step_logits, temperature=1.0):
  """float64 [K*K] leaf probabilities of the (tempered) tree."""
  root, kids = (np.asarray(a, dtype=np.float64) / float(temperature) for a in step_logits)
  return np.exp(log_softmax(root)[:, None] + log_softmax(kids)).reshape(-1)
