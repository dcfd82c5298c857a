# coding=utf-8
"""Test-side restatement of the SCORING forward (mv_score_futures; the reference has no such
call, it is defined by include/multiverse_hip.h): the loop of sampling_oracle.forward with the
ids GIVEN instead of drawn, assembled from the building blocks of oracle/multiverse_oracle.py
(which it does not modify).

Decode step t of future f of batch row n, K cells, id = ids[n, f, t], for t < lengths[n, f]:
  lp                     = log_softmax(hidden2grid(h'))
  step_logprobs[n, f, t] = lp[id];  logprobs[n, f] += lp[id];  next input = grid_emb(one_hot(id))
  ranks[n, f, t]         = #{k : logit[k] > logit[id], or logit[k] == logit[id] and k < id}
and for t >= lengths[n, f]: step_logprobs 0, ranks -1, logits 0 (a finished future keeps
decoding on its last valid cell, which nothing reports)."""
import copy

import numpy as np
import torch

from oracle import multiverse_oracle as oracle


def ranks_of(logits, ids):
  """[..., K] logits, [...] ids -> the number of cells ranked before the given one."""
  logits = np.asarray(logits)
  ids = np.asarray(ids).astype(np.int64)
  at = np.take_along_axis(logits, ids[..., None], axis=-1)
  k = np.arange(logits.shape[-1])
  before = (logits > at) | ((logits == at) & (k < ids[..., None]))
  return before.sum(-1).astype(np.int32)


def gaps_of(logits, ids):
  """The distance from the given cell's logit to the nearest other logit of its row."""
  logits = np.asarray(logits, dtype=np.float64)
  ids = np.asarray(ids).astype(np.int64)
  at = np.take_along_axis(logits, ids[..., None], axis=-1)
  d = np.abs(logits - at)
  np.put_along_axis(d, ids[..., None], np.inf, axis=-1)
  return d.min(-1)


def forward(params, cfg, feed, ids, lengths=None, dtype=torch.float32):
  """The scoring forward of a beam config (F = cfg.beam_size, one scale) ->
  {"logits" [N,F,T,K], "step_logprobs" [N,F,T], "logprobs" [N,F], "ranks" [N,F,T],
   "grid_reg" [N,T,H,W,2], "gap" [N,F,T]}; logprobs accumulate in `dtype` in step order."""
  assert cfg.use_beam_search and sum(cfg.use_grids) == 1 and not cfg.use_single_decoder
  s = list(cfg.use_grids).index(True)
  H, W = cfg.scene_grids[s]
  K, F = H * W, cfg.beam_size
  T_pred = int(feed["pred_length"])
  npdt = np.float64 if dtype == torch.float64 else np.float32
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
    ids = np.asarray(ids).reshape(N, F, T_pred).astype(np.int64)
    lens = (np.full((N, F), T_pred, dtype=np.int64) if lengths is None
            else np.asarray(lengths).reshape(N, F).astype(np.int64))
    assert ((lens >= 0) & (lens <= T_pred)).all()
    # what the upload feeds a finished future: its last valid cell (0 for a padding future)
    fed = ids.copy()
    for n in range(N):
      for f in range(F):
        L = int(lens[n, f])
        assert L == 0 or ((fed[n, f, :L] >= 0) & (fed[n, f, :L] < K)).all()
        fed[n, f, L:] = fed[n, f, L - 1] if L else 0
    labels = np.asarray(feed["grid_obs_labels"][s])
    first = oracle.one_hot_grid(labels, H, W, dtype)[:, -1]

    def tile(t):
      return t.unsqueeze(1).expand(-1, F, -1, -1, -1).reshape(N * F, H, W, -1)

    scope = "decoder_grid_class_%d" % s
    kernel = P["%s/decoder_rnn/dec_grid_%d/kernel" % (scope, s)]
    biases = P["%s/decoder_rnn/dec_grid_%d/biases" % (scope, s)]
    embW = P["%s/decoder_rnn/grid_emb/W" % scope]
    embb = P["%s/decoder_rnn/grid_emb/b" % scope]
    outW = P["hidden2grid_%s/out_dec_grid/W" % scope]
    c, h, sm, x_in = tile(c0), tile(h0), tile(sm0), tile(first)
    logprobs = np.zeros((N, F), dtype=npdt)
    all_logits, all_lp, all_rank, all_gap = [], [], [], []
    for t in range(T_pred):
      if cfg.use_gnn:
        h = h + oracle.gnn_dense(h, sm)
      x = oracle.conv_layer(x_in, embW, embb, act=oracle.activation_of(cfg))
      c, h = oracle.convlstm_cell(x, c, h, kernel, biases)
      logits = oracle.conv2d_same(h, outW).reshape(N, F, K)
      lp = oracle.log_softmax_tf(logits).to(dtype).numpy()
      live = t < lens
      at = np.take_along_axis(lp, fed[:, :, t, None], axis=-1)[..., 0]
      step = np.where(live, at, 0).astype(npdt)
      logprobs = (logprobs + step).astype(npdt)
      lg = logits.numpy()
      all_logits.append(np.where(live[..., None], lg, 0).astype(npdt))
      all_lp.append(step)
      all_rank.append(np.where(live, ranks_of(lg, fed[:, :, t]), -1).astype(np.int32))
      all_gap.append(np.where(live, gaps_of(lg, fed[:, :, t]), np.inf))
      x_in = oracle.one_hot_grid(fed[:, :, t].reshape(-1), H, W, dtype)
  grid_reg = reg_out[s].numpy().copy()
  for n in range(N):
    grid_reg[n, int(lens[n].max()):] = 0
  return {"logits": np.stack(all_logits, axis=2), "step_logprobs": np.stack(all_lp, axis=2),
          "logprobs": logprobs, "ranks": np.stack(all_rank, axis=2), "grid_reg": grid_reg,
          "gap": np.stack(all_gap, axis=2)}
