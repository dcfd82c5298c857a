# coding=utf-8
"""Test-side restatement of the SAMPLED multi-future decode (mv_set_sampling; the reference has
no sampler, the draw is defined by include/multiverse_hip.h): the class decoder loop of
oracle.beam_decoder with the top-B selection replaced by one Gumbel-max draw per row, assembled
from the building blocks of oracle/multiverse_oracle.py (which it does not modify), and the
counter-based generator the engine shares with the training dropout.

Decode step t of future s of batch row n, float32, K cells:
  lp    = log_softmax(hidden2grid(h'))
  u[k]  = (top 24 bits of hash32(s*K + k, row_seed(seed, n), t) + 0.5) * 2^-24, held below 1
  id    = argmax_k lp[k] / temperature - log(-log(u[k])), lowest index among equal scores
  next input = grid_emb(one_hot(id));  logprob[n, s] += lp[id]"""
import copy

import numpy as np
import torch

from oracle import multiverse_oracle as oracle

ROW_SEED = 0x632BE5AB
_M32 = np.uint64(0xFFFFFFFF)


def row_seed(seed, n):
  """Batch row n draws as row 0 of a forward seeded row_seed(seed, n) does."""
  return (int(seed) + int(n) * ROW_SEED) & 0xFFFFFFFF


def hash32(i, seed, stream):
  """csrc/kernels_misc.h hash32 on an array of element numbers -> uint32."""
  i = np.asarray(i, dtype=np.uint64) & _M32
  x = (i * np.uint64(0x9E3779B1) + np.uint64(seed & 0xFFFFFFFF) * np.uint64(0x85EBCA77) +
       np.uint64(stream & 0xFFFFFFFF) * np.uint64(0xC2B2AE3D)) & _M32
  x ^= x >> np.uint64(16)
  x = (x * np.uint64(0x7FEB352D)) & _M32
  x ^= x >> np.uint64(15)
  x = (x * np.uint64(0x846CA68B)) & _M32
  x ^= x >> np.uint64(16)
  return x.astype(np.uint32)


def uniform_from_bits(top24):
  """(top24 + 0.5) * 2^-24 evaluated in float32 (codes from 2^23 on round to even), the one
  code that rounds to 1.0 held at the largest float32 below it."""
  u = (np.asarray(top24).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)
  return np.minimum(u, np.float32(1.0) - np.float32(2.0 ** -24)).astype(np.float32)


def uniform(i, seed, stream):
  return uniform_from_bits(hash32(i, seed, stream) >> np.uint32(8))


def gumbel(i, seed, stream):
  u = uniform(i, seed, stream)
  return (-np.log(-np.log(u))).astype(np.float32)


def step_noise(N, S, K, seed, t, row_base=0):
  """g [N, S, K] of decode step t."""
  i = (np.arange(S, dtype=np.uint64)[:, None] * np.uint64(K) +
       np.arange(K, dtype=np.uint64)[None, :])
  return np.stack([gumbel(i, row_seed(seed, row_base + n), t) for n in range(N)])


def sample_ids(lp, temperature, g):
  """(ids, top-1 / top-2 score margin) of float32 lp, g [..., K]."""
  score = (np.asarray(lp, dtype=np.float32) / np.float32(temperature) +
           np.asarray(g, dtype=np.float32)).astype(np.float32)
  top2 = np.sort(score, axis=-1)[..., -2:].astype(np.float64)
  return np.argmax(score, axis=-1).astype("int32"), top2[..., 1] - top2[..., 0]


def forward(params, cfg, feed, temperature=1.0, seed=0, dtype=torch.float32):
  """The sampled forward of a beam config (S = cfg.beam_size, one scale) ->
  {"logits" [N,S,T,K], "ids" [N,S,T], "logprobs" [N,S], "grid_reg" [N,T,H,W,2],
   "margin" [N,S,T] (top-1 / top-2 gap of the step's scores)}."""
  assert cfg.use_beam_search and sum(cfg.use_grids) == 1 and not cfg.use_single_decoder
  s = list(cfg.use_grids).index(True)
  H, W = cfg.scene_grids[s]
  K, S = H * W, cfg.beam_size
  T_pred = int(feed["pred_length"])
  # encoders, scene mean and the un-beamed regression decoder: the oracle's greedy graph
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
    all_logits, all_ids, all_margin = [], [], []
    for t in range(T_pred):
      if cfg.use_gnn:
        h = h + oracle.gnn_dense(h, sm)
      x = oracle.conv_layer(x_in, embW, embb, act=oracle.activation_of(cfg))
      c, h = oracle.convlstm_cell(x, c, h, kernel, biases)
      logits = oracle.conv2d_same(h, outW).reshape(N, S, K)
      lp = oracle.log_softmax_tf(logits).to(torch.float32).numpy()
      ids, margin = sample_ids(lp, temperature, step_noise(N, S, K, seed, t))
      logprobs = (logprobs + np.take_along_axis(lp, ids[..., None].astype(np.int64),
                                                axis=-1)[..., 0]).astype(np.float32)
      all_logits.append(logits.numpy())
      all_ids.append(ids)
      all_margin.append(margin)
      x_in = oracle.one_hot_grid(ids.reshape(-1), H, W, dtype)
  return {"logits": np.stack(all_logits, axis=2), "ids": np.stack(all_ids, axis=2),
          "logprobs": logprobs, "grid_reg": reg_out[s].numpy(),
          "margin": np.stack(all_margin, axis=2)}


def compared_steps(margin, bar=1e-4):
  """[N, S] number of leading steps whose ids are compared: up to the first step whose oracle
  margin is below `bar` (that step's logits are still compared, its id is not)."""
  N, S, T = margin.shape
  upto = np.full((N, S), T, dtype=np.int64)
  for n in range(N):
    for s in range(S):
      tied = np.nonzero(margin[n, s] < bar)[0]
      if len(tied):
        upto[n, s] = int(tied[0])
  return upto
