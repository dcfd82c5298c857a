# coding=utf-8
"""The reference of a mixed-length training step (include/multiverse_hip.h
mv_set_train_lengths), composed from UNIFORM runs of oracle.loss_and_grads.

No operation of the model couples batch rows, so with per-row lengths (Lo[n], L[n]) the loss
parts and every gradient are sums over the groups of rows with the same (Lo, L) pair:

  * run the uniform model at obs_len = Lo, pred_len = L on the group's sub-batch (observations:
    the rows' LAST Lo columns; targets: their FIRST L columns), wd = 0;
  * weight the group's classification part by |g| L / M, M = sum_n L[n]: the group's own mean
    runs over |g| L rows, the batch's over M;
  * weight its regression part the same way, or -- mask_grid_regression -- by the group's
    foreground count over the batch's (the masked mean runs over the foreground cells);
  * add wd * W once (wd_cost over every */W).

The weights are folded into the group's grid_loss_weight / grid_reg_loss_weight, which scale
the two parts and nothing else, so that one autograd pass per group gives the weighted
gradients; a weight of exactly 1 leaves the run the whole batch's, bit for bit.
"""
import copy

import numpy as np
import torch

from oracle import multiverse_oracle as oracle

_GROUP_CACHE = {}


def groups_of(obs_lengths, pred_lengths):
  """{(Lo, L): [rows]} over the rows with L > 0, in first-appearance order."""
  out = {}
  for n, (lo, l) in enumerate(zip(obs_lengths, pred_lengths)):
    if int(l) > 0:
      out.setdefault((int(lo), int(l)), []).append(n)
  return out


def slice_feed(cfg, feed, rows, Lo, L):
  """(cfg, feed) of the uniform (obs_len = Lo, pred_len = L) model on the rows `rows`."""
  rows = np.asarray(rows, dtype=np.int64)
  sub = copy.copy(cfg)
  sub.batch_size = len(rows)
  sub.obs_len = int(Lo)
  sub.pred_len = int(L)
  sub.wd = 0.0
  To = np.asarray(feed["obs_scene"]).shape[1]
  out = dict(feed)
  out["pred_length"] = int(L)
  out["obs_scene"] = np.ascontiguousarray(np.asarray(feed["obs_scene"])[rows][:, To - Lo:])

  def per_scale(key, take):
    if feed.get(key) is None:
      return
    out[key] = [None if a is None else np.ascontiguousarray(take(np.asarray(a)[rows]))
                for a in feed[key]]

  per_scale("grid_obs_labels", lambda a: a[:, To - Lo:])
  per_scale("grid_obs_regress", lambda a: a[:, To - Lo:])
  per_scale("grid_pred_labels", lambda a: a[:, :L])
  per_scale("grid_pred_regress", lambda a: a[:, :L])
  per_scale("grid_pred_soft", lambda a: a[:, :L])
  return sub, out


def _foreground(cfg, feed, rows, L):
  """Foreground cells of the rows' first L target steps, per used scale."""
  counts = []
  for s, use in enumerate(cfg.use_grids):
    if not use:
      continue
    if getattr(cfg, "use_soft_grid_class", False):
      soft = np.asarray(feed["grid_pred_soft"][s])[np.asarray(rows)][:, :L]
      counts.append(int((soft > 0).sum()))
    else:
      counts.append(len(rows) * int(L))      # one-hot maps: one cell per (n, t)
  return counts


def loss_and_grads(params, cfg, feed, obs_lengths, pred_lengths, dtype=torch.float32,
                   cache_key=None):
  """-> (loss, wd_loss, pred_grid_loss, grads) of the mixed-length step, as
  oracle.loss_and_grads returns them for a uniform one.  cache_key: the group runs (wd = 0) of
  a case are kept, so that engine runs in several compute modes -- and with several wd -- share
  them."""
  key = None if cache_key is None else (cache_key, str(dtype))
  if key is None or key not in _GROUP_CACHE:
    groups = groups_of(obs_lengths, pred_lengths)
    assert groups, "at least one row must have a prediction length > 0"
    M = sum(L * len(rows) for (_, L), rows in groups.items())
    masked = bool(getattr(cfg, "mask_grid_regression", False))
    fg = {g: _foreground(cfg, feed, rows, g[1]) for g, rows in groups.items()}
    fg_total = [sum(fg[g][i] for g in groups) for i in range(len(next(iter(fg.values()))))]
    pgl, grads = None, None
    for (Lo, L), rows in groups.items():
      sub, sfeed = slice_feed(cfg, feed, rows, Lo, L)
      w_cls = len(rows) * L / float(M)
      if masked:
        ws = [fg[(Lo, L)][i] / float(fg_total[i]) for i in range(len(fg_total))]
        assert max(ws) - min(ws) < 1e-15, "the scales' foreground shares differ: weight per part"
        w_reg = ws[0]
      else:
        w_reg = w_cls
      if len(groups) > 1 or w_cls != 1.0 or w_reg != 1.0:
        sub.grid_loss_weight = cfg.grid_loss_weight * w_cls
        sub.grid_reg_loss_weight = cfg.grid_reg_loss_weight * w_reg
      _, _, gp, gg = oracle.loss_and_grads(params, sub, sfeed, dtype=dtype)
      npd = np.float64 if dtype == torch.float64 else np.float32
      if pgl is None:
        pgl = [npd(v) for v in gp]
        grads = {n: (np.zeros_like(params[n], dtype=npd) if g is None else g.astype(npd))
                 for n, g in gg.items()}
      else:
        pgl = [a + npd(b) for a, b in zip(pgl, gp)]
        for n, g in gg.items():
          if g is not None:
            grads[n] = grads[n] + g.astype(npd)
    if key is not None:
      _GROUP_CACHE[key] = (pgl, grads)
  else:
    pgl, grads = _GROUP_CACHE[key]
  npd = np.float64 if dtype == torch.float64 else np.float32
  grads = dict(grads)
  wd_loss = npd(0)
  if cfg.wd:
    for n in sorted(params):
      if n.endswith("/W"):
        w = params[n].astype(npd)
        grads[n] = grads[n] + npd(cfg.wd) * w
        wd_loss = wd_loss + npd(cfg.wd) * npd(0.5) * (w * w).sum(dtype=npd)
  loss = pgl[0]
  for v in pgl[1:]:
    loss = loss + v
  loss = loss + wd_loss
  return float(loss), float(wd_loss), [float(v) for v in pgl], grads


def train_step(params, opt_state, global_step, cfg, feed, obs_lengths, pred_lengths,
               dtype=torch.float32):
  """oracle.train_step with the composed gradients: clip, oracle.apply_optimizer,
  -> (loss, wd_loss, pred_grid_loss, new_params, new_state, grads)."""
  loss, wd, pgl, grads = loss_and_grads(params, cfg, feed, obs_lengths, pred_lengths, dtype)
  lr = oracle.learning_rate(cfg, global_step)
  npd = np.float64 if dtype == torch.float64 else np.float32
  new_params, new_state = {}, {}
  powers = opt_state.get("")
  for n, v in params.items():
    g = grads[n].astype(npd)
    if cfg.clip_gradient_norm is not None:
      g = np.clip(g, -cfg.clip_gradient_norm, cfg.clip_gradient_norm)
    new_params[n], new_state[n] = oracle.apply_optimizer(cfg, lr, v, g, opt_state[n], npd, powers)
  if powers is not None:
    new_state[""] = (np.float32(powers[0]) * np.float32(0.9),
                     np.float32(powers[1]) * np.float32(0.999))
  return loss, wd, pgl, new_params, new_state, grads
