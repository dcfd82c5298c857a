# coding=utf-8
"""Test-side oracle of a model built WITHOUT the scene encoder (`--use_scene_enc` off, the
reference's default graph): `Model.build_forward` of code/pred_models.py with
`config.use_scene_enc == False`, assembled from the building blocks of
oracle/multiverse_oracle.py (which it does not modify).

Differences from the published graph:
  - no scene stack (:146-165 skipped);
  - class encoder input x_t = grid_emb(one_hot(grid_obs_labels[:, t])) through ONE pair
    person_pred/grid_emb/{W,b} shared by the scales (:218-229);
  - graph attention node features = h alone, greedy and beam (:824-838): here a scene mean
    with zero channels, which the oracle's gnn_dense concatenates as nothing.
Everything else (decoders, beam search, loss, optimizers) is the oracle's own code."""
import numpy as np
import torch

from oracle import multiverse_oracle as oracle

EMB_W = "person_pred/grid_emb/W"
EMB_B = "person_pred/grid_emb/b"


def forward_tensors(P, cfg, feed, dtype=torch.float32, trace=None):
  assert not cfg.use_scene_enc
  drop = None
  if cfg.is_train and cfg.keep_prob < 1.0:
    drop = oracle._Dropout(cfg.keep_prob, int(feed.get("dropout_seed", 0)))  # pylint: disable=protected-access
  cls_fb = "onehot" if (not cfg.is_train or cfg.train_w_onehot) else "dense"
  C = cfg.enc_hidden_size
  T_pred = int(feed["pred_length"])
  act = oracle.activation_of(cfg)
  cls_out, reg_out, beam_out = [], [], None
  for s, (H, W) in enumerate(cfg.scene_grids):
    if not cfg.use_grids[s]:
      cls_out.append([])
      reg_out.append([])
      continue
    labels = np.asarray(feed["grid_obs_labels"][s])
    obs_oh = oracle.one_hot_grid(labels, H, W, dtype)           # [N,T,H,W,1]
    N, T = labels.shape
    emb = oracle.conv_layer(obs_oh.reshape(N * T, H, W, 1), P["grid_emb/W"], P["grid_emb/b"],
                            act=act)
    x_cls = emb.reshape(N, T, H, W, -1)
    obs_reg = oracle._t(feed["grid_obs_regress"][s], dtype)     # pylint: disable=protected-access
    enc_c = oracle.run_encoder(
        x_cls, P["encoder_grid_class_%d/enc_grid_%d/kernel" % (s, s)],
        P["encoder_grid_class_%d/enc_grid_%d/biases" % (s, s)], C, drop)
    enc_r = oracle.run_encoder(
        obs_reg, P["encoder_grid_reg_%d/enc_grid_regress_%d/kernel" % (s, s)],
        P["encoder_grid_reg_%d/enc_grid_regress_%d/biases" % (s, s)], C, drop)
    no_scene = torch.zeros(N, H, W, 0, dtype=dtype)             # node features = h alone
    if trace is not None:
      trace["enc_class_h_%d" % s] = enc_c[1].detach().numpy()
    if cfg.use_beam_search:
      assert not cfg.is_train and sum(cfg.use_grids) == 1
      best, lg, ids, lps = oracle.beam_decoder(P, cfg, s, obs_oh[:, -1], enc_c, T_pred,
                                               no_scene, trace)
      dec_cls = best
      beam_out = [lg, ids, lps]
    else:
      dec_cls, _ = oracle.greedy_decoder(P, cfg, s, "class", obs_oh[:, -1], enc_c, T_pred,
                                         no_scene, trace, feedback=cls_fb, drop=drop)
    dec_reg, _ = oracle.greedy_decoder(P, cfg, s, "reg", obs_reg[:, -1], enc_r, T_pred,
                                       no_scene, trace, feedback="dense", drop=drop)
    cls_out.append(dec_cls)
    reg_out.append(dec_reg)
  return cls_out, reg_out, beam_out


def forward(params, cfg, feed, dtype=torch.float32, trace=None):
  P = oracle.Params(params, dtype)
  with torch.no_grad():
    cls_out, reg_out, beam_out = forward_tensors(P, cfg, feed, dtype, trace)
  cls_out = [c if isinstance(c, list) else c.numpy() for c in cls_out]
  reg_out = [r if isinstance(r, list) else r.numpy() for r in reg_out]
  if beam_out is not None:
    beam_out = [beam_out[0].numpy(), beam_out[1], beam_out[2].numpy()]
  return cls_out, reg_out, beam_out


def loss_and_grads(params, cfg, feed, dtype=torch.float32):
  P = oracle.Params(params, dtype)
  for v in P.p.values():
    v.requires_grad_(True)
  cls_out, reg_out, _ = forward_tensors(P, cfg, feed, dtype)
  loss, wd, pgl = oracle.build_loss(P, cfg, cls_out, reg_out, feed, dtype)
  names = sorted(P.p)
  gs = torch.autograd.grad(loss, [P.p[n] for n in names], allow_unused=True)
  grads = {n: (None if g is None else g.numpy()) for n, g in zip(names, gs)}
  return (float(loss.detach()), float(wd.detach()), [float(l.detach()) for l in pgl], grads)


def train_step(params, opt_state, global_step, cfg, feed, dtype=torch.float32):
  """oracle.train_step on this graph: loss, gradients, element-wise clip, optimizer."""
  loss, wd, pgl, grads = loss_and_grads(params, cfg, feed, dtype)
  lr = oracle.learning_rate(cfg, global_step)
  npd = np.float64 if dtype == torch.float64 else np.float32
  new_params, new_state = {}, {}
  powers = opt_state.get("")
  for n, v in params.items():
    g = grads[n].astype(npd)
    if cfg.clip_gradient_norm is not None:
      g = np.clip(g, -cfg.clip_gradient_norm, cfg.clip_gradient_norm)
    new_params[n], new_state[n] = oracle.apply_optimizer(cfg, lr, v, g, opt_state[n], npd,
                                                         powers)
  return loss, wd, pgl, new_params, new_state, grads
