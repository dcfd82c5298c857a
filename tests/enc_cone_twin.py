# coding=utf-8
"""numpy twin of the class encoder's light cone (csrc/engine_io.h build_enc_cone),
shared by tests/test_enc_cone_model.py and tests/test_gpu_enc_cone.py.

The encoder starts from the zero state and sees one hot cell per row and step, so a row's state
equals the input-free (background) row's except at DIRTY cells.  In exact arithmetic the dirty
cells after step t are those within Chebyshev distance t - s + r0 of an observed cell s <= t
(r0: how far a step's own input reaches; chebyshev_cells).  The F(3,3) gate kernel computes the
three rows of a triple from the FIVE input rows 3k - 1 .. 3k + 3, and the rows a 3 x 3 stencil
would not read cancel only in exact arithmetic, so for a bit-identical result dirt spreads from
any of those five rows to the whole triple, and one column per step along x (rule_cells).  The
gate kernel's unit is a wave tile: 32 consecutive triple-cells
q = (row * ceil(H / 3) + y // 3) * W + x of the N + 1 rows (row N = the background row)."""
import numpy as np


def chebyshev_cells(labels, H, W, r0):
  """labels [N, T] -> bool [T, N, H, W]: where the state can differ in exact arithmetic."""
  N, T = labels.shape
  yy, xx = np.mgrid[0:H, 0:W]
  out = np.zeros((T, N, H, W), bool)
  for n in range(N):
    for t in range(T):
      for s in range(t + 1):
        ys, xs = divmod(int(labels[n, s]), W)
        out[t, n] |= np.maximum(np.abs(yy - ys), np.abs(xx - xs)) <= t - s + r0
  return out


def rule_cells(labels, H, W, r0):
  """labels [N, T] -> bool [T, N, H, W]: the dirty cells after step t, as the kernel's row
  triples spread them."""
  N, T = labels.shape
  yy, xx = np.mgrid[0:H, 0:W]
  out = np.zeros((T, N, H, W), bool)
  D = np.zeros((N, H, W), bool)
  for t in range(T):
    Dx = D.copy()
    Dx[:, :, 1:] |= D[:, :, :-1]
    Dx[:, :, :-1] |= D[:, :, 1:]
    G = np.zeros_like(D)
    for k in range((H + 2) // 3):
      lo, hi = max(3 * k - 1, 0), min(3 * k + 3, H - 1)
      G[:, 3 * k:3 * k + 3, :] = Dx[:, lo:hi + 1, :].any(1)[:, None, :]
    for n in range(N):
      ys, xs = divmod(int(labels[n, t]), W)
      G[n] |= np.maximum(np.abs(yy - ys), np.abs(xx - xs)) <= r0
    D = G
    out[t] = D
  return out


def tile_of_cells(N, H, W):
  """int [N + 1, H, W]: the wave tile of every cell of the N + 1 rows."""
  Kt = ((H + 2) // 3) * W
  r, y, x = np.mgrid[0:N + 1, 0:H, 0:W]
  return (r * Kt + (y // 3) * W + x) >> 5


def twin_lists(labels, H, W, r0):
  """What mv_enc_cone_build returns: lists [T, 4 + 2 ntile], cells [T], ntile.  The first and
  the last step run every tile, the background row's tiles are always active."""
  N, T = labels.shape
  tiles = tile_of_cells(N, H, W)
  ntile = int(tiles.max()) + 1
  cells_rule = rule_cells(labels, H, W, r0)
  lists = np.zeros((T, 4 + 2 * ntile), np.int32)
  cells = np.zeros((T,), np.int64)
  for t in range(T):
    flag = np.zeros(ntile, bool)
    if t == 0 or t == T - 1:
      flag[:] = True
    else:
      flag[np.unique(tiles[N])] = True
      flag[np.unique(tiles[:N][cells_rule[t]])] = True
    act = np.nonzero(flag)[0]
    lists[t, 0] = len(act)
    lists[t, 4:4 + len(act)] = act
    lists[t, 4 + ntile:] = flag
    cells[t] = int(flag[tiles].sum())
  return lists, cells, ntile


def executed_gate_flops(cfg, feed, cone):
  """kernel_stats()["convlstm_step"]["flops"] of one greedy forward of an f16x3 / bf16 inference
  engine with sparse x (csrc/engine_forward.h gate_group_cost): 2 * cells * 9 * Cin * 4C per
  launch, Cin = the channels whose k-steps run.  cone: the class encoder's h-steps count the
  cone's cells (and steps 0 / T - 1 the background row's)."""
  N, T, Tp, C = cfg.batch_size, cfg.obs_len, int(feed.get("pred_length", cfg.pred_len)), 256
  E = cfg.emb_size
  total = 0.0
  for s, (H, W) in enumerate(cfg.scene_grids):
    if not cfg.use_grids[s]:
      continue
    M = N * H * W
    enc_cls = [float(M)] * T
    # (csrc/gate_plan.h enc_cone_geometry: grids of fewer than five row triples stay dense)
    if cone and T >= 3 and H % 3 == 0 and H // 3 >= 5 and W == 32:
      _, cells, _ = twin_lists(np.asarray(feed["grid_obs_labels"][s]).reshape(N, T), H, W,
                               1 if cfg.use_scene_enc else 2)
      enc_cls = [float(c) for c in cells]
    for t in range(T):
      hc = 0 if t == 0 else C
      total += 2.0 * enc_cls[t] * 9 * hc * 4 * C          # class encoder: x is table terms
      total += 2.0 * M * 9 * (2 + hc) * 4 * C             # regression encoder: 2 fp32 x channels
    for _ in range(Tp):
      total += 2.0 * M * 9 * C * 4 * C                    # class decoder: x is table terms
      total += 2.0 * M * 9 * (E + C) * 4 * C              # regression decoder
  return total
