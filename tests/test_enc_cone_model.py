# coding=utf-8
"""The light cone of the class encoder (MV_ENC_CONE), on the CPU.

A 3x3 ConvLSTM that starts from the zero state and sees one hot cell per step: the cells where a
row's state differs AT ALL (bit for bit, fp64) from the input-free row's must lie inside the
exact-arithmetic cone of tests/enc_cone_twin.py at every step, and that cone inside the wider
rule the lists are built by (the F(3,3) kernel spreads dirt by whole row triples), for the scene
form of the input
(x = features * one_hot: reach r0 = 1) and for the embedded one-hot of models without scene
encoder (x = tanh(conv3x3(one_hot) + b): constant outside the 3x3, r0 = 2).  The library's host
builder (mv_enc_cone_build) must give the twin's lists, flags and counts."""
import numpy as np
import pytest

import enc_cone_twin as twin

T = 8
C = 4
GRIDS = [(18, 32), (9, 16)]


def paths(H, W):
  """name -> [T] cells of one row"""
  def cells(yx):
    return [y * W + x for y, x in yx]
  mid_y, mid_x = H // 2, W // 2
  return {
      "corner_still": cells([(0, 0)] * T),
      # image rows 2 | 3: the boundary between the first two row triples
      "triple_boundary": cells([(2, 5), (2, 5), (2, 6), (3, 6), (3, 7), (2, 7), (3, 8), (3, 8)]),
      # one step in a corner, the next in the opposite one: two disjoint cones
      "jump": cells([(H - 1, W - 1)] * 3 + [(0, 0)] * 5),
      # through the middle: the cone reaches every tile of the row before the last step
      "every_tile": cells([(mid_y, mid_x - 3 + t) for t in range(T)]),
  }


def conv3x3(x, w):
  """SAME 3x3 convolution, x [H, W, Ci], w [3, 3, Ci, Co]: elementwise sums in ONE fixed order,
  so equal neighbourhoods give equal bits wherever they sit."""
  H, W, Ci = x.shape
  xp = np.zeros((H + 2, W + 2, Ci))
  xp[1:-1, 1:-1] = x
  out = np.zeros((H, W, w.shape[3]))
  for dy in range(3):
    for dx in range(3):
      win = xp[dy:dy + H, dx:dx + W]
      for ci in range(Ci):
        out = out + win[:, :, ci:ci + 1] * w[dy, dx, ci][None, None, :]
  return out


def lstm_step(x, h, c, w, b):
  pre = conv3x3(np.concatenate([x, h], -1), w) + b
  i, j, f, o = np.split(pre, 4, -1)
  sig = lambda v: 1.0 / (1.0 + np.exp(-v))
  c2 = sig(f + 1.0) * c + sig(i) * np.tanh(j)
  return np.tanh(c2) * sig(o), c2


def differing_cells(path, H, W, r0, rng):
  """bool [T, H, W]: where (h, c) of the row with inputs differs from the input-free row's."""
  Cx = 3
  w = rng.standard_normal((3, 3, Cx + C, 4 * C)) * 0.5
  b = rng.standard_normal(4 * C) * 0.1
  emb_w = rng.standard_normal((3, 3, 1, Cx))
  emb_b = rng.standard_normal(Cx)
  def x_of(cell, t):
    hot = np.zeros((H, W, 1))
    if cell is not None:
      hot[cell // W, cell % W, 0] = 1.0
    if r0 == 1:          # features of the step's frame at the hot cell, zero elsewhere
      return hot * rng_feat[t][None, None, :]
    return np.tanh(conv3x3(hot, emb_w) + emb_b)
  rng_feat = rng.standard_normal((T, Cx))
  h = c = hb = cb = np.zeros((H, W, C))
  out = np.zeros((T, H, W), bool)
  for t in range(T):
    h, c = lstm_step(x_of(path[t], t), h, c, w, b)
    hb, cb = lstm_step(x_of(None, t), hb, cb, w, b)
    out[t] = (h != hb).any(-1) | (c != cb).any(-1)
  return out


@pytest.mark.parametrize("r0", [1, 2])
@pytest.mark.parametrize("grid", GRIDS)
def test_state_differs_only_inside_the_rule(grid, r0):
  H, W = grid
  rng = np.random.default_rng(1234 + 10 * r0 + H)
  for name, path in paths(H, W).items():
    labels = np.asarray([path], np.int32)
    cheb = twin.chebyshev_cells(labels, H, W, r0)[:, 0]
    rule = twin.rule_cells(labels, H, W, r0)[:, 0]
    diff = differing_cells(path, H, W, r0, rng)
    assert diff[0].any(), name                      # (the input does reach the state)
    for t in range(T):
      assert not (diff[t] & ~cheb[t]).any(), (name, t)
      assert not (cheb[t] & ~rule[t]).any(), (name, t)     # the kernel's rule is the wider one
    # neither is vacuous: a still corner reaches 9 x 9 cells (r0 = 1) by the last step in exact
    # arithmetic, and 9 columns of every row under the kernel's rule
    if name == "corner_still":
      assert cheb[T - 1].sum() == min(H, T + r0) * min(W, T + r0) < H * W
      assert rule[T - 1].sum() == H * min(W, T + r0) < H * W
      assert rule[1].sum() < cheb[T - 1].sum()


@pytest.mark.parametrize("grid", GRIDS)
def test_every_tile_path_activates_every_tile(grid):
  H, W = grid
  labels = np.asarray([paths(H, W)["every_tile"]], np.int32)
  lists, cells, ntile = twin.twin_lists(labels, H, W, 1)
  assert lists[3, 0] == ntile and cells[3] == 2 * H * W
  corner = np.asarray([paths(H, W)["corner_still"]], np.int32)
  lists, _, _ = twin.twin_lists(corner, H, W, 1)
  if W == 32:      # (at 9 x 16 and one row, every wave tile holds cells of the background row)
    assert lists[1, 0] == 1 + 6 < ntile


@pytest.mark.parametrize("r0", [1, 2])
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("N", [1, 3, 64])
def test_library_builder_is_the_twin(built_lib, grid, r0, N):
  """mv_enc_cone_build (host only) against the twin: hand-made paths in the first rows, random
  walks in the rest; lists, per-tile flags, counts and executed cells."""
  H, W = grid
  rng = np.random.default_rng(77 + N + H + r0)
  hand = list(paths(H, W).values())
  labels = np.zeros((N, T), np.int32)
  for n in range(N):
    if n < len(hand):
      labels[n] = hand[(n + N) % len(hand)]
    else:
      y, x = int(rng.integers(H)), int(rng.integers(W))
      for t in range(T):
        y = int(np.clip(y + rng.integers(-1, 2), 0, H - 1))
        x = int(np.clip(x + rng.integers(-1, 2), 0, W - 1))
        labels[n, t] = y * W + x
  lists, cells, ntile = built_lib.enc_cone_build(labels, H, W, r0)
  tl, tc, tn = twin.twin_lists(labels, H, W, r0)
  assert ntile == tn == ((N + 1) * ((H + 2) // 3) * W + 31) // 32
  assert (lists == tl).all()
  assert (cells == tc).all()
  assert cells[0] == cells[T - 1] == (N + 1) * H * W


def test_builder_rejects_bad_arguments(built_lib):
  with pytest.raises(built_lib.MvError):
    built_lib.enc_cone_build(np.full((2, T), 9 * 16, np.int32), 9, 16, 1)
