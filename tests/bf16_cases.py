# coding=utf-8
"""Inputs and operand rounding shared by the bf16 kernel tests (tests/test_gpu_bf16_kernels.py) and
their CPU-side checks (tests/test_bf16_oracle.py): which operand parts compute mode 2 holds as one
bf16 plane, and the one-hot cases of the 32-cell body."""

import numpy as np


def bf16_round(a):
  """round-to-nearest-even to bf16, as the planes hold the operands in compute mode 2"""
  u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
  u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
  return u.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def rounded_operands(x, h, kernel, x_passes=1):
  """(x, h, kernel) as the gate kernels of compute mode 2 see them: h and the kernel rows it meets
  as bf16; a dense x (16-channel groups) and its rows as bf16 too when it takes ONE pass; the
  fp32 chunk of a <= 3-channel x, and an x that takes three passes (the f16x3 split of models
  with unbounded activations), exact with their kernel rows.  h None: zero state."""
  Cx = x.shape[-1]
  kr = np.array(kernel, dtype=np.float32, copy=True)
  kr[:, :, Cx:, :] = bf16_round(kernel[:, :, Cx:, :])
  xr = x
  if Cx > 3 and x_passes == 1:
    kr[:, :, :Cx, :] = bf16_round(kernel[:, :, :Cx, :])
    xr = bf16_round(x)
  return xr, (None if h is None else bf16_round(h)), kr


# one-hot grids of the 32-cell body: (H, W) -> hot cells, one per image of the batch.
#   6 x 8: columns shifted inside a wave tile (32 % W == 0); the seam between the first and the
#          second 32-cell tile lies between (3, 7) and (4, 0)
#   5 x 7: no column shift, image rows ending inside a tile; the seam lies between (4, 3) and (4, 4)
ONE_HOT_GRIDS = {
    (6, 8): ((0, 0), (5, 7), (3, 7), (4, 0), (2, 5), (0, 7), (5, 0)),
    (5, 7): ((0, 0), (4, 6), (4, 3), (4, 4), (2, 0), (2, 6), (0, 6)),
}
HOT_X, HOT_H = (3, 17), (40, 99)       # (input channel, output channel of gate j)


def one_hot_case(H, W, ky, kx, Cx=32, C=256, tap=None):
  """One hot x cell and one hot h cell per image (image m: ONE_HOT_GRIDS[(H, W)][m]), one hot
  weight tap (ky, kx) for each; every value exact in bf16 and fp16.  `tap`: the tap the KERNEL
  holds instead of (ky, kx) -- a reference with a misplaced tap."""
  cells = ONE_HOT_GRIDS[(H, W)]
  M = len(cells)
  x = np.zeros((M, H, W, Cx), "f4")
  h = np.zeros((M, H, W, C), "f4")
  for m, (sy, sx) in enumerate(cells):
    x[m, sy, sx, HOT_X[0]] = 1.0
    h[m, sy, sx, HOT_H[0]] = 0.5
  ty, tx = (ky, kx) if tap is None else tap
  kernel = np.zeros((3, 3, Cx + C, 4 * C), "f4")
  kernel[ty, tx, HOT_X[0], 1 * C + HOT_X[1]] = 2.0         # gate j
  kernel[ty, tx, Cx + HOT_H[0], 1 * C + HOT_H[1]] = 2.0
  biases = np.zeros(4 * C, "f4")
  biases[0 * C:1 * C] = 5.0                                  # input gate ~ open
  c = np.zeros((M, H, W, C), "f4")
  return x, c, h, kernel, biases
