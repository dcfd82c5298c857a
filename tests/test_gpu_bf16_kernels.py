# coding=utf-8
"""GPU: the 32-cell body of compute mode 2's gate kernel (csrc/convlstm_f16x3.h
convlstm_step_bf16_kernel, GateForm::Bf16) by the single-kernel door -- op variant 5, ONE bf16 plane
per operand, and op variant 6, the three-pass form of models with unbounded activations (x as an
f16x3 split under the tensor's own exponent, h one bf16 plane).  Every grid with H < 3 takes this
body, every launch the halo tiling cannot address, every relu / lrelu model, and MV_BF16T=0.

Reference: oracle.convlstm_step_np ON THE OPERANDS AS THE PLANES HOLD THEM (bf16_cases.
rounded_operands: the rule of tests/test_gpu_wino.py's bf16 test; for variant 6 x and the x rows of
the kernel stay unrounded), so that what is left is fp32 accumulation order.

Bars, the project's own: 2e-5 absolute on c' and h' for variant 5 (the row-triple tile's, variant
4) and for variant 6 (the f16x3 kernels'); the emitted plane == bf16(h') bit for bit; the one-hot
taps 1e-6 (every operand exact in its plane, one product per output: tests/test_gpu_wino.py).

Measured on an MI355X (printed by the tests): variant 5 max|dc'| 1.91e-6 (18 x 9), max|dh'| 1.22e-6;
variant 6 max|dc'| 1.76e-6 (5 x 7), max|dh'| 9.8e-7; zero state 1.5e-7 / 3.9e-7; the fp32 x chunk
1.43e-6; plane - bf16(h') 0 everywhere; one-hot taps 5.96e-8 in all four (grid, variant) runs.

The 16-channel x groups travel through an LDS stage in PAIRS (MV_BF16_UNITS = 2): Cx = 16 is
refused by the engine ("must be multiples of 32") and by these variants alike; that refusal is the
Cx = 16 case here."""

import numpy as np
import pytest

import bf16_cases
from bf16_cases import bf16_round
from oracle import multiverse_oracle as oracle

pytestmark = pytest.mark.gpu

BAR, ONE_HOT_BAR = 2e-5, 1e-6
VARIANTS = [(5, 1), (6, 3)]        # (op variant, x passes)


def _case(M, H, W, Cx, C, zero, seed, unbounded):
  rng = np.random.default_rng(seed)
  x = rng.normal(size=(M, H, W, Cx)).astype("f4")
  if Cx <= 3:
    x = (x * 300.0).astype("f4")            # pixel offsets of the regression encoder
  elif unbounded:
    x = (np.maximum(x, 0.0) * 6.0).astype("f4")     # relu embeddings: no bounding tanh
  else:
    x = np.tanh(x)
  lim = np.sqrt(6.0 / (9 * (Cx + C) + 9 * 4 * C)) * 3.0
  kernel = rng.uniform(-lim, lim, size=(3, 3, Cx + C, 4 * C)).astype("f4")
  if Cx <= 3:
    kernel[:, :, :Cx, :] *= 1.0 / 300.0
  elif unbounded:
    kernel[:, :, :Cx, :] *= 1.0 / 6.0
  biases = (0.1 * rng.normal(size=4 * C)).astype("f4")
  if zero:
    c = h = None
  else:
    c = rng.normal(size=(M, H, W, C)).astype("f4")
    h = np.tanh(rng.normal(size=(M, H, W, C))).astype("f4")
  return x, c, h, kernel, biases


def _where(err, name):
  M, H, W, C = err.shape
  lines = ["%s: max %.3g at %s" % (name, err.max(), np.unravel_index(err.argmax(), err.shape))]
  lines.append("  by image      " + " ".join("%.1e" % err[m].max() for m in range(M)))
  lines.append("  by row        " + " ".join("%.1e" % err[:, y].max() for y in range(H)))
  lines.append("  by column     " + " ".join("%.1e" % err[:, :, xx].max() for xx in range(W)))
  lines.append("  by ch mod 16  " + " ".join("%.1e" % err[..., k::16].max() for k in range(16)))
  lines.append("  by ch block16 " + " ".join("%.1e" % err[..., b * 16:(b + 1) * 16].max()
                                            for b in range(C // 16)))
  return "\n".join(lines)


def _reference(x, c, h, kernel, biases, x_passes):
  xr, hr, kr = bf16_cases.rounded_operands(x, h, kernel, x_passes)
  z = np.zeros(x.shape[:3] + (kernel.shape[3] // 4,), "f4")
  return oracle.convlstm_step_np(xr, z if c is None else c, z if hr is None else hr, kr, biases)


# M, H, W, Cx, C, zero state
SHAPES = [
    (2, 2, 16, 32, 256, False),   # H = 2: the tile form cannot run -- what a model takes
    (3, 5, 7, 32, 256, False),    # 105 cells: partial last 32-cell tile, no column shift, image
                                  # rows ending inside a tile
    (1, 4, 8, 32, 256, False),    # shifted columns, exactly one tile
    (2, 3, 16, 32, 256, False),   # a single row triple
    (1, 18, 9, 32, 256, False),   # the literal grid
    (2, 4, 8, 64, 256, False),    # two pairs of dense x groups
    (2, 6, 8, 32, 256, True),     # zero state: x only
    (2, 5, 7, 32, 128, False),    # C = 128
]
SMALL_X = [
    (2, 5, 7, 2, 256, False),     # the fp32 x chunk (regression encoder), ragged grid
    (1, 4, 8, 2, 256, True),      # ... alone: zero state
]


def _run(built_lib, M, H, W, Cx, C, zero, variant, x_passes):
  x, c, h, kernel, biases = _case(M, H, W, Cx, C, zero, M * 1000 + H * 10 + W + Cx + variant,
                                  unbounded=x_passes == 3)
  co, ho = _reference(x, c, h, kernel, biases, x_passes)
  cg, hg, h16 = built_lib.op_convlstm_step16(x, c, h, kernel, biases, variant=variant)
  ec, eh, ep = np.abs(cg - co), np.abs(hg - ho), np.abs(h16 - bf16_round(hg))
  print("bf16 32-cell body variant %d M=%d %dx%d Cx=%d C=%d zero=%s: max|dc| %.3g max|dh| %.3g, "
        "plane vs bf16(h') %.3g" % (variant, M, H, W, Cx, C, zero, ec.max(), eh.max(), ep.max()))
  assert ec.max() < BAR, _where(ec, "c'")
  assert eh.max() < BAR, _where(eh, "h'")
  assert ep.max() == 0, _where(ep, "plane")      # the emitted plane IS h' rounded to bf16


@pytest.mark.parametrize("variant,x_passes", VARIANTS)
@pytest.mark.parametrize("M,H,W,Cx,C,zero", SHAPES)
def test_bf16_body_vs_oracle_on_rounded_operands(built_lib, M, H, W, Cx, C, zero, variant,
                                                 x_passes):
  _run(built_lib, M, H, W, Cx, C, zero, variant, x_passes)


@pytest.mark.parametrize("M,H,W,Cx,C,zero", SMALL_X)
def test_bf16_body_fp32_x_chunk(built_lib, M, H, W, Cx, C, zero):
  """Cx <= 3: the x part is the fp32 chunk (exact operands), h one bf16 plane.  There is no
  three-pass form of it (gate_plan.h bf16_x_passes): variant 6 refuses."""
  _run(built_lib, M, H, W, Cx, C, zero, 5, 1)
  x, c, h, kernel, biases = _case(M, H, W, Cx, C, zero, 1, False)
  with pytest.raises(built_lib.MvError, match="dense x"):
    built_lib.op_convlstm_step16(x, c, h, kernel, biases, variant=6)


@pytest.mark.parametrize("variant,x_passes", VARIANTS)
def test_bf16_body_refuses_an_odd_number_of_x_groups(built_lib, variant, x_passes):
  """Cx = 16: one 16-channel group does not fill an LDS stage of two row units; the engine
  refuses such a model in this mode and so does the op -- before any launch."""
  x, c, h, kernel, biases = _case(1, 4, 8, 16, 256, False, 16, False)
  with pytest.raises(built_lib.MvError, match="multiples of 32"):
    built_lib.op_convlstm_step16(x, c, h, kernel, biases, variant=variant)


@pytest.mark.parametrize("variant,x_passes", VARIANTS)
@pytest.mark.parametrize("H,W", sorted(bf16_cases.ONE_HOT_GRIDS))
def test_bf16_body_transpose_detecting(built_lib, H, W, variant, x_passes):
  """One hot x cell, one hot h cell and one hot weight tap each (tests/test_gpu_kernels.py
  test_convlstm_step_transpose_detecting), for every (ky, kx): the hot cells in the first and
  last row, the first and last column and on both sides of a 32-cell tile seam, one per image."""
  worst = 0.0
  for ky in range(3):
    for kx in range(3):
      x, c, h, kernel, biases = bf16_cases.one_hot_case(H, W, ky, kx)
      co, ho = oracle.convlstm_step_np(x, c, h, kernel, biases)      # exact in every plane
      cg, hg, h16 = built_lib.op_convlstm_step16(x, c, h, kernel, biases, variant=variant)
      for m, (sy, sx) in enumerate(bf16_cases.ONE_HOT_GRIDS[(H, W)]):
        oy, ox = sy - (ky - 1), sx - (kx - 1)      # out(y,x) sees in(y+ky-1, x+kx-1)
        if 0 <= oy < H and 0 <= ox < W:
          assert abs(co[m, oy, ox, bf16_cases.HOT_X[1]]) > 0.5
          assert abs(co[m, oy, ox, bf16_cases.HOT_H[1]]) > 0.5
      ec, eh = np.abs(cg - co), np.abs(hg - ho)
      worst = max(worst, float(ec.max()), float(eh.max()))
      assert ec.max() < ONE_HOT_BAR, "tap (%d,%d)\n%s" % (ky, kx, _where(ec, "c'"))
      assert eh.max() < ONE_HOT_BAR, "tap (%d,%d)\n%s" % (ky, kx, _where(eh, "h'"))
      assert np.abs(h16 - bf16_round(hg)).max() == 0
  print("bf16 32-cell body variant %d one-hot %dx%d: worst %.3g" % (variant, H, W, worst))
