# coding=utf-8
"""CPU: the inputs and bars of tests/test_gpu_bwd_kernels.py hold what that file relies on --
before any GPU run.

  * every operand of every case is a fixed point of the rounding its form applies (a degenerate
    draw cannot pass), and is not trivially so where the form has a lower plane (f16x3: lo != 0);
  * each form's bar is at least 8 x the largest float32-accumulation error E32 of its cases and at
    most a quarter of the mutation floor F of every case (bwd_cases.dgrad_floor / wgrad_floor): a
    tap dropped for one image-edge row, or for the last block of cells, fails the GPU test;
  * the one-hot constructions have the nonzeros they claim, the cross-image pairs none;
  * the references agree with the project's oracle (oracle.OperandRounding, torch autograd)."""

import numpy as np
import pytest
import torch

import bwd_cases as bc
from oracle import multiverse_oracle as oracle

_DG = [(f, s) for f in bc.DGRAD_FORMS for s in bc.dgrad_shapes(f)]
_WG = [(f, s) for f in bc.WGRAD_FORMS for s in bc.wgrad_shapes(f)]


@pytest.mark.parametrize("form,shape", _DG)
def test_dgrad_operands_exact_and_bar_between_e32_and_floor(form, shape):
  M, H, W, Cx, C = shape
  x, h, G, kernel = bc.operands(form, *shape)
  for name, ok in bc.operands_are_fixed_points(form, x, h, G, kernel, "dgrad"):
    assert ok, (form, shape, name)
  if form != "bf16":        # the lower planes carry something: a kernel that dropped them fails
    s = (G * np.float32(2.0 ** bc.scale_exp(G, 13))).astype(np.float32)
    assert np.count_nonzero(s - s.astype(np.float16).astype(np.float32)) > G.size // 2
  e32 = bc.dgrad_e32(G, kernel, Cx)
  F, where = bc.dgrad_floor(G, kernel, Cx)
  bar = bc.DGRAD_BAR[form]
  print("dgrad %-6s %-22s E32 %.3g  F %.3g at %s  bar %.3g" % (form, shape, e32, F, where, bar))
  assert 8 * e32 <= bar <= F / 4, (form, shape, e32, F, bar)


@pytest.mark.parametrize("form,shape", _WG)
def test_wgrad_operands_exact_and_bar_between_e32_and_floor(form, shape):
  M, H, W, Cx, C = shape
  x, h, G, kernel = bc.operands(form, *shape)
  for name, ok in bc.operands_are_fixed_points(form, x, h, G, kernel, "wgrad"):
    assert ok, (form, shape, name)
  if bc.PLANES[form] == 2:
    s = (h * np.float32(256.0)).astype(np.float32)
    assert np.count_nonzero(s - s.astype(np.float16).astype(np.float32)) > h.size // 2
  e32 = bc.wgrad_e32(form, x, h, G, C)
  F, where = bc.wgrad_floor(np.concatenate([x, h], axis=-1), G, C)
  bar = bc.WGRAD_BAR[form]
  print("wgrad %-12s %-22s E32 %.3g  F %.3g at %s  bar %.3g" % (form, shape, e32, F, where, bar))
  assert 8 * e32 <= bar <= F / 4, (form, shape, e32, F, bar)


def test_references_agree_with_the_oracle():
  """dgrad_ref / wgrad_ref against torch autograd through oracle.conv2d_same, and
  wgrad_form_ref against oracle.OperandRounding.wgrad on operands that are NOT fixed points (the
  oracle forms the components in float64, this reference in float32 as csrc does: a float32
  rounding of U2 or U3 now and then tips the half rounding behind it to the other neighbour, 2^-11
  of ONE of the 32 products of a sum -- measured 1.7e-4 of a slice at the worst, held to 5e-4, where
  a misplaced component or tap is 1e-1)."""
  rng = np.random.default_rng(5)
  M, H, W, Cx, C = 2, 3, 16, 2, 128
  x = (rng.normal(size=(M, H, W, Cx)) * 100).astype("f4")
  h = np.tanh(rng.normal(size=(M, H, W, C))).astype("f4")
  G = (rng.normal(size=(M, H, W, 4 * C)) * 1e-3).astype("f4")
  kernel = (rng.normal(size=(3, 3, Cx + C, 4 * C)) * 0.05).astype("f4")
  t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
  a = torch.cat([t(x), t(h)], dim=-1).requires_grad_(True)
  k = t(kernel).requires_grad_(True)
  y = oracle.conv2d_same(a, k)
  da, dk = torch.autograd.grad(y, [a, k], t(G))
  assert np.abs(bc.dgrad_ref(G, kernel) - da.numpy()).max() < 1e-12
  assert np.abs(bc.wgrad_ref(np.concatenate([x, h], -1), G) - dk.numpy()).max() < 1e-12
  rnd = oracle.OperandRounding(train=True)
  for form in ("one", "one_triple"):
    want = (rnd.wgrad(t(x), t(h), t(G)) if form == "one_triple" else
            oracle._wgrad_plain(torch.cat([rnd.f16_scaled(t(x), bc.scale_exp(x, 13)),
                                           rnd.f16_scaled(t(h), 8)], dim=-1),
                                rnd.f16_scaled(t(G), bc.scale_exp(G, 13)))).numpy()
    got = bc.wgrad_form_ref(form, x, h, G)
    for (what, g), (_, w) in zip(bc.kernel_slices(got, C), bc.kernel_slices(want, C)):
      assert bc.rel_err(g, w) < (5e-4 if form == "one_triple" else 1e-12), (form, what)


@pytest.mark.parametrize("H,W", [(5, 7), (4, 8)])
def test_one_hot_dgrad_has_one_product_per_tap_and_image(H, W):
  Cx, C = 32, 256
  x, h, G, kernel, cells = bc.one_hot_dgrad(H, W, Cx, C)
  ref = bc.dgrad_ref(G, kernel)
  K = H * W
  flat = [m * K + y * W + xx for m, (y, xx) in enumerate(cells)]
  assert any(f % 32 == 31 for f in flat) and any(f % 32 == 0 and f > 0 for f in flat), flat
  assert {(0, 0), (H - 1, W - 1), (0, W - 1), (H - 1, 0)} <= set(cells), cells
  for m, (sy, sx) in enumerate(cells):
    for t in range(9):
      cx, ch, n = bc.tap_channels(t, Cx, C)
      oy, ox = sy + t // 3 - 1, sx + t % 3 - 1
      inside = 0 <= oy < H and 0 <= ox < W
      for col, w in ((cx, kernel[t // 3, t % 3, cx, n]), (Cx + ch, kernel[t // 3, t % 3, Cx + ch, n])):
        nz = np.argwhere(ref[m, :, :, col] != 0)
        assert len(nz) == (1 if inside else 0), (m, t, col, nz)
        if inside:
          assert tuple(nz[0]) == (oy, ox) and ref[m, oy, ox, col] == float(w) * float(G[m, sy, sx, n])


@pytest.mark.parametrize("H,W", [(5, 16), (6, 16)])
def test_one_hot_wgrad_pairs_and_the_pairs_that_must_give_zero(H, W):
  Cx, C = 32, 256
  x, h, G, cells = bc.one_hot_wgrad(H, W, Cx, C, extra=[(2, 5), (3, 5)])
  a = np.concatenate([x, h], axis=-1)
  ref = bc.wgrad_ref(a, G)
  K = H * W
  flat = [m * K + y * W + xx for m, (y, xx) in enumerate(cells)]
  assert any(f % 64 == 63 for f in flat) and any(f % 64 == 0 and f > 0 for f in flat), flat
  assert (2, 5) in cells and (3, 5) in cells        # either side of a row-triple boundary (H = 6)
  # every tap and both row kinds carry a product, each entry a sum of a few exact products
  for (what, r) in bc.kernel_slices(ref, C):
    assert np.count_nonzero(r) >= 1, what
  # a kernel that ran over the image edges in the flat cell order (rows of the next image below
  # the last row) computes something else: the hot pairs that straddle an image edge see to it
  flat_ref = bc.wgrad_ref(a.reshape(1, -1, W, Cx + C), G.reshape(1, -1, W, 4 * C))
  assert np.count_nonzero(flat_ref != ref) >= 8
  # pairs a flat index would join across an image edge exist in the operands
  across = 0
  for m, (sy, sx) in enumerate(cells):
    for t in range(9):
      f = m * K + sy * W + sx + (t // 3 - 1) * W + (t % 3 - 1)
      inside = 0 <= sy + t // 3 - 1 < H and 0 <= sx + t % 3 - 1 < W
      if not inside and 0 <= f < len(cells) * K:
        across += 1
        assert x.reshape(-1, Cx)[f, bc.tap_channels(t, Cx, C)[0]] != 0
  assert across >= 8
