# coding=utf-8
"""GPU: the matrix-pipe backward of the gate convolution, ONE kernel form at a time, through the
single-kernel doors mv_op_convlstm_bwd16 and mv_op_lstm_gate_bwd (csrc/engine_ops.h) -- the
backward's counterpart of tests/test_gpu_bf16_kernels.py, test_gpu_wino.py and test_gpu_f16x3.py.

  dgrad   f16x3 direct (split-K as planned, DPP column shift where 32 % W == 0), f16x3 Winograd
          F(2,3), bf16 one plane whole-K
  wgrad   f16x3 direct, f16x3 row-triple, one fp16 plane direct, one plane row-triple; narrow and
          wide tile as csrc/gate_plan.h plan_wgrad picks them -- asserted (test 5)
  gate    lstm_gate_bwd_kernel, lstm_gate_bwd4_kernel, lstm_gate_bwd4_plane_kernel

G is an INPUT of the door and every operand is a fixed point of the rounding its form applies
(tests/bwd_cases.py; tests/test_bwd_cases_host.py asserts it on the CPU): nothing rounds on the
way in, no element can flip between two references, and what is measured is the kernel's fp32
accumulation -- and its indexing.

1 one-hot, every tap: nine hot gate columns in one hot G cell per image, one weight (dgrad) or one
  hot operand cell (wgrad) per tap; hot cells in the corners, either side of a 32-cell (dgrad) /
  64-cell (wgrad) seam, either side of a row-triple boundary; wgrad pairs that a flat cell index
  would join across an image edge must give zero.  1e-6 absolute; zero where the reference is zero.
2 random fixed-point operands against float64: max|d| / max|ref| per output tensor, per tap and
  x rows / h rows for d kernel.  The bar is one constant per form, NOT taken from the kernel:
  between 8 x E32 (float32 accumulation of the same contraction on the CPU) and F / 4 (F: what the
  reference loses when ONE tap skips one image-edge row or the last block of cells).
3 the exponents the device computed; elements 2^-16 .. 2^-40 of the maximum (normal halves down
  to 2^-26, the gradual-underflow band of the planes below, the flush at the end) against the
  restated plane rule; a maximum that is a power of two.
4 the gate backward's three forms: float64 formula to 2e-4 (the bar of tests/test_gpu_train.py
  test_convlstm_backward_op), bitwise equal among themselves, plane == bf16(G) bit for bit, gmax.
5 which tile and how many splits ran, against values written out by hand.

Figures (E32 and F from tests/test_bwd_cases_host.py on the CPU; the MI355X column is what these
tests print):

  form               E32 (largest)   F (smallest)   bar      MI355X (largest)
  dgrad f16x3        4.7e-7          0.17           4e-6     9.0e-7
  dgrad wino         4.2e-7          0.21           4e-6     8.6e-7
  dgrad bf16         0               0.15           1e-6     0
  wgrad f16x3        5.4e-7          0.30           5e-6     1.6e-7
  wgrad f16x3 triple 1.8e-6          0.20           2e-5     6.2e-7
  wgrad one          2.6e-7          0.26           2.5e-6   5.7e-8
  wgrad one triple   6.6e-7          0.21           1e-5     3.3e-7

(7-bit operands -- bf16 dgrad, one-plane row-triple -- make every partial sum an integer below
2^24 quanta: fp32 accumulation is exact, E32 is 0 and the bar 8 x 2^-23.)  One-hot: 0 everywhere
but the f16x3 row-triple wgrad, 2e-8.  Gate backward: 7.8e-8 (G), 8.0e-8 (d c) from float64.
The bf16 stage-count refusal of the dgrad cannot be reached with C % 128 == 0 (3 C / 4 stages are
even) and has no case here."""

import numpy as np
import pytest

import bwd_cases as bc
from bf16_cases import bf16_round

pytestmark = pytest.mark.gpu

_RUNS = {}          # (kind, form, shape) -> the door's result, shared by tests 2, 3 and 5


def _run(lib, kind, form, shape, outputs=False):
  """The door's result for a case of bwd_cases.operands, run once.  `outputs`: the caller
  compares the output tensors -- and drops them when done (_done: a d kernel is 10 MB)."""
  key = (kind, form, shape)
  x, h, G, kernel = bc.operands(form, *shape)
  if key not in _RUNS or (outputs and _RUNS[key].get("dropped")):
    _RUNS[key] = lib.op_convlstm_bwd16(x, h, G, kernel, **{kind: form})
  return _RUNS[key], (x, h, G, kernel)


def _done(r):
  r.update(dx=None, dh=None, dkernel=None, dropped=True)


def _check_cells(got, ref, bar, name, absolute=False):
  err = np.abs(got.astype(np.float64) - ref)
  den = 1.0 if absolute else np.abs(ref).max()
  print("    %s" % bc.where_cells(err / den, name).replace("\n", "\n    "))
  assert np.isfinite(got).all(), name
  assert err.max() / den < bar, bc.where_cells(err / den, name)
  return err.max() / den


def _check_kernel(got, ref, C, bar, name):
  """per tap and x rows / h rows: max|d| / max|ref slice|"""
  Cx = ref.shape[2] - C
  assert np.isfinite(got).all(), name
  rel = np.zeros(ref.shape)
  for (what, g), (_, r), (_, e) in zip(bc.kernel_slices(got, C), bc.kernel_slices(ref, C),
                                       bc.kernel_slices(rel, C)):
    assert np.abs(r).max() > 0, what
    e[...] = np.abs(g.astype(np.float64) - r) / np.abs(r).max()
  print("    %s" % bc.where_kernel(rel, Cx, name).replace("\n", "\n    "))
  assert rel.max() < bar, bc.where_kernel(rel, Cx, name)
  return rel.max()


# ---------------------------------------------------------------- 1 one-hot, every tap
@pytest.mark.parametrize("form,H,W", [("f16x3", 5, 7), ("f16x3", 4, 8), ("bf16", 5, 7),
                                      ("bf16", 4, 8), ("wino", 4, 8), ("wino", 3, 16)])
def test_dgrad_one_hot_every_tap(built_lib, form, H, W):
  """(5, 7): no column shift, image rows ending inside a 32-cell tile, seams inside images;
  (4, 8): shifted, an image is exactly a tile (the corners are the seam cells); (3, 16): an odd
  last row pair of F(2,3)."""
  Cx, C = 32, 256
  x, h, G, kernel, cells = bc.one_hot_dgrad(H, W, Cx, C)
  for name, ok in bc.operands_are_fixed_points(form, x, h, G, kernel, "dgrad"):
    assert ok, name
  ref = bc.dgrad_ref(G, kernel)
  r = built_lib.op_convlstm_bwd16(x, h, G, kernel, dgrad=form)
  print("dgrad %s one-hot %dx%d, hot cells %s" % (form, H, W, cells))
  for name, got, want in (("dx", r["dx"], ref[..., :Cx]), ("dh", r["dh"], ref[..., Cx:])):
    assert np.count_nonzero(want) > 9 * len(cells) // 2
    _check_cells(got, want, bc.ONE_HOT_BAR, name, absolute=True)
    assert (got[want == 0] == 0).all(), "%s: %d nonzeros where the reference has none, first at %s" % (
        name, np.count_nonzero(got[want == 0]), np.argwhere((want == 0) & (got != 0))[0])


@pytest.mark.parametrize("form", bc.WGRAD_FORMS)
def test_wgrad_one_hot_every_tap(built_lib, form):
  """direct forms on 5 x 16 (80 cells an image: 64-cell seams inside images), row-triple forms on
  6 x 16 with hot cells in rows 2 and 3 (either side of a triple boundary)."""
  Cx, C = 32, 256
  H, W = (6, 16) if bc.TRIPLE[form] else (5, 16)
  x, h, G, cells = bc.one_hot_wgrad(H, W, Cx, C, extra=[(2, 5), (3, 5)])
  ref = bc.wgrad_form_ref(form, x, h, G)
  if not bc.TRIPLE[form]:       # every operand exact: the plain contraction
    kernel = np.zeros((3, 3, Cx + C, 4 * C), "f4")
    for name, ok in bc.operands_are_fixed_points(form, x, h, G, kernel, "wgrad"):
      assert ok, name
    assert np.array_equal(ref, bc.wgrad_ref(np.concatenate([x, h], -1), G))
  r = built_lib.op_convlstm_bwd16(x, h, G, np.zeros((3, 3, Cx + C, 4 * C), "f4"), wgrad=form)
  got = r["dkernel"]
  err = np.abs(got.astype(np.float64) - ref)
  print("wgrad %s one-hot %dx%d, hot cells %s\n    %s" % (
      form, H, W, cells, bc.where_kernel(err, Cx, "dkernel").replace("\n", "\n    ")))
  assert np.count_nonzero(ref) >= 18
  assert err.max() < bc.ONE_HOT_BAR, bc.where_kernel(err, Cx, "dkernel")
  # exactly zero where no product reaches (bwd_cases.wgrad_structural_zeros: in the row-triple
  # forms the other zeros are cancellations of partial taps, held by the bar above)
  none = bc.wgrad_structural_zeros(form, x, h, G)
  assert none.sum() > none.size // 2 and not ref[none].any()
  assert (got[none] == 0).all(), "%d nonzeros where no product reaches, first at %s" % (
      np.count_nonzero(got[none]), np.argwhere(none & (got != 0))[0])


# ---------------------------------------------------------------- 2 random fixed-point operands
@pytest.mark.parametrize("form,shape", [(f, s) for f in bc.DGRAD_FORMS for s in bc.dgrad_shapes(f)])
def test_dgrad_vs_float64_on_exact_operands(built_lib, form, shape):
  M, H, W, Cx, C = shape
  r, (x, h, G, kernel) = _run(built_lib, "dgrad", form, shape, outputs=True)
  for name, ok in bc.operands_are_fixed_points(form, x, h, G, kernel, "dgrad"):
    assert ok, name
  ref = bc.dgrad_ref(G, kernel)
  print("dgrad %s M=%d %dx%d Cx=%d C=%d  slices %s shift %s" % (
      (form,) + shape + (r["dgrad_slices"], r["shift"])))
  ex = _check_cells(r["dx"], ref[..., :Cx], bc.DGRAD_BAR[form], "dx")
  eh = _check_cells(r["dh"], ref[..., Cx:], bc.DGRAD_BAR[form], "dh")
  print("dgrad %s %s: dx %.3g dh %.3g (bar %.3g)" % (form, shape, ex, eh, bc.DGRAD_BAR[form]))
  _done(r)


@pytest.mark.parametrize("form,shape", [(f, s) for f in bc.WGRAD_FORMS for s in bc.wgrad_shapes(f)])
def test_wgrad_vs_float64_on_exact_operands(built_lib, form, shape):
  M, H, W, Cx, C = shape
  r, (x, h, G, kernel) = _run(built_lib, "wgrad", form, shape, outputs=True)
  for name, ok in bc.operands_are_fixed_points(form, x, h, G, kernel, "wgrad"):
    assert ok, name
  ref = bc.wgrad_form_ref(form, x, h, G)
  print("wgrad %s M=%d %dx%d Cx=%d C=%d  wide %s nsplit %d / %d" % (
      (form,) + shape + (r["wide"], r["nsplit"], r["nsplit_x"])))
  e = _check_kernel(r["dkernel"], ref, C, bc.WGRAD_BAR[form], "dkernel")
  print("wgrad %s %s: worst slice %.3g (bar %.3g)" % (form, shape, e, bc.WGRAD_BAR[form]))
  _done(r)


# ---------------------------------------------------------------- 3 exponents and underflow
@pytest.mark.parametrize("form,shape", [(f, s) for f in bc.WGRAD_FORMS for s in bc.wgrad_shapes(f)])
def test_wgrad_exponents(built_lib, form, shape):
  r, (x, h, G, kernel) = _run(built_lib, "wgrad", form, shape)
  want = (13 - bc.ilogb(np.abs(G).max()), 8,
          (10 if bc.TRIPLE[form] else 13) - bc.ilogb(np.abs(x).max()))
  assert r["exps"] == want, (r["exps"], want)


@pytest.mark.parametrize("form", ["f16x3", "wino"])
def test_dgrad_exponent(built_lib, form):
  shape = bc.dgrad_shapes(form)[2]
  r, (x, h, G, kernel) = _run(built_lib, "dgrad", form, shape)
  assert r["exps"][0] == 13 - bc.ilogb(np.abs(G).max()), r["exps"]


_UNDERFLOW_SHAPE = {False: (2, 4, 16, 32, 256), True: (2, 3, 16, 32, 256)}


_SMALL = list(range(16, 41, 2))       # 2^-16 .. 2^-40 of the maximum


@pytest.mark.parametrize("form", bc.WGRAD_FORMS)
def test_wgrad_underflow_band(built_lib, form):
  """Thirteen elements of G and of x at 1.25 x 2^-16, 2^-18 .. 2^-40 of the tensor's maximum, each
  ALONE in a gate column (5 + 8 i) / an x channel (i) of its own.  The maximum is scaled into
  [2^13, 2^14) (x in the row-triple form [2^10, 2^11)), so 2^-16 .. 2^-26 are still normal halves,
  2^-28 .. 2^-38 lie in the band where a half keeps fewer and fewer bits, 2^-40 is zero (one
  plane; with two the lower plane picks up what the upper drops, until it underflows too).  The
  reference holds what the planes hold (bwd_cases.planes: the rule of oracle.OperandRounding.
  f16_scaled).  Whole slices at the bar of test 2 -- and every column / row that ONE small element
  feeds, relative to ITS maximum (1e-12 of the tensor's): exactly zero where the planes hold zero;
  one plane: at the same bar (measured on an MI355X: 0 in every column, down to the flush: the
  MFMA takes subnormal halves and the restated rule is the kernels');  two planes: within 2^-11,
  what the lower planes carry of one product at the most.  Measured for two planes: 0 down to
  2^-32 of the maximum, then 7.6e-7 / 2.3e-6 at 2^-34 and 5.3e-6 at 2^-36 (direct); 1e-7 .. 7e-7
  down to 2^-26, 1.4e-6 at 2^-28, 2.5e-5 at 2^-32 (row-triple) -- a roughly constant ABSOLUTE
  distance (2^-27 / 2^-23 of the accumulator's scaled unit) that neither the planes' rule nor the
  missing lo lo product of the f16x3 split (tried as a reference: no change) accounts for.  Its
  cause is not found; it is 1e-17 of the tensor's maximum and far below every bar here, so the
  column check of the two-plane forms asserts only the format's own bound."""
  shape = _UNDERFLOW_SHAPE[bc.TRIPLE[form]]
  M, H, W, Cx, C = shape
  x, h, G, kernel = bc.operands(form, *shape, seed=7)
  gmax, xmax = np.abs(G).max(), np.abs(x).max()
  cols = [5 + 8 * i for i in range(len(_SMALL))]
  G[..., cols] = 0.0
  x[..., :len(_SMALL)] = 0.0
  for i, k in enumerate(_SMALL):
    m, y, xx = i % M, (i * 5 + 1) % H, (i * 7 + 2) % W
    G[m, y, xx, cols[i]] = np.float32(1.25 * gmax * 2.0 ** -k) * (-1) ** i
    x[m, (y + 1) % H, xx, i] = np.float32(1.25 * xmax * 2.0 ** -k) * (-1) ** i
  assert np.abs(G).max() == gmax and np.abs(x).max() == xmax
  ref = bc.wgrad_form_ref(form, x, h, G)
  r = built_lib.op_convlstm_bwd16(x, h, G, kernel, wgrad=form)
  got = r["dkernel"].astype(np.float64)
  assert r["exps"] == bc.wgrad_exps(form, x, G)
  bar = bc.WGRAD_BAR[form]
  print("wgrad %s underflow band %s" % (form, shape))
  _check_kernel(r["dkernel"], ref, C, bar, "dkernel")
  zero_cols = 0
  for i, k in enumerate(_SMALL):
    for name, sl in (("gate column of G 2^-%d" % k, np.s_[:, :, Cx:, cols[i]]),
                     ("x channel of x 2^-%d" % k, np.s_[:, :, i, :])):
      g, w = got[sl], ref[sl]
      mx = np.abs(w).max()
      e = np.abs(g - w).max() / mx if mx > 0 else float(np.abs(g).max())
      print("    %-28s max|ref| %.3g  gpu vs the plane rule %.3g" % (name, mx, e))
      if mx == 0:
        zero_cols += 1
        assert not g.any(), name
      else:
        assert e < (bar if bc.PLANES[form] == 1 else 2.0 ** -11), (name, e)
  if bc.PLANES[form] == 1:      # the flush is reached
    assert zero_cols >= 1


@pytest.mark.parametrize("kind,form", [("dgrad", "f16x3"), ("wgrad", "f16x3"),
                                       ("wgrad", "one_triple")])
def test_maximum_an_exact_power_of_two(built_lib, kind, form):
  """max|G| = 2^-7 and max|x| = 2^-1 exactly: ilogb's boundary (one below would scale the
  maximum to 2^14, outside the planes' range)."""
  shape = (2, 3, 16, 32, 256)
  M, H, W, Cx, C = shape
  x, h, G, kernel = bc.operands(form, *shape, seed=3)
  G, x = G * np.float32(0.5), x * np.float32(0.5)
  G[1, 2, 3, 4], x[0, 1, 2, 3] = -2.0 ** -7, 2.0 ** -1
  assert np.abs(G).max() == 2.0 ** -7 and np.abs(x).max() == 2.0 ** -1
  for name, ok in bc.operands_are_fixed_points(form, x, h, G, kernel, kind):
    assert ok, name
  if kind == "dgrad":
    r = built_lib.op_convlstm_bwd16(x, h, G, kernel, dgrad=form)
    assert r["exps"][0] == 20
    ref = bc.dgrad_ref(G, kernel)
    _check_cells(r["dx"], ref[..., :Cx], bc.DGRAD_BAR[form], "dx")
    _check_cells(r["dh"], ref[..., Cx:], bc.DGRAD_BAR[form], "dh")
  else:
    r = built_lib.op_convlstm_bwd16(x, h, G, kernel, wgrad=form)
    assert r["exps"] == (20, 8, 11 if bc.TRIPLE[form] else 14)
    _check_kernel(r["dkernel"], bc.wgrad_form_ref(form, x, h, G), C, bc.WGRAD_BAR[form], "dkernel")


# ---------------------------------------------------------------- refusals
def test_refusals_name_the_planners_condition(built_lib):
  def run(shape, **kw):
    x, h, G, kernel = bc.operands("bf16", *shape)
    return built_lib.op_convlstm_bwd16(x, h, G, kernel, **kw)
  with pytest.raises(built_lib.MvError, match="wino_dgrad_geometry_ok"):
    run((2, 5, 7, 32, 256), dgrad="wino")
  for form in ("f16x3_triple", "one_triple"):
    with pytest.raises(built_lib.MvError, match="wgrad16_wino3_ok"):
      run((2, 4, 16, 32, 256), wgrad=form)
  for form in bc.WGRAD_FORMS:
    with pytest.raises(built_lib.MvError, match="wgrad16_ok"):
      run((2, 6, 8, 32, 256), wgrad=form)


# ---------------------------------------------------------------- 4 the gate backward
def _gate_ref(gates, c_prev, c_new, dh, dc):
  """the comment of csrc/train_kernels.h lstm_gate_bwd_kernel, in float64"""
  g = gates.astype(np.float64)
  si, tj, sf, so = g[:, 0], g[:, 1], g[:, 2], g[:, 3]
  tc = np.tanh(c_new.astype(np.float64))
  dcv = dc + dh.astype(np.float64) * so * (1 - tc * tc)
  cp = 0.0 if c_prev is None else c_prev.astype(np.float64)
  G = np.stack([dcv * tj * (si * (1 - si)), dcv * si * (1 - tj * tj), dcv * cp * (sf * (1 - sf)),
                dh * tc * (so * (1 - so))], axis=1)
  return G.reshape(len(g), -1), dcv * sf


@pytest.mark.parametrize("cells,C", [(105, 128), (105, 256), (64, 128), (64, 256)])
def test_gate_backward_three_forms(built_lib, cells, C):
  """105 cells: a partial last 32-cell group of the plane form, with C = 128 a half-full last
  block of the scalar form (whose block-wide maximum read LDS slots of waves that had left)."""
  rng = np.random.default_rng(cells + C)
  sig = lambda a: 1.0 / (1.0 + np.exp(-a))
  pre = rng.normal(size=(cells, 4, C))
  gates = np.stack([sig(pre[:, 0]), np.tanh(pre[:, 1]), sig(pre[:, 2]), sig(pre[:, 3])],
                   axis=1).astype("f4")
  c_prev = rng.normal(0, 0.5, (cells, C)).astype("f4")
  c_new = rng.normal(0, 0.7, (cells, C)).astype("f4")
  dh = rng.normal(size=(cells, C)).astype("f4")
  dc = rng.normal(size=(cells, C)).astype("f4")
  Gr, dcr = _gate_ref(gates, c_prev, c_new, dh, dc)
  out = [built_lib.op_lstm_gate_bwd(gates, c_prev, c_new, dh, dc, form) for form in (0, 1, 2)]
  for form, (G, dco, bits, plane) in enumerate(out):
    eg = np.abs(G - Gr).max() / np.abs(Gr).max()
    ed = np.abs(dco - dcr).max() / np.abs(dcr).max()
    print("gate bwd form %d cells=%d C=%d: G %.3g dc %.3g gmax bits %#x" % (form, cells, C, eg,
                                                                           ed, bits))
    assert eg < 2e-4 and ed < 2e-4, (form, eg, ed)
    assert np.array_equal(G.view(np.uint32), out[0][0].view(np.uint32)), form
    assert np.array_equal(dco.view(np.uint32), out[0][1].view(np.uint32)), form
    assert bits == int(np.abs(G).max().view(np.int32)), (form, bits)
  G2, plane = out[2][0], out[2][3]
  bad = np.argwhere(plane.view(np.uint32) != bf16_round(G2).view(np.uint32))
  assert len(bad) == 0, "plane != bf16(G) at %d places, first (cell, column) %s" % (len(bad), bad[0])
  # zero previous cell state (the first step of a chain)
  Gz, dcz, bz, _ = built_lib.op_lstm_gate_bwd(gates, None, c_new, dh, dc, 1)
  Gzr, dczr = _gate_ref(gates, None, c_new, dh, dc)
  assert np.abs(Gz - Gzr).max() / np.abs(Gzr).max() < 2e-4 and not Gz[:, 2 * C:3 * C].any()


# ---------------------------------------------------------------- 5 forms that ran
@pytest.mark.parametrize("form,shape", [(f, s) for f in bc.WGRAD_FORMS for s in bc.wgrad_shapes(f)])
def test_wgrad_tile_and_splits_that_ran(built_lib, form, shape):
  r, _ = _run(built_lib, "wgrad", form, shape)
  want = bc.wgrad_form_expected(form, *shape)
  got = {k: r[k] for k in want}
  assert got == want, (form, shape, got, want)
  assert r["transpose3"]


@pytest.mark.parametrize("form,shape", [(f, s) for f in bc.DGRAD_FORMS for s in bc.dgrad_shapes(f)])
def test_dgrad_slices_and_shift_that_ran(built_lib, form, shape):
  r, _ = _run(built_lib, "dgrad", form, shape)
  want = bc.dgrad_form_expected(form, *shape)
  got = {k: r[k] for k in want}
  assert got == want, (form, shape, got, want)
