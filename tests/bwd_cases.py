# coding=utf-8
"""Operands, references and bars of the backward gate kernels' single-kernel tests
(tests/test_gpu_bwd_kernels.py) and of their CPU-side checks (tests/test_bwd_cases_host.py).

Operands are FIXED-POINT: small integers times a power of two, so coarse that every plane a form
builds from them holds the value itself (`operands_are_fixed_points` applies the form's rounding,
restated here in numpy from csrc/, and asks for equality).  A kernel handed such operands rounds
nothing on the way in; what is left is its fp32 accumulation.

References are float64 numpy: `dgrad_ref`, `wgrad_ref` (the plain contractions), `wgrad_triple_ref`
(the row-triple form: components in float32 in the order csrc/convlstm_wgrad_f16x3.h states --
wino3_transpose_a3_kernel, wino3_transpose_g_kernel --, rounded into planes, accumulated in
float64, combined as wgrad_wino3_reduce_kernel combines)."""

import numpy as np

from bf16_cases import bf16_round

# ------------------------------------------------------------------ forms
DGRAD_FORMS = ("f16x3", "wino", "bf16")
WGRAD_FORMS = ("f16x3", "f16x3_triple", "one", "one_triple")
# significant bits of the integers an operand is drawn from (sign apart)
#   bf16 dgrad         bf16 holds 8: 7
#   one plane direct   half holds 11: 10
#   one plane triple   |V| <= 6 |a| adds three bits, U1 two: 7
#   f16x3              hi + lo hold 22 (11 + 11): 18, so that V (21 bits) and U1, U3 (20, 21) still
#                      fit, the lower plane is NOT zero, and fp32 accumulation does round
BITS = {"bf16": 7, "one": 10, "one_triple": 7, "f16x3": 18, "wino": 18, "f16x3_triple": 18}
PLANES = {"one": 1, "one_triple": 1, "f16x3": 2, "f16x3_triple": 2}
TRIPLE = {"one": False, "one_triple": True, "f16x3": False, "f16x3_triple": True}

# M, H, W, Cx, C
DGRAD_SHAPES = [
    (3, 5, 7, 32, 256),      # 105 cells, no column shift, image rows ending inside a tile
    (1, 4, 8, 32, 256),      # shifted, exactly one tile
    (2, 2, 16, 32, 256),
    (1, 18, 9, 32, 256),
    (2, 4, 8, 64, 256),
    (2, 5, 7, 2, 256),       # the d x of the fp32 x chunk: two columns padded to four
    (2, 5, 7, 32, 128),
]
WINO_DGRAD_SHAPES = [
    (2, 2, 16, 32, 256),     # one row pair
    (2, 3, 16, 32, 256),     # odd last pair
    (1, 4, 8, 32, 256),
    (1, 5, 32, 32, 256),
    (2, 4, 8, 2, 256),
]
WGRAD_DIRECT_SHAPES = [
    (1, 5, 16, 32, 256),     # 80 cells: one full and one partial 64-cell block, wide tile
    (2, 2, 16, 32, 256),
    (2, 4, 16, 32, 128),     # narrow tile
    (2, 4, 16, 2, 256),
    (2, 4, 16, 64, 256),
]
WGRAD_TRIPLE_SHAPES = [
    (2, 3, 16, 32, 256),     # 32 triple-cells, under one block
    (2, 6, 32, 32, 256),     # two triples per image
    (3, 3, 16, 128 // 4, 128),     # narrow
    (2, 6, 16, 2, 256),
]


def dgrad_shapes(form):
  return WINO_DGRAD_SHAPES if form == "wino" else DGRAD_SHAPES


def wgrad_shapes(form):
  return WGRAD_TRIPLE_SHAPES if TRIPLE[form] else WGRAD_DIRECT_SHAPES


# Which tile and how many splits run: written out by hand from csrc/gate_plan.h plan_wgrad,
# csrc/convlstm_wgrad.h wgrad_plan and csrc/convlstm_wgrad_f16x3.h (NOT obtained from the planner).
#   wide     W % 16 == 0 and C % 256 == 0 (wgrad16_wide_ok); wide_x stays off (MV_WGRAD_WIDE_X)
#   nsplit   narrow: the fp32 plan's count; wide, block map 0: 7 where the plan has at least 7
#            (14 / 21 need 896 / 1344 k-steps of 16 cells: none here)
#   nsplit_x row-triple: 12 only with at least 12 * 32 k-steps, else nsplit; direct: nsplit
# dgrad: the f16x3 direct form splits K in four where 9 (4C / 16) / 3 stages divide by 8 (C = 256:
# 192, C = 128: 96: both), bf16 runs whole-K (reported as 0: no partial sums); F(2,3): d h in
# 8 / (C / 64) slices, d x in eight.  DPP column shift where 32 % W == 0.
#   the fp32 plan (W % 4 == 0): 3072 / (9 (ceil(Cx / 64) + C / 64) (C / 64)) rounded up to a
#   multiple of 8 -- C = 256: 3072 / 180 = 17 -> 24; C = 128: 3072 / 54 = 56 -> 56
#   so: C = 256 wide, 7 splits; C = 128 narrow, 56 splits; nsplit_x = nsplit (7 < 12; 3 k-steps)
def wgrad_form_expected(form, M, H, W, Cx, C):
  return {256: dict(wide=True, wide_x=False, nsplit=7, nsplit_x=7),
          128: dict(wide=False, wide_x=False, nsplit=56, nsplit_x=56)}[C]


def dgrad_form_expected(form, M, H, W, Cx, C):
  if form == "wino":
    return dict(dgrad_slices=(max(1, 8 // (C // 64)), 8), shift=False)
  return dict(dgrad_slices=(0, 0) if form == "bf16" else (4, 4), shift=32 % W == 0)


# ------------------------------------------------------------------ operands
def draw(rng, shape, bits, top):
  """integers of `bits` bits (and a sign) times 2^(top - bits): |v| < 2^top"""
  k = rng.integers(-(2 ** bits - 1), 2 ** bits, size=shape)
  return (k.astype(np.float64) * 2.0 ** (top - bits)).astype(np.float32)


def operands(form, M, H, W, Cx, C, seed=0):
  """x, h, G, kernel on the form's grid.  |h| < 1, |G| < 2^-6, |w| < 2^-4, a dense |x| < 1, the
  pixel offsets of a <= 3-channel x below 512."""
  rng = np.random.default_rng(1000 * M + 100 * H + 10 * W + Cx + C + seed)
  b = BITS[form]
  x = draw(rng, (M, H, W, Cx), b, 9 if Cx <= 3 else 0)
  h = draw(rng, (M, H, W, C), b, 0)
  G = draw(rng, (M, H, W, 4 * C), b, -6)
  kernel = draw(rng, (3, 3, Cx + C, 4 * C), b, -4)
  return x, h, G, kernel


def ilogb(v):
  return int(np.frexp(float(v))[1]) - 1


def scale_exp(t, top):
  """csrc/convlstm_wgrad_f16x3.h chain_exp_kernel, csrc/convlstm_f16x3.h split_planes_dyn_kernel"""
  mx = float(np.abs(t).max())
  return int(min(100, max(-100, top - ilogb(mx)))) if mx > 0 else 0


def planes(v, e, npl, part="sum"):
  """The value the planes of v hold under the scale 2^e: `const float s = v * sc2e; h0 =
  (_Float16)s;` and, with two planes, `(_Float16)(s - (float)h0)` -- float64 of (hi [+ lo]) / 2^e.
  numpy's float16 cast is the conversion: nearest even, gradual underflow.  part "lo": the lower
  plane alone (zero with one plane)."""
  s = (np.asarray(v, np.float32) * np.float32(2.0 ** e)).astype(np.float32)
  hi = s.astype(np.float16)
  lo = (s - hi.astype(np.float32)).astype(np.float16).astype(np.float64) * (npl == 2)
  if part == "lo":
    return lo * 2.0 ** -e
  return (hi.astype(np.float64) + lo) * 2.0 ** -e


def wgrad_exps(form, x, G):
  return scale_exp(G, 13), 8, scale_exp(x, 10 if TRIPLE[form] else 13)


def _rows5(t):
  """image rows 3t - 1 .. 3t + 3 of every triple, zero outside the image: five [M, H/3, W, c]"""
  H = t.shape[1]
  p = np.pad(t, ((0, 0), (1, 1), (0, 0), (0, 0)))
  return [p[:, i:i + H - 2:3] for i in range(5)]


def triple_components(x, h, G, exps, npl, part="sum"):
  """V0..V4 of [x | h] and U0..U4 of G as the planes hold them (float64), and the same before the
  rounding into planes (float32): csrc/convlstm_wgrad_f16x3.h wino3_transpose_a3_kernel and
  wino3_transpose_g_kernel, statement by statement in float32."""
  eg, eh, ex = exps
  f2, f4 = np.float32(2.0), np.float32(4.0)

  def comps_a(t):
    d = _rows5(np.asarray(t, np.float32))
    v3, d32 = d[3] - d[1], d[3] - d[2]
    return [f2 * (d[0] - d[2]) + v3, d32 - f2 * d[1], f2 * (d[1] - d[2]) + d32, v3,
            f2 * v3 + (d[2] - d[4])]

  g = np.asarray(G, np.float32)
  g0, g1, g2 = g[:, 0::3], g[:, 1::3], g[:, 2::3]
  sixth = np.float32(1.0) / np.float32(6.0)
  U32 = [np.float32(0.5) * g0, np.float32(-0.5) * ((g0 + g1) + g2), ((g1 - g0) - g2) * sixth,
         ((g0 + f2 * g1) + f4 * g2) * sixth, -g2]
  Vx32, Vh32 = comps_a(x), comps_a(h)
  V = [np.concatenate([planes(vx, ex, npl, part), planes(vh, eh, npl, part)], axis=-1)
       for vx, vh in zip(Vx32, Vh32)]
  U = [planes(u, eg, npl, part) for u in U32]
  return V, U, (Vx32, Vh32, U32)


def operands_are_fixed_points(form, x, h, G, kernel, kind):
  """kind "dgrad" / "wgrad": list of (name, bool) -- is every operand the value its planes hold?"""
  out = []
  if kind == "dgrad":
    if form == "bf16":
      out += [("G bf16", np.array_equal(bf16_round(G), G)),
              ("kernel bf16", np.array_equal(bf16_round(kernel), kernel))]
    else:            # split_planes_dyn_kernel, pack_f16x3_dgrad_kernel (kF16Scale = 2^8)
      out += [("G hi+lo", np.array_equal(planes(G, scale_exp(G, 13), 2), G.astype(np.float64))),
              ("kernel hi+lo", np.array_equal(planes(kernel, 8, 2), kernel.astype(np.float64)))]
    return out
  npl = PLANES[form]
  eg, eh, ex = wgrad_exps(form, x, G)
  if not TRIPLE[form]:
    return [("G", np.array_equal(planes(G, eg, npl), G.astype(np.float64))),
            ("h", np.array_equal(planes(h, eh, npl), h.astype(np.float64))),
            ("x", np.array_equal(planes(x, ex, npl), x.astype(np.float64)))]
  # the row-triple form: V0..V4 exact in float32 AND in the planes; U0, U1, U4 likewise; of U2 and
  # U3 the integer part (before the single fp32 multiply by 1/6)
  V, U, (Vx32, Vh32, U32) = triple_components(x, h, G, (eg, eh, ex), npl)
  x64, h64, g64 = (np.asarray(t, np.float64) for t in (x, h, G))
  dx, dh = _rows5(x64), _rows5(h64)
  Cx = x.shape[-1]

  def exact_v(d):
    v3, d32 = d[3] - d[1], d[3] - d[2]
    return [2 * (d[0] - d[2]) + v3, d32 - 2 * d[1], 2 * (d[1] - d[2]) + d32, v3,
            2 * v3 + (d[2] - d[4])]

  for c, (vx, vh) in enumerate(zip(exact_v(dx), exact_v(dh))):
    out.append(("V%d x" % c, np.array_equal(V[c][..., :Cx], vx)))
    out.append(("V%d h" % c, np.array_equal(V[c][..., Cx:], vh)))
  g0, g1, g2 = g64[:, 0::3], g64[:, 1::3], g64[:, 2::3]
  out.append(("U0", np.array_equal(U[0], 0.5 * g0)))
  out.append(("U1", np.array_equal(U[1], -0.5 * (g0 + g1 + g2))))
  out.append(("U4", np.array_equal(U[4], -g2)))
  n2, n3 = (g1 - g0) - g2, (g0 + 2 * g1) + 4 * g2
  sixth = np.float32(1.0) / np.float32(6.0)
  out.append(("U2 integer part", np.array_equal(
      U32[2], (n2.astype(np.float32) * sixth)) and np.array_equal(n2.astype(np.float32), n2)))
  out.append(("U3 integer part", np.array_equal(
      U32[3], (n3.astype(np.float32) * sixth)) and np.array_equal(n3.astype(np.float32), n3)))
  return out


# ------------------------------------------------------------------ references
def shift(t, dy, dx):
  """out[m, y, x] = t[m, y + dy, x + dx], zero outside the image"""
  M, H, W = t.shape[:3]
  out = np.zeros_like(t)
  ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
  xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
  out[:, yd, xd] = t[:, ys, xs]
  return out


def _mm(a, b, dtype):
  if dtype == np.float32:       # fp32 accumulation on the CPU (torch), for E32
    import torch
    return torch.matmul(torch.from_numpy(np.ascontiguousarray(a, np.float32)),
                        torch.from_numpy(np.ascontiguousarray(b, np.float32))).numpy()
  return np.matmul(np.asarray(a, np.float64), np.asarray(b, np.float64))


def dgrad_taps(G, kernel, dtype=np.float64):
  """[9][M, H, W, Cx + C]: tap (ky, kx)'s share of d [x | h] -- out(y, x) of the forward sees
  in(y + ky - 1, x + kx - 1), so in(y, x) collects G(y - ky + 1, x - kx + 1) K[ky, kx]^T"""
  M, H, W, N4 = G.shape
  out = []
  for ky in range(3):
    for kx in range(3):
      g = shift(G, -(ky - 1), -(kx - 1)).reshape(-1, N4)
      out.append(_mm(g, np.asarray(kernel[ky, kx]).T, dtype).reshape(M, H, W, -1))
  return out


def dgrad_ref(G, kernel, dtype=np.float64):
  t = dgrad_taps(G, kernel, dtype)
  acc = t[0].copy()
  for u in t[1:]:
    acc = acc + u
  return acc


def wgrad_ref(a, G, dtype=np.float64, cells=None, kh=3):
  """dW[ky, kx, ci, n] = sum over cells m of a[m + (ky - 1, kx - 1)][ci] G[m][n]; kh = 1: the row
  of taps ky = 1 alone.  `cells`: a boolean [M, H, W] mask of the cells m summed over."""
  N4 = G.shape[-1]
  g = np.asarray(G, dtype)
  if cells is not None:
    g = g * cells[..., None]
  out = np.zeros((kh, 3, a.shape[-1], N4), dtype)
  for iy, ky in enumerate(range(3) if kh == 3 else [1]):
    for kx in range(3):
      s = shift(np.asarray(a, dtype), ky - 1, kx - 1).reshape(-1, a.shape[-1])
      out[iy, kx] = _mm(s.T, g.reshape(-1, N4), dtype)
  return out


def wgrad_triple_partials(x, h, G, exps, npl, dtype=np.float64, part="sum"):
  """the 15 partial taps M_c = sum over triple-cells of V_c U_c: five [1, 3, Cx + C, 4C]"""
  V, U, _ = triple_components(x, h, G, exps, npl, part)
  return [wgrad_ref(V[c], U[c], dtype, kh=1) for c in range(5)]


def wgrad_triple_ref(x, h, G, exps, npl, dtype=np.float64, part="sum"):
  Mc = wgrad_triple_partials(x, h, G, exps, npl, dtype, part)
  return np.concatenate([((Mc[0] + Mc[1]) + Mc[2]) + Mc[3], (Mc[1] - Mc[2]) + 2 * Mc[3],
                         ((Mc[1] + Mc[2]) + 4 * Mc[3]) + Mc[4]], axis=0)


def wgrad_structural_zeros(form, x, h, G):
  """Boolean [3, 3, Cx + C, 4C]: the entries NO product reaches.  Direct forms: where the
  reference is zero (sums of products of one sign pattern per entry in the one-hot cases: no
  cancellation).  Row-triple forms: where all five partial taps of the column shift are zero --
  the other zeros of the reference are CANCELLATIONS of the 15 partial taps (a pair one image
  row apart feeds all three kernel rows and cancels in two), exact in float64 and to a few 1e-9
  in the fp32 reduce."""
  if not TRIPLE[form]:
    return wgrad_form_ref(form, x, h, G) == 0
  Mc = wgrad_triple_partials(x, h, G, wgrad_exps(form, x, G), PLANES[form])
  none = np.all([m == 0 for m in Mc], axis=0)          # [1, 3, Cx + C, 4C]
  return np.repeat(none, 3, axis=0)


def wgrad_form_ref(form, x, h, G, dtype=np.float64, part="sum"):
  """The reference of a wgrad form on operands that need NOT be fixed points: the planes' values
  (f16_scaled of the oracle for one plane), float64 accumulation.  part "lo": the same
  contraction of the LOWER planes alone."""
  npl, exps = PLANES[form], wgrad_exps(form, x, G)
  if TRIPLE[form]:
    return wgrad_triple_ref(x, h, G, exps, npl, dtype, part)
  a = np.concatenate([planes(x, exps[2], npl, part), planes(h, exps[1], npl, part)], axis=-1)
  return wgrad_ref(a, planes(G, exps[0], npl, part), dtype)


def kernel_slices(a, C):
  """(label, view) of a gate kernel [3, 3, Cx + C, 4C]: per tap, x rows and h rows."""
  Cx = a.shape[2] - C
  out = []
  for ky in range(3):
    for kx in range(3):
      if Cx > 0:
        out.append(("tap %d,%d x rows" % (ky, kx), a[ky, kx, :Cx]))
      out.append(("tap %d,%d h rows" % (ky, kx), a[ky, kx, Cx:]))
  return out


def rel_err(got, ref):
  """max |got - ref| / max |ref|"""
  return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


# ------------------------------------------------------------------ the mutation floor
def edge_sets(M, H, W, block):
  """Boolean [M, H, W] masks of the cell sets a broken kernel would lose: the first and the last
  row of every image, and the last (partial) block of `block` cells."""
  sets = []
  for m in range(M):
    for y in (0, H - 1):
      s = np.zeros((M, H, W), bool)
      s[m, y] = True
      sets.append(("image %d row %d" % (m, y), s))
  tot = M * H * W
  s = np.zeros(tot, bool)
  s[(tot - 1) // block * block:] = True
  sets.append(("last block of %d" % block, s.reshape(M, H, W)))
  return sets


def dgrad_floor(G, kernel, Cx):
  """F of a dgrad case: the smallest max|ref - mutant| / max|ref| per output tensor over the
  mutants 'tap t adds nothing to the OUTPUT cells of one edge set' (32-cell tiles)."""
  taps = dgrad_taps(G, kernel)
  ref = dgrad_ref(G, kernel)
  M, H, W = G.shape[:3]
  best = (np.inf, None)
  for what, sl in (("dx", slice(0, Cx)), ("dh", slice(Cx, None))):
    den = np.abs(ref[..., sl]).max()
    for t, tp in enumerate(taps):
      for name, s in edge_sets(M, H, W, 32):
        e = np.abs(tp[..., sl][s]).max() / den
        if e > 0 and e < best[0]:           # (a tap that reaches outside the image adds nothing)
          best = (float(e), (what, t, name))
  return best


def wgrad_floor(a, G, C):
  """F of a wgrad case: the same with 'tap t loses the cells of one edge set from its sum', per
  slice (tap, x rows / h rows), 64-cell blocks."""
  ref = wgrad_ref(a, G)
  M, H, W = G.shape[:3]
  best = (np.inf, None)
  for name, s in edge_sets(M, H, W, 64):
    lost = wgrad_ref(a, G, cells=s)
    for (what, l), (_, r) in zip(kernel_slices(lost, C), kernel_slices(ref, C)):
      e = np.abs(l).max() / np.abs(r).max()
      if e > 0 and e < best[0]:
        best = (float(e), (what, name))
  return best


# ------------------------------------------------------------------ bars
# One constant per form: max|got - ref| / max|ref slice|.  At least 8 x the largest E32 of the
# form's cases (E32: the same contraction on the same operands accumulated in float32 on the CPU,
# against float64), at most F / 4 of every case: tests/test_bwd_cases_host.py asserts both and
# prints the figures; the docstring of tests/test_gpu_bwd_kernels.py carries them.  Where E32 is
# zero (7-bit operands: every partial sum is an integer below 2^24 quanta) the constant is one fp32
# rounding of a sum that large, 2^-23, times the same 8.
DGRAD_BAR = {"f16x3": 4e-6, "wino": 4e-6, "bf16": 1e-6}
WGRAD_BAR = {"f16x3": 5e-6, "f16x3_triple": 2e-5, "one": 2.5e-6, "one_triple": 1e-5}
ONE_HOT_BAR = 1e-6


def dgrad_e32(G, kernel, Cx):
  ref, r32 = dgrad_ref(G, kernel), dgrad_ref(G, kernel, np.float32)
  return max(rel_err(r32[..., :Cx], ref[..., :Cx]), rel_err(r32[..., Cx:], ref[..., Cx:]))


def wgrad_e32(form, x, h, G, C):
  ref, r32 = wgrad_form_ref(form, x, h, G), wgrad_form_ref(form, x, h, G, np.float32)
  return max(rel_err(b, a) for (_, a), (_, b) in zip(kernel_slices(ref, C), kernel_slices(r32, C)))


# ------------------------------------------------------------------ one-hot cases
def tap_channels(t, Cx, C):
  """(x channel, h channel, gate column) of tap t = 3 ky + kx: distinct per tap, spread over the
  channel blocks"""
  return (t * 3 + 1) % Cx, (7 + 29 * t) % C, (11 + 113 * t) % (4 * C)


def hot_cells(M, H, W, block, extra=()):
  """One hot cell (y, x) per image: the cells either side of a `block`-cell seam of the flat cell
  index (in the first two images that hold a seam inside; where seams fall between images the
  corners are those cells), the four corners, `extra`, then the middle."""
  K = H * W
  cells = [None] * M
  inside = [(m, s) for s in range(block, M * K, block) for m in range(M) if m * K < s < (m + 1) * K]
  if inside:
    m, s = inside[0]
    cells[m] = divmod(s - 1 - m * K, W)            # left of a seam
    for m2, s2 in inside[1:]:
      if m2 != m:
        cells[m2] = divmod(s2 - m2 * K, W)          # right of one
        break
  want = [(H - 1, W - 1), (0, W - 1), (H - 1, 0), (0, 0)] + list(extra)
  for m in range(M):
    if cells[m] is None:
      cells[m] = want.pop(0) if want else (H // 2, W // 2)
  return cells


def one_hot_dgrad(H, W, Cx, C, M=8):
  """G: one hot cell per image, nine hot gate columns in it (one per tap); kernel: tap t holds one
  weight for the x channel and one for the h channel of tap_channels(t).  Then every image of dx
  and of dh has at most nine nonzeros, one per tap and channel, each ONE exact product."""
  cells = hot_cells(M, H, W, 32)
  x = np.zeros((M, H, W, Cx), "f4")
  h = np.zeros((M, H, W, C), "f4")
  G = np.zeros((M, H, W, 4 * C), "f4")
  kernel = np.zeros((3, 3, Cx + C, 4 * C), "f4")
  for t in range(9):
    cx, ch, n = tap_channels(t, Cx, C)
    kernel[t // 3, t % 3, cx, n] = 0.25 + t / 32.0
    kernel[t // 3, t % 3, Cx + ch, n] = -(0.5 + t / 32.0)
    for m, (sy, sx) in enumerate(cells):
      G[m, sy, sx, n] = (m + 1) / 64.0
  return x, h, G, kernel, cells


def one_hot_wgrad(H, W, Cx, C, M=8, extra=()):
  """G: one hot cell g per image with nine hot gate columns; x and h: for every tap t a hot cell
  at the FLAT index of g + (ky - 1) W + (kx - 1), channel tap_channels(t) -- the neighbour where
  it lies inside the image, else the cell a kernel that forgot the image's edge would read (the
  previous / next image row, the neighbouring image): the reference holds those to zero."""
  cells = hot_cells(M, H, W, 64, extra)
  K = H * W
  x = np.zeros((M * K, Cx), "f4")
  h = np.zeros((M * K, C), "f4")
  G = np.zeros((M, H, W, 4 * C), "f4")
  for m, (sy, sx) in enumerate(cells):
    for t in range(9):
      cx, ch, n = tap_channels(t, Cx, C)
      G[m, sy, sx, n] = (t + 1) / 64.0
      f = m * K + sy * W + sx + (t // 3 - 1) * W + (t % 3 - 1)
      if 0 <= f < M * K:
        x[f, cx] = (m + 1) / 16.0
        h[f, ch] = -(m + 2) / 32.0
  return x.reshape(M, H, W, Cx), h.reshape(M, H, W, C), G, cells


# ------------------------------------------------------------------ where an error sits
def where_cells(err, name):
  """worst error of an [M, H, W, C] tensor: by image, row, column, channel block"""
  M, H, W, C = err.shape
  lines = ["%s: max %.3g at %s" % (name, err.max(), np.unravel_index(err.argmax(), err.shape))]
  lines.append("  by image      " + " ".join("%.1e" % err[m].max() for m in range(M)))
  lines.append("  by row        " + " ".join("%.1e" % err[:, y].max() for y in range(H)))
  lines.append("  by column     " + " ".join("%.1e" % err[:, :, xx].max() for xx in range(W)))
  nb = max(1, C // 16)
  lines.append("  by ch block16 " + " ".join("%.1e" % err[..., b * 16:(b + 1) * 16].max()
                                            for b in range(nb)))
  return "\n".join(lines)


def where_kernel(err, Cx, name):
  """worst error of a [3, 3, Cx + C, 4C] tensor: by tap, x rows / h rows, gate-column block"""
  lines = ["%s: max %.3g at %s" % (name, err.max(), np.unravel_index(err.argmax(), err.shape))]
  for ky in range(3):
    lines.append("  tap %d,*  x rows " % ky + " ".join("%.1e" % err[ky, kx, :Cx].max()
                                                       for kx in range(3)) +
                 "   h rows " + " ".join("%.1e" % err[ky, kx, Cx:].max() for kx in range(3)))
  N4 = err.shape[3]
  lines.append("  by column block128 " + " ".join("%.1e" % err[..., b * 128:(b + 1) * 128].max()
                                                 for b in range(N4 // 128)))
  return "\n".join(lines)
