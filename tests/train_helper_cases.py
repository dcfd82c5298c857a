# coding=utf-8
"""Inputs, float64 references and bars of the training helper kernels' single-kernel tests
(tests/test_gpu_train_helpers.py) and of their CPU-side checks
(tests/test_train_helper_cases_host.py): the losses, the small 3x3 convolutions behind
hidden2grid and grid_emb, the stride-2 scene stack, the column sums and long sums, and the
one-hot embedding wgrad (csrc/train_kernels.h, csrc/kernels_misc.h, launched by
csrc/engine_train.h).

EXACT OPERANDS.  Data are multiples of 2^-3 in [-1, 1], weights multiples of 2^-4 in [-1, 1].
Every product is then a multiple of a common quantum, and as long as the sum of the |terms| of an
output stays below 2^24 quanta (`premise`), every partial sum in ANY order is a float32: nothing
rounds, and the device must equal the float64 reference with ==.  Only the cross entropies
(exp, log) have a tolerance (`ce_bars`).

REFERENCES are plain tap loops in numpy float64 written from the TF semantics
(tf.nn.conv2d SAME, tf.losses.huber_loss, softmax cross entropy), not from the kernels.  The host
test holds them to torch.autograd in float64.

DEVICE MODELS (`model_*`) are float32 restatements of the kernels' arithmetic in the kernels'
own flat-index form.  They are NOT the reference: the host test shows that the comparison
functions pass them, and that every entry of MUTATIONS, a switch that makes a model wrong the
way a kernel could be, fails at least one named case."""

import numpy as np

QD, QW = 2.0 ** -3, 2.0 ** -4        # quanta of data and of weights
EXACT_LIMIT = 2.0 ** 24
U32 = 2.0 ** -24                     # unit roundoff of float32


def data(rng, shape, lo=-8, hi=8):
  """multiples of 2^-3 in [lo/8, hi/8]"""
  return rng.integers(lo, hi + 1, size=shape).astype(np.float64) * QD


def weights(rng, shape):
  """multiples of 2^-4 in [-1, 1]"""
  return rng.integers(-16, 17, size=shape).astype(np.float64) * QW


def _seed(name):
  """a stable seed from a case name (hash() of a str changes from run to run)"""
  s = 0
  for ch in name:
    s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
  return s


def premise(abs_sum, quantum, nterms=None):
  """The exactness premise: sum |terms| of every output < 2^24 quanta -- or, where the terms
  are not on a common grid (the leaky slope), at most ONE non-zero term per output."""
  if nterms is not None:
    return bool(np.max(nterms) <= 1)
  return bool(np.max(abs_sum) / quantum < EXACT_LIMIT)


def compare_exact(got, want, keys=None):
  """== on values (0.0 == -0.0) of every array of `want` (or of `keys`): the list of
  mismatches, empty when all agree."""
  bad = []
  for k in (keys if keys is not None else sorted(want)):
    g, w = np.asarray(got[k]), np.asarray(want[k], dtype=np.float64).astype(np.float32)
    if g.shape != w.shape:
      bad.append("%s: shape %s, expected %s" % (k, g.shape, w.shape))
      continue
    ne = ~(g == w)              # a NaN on either side is a mismatch
    if ne.any():
      i = tuple(int(v[0]) for v in np.nonzero(ne)) if g.ndim else ()
      bad.append("%s: %d of %d differ, first at %s: %r, expected %r"
                 % (k, int(ne.sum()), g.size, i, float(g[i]), float(w[i])))
  return bad


# =================================================================== 3x3 SAME, stride 1
TAPS = [(ky, kx) for ky in range(3) for kx in range(3)]


def _tap_slices(H, W, ky, kx):
  """tf.nn.conv2d SAME 3x3: out(y, x) reads in(y + ky - 1, x + kx - 1).  The out cells whose
  tap lies inside the image, and the in cells they read."""
  dy, dx = ky - 1, kx - 1
  y0, y1 = max(0, -dy), min(H, H - dy)
  x0, x1 = max(0, -dx), min(W, W - dx)
  if y1 <= y0 or x1 <= x0:
    return None
  return (slice(y0, y1), slice(x0, x1)), (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))


def conv3x3_ref(x, w):
  M, H, W, _ = x.shape
  out = np.zeros((M, H, W, w.shape[3]))
  for ky, kx in TAPS:
    s = _tap_slices(H, W, ky, kx)
    if s:
      (oy, ox), (iy, ix) = s
      out[:, oy, ox, :] += x[:, iy, ix, :] @ w[ky, kx]
  return out


def conv3x3_dgrad_ref(dout, w):
  """d in of out = conv3x3(in, w): in(y + ky - 1, x + kx - 1) gets dout(y, x) w[ky, kx]^T"""
  M, H, W, _ = dout.shape
  din = np.zeros((M, H, W, w.shape[2]))
  for ky, kx in TAPS:
    s = _tap_slices(H, W, ky, kx)
    if s:
      (oy, ox), (iy, ix) = s
      din[:, iy, ix, :] += dout[:, oy, ox, :] @ w[ky, kx].T
  return din


def conv3x3_wgrad_ref(x, dout):
  M, H, W, Ci = x.shape
  dw = np.zeros((3, 3, Ci, dout.shape[3]))
  for ky, kx in TAPS:
    s = _tap_slices(H, W, ky, kx)
    if s:
      (oy, ox), (iy, ix) = s
      dw[ky, kx] = np.einsum("myxi,myxo->io", x[:, iy, ix, :], dout[:, oy, ox, :])
  return dw


# ------------------------------------------------------------------ small dgrad
SMALL_DGRAD_SHAPES = [(1, 1, 1), (1, 4, 5), (5, 2, 7), (2, 9, 16)]
SMALL_DGRAD_CHANNELS = [(256, 1), (256, 2), (512, 2), (128, 1),      # dgrad4
                        (2, 32), (1, 32), (2, 64),                   # scalar, 16-byte loads
                        (3, 6)]                                      # scalar, no vector path
# row strides: extra floats after the H*W*C of a row, for (dout, din)
SMALL_DGRAD_STRIDES = {"tight": (0, 0), "slice": (8, 12), "odd": (2, 2)}


def small_dgrad_form_expected(Ci, Co, din_rs):
  """engine_train.h plan_small_dgrad, written out: four input channels per thread where Ci is a
  multiple of 4, Co is 1 or 2 and the din row stride keeps 16-byte alignment."""
  if Ci % 4 == 0 and Co in (1, 2) and din_rs % 4 == 0:
    return "dgrad4<%d>" % Co
  return "scalar"


def small_dgrad_cases():
  out = []
  for (Ci, Co) in SMALL_DGRAD_CHANNELS:
    for (M, H, W) in SMALL_DGRAD_SHAPES:
      for acc in (0, 1):
        strides = ["tight"]
        if (M, H, W) == (5, 2, 7):
          strides += ["slice"] + (["odd"] if (Ci, Co) in ((256, 2), (2, 32), (3, 6)) else [])
        for st in strides:
          out.append(dict(name="dgrad_%dx%d_%d.%d.%d_%s_acc%d" % (Ci, Co, M, H, W, st, acc),
                          M=M, H=H, W=W, Ci=Ci, Co=Co, stride=st, accumulate=acc))
  return out


def small_dgrad_inputs(c):
  rng = np.random.default_rng(_seed(c["name"]))
  M, H, W, Ci, Co = c["M"], c["H"], c["W"], c["Ci"], c["Co"]
  eo, ei = SMALL_DGRAD_STRIDES[c["stride"]]
  dout = data(rng, (M, H * W * Co + eo))       # the padding holds data too: it must not be read
  w = weights(rng, (3, 3, Ci, Co))
  din = data(rng, (M, H * W * Ci + ei))
  return dout, w, din


def small_dgrad_ref(c, dout, w, din):
  """-> (the whole din buffer afterwards, sum |terms| per element)"""
  M, H, W, Ci, Co = c["M"], c["H"], c["W"], c["Ci"], c["Co"]
  n_o, n_i = H * W * Co, H * W * Ci
  d = dout[:, :n_o].reshape(M, H, W, Co)
  g = conv3x3_dgrad_ref(d, w).reshape(M, n_i)
  a = conv3x3_dgrad_ref(np.abs(d), np.abs(w)).reshape(M, n_i)
  out, mag = din.copy(), np.abs(din)
  if c["accumulate"]:
    out[:, :n_i] += g
    mag[:, :n_i] += a
  else:
    out[:, :n_i] = g
    mag[:, :n_i] = a
  return out, mag


# one-hot dout: the four corners, an edge midpoint and an interior cell of a 4 x 5 image, one
# image each; tap t has its only weight at input channel t, so channel t of din shows tap t
ONEHOT_H, ONEHOT_W = 4, 5
ONEHOT_POSITIONS = [(0, 0), (0, 4), (3, 0), (3, 4), (0, 2), (2, 2)]


def small_dgrad_onehot(Ci, Co):
  M = len(ONEHOT_POSITIONS)
  dout = np.zeros((M, ONEHOT_H, ONEHOT_W, Co))
  w = np.zeros((3, 3, Ci, Co))
  co0 = Co - 1
  for m, (py, px) in enumerate(ONEHOT_POSITIONS):
    dout[m, py, px, co0] = 0.5
  for t, (ky, kx) in enumerate(TAPS):
    w[ky, kx, t, co0] = (t + 1) * QW                 # distinct per tap
  # out(py, px) reads in(py + ky - 1, px + kx - 1): that cell of channel t, nothing else
  cells = set()
  for m, (py, px) in enumerate(ONEHOT_POSITIONS):
    for t, (ky, kx) in enumerate(TAPS):
      y, x = py + ky - 1, px + kx - 1
      if 0 <= y < ONEHOT_H and 0 <= x < ONEHOT_W:
        cells.add((m, y, x, t))
  return dout, w, cells


# ------------------------------------------------------------------ small wgrad
SMALL_WGRAD_SHAPES = [(1, 1, 1), (1, 4, 5), (5, 2, 7), (3, 5, 7), (2, 9, 16), (1, 3, 31)]
# (Ci, Co) -> the plan's form and G, written out from engine_train.h plan_small_wgrad:
#   P = Ci Co, G = max(1, 256 // P) cell groups per workgroup
#   h2g where Ci > Co, Ci <= 512, Co is 1 or 2 AND G == 1 (P > 128); else <true> where Ci > Co;
#   else <false>
SMALL_WGRAD_CHANNELS = {
    (256, 1): ("h2g", 1), (256, 2): ("h2g", 1), (512, 2): ("h2g", 1), (128, 2): ("h2g", 1),
    (128, 1): ("small_wgrad<true>", 2), (64, 1): ("small_wgrad<true>", 4),
    (64, 2): ("small_wgrad<true>", 2),
    (1, 32): ("small_wgrad<false>", 8), (2, 32): ("small_wgrad<false>", 4),
    (1, 64): ("small_wgrad<false>", 4), (2, 128): ("small_wgrad<false>", 1),
}
SMALL_WGRAD_REFUSED = (2, 512)
# cells -> (blocks, cells per block): blocks = min(4096, ceil(cells / 64)), cells per block =
# ceil(cells / blocks), blocks = ceil(cells / cells per block)
SMALL_WGRAD_BLOCKS = {1: (1, 1), 20: (1, 20), 70: (2, 35), 105: (2, 53), 288: (5, 58),
                      93: (2, 47)}


def small_wgrad_forms_allowed(Ci, Co):
  """the forms a shape can be forced into (engine_ops.h mv_op_small_conv_wgrad)"""
  out = []
  if Ci * Co <= 512:
    out += ["small_wgrad<false>", "small_wgrad<true>"]
  if Co in (1, 2):
    out.append("h2g")
  return out


def small_wgrad_inputs(R, H, W, Ci, Co):
  rng = np.random.default_rng(_seed("wgrad_%d_%d_%d_%d_%d" % (R, H, W, Ci, Co)))
  return data(rng, (R, H, W, Ci)), data(rng, (R, H, W, Co))


def small_wgrad_seam_cells(R, H, W):
  """flat cells either side of the first image seam and of the first block seam (from the
  blocks rule above; the GPU test takes the block seam from what the door reports)"""
  hw = H * W
  cpb = SMALL_WGRAD_BLOCKS[R * hw][1]
  return dict(image=(hw - 1, hw), block=(cpb - 1, cpb))


def small_wgrad_onehot(R, H, W, Ci, Co, s):
  """One-hot pairs around flat cell s.  The wide operand carries one hot cell per flat offset o
  (in its own channel), the narrow operand is hot at s: channel j shows the pair at distance
  OFFSETS[j].  -> (in, dout, the set of (ky, kx, ci, co) that are non-zero)"""
  total, hw = R * H * W, H * W
  offs = [dy * W + dx for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
  x = np.zeros((total, Ci))
  d = np.zeros((total, Co))
  pairs = []                                   # (a = in cell, b = dout cell, ci, co)
  if Ci >= 9:                                  # wide in: in hot at s + o, dout hot at s
    d[s, Co - 1] = 0.5
    for j, o in enumerate(offs):
      if 0 <= s + o < total:
        x[s + o, j] = 0.25 * (j + 1)
        pairs.append((s + o, s, j, Co - 1))
  else:                                        # wide out: in hot at s, dout hot at s - o
    x[s, Ci - 1] = 0.5
    for j, o in enumerate(offs):
      if 0 <= s - o < total:
        d[s - o, j] = 0.25 * (j + 1)
        pairs.append((s, s - o, Ci - 1, j))
  # dw[ky, kx, ci, co] = sum over out cells b of in(b + tap) dout(b): the pair (a, b) feeds tap
  # (ky, kx) iff a is b's neighbour (ky - 1, kx - 1) INSIDE b's image
  nz = set()
  for a, b, ci, co in pairs:
    r, cell = divmod(b, hw)
    y, xx = divmod(cell, W)
    for ky, kx in TAPS:
      ny, nx = y + ky - 1, xx + kx - 1
      if 0 <= ny < H and 0 <= nx < W and a == r * hw + ny * W + nx:
        nz.add((ky, kx, ci, co))
  return x.reshape(R, H, W, Ci), d.reshape(R, H, W, Co), nz


# =================================================================== column sums, long sums
COLSUM_ROWS = [1, 64, 65, 2048, 2049, 65537]
COLSUM_NCOLS_NARROW = [1, 2, 32, 128]
COLSUM_NCOLS_WIDE = [48, 300, 1024]
# rows -> slabs, from engine_train.h plan_colsum: slabs = min(1024, ceil(rows / 64)), rows per
# slab = ceil(rows / slabs), slabs = ceil(rows / rows per slab)
#   65: 2 slabs of 33 (33 + 32)        2048: 32 of 64 (no fold pass)
#   2049: 33 slabs of 63 (the fold runs: 33 -> 2 -> 1, its second row holds ONE partial)
#   65537: 1024 -> 65 rows per slab -> 1009 slabs (1008 full + 17 rows), fold 1009 -> 32 -> 1
COLSUM_SLABS = {1: 1, 64: 1, 65: 2, 2048: 32, 2049: 33, 65537: 1009}
COLSUM_RPS = {1: 1, 64: 64, 65: 33, 2048: 64, 2049: 63, 65537: 65}


def colsum_cases():
  return [(r, n) for n in COLSUM_NCOLS_NARROW + COLSUM_NCOLS_WIDE for r in COLSUM_ROWS
          if not (r == 65537 and n > 128)]


def colsum_narrow_expected(rows, ncols):
  """the narrow kernel sums the slabs where there is more than one and ncols divides 256
  (ncols <= 128)"""
  return COLSUM_SLABS[rows] > 1 and ncols <= 128 and 256 % ncols == 0


def colsum_input(rows, ncols):
  rng = np.random.default_rng(rows * 4099 + ncols)
  return rng.integers(-8, 9, size=(rows, ncols)).astype(np.int8)     # x 2^-3


def colsum_ref(xi):
  """-> (sums, sum |terms|) of x = xi * 2^-3"""
  return xi.sum(axis=0, dtype=np.int64) * QD, np.abs(xi).sum(axis=0, dtype=np.int64) * QD


LONG_SUM_CHUNK = 4096                  # train_kernels.h kSumChunk
LONG_SUM_N = [1, 255, 257, 4 * LONG_SUM_CHUNK, 4 * LONG_SUM_CHUNK + 1, 40000]
LONG_SUM_SCALES = [1.0, 2.0 ** -3]


def long_sum_input(n):
  x = data(np.random.default_rng(7000 + n), (n,))
  x[-1] = 1.0                          # the last element counts
  return x


# =================================================================== stride-2 SAME scene stack
def same_pad(n_in, k, stride=2):
  """tf SAME: out = ceil(in / stride), total padding max((out - 1) stride + k - in, 0), the
  smaller half in front"""
  n_out = -(-n_in // stride)
  return n_out, max((n_out - 1) * stride + k - n_in, 0) // 2


def _s2_index(n_in, k, kk):
  """out index o reads in index 2 o + kk - pad: (the o inside, the in index they read)"""
  n_out, pad = same_pad(n_in, k)
  o = np.arange(n_out)
  i = 2 * o + kk - pad
  ok = (i >= 0) & (i < n_in)
  return o[ok], i[ok]


def conv_s2_ref(x, w):
  U, Hi, Wi, _ = x.shape
  k = w.shape[0]
  out = np.zeros((U, same_pad(Hi, k)[0], same_pad(Wi, k)[0], w.shape[3]))
  for ky in range(k):
    oy, iy = _s2_index(Hi, k, ky)
    for kx in range(k):
      ox, ix = _s2_index(Wi, k, kx)
      if len(oy) and len(ox):
        out[:, oy[:, None], ox[None, :], :] += x[:, iy[:, None], ix[None, :], :] @ w[ky, kx]
  return out


def conv_s2_dgrad_ref(dpre, w, Hi, Wi):
  U = dpre.shape[0]
  k = w.shape[0]
  din = np.zeros((U, Hi, Wi, w.shape[2]))
  for ky in range(k):
    oy, iy = _s2_index(Hi, k, ky)
    for kx in range(k):
      ox, ix = _s2_index(Wi, k, kx)
      if len(oy) and len(ox):
        din[:, iy[:, None], ix[None, :], :] += dpre[:, oy[:, None], ox[None, :], :] @ w[ky, kx].T
  return din


def conv_s2_wgrad_ref(x, dpre, k):
  U, Hi, Wi, Ci = x.shape
  dw = np.zeros((k, k, Ci, dpre.shape[3]))
  for ky in range(k):
    oy, iy = _s2_index(Hi, k, ky)
    for kx in range(k):
      ox, ix = _s2_index(Wi, k, kx)
      if len(oy) and len(ox):
        dw[ky, kx] = np.einsum("uyxi,uyxo->io", x[:, iy[:, None], ix[None, :], :],
                               dpre[:, oy[:, None], ox[None, :], :])
  return dw


LRELU_SLOPE = float(np.float32(0.2))   # the float32 the kernels multiply by


def act_grad_ref(act, y):
  """d act / d pre from the output y: tanh 1 - y^2; relu / leaky relu the slope of y's sign"""
  if act == 0:
    return 1.0 - y * y
  return np.where(y > 0, 1.0, 0.0 if act == 1 else LRELU_SLOPE)


# (U, Hi, Wi, Ci, Co, k) -> pad_t, pad_l, wgrad slabs, output rows per slab.  Slabs from
# engine_train.h plan_scene_wgrad: rows = U Ho, rows per slab = ceil(rows / 64), slabs =
# ceil(rows / rows per slab)
SCENE_SHAPES = {
    (3, 7, 10, 11, 64, 3): (1, 0, 12, 1),       # Ho 4: (3 2 + 3 - 7) / 2 = 1; Wo 5: 8 + 3 - 10 = 1 -> 0
    (1, 5, 6, 64, 64, 3): (1, 0, 3, 1),
    (2, 9, 9, 11, 64, 1): (0, 0, 10, 1),
    (1, 8, 6, 3, 8, 5): (1, 1, 4, 1),           # Ho 4: 6 + 5 - 8 = 3 -> 1; Wo 3: 4 + 5 - 6 = 3 -> 1
    (1, 7, 5, 3, 8, 5): (2, 2, 4, 1),           # Ho 4: 6 + 5 - 7 = 4 -> 2; Wo 3: 4 + 5 - 5 = 4 -> 2
    (2, 1, 1, 4, 4, 3): (1, 1, 2, 1),           # Ho 1: 0 + 3 - 1 = 2 -> 1
    (17, 8, 4, 3, 8, 3): (0, 0, 34, 2),         # 68 output rows: slabs of 2 straddle images
}
SCENE_ACTS = ("tanh", "relu", "lrelu", "lrelu_dpre", "lrelu_slope")
ACT_CODE = {"tanh": 0, "relu": 1, "lrelu": 2, "lrelu_dpre": 2, "lrelu_slope": 2}


def scene_cases():
  # (the two extra leaky cases write din fresh: init + ONE rounded product would round twice)
  return [dict(name="scene_%s_%s_acc%d" % (".".join(map(str, s)), a, acc), shape=s, act=a,
               accumulate=acc)
          for s in SCENE_SHAPES for a in SCENE_ACTS
          for acc in ((0, 1) if a in ("tanh", "relu", "lrelu") else (0,))]


def scene_inputs(c):
  """x, y (the forward OUTPUT, an input of the door), dy, w, din_init.  tanh: y a multiple of 2^-3
  inside (-1, 1), so 1 - y^2 is exact.  The leaky slope 0.2f is no dyadic: `lrelu` has dy = 0
  where y <= 0 (every sum exact), `lrelu_dpre` dense dy (dpre alone is checked: one rounding on
  either side), `lrelu_slope` ONE non-zero dy, at a cell with y < 0 (every output one term)."""
  U, Hi, Wi, Ci, Co, k = c["shape"]
  rng = np.random.default_rng(_seed(c["name"]))
  Ho, Wo = same_pad(Hi, k)[0], same_pad(Wi, k)[0]
  x = data(rng, (U, Hi, Wi, Ci))
  w = weights(rng, (k, k, Ci, Co))
  dy = data(rng, (U, Ho, Wo, Co))
  act = c["act"]
  if act == "tanh":
    y = data(rng, (U, Ho, Wo, Co), -7, 7)
  elif act == "relu":
    y = np.maximum(data(rng, (U, Ho, Wo, Co), -5, 8), 0.0)
  else:
    y = data(rng, (U, Ho, Wo, Co))
    y[y == 0] = -QD
    if act == "lrelu":
      dy = np.where(y > 0, dy, 0.0)
    elif act == "lrelu_slope":
      flat = np.flatnonzero(y.reshape(-1) < 0)
      hot = flat[len(flat) // 2]
      dy = np.zeros(y.size)
      dy[hot] = 0.75
      dy = dy.reshape(y.shape)
  init = data(rng, x.shape)
  return x, y, dy, w, init


def scene_check_keys(c):
  return ("dpre",) if c["act"] == "lrelu_dpre" else ("dpre", "din", "dw", "db")


def scene_ref(c, x, y, dy, w, init):
  """-> (dict of dpre, din, dw, db; dict of sum |terms|; quantum; dict of term counts or None)"""
  U, Hi, Wi, Ci, Co, k = c["shape"]
  g = act_grad_ref(ACT_CODE[c["act"]], y)
  dpre = dy * g
  # float32 has ONE rounding here (the leaky slope); the sums then run on the rounded value
  dpre = dpre.astype(np.float32).astype(np.float64)
  ref = dict(dpre=dpre, din=conv_s2_dgrad_ref(dpre, w, Hi, Wi), dw=conv_s2_wgrad_ref(x, dpre, k),
             db=dpre.sum(axis=(0, 1, 2)))
  a = np.abs(dpre)
  mag = dict(dpre=a, din=conv_s2_dgrad_ref(a, np.abs(w), Hi, Wi),
             dw=conv_s2_wgrad_ref(np.abs(x), a, k), db=a.sum(axis=(0, 1, 2)))
  if c["accumulate"]:
    ref["din"] = ref["din"] + init
    mag["din"] = mag["din"] + np.abs(init)
  cnt = None
  if c["act"] == "lrelu_slope":
    n = (dpre != 0).astype(np.float64)
    cnt = dict(dpre=n, din=conv_s2_dgrad_ref(n, (w != 0) * 1.0, Hi, Wi),
               dw=conv_s2_wgrad_ref((x != 0) * 1.0, n, k), db=n.sum(axis=(0, 1, 2)))
  # dy 2^-3, 1 - y^2 2^-6, w 2^-4, x 2^-3: din on 2^-13, dw on 2^-12
  return ref, mag, 2.0 ** -13, cnt


def scene_onehot(Hi, Wi):
  """One-hot dy at the four output corners (one image each), k = 3, relu with y = 1; tap t has
  its only weight at input channel t.  -> x, y, dy, w, the set of non-zero din cells."""
  k, Ci, Co = 3, 11, 64
  Ho, Wo = same_pad(Hi, k)[0], same_pad(Wi, k)[0]
  pt, pl = same_pad(Hi, k)[1], same_pad(Wi, k)[1]
  corners = [(0, 0), (0, Wo - 1), (Ho - 1, 0), (Ho - 1, Wo - 1)]
  U = len(corners)
  dy = np.zeros((U, Ho, Wo, Co))
  w = np.zeros((k, k, Ci, Co))
  cells = set()
  for u, (oy, ox) in enumerate(corners):
    dy[u, oy, ox, 5] = 0.5
  for t, (ky, kx) in enumerate(TAPS):
    w[ky, kx, t, 5] = 0.25 * (t + 1)
    for u, (oy, ox) in enumerate(corners):     # out(oy, ox) reads in(2 oy + ky - pad_t, ..)
      iy, ix = 2 * oy + ky - pt, 2 * ox + kx - pl
      if 0 <= iy < Hi and 0 <= ix < Wi:
        cells.add((u, iy, ix, t))
  x = data(np.random.default_rng(Hi * 100 + Wi), (U, Hi, Wi, Ci))
  return x, np.ones_like(dy), dy, w, cells


# =================================================================== one-hot embedding wgrad
ONEHOT_WGRAD_SHAPES = [(1, 1, 1, 1, 32), (3, 2, 4, 5, 32), (5, 3, 2, 7, 64), (9, 1, 3, 3, 128)]


def onehot_wgrad_inputs(N, T, H, W, E):
  rng = np.random.default_rng(N * 1000 + T * 100 + H * 10 + W + E)
  labels = rng.integers(0, H * W, size=(N, T))
  corners = [0, W - 1, (H - 1) * W, H * W - 1]
  flat = labels.reshape(-1)
  for i, cnr in enumerate(corners[:flat.size]):
    flat[(i * flat.size) // 4] = cnr             # (the 1 x 1 grid: the one cell is every corner)
  if flat.size >= 4:
    assert set(corners) <= set(flat.tolist())
  return data(rng, (T, N, H, W, E)), labels.astype(np.int32), data(rng, (3, 3, E))


def onehot_wgrad_ref(dpre, labels, dw_init, accumulate):
  """grid_emb is conv3x3 SAME of the one-hot map [H, W, 1]: its dW is the plain wgrad on the
  LITERAL one-hot input (time-major rows m = t N + n, labels [N][T])"""
  T, N, H, W, E = dpre.shape
  hot = np.zeros((T, N, H * W, 1))
  for t in range(T):
    for n in range(N):
      hot[t, n, labels[n, t], 0] = 1.0
  hot = hot.reshape(T * N, H, W, 1)
  d = dpre.reshape(T * N, H, W, E)
  dw = conv3x3_wgrad_ref(hot, d)[:, :, 0, :]
  mag = conv3x3_wgrad_ref(hot, np.abs(d))[:, :, 0, :]
  if accumulate:
    return dw + dw_init, mag + np.abs(dw_init)
  return dw, mag


# =================================================================== Huber
HUBER_E = [0.0, QD, -QD, 1.0, -1.0, 1.0 + QD, -(1.0 + QD), 1.5, -1.5, 4.0, -4.0]
HUBER_SCALE = 2.0 ** -5


def huber_cases():
  big = dict(T=2, N=2, K=2052)          # 16416 elements: the summed loss takes the chunk stage
  small = dict(T=3, N=2, K=20)
  out = [dict(name="huber", kind="huber", **small),
         dict(name="huber_long", kind="huber", **big),
         dict(name="huber_len", kind="huber_len", T=3, N=4, K=20, pred_lens=(0, 3, 1, 2))]
  for cnt, shape in ((0, small), (1, small), (8, big), (70, small)):
    out.append(dict(name="huber_masked_%d" % cnt, kind="huber_masked", count=cnt, **shape))
  return out


def huber_inputs(c):
  """pred [T, N, K, 2] time-major, target [N, T, K, 2]; e = pred - target walks HUBER_E; the
  masked kind's foreground map [T, N, K] with c['count'] cells > 0, spread over the map"""
  T, N, K = c["T"], c["N"], c["K"]
  rng = np.random.default_rng(_seed(c["name"]))
  target = data(rng, (N, T, K, 2))
  e = np.resize(np.array(HUBER_E), (T, N, K, 2))
  pred = target.transpose(1, 0, 2, 3) + e
  fg = None
  if c["kind"] == "huber_masked":
    fg = np.zeros(T * N * K)
    cnt = c["count"]
    if cnt:
      idx = np.unique(np.linspace(0, fg.size - 1, cnt).astype(np.int64))
      assert len(idx) == cnt
      fg[idx] = np.where(np.arange(cnt) % 2 == 0, 1.0, 0.25)     # soft maps: any value > 0
    fg[np.flatnonzero(fg == 0)[0]] = -0.5                        # a negative value is no foreground
    assert int((fg > 0).sum()) == cnt
    fg = fg.reshape(T, N, K)
  return pred, target, fg


def huber_ref(c, pred, target, fg):
  """tf.losses.huber_loss(delta = 1) per element: 0.5 e^2 inside |e| <= 1, |e| - 0.5 outside;
  gradient clip(e, -1, 1) * scale.  -> dict loss, grad, loss_sum (, count), and whether every
  output is exact"""
  T, N, K = c["T"], c["N"], c["K"]
  e = pred - target.transpose(1, 0, 2, 3)
  a = np.abs(e)
  loss = np.where(a <= 1.0, 0.5 * e * e, a - 0.5)
  clip = np.clip(e, -1.0, 1.0)
  exact = True
  if c["kind"] == "huber_masked":
    on = (fg > 0)[..., None]
    cnt = int((fg > 0).sum())
    weight = 0.5
    loss = np.where(on, loss, 0.0)
    # mean over the 2 count foreground elements, times the weight
    scale = weight / (2.0 * cnt) if cnt else 0.0
    grad = np.where(on, clip * scale, 0.0)
    total = loss.sum() * scale
    exact = cnt == 0 or (cnt & (cnt - 1)) == 0
    return dict(loss=loss, grad=grad, loss_sum=total, count=cnt), exact, weight
  scale = HUBER_SCALE
  if c["kind"] == "huber_len":
    valid = (np.arange(T)[:, None] < np.array(c["pred_lens"])[None, :])[..., None, None]
    loss = np.where(valid, loss, 0.0)
    clip = np.where(valid, clip, 0.0)
  return dict(loss=loss, grad=clip * scale, loss_sum=loss.sum() * scale), exact, scale


def compare_huber(c, got, ref, exact):
  """== everywhere; a masked count that is no power of two divides inexactly: there the loss
  elements, the count and the zero pattern are still exact, and the gradient and the summed loss
  are within two roundings (the division, the product) of the float64 value"""
  bad = compare_exact(got, ref, ("loss",) if not exact else ("loss", "grad", "loss_sum"))
  if "count" in ref and got["count"] != ref["count"]:
    bad.append("count %d, expected %d" % (got["count"], ref["count"]))
  if not exact:
    for k in ("grad", "loss_sum"):
      g, w = np.asarray(got[k], dtype=np.float64), np.asarray(ref[k])
      if ((g == 0) != (w == 0)).any() or (np.abs(g - w) > 2 * U32 * np.abs(w)).any():
        bad.append("%s: beyond two roundings of the float64 value (max %.3g x 2^-24 |ref|)"
                   % (k, float(np.max(np.abs(g - w) / np.maximum(np.abs(w), 1e-300)) / U32)))
  return bad


# =================================================================== cross entropies
CE_K = [1, 2, 63, 64, 65, 144, 576, 1100]
CE_LOGITS = ("n01", "hi", "lo")        # N(0,1) with one constant row; 30 N(0,1) + 80; .. - 80
CE_SCALE = 2.0 ** -2
CE_GPU_FACTOR = 4.0                    # the GPU may use 4 x the fp32 torch oracle's constant,
                                       # which counts as 1 where it comes out smaller


def ce_cases():
  out = []
  for K in CE_K:
    for lg in CE_LOGITS:
      out.append(dict(name="ce_K%d_%s" % (K, lg), kind="ce", K=K, logits=lg, T=3, N=2))
      out.append(dict(name="ce_len_K%d_%s" % (K, lg), kind="ce_len", K=K, logits=lg, T=2, N=3,
                      pred_lens=(0, 1, 2)))
    for soft in (1.0, 0.4, 2.5):
      out.append(dict(name="ce_soft_K%d_sum%g" % (K, soft), kind="ce_soft", K=K, logits="n01",
                      T=3, N=2, soft_sum=soft))
    out.append(dict(name="ce_soft_K%d_hi_sw" % K, kind="ce_soft", K=K, logits="hi", T=3, N=2,
                    soft_sum=2.5, sample_w=(0.25, 1.75)))
    out.append(dict(name="ce_K%d_n01_sw" % K, kind="ce", K=K, logits="n01", T=3, N=2,
                    sample_w=(0.25, 1.75)))
    out.append(dict(name="ce_len_soft_K%d" % K, kind="ce_len", K=K, logits="lo", T=2, N=3,
                    pred_lens=(2, 0, 1), soft_sum=0.4))
  return out


def ce_inputs(c):
  """logits [T, N, K] (float32 values), labels [N, T] at 0 / 63 / 64 / K - 1 where they exist,
  soft labels [T, N, K] or None"""
  T, N, K = c["T"], c["N"], c["K"]
  rng = np.random.default_rng(_seed(c["name"]))
  z = rng.standard_normal((T, N, K))
  if c["logits"] == "hi":
    z = z * 30.0 + 80.0
  elif c["logits"] == "lo":
    z = z * 30.0 - 80.0
  else:
    z[T - 1, N - 1, :] = 1.5                       # a constant row
  z = z.astype(np.float32).astype(np.float64)
  named = [v for v in (0, 63, 64, K - 1) if v < K]
  labels = rng.integers(0, K, size=(N, T))
  flat = labels.reshape(-1)
  for i, v in enumerate(named):
    flat[(i * 5 + 1) % flat.size] = v
  soft = None
  if "soft_sum" in c:
    q = rng.random((T, N, K)) ** 4
    q = q / q.sum(axis=-1, keepdims=True) * c["soft_sum"]
    soft = q.astype(np.float32).astype(np.float64)
  return z, labels.astype(np.int32), soft


def ce_ref(c, z, labels, soft):
  """float64: loss row = lse - logit[label] (soft: - sum q (logit - lse)); gradient TF's
  REGISTERED one, (softmax - labels) * scale, whatever the soft labels sum to.  -> ref dict and
  the magnitudes m the bars are relative to."""
  T, N, K = c["T"], c["N"], c["K"]
  mx = z.max(axis=-1)
  lse = np.log(np.exp(z - mx[..., None]).sum(axis=-1)) + mx
  sm = np.exp(z - lse[..., None])
  if soft is not None:
    loss = -(soft * (z - lse[..., None])).sum(axis=-1)
    lab = soft
    m_loss = (np.abs(mx) + np.abs(lse)) * np.abs(soft).sum(axis=-1) + np.abs(soft * z).sum(axis=-1)
    m_grad = np.maximum(1.0, soft.max(axis=-1))
  else:
    zl = np.take_along_axis(z, labels.T[..., None].astype(np.int64), axis=-1)[..., 0]
    loss = lse - zl
    lab = np.zeros_like(z)
    np.put_along_axis(lab, labels.T[..., None].astype(np.int64), 1.0, axis=-1)
    m_loss = np.abs(mx) + np.abs(lse) + np.abs(zl)
    m_grad = np.ones((T, N))
  grad = (sm - lab) * CE_SCALE
  roww = np.ones((T, N))
  if "sample_w" in c:
    roww = roww * np.array(c["sample_w"])[None, :]
  if "pred_lens" in c:
    roww = roww * (np.arange(T)[:, None] < np.array(c["pred_lens"])[None, :])
  loss, grad = loss * roww, grad * roww[..., None]
  m_loss, m_grad = m_loss * np.abs(roww), m_grad * np.abs(roww) * CE_SCALE
  ref = dict(loss=loss, grad=grad, loss_sum=loss.sum() * CE_SCALE)
  # the summed loss: the rows' own errors, then at most T N + 8 adds and one product, each
  # within 2^-24 of a partial sum no larger than sum |rows|
  m_sum = CE_SCALE * (m_loss.sum() + (T * N + 9) * np.abs(loss).sum())
  return ref, dict(loss=m_loss, grad=m_grad, loss_sum=m_sum, valid=roww != 0)


def ce_constants(got, ref, m):
  """the distances of a result in units of 2^-24 m: (loss rows, gradient, summed loss)"""
  def worst(d, mm):
    d, mm = np.asarray(d, dtype=np.float64), np.asarray(mm, dtype=np.float64)
    if (d[mm == 0] != 0).any():
      return float("inf")
    return float(np.max(np.where(mm > 0, d / np.where(mm > 0, mm, 1.0), 0.0)) / U32)
  return (worst(np.abs(got["loss"] - ref["loss"]), m["loss"]),
          worst(np.abs(got["grad"] - ref["grad"]), np.broadcast_to(m["grad"][..., None],
                                                                   ref["grad"].shape)),
          worst(abs(float(got["loss_sum"]) - ref["loss_sum"]), m["loss_sum"]))


# The float32 torch oracle's constants (torch.float32 log_softmax / softmax on the CPU against
# ce_ref), measured by tests/test_train_helper_cases_host.py as the largest over every case of a
# kind and rounded up to a tenth; a constant below 1 counts as 1.  Measured:
#   ce       loss rows 1.178  gradient 1.938  summed loss 0.087
#   ce_len   loss rows 2.352  gradient 2.399  summed loss 0.095
#   ce_soft  loss rows 1.614  gradient 1.778  summed loss 0.127
# The GPU's bar is CE_GPU_FACTOR x these.  GPU_MEASURED: the distances of an MI355X in the same
# units, as tests/test_gpu_train_helpers.py prints them.
#                       loss rows   gradient   summed loss
CE_ORACLE_C = {
    "ce":      (1.2, 2.0, 1.0),
    "ce_len":  (2.4, 2.5, 1.0),
    "ce_soft": (1.7, 1.8, 1.0),
}
GPU_MEASURED = {
    "ce":      (1.020, 1.938, 0.094),
    "ce_len":  (1.373, 2.399, 0.095),
    "ce_soft": (1.366, 1.778, 0.114),
}


def ce_bars(c):
  return tuple(CE_GPU_FACTOR * max(1.0, v) for v in CE_ORACLE_C[c["kind"]])


def compare_ce(c, got, ref, m):
  """|got - ref64| <= c 2^-24 m per loss row, gradient element and summed loss; an invalid row
  (pred_lens) is exactly 0.0; the gradient rows of a hard-label case sum to 0 within
  K 2^-24 scale.  -> (mismatches, the constants)"""
  bad = []
  cs = ce_constants(got, ref, m)
  for what, v, bar in zip(("loss rows", "gradient", "summed loss"), cs, ce_bars(c)):
    if not v <= bar:
      bad.append("%s: %.3g x 2^-24 m, bar %.3g" % (what, v, bar))
  dead = ~m["valid"]
  if (np.asarray(got["loss"])[dead] != 0).any() or (np.asarray(got["grad"])[dead] != 0).any():
    bad.append("an invalid row is not exactly 0.0")
  if "soft_sum" not in c:
    rs = np.abs(np.asarray(got["grad"], dtype=np.float64).sum(axis=-1))
    lim = c["K"] * U32 * m["grad"]
    if (rs > lim).any():
      bad.append("a hard-label gradient row sums to %.3g (bar K 2^-24 scale = %.3g)"
                 % (float(rs.max()), float(lim.max())))
  return bad, cs


# =================================================================== device models (float32)
# Switches that make a model wrong the way a kernel could be; the host test shows that each one
# fails at least one named case of every family it applies to.
MUTATIONS = {
    "tap_mirror_x": ("small_dgrad", "small_wgrad", "scene", "onehot_wgrad"),
    "tap_mirror_y": ("small_dgrad", "small_wgrad", "scene", "onehot_wgrad"),
    "edge_dropped_at_block_seam": ("small_wgrad",),
    "edge_dropped_at_image_seam": ("small_wgrad",),
    "pad_t_zero": ("scene",),
    "parity_test_dropped": ("scene",),
    "accumulate_ignored": ("small_dgrad", "scene", "onehot_wgrad"),
    "last_partial_slab_dropped": ("colsum",),
    "fold_row_33_dropped": ("colsum",),
    "chunk_tail_skipped": ("long_sum",),
    "huber_clamp_strict": ("huber",),
    "masked_mean_by_count": ("huber",),
    "soft_labels_normalised": ("ce",),
    "pred_lens_le": ("huber", "ce"),
    "labels_time_major": ("ce", "onehot_wgrad"),
}
F32 = np.float32


def _flat_cells(M, H, W):
  m = np.arange(M * H * W)
  cell = m % (H * W)
  return m, cell // W, cell % W


def model_small_dgrad(c, dout, w, din, fault=None):
  """conv3x3_small_dgrad*_kernel: one thread per (cell, ci); tap t reads dout at
  (y - (t / 3 - 1), x - (t % 3 - 1)) when inside"""
  M, H, W, Ci, Co = c["M"], c["H"], c["W"], c["Ci"], c["Co"]
  n_o, n_i = H * W * Co, H * W * Ci
  d = dout[:, :n_o].astype(F32).reshape(M * H * W, Co)
  w32 = w.astype(F32).reshape(9, Ci, Co)
  m, y, x = _flat_cells(M, H, W)
  acc = np.zeros((M * H * W, Ci), dtype=F32)
  for t in range(9):
    dy, dx = t // 3 - 1, t % 3 - 1
    if fault == "tap_mirror_x":
      dx = -dx
    if fault == "tap_mirror_y":
      dy = -dy
    sy, sx = y - dy, x - dx
    ok = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
    src = m[ok] - dy * W - dx
    acc[ok] += d[src] @ w32[t].T
  out = din.astype(F32).copy()
  acc = acc.reshape(M, n_i)
  if c["accumulate"] and fault != "accumulate_ignored":
    out[:, :n_i] = out[:, :n_i] + acc
  else:
    out[:, :n_i] = acc
  return out


def model_small_wgrad(x, dout, cpb, fault=None):
  """conv3x3_small_wgrad_kernel<false>: a block of cpb flat cells; tap t of cell m reads
  in[m + (t / 3 - 1) W + (t % 3 - 1)] when (y, x) + tap is inside the image"""
  R, H, W, Ci = x.shape
  Co = dout.shape[3]
  total = R * H * W
  xi = x.astype(F32).reshape(total, Ci)
  d = dout.astype(F32).reshape(total, Co)
  m, y, xx = _flat_cells(R, H, W)
  cell = m % (H * W)
  dw = np.zeros((9, Ci, Co), dtype=F32)
  for t in range(9):
    dy, dx = t // 3 - 1, t % 3 - 1
    if fault == "tap_mirror_x":
      dx = -dx
    if fault == "tap_mirror_y":
      dy = -dy
    ok = (y + dy >= 0) & (y + dy < H) & (xx + dx >= 0) & (xx + dx < W)
    src = m + dy * W + dx
    flat_ok = (src >= 0) & (src < total)
    if fault == "edge_dropped_at_block_seam":
      seam = (m % cpb == 0) | (m % cpb == cpb - 1)
      ok = np.where(seam, flat_ok, ok)
    if fault == "edge_dropped_at_image_seam":
      seam = (cell == 0) | (cell == H * W - 1)
      ok = np.where(seam, flat_ok, ok)
    dw[t] = xi[src[ok]].T @ d[ok]
  return dw.reshape(3, 3, Ci, Co)


def model_scene_bwd(c, x, y, dy, w, init, fault=None):
  """tanh_bwd_kernel, conv_s2_dgrad_kernel (ty = iy + pad_t - ky: skipped when negative or odd,
  oy = ty / 2 < Ho), conv_s2_wgrad_kernel, the bias column sum"""
  U, Hi, Wi, Ci, Co, k = c["shape"]
  (Ho, pt), (Wo, pl) = same_pad(Hi, k), same_pad(Wi, k)
  if fault == "pad_t_zero":
    pt = 0
  act = ACT_CODE[c["act"]]
  y32, dy32 = y.astype(F32), dy.astype(F32)
  if act == 0:
    g = F32(1) - y32 * y32
  else:
    g = np.where(y32 > 0, F32(1), F32(0) if act == 1 else F32(0.2))
  dpre = (dy32 * g).astype(F32)
  w32, x32 = w.astype(F32), x.astype(F32)
  din = np.zeros((U, Hi, Wi, Ci), dtype=F32)
  dw = np.zeros((k, k, Ci, Co), dtype=F32)
  iy, ix = np.arange(Hi), np.arange(Wi)
  for ky in range(k):
    ty = iy + pt - (k - 1 - ky if fault == "tap_mirror_y" else ky)
    oky = (ty >= 0) & ((ty >> 1) < Ho)
    if fault != "parity_test_dropped":
      oky &= (ty & 1) == 0
    for kx in range(k):
      tx = ix + pl - (k - 1 - kx if fault == "tap_mirror_x" else kx)
      okx = (tx >= 0) & ((tx & 1) == 0) & ((tx >> 1) < Wo)
      if not (oky.any() and okx.any()):
        continue
      a, b = iy[oky][:, None], ix[okx][None, :]
      oa, ob = (ty[oky] >> 1)[:, None], (tx[okx] >> 1)[None, :]
      din[:, a, b, :] += dpre[:, oa, ob, :] @ w32[ky, kx].T
      dw[ky, kx] = np.einsum("uyxi,uyxo->io", x32[:, a, b, :], dpre[:, oa, ob, :])
  if c["accumulate"] and fault != "accumulate_ignored":
    din = init.astype(F32) + din
  return dict(dpre=dpre, din=din, dw=dw, db=dpre.sum(axis=(0, 1, 2), dtype=F32))


def model_onehot_wgrad(dpre, labels, dw_init, accumulate, fault=None):
  """grid_emb_onehot_wgrad_kernel: tap (ky, kx) of row m = t N + n reads the cell
  hot - (ky - 1, kx - 1)"""
  T, N, H, W, E = dpre.shape
  d = dpre.astype(F32)
  dw = np.zeros((3, 3, E), dtype=F32)
  lab = labels.reshape(-1)
  for ky in range(3):
    for kx in range(3):
      dy = -(ky - 1) if fault == "tap_mirror_y" else ky - 1
      dx = -(kx - 1) if fault == "tap_mirror_x" else kx - 1
      for t in range(T):
        for n in range(N):
          hot = lab[t * N + n] if fault == "labels_time_major" else lab[n * T + t]
          yy, xx = hot // W - dy, hot % W - dx
          if 0 <= yy < H and 0 <= xx < W:
            dw[ky, kx] += d[t, n, yy, xx]
  if accumulate and fault != "accumulate_ignored":
    dw = dw_init.astype(F32) + dw
  return dw


def model_colsum(xi, fault=None):
  """run_colsum: slabs of rows, then folds of 32 partial rows until at most 32 are left"""
  rows, ncols = xi.shape
  x = xi.astype(F32) * F32(QD)
  nslab = max(1, min(1024, (rows + 63) // 64))
  rps = (rows + nslab - 1) // nslab
  nslab = (rows + rps - 1) // rps
  if fault == "last_partial_slab_dropped" and rows % rps:
    nslab -= 1
  part = np.stack([x[s * rps:min(rows, (s + 1) * rps)].sum(axis=0, dtype=F32)
                   for s in range(nslab)]) if nslab else np.zeros((1, ncols), dtype=F32)
  while part.shape[0] > 32:
    n = part.shape[0]
    m = n // 32 if fault == "fold_row_33_dropped" else (n + 31) // 32
    part = np.stack([part[s * 32:min(n, (s + 1) * 32)].sum(axis=0, dtype=F32) for s in range(m)])
  return part.sum(axis=0, dtype=F32)


def model_long_sum(x, scale, fault=None):
  """run_long_sum: up to 4 chunks in one workgroup, else a partial per chunk of 4096 first"""
  x = x.astype(F32)
  n = x.size
  if n <= 4 * LONG_SUM_CHUNK:
    return F32(x.sum(dtype=F32) * F32(scale))
  nblk = n // LONG_SUM_CHUNK if fault == "chunk_tail_skipped" else -(-n // LONG_SUM_CHUNK)
  part = np.array([x[b * LONG_SUM_CHUNK:(b + 1) * LONG_SUM_CHUNK].sum(dtype=F32)
                   for b in range(nblk)], dtype=F32)
  return F32(part.sum(dtype=F32) * F32(scale))


def model_huber(c, pred, target, fg, scale, fault=None):
  """huber_loss_kernel / _len / _masked: q = min(|e|, 1), loss 0.5 q^2 + (|e| - q), gradient
  clamp(e, -1, 1) * scale"""
  T, N, K = c["T"], c["N"], c["K"]
  e = pred.astype(F32) - target.transpose(1, 0, 2, 3).astype(F32)
  a = np.abs(e)
  q = np.minimum(a, F32(1))
  loss = F32(0.5) * q * q + (a - q)
  clip = np.clip(e, F32(-1), F32(1))
  if fault == "huber_clamp_strict":     # two strict comparisons: |e| == 1 falls through both
    loss = np.where(a == 1, F32(0), loss)
    clip = np.where(a == 1, F32(0), clip)
  if c["kind"] == "huber_masked":
    on = (fg.astype(F32) > 0)[..., None]
    cnt = int((fg > 0).sum())
    den = F32(cnt) if fault == "masked_mean_by_count" else F32(2) * F32(cnt)
    s = F32(scale) / den if cnt else F32(0)
    loss = np.where(on, loss, F32(0))
    grad = np.where(on, clip * s, F32(0))
    total = (loss.sum(dtype=F32) / den * F32(scale)) if cnt else F32(0)
    return dict(loss=loss, grad=grad, loss_sum=F32(total), count=cnt)
  if c["kind"] == "huber_len":
    lens = np.array(c["pred_lens"])[None, :]
    t = np.arange(T)[:, None]
    valid = (t <= lens if fault == "pred_lens_le" else t < lens)[..., None, None]
    loss = np.where(valid, loss, F32(0))
    clip = np.where(valid, clip, F32(0))
  return dict(loss=loss, grad=clip * F32(scale), loss_sum=F32(loss.sum(dtype=F32) * F32(scale)))


def model_ce(c, z, labels, soft, fault=None):
  """ce_loss_kernel / ce_soft_loss_kernel / ce_loss_len_kernel / scale_rows_kernel in float32"""
  T, N, K = c["T"], c["N"], c["K"]
  p = z.astype(F32)
  mx = p.max(axis=-1, keepdims=True)
  ex = np.exp(p - mx)
  s = ex.sum(axis=-1, keepdims=True, dtype=F32)
  sm = ex * (F32(1) / s)
  scale = F32(CE_SCALE)
  if soft is not None:
    q = soft.astype(F32)
    loss = -(q * ((p - mx) - np.log(s))).sum(axis=-1, dtype=F32)
    if fault == "soft_labels_normalised":
      q = q / q.sum(axis=-1, keepdims=True, dtype=F32)
    grad = (sm - q) * scale
  else:
    lab = (labels.reshape(T, N) if fault == "labels_time_major" else labels.T).astype(np.int64)
    zl = np.take_along_axis(p, lab[..., None], axis=-1)[..., 0]
    loss = (np.log(s) + mx)[..., 0] - zl
    hot = np.zeros_like(p)
    np.put_along_axis(hot, lab[..., None], F32(1), axis=-1)
    grad = (sm - hot) * scale
  if "pred_lens" in c:
    lens = np.array(c["pred_lens"])[None, :]
    t = np.arange(T)[:, None]
    valid = t <= lens if fault == "pred_lens_le" else t < lens
    loss = np.where(valid, loss, F32(0))
    grad = np.where(valid[..., None], grad, F32(0))
  if "sample_w" in c:
    sw = np.array(c["sample_w"], dtype=F32)[None, :]
    loss, grad = loss * sw, grad * sw[..., None]
  return dict(loss=loss.astype(F32), grad=grad.astype(F32),
              loss_sum=F32(loss.sum(dtype=F32) * scale))
