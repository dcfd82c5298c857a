# coding=utf-8
"""The decoder tail of a step -- hidden2grid, argmax, the next step's input embedding and its
operand planes -- through the single-call door mv_op_decode_tail (csrc/engine_ops.h), in both of
its forms: grouped (pack_h2g_kernel, ONE h2g_q launch, ONE decode_tail launch for up to four
chains, csrc/decode_tail.h) and separate (hidden2grid_kernel, argmax_rows_kernel, grid_emb_*,
csrc/kernels_misc.h).  The reference is fp64 numpy written out below: a SAME 3x3 convolution,
np.argmax (first maximum), act(conv3x3(one_hot or map) + b), and the plane split; plane_index
is restated from csrc/plane_layout.h.

Two data sets.  FLOAT: h = tanh(normal), hidden2grid weights 0.05 * normal (the scaling of
test_hidden2grid), embedding weights normal / sqrt(9 P), bias 0.1 * normal.  EXACT: h in
multiples of 1/4 within [-1, 1], hidden2grid weights in multiples of 1/8 within [-1, 1],
embedding weights in multiples of 1/8: every partial sum of the hidden2grid is a multiple of
1/32 below 9 * 512 = 4608, exact in fp32 in any order and under fmaf (4608 * 32 < 2^24), so the
output rows of both forms equal the fp64 reference bit for bit and ties can be planted.

Bars on float data.  Output rows 2e-5 absolute, the bar test_hidden2grid sets for these sums at
this scaling.  Embedding 1e-5 absolute against fp64: at most 18 products of size about 1, so at
most 19 roundings of 2^-24 on a pre-activation of size up to about 3 (3.4e-6), the three
activations are 1-Lipschitz, tanhf adds a few ulp (< 4e-7); a dropped or misplaced tap moves the
result by about 0.3.  Argmax: the reference's best and second-best logit of every class row
differ by more than 2e-4, ten times the logit bar -- asserted, a precondition of the seeds."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OUT_TOL = 2e-5
EMB_TOL = 1e-5
ARGMAX_GAP = 2e-4
FORMS = (False, True)                 # grouped, separate
FORM_IDS = ("grouped", "separate")


# ------------------------------------------------------------------ the fp64 reference

def _conv3(x, w):
  """SAME 3x3 convolution in fp64: x [M, H, W, Ci], w [3, 3, Ci, Co]."""
  M, H, W, Ci = x.shape
  xp = np.zeros((M, H + 2, W + 2, Ci))
  xp[:, 1:-1, 1:-1] = x
  out = np.zeros((M, H, W, w.shape[3]))
  for ky in range(3):
    for kx in range(3):
      out += xp[:, ky:ky + H, kx:kx + W] @ w[ky, kx].astype(np.float64)
  return out


def _act(v, act):
  if act == 0:
    return np.tanh(v)
  return np.where(v > 0, v, 0.0 if act == 1 else 0.2 * v)


def _ref_tail(ch, act=0):
  """out [rows, K, P], ids [rows] (class chain, else None), x [rows * K, E], all fp64."""
  h = ch["h"].astype(np.float64)
  rows, H, W, _ = h.shape
  K = H * W
  out = _conv3(h, ch["w_out"])
  ids = None
  if ch["kind"] == "cls":
    ids = out.reshape(rows, K).argmax(1)
    m = np.zeros((rows, K, 1))
    m[np.arange(rows), ids, 0] = 1.0
    m = m.reshape(rows, H, W, 1)
  else:
    m = out
  x = _act(_conv3(m, ch["emb_w"]) + ch["emb_b"].astype(np.float64), act)
  return out.reshape(rows, K, -1), ids, x.reshape(rows * K, -1)


def _plane_index(m, c, C):
  """csrc/plane_layout.h plane_index: tile (m >> 5, c >> 4) of 32 cells x 16 channels, stored
  [k half][cell & 31][8 channels]."""
  return ((m >> 5) * (C >> 4) + (c >> 4)) * 512 + ((c >> 3) & 1) * 256 + (m & 31) * 8 + (c & 7)


def _bits(a):
  a = np.ascontiguousarray(a)
  return a.view({4: np.uint32, 2: np.uint16}[a.dtype.itemsize])


def _same_bits(a, b):
  return a.shape == b.shape and a.dtype == b.dtype and bool((_bits(a) == _bits(b)).all())


def _expected_planes(built_lib, x, mode):
  """The whole raw plane buffer the call must hand back for the RETURNED x [M, E]: the split
  in numpy float32 / float16 at plane_index, the sentinel everywhere else."""
  M, E = x.shape
  sent = np.uint16(built_lib.OP_SENTINEL_BYTE * 0x0101)
  exp = np.full(built_lib.plane_buffer_elems(M, E), sent, dtype=np.uint16)
  m, c = np.meshgrid(np.arange(M, dtype=np.int64), np.arange(E, dtype=np.int64), indexing="ij")
  idx = built_lib.PLANE_PAD + _plane_index(m, c, E)
  half = exp.size // 2
  assert np.unique(idx).size == idx.size and idx.max() < half        # an injective image
  if mode == "bf16":            # round-to-nearest-even upper half of x's bits
    u = _bits(x).astype(np.uint64)
    finite = (u & 0x7f800000) != 0x7f800000
    u = np.where(finite, u + 0x7fff + ((u >> 16) & 1), u)
    exp[idx] = (u >> 16).astype(np.uint16)
    return exp
  s = x * np.float32(256.0)
  h0 = s.astype(np.float16)
  h1 = (s - h0.astype(np.float32)).astype(np.float16)
  exp[idx] = _bits(h0)
  exp[half + idx] = _bits(h1)
  return exp


def _untouched(built_lib, a):
  b = a.view(np.uint8)
  return bool((b == built_lib.OP_SENTINEL_BYTE).all())


# ------------------------------------------------------------------ the data

def _seed(*key):
  s = 20261
  for k in key:
    s = (s * 1000003 + int(k)) % (2 ** 31 - 1)
  return s


@functools.lru_cache(maxsize=None)
def _float_chain_cached(kind, rows, H, W, C, E, salt):
  rng = np.random.default_rng(_seed(kind == "cls", rows, H, W, C, E, salt))
  P = 1 if kind == "cls" else 2
  ch = {"kind": kind,
        "h": np.tanh(rng.standard_normal((rows, H, W, C))).astype(np.float32),
        "w_out": (0.05 * rng.standard_normal((3, 3, C, P))).astype(np.float32),
        "emb_w": (rng.standard_normal((3, 3, P, E)) / np.sqrt(9 * P)).astype(np.float32),
        "emb_b": (0.1 * rng.standard_normal(E)).astype(np.float32)}
  for k, v in ch.items():
    if k != "kind":
      v.setflags(write=False)
  return ch


def _float_chain(kind, rows, H, W, C=256, E=32, salt=0):
  return dict(_float_chain_cached(kind, rows, H, W, C, E, salt))


@functools.lru_cache(maxsize=None)
def _ref_cached(kind, rows, H, W, C, E, salt, act):
  return _ref_tail(_float_chain_cached(kind, rows, H, W, C, E, salt), act)


def _exact_chain(kind, rows, H, W, C=256, E=32, salt=0):
  rng = np.random.default_rng(_seed(7, kind == "cls", rows, H, W, C, E, salt))
  P = 1 if kind == "cls" else 2
  return {"kind": kind,
          "h": (rng.integers(-4, 5, size=(rows, H, W, C)) / 4).astype(np.float32),
          "w_out": (rng.integers(-8, 9, size=(3, 3, C, P)) / 8).astype(np.float32),
          "emb_w": (rng.integers(-8, 9, size=(3, 3, P, E)) / 8).astype(np.float32),
          "emb_b": (rng.integers(-4, 5, size=E) / 8).astype(np.float32)}


def _rows_of(ch, lo, hi=None):
  c = dict(ch)
  c["h"] = np.ascontiguousarray(ch["h"][lo:hi])
  return c


def _gap_precondition(ref_out):
  """Best and second-best logit of every class row of the REFERENCE more than 2e-4 apart."""
  if ref_out.shape[1] < 2:
    return
  top = np.sort(ref_out[:, :, 0], axis=1)[:, -2:]
  gap = top[:, 1] - top[:, 0]
  assert (gap > ARGMAX_GAP).all(), ("seed precondition: a near-tie in the reference", gap)


def _check_float(res, ch, ref, tag, emb_tol=EMB_TOL):
  ro, ri, rx = ref
  do = float(np.abs(res["out"] - ro).max())
  dx = float(np.abs(res["x"] - rx).max())
  print("%s %s: max|d out| %.3g  max|d x| %.3g" % (tag, ch["kind"], do, dx))
  assert res["out"].shape == ro.shape and res["x"].shape == rx.shape
  assert do <= OUT_TOL, (tag, ch["kind"], do)
  if ch["kind"] == "cls":
    _gap_precondition(ro)
    assert (res["ids"] == ri).all(), (tag, res["ids"], ri)
  assert dx <= emb_tol, (tag, ch["kind"], dx)


# ------------------------------------------------------------------ a. shapes against fp64

SHAPES = [(1, 1, 1),       # every tap but the centre is outside the image
          (3, 1, 7), (2, 5, 1),
          (5, 3, 5),       # 75 cells: a partial wave tile and a partial block
          (1, 9, 16),      # 144 cells: a second block with one half-filled wave
          (2, 18, 9),      # W divides nothing
          (1, 32, 32)]     # K = 1024: the LDS bound, one cell per thread


@pytest.mark.parametrize("separate", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_shapes_against_fp64(built_lib, shape, separate):
  chains = [_float_chain("cls", *shape), _float_chain("reg", *shape)]
  res = built_lib.op_decode_tail(chains, separate=separate)
  for ch, r in zip(chains, res):
    _check_float(r, ch, _ref_cached(ch["kind"], *shape, 256, 32, 0, 0), str(shape))


@pytest.mark.parametrize("separate", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("act", [1, 2], ids=["relu", "lrelu"])
def test_relu_and_lrelu_against_fp64(built_lib, act, separate):
  shape = (5, 3, 5)
  chains = [_float_chain("cls", *shape), _float_chain("reg", *shape)]
  res = built_lib.op_decode_tail(chains, act=act, separate=separate)
  for ch, r in zip(chains, res):
    _check_float(r, ch, _ref_cached(ch["kind"], *shape, 256, 32, 0, act), "act %d" % act)


def test_a_grid_of_1025_cells_is_refused_by_the_grouped_form(built_lib):
  """Host side: the LDS row buffer holds K * 2 <= 2048 values; nothing is launched."""
  chains = [_float_chain("cls", 1, 25, 41), _float_chain("reg", 1, 25, 41)]
  with pytest.raises(built_lib.MvError, match="decode tail: K 1025"):
    built_lib.op_decode_tail(chains)
  with pytest.raises(built_lib.MvError, match="decode tail: K 1025"):
    built_lib.op_decode_tail(chains[1:], next="none")


# ------------------------------------------------------------------ b. channel and embedding widths

@pytest.mark.parametrize("separate", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("C,E,shape", [(128, 32, (2, 3, 5)),     # the NK = 16 instance of h2g_q
                                       (512, 32, (2, 3, 5)),     # its dynamic LDS is exactly 64 KB
                                       (256, 64, (1, 2, 3)),
                                       (256, 512, (1, 2, 3))])   # the tail's largest LDS
def test_channel_and_embedding_widths(built_lib, C, E, shape, separate):
  chains = [_float_chain("cls", *shape, C=C, E=E), _float_chain("reg", *shape, C=C, E=E)]
  res = built_lib.op_decode_tail(chains, separate=separate)
  for ch, r in zip(chains, res):
    _check_float(r, ch, _ref_cached(ch["kind"], *shape, C, E, 0, 0), "C %d E %d" % (C, E))


# ------------------------------------------------------------------ c. ties and extremes

def _twin_row(ch, H, W, a, b, rng):
  """A zero background with the same vector at two interior cells whose 3x3 neighbourhoods do
  not overlap: every output around the two repeats exactly, wherever the maximum falls."""
  C = ch["h"].shape[3]
  assert abs(a[0] - b[0]) >= 3 or abs(a[1] - b[1]) >= 3
  for p in (a, b):
    assert 1 <= p[0] < H - 1 and 1 <= p[1] < W - 1
  row = np.zeros((H, W, C), np.float32)
  v = (rng.integers(-4, 5, size=C) / 4).astype(np.float32)
  row[a] = v
  row[b] = v
  return row


def _lone_row(ch, H, W, cell):
  """One vector on a zero background, aligned with the centre tap: the lone maximum at `cell`."""
  C = ch["h"].shape[3]
  row = np.zeros((H * W, C), np.float32)
  row[cell] = np.sign(ch["w_out"][1, 1, :, 0])
  return row.reshape(H, W, C)


def _ids_of_both_forms(built_lib, ch):
  ref_out, ref_ids, _ = _ref_tail(ch)
  for separate in FORMS:
    for nxt in ("ids", "embed"):
      r = built_lib.op_decode_tail([ch], next=nxt, separate=separate)[0]
      assert _same_bits(r["out"], ref_out.astype(np.float32)), (separate, nxt)
      assert (r["ids"] == ref_ids).all(), (separate, nxt, r["ids"], ref_ids)
  return ref_out[:, :, 0], ref_ids


def _attained_at(row):
  return np.nonzero(row == row.max())[0]


@pytest.mark.parametrize("C", [128, 256, 512])
def test_tie_across_waves(built_lib, C):
  """Twins at (1, 2) and (6, 12) of 9 x 16: the maximum at exactly two cells, 90 apart, so in
  different waves of the tail's workgroup (cell i is thread i's)."""
  H, W = 9, 16
  ch = _exact_chain("cls", 2, H, W, C=C)
  ch["h"][1] = _twin_row(ch, H, W, (1, 2), (6, 12), np.random.default_rng(C))
  ref = _conv3(ch["h"].astype(np.float64), ch["w_out"]).reshape(2, -1)
  at = _attained_at(ref[1])
  assert at.size == 2 and at[1] - at[0] == 90 and (at[0] >> 6) != (at[1] >> 6), at
  assert _attained_at(ref[0]).size == 1
  _, ids = _ids_of_both_forms(built_lib, ch)
  assert ids[1] == at[0]


def test_tie_within_one_wave(built_lib):
  H, W = 4, 16
  ch = _exact_chain("cls", 1, H, W)
  ch["h"][0] = _twin_row(ch, H, W, (1, 2), (1, 7), np.random.default_rng(3))
  ref = _conv3(ch["h"].astype(np.float64), ch["w_out"]).reshape(-1)
  at = _attained_at(ref)
  assert at.size == 2 and at[1] - at[0] == 5 and at[1] < 64, at
  _, ids = _ids_of_both_forms(built_lib, ch)
  assert ids[0] == at[0]


def test_all_zero_lone_maxima_and_a_tie_in_a_late_row(built_lib):
  """Rows of one call: all zero (every cell ties, the answer is 0); a lone maximum at cell 0 and
  at cell K - 1; then untied, untied, tied -- a tie in row 2 of 3 does not leak into another."""
  H, W = 9, 16
  K = H * W
  ch = _exact_chain("cls", 6, H, W)
  ch["h"][0] = 0
  ch["h"][1] = _lone_row(ch, H, W, 0)
  ch["h"][2] = _lone_row(ch, H, W, K - 1)
  ch["h"][5] = _twin_row(ch, H, W, (1, 2), (6, 12), np.random.default_rng(11))
  ref = _conv3(ch["h"].astype(np.float64), ch["w_out"]).reshape(6, K)
  assert (ref[0] == 0).all()
  assert list(_attained_at(ref[1])) == [0] and list(_attained_at(ref[2])) == [K - 1]
  assert _attained_at(ref[3]).size == 1 and _attained_at(ref[4]).size == 1
  at = _attained_at(ref[5])
  assert at.size == 2 and at[1] - at[0] == 90, at
  _, ids = _ids_of_both_forms(built_lib, ch)
  assert list(ids[:3]) == [0, 0, K - 1] and ids[5] == at[0]
  # the late rows alone: rows 3 .. 5 are a call of three rows with the tie in row 2
  late = _rows_of(ch, 3)
  _, ids3 = _ids_of_both_forms(built_lib, late)
  assert (ids3 == ids[3:]).all()


def test_a_row_of_negative_logits(built_lib):
  """Non-negative weights under a strictly negative h: every logit is below zero."""
  H, W = 5, 7
  ch = _exact_chain("cls", 2, H, W)
  ch["w_out"] = np.abs(ch["w_out"])
  ch["h"] = -np.abs(ch["h"]) - np.float32(0.25)
  ch["h"] = np.maximum(ch["h"], np.float32(-1.0))
  ref = _conv3(ch["h"].astype(np.float64), ch["w_out"])
  assert ref.max() < 0
  _ids_of_both_forms(built_lib, ch)


# ------------------------------------------------------------------ d. one launch, several chains

def _assert_same_result(a, b, tag):
  assert a.keys() == b.keys(), tag
  for k in a:
    assert _same_bits(a[k], b[k]), (tag, k)


def test_four_chains_in_one_launch_equal_each_chain_alone(built_lib):
  chains = [_float_chain("cls", 3, 9, 16), _float_chain("reg", 3, 9, 16),
            _float_chain("cls", 2, 5, 7), _float_chain("reg", 2, 5, 7)]
  for planes in (None, "f16x3"):
    together = built_lib.op_decode_tail(chains, planes=planes)
    for i, ch in enumerate(chains):
      alone = built_lib.op_decode_tail([ch], planes=planes)[0]
      _assert_same_result(together[i], alone, (planes, i))
  # every order of the block_end dispatch: the same chains reversed
  back = built_lib.op_decode_tail(chains[::-1])[::-1]
  for i, r in enumerate(built_lib.op_decode_tail(chains)):
    _assert_same_result(back[i], r, ("reversed", i))
  for ch, r in zip(chains, back):
    rows, H, W, _ = ch["h"].shape
    _check_float(r, ch, _ref_cached(ch["kind"], rows, H, W, 256, 32, 0, 0), "four chains")


def test_chains_of_different_row_counts(built_lib):
  """A class chain with 6 rows beside a regression chain with 2: the beam step's launch."""
  chains = [_float_chain("cls", 6, 9, 16), _float_chain("reg", 2, 9, 16)]
  for nxt in ("none", "embed"):
    together = built_lib.op_decode_tail(chains, next=nxt)
    for i, ch in enumerate(chains):
      _assert_same_result(together[i], built_lib.op_decode_tail([ch], next=nxt)[0], (nxt, i))
  for ch, r in zip(chains, together):
    rows = ch["h"].shape[0]
    _check_float(r, ch, _ref_cached(ch["kind"], rows, 9, 16, 256, 32, 0, 0), "6 + 2 rows")


# ------------------------------------------------------------------ e. position independence

@pytest.mark.parametrize("separate", FORMS, ids=FORM_IDS)
def test_rows_do_not_depend_on_where_they_sit(built_lib, separate):
  """5 x 7 (K = 35: the 32-cell tiles of h2g_q straddle rows): rows [lo:] of a call give the
  bits those rows had in the full call."""
  H, W, K = 5, 7, 35
  chains = [_float_chain("cls", 4, H, W), _float_chain("reg", 4, H, W)]
  full = built_lib.op_decode_tail(chains, separate=separate)
  for lo in (1, 2):
    part = built_lib.op_decode_tail([_rows_of(c, lo) for c in chains], separate=separate)
    for f, p in zip(full, part):
      assert _same_bits(p["out"], f["out"][lo:]), lo
      assert _same_bits(p["x"], f["x"][lo * K:]), lo
      if "ids" in f:
        assert (p["ids"] == f["ids"][lo:]).all(), lo


# ------------------------------------------------------------------ f. forms

def test_forms_agree_on_float_data(built_lib):
  chains = [_float_chain("cls", 3, 9, 16), _float_chain("reg", 3, 9, 16)]
  g = built_lib.op_decode_tail(chains)
  s = built_lib.op_decode_tail(chains, separate=True)
  for a, b in zip(g, s):
    assert np.abs(a["out"] - b["out"]).max() <= OUT_TOL
  _gap_precondition(_ref_cached("cls", 3, 9, 16, 256, 32, 0, 0)[0])
  assert (g[0]["ids"] == s[0]["ids"]).all()


@pytest.mark.parametrize("act", [0, 2], ids=["tanh", "lrelu"])
@pytest.mark.parametrize("C", [128, 256, 512])
def test_forms_are_bit_equal_on_exact_data(built_lib, C, act):
  """Exact data: the output rows of both forms are the fp64 reference's bits, hence the tail's
  regression embedding ("same accumulation order as grid_emb_dense_kernel") is bit-equal to
  grid_emb_dense_kernel's, and the class embedding to grid_emb_onehot_kernel's."""
  chains = [_exact_chain("cls", 3, 5, 7, C=C), _exact_chain("reg", 3, 5, 7, C=C)]
  g = built_lib.op_decode_tail(chains, act=act)
  s = built_lib.op_decode_tail(chains, act=act, separate=True)
  for ch, a, b in zip(chains, g, s):
    ro, ri, rx = _ref_tail(ch, act)
    assert np.abs(ro).max() < 4608 and (ro * 32 == np.round(ro * 32)).all()
    assert _same_bits(a["out"], ro.astype(np.float32)), ch["kind"]
    assert _same_bits(b["out"], ro.astype(np.float32)), ch["kind"]
    if ri is not None:
      assert (a["ids"] == ri).all() and (b["ids"] == ri).all()
    assert _same_bits(a["x"], b["x"]), ch["kind"]
    # the pre-activation of exact data is exact as well: multiples of 1/256 (1/8 for the class
    # chain) whose partial sums stay below 2^24 / 256, so only the activation rounds -- 0.2f * v
    # once, tanhf a few ulp: orders below 1e-5 of the value
    assert 18 * np.abs(ro).max() * np.abs(ch["emb_w"]).max() + 1 < 2 ** 16
    assert (np.abs(a["x"] - rx) <= EMB_TOL * np.maximum(1.0, np.abs(rx))).all()


@pytest.mark.parametrize("act", [0, 1, 2], ids=["tanh", "relu", "lrelu"])
def test_the_closed_form_one_hot_embedding_four_ways(built_lib, act):
  """The hot cell at the four corners, on an edge and in the interior of 5 x 7: the tail,
  grid_emb_onehot8_kernel, grid_emb_onehot_kernel and grid_emb_dense_kernel fed the literal
  one-hot map with the class weights give the same bits."""
  H, W = 5, 7
  hot = [0, W - 1, (H - 1) * W, H * W - 1, 3, 2 * W + 3]
  for data in ("exact", "float"):
    ch = _exact_chain("cls", len(hot), H, W, E=64) if data == "exact" else \
        dict(_float_chain("cls", len(hot), H, W, E=64))
    ch["h"] = np.stack([_lone_row(ch, H, W, c) for c in hot])
    ref_out, ref_ids, ref_x = _ref_tail(ch, act)
    assert list(ref_ids) == hot
    _gap_precondition(ref_out)
    got = [built_lib.op_decode_tail([ch], act=act, separate=f)[0]
           for f in (False, True, "onehot8", "dense")]
    for r in got:
      assert list(r["ids"]) == hot, data
      assert np.abs(r["x"] - ref_x).max() <= EMB_TOL
      assert _same_bits(r["x"], got[0]["x"]), data


# ------------------------------------------------------------------ g. planes

@pytest.mark.parametrize("mode", ["f16x3", "bf16"])
@pytest.mark.parametrize("E", [32, 64])
@pytest.mark.parametrize("shape", [(5, 3, 5),        # the last 32-cell tile is partial
                                   (2, 9, 16)], ids=lambda s: "%dx%dx%d" % s)
def test_planes_land_where_plane_index_puts_them(built_lib, shape, E, mode):
  """emb_store8's 16-byte stores (grouped) and emit_planes (separate): at plane_index(m, c, E)
  the split of the RETURNED x, bitwise; every other half of the buffer still the sentinel."""
  chains = [_float_chain("cls", *shape, E=E), _float_chain("reg", *shape, E=E)]
  for separate in (False, True, "onehot8"):
    res = built_lib.op_decode_tail(chains, planes=mode, separate=separate)
    for ch, r in zip(chains, res):
      exp = _expected_planes(built_lib, r["x"], mode)
      bad = np.nonzero(r["planes"] != exp)[0]
      assert bad.size == 0, (separate, ch["kind"], bad[:8], r["planes"][bad[:8]], exp[bad[:8]])
      _check_float(r, ch, _ref_cached(ch["kind"], *shape, 256, E, 0, 0), "planes %s" % mode)


@pytest.mark.parametrize("mode", ["f16x3", "bf16"])
def test_planes_of_both_forms_are_bit_equal_on_exact_data(built_lib, mode):
  shape = (5, 3, 5)
  chains = [_exact_chain("cls", *shape), _exact_chain("reg", *shape)]
  g = built_lib.op_decode_tail(chains, act=2, planes=mode)
  s = built_lib.op_decode_tail(chains, act=2, planes=mode, separate=True)
  for a, b in zip(g, s):
    assert _same_bits(a["x"], b["x"])
    assert (a["planes"] == _expected_planes(built_lib, a["x"], mode)).all()
    assert (a["planes"] == b["planes"]).all()


# ------------------------------------------------------------------ h. optional outputs

@pytest.mark.parametrize("separate", FORMS, ids=FORM_IDS)
def test_optional_outputs_stay_untouched(built_lib, separate):
  shape = (3, 5, 7)
  chains = [_float_chain("cls", *shape), _float_chain("reg", *shape)]
  full = built_lib.op_decode_tail(chains, planes="f16x3", separate=separate)
  none = built_lib.op_decode_tail(chains, next="none", planes="f16x3", separate=separate)
  only = built_lib.op_decode_tail(chains, next="ids", planes="f16x3", separate=separate)
  for f, n, o in zip(full, none, only):
    assert _same_bits(n["out"], f["out"]) and _same_bits(o["out"], f["out"])
    assert _untouched(built_lib, n["x"]) and _untouched(built_lib, o["x"])
    assert _untouched(built_lib, n["planes"]) and _untouched(built_lib, o["planes"])
    assert not _untouched(built_lib, f["x"])
    if "ids" in f:
      assert _untouched(built_lib, n["ids"])
      assert (o["ids"] == f["ids"]).all() and not _untouched(built_lib, o["ids"])
