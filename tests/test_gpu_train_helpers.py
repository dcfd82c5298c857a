# coding=utf-8
"""GPU: the helper kernels of a training step, ONE at a time, through the single-kernel doors
mv_op_small_conv_dgrad / _wgrad, mv_op_colsum, mv_op_long_sum, mv_op_scene_conv_bwd,
mv_op_grid_emb_onehot_wgrad and mv_op_train_loss (csrc/engine_ops.h).  The doors call the
launchers the engine calls (csrc/engine_train.h launch_*), so the kernel form, the launch
geometry and the folds are the engine's own.

Inputs, float64 references and bars: tests/train_helper_cases.py (its CPU checks:
tests/test_train_helper_cases_host.py).  Operands are small dyadic rationals: every partial sum
is a float32 in any order, so everything but the cross entropies is held with == (0.0 == -0.0)
against the float64 reference.  The cross entropies are held to 4 x the float32 torch oracle's own
distance from float64; their distances are printed next to the bars.

Cross-entropy distances on an MI355X, in units of 2^-24 m (loss rows / gradient / summed loss):
ce 1.02 / 1.94 / 0.09 (bars 4.8 / 8.0 / 4.0), ce_len 1.37 / 2.40 / 0.10 (9.6 / 10.0 / 4.0),
ce_soft 1.37 / 1.78 / 0.11 (6.8 / 7.2 / 4.0).  Every exact case: equal.

The forms that ran are asserted from what the doors report, against values written out from the
rules of engine_train.h in train_helper_cases.py (not asked of the planner)."""

import numpy as np
import pytest

import train_helper_cases as hc

pytestmark = pytest.mark.gpu


def _nonzero(a):
  return {tuple(int(v) for v in i) for i in np.argwhere(np.asarray(a) != 0)}


# ------------------------------------------------------------------ small 3x3 dgrad
@pytest.mark.parametrize("Ci,Co", hc.SMALL_DGRAD_CHANNELS)
def test_small_conv_dgrad_exact(built_lib, Ci, Co):
  for c in [c for c in hc.small_dgrad_cases() if (c["Ci"], c["Co"]) == (Ci, Co)]:
    dout, w, din = hc.small_dgrad_inputs(c)
    ref = hc.small_dgrad_ref(c, dout, w, din)[0]
    want = hc.small_dgrad_form_expected(Ci, Co, din.shape[1])
    got, form = built_lib.op_small_conv_dgrad(dout, w, din, c["H"], c["W"],
                                              accumulate=c["accumulate"])
    assert form == want, c["name"]
    # the whole buffer: what lies between the rows must come back untouched
    assert hc.compare_exact(dict(din=got), dict(din=ref)) == [], c["name"]
    forced = ["scalar"] + ([want] if want != "scalar" else [])
    for f in forced:
      g2, ran = built_lib.op_small_conv_dgrad(dout, w, din, c["H"], c["W"],
                                              accumulate=c["accumulate"], form=f)
      assert ran == f and np.array_equal(g2.view(np.int32), got.view(np.int32)), (c["name"], f)


def test_small_conv_dgrad_stride_cases_are_there():
  names = [c["name"] for c in hc.small_dgrad_cases()]
  assert "dgrad_256x2_5.2.7_odd_acc1" in names and "dgrad_2x32_5.2.7_slice_acc0" in names


@pytest.mark.parametrize("Ci,Co", [(256, 1), (256, 2), (12, 6), (16, 32)])
def test_small_conv_dgrad_onehot_every_tap(built_lib, Ci, Co):
  dout, w, cells = hc.small_dgrad_onehot(Ci, Co)
  M = len(hc.ONEHOT_POSITIONS)
  ref = hc.conv3x3_dgrad_ref(dout, w)
  assert _nonzero(ref) == cells
  got, _ = built_lib.op_small_conv_dgrad(dout.reshape(M, -1), w, np.zeros((M, ref[0].size)),
                                         hc.ONEHOT_H, hc.ONEHOT_W)
  got = got.reshape(ref.shape)
  assert _nonzero(got) == cells              # exactly the cells the taps name, nothing else
  assert hc.compare_exact(dict(din=got), dict(din=ref)) == []


def test_small_conv_dgrad_refuses_forms_the_shape_cannot_take(built_lib):
  dout, w, din = np.zeros((1, 6)), np.zeros((3, 3, 3, 6)), np.zeros((1, 3))
  for form in ("dgrad4<1>", "dgrad4<2>"):
    with pytest.raises(built_lib.MvError, match="form dgrad4<[12]> needs"):
      built_lib.op_small_conv_dgrad(dout, w, din, 1, 1, form=form)
  c = [c for c in hc.small_dgrad_cases() if c["name"] == "dgrad_256x2_5.2.7_odd_acc0"][0]
  dout, w, din = hc.small_dgrad_inputs(c)
  with pytest.raises(built_lib.MvError, match="row stride that is a multiple of 4"):
    built_lib.op_small_conv_dgrad(dout, w, din, 2, 7, form="dgrad4<2>")
  with pytest.raises(built_lib.MvError, match="form dgrad4<1> needs"):     # Co is 2
    built_lib.op_small_conv_dgrad(dout[:, :-2], w, din[:, :-2], 2, 7, form="dgrad4<1>")


# ------------------------------------------------------------------ small 3x3 wgrad
def _assert_taps(got, ref, what):
  for ky, kx in hc.TAPS:                     # every tap on its own
    bad = hc.compare_exact(dict(tap=got[ky, kx]), dict(tap=ref[ky, kx]))
    assert bad == [], (what, "tap", ky, kx, bad)


@pytest.mark.parametrize("Ci,Co", sorted(hc.SMALL_WGRAD_CHANNELS))
def test_small_conv_wgrad_exact_every_form(built_lib, Ci, Co):
  form, G = hc.SMALL_WGRAD_CHANNELS[(Ci, Co)]
  for (R, H, W) in hc.SMALL_WGRAD_SHAPES:
    x, d = hc.small_wgrad_inputs(R, H, W, Ci, Co)
    ref = hc.conv3x3_wgrad_ref(x, d)
    got, info = built_lib.op_small_conv_wgrad(x, d)
    blocks, cpb = hc.SMALL_WGRAD_BLOCKS[R * H * W]
    assert info == dict(form=form, blocks=blocks, cells_per_block=cpb, G=G), (R, H, W, info)
    _assert_taps(got, ref, (R, H, W))
    for f in hc.small_wgrad_forms_allowed(Ci, Co):
      g2, i2 = built_lib.op_small_conv_wgrad(x, d, form=f)
      assert i2["form"] == f and (i2["blocks"], i2["cells_per_block"]) == (blocks, cpb)
      assert np.array_equal(g2.view(np.int32), got.view(np.int32)), (R, H, W, f)


@pytest.mark.parametrize("Ci,Co", [(256, 2), (128, 1), (64, 2), (2, 32), (2, 128)])
@pytest.mark.parametrize("R,H,W", [(3, 5, 7), (5, 2, 7)])
def test_small_conv_wgrad_onehot_pairs_across_seams(built_lib, R, H, W, Ci, Co):
  """One-hot in x one-hot dout either side of an image seam and of a block seam: a kernel that
  carries a tap from the last cell of image r into the first of image r + 1 shows here."""
  x0, d0 = hc.small_wgrad_inputs(R, H, W, Ci, Co)
  cpb = built_lib.op_small_conv_wgrad(x0, d0)[1]["cells_per_block"]     # the seam the door reports
  assert cpb == hc.SMALL_WGRAD_BLOCKS[R * H * W][1]
  for seam, cells in (("image", (H * W - 1, H * W)), ("block", (cpb - 1, cpb))):
    for s in cells:
      x, d, nz = hc.small_wgrad_onehot(R, H, W, Ci, Co, s)
      ref = hc.conv3x3_wgrad_ref(x, d)
      assert _nonzero(ref) == nz and nz
      for f in [None] + hc.small_wgrad_forms_allowed(Ci, Co):
        got, _ = built_lib.op_small_conv_wgrad(x, d, form=f)
        assert _nonzero(got) == nz, (seam, s, f)
        _assert_taps(got, ref, (seam, s, f))


def test_small_conv_wgrad_refusals(built_lib):
  Ci, Co = hc.SMALL_WGRAD_REFUSED
  x, d = np.zeros((1, 2, 2, Ci)), np.zeros((1, 2, 2, Co))
  with pytest.raises(built_lib.MvError, match=r"small wgrad: Ci\*Co 1024 > 512"):
    built_lib.op_small_conv_wgrad(x, d)
  x, d = np.zeros((1, 2, 2, 512)), np.zeros((1, 2, 2, 2))
  for f in ("small_wgrad<false>", "small_wgrad<true>"):
    with pytest.raises(built_lib.MvError, match=r"needs Ci\*Co <= 512"):
      built_lib.op_small_conv_wgrad(x, d, form=f)
  with pytest.raises(built_lib.MvError, match="form h2g needs Co 1 or 2"):
    built_lib.op_small_conv_wgrad(np.zeros((1, 2, 2, 2)), np.zeros((1, 2, 2, 32)), form="h2g")


# ------------------------------------------------------------------ column sums, long sums
@pytest.mark.parametrize("ncols", hc.COLSUM_NCOLS_NARROW + hc.COLSUM_NCOLS_WIDE)
def test_colsum_exact(built_lib, ncols):
  for rows in [r for r, n in hc.colsum_cases() if n == ncols]:
    xi = hc.colsum_input(rows, ncols)
    ref = hc.colsum_ref(xi)[0]
    got, slabs, narrow = built_lib.op_colsum(xi.astype(np.float32) * np.float32(hc.QD))
    assert slabs == hc.COLSUM_SLABS[rows], (rows, slabs)
    assert narrow == hc.colsum_narrow_expected(rows, ncols), (rows, narrow)
    assert hc.compare_exact(dict(out=got), dict(out=ref)) == [], rows


def test_colsum_forms_written_out():
  """the slab counts and the wide / narrow choice, from the rule in engine_train.h"""
  assert hc.COLSUM_SLABS == {1: 1, 64: 1, 65: 2, 2048: 32, 2049: 33, 65537: 1009}
  assert [hc.colsum_narrow_expected(2049, n) for n in (1, 2, 32, 128, 48, 300, 1024)] == \
      [True, True, True, True, False, False, False]
  assert not hc.colsum_narrow_expected(64, 32)      # one slab: the plain kernel writes the result


@pytest.mark.parametrize("n", hc.LONG_SUM_N)
def test_long_sum_exact(built_lib, n):
  x = hc.long_sum_input(n)
  for scale in hc.LONG_SUM_SCALES:
    got, chunked = built_lib.op_long_sum(x, scale)
    assert chunked == (n > 4 * hc.LONG_SUM_CHUNK), n        # 16384: one workgroup; 16385: chunks
    assert hc.compare_exact(dict(out=got), dict(out=x.sum() * scale)) == [], (n, scale)


# ------------------------------------------------------------------ stride-2 scene stack
@pytest.mark.parametrize("shape", sorted(hc.SCENE_SHAPES), ids=lambda s: ".".join(map(str, s)))
def test_scene_conv_bwd_exact(built_lib, shape):
  pt, pl, slabs, rps = hc.SCENE_SHAPES[shape]
  for c in [c for c in hc.scene_cases() if c["shape"] == shape]:
    x, y, dy, w, init = hc.scene_inputs(c)
    ref = hc.scene_ref(c, x, y, dy, w, init)[0]
    got = built_lib.op_scene_conv_bwd(x, y, dy, w, act=hc.ACT_CODE[c["act"]],
                                      din_init=init if c["accumulate"] else None,
                                      accumulate=c["accumulate"])
    assert (got["pad_t"], got["pad_l"], got["slabs"], got["rows_per_slab"]) == \
        (pt, pl, slabs, rps), c["name"]
    assert hc.compare_exact(got, ref, hc.scene_check_keys(c)) == [], c["name"]


@pytest.mark.parametrize("Hi,Wi", [(7, 9), (8, 6)])
def test_scene_conv_bwd_onehot_corners_every_tap(built_lib, Hi, Wi):
  x, y, dy, w, cells = hc.scene_onehot(Hi, Wi)
  c = dict(name="onehot", shape=(4, Hi, Wi, 11, 64, 3), act="relu", accumulate=0)
  ref = hc.scene_ref(c, x, y, dy, w, None)[0]
  assert _nonzero(ref["din"]) == cells
  got = built_lib.op_scene_conv_bwd(x, y, dy, w, act=1)
  assert (got["pad_t"], got["pad_l"]) == ((1, 1) if Hi % 2 else (0, 0))
  assert _nonzero(got["din"]) == cells
  assert hc.compare_exact(got, ref) == []


# ------------------------------------------------------------------ one-hot embedding wgrad
@pytest.mark.parametrize("N,T,H,W,E", hc.ONEHOT_WGRAD_SHAPES)
def test_grid_emb_onehot_wgrad_exact(built_lib, N, T, H, W, E):
  dpre, labels, init = hc.onehot_wgrad_inputs(N, T, H, W, E)
  for acc in (0, 1):
    ref = hc.onehot_wgrad_ref(dpre, labels, init, acc)[0]
    got = built_lib.op_grid_emb_onehot_wgrad(dpre, labels, dw_init=init, accumulate=acc)
    for ky, kx in hc.TAPS:
      assert hc.compare_exact(dict(t=got[ky, kx]), dict(t=ref[ky, kx])) == [], (acc, ky, kx)
  bad = labels.copy()
  bad[0, 0] = H * W
  with pytest.raises(built_lib.MvError, match="is not a cell of the"):
    built_lib.op_grid_emb_onehot_wgrad(dpre, bad)


# ------------------------------------------------------------------ Huber
@pytest.mark.parametrize("c", hc.huber_cases(), ids=lambda c: c["name"])
def test_huber_losses_exact(built_lib, c):
  pred, target, fg = hc.huber_inputs(c)
  ref, exact, scale = hc.huber_ref(c, pred, target, fg)
  got = built_lib.op_train_loss(c["kind"], pred, scale, target=target, fg=fg,
                                pred_lens=c.get("pred_lens"))
  assert got["chunked"] == (pred.size > 4 * hc.LONG_SUM_CHUNK)
  assert hc.compare_huber(c, got, ref, exact) == [], c["name"]
  if c.get("count") == 0:                    # no foreground: loss 0 and gradient 0, not NaN
    assert got["loss_sum"] == 0 and not got["grad"].any() and not got["loss"].any()


# ------------------------------------------------------------------ cross entropies
def test_cross_entropies_within_four_oracle_constants(built_lib):
  worst, failures = {}, []
  for c in hc.ce_cases():
    z, labels, soft = hc.ce_inputs(c)
    ref, m = hc.ce_ref(c, z, labels, soft)
    got = built_lib.op_train_loss(c["kind"], z, hc.CE_SCALE, labels=labels if soft is None else None,
                                  soft=soft, sample_w=c.get("sample_w"),
                                  pred_lens=c.get("pred_lens"))
    bad, cs = hc.compare_ce(c, got, ref, m)
    if bad:
      failures.append((c["name"], bad))
    worst[c["kind"]] = tuple(max(a, b) for a, b in zip(worst.get(c["kind"], (0, 0, 0)), cs))
  for kind, cs in sorted(worst.items()):
    print("%-8s x 2^-24 m: loss rows %.3f (bar %.1f)  gradient %.3f (bar %.1f)  summed loss %.3f "
          "(bar %.1f)" % ((kind,) + tuple(v for pair in zip(cs, hc.ce_bars(dict(kind=kind)))
                                          for v in pair)))
  assert failures == []


def test_train_loss_refuses_what_the_kernels_would_index_with(built_lib):
  z = np.zeros((3, 2, 5))
  lab = np.zeros((2, 3), dtype=np.int32)
  for v in (-1, 5):
    bad = lab.copy()
    bad[1, 2] = v
    with pytest.raises(built_lib.MvError, match=r"label -?\d+ outside \[0, 5\)"):
      built_lib.op_train_loss("ce", z, 1.0, labels=bad)
  for v in (-1, 4):
    with pytest.raises(built_lib.MvError, match=r"pred_lens\[1\] = -?\d+ outside \[0, 3\]"):
      built_lib.op_train_loss("ce_len", z, 1.0, labels=lab, pred_lens=(0, v))
  with pytest.raises(built_lib.MvError, match="pred_lens"):
    built_lib.op_train_loss("huber_len", np.zeros((3, 2, 5, 2)), 1.0,
                            target=np.zeros((2, 3, 5, 2)), pred_lens=(9, 0))
