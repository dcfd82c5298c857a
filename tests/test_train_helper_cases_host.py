# coding=utf-8
"""CPU-side checks of tests/train_helper_cases.py, the inputs, references and bars of
tests/test_gpu_train_helpers.py:

  * the exactness premise of every exact case (sum |terms| < 2^24 quanta per output);
  * the numpy float64 references against torch.autograd in float64 (1e-12);
  * the float32 device models pass the GPU test's own comparison functions;
  * every mutation of a model fails at least one named case (listed with -s);
  * the float32 torch oracle's cross-entropy constants stay below the ones written down."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_helper_cases as hc
from oracle import multiverse_oracle as oracle

T64 = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), dtype=torch.float64)
CLOSE = 1e-12


def _close(a, b, what):
  a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
  assert a.shape == b.shape, what
  assert np.abs(a - b).max() <= CLOSE * max(1.0, np.abs(b).max()), what


# ------------------------------------------------------------------ the written-out plans
def test_written_plans_follow_their_rules():
  for cells, (blocks, cpb) in hc.SMALL_WGRAD_BLOCKS.items():
    nb = min(4096, -(-cells // 64))
    c = -(-cells // nb)
    assert (blocks, cpb) == (-(-cells // c), c), cells
  assert {r * h * w for r, h, w in hc.SMALL_WGRAD_SHAPES} == set(hc.SMALL_WGRAD_BLOCKS)
  for (Ci, Co), (form, G) in hc.SMALL_WGRAD_CHANNELS.items():
    P = Ci * Co
    g = max(1, 256 // P)
    want = ("h2g" if Ci > Co and Ci <= 512 and Co in (1, 2) and g == 1
            else "small_wgrad<true>" if Ci > Co else "small_wgrad<false>")
    assert (form, G) == (want, g), (Ci, Co)
    assert form in hc.small_wgrad_forms_allowed(Ci, Co)
  for rows, slabs in hc.COLSUM_SLABS.items():
    n = max(1, min(1024, -(-rows // 64)))
    rps = -(-rows // n)
    assert (slabs, hc.COLSUM_RPS[rows]) == (-(-rows // rps), rps), rows
  for (U, Hi, Wi, Ci, Co, k), (pt, pl, slabs, rps) in hc.SCENE_SHAPES.items():
    Ho = (Hi + 1) // 2
    assert pt == max((Ho - 1) * 2 + k - Hi, 0) // 2
    assert pl == max(((Wi + 1) // 2 - 1) * 2 + k - Wi, 0) // 2
    r = -(-(U * Ho) // 64)
    assert (slabs, rps) == (-(-(U * Ho) // r), r)
  # the cases the issue names are all there
  assert sorted({hc.small_dgrad_form_expected(ci, co, 4 * ci) for ci, co in
                 hc.SMALL_DGRAD_CHANNELS}) == ["dgrad4<1>", "dgrad4<2>", "scalar"]
  assert hc.small_dgrad_form_expected(256, 2, 14 * 256 + 2) == "scalar"


# ------------------------------------------------------------------ the exactness premise
def test_exactness_premise_small_convs():
  for c in hc.small_dgrad_cases():
    _, mag = hc.small_dgrad_ref(c, *hc.small_dgrad_inputs(c))
    assert hc.premise(mag, hc.QD * hc.QW), c["name"]
  for (R, H, W) in hc.SMALL_WGRAD_SHAPES:
    for (Ci, Co) in hc.SMALL_WGRAD_CHANNELS:
      x, d = hc.small_wgrad_inputs(R, H, W, Ci, Co)
      assert hc.premise(hc.conv3x3_wgrad_ref(np.abs(x), np.abs(d)), hc.QD * hc.QD)
  for (N, T, H, W, E) in hc.ONEHOT_WGRAD_SHAPES:
    dpre, labels, init = hc.onehot_wgrad_inputs(N, T, H, W, E)
    assert hc.premise(hc.onehot_wgrad_ref(dpre, labels, init, True)[1], hc.QD)


def test_exactness_premise_scene():
  for c in hc.scene_cases():
    ref, mag, q, cnt = hc.scene_ref(c, *hc.scene_inputs(c))
    for k in hc.scene_check_keys(c):
      if c["act"] in ("lrelu_dpre", "lrelu_slope"):      # one term per output, one rounding
        n = cnt[k] if cnt else (ref[k] != 0) * 1.0
        assert hc.premise(None, None, nterms=n), (c["name"], k)
      else:
        assert hc.premise(mag[k], q), (c["name"], k)
    x, y, dy, w, init = hc.scene_inputs(c)
    if c["act"] == "tanh":
      assert np.abs(y).max() < 1.0
    if c["act"] == "lrelu":
      assert (y > 0).any() and (y < 0).any() and not dy[y <= 0].any()


def test_exactness_premise_sums_and_huber():
  for rows, ncols in hc.colsum_cases():
    _, mag = hc.colsum_ref(hc.colsum_input(rows, ncols))
    assert hc.premise(mag, hc.QD), (rows, ncols)
  for n in hc.LONG_SUM_N:
    x = hc.long_sum_input(n)
    assert hc.premise(np.abs(x).sum(), hc.QD * min(hc.LONG_SUM_SCALES)) and x[-1] != 0
  for c in hc.huber_cases():
    pred, target, fg = hc.huber_inputs(c)
    ref, exact, scale = hc.huber_ref(c, pred, target, fg)
    e = pred - target.transpose(1, 0, 2, 3)
    assert set(np.abs(hc.HUBER_E)) <= set(np.abs(e).reshape(-1).tolist())
    # loss elements on 2^-7 (0.5 (2^-3)^2), their sum below 2^24 of them
    assert hc.premise(np.abs(ref["loss"]).sum(), 2.0 ** -7), c["name"]
    assert exact == (c.get("count") != 70)
    if "pred_lens" in c:
      assert 0 in c["pred_lens"] and c["T"] in c["pred_lens"]


# ------------------------------------------------------------------ references vs torch float64
def _conv_grads(x, w, g, stride):
  xt, wt = T64(x).requires_grad_(True), T64(w).requires_grad_(True)
  out = oracle.conv2d_same(xt, wt, stride=stride)
  out.backward(T64(g))
  return out.detach().numpy(), xt.grad.numpy(), wt.grad.numpy()


@pytest.mark.parametrize("M,H,W,Ci,Co", [(1, 1, 1, 3, 6), (1, 4, 5, 8, 2), (5, 2, 7, 2, 32),
                                         (2, 9, 16, 4, 1)])
def test_conv3x3_refs_match_torch_autograd(M, H, W, Ci, Co):
  rng = np.random.default_rng(M + H + W)
  x, w, g = rng.standard_normal((M, H, W, Ci)), rng.standard_normal((3, 3, Ci, Co)), \
      rng.standard_normal((M, H, W, Co))
  out, dx, dw = _conv_grads(x, w, g, 1)
  _close(hc.conv3x3_ref(x, w), out, "forward")
  _close(hc.conv3x3_dgrad_ref(g, w), dx, "dgrad")
  _close(hc.conv3x3_wgrad_ref(x, g), dw, "wgrad")


@pytest.mark.parametrize("shape", sorted(hc.SCENE_SHAPES))
def test_scene_refs_match_torch_autograd(shape):
  U, Hi, Wi, Ci, Co, k = shape
  rng = np.random.default_rng(sum(shape))
  x, w = rng.standard_normal((U, Hi, Wi, Ci)), rng.standard_normal((k, k, Ci, Co))
  Ho, Wo = (Hi + 1) // 2, (Wi + 1) // 2
  g = rng.standard_normal((U, Ho, Wo, Co))
  out, dx, dw = _conv_grads(x, w, g, 2)
  _close(hc.conv_s2_ref(x, w), out, "forward")
  _close(hc.conv_s2_dgrad_ref(g, w, Hi, Wi), dx, "dgrad")
  _close(hc.conv_s2_wgrad_ref(x, g, k), dw, "wgrad")
  assert hc.same_pad(Hi, k) == (Ho, hc.SCENE_SHAPES[shape][0])
  assert hc.same_pad(Wi, k) == (Wo, hc.SCENE_SHAPES[shape][1])
  assert oracle.same_pads(Hi, k, 2)[0] == hc.SCENE_SHAPES[shape][0]
  # the whole level on a case's own inputs: x.grad, W.grad and b.grad of act(conv + b)
  for act in ("tanh", "relu", "lrelu"):
    c = dict(name="t_%s" % act, shape=shape, act=act, accumulate=0)
    x, y, dy, w, init = hc.scene_inputs(c)
    ref = hc.scene_ref(c, x, y, dy, w, init)[0]
    if act == "tanh":        # a pre-activation that gives y
      pre = torch.atanh(T64(y))
      fn = torch.tanh
    elif act == "relu":
      pre = T64(np.where(y > 0, y, -1.0))
      fn = torch.relu
    else:
      pre = T64(np.where(y > 0, y, y / hc.LRELU_SLOPE))
      fn = lambda v: F.leaky_relu(v, negative_slope=hc.LRELU_SLOPE)
    pre.requires_grad_(True)
    fn(pre).backward(T64(dy))
    assert np.abs(pre.grad.numpy() - ref["dpre"]).max() <= 2.0 ** -24      # (dpre: one fp32 rounding)
    xt, wt, bt = T64(x).requires_grad_(True), T64(w).requires_grad_(True), \
        torch.zeros(Co, dtype=torch.float64, requires_grad=True)
    (oracle.conv2d_same(xt, wt, stride=2) + bt).backward(T64(ref["dpre"]))
    _close(ref["din"], xt.grad.numpy(), "din")
    _close(ref["dw"], wt.grad.numpy(), "dw")
    _close(ref["db"], bt.grad.numpy(), "db")


@pytest.mark.parametrize("N,T,H,W,E", hc.ONEHOT_WGRAD_SHAPES)
def test_onehot_wgrad_ref_matches_torch_autograd(N, T, H, W, E):
  dpre, labels, init = hc.onehot_wgrad_inputs(N, T, H, W, E)
  hot = F.one_hot(torch.tensor(labels.T.astype(np.int64)), H * W).to(torch.float64)   # [T, N, K]
  wt = torch.zeros(3, 3, 1, E, dtype=torch.float64, requires_grad=True)
  oracle.conv2d_same(hot.reshape(T * N, H, W, 1), wt).backward(T64(dpre).reshape(T * N, H, W, E))
  _close(hc.onehot_wgrad_ref(dpre, labels, init, False)[0], wt.grad.numpy()[:, :, 0, :], "dw")
  _close(hc.onehot_wgrad_ref(dpre, labels, init, True)[0], wt.grad.numpy()[:, :, 0, :] + init,
         "dw accumulated")


@pytest.mark.parametrize("c", hc.huber_cases(), ids=lambda c: c["name"])
def test_huber_ref_matches_torch(c):
  pred, target, fg = hc.huber_inputs(c)
  ref, _, scale = hc.huber_ref(c, pred, target, fg)
  p = T64(pred).requires_grad_(True)
  el = F.huber_loss(p, T64(target).permute(1, 0, 2, 3), reduction="none", delta=1.0)
  if c["kind"] == "huber_masked":
    on = T64((fg > 0) * 1.0)[..., None]
    cnt = int((fg > 0).sum())
    el = el * on
    total = el.sum() / (2.0 * cnt) * scale if cnt else el.sum() * 0.0
  else:
    if c["kind"] == "huber_len":
      valid = np.arange(c["T"])[:, None] < np.array(c["pred_lens"])[None, :]
      el = el * T64(valid * 1.0)[..., None, None]
    total = el.sum() * scale
  total.backward()
  _close(ref["loss"], el.detach().numpy(), "elements")
  _close(ref["grad"], p.grad.numpy(), "gradient")
  _close(ref["loss_sum"], total.item(), "sum")


@pytest.mark.parametrize("c", hc.ce_cases(), ids=lambda c: c["name"])
def test_ce_ref_matches_torch(c):
  z, labels, soft = hc.ce_inputs(c)
  ref, m = hc.ce_ref(c, z, labels, soft)
  zt = T64(z).requires_grad_(True)
  lsm = F.log_softmax(zt, dim=-1)
  roww = np.ones((c["T"], c["N"]))
  if "sample_w" in c:
    roww = roww * np.array(c["sample_w"])[None, :]
  if "pred_lens" in c:
    roww = roww * (np.arange(c["T"])[:, None] < np.array(c["pred_lens"])[None, :])
  if soft is None:
    rows = F.cross_entropy(zt.reshape(-1, c["K"]), torch.tensor(labels.T.reshape(-1).astype(np.int64)),
                           reduction="none").reshape(c["T"], c["N"])
  else:
    rows = -(T64(soft) * lsm).sum(dim=-1)
  rows = rows * T64(roww)
  (rows.sum() * hc.CE_SCALE).backward()
  _close(ref["loss"], rows.detach().numpy(), "rows")
  _close(ref["loss_sum"], rows.sum().item() * hc.CE_SCALE, "sum")
  if soft is None or c["soft_sum"] == 1.0:
    # (autograd of -sum q log_softmax is softmax sum(q) - q: TF's registered gradient only
    # where the labels sum to one -- which float32 soft labels do to K 2^-24)
    assert np.abs(zt.grad.numpy() - ref["grad"]).max() <= 1e-12 + c["K"] * 2.0 ** -24
  want = (torch.softmax(T64(z), dim=-1).numpy() - (soft if soft is not None else
                                                   np.eye(c["K"])[labels.T])) * hc.CE_SCALE
  _close(ref["grad"], want * roww[..., None], "registered gradient")
  named = [v for v in (0, 63, 64, c["K"] - 1) if v < c["K"]]
  assert set(named) <= set(labels.reshape(-1).tolist())


# ------------------------------------------------------------------ models and mutations
WGRAD_MODEL_CHANNELS = [(2, 32), (64, 2)]      # (the model is one for all forms)
SEAM_SHAPES = [(3, 5, 7), (5, 2, 7)]


def _family(name):
  """(case name, fn(fault) -> list of mismatches) of every case of a family"""
  out = []
  if name == "small_dgrad":
    for c in hc.small_dgrad_cases():
      if c["Ci"] > 256 or (c["M"], c["H"], c["W"]) == (2, 9, 16) and c["Ci"] > 3:
        continue                                 # (the model is slow and no different there)
      a = hc.small_dgrad_inputs(c)
      ref = hc.small_dgrad_ref(c, *a)[0]
      out.append((c["name"], lambda f, c=c, a=a, ref=ref: hc.compare_exact(
          dict(din=hc.model_small_dgrad(c, *a, fault=f)), dict(din=ref))))
    for Ci, Co in ((256, 2), (9, 6)):
      dout, w, cells = hc.small_dgrad_onehot(Ci, Co)
      M = len(hc.ONEHOT_POSITIONS)
      c = dict(M=M, H=hc.ONEHOT_H, W=hc.ONEHOT_W, Ci=Ci, Co=Co, accumulate=0)
      flat = dout.reshape(M, -1)
      ref = hc.conv3x3_dgrad_ref(dout, w)
      assert {tuple(int(v) for v in i) for i in np.argwhere(ref != 0)} == cells
      out.append(("dgrad_onehot_%dx%d" % (Ci, Co), lambda f, c=c, flat=flat, w=w, ref=ref:
                  hc.compare_exact(dict(din=hc.model_small_dgrad(
                      c, flat, w, np.zeros((c["M"], ref[0].size)), fault=f)),
                      dict(din=ref.reshape(c["M"], -1)))))
  elif name == "small_wgrad":
    for (R, H, W) in hc.SMALL_WGRAD_SHAPES:
      cpb = hc.SMALL_WGRAD_BLOCKS[R * H * W][1]
      for (Ci, Co) in WGRAD_MODEL_CHANNELS:
        x, d = hc.small_wgrad_inputs(R, H, W, Ci, Co)
        ref = hc.conv3x3_wgrad_ref(x, d)
        out.append(("wgrad_%dx%d_%d.%d.%d" % (Ci, Co, R, H, W), lambda f, x=x, d=d, cpb=cpb, ref=ref:
                    hc.compare_exact(dict(dw=hc.model_small_wgrad(x, d, cpb, fault=f)),
                                     dict(dw=ref))))
    for (R, H, W) in SEAM_SHAPES:
      cpb = hc.SMALL_WGRAD_BLOCKS[R * H * W][1]
      for seam, cells in hc.small_wgrad_seam_cells(R, H, W).items():
        for s in cells:
          for (Ci, Co) in WGRAD_MODEL_CHANNELS:
            x, d, nz = hc.small_wgrad_onehot(R, H, W, Ci, Co, s)
            ref = hc.conv3x3_wgrad_ref(x, d)
            assert {tuple(int(v) for v in i) for i in np.argwhere(ref != 0)} == nz
            out.append(("wgrad_onehot_%dx%d_%d.%d.%d_%s_seam_cell%d" % (Ci, Co, R, H, W, seam, s),
                        lambda f, x=x, d=d, cpb=cpb, ref=ref: hc.compare_exact(
                            dict(dw=hc.model_small_wgrad(x, d, cpb, fault=f)), dict(dw=ref))))
  elif name == "scene":
    for c in hc.scene_cases():
      a = hc.scene_inputs(c)
      ref = hc.scene_ref(c, *a)[0]
      out.append((c["name"], lambda f, c=c, a=a, ref=ref: hc.compare_exact(
          hc.model_scene_bwd(c, *a, fault=f), ref, hc.scene_check_keys(c))))
    for (Hi, Wi) in ((7, 9), (8, 6)):
      x, y, dy, w, cells = hc.scene_onehot(Hi, Wi)
      c = dict(name="scene_onehot_%dx%d" % (Hi, Wi), shape=(4, Hi, Wi, 11, 64, 3), act="relu",
               accumulate=0)
      ref = hc.scene_ref(c, x, y, dy, w, None)[0]
      assert {tuple(int(v) for v in i) for i in np.argwhere(ref["din"] != 0)} == cells
      out.append((c["name"], lambda f, c=c, a=(x, y, dy, w, None), ref=ref: hc.compare_exact(
          hc.model_scene_bwd(c, *a, fault=f), ref)))
  elif name == "onehot_wgrad":
    for shape in hc.ONEHOT_WGRAD_SHAPES:
      dpre, labels, init = hc.onehot_wgrad_inputs(*shape)
      for acc in (0, 1):
        ref = hc.onehot_wgrad_ref(dpre, labels, init, acc)[0]
        out.append(("onehot_wgrad_%s_acc%d" % (".".join(map(str, shape)), acc),
                    lambda f, dpre=dpre, labels=labels, init=init, acc=acc, ref=ref:
                    hc.compare_exact(dict(dw=hc.model_onehot_wgrad(dpre, labels, init, acc, fault=f)),
                                     dict(dw=ref))))
  elif name == "colsum":
    for rows, ncols in hc.colsum_cases():
      if rows == 65537 and ncols != 2:
        continue                                 # (one column count is enough for the model)
      xi = hc.colsum_input(rows, ncols)
      ref = hc.colsum_ref(xi)[0]
      out.append(("colsum_%dx%d" % (rows, ncols), lambda f, xi=xi, ref=ref: hc.compare_exact(
          dict(out=hc.model_colsum(xi, fault=f)), dict(out=ref))))
  elif name == "long_sum":
    for n in hc.LONG_SUM_N:
      for scale in hc.LONG_SUM_SCALES:
        x = hc.long_sum_input(n)
        out.append(("long_sum_%d_x%g" % (n, scale), lambda f, x=x, scale=scale: hc.compare_exact(
            dict(out=hc.model_long_sum(x, scale, fault=f)), dict(out=x.sum() * scale))))
  elif name == "huber":
    for c in hc.huber_cases():
      pred, target, fg = hc.huber_inputs(c)
      ref, exact, scale = hc.huber_ref(c, pred, target, fg)
      out.append((c["name"], lambda f, c=c, a=(pred, target, fg), ref=ref, exact=exact, scale=scale:
                  hc.compare_huber(c, hc.model_huber(c, *a, scale, fault=f), ref, exact)))
  elif name == "ce":
    for c in hc.ce_cases():
      a = hc.ce_inputs(c)
      ref, m = hc.ce_ref(c, *a)
      out.append((c["name"], lambda f, c=c, a=a, ref=ref, m=m:
                  hc.compare_ce(c, hc.model_ce(c, *a, fault=f), ref, m)[0]))
  return out


FAMILIES = ("small_dgrad", "small_wgrad", "scene", "onehot_wgrad", "colsum", "long_sum", "huber",
            "ce")
_cache = {}


def _cases(family):
  if family not in _cache:
    _cache[family] = _family(family)
  return _cache[family]


@pytest.mark.parametrize("family", FAMILIES)
def test_device_models_pass_the_gpu_comparison(family):
  cases = _cases(family)
  assert cases
  for name, run in cases:
    assert run(None) == [], name


@pytest.mark.parametrize("mutation", sorted(hc.MUTATIONS))
def test_every_mutation_fails_a_named_case(mutation):
  for family in hc.MUTATIONS[mutation]:
    caught = [name for name, run in _cases(family) if run(mutation)]
    print("%-28s %-13s caught by %d cases, e.g. %s" % (mutation, family, len(caught),
                                                       ", ".join(caught[:3])))
    assert caught, "%s / %s: no case catches it -- a case is missing" % (mutation, family)


def test_seam_mutations_are_caught_by_the_seam_cases():
  """the one-hot pairs across a seam are what names the seam bugs"""
  for mutation, seam in (("edge_dropped_at_block_seam", "block"),
                         ("edge_dropped_at_image_seam", "image")):
    caught = [n for n, run in _cases("small_wgrad")
              if "onehot" in n and "%s_seam" % seam in n and run(mutation)]
    assert caught, mutation


# ------------------------------------------------------------------ the oracle's constants
def test_torch_float32_oracle_constants_are_below_the_written_ones():
  worst = {}
  for c in hc.ce_cases():
    z, labels, soft = hc.ce_inputs(c)
    ref, m = hc.ce_ref(c, z, labels, soft)
    zt = torch.tensor(z, dtype=torch.float32)
    lsm = F.log_softmax(zt, dim=-1)
    sm = torch.softmax(zt, dim=-1)
    if soft is None:
      lab = torch.tensor(labels.T.astype(np.int64))
      rows = -torch.gather(lsm, -1, lab[..., None])[..., 0]
      hot = F.one_hot(lab, c["K"]).to(torch.float32)
    else:
      hot = torch.tensor(soft, dtype=torch.float32)
      rows = -(hot * lsm).sum(dim=-1)
    roww = torch.tensor(m["valid"] * 1.0, dtype=torch.float32)
    if "sample_w" in c:
      roww = roww * torch.tensor(c["sample_w"], dtype=torch.float32)[None, :]
    rows = rows * roww
    grad = (sm - hot) * np.float32(hc.CE_SCALE) * roww[..., None]
    got = dict(loss=rows.numpy(), grad=grad.numpy(),
               loss_sum=np.float32(rows.sum().item() * hc.CE_SCALE))
    cs = hc.ce_constants(got, ref, m)
    worst[c["kind"]] = tuple(max(a, b) for a, b in zip(worst.get(c["kind"], (0, 0, 0)), cs))
  for kind, cs in sorted(worst.items()):
    print("float32 torch oracle, %-8s loss rows %.3f  gradient %.3f  summed loss %.3f  (x 2^-24 m)"
          % ((kind,) + cs))
  for kind, cs in sorted(worst.items()):
    for got, written in zip(cs, hc.CE_ORACLE_C[kind]):
      assert got <= written, (kind, cs)
