# coding=utf-8
"""Engine-level gradients of the training step at the grids where csrc/gate_plan.h leaves the
fast forms: mv_train_forward_backward against oracle.loss_and_grads, per weight tap, one scale per
engine (so the per-name kernel statistics describe ONE form), the form that ran asserted from
those statistics.

The default 18 x 32 / 9 x 16 grids of tests/test_gpu_train.py are exactly where every fast form
applies.  The rows here (scene -> scene_grids, the scale used, batch) and what each reaches:

  A  20x28 -> (10,14),(5,7)    scale 0, N=2  W divides neither 32 nor 16, H % 3 != 0: halo tiling
                                             of the training forward (gates saved), direct dgrad
                                             without the column shift, fp32 wgrad in every mode
  B  20x28 -> same             scale 1, N=3  105 cells: odd cell count, one full and one partial
                                             64-cell block, image rows ending inside a block
  C  72x36 -> (36,18),(18,9)   scale 1, N=2  the literal grid, W = 9
  D  16x32 -> (8,16),(4,8)     scale 0, N=2  W | 32, W % 16 == 0, H % 3 != 0: Winograd F(2,3) dgrad,
                                             DIRECT f16x3 wgrad on the wide tile
  E  16x32 -> same             scale 1, N=2  W = 8: Winograd dgrad with the fp32 wgrad fallback
  F   8x64 -> (4,32),(2,16)    scale 1, N=2  H = 2, the smallest grid of F(2,3): one row pair, no
                                             F(3,3) forward, no row-triple wgrad
  G  12x64 -> (6,32),(3,16)    scale 0, N=2  small all-fast-forms control: exact F(3,3), row-triple
                                             wgrad, two triples
  H  12x64 -> same             scale 1, N=3  H = 3: a single triple, an odd row pair for F(2,3)
  I  as H, hidden size 128     scale 1, N=2  f16x3 wgrad NOT on the wide tile (needs C % 256 == 0)
  Gr as G, --activation_func relu            bf16 only: the three-pass x forward, x exact

Modes: f32 and f16x3 for every row (I: f16x3 only), bf16 for A, B, D, F, G, H and Gr -- the halo
forward with the fp32 wgrad fallback (A, B), the wide direct one-plane wgrad (D, F), the
row-triple one-plane wgrad at two triples and at one (G, H).

Bars.  A ConvLSTM kernel [3,3,Cx+C,4C] is cut into 9 taps x {x rows, h rows}, every other tensor is
one slice; per slice max|gpu - fp64| / max|fp64 slice| < 2e-3 (the per-tensor bar of
test_gradients_match_oracle, per slice: a tap that is wrong only at an image edge otherwise hides
behind the other eight).  Two guards on the inputs keep a degenerate feed from passing: the fp32
CPU oracle's own per-slice error against fp64 < 2e-4, and every slice's max|fp64| > 1e-5.  f16x3
against the f32 mode of the same engine: 5e-5 per tensor, kernels as x rows / h rows
(test_f16x3_gradients_match_f32_mode).  bf16: finite, cosine against the fp32 oracle > 0.999 (a
per-slice bar against an oracle on rounded operands does not exist at this level: DESIGN.md 3d --
it exists one level down, kernel by kernel on operands exact in every plane:
tests/test_gpu_bwd_kernels.py).
"""

import numpy as np
import pytest
import torch

from bwd_cases import kernel_slices
from multiverse_amd import synth
from oracle import multiverse_oracle as oracle

pytestmark = pytest.mark.gpu

_G2010 = dict(scene_h=20, scene_w=28, scene_grids=[(10, 14), (5, 7)])
_LITERAL = dict(scene_h=72, scene_w=36, scene_grids=[(36, 18), (18, 9)])
_G0816 = dict(scene_h=16, scene_w=32, scene_grids=[(8, 16), (4, 8)])
_G0432 = dict(scene_h=8, scene_w=64, scene_grids=[(4, 32), (2, 16)])
_G0632 = dict(scene_h=12, scene_w=64, scene_grids=[(6, 32), (3, 16)])

# row -> (config overrides, scale, batch)
ROWS = {
    "A": (_G2010, 0, 2),
    "B": (_G2010, 1, 3),
    "C": (_LITERAL, 1, 2),
    "D": (_G0816, 0, 2),
    "E": (_G0816, 1, 2),
    "F": (_G0432, 1, 2),
    "G": (_G0632, 0, 2),
    "H": (_G0632, 1, 3),
    "I": (dict(_G0632, enc_hidden_size=128, dec_hidden_size=128), 1, 2),
    "Gr": (dict(_G0632, activation_func="relu"), 0, 2),
}

# Which form runs, written out from csrc/gate_plan.h (NOT obtained from the planner): MFMA FLOPs
# issued per executed FLOP of convlstm_dgrad / convlstm_wgrad (and convlstm_wgrad_x, which exists
# only where the f16 wgrad runs) / the training forward's convlstm_step.
#   dgrad   f16x3: 2 where 32 % W == 0 and H >= 2 (Winograd F(2,3)), else 3; f32 and bf16: 1
#   wgrad   f16x3: W % 16 != 0 -> 1 (the fp32 kernel, no wgrad_transpose); H % 3 == 0 -> 5/3
#           (row triples); else 3.   bf16: 1 / 5/9 / 1 by the same rule.   f32: 1
#   step    f16x3: H >= 3 -> 5 ceil(H/3) / H, times 32/30 in the halo tiling (32 % W != 0);
#           H = 2 -> F(2,3): 4 ceil(H/2) / H = 2
#   dgrad_slice_sum: the f16x3 dgrads split K (four slices direct, per column block in F(2,3));
#           the fp32 kernel and the bf16 dgrad (one slice) write their outputs whole
# row -> (dgrad f16x3, wgrad f16x3, wgrad bf16, step f16x3, f16 wgrad?)
FORMS = {
    "A": (3.0, 1.0, 1.0, 5.0 * 4 / 10 * 32 / 30, False),     # 10 x 14
    "B": (3.0, 1.0, 1.0, 5.0 * 2 / 5 * 32 / 30, False),      # 5 x 7
    "C": (3.0, 1.0, 1.0, 5.0 * 6 / 18 * 32 / 30, False),     # 18 x 9
    "D": (2.0, 3.0, 1.0, 5.0 * 3 / 8, True),                 # 8 x 16
    "E": (2.0, 1.0, 1.0, 5.0 * 2 / 4, False),                # 4 x 8
    "F": (2.0, 3.0, 1.0, 2.0, True),                         # 2 x 16
    "G": (2.0, 5.0 / 3, 5.0 / 9, 5.0 / 3, True),             # 6 x 32
    "H": (2.0, 5.0 / 3, 5.0 / 9, 5.0 / 3, True),             # 3 x 16
    "I": (2.0, 5.0 / 3, 5.0 / 9, 5.0 / 3, True),             # 3 x 16, C = 128
    "Gr": (2.0, 5.0 / 3, 5.0 / 9, 5.0 / 3, True),            # 6 x 32, relu
}

CASES = [(r, m) for r in "ABCDEFGH" for m in ("f32", "f16x3")] + [("I", "f16x3")]
CASES += [(r, "bf16") for r in ("A", "B", "D", "F", "G", "H", "Gr")]
CASES.sort(key=lambda c: c[0])          # a row's modes run back to back: one oracle, one f32 run

SLICE_BAR, ORACLE_BAR, MAG_BAR, F16X3_BAR, COS_BAR = 2e-3, 2e-4, 1e-5, 5e-5, 0.999

# the last row's CPU oracle and f32-mode GPU gradients (one row at a time: a gate kernel's
# gradient is 10 MB and a row holds four, in three precisions)
_ORACLE, _F32 = {}, {}


def _case(row):
  over, scale, N = ROWS[row]
  cfg = synth.default_config(batch_size=N, use_grids=(1, 0) if scale == 0 else (0, 1),
                             is_train=True, obs_len=3, pred_len=2, **over)
  params = synth.make_params(cfg, seed=synth.SEED_BASE + 1, recurrent_gain=2.0, bias_scale=0.1)
  feed = synth.make_feed(cfg, seed=synth.SEED_BASE + 51)
  return cfg, params, feed


def _oracle(row, cfg, params, feed):
  if row not in _ORACLE:
    _ORACLE.clear()
    _ORACLE[row] = (oracle.loss_and_grads(params, cfg, feed),
                    oracle.loss_and_grads(params, cfg, feed, dtype=torch.float64)[3])
  return _ORACLE[row]


def _gpu(lib, row, cfg, params, feed, mode):
  """One engine, one forward/backward with the kernel statistics on -> losses, gradients, stats."""
  if mode == "f32" and row in _F32:
    return _F32[row]
  eng = lib.Engine(cfg, device=0)
  eng.set_params(params)
  eng.set_compute_mode(mode)
  eng.set_profiling(True)
  eng.train_init()
  eng.reset_kernel_stats()
  losses = eng.train_forward_backward(feed)
  stats = eng.kernel_stats()
  grads = {n: eng.get_grad(n) for n, _ in eng.param_specs()}
  eng.close()
  out = (losses, grads, stats)
  if mode == "f32":
    _F32.clear()
    _F32[row] = out
  return out


def is_gate_kernel(name, a, C):
  return name.endswith("/kernel") and a.ndim == 4 and a.shape[:2] == (3, 3) and a.shape[3] == 4 * C


def slices(name, a, C):
  """(label, view) of a gradient: a gate kernel per tap and x rows / h rows, else whole."""
  if not is_gate_kernel(name, a, C):
    return [("all", a)]
  return kernel_slices(a, C)


def _err(a, b):
  return float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())


def _ratio(stats, name):
  s = stats[name]
  assert s["launches"] > 0 and s["flops"] > 0, name
  return s["flops_mfma"] / s["flops"]


def _check_forms(row, mode, stats):
  dg16, wg16, wgbf, step16, f16_wgrad = FORMS[row]
  want = {"f32": {"convlstm_dgrad": 1.0, "convlstm_wgrad": 1.0},
          "f16x3": {"convlstm_dgrad": dg16, "convlstm_wgrad": wg16, "convlstm_step": step16},
          "bf16": {"convlstm_dgrad": 1.0, "convlstm_wgrad": wgbf}}[mode]
  f16 = mode != "f32" and f16_wgrad
  if f16:
    want["convlstm_wgrad_x"] = want["convlstm_wgrad"]
  got = {k: _ratio(stats, k) for k in want}
  present = {k: k in stats and stats[k]["launches"] > 0
             for k in ("dgrad_slice_sum", "wgrad_transpose", "convlstm_wgrad_x")}
  print("%s %-5s forms: %s | %s" % (row, mode, " ".join("%s %.6f" % (k[9:], v) for k, v in
                                                        sorted(got.items())), present))
  for k, v in want.items():
    assert abs(got[k] - v) < 1e-6, (row, mode, k, got[k], v)
  assert present["dgrad_slice_sum"] == (mode == "f16x3"), (row, mode, "dgrad_slice_sum")
  assert present["wgrad_transpose"] == f16, (row, mode, "wgrad_transpose")
  assert present["convlstm_wgrad_x"] == f16, (row, mode, "convlstm_wgrad_x")


@pytest.mark.parametrize("row,mode", CASES)
def test_gradients_per_slice_and_form(built_lib, row, mode):
  cfg, params, feed = _case(row)
  C = cfg.enc_hidden_size
  # (the engine before the oracle, as everywhere in this suite: the library opens the device)
  (loss, wd, pgl), grads, stats = _gpu(built_lib, row, cfg, params, feed, mode)
  (oloss, owd, opgl, og32), og64 = _oracle(row, cfg, params, feed)
  print("%s %-5s loss gpu %.6f oracle %.6f | wd %.6g / %.6g | parts %s / %s"
        % (row, mode, loss, oloss, wd, owd, pgl, opgl))
  names = [n for n in sorted(grads) if og64.get(n) is not None]     # None: the unused scale's
  assert any(is_gate_kernel(n, grads[n], C) for n in names)

  # guards on the inputs: the oracle itself is fp32-class on every slice, and no slice is so
  # small that its relative error means nothing
  worst_cpu, least = 0.0, np.inf
  for n in names:
    for what, r64 in slices(n, og64[n], C):
      mag = float(np.abs(r64).max())
      least = min(least, mag)
      assert mag > MAG_BAR, (n, what, mag)
    for (what, r32), (_, r64) in zip(slices(n, og32[n], C), slices(n, og64[n], C)):
      e = _err(r32, r64)
      worst_cpu = max(worst_cpu, e)
      assert e < ORACLE_BAR, (n, what, e)
  print("%s guards: fp32 oracle worst slice %.2e, least max|fp64 slice| %.3g"
        % (row, worst_cpu, least))

  assert abs(wd - owd) < 1e-5 * max(1.0, abs(owd))
  if mode == "bf16":
    assert abs(loss - oloss) < 2e-2 * abs(oloss)
    worst = 1.0
    for n in names:
      a, b = grads[n].reshape(-1).astype(np.float64), og32[n].reshape(-1).astype(np.float64)
      cos = float(a @ b / max(np.linalg.norm(a) * np.linalg.norm(b), 1e-300))
      worst = min(worst, cos)
      assert np.isfinite(a).all() and cos > COS_BAR, (n, cos)
    print("%s bf16  worst gradient cosine vs the fp32 oracle %.6f" % (row, worst))
  else:
    assert abs(loss - oloss) < 1e-4 * max(1.0, abs(oloss))
    assert np.allclose(pgl, opgl, rtol=1e-4, atol=1e-5)
    worst, where, failed = 0.0, None, []
    for n in names:
      for (what, g), (_, r64) in zip(slices(n, grads[n], C), slices(n, og64[n], C)):
        e = _err(g, r64)
        if e > worst:
          worst, where = e, (n, what)
        if not e < SLICE_BAR:
          failed.append((n, what, e))
    print("%s %-5s worst slice vs fp64 %.2e at %s" % (row, mode, worst, where))
    assert not failed, failed

  if mode == "f16x3":
    _, g32, _ = _gpu(built_lib, row, cfg, params, feed, "f32")
    worst, where = 0.0, None
    for n in names:
      a, b = g32[n], grads[n]
      assert np.isfinite(b).all(), n
      parts = [("all", a, b)]
      if is_gate_kernel(n, a, C):
        Cx = a.shape[2] - C
        parts = [("x rows", a[:, :, :Cx], b[:, :, :Cx]), ("h rows", a[:, :, Cx:], b[:, :, Cx:])]
      for what, u, v in parts:
        e = float(np.abs(u - v).max() / max(np.abs(u).max(), 1e-30))
        if e > worst:
          worst, where = e, (n, what)
        assert e < F16X3_BAR, (n, what, e)
    print("%s f16x3 vs f32 mode: worst %.2e at %s" % (row, worst, where))

  _check_forms(row, mode, stats)
