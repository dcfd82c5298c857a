# coding=utf-8
"""The scene stack's convolution comes in two forms -- tiled for k = 3 with 64 output channels,
one thread per output for every other shape -- compared form against form BIT FOR BIT through
the single-kernel entry point mv_op_scene_conv (csrc/engine_ops.h).  The tiled form re-schedules
the work and keeps every output's chain of operations, so nothing but `==` on the bits is asked.
Which kernel a shape takes is csrc/step_plan.h's answer (scene_conv_form), asserted here as well
so that no case compares a kernel with itself unnoticed."""
import numpy as np
import pytest

ACTS = (0, 1, 2)                                  # tanh, relu, lrelu (kernels_misc.h act_apply)
# the fp64 guard of the scene convolution: an fp32 chain of n <= 576 products of size ~ 1 / sqrt(n)
# each drifts by about sqrt(n) * 2^-24 * |sum| ~ 1e-6 from fp64; 1e-4 leaves two decades and still
# catches a dropped or doubled tap (~ 0.04)
SCENE_GUARD = 1e-4


def _bits(a):
  a = np.ascontiguousarray(a)
  return a.view({4: np.uint32, 2: np.uint16}[a.dtype.itemsize])


def _same_bits(a, b):
  return a.shape == b.shape and bool((_bits(a) == _bits(b)).all())


# ------------------------------------------------------------------ scene conv

def test_scene_conv_plan_refuses_what_the_tiled_kernel_does_not_tile(built_lib):
  """Host only: k = 3 with 64 output channels and at most 64 input channels is tiled; every
  other shape keeps the kernel it had."""
  f = built_lib.scene_conv_form
  assert f(3, 11, 64) == "tiled" and f(3, 64, 64) == "tiled" and f(3, 1, 64) == "tiled"
  assert f(3, 65, 64) == "per_output"             # a tap's weights would not fit the LDS tile
  assert f(3, 11, 32) == "per_output" and f(3, 11, 128) == "per_output"   # Co it does not tile
  assert f(5, 11, 64) == "per_output" and f(7, 64, 64) == "per_output"
  assert f(1, 11, 64) == "proj1x1" and f(1, 64, 32) == "proj1x1"
  assert f(1, 11, 128) == "per_output"


def _scene_case(rng, U, Hi, Wi, Ci, Co, k=3):
  x = rng.standard_normal((U, Hi, Wi, Ci)).astype(np.float32)
  w = (rng.standard_normal((k, k, Ci, Co)) / np.sqrt(k * k * Ci)).astype(np.float32)
  b = (0.1 * rng.standard_normal(Co)).astype(np.float32)
  return x, w, b


def _scene_numpy(x, w, b, act):
  """fp64 stride-2 SAME convolution: not the bit reference (the per-output kernel is), a guard
  against both forms being wrong together."""
  U, Hi, Wi, Ci = x.shape
  k, Co = w.shape[0], w.shape[3]
  Ho, Wo = (Hi + 1) // 2, (Wi + 1) // 2
  pt = max((Ho - 1) * 2 + k - Hi, 0) // 2
  pl = max((Wo - 1) * 2 + k - Wi, 0) // 2
  xp = np.zeros((U, Hi + 2 * k, Wi + 2 * k, Ci))
  xp[:, pt:pt + Hi, pl:pl + Wi] = x
  out = np.zeros((U, Ho, Wo, Co))
  for ky in range(k):
    for kx in range(k):
      out += xp[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2] @ w[ky, kx].astype(np.float64)
  out += b
  if act == 0:
    return np.tanh(out)
  return np.where(out > 0, out, 0.0 if act == 1 else 0.2 * out)


@pytest.mark.gpu
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape", [(3, 7, 10, 11, 64),      # odd sizes, asymmetric SAME padding
                                   (1, 5, 6, 64, 64)])
def test_scene_conv_tiled_equals_per_output(built_lib, shape, act):
  U, Hi, Wi, Ci, Co = shape
  assert built_lib.scene_conv_form(3, Ci, Co) == "tiled"
  x, w, b = _scene_case(np.random.default_rng(17 + act), *shape)
  new = built_lib.op_scene_conv(x, w, b, act=act)
  old = built_lib.op_scene_conv(x, w, b, act=act, per_output=True)
  assert np.abs(old - _scene_numpy(x, w, b, act)).max() < SCENE_GUARD
  assert _same_bits(new, old), int((_bits(new) != _bits(old)).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("act", ACTS)
def test_scene_conv_published_stack(built_lib, act):
  """36 x 64 x 11 -> 18 x 32 x 64 -> 9 x 16 x 64, the second level fed by the first."""
  rng = np.random.default_rng(5 + act)
  x, w1, b1 = _scene_case(rng, 2, 36, 64, 11, 64)
  _, w2, b2 = _scene_case(rng, 1, 1, 1, 64, 64)
  l1 = built_lib.op_scene_conv(x, w1, b1, act=act)
  l1_old = built_lib.op_scene_conv(x, w1, b1, act=act, per_output=True)
  assert l1.shape == (2, 18, 32, 64)
  assert np.abs(l1_old - _scene_numpy(x, w1, b1, act)).max() < SCENE_GUARD
  assert _same_bits(l1, l1_old)
  l2 = built_lib.op_scene_conv(l1, w2, b2, act=act)
  l2_old = built_lib.op_scene_conv(l1, w2, b2, act=act, per_output=True)
  assert l2.shape == (2, 9, 16, 64)
  assert np.abs(l2_old - _scene_numpy(l1, w2, b2, act)).max() < SCENE_GUARD
  assert _same_bits(l2, l2_old)


@pytest.mark.gpu
def test_scene_conv_refused_shape_runs_the_old_kernel(built_lib):
  """A shape the plan keeps on the per-output kernel gives that kernel's bits by either door."""
  x, w, b = _scene_case(np.random.default_rng(3), 2, 7, 9, 11, 32)
  assert built_lib.scene_conv_form(3, 11, 32) == "per_output"
  assert _same_bits(built_lib.op_scene_conv(x, w, b), built_lib.op_scene_conv(x, w, b, per_output=True))
