# coding=utf-8
"""Inputs, fp64 reference and bounds of the optimizer-apply parity tests
(test_gpu_optimizer_apply.py on the GPU, test_optimizer_cases_host.py on the host).

The last stage of a training step (csrc/engine_train.h train_apply: learning rate, scale,
element-wise clip, one of the four optimizer kernels of csrc/train_kernels.h, Adam's beta powers,
global_step) is element-wise, so it can be handed a gradient of which the reference knows every
value.  This module holds what both halves need and nothing that touches the GPU:

  inputs       weights, gradients and slots drawn per parameter (`make_inputs`)
  reference    `reference_run`: oracle.apply_optimizer / oracle.learning_rate over successive
               applies, the scale and the clip as oracle.train_step states them (scale first, in
               float32 like the kernel's operand, then np.clip), in float64 (the expected value)
               or float32 (a correctly rounded fp32 implementation: it sets the tolerance)
  bounds       `error_constants`: the error of a result against the fp64 run in units of
               2^-24 * path (parameters, path = |w0| + sum |dw|) and 2^-24 * |ref| (slots)
  device model `device_model_run`: a float32 numpy restatement of the four kernels, with switches
               that make it wrong the way a kernel could be (FAULTS); the host test shows that
               the bounds pass the right model and fail each wrong one
"""
import copy

import numpy as np

from multiverse_amd import synth
from oracle import multiverse_oracle as oracle

OPTIMIZERS = ("adadelta", "momentum", "adam", "rmsprop")
NUM_SLOTS = {"adadelta": 2, "momentum": 1, "adam": 2, "rmsprop": 2}
# (grad_scale, clip): the plain step; a data-parallel mean that is no power of two, clipped; a
# power-of-two scale with the clip off
SCALE_CLIP = ((1.0, 10.0), (1.0 / 3.0, 10.0), (0.125, None))
# a sane step size per optimizer (the default 0.3 is Adadelta's)
INIT_LR = {"adadelta": 0.3, "momentum": 0.01, "adam": 0.001, "rmsprop": 0.001}
ADAM_START_POWERS = (np.float32(0.9 ** 5), np.float32(0.999 ** 5))
U = 2.0 ** -24                     # unit roundoff of float32
GPU_FACTOR = 4.0                   # the GPU may use 4 x the fp32 oracle's own constant ...
ORACLE_CEILING = 16.0              # ... which has to stay below this, else the INPUT is bad
# Single elements (corners, Adam's alpha) have no fp32 constant worth measuring (a lone element is
# often exact): they use the ceiling itself.  The longest chain to a parameter (Adadelta) is 11
# roundings of at most 2^-24 each, relative to intermediate values no larger than the path.
CORNER_C = 16.0
TINY = 1e-30                       # slots at or below this: an absolute bound of TINY
PAD_SENTINEL = np.float32(-7.5e8)  # in the gradient buffer's pad elements
SEED = 20241021


def base_config(single_decoder=False, **over):
  """The batch-2, hidden-128 training engine of every test here: both grids, two predicted
  steps.  single_decoder: --use_single_decoder, the one wiring with no_grad parameters (the
  regression encoders exist, are not trained: csrc/engine_setup.h)."""
  kw = dict(batch_size=2, use_grids=(1, 1), is_train=True, enc_hidden_size=128,
            dec_hidden_size=128, pred_len=2, use_single_decoder=single_decoder,
            train_num_examples=2)        # decay_steps = 2: the staircase moves at step 2
  kw.update(over)
  return synth.default_config(**kw)


def optimizer_config(cfg, optimizer, clip=10.0, **over):
  c = copy.copy(cfg)
  c.optimizer = optimizer
  c.init_lr = INIT_LR[optimizer]
  c.clip_gradient_norm = clip
  for k, v in over.items():
    setattr(c, k, v)
  return c


def is_no_grad(cfg, name):
  return bool(getattr(cfg, "use_single_decoder", False)) and "encoder_grid_reg" in name


def layout(specs):
  """[(name, shape, offset, size)] and the element count of the flat gradient buffer: parameters
  in param_specs() order, each offset padded up to a multiple of 64 elements."""
  out, off = [], 0
  for name, shape in specs:
    size = int(np.prod(shape))
    out.append((name, tuple(shape), off, size))
    off += (size + 63) // 64 * 64
  return out, off


def flat_gradients(specs, grads, fill=PAD_SENTINEL):
  """The flat buffer holding grads[name] at each parameter's offset and `fill` elsewhere."""
  lay, total = layout(specs)
  flat = np.full(total, fill, dtype=np.float32)
  for name, shape, off, size in lay:
    flat[off:off + size] = np.asarray(grads[name], dtype=np.float32).reshape(-1)
  return flat


def make_inputs(specs, optimizer, seed=SEED):
  """{name: (w, g, slot0, slot1)} float32, seeded per parameter.  Weights N(0, 0.05); gradients
  N(0,1) * 10^U(-6, 1.5): some clipped at 10, most not; slot 0 |N(0, 1e-2)|, slot 1 |N(0, 1e-4)|.
  momentum / adam: slot 0 carries the gradient's sign (accum * 0.9 + g and m + (g - m) * 0.1
  would otherwise cancel, and no fp32 implementation is close to fp64 there); rmsprop: slot 0 is
  1 + that (ms starts at one), slot 1 zero."""
  out = {}
  for i, (name, shape) in enumerate(specs):
    rng = np.random.default_rng([seed, i])
    w = rng.normal(0.0, 0.05, shape).astype(np.float32)
    g = (rng.normal(0.0, 1.0, shape) * 10.0 ** rng.uniform(-6.0, 1.5, shape)).astype(np.float32)
    s0 = np.abs(rng.normal(0.0, 1e-2, shape)).astype(np.float32)
    s1 = np.abs(rng.normal(0.0, 1e-4, shape)).astype(np.float32)
    if optimizer in ("momentum", "adam"):
      s0 = np.copysign(s0, g)
    if optimizer == "rmsprop":
      s0, s1 = (np.float32(1) + s0).astype(np.float32), np.zeros_like(s1)
    out[name] = (w, g, s0, s1)
  return out


def zero_slots(optimizer, shape):
  """The slots as train_init creates them (RMSProp's ms = ones)."""
  z = np.zeros(shape, np.float32)
  return (np.ones(shape, np.float32) if optimizer == "rmsprop" else z, z.copy())


def _powers_after(powers):
  return (np.float32(powers[0]) * np.float32(0.9), np.float32(powers[1]) * np.float32(0.999))


def reference_run(cfg, inputs, grad_scale, steps, npd, step0=0, powers=None, skip=()):
  """`steps` successive applies of the SAME gradients, as oracle.train_step does one:
  -> [per apply: {"params": {name: array}, "slots": {name: tuple}, "powers": (b1p, b2p) | None,
                  "lr": float, "step": global_step after}].  Parameters in `skip` (no_grad) pass
  through untouched.  npd float64 is the expected value; float32 measures correct rounding."""
  nsl = NUM_SLOTS[cfg.optimizer]
  params = {n: v[0] for n, v in inputs.items()}
  slots = {n: tuple(v[2:2 + nsl]) for n, v in inputs.items()}
  if cfg.optimizer == "adam" and powers is None:
    powers = (np.float32(0.9), np.float32(0.999))
  out = []
  for k in range(steps):
    lr = oracle.learning_rate(cfg, step0 + k)
    new_p, new_s = {}, {}
    for n, v in inputs.items():
      if n in skip:
        new_p[n], new_s[n] = params[n], slots[n]
        continue
      g = v[1].astype(npd) * npd(np.float32(grad_scale))
      if cfg.clip_gradient_norm is not None:
        g = np.clip(g, -cfg.clip_gradient_norm, cfg.clip_gradient_norm)
      new_p[n], new_s[n] = oracle.apply_optimizer(cfg, lr, params[n], g, slots[n], npd, powers)
    params, slots = new_p, new_s
    if cfg.optimizer == "adam":
      powers = _powers_after(powers)
    out.append({"params": params, "slots": slots, "lr": lr, "step": step0 + k + 1,
                "powers": powers if cfg.optimizer == "adam" else None})
  return out


def paths(inputs, ref64):
  """Per apply k: {name: |w0| + sum_{j <= k} |dw_ref64|}, the magnitude a parameter's roundings
  are relative to."""
  out, acc = [], {n: np.abs(v[0].astype(np.float64)) for n, v in inputs.items()}
  prev = {n: v[0].astype(np.float64) for n, v in inputs.items()}
  for st in ref64:
    acc = {n: acc[n] + np.abs(np.asarray(st["params"][n], np.float64) - prev[n]) for n in acc}
    prev = {n: np.asarray(st["params"][n], np.float64) for n in acc}
    out.append(acc)
  return out


def param_constant(got, ref, path):
  """max |got - ref| / (2^-24 path) over one tensor."""
  d = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
  with np.errstate(divide="ignore", invalid="ignore"):
    r = np.where(d == 0, 0.0, d / (U * path))
  return float(np.max(r)) if r.size else 0.0


def slot_constant(got, ref):
  """(max |got - ref| / (2^-24 |ref|) over the elements with |ref| > TINY, max |got - ref| over
  the rest)."""
  got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
  d = np.abs(got - ref)
  big = np.abs(ref) > TINY
  rel = float(np.max(d[big] / (U * np.abs(ref[big])))) if big.any() else 0.0
  small = float(np.max(d[~big])) if (~big).any() else 0.0
  return rel, small


def _worse(a, b):
  """max that keeps a NaN (which then fails every <=)."""
  return float("nan") if (np.isnan(a) or np.isnan(b)) else max(a, b)


def error_constants(got_params, got_slots, ref64_step, path, nslots, skip=()):
  """-> (c_p, c_s, worst absolute error of a tiny slot element) of one apply over every element
  of every parameter.  NaN anywhere gives NaN (which fails every <=)."""
  c_p, c_s, tiny = 0.0, 0.0, 0.0
  for n, ref in ref64_step["params"].items():
    if n in skip:
      continue
    c_p = _worse(c_p, param_constant(got_params[n], ref, path[n]))
    for i in range(nslots):
      rel, small = slot_constant(got_slots[n][i], ref64_step["slots"][n][i])
      c_s, tiny = _worse(c_s, rel), _worse(tiny, small)
  return c_p, c_s, tiny


def within_bounds(gpu, oracle32):
  """The acceptance rule for (c_p, c_s, tiny) triples: the fp32 oracle itself is well
  conditioned (<= ORACLE_CEILING), and the result under test stays within GPU_FACTOR times the
  oracle's constants; tiny slot elements within TINY."""
  ok_input = oracle32[0] <= ORACLE_CEILING and oracle32[1] <= ORACLE_CEILING
  return bool(ok_input and gpu[0] <= GPU_FACTOR * oracle32[0] and
              gpu[1] <= GPU_FACTOR * oracle32[1] and gpu[2] <= TINY)


# ---------------------------------------------------------------- the device, restated
FAULTS = ("adam_eps_1e-7", "clip_before_scale", "stale_beta_power", "slots_swapped")


def device_model_run(cfg, inputs, grad_scale, steps, step0=0, powers=None, fault=None,
                     nan_dropping_clip=False):
  """The four kernels of csrc/train_kernels.h and train_apply's host arithmetic in float32
  numpy, operation for operation (not the oracle's association: sqrt(a) * (1 / sqrt(b)) * g as
  the kernel writes it).  Same return shape as reference_run.  fault: one of FAULTS, a model
  that is wrong the way a kernel could be; nan_dropping_clip: the fminf(fmaxf()) clip the
  kernels had, which turns a NaN into -clip."""
  f = np.float32
  opt = cfg.optimizer
  nsl = NUM_SLOTS[opt]
  params = {n: v[0].copy() for n, v in inputs.items()}
  slots = {n: [v[2].copy(), v[3].copy()] for n, v in inputs.items()}
  if powers is None:
    powers = (f(0.9), f(0.999))
  b1p, b2p = f(powers[0]), f(powers[1])
  clip = cfg.clip_gradient_norm
  out = []
  for k in range(steps):
    lr = f(oracle.learning_rate(cfg, step0 + k))
    pw = (b1p * f(0.9), b2p * f(0.999)) if fault == "stale_beta_power" else (b1p, b2p)
    with np.errstate(all="ignore"):
      alpha = lr * np.sqrt(f(1) - pw[1]) / (f(1) - pw[0])
      for n, v in inputs.items():
        g = v[1]
        if fault == "clip_before_scale" and clip is not None:
          g = np.clip(g, f(-clip), f(clip))
        g = g * f(grad_scale)
        if clip is not None and fault != "clip_before_scale":
          if nan_dropping_clip:
            g = np.fmin(np.fmax(g, f(-clip)), f(clip))     # fmaxf(NaN, -clip) = -clip
          else:
            g = np.where(g < f(-clip), f(-clip), np.where(g > f(clip), f(clip), g)).astype(f)
        s0, s1 = slots[n]
        if fault == "slots_swapped":
          s0, s1 = s1, s0
        w = params[n]
        if opt == "adadelta":
          rho, eps = f(0.95), f(1e-8)
          a = s0 * rho + g * g * (f(1) - rho)
          upd = np.sqrt(s1 + eps) * (f(1) / np.sqrt(a + eps)) * g
          w = w - upd * lr
          s0, s1 = a, s1 * rho + upd * upd * (f(1) - rho)
        elif opt == "momentum":
          a = s0 * f(0.9) + g
          w = w - a * lr
          s0 = a
        elif opt == "adam":
          eps = f(1e-7) if fault == "adam_eps_1e-7" else f(1e-8)
          mm = s0 + (g - s0) * (f(1) - f(0.9))
          vv = s1 + (g * g - s1) * (f(1) - f(0.999))
          w = w - (mm * alpha) / (np.sqrt(vv) + eps)
          s0, s1 = mm, vv
        else:
          s2 = s0 + (g * g - s0) * (f(1) - f(0.9))
          mo = s1 * f(0.0) + (g * lr) * (f(1) / np.sqrt(s2 + f(1e-10)))
          w = w - mo
          s0, s1 = s2, mo
        if fault == "slots_swapped":
          s0, s1 = s1, s0
        params[n], slots[n] = w.astype(f), [np.asarray(s0, f), np.asarray(s1, f)]
    if opt == "adam":
      b1p, b2p = b1p * f(0.9), b2p * f(0.999)
    out.append({"params": dict(params), "slots": {n: tuple(s[:nsl]) for n, s in slots.items()},
                "lr": float(lr), "step": step0 + k + 1,
                "powers": (b1p, b2p) if opt == "adam" else None})
  return out


# ---------------------------------------------------------------- corners
def next_up(x):
  return np.nextafter(np.float32(x), np.float32(np.inf))


def next_down(x):
  return np.nextafter(np.float32(x), np.float32(-np.inf))


CLIP = 10.0
# name -> (grad_scale, clip, gradient values).  One apply per entry: the optimizers are
# element-wise, so every value is a case of its own.
CORNER_CASES = {
    # g * scale exactly +-clip, one float32 beyond and one inside; +-inf clip to +-clip; NaN stays
    "boundary": (1.0, CLIP, [0.0, -0.0, CLIP, -CLIP, next_up(CLIP), next_down(CLIP),
                             -next_up(CLIP), -next_down(CLIP), np.inf, -np.inf, 1.0, np.nan,
                             -3.0]),
    # clipped only if the SCALED value exceeds clip: 3 clip + tiny with scale 1/3 lands on clip
    # (a kernel that clips first gives clip / 3); 29 and -29.5 stay unclipped
    "scale_third": (1.0 / 3.0, CLIP, [next_up(3 * CLIP), -next_up(3 * CLIP), 29.0, -29.5, 0.5]),
    # 0.9 clip with scale 2 must be clipped (a kernel that clips first gives 1.8 clip)
    "scale_two": (2.0, CLIP, [0.9 * CLIP, -0.9 * CLIP, 4.0, np.inf]),
    # clip off: the full value, and a NaN stays a NaN here too
    "clip_off": (1.0, None, [1e6, -1e6, 0.25, np.nan, 0.0, -0.0]),
}
CORNER_LR = 2.0 ** -6      # a power of two: momentum's w - lr * g has ONE rounding


def corner_inputs(optimizer, name, size, case):
  """One parameter of `size` elements: the case's values first, N(0,1) gradients after
  (neighbours that must stay right), weights N(0, 0.05), slots as train_init leaves them."""
  _, _, vals = CORNER_CASES[case]
  rng = np.random.default_rng([SEED, 77, sorted(CORNER_CASES).index(case)])
  assert len(vals) < size
  g = rng.normal(0.0, 1.0, size).astype(np.float32)
  g[:len(vals)] = np.asarray(vals, dtype=np.float32)
  w = rng.normal(0.0, 0.05, size).astype(np.float32)
  s0, s1 = zero_slots(optimizer, (size,))
  return {name: (w, g, s0, s1)}
