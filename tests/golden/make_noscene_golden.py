#!/usr/bin/env python
# coding=utf-8
"""Freeze outputs of the reference's UNMODIFIED code/pred_models.py for a model built
WITHOUT the scene encoder (`--use_scene_enc` left out: the reference's default graph) into
tests/golden/golden_shim_noscene_*.npz, in the compact format of
oracle/tf1_shim/make_shim_golden.py.

    python tests/golden/make_noscene_golden.py        # needs the reference checkout

Cases (synthetic weights / inputs from multiverse_amd.synth):
  - greedy Tester.step on both scales, N = 2;
  - beam search on scale 1, N = 2, B = 5, diverse;
  - the reference's own inference configuration on scale 0: batch 1, beam 20, gamma 0.01,
    fix_num_timestep 1;
  - two Trainer.steps on both scales (Adadelta), one with --activation_func relu on scale 1;
  - the variable names / shapes the reference asks tf.get_variable for.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from multiverse_amd import synth  # noqa: E402
from oracle.tf1_shim import run_reference as rr  # noqa: E402
from oracle.tf1_shim.make_shim_golden import digest  # noqa: E402

SEED = synth.SEED_BASE + 60


def config(**kw):
  return synth.default_config(use_scene_enc=False, **kw)


def forward_case(name, cfg, seed):
  params = synth.make_params(cfg, seed=seed, recurrent_gain=3.0, bias_scale=0.1)
  feed = synth.make_feed(cfg, seed=seed)
  cls, reg, beam = rr.forward(cfg, params, feed)
  out = {"seed": np.array([seed]),
         "var_names": np.array(["%s|%s" % (n, ",".join(map(str, s)))
                                for n, s in rr.variable_names()])}
  for s in range(len(cfg.scene_grids)):
    if cfg.use_grids[s]:
      out["cls_%d" % s] = np.asarray(cls[s])
      out["reg_%d" % s] = np.asarray(reg[s])
  if beam is not None:
    out["beam_logits"], out["beam_ids"], out["beam_logprobs"] = [np.asarray(b) for b in beam]
  np.savez_compressed(os.path.join(HERE, name), **out)
  print("wrote", name, {k: v.shape for k, v in out.items()})


def train_case(name, cfg, seed, steps):
  cfg.train_num_examples = 2
  params = synth.make_params(cfg, seed=seed, recurrent_gain=2.0, bias_scale=0.1)
  out = {"seed": np.array([seed]), "steps": np.array([steps])}
  slots, gs = {}, 0
  for step in range(steps):
    feed = synth.make_feed(cfg, seed=seed + 100 + step)
    loss, wd, pgl, grads, params, slots, gs = rr.train_step(cfg, params, feed, slots, gs)
    out["loss_%d" % step] = np.array([loss, wd] + pgl, dtype=np.float64)
    for n in sorted(grads):
      assert grads[n] is not None, n
      out["grad_%d|%s" % (step, n)] = digest(grads[n])
    print(name, "step", step, "loss", loss)
  for n in sorted(params):
    out["param|%s" % n] = digest(params[n])
  for n in sorted(slots):
    for i, sl in enumerate(slots[n]):
      out["slot%d|%s" % (i, n)] = digest(np.asarray(sl))
  out["global_step"] = np.array([gs])
  np.savez_compressed(os.path.join(HERE, name), **out)
  print("wrote", name)


CASES = {
    "greedy_both": lambda: forward_case(
        "golden_shim_noscene_greedy_both.npz", config(batch_size=2, use_grids=(1, 1)), SEED),
    "beam_s1": lambda: forward_case(
        "golden_shim_noscene_beam_s1.npz",
        config(batch_size=2, use_grids=(0, 1), beam_size=5), SEED + 1),
    "beam20_s0": lambda: forward_case(
        "golden_shim_noscene_beam20_s0.npz",
        config(batch_size=1, use_grids=(1, 0), beam_size=20), SEED + 2),
    "train_both": lambda: train_case(
        "golden_shim_noscene_train_both.npz",
        config(batch_size=2, use_grids=(1, 1), is_train=True), SEED + 3, 2),
    "train_relu": lambda: train_case(
        "golden_shim_noscene_train_relu.npz",
        config(batch_size=2, use_grids=(0, 1), is_train=True, activation_func="relu"),
        SEED + 4, 1),
}


def main():
  assert rr.available(), "needs the reference checkout"
  for name in (sys.argv[1:] or list(CASES)):
    CASES[name]()


if __name__ == "__main__":
  main()
