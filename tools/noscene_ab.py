#!/usr/bin/env python
# coding=utf-8
"""Same-session A/B of the greedy forward: the model built WITHOUT the scene encoder
(--use_scene_enc off) against the published model, on cfg-1 shapes (batch 64, both scales,
f16x3, hipGraph replay), timed with mv_time_greedy_resident (inputs resident in HBM).

    python tools/noscene_ab.py [--iters 50] [--reps 5]

Prints one JSON line: trajectories per second of each model (best of --reps timed runs,
alternating the two models so that clocks and neighbours affect both alike) and the ratio."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multiverse_amd import _lib, synth  # noqa: E402


def engine(use_scene_enc):
  cfg = synth.default_config(batch_size=64, use_grids=(1, 1), use_scene_enc=use_scene_enc)
  eng = _lib.Engine(cfg, device=0)
  eng.set_params(synth.make_params(cfg, seed=synth.SEED_BASE + 2))
  eng.set_compute_mode("f16x3")
  eng.set_graph_mode(True)
  eng.upload(synth.make_feed(cfg, seed=synth.SEED_BASE + 2))
  return cfg, eng


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--iters", type=int, default=50)
  ap.add_argument("--reps", type=int, default=5)
  ap.add_argument("--only", choices=["noscene", "published"], default=None,
                  help="time one model only (e.g. under a profiler)")
  a = ap.parse_args()
  models = {"published": engine(True), "noscene": engine(False)}
  if a.only:
    models = {a.only: models[a.only]}
  best = {}
  for name, (_, eng) in models.items():
    eng.time_resident(5)                       # warm-up: graph capture, packs, tables
  for _ in range(a.reps):
    for name, (cfg, eng) in models.items():
      ms = eng.time_resident(a.iters) / a.iters
      best[name] = min(best.get(name, 1e30), ms)
  out = {name: {"ms_per_forward": ms, "traj_per_s": 64 * 1000.0 / ms}
         for name, ms in best.items()}
  if len(out) == 2:
    out["noscene_over_published"] = out["noscene"]["traj_per_s"] / out["published"]["traj_per_s"]
  print(json.dumps(out))
  for _, eng in models.values():
    eng.close()


if __name__ == "__main__":
  main()
