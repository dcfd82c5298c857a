#!/usr/bin/env python
"""Grouped against ragged batches of a multi-future beam decode (batch 128, scale 0, diverse
beam 20, f16x3, hipGraph on, device decode with the occupancy map), on a synthetic set whose
prediction lengths are drawn uniformly from 14..25:

  grouped  samples grouped by T_pred, every group's last batch padded to the batch size
           (the schedule of multifuture.run_inference without --ragged_batches)
  ragged   multifuture.plan_ragged_batches: sorted by length, one length per row, the last
           batch padded with length-0 rows (--ragged_batches)

Each schedule is timed in fresh processes of one session, alternating (A B A B ...); a process
runs its schedule once to warm up (weight packs, graph captures) and then `--reps` times.
Prints one JSON line; --write_md PATH also writes the table of profiles/ragged_batches_ab.md."""
import argparse
import collections
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def lengths_of(a):
  return np.random.default_rng(a.seed).integers(14, 26, size=a.samples).tolist()


def schedule(kind, lens, N):
  """[(pred_length, row lengths or None, real rows)]"""
  from multiverse_amd import multifuture as mf
  if kind == "ragged":
    return [(T, l, len(idxs)) for idxs, l, T in mf.plan_ragged_batches(lens, N).batches]
  groups = collections.Counter(lens)
  return [(T, None, min(N, groups[T] - lo)) for T in sorted(groups)
          for lo in range(0, groups[T], N)]


def child(a):
  from multiverse_amd import multifuture as mf, pred_models, synth
  N, B = a.batch, a.beam
  cfg = synth.default_config(batch_size=N, use_grids=(1, 0), beam_size=B)
  cfg.max_pred_len = 25
  cfg.compute_mode = "f16x3"
  model = pred_models.Model(cfg, "model")
  model.load_params(synth.make_params(cfg, seed=synth.SEED_BASE + 2, recurrent_gain=3.0,
                                      bias_scale=0.1))
  model.engine.set_graph_mode(True)
  feed = synth.make_feed(cfg, seed=synth.SEED_BASE + 2)     # one batch of inputs, reused
  centers = mf.add_grid(argparse.Namespace(
      grid_strides="2,4", use_grids=[True, False], scene_h=36, scene_w=64, video_h=1080,
      video_w=1920)).scene_grid_centers
  lens = lengths_of(a)
  plan = schedule(a.child, lens, N)

  def one_pass():
    for T, row_lengths, _ in plan:
      f = dict(feed, pred_length=T)
      if row_lengths is not None:
        f["pred_lengths"] = row_lengths
      model.run_forward_decoded(f, occupancy=True, grid_centers=centers)
  one_pass()
  times = []
  for _ in range(a.reps):
    t0 = time.perf_counter()
    one_pass()
    times.append(time.perf_counter() - t0)
  model.close()
  print(json.dumps({"kind": a.child, "batches": len(plan), "seconds": times}))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--batch", type=int, default=128)
  ap.add_argument("--beam", type=int, default=20)
  ap.add_argument("--samples", type=int, default=512)
  ap.add_argument("--seed", type=int, default=20260)
  ap.add_argument("--reps", type=int, default=2)
  ap.add_argument("--rounds", type=int, default=2, help="fresh processes per schedule")
  ap.add_argument("--child", choices=["grouped", "ragged"], default=None)
  ap.add_argument("--write_md", default=None)
  a = ap.parse_args()
  if a.child:
    return child(a)
  from multiverse_amd import multifuture as mf
  lens = lengths_of(a)
  plan = mf.plan_ragged_batches(lens, a.batch)
  best = {"grouped": [], "ragged": []}
  batches = {}
  for _ in range(a.rounds):
    for kind in ("grouped", "ragged"):
      cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--batch", str(a.batch),
             "--beam", str(a.beam), "--samples", str(a.samples), "--seed", str(a.seed),
             "--reps", str(a.reps)]
      out = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=600).stdout.decode()
      rec = json.loads(out.strip().splitlines()[-1])
      best[kind] += rec["seconds"]
      batches[kind] = rec["batches"]
  res = {
      "batch": a.batch, "beam": a.beam, "samples": a.samples, "seed": a.seed,
      "lengths": "uniform 14..25", "unit": "trajectories/sec",
      "grouped": round(a.samples / min(best["grouped"]), 1),
      "ragged": round(a.samples / min(best["ragged"]), 1),
      "grouped_seconds": [round(x, 3) for x in best["grouped"]],
      "ragged_seconds": [round(x, 3) for x in best["ragged"]],
      "grouped_batches": batches["grouped"], "ragged_batches": batches["ragged"],
      "grouped_row_steps": plan.grouped_row_steps, "ragged_row_steps": plan.ragged_row_steps,
  }
  res["row_step_ratio"] = round(plan.grouped_row_steps / plan.ragged_row_steps, 3)
  res["time_ratio"] = round(min(best["grouped"]) / min(best["ragged"]), 3)
  print(json.dumps(res))
  if a.write_md:
    with open(a.write_md, "w") as f:
      f.write(MD % res)


MD = """# Grouped against ragged batches of the multi-future beam decode

`python tools/ragged_batches_ab.py --write_md profiles/ragged_batches_ab.md` on one MI355X: batch
%(batch)d, scale 0 (18x32), diverse beam %(beam)d, f16x3, graph mode on, device decode with the
occupancy map; %(samples)d synthetic samples, prediction lengths drawn uniformly from 14..25
(seed %(seed)d).  Fresh processes of one session, alternating; best pass of each schedule.  The
grouped schedule is the one the parent commit runs.

| schedule | batches | decoder row-steps | seconds (all passes) | trajectories/s |
|---|---|---|---|---|
| grouped by T_pred (every group's last batch padded) | %(grouped_batches)d | %(grouped_row_steps)d | %(grouped_seconds)s | %(grouped)s |
| ragged (`--ragged_batches`, one length per row) | %(ragged_batches)d | %(ragged_row_steps)d | %(ragged_seconds)s | %(ragged)s |

Row-step ratio grouped / ragged: %(row_step_ratio)s.  Time ratio grouped / ragged: %(time_ratio)s.
"""


if __name__ == "__main__":
  main()
