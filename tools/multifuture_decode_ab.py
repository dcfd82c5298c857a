#!/usr/bin/env python
"""Host-inclusive rate of one multi-future beam decode at the configs[3] shapes (batch 128,
scale 0, diverse beam 20, T_pred 12, synthetic feed, f16x3, hipGraph), two ways, in ONE
process, alternating:

  (a) host tail   Model.run_forward (every beam's logits, the offsets and best_beam over
                  PCIe) + multifuture.decode_trajectories for every row + the numpy occupancy
                  mixture of multifuture.eval_grid_nll for every step
  (b) device tail Model.run_forward_decoded(occupancy=True): trajectories, ids,
                  log-probabilities and the occupancy map only

plus the resident rate (mv_time_beam_resident: no feed, no fetch) and, from a profiled call,
the beam_occupancy kernel's time against the HBM roofline.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multiverse_amd import multifuture as mf, pred_models, synth  # noqa: E402

HBM_PEAK = 8.0e12      # bytes / s, MI355X


def host_tail(model, feed, args, N, T):
  cls, reg, beam = model.run_forward(feed)
  trajs = [mf.decode_trajectories(args, cls[0][n], reg[0][n],
                                  (beam[0][n], beam[1][n], beam[2][n]), T, 0)
           for n in range(N)]
  occ = []
  for n in range(N):                       # the lines of eval_grid_nll, every step
    probs = mf._softmax(np.squeeze(beam[2][n][None]))
    beams = mf._softmax(np.squeeze(beam[0][n][None]), axis=-1)
    occ.append((beams.astype("float32") * probs[:, None, None].astype("float32")).sum(0))
  return trajs, occ


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--batch", type=int, default=128)
  ap.add_argument("--beam", type=int, default=20)
  ap.add_argument("--reps", type=int, default=5)
  ap.add_argument("--resident_iters", type=int, default=10)
  a = ap.parse_args()
  N, B, T = a.batch, a.beam, 12
  cfg = synth.default_config(batch_size=N, use_grids=(1, 0), beam_size=B)
  cfg.compute_mode = "f16x3"
  model = pred_models.Model(cfg, "model")
  model.load_params(synth.make_params(cfg, seed=synth.SEED_BASE + 2, recurrent_gain=3.0,
                                      bias_scale=0.1))
  eng = model.engine
  eng.set_graph_mode(True)
  feed = synth.make_feed(cfg, seed=synth.SEED_BASE + 2)
  args = mf.add_grid(argparse.Namespace(
      grid_strides="2,4", use_grids=[True, False], scene_h=36, scene_w=64, video_h=1080,
      video_w=1920, greedy=False, center_only=False, num_out=B))
  dev = lambda: model.run_forward_decoded(feed, occupancy=True,
                                          grid_centers=args.scene_grid_centers)
  host = lambda: host_tail(model, feed, args, N, T)
  # warm-up (graph capture, packs) and the two paths against each other
  trajs, occ = host()
  d = dev()
  same = bool((np.asarray(trajs) == d["trajs"]).all())
  occ_err = float((np.abs(np.asarray(occ) - d["occupancy"]) / np.asarray(occ)).max())
  t = {"host": [], "device": []}
  for _ in range(a.reps):
    for name, fn in (("host", host), ("device", dev)):
      t0 = time.perf_counter()
      fn()
      t[name].append(time.perf_counter() - t0)
  res_ms = min(eng.time_resident(a.resident_iters, beam=True) / a.resident_iters
               for _ in range(3))
  eng.set_profiling(True)
  eng.reset_kernel_stats()
  dev()
  st = eng.kernel_stats()
  eng.set_profiling(False)
  ko, kt = st["beam_occupancy"], st["decode_traj"]
  occ_ms = ko["total_ms"] / ko["launches"]
  out = {
      "batch": N, "beam": B, "T_pred": T, "unit": "trajectories/sec", "reps": a.reps,
      "host_tail": round(N / min(t["host"]), 1),
      "device_tail": round(N / min(t["device"]), 1),
      "host_tail_ms": [round(1e3 * x, 1) for x in t["host"]],
      "device_tail_ms": [round(1e3 * x, 1) for x in t["device"]],
      "resident": round(N * 1e3 / res_ms, 1), "resident_ms": round(res_ms, 2),
      "trajectories_bit_identical": same, "occupancy_rel_vs_host_float32": occ_err,
      "beam_occupancy_ms": round(occ_ms, 4),
      "beam_occupancy_MB": round(ko["bytes"] / ko["launches"] / 1e6, 1),
      "beam_occupancy_hbm_fraction": round(ko["bytes"] / ko["launches"] / (occ_ms * 1e-3)
                                           / HBM_PEAK, 3),
      "decode_traj_ms": round(kt["total_ms"] / kt["launches"], 4),
      "d2h_MB_host_tail": round(4e-6 * (N * B * T * 576 + N * T * 576 * 3 + N * B * (T + 1)), 1),
      "d2h_MB_device_tail": round(1e-6 * (16 * N * B * T + 4 * N * B * (T + 1)
                                          + 4 * N * T * 576), 1),
  }
  print(json.dumps(out))
  model.close()


if __name__ == "__main__":
  main()
