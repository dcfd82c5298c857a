# coding=utf-8
"""The greedy forwards that tests/test_gpu_chain_streams.py compares between MV_CHAIN_STREAMS=1
(one launch stream, the order of before) and =2 (class chains and regression chains as two
chain pairs on two streams).  The switch is read once per process, so the test runs this file
once per value:

    MV_CHAIN_STREAMS=<1|2> python tests/chain_streams_cases.py OUT.npz

and compares the two files byte for byte.  Nothing here asserts; every array a case produces
goes into OUT.npz under "<case>/<name>", the kernel statistics of one profiled headline step
as JSON under "stats"."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from multiverse_amd import _lib, synth  # noqa: E402

# bench.py's literal 36x18 / 18x9 grids: 18 and 9 columns, the halo tiling of the F(3,3) tile
LITERAL_GRIDS = dict(scene_h=72, scene_w=36, scene_grids=[(36, 18), (18, 9)])

N_FEEDS = 20

# name -> (default_config arguments, compute mode)
CASES = {
    "headline": (dict(batch_size=64, use_grids=(1, 1)), "f16x3"),
    "f32": (dict(batch_size=64, use_grids=(1, 1)), "f32"),
    "bf16": (dict(batch_size=64, use_grids=(1, 1)), "bf16"),
    "scale0_only": (dict(batch_size=5, use_grids=(1, 0)), "f16x3"),
    "scale1_only": (dict(batch_size=5, use_grids=(0, 1)), "f16x3"),
    "single_decoder": (dict(batch_size=5, use_grids=(1, 1), use_single_decoder=True), "f16x3"),
    "no_gnn": (dict(batch_size=5, use_grids=(1, 1), use_gnn=False), "f16x3"),
    "no_scene_enc": (dict(batch_size=5, use_grids=(1, 1), use_scene_enc=False), "f16x3"),
    "literal_grids": (dict(batch_size=5, use_grids=(1, 1), **LITERAL_GRIDS), "f16x3"),
    "literal_grids_bf16": (dict(batch_size=5, use_grids=(1, 1), **LITERAL_GRIDS), "bf16"),
    "relu_f16x3": (dict(batch_size=5, use_grids=(1, 1), activation_func="relu"), "f16x3"),
}


def put(out, case, name, pair):
  cls, reg = pair
  for s in range(len(cls)):
    if not isinstance(cls[s], np.ndarray):      # a scale the model does not use
      continue
    out["%s/%s/cls%d" % (case, name, s)] = np.ascontiguousarray(cls[s])
    out["%s/%s/reg%d" % (case, name, s)] = np.ascontiguousarray(reg[s])


def main():
  out = {}
  stats = None
  for case, (kw, mode) in CASES.items():
    cfg = synth.default_config(**kw)
    params = synth.make_params(cfg, recurrent_gain=3.0, bias_scale=0.1)
    eng = _lib.Engine(cfg, device=0)
    eng.set_params(params)
    eng.set_compute_mode(mode)
    n_feeds = N_FEEDS if case == "headline" else 3
    feeds = [synth.make_feed(cfg, seed=synth.SEED_BASE + 300 + k) for k in range(n_feeds)]
    # forwards back to back on changing feeds: the second run_resident of a feed is queued
    # behind the first without a host synchronisation between them
    for k, feed in enumerate(feeds):
      eng.upload(feed)
      eng.run_resident(False)
      eng.run_resident(False)
      put(out, case, "resident%d" % k, eng.download())
    # the same feeds through the feed / compute / fetch pipeline
    for k, pair in enumerate(eng.forward_greedy_pipelined(feeds)):
      put(out, case, "pipelined%d" % k, pair)
    if case == "headline":
      eng.upload(feeds[0])
      eng.set_profiling(True)
      eng.reset_kernel_stats()
      eng.run_resident(False)
      eng.synchronize()
      stats = eng.kernel_stats()
      eng.set_profiling(False)
      # and an un-profiled forward right after the profiled one
      eng.run_resident(False)
      put(out, case, "after_profile", eng.download())
    eng.close()
  for st in stats.values():
    del st["total_ms"]
  out["stats"] = np.frombuffer(json.dumps(stats, sort_keys=True).encode(), dtype=np.uint8)
  np.savez(sys.argv[1], **out)
  print("[chain_streams_cases] MV_CHAIN_STREAMS=%s: %d arrays" %
        (os.environ.get("MV_CHAIN_STREAMS", "(unset)"), len(out)))


if __name__ == "__main__":
  main()
