# coding=utf-8
"""Mixed-length training step (mv_set_train_lengths) at the train_n32 shapes
(bench.py configs[2]: batch 32, both scales, f16x3, resident batch): ms per step of
  parent   (a) the uniform step of the library MV_LIB_PATH names (the parent commit's build)
  change   (b) the built library without lengths and (c) with sorted half-and-half lengths --
           rows 0 - 15 at (8, 12), rows 16 - 31 at (4, 6) -- alternating on one handle, the
           row counts of both, then one profiled step each (mv_kernel_stat)
One process and one JSON line per call; run the two as alternating fresh processes in one
session from the repository root (profiles/train_lengths_ab.md)."""
import json, os, sys, time
sys.path.insert(0, os.getcwd())
import numpy as np
from multiverse_amd import _lib, synth

which = sys.argv[1]                       # "parent" | "change"
REPS, STEPS, WARM = 4, 20, 3
cfg = synth.default_config(batch_size=32, use_grids=(1, 1), is_train=True)
params = synth.make_params(cfg, seed=synth.SEED_BASE + 2)
feed = synth.make_feed(cfg, seed=synth.SEED_BASE + 2)
LO = [8] * 16 + [4] * 16
LP = [12] * 16 + [6] * 16

def engine():
  eng = _lib.Engine(cfg, device=0)
  eng.set_params(params)
  eng.upload(feed)
  eng.set_compute_mode("f16x3")
  eng.train_init()
  eng.upload_targets(feed)
  return eng

def timed(eng):
  for _ in range(WARM):
    eng.train_step(None)
  eng.synchronize()
  t0 = time.perf_counter()
  for _ in range(STEPS):
    eng.train_step(None)
  eng.synchronize()
  return 1e3 * (time.perf_counter() - t0) / STEPS

out = {"which": which, "lib": os.environ.get("MV_LIB_PATH", "built"), "figures": {}}
eng = engine()
if which == "parent":
  out["figures"]["a"] = [timed(eng) for _ in range(REPS)]
else:
  fb, fc = [], []
  for _ in range(REPS):                   # (b) and (c) alternate on ONE handle
    eng.set_train_lengths(None, None)
    fb.append(timed(eng))
    rows_b = eng.last_train_gate_rows()
    eng.set_train_lengths(LO, LP)
    fc.append(timed(eng))
    rows_c = eng.last_train_gate_rows()
  out["figures"]["b"], out["figures"]["c"] = fb, fc
  out["gate_rows"] = {"b": rows_b, "c": rows_c}
  # per-kernel tables: one profiled step each, a run of its own after the timed ones
  for tag, lens in (("b", (None, None)), ("c", (LO, LP))):
    eng.set_train_lengths(*lens)
    eng.train_step(None)
    eng.set_profiling(True)
    eng.reset_kernel_stats()
    eng.train_step(None)
    eng.synchronize()
    st = eng.kernel_stats()
    eng.set_profiling(False)
    out["kernels_" + tag] = {k: {"launches": v["launches"], "ms": round(v["total_ms"], 4)}
                            for k, v in sorted(st.items(), key=lambda kv: -kv[1]["total_ms"])}
eng.close()
print(json.dumps(out))
