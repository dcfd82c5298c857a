#!/usr/bin/env python
# coding=utf-8
"""Same-session A/B of the greedy forward's launch structure: MV_CHAIN_STREAMS=1 (every launch
on one stream) against 2 (class chains and regression chains as two chain pairs on two
streams), optionally 2 with MV_CHAIN_PRIORITY=1 (the regression pair's stream at the lowest
priority).  The switches are read once per process, so every run is a fresh `python bench.py`
process; the variants alternate so that clocks and neighbours affect all alike.

    python tools/chain_streams_ab.py [--reps 5] [--priority] [--lib-a PATH] [-- bench.py options]

--lib-a PATH: variant A runs another build of the library (MV_LIB_PATH), e.g. the parent
commit's, instead of this tree's with MV_CHAIN_STREAMS=1.

Prints one JSON line: ms_per_step of every run per variant, medians, whether the ranges are
apart (slowest two-stream run faster than the fastest single-stream run) and the ratio of the
medians."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench(env_over, bench_args, timeout):
  env = dict(os.environ)
  env.update(env_over)
  out = subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py")] + bench_args,
                                env=env, stderr=subprocess.DEVNULL, timeout=timeout)
  return json.loads(out.decode().strip().splitlines()[-1])["ms_per_step"]


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--reps", type=int, default=5)
  ap.add_argument("--priority", action="store_true", help="also time MV_CHAIN_PRIORITY=1")
  ap.add_argument("--lib-a", default=None)
  ap.add_argument("--timeout", type=float, default=300.0, help="seconds per bench.py run")
  ap.add_argument("bench_args", nargs="*", help="options passed to bench.py (after --)")
  a = ap.parse_args()
  variants = {"one_stream": {"MV_LIB_PATH": a.lib_a} if a.lib_a else {"MV_CHAIN_STREAMS": "1"},
              "two_streams": {"MV_CHAIN_STREAMS": "2", "MV_CHAIN_PRIORITY": "0"}}
  if a.priority:
    variants["two_streams_priority"] = {"MV_CHAIN_STREAMS": "2", "MV_CHAIN_PRIORITY": "1"}
  ms = {name: [] for name in variants}
  for _ in range(a.reps):
    for name, env in variants.items():      # a failing run ends the A/B (check_output raises)
      ms[name].append(bench(env, a.bench_args, a.timeout))
  out = {"bench_args": a.bench_args, "ms_per_step": ms,
         "median": {name: statistics.median(v) for name, v in ms.items()}}
  for name in variants:
    if name == "one_stream":
      continue
    out[name + "_ranges_apart"] = max(ms[name]) < min(ms["one_stream"])
    out[name + "_speedup"] = out["median"]["one_stream"] / out["median"][name]
  print(json.dumps(out))


if __name__ == "__main__":
  main()
