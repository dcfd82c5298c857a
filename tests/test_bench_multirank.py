# coding=utf-8
"""CPU: bench.py's multi-rank control flow at N = 8 (the run the driver makes on an 8-GPU node,
which no 1-GPU lease can rehearse): `--gpus 8` with no launcher spawns eight ranks on
127.0.0.1, every rank builds its OWN feed (seed offset 1000 x rank), the timed region is
bracketed by barriers and its length is the MAXIMUM over the ranks, rank 0 prints ONE JSON line
with n_gpus 8 and the whole-job value.  The engine is a stand-in (tests/bench_cpu_harness.py):
what is under test is bench.py and multiverse_amd/parallel.py, over gloo."""
import glob
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "bench_cpu_harness.py")


def _run(tmp_path, workload, n=8, steps=3, batch=2):
  env = dict(os.environ, MV_BENCH_BACKEND="gloo", MV_HARNESS_DIR=str(tmp_path),
             OMP_NUM_THREADS="1", MASTER_ADDR="127.0.0.1")
  for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
    env.pop(k, None)
  r = subprocess.run([sys.executable, HARNESS, "--gpus", str(n), "--steps", str(steps),
                      "--warmup", "1", "--batch", str(batch), "--workload", workload,
                      "--no-cpu-baseline", "--no-fp32-ref"],
                     env=env, capture_output=True, timeout=600)
  assert r.returncode == 0, r.stderr.decode()[-3000:]
  lines = [l for l in r.stdout.decode().splitlines() if l.strip()]
  assert len(lines) == 1, lines                      # ONE line, from rank 0 only
  recs = [json.load(open(f)) for f in sorted(glob.glob(os.path.join(str(tmp_path), "rank*.json")))]
  return json.loads(lines[0]), recs


@pytest.mark.timeout(900)
def test_bench_gpus_8_greedy_control_flow(tmp_path):
  from multiverse_amd import synth
  n, steps, batch = 8, 3, 2
  line, recs = _run(tmp_path, "greedy", n, steps, batch)
  assert line["n_gpus"] == n and line["steps"] == steps and line["warmup"] == 1
  assert line["scaling"] == "weak" and line["higher_is_better"] is True
  assert line["config"]["batch_per_gpu"] == batch and line["config"]["global_batch"] == n * batch
  assert "batch-sharded x8, no data-path collective" in line["config"]["parallelism"]
  # every rank ran, each on its own feed
  assert sorted(r["rank"] for r in recs) == list(range(n))
  for r in recs:
    assert r["feed_seeds"] == [synth.SEED_BASE + 2 + 1000 * r["rank"]]
  # max over ranks: the stand-in's rank r takes 2 (r + 1) ms per step, the line must carry
  # the slowest rank's 16 ms (not rank 0's 2 ms), and value = ALL ranks' trajectories / that
  assert line["ms_per_step"] >= 0.9 * 2.0 * n
  want = n * batch * steps / (line["ms_per_step"] * 1e-3 * steps)
  assert abs(line["value"] - want) <= 0.02 * want
  assert "cpu_baseline" not in line                  # rank 0 at N = 1 only


@pytest.mark.timeout(900)
def test_bench_gpus_8_training_step_control_flow(tmp_path):
  n, steps = 8, 2
  line, recs = _run(tmp_path, "train", n, steps, batch=2)
  assert line["n_gpus"] == n
  # gloo: the library's RCCL path is off (rccl_ranks 0) and the step all-reduces through
  # torch.distributed once per step -- warm-up, timed steps, the sizing probe is skipped
  # (--steps given), one profiled step
  assert line["rccl_ranks"] == 0 and "allreduce" not in line
  assert "data-parallel x8, gradient all-reduce" in line["config"]["parallelism"]
  for r in recs:
    assert r["allreduce_calls"] == 1 + steps + 1
  assert line["ms_per_step"] >= 0.9 * 2.0 * n


@pytest.mark.timeout(900)
def test_stalled_rccl_bootstrap_in_a_sub_workload_keeps_the_headline_line(tmp_path):
  """The --full run measures the headline first and the sub-workloads after it.  If the
  in-library RCCL bootstrap of the training sub-workload never returns (here: a stand-in that
  sleeps), its deadline ends the ranks -- and rank 0 still emits ONE line carrying the measured
  headline and the reason, instead of the job dying without output or hanging."""
  env = dict(os.environ, MV_BENCH_BACKEND="gloo", MV_HARNESS_DIR=str(tmp_path),
             OMP_NUM_THREADS="1", MASTER_ADDR="127.0.0.1", MV_HARNESS_STUCK_COMM="1")
  for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
    env.pop(k, None)
  r = subprocess.run([sys.executable, HARNESS, "--gpus", "2", "--steps", "2", "--warmup", "1",
                      "--full", "--no-cpu-baseline", "--no-fp32-ref", "--only-sub", "train_n32"],
                     env=env, capture_output=True, timeout=600)
  assert r.returncode != 0                       # the job failed, loudly ...
  assert b"FATAL: mv_allreduce_init" in r.stderr
  lines = [l for l in r.stdout.decode().splitlines() if l.strip().startswith("{")]
  assert len(lines) == 1, r.stdout.decode()[-2000:]   # ... with the headline on the record
  line = json.loads(lines[0])
  assert line["n_gpus"] == 2 and line["value"] > 0 and "did not return" in line["aborted"]
  assert "train_n32" not in line


@pytest.mark.timeout(900)
def test_plain_run_is_the_headline_alone_and_dumps_its_outputs(tmp_path):
  """A plain run (no --full) carries the headline's contract fields and nothing that takes
  runs of its own; --steps sets the timed steps; --dump-outputs writes the arrays of the
  last timed step as float32 .npy, the same ones for the same arguments.  --full brings the
  roofline back."""
  import numpy as np
  env = dict(os.environ, MV_BENCH_BACKEND="gloo", MV_HARNESS_DIR=str(tmp_path),
             OMP_NUM_THREADS="1", MASTER_ADDR="127.0.0.1")
  for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
    env.pop(k, None)

  def run(*extra):
    r = subprocess.run([sys.executable, HARNESS, "--gpus", "1", "--steps", "4", "--warmup", "1",
                        "--batch", "2"] + list(extra), env=env, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])

  dumps = []
  for k in range(2):
    d = os.path.join(str(tmp_path), "dump%d" % k)
    line = run("--dump-outputs", d)
    assert line["steps"] == 4 and line["warmup"] == 1
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
      assert key in line, key
    assert abs(line["value"] - 2 * 4 / (line["ms_per_step"] * 4e-3)) <= 0.02 * line["value"]
    assert not set(line) & {"roofline", "cpu_baseline", "fp32_mfma_reference", "host_path",
                            "train_n32", "beam_n128_b20", "greedy_b256", "bf16"}
    names = sorted(os.listdir(d))
    assert names == ["grid_pred_class_s0.npy", "grid_pred_class_s1.npy",
                     "grid_pred_reg_s0.npy", "grid_pred_reg_s1.npy"]
    dumps.append({n: np.load(os.path.join(d, n)) for n in names})
  for n, a in dumps[0].items():
    assert a.dtype == np.float32 and (a == dumps[1][n]).all(), n
  # the stand-in's arrays carry its step count: warm-up 1 + timed 4 = the last timed step
  assert (dumps[0]["grid_pred_class_s0.npy"] == 5).all()
  assert "roofline" in run("--full", "--no-sub", "--no-cpu-baseline", "--no-fp32-ref")
