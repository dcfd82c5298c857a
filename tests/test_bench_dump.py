# coding=utf-8
"""CPU: bench.py --dump-outputs.  The budget split of bench.dump_outputs on the real output
shapes of batch sizes bench.py accepts (arrays written whole or as a fixed, seeded sample,
everything under the 64 MB limit), and the beam and training dumps of a whole run through
the stand-in engine of tests/bench_cpu_harness.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "bench_cpu_harness.py")
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

import bench  # noqa: E402

LIMIT = 64 * 10 ** 6


class _Stub(object):
  """Outputs of the real shapes (18x32 / 9x16 grids, 12 predicted steps) whose values
  increase along the flat index, so a sample in flat order is nondecreasing."""

  def __init__(self, batch, beam=20, n_params=0):
    self.N, self.B, self.n_params = batch, beam, n_params

  @staticmethod
  def _ramp(shape, dtype=np.float32):
    return np.arange(int(np.prod(shape)), dtype=dtype).reshape(shape)

  def download(self):
    N = self.N
    return ([self._ramp((N, 12, 18, 32, 1)), self._ramp((N, 12, 9, 16, 1))],
            [self._ramp((N, 12, 18, 32, 2)), self._ramp((N, 12, 9, 16, 2))])

  def download_beam(self):
    N, B = self.N, self.B
    return {"best_beam": self._ramp((N, 12, 18, 32, 1)),
            "grid_reg": self._ramp((N, 12, 18, 32, 2)),
            "logits": self._ramp((N, B, 12, 18 * 32)),
            "ids": self._ramp((N, B, 12), np.int32),
            "logprobs": self._ramp((N, B))}, 0

  def param_specs(self):
    return [("w", (self.n_params - 16,)), ("b", (16,))]

  def get_param(self, name):
    """the ramp goes on across parameters in param_specs order"""
    start = 0
    for n, shape in self.param_specs():
      if n == name:
        return self._ramp(shape) + np.float32(start)
      start += int(np.prod(shape))


def _whole(stub, kind):
  if kind == "greedy":
    cls, reg = stub.download()
    return {"grid_pred_class_s0": cls[0], "grid_pred_class_s1": cls[1],
            "grid_pred_reg_s0": reg[0], "grid_pred_reg_s1": reg[1]}
  if kind == "beam":
    return {"beam_" + k: v for k, v in stub.download_beam()[0].items()}
  return {"losses": np.array([1.0, 0.5, 0.25]),
          "params": np.concatenate([stub.get_param(n) for n, _ in stub.param_specs()])}


@pytest.mark.parametrize("kind,batch,world,n_params", [
    ("beam", 256, 1, 0),          # logits alone are 141 MB
    ("beam", 128, 2, 0),          # two ranks: half the budget each
    ("greedy", 768, 1, 0),        # every array but the smallest over its first share
    ("greedy", 64, 1, 0),         # the headline: 6.6 MB, written whole
    ("train", 2, 1, 21_300_000),  # the 21.3M-float weights
])
def test_dump_fits_the_budget_and_samples_in_order(tmp_path, kind, batch, world, n_params):
  stub = _Stub(batch, n_params=n_params)
  out = str(tmp_path / "dump")
  budget = bench.DUMP_BYTES // world
  for rank in range(world):
    bench.dump_outputs(out, stub, kind, (1.0, 0.5, [0.25]), rank, world)
  whole = _whole(stub, kind)
  prefix = lambda r: "rank%d_" % r if world > 1 else ""
  files = sorted(os.listdir(out))
  assert sum(os.path.getsize(os.path.join(out, f)) for f in files) <= LIMIT
  for rank in range(world):
    got = {f[len(prefix(rank)):-4]: np.load(os.path.join(out, f))
           for f in files if f.startswith(prefix(rank))}
    assert sum(a.nbytes for a in got.values()) <= budget
    assert sorted(k[:-len("_sample")] if k.endswith("_sample") else k for k in got) == \
        sorted(whole)
    for k, a in got.items():
      src = whole[k[:-len("_sample")]] if k.endswith("_sample") else whole[k]
      assert a.dtype == (np.float64 if src.dtype.kind in "iu" or src.dtype == np.float64
                         else np.float32), k
      if not k.endswith("_sample"):
        assert (a == src.astype(a.dtype)).all(), k
        continue
      assert src.nbytes * world > bench.DUMP_BYTES // len(whole), k   # only large arrays
      assert a.ndim == 1 and 0 < a.size < src.size, k
      assert (np.diff(a) >= 0).all(), k         # flat order kept
      assert a.nbytes > budget // (2 * len(whole)), k   # the sample uses its share
  if kind == "greedy" and batch == 64:
    assert not any(f.endswith("_sample.npy") for f in files)


def _harness(tmp_path, *args):
  env = dict(os.environ, MV_BENCH_BACKEND="gloo", MV_HARNESS_DIR=str(tmp_path),
             OMP_NUM_THREADS="1", MASTER_ADDR="127.0.0.1")
  for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
    env.pop(k, None)
  r = subprocess.run([sys.executable, HARNESS, "--gpus", "1", "--batch", "2"] + list(args),
                     env=env, capture_output=True, timeout=600)
  assert r.returncode == 0, r.stderr.decode()[-3000:]
  lines = [l for l in r.stdout.decode().splitlines() if l.strip()]
  assert len(lines) == 1, lines
  return json.loads(lines[0])


@pytest.mark.timeout(900)
@pytest.mark.parametrize("workload,names", [
    ("beam", ["beam_best_beam", "beam_grid_reg", "beam_ids", "beam_logits", "beam_logprobs"]),
    ("train", ["losses", "params"]),
])
def test_beam_and_training_runs_dump_their_last_step(tmp_path, workload, names):
  """Same arguments, same arrays; another number of steps, other arrays (the stand-in makes
  them from the uploaded inputs and its step count).  Training: the losses of the last timed
  step (the stand-in's first loss is half its step count: warm-up 1 + timed 3 = 4)."""
  def dump(tag, steps):
    d = str(tmp_path / tag)
    line = _harness(tmp_path, "--workload", workload, "--steps", str(steps), "--warmup", "1",
                    "--dump-outputs", d)
    assert line["steps"] == steps
    got = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}
    assert sorted(got) == names
    return got
  a, b, c = dump("a", 3), dump("b", 3), dump("c", 4)
  for n in names:
    assert a[n].dtype in (np.float32, np.float64), n
    assert (a[n] == b[n]).all(), n
    assert not np.array_equal(a[n], c[n]), n
  if workload == "beam":
    assert a["beam_ids"].dtype == np.float64 and (a["beam_ids"] == np.round(a["beam_ids"])).all()
    assert a["beam_logits"].shape == (2, 20, 12, 18 * 32)
  else:
    assert a["losses"].dtype == np.float64
    assert list(a["losses"]) == [2.0, 0.25, 0.125, 0.0625]
    assert a["params"].shape == (3 * 3 * 8 * 16 + 16,)
