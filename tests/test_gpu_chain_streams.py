# coding=utf-8
"""The greedy inference forward issues its class chains and its regression chains as two chain
pairs on two streams (csrc/engine_forward.h enqueue_forward).  A chain's kernels, operands and
tile maps are those of the single-stream forward, and a tile's result does not depend on the
launch that carries it, so the bar is bitwise: every output with MV_CHAIN_STREAMS=2 (the
default) equals the output with MV_CHAIN_STREAMS=1.  The switch is read once per process: each
value runs tests/chain_streams_cases.py in a process of its own, once."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import chain_streams_cases as cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def runs(built_lib, tmp_path_factory):
  d = tmp_path_factory.mktemp("chain_streams")
  out = {}
  for n in ("1", "2"):
    path = str(d / ("streams%s.npz" % n))
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tests", "chain_streams_cases.py"),
                           path], env=dict(os.environ, MV_CHAIN_STREAMS=n), timeout=1500)
    out[n] = dict(np.load(path))
  return out


def _keys(runs, case):
  keys = sorted(k for k in runs["1"] if k.startswith(case + "/"))
  assert keys, case
  return keys


def test_both_runs_produced_the_same_arrays(runs):
  assert sorted(runs["1"]) == sorted(runs["2"])
  for case, (kw, _) in cases.CASES.items():
    n_feeds = cases.N_FEEDS if case == "headline" else 3
    scales = sum(1 for g in kw["use_grids"] if g)
    extra = 1 if case == "headline" else 0
    assert len(_keys(runs, case)) == (2 * n_feeds + extra) * scales * 2, case


@pytest.mark.parametrize("case", list(cases.CASES))
def test_two_streams_are_bitwise_one_stream(runs, case):
  """Benchmark configuration (both scales, batch 64, f16x3), f32, bf16, one scale only,
  use_single_decoder, use_gnn off, no scene encoder, the literal 36x18 / 18x9 grids (halo
  tiling), a relu model (per-tensor x exponents: the per-slot exponent scratch): resident
  forwards queued back to back on changing feeds (20 feeds on the headline) and the same
  feeds through forward_greedy_pipelined, byte for byte."""
  for k in _keys(runs, case):
    a, b = runs["1"][k], runs["2"][k]
    assert a.dtype == b.dtype and a.shape == b.shape, k
    assert np.isfinite(a).all(), k
    assert a.tobytes() == b.tobytes(), k


@pytest.mark.parametrize("case", list(cases.CASES))
def test_pipelined_equals_resident(runs, case):
  """Within one process: the pipelined forward of feed k is the resident forward of feed k,
  bit for bit, with either value of the switch."""
  for n in ("1", "2"):
    for k in _keys(runs, case):
      if "/resident" in k:
        assert runs[n][k].tobytes() == runs[n][k.replace("/resident", "/pipelined")].tobytes(), k


def test_feeds_differ(runs):
  """(the 20 feeds are 20 different problems: a stale buffer would not go unseen)"""
  a = runs["2"]["headline/resident0/cls0"]
  for k in range(1, cases.N_FEEDS):
    assert a.tobytes() != runs["2"]["headline/resident%d/cls0" % k].tobytes()


def test_profiled_step_names_counts_and_gate_form(runs):
  """kernel_stats() of a profiled headline step: the same kernel names, launches, FLOPs and
  bytes per name with either value (a profiled step is issued on one stream: event brackets
  around overlapped launches time nothing), and the gate launches in the F(3,3) form: 5 fp16
  MFMA products issued per 3 executed.  The un-profiled two-stream forwards of the headline
  equal these single-stream ones bit for bit (above), which a launch in another form -- other
  products, other roundoff -- would not."""
  s1 = json.loads(runs["1"]["stats"].tobytes().decode())
  s2 = json.loads(runs["2"]["stats"].tobytes().decode())
  assert sorted(s1) == sorted(s2)
  for name in s1:
    assert s1[name] == s2[name], name
  for s in (s1, s2):
    g = s["convlstm_step"]
    assert g["launches"] == 20
    assert g["flops_mfma"] / g["flops"] == pytest.approx(5.0 / 3.0, rel=1e-12)
    assert s["wino3_transform"]["launches"] == 19
