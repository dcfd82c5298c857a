# coding=utf-8
"""The class encoder on the light cone of the observed cells: h-steps between the
first and the last run only the wave tiles the cone touches, every other cell takes the state of
ONE input-free background row.  A background cell's value comes from the same instruction
sequence on the same operand values whichever row holds it, and the MFMA columns are
independent, so the bar is bitwise: every output with the cone equals the output with
MV_ENC_CONE=0.  The shapes here are the smallest that can go wrong, below the batch size from which
the default cones (the background row would cost more than it saves), so the coned run sets
MV_ENC_CONE=2: the cone at any batch size.  The switch is read once per process: each value runs tests/enc_cone_cases.py in
a process of its own, once."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import enc_cone_cases as cases
import enc_cone_twin as twin

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def runs(built_lib, tmp_path_factory):
  d = tmp_path_factory.mktemp("enc_cone")
  out = {}
  # (MV_ENC_CONE=2: the cone at any batch size; the default takes it from 16 rows on)
  for name, env in (("cone", {"MV_ENC_CONE": "2"}), ("dense", {"MV_ENC_CONE": "0"})):
    path = str(d / (name + ".npz"))
    base = {k: v for k, v in os.environ.items() if k != "MV_ENC_CONE"}
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tests", "enc_cone_cases.py"), path],
                          env=dict(base, **env), timeout=600)
    out[name] = dict(np.load(path))
  return out


CASES = list(cases.GREEDY) + ["beam_scale0", "beam_scale1"]


def test_both_runs_produced_the_same_arrays(runs):
  assert sorted(runs["cone"]) == sorted(runs["dense"])
  for case in CASES:
    assert any(k.startswith(case + "/") for k in runs["cone"]), case


@pytest.mark.parametrize("case", CASES)
def test_cone_is_bitwise_dense(runs, case):
  """batch 3 and batch 1 on both scales (at 9 x 16 a row is 48 triple-cells: wave tiles straddle
  two images and the background row), obs_len 8 and 2, hand-made label paths (corner held still,
  a path across a triple boundary, a jump across the grid, a path that makes every tile active)
  and the synthetic feed, ragged lengths with a row that does not decode, a model without scene
  encoder (r0 = 2), bf16 mode, the pipelined path with different feeds in flight; beam 3 under
  graph replay and the sampled forward, one scale at a time.

  Dense on both sides BY DESIGN (csrc/gate_plan.h enc_cone_geometry and its callers; these cases
  show that the switch leaves those paths alone, not that a cone is right there): everything at
  scale 1 (9 x 16: three row triples, width 16), beam_scale1, obs2 (no step between the first
  and the last), bf16 (the bf16 tile takes no lists) and the ragged forward (its encoders run on
  a prefix of the batch).  Coned: scale 0 of batch3, batch1, no_scene_enc and beam_scale0
  (test_accounting_* and test_beam_and_sampled_forwards_run_coned prove it from the executed
  FLOPs)."""
  keys = sorted(k for k in runs["cone"] if k.startswith(case + "/"))
  assert keys
  for k in keys:
    a, b = runs["cone"][k], runs["dense"][k]
    assert a.dtype == b.dtype and a.shape == b.shape, k
    if a.dtype.kind == "f":
      assert not np.isnan(a).any(), k
    assert a.tobytes() == b.tobytes(), k


def test_feeds_differ_and_pipelined_is_resident(runs):
  """(a stale list would not go unseen: the feeds are different problems, and the pipelined
  forward of feed k is the resident forward of feed k)"""
  for r in ("cone", "dense"):
    a = runs[r]["batch3/resident0/cls0"]
    assert a.tobytes() != runs[r]["batch3/resident1/cls0"].tobytes()
    for k in runs[r]:
      if "/resident" in k:
        assert runs[r][k].tobytes() == runs[r][k.replace("/resident", "/pipelined")].tobytes(), k


@pytest.mark.parametrize("case", cases.STATS_CASES)
def test_accounting_counts_executed_tiles(runs, case):
  """kernel_stats()["convlstm_step"]["flops"] of a profiled step is the twin's executed count;
  with the switch off it is the dense encoder's; flops_dense, the launches and the F(3,3) factor
  do not move."""
  from multiverse_amd import synth
  kw, _ = cases.GREEDY[case]
  cfg = synth.default_config(**kw)
  for k in range(2):
    st = {r: json.loads(runs[r]["stats/%s/%d" % (case, k)].tobytes().decode())
          for r in ("cone", "dense")}
    feed = {"grid_obs_labels": [runs["cone"]["labels/%s/%d/%d" % (case, k, s)] for s in range(2)]}
    want = {r: twin.executed_gate_flops(cfg, feed, r == "cone") for r in ("cone", "dense")}
    for r in ("cone", "dense"):
      g = st[r]["convlstm_step"]
      print(case, k, r, "flops", g["flops"], "twin", want[r], "dense", g["flops_dense"])
    for r in ("cone", "dense"):
      g = st[r]["convlstm_step"]
      assert g["flops"] == want[r], (case, k, r)
      assert g["flops_mfma"] / g["flops"] == pytest.approx(5.0 / 3.0, rel=1e-12)
    assert st["cone"]["convlstm_step"]["flops_dense"] == st["dense"]["convlstm_step"]["flops_dense"]
    assert sorted(st["cone"]) == sorted(st["dense"])
    for name in st["cone"]:
      assert st["cone"][name]["launches"] == st["dense"][name]["launches"], name


@pytest.mark.parametrize("name", ["beam", "sampled"])
def test_beam_and_sampled_forwards_run_coned(runs, name):
  """A profiled beam-3 forward and a profiled sampled forward (graph mode off) at scale 0: the
  executed FLOPs of the gate launches differ from the dense run's by exactly the class encoder's
  h-steps on the twin's cells instead of the batch's; at scale 1 (dense by design) not at all."""
  C, N, T = 256, 3, 8
  for scale, (H, W) in enumerate([(18, 32), (9, 16)]):
    case = "beam_scale%d" % scale
    fl = {r: json.loads(runs[r]["stats/%s/%s" % (case, name)].tobytes().decode())
          ["convlstm_step"] for r in ("cone", "dense")}
    print(case, name, "flops cone", fl["cone"]["flops"], "dense", fl["dense"]["flops"])
    want = 0.0
    if scale == 0:
      _, cells, _ = twin.twin_lists(runs["cone"]["labels/" + case].reshape(N, T), H, W, 1)
      want = sum(2.0 * (float(cells[t]) - N * H * W) * 9 * C * 4 * C for t in range(1, T))
      assert want != 0.0
    assert fl["cone"]["flops"] - fl["dense"]["flops"] == want
    assert fl["cone"]["flops_dense"] == fl["dense"]["flops_dense"]
    assert fl["cone"]["launches"] == fl["dense"]["launches"]
