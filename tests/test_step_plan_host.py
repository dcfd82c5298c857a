# coding=utf-8
"""The rule functions of csrc/step_plan.h, compiled alone on the host (no GPU, no HIP): the file
answers questions and launches nothing, so a small program that supplies the four names it takes
from the rest of the translation unit can include it and print its answers.  The expected answers
are written out here, not obtained from the header."""

import itertools
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multiverse_amd", "csrc")

_PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <cstddef>
#include "multiverse_hip.h"
// what step_plan.h takes from the headers in front of it in engine.hip
namespace mv { constexpr int kBeamRankJ = %(rank_j)d; }   // kernels_misc.h (read from there)
#define MV_REQUIRE(cond, ...) do { if (!(cond)) { printf(__VA_ARGS__); printf("\n"); } } while (0)
namespace {
inline int env_num(const char* name, int unset) { const char* v = getenv(name); return v ? atoi(v) : unset; }
inline bool env_on(const char* name) { return env_num(name, 1) != 0; }
}
#include "step_plan.h"

int main() {
  const int Ws[] = {16, 32, 33}, Cs[] = {128, 256, 512}, Ds[] = {0, 32, 64, 128};
  const size_t bytes[] = {((size_t)1 << 32) - 4, (size_t)1 << 32};
  for (int ver = 0; ver <= 3; ++ver)
    for (int W : Ws) for (int C : Cs) for (int D : Ds) for (int b = 0; b < 2; ++b)
      printf("gnn %%d %%d %%d %%d %%d %%d\n", ver, W, C, D, b, (int)gnn_form(ver, W, C, D, bytes[b]));
  printf("weaker %%d\n", (int)weaker(GnnForm::Blocked, GnnForm::Tiled));
  const int Ks[] = {1024, 1025};
  for (int K : Ks) {
    printf("tail_fits %%d %%d\n", K, (int)tail_grouped_fits(64, K));
    printf("tail_form %%d %%d %%d\n", K, (int)tail_form(false, 64, K), (int)tail_form(true, 64, K));
    printf("row_fits %%d %%d\n", K, (int)row_fits_wave(K));
    for (int masked = 0; masked < 2; ++masked)
      for (int cand = 0; cand < 2; ++cand)
        printf("beam %%d %%d %%d %%d\n", K, cand, masked, (int)beam_step_form(K, cand != 0, masked != 0));
  }
  printf("lds %%zu\n", beam_step_lds_bytes(2, 1100));
  require_row_fits_wave("mv_op_x", 1100);
  mv_config c{};
  c.use_gnn = 1; c.beam_size = 1; c.batch_size = 64; c.emb_size = 64;
  printf("dedupe %%d %%d %%d\n", (int)beam_gnn_dedupe(c, 1024, true), (int)beam_gnn_dedupe(c, 1025, true),
         (int)beam_gnn_dedupe(c, 1024, false));
  printf("pairs %%d", (int)chain_pairs_planned(c, true, true, false, false, true));
  c.batch_size = 65;
  printf(" %%d", (int)chain_pairs_planned(c, true, true, false, false, true));
  c.batch_size = 64;
  printf(" %%d %%d\n", (int)chain_pairs_planned(c, true, true, false, true, true),
         (int)chain_pairs_planned(c, true, true, false, false, false));
  for (int f = 0; f < 16; ++f)
    printf("row_form %%d %%d %%d %%d %%d\n", f & 1, (f >> 1) & 1, (f >> 2) & 1, (f >> 3) & 1,
           (int)row_form((f & 1) != 0, (f & 2) != 0, (f & 4) != 0, (f & 8) != 0));
  for (int m = 0; m < 3; ++m) for (int b = 0; b < 3; ++b)
    for (int radius = 0; radius <= MV_MOTION_MAX_RADIUS; ++radius) for (int acc = 0; acc < 2; ++acc)
      for (int rv = 0; rv < 3; ++rv)
        printf("key %%d %%d %%d %%d %%d %%d\n", m, b, radius, acc, rv,
               constraint_graph_key(m, b, radius, acc != 0, rv != 0, rv == 2));
  printf("max_radius %%d\n", MV_MOTION_MAX_RADIUS);
  return 0;
}
"""

PER_CELL, TILED, BLOCKED = 0, 1, 2        # GnnForm, in its declared (weaker-first) order
SINGLE, RANK_SELECT = 0, 1                # BeamStepForm
GROUPED, SEPARATE = 0, 1                  # TailForm
PLAIN, MASKED, BIASED, MOTION, PATH = range(5)   # RowForm (row_form.h), in its declared order

_SWITCHES = ("MV_GNN", "MV_TAIL", "MV_TRAIN_TAIL", "MV_BEAM_STEP", "MV_BEAM_SHARED_FIRST",
             "MV_BEAM_GNN_DEDUPE", "MV_SPARSE_X", "MV_CHAIN_STREAMS", "MV_CHAIN_PRIORITY")


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
  cxx = shutil.which("g++") or shutil.which("c++")
  if cxx is None:
    pytest.skip("no host C++ compiler")
  with open(os.path.join(CSRC, "kernels_misc.h")) as f:
    rank_j = int(re.search(r"constexpr int kBeamRankJ = (\d+);", f.read()).group(1))
  d = tmp_path_factory.mktemp("step_plan")
  src = d / "step_plan_host.cpp"
  src.write_text(_PROGRAM % dict(rank_j=rank_j))
  exe = str(d / "step_plan_host")
  subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function",
                         "-I", os.path.join(ROOT, "include"), "-I", CSRC, str(src), "-o", exe])
  return exe


def _run(exe, **switches):
  env = {k: v for k, v in os.environ.items() if k not in _SWITCHES}
  env.update(switches)
  out = subprocess.check_output([exe], env=env, timeout=60).decode().splitlines()
  return [l.split() for l in out]


def _expected_gnn(ver, W, C, D, below):
  """The table, written out: the tiled kernels want W <= 32, C == 256 and at most one 64-channel
  scene chunk; the blocked one no chunk or a whole one, and h below 2^32 bytes."""
  if ver == 1 or W == 33 or C != 256 or D == 128:
    return PER_CELL
  if ver == 2:
    return TILED
  return BLOCKED if (D in (0, 64) and below) else TILED


def test_gnn_form_table(plan_exe):
  for knob, knob_ver in ((None, 3), ("v1", 1), ("v2", 2)):
    rows = [r for r in _run(plan_exe, **({"MV_GNN": knob} if knob else {})) if r[0] == "gnn"]
    assert len(rows) == 4 * 3 * 3 * 4 * 2
    for _, ver, W, C, D, b, got in rows:
      ver, W, C, D, b, got = int(ver), int(W), int(C), int(D), int(b), int(got)
      want = _expected_gnn(ver or knob_ver, W, C, D, below=(b == 0))
      assert got == want, (knob, ver, W, C, D, b, got, want)
  assert ["weaker", str(TILED)] in _run(plan_exe)


def test_row_tail_and_beam_step_bounds(plan_exe):
  got = {tuple(r[:-1]) if r[0] != "tail_form" else tuple(r[:2]): r for r in _run(plan_exe)}
  assert got[("tail_fits", "1024")][-1] == "1" and got[("tail_fits", "1025")][-1] == "0"
  assert got[("row_fits", "1024")][-1] == "1" and got[("row_fits", "1025")][-1] == "0"
  # inference keeps the grouped tail (and fails in it) above 1024 cells; training falls back
  assert got[("tail_form", "1024")][2:] == [str(GROUPED), str(GROUPED)]
  assert got[("tail_form", "1025")][2:] == [str(GROUPED), str(SEPARATE)]
  for K, cand, masked in itertools.product((1024, 1025), (0, 1), (0, 1)):
    want = RANK_SELECT if masked or (K == 1024 and cand) else SINGLE
    assert int(got[("beam", str(K), str(cand), str(masked))][-1]) == want, (K, cand, masked)
  assert got[("lds",)][-1] == str((2 * 2 * 1100 + 512) * 4)
  # the one message of the row bound: the caller's name, "K = <n>" and "<n> cells"
  msg = [" ".join(r) for r in _run(plan_exe) if r[0] == "mv_op_x:"]
  assert msg == ["mv_op_x: K = 1100 cells (one wave holds a row of at most 1024)"]
  assert got[("dedupe", "1", "0")][-1] == "0"        # K = 1024 yes, K = 1025 no, tiled first step no
  assert got[("pairs", "1", "0", "0")][-1] == "0"    # batch 64 yes; 65, capturing, separate tail no


def test_switches_select_the_fallback_forms(plan_exe):
  got = {tuple(r[:2]): r for r in _run(plan_exe, MV_TAIL="v1") if r[0] == "tail_form"}
  assert got[("tail_form", "1024")][2:] == [str(SEPARATE), str(SEPARATE)]
  got = {tuple(r[:2]): r for r in _run(plan_exe, MV_TRAIN_TAIL="v1") if r[0] == "tail_form"}
  assert got[("tail_form", "1024")][2:] == [str(GROUPED), str(SEPARATE)]
  rows = _run(plan_exe, MV_BEAM_STEP="v1")
  beam = {tuple(r[1:4]): int(r[4]) for r in rows if r[0] == "beam"}
  assert beam[("1024", "1", "0")] == SINGLE and beam[("1024", "1", "1")] == RANK_SELECT
  assert [r for r in rows if r[0] == "dedupe"] == [["dedupe", "0", "0", "0"]]
  for switch in ({"MV_GNN": "v1"}, {"MV_BEAM_GNN_DEDUPE": "0"}):
    assert [r for r in _run(plan_exe, **switch) if r[0] == "dedupe"] == [["dedupe", "0", "0", "0"]]


def test_row_form_table(plan_exe):
  """One rule for the form of a constrained step: the last of mask / bias / motion / revisit that
  is set names it, whatever is set below it."""
  rows = [[int(x) for x in r[1:]] for r in _run(plan_exe) if r[0] == "row_form"]
  assert len(rows) == 16
  for masked, biased, motion, revisit, got in rows:
    want = (PATH if revisit else MOTION if motion else BIASED if biased else MASKED if masked
            else PLAIN)
    assert got == want, (masked, biased, motion, revisit, got, want)


def test_graph_key_members_are_distinct(plan_exe):
  """The constraint member of the graph key: mask layout 0 - 2, bias layout 0 - 2, the motion
  member (unset, or a radius from 1 to MV_MOTION_MAX_RADIUS with acc absent or present) and the
  revisit member 0 - 2 -- two different states never share a key."""
  out = _run(plan_exe)
  max_radius = int([r for r in out if r[0] == "max_radius"][0][1])
  assert max_radius == 4                  # motion member 0 - 8
  keys = {}
  for r in out:
    if r[0] != "key":
      continue
    m, b, radius, acc, rv, key = (int(x) for x in r[1:])
    motion = 0 if radius == 0 else 2 * radius - 1 + acc     # acc means nothing without a radius
    keys.setdefault((m, b, motion, rv), set()).add(key)
  assert len(keys) == 3 * 3 * (2 * max_radius + 1) * 3 == 243
  assert all(len(v) == 1 for v in keys.values()), "a member combination with two keys"
  assert len({next(iter(v)) for v in keys.values()}) == 243
