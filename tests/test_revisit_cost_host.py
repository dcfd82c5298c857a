# coding=utf-8
"""CPU: the revisit cost (mv_set_revisit_cost) around the engine -- the new symbols and their
prototypes, `multifuture.path_revisit_cost` against plain loops, the "revisit_cost" key of
`inference_feed`, the script's flags and their refusals -- and the restatement
(tests/revisit_cost_oracle.py) against the ones it stands on: with zero cost it is
motion_cost_oracle bit for bit (cell_bias_oracle without a motion cost), and at a first step with
seed_observed, where every row of a sample has the same set, it is cell_bias_oracle under the
plane b[n, k] = rterm built from the labels, bit for bit."""
import ctypes
import inspect
import os
import re
from glob import glob

import numpy as np
import pytest

from multiverse_amd import cli, multifuture as mf

import cell_bias_oracle as cb
import motion_cost_oracle as mo
import revisit_cost_oracle as ro
import mf_fixture
from test_cell_mask_host import _mf_args
from test_motion_cost_host import _inputs, _tables, R, S, K, W, N, B, LIMITS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = (("mv_op_beam_step", 5), ("mv_op_sbs_step", 7), ("mv_op_sample_step", 4))


# ------------------------------------------------------------ symbols

def test_library_exports_the_new_symbols(built_lib):
  text = open(os.path.join(ROOT, "include", "multiverse_hip.h")).read()
  text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
  protos = dict(re.findall(r"\bint\s+(mv_\w+)\s*\(([^;{]*?)\)\s*;", text))
  raw = ctypes.CDLL(built_lib.LIB_PATH)
  lib = built_lib.load()
  for name in ("mv_set_revisit_cost", "mv_op_beam_step_path", "mv_op_sbs_step_path",
               "mv_op_sample_step_path"):
    assert hasattr(raw, name), "libmultiverse_hip.so does not export " + name
    assert name in built_lib.EXPORTED_SYMBOLS and name in protos
  norm = lambda name: [" ".join(p.split()) for p in protos[name].split(",")]
  assert norm("mv_set_revisit_cost") == ["mv_handle h", "const float* cost",
                                         "int32_t seed_observed"]
  fp = ctypes.POINTER(ctypes.c_float)
  assert lib.mv_set_revisit_cost.argtypes[1:] == [fp, ctypes.c_int32]
  # each _path op is its _motion op plus one pointer, directly behind `motion`
  rp = ctypes.POINTER(built_lib.mv_step_revisit)
  for name, at in OPS:
    want = norm(name + "_motion")
    assert want[at] == "const mv_step_motion* motion"
    want.insert(at + 1, "const mv_step_revisit* revisit")
    assert norm(name + "_path") == want, name
    motion, path = getattr(lib, name + "_motion").argtypes, getattr(lib, name + "_path").argtypes
    assert list(path) == list(motion[:at + 1]) + [rp] + list(motion[at + 1:]), name
  # the one new struct, as the header declares it
  m = re.search(r"typedef struct mv_step_revisit \{(.*?)\} mv_step_revisit;", text, flags=re.S)
  members = [" ".join(d.split()) for d in m.group(1).split(";") if d.strip()]
  assert members == ["const float* cost", "const int32_t* prev1", "const uint8_t* visited",
                     "uint8_t* visited_out"]
  assert [f[0] for f in built_lib.mv_step_revisit._fields_] == \
      ["cost", "prev1", "visited", "visited_out"]
  assert ctypes.sizeof(built_lib.mv_step_revisit) == 4 * 8
  assert ctypes.sizeof(built_lib.mv_step_motion) == 8 + 6 * 8     # the motion struct keeps its own
  assert lib.mv_abi_version() == 5 == built_lib.MV_ABI_VERSION    # new symbols only
  assert lib.mv_set_revisit_cost(None, None, 0) != 0              # NULL handle: an error
  assert ctypes.sizeof(built_lib.mv_config) == 28 * 4             # the structs keep their layout
  assert list(inspect.signature(built_lib.Engine.set_revisit_cost).parameters)[1:] == \
      ["cost", "seed_observed"]
  assert inspect.signature(built_lib.Engine.set_revisit_cost).parameters["seed_observed"].default \
      is True
  for op in (built_lib.op_beam_step, built_lib.op_sbs_step, built_lib.op_sample_step):
    assert inspect.signature(op).parameters["revisit"].default is None


# ------------------------------------------------------------ path_revisit_cost

def _loops(ids, labels, cost, obs, seed_observed):
  """The definition with lists, no sets: a cell pays when it equals an earlier cell of the path
  (or an observed one) and is not the cell the path is in."""
  Nn, Bb, T = ids.shape
  To = labels.shape[1]
  out = np.zeros((Nn, Bb, T), dtype=np.float32)
  for n in range(Nn):
    lo = To if obs is None else obs[n]
    for b in range(Bb):
      held = [int(c) for c in labels[n, To - lo:]] if seed_observed else []
      cur = int(labels[n, To - 1])
      for t in range(T):
        k = int(ids[n, b, t])
        if k < 0:
          break
        hit = False
        for h in held:
          hit = hit or h == k
        if hit and k != cur:
          out[n, b, t] = np.float32(cost[n])
        held.append(k)
        cur = k
  return out


def test_path_revisit_cost_is_the_definition_along_each_path():
  A, Bc, C = 11, 12, 13
  labels = np.array([[C, C, Bc]])
  cost = np.array([-2.5], dtype=np.float32)
  path = lambda *cells: np.array([[list(cells)]])
  # staying is free, whether the cell was observed or entered
  assert (mf.path_revisit_cost(path(Bc, Bc, A, A), labels, cost) == 0).all()
  # A, A, B, A pays once, at its last step (seed off: B is no observed cell)
  got = mf.path_revisit_cost(path(A, A, Bc, A), labels, cost, seed_observed=False)
  assert got.tolist() == [[[0, 0, 0, -2.5]]]
  # with the observed cells: B was observed, and is left at step 0
  got = mf.path_revisit_cost(path(A, A, Bc, A), labels, cost)
  assert got.tolist() == [[[0, 0, -2.5, -2.5]]]
  # an observed cell left before the last frame pays at once; seed off: it does not
  assert mf.path_revisit_cost(path(C, A), labels, cost).tolist() == [[[-2.5, 0]]]
  assert (mf.path_revisit_cost(path(C, A), labels, cost, seed_observed=False) == 0).all()
  # a one-frame row: the columns in front of the track are not read
  assert (mf.path_revisit_cost(path(C, A), labels, cost, obs_lengths=[1]) == 0).all()
  assert mf.path_revisit_cost(path(A, Bc), labels, cost, obs_lengths=[1]).tolist() == \
      [[[0, -2.5]]]
  # the last observed cell is no revisit at step 0, but is one after the path has left it
  assert mf.path_revisit_cost(path(A, Bc), labels, cost, seed_observed=False).tolist() == \
      [[[0, 0]]]
  # -1 ends a row; a scalar cost serves every row
  got = mf.path_revisit_cost(path(A, C, -1, -1), labels, -1.0)
  assert got.tolist() == [[[0, -1, 0, 0]]] and got.dtype == np.float32
  rng = np.random.RandomState(12)
  Nn, Bb, T, To = 3, 4, 6, 3
  labels = rng.randint(0, 9, size=(Nn, To))
  ids = rng.randint(0, 9, size=(Nn, Bb, T))                # nine cells: many returns
  ids[2, :, 4:] = -1
  cost = rng.randn(Nn).astype(np.float32)
  for obs in (None, [3, 1, 2]):
    for seed_observed in (True, False):
      got = mf.path_revisit_cost(ids, labels, cost, obs_lengths=obs, seed_observed=seed_observed)
      want = _loops(ids, labels, cost, obs, seed_observed)
      assert got.shape == (Nn, Bb, T) and got.tobytes() == want.tobytes(), (obs, seed_observed)
      assert (got != 0).sum() > Nn                         # (returns do happen)
  # along rows that continue themselves the restatement's walk pays what path_revisit_cost reports
  for seed_observed in (True, False):
    walk = ro.Path(labels, Bb, 9, [3, 1, 2], seed_observed)
    paid = np.zeros((Nn, Bb, 4), dtype=np.float32)
    for t in range(4):
      planes = ro.row_planes(walk.p1, walk.p0, walk.visited, 3, 9, cost)
      paid[:, :, t] = np.take_along_axis(planes, ids[:, :, t, None], axis=-1)[..., 0]
      walk.advance(ids[:, :, t])
    assert paid.tobytes() == mf.path_revisit_cost(ids[:, :, :4], labels, cost, [3, 1, 2],
                                                  seed_observed).tobytes()


def test_a_slot_continues_its_parents_set():
  labels = np.array([[3, 14], [50, 61]])
  path = ro.Path(labels, 3, K)
  assert sorted(np.flatnonzero(path.visited[0, 1])) == [3, 14]
  path.advance(np.array([[15, 24, 4], [62, 51, 60]]), np.array([[0, 0, 0], [0, 0, 0]]))
  path.advance(np.array([[25, 16, 26], [52, 63, 41]]), np.array([[1, 0, 1], [1, 0, 2]]))
  assert sorted(np.flatnonzero(path.visited[0, 0])) == [3, 14, 24, 25]    # the PARENT's set
  assert sorted(np.flatnonzero(path.visited[0, 1])) == [3, 14, 15, 16]
  assert sorted(np.flatnonzero(path.visited[1, 2])) == [41, 50, 60, 61]
  assert path.p0.tolist() == [[24, 15, 24], [51, 62, 60]]
  off = ro.Path(labels, 3, K, seed_observed=False)
  assert not off.visited.any()
  short = ro.Path(labels, 3, K, obs_lengths=[2, 1])
  assert sorted(np.flatnonzero(short.visited[1, 0])) == [61]


# ------------------------------------------------------------ inference_feed

def test_inference_feed_carries_the_revisit_cost(tmp_path):
  ds = mf_fixture.make_dataset(str(tmp_path / "fp"), n_traj=4)
  files = sorted(glob(os.path.join(ds["traj_path"], "*.txt")))
  ids = [os.path.splitext(os.path.basename(f))[0] for f in files]
  gt = mf.load_gt(ds["multifuture_path"], ids)
  plain_args = _mf_args(ds)
  inputs = mf.get_inputs(plain_args, files, gt)
  idxs = [0, 2]
  T_pred = max(inputs["max_pred_lengths"][i] for i in idxs)
  plain, _ = mf.inference_feed(inputs, plain_args, idxs, batch_size=3, pred_length=T_pred)
  assert "revisit_cost" not in plain
  args = _mf_args(ds, revisit_cost={"cost": -1.5, "seed_observed": False})
  feed, n_real = mf.inference_feed(inputs, args, idxs, batch_size=3, pred_length=T_pred)
  rc = feed["revisit_cost"]
  assert n_real == 2 and rc["seed_observed"] is False
  assert rc["cost"].dtype == np.float32 and rc["cost"].tolist() == [-1.5, -1.5, 0.0]   # padding
  for k in plain:                                                           # all else unchanged
    a, b = plain[k], feed[k]
    if isinstance(a, list):
      assert all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b)), k
    else:
      assert np.array_equal(a, b), k
  both = _mf_args(ds, revisit_cost={"cost": float(mf.MOTION_LIMIT), "seed_observed": True},
                  motion_cost=mf.motion_tables(2, None, 0.3), class_costs=[(1, -2.0)],
                  allowed_classes=[1, 2, 3], allowed_min_share=0.25)
  feed2, _ = mf.inference_feed(inputs, both, idxs, batch_size=3, pred_length=T_pred)
  assert feed2["revisit_cost"]["cost"][0] == np.float32(-1e30)
  assert feed2["revisit_cost"]["seed_observed"] is True
  assert "cell_bias" in feed2 and "cell_mask" in feed2 and "motion_cost" in feed2


# ------------------------------------------------------------ flags

def test_script_flags_and_their_refusals():
  flags = {f: (t, d) for f, t, d in cli._MF_FLAGS}                # pylint: disable=protected-access
  assert flags["--revisit_cost"] == (float, None)
  assert flags["--no_revisit"][0] == "store_true"
  assert flags["--revisit_ignore_observed"][0] == "store_true"
  p = cli.multifuture_inference_parser()
  base = ["traj", "mfut", "model", "out.p"]
  off = p.parse_args(base)
  cli.parse_revisit_cost(off)
  assert off.revisit_cost is None
  a = p.parse_args(base + ["--revisit_cost", "1.5", "--max_step_cells", "1", "--class_costs",
                           "1:-2", "--allowed_classes", "1,4", "--sample"])
  cli.parse_allowed_classes(a)
  cli.parse_class_costs(a)
  cli.parse_motion_cost(a)
  cli.parse_revisit_cost(a)
  assert a.revisit_cost == {"cost": -1.5, "seed_observed": True}  # the cost set is -c
  assert a.motion_cost["radius"] == 2 and a.class_costs == [(1, -2.0)]
  a = p.parse_args(base + ["--no_revisit", "--revisit_ignore_observed"])
  cli.parse_revisit_cost(a)
  assert np.float32(a.revisit_cost["cost"]) == np.float32(-1e30)
  assert a.revisit_cost["seed_observed"] is False
  a = p.parse_args(base + ["--revisit_cost", "0"])
  cli.parse_revisit_cost(a)
  assert a.revisit_cost["cost"] == 0 and a.revisit_cost["seed_observed"] is True
  for extra, words in ((["--revisit_cost", "1", "--greedy"], ("--revisit_cost", "--greedy")),
                       (["--no_revisit", "--greedy"], ("--no_revisit", "--greedy")),
                       (["--revisit_cost", "1", "--score_gt", "s.p"],
                        ("--revisit_cost", "--score_gt")),
                       (["--no_revisit", "--score_gt", "s.p"], ("--no_revisit", "--score_gt")),
                       (["--revisit_cost", "1", "--no_revisit"],
                        ("--revisit_cost", "--no_revisit", "contradict")),
                       (["--revisit_ignore_observed"],
                        ("--revisit_ignore_observed", "--revisit_cost")),
                       (["--revisit_cost=-1"], ("--revisit_cost", "finite")),
                       (["--revisit_cost", "inf"], ("--revisit_cost", "finite")),
                       (["--revisit_cost", "nan"], ("--revisit_cost", "finite"))):
    with pytest.raises(SystemExit) as err:
      cli.multifuture_inference_main(base + extra)
    assert all(w in str(err.value) for w in words), (extra, str(err.value))


# ------------------------------------------------------------ the restatement

def _visited(rng, rows_shape, p1):
  v = rng.rand(*(rows_shape + (K,))) < 0.3
  flat = v.reshape(-1, K)
  flat[np.arange(flat.shape[0]), np.asarray(p1).reshape(-1)] = True   # p1 itself: costs nothing
  return v


def test_zero_cost_is_the_motion_and_the_bias_restatement_bit_for_bit():
  rng, logits, l3, phi, LP, G = _inputs(15)
  for motion_on in (False, True):
    for bias_on in (False, True):
      for allowed in (None, rng.rand(R // S, K) < 0.5):
        bias = (2.0 * rng.randn(R // S, K)).astype(np.float32) if bias_on else \
            np.zeros((R // S, K), dtype=np.float32)
        tables = _tables(rng, R // S, 2) if motion_on else None
        p1, p0 = rng.randint(0, K, size=(R // S, S)), rng.randint(-1, K, size=(R // S, S))
        vis = _visited(rng, (R // S, S), p1)
        planes = ro.row_planes(p1, p0, vis, W, K, np.zeros(R // S, np.float32), tables,
                               bias if bias_on else None)
        base = mo.row_planes(p1, p0, W, K, tables, bias if bias_on else None) if motion_on \
            else np.repeat(bias[:, None], S, axis=1)
        assert planes.tobytes() == (base + np.float32(0)).tobytes()
        for temp in (1.0, 0.7):
          for limits in LIMITS:
            a = ro.sample_step(logits, S, 1, allowed, planes, temp, 9, limits[0], limits[1],
                               dtype=np.float32)
            if motion_on:
              b = mo.sample_step(logits, S, 1, allowed, base, temp, 9, limits[0], limits[1],
                                 dtype=np.float32)
            else:
              b = cb.sample_step(logits, S, 1, allowed, bias, temp, 9, limits[0], limits[1],
                                 dtype=np.float32)
            for k in ("keep", "tight", "wide", "ids", "q", "lp_id", "compared"):
              assert a[k].tobytes() == b[k].tobytes(), (motion_on, bias_on, temp, limits, k)
      for am in (None, rng.rand(N, K) < 0.5):
        bias = (2.0 * rng.randn(N, K)).astype(np.float32) if bias_on else \
            np.zeros((N, K), dtype=np.float32)
        tables = _tables(rng, N, 4) if motion_on else None
        p1, p0 = rng.randint(0, K, size=(N, B)), rng.randint(-1, K, size=(N, B))
        vis = _visited(rng, (N, B), p1)
        planes = ro.row_planes(p1, p0, vis, W, K, np.zeros(N, np.float32), tables,
                               bias if bias_on else None)
        base = mo.row_planes(p1, p0, W, K, tables, bias if bias_on else None) if motion_on else None
        for t in (0, 1):
          a = ro.sbs_step(l3, phi, LP, G, t, am, planes, 0.8, 3)
          b = mo.sbs_step(l3, phi, LP, G, t, am, base, 0.8, 3) if motion_on else \
              cb.sbs_step(l3, phi, LP, G, t, am, bias, 0.8, 3)
          for k in ("new_phi", "new_lp", "new_g", "ids", "parents", "q"):
            assert a[k].tobytes() == b[k].tobytes(), (t, k)
        for time in (1, 2):
          for diverse in (False, True):
            a = ro.beam_step(l3, LP, am, planes, time, diverse, 0.01, 0)
            b = mo.beam_step(l3, LP, am, base, time, diverse, 0.01, 0) if motion_on else \
                cb.beam_step(l3, LP, am, bias, time, diverse, 0.01, 0)
            for k in ("new_lp", "ids", "parents", "cand"):
              assert a[k].tobytes() == b[k].tobytes(), (time, diverse, k)


def test_a_first_step_is_the_bias_of_the_plane_built_from_the_labels():
  """At step 0 every row of a sample holds the same set -- the row's observed cells -- so the
  rows' planes are one plane per sample, b[n, k] = b0 + cost[n] on the observed cells other than
  the last, and the restatement is cell_bias_oracle under it."""
  rng, logits, l3, phi, LP, G = _inputs(16)
  labels = rng.randint(0, K, size=(N, 4))
  labels[0, 1] = labels[0, 3]                              # the last cell, seen before: free
  cost = np.array([-3.0, 2.0], dtype=np.float32)
  for obs in (None, [4, 1], [2, 3]):
    path = ro.Path(labels, B, K, obs)
    b0 = (2.0 * rng.randn(N, K)).astype(np.float32)
    planes = ro.row_planes(path.p1, path.p0, path.visited, W, K, cost, None, b0)
    want = b0.copy()
    for n in range(N):
      lo = 4 if obs is None else obs[n]
      for c in labels[n, 4 - lo:]:
        if c != labels[n, -1]:
          want[n, c] = b0[n, c] + cost[n]
    assert (want != b0).any() and want[0, labels[0, 3]] == b0[0, labels[0, 3]]
    assert planes.tobytes() == np.repeat(want[:, None], B, axis=1).tobytes()
    am = rng.rand(N, K) < 0.5
    a = ro.sbs_step(l3, phi, LP, G, 0, am, planes, 0.8, 3)
    b = cb.sbs_step(l3, phi, LP, G, 0, am, want, 0.8, 3)
    for k in ("new_phi", "new_lp", "new_g", "ids", "parents", "q"):
      assert a[k].tobytes() == b[k].tobytes(), k
    for diverse in (False, True):
      a = ro.beam_step(l3, LP, am, planes, 1, diverse, 0.01, 0)
      b = cb.beam_step(l3, LP, am, want, 1, diverse, 0.01, 0)
      for k in ("new_lp", "ids", "parents", "cand"):
        assert a[k].tobytes() == b[k].tobytes(), (diverse, k)
    lg = logits[:N * B]
    a = ro.sample_step(lg, B, 0, am, planes.reshape(N * B, K), 0.7, 9, 8, 0.9, dtype=np.float32)
    b = cb.sample_step(lg, B, 0, am, want, 0.7, 9, 8, 0.9, dtype=np.float32)
    for k in ("keep", "ids", "q", "lp_id"):
      assert a[k].tobytes() == b[k].tobytes(), k
  # seed_observed off: nothing is paid at a first step
  off = ro.Path(labels, B, K, None, False)
  assert (ro.row_planes(off.p1, off.p0, off.visited, W, K, cost) == 0).all()
