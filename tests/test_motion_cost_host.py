# coding=utf-8
"""CPU: the motion costs (mv_set_motion_cost) around the engine -- the new symbols and their
prototypes, `multifuture.motion_tables` and `multifuture.path_motion_cost` against plain loops,
the "motion_cost" key of `inference_feed`, the script's flags and their refusals -- and the
restatement (tests/motion_cost_oracle.py) against the one it stands on: with zero tables it is
cell_bias_oracle bit for bit, and at a first step, where every row of a sample has the same path,
it is cell_bias_oracle under the plane b[n, k] = vterm + aterm built from the labels, bit for
bit."""
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
import mf_fixture
from test_cell_mask_host import _mf_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = (("mv_op_beam_step", 4), ("mv_op_sbs_step", 6), ("mv_op_sample_step", 3))


# ------------------------------------------------------------ symbols

def test_library_exports_the_new_symbols(built_lib):
  text = open(os.path.join(ROOT, "include", "multiverse_hip.h")).read()
  assert re.search(r"#define\s+MV_MOTION_MAX_RADIUS\s+4\b", text)
  text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
  protos = dict(re.findall(r"\bint\s+(mv_\w+)\s*\(([^;{]*?)\)\s*;", text))
  raw = ctypes.CDLL(built_lib.LIB_PATH)
  lib = built_lib.load()
  for name in ("mv_set_motion_cost", "mv_op_beam_step_motion", "mv_op_sbs_step_motion",
               "mv_op_sample_step_motion"):
    assert hasattr(raw, name), "libmultiverse_hip.so does not export " + name
    assert name in built_lib.EXPORTED_SYMBOLS and name in protos
  norm = lambda name: [" ".join(p.split()) for p in protos[name].split(",")]
  assert norm("mv_set_motion_cost") == ["mv_handle h", "int32_t radius", "const float* vel",
                                        "const float* vel_far", "const float* acc",
                                        "const float* acc_far"]
  fp = ctypes.POINTER(ctypes.c_float)
  assert lib.mv_set_motion_cost.argtypes[1:] == [ctypes.c_int32, fp, fp, fp, fp]
  # each _motion op is its _biased op plus one pointer, directly behind `bias`
  mp = ctypes.POINTER(built_lib.mv_step_motion)
  for name, at in OPS:
    want = norm(name + "_biased")
    assert want[at] == "const float* bias"
    want.insert(at + 1, "const mv_step_motion* motion")
    assert norm(name + "_motion") == want, name
    biased, motion = getattr(lib, name + "_biased").argtypes, getattr(lib, name + "_motion").argtypes
    assert list(motion) == list(biased[:at + 1]) + [mp] + list(biased[at + 1:]), name
  # the one new struct, as the header declares it
  m = re.search(r"typedef struct mv_step_motion \{(.*?)\} mv_step_motion;", text, flags=re.S)
  members = [" ".join(d.split()) for d in m.group(1).split(";") if d.strip()]
  assert members == ["int32_t W, radius", "const float* vel", "const float* vel_far",
                     "const float* acc", "const float* acc_far", "const int32_t* prev1",
                     "const int32_t* prev0"]
  assert [f[0] for f in built_lib.mv_step_motion._fields_] == \
      ["W", "radius", "vel", "vel_far", "acc", "acc_far", "prev1", "prev0"]
  assert ctypes.sizeof(built_lib.mv_step_motion) == 8 + 6 * 8
  assert lib.mv_abi_version() == 5 == built_lib.MV_ABI_VERSION    # new symbols only
  assert lib.mv_set_motion_cost(None, 1, None, None, None, None) != 0   # NULL handle: an error
  assert ctypes.sizeof(built_lib.mv_config) == 28 * 4             # the structs keep their layout
  assert hasattr(built_lib.Engine, "set_motion_cost")
  assert list(inspect.signature(built_lib.Engine.set_motion_cost).parameters)[1:] == \
      ["radius", "vel", "vel_far", "acc", "acc_far"]
  for op in (built_lib.op_beam_step, built_lib.op_sbs_step, built_lib.op_sample_step):
    assert inspect.signature(op).parameters["motion"].default is None


# ------------------------------------------------------------ motion_tables, path_motion_cost

def test_motion_tables_are_the_plain_loops():
  for R in (1, 2, 4):
    for M in (None, 1, R):
      for sc, ac in ((0.0, 0.0), (0.25, 0.0), (0.5, 1.5)):
        t = mf.motion_tables(R, M, sc, ac)
        D = 2 * R + 1
        assert t["radius"] == R and t["vel"].shape == (D, D) and t["vel"].dtype == np.float32
        for i in range(D):
          for j in range(D):
            dy, dx = i - R, j - R
            inside = M is None or max(abs(dy), abs(dx)) <= M
            want = np.float32(-np.float32(sc) * np.float32(dy * dy + dx * dx)) if inside \
                else np.float32(-1e30)
            assert t["vel"][i, j] == want, (R, M, sc, i, j)
            if ac:
              assert t["acc"][i, j] == np.float32(-np.float32(ac) * np.float32(dy * dy + dx * dx))
        far2 = np.float32(2 * (R + 1) ** 2)
        assert t["vel_far"] == (np.float32(-1e30) if M is not None else -np.float32(sc) * far2)
        if ac:
          assert t["acc_far"] == -np.float32(ac) * far2
        else:
          assert t["acc"] is None and t["acc_far"] is None
        every = [t["vel"].ravel(), np.ravel(t["vel_far"])] + \
            ([t["acc"].ravel(), np.ravel(t["acc_far"])] if ac else [])
        assert all(np.isfinite(a).all() for a in every)
  assert np.exp(np.float32(-1e30)) == 0                   # a limit's e is exactly 0
  for bad in (dict(radius=0), dict(radius=5), dict(radius=2, max_step=0), dict(radius=2, max_step=3),
              dict(radius=2, speed_cost=-1.0), dict(radius=2, accel_cost=float("nan")),
              dict(radius=2, speed_cost=float("inf"))):
    with pytest.raises(ValueError):
      mf.motion_tables(**bad)


def test_path_motion_cost_is_the_definition_along_each_path():
  rng = np.random.RandomState(11)
  H, W, N, B, T, To, R = 9, 10, 3, 4, 5, 3, 2
  K, D = H * W, 5
  tables = {"radius": R, "vel": rng.randn(N, D, D).astype(np.float32),
            "vel_far": rng.randn(N).astype(np.float32),
            "acc": rng.randn(N, D, D).astype(np.float32),
            "acc_far": rng.randn(N).astype(np.float32)}
  labels = rng.randint(0, K, size=(N, To))
  ids = rng.randint(0, K, size=(N, B, T))
  # half of the steps short enough to fall inside the windows
  for n in range(N):
    for b in range(B):
      for t in range(0, T, 2):
        p = labels[n, -1] if t == 0 else ids[n, b, t - 1]
        y = min(max(p // W + rng.randint(-2, 3), 0), H - 1)
        x = min(max(p % W + rng.randint(-2, 3), 0), W - 1)
        ids[n, b, t] = y * W + x
  ids[2, :, 3:] = -1                                      # a row of length 3
  obs = [3, 1, 2]
  got = mf.path_motion_cost(ids, labels, W, tables, obs_lengths=obs)
  assert got.shape == (N, B, T) and got.dtype == np.float32
  inside = 0
  for n in range(N):
    for b in range(B):
      p1, p0 = labels[n, -1], (labels[n, -2] if obs[n] >= 2 else -1)
      for t in range(T):
        k = ids[n, b, t]
        if k < 0:
          assert got[n, b, t] == 0
          continue
        v, a = mo.terms(p1, p0, W, K, mo.tables_for(tables, N), n)
        assert got[n, b, t] == np.float32(v[k] + a[k]), (n, b, t)
        inside += int(v[k] != tables["vel_far"][n])
        p0, p1 = p1, k
  assert inside > N * B                                   # (the windows are exercised)
  # no acc table: the speed term alone; one row's tables serve every row
  one = {"radius": R, "vel": tables["vel"][0], "vel_far": tables["vel_far"][0], "acc": None,
         "acc_far": None}
  got1 = mf.path_motion_cost(ids[:1], labels[:1], W, one)
  v, _ = mo.terms(labels[0, -1], labels[0, -2], W, K, mo.tables_for(one, 1), 0)
  assert got1[0, 0, 0] == v[ids[0, 0, 0]]
  # W is no power of two here: the window does not wrap around a row's end
  v, _ = mo.terms(W - 1, -1, W, K, mo.tables_for(one, 1), 0)
  assert v[W] == one["vel_far"] and v[2 * W - 1] == one["vel"][R + 1, R]


# ------------------------------------------------------------ inference_feed

def test_inference_feed_carries_the_motion_cost(tmp_path):
  ds = mf_fixture.make_dataset(str(tmp_path / "fp"), n_traj=4)
  files = sorted(glob(os.path.join(ds["traj_path"], "*.txt")))
  ids = [os.path.splitext(os.path.basename(f))[0] for f in files]
  gt = mf.load_gt(ds["multifuture_path"], ids)
  plain_args = _mf_args(ds)
  inputs = mf.get_inputs(plain_args, files, gt)
  idxs = [0, 2]
  T_pred = max(inputs["max_pred_lengths"][i] for i in idxs)
  plain, _ = mf.inference_feed(inputs, plain_args, idxs, batch_size=3, pred_length=T_pred)
  assert "motion_cost" not in plain
  tables = mf.motion_tables(2, 1, 0.0, 0.5)
  args = _mf_args(ds, motion_cost=tables)
  feed, n_real = mf.inference_feed(inputs, args, idxs, batch_size=3, pred_length=T_pred)
  cost = feed["motion_cost"]
  assert n_real == 2 and cost["radius"] == 2
  assert cost["vel"].shape == (3, 5, 5) and cost["acc"].shape == (3, 5, 5)
  assert cost["vel_far"].shape == (3,) and cost["acc_far"].shape == (3,)
  for r in range(2):
    for key in ("vel", "vel_far", "acc", "acc_far"):
      assert np.array_equal(cost[key][r], tables[key]), (r, key)
  assert all((cost[key][2] == 0).all() for key in ("vel", "vel_far", "acc", "acc_far"))  # padding
  for k in plain:                                                           # all else unchanged
    a, b = plain[k], feed[k]
    if isinstance(a, list):
      assert all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b)), k
    else:
      assert np.array_equal(a, b), k
  speed_only = _mf_args(ds, motion_cost=mf.motion_tables(2, None, 0.3), class_costs=[(1, -2.0)],
                        allowed_classes=[1, 2, 3], allowed_min_share=0.25)
  feed2, _ = mf.inference_feed(inputs, speed_only, idxs, batch_size=3, pred_length=T_pred)
  assert feed2["motion_cost"]["acc"] is None and feed2["motion_cost"]["acc_far"] is None
  assert "cell_bias" in feed2 and "cell_mask" in feed2


# ------------------------------------------------------------ flags

def test_script_flags_and_their_refusals():
  flags = {f: (t, d) for f, t, d in cli._MF_FLAGS}                # pylint: disable=protected-access
  assert flags["--max_step_cells"] == (int, None) and flags["--motion_radius"] == (int, 2)
  assert flags["--speed_cost"] == (float, 0.0) and flags["--accel_cost"] == (float, 0.0)
  p = cli.multifuture_inference_parser()
  base = ["traj", "mfut", "model", "out.p"]
  off = p.parse_args(base)
  cli.parse_motion_cost(off)
  assert off.motion_cost is None
  a = p.parse_args(base + ["--max_step_cells", "1", "--accel_cost", "0.5", "--class_costs", "1:-2",
                           "--allowed_classes", "1,4", "--sample"])
  cli.parse_allowed_classes(a)
  cli.parse_class_costs(a)
  cli.parse_motion_cost(a)
  want = mf.motion_tables(2, 1, 0.0, 0.5)
  assert a.motion_cost["radius"] == 2 and np.array_equal(a.motion_cost["vel"], want["vel"])
  assert np.array_equal(a.motion_cost["acc"], want["acc"]) and a.class_costs == [(1, -2.0)]
  a = p.parse_args(base + ["--speed_cost", "0.25", "--motion_radius", "4"])
  cli.parse_motion_cost(a)
  assert a.motion_cost["radius"] == 4 and a.motion_cost["acc"] is None
  for extra, words in ((["--max_step_cells", "1", "--greedy"], ("--max_step_cells", "--greedy")),
                       (["--speed_cost", "1", "--greedy"], ("--speed_cost", "--greedy")),
                       (["--accel_cost", "1", "--score_gt", "s.p"], ("--accel_cost", "--score_gt")),
                       (["--max_step_cells", "0"], ("--max_step_cells", "at least")),
                       (["--max_step_cells", "3"], ("--max_step_cells", "--motion_radius")),
                       (["--max_step_cells", "1", "--motion_radius", "5"], ("--motion_radius",)),
                       (["--max_step_cells", "1", "--motion_radius", "0"], ("--motion_radius",)),
                       (["--speed_cost=-1"], ("--speed_cost", "finite")),
                       (["--speed_cost", "inf"], ("--speed_cost", "finite")),
                       (["--max_step_cells", "1", "--accel_cost", "nan"], ("--accel_cost", "finite")),
                       (["--speed_cost", "1", "--accel_cost=-0.5"], ("--accel_cost", "finite"))):
    with pytest.raises(SystemExit) as err:
      cli.multifuture_inference_main(base + extra)
    assert all(w in str(err.value) for w in words), (extra, str(err.value))


# ------------------------------------------------------------ the restatement

R, S, K, W = 8, 2, 70, 10
N, B = 2, 3
LIMITS = ((0, 1.0), (8, 0.9))


def _inputs(seed):
  rng = np.random.RandomState(seed)
  logits = (4.0 * rng.randn(R, K)).astype(np.float32)
  l3 = (2.0 * rng.randn(N, B, K)).astype(np.float32)
  phi, LP, G = (-rng.rand(N, B).astype(np.float32) for _ in range(3))
  return rng, logits, l3, phi, LP, G


def _tables(rng, samples, radius, acc=True):
  D = 2 * radius + 1
  t = {"radius": radius, "vel": (2.0 * rng.randn(samples, D, D)).astype(np.float32),
       "vel_far": (2.0 * rng.randn(samples)).astype(np.float32), "acc": None, "acc_far": None}
  if acc:
    t["acc"] = (2.0 * rng.randn(samples, D, D)).astype(np.float32)
    t["acc_far"] = (2.0 * rng.randn(samples)).astype(np.float32)
  return t


def _zero_tables(samples, radius, acc=True):
  """What `motion_tables` gives at cost 0 (zeros of either sign), with zero acc tables if asked."""
  t = mo.tables_for(mf.motion_tables(radius), samples)
  assert (t["vel"] == 0).all() and (t["vel_far"] == 0).all() and t["acc"] is None
  if acc:
    t["acc"], t["acc_far"] = np.zeros_like(t["vel"]), np.zeros_like(t["vel_far"])
  return t


def test_zero_tables_are_the_bias_restatement_bit_for_bit():
  rng, logits, l3, phi, LP, G = _inputs(5)
  for acc in (False, True):
    for bias_on in (False, True):
      for allowed in (None, rng.rand(R // S, K) < 0.5):
        bias = (2.0 * rng.randn(R // S, K)).astype(np.float32) if bias_on else \
            np.zeros((R // S, K), dtype=np.float32)
        p1, p0 = rng.randint(0, K, size=(R // S, S)), rng.randint(-1, K, size=(R // S, S))
        planes = mo.row_planes(p1, p0, W, K, _zero_tables(R // S, 2, acc), bias if bias_on else None)
        assert planes.tobytes() == np.repeat(bias[:, None], S, axis=1).tobytes()
        for temp in (1.0, 0.7):
          for limits in LIMITS:
            a = mo.sample_step(logits, S, 1, allowed, planes, temp, 9, limits[0], limits[1],
                               dtype=np.float32)
            b = cb.sample_step(logits, S, 1, allowed, bias, temp, 9, limits[0], limits[1],
                               dtype=np.float32)
            for k in ("keep", "tight", "wide", "ids", "q", "lp_id", "q_id", "compared"):
              assert a[k].tobytes() == b[k].tobytes(), (acc, bias_on, temp, limits, k)
      for am in (None, rng.rand(N, K) < 0.5):
        bias = (2.0 * rng.randn(N, K)).astype(np.float32) if bias_on else \
            np.zeros((N, K), dtype=np.float32)
        p1, p0 = rng.randint(0, K, size=(N, B)), rng.randint(-1, K, size=(N, B))
        planes = mo.row_planes(p1, p0, W, K, _zero_tables(N, 4, acc), bias if bias_on else None)
        for t in (0, 1):
          a = mo.sbs_step(l3, phi, LP, G, t, am, planes, 0.8, 3)
          b = cb.sbs_step(l3, phi, LP, G, t, am, bias, 0.8, 3)
          for k in ("new_phi", "new_lp", "new_g", "ids", "parents", "q"):
            assert a[k].tobytes() == b[k].tobytes(), (t, k)
        for time in (1, 2):
          for diverse in (False, True):
            a = mo.beam_step(l3, LP, am, planes, time, diverse, 0.01, 0)
            b = cb.beam_step(l3, LP, am, bias, time, diverse, 0.01, 0)
            for k in ("new_lp", "ids", "parents", "cand"):
              assert a[k].tobytes() == b[k].tobytes(), (time, diverse, k)


def test_a_first_step_is_the_bias_of_the_plane_built_from_the_labels():
  """At step 0 every row of a sample continues the observed track, so the rows' planes are one
  plane per sample, b[n, k] = (b0 + vterm) + aterm from labels[n, -1] and labels[n, -2] (no turn
  term for a row observed for one frame), and the restatement is cell_bias_oracle under it."""
  rng, logits, l3, phi, LP, G = _inputs(6)
  labels = rng.randint(0, K, size=(N, 4))
  for acc in (False, True, "limit"):
    for obs in (None, [4, 1]):
      # random tables, and a speed limit with a turn cost as `motion_tables` builds them
      tables = mf.motion_tables(2, 1, 0.25, 0.5) if acc == "limit" else _tables(rng, N, 2, acc)
      path = mo.Path(labels, B, obs)
      assert (path.p1 == labels[:, -1:]).all()
      assert (path.p0[0] == labels[0, -2]).all()
      assert (path.p0[1] == (labels[1, -2] if obs is None else -1)).all()
      b0 = (2.0 * rng.randn(N, K)).astype(np.float32)
      planes = mo.row_planes(path.p1, path.p0, W, K, tables, b0)
      want = np.empty((N, K), dtype=np.float32)
      for n in range(N):
        v, a = mo.terms(labels[n, -1], path.p0[n, 0], W, K, mo.tables_for(tables, N), n)
        assert (a == 0).all() == (not acc or path.p0[n, 0] < 0)
        want[n] = ((b0[n] + v).astype(np.float32) + a).astype(np.float32)
      assert planes.tobytes() == np.repeat(want[:, None], B, axis=1).tobytes()
      am = rng.rand(N, K) < 0.5
      a = mo.sbs_step(l3, phi, LP, G, 0, am, planes, 0.8, 3)
      b = cb.sbs_step(l3, phi, LP, G, 0, am, want, 0.8, 3)
      for k in ("new_phi", "new_lp", "new_g", "ids", "parents", "q"):
        assert a[k].tobytes() == b[k].tobytes(), k
      for diverse in (False, True):
        a = mo.beam_step(l3, LP, am, planes, 1, diverse, 0.01, 0)
        b = cb.beam_step(l3, LP, am, want, 1, diverse, 0.01, 0)
        for k in ("new_lp", "ids", "parents", "cand"):
          assert a[k].tobytes() == b[k].tobytes(), (diverse, k)
      lg = logits[:N * B]
      a = mo.sample_step(lg, B, 0, am, planes.reshape(N * B, K), 0.7, 9, 8, 0.9, dtype=np.float32)
      b = cb.sample_step(lg, B, 0, am, want, 0.7, 9, 8, 0.9, dtype=np.float32)
      for k in ("keep", "ids", "q", "lp_id", "q_id"):
        assert a[k].tobytes() == b[k].tobytes(), k


def test_a_slot_continues_its_parents_path():
  labels = np.array([[3, 14], [50, 61]])
  path = mo.Path(labels, 3)
  path.advance(np.array([[15, 24, 4], [62, 51, 60]]), np.array([[0, 0, 0], [0, 0, 0]]))
  assert (path.p0 == labels[:, -1:]).all() and path.p1[1, 2] == 60
  path.advance(np.array([[25, 16, 26], [52, 63, 41]]), np.array([[1, 0, 1], [1, 0, 2]]))
  assert path.p0.tolist() == [[24, 15, 24], [51, 62, 60]]   # ids[t-1] of the PARENT slot
  path.advance(np.array([[1, 2, 3], [4, 5, 6]]))             # rows that continue themselves
  assert path.p0.tolist() == [[25, 16, 26], [52, 63, 41]]
  # along rows that continue themselves the walk pays what path_motion_cost reports
  rng = np.random.RandomState(3)
  tables = _tables(rng, 2, 2)
  ids = rng.randint(0, K, size=(2, 3, 4))
  walk, paid = mo.Path(labels, 3), np.zeros((2, 3, 4), dtype=np.float32)
  for t in range(4):
    planes = mo.row_planes(walk.p1, walk.p0, W, K, tables)
    paid[:, :, t] = np.take_along_axis(planes, ids[:, :, t, None], axis=-1)[..., 0]
    walk.advance(ids[:, :, t])
  assert paid.tobytes() == mf.path_motion_cost(ids, labels, W, tables).tobytes()
