# coding=utf-8
"""GPU: per-row observation lengths (mv_set_obs_lengths, feed["obs_lengths"]).  One forward
encodes rows of different history lengths, right-aligned; row n of every output of every
forward kind must be, bit for bit, row n of a uniform forward of an engine created with
obs_len = Lo[n] (same weights) on the row's last Lo[n] columns; the columns in front are
ignored; and the encoder steps a row has not reached must really not be launched
(mv_last_forward_gate_rows against the closed form)."""
import argparse
import functools
import os
import pickle
import shutil

import numpy as np
import pytest

from multiverse_amd import cli, multifuture as mf, synth, tf_checkpoint
from oracle import multiverse_oracle as oracle

import mf_fixture

pytestmark = pytest.mark.gpu

TOL = 1e-4          # the project's bar on logits and offsets against the oracle
T_OBS = 4
T_MAX = 5
BEAM_CASES = {"sorted": [4, 3, 3, 1, 1], "late": [3, 2, 2, 1, 1], "unsorted": [1, 4, 2, 4, 3]}
GREEDY_CASES = {"sorted": [4, 3, 2, 1], "unsorted": [2, 4, 1, 3]}
VARIANT_CASE = [4, 2, 1]                 # sorted: a runner, a mid-way joiner, a one-step row
BOTH_PRED, BOTH_OBS = [5, 3, 3, 1, 0], [4, 1, 3, 2, 4]


def _centers(cfg):
  return mf.add_grid(argparse.Namespace(
      grid_strides="2,4", use_grids=[bool(u) for u in cfg.use_grids], scene_h=36, scene_w=64,
      video_h=1080, video_w=1920)).scene_grid_centers


def _with_obs_len(cfg, L):
  out = argparse.Namespace(**vars(cfg))
  out.obs_len = L
  return out


def _make_feed(cfg, seed):
  """synth.make_feed with a scene frame of its own per (row, column): a wrong window of the
  scene mean or a wrong frame of a step cannot hide behind equal frames."""
  feed = synth.make_feed(cfg, seed=seed, frames_per_group=1, pred_len=T_MAX)
  U = feed["scene_feat"].shape[0]
  n, t = np.meshgrid(np.arange(cfg.batch_size), np.arange(cfg.obs_len), indexing="ij")
  feed["obs_scene"] = ((n + 2 * t) % U).astype("int32")
  return feed


def _last_columns(feed, L):
  """The feed of an engine with obs_len = L: the last L observation columns."""
  out = dict(feed)
  out.pop("obs_lengths", None)
  out["obs_scene"] = np.ascontiguousarray(feed["obs_scene"][:, -L:])
  out["grid_obs_labels"] = [np.ascontiguousarray(a[:, -L:]) for a in feed["grid_obs_labels"]]
  out["grid_obs_regress"] = [np.ascontiguousarray(a[:, -L:]) for a in feed["grid_obs_regress"]]
  out["obs_xy"] = np.ascontiguousarray(feed["obs_xy"][:, -L:])
  return out


def _engine(lib, cfg, params, mode, centers=True):
  eng = lib.Engine(cfg, device=0)
  eng.set_params(params)
  eng.set_compute_mode(mode)
  if centers:
    eng.set_grid_centers(_centers(cfg))
  return eng


# ------------------------------------------------------------------ beam handles

def _beam_cfg(**over):
  cfg = synth.default_config(batch_size=over.pop("batch_size", 5), use_grids=(0, 1), beam_size=3,
                             **over)
  cfg.obs_len = T_OBS
  cfg.max_pred_len = T_MAX
  return cfg


def _beam_forward(eng, feed, decoded=True):
  arrs, _ = eng.forward_beam(feed)
  arrs = dict(arrs)
  if decoded:
    arrs["trajs"] = eng.decode_trajectories()
    arrs["occupancy"] = eng.beam_occupancy()
  arrs["gate_rows"] = eng.last_forward_gate_rows()
  return arrs


def _row(arrs, cfg, n):
  """Row n of every output field."""
  N, B = cfg.batch_size, cfg.beam_size
  out = {}
  for name, a in arrs.items():
    if name == "gate_rows":
      continue
    if name == "grid_reg" and a.shape[0] == N * B:        # use_single_decoder: per beam
      out[name] = a[n * B:(n + 1) * B]
    else:
      out[name] = a[n]
  return out


def _assert_rows_equal(got, want, cfg, n, what):
  g, w = _row(got, cfg, n), _row(want, cfg, n)
  assert sorted(g) == sorted(w), (what, sorted(g), sorted(w))
  for name in g:
    assert g[name].shape == w[name].shape, (what, n, name)
    assert g[name].tobytes() == w[name].tobytes(), (what, n, name)


SAMPLING = {"sampled": dict(temperature=1.3, seed=77),
            "wor": dict(temperature=1.3, seed=78, without_replacement=True)}


@functools.lru_cache(maxsize=None)
def _beam_runs():
  """Every forward of the f16x3 beam handle the tests below compare: the obs_len = 4 engine's
  (obs-ragged and uniform), then those of the reference engines with obs_len 1 .. 4."""
  import multiverse_amd._lib as lib
  cfg = _beam_cfg()
  params = synth.make_params(cfg, seed=synth.SEED_BASE + 41, recurrent_gain=3.0, bias_scale=0.1)
  feed = _make_feed(cfg, synth.SEED_BASE + 41)
  runs = {}
  eng = _engine(lib, cfg, params, "f16x3")
  # obs-ragged before and after a uniform forward: nothing may leak either way
  runs["unsorted"] = _beam_forward(eng, dict(feed, obs_lengths=BEAM_CASES["unsorted"]))
  runs["uniform"] = _beam_forward(eng, feed)
  runs["sorted"] = _beam_forward(eng, dict(feed, obs_lengths=BEAM_CASES["sorted"]))
  runs["late"] = _beam_forward(eng, dict(feed, obs_lengths=BEAM_CASES["late"]))
  runs["all4"] = _beam_forward(eng, dict(feed, obs_lengths=[T_OBS] * cfg.batch_size))
  runs["uniform_again"] = _beam_forward(eng, feed)
  # ignored columns: other in-range labels / frame indices / finite offsets in front
  other = _make_feed(cfg, synth.SEED_BASE + 42)
  scribbled = dict(feed)
  for key in ("obs_scene", "obs_xy"):
    scribbled[key] = feed[key].copy()
  for key in ("grid_obs_labels", "grid_obs_regress"):
    scribbled[key] = [a.copy() for a in feed[key]]
  for n, L in enumerate(BEAM_CASES["unsorted"]):
    scribbled["obs_scene"][n, :T_OBS - L] = other["obs_scene"][n, :T_OBS - L][::-1]
    scribbled["obs_xy"][n, :T_OBS - L] = other["obs_xy"][n, :T_OBS - L]
    for s in range(2):
      scribbled["grid_obs_labels"][s][n, :T_OBS - L] = other["grid_obs_labels"][s][n, :T_OBS - L]
      scribbled["grid_obs_regress"][s][n, :T_OBS - L] = \
          -3.0 * other["grid_obs_regress"][s][n, :T_OBS - L]
  assert not np.array_equal(scribbled["grid_obs_labels"][1], feed["grid_obs_labels"][1])
  runs["scribbled"] = _beam_forward(eng, dict(scribbled, obs_lengths=BEAM_CASES["unsorted"]))
  # the compact upload takes the lengths the same way (obs_xy right-aligned)
  runs["compact"] = dict(eng.forward_beam_compact(
      dict(feed, obs_lengths=BEAM_CASES["unsorted"]))[0])
  # both kinds of lengths at once
  runs["both"] = _beam_forward(eng, dict(feed, obs_lengths=BOTH_OBS, pred_lengths=BOTH_PRED))
  # sampled, sampled without replacement, scored
  for kind, kw in SAMPLING.items():
    eng.set_sampling(**kw)
    runs[kind] = _beam_forward(eng, dict(feed, obs_lengths=BEAM_CASES["sorted"]))
  eng.clear_sampling()
  ids = runs["sampled"]["ids"]
  runs["scored"] = eng.score_futures(dict(feed, obs_lengths=BEAM_CASES["sorted"]), ids)
  runs["scored"]["logits"] = eng.download_beam()[0]["logits"]
  eng.close()
  for L in range(1, T_OBS + 1):
    ref = _engine(lib, _with_obs_len(cfg, L), params, "f16x3")
    f = _last_columns(feed, L)
    runs["ref%d" % L] = _beam_forward(ref, f)
    for Lp in sorted({p for p, o in zip(BOTH_PRED, BOTH_OBS) if o == L and p not in (0, T_MAX)}):
      runs["ref%d_pred%d" % (L, Lp)] = _beam_forward(ref, dict(f, pred_length=Lp))
    for kind, kw in SAMPLING.items():
      ref.set_sampling(**kw)
      runs["ref%d_%s" % (L, kind)] = _beam_forward(ref, f)
    ref.clear_sampling()
    runs["ref%d_scored" % L] = ref.score_futures(f, ids)
    runs["ref%d_scored" % L]["logits"] = ref.download_beam()[0]["logits"]
    ref.close()
  return cfg, params, feed, runs


@pytest.mark.parametrize("case", sorted(BEAM_CASES))
def test_beam_rows_are_bitwise_the_engine_of_their_obs_len(built_lib, case):
  cfg, _, _, runs = _beam_runs()
  for n, L in enumerate(BEAM_CASES[case]):
    _assert_rows_equal(runs[case], runs["ref%d" % L], cfg, n, (case, L))


def test_uniform_forward_between_obs_ragged_ones_is_untouched(built_lib):
  cfg, _, _, runs = _beam_runs()
  for n in range(cfg.batch_size):
    _assert_rows_equal(runs["uniform"], runs["ref%d" % T_OBS], cfg, n, "uniform")
    _assert_rows_equal(runs["uniform_again"], runs["uniform"], cfg, n, "uniform again")


def test_all_lengths_equal_obs_len_is_the_uniform_forward(built_lib):
  cfg, _, _, runs = _beam_runs()
  for n in range(cfg.batch_size):
    _assert_rows_equal(runs["all4"], runs["uniform"], cfg, n, "all4")
  assert runs["all4"]["gate_rows"] == runs["uniform"]["gate_rows"]


def test_ignored_columns_change_nothing(built_lib):
  cfg, _, _, runs = _beam_runs()
  for n in range(cfg.batch_size):
    _assert_rows_equal(runs["scribbled"], runs["unsorted"], cfg, n, "scribbled")


def test_compact_upload_takes_the_lengths(built_lib):
  cfg, _, _, runs = _beam_runs()
  for name, a in runs["compact"].items():
    assert a.tobytes() == runs["unsorted"][name].tobytes(), name


@pytest.mark.parametrize("kind", sorted(SAMPLING) + ["scored"])
def test_sampled_and_scored_rows_are_bitwise_the_engine_of_their_obs_len(built_lib, kind):
  cfg, _, _, runs = _beam_runs()
  if kind == "wor":
    assert "gumbels" in runs[kind]
  for n, L in enumerate(BEAM_CASES["sorted"]):
    _assert_rows_equal(runs[kind], runs["ref%d_%s" % (L, kind)], cfg, n, (kind, L))


def test_scoring_the_drawn_ids_returns_their_logprobs(built_lib):
  _, _, _, runs = _beam_runs()
  assert runs["scored"]["logprobs"].tobytes() == runs["sampled"]["logprobs"].tobytes()
  assert (runs["scored"]["ranks"] >= 0).all()


def test_obs_and_pred_lengths_together(built_lib):
  """Row n = the (obs_len = Lo[n], pred_len = L[n]) uniform forward; zeros / -1 past its end."""
  cfg, _, _, runs = _beam_runs()
  got_all = runs["both"]

  def cut(name, a, lo, hi):
    if name == "logprobs":
      return a
    if name in ("best_beam", "grid_reg", "occupancy"):      # [T, ..] per row
      return a[lo:hi]
    return a[:, lo:hi]                                      # [B, T, ..] per row

  for n, (Lp, Lo) in enumerate(zip(BOTH_PRED, BOTH_OBS)):
    got = _row(got_all, cfg, n)
    want_run = runs["ref%d" % Lo] if Lp in (0, T_MAX) else runs["ref%d_pred%d" % (Lo, Lp)]
    want = _row(want_run, cfg, n)
    for name, a in got.items():
      if name != "logprobs":
        tail = cut(name, a, Lp, T_MAX)
        assert (tail == (-1 if name == "ids" else 0)).all(), (n, name)
      if Lp == 0:
        assert name != "logprobs" or (a == 0).all(), n
        continue
      head = cut(name, a, 0, Lp)
      assert head.shape == want[name].shape, (n, name, head.shape, want[name].shape)
      assert head.tobytes() == want[name].tobytes(), (n, Lo, Lp, name)


def _beam_gate_rows(cfg, obs_lens, pred_lens=None):
  """chains x sum_t p_t for the encoders + the decoder rows of tests/test_gpu_ragged.py."""
  N, B = cfg.batch_size, cfg.beam_size
  pred_lens = pred_lens or [T_MAX] * N
  A = [max([n + 1 for n, l in enumerate(pred_lens) if l > t] or [0]) for t in range(T_MAX)]
  enc = 2 * mf.sum_enc_prefix_rows(obs_lens, T_OBS, live_rows=A[0])
  return enc + sum(A) + A[0] + B * sum(A[1:])


def test_unstarted_rows_are_not_launched(built_lib):
  cfg, _, _, runs = _beam_runs()
  N = cfg.batch_size
  uniform = runs["uniform"]["gate_rows"]
  assert uniform == _beam_gate_rows(cfg, [T_OBS] * N)
  for case, lens in BEAM_CASES.items():
    assert runs[case]["gate_rows"] == _beam_gate_rows(cfg, lens), case
    assert runs[case]["gate_rows"] < uniform, case
  assert mf.sum_enc_prefix_rows(BEAM_CASES["sorted"], T_OBS) == sum(BEAM_CASES["sorted"])
  assert mf.sum_enc_prefix_rows(BEAM_CASES["unsorted"], T_OBS) > sum(BEAM_CASES["unsorted"])
  assert runs["both"]["gate_rows"] == _beam_gate_rows(cfg, BOTH_OBS, BOTH_PRED)


def test_beam_against_the_oracle_at_every_obs_len(built_lib):
  cfg, params, feed, runs = _beam_runs()
  lens = BEAM_CASES["sorted"]
  rag = runs["sorted"]
  for L in sorted(set(lens)):
    _, oreg, (ologits, oids, _) = oracle.forward(params, _with_obs_len(cfg, L),
                                                 _last_columns(feed, L))
    oreg = np.asarray(oreg[1])
    for n in [n for n in range(cfg.batch_size) if lens[n] == L]:
      assert (rag["ids"][n] == oids[n]).all(), (L, n)
      d = float(np.abs(rag["logits"][n] - ologits[n]).max())
      r = float(np.abs(rag["grid_reg"][n] - oreg[n]).max())
      print("obs_len %d n=%d: logits %.3g offsets %.3g (bar %g)" % (L, n, d, r, TOL))
      assert d < TOL and r < TOL, (L, n, d, r)


def test_graph_mode_issues_obs_ragged_forwards_eagerly(built_lib):
  cfg, params, feed, runs = _beam_runs()
  eng = _engine(built_lib, cfg, params, "f16x3")
  eng.set_graph_mode(True)
  for key, f in (("uniform", feed),                                      # captured
                 ("sorted", dict(feed, obs_lengths=BEAM_CASES["sorted"])),
                 ("unsorted", dict(feed, obs_lengths=BEAM_CASES["unsorted"])),
                 ("uniform", feed),                                      # replayed
                 ("all4", dict(feed, obs_lengths=[T_OBS] * cfg.batch_size))):
    got = _beam_forward(eng, f)
    for n in range(cfg.batch_size):
      _assert_rows_equal(got, runs[key], cfg, n, ("graph", key))
    assert got["gate_rows"] == runs[key]["gate_rows"], key
  eng.close()


# ------------------------------------------------------------------ variants on the beam handle

VARIANTS = {
    "f32": dict(mode="f32"),
    "bf16": dict(mode="bf16"),
    "kernel5": dict(mode="f32", convlstm_kernel=5),
    "noscene": dict(mode="f16x3", use_scene_enc=False),
    "single_decoder": dict(mode="f16x3", use_single_decoder=True),
}


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_variant_rows_are_bitwise_the_engine_of_their_obs_len(built_lib, name):
  over = dict(VARIANTS[name])
  mode = over.pop("mode")
  cfg = _beam_cfg(batch_size=len(VARIANT_CASE), **over)
  params = synth.make_params(cfg, seed=synth.SEED_BASE + 43, recurrent_gain=3.0, bias_scale=0.1)
  feed = _make_feed(cfg, synth.SEED_BASE + 43)
  decoded = not cfg.use_single_decoder        # single decoder + beam decodes on the host only
  eng = _engine(built_lib, cfg, params, mode, centers=decoded)
  got = _beam_forward(eng, dict(feed, obs_lengths=VARIANT_CASE), decoded)
  eng.close()
  for n, L in enumerate(VARIANT_CASE):
    ref = _engine(built_lib, _with_obs_len(cfg, L), params, mode, centers=decoded)
    want = _beam_forward(ref, _last_columns(feed, L), decoded)
    ref.close()
    _assert_rows_equal(got, want, cfg, n, (name, L))


# ------------------------------------------------------------------ greedy, both scales

@functools.lru_cache(maxsize=None)
def _greedy_runs():
  import multiverse_amd._lib as lib
  cfg = synth.default_config(batch_size=4, use_grids=(1, 1))
  cfg.obs_len = T_OBS
  cfg.max_pred_len = T_MAX
  params = synth.make_params(cfg, seed=synth.SEED_BASE + 44, recurrent_gain=3.0, bias_scale=0.1)
  feed = _make_feed(cfg, synth.SEED_BASE + 44)
  feed["pred_length"] = 3

  def run(eng, f):
    cls, reg = eng.forward_greedy(f)
    return {"cls": cls, "reg": reg, "gate_rows": eng.last_forward_gate_rows(),
            "trajs": [eng.decode_trajectories(scale=s) for s in range(2)]}
  runs = {}
  eng = _engine(lib, cfg, params, "f16x3")
  runs["unsorted"] = run(eng, dict(feed, obs_lengths=GREEDY_CASES["unsorted"]))
  runs["uniform"] = run(eng, feed)
  runs["sorted"] = run(eng, dict(feed, obs_lengths=GREEDY_CASES["sorted"]))
  eng.close()
  for L in range(1, T_OBS + 1):
    ref = _engine(lib, _with_obs_len(cfg, L), params, "f16x3")
    runs[L] = run(ref, _last_columns(feed, L))
    ref.close()
  return cfg, params, feed, runs


@pytest.mark.parametrize("case", sorted(GREEDY_CASES) + ["uniform"])
def test_greedy_rows_are_bitwise_the_engine_of_their_obs_len(built_lib, case):
  cfg, _, _, runs = _greedy_runs()
  lens = GREEDY_CASES.get(case, [T_OBS] * cfg.batch_size)
  for s in range(2):
    for n, L in enumerate(lens):
      for name in ("cls", "reg", "trajs"):
        a, b = runs[case][name][s][n], runs[L][name][s][n]
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (case, s, n, L, name)


def test_greedy_unstarted_rows_are_not_launched(built_lib):
  cfg, _, _, runs = _greedy_runs()
  N, Tp = cfg.batch_size, 3

  def closed_form(lens):       # per scale: two encoder chains, two decoder chains of N rows
    return 2 * (2 * mf.sum_enc_prefix_rows(lens, T_OBS) + 2 * N * Tp)
  assert runs["uniform"]["gate_rows"] == closed_form([T_OBS] * N)
  for case, lens in GREEDY_CASES.items():
    assert runs[case]["gate_rows"] == closed_form(lens), case
    assert runs[case]["gate_rows"] < runs["uniform"]["gate_rows"], case
  assert closed_form(GREEDY_CASES["sorted"]) == 2 * (2 * sum(GREEDY_CASES["sorted"]) + 2 * N * Tp)


def test_greedy_against_the_oracle_at_every_obs_len(built_lib):
  cfg, params, feed, runs = _greedy_runs()
  lens = GREEDY_CASES["sorted"]
  Tp = 3
  for L in sorted(set(lens)):
    ocls, oreg, _ = oracle.forward(params, _with_obs_len(cfg, L), _last_columns(feed, L))
    for s in range(2):
      for n in [n for n in range(cfg.batch_size) if lens[n] == L]:
        got_c, got_r = runs["sorted"]["cls"][s][n], runs["sorted"]["reg"][s][n]
        K = ocls[s][n].reshape(Tp, -1).shape[1]
        assert (got_c.reshape(Tp, K).argmax(-1) == ocls[s][n].reshape(Tp, K).argmax(-1)).all()
        d = float(np.abs(got_c - ocls[s][n]).max())
        r = float(np.abs(got_r - oreg[s][n]).max())
        print("obs_len %d scale %d n=%d: logits %.3g offsets %.3g (bar %g)" % (L, s, n, d, r, TOL))
        assert d < TOL and r < TOL, (L, s, n, d, r)


# ------------------------------------------------------------------ refusals

def test_errors_name_the_call(built_lib):
  cfg = synth.default_config(batch_size=2, use_grids=(0, 1), is_train=True)
  cfg.obs_len = T_OBS
  cfg.max_pred_len = cfg.pred_len = 3
  params = synth.make_params(cfg, seed=synth.SEED_BASE + 45, recurrent_gain=3.0, bias_scale=0.1)
  feed = synth.make_feed(cfg, seed=synth.SEED_BASE + 45, pred_len=3)
  eng = built_lib.Engine(cfg, device=0)
  eng.set_params(params)
  uni = eng.forward_greedy(feed)
  for bad in (0, T_OBS + 1):
    with pytest.raises(built_lib.MvError, match=r"obs_lengths\[1\] = %d not in \[1, obs_len=4\]" % bad):
      eng.forward_greedy(dict(feed, obs_lengths=[T_OBS, bad]))
  with pytest.raises(built_lib.MvError, match="obs_lengths: 3 values for batch_size 2"):
    eng.forward_greedy(dict(feed, obs_lengths=[4, 2, 1]))
  short = dict(feed, obs_lengths=[4, 2])
  rag = eng.forward_greedy(short)                                # lengths stay set
  assert rag[0][1][0].tobytes() == uni[0][1][0].tobytes()
  assert rag[0][1][1].tobytes() != uni[0][1][1].tobytes()
  with pytest.raises(built_lib.MvError, match="mv_submit_greedy.*mv_set_obs_lengths"):
    eng.submit_greedy(short)
  with pytest.raises(built_lib.MvError, match="mv_train_init.*mv_set_obs_lengths"):
    eng.train_init(cfg)
  again = eng.forward_greedy(feed)                               # the feed clears them
  assert again[0][1].tobytes() == uni[0][1].tobytes()
  eng.train_init(cfg)
  eng.forward_greedy(short)
  # (a feed without "obs_lengths" clears them: the resident forms keep what is set)
  for call, name in ((lambda: eng.train_step(None), "mv_train_step"),
                     (lambda: eng.train_forward_backward(None), "mv_train_forward_backward"),
                     (lambda: eng.train_apply(1.0), "mv_train_apply"),
                     (eng.attack_begin, "mv_attack_begin"),
                     (lambda: eng.attack_step(0.1, 0.1), "mv_attack_step")):
    with pytest.raises(built_lib.MvError, match=name + ".*mv_set_obs_lengths"):
      call()
  # all lengths == obs_len: nothing is refused
  full = dict(feed, obs_lengths=[T_OBS, T_OBS])
  eng.forward_greedy(full)
  losses = eng.train_step(full)
  assert np.isfinite(losses[0])
  assert np.isfinite(eng.train_step(None)[0])                    # ... and they stay set
  eng.close()


# ------------------------------------------------------------------ command line

CLI_LENGTHS = {1: 5, 2: 2, 3: 5}       # sample index -> observed frames (the others keep 8)


def _cli(ds, model_dir, out_file, obs_length, extra):
  cli.multifuture_inference_main(
      [ds["traj_path"], ds["multifuture_path"], model_dir, out_file,
       "--num_out", "3", "--emb_size", "32", "--use_grids", "0,1", "--use_gnn",
       "--use_scene_enc", "--diverse_beam", "--diverse_gamma", "0.01",
       "--fix_num_timestep", "1", "--scene_feat_path", ds["scene_feat_path"],
       "--scene_id2name", ds["scene_id2name"], "--obs_length", str(obs_length)] + extra)
  with open(out_file, "rb") as f:
    return pickle.load(f)


def test_multifuture_cli_allow_short_obs(built_lib, tmp_path):
  ds = mf_fixture.make_dataset(str(tmp_path / "fp"), n_traj=4)
  cfg = synth.default_config(batch_size=1, use_grids=(0, 1), beam_size=3)
  params = synth.make_params(cfg, seed=synth.SEED_BASE + 46, recurrent_gain=3.0, bias_scale=0.1)
  model_dir = str(tmp_path / "model")
  tf_checkpoint.save_checkpoint(os.path.join(model_dir, "save-best"), params, global_step=100)
  # a copy whose tracks 1, 2, 3 entered the scene late: their first frames are gone (two
  # lines per frame: the agent and another one)
  short_dir = str(tmp_path / "traj_short")
  os.makedirs(short_dir)
  lengths = {}
  for k, traj_id in enumerate(ds["traj_ids"]):
    with open(os.path.join(ds["traj_path"], traj_id + ".txt")) as f:
      lines = f.read().splitlines()
    L = CLI_LENGTHS.get(k, 8)
    lengths[traj_id] = L
    with open(os.path.join(short_dir, traj_id + ".txt"), "w") as f:
      f.write("\n".join(lines[2 * (8 - L):]) + "\n")
  short = dict(ds, traj_path=short_dir)
  with pytest.raises(AssertionError):
    _cli(short, model_dir, str(tmp_path / "refused.p"), 8, ["--batch_size", "4"])
  got = _cli(short, model_dir, str(tmp_path / "short.p"), 8,
             ["--batch_size", "4", "--ragged_batches", "--allow_short_obs"])
  assert sorted(got) == sorted(ds["traj_ids"])
  # every sample alone, on an engine of its own obs_length
  for traj_id, L in lengths.items():
    one_dir = str(tmp_path / ("one_" + traj_id))
    os.makedirs(one_dir)
    shutil.copy(os.path.join(short_dir, traj_id + ".txt"), one_dir)
    want = _cli(dict(ds, traj_path=one_dir), model_dir, str(tmp_path / (traj_id + ".p")), L, [])
    a, b = np.asarray(got[traj_id]), np.asarray(want[traj_id])
    assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), (traj_id, L)
