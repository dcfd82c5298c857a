# coding=utf-8
"""GPU: the multi-future decode on the device (csrc/multifuture_decode.h,
mv_decode_trajectories / mv_beam_occupancy) -- trajectories bit-identical to the host
decode of the same run's downloaded outputs, the occupancy map against the reference's
float32 arithmetic (yardstick: that arithmetic against fp64) and against the maps the
reference's own script made from the frozen beam fixtures
(tests/golden/make_multifuture_decode_records.py)."""
import argparse
import os
import pickle
import sys

import numpy as np
import pytest

from multiverse_amd import cli, multifuture as mf, pred_models, synth, tf_checkpoint

import mf_fixture
import noscene_golden as ng
import shim_golden as sg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import reference_records  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURES = ["golden_shim_beam20_s0.npz", "golden_shim_beam_s1.npz",
            "golden_shim_noscene_beam20_s0.npz"]
CASES = FIXTURES + ["synthetic_n8_beam20_t9"]


def _case(name):
  """(fixture or None, cfg, params, feed, compute mode)."""
  if name == "synthetic_n8_beam20_t9":
    cfg = synth.default_config(batch_size=8, use_grids=(1, 0), beam_size=20)
    params = synth.make_params(cfg, seed=synth.SEED_BASE + 2, recurrent_gain=3.0,
                               bias_scale=0.1)
    return None, cfg, params, synth.make_feed(cfg, seed=synth.SEED_BASE + 2, pred_len=9), \
        "f16x3"
  g, cfg, params, feed = (ng.forward_case(name) if "noscene" in name
                          else sg.forward_case(name))
  return g, cfg, params, feed, "f32"


def _args(cfg, **over):
  """The multi-future script's view of the grids (centres as add_grid builds them)."""
  a = mf.add_grid(argparse.Namespace(
      grid_strides="2,4", use_grids=[bool(u) for u in cfg.use_grids], scene_h=36, scene_w=64,
      video_h=1080, video_w=1920, greedy=False, center_only=False, num_out=cfg.beam_size))
  for k, v in over.items():
    setattr(a, k, v)
  return a


def _engine(lib, cfg, params, mode, centers=True):
  eng = lib.Engine(cfg, device=0)
  eng.set_params(params)
  eng.set_compute_mode(mode)
  if centers:
    eng.set_grid_centers(_args(cfg).scene_grid_centers)
  return eng


def _host_trajs(cfg, arrs, s, T, center_only):
  args = _args(cfg, center_only=center_only)
  out = []
  for n in range(cfg.batch_size):
    out.append(mf.decode_trajectories(
        args, None, arrs["grid_reg"][n],
        (arrs["logits"][n], arrs["ids"][n], arrs["logprobs"][n]), T, s))
  return np.asarray(out)                                  # [N, B, T, 2] float64


def _mixture(logits, logprobs, dtype):
  """The formula of eval_grid_nll / the reference's script for every t: [N, T, K]."""
  out = []
  for n in range(logits.shape[0]):
    if dtype == np.float32:                               # exactly as eval_grid_nll does
      probs = mf._softmax(np.squeeze(logprobs[n][None]))
      beams = mf._softmax(np.squeeze(logits[n][None]), axis=-1)
      out.append(np.stack([
          (beams[:, t, :].astype("float32") * probs[:, None].astype("float32")).sum(0)
          for t in range(beams.shape[1])]))
    else:
      probs = mf._softmax(logprobs[n].astype(np.float64))
      beams = mf._softmax(logits[n].astype(np.float64), axis=-1)
      out.append((beams * probs[:, None, None]).sum(0))
  return np.stack(out)


@pytest.mark.parametrize("name", CASES)
def test_beam_trajectories_are_bit_identical_to_the_host_decode(built_lib, name):
  _, cfg, params, feed, mode = _case(name)
  eng = _engine(built_lib, cfg, params, mode)
  arrs, s = eng.forward_beam(feed)
  T = feed["pred_length"]
  for center_only in (False, True):
    dev = eng.decode_trajectories(center_only=center_only)
    want = _host_trajs(cfg, arrs, s, T, center_only)
    assert dev.dtype == np.float64 and dev.shape == want.shape == \
        (cfg.batch_size, cfg.beam_size, T, 2)
    assert (dev == want).all(), (name, center_only, np.abs(dev - want).max())
  ids, lp = eng.beam_ids()
  assert (ids == arrs["ids"]).all() and (lp == arrs["logprobs"]).all()
  eng.close()


def test_greedy_trajectories_and_the_tie_rule(built_lib):
  g, cfg, params, feed = sg.forward_case("golden_shim_greedy_both.npz")
  N, T = cfg.batch_size, feed["pred_length"]
  zero = dict(params)
  for s in range(2):
    k = "person_pred/hidden2grid_decoder_grid_class_%d/out_dec_grid/W" % s
    zero[k] = np.zeros_like(params[k])
  for tied, p in ((False, params), (True, zero)):
    eng = _engine(built_lib, cfg, p, "f32")
    cls, reg = eng.forward_greedy(feed)
    for s in range(2):
      if tied:
        assert (cls[s] == 0).all()                        # every row one K-way tie
      for center_only in (False, True):
        args = _args(cfg, greedy=True, center_only=center_only, num_out=1)
        dev = eng.decode_trajectories(scale=s, center_only=center_only)
        want = np.asarray([mf.decode_trajectories(args, cls[s][n], reg[s][n], None, T, s)
                           for n in range(N)])
        assert dev.shape == want.shape == (N, 1, T, 2) and dev.dtype == np.float64
        assert (dev == want).all(), (tied, s, center_only)
        if tied:                                          # numpy's argmax: cell 0
          c0 = args.scene_grid_centers[s].reshape(-1, 2)[0]
          off = 0.0 if center_only else reg[s].reshape(N, T, -1, 2)[:, :, 0].astype(np.float64)
          assert (dev[:, 0] == c0 + off).all()
    eng.close()


@pytest.mark.parametrize("name", CASES)
def test_occupancy_kernel_arithmetic_against_fp64(built_lib, name):
  """Distance to an fp64 evaluation of the mixture on the engine's own logits: the device
  map may be 4 x as far as the reference's float32 arithmetic is (a different but equally
  legitimate fp32 summation order and the device expf).  Both distances are printed."""
  _, cfg, params, feed, mode = _case(name)
  eng = _engine(built_lib, cfg, params, mode)
  arrs, _ = eng.forward_beam(feed)
  dev = eng.beam_occupancy()
  eng.close()
  exact = _mixture(arrs["logits"], arrs["logprobs"], np.float64)
  ref32 = _mixture(arrs["logits"], arrs["logprobs"], np.float32)
  assert dev.dtype == np.float32 and dev.shape == exact.shape and ref32.dtype == np.float32
  d_ref = float((np.abs(ref32 - exact) / exact).max())
  d_dev = float((np.abs(dev - exact) / exact).max())
  rows = float(np.abs(dev.astype(np.float64).sum(-1) - 1).max())
  print("%s: reference float32 vs fp64 %.3g, device vs fp64 %.3g (bar %.3g), rows sum to 1 "
        "within %.3g" % (name, d_ref, d_dev, 4 * d_ref, rows))
  assert d_dev <= 4 * d_ref
  assert rows <= 1e-6


@pytest.mark.parametrize("name", FIXTURES)
def test_occupancy_against_the_recorded_reference_maps(built_lib, name):
  """2.2e-3 relative = 2 x 1e-4 (the bar on logits) + 2 x 1e-3 (the bar on beam
  log-probabilities, tests/beam_compare.py): a softmax turns an input error d into at most
  2 d relative."""
  g, cfg, params, feed, mode = _case(name)
  rec = reference_records.load("multifuture_decode")[name]
  eng = _engine(built_lib, cfg, params, mode)
  arrs, _ = eng.forward_beam(feed)
  dev = eng.beam_occupancy()
  eng.close()
  assert (arrs["ids"] == g["beam_ids"]).all()
  d = float((np.abs(dev - rec["occupancy"]) / rec["occupancy"]).max())
  print("%s: device map vs the reference script's map: %.3g relative (bar 2.2e-3)" % (name, d))
  assert d <= 2.2e-3


def test_determinism_and_row_independence(built_lib):
  _, cfg, params, feed, mode = _case("synthetic_n8_beam20_t9")
  eng = _engine(built_lib, cfg, params, mode)
  eng.upload(feed)
  eng.run_resident(True)
  t0, o0 = eng.decode_trajectories(), eng.beam_occupancy()
  t1, o1 = eng.decode_trajectories(), eng.beam_occupancy()
  assert (t0 == t1).all() and (o0 == o1).all()            # two calls after one forward
  eng.run_resident(True)
  t2, o2 = eng.decode_trajectories(), eng.beam_occupancy()
  assert (t0 == t2).all() and (o0 == o2).all()            # after a second forward
  eng.close()
  cfg1 = synth.default_config(batch_size=1, use_grids=(1, 0), beam_size=20)
  eng1 = _engine(built_lib, cfg1, params, mode)
  for n in range(cfg.batch_size):
    f1 = dict(feed)
    uniq, inv = np.unique(feed["obs_scene"][n], return_inverse=True)
    f1["scene_feat"] = np.ascontiguousarray(feed["scene_feat"][uniq])
    f1["obs_scene"] = np.ascontiguousarray(inv.reshape(1, -1).astype("int32"))
    f1["grid_obs_labels"] = [a[n:n + 1] for a in feed["grid_obs_labels"]]
    f1["grid_obs_regress"] = [a[n:n + 1] for a in feed["grid_obs_regress"]]
    eng1.upload(f1)
    eng1.run_resident(True)
    assert (eng1.decode_trajectories()[0] == t0[n]).all(), n
    assert (eng1.beam_occupancy()[0] == o0[n]).all(), n
  eng1.close()


def test_model_layer_and_transfer(built_lib, monkeypatch):
  cfg = synth.default_config(batch_size=3, use_grids=(1, 0), beam_size=5)
  params = synth.make_params(cfg, seed=synth.SEED_BASE + 4, recurrent_gain=3.0, bias_scale=0.1)
  feed = synth.make_feed(cfg, seed=synth.SEED_BASE + 32)
  model = pred_models.Model(cfg, "model")
  model.load_params(params)
  _, reg, beam = model.run_forward(feed)
  lib = model.engine.lib
  calls = []

  def spy(name):
    real = getattr(lib, name)

    def call(*a):
      calls.append(name)
      return real(*a)
    return call

  # the two entry points that copy every beam's logits to the host
  monkeypatch.setattr(model.engine, "lib", argparse.Namespace(**{
      k: getattr(lib, k) for k in built_lib.EXPORTED_SYMBOLS}))
  model.engine.lib.mv_download_beam_outputs = spy("mv_download_beam_outputs")
  model.engine.lib.mv_forward_beam = spy("mv_forward_beam")
  args = _args(cfg)
  for f in (feed, dict(feed, compact=True)):
    dec = model.run_forward_decoded(f, occupancy=True, grid_centers=args.scene_grid_centers)
    assert sorted(dec) == ["ids", "logprobs", "occupancy", "trajs"]
    assert (dec["ids"] == beam[1]).all() and (dec["logprobs"] == beam[2]).all()
    arrs = {"grid_reg": reg[0], "logits": beam[0], "ids": beam[1], "logprobs": beam[2]}
    assert (dec["trajs"] == _host_trajs(cfg, arrs, 0, feed["pred_length"], False)).all()
    assert dec["occupancy"].shape == (3, 12, 576)
  assert not calls, "the decoded path called %s" % calls
  model.run_forward(feed)                                  # the spies do see the host paths
  model.run_forward(dict(feed, compact=True))
  assert calls == ["mv_forward_beam", "mv_download_beam_outputs"]
  # a greedy model: trajectories only
  model.close()
  gcfg = synth.default_config(batch_size=2, use_grids=(0, 1))
  gm = pred_models.Model(gcfg, "model")
  gm.load_params(synth.make_params(gcfg, seed=synth.SEED_BASE + 4, recurrent_gain=3.0,
                                   bias_scale=0.1))
  gfeed = synth.make_feed(gcfg, seed=synth.SEED_BASE + 33)
  cls, greg, _ = gm.run_forward(gfeed)
  gargs = _args(gcfg, greedy=True, num_out=1)
  dec = gm.run_forward_decoded(gfeed, grid_centers=gargs.scene_grid_centers)
  assert sorted(dec) == ["trajs"]
  want = np.asarray([mf.decode_trajectories(gargs, cls[1][n], greg[1][n], None, 12, 1)
                     for n in range(2)])
  assert (dec["trajs"] == want).all()
  with pytest.raises(built_lib.MvError, match="greedily"):
    gm.run_forward_decoded(gfeed, occupancy=True)
  gm.close()


def test_errors_name_their_cause(built_lib):
  cfg = synth.default_config(batch_size=2, use_grids=(0, 1), beam_size=4)
  params = synth.make_params(cfg, seed=synth.SEED_BASE + 4)
  feed = synth.make_feed(cfg, seed=synth.SEED_BASE + 34)
  eng = _engine(built_lib, cfg, params, "f32", centers=False)
  for call in (eng.decode_trajectories, eng.beam_occupancy, eng.beam_ids):
    with pytest.raises(built_lib.MvError, match="no (beam )?forward has run"):
      call()
  eng.forward_beam(feed)
  with pytest.raises(built_lib.MvError, match=r"mv_set_grid_centers\(1\) has not been called"):
    eng.decode_trajectories()
  assert eng.beam_occupancy().shape == (2, 12, 144)        # needs no centres
  eng.close()
  gcfg = synth.default_config(batch_size=2, use_grids=(0, 1))
  geng = _engine(built_lib, gcfg, synth.make_params(gcfg, seed=synth.SEED_BASE + 4), "f32")
  geng.forward_greedy(synth.make_feed(gcfg, seed=synth.SEED_BASE + 34))
  with pytest.raises(built_lib.MvError, match="beam_size 1"):
    geng.beam_occupancy()
  with pytest.raises(built_lib.MvError, match="scale 0 is not an enabled scale"):
    geng.decode_trajectories(scale=0)
  geng.close()
  g, scfg, sparams, sfeed = sg.single_decoder_beam_case()
  seng = _engine(built_lib, scfg, sparams, "f32")
  seng.forward_beam(sfeed)
  for call in (seng.decode_trajectories, seng.beam_occupancy):
    with pytest.raises(built_lib.MvError, match="use_single_decoder with beam search"):
      call()
  seng.close()


def test_multifuture_cli_device_decode(built_lib, tmp_path, capsys):
  ds = mf_fixture.make_dataset(str(tmp_path / "fp"), n_traj=4)
  cfg = synth.default_config(batch_size=1, use_grids=(0, 1), beam_size=5)
  params = synth.make_params(cfg, seed=synth.SEED_BASE + 31, recurrent_gain=3.0,
                             bias_scale=0.1)
  model_dir = str(tmp_path / "model")
  tf_checkpoint.save_checkpoint(os.path.join(model_dir, "save-best"), params, global_step=100)
  out_file, prob_file = str(tmp_path / "out.p"), str(tmp_path / "prob.p")
  argv = [ds["traj_path"], ds["multifuture_path"], model_dir, out_file,
          "--save_prob_file", prob_file, "--num_out", "5", "--emb_size", "32",
          "--use_grids", "0,1", "--use_gnn", "--use_scene_enc", "--diverse_beam",
          "--diverse_gamma", "0.01", "--fix_num_timestep", "1",
          "--scene_feat_path", ds["scene_feat_path"], "--scene_id2name", ds["scene_id2name"],
          "--obs_len", "8", "--batch_size", "3"]
  cli.multifuture_inference_main(argv)
  out2_file, occ_file, prob2_file = (str(tmp_path / n) for n in ("out2.p", "occ.p", "prob2.p"))
  argv2 = argv[:3] + [out2_file, "--save_prob_file", prob2_file] + argv[6:]
  cli.multifuture_inference_main(argv2 + ["--device_decode"])
  out = pickle.load(open(out_file, "rb"))
  out2 = pickle.load(open(out2_file, "rb"))
  assert list(out) == list(out2) and len(out) == 4
  for t in out:
    a, b = np.asarray(out[t]), np.asarray(out2[t])
    assert a.shape == b.shape and a.dtype == b.dtype == np.float64 and (a == b).all(), t
  # --save_prob_file with the device decode still writes the reference's pairs
  prob, prob2 = pickle.load(open(prob_file, "rb")), pickle.load(open(prob2_file, "rb"))
  for t in prob:
    assert (prob[t][0] == prob2[t][0]).all() and (prob[t][1] == prob2[t][1]).all()
  # --save_occupancy_file alone implies the device decode
  out3_file = str(tmp_path / "out3.p")
  cli.multifuture_inference_main(argv[:3] + [out3_file] + argv[6:] +
                                 ["--save_occupancy_file", occ_file])
  out3 = pickle.load(open(out3_file, "rb"))
  for t in out:
    assert (np.asarray(out[t]) == np.asarray(out3[t])).all()
  occ = pickle.load(open(occ_file, "rb"))
  assert list(occ) == list(out) and all(v.dtype == np.float32 and v.shape[1] == 144
                                        for v in occ.values())
  capsys.readouterr()
  lines = []
  for f in (prob_file, occ_file):
    cli.multifuture_eval_trajs_prob_main([ds["multifuture_path"], f, "--scene_h", "9",
                                          "--scene_w", "16"])
    log = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert log[1] == "NLL:"
    lines.append((log[0], log[2], [float(x) for x in log[3].split()]))
  assert lines[0][0] == lines[1][0] and lines[0][1] == lines[1][1]
  print("NLL from (logits, logprobs): %s\nNLL from the occupancy file: %s"
        % (lines[0][2], lines[1][2]))
  assert len(lines[0][2]) == 5
  assert np.abs(np.asarray(lines[0][2]) - np.asarray(lines[1][2])).max() <= 1e-5
