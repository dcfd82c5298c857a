# coding=utf-8
"""GPU: a model built WITHOUT the scene encoder (--use_scene_enc off, the reference's default
graph; mv_config.scene_conv_dim 0).  The engine against the reference's own runs on the TF-1
shim (tests/golden/golden_shim_noscene_*.npz) in the three compute modes, and at the
benchmarked sizes against the test-side oracle (tests/noscene_oracle.py)."""
import os
import pickle

import numpy as np
import pytest
import torch

from multiverse_amd import cli, synth, tf_checkpoint

import mf_fixture
import noscene_golden as ng
import noscene_oracle as nso
import shim_golden as sg
from beam_compare import compare_beams
from test_gpu_at_size import check_greedy_rows

pytestmark = pytest.mark.gpu
TOL = 1e-4
BF16_TOL = 3e-2


def _engine(lib, cfg, params, mode):
  eng = lib.Engine(cfg, device=0)
  eng.set_params(params)
  eng.set_compute_mode(mode)
  return eng


@pytest.mark.parametrize("mode", ["f32", "f16x3"])
def test_noscene_greedy_against_reference_run(built_lib, mode):
  g, cfg, params, feed = ng.forward_case("golden_shim_noscene_greedy_both.npz")
  eng = _engine(built_lib, cfg, params, mode)
  ref = sg.var_table(g)
  ref.pop("global_step")
  assert dict(eng.param_specs()) == ref        # names / shapes the reference creates
  cls, reg = eng.forward_greedy(feed)
  eng.set_graph_mode(True)                     # hipGraph replay: bit-identical
  cls2, reg2 = eng.forward_greedy(feed)
  eng.close()
  N = cfg.batch_size
  for s in range(2):
    assert (cls[s] == cls2[s]).all() and (reg[s] == reg2[s]).all()
    assert (cls[s].reshape(N, 12, -1).argmax(-1) ==
            g["cls_%d" % s].reshape(N, 12, -1).argmax(-1)).all()
    assert np.abs(cls[s] - g["cls_%d" % s]).max() < TOL
    assert np.abs(reg[s] - g["reg_%d" % s]).max() < TOL


def test_noscene_greedy_bf16_within_its_tolerance(built_lib):
  g, cfg, params, feed = ng.forward_case("golden_shim_noscene_greedy_both.npz")
  eng = _engine(built_lib, cfg, params, "bf16")
  cls, reg = eng.forward_greedy(feed)
  eng.close()
  for s in range(2):
    rc = float(np.ptp(g["cls_%d" % s])), float(np.ptp(g["reg_%d" % s]))
    assert np.abs(cls[s] - g["cls_%d" % s]).max() <= BF16_TOL * rc[0]
    assert np.abs(reg[s] - g["reg_%d" % s]).max() <= BF16_TOL * rc[1]


@pytest.mark.parametrize("mode", ["f32", "f16x3", "bf16"])
@pytest.mark.parametrize("name,scale", [("golden_shim_noscene_beam_s1.npz", 1),
                                        ("golden_shim_noscene_beam20_s0.npz", 0)])
def test_noscene_beam_against_reference_run(built_lib, name, scale, mode):
  g, cfg, params, feed = ng.forward_case(name)
  eng = _engine(built_lib, cfg, params, mode)
  arrs, s = eng.forward_beam(feed)
  eng.close()
  assert s == scale
  if mode == "bf16":        # reduced precision: a well-formed decode, not the fp32 one
    K = cfg.scene_grids[scale][0] * cfg.scene_grids[scale][1]
    assert arrs["ids"].min() >= 0 and arrs["ids"].max() < K
    assert np.isfinite(arrs["logprobs"]).all()
    return
  trace = {}
  _, _, obeam = nso.forward(params, cfg, feed, trace=trace)
  assert (obeam[1] == g["beam_ids"]).all()
  compare_beams(arrs, g["reg_%d" % scale], g["beam_logits"], g["beam_ids"],
                g["beam_logprobs"], np.stack(trace["beam_step_topvals"], axis=-1),
                trace["beam_trace"])


@pytest.mark.parametrize("mode", ["f32", "f16x3"])
@pytest.mark.parametrize("name", sorted(ng.TRAIN))
def test_noscene_train_steps_against_reference_trainer(built_lib, name, mode):
  g, cfg, params, feeds = ng.train_case(name)
  eng = _engine(built_lib, cfg, params, mode)
  eng.train_init()
  for step, feed in enumerate(feeds):
    loss, wd, pgl = eng.train_step(feed)
    ref = g["loss_%d" % step]
    assert np.allclose([loss, wd] + pgl, ref, rtol=1e-4, atol=1e-5), (loss, ref)
    for n, _ in eng.param_specs():
      e_s, e_a = sg.digest_err(eng.get_grad(n), g["grad_%d|%s" % (step, n)])
      assert e_s < 2e-3 and e_a < 2e-3, (n, e_s, e_a)
  for n, _ in eng.param_specs():
    e_s, e_a = sg.digest_err(eng.get_param(n), g["param|%s" % n])
    assert e_s < 1e-4 and e_a < 1e-5, (n, e_s, e_a)
    for i in range(2):       # Adadelta slots under the reference's names
      e_s, e_a = sg.digest_err(eng.get_opt_slot(n, i), g["slot%d|%s" % (i, n)])
      assert e_s < 1e-3 and e_a < 1e-3, (n, i, e_s, e_a)
  assert eng.global_step == int(g["global_step"][0])
  eng.close()


def _cosine(a, b):
  a, b = a.reshape(-1).astype(np.float64), b.reshape(-1).astype(np.float64)
  return float(a @ b / max(np.linalg.norm(a) * np.linalg.norm(b), 1e-300))


def test_noscene_greedy_at_size_every_row(built_lib):
  """configs[1] shapes: N = 64, both scales, f16x3 + hipGraph, every row against the oracle."""
  cfg = ng.config(batch_size=64, use_grids=(1, 1))
  params = synth.make_params(cfg, seed=synth.SEED_BASE + 2)
  feed = synth.make_feed(cfg, seed=synth.SEED_BASE + 2)
  torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
  ocls, oreg, _ = nso.forward(params, cfg, feed)
  eng = _engine(built_lib, cfg, params, "f16x3")
  eng.set_graph_mode(True)
  cls, reg = eng.forward_greedy(feed)
  cls2, reg2 = eng.forward_greedy(feed)
  eng.set_graph_mode(False)
  eng.set_compute_mode("f32")
  fcls, freg = eng.forward_greedy(feed)
  eng.close()
  for s in range(2):
    assert (cls[s] == cls2[s]).all() and (reg[s] == reg2[s]).all()
  assert check_greedy_rows(cfg, cls, reg, ocls, oreg, 12, "f16x3") <= 2
  assert check_greedy_rows(cfg, fcls, freg, ocls, oreg, 12, "f32") <= 2


def test_noscene_beam20_rows_equal_their_batch1_decode(built_lib):
  """N = 32, beam 20, scale 0, f16x3: ids of every row bitwise those of its batch-1 decode;
  a hipGraph replay is bit-identical; row 0 against the oracle."""
  N = 32
  cfg = ng.config(batch_size=N, use_grids=(1, 0), beam_size=20)
  params = synth.make_params(cfg, seed=synth.SEED_BASE + 6, recurrent_gain=3.0, bias_scale=0.1)
  feed = synth.make_feed(cfg, seed=synth.SEED_BASE + 6)
  eng = _engine(built_lib, cfg, params, "f16x3")
  arrs, _ = eng.forward_beam(feed)
  eng.set_graph_mode(True)
  arrs2, _ = eng.forward_beam(feed)
  eng.close()
  for k in arrs:
    assert (np.asarray(arrs[k]) == np.asarray(arrs2[k])).all(), k
  cfg1 = ng.config(batch_size=1, use_grids=(1, 0), beam_size=20)
  eng1 = _engine(built_lib, cfg1, params, "f16x3")
  for n in range(N):
    f1 = dict(feed)
    for key in ("grid_obs_labels", "grid_obs_regress", "grid_pred_labels", "grid_pred_regress"):
      f1[key] = [a[n:n + 1] for a in feed[key]]
    one, _ = eng1.forward_beam(f1)
    assert (one["ids"][0] == arrs["ids"][n]).all(), n
    assert (one["logits"][0] == arrs["logits"][n]).all(), n
    assert (one["logprobs"][0] == arrs["logprobs"][n]).all(), n
    if n == 0:
      trace = {}
      _, oreg, obeam = nso.forward(params, cfg1, f1, trace=trace)
      compare_beams(one, oreg[0], obeam[0], obeam[1], obeam[2],
                    np.stack(trace["beam_step_topvals"], axis=-1), trace["beam_trace"])
  eng1.close()


def test_noscene_training_step_at_size(built_lib):
  """N = 32, both scales, one f16x3 training step: losses and every gradient tensor (the
  shared person_pred/grid_emb included) against the oracle's autograd."""
  cfg = ng.config(batch_size=32, use_grids=(1, 1), is_train=True)
  params = synth.make_params(cfg, seed=synth.SEED_BASE + 3, recurrent_gain=2.0, bias_scale=0.1)
  feed = synth.make_feed(cfg, seed=synth.SEED_BASE + 3)
  torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
  oloss, owd, opgl, ograds = nso.loss_and_grads(params, cfg, feed)
  eng = _engine(built_lib, cfg, params, "f16x3")
  eng.train_init()
  loss, wd, pgl = eng.train_forward_backward(feed)
  assert np.allclose([loss, wd] + pgl, [oloss, owd] + opgl, rtol=1e-4, atol=1e-5)
  worst = 1.0
  for n, _ in eng.param_specs():
    a, b = eng.get_grad(n), ograds[n]
    cos = _cosine(a, b)
    rel = float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))
    worst = min(worst, cos)
    assert cos >= 0.999 and rel < 2e-3, (n, cos, rel)
  print("worst gradient cosine %.6f" % worst)
  assert "person_pred/grid_emb/W" in dict(eng.param_specs())
  eng.close()


def test_noscene_checkpoint_round_trip(built_lib, tmp_path):
  """TF-format checkpoint of a trained no-scene engine: save, restore into a fresh engine,
  identical weights and identical forward outputs"""
  cfg = ng.config(batch_size=2, use_grids=(0, 1), is_train=True)
  cfg.train_num_examples = 2
  params = synth.make_params(cfg, seed=synth.SEED_BASE + 4, recurrent_gain=2.0, bias_scale=0.1)
  feed = synth.make_feed(cfg, seed=synth.SEED_BASE + 4)
  eng = _engine(built_lib, cfg, params, "f32")
  eng.train_init()
  eng.train_step(feed)
  trained = {n: eng.get_param(n) for n, _ in eng.param_specs()}
  prefix = str(tmp_path / "save-1")
  tf_checkpoint.save_checkpoint(prefix, trained, global_step=1)
  names = dict((n, s) for n, s, _ in tf_checkpoint.list_variables(str(tmp_path)))
  assert names["person_pred/grid_emb/W"] == (3, 3, 1, 32)
  assert not any("scene_conv" in n for n in names)
  back = tf_checkpoint.load_checkpoint(str(tmp_path))
  back.pop("global_step", None)
  assert sorted(back) == sorted(trained)
  cls1, reg1 = eng.forward_greedy(feed)
  eng.close()
  eng2 = _engine(built_lib, ng.config(batch_size=2, use_grids=(0, 1)), back, "f32")
  cls2, reg2 = eng2.forward_greedy(feed)
  eng2.close()
  assert (cls1[1] == cls2[1]).all() and (reg1[1] == reg2[1]).all()


def test_noscene_null_scene_inputs_and_refused_attack(built_lib):
  """the scene arrays may be NULL (the binding passes none); the scene attacks are refused"""
  cfg = ng.config(batch_size=2, use_grids=(0, 1), is_train=True)
  params = synth.make_params(cfg, recurrent_gain=3.0, bias_scale=0.1)
  feed = synth.make_feed(cfg, seed=synth.SEED_BASE + 9)
  eng = _engine(built_lib, cfg, params, "f32")
  inp = eng._inputs(feed)                       # pylint: disable=protected-access
  assert not inp.obs_scene and not inp.scene_feat
  eng.train_init()
  eng.upload(feed)
  eng.upload_targets(feed)
  eng.train_forward_backward()
  with pytest.raises(built_lib.MvError, match="no scene encoder"):
    eng.attack_begin()
  rc = eng.lib.mv_set_scene_feat(eng.handle, None)
  assert rc != 0 and b"no scene encoder" in eng.lib.mv_last_error(eng.handle)
  cls, _ = eng.forward_greedy({k: v for k, v in feed.items()
                               if k not in ("scene_feat", "obs_scene")})
  assert np.isfinite(cls[1]).all()
  eng.close()


def test_noscene_train_test_multifuture_cli(built_lib, tmp_path, capsys):
  """train.py / test.py / multifuture_inference.py without --use_scene_enc on the engine"""
  from test_gpu_cli import MODEL_FLAGS, _write_npz
  flags = [f for f in MODEL_FLAGS if f != "--use_scene_enc"]
  cfg = ng.config(batch_size=4, use_grids=(0, 1))
  prepro, out = str(tmp_path / "prepro"), str(tmp_path / "out")
  _write_npz(prepro, cfg)
  cli.train_main([prepro, out, "mv", "--train_w_onehot", "--num_epochs", "1",
                  "--save_period", "2"] + flags)
  save_dir = os.path.join(out, "mv", "00", "save")
  names = dict((n, s) for n, s, _ in tf_checkpoint.list_variables(save_dir))
  assert names["person_pred/grid_emb/W"] == (3, 3, 1, 32)
  assert names["person_pred/grid_emb/W/Adadelta"] == (3, 3, 1, 32)
  assert not any("scene_conv" in n for n in names)
  perf = cli.test_main([prepro, out, "mv"] + flags)
  assert 0 <= perf["grid1_acc"] <= 1 and perf["grid1_traj_ade"] > 0
  capsys.readouterr()
  ds = mf_fixture.make_dataset(str(tmp_path / "fp"), n_traj=2)
  bcfg = ng.config(batch_size=1, use_grids=(0, 1), beam_size=5)
  params = synth.make_params(bcfg, seed=synth.SEED_BASE + 31, recurrent_gain=3.0,
                             bias_scale=0.1)
  model_dir = str(tmp_path / "model")
  tf_checkpoint.save_checkpoint(os.path.join(model_dir, "save-best"), params, global_step=1)
  out_file = str(tmp_path / "out.p")
  cli.multifuture_inference_main(
      [ds["traj_path"], ds["multifuture_path"], model_dir, out_file, "--num_out", "5",
       "--emb_size", "32", "--use_grids", "0,1", "--use_gnn", "--diverse_beam",
       "--diverse_gamma", "0.01", "--fix_num_timestep", "1",
       "--scene_feat_path", ds["scene_feat_path"], "--scene_id2name", ds["scene_id2name"],
       "--obs_len", "8"])
  res = pickle.load(open(out_file, "rb"))
  assert len(res) == 2
