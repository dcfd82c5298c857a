# coding=utf-8
"""GPU: the drop-in multifuture_inference.py under --max_step_cells / --accel_cost (the motion
costs, mv_set_motion_cost; tests/test_gpu_motion_cost.py has the engine's side): the written
futures respect the limit in grid cells, alone and with --class_costs, what the script writes is
what `multifuture.run_inference` gives a model fed the same tables, and the flags' refusals end
the script before it loads anything."""
import os
import pickle
from glob import glob

import numpy as np
import pytest

from multiverse_amd import cli, multifuture as mf, pred_models, pred_utils, synth, tf_checkpoint

import mf_fixture

pytestmark = pytest.mark.gpu

MOTION = ["--max_step_cells", "1", "--accel_cost", "0.5"]


def _cells(args, futures):
  """The grid cells of written futures (--center_only: every point is a cell centre)."""
  centers = args.scene_grid_centers[1].reshape(-1, 2)
  pts = np.asarray(futures)
  flat = pts.reshape(-1, 2)
  cells = np.argmin(((flat[:, None, :] - centers[None]) ** 2).sum(-1), axis=1)
  assert (np.abs(centers[cells] - flat) == 0).all()
  return cells.reshape(pts.shape[:-1])


def test_script_futures_respect_the_limit(built_lib, tmp_path):
  ds = mf_fixture.make_dataset(str(tmp_path / "fp"), n_traj=4)
  cfg = synth.default_config(batch_size=1, use_grids=(0, 1), beam_size=3)
  params = synth.make_params(cfg, seed=synth.SEED_BASE + 31, recurrent_gain=3.0,
                             bias_scale=0.1)
  model_dir = str(tmp_path / "model")
  tf_checkpoint.save_checkpoint(os.path.join(model_dir, "save-best"), params, global_step=100)
  files = [str(tmp_path / n) for n in ("moved.p", "plain.p", "both.p")]
  tail = ["--num_out", "3", "--emb_size", "32", "--use_grids", "0,1", "--use_gnn",
          "--use_scene_enc", "--scene_feat_path", ds["scene_feat_path"],
          "--scene_id2name", ds["scene_id2name"], "--obs_length", "8", "--batch_size", "2",
          "--center_only", "--sample", "--sample_temperature", "0.9", "--sample_seed", "5"]
  head = [ds["traj_path"], ds["multifuture_path"], model_dir]
  cli.multifuture_inference_main(head + [files[0]] + tail + MOTION)
  cli.multifuture_inference_main(head + [files[1]] + tail)
  cli.multifuture_inference_main(head + [files[2]] + tail + MOTION + ["--class_costs",
                                                                      "1:-3.0,2:1.5,3:0.5"])
  moved, plain, both = (pickle.load(open(f, "rb")) for f in files)
  assert list(moved) == list(plain) == list(both) and len(moved) == 4
  p = cli.multifuture_inference_parser().parse_args(head + ["x.p"] + tail + MOTION)
  cli.parse_allowed_classes(p)
  cli.parse_class_costs(p)
  cli.parse_motion_cost(p)
  assert p.motion_cost["radius"] == 2 and p.motion_cost["acc"] is not None
  args = mf.add_grid(p)
  traj_files = glob(os.path.join(ds["traj_path"], "*.txt"))
  ids = [os.path.splitext(os.path.basename(f))[0] for f in traj_files]
  inputs = mf.get_inputs(args, traj_files, mf.load_gt(ds["multifuture_path"], ids))
  W = args.scene_grids[1][1]
  longest = {"moved": 0, "plain": 0, "both": 0}
  for i, t in enumerate(ids):
    last = int(np.asarray(inputs["obs_grid_class"][i])[1][-1])     # the last observed cell
    for name, res in (("moved", moved), ("plain", plain), ("both", both)):
      cells = _cells(args, res[t])                                  # [num_out, T]
      prev = np.concatenate([np.full((cells.shape[0], 1), last), cells[:, :-1]], axis=1)
      step = np.maximum(np.abs(cells // W - prev // W), np.abs(cells % W - prev % W))
      longest[name] = max(longest[name], int(step.max()))
  assert longest["moved"] <= 1 and longest["both"] <= 1, longest
  assert longest["plain"] > 1, longest                     # ... which the plain draw does not
  assert any((np.asarray(both[t]) != np.asarray(moved[t])).any() for t in ids)
  # the same through run_inference with a model fed the tables by inference_feed
  T_pred = max(inputs["max_pred_lengths"][i] for i in (0, 1))
  feed, _ = mf.inference_feed(inputs, args, [0, 1], batch_size=2, pred_length=T_pred)
  assert feed["motion_cost"]["vel"].shape == (2, 5, 5)
  mcfg = mf.model_config(args, batch_size=args.batch_size,
                         max_pred_len=max(inputs["max_pred_lengths"] + [12]))
  model = pred_models.Model(mcfg, mcfg.modelname, gpuid=args.gpuid)
  model.load_params(pred_utils.load_weights(model_dir, scope="person_pred"))
  want = mf.run_inference(args, model, inputs, ids)[0]
  model.close()
  for t in ids:
    assert (np.asarray(want[t]) == np.asarray(moved[t])).all(), t


def test_script_refusals(built_lib, tmp_path):
  base = [str(tmp_path / n) for n in ("traj", "mfut", "model", "out.p")]
  for extra, words in ((["--max_step_cells", "1", "--greedy"], ("--max_step_cells", "--greedy")),
                       (["--accel_cost", "1", "--score_gt", "s.p"], ("--accel_cost", "--score_gt")),
                       (["--max_step_cells", "0"], ("--max_step_cells",)),
                       (["--max_step_cells", "3"], ("--max_step_cells", "--motion_radius")),
                       (["--speed_cost=-1"], ("--speed_cost", "finite")),
                       (["--accel_cost", "nan", "--speed_cost", "1"], ("--accel_cost", "finite"))):
    with pytest.raises(SystemExit) as err:
      cli.multifuture_inference_main(base + extra)
    assert all(w in str(err.value) for w in words), extra
  assert not os.path.exists(base[3])
