# coding=utf-8
"""GPU: the drop-in multifuture_inference.py under --class_costs (the cell costs,
mv_set_cell_bias; tests/test_gpu_cell_bias.py has the engine's side): what it writes is what
`multifuture.run_inference` gives a model fed the same bias, a cost moves the futures, and the
flag's refusals end the script before it loads anything."""
import os
import pickle
from glob import glob

import numpy as np
import pytest

from multiverse_amd import cli, multifuture as mf, pred_models, pred_utils, synth, tf_checkpoint

import mf_fixture

pytestmark = pytest.mark.gpu

COSTS = "1:-3.0,2:1.5,3:0.5"


def test_script_output_is_run_inference_under_the_same_bias(built_lib, tmp_path):
  ds = mf_fixture.make_dataset(str(tmp_path / "fp"), n_traj=4)
  cfg = synth.default_config(batch_size=1, use_grids=(0, 1), beam_size=3)
  params = synth.make_params(cfg, seed=synth.SEED_BASE + 31, recurrent_gain=3.0,
                             bias_scale=0.1)
  model_dir = str(tmp_path / "model")
  tf_checkpoint.save_checkpoint(os.path.join(model_dir, "save-best"), params, global_step=100)
  files = [str(tmp_path / n) for n in ("biased.p", "zero.p", "plain.p", "both.p")]
  tail = ["--num_out", "3", "--emb_size", "32", "--use_grids", "0,1", "--use_gnn",
          "--use_scene_enc", "--scene_feat_path", ds["scene_feat_path"],
          "--scene_id2name", ds["scene_id2name"], "--obs_length", "8", "--batch_size", "2",
          "--center_only", "--sample", "--sample_temperature", "0.9", "--sample_seed", "5"]
  head = [ds["traj_path"], ds["multifuture_path"], model_dir]
  script = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts",
                        "multifuture_inference.py")
  assert os.path.exists(script)            # the drop-in script calls this entry point
  cli.multifuture_inference_main(head + [files[0]] + tail + ["--class_costs", COSTS])
  cli.multifuture_inference_main(head + [files[1]] + tail + ["--class_costs", "1:0.0"])
  cli.multifuture_inference_main(head + [files[2]] + tail)
  cli.multifuture_inference_main(head + [files[3]] + tail + ["--class_costs", COSTS,
                                                             "--allowed_classes", "1,2,3",
                                                             "--allowed_min_share", "0.25"])
  biased, zero, plain, both = (pickle.load(open(f, "rb")) for f in files)
  assert list(biased) == list(zero) == list(plain) == list(both) and len(biased) == 4
  moved = 0
  for t in plain:
    assert (np.asarray(zero[t]) == np.asarray(plain[t])).all(), t      # zero cost: the plain draw
    moved += int(not (np.asarray(biased[t]) == np.asarray(plain[t])).all())
  assert moved >= 1
  # the same through run_inference with a model fed the bias by inference_feed
  p = cli.multifuture_inference_parser().parse_args(head + ["x.p"] + tail +
                                                    ["--class_costs", COSTS])
  cli.parse_allowed_classes(p)
  cli.parse_class_costs(p)
  assert p.class_costs == [(1, -3.0), (2, 1.5), (3, 0.5)]
  args = mf.add_grid(p)
  traj_files = glob(os.path.join(ds["traj_path"], "*.txt"))
  ids = [os.path.splitext(os.path.basename(f))[0] for f in traj_files]
  inputs = mf.get_inputs(args, traj_files, mf.load_gt(ds["multifuture_path"], ids))
  T_pred = max(inputs["max_pred_lengths"][i] for i in (0, 1))
  feed, _ = mf.inference_feed(inputs, args, [0, 1], batch_size=2, pred_length=T_pred)
  assert feed["cell_bias"].shape == (2, 144) and (feed["cell_bias"] != 0).any()
  mcfg = mf.model_config(args, batch_size=args.batch_size,
                         max_pred_len=max(inputs["max_pred_lengths"] + [12]))
  model = pred_models.Model(mcfg, mcfg.modelname, gpuid=args.gpuid)
  model.load_params(pred_utils.load_weights(model_dir, scope="person_pred"))
  want = mf.run_inference(args, model, inputs, ids)[0]
  model.close()
  for t in ids:
    assert (np.asarray(want[t]) == np.asarray(biased[t])).all(), t
  # with --allowed_classes as well: every future stays in its row's mask
  centers = args.scene_grid_centers[1].reshape(-1, 2)
  for i, t in enumerate(ids):
    last = inputs["scene_feats"][int(inputs["obs_scene"][i][-1][0])]
    allowed = mf.cell_mask_from_scene(args, last, [1, 2, 3], 0.25).reshape(-1)
    pts = np.asarray(both[t]).reshape(-1, 2)
    cells = np.argmin(((pts[:, None, :] - centers[None]) ** 2).sum(-1), axis=1)
    assert (np.abs(centers[cells] - pts) == 0).all() and allowed[cells].all(), t


def test_script_refusals(built_lib, tmp_path):
  base = [str(tmp_path / n) for n in ("traj", "mfut", "model", "out.p")]
  for extra, word in ((["--class_costs", "1:-2", "--greedy"], "--greedy"),
                      (["--class_costs", "1:-2", "--score_gt", "s.p"], "--score_gt"),
                      (["--class_costs", "1;2"], "id:cost"),
                      (["--class_costs", "99:1.0"], "scene_class"),
                      (["--class_costs", "1:inf"], "finite")):
    with pytest.raises(SystemExit) as err:
      cli.multifuture_inference_main(base + extra)
    assert word in str(err.value) and "--class_costs" in str(err.value), extra
  assert not os.path.exists(base[3])
