# coding=utf-8
"""GPU: the drop-in multifuture_inference.py under --no_revisit / --revisit_cost (the revisit
cost, mv_set_revisit_cost; tests/test_gpu_revisit_cost.py has the engine's side): no written
future returns to a cell it left, alone and with the motion flags, what the script writes is what
`multifuture.run_inference` gives a model fed the same cost, and the flags' refusals end the
script before it loads anything."""
import os
import pickle
from glob import glob

import numpy as np
import pytest

from multiverse_amd import cli, multifuture as mf, pred_models, pred_utils, synth, tf_checkpoint

import mf_fixture
from test_gpu_motion_cost_cli import _cells

pytestmark = pytest.mark.gpu

NEVER = ["--no_revisit"]


def test_script_futures_do_not_return(built_lib, tmp_path):
  ds = mf_fixture.make_dataset(str(tmp_path / "fp"), n_traj=4)
  cfg = synth.default_config(batch_size=1, use_grids=(0, 1), beam_size=3)
  params = synth.make_params(cfg, seed=synth.SEED_BASE + 31, recurrent_gain=3.0,
                             bias_scale=0.1)
  model_dir = str(tmp_path / "model")
  tf_checkpoint.save_checkpoint(os.path.join(model_dir, "save-best"), params, global_step=100)
  files = [str(tmp_path / n) for n in ("held.p", "plain.p", "both.p")]
  tail = ["--num_out", "3", "--emb_size", "32", "--use_grids", "0,1", "--use_gnn",
          "--use_scene_enc", "--scene_feat_path", ds["scene_feat_path"],
          "--scene_id2name", ds["scene_id2name"], "--obs_length", "8", "--batch_size", "2",
          "--center_only", "--sample", "--sample_temperature", "0.9", "--sample_seed", "5"]
  head = [ds["traj_path"], ds["multifuture_path"], model_dir]
  cli.multifuture_inference_main(head + [files[0]] + tail + NEVER)
  cli.multifuture_inference_main(head + [files[1]] + tail)
  cli.multifuture_inference_main(head + [files[2]] + tail + NEVER + ["--max_step_cells", "2"])
  held, plain, both = (pickle.load(open(f, "rb")) for f in files)
  assert list(held) == list(plain) == list(both) and len(held) == 4
  p = cli.multifuture_inference_parser().parse_args(head + ["x.p"] + tail + NEVER)
  cli.parse_allowed_classes(p)
  cli.parse_class_costs(p)
  cli.parse_motion_cost(p)
  cli.parse_revisit_cost(p)
  assert np.float32(p.revisit_cost["cost"]) == np.float32(-1e30) and p.revisit_cost["seed_observed"]
  args = mf.add_grid(p)
  traj_files = glob(os.path.join(ds["traj_path"], "*.txt"))
  ids = [os.path.splitext(os.path.basename(f))[0] for f in traj_files]
  inputs = mf.get_inputs(args, traj_files, mf.load_gt(ds["multifuture_path"], ids))
  returns = {"held": 0, "plain": 0, "both": 0}
  for i, t in enumerate(ids):
    labels = np.asarray(inputs["obs_grid_class"][i])[1][None]        # the observed cells [1, T_o]
    for name, res in (("held", held), ("plain", plain), ("both", both)):
      cells = _cells(args, res[t])[None]                              # [1, num_out, T]
      returns[name] += int((mf.path_revisit_cost(cells, labels, 1.0) != 0).sum())
  assert returns["held"] == 0 and returns["both"] == 0, returns
  assert returns["plain"] > 0, returns                     # ... which the plain draw does
  # the same through run_inference with a model fed the cost by inference_feed
  T_pred = max(inputs["max_pred_lengths"][i] for i in (0, 1))
  feed, _ = mf.inference_feed(inputs, args, [0, 1], batch_size=2, pred_length=T_pred)
  assert feed["revisit_cost"]["cost"].tolist() == [np.float32(-1e30)] * 2
  mcfg = mf.model_config(args, batch_size=args.batch_size,
                         max_pred_len=max(inputs["max_pred_lengths"] + [12]))
  model = pred_models.Model(mcfg, mcfg.modelname, gpuid=args.gpuid)
  model.load_params(pred_utils.load_weights(model_dir, scope="person_pred"))
  want = mf.run_inference(args, model, inputs, ids)[0]
  model.close()
  for t in ids:
    assert (np.asarray(want[t]) == np.asarray(held[t])).all(), t


def test_script_refusals(built_lib, tmp_path):
  base = [str(tmp_path / n) for n in ("traj", "mfut", "model", "out.p")]
  for extra, words in ((["--no_revisit", "--greedy"], ("--no_revisit", "--greedy")),
                       (["--revisit_cost", "1", "--score_gt", "s.p"],
                        ("--revisit_cost", "--score_gt")),
                       (["--revisit_cost", "1", "--no_revisit"], ("contradict",)),
                       (["--revisit_ignore_observed"], ("--revisit_ignore_observed",)),
                       (["--revisit_cost=-1"], ("--revisit_cost", "finite"))):
    with pytest.raises(SystemExit) as err:
      cli.multifuture_inference_main(base + extra)
    assert all(w in str(err.value) for w in words), extra
  assert not os.path.exists(base[3])
