# coding=utf-8
"""GPU: the drop-in multifuture_inference.py under --allowed_classes (the constrained decode,
mv_set_cell_mask; tests/test_gpu_cell_mask.py has the engine's side): the futures it writes never
leave the mask built from each row's last observed frame, and it prints how many rows were decoded
unconstrained."""
import os
import pickle
from glob import glob

import numpy as np
import pytest

from multiverse_amd import cli, multifuture as mf, synth, tf_checkpoint

import mf_fixture

pytestmark = pytest.mark.gpu


def test_script_futures_never_leave_the_mask(built_lib, tmp_path, capsys):
  ds = mf_fixture.make_dataset(str(tmp_path / "fp"), n_traj=4)
  cfg = synth.default_config(batch_size=1, use_grids=(0, 1), beam_size=3)
  params = synth.make_params(cfg, seed=synth.SEED_BASE + 31, recurrent_gain=3.0,
                             bias_scale=0.1)
  model_dir = str(tmp_path / "model")
  tf_checkpoint.save_checkpoint(os.path.join(model_dir, "save-best"), params, global_step=100)
  files = [str(tmp_path / n) for n in ("masked.p", "none.p", "plain.p")]
  tail = ["--num_out", "3", "--emb_size", "32", "--use_grids", "0,1", "--use_gnn",
          "--use_scene_enc", "--scene_feat_path", ds["scene_feat_path"],
          "--scene_id2name", ds["scene_id2name"], "--obs_length", "8", "--batch_size", "2",
          "--center_only", "--sample", "--sample_temperature", "0.9", "--sample_seed", "5"]
  head = [ds["traj_path"], ds["multifuture_path"], model_dir]
  script = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts",
                        "multifuture_inference.py")
  assert os.path.exists(script)            # the drop-in script calls this entry point
  cli.multifuture_inference_main(head + [files[0]] + tail +
                                 ["--allowed_classes", "1,2,3", "--allowed_min_share", "0.25"])
  out_masked = capsys.readouterr().out
  cli.multifuture_inference_main(head + [files[1]] + tail +
                                 ["--allowed_classes", "1", "--allowed_min_share", "0.5"])
  out_none = capsys.readouterr().out
  cli.multifuture_inference_main(head + [files[2]] + tail)
  out_plain = capsys.readouterr().out
  masked, none, plain = (pickle.load(open(f, "rb")) for f in files)
  assert "unconstrained: 0 of 4" in out_masked and "unconstrained: 4 of 4" in out_none
  assert "unconstrained" not in out_plain
  assert all(t in out_none for t in masked)                # the fallen-back ids are printed
  assert list(masked) == list(none) == list(plain) and len(masked) == 4
  # every future stays in its row's mask: with --center_only a point IS its cell's centre
  p = cli.multifuture_inference_parser().parse_args(head + ["x.p"] + tail)
  args = mf.add_grid(p)
  traj_files = glob(os.path.join(ds["traj_path"], "*.txt"))
  ids = [os.path.splitext(os.path.basename(f))[0] for f in traj_files]
  inputs = mf.get_inputs(args, traj_files, mf.load_gt(ds["multifuture_path"], ids))
  centers = args.scene_grid_centers[1].reshape(-1, 2)
  moved = 0
  for i, t in enumerate(ids):
    last = inputs["scene_feats"][int(inputs["obs_scene"][i][-1][0])]
    allowed = mf.cell_mask_from_scene(args, last, [1, 2, 3], 0.25).reshape(-1)
    pts = np.asarray(masked[t]).reshape(-1, 2)
    cells = np.argmin(((pts[:, None, :] - centers[None]) ** 2).sum(-1), axis=1)
    assert (np.abs(centers[cells] - pts) == 0).all() and allowed[cells].all(), t
    assert (np.asarray(none[t]) == np.asarray(plain[t])).all(), t     # all ones: the plain draw
    moved += int(not (np.asarray(masked[t]) == np.asarray(plain[t])).all())
  assert moved >= 1
