# coding=utf-8
"""Cases of the fixtures written by tests/golden/make_noscene_golden.py (the reference's
unmodified pred_models.py on the TF-1 shim, model built without --use_scene_enc)."""
from multiverse_amd import synth

import shim_golden as sg

SEED = synth.SEED_BASE + 60

FORWARD = {   # fixture -> (config overrides, seed)
    "golden_shim_noscene_greedy_both.npz": (dict(batch_size=2, use_grids=(1, 1)), SEED),
    "golden_shim_noscene_beam_s1.npz": (dict(batch_size=2, use_grids=(0, 1), beam_size=5),
                                        SEED + 1),
    "golden_shim_noscene_beam20_s0.npz": (dict(batch_size=1, use_grids=(1, 0), beam_size=20),
                                          SEED + 2),
}
TRAIN = {
    "golden_shim_noscene_train_both.npz": (dict(batch_size=2, use_grids=(1, 1)), SEED + 3),
    "golden_shim_noscene_train_relu.npz": (dict(batch_size=2, use_grids=(0, 1),
                                                activation_func="relu"), SEED + 4),
}


def config(**kw):
  return synth.default_config(use_scene_enc=False, **kw)


def forward_case(name):
  over, seed = FORWARD[name]
  g = sg.load(name)
  cfg = config(**over)
  params = synth.make_params(cfg, seed=seed, recurrent_gain=3.0, bias_scale=0.1)
  return g, cfg, params, synth.make_feed(cfg, seed=seed)


def train_case(name):
  over, seed = TRAIN[name]
  g = sg.load(name)
  cfg = config(is_train=True, **over)
  cfg.train_num_examples = 2
  params = synth.make_params(cfg, seed=seed, recurrent_gain=2.0, bias_scale=0.1)
  feeds = [synth.make_feed(cfg, seed=seed + 100 + s) for s in range(int(g["steps"][0]))]
  return g, cfg, params, feeds
