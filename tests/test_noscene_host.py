# coding=utf-8
"""CPU: a model built without the scene encoder (--use_scene_enc off).  The test-side oracle
(tests/noscene_oracle.py) against the reference's own runs on the TF-1 shim, the parameter
table, and the binding's mapping of the flag onto the C ABI."""
import numpy as np
import pytest

from multiverse_amd import _lib, synth
from oracle import multiverse_oracle as oracle

import noscene_golden as ng
import noscene_oracle as nso
import shim_golden as sg


@pytest.mark.parametrize("name", sorted(ng.FORWARD) + sorted(ng.TRAIN))
def test_param_shapes_are_the_ones_the_reference_creates(name):
  g = sg.load(name) if name in ng.FORWARD else None
  if g is None:        # the training fixtures carry no name table: take the forward one's
    g = sg.load("golden_shim_noscene_greedy_both.npz")
  over = dict((ng.FORWARD.get(name) or ng.TRAIN[name])[0])
  ref = sg.var_table(g)
  ref.pop("global_step")
  ours = synth.param_shapes(ng.config(**over))
  if name in ng.FORWARD:
    assert ours == ref, set(ours) ^ set(ref)
  else:
    assert set(ours) <= set(ref)
  assert ours["person_pred/grid_emb/W"] == (3, 3, 1, 32)
  assert not any("scene_conv" in n for n in ours)


def test_published_draws_do_not_move():
  """the published config's weights (every existing fixture's source) are unchanged"""
  cfg = synth.default_config(batch_size=2, use_grids=(1, 1))
  assert "person_pred/scene_conv1/W" in synth.param_shapes(cfg)
  assert "person_pred/grid_emb/W" not in synth.param_shapes(cfg)
  g = sg.load("golden_shim_greedy_both.npz")
  ref = sg.var_table(g)
  ref.pop("global_step")
  assert synth.param_shapes(cfg) == ref


@pytest.mark.parametrize("name", sorted(ng.FORWARD))
def test_noscene_oracle_forward_equals_reference_run(name):
  g, cfg, params, feed = ng.forward_case(name)
  cls, reg, beam = nso.forward(params, cfg, feed)
  N = cfg.batch_size
  for s in range(2):
    if not cfg.use_grids[s]:
      continue
    assert np.abs(cls[s] - g["cls_%d" % s]).max() <= 2e-5
    assert np.abs(reg[s] - g["reg_%d" % s]).max() <= 2e-5
    assert (cls[s].reshape(N, 12, -1).argmax(-1) ==
            g["cls_%d" % s].reshape(N, 12, -1).argmax(-1)).all()
  if beam is not None:
    assert (beam[1] == g["beam_ids"]).all()
    assert np.abs(beam[0] - g["beam_logits"]).max() <= 2e-5
    assert np.abs(beam[2] - g["beam_logprobs"]).max() <= 2e-5


@pytest.mark.parametrize("name", sorted(ng.TRAIN))
def test_noscene_oracle_training_equals_reference_trainer(name):
  g, cfg, params, feeds = ng.train_case(name)
  p, st = dict(params), oracle.optimizer_init(cfg, params)
  for step, feed in enumerate(feeds):
    loss, wd, pgl, p, st, grads = nso.train_step(p, st, step, cfg, feed)
    ref = g["loss_%d" % step]
    assert np.allclose([loss, wd] + pgl, ref, rtol=2e-6, atol=1e-6), (loss, ref)
    assert sorted(grads) == sorted(k.split("|", 1)[1] for k in g.files
                                   if k.startswith("grad_%d|" % step))
    for n, gr in grads.items():
      e_s, e_a = sg.digest_err(gr, g["grad_%d|%s" % (step, n)])
      assert e_s < 2e-5 and e_a < 1e-4, (n, e_s, e_a)
  for n in p:
    e_s, e_a = sg.digest_err(p[n], g["param|%s" % n])
    assert e_s < 2e-6 and e_a < 2e-6, (n, e_s, e_a)
  assert int(g["global_step"][0]) == len(feeds)


def test_binding_maps_no_scene_encoder_to_scene_conv_dim_zero():
  cfg = ng.config(batch_size=2, use_grids=(1, 1))
  c = _lib.make_config(cfg)
  assert c.scene_conv_dim == 0
  assert _lib.make_config(synth.default_config()).scene_conv_dim == 64
