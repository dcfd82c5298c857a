# coding=utf-8
"""GPU: what one handle keeps between forwards of different kinds (csrc/engine_state.h
ForwardKind, LengthPlan) and the finalisers that the uniform and the ragged forward share
(csrc/engine_forward.h beam_backtrace_kernel / beam_gather_kernel, csrc/multifuture_decode.h).
A uniform beam forward must not see that a ragged one ran before it, a ragged one must leave
exact -1 / 0 past a row's length, every download must accept the kinds it accepts and no other,
and a beam search must come back bit for bit after a sampled and a scoring forward, eagerly and
as a replayed graph."""
import argparse

import numpy as np
import pytest

from multiverse_amd import multifuture as mf, synth

from test_gpu_multifuture_decode import _mixture

pytestmark = pytest.mark.gpu

N, B, T = 3, 4, 3
LENS = [3, 1, 0]
FIELDS = ("ids", "logits", "logprobs", "best_beam", "grid_reg", "trajs", "occupancy")
# name -> (config overrides, used grid, compute mode): the two register forms of the occupancy
# kernel (K <= 256: one cell per thread; K <= 768: three), and the any-K form above 768 cells
# (a literal 36 x 22 grid; the stride-2 conv chain of a 72 x 44 scene map)
CASES = {
    "k576_cpt3": (dict(), (1, 0), "f16x3"),
    "k144_cpt1": (dict(), (0, 1), "f16x3"),
    "k792_anyk": (dict(scene_h=72, scene_w=44, scene_grids=[(36, 22), (18, 11)]), (1, 0), "f32"),
}


def _engine(lib, name, graph=False):
  over, grids, mode = CASES[name]
  cfg = synth.default_config(batch_size=N, use_grids=grids, beam_size=B, **over)
  cfg.max_pred_len = T
  params = synth.make_params(cfg, seed=synth.SEED_BASE + 91, recurrent_gain=3.0, bias_scale=0.1)
  feed = synth.make_feed(cfg, seed=synth.SEED_BASE + 91, pred_len=T)
  eng = lib.Engine(cfg, device=0)
  eng.set_params(params)
  eng.set_compute_mode(mode)
  eng.set_graph_mode(graph)
  eng.set_grid_centers(mf.add_grid(argparse.Namespace(
      grid_strides="2,4", use_grids=[bool(u) for u in cfg.use_grids], scene_h=cfg.scene_h,
      scene_w=cfg.scene_w, video_h=1080, video_w=1920)).scene_grid_centers)
  return eng, feed


def _beam(eng, feed):
  arrs = dict(eng.forward_beam(feed)[0])
  arrs["trajs"] = eng.decode_trajectories()
  arrs["occupancy"] = eng.beam_occupancy()
  return arrs


def _assert_same(a, b, what):
  for k in FIELDS:
    assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, k)


def _assert_ragged(rag, uni, what):
  """Rows of length T are the uniform rows; past a row's length: ids -1, logits, occupancy and
  offsets 0, trajectories (0, 0)."""
  for n, L in enumerate(LENS):
    if L == T:
      for k in FIELDS:
        assert rag[k][n].tobytes() == uni[k][n].tobytes(), (what, n, k)
    assert (rag["ids"][n, :, L:] == -1).all(), (what, n)
    assert (rag["logits"][n, :, L:] == 0).all(), (what, n)
    assert (rag["trajs"][n, :, L:] == 0).all(), (what, n)
    for k in ("occupancy", "best_beam", "grid_reg"):
      assert (rag[k][n, L:] == 0).all(), (what, n, k)
    if L == 0:
      assert (rag["logprobs"][n] == 0).all(), (what, n)


@pytest.mark.parametrize("name", ["k576_cpt3", "k144_cpt1"])
def test_uniform_ragged_uniform_on_one_handle(built_lib, name):
  eng, feed = _engine(built_lib, name)
  first = _beam(eng, feed)
  rag = _beam(eng, dict(feed, pred_lengths=LENS))
  third = _beam(eng, feed)                        # the feed clears the lengths
  eng.close()
  assert (first["ids"] >= 0).all()
  _assert_same(first, third, name)
  _assert_ragged(rag, first, name)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_beam_sampled_scored_beam_on_one_handle(built_lib, graph):
  lib = built_lib
  eng, feed = _engine(lib, "k144_cpt1", graph)
  not_scored = "was not a scoring one"
  with pytest.raises(lib.MvError, match="no beam forward has run"):
    eng.beam_ids()
  first = _beam(eng, feed)
  with pytest.raises(lib.MvError, match=not_scored):
    eng.scores()
  eng.set_sampling(0.8, 1234)
  sampled = dict(eng.forward_beam(feed)[0])
  assert sampled["ids"].tobytes() != first["ids"].tobytes()
  occ = eng.beam_occupancy()                      # draws: uniform weights
  assert np.abs(occ.astype(np.float64).sum(-1) - 1).max() <= 1e-6
  ids, lp = eng.beam_ids()
  assert (ids == sampled["ids"]).all() and (lp == sampled["logprobs"]).all()
  with pytest.raises(lib.MvError, match=not_scored):
    eng.scores()
  eng.clear_sampling()
  scored = eng.score_futures(feed, sampled["ids"])
  assert scored["logprobs"].tobytes() == sampled["logprobs"].tobytes()
  assert eng.scores()["step_logprobs"].tobytes() == scored["step_logprobs"].tobytes()
  with pytest.raises(lib.MvError, match="scored given futures"):
    eng.beam_occupancy()
  assert (eng.beam_ids()[0] == sampled["ids"]).all()
  assert eng.decode_trajectories().shape == (N, B, T, 2)
  last = _beam(eng, feed)
  with pytest.raises(lib.MvError, match=not_scored):
    eng.scores()
  eng.close()
  _assert_same(first, last, "graph" if graph else "eager")


def test_any_k_occupancy_uniform_and_ragged(built_lib):
  """A grid above 768 cells takes the any-K form of the occupancy kernel: against the fp64
  mixture at the bar of test_occupancy_kernel_arithmetic_against_fp64 (4 x the distance of
  the reference's float32 arithmetic), uniform and with per-row lengths."""
  eng, feed = _engine(built_lib, "k792_anyk")
  uni = _beam(eng, feed)
  rag = _beam(eng, dict(feed, pred_lengths=LENS))
  eng.close()
  assert uni["logits"].shape[-1] == 792
  _assert_ragged(rag, uni, "k792")
  for what, arrs, lens in (("uniform", uni, [T] * N), ("ragged", rag, LENS)):
    exact = _mixture(arrs["logits"], arrs["logprobs"], np.float64)
    ref32 = _mixture(arrs["logits"], arrs["logprobs"], np.float32)
    live = np.asarray([[t < L for t in range(T)] for L in lens])
    dev = arrs["occupancy"]
    assert dev.dtype == np.float32 and dev.shape == exact.shape
    d_ref = float((np.abs(ref32 - exact) / exact)[live].max())
    d_dev = float((np.abs(dev - exact) / exact)[live].max())
    rows = float(np.abs(dev.astype(np.float64).sum(-1) - 1)[live].max())
    print("k792 %s: reference float32 vs fp64 %.3g, device vs fp64 %.3g (bar %.3g), rows sum "
          "to 1 within %.3g" % (what, d_ref, d_dev, 4 * d_ref, rows))
    assert d_dev <= 4 * d_ref
    assert rows <= 1e-6
