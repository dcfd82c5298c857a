# coding=utf-8
"""The forwards that tests/test_gpu_enc_cone.py compares between MV_ENC_CONE=2 (the class encoder
runs on the light cone of the observed cells at any batch size) and MV_ENC_CONE=0
(the dense encoder).  The switch is read once per process, so the test runs this file once per
value:

    MV_ENC_CONE=<2|0> python tests/enc_cone_cases.py OUT.npz

and compares the two files byte for byte.  Nothing here asserts; every array a case produces goes
into OUT.npz under "<case>/<name>", kernel statistics of profiled steps as JSON under
"stats/<name>"."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from multiverse_amd import _lib, synth  # noqa: E402


def hand_paths(H, W, T):
  """The hand-made label paths of tests/test_enc_cone_model.py, cut or held to T steps."""
  def cells(yx):
    yx = (list(yx) + [yx[-1]] * T)[:T]
    return [y * W + x for y, x in yx]
  return [
      cells([(0, 0)] * 8),
      cells([(2, 5), (2, 5), (2, 6), (3, 6), (3, 7), (2, 7), (3, 8), (3, 8)]),
      cells([(H - 1, W - 1)] * 3 + [(0, 0)] * 5),
      cells([(H // 2, W // 2 - 3 + t) for t in range(8)]),
  ]


def feeds_of(cfg, n_synth=1):
  """Synthetic feeds, then the same scene with the hand-made paths as labels: feed k puts path
  (n + k) % 4 into row n."""
  N, T = cfg.batch_size, cfg.obs_len
  out = [synth.make_feed(cfg, seed=synth.SEED_BASE + 500 + k) for k in range(n_synth)]
  for k in range(4 if N < 4 else 1):
    feed = synth.make_feed(cfg, seed=synth.SEED_BASE + 600 + k)
    for s, (H, W) in enumerate(cfg.scene_grids):
      hp = hand_paths(H, W, T)
      feed["grid_obs_labels"][s] = np.asarray([hp[(n + k) % 4] for n in range(N)], np.int32)
    out.append(feed)
  return out


def put(out, case, name, pair):
  cls, reg = pair
  for s in range(len(cls)):
    if not isinstance(cls[s], np.ndarray):      # a scale the model does not use
      continue
    out["%s/%s/cls%d" % (case, name, s)] = np.ascontiguousarray(cls[s])
    out["%s/%s/reg%d" % (case, name, s)] = np.ascontiguousarray(reg[s])


def put_beam(out, case, name, res):
  arrs, _ = res
  for k, v in arrs.items():
    if isinstance(v, np.ndarray):
      out["%s/%s/%s" % (case, name, k)] = np.ascontiguousarray(v)


def engine(cfg, mode):
  eng = _lib.Engine(cfg, device=0)
  eng.set_params(synth.make_params(cfg, recurrent_gain=3.0, bias_scale=0.1))
  eng.set_compute_mode(mode)
  return eng


# name -> (default_config arguments, compute mode)
GREEDY = {
    "batch3": (dict(batch_size=3, use_grids=(1, 1)), "f16x3"),
    "batch1": (dict(batch_size=1, use_grids=(1, 1)), "f16x3"),
    "obs2": (dict(batch_size=3, use_grids=(1, 1), obs_len=2), "f16x3"),
    "no_scene_enc": (dict(batch_size=3, use_grids=(1, 1), use_scene_enc=False), "f16x3"),
    "bf16": (dict(batch_size=3, use_grids=(1, 1)), "bf16"),
}
STATS_CASES = ("batch3", "batch1", "no_scene_enc")


def main():
  out = {}
  for case, (kw, mode) in GREEDY.items():
    cfg = synth.default_config(**kw)
    eng = engine(cfg, mode)
    feeds = feeds_of(cfg)
    for k, feed in enumerate(feeds):
      eng.upload(feed)
      eng.run_resident(False)
      put(out, case, "resident%d" % k, eng.download())
    # two different feeds in flight: a slot's lists must be its own
    for k, pair in enumerate(eng.forward_greedy_pipelined(feeds)):
      put(out, case, "pipelined%d" % k, pair)
    if case in STATS_CASES:
      for k, feed in enumerate(feeds[:2]):
        eng.upload(feed)
        eng.set_profiling(True)
        eng.reset_kernel_stats()
        eng.run_resident(False)
        eng.synchronize()
        st = eng.kernel_stats()
        eng.set_profiling(False)
        for v in st.values():
          del v["total_ms"]
        out["stats/%s/%d" % (case, k)] = np.frombuffer(
            json.dumps(st, sort_keys=True).encode(), dtype=np.uint8)
        for s in range(2):
          out["labels/%s/%d/%d" % (case, k, s)] = np.asarray(feed["grid_obs_labels"][s], np.int32)
    if case == "batch3":
      # ragged lengths with a row that does not decode: the encoders run on a prefix of the batch
      feed = dict(feeds[1], pred_lengths=np.asarray([12, 5, 0], np.int32))
      put(out, case, "ragged", eng.forward_greedy(feed))
      put(out, case, "after_ragged", eng.forward_greedy(feeds[1]))
    eng.close()
  # beam 3 under graph replay (a captured forward must follow the labels of a later upload), the
  # sampled forward on the same handle; one scale at a time
  for grids in ((1, 0), (0, 1)):
    case = "beam_scale%d" % grids.index(1)
    cfg = synth.default_config(batch_size=3, use_grids=grids, beam_size=3)
    eng = engine(cfg, "f16x3")
    feeds = feeds_of(cfg)
    # one profiled beam forward and one profiled sampled forward, graph mode off: their executed
    # FLOPs show whether the class encoder ran on the cone
    for name, sampling in (("beam", False), ("sampled", True)):
      if sampling:
        eng.set_sampling(temperature=1.0, seed=11)
      eng.forward_beam(feeds[1])
      eng.set_profiling(True)
      eng.reset_kernel_stats()
      eng.forward_beam(feeds[1])
      st = eng.kernel_stats()
      eng.set_profiling(False)
      if sampling:
        eng.clear_sampling()
      for v in st.values():
        del v["total_ms"]
      out["stats/%s/%s" % (case, name)] = np.frombuffer(
          json.dumps(st, sort_keys=True).encode(), dtype=np.uint8)
    out["labels/%s" % case] = np.asarray(feeds[1]["grid_obs_labels"][grids.index(1)], np.int32)
    eng.set_graph_mode(True)
    for rep in range(2):
      for k, feed in enumerate(feeds):
        put_beam(out, case, "beam%d_%d" % (rep, k), eng.forward_beam(feed))
    eng.set_sampling(temperature=1.0, seed=11)
    for k, feed in enumerate(feeds[:3]):
      put_beam(out, case, "sampled%d" % k, eng.forward_beam(feed))
    eng.close()
  np.savez(sys.argv[1], **out)
  print("[enc_cone_cases] MV_ENC_CONE=%s: %d arrays" %
        (os.environ.get("MV_ENC_CONE", "(unset)"), len(out)))


if __name__ == "__main__":
  main()
