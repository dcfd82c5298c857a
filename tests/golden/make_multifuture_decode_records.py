# coding=utf-8
"""Write tests/golden/reference_multifuture_decode.npz: the occupancy maps the reference's
own grid-NLL script (code/multifuture_eval_trajs_prob.py: its `softmax` and `get_hw_prob`)
builds from the beam outputs already frozen in the beam fixtures of this folder, for EVERY
step t, one sample at a time as the script does -- what the device map of
csrc/multifuture_decode.h is compared with.  Each record also carries the distance of that
float32 result from an fp64 evaluation of the same formula.  Needs a checkout of the
reference; its code/ folder is taken from $MULTIVERSE_REFERENCE, as in
make_reference_records.py.

    MULTIVERSE_REFERENCE=<checkout>/code python tests/golden/make_multifuture_decode_records.py
"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, os.path.join(ROOT, "oracle", "tf1_shim")):
  if p not in sys.path:
    sys.path.insert(0, p)

import reference_records  # noqa: E402
import run_reference as rr  # noqa: E402

FIXTURES = ("golden_shim_beam20_s0.npz", "golden_shim_beam_s1.npz",
            "golden_shim_noscene_beam20_s0.npz")


def reference_module():
  sys.path.insert(0, rr.REFERENCE_CODE)
  try:
    mod = importlib.import_module("multifuture_eval_trajs_prob")
  finally:
    sys.path.remove(rr.REFERENCE_CODE)
  assert os.path.abspath(mod.__file__).startswith(os.path.abspath(rr.REFERENCE_CODE))
  return mod


def fp64_map(logits, logprobs):
  """The same formula in float64: [B, T, K], [B] -> [T, K]."""
  x = logits.astype(np.float64)
  x = np.exp(x - x.max(-1, keepdims=True))
  x = x / x.sum(-1, keepdims=True)
  w = np.exp(logprobs.astype(np.float64) - logprobs.astype(np.float64).max())
  w = w / w.sum()
  return (x * w[:, None, None]).sum(0)


def main():
  assert rr.available(), "no reference code at %s (set MULTIVERSE_REFERENCE)" % rr.REFERENCE_CODE
  ref = reference_module()
  rec = {}
  for name in FIXTURES:
    g = np.load(os.path.join(HERE, name))
    logits, logprobs = g["beam_logits"], g["beam_logprobs"]       # [N, B, T, K], [N, B]
    N, _, T, K = logits.shape
    maps = np.zeros((N, T, K), dtype=np.float32)
    rel = ab = 0.0
    for n in range(N):
      # the script's own lines on one prediction entry ([1, B, T, K], [1, B])
      probs = ref.softmax(np.squeeze(logprobs[n][None]))
      beams = ref.softmax(np.squeeze(logits[n][None]), axis=-1)
      for t in range(T):
        maps[n, t] = ref.get_hw_prob(beams, probs, t)
      exact = fp64_map(logits[n], logprobs[n])
      rel = max(rel, float((np.abs(maps[n] - exact) / exact).max()))
      ab = max(ab, float(np.abs(maps[n] - exact).max()))
    assert maps.dtype == np.float32 and np.abs(maps.sum(-1) - 1).max() < 1e-6
    print("%s: map %s, rows sum to 1 within %.2g, largest cell %.3g, float32 vs fp64: %.3g "
          "relative, %.3g absolute" % (name, maps.shape, np.abs(maps.sum(-1) - 1).max(),
                                       maps.max(), rel, ab))
    rec[name] = {"occupancy": maps, "rel_vs_fp64": rel, "abs_vs_fp64": ab}
  reference_records.save("multifuture_decode", rec)
  print("wrote %s (%d bytes)" % (reference_records.path("multifuture_decode"),
                                 os.path.getsize(reference_records.path("multifuture_decode"))))


if __name__ == "__main__":
  main()
