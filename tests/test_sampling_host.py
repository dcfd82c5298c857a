# coding=utf-8
"""CPU: the layers around the sampled multi-future decode (mv_set_sampling) -- the generator
restatement of tests/sampling_oracle.py against the oracle's dropout generator, the Gumbel-max
draw against the distribution it samples, the new C-ABI symbol, the errors raised before any
engine exists, and the script's flags."""
import argparse
import ctypes
import os
import re

import numpy as np
import pytest

from multiverse_amd import cli, multifuture as mf, pred_models, synth
from multiverse_amd import _lib as lib_module
from oracle import multiverse_oracle as oracle

import sampling_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hash32_is_the_dropout_generator():
  """keep(i) of oracle.dropout_keep_mask <=> top 24 bits of hash32(i, seed, stream) below
  keep_prob * 2^24, for several thresholds, seeds and streams (so the bits agree, not one
  comparison of them)."""
  n = 1 << 16
  i = np.arange(n)
  for seed, stream in ((0, 0), (99, 3), (0xFFFFFFFF, 11), (20200614, 250)):
    top = so.hash32(i, seed, stream) >> np.uint32(8)
    assert top.dtype == np.uint32 and int(top.max()) < (1 << 24)
    for keep in (0.5, 0.7, 1.0 / 3, 0.999):
      thr = int(round(keep * (1 << 24)))
      assert (oracle.dropout_keep_mask((n,), keep, seed, stream) == (top < thr)).all()
  # a dyadic ladder of thresholds (keep <=> top < threshold) rebuilds all 24 bits of a few draws
  top = so.hash32(np.arange(64), 7, 5) >> np.uint32(8)
  rebuilt = np.zeros(64, dtype=np.int64)
  for bit in range(23, -1, -1):
    trial = rebuilt + (1 << bit)
    below = np.array([oracle.dropout_keep_mask((64,), float(t) / (1 << 24), 7, 5)[j]
                      for j, t in enumerate(trial)])
    rebuilt = np.where(below, rebuilt, trial)
  assert (rebuilt == top.astype(np.int64)).all()


def test_uniform_is_strictly_inside_the_unit_interval():
  edge = np.array([0, 1, (1 << 23) - 1, 1 << 23, (1 << 23) + 1, (1 << 24) - 2, (1 << 24) - 1])
  u = so.uniform_from_bits(edge)
  assert u.dtype == np.float32 and (u > 0).all() and (u < 1).all()
  assert u[0] == np.float32(2.0 ** -25) and u[-1] == np.nextafter(np.float32(1), np.float32(0))
  assert (np.diff(u.astype(np.float64)) >= 0).all()
  # codes below 2^23 are exact
  assert (u[:3].astype(np.float64) == (edge[:3] + 0.5) * 2.0 ** -24).all()
  g = -np.log(-np.log(u))
  assert np.isfinite(g).all() and g.dtype == np.float32
  draws = so.uniform(np.arange(1 << 20), 12345, 2)
  assert (draws > 0).all() and (draws < 1).all()
  assert abs(float(draws.astype(np.float64).mean()) - 0.5) < 5 * (1 / 12.0 / (1 << 20)) ** 0.5


FREQ_SEED = 2024


@pytest.mark.parametrize("tau", [0.5, 1.0, 2.0])
def test_gumbel_max_samples_the_tempered_softmax(tau):
  """2^20 futures of one row on a fixed 16-way distribution: the count of every cell within 5
  standard deviations of Binomial(2^20, softmax(lp / tau)[k])."""
  K, S = 16, 1 << 20
  logits = np.array([0.0, 1.5, -2.0, 0.3, 2.2, -0.7, 0.9, -3.5, 1.1, 0.0, -1.2, 2.9, 0.4, -0.1,
                     1.8, -2.6], dtype=np.float32)
  lp = (logits - logits.max()).astype(np.float32)
  lp = (lp - np.log(np.exp(lp).sum(dtype=np.float32))).astype(np.float32)
  g = so.step_noise(1, S, K, FREQ_SEED, 0)[0]                    # [S, K]
  ids, _ = so.sample_ids(np.broadcast_to(lp, (S, K)), tau, g)
  counts = np.bincount(ids, minlength=K).astype(np.float64)
  p = np.exp(lp.astype(np.float64) / tau)
  p /= p.sum()
  sd = np.sqrt(S * p * (1 - p))
  z = (counts - S * p) / sd
  print("tau %g: worst |z| %.2f" % (tau, np.abs(z).max()))
  assert (np.abs(z) <= 5).all(), z


def test_noise_indexing_of_rows_and_futures():
  """The two statements of the header: row n draws as row 0 under row_seed(seed, n); future s
  draws the same noise for every beam_size > s."""
  K = 144
  g3 = so.step_noise(3, 4, K, 77, 2)
  for n in range(3):
    assert (so.step_noise(1, 4, K, so.row_seed(77, n), 2)[0] == g3[n]).all()
    assert (so.step_noise(1, 4, K, 77, 2, row_base=n)[0] == g3[n]).all()
  for S in (1, 2, 3):
    assert (so.step_noise(3, S, K, 77, 2) == g3[:, :S]).all()
  assert so.row_seed(5, 0) == 5 and so.row_seed(0xFFFFFFFF, 1) == so.ROW_SEED - 1
  assert not (so.step_noise(1, 1, K, 77, 2) == so.step_noise(1, 1, K, 78, 2)).all()
  assert not (so.step_noise(1, 1, K, 77, 2) == so.step_noise(1, 1, K, 77, 3)).all()


def test_library_exports_mv_set_sampling(built_lib):
  text = open(os.path.join(ROOT, "include", "multiverse_hip.h")).read()
  text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
  protos = dict(re.findall(r"\bint\s+(mv_\w+)\s*\(([^;{]*?)\)\s*;", text))
  raw = ctypes.CDLL(built_lib.LIB_PATH)
  lib = built_lib.load()
  assert hasattr(raw, "mv_set_sampling"), "libmultiverse_hip.so does not export mv_set_sampling"
  assert "mv_set_sampling" in built_lib.EXPORTED_SYMBOLS
  assert [" ".join(p.split()) for p in protos["mv_set_sampling"].split(",")] == \
      ["mv_handle h", "int32_t enabled", "float temperature", "uint32_t seed"]
  assert lib.mv_set_sampling.argtypes[1:] == [ctypes.c_int32, ctypes.c_float, ctypes.c_uint32]
  assert lib.mv_abi_version() == 5 == built_lib.MV_ABI_VERSION    # new symbols only
  assert lib.mv_set_sampling(None, 1, 1.0, 0) != 0                # NULL handle: an error code
  assert ctypes.sizeof(built_lib.mv_config) == 28 * 4             # the structs keep their layout
  assert hasattr(built_lib.Engine, "set_sampling") and hasattr(built_lib.Engine, "clear_sampling")


def test_model_refuses_what_cannot_be_sampled_before_creating_an_engine(monkeypatch):
  def no_engine(*a, **k):
    raise AssertionError("the configuration must be refused before an engine is created")
  monkeypatch.setattr(lib_module, "Engine", no_engine)
  greedy = synth.default_config(batch_size=2, use_grids=(0, 1), sample_futures=True)
  with pytest.raises(lib_module.MvError) as err:
    pred_models.Model(greedy, "m")
  assert "greedy" in str(err.value) and "sample_futures" in str(err.value)
  for temp in (0.0, -1.0, float("nan")):
    cfg = synth.default_config(batch_size=2, use_grids=(0, 1), beam_size=3, sample_futures=True,
                               sample_temperature=temp)
    with pytest.raises(lib_module.MvError) as err:
      pred_models.Model(cfg, "m")
    assert "sample_temperature" in str(err.value)


def test_script_flags():
  flags = {f: (t, d) for f, t, d in cli._MF_FLAGS}                # pylint: disable=protected-access
  assert flags["--sample"][0] == cli.B
  assert flags["--sample_temperature"] == (float, 1.0) and flags["--sample_seed"] == (int, 0)
  # marked as additions, like the other flags the reference's script does not have
  src = open(os.path.join(ROOT, "multiverse_amd", "cli.py")).read()
  table = src[src.index("_MF_FLAGS = ["):src.index("def multifuture_inference_parser")]
  before = table[:table.index('("--sample"')]
  assert '("--' not in before[before.rindex("# not in the reference"):]
  p = cli.multifuture_inference_parser()
  base = ["traj", "mfut", "model", "out.p"]
  a = p.parse_args(base)
  assert a.sample is False and a.sample_temperature == 1.0 and a.sample_seed == 0
  a = p.parse_args(base + ["--sample", "--sample_temperature", "0.7", "--sample_seed", "9",
                           "--batch_size", "2", "--device_decode", "--ragged_batches",
                           "--save_occupancy_file", "occ.p", "--num_out", "6",
                           "--use_grids", "0,1"])
  assert a.sample and a.sample_temperature == 0.7 and a.sample_seed == 9
  cfg = mf.model_config(mf.add_grid(a), batch_size=a.batch_size)
  assert cfg.sample_futures is True and cfg.sample_temperature == 0.7 and cfg.sample_seed == 9
  assert cfg.use_beam_search and cfg.beam_size == 6
  plain = mf.model_config(mf.add_grid(p.parse_args(base + ["--use_grids", "0,1"])))
  assert plain.sample_futures is False
  # a Namespace built before the flags existed (other callers of model_config) still works
  old = argparse.Namespace(**{k: v for k, v in vars(mf.add_grid(p.parse_args(base))).items()
                              if not k.startswith("sample")})
  assert mf.model_config(old).sample_futures is False
  with pytest.raises(SystemExit) as err:
    cli.multifuture_inference_main(base + ["--sample", "--greedy"])
  assert "--sample" in str(err.value)
