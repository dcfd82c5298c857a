# coding=utf-8
"""CPU: the sampling WITHOUT replacement (mv_set_sampling_mode 1, stochastic beam search) --
that the DEFINITION (include/multiverse_hip.h, restated by tests/sbs_oracle.py) draws ordered
B-tuples of whole sequences without replacement, the importance weights of multifuture.
wor_importance_weights, and the layers around the engine: symbols, bindings, script flag."""
import ctypes
import os
import re

import numpy as np
import pytest

from multiverse_amd import _lib as lib_module, cli, multifuture as mf, pred_models, synth

import sbs_oracle as sbs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The tree of the distribution tests: K = 5 cells, two steps, B = 3 slots; fixed logits of
# scale ~1.5 (a step distribution about as peaked as DESIGN.md 0 reports for trained weights).
K, B = 5, 3
_rng = np.random.RandomState(20260318)
TREE = (1.5 * _rng.randn(K).astype(np.float32), 1.5 * _rng.randn(K, K).astype(np.float32))
# 200 000 row seeds, fixed (the tests below were run with exactly these): with 20 000 the
# expected count of most of the 13 800 ordered triples is below 5, where chi-square does not hold
N_DRAWS = 200000
SEEDS = (np.arange(N_DRAWS, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(12345)) \
    & np.uint64(0xFFFFFFFF)


def chi2_quantile_999(k):
  """The 99.9 % quantile of chi-square with k degrees of freedom (Wilson-Hilferty; within
  0.5 % of the exact quantile for k >= 3)."""
  z = 3.090232306167813
  return k * (1.0 - 2.0 / (9.0 * k) + z * np.sqrt(2.0 / (9.0 * k))) ** 3


def plackett_luce(p, b):
  """{ordered b-tuple of distinct leaves: probability} of drawing without replacement."""
  out = {(): 1.0}
  for _ in range(b):
    nxt = {}
    for tup, pr in out.items():
      rest = 1.0 - sum(p[i] for i in tup)
      for i in range(len(p)):
        if i not in tup:
          nxt[tup + (i,)] = pr * p[i] / rest
    out = nxt
  return out


def chi_square(counts, expected, min_expected=5.0):
  """(statistic, degrees of freedom) with the cells whose expected count is below
  `min_expected` pooled into one."""
  counts, expected = np.asarray(counts, dtype=np.float64), np.asarray(expected, dtype=np.float64)
  small = expected < min_expected
  c = np.append(counts[~small], counts[small].sum())
  e = np.append(expected[~small], expected[small].sum())
  if e[-1] == 0:
    c, e = c[:-1], e[:-1]
  return float(((c - e) ** 2 / e).sum()), len(e) - 1


_draws = {}


def draws(temperature):
  if temperature not in _draws:
    _draws[temperature] = sbs.tree_draws(TREE, B, temperature, SEEDS)
  return _draws[temperature]


@pytest.mark.parametrize("temperature", [1.0, 0.7])
def test_the_definition_samples_without_replacement(temperature):
  d = draws(temperature)
  leaves = d["leaves"]
  p = sbs.tree_leaf_probs(TREE, temperature)
  assert abs(p.sum() - 1) < 1e-12
  # distinct, ordered by a non-increasing perturbed score that starts at exactly 0
  assert (leaves[:, 0] != leaves[:, 1]).all() and (leaves[:, 0] != leaves[:, 2]).all() and \
      (leaves[:, 1] != leaves[:, 2]).all()
  g = d["gumbels"]
  assert (g[:, 0] == 0).all() and (np.diff(g, axis=1) <= 0).all()
  # ordered triples against Plackett-Luce
  pl = plackett_luce(p, B)
  keys = sorted(pl)
  code = {k: i for i, k in enumerate(keys)}
  L = K * K
  flat = (leaves[:, 0].astype(np.int64) * L + leaves[:, 1]) * L + leaves[:, 2]
  lut = np.full(L ** 3, -1, dtype=np.int64)
  for k, i in code.items():
    lut[(k[0] * L + k[1]) * L + k[2]] = i
  counts = np.bincount(lut[flat], minlength=len(keys))
  stat, dof = chi_square(counts, N_DRAWS * np.asarray([pl[k] for k in keys]))
  bar = chi2_quantile_999(dof)
  print("tau %.1f: ordered triples chi2 %.1f on %d dof (99.9 %% quantile %.1f)"
        % (temperature, stat, dof, bar))
  assert dof > 500 and stat < bar
  # slot 0 is an exact sample of the (tempered) model
  stat0, dof0 = chi_square(np.bincount(leaves[:, 0], minlength=L), N_DRAWS * p)
  bar0 = chi2_quantile_999(dof0)
  print("tau %.1f: slot 0 chi2 %.1f on %d dof (99.9 %% quantile %.1f)"
        % (temperature, stat0, dof0, bar0))
  assert dof0 >= 20 and stat0 < bar0
  # the reported log-probabilities are the UNTEMPERED model's
  p1 = sbs.tree_leaf_probs(TREE, 1.0)
  assert np.abs(d["logprobs"] - np.log(p1)[leaves]).max() < 1e-5


@pytest.mark.parametrize("temperature", [1.0, 0.7])
def test_expm1_form_gives_every_parents_best_child_its_parents_score(temperature):
  assert draws(temperature)["best_equal"]


def test_chi_square_quantile():
  # exact 99.9 % quantiles (tables): 24 dof 51.179, 100 dof 149.449, 1000 dof 1143.92
  for k, want in ((24, 51.179), (100, 149.449), (1000, 1143.92)):
    assert abs(chi2_quantile_999(k) - want) / want < 5e-3


def test_importance_weights():
  """The raw estimator of a fixed f over leaves averages to sum p f within four standard errors
  of that average.  The engine's perturbed scores are conditioned on their maximum being 0, so
  the weights are those derived in multifuture.wor_importance_weights; the paper's own weight
  p / (1 - exp(-exp(logprob - kappa))) on the same draws is biased (measured here: mean 0.932
  against 1.107 at a standard error of 0.0014), which the last assertion pins."""
  d = draws(1.0)
  p = sbs.tree_leaf_probs(TREE, 1.0)
  f = np.cos(np.arange(K * K) * 0.7) + 0.1 * np.arange(K * K)        # a fixed f over leaves
  raw, norm = mf.wor_importance_weights(d["logprobs"], d["gumbels"])
  assert raw.shape == norm.shape == (N_DRAWS, B - 1)
  assert np.abs(norm.sum(-1) - 1).max() < 1e-12 and (raw > 0).all()
  fl = f[d["leaves"][:, :B - 1]]
  est = (raw * fl).sum(-1)
  mean, se = est.mean(), est.std(ddof=1) / np.sqrt(N_DRAWS)
  want = float((p * f).sum())
  print("raw estimator: mean %.5f, exact %.5f, standard error %.5f" % (mean, want, se))
  assert abs(mean - want) < 4 * se
  # E[sum of the raw weights] = 1 as well (f = 1)
  tot = raw.sum(-1)
  assert abs(tot.mean() - 1) < 4 * tot.std(ddof=1) / np.sqrt(N_DRAWS)
  with pytest.raises(ValueError):
    mf.wor_importance_weights(np.zeros((2, 3)), np.zeros((2, 4)))
  with pytest.raises(ValueError):
    mf.wor_importance_weights(np.zeros((2, 2)), np.zeros((2, 2)))
  # the paper's weight with kappa = the last slot's conditioned score: off by many standard errors
  lp = d["logprobs"][:, :B - 1].astype(np.float64)
  paper = np.exp(lp) / -np.expm1(-np.exp(lp - d["gumbels"][:, -1:].astype(np.float64)))
  pe = (paper * fl).sum(-1)
  pse = pe.std(ddof=1) / np.sqrt(N_DRAWS)
  print("paper's weight on conditioned scores: mean %.5f, standard error %.5f" % (pe.mean(), pse))
  assert abs(pe.mean() - want) > 20 * pse


def test_step_restatement_invariants():
  """The step of the oracle itself, float32 and float64: distinct (parent, id) pairs, the first
  slot keeps the largest parent score bit for bit, the scores do not increase."""
  rng = np.random.RandomState(5)
  for (N, Bs, Ks), t, temp in (((3, 3, 70), 2, 1.0), ((2, 4, 144), 2, 0.7), ((2, 3, 162), 0, 0.7)):
    logits = (2.0 * rng.randn(N, Bs, Ks)).astype(np.float32)
    prev_g = -np.sort(rng.rand(N, Bs).astype(np.float32), axis=1)
    prev_phi = -rng.rand(N, Bs).astype(np.float32) * 5
    for dtype in (np.float32, np.float64):
      st = sbs.step(logits, prev_phi, prev_phi, prev_g, t, temp, 77, dtype=dtype)
      want0 = prev_g[:, 0] if t == 0 else prev_g.max(axis=1)
      assert (st["new_g"][:, 0] == want0.astype(dtype)).all()
      assert (np.diff(st["new_g"], axis=1) <= 0).all()
      pairs = st["parents"].astype(np.int64) * Ks + st["ids"]
      assert all(len(set(row)) == Bs for row in pairs.tolist())


def test_library_exports_the_new_symbols(built_lib):
  text = open(os.path.join(ROOT, "include", "multiverse_hip.h")).read()
  text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
  protos = dict(re.findall(r"\bint\s+(mv_\w+)\s*\(([^;{]*?)\)\s*;", text))
  raw = ctypes.CDLL(built_lib.LIB_PATH)
  lib = built_lib.load()
  for name in ("mv_set_sampling_mode", "mv_download_beam_gumbels", "mv_op_sbs_step"):
    assert hasattr(raw, name), "libmultiverse_hip.so does not export " + name
    assert name in built_lib.EXPORTED_SYMBOLS and name in protos
  norm = lambda name: [" ".join(p.split()) for p in protos[name].split(",")]
  assert norm("mv_set_sampling_mode") == ["mv_handle h", "int32_t mode"]
  assert norm("mv_download_beam_gumbels") == ["mv_handle h", "float* out"]
  assert norm("mv_op_sbs_step") == [
      "int device", "const float* logits", "const float* prev_phi", "const float* prev_logprob",
      "const float* prev_gumbel", "int32_t N", "int32_t B", "int32_t K", "int32_t t",
      "float temperature", "uint32_t seed", "float* new_phi", "float* new_logprob",
      "float* new_gumbel", "int32_t* ids", "int32_t* parents"]
  assert lib.mv_set_sampling_mode.argtypes[1:] == [ctypes.c_int32]
  assert len(lib.mv_op_sbs_step.argtypes) == 16
  assert lib.mv_abi_version() == 5 == built_lib.MV_ABI_VERSION    # new symbols only
  assert lib.mv_set_sampling_mode(None, 1) != 0                   # NULL handle: an error code
  assert lib.mv_download_beam_gumbels(None, None) != 0
  assert ctypes.sizeof(built_lib.mv_config) == 28 * 4             # the structs keep their layout
  assert hasattr(built_lib.Engine, "beam_gumbels") and hasattr(built_lib, "op_sbs_step")


def test_script_flag_and_model_config(monkeypatch):
  flags = {f: (t, d) for f, t, d in cli._MF_FLAGS}                # pylint: disable=protected-access
  assert flags["--sample_without_replacement"][0] == cli.B
  p = cli.multifuture_inference_parser()
  base = ["traj", "mfut", "model", "out.p"]
  assert p.parse_args(base).sample_without_replacement is False
  a = p.parse_args(base + ["--sample", "--sample_without_replacement", "--use_grids", "0,1"])
  cfg = mf.model_config(mf.add_grid(a))
  assert cfg.sample_futures is True and cfg.sample_without_replacement is True
  plain = mf.model_config(mf.add_grid(p.parse_args(base + ["--sample", "--use_grids", "0,1"])))
  assert plain.sample_without_replacement is False
  with pytest.raises(SystemExit) as err:
    cli.multifuture_inference_main(base + ["--sample_without_replacement"])
  assert "--sample" in str(err.value)

  def no_engine(*a, **k):
    raise AssertionError("the configuration must be refused before an engine is created")
  monkeypatch.setattr(lib_module, "Engine", no_engine)
  bad = synth.default_config(batch_size=2, use_grids=(0, 1), beam_size=3,
                             sample_without_replacement=True)
  with pytest.raises(lib_module.MvError) as err:
    pred_models.Model(bad, "m")
  assert "sample_futures" in str(err.value)
