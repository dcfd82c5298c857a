# coding=utf-8
"""CPU: the TRUNCATED sampling (mv_set_sampling_truncation: top-k and nucleus limits on both
samplers) -- that the DEFINITION (include/multiverse_hip.h, restated by tests/truncation_oracle.py)
draws from the step distribution renormalised over the kept set, that it is today's definition
bit for bit with the limits off, the weights of multifuture.proposal_importance_weights, and the
layers around the engine: symbols, bindings, script flags, configuration."""
import ctypes
import os
import re

import numpy as np
import pytest

from multiverse_amd import _lib as lib_module, cli, multifuture as mf, pred_models, synth

import sampling_oracle as so
import sbs_oracle as sbs
import truncation_oracle as to

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N_DRAWS = 200000
SEEDS = (np.arange(N_DRAWS, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(12345)) \
    & np.uint64(0xFFFFFFFF)
# a fixed peaked row: K = 70 cells, logits 4 * randn (a generator seed whose head of mass 0.8 has
# 9 cells at temperature 1 and 6 at 0.7: enough degrees of freedom for the chi-square)
ROW = (4.0 * np.random.RandomState(20260432).randn(70)).astype(np.float32)
# the two-step tree of test_sbs_host.py: K = 5 cells, B = 3 slots
K, B = 5, 3
_rng = np.random.RandomState(20260318)
TREE = (1.5 * _rng.randn(K).astype(np.float32), 1.5 * _rng.randn(K, K).astype(np.float32))


def chi2_quantile_999(k):
  """The 99.9 % quantile of chi-square with k degrees of freedom (Wilson-Hilferty; within 3 % of
  the exact quantile from k = 1 on: 11.16 against 10.83)."""
  z = 3.090232306167813
  return k * (1.0 - 2.0 / (9.0 * k) + z * np.sqrt(2.0 / (9.0 * k))) ** 3


def chi_square(counts, expected, min_expected=5.0):
  """(statistic, degrees of freedom), cells with an expected count below `min_expected` pooled."""
  counts, expected = np.asarray(counts, dtype=np.float64), np.asarray(expected, dtype=np.float64)
  small = expected < min_expected
  c = np.append(counts[~small], counts[small].sum())
  e = np.append(expected[~small], expected[small].sum())
  if e[-1] == 0:
    c, e = c[:-1], e[:-1]
  return float(((c - e) ** 2 / e).sum()), len(e) - 1


def _row_draws(temperature, top_k, top_p):
  """N_DRAWS restated draws of future 0, step 0 on ROW, one per row seed -> (ids, keep)."""
  Kr = len(ROW)
  keep = to.keep_sets(ROW, temperature, top_k, top_p)[0]
  lp = sbs.log_softmax(ROW)
  ids = []
  for chunk in np.array_split(SEEDS, 8):
    g = so.gumbel(np.arange(Kr, dtype=np.uint64)[None, :], chunk[:, None], 0)
    ids.append(to.masked_ids(lp[None, :], temperature, g, keep[None, :])[0])
  return np.concatenate(ids), keep


@pytest.mark.parametrize("temperature", [1.0, 0.7])
@pytest.mark.parametrize("limits", [(5, 1.0), (0, 0.8)], ids=["top_k5", "top_p0.8"])
def test_draws_follow_the_renormalised_kept_distribution(limits, temperature):
  top_k, top_p = limits
  ids, keep = _row_draws(temperature, top_k, top_p)
  assert keep[ids].all()                                   # no draw outside the kept set
  w = ROW.astype(np.float64) / temperature
  p = np.where(keep, np.exp(w - w.max()), 0.0)
  head = p.sum() / np.exp(w - w.max()).sum()
  p /= p.sum()
  if top_k:
    assert keep.sum() == top_k
  else:                                                    # the smallest head of mass >= top_p
    order = np.argsort(-ROW)
    full = np.exp(w - w.max()) / np.exp(w - w.max()).sum()
    assert head >= top_p and head - full[order[keep.sum() - 1]] < top_p
  assert 3 <= keep.sum() < len(ROW)
  stat, dof = chi_square(np.bincount(ids, minlength=len(ROW))[keep], N_DRAWS * p[keep])
  bar = chi2_quantile_999(dof)
  print("tau %.1f top_k %d top_p %.1f: %d cells kept (mass %.3f), chi2 %.1f on %d dof "
        "(99.9 %% quantile %.1f)" % (temperature, top_k, top_p, keep.sum(), head, stat, dof, bar))
  assert dof >= 2 and stat < bar
  # and the proposal's log-probability is the log of that distribution
  q = to.proposal(ROW, temperature, keep, np.float64)
  assert np.abs(np.exp(q[keep]) - p[keep]).max() < 1e-12 and np.isneginf(q[~keep]).all()


def test_kept_set_edge_cases():
  l = np.asarray([3.0, 1.0, 3.0, 0.0, 2.0, 2.0, -1.0], dtype=np.float32)
  k = lambda *a, **kw: to.keep_sets(l, 1.0, *a, **kw)[0].tolist()
  assert k(1, 1.0) == [True, False, True, False, False, False, False]     # a tie group stays whole
  assert k(3, 1.0) == [True, False, True, False, True, True, False]       # ... and may exceed top_k
  assert k(0, 1.0) == [True] * 7                                          # off means off
  assert k(0, 1e-6) == [True, False, True, False, False, False, False]    # m(k) = 0 is always kept
  assert k(1, 1.0, floor=3) == [True, False, True, False, True, True, False]
  assert k(0, 1e-6, floor=5) == [True, True, True, False, True, True, False]
  # cells within the band of the boundary are in wide and not in tight
  l2 = np.asarray([2.0, 1.0, 1.0 - 1e-4, 0.0], dtype=np.float32)
  keep, tight, wide = to.keep_sets(l2, 1.0, 2, 1.0)
  assert keep.tolist() == [True, True, False, False]
  assert tight.tolist() == [True, False, False, False]
  assert wide.tolist() == [True, True, True, False]


@pytest.mark.parametrize("temperature", [1.0, 0.7])
def test_without_replacement_on_a_pruned_tree(temperature):
  top_k = 2                                                # prunes 3 of 5 cells below the root
  d = to.tree_draws(TREE, B, temperature, SEEDS, top_k=top_k)
  leaves, g = d["leaves"], d["gumbels"]
  p = to.tree_leaf_probs(TREE, temperature, top_k=top_k, B=B)
  assert abs(p.sum() - 1) < 1e-12 and (p > 0).sum() == B * top_k          # floor B at the root
  assert (p[leaves] > 0).all()                             # no pruned leaf is ever drawn
  assert (leaves[:, 0] != leaves[:, 1]).all() and (leaves[:, 0] != leaves[:, 2]).all() and \
      (leaves[:, 1] != leaves[:, 2]).all()
  assert (g[:, 0] == 0).all() and (np.diff(g, axis=1) <= 0).all()
  for key in ("phi", "logprobs", "gumbels"):               # no -inf, no NaN
    assert np.isfinite(d[key]).all(), key
  assert d["best_equal"]
  # slot 0 is an exact sample of the truncated (tempered) model
  stat, dof = chi_square(np.bincount(leaves[:, 0], minlength=K * K)[p > 0], N_DRAWS * p[p > 0])
  bar = chi2_quantile_999(dof)
  print("tau %.1f: slot 0 chi2 %.1f on %d dof (99.9 %% quantile %.1f)"
        % (temperature, stat, dof, bar))
  assert dof == B * top_k - 1 and stat < bar
  # phi is the leaf's log-probability under the proposal, logprobs under the untempered model
  assert np.abs(d["phi"] - np.log(p[leaves])).max() < 1e-5
  assert np.abs(d["logprobs"] - np.log(sbs.tree_leaf_probs(TREE, 1.0))[leaves]).max() < 1e-5


def test_top_k_1_still_yields_b_distinct_futures():
  d = to.tree_draws(TREE, B, 1.0, SEEDS[:20000], top_k=1)
  leaves = d["leaves"]
  p = to.tree_leaf_probs(TREE, 1.0, top_k=1, B=B)
  assert (p > 0).sum() == B                                # the floor keeps B children of the root
  assert (np.sort(leaves, axis=1) == np.nonzero(p > 0)[0][None, :]).all()
  assert np.isfinite(d["phi"]).all() and np.isfinite(d["gumbels"]).all()
  assert (d["gumbels"][:, 0] == 0).all()


@pytest.mark.parametrize("temperature", [1.0, 0.7])
def test_limits_off_is_the_untruncated_restatement_bit_for_bit(temperature):
  a = to.tree_draws(TREE, B, temperature, SEEDS[:5000])
  b = sbs.tree_draws(TREE, B, temperature, SEEDS[:5000])
  for key in ("leaves", "gumbels", "logprobs"):
    assert a[key].tobytes() == b[key].tobytes(), key
  assert a["best_equal"] == b["best_equal"]
  rng = np.random.RandomState(7)
  for R, S, Kc in ((6, 3, 70), (4, 2, 162)):
    logits = (2.0 * rng.randn(R, Kc)).astype(np.float32)
    st = to.sample_step(logits, S, 2, temperature, 77, dtype=np.float32)
    lp = sbs.log_softmax(logits)
    want, _ = so.sample_ids(lp, temperature, so.step_noise(R // S, S, Kc, 77, 2).reshape(R, Kc))
    assert st["keep"].all() and st["tight"].all() and st["wide"].all()
    assert (st["ids"] == want).all()
    q = lp if temperature == 1.0 else \
        sbs.log_softmax((logits / np.float32(temperature)).astype(np.float32))
    assert st["q"].tobytes() == q.tobytes()                # q~ == lp at tau 1, == q otherwise
    assert st["lp_id"].tobytes() == lp[np.arange(R), want].tobytes()


def test_proposal_importance_weights():
  """Independent draws on the tree from a tempered, truncated proposal: the self-normalised
  estimate of a fixed f recovers its expectation under the MODEL restricted to the proposal's
  support, within four (delta-method) standard errors."""
  temperature, top_k = 0.7, 3
  keep0 = to.keep_sets(TREE[0], temperature, top_k, 1.0)[0]
  keepk = to.keep_sets(TREE[1], temperature, top_k, 1.0)[0]
  lp0, lpk = sbs.log_softmax(TREE[0]), sbs.log_softmax(TREE[1])
  q0 = to.proposal(TREE[0], temperature, keep0, np.float64)
  qk = to.proposal(TREE[1], temperature, keepk, np.float64)
  cells = np.arange(K, dtype=np.uint64)[None, :]
  first, _ = to.masked_ids(lp0[None, :], temperature, so.gumbel(cells, SEEDS[:, None], 0),
                           keep0[None, :])
  second, _ = to.masked_ids(lpk[first], temperature, so.gumbel(cells, SEEDS[:, None], 1),
                            keepk[first])
  leaves = first * K + second
  logprobs = lp0[first].astype(np.float64) + lpk[first, second]
  proposal = q0[first] + qk[first, second]
  assert np.isfinite(proposal).all()
  w = mf.proposal_importance_weights(logprobs[None, :], proposal[None, :])
  assert w.shape == (1, N_DRAWS) and w.dtype == np.float64 and abs(w.sum() - 1) < 1e-9
  f = np.cos(np.arange(K * K) * 0.7) + 0.1 * np.arange(K * K)
  est = float((w[0] * f[leaves]).sum())
  se = float(np.sqrt((w[0] ** 2 * (f[leaves] - est) ** 2).sum()))
  p1 = sbs.tree_leaf_probs(TREE, 1.0)
  support = (keep0[:, None] & keepk).reshape(-1)
  want = float((p1 * f)[support].sum() / p1[support].sum())
  model = float((p1 * f).sum())
  plain = float(f[leaves].mean())                          # unweighted: the proposal's own mean
  print("estimate %.5f +- %.5f, restricted model %.5f (whole model %.5f, unweighted %.5f)"
        % (est, se, want, model, plain))
  assert abs(est - want) < 4 * se
  assert abs(plain - want) > 4 * se                        # the weights do the work
  # equal log-probabilities: uniform weights; shapes must agree
  assert np.allclose(mf.proposal_importance_weights(np.zeros((2, 4)), np.zeros((2, 4))), 0.25)
  with pytest.raises(ValueError):
    mf.proposal_importance_weights(np.zeros((2, 3)), np.zeros((2, 4)))
  doc = mf.proposal_importance_weights.__doc__
  assert "support" in doc and "wor_importance_weights" in doc


def test_library_exports_the_new_symbols(built_lib):
  text = open(os.path.join(ROOT, "include", "multiverse_hip.h")).read()
  text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
  protos = dict(re.findall(r"\bint\s+(mv_\w+)\s*\(([^;{]*?)\)\s*;", text))
  raw = ctypes.CDLL(built_lib.LIB_PATH)
  lib = built_lib.load()
  for name in ("mv_set_sampling_truncation", "mv_download_beam_proposal_logprobs",
               "mv_op_sample_step"):
    assert hasattr(raw, name), "libmultiverse_hip.so does not export " + name
    assert name in built_lib.EXPORTED_SYMBOLS and name in protos
  norm = lambda name: [" ".join(p.split()) for p in protos[name].split(",")]
  assert norm("mv_set_sampling_truncation") == ["mv_handle h", "int32_t top_k", "float top_p"]
  assert norm("mv_download_beam_proposal_logprobs") == ["mv_handle h", "float* out"]
  assert norm("mv_op_sample_step") == [
      "int device", "const float* logits", "int32_t R", "int32_t S", "int32_t K", "int32_t t",
      "float temperature", "uint32_t seed", "int32_t top_k", "float top_p", "int32_t floor",
      "int32_t* ids", "float* lp", "float* qlp", "uint8_t* keep"]
  # mv_op_sbs_step keeps its signature
  assert norm("mv_op_sbs_step") == [
      "int device", "const float* logits", "const float* prev_phi", "const float* prev_logprob",
      "const float* prev_gumbel", "int32_t N", "int32_t B", "int32_t K", "int32_t t",
      "float temperature", "uint32_t seed", "float* new_phi", "float* new_logprob",
      "float* new_gumbel", "int32_t* ids", "int32_t* parents"]
  assert lib.mv_set_sampling_truncation.argtypes[1:] == [ctypes.c_int32, ctypes.c_float]
  assert len(lib.mv_op_sample_step.argtypes) == 15 and len(lib.mv_op_sbs_step.argtypes) == 16
  assert lib.mv_abi_version() == 5 == built_lib.MV_ABI_VERSION    # new symbols only
  assert lib.mv_set_sampling_truncation(None, 8, 0.9) != 0        # NULL handle: an error code
  assert lib.mv_download_beam_proposal_logprobs(None, None) != 0
  assert ctypes.sizeof(built_lib.mv_config) == 28 * 4             # the structs keep their layout
  assert hasattr(built_lib.Engine, "beam_proposal_logprobs")
  assert hasattr(built_lib.Engine, "set_sampling_truncation") and hasattr(built_lib, "op_sample_step")


def test_script_flags_and_model_config(monkeypatch):
  flags = {f: (t, d) for f, t, d in cli._MF_FLAGS}                # pylint: disable=protected-access
  assert flags["--sample_top_k"] == (int, 0) and flags["--sample_top_p"] == (float, 1.0)
  p = cli.multifuture_inference_parser()
  base = ["traj", "mfut", "model", "out.p"]
  off = p.parse_args(base)
  assert off.sample_top_k == 0 and off.sample_top_p == 1.0
  a = p.parse_args(base + ["--sample", "--sample_top_k", "8", "--sample_top_p", "0.9",
                           "--use_grids", "0,1"])
  cfg = mf.model_config(mf.add_grid(a))
  assert cfg.sample_futures is True and cfg.sample_top_k == 8 and cfg.sample_top_p == 0.9
  plain = mf.model_config(mf.add_grid(p.parse_args(base + ["--sample", "--use_grids", "0,1"])))
  assert plain.sample_top_k == 0 and plain.sample_top_p == 1.0
  for extra in (["--sample_top_k", "8"], ["--sample_top_p", "0.9"]):
    with pytest.raises(SystemExit) as err:
      cli.multifuture_inference_main(base + extra)
    assert "--sample" in str(err.value)

  def no_engine(*a, **k):
    raise AssertionError("the configuration must be refused before an engine is created")
  monkeypatch.setattr(lib_module, "Engine", no_engine)
  for over in (dict(sample_top_k=8), dict(sample_top_p=0.9)):
    bad = synth.default_config(batch_size=2, use_grids=(0, 1), beam_size=3, **over)
    with pytest.raises(lib_module.MvError) as err:
      pred_models.Model(bad, "m")
    assert "sample_futures" in str(err.value)
  for over, word in ((dict(sample_top_k=-1), "sample_top_k"), (dict(sample_top_p=0.0), "sample_top_p"),
                     (dict(sample_top_p=1.5), "sample_top_p")):
    bad = synth.default_config(batch_size=2, use_grids=(0, 1), beam_size=3, use_beam_search=True,
                               sample_futures=True, **over)
    with pytest.raises(lib_module.MvError) as err:
      pred_models.Model(bad, "m")
    assert word in str(err.value)
