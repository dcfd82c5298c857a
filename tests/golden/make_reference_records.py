# coding=utf-8
"""Write tests/golden/reference_*.npz: the reference implementation's own results on the
inputs of the tests that compare against it (reference_records.py).  Needs a checkout of
the reference; its code/ folder is taken from $MULTIVERSE_REFERENCE, as in
oracle/tf1_shim/run_reference.py.

    MULTIVERSE_REFERENCE=<checkout>/code python tests/golden/make_reference_records.py
"""
import os
import pathlib
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (ROOT, TESTS, HERE, os.path.join(ROOT, "oracle", "tf1_shim")):
  if p not in sys.path:
    sys.path.insert(0, p)

import reference_records  # noqa: E402
import run_reference as rr  # noqa: E402


def main():
  assert rr.available(), "no reference code at %s (set MULTIVERSE_REFERENCE)" % rr.REFERENCE_CODE
  import test_cli_flags
  import test_eval_scripts_vs_reference
  import test_multifuture_inputs_vs_reference
  import test_pred_utils_vs_reference
  with tempfile.TemporaryDirectory() as tmp:
    recs = {
        "cli_flags": test_cli_flags.record(rr.REFERENCE_CODE),
        "eval_scripts": test_eval_scripts_vs_reference.record(
            rr.REFERENCE_CODE, pathlib.Path(tmp) / "eval"),
        "multifuture_inputs": test_multifuture_inputs_vs_reference.record(
            os.path.join(tmp, "mf")),
        "pred_utils": test_pred_utils_vs_reference.record(os.path.join(tmp, "pu")),
    }
  for name, rec in recs.items():
    reference_records.save(name, rec)
    print("wrote %s (%d bytes)" % (reference_records.path(name),
                                   os.path.getsize(reference_records.path(name))))


if __name__ == "__main__":
  main()
