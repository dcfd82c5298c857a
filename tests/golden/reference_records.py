# coding=utf-8
"""Recorded results of the reference implementation's own host code (argparse tables,
evaluation scripts, input pipeline, batcher, metrics) on the deterministic inputs of the
tests that compare against it, so that those tests run from the repository alone.

A record is a nested structure of dicts, lists, tuples, numpy arrays and JSON scalars,
stored as tests/golden/reference_<name>.npz: the arrays as members a0, a1, ... and the
structure as JSON (no pickles).  `make_reference_records.py` in this folder writes them
from a reference checkout."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def path(name):
  return os.path.join(HERE, "reference_%s.npz" % name)


def _pack(obj, arrays):
  if isinstance(obj, dict):
    return {"d": [[k, _pack(v, arrays)] for k, v in obj.items()]}
  if isinstance(obj, (list, tuple)):
    return {"l": [_pack(v, arrays) for v in obj], "t": isinstance(obj, tuple)}
  if isinstance(obj, (np.ndarray, np.generic)):
    key = "a%d" % len(arrays)
    arrays[key] = np.asarray(obj)
    return {"a": key, "s": isinstance(obj, np.generic)}
  if obj is None or isinstance(obj, (bool, int, float, str)):
    return {"v": obj}
  raise TypeError("cannot record %r" % type(obj))


def _unpack(node, z):
  if "d" in node:
    return {k: _unpack(v, z) for k, v in node["d"]}
  if "l" in node:
    items = [_unpack(v, z) for v in node["l"]]
    return tuple(items) if node["t"] else items
  if "a" in node:
    a = z[node["a"]]
    return a[()] if node["s"] else a
  return node["v"]


def save(name, obj):
  arrays = {}
  tree = _pack(obj, arrays)
  np.savez_compressed(path(name), __structure__=np.array(json.dumps(tree)), **arrays)


def load(name):
  with np.load(path(name), allow_pickle=False) as z:
    return _unpack(json.loads(str(z["__structure__"])), z)
