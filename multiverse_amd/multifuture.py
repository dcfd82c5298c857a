# coding=utf-8
"""Multi-future (Forking Paths) host pipeline around the beam-search decode:
the callers either side of the hot path.  numpy only.

  inputs      code/multifuture_inference.py:78-272   traj txt + scene-seg npy -> arrays
  feed        code/multifuture_inference.py:304-385  PredictionModelInference.get_feed_dict
  decode      code/multifuture_inference.py:475-523  ids + offsets -> pixel trajectories
  minADE/FDE  code/multifuture_eval_trajs.py:16-88
  grid NLL    code/multifuture_eval_trajs_prob.py:19-119

File formats (forking_paths_dataset/code/get_prepared_data_multifuture.py:192-251):
  traj_2.5fps/<scene>_<moment>_<pid>_<cam>.txt   lines "frame\\tpid\\tx\\ty"
  scene_seg/<traj_id>/<traj_id>_F_%08d.npy        int class map [36, 64]
  multifuture/<traj_id>.p                         {future_id: {"x_agent_traj": [(frame, pid, x, y)]}}
  scene_id2name json                              {"oldid2new": {...}, "id2name": {...}}

The reference runs one sample at a time (batch 1, beam 20, run-time T_pred);
`run_inference` keeps that order of results and additionally batches samples
that share T_pred when the engine was created with batch_size > 1; with
`args.ragged_batches` it batches samples of DIFFERENT T_pred (`plan_ragged_batches`:
one length per row, the engine stops launching the rows that have finished).
With `args.allow_short_obs` (not in the reference) a track may have FEWER than obs_length
observed frames: `get_inputs` keeps its own length, `inference_feed` right-aligns it and the
feed carries "obs_lengths" (the engine then encodes the row over its own frames only, as an
engine of that obs_len would; include/multiverse_hip.h mv_set_obs_lengths).
"""

from __future__ import annotations

import collections
import json
import os
import pickle

import numpy as np


def load_traj(traj_file):
  """code/multifuture_inference.py:78-85."""
  rows = []
  with open(traj_file, "r") as f:
    for line in f:
      line = line.strip()
      if line:
        rows.append(line.split("\t"))
  return np.array(rows, dtype="float32")


def add_grid(args):
  """code/multifuture_inference.py:88-113: grid sizes (Python round), cell
  centres and cell box sizes per scale."""
  args.scene_grid_strides = [int(o) for o in str(args.grid_strides).split(",")]
  assert args.scene_grid_strides
  args.num_scene_grid = len(args.scene_grid_strides)
  if isinstance(args.use_grids, str):
    args.use_grids = [bool(int(o)) for o in args.use_grids.split(",")]
  args.scene_grids = []
  for stride in args.scene_grid_strides:
    args.scene_grids.append((int(round(args.scene_h * 1.0 / stride)),
                             int(round(args.scene_w * 1.0 / stride))))
  args.scene_grid_centers = []
  args.grid_box_sizes = []
  for h, w in args.scene_grids:
    h_gap, w_gap = args.video_h * 1.0 / h, args.video_w * 1.0 / w
    args.grid_box_sizes.append((h_gap, w_gap))
    cx = np.cumsum([w_gap for _ in range(w)]) - w_gap / 2.0
    cy = np.cumsum([h_gap for _ in range(h)]) - h_gap / 2.0
    args.scene_grid_centers.append(np.stack(
        (np.tile(cx[None, :], [h, 1]), np.tile(cy[:, None], [1, w])), axis=-1))
  return args


def xy_to_grid_class(xy, h, w, video_h, video_w):
  """ceil(x / w_gap) (0 -> 1) - 1, likewise y; class = y * w + x
  (code/multifuture_inference.py:122-141, multifuture_eval_trajs_prob.py:47-66)."""
  xy = np.asarray(xy)
  xi = np.asarray(np.ceil(xy[:, 0] / (video_w * 1.0 / w)), dtype="int")
  yi = np.asarray(np.ceil(xy[:, 1] / (video_h * 1.0 / h)), dtype="int")
  xi[xi == 0] = 1
  yi[yi == 0] = 1
  return (yi - 1) * w + (xi - 1)


def get_grid_input(args, traj):
  """traj [obs_length, 2] -> (grid_class [n_scale, T] int32, targets list_s
  [T, h, w, 2] float32 = xy - centre).  code/multifuture_inference.py:115-156."""
  T = len(traj)
  grid_class = np.zeros([len(args.scene_grids), T], dtype="int32")
  targets = []
  for i, (center, (h, w)) in enumerate(zip(args.scene_grid_centers, args.scene_grids)):
    grid_class[i] = xy_to_grid_class(traj, h, w, args.video_h, args.video_w)
    targets.append((traj[:, None, None, :] - center[None]).astype("float32"))
  return grid_class, targets


def load_scene_id_map(path):
  """code/multifuture_inference.py:172-184 -> (oldid2new dict incl. 0 -> 0,
  total_scene_class)."""
  with open(path, "r") as f:
    m = json.load(f)
  old2new = {int(k): v for k, v in m["oldid2new"].items()}
  assert 0 not in old2new
  old2new[0] = 0
  id2name = dict(m["id2name"])
  id2name[0] = "BG"
  assert len(old2new) == len(id2name)
  return old2new, len(old2new)


def scene_to_masks(scene_feat, old2new, total_class):
  """int class map [H, W] -> uint8 one-hot [H, W, total_class]; ids missing from
  the map go to background 0 (code/multifuture_inference.py:242-258)."""
  sf = np.asarray(scene_feat)
  lut_size = int(max(int(sf.max()) if sf.size else 0, max(old2new))) + 1
  lut = np.zeros(lut_size, dtype=np.int64)
  for k, v in old2new.items():
    lut[k] = v
  neg = sf < 0
  new = lut[np.where(neg, 0, sf).astype(np.int64)]
  new[neg] = 0
  out = np.zeros(sf.shape + (total_class,), dtype="uint8")
  hh, ww = np.meshgrid(np.arange(sf.shape[0]), np.arange(sf.shape[1]), indexing="ij")
  out[hh, ww, new] = 1
  return out


def get_inputs(args, traj_files, gt_trajs):
  """code/multifuture_inference.py:158-272.  `args.allow_short_obs`: a track of 1 ..
  obs_length observed frames is accepted, its arrays keep its own length, and the result
  carries "obs_lengths" (one per sample); without it every track has obs_length frames."""
  old2new, total_class = load_scene_id_map(args.scene_id2name)
  allow_short = bool(getattr(args, "allow_short_obs", False))
  out = {"obs_traj": [], "obs_traj_rel": [], "obs_grid_class": [], "obs_grid_target": [],
         "obs_scene": [], "max_pred_lengths": []}
  if allow_short:
    out["obs_lengths"] = []
  scene_feats = []
  for traj_file in traj_files:
    traj_id = os.path.splitext(os.path.basename(traj_file))[0]
    _, _, x_agent_pid, _ = traj_id.split("_")
    x_agent_pid = int(x_agent_pid)
    data = load_traj(traj_file)
    frame_idxs = np.unique(data[:, 0]).tolist()
    obs = data[x_agent_pid == data[:, 1], 2:]
    if allow_short:
      assert 1 <= len(obs) <= args.obs_length, (traj_id, obs.shape)
      assert len(frame_idxs) == len(obs), (traj_id, len(frame_idxs), obs.shape)
      out["obs_lengths"].append(len(obs))
    else:
      assert len(obs) == args.obs_length, (traj_id, obs.shape)
    rel = np.zeros_like(obs)
    rel[1:] = obs[1:] - obs[:-1]
    grid_class, grid_target = get_grid_input(args, obs)
    featidx = np.zeros([len(obs), 1], dtype="int32")
    for i, frame_idx in enumerate(frame_idxs):
      featidx[i, 0] = len(scene_feats)
      scene_feats.append(np.load(os.path.join(
          args.scene_feat_path, traj_id, "%s_F_%08d.npy" % (traj_id, frame_idx))))
    out["obs_traj"].append(obs)
    out["obs_traj_rel"].append(rel)
    out["obs_scene"].append(featidx)
    out["obs_grid_class"].append(grid_class)
    out["obs_grid_target"].append(grid_target)
    out["max_pred_lengths"].append(max(
        len(gt_trajs[traj_id][fid]["x_agent_traj"]) for fid in gt_trajs[traj_id]))
  feats = np.zeros([len(scene_feats), args.scene_h, args.scene_w, total_class],
                   dtype="uint8")
  for k, sf in enumerate(scene_feats):
    feats[k] = scene_to_masks(sf, old2new, total_class)
  out["scene_feats"] = feats
  return out


RaggedPlan = collections.namedtuple(
    "RaggedPlan", ["batches", "ragged_row_steps", "grouped_row_steps"])


def sum_enc_prefix_rows(obs_lengths, obs_len, live_rows=None):
  """Rows the encoders of an obs-ragged forward launch per chain: sum over the steps t of
  p_t = 1 + max{n < live_rows : Lo[n] >= obs_len - t} (0 for a step no row has reached;
  include/multiverse_hip.h mv_set_obs_lengths).  Row n is inside the prefix of step t iff some
  row n' >= n has started by then, which holds for m_n = max(Lo[n:]) steps: the sum is
  sum_n m_n -- sum(Lo) when the lengths are sorted descending.  live_rows: the rows that decode
  at all (a batch with prediction lengths: 1 + the last row whose length is not 0)."""
  lo = [int(l) for l in obs_lengths]
  if live_rows is not None:
    lo = lo[:int(live_rows)]
  assert all(1 <= l <= obs_len for l in lo), "observation lengths must be in [1, obs_len]"
  total, m = 0, 0
  for l in reversed(lo):
    m = max(m, l)
    total += m
  return total


def plan_ragged_batches(lengths, N, obs_lengths=None):
  """Batches of `N` rows over samples of different prediction lengths.  The samples are
  sorted by length descending (ties by index; with `obs_lengths`, one observation length per
  sample, ties by observation length descending first: the rows that join the encoders late
  then sit at the end of their run, and the encoders launch fewer unstarted rows) and cut into
  batches of N; the last batch is
  padded with rows of length 0; a batch's pred_length is its maximum (its first row's).
  -> RaggedPlan(batches, ragged_row_steps, grouped_row_steps): batches = [(idxs, row_lengths
  [N], pred_length)] with idxs the real samples of the batch in row order, and the decoder
  row-steps (rows x steps the decoder launches) of the two schedules: sorted rows are a tight
  prefix at every step, so the ragged one spends sum(lengths) exactly; grouping by length and
  padding every group's last batch spends sum over groups of ceil(g / N) * N * T_g."""
  lengths = [int(l) for l in lengths]
  assert N >= 1 and all(l >= 1 for l in lengths), "prediction lengths must be >= 1"
  if obs_lengths is None:
    order = sorted(range(len(lengths)), key=lambda i: (-lengths[i], i))
  else:
    obs_lengths = [int(l) for l in obs_lengths]
    assert len(obs_lengths) == len(lengths)
    order = sorted(range(len(lengths)), key=lambda i: (-lengths[i], -obs_lengths[i], i))
  batches = []
  for lo in range(0, len(order), N):
    idxs = order[lo:lo + N]
    row_lengths = [lengths[i] for i in idxs] + [0] * (N - len(idxs))
    batches.append((idxs, row_lengths, row_lengths[0]))
  groups = collections.Counter(lengths)
  grouped = sum(-(-g // N) * N * T for T, g in groups.items())
  return RaggedPlan(batches, sum(lengths), grouped)


TrainRowOrder = collections.namedtuple(
    "TrainRowOrder", ["order", "enc_rows", "dec_rows", "enc_rows_unsorted", "dec_rows_unsorted"])


def sum_dec_prefix_rows(pred_lengths):
  """Rows the decoders of a ragged step launch per chain: sum over the steps t of
  1 + max{n : L[n] > t} = sum_n max(L[n:]) -- sum(L) when the lengths are sorted descending."""
  total, m = 0, 0
  for l in reversed([int(l) for l in pred_lengths]):
    m = max(m, l)
    total += m
  return total


def order_train_rows(obs_lengths, pred_lengths, obs_len=None):
  """Row order of a mixed-length TRAINING batch (Engine.set_train_lengths; the training
  counterpart of plan_ragged_batches' ordering): prediction length descending, ties by
  observation length descending, then by index.  Padding rows (length 0) go last; the decoder
  steps of a sorted batch launch no finished row, its encoder steps an unstarted row only in
  front of a row with a longer history.  -> TrainRowOrder(order, enc_rows, dec_rows,
  enc_rows_unsorted, dec_rows_unsorted): the permutation, and the rows one chain launches over
  the encoder / decoder steps in that order and in the given one (Engine.last_train_gate_rows
  counts them once per chain and used scale, forward and dgrad)."""
  lo = [int(l) for l in obs_lengths]
  lp = [int(l) for l in pred_lengths]
  assert len(lo) == len(lp), "one observation and one prediction length per row"
  if obs_len is None:
    obs_len = max(lo)
  order = sorted(range(len(lp)), key=lambda i: (-lp[i], -lo[i], i))

  def sums(idx):
    live = 0
    for r, i in enumerate(idx):
      if lp[i] > 0:
        live = r + 1
    head = idx[:live]
    if all(lp[i] > 0 for i in head):
      enc = sum_enc_prefix_rows([lo[i] for i in head], obs_len)
    else:        # a padding row inside the prefix is launched, but extends no step's prefix
      enc, m = 0, 0
      for i in reversed(head):
        if lp[i] > 0:
          m = max(m, lo[i])
        enc += m
    return enc, sum_dec_prefix_rows([lp[i] for i in idx])

  e1, d1 = sums(order)
  e0, d0 = sums(list(range(len(lp))))
  return TrainRowOrder(order, e1, d1, e0, d0)


def cell_mask_from_scene(args, scene_onehot_last_frame, allowed_classes, min_share=0.0):
  """The cells of the used grid a future may enter, from one frame of scene semantics (not in
  the reference; include/multiverse_hip.h mv_set_cell_mask): scene_onehot_last_frame
  [scene_h, scene_w, scene_class] one-hot over the NEW class ids of the scene_id2name map ->
  bool [h, w].  Pixel row i belongs to grid row floor(i * h / H), columns likewise; a cell is
  allowed iff the count of its pixels whose class is in `allowed_classes` is at least
  max(1, ceil(min_share * pixels of the cell))."""
  h, w = args.scene_grids[list(args.use_grids).index(True)]
  sf = np.asarray(scene_onehot_last_frame)
  H, W = sf.shape[:2]
  ok = sf[..., [int(c) for c in allowed_classes]].any(axis=-1)
  rows = (np.arange(H) * h) // H
  cols = (np.arange(W) * w) // W
  cell = rows[:, None] * w + cols[None, :]
  total = np.bincount(cell.reshape(-1), minlength=h * w)
  count = np.bincount(cell.reshape(-1), weights=ok.reshape(-1), minlength=h * w)
  need = np.maximum(1, np.ceil(float(min_share) * total))
  return (count >= need).reshape(h, w)


def cell_bias_from_scene(args, scene_onehot_last_frame, class_costs):
  """The cost of entering each cell of the used grid, from one frame of scene semantics (not in
  the reference; include/multiverse_hip.h mv_set_cell_bias): scene_onehot_last_frame
  [scene_h, scene_w, scene_class] one-hot over the NEW class ids, class_costs {class id: cost in
  nats} (or a list of pairs) -> float32 [h, w],
    b[cell] = sum over c of cost[c] * share(cell, c)
  with share(cell, c) the fraction of the cell's pixels of class c, under the pixel-to-cell map
  of `cell_mask_from_scene` (pixel row i belongs to grid row floor(i * h / H), columns
  likewise).  A cell that no pixel maps to costs 0."""
  h, w = args.scene_grids[list(args.use_grids).index(True)]
  sf = np.asarray(scene_onehot_last_frame)
  H, W = sf.shape[:2]
  rows = (np.arange(H) * h) // H
  cols = (np.arange(W) * w) // W
  cell = (rows[:, None] * w + cols[None, :]).reshape(-1)
  total = np.bincount(cell, minlength=h * w).astype(np.float64)
  b = np.zeros(h * w, dtype=np.float64)
  for c, cost in (class_costs.items() if hasattr(class_costs, "items") else class_costs):
    count = np.bincount(cell, weights=(sf[..., int(c)] != 0).reshape(-1).astype(np.float64),
                        minlength=h * w)
    b += float(cost) * (count / np.maximum(total, 1.0))
  return b.reshape(h, w).astype(np.float32)


MOTION_LIMIT = np.float32(-1e30)   # the cost that stands for "never": exp of it is exactly 0


def motion_tables(radius, max_step=None, speed_cost=0.0, accel_cost=0.0):
  """The tables of a motion cost (not in the reference; include/multiverse_hip.h
  mv_set_motion_cost) for one row, as the dict that feed["motion_cost"] and
  Engine.set_motion_cost(**tables) take.  With R = radius, D = 2 R + 1 and offsets d, a in
  [-R, R]^2 (rows, columns), |.|^2 the squared Euclidean length in cells:
    vel[d] = -speed_cost * |d|^2 where max(|d.y|, |d.x|) <= max_step (everywhere inside the
             window when max_step is None), else -1e30: at most max_step cells per step
    vel_far = -1e30 when max_step is given, else -speed_cost * 2 (R + 1)^2
    acc[a] = -accel_cost * |a|^2, acc_far = -accel_cost * 2 (R + 1)^2: prefer constant velocity
  acc / acc_far are None when accel_cost is 0 (no turn term)."""
  R = int(radius)
  if not 1 <= R <= 4:
    raise ValueError("motion_tables: radius = %d not in [1, 4]" % R)
  if max_step is not None and not 1 <= int(max_step) <= R:
    raise ValueError("motion_tables: max_step = %s not in [1, radius = %d]" % (max_step, R))
  for name, c in (("speed_cost", speed_cost), ("accel_cost", accel_cost)):
    if not np.isfinite(c) or c < 0:
      raise ValueError("motion_tables: %s = %r is not a finite cost >= 0" % (name, c))
  off = np.arange(-R, R + 1)
  dy, dx = np.meshgrid(off, off, indexing="ij")
  sq = (dy * dy + dx * dx).astype(np.float32)
  far2 = np.float32(2 * (R + 1) ** 2)
  vel = (-np.float32(speed_cost) * sq).astype(np.float32)
  vel_far = -np.float32(speed_cost) * far2
  if max_step is not None:
    vel[np.maximum(np.abs(dy), np.abs(dx)) > int(max_step)] = MOTION_LIMIT
    vel_far = MOTION_LIMIT
  out = {"radius": R, "vel": vel, "vel_far": np.float32(vel_far), "acc": None, "acc_far": None}
  if accel_cost != 0:
    out["acc"] = (-np.float32(accel_cost) * sq).astype(np.float32)
    out["acc_far"] = np.float32(-np.float32(accel_cost) * far2)
  return out


def path_motion_cost(ids, labels, W, tables, obs_lengths=None):
  """The motion cost each returned path paid: ids int [N, B, T] (the engine's "ids"; -1 past a
  row's length), labels int [N, T_o] the observed cells, W the grid's columns, tables the dict of
  `motion_tables` (vel / acc [D, D] or [N, D, D], the far values scalars or [N]) ->
  float32 [N, B, T], vterm + aterm of every step as mv_set_motion_cost defines them (0 where the
  id is -1).  obs_lengths [N]: a row observed for one frame pays no turn term at step 0.  Plain
  numpy on the host: a beam score minus the sum of this over T (and minus the cell bias along the
  path) is the model's log-probability of the path."""
  ids = np.asarray(ids)
  labels = np.asarray(labels)
  N, B, T = ids.shape
  R = int(tables["radius"])
  D = 2 * R + 1
  vel = np.broadcast_to(np.asarray(tables["vel"], dtype=np.float32), (N, D, D))
  vel_far = np.broadcast_to(np.asarray(tables["vel_far"], dtype=np.float32), (N,))
  acc = acc_far = None
  if tables.get("acc") is not None:
    acc = np.broadcast_to(np.asarray(tables["acc"], dtype=np.float32), (N, D, D))
    acc_far = np.broadcast_to(np.asarray(tables["acc_far"], dtype=np.float32), (N,))
  To = labels.shape[1]
  out = np.zeros((N, B, T), dtype=np.float32)
  for n in range(N):
    lo = To if obs_lengths is None else int(obs_lengths[n])
    for b in range(B):
      p1 = int(labels[n, To - 1])
      p0 = int(labels[n, To - 2]) if lo >= 2 else -1
      for t in range(T):
        k = int(ids[n, b, t])
        if k < 0:
          break
        dy, dx = k // W - p1 // W, k % W - p1 % W
        v = vel[n, dy + R, dx + R] if max(abs(dy), abs(dx)) <= R else vel_far[n]
        a = np.float32(0.0)
        if acc is not None and p0 >= 0:
          ay, ax = dy - (p1 // W - p0 // W), dx - (p1 % W - p0 % W)
          a = acc[n, ay + R, ax + R] if max(abs(ay), abs(ax)) <= R else acc_far[n]
        out[n, b, t] = np.float32(v) + np.float32(a)
        p0, p1 = p1, k
  return out


def path_revisit_cost(ids, labels, cost, obs_lengths=None, seed_observed=True):
  """The revisit cost each returned path paid (not in the reference; include/multiverse_hip.h
  mv_set_revisit_cost): ids int [N, B, T] (the engine's "ids"; -1 past a row's length), labels int
  [N, T_o] the observed cells, cost [N] or a scalar -> float32 [N, B, T]: cost[n] where the step
  enters a cell the path held before (with seed_observed: or one of the row's observed cells,
  the last obs_lengths[n] of them) other than the cell it is in, 0 elsewhere and where the id is
  -1.  Staying is free; the path A, A, B, A pays once, at its last step.  Plain numpy on the host:
  under cost 1 the result is all zero exactly when no path returns to a cell it left."""
  ids = np.asarray(ids)
  labels = np.asarray(labels)
  N, B, T = ids.shape
  cost = np.broadcast_to(np.asarray(cost, dtype=np.float32), (N,))
  To = labels.shape[1]
  out = np.zeros((N, B, T), dtype=np.float32)
  for n in range(N):
    lo = To if obs_lengths is None else int(obs_lengths[n])
    seen0 = set(int(c) for c in labels[n, To - lo:]) if seed_observed else set()
    for b in range(B):
      seen = set(seen0)
      p1 = int(labels[n, To - 1])
      for t in range(T):
        k = int(ids[n, b, t])
        if k < 0:
          break
        if k in seen and k != p1:
          out[n, b, t] = cost[n]
        seen.add(k)
        p1 = k
  return out


def inference_feed(inputs, args, idxs, batch_size=None, lengths=None, pred_length=None):
  """Engine feed for the samples `idxs` (all with the same T_pred), padded to
  `batch_size` by repeating the last one.  For one sample this is the feed of
  PredictionModelInference.get_feed_dict (code/multifuture_inference.py:304-385):
  the scene table is compacted to the frames the batch uses, in first-use order.
  lengths (a batch of `plan_ragged_batches`): one prediction length per row, 0 for the
  padding rows; the feed then carries them as "pred_lengths" and their maximum as
  "pred_length", and the padding rows cost nothing.
  pred_length (a batch of `plan_score_batches`): the feed's "pred_length" as given, whatever
  the samples' own; the lengths then travel with the futures, not with the feed.
  Short tracks (`get_inputs` with args.allow_short_obs): a sample with fewer than obs_length
  frames is RIGHT-ALIGNED, the columns in front of it repeat its first observation (label,
  frame index, regress map: in range and finite, and ignored by the engine), and the feed
  carries "obs_lengths" [N] -- only when some row of the batch is short.
  args.allowed_classes (a list of new scene class ids; not in the reference): the feed carries
  "cell_mask" [N, K] for the used grid, row n built by `cell_mask_from_scene` from the row's
  LAST observed frame with args.allowed_min_share.  A row with fewer than num_out allowed cells
  gets the all-ones row (a beam of num_out needs that many first cells) and is listed in
  "cell_mask_fallback" (positions in `idxs`); padding rows get all ones.
  args.class_costs (a list of (new scene class id, cost in nats); not in the reference): the feed
  carries "cell_bias" float32 [N, K], row n built by `cell_bias_from_scene` from the same frame;
  padding rows get zeros.
  args.motion_cost (the dict of `motion_tables`; not in the reference): the feed carries
  "motion_cost", the same tables for every real row and zero tables for the padding rows.
  args.revisit_cost (a dict {"cost": nats <= 0, "seed_observed": bool}; not in the reference):
  the feed carries "revisit_cost" with that cost for every real row and 0 for the padding rows."""
  idxs = list(idxs)
  n_real = len(idxs)
  N = batch_size or n_real
  idxs = idxs + [idxs[-1]] * (N - n_real)
  T_in = args.obs_length
  obs_lens = [int(inputs["obs_lengths"][i]) if "obs_lengths" in inputs else T_in for i in idxs]

  def right_aligned(a, L, axis):
    """[.., L, ..] -> [.., T_in, ..]: the first observation repeated in front"""
    a = np.asarray(a)
    assert a.shape[axis] == L, (a.shape, L, axis)
    if L == T_in:
      return a
    first = np.take(a, [0], axis=axis)
    return np.concatenate([np.repeat(first, T_in - L, axis=axis), a], axis=axis)

  if lengths is not None:
    lengths = [int(l) for l in lengths]
    assert len(lengths) == N and all(l == 0 for l in lengths[n_real:])
    assert all(inputs["max_pred_lengths"][i] == l for i, l in zip(idxs[:n_real], lengths))
    T_pred = max(lengths)
  elif pred_length is not None:
    T_pred = int(pred_length)
  else:
    T_pred = inputs["max_pred_lengths"][idxs[0]]
    assert all(inputs["max_pred_lengths"][i] == T_pred for i in idxs)
  feed = {"pred_length": int(T_pred), "grid_obs_labels": [], "grid_obs_regress": []}
  if lengths is not None:
    feed["pred_lengths"] = np.asarray(lengths, dtype="int32")
  if any(L != T_in for L in obs_lens):
    feed["obs_lengths"] = np.asarray(obs_lens, dtype="int32")
  for j, (h, w) in enumerate(args.scene_grids):
    feed["grid_obs_labels"].append(np.stack(
        [right_aligned(inputs["obs_grid_class"][i][j], L, 0)
         for i, L in zip(idxs, obs_lens)]).astype("int32"))
    if not args.use_grids[j]:
      feed["grid_obs_regress"].append(None)
      continue
    feed["grid_obs_regress"].append(np.stack(
        [right_aligned(inputs["obs_grid_target"][i][j], L, 0)
         for i, L in zip(idxs, obs_lens)]).astype("float32"))
  old2new = {}
  obs_scene = np.zeros((N, T_in), dtype="int32")
  for r, (i, L) in enumerate(zip(idxs, obs_lens)):
    frames = right_aligned(inputs["obs_scene"][i], L, 0)
    for t in range(T_in):
      old = int(frames[t][0])
      if old not in old2new:
        old2new[old] = len(old2new)
      obs_scene[r, t] = old2new[old]
  scene_feat = np.zeros((len(old2new), args.scene_h, args.scene_w, args.scene_class),
                        dtype="float32")
  for old, new in old2new.items():
    scene_feat[new] = inputs["scene_feats"][old]
  feed["obs_scene"] = obs_scene
  feed["scene_feat"] = scene_feat
  allowed_classes = getattr(args, "allowed_classes", None)
  if allowed_classes:
    h, w = args.scene_grids[list(args.use_grids).index(True)]
    mask = np.ones((N, h * w), dtype="uint8")
    fallback = []
    for r in range(n_real):
      last = inputs["scene_feats"][int(np.asarray(inputs["obs_scene"][idxs[r]])[-1][0])]
      m = cell_mask_from_scene(args, last, allowed_classes,
                               float(getattr(args, "allowed_min_share", 0.0))).reshape(-1)
      if int(m.sum()) < int(args.num_out):
        fallback.append(r)
      else:
        mask[r] = m
    feed["cell_mask"] = mask
    feed["cell_mask_fallback"] = fallback
  class_costs = getattr(args, "class_costs", None)
  if class_costs:
    h, w = args.scene_grids[list(args.use_grids).index(True)]
    bias = np.zeros((N, h * w), dtype="float32")
    for r in range(n_real):
      last = inputs["scene_feats"][int(np.asarray(inputs["obs_scene"][idxs[r]])[-1][0])]
      bias[r] = cell_bias_from_scene(args, last, class_costs).reshape(-1)
    feed["cell_bias"] = bias
  motion = getattr(args, "motion_cost", None)
  if motion:
    # one row's tables for every real row; a padding row pays nothing
    D = 2 * int(motion["radius"]) + 1
    pad = np.arange(N) >= n_real
    cost = {"radius": int(motion["radius"])}
    for key, shape in (("vel", (N, D, D)), ("vel_far", (N,)), ("acc", (N, D, D)),
                       ("acc_far", (N,))):
      one = motion.get(key)
      if one is None:
        cost[key] = None
        continue
      full = np.broadcast_to(np.asarray(one, dtype="float32"), shape).copy()
      full[pad] = 0
      cost[key] = full
    feed["motion_cost"] = cost
  revisit = getattr(args, "revisit_cost", None)
  if revisit:
    per_row = np.full(N, revisit["cost"], dtype="float32")
    per_row[n_real:] = 0                    # a padding row pays nothing
    feed["revisit_cost"] = {"cost": per_row,
                            "seed_observed": bool(revisit.get("seed_observed", True))}
  return feed, n_real


def decode_trajectories(args, class_output, reg_output, beam_outputs, pred_len,
                        use_grid_idx):
  """One sample's outputs -> `num_out` trajectories of `pred_len` (x, y) points
  (code/multifuture_inference.py:475-517).  class_output [T,H,W,1] (greedy),
  reg_output [T,H,W,2], beam_outputs (logits [B,T,K], ids [B,T], logprobs [B])."""
  reg = np.asarray(reg_output).reshape([pred_len, -1, 2])
  centers = args.scene_grid_centers[use_grid_idx].reshape([-1, 2])

  def point(t, cls):
    return centers[cls] if args.center_only else centers[cls] + reg[t, cls]

  if args.greedy:
    sel = np.argmax(np.asarray(class_output).reshape([pred_len, -1]), axis=1)
    one = [point(t, sel[t]) for t in range(pred_len)]
    return [one for _ in range(args.num_out)]
  ids = beam_outputs[1]
  return [[point(t, ids[j, t]) for t in range(pred_len)] for j in range(args.num_out)]


def model_config(args, batch_size=1, max_pred_len=None):
  """The Namespace the reference builds for the model
  (code/multifuture_inference.py:419-452)."""
  import argparse
  return argparse.Namespace(
      modelname="model", batch_size=batch_size,
      beam_size=args.num_out, use_beam_search=not args.greedy,
      diverse_beam=args.diverse_beam, diverse_gamma=args.diverse_gamma,
      fix_num_timestep=args.fix_num_timestep,
      # --sample (not in the reference): num_out sampled futures instead of the beam search
      sample_futures=bool(getattr(args, "sample", False)),
      sample_temperature=float(getattr(args, "sample_temperature", 1.0)),
      sample_seed=int(getattr(args, "sample_seed", 0)),
      sample_without_replacement=bool(getattr(args, "sample_without_replacement", False)),
      sample_top_k=int(getattr(args, "sample_top_k", 0)),
      sample_top_p=float(getattr(args, "sample_top_p", 1.0)),
      use_teacher_forcing=False, is_train=False,
      scene_h=args.scene_h, scene_w=args.scene_w, scene_class=args.scene_class,
      use_soft_grid_class=args.use_soft_grid_class,
      use_single_decoder=args.use_single_decoder,
      obs_len=args.obs_length, pred_len=12,
      max_pred_len=max_pred_len or 12,
      emb_size=args.emb_size, enc_hidden_size=args.enc_hidden_size,
      dec_hidden_size=args.dec_hidden_size, activation_func="tanh",
      scene_conv_kernel=args.scene_conv_kernel, use_scene_enc=args.use_scene_enc,
      scene_conv_dim=args.scene_conv_dim, convlstm_kernel=args.convlstm_kernel,
      use_gnn=args.use_gnn, keep_prob=1.0,
      scene_grid_strides=args.scene_grid_strides, scene_grids=args.scene_grids,
      use_grids=args.use_grids)


def _inference_batches(args, inputs, n, N):
  """[(idxs, row lengths or None)] of one run: grouped by T_pred (every group's last batch
  padded by `inference_feed`), or -- `args.ragged_batches` -- the plan of
  `plan_ragged_batches` over all samples."""
  lens = [inputs["max_pred_lengths"][i] for i in range(n)]
  obs = [inputs["obs_lengths"][i] for i in range(n)] if "obs_lengths" in inputs else None
  if getattr(args, "ragged_batches", False):
    return [(idxs, lengths)
            for idxs, lengths, _ in plan_ragged_batches(lens, N, obs_lengths=obs).batches]
  by_len = {}
  for i in range(n):
    by_len.setdefault(lens[i], []).append(i)
  if obs is not None:      # short tracks: a group's rows by observation length, descending
    for T in by_len:
      by_len[T].sort(key=lambda i: (-obs[i], i))
  return [(by_len[T][lo:lo + N], None) for T in sorted(by_len)
          for lo in range(0, len(by_len[T]), N)]


def _note_unconstrained(args, feed, idxs, traj_ids):
  """args.unconstrained (a list, when the caller keeps one) collects the trajectory ids whose
  row fell back to the all-ones cell mask (`inference_feed`)."""
  if getattr(args, "unconstrained", None) is not None:
    args.unconstrained.extend(traj_ids[idxs[r]] for r in feed.get("cell_mask_fallback", []))


def run_inference(args, model, inputs, traj_ids):
  """The per-sample loop of code/multifuture_inference.py:458-523 ->
  (output_data {traj_id: [num_out][T][2]}, beam_prob {traj_id: (logits
  [1,B,T,K], logprobs [1,B])}).  `model.run_forward(feed)` is one sess.run."""
  if getattr(args, "device_decode", False):
    return run_inference_device(args, model, inputs, traj_ids)
  use_grid_idx = list(args.use_grids).index(True)
  N = model.config.batch_size
  output_data, beam_prob = {}, {}
  for idxs, lengths in _inference_batches(args, inputs, len(traj_ids), N):
    feed, n_real = inference_feed(inputs, args, idxs, batch_size=N, lengths=lengths)
    _note_unconstrained(args, feed, idxs, traj_ids)
    cls, reg, beam = model.run_forward(feed)
    # --use_single_decoder with beam search: the offsets come per beam, [N*B, T, H, W, 2]
    # (code/pred_models.py:287-296); the reference's script reshapes the B rows of its one
    # sample as [1, T, -1, 2] (code/multifuture_inference.py:478) -- kept as it is
    rows_per = reg[use_grid_idx].shape[0] // N
    for r in range(n_real):
      i = idxs[r]
      # (ragged batch: the row's own length; its outputs past it are padding)
      T_pred = inputs["max_pred_lengths"][i]
      b = None if beam is None else (beam[0][r][:, :T_pred], beam[1][r][:, :T_pred],
                                     beam[2][r])
      reg_r = (reg[use_grid_idx][r][:T_pred] if rows_per == 1
               else reg[use_grid_idx][r * rows_per:(r + 1) * rows_per][:, :T_pred])
      output_data[traj_ids[i]] = decode_trajectories(
          args, np.asarray(cls[use_grid_idx][r])[:T_pred], reg_r, b, T_pred, use_grid_idx)
      if b is not None and getattr(args, "save_prob_file", None) is not None:
        beam_prob[traj_ids[i]] = (b[0][None], b[2][None])
  ordered = {t: output_data[t] for t in traj_ids}
  return ordered, ({t: beam_prob[t] for t in traj_ids if t in beam_prob})


def run_inference_device(args, model, inputs, traj_ids):
  """`run_inference` with the decode on the device (`args.device_decode`):
  `model.run_forward_decoded(feed, ...)` returns the trajectories themselves -- centre +
  offset in float64, the operation of `decode_trajectories`, so the same values -- and only
  the beams' ids / log-probabilities besides.  Same first two return values; with
  `args.save_occupancy_file` a third, {traj_id: float32 [T, K]} (the map `eval_grid_nll`
  builds from the logits).  `args.save_prob_file` still needs every beam's logits: they are
  then fetched as well."""
  use_grid_idx = list(args.use_grids).index(True)
  N = model.config.batch_size
  greedy = bool(args.greedy)
  want_occ = getattr(args, "save_occupancy_file", None) is not None and not greedy
  want_prob = getattr(args, "save_prob_file", None) is not None and not greedy
  output_data, beam_prob, occupancy = {}, {}, {}
  for idxs, lengths in _inference_batches(args, inputs, len(traj_ids), N):
    feed, n_real = inference_feed(inputs, args, idxs, batch_size=N, lengths=lengths)
    _note_unconstrained(args, feed, idxs, traj_ids)
    dec = model.run_forward_decoded(feed, center_only=bool(args.center_only),
                                    occupancy=want_occ,
                                    grid_centers=args.scene_grid_centers,
                                    logits=want_prob)
    trajs = dec["trajs"]                                   # [N, B, T, 2]
    for r in range(n_real):
      i = idxs[r]
      T_pred = inputs["max_pred_lengths"][i]     # (ragged batch: the row's own length)
      rows = [trajs[r, 0]] * args.num_out if greedy else trajs[r, :args.num_out]
      output_data[traj_ids[i]] = [[row[t] for t in range(T_pred)] for row in rows]
      if want_occ:
        occupancy[traj_ids[i]] = dec["occupancy"][r][:T_pred]
      if want_prob:
        beam_prob[traj_ids[i]] = (dec["logits"][r][:, :T_pred][None],
                                  dec["logprobs"][r][None])
  ordered = {t: output_data[t] for t in traj_ids}
  ret = (ordered, {t: beam_prob[t] for t in traj_ids if t in beam_prob})
  if getattr(args, "save_occupancy_file", None) is not None:
    ret += ({t: occupancy[t] for t in traj_ids if t in occupancy},)
  return ret


def wor_importance_weights(logprobs, gumbels):
  """Importance weights of futures sampled WITHOUT replacement (stochastic beam search; after
  Kool, van Hoof, Welling, ICML 2019, eq. 19-20).  logprobs, gumbels [..., B] of one forward
  (Engine.forward_beam in that mode: exact log-probabilities and perturbed scores, the latter
  non-increasing along B, gumbels[..., 0] == 0), B >= 3.  kappa = the last slot's perturbed
  score is the threshold the first B - 1 futures exceeded; with p = exp(logprob)
      w_0 = p_0
      w_j = p_j / (1 - exp(-(exp(logprob_j - kappa) - p_j)))      0 < j < B - 1
  makes  sum_j w_j f(future_j)  an unbiased estimate of  E_model[f].

  The paper's weight, p / (1 - exp(-exp(logprob - kappa))), is unbiased for perturbed scores
  whose maximum is itself Gumbel(0)-distributed.  The engine's are CONDITIONED on that maximum
  being 0 (the root starts at G = 0; the drawn set does not depend on the maximum), and under
  that condition the paper's weight is biased (tests/test_sbs_host.py measures it).  In arrival
  times exp(-G): future i arrives at an Exp(p_i) time, the first arrival is at time 1, and by
  memorylessness every other future arrives at 1 + Exp(p_i): slot 0 is certain and weighs p_0,
  and a later one was included with probability 1 - exp(-p_j (exp(-kappa) - 1)), which is the
  denominator above.  (B = 2 leaves no future between slot 0 and the threshold: refused.)
  -> (raw [..., B - 1] float64, normalised [..., B - 1] float64 summing to 1: the lower-variance,
  biased estimator).  Valid for temperature 1 -- at another temperature the futures are a sample
  of the TEMPERED model, whose log-probabilities the engine does not report."""
  lp = np.asarray(logprobs, dtype=np.float64)
  g = np.asarray(gumbels, dtype=np.float64)
  if lp.shape != g.shape or lp.shape[-1] < 3:
    raise ValueError("wor_importance_weights: logprobs %s and gumbels %s must agree, B >= 3"
                     % (lp.shape, g.shape))
  kappa = g[..., -1:]
  lp = lp[..., :-1]
  p = np.exp(lp)
  with np.errstate(divide="ignore", invalid="ignore"):
    # 1 - exp(-x) = -expm1(-x)
    raw = p / -np.expm1(-(np.exp(lp - kappa) - p))
  raw[..., 0] = p[..., 0]
  return raw, raw / raw.sum(axis=-1, keepdims=True)


def proposal_importance_weights(logprobs, proposal_logprobs):
  """Self-normalised importance weights of INDEPENDENTLY sampled futures whose proposal differs
  from the model (a temperature != 1, a top-k / nucleus limit): logprobs, proposal_logprobs
  [..., S] of one forward (Engine.forward_beam: the model's exact log-probabilities and
  "proposal_logprobs", those of the distribution the futures were drawn from) ->
  softmax_s(logprobs - proposal_logprobs), float64 [..., S] summing to 1.
  sum_s w_s f(future_s) estimates E[f] under the model RESTRICTED TO THE PROPOSAL'S SUPPORT (and
  renormalised there): a future with a dropped cell has proposal probability 0, is never drawn,
  and no weight can bring it back -- with a temperature alone the support is everything and the
  estimate is of the model itself.  Consistent, biased of order 1 / S as every self-normalised
  estimator.  Futures sampled WITHOUT replacement are not independent draws: use
  wor_importance_weights on their logprobs and gumbels instead."""
  lp = np.asarray(logprobs, dtype=np.float64)
  lq = np.asarray(proposal_logprobs, dtype=np.float64)
  if lp.shape != lq.shape:
    raise ValueError("proposal_importance_weights: logprobs %s and proposal_logprobs %s must "
                     "agree" % (lp.shape, lq.shape))
  d = lp - lq
  w = np.exp(d - d.max(axis=-1, keepdims=True))
  return w / w.sum(axis=-1, keepdims=True)


# ------------------------------------------------- scoring given futures (not in the reference)

def futures_to_grid_ids(args, gt_by_traj, traj_id, use_grid_idx):
  """The ground-truth futures of one sample as grid cells of scale `use_grid_idx`, in the
  order of the sample's future ids -> (ids int32 [n_fut, T_max], lengths int32 [n_fut]);
  every (x, y) goes through `xy_to_grid_class`, steps past a future's length hold 0."""
  h, w = args.scene_grids[use_grid_idx]
  gt = gt_by_traj[traj_id]
  lengths = np.asarray([len(gt[fid]["x_agent_traj"]) for fid in gt], dtype="int32")
  ids = np.zeros((len(lengths), int(lengths.max()) if len(lengths) else 0), dtype="int32")
  for j, fid in enumerate(gt):
    xy = np.asarray([one[2:] for one in gt[fid]["x_agent_traj"]], dtype="float64")
    if len(xy):
      ids[j, :len(xy)] = xy_to_grid_class(xy, h, w, args.video_h, args.video_w)
  return ids, lengths


ScoreRow = collections.namedtuple("ScoreRow", ["sample", "futures", "lengths"])


def plan_score_batches(n_futures_per_sample, lengths, N, F, obs_lengths=None):
  """Batches of N rows x F futures over samples with any number of futures of any length.
  lengths[i][j] >= 1: the length of future j of sample i (n_futures_per_sample[i] of them).
  A sample's futures fill a row in order; a sample with more than F futures takes several
  rows (the engine then runs the same inputs once per row); a row's last futures and a
  batch's last rows are padding of length 0.  Rows are sorted by their longest future,
  descending (ties by sample, then by position), as `plan_ragged_batches` sorts samples: the
  live rows of every step are a prefix.  obs_lengths (one observation length per sample, short
  tracks): ties of the longest future are ordered by observation length descending first.
  -> [(rows, pred_length)], rows = N x ScoreRow(sample or None for a padding row, futures
  [indices into the sample's futures], lengths [F]), pred_length = the first row's longest."""
  assert N >= 1 and F >= 1
  rows = []
  for i, n_fut in enumerate(n_futures_per_sample):
    lens = [int(l) for l in lengths[i]]
    assert len(lens) == int(n_fut) and all(l >= 1 for l in lens), \
        "future lengths must be >= 1"
    for lo in range(0, len(lens), F):
      futs = list(range(lo, min(lo + F, len(lens))))
      rows.append(ScoreRow(i, futs, [lens[j] for j in futs] + [0] * (F - len(futs))))
  if obs_lengths is None:
    order = sorted(range(len(rows)), key=lambda r: (-max(rows[r].lengths), r))
  else:
    assert len(obs_lengths) == len(n_futures_per_sample)
    order = sorted(range(len(rows)), key=lambda r: (-max(rows[r].lengths),
                                                    -int(obs_lengths[rows[r].sample]), r))
  batches = []
  for lo in range(0, len(order), N):
    batch = [rows[r] for r in order[lo:lo + N]]
    batch += [ScoreRow(None, [], [0] * F)] * (N - len(batch))
    batches.append((batch, max(batch[0].lengths)))
  return batches


def run_scoring(args, model, inputs, traj_ids, gt):
  """Exact teacher-forced log-likelihood of every ground-truth future under the model
  (`model.run_score`: one scoring forward per batch of `plan_score_batches`) ->
  {traj_id: {future_id: {"logprob": float32, "step_logprobs": float32 [T], "ranks": int32
  [T]}}}, T the future's own length."""
  use_grid_idx = list(args.use_grids).index(True)
  N, F = model.config.batch_size, model.config.beam_size
  cells = [futures_to_grid_ids(args, gt, t, use_grid_idx) for t in traj_ids]
  plan = plan_score_batches([len(c[1]) for c in cells], [c[1] for c in cells], N, F,
                            obs_lengths=inputs.get("obs_lengths"))
  scores = {t: {} for t in traj_ids}
  for rows, T_pred in plan:
    real = [row.sample for row in rows if row.sample is not None]
    feed, _ = inference_feed(inputs, args, real, batch_size=N, pred_length=T_pred)
    ids = np.zeros((N, F, T_pred), dtype="int32")
    lens = np.asarray([row.lengths for row in rows], dtype="int32")
    for n, row in enumerate(rows):
      for f, j in enumerate(row.futures):
        ids[n, f, :lens[n, f]] = cells[row.sample][0][j, :lens[n, f]]
    out = model.run_score(feed, ids, lens)
    for n, row in enumerate(rows):
      if row.sample is None:
        continue
      fids = list(gt[traj_ids[row.sample]])
      for f, j in enumerate(row.futures):
        L = int(lens[n, f])
        scores[traj_ids[row.sample]][fids[j]] = {
            "logprob": out["logprobs"][n, f],
            "step_logprobs": out["step_logprobs"][n, f, :L].copy(),
            "ranks": out["ranks"][n, f, :L].copy()}
  return {t: {fid: scores[t][fid] for fid in gt[t]} for t in traj_ids}


def eval_exact_nll(scores, time_list=(0, 1, 2, 3, 4)):
  """Exact per-step negative log-likelihood of the scored futures (`run_scoring`) at
  T=1..5: the mean of -step_logprob[t] over the futures that reach step t.
  -> (nll, counts) in the form of `eval_grid_nll`, and the hit rates of the model's step
  distribution over every scored step, {"top1": share of ranks == 0, "top5": of ranks < 5,
  "steps": their number}."""
  nlls = {"T=%d" % (t + 1): [] for t in time_list}
  ranks = []
  for traj_id in scores:
    for fid in scores[traj_id]:
      one = scores[traj_id][fid]
      ranks.append(np.asarray(one["ranks"]).reshape(-1))
      for t in time_list:
        if len(one["step_logprobs"]) > t:
          nlls["T=%d" % (t + 1)].append(-float(one["step_logprobs"][t]))
  ranks = np.concatenate(ranks) if ranks else np.zeros(0, dtype="int32")
  hits = {"top1": float(np.mean(ranks == 0)) if ranks.size else float("nan"),
          "top5": float(np.mean(ranks < 5)) if ranks.size else float("nan"),
          "steps": int(ranks.size)}
  return {k: (float(np.mean(v)) if v else float("nan")) for k, v in nlls.items()}, \
      {k: len(v) for k, v in nlls.items()}, hits


# ------------------------------------------------------------------ metrics

def _get_min(errors):
  sums = [sum(e) for e in errors]
  idx = sums.index(min(sums))
  return errors[idx], idx


def eval_min_ade_fde(gt_by_traj, prediction):
  """minADE_K / minFDE_K (code/multifuture_eval_trajs.py:16-88): for every GT
  future, the prediction with the smallest summed (resp. final) error; errors
  pooled over all GT timesteps; cam4 = top-down, the rest = 45-degree.
  Returns {"ade": {...}, "fde": {...}} over ("45-degree", "top-down", "all")."""
  keys = ("45-degree", "top-down", "all")
  ade = {k: [] for k in keys}
  fde = {k: [] for k in keys}
  for traj_id in prediction:
    camera = traj_id.split("_")[-1]
    gt = gt_by_traj[traj_id]
    for future_id in gt:
      gt_traj = np.array([one[2:] for one in gt[future_id]["x_agent_traj"]])
      pred_len = len(gt_traj)
      a_err, f_err = [], []
      for pred_out in prediction[traj_id]:
        assert len(pred_out) >= pred_len
        d = np.sqrt(np.sum((gt_traj - np.asarray(pred_out)[:pred_len]) ** 2, axis=1))
        a_err.append(d.tolist())
        f_err.append([d[-1]])
      min_a, _ = _get_min(a_err)
      min_f, _ = _get_min(f_err)
      view = "top-down" if camera == "cam4" else "45-degree"
      ade[view] += min_a
      fde[view] += min_f
      ade["all"] += min_a
      fde["all"] += min_f
  mean = lambda v: float(np.mean(v)) if len(v) else float("nan")
  return {"ade": {k: mean(ade[k]) for k in keys}, "fde": {k: mean(fde[k]) for k in keys}}


def _softmax(x, axis=None):
  x = x - x.max(axis=axis, keepdims=True)
  y = np.exp(x)
  return y / y.sum(axis=axis, keepdims=True)


def eval_grid_nll(gt_by_traj, predictions, scene_h=18, scene_w=32, video_h=1080,
                  video_w=1920, time_list=(0, 1, 2, 3, 4)):
  """Grid negative log-likelihood at T=1..5 (code/multifuture_eval_trajs_prob.py:
  69-119): beams' per-step softmax maps mixed with softmax(beam logprobs)."""
  nlls = {"T=%d" % (t + 1): [] for t in time_list}
  for traj_id in predictions:
    gt = gt_by_traj[traj_id]
    entry = predictions[traj_id]
    occ = None
    if isinstance(entry, np.ndarray):     # already the mixture: float32 [T, K] (device decode)
      occ = entry
      assert occ.ndim == 2 and occ.shape[-1] == scene_h * scene_w
    else:
      beams, logprobs = entry
      probs = _softmax(np.squeeze(logprobs))
      beams = _softmax(np.squeeze(beams), axis=-1)          # [B, T, K]
      assert beams.shape[-1] == scene_h * scene_w
    for t in time_list:
      xys = [gt[fid]["x_agent_traj"][t][2:] for fid in gt
             if len(gt[fid]["x_agent_traj"]) > t]
      if not xys:
        continue
      grid = occ[t] if occ is not None else \
          (beams[:, t, :].astype("float32") * probs[:, None].astype("float32")).sum(0)
      idx = xy_to_grid_class(np.asarray(xys), scene_h, scene_w, video_h, video_w)
      nll = float(np.mean([-np.log(grid[k] + np.finfo(float).eps) for k in idx]))
      nlls["T=%d" % (t + 1)].append(nll)
  return {k: (float(np.mean(v)) if v else float("nan")) for k, v in nlls.items()}, \
      {k: len(v) for k, v in nlls.items()}


def load_gt(multifuture_path, traj_ids):
  out = {}
  for traj_id in traj_ids:
    with open(os.path.join(multifuture_path, "%s.p" % traj_id), "rb") as f:
      out[traj_id] = pickle.load(f)
  return out
