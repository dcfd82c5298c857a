# coding=utf-8
"""ctypes binding of libmultiverse_hip.so (C ABI: include/multiverse_hip.h).

There is NO CPU fallback: if the HIP library is missing or a call fails this
module raises.  The library is built in-tree by `__graft_entry__.build()`
(`hipcc --offload-arch=gfx950`), so it travels with the source snapshot.
"""

from __future__ import annotations

import ctypes as C
import os

import numpy as np

MV_MAX_SCALES = 2
MV_ABI_VERSION = 5

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmultiverse_hip.so")

# every symbol include/multiverse_hip.h declares
EXPORTED_SYMBOLS = [
    "mv_create", "mv_destroy", "mv_last_error", "mv_abi_version",
    "mv_set_param", "mv_get_param", "mv_num_params", "mv_param_info",
    "mv_forward_greedy", "mv_forward_beam",
    "mv_upload_inputs", "mv_run_greedy_resident", "mv_run_beam_resident",
    "mv_synchronize", "mv_download_outputs", "mv_download_beam_outputs",
    "mv_set_graph_mode", "mv_set_compute_mode", "mv_set_profiling", "mv_reset_kernel_stats", "mv_num_kernel_stats",
    "mv_kernel_stat", "mv_kernel_stat_dense_flops", "mv_kernel_stat_mfma_flops",
    "mv_time_greedy_resident",
    "mv_time_beam_resident",
    "mv_op_convlstm_step", "mv_op_convlstm_step16", "mv_op_gnn", "mv_op_gnn_variant",
    "mv_op_hidden2grid", "mv_op_beam_step",
    "mv_train_init", "mv_train_step", "mv_train_forward_backward",
    "mv_upload_targets", "mv_grad_buffer", "mv_train_apply", "mv_get_grad", "mv_get_global_step",
    "mv_set_global_step", "mv_get_opt_slot", "mv_set_opt_slot",
    "mv_set_dropout_seed", "mv_get_opt_scalars", "mv_set_opt_scalars",
    "mv_comm_unique_id", "mv_allreduce_init", "mv_allreduce_info",
    "mv_attack_begin", "mv_attack_end", "mv_set_scene_feat", "mv_get_scene_feat",
    "mv_get_scene_grad", "mv_attack_step", "mv_scene_mix", "mv_get_sample_losses",
    "mv_set_label_mixup", "mv_clear_label_mixup",
    "mv_op_convlstm_bwd", "mv_op_gnn_bwd", "mv_op_convlstm_bwd16", "mv_op_lstm_gate_bwd",
    "mv_set_grid_centers", "mv_upload_inputs_compact", "mv_upload_targets_compact",
    "mv_pipeline_create", "mv_submit_greedy", "mv_collect_greedy",
    "mv_decode_trajectories", "mv_beam_occupancy", "mv_download_beam_ids",
    "mv_set_pred_lengths", "mv_last_forward_gate_rows", "mv_set_sampling",
    "mv_score_futures", "mv_upload_score_futures", "mv_run_score_resident",
    "mv_download_scores", "mv_time_score_resident",
    "mv_set_sampling_mode", "mv_download_beam_gumbels", "mv_op_sbs_step",
    "mv_set_sampling_truncation", "mv_download_beam_proposal_logprobs", "mv_op_sample_step",
    "mv_enc_cone_build",
    "mv_set_obs_lengths",
    "mv_set_cell_mask", "mv_graph_captures", "mv_op_beam_step_masked", "mv_op_sbs_step_masked",
    "mv_op_sample_step_masked",
    "mv_set_train_lengths", "mv_last_train_gate_rows",
    "mv_set_cell_bias", "mv_op_beam_step_biased", "mv_op_sbs_step_biased",
    "mv_op_sample_step_biased",
    "mv_scene_conv_form", "mv_op_scene_conv",
    "mv_op_decode_tail",
    "mv_set_motion_cost", "mv_op_beam_step_motion", "mv_op_sbs_step_motion",
    "mv_op_sample_step_motion",
    "mv_set_revisit_cost", "mv_op_beam_step_path", "mv_op_sbs_step_path",
    "mv_op_sample_step_path",
    "mv_op_small_conv_dgrad", "mv_op_small_conv_wgrad", "mv_op_colsum", "mv_op_long_sum",
    "mv_op_scene_conv_bwd", "mv_op_grid_emb_onehot_wgrad", "mv_op_train_loss",
]


class MvError(RuntimeError):
  pass


class mv_config(C.Structure):
  _fields_ = [
      ("abi_version", C.c_int32),
      ("batch_size", C.c_int32),
      ("obs_len", C.c_int32),
      ("max_pred_len", C.c_int32),
      ("scene_h", C.c_int32), ("scene_w", C.c_int32), ("scene_class", C.c_int32),
      ("scene_conv_dim", C.c_int32), ("scene_conv_kernel", C.c_int32),
      ("emb_size", C.c_int32),
      ("hidden_size", C.c_int32),
      ("convlstm_kernel", C.c_int32),
      ("num_scales", C.c_int32),
      ("grid_h", C.c_int32 * MV_MAX_SCALES),
      ("grid_w", C.c_int32 * MV_MAX_SCALES),
      ("use_grid", C.c_int32 * MV_MAX_SCALES),
      ("use_gnn", C.c_int32),
      ("beam_size", C.c_int32),
      ("diverse_beam", C.c_int32),
      ("diverse_gamma", C.c_float),
      ("fix_num_timestep", C.c_int32),
      ("class_feedback_dense", C.c_int32),
      ("use_single_decoder", C.c_int32),
      ("simaug_graph", C.c_int32),
      ("activation", C.c_int32),
  ]


_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int32)


class mv_inputs(C.Structure):
  _fields_ = [
      ("obs_scene", _ip),
      ("scene_feat", _fp),
      ("num_scene_frames", C.c_int32),
      ("pred_len", C.c_int32),
      ("grid_obs_labels", _ip * MV_MAX_SCALES),
      ("grid_obs_regress", _fp * MV_MAX_SCALES),
  ]


_dp = C.POINTER(C.c_double)
_u8p = C.POINTER(C.c_uint8)


class mv_step_motion(C.Structure):
  """The motion argument of the three `_motion` step ops (include/multiverse_hip.h)."""
  _fields_ = [
      ("W", C.c_int32), ("radius", C.c_int32),
      ("vel", _fp), ("vel_far", _fp), ("acc", _fp), ("acc_far", _fp),
      ("prev1", _ip), ("prev0", _ip),
  ]


MV_MOTION_MAX_RADIUS = 4


class mv_step_revisit(C.Structure):
  """The revisit argument of the three `_path` step ops (include/multiverse_hip.h)."""
  _fields_ = [("cost", _fp), ("prev1", _ip), ("visited", _u8p), ("visited_out", _u8p)]


class mv_inputs_compact(C.Structure):
  _fields_ = [
      ("obs_scene", _ip),
      ("scene_feat_u8", _u8p),
      ("num_scene_frames", C.c_int32),
      ("pred_len", C.c_int32),
      ("grid_obs_labels", _ip * MV_MAX_SCALES),
      ("obs_xy", _dp),
      ("num_rows", C.c_int32),
  ]


class mv_targets_compact(C.Structure):
  _fields_ = [
      ("grid_pred_labels", _ip * MV_MAX_SCALES),
      ("pred_xy", _dp),
      ("num_rows", C.c_int32),
  ]


class mv_outputs(C.Structure):
  _fields_ = [
      ("grid_pred_class", _fp * MV_MAX_SCALES),
      ("grid_pred_reg", _fp * MV_MAX_SCALES),
  ]


class mv_beam_outputs(C.Structure):
  _fields_ = [
      ("best_beam", _fp), ("grid_reg", _fp), ("logits", _fp), ("ids", _ip),
      ("logprobs", _fp),
  ]


class mv_score_futures_in(C.Structure):
  _fields_ = [("ids", _ip), ("lengths", _ip)]


class mv_score_outputs(C.Structure):
  _fields_ = [("step_logprobs", _fp), ("logprobs", _fp), ("ranks", _ip)]


class mv_tail_chain(C.Structure):
  _fields_ = [
      ("rows", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("kind", C.c_int32),
      ("h", _fp), ("w_out", _fp), ("emb_w", _fp), ("emb_b", _fp),
      ("out", _fp), ("ids", _ip), ("x", _fp), ("planes", C.POINTER(C.c_uint16)),
      ("planes_elems", C.c_int64),
  ]


class mv_train_config(C.Structure):
  _fields_ = [
      ("optimizer", C.c_int32),
      ("init_lr", C.c_float), ("emb_lr", C.c_float),
      ("use_cosine_lr", C.c_int32),
      ("has_decay", C.c_int32), ("learning_rate_decay", C.c_float),
      ("decay_steps", C.c_int32), ("max_steps", C.c_int32),
      ("do_clip", C.c_int32), ("clip_gradient_norm", C.c_float),
      ("wd", C.c_float),
      ("grid_loss_weight", C.c_float), ("grid_reg_loss_weight", C.c_float),
      ("class_feedback", C.c_int32), ("reg_teacher_forcing", C.c_int32),
      ("use_soft_grid_class", C.c_int32), ("soft_kernel_size", C.c_int32),
      ("soft_kernel", C.c_float * 25),
      ("mask_grid_regression", C.c_int32), ("keep_prob", C.c_float),
  ]


class mv_targets(C.Structure):
  _fields_ = [
      ("grid_pred_labels", _ip * MV_MAX_SCALES),
      ("grid_pred_regress", _fp * MV_MAX_SCALES),
  ]


class mv_losses(C.Structure):
  _fields_ = [
      ("loss", C.c_float), ("wd_loss", C.c_float),
      ("pred_grid_loss", C.c_float * (2 * MV_MAX_SCALES)),
      ("num_pred_grid_loss", C.c_int32),
  ]


_lib = None


def load():
  """dlopen the in-tree library; raises MvError if it has not been built."""
  global _lib
  if _lib is not None:
    return _lib
  path = os.environ.get("MV_LIB_PATH", LIB_PATH)   # A/B builds of the same ABI (tuning)
  if not os.path.exists(path):
    raise MvError(
        "%s not found: the HIP extension has not been built "
        "(run `python -c 'import __graft_entry__ as g; g.build()'`). "
        "There is no CPU fallback." % LIB_PATH)
  lib = C.CDLL(path)
  h = C.c_void_p
  lib.mv_last_error.restype = C.c_char_p
  lib.mv_last_error.argtypes = [h]
  lib.mv_abi_version.argtypes = []
  lib.mv_create.argtypes = [C.POINTER(mv_config), C.c_int, C.POINTER(h)]
  lib.mv_destroy.argtypes = [h]
  lib.mv_set_param.argtypes = [h, C.c_char_p, _fp, C.POINTER(C.c_int64), C.c_int32]
  lib.mv_get_param.argtypes = [h, C.c_char_p, _fp, C.c_int64]
  lib.mv_num_params.argtypes = [h]
  lib.mv_param_info.argtypes = [h, C.c_int32, C.c_char_p, C.c_int32,
                                C.POINTER(C.c_int64)]
  lib.mv_forward_greedy.argtypes = [h, C.POINTER(mv_inputs), C.POINTER(mv_outputs)]
  lib.mv_forward_beam.argtypes = [h, C.POINTER(mv_inputs),
                                  C.POINTER(mv_beam_outputs)]
  lib.mv_upload_inputs.argtypes = [h, C.POINTER(mv_inputs)]
  lib.mv_pipeline_create.argtypes = [h, C.c_int32]
  lib.mv_submit_greedy.argtypes = [h, C.POINTER(mv_inputs)]
  lib.mv_collect_greedy.argtypes = [h, C.POINTER(mv_outputs), C.POINTER(C.c_int32)]
  lib.mv_set_grid_centers.argtypes = [h, C.c_int32, _dp]
  lib.mv_upload_inputs_compact.argtypes = [h, C.POINTER(mv_inputs_compact)]
  lib.mv_upload_targets_compact.argtypes = [h, C.POINTER(mv_targets_compact)]
  lib.mv_run_greedy_resident.argtypes = [h]
  lib.mv_run_beam_resident.argtypes = [h]
  lib.mv_synchronize.argtypes = [h]
  lib.mv_download_outputs.argtypes = [h, C.POINTER(mv_outputs)]
  lib.mv_download_beam_outputs.argtypes = [h, C.POINTER(mv_beam_outputs)]
  lib.mv_decode_trajectories.argtypes = [h, C.c_int32, C.c_int32, _dp]
  lib.mv_beam_occupancy.argtypes = [h, _fp]
  lib.mv_download_beam_ids.argtypes = [h, _ip, _fp]
  lib.mv_set_pred_lengths.argtypes = [h, _ip]
  if hasattr(lib, "mv_set_obs_lengths"):    # (an A/B build through MV_LIB_PATH may predate it)
    lib.mv_set_obs_lengths.argtypes = [h, _ip]
  if hasattr(lib, "mv_set_cell_mask"):      # (as above)
    lib.mv_set_cell_mask.argtypes = [h, _u8p, C.c_int32]
    lib.mv_graph_captures.argtypes = [h, C.POINTER(C.c_int64)]
    lib.mv_op_beam_step_masked.argtypes = [C.c_int, _fp, _fp, _u8p, C.c_int32, C.c_int32,
                                           C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                           C.c_int32, _fp, _ip, _ip]
    lib.mv_op_sbs_step_masked.argtypes = [C.c_int, _fp, _fp, _fp, _fp, _u8p, C.c_int32,
                                          C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_uint32,
                                          _fp, _fp, _fp, _ip, _ip]
    lib.mv_op_sample_step_masked.argtypes = [C.c_int, _fp, _u8p, C.c_int32, C.c_int32, C.c_int32,
                                             C.c_int32, C.c_float, C.c_uint32, C.c_int32,
                                             C.c_float, C.c_int32, _ip, _fp, _fp, _u8p]
  if hasattr(lib, "mv_set_cell_bias"):      # (as above)
    lib.mv_set_cell_bias.argtypes = [h, _fp, C.c_int32]
    lib.mv_op_beam_step_biased.argtypes = [C.c_int, _fp, _fp, _u8p, _fp, C.c_int32, C.c_int32,
                                           C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                           C.c_int32, _fp, _ip, _ip]
    lib.mv_op_sbs_step_biased.argtypes = [C.c_int, _fp, _fp, _fp, _fp, _u8p, _fp, C.c_int32,
                                          C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_uint32,
                                          _fp, _fp, _fp, _ip, _ip]
    lib.mv_op_sample_step_biased.argtypes = [C.c_int, _fp, _u8p, _fp, C.c_int32, C.c_int32,
                                             C.c_int32, C.c_int32, C.c_float, C.c_uint32,
                                             C.c_int32, C.c_float, C.c_int32, _ip, _fp, _fp, _u8p]
  if hasattr(lib, "mv_set_motion_cost"):    # (as above)
    _mp = C.POINTER(mv_step_motion)
    lib.mv_set_motion_cost.argtypes = [h, C.c_int32, _fp, _fp, _fp, _fp]
    lib.mv_op_beam_step_motion.argtypes = [C.c_int, _fp, _fp, _u8p, _fp, _mp, C.c_int32,
                                           C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                           C.c_int32, _fp, _ip, _ip]
    lib.mv_op_sbs_step_motion.argtypes = [C.c_int, _fp, _fp, _fp, _fp, _u8p, _fp, _mp, C.c_int32,
                                          C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_uint32,
                                          _fp, _fp, _fp, _ip, _ip]
    lib.mv_op_sample_step_motion.argtypes = [C.c_int, _fp, _u8p, _fp, _mp, C.c_int32, C.c_int32,
                                             C.c_int32, C.c_int32, C.c_float, C.c_uint32,
                                             C.c_int32, C.c_float, C.c_int32, _ip, _fp, _fp, _u8p]
  if hasattr(lib, "mv_set_revisit_cost"):   # (as above)
    _mp = C.POINTER(mv_step_motion)
    _rp = C.POINTER(mv_step_revisit)
    lib.mv_set_revisit_cost.argtypes = [h, _fp, C.c_int32]
    lib.mv_op_beam_step_path.argtypes = [C.c_int, _fp, _fp, _u8p, _fp, _mp, _rp, C.c_int32,
                                         C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                         C.c_int32, _fp, _ip, _ip]
    lib.mv_op_sbs_step_path.argtypes = [C.c_int, _fp, _fp, _fp, _fp, _u8p, _fp, _mp, _rp,
                                        C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                        C.c_uint32, _fp, _fp, _fp, _ip, _ip]
    lib.mv_op_sample_step_path.argtypes = [C.c_int, _fp, _u8p, _fp, _mp, _rp, C.c_int32,
                                           C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_uint32,
                                           C.c_int32, C.c_float, C.c_int32, _ip, _fp, _fp, _u8p]
  lib.mv_last_forward_gate_rows.argtypes = [h, C.POINTER(C.c_int64)]
  lib.mv_set_sampling.argtypes = [h, C.c_int32, C.c_float, C.c_uint32]
  lib.mv_set_sampling_mode.argtypes = [h, C.c_int32]
  lib.mv_download_beam_gumbels.argtypes = [h, _fp]
  lib.mv_set_sampling_truncation.argtypes = [h, C.c_int32, C.c_float]
  lib.mv_download_beam_proposal_logprobs.argtypes = [h, _fp]
  lib.mv_op_sample_step.argtypes = [C.c_int, _fp, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                    C.c_float, C.c_uint32, C.c_int32, C.c_float, C.c_int32,
                                    _ip, _fp, _fp, _u8p]
  if hasattr(lib, "mv_enc_cone_build"):     # (an A/B build through MV_LIB_PATH may predate it)
    lib.mv_enc_cone_build.argtypes = [_ip] + [C.c_int32] * 5 + [_ip, C.POINTER(C.c_int64)]
  if hasattr(lib, "mv_op_scene_conv"):      # (as above)
    lib.mv_scene_conv_form.argtypes = [C.c_int32] * 3
    lib.mv_op_scene_conv.argtypes = [C.c_int, C.c_int32, _fp, _fp, _fp] + [C.c_int32] * 7 + [_fp]
  if hasattr(lib, "mv_op_decode_tail"):     # (as above)
    lib.mv_op_decode_tail.argtypes = [C.c_int] + [C.c_int32] * 6 + [C.POINTER(mv_tail_chain),
                                                                    C.c_int32]
  lib.mv_op_sbs_step.argtypes = [C.c_int, _fp, _fp, _fp, _fp, C.c_int32, C.c_int32, C.c_int32,
                                 C.c_int32, C.c_float, C.c_uint32, _fp, _fp, _fp, _ip, _ip]
  lib.mv_score_futures.argtypes = [h, C.POINTER(mv_inputs), C.POINTER(mv_score_futures_in),
                                   C.POINTER(mv_score_outputs)]
  lib.mv_upload_score_futures.argtypes = [h, C.POINTER(mv_score_futures_in)]
  lib.mv_run_score_resident.argtypes = [h]
  lib.mv_download_scores.argtypes = [h, C.POINTER(mv_score_outputs)]
  lib.mv_time_score_resident.argtypes = [h, C.c_int32, _fp]
  lib.mv_set_profiling.argtypes = [h, C.c_int32]
  lib.mv_set_graph_mode.argtypes = [h, C.c_int32]
  lib.mv_set_compute_mode.argtypes = [h, C.c_int32]
  lib.mv_reset_kernel_stats.argtypes = [h]
  lib.mv_num_kernel_stats.argtypes = [h]
  lib.mv_kernel_stat.argtypes = [h, C.c_int32, C.c_char_p, C.c_int32,
                                 C.POINTER(C.c_int64), C.POINTER(C.c_double),
                                 C.POINTER(C.c_double), C.POINTER(C.c_double)]
  lib.mv_kernel_stat_dense_flops.argtypes = [h, C.c_int32, C.POINTER(C.c_double)]
  lib.mv_kernel_stat_mfma_flops.argtypes = [h, C.c_int32, C.POINTER(C.c_double)]
  lib.mv_time_greedy_resident.argtypes = [h, C.c_int32, _fp]
  lib.mv_time_beam_resident.argtypes = [h, C.c_int32, _fp]
  lib.mv_op_convlstm_step.argtypes = [C.c_int, _fp, _fp, _fp, _fp, _fp] + \
      [C.c_int32] * 5 + [_fp, _fp]
  lib.mv_op_convlstm_step16.argtypes = [C.c_int, C.c_int32, _fp, _fp, _fp, _fp, _fp] + \
      [C.c_int32] * 5 + [_fp, _fp, _fp]
  lib.mv_op_gnn.argtypes = [C.c_int, _fp, _fp] + [C.c_int32] * 5 + [_fp]
  if hasattr(lib, "mv_op_gnn_variant"):     # (an A/B build through MV_LIB_PATH may predate it)
    lib.mv_op_gnn_variant.argtypes = [C.c_int, _fp, _fp] + [C.c_int32] * 6 + [_fp]
  lib.mv_op_hidden2grid.argtypes = [C.c_int, _fp, _fp] + [C.c_int32] * 5 + [_fp]
  lib.mv_op_beam_step.argtypes = [C.c_int, _fp, _fp, C.c_int32, C.c_int32,
                                  C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                  C.c_int32, _fp, _ip, _ip]
  lib.mv_train_init.argtypes = [h, C.POINTER(mv_train_config)]
  lib.mv_train_step.argtypes = [h, C.POINTER(mv_inputs), C.POINTER(mv_targets),
                                C.POINTER(mv_losses)]
  lib.mv_train_forward_backward.argtypes = lib.mv_train_step.argtypes
  lib.mv_upload_targets.argtypes = [h, C.POINTER(mv_targets)]
  lib.mv_grad_buffer.argtypes = [h, C.POINTER(_fp), C.POINTER(C.c_int64)]
  lib.mv_train_apply.argtypes = [h, C.c_float]
  if hasattr(lib, "mv_set_train_lengths"):  # (an A/B build through MV_LIB_PATH may predate it)
    lib.mv_set_train_lengths.argtypes = [h, _ip, _ip]
    lib.mv_last_train_gate_rows.argtypes = [h, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
  lib.mv_get_grad.argtypes = [h, C.c_char_p, _fp, C.c_int64]
  lib.mv_get_global_step.argtypes = [h, C.POINTER(C.c_int64)]
  lib.mv_set_global_step.argtypes = [h, C.c_int64]
  lib.mv_comm_unique_id.argtypes = [_u8p]
  lib.mv_allreduce_init.argtypes = [h, C.c_int32, C.c_int32, _u8p]
  lib.mv_allreduce_info.argtypes = [h, _ip, _ip, _ip, _dp]
  lib.mv_attack_begin.argtypes = [h]
  lib.mv_attack_end.argtypes = [h]
  lib.mv_set_scene_feat.argtypes = [h, _fp]
  lib.mv_get_scene_feat.argtypes = [h, _fp]
  lib.mv_get_scene_grad.argtypes = [h, _fp]
  lib.mv_attack_step.argtypes = [h, C.c_float, C.c_float]
  lib.mv_scene_mix.argtypes = [h, _fp, C.c_float]
  lib.mv_get_sample_losses.argtypes = [h, C.c_int32, _fp]
  lib.mv_set_label_mixup.argtypes = [h, C.POINTER(_ip), C.POINTER(_ip), C.c_float, _fp]
  lib.mv_clear_label_mixup.argtypes = [h]
  lib.mv_set_dropout_seed.argtypes = [h, C.c_uint32]
  lib.mv_get_opt_scalars.argtypes = [h, _fp, _fp]
  lib.mv_set_opt_scalars.argtypes = [h, C.c_float, C.c_float]
  lib.mv_get_opt_slot.argtypes = [h, C.c_char_p, C.c_int32, _fp, C.c_int64]
  lib.mv_set_opt_slot.argtypes = [h, C.c_char_p, C.c_int32, _fp, C.c_int64]
  lib.mv_op_convlstm_bwd.argtypes = [C.c_int] + [_fp] * 7 + [C.c_int32] * 5 + [_fp] * 5
  lib.mv_op_gnn_bwd.argtypes = [C.c_int, _fp, _fp, _fp] + [C.c_int32] * 5 + [_fp, _fp]
  if hasattr(lib, "mv_op_convlstm_bwd16"):  # (an A/B build through MV_LIB_PATH may predate it)
    lib.mv_op_convlstm_bwd16.argtypes = [C.c_int, C.c_int32, C.c_int32] + [_fp] * 4 + \
        [C.c_int32] * 5 + [_fp] * 3 + [_ip, _ip]
    lib.mv_op_lstm_gate_bwd.argtypes = [C.c_int, C.c_int32] + [_fp] * 5 + [C.c_int32] * 2 + \
        [_fp, _fp, _ip, _fp]
  if hasattr(lib, "mv_op_train_loss"):      # (an A/B build through MV_LIB_PATH may predate them)
    i64 = C.c_int64
    lib.mv_op_small_conv_dgrad.argtypes = [C.c_int, C.c_int32, _fp, i64, _fp, _fp, i64] + \
        [C.c_int32] * 6 + [_ip]
    lib.mv_op_small_conv_wgrad.argtypes = [C.c_int, C.c_int32, _fp, _fp] + [C.c_int32] * 5 + \
        [_fp, _ip]
    lib.mv_op_colsum.argtypes = [C.c_int, _fp, i64, i64, _fp, _ip]
    lib.mv_op_long_sum.argtypes = [C.c_int, _fp, i64, C.c_float, _fp, _ip]
    lib.mv_op_scene_conv_bwd.argtypes = [C.c_int, _fp, _fp, _fp, _fp] + [C.c_int32] * 7 + \
        [_fp, C.c_int32, _fp, _fp, _fp, _fp, _ip]
    lib.mv_op_grid_emb_onehot_wgrad.argtypes = [C.c_int, _fp, _ip] + [C.c_int32] * 6 + [_fp]
    lib.mv_op_train_loss.argtypes = [C.c_int, C.c_int32, _fp, _ip, _fp, _fp, _fp, _fp, _ip] + \
        [C.c_int32] * 3 + [C.c_float, _fp, _fp, _fp, _ip]
  if lib.mv_abi_version() != MV_ABI_VERSION:
    raise MvError("ABI version mismatch: library %d, binding %d"
                  % (lib.mv_abi_version(), MV_ABI_VERSION))
  _lib = lib
  return lib


def f32(a):
  return np.ascontiguousarray(a, dtype=np.float32)


def i32(a):
  return np.ascontiguousarray(a, dtype=np.int32)


def fptr(a):
  return a.ctypes.data_as(_fp) if a is not None else _fp()


def iptr(a):
  return a.ctypes.data_as(_ip) if a is not None else _ip()


def check(rc, handle=None):
  if rc != 0:
    msg = load().mv_last_error(handle)
    raise MvError(msg.decode("utf-8", "replace") if msg else "error %d" % rc)


ACTIVATIONS = {"tanh": 0, "relu": 1, "lrelu": 2, "leaky_relu": 2}


def activation_code(act):
  """--activation_func (code/pred_utils.py:86-94): a name, or the TF function process_args
  replaced it with (its __name__: tanh / relu / leaky_relu)."""
  name = act if isinstance(act, str) else getattr(act, "__name__", None)
  if name not in ACTIVATIONS:
    raise MvError("activation_func %r: tanh, relu or lrelu" % (act,))
  return ACTIVATIONS[name]


def uses_scene(cfg):
  """--use_scene_enc: the scene stack feeds the class encoders and the graph attention."""
  return bool(getattr(cfg, "use_scene_enc", True))


def make_config(cfg):
  """argparse.Namespace (after process_args) -> mv_config."""
  c = mv_config()
  c.abi_version = MV_ABI_VERSION
  c.batch_size = int(cfg.batch_size)
  c.obs_len = int(cfg.obs_len)
  c.max_pred_len = int(getattr(cfg, "max_pred_len", None) or cfg.pred_len)
  c.scene_h, c.scene_w, c.scene_class = int(cfg.scene_h), int(cfg.scene_w), \
      int(cfg.scene_class)
  # a model built without the scene encoder (--use_scene_enc off, the reference's default
  # graph, code/pred_models.py:146-165, 218-229) is scene_conv_dim 0 on the C ABI
  c.scene_conv_dim = int(cfg.scene_conv_dim) if uses_scene(cfg) else 0
  c.scene_conv_kernel = int(cfg.scene_conv_kernel)
  c.emb_size = int(cfg.emb_size)
  if int(cfg.enc_hidden_size) != int(cfg.dec_hidden_size):
    raise MvError("enc_hidden_size != dec_hidden_size is not supported")
  c.hidden_size = int(cfg.enc_hidden_size)
  c.convlstm_kernel = int(cfg.convlstm_kernel)
  if len(cfg.scene_grids) > MV_MAX_SCALES:
    raise MvError("at most %d scales" % MV_MAX_SCALES)
  c.num_scales = len(cfg.scene_grids)
  for s, (h, w) in enumerate(cfg.scene_grids):
    c.grid_h[s], c.grid_w[s] = int(h), int(w)
    c.use_grid[s] = 1 if cfg.use_grids[s] else 0
  c.use_gnn = 1 if cfg.use_gnn else 0
  c.beam_size = int(cfg.beam_size) if getattr(cfg, "use_beam_search", False) else 1
  c.diverse_beam = 1 if getattr(cfg, "diverse_beam", False) else 0
  c.diverse_gamma = float(getattr(cfg, "diverse_gamma", 1.0))
  c.fix_num_timestep = int(getattr(cfg, "fix_num_timestep", 0))
  # --use_teacher_forcing at test time: the class decoder is fed its raw logits
  # (code/pred_models.py:388-406, the not-training arm of the teacher_forcing branch)
  c.class_feedback_dense = 1 if (getattr(cfg, "use_teacher_forcing", False) and
                                 not getattr(cfg, "is_train", False)) else 0
  c.use_single_decoder = 1 if getattr(cfg, "use_single_decoder", False) else 0
  c.simaug_graph = 1 if getattr(cfg, "simaug_graph", False) else 0
  c.activation = activation_code(getattr(cfg, "activation_func", "tanh"))
  return c


def soft_grid_kernel(soft_grid):
  """The `--soft_grid` stamp of Model.get_feed_dict (code/pred_models.py:1084-1120)."""
  table = {1: (0.1, 1.0), 2: (0.01, 1.0), 3: (0.05, 1.0), 4: (0.0125, 0.9),
           5: (0.05, 0.6), 6: (0.1, 0.2)}
  if soft_grid == 7:
    k = np.full((5, 5), 0.0625)
    k[1:4, 1:4] = 0.0125
    k[2, 2] = 0.8
    return k
  if soft_grid not in table:
    raise MvError("soft_grid %r not in 1..7" % (soft_grid,))
  ring, centre = table[soft_grid]
  k = np.full((3, 3), ring)
  k[1, 1] = centre
  return k


def make_train_config(cfg, world=1):
  """Trainer.__init__ / Model.build_loss fields of the config
  (reference code/pred_models.py:1636-1717, 961-1040) -> mv_train_config.
  `world`: data-parallel ranks.  cfg.batch_size is the PER-RANK batch; the schedules
  count optimizer steps over the global batch (batch_size * world), as a single-GPU
  run of the reference with that batch size would."""
  kinds = {"adadelta": 0, "momentum": 1, "adam": 2, "rmsprop": 3}
  if cfg.optimizer not in kinds:
    raise MvError("Optimizer not implemented: %r" % (cfg.optimizer,))   # pred_models.py:1681
  if not (0.0 < float(cfg.keep_prob) <= 1.0):
    raise MvError("keep_prob %r not in (0, 1]" % (cfg.keep_prob,))
  t = mv_train_config()
  t.optimizer = kinds[cfg.optimizer]
  tf_mode = bool(getattr(cfg, "use_teacher_forcing", False))
  # decoder_loop_fn (code/pred_models.py:388-436): teacher forcing wins over
  # input_onehot = not is_train or train_w_onehot (:285)
  t.class_feedback = 2 if tf_mode else (0 if cfg.train_w_onehot else 1)
  t.reg_teacher_forcing = 1 if tf_mode else 0
  t.use_soft_grid_class = 1 if getattr(cfg, "use_soft_grid_class", False) else 0
  k = soft_grid_kernel(int(getattr(cfg, "soft_grid", 1))) if t.use_soft_grid_class \
      else np.zeros((3, 3))
  t.soft_kernel_size = int(k.shape[0])
  for i, v in enumerate(np.asarray(k, dtype=np.float64).reshape(-1)):
    t.soft_kernel[i] = float(v)
  t.mask_grid_regression = 1 if getattr(cfg, "mask_grid_regression", False) else 0
  t.keep_prob = float(cfg.keep_prob)
  t.init_lr = float(cfg.init_lr)
  t.emb_lr = float(cfg.emb_lr)
  t.use_cosine_lr = 1 if getattr(cfg, "use_cosine_lr", False) else 0
  t.has_decay = 0 if cfg.learning_rate_decay is None else 1
  t.learning_rate_decay = float(cfg.learning_rate_decay or 1.0)
  gbatch = cfg.batch_size * max(1, int(world))
  t.decay_steps = int(cfg.train_num_examples / gbatch * cfg.num_epoch_per_decay)
  t.max_steps = int(cfg.train_num_examples / gbatch * cfg.num_epochs)
  t.do_clip = 0 if cfg.clip_gradient_norm is None else 1
  t.clip_gradient_norm = float(cfg.clip_gradient_norm or 0.0)
  t.wd = float(cfg.wd or 0.0)
  t.grid_loss_weight = float(cfg.grid_loss_weight)
  t.grid_reg_loss_weight = float(cfg.grid_reg_loss_weight)
  return t


MV_COMM_ID_BYTES = 128


def comm_unique_id():
  """128-byte RCCL unique id (rank 0 draws it, every rank passes it to comm_init)."""
  buf = (C.c_uint8 * MV_COMM_ID_BYTES)()
  check(load().mv_comm_unique_id(buf))
  return bytes(buf)


class Engine(object):
  """Owns one mv_handle."""

  def __init__(self, cfg, device=0):
    self.lib = load()
    self.cfg = cfg
    self.c_cfg = make_config(cfg)
    self.handle = C.c_void_p()
    rc = self.lib.mv_create(C.byref(self.c_cfg), int(device), C.byref(self.handle))
    if rc != 0:
      msg = self.lib.mv_last_error(None)
      self.handle = None
      raise MvError(msg.decode("utf-8", "replace"))
    self._keep = []

  def close(self):
    if getattr(self, "handle", None):
      self.lib.mv_destroy(self.handle)
      self.handle = None

  def __del__(self):
    try:
      self.close()
    except Exception:  # pylint: disable=broad-except
      pass

  # ---- weights
  def param_specs(self):
    out = []
    name = C.create_string_buffer(512)
    shape = (C.c_int64 * 4)()
    for i in range(self.lib.mv_num_params(self.handle)):
      rank = self.lib.mv_param_info(self.handle, i, name, 512, shape)
      out.append((name.value.decode(), tuple(int(shape[d]) for d in range(rank))))
    return out

  def set_param(self, name, value):
    a = f32(value)
    shape = (C.c_int64 * max(a.ndim, 1))(*a.shape)
    check(self.lib.mv_set_param(self.handle, name.encode(), fptr(a), shape, a.ndim),
          self.handle)

  def set_params(self, params):
    for name, _ in self.param_specs():
      if name not in params:
        raise MvError("missing parameter %s" % name)
      self.set_param(name, params[name])

  def get_param(self, name):
    shape = dict(self.param_specs())[name]
    out = np.empty(shape, dtype=np.float32)
    check(self.lib.mv_get_param(self.handle, name.encode(), fptr(out), out.size),
          self.handle)
    return out

  # ---- inputs / outputs
  def _inputs(self, feed):
    cfg = self.cfg
    N, T = cfg.batch_size, cfg.obs_len
    inp = mv_inputs()
    keep = []
    if uses_scene(cfg):
      obs_scene = i32(feed["obs_scene"]).reshape(N, T)
      scene_feat = f32(feed["scene_feat"])
      keep += [obs_scene, scene_feat]
      inp.obs_scene = iptr(obs_scene)
      inp.scene_feat = fptr(scene_feat)
      inp.num_scene_frames = int(scene_feat.shape[0])
      self._num_frames = int(scene_feat.shape[0])
    else:     # no scene encoder: nothing reads the scene arrays, none is handed over
      inp.num_scene_frames = 0
      self._num_frames = 0
    inp.pred_len = int(feed.get("pred_length", cfg.pred_len))
    for s, (h, w) in enumerate(cfg.scene_grids):
      if not cfg.use_grids[s]:
        continue
      lab = i32(feed["grid_obs_labels"][s]).reshape(N, T)
      reg = f32(feed["grid_obs_regress"][s]).reshape(N, T, h, w, 2)
      keep += [lab, reg]
      inp.grid_obs_labels[s] = iptr(lab)
      inp.grid_obs_regress[s] = fptr(reg)
    self._keep = keep
    self._pred_len = inp.pred_len
    self._set_pred_lengths(feed.get("pred_lengths"))
    self._set_obs_lengths(feed.get("obs_lengths"))
    self._set_feed_cell_mask(feed.get("cell_mask"))
    self._set_feed_cell_bias(feed.get("cell_bias"))
    self._set_feed_motion_cost(feed.get("motion_cost"))
    self._set_feed_revisit_cost(feed.get("revisit_cost"))
    return inp

  def _set_pred_lengths(self, lengths):
    """Per-row prediction lengths of the next forward (feed["pred_lengths"], int [N]); None
    clears the ones a previous feed set.  Called with every feed that is uploaded."""
    if lengths is None:
      if getattr(self, "_lengths_set", False):
        check(self.lib.mv_set_pred_lengths(self.handle, None), self.handle)
        self._lengths_set = False
      return
    lens = i32(lengths).reshape(-1)
    if lens.size != self.cfg.batch_size:
      raise MvError("pred_lengths: %d values for batch_size %d" % (lens.size, self.cfg.batch_size))
    check(self.lib.mv_set_pred_lengths(self.handle, iptr(lens)), self.handle)
    self._lengths_set = True

  def _set_obs_lengths(self, lengths):
    """Per-row observation lengths of the next forward (feed["obs_lengths"], int [N], the
    observations right-aligned; include/multiverse_hip.h mv_set_obs_lengths); None clears the
    ones a previous feed set.  Called with every feed that is uploaded."""
    if lengths is None:
      if getattr(self, "_obs_lengths_set", False):
        check(self.lib.mv_set_obs_lengths(self.handle, None), self.handle)
        self._obs_lengths_set = False
      return
    lens = i32(lengths).reshape(-1)
    if lens.size != self.cfg.batch_size:
      raise MvError("obs_lengths: %d values for batch_size %d" % (lens.size, self.cfg.batch_size))
    check(self.lib.mv_set_obs_lengths(self.handle, iptr(lens)), self.handle)
    self._obs_lengths_set = True

  def set_cell_mask(self, mask):
    """The cells the futures of each row may choose (include/multiverse_hip.h mv_set_cell_mask):
    [N, K] (one mask for every decode step) or [N, Tm, K] (plane t for step t, Tm >= pred_len),
    non-zero = allowed; a grid-shaped [N, (Tm,) h, w] is taken as well.  None clears.  Sticky:
    a mask set here stays through every later feed that has no "cell_mask" key, until it is
    cleared here or a feed brings its own (which then follows the feeds' rule: the next feed
    without the key clears it).  The beam search, both samplers and beam_occupancy read it,
    score_futures does not.  While sampling is on under a mask, the forwards add
    "proposal_logprobs"."""
    self._cell_mask_from_feed = False
    if mask is None:
      check(self.lib.mv_set_cell_mask(self.handle, None, 0), self.handle)
      self._cell_mask_set = False
      return
    N = self.cfg.batch_size
    h, w = self.cfg.scene_grids[self._beam_scale()]
    m = np.asarray(mask)
    if m.ndim >= 2 and m.shape[-2:] == (h, w) and m.shape[-1] != h * w:
      m = m.reshape(m.shape[:-2] + (h * w,))
    if m.ndim == 2:
      m = m[:, None, :]
    if m.ndim != 3 or m.shape[0] != N or m.shape[2] != h * w:
      raise MvError("cell_mask: shape %s is neither [N=%d, K=%d] nor [N, Tm, K]"
                    % (tuple(np.asarray(mask).shape), N, h * w))
    m = np.ascontiguousarray(m != 0, dtype=np.uint8)
    check(self.lib.mv_set_cell_mask(self.handle, m.ctypes.data_as(_u8p), int(m.shape[1])),
          self.handle)
    self._cell_mask_set = True

  def _set_feed_cell_mask(self, mask):
    """feed["cell_mask"], handled as feed["obs_lengths"] is: set when present; a feed without
    the key clears the mask a previous FEED set, and leaves one set through set_cell_mask alone.
    Called with every feed that is uploaded."""
    if mask is None:
      if getattr(self, "_cell_mask_from_feed", False):
        self.set_cell_mask(None)
      return
    self.set_cell_mask(mask)
    self._cell_mask_from_feed = True

  def set_cell_bias(self, bias):
    """A float32 log-potential per row, decode step and cell, added to the choice of cells
    (include/multiverse_hip.h mv_set_cell_bias): [N, K] (one plane for every decode step) or
    [N, Tm, K] (plane t for step t, Tm >= pred_len), in nats, negative = less likely, every value
    finite; a grid-shaped [N, (Tm,) h, w] is taken as well.  None clears.  Sticky, with the rule
    of set_cell_mask: a bias set here stays through every later feed that has no "cell_bias"
    key; one that a feed brought is cleared by the next feed without the key.  The beam search,
    both samplers and beam_occupancy read it, score_futures does not.  While sampling is on
    under a bias, the forwards add "proposal_logprobs"."""
    self._cell_bias_from_feed = False
    if bias is None:
      check(self.lib.mv_set_cell_bias(self.handle, None, 0), self.handle)
      self._cell_bias_set = False
      return
    N = self.cfg.batch_size
    h, w = self.cfg.scene_grids[self._beam_scale()]
    b = np.asarray(bias)
    if b.ndim >= 2 and b.shape[-2:] == (h, w) and b.shape[-1] != h * w:
      b = b.reshape(b.shape[:-2] + (h * w,))
    if b.ndim == 2:
      b = b[:, None, :]
    if b.ndim != 3 or b.shape[0] != N or b.shape[2] != h * w:
      raise MvError("cell_bias: shape %s is neither [N=%d, K=%d] nor [N, Tm, K]"
                    % (tuple(np.asarray(bias).shape), N, h * w))
    b = f32(b)
    check(self.lib.mv_set_cell_bias(self.handle, fptr(b), int(b.shape[1])), self.handle)
    self._cell_bias_set = True

  def _set_feed_cell_bias(self, bias):
    """feed["cell_bias"], with the feed-scoped rule of feed["cell_mask"]."""
    if bias is None:
      if getattr(self, "_cell_bias_from_feed", False):
        self.set_cell_bias(None)
      return
    self.set_cell_bias(bias)
    self._cell_bias_from_feed = True

  def set_motion_cost(self, radius, vel=None, vel_far=None, acc=None, acc_far=None):
    """Per-row speed and turn priors of a multi-future decode (include/multiverse_hip.h
    mv_set_motion_cost): what a step costs by how far it moves from the path's last cell
    (vel [N, D, D], vel_far [N]; D = 2 * radius + 1) and by how much that move differs from the
    move before it (acc [N, D, D], acc_far [N]; both or neither).  Tables of one row ([D, D] and a
    scalar) are taken for every row; `multifuture.motion_tables` builds them.  Every value finite;
    a limit is the cost -1e30.  vel None (or radius None) clears.  Sticky, with the rule of
    set_cell_bias: a cost set here stays through every later feed that has no "motion_cost" key;
    one that a feed brought is cleared by the next feed without the key.  The beam search and both
    samplers read it; score_futures does not, and beam_occupancy refuses while one is set."""
    self._motion_cost_from_feed = False
    if vel is None or radius is None:
      check(self.lib.mv_set_motion_cost(self.handle, 0, None, None, None, None), self.handle)
      self._motion_cost_set = False
      return
    if (acc is None) != (acc_far is None):
      raise MvError("motion_cost: acc and acc_far are given both or neither")
    N, D = self.cfg.batch_size, 2 * int(radius) + 1

    def table(a, name):
      a = np.asarray(a, dtype=np.float32)
      if a.shape == (D, D):
        a = np.broadcast_to(a, (N, D, D))
      if a.shape != (N, D, D):
        raise MvError("motion_cost: %s has shape %s, not [N=%d, D=%d, D] (radius %d)"
                      % (name, tuple(a.shape), N, D, int(radius)))
      return f32(a)

    def far(a, name):
      a = np.asarray(a, dtype=np.float32)
      if a.ndim == 0:
        a = np.broadcast_to(a, (N,))
      if a.shape != (N,):
        raise MvError("motion_cost: %s has shape %s, not [N=%d]" % (name, tuple(a.shape), N))
      return f32(a)

    if not 1 <= int(radius) <= MV_MOTION_MAX_RADIUS:
      raise MvError("motion_cost: radius = %d not in [1, %d]" % (int(radius), MV_MOTION_MAX_RADIUS))
    v, vf = table(vel, "vel"), far(vel_far, "vel_far")
    a = table(acc, "acc") if acc is not None else None
    af = far(acc_far, "acc_far") if acc is not None else None
    check(self.lib.mv_set_motion_cost(self.handle, int(radius), fptr(v), fptr(vf),
                                      fptr(a) if a is not None else None,
                                      fptr(af) if af is not None else None), self.handle)
    self._motion_cost_set = True

  def _set_feed_motion_cost(self, cost):
    """feed["motion_cost"]: the dict of `multifuture.motion_tables` (radius, vel, vel_far and,
    optionally, acc, acc_far), with the feed-scoped rule of feed["cell_bias"]."""
    if cost is None:
      if getattr(self, "_motion_cost_from_feed", False):
        self.set_motion_cost(None)
      return
    self.set_motion_cost(cost["radius"], cost["vel"], cost["vel_far"], cost.get("acc"),
                         cost.get("acc_far"))
    self._motion_cost_from_feed = True

  def set_revisit_cost(self, cost, seed_observed=True):
    """A per-row penalty for paths that return to a cell they left (include/multiverse_hip.h
    mv_set_revisit_cost): a step into a cell the row's path (and, with seed_observed, its observed
    track) has held before, other than the one it is in, pays cost[n].  cost float32 [N], or a
    scalar taken for every row; every value finite, "never" is the cost -1e30
    (multifuture.MOTION_LIMIT); None clears.  Sticky, with the rule of set_motion_cost: a cost set
    here stays through every later feed that has no "revisit_cost" key; one that a feed brought is
    cleared by the next feed without the key.  The beam search and both samplers read it;
    score_futures does not, and beam_occupancy refuses while one is set."""
    self._revisit_cost_from_feed = False
    if cost is None:
      check(self.lib.mv_set_revisit_cost(self.handle, None, 0), self.handle)
      self._revisit_cost_set = False
      return
    N = self.cfg.batch_size
    c = np.asarray(cost, dtype=np.float32)
    if c.ndim == 0:
      c = np.broadcast_to(c, (N,))
    if c.shape != (N,):
      raise MvError("revisit_cost: cost has shape %s, not [N=%d]" % (tuple(c.shape), N))
    c = f32(c)
    check(self.lib.mv_set_revisit_cost(self.handle, fptr(c), 1 if seed_observed else 0),
          self.handle)
    self._revisit_cost_set = True

  def _set_feed_revisit_cost(self, cost):
    """feed["revisit_cost"]: {"cost": [N] or a scalar, "seed_observed": bool (default True)},
    with the feed-scoped rule of feed["motion_cost"]."""
    if cost is None:
      if getattr(self, "_revisit_cost_from_feed", False):
        self.set_revisit_cost(None)
      return
    self.set_revisit_cost(cost["cost"], cost.get("seed_observed", True))
    self._revisit_cost_from_feed = True

  def graph_captures(self):
    """Forwards captured into a hipGraph on this handle so far (a replay does not count)."""
    n = C.c_int64()
    check(self.lib.mv_graph_captures(self.handle, C.byref(n)), self.handle)
    return int(n.value)

  def set_sampling(self, temperature=1.0, seed=0, without_replacement=False, top_k=0,
                   top_p=1.0):
    """The beam_size futures of every row are SAMPLED (Gumbel-max over the step's
    log-softmax / temperature; include/multiverse_hip.h mv_set_sampling) by forward_beam and
    the calls around it, until clear_sampling().  without_replacement: the futures of a row are
    DISTINCT, a sample without replacement (stochastic beam search; mv_set_sampling_mode),
    and forward_beam / forward_beam_decoded add their perturbed scores as "gumbels".
    top_k (0 = off) / top_p (1 = off): the step distribution is cut to its top_k best cells /
    its smallest head of mass top_p and renormalised (mv_set_sampling_truncation); while a
    limit is on, the forwards add the futures' log-probability under that proposal as
    "proposal_logprobs" (logprobs stays the model's own)."""
    if (int(top_k), float(top_p)) != getattr(self, "_sampling_limits", (0, 1.0)):
      self.set_sampling_truncation(top_k, top_p)
    mode = 1 if without_replacement else 0
    if mode != getattr(self, "_sampling_mode", 0):
      check(self.lib.mv_set_sampling_mode(self.handle, mode), self.handle)
      self._sampling_mode = mode
    check(self.lib.mv_set_sampling(self.handle, 1, float(temperature),
                                   int(seed) & 0xFFFFFFFF), self.handle)
    self._sampling_on = True

  def clear_sampling(self):
    check(self.lib.mv_set_sampling(self.handle, 0, 1.0, 0), self.handle)
    self._sampling_on = False

  def set_sampling_truncation(self, top_k=0, top_p=1.0):
    """The top-k / nucleus limits of the sampled decode (mv_set_sampling_truncation): sticky,
    stored while sampling is off, followed by a replayed graph.  (0, 1.0) = off."""
    check(self.lib.mv_set_sampling_truncation(self.handle, int(top_k), float(top_p)),
          self.handle)
    self._sampling_limits = (int(top_k), float(top_p))

  def _truncated(self):
    """Does the next / did the last beam forward sample under a top-k / nucleus limit, a cell
    mask or a cell bias, i.e. from a proposal that is not the (tempered) model?"""
    top_k, top_p = getattr(self, "_sampling_limits", (0, 1.0))
    return getattr(self, "_sampling_on", False) and \
        (top_k > 0 or top_p < 1.0 or getattr(self, "_cell_mask_set", False) or
         getattr(self, "_cell_bias_set", False) or getattr(self, "_motion_cost_set", False) or
         getattr(self, "_revisit_cost_set", False))

  def beam_proposal_logprobs(self):
    """float32 [N, B]: the log-probability of each future of the last SAMPLED forward under the
    proposal it was drawn from -- the tempered, truncated step distribution -- where logprobs
    is the model's own (multifuture.proposal_importance_weights turns the two into weights)."""
    c = self.c_cfg
    q = np.empty((c.batch_size, c.beam_size), dtype=np.float32)
    check(self.lib.mv_download_beam_proposal_logprobs(self.handle, fptr(q)), self.handle)
    return q

  def _without_replacement(self):
    """Does the next / did the last beam forward sample without replacement?"""
    return getattr(self, "_sampling_on", False) and getattr(self, "_sampling_mode", 0) == 1

  def beam_gumbels(self):
    """float32 [N, B]: the perturbed scores G of the last forward that sampled without
    replacement -- non-increasing along B, gumbels[:, 0] == 0 (multifuture.
    wor_importance_weights turns them and the logprobs into importance weights)."""
    c = self.c_cfg
    g = np.empty((c.batch_size, c.beam_size), dtype=np.float32)
    check(self.lib.mv_download_beam_gumbels(self.handle, fptr(g)), self.handle)
    return g

  # ---- scoring given futures (include/multiverse_hip.h mv_score_futures)
  def _score_futures_in(self, ids, lengths):
    N, F, Tp = self.cfg.batch_size, self.cfg.beam_size, self._pred_len
    ids = i32(ids)
    if ids.size != N * F * Tp:
      raise MvError("score futures: ids of shape %s, expected [N=%d, F=%d, pred_len=%d]"
                    % (ids.shape, N, F, Tp))
    fut = mv_score_futures_in()
    fut.ids = iptr(ids)
    keep = [ids]
    if lengths is not None:
      lens = i32(lengths).reshape(-1)
      if lens.size != N * F:
        raise MvError("score futures: %d lengths, expected [N=%d, F=%d]" % (lens.size, N, F))
      fut.lengths = iptr(lens)
      keep.append(lens)
    return fut, keep

  def _alloc_scores(self):
    N, F, Tp = self.cfg.batch_size, self.cfg.beam_size, self._pred_len
    arrs = {"step_logprobs": np.empty((N, F, Tp), dtype=np.float32),
            "logprobs": np.empty((N, F), dtype=np.float32),
            "ranks": np.empty((N, F, Tp), dtype=np.int32)}
    out = mv_score_outputs()
    out.step_logprobs = fptr(arrs["step_logprobs"])
    out.logprobs = fptr(arrs["logprobs"])
    out.ranks = iptr(arrs["ranks"])
    return out, arrs

  def score_futures(self, feed, ids, lengths=None):
    """Teacher-forced log-likelihood of F = beam_size GIVEN futures per row: ids int
    [N, F, pred_len] grid cells, lengths int [N, F] in [0, pred_len] (None: all pred_len) ->
    {"step_logprobs" float32 [N, F, T], "logprobs" float32 [N, F], "ranks" int32 [N, F, T]}.
    download_beam / beam_ids / decode_trajectories afterwards see the forward's logits, the
    given ids and the model's offsets along them."""
    inp = self._inputs(feed)
    fut, keep = self._score_futures_in(ids, lengths)
    out, arrs = self._alloc_scores()
    check(self.lib.mv_score_futures(self.handle, C.byref(inp), C.byref(fut), C.byref(out)),
          self.handle)
    del keep
    return arrs

  def upload_score_futures(self, ids, lengths=None):
    """After upload(feed): the futures the next run_score_resident scores."""
    fut, keep = self._score_futures_in(ids, lengths)
    check(self.lib.mv_upload_score_futures(self.handle, C.byref(fut)), self.handle)
    del keep      # copied synchronously

  def run_score_resident(self):
    check(self.lib.mv_run_score_resident(self.handle), self.handle)

  def scores(self):
    """The outputs of the last scoring forward (see score_futures)."""
    out, arrs = self._alloc_scores()
    check(self.lib.mv_download_scores(self.handle, C.byref(out)), self.handle)
    return arrs

  def time_score_resident(self, iters):
    ms = C.c_float()
    check(self.lib.mv_time_score_resident(self.handle, int(iters), C.byref(ms)), self.handle)
    return float(ms.value)

  def last_forward_gate_rows(self):
    """Rows of every ConvLSTM problem of every gate launch of the last forward, summed."""
    rows = C.c_int64()
    check(self.lib.mv_last_forward_gate_rows(self.handle, C.byref(rows)), self.handle)
    return int(rows.value)

  def _alloc_outputs(self, Tp):
    cfg = self.cfg
    N = cfg.batch_size
    out = mv_outputs()
    cls, reg = [], []
    for s, (h, w) in enumerate(cfg.scene_grids):
      if not cfg.use_grids[s]:
        cls.append([])
        reg.append([])
        continue
      a = np.empty((N, Tp, h, w, 1), dtype=np.float32)
      b = np.empty((N, Tp, h, w, 2), dtype=np.float32)
      out.grid_pred_class[s] = fptr(a)
      out.grid_pred_reg[s] = fptr(b)
      cls.append(a)
      reg.append(b)
    return out, cls, reg

  def _alloc_beam(self, Tp):
    cfg = self.cfg
    N, B = cfg.batch_size, cfg.beam_size
    s = [i for i, u in enumerate(cfg.use_grids) if u][0]
    h, w = cfg.scene_grids[s]
    out = mv_beam_outputs()
    arrs = {
        "best_beam": np.empty((N, Tp, h, w, 1), dtype=np.float32),
        # --use_single_decoder: per beam, [N*B, T, h, w, 2] (code/pred_models.py:287-296)
        "grid_reg": np.empty((N * B if getattr(cfg, "use_single_decoder", False) else N,
                              Tp, h, w, 2), dtype=np.float32),
        "logits": np.empty((N, B, Tp, h * w), dtype=np.float32),
        "ids": np.empty((N, B, Tp), dtype=np.int32),
        "logprobs": np.empty((N, B), dtype=np.float32),
    }
    out.best_beam = fptr(arrs["best_beam"])
    out.grid_reg = fptr(arrs["grid_reg"])
    out.logits = fptr(arrs["logits"])
    out.ids = iptr(arrs["ids"])
    out.logprobs = fptr(arrs["logprobs"])
    return out, arrs, s

  def forward_greedy(self, feed):
    inp = self._inputs(feed)
    out, cls, reg = self._alloc_outputs(inp.pred_len)
    check(self.lib.mv_forward_greedy(self.handle, C.byref(inp), C.byref(out)),
          self.handle)
    return cls, reg

  def forward_beam(self, feed):
    inp = self._inputs(feed)
    out, arrs, s = self._alloc_beam(inp.pred_len)
    check(self.lib.mv_forward_beam(self.handle, C.byref(inp), C.byref(out)),
          self.handle)
    if self._without_replacement():
      arrs["gumbels"] = self.beam_gumbels()
    if self._truncated():
      arrs["proposal_logprobs"] = self.beam_proposal_logprobs()
    return arrs, s

  # ---- resident-input path (bench)
  def upload(self, feed):
    inp = self._inputs(feed)
    self._pred_len = inp.pred_len
    check(self.lib.mv_upload_inputs(self.handle, C.byref(inp)), self.handle)

  # ---- compact inputs (device-side batch assembly)
  def set_grid_centers(self, centers):
    """centers: list over scales of float64 [H, W, 2] (data["grid_center_<s>"])."""
    sent = []
    for s, (h, w) in enumerate(self.cfg.scene_grids):
      if not self.cfg.use_grids[s]:
        sent.append(None)
        continue
      c = np.ascontiguousarray(np.asarray(centers[s], dtype=np.float64).reshape(h, w, 2))
      check(self.lib.mv_set_grid_centers(self.handle, s, c.ctypes.data_as(_dp)),
            self.handle)
      sent.append(c.copy())
    self._centers_sent = sent

  def _centers_current(self, centers):
    """Are the centres resident in the engine the ones of this feed?  (A second
    dataset -- val after train -- may carry different grid centres.)"""
    sent = getattr(self, "_centers_sent", None)
    if sent is None:
      return False
    for s, (h, w) in enumerate(self.cfg.scene_grids):
      if not self.cfg.use_grids[s]:
        continue
      c = np.asarray(centers[s], dtype=np.float64).reshape(h, w, 2)
      if sent[s] is None or not np.array_equal(sent[s], c):
        return False
    return True

  def upload_compact(self, feed):
    """feed: obs_scene, scene_feat (0/1, any dtype), grid_obs_labels, obs_xy
    [N, T_o, 2], optional num_rows, pred_length; with grid_pred_labels + pred_xy
    also the training targets (after train_init)."""
    cfg = self.cfg
    N, T = cfg.batch_size, cfg.obs_len
    if not self._centers_current(feed["grid_centers"]):
      self.set_grid_centers(feed["grid_centers"])
    inp = mv_inputs_compact()
    xy = np.ascontiguousarray(np.asarray(feed["obs_xy"], dtype=np.float64).reshape(N, T, 2))
    keep = [xy]
    if uses_scene(cfg):
      scene_any = np.asarray(feed["scene_feat"])
      if scene_any.dtype != np.uint8 and not ((scene_any == 0) | (scene_any == 1)).all():
        raise MvError("upload_compact: scene_feat must be 0/1 masks (it is handed over as "
                      "uint8); use the dense upload for real-valued scene features")
      obs_scene = i32(feed["obs_scene"]).reshape(N, T)
      scene = np.ascontiguousarray(np.asarray(feed["scene_feat"]).astype(np.uint8, copy=False))
      keep += [obs_scene, scene]
      inp.obs_scene = iptr(obs_scene)
      inp.scene_feat_u8 = scene.ctypes.data_as(_u8p)
      inp.num_scene_frames = int(scene.shape[0])
    else:
      inp.num_scene_frames = 0
    inp.pred_len = int(feed.get("pred_length", cfg.pred_len))
    inp.obs_xy = xy.ctypes.data_as(_dp)
    inp.num_rows = int(feed.get("num_rows", N))
    for s in range(len(cfg.scene_grids)):
      if not cfg.use_grids[s]:
        continue
      lab = i32(feed["grid_obs_labels"][s]).reshape(N, T)
      keep.append(lab)
      inp.grid_obs_labels[s] = iptr(lab)
    self._pred_len = inp.pred_len
    self._set_pred_lengths(feed.get("pred_lengths"))
    self._set_obs_lengths(feed.get("obs_lengths"))
    self._set_feed_cell_mask(feed.get("cell_mask"))
    self._set_feed_cell_bias(feed.get("cell_bias"))
    self._set_feed_motion_cost(feed.get("motion_cost"))
    self._set_feed_revisit_cost(feed.get("revisit_cost"))
    check(self.lib.mv_upload_inputs_compact(self.handle, C.byref(inp)), self.handle)
    if feed.get("pred_xy") is not None and getattr(self, "_tc", None) is not None:
      Tp = inp.pred_len
      tg = mv_targets_compact()
      pxy = np.ascontiguousarray(
          np.asarray(feed["pred_xy"], dtype=np.float64).reshape(N, -1, 2)[:, :Tp])
      keep.append(pxy)
      tg.pred_xy = pxy.ctypes.data_as(_dp)
      tg.num_rows = inp.num_rows
      for s in range(len(cfg.scene_grids)):
        if not cfg.use_grids[s]:
          continue
        lab = i32(feed["grid_pred_labels"][s]).reshape(N, Tp)
        keep.append(lab)
        tg.grid_pred_labels[s] = iptr(lab)
      check(self.lib.mv_upload_targets_compact(self.handle, C.byref(tg)), self.handle)
      self._set_feed_train_lengths(feed.get("train_obs_lengths"),
                                   feed.get("train_pred_lengths"))
    del keep      # both calls copy synchronously

  # ---- pipelined greedy forward: feed of batch k+1 / fetch of batch k-1 under batch k
  def submit_greedy(self, feed, depth=2):
    """Queue one batch (H2D -> forward -> D2H on the engine's streams) and return; the
    caller's arrays are free again on return.  At most `depth` batches outstanding."""
    if not getattr(self, "_pipe_depth", 0):
      check(self.lib.mv_pipeline_create(self.handle, int(depth)), self.handle)
      self._pipe_depth = int(depth)
    inp = self._inputs(feed)
    check(self.lib.mv_submit_greedy(self.handle, C.byref(inp)), self.handle)
    self._pipe_lens = getattr(self, "_pipe_lens", []) + [inp.pred_len]

  def collect_greedy(self):
    """-> (cls, reg) of the OLDEST submitted batch (blocks until it is on the host)."""
    Tp = self._pipe_lens.pop(0)
    out, cls, reg = self._alloc_outputs(Tp)
    check(self.lib.mv_collect_greedy(self.handle, C.byref(out), None), self.handle)
    return cls, reg

  def forward_greedy_pipelined(self, feeds, depth=2):
    """[(cls, reg)] of a sequence of batches, bitwise those of forward_greedy on each; batch
    k+1 is submitted before batch k is collected."""
    feeds = list(feeds)
    outs = []
    for k, feed in enumerate(feeds):
      if k >= depth:
        outs.append(self.collect_greedy())
      self.submit_greedy(feed, depth)
    while len(outs) < len(feeds):
      outs.append(self.collect_greedy())
    return outs

  def forward_greedy_compact(self, feed):
    self.upload_compact(feed)
    self.run_resident(False)
    return self.download()

  def forward_beam_compact(self, feed):
    self.upload_compact(feed)
    self.run_resident(True)
    return self.download_beam()

  def train_step_compact(self, feed):
    self.upload_compact(feed)
    return self.train_step(None)

  def run_resident(self, beam=False):
    fn = self.lib.mv_run_beam_resident if beam else self.lib.mv_run_greedy_resident
    check(fn(self.handle), self.handle)

  def synchronize(self):
    check(self.lib.mv_synchronize(self.handle), self.handle)

  def time_resident(self, iters, beam=False):
    ms = C.c_float()
    fn = self.lib.mv_time_beam_resident if beam else self.lib.mv_time_greedy_resident
    check(fn(self.handle, int(iters), C.byref(ms)), self.handle)
    return float(ms.value)

  def download(self):
    out, cls, reg = self._alloc_outputs(self._pred_len)
    check(self.lib.mv_download_outputs(self.handle, C.byref(out)), self.handle)
    return cls, reg

  def download_beam(self):
    out, arrs, s = self._alloc_beam(self._pred_len)
    check(self.lib.mv_download_beam_outputs(self.handle, C.byref(out)), self.handle)
    return arrs, s

  # ---- multi-future decode of the last forward, on the device (csrc/multifuture_decode.h)
  def _beam_scale(self):
    return [i for i, u in enumerate(self.cfg.use_grids) if u][0]

  def _last_pred_len(self):
    return int(getattr(self, "_pred_len", self.cfg.pred_len))

  def decode_trajectories(self, scale=None, center_only=False):
    """Pixel trajectories of the last forward -> float64 [N, B, T_pred, 2] (B = beam_size,
    1 for a greedy engine, whose `scale` picks the grid): centre of the decoded cell plus
    its offset, bit-identical to multifuture.decode_trajectories on the downloaded outputs.
    Needs set_grid_centers."""
    c = self.c_cfg
    if scale is None:
      scale = self._beam_scale()
    Tp = self._last_pred_len()
    buf = np.empty(c.batch_size * c.beam_size * max(c.max_pred_len, Tp) * 2, dtype=np.float64)
    check(self.lib.mv_decode_trajectories(self.handle, int(scale), 1 if center_only else 0,
                                          buf.ctypes.data_as(_dp)), self.handle)
    return buf[:c.batch_size * c.beam_size * Tp * 2].reshape(c.batch_size, c.beam_size, Tp, 2)

  def beam_occupancy(self):
    """Occupancy map of the last beam decode -> float32 [N, T_pred, K]: every beam's
    per-step softmax over the grid, mixed with softmax(beam log-probabilities) -- the map
    multifuture.eval_grid_nll builds from the downloaded logits."""
    c = self.c_cfg
    h, w = self.cfg.scene_grids[self._beam_scale()]
    Tp = self._last_pred_len()
    buf = np.empty(c.batch_size * max(c.max_pred_len, Tp) * h * w, dtype=np.float32)
    check(self.lib.mv_beam_occupancy(self.handle, fptr(buf)), self.handle)
    return buf[:c.batch_size * Tp * h * w].reshape(c.batch_size, Tp, h * w)

  def beam_ids(self):
    """(ids int32 [N, B, T_pred], logprobs float32 [N, B]) of the last beam decode -- the
    small members of download_beam, without its logits / best_beam / offsets."""
    c = self.c_cfg
    Tp = self._last_pred_len()
    ids = np.empty(c.batch_size * c.beam_size * max(c.max_pred_len, Tp), dtype=np.int32)
    lp = np.empty((c.batch_size, c.beam_size), dtype=np.float32)
    check(self.lib.mv_download_beam_ids(self.handle, iptr(ids), fptr(lp)), self.handle)
    return ids[:c.batch_size * c.beam_size * Tp].reshape(c.batch_size, c.beam_size, Tp), lp

  def forward_beam_decoded(self, feed, center_only=False, occupancy=False, logits=False):
    """One beam decode whose fetch is what a caller uses: upload (the compact form when
    feed["compact"]), run_resident(beam=True), then {"trajs" float64 [N, B, T, 2], "ids"
    [N, B, T], "logprobs" [N, B][, "occupancy" float32 [N, T, K]]} -- every beam's logits,
    the offsets maps and best_beam stay in HBM (logits=True fetches "logits" [N, B, T, K] as
    well, for callers that store them).  The grid centres are those of set_grid_centers
    (feed["grid_centers"] when the feed carries them)."""
    if feed.get("compact", False):
      self.upload_compact(feed)
    else:
      if feed.get("grid_centers") is not None and \
          not self._centers_current(feed["grid_centers"]):
        self.set_grid_centers(feed["grid_centers"])
      self.upload(feed)
    self.run_resident(True)
    c = self.c_cfg
    Tp = self._last_pred_len()
    arrs = {"trajs": self.decode_trajectories(center_only=center_only)}
    arrs["ids"], arrs["logprobs"] = self.beam_ids()
    if self._without_replacement():
      arrs["gumbels"] = self.beam_gumbels()
    if self._truncated():
      arrs["proposal_logprobs"] = self.beam_proposal_logprobs()
    if occupancy:
      arrs["occupancy"] = self.beam_occupancy()
    if logits:
      arrs["logits"] = self.download_beam()[0]["logits"]
    return arrs, self._beam_scale()

  def forward_beam_decoded_compact(self, feed, center_only=False, occupancy=False,
                                   logits=False):
    return self.forward_beam_decoded(dict(feed, compact=True), center_only, occupancy, logits)

  # ---- training (Trainer.step)
  def train_init(self, cfg=None, world=None):
    """world None = the world of the previous train_init of this engine (1 for the first):
    re-initialising with another configuration (the SimAug attacks switch to their loss
    and back) must not reset the data-parallel LR / decay schedule to a single rank."""
    if world is None:
      world = getattr(self, "_train_world", 1)
    self._train_world = int(world)
    self._tc = make_train_config(cfg or self.cfg, world=world)
    check(self.lib.mv_train_init(self.handle, C.byref(self._tc)), self.handle)

  def _targets(self, feed):
    cfg = self.cfg
    N, Tp = cfg.batch_size, int(feed.get("pred_length", cfg.pred_len))
    tg = mv_targets()
    keep = []
    for s, (h, w) in enumerate(cfg.scene_grids):
      if not cfg.use_grids[s]:
        continue
      lab = i32(feed["grid_pred_labels"][s]).reshape(N, Tp)
      reg = f32(feed["grid_pred_regress"][s]).reshape(N, Tp, h, w, 2)
      keep += [lab, reg]
      tg.grid_pred_labels[s] = iptr(lab)
      tg.grid_pred_regress[s] = fptr(reg)
    self._keep_t = keep
    self._set_feed_train_lengths(feed.get("train_obs_lengths"), feed.get("train_pred_lengths"))
    return tg

  def _set_feed_train_lengths(self, obs_lengths, pred_lengths):
    """feed["train_obs_lengths"] / feed["train_pred_lengths"], handled as feed["obs_lengths"]
    is: set when present; a feed without them clears what an earlier FEED set.  Lengths set
    through set_train_lengths stay (sticky until set_train_lengths(None, None))."""
    if obs_lengths is None and pred_lengths is None:
      if getattr(self, "_feed_train_lengths", False):
        self.set_train_lengths(None, None)
        self._feed_train_lengths = False
      return
    self.set_train_lengths(obs_lengths, pred_lengths)
    self._feed_train_lengths = True

  def set_train_lengths(self, obs_lengths=None, pred_lengths=None):
    """Per-row lengths of the TRAINING step (include/multiverse_hip.h mv_set_train_lengths):
    obs_lengths int [N] in [1, obs_len] (observations right-aligned), pred_lengths int [N] in
    [0, pred_len] (targets left-aligned; 0 = padding row).  None = that side uniform; both None
    clears.  Sticky; read by train_step / train_forward_backward only."""
    arrs = []
    for name, lengths in (("train_obs_lengths", obs_lengths), ("train_pred_lengths", pred_lengths)):
      if lengths is None:
        arrs.append(None)
        continue
      lens = i32(lengths).reshape(-1)
      if lens.size != self.cfg.batch_size:
        raise MvError("%s: %d values for batch_size %d" % (name, lens.size, self.cfg.batch_size))
      arrs.append(lens)
    check(self.lib.mv_set_train_lengths(self.handle,
                                        iptr(arrs[0]) if arrs[0] is not None else None,
                                        iptr(arrs[1]) if arrs[1] is not None else None),
          self.handle)

  def last_train_gate_rows(self):
    """(forward_rows, dgrad_rows) of the last training step: the row counts summed over every
    ConvLSTM problem of its grouped gate launches / dgrad groups."""
    f, d = C.c_int64(), C.c_int64()
    check(self.lib.mv_last_train_gate_rows(self.handle, C.byref(f), C.byref(d)), self.handle)
    return int(f.value), int(d.value)

  @staticmethod
  def _losses(L):
    return (float(L.loss), float(L.wd_loss),
            [float(L.pred_grid_loss[i]) for i in range(L.num_pred_grid_loss)])

  def train_step(self, feed=None):
    """-> (loss, wd_loss, pred_grid_loss list); feed None = resident batch."""
    L = mv_losses()
    if feed is None:
      rc = self.lib.mv_train_step(self.handle, None, None, C.byref(L))
    else:
      inp, tg = self._inputs(feed), self._targets(feed)
      rc = self.lib.mv_train_step(self.handle, C.byref(inp), C.byref(tg), C.byref(L))
    check(rc, self.handle)
    return self._losses(L)

  def train_forward_backward(self, feed=None):
    L = mv_losses()
    if feed is None:
      rc = self.lib.mv_train_forward_backward(self.handle, None, None, C.byref(L))
    else:
      inp, tg = self._inputs(feed), self._targets(feed)
      rc = self.lib.mv_train_forward_backward(self.handle, C.byref(inp), C.byref(tg),
                                              C.byref(L))
    check(rc, self.handle)
    return self._losses(L)

  def upload_targets(self, feed):
    tg = self._targets(feed)
    check(self.lib.mv_upload_targets(self.handle, C.byref(tg)), self.handle)

  def train_apply(self, grad_scale=1.0):
    check(self.lib.mv_train_apply(self.handle, float(grad_scale)), self.handle)

  def grad_buffer(self):
    """(device pointer, element count) of the flat gradient buffer."""
    p, n = _fp(), C.c_int64()
    check(self.lib.mv_grad_buffer(self.handle, C.byref(p), C.byref(n)), self.handle)
    return C.cast(p, C.c_void_p).value, int(n.value)

  def get_grad(self, name):
    shape = dict(self.param_specs())[name]
    out = np.empty(shape, dtype=np.float32)
    check(self.lib.mv_get_grad(self.handle, name.encode(), fptr(out), out.size),
          self.handle)
    return out

  def get_opt_slot(self, name, slot):
    shape = dict(self.param_specs())[name]
    out = np.empty(shape, dtype=np.float32)
    check(self.lib.mv_get_opt_slot(self.handle, name.encode(), int(slot), fptr(out),
                                   out.size), self.handle)
    return out

  def set_opt_slot(self, name, slot, value):
    a = f32(value)
    check(self.lib.mv_set_opt_slot(self.handle, name.encode(), int(slot), fptr(a),
                                   a.size), self.handle)

  # ---- in-library gradient all-reduce (RCCL)
  def comm_init(self, rank, world, unique_id):
    if len(unique_id) != MV_COMM_ID_BYTES:
      raise MvError("unique id must be %d bytes" % MV_COMM_ID_BYTES)
    buf = (C.c_uint8 * MV_COMM_ID_BYTES).from_buffer_copy(unique_id)
    check(self.lib.mv_allreduce_init(self.handle, int(rank), int(world), buf), self.handle)
    self.comm_world = int(world)

  def comm_info(self):
    r, w, b, by = C.c_int32(), C.c_int32(), C.c_int32(), C.c_double()
    if self.lib.mv_allreduce_info(self.handle, C.byref(r), C.byref(w), C.byref(b),
                                  C.byref(by)) != 0:
      return None
    return {"rank": r.value, "world": w.value, "buckets": b.value, "bytes": by.value}

  # ---- SimAug extras: attacks on the resident scene features
  def _scene_shape(self):
    cfg = self.cfg
    return (self._num_frames, cfg.scene_h, cfg.scene_w, cfg.scene_class)

  def attack_begin(self):
    check(self.lib.mv_attack_begin(self.handle), self.handle)

  def attack_end(self):
    check(self.lib.mv_attack_end(self.handle), self.handle)

  def set_scene_feat(self, a):
    a = f32(a).reshape(self._scene_shape())
    check(self.lib.mv_set_scene_feat(self.handle, fptr(a)), self.handle)

  def get_scene_feat(self):
    out = np.empty(self._scene_shape(), dtype=np.float32)
    check(self.lib.mv_get_scene_feat(self.handle, fptr(out)), self.handle)
    return out

  def get_scene_grad(self):
    out = np.empty(self._scene_shape(), dtype=np.float32)
    check(self.lib.mv_get_scene_grad(self.handle, fptr(out)), self.handle)
    return out

  def attack_step(self, epsilon, step):
    check(self.lib.mv_attack_step(self.handle, float(epsilon), float(step)), self.handle)

  def scene_mix(self, other, weight):
    o = None if other is None else f32(other).reshape(self._scene_shape())
    check(self.lib.mv_scene_mix(self.handle, fptr(o), float(weight)), self.handle)

  def sample_losses(self, scale):
    out = np.empty((self.cfg.batch_size,), dtype=np.float32)
    check(self.lib.mv_get_sample_losses(self.handle, int(scale), fptr(out)), self.handle)
    return out

  def set_label_mixup(self, obs_labels2, pred_labels2, weight, sample_weight=None):
    """SimAug multi-view experiment 3: train on w * one_hot(label) + (1 - w) * one_hot(label2)
    (lists over scales of [N, T_o] / [N, T_p] int arrays, None for unused scales) until
    clear_label_mixup(); sample_weight [N]: per-sample weights of the class loss."""
    S = len(self.cfg.scene_grids)
    keep, po, pp = [], (_ip * MV_MAX_SCALES)(), (_ip * MV_MAX_SCALES)()
    for s in range(S):
      if not self.cfg.use_grids[s]:
        continue
      o = np.ascontiguousarray(obs_labels2[s], dtype=np.int32).reshape(self.cfg.batch_size, -1)
      p = np.ascontiguousarray(pred_labels2[s], dtype=np.int32).reshape(self.cfg.batch_size, -1)
      if o.shape[1] != self.cfg.obs_len or p.shape[1] != getattr(self, "_pred_len", p.shape[1]):
        raise MvError("set_label_mixup: labels of scale %d have shapes %s / %s" %
                      (s, o.shape, p.shape))
      keep += [o, p]
      po[s], pp[s] = o.ctypes.data_as(_ip), p.ctypes.data_as(_ip)
    sw = None
    if sample_weight is not None:
      sw = np.ascontiguousarray(sample_weight, dtype=np.float32).reshape(self.cfg.batch_size)
    check(self.lib.mv_set_label_mixup(self.handle, po, pp, float(weight),
                                      fptr(sw) if sw is not None else None), self.handle)

  def clear_label_mixup(self):
    check(self.lib.mv_clear_label_mixup(self.handle), self.handle)

  def set_dropout_seed(self, seed):
    check(self.lib.mv_set_dropout_seed(self.handle, int(seed) & 0xFFFFFFFF), self.handle)

  def opt_scalars(self):
    a, b = C.c_float(), C.c_float()
    check(self.lib.mv_get_opt_scalars(self.handle, C.byref(a), C.byref(b)), self.handle)
    return float(a.value), float(b.value)

  def set_opt_scalars(self, b1p, b2p):
    check(self.lib.mv_set_opt_scalars(self.handle, float(b1p), float(b2p)), self.handle)

  @property
  def global_step(self):
    v = C.c_int64()
    if self.lib.mv_get_global_step(self.handle, C.byref(v)) != 0:
      raise MvError("mv_train_init has not been called")
    return int(v.value)

  @global_step.setter
  def global_step(self, step):
    if self.lib.mv_set_global_step(self.handle, int(step)) != 0:
      raise MvError("mv_train_init has not been called")

  def set_compute_mode(self, mode):
    """0 / "f32": fp32 MFMA; 1 / "f16x3": split-fp16 matrix pipe at fp32 accuracy;
    2 / "bf16": bf16 operands, fp32 accumulate and state (BASELINE configs[4])."""
    mode = {"f32": 0, "f16x3": 1, "bf16": 2}.get(mode, mode)
    check(self.lib.mv_set_compute_mode(self.handle, int(mode)), self.handle)

  def set_graph_mode(self, on):
    check(self.lib.mv_set_graph_mode(self.handle, 1 if on else 0), self.handle)

  # ---- measurement
  def set_profiling(self, on):
    check(self.lib.mv_set_profiling(self.handle, 1 if on else 0), self.handle)

  def reset_kernel_stats(self):
    check(self.lib.mv_reset_kernel_stats(self.handle), self.handle)

  def kernel_stats(self):
    out = {}
    name = C.create_string_buffer(256)
    n, ms, fl, by, dn = C.c_int64(), C.c_double(), C.c_double(), C.c_double(), C.c_double()
    mf = C.c_double()
    for i in range(self.lib.mv_num_kernel_stats(self.handle)):
      self.lib.mv_kernel_stat(self.handle, i, name, 256, C.byref(n), C.byref(ms),
                              C.byref(fl), C.byref(by))
      self.lib.mv_kernel_stat_dense_flops(self.handle, i, C.byref(dn))
      self.lib.mv_kernel_stat_mfma_flops(self.handle, i, C.byref(mf))
      # flops: algorithmic FLOPs the launches executed; flops_dense: the same steps as
      # the reference computes them (a zero-state encoder step still multiplies h = 0);
      # flops_mfma: FLOPs issued to the matrix pipe (f16x3: 3 MFMAs per product in the
      # direct form, 2 in the Winograd form)
      out[name.value.decode()] = {"launches": int(n.value), "total_ms": ms.value,
                                  "flops": fl.value, "bytes": by.value,
                                  "flops_dense": dn.value, "flops_mfma": mf.value}
    return out


# ------------------------------------------------ single-kernel entry points

def op_convlstm_step(x, c, h, kernel, biases, device=0):
  lib = load()
  x = f32(x)
  M, H, W, Cx = x.shape
  Cc = int(kernel.shape[3]) // 4
  kernel, biases = f32(kernel), f32(biases)
  c_out = np.empty((M, H, W, Cc), dtype=np.float32)
  h_out = np.empty((M, H, W, Cc), dtype=np.float32)
  if c is None:
    cp, hp = _fp(), _fp()
  else:
    c, h = f32(c), f32(h)
    cp, hp = fptr(c), fptr(h)
  check(lib.mv_op_convlstm_step(device, fptr(x), cp, hp, fptr(kernel), fptr(biases),
                                M, H, W, Cx, Cc, fptr(c_out), fptr(h_out)))
  return c_out, h_out


def op_convlstm_step16(x, c, h, kernel, biases, variant, device=0):
  """The step on the fp16 matrix pipe (f16x3 planes): variant 1 = direct form, 2 = Winograd
  F(2,3) over image rows, 3 = Winograd F(3,3), 4 = bf16 on the row-triple tile, 5 = bf16 on the
  32-cell body, 6 = that body with three x passes (include/multiverse_hip.h).  Returns c', h' and
  the h' operand planes decoded to fp32."""
  lib = load()
  x = f32(x)
  M, H, W, Cx = x.shape
  Cc = int(kernel.shape[3]) // 4
  kernel, biases = f32(kernel), f32(biases)
  c_out = np.empty((M, H, W, Cc), dtype=np.float32)
  h_out = np.empty((M, H, W, Cc), dtype=np.float32)
  h16 = np.empty((M, H, W, Cc), dtype=np.float32)
  if c is None:
    cp, hp = _fp(), _fp()
  else:
    c, h = f32(c), f32(h)
    cp, hp = fptr(c), fptr(h)
  check(lib.mv_op_convlstm_step16(device, int(variant), fptr(x), cp, hp, fptr(kernel),
                                  fptr(biases), M, H, W, Cx, Cc, fptr(c_out), fptr(h_out),
                                  fptr(h16)))
  return c_out, h_out, h16


def op_gnn(h, scene_mean, device=0, version=0):
  """version: 0 = the library's choice, 1 / 2 / 3 = that kernel version where it takes the shape
  (mv_op_gnn_variant)."""
  lib = load()
  h, scene_mean = f32(h), f32(scene_mean)
  M, H, W, Cc = h.shape
  out = np.empty_like(h)
  check(lib.mv_op_gnn_variant(device, fptr(h), fptr(scene_mean), M, H, W, Cc,
                              scene_mean.shape[-1], int(version), fptr(out)))
  return out


def op_hidden2grid(h, w, device=0):
  lib = load()
  h, w = f32(h), f32(w)
  M, H, W, Cc = h.shape
  P = w.shape[-1]
  out = np.empty((M, H, W, P), dtype=np.float32)
  check(lib.mv_op_hidden2grid(device, fptr(h), fptr(w), M, H, W, Cc, P, fptr(out)))
  return out


def _allowed_plane(allowed, samples, K):
  a = np.ascontiguousarray(np.asarray(allowed).reshape(samples, K) != 0, dtype=np.uint8)
  return a, a.ctypes.data_as(_u8p)


def _bias_plane(bias, samples, K):
  return f32(np.asarray(bias, dtype=np.float32).reshape(samples, K))


def _step_motion(motion, samples, rows):
  """motion: a dict with W, radius, vel [samples, D, D], vel_far [samples], optionally acc /
  acc_far, and prev1 / prev0 int32 [rows] (prev0 -1 = absent) -> (mv_step_motion, the arrays it
  points into, to be kept alive over the call)."""
  D = 2 * int(motion["radius"]) + 1
  m = mv_step_motion()
  m.W, m.radius = int(motion["W"]), int(motion["radius"])
  keep = []
  for name, count in (("vel", samples * D * D), ("vel_far", samples), ("acc", samples * D * D),
                      ("acc_far", samples)):
    if motion.get(name) is None:
      continue                   # (the library names a missing table)
    a = f32(np.asarray(motion[name], dtype=np.float32).reshape(-1))
    if 1 <= m.radius <= MV_MOTION_MAX_RADIUS and a.size != count:
      raise MvError("motion: %s has %d values, not %d (samples = %d, radius = %d)"
                    % (name, a.size, count, samples, m.radius))
    keep.append(a)
    setattr(m, name, fptr(a))
  p1 = np.ascontiguousarray(np.asarray(motion["prev1"], dtype=np.int32).reshape(rows))
  p0 = np.ascontiguousarray(np.asarray(motion["prev0"], dtype=np.int32).reshape(rows))
  keep += [p1, p0]
  m.prev1, m.prev0 = iptr(p1), iptr(p0)
  return m, keep


def _step_revisit(revisit, samples, rows, K):
  """revisit: a dict with cost [samples], prev1 int32 [rows] and, optionally, visited [rows, K]
  (non-zero = in the row's set going into the step; absent = empty) -> (mv_step_revisit, the
  arrays it points into, visited_out uint8 [rows, K] that the op fills with the stored sets)."""
  m = mv_step_revisit()
  cost = f32(np.asarray(revisit["cost"], dtype=np.float32).reshape(samples))
  p1 = np.ascontiguousarray(np.asarray(revisit["prev1"], dtype=np.int32).reshape(rows))
  out = np.zeros((rows, K), dtype=np.uint8)
  keep = [cost, p1, out]
  m.cost, m.prev1 = fptr(cost), iptr(p1)
  if revisit.get("visited") is not None:
    v = np.ascontiguousarray((np.asarray(revisit["visited"]).reshape(rows, K) != 0)
                             .astype(np.uint8))
    keep.append(v)
    m.visited = v.ctypes.data_as(_u8p)
  m.visited_out = out.ctypes.data_as(_u8p)
  return m, keep, out


def op_beam_step(logits, prev_lp, time, diverse, gamma, fix_num_timestep, device=0,
                 allowed=None, bias=None, motion=None, revisit=None):
  """allowed [N, K] (non-zero = the cell may be chosen): the masked step, mv_op_beam_step_masked.
  bias [N, K] float32 cell costs: the biased step, mv_op_beam_step_biased (allowed optional).
  motion (the dict of `_step_motion`, prev1 / prev0 [N, B]): the step under a motion cost,
  mv_op_beam_step_motion (allowed and bias optional)."""
  lib = load()
  logits, prev_lp = f32(logits), f32(prev_lp)
  N, B, K = logits.shape
  new_lp = np.empty((N, B), dtype=np.float32)
  ids = np.empty((N, B), dtype=np.int32)
  parents = np.empty((N, B), dtype=np.int32)
  if revisit is not None:
    # mv_op_beam_step_path (the dict of `_step_revisit`, prev1 / visited per row [N, B]; allowed,
    # bias and motion optional) -> (new_lp, ids, parents, visited_out bool [N, B, K])
    a, ap = _allowed_plane(allowed, N, K) if allowed is not None else (None, None)
    bz = _bias_plane(bias, N, K) if bias is not None else None
    m, keep = _step_motion(motion, N, N * B) if motion is not None else (None, None)
    rv, alive, vout = _step_revisit(revisit, N, N * B, K)
    check(lib.mv_op_beam_step_path(device, fptr(logits), fptr(prev_lp), ap,
                                   fptr(bz) if bz is not None else None,
                                   C.byref(m) if m is not None else None, C.byref(rv), N, B, K,
                                   int(time), 1 if diverse else 0, float(gamma),
                                   int(fix_num_timestep), fptr(new_lp), iptr(ids), iptr(parents)))
    return new_lp, ids, parents, vout.reshape(N, B, K).astype(bool)
  if motion is not None:
    a, ap = _allowed_plane(allowed, N, K) if allowed is not None else (None, None)
    bz = _bias_plane(bias, N, K) if bias is not None else None
    m, keep = _step_motion(motion, N, N * B)
    check(lib.mv_op_beam_step_motion(device, fptr(logits), fptr(prev_lp), ap,
                                     fptr(bz) if bz is not None else None, C.byref(m), N, B, K,
                                     int(time), 1 if diverse else 0, float(gamma),
                                     int(fix_num_timestep), fptr(new_lp), iptr(ids),
                                     iptr(parents)))
    return new_lp, ids, parents
  if bias is not None:
    a, ap = _allowed_plane(allowed, N, K) if allowed is not None else (None, None)
    bz = _bias_plane(bias, N, K)
    check(lib.mv_op_beam_step_biased(device, fptr(logits), fptr(prev_lp), ap, fptr(bz), N, B, K,
                                     int(time), 1 if diverse else 0, float(gamma),
                                     int(fix_num_timestep), fptr(new_lp), iptr(ids),
                                     iptr(parents)))
    return new_lp, ids, parents
  if allowed is not None:
    a, ap = _allowed_plane(allowed, N, K)
    check(lib.mv_op_beam_step_masked(device, fptr(logits), fptr(prev_lp), ap, N, B, K, int(time),
                                     1 if diverse else 0, float(gamma), int(fix_num_timestep),
                                     fptr(new_lp), iptr(ids), iptr(parents)))
    return new_lp, ids, parents
  check(lib.mv_op_beam_step(device, fptr(logits), fptr(prev_lp), N, B, K, int(time),
                            1 if diverse else 0, float(gamma), int(fix_num_timestep),
                            fptr(new_lp), iptr(ids), iptr(parents)))
  return new_lp, ids, parents


def op_sbs_step(logits, prev_phi, prev_lp, prev_g, t, temperature=1.0, seed=0, device=0,
                allowed=None, bias=None, motion=None, revisit=None):
  """One step of the sampling without replacement (mv_op_sbs_step): logits [N, B, K], prev_*
  [N, B] -> (new_phi, new_logprob, new_gumbel, ids, parents), each [N, B].  allowed [N, K]: the
  masked step (mv_op_sbs_step_masked).  bias [N, K]: the biased step (mv_op_sbs_step_biased;
  allowed optional)."""
  lib = load()
  logits, prev_phi, prev_lp, prev_g = f32(logits), f32(prev_phi), f32(prev_lp), f32(prev_g)
  N, B, K = logits.shape
  phi, lp, g = (np.empty((N, B), dtype=np.float32) for _ in range(3))
  ids = np.empty((N, B), dtype=np.int32)
  parents = np.empty((N, B), dtype=np.int32)
  if revisit is not None:      # mv_op_sbs_step_path: the rest optional; + visited_out [N, B, K]
    a, ap = _allowed_plane(allowed, N, K) if allowed is not None else (None, None)
    bz = _bias_plane(bias, N, K) if bias is not None else None
    m, keep = _step_motion(motion, N, N * B) if motion is not None else (None, None)
    rv, alive, vout = _step_revisit(revisit, N, N * B, K)
    check(lib.mv_op_sbs_step_path(device, fptr(logits), fptr(prev_phi), fptr(prev_lp),
                                  fptr(prev_g), ap, fptr(bz) if bz is not None else None,
                                  C.byref(m) if m is not None else None, C.byref(rv), N, B, K,
                                  int(t), float(temperature), int(seed) & 0xFFFFFFFF, fptr(phi),
                                  fptr(lp), fptr(g), iptr(ids), iptr(parents)))
    return phi, lp, g, ids, parents, vout.reshape(N, B, K).astype(bool)
  if motion is not None:       # mv_op_sbs_step_motion: allowed and bias optional
    a, ap = _allowed_plane(allowed, N, K) if allowed is not None else (None, None)
    bz = _bias_plane(bias, N, K) if bias is not None else None
    m, keep = _step_motion(motion, N, N * B)
    check(lib.mv_op_sbs_step_motion(device, fptr(logits), fptr(prev_phi), fptr(prev_lp),
                                    fptr(prev_g), ap, fptr(bz) if bz is not None else None,
                                    C.byref(m), N, B, K, int(t), float(temperature),
                                    int(seed) & 0xFFFFFFFF, fptr(phi), fptr(lp), fptr(g),
                                    iptr(ids), iptr(parents)))
    return phi, lp, g, ids, parents
  if bias is not None:
    a, ap = _allowed_plane(allowed, N, K) if allowed is not None else (None, None)
    bz = _bias_plane(bias, N, K)
    check(lib.mv_op_sbs_step_biased(device, fptr(logits), fptr(prev_phi), fptr(prev_lp),
                                    fptr(prev_g), ap, fptr(bz), N, B, K, int(t),
                                    float(temperature), int(seed) & 0xFFFFFFFF, fptr(phi),
                                    fptr(lp), fptr(g), iptr(ids), iptr(parents)))
    return phi, lp, g, ids, parents
  if allowed is not None:
    a, ap = _allowed_plane(allowed, N, K)
    check(lib.mv_op_sbs_step_masked(device, fptr(logits), fptr(prev_phi), fptr(prev_lp),
                                    fptr(prev_g), ap, N, B, K, int(t), float(temperature),
                                    int(seed) & 0xFFFFFFFF, fptr(phi), fptr(lp), fptr(g),
                                    iptr(ids), iptr(parents)))
    return phi, lp, g, ids, parents
  check(lib.mv_op_sbs_step(device, fptr(logits), fptr(prev_phi), fptr(prev_lp), fptr(prev_g),
                           N, B, K, int(t), float(temperature), int(seed) & 0xFFFFFFFF,
                           fptr(phi), fptr(lp), fptr(g), iptr(ids), iptr(parents)))
  return phi, lp, g, ids, parents


def enc_cone_build(labels, H, W, r0=1):
  """Tile lists of the class encoder's light cone as every upload builds them
  (mv_enc_cone_build; host only).  labels [N, T] -> (lists [T, 4 + 2 * ntile] int32,
  cells [T] int64, ntile)."""
  lib = load()
  labels = np.ascontiguousarray(labels, dtype=np.int32)
  N, T = labels.shape
  ip = lambda a: a.ctypes.data_as(_ip)
  ntile = lib.mv_enc_cone_build(None, N, T, int(H), int(W), int(r0), None, None)
  if ntile < 0:
    raise MvError("mv_enc_cone_build: bad arguments")
  lists = np.zeros((T, 4 + 2 * ntile), np.int32)
  cells = np.zeros((T,), np.int64)
  if lib.mv_enc_cone_build(ip(labels), N, T, int(H), int(W), int(r0), ip(lists),
                           cells.ctypes.data_as(C.POINTER(C.c_int64))) < 0:
    raise MvError("mv_enc_cone_build: a label is not a cell of the %d x %d grid" % (H, W))
  return lists, cells, int(ntile)


SCENE_CONV_FORMS = ("per_output", "proj1x1", "tiled")    # SceneConvForm, csrc/step_plan.h


def scene_conv_form(k, Ci, Co):
  """The kernel the engine launches for a level of the scene stack (host only)."""
  return SCENE_CONV_FORMS[load().mv_scene_conv_form(int(k), int(Ci), int(Co))]


def op_scene_conv(x, w, b, act=0, per_output=False, device=0):
  """One scene-stack level (mv_op_scene_conv): x [U, Hi, Wi, Ci], w [k, k, Ci, Co], b [Co] ->
  [U, ceil(Hi/2), ceil(Wi/2), Co].  per_output: the one-thread-per-output kernel whatever the
  shape; otherwise the engine's choice."""
  lib = load()
  x, w, b = f32(x), f32(w), f32(b)
  U, Hi, Wi, Ci = x.shape
  k, Co = int(w.shape[0]), int(w.shape[3])
  out = np.empty((U, (Hi + 1) // 2, (Wi + 1) // 2, Co), dtype=np.float32)
  check(lib.mv_op_scene_conv(device, 1 if per_output else 0, fptr(x), fptr(w), fptr(b), U, Hi,
                             Wi, Ci, Co, k, int(act), fptr(out)))
  return out


# mv_op_decode_tail: the plane buffer of an [M, E] operand as an engine allocates it
# (csrc/plane_layout.h kPlaneSlack, csrc/convlstm_f16x3.h kPlanePad; the call refuses any other
# size) and the byte every output buffer holds before the launches
PLANE_SLACK, PLANE_PAD = 32 * 1024, 16
OP_SENTINEL_BYTE = 0xA5
TAIL_NEXT = {"none": 0, "ids": 1, "embed": 2}
TAIL_PLANES = {None: 0, "f16x3": 1, "bf16": 2}
TAIL_FORMS = {False: 0, True: 1, "onehot8": 2, "dense": 3}


def plane_buffer_elems(M, E):
  return 2 * (int(M) * int(E) + PLANE_SLACK + PLANE_PAD)


def op_decode_tail(chains, act=0, next="embed", planes=None, separate=False, device=0):
  """The decoder tail of one step for 1 to 4 chains in one call (mv_op_decode_tail).  chains:
  dicts with kind ("cls": P = 1, one-hot; "reg": P = 2, dense), h [rows, H, W, C], w_out
  [3, 3, C, P], emb_w [3, 3, P, E], emb_b [E].  next: "none" (output rows only), "ids" (argmax
  without embedding) or "embed".  planes: None, "f16x3" (two fp16 planes) or "bf16" (one).
  separate: False = the grouped tail (h2g_q + decode_tail, one launch each for all chains); True =
  the separate tail's kernels per chain; "onehot8" / "dense" = the separate tail with the class
  embedding by grid_emb_onehot8_kernel / by grid_emb_dense_kernel on the literal one-hot map.
  Returns per chain a dict: out [rows, K, P]; ids [rows] (class chains); x [rows * K, E]; planes,
  the whole raw uint16 plane buffer (plane_buffer_elems; plane 0 at PLANE_PAD, plane 1 half the
  buffer further), when planes is not None.  Whatever the call did not write holds
  OP_SENTINEL_BYTE in every byte."""
  lib = load()
  n = len(chains)
  arr = (mv_tail_chain * max(n, 1))()
  keep, res = [], []
  C_, E = None, None
  for i, ch in enumerate(chains):
    cls = {"cls": True, "reg": False}[ch["kind"]]
    P = 1 if cls else 2
    h, w = f32(ch["h"]), f32(ch["w_out"])
    ew, eb = f32(ch["emb_w"]), f32(ch["emb_b"])
    rows, H, W, Ch = h.shape
    if w.shape != (3, 3, Ch, P) or ew.shape[:3] != (3, 3, P) or eb.shape != (ew.shape[3],):
      raise MvError("op_decode_tail: chain %d: weight shapes %r %r %r" % (i, w.shape, ew.shape,
                                                                         eb.shape))
    if (C_, E) not in ((None, None), (Ch, ew.shape[3])):
      raise MvError("op_decode_tail: the chains of a call share C and E")
    C_, E = Ch, int(ew.shape[3])
    K = H * W
    out = np.empty((rows, K, P), dtype=np.float32)
    x = np.empty((rows * K, E), dtype=np.float32)
    r = {"out": out, "x": x}
    a = arr[i]
    a.rows, a.H, a.W, a.kind = rows, H, W, 0 if cls else 1
    a.h, a.w_out, a.emb_w, a.emb_b = fptr(h), fptr(w), fptr(ew), fptr(eb)
    a.out, a.x = fptr(out), fptr(x)
    if cls:
      r["ids"] = np.empty(rows, dtype=np.int32)
      a.ids = iptr(r["ids"])
    if planes is not None:
      r["planes"] = np.empty(plane_buffer_elems(rows * K, E), dtype=np.uint16)
      a.planes = r["planes"].ctypes.data_as(C.POINTER(C.c_uint16))
      a.planes_elems = r["planes"].size
    keep.append((h, w, ew, eb))
    res.append(r)
  check(lib.mv_op_decode_tail(device, TAIL_FORMS[separate], TAIL_NEXT[next], TAIL_PLANES[planes],
                              int(C_ or 0), int(E or 0), int(act), arr, n))
  return res


def op_sample_step(logits, S, t, temperature=1.0, seed=0, top_k=0, top_p=1.0, floor=1, device=0,
                   allowed=None, bias=None, motion=None, revisit=None):
  """One step of the independent sampler under top-k / nucleus limits (mv_op_sample_step):
  logits [R, K], row r = future r % S of sample r // S -> (ids int32 [R], lp [R] the model's
  log-probability of the drawn cell, qlp [R] the proposal's, keep bool [R, K] the kept set).
  allowed [R // S, K], one plane per sample: the masked step (mv_op_sample_step_masked).
  bias [R // S, K]: the biased step (mv_op_sample_step_biased; allowed optional)."""
  lib = load()
  logits = f32(logits)
  R, K = logits.shape
  ids = np.empty(R, dtype=np.int32)
  lp, qlp = (np.empty(R, dtype=np.float32) for _ in range(2))
  keep = np.empty((R, K), dtype=np.uint8)
  if revisit is not None:      # mv_op_sample_step_path: the rest optional; + visited_out [R, K]
    a, ap = _allowed_plane(allowed, R // int(S), K) if allowed is not None else (None, None)
    bz = _bias_plane(bias, R // int(S), K) if bias is not None else None
    m, alive = _step_motion(motion, R // int(S), R) if motion is not None else (None, None)
    rv, alive2, vout = _step_revisit(revisit, R // int(S), R, K)
    check(lib.mv_op_sample_step_path(device, fptr(logits), ap,
                                     fptr(bz) if bz is not None else None,
                                     C.byref(m) if m is not None else None, C.byref(rv), R, int(S),
                                     K, int(t), float(temperature), int(seed) & 0xFFFFFFFF,
                                     int(top_k), float(top_p), int(floor), iptr(ids), fptr(lp),
                                     fptr(qlp), keep.ctypes.data_as(_u8p)))
    return ids, lp, qlp, keep.astype(bool), vout.astype(bool)
  if motion is not None:       # mv_op_sample_step_motion (prev1 / prev0 [R]): the rest optional
    a, ap = _allowed_plane(allowed, R // int(S), K) if allowed is not None else (None, None)
    bz = _bias_plane(bias, R // int(S), K) if bias is not None else None
    m, alive = _step_motion(motion, R // int(S), R)
    check(lib.mv_op_sample_step_motion(device, fptr(logits), ap,
                                       fptr(bz) if bz is not None else None, C.byref(m), R, int(S),
                                       K, int(t), float(temperature), int(seed) & 0xFFFFFFFF,
                                       int(top_k), float(top_p), int(floor), iptr(ids), fptr(lp),
                                       fptr(qlp), keep.ctypes.data_as(_u8p)))
    return ids, lp, qlp, keep.astype(bool)
  if bias is not None:
    a, ap = _allowed_plane(allowed, R // int(S), K) if allowed is not None else (None, None)
    bz = _bias_plane(bias, R // int(S), K)
    check(lib.mv_op_sample_step_biased(device, fptr(logits), ap, fptr(bz), R, int(S), K, int(t),
                                       float(temperature), int(seed) & 0xFFFFFFFF, int(top_k),
                                       float(top_p), int(floor), iptr(ids), fptr(lp), fptr(qlp),
                                       keep.ctypes.data_as(_u8p)))
    return ids, lp, qlp, keep.astype(bool)
  if allowed is not None:
    a, ap = _allowed_plane(allowed, R // int(S), K)
    check(lib.mv_op_sample_step_masked(device, fptr(logits), ap, R, int(S), K, int(t),
                                       float(temperature), int(seed) & 0xFFFFFFFF, int(top_k),
                                       float(top_p), int(floor), iptr(ids), fptr(lp), fptr(qlp),
                                       keep.ctypes.data_as(_u8p)))
    return ids, lp, qlp, keep.astype(bool)
  check(lib.mv_op_sample_step(device, fptr(logits), R, int(S), K, int(t), float(temperature),
                              int(seed) & 0xFFFFFFFF, int(top_k), float(top_p), int(floor),
                              iptr(ids), fptr(lp), fptr(qlp), keep.ctypes.data_as(_u8p)))
  return ids, lp, qlp, keep.astype(bool)


def op_convlstm_bwd(x, c, h, kernel, biases, dh_new, dc_new, device=0):
  """-> (dx, dh, dc, dkernel, dbiases)"""
  lib = load()
  x = f32(x)
  M, H, W, Cx = x.shape
  Cc = int(kernel.shape[3]) // 4
  kernel, biases = f32(kernel), f32(biases)
  dh_new, dc_new = f32(dh_new), f32(dc_new)
  if c is None:
    cp, hp = _fp(), _fp()
  else:
    c, h = f32(c), f32(h)
    cp, hp = fptr(c), fptr(h)
  dx = np.empty((M, H, W, Cx), dtype=np.float32)
  dh = np.empty((M, H, W, Cc), dtype=np.float32)
  dc = np.empty((M, H, W, Cc), dtype=np.float32)
  dk = np.empty(kernel.shape, dtype=np.float32)
  db = np.empty(biases.shape, dtype=np.float32)
  check(lib.mv_op_convlstm_bwd(device, fptr(x), cp, hp, fptr(kernel), fptr(biases),
                               fptr(dh_new), fptr(dc_new), M, H, W, Cx, Cc, fptr(dx),
                               fptr(dh), fptr(dc), fptr(dk), fptr(db)))
  return dx, dh, dc, dk, db


BWD16_DGRAD = {None: 0, "f16x3": 1, "wino": 2, "bf16": 3}
BWD16_WGRAD = {None: 0, "f16x3": 1, "f16x3_triple": 2, "one": 3, "one_triple": 4}


def op_convlstm_bwd16(x, h, G, kernel, dgrad=None, wgrad=None, device=0):
  """The matrix-pipe backward of one gate convolution by its single kernels
  (mv_op_convlstm_bwd16): dgrad in BWD16_DGRAD, wgrad in BWD16_WGRAD, None skips that half.
  -> dict(dx, dh, dkernel (None where skipped), exps=(G, h, x), wide, wide_x, nsplit, nsplit_x,
  dgrad_slices=(d h, d x), shift, transpose3)."""
  lib = load()
  x, h, G, kernel = f32(x), f32(h), f32(G), f32(kernel)
  M, H, W, Cx = x.shape
  Cc = int(kernel.shape[3]) // 4
  assert h.shape == (M, H, W, Cc) and G.shape == (M, H, W, 4 * Cc)
  assert kernel.shape == (3, 3, Cx + Cc, 4 * Cc)
  vd, vw = BWD16_DGRAD[dgrad], BWD16_WGRAD[wgrad]
  dx = np.empty((M, H, W, Cx), dtype=np.float32) if vd else None
  dh = np.empty((M, H, W, Cc), dtype=np.float32) if vd else None
  dk = np.empty(kernel.shape, dtype=np.float32) if vw else None
  exps = np.zeros(3, dtype=np.int32)
  forms = np.zeros(8, dtype=np.int32)
  opt = lambda a: fptr(a) if a is not None else _fp()
  check(lib.mv_op_convlstm_bwd16(device, vd, vw, fptr(x), fptr(h), fptr(G), fptr(kernel), M, H,
                                 W, Cx, Cc, opt(dx), opt(dh), opt(dk), iptr(exps), iptr(forms)))
  return dict(dx=dx, dh=dh, dkernel=dk, exps=tuple(int(e) for e in exps), wide=bool(forms[0]),
              wide_x=bool(forms[1]), nsplit=int(forms[2]), nsplit_x=int(forms[3]),
              dgrad_slices=(int(forms[4]), int(forms[5])), shift=bool(forms[6]),
              transpose3=bool(forms[7]))


def op_lstm_gate_bwd(gates, c_prev, c_new, dh, dc, form, device=0):
  """lstm_gate_bwd in its form 0 (scalar), 1 (four channels per thread) or 2 (the same with the
  bf16 plane): gates [cells, 4, C] -> (G [cells, 4C], dc [cells, C], gmax bits, plane or None)."""
  lib = load()
  gates, c_new, dh, dc = f32(gates), f32(c_new), f32(dh), f32(dc)
  cells, Cc = c_new.shape
  assert gates.size == cells * 4 * Cc
  cp = _fp()
  if c_prev is not None:
    c_prev = f32(c_prev)
    cp = fptr(c_prev)
  G = np.empty((cells, 4 * Cc), dtype=np.float32)
  dco = np.empty((cells, Cc), dtype=np.float32)
  plane = np.empty((cells, 4 * Cc), dtype=np.float32) if form == 2 else None
  bits = np.zeros(1, dtype=np.int32)
  check(lib.mv_op_lstm_gate_bwd(device, int(form), fptr(gates), cp, fptr(c_new), fptr(dh),
                                fptr(dc), cells, Cc, fptr(G), fptr(dco), iptr(bits),
                                fptr(plane) if plane is not None else _fp()))
  return G, dco, int(bits[0]), plane


def op_gnn_bwd(h, scene_mean, g, device=0):
  lib = load()
  h, scene_mean, g = f32(h), f32(scene_mean), f32(g)
  M, H, W, Cc = h.shape
  dh = np.empty_like(h)
  ds = np.empty_like(scene_mean)
  check(lib.mv_op_gnn_bwd(device, fptr(h), fptr(scene_mean), fptr(g), M, H, W, Cc,
                          scene_mean.shape[-1], fptr(dh), fptr(ds)))
  return dh, ds


# ---- the helper kernels of a training step, one door each (include/multiverse_hip.h)
SMALL_DGRAD_FORMS = {None: 0, "scalar": 1, "dgrad4<1>": 2, "dgrad4<2>": 3}
SMALL_WGRAD_FORMS = {None: 0, "small_wgrad<false>": 1, "small_wgrad<true>": 2, "h2g": 3}
TRAIN_LOSS_KINDS = {"ce": 0, "ce_soft": 1, "ce_len": 2, "huber": 3, "huber_len": 4,
                    "huber_masked": 5}


def _name_of(table, code):
  return [k for k, v in table.items() if v == code][0]


def op_small_conv_dgrad(dout, w, din, H, W, accumulate=False, form=None, device=0):
  """mv_op_small_conv_dgrad: dout [M, dout_rs] and din [M, din_rs] are whole strided buffers (the
  first H*W*C floats of a row in use); w [3, 3, Ci, Co].  Returns (din after the launch, the name
  of the form that ran)."""
  lib = load()
  dout, w = f32(dout), f32(w)
  din = f32(din).copy()
  M = int(dout.shape[0])
  Ci, Co = int(w.shape[2]), int(w.shape[3])
  assert dout.ndim == 2 and din.ndim == 2 and din.shape[0] == M and w.shape[:2] == (3, 3)
  ran = np.zeros(1, dtype=np.int32)
  check(lib.mv_op_small_conv_dgrad(device, SMALL_DGRAD_FORMS[form], fptr(dout),
                                   int(dout.shape[1]), fptr(w), fptr(din), int(din.shape[1]), M,
                                   int(H), int(W), Ci, Co, 1 if accumulate else 0, iptr(ran)))
  return din, _name_of(SMALL_DGRAD_FORMS, int(ran[0]))


def op_small_conv_wgrad(x, dout, form=None, device=0):
  """mv_op_small_conv_wgrad: x [R, H, W, Ci], dout [R, H, W, Co] -> (dw [3, 3, Ci, Co], dict of
  form, blocks, cells_per_block, G)."""
  lib = load()
  x, dout = f32(x), f32(dout)
  R, H, W, Ci = x.shape
  Co = int(dout.shape[3])
  assert dout.shape[:3] == (R, H, W)
  dw = np.empty((3, 3, Ci, Co), dtype=np.float32)
  info = np.zeros(4, dtype=np.int32)
  check(lib.mv_op_small_conv_wgrad(device, SMALL_WGRAD_FORMS[form], fptr(x), fptr(dout), R, H, W,
                                   Ci, Co, fptr(dw), iptr(info)))
  return dw, dict(form=_name_of(SMALL_WGRAD_FORMS, int(info[0])), blocks=int(info[1]),
                  cells_per_block=int(info[2]), G=int(info[3]))


def op_colsum(x, device=0):
  """mv_op_colsum: x [rows, ncols] -> (column sums [ncols], slabs, narrow)."""
  lib = load()
  x = f32(x)
  rows, ncols = x.shape
  out = np.empty(ncols, dtype=np.float32)
  info = np.zeros(2, dtype=np.int32)
  check(lib.mv_op_colsum(device, fptr(x), rows, ncols, fptr(out), iptr(info)))
  return out, int(info[0]), bool(info[1])


def op_long_sum(x, scale=1.0, device=0):
  """mv_op_long_sum: x [n] -> (scale * sum, whether the chunk stage ran)."""
  lib = load()
  x = f32(x).reshape(-1)
  out = np.empty(1, dtype=np.float32)
  ch = np.zeros(1, dtype=np.int32)
  check(lib.mv_op_long_sum(device, fptr(x), x.size, float(scale), fptr(out), iptr(ch)))
  return out[0], bool(ch[0])


def op_scene_conv_bwd(x, y, dy, w, act=0, din_init=None, accumulate=False, device=0):
  """mv_op_scene_conv_bwd: x [U, Hi, Wi, Ci], y / dy [U, Ho, Wo, Co], w [k, k, Ci, Co] -> dict of
  dpre, din, dw, db, pad_t, pad_l, slabs, rows_per_slab."""
  lib = load()
  x, y, dy, w = f32(x), f32(y), f32(dy), f32(w)
  U, Hi, Wi, Ci = x.shape
  k, Co = int(w.shape[0]), int(w.shape[3])
  assert y.shape == dy.shape == (U, (Hi + 1) // 2, (Wi + 1) // 2, Co)
  init = f32(din_init) if din_init is not None else None
  dpre, din = np.empty_like(y), np.empty_like(x)
  dw, db = np.empty_like(w), np.empty(Co, dtype=np.float32)
  info = np.zeros(4, dtype=np.int32)
  check(lib.mv_op_scene_conv_bwd(device, fptr(x), fptr(y), fptr(dy), fptr(w), U, Hi, Wi, Ci, Co,
                                 k, int(act), fptr(init), 1 if accumulate else 0, fptr(dpre),
                                 fptr(din), fptr(dw), fptr(db), iptr(info)))
  return dict(dpre=dpre, din=din, dw=dw, db=db, pad_t=int(info[0]), pad_l=int(info[1]),
              slabs=int(info[2]), rows_per_slab=int(info[3]))


def op_grid_emb_onehot_wgrad(dpre, labels, dw_init=None, accumulate=False, device=0):
  """mv_op_grid_emb_onehot_wgrad: dpre [T, N, H, W, E], labels [N, T] -> dw [3, 3, E]."""
  lib = load()
  dpre, labels = f32(dpre), i32(labels)
  T, N, H, W, E = dpre.shape
  assert labels.shape == (N, T)
  dw = f32(dw_init).copy() if dw_init is not None else np.zeros((3, 3, E), dtype=np.float32)
  assert dw.shape == (3, 3, E)
  check(lib.mv_op_grid_emb_onehot_wgrad(device, fptr(dpre), iptr(labels), N, T, H, W, E,
                                        1 if accumulate else 0, fptr(dw)))
  return dw


def op_train_loss(kind, pred, scale, labels=None, soft=None, target=None, fg=None,
                  sample_w=None, pred_lens=None, device=0):
  """mv_op_train_loss: pred [T, N, K] (cross entropies) or [T, N, K, 2] (Huber kinds, target
  [N, T, K, 2], fg [T, N, K]) -> dict of loss (rows [T, N] or elements), grad, loss_sum, count,
  chunked."""
  lib = load()
  pred = f32(pred)
  T, N, K = pred.shape[:3]
  ce = TRAIN_LOSS_KINDS[kind] <= 2
  assert pred.ndim == (3 if ce else 4)
  opt = lambda a, conv: conv(a) if a is not None else None
  labels, pred_lens = opt(labels, i32), opt(pred_lens, i32)
  soft, target, fg, sample_w = opt(soft, f32), opt(target, f32), opt(fg, f32), opt(sample_w, f32)
  assert labels is None or labels.shape == (N, T)
  assert soft is None or soft.shape == pred.shape
  assert target is None or target.shape == (N, T, K, 2)
  assert fg is None or fg.shape == (T, N, K)
  assert sample_w is None or sample_w.shape == (N,)
  assert pred_lens is None or pred_lens.shape == (N,)
  loss = np.empty((T, N) if ce else pred.shape, dtype=np.float32)
  grad = np.empty_like(pred)
  total = np.empty(1, dtype=np.float32)
  info = np.zeros(2, dtype=np.int32)
  check(lib.mv_op_train_loss(device, TRAIN_LOSS_KINDS[kind], fptr(pred), iptr(labels), fptr(soft),
                             fptr(target), fptr(fg), fptr(sample_w), iptr(pred_lens), T, N, K,
                             float(scale), fptr(loss), fptr(grad), fptr(total), iptr(info)))
  return dict(loss=loss, grad=grad, loss_sum=total[0], count=int(info[0]), chunked=bool(info[1]))
