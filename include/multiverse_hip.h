/*
 * multiverse_hip.h -- C ABI of the MI355X-native Multiverse engine
 * (libmultiverse_hip.so, built from multiverse_amd/csrc/).
 *
 * The reference (JunweiLiang/Multiverse) has no plugin / operator / FFI
 * interface: its device boundary is `sess.run(fetches, feed_dict)` inside
 *   Tester.step   code/pred_models.py:1761-1790   (greedy forward)
 *   Trainer.step  code/pred_models.py:1719-1742   (training step)
 *   multifuture_inference.py:460-472              (beam-search forward)
 * over the TF-1 graph built by Model.build_forward (code/pred_models.py:123-308).
 * The entry points below are what a binding for that boundary binds: one call
 * per `sess.run`, numpy buffers in, numpy buffers out, weights addressed by
 * their TF-1 variable names (HWIO layout, exactly what tf.train.Saver stores).
 * No torch / TF types appear in any signature.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on error; the message is
 *     available from mv_last_error(handle) (or mv_last_error(NULL) for
 *     create-time failures).
 *   - all tensors are dense, row-major, NHWC; float = IEEE binary32,
 *     integers = int32.
 *   - input buffers are caller-owned and only read during the call; output
 *     buffers are caller-allocated and fully written on success.
 *   - calls on one handle are not re-entrant (the reference is a single
 *     synchronous Python thread).  Each handle owns one
 *     HIP stream; calls return after their results are on the host unless the
 *     *_async / *_resident variants are used.
 */
#ifndef MULTIVERSE_HIP_H_
#define MULTIVERSE_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MV_MAX_SCALES 2
#define MV_ABI_VERSION 5

typedef struct mv_engine* mv_handle;

/* Mirrors the config fields Model reads; authoritative list:
 * reference code/multifuture_inference.py:419-452. */
typedef struct mv_config {
  int32_t abi_version;       /* MV_ABI_VERSION */
  int32_t batch_size;        /* N, fixed per model instance (pred_models.py:47) */
  int32_t obs_len;           /* T_o */
  int32_t max_pred_len;      /* upper bound of the run-time T_pred */
  int32_t scene_h, scene_w, scene_class;        /* 36, 64, 11 */
  /* scene_conv_dim 0 = a model built WITHOUT the scene encoder (--use_scene_enc off, the
   * reference's default graph, code/pred_models.py:146-165, 218-229): no scene stack; the class
   * encoders take grid_emb(one_hot(labels)) through ONE person_pred/grid_emb/{W [3,3,1,E], b [E]}
   * shared by the scales, their kernels [k,k,E+C,4C]; the graph attention sees h alone.
   * scene_conv_kernel and simaug_graph then have no effect; mv_inputs.obs_scene / scene_feat and
   * mv_inputs_compact.obs_scene / scene_feat_u8 may be NULL and are never read; mv_attack_*,
   * mv_set/get_scene_feat, mv_get_scene_grad, mv_scene_mix and mv_set_label_mixup fail. */
  int32_t scene_conv_dim, scene_conv_kernel;    /* 64 (a multiple of 32 up to 128), 3 */
  int32_t emb_size;          /* 32 */
  int32_t hidden_size;       /* enc_hidden_size == dec_hidden_size, 256 */
  int32_t convlstm_kernel;   /* 3; other sizes 1 .. 9 run the generic fp32 loops (compute
                              * mode 0 only, csrc/convlstm_generic.h) */
  int32_t num_scales;        /* len(scene_grid_strides), <= MV_MAX_SCALES */
  int32_t grid_h[MV_MAX_SCALES];
  int32_t grid_w[MV_MAX_SCALES];
  int32_t use_grid[MV_MAX_SCALES];
  int32_t use_gnn;           /* --use_gnn */
  int32_t beam_size;         /* 1 = greedy (pred_models.py:260-285) */
  int32_t diverse_beam;      /* --diverse_beam */
  float   diverse_gamma;     /* --diverse_gamma */
  int32_t fix_num_timestep;  /* --fix_num_timestep */
  /* --use_teacher_forcing at TEST time: decoder_loop_fn takes its teacher_forcing branch
   * (code/pred_models.py:388-406), whose not-training arm feeds hidden2grid(h') itself --
   * raw logits, no argmax / one-hot -- to the class decoder's grid_emb.  0 = the
   * published one-hot feedback. */
  int32_t class_feedback_dense;
  /* --use_single_decoder (code/pred_models.py:274,287-296; "# bad" in code/train.py:98): no
   * regression decoder; the offsets are hidden2grid(class-decoder states) through ONE
   * kernel "person_pred/decode_reg/out_dec_grid/W" shared by the scales.  The regression
   * encoder's variables still exist (it is built, :232-234) but are neither run nor
   * trained.  Greedy decode and training; refused with beam search (the reference's
   * inference script reshapes the [N*B, ...] offsets of that combination as [1, T, -1, 2],
   * code/multifuture_inference.py:478). */
  int32_t use_single_decoder;
  /* 1 = the graph of SimAug/code/pred_models.py (the fork N4 trains with): its gnn_edge
   * concatenates the scene features to the hidden state only under tile_to_beam
   * (SimAug/code/pred_models.py:1219-1227), so the GREEDY decoder's graph attention -- test
   * and training -- sees the hidden state alone; the beam-search decoder is unchanged.
   * Found by executing that file on the TF-1 shim next to code/pred_models.py. */
  int32_t simaug_graph;
  /* --activation_func (code/train.py:58-59, code/pred_utils.py:86-94): the activation of
   * the scene convolutions (code/pred_models.py:155-165) and of grid_emb (:444, :664).
   * 0 = tanh (published), 1 = relu, 2 = lrelu (tf.nn.leaky_relu, alpha 0.2).  relu / lrelu
   * outputs are unbounded: in compute mode 1 their x operand planes carry a per-tensor
   * power-of-two scale taken from max |x| (DESIGN.md section 3c "x exponent"), so every
   * compute mode decodes AND trains them.  In compute mode 2 (bf16) the x k-steps of such a
   * model run as an f16x3 split of the x part alone (fp16 planes under that exponent, three
   * fp16 MFMAs per product) while the h k-steps stay one bf16 plane: one bf16 plane of a
   * pixel-offset embedding of hundreds had cost the regression decoder's kernel gradient its
   * direction (cosine 0.96 vs the fp32 oracle; now 0.99995, the tanh models' figure). */
  int32_t activation;
} mv_config;

/* The feed_dict of Model.get_feed_dict (pred_models.py:1042-1194), minus the
 * placeholders the forward graph never consumes. */
typedef struct mv_inputs {
  const int32_t* obs_scene;        /* [N, T_o] row index into scene_feat */
  const float*   scene_feat;       /* [U, SH, SW, SC] 0/1 masks */
  int32_t        num_scene_frames; /* U */
  int32_t        pred_len;         /* run-time T_pred (<= max_pred_len) */
  const int32_t* grid_obs_labels[MV_MAX_SCALES];   /* [N, T_o] */
  const float*   grid_obs_regress[MV_MAX_SCALES];  /* [N, T_o, H, W, 2] */
} mv_inputs;

/* Fetches of Tester.step (pred_models.py:1774-1790).  Pointers for unused
 * scales may be NULL. */
typedef struct mv_outputs {
  float* grid_pred_class[MV_MAX_SCALES]; /* [N, T_p, H, W, 1] logits */
  float* grid_pred_reg[MV_MAX_SCALES];   /* [N, T_p, H, W, 2] */
} mv_outputs;

/* model.beam_outputs (pred_models.py:276, 805-806) + the two greedy fetches
 * of multifuture_inference.py:468-472 for the single active scale. */
typedef struct mv_beam_outputs {
  float*   best_beam;   /* [N, T, H, W, 1]  == logits[:, 0] */
  float*   grid_reg;    /* [N, T, H, W, 2]  (regression decoder, un-beamed); with
                         * use_single_decoder [N*B, T, H, W, 2]: the offsets decoded from the
                         * class decoder's states traced back along every beam
                         * (code/pred_models.py:287-296) */
  float*   logits;      /* [N, B, T, H*W] */
  int32_t* ids;         /* [N, B, T] */
  float*   logprobs;    /* [N, B] */
} mv_beam_outputs;

/* -- training step: Trainer (pred_models.py:1636-1742) ------------------- */
/* The optimizer / loss fields Trainer.__init__ and Model.build_loss read from
 * the config (train.py:25-138 after process_args). */
typedef struct mv_train_config {
  /* --optimizer (code/pred_models.py:1667-1681): 0 adadelta (published), 1 momentum
   * (0.9), 2 adam, 3 rmsprop; TF-1.15 defaults and ApplyXxx kernel arithmetic */
  int32_t optimizer;
  float   init_lr, emb_lr;
  int32_t use_cosine_lr;      /* --use_cosine_lr */
  int32_t has_decay;          /* learning_rate_decay is not None */
  float   learning_rate_decay;
  int32_t decay_steps;        /* int(train_num_examples / batch_size * num_epoch_per_decay) */
  int32_t max_steps;          /* cosine: int(train_num_examples / batch_size * num_epochs) */
  int32_t do_clip;            /* clip_gradient_norm is not None */
  float   clip_gradient_norm; /* ELEMENT-WISE clip_by_value bound (pred_models.py:1700-1705) */
  float   wd;                 /* weight decay on every variable named .../W */
  float   grid_loss_weight, grid_reg_loss_weight;
  /* --- switches of Model.build_forward / build_loss beyond the published run --- */
  /* class-decoder next input while training (decoder_loop_fn, :388-436):
   *   0  one_hot(argmax(hidden2grid(h')))   --train_w_onehot (published; no gradient)
   *   1  hidden2grid(h') itself             neither flag (differentiable feedback)
   *   2  the ground-truth map of the step   --use_teacher_forcing (pred_gt.read(time)) */
  int32_t class_feedback;
  int32_t reg_teacher_forcing;   /* regression decoder: 0 own output, 1 ground truth */
  /* --use_soft_grid_class (:974-990, 1077-1124): labels = the one-hot map stamped with
   * the --soft_grid kernel (soft_kernel_size 3 or 5, row-major soft_kernel); the loss is
   * softmax_cross_entropy_with_logits with TF's registered gradient softmax - labels */
  int32_t use_soft_grid_class;
  int32_t soft_kernel_size;
  float   soft_kernel[25];
  int32_t mask_grid_regression;  /* --mask_grid_regression (:999-1018) */
  float   keep_prob;             /* DropoutWrapper input keep probability (:130-132) */
} mv_train_config;

/* Training-only placeholders of Model.get_feed_dict(is_train=True)
 * (pred_models.py:1149-1152). */
typedef struct mv_targets {
  const int32_t* grid_pred_labels[MV_MAX_SCALES];   /* [N, T_p] */
  const float*   grid_pred_regress[MV_MAX_SCALES];  /* [N, T_p, H, W, 2] */
} mv_targets;
/* (soft labels, the teacher-forcing inputs and the foreground mask of the masked
 * regression loss are all functions of grid_pred_labels: the engine builds them in HBM) */

/* Fetches of Trainer.step: loss, wd_loss, pred_grid_loss = [cls_s, reg_s, ...]
 * over the enabled scales (pred_models.py:1029, 1719-1742). */
typedef struct mv_losses {
  float   loss, wd_loss;
  float   pred_grid_loss[2 * MV_MAX_SCALES];
  int32_t num_pred_grid_loss;
} mv_losses;

/* -- lifetime ------------------------------------------------------------ */
int  mv_create(const mv_config* cfg, int device, mv_handle* out);
int  mv_destroy(mv_handle h);
const char* mv_last_error(mv_handle h);
int  mv_abi_version(void);

/* -- weights: tf.train.Saver role (pred_utils.py:149-205) ---------------- */
/* tf_name e.g. "person_pred/decoder_grid_class_0/decoder_rnn/dec_grid_0/kernel" */
int  mv_set_param(mv_handle h, const char* tf_name, const float* data,
                  const int64_t* shape, int32_t rank);
int  mv_get_param(mv_handle h, const char* tf_name, float* out,
                  int64_t capacity_elems);
int  mv_num_params(mv_handle h);
/* name/shape of the i-th parameter the engine expects; rank is returned */
int  mv_param_info(mv_handle h, int32_t i, char* name_out, int32_t name_cap,
                   int64_t* shape_out /* [4] */);

/* -- forward: one call == one sess.run ------------------------------------ */
int  mv_forward_greedy(mv_handle h, const mv_inputs* in, mv_outputs* out);
int  mv_forward_beam(mv_handle h, const mv_inputs* in, mv_beam_outputs* out);

/* -- resident-input variants (bench: inputs already in HBM) -------------- */
int  mv_upload_inputs(mv_handle h, const mv_inputs* in);   /* H2D + sync */

/* Device-side batch assembly.  The dense regression maps the graph
 * consumes are a pure function of one (x, y) per trajectory step,
 *   map[n, t, h, w, :] = (float)((double)xy[n, t, :] - centre[h, w, :])
 * (code/preprocess.py:463-475: float32 trajectory minus float64 grid centres, stored
 * as float32), and the scene masks are 0/1 bytes in data_*.npz (preprocess.py:831).
 * The compact forms hand over 16 bytes per step instead of 2*H*W*4 per scale and
 * uint8 masks; the engine expands both in HBM, bit-identical to the dense upload.
 * Rows n >= num_rows (the batcher's padding, code/pred_models.py:1070-1191) get zero
 * maps.  mv_set_grid_centers once per scale (data["grid_center_<s>"], float64
 * [H, W, 2]); then mv_upload_inputs_compact (+ mv_upload_targets_compact when
 * training) and the resident calls (mv_run_*_resident, mv_train_step(h, NULL, NULL, ..)). */
typedef struct mv_inputs_compact {
  const int32_t* obs_scene;        /* [N, T_o] row index into scene_feat_u8 */
  const uint8_t* scene_feat_u8;    /* [U, SH, SW, SC] 0/1 masks */
  int32_t        num_scene_frames; /* U */
  int32_t        pred_len;         /* run-time T_pred (<= max_pred_len) */
  const int32_t* grid_obs_labels[MV_MAX_SCALES];   /* [N, T_o] */
  const double*  obs_xy;           /* [N, T_o, 2] pixel coordinates */
  int32_t        num_rows;         /* rows that carry data (<= N) */
} mv_inputs_compact;

typedef struct mv_targets_compact {
  const int32_t* grid_pred_labels[MV_MAX_SCALES];  /* [N, T_p] */
  const double*  pred_xy;          /* [N, T_p, 2] */
  int32_t        num_rows;
} mv_targets_compact;

int  mv_set_grid_centers(mv_handle h, int32_t scale, const double* centers /* [H, W, 2] */);
int  mv_upload_inputs_compact(mv_handle h, const mv_inputs_compact* in);
int  mv_upload_targets_compact(mv_handle h, const mv_targets_compact* tg);
/* Pipelined greedy forward.  One sess.run of the reference is feed + compute + fetch in turn
 * (code/pred_models.py:1761-1790); an evaluation loop (code/pred_utils.py:415) knows its next
 * batch while the current one computes.  mv_submit_greedy copies the caller's buffers (free
 * again on return) into one of `depth` pinned slots and queues H2D -> forward -> D2H on the
 * engine's copy and compute streams; mv_collect_greedy blocks for the OLDEST submission and
 * fills `out` (sized for that submission's pred_len, returned through *pred_len when not
 * NULL).  At most `depth` submissions may be outstanding.  Results are bitwise those of
 * mv_forward_greedy. */
int  mv_pipeline_create(mv_handle h, int32_t depth);
int  mv_submit_greedy(mv_handle h, const mv_inputs* in);
int  mv_collect_greedy(mv_handle h, mv_outputs* out, int32_t* pred_len);
int  mv_run_greedy_resident(mv_handle h);   /* enqueue on the handle's stream */
int  mv_run_beam_resident(mv_handle h);
int  mv_synchronize(mv_handle h);
int  mv_download_outputs(mv_handle h, mv_outputs* out);
int  mv_download_beam_outputs(mv_handle h, mv_beam_outputs* out);
/* Multi-future decode of the LAST forward, on the device (code/multifuture_inference.py:475-517,
 * code/multifuture_eval_trajs_prob.py:19-34, 88-93): what a caller wants from a decode is
 * [N, B, T_p, 2] trajectories and, for the grid-NLL evaluation, one [N, T_p, K] occupancy map,
 * not every beam's logits.  Both calls run on the handle's stream behind whatever forward was
 * queued (mv_run_*_resident, mv_forward_*), copy their result to `out` and synchronise.
 * mv_decode_trajectories: out[n, b, t, :] = centre[id] (+ offset[n, t, id, :] unless
 *   center_only), doubles, B = beam_size; id = the beam's cell on a beam handle (its single
 *   active scale; `scale` is ignored), argmax_k of the class logits of `scale` (first index of
 *   the maximum) on a greedy handle (B = 1).  The centres are those of mv_set_grid_centers;
 *   double centre + widened float offset is the reference's own operation: bit-identical.
 * mv_beam_occupancy (beam handles): out[n, t, k] = sum_b softmax_b(logprobs[n, :])[b] *
 *   softmax_k(logits[n, b, t, :])[k], float32 throughout, bitwise reproducible.
 * Errors: no forward has run; the centres of the scale were never set; mv_beam_occupancy on
 * a greedy handle; either call on a use_single_decoder beam handle (host decode only). */
int  mv_decode_trajectories(mv_handle h, int32_t scale, int32_t center_only, double* out);
int  mv_beam_occupancy(mv_handle h, float* out /* [N, T_p, K] */);
/* the small members of mv_download_beam_outputs on their own (beam handles, after a forward):
 * ids [N, B, T_p], logprobs [N, B]; either may be NULL */
int  mv_download_beam_ids(mv_handle h, int32_t* ids, float* logprobs);
/* Per-row prediction lengths: one forward decodes samples of different lengths.  lengths[n] =
 * L[n] in [0, pred_len] (checked at the forward; pred_len is the forward's mv_inputs.pred_len);
 * NULL clears.  Sticky until cleared; applies to mv_forward_*, mv_run_*_resident, the downloads
 * and the three multi-future decode calls above.  Every output keeps its shape (time dimension
 * pred_len).  For t < L[n], row n of every output is bit-identical to row n of a uniform forward
 * of this engine with pred_len = L[n]: its beams are traced back from step L[n] - 1, its
 * logprobs are the scores after the selection at time L[n].  For t >= L[n]: greedy logits and
 * offsets, best_beam, beam logits, grid_reg, decoded trajectories and occupancy maps are 0, ids
 * are -1.  L[n] = 0 is a padding row: all 0 (ids -1).  Step t issues its launches on the prefix
 * of 1 + max{n : L[n] > t} rows, so lengths sorted descending launch no finished row; any order
 * is correct.  With all L[n] == pred_len the forward is the uniform one.  Keep the lengths set
 * until the last forward's outputs have been decoded.  While lengths are set, mv_train_* and
 * mv_submit_greedy fail with a message. */
int  mv_set_pred_lengths(mv_handle h, const int32_t* lengths /* [N]; NULL clears */);
/* Per-row observation lengths: one forward encodes tracks of different history lengths.
 * lengths[n] = Lo[n] in [1, obs_len] (checked at the forward); NULL clears.  Sticky until
 * cleared; applies to every forward kind (greedy, beam, sampled, sampled without replacement,
 * scored).  Row n's observations are RIGHT-ALIGNED: columns obs_len - Lo[n] .. obs_len - 1 of
 * obs_scene, grid_obs_labels[s], grid_obs_regress[s] (and obs_xy of the compact upload) hold
 * them, so the decoders' first inputs stay labels[:, -1] and obs_grid_reg[:, -1].  The columns
 * before them are ignored: they must hold in-range labels / frame indices and finite floats (the
 * upload checks read them), and no output depends on them.
 * Meaning: row n of every output is, bit for bit, row n of a uniform forward of an engine
 * created with obs_len = Lo[n], the same weights, fed the row's last Lo[n] columns.  The encoders
 * start from the zero state at the row's first observation, and scene_mean is the mean over the
 * row's own Lo[n] frames, summed in ascending time order and divided by (float)Lo[n].  This is
 * the reference's model at another obs_len, NOT dynamic_rnn's left-aligned copy-through of a
 * sequence_length (the reference's obs_length placeholder, which its feed code always fills with
 * obs_len): that would take the decoders' first inputs from padding.
 * Encoder step t (0-based) issues each chain on the prefix of p_t = 1 + max{n < rows that decode
 * at all : Lo[n] >= obs_len - t} rows, and a step with no such row is not launched: lengths
 * sorted descending launch no unstarted row (sum_t p_t = sum_n Lo[n]); any order is correct.
 * Combines with mv_set_pred_lengths (row n equals the obs_len = Lo[n] engine's forward at
 * pred_len = L[n]).  With all Lo[n] == obs_len the forward is the uniform one, launch for launch;
 * otherwise it is issued eagerly in graph mode and the class encoder's light cone stays off, and
 * mv_train_*, mv_attack_begin / mv_attack_step and mv_submit_greedy fail with a message that
 * names the call. */
int  mv_set_obs_lengths(mv_handle h, const int32_t* lengths /* [N]; NULL clears */);
/* sum of the row counts over every ConvLSTM problem of every grouped gate launch of the last
 * forward (encoders and decoders): what the forward really launched, without timing anything */
int  mv_last_forward_gate_rows(mv_handle h, int64_t* rows);

/* ---- sampled multi-future decode (not in the reference; the draw is defined here) --------------
 * S = beam_size independent samples per row instead of beam search.  temperature > 0.
 * Sticky until mv_set_sampling(h, 0, ..).  Applies to mv_forward_beam, mv_run_beam_resident,
 * the beam downloads, mv_decode_trajectories, mv_beam_occupancy, mv_set_pred_lengths.
 *
 * Decode step t (0-based) of future s of batch row n, all in float32, K = cells of the grid:
 *   lp[k]    = log_softmax(hidden2grid logits of the step)[k]
 *   u[k]     = (top 24 bits of hash32(s*K + k, seed_n, t) + 0.5) * 2^-24, held below 1.0 (the
 *              last code rounds to 1.0 in float32: it becomes the largest float32 under 1);
 *              hash32(i, seed, stream) is the generator of the training dropout (below), and
 *              seed_n = seed + n * 0x632BE5AB (mod 2^32): batch row n draws as row 0 of a forward
 *              seeded seed_n does, whatever the batch around it, and future s draws the same
 *              noise for every beam_size > s
 *   id       = argmax_k lp[k] / temperature - log(-log(u[k])), lowest index among equal scores
 *   next input = grid_emb(one_hot(id));  logprobs[n, s] += lp[id]  (untempered)
 * Step 0 runs on the shared encoder state; there is no fix_num_timestep and no parent: future
 * (n, s) continues itself.  Outputs keep the beam's shapes: logits [N,S,T,K], ids [N,S,T],
 * logprobs [N,S] (futures in order s, unsorted), best_beam = future 0, grid_reg.
 * mv_beam_occupancy weights the futures uniformly (1/S).  Per-row lengths hold as for the
 * beam (the noise does not depend on them).  Graph mode: seed and temperature live in a device
 * buffer the step kernel reads, so a replayed graph follows this call.
 * Errors: a greedy handle, a use_single_decoder handle, temperature <= 0, a grid of more than
 * 1024 cells (at the forward); mv_train_* while sampling is on. */
int  mv_set_sampling(mv_handle h, int32_t enabled, float temperature, uint32_t seed);

/* ---- sampling WITHOUT replacement (not in the reference; defined here) -----------------------
 * Stochastic beam search (Kool, van Hoof, Welling, ICML 2019): the B = beam_size futures of a row
 * are DISTINCT and still a sample of the model -- a Gumbel-top-B over whole sequences, computed
 * top-down -- each with its exact log-probability.  mode 0 = independent draws (the default, the
 * sampler above), 1 = without replacement.  Sticky; stored while sampling is off, in effect while
 * sampling is on (mv_set_sampling(h, 1, temperature, seed)).  Everything is float32, K = cells.
 *
 * Slot b of batch row n carries phi (the tempered log-probability that drives the search), LP (the
 * untempered log-probability that is reported) and G (the slot's perturbed score).  Before the
 * first step there is one root per row with phi = LP = G = 0.  Decode step t (0-based), parent
 * slot b of row n, logits l:
 *   lp      = log_softmax(l), the arithmetic of the sampler and the scorer
 *   q       = lp when temperature == 1 (same bits), else log_softmax(l / temperature) formed the
 *             same way on the divided logits
 *   u[k]    = the sampler's uniform of (b*K + k, seed_n, t), b the PARENT's slot,
 *             seed_n = seed + n * 0x632BE5AB (mod 2^32);  gum[k] = -logf(-logf(u[k]))
 *   g[k]    = (phi_b + q[k]) + gum[k];  Z = max_k g[k];  d = g[k] - Z
 *   v       = (G_b - g[k]) + logf(-expm1f(d)) for d < 0, v = -inf for d == 0
 *   Gt[k]   = (G_b - fmaxf(v, 0)) - log1pf(expf(-fabsf(v)))
 * (the expm1 form, not log1p(-exp(d)): the best child of a parent gets Gt == G_b bit for bit).
 * The new slots are the B largest Gt over all (parent, k) of the row, in descending order, ties
 * to the lower flat index b*K + k.  At step 0 the candidates are the root's K children (the step
 * runs once per sample, as the beam's shared first step).  New slot j from (b, k) carries
 * phi = phi_b + q[k], LP = LP_b + lp[k], G = Gt[k], parent b, id k.  diverse_beam, diverse_gamma
 * and fix_num_timestep are not read.
 * Consequences: the B futures of a row are pairwise different id sequences; gumbels[n, :] is
 * non-increasing and <= 0 with gumbels[n, 0] == 0.0 exactly; slot 0 is an exact sample of the
 * (tempered) model; logprobs are exact untempered model log-probabilities; row n does not depend
 * on its batch; the futures of a width-B handle are the first B futures of any wider handle.
 * Outputs as the beam's: mv_download_beam_outputs / mv_download_beam_ids return the back-traced
 * ids and logits, logprobs = LP, best_beam = slot 0; mv_decode_trajectories works unchanged;
 * mv_beam_occupancy takes the BEAM's weighting softmax_b(logprobs) (the model's distribution
 * renormalised over the drawn distinct set), not the sampler's 1/B; per-row lengths hold as for
 * the beam (row n's LP and G are those after the selection at time L[n]); a replayed graph
 * follows mv_set_sampling.  mv_download_beam_gumbels: G [N, B] of the last forward of this kind.
 * Errors: a greedy handle, a mode outside {0, 1}; at the forward: use_single_decoder, a grid of
 * more than 1024 cells, beam_size > K; mv_download_beam_gumbels after a forward of another kind
 * (the message names it); mv_train_* while sampling is on. */
int  mv_set_sampling_mode(mv_handle h, int32_t mode);
int  mv_download_beam_gumbels(mv_handle h, float* out /* [N, B] */);

/* ---- truncated sampling: top-k and nucleus limits (not in the reference; defined here) -------
 * Cuts the tail of the step distribution both samplers draw from and keeps the temperature.  In
 * effect while sampling is on, in both sampling modes.  Everything is float32, K = cells, l = the
 * step's hidden2grid logits, tau = the temperature; top_k is an int32 >= 0 (0 = off), top_p a
 * float in (0, 1] (1 = off).  Per row, at decode step t:
 *   w[k]    = l[k] / tau (the division of the sampling without replacement);  mxq = max w
 *   e[k]    = expf(w[k] - mxq);  sum_e = their sum in the order of the log-softmax (per lane over
 *             j, lane owning k = lane + 64 j, then the wave butterfly); at tau = 1 the terms of lp
 *   c(k)    = #{j : l[j] > l[k]}  (strictly better, an integer)
 *   m(k)    = sum of e[j] over {j : l[j] > l[k]}, in that same order over the masked terms
 *   keep(k) = c(k) < floor, or both of
 *               top_k == 0 or c(k) < top_k
 *               top_p >= 1 or m(k) < top_p * sum_e
 * A top_p >= 1 is never evaluated: off means off (m(k) < sum_e is not guaranteed in float32).
 * floor is 1 everywhere except step 0 of a forward that samples without replacement, where it is
 * beam_size: the root needs B children.  With the floor no slot can lack a finite candidate.
 * Cells with exactly equal logits are kept or dropped together, so the kept set may exceed top_k
 * by a tie group; keep is an upper set of the logit order, described by one threshold.
 * The proposal is  q~[k] = (w[k] - mxq) - logf(sum of e over the kept cells)  on kept cells (that
 * sum in the same order) and -inf elsewhere.  Both limits off: q~ == lp bit for bit at tau = 1,
 * and q~ == the q of the sampling without replacement bit for bit at any other tau.
 * Independent mode: id = argmax over the KEPT k of lp[k] / tau + gum[k]; noise, tie rule and all
 * else as above.  logprobs[n, s] += lp[id] stays the model's exact, untruncated, untempered
 * log-probability (scoring the drawn ids reproduces it bit for bit); a second accumulator takes
 * qlogprobs[n, s] += q~[id] and stops at the row's length as logprobs does.
 * Without replacement: q~ replaces q in g, in the winner's phi and in the plane the selection
 * reads (written whenever tau != 1 or a limit is on).  A dropped cell is the candidate -inf and
 * is never selected.  LP, G and every consequence listed above hold: distinct futures,
 * gumbels[n, 0] == 0.0, exact LP.  qlogprobs is the final phi; a ragged forward captures it at
 * L[n] as it does LP and G.  One exception: "a width-B handle draws the first B futures of a
 * wider one" holds only while the step-0 floor does not widen either handle's kept set.
 * With both limits off every output of every call is bit-identical to a handle that never had
 * them.  Sticky; stored while sampling is off (as mv_set_sampling_mode); the limits live in the
 * sampler's device buffer {seed, tau bits, top_k, top_p bits}, so a replayed graph follows this
 * call without re-capture.
 * mv_download_beam_proposal_logprobs: qlogprobs [N, B] of the last forward, which must have been
 * a sampled one of either mode (the message names the kind otherwise).
 * Errors: a greedy handle; top_k < 0; top_p outside (0, 1] or NaN. */
int  mv_set_sampling_truncation(mv_handle h, int32_t top_k, float top_p);
int  mv_download_beam_proposal_logprobs(mv_handle h, float* out /* [N, B] */);

/* ---- constrained decode: per-row allowed cells (not in the reference; defined here) ---------
 * allowed [N, Tm, K] bytes, K = the cells of the handle's one used grid; allowed[n, tm, k] != 0
 * means row n may choose cell k.  Tm == 1: one mask for every decode step; otherwise step t reads
 * plane t, and Tm must be at least the forward's pred_len (checked at the forward).  NULL clears.
 * Sticky until cleared.  It applies to every forward of a beam handle that CHOOSES cells -- the
 * beam search, the independent sampler, the sampling without replacement -- and to
 * mv_beam_occupancy after them.  mv_score_futures neither reads nor changes it: the likelihood of
 * a given future is the model's.  Everything is float32; A = A(n, t) is the allowed set of the row
 * at the step, l the step's hidden2grid logits, tau the temperature.
 *   lp = log_softmax(l) over ALL K cells, unchanged: logprobs of both samplers stay the model's
 *        exact log-probabilities (scoring the returned ids with mv_score_futures reproduces them
 *        bit for bit), and the logits outputs are the model's, unmasked.
 * Beam search: after lp + prev_lp and BEFORE the diversity ranks a cell outside A becomes the
 * candidate -inf.  The rank and penalty arithmetic then runs as it is -- a -inf candidate precedes
 * nothing, so an allowed cell's rank counts allowed cells only -- and the selection is unchanged.
 * With a mask the step always takes the two-launch rank + select form, whatever MV_BEAM_STEP says.
 * Independent sampler and sampling without replacement: a cell outside A is treated exactly as a
 * cell past K, i.e. absent from the proposal.  In the terms of mv_set_sampling_truncation:
 *   w[k]    = l[k] / tau;  mxq = max of w over A  (deliberately over A: with the row maximum
 *             outside A every allowed e could underflow and q~ would not be finite)
 *   e, sum_e, c(k), m(k) and the step-0 floor run over A
 *   keep(k) = k in A and the predicate of mv_set_sampling_truncation
 *   q~[k]   = (w[k] - mxq) - logf(sum of e over the kept cells) on kept cells, that sum in the
 *             order of the log-softmax; -inf elsewhere
 * A mask makes the proposal differ from the model: qlogprobs accumulates q~[id], and the
 * without-replacement q plane is written and read, whenever a mask is set -- even at tau == 1 with
 * no limit.  mv_download_beam_proposal_logprobs returns it as under a limit.
 * mv_beam_occupancy: each future's step map is the softmax over A (maximum and sum over A, a cell
 * outside exactly 0.0f); the mixture weights are unchanged.  It reads the mask that is set when
 * it is called.
 * Identity, in eager and in graph mode: with allowed all non-zero every output of every call is
 * bit-identical to a handle that never had a mask; with no mask set no launch differs.
 * Validity: the allowed cells per (n, tm) are counted on the host when the mask is set and checked
 * at the forward, for rows that decode at all and steps below the row's length:
 *   |A(n, t)| >= 1 at every such step;  |A(n, 0)| >= beam_size for the beam search and for the
 *   sampling without replacement (only the root's K children are candidates at the first step).
 * The message names n, t and the count.  With these no slot ever lacks a finite candidate: a dead
 * beam cannot occur and is not defined.
 * The mask lives in an engine-owned device buffer; this call synchronises the stream and rewrites
 * it, so a replayed graph follows a new mask without re-capture (the graph key carries whether a
 * mask is set and whether Tm > 1).  It combines with mv_set_pred_lengths and mv_set_obs_lengths
 * with no new rule: row n equals its own uniform forward under the same mask row.
 * Errors: a greedy handle (the constrained argmax decode is the beam search of width 1 without
 * diversity, which a greedy handle does not run: its forward reads no mask); Tm < 1;
 * 1 < Tm < pred_len (at the forward); a grid of more than 1024 cells (at the forward); mv_train_*
 * and mv_submit_greedy while a mask is set (the message names the call). */
int  mv_set_cell_mask(mv_handle h, const uint8_t* allowed /* [N, Tm, K]; NULL clears */,
                      int32_t Tm);
/* forwards captured into a hipGraph on this handle so far (a replay does not count) */
int  mv_graph_captures(mv_handle h, int64_t* captures);

/* ---- cell costs: per-row additive logit bias (not in the reference; defined here) -------------
 * bias [N, Tm, K] float32, K = the cells of the handle's one used grid: b[n, tm, k] is a
 * log-potential, in nats, that row n's choice of cell k carries beside the model's own -- a map
 * cost, a goal heat-map, another model's occupancy.  Negative = less likely.  Tm == 1: one plane
 * for every decode step; otherwise step t reads plane t, and Tm must be at least the forward's
 * pred_len (checked at the forward).  NULL clears.  Sticky until cleared.  It applies to the
 * forwards that mv_set_cell_mask applies to, and to mv_beam_occupancy after them;
 * mv_score_futures neither reads nor changes it.  A mask is the special case "cost = -inf", and
 * stays the mask's job: every value here is finite.  Notation as above: l the step's logits, tau
 * the temperature, A the allowed set (all K cells when no mask is set), b the row's plane.
 *   lp = log_softmax(l) over ALL K cells, unchanged: the logits outputs and both samplers'
 *        logprobs stay the model's, and scoring the returned ids with mv_score_futures reproduces
 *        logprobs bit for bit.
 * Beam search: the candidate is (prev_lp + lp) + b, formed BEFORE the mask's -inf and before the
 * diversity ranks; ranks, penalty and selection run as they are.  The carried and returned beam
 * score therefore includes the bias, as it includes the diversity penalty.  With a bias the step
 * takes the two-launch rank + select form, as under a mask.
 * Independent sampler and sampling without replacement: the proposal's
 *   w[k]    = l[k] / tau + b[k], -inf outside A;  mxq = max of w over A
 *   e, sum_e, c(k), m(k), the step-0 floor and q~ are as documented for the mask, over THIS w;
 *             in particular the order of the top-k and nucleus limits is the order of w, not of l:
 *             c(k) = #{j in A : w[j] > w[k]}, m(k) the sum of e over that set
 *   the independent sampler's score is (lp[k] / tau + b[k]) + g[k]
 * qlogprobs, and the without-replacement q plane, are written whenever a bias is set -- also at
 * tau == 1 with no limit -- and mv_download_beam_proposal_logprobs returns them as under a limit.
 * mv_beam_occupancy: each future's step map is the softmax of l + b over A; the mixture weights
 * are unchanged.  It reads the bias that is set when it is called.
 * Identity, in eager and in graph mode: with no bias set no launch differs (the same kernels, the
 * same graph keys, mv_graph_captures unchanged); with an all-zero bias every output that both
 * handles define is bit-identical to a handle that never had one.
 * The bias lives in an engine-owned device buffer; this call synchronises the stream and rewrites
 * it, so a replayed graph follows a new bias without re-capture (the graph key carries whether a
 * bias is set and whether Tm > 1).  It combines with mv_set_cell_mask, mv_set_pred_lengths and
 * mv_set_obs_lengths with no new rule: row n equals its own uniform forward under its own bias row.
 * Errors: a greedy handle; Tm < 1; a value that is NaN or +-inf (checked on the host here; the
 * message names n, tm and k); 1 < Tm < pred_len (at the forward); a grid of more than 1024 cells
 * (at the forward); mv_train_* and mv_submit_greedy while a bias is set (the message names the
 * call). */
int  mv_set_cell_bias(mv_handle h, const float* bias /* [N, Tm, K]; NULL clears */, int32_t Tm);

/* ---- motion costs: per-row speed and turn priors (not in the reference; defined here) ---------
 * A cell bias whose plane depends on the path so far: what a step costs depends on how far it
 * moves from the path's last cell (a speed prior or limit) and on how much that move differs from
 * the move before it (a turn prior).  The grid is the handle's one used scale, H x W,
 * K = H * W <= 1024; cell k is (y, x) = (k / W, k % W), as multifuture.xy_to_grid_class numbers
 * them.  For the row or slot (n, s) at decode step t:
 *   p1 = the cell the row's path holds at step t - 1; at t == 0 the row's last observed label,
 *        labels[n, obs_len - 1].
 *   p0 = the cell before p1 on the same path: at t == 1 labels[n, obs_len - 1], at t == 0
 *        labels[n, obs_len - 2]; ABSENT at t == 0 for a row whose observation length
 *        (mv_set_obs_lengths; obs_len without it) is 1.
 *   Beam search and sampling without replacement: a slot's path is its parent's path, the order
 *        of the back-trace: p1 = ids[t-1][n, slot], p0 = ids[t-2][n, parents[t-1][n, slot]].
 *   d(k) = cell(k) - cell(p1),  u = cell(p1) - cell(p0),  a(k) = d(k) - u, each a pair of ints
 *        (rows, columns).
 * With radius R (1 .. MV_MOTION_MAX_RADIUS) and D = 2 R + 1:
 *   vterm(k) = vel[n, d.y + R, d.x + R] if max(|d.y|, |d.x|) <= R, else vel_far[n]
 *   aterm(k) = acc[n, a.y + R, a.x + R] if max(|a.y|, |a.x|) <= R, else acc_far[n];
 *              exactly 0.0f when no acc table is set or p0 is absent
 *   b_eff[k] = (b[k] + vterm(k)) + aterm(k)   in float32, in this order; b is the row's cell-bias
 *              plane of the step (mv_set_cell_bias), or 0.0f when no bias is set.
 * Everything mv_set_cell_bias defines then holds with b_eff in place of b: the beam candidate
 * (prev_lp + lp) + b_eff, formed before the mask's -inf and before the diversity ranks; the
 * samplers' w = l / tau + b_eff and the limits ordered by w; qlogprobs and the without-replacement
 * q plane, written whenever a motion cost is set; the two-launch beam step; lp, logits and
 * logprobs stay the model's; mv_score_futures neither reads nor changes it, so scoring the
 * returned ids reproduces logprobs bit for bit.  The carried and returned beam score includes
 * every step's vterm + aterm (multifuture.path_motion_cost recomputes them on the host).
 * Every table value is finite.  A speed LIMIT is the cost -1e30: exp(w - mxq) of such a cell is
 * exactly 0, so the samplers never draw it while a cheaper cell is allowed.  The beam search and
 * the sampling without replacement SELECT beam_size candidates: a slot that cannot be filled from
 * inside the windows takes an outside cell and carries the -1e30 in its score (for example at
 * step 0, where only the root's K children are candidates, with fewer in-window cells than
 * beam_size).  That is defined and deterministic (ties by index); the caller filters on the score.
 * Stickiness, the forwards it applies to, and how it combines with mv_set_cell_mask,
 * mv_set_cell_bias, mv_set_pred_lengths and mv_set_obs_lengths are the bias's: row n equals its
 * own uniform forward under its own tables.  The tables live in one engine-owned device
 * allocation; this call synchronises the stream and rewrites it.  The graph key carries whether a
 * motion cost is set, its radius and whether acc is present, so a replay follows new table VALUES
 * without re-capture.
 * Identity, eager and graph: with none set no launch differs (the same kernels, the same graph
 * keys, mv_graph_captures unchanged).  With all-zero tables and zero far values every output that
 * both handles define is bit-identical to the same handle without a motion cost.  (b + 0.0f turns
 * a bias of -0.0f into +0.0f; the two differ in no comparison and in no sum with a non-zero term.)
 * Errors, each message naming its cause: a greedy handle; radius outside 1 .. 4; a NaN or +-inf
 * (the message names the table, n and the entry); acc / acc_far not both or neither; a grid of
 * more than 1024 cells (at the forward); mv_train_*, mv_submit_greedy and mv_beam_occupancy while
 * one is set (the message names the call: the occupancy map under a path-dependent plane is not
 * defined here). */
#define MV_MOTION_MAX_RADIUS 4
int  mv_set_motion_cost(mv_handle h, int32_t radius,
                        const float* vel     /* [N, D, D]; NULL clears */,
                        const float* vel_far /* [N] */,
                        const float* acc     /* [N, D, D] or NULL: no turn term */,
                        const float* acc_far /* [N]; NULL exactly when acc is */);

/* ---- revisit cost: a per-row penalty for paths that return to a cell they left (not in the
 * reference; defined here) ------------------------------------------------------------------
 * The first constraint on a WHOLE path: what a step costs depends on every cell the path has held,
 * not on its last two.  The grid, the cell numbering, p1, the parent order of a slot's path and
 * the condition K <= 1024 are those of mv_set_motion_cost.  For the row or slot (n, s) at decode
 * step t the visited set V is
 *   with seed_observed != 0: the row's own observed cells labels[n, obs_len - Lo[n] .. obs_len - 1]
 *        (Lo[n] from mv_set_obs_lengths, obs_len without it; the columns in front of a short track
 *        are not read),
 *   plus the cells its path holds at steps 0 .. t - 1: the back-traced ids through the parents for
 *        the beam search and the sampling without replacement, the row's own ids for the
 *        independent sampler.
 *   rterm(k) = cost[n] if k is in V and k != p1, else exactly 0.0f.  Staying in the current cell is
 *        never a revisit (a cell is about 60 px wide and a pedestrian often stays); the path
 *        A, A, B, A pays once, at its last step.
 *   b_eff[k] = b_m[k] + rterm(k)   in float32; b_m is the motion b_eff of mv_set_motion_cost when a
 *        motion cost is set, otherwise the step's bias plane, or 0.0f without one.
 * Everything mv_set_cell_bias and mv_set_motion_cost define then holds with this b_eff: the beam
 * candidate (prev_lp + lp) + b_eff, formed before the mask's -inf and before the diversity ranks;
 * the samplers' w = l / tau + b_eff and the limits ordered by w; qlogprobs and the
 * without-replacement q plane, written whenever a revisit cost is set; the two-launch beam step;
 * lp, logits and logprobs stay the model's; the carried and returned beam score includes every
 * step's rterm (multifuture.path_revisit_cost recomputes them on the host).  mv_score_futures
 * neither reads nor changes the cost.
 * cost[n] is any finite float.  0 is the identity.  -1e30 means "never", with the semantics of the
 * motion LIMIT: the samplers never draw such a cell while another is allowed, and a beam or
 * without-replacement slot that cannot be filled otherwise takes one, deterministically (ties by
 * index), and carries the -1e30 in its score.
 * Sticky as the motion cost is, and combined with mv_set_cell_mask, mv_set_cell_bias,
 * mv_set_motion_cost, mv_set_pred_lengths and mv_set_obs_lengths in the same way: row n equals its
 * own uniform forward under its own cost.  The call synchronises the stream and rewrites one
 * engine-owned allocation; the visited sets live in a second one (256 B per row and step parity),
 * maintained by the step kernels themselves: no launch is added.  The graph key carries whether a
 * cost is set and seed_observed, not the values, so a replay follows new values without
 * re-capture.
 * Identity, eager and graph: with none set no launch differs (the same kernels, the same graph
 * keys, mv_graph_captures unchanged).  With all-zero costs every output that both handles define
 * is bit-identical to the handle without one (b + 0.0f turns a bias of -0.0f into +0.0f, as under
 * a motion cost).
 * Errors, each message naming its cause: a greedy handle; a NaN or +-inf (the message names n); a
 * grid of more than 1024 cells (at the forward); mv_train_*, mv_submit_greedy and
 * mv_beam_occupancy while one is set. */
int  mv_set_revisit_cost(mv_handle h, const float* cost /* [N]; NULL clears */,
                         int32_t seed_observed);

/* ---- scoring given futures (not in the reference) ------------------------------------------
 * The teacher-forced log-likelihood of F = beam_size GIVEN futures per batch row under the class
 * decoder: the forward of mv_set_sampling with every id given instead of drawn.  Decode step t
 * of future (n, f), float32, K = cells of the grid, id = ids[n, f, t], for t < lengths[n, f]:
 *   lp                     = log_softmax(hidden2grid logits of the step), the arithmetic of the
 *                            sampled decode: scoring the ids a sampled forward drew returns its
 *                            logprobs bit for bit
 *   step_logprobs[n, f, t] = lp[id];  logprobs[n, f] += lp[id];  next input = grid_emb(one_hot(id))
 *   ranks[n, f, t]         = number of cells k whose logit is greater than logit[id], or equal
 *                            with k < id (0: the given cell is the model's argmax)
 * and for t >= lengths[n, f]: step_logprobs 0, ranks -1.  Lengths are per future, in
 * [0, pred_len]; 0 is a padding future, a sample whose futures are all 0 a padding sample.  The
 * forward decodes sample n for max_f lengths[n, f] steps and does not launch finished samples
 * (order the batch by that maximum, descending, as for mv_set_pred_lengths); it is ragged, and
 * issued eagerly in graph mode, unless every length is pred_len.  Ids at t >= lengths[n, f] are
 * not read.  In graph mode the uniform forward is a graph of its own whose ids live in an
 * engine-owned buffer: a replay scores the latest upload.
 * Afterwards mv_download_beam_outputs / mv_download_beam_ids return logits [N,F,T,K] (0 from
 * step lengths[n, f] on), the given ids (-1 from there on), logprobs and grid_reg (0 from the
 * sample's maximum on), mv_decode_trajectories returns centre + the model's offset along the
 * given cells ((0, 0) past a future's length), and mv_last_forward_gate_rows counts the launch.
 * Scoring is not sticky and neither reads nor changes mv_set_sampling: the next beam forward
 * and mv_train_* are unaffected.
 * Errors: a greedy handle, a use_single_decoder handle, a grid of more than 1024 cells (at the
 * forward), an id outside [0, K) at t < length (checked on the host at upload; the message
 * names n, f, t), a length outside [0, pred_len], mv_set_pred_lengths set at the same time,
 * mv_run_score_resident without uploaded futures or after an mv_upload_inputs with another
 * pred_len, mv_beam_occupancy after a scoring forward (given futures are no predictive
 * mixture), mv_download_scores after another kind of forward. */
typedef struct {
  const int32_t* ids;      /* [N, F, pred_len], F = beam_size */
  const int32_t* lengths;  /* [N, F] in [0, pred_len]; NULL = all pred_len */
} mv_score_futures_in;
typedef struct {           /* each may be NULL */
  float* step_logprobs;    /* [N, F, pred_len] */
  float* logprobs;         /* [N, F] = sum over t < length, in step order */
  int32_t* ranks;          /* [N, F, pred_len] */
} mv_score_outputs;

/* upload + run + download */
int  mv_score_futures(mv_handle h, const mv_inputs* in, const mv_score_futures_in* fut,
                      mv_score_outputs* out);
/* after mv_upload_inputs (which sets pred_len) */
int  mv_upload_score_futures(mv_handle h, const mv_score_futures_in* fut);
int  mv_run_score_resident(mv_handle h);
int  mv_download_scores(mv_handle h, mv_score_outputs* out);
int  mv_time_score_resident(mv_handle h, int32_t iters, float* ms_out);

/* -- training: one call == sess.run([loss, train_op, wd_loss, pred_grid_loss]) */
int  mv_train_init(mv_handle h, const mv_train_config* tc);
/* forward (is_train, --train_w_onehot wiring) + loss + backward + clip +
 * Adadelta + global_step++ on one device */
int  mv_train_step(mv_handle h, const mv_inputs* in, const mv_targets* tg,
                   mv_losses* out);
/* data-parallel form: gradients of the LOCAL batch mean are left in one flat
 * device buffer (mv_grad_buffer) for the caller's all-reduce(sum) over the
 * ranks (RCCL via torch.distributed), then mv_train_apply(1/world) clips,
 * applies Adadelta and advances global_step -- clip AFTER the all-reduce, as a
 * single-device step over the global batch would. */
int  mv_train_forward_backward(mv_handle h, const mv_inputs* in,
                               const mv_targets* tg, mv_losses* out);
/* resident form (bench: batch already in HBM): mv_upload_inputs +
 * mv_upload_targets once, then pass in == tg == NULL to the two calls above */
int  mv_upload_targets(mv_handle h, const mv_targets* tg);
int  mv_grad_buffer(mv_handle h, float** device_ptr, int64_t* elems);
int  mv_train_apply(mv_handle h, float grad_scale);
/* Per-row TRAINING lengths: one training step over rows of different history and horizon.
 * obs_lengths[n] = Lo[n] in [1, obs_len], pred_lengths[n] = L[n] in [0, pred_len] (pred_len is
 * the step's mv_inputs.pred_len); both are checked at the step, whose message names n and the
 * value.  Either pointer NULL means that side is uniform (obs_len / pred_len for every row);
 * both NULL clears.  Sticky until cleared.  Read ONLY by mv_train_step and
 * mv_train_forward_backward (their resident forms included): no inference forward reads it, and
 * mv_set_pred_lengths / mv_set_obs_lengths stay the forward's and keep refusing training.
 * L[n] = 0 is a padding row: it contributes nothing, whatever its inputs hold.  At least one
 * row must have L[n] > 0.
 * Row layout (the forward's): observations RIGHT-ALIGNED in columns obs_len - Lo[n] ..
 * obs_len - 1; targets (grid_pred_labels, grid_pred_regress, pred_xy of the compact upload, the
 * soft maps made from them) LEFT-ALIGNED in columns 0 .. L[n] - 1.  The ignored columns must
 * hold in-range labels / frame indices and finite floats (the upload checks read them); no loss
 * and no gradient bit depends on them.
 * Model per row: row n is the reference's model at obs_len = Lo[n], pred_len = L[n].  The
 * encoders start from the zero state at the row's first observation; scene_mean is taken over
 * the row's own frames, summed in ascending time order and divided by (float)Lo[n]; the
 * decoders' first inputs are the last observed column; decode steps t >= L[n] do not exist for
 * the row.
 * Loss: with M = sum_n L[n], per used scale
 *   cls_loss = grid_loss_weight * (1/M) sum_n sum_{t < L[n]} ce(n, t)
 *   reg_loss = grid_reg_loss_weight * (1/(2 K M)) sum of the Huber elements of the valid (n, t)
 * and with mask_grid_regression reg_loss is the foreground-masked mean over the valid (n, t)
 * only (the foreground count is taken over them).  wd_loss is unchanged.  This is the mean over
 * what exists; with every length full it is the uniform loss, and the step is the uniform one,
 * launch for launch and bit for bit.  No operation couples batch rows, so (wd = 0) losses and
 * gradients are the sums over the groups of rows with equal (Lo, L) of the uniform model's at
 * (obs_len = Lo, pred_len = L) on the group, weighted |g| L / M (masked regression: by the
 * group's foreground count over the total); wd > 0 adds wd * W once.
 * Launches: encoder step t issues every launch of the step (input builders, dropout, gate
 * group and their backward counterparts) on the prefix of 1 + max{n : L[n] > 0, Lo[n] >=
 * obs_len - t} rows, decoder step t (the graph attention, tail and hidden2grid included) on the
 * prefix of 1 + max{n : L[n] > t} rows; a step with no row is not issued.  Any row order is
 * correct; rows sorted by L descending (ties by Lo descending) launch no finished and no padding
 * row, and an unstarted row only in front of a row with a longer history.  The weight-gradient
 * GEMMs run at full extent over rows whose gate gradients are cleared.
 * Dropout (keep_prob < 1): the draw of an element is the uniform step's -- the same seed, the
 * stream number computed from the uniform obs_len / pred_len, the element's index within the
 * full [N, ..] step tensor -- so a row's mask does not depend on the other rows' lengths.
 * With the in-library all-reduce (and mv_train_forward_backward + the caller's) the mean is
 * the LOCAL one, as for uniform steps: ranks with different M are averaged, not M-weighted.
 * A step whose lengths are not all full fails, with a message naming the call and the reason,
 * in bf16 compute mode, for use_single_decoder models, models without the scene encoder,
 * convlstm_kernel != 3 and under label mixup; mv_attack_begin / mv_attack_step and a training
 * step inside an attack pass fail while training lengths are set at all. */
int  mv_set_train_lengths(mv_handle h, const int32_t* obs_lengths /* [N] or NULL */,
                          const int32_t* pred_lengths /* [N] or NULL */);
/* the row counts of the last training step, summed over every ConvLSTM problem of every grouped
 * gate launch: forward_rows as mv_last_forward_gate_rows counts a forward, dgrad_rows over the
 * backward's dgrad groups.  With no training lengths set: the uniform counts. */
int  mv_last_train_gate_rows(mv_handle h, int64_t* forward_rows, int64_t* dgrad_rows);
/* -- in-library gradient all-reduce (RCCL over xGMI) ----
 * One process per GPU.  Rank 0 draws an id (mv_comm_unique_id) and hands its 128 bytes to
 * the other ranks out of band (any bootstrap: a file, MPI, torch.distributed); every rank
 * then calls mv_allreduce_init(h, rank, world, id) after hipSetDevice / mv_create on ITS
 * device.  From then on mv_train_forward_backward leaves the SUM over the ranks in the
 * gradient buffer: the buffer is reduced in buckets (one per ConvLSTM kernel + biases, then
 * the small tensors as one group) on a side stream, each bucket issued as soon as its
 * gradients are final, overlapped with the rest of the backward pass; mv_train_step
 * applies 1/world before the clip and the optimizer.  RCCL is dlopen'ed at the first call;
 * a single-device user never needs it. */
#define MV_COMM_ID_BYTES 128
int  mv_comm_unique_id(uint8_t* id_out /* [MV_COMM_ID_BYTES] */);
int  mv_allreduce_init(mv_handle h, int32_t rank, int32_t world,
                       const uint8_t* unique_id /* [MV_COMM_ID_BYTES] */);
/* rank / world of the communicator, collectives and bytes of the last step */
int  mv_allreduce_info(mv_handle h, int32_t* rank, int32_t* world, int32_t* buckets,
                       double* bytes);
/* -- SimAug training extras (SimAug/code/pred_models.py:60-172
 * white_box_attack, :346-543 multiview_augmentation): targeted FGSM / PGD on the scene
 * features and mixup, on the SAME forward / backward kernels.  The attack loss is the
 * class cross entropy against target labels: run the engine with those labels as
 * grid_pred_labels, grid_reg_loss_weight = 0 and wd = 0 (sign() ignores the loss scale).
 *   mv_attack_begin        snapshot the resident scene features as "clean" and make the
 *                          backward pass go down to d loss / d scene_feat
 *   mv_set/get_scene_feat  replace / read the resident features [U, SH, SW, SC] (the
 *                          attack perturbs per (n, t): upload U = N*T_o frames)
 *   mv_get_scene_grad      d loss / d scene_feat of the last mv_train_forward_backward
 *   mv_attack_step         x <- clip(x - step * sign(g), clip(clean - eps, -1, 1),
 *                          clip(clean + eps, -1, 1))   (FGSM: step = eps, once)
 *   mv_scene_mix           x <- other * weight + x * (1 - weight); other NULL = clean
 *   mv_get_sample_losses   per-sample mean cross entropy [N] of the last step (the
 *                          multi-view selection ranks views by it)
 *   mv_attack_end          back to plain training */
int  mv_attack_begin(mv_handle h);
int  mv_attack_end(mv_handle h);
int  mv_set_scene_feat(mv_handle h, const float* scene_feat);
int  mv_get_scene_feat(mv_handle h, float* out);
int  mv_get_scene_grad(mv_handle h, float* out);
int  mv_attack_step(mv_handle h, float epsilon, float step);
int  mv_scene_mix(mv_handle h, const float* other, float weight);
int  mv_get_sample_losses(mv_handle h, int32_t scale, float* out);
/* SimAug multi-view experiment 3 (SimAug/code/pred_models.py:486-517, 616-636, 1371-1398): the
 * training step on MIXED-UP labels.  obs_labels2[s] [N, T_o] / pred_labels2[s] [N, T_p] = the
 * grid labels of the selected extra camera view (NULL for unused scales); `weight` = the beta
 * weight of the original labels: the class-encoder input and the first decoder input use
 * w * one_hot(label) + one_hot(label2) * (1 - w), the class loss is
 * softmax_cross_entropy_with_logits_v2 against the same mix of the future labels;
 * sample_weight [N] (or NULL) multiplies each sample's class-loss rows (double_weighting: the
 * focal weights).  In force for every following mv_train_* call until cleared. */
int  mv_set_label_mixup(mv_handle h, const int32_t* const* obs_labels2,
                        const int32_t* const* pred_labels2, float weight,
                        const float* sample_weight);
int  mv_clear_label_mixup(mv_handle h);
/* tf.gradients(loss, var) of the last forward_backward, by variable name */
int  mv_get_grad(mv_handle h, const char* tf_name, float* out, int64_t capacity_elems);
int  mv_get_global_step(mv_handle h, int64_t* step);
int  mv_set_global_step(mv_handle h, int64_t step);
/* keep_prob < 1: seed of the NEXT step's dropout masks.  TensorFlow's dropout is
 * unseeded; the engine's masks come from a counter-based hash of (seed, draw number,
 * element) -- oracle/multiverse_oracle.py dropout_keep_mask restates it -- with draws
 * numbered in the reference's cell-call order. */
int  mv_set_dropout_seed(mv_handle h, uint32_t seed);
/* Adam's beta1_power / beta2_power (float32 non-slot variables of the checkpoint) */
int  mv_get_opt_scalars(mv_handle h, float* beta1_power, float* beta2_power);
int  mv_set_opt_scalars(mv_handle h, float beta1_power, float beta2_power);
/* optimizer slots for checkpoint save / restore, TF slot names by optimizer:
 *   adadelta  0 "Adadelta" (accum)   1 "Adadelta_1" (accum_update)
 *   momentum  0 "Momentum"
 *   adam      0 "Adam" (m)           1 "Adam_1" (v)
 *   rmsprop   0 "RMSProp" (ms, initialised to ones)   1 "RMSProp_1" (momentum) */
int  mv_get_opt_slot(mv_handle h, const char* tf_name, int32_t slot, float* out,
                     int64_t capacity_elems);
int  mv_set_opt_slot(mv_handle h, const char* tf_name, int32_t slot,
                     const float* data, int64_t elems);

/* Arithmetic of the gate convolutions (forward, and dgrad / wgrad of a training engine):
 *   0  fp32 MFMA (v_mfma_f32_32x32x2_f32), default;
 *   1  "f16x3": every fp32 operand as two pre-scaled fp16 planes, each product as
 *      three fp16 MFMAs accumulating in fp32 -- fp32-roundoff-class error (DESIGN.md
 *      section 3c).  Where the grid fits its tiling the forward step and dgrad run in
 *      Winograd form over image rows (csrc/convlstm_wino.h: fewer MFMA products for the
 *      same pre-activations, kernel transform in fp64 at pack time); otherwise the direct
 *      3x3 form.  Same outputs contract;
 *   2  bf16 operands (one MFMA per product), fp32 accumulate: REDUCED precision
 *      (BASELINE configs[4]). */
int  mv_set_compute_mode(mv_handle h, int32_t mode);

/* Replay the forward as a captured hipGraph (one graph per (mode, T_pred, U)):
 * the reference's whole forward is ONE sess.run (pred_models.py:1779), here it
 * is one hipGraphLaunch instead of ~150 kernel launches.  Off by default. */
int  mv_set_graph_mode(mv_handle h, int32_t enabled);

/* -- measurement --------------------------------------------------------- */
/* When enabled every kernel launch is bracketed by hipEvents on the handle's
 * stream; totals are read back per kernel name. */
int  mv_set_profiling(mv_handle h, int32_t enabled);
int  mv_reset_kernel_stats(mv_handle h);
int  mv_num_kernel_stats(mv_handle h);
int  mv_kernel_stat(mv_handle h, int32_t i, char* name_out, int32_t name_cap,
                    int64_t* launches, double* total_ms, double* flops,
                    double* bytes);
/* `flops` above are the algorithmic FLOPs the launches EXECUTED (the zero-state first
 * encoder step skips the h half of the gate convolution, SURVEY.md 8d: "do not count
 * them as achieved FLOPs"); this returns the same steps counted densely, as the
 * reference computes them: 2 M 9 (Cx + C) 4C per ConvLSTM step. */
int  mv_kernel_stat_dense_flops(mv_handle h, int32_t i, double* flops_dense);
/* FLOPs the launches ISSUED to the matrix pipe: the executed algorithmic count x 3 for the
 * direct f16x3 gate kernel (three fp16 MFMAs per fp32 product), x 2 for its Winograd F(2,3)
 * form, x 1 on the fp32 / bf16 pipes; 0 for kernels that carry no such figure. */
int  mv_kernel_stat_mfma_flops(mv_handle h, int32_t i, double* flops_mfma);
/* elapsed ms between two events recorded around fn on the engine's stream */
int  mv_time_greedy_resident(mv_handle h, int32_t iters, float* ms_out);
int  mv_time_beam_resident(mv_handle h, int32_t iters, float* ms_out);

/* -- single-kernel entry points (parity tests go through these) ----------- */
/* One tf.contrib.rnn.ConvLSTMCell step on host buffers:
 * x [M,H,W,Cx], c,h [M,H,W,C], kernel [3,3,Cx+C,4C] HWIO, biases [4C]. */
int  mv_op_convlstm_step(int device, const float* x, const float* c,
                         const float* h, const float* kernel,
                         const float* biases, int32_t M, int32_t H, int32_t W,
                         int32_t Cx, int32_t C, float* c_out, float* h_out);
/* The same step on the fp16 matrix pipe at fp32 accuracy (f16x3 operand planes):
 * variant 1 = direct 3x3 form, 2 = Winograd F(2,3) over image rows (W must divide 32),
 * 3 = Winograd F(3,3) over image rows (any W -- widths that do not divide 32 take the halo
 * tiling, operands below 2 GiB --, H >= 3; csrc/convlstm_wino3.h), 4 = REDUCED precision: one
 * bf16 plane per operand on the same row-triple tile (compute mode 2's gate kernel; h16_out is
 * then that one plane decoded), 5 = the same precision on the 32-cell body (what compute mode 2
 * takes where the tile cannot run: H < 3, MV_BF16T=0; 16-channel x groups in pairs), 6 = that
 * body with three x passes: x as two fp16 planes under its own exponent against the x rows of
 * the kernel as an fp16 pair, h one bf16 plane (models with unbounded activations; dense x only).
 * h16_out (optional) [M,H,W,C]: the h' OPERAND PLANES the kernel emitted for the next
 * step, decoded back to fp32 ((hi + lo) / 256), so that a test sees the plane layout. */
int  mv_op_convlstm_step16(int device, int32_t variant, const float* x, const float* c,
                           const float* h, const float* kernel, const float* biases,
                           int32_t M, int32_t H, int32_t W, int32_t Cx, int32_t C,
                           float* c_out, float* h_out, float* h16_out);
/* h + GNN(h): gnn_edge/gnn_mask_edge/gnn_node (pred_models.py:808-909);
 * h [M,H,W,C], scene_mean [M,H,W,D]. */
int  mv_op_gnn(int device, const float* h, const float* scene_mean, int32_t M,
               int32_t H, int32_t W, int32_t C, int32_t D, float* out);
/* The same with the kernel version asked for: 0 = the library's choice (mv_op_gnn), 1 = one wave
 * per cell, 2 = LDS-tiled, 3 = register-blocked.  A version whose kernel does not take the shape
 * runs the next one down that does (csrc/step_plan.h gnn_form), as in an engine. */
int  mv_op_gnn_variant(int device, const float* h, const float* scene_mean, int32_t M,
                       int32_t H, int32_t W, int32_t C, int32_t D, int32_t version, float* out);
/* hidden2grid (pred_models.py:925-959): h [M,H,W,C], w [3,3,C,P] -> [M,H,W,P] */
int  mv_op_hidden2grid(int device, const float* h, const float* w, int32_t M,
                       int32_t H, int32_t W, int32_t C, int32_t P, float* out);
/* One beam expansion (pred_models.py:557-591 + add_div_penalty :1197-1223):
 * logits [N,B,K], prev_logprob [N,B] -> new_logprob, ids, parents [N,B]. */
int  mv_op_beam_step(int device, const float* logits, const float* prev_logprob,
                     int32_t N, int32_t B, int32_t K, int32_t time,
                     int32_t diverse, float gamma, int32_t fix_num_timestep,
                     float* new_logprob, int32_t* ids, int32_t* parents);

/* One step of the sampling without replacement (mv_set_sampling_mode above): logits [N,B,K],
 * prev_phi, prev_logprob, prev_gumbel [N,B] -> new_phi, new_logprob, new_gumbel, ids, parents
 * [N,B].  t = 0-based decode step; with t == 0 only row n*B of the logits and of the prev_* (the
 * root's values) are read.  K <= 1024, B <= K, temperature > 0. */
int  mv_op_sbs_step(int device, const float* logits, const float* prev_phi,
                    const float* prev_logprob, const float* prev_gumbel, int32_t N, int32_t B,
                    int32_t K, int32_t t, float temperature, uint32_t seed, float* new_phi,
                    float* new_logprob, float* new_gumbel, int32_t* ids, int32_t* parents);

/* One step of the independent sampler with the limits of mv_set_sampling_truncation: logits
 * [R, K], R = samples x S rows (row r is future r % S of sample r / S) -> ids [R], lp [R] (the
 * model's log-probability of the drawn cell), qlp [R] (the proposal's), keep [R, K] (1 = the cell
 * is in the kept set).  t = 0-based decode step; floor >= 1 as in the definition; K <= 1024. */
int  mv_op_sample_step(int device, const float* logits /* [R, K] */, int32_t R, int32_t S,
                       int32_t K, int32_t t, float temperature, uint32_t seed, int32_t top_k,
                       float top_p, int32_t floor, int32_t* ids, float* lp, float* qlp,
                       uint8_t* keep /* [R, K] */);

/* The masked forms of the three step ops (mv_set_cell_mask above): allowed [samples, K] bytes,
 * one plane per SAMPLE (N for the beam and the sampling without replacement, R / S for the
 * sampler), non-zero = the cell may be chosen; all else as the unmasked op.  K <= 1024. */
int  mv_op_beam_step_masked(int device, const float* logits, const float* prev_logprob,
                            const uint8_t* allowed /* [N, K] */, int32_t N, int32_t B, int32_t K,
                            int32_t time, int32_t diverse, float gamma, int32_t fix_num_timestep,
                            float* new_logprob, int32_t* ids, int32_t* parents);
int  mv_op_sbs_step_masked(int device, const float* logits, const float* prev_phi,
                           const float* prev_logprob, const float* prev_gumbel,
                           const uint8_t* allowed /* [N, K] */, int32_t N, int32_t B, int32_t K,
                           int32_t t, float temperature, uint32_t seed, float* new_phi,
                           float* new_logprob, float* new_gumbel, int32_t* ids, int32_t* parents);
int  mv_op_sample_step_masked(int device, const float* logits /* [R, K] */,
                              const uint8_t* allowed /* [R / S, K] */, int32_t R, int32_t S,
                              int32_t K, int32_t t, float temperature, uint32_t seed,
                              int32_t top_k, float top_p, int32_t floor, int32_t* ids, float* lp,
                              float* qlp, uint8_t* keep /* [R, K] */);

/* The biased forms of the three step ops (mv_set_cell_bias above): the masked prototype with
 * bias [samples, K] float32, one plane per SAMPLE as `allowed`, directly behind it; `allowed` may
 * be NULL (every cell allowed).  Every bias value is finite.  K <= 1024. */
int  mv_op_beam_step_biased(int device, const float* logits, const float* prev_logprob,
                            const uint8_t* allowed /* [N, K] or NULL */,
                            const float* bias /* [N, K] */, int32_t N, int32_t B, int32_t K,
                            int32_t time, int32_t diverse, float gamma, int32_t fix_num_timestep,
                            float* new_logprob, int32_t* ids, int32_t* parents);
int  mv_op_sbs_step_biased(int device, const float* logits, const float* prev_phi,
                           const float* prev_logprob, const float* prev_gumbel,
                           const uint8_t* allowed /* [N, K] or NULL */,
                           const float* bias /* [N, K] */, int32_t N, int32_t B, int32_t K,
                           int32_t t, float temperature, uint32_t seed, float* new_phi,
                           float* new_logprob, float* new_gumbel, int32_t* ids, int32_t* parents);
int  mv_op_sample_step_biased(int device, const float* logits /* [R, K] */,
                              const uint8_t* allowed /* [R / S, K] or NULL */,
                              const float* bias /* [R / S, K] */, int32_t R, int32_t S,
                              int32_t K, int32_t t, float temperature, uint32_t seed,
                              int32_t top_k, float top_p, int32_t floor, int32_t* ids, float* lp,
                              float* qlp, uint8_t* keep /* [R, K] */);

/* The motion forms of the three step ops (mv_set_motion_cost above): the biased prototype with
 * `motion` directly behind `bias`; `allowed` and `bias` may both be NULL.  The tables are per
 * SAMPLE as `bias` is ([samples, D, D] and [samples]); prev1 / prev0 hold p1 / p0 of every ROW
 * ([N * B] or [R]), prev0[r] = -1: absent.  W divides K; prev1 in [0, K), prev0 in [-1, K). */
typedef struct mv_step_motion {
  int32_t W, radius;
  const float* vel;
  const float* vel_far;
  const float* acc;       /* NULL: no turn term */
  const float* acc_far;   /* NULL exactly when acc is */
  const int32_t* prev1;
  const int32_t* prev0;
} mv_step_motion;
int  mv_op_beam_step_motion(int device, const float* logits, const float* prev_logprob,
                            const uint8_t* allowed /* [N, K] or NULL */,
                            const float* bias /* [N, K] or NULL */, const mv_step_motion* motion,
                            int32_t N, int32_t B, int32_t K, int32_t time, int32_t diverse,
                            float gamma, int32_t fix_num_timestep, float* new_logprob,
                            int32_t* ids, int32_t* parents);
int  mv_op_sbs_step_motion(int device, const float* logits, const float* prev_phi,
                           const float* prev_logprob, const float* prev_gumbel,
                           const uint8_t* allowed /* [N, K] or NULL */,
                           const float* bias /* [N, K] or NULL */, const mv_step_motion* motion,
                           int32_t N, int32_t B, int32_t K, int32_t t, float temperature,
                           uint32_t seed, float* new_phi, float* new_logprob, float* new_gumbel,
                           int32_t* ids, int32_t* parents);
int  mv_op_sample_step_motion(int device, const float* logits /* [R, K] */,
                              const uint8_t* allowed /* [R / S, K] or NULL */,
                              const float* bias /* [R / S, K] or NULL */,
                              const mv_step_motion* motion, int32_t R, int32_t S, int32_t K,
                              int32_t t, float temperature, uint32_t seed, int32_t top_k,
                              float top_p, int32_t floor, int32_t* ids, float* lp, float* qlp,
                              uint8_t* keep /* [R, K] */);

/* The path forms of the three step ops (mv_set_revisit_cost above): the motion prototype with
 * `revisit` directly behind `motion`; `allowed`, `bias` and `motion` may all be NULL.  The op has
 * no parent indirection and takes byte planes: visited[r, k] != 0 means cell k is in row r's set
 * going INTO the step; the kernel ORs prev1[r] in, charges cost[sample] on the set without
 * prev1[r], and visited_out (if given) receives the set it stored.  A row the step does not run
 * (slots > 0 of the first beam / without-replacement step) stores nothing: its visited_out is its
 * visited. */
typedef struct mv_step_revisit {
  const float* cost;        /* [samples] */
  const int32_t* prev1;     /* [rows], in [0, K) */
  const uint8_t* visited;   /* [rows, K] bytes, non-zero = in the row's set; NULL = empty */
  uint8_t* visited_out;     /* [rows, K] or NULL: the set the kernel stored, visited | {prev1} */
} mv_step_revisit;
int  mv_op_beam_step_path(int device, const float* logits, const float* prev_logprob,
                          const uint8_t* allowed /* [N, K] or NULL */,
                          const float* bias /* [N, K] or NULL */,
                          const mv_step_motion* motion /* or NULL */,
                          const mv_step_revisit* revisit, int32_t N, int32_t B, int32_t K,
                          int32_t time, int32_t diverse, float gamma, int32_t fix_num_timestep,
                          float* new_logprob, int32_t* ids, int32_t* parents);
int  mv_op_sbs_step_path(int device, const float* logits, const float* prev_phi,
                         const float* prev_logprob, const float* prev_gumbel,
                         const uint8_t* allowed /* [N, K] or NULL */,
                         const float* bias /* [N, K] or NULL */,
                         const mv_step_motion* motion /* or NULL */,
                         const mv_step_revisit* revisit, int32_t N, int32_t B, int32_t K,
                         int32_t t, float temperature, uint32_t seed, float* new_phi,
                         float* new_logprob, float* new_gumbel, int32_t* ids, int32_t* parents);
int  mv_op_sample_step_path(int device, const float* logits /* [R, K] */,
                            const uint8_t* allowed /* [R / S, K] or NULL */,
                            const float* bias /* [R / S, K] or NULL */,
                            const mv_step_motion* motion /* or NULL */,
                            const mv_step_revisit* revisit, int32_t R, int32_t S, int32_t K,
                            int32_t t, float temperature, uint32_t seed, int32_t top_k,
                            float top_p, int32_t floor, int32_t* ids, float* lp, float* qlp,
                            uint8_t* keep /* [R, K] */);

/* Light cone of the class encoder (MV_ENC_CONE): the wave tiles of the F(3,3) gate
 * kernel each encoder step computes, as every upload builds them from the labels.  Host only: no
 * device is touched.  labels [N, T] cell indices of an H x W grid; r0: reach of a step's own input
 * (1 with the scene encoder, 2 without).  A tile is 32 consecutive triple-cells
 * q = (row * ceil(H / 3) + y / 3) * W + x of the N + 1 rows (row N: the input-free background row),
 * ntile = ceil((N + 1) * ceil(H / 3) * W / 32).  lists [T, 4 + 2 * ntile]: count | 3 zeros | the
 * active tile indices, ascending, zero-filled | per tile 1 = computed at this step; cells [T]: the
 * cells the step computes.  Returns ntile (lists / cells may be NULL to ask for it), -1 on bad
 * arguments. */
int  mv_enc_cone_build(const int32_t* labels, int32_t N, int32_t T, int32_t H, int32_t W,
                       int32_t r0, int32_t* lists, int64_t* cells);

/* One level of the scene stack (conv k x k, stride 2, SAME, + b, activation) in either of its
 * forms: in [U, Hi, Wi, Ci], w [k, k, Ci, Co], b [Co] -> out [U, ceil(Hi/2), ceil(Wi/2), Co].
 * form 0: the kernel the engine launches for this shape; 1: one thread per output element, the
 * form every shape can take.  The two give the same bits.  mv_scene_conv_form (host only): the
 * engine's choice for a shape, 0 = one thread per output, 1 = the 1x1 MFMA projection, 2 = the
 * tiled k = 3 kernel. */
int  mv_scene_conv_form(int32_t k, int32_t Ci, int32_t Co);
int  mv_op_scene_conv(int device, int32_t form, const float* in, const float* w, const float* b,
                      int32_t U, int32_t Hi, int32_t Wi, int32_t Ci, int32_t Co, int32_t k,
                      int32_t act, float* out);

/* The decoder tail of one step (hidden2grid, argmax, the next step's input embedding and its
 * operand planes) for 1 to 4 chains in one call, in either of its forms.  The chains share C
 * (128, 256 or 512), E (a multiple of 16) and the activation (0 tanh, 1 relu, 2 lrelu); each has
 * its own rows, H, W and kind.
 *   form   0: the grouped tail -- the weights packed, ONE h2g_q launch and ONE decode_tail launch
 *             for all chains, as a decode step issues them; a grid of more than 1024 cells or an
 *             E above 512 is refused and nothing is launched.
 *          1: the separate tail, per chain hidden2grid_kernel, argmax_rows_kernel,
 *             grid_emb_onehot_kernel (class) / grid_emb_dense_kernel (regression);
 *          2: as 1 with grid_emb_onehot8_kernel for the class embedding;
 *          3: as 1 with grid_emb_dense_kernel on the literal one-hot map for the class embedding.
 *   next   0: no next step (output rows only); 1: ids only (class chains); 2: ids and embedding.
 *   planes 0: none; 1: two fp16 planes (f16x3); 2: one bf16 plane -- of x, with next == 2.
 * Every device buffer behind ids, x and planes is filled with the byte 0xA5 before the launches
 * and copied back whole, so a caller sees what was not written.  `planes` receives the plane
 * buffer as an engine allocates it: planes_elems = 2 * (rows*K*E + 32768 + 16) halves, plane 0
 * at half 16, plane 1 (f16x3) at half 16 + planes_elems / 2; the layout inside a plane is
 * csrc/plane_layout.h. */
typedef struct mv_tail_chain {
  int32_t rows, H, W;
  int32_t kind;              /* 0: class chain (P = 1, one-hot); 1: regression chain (P = 2, dense) */
  const float* h;            /* [rows, H, W, C] */
  const float* w_out;        /* hidden2grid [3, 3, C, P] */
  const float* emb_w;        /* [3, 3, P, E]; may be NULL unless next == 2 */
  const float* emb_b;        /* [E]; likewise */
  float* out;                /* [rows, K, P] */
  int32_t* ids;              /* [rows]; may be NULL (always for a regression chain) */
  float* x;                  /* [rows * K, E]; may be NULL */
  uint16_t* planes;          /* [planes_elems]; may be NULL */
  int64_t planes_elems;
} mv_tail_chain;
int  mv_op_decode_tail(int device, int32_t form, int32_t next, int32_t planes, int32_t C,
                       int32_t E, int32_t act, const mv_tail_chain* chains, int32_t n);

/* Backward of one ConvLSTMCell step (tf.gradients through the cell): inputs as
 * mv_op_convlstm_step (c == h == NULL: zero state) plus d h', d c' [M,H,W,C];
 * outputs d x [M,H,W,Cx], d h, d c [M,H,W,C], d kernel [3,3,Cx+C,4C], d biases [4C]. */
int  mv_op_convlstm_bwd(int device, const float* x, const float* c, const float* h,
                        const float* kernel, const float* biases,
                        const float* dh_new, const float* dc_new, int32_t M,
                        int32_t H, int32_t W, int32_t Cx, int32_t C, float* dx,
                        float* dh, float* dc, float* dkernel, float* dbiases);
/* The matrix-pipe backward of ONE gate convolution, kernel by kernel (the backward's counterpart
 * of mv_op_convlstm_step16): x [M,H,W,Cx], h [M,H,W,C] (the step's INPUT state), G [M,H,W,4C] the
 * pre-activation gate gradient -- an input, so that nothing upstream of the two GEMMs rounds --,
 * kernel [3,3,Cx+C,4C] -> dx [M,H,W,Cx], dh [M,H,W,C], dkernel [3,3,Cx+C,4C].  The engine's own
 * packs, plane splits, transposes, exponent kernels and launchers; the variant picks the form,
 * everything else (split-K, DPP column shift, narrow or wide tile, split counts) is the
 * planner's (csrc/gate_plan.h).  0 skips that half (its outputs and inputs may then be NULL).
 *   variant_dgrad  1 f16x3 direct; 2 f16x3 Winograd F(2,3) (32 % W == 0, H >= 2); 3 ONE bf16
 *                  plane per operand, whole-K
 *   variant_wgrad  1 f16x3 direct; 2 f16x3 row-triple (H % 3 == 0); 3 ONE fp16 plane per operand,
 *                  direct; 4 one plane, row-triple.  All four: W % 16 == 0, C % 128 == 0.
 * A shape the planner would not give the form is refused before any launch, the message naming
 * the planner's condition.  exps [3]: the power-of-two scale exponents the device computed for G,
 * h and x (wgrad; with variant_wgrad 0 and an f16x3 dgrad exps[0] is the dgrad's G exponent, the
 * rest 0).  forms [8]: wide, wide_x, nsplit, nsplit_x (wgrad); split-K slices of the d h and of
 * the d x blocks, DPP column shift (dgrad); transpose3 (wgrad).  Every output and partial buffer
 * holds the byte 0xA5 before the launches. */
int  mv_op_convlstm_bwd16(int device, int32_t variant_dgrad, int32_t variant_wgrad,
                          const float* x, const float* h, const float* G, const float* kernel,
                          int32_t M, int32_t H, int32_t W, int32_t Cx, int32_t C, float* dx,
                          float* dh, float* dkernel, int32_t* exps, int32_t* forms);
/* The pointwise backward of one step in each of its kernels: form 0 scalar, 1 four channels per
 * thread, 2 the same emitting G also as ONE bf16 plane.  gates [cells,4,C] the saved activations
 * (si | tj | sf | so), c_prev (NULL: zero), c_new, dh, dc [cells,C] -> G [cells,4C], dc_out
 * [cells,C], gmax_bits: the float bits of max |G| as the kernel tracked them; plane_out (form 2;
 * else it may be NULL) [cells,4C]: the plane's values. */
int  mv_op_lstm_gate_bwd(int device, int32_t form, const float* gates, const float* c_prev,
                         const float* c_new, const float* dh, const float* dc, int32_t cells,
                         int32_t C, float* G_out, float* dc_out, int32_t* gmax_bits,
                         float* plane_out);
/* Backward of h + GNN(h) given g = d out: d h [M,H,W,C], d scene_mean [M,H,W,D]. */
int  mv_op_gnn_bwd(int device, const float* h, const float* scene_mean,
                   const float* g, int32_t M, int32_t H, int32_t W, int32_t C,
                   int32_t D, float* dh, float* dscene_mean);

/* ---- The helper kernels of a training step, one entry point each (kernel-level parity tests,
 * tests/test_gpu_train_helpers.py).  Each runs the engine's own host-side choice of kernel and its
 * launch on the operands given; a forced form the shape cannot take is refused by name before
 * any launch.  Output buffers hold the byte 0xA5 before the launches.
 *
 * dgrad of a small 3x3 SAME conv (hidden2grid, grid_emb): dout [M][dout_rs] with the first
 * H*W*Co floats of a row in use, w [9][Ci][Co], din [M][din_rs] IN and OUT (the whole buffer
 * travels both ways, so what lies between the rows comes back as it went in).  form 0 the plan's,
 * 1 scalar, 2 dgrad4<1>, 3 dgrad4<2>; form_ran: 1, 2 or 3. */
int  mv_op_small_conv_dgrad(int device, int32_t form, const float* dout, int64_t dout_rs,
                            const float* w, float* din, int64_t din_rs, int32_t M, int32_t H,
                            int32_t W, int32_t Ci, int32_t Co, int32_t accumulate,
                            int32_t* form_ran);
/* wgrad of the same conv over R images: in [R,H,W,Ci], dout [R,H,W,Co] -> dw [9][Ci][Co] after
 * the two-level fold.  form 0 the plan's, 1 small_wgrad<false> (walks the output cells), 2
 * small_wgrad<true> (walks the input cells), 3 the hidden2grid kernel.  Ci*Co > 512 is refused
 * outside the hidden2grid shape.  info [4]: form that ran, blocks, cells per block, cell groups
 * G per workgroup. */
int  mv_op_small_conv_wgrad(int device, int32_t form, const float* in, const float* dout,
                            int32_t R, int32_t H, int32_t W, int32_t Ci, int32_t Co, float* dw,
                            int32_t* info);
/* The deterministic column sum of x [rows, ncols] -> out [ncols].  info [2]: slabs, and whether
 * the narrow kernel summed them. */
int  mv_op_colsum(int device, const float* x, int64_t rows, int64_t ncols, float* out,
                  int32_t* info);
/* out[0] = scale * sum of x [n]; chunked: whether the per-chunk stage ran. */
int  mv_op_long_sum(int device, const float* x, int64_t n, float scale, float* out,
                    int32_t* chunked);
/* Backward of one level of the stride-2 SAME scene stack given its input, its forward output y
 * and dy: dpre = dy * act'(y) [U,Ho,Wo,Co], din [U,Hi,Wi,Ci] (accumulate: onto din_init; else
 * din_init may be NULL), dw [k,k,Ci,Co] (slab partials folded), db [Co].  info [4]: pad_t,
 * pad_l, wgrad slabs, output rows per slab. */
int  mv_op_scene_conv_bwd(int device, const float* in, const float* y, const float* dy,
                          const float* w, int32_t U, int32_t Hi, int32_t Wi, int32_t Ci,
                          int32_t Co, int32_t k, int32_t act, const float* din_init,
                          int32_t accumulate, float* dpre, float* din, float* dw, float* db,
                          int32_t* info);
/* dW [9][E] of the class encoder's grid_emb from its one-hot input: dpre [T,N,H,W,E] time-major,
 * labels [N][T] (each a cell of the grid, checked on the host); dw IN and OUT (accumulate adds
 * onto it). */
int  mv_op_grid_emb_onehot_wgrad(int device, const float* dpre, const int32_t* labels, int32_t N,
                                 int32_t T, int32_t H, int32_t W, int32_t E, int32_t accumulate,
                                 float* dw);
/* One loss of a training step.  kind 0 ce (labels [N][T]), 1 ce_soft (soft [T*N,K]), 2 ce_len
 * (pred_lens [N]; labels, or soft when given), 3 huber, 4 huber_len, 5 huber_masked (fg [T,N,K];
 * with the foreground count in front and the masked mean behind).  pred time-major: logits
 * [T,N,K], or [T,N,K,2] against target [N,T,K,2].  scale multiplies the gradient and the summed
 * loss (kind 5: the loss weight).  sample_w [N] (kinds 0 and 1, or NULL) scales the rows.  Labels
 * outside [0, K) and lengths outside [0, T] are refused before any launch.  loss: [T*N] rows, or
 * [T,N,K,2] elements; grad as pred; loss_sum [1]; info [2]: the foreground count (kind 5),
 * whether the long sum ran its chunk stage. */
int  mv_op_train_loss(int device, int32_t kind, const float* pred, const int32_t* labels,
                      const float* soft, const float* target, const float* fg,
                      const float* sample_w, const int32_t* pred_lens, int32_t T, int32_t N,
                      int32_t K, float scale, float* loss, float* grad, float* loss_sum,
                      int32_t* info);

#ifdef __cplusplus
}
#endif
#endif  /* MULTIVERSE_HIP_H_ */
