// engine state: device buffers, parameters, per-scale state, mv_engine -- part of the ONE translation unit engine.hip (included from there, in order;
// not a stand-alone header).
#pragma once

struct mv_train_holder;

namespace {

thread_local std::string g_create_error;



struct HipError { std::string msg; };

#define HIP_CHECK(expr)                                                       \
  do {                                                                        \
    hipError_t _e = (expr);                                                   \
    if (_e != hipSuccess) {                                                   \
      char _b[512];                                                           \
      snprintf(_b, sizeof(_b), "%s failed: %s (%s:%d)", #expr,                \
               hipGetErrorString(_e), __FILE__, __LINE__);                    \
      throw HipError{_b};                                                     \
    }                                                                         \
  } while (0)

#define MV_REQUIRE(cond, ...)                                                 \
  do {                                                                        \
    if (!(cond)) {                                                            \
      char _b[512];                                                           \
      snprintf(_b, sizeof(_b), __VA_ARGS__);                                  \
      throw HipError{_b};                                                     \
    }                                                                         \
  } while (0)

template <typename T>
struct DevBuf {
  T* p = nullptr;
  T* base = nullptr;     // allocation start (p - pad)
  size_t n = 0;
  // `pad` elements of zeroed slack before and after (operands of the wgrad
  // kernel, whose masked lanes may read one cell outside the tensor)
  void alloc(size_t count, size_t pad = 0) {
    if (count <= n && p) return;
    release();
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&base), (count + 2 * pad) * sizeof(T)));
    if (pad) HIP_CHECK(hipMemset(base, 0, (count + 2 * pad) * sizeof(T)));
    p = base + pad;
    n = count;
  }
  void release() {
    if (base) (void)hipFree(base);
    p = nullptr; base = nullptr; n = 0;
  }
  ~DevBuf() { release(); }
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
};

struct Param {
  std::string name;
  std::vector<int64_t> shape;
  std::vector<float> host;
  DevBuf<float> dev;
  bool set = false;
  bool no_grad = false;     // exists in the graph / checkpoints but is neither run nor trained
  size_t elems() const {
    size_t e = 1;
    for (auto d : shape) e *= (size_t)d;
    return e;
  }
};

struct ConvCell {           // one ConvLSTMCell: packed kernel + biases
  Param* kernel = nullptr;
  Param* biases = nullptr;
  DevBuf<float> wpack;
  DevBuf<_Float16> wp16;    // f16x3 compute mode: two scaled fp16 planes, fragment order
  DevBuf<float> wx32;       // f16x3, Cx <= 3: the fp32 x chunk scaled by 2^16
  DevBuf<_Float16> wpb;     // bf16 compute mode: one unscaled bf16 plane, fragment order
  DevBuf<float> wx32u;      // bf16, Cx <= 3: the fp32 x chunk, unscaled
  DevBuf<_Float16> wpw;     // f16x3, Winograd F(2,3) form of the kernel (convlstm_wino.h)
  DevBuf<_Float16> wpw3;    // f16x3, Winograd F(3,3) form of the kernel (convlstm_wino3.h)
  DevBuf<_Float16> wpbt;    // bf16 mode on the row-triple tile (convlstm_wino3.h BF16D)
  bool host_stale = false;  // device copy was updated by the optimizer
  // f16x3: may this kernel take a Winograd form?  A Winograd form spreads EVERY tap over all
  // its components, so an outlier weight (|w| thousands of times the kernel's typical weight)
  // leaves roundoff of ITS size in outputs it does not feed at all -- the direct form keeps it
  // in the outputs that carry it.  Measured (tests/test_gpu_at_size.py, +-230 outliers in
  // kernels of median |w| 3e-3): F(2,3) / F(3,3) 7e-5 / 1.8e-4 of the output range against
  // fp64, direct form 2.6e-5 / 3.7e-5 (fp32 matrix pipe 2.0e-5 / 2.9e-5).  Set by
  // ensure_packed16 from the host copy: max |w| <= kWinoOutlierRatio x median |w|.
  bool wino_numerics_ok = true;
  int Cx = 0;
};
constexpr float kWinoOutlierRatio = 4096.f;

struct KernelStat {
  std::string name;
  int64_t launches = 0;
  // flops: algorithmic FLOPs the launches EXECUTED (a zero-state step skips the h
  // half of the gate convolution); flops_dense: the same steps as the reference
  // computes them (dense 2*M*9*(Cx+C)*4C).  bytes: algorithmic HBM bytes.
  double total_ms = 0, flops = 0, bytes = 0, flops_dense = 0;
  // FLOPs the launches ISSUED to the matrix pipe (0 for non-MFMA kernels): the algorithmic
  // count x 3 for the direct f16x3 form (three fp16 MFMAs per product), x 2 for its Winograd
  // F(2,3) form (two thirds of them), x 1 for the fp32 and bf16 pipes
  double flops_mfma = 0;
};

struct PendingEvent {
  int stat;
  hipEvent_t a, b;
};

// What a forward decodes with.  Beam, Sampled, SampledWor and Scored run on a beam handle
// (beam_size > 1) and leave their results in the bm_* buffers; Greedy leaves out_cls / out_reg.
// SampledWor: the beam driver with the stochastic-beam-search step (mv_set_sampling_mode 1).
enum class ForwardKind { None, Greedy, Beam, Sampled, Scored, SampledWor };

// Per-sample prediction lengths L[n] in [0, pred_len] as a launch plan.  A forward whose lengths
// are not all pred_len is RAGGED: step t issues its launches on the prefix of
// act_rows[t] = 1 + max{n : L[n] > t} rows, for steps = max L steps.  Otherwise every step runs
// on the whole batch and the forward is the uniform one, launch for launch.
struct LengthPlan {
  bool ragged = false;               // the forward being issued / issued last is ragged
  int steps = 0;
  std::vector<int> act_rows;         // [pred_len + 1] of that forward
  void reset() { ragged = false; steps = 0; }
  void build(const std::vector<int32_t>& L, int pred_len) {
    act_rows.assign((size_t)pred_len + 1, 0);
    steps = 0;
    for (int n = 0; n < (int)L.size(); ++n) {
      for (int t = 0; t < L[n]; ++t) act_rows[t] = n + 1;   // n ascending: the max
      steps = std::max(steps, (int)L[n]);
    }
    ragged = true;
  }
  int rows_at(int t, int batch) const {
    if (!ragged) return batch;
    return t < (int)act_rows.size() ? act_rows[t] : 0;
  }
};

// Per-sample observation lengths Lo[n] in [1, obs_len] as a launch plan (mv_set_obs_lengths;
// DESIGN.md 8.9).  The observations are right-aligned: row n JOINS the encoders at step
// obs_len - Lo[n], from the zero state.  A forward whose lengths are not all obs_len is
// OBS-RAGGED: encoder step t issues its launches on the prefix of
// rows[t] = 1 + max{n < rows_at(0) : Lo[n] >= obs_len - t} rows, and the first step that has
// rows (`first`) runs the zero-state form.  At a later step the rows that join have their
// state rows (c, h and the operand planes of h) cleared in front of the gate launch, so the
// ordinary form reads the zero state for them (mv_engine::obs_join_rows lists them by step).
struct ObsPlan {
  bool ragged = false;               // the forward being issued / issued last is obs-ragged
  int first = 0;
  std::vector<int> rows;             // [obs_len] of that forward
  void reset() { ragged = false; first = 0; }
  void build(const std::vector<int32_t>& Lo, int obs_len, int live_rows) {
    rows.assign((size_t)obs_len, 0);
    for (int n = 0; n < live_rows; ++n)
      for (int t = obs_len - Lo[n]; t < obs_len; ++t) rows[t] = n + 1;   // n ascending: the max
    first = 0;
    while (first < obs_len && rows[first] == 0) ++first;
    ragged = true;
  }
};

// Per-row TRAINING lengths (mv_set_train_lengths): the two plans above for a
// training step.  Row n is the model at obs_len = Lo[n], pred_len = L[n]; L[n] == 0 is a padding
// row.  A step whose lengths are not all full is RAGGED: encoder step t issues its launches on
// the prefix of enc_rows[t] = 1 + max{n : L[n] > 0, Lo[n] >= obs_len - t} rows, decoder step t on
// dec_rows[t] = 1 + max{n : L[n] > t}; a step without rows is not issued.  live [obs_len +
// pred_len][N] says per step which rows of [0, N) the step runs for their own model -- the
// others (outside the prefix, not yet joined, finished, padding) are cleared by
// zero_dead_rows_kernel.  Otherwise the step is the uniform one, launch for launch.
struct TrainLens {
  bool set = false;                  // mv_set_train_lengths holds a value
  std::vector<int32_t> obs_host, pred_host;   // as given ([N]); empty: that side is uniform
  bool dirty = true;                 // the device copy predates the setting
  int built_pred_len = -1;
  // the step being issued / issued last
  bool ragged = false;
  bool issuing = false;              // ... and its launches are being issued right now
  std::vector<int32_t> Lo, L;        // [N] with the uniform side filled in
  std::vector<int> enc_rows, dec_rows;   // [obs_len], [pred_len]
  int64_t M = 0;                     // sum of L: the valid (n, t) of the losses
  DevBuf<int32_t> dev;               // Lo [N] | L [N] | live [obs_len + pred_len][N]
  int N = 0, To = 0;
  const int32_t* d_obs() const { return dev.p; }
  const int32_t* d_pred() const { return dev.p + N; }
  const int32_t* d_enc_live(int t) const { return dev.p + (size_t)(2 + t) * N; }
  const int32_t* d_dec_live(int t) const { return dev.p + (size_t)(2 + To + t) * N; }
  void build(int n_rows, int obs_len, int pred_len, std::vector<int32_t>& live) {
    N = n_rows; To = obs_len;
    enc_rows.assign((size_t)obs_len, 0);
    dec_rows.assign((size_t)pred_len, 0);
    live.assign((size_t)(obs_len + pred_len) * N, 0);
    M = 0;
    for (int n = 0; n < N; ++n) {      // n ascending: the max
      M += L[n];
      for (int t = 0; t < L[n]; ++t) { dec_rows[t] = n + 1; live[(size_t)(To + t) * N + n] = 1; }
      if (L[n] > 0)
        for (int t = obs_len - Lo[n]; t < obs_len; ++t) {
          enc_rows[t] = n + 1; live[(size_t)t * N + n] = 1;
        }
    }
  }
};

struct ScaleState {
  int H = 0, W = 0, K = 0;
  bool use = false;
  ConvCell enc_cls, enc_reg, dec_cls, dec_reg;
  Param *emb_cls_W = nullptr, *emb_cls_b = nullptr, *emb_reg_W = nullptr,
        *emb_reg_b = nullptr, *out_cls_W = nullptr, *out_reg_W = nullptr;
  DevBuf<float> scene_mean;                 // [N, K, D]
  DevBuf<int32_t> labels;                   // [N, T_o]
  DevBuf<float> obs_reg;                    // [N, T_o, K, 2]
  DevBuf<double> centers;                   // [K, 2] cell centres (compact inputs)
  DevBuf<float> cls_c[2], cls_h[2], cls_hg; // class chain state [R, K, C]
  DevBuf<float> reg_c[2], reg_h[2];         // regression chain state [N, K, C]
  DevBuf<float> xbuf_cls, xbuf_reg;         // ConvLSTM x operand
  DevBuf<float> out_cls;                    // [N, T_p, K, 1]
  DevBuf<float> out_reg;                    // [N, T_p, K, 2]
  DevBuf<int32_t> ids;                      // [N] greedy argmax
  // decoder tail (decode_tail.h): per-cell tap products of hidden2grid and its packs
  DevBuf<float> q_cls, q_reg;               // [R, K, 9], [N, K, 18]
  DevBuf<float> wq_cls, wq_reg;             // pack_h2g_kernel of out_cls_W / out_reg_W
  bool wq_valid = false;
  // sparse x operand of the class chains (sparse_x.h)
  DevBuf<uint32_t> sx_cellyx;               // [K] y << 16 | x
  DevBuf<float> sx_dec_bias, sx_dec_corr;   // [9][4C], [9][25][4C]: functions of the weights
  DevBuf<float> sx_enc_corr;                // [T_o][N][9][4C]: every encoder step
  // no scene encoder (scene_conv_dim 0): the class encoder's x is grid_emb(one_hot) as the
  // decoder's -- by-class tables of the encoder kernel and the shared person_pred/grid_emb
  DevBuf<float> sx_enc_bias, sx_enc_tab;    // [9][4C], [9][25][4C]
  bool sx_valid = false;
  // light cone of the class encoder (engine_io.h build_enc_cone): the tile lists of every encoder
  // step, built from the labels at upload; cone_cells [T_o]: cells each step executes
  DevBuf<int32_t> cone;
  std::vector<int32_t> cone_host;
  std::vector<int64_t> cone_cells;
  bool cone_ready = false;
};

// Caller-given planes per (sample, step) of a beam handle: the allowed cells (uint8_t,
// mv_set_cell_mask) and the cell costs (float32 log-potentials, mv_set_cell_bias,
// DESIGN.md 8.12).  The device copy has ONE address and one of two layouts, so that a captured
// forward follows a later upload: [N, 1, K] for Tm == 1, [N, Tcap, K] for Tm > 1 with
// Tcap = max_pred_len (planes past it are never read and not kept).
template <typename T>
struct CellPlanes {
  DevBuf<T> dev;
  int tm = 0;                      // 0 = not set
  bool set() const { return tm > 0; }
  int layout() const { return tm > 1 ? 2 : tm; }    // step_plan.h constraint_graph_key's code
  int64_t stride(int K, int Tcap) const { return tm > 1 ? (int64_t)Tcap * K : K; }
  int64_t step(int K) const { return tm > 1 ? K : 0; }
  const T* at(int K, int t) const { return dev.p + (size_t)t * step(K); }   // plane t of sample 0
  // one allocation for both layouts: the address a captured forward holds never changes
  void upload(const T* host, size_t N, int Tm, size_t K, size_t Tcap) {
    dev.alloc(N * Tcap * K);
    if (Tm == 1) {
      HIP_CHECK(hipMemcpy(dev.p, host, N * K * sizeof(T), hipMemcpyHostToDevice));
    } else {
      const size_t planes = std::min((size_t)Tm, Tcap);   // a forward reads planes < pred_len
      HIP_CHECK(hipMemcpy2D(dev.p, Tcap * K * sizeof(T), host, (size_t)Tm * K * sizeof(T),
                            planes * K * sizeof(T), N, hipMemcpyHostToDevice));
    }
    tm = Tm;
  }
};

struct StepConstraints {
  CellPlanes<uint8_t> mask;
  std::vector<int32_t> mask_count; // [N, Tm] allowed cells per plane, taken on the host when the
                                   // mask is set and checked at the forward
  CellPlanes<float> bias;
  // motion costs: ONE allocation sized for the largest radius, so that the
  // addresses a captured forward holds never change: vel [N, D, D] at 0, vel_far [N],
  // acc [N, D, D], acc_far [N] at the offsets below (N = batch_size).
  DevBuf<float> motion_dev;
  int motion_radius = 0;           // 0 = no motion cost
  bool motion_acc = false;
  bool motion_set() const { return motion_radius > 0; }
  static constexpr size_t kMotionCells = (2 * MV_MOTION_MAX_RADIUS + 1) * (2 * MV_MOTION_MAX_RADIUS + 1);
  static size_t motion_vel_far_at(size_t N) { return N * kMotionCells; }
  static size_t motion_acc_at(size_t N) { return motion_vel_far_at(N) + N; }
  static size_t motion_acc_far_at(size_t N) { return motion_acc_at(N) + motion_vel_far_at(N); }
  static size_t motion_floats(size_t N) { return motion_acc_far_at(N) + N; }
  // revisit cost: the cost [N], and the visited sets of every row,
  // [2][rows][64] words (kernels_misc.h RevisitRow; rows = batch_size * beam_size; step t reads
  // half (t - 1) & 1 and stores half t & 1).  Both allocated once at their largest size, so that
  // the addresses a captured forward holds never change.
  DevBuf<float> revisit_dev;
  DevBuf<uint32_t> revisit_sets;
  bool revisit_on = false;
  bool revisit_seed = false;       // seed_observed
  bool revisit_set() const { return revisit_on; }
  static size_t revisit_set_words(size_t rows) { return rows * 64; }
};

}  // namespace

struct mv_engine {
  mv_config cfg{};
  int device = 0;
  hipStream_t stream = nullptr;
  // Two launch streams of the greedy inference forward (engine_forward.h enqueue_forward): the
  // class chains (pair 0) stay on `stream`, the regression chains (pair 1) run on `stream_b`
  // between one fork and one join per forward.  Every launch of the forward goes to `issue`, and
  // a gate group takes its scratch from the group slots slot0, slot0 + 1 (pair 0: {0, 1}, pair
  // 1: {2, 3}); outside a forward that has forked, issue == stream and slot0 == 0.  Host issue is
  // single-threaded, so the pair being issued is engine state (IssueOn sets and restores it).
  hipStream_t stream_b = nullptr;
  hipEvent_t fork_ev = nullptr, join_ev = nullptr;
  hipStream_t issue = nullptr;
  int slot0 = 0;
  std::string err;
  std::vector<std::unique_ptr<Param>> params;
  Param* decode_reg_W = nullptr;   // --use_single_decoder: the offset kernel shared by the scales
  std::map<std::string, Param*> by_name;
  std::vector<Param*> scene_W, scene_b;
  // no scene encoder (mv_config.scene_conv_dim == 0): the class encoders' input embedding
  // person_pred/grid_emb/{W,b}, ONE pair shared by the scales (code/pred_models.py:218-229)
  Param *enc_emb_W = nullptr, *enc_emb_b = nullptr;
  bool no_scene() const { return cfg.scene_conv_dim == 0; }
  ScaleState sc[MV_MAX_SCALES];
  // inputs
  DevBuf<int32_t> obs_scene;       // [N, T_o]
  DevBuf<float> scene_feat;        // [U, SH, SW, SC]
  DevBuf<uint8_t> scene_u8;        // compact inputs: the masks as uploaded
  DevBuf<double> xy_dev;           // compact inputs: [N, T, 2] coordinates
  DevBuf<float> scene_conv[MV_MAX_SCALES];  // per level [U, h*w, D]
  std::vector<int> conv_h, conv_w;
  int num_frames = 0;
  int pred_len = 0;
  bool inputs_ready = false;
  // per-row prediction lengths (mv_set_pred_lengths; sticky until cleared): L[n] in [0, pred_len],
  // a host copy (which launches a step gets) and a device copy (the finalisers and the
  // multi-future decode); `len` is the plan of the forward being issued / issued last.
  std::vector<int32_t> lens_host;
  DevBuf<int32_t> lens_dev;          // [N]
  bool lens_set = false;
  LengthPlan len;
  int rows_at(int t) const { return len.rows_at(t, cfg.batch_size); }
  // per-row observation lengths (mv_set_obs_lengths; sticky until cleared): Lo[n] in [1, obs_len],
  // a host copy, a device copy (the scene mean's window) and the rows in the order they join
  // the encoders (obs_join_rows [N], ascending join step; obs_join_at [obs_len + 1] its offsets);
  // `obs` is the plan of the forward being issued / issued last.
  std::vector<int32_t> obs_lens_host;
  DevBuf<int32_t> obs_lens_dev;      // [N]
  DevBuf<int32_t> obs_join_rows;     // [N]
  std::vector<int> obs_join_at;
  bool obs_lens_set = false;
  ObsPlan obs;
  // set and not all obs_len: what training, the attack calls and the pipelined forward refuse
  bool obs_lens_short() const {
    if (!obs_lens_set) return false;
    for (int32_t l : obs_lens_host) if (l != cfg.obs_len) return true;
    return false;
  }
  // rows encoder step t runs on
  int enc_rows_at(int t) const { return obs.ragged ? obs.rows[(size_t)t] : rows_at(0); }
  // rows of every ConvLSTM problem of every grouped gate launch of the last forward
  // (mv_last_forward_gate_rows); a replayed graph carries the count of its capture
  int64_t gate_rows = 0;
  std::map<std::tuple<ForwardKind, int, int, int>, int64_t> graph_gate_rows;
  // beam
  DevBuf<float> bm_logits;         // [T, N, B, K] per-step logits
  DevBuf<int32_t> bm_ids, bm_parents;  // [T, N, B]
  DevBuf<float> bm_lp[2];          // [N, B]
  DevBuf<float> bm_lp_final;       // [N, B] ragged forward: row n's scores after the selection at time L[n]
  DevBuf<float> bm_cand;           // [N, B, K] candidate log-probs of one step
  // sampling without replacement (ForwardKind::SampledWor): bm_lp carries LP; phi (the tempered
  // log-probability that drives the search) and G (the perturbed score) ping-pong beside it, and
  // the perturb kernel leaves the step's lp / q planes for the selection
  DevBuf<float> bm_phi[2], bm_g[2];    // [N, B]; the final G goes to bm_g[0]
  DevBuf<float> bm_g_final;            // [N, B] ragged forward: row n's G after the selection at time L[n]
  DevBuf<float> bm_phi_final;          // [N, B] the same for phi (the proposal's log-probability)
  DevBuf<float> bm_sbs_lp, bm_sbs_q;   // [N, B, K]
  DevBuf<int32_t> bm_src_row;      // [N*B]
  DevBuf<int32_t> bm_ref;          // [N*B] 1 = some surviving beam continues this state row
  DevBuf<int32_t> bm_trace;        // [N, B, T]
  DevBuf<float> bm_out_logits;     // [N, B, T, K]
  // --use_single_decoder with beam search (code/pred_models.py:274, 287-296): the offsets
  // are hidden2grid of the class decoder's states traced back along every beam
  DevBuf<float> bm_reg_steps;      // [T, N*B, K, 2]   per step, in the step's own row order
  DevBuf<float> bm_out_reg;        // [N*B, T, K, 2]   traced back
  DevBuf<int32_t> bm_out_ids;      // [N, B, T]
  // sampled multi-future decode (mv_set_sampling): the beam handle draws beam_size futures per
  // row instead of searching.  {seed, temperature bits, top_k, top_p bits} live on the device,
  // where the step kernels read them: a captured forward follows a later mv_set_sampling or
  // mv_set_sampling_truncation.
  bool sampling = false;
  int sampling_mode = 0;           // mv_set_sampling_mode: 0 independent draws, 1 without replacement
  int32_t samp_top_k = 0;          // mv_set_sampling_truncation: 0 = off
  float samp_top_p = 1.f;          //                             1 = off
  DevBuf<uint32_t> samp_params;    // [4]
  // [N, B] log-probability of each future under the PROPOSAL (tempered, truncated):
  // the independent sampler accumulates it beside bm_lp[0]; without replacement it is the final phi
  DevBuf<float> lq_acc;
  // what constrains the cells a beam / sampled forward chooses (mv_set_cell_mask, mv_set_cell_bias,
  // mv_set_motion_cost, mv_set_revisit_cost; sticky until cleared)
  StepConstraints con;
  // scoring of GIVEN futures (mv_score_futures): a teacher-forced forward of the
  // sampled driver, asked for per forward (ForwardKind::Scored): nothing about it is sticky.
  // The uploaded ids live in score_ids with a valid cell at every step (a finished future keeps
  // decoding); every forward copies them into bm_out_ids, which the cell steps read and the
  // finalisers mark -1 past a future's length, so a replayed graph scores the latest upload.
  bool score_ready = false;        // futures uploaded (mv_upload_score_futures) ...
  int score_pred_len = 0;          // ... for inputs of this pred_len
  bool score_uniform = true;       // every future's length is pred_len
  std::vector<int32_t> score_L;    // [N] per-sample length = max over its futures
  DevBuf<int32_t> score_ids;       // [N, F, T] as uploaded, filled past the length
  DevBuf<int32_t> score_len;       // [N, F] per-future lengths
  DevBuf<float> score_step_lp;     // [N, F, T]
  DevBuf<int32_t> score_rank;      // [N, F, T]
  // the kind of the last forward: which downloads and which multi-future decode
  // (multifuture_decode.h) its results allow
  ForwardKind last = ForwardKind::None;
  bool last_on_beams() const { return last != ForwardKind::None && last != ForwardKind::Greedy; }
  DevBuf<double> mf_traj;          // [N, B, T, 2] pixel trajectories
  DevBuf<float> mf_occ;            // [N, T, K] occupancy map of the beams
  // 0 = fp32 MFMA (v_mfma_f32_32x32x2_f32), 1 = f16x3 split on the fp16 matrix pipe,
  // 2 = bf16 operands / fp32 accumulate (one plane, one MFMA per product)
  int compute_mode = 0;
  DevBuf<_Float16> px16[mv::kMaxGroup], ph16[mv::kMaxGroup];   // fallback plane scratch per slot
  // F(3,3) gate kernel: the pre-transformed operands of a group slot (convlstm_wino3.h
  // wino3_transform_kernel), x and h
  DevBuf<_Float16> pv3x[mv::kMaxGroup], pv3h[mv::kMaxGroup];
  // relu / lrelu models on the fp16 / bf16 pipe: the x operands of the gate convolutions are
  // unbounded, so their planes carry a per-tensor exponent (max |x| as float bits [64] |
  // exponent [1]) instead of the fixed 2^8; the producers do not emit planes for these buffers.
  // In bf16 mode (round 6) the x k-steps of such models run on the LEADING fp16 plane of that
  // split (11 significand bits under the exponent, fp16 weights for the x rows, fp16 MFMA)
  // instead of one bf16 plane (8 bits): a pixel-offset embedding of hundreds rounded to bf16
  // cost the regression decoder's kernel gradient its direction (cosine 0.96)
  DevBuf<int32_t> xexp[mv::kMaxGroup];
  std::set<const float*> xbufs;
  bool dyn_x() const { return compute_mode != 0 && cfg.activation != 0; }
  // planes that travel with an fp32 operand buffer: producers (conv epilogue, graph
  // attention, embeddings) emit them, the next conv launch consumes them
  struct PlaneBuf { _Float16* p; size_t n; bool valid; };
  std::map<const float*, PlaneBuf> planes;
  std::vector<std::unique_ptr<DevBuf<_Float16>>> plane_store;
  // producer side; stride 0 tells the producer kernels to write ONE bf16 plane
  _Float16* plane_out(const float* dst, size_t* stride) {
    if (compute_mode == 0) return nullptr;
    if (dyn_x() && xbufs.count(dst)) return nullptr;
    auto it = planes.find(dst);
    if (it == planes.end()) return nullptr;
    it->second.valid = true;
    *stride = compute_mode == 2 ? 0 : it->second.n;
    return it->second.p;
  }
  void plane_invalidate(const float* dst) {
    auto it = planes.find(dst);
    if (it != planes.end()) it->second.valid = false;
  }
  // hipGraph replay of the forward (one graph per (kind, T_pred, U, cell mask: 0 none, 1 one
  // plane, 2 a plane per step -- plus 3 times the same code for the cell bias))
  bool graph_mode = false;
  std::map<std::tuple<ForwardKind, int, int, int>, hipGraphExec_t> graphs;
  int64_t graph_captures = 0;        // forwards captured so far (mv_graph_captures)
  void drop_graphs() {
    for (auto& kv : graphs) (void)hipGraphExecDestroy(kv.second);
    graphs.clear();
    graph_gate_rows.clear();
  }
  // pipelined greedy forward (mv_submit_greedy / mv_collect_greedy): feed of batch k+1 and
  // fetch of batch k-1 on a copy stream while batch k computes
  struct PipeSlot {
    void* pin = nullptr;            // pinned host: inputs, then outputs
    char* dev = nullptr;            // device staging, same layout
    size_t in_bytes = 0, out_bytes = 0;
    hipEvent_t h2d = nullptr, done = nullptr, d2h = nullptr;
    int num_frames = 0, pred_len = 0;
    bool busy = false;
  };
  std::vector<PipeSlot> pipe;
  hipStream_t copy_stream = nullptr;     // H2D (feeds)
  hipStream_t fetch_stream = nullptr;    // D2H (fetches): its own queue, else the feed of
                                         // batch k+1 would sit behind the fetch of batch k,
                                         // which waits for batch k's kernels
  size_t pipe_head = 0, pipe_tail = 0;      // next slot to submit into / to collect from
  // in-library gradient all-reduce (mv_allreduce_init, comm.h); null: single device
  mv::Comm* comm = nullptr;
  // per-row training lengths (mv_set_train_lengths; sticky until cleared): read by the training
  // step alone, never by an inference forward
  TrainLens tl;
  // training state (mv_train_init)
  mv_train_holder* train = nullptr;
  bool train_packs_valid = false;
  // profiling
  bool profiling = false;
  std::vector<KernelStat> stats;
  std::vector<PendingEvent> pending;

  Param* add_param(const std::string& name, std::vector<int64_t> shape) {
    params.emplace_back(new Param());
    Param* p = params.back().get();
    p->name = name;
    p->shape = std::move(shape);
    by_name[name] = p;
    return p;
  }
  int stat_index(const char* name) {
    for (size_t i = 0; i < stats.size(); ++i)
      if (stats[i].name == name) return (int)i;
    stats.push_back(KernelStat{name});
    return (int)stats.size() - 1;
  }
};
