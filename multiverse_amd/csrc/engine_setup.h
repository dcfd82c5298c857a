// engine set-up: parameter table, config validation, buffers, weight packs -- part of the ONE translation unit engine.hip (included from there, in order;
// not a stand-alone header).
#pragma once

namespace {

inline unsigned cdiv(size_t a, size_t b) { return (unsigned)((a + b - 1) / b); }

// hipFuncAttributeMaxDynamicSharedMemorySize is a PROCESS-wide property of the kernel
// (per device): it is only ever raised, so a second engine / mv_op_beam_step with a
// smaller beam_size * K cannot lower the limit under a live engine.
void ensure_beam_step_lds(int device, size_t lds) {
  static std::mutex mu;
  static std::map<int, size_t> granted;
  std::lock_guard<std::mutex> lk(mu);
  MV_REQUIRE(lds <= 160 * 1024, "beam_size*K too large for the LDS beam step (%zu B)", lds);
  size_t& cur = granted[device];
  if (lds > cur) {
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(mv::beam_step_kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(mv::beam_select_kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(mv::sbs_select_kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    cur = lds;
  }
}

// The kernels that hold a K-cell row in one wave's registers (lane l owns k = l + 64 j, j < J)
// are instantiated for J = 3, 9 and kBeamRankJ: fn(std::integral_constant<int, J>) for the
// smallest of them that holds K <= 64 * kBeamRankJ cells.
template <typename F>
void with_rank_j(int K, F&& fn) {
  if (K <= 64 * 3) fn(std::integral_constant<int, 3>{});
  else if (K <= 64 * 9) fn(std::integral_constant<int, 9>{});
  else fn(std::integral_constant<int, mv::kBeamRankJ>{});
}

// fn(std::integral_constant<RowForm, F>) for the form of a constrained step (row_form.h).
template <typename Fn>
void with_row_form(RowForm form, Fn&& fn) {
  switch (form) {
    case RowForm::Plain:  fn(std::integral_constant<RowForm, RowForm::Plain>{}); break;
    case RowForm::Masked: fn(std::integral_constant<RowForm, RowForm::Masked>{}); break;
    case RowForm::Biased: fn(std::integral_constant<RowForm, RowForm::Biased>{}); break;
    case RowForm::Motion: fn(std::integral_constant<RowForm, RowForm::Motion>{}); break;
    case RowForm::Path:   fn(std::integral_constant<RowForm, RowForm::Path>{}); break;
  }
}

// What constrains one decode step, as the step kernels take it (kernels_misc.h RowTerms): the
// allowed cells (mv_set_cell_mask), the cell costs (mv_set_cell_bias), the motion cost of the step
// (mv_set_motion_cost: the tables and where each row's p1 / p0 lie) and its revisit cost
// (mv_set_revisit_cost: the cost and the rows' visited sets).  A part that is not set stays as
// constructed; form() names the launch's instantiation, the empty one launches the plain step.
using StepTerms = mv::RowTerms;

// One beam step (log-softmax + diversity penalty + top-B) in the form step_plan.h's
// beam_step_form chooses.  `cand` = [N*B, K] scratch of the two-launch form.
void launch_beam_step(hipStream_t stream, const float* logits, const float* prev_lp,
                      float* cand, int N, int B, int K, int time, int diverse,
                      float log_gamma, int fix_num_timestep, float* new_lp, int32_t* ids,
                      int32_t* parents, int32_t* src_row, int rows_per_sample,
                      int32_t* row_ref = nullptr, StepTerms terms = StepTerms{}) {
  if (terms.constrained()) {
    require_row_fits_wave(terms.rv.cost ? "beam step under a revisit cost"
                          : terms.mo.vel ? "beam step under a motion cost"
                          : terms.bias ? "beam step under a cell bias"
                                       : "beam step under a cell mask", K);
    MV_REQUIRE(cand, "internal: beam step under a cell mask, bias or motion cost without the "
               "candidate scratch");
  }
  if (beam_step_form(K, cand != nullptr, terms.constrained()) == BeamStepForm::Single) {
    hipLaunchKernelGGL(mv::beam_step_kernel, dim3(N), dim3(512), beam_step_lds_bytes(B, K),
                       stream, logits, prev_lp, B, K, time, diverse, log_gamma,
                       fix_num_timestep, new_lp, ids, parents, src_row, rows_per_sample, row_ref);
    HIP_CHECK(hipGetLastError());   // a refused LDS size must not pass silently
    return;
  }
  const int R = N * B;
  const dim3 grid(cdiv((size_t)R, 4)), block(256);
  with_rank_j(K, [&](auto j) {
    constexpr int J = decltype(j)::value;
    with_row_form(terms.form(), [&](auto f) {
      hipLaunchKernelGGL((mv::beam_rank_kernel<J, decltype(f)::value>), grid, block, 0, stream,
                         logits, prev_lp, R, B, K, time, diverse, log_gamma, cand, terms);
    });
  });
  hipLaunchKernelGGL(mv::beam_select_kernel, dim3(N), dim3(1024),
                     ((size_t)B * K + 64) * sizeof(float), stream, cand, B, K, time,
                     fix_num_timestep, new_lp, ids, parents, src_row, rows_per_sample, row_ref);
  HIP_CHECK(hipGetLastError());
}

// One step of the sampling without replacement (stochastic beam search, kernels_misc.h): the
// perturbed candidates on one wave per parent row, then the per-sample top-B that carries phi,
// LP and G.  t = 0-based decode step; K <= 1024, B <= K.  `cand`, `lp_plane`, `q_plane` =
// [N*B, K] scratch; params = {seed, temperature bits, top_k, top_p bits} on the device.  The
// truncation's floor is B at the first step (the root needs B children), 1 after it.
void launch_sbs_step(hipStream_t stream, const float* logits, const float* prev_phi,
                     const float* prev_lp, const float* prev_g, float* cand, float* lp_plane,
                     float* q_plane, const uint32_t* params, int N, int B, int K, int t,
                     float* new_phi, float* new_lp, float* new_g, int32_t* ids, int32_t* parents,
                     int32_t* src_row, int rows_per_sample, int32_t* row_ref = nullptr,
                     StepTerms terms = StepTerms{}) {
  require_row_fits_wave("sampling without replacement", K);
  MV_REQUIRE(B <= K, "sampling without replacement: beam_size %d > K = %d cells (the first step "
             "has only K distinct candidates)", B, K);
  const int R = N * B;
  const dim3 grid(cdiv((size_t)R, 4)), block(256);
  with_rank_j(K, [&](auto j) {
    constexpr int J = decltype(j)::value;
    with_row_form(terms.form(), [&](auto f) {
      hipLaunchKernelGGL((mv::sbs_perturb_kernel<J, decltype(f)::value>), grid, block, 0, stream,
                         logits, prev_phi, prev_g, R, B, K, t, params, t == 0 ? B : 1, cand,
                         lp_plane, q_plane, terms);
    });
  });
  hipLaunchKernelGGL(mv::sbs_select_kernel, dim3(N), dim3(1024),
                     ((size_t)B * K + 64) * sizeof(float), stream, cand, lp_plane, q_plane, params,
                     prev_phi, prev_lp, B, K, t, new_phi, new_lp, new_g, ids, parents, src_row,
                     rows_per_sample, row_ref, terms.constrained() ? 1 : 0);
  HIP_CHECK(hipGetLastError());
}

// One step of the independent sampler (sample_step_kernel), masked or not; arguments as the
// kernel's.
void launch_sample_step(hipStream_t stream, float* logits, int64_t row_stride, int R, int S,
                        int K, int t, int shared, const uint32_t* params, int floor,
                        const int32_t* lens, float* lp_acc, float* lq_acc, int32_t* ids,
                        int ids_stride, int32_t* src_row, uint8_t* keep_out, StepTerms terms) {
  const dim3 grid(cdiv((size_t)R, 4)), block(256);
  with_rank_j(K, [&](auto j) {
    constexpr int J = decltype(j)::value;
    with_row_form(terms.form(), [&](auto f) {
      hipLaunchKernelGGL((mv::sample_step_kernel<J, decltype(f)::value>), grid, block, 0, stream,
                         logits, row_stride, R, S, K, t, shared, params, floor, lens, lp_acc,
                         lq_acc, ids, ids_stride, src_row, keep_out, terms);
    });
  });
}

// MV_CHAIN_STREAMS=1 keeps the whole greedy forward on one stream (the order before the chain
// pairs, for A/B runs).  MV_CHAIN_PRIORITY=1 creates the regression pair's stream at the lowest
// priority, so that the class pair (attention + transform + gate + tail: the longer critical
// path of a step) is dispatched first; default: plain streams.
void create_chain_streams(mv_engine* e) {
  if (step_knobs().chain_streams != 2) return;
  if (step_knobs().chain_priority) {
    int least = 0, greatest = 0;
    HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    HIP_CHECK(hipStreamCreateWithPriority(&e->stream_b, hipStreamDefault, least));
  } else {
    HIP_CHECK(hipStreamCreate(&e->stream_b));
  }
  HIP_CHECK(hipEventCreateWithFlags(&e->fork_ev, hipEventDisableTiming));
  HIP_CHECK(hipEventCreateWithFlags(&e->join_ev, hipEventDisableTiming));
}

// The chain pair whose launches are being issued (mv_engine::issue / slot0), for a scope.
struct IssueOn {
  mv_engine* e;
  hipStream_t prev;
  int prev_slot0;
  IssueOn(mv_engine* e_, int pair) : e(e_), prev(e_->issue), prev_slot0(e_->slot0) {
    e->issue = pair ? e->stream_b : e->stream;
    e->slot0 = pair ? 2 : 0;
  }
  ~IssueOn() { e->issue = prev; e->slot0 = prev_slot0; }
  IssueOn(const IssueOn&) = delete;
  IssueOn& operator=(const IssueOn&) = delete;
};

// Fork / join of the two chain pairs: stream_b starts after everything queued on `stream` so
// far, and `stream` continues after everything queued on stream_b -- on every way out of the
// forward (a failed check throws between the two).
struct ChainFork {
  mv_engine* e;
  explicit ChainFork(mv_engine* e_) : e(e_) {
    HIP_CHECK(hipEventRecord(e->fork_ev, e->stream));
    HIP_CHECK(hipStreamWaitEvent(e->stream_b, e->fork_ev, 0));
  }
  ~ChainFork() {
    e->issue = e->stream;
    e->slot0 = 0;
    if (hipEventRecord(e->join_ev, e->stream_b) != hipSuccess ||
        hipStreamWaitEvent(e->stream, e->join_ev, 0) != hipSuccess)
      (void)hipStreamSynchronize(e->stream_b);
  }
  ChainFork(const ChainFork&) = delete;
  ChainFork& operator=(const ChainFork&) = delete;
};

// Launch wrapper: optional hipEvent bracket per launch for the roofline figure.
template <typename F>
void launch(mv_engine* e, const char* name, double flops, double bytes, F&& fn,
            double flops_dense = -1.0, double mfma_factor = 0.0) {
  if (!e->profiling) {
    fn();
    return;
  }
  int si = e->stat_index(name);
  PendingEvent pe{si, nullptr, nullptr};
  HIP_CHECK(hipEventCreate(&pe.a));
  HIP_CHECK(hipEventCreate(&pe.b));
  HIP_CHECK(hipEventRecord(pe.a, e->issue));
  fn();
  HIP_CHECK(hipEventRecord(pe.b, e->issue));
  e->stats[si].launches += 1;
  e->stats[si].flops += flops;
  e->stats[si].flops_dense += flops_dense >= 0 ? flops_dense : flops;
  e->stats[si].flops_mfma += mfma_factor * flops;
  e->stats[si].bytes += bytes;
  e->pending.push_back(pe);
}

void drain_events(mv_engine* e) {
  for (auto& pe : e->pending) {
    float ms = 0.f;
    HIP_CHECK(hipEventSynchronize(pe.b));
    HIP_CHECK(hipEventElapsedTime(&ms, pe.a, pe.b));
    e->stats[pe.stat].total_ms += ms;
    (void)hipEventDestroy(pe.a);
    (void)hipEventDestroy(pe.b);
  }
  e->pending.clear();
}

// ------------------------------------------------------------------ setup

void build_param_table(mv_engine* e) {
  const mv_config& c = e->cfg;
  const int64_t C = c.hidden_size, D = c.scene_conv_dim, E = c.emb_size,
                k = c.convlstm_kernel, sk = c.scene_conv_kernel;
  int64_t cin = c.scene_class;
  char nm[256];
  if (e->no_scene()) {
    // no scene stack; the class encoders embed the one-hot map through ONE grid_emb shared by
    // the scales (scope "grid_emb" under person_pred, AUTO_REUSE: code/pred_models.py:218-229)
    e->enc_emb_W = e->add_param("person_pred/grid_emb/W", {3, 3, 1, E});
    e->enc_emb_b = e->add_param("person_pred/grid_emb/b", {E});
  }
  for (int i = 0; i < c.num_scales && !e->no_scene(); ++i) {
    snprintf(nm, sizeof(nm), "person_pred/scene_conv%d/W", i + 1);
    e->scene_W.push_back(e->add_param(nm, {sk, sk, cin, D}));
    snprintf(nm, sizeof(nm), "person_pred/scene_conv%d/b", i + 1);
    e->scene_b.push_back(e->add_param(nm, {D}));
    cin = D;
  }
  for (int s = 0; s < c.num_scales; ++s) {
    ScaleState& S = e->sc[s];
    S.H = c.grid_h[s]; S.W = c.grid_w[s]; S.K = S.H * S.W;
    S.use = c.use_grid[s] != 0;
    if (!S.use) continue;
    auto cell = [&](ConvCell& cc, const char* fmt, int64_t Cx) {
      char base[200];
      snprintf(base, sizeof(base), fmt, s, s);
      cc.Cx = (int)Cx;
      cc.kernel = e->add_param(std::string("person_pred/") + base + "/kernel",
                               {k, k, Cx + C, 4 * C});
      cc.biases = e->add_param(std::string("person_pred/") + base + "/biases", {4 * C});
    };
    cell(S.enc_cls, "encoder_grid_class_%d/enc_grid_%d", e->no_scene() ? E : D);
    cell(S.enc_reg, "encoder_grid_reg_%d/enc_grid_regress_%d", 2);
    cell(S.dec_cls, "decoder_grid_class_%d/decoder_rnn/dec_grid_%d", E);
    snprintf(nm, sizeof(nm), "person_pred/decoder_grid_class_%d/decoder_rnn/grid_emb/W", s);
    S.emb_cls_W = e->add_param(nm, {3, 3, 1, E});
    snprintf(nm, sizeof(nm), "person_pred/decoder_grid_class_%d/decoder_rnn/grid_emb/b", s);
    S.emb_cls_b = e->add_param(nm, {E});
    snprintf(nm, sizeof(nm), "person_pred/hidden2grid_decoder_grid_class_%d/out_dec_grid/W", s);
    S.out_cls_W = e->add_param(nm, {3, 3, C, 1});
    if (c.use_single_decoder) {
      // --use_single_decoder (code/pred_models.py:287-296): no regression decoder; ONE
      // offset kernel for all scales (scope "decode_reg" has no scale index).  The
      // regression encoder is built by the reference but feeds nothing: its variables
      // exist (checkpoints hold them), it is not run and not trained.
      S.enc_reg.kernel->no_grad = S.enc_reg.biases->no_grad = true;
      if (!e->decode_reg_W)
        e->decode_reg_W = e->add_param("person_pred/decode_reg/out_dec_grid/W", {3, 3, C, 2});
      S.out_reg_W = e->decode_reg_W;
      continue;
    }
    cell(S.dec_reg, "decoder_grid_reg_%d/decoder_rnn/dec_grid_reg_%d", E);
    snprintf(nm, sizeof(nm), "person_pred/decoder_grid_reg_%d/decoder_rnn/grid_emb/W", s);
    S.emb_reg_W = e->add_param(nm, {3, 3, 2, E});
    snprintf(nm, sizeof(nm), "person_pred/decoder_grid_reg_%d/decoder_rnn/grid_emb/b", s);
    S.emb_reg_b = e->add_param(nm, {E});
    snprintf(nm, sizeof(nm), "person_pred/hidden2grid_decoder_grid_reg_%d/out_dec_grid/W", s);
    S.out_reg_W = e->add_param(nm, {3, 3, C, 2});
  }
}

// the ConvLSTM cells a forward / training step of this engine runs
std::vector<ConvCell*> active_cells(const mv_engine* e, ScaleState& S) {
  if (e->cfg.use_single_decoder) return {&S.enc_cls, &S.dec_cls};
  return {&S.enc_cls, &S.enc_reg, &S.dec_cls, &S.dec_reg};
}

void validate_config(const mv_config& c) {
  MV_REQUIRE(c.abi_version == MV_ABI_VERSION, "mv_config.abi_version %d != %d",
             c.abi_version, MV_ABI_VERSION);
  MV_REQUIRE(c.activation >= 0 && c.activation <= 2, "mv_config.activation %d (0 tanh, 1 relu, "
             "2 lrelu; reference code/pred_utils.py:86-94)", c.activation);
  MV_REQUIRE(c.batch_size > 0 && c.obs_len > 0 && c.max_pred_len > 0,
             "batch_size/obs_len/max_pred_len must be positive");
  MV_REQUIRE(c.num_scales >= 1 && c.num_scales <= MV_MAX_SCALES,
             "num_scales %d not in [1,%d]", c.num_scales, MV_MAX_SCALES);
  // --enc_hidden_size / --dec_hidden_size (code/train.py:54-57; one value for both, as the
  // reference's own graph requires): whole 128-column blocks of the gate GEMMs and of the
  // f16x3 wgrad tile; the one-wave-per-cell kernels take up to two 256-channel groups
  MV_REQUIRE(c.hidden_size == 128 || c.hidden_size == 256 || c.hidden_size == 512,
             "hidden_size %d unsupported (128, 256 or 512)", c.hidden_size);
  // --convlstm_kernel (code/train.py:70): 3 runs the matrix-pipe kernels; any other size runs
  // the plain fp32 loops of csrc/convlstm_generic.h (compute mode 0 only: slow, but it runs)
  MV_REQUIRE(c.convlstm_kernel >= 1 && c.convlstm_kernel <= 9,
             "convlstm_kernel %d unsupported (1 .. 9)", c.convlstm_kernel);
  // --scene_conv_dim (code/train.py:69): whole 32-channel chunks of the class encoder's x
  // operand; above 64 the graph attention takes its one-wave-per-cell form (two scene
  // channels per lane) and the class encoder its dense x operand
  // (0: a model built without the scene encoder, the reference's default graph)
  MV_REQUIRE(c.scene_conv_dim == 0 ||
             (c.scene_conv_dim > 0 && c.scene_conv_dim <= 128 &&
              mv::convlstm_cx_supported(c.scene_conv_dim)),
             "scene_conv_dim %d unsupported (0 = no scene encoder, or a multiple of 32 up to "
             "128)", c.scene_conv_dim);
  // the decoders' x operand: whole 32-channel chunks of the gate GEMM, 16-byte plane vectors
  // and the decode tail's LDS (decode_tail.h) -- checked here, not at the first decode step
  MV_REQUIRE(c.emb_size >= 32 && c.emb_size % 32 == 0 && c.emb_size <= 512 &&
             mv::convlstm_cx_supported(c.emb_size),
             "emb_size %d unsupported (a multiple of 32 up to 512)", c.emb_size);
  MV_REQUIRE(c.beam_size >= 1, "beam_size must be >= 1");
  MV_REQUIRE(!(c.class_feedback_dense && c.beam_size > 1), "class_feedback_dense: greedy only "
             "(grid_decoder_beam_search always feeds one-hot ids)");
  int hh = c.scene_h, ww = c.scene_w, used = 0;
  for (int s = 0; s < c.num_scales; ++s) {
    hh = (hh + 1) / 2; ww = (ww + 1) / 2;   // stride-2 SAME conv chain
    // process_args' round() and the conv chain's ceil()
    // must agree (true for strides 2,4 on 36x64).
    MV_REQUIRE(c.grid_h[s] == hh && c.grid_w[s] == ww,
               "scene_grids[%d] = %dx%d does not match the stride-2 conv chain "
               "(%dx%d); only scene_grid_strides 2,4,.. are supported",
               s, c.grid_h[s], c.grid_w[s], hh, ww);
    used += c.use_grid[s] != 0;
  }
  MV_REQUIRE(used >= 1, "no grid scale enabled");
  if (c.beam_size > 1)
    MV_REQUIRE(used == 1, "beam search: only one scale at a time "
               "(reference pred_models.py:262)");
}

void alloc_buffers(mv_engine* e) {
  const mv_config& c = e->cfg;
  const size_t N = c.batch_size, T = c.obs_len, Tp = c.max_pred_len,
               C = c.hidden_size, D = c.scene_conv_dim, B = c.beam_size;
  const size_t maxU = N * T;
  const bool scene = !e->no_scene();     // no scene encoder: no scene inputs, no scene stack
  e->obs_scene.alloc(N * T);
  e->lens_dev.alloc(N);
  e->obs_lens_dev.alloc(N);
  e->obs_join_rows.alloc(N);
  if (scene) e->scene_feat.alloc(maxU * c.scene_h * c.scene_w * c.scene_class);
  int hh = c.scene_h, ww = c.scene_w;
  for (int i = 0; i < c.num_scales; ++i) {
    hh = (hh + 1) / 2; ww = (ww + 1) / 2;
    e->conv_h.push_back(hh); e->conv_w.push_back(ww);
    if (scene) e->scene_conv[i].alloc(maxU * hh * ww * D);
  }
  const size_t xc = (size_t)std::max((int)D, c.emb_size);
  for (int s = 0; s < c.num_scales; ++s) {
    ScaleState& S = e->sc[s];
    if (!S.use) continue;
    const size_t K = S.K, R = N * B;
    // (no scene encoder: the graph attention reads no scene channels; one zeroed channel
    // keeps its scene-mean pointer valid)
    S.scene_mean.alloc(N * K * std::max<size_t>(D, 1));
    if (!scene) HIP_CHECK(hipMemset(S.scene_mean.p, 0, N * K * sizeof(float)));
    S.labels.alloc(N * T);
    S.obs_reg.alloc(N * T * K * 2);
    for (int i = 0; i < 2; ++i) {
      // (one more row: the class encoder's background row, enc_cone_on)
      S.cls_c[i].alloc((R + 1) * K * C); S.cls_h[i].alloc((R + 1) * K * C);
      S.reg_c[i].alloc(N * K * C); S.reg_h[i].alloc(N * K * C);
    }
    if (c.use_gnn) S.cls_hg.alloc(R * K * C);
    S.xbuf_cls.alloc(R * K * xc);
    S.xbuf_reg.alloc(N * K * xc);
    S.out_cls.alloc(N * Tp * K);
    S.out_reg.alloc(N * Tp * K * 2);
    S.ids.alloc(R);
    // single decoder + beam: the offsets are decoded from all N*B state rows
    S.q_cls.alloc(R * K * 9); S.q_reg.alloc((c.use_single_decoder ? R : N) * K * 18);
    S.wq_cls.alloc(C * 32); S.wq_reg.alloc(C * 32);
    S.sx_cellyx.alloc(K);
    S.sx_dec_bias.alloc(9 * 4 * C); S.sx_dec_corr.alloc(9 * 25 * 4 * C);
    if (scene) S.sx_enc_corr.alloc(T * N * 9 * 4 * C);
    else { S.sx_enc_bias.alloc(9 * 4 * C); S.sx_enc_tab.alloc(9 * 25 * 4 * C); }
    if (B > 1) {
      e->bm_logits.alloc(Tp * R * K);
      e->bm_ids.alloc(Tp * R);
      e->bm_parents.alloc(Tp * R);
      e->bm_lp[0].alloc(R); e->bm_lp[1].alloc(R);
      e->bm_lp_final.alloc(R);
      e->bm_cand.alloc((size_t)R * K);
      for (int i = 0; i < 2; ++i) { e->bm_phi[i].alloc(R); e->bm_g[i].alloc(R); }
      e->bm_g_final.alloc(R); e->bm_phi_final.alloc(R);
      e->lq_acc.alloc(R);
      e->bm_sbs_lp.alloc((size_t)R * K); e->bm_sbs_q.alloc((size_t)R * K);
      e->bm_src_row.alloc(R);
      e->bm_ref.alloc(R);
      e->bm_trace.alloc(R * Tp);
      e->bm_out_logits.alloc(R * Tp * K);
      e->bm_out_ids.alloc(R * Tp);
      if (c.use_single_decoder) {
        e->bm_reg_steps.alloc(Tp * R * K * 2);
        e->bm_out_reg.alloc(R * Tp * K * 2);
      }
    }
  }
}

void ensure_packed(mv_engine* e, ConvCell& cc) {
  MV_REQUIRE(cc.kernel->set, "parameter %s not set", cc.kernel->name.c_str());
  MV_REQUIRE(cc.biases->set, "parameter %s not set", cc.biases->name.c_str());
  if (cc.wpack.p) return;
  if (e->cfg.convlstm_kernel != 3) return;      // generic taps: straight from the HWIO kernel
  const int C = e->cfg.hidden_size;
  std::vector<float> packed(mv::convlstm_wpack_elems(cc.Cx, C));
  mv::pack_convlstm_weights(cc.kernel->host.data(), cc.Cx, C, packed.data());
  cc.wpack.alloc(packed.size());
  HIP_CHECK(hipMemcpy(cc.wpack.p, packed.data(), packed.size() * sizeof(float),
                      hipMemcpyHostToDevice));
}

CellPacks packs_of(const mv_engine* e, const ConvCell& cc) {
  return cell_packs(e->compute_mode, e->cfg.activation, cc.Cx, e->cfg.hidden_size,
                    cc.wino_numerics_ok);
}

// A small x operand (gate_plan.h x_is_small) is one fp32 chunk of the gate GEMM: the matrix-pipe
// packs then hold the h rows alone ...
std::vector<float> kernel_h_rows(const float* kernel, int Cx, int C) {
  const int Cin = Cx + C, N4 = 4 * C;
  std::vector<float> wh((size_t)9 * C * N4);
  for (int t = 0; t < 9; ++t)
    memcpy(&wh[(size_t)t * C * N4], &kernel[((size_t)t * Cin + Cx) * N4],
           (size_t)C * N4 * sizeof(float));
  return wh;
}
// ... and the x chunk travels beside them: chunk 0 of every column block of the fp32 pack,
// scaled (f16x3: 2^16, bf16: 1)
std::vector<float> small_x_chunk(const float* kernel, int Cx, int C, float scale) {
  std::vector<float> packed(mv::convlstm_wpack_elems(Cx, C));
  mv::pack_convlstm_weights(kernel, Cx, C, packed.data());
  const int nch = mv::convlstm_xchunks(Cx) + 9 * (C / mv::kBK);
  std::vector<float> wx((size_t)(C / mv::kChBlock) * mv::kBN * mv::kBK);
  for (int cb = 0; cb < C / mv::kChBlock; ++cb)
    for (int i = 0; i < mv::kBN * mv::kBK; ++i)
      wx[(size_t)cb * mv::kBN * mv::kBK + i] =
          packed[((size_t)cb * nch + 0) * mv::kBN * mv::kBK + i] * scale;
  return wx;
}
template <typename T>
void upload(DevBuf<T>& dst, const std::vector<T>& src) {
  dst.alloc(src.size());
  HIP_CHECK(hipMemcpy(dst.p, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
}
void refresh_host_copy(ConvCell& cc) {
  if (!cc.host_stale) return;
  HIP_CHECK(hipMemcpy(cc.kernel->host.data(), cc.kernel->dev.p,
                      cc.kernel->elems() * sizeof(float), hipMemcpyDeviceToHost));
  cc.host_stale = false;
}

// f16x3 packs (two scaled fp16 planes in fragment order; the fp32 x chunk of the
// 2-channel regression-encoder input scaled by 2^16), from the CURRENT weights.
void ensure_packed16(mv_engine* e, ConvCell& cc) {
  if (cc.wp16.p) return;
  const int C = e->cfg.hidden_size;
  MV_REQUIRE(mv::f16x3_cx_supported(cc.Cx), "f16x3: Cx %d unsupported", cc.Cx);
  refresh_host_copy(cc);
  {   // 256 w must stay inside fp16 (|w| < 255): true of any sane checkpoint, checked anyway
    float mx = 0.f;
    for (float v : cc.kernel->host) mx = std::max(mx, std::fabs(v));
    // the Winograd packs store TRANSFORMED kernel rows -- (g0 +- g1 + g2) / 2 (F(2,3));
    // (g0 + g1 + g2) / 2, (g0 - g1 + g2) / 6, (g0 + 2 g1 + 4 g2) / 6 (F(3,3)); the dgrad pack the
    // same of the flipped rows -- which reach up to 1.5 max |w| when three taps of one column
    // share a sign: the bound is taken on THOSE values, column by column
    float reach = mx;
    if (cell_packs(1, e->cfg.activation, cc.Cx, C, true).wpw) {   // whatever the outlier test says
      const size_t Cin = (size_t)cc.Cx + C, N4 = 4 * (size_t)C;
      const float* w = cc.kernel->host.data();
      for (size_t dxc = 0; dxc < 3 * Cin; ++dxc) {          // (dx, input channel) pairs
        const size_t dx = dxc / Cin, ci = dxc - dx * Cin;
        const float* g0 = w + ((0 * 3 + dx) * Cin + ci) * N4;
        const float* g1 = w + ((1 * 3 + dx) * Cin + ci) * N4;
        const float* g2 = w + ((2 * 3 + dx) * Cin + ci) * N4;
        for (size_t n = 0; n < N4; ++n) {
          const float a = g0[n], b = g1[n], c2 = g2[n];
          const float t = std::max(std::max(std::fabs(a + b + c2), std::fabs(a - b + c2)) * 0.5f,
                                   std::max(std::fabs(a + 2.f * b + 4.f * c2),
                                            std::fabs(4.f * a + 2.f * b + c2)) * (1.f / 6.f));
          reach = std::max(reach, t);
        }
      }
    }
    MV_REQUIRE(reach * mv::kF16Scale < 60000.f, "f16x3: |%s| reaches %g (%g in the transformed "
               "kernel planes of the Winograd forms), outside the scaled fp16 range; use compute "
               "mode f32", cc.kernel->name.c_str(), mx, reach);
    // outlier test for the Winograd forms (ConvCell::wino_numerics_ok): median of |w|
    std::vector<float> mag(cc.kernel->host.size());
    for (size_t i = 0; i < mag.size(); ++i) mag[i] = std::fabs(cc.kernel->host[i]);
    std::nth_element(mag.begin(), mag.begin() + mag.size() / 2, mag.end());
    const float med = mag[mag.size() / 2];
    const bool ok = mx <= kWinoOutlierRatio * med;
    if (!ok && cc.wino_numerics_ok)
      fprintf(stderr, "[multiverse_hip] f16x3: %s has max |w| %g at a median |w| of %g (> %g x): "
              "its gate convolution takes the direct 3x3 form instead of a Winograd form "
              "(roundoff of outlier weights would reach unrelated outputs)\n",
              cc.kernel->name.c_str(), mx, med, kWinoOutlierRatio);
    if (ok != cc.wino_numerics_ok) { cc.wpw.release(); cc.wpw3.release(); }
    cc.wino_numerics_ok = ok;
  }
  // the h part (and an x part that is a multiple of 16 channels) as fp16 planes
  std::vector<_Float16> p16(mv::f16x3_wpack_elems(x_chunk16(cc.Cx), C));
  if (x_is_small(cc.Cx)) {
    mv::pack_f16x3_weights(kernel_h_rows(cc.kernel->host.data(), cc.Cx, C).data(), 0, C, p16.data());
    upload(cc.wx32, small_x_chunk(cc.kernel->host.data(), cc.Cx, C, 65536.0f));
  } else {
    mv::pack_f16x3_weights(cc.kernel->host.data(), cc.Cx, C, p16.data());
  }
  upload(cc.wp16, p16);
}

// Device-side packs of the kernel `w` (HWIO, fp32, on the device) into `dst`: Winograd F(2,3) of
// the f16x3 forward (convlstm_wino.h; the transform of the kernel rows runs in fp64), Winograd
// F(3,3) (convlstm_wino3.h), and the bf16 mode's row-triple tile (convlstm_wino3.h BF16D).  The
// first two also raise their kernels' dynamic-LDS limit: packing never runs inside a graph capture.
void pack_wino(hipStream_t stream, const float* w, int Cx, int C, DevBuf<_Float16>& dst) {
  const size_t halves = mv::wino_wpack_elems(x_chunk16(Cx), C);
  mv::wino_init_attributes();
  dst.alloc(halves);
  hipLaunchKernelGGL(mv::pack_wino_kernel, dim3(cdiv(halves / 2, 256)), dim3(256), 0, stream, w,
                     dst.p, Cx, x_chunk16(Cx), C, halves / 2);
}
void pack_wino3(hipStream_t stream, const float* w, int Cx, int C, DevBuf<_Float16>& dst) {
  const size_t halves = mv::wino3_wpack_elems(x_chunk16(Cx), C, mv::kW3Nrb);
  mv::wino3_init_attributes();
  dst.alloc(halves);
  hipLaunchKernelGGL(mv::pack_wino3_kernel, dim3(cdiv(halves / 2, 256)), dim3(256), 0, stream, w,
                     dst.p, Cx, x_chunk16(Cx), C, mv::kW3Nrb, halves / 2);
}
void pack_bf16t(hipStream_t stream, const float* w, int Cx, int C, DevBuf<_Float16>& dst) {
  const size_t halves = mv::bf16t_wpack_elems(x_chunk16(Cx), C, mv::kW3Nrb);
  dst.alloc(halves);
  hipLaunchKernelGGL(mv::pack_bf16t_kernel, dim3(cdiv(halves, 256)), dim3(256), 0, stream, w,
                     dst.p, Cx, x_chunk16(Cx), C, mv::kW3Nrb, halves);
}
// every weight-mutating path comes through here (or releases the packs): a non-null pack is by
// construction a pack of the CURRENT device weights -- re-packed in place when the cell carries
// the form (no hipFree / hipMalloc per training step: they synchronise the device), released
// otherwise
void pack_tile_forms(mv_engine* e, ConvCell& cc) {
  const CellPacks p = packs_of(e, cc);
  const int C = e->cfg.hidden_size;
  if (e->compute_mode == 1) {      // (another mode's packs stay: they are of the same weights)
    if (p.wpw) pack_wino(e->stream, cc.kernel->dev.p, cc.Cx, C, cc.wpw); else cc.wpw.release();
    if (p.wpw3) pack_wino3(e->stream, cc.kernel->dev.p, cc.Cx, C, cc.wpw3); else cc.wpw3.release();
  } else if (e->compute_mode == 2) {
    if (p.wpbt) pack_bf16t(e->stream, cc.kernel->dev.p, cc.Cx, C, cc.wpbt); else cc.wpbt.release();
  }
}

// bf16 packs (one unscaled plane; the 2-channel regression-encoder input keeps its fp32
// chunk), from the CURRENT weights.
void ensure_packed_bf16(mv_engine* e, ConvCell& cc) {
  if (cc.wpb.p) return;
  const int C = e->cfg.hidden_size;
  MV_REQUIRE(mv::f16x3_cx_supported(cc.Cx), "bf16: Cx %d unsupported", cc.Cx);
  refresh_host_copy(cc);
  const bool xf16 = bf16_x_passes(2, e->dyn_x(), x_is_small(cc.Cx)) == 3;
  std::vector<_Float16> pb(mv::bf16_wpack_elems(x_chunk16(cc.Cx), C, xf16));
  if (x_is_small(cc.Cx)) {
    mv::pack_bf16_weights(kernel_h_rows(cc.kernel->host.data(), cc.Cx, C).data(), 0, C, pb.data());
    upload(cc.wx32u, small_x_chunk(cc.kernel->host.data(), cc.Cx, C, 1.0f));
  } else {
    if (xf16) {        // the x rows travel as fp16 of 256 w there: same range bound as f16x3
      const int Cin = cc.Cx + C, N4 = 4 * C;
      float mx = 0.f;
      for (int t = 0; t < 9; ++t)
        for (int ci = 0; ci < cc.Cx; ++ci)
          for (int n = 0; n < N4; ++n)
            mx = std::max(mx, std::fabs(cc.kernel->host[((size_t)t * Cin + ci) * N4 + n]));
      MV_REQUIRE(mx * mv::kF16Scale < 60000.f, "bf16 mode, unbounded activations: the x rows of "
                 "%s reach %g, outside the scaled fp16 range; use compute mode f32",
                 cc.kernel->name.c_str(), mx);
    }
    mv::pack_bf16_weights(cc.kernel->host.data(), cc.Cx, C, pb.data(), xf16);
  }
  upload(cc.wpb, pb);
  pack_tile_forms(e, cc);
}

// scene channels the graph attention sees: all of them, except in the greedy decoder of the
// SimAug fork's graph (mv_config.simaug_graph), which attends over the hidden state alone
int gnn_scene_dim(const mv_engine* e) {
  return (e->cfg.simaug_graph && e->cfg.beam_size == 1) ? 0 : e->cfg.scene_conv_dim;
}

bool sparse_x_on(const mv_engine* e, const ScaleState& S) {
  const mv_config& c = e->cfg;
  return step_knobs().sparse_x && e->compute_mode != 0 && !e->train && S.use && S.H >= 3 && S.W >= 3 &&
         S.dec_cls.Cx == c.emb_size && c.emb_size % 16 == 0 && c.scene_conv_dim % 16 == 0 &&
         c.scene_conv_dim <= 64;
}

// Does the class encoder of this scale run on its light cone in the forward being issued
// (gate_plan.h enc_cone_planned decides; this gathers what it asks)?  Asked after ensure_params:
// the packs say which form the encoder cells take.  A ragged forward whose encoders run on a
// prefix of the batch keeps the dense encoder (the lists are built for the whole batch), and so
// does an obs-ragged one (mv_set_obs_lengths: the lists and the one background row are built for
// a common start).
bool enc_cone_on(mv_engine* e, ScaleState& S) {
  const mv_config& c = e->cfg;
  bool step_exact = true;
  for (int s = 0; s < c.num_scales; ++s) {
    ScaleState& O = e->sc[s];
    if (!O.use) continue;
    step_exact = step_exact &&
                 cone_step_member_ok(O.H, O.W, O.enc_cls.wpw3.p &&
                                                   (c.use_single_decoder || O.enc_reg.wpw3.p));
  }
  return S.cone_ready && S.cone.p && e->rows_at(0) == c.batch_size && !e->obs.ragged &&
         enc_cone_planned(e->compute_mode, c.activation, sparse_x_on(e, S), step_exact, c.obs_len,
                          S.H, S.W, c.hidden_size, c.batch_size);
}

void ensure_params(mv_engine* e) {
  for (auto& p : e->params)
    MV_REQUIRE(p->set, "parameter %s not set (mv_set_param)", p->name.c_str());
  for (int s = 0; s < e->cfg.num_scales; ++s) {
    ScaleState& S = e->sc[s];
    if (!S.use) continue;
    for (ConvCell* cc : active_cells(e, S)) ensure_packed(e, *cc);
    if (e->compute_mode == 1)
      for (ConvCell* cc : active_cells(e, S)) ensure_packed16(e, *cc);
    if (e->compute_mode == 1)     // (after ensure_packed16: it runs the outlier test)
      for (ConvCell* cc : active_cells(e, S))
        if (packs_of(e, *cc).wpw && !cc->wpw.p) pack_tile_forms(e, *cc);
    if (e->compute_mode == 2)
      for (ConvCell* cc : active_cells(e, S)) ensure_packed_bf16(e, *cc);
    if (!S.wq_valid) {     // hidden2grid tap packs, from the CURRENT device weights
      const int C = e->cfg.hidden_size;
      hipLaunchKernelGGL(mv::pack_h2g_kernel, dim3(cdiv((size_t)C * 32, 256)), dim3(256), 0,
                         e->stream, S.out_cls_W->dev.p, S.wq_cls.p, C, 1);
      hipLaunchKernelGGL(mv::pack_h2g_kernel, dim3(cdiv((size_t)C * 32, 256)), dim3(256), 0,
                         e->stream, S.out_reg_W->dev.p, S.wq_reg.p, C, 2);
      S.wq_valid = true;
    }
    if (!S.sx_valid && sparse_x_on(e, S)) {
      const int C = e->cfg.hidden_size;
      hipLaunchKernelGGL(mv::cell_yx_kernel, dim3(cdiv((size_t)S.K, 256)), dim3(256), 0,
                         e->stream, S.sx_cellyx.p, S.H, S.W);
      hipLaunchKernelGGL(mv::sx_decoder_tables_kernel,
                         dim3(cdiv((size_t)(9 + 9 * 25) * 4 * C, 256)), dim3(256), 0, e->stream,
                         S.dec_cls.kernel->dev.p, S.dec_cls.biases->dev.p, S.emb_cls_W->dev.p,
                         S.emb_cls_b->dev.p, S.dec_cls.Cx, C, S.sx_dec_bias.p, S.sx_dec_corr.p,
                         e->cfg.activation);
      if (e->no_scene())   // the class encoder's x is grid_emb(one_hot) too: the same tables
        hipLaunchKernelGGL(mv::sx_decoder_tables_kernel,
                           dim3(cdiv((size_t)(9 + 9 * 25) * 4 * C, 256)), dim3(256), 0,
                           e->stream, S.enc_cls.kernel->dev.p, S.enc_cls.biases->dev.p,
                           e->enc_emb_W->dev.p, e->enc_emb_b->dev.p, S.enc_cls.Cx, C,
                           S.sx_enc_bias.p, S.sx_enc_tab.p, e->cfg.activation);
      S.sx_valid = true;
    }
  }
}

}  // namespace
