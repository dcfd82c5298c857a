// the forward pass: grouped gate launches, scene stack, encoders, graph attention, decode tail, greedy / beam decoders -- part of the ONE translation unit engine.hip (included from there, in order;
// not a stand-alone header).
#pragma once

namespace {

// ------------------------------------------------------------------ launches

using mv::ConvLstmArgs;

// class-chain x operands as table terms (sparse_x.h): f16x3 / bf16 inference engines only
// (the training forward keeps the dense x: the backward pass needs it).  MV_SPARSE_X=0
// restores the dense operand for A/B runs.
void set_sparse_x(mv_engine* e, ScaleState& S, ConvLstmArgs& a, bool decoder,
                  const int32_t* hot, int hot_stride, int hot_div) {
  a.sx_bias = decoder ? S.sx_dec_bias.p : nullptr;
  a.sx_corr = decoder ? S.sx_dec_corr.p : S.sx_enc_corr.p;
  a.sx_hot = hot; a.sx_hot_stride = hot_stride; a.sx_hot_div = hot_div;
  a.sx_cellyx = S.sx_cellyx.p;
  a.sx_rad = decoder ? 2 : 1;
  a.sx_by_class = decoder ? 1 : 0;
}

ConvLstmArgs conv_problem(mv_engine* e, const ConvCell& cc, const float* x,
                          const float* h, const float* c, const int32_t* src_row_h,
                          const int32_t* src_row_c, float* h_out, float* c_out,
                          int rows, int H, int W, bool zero_state,
                          size_t x_row_stride = 0, bool want_h16 = true) {
  ConvLstmArgs a{};
  // the kernel forms element offsets in 32-bit registers
  const size_t xrs = x_row_stride ? x_row_stride : (size_t)H * W * cc.Cx;
  MV_REQUIRE((size_t)rows * H * W * e->cfg.hidden_size < ((size_t)1 << 31) &&
             (size_t)rows * xrs < ((size_t)1 << 31),
             "ConvLSTM state of %d rows exceeds the 2^31-element addressing of one "
             "launch; lower batch_size x beam_size", rows);
  a.x_row_stride = (int32_t)xrs;
  a.x = x; a.h = h; a.c = c; a.src_row_h = src_row_h; a.src_row_c = src_row_c;
  a.wpack = cc.wpack.p; a.bias = cc.biases->dev.p;
  a.h_out = h_out; a.c_out = c_out;
  a.rows = rows; a.H = H; a.W = W; a.Cx = cc.Cx; a.C = e->cfg.hidden_size;
  mv::convlstm_finish_args(a, zero_state);
  a.want_h16 = want_h16 ? 1 : 0;
  return a;
}

ConvCell* cell_of_bias(mv_engine* e, const float* bias) {
  for (int s = 0; s < e->cfg.num_scales; ++s) {
    ScaleState& S = e->sc[s];
    if (!S.use) continue;                  // an unused scale's cells have no parameters
    for (ConvCell* cc : active_cells(e, S))
      if (cc->biases && cc->biases->dev.p == bias) return cc;
  }
  throw HipError{"internal: unknown ConvLSTM cell"};
}

ConvCell* cell_of_pack(mv_engine* e, const float* wpack) {
  for (int s = 0; s < e->cfg.num_scales; ++s) {
    ScaleState& S = e->sc[s];
    for (ConvCell* cc : active_cells(e, S))
      if (cc->wpack.p == wpack) return cc;
  }
  throw HipError{"internal: unknown weight pack"};
}

// ---- f16x3 / bf16 compute modes: prepare the operand planes, plan the launch (gate_plan.h),
// queue the F(3,3) input transforms, launch.

// Operand planes of every problem of a group: the planes a producer left, or a split of the fp32
// operand into the slot's scratch (one grouped launch; unbounded x operands one by one, under
// their own exponent).  Fills p16[i] up to the weight packs.
void prepare_gate_operands(mv_engine* e, const std::vector<ConvLstmArgs>& probs,
                           const std::vector<ConvCell*>& cells,
                           std::vector<mv::ConvLstm16Args>& p16) {
  struct SplitItem { const float* in; _Float16* p0; _Float16* p1; int cells, C; };
  std::vector<SplitItem> splits;
  struct DynItem { const float* in; _Float16* p0; _Float16* p1; int cells, C; int32_t* bits; };
  std::vector<DynItem> dyn_splits;
  const bool bf16 = e->compute_mode == 2;
  auto ready = [&](const float* src) -> const mv_engine::PlaneBuf* {
    auto it = e->planes.find(src);
    return (it != e->planes.end() && it->second.valid) ? &it->second : nullptr;
  };
  for (size_t i = 0; i < probs.size(); ++i) {
    const ConvLstmArgs& a = probs[i];
    mv::ConvLstm16Args& q = p16[i];
    const size_t sl = (size_t)e->slot0 + i;      // the group slot of the pair being issued
    // the kernel's epilogue lets a 32-cell wave tile span at most two images
    MV_REQUIRE(a.H * a.W >= 32, "f16x3 / bf16 compute modes need grids of at least 32 cells "
               "(%d x %d); use compute mode f32", a.H, a.W);
    MV_REQUIRE((double)a.rows * a.H * a.W * a.C * 4.0 < 4294967296.0,
               "f16x3 / bf16 compute modes: state tensor of %d rows exceeds 4 GB", a.rows);
    // the training forward stores the four gate activations [M][4C] through a buffer
    // resource with 32-bit byte offsets (convlstm_f16x3.h epilogue: num_records = 16 M C)
    MV_REQUIRE(!a.gates_out || (double)a.rows * a.H * a.W * a.C * 16.0 < 4294967296.0,
               "f16x3 / bf16 training forward: gate tensor of %d rows exceeds 4 GB "
               "(lower the per-GPU batch or use compute mode f32)", a.rows);
    q.f = a;
    q.wp16 = bf16 ? cells[i]->wpb.p : cells[i]->wp16.p;
    q.wx32 = bf16 ? cells[i]->wx32u.p : cells[i]->wx32.p;
    const size_t ncell = (size_t)a.rows * a.H * a.W;
    // A ragged TRAINING step (TrainLens) changes a.rows from launch to launch, and its operands
    // always take the slot's scratch: the second plane keeps the place it has at full batch, so
    // that the zero halves in front of it (kPlanePad, which no split writes) are never inside
    // what an earlier launch of another row count left there.
    const size_t ncell_st = e->tl.issuing ? (size_t)e->cfg.batch_size * a.H * a.W : ncell;
    // bf16 mode, unbounded activations: three x passes (convlstm_f16x3.h xpasses)
    const int xpass = bf16_x_passes(e->compute_mode, e->dyn_x(), a.x_small);
    q.n_xk = a.x_small ? 0 : xpass * mv::f16x3_xksteps(a.Cx);
    q.n_hk = a.zero_state ? 0 : 9 * (a.C / 16);
    q.w_ksteps = (a.x_small ? 0 : xpass * mv::f16x3_xksteps(a.Cx)) + 9 * (a.C / 16);
    if (bf16)       // an LDS stage of the bf16 kernel holds MV_BF16_UNITS row units of 3 k-steps
      MV_REQUIRE((q.n_xk / 3) % MV_BF16_UNITS == 0 && (q.n_hk / 3) % MV_BF16_UNITS == 0,
                 "bf16 mode: %d x / %d h k-steps do not fill whole LDS stages (emb_size and "
                 "scene_conv_dim must be multiples of 32)", q.n_xk, q.n_hk);
    q.x16 = nullptr; q.h16 = nullptr;
    q.x_plane_stride = q.h_plane_stride = 0;
    // The conv epilogue emits the operand planes of h' (assembled per wave in LDS,
    // 16-byte stores) when the next consumer of h' is a gate convolution; MV_EPI_PLANES=0
    // falls back to the separate split pass over the fp32 h'.
    q.h16_out = nullptr;
    q.h16_out_stride = 0;
    e->plane_invalidate(a.h_out);
    if (gate_knobs().epi_planes && a.want_h16 && !a.gates_out) {
      size_t pst = 0;
      if (_Float16* po = e->plane_out(a.h_out, &pst)) {   // marks the planes valid
        q.h16_out = po;
        q.h16_out_stride = (int64_t)pst;
      }
    }
    q.f.skip_h32 = (a.skip_h32 && q.h16_out && !e->train) ? 1 : 0;
    if (has_dense_x(a)) {
      MV_REQUIRE((size_t)a.x_row_stride == (size_t)a.H * a.W * a.Cx,
                 "internal: f16x3 needs a contiguous x operand");
      if (const auto* pb = ready(a.x)) {
        q.x16 = pb->p; q.x_plane_stride = (int64_t)pb->n;
      } else {
        const size_t pst = ncell_st * a.Cx + mv::kPlaneSlack + mv::kPlanePad;
        MV_REQUIRE(e->px16[sl].n >= 2 * pst, "internal: f16x3 x plane scratch");
        _Float16* p0 = e->px16[sl].p + mv::kPlanePad;
        q.x16 = p0; q.x_plane_stride = (int64_t)pst;
        if (e->dyn_x()) {       // unbounded activations: planes of 2^e x, e from max |x|
          MV_REQUIRE(e->xexp[sl].p, "internal: x exponent scratch");
          q.x_exp = e->xexp[sl].p + 64;
          dyn_splits.push_back(DynItem{a.x, p0, p0 + pst, (int)ncell, a.Cx, e->xexp[sl].p});
        } else {
          splits.push_back(SplitItem{a.x, p0, bf16 ? (_Float16*)nullptr : p0 + pst, (int)ncell, a.Cx});
        }
      }
      // the three-pass x kernel of the bf16 mode is chosen per launch from the problems' x
      // exponents, the weight packs per cell from dyn_x(): they must agree
      MV_REQUIRE(!(bf16 && e->dyn_x()) || q.x_exp, "internal: bf16 mode, unbounded activations: "
                 "a dense x operand came as producer planes, without its exponent");
    }
    if (!a.zero_state) {      // source rows == rows (beam: permuted, same count)
      if (const auto* pb = ready(a.h)) {
        q.h16 = pb->p; q.h_plane_stride = (int64_t)pb->n;
      } else {
        const size_t pst = ncell_st * a.C + mv::kPlaneSlack + mv::kPlanePad;
        MV_REQUIRE(e->ph16[sl].n >= 2 * pst, "internal: f16x3 h plane scratch");
        _Float16* p0 = e->ph16[sl].p + mv::kPlanePad;
        q.h16 = p0; q.h_plane_stride = (int64_t)pst;
        splits.push_back(SplitItem{a.h, p0, bf16 ? (_Float16*)nullptr : p0 + pst, (int)ncell, a.C});
      }
    }
  }
  for (const DynItem& it : dyn_splits) {
    launch(e, "split_planes", 0, 12.0 * (double)it.cells * it.C, [&] {
      HIP_CHECK(hipMemsetAsync(it.bits, 0, 64 * sizeof(int32_t), e->issue));
      hipLaunchKernelGGL(mv::absmax_bits_kernel, dim3(256), dim3(256), 0, e->issue, it.in,
                         (size_t)it.cells * it.C, it.bits);
      hipLaunchKernelGGL(mv::split_planes_dyn_kernel,
                         dim3(mv::split_planes_blocks((size_t)it.cells, it.C)), dim3(256), 0,
                         e->issue, it.in, it.p0, it.p1, it.cells, it.C, it.bits, it.bits + 64);
    });
  }
  // operands no producer left as planes: one grouped split launch in front of the gate kernel
  for (size_t s0 = 0; s0 < splits.size(); s0 += mv::kSplitGroup) {
    mv::SplitGroup g{};
    double sbytes = 0;
    unsigned nb = 0;
    g.n = (int)std::min<size_t>(mv::kSplitGroup, splits.size() - s0);
    for (int j = 0; j < g.n; ++j) {
      const SplitItem& it = splits[s0 + j];
      g.in[j] = it.in; g.p0[j] = it.p0; g.p1[j] = it.p1; g.M[j] = it.cells; g.C[j] = it.C;
      nb += mv::split_planes_blocks((size_t)it.cells, it.C);
      g.blk_end[j] = nb;
      sbytes += (bf16 ? 6.0 : 8.0) * (double)it.cells * it.C;
    }
    launch(e, "split_planes", 0, sbytes, [&] {
      hipLaunchKernelGGL(mv::split_planes_group_kernel, dim3(nb), dim3(256), 0, e->issue, g);
    });
  }
}

// F(3,3): the input transform of every operand of the group runs ONCE, in a pre-pass into `out`,
// instead of in every one of the C / 16 column-block workgroups of the gate kernel.
double queue_wino3_transform(std::vector<mv::Wn3TransformItem>& tr, const mv::Wn3TransformItem& it) {
  tr.push_back(it);
  // (light cone: the tiles the step transforms, not the whole operand)
  const double cells = it.cone_cells ? (double)it.cone_cells : (double)it.rows * it.H * it.W;
  return cells * it.Cc * 4.0 * (1.0 + 5.0 / 3.0);     // bytes moved
}

// The grouped gate launch in the planned form.  p16: the prepared problems; packs: per problem
// the pack of that form; v3x / v3h: per problem the pre-transformed operands (Wino3), or NULL.
void launch_gate_group(const ForwardPlan& pl, const mv::ConvLstm16Args* p16,
                       const _Float16* const* packs, const float* const* w_hwio,
                       _Float16* const* v3x, _Float16* const* v3h, int n, hipStream_t stream) {
  if (pl.form == GateForm::Direct16)
    return mv::launch_convlstm16_steps(p16, n, pl.shift, pl.map_mode, stream);
  if (pl.form == GateForm::Bf16)
    return mv::launch_convlstm_bf16_steps(p16, n, pl.shift, pl.map_mode, pl.x_passes == 3, stream);
  mv::ConvLstmWinoArgs pw[mv::kMaxGroup] = {};
  for (int i = 0; i < n; ++i) {
    pw[i].b = p16[i];
    pw[i].wpw = packs[i];
    pw[i].w_hwio = w_hwio[i];
    pw[i].n_xc = p16[i].f.x_small ? 0 : p16[i].f.Cx / 16;
    pw[i].v3x = v3x ? v3x[i] : nullptr;
    pw[i].v3h = v3h ? v3h[i] : nullptr;
  }
  if (pl.form == GateForm::Wino2) mv::launch_convlstm_wino_steps(pw, n, pl.map_mode, stream);
  else if (pl.form == GateForm::Wino3)
    mv::launch_convlstm_wino3_steps(pw, n, pl.halo, pl.map_mode, stream);
  else mv::launch_convlstm_bf16t_steps(pw, n, pl.halo, pl.map_mode, stream);
}

// A gate group with its operands prepared: the problems, their cells, the group slots they use.
struct GatePrep {
  std::vector<ConvCell*> cells;
  std::vector<mv::ConvLstm16Args> p16;
  int slot0 = 0;
  double flops = 0, bytes = 0, dense = 0;
  int n() const { return (int)p16.size(); }
};

// dense: the step as the reference computes it; executed: a zero-state step
// (first encoder step) never multiplies the h half and never reads h, c
void gate_group_cost(const std::vector<ConvLstmArgs>& probs, double& flops, double& bytes,
                     double& dense) {
  flops = bytes = dense = 0;
  for (const auto& a : probs) {
    // light cone of the class encoder: the reference computes the batch's rows, the launch the
    // cone's tiles (and the background row)
    const double Md = (double)(a.rows - (a.cone_on ? 1 : 0)) * a.H * a.W;
    const double M = a.cone_cells ? (double)a.cone_cells : (double)a.rows * a.H * a.W;
    dense += 2.0 * Md * 9.0 * (a.Cx + a.C) * 4.0 * a.C;
    // sparse x: the x k-steps are not executed (table terms in the epilogue)
    const double cx = a.sx_corr ? 0.0 : (double)a.Cx;
    flops += 2.0 * M * 9.0 * (cx + (a.zero_state ? 0 : a.C)) * 4.0 * a.C;
    bytes += M * (cx + (a.zero_state ? 2.0 : 4.0) * a.C) * 4.0;   // x,(h,c) in; h,c out
  }
}

GatePrep prepare_gate_group(mv_engine* e, const std::vector<ConvLstmArgs>& probs) {
  GatePrep g;
  const int n = (int)probs.size();
  MV_REQUIRE(e->slot0 + n <= mv::kMaxGroup, "internal: gate group of %d problems from slot %d",
             n, e->slot0);
  g.slot0 = e->slot0;
  g.cells.resize(n);
  for (int i = 0; i < n; ++i) g.cells[i] = cell_of_pack(e, probs[i].wpack);
  g.p16.resize(n);
  prepare_gate_operands(e, probs, g.cells, g.p16);
  gate_group_cost(probs, g.flops, g.bytes, g.dense);
  return g;
}

// ONE plan for the gate launches of a step: the groups of both chain pairs take the form, the
// tiling and the block map that the step's single grouped launch would take, so a chain's
// kernel does not depend on how the step's problems are spread over launches.
ForwardPlan plan_gate_groups(mv_engine* e, const GatePrep* const* groups, int ngroups) {
  ForwardProblem fp[mv::kMaxGroup];
  int n = 0;
  for (int g = 0; g < ngroups; ++g)
    for (int i = 0; i < groups[g]->n(); ++i) {
      MV_REQUIRE(n < mv::kMaxGroup, "internal: more than %d gate problems in a step", mv::kMaxGroup);
      const int sl = groups[g]->slot0 + i;
      fp[n++] = ForwardProblem{&groups[g]->p16[i], groups[g]->cells[i], e->pv3x[sl].n, e->pv3h[sl].n};
    }
  const ForwardPlan pl = plan_forward_group(e->compute_mode, fp, n);
  check_cone_plan(pl, fp, n);
  return pl;
}

// Input transforms (F(3,3)) and the grouped gate launch of a prepared group, on e->issue.
void issue_gate_group(mv_engine* e, const GatePrep& g, const ForwardPlan& pl) {
  const int n = g.n();
  const _Float16* packs[mv::kMaxGroup] = {};
  const float* w_hwio[mv::kMaxGroup] = {};
  _Float16 *v3x[mv::kMaxGroup] = {}, *v3h[mv::kMaxGroup] = {};
  std::vector<mv::Wn3TransformItem> tr3;
  double tr3_bytes = 0;
  for (int i = 0; i < n; ++i) {
    const mv::ConvLstm16Args& q = g.p16[i];
    const ConvLstmArgs& a = q.f;
    const int sl = g.slot0 + i;
    w_hwio[i] = g.cells[i]->kernel->dev.p;
    packs[i] = pl.form == GateForm::Wino2 ? g.cells[i]->wpw.p
             : pl.form == GateForm::Wino3 ? g.cells[i]->wpw3.p
             : pl.form == GateForm::Bf16T ? g.cells[i]->wpbt.p : nullptr;
    if (pl.form != GateForm::Wino3) continue;
    if (!a.zero_state) {
      v3h[i] = e->pv3h[sl].p;
      tr3_bytes += queue_wino3_transform(tr3, {q.h16, q.h_plane_stride, v3h[i], a.src_row_h,
                                               a.rows, a.H, a.W, a.C, a.cone_list, a.cone_prev,
                                               a.cone_cells});
    }
    if (has_dense_x(a)) {
      v3x[i] = e->pv3x[sl].p;
      tr3_bytes += queue_wino3_transform(tr3, {q.x16, q.x_plane_stride, v3x[i], nullptr,
                                               a.rows, a.H, a.W, a.Cx});
    }
  }
  if (!tr3.empty())
    launch(e, "wino3_transform", 0, tr3_bytes, [&] {
      mv::launch_wino3_transforms(tr3.data(), (int)tr3.size(), e->issue);
    });
  for (int i = 0; i < n; ++i)      // (the batch's rows: not the encoder's background row)
    e->gate_rows += g.p16[i].f.rows - (g.p16[i].f.cone_on ? 1 : 0);
  launch(e, "convlstm_step", g.flops, g.bytes, [&] {
    launch_gate_group(pl, g.p16.data(), packs, w_hwio, v3x, v3h, n, e->issue);
  }, g.dense, pl.mfma_factor);
}

void run_conv_group_f16x3(mv_engine* e, const std::vector<ConvLstmArgs>& probs) {
  const GatePrep g = prepare_gate_group(e, probs);
  const GatePrep* gp = &g;
  issue_gate_group(e, g, plan_gate_groups(e, &gp, 1));
}

// One launch for up to four independent ConvLSTM steps (class / regression
// chain of each scale advance in lockstep).
void run_conv_group(mv_engine* e, const std::vector<ConvLstmArgs>& probs) {
  if (probs.empty()) return;
  if (e->compute_mode != 0) {
    run_conv_group_f16x3(e, probs);
    return;
  }
  double flops = 0, bytes = 0, dense = 0;
  gate_group_cost(probs, flops, bytes, dense);
  for (const auto& a : probs) e->gate_rows += a.rows;
  if (e->cfg.convlstm_kernel != 3) {            // --convlstm_kernel 1 / 5 / ...: plain fp32 loops
    const double kk = (double)e->cfg.convlstm_kernel * e->cfg.convlstm_kernel / 9.0;
    launch(e, "convlstm_step", flops * kk, bytes, [&] {
      for (const auto& a : probs) {
        mv::ConvGenericArgs ga{};
        ga.f = a;
        ga.w = cell_of_bias(e, a.bias)->kernel->dev.p;
        ga.ksize = e->cfg.convlstm_kernel;
        mv::launch_convlstm_generic_step(ga, e->issue);
      }
    }, dense * kk, 0.0);
    return;
  }
  launch(e, "convlstm_step", flops, bytes, [&] {
    mv::launch_convlstm_steps(probs.data(), (int)probs.size(), e->issue);
  }, dense, 1.0);
}

// The gate launches of a step whose chains run as two pairs: group `a` (class chains) on the
// engine's stream, group `b` (regression chains) on the second one, each with its own group
// slots, both in the form planned for the step's problems together.
void run_conv_pairs(mv_engine* e, const std::vector<ConvLstmArgs>& a,
                    const std::vector<ConvLstmArgs>& b) {
  if (e->compute_mode == 0 || a.empty() || b.empty()) {
    { IssueOn on(e, 0); run_conv_group(e, a); }
    { IssueOn on(e, 1); run_conv_group(e, b); }
    return;
  }
  MV_REQUIRE(a.size() <= 2 && b.size() <= 2, "internal: chain pairs of %zu / %zu problems",
             a.size(), b.size());
  GatePrep ga, gb;
  { IssueOn on(e, 0); ga = prepare_gate_group(e, a); }
  { IssueOn on(e, 1); gb = prepare_gate_group(e, b); }
  // (the step's single launch dispatches the dense-x problems first: same order here; it
  // weights nothing but the profile's MFMA factor)
  const GatePrep* both[2] = {&gb, &ga};
  const ForwardPlan pl = plan_gate_groups(e, both, 2);
  { IssueOn on(e, 0); issue_gate_group(e, ga, pl); }
  { IssueOn on(e, 1); issue_gate_group(e, gb, pl); }
}

// One level of the scene stack in the form scene_conv_form (step_plan.h) chose; the forward, the
// training forward and mv_op_scene_conv launch through here.
static_assert(mv::kSceneTileCo == 64 && mv::kSceneTileCiMax == 64,
              "scene_conv_form states the tiled kernel's channel bounds");
void launch_scene_conv(hipStream_t stream, SceneConvForm form, const float* in, const float* w,
                       const float* b, float* out, int U, int Hi, int Wi, int Ci, int Ho, int Wo,
                       int Co, int k, int pad_t, int pad_l, int act) {
  const size_t M = (size_t)U * Ho * Wo;
  switch (form) {
    case SceneConvForm::Proj1x1:
      hipLaunchKernelGGL(mv::scene_proj1x1_mfma_kernel, dim3(cdiv(M, 128)), dim3(256), 0, stream,
                         in, w, b, out, U, Hi, Wi, Ci, Ho, Wo, Co, act);
      break;
    case SceneConvForm::Tiled:
      hipLaunchKernelGGL(mv::scene_conv3_s2_tiled_kernel, dim3(cdiv(M, mv::kSceneTilePix)),
                         dim3(256), 0, stream, in, w, b, out, U, Hi, Wi, Ci, Ho, Wo, pad_t, pad_l,
                         act);
      break;
    case SceneConvForm::PerOutput:
      hipLaunchKernelGGL(mv::scene_conv_s2_tanh_kernel, dim3(cdiv(M * Co, 256)), dim3(256), 0,
                         stream, in, w, b, out, U, Hi, Wi, Ci, Ho, Wo, Co, k, pad_t, pad_l, act);
      break;
  }
}

// mean_lens (the training step's per-row observation lengths, engine_train.h): the window of
// the scene mean when the forward's own obs plan is not in force
void run_scene(mv_engine* e, const int32_t* mean_lens = nullptr) {
  const mv_config& c = e->cfg;
  const int U = e->num_frames;
  const float* in = e->scene_feat.p;
  int Hi = c.scene_h, Wi = c.scene_w, Ci = c.scene_class;
  const int k = c.scene_conv_kernel;
  for (int i = 0; i < c.num_scales; ++i) {
    const int Ho = e->conv_h[i], Wo = e->conv_w[i], Co = c.scene_conv_dim;
    const int pad_h = std::max((Ho - 1) * 2 + k - Hi, 0);
    const int pad_w = std::max((Wo - 1) * 2 + k - Wi, 0);
    const size_t total = (size_t)U * Ho * Wo * Co;
    float* out = e->scene_conv[i].p;
    const float *w = e->scene_W[i]->dev.p, *b = e->scene_b[i]->dev.p;
    const SceneConvForm form = scene_conv_form(k, Ci, Co);
    if (form == SceneConvForm::Proj1x1) {     // --scene_conv_kernel 1: the dense 1x1 projection, on MFMA
      const size_t M = (size_t)U * Ho * Wo;
      launch(e, "scene_proj1x1_mfma", 2.0 * M * Ci * Co,
             4.0 * (total + (double)M * Ci), [&] {
        launch_scene_conv(e->issue, form, in, w, b, out, U, Hi, Wi, Ci, Ho, Wo, Co, k, 0, 0,
                          c.activation);
      });
    } else {
    launch(e, "scene_conv_s2_tanh", 2.0 * total * k * k * Ci,
           4.0 * (total + (double)U * Hi * Wi * Ci), [&] {
      launch_scene_conv(e->issue, form, in, w, b, out, U, Hi, Wi, Ci, Ho, Wo, Co, k, pad_h / 2,
                        pad_w / 2, c.activation);
    });
    }
    in = out; Hi = Ho; Wi = Wo; Ci = Co;
  }
  for (int s = 0; s < c.num_scales; ++s) {
    ScaleState& S = e->sc[s];
    if (!S.use) continue;
    const int rows = e->rows_at(0);      // ragged forward: the rows that decode at all
    const size_t total = (size_t)rows * S.K * c.scene_conv_dim;
    launch(e, "scene_mean", (double)total * c.obs_len,
           4.0 * total * (c.obs_len + 1), [&] {
      hipLaunchKernelGGL(mv::scene_mean_kernel, dim3(cdiv(total, 256)), dim3(256),
                         0, e->issue, e->scene_conv[s].p, e->obs_scene.p,
                         S.scene_mean.p, rows, c.obs_len, S.K,
                         c.scene_conv_dim,
                         mean_lens ? mean_lens
                                   : e->obs.ragged ? e->obs_lens_dev.p : (const int32_t*)nullptr);
    });
  }
}

struct Cursors {                 // which ping-pong buffer holds the live state
  int cls[MV_MAX_SCALES] = {0, 0};
  int reg[MV_MAX_SCALES] = {0, 0};
};

// Encoders of every enabled scale (dynamic_rnn from the zero state, T_o steps;
// code/pred_models.py:212-215, 232-234), all chains advanced in lockstep: step t's input
// launches (on e->issue) and gate problems for the chains in `chains`.
enum : int { kChainCls = 1, kChainReg = 2, kChainAll = 3 };

void encoder_step_problems(mv_engine* e, Cursors& cur, int t, int chains,
                           std::vector<ConvLstmArgs>& probs) {
  const mv_config& c = e->cfg;
  // N: the rows the step runs on (ragged forward: those that decode at all; obs-ragged forward:
  // the prefix that has started by step t); the sparse-x tables of the encoder keep the batch's
  // row layout
  const int N = e->enc_rows_at(t), Nb = c.batch_size, T = c.obs_len, D = c.scene_conv_dim;
  // obs-ragged forward: the first step that has rows takes the zero-state form; later steps
  // clear the state rows of the rows that join (one launch for the chains of this call)
  const int t0 = e->obs.ragged ? e->obs.first : 0;
  const int njoin = (e->obs.ragged && t > t0) ? e->obs_join_at[t + 1] - e->obs_join_at[t] : 0;
  mv::ZeroRowsArgs zr{};
  int nzr = 0, zrK = 0;
  auto join_rows = [&](float* cbuf, float* hbuf, int K) {
    if (!njoin) return;
    mv::ZeroRowsJob& j = zr.job[nzr++];
    j.c = cbuf; j.h = hbuf; j.K = K;
    zrK = std::max(zrK, K);
    auto it = e->planes.find(hbuf);
    if (e->compute_mode != 0 && it != e->planes.end()) {
      j.p0 = it->second.p;
      j.p1 = e->compute_mode == 2 ? nullptr : it->second.p + it->second.n;
    }
  };
  for (int s = 0; s < c.num_scales; ++s) {
    {
      ScaleState& S = e->sc[s];
      if (!S.use) continue;
      if (chains & kChainCls) {
      const size_t total = (size_t)N * S.K * D;
      const bool sparse = sparse_x_on(e, S);
      const size_t nc = (size_t)Nb * 9 * 4 * c.hidden_size;   // table of one step
      if (e->no_scene()) {
        // x = grid_emb(one_hot(labels[:, t])): table terms of the weights alone (built with
        // the decoder's, ensure_params), or the dense embedding of this step
        if (!sparse) {
          const int E = S.enc_cls.Cx;
          const size_t tx = (size_t)N * S.K * E;
          launch(e, "enc_grid_emb_onehot", (double)tx, 4.0 * tx, [&] {
            size_t pst = 0;
            _Float16* p16 = e->plane_out(S.xbuf_cls.p, &pst);
            hipLaunchKernelGGL(mv::enc_grid_emb_onehot_kernel, dim3(cdiv(tx, 256)), dim3(256),
                               0, e->issue, S.labels.p, T, t, 1, e->enc_emb_W->dev.p,
                               e->enc_emb_b->dev.p, S.xbuf_cls.p, N, S.H, S.W, E, p16, pst,
                               c.activation);
          });
        }
      } else if (sparse) {
        if (t == t0)     // the tables of all T_o steps in one launch
          launch(e, "sx_encoder_corr", 2.0 * nc * D * T, 4.0 * nc * T, [&] {
            hipLaunchKernelGGL(mv::sx_encoder_corr_kernel,
                               dim3(cdiv((size_t)4 * c.hidden_size, 256), 9,
                                    cdiv((size_t)Nb, mv::kSxRows) * T),
                               dim3(256), 0, e->issue, S.enc_cls.kernel->dev.p,
                               e->scene_conv[s].p, e->obs_scene.p, S.labels.p, Nb, T, -1, S.K, D,
                               c.hidden_size, S.sx_enc_corr.p);
          });
      } else {
      launch(e, "enc_class_input", 0, 4.0 * total, [&] {
        size_t pst = 0;
        _Float16* p16 = e->plane_out(S.xbuf_cls.p, &pst);
        hipLaunchKernelGGL(mv::enc_class_input_kernel, dim3(cdiv(total, 256)),
                           dim3(256), 0, e->issue, e->scene_conv[s].p,
                           e->obs_scene.p, S.labels.p, S.xbuf_cls.p, N, T, t, S.K, D, p16,
                           pst);
      });
      }
      const int cc = cur.cls[s];
      // light cone (gate_plan.h enc_cone_planned): one more row, the input-free background row
      const bool cone = sparse && enc_cone_on(e, S);
      probs.push_back(conv_problem(e, S.enc_cls, S.xbuf_cls.p, S.cls_h[cc].p,
                                   S.cls_c[cc].p, nullptr, nullptr, S.cls_h[cc ^ 1].p,
                                   S.cls_c[cc ^ 1].p, N + (cone ? 1 : 0), S.H, S.W, t == t0, 0,
                                   /*want_h16=*/t + 1 < T || !c.use_gnn));
      join_rows(S.cls_c[cc].p, S.cls_h[cc].p, S.K);
      if (cone) {
        // the first and the last step run every tile; a step reads the flags of the one before
        // it unless that one ran every tile
        ConvLstmArgs& a = probs.back();
        const size_t stride = enc_cone_step_elems(Nb + 1, S.H, S.W);
        const int ntile = enc_cone_tiles(Nb + 1, S.H, S.W);
        a.cone_on = 1;
        a.cone_list = (t > 0 && t + 1 < T) ? S.cone.p + (size_t)t * stride : nullptr;
        a.cone_prev = t > 1 ? S.cone.p + (size_t)(t - 1) * stride + 4 + ntile : nullptr;
        // (fits: conv_problem bounds rows * H * W * C by 2^31)
        MV_REQUIRE(S.cone_cells[t] > 0 && S.cone_cells[t] <= (int64_t)(N + 1) * S.H * S.W,
                   "internal: cone cell count %lld", (long long)S.cone_cells[t]);
        a.cone_cells = (int32_t)S.cone_cells[t];
      }
      // the class encoder's h' is read as fp32 only by the graph attention in front of the
      // first decoder step (and by the tiled-first-step A/B path of the beam decoder); the
      // regression encoder's never
      probs.back().skip_h32 =
          (t + 1 < T || (!c.use_gnn && (c.beam_size == 1 || step_knobs().beam_shared_first))) ? 1 : 0;
      if (sparse && e->no_scene()) {   // the decoder's by-class form, radius 2
        set_sparse_x(e, S, probs.back(), true, S.labels.p + t, T, 1);
        probs.back().sx_bias = S.sx_enc_bias.p;
        probs.back().sx_corr = S.sx_enc_tab.p;
      } else if (sparse) {
        set_sparse_x(e, S, probs.back(), false, S.labels.p + t, T, 1);
        probs.back().sx_corr = S.sx_enc_corr.p + (size_t)t * nc;
      }
      cur.cls[s] ^= 1;
      }
      if (!(chains & kChainReg)) continue;
      // x = grid_obs_regress[:, t] is read in place through the row stride
      const size_t row = (size_t)S.K * 2;
      const int cr = cur.reg[s];
      if (!c.use_single_decoder) {   // single decoder: the regression encoder feeds nothing
        probs.push_back(conv_problem(e, S.enc_reg, S.obs_reg.p + (size_t)t * row,
                                     S.reg_h[cr].p, S.reg_c[cr].p, nullptr, nullptr,
                                     S.reg_h[cr ^ 1].p, S.reg_c[cr ^ 1].p, N, S.H, S.W,
                                     t == t0, (size_t)T * row));
        join_rows(S.reg_c[cr].p, S.reg_h[cr].p, S.K);
      }
      if (!c.use_single_decoder) probs.back().skip_h32 = 1;
      cur.reg[s] ^= 1;
    }
  }
  if (nzr) {
    zr.rows = e->obs_join_rows.p + e->obs_join_at[t];
    zr.nrows = njoin; zr.C = c.hidden_size;
    const size_t total = (size_t)njoin * zrK * (c.hidden_size / 8);    // 8 channels per thread
    launch(e, "enc_join_zero", 0, (double)nzr * total * 8 * 12.0, [&] {
      hipLaunchKernelGGL(mv::zero_state_rows_kernel, dim3(cdiv(total, 256), nzr), dim3(256), 0,
                         e->issue, zr);
    });
  }
}

void run_encoders(mv_engine* e, Cursors& cur, bool pairs) {
  // (obs-ragged forward: a step no row has reached is not launched and moves no cursor; every
  // row ends in the buffer the last step writes, which the decoders find through `cur`)
  for (int t = e->obs.ragged ? e->obs.first : 0; t < e->cfg.obs_len; ++t) {
    if (!pairs) {
      std::vector<ConvLstmArgs> probs;
      encoder_step_problems(e, cur, t, kChainAll, probs);
      run_conv_group(e, probs);
      continue;
    }
    std::vector<ConvLstmArgs> pa, pb;
    { IssueOn on(e, 0); encoder_step_problems(e, cur, t, kChainCls, pa); }
    { IssueOn on(e, 1); encoder_step_problems(e, cur, t, kChainReg, pb); }
    run_conv_pairs(e, pa, pb);
  }
}

// One attention launch in the form step_plan.h's gnn_form chose: the one or (tiled forms) two
// problems of `group`, whose block counts are filled in here.  PerCell carries one problem.
void launch_gnn(hipStream_t stream, GnnForm form, const mv::GnnGroup& group, int njobs, int C,
                int D) {
  if (form == GnnForm::PerCell) {
    MV_REQUIRE(njobs == 1, "internal: the per-cell attention carries one job per launch");
    const mv::GnnProblem& P = group.p[0];
    const size_t cells = (size_t)P.M * P.H * P.W;
    if (C <= 256)
      hipLaunchKernelGGL(mv::gnn_attend_kernel<1>, dim3(cdiv(cells, 4)), dim3(256), 0, stream,
                         P.h, P.scene_mean, P.src_row, P.out, P.M, P.H, P.W, C, D, P.sm_div,
                         P.p16, P.p16_stride);
    else
      hipLaunchKernelGGL(mv::gnn_attend_kernel<2>, dim3(cdiv(cells, 4)), dim3(256), 0, stream,
                         P.h, P.scene_mean, P.src_row, P.out, P.M, P.H, P.W, C, D, P.sm_div,
                         P.p16, P.p16_stride);
    return;
  }
  mv::GnnGroup grp = group;
  unsigned nblocks = 0;
  for (int j = 0; j < njobs; ++j) {
    mv::GnnProblem& P = grp.p[j];
    const size_t cells = (size_t)P.M * P.H * P.W;
    const unsigned nb = form == GnnForm::Blocked ? mv::gnn_v3_blocks(cells, &P.ngroups)
                                                 : mv::gnn_v2_blocks(cells, &P.ngroups);
    if (j == 0) grp.nblocks0 = nb;
    nblocks += nb;
  }
  if (form == GnnForm::Blocked)
    hipLaunchKernelGGL(mv::gnn_attend_v3_kernel, dim3(nblocks), dim3(mv::kGnn3Threads), 0, stream,
                       grp, C, D);
  else
    hipLaunchKernelGGL(mv::gnn_attend_v2_kernel, dim3(nblocks), dim3(mv::kGnnThreads), 0, stream,
                       grp, C, D);
}

// One attention pass per job; the tiled forms take up to two jobs per launch (the two grid
// scales of a greedy step are 62 + 22 us back to back, one round of workgroups each: together
// they fill the chip better).  The form: step_plan.h gnn_form, the weaker of a pair's two.
struct GnnJob {
  ScaleState* S; const float* h; const int32_t* src_row; float* out; int rows, sm_div;
  const int32_t* row_ref = nullptr;
};

void run_gnn_jobs(mv_engine* e, const std::vector<GnnJob>& jobs) {
  const mv_config& c = e->cfg;
  const int C = c.hidden_size, D = gnn_scene_dim(e);
  // The kernels see D = gnn_scene_dim channels; a model of more than 64 scene channels keeps the
  // per-cell form even where its attention reads none of them (SimAug's greedy graph).
  const int D_form = c.scene_conv_dim > 64 ? c.scene_conv_dim : D;
  // worst case of the engine, not this step's rows: one form per scale
  const size_t max_rows = (size_t)c.batch_size * (size_t)std::max(1, c.beam_size);
  auto form_of = [&](const GnnJob& J) {
    return gnn_form(0, J.S->W, C, D_form, max_rows * J.S->K * C * 4);
  };
  for (size_t j0 = 0; j0 < jobs.size();) {
    GnnForm form = form_of(jobs[j0]);
    size_t nj = 1;
    if (form != GnnForm::PerCell && j0 + 1 < jobs.size() &&
        form_of(jobs[j0 + 1]) != GnnForm::PerCell) {
      nj = 2;
      form = weaker(form, form_of(jobs[j0 + 1]));
    }
    const bool tiled = form != GnnForm::PerCell;
    mv::GnnGroup grp{};
    double flops = 0, bytes = 0;
    for (size_t j = 0; j < nj; ++j) {
      const GnnJob& J = jobs[j0 + j];
      const size_t cells = (size_t)J.rows * J.S->K;
      size_t pst = 0;
      _Float16* p16 = e->plane_out(J.out, &pst);
      // f16x3 inference: the only consumer of h + GNN(h) is the gate convolution, which
      // reads the operand planes -- the fp32 copy is not written at all
      const bool need_f32 = !(tiled && p16 && !e->train && e->compute_mode != 0);
      flops += cells * (9.0 * 2 * 2 * (C + D) + 9.0 * 2 * C);
      bytes += 4.0 * cells * C * (1.0 + (need_f32 ? 1.0 : 0.0) + (p16 ? 1.0 : 0.0)) +
               4.0 * (cells / J.sm_div) * D;
      mv::GnnProblem& P = grp.p[j];
      P.h = J.h; P.scene_mean = J.S->scene_mean.p; P.src_row = J.src_row;
      P.out = need_f32 ? J.out : nullptr; P.p16 = p16; P.p16_stride = pst;
      P.M = J.rows; P.H = J.S->H; P.W = J.S->W; P.sm_div = J.sm_div;
      P.row_ref = J.row_ref;
    }
    launch(e, "gnn_attend", flops, bytes, [&] {
      launch_gnn(e->issue, form, grp, (int)nj, C, D);
    });
    j0 += nj;
  }
}

void run_gnn(mv_engine* e, ScaleState& S, const float* h, const int32_t* src_row,
             float* out, int rows, int sm_div) {
  run_gnn_jobs(e, {GnnJob{&S, h, src_row, out, rows, sm_div}});
}

template <int P>
void run_hidden2grid(mv_engine* e, ScaleState& S, const float* h, const float* w,
                     float* out, size_t out_row_stride, int rows) {
  const size_t cells = (size_t)rows * S.K;
  const int C = e->cfg.hidden_size;
  launch(e, "hidden2grid", cells * 2.0 * 9 * C * P, 4.0 * cells * (C + P), [&] {
    hipLaunchKernelGGL(mv::hidden2grid_kernel<P>, dim3(cdiv(cells, 4)), dim3(256),
                       0, e->issue, h, w, out, out_row_stride, rows, S.H, S.W, C);
  });
}

// Does this engine's forward take the grouped decoder tail (step_plan.h tail_form)?
bool tail_grouped(const mv_engine* e, bool training = false) {
  int Kmax = 0;
  for (int s = 0; s < e->cfg.num_scales; ++s)
    if (e->sc[s].use) Kmax = std::max(Kmax, e->sc[s].K);
  return tail_form(training, e->cfg.emb_size, Kmax) == TailForm::Grouped;
}

void run_emb_onehot(mv_engine* e, ScaleState& S, const int32_t* ids, int stride,
                    float* out, int rows, int ids_div = 1) {
  const int E = e->cfg.emb_size;
  const size_t total = (size_t)rows * S.K * E;
  launch(e, "grid_emb_onehot", (double)total, 4.0 * total, [&] {
    size_t pst = 0;
    _Float16* p16 = e->plane_out(out, &pst);
    if (step_knobs().tail_grouped && E % 8 == 0)   // (the 8-channel form came with that tail)
      hipLaunchKernelGGL(mv::grid_emb_onehot8_kernel, dim3(cdiv(total / 8, 256)), dim3(256), 0,
                         e->issue, ids, stride, ids_div, S.emb_cls_W->dev.p,
                         S.emb_cls_b->dev.p, out, rows, S.H, S.W, E, p16, pst, e->cfg.activation);
    else
      hipLaunchKernelGGL(mv::grid_emb_onehot_kernel, dim3(cdiv(total, 256)),
                         dim3(256), 0, e->issue, ids, stride, ids_div, S.emb_cls_W->dev.p,
                         S.emb_cls_b->dev.p, out, rows, S.H, S.W, E, p16, pst, e->cfg.activation);
  });
}

// grid_emb on a dense P-channel map: the regression decoder's (dx, dy) maps (default
// weights), or -- class decoder fed its own logits / the ground-truth map (training
// without --train_w_onehot, teacher forcing) -- a 1-channel map with the class weights
void run_emb_dense(mv_engine* e, ScaleState& S, const float* x, size_t row_stride,
                   float* out, int rows, Param* W = nullptr, Param* b = nullptr, int P = 2) {
  const int E = e->cfg.emb_size;
  const size_t total = (size_t)rows * S.K * E;
  if (!W) { W = S.emb_reg_W; b = S.emb_reg_b; }
  launch(e, "grid_emb_dense", total * 2.0 * 9 * P, 4.0 * total, [&] {
    size_t pst = 0;
    _Float16* p16 = e->plane_out(out, &pst);
    hipLaunchKernelGGL(mv::grid_emb_dense_kernel, dim3(cdiv(total, 256)), dim3(256),
                       0, e->issue, x, row_stride, W->dev.p, b->dev.p, out, rows, S.H, S.W,
                       P, E, p16, pst, e->cfg.activation);
  });
}

// Regression decoder step t, always greedy and un-beamed
// (code/pred_models.py:298-305 -> grid_decoder :311-471 with input_onehot=False,
// use_gnn=False): input embedding + the conv problem; the caller launches it.
ConvLstmArgs reg_decoder_problem(mv_engine* e, int s, Cursors& cur, int t, int Tp,
                                 bool embed = true) {
  const mv_config& c = e->cfg;
  ScaleState& S = e->sc[s];
  const int N = e->rows_at(t), T = c.obs_len;
  const size_t orow = (size_t)Tp * S.K * 2;
  if (t == 0)  // first_input = obs_grid_reg[:, -1]
    run_emb_dense(e, S, S.obs_reg.p + (size_t)(T - 1) * S.K * 2, (size_t)T * S.K * 2,
                  S.xbuf_reg.p, N);
  else if (embed)   // hidden2grid output of the previous step (else: the tail embedded it)
    run_emb_dense(e, S, S.out_reg.p + (size_t)(t - 1) * S.K * 2, orow, S.xbuf_reg.p, N);
  const int cr = cur.reg[s];
  cur.reg[s] ^= 1;
  return conv_problem(e, S.dec_reg, S.xbuf_reg.p, S.reg_h[cr].p, S.reg_c[cr].p, nullptr,
                      nullptr, S.reg_h[cr ^ 1].p, S.reg_c[cr ^ 1].p, N, S.H, S.W, false);
}

void reg_decoder_output(mv_engine* e, int s, const Cursors& cur, int t, int Tp) {
  ScaleState& S = e->sc[s];
  const size_t orow = (size_t)Tp * S.K * 2;
  run_hidden2grid<2>(e, S, S.reg_h[cur.reg[s]].p, S.out_reg_W->dev.p,
                     S.out_reg.p + (size_t)t * S.K * 2, orow, e->rows_at(t));
}

// The decoder tail of step t for all chains (decode_tail.h): hidden2grid as one
// grouped GEMM launch reading every h' once, then one workgroup per (chain, row) for
// the 9-tap gather, the output row, the greedy argmax and the NEXT step's embedding.
// cls_rows / cls_out / cls_stride describe the class chain's logits destination
// (greedy: out_cls step t; beam: bm_logits of this time step, no argmax / embedding).
struct TailPlan {
  int s;
  const float* cls_h; int cls_rows; float* cls_out; int64_t cls_stride;
  bool cls_next;       // class chain: argmax + embedding of step t+1 (greedy only)
  const float* reg_h; float* reg_out; int64_t reg_stride; bool reg_next;
  int reg_rows = 0;    // 0: N (the un-beamed regression chain)
  // training forward: where the argmax ids and the next step's embeddings go (null: the
  // inference buffers S.ids / S.xbuf_cls / S.xbuf_reg with their operand planes)
  int32_t* cls_ids_out = nullptr; float* cls_x_out = nullptr; float* reg_x_out = nullptr;
  bool cls_embed = true;   // false: ids only (the embedding is made elsewhere)
  // the chains of this scale that the launch carries (the chain pairs of the greedy forward
  // run the class chains' tail and the regression chains' tail as launches of their own)
  bool do_cls = true, do_reg = true;
};

// What every filler of a grouped tail launch (run_tail, mv_op_decode_tail) sets: the refusal of a
// shape the tail does not fit, a chain's problem without a next step, and the next step's
// embedding with its operand planes (x16 null: none; pst 0 with x16: the single bf16 plane).
void require_tail_fits(int E, int K) {
  MV_REQUIRE(tail_grouped_fits(E, K), "decode tail: K %d / emb_size %d", K, E);
}
mv::TailProblem tail_problem(const float* q, float* out, int64_t out_row_stride, int rows, int H,
                             int W, bool cls, int E, int act) {
  mv::TailProblem a{};
  a.q = q; a.out = out; a.out_row_stride = out_row_stride;
  a.rows = rows; a.H = H; a.W = W; a.P = cls ? 1 : 2; a.E = E; a.onehot = cls ? 1 : 0;
  a.act = act;
  return a;
}
void tail_embed(mv::TailProblem& a, const float* emb_w, const float* emb_b, float* x_out,
                _Float16* x16 = nullptr, size_t pst = 0) {
  a.emb_w = emb_w; a.emb_b = emb_b;
  a.x_out = x_out;
  a.x16 = x16; a.x16_stride = (int64_t)pst;
}

void run_tail(mv_engine* e, const std::vector<TailPlan>& plans) {
  const mv_config& c = e->cfg;
  const int C = c.hidden_size, E = c.emb_size, N = c.batch_size;
  std::vector<mv::H2gQProblem> qp;
  std::vector<mv::TailProblem> tp;
  double qbytes = 0, qflops = 0, tbytes = 0;
  for (const TailPlan& pl : plans) {
    ScaleState& S = e->sc[pl.s];
    require_tail_fits(E, S.K);
    const int reg_rows = pl.reg_rows ? pl.reg_rows : N;
    const size_t cc = (size_t)pl.cls_rows * S.K, cr = (size_t)reg_rows * S.K;
    if (pl.do_cls) {
      qp.push_back(mv::H2gQProblem{pl.cls_h, S.wq_cls.p, S.q_cls.p, (int32_t)cc, 1});
      qbytes += 4.0 * cc * (C + 9.0);
      qflops += 2.0 * 9 * C * cc;
    }
    if (pl.do_reg) {
      qp.push_back(mv::H2gQProblem{pl.reg_h, S.wq_reg.p, S.q_reg.p, (int32_t)cr, 2});
      qbytes += 4.0 * cr * (C + 18.0);
      qflops += 2.0 * 9 * C * 2.0 * cr;
    }
    if (pl.do_cls) {
      mv::TailProblem a = tail_problem(S.q_cls.p, pl.cls_out, pl.cls_stride, pl.cls_rows, S.H, S.W,
                                       true, E, c.activation);
      tbytes += 4.0 * cc * (9 + 1);
      if (pl.cls_next) {
        a.ids_out = pl.cls_ids_out ? pl.cls_ids_out : S.ids.p;
        if (pl.cls_x_out) {           // training: fp32 embedding into the time-major x buffer
          if (pl.cls_embed) {
            tail_embed(a, S.emb_cls_W->dev.p, S.emb_cls_b->dev.p, pl.cls_x_out);
            tbytes += 4.0 * cc * E;
          }
        } else if (!sparse_x_on(e, S)) {     // sparse x: the next step needs the id, not the embedding
          size_t pst = 0;
          _Float16* x16 = e->plane_out(S.xbuf_cls.p, &pst);
          tail_embed(a, S.emb_cls_W->dev.p, S.emb_cls_b->dev.p, S.xbuf_cls.p, x16, pst);
          tbytes += 4.0 * cc * E * (a.x16 ? 2 : 1);
        }
      }
      tp.push_back(a);
    }
    if (!pl.do_reg) continue;
    mv::TailProblem b = tail_problem(S.q_reg.p, pl.reg_out, pl.reg_stride, reg_rows, S.H, S.W,
                                     false, E, c.activation);
    tbytes += 4.0 * cr * (18 + 2);
    if (pl.reg_next) {
      if (pl.reg_x_out) {
        tail_embed(b, S.emb_reg_W->dev.p, S.emb_reg_b->dev.p, pl.reg_x_out);
        tbytes += 4.0 * cr * E;
      } else {
        size_t pst = 0;
        _Float16* x16 = e->plane_out(S.xbuf_reg.p, &pst);
        tail_embed(b, S.emb_reg_W->dev.p, S.emb_reg_b->dev.p, S.xbuf_reg.p, x16, pst);
        tbytes += 4.0 * cr * E * (b.x16 ? 2 : 1);
      }
    }
    tp.push_back(b);
  }
  MV_REQUIRE(qp.size() <= (size_t)mv::kTailMax, "decode tail: too many chains");
  if (qp.empty()) return;
  launch(e, "hidden2grid", qflops, qbytes, [&] {
    mv::launch_h2g_q(qp.data(), (int)qp.size(), C, e->issue);
  });
  launch(e, "decode_tail", 0, tbytes, [&] {
    mv::launch_decode_tail(tp.data(), (int)tp.size(), e->issue);
  });
}

// The un-beamed regression chain's part of step t's tail: offsets into out_reg step t, and the
// embedding of step t + 1.
void tail_reg_chain(const ScaleState& S, const Cursors& cur, int s, int t, int Tp, int rows,
                    TailPlan& pl) {
  pl.reg_h = S.reg_h[cur.reg[s]].p;
  pl.reg_out = S.out_reg.p + (size_t)t * S.K * 2; pl.reg_stride = (int64_t)Tp * S.K * 2;
  pl.reg_next = t + 1 < Tp;
  pl.reg_rows = rows;
}

// The class decoder's gate problem of cell step `time` >= 1 of a beam-handle forward (beam search,
// sampled, scored) and the cursor flip: h from the attention buffer when use_gnn, the state rows
// through src_h / src_c.  Sparse x: the one-hot input enters as table terms -- at the first step
// the last observed cell (first_div rows share a sample's label), afterwards the previous step's
// ids, row r's at prev_ids[r * prev_stride].
ConvLstmArgs beam_cls_problem(mv_engine* e, int s, Cursors& cur, int time, int rows,
                              const int32_t* src_h, const int32_t* src_c, int first_div,
                              const int32_t* prev_ids, int prev_stride) {
  const mv_config& c = e->cfg;
  ScaleState& S = e->sc[s];
  const int cc = cur.cls[s], T = c.obs_len;
  const float* hin = c.use_gnn ? S.cls_hg.p : S.cls_h[cc].p;
  ConvLstmArgs a = conv_problem(e, S.dec_cls, S.xbuf_cls.p, hin, S.cls_c[cc].p, src_h, src_c,
                                S.cls_h[cc ^ 1].p, S.cls_c[cc ^ 1].p, rows, S.H, S.W, false, 0,
                                /*want_h16=*/!c.use_gnn);
  if (sparse_x_on(e, S)) {
    if (time == 1) set_sparse_x(e, S, a, true, S.labels.p + (T - 1), T, first_div);
    else set_sparse_x(e, S, a, true, prev_ids, prev_stride, 1);
  }
  cur.cls[s] ^= 1;
  return a;
}

// Greedy decoders of every enabled scale in lockstep: class decoder
// (grid_decoder with input_onehot, use_gnn; code/pred_models.py:311-471) and
// regression decoder.  `pairs`: the class chains and the regression chains are issued as two
// chain pairs (enqueue_forward) instead of sharing every launch.
void run_decoders_greedy(mv_engine* e, Cursors& cur, int Tp, bool pairs) {
  const mv_config& c = e->cfg;
  const int T = c.obs_len;
  const bool v2 = tail_grouped(e);
  MV_REQUIRE(!pairs || (v2 && !c.use_single_decoder), "internal: chain pairs need the grouped "
             "decoder tail and a regression decoder");
  // ragged forward: max L steps, step t on the rows_at(t) rows of its active prefix
  const int Tsteps = e->len.ragged ? e->len.steps : Tp;
  for (int t = 0; t < Tsteps; ++t) {
    const int N = e->rows_at(t);
    // input launches (on e->issue) and gate problems of step t for the chains in `chains`
    auto step_problems = [&](int chains, std::vector<ConvLstmArgs>& probs) {
      if ((chains & kChainCls) && c.use_gnn) {
        std::vector<GnnJob> jobs;
        for (int s = 0; s < c.num_scales; ++s)
          if (e->sc[s].use)
            jobs.push_back(GnnJob{&e->sc[s], e->sc[s].cls_h[cur.cls[s]].p, nullptr,
                                  e->sc[s].cls_hg.p, N, 1});
        run_gnn_jobs(e, jobs);
      }
      for (int s = 0; s < c.num_scales; ++s) {
        ScaleState& S = e->sc[s];
        if (!S.use) continue;
        if (chains & kChainCls) {
          const int cc = cur.cls[s];
          const float* hin = c.use_gnn ? S.cls_hg.p : S.cls_h[cc].p;
          // sparse x: the embedding of a one-hot map enters the gate kernel as table terms
          const bool sparse = sparse_x_on(e, S) && (t == 0 || !c.class_feedback_dense);
          if (sparse)
            ;
          else if (t == 0)  // one_hot(last observed cell)
            run_emb_onehot(e, S, S.labels.p + (T - 1), T, S.xbuf_cls.p, N);
          else if (c.class_feedback_dense)   // raw logits of the previous step (:388-406)
            run_emb_dense(e, S, S.out_cls.p + (size_t)(t - 1) * S.K, (size_t)Tp * S.K,
                          S.xbuf_cls.p, N, S.emb_cls_W, S.emb_cls_b, 1);
          else if (!v2)
            run_emb_onehot(e, S, S.ids.p, 1, S.xbuf_cls.p, N);
          probs.push_back(conv_problem(e, S.dec_cls, S.xbuf_cls.p, hin, S.cls_c[cc].p,
                                       nullptr, nullptr, S.cls_h[cc ^ 1].p,
                                       S.cls_c[cc ^ 1].p, N, S.H, S.W, false, 0,
                                       /*want_h16=*/!c.use_gnn));
          if (sparse) {
            if (t == 0) set_sparse_x(e, S, probs.back(), true, S.labels.p + (T - 1), T, 1);
            else set_sparse_x(e, S, probs.back(), true, S.ids.p, 1, 1);
          }
          cur.cls[s] ^= 1;
        }
        if ((chains & kChainReg) && !c.use_single_decoder)
          probs.push_back(reg_decoder_problem(e, s, cur, t, Tp, !v2));
      }
      // longest tiles first: the dense-x problems (162 k-steps per tile) are dispatched
      // before the sparse-x ones (144), so the last, partly filled round of workgroups is
      // made of the short ones
      std::stable_sort(probs.begin(), probs.end(), [](const ConvLstmArgs& a, const ConvLstmArgs& b) {
        return (a.sx_corr == nullptr) > (b.sx_corr == nullptr);
      });
    };
    // the grouped decoder tail of step t for the chains in `chains`
    auto step_tail = [&](int chains) {
      std::vector<TailPlan> plans;
      for (int s = 0; s < c.num_scales; ++s) {
        ScaleState& S = e->sc[s];
        if (!S.use) continue;
        TailPlan pl{};
        pl.s = s;
        pl.cls_h = S.cls_h[cur.cls[s]].p; pl.cls_rows = N;
        pl.cls_out = S.out_cls.p + (size_t)t * S.K; pl.cls_stride = (int64_t)Tp * S.K;
        pl.cls_next = t + 1 < Tp && !c.class_feedback_dense;
        tail_reg_chain(S, cur, s, t, Tp, N, pl);
        if (c.use_single_decoder) {    // offsets from the class decoder's state (:287-296)
          pl.reg_h = pl.cls_h;
          pl.reg_next = false;
        }
        pl.do_cls = (chains & kChainCls) != 0;
        pl.do_reg = (chains & kChainReg) != 0;
        plans.push_back(pl);
      }
      run_tail(e, plans);
    };
    if (pairs) {
      std::vector<ConvLstmArgs> pa, pb;
      { IssueOn on(e, 0); step_problems(kChainCls, pa); }
      { IssueOn on(e, 1); step_problems(kChainReg, pb); }
      run_conv_pairs(e, pa, pb);
      { IssueOn on(e, 0); step_tail(kChainCls); }
      { IssueOn on(e, 1); step_tail(kChainReg); }
      continue;
    }
    std::vector<ConvLstmArgs> probs;
    step_problems(kChainAll, probs);
    run_conv_group(e, probs);
    if (v2) {
      step_tail(kChainAll);
      continue;
    }
    for (int s = 0; s < c.num_scales; ++s) {
      ScaleState& S = e->sc[s];
      if (!S.use) continue;
      const size_t orow = (size_t)Tp * S.K;
      float* logits = S.out_cls.p + (size_t)t * S.K;
      run_hidden2grid<1>(e, S, S.cls_h[cur.cls[s]].p, S.out_cls_W->dev.p, logits, orow, N);
      if (t + 1 < Tp && !c.class_feedback_dense) {
        launch(e, "argmax_rows", 0, 4.0 * N * S.K, [&] {
          hipLaunchKernelGGL(mv::argmax_rows_kernel, dim3(N), dim3(64), 0, e->issue,
                             logits, orow, S.ids.p, N, S.K);
        });
      }
      if (c.use_single_decoder)
        run_hidden2grid<2>(e, S, S.cls_h[cur.cls[s]].p, S.out_reg_W->dev.p,
                           S.out_reg.p + (size_t)t * S.K * 2, (size_t)Tp * S.K * 2, N);
      else
        reg_decoder_output(e, s, cur, t, Tp);
    }
  }
}

__global__ void tile_rows_kernel(const float* __restrict__ in, float* __restrict__ out,
                                 size_t row_elems4, int B, size_t total4) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total4) return;
  const size_t r = idx / row_elems4, off = idx - r * row_elems4;
  reinterpret_cast<mv::f32x4_t*>(out)[idx] =
      reinterpret_cast<const mv::f32x4_t*>(in)[(r / B) * row_elems4 + off];
}

// logits[(n*B + b), :] = logits[(n*B), :] for b > 0 (the shared first beam step)
__global__ void tile_beam0_kernel(float* __restrict__ logits, int K, int B, size_t total) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const size_t r = idx / K;
  if (r % B) logits[idx] = logits[(r - r % B) * K + (idx - r * K)];
}

// Back-trace (:689-806) of row n's beams from step L[n] - 1 with parents_0 = arange(B)
// (code/pred_models.py:714-716), as a forward of pred_len L[n] does; from step L[n] on the ids and
// the trace are -1 (nothing to gather).  lens == NULL (no per-row lengths): L[n] = T.
__global__ void beam_backtrace_kernel(const int32_t* __restrict__ step_ids,
                                      const int32_t* __restrict__ step_parents,
                                      const int32_t* __restrict__ lens,
                                      int32_t* __restrict__ out_ids,
                                      int32_t* __restrict__ trace, int N, int B, int T) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= N * B) return;
  const int n = idx / B, b = idx - n * B;
  const int L = lens ? min(max(lens[n], 0), T) : T;
  const size_t row = ((size_t)n * B + b) * T;
  for (int t = T - 1; t >= L; --t) { out_ids[row + t] = -1; trace[row + t] = -1; }
  int par = b;
  for (int t = L - 1; t >= 0; --t) {
    const size_t o = ((size_t)t * N + n) * B + par;
    out_ids[row + t] = step_ids[o];
    trace[row + t] = par;
    par = step_parents[o];
  }
}

// out[n, b, t, :] = step_vals[t, n, trace[n, b, t], :], exact zeros where the trace is -1 (steps
// past L[n]; a back-trace without lengths leaves none)
__global__ void beam_gather_kernel(const float* __restrict__ step_vals,
                                   const int32_t* __restrict__ trace,
                                   float* __restrict__ out, int N, int B, int T, int K) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)N * B * T * K;
  if (idx >= total) return;
  const int k = idx % K;
  size_t r = idx / K;
  const int t = r % T; r /= T;
  const int b = r % B;
  const int n = r / B;
  const int par = trace[((size_t)n * B + b) * T + t];
  out[idx] = par < 0 ? 0.f : step_vals[(((size_t)t * N + n) * B + par) * K + k];
}

// ---- finalisers of a ragged forward (per-row lengths `lens`, mv_set_pred_lengths)

// final[n, :] = lp[n, :] for the rows whose last selection was this one (L[n] == time)
__global__ void ragged_capture_lp_kernel(const float* __restrict__ lp,
                                         const int32_t* __restrict__ lens,
                                         float* __restrict__ final_lp, int rows, int B, int time) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= rows) return;
  if (lens[idx / B] == time) final_lp[idx] = lp[idx];
}

// out[n, t, :] = 0 for t >= L[n]: what raw_rnn emits for a finished row, through the bias-free
// hidden2grid.  out is [N, T, row_elems]; one thread per element.
// (N rows that share a length in groups of `per_len`: the S futures of a sampled row)
__global__ void ragged_zero_tail_kernel(float* __restrict__ out, const int32_t* __restrict__ lens,
                                        int N, int T, int row_elems, int per_len = 1) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)N * T * row_elems) return;
  const size_t r = idx / row_elems;
  const int t = r % T, n = r / T;
  if (t >= lens[n / per_len]) out[idx] = 0.f;
}

// ids[r, t] = -1 for t >= L[r / S] (sampled forward: the ids are written in place, step by step)
__global__ void ragged_ids_tail_kernel(int32_t* __restrict__ ids, const int32_t* __restrict__ lens,
                                       int R, int S, int T) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= R * T) return;
  if (idx % T >= lens[idx / T / S]) ids[idx] = -1;
}

// What constrains decode step t (StepTerms, engine_setup.h), from what is set on the engine;
// nothing set: the empty StepTerms, and the step launches exactly what it launched before.
//   mask, bias  plane t of every row, or the one plane.
//   motion      the tables, and where the step kernels find each row's p1 / p0 in what the
//               forward already holds on the device -- the labels for the observed cells, and the
//               ids (and, for the beams, the parents) the earlier steps wrote.
//   revisit     the cost, the half of the engine's set buffer that holds every row's visited set
//               of step t - 1 and the half step t stores into, and where the row's p1 lies.  At
//               t == 0 there is no set yet: the kernel starts from the row's observed cells
//               (seed_observed) or from nothing, and p1 -- the last observed cell -- joins the
//               set only as one of those.
// No launch and no buffer is added.  `ids` [.., R] x ids_stride: the chosen cell of row r at step
// u is ids[u * ids_step + r * ids_stride]; parents (beam, wor): [T, R], or NULL for rows that
// continue themselves.
StepTerms step_terms(const mv_engine* e, const ScaleState& S, int t, const int32_t* ids,
                     size_t ids_step, int ids_stride, const int32_t* parents) {
  const StepConstraints& con = e->con;
  const int T = e->cfg.obs_len, K = S.K, Tcap = e->cfg.max_pred_len;
  const size_t N = (size_t)e->cfg.batch_size, R = N * e->cfg.beam_size;
  const int32_t* last = S.labels.p + (T - 1);      // labels[:, -1], one per sample
  StepTerms m;
  if (con.mask.set()) {
    m.amask = con.mask.at(K, t);
    m.mask_stride = con.mask.stride(K, Tcap);
  }
  if (con.bias.set()) {
    m.bias = con.bias.at(K, t);
    m.bias_stride = con.bias.stride(K, Tcap);
  }
  if (con.motion_set()) {
    mv::MotionRow& mo = m.mo;
    const float* d = con.motion_dev.p;
    mo.vel = d;
    mo.vel_far = d + StepConstraints::motion_vel_far_at(N);
    mo.acc = con.motion_acc ? d + StepConstraints::motion_acc_at(N) : nullptr;
    mo.acc_far = con.motion_acc ? d + StepConstraints::motion_acc_far_at(N) : nullptr;
    mo.W = S.W;
    mo.radius = con.motion_radius;
    if (t == 0) {
      mo.prev1 = last; mo.p1_stride = T; mo.p1_per_row = 0;
      mo.prev0 = T >= 2 ? last - 1 : nullptr; mo.p0_stride = T; mo.p0_per_row = 0;
      // a row observed for one frame has no cell before its last (right-aligned observations)
      mo.obs_lens = e->obs.ragged ? e->obs_lens_dev.p : nullptr;
    } else {
      mo.prev1 = ids + (size_t)(t - 1) * ids_step; mo.p1_stride = ids_stride; mo.p1_per_row = 1;
      if (t == 1) {
        mo.prev0 = last; mo.p0_stride = T; mo.p0_per_row = 0;
      } else {
        mo.prev0 = ids + (size_t)(t - 2) * ids_step; mo.p0_stride = ids_stride; mo.p0_per_row = 1;
        mo.prev0_via = parents ? parents + (size_t)(t - 1) * R : nullptr;
      }
    }
  }
  if (con.revisit_set()) {
    mv::RevisitRow& rv = m.rv;
    const size_t words = StepConstraints::revisit_set_words(R);
    rv.cost = con.revisit_dev.p;
    rv.set_out = con.revisit_sets.p + (size_t)(t & 1) * words;
    if (t == 0) {
      rv.prev1 = last; rv.p1_stride = T; rv.p1_per_row = 0;
      rv.or_p1 = 0;
      if (con.revisit_seed) {
        rv.seed = S.labels.p;
        rv.seed_T = T;
        // the columns in front of a short track are not read (right-aligned observations)
        rv.obs_lens = e->obs.ragged ? e->obs_lens_dev.p : nullptr;
      }
    } else {
      rv.set_in = con.revisit_sets.p + (size_t)((t - 1) & 1) * words;
      rv.via = parents ? parents + (size_t)(t - 1) * R : nullptr;
      rv.prev1 = ids + (size_t)(t - 1) * ids_step; rv.p1_stride = ids_stride; rv.p1_per_row = 1;
    }
  }
  return m;
}

// Beam-search class decoder (grid_decoder_beam_search,
// code/pred_models.py:474-806) with the un-beamed regression decoder advanced
// in lockstep (its step t shares a launch with beam time t+1).
//
// `wor` (mv_set_sampling_mode 1): the same loop with the selection replaced by the
// stochastic-beam-search step (launch_sbs_step): bm_lp carries the untempered LP, bm_phi / bm_g
// the tempered log-probability and the perturbed score.  Shared first step, bm_ref dedupe, parent
// indirection, back-trace and gather are the beam's.
void run_decoders_beam(mv_engine* e, int s, Cursors& cur, int Tp, bool wor) {
  const mv_config& c = e->cfg;
  ScaleState& S = e->sc[s];
  const int N = c.batch_size, T = c.obs_len, B = c.beam_size, K = S.K,
            C = c.hidden_size;
  const int R = N * B;
  // The reference tiles the encoder state and the first input over the beams (:497-502,
  // 531-532), so the first cell step (and the attention before it) sees B identical rows
  // per sample.  Rows are independent in every kernel of the step, so that step runs ONCE
  // per sample on the N encoder rows (bit-identical to the tiled computation): its logits
  // are copied to the B beam rows, and the first selection hands out state rows n instead
  // of n * B + parent.  MV_BEAM_SHARED_FIRST=0 restores the tiled first step for A/B runs.
  const bool shared_first = step_knobs().beam_shared_first;
  if (!shared_first) {
    const int cc = cur.cls[s];
    const size_t row4 = (size_t)K * C / 4, total4 = (size_t)R * row4;
    launch(e, "beam_tile_state", 0, 8.0 * total4 * 16, [&] {
      hipLaunchKernelGGL(tile_rows_kernel, dim3(cdiv(total4, 256)), dim3(256), 0,
                         e->issue, S.cls_h[cc].p, S.cls_h[cc ^ 1].p, row4, B, total4);
      hipLaunchKernelGGL(tile_rows_kernel, dim3(cdiv(total4, 256)), dim3(256), 0,
                         e->issue, S.cls_c[cc].p, S.cls_c[cc ^ 1].p, row4, B, total4);
    });
    e->plane_invalidate(S.cls_h[cc ^ 1].p);   // fp32 copy only: planes are re-split
    cur.cls[s] ^= 1;
  }
  HIP_CHECK(hipMemsetAsync(e->bm_lp[0].p, 0, (size_t)R * sizeof(float), e->issue));
  if (wor) {
    MV_REQUIRE(!c.use_single_decoder, "sampling without replacement: use_single_decoder is not "
               "supported");
    require_row_fits_wave("sampling without replacement", K);
    MV_REQUIRE(B <= K, "sampling without replacement: beam_size %d > K = %d cells (the first "
               "step has only K distinct candidates)", B, K);
    HIP_CHECK(hipMemsetAsync(e->bm_phi[0].p, 0, (size_t)R * sizeof(float), e->issue));
    HIP_CHECK(hipMemsetAsync(e->bm_g[0].p, 0, (size_t)R * sizeof(float), e->issue));
  }
  // ragged forward (per-row lengths): the cell step of time t runs on the samples that take
  // prediction step t - 1, a prefix of rows_at(t - 1) of them; the buffers keep the batch's
  // layout.  Row n's final scores are those after the selection at time L[n] (0 for L[n] = 0).
  const bool ragged = e->len.ragged;
  const int Tsteps = ragged ? e->len.steps : Tp;
  if (ragged)
    HIP_CHECK(hipMemsetAsync(e->bm_lp_final.p, 0, (size_t)R * sizeof(float), e->issue));
  if (ragged && wor) {
    HIP_CHECK(hipMemsetAsync(e->bm_g_final.p, 0, (size_t)R * sizeof(float), e->issue));
    HIP_CHECK(hipMemsetAsync(e->bm_phi_final.p, 0, (size_t)R * sizeof(float), e->issue));
  }
  int lpi = 0;
  const int32_t* src = nullptr;  // state row indirection for the next cell step
  const bool sparse = sparse_x_on(e, S);
  // Graph attention BEFORE the parent gather: h + GNN(h) depends on the state row alone, and
  // the B beams of a sample descend from few distinct parents, so it is computed once per
  // state row that some surviving beam continues (beam_select marks them in bm_ref; the rest
  // are skipped) and the next cell step reads it through the parent indirection, like c.
  // Bit-identical to attention after the gather.  MV_BEAM_GNN_DEDUPE=0 gathers first; when
  // else: step_plan.h beam_gnn_dedupe.
  const bool dedupe = beam_gnn_dedupe(c, K, shared_first);
  for (int time = 0; time <= Tsteps && Tsteps > 0; ++time) {
    // samples of this iteration's cell step / of the next one (uniform forward: N both)
    const int n_now = e->rows_at(std::max(time - 1, 0)), n_next = e->rows_at(time);
    // rows the state holds going INTO this iteration's kernels
    const bool one_per_sample = shared_first && time <= 1;
    const int rows_now = one_per_sample ? n_now : n_now * B;
    if (time > 0) {
      // cell step; h comes from the GNN buffer (identity rows) when use_gnn, c through
      // the parent indirection
      std::vector<ConvLstmArgs> probs;
      probs.push_back(beam_cls_problem(e, s, cur, time, rows_now,
                                       (c.use_gnn && !dedupe) ? nullptr : src, src,
                                       one_per_sample ? 1 : B,
                                       e->bm_ids.p + (size_t)std::max(time - 2, 0) * R, 1));
      const bool v2 = tail_grouped(e);
      const bool single = c.use_single_decoder != 0;
      MV_REQUIRE(!single || v2, "use_single_decoder with beam search needs the v2 decoder tail");
      if (!single) probs.push_back(reg_decoder_problem(e, s, cur, time - 1, Tp, !v2));
      run_conv_group(e, probs);
      float* logits = e->bm_logits.p + (size_t)(time - 1) * R * K;
      // single decoder: the offsets of this step, decoded from every state row (traced back
      // along the beams after the loop)
      float* regstep = single ? e->bm_reg_steps.p + (size_t)(time - 1) * R * K * 2 : nullptr;
      // one row per sample: the logits land in beam 0's row of each sample
      const size_t lrow = one_per_sample ? (size_t)B * K : (size_t)K;
      if (v2) {
        TailPlan pl{};
        pl.s = s;
        pl.cls_h = S.cls_h[cur.cls[s]].p; pl.cls_rows = rows_now;
        pl.cls_out = logits; pl.cls_stride = lrow; pl.cls_next = false;   // beam_step selects
        if (single) {
          pl.reg_h = pl.cls_h; pl.reg_rows = rows_now;
          pl.reg_out = regstep; pl.reg_stride = (int64_t)lrow * 2; pl.reg_next = false;
        } else {
          tail_reg_chain(S, cur, s, time - 1, Tp, n_now, pl);
        }
        run_tail(e, {pl});
      } else {
        reg_decoder_output(e, s, cur, time - 1, Tp);
        run_hidden2grid<1>(e, S, S.cls_h[cur.cls[s]].p, S.out_cls_W->dev.p, logits,
                           lrow, rows_now);
      }
      if (one_per_sample) {
        const size_t total = (size_t)n_now * B * K;
        hipLaunchKernelGGL(tile_beam0_kernel, dim3(cdiv(total, 256)), dim3(256), 0,
                           e->issue, logits, K, B, total);
        if (single)
          hipLaunchKernelGGL(tile_beam0_kernel, dim3(cdiv(total * 2, 256)), dim3(256), 0,
                             e->issue, regstep, K * 2, B, total * 2);
      }
      int32_t* ids = e->bm_ids.p + (size_t)(time - 1) * R;
      int32_t* parents = e->bm_parents.p + (size_t)(time - 1) * R;
      if (dedupe)
        HIP_CHECK(hipMemsetAsync(e->bm_ref.p, 0, (size_t)n_now * B * sizeof(int32_t), e->issue));
      const StepTerms terms =
          step_terms(e, S, time - 1, e->bm_ids.p, (size_t)R, 1, e->bm_parents.p);
      if (wor) launch(e, "sbs_step", 0, 16.0 * n_now * B * K, [&] {
        launch_sbs_step(e->issue, logits, e->bm_phi[lpi].p, e->bm_lp[lpi].p, e->bm_g[lpi].p,
                        e->bm_cand.p, e->bm_sbs_lp.p, e->bm_sbs_q.p, e->samp_params.p, n_now, B,
                        K, time - 1, e->bm_phi[lpi ^ 1].p, e->bm_lp[lpi ^ 1].p,
                        e->bm_g[lpi ^ 1].p, ids, parents, e->bm_src_row.p,
                        one_per_sample ? 1 : B, dedupe ? e->bm_ref.p : nullptr, terms);
      });
      else launch(e, "beam_step", 0, 4.0 * n_now * B * K, [&] {
        launch_beam_step(e->issue, logits, e->bm_lp[lpi].p, e->bm_cand.p, n_now, B, K, time,
                         c.diverse_beam, logf(c.diverse_gamma), c.fix_num_timestep,
                         e->bm_lp[lpi ^ 1].p, ids, parents, e->bm_src_row.p,
                         one_per_sample ? 1 : B, dedupe ? e->bm_ref.p : nullptr, terms);
      });
      lpi ^= 1;
      src = e->bm_src_row.p;
      if (ragged)
        hipLaunchKernelGGL(ragged_capture_lp_kernel, dim3(cdiv((size_t)n_now * B, 256)), dim3(256),
                           0, e->issue, e->bm_lp[lpi].p, e->lens_dev.p, e->bm_lp_final.p,
                           n_now * B, B, time);
      if (ragged && wor)
        hipLaunchKernelGGL(ragged_capture_lp_kernel, dim3(cdiv((size_t)n_now * B, 256)), dim3(256),
                           0, e->issue, e->bm_g[lpi].p, e->lens_dev.p, e->bm_g_final.p,
                           n_now * B, B, time);
      if (ragged && wor)
        hipLaunchKernelGGL(ragged_capture_lp_kernel, dim3(cdiv((size_t)n_now * B, 256)), dim3(256),
                           0, e->issue, e->bm_phi[lpi].p, e->lens_dev.p, e->bm_phi_final.p,
                           n_now * B, B, time);
      if (time == Tsteps) break;
      if (!sparse) run_emb_onehot(e, S, ids, 1, S.xbuf_cls.p, n_next * B);
    } else if (sparse) {
      // the embedded one-hot input enters the gate kernel as table terms (sparse_x.h)
    } else if (shared_first) {
      // one_hot(last observed cell) (:497-498, 531-532), one row per sample
      run_emb_onehot(e, S, S.labels.p + (T - 1), T, S.xbuf_cls.p, n_next, 1);
    } else {
      run_emb_onehot(e, S, S.labels.p + (T - 1), T, S.xbuf_cls.p, n_next * B, B);
    }
    if (c.use_gnn) {
      // time 0 (shared): N rows in, N rows out; afterwards R rows gathered through src
      // (which, after the first selection, indexes the N-row state)
      if (dedupe) {
        // on the state rows themselves (N of them up to the first selection)
        GnnJob job{&S, S.cls_h[cur.cls[s]].p, nullptr, S.cls_hg.p,
                   one_per_sample ? n_next : n_next * B, one_per_sample ? 1 : B};
        job.row_ref = time >= 2 ? e->bm_ref.p : nullptr;
        run_gnn_jobs(e, {job});
      } else {
      const int out_rows = (shared_first && time == 0) ? n_next : n_next * B;
      run_gnn(e, S, S.cls_h[cur.cls[s]].p, src, S.cls_hg.p, out_rows,
              (shared_first && time == 0) ? 1 : B);
      }
    }
  }
  // back-trace of row n from step L[n] - 1 (uniform: pred_len - 1); ids -1, logits / offsets 0
  // from step L[n] on
  hipLaunchKernelGGL(beam_backtrace_kernel, dim3(cdiv(R, 256)), dim3(256), 0, e->issue,
                     e->bm_ids.p, e->bm_parents.p, ragged ? e->lens_dev.p : nullptr,
                     e->bm_out_ids.p, e->bm_trace.p, N, B, Tp);
  const size_t total = (size_t)R * Tp * K;
  hipLaunchKernelGGL(beam_gather_kernel, dim3(cdiv(total, 256)), dim3(256), 0, e->issue,
                     e->bm_logits.p, e->bm_trace.p, e->bm_out_logits.p, N, B, Tp, K);
  if (c.use_single_decoder)         // offsets along every beam: the same gather, 2K per row
    hipLaunchKernelGGL(beam_gather_kernel, dim3(cdiv(total * 2, 256)), dim3(256), 0, e->issue,
                       e->bm_reg_steps.p, e->bm_trace.p, e->bm_out_reg.p, N, B, Tp, K * 2);
  // the final logprobs go to bm_lp[0]
  const float* lp_final = ragged ? e->bm_lp_final.p : e->bm_lp[lpi].p;
  if (lp_final != e->bm_lp[0].p)
    HIP_CHECK(hipMemcpyAsync(e->bm_lp[0].p, lp_final, (size_t)R * sizeof(float),
                             hipMemcpyDeviceToDevice, e->issue));
  if (wor) {                        // and the final perturbed scores to bm_g[0]
    const float* g_final = ragged ? e->bm_g_final.p : e->bm_g[lpi].p;
    if (g_final != e->bm_g[0].p)
      HIP_CHECK(hipMemcpyAsync(e->bm_g[0].p, g_final, (size_t)R * sizeof(float),
                               hipMemcpyDeviceToDevice, e->issue));
    // the final phi is the futures' log-probability under the proposal
    HIP_CHECK(hipMemcpyAsync(e->lq_acc.p, ragged ? e->bm_phi_final.p : e->bm_phi[lpi].p,
                             (size_t)R * sizeof(float), hipMemcpyDeviceToDevice, e->issue));
  }
}

// Sampled multi-future decoder (mv_set_sampling; defined here): the class decoder
// of run_decoders_beam with the selection replaced by one Gumbel-max draw per row.  Row (n, s)
// always continues itself, so there is no parent indirection, no back-trace and no gather: the
// decode tail writes step t's logits into the [R, T, K] output, sample_step_kernel draws the id
// into the [R, T] output, and the next cell step reads it from there.  The first cell step runs
// once per sample on the shared encoder state, like the beam's; the S rows of sample n pick that
// state row up through bm_src_row (= n) at the second cell step, the only indexed read.
//
// `scored` (mv_score_futures): the same loop teacher-forced.  The ids are GIVEN:
// the forward starts by copying the uploaded futures into the [R, T] output, score_step_kernel
// reads step t's id there instead of drawing it (log-probability and rank of the given cell),
// and the lengths are per FUTURE (score_len [R]); the per-sample maxima drive rows_at.
void run_decoders_selfcont(mv_engine* e, int s, Cursors& cur, int Tp, bool scored) {
  const mv_config& c = e->cfg;
  ScaleState& S = e->sc[s];
  const int N = c.batch_size, T = c.obs_len, B = c.beam_size, K = S.K;
  const int R = N * B;
  const char* who = scored ? "scoring forward" : "sampled decode";
  require_row_fits_wave(who, K);
  MV_REQUIRE(!c.use_single_decoder, "%s: use_single_decoder is not supported", who);
  MV_REQUIRE(tail_grouped(e), "%s needs the v2 decoder tail", who);
  HIP_CHECK(hipMemsetAsync(e->bm_lp[0].p, 0, (size_t)R * sizeof(float), e->issue));
  if (!scored) HIP_CHECK(hipMemsetAsync(e->lq_acc.p, 0, (size_t)R * sizeof(float), e->issue));
  if (scored) {
    // rows a ragged step does not launch keep step_lp 0 / rank -1 (0xFF bytes: int32 -1)
    const size_t rt = (size_t)R * Tp;
    HIP_CHECK(hipMemsetAsync(e->score_step_lp.p, 0, rt * sizeof(float), e->issue));
    HIP_CHECK(hipMemsetAsync(e->score_rank.p, 0xFF, rt * sizeof(int32_t), e->issue));
    HIP_CHECK(hipMemcpyAsync(e->bm_out_ids.p, e->score_ids.p, rt * sizeof(int32_t),
                             hipMemcpyDeviceToDevice, e->issue));
  }
  const bool ragged = e->len.ragged;
  const int Tsteps = ragged ? e->len.steps : Tp;
  const bool sparse = sparse_x_on(e, S);
  const int64_t orow = (int64_t)Tp * K;             // one row of the [R, T, K] logits
  for (int time = 0; time <= Tsteps && Tsteps > 0; ++time) {
    const int n_now = e->rows_at(std::max(time - 1, 0)), n_next = e->rows_at(time);
    const bool one_per_sample = time <= 1;          // the state going into this iteration
    const int rows_now = one_per_sample ? n_now : n_now * B;
    if (time > 0) {
      const int t = time - 1;
      const int32_t* src = time == 2 ? e->bm_src_row.p : nullptr;
      std::vector<ConvLstmArgs> probs;
      probs.push_back(beam_cls_problem(e, s, cur, time, rows_now, src, src, 1,
                                       e->bm_out_ids.p + std::max(t - 1, 0), Tp));
      probs.push_back(reg_decoder_problem(e, s, cur, t, Tp, false));
      run_conv_group(e, probs);
      float* logits = e->bm_out_logits.p + (size_t)t * K;
      TailPlan pl{};
      pl.s = s;
      pl.cls_h = S.cls_h[cur.cls[s]].p; pl.cls_rows = rows_now;
      // one row per sample: the logits land in future 0's row of each sample
      pl.cls_out = logits; pl.cls_stride = one_per_sample ? orow * B : orow;
      pl.cls_next = false;                          // sample_step_kernel draws
      tail_reg_chain(S, cur, s, t, Tp, n_now, pl);
      run_tail(e, {pl});
      int32_t* ids = e->bm_out_ids.p + t;
      const int rows = n_now * B;
      const double step_bytes = 4.0 * rows * K * (one_per_sample ? 2 : 1);
      const dim3 grid(cdiv((size_t)rows, 4)), block(256);
      const int shared = one_per_sample ? 1 : 0;
      int32_t* srow = time == 1 ? e->bm_src_row.p : nullptr;
      if (scored) launch(e, "score_step", 0, step_bytes, [&] {
        const int32_t* lens = ragged ? e->score_len.p : nullptr;
        with_rank_j(K, [&](auto j) {
          hipLaunchKernelGGL(mv::score_step_kernel<decltype(j)::value>, grid, block, 0, e->issue,
                             logits, orow, rows, B, K, t, shared, lens, e->bm_lp[0].p, ids, Tp,
                             e->score_step_lp.p + t, e->score_rank.p + t, srow);
        });
      });
      else launch(e, "sample_step", 0, step_bytes, [&] {
        const int32_t* lens = ragged ? e->lens_dev.p : nullptr;
        // the sampler's rows continue themselves: their path is their own row of the [R, T] ids
        launch_sample_step(e->issue, logits, orow, rows, B, K, t, shared, e->samp_params.p, 1,
                           lens, e->bm_lp[0].p, e->lq_acc.p, ids, Tp, srow, (uint8_t*)nullptr,
                           step_terms(e, S, t, e->bm_out_ids.p, 1, Tp, nullptr));
      });
      if (time == Tsteps) break;
      if (!sparse) run_emb_onehot(e, S, ids, Tp, S.xbuf_cls.p, n_next * B);
    } else if (!sparse) {
      // one_hot(last observed cell), one row per sample
      run_emb_onehot(e, S, S.labels.p + (T - 1), T, S.xbuf_cls.p, n_next, 1);
    }
    if (c.use_gnn)     // on the state rows: one per sample until the second cell step has run
      run_gnn(e, S, S.cls_h[cur.cls[s]].p, nullptr, S.cls_hg.p,
              time <= 1 ? n_next : n_next * B, time <= 1 ? 1 : B);
  }
  if (ragged) {
    // logits 0 and ids -1 from step L[n] on (a finished row inside a step's prefix kept decoding)
    // (scored: from step len[n, f] on, one length per future)
    const size_t total = (size_t)R * Tp * K;
    const int32_t* lens = scored ? e->score_len.p : e->lens_dev.p;
    const int per_len = scored ? 1 : B;
    hipLaunchKernelGGL(ragged_zero_tail_kernel, dim3(cdiv(total, 256)), dim3(256), 0, e->issue,
                       e->bm_out_logits.p, lens, R, Tp, K, per_len);
    hipLaunchKernelGGL(ragged_ids_tail_kernel, dim3(cdiv((size_t)R * Tp, 256)), dim3(256), 0,
                       e->issue, e->bm_out_ids.p, lens, R, per_len, Tp);
  }
}

// "The last enabled scale": the one a beam handle decodes on.
int beam_scale(const mv_engine* e) {
  int s = 0;
  for (int i = 0; i < e->cfg.num_scales; ++i) if (e->sc[i].use) s = i;
  return s;
}

void enqueue_forward(mv_engine* e, ForwardKind kind, bool capturing = false) {
  const mv_config& c = e->cfg;
  const int Tp = e->pred_len;
  const bool beam = kind != ForwardKind::Greedy;
  // the greedy forward as two chain pairs on two streams, or everything on one (step_plan.h)
  const bool pairs = chain_pairs_planned(c, !beam, e->stream_b != nullptr, e->profiling,
                                         capturing, tail_grouped(e));
  Cursors cur;
  auto decode_on_beams = [&] {
    if (kind == ForwardKind::Beam || kind == ForwardKind::SampledWor)
      run_decoders_beam(e, beam_scale(e), cur, Tp, kind == ForwardKind::SampledWor);
    else run_decoders_selfcont(e, beam_scale(e), cur, Tp, kind == ForwardKind::Scored);
  };
  if (e->len.ragged && e->len.steps == 0) {       // every row is padding: nothing to compute
    if (beam) decode_on_beams();                  // (its finalisers alone)
    return;
  }
  if (pairs) {
    ChainFork fork(e);
    if (!e->no_scene()) { IssueOn on(e, 0); run_scene(e); }
    run_encoders(e, cur, true);
    run_decoders_greedy(e, cur, Tp, true);
    HIP_CHECK(hipGetLastError());
    return;
  }
  if (!e->no_scene()) run_scene(e);
  run_encoders(e, cur, false);
  if (beam) decode_on_beams();
  else run_decoders_greedy(e, cur, Tp, false);
  HIP_CHECK(hipGetLastError());
}

// The per-row lengths of this forward (mv_set_pred_lengths): checked against pred_len, and the
// active-row prefix of every step.  All lengths == pred_len (or none set): the uniform forward.
void plan_ragged(mv_engine* e) {
  e->len.reset();
  if (!e->lens_set) return;
  const int N = e->cfg.batch_size, Tp = e->pred_len;
  bool uniform = true;
  for (int n = 0; n < N; ++n) {
    MV_REQUIRE(e->lens_host[n] >= 0 && e->lens_host[n] <= Tp,
               "pred_lengths[%d] = %d not in [0, pred_len=%d]", n, e->lens_host[n], Tp);
    uniform = uniform && e->lens_host[n] == Tp;
  }
  if (!uniform) e->len.build(e->lens_host, Tp);
}

// The per-row observation lengths of this forward (mv_set_obs_lengths): checked against
// obs_len, and the started-row prefix of every encoder step over the rows that decode at all
// (after plan_ragged / plan_scored).  All lengths == obs_len (or none set): the uniform forward.
void plan_obs(mv_engine* e) {
  e->obs.reset();
  if (!e->obs_lens_set) return;
  const int N = e->cfg.batch_size, T = e->cfg.obs_len;
  bool uniform = true;
  for (int n = 0; n < N; ++n) {
    MV_REQUIRE(e->obs_lens_host[n] >= 1 && e->obs_lens_host[n] <= T,
               "obs_lengths[%d] = %d not in [1, obs_len=%d]", n, e->obs_lens_host[n], T);
    uniform = uniform && e->obs_lens_host[n] == T;
  }
  if (!uniform) e->obs.build(e->obs_lens_host, T, e->rows_at(0));
}

// The plan of a scoring forward: the lengths came with the futures (mv_upload_score_futures
// checked them), one per future.  Uniform only if EVERY future runs to pred_len; otherwise the
// per-sample maxima L[n] give the active-row prefixes and go to lens_dev, where the finalisers
// and the trajectory decode read per-sample lengths (mv_set_pred_lengths is not set: its copy
// there is dead until it is set again, which uploads it again).
void plan_scored(mv_engine* e) {
  MV_REQUIRE(!e->lens_set, "mv_run_score_resident: per-row prediction lengths are set "
             "(mv_set_pred_lengths); the lengths of a scoring forward come with the futures -- "
             "clear them first");
  MV_REQUIRE(e->score_ready, "mv_run_score_resident: no futures uploaded "
             "(mv_upload_score_futures)");
  MV_REQUIRE(e->score_pred_len == e->pred_len, "mv_run_score_resident: the futures were uploaded "
             "for pred_len %d, the inputs now have pred_len %d (upload the futures again after "
             "mv_upload_inputs)", e->score_pred_len, e->pred_len);
  e->len.reset();
  if (e->score_uniform) return;
  e->len.build(e->score_L, e->pred_len);
  HIP_CHECK(hipMemcpyAsync(e->lens_dev.p, e->score_L.data(), e->score_L.size() * sizeof(int32_t),
                           hipMemcpyHostToDevice, e->stream));
}

// The cell mask of this forward (mv_set_cell_mask), checked for the forwards that CHOOSE cells
// (after plan_ragged): every row that decodes needs an allowed cell at every step below its
// length, and beam_size of them at step 0 where only the root's K children are candidates.
void plan_cell_mask(mv_engine* e, ForwardKind kind) {
  if (kind == ForwardKind::Scored || kind == ForwardKind::Greedy) return;
  const StepConstraints& con = e->con;
  if (con.bias.set())
    MV_REQUIRE(con.bias.tm == 1 || con.bias.tm >= e->pred_len, "mv_set_cell_bias: the bias has "
               "Tm = %d planes, the forward pred_len = %d steps (Tm must be 1 or at least "
               "pred_len)", con.bias.tm, e->pred_len);
  if (!con.mask.set()) return;
  const mv_config& c = e->cfg;
  const int N = c.batch_size, Tp = e->pred_len, Tm = con.mask.tm, B = c.beam_size;
  MV_REQUIRE(Tm == 1 || Tm >= Tp, "mv_set_cell_mask: the mask has Tm = %d planes, the forward "
             "pred_len = %d steps (Tm must be 1 or at least pred_len)", Tm, Tp);
  const bool top_b = kind == ForwardKind::Beam || kind == ForwardKind::SampledWor;
  for (int n = 0; n < N; ++n) {
    const int L = e->len.ragged ? e->lens_host[n] : Tp;
    for (int t = 0; t < L; ++t) {
      const int cnt = con.mask_count[(size_t)n * Tm + (Tm > 1 ? t : 0)];
      MV_REQUIRE(cnt >= 1, "mv_set_cell_mask: row n = %d has %d allowed cells at step t = %d "
                 "(every step below the row's length needs at least one)", n, cnt, t);
      if (t == 0 && top_b)
        MV_REQUIRE(cnt >= B, "mv_set_cell_mask: row n = %d has %d allowed cells at step t = 0, "
                   "fewer than beam_size = %d (only the root's children are candidates at the "
                   "first step)", n, cnt, B);
    }
  }
}

// out_cls / out_reg of a ragged forward: exact zeros from step L[n] on (rows past a step's
// active prefix were not written at all).  On the engine's stream, after the chain pairs met.
void finish_ragged(mv_engine* e, bool beam) {
  const mv_config& c = e->cfg;
  const int N = c.batch_size, Tp = e->pred_len;
  for (int s = 0; s < c.num_scales; ++s) {
    ScaleState& S = e->sc[s];
    if (!S.use) continue;
    const size_t nc = (size_t)N * Tp * S.K;
    if (!beam)
      hipLaunchKernelGGL(ragged_zero_tail_kernel, dim3(cdiv(nc, 256)), dim3(256), 0, e->stream,
                         S.out_cls.p, e->lens_dev.p, N, Tp, S.K);
    if (!(beam && c.use_single_decoder))     // (beam, single decoder: bm_out_reg, gathered)
      hipLaunchKernelGGL(ragged_zero_tail_kernel, dim3(cdiv(nc * 2, 256)), dim3(256), 0,
                         e->stream, S.out_reg.p, e->lens_dev.p, N, Tp, S.K * 2);
  }
  HIP_CHECK(hipGetLastError());
}

// One forward = one `sess.run`.  In graph mode the ~150 (greedy) / ~120 (beam)
// launches of a forward are captured once per (kind, T_pred, U) into a hipGraph
// and replayed; every device pointer in it is engine-owned and stable.  (A sampled forward reads
// its seed and temperature on the device, a scoring forward its ids from an engine-owned buffer:
// their graphs follow a later mv_set_sampling / mv_upload_score_futures.)
void run_forward(mv_engine* e, ForwardKind kind) {
  const mv_config& c = e->cfg;
  const bool beam = kind != ForwardKind::Greedy;
  if (kind == ForwardKind::Scored) {
    MV_REQUIRE(c.beam_size > 1, "mv_score_futures: engine was created with beam_size 1 (a scoring "
               "forward scores beam_size futures per row: create a beam handle)");
    MV_REQUIRE(!c.use_single_decoder, "mv_score_futures: use_single_decoder handles are not "
               "supported (the scoring forward keeps the un-beamed regression decoder)");
  }
  MV_REQUIRE(e->inputs_ready, "no inputs uploaded (mv_upload_inputs)");
  // a constrained step holds a row in one wave: refused before anything is launched
  const StepConstraints& con = e->con;
  const bool constrainable = kind != ForwardKind::Scored && kind != ForwardKind::Greedy;
  const struct { bool set; const char* who; } row_bound[] = {
      {con.mask.set(), "mv_set_cell_mask: a masked step"},
      {con.bias.set(), "mv_set_cell_bias: a biased step"},
      {con.motion_set(), "mv_set_motion_cost: a step under a motion cost"},
      {con.revisit_set(), "mv_set_revisit_cost: a step under a revisit cost"}};
  for (const auto& b : row_bound)
    if (constrainable && b.set) require_row_fits_wave(b.who, e->sc[beam_scale(e)].K);
  ensure_params(e);
  if (beam)
    MV_REQUIRE(c.beam_size > 1, "engine was created with beam_size 1");
  if (kind == ForwardKind::Scored) plan_scored(e); else plan_ragged(e);
  plan_obs(e);
  plan_cell_mask(e, kind);
  // a ragged forward's launches depend on the lengths, which the graph key does not carry: it
  // is issued eagerly; so is an obs-ragged one
  if (!e->graph_mode || e->profiling || e->len.ragged || e->obs.ragged) {
    e->gate_rows = 0;
    enqueue_forward(e, kind);
    if (e->len.ragged) finish_ragged(e, beam);
    e->last = kind;
    return;
  }
  // (a scoring forward reads no mask and no bias: one graph whatever is set)
  const int mask_key = !constrainable ? 0
      : constraint_graph_key(con.mask.layout(), con.bias.layout(), con.motion_radius,
                             con.motion_acc, con.revisit_set(), con.revisit_seed);
  const auto key = std::make_tuple(kind, e->pred_len, e->num_frames, mask_key);
  auto it = e->graphs.find(key);
  if (it == e->graphs.end()) {
    e->gate_rows = 0;
    hipGraph_t g = nullptr;
    HIP_CHECK(hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal));
    try {
      enqueue_forward(e, kind, /*capturing=*/true);
    } catch (...) {
      (void)hipStreamEndCapture(e->stream, &g);
      if (g) (void)hipGraphDestroy(g);
      throw;
    }
    HIP_CHECK(hipStreamEndCapture(e->stream, &g));
    hipGraphExec_t ex = nullptr;
    hipError_t ie = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    HIP_CHECK(ie);
    it = e->graphs.emplace(key, ex).first;
    ++e->graph_captures;
    e->graph_gate_rows[key] = e->gate_rows;
  }
  e->gate_rows = e->graph_gate_rows[key];
  HIP_CHECK(hipGraphLaunch(it->second, e->stream));
  e->last = kind;
}

}  // namespace
