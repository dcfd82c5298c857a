// single-kernel entry points of the C ABI (mv_op_*: what the kernel-level parity tests call) -- part of the ONE translation unit engine.hip (included from there, in order;
// not a stand-alone header).
#pragma once

extern "C" {

// ------------------------------------------------------- single-kernel ops

int mv_op_convlstm_step(int device, const float* x, const float* c, const float* h,
                        const float* kernel, const float* biases, int32_t M,
                        int32_t H, int32_t W, int32_t Cx, int32_t C, float* c_out,
                        float* h_out) {
  return guarded(nullptr, [&] {
    MV_REQUIRE(C % mv::kChBlock == 0 && C % mv::kBK == 0, "C %d must be a multiple of 32", C);
    MV_REQUIRE(mv::convlstm_cx_supported(Cx), "Cx %d unsupported (multiple of 32, or <= 3)", Cx);
    OpCtx ctx(device);
    const size_t cells = (size_t)M * H * W;
    DevBuf<float> dx, dc, dh, dw, db, dco, dho;
    ctx.up(dx, x, cells * Cx);
    ctx.up(db, biases, (size_t)4 * C);
    std::vector<float> packed(mv::convlstm_wpack_elems(Cx, C));
    mv::pack_convlstm_weights(kernel, Cx, C, packed.data());
    ctx.up(dw, packed.data(), packed.size());
    const bool zero = (c == nullptr && h == nullptr);
    if (!zero) {
      MV_REQUIRE(c && h, "c and h must both be given or both be NULL");
      ctx.up(dc, c, cells * C);
      ctx.up(dh, h, cells * C);
    }
    dco.alloc(cells * C); dho.alloc(cells * C);
    mv::ConvLstmArgs a{};
    a.x = dx.p; a.h = dh.p; a.c = dc.p; a.wpack = dw.p; a.bias = db.p;
    a.h_out = dho.p; a.c_out = dco.p;
    a.rows = M; a.H = H; a.W = W; a.Cx = Cx; a.C = C;
    mv::convlstm_finish_args(a, zero);
    mv::launch_convlstm_steps(&a, 1, ctx.stream);
    HIP_CHECK(hipGetLastError());
    ctx.down(c_out, dco, cells * C);
    ctx.down(h_out, dho, cells * C);
  });
}

namespace {
// planes (hi + lo) / 256 of an [M][C] tensor in the tiled operand layout -> fp32 [M][C]
__global__ void decode_planes_kernel(const _Float16* __restrict__ p0,
                                     const _Float16* __restrict__ p1, float* __restrict__ out,
                                     size_t M, int C) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M * (size_t)C) return;
  const size_t m = i / C;
  const int ch = (int)(i - m * C);
  const size_t o = mv::plane_index((long long)m, ch, C);
  out[i] = ((float)p0[o] + (float)p1[o]) * (1.0f / 256.0f);
}
// ONE bf16 plane of an [M][C] tensor in the tiled operand layout -> fp32 [M][C]
__global__ void decode_plane_bf16_kernel(const _Float16* __restrict__ p0, float* __restrict__ out,
                                         size_t M, int C) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M * (size_t)C) return;
  const size_t m = i / C;
  const int ch = (int)(i - m * C);
  const uint16_t b = __builtin_bit_cast(uint16_t, p0[mv::plane_index((long long)m, ch, C)]);
  out[i] = __uint_as_float((uint32_t)b << 16);
}
}  // namespace

int mv_op_convlstm_step16(int device, int32_t variant, const float* x, const float* c,
                          const float* h, const float* kernel, const float* biases,
                          int32_t M, int32_t H, int32_t W, int32_t Cx, int32_t C,
                          float* c_out, float* h_out, float* h16_out) {
  return guarded(nullptr, [&] {
    MV_REQUIRE(variant >= 1 && variant <= 6, "variant %d: 1 = direct f16x3, 2 = Winograd F(2,3), "
               "3 = Winograd F(3,3), 4 = bf16 on the row-triple tile, 5 = bf16 on the 32-cell body, "
               "6 = the same with three x passes", variant);
    const bool bf = variant >= 4;
    // variant 6: the x operand of an unbounded-activation model -- two fp16 planes of 2^e x under
    // the tensor's own exponent; h stays one bf16 plane
    const bool xf16 = variant == 6;
    MV_REQUIRE(C % mv::kChBlock == 0 && C % mv::kBK == 0, "C %d must be a multiple of 32", C);
    MV_REQUIRE(mv::f16x3_cx_supported(Cx), "Cx %d unsupported (multiple of 16, or <= 3)", Cx);
    MV_REQUIRE(H * W >= 32, "grids of at least 32 cells");
    const bool small = x_is_small(Cx);
    const int xpass = xf16 ? 3 : 1;
    if (variant >= 5) {       // the 32-cell body's own refusals, as prepare_gate_operands states them
      MV_REQUIRE(!(xf16 && small), "variant 6: the three x passes are of a dense x operand "
                 "(Cx %d travels as the fp32 chunk)", Cx);
      const int nxk = small ? 0 : xpass * mv::f16x3_xksteps(Cx), nhk = 9 * (C / 16);
      MV_REQUIRE((nxk / 3) % MV_BF16_UNITS == 0 && (nhk / 3) % MV_BF16_UNITS == 0,
                 "bf16 mode: %d x / %d h k-steps do not fill whole LDS stages (emb_size and "
                 "scene_conv_dim must be multiples of 32)", nxk, nhk);
    }
    OpCtx ctx(device);
    const size_t cells = (size_t)M * H * W;
    const int Cx16 = x_chunk16(Cx);
    const int Cin = Cx + C, N4 = 4 * C;
    DevBuf<float> dx, dc, dh, dw, db, dco, dho, dk, dwx, dplanes;
    DevBuf<_Float16> px, ph, pho, wp, v3x, v3h;
    DevBuf<int32_t> xexp;
    ctx.up(dx, x, cells * Cx);
    ctx.up(db, biases, (size_t)4 * C);
    ctx.up(dk, kernel, (size_t)9 * Cin * N4);
    std::vector<float> packed(mv::convlstm_wpack_elems(Cx, C));
    mv::pack_convlstm_weights(kernel, Cx, C, packed.data());
    ctx.up(dw, packed.data(), packed.size());
    const bool zero = (c == nullptr && h == nullptr);
    if (!zero) {
      MV_REQUIRE(c && h, "c and h must both be given or both be NULL");
      ctx.up(dc, c, cells * C);
      ctx.up(dh, h, cells * C);
    }
    dco.alloc(cells * C); dho.alloc(cells * C);
    mv::ConvLstm16Args q{};
    mv::ConvLstmArgs& a = q.f;
    // operand planes: [pad | plane 0 | slack][pad | plane 1 | slack], zero-filled
    auto make_planes = [&](DevBuf<_Float16>& buf, const float* src, int Cc, size_t* stride) {
      const size_t pst = cells * Cc + mv::kPlaneSlack + mv::kPlanePad;
      buf.alloc(2 * pst + mv::kPlanePad);
      HIP_CHECK(hipMemsetAsync(buf.p, 0, (2 * pst + mv::kPlanePad) * sizeof(_Float16), ctx.stream));
      _Float16* p0 = buf.p + mv::kPlanePad;
      if (src && xf16 && src == dx.p) {       // as prepare_gate_operands splits an unbounded x
        xexp.alloc(65);
        HIP_CHECK(hipMemsetAsync(xexp.p, 0, 64 * sizeof(int32_t), ctx.stream));
        hipLaunchKernelGGL(mv::absmax_bits_kernel, dim3(256), dim3(256), 0, ctx.stream, src,
                           cells * Cc, xexp.p);
        hipLaunchKernelGGL(mv::split_planes_dyn_kernel, dim3(mv::split_planes_blocks(cells, Cc)),
                           dim3(256), 0, ctx.stream, src, p0, p0 + pst, (int)cells, Cc, xexp.p,
                           xexp.p + 64);
        q.x_exp = xexp.p + 64;
      } else if (src && bf)        // ONE unscaled bf16 plane (compute mode 2)
        hipLaunchKernelGGL(mv::split_plane_bf16_kernel, dim3(mv::split_planes_blocks(cells, Cc)),
                           dim3(256), 0, ctx.stream, src, p0, (int)cells, Cc);
      else if (src)
        hipLaunchKernelGGL(mv::split_planes_kernel, dim3(mv::split_planes_blocks(cells, Cc)),
                           dim3(256), 0, ctx.stream, src, p0, p0 + pst, (int)cells, Cc);
      *stride = pst;
      return p0;
    };
    a.x = dx.p; a.h = dh.p; a.c = dc.p; a.wpack = dw.p; a.bias = db.p;
    a.h_out = dho.p; a.c_out = dco.p;
    a.rows = M; a.H = H; a.W = W; a.Cx = Cx; a.C = C;
    mv::convlstm_finish_args(a, zero);
    size_t xst = 0, hst = 0, ost = 0;
    if (Cx16 > 0) { q.x16 = make_planes(px, dx.p, Cx16, &xst); q.x_plane_stride = (int64_t)xst; }
    if (!zero) { q.h16 = make_planes(ph, dh.p, C, &hst); q.h_plane_stride = (int64_t)hst; }
    q.h16_out = make_planes(pho, nullptr, C, &ost);
    q.h16_out_stride = (int64_t)ost;
    q.n_xk = small ? 0 : xpass * mv::f16x3_xksteps(Cx);
    q.n_hk = zero ? 0 : 9 * (C / 16);
    q.w_ksteps = (small ? 0 : xpass * mv::f16x3_xksteps(Cx)) + 9 * (C / 16);
    // the variant forces its form: the engine's packs and launcher, under an explicit plan
    // (block maps and shift as the engine would choose them)
    ForwardPlan pl;
    pl.shift = gate_knobs().conv_shift && 32 % W == 0;
    pl.map_mode = gate_knobs().conv_map;
    _Float16 *v3xp = nullptr, *v3hp = nullptr;
    if (variant == 1) {
      std::vector<_Float16> p16(mv::f16x3_wpack_elems(Cx16, C));
      if (small) {
        mv::pack_f16x3_weights(kernel_h_rows(kernel, Cx, C).data(), 0, C, p16.data());
        upload(dwx, small_x_chunk(kernel, Cx, C, 65536.0f));
        q.wx32 = dwx.p;
      } else {
        mv::pack_f16x3_weights(kernel, Cx, C, p16.data());
      }
      upload(wp, p16);
      q.wp16 = wp.p;
    } else if (variant >= 5) {
      // the 32-cell body of compute mode 2 (GateForm::Bf16), packed as ensure_packed_bf16 packs
      std::vector<_Float16> pb(mv::bf16_wpack_elems(Cx16, C, xf16));
      if (small) {
        mv::pack_bf16_weights(kernel_h_rows(kernel, Cx, C).data(), 0, C, pb.data());
        upload(dwx, small_x_chunk(kernel, Cx, C, 1.0f));
        q.wx32 = dwx.p;
      } else {
        if (xf16) {       // the x rows travel as fp16 of 256 w: the engine's range bound
          float mx = 0.f;
          for (int t = 0; t < 9; ++t)
            for (int ci = 0; ci < Cx; ++ci)
              for (int n = 0; n < N4; ++n)
                mx = std::max(mx, std::fabs(kernel[((size_t)t * Cin + ci) * N4 + n]));
          MV_REQUIRE(mx * mv::kF16Scale < 60000.f, "variant 6: the x rows of the kernel reach %g, "
                     "outside the scaled fp16 range", mx);
        }
        mv::pack_bf16_weights(kernel, Cx, C, pb.data(), xf16);
      }
      upload(wp, pb);
      q.wp16 = wp.p;
      pl.form = GateForm::Bf16;
      pl.x_passes = xpass;
    } else if (variant == 4) {
      MV_REQUIRE(mv::bf16t_geometry_ok(a, q), "bf16 row-triple tile: H %d >= 3", H);
      pack_bf16t(ctx.stream, dk.p, Cx, C, wp);
      q.x_plane_stride = q.h_plane_stride = q.h16_out_stride = 0;     // single planes
      pl.form = GateForm::Bf16T;
      pl.halo = mv::wino3_needs_halo(a);
      pl.map_mode = gate_knobs().wino_map_bf16t;
    } else if (variant == 3) {
      MV_REQUIRE(mv::wino3_geometry_ok(a, q), "Winograd F(3,3) form: H %d >= 3", H);
      MV_REQUIRE(!mv::wino3_needs_halo(a) || mv::wino3_halo_addressable(a),
                 "Winograd F(3,3) form, halo tiling (W %d does "
                 "not divide 32): an operand of 2 GiB or more is not addressable", W);
      pack_wino3(ctx.stream, dk.p, Cx, C, wp);
      pl.form = GateForm::Wino3;
      pl.halo = mv::wino3_needs_halo(a);
      pl.map_mode = gate_knobs().wino_map_f33;
      // the pre-transformed operands, as the engine hands them over
      std::vector<mv::Wn3TransformItem> tr;
      if (!zero) {
        v3h.alloc(mv::wino3_v_elems(M, H, W, C));
        queue_wino3_transform(tr, {q.h16, q.h_plane_stride, v3hp = v3h.p, nullptr, M, H, W, C});
      }
      if (Cx16 > 0) {
        v3x.alloc(mv::wino3_v_elems(M, H, W, Cx16));
        queue_wino3_transform(tr, {q.x16, q.x_plane_stride, v3xp = v3x.p, nullptr, M, H, W, Cx16});
      }
      mv::launch_wino3_transforms(tr.data(), (int)tr.size(), ctx.stream);
    } else {
      MV_REQUIRE(mv::wino_geometry_ok(a), "Winograd form: W %d must divide 32, H >= 2", W);
      pack_wino(ctx.stream, dk.p, Cx, C, wp);
      pl.form = GateForm::Wino2;
      pl.map_mode = gate_knobs().wino_map_f23;
    }
    const _Float16* pack = wp.p;
    const float* hwio = dk.p;
    launch_gate_group(pl, &q, &pack, &hwio, &v3xp, &v3hp, 1, ctx.stream);
    HIP_CHECK(hipGetLastError());
    if (h16_out) {
      dplanes.alloc(cells * C);
      if (bf)
        hipLaunchKernelGGL(decode_plane_bf16_kernel, dim3(cdiv(cells * C, 256)), dim3(256), 0,
                           ctx.stream, q.h16_out, dplanes.p, cells, C);
      else
      hipLaunchKernelGGL(decode_planes_kernel, dim3(cdiv(cells * C, 256)), dim3(256), 0,
                         ctx.stream, q.h16_out, q.h16_out + ost, dplanes.p, cells, C);
      HIP_CHECK(hipGetLastError());
      ctx.down(h16_out, dplanes, cells * C);
    }
    ctx.down(c_out, dco, cells * C);
    ctx.down(h_out, dho, cells * C);
  });
}

// version: 0 = step_plan.h's choice (the MV_GNN knob), 1 / 2 / 3 = at most that kernel version;
// gnn_form's demotions apply to a version asked for as to the knob's.
int mv_op_gnn_variant(int device, const float* h, const float* scene_mean, int32_t M,
                      int32_t H, int32_t W, int32_t C, int32_t D, int32_t version, float* out) {
  return guarded(nullptr, [&] {
    MV_REQUIRE(C % 64 == 0 && C <= 512 && D >= 0 && D <= 128,
               "gnn: C a multiple of 64 up to 512, D <= 128");
    MV_REQUIRE(version >= 0 && version <= 3, "gnn: version %d not in [0, 3]", (int)version);
    OpCtx ctx(device);
    const size_t cells = (size_t)M * H * W;
    DevBuf<float> dh, ds, dout;
    ctx.up(dh, h, cells * C);
    ctx.up(ds, scene_mean, cells * D);
    dout.alloc(cells * C);
    mv::GnnGroup grp{};
    grp.p[0] = mv::GnnProblem{dh.p, ds.p, nullptr, dout.p, nullptr, 0, M, H, W, 1, 0, nullptr};
    // (the bytes this call addresses, not an engine's worst case)
    launch_gnn(ctx.stream, gnn_form(version, W, C, D, cells * C * 4), grp, 1, C, D);
    HIP_CHECK(hipGetLastError());
    ctx.down(out, dout, cells * C);
  });
}

int mv_op_gnn(int device, const float* h, const float* scene_mean, int32_t M,
              int32_t H, int32_t W, int32_t C, int32_t D, float* out) {
  return mv_op_gnn_variant(device, h, scene_mean, M, H, W, C, D, 0, out);
}

int mv_op_hidden2grid(int device, const float* h, const float* w, int32_t M,
                      int32_t H, int32_t W, int32_t C, int32_t P, float* out) {
  return guarded(nullptr, [&] {
    MV_REQUIRE(C % 4 == 0 && (P == 1 || P == 2), "hidden2grid: C %% 4 == 0, P in {1,2}");
    OpCtx ctx(device);
    const size_t cells = (size_t)M * H * W;
    DevBuf<float> dh, dw, dout;
    ctx.up(dh, h, cells * C);
    ctx.up(dw, w, (size_t)9 * C * P);
    dout.alloc(cells * P);
    if (P == 1)
      hipLaunchKernelGGL(mv::hidden2grid_kernel<1>, dim3(cdiv(cells, 4)), dim3(256), 0,
                         ctx.stream, dh.p, dw.p, dout.p, (size_t)H * W, M, H, W, C);
    else
      hipLaunchKernelGGL(mv::hidden2grid_kernel<2>, dim3(cdiv(cells, 4)), dim3(256), 0,
                         ctx.stream, dh.p, dw.p, dout.p, (size_t)H * W * 2, M, H, W, C);
    HIP_CHECK(hipGetLastError());
    ctx.down(out, dout, cells * P);
  });
}

// What constrains the step of a single-kernel step op: the device copies of the four optional
// inputs and the StepTerms that point at them.  Every part that is given -- and the one the entry
// point `who` needs, given or not -- validates and uploads itself.
enum class OpNeeds { Nothing, Allowed, Bias, Motion, Revisit };
struct OpStepTerms {
  DevBuf<uint8_t> allowed;
  DevBuf<float> bias, vel, vel_far, acc, acc_far, cost;
  DevBuf<int32_t> motion_prev1, motion_prev0, revisit_prev1;
  DevBuf<uint32_t> set_in, set_out;
  std::vector<uint32_t> words;
  const mv_step_revisit* revisit = nullptr;
  size_t rows = 0;
  int K = 0;
  StepTerms terms;

  // `allowed` [samples, K], `bias` [samples, K] floats, the motion tables with every row's
  // p1 / p0, the revisit cost with every row's p1 and visited set
  void up(OpCtx& ctx, const uint8_t* allowed_h, const float* bias_h, const mv_step_motion* mo,
          const mv_step_revisit* rv, OpNeeds needs, size_t samples, size_t rows_, int K_,
          const char* who) {
    rows = rows_;
    K = K_;
    if (rv || needs == OpNeeds::Revisit) up_revisit(ctx, rv, samples, who);
    if (mo || needs == OpNeeds::Motion) up_motion(ctx, mo, samples, who);
    if (bias_h || needs == OpNeeds::Bias) up_bias(ctx, bias_h, samples, who);
    if (allowed_h || needs == OpNeeds::Allowed) {
      MV_REQUIRE(allowed_h, "%s: NULL allowed", who);
      require_row_fits_wave(who, K);
      ctx.up(allowed, allowed_h, samples * K);
      terms.amask = allowed.p;
      terms.mask_stride = K;
    }
  }

  void up_bias(OpCtx& ctx, const float* bias_h, size_t samples, const char* who) {
    MV_REQUIRE(bias_h, "%s: NULL bias", who);
    require_row_fits_wave(who, K);
    for (size_t i = 0; i < samples * K; ++i)
      MV_REQUIRE(std::isfinite(bias_h[i]), "%s: bias[%d, %d] = %g is not finite", who,
                 (int)(i / K), (int)(i % K), (double)bias_h[i]);
    ctx.up(bias, bias_h, samples * K);
    terms.bias = bias.p;
    terms.bias_stride = K;
  }

  void up_motion(OpCtx& ctx, const mv_step_motion* mo, size_t samples, const char* who) {
    MV_REQUIRE(mo && mo->vel && mo->vel_far && mo->prev1 && mo->prev0,
               "%s: NULL motion, vel, vel_far, prev1 or prev0", who);
    require_row_fits_wave(who, K);
    MV_REQUIRE(mo->radius >= 1 && mo->radius <= MV_MOTION_MAX_RADIUS,
               "%s: radius %d not in [1, %d]", who, (int)mo->radius, MV_MOTION_MAX_RADIUS);
    MV_REQUIRE(mo->W >= 1 && K % mo->W == 0, "%s: W = %d does not divide K = %d", who, (int)mo->W,
               K);
    MV_REQUIRE((mo->acc != nullptr) == (mo->acc_far != nullptr),
               "%s: acc and acc_far are given both or neither", who);
    const size_t DD = (size_t)(2 * mo->radius + 1) * (2 * mo->radius + 1);
    auto finite = [&](const float* p, size_t per, const char* name) {
      for (size_t i = 0; i < samples * per; ++i)
        MV_REQUIRE(std::isfinite(p[i]), "%s: %s[n = %d, entry %d] = %g is not finite", who, name,
                   (int)(i / per), (int)(i % per), (double)p[i]);
    };
    finite(mo->vel, DD, "vel");
    finite(mo->vel_far, 1, "vel_far");
    if (mo->acc) { finite(mo->acc, DD, "acc"); finite(mo->acc_far, 1, "acc_far"); }
    for (size_t r = 0; r < rows; ++r) {
      MV_REQUIRE(mo->prev1[r] >= 0 && mo->prev1[r] < K, "%s: prev1[%d] = %d not in [0, K = %d)",
                 who, (int)r, (int)mo->prev1[r], K);
      MV_REQUIRE(mo->prev0[r] >= -1 && mo->prev0[r] < K, "%s: prev0[%d] = %d not in [-1, K = %d)",
                 who, (int)r, (int)mo->prev0[r], K);
    }
    ctx.up(vel, mo->vel, samples * DD);
    ctx.up(vel_far, mo->vel_far, samples);
    if (mo->acc) { ctx.up(acc, mo->acc, samples * DD); ctx.up(acc_far, mo->acc_far, samples); }
    ctx.up(motion_prev1, mo->prev1, rows);
    ctx.up(motion_prev0, mo->prev0, rows);
    mv::MotionRow& m = terms.mo;
    m.vel = vel.p; m.vel_far = vel_far.p;
    m.acc = mo->acc ? acc.p : nullptr; m.acc_far = mo->acc ? acc_far.p : nullptr;
    m.prev1 = motion_prev1.p; m.prev0 = motion_prev0.p;
    m.W = mo->W; m.radius = mo->radius;
  }

  // the rows' visited sets go up packed from the op's byte planes into the device's lane-major
  // words (kernels_misc.h RevisitRow: bit j of word l = cell l + 64 j).  The stored sets start as
  // the given ones, so that a row the step does not run reports its set as given.
  void up_revisit(OpCtx& ctx, const mv_step_revisit* rv, size_t samples, const char* who) {
    MV_REQUIRE(rv && rv->cost && rv->prev1, "%s: NULL revisit, cost or prev1", who);
    require_row_fits_wave(who, K);
    for (size_t n = 0; n < samples; ++n)
      MV_REQUIRE(std::isfinite(rv->cost[n]), "%s: cost[n = %d] = %g is not finite", who, (int)n,
                 (double)rv->cost[n]);
    for (size_t r = 0; r < rows; ++r)
      MV_REQUIRE(rv->prev1[r] >= 0 && rv->prev1[r] < K, "%s: prev1[%d] = %d not in [0, K = %d)",
                 who, (int)r, (int)rv->prev1[r], K);
    revisit = rv;
    words.assign(rows * 64, 0u);
    if (rv->visited)
      for (size_t r = 0; r < rows; ++r)
        for (int k = 0; k < K; ++k)
          if (rv->visited[r * K + k]) words[r * 64 + (k & 63)] |= 1u << (k >> 6);
    ctx.up(cost, rv->cost, samples);
    ctx.up(revisit_prev1, rv->prev1, rows);
    ctx.up(set_in, words.data(), rows * 64);
    ctx.up(set_out, words.data(), rows * 64);
    terms.rv.cost = cost.p;
    terms.rv.prev1 = revisit_prev1.p;
    terms.rv.set_in = set_in.p;
    terms.rv.set_out = set_out.p;
  }

  // the sets the step stored, unpacked into visited_out (where a revisit cost went up and asks)
  void down(OpCtx& ctx) {
    if (!revisit || !revisit->visited_out) return;
    ctx.down(words.data(), set_out, rows * 64);
    for (size_t r = 0; r < rows; ++r)
      for (int k = 0; k < K; ++k)
        revisit->visited_out[r * K + k] = (words[r * 64 + (k & 63)] >> (k >> 6)) & 1u;
  }
};

static int op_beam_step(int device, const float* logits, const float* prev_logprob,
                        int32_t N, int32_t B, int32_t K, int32_t time, int32_t diverse,
                        float gamma, int32_t fix_num_timestep, float* new_logprob,
                        int32_t* ids, int32_t* parents, const char* who, OpNeeds needs,
                        const uint8_t* allowed = nullptr, const float* bias = nullptr,
                        const mv_step_motion* motion = nullptr,
                        const mv_step_revisit* revisit = nullptr) {
  return guarded(nullptr, [&] {
    OpCtx ctx(device);
    OpStepTerms st;
    st.up(ctx, allowed, bias, motion, revisit, needs, (size_t)N, (size_t)N * B, K, who);
    ensure_beam_step_lds(device, beam_step_lds_bytes(B, K));
    DevBuf<float> dl, dp, dn;
    DevBuf<int32_t> di, dpa;
    ctx.up(dl, logits, (size_t)N * B * K);
    ctx.up(dp, prev_logprob, (size_t)N * B);
    dn.alloc((size_t)N * B); di.alloc((size_t)N * B); dpa.alloc((size_t)N * B);
    DevBuf<float> dc;
    dc.alloc((size_t)N * B * K);
    launch_beam_step(ctx.stream, dl.p, dp.p, dc.p, N, B, K, time, diverse, logf(gamma),
                     fix_num_timestep, dn.p, di.p, dpa.p, (int32_t*)nullptr, B, nullptr, st.terms);
    ctx.down(new_logprob, dn, (size_t)N * B);
    ctx.down(ids, di, (size_t)N * B);
    ctx.down(parents, dpa, (size_t)N * B);
    st.down(ctx);
  });
}

int mv_op_beam_step(int device, const float* logits, const float* prev_logprob,
                    int32_t N, int32_t B, int32_t K, int32_t time, int32_t diverse,
                    float gamma, int32_t fix_num_timestep, float* new_logprob,
                    int32_t* ids, int32_t* parents) {
  return op_beam_step(device, logits, prev_logprob, N, B, K, time, diverse, gamma,
                      fix_num_timestep, new_logprob, ids, parents,
                      "mv_op_beam_step", OpNeeds::Nothing);
}

int mv_op_beam_step_masked(int device, const float* logits, const float* prev_logprob,
                           const uint8_t* allowed, int32_t N, int32_t B, int32_t K, int32_t time,
                           int32_t diverse, float gamma, int32_t fix_num_timestep,
                           float* new_logprob, int32_t* ids, int32_t* parents) {
  return op_beam_step(device, logits, prev_logprob, N, B, K, time, diverse, gamma,
                      fix_num_timestep, new_logprob, ids, parents,
                      "mv_op_beam_step_masked", OpNeeds::Allowed, allowed);
}

int mv_op_beam_step_biased(int device, const float* logits, const float* prev_logprob,
                           const uint8_t* allowed, const float* bias, int32_t N, int32_t B,
                           int32_t K, int32_t time, int32_t diverse, float gamma,
                           int32_t fix_num_timestep, float* new_logprob, int32_t* ids,
                           int32_t* parents) {
  return op_beam_step(device, logits, prev_logprob, N, B, K, time, diverse, gamma,
                      fix_num_timestep, new_logprob, ids, parents,
                      "mv_op_beam_step_biased", OpNeeds::Bias, allowed, bias);
}

int mv_op_beam_step_motion(int device, const float* logits, const float* prev_logprob,
                           const uint8_t* allowed, const float* bias, const mv_step_motion* motion,
                           int32_t N, int32_t B, int32_t K, int32_t time, int32_t diverse,
                           float gamma, int32_t fix_num_timestep, float* new_logprob, int32_t* ids,
                           int32_t* parents) {
  return op_beam_step(device, logits, prev_logprob, N, B, K, time, diverse, gamma,
                      fix_num_timestep, new_logprob, ids, parents,
                      "mv_op_beam_step_motion", OpNeeds::Motion, allowed, bias, motion);
}

int mv_op_beam_step_path(int device, const float* logits, const float* prev_logprob,
                         const uint8_t* allowed, const float* bias, const mv_step_motion* motion,
                         const mv_step_revisit* revisit, int32_t N, int32_t B, int32_t K,
                         int32_t time, int32_t diverse, float gamma, int32_t fix_num_timestep,
                         float* new_logprob, int32_t* ids, int32_t* parents) {
  return op_beam_step(device, logits, prev_logprob, N, B, K, time, diverse, gamma,
                      fix_num_timestep, new_logprob, ids, parents,
                      "mv_op_beam_step_path", OpNeeds::Revisit, allowed, bias, motion, revisit);
}

static int op_sbs_step(int device, const float* logits, const float* prev_phi,
                       const float* prev_logprob, const float* prev_gumbel, int32_t N, int32_t B,
                       int32_t K, int32_t t, float temperature, uint32_t seed, float* new_phi,
                       float* new_logprob, float* new_gumbel, int32_t* ids, int32_t* parents,
                       const char* who, OpNeeds needs, const uint8_t* allowed = nullptr,
                       const float* bias = nullptr, const mv_step_motion* motion = nullptr,
                       const mv_step_revisit* revisit = nullptr) {
  return guarded(nullptr, [&] {
    MV_REQUIRE(N > 0 && B > 0 && K > 0 && t >= 0, "mv_op_sbs_step: N, B, K > 0 and t >= 0");
    MV_REQUIRE(temperature > 0.f, "mv_op_sbs_step: temperature %g must be > 0",
               (double)temperature);
    OpCtx ctx(device);
    OpStepTerms st;
    st.up(ctx, allowed, bias, motion, revisit, needs, (size_t)N, (size_t)N * B, K, who);
    ensure_beam_step_lds(device, beam_step_lds_bytes(B, K));
    const size_t R = (size_t)N * B;
    DevBuf<float> dl, dphi, dlp, dg, nphi, nlp, ng, cand, lpp, qp;
    DevBuf<int32_t> di, dpa;
    DevBuf<uint32_t> dprm;
    const uint32_t params[4] = {seed, __builtin_bit_cast(uint32_t, temperature), 0u,
                                __builtin_bit_cast(uint32_t, 1.f)};       // limits off
    ctx.up(dl, logits, R * K);
    ctx.up(dphi, prev_phi, R); ctx.up(dlp, prev_logprob, R); ctx.up(dg, prev_gumbel, R);
    ctx.up(dprm, params, (size_t)4);
    nphi.alloc(R); nlp.alloc(R); ng.alloc(R); di.alloc(R); dpa.alloc(R);
    cand.alloc(R * K); lpp.alloc(R * K); qp.alloc(R * K);
    launch_sbs_step(ctx.stream, dl.p, dphi.p, dlp.p, dg.p, cand.p, lpp.p, qp.p, dprm.p, N, B, K,
                    t, nphi.p, nlp.p, ng.p, di.p, dpa.p, (int32_t*)nullptr, B, nullptr, st.terms);
    ctx.down(new_phi, nphi, R); ctx.down(new_logprob, nlp, R); ctx.down(new_gumbel, ng, R);
    ctx.down(ids, di, R); ctx.down(parents, dpa, R);
    st.down(ctx);
  });
}

int mv_op_sbs_step(int device, const float* logits, const float* prev_phi,
                   const float* prev_logprob, const float* prev_gumbel, int32_t N, int32_t B,
                   int32_t K, int32_t t, float temperature, uint32_t seed, float* new_phi,
                   float* new_logprob, float* new_gumbel, int32_t* ids, int32_t* parents) {
  return op_sbs_step(device, logits, prev_phi, prev_logprob, prev_gumbel, N, B, K, t, temperature,
                     seed, new_phi, new_logprob, new_gumbel, ids, parents,
                     "mv_op_sbs_step", OpNeeds::Nothing);
}

int mv_op_sbs_step_masked(int device, const float* logits, const float* prev_phi,
                          const float* prev_logprob, const float* prev_gumbel,
                          const uint8_t* allowed, int32_t N, int32_t B, int32_t K, int32_t t,
                          float temperature, uint32_t seed, float* new_phi, float* new_logprob,
                          float* new_gumbel, int32_t* ids, int32_t* parents) {
  return op_sbs_step(device, logits, prev_phi, prev_logprob, prev_gumbel, N, B, K, t, temperature,
                     seed, new_phi, new_logprob, new_gumbel, ids, parents,
                     "mv_op_sbs_step_masked", OpNeeds::Allowed, allowed);
}

int mv_op_sbs_step_biased(int device, const float* logits, const float* prev_phi,
                          const float* prev_logprob, const float* prev_gumbel,
                          const uint8_t* allowed, const float* bias, int32_t N, int32_t B,
                          int32_t K, int32_t t, float temperature, uint32_t seed, float* new_phi,
                          float* new_logprob, float* new_gumbel, int32_t* ids, int32_t* parents) {
  return op_sbs_step(device, logits, prev_phi, prev_logprob, prev_gumbel, N, B, K, t, temperature,
                     seed, new_phi, new_logprob, new_gumbel, ids, parents,
                     "mv_op_sbs_step_biased", OpNeeds::Bias, allowed, bias);
}

int mv_op_sbs_step_motion(int device, const float* logits, const float* prev_phi,
                          const float* prev_logprob, const float* prev_gumbel,
                          const uint8_t* allowed, const float* bias, const mv_step_motion* motion,
                          int32_t N, int32_t B, int32_t K, int32_t t, float temperature,
                          uint32_t seed, float* new_phi, float* new_logprob, float* new_gumbel,
                          int32_t* ids, int32_t* parents) {
  return op_sbs_step(device, logits, prev_phi, prev_logprob, prev_gumbel, N, B, K, t, temperature,
                     seed, new_phi, new_logprob, new_gumbel, ids, parents,
                     "mv_op_sbs_step_motion", OpNeeds::Motion, allowed, bias, motion);
}

int mv_op_sbs_step_path(int device, const float* logits, const float* prev_phi,
                        const float* prev_logprob, const float* prev_gumbel,
                        const uint8_t* allowed, const float* bias, const mv_step_motion* motion,
                        const mv_step_revisit* revisit, int32_t N, int32_t B, int32_t K, int32_t t,
                        float temperature, uint32_t seed, float* new_phi, float* new_logprob,
                        float* new_gumbel, int32_t* ids, int32_t* parents) {
  return op_sbs_step(device, logits, prev_phi, prev_logprob, prev_gumbel, N, B, K, t, temperature,
                     seed, new_phi, new_logprob, new_gumbel, ids, parents,
                     "mv_op_sbs_step_path", OpNeeds::Revisit, allowed, bias, motion, revisit);
}

static int op_sample_step(int device, const float* logits, int32_t R, int32_t S, int32_t K,
                          int32_t t, float temperature, uint32_t seed, int32_t top_k, float top_p,
                          int32_t floor, int32_t* ids, float* lp, float* qlp, uint8_t* keep,
                          const char* who, OpNeeds needs, const uint8_t* allowed = nullptr,
                          const float* bias = nullptr, const mv_step_motion* motion = nullptr,
                          const mv_step_revisit* revisit = nullptr) {
  return guarded(nullptr, [&] {
    MV_REQUIRE(R > 0 && S > 0 && K > 0 && t >= 0, "mv_op_sample_step: R, S, K > 0 and t >= 0");
    MV_REQUIRE(R % S == 0, "mv_op_sample_step: R = %d rows are not S = %d futures per sample",
               (int)R, (int)S);
    require_row_fits_wave(needs >= OpNeeds::Motion ? who : "mv_op_sample_step", K);
    MV_REQUIRE(temperature > 0.f, "mv_op_sample_step: temperature %g must be > 0",
               (double)temperature);
    MV_REQUIRE(top_k >= 0, "mv_op_sample_step: top_k %d must be >= 0 (0 = off)", (int)top_k);
    MV_REQUIRE(top_p > 0.f && top_p <= 1.f, "mv_op_sample_step: top_p %g not in (0, 1] (1 = off)",
               (double)top_p);
    MV_REQUIRE(floor >= 1, "mv_op_sample_step: floor %d must be >= 1", (int)floor);
    OpCtx ctx(device);
    OpStepTerms st;
    st.up(ctx, allowed, bias, motion, revisit, needs, (size_t)(R / S), (size_t)R, K, who);
    DevBuf<float> dl, dlp, dq;
    DevBuf<int32_t> di;
    DevBuf<uint8_t> dk;
    DevBuf<uint32_t> dprm;
    const uint32_t params[4] = {seed, __builtin_bit_cast(uint32_t, temperature), (uint32_t)top_k,
                                __builtin_bit_cast(uint32_t, top_p)};
    ctx.up(dl, logits, (size_t)R * K);
    ctx.up(dprm, params, (size_t)4);
    dlp.alloc(R); dq.alloc(R); di.alloc(R); dk.alloc((size_t)R * K);
    HIP_CHECK(hipMemsetAsync(dlp.p, 0, (size_t)R * sizeof(float), ctx.stream));
    HIP_CHECK(hipMemsetAsync(dq.p, 0, (size_t)R * sizeof(float), ctx.stream));
    launch_sample_step(ctx.stream, dl.p, (int64_t)K, R, S, K, t, 0, dprm.p, floor,
                       (const int32_t*)nullptr, dlp.p, dq.p, di.p, 1, (int32_t*)nullptr, dk.p,
                       st.terms);
    HIP_CHECK(hipGetLastError());
    ctx.down(ids, di, R); ctx.down(lp, dlp, R); ctx.down(qlp, dq, R);
    ctx.down(keep, dk, (size_t)R * K);
    st.down(ctx);
  });
}

int mv_op_sample_step(int device, const float* logits, int32_t R, int32_t S, int32_t K, int32_t t,
                      float temperature, uint32_t seed, int32_t top_k, float top_p, int32_t floor,
                      int32_t* ids, float* lp, float* qlp, uint8_t* keep) {
  return op_sample_step(device, logits, R, S, K, t, temperature, seed, top_k, top_p, floor, ids, lp,
                        qlp, keep, "mv_op_sample_step", OpNeeds::Nothing);
}

int mv_op_sample_step_masked(int device, const float* logits, const uint8_t* allowed, int32_t R,
                             int32_t S, int32_t K, int32_t t, float temperature, uint32_t seed,
                             int32_t top_k, float top_p, int32_t floor, int32_t* ids, float* lp,
                             float* qlp, uint8_t* keep) {
  return op_sample_step(device, logits, R, S, K, t, temperature, seed, top_k, top_p, floor, ids, lp,
                        qlp, keep, "mv_op_sample_step_masked", OpNeeds::Allowed, allowed);
}

int mv_op_sample_step_biased(int device, const float* logits, const uint8_t* allowed,
                             const float* bias, int32_t R, int32_t S, int32_t K, int32_t t,
                             float temperature, uint32_t seed, int32_t top_k, float top_p,
                             int32_t floor, int32_t* ids, float* lp, float* qlp, uint8_t* keep) {
  return op_sample_step(device, logits, R, S, K, t, temperature, seed, top_k, top_p, floor, ids, lp,
                        qlp, keep, "mv_op_sample_step_biased", OpNeeds::Bias, allowed, bias);
}

int mv_op_sample_step_motion(int device, const float* logits, const uint8_t* allowed,
                             const float* bias, const mv_step_motion* motion, int32_t R, int32_t S,
                             int32_t K, int32_t t, float temperature, uint32_t seed, int32_t top_k,
                             float top_p, int32_t floor, int32_t* ids, float* lp, float* qlp,
                             uint8_t* keep) {
  return op_sample_step(device, logits, R, S, K, t, temperature, seed, top_k, top_p, floor, ids, lp,
                        qlp, keep,
                        "mv_op_sample_step_motion", OpNeeds::Motion, allowed, bias, motion);
}

int mv_op_sample_step_path(int device, const float* logits, const uint8_t* allowed,
                           const float* bias, const mv_step_motion* motion,
                           const mv_step_revisit* revisit, int32_t R, int32_t S, int32_t K,
                           int32_t t, float temperature, uint32_t seed, int32_t top_k, float top_p,
                           int32_t floor, int32_t* ids, float* lp, float* qlp, uint8_t* keep) {
  return op_sample_step(device, logits, R, S, K, t, temperature, seed, top_k, top_p, floor, ids, lp,
                        qlp, keep,
                        "mv_op_sample_step_path", OpNeeds::Revisit, allowed, bias, motion, revisit);
}

int mv_enc_cone_build(const int32_t* labels, int32_t N, int32_t T, int32_t H, int32_t W,
                      int32_t r0, int32_t* lists, int64_t* cells) {
  if (N <= 0 || T <= 0 || H <= 0 || W <= 0 || W > 32 || r0 < 0) return -1;
  if (lists) {
    if (!labels) return -1;
    for (size_t i = 0; i < (size_t)N * T; ++i)
      if (labels[i] < 0 || labels[i] >= H * W) return -1;
    build_enc_cone(labels, N, T, H, W, r0, lists, cells);
  }
  return enc_cone_tiles(N + 1, H, W);
}

// ---- the scene stack's convolution in either of its forms (tests/test_gpu_helper_forms.py)

int mv_scene_conv_form(int32_t k, int32_t Ci, int32_t Co) {
  return (int)scene_conv_form(k, Ci, Co);
}

int mv_op_scene_conv(int device, int32_t form, const float* in, const float* w, const float* b,
                     int32_t U, int32_t Hi, int32_t Wi, int32_t Ci, int32_t Co, int32_t k,
                     int32_t act, float* out) {
  return guarded(nullptr, [&] {
    MV_REQUIRE(in && w && b && out, "mv_op_scene_conv: NULL argument");
    MV_REQUIRE(U >= 1 && Hi >= 1 && Wi >= 1 && Ci >= 1 && Co >= 1 && k >= 1,
               "mv_op_scene_conv: bad shape");
    MV_REQUIRE(act >= 0 && act <= 2, "mv_op_scene_conv: activation %d", (int)act);
    MV_REQUIRE(form == 0 || form == 1, "mv_op_scene_conv: form %d (0 = the plan's, 1 = one thread "
               "per output)", (int)form);
    const SceneConvForm f = form == 1 ? SceneConvForm::PerOutput : scene_conv_form(k, Ci, Co);
    OpCtx ctx(device);
    const int Ho = (Hi + 1) / 2, Wo = (Wi + 1) / 2;      // SAME, stride 2
    const int pad_h = std::max((Ho - 1) * 2 + k - Hi, 0), pad_w = std::max((Wo - 1) * 2 + k - Wi, 0);
    DevBuf<float> di, dw, db, dout;
    ctx.up(di, in, (size_t)U * Hi * Wi * Ci);
    ctx.up(dw, w, (size_t)k * k * Ci * Co);
    ctx.up(db, b, (size_t)Co);
    const size_t total = (size_t)U * Ho * Wo * Co;
    dout.alloc(total);
    launch_scene_conv(ctx.stream, f, di.p, dw.p, db.p, dout.p, U, Hi, Wi, Ci, Ho, Wo, Co, k,
                      pad_h / 2, pad_w / 2, act);
    HIP_CHECK(hipGetLastError());
    ctx.down(out, dout, total);
  });
}

// ---- the decoder tail of one step in either of its forms (tests/test_gpu_decode_tail.py):
// grouped through the engine's own pack_h2g_kernel, launch_h2g_q and launch_decode_tail on
// problems filled by run_tail's helpers, or the separate tail's kernels chain by chain

namespace {
struct TailChainDev {
  DevBuf<float> h, w, wq, q, ew, eb, out, x, hot;
  DevBuf<int32_t> ids;
  DevBuf<_Float16> pl;
  _Float16* p0 = nullptr;       // plane 0 (null: no planes) and the stride the kernels are given
  size_t pst = 0;
};
constexpr int kOpSentinel = 0xA5;     // the byte every output buffer holds before the launches
}  // namespace

int mv_op_decode_tail(int device, int32_t form, int32_t next, int32_t planes, int32_t C,
                      int32_t E, int32_t act, const mv_tail_chain* chains, int32_t n) {
  return guarded(nullptr, [&] {
    MV_REQUIRE(chains && n >= 1 && n <= mv::kTailMax, "mv_op_decode_tail: 1 to %d chains, not %d",
               mv::kTailMax, (int)n);
    MV_REQUIRE(C == 128 || C == 256 || C == 512, "mv_op_decode_tail: C %d not 128, 256 or 512",
               (int)C);
    MV_REQUIRE(E >= 16 && E % 16 == 0, "mv_op_decode_tail: E %d must be a multiple of 16", (int)E);
    MV_REQUIRE(act >= 0 && act <= 2, "mv_op_decode_tail: activation %d", (int)act);
    MV_REQUIRE(form >= 0 && form <= 3, "mv_op_decode_tail: form %d (0 grouped, 1 separate, 2 "
               "separate with the 8-channel one-hot embedding, 3 separate with the dense embedding "
               "of the one-hot map)", (int)form);
    MV_REQUIRE(next >= 0 && next <= 2, "mv_op_decode_tail: next %d (0 none, 1 ids only, 2 ids and "
               "embedding)", (int)next);
    MV_REQUIRE(planes >= 0 && planes <= 2, "mv_op_decode_tail: planes %d (0 none, 1 f16x3, 2 bf16)",
               (int)planes);
    // every refusal comes before the first launch
    for (int i = 0; i < n; ++i) {
      const mv_tail_chain& ch = chains[i];
      MV_REQUIRE(ch.rows >= 1 && ch.H >= 1 && ch.W >= 1 && (ch.kind == 0 || ch.kind == 1),
                 "mv_op_decode_tail: chain %d: bad shape or kind", i);
      MV_REQUIRE((int64_t)ch.rows * ch.H * ch.W * std::max(C, E) < ((int64_t)1 << 31),
                 "mv_op_decode_tail: chain %d: too large for an op call", i);
      MV_REQUIRE(ch.h && ch.w_out && ch.out, "mv_op_decode_tail: chain %d: NULL h, w_out or out", i);
      MV_REQUIRE(next < 2 || (ch.emb_w && ch.emb_b), "mv_op_decode_tail: chain %d: next == 2 "
                 "needs emb_w and emb_b", i);
      if (form == 0) require_tail_fits(E, ch.H * ch.W);
      if (ch.planes) {
        const int64_t want = 2 * ((int64_t)ch.rows * ch.H * ch.W * E + (int64_t)mv::kPlaneSlack +
                                  mv::kPlanePad);
        MV_REQUIRE(ch.planes_elems == want, "mv_op_decode_tail: chain %d: planes_elems %lld, the "
                   "engine allocates %lld", i, (long long)ch.planes_elems, (long long)want);
      }
    }
    OpCtx ctx(device);
    TailChainDev dv[mv::kTailMax];
    for (int i = 0; i < n; ++i) {
      const mv_tail_chain& ch = chains[i];
      TailChainDev& d = dv[i];
      const int P = ch.kind == 0 ? 1 : 2;
      const size_t cells = (size_t)ch.rows * ch.H * ch.W;
      ctx.up(d.h, ch.h, cells * C);
      ctx.up(d.w, ch.w_out, (size_t)9 * C * P);
      if (ch.emb_w) ctx.up(d.ew, ch.emb_w, (size_t)9 * P * E);
      if (ch.emb_b) ctx.up(d.eb, ch.emb_b, (size_t)E);
      d.out.alloc(cells * P); d.x.alloc(cells * E); d.ids.alloc(ch.rows);
      HIP_CHECK(hipMemsetAsync(d.out.p, kOpSentinel, cells * P * sizeof(float), ctx.stream));
      HIP_CHECK(hipMemsetAsync(d.x.p, kOpSentinel, cells * E * sizeof(float), ctx.stream));
      HIP_CHECK(hipMemsetAsync(d.ids.p, kOpSentinel, ch.rows * sizeof(int32_t), ctx.stream));
      if (ch.planes) {     // [pad | plane 0 | slack][pad | plane 1 | slack], as mv_create lays it out
        const size_t pst = cells * E + mv::kPlaneSlack + mv::kPlanePad;
        d.pl.alloc(2 * pst);
        HIP_CHECK(hipMemsetAsync(d.pl.p, kOpSentinel, 2 * pst * sizeof(_Float16), ctx.stream));
        if (planes != 0 && next == 2) {
          d.p0 = d.pl.p + mv::kPlanePad;
          d.pst = planes == 2 ? 0 : pst;        // bf16: the single plane (stride 0)
        }
      }
    }
    if (form == 0) {
      std::vector<mv::H2gQProblem> qp;
      std::vector<mv::TailProblem> tp;
      for (int i = 0; i < n; ++i) {
        const mv_tail_chain& ch = chains[i];
        TailChainDev& d = dv[i];
        const bool cls = ch.kind == 0;
        const int P = cls ? 1 : 2, K = ch.H * ch.W;
        d.wq.alloc((size_t)C * 32); d.q.alloc((size_t)ch.rows * K * 9 * P);
        hipLaunchKernelGGL(mv::pack_h2g_kernel, dim3(cdiv((size_t)C * 32, 256)), dim3(256), 0,
                           ctx.stream, d.w.p, d.wq.p, C, P);
        qp.push_back(mv::H2gQProblem{d.h.p, d.wq.p, d.q.p, (int32_t)(ch.rows * K), P});
        mv::TailProblem a = tail_problem(d.q.p, d.out.p, (int64_t)K * P, ch.rows, ch.H, ch.W, cls,
                                         E, act);
        if (cls && next >= 1) a.ids_out = d.ids.p;
        if (next == 2) tail_embed(a, d.ew.p, d.eb.p, d.x.p, d.p0, d.pst);
        tp.push_back(a);
      }
      mv::launch_h2g_q(qp.data(), n, C, ctx.stream);
      mv::launch_decode_tail(tp.data(), n, ctx.stream);
      HIP_CHECK(hipGetLastError());
    } else {
      for (int i = 0; i < n; ++i) {
        const mv_tail_chain& ch = chains[i];
        TailChainDev& d = dv[i];
        const bool cls = ch.kind == 0;
        const int K = ch.H * ch.W;
        const size_t cells = (size_t)ch.rows * K, total = cells * E;
        if (cls)
          hipLaunchKernelGGL(mv::hidden2grid_kernel<1>, dim3(cdiv(cells, 4)), dim3(256), 0,
                             ctx.stream, d.h.p, d.w.p, d.out.p, (size_t)K, ch.rows, ch.H, ch.W, C);
        else
          hipLaunchKernelGGL(mv::hidden2grid_kernel<2>, dim3(cdiv(cells, 4)), dim3(256), 0,
                             ctx.stream, d.h.p, d.w.p, d.out.p, (size_t)K * 2, ch.rows, ch.H, ch.W,
                             C);
        if (cls && next >= 1)
          hipLaunchKernelGGL(mv::argmax_rows_kernel, dim3(ch.rows), dim3(64), 0, ctx.stream,
                             d.out.p, (size_t)K, d.ids.p, ch.rows, K);
        HIP_CHECK(hipGetLastError());
        if (next < 2) continue;
        if (!cls) {
          hipLaunchKernelGGL(mv::grid_emb_dense_kernel, dim3(cdiv(total, 256)), dim3(256), 0,
                             ctx.stream, d.out.p, (size_t)K * 2, d.ew.p, d.eb.p, d.x.p, ch.rows,
                             ch.H, ch.W, 2, E, d.p0, d.pst, act);
        } else if (form == 1) {
          hipLaunchKernelGGL(mv::grid_emb_onehot_kernel, dim3(cdiv(total, 256)), dim3(256), 0,
                             ctx.stream, d.ids.p, 1, 1, d.ew.p, d.eb.p, d.x.p, ch.rows, ch.H, ch.W,
                             E, d.p0, d.pst, act);
        } else if (form == 2) {
          hipLaunchKernelGGL(mv::grid_emb_onehot8_kernel, dim3(cdiv(total / 8, 256)), dim3(256), 0,
                             ctx.stream, d.ids.p, 1, 1, d.ew.p, d.eb.p, d.x.p, ch.rows, ch.H, ch.W,
                             E, d.p0, d.pst, act);
        } else {           // the literal one-hot map of the ids through the dense kernel, P = 1
          std::vector<int32_t> hid(ch.rows);
          ctx.down(hid.data(), d.ids, (size_t)ch.rows);
          std::vector<float> hot(cells, 0.f);
          for (int r = 0; r < ch.rows; ++r) {
            MV_REQUIRE(hid[r] >= 0 && hid[r] < K, "mv_op_decode_tail: argmax %d of row %d is "
                       "outside the grid", (int)hid[r], r);
            hot[(size_t)r * K + hid[r]] = 1.f;
          }
          ctx.up(d.hot, hot.data(), cells);
          hipLaunchKernelGGL(mv::grid_emb_dense_kernel, dim3(cdiv(total, 256)), dim3(256), 0,
                             ctx.stream, d.hot.p, (size_t)K, d.ew.p, d.eb.p, d.x.p, ch.rows, ch.H,
                             ch.W, 1, E, d.p0, d.pst, act);
        }
        HIP_CHECK(hipGetLastError());
      }
    }
    for (int i = 0; i < n; ++i) {
      const mv_tail_chain& ch = chains[i];
      const size_t cells = (size_t)ch.rows * ch.H * ch.W;
      ctx.down(ch.out, dv[i].out, cells * (ch.kind == 0 ? 1 : 2));
      if (ch.ids) ctx.down(ch.ids, dv[i].ids, (size_t)ch.rows);
      if (ch.x) ctx.down(ch.x, dv[i].x, cells * E);
      if (ch.planes)
        ctx.down(reinterpret_cast<_Float16*>(ch.planes), dv[i].pl, (size_t)ch.planes_elems);
    }
  });
}

int mv_op_convlstm_bwd(int device, const float* x, const float* c, const float* h,
                       const float* kernel, const float* biases, const float* dh_new,
                       const float* dc_new, int32_t M, int32_t H, int32_t W, int32_t Cx,
                       int32_t C, float* dx, float* dh, float* dc, float* dkernel,
                       float* dbiases) {
  return guarded(nullptr, [&] {
    MV_REQUIRE(C % 128 == 0 && C <= 512, "convlstm_bwd: C 128, 256, 384 or 512");
    MV_REQUIRE(mv::convlstm_cx_supported(Cx), "Cx %d unsupported", Cx);
    OpCtx ctx(device);
    const size_t cells = (size_t)M * H * W;
    DevBuf<float> dx_, dc_, dh_, dw, db, dco, dho, dg, ddh, ddc, dwd, dxo, dho2, part, dW,
        dB, tmp;
    dx_.alloc(cells * Cx ? cells * Cx : 1, mv::kWgradPad);
    if (cells * Cx)
      HIP_CHECK(hipMemcpy(dx_.p, x, cells * Cx * sizeof(float), hipMemcpyHostToDevice));
    ctx.up(db, biases, (size_t)4 * C);
    std::vector<float> packed(mv::convlstm_wpack_elems(Cx, C));
    mv::pack_convlstm_weights(kernel, Cx, C, packed.data());
    ctx.up(dw, packed.data(), packed.size());
    std::vector<float> packedT(mv::convlstm_dgrad_wpack_elems(Cx, C));
    mv::pack_convlstm_dgrad_weights(kernel, Cx, C, packedT.data());
    ctx.up(dwd, packedT.data(), packedT.size());
    const bool zero = (c == nullptr && h == nullptr);
    dc_.alloc(cells * C); dh_.alloc(cells * C, mv::kWgradPad);
    if (!zero) {
      MV_REQUIRE(c && h, "c and h must both be given or both be NULL");
      HIP_CHECK(hipMemcpy(dc_.p, c, cells * C * sizeof(float), hipMemcpyHostToDevice));
      HIP_CHECK(hipMemcpy(dh_.p, h, cells * C * sizeof(float), hipMemcpyHostToDevice));
    } else {
      HIP_CHECK(hipMemset(dc_.p, 0, cells * C * sizeof(float)));
      HIP_CHECK(hipMemset(dh_.p, 0, cells * C * sizeof(float)));
    }
    dco.alloc(cells * C); dho.alloc(cells * C); dg.alloc(cells * 4 * C, mv::kWgradPad);
    ctx.up(ddh, dh_new, cells * C);
    ctx.up(ddc, dc_new, cells * C);
    // forward with saved gate activations
    mv::ConvLstmArgs a{};
    a.x = dx_.p; a.h = dh_.p; a.c = dc_.p; a.wpack = dw.p; a.bias = db.p;
    a.h_out = dho.p; a.c_out = dco.p; a.gates_out = dg.p;
    a.rows = M; a.H = H; a.W = W; a.Cx = Cx; a.C = C;
    mv::convlstm_finish_args(a, zero);
    mv::launch_convlstm_steps(&a, 1, ctx.stream);
    // pointwise backward: gates -> G in place, ddc -> d c
    const size_t total = cells * C;
    hipLaunchKernelGGL(mv::lstm_gate_bwd_kernel, dim3(cdiv(total, 256)), dim3(256), 0,
                       ctx.stream, dg.p, dc_.p, dco.p, ddh.p, ddc.p, total, C);
    // dgrad
    dxo.alloc(cells * (Cx ? Cx : 1)); dho2.alloc(cells * C);
    mv::ConvLstmArgs d{};
    mv::convlstm_dgrad_args(d, dg.p, dwd.p, dho2.p, dxo.p, M, H, W, Cx, C, true, Cx > 0);
    mv::launch_convlstm_dgrads(&d, 1, ctx.stream);
    // wgrad (device-side packs are checked against the host packs on the way)
    const WgradPlan wpl = plan_wgrad(0, 3, M, H, W, Cx, C);
    mv::WgradArgs wa = wpl.fp32;
    wa.x = Cx ? dx_.p : nullptr; wa.h = dh_.p; wa.g = dg.p;
    part.alloc(wpl.partial_elems);
    wa.partial = part.p;
    mv::launch_convlstm_wgrad(wa, ctx.stream);
    const size_t ncols = (size_t)9 * (Cx + C) * 4 * C;
    dW.alloc(ncols);
    hipLaunchKernelGGL(mv::colsum_kernel, dim3(1, cdiv(ncols, 256)), dim3(256), 0,
                       ctx.stream, part.p, dW.p, (size_t)wa.nsplit, ncols,
                       (size_t)wa.nsplit);
    dB.alloc((size_t)4 * C);
    hipLaunchKernelGGL(mv::colsum_kernel, dim3(1, cdiv((size_t)4 * C, 256)), dim3(256), 0,
                       ctx.stream, dg.p, dB.p, cells, (size_t)4 * C, cells);
    // device packs == host packs (the training step repacks on the device)
    {
      DevBuf<float> wsrc, p1, p2;
      ctx.up(wsrc, kernel, (size_t)9 * (Cx + C) * 4 * C);
      const int nx = mv::convlstm_xchunks(Cx), nch = nx + 9 * (C / mv::kBK);
      p1.alloc(packed.size()); p2.alloc(packedT.size());
      hipLaunchKernelGGL(mv::pack_fwd_kernel, dim3(cdiv(packed.size(), 256)), dim3(256), 0,
                         ctx.stream, wsrc.p, p1.p, Cx, C, nx, nch, x_is_small(Cx) ? 1 : 0,
                         packed.size());
      hipLaunchKernelGGL(mv::pack_dgrad_kernel, dim3(cdiv(packedT.size(), 256)), dim3(256),
                         0, ctx.stream, wsrc.p, p2.p, Cx, C, 9 * (4 * C / mv::kBK),
                         packedT.size());
      std::vector<float> c1(packed.size()), c2(packedT.size());
      ctx.down(c1.data(), p1, c1.size());
      ctx.down(c2.data(), p2, c2.size());
      MV_REQUIRE(memcmp(c1.data(), packed.data(), c1.size() * 4) == 0,
                 "device forward weight pack differs from the host pack");
      MV_REQUIRE(memcmp(c2.data(), packedT.data(), c2.size() * 4) == 0,
                 "device dgrad weight pack differs from the host pack");
    }
    HIP_CHECK(hipGetLastError());
    if (dx && Cx) ctx.down(dx, dxo, cells * Cx);
    ctx.down(dh, dho2, cells * C);
    ctx.down(dc, ddc, cells * C);
    ctx.down(dkernel, dW, ncols);
    ctx.down(dbiases, dB, (size_t)4 * C);
  });
}

// ---- the matrix-pipe backward of one gate convolution, kernel by kernel
// (tests/test_gpu_bwd_kernels.py): G is an INPUT, so nothing upstream of the two GEMMs rounds; the
// engine's own packs, splits, transposes, exponent kernels and launchers (run_dgrad_group_f16x3 and
// run_wgrad of engine_train.h, on one problem = one chain of one step), the form forced by the
// variant, the rest of the plan from gate_plan.h.  Every output and partial buffer holds the byte
// 0xA5 before the launches: what a kernel leaves unwritten is seen.
int mv_op_convlstm_bwd16(int device, int32_t variant_dgrad, int32_t variant_wgrad, const float* x,
                         const float* h, const float* G, const float* kernel, int32_t M,
                         int32_t H, int32_t W, int32_t Cx, int32_t C, float* dx, float* dh,
                         float* dkernel, int32_t* exps, int32_t* forms) {
  return guarded(nullptr, [&] {
    const int vd = variant_dgrad, vw = variant_wgrad;
    MV_REQUIRE(vd >= 0 && vd <= 3, "convlstm_bwd16: dgrad variant %d (0 none, 1 f16x3 direct, 2 "
               "f16x3 Winograd F(2,3), 3 bf16 one plane)", vd);
    MV_REQUIRE(vw >= 0 && vw <= 4, "convlstm_bwd16: wgrad variant %d (0 none, 1 f16x3 direct, 2 "
               "f16x3 row-triple, 3 one-plane direct, 4 one-plane row-triple)", vw);
    MV_REQUIRE(vd != 0 || vw != 0, "convlstm_bwd16: nothing to run");
    MV_REQUIRE(G && kernel && exps && forms, "convlstm_bwd16: NULL G, kernel, exps or forms");
    MV_REQUIRE(M >= 1 && H >= 1 && W >= 1 && H * W >= 32, "convlstm_bwd16: grids of at least 32 "
               "cells");
    MV_REQUIRE(C % 128 == 0 && C <= 512, "convlstm_bwd16: C 128, 256, 384 or 512");
    MV_REQUIRE(Cx >= 1 && (Cx % 16 == 0 || x_is_small(Cx)) && (Cx <= 64 || Cx % 64 == 0),
               "convlstm_bwd16: Cx %d unsupported (<= 3, 16, 32, 48, 64 or a multiple of 64)", Cx);
    MV_REQUIRE((int64_t)M * H * W * 4 * C < ((int64_t)1 << 31), "convlstm_bwd16: too large for an "
               "op call");
    MV_REQUIRE(vd == 0 || (dh && dx), "convlstm_bwd16: NULL dx or dh");
    MV_REQUIRE(vw == 0 || (x && h && dkernel), "convlstm_bwd16: NULL x, h or dkernel");
    const size_t cells = (size_t)M * H * W;
    const int N4 = 4 * C, Cin = Cx + C;
    // ---- every refusal before the first launch: the planner's conditions, by name
    mv::ConvLstmArgs da{};
    mv::convlstm_dgrad_args(da, nullptr, nullptr, nullptr, nullptr, M, H, W, Cx, C, true, true);
    if (vd == 2)
      MV_REQUIRE(wino_dgrad_geometry_ok(da), "convlstm_bwd16: wino_dgrad_geometry_ok: W %d must "
                 "divide 32, H %d >= 2, C in whole 64-column blocks, 4C / 16 a multiple of 8", W, H);
    if (vd == 3)
      MV_REQUIRE((9 * (N4 / 16) / 3) % MV_BF16_UNITS == 0, "convlstm_bwd16: bf16 dgrad stage "
                 "count %d does not fill whole LDS stages", 9 * (N4 / 16) / 3);
    if (vw != 0)
      MV_REQUIRE(mv::wgrad16_ok(W, C), "convlstm_bwd16: wgrad16_ok: W %d %% 16 == 0 and C %d %% "
                 "128 == 0", W, C);
    const bool wn = vw == 2 || vw == 4;
    if (wn)
      MV_REQUIRE(mv::wgrad16_wino3_ok(H), "convlstm_bwd16: wgrad16_wino3_ok: H %d >= 3 and a "
                 "multiple of 3", H);
    for (int i = 0; i < 3; ++i) exps[i] = 0;
    for (int i = 0; i < 8; ++i) forms[i] = 0;

    OpCtx ctx(device);
    DevBuf<float> dG, dK;
    DevBuf<int32_t> gmax, cexp;       // [64] max |G| bits; [0] G exp [1] 8 [2] x exp [64..127] max |x|
    ctx.up(dG, G, cells * N4);
    ctx.up(dK, kernel, (size_t)9 * Cin * N4);
    gmax.alloc(64); cexp.alloc(128);
    HIP_CHECK(hipMemsetAsync(gmax.p, 0, 64 * sizeof(int32_t), ctx.stream));
    HIP_CHECK(hipMemsetAsync(cexp.p, 0, 128 * sizeof(int32_t), ctx.stream));
    hipLaunchKernelGGL(mv::absmax_bits_kernel, dim3(256), dim3(256), 0, ctx.stream, dG.p,
                       cells * N4, gmax.p);

    // ------------------------------------------------------------------ dgrad
    DevBuf<float> dxo, dho, part0, part1;
    DevBuf<_Float16> g16, wd16, wdb, wdw;
    DevBuf<int32_t> gexp;
    if (vd != 0) {
      dxo.alloc(cells * Cx); dho.alloc(cells * C);
      HIP_CHECK(hipMemsetAsync(dxo.p, kOpSentinel, cells * Cx * sizeof(float), ctx.stream));
      HIP_CHECK(hipMemsetAsync(dho.p, kOpSentinel, cells * C * sizeof(float), ctx.stream));
      mv::ConvLstmArgs a{};
      mv::convlstm_dgrad_args(a, dG.p, nullptr, dho.p, dxo.p, M, H, W, Cx, C, true, true);
      const bool has_wdw = vd == 2;
      const DgradPlan pl = plan_dgrad_group(vd == 3 ? 2 : 1, &a, &has_wdw, 1);
      MV_REQUIRE(pl.bf16 == (vd == 3) && pl.wino == (vd == 2), "convlstm_bwd16: dgrad variant %d "
                 "is switched off in this process (MV_BF16_BWD, MV_WINO, MV_WINO_DGRAD)", vd);
      const bool bf = pl.bf16;
      const size_t nel = cells * a.C;                 // a.C == 4C
      const size_t pst = nel + mv::kPlaneSlack + mv::kPlanePad;
      g16.alloc(2 * pst + mv::kPlanePad);
      HIP_CHECK(hipMemsetAsync(g16.p, 0, (2 * pst + mv::kPlanePad) * sizeof(_Float16), ctx.stream));
      _Float16* p0 = g16.p + mv::kPlanePad;
      gexp.alloc(1);
      HIP_CHECK(hipMemsetAsync(gexp.p, 0, sizeof(int32_t), ctx.stream));
      if (bf) {
        hipLaunchKernelGGL(mv::split_plane_bf16_kernel, dim3(mv::split_planes_blocks(cells, a.C)),
                           dim3(256), 0, ctx.stream, a.h, p0, (int)cells, a.C);
        const size_t db = mv::bf16_dgrad_wpack_elems(Cx, C);
        wdb.alloc(db);
        hipLaunchKernelGGL(mv::pack_bf16_dgrad_kernel, dim3(cdiv(db, 256)), dim3(256), 0,
                           ctx.stream, dK.p, wdb.p, Cx, C, db);
      } else {
        hipLaunchKernelGGL(mv::split_planes_dyn_kernel, dim3(mv::split_planes_blocks(cells, a.C)),
                           dim3(256), 0, ctx.stream, a.h, p0, p0 + pst, (int)cells, a.C, gmax.p,
                           gexp.p);
        const size_t dhv = mv::f16x3_dgrad_wpack_elems(Cx, C);
        wd16.alloc(dhv);
        hipLaunchKernelGGL(mv::pack_f16x3_dgrad_kernel, dim3(cdiv(dhv / 2, 256)), dim3(256), 0,
                           ctx.stream, dK.p, wd16.p, Cx, C, dhv / 2);
        if (pl.wino) {
          const size_t dw = mv::wino_dgrad_wpack_elems(Cx, C);
          wdw.alloc(dw);
          hipLaunchKernelGGL(mv::pack_wino_dgrad_kernel, dim3(cdiv(dw / 2, 256)), dim3(256), 0,
                             ctx.stream, dK.p, wdw.p, Cx, C, dw / 2);
        }
      }
      mv::ConvLstm16Args q{};
      q.f = a;
      q.h16 = p0; q.h_plane_stride = (int64_t)pst;
      q.x16 = nullptr; q.x_plane_stride = 0;
      q.wp16 = bf ? wdb.p : wd16.p;
      q.n_xk = 0; q.n_hk = 9 * (a.C / 16); q.w_ksteps = q.n_hk;
      q.g_exp = bf ? nullptr : gexp.p;
      const DgradPlan::Slices& ks = pl.s[0];
      const int ns0 = pl.wino ? ks.nks_main : ks.n_kslice, ns1 = pl.wino ? ks.nks_x : ks.n_kslice;
      const bool need_dx = pl.wino ? ns1 > 1 : a.out1_cols > 0;
      q.n_kslice = ks.n_kslice;
      if (ns0 > 1) {
        part0.alloc((size_t)ns0 * cells * a.out0_cols);
        HIP_CHECK(hipMemsetAsync(part0.p, kOpSentinel, part0.n * sizeof(float), ctx.stream));
        q.part0 = part0.p;
      }
      if (ns1 > 1 && need_dx) {
        part1.alloc((size_t)ns1 * cells * ((a.out1_cols + 3) / 4 * 4));
        HIP_CHECK(hipMemsetAsync(part1.p, kOpSentinel, part1.n * sizeof(float), ctx.stream));
        q.part1 = part1.p;
      }
      if (pl.wino) {
        mv::ConvLstmWinoArgs w{};
        w.nks_main = ks.nks_main; w.nks_x = ks.nks_x;
        w.b = q;
        w.b.f.n_colblocks = ns1 > 1 ? mv::wino_dgrad_colblocks(a.out1_cols, a.out0_cols)
                                    : a.out0_cols / 64;
        w.wpw = wdw.p;
        w.n_xc = 0;
        mv::launch_convlstm_wino_dgrads(&w, 1, ctx.stream);
      } else {
        mv::launch_convlstm16_dgrads(&q, 1, bf, pl.shift, ctx.stream);
      }
      HIP_CHECK(hipGetLastError());
      mv::SumSlicesArgs sa{};
      unsigned blocks = 0;
      sa.nslice = 1;
      for (int o = 0; o < 2; ++o) {
        const int ns = o ? ns1 : ns0;
        if (ns <= 1) continue;
        float* out = o ? q.f.out1 : q.f.out0;
        const size_t n = cells * (size_t)(o ? q.f.out1_cols : q.f.out0_cols);
        if (!out || n == 0) continue;
        MV_REQUIRE(n % 4 == 0, "convlstm_bwd16: the dgrad slice sum needs a multiple of 4 elements");
        sa.part[sa.nseg] = o ? q.part1 : q.part0;
        sa.out[sa.nseg] = out;
        sa.n[sa.nseg] = n;
        sa.nslice_seg[sa.nseg] = ns;
        blocks += cdiv(n / 4, 256);
        sa.block_end[sa.nseg] = blocks;
        ++sa.nseg;
      }
      if (sa.nseg > 0)
        hipLaunchKernelGGL(mv::sum_slices_kernel, dim3(blocks), dim3(256), 0, ctx.stream, sa);
      HIP_CHECK(hipGetLastError());
      forms[4] = ns0; forms[5] = ns1; forms[6] = (!pl.wino && pl.shift) ? 1 : 0;
    }

    // ------------------------------------------------------------------ wgrad
    DevBuf<float> dX, dH, partial, bias_part, dW;
    DevBuf<_Float16> gt16, at16[3], xt16[3];
    const size_t ncols = (size_t)9 * Cin * N4;
    if (vw != 0) {
      ctx.up(dX, x, cells * Cx);
      ctx.up(dH, h, cells * C);
      const WgradPlan pl = plan_wgrad(vw >= 3 ? 2 : 1, 3, M, H, W, Cx, C, wn ? 1 : 0);
      MV_REQUIRE(pl.f16 && pl.one == (vw >= 3) && pl.wino == wn && pl.nsplit_x <= pl.nsplit,
                 "convlstm_bwd16: wgrad variant %d is switched off in this process (MV_BF16_BWD)",
                 vw);
      const int npl = pl.one ? 1 : 2;
      const size_t pl_cells = pl.wino ? 5 * ((size_t)pl.Mrow3 + 64) : (size_t)pl.Mrow;
      auto zalloc = [&](DevBuf<_Float16>& b, size_t n) {
        b.alloc(n);
        HIP_CHECK(hipMemsetAsync(b.p, 0, n * sizeof(_Float16), ctx.stream));
      };
      zalloc(gt16, (size_t)2 * N4 * pl_cells);
      for (int d = 0; d < 3; ++d) zalloc(at16[d], (size_t)2 * C * pl_cells);
      for (int d = 0; d < 3; ++d) zalloc(xt16[d], (size_t)2 * std::max(64, Cx) * pl_cells);
      bias_part.alloc((size_t)(pl.Mrow / 64) * N4);
      partial.alloc(pl.partial_elems);
      HIP_CHECK(hipMemsetAsync(partial.p, kOpSentinel, pl.partial_elems * sizeof(float), ctx.stream));
      dW.alloc(ncols);
      HIP_CHECK(hipMemsetAsync(dW.p, kOpSentinel, ncols * sizeof(float), ctx.stream));
      { const int32_t eight = 8;
        HIP_CHECK(hipMemcpyAsync(cexp.p + 1, &eight, sizeof(eight), hipMemcpyHostToDevice,
                                 ctx.stream));
        HIP_CHECK(hipStreamSynchronize(ctx.stream)); }
      wgrad16_set_attributes();
      hipLaunchKernelGGL(mv::chain_exp_kernel, dim3(1), dim3(64), 0, ctx.stream, gmax.p, 1, 64,
                         cexp.p);
      if (pl.wino)
        hipLaunchKernelGGL(mv::wino3_transpose_g_kernel, dim3((unsigned)(pl.Mrow3 / 64), N4 / 32),
                           dim3(256), 0, ctx.stream, dG.p, gt16.p, pl.Mtot3, N4, pl.Mrow3, W,
                           cexp.p, bias_part.p, (long long)2 * N4 * pl.Mrow3, npl);
      else
        hipLaunchKernelGGL(mv::transpose_split_kernel, dim3((unsigned)(pl.Mrow / 64), N4 / 64),
                           dim3(256), 0, ctx.stream, dG.p, gt16.p, pl.Mtot, N4, pl.Mrow, W, 0,
                           cexp.p, 0, bias_part.p, npl);
      wgrad_transpose_operand(ctx.stream, pl, dH.p, at16, C, H, W, nullptr, 8, npl);
      hipLaunchKernelGGL(mv::absmax_bits_kernel, dim3(256), dim3(256), 0, ctx.stream, dX.p,
                         (size_t)pl.Mtot * Cx, cexp.p + 64);
      hipLaunchKernelGGL(mv::chain_exp_kernel, dim3(1), dim3(64), 0, ctx.stream, cexp.p + 64, 1,
                         64, cexp.p + 2, pl.wino ? 10 : 13);
      wgrad_transpose_operand(ctx.stream, pl, dX.p, xt16, Cx, H, W, cexp.p + 2, 0, npl);
      HIP_CHECK(hipGetLastError());
      mv::Wgrad16Args q{};
      for (int d = 0; d < 3; ++d) q.at[d] = at16[d].p;
      q.gt = gt16.p; q.partial = partial.p; q.g_exp = cexp.p;
      q.a_exp = cexp.p + 1;
      q.Mrow = pl.Mrow; q.H = H; q.W = W; q.Cx = Cx; q.C = C; q.Ca = C;
      if (pl.wino) {
        q.ntaps = 15; q.Mrow = pl.Mrow3; q.H = H / 3;
        q.a_comp_stride = (int64_t)2 * C * pl.Mrow3; q.g_comp_stride = (int64_t)2 * N4 * pl.Mrow3;
      }
      if (pl.wide) q.map_mode = pl.map_mode;
      mv::wgrad16_plan(q, pl.Mgemm, pl.nsplit);
      launch_wgrad16(ctx.stream, q, pl.wide, pl.one, false);
      mv::Wgrad16Args qx = q;
      for (int d = 0; d < 3; ++d) qx.at[d] = xt16[d].p;
      qx.Ca = Cx; qx.a_exp = cexp.p + 2;
      if (pl.wino) {
        qx.a_comp_stride = (int64_t)2 * Cx * pl.Mrow3;
        mv::wgrad16_plan(qx, pl.Mgemm, pl.nsplit_x);
      }
      launch_wgrad16(ctx.stream, qx, pl.wide_x, pl.one, true);
      HIP_CHECK(hipGetLastError());
      if (pl.wino)
        hipLaunchKernelGGL(mv::wgrad_wino3_reduce_kernel, dim3(cdiv(ncols / 3, 256)), dim3(256), 0,
                           ctx.stream, partial.p, pl.nsplit, pl.nsplit_x, (size_t)Cx * N4,
                           ncols / 9, dW.p);
      else
        hipLaunchKernelGGL(mv::colsum_kernel, dim3(1, cdiv(ncols, 256)), dim3(256), 0, ctx.stream,
                           partial.p, dW.p, (size_t)pl.nsplit, ncols, (size_t)pl.nsplit);
      HIP_CHECK(hipGetLastError());
      forms[0] = pl.wide; forms[1] = pl.wide_x; forms[2] = pl.nsplit; forms[3] = pl.nsplit_x;
      forms[7] = pl.transpose3;
    }
    if (vd != 0) {
      ctx.down(dx, dxo, cells * Cx);
      ctx.down(dh, dho, cells * C);
    }
    if (vw != 0) ctx.down(dkernel, dW, ncols);
    int32_t ce[3] = {0, 0, 0};
    { DevBuf<int32_t>& src = cexp; HIP_CHECK(hipStreamSynchronize(ctx.stream));
      HIP_CHECK(hipMemcpy(ce, src.p, sizeof(ce), hipMemcpyDeviceToHost)); }
    if (vw != 0) { exps[0] = ce[0]; exps[1] = ce[1]; exps[2] = ce[2]; }
    else if (vd == 1 || vd == 2) ctx.down(exps, gexp, 1);
  });
}

// The pointwise backward of one step in each of its three kernels: form 0 lstm_gate_bwd_kernel,
// 1 lstm_gate_bwd4_kernel, 2 lstm_gate_bwd4_plane_kernel (train_kernels.h).  gates [cells,4,C] the
// saved activations, dc the incoming d c'; G_out [cells,4C], dc_out [cells,C], gmax_bits the
// largest of the 64 spread maxima; plane_out (form 2) [cells,4C]: the bf16 plane decoded.
int mv_op_lstm_gate_bwd(int device, int32_t form, const float* gates, const float* c_prev,
                        const float* c_new, const float* dh, const float* dc, int32_t cells,
                        int32_t C, float* G_out, float* dc_out, int32_t* gmax_bits,
                        float* plane_out) {
  return guarded(nullptr, [&] {
    MV_REQUIRE(form >= 0 && form <= 2, "lstm_gate_bwd: form %d (0 scalar, 1 four channels per "
               "thread, 2 the same with the bf16 plane)", (int)form);
    MV_REQUIRE(cells >= 1 && C >= 32 && C % 32 == 0 && C <= 512, "lstm_gate_bwd: C a multiple of "
               "32 up to 512");
    MV_REQUIRE(gates && c_new && dh && dc && G_out && dc_out && gmax_bits,
               "lstm_gate_bwd: NULL argument");
    MV_REQUIRE(form != 2 || plane_out, "lstm_gate_bwd: form 2 needs plane_out");
    OpCtx ctx(device);
    const size_t n = (size_t)cells, total = n * C;
    DevBuf<float> g, cp, cn, d_h, d_c, dec;
    DevBuf<int32_t> mb;
    DevBuf<_Float16> plane;
    ctx.up(g, gates, total * 4);
    if (c_prev) ctx.up(cp, c_prev, total);
    ctx.up(cn, c_new, total);
    ctx.up(d_h, dh, total);
    ctx.up(d_c, dc, total);
    mb.alloc(64);
    HIP_CHECK(hipMemsetAsync(mb.p, 0, 64 * sizeof(int32_t), ctx.stream));
    if (form == 2) {
      const size_t pn = 2 * (total * 4 + mv::kPlaneSlack + mv::kPlanePad);
      plane.alloc(pn);
      HIP_CHECK(hipMemsetAsync(plane.p, kOpSentinel, pn * sizeof(_Float16), ctx.stream));
      hipLaunchKernelGGL(mv::lstm_gate_bwd4_plane_kernel,
                         dim3((unsigned)(((n + 31) / 32) * (size_t)(C / 32))), dim3(256), 0,
                         ctx.stream, g.p, cp.p, cn.p, d_h.p, d_c.p, (long long)cells, C,
                         plane.p + mv::kPlanePad, mb.p);
      dec.alloc(total * 4);
      hipLaunchKernelGGL(decode_plane_bf16_kernel, dim3(cdiv(total * 4, 256)), dim3(256), 0,
                         ctx.stream, plane.p + mv::kPlanePad, dec.p, n, 4 * C);
    } else if (form == 1) {
      hipLaunchKernelGGL(mv::lstm_gate_bwd4_kernel, dim3(cdiv(total / 4, 256)), dim3(256), 0,
                         ctx.stream, g.p, cp.p, cn.p, d_h.p, d_c.p, total / 4, C, mb.p);
    } else {
      hipLaunchKernelGGL(mv::lstm_gate_bwd_kernel, dim3(cdiv(total, 256)), dim3(256), 0,
                         ctx.stream, g.p, cp.p, cn.p, d_h.p, d_c.p, total, C, mb.p);
    }
    HIP_CHECK(hipGetLastError());
    ctx.down(G_out, g, total * 4);
    ctx.down(dc_out, d_c, total);
    if (form == 2) ctx.down(plane_out, dec, total * 4);
    int32_t hb[64];
    ctx.down(hb, mb, (size_t)64);
    int32_t best = 0;
    for (int i = 0; i < 64; ++i) best = std::max(best, hb[i]);
    *gmax_bits = best;
  });
}

int mv_op_gnn_bwd(int device, const float* h, const float* scene_mean, const float* g,
                  int32_t M, int32_t H, int32_t W, int32_t C, int32_t D, float* dh,
                  float* dscene_mean) {
  return guarded(nullptr, [&] {
    MV_REQUIRE(C % 64 == 0 && C <= 512 && D >= 0 && D <= 128,
               "gnn_bwd: C a multiple of 64 up to 512, D <= 128");
    OpCtx ctx(device);
    const size_t cells = (size_t)M * H * W;
    DevBuf<float> dh_, ds_, dg_, a, de, n, odh, ods;
    ctx.up(dh_, h, cells * C);
    ctx.up(ds_, scene_mean, cells * D);
    ctx.up(dg_, g, cells * C);
    a.alloc(cells * 9); de.alloc(cells * 9); n.alloc(cells);
    odh.alloc(cells * C); ods.alloc(cells * (D ? D : 1));
    launch_gnn_bwd(ctx.stream, dh_.p, ds_.p, dg_.p, a.p, de.p, n.p, odh.p, ods.p, M, H, W, C, D, 0);
    HIP_CHECK(hipGetLastError());
    ctx.down(dh, odh, cells * C);
    if (dscene_mean && D) ctx.down(dscene_mean, ods, cells * D);
  });
}

// ---- the helper kernels of a training step, one door each (tests/test_gpu_train_helpers.py):
// every door uploads its operands, calls the launcher the engine calls (engine_train.h
// launch_small_dgrad / launch_small_wgrad / launch_colsum / launch_long_sum / launch_scene_dgrad
// / launch_scene_wgrad / launch_grid_emb_onehot_wgrad / launch_ce_loss / launch_huber_loss) and
// reports the form that ran.  Output buffers hold kOpSentinel bytes before the launches.

int mv_op_small_conv_dgrad(int device, int32_t form, const float* dout, int64_t dout_rs,
                           const float* w, float* din, int64_t din_rs, int32_t M, int32_t H,
                           int32_t W, int32_t Ci, int32_t Co, int32_t accumulate,
                           int32_t* form_ran) {
  return guarded(nullptr, [&] {
    MV_REQUIRE(dout && w && din && form_ran, "mv_op_small_conv_dgrad: NULL argument");
    MV_REQUIRE(M >= 1 && H >= 1 && W >= 1 && Ci >= 1 && Co >= 1,
               "mv_op_small_conv_dgrad: bad shape");
    MV_REQUIRE(dout_rs >= (int64_t)H * W * Co && din_rs >= (int64_t)H * W * Ci,
               "mv_op_small_conv_dgrad: a row stride is shorter than a row");
    MV_REQUIRE(form >= 0 && form <= 3, "mv_op_small_conv_dgrad: form %d (0 = the plan's, 1 scalar, "
               "2 dgrad4<1>, 3 dgrad4<2>)", (int)form);
    const bool v4 = small_dgrad_vec4_ok((size_t)din_rs, M, H, W, Ci, Co);
    MV_REQUIRE(form != 2 || (v4 && Co == 1), "mv_op_small_conv_dgrad: form dgrad4<1> needs "
               "Ci %% 4 == 0, Co == 1 and a din row stride that is a multiple of 4");
    MV_REQUIRE(form != 3 || (v4 && Co == 2), "mv_op_small_conv_dgrad: form dgrad4<2> needs "
               "Ci %% 4 == 0, Co == 2 and a din row stride that is a multiple of 4");
    const SmallDgradForm f = form == 0 ? plan_small_dgrad((size_t)din_rs, M, H, W, Ci, Co)
                                       : (SmallDgradForm)form;
    OpCtx ctx(device);
    DevBuf<float> d_o, d_w, d_i;
    ctx.up(d_o, dout, (size_t)M * dout_rs);
    ctx.up(d_w, w, (size_t)9 * Ci * Co);
    ctx.up(d_i, din, (size_t)M * din_rs);
    launch_small_dgrad(ctx.stream, f, d_o.p, (size_t)dout_rs, d_w.p, d_i.p, (size_t)din_rs, M, H,
                       W, Ci, Co, accumulate != 0);
    HIP_CHECK(hipGetLastError());
    ctx.down(din, d_i, (size_t)M * din_rs);
    *form_ran = (int32_t)f;
  });
}

int mv_op_small_conv_wgrad(int device, int32_t form, const float* in, const float* dout,
                           int32_t R, int32_t H, int32_t W, int32_t Ci, int32_t Co, float* dw,
                           int32_t* info) {
  return guarded(nullptr, [&] {
    MV_REQUIRE(in && dout && dw && info, "mv_op_small_conv_wgrad: NULL argument");
    MV_REQUIRE(R >= 1 && H >= 1 && W >= 1 && Ci >= 1 && Co >= 1,
               "mv_op_small_conv_wgrad: bad shape");
    MV_REQUIRE(form >= 0 && form <= 3, "mv_op_small_conv_wgrad: form %d (0 = the plan's, 1 "
               "small_wgrad<false>, 2 small_wgrad<true>, 3 h2g)", (int)form);
    const SmallWgradPlan p = plan_small_wgrad(R, H, W, Ci, Co);
    require_small_wgrad_shape(p);
    MV_REQUIRE(p.P <= 512 || p.lds2 <= 48 * 1024, "small wgrad: LDS of the hidden2grid form");
    MV_REQUIRE((form != 1 && form != 2) || p.P <= 512, "mv_op_small_conv_wgrad: form "
               "small_wgrad<%s> needs Ci*Co <= 512", form == 2 ? "true" : "false");
    MV_REQUIRE(form != 3 || ((Co == 1 || Co == 2) && p.lds2 <= 48 * 1024),
               "mv_op_small_conv_wgrad: form h2g needs Co 1 or 2 and its slab in 48 KB of LDS");
    const SmallWgradForm f = form == 0 ? p.form : (SmallWgradForm)form;
    OpCtx ctx(device);
    DevBuf<float> d_i, d_o, d_w, partial, scratch;
    ctx.up(d_i, in, (size_t)p.cells * Ci);
    ctx.up(d_o, dout, (size_t)p.cells * Co);
    d_w.alloc(p.ncols); partial.alloc((size_t)p.nblk * p.ncols); scratch.alloc(64 * p.ncols);
    HIP_CHECK(hipMemsetAsync(d_w.p, kOpSentinel, p.ncols * sizeof(float), ctx.stream));
    launch_small_wgrad(ctx.stream, p, f, d_i.p, d_o.p, d_w.p, R, H, W, Ci, Co, partial.p,
                       scratch.p);
    HIP_CHECK(hipGetLastError());
    ctx.down(dw, d_w, p.ncols);
    info[0] = (int32_t)f; info[1] = (int32_t)p.nblk; info[2] = p.cpb;
    info[3] = f == SmallWgradForm::H2g ? 1 : p.G;
  });
}

int mv_op_colsum(int device, const float* x, int64_t rows, int64_t ncols, float* out,
                 int32_t* info) {
  return guarded(nullptr, [&] {
    MV_REQUIRE(x && out && info, "mv_op_colsum: NULL argument");
    MV_REQUIRE(rows >= 1 && ncols >= 1, "mv_op_colsum: bad shape");
    OpCtx ctx(device);
    DevBuf<float> d_x, d_o, tmp;
    ctx.up(d_x, x, (size_t)rows * ncols);
    d_o.alloc((size_t)ncols); tmp.alloc((size_t)1056 * ncols);
    HIP_CHECK(hipMemsetAsync(d_o.p, kOpSentinel, (size_t)ncols * sizeof(float), ctx.stream));
    const ColsumPlan p = launch_colsum(ctx.stream, d_x.p, (size_t)rows, (size_t)ncols, d_o.p,
                                       tmp.p);
    HIP_CHECK(hipGetLastError());
    ctx.down(out, d_o, (size_t)ncols);
    info[0] = (int32_t)p.nslab; info[1] = p.narrow ? 1 : 0;
  });
}

int mv_op_long_sum(int device, const float* x, int64_t n, float scale, float* out,
                   int32_t* chunked) {
  return guarded(nullptr, [&] {
    MV_REQUIRE(x && out && chunked, "mv_op_long_sum: NULL argument");
    MV_REQUIRE(n >= 1, "mv_op_long_sum: bad length");
    OpCtx ctx(device);
    DevBuf<float> d_x, d_o, partial;
    ctx.up(d_x, x, (size_t)n);
    d_o.alloc(1);
    const size_t pn = cdiv((size_t)n, mv::kSumChunk);
    partial.alloc(pn);
    HIP_CHECK(hipMemsetAsync(d_o.p, kOpSentinel, sizeof(float), ctx.stream));
    const bool c = launch_long_sum(ctx.stream, d_x.p, (size_t)n, d_o.p, scale, partial.p, pn);
    HIP_CHECK(hipGetLastError());
    ctx.down(out, d_o, (size_t)1);
    *chunked = c ? 1 : 0;
  });
}

int mv_op_scene_conv_bwd(int device, const float* in, const float* y, const float* dy,
                         const float* w, int32_t U, int32_t Hi, int32_t Wi, int32_t Ci,
                         int32_t Co, int32_t k, int32_t act, const float* din_init,
                         int32_t accumulate, float* dpre, float* din, float* dw, float* db,
                         int32_t* info) {
  return guarded(nullptr, [&] {
    MV_REQUIRE(in && y && dy && w && dpre && din && dw && db && info,
               "mv_op_scene_conv_bwd: NULL argument");
    MV_REQUIRE(U >= 1 && Hi >= 1 && Wi >= 1 && Ci >= 1 && Co >= 1 && k >= 1,
               "mv_op_scene_conv_bwd: bad shape");
    MV_REQUIRE(act >= 0 && act <= 2, "mv_op_scene_conv_bwd: activation %d", (int)act);
    MV_REQUIRE(!accumulate || din_init, "mv_op_scene_conv_bwd: accumulate needs din_init");
    OpCtx ctx(device);
    const int Ho = (Hi + 1) / 2, Wo = (Wi + 1) / 2;      // SAME, stride 2
    const size_t nin = (size_t)U * Hi * Wi * Ci, nout = (size_t)U * Ho * Wo * Co;
    const SceneWgradPlan p = plan_scene_wgrad(U, Ho, Ci, Co, k);
    DevBuf<float> d_in, d_y, d_dy, d_w, d_pre, d_din, d_dw, d_db, partial;
    ctx.up(d_in, in, nin);
    ctx.up(d_y, y, nout);
    ctx.up(d_dy, dy, nout);
    ctx.up(d_w, w, p.nw);
    if (din_init) ctx.up(d_din, din_init, nin);
    else {
      d_din.alloc(nin);
      HIP_CHECK(hipMemsetAsync(d_din.p, kOpSentinel, nin * sizeof(float), ctx.stream));
    }
    d_pre.alloc(nout); d_dw.alloc(p.nw); d_db.alloc((size_t)Co);
    const size_t pn = std::max((size_t)p.nslab * p.nw, (size_t)1056 * Co);
    partial.alloc(pn);
    HIP_CHECK(hipMemsetAsync(d_pre.p, kOpSentinel, nout * sizeof(float), ctx.stream));
    HIP_CHECK(hipMemsetAsync(d_dw.p, kOpSentinel, p.nw * sizeof(float), ctx.stream));
    HIP_CHECK(hipMemsetAsync(d_db.p, kOpSentinel, (size_t)Co * sizeof(float), ctx.stream));
    hipLaunchKernelGGL(mv::tanh_bwd_kernel, dim3(cdiv(nout, 256)), dim3(256), 0, ctx.stream,
                       d_dy.p, d_y.p, d_pre.p, nout, (int)act);
    launch_scene_dgrad(ctx.stream, d_pre.p, d_w.p, d_din.p, U, Hi, Wi, Ci, Ho, Wo, Co, k,
                       accumulate != 0);
    launch_scene_wgrad(ctx.stream, d_in.p, d_pre.p, d_dw.p, U, Hi, Wi, Ci, Ho, Wo, Co, k,
                       partial.p, pn);
    launch_colsum(ctx.stream, d_pre.p, (size_t)U * Ho * Wo, (size_t)Co, d_db.p, partial.p);
    HIP_CHECK(hipGetLastError());
    ctx.down(dpre, d_pre, nout);
    ctx.down(din, d_din, nin);
    ctx.down(dw, d_dw, p.nw);
    ctx.down(db, d_db, (size_t)Co);
    info[0] = scene_same_pad(Ho, k, Hi); info[1] = scene_same_pad(Wo, k, Wi);
    info[2] = p.nslab; info[3] = p.rps;
  });
}

int mv_op_grid_emb_onehot_wgrad(int device, const float* dpre, const int32_t* labels, int32_t N,
                                int32_t T, int32_t H, int32_t W, int32_t E, int32_t accumulate,
                                float* dw) {
  return guarded(nullptr, [&] {
    MV_REQUIRE(dpre && labels && dw, "mv_op_grid_emb_onehot_wgrad: NULL argument");
    MV_REQUIRE(N >= 1 && T >= 1 && H >= 1 && W >= 1 && E >= 32 && E % 32 == 0,
               "mv_op_grid_emb_onehot_wgrad: bad shape (E a multiple of 32)");
    for (size_t i = 0; i < (size_t)N * T; ++i)
      MV_REQUIRE(labels[i] >= 0 && labels[i] < H * W, "mv_op_grid_emb_onehot_wgrad: label %d "
                 "is not a cell of the %d x %d grid", (int)labels[i], (int)H, (int)W);
    OpCtx ctx(device);
    DevBuf<float> d_p, d_w;
    DevBuf<int32_t> d_l;
    ctx.up(d_p, dpre, (size_t)T * N * H * W * E);
    ctx.up(d_l, labels, (size_t)N * T);
    ctx.up(d_w, dw, (size_t)9 * E);
    launch_grid_emb_onehot_wgrad(ctx.stream, d_p.p, d_l.p, N, T, H, W, E, d_w.p,
                                 accumulate != 0);
    HIP_CHECK(hipGetLastError());
    ctx.down(dw, d_w, (size_t)9 * E);
  });
}

// kind: 0 ce, 1 ce_soft, 2 ce_len (hard labels, or soft when given), 3 huber, 4 huber_len,
// 5 huber_masked (with count_positive_kernel in front and masked_mean_kernel behind)
int mv_op_train_loss(int device, int32_t kind, const float* pred, const int32_t* labels,
                     const float* soft, const float* target, const float* fg,
                     const float* sample_w, const int32_t* pred_lens, int32_t T, int32_t N,
                     int32_t K, float scale, float* loss, float* grad, float* loss_sum,
                     int32_t* info) {
  return guarded(nullptr, [&] {
    MV_REQUIRE(kind >= 0 && kind <= 5, "mv_op_train_loss: kind %d (0 ce, 1 ce_soft, 2 ce_len, "
               "3 huber, 4 huber_len, 5 huber_masked)", (int)kind);
    MV_REQUIRE(pred && loss && grad && loss_sum && info, "mv_op_train_loss: NULL argument");
    MV_REQUIRE(T >= 1 && N >= 1 && K >= 1, "mv_op_train_loss: bad shape");
    const bool ce = kind <= 2, lens = kind == 2 || kind == 4;
    MV_REQUIRE(!lens || pred_lens, "mv_op_train_loss: the kind needs pred_lens");
    MV_REQUIRE(lens || !pred_lens, "mv_op_train_loss: the kind takes no pred_lens");
    if (lens)
      for (int n = 0; n < N; ++n)
        MV_REQUIRE(pred_lens[n] >= 0 && pred_lens[n] <= T, "mv_op_train_loss: pred_lens[%d] = %d "
                   "outside [0, %d]", n, (int)pred_lens[n], (int)T);
    const size_t rows = (size_t)T * N;
    const bool hard = kind == 0 || (kind == 2 && !soft);
    if (ce) {
      MV_REQUIRE(kind != 0 || !soft, "mv_op_train_loss: ce takes labels, not soft labels");
      MV_REQUIRE(kind != 1 || soft, "mv_op_train_loss: ce_soft needs soft labels");
      MV_REQUIRE(!hard || labels, "mv_op_train_loss: the kind needs labels");
      MV_REQUIRE(!sample_w || kind != 2, "mv_op_train_loss: ce_len takes no sample weights");
      if (hard)
        for (size_t i = 0; i < rows; ++i)
          MV_REQUIRE(labels[i] >= 0 && labels[i] < K, "mv_op_train_loss: label %d outside "
                     "[0, %d)", (int)labels[i], (int)K);
    } else {
      MV_REQUIRE(target, "mv_op_train_loss: the kind needs a target");
      MV_REQUIRE(kind != 5 || fg, "mv_op_train_loss: huber_masked needs the foreground map");
      MV_REQUIRE(!sample_w, "mv_op_train_loss: the Huber kinds take no sample weights");
    }
    OpCtx ctx(device);
    DevBuf<float> d_pred, d_soft, d_tgt, d_fg, d_sw, d_loss, d_grad, d_sum, d_tmp, partial;
    DevBuf<int32_t> d_lab, d_len, d_cnt;
    const size_t nel = rows * K * (ce ? 1 : 2), nloss = ce ? rows : nel;
    ctx.up(d_pred, pred, nel);
    if (hard) ctx.up(d_lab, labels, rows);
    if (ce && soft) ctx.up(d_soft, soft, nel);
    if (!ce) ctx.up(d_tgt, target, nel);
    if (kind == 5) ctx.up(d_fg, fg, rows * K);
    if (sample_w) ctx.up(d_sw, sample_w, (size_t)N);
    if (lens) ctx.up(d_len, pred_lens, (size_t)N);
    d_loss.alloc(nloss); d_grad.alloc(nel); d_sum.alloc(1); d_tmp.alloc(1); d_cnt.alloc(1);
    const size_t pn = cdiv(nel, mv::kSumChunk);
    partial.alloc(pn);
    HIP_CHECK(hipMemsetAsync(d_loss.p, kOpSentinel, nloss * sizeof(float), ctx.stream));
    HIP_CHECK(hipMemsetAsync(d_grad.p, kOpSentinel, nel * sizeof(float), ctx.stream));
    HIP_CHECK(hipMemsetAsync(d_sum.p, kOpSentinel, sizeof(float), ctx.stream));
    HIP_CHECK(hipMemsetAsync(d_cnt.p, 0, sizeof(int32_t), ctx.stream));
    bool chunked = false;
    if (ce) {
      CeLossArgs a{};
      a.logits = d_pred.p; a.labels = hard ? d_lab.p : nullptr;
      a.soft = soft ? d_soft.p : nullptr; a.sample_w = sample_w ? d_sw.p : nullptr;
      a.pred_lens = lens ? d_len.p : nullptr;
      a.loss_row = d_loss.p; a.dlogits = d_grad.p; a.loss_out = d_sum.p;
      a.T = T; a.N = N; a.K = K; a.scale = scale;
      launch_ce_loss(ctx.stream, a);
    } else {
      HuberLossArgs a{};
      a.pred = d_pred.p; a.target = d_tgt.p;
      a.loss_elem = d_loss.p; a.dpred = d_grad.p; a.loss_out = d_sum.p;
      a.T = T; a.N = N; a.KP = K * 2; a.scale = scale;
      a.sum_tmp = d_tmp.p; a.partial = partial.p; a.partial_n = pn;
      if (kind == 5) {
        launch_count_positive(ctx.stream, d_fg.p, rows * K, d_cnt.p);
        a.fg = d_fg.p; a.count = d_cnt.p;
      } else if (lens) {
        a.pred_lens = d_len.p;
      }
      chunked = launch_huber_loss(ctx.stream, a);
    }
    HIP_CHECK(hipGetLastError());
    ctx.down(loss, d_loss, nloss);
    ctx.down(grad, d_grad, nel);
    ctx.down(loss_sum, d_sum, (size_t)1);
    ctx.down(info, d_cnt, (size_t)1);
    info[1] = chunked ? 1 : 0;
  });
}

// Debug probe (not part of the public header): XCC id of every workgroup of a
// 1-D launch of `nblocks` x 256 threads -- checks the "linear id % 8 -> XCD"
// dispatch pattern the XCD-aware block maps rely on for speed.
__global__ void xcc_probe_kernel(int32_t* out) {
  if (threadIdx.x == 0) {
    uint32_t v;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(v));
    out[blockIdx.x] = (int32_t)(v & 0xf);
  }
}

int mv_debug_xcc_map(int device, int32_t nblocks, int32_t* out) {
  return guarded(nullptr, [&] {
    OpCtx ctx(device);
    DevBuf<int32_t> d;
    d.alloc(nblocks);
    hipLaunchKernelGGL(xcc_probe_kernel, dim3(nblocks), dim3(256), 0, ctx.stream, d.p);
    HIP_CHECK(hipGetLastError());
    ctx.down(out, d, (size_t)nblocks);
  });
}

}  // extern "C"
