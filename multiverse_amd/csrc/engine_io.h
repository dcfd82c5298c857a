// host <-> device: input upload (dense / compact), output download, the pipelined feed / fetch -- part of the ONE translation unit engine.hip (included from there, in order;
// not a stand-alone header).
#pragma once

namespace {

// The checks every input upload makes (dense, compact, pipelined) after its own NULL checks: the
// scene frame count, pred_len, the compact form's row count, the scene indices.
void check_inputs(const mv_engine* e, int num_scene_frames, int pred_len,
                  const int32_t* obs_scene, int num_rows = 0) {
  const mv_config& c = e->cfg;
  const size_t N = c.batch_size, T = c.obs_len;
  const bool scene = !e->no_scene();
  MV_REQUIRE(!scene || (num_scene_frames >= 1 && (size_t)num_scene_frames <= N * T),
             "num_scene_frames %d not in [1, N*T_o=%zu]", num_scene_frames, N * T);
  MV_REQUIRE(pred_len >= 1 && pred_len <= c.max_pred_len,
             "pred_len %d not in [1, max_pred_len=%d]", pred_len, c.max_pred_len);
  MV_REQUIRE(num_rows >= 0 && (size_t)num_rows <= N, "num_rows %d not in [0, N=%zu]",
             num_rows, N);
  for (size_t i = 0; scene && i < N * T; ++i)
    MV_REQUIRE(obs_scene[i] >= 0 && obs_scene[i] < num_scene_frames,
               "obs_scene[%zu] = %d out of range [0,%d)", i, obs_scene[i], num_scene_frames);
}

// ... and per enabled scale: every observed label is a cell of the grid
void check_labels(const mv_engine* e, int s, const int32_t* labels) {
  const size_t NT = (size_t)e->cfg.batch_size * e->cfg.obs_len;
  const int K = e->sc[s].K;
  for (size_t i = 0; i < NT; ++i)
    MV_REQUIRE(labels[i] >= 0 && labels[i] < K,
               "grid_obs_labels[%d][%zu] = %d out of range [0,%d)", s, i, labels[i], K);
}

// ---- light cone of the class encoder (gate_plan.h enc_cone_planned): which wave tiles of the
// gate kernel -- 32 consecutive triple-cells q = (row * ceil(H / 3) + triple) * W + x -- each
// encoder step has to compute.  The encoder starts from the zero state and its x is one hot cell
// per row and step, so a row's state equals the input-free (background) row's except at DIRTY
// cells.  A cell is dirty after step t if the step's own x reaches it (within Chebyshev distance
// r0 of the observed cell: 1 for scene_conv * one_hot, 2 for grid_emb(one_hot), the kernels'
// sx_rad) or if the h operand of its gate convolution held a dirty cell.  That operand is NOT the
// 3 x 3 neighbourhood: the F(3,3) form computes the three rows of a triple from the FIVE input
// rows 3k - 1 .. 3k + 3, and the rows a 3 x 3 stencil would not read cancel only in exact
// arithmetic -- they reach the result's last bits.  So dirt spreads one column per step along x
// (the direct taps) and from any of those five rows to the whole triple along y, and the result
// stays bit-identical to the dense encoder's.  A tile is active at step t if it holds a dirty
// cell or any cell of the background row (row N).  The first step (zero state: no main loop) and
// the last (the decoders want a dense state) run every tile.  Host loop over the labels, no
// device; W <= 32 (a grid row is one 32-bit column mask).
//   out [T][enc_cone_step_elems(N + 1, H, W)]: count | 3 pad | active tile indices, ascending |
//       per tile 1 = computed at this step;  cells [T]: cells the step executes
void build_enc_cone(const int32_t* labels, int N, int T, int H, int W, int r0, int32_t* out,
                    int64_t* cells) {
  const int Ht = (H + 2) / 3, Kt = Ht * W, Q = (N + 1) * Kt;
  const int ntile = enc_cone_tiles(N + 1, H, W);
  const size_t stride = enc_cone_step_elems(N + 1, H, W);
  const uint32_t wmask = W >= 32 ? 0xffffffffu : ((1u << W) - 1u);
  std::vector<uint32_t> dirty((size_t)N * H, 0u), tmp(H);
  for (int t = 0; t < T; ++t) {
    int32_t* blk = out + (size_t)t * stride;
    int32_t* list = blk + 4;
    int32_t* flag = blk + 4 + ntile;
    const bool all = t == 0 || t == T - 1;
    for (int g = 0; g < ntile; ++g) flag[g] = all ? 1 : 0;
    if (!all)
      for (int q = N * Kt; q < Q; ++q) flag[q >> 5] = 1;          // the background row
    for (int n = 0; n < N; ++n) {
      uint32_t* d = &dirty[(size_t)n * H];
      for (int k = 0; k < Ht; ++k) {          // the h operand: rows 3k - 1 .. 3k + 3, columns +- 1
        uint32_t m = 0;
        for (int y = std::max(3 * k - 1, 0); y <= std::min(3 * k + 3, H - 1); ++y) m |= d[y];
        m = (m | (m << 1) | (m >> 1)) & wmask;
        for (int y = 3 * k; y < std::min(3 * k + 3, H); ++y) tmp[y] = m;
      }
      const int cell = labels[(size_t)n * T + t], ys = cell / W, xs = cell % W;
      uint32_t xm = 0;                        // the step's own x
      for (int x = std::max(xs - r0, 0); x <= std::min(xs + r0, W - 1); ++x) xm |= 1u << x;
      for (int y = 0; y < H; ++y) d[y] = tmp[y] | ((y >= ys - r0 && y <= ys + r0) ? xm : 0u);
      if (all) continue;
      for (int k = 0; k < Ht; ++k) {
        uint32_t m = 0;
        for (int y = 3 * k; y < std::min(3 * k + 3, H); ++y) m |= d[y];
        for (int x = 0; m; ++x, m >>= 1)
          if (m & 1u) flag[(n * Kt + k * W + x) >> 5] = 1;
      }
    }
    int cnt = 0;
    int64_t nc = 0;
    for (int g = 0; g < ntile; ++g) {
      if (!flag[g]) continue;
      list[cnt++] = g;
      for (int q = 32 * g; q < std::min(32 * g + 32, Q); ++q)
        nc += std::min(3, H - 3 * ((q % Kt) / W));
    }
    for (int g = cnt; g < ntile; ++g) list[g] = 0;
    blk[0] = cnt; blk[1] = blk[2] = blk[3] = 0;
    if (cells) cells[t] = nc;
  }
}

// do the uploads of this scale build the lists?  Geometry and the switch only: the compute mode
// may still change before the forward, which asks enc_cone_on (engine_setup.h)
bool enc_cone_wanted(const mv_engine* e, const ScaleState& S) {
  return S.use && enc_cone_geometry(e->cfg.obs_len, S.H, S.W, e->cfg.batch_size);
}
size_t enc_cone_elems(const mv_engine* e, const ScaleState& S) {
  return (size_t)e->cfg.obs_len * enc_cone_step_elems(e->cfg.batch_size + 1, S.H, S.W);
}
// the lists of `labels` into `dst` (host; pinned slot or the scale's own staging vector) and the
// per-step cell counts into the scale: once per upload, on every path that brings labels
void build_scale_cone(mv_engine* e, ScaleState& S, const int32_t* labels, int32_t* dst) {
  S.cone_cells.assign(e->cfg.obs_len, 0);
  build_enc_cone(labels, e->cfg.batch_size, e->cfg.obs_len, S.H, S.W, e->no_scene() ? 2 : 1, dst,
                 S.cone_cells.data());
  S.cone_ready = true;
}
void upload_scale_cone(mv_engine* e, ScaleState& S, const int32_t* labels) {
  if (!enc_cone_wanted(e, S)) return;
  S.cone_host.resize(enc_cone_elems(e, S));
  S.cone.alloc(S.cone_host.size());
  build_scale_cone(e, S, labels, S.cone_host.data());
  HIP_CHECK(hipMemcpyAsync(S.cone.p, S.cone_host.data(), S.cone_host.size() * sizeof(int32_t),
                           hipMemcpyHostToDevice, e->stream));
}

void upload_inputs(mv_engine* e, const mv_inputs* in) {
  const mv_config& c = e->cfg;
  const size_t N = c.batch_size, T = c.obs_len;
  const bool scene = !e->no_scene();   // no scene encoder: the scene arrays may be NULL
  MV_REQUIRE(!scene || (in->obs_scene && in->scene_feat), "obs_scene / scene_feat is NULL");
  check_inputs(e, in->num_scene_frames, in->pred_len, in->obs_scene);
  e->num_frames = scene ? in->num_scene_frames : 0;
  e->pred_len = in->pred_len;
  if (scene) {
    HIP_CHECK(hipMemcpyAsync(e->obs_scene.p, in->obs_scene, N * T * sizeof(int32_t),
                             hipMemcpyHostToDevice, e->stream));
    HIP_CHECK(hipMemcpyAsync(e->scene_feat.p, in->scene_feat,
                             (size_t)e->num_frames * c.scene_h * c.scene_w *
                                 c.scene_class * sizeof(float),
                             hipMemcpyHostToDevice, e->stream));
  }
  for (int s = 0; s < c.num_scales; ++s) {
    ScaleState& S = e->sc[s];
    if (!S.use) continue;
    MV_REQUIRE(in->grid_obs_labels[s] && in->grid_obs_regress[s],
               "grid_obs_labels/grid_obs_regress[%d] is NULL for an enabled scale", s);
    check_labels(e, s, in->grid_obs_labels[s]);
    HIP_CHECK(hipMemcpyAsync(S.labels.p, in->grid_obs_labels[s],
                             N * T * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    upload_scale_cone(e, S, in->grid_obs_labels[s]);
    HIP_CHECK(hipMemcpyAsync(S.obs_reg.p, in->grid_obs_regress[s],
                             N * T * S.K * 2 * sizeof(float), hipMemcpyHostToDevice,
                             e->stream));
  }
  HIP_CHECK(hipStreamSynchronize(e->stream));
  e->inputs_ready = true;
}

// compact inputs: labels / scene indices as before, maps and masks expanded in HBM
void upload_inputs_compact(mv_engine* e, const mv_inputs_compact* in) {
  const mv_config& c = e->cfg;
  const size_t N = c.batch_size, T = c.obs_len;
  const bool scene = !e->no_scene();   // no scene encoder: the scene arrays may be NULL
  MV_REQUIRE(in->obs_xy && (!scene || (in->obs_scene && in->scene_feat_u8)),
             "obs_scene / scene_feat_u8 / obs_xy is NULL");
  check_inputs(e, in->num_scene_frames, in->pred_len, in->obs_scene, in->num_rows);
  e->num_frames = scene ? in->num_scene_frames : 0;
  e->pred_len = in->pred_len;
  if (scene) {
    HIP_CHECK(hipMemcpyAsync(e->obs_scene.p, in->obs_scene, N * T * sizeof(int32_t),
                             hipMemcpyHostToDevice, e->stream));
    const size_t nscene = (size_t)e->num_frames * c.scene_h * c.scene_w * c.scene_class;
    e->scene_u8.alloc(N * T * c.scene_h * c.scene_w * c.scene_class);
    HIP_CHECK(hipMemcpyAsync(e->scene_u8.p, in->scene_feat_u8, nscene, hipMemcpyHostToDevice,
                             e->stream));
    hipLaunchKernelGGL(mv::u8_to_f32_kernel, dim3(cdiv(nscene, 256)), dim3(256), 0,
                       e->stream, e->scene_u8.p, e->scene_feat.p, nscene);
  }
  e->xy_dev.alloc(2 * N * std::max<size_t>(T, c.max_pred_len));
  HIP_CHECK(hipMemcpyAsync(e->xy_dev.p, in->obs_xy, 2 * N * T * sizeof(double),
                           hipMemcpyHostToDevice, e->stream));
  for (int s = 0; s < c.num_scales; ++s) {
    ScaleState& S = e->sc[s];
    if (!S.use) continue;
    MV_REQUIRE(in->grid_obs_labels[s], "grid_obs_labels[%d] is NULL for an enabled scale", s);
    MV_REQUIRE(S.centers.p, "mv_set_grid_centers(%d) has not been called", s);
    check_labels(e, s, in->grid_obs_labels[s]);
    HIP_CHECK(hipMemcpyAsync(S.labels.p, in->grid_obs_labels[s],
                             N * T * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    upload_scale_cone(e, S, in->grid_obs_labels[s]);
    hipLaunchKernelGGL(mv::regress_from_xy_kernel, dim3(cdiv(N * T * S.K, 256)), dim3(256), 0,
                       e->stream, e->xy_dev.p, S.centers.p, S.obs_reg.p, (int)(N * T), (int)T,
                       S.K, in->num_rows);
  }
  HIP_CHECK(hipStreamSynchronize(e->stream));
  e->inputs_ready = true;
}

void download_outputs(mv_engine* e, mv_outputs* out) {
  const mv_config& c = e->cfg;
  const size_t N = c.batch_size, Tp = e->pred_len;
  for (int s = 0; s < c.num_scales; ++s) {
    ScaleState& S = e->sc[s];
    if (!S.use) continue;
    if (out->grid_pred_class[s])
      HIP_CHECK(hipMemcpyAsync(out->grid_pred_class[s], S.out_cls.p,
                               N * Tp * S.K * sizeof(float), hipMemcpyDeviceToHost,
                               e->stream));
    if (out->grid_pred_reg[s])
      HIP_CHECK(hipMemcpyAsync(out->grid_pred_reg[s], S.out_reg.p,
                               N * Tp * S.K * 2 * sizeof(float), hipMemcpyDeviceToHost,
                               e->stream));
  }
  HIP_CHECK(hipStreamSynchronize(e->stream));
}

// ---- pipelined greedy forward.  One `sess.run` of the reference is feed + compute + fetch,
// strictly in turn (code/pred_models.py:1761-1790).  An evaluation loop knows its next batch
// while the current one computes: mv_submit_greedy copies the caller's buffers into a pinned
// slot and queues H2D (copy stream) -> device staging -> [compute stream: D2D into the live
// input buffers, the forward, D2D of the outputs into the slot] -> D2H (copy stream) and
// returns; mv_collect_greedy waits for the OLDEST submission and hands its outputs over.
// With two slots the PCIe traffic of batches k+1 and k-1 runs under the kernels of batch k.
// Layout of a slot: obs_scene | scene_feat (N*T frames max) | per used scale labels,
// obs_regress, class-encoder tile lists || per used scale out_cls, out_reg (max_pred_len).
struct PipeLayout {
  size_t obs_scene = 0, scene_feat = 0, labels[MV_MAX_SCALES] = {0, 0},
         obs_reg[MV_MAX_SCALES] = {0, 0}, cone[MV_MAX_SCALES] = {0, 0}, in_bytes = 0;
  size_t out_cls[MV_MAX_SCALES] = {0, 0}, out_reg[MV_MAX_SCALES] = {0, 0}, out_bytes = 0;
};
static PipeLayout pipe_layout(const mv_engine* e) {
  const mv_config& c = e->cfg;
  const size_t N = c.batch_size, T = c.obs_len, Tp = c.max_pred_len;
  auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
  PipeLayout L;
  size_t o = 0;
  L.obs_scene = o; o = al(o + N * T * sizeof(int32_t));
  const size_t frames = e->no_scene() ? 0 : N * T;     // no scene encoder: no scene block
  L.scene_feat = o; o = al(o + frames * c.scene_h * c.scene_w * c.scene_class * sizeof(float));
  for (int s = 0; s < c.num_scales; ++s) {
    if (!e->sc[s].use) continue;
    const size_t K = e->sc[s].K;
    L.labels[s] = o; o = al(o + N * T * sizeof(int32_t));
    L.obs_reg[s] = o; o = al(o + N * T * K * 2 * sizeof(float));
    // the class encoder's tile lists travel with the labels they were built from
    L.cone[s] = o;
    if (enc_cone_wanted(e, e->sc[s])) o = al(o + enc_cone_elems(e, e->sc[s]) * sizeof(int32_t));
  }
  L.in_bytes = o;
  for (int s = 0; s < c.num_scales; ++s) {
    if (!e->sc[s].use) continue;
    const size_t K = e->sc[s].K;
    L.out_cls[s] = o; o = al(o + N * Tp * K * sizeof(float));
    L.out_reg[s] = o; o = al(o + N * Tp * K * 2 * sizeof(float));
  }
  L.out_bytes = o - L.in_bytes;
  return L;
}

void pipeline_create(mv_engine* e, int depth) {
  MV_REQUIRE(depth >= 1 && depth <= 8, "pipeline depth %d not in [1, 8]", depth);
  MV_REQUIRE(e->cfg.beam_size == 1, "the pipelined forward is the greedy one");
  MV_REQUIRE(e->pipe.empty(), "pipeline already created");
  const PipeLayout L = pipe_layout(e);
  HIP_CHECK(hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking));
  HIP_CHECK(hipStreamCreateWithFlags(&e->fetch_stream, hipStreamNonBlocking));
  e->pipe.resize(depth);
  for (auto& sl : e->pipe) {
    sl.in_bytes = L.in_bytes; sl.out_bytes = L.out_bytes;
    HIP_CHECK(hipHostMalloc(&sl.pin, L.in_bytes + L.out_bytes, hipHostMallocDefault));
    HIP_CHECK(hipMalloc((void**)&sl.dev, L.in_bytes + L.out_bytes));
    HIP_CHECK(hipEventCreateWithFlags(&sl.h2d, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&sl.d2h, hipEventDisableTiming));
  }
  e->pipe_head = e->pipe_tail = 0;
}

void pipeline_destroy(mv_engine* e) {
  for (auto& sl : e->pipe) {
    if (sl.pin) (void)hipHostFree(sl.pin);
    if (sl.dev) (void)hipFree(sl.dev);
    if (sl.h2d) (void)hipEventDestroy(sl.h2d);
    if (sl.done) (void)hipEventDestroy(sl.done);
    if (sl.d2h) (void)hipEventDestroy(sl.d2h);
  }
  e->pipe.clear();
  if (e->copy_stream) { (void)hipStreamDestroy(e->copy_stream); e->copy_stream = nullptr; }
  if (e->fetch_stream) { (void)hipStreamDestroy(e->fetch_stream); e->fetch_stream = nullptr; }
}

void pipeline_submit(mv_engine* e, const mv_inputs* in) {
  const mv_config& c = e->cfg;
  const size_t N = c.batch_size, T = c.obs_len;
  MV_REQUIRE(!e->pipe.empty(), "mv_pipeline_create has not been called");
  mv_engine::PipeSlot& sl = e->pipe[e->pipe_head % e->pipe.size()];
  MV_REQUIRE(!sl.busy, "pipeline full: %zu submissions not collected (mv_collect_greedy)",
             e->pipe.size());
  const bool scene = !e->no_scene();   // no scene encoder: the scene arrays may be NULL
  MV_REQUIRE(!scene || (in->obs_scene && in->scene_feat), "obs_scene / scene_feat is NULL");
  check_inputs(e, in->num_scene_frames, in->pred_len, in->obs_scene);
  const PipeLayout L = pipe_layout(e);
  char* pin = static_cast<char*>(sl.pin);
  const size_t sf_bytes = scene ? (size_t)in->num_scene_frames * c.scene_h * c.scene_w *
                                      c.scene_class * sizeof(float) : 0;
  if (scene) {
    memcpy(pin + L.obs_scene, in->obs_scene, N * T * sizeof(int32_t));
    memcpy(pin + L.scene_feat, in->scene_feat, sf_bytes);
  }
  for (int s = 0; s < c.num_scales; ++s) {
    ScaleState& S = e->sc[s];
    if (!S.use) continue;
    MV_REQUIRE(in->grid_obs_labels[s] && in->grid_obs_regress[s],
               "grid_obs_labels/grid_obs_regress[%d] is NULL for an enabled scale", s);
    check_labels(e, s, in->grid_obs_labels[s]);
    memcpy(pin + L.labels[s], in->grid_obs_labels[s], N * T * sizeof(int32_t));
    memcpy(pin + L.obs_reg[s], in->grid_obs_regress[s], N * T * S.K * 2 * sizeof(float));
    if (enc_cone_wanted(e, S))
      build_scale_cone(e, S, in->grid_obs_labels[s], reinterpret_cast<int32_t*>(pin + L.cone[s]));
  }
  MV_REQUIRE(!e->lens_set, "mv_submit_greedy: per-row prediction lengths are set "
             "(mv_set_pred_lengths); the pipelined forward is uniform -- clear them first");
  MV_REQUIRE(!e->obs_lens_short(), "mv_submit_greedy: per-row observation lengths are set "
             "(mv_set_obs_lengths); the pipelined forward is uniform -- clear them first");
  sl.num_frames = scene ? in->num_scene_frames : 0; sl.pred_len = in->pred_len;
  // copy stream: the whole input block in one transfer (it must not start before the
  // slot's previous fetch has left the same pinned / staging buffers: collect waited d2h)
  HIP_CHECK(hipMemcpyAsync(sl.dev, sl.pin, L.in_bytes, hipMemcpyHostToDevice, e->copy_stream));
  HIP_CHECK(hipEventRecord(sl.h2d, e->copy_stream));
  // compute stream: staging -> live inputs, forward, outputs -> staging
  HIP_CHECK(hipStreamWaitEvent(e->stream, sl.h2d, 0));
  auto d2d = [&](void* dst, const void* src, size_t n) {
    HIP_CHECK(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, e->stream));
  };
  if (scene) {
    d2d(e->obs_scene.p, sl.dev + L.obs_scene, N * T * sizeof(int32_t));
    d2d(e->scene_feat.p, sl.dev + L.scene_feat, sf_bytes);
  }
  for (int s = 0; s < c.num_scales; ++s) {
    ScaleState& S = e->sc[s];
    if (!S.use) continue;
    d2d(S.labels.p, sl.dev + L.labels[s], N * T * sizeof(int32_t));
    d2d(S.obs_reg.p, sl.dev + L.obs_reg[s], N * T * S.K * 2 * sizeof(float));
    if (enc_cone_wanted(e, S)) {
      S.cone.alloc(enc_cone_elems(e, S));
      d2d(S.cone.p, sl.dev + L.cone[s], enc_cone_elems(e, S) * sizeof(int32_t));
    }
  }
  e->num_frames = sl.num_frames;
  e->pred_len = sl.pred_len;
  e->inputs_ready = true;
  run_forward(e, ForwardKind::Greedy);
  const size_t Tp = sl.pred_len;
  for (int s = 0; s < c.num_scales; ++s) {
    ScaleState& S = e->sc[s];
    if (!S.use) continue;
    d2d(sl.dev + L.out_cls[s], S.out_cls.p, N * Tp * S.K * sizeof(float));
    d2d(sl.dev + L.out_reg[s], S.out_reg.p, N * Tp * S.K * 2 * sizeof(float));
  }
  HIP_CHECK(hipEventRecord(sl.done, e->stream));
  // fetch stream
  HIP_CHECK(hipStreamWaitEvent(e->fetch_stream, sl.done, 0));
  HIP_CHECK(hipMemcpyAsync(pin + L.in_bytes, sl.dev + L.in_bytes, L.out_bytes,
                           hipMemcpyDeviceToHost, e->fetch_stream));
  HIP_CHECK(hipEventRecord(sl.d2h, e->fetch_stream));
  sl.busy = true;
  e->pipe_head += 1;
}

void pipeline_collect(mv_engine* e, mv_outputs* out) {
  const mv_config& c = e->cfg;
  MV_REQUIRE(!e->pipe.empty(), "mv_pipeline_create has not been called");
  mv_engine::PipeSlot& sl = e->pipe[e->pipe_tail % e->pipe.size()];
  MV_REQUIRE(sl.busy, "mv_collect_greedy: nothing submitted");
  HIP_CHECK(hipEventSynchronize(sl.d2h));
  const PipeLayout L = pipe_layout(e);
  const char* pin = static_cast<const char*>(sl.pin);
  const size_t N = c.batch_size, Tp = sl.pred_len;
  for (int s = 0; s < c.num_scales; ++s) {
    ScaleState& S = e->sc[s];
    if (!S.use) continue;
    if (out->grid_pred_class[s])
      memcpy(out->grid_pred_class[s], pin + L.out_cls[s], N * Tp * S.K * sizeof(float));
    if (out->grid_pred_reg[s])
      memcpy(out->grid_pred_reg[s], pin + L.out_reg[s], N * Tp * S.K * 2 * sizeof(float));
  }
  sl.busy = false;
  e->pipe_tail += 1;
}

void download_beam(mv_engine* e, mv_beam_outputs* out) {
  const mv_config& c = e->cfg;
  const size_t N = c.batch_size, Tp = e->pred_len, B = c.beam_size;
  ScaleState& S = e->sc[beam_scale(e)];
  const size_t K = S.K;
  if (out->logits)
    HIP_CHECK(hipMemcpyAsync(out->logits, e->bm_out_logits.p, N * B * Tp * K * sizeof(float),
                             hipMemcpyDeviceToHost, e->stream));
  if (out->ids)
    HIP_CHECK(hipMemcpyAsync(out->ids, e->bm_out_ids.p, N * B * Tp * sizeof(int32_t),
                             hipMemcpyDeviceToHost, e->stream));
  if (out->logprobs)
    HIP_CHECK(hipMemcpyAsync(out->logprobs, e->bm_lp[0].p, N * B * sizeof(float),
                             hipMemcpyDeviceToHost, e->stream));
  if (out->grid_reg) {
    if (c.use_single_decoder)       // per beam: [N*B, T, K, 2]
      HIP_CHECK(hipMemcpyAsync(out->grid_reg, e->bm_out_reg.p,
                               N * B * Tp * K * 2 * sizeof(float), hipMemcpyDeviceToHost,
                               e->stream));
    else
    HIP_CHECK(hipMemcpyAsync(out->grid_reg, S.out_reg.p, N * Tp * K * 2 * sizeof(float),
                             hipMemcpyDeviceToHost, e->stream));
  }
  if (out->best_beam)  // logits[:, 0] -> [N, T, K]: rows n*B of [N,B,T,K]
    HIP_CHECK(hipMemcpy2DAsync(out->best_beam, Tp * K * sizeof(float),
                               e->bm_out_logits.p, B * Tp * K * sizeof(float),
                               Tp * K * sizeof(float), N, hipMemcpyDeviceToHost,
                               e->stream));
  HIP_CHECK(hipStreamSynchronize(e->stream));
}

// ---- multi-future decode of the last forward, on the device (multifuture_decode.h).  Both
// run on the handle's stream behind whatever forward was queued, copy their small result to
// the caller's buffer and synchronise.
static void mf_require_forward(const mv_engine* e, const char* who) {
  const mv_config& c = e->cfg;
  MV_REQUIRE(!(c.beam_size > 1 && c.use_single_decoder),
             "%s: use_single_decoder with beam search decodes on the host (the offsets come "
             "per beam, and the reference's own reshape of them mixes beams)", who);
  MV_REQUIRE(e->last != ForwardKind::None, "%s: no forward has run on this handle", who);
  MV_REQUIRE(e->last_on_beams() == (c.beam_size > 1),
             "%s: the last forward of this beam handle was a greedy one", who);
}

void decode_trajectories(mv_engine* e, int scale, int center_only, double* out) {
  const mv_config& c = e->cfg;
  MV_REQUIRE(out, "mv_decode_trajectories: NULL out");
  mf_require_forward(e, "mv_decode_trajectories");
  const bool beam = c.beam_size > 1;
  if (beam) scale = beam_scale(e);
  MV_REQUIRE(scale >= 0 && scale < c.num_scales && e->sc[scale].use,
             "mv_decode_trajectories: scale %d is not an enabled scale", scale);
  ScaleState& S = e->sc[scale];
  MV_REQUIRE(S.centers.p, "mv_set_grid_centers(%d) has not been called", scale);
  const int N = c.batch_size, B = c.beam_size, Tp = e->pred_len, K = S.K;
  const size_t rows = (size_t)N * B * Tp;
  e->mf_traj.alloc((size_t)N * B * c.max_pred_len * 2);
  const size_t grid = beam ? cdiv(rows, (size_t)mv::kMfBlock) : cdiv(rows, (size_t)mv::kMfWaves);
  const double bytes = beam ? rows * (4.0 + 16.0 + (center_only ? 16.0 : 24.0))
                            : rows * (4.0 * K + 16.0 + (center_only ? 16.0 : 24.0));
  launch(e, "decode_traj", center_only ? 0.0 : 2.0 * rows, bytes, [&] {
    // the last forward ran with per-row lengths: (0, 0) past a row's end
    const bool ragged = e->len.ragged;
    hipLaunchKernelGGL(ragged ? mv::decode_traj_kernel<true> : mv::decode_traj_kernel<false>,
                       dim3(grid), dim3(mv::kMfBlock), 0, e->stream,
                       beam ? e->bm_out_ids.p : nullptr, S.out_cls.p, S.out_reg.p, S.centers.p,
                       e->mf_traj.p, (int)rows, B, Tp, K, center_only,
                       ragged ? e->lens_dev.p : nullptr);
  });
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(out, e->mf_traj.p, rows * 2 * sizeof(double), hipMemcpyDeviceToHost,
                           e->stream));
  HIP_CHECK(hipStreamSynchronize(e->stream));
}

// K <= CPT * 256 cells: a thread's cells in registers (CPT 1 or 3); any K beyond
// Masked (mv_set_cell_mask): each future's step map is the softmax over the allowed cells
// Biased (mv_set_cell_bias; the kernels' MASKED form with the mask plane optional): of l + b
// (the occupancy kernels have no Motion and no Path form: beam_occupancy refuses before it asks)
template <bool RAGGED, RowForm F>
void launch_beam_occupancy(mv_engine* e, const float* lp, int N, int B, int Tp, int K) {
  static_assert(F <= RowForm::Biased, "the occupancy kernels come in the first three forms");
  constexpr bool MASKED = mv::row_has_bits(F), BIASED = mv::row_has_bias(F);
  const StepConstraints& con = e->con;
  const int Tcap = e->cfg.max_pred_len;
  const bool mask = MASKED && con.mask.set();
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(N * Tp), dim3(mv::kMfBlock), 0, e->stream, e->bm_out_logits.p,
                       lp, e->mf_occ.p, B, Tp, K, RAGGED ? e->lens_dev.p : nullptr,
                       mask ? con.mask.dev.p : (const uint8_t*)nullptr,
                       mask ? con.mask.stride(K, Tcap) : (int64_t)0,
                       mask ? con.mask.step(K) : (int64_t)0,
                       BIASED ? con.bias.dev.p : (const float*)nullptr,
                       BIASED ? con.bias.stride(K, Tcap) : (int64_t)0,
                       BIASED ? con.bias.step(K) : (int64_t)0);
  };
  if (K <= mv::kMfBlock) go(mv::beam_occupancy_kernel<1, RAGGED, MASKED, BIASED>);
  else if (K <= 3 * mv::kMfBlock) go(mv::beam_occupancy_kernel<3, RAGGED, MASKED, BIASED>);
  else go(mv::beam_occupancy_anyk_kernel<RAGGED, MASKED, BIASED>);
}

void beam_occupancy(mv_engine* e, float* out) {
  const mv_config& c = e->cfg;
  MV_REQUIRE(out, "mv_beam_occupancy: NULL out");
  MV_REQUIRE(c.beam_size > 1, "mv_beam_occupancy: engine was created with beam_size 1 (the "
             "occupancy map mixes the beams of a beam-search decode)");
  mf_require_forward(e, "mv_beam_occupancy");
  MV_REQUIRE(e->last != ForwardKind::Scored, "mv_beam_occupancy: the last forward scored given "
             "futures (mv_score_futures); a set of given futures is not a predictive mixture");
  // (a plane that depends on each future's path has no per-step map of the mixture: left out)
  const StepConstraints& con = e->con;
  MV_REQUIRE(!con.motion_set(), "mv_beam_occupancy: a motion cost is set (mv_set_motion_cost); the "
             "occupancy map under a path-dependent cost is not defined -- clear it first");
  MV_REQUIRE(!con.revisit_set(), "mv_beam_occupancy: a revisit cost is set (mv_set_revisit_cost); "
             "the occupancy map under a path-dependent cost is not defined -- clear it first");
  const ScaleState& S = e->sc[beam_scale(e)];
  const int N = c.batch_size, B = c.beam_size, Tp = e->pred_len, K = S.K;
  const size_t cells = (size_t)N * Tp * K;
  // the mask the forward chose its cells under, if it is still set (the forward checked it)
  const bool masked = con.mask.set();
  if (masked) {
    MV_REQUIRE(con.mask.tm == 1 || con.mask.tm >= Tp, "mv_beam_occupancy: the cell mask has "
               "Tm = %d planes, the last forward pred_len = %d steps", con.mask.tm, Tp);
    // the mask may have been set after the forward, which checked ITS mask: a step map over an
    // empty set would be 0 / 0
    const bool rag = e->len.ragged && e->lens_host.size() == (size_t)N;
    for (int n = 0; n < N; ++n)
      for (int t = 0; t < (rag ? e->lens_host[n] : Tp); ++t) {
        const int cnt = con.mask_count[(size_t)n * con.mask.tm + (con.mask.tm > 1 ? t : 0)];
        MV_REQUIRE(cnt >= 1, "mv_beam_occupancy: row n = %d has %d allowed cells at step t = %d "
                   "under the cell mask that is set now (mv_set_cell_mask)", n, cnt, t);
      }
  }
  // the bias that is set now, as the mask
  const RowForm form = row_form(masked, con.bias.set(), false, false);
  if (form == RowForm::Biased)
    MV_REQUIRE(con.bias.tm == 1 || con.bias.tm >= Tp, "mv_beam_occupancy: the cell bias has "
               "Tm = %d planes, the last forward pred_len = %d steps", con.bias.tm, Tp);
  e->mf_occ.alloc((size_t)N * c.max_pred_len * K);
  // HBM-bound: every beam's logits row read once, the map written once
  // independently sampled futures are draws, not scored hypotheses: uniform weights, which the
  // kernels form as softmax_b of all-zero scores (exp(0) / B, exactly 1 / B).  (Futures drawn
  // WITHOUT replacement are distinct: the model's own distribution renormalised over the drawn
  // set, softmax_b(logprobs), the beam's weighting.)
  const float* lp = e->bm_lp[0].p;
  if (e->last == ForwardKind::Sampled) {
    HIP_CHECK(hipMemsetAsync(e->bm_lp[1].p, 0, (size_t)N * B * sizeof(float), e->stream));
    lp = e->bm_lp[1].p;
  }
  launch(e, "beam_occupancy", 5.0 * cells * B, 4.0 * cells * (B + 1) + 4.0 * N * B, [&] {
    // the last forward ran with per-row lengths: 0 past a row's end
    with_row_form(form, [&](auto f) {
      constexpr RowForm F = decltype(f)::value;
      if constexpr (F <= RowForm::Biased) {
        if (e->len.ragged) launch_beam_occupancy<true, F>(e, lp, N, B, Tp, K);
        else launch_beam_occupancy<false, F>(e, lp, N, B, Tp, K);
      }
    });
  });
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(out, e->mf_occ.p, cells * sizeof(float), hipMemcpyDeviceToHost,
                           e->stream));
  HIP_CHECK(hipStreamSynchronize(e->stream));
}

void download_beam_ids(mv_engine* e, int32_t* ids, float* logprobs) {
  const mv_config& c = e->cfg;
  MV_REQUIRE(c.beam_size > 1, "mv_download_beam_ids: engine was created with beam_size 1");
  MV_REQUIRE(e->last_on_beams(), "mv_download_beam_ids: no beam forward has run on this handle");
  const size_t R = (size_t)c.batch_size * c.beam_size;
  if (ids)
    HIP_CHECK(hipMemcpyAsync(ids, e->bm_out_ids.p, R * e->pred_len * sizeof(int32_t),
                             hipMemcpyDeviceToHost, e->stream));
  if (logprobs)
    HIP_CHECK(hipMemcpyAsync(logprobs, e->bm_lp[0].p, R * sizeof(float), hipMemcpyDeviceToHost,
                             e->stream));
  HIP_CHECK(hipStreamSynchronize(e->stream));
}

const char* forward_kind_name(ForwardKind k) {
  switch (k) {
    case ForwardKind::None: return "none";
    case ForwardKind::Greedy: return "greedy";
    case ForwardKind::Beam: return "beam search";
    case ForwardKind::Sampled: return "independent samples";
    case ForwardKind::Scored: return "scoring";
    case ForwardKind::SampledWor: return "sampling without replacement";
  }
  return "?";
}

// the perturbed scores G [N, B] of a forward that sampled without replacement
void download_beam_gumbels(mv_engine* e, float* out) {
  const mv_config& c = e->cfg;
  MV_REQUIRE(out, "mv_download_beam_gumbels: NULL out");
  MV_REQUIRE(e->last == ForwardKind::SampledWor, "mv_download_beam_gumbels: the last forward of "
             "this handle was not one that sampled without replacement (mv_set_sampling + "
             "mv_set_sampling_mode 1); last forward: %s", forward_kind_name(e->last));
  const size_t R = (size_t)c.batch_size * c.beam_size;
  HIP_CHECK(hipMemcpyAsync(out, e->bm_g[0].p, R * sizeof(float), hipMemcpyDeviceToHost,
                           e->stream));
  HIP_CHECK(hipStreamSynchronize(e->stream));
}

// the futures' log-probability under the PROPOSAL [N, B] of a sampled forward:
// tempered and truncated, where logprobs is the model's own
void download_beam_proposal_logprobs(mv_engine* e, float* out) {
  const mv_config& c = e->cfg;
  MV_REQUIRE(out, "mv_download_beam_proposal_logprobs: NULL out");
  MV_REQUIRE(e->last == ForwardKind::Sampled || e->last == ForwardKind::SampledWor,
             "mv_download_beam_proposal_logprobs: the last forward of this handle was not a "
             "sampled one (mv_set_sampling); last forward: %s", forward_kind_name(e->last));
  const size_t R = (size_t)c.batch_size * c.beam_size;
  HIP_CHECK(hipMemcpyAsync(out, e->lq_acc.p, R * sizeof(float), hipMemcpyDeviceToHost,
                           e->stream));
  HIP_CHECK(hipStreamSynchronize(e->stream));
}

// ---- scoring of given futures (mv_score_futures)

// Checks the futures on the host and uploads them: ids with a valid cell at every step (a
// finished future inside a live sample keeps decoding on its last valid cell, a padding future
// on cell 0), the per-future lengths, and the per-sample maxima for the launch plan.
void upload_score_futures(mv_engine* e, const mv_score_futures_in* in) {
  const mv_config& c = e->cfg;
  MV_REQUIRE(in && in->ids, "mv_upload_score_futures: NULL futures");
  MV_REQUIRE(c.beam_size > 1, "mv_upload_score_futures: engine was created with beam_size 1 (a "
             "scoring forward scores beam_size futures per row: create a beam handle)");
  MV_REQUIRE(!c.use_single_decoder, "mv_upload_score_futures: use_single_decoder handles are "
             "not supported (the scoring forward keeps the un-beamed regression decoder)");
  MV_REQUIRE(e->inputs_ready, "mv_upload_score_futures: no inputs uploaded (mv_upload_inputs "
             "first: it sets pred_len)");
  MV_REQUIRE(!e->lens_set, "mv_upload_score_futures: per-row prediction lengths are set "
             "(mv_set_pred_lengths); the lengths of a scoring forward come with the futures -- "
             "clear them first");
  const int N = c.batch_size, F = c.beam_size, Tp = e->pred_len;
  const int K = e->sc[beam_scale(e)].K;
  const size_t R = (size_t)N * F;
  std::vector<int32_t> ids(R * Tp), lens(R);
  std::vector<int32_t> L(N, 0);
  bool uniform = true;
  for (int n = 0; n < N; ++n)
    for (int f = 0; f < F; ++f) {
      const size_t r = (size_t)n * F + f;
      const int len = in->lengths ? in->lengths[r] : Tp;
      MV_REQUIRE(len >= 0 && len <= Tp, "mv_upload_score_futures: lengths[%d, %d] = %d not in "
                 "[0, pred_len=%d]", n, f, len, Tp);
      lens[r] = len;
      L[n] = std::max(L[n], (int32_t)len);
      uniform = uniform && len == Tp;
      int32_t last = 0;
      for (int t = 0; t < Tp; ++t) {
        if (t < len) {
          last = in->ids[r * Tp + t];
          MV_REQUIRE(last >= 0 && last < K, "mv_upload_score_futures: ids[n=%d, f=%d, t=%d] = %d "
                     "out of range [0, %d)", n, f, t, last, K);
        }
        ids[r * Tp + t] = last;
      }
    }
  const size_t cap = R * (size_t)c.max_pred_len;
  e->score_ids.alloc(cap); e->score_len.alloc(R);
  e->score_step_lp.alloc(cap); e->score_rank.alloc(cap);
  // behind whatever forward still reads the previous futures on the device
  HIP_CHECK(hipStreamSynchronize(e->stream));
  HIP_CHECK(hipMemcpy(e->score_ids.p, ids.data(), ids.size() * sizeof(int32_t),
                      hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(e->score_len.p, lens.data(), R * sizeof(int32_t), hipMemcpyHostToDevice));
  e->score_L = L;
  e->score_uniform = uniform;
  e->score_pred_len = Tp;
  e->score_ready = true;
}

void download_scores(mv_engine* e, mv_score_outputs* out) {
  const mv_config& c = e->cfg;
  MV_REQUIRE(e->last == ForwardKind::Scored, "mv_download_scores: the last forward of "
             "this handle was not a scoring one (mv_run_score_resident)");
  const size_t R = (size_t)c.batch_size * c.beam_size, Tp = e->pred_len;
  if (out->step_logprobs)
    HIP_CHECK(hipMemcpyAsync(out->step_logprobs, e->score_step_lp.p, R * Tp * sizeof(float),
                             hipMemcpyDeviceToHost, e->stream));
  if (out->logprobs)
    HIP_CHECK(hipMemcpyAsync(out->logprobs, e->bm_lp[0].p, R * sizeof(float),
                             hipMemcpyDeviceToHost, e->stream));
  if (out->ranks)
    HIP_CHECK(hipMemcpyAsync(out->ranks, e->score_rank.p, R * Tp * sizeof(int32_t),
                             hipMemcpyDeviceToHost, e->stream));
  HIP_CHECK(hipStreamSynchronize(e->stream));
}

template <typename F>
int guarded(mv_engine* e, F&& fn) {
  try {
    if (e) HIP_CHECK(hipSetDevice(e->device));
    fn();
    return 0;
  } catch (const HipError& err) {
    if (e) e->err = err.msg; else g_create_error = err.msg;
    return 1;
  } catch (const std::exception& ex) {
    if (e) e->err = ex.what(); else g_create_error = ex.what();
    return 2;
  }
}

}  // namespace
