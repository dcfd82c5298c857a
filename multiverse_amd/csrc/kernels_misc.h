// The HBM-bound members of the Multiverse hot path: scene encoder, decoder
// input embeddings, graph attention, hidden2grid + argmax, beam expansion.
// Every kernel cites the reference lines it replaces.
#pragma once
#include <hip/hip_runtime.h>
#include "plane_layout.h"
#include "row_form.h"
#include <stdint.h>
#include <math.h>

namespace mv {

typedef float f32x4_t __attribute__((ext_vector_type(4)));

// f16x3 compute mode (convlstm_f16x3.h): a producer of a ConvLSTM operand can
// emit the two pre-scaled fp16 planes of its output next to the fp32 value, so
// that no separate split pass is needed.  p16 == nullptr: off.
// stride == 0 selects the bf16 mode: ONE plane holding bf16(v) (compute mode 2).
__device__ __forceinline__ _Float16 bf16_half_bits(float v) {
  uint32_t u = __builtin_bit_cast(uint32_t, v);
  if ((u & 0x7f800000u) != 0x7f800000u) u += 0x7fffu + ((u >> 16) & 1u);   // RNE
  return __builtin_bit_cast(_Float16, (uint16_t)(u >> 16));
}
__device__ __forceinline__ void emit_planes(_Float16* p16, size_t stride, size_t idx, int C,
                                            float v) {
  if (!p16) return;
  const size_t m = idx / (size_t)C;
  const size_t o = plane_index((long long)m, (int)(idx - m * C), C);
  if (stride == 0) { p16[o] = bf16_half_bits(v); return; }
  const float s = v * 256.0f;
  const _Float16 h0 = (_Float16)s;
  p16[o] = h0;
  p16[stride + o] = (_Float16)(s - (float)h0);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// ---------------------------------------------------------------- activation
// --activation_func of the reference (code/train.py:58-59 -> code/pred_utils.py:86-94):
// tanh (published), relu, lrelu = tf.nn.leaky_relu with its default alpha 0.2.  It is the
// activation of the scene convolutions (code/pred_models.py:155-165) and of grid_emb
// (:444, :664); the ConvLSTM cells and hidden2grid do not use it.  mv_config.activation.
constexpr int kActTanh = 0, kActRelu = 1, kActLrelu = 2;
__device__ __forceinline__ float act_apply(int act, float v) {
  if (act == kActTanh) return tanhf(v);
  if (act == kActRelu) return v > 0.f ? v : 0.f;
  return v > 0.f ? v : 0.2f * v;
}
// d act / d pre-activation from the OUTPUT y (lrelu: y > 0 <=> pre-activation > 0)
__device__ __forceinline__ float act_grad(int act, float y) {
  if (act == kActTanh) return 1.f - y * y;
  if (act == kActRelu) return y > 0.f ? 1.f : 0.f;
  return y > 0.f ? 1.f : 0.2f;
}

// ---------------------------------------------------------------- scene conv
// conv k x k, stride 2, SAME, + b, tanh (reference code/pred_models.py:155-160
// via conv2d :1333-1373) on the U unique frames of the batch; one thread per
// output element.  in [U, Hi, Wi, Ci], w [k,k,Ci,Co] HWIO, out [U, Ho, Wo, Co].
__global__ void scene_conv_s2_tanh_kernel(const float* __restrict__ in,
                                          const float* __restrict__ w,
                                          const float* __restrict__ b,
                                          float* __restrict__ out, int U, int Hi,
                                          int Wi, int Ci, int Ho, int Wo, int Co,
                                          int k, int pad_t, int pad_l, int act = 0) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)U * Ho * Wo * Co;
  if (idx >= total) return;
  const int co = idx % Co;
  size_t r = idx / Co;
  const int ox = r % Wo; r /= Wo;
  const int oy = r % Ho;
  const int u = r / Ho;
  float acc = 0.f;
  for (int ky = 0; ky < k; ++ky) {
    const int iy = oy * 2 + ky - pad_t;
    if (iy < 0 || iy >= Hi) continue;
    for (int kx = 0; kx < k; ++kx) {
      const int ix = ox * 2 + kx - pad_l;
      if (ix < 0 || ix >= Wi) continue;
      const float* ip = in + (((size_t)u * Hi + iy) * Wi + ix) * Ci;
      const float* wp = w + ((size_t)(ky * k + kx) * Ci) * Co + co;
      for (int ci = 0; ci < Ci; ++ci) acc = fmaf(ip[ci], wp[(size_t)ci * Co], acc);
    }
  }
  out[idx] = act_apply(act, acc + b[co]);
}

// The same convolution for k = 3, tiled (step_plan.h scene_conv_form decides).
// The kernel above walks one dependent fmaf chain per thread with a global input load and a
// strided global weight load in every link: its time is chain length x load latency.  Here a
// workgroup owns kSceneTilePix consecutive output pixels (flat over u, oy, ox) x all 64 output
// channels; thread = (pixel ps = tid / 16, channel quad cq = tid % 16), four adjacent co, so four
// independent chains per thread.  Per tap (ky, kx) the workgroup stages the tap's weights
// [Ci][64] and the 16 pixels' input vectors [Ci] in LDS -- the next tap's loads are issued into
// registers before the current tap is computed -- and every thread whose pixel has the tap in
// the image walks ci: one LDS broadcast read of the input, one 16-byte LDS read of the weights,
// four fmaf.  Each output's chain is the one of the kernel above: from 0.f, taps in ky, kx
// order, ci ascending, taps outside the image skipped, + b[co], act_apply: the same bits.
constexpr int kSceneTilePix = 16;      // output pixels per workgroup
constexpr int kSceneTileCo = 64;       // output channels: 16 threads x 4
constexpr int kSceneTileCiMax = 64;    // LDS: weights Ci x 64 floats (<= 16 KB) + inputs 16 x (Ci + 1)
__global__ __launch_bounds__(256)
void scene_conv3_s2_tiled_kernel(const float* __restrict__ in, const float* __restrict__ w,
                                 const float* __restrict__ b, float* __restrict__ out, int U,
                                 int Hi, int Wi, int Ci, int Ho, int Wo, int pad_t, int pad_l,
                                 int act) {
  constexpr int TP = kSceneTilePix, CO = kSceneTileCo, CIM = kSceneTileCiMax;
  constexpr int NX = TP * CIM / 256;             // staged input floats per thread, at most
  constexpr int NW = CIM * CO / 4 / 256;         // staged weight quads per thread, at most
  __shared__ __attribute__((aligned(16))) float wl[CIM * CO];
  __shared__ float xl[TP * (CIM + 1)];
  const int tid = threadIdx.x, cq = tid & 15, ps = tid >> 4;
  const int M = U * Ho * Wo;
  const int m0 = blockIdx.x * TP;
  // the thread's own pixel
  const int m = m0 + ps;
  int oy2 = 0, ox2 = 0;
  if (m < M) {
    const int ox = m % Wo, oy = (m / Wo) % Ho;
    oy2 = oy * 2 - pad_t; ox2 = ox * 2 - pad_l;
  }
  // the input elements this thread stages: element i = tid + 256 j is (pixel i / Ci, ci i % Ci)
  int sy2[NX], sx2[NX], sdst[NX];
  size_t sbase[NX];
  bool son[NX];
#pragma unroll
  for (int j = 0; j < NX; ++j) {
    const int i = tid + 256 * j;
    const int sp = i / Ci, sc = i - sp * Ci;
    const int sm = m0 + sp;
    son[j] = i < TP * Ci && sm < M;
    sy2[j] = sx2[j] = 0; sbase[j] = 0; sdst[j] = 0;
    if (son[j]) {
      const int ox = sm % Wo, r = sm / Wo, oy = r % Ho, u = r / Ho;
      sy2[j] = oy * 2 - pad_t; sx2[j] = ox * 2 - pad_l;
      sbase[j] = (size_t)u * Hi * Wi * Ci + sc;
      sdst[j] = sp * (Ci + 1) + sc;
    }
  }
  const int nwq = Ci * (CO / 4);                 // weight quads of one tap
  float xr[NX];
  f32x4_t wr[NW];
  auto fetch = [&](int tap) {
    const int ky = tap / 3, kx = tap - ky * 3;
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      const int iy = sy2[j] + ky, ix = sx2[j] + kx;
      xr[j] = (son[j] && iy >= 0 && iy < Hi && ix >= 0 && ix < Wi)
                  ? in[sbase[j] + ((size_t)iy * Wi + ix) * Ci] : 0.f;
    }
    const f32x4_t* wg = reinterpret_cast<const f32x4_t*>(w + (size_t)tap * Ci * CO);
#pragma unroll
    for (int j = 0; j < NW; ++j)
      if (tid + 256 * j < nwq) wr[j] = wg[tid + 256 * j];
  };
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  fetch(0);
  for (int tap = 0; tap < 9; ++tap) {
    if (tap) __syncthreads();                    // the previous tap's reads of LDS are done
#pragma unroll
    for (int j = 0; j < NX; ++j)
      if (son[j]) xl[sdst[j]] = xr[j];
#pragma unroll
    for (int j = 0; j < NW; ++j)
      if (tid + 256 * j < nwq) reinterpret_cast<f32x4_t*>(wl)[tid + 256 * j] = wr[j];
    __syncthreads();
    if (tap + 1 < 9) fetch(tap + 1);
    const int ky = tap / 3, kx = tap - ky * 3;
    const int iy = oy2 + ky, ix = ox2 + kx;
    if (m < M && iy >= 0 && iy < Hi && ix >= 0 && ix < Wi) {
      const float* xp = xl + ps * (Ci + 1);
      const f32x4_t* wp = reinterpret_cast<const f32x4_t*>(wl) + cq;
#pragma unroll 8
      for (int ci = 0; ci < Ci; ++ci) {
        const float xv = xp[ci];
        const f32x4_t wv = wp[ci * (CO / 4)];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = fmaf(xv, wv[j], acc[j]);
      }
    }
  }
  if (m >= M) return;
  const f32x4_t bv = reinterpret_cast<const f32x4_t*>(b)[cq];
  f32x4_t o;
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = act_apply(act, acc[j] + bv[j]);
  reinterpret_cast<f32x4_t*>(out + (size_t)m * CO)[cq] = o;
}

// --scene_conv_kernel 1 (code/train.py:65, conv2d code/pred_models.py:155-165): the scene
// stack degenerates to a strided 1x1 projection, a true dense GEMM
//   out[(u, oy, ox)][co] = tanh(sum_ci in[u, 2 oy, 2 ox, ci] W[ci][co] + b[co])
// (SAME padding of a 1x1 stride-2 conv is zero: the even input positions), M = U Ho Wo
// rows, K = Ci (11 / 64), N = Co <= 64 -- the one place BASELINE.json's north_star puts on
// the matrix cores.  v_mfma_f32_32x32x2_f32: exact fp32, the same ci-ordered fmaf chain as
// the generic kernel above.  A wave owns 32 rows x Co columns (two accumulators).
typedef float f32x16_t __attribute__((ext_vector_type(16)));
__global__ __launch_bounds__(256)
void scene_proj1x1_mfma_kernel(const float* __restrict__ in, const float* __restrict__ w,
                               const float* __restrict__ b, float* __restrict__ out, int U,
                               int Hi, int Wi, int Ci, int Ho, int Wo, int Co, int act = 0) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int M = U * Ho * Wo;
  const int m_wave = (blockIdx.x * 4 + wave) * 32;
  if (m_wave >= M) return;
  const int m = m_wave + (lane & 31);
  const int kh = lane >> 5;                       // which of the k-step's two channels
  size_t src = 0;
  if (m < M) {
    const int ox = m % Wo, r = m / Wo, oy = r % Ho, u = r / Ho;
    src = (((size_t)u * Hi + 2 * oy) * Wi + 2 * ox) * Ci;
  }
  f32x16_t acc0, acc1;
#pragma unroll
  for (int i = 0; i < 16; ++i) { acc0[i] = 0.f; acc1[i] = 0.f; }
  const int col = lane & 31;
  for (int kk = 0; kk < (Ci + 1) / 2; ++kk) {
    const int ci = 2 * kk + kh;
    const bool okc = ci < Ci;
    const float a = (okc && m < M) ? in[src + ci] : 0.f;
    const float b0 = (okc && col < Co) ? w[(size_t)ci * Co + col] : 0.f;
    const float b1 = (okc && 32 + col < Co) ? w[(size_t)ci * Co + 32 + col] : 0.f;
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc1, 0, 0, 0);
  }
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
    const int mm = m_wave + row;
    if (mm >= M) continue;
    if (col < Co) out[(size_t)mm * Co + col] = act_apply(act, acc0[reg] + b[col]);
    if (32 + col < Co) out[(size_t)mm * Co + 32 + col] = act_apply(act, acc1[reg] + b[32 + col]);
  }
}

// mean over the T_o observed frames of the per-sample scene feature
// (tf.reduce_mean(scene_features, axis=1), code/pred_models.py:826-828).
// conv [U, K, D] (K = H*W), obs_scene [N, T], out [N, K, D].
// obs_lens (mv_set_obs_lengths; NULL: every row has T frames): row n's mean is taken over its
// own last obs_lens[n] columns, in ascending time order, as an engine of that obs_len takes it.
__global__ void scene_mean_kernel(const float* __restrict__ conv,
                                  const int32_t* __restrict__ obs_scene,
                                  float* __restrict__ out, int N, int T, int K,
                                  int D, const int32_t* __restrict__ obs_lens) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t per = (size_t)K * D;
  if (idx >= (size_t)N * per) return;
  const int n = idx / per;
  const size_t off = idx - (size_t)n * per;
  float s = 0.f;
  if (!obs_lens) {
    for (int t = 0; t < T; ++t) s += conv[(size_t)obs_scene[n * T + t] * per + off];
    out[idx] = s / (float)T;
    return;
  }
  const int L = min(max(obs_lens[n], 1), T);      // (host-checked: in [1, T])
  for (int t = T - L; t < T; ++t) s += conv[(size_t)obs_scene[n * T + t] * per + off];
  out[idx] = s / (float)L;
}

// Rows that join the encoders at this step (mv_set_obs_lengths): their state rows are cleared
// in front of the gate launch, which then reads the zero state for them -- fp32 c and h [M][C]
// and the operand planes of h (plane_layout.h; p1 NULL: one plane, p0 NULL: none).
struct ZeroRowsJob { float* c; float* h; _Float16* p0; _Float16* p1; int K; };
struct ZeroRowsArgs {
  ZeroRowsJob job[4];
  const int32_t* rows;         // [nrows] the joining rows
  int nrows, C;
};
// One thread clears 8 channels of a cell (C % 32 == 0): two 16-byte stores per fp32 tensor, one
// per plane -- 8 channels of a cell are contiguous in the tiled plane layout.
__global__ void zero_state_rows_kernel(ZeroRowsArgs a) {
  const ZeroRowsJob j = a.job[blockIdx.y];
  const int C8 = a.C >> 3;
  const size_t per = (size_t)j.K * C8;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)a.nrows * per) return;
  const int i = (int)(idx / per);
  const size_t e = idx - (size_t)i * per;
  const size_t cell = e / C8;
  const int ch = (int)(e - cell * C8) * 8;
  const long long m = (long long)a.rows[i] * j.K + (long long)cell;
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float4* c4 = reinterpret_cast<float4*>(j.c + (size_t)m * a.C + ch);
  float4* h4 = reinterpret_cast<float4*>(j.h + (size_t)m * a.C + ch);
  c4[0] = z4; c4[1] = z4;
  h4[0] = z4; h4[1] = z4;
  const size_t o = plane_index(m, ch, a.C);
  const uint4 z8 = make_uint4(0u, 0u, 0u, 0u);
  if (j.p0) *reinterpret_cast<uint4*>(j.p0 + o) = z8;
  if (j.p1) *reinterpret_cast<uint4*>(j.p1 + o) = z8;
}

// Class-encoder input: scene feature masked to the occupied cell
// (tf.multiply(scene_convs[i], one_hot), code/pred_models.py:174-175,210).
// out [N, K, D] for time step t.
__global__ void enc_class_input_kernel(const float* __restrict__ conv,
                                       const int32_t* __restrict__ obs_scene,
                                       const int32_t* __restrict__ labels,
                                       float* __restrict__ out, int N, int T,
                                       int t, int K, int D, _Float16* p16 = nullptr,
                                       size_t p16_stride = 0,
                                       const int32_t* __restrict__ labels2 = nullptr,
                                       float mixw = 1.f) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t per = (size_t)K * D;
  if (idx >= (size_t)N * per) return;
  const int n = idx / per;
  const size_t off = idx - (size_t)n * per;
  const int cell = off / D;
  float v = 0.f;
  if (labels2) {
    // label mixup (SimAug/code/pred_models.py:616-636): the one-hot map is
    // w * one_hot(l1) + one_hot(l2) * (1 - w), then the same product
    const float m = mixw * (cell == labels[n * T + t] ? 1.f : 0.f) +
                    (cell == labels2[n * T + t] ? 1.f : 0.f) * (1.f - mixw);
    if (m != 0.f) v = conv[(size_t)obs_scene[n * T + t] * per + off] * m;
  } else if (cell == labels[n * T + t])
    v = conv[(size_t)obs_scene[n * T + t] * per + off];
  out[idx] = v;
  emit_planes(p16, p16_stride, idx, D, v);
}

// ---------------------------------------------------------------- grid_emb
// tanh(conv3x3_SAME(x) + b), P in {1,2} input channels, E outputs
// (grid_emb, code/pred_models.py:912-919).  Dense form, one thread per output.
// x [M, H, W, P] with row stride x_row_stride (elements) so a time slice of a
// [N, T, H, W, P] tensor can be embedded without a copy.
__global__ void grid_emb_dense_kernel(const float* __restrict__ x,
                                      size_t x_row_stride,
                                      const float* __restrict__ w,
                                      const float* __restrict__ b,
                                      float* __restrict__ out, int M, int H,
                                      int W, int P, int E, _Float16* p16 = nullptr,
                                      size_t p16_stride = 0, int act = 0) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)M * H * W * E;
  if (idx >= total) return;
  const int e = idx % E;
  size_t r = idx / E;
  const int xx = r % W; r /= W;
  const int yy = r % H;
  const int m = r / H;
  float acc = 0.f;
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = yy + ky - 1;
    if (iy < 0 || iy >= H) continue;
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = xx + kx - 1;
      if (ix < 0 || ix >= W) continue;
      const float* ip = x + (size_t)m * x_row_stride + ((size_t)iy * W + ix) * P;
      for (int p = 0; p < P; ++p)
        acc = fmaf(ip[p], w[((ky * 3 + kx) * P + p) * E + e], acc);
    }
  }
  const float v = act_apply(act, acc + b[e]);
  out[idx] = v;
  emit_planes(p16, p16_stride, idx, E, v);
}

// One-hot input in closed form: the cell at offset (dy,dx) from the hot cell
// sees exactly tap (1-dy, 1-dx); every other cell sees tanh(b).
// (grid_emb of tf.one_hot(argmax), code/pred_models.py:411-425, 442-446,
// 602-606.)  Row m reads ids[(m / ids_div) * ids_stride], so the obs labels
// [N,T] column T-1, tiled over beams (ids_div = B), or per-beam ids are used in
// place.  out [M, H, W, E].
__global__ void grid_emb_onehot_kernel(const int32_t* __restrict__ ids,
                                       int ids_stride, int ids_div,
                                       const float* __restrict__ w,
                                       const float* __restrict__ b,
                                       float* __restrict__ out, int M, int H,
                                       int W, int E, _Float16* p16 = nullptr,
                                       size_t p16_stride = 0, int act = 0) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)M * H * W * E;
  if (idx >= total) return;
  const int e = idx % E;
  size_t r = idx / E;
  const int xx = r % W; r /= W;
  const int yy = r % H;
  const int m = r / H;
  const int id = ids[(size_t)(m / ids_div) * ids_stride];
  const int py = id / W, px = id - py * W;
  const int dy = yy - py, dx = xx - px;
  float acc = 0.f;
  if (dy >= -1 && dy <= 1 && dx >= -1 && dx <= 1)
    acc = w[((1 - dy) * 3 + (1 - dx)) * E + e];  // P == 1
  const float v = act_apply(act, acc + b[e]);
  out[idx] = v;
  emit_planes(p16, p16_stride, idx, E, v);
}

// Class-encoder input of a model built WITHOUT the scene encoder (code/pred_models.py:218-229):
// x_t = act(grid_emb(one_hot(labels[:, t])) + b) through the ONE person_pred/grid_emb shared by
// the scales, in the closed form of grid_emb_onehot_kernel, for the steps t0 .. t0 + nsteps - 1
// in one launch: out [nsteps][N][H][W][E] time-major (the training chain's x of every step, or
// one step of the inference x buffer with its operand planes through p16).  labels [N][T].
__global__ void enc_grid_emb_onehot_kernel(const int32_t* __restrict__ labels, int T, int t0,
                                           int nsteps, const float* __restrict__ w,
                                           const float* __restrict__ b,
                                           float* __restrict__ out, int N, int H, int W, int E,
                                           _Float16* p16 = nullptr, size_t p16_stride = 0,
                                           int act = 0) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int K = H * W;
  const size_t total = (size_t)nsteps * N * K * E;
  if (idx >= total) return;
  const int e = idx % E;
  size_t r = idx / E;
  const int cell = r % K; r /= K;
  const int n = r % N;
  const int ts = r / N;
  const int id = labels[(size_t)n * T + t0 + ts];
  const int py = id / W, px = id - py * W;
  const int yy = cell / W, xx = cell - yy * W;
  const int dy = yy - py, dx = xx - px;
  float acc = 0.f;
  if (dy >= -1 && dy <= 1 && dx >= -1 && dx <= 1)
    acc = w[((1 - dy) * 3 + (1 - dx)) * E + e];
  const float v = act_apply(act, acc + b[e]);
  out[idx] = v;
  emit_planes(p16, p16_stride, idx, E, v);
}

// Weight gradient of that embedding: a 3x3 conv whose input is one-hot sees tap (ky, kx) only
// at the cell hot - (ky - 1, kx - 1), so
//   dW[ky][kx][e] = sum over (t, n) of dpre[t][n][hot(n, t) - (ky - 1, kx - 1)][e]
// (cells outside the image skipped): 9 cells per map instead of the whole grid.  dpre
// [T][N][H][W][E] time-major (d pre-activation), labels [N][T].  One workgroup per (tap, 32
// columns): 8 row groups of 32 lanes sum rows m = g, g + 8, .. in order, then the 8 partials
// are added in a fixed order -- bitwise reproducible.  accumulate: dw += the sum (the second
// scale onto the first: the encoders of both scales share the variable).
constexpr int kEmbWgradGroups = 8;
__global__ __launch_bounds__(256)
void grid_emb_onehot_wgrad_kernel(const float* __restrict__ dpre,
                                  const int32_t* __restrict__ labels, int N, int T, int H,
                                  int W, int E, float* __restrict__ dw, int accumulate) {
  __shared__ float part[kEmbWgradGroups][32];
  const int tap = blockIdx.x, ky = tap / 3, kx = tap - ky * 3;
  const int lane = threadIdx.x & 31, g = threadIdx.x >> 5;
  const int e = blockIdx.y * 32 + lane;      // E is a multiple of 32 (validate_config)
  const int K = H * W, M = T * N;
  float s = 0.f;
  for (int m = g; m < M; m += kEmbWgradGroups) {
    const int t = m / N, n = m - t * N;
    const int id = labels[(size_t)n * T + t];
    const int py = id / W, px = id - py * W;
    const int y = py - (ky - 1), x = px - (kx - 1);
    if (y < 0 || y >= H || x < 0 || x >= W) continue;
    s += dpre[((size_t)m * K + (size_t)y * W + x) * E + e];
  }
  part[g][lane] = s;
  __syncthreads();
  if (g != 0) return;
  float tot = part[0][lane];
  for (int i = 1; i < kEmbWgradGroups; ++i) tot += part[i][lane];
  float* dst = dw + (size_t)tap * E + e;
  *dst = accumulate ? *dst + tot : tot;
}

// ---------------------------------------------------------------- graph attention
// h_out = h + sum_j softmax_j(<f_i, f_j>) h_j over the <= 9 in-bounds 3x3
// neighbours, f = l2_normalize([h ; scene_mean]).  The reference builds the
// dense K x K edge matrix, adds -1e30 off the neighbourhood and softmaxes
// (gnn_edge / gnn_mask_edge / gnn_node, code/pred_models.py:808-909,
// exp_mask :1399-1401); exp(-1e30 - max) is exactly 0 in fp32, so the 9-point
// stencil is the same function.  One wave per cell: lane l holds channels
// 256 g + 4l..4l+3 of h (NG groups: C <= 256 NG) and channels l, l + 64 of the scene mean
// (D <= 128).
// scene_mean rows are indexed by m / sm_div (beam tiling, :831-834).
// src_row: optional state-row indirection (beam parents): input row for
// output row r is src_row[r].
// Channel groups of the one-wave-per-cell kernels: lane l owns channels 256 g + 4 l .. + 3 of
// group g < NG (C <= 256 NG: hidden sizes 128 / 256 / 512; lanes past C idle with zeros).
template <int NG>
struct CVec {
  f32x4_t v[NG];
};
template <int NG>
__device__ __forceinline__ CVec<NG> cvec_load(const float* __restrict__ row, int lane, int C) {
  CVec<NG> r;
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int c0 = g * 256 + lane * 4;
    r.v[g] = c0 < C ? *reinterpret_cast<const f32x4_t*>(row + c0) : f32x4_t{0.f, 0.f, 0.f, 0.f};
  }
  return r;
}
// the scene part of a cell's feature in the one-wave-per-cell kernels: lane l owns scene
// channels l and l + 64 (--scene_conv_dim up to 128; the published 64 leaves .b zero)
struct SVec { float a, b; };
__device__ __forceinline__ SVec svec_load(const float* __restrict__ row, int lane, int D) {
  SVec r;
  r.a = lane < D ? row[lane] : 0.f;
  r.b = lane + 64 < D ? row[lane + 64] : 0.f;
  return r;
}
__device__ __forceinline__ float svec_dot(const SVec& x, const SVec& y) {
  return x.a * y.a + x.b * y.b;
}
template <int NG>
__device__ __forceinline__ float cvec_dot(const CVec<NG>& a, const CVec<NG>& b) {
  float s = 0.f;
#pragma unroll
  for (int g = 0; g < NG; ++g)
    s += a.v[g][0] * b.v[g][0] + a.v[g][1] * b.v[g][1] + a.v[g][2] * b.v[g][2] +
         a.v[g][3] * b.v[g][3];
  return s;
}

template <int NG>
__global__ __launch_bounds__(256)
void gnn_attend_kernel(const float* __restrict__ h,
                       const float* __restrict__ scene_mean,
                       const int32_t* __restrict__ src_row,
                       float* __restrict__ out, int M, int H, int W, int C,
                       int D, int sm_div, _Float16* p16 = nullptr, size_t p16_stride = 0) {
  const int lane = threadIdx.x & 63;
  const size_t cell_id = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int K = H * W;
  if (cell_id >= (size_t)M * K) return;
  const int m = cell_id / K;
  const int cell = cell_id - (size_t)m * K;
  const int y = cell / W, x = cell - y * W;
  const int ms = src_row ? src_row[m] : m;
  const float* hrow = h + (size_t)ms * K * C;
  const float* srow = scene_mean + (size_t)(m / sm_div) * K * D;

  const CVec<NG> hi = cvec_load<NG>(hrow + (size_t)cell * C, lane, C);
  const SVec si = svec_load(srow + (size_t)cell * D, lane, D);
  float ssi = cvec_dot<NG>(hi, hi) + svec_dot(si, si);
  ssi = wave_sum(ssi);
  const float invi = rsqrtf(fmaxf(ssi, 1e-12f));

  CVec<NG> hj[9];
  float e[9];
  bool ok[9];
  float emax = -INFINITY;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
    ok[t] = (yy >= 0 && yy < H && xx >= 0 && xx < W);
    e[t] = 0.f;
#pragma unroll
    for (int g = 0; g < NG; ++g) hj[t].v[g] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    if (ok[t]) {  // wave-uniform
      const int cj = yy * W + xx;
      hj[t] = cvec_load<NG>(hrow + (size_t)cj * C, lane, C);
      const SVec sj = svec_load(srow + (size_t)cj * D, lane, D);
      float ssj = cvec_dot<NG>(hj[t], hj[t]) + svec_dot(sj, sj);
      float dot = cvec_dot<NG>(hi, hj[t]) + svec_dot(si, sj);
      ssj = wave_sum(ssj);
      dot = wave_sum(dot);
      e[t] = dot * invi * rsqrtf(fmaxf(ssj, 1e-12f));
      emax = fmaxf(emax, e[t]);
    }
  }
  float den = 0.f;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    e[t] = ok[t] ? expf(e[t] - emax) : 0.f;
    den += e[t];
  }
  const float inv = 1.0f / den;
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int c0 = g * 256 + lane * 4;
    if (c0 >= C) continue;
    f32x4_t node = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const float a = e[t] * inv;
      node[0] = fmaf(a, hj[t].v[g][0], node[0]);
      node[1] = fmaf(a, hj[t].v[g][1], node[1]);
      node[2] = fmaf(a, hj[t].v[g][2], node[2]);
      node[3] = fmaf(a, hj[t].v[g][3], node[3]);
    }
    f32x4_t o = {hi.v[g][0] + node[0], hi.v[g][1] + node[1], hi.v[g][2] + node[2],
                 hi.v[g][3] + node[3]};
    *reinterpret_cast<f32x4_t*>(out + ((size_t)m * K + cell) * C + c0) = o;
    if (p16) {
      typedef _Float16 f16x4_t __attribute__((ext_vector_type(4)));
      f16x4_t a, b;
      const size_t idx = plane_index((long long)m * K + cell, c0, C);   // 4 of one 8-group
      if (p16_stride == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = bf16_half_bits(o[j]);
        *reinterpret_cast<f16x4_t*>(p16 + idx) = a;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float sc = o[j] * 256.0f;
          const _Float16 h0 = (_Float16)sc;
          a[j] = h0;
          b[j] = (_Float16)(sc - (float)h0);
        }
        *reinterpret_cast<f16x4_t*>(p16 + idx) = a;
        *reinterpret_cast<f16x4_t*>(p16 + p16_stride + idx) = b;
      }
    }
  }
}

// ---- graph attention, second version: LDS-tiled.
// The first version (above) gives one wave to a cell: it gathers the nine neighbours'
// 1.25 KB feature vectors from global memory (9x the L1/L2 traffic of the tensor) and
// spends most of its instructions in 19 wave-wide reductions per cell; measured 1.2 TB/s
// of algorithmic bytes (profiles/r2_*).  Here a workgroup owns 32 consecutive cells of
// the flat [rows*K] index (= one operand-plane tile row) and stages the contiguous range
// of cells that holds every in-image neighbour (32 + 2W + 2 <= 98 cells) through LDS in
// chunks of 64 channels:
//   pass 1  (4 chunks of h + 1 of scene_mean)  partial dot products: thread = (cell,
//           8-channel slice) accumulates its 9 dots over the chunks; |u|^2 of every staged
//           cell the same way; 8-lane shuffles at the end -> e_ij, softmax weights in LDS;
//   pass 2  (4 chunks of h again, an L2 hit)   out = h_i + sum_j a_ij h_j: thread = (cell,
//           8 channels), results leave as 16-byte operand-plane vectors (1 KB contiguous
//           per wave) and, when a consumer needs them, fp32 rows.
// Consecutive 32-cell groups are mapped to the same XCD (block % 8 -> contiguous range of
// groups) so that a group's halo cells are its neighbours' own cells in that L2.
constexpr int kGnnPitch = 68;        // floats per staged cell and chunk (64 + 4: bank spread)
// cells per workgroup: MV_GNN_CELLS = 32 (256 threads, 98 staged cells: every staged byte is
// read 3.1 x per pass) or 64 (512 threads, 130 staged cells: 2.0 x).  Same arithmetic per cell
// in the same order: bitwise the same result.  Measured (beam 20, 2 560 rows, same box): 64
// cells 16.7 ms per forward, 32 cells 15.8 -- the kernel is not bound by its L2 re-reads.
#ifndef MV_GNN_CELLS
#define MV_GNN_CELLS 32
#endif
constexpr int kGnnCells = MV_GNN_CELLS;
constexpr int kGnnThreads = kGnnCells * 8;
constexpr int kGnnStage = kGnnCells + 2 * 32 + 2;   // + a halo of W + 1 <= 33 cells each side

// One launch serves up to two problems (the two grid scales of a greedy decode step):
// blocks [0, nblocks0) belong to p[0], the rest to p[1]; both counts are multiples of 8,
// so the block -> XCD mapping below holds for each.
struct GnnProblem {
  const float* h; const float* scene_mean; const int32_t* src_row; float* out;
  _Float16* p16; size_t p16_stride;
  int M, H, W, sm_div, ngroups;
  const int32_t* row_ref;   // optional [M]: rows with 0 are not computed (no beam continues them)
};
struct GnnGroup { GnnProblem p[2]; unsigned nblocks0; };

__global__ __launch_bounds__(kGnnThreads)
void gnn_attend_v2_kernel(const GnnGroup grp, int C, int D) {
  __shared__ __attribute__((aligned(16))) float buf[kGnnStage * kGnnPitch];
  __shared__ float ssq[kGnnStage];
  __shared__ float edot[kGnnCells * 9];
  __shared__ float alpha[kGnnCells * 9];
  __shared__ int hsrc[kGnnStage], ssrc[kGnnStage];
  const bool second = blockIdx.x >= grp.nblocks0;
  const GnnProblem& pr = grp.p[second ? 1 : 0];
  const unsigned blk = second ? blockIdx.x - grp.nblocks0 : blockIdx.x;
  const float* __restrict__ h = pr.h;
  const float* __restrict__ scene_mean = pr.scene_mean;
  const int32_t* __restrict__ src_row = pr.src_row;
  float* __restrict__ out = pr.out;
  _Float16* p16 = pr.p16;
  const size_t p16_stride = pr.p16_stride;
  const int M = pr.M, H = pr.H, W = pr.W, sm_div = pr.sm_div, ngroups = pr.ngroups;
  const int per = (ngroups + 7) >> 3;
  const int g = (blk & 7) * per + (blk >> 3);
  if (g >= ngroups) return;
  const int tid = threadIdx.x;
  const int K = H * W;
  const long long Mtot = (long long)M * K;
  const long long m0 = (long long)g * kGnnCells;
  if (pr.row_ref) {     // beam decode: skip the rows no surviving beam descends from
    const long long mlast = m0 + kGnnCells - 1 < Mtot ? m0 + kGnnCells - 1 : Mtot - 1;
    bool any = false;
    for (long long r = m0 / K; r <= mlast / K; ++r) any |= pr.row_ref[r] != 0;
    if (!any) return;
  }
  const long long s0 = m0 - W - 1 > 0 ? m0 - W - 1 : 0;
  const long long s1 = m0 + kGnnCells + W + 1 < Mtot ? m0 + kGnnCells + W + 1 : Mtot;
  const int NS = (int)(s1 - s0);
  if (tid < NS) {
    const long long m = s0 + tid;
    const int r = (int)(m / K), c = (int)(m - (long long)r * K);
    hsrc[tid] = (src_row ? src_row[r] : r) * K + c;
    ssrc[tid] = (r / sm_div) * K + c;
    ssq[tid] = 0.f;
  }
  // pass-1 role: own cell i1 = tid >> 3, channel slice sl = tid & 7
  const int i1 = tid >> 3, sl = tid & 7;
  // pass-2 role: own cell i2 = tid % cells, channel group c8 = tid / cells
  const int i2 = tid % kGnnCells, c8 = tid / kGnnCells;
  auto cell_info = [&](int i, int& li, int& mask) {
    const long long m = m0 + i;
    li = (int)(m - s0);
    mask = 0;
    if (m < Mtot) {
      const int c = (int)(m % K);
      const int y = c / W, x = c - y * W;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) mask |= 1 << t;
      }
    }
  };
  int li1, mask1, li2, mask2;
  cell_info(i1, li1, mask1);
  cell_info(i2, li2, mask2);

  // A chunk travels global -> registers -> LDS; the loads of chunk q+1 are issued
  // before chunk q is computed on, so their HBM / L2 latency runs under the compute
  // phase.  (First version: load -> wait -> store inside a run-time loop: seven
  // serialised round trips per chunk, 48 us per workgroup.)
  constexpr int kIt = (kGnnStage * 16 + kGnnThreads - 1) / kGnnThreads;     // 7 (32 cells) / 5 (64)
  f32x4_t val[kIt];
  auto stage_load = [&](int q) {     // q < 4: channels q*64.. of h; q == 4: scene_mean
#pragma unroll
    for (int k = 0; k < kIt; ++k) {
      const int v = tid + k * kGnnThreads;
      const int ls = v >> 4, part = v & 15;
      val[k] = f32x4_t{0.f, 0.f, 0.f, 0.f};
      if (v < NS * 16) {
        if (q < 4) {
          val[k] = *reinterpret_cast<const f32x4_t*>(h + (size_t)hsrc[ls] * C + q * 64 + part * 4);
        } else if (D == 64) {
          val[k] = *reinterpret_cast<const f32x4_t*>(scene_mean + (size_t)ssrc[ls] * 64 + part * 4);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            val[k][j] = (part * 4 + j < D) ? scene_mean[(size_t)ssrc[ls] * D + part * 4 + j] : 0.f;
        }
      }
    }
  };
  auto stage_store = [&]() {
#pragma unroll
    for (int k = 0; k < kIt; ++k) {
      const int v = tid + k * kGnnThreads;
      if (v < NS * 16)
        *reinterpret_cast<f32x4_t*>(&buf[(v >> 4) * kGnnPitch + (v & 15) * 4]) = val[k];
    }
  };
  auto dot8 = [&](const float* a, const float* b) {
    const f32x4_t a0 = *reinterpret_cast<const f32x4_t*>(a), a1 = *reinterpret_cast<const f32x4_t*>(a + 4);
    const f32x4_t b0 = *reinterpret_cast<const f32x4_t*>(b), b1 = *reinterpret_cast<const f32x4_t*>(b + 4);
    float d = a0[0] * b0[0];
    d = fmaf(a0[1], b0[1], d); d = fmaf(a0[2], b0[2], d); d = fmaf(a0[3], b0[3], d);
    d = fmaf(a1[0], b1[0], d); d = fmaf(a1[1], b1[1], d); d = fmaf(a1[2], b1[2], d);
    d = fmaf(a1[3], b1[3], d);
    return d;
  };

  float pd[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) pd[t] = 0.f;
  __syncthreads();                    // hsrc / ssrc / ssq visible
  const int nchunk = D > 0 ? 5 : 4;
  stage_load(0);
  for (int q = 0; q < nchunk; ++q) {
    stage_store();
    __syncthreads();
    stage_load(q + 1 < nchunk ? q + 1 : 0);   // next chunk; after the last: pass 2's first
    if (mask1) {
      const float* fi = &buf[li1 * kGnnPitch + sl * 8];
#pragma unroll
      for (int t = 0; t < 9; ++t)
        if ((mask1 >> t) & 1)
          pd[t] += dot8(fi, &buf[(li1 + (t / 3 - 1) * W + (t % 3 - 1)) * kGnnPitch + sl * 8]);
    }
    for (int base = 0; base < NS * 8; base += kGnnThreads) {     // |u|^2 of every staged cell
      const int idx = base + tid;
      const int ls = idx >> 3;
      float pp = 0.f;
      if (idx < NS * 8) {
        const float* f = &buf[ls * kGnnPitch + sl * 8];
        pp = dot8(f, f);
      }
      pp += __shfl_xor(pp, 1, 64);
      pp += __shfl_xor(pp, 2, 64);
      pp += __shfl_xor(pp, 4, 64);
      if (idx < NS * 8 && sl == 0) ssq[ls] += pp;        // one writer per staged cell
    }
    __syncthreads();
  }
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    float v = pd[t];
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    if (sl == 0) edot[i1 * 9 + t] = v;
  }
  __syncthreads();
  if (tid < kGnnCells) {              // softmax over the in-image neighbours of cell tid
    int li, mask;
    cell_info(tid, li, mask);
    float e[9];
    float emax = -INFINITY;
    const float invi = mask ? rsqrtf(fmaxf(ssq[li], 1e-12f)) : 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      e[t] = 0.f;
      if ((mask >> t) & 1) {
        const int lj = li + (t / 3 - 1) * W + (t % 3 - 1);
        e[t] = edot[tid * 9 + t] * invi * rsqrtf(fmaxf(ssq[lj], 1e-12f));
        emax = fmaxf(emax, e[t]);
      }
    }
    float den = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      e[t] = ((mask >> t) & 1) ? expf(e[t] - emax) : 0.f;
      den += e[t];
    }
    const float inv = 1.0f / den;
#pragma unroll
    for (int t = 0; t < 9; ++t) alpha[tid * 9 + t] = e[t] * inv;
  }
  __syncthreads();
  const long long m2 = m0 + i2;
  for (int q = 0; q < 4; ++q) {
    stage_store();
    __syncthreads();
    if (q < 3) stage_load(q + 1);
    if (mask2) {
      const float* hi = &buf[li2 * kGnnPitch + c8 * 8];
      float node[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) node[j] = 0.f;
#pragma unroll
      for (int t = 0; t < 9; ++t)
        if ((mask2 >> t) & 1) {
          const float a = alpha[i2 * 9 + t];
          const float* hj = &buf[(li2 + (t / 3 - 1) * W + (t % 3 - 1)) * kGnnPitch + c8 * 8];
          const f32x4_t h0 = *reinterpret_cast<const f32x4_t*>(hj);
          const f32x4_t h1 = *reinterpret_cast<const f32x4_t*>(hj + 4);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            node[j] = fmaf(a, h0[j], node[j]);
            node[4 + j] = fmaf(a, h1[j], node[4 + j]);
          }
        }
      const f32x4_t s0v = *reinterpret_cast<const f32x4_t*>(hi);
      const f32x4_t s1v = *reinterpret_cast<const f32x4_t*>(hi + 4);
      float o[8];
#pragma unroll
      for (int j = 0; j < 4; ++j) { o[j] = s0v[j] + node[j]; o[4 + j] = s1v[j] + node[4 + j]; }
      const int ch = q * 64 + c8 * 8;
      if (out) {
        f32x4_t* dst = reinterpret_cast<f32x4_t*>(out + (size_t)m2 * C + ch);
        dst[0] = f32x4_t{o[0], o[1], o[2], o[3]};
        dst[1] = f32x4_t{o[4], o[5], o[6], o[7]};
      }
      if (p16) {
        typedef _Float16 h8 __attribute__((ext_vector_type(8)));
        h8 pa, pb;
        const size_t idx = plane_index(m2, ch, C);
        if (p16_stride == 0) {
#pragma unroll
          for (int j = 0; j < 8; ++j) pa[j] = bf16_half_bits(o[j]);
          *reinterpret_cast<h8*>(p16 + idx) = pa;
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float sc = o[j] * 256.0f;
            const _Float16 h0h = (_Float16)sc;
            pa[j] = h0h;
            pb[j] = (_Float16)(sc - (float)h0h);
          }
          *reinterpret_cast<h8*>(p16 + idx) = pa;
          *reinterpret_cast<h8*>(p16 + p16_stride + idx) = pb;
        }
      }
    }
    __syncthreads();
  }
}
static inline unsigned gnn_v2_blocks(size_t cells, int* ngroups) {
  const size_t g = (cells + kGnnCells - 1) / kGnnCells;
  *ngroups = (int)g;
  return (unsigned)(((g + 7) / 8) * 8);
}

// ---- graph attention, third version: the same two-pass scheme, register-blocked, with the
// staging done by the LDS-DMA.
// The second version is bound by its LDS reads, not by memory: every thread owns ONE cell
// and reads ten staged vectors (itself + 9 neighbours) for 72 FMAs -- 26.9 KB of LDS reads
// per cell over the two passes plus 7 KB of staging writes -- and a chunk travels global ->
// registers -> LDS, 28 registers per thread that live across the whole compute phase.
// Here a workgroup of 256 threads owns 64 consecutive cells of the flat index (<= 128
// staged) and a thread owns several ADJACENT cells, so a row of staged vectors is shared:
//   pass 1  thread = (4 cells, 4 channels of the 64-channel chunk): 18 16-byte LDS reads
//           feed the 36 dot products of the quad (v2: 40 reads of twice the channels); the
//           16 channel slices of a cell are 16 consecutive lanes, folded once, after the
//           last chunk, with four DPP adds per value.  |u|^2 of an owned cell is its self
//           dot product; the <= 64 halo cells get theirs from four more reads per thread,
//           computed exactly the way their owner computes it (same chain, same fold);
//   pass 2  thread = (2 cells, 8 channels): 24 reads for 144 FMAs, 16-byte plane stores.
// 13 KB of LDS reads per cell and no staging writes by the waves: chunk q + 1 is copied
// global -> LDS by the DMA (16 bytes per lane, lane-linear destination) into the second
// of two tiles while the waves compute on chunk q; one barrier per chunk.
// LDS tile: 128 cells x 256 bytes, no pad.  Pass 1: part p of staged cell l at l*256 + p*16:
// its readers (16 consecutive lanes = the 16 parts of one cell) are conflict-free and every
// read is one of three row bases + an immediate; a window may reach one cell past its tile
// -- the other tile, or the small arrays behind them -- where it reads garbage that only
// ever feeds dot products of out-of-image neighbours, which nothing uses.  Pass 2: the lane that fills slot p of cell l fetches part
// p ^ ((l >> 1) & 15) instead, which makes the pass-2 pattern (16 consecutive lanes = 16
// consecutive cell pairs, same part) hit 16 different bank groups; reads are clamped into
// the tile, every slot of which holds a real cell (indices are clamped into the tensor): an
// out-of-image neighbour is a finite value times a weight of exactly 0.
// Arithmetic per cell depends only on the cell's data, not on where the cell sits in its
// workgroup (the engine's A/B tests compare layouts bit for bit).
constexpr int kGnn3Cells = 64;
constexpr int kGnn3Threads = 256;
constexpr int kGnn3Stage = kGnn3Cells + 2 * 32;       // halo: W (+ 1 unless W divides 64) per side
constexpr int kGnn3It = kGnn3Stage * 16 / kGnn3Threads;   // 8 DMA pieces per thread and chunk
constexpr int kGnn3Tile = kGnn3Stage * 64;            // floats per chunk tile
constexpr int kGnn3Small = 1024;                      // floats behind the tiles: e_ij / weights, |u|^2, row maps
static_assert(kGnn3Stage * 16 % kGnn3Threads == 0, "the DMA pieces cover the tile exactly");

template <int CTRL>
__device__ __forceinline__ float dpp_lane_f(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
// Sum over the 16 lanes of a DPP row; every lane of the row ends with the total.  All 16
// lanes must be active.
__device__ __forceinline__ float row16_sum(float v) {
  v += dpp_lane_f<0xB1>(v);     // quad_perm [1,0,3,2]
  v += dpp_lane_f<0x4E>(v);     // quad_perm [2,3,0,1]
  v += dpp_lane_f<0x141>(v);    // row_half_mirror: lane i <- lane 7 - i of its half row
  v += dpp_lane_f<0x140>(v);    // row_mirror:      lane i <- lane 15 - i
  return v;
}
__device__ __forceinline__ float dot4_acc(const f32x4_t a, const f32x4_t b, float acc) {
  acc = fmaf(a[0], b[0], acc); acc = fmaf(a[1], b[1], acc);
  acc = fmaf(a[2], b[2], acc); acc = fmaf(a[3], b[3], acc);
  return acc;
}

__global__ __launch_bounds__(kGnn3Threads, 2)
void gnn_attend_v3_kernel(const GnnGroup grp, int C, int D) {
  typedef __attribute__((address_space(3))) void lds_void;
  // The two tiles come first: every LDS-DMA destination then lies below 64 KB.
  __shared__ __attribute__((aligned(16))) float smem[2 * kGnn3Tile + kGnn3Small];
  float* const buf0 = smem;                                 // tiles: buf0, buf0 + kGnn3Tile
  float* const ea = smem + 2 * kGnn3Tile;                   // [64][9] e_ij, then the softmax weights
  float* const ssq = ea + kGnn3Cells * 9;                   // [128]
  int* const hsrc = reinterpret_cast<int*>(ssq + kGnn3Stage);      // [128]
  int* const ssrc = hsrc + kGnn3Stage;                             // [128]
  static_assert(kGnn3Cells * 9 + 3 * kGnn3Stage <= kGnn3Small, "small arrays");
  const bool second = blockIdx.x >= grp.nblocks0;
  const GnnProblem& pr = grp.p[second ? 1 : 0];
  const unsigned blk = second ? blockIdx.x - grp.nblocks0 : blockIdx.x;
  const float* __restrict__ h = pr.h;
  const float* __restrict__ scene_mean = pr.scene_mean;
  const int32_t* __restrict__ src_row = pr.src_row;
  float* __restrict__ out = pr.out;
  _Float16* p16 = pr.p16;
  const size_t p16_stride = pr.p16_stride;
  const int M = pr.M, H = pr.H, W = pr.W, sm_div = pr.sm_div, ngroups = pr.ngroups;
  const int per = (ngroups + 7) >> 3;
  const int g = (blk & 7) * per + (blk >> 3);
  if (g >= ngroups) return;
  const int tid = threadIdx.x;
  const int K = H * W;
  const long long Mtot = (long long)M * K;
  const long long m0 = (long long)g * kGnn3Cells;
  if (pr.row_ref) {     // beam decode: skip the rows no surviving beam descends from
    const long long mlast = m0 + kGnn3Cells - 1 < Mtot ? m0 + kGnn3Cells - 1 : Mtot - 1;
    bool any = false;
    for (long long r = m0 / K; r <= mlast / K; ++r) any |= pr.row_ref[r] != 0;
    if (!any) return;
  }
  // When W divides 64 the group starts at x == 0 and ends at x == W - 1: the corner
  // neighbours m0 - W - 1 and m0 + 64 + W are out of the image and need no staging.
  // Tile slot l holds cell s0 + l, clamped into the tensor (the first and the last group:
  // cells that do not exist are nobody's in-image neighbour); the owned cells are slots
  // own0 .. own0 + 63.
  const int own0 = kGnn3Cells % W == 0 ? W : W + 1;
  const long long s0 = m0 - own0;
  if (tid < kGnn3Stage) {
    long long m = s0 + tid;
    m = m < 0 ? 0 : (m > Mtot - 1 ? Mtot - 1 : m);
    const int r = (int)(m / K), c = (int)(m - (long long)r * K);
    hsrc[tid] = (src_row ? src_row[r] : r) * K + c;
    ssrc[tid] = (r / sm_div) * K + c;
  }
  __syncthreads();

  // DMA role: slot (tid & 15) of staged cells (tid >> 4) + 16 k.  A wave's 64 lanes fill 64
  // consecutive 16-byte slots of the tile.
  // Buffer addressing: one uniform descriptor per tensor + a 32-bit lane offset (rows of h
  // and of the scene means lie below 4 GB: host-checked).
  const int part = tid & 15, ls0 = tid >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const __amdgpu_buffer_rsrc_t h_rs = __builtin_amdgcn_make_buffer_rsrc(
      uniform_ptr(const_cast<float*>(h)), 0, 0xffffffffu, 0x00020000);
  const __amdgpu_buffer_rsrc_t sm_rs = __builtin_amdgcn_make_buffer_rsrc(
      uniform_ptr(const_cast<float*>(scene_mean)), 0, 0xffffffffu, 0x00020000);
  uint32_t goff[kGnn3It];                     // byte offset of the cell's row in h
#pragma unroll
  for (int k = 0; k < kGnn3It; ++k) {
    goff[k] = (uint32_t)hsrc[ls0 + 16 * k] * (uint32_t)(C * 4);
  }
  // (ls >> 1) & 15 of cell ls0 + 16 k is (ls0 >> 1) + 8 (k & 1)
  const uint32_t p_plain = part * 16;
  const uint32_t p_swz0 = (part ^ (ls0 >> 1)) * 16, p_swz1 = (part ^ ((ls0 >> 1) + 8)) * 16;
  auto dma_h = [&](int q, float* tile, bool swizzled) {     // channels q*64 .. q*64+63 of h
#pragma unroll
    for (int k = 0; k < kGnn3It; ++k)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          h_rs, (lds_void*)(tile + (wave * 64 + k * kGnn3Threads) * 4), 16,
          goff[k] + (swizzled ? ((k & 1) ? p_swz1 : p_swz0) : p_plain), q * 256, 0, 0);
  };
  auto dma_scene = [&](float* tile) {         // the 64 scene-mean channels (D is 0 or 64: host-checked)
#pragma unroll
    for (int k = 0; k < kGnn3It; ++k)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          sm_rs, (lds_void*)(tile + (wave * 64 + k * kGnn3Threads) * 4), 16,
          (uint32_t)ssrc[ls0 + 16 * k] * 256u + p_plain, 0, 0, 0);
  };

  // ---- pass 1: thread = (quad of cells 4 cp .. 4 cp + 3, channel slice sl); plain layout
  const int cp = tid >> 4, sl = tid & 15;
  const int lq = own0 + cp * 4;
  float pd[4][9], hq[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    hq[k] = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) pd[k][t] = 0.f;
  }
  const int o0 = (lq - 1) * 64 + sl * 4;      // row dy = 0, window cell j: + j * 64 (floats)
  // The window of row dy = -1 starts at slot own0 - 1 - W + 4 cp >= -1: slot -1 (quad 0 when
  // W divides 64) is the out-of-image corner and is read from slot 0 instead.  Windows end
  // at slot 128 at most: one cell past a tile is the other tile or the small arrays.
  const int om = o0 - W * 64, om0 = om < 0 ? sl * 4 : om;
  // halo cells of this thread: the i-th is staged cell hc, hc = cp + 16 i below the owned
  // range, + 64 above it
  int ho[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int hc = cp + 16 * i;
    ho[i] = (hc < own0 ? hc : hc + kGnn3Cells) * 64 + sl * 4;
  }
  auto dots1 = [&](const float* tile) {
    f32x4_t own[4], r[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) r[j] = *reinterpret_cast<const f32x4_t*>(tile + o0 + j * 64);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      own[k] = r[k + 1];
      pd[k][3] = dot4_acc(own[k], r[k], pd[k][3]);
      pd[k][4] = dot4_acc(own[k], own[k], pd[k][4]);
      pd[k][5] = dot4_acc(own[k], r[k + 2], pd[k][5]);
    }
#pragma unroll
    for (int j = 0; j < 6; ++j)
      r[j] = *reinterpret_cast<const f32x4_t*>(tile + (j == 0 ? om0 : om + j * 64));
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      pd[k][0] = dot4_acc(own[k], r[k], pd[k][0]);
      pd[k][1] = dot4_acc(own[k], r[k + 1], pd[k][1]);
      pd[k][2] = dot4_acc(own[k], r[k + 2], pd[k][2]);
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) r[j] = *reinterpret_cast<const f32x4_t*>(tile + o0 + W * 64 + j * 64);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      pd[k][6] = dot4_acc(own[k], r[k], pd[k][6]);
      pd[k][7] = dot4_acc(own[k], r[k + 1], pd[k][7]);
      pd[k][8] = dot4_acc(own[k], r[k + 2], pd[k][8]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const f32x4_t v = *reinterpret_cast<const f32x4_t*>(tile + ho[i]);
      hq[i] = dot4_acc(v, v, hq[i]);
    }
  };
  // Chunk c of the kernel's nchunk + 4 lands in tile c & 1.  The barrier at the top of a
  // step carries the vmcnt(0) of this wave's pending DMA pieces and closes the reads of
  // the tile the next DMA overwrites.
  const int nchunk = D > 0 ? 5 : 4;
  dma_h(0, buf0, false);
#pragma unroll 1
  for (int c = 0; c < nchunk; ++c) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's pieces of chunk c
    __syncthreads();
    float* const next = buf0 + ((c + 1) & 1) * kGnn3Tile;
    if (c + 1 < 4) dma_h(c + 1, next, false);
    else if (c + 1 < nchunk) dma_scene(next);
    else dma_h(0, next, true);                // pass 2's first chunk
    dots1(buf0 + (c & 1) * kGnn3Tile);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const float v = row16_sum(pd[k][t]);
      if (sl == 0) {
        ea[(cp * 4 + k) * 9 + t] = v;
        if (t == 4) ssq[lq + k] = v;
      }
    }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float v = row16_sum(hq[i]);
    const int hc = cp + 16 * i;
    const int l = hc < own0 ? hc : hc + kGnn3Cells;
    if (sl == 0) ssq[l] = v;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // pass 2's first chunk
  __syncthreads();

  auto cell_mask = [&](long long m) {
    int mask = 0;
    if (m < Mtot) {
      const int c = (int)(m % K);
      const int y = c / W, x = c - y * W;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) mask |= 1 << t;
      }
    }
    return mask;
  };
  if (tid < kGnn3Cells) {              // softmax over the in-image neighbours of cell tid
    const int mask = cell_mask(m0 + tid);
    const int li = own0 + tid;
    float e[9];
    float emax = -INFINITY;
    const float invi = mask ? rsqrtf(fmaxf(ssq[li], 1e-12f)) : 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      e[t] = 0.f;
      if ((mask >> t) & 1) {
        const int lj = li + (t / 3 - 1) * W + (t % 3 - 1);
        e[t] = ea[tid * 9 + t] * invi * rsqrtf(fmaxf(ssq[lj], 1e-12f));
        emax = fmaxf(emax, e[t]);
      }
    }
    float den = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      e[t] = ((mask >> t) & 1) ? expf(e[t] - emax) : 0.f;
      den += e[t];
    }
    const float inv = mask ? 1.0f / den : 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) ea[tid * 9 + t] = e[t] * inv;
  }
  __syncthreads();                     // weights visible; pass 2's first chunk has landed

  // ---- pass 2: thread = (pair of cells 2 pi, 2 pi + 1, channels c8*8 .. +7 of the chunk);
  // swizzled layout, reads clamped into the tile
  const int pi = tid & 31, c8 = tid >> 5;
  const int lp = own0 + pi * 2;
  const long long m2 = m0 + pi * 2;
  // h_i + sum_t a_t h_t = sum_t (a_t + [t == 4]) h_t: the residual rides on the self weight
  float al[2][9];
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int t = 0; t < 9; ++t) al[k][t] = ea[(pi * 2 + k) * 9 + t] + (t == 4 ? 1.0f : 0.f);
  // The stores of chunk q are issued at the top of step q + 1, in front of that step's DMA:
  // the vmcnt(0) in front of a barrier then only waits for requests that are a whole compute
  // phase old (vmcnt counts loads and stores alike).
  auto store_pair = [&](const float (&o2)[2][8], int ch) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (m2 + k < Mtot) {
        const float* o = o2[k];
        if (out) {
          f32x4_t* dst = reinterpret_cast<f32x4_t*>(out + (size_t)(m2 + k) * C + ch);
          dst[0] = f32x4_t{o[0], o[1], o[2], o[3]};
          dst[1] = f32x4_t{o[4], o[5], o[6], o[7]};
        }
        if (p16) {
          typedef _Float16 h8 __attribute__((ext_vector_type(8)));
          h8 pa, pb;
          const size_t idx = plane_index(m2 + k, ch, C);
          if (p16_stride == 0) {
#pragma unroll
            for (int j = 0; j < 8; ++j) pa[j] = bf16_half_bits(o[j]);
            *reinterpret_cast<h8*>(p16 + idx) = pa;
          } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const float sc = o[j] * 256.0f;
              const _Float16 h0h = (_Float16)sc;
              pa[j] = h0h;
              pb[j] = (_Float16)(sc - (float)h0h);
            }
            *reinterpret_cast<h8*>(p16 + idx) = pa;
            *reinterpret_cast<h8*>(p16 + p16_stride + idx) = pb;
          }
        }
      }
    }
  };
  float node[2][8];
#pragma unroll 1
  for (int q = 0; q < 4; ++q) {
    const int c = nchunk + q;
    if (q > 0) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // this wave's pieces of chunk c
      __syncthreads();
      store_pair(node, (q - 1) * 64 + c8 * 8);
    }
    if (q < 3) dma_h(q + 1, buf0 + ((c + 1) & 1) * kGnn3Tile, true);
    const float* const tile = buf0 + (c & 1) * kGnn3Tile;
    auto staged = [&](int l, int p) -> f32x4_t {
      l = l < 0 ? 0 : (l > kGnn3Stage - 1 ? kGnn3Stage - 1 : l);
      return *reinterpret_cast<const f32x4_t*>(&tile[l * 64 + ((p ^ ((l >> 1) & 15)) << 2)]);
    };
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int j = 0; j < 8; ++j) node[k][j] = 0.f;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy) {
        f32x4_t r[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = staged(lp - 1 + j + dy * W, c8 * 2 + half);
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
          for (int dx = -1; dx <= 1; ++dx) {
            const float a = al[k][(dy + 1) * 3 + dx + 1];
#pragma unroll
            for (int j = 0; j < 4; ++j)
              node[k][half * 4 + j] = fmaf(a, r[k + 1 + dx][j], node[k][half * 4 + j]);
          }
      }
    }
  }
  store_pair(node, 3 * 64 + c8 * 8);
}
static inline unsigned gnn_v3_blocks(size_t cells, int* ngroups) {
  const size_t g = (cells + kGnn3Cells - 1) / kGnn3Cells;
  *ngroups = (int)g;
  return (unsigned)(((g + 7) / 8) * 8);
}

// ---------------------------------------------------------------- hidden2grid
// conv3x3 SAME, no bias, identity, C -> P (P in {1,2}); hidden2grid,
// code/pred_models.py:925-959.  One wave per cell, lane l holds channels
// 4l..4l+3.  out has row stride out_row_stride elements so step t of a
// [N, T, H, W, P] output tensor is written in place.
template <int P>
__global__ __launch_bounds__(256)
void hidden2grid_kernel(const float* __restrict__ h, const float* __restrict__ w,
                        float* __restrict__ out, size_t out_row_stride, int M,
                        int H, int W, int C) {
  const int lane = threadIdx.x & 63;
  const size_t cell_id = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int K = H * W;
  if (cell_id >= (size_t)M * K) return;
  const int m = cell_id / K;
  const int cell = cell_id - (size_t)m * K;
  const int y = cell / W, x = cell - y * W;
  const float* hrow = h + (size_t)m * K * C;
  float acc[P];
#pragma unroll
  for (int p = 0; p < P; ++p) acc[p] = 0.f;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
    if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
      for (int c0 = lane * 4; c0 < C; c0 += 256) {     // channel groups of 256 (any C % 4 == 0)
        const f32x4_t hv = *reinterpret_cast<const f32x4_t*>(
            hrow + (size_t)(yy * W + xx) * C + c0);
        const float* wp = w + ((size_t)t * C + c0) * P;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int p = 0; p < P; ++p) acc[p] = fmaf(hv[j], wp[j * P + p], acc[p]);
      }
    }
  }
#pragma unroll
  for (int p = 0; p < P; ++p) acc[p] = wave_sum(acc[p]);
  if (lane == 0) {
#pragma unroll
    for (int p = 0; p < P; ++p)
      out[(size_t)m * out_row_stride + (size_t)cell * P + p] = acc[p];
  }
}

// argmax over K logits per row, lowest index wins ties (tf.argmax,
// code/pred_models.py:411-415).  One wave per row.
__global__ __launch_bounds__(64)
void argmax_rows_kernel(const float* __restrict__ logits, size_t row_stride,
                        int32_t* __restrict__ ids, int M, int K) {
  const int m = blockIdx.x;
  const int lane = threadIdx.x;
  const float* p = logits + (size_t)m * row_stride;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int k = lane; k < K; k += 64) {
    const float v = p[k];
    if (v > best || (v == best && k < bi)) { best = v; bi = k; }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(best, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
  }
  if (lane == 0) ids[m] = bi;
}

// ---------------------------------------------------------------- beam step
// One workgroup per sample.  (code/pred_models.py:557-591, add_div_penalty
// :1197-1223.)  logits [N,B,K]:
//   lp = log_softmax(logits) + prev_lp[b]
//   if diverse: lp += log(gamma) * rank_desc(lp within (n,b)), ties -> lower idx
//   candidates = time > 1 ? lp[N, B*K] : lp[:, 0]
//   (new_lp, idx) = top_k(candidates, B) descending, ties -> lower index
//   new_lp = 0 unless time > fix_num_timestep; ids = idx % K; parents = idx / K
// The rank of element v is the number of elements that precede it in the
// stable descending order: #{u : lp[u] > lp[v]} + #{u < v : lp[u] == lp[v]}.
// Dynamic LDS: lp [B*K] + 512 words of reduction scratch + pen [B*K].
__global__ __launch_bounds__(512)
void beam_step_kernel(const float* __restrict__ logits,
                      const float* __restrict__ prev_lp, int B, int K, int time,
                      int diverse, float log_gamma, int fix_num_timestep,
                      float* __restrict__ new_lp, int32_t* __restrict__ ids,
                      int32_t* __restrict__ parents,
                      int32_t* __restrict__ state_src_row, int state_rows_per_sample,
                      int32_t* __restrict__ row_ref = nullptr) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* lp = sm;                 // [B*K]
  float* red = sm + B * K;        // [256] reduction scratch
  int* redi = reinterpret_cast<int*>(red + 256);  // [256]
  const int n = blockIdx.x;
  const int tid = threadIdx.x;
  const int nthr = blockDim.x;
  const int lane = tid & 63, wave = tid >> 6, nwave = nthr >> 6;
  const float* lg = logits + (size_t)n * B * K;

  // log_softmax per beam: one wave per beam row (strided over beams)
  for (int b = wave; b < B; b += nwave) {
    const float* row = lg + (size_t)b * K;
    float mx = -INFINITY;
    for (int k = lane; k < K; k += 64) mx = fmaxf(mx, row[k]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    float s = 0.f;
    for (int k = lane; k < K; k += 64) s += expf(row[k] - mx);
    s = wave_sum(s);
    const float lse = logf(s);
    const float pl = prev_lp[(size_t)n * B + b];
    for (int k = lane; k < K; k += 64) lp[b * K + k] = pl + ((row[k] - mx) - lse);
  }
  __syncthreads();
  if (diverse) {
    // rank by counting over the un-penalised values; penalties go to a second
    // LDS plane and are applied once every rank has been taken.
    float* pen = sm + B * K + 512;
    const int total = B * K;
    for (int v = tid; v < total; v += nthr) {
      const int b = v / K, kv = v - b * K;
      const float val = lp[v];
      const float* row = lp + b * K;
      int rank = 0;
      for (int u = 0; u < K; ++u) {
        const float o = row[u];
        rank += (o > val) || (o == val && u < kv);
      }
      pen[v] = log_gamma * (float)rank;
    }
    __syncthreads();
    for (int v = tid; v < total; v += nthr) lp[v] = lp[v] + pen[v];
    __syncthreads();
  }
  // top-B selection by repeated arg-max with (value desc, index asc) order.
  const int ncand = (time > 1) ? B * K : K;
  for (int sel = 0; sel < B; ++sel) {
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int v = tid; v < ncand; v += nthr) {
      const float val = lp[v];
      if (val > best || (val == best && v < bi)) { best = val; bi = v; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(best, off, 64);
      const int oi = __shfl_xor(bi, off, 64);
      if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    if (lane == 0) { red[wave] = best; redi[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
      for (int wv = 1; wv < nwave; ++wv) {
        const float ov = red[wv];
        const int oi = redi[wv];
        if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
      }
      const int par = bi / K;
      new_lp[(size_t)n * B + sel] = (time > fix_num_timestep) ? best : 0.f;
      ids[(size_t)n * B + sel] = bi - par * K;
      parents[(size_t)n * B + sel] = par;
      if (state_src_row) state_src_row[(size_t)n * B + sel] = n * state_rows_per_sample + par;
      if (row_ref) row_ref[n * state_rows_per_sample + par] = 1;   // a state row some beam continues
      lp[bi] = -INFINITY;  // remove from the candidate set
    }
    __syncthreads();
  }
}

// The same step in two launches, so that the O(K^2) rank count of the diversity penalty
// spreads over the whole chip instead of one CU per sample (447 us -> ~60 us per step at
// N=128, B=20, K=576):
//   beam_rank_kernel    one WAVE per (n, b) row, the row held in registers (lane l owns
//                       k = l + 64 j); element u is broadcast with v_readlane and compared
//                       against the 64 * J owned values; writes the candidates lp [R, K].
//                       Same arithmetic, in the same order, as beam_step_kernel.
//   beam_select_kernel  one workgroup per sample: candidates in LDS, every thread caches
//                       the best of the ones it owns, B rounds of (wave reduce -> 16-entry
//                       LDS table -> every thread re-derives the winner); only the winner's
//                       owner rescans.  One barrier per round.
constexpr int kBeamRankJ = 16;   // K <= 1024

// Caller-given allowed cells (include/multiverse_hip.h mv_set_cell_mask): the kernels that hold a
// row in one wave's registers come in a Masked form (row_form.h), instantiated beside the plain
// one, whose in-row predicate `lane + 64 j < K` is "in row AND allowed".  The row's mask plane [K]
// (one byte per cell, non-zero = allowed) is read once per wave into one bit per owned cell (bit
// j: k = lane + 64 j); a cell past the row is not allowed.  No LDS, no scratch, no indexed arrays.
template <int J>
__device__ __forceinline__ uint32_t step_row_allowed_bits(const uint8_t* __restrict__ plane,
                                                          int K, int lane) {
  static_assert(J <= 32, "one bit per owned cell");
  uint32_t am = 0u;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int k = lane + 64 * j;
    if (k < K && plane[k] != 0) am |= 1u << j;
  }
  return am;
}

// the in-row predicate of owned cell j; the unmasked form does not read `am`
template <bool MASKED>
__device__ __forceinline__ bool step_cell_in(uint32_t am, int lane, int j, int K) {
  if constexpr (MASKED) return ((am >> j) & 1u) != 0u;   // (a set bit is in the row)
  else return lane + 64 * j < K;
}

// Caller-given cell costs (include/multiverse_hip.h mv_set_cell_bias): a third, Biased form of
// the same kernels.  It serves "bias only" and "bias + mask"
// alike: it always works on the `am` bits, which are the in-row bits when no mask plane is given.
// The row's bias plane [K] floats is read once per wave into b[J] exactly as the logits are
// (lane l owns k = l + 64 j; 0 past the row).
template <int J>
__device__ __forceinline__ uint32_t step_row_biased_bits(const uint8_t* __restrict__ plane,
                                                         int K, int lane) {
  if (plane) return step_row_allowed_bits<J>(plane, K, lane);   // uniform
  uint32_t am = 0u;
#pragma unroll
  for (int j = 0; j < J; ++j)
    if (lane + 64 * j < K) am |= 1u << j;
  return am;
}

template <int J>
__device__ __forceinline__ void step_row_bias(const float* __restrict__ plane, int K, int lane,
                                              float (&b)[J]) {
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int k = lane + 64 * j;
    b[j] = k < K ? plane[k] : 0.f;
  }
}

// Caller-given motion costs (include/multiverse_hip.h mv_set_motion_cost): a fourth, Motion form
// of the same kernels.  It is the Biased form whose b[J]
// is b_eff = (b + vterm) + aterm, with the two terms derived per wave from the row's own path:
// one instantiation serves motion alone (no bias plane: b = 0.0f) and every combination with a
// mask and a bias.  Where the row's path lies, per launch:
//   p1 = prev1[(p1_per_row ? r : n) * p1_stride]
//   p0 = prev0[(p0_per_row ? (prev0_via ? n * B + prev0_via[r] : r) : n) * p0_stride]
//        (prev0 == NULL or a value < 0: absent; obs_lens: absent where obs_lens[n] < 2)
// so that the engine points at the labels and at the ids / parents its steps already write, and
// no launch and no [R, K] plane is added.  The tables [samples, D, D] hold at most 81 floats per
// sample and are read through the cache, only by the lanes whose cell lies inside the window.
struct MotionRow {
  const float* vel = nullptr;         // [samples, D, D]; NULL: no motion cost
  const float* vel_far = nullptr;     // [samples]
  const float* acc = nullptr;         // [samples, D, D] or NULL: no turn term
  const float* acc_far = nullptr;     // [samples]
  const int32_t* prev1 = nullptr;
  const int32_t* prev0 = nullptr;
  const int32_t* prev0_via = nullptr; // the slot, within the sample, that holds the row's p0
  const int32_t* obs_lens = nullptr;
  int32_t p1_stride = 1, p0_stride = 1;
  int32_t p1_per_row = 1, p0_per_row = 1;
  int32_t W = 1, radius = 1;
};

// b[j] = (plane[k] + vterm(k)) + aterm(k) for the owned cells k = lane + 64 j of row r (sample n,
// B rows per sample); plane == NULL: b = 0.0f.  0.0f past the row.  (y, x) of the owned cells
// advance by 64 cells per j in (rows, columns) with one carry: no division per cell, and none
// of a difference of cell indices (W is no power of two on the 9-, 10- and 18-column grids).
template <int J>
__device__ __forceinline__ void step_row_motion(const MotionRow& mo,
                                                const float* __restrict__ plane, int n, int r,
                                                int B, int K, int lane, float (&b)[J]) {
  const int W = mo.W, rad = mo.radius, D = 2 * rad + 1;
  int p1 = mo.prev1[(size_t)(mo.p1_per_row ? r : n) * mo.p1_stride];
  int p0 = -1;
  if (mo.prev0) {
    const int row0 = mo.p0_per_row ? (mo.prev0_via ? n * B + mo.prev0_via[r] : r) : n;
    p0 = mo.prev0[(size_t)row0 * mo.p0_stride];
  }
  if (mo.obs_lens && mo.obs_lens[n] < 2) p0 = -1;
  p1 = __builtin_amdgcn_readfirstlane(p1);        // the wave's row: uniform
  p0 = __builtin_amdgcn_readfirstlane(p0);
  const int y1 = p1 / W, x1 = p1 - y1 * W;
  const bool turn = mo.acc != nullptr && p0 >= 0;
  int uy = 0, ux = 0;
  if (turn) {
    const int y0 = p0 / W, x0 = p0 - y0 * W;
    uy = y1 - y0;
    ux = x1 - x0;
  }
  const float* vel = mo.vel + (size_t)n * D * D;
  const float* acc = turn ? mo.acc + (size_t)n * D * D : nullptr;
  const float vfar = mo.vel_far[n];
  const float afar = turn ? mo.acc_far[n] : 0.f;
  const int qy = 64 / W, qx = 64 - qy * W;        // 64 cells on = qy rows and qx columns on
  int y = lane / W, x = lane - y * W;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int k = lane + 64 * j;
    float bj = 0.f;
    if (k < K) {
      if (plane) bj = plane[k];
      const int dy = y - y1 + rad, dx = x - x1 + rad;          // inside the window: in [0, D)
      const bool vin = (unsigned)dy < (unsigned)D && (unsigned)dx < (unsigned)D;
      bj = bj + (vin ? vel[dy * D + dx] : vfar);
      float at = 0.f;
      if (turn) {
        const int ay = dy - uy, ax = dx - ux;
        const bool ain = (unsigned)ay < (unsigned)D && (unsigned)ax < (unsigned)D;
        at = ain ? acc[ay * D + ax] : afar;
      }
      bj = bj + at;
    }
    b[j] = bj;
    x += qx;
    y += qy;
    if (x >= W) { x -= W; y += 1; }
  }
}

// Caller-given revisit cost (include/multiverse_hip.h mv_set_revisit_cost): a fifth, Path form of
// the same kernels.  It is the Motion form with
// rterm added to b[J]; the motion part runs only when mo.vel is set (a wave-uniform branch), so
// ONE instantiation serves the revisit cost alone and every combination with a mask, a bias and
// a motion cost.  The visited set of a row is 64 words, lane-major as the `am` bits are: bit j of
// word l = cell l + 64 j, so a lane loads one word, ORs one bit and stores one word -- 256 B a row
// for any K <= 1024, no LDS, no indexed arrays.  The step kernel maintains the sets itself:
//   set = set_in[(via ? n * B + via[r] : r)]   (set_in == NULL: empty)
//       | the row's observed cells seed[n, seed_T - Lo[n] .. seed_T - 1]   (seed == NULL: none)
//       | (or_p1 ? {p1} : {})
//   set_out[r] = set;   rterm(k) = cost[n] where k is in set and k != p1, else 0.0f
// with p1 = prev1[(p1_per_row ? r : n) * p1_stride].  set_in and set_out differ (slots read other
// slots' rows of the step before), so the engine keeps two and alternates.  No bit index is
// formed from a value outside [0, K).
struct RevisitRow {
  const float* cost = nullptr;        // [samples]; NULL: no revisit cost
  const uint32_t* set_in = nullptr;   // [rows, 64] the sets of the step before, or NULL: empty
  uint32_t* set_out = nullptr;        // [rows, 64]
  const int32_t* via = nullptr;       // the slot, within the sample, whose set the row continues
  const int32_t* prev1 = nullptr;
  const int32_t* seed = nullptr;      // labels [samples, seed_T], or NULL
  const int32_t* obs_lens = nullptr;  // Lo [samples], or NULL: seed_T
  int32_t p1_stride = 1, p1_per_row = 1;
  int32_t seed_T = 0, or_p1 = 1;
};

// b[j] = b_m[k] + rterm(k) for the owned cells k = lane + 64 j of row r (sample n, B rows per
// sample): b_m is step_row_motion's b_eff when a motion cost is set, else the bias plane or 0.0f.
template <int J>
__device__ __forceinline__ void step_row_path(const MotionRow& mo, const RevisitRow& rv,
                                              const float* __restrict__ plane, int n, int r,
                                              int B, int K, int lane, float (&b)[J]) {
  static_assert(J <= 32, "one bit per owned cell");
  if (mo.vel != nullptr) {                       // uniform
    step_row_motion<J>(mo, plane, n, r, B, K, lane, b);
  } else {
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int k = lane + 64 * j;
      b[j] = (plane != nullptr && k < K) ? plane[k] : 0.f;
    }
  }
  int p1 = rv.prev1[(size_t)(rv.p1_per_row ? r : n) * rv.p1_stride];
  p1 = __builtin_amdgcn_readfirstlane(p1);       // the wave's row: uniform
  uint32_t set = 0u;
  if (rv.set_in) {
    int row = r;
    if (rv.via) row = n * B + min(max(rv.via[r], 0), B - 1);
    set = rv.set_in[(size_t)row * 64 + lane];
  }
  if (rv.seed) {
    const int T = rv.seed_T;
    int lo = rv.obs_lens ? min(max(rv.obs_lens[n], 0), T) : T;
    lo = __builtin_amdgcn_readfirstlane(lo);
    for (int i = T - lo; i < T; ++i) {           // uniform: at most obs_len cells
      const int c = __builtin_amdgcn_readfirstlane(rv.seed[(size_t)n * T + i]);
      if (c >= 0 && c < K && (c & 63) == lane) set |= 1u << (c >> 6);
    }
  }
  const uint32_t p1bit = (p1 >= 0 && p1 < K && (p1 & 63) == lane) ? 1u << (p1 >> 6) : 0u;
  if (rv.or_p1) set |= p1bit;
  rv.set_out[(size_t)r * 64 + lane] = set;
  const uint32_t pay = set & ~p1bit;             // staying in the current cell is no revisit
  const float c = rv.cost[n];
#pragma unroll
  for (int j = 0; j < J; ++j) b[j] = b[j] + (((pay >> j) & 1u) ? c : 0.f);
}

// Everything a constrained step reads beyond its logits, as ONE kernel argument (the launchers'
// StepTerms, engine_setup.h): sample n's mask plane [K] is amask + n * mask_stride, its bias plane
// [K] floats bias + n * bias_stride; a NULL amask / bias / mo.vel / rv.cost: that part is not set.
struct RowTerms {
  const uint8_t* amask = nullptr;
  int64_t mask_stride = 0;
  const float* bias = nullptr;
  int64_t bias_stride = 0;
  MotionRow mo;
  RevisitRow rv;
  RowForm form() const {
    return row_form(amask != nullptr, bias != nullptr, mo.vel != nullptr, rv.cost != nullptr);
  }
  bool constrained() const { return form() != RowForm::Plain; }
};

// The per-row block of the three step kernels: the allowed bits `am` and the additive terms b[J]
// of row r (sample n, B rows per sample), as form F has them.  Plain reads nothing of `tm` and
// leaves both alone; Masked forms `am` only (b is a one-element dummy below Biased).
template <int J, RowForm F>
__device__ __forceinline__ void step_row_terms(const RowTerms& tm, int n, int r, int B, int K,
                                               int lane, uint32_t& am,
                                               float (&b)[row_has_bias(F) ? J : 1]) {
  if constexpr (row_has_bias(F)) {
    if constexpr (row_has_motion(F)) {
      const float* plane = tm.bias ? tm.bias + (size_t)n * tm.bias_stride : nullptr;
      if constexpr (row_has_path(F)) step_row_path<J>(tm.mo, tm.rv, plane, n, r, B, K, lane, b);
      else step_row_motion<J>(tm.mo, plane, n, r, B, K, lane, b);
    } else {
      step_row_bias<J>(tm.bias + (size_t)n * tm.bias_stride, K, lane, b);
    }
    am = step_row_biased_bits<J>(tm.amask ? tm.amask + (size_t)n * tm.mask_stride : nullptr, K,
                                 lane);
  } else if constexpr (row_has_bits(F)) {
    am = step_row_allowed_bits<J>(tm.amask + (size_t)n * tm.mask_stride, K, lane);
  }
}

// Masked: terms.amask + (r / B) * mask_stride is the plane of the row's sample at this step.  A
// cell outside it becomes the candidate -inf after lp + prev_lp and BEFORE the ranks: it precedes
// nothing, so an allowed cell's rank counts allowed cells only.
// Biased (amask may be NULL): the candidate is (prev_lp + lp) + b, with
// b = bias + (r / B) * bias_stride, formed before the mask's -inf and before the ranks.
// Motion (bias may be NULL): b is step_row_motion's b_eff of the row.
// Path (mo.vel may be NULL): b is step_row_path's, and the row's set is stored.
template <int J, RowForm F>
__global__ __launch_bounds__(256)
void beam_rank_kernel(const float* __restrict__ logits, const float* __restrict__ prev_lp,
                      int R, int B, int K, int time, int diverse, float log_gamma,
                      float* __restrict__ cand, RowTerms terms) {
  constexpr bool MASKED = row_has_bits(F), BIASED = row_has_bias(F);
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  if (time <= 1 && (r % B) != 0) return;   // only beam 0 is a candidate at the first step
  const float* row = logits + (size_t)r * K;
  float v[J];
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int k = lane + 64 * j;
    v[j] = k < K ? row[k] : -INFINITY;
    mx = fmaxf(mx, v[j]);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < J; ++j)
    if (lane + 64 * j < K) s += expf(v[j] - mx);
  s = wave_sum(s);
  const float lse = logf(s);
  const float pl = prev_lp[r];
#pragma unroll
  for (int j = 0; j < J; ++j) v[j] = pl + ((v[j] - mx) - lse);
  if constexpr (MASKED) {
    uint32_t am = 0u;
    float b[BIASED ? J : 1];
    step_row_terms<J, F>(terms, r / B, r, B, K, lane, am, b);
    if constexpr (BIASED) {
#pragma unroll
      for (int j = 0; j < J; ++j) v[j] = v[j] + b[j];
    }
#pragma unroll
    for (int j = 0; j < J; ++j)
      if (!step_cell_in<true>(am, lane, j, K)) v[j] = -INFINITY;
  }
  if (diverse) {
    int rank[J];
#pragma unroll
    for (int j = 0; j < J; ++j) rank[j] = 0;
#pragma unroll
    for (int jj = 0; jj < J; ++jj) {
      const int lim = min(64, K - 64 * jj);      // uniform
      for (int l = 0; l < lim; ++l) {
        const float o = __builtin_bit_cast(float, __builtin_amdgcn_readlane(
                                                      __builtin_bit_cast(int, v[jj]), l));
#pragma unroll
        for (int j = 0; j < J; ++j) {
          // u = l + 64 jj precedes kv = lane + 64 j  <=>  jj < j, or jj == j and l < lane
          const bool before = jj < j || (jj == j && l < lane);
          rank[j] += (o > v[j] || (before && o == v[j])) ? 1 : 0;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < J; ++j) v[j] = v[j] + log_gamma * (float)rank[j];
  }
  float* out = cand + (size_t)r * K;
#pragma unroll
  for (int j = 0; j < J; ++j)
    if (lane + 64 * j < K) out[lane + 64 * j] = v[j];
}

__device__ __forceinline__ bool beam_better(float v, int i, float bv, int bi) {
  return v > bv || (v == bv && i < bi);
}

// Dynamic LDS: lp [B*K] + 2 x 16 (value, index) reduction entries.
__global__ __launch_bounds__(1024)
void beam_select_kernel(const float* __restrict__ cand, int B, int K, int time,
                        int fix_num_timestep, float* __restrict__ new_lp,
                        int32_t* __restrict__ ids, int32_t* __restrict__ parents,
                        int32_t* __restrict__ state_src_row, int state_rows_per_sample,
                        int32_t* __restrict__ row_ref = nullptr) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ncand = (time > 1) ? B * K : K;
  float* lp = sm;
  float* redv = sm + B * K;                              // [2][16]
  int* redi = reinterpret_cast<int*>(redv + 32);         // [2][16]
  const float* src = cand + (size_t)n * B * K;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int v = tid; v < ncand; v += 1024) {
    const float x = src[v];
    lp[v] = x;
    if (beam_better(x, v, best, bi)) { best = x; bi = v; }
  }
  for (int sel = 0; sel < B; ++sel) {
    float wv = best;
    int wi = bi;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(wv, off, 64);
      const int oi = __shfl_xor(wi, off, 64);
      if (beam_better(ov, oi, wv, wi)) { wv = ov; wi = oi; }
    }
    const int pp = (sel & 1) * 16;
    if (lane == 0) { redv[pp + wave] = wv; redi[pp + wave] = wi; }
    __syncthreads();
    wv = redv[pp];
    wi = redi[pp];
#pragma unroll
    for (int w = 1; w < 16; ++w) {
      const float ov = redv[pp + w];
      const int oi = redi[pp + w];
      if (beam_better(ov, oi, wv, wi)) { wv = ov; wi = oi; }
    }
    if (tid == 0) {
      const int par = wi / K;
      new_lp[(size_t)n * B + sel] = (time > fix_num_timestep) ? wv : 0.f;
      ids[(size_t)n * B + sel] = wi - par * K;
      parents[(size_t)n * B + sel] = par;
      if (state_src_row) state_src_row[(size_t)n * B + sel] = n * state_rows_per_sample + par;
      if (row_ref) row_ref[n * state_rows_per_sample + par] = 1;   // a state row some beam continues
    }
    if ((wi & 1023) == tid) {          // the owner removes the winner and rescans its own
      lp[wi] = -INFINITY;
      best = -INFINITY;
      bi = 0x7fffffff;
      for (int v = tid; v < ncand; v += 1024) {
        const float x = lp[v];
        if (beam_better(x, v, best, bi)) { best = x; bi = v; }
      }
    }
  }
}

// ------------------------------------------------------------ sampled step
// Counter-based generator shared by the input dropout of training (train_kernels.h
// dropout_keep) and the sampled decode: 32 mixed bits of (element, seed, stream).
__device__ __forceinline__ uint32_t hash32(uint32_t i, uint32_t seed, uint32_t stream) {
  uint32_t x = i * 0x9E3779B1u + seed * 0x85EBCA77u + stream * 0xC2B2AE3Du;
  x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
  return x;
}

// Batch row n of a sampled forward draws with seed + n * kSampleRowSeed (mod 2^32): row n is row
// 0 of a forward seeded that way, whatever the batch around it.
constexpr uint32_t kSampleRowSeed = 0x632BE5ABu;

// u in (0, 1): (top 24 bits + 0.5) * 2^-24 in fp32.  Codes from 2^23 on need 25 significand
// bits and round to even; the last one would round to 1.0 and is held at the largest fp32 below.
__device__ __forceinline__ float sample_uniform(uint32_t i, uint32_t seed, uint32_t stream) {
  const float u = ((float)(hash32(i, seed, stream) >> 8) + 0.5f) * 0x1p-24f;
  return fminf(u, 0x1.fffffep-1f);
}

// What the step kernels of the sampled and the scoring forward share, so that scoring the ids a
// sampled forward drew reproduces its log-probabilities bit for bit: one WAVE per row, the row
// held in registers as in beam_rank_kernel (lane l owns k = l + 64 j).
// The row's logits (-inf past K) and the terms of lp[k] = (v[k] - mx) - lse.
template <int J>
__device__ __forceinline__ void step_row_log_softmax(const float* __restrict__ row, int K,
                                                     int lane, float (&v)[J], float& mx,
                                                     float& lse) {
  mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int k = lane + 64 * j;
    v[j] = k < K ? row[k] : -INFINITY;
    mx = fmaxf(mx, v[j]);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < J; ++j)
    if (lane + 64 * j < K) sum += expf(v[j] - mx);
  sum = wave_sum(sum);
  lse = logf(sum);
}

// log_softmax terms of a row already in registers (-inf past K): step_row_log_softmax's
// arithmetic in its order
// MASKED: v is -inf outside the allowed cells too, and the sum runs over the allowed cells
template <int J, bool MASKED = false>
__device__ __forceinline__ void step_regs_log_softmax(const float (&v)[J], int K, int lane,
                                                      float& mx, float& lse, uint32_t am = 0u) {
  mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < J; ++j) mx = fmaxf(mx, v[j]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < J; ++j)
    if (step_cell_in<MASKED>(am, lane, j, K)) sum += expf(v[j] - mx);
  sum = wave_sum(sum);
  lse = logf(sum);
}

// ------------------------------------------------------------ truncated sampling
// Top-k / nucleus limits of the two samplers (include/multiverse_hip.h
// mv_set_sampling_truncation).  With w = l / temperature, e[k] = exp(w[k] - max w),
//   c(k) = #{j : l[j] > l[k]},  m(k) = sum of e[j] over {j : l[j] > l[k]},
//   keep(k) = c(k) < floor || ((top_k == 0 || c(k) < top_k) && (top_p >= 1 || m(k) < top_p * sum_e))
// keep is an upper set of the logit order: one threshold on an order-preserving integer key of
// the logit describes it.  The sums run in step_row_log_softmax's order (per lane over j, then
// wave_sum), so that a fixed-order sum of non-negative terms is monotone in its term set and the
// predicate is monotone in the threshold.

// Order-preserving key of a float (no NaN): a > b <=> key(a) > key(b); -0 and +0 share a key.
__device__ __forceinline__ uint32_t float_order_key(float x) {
  const uint32_t u = __builtin_bit_cast(uint32_t, x + 0.f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// The row in registers (v = logits, -inf past K; w = v / temperature; mxq = max w): bisection over
// the 32 key bits for the smallest key whose cells are kept, 32 probes of one masked per-lane
// count and sum over j and two butterflies.  No LDS, no scratch, no indexed register arrays.
// -> the threshold (keep(k) <=> float_order_key(v[k]) >= threshold); lse_kept = logf of the kept
// cells' sum of e, taken in the same order.
// MASKED (mv_set_cell_mask): a cell outside the allowed set `am` is absent, as a cell past K is:
// e, sum_e, c(k), m(k) and the floor run over the allowed cells, and mxq is their maximum.
// BIASED (mv_set_cell_bias): w carries the bias, and the order of the limits is the order of w,
// not of the logits: the key is taken of w, and keep(k) <=> float_order_key(w[k]) >= threshold.
template <int J, bool MASKED = false, bool BIASED = false>
__device__ __forceinline__ uint32_t step_row_keep_threshold(const float (&v)[J],
                                                            const float (&w)[J], float mxq, int K,
                                                            int lane, int top_k, float top_p,
                                                            int floor, float& lse_kept,
                                                            uint32_t am = 0u) {
  uint32_t key[J];
  float e[J];
  float sum_e = 0.f;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const bool in = step_cell_in<MASKED>(am, lane, j, K);
    // (a pad never counts: masked by e and `in`)
    key[j] = in ? float_order_key(BIASED ? w[j] : v[j]) : 0u;
    e[j] = in ? expf(w[j] - mxq) : 0.f;
    if (in) sum_e += e[j];
  }
  sum_e = wave_sum(sum_e);
  const bool use_p = top_p < 1.f;                 // off means off: never evaluated at top_p >= 1
  const float mass = top_p * sum_e;
  uint32_t thr = 0u;                              // the smallest kept key lies in [thr, thr + 2^(bit+1))
#pragma unroll 1
  for (int bit = 31; bit >= 0; --bit) {
    const uint32_t cand = thr | (1u << bit);
    const uint32_t probe = cand - 1u;             // are the cells of key `probe` kept?
    int cnt = 0;
    float m = 0.f;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const bool above = step_cell_in<MASKED>(am, lane, j, K) && key[j] > probe;
      cnt += above ? 1 : 0;
      if (above) m += e[j];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    m = wave_sum(m);
    const bool kept = cnt < floor || ((top_k == 0 || cnt < top_k) && (!use_p || m < mass));
    if (!kept) thr = cand;                        // uniform: cnt and m are the wave's
  }
  float sum_kept = 0.f;
#pragma unroll
  for (int j = 0; j < J; ++j)
    if (step_cell_in<MASKED>(am, lane, j, K) && key[j] >= thr) sum_kept += e[j];
  lse_kept = logf(wave_sum(sum_kept));
  return thr;
}

// `shared` step: the logits the tail left in the sample's first row, copied to row r's own
template <int J>
__device__ __forceinline__ void step_row_copy_out(float* __restrict__ out, int K, int lane,
                                                  const float (&v)[J]) {
#pragma unroll
  for (int j = 0; j < J; ++j)
    if (lane + 64 * j < K) out[lane + 64 * j] = v[j];
}

// The tail of decode step t of a SAMPLED multi-future forward (mv_set_sampling), one WAVE per
// row r = n * S + s, the row held in registers as in beam_rank_kernel (lane l owns
// k = l + 64 j):
//   lp = log_softmax(logits[r]);  g[k] = -log(-log(u(s * K + k, seed_n, t)))
//   id = argmax over the KEPT k of lp[k] / temperature + g[k]   (lowest index among equal scores)
//   ids[r, t] = id;  lp_acc[r] += lp[id], lq_acc[r] += q~[id] unless the row is past its length
// q~ is the proposal's log-probability: log_softmax(l / temperature) renormalised over the kept
// cells (step_row_keep_threshold; with both limits off every cell is kept, and at temperature 1
// q~ is lp bit for bit).
// logits is the forward's [R, T, K] output at step t (row_stride = T * K), written by the
// decode tail.  `shared` (step 0): the tail ran once per sample and left the logits in row
// n * S; rows s > 0 read them there and copy them to their own row.  src_row (step 0): the
// state row the S rows of sample n continue from.  params: {seed, temperature bits, top_k,
// top_p bits}, read on the device so that a replayed graph follows mv_set_sampling and
// mv_set_sampling_truncation.  keep_out (mv_op_sample_step only): the kept set [R, K].
// Masked (mv_set_cell_mask): terms.amask + n * mask_stride is the sample's plane at this step.  lp
// stays the log-softmax over ALL cells; the proposal treats a cell outside the plane as absent: w
// is -inf there, mxq and the sums run over the allowed cells (also at temperature 1 with no limit:
// the proposal differs from the model), and keep(k) = allowed and the limits' predicate.
// Biased (mv_set_cell_bias; amask may be NULL): b = bias + n * bias_stride,
// w = l / temperature + b, the limits order by w, and the score is (lp / temperature + b) + g.
// Motion (bias may be NULL): b is step_row_motion's b_eff of row r.
// Path (mo.vel may be NULL): b is step_row_path's, and the row's set is stored.
template <int J, RowForm F>
__global__ __launch_bounds__(256)
void sample_step_kernel(float* __restrict__ logits, int64_t row_stride, int R, int S, int K,
                        int t, int shared, const uint32_t* __restrict__ params, int floor,
                        const int32_t* __restrict__ lens, float* __restrict__ lp_acc,
                        float* __restrict__ lq_acc, int32_t* __restrict__ ids, int ids_stride,
                        int32_t* __restrict__ src_row, uint8_t* __restrict__ keep_out,
                        RowTerms terms) {
  constexpr bool MASKED = row_has_bits(F), BIASED = row_has_bias(F);
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const int n = r / S, s = r - n * S;
  const float* row = logits + (size_t)(shared ? n * S : r) * row_stride;
  float v[J], mx, lse;
  step_row_log_softmax<J>(row, K, lane, v, mx, lse);
  const uint32_t seed = params[0] + (uint32_t)n * kSampleRowSeed;
  const float temperature = __builtin_bit_cast(float, params[1]);
  const int top_k = (int)params[2];
  const float top_p = __builtin_bit_cast(float, params[3]);
  const bool tempered = temperature != 1.f;            // uniform, as is `limited`
  const bool limited = top_k > 0 || top_p < 1.f;
  float mxq = mx, lseq = lse;
  uint32_t thr = 0u;
  float w[J];
#pragma unroll
  for (int j = 0; j < J; ++j) w[j] = tempered ? v[j] / temperature : v[j];
  uint32_t am = 0u;
  float b[BIASED ? J : 1];     // live to the score below
  step_row_terms<J, F>(terms, n, r, S, K, lane, am, b);
  if constexpr (BIASED) {
#pragma unroll
    for (int j = 0; j < J; ++j) w[j] = w[j] + b[j];
  }
  if constexpr (MASKED) {
#pragma unroll
    for (int j = 0; j < J; ++j)
      if (!step_cell_in<true>(am, lane, j, K)) w[j] = -INFINITY;
  }
  if (tempered || MASKED) step_regs_log_softmax<J, MASKED>(w, K, lane, mxq, lseq, am);
  if (limited)
    thr = step_row_keep_threshold<J, MASKED, BIASED>(v, w, mxq, K, lane, top_k, top_p, floor, lseq,
                                                     am);
  float best = -INFINITY, blp = 0.f, blq = 0.f;
  int bi = 0x7fffffff;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int k = lane + 64 * j;
    if (k < K) {
      const bool kept = step_cell_in<MASKED>(am, lane, j, K) &&
                        (!limited || float_order_key(BIASED ? w[j] : v[j]) >= thr);
      if (keep_out) keep_out[(size_t)r * K + k] = kept ? 1 : 0;
      if (kept) {
        const float lp = (v[j] - mx) - lse;
        const float u = sample_uniform((uint32_t)s * (uint32_t)K + (uint32_t)k, seed, (uint32_t)t);
        float sc;
        if constexpr (BIASED) sc = (lp / temperature + b[j]) + (-logf(-logf(u)));
        else sc = lp / temperature + (-logf(-logf(u)));
        // strict: the lane's lowest index stays
        if (sc > best) { best = sc; bi = k; blp = lp; blq = (w[j] - mxq) - lseq; }
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(best, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    const float ol = __shfl_xor(blp, off, 64);
    const float oq = __shfl_xor(blq, off, 64);
    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; blp = ol; blq = oq; }
  }
  if (shared && s != 0) step_row_copy_out<J>(logits + (size_t)r * row_stride, K, lane, v);
  if (lane == 0) {
    ids[(size_t)r * ids_stride] = min(bi, K - 1);   // (no score ranked: NaN logits; none is made)
    if (!lens || t < lens[n]) { lp_acc[r] += blp; lq_acc[r] += blq; }
    if (src_row) src_row[r] = n;
  }
}

// The tail of decode step t of a SCORING forward (mv_score_futures): sample_step_kernel with
// the id GIVEN instead of drawn, one wave per row r = n * F + f, the row in registers.
//   lp = log_softmax(logits[r]) through step_row_log_softmax, as sample_step_kernel
//   id = ids[r, t];  live = t < lens[r] (lens: one length per FUTURE; NULL = every step live)
//   live:  step_lp[r, t] = lp[id];  lp_acc[r] += lp[id]
//          rank[r, t] = #{k : logit[k] > logit[id], or logit[k] == logit[id] and k < id}
//   else:  step_lp[r, t] = 0;  rank[r, t] = -1
// `shared` and src_row as in sample_step_kernel.  ids is only read: the upload holds a valid
// cell at every step (the clamp below keeps a foreign buffer from indexing outside the row).
template <int J>
__global__ __launch_bounds__(256)
void score_step_kernel(float* __restrict__ logits, int64_t row_stride, int R, int S, int K,
                       int t, int shared, const int32_t* __restrict__ lens,
                       float* __restrict__ lp_acc, const int32_t* __restrict__ ids,
                       int ids_stride, float* __restrict__ step_lp, int32_t* __restrict__ rank,
                       int32_t* __restrict__ src_row) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const int n = r / S, s = r - n * S;
  const float* row = logits + (size_t)(shared ? n * S : r) * row_stride;
  float v[J], mx, lse;
  step_row_log_softmax<J>(row, K, lane, v, mx, lse);
  const int id = min(max(ids[(size_t)r * ids_stride], 0), K - 1);
  // the given cell's logit: lane id % 64 holds it in slot id / 64 (static indexing: no scratch)
  float mine = 0.f;
#pragma unroll
  for (int j = 0; j < J; ++j)
    if (j == (id >> 6)) mine = v[j];
  const float vid = __shfl(mine, id & 63, 64);
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int k = lane + 64 * j;
    if (k < K && (v[j] > vid || (v[j] == vid && k < id))) cnt += 1;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
  if (shared && s != 0) step_row_copy_out<J>(logits + (size_t)r * row_stride, K, lane, v);
  if (lane == 0) {
    const bool live = !lens || t < lens[r];
    const float lp = (vid - mx) - lse;
    step_lp[(size_t)r * ids_stride] = live ? lp : 0.f;
    rank[(size_t)r * ids_stride] = live ? cnt : -1;
    if (live) lp_acc[r] += lp;
    if (src_row) src_row[r] = n;
  }
}

// ------------------------------------------------------------ sampling without replacement
// Stochastic beam search (Kool, van Hoof, Welling, ICML 2019; defined in
// include/multiverse_hip.h mv_set_sampling_mode): one step in two launches, split as the beam's.
//   sbs_perturb_kernel  one WAVE per parent row r = n * B + b, the row in registers (lane l owns
//                       k = l + 64 j; no LDS, no scratch):
//                         lp = log_softmax(l) through step_row_log_softmax;  q = lp at
//                         temperature 1, else log_softmax(l / temperature) formed the same way
//                         g[k] = (phi_b + q[k]) - log(-log(u(b * K + k, seed_n, t)))
//                         Z = max_k g[k] (butterfly);  d = g[k] - Z
//                         v = (G_b - g[k]) + log(-expm1(d)), -inf at d == 0
//                         cand[r, k] = (G_b - max(v, 0)) - log1p(exp(-|v|))
//                       and the planes lp [R, K] and (temperature != 1) q [R, K] the selection
//                       forms a winner's LP and phi from.  t == 0: only slot 0 of a sample is a
//                       candidate row (the root; its phi and G are read at n * B).
//   sbs_select_kernel   beam_select_kernel's algorithm over cand; winner j from (b, k) carries
//                       G = cand, phi = phi_b + q[k], LP = LP_b + lp[k], parent b, id k.
// params: {seed, temperature bits, top_k, top_p bits} of the sampler, read on the device.
// With a top-k / nucleus limit on (step_row_keep_threshold; floor = B at t == 0, else 1), q is
// renormalised over the kept cells and a dropped cell is the candidate -inf, never selected.

// Masked (mv_set_cell_mask; terms.amask + n * mask_stride = the sample's plane at this step): a
// cell outside the plane is absent from the proposal as in sample_step_kernel -- q = cand = -inf --
// and the q plane is always written (sbs_select_kernel's force_q).
// Biased (mv_set_cell_bias; amask may be NULL): w = l / temperature + b with
// b = bias + n * bias_stride; q, the limits' order and the q plane follow w as in
// sample_step_kernel.
// Motion (bias may be NULL): b is step_row_motion's b_eff of parent row r.
// Path (mo.vel may be NULL): b is step_row_path's, and the row's set is stored.
template <int J, RowForm F>
__global__ __launch_bounds__(256)
void sbs_perturb_kernel(const float* __restrict__ logits, const float* __restrict__ prev_phi,
                        const float* __restrict__ prev_g, int R, int B, int K, int t,
                        const uint32_t* __restrict__ params, int floor,
                        float* __restrict__ cand, float* __restrict__ lp_plane,
                        float* __restrict__ q_plane, RowTerms terms) {
  constexpr bool MASKED = row_has_bits(F), BIASED = row_has_bias(F);
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const int n = r / B, b = r - n * B;
  if (t == 0 && b != 0) return;              // the root's K children are the candidates
  float v[J], mx, lse;
  step_row_log_softmax<J>(logits + (size_t)r * K, K, lane, v, mx, lse);
  const uint32_t seed = params[0] + (uint32_t)n * kSampleRowSeed;
  const float temperature = __builtin_bit_cast(float, params[1]);
  const bool tempered = temperature != 1.f;  // uniform
  float mxq = mx, lseq = lse;
  float w[J];
#pragma unroll
  for (int j = 0; j < J; ++j) w[j] = tempered ? v[j] / temperature : v[j];
  uint32_t am = 0u;
  if constexpr (MASKED) {
    float bz[BIASED ? J : 1];
    step_row_terms<J, F>(terms, n, r, B, K, lane, am, bz);
    if constexpr (BIASED) {
#pragma unroll
      for (int j = 0; j < J; ++j) w[j] = w[j] + bz[j];
    }
#pragma unroll
    for (int j = 0; j < J; ++j)
      if (!step_cell_in<true>(am, lane, j, K)) w[j] = -INFINITY;
  }
  if (tempered || MASKED) step_regs_log_softmax<J, MASKED>(w, K, lane, mxq, lseq, am);
  // top-k / nucleus limits (mv_set_sampling_truncation): q renormalised over the kept cells; a
  // dropped cell is no candidate (q = cand = -inf, written as such, not computed)
  const int top_k = (int)params[2];
  const float top_p = __builtin_bit_cast(float, params[3]);
  const bool limited = top_k > 0 || top_p < 1.f;   // uniform
  uint32_t thr = 0u;
  if (limited)
    thr = step_row_keep_threshold<J, MASKED, BIASED>(v, w, mxq, K, lane, top_k, top_p, floor, lseq,
                                                     am);
  const float phi = prev_phi[r], G = prev_g[r];
  float* lp_out = lp_plane + (size_t)r * K;
  float* q_out = q_plane + (size_t)r * K;
  float Z = -INFINITY;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int k = lane + 64 * j;
    if (k < K) {
      const float lp = (v[j] - mx) - lse;
      const bool kept = step_cell_in<MASKED>(am, lane, j, K) &&
                        (!limited || float_order_key(BIASED ? w[j] : v[j]) >= thr);
      // == lp bit for bit at temperature 1 with the limits off
      const float q = kept ? (w[j] - mxq) - lseq : -INFINITY;
      lp_out[k] = lp;
      if (tempered || limited || MASKED) q_out[k] = q;
      const float u = sample_uniform((uint32_t)b * (uint32_t)K + (uint32_t)k, seed, (uint32_t)t);
      w[j] = kept ? (phi + q) + (-logf(-logf(u))) : -INFINITY;
      Z = fmaxf(Z, w[j]);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) Z = fmaxf(Z, __shfl_xor(Z, off, 64));
  float* out = cand + (size_t)r * K;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int k = lane + 64 * j;
    if (k < K) {
      const float g = w[j], d = g - Z;
      const float vv = d < 0.f ? (G - g) + logf(-expm1f(d)) : -INFINITY;
      out[k] = g == -INFINITY ? -INFINITY : (G - fmaxf(vv, 0.f)) - log1pf(expf(-fabsf(vv)));
    }
  }
}

// Dynamic LDS as beam_select_kernel: cand [B*K] + 2 x 16 (value, index) reduction entries.
__global__ __launch_bounds__(1024)
void sbs_select_kernel(const float* __restrict__ cand, const float* __restrict__ lp_plane,
                       const float* __restrict__ q_plane, const uint32_t* __restrict__ params,
                       const float* __restrict__ prev_phi, const float* __restrict__ prev_lp,
                       int B, int K, int t, float* __restrict__ new_phi,
                       float* __restrict__ new_lp, float* __restrict__ new_g,
                       int32_t* __restrict__ ids, int32_t* __restrict__ parents,
                       int32_t* __restrict__ state_src_row, int state_rows_per_sample,
                       int32_t* __restrict__ row_ref, int force_q = 0) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ncand = (t > 0) ? B * K : K;
  float* lp = sm;
  float* redv = sm + B * K;                              // [2][16]
  int* redi = reinterpret_cast<int*>(redv + 32);         // [2][16]
  const float* src = cand + (size_t)n * B * K;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int v = tid; v < ncand; v += 1024) {
    const float x = src[v];
    lp[v] = x;
    if (beam_better(x, v, best, bi)) { best = x; bi = v; }
  }
  for (int sel = 0; sel < B; ++sel) {
    float wv = best;
    int wi = bi;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(wv, off, 64);
      const int oi = __shfl_xor(wi, off, 64);
      if (beam_better(ov, oi, wv, wi)) { wv = ov; wi = oi; }
    }
    const int pp = (sel & 1) * 16;
    if (lane == 0) { redv[pp + wave] = wv; redi[pp + wave] = wi; }
    __syncthreads();
    wv = redv[pp];
    wi = redi[pp];
#pragma unroll
    for (int w = 1; w < 16; ++w) {
      const float ov = redv[pp + w];
      const int oi = redi[pp + w];
      if (beam_better(ov, oi, wv, wi)) { wv = ov; wi = oi; }
    }
    if (tid == 0) {
      // (no candidate ranked: NaN logits; none is made -- the clamp keeps the reads in the row)
      const int flat = min(max(wi, 0), ncand - 1);
      const int par = flat / K;
      const size_t o = (size_t)n * B + sel, pr = (size_t)n * B + par;
      const size_t cell = (size_t)n * B * K + flat;
      // the q plane exists when the proposal differs from the model: tempered, truncated or
      // (force_q) under a cell mask or a cell bias
      const bool has_q = force_q != 0 ||
                         __builtin_bit_cast(float, params[1]) != 1.f || (int)params[2] > 0 ||
                         __builtin_bit_cast(float, params[3]) < 1.f;
      const float lpk = lp_plane[cell];
      new_g[o] = wv;
      new_phi[o] = prev_phi[pr] + (has_q ? q_plane[cell] : lpk);
      new_lp[o] = prev_lp[pr] + lpk;
      ids[o] = flat - par * K;
      parents[o] = par;
      if (state_src_row) state_src_row[o] = n * state_rows_per_sample + par;
      if (row_ref) row_ref[n * state_rows_per_sample + par] = 1;   // a state row some beam continues
    }
    if (wi < ncand && (wi & 1023) == tid) {   // the owner removes the winner and rescans its own
      lp[wi] = -INFINITY;
      best = -INFINITY;
      bi = 0x7fffffff;
      for (int v = tid; v < ncand; v += 1024) {
        const float x = lp[v];
        if (beam_better(x, v, best, bi)) { best = x; bi = v; }
      }
    }
  }
}

// ------------------------------------------------------------ batch assembly
// Dense regression maps from one (x, y) per row-step: out[r, cell, :] =
// (float)(xy[r, :] - centre[cell, :]) in double, the rounding of
// code/preprocess.py:463-475; rows of samples n >= num_rows are zero.
__global__ void regress_from_xy_kernel(const double* __restrict__ xy,
                                       const double* __restrict__ centers,
                                       float* __restrict__ out, int rows, int T, int K,
                                       int num_rows) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;   // (row-step, cell)
  if (idx >= (size_t)rows * K) return;
  const int r = (int)(idx / K), cell = (int)(idx - (size_t)r * K);
  float2 v = {0.f, 0.f};
  if (r / T < num_rows) {
    v.x = (float)(xy[2 * (size_t)r] - centers[2 * cell]);
    v.y = (float)(xy[2 * (size_t)r + 1] - centers[2 * cell + 1]);
  }
  reinterpret_cast<float2*>(out)[idx] = v;
}

__global__ void u8_to_f32_kernel(const uint8_t* __restrict__ in, float* __restrict__ out,
                                 size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (float)in[i];
}

}  // namespace mv
