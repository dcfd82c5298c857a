// Multi-future decode of the LAST forward's outputs, where they already are (HBM): pixel
// trajectories and the beams' occupancy map -- part of the ONE translation unit engine.hip
// (included from there, in order; not a stand-alone header).
//
//   decode_traj_kernel      code/multifuture_inference.py:475-517  ids + offsets -> (x, y)
//   beam_occupancy_kernel   code/multifuture_eval_trajs_prob.py:19-34, 88-93
//
// Neither is part of the captured forward; mv_decode_trajectories / mv_beam_occupancy queue
// them on the handle's stream behind it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mv {

constexpr int kMfBlock = 256;                 // threads of both kernels: 4 waves of 64
constexpr int kMfWaves = kMfBlock / 64;
constexpr int kOccBeamChunk = 20;             // beams of one (n, t) held in registers at a time

// out[n, b, t, :] = centers[id] (+ reg[n, t, id, :] unless center_only), as doubles: the
// centre is a double, the offset a float widened to double, ONE IEEE add -- the operation numpy
// performs in the reference's loop, so the result is bit-identical.
//   ids != NULL (beam):    id = ids[n, b, t]; one thread per (n, b, t), `rows` = N*B*T of them.
//   ids == NULL (greedy):  B = 1, id = argmax_k cls[n, t, k] with numpy's rule (FIRST index of
//     the maximum); one wave per (n, t) row, `rows` = N*T.  A lane keeps the first maximum of
//     its cells k = lane, lane + 64, ..; the wave reduction carries (value, index) and breaks
//     ties toward the lower index.  (NaN logits are not ranked; the engine produces none.)
// reg is [N, T, K, 2]; an id outside [0, K) -- none is produced -- is clamped rather than
// followed outside the buffers.
// RAGGED (per-row lengths `lens`, mv_set_pred_lengths): a row (n, b, t) with t >= lens[n] is
// past its sample's end and decodes to (0, 0); the others exactly as without lengths.  (Here and
// below, a kernel instantiated without RAGGED does not read `lens` at all.)
template <bool RAGGED>
__global__ __launch_bounds__(kMfBlock) void decode_traj_kernel(
    const int32_t* __restrict__ ids, const float* __restrict__ cls,
    const float* __restrict__ reg, const double* __restrict__ centers,
    double* __restrict__ out, int rows, int B, int T, int K, int center_only,
    const int32_t* __restrict__ lens) {
  const int lane = threadIdx.x & 63;
  int row, id;
  if (ids) {
    row = blockIdx.x * kMfBlock + threadIdx.x;
    if (row >= rows) return;
  } else {
    row = blockIdx.x * kMfWaves + (threadIdx.x >> 6);
    if (row >= rows) return;                       // wave-uniform
  }
  if constexpr (RAGGED) {
    if (row % T >= lens[row / (T * B)]) {          // greedy: wave-uniform
      if (ids || lane == 0) { out[2 * (size_t)row] = 0.0; out[2 * (size_t)row + 1] = 0.0; }
      return;
    }
  }
  if (ids) {
    id = ids[row];
    if constexpr (RAGGED) {
      // a scoring forward's lengths are per future: -1 marks a step past this future's own end
      if (id < 0) { out[2 * (size_t)row] = 0.0; out[2 * (size_t)row + 1] = 0.0; return; }
    }
  } else {
    const float* x = cls + (size_t)row * K;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    if (lane < K) { best = x[lane]; bi = lane; }
    for (int k = lane + 64; k < K; k += 64) {
      const float v = x[k];
      if (v > best) { best = v; bi = k; }          // strict: the lane's first maximum stays
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const float ov = __shfl_xor(best, off);
      const int oi = __shfl_xor(bi, off);
      if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    if (lane != 0) return;
    id = bi;
  }
  id = min(max(id, 0), K - 1);
  // (n, b, t) -> the offsets of (n, t): they do not depend on the beam
  const int t = row % T, n = row / (T * B);
  double x = centers[2 * id], y = centers[2 * id + 1];
  if (!center_only) {
    const float* r = reg + (((size_t)n * T + t) * K + id) * 2;
    x = x + (double)r[0];
    y = y + (double)r[1];
  }
  out[2 * (size_t)row] = x;
  out[2 * (size_t)row + 1] = y;
}

// Block-wide max / sum of `cnt` values per thread in ONE pass over LDS: butterfly within each
// wave (every lane ends with the wave's result), the kMfWaves partials through `red`, combined
// by every thread in wave order -- a fixed order, so the result is bitwise reproducible.
// red: [kOccBeamChunk][kMfWaves] floats.  Ends with the block in step (two barriers).
template <bool kMax, int CNT>
__device__ __forceinline__ void occ_block_reduce(float (&v)[CNT], float* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < CNT; ++j) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const float o = __shfl_xor(v[j], off);
      v[j] = kMax ? fmaxf(v[j], o) : v[j] + o;
    }
    if (lane == 0) red[j * kMfWaves + wave] = v[j];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < CNT; ++j) {
    float r = red[j * kMfWaves];
#pragma unroll
    for (int w = 1; w < kMfWaves; ++w)
      r = kMax ? fmaxf(r, red[j * kMfWaves + w]) : r + red[j * kMfWaves + w];
    v[j] = r;
  }
  __syncthreads();                                 // red is free again
}

// w[b] = softmax_b(lp[b]) of one sample, fp32, sequential over b (every thread the same).
__device__ __forceinline__ void occ_beam_weight_norm(const float* __restrict__ lp, int B,
                                                     float* m_out, float* s_out) {
  float m = lp[0];
  for (int b = 1; b < B; ++b) m = fmaxf(m, lp[b]);
  float s = 0.f;
  for (int b = 0; b < B; ++b) s += expf(lp[b] - m);
  *m_out = m;
  *s_out = s;
}

// out[n, t, k] = sum_b w[n, b] * softmax_k(logits[n, b, t, :])[k], w[n, :] = softmax_b(lp[n, :]),
// fp32 throughout, as the reference evaluates it: softmax = exp(x - max) / sum, the product
// with w rounded, the beams added in the order b = 0, 1, ...  One workgroup per (n, t).
// K <= CPT * 256: a thread holds its CPT cells of up to kOccBeamChunk beams in registers, so
// every logits row is read from HBM once and the row maxima / sums of a whole chunk of beams
// cost two barriers each.  Reductions in a fixed order, no atomics: the map is bitwise
// reproducible, and a row's result depends on that row alone.
// RAGGED (per-row lengths): the map of a step past its sample's end (t >= lens[n]) is 0.
// MASKED (mv_set_cell_mask): every future's step map is the softmax over the allowed cells of
// (n, t) -- maximum and sum over them, a cell outside exactly 0.0f; the plane is
// amask + n * mask_stride + t * mask_step, read once into one bit per owned cell.
// BIASED (mv_set_cell_bias; implies MASKED, amask may be NULL = every cell of the row): the step
// map is the softmax of l + b over the allowed cells, b = bias + n * bias_stride + t * bias_step,
// read once into a register per owned cell.
template <int CPT, bool RAGGED, bool MASKED = false, bool BIASED = false>
__global__ __launch_bounds__(kMfBlock) void beam_occupancy_kernel(
    const float* __restrict__ logits, const float* __restrict__ lp, float* __restrict__ out,
    int B, int T, int K, const int32_t* __restrict__ lens,
    const uint8_t* __restrict__ amask = nullptr, int64_t mask_stride = 0, int64_t mask_step = 0,
    const float* __restrict__ bias = nullptr, int64_t bias_stride = 0, int64_t bias_step = 0) {
  static_assert(MASKED || !BIASED, "the BIASED form works on the allowed bits");
  __shared__ float red[kOccBeamChunk * kMfWaves];
  const int n = blockIdx.x / T, t = blockIdx.x % T, tid = threadIdx.x;
  uint32_t am = 0u;                                // MASKED: bit c = cell tid + c * 256 is allowed
  if constexpr (MASKED) {
    const uint8_t* plane = amask + (size_t)n * mask_stride + (size_t)t * mask_step;
    const bool all = BIASED && !amask;             // block-uniform
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
      const int k = tid + c * kMfBlock;
      if (k < K && (all || plane[k] != 0)) am |= 1u << c;
    }
  }
  float bz[BIASED ? CPT : 1];
  if constexpr (BIASED) {
    const float* plane = bias + (size_t)n * bias_stride + (size_t)t * bias_step;
#pragma unroll
    for (int c = 0; c < CPT; ++c) bz[c] = plane[min(tid + c * kMfBlock, K - 1)];
  }
  // cell c of this thread takes part in the softmax (the unmasked form does not read `am`)
  auto in = [&](int c) {
    if constexpr (MASKED) return ((am >> c) & 1u) != 0u;
    else return tid + c * kMfBlock < K;
  };
  if constexpr (RAGGED) {
    if (t >= lens[n]) {                            // block-uniform, before any barrier
      for (int k = tid; k < K; k += kMfBlock) out[(size_t)blockIdx.x * K + k] = 0.f;
      return;
    }
  }
  float wm, ws;
  occ_beam_weight_norm(lp + (size_t)n * B, B, &wm, &ws);
  float acc[CPT];
#pragma unroll
  for (int c = 0; c < CPT; ++c) acc[c] = 0.f;
  for (int b0 = 0; b0 < B; b0 += kOccBeamChunk) {
    float v[kOccBeamChunk][CPT];
    float mx[kOccBeamChunk], sm[kOccBeamChunk];
    const float* x0 = logits + (((size_t)n * B + b0) * T + t) * K;
#pragma unroll
    for (int j = 0; j < kOccBeamChunk; ++j) {
      const bool live = b0 + j < B;                // block-uniform
      const float* x = x0 + (size_t)j * T * K;     // beam b0 + j
      mx[j] = -INFINITY;
#pragma unroll
      for (int c = 0; c < CPT; ++c) {
        const int k = tid + c * kMfBlock;
        // a cell past the row reads the row's last one (no divergent load) and is masked
        float xv = live ? x[min(k, K - 1)] : 0.f;
        if constexpr (BIASED) xv = xv + bz[c];
        v[j][c] = (live && in(c)) ? xv : -INFINITY;
        mx[j] = fmaxf(mx[j], v[j][c]);
      }
    }
    occ_block_reduce<true>(mx, red);
#pragma unroll
    for (int j = 0; j < kOccBeamChunk; ++j) {
      sm[j] = 0.f;
#pragma unroll
      for (int c = 0; c < CPT; ++c) {
        v[j][c] = (b0 + j < B && in(c)) ? expf(v[j][c] - mx[j]) : 0.f;
        sm[j] += v[j][c];
      }
    }
    occ_block_reduce<false>(sm, red);
#pragma unroll
    for (int j = 0; j < kOccBeamChunk; ++j) {
      if (b0 + j >= B) continue;
      const float w = expf(lp[(size_t)n * B + b0 + j] - wm) / ws;
#pragma unroll
      for (int c = 0; c < CPT; ++c) acc[c] += (v[j][c] / sm[j]) * w;
    }
  }
#pragma unroll
  for (int c = 0; c < CPT; ++c) {
    const int k = tid + c * kMfBlock;
    if (k < K) out[(size_t)blockIdx.x * K + k] = acc[c];
  }
}

// Any K: the same arithmetic in the same order, one beam at a time; a thread's cells are
// k = tid, tid + 256, ...  The row is read three times (maximum, sum, accumulation), the second
// and third time from cache; the running map lives in the output row, which only this
// workgroup -- and each cell only its own thread -- touches.
// MASKED and BIASED as above; the planes are read beside the row in every pass.
template <bool RAGGED, bool MASKED = false, bool BIASED = false>
__global__ __launch_bounds__(kMfBlock) void beam_occupancy_anyk_kernel(
    const float* __restrict__ logits, const float* __restrict__ lp, float* __restrict__ out,
    int B, int T, int K, const int32_t* __restrict__ lens,
    const uint8_t* __restrict__ amask = nullptr, int64_t mask_stride = 0, int64_t mask_step = 0,
    const float* __restrict__ bias = nullptr, int64_t bias_stride = 0, int64_t bias_step = 0) {
  static_assert(MASKED || !BIASED, "the BIASED form works on the allowed bits");
  __shared__ float red[kOccBeamChunk * kMfWaves];
  const int n = blockIdx.x / T, t = blockIdx.x % T, tid = threadIdx.x;
  if constexpr (RAGGED) {
    if (t >= lens[n]) {                            // block-uniform, before any barrier
      for (int k = tid; k < K; k += kMfBlock) out[(size_t)blockIdx.x * K + k] = 0.f;
      return;
    }
  }
  float wm, ws;
  occ_beam_weight_norm(lp + (size_t)n * B, B, &wm, &ws);
  float* o = out + (size_t)blockIdx.x * K;
  const uint8_t* am = nullptr;
  if constexpr (MASKED)
    if (!BIASED || amask) am = amask + (size_t)n * mask_stride + (size_t)t * mask_step;
  const float* bz = nullptr;
  if constexpr (BIASED) bz = bias + (size_t)n * bias_stride + (size_t)t * bias_step;
  auto in = [&](int k) {
    if constexpr (BIASED) return !am || am[k] != 0;
    else if constexpr (MASKED) return am[k] != 0;
    else return true;
  };
  for (int b = 0; b < B; ++b) {
    const float* x = logits + (((size_t)n * B + b) * T + t) * K;
    // the cell's logit, plus its cost in the BIASED form
    auto xb = [&](int k) { if constexpr (BIASED) return x[k] + bz[k]; else return x[k]; };
    float mx[1] = {-INFINITY};
    for (int k = tid; k < K; k += kMfBlock) if (in(k)) mx[0] = fmaxf(mx[0], xb(k));
    occ_block_reduce<true>(mx, red);
    float sm[1] = {0.f};
    for (int k = tid; k < K; k += kMfBlock) if (in(k)) sm[0] += expf(xb(k) - mx[0]);
    occ_block_reduce<false>(sm, red);
    const float w = expf(lp[(size_t)n * B + b] - wm) / ws;
    for (int k = tid; k < K; k += kMfBlock) {
      const float p = in(k) ? (expf(xb(k) - mx[0]) / sm[0]) * w : 0.f;
      o[k] = b == 0 ? p : o[k] + p;
    }
  }
}

}  // namespace mv
