// ConvLSTM step, f16x3 arithmetic, with the 3x3 gate convolution in Winograd F(3,3) form
// along the image's ROW axis: five products per THREE output rows and stencil column -- 5/9 of
// the matrix-pipe work of the direct form (convlstm_f16x3.h), 5/6 of the F(2,3) row-pair form
// (convlstm_wino.h) -- for the same pre-activations.
//
// Why (profiles/r5b_energy_attribution.md): the F(2,3) kernel
// runs at the package power cap, and the attribution of its energy per launch puts ~4/5 of
// the dynamic energy into the MFMAs themselves (dropping two of the three MFMAs of every
// product saves more than half of the launch's energy).  What is left to cut is MFMAs per
// product.  18 = 6 x 3 and 9 = 3 x 3: on the grids of the published configuration row
// triples tile exactly (F(4,3) needs a fifth, half-empty tile at 18 rows and computes 12 rows
// for 9: 30 and 18 products per column against 30 and 15 here, 36 and 20 for F(2,3)).
//
// Algebra (points 0, 1, -1, 2, inf; d0..d4 = input rows 3t-1 .. 3t+3, g0..g2 = the kernel rows
// of one stencil column dx; numpy twin: tests/test_wino_model.py):
//     V0 = 2 (d0 - d2) + V3          U0 = g0 / 2                 y(3t)   = M0 + M1 + M2 + M3
//     V1 = (d3 - d2) - 2 d1          U1 = -(g0 + g1 + g2) / 2    y(3t+1) = M1 - M2 + 2 M3
//     V2 = 2 (d1 - d2) + (d3 - d2)   U2 = (-g0 + g1 - g2) / 6    y(3t+2) = M1 + M2 + 4 M3 + M4
//     V3 = d3 - d1                   U3 = (g0 + 2 g1 + 4 g2) / 6
//     V4 = 2 V3 + (d2 - d4)          U4 = -g2
// M_c[triple-cell][column] = sum_{dx, ci} V_c[triple-cell + dx][ci] U_c[dx][ci][column].
// As in the row-pair form the dx taps are ONE operand fragment per (component, 16 channels)
// moved a lane up / down the wave by DPP (a wave's 32 triple-cells are consecutive x of whole
// image rows: every W of the launch divides 32).
//
// Operands.  U_c in fp64 at pack time, two fp16 planes of 256 U (pack_wino3_kernel).  V_c IN
// the kernel from the ordinary operand planes (plane_layout.h): nine wn_lin<KA, KB> steps per
// 16 input channels, each KA a + KB b on (high, low) plane pairs with an error-free TwoSum of
// the high planes and the factors 2 folded into the fused multiply-adds (8 packed-fp16
// instructions per register, like wn_combine).  |256 V| <= 6 * 256: far inside fp16.
//
// Tile.  Weights = A operand (rows = 4 gates x 8 channels), activations = B operand (columns
// = 32 triple-cells), so a lane's accumulators hold i, j, f, o of four consecutive channels of
// ONE triple-cell.  A wave owns 32 triple-cells (96 cells) x 16 channels x 4 gates x 5
// components = 160 accumulator registers; a workgroup = 4 waves = 128 triple-cells of one
// 16-channel column block, TWO workgroups per CU (two waves per SIMD, <= 256 registers --
// possible because the main loop holds no operand rows and no transform temporaries, see
// below).  The (chunk, component) pairs are ONE sequence; an LDS stage holds two consecutive
// components (24 KB), double-buffered by LDS-DMA: 36 MFMAs per wave and barrier.
//
// What round 5 measured on the way here (profiles/r5*): with the input
// transform IN the kernel the row-triple form needs the operand rows of a chunk (40
// registers) next to 160 accumulators -- one wave per SIMD, one workgroup per CU.  In that
// regime nothing covers a workgroup's prologue, epilogue and dispatch (0.29 of 0.83 ms: the
// K loop of this problem is only 16-18 chunks long), and the shadow of an MFMA holds five
// single-issue instructions where transform + shifts + requests need seven: 3-6 % SLOWER
// than the row-pair kernel, hand-pipelined or not (profiles/r5f_*, r5h_*).  Hence the
// pre-pass: the transform once per operand instead of once per column block, and a gate
// kernel that fits twice on a CU again.
#pragma once
#include "convlstm_wino.h"

namespace mv {

template <int NRB>
struct Wn3 {
  static constexpr int kCh = 8 * NRB;                         // output channels per workgroup
  static constexpr int kChunkVec = 5 * 3 * 2 * NRB * 64;      // 16-byte vectors per chunk
  static constexpr uint32_t kChunkBytes = kChunkVec * 16;
  static constexpr int kTileFloats = 96 * kCh;                // state tile of a wave
};

static inline size_t wino3_wpack_elems(int Cx16, int C, int nrb) {   // in halves
  return (size_t)(C / (8 * nrb)) * (size_t)(Cx16 / 16 + C / 16) * 5 * 3 * 2 * nrb * 64 * 8;
}

// The pack, from the CURRENT device weights: one thread per (cb, chunk, comp, dx, rb, lane,
// element), both planes.  Layout [cb][chunk][comp 5][dx 3][plane 2][rb][lane 64][8]: a chunk
// IS the LDS image of its stage.  Element e of lane l: A-operand row l & 31 = gate (row >> 3),
// channel cb * 8 nrb + rb * 8 + (row & 7); k = 8 (l >> 5) + e = input channel of the chunk;
// chunks = x groups of 16 first, then h groups.
__global__ void pack_wino3_kernel(const float* __restrict__ w, _Float16* __restrict__ out,
                                  int Cx_total, int Cx16, int C, int nrb, size_t total) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int e = idx & 7;
  const int l = (idx >> 3) & 63;
  size_t t = idx >> 9;
  const int rb = (int)(t % nrb); t /= nrb;
  const int dx = (int)(t % 3); t /= 3;
  const int comp = (int)(t % 5); t /= 5;
  const int nxc = Cx16 / 16, nch = nxc + C / 16;
  const int chunk = (int)(t % nch), cb = (int)(t / nch);
  const bool is_x = chunk < nxc;
  const int cg = is_x ? chunk : chunk - nxc;
  const int k = 8 * (l >> 5) + e;
  const int cin = (is_x ? 0 : Cx_total) + cg * 16 + k;
  const int row = l & 31;
  const int n = (row >> 3) * C + cb * 8 * nrb + rb * 8 + (row & 7);
  const int Cin = Cx_total + C, N4 = 4 * C;
  const double g0 = w[((size_t)(0 * 3 + dx) * Cin + cin) * N4 + n];
  const double g1 = w[((size_t)(1 * 3 + dx) * Cin + cin) * N4 + n];
  const double g2 = w[((size_t)(2 * 3 + dx) * Cin + cin) * N4 + n];
  double u;
  switch (comp) {
    case 0: u = 0.5 * g0; break;
    case 1: u = -0.5 * (g0 + g1 + g2); break;
    case 2: u = (-g0 + g1 - g2) / 6.0; break;
    case 3: u = (g0 + 2.0 * g1 + 4.0 * g2) / 6.0; break;
    default: u = -g2; break;
  }
  const double sv = u * 256.0;
  note_pack_range(sv);
  const _Float16 v0 = (_Float16)sv;
  const _Float16 v1 = (_Float16)(sv - (double)v0);
  const size_t vec = ((((size_t)cb * nch + chunk) * 5 + comp) * 3 + dx) * 2;   // + plane
  out[(((vec + 0) * nrb + rb) * 64 + l) * 8 + e] = v0;
  out[(((vec + 1) * nrb + rb) * 64 + l) * 8 + e] = v1;
}

struct Wn3Consts { f16x8 m1, p2, m2; };   // (-1), (2), (-2) as packed halves (laundered SGPRs)

// KA (a_hi + a_lo) + KB (b_hi + b_lo) as a plane pair, KA in {1, 2}, KB in {1, -1, -2}: TwoSum
// of KA a_hi and KB b_hi (both exact in fp16), everything else into the low plane.  Every
// line is one packed instruction per register; the products by 1 / 2 are exact, so each
// fused multiply-add rounds exactly like the sum it stands for.
template <int KA, int KB>
__device__ __forceinline__ void wn_lin(const f16x8 a_hi, const f16x8 a_lo, const f16x8 b_hi,
                                       const f16x8 b_lo, const Wn3Consts& k, f16x8& hi,
                                       f16x8& lo) {
  static_assert((KA == 1 && (KB == 1 || KB == -1 || KB == -2)) || (KA == 2 && KB == 1), "form");
  const f16x8 nka = KA == 1 ? k.m1 : k.m2;                      // -KA
  f16x8 s, ne2, l1;
  if (KA == 2) {
    s = __builtin_elementwise_fma(a_hi, k.p2, b_hi);
    l1 = __builtin_elementwise_fma(a_lo, k.p2, b_lo);
  } else if (KB == 1) {
    s = a_hi + b_hi;
    l1 = a_lo + b_lo;
  } else {
    s = __builtin_elementwise_fma(b_hi, KB == -1 ? k.m1 : k.m2, a_hi);
    l1 = __builtin_elementwise_fma(b_lo, KB == -1 ? k.m1 : k.m2, a_lo);
  }
  const f16x8 bb = __builtin_elementwise_fma(a_hi, nka, s);    // the part of KB b_hi that arrived
  const f16x8 t = __builtin_elementwise_fma(bb, k.m1, s);      // the part of KA a_hi that arrived
  const f16x8 ne1 = __builtin_elementwise_fma(a_hi, nka, t);   // -(KA a_hi - t)
  if (KB == -1) ne2 = bb + b_hi;                                // -(KB b_hi - bb)
  else ne2 = __builtin_elementwise_fma(b_hi, KB == 1 ? k.m1 : k.p2, bb);
  hi = s;
  lo = __builtin_elementwise_fma(ne1 + ne2, k.m1, l1);
}

// ---------------------------------------------------------------- the input transform, ONCE
// In the kernel the transform costs 288 packed-fp16 instructions per wave and 16 input
// channels -- and every one of the C / 16 column-block workgroups that share a row tile redoes
// it.  With one wave per SIMD (the accumulator tile leaves no room for a second) those
// instructions have nowhere to hide: the shadow of an MFMA holds about five single-issue
// instructions (MI355X guide, "one wave per SIMD"), the transform alone needs 3.2 per MFMA.
// So the components are formed once per gate step by this pre-pass and the gate kernel loads
// them like any operand:
//   out[tile = q >> 5][channel group of 16][component 5][plane 2][k half 2][column q & 31][8]
// (q = triple-cell index rows x ceil(H / 3) x W; 16 bytes per lane, the 64 lanes of a wave one
// contiguous KB: lane l IS (k half = l >> 5, column = l & 31), MFMA B-fragment order).  The
// beam's parent indirection is applied HERE (src_row), the gate kernel reads in output order.
// Same arithmetic as the in-kernel form (wn_lin chain, error-free TwoSum of the high planes).
struct Wn3TransformItem {
  const _Float16* p0;        // plane 0 of the operand (tiled layout, plane_layout.h)
  int64_t pstride;           // halves to plane 1
  _Float16* out;
  const int32_t* src_row;    // optional [rows]
  int32_t rows, H, W, Cc;    // Cc: channels, a multiple of 16
  // light cone of the class encoder (ConvLstmArgs::cone_*): the tiles to transform (null: all),
  // which (row, triple) tiles the previous step computed (null: all), rows - 1 = background row
  const int32_t* cone_list;
  const int32_t* cone_prev;
  int32_t cone_cells;        // host-side: cells transformed (0: rows * H * W)
};
constexpr int kW3TrGroup = 8;
struct Wn3TransformGroup {
  Wn3TransformItem it[kW3TrGroup];
  int32_t blk_end[kW3TrGroup];
  int32_t n;
};
static inline size_t wino3_v_elems(int rows, int H, int W, int Cc) {   // in halves
  const size_t Q = (size_t)rows * ((H + 2) / 3) * W;
  return ((Q + 31) / 32) * (size_t)(Cc / 16) * 5 * 2 * 64 * 8;
}
static inline unsigned wino3_transform_blocks(int rows, int H, int W, int Cc) {
  const size_t Q = (size_t)rows * ((H + 2) / 3) * W;
  return (unsigned)((((Q + 31) / 32) * (size_t)(Cc / 16) + 3) / 4);     // 4 waves per block
}
__global__ __launch_bounds__(256)
void wino3_transform_kernel(const Wn3TransformGroup g) {
  int block = blockIdx.x, pi = 0;
#pragma unroll
  for (int i = 0; i < kW3TrGroup - 1; ++i)
    if (i + 1 < g.n && (int)blockIdx.x >= g.blk_end[i]) pi = i + 1;
  if (pi > 0) block -= g.blk_end[pi - 1];
  const Wn3TransformItem& it = g.it[pi];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int KG = it.Cc >> 4;
  const int H = it.H, W = it.W, HW = H * W;
  const int Kt = ((H + 2) / 3) * W, Q_total = it.rows * Kt;
  const int ntile = (Q_total + 31) >> 5;
  const int wid = block * 4 + wave;
  if (wid >= ntile * KG) return;
  int tile = wid / KG;
  const int cg = wid - tile * KG;
  if (it.cone_list) {        // the grid is the dense one: waves past the count have nothing to do
    if (tile >= it.cone_list[0]) return;
    tile = it.cone_list[4 + tile];
  }
  const int col = lane & 31, half = lane >> 5;
  const int q = tile * 32 + col;
  const bool valid = q < Q_total;
  int r = 0, y0 = 0, xpos = 0;
  if (valid) {
    r = q / Kt;
    const int pc = q - r * Kt;
    const int t = pc / W;
    y0 = 3 * t;
    xpos = pc - t * W;
  }
  const int sr = (valid && it.src_row) ? it.src_row[r] : r;
  // light cone: rows d1 .. d3 are the lane's own triple, d0 / d4 the neighbour triples'; a
  // (row, triple) tile the previous step did not compute holds the background row's values
  int sr_up = sr, sr_mid = sr, sr_dn = sr;
  if (it.cone_prev && valid) {
    const int bg = it.rows - 1;
    const int* prev = it.cone_prev;
    sr_mid = prev[q >> 5] ? sr : bg;
    sr_up = (y0 > 0 && !prev[(q - W) >> 5]) ? bg : sr;
    sr_dn = (y0 + 3 < H && !prev[(q + W) >> 5]) ? bg : sr;
  }
  f16x8 dh[5], dl[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int rho = y0 - 1 + i;
    const bool ok = valid & (rho >= 0) & (rho < H);
    const long long m = (long long)(i == 0 ? sr_up : (i == 4 ? sr_dn : sr_mid)) * HW + rho * W + xpos;
    const size_t o = ((size_t)(m >> 5) * KG + cg) * 512 + (size_t)(half * 256 + (int)(m & 31) * 8);
    const f16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    dh[i] = ok ? *reinterpret_cast<const f16x8*>(it.p0 + o) : z;
    dl[i] = ok ? *reinterpret_cast<const f16x8*>(it.p0 + it.pstride + o) : z;
  }
  uint32_t mone = 0xBC00BC00u, ptwo = 0x40004000u, mtwo = 0xC000C000u;   // opaque to hipcc
  asm volatile("" : "+s"(mone), "+s"(ptwo), "+s"(mtwo));
  Wn3Consts kc;
  kc.m1 = __builtin_bit_cast(f16x8, u32x4{mone, mone, mone, mone});
  kc.p2 = __builtin_bit_cast(f16x8, u32x4{ptwo, ptwo, ptwo, ptwo});
  kc.m2 = __builtin_bit_cast(f16x8, u32x4{mtwo, mtwo, mtwo, mtwo});
  f16x8 vh[5], vl[5], th, tl, t3h, t3l;
  wn_lin<1, -1>(dh[3], dl[3], dh[1], dl[1], kc, vh[3], vl[3]);     // V3 = d3 - d1
  wn_lin<1, -1>(dh[0], dl[0], dh[2], dl[2], kc, th, tl);           // d0 - d2
  wn_lin<2, 1>(th, tl, vh[3], vl[3], kc, vh[0], vl[0]);            // V0
  wn_lin<1, -1>(dh[3], dl[3], dh[2], dl[2], kc, t3h, t3l);         // d3 - d2
  wn_lin<1, -2>(t3h, t3l, dh[1], dl[1], kc, vh[1], vl[1]);         // V1
  wn_lin<1, -1>(dh[1], dl[1], dh[2], dl[2], kc, th, tl);           // d1 - d2
  wn_lin<2, 1>(th, tl, t3h, t3l, kc, vh[2], vl[2]);                // V2
  wn_lin<1, -1>(dh[2], dl[2], dh[4], dl[4], kc, th, tl);           // d2 - d4
  wn_lin<2, 1>(vh[3], vl[3], th, tl, kc, vh[4], vl[4]);            // V4
  f16x8* o = reinterpret_cast<f16x8*>(it.out) + ((size_t)tile * KG + cg) * (5 * 2 * 64) + lane;
#pragma unroll
  for (int c = 0; c < 5; ++c) {
    o[(c * 2 + 0) * 64] = vh[c];
    o[(c * 2 + 1) * 64] = vl[c];
  }
}
static inline void launch_wino3_transforms(const Wn3TransformItem* items, int n,
                                           hipStream_t stream) {
  for (int i0 = 0; i0 < n; i0 += kW3TrGroup) {
    Wn3TransformGroup g{};
    g.n = n - i0 < kW3TrGroup ? n - i0 : kW3TrGroup;
    unsigned nb = 0;
    for (int j = 0; j < g.n; ++j) {
      g.it[j] = items[i0 + j];
      nb += wino3_transform_blocks(g.it[j].rows, g.it[j].H, g.it[j].W, g.it[j].Cc);
      g.blk_end[j] = (int32_t)nb;
    }
    for (int j = g.n; j < kW3TrGroup; ++j) g.blk_end[j] = (int32_t)nb;
    if (nb) hipLaunchKernelGGL(wino3_transform_kernel, dim3(nb), dim3(256), 0, stream, g);
  }
}

// HALO: grids whose width does not divide 32.  A wave's 32 lanes are still 32 CONSECUTIVE
// triple-cells, so the DPP lane shift still finds the x neighbour -- except for the tile's first
// and last lane, whose neighbours sit in other waves.  With HALO a wave's tile starts one
// triple-cell early and OWNS only its inner 30 lanes: lanes 0 and 31 load and multiply like the
// rest (their fragments are the neighbours of lanes 1 and 30) but store nothing -- 1 / 16 of the
// matrix work for any W (the literal 36 x 18 / 18 x 9 grids of BASELINE.json, --scene_h /
// --scene_w other than 36 x 64).
// BF16D (round 6): the same tile, block map, halo tiling and epilogue around a DIRECT 3x3 main
// loop on ONE bf16 plane per operand (compute mode 2): three accumulator sets (the output rows
// 3t .. 3t + 2) instead of five components, raw operand rows instead of pre-transformed ones,
// one MFMA per product.  Against the 32-cell tile of convlstm_f16x3.h's bf16 body each weight
// fragment read from LDS feeds THREE MFMAs (the three output rows) instead of one, and a stage
// = a whole chunk: 54 MFMAs per wave and barrier on 18 KB of weights -- 0.5 KB moved per MFMA
// instead of 1.2.
template <int WAVES, int NRB, bool HALO, bool BF16D = false>
__device__ __forceinline__ void convlstm_wino3_body(const ConvLstmWinoArgs& p, int cb, int mt,
                                                    f16x8* lds) {
  using G = Wn3<NRB>;
  constexpr int CH = G::kCh;
  constexpr int kOwn = HALO ? 30 : 32;                 // triple-cells a wave stores
  constexpr int kTriples = WAVES * kOwn;               // triple-cells per workgroup
  constexpr int kPieces = CH / 4;                      // 16-byte pieces of a tile row
  constexpr int kPasses = (96 * kPieces + 63) / 64;    // wave passes over a state tile
  const ConvLstm16Args& q = p.b;
  const ConvLstmArgs& a = q.f;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int H = a.H, W = a.W, HW = H * W, C = a.C, Cx = a.Cx;
  const int Ht = (H + 2) / 3, Kt = Ht * W;
  const int Q_total = a.rows * Kt;
  int q_own = mt * kTriples + wave * kOwn;             // first triple-cell the wave owns
  // light cone of the class encoder (exact tiling only): wave w of row tile mt takes entry
  // 4 mt + w of the step's tile list; the grid is the dense one (a captured graph must not hold
  // one batch's count), so a workgroup past the count leaves here, before its first barrier
  constexpr bool kCone = !HALO && !BF16D;
  bool cone_bg_src = false;                            // the wave's tile reads the background row's c
  if (kCone && a.cone_list) {
    const int cnt = a.cone_list[0];
    if (mt * WAVES >= cnt) return;
    const int li = mt * WAVES + wave;
    q_own = li < cnt ? 32 * a.cone_list[4 + li] : Q_total;
  }
  if (kCone && a.cone_prev && q_own < Q_total) cone_bg_src = a.cone_prev[q_own >> 5] == 0;
  const int q_wave = HALO ? q_own - 1 : q_own;         // ... and lane 0's
  const bool wave_live = q_own < Q_total;        // dead waves still copy and hit barriers
  const int col = lane & 31, half = lane >> 5;

  int r = 0, y0 = 0, xpos = 0;
  bool valid;
  {
    const int qq = q_wave + col;
    valid = qq >= 0 && qq < Q_total;
    if (valid) {
      r = qq / Kt;
      const int pc = qq - r * Kt;
      const int t = pc / W;
      y0 = 3 * t;
      xpos = pc - t * W;
    }
  }
  const int srh = (valid && a.src_row_h) ? a.src_row_h[r] : r;
  const bool okx0 = valid & (xpos > 0), okx2 = valid & (xpos + 1 < W);

  // operand rows y0 - 1 .. y0 + 3 of the lane's column: byte offsets of the lane's 16-byte
  // vector in channel group 0 of the tiled planes (from the zero pad in front of a plane, so
  // that offset 0 reads zeros); an out-of-image row reads offset 0
  uint32_t roffx[5], roffh[5];
  {
    const int KGx = Cx >> 4, KGh = C >> 4;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const int rho = y0 - 1 + i;
      const bool ok = valid & (rho >= 0) & (rho < H);
      const int cx = r * HW + rho * W + xpos, chh = srh * HW + rho * W + xpos;
      roffx[i] = ok ? (uint32_t)((((cx >> 5) * KGx) * 512 + half * 256 + (cx & 31) * 8 + kPlanePad) * 2) : 0u;
      roffh[i] = ok ? (uint32_t)((((chh >> 5) * KGh) * 512 + half * 256 + (chh & 31) * 8 + kPlanePad) * 2) : 0u;
    }
  }

  // acc[0..4]: the Winograd components (BF16D: acc[0..2] = the three output rows)
  constexpr int kAcc = BF16D ? 3 : 5;
  f32x16 acc[kAcc][NRB];
#pragma unroll
  for (int c = 0; c < kAcc; ++c)
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[c][rb][i] = 0.f;

  // LDS: [stage buffer 0 | stage buffer 1 (two components each; the epilogue reuses them as the
  // waves' h' tiles) | per wave: c tile 96 x CH floats | per wave: two tables of 96 cell
  // offsets (state source rows, output rows)]
  constexpr int kStageVec = BF16D ? 3 * 3 * NRB * 64         // a chunk: 9 taps, one plane
                                  : 2 * 3 * 2 * NRB * 64;    // 16-byte vectors per stage
  constexpr uint32_t kStageBytes = kStageVec * 16;
  static_assert(2 * kStageVec * 16 >= WAVES * G::kTileFloats * 4, "h' tiles fit the stage buffers");
  float* const ctile = reinterpret_cast<float*>(lds + 2 * kStageVec) + wave * G::kTileFloats;
  uint32_t* const otab = reinterpret_cast<uint32_t*>(
      reinterpret_cast<float*>(lds + 2 * kStageVec) + WAVES * G::kTileFloats) + wave * 192;
  constexpr uint32_t kNone = 0xffffffffu;
  const uint32_t rowb = (uint32_t)C * 4u;                    // bytes per cell of a state tensor
  bool okc[3];
  int cell[3];                                               // cell index inside its image
  const bool owned = valid && (!HALO || (col >= 1 && col <= 30));
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    okc[e] = owned & (y0 + e < H);
    cell[e] = (y0 + e) * W + xpos;
  }
  if (wave_live) {
    const int src_c0 = cone_bg_src ? a.rows - 1 : ((valid && a.src_row_c) ? a.src_row_c[r] : r);
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      otab[e * 32 + col] = okc[e] ? (uint32_t)(src_c0 * HW + cell[e]) * rowb : kNone;
      otab[96 + e * 32 + col] = okc[e] ? (uint32_t)(r * HW + cell[e]) * rowb : kNone;
    }
  }
  // ---- the wave's tile of the cell state c (96 cells x CH channels) starts its way into LDS
  // NOW, by LDS-DMA: pass k moves the tile's bytes [1024 k, 1024 k + 1024), lane l the 16 bytes
  // of tile row i / kPieces, piece i % kPieces, i = 64 k + l (a row = one cell's CH channels).
  const uint32_t colb = (uint32_t)(cb * CH) * 4u;            // the workgroup's first channel
  if (wave_live && !a.zero_state) {
    const __amdgpu_buffer_rsrc_t c_rs0 = __builtin_amdgcn_make_buffer_rsrc(
        uniform_ptr(const_cast<float*>(a.c)), 0, (uint32_t)(a.rows * HW) * rowb, 0x00020000);
#pragma unroll
    for (int k = 0; k < kPasses; ++k) {
      const int i = k * 64 + lane;
      const int trow = i / kPieces, piece = i - trow * kPieces;
      const uint32_t ro = trow < 96 ? otab[trow] : kNone;
      // rows that own no cell read offset 0 (the value is never used)
      const uint32_t off = ro != kNone ? ro + colb + (uint32_t)piece * 16u : 0u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          c_rs0, (__attribute__((address_space(3))) void*)(ctile + k * 256), 16, off, 0, 0,
          MV_EPI_LD_AUX);
    }
  }

  // ---- the 2-channel fp32 x chunk (regression encoder), direct form: row y0 into M0 (only
  // y(3t) holds M0), row y0 + 2 into M4 (only y(3t+2)); the middle row has no component of its
  // own: D / 2 into M1 and -D / 2 into M2 leave y(3t) and y(3t+2) alone (their M1 + M2 terms
  // cancel) and give y(3t+1) = M1 - M2 its D
  if (a.x_small && wave_live) {
    const int Cin = Cx + C, N4 = 4 * C;
    const int nk = 9 * Cx;
    const int n0 = (col >> 3) * C + cb * CH + (col & 7);
    for (int k2 = 0; 2 * k2 < nk; ++k2) {
      const int k = 2 * k2 + half;
      const bool kok = k < nk;
      const int tap = kok ? k / Cx : 0, chn = kok ? k - tap * Cx : 0;
      const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
      float wv[NRB];
#pragma unroll
      for (int rb = 0; rb < NRB; ++rb) {
        const float tw = p.w_hwio[((size_t)tap * Cin + chn) * N4 + n0 + rb * 8];
        wv[rb] = kok ? tw * (BF16D ? 1.0f : 65536.0f) : 0.f;     // bf16 mode: unscaled sums
      }
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        const int yy = y0 + e + dy, xx = xpos + dx;
        const bool ok = kok & valid & (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W);
        const int off = ok ? r * a.x_row_stride + (yy * W + xx) * Cx + chn : 0;
        const float tv = a.x[off];
        const float v = ok ? tv : 0.f;
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb) {
          if constexpr (BF16D) {
            acc[e][rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[rb], v, acc[e][rb], 0, 0, 0);
          } else if (e == 1) {
            acc[1][rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[rb], 0.5f * v, acc[1][rb], 0, 0, 0);
            acc[2][rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[rb], -0.5f * v, acc[2][rb], 0, 0, 0);
          } else {
            acc[e == 0 ? 0 : 4][rb] =
                __builtin_amdgcn_mfma_f32_32x32x2f32(wv[rb], v, acc[e == 0 ? 0 : 4][rb], 0, 0, 0);
          }
        }
      }
    }
  }

  // ---- f16 chunks of 16 input channels (x chunks first, then h chunks), five components each,
  // on PRE-TRANSFORMED operands.  The (chunk, component) pairs form ONE sequence g = 0 .. G - 1
  // (the pack is laid out in exactly that order); an LDS stage holds two consecutive
  // components (24 KB), double-buffered by LDS-DMA: 36 MFMAs per wave and barrier, like the
  // row-pair kernel.  The accumulator a component adds to must be known at compile time: five
  // stages walk through the pairs (0,1) (2,3) (4,0) (1,2) (3,4), a switch picks the pair.
  const int nxc = p.n_xc;
  const int ck_lo = a.sx_corr ? nxc : 0;                          // sparse x: table terms instead
  const int ck_hi = a.zero_state ? nxc : nxc + (C >> 4);
  if constexpr (BF16D) {
    // ---- direct 3 x 3 on ONE bf16 plane per operand.  A stage = a whole chunk of 16 input
    // channels: 9 taps x NRB row blocks of weights (18 KB), double-buffered by LDS-DMA; the
    // lane's five operand rows y0 - 1 .. y0 + 3 of the chunk (16 bytes each, from the ordinary
    // tiled planes, the beam's parent indirection in the row offsets) are requested a chunk
    // ahead.  Per stencil column dx: the five rows moved a lane (DPP) once, then for every
    // kernel row dy one weight fragment per row block feeds THREE MFMAs (output rows 3t + e
    // read operand row e + dy).
    if (ck_hi > ck_lo) {
      constexpr int kChunkVecD = 3 * 3 * NRB * 64;
      constexpr int kPiecesD = 3 * 3 * NRB;                  // 1 KB pieces of a stage
      const f16x8* wblk = reinterpret_cast<const f16x8*>(p.wpw) +
                          ((size_t)cb * (nxc + (C >> 4)) + ck_lo) * kChunkVecD;
      const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(
          uniform_ptr(const_cast<f16x8*>(wblk)), 0, 0x7fffffff, 0x00020000);
      const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
          uniform_ptr(const_cast<_Float16*>(q.x16 ? q.x16 - kPlanePad : q.h16 - kPlanePad)), 0,
          0x7fffffff, 0x00020000);
      const __amdgpu_buffer_rsrc_t hrs = __builtin_amdgcn_make_buffer_rsrc(
          uniform_ptr(const_cast<_Float16*>(q.h16 ? q.h16 - kPlanePad : q.x16 - kPlanePad)), 0,
          0x7fffffff, 0x00020000);
      const int wave_u = __builtin_amdgcn_readfirstlane(wave);
      const uint32_t lane16 = (uint32_t)lane * 16u;
      auto stage_dma = [&](int st, f16x8* dstbuf) {
#pragma unroll
        for (int i = 0; i < (kPiecesD + WAVES - 1) / WAVES; ++i) {
          const int piece = i * WAVES + wave_u;
          if (piece < kPiecesD)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(
                wrs, (__attribute__((address_space(3))) void*)(dstbuf + piece * 64), 16, lane16,
                (uint32_t)st * (uint32_t)(kChunkVecD * 16) + (uint32_t)piece * 1024u, 0,
                MV_DMA_AUX);
        }
      };
      struct Rows { f16x8 d[5]; };
      // chunk ck of the sequence (x chunks first); a request past the end repeats the last one
      auto rload = [&](int ck, Rows& rw) {
        const int cc = ck < ck_hi ? ck : ck_hi - 1;
        const bool is_x = cc < nxc;
        const uint32_t so = (uint32_t)(is_x ? cc : cc - nxc) * 1024u;   // channel group: 512 halves
#pragma unroll
        for (int i = 0; i < 5; ++i) {
          // an out-of-image row keeps offset 0 = the zero pad in front of the plane (the channel
          // group must not move it into the plane)
          const uint32_t ro = is_x ? roffx[i] : roffh[i];
          rw.d[i] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(
                                                  is_x ? xrs : hrs, (int)(ro ? ro + so : 0u), 0, 0));
        }
      };
      // (two row sets alternating without the copy below measured 3 % SLOWER: 0.368 vs 0.352 ms
      // per launch, same box -- hipcc's schedule of the unrolled pair is worse; requesting the
      // weight fragments of tap s + 1 before the MFMAs of tap s, pinned with sched_barrier:
      // 0.3436 / 0.3471 against 0.3441 / 0.3435 ms -- nothing: the second wave of the SIMD
      // already covers the fragment reads, profiles/r6q_*)
      Rows cur, nxt;
      rload(ck_lo, cur);
      nxt = cur;
      stage_dma(0, lds);
      __syncthreads();
      for (int ck = ck_lo; ck < ck_hi; ++ck) {
        const int st = ck - ck_lo;
        f16x8* const buf = lds + ((st & 1) ? kStageVec : 0);
        f16x8* const nbuf = lds + ((st & 1) ? 0 : kStageVec);
        if (ck + 1 < ck_hi) {
          stage_dma(st + 1, nbuf);       // its buffer was last read before the barrier
          rload(ck + 1, nxt);
        }
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          f16x8 sft[5];
#pragma unroll
          for (int i = 0; i < 5; ++i)
            sft[i] = dx == 1 ? cur.d[i]
                             : wn_lane_shift(cur.d[i], dx == 0, dx == 0 ? okx0 : okx2);
#pragma unroll
          for (int dy = 0; dy < 3; ++dy) {
            f16x8 w[NRB];
#pragma unroll
            for (int rb = 0; rb < NRB; ++rb) w[rb] = buf[((dy * 3 + dx) * NRB + rb) * 64 + lane];
#pragma unroll
            for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
              for (int e = 0; e < 3; ++e)
                acc[e][rb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                    __builtin_bit_cast(bf16x8, w[rb]), __builtin_bit_cast(bf16x8, sft[e + dy]),
                    acc[e][rb], 0, 0, 0);
          }
        }
        cur = nxt;
        __syncthreads();                 // DMA + rows of the next chunk have landed
      }
    }
  } else
  if (ck_hi > ck_lo) {
    static_assert(NRB == 2, "stage copy: 24 pieces of 64 vectors");
    const int G_total = (ck_hi - ck_lo) * 5;
    const int S_total = (G_total + 1) >> 1;
    const f16x8* wblk = reinterpret_cast<const f16x8*>(p.wpw) +
                        ((size_t)cb * (nxc + (C >> 4)) + ck_lo) * G::kChunkVec;
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(
        uniform_ptr(const_cast<f16x8*>(wblk)), 0, 0x7fffffff, 0x00020000);
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const uint32_t lane16 = (uint32_t)lane * 16u;
    // stage copy: the pack IS the LDS image; 24 pieces of 64 vectors (12 when the last stage
    // holds one component), 24 / WAVES per wave
    auto stage_dma = [&](int st, f16x8* dstbuf) {
      const int npiece = (2 * st + 1 < G_total) ? 24 : 12;
#pragma unroll
      for (int i = 0; i < 24 / WAVES; ++i) {
        const int piece = i * WAVES + wave_u;
        if (piece < npiece)
          __builtin_amdgcn_raw_ptr_buffer_load_lds(
              wrs, (__attribute__((address_space(3))) void*)(dstbuf + piece * 64), 16, lane16,
              (uint32_t)st * kStageBytes + (uint32_t)piece * 1024u, 0, MV_DMA_AUX);
      }
    };
    // B fragments: the centre fragment of (component, plane) is one 16-byte load per lane (the
    // wave's 64 lanes = one contiguous KB of the pre-pass's output: lane l IS k half l >> 5,
    // column l & 31); a dead wave -- past the last triple-cell -- reads tile 0
    const int KGx = Cx >> 4, KGh = C >> 4;
    // (HALO: the wave's 32 triple-cells start anywhere: one offset per lane; a lane past either
    // end of the sequence reads beyond the buffer = zeros)
    const int tile = __builtin_amdgcn_readfirstlane((wave_live && !HALO) ? (q_wave >> 5) : 0);
    const size_t ntile_b = (size_t)((Q_total + 31) >> 5) * 10240u;          // bytes per channel group
    const __amdgpu_buffer_rsrc_t vxrs = __builtin_amdgcn_make_buffer_rsrc(
        uniform_ptr(const_cast<char*>(reinterpret_cast<const char*>(p.v3x ? p.v3x : p.v3h) +
                                      (p.v3x ? (size_t)tile * (size_t)KGx * 10240u : 0))),
        0, (uint32_t)(HALO ? ntile_b * (size_t)(KGx > 0 ? KGx : 1) : (size_t)(KGx > 0 ? KGx : 1) * 10240u),
        0x00020000);
    const __amdgpu_buffer_rsrc_t vhrs = __builtin_amdgcn_make_buffer_rsrc(
        uniform_ptr(const_cast<char*>(reinterpret_cast<const char*>(p.v3h ? p.v3h : p.v3x) +
                                      (p.v3h ? (size_t)tile * (size_t)KGh * 10240u : 0))),
        0, (uint32_t)(HALO ? ntile_b * (size_t)KGh : (size_t)KGh * 10240u), 0x00020000);
    uint32_t vo_x = lane16, vo_h = lane16;
    if (HALO) {
      const int qq = q_wave + col;
      const uint32_t in_tile = (uint32_t)((qq & 31) + 32 * half) * 16u;
      vo_x = valid ? (uint32_t)(qq >> 5) * (uint32_t)KGx * 10240u + in_tile : 0x80000000u;
      vo_h = valid ? (uint32_t)(qq >> 5) * (uint32_t)KGh * 10240u + in_tile : 0x80000000u;
    }
    struct Vc { f16x8 h, l; };
    // component g of the sequence (clamped to the last one: a request past the end fetches
    // that component again)
    auto vload = [&](int g, Vc& v) {
      const int gc = g < G_total ? g : G_total - 1;
      const int ck = ck_lo + gc / 5, comp = gc - (gc / 5) * 5;
      const bool is_x = ck < nxc;
      const int so = (is_x ? ck : ck - nxc) * 10240 + comp * 2048;
      v.h = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(
                                          is_x ? vxrs : vhrs, (int)(is_x ? vo_x : vo_h), so, 0));
      v.l = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(
                                          is_x ? vxrs : vhrs, (int)(is_x ? vo_x : vo_h), so + 1024, 0));
    };
    // one component: 3 dx x NRB row blocks x 3 MFMAs from stage buffer `buf`, slot ci
#define MV_W3_COMP(COMP, CI, VHI, VLO, BUF)                                                   \
  do {                                                                                        \
    _Pragma("unroll") for (int dx = 0; dx < 3; ++dx) {                                        \
      const bool sh_ = dx != 1;                                                               \
      const f16x8 b0 = !sh_ ? (VHI) : wn_lane_shift((VHI), dx == 0, dx == 0 ? okx0 : okx2);   \
      const f16x8 b1 = !sh_ ? (VLO) : wn_lane_shift((VLO), dx == 0, dx == 0 ? okx0 : okx2);   \
      f16x8 w0[NRB], w1[NRB];                                                                 \
      _Pragma("unroll") for (int rb = 0; rb < NRB; ++rb) {                                    \
        w0[rb] = (BUF)[((((CI) * 3 + dx) * 2 + 0) * NRB + rb) * 64 + lane];                   \
        w1[rb] = (BUF)[((((CI) * 3 + dx) * 2 + 1) * NRB + rb) * 64 + lane];                   \
      }                                                                                       \
      _Pragma("unroll") for (int rb = 0; rb < NRB; ++rb)                                      \
        acc[COMP][rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w1[rb], b0, acc[COMP][rb], 0, 0, 0); \
      _Pragma("unroll") for (int rb = 0; rb < NRB; ++rb)                                      \
        acc[COMP][rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w0[rb], b1, acc[COMP][rb], 0, 0, 0); \
      _Pragma("unroll") for (int rb = 0; rb < NRB; ++rb)                                      \
        acc[COMP][rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w0[rb], b0, acc[COMP][rb], 0, 0, 0); \
    }                                                                                         \
  } while (0)
    // one stage: components CA (slot 0) and CB (slot 1; CB < 0: the sequence's last, single
    // component); the next stage's weights and fragments are requested first
#define MV_W3_STAGE(CA, CB)                                                                   \
  do {                                                                                        \
    f16x8* const buf = lds + ((st & 1) ? kStageVec : 0);                                      \
    f16x8* const nbuf = lds + ((st & 1) ? 0 : kStageVec);                                     \
    if (st + 1 < S_total) {                                                                   \
      stage_dma(st + 1, nbuf);          /* its buffer was last read before the barrier */     \
      vload(2 * st + 2, na); vload(2 * st + 3, nb);      /* a whole stage ahead */            \
    }                                                                                         \
    MV_W3_COMP(CA, 0, va.h, va.l, buf);                                                       \
    if ((CB) >= 0) MV_W3_COMP((CB) < 0 ? 0 : (CB), 1, vb.h, vb.l, buf);                       \
    va = na; vb = nb;                                                                         \
    ++st;                                                                                     \
    __syncthreads();     /* DMA + fragments of the next stage have landed */                  \
  } while (0)

    Vc va, vb, na, nb;
    vload(0, va); vload(1, vb);
    na = va; nb = vb;
    stage_dma(0, lds);
    __syncthreads();                         // carries the vmcnt(0) of the pending LDS-DMA
    // five stages = ten components = two chunks: (0,1) (2,3) (4,0) (1,2) (3,4); an odd chunk
    // count ends on (0,1) (2,3) (4)
    const int nck = ck_hi - ck_lo;
    int st = 0;
    for (int pr = 0; pr < (nck >> 1); ++pr) {
      MV_W3_STAGE(0, 1); MV_W3_STAGE(2, 3); MV_W3_STAGE(4, 0); MV_W3_STAGE(1, 2); MV_W3_STAGE(3, 4);
    }
    if (nck & 1) {
      MV_W3_STAGE(0, 1); MV_W3_STAGE(2, 3); MV_W3_STAGE(4, -1);
    }
#undef MV_W3_COMP
#undef MV_W3_STAGE
  }
  if (!wave_live) return;

  // ---------------------------------------------------------------- epilogue
  // registers of acc[c][rb]: gate = reg >> 2, channel = cb * CH + rb * 8 + 4 * half + (reg & 3);
  // the lane's triple-cell gives rows y0 + e, e = 0, 1, 2.
  int lane_e = lane;
  asm volatile("" : "+v"(lane_e));          // keep the address arithmetic below the loop
  const int half_e = lane_e >> 5;
  const int ch0 = cb * CH + 4 * half_e;                      // + rb * 8
  const uint32_t out_bytes = (uint32_t)(a.rows * HW) * rowb;
  const __amdgpu_buffer_rsrc_t co_rs = __builtin_amdgcn_make_buffer_rsrc(
      uniform_ptr(a.c_out), 0, out_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t ho_rs = __builtin_amdgcn_make_buffer_rsrc(
      uniform_ptr(a.h_out), 0, out_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t go_rs = __builtin_amdgcn_make_buffer_rsrc(
      uniform_ptr(a.gates_out ? a.gates_out : a.h_out), 0, a.gates_out ? 4u * out_bytes : 0u,
      0x00020000);
  // ---- state I/O through LDS.  A lane owns 4 channels per row block of the three cells of its
  // triple-cell: stored from the accumulator layout every lane of a wave instruction would
  // touch its own cache line.  Instead the wave's tile of a state tensor -- 96 cells x CH
  // channels fp32, row e * 32 + column -- passes through a wave-private LDS tile and moves to /
  // from memory LINEARLY: pass k, lane l = 16 bytes at tile byte 1024 k + 16 l, i.e. kPieces
  // lanes cover the contiguous bytes the workgroup's CH channels have in a cell.
  float* const tl0 = ctile;                   // c in, then c' out
  float* const tl1 = reinterpret_cast<float*>(lds) + wave * G::kTileFloats;   // h' out (dead chunk buffer)
  const int wr_idx = (lane_e & 31) * CH + half_e * 4;        // + e * 32 * CH + rb * 8 (floats)
  f32x4 cprev[3][NRB];
#pragma unroll
  for (int e = 0; e < 3; ++e)
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb) cprev[e][rb] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (!a.zero_state) {
    // the tile was requested before the main loop; its barriers carried the vmcnt(0) -- the
    // explicit wait covers a launch without f16 chunks
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int e = 0; e < 3; ++e)
#pragma unroll
      for (int rb = 0; rb < NRB; ++rb)
        cprev[e][rb] = *reinterpret_cast<const f32x4*>(tl0 + wr_idx + e * 32 * CH + rb * 8);
  }
  // sparse x: hot cell of the lane's image
  int hot_y = 0, hot_x = 0;
  // (light cone: the background row has no hot cell -- row 0's stands in, its terms are dropped)
  const bool bg_row = kCone && a.cone_on && r == a.rows - 1;
  if (a.sx_corr) {
    const int hr = bg_row ? 0 : (a.sx_hot_div > 1 ? r / a.sx_hot_div : r);
    const uint32_t hyx = a.sx_cellyx[a.sx_hot[(size_t)hr * a.sx_hot_stride]];
    hot_y = (int)(hyx >> 16); hot_x = (int)(hyx & 0xffffu);
  }
  const float un = BF16D ? 1.0f : kF16Unscale;
  const bool planes = q.h16_out != nullptr;
  u32x2 ph[3][NRB], pl[3][NRB];               // h' as plane halves (hi, lo), [e][rb]
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    const int y = y0 + e;
    const uint32_t mcell = (uint32_t)(r * HW + cell[e]);     // output cell, flat
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb) {
      const int ch = ch0 + rb * 8;
      // per-gate additive terms (4 channels each)
      f32x4 add[4];
      {
        const float* bsrc = a.bias;
        if (a.sx_corr && a.sx_bias) {
          const int cls = 3 * (y == 0 ? 0 : (y == H - 1 ? 2 : 1)) +
                          (xpos == 0 ? 0 : (xpos == W - 1 ? 2 : 1));
          bsrc = a.sx_bias + (size_t)(okc[e] ? cls : 4) * 4 * C;
        }
#pragma unroll
        for (int g = 0; g < 4; ++g)
          add[g] = *reinterpret_cast<const f32x4*>(bsrc + g * C + ch);
        if (a.sx_corr) {
          // UNCONDITIONAL loads (a branch around them would serialise one L2 round trip per
          // row and row block behind the bias row's): a cell outside the radius reads the
          // clamped table row and drops it
          const int dy = y - hot_y, dxh = xpos - hot_x, rad = a.sx_rad;
          const bool inr = okc[e] && !bg_row && dy >= -rad && dy <= rad && dxh >= -rad && dxh <= rad;
          const int dyc = dy < -rad ? -rad : (dy > rad ? rad : dy);
          const int dxc = dxh < -rad ? -rad : (dxh > rad ? rad : dxh);
          const int side = 2 * rad + 1;
          const int idx = a.sx_by_class
                              ? 3 * (hot_y == 0 ? 0 : (hot_y == H - 1 ? 2 : 1)) +
                                    (hot_x == 0 ? 0 : (hot_x == W - 1 ? 2 : 1))
                              : ((valid && !bg_row) ? r : 0);
          const float* ct = a.sx_corr +
              ((size_t)idx * side * side + (dyc + rad) * side + (dxc + rad)) * 4 * C + ch;
          const float keep = inr ? 1.0f : 0.0f;
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const f32x4 cv = *reinterpret_cast<const f32x4*>(ct + g * C);
            add[g][0] = __builtin_fmaf(cv[0], keep, add[g][0]);
            add[g][1] = __builtin_fmaf(cv[1], keep, add[g][1]);
            add[g][2] = __builtin_fmaf(cv[2], keep, add[g][2]);
            add[g][3] = __builtin_fmaf(cv[3], keep, add[g][3]);
          }
        }
      }
      f32x4 cn4, hn4, si4, tj4, sf4, so4;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float pre[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int reg = g * 4 + j;
          float yv;
          if constexpr (BF16D) {
            yv = acc[e][rb][reg];
          } else {
            const float m0 = acc[0][rb][reg], m1 = acc[1][rb][reg], m2 = acc[2][rb][reg],
                        m3 = acc[3][rb][reg], m4 = acc[kAcc - 1][rb][reg];
            if (e == 0) yv = (m0 + m1) + (m2 + m3);
            else if (e == 1) yv = (m1 - m2) + 2.0f * m3;
            else yv = (m1 + m2) + (4.0f * m3 + m4);
          }
          pre[g] = __builtin_fmaf(yv, un, add[g][j]);   // un = 2^-16: the product is exact
        }
        const float si = sigm_(pre[0]), tj = tanh_(pre[1]), sf = sigm_(pre[2] + a.forget_bias),
                    so = sigm_(pre[3]);
        float cn = sf * cprev[e][rb][j];
        cn = cn + si * tj;
        const float hn = tanh_(cn) * so;
        cn4[j] = cn; hn4[j] = hn; si4[j] = si; tj4[j] = tj; sf4[j] = sf; so4[j] = so;
      }
      // c' and h' into the wave's two LDS tiles (the c tile was read into cprev above)
      *reinterpret_cast<f32x4*>(tl0 + wr_idx + e * 32 * CH + rb * 8) = cn4;
      if (!a.skip_h32) *reinterpret_cast<f32x4*>(tl1 + wr_idx + e * 32 * CH + rb * 8) = hn4;
      if (a.gates_out && okc[e]) {
        // training forward: the four gate activations [m][4][C] (stored from the lane)
        const uint32_t g0 = (mcell * 4u * (uint32_t)C + (uint32_t)ch) * 4u;
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, si4), go_rs, (int)g0,
                                               0, MV_EPI_ST_AUX);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, tj4), go_rs,
                                               (int)(g0 + rowb), 0, MV_EPI_ST_AUX);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, sf4), go_rs,
                                               (int)(g0 + 2 * rowb), 0, MV_EPI_ST_AUX);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, so4), go_rs,
                                               (int)(g0 + 3 * rowb), 0, MV_EPI_ST_AUX);
      }
      if (planes) {
        f16x4 p0, p1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if constexpr (BF16D) {         // ONE unscaled bf16 plane
            p0[j] = bf16_as_half(hn4[j]);
            p1[j] = p0[j];
          } else {
            const float sc = hn4[j] * kF16Scale;
            const _Float16 h0 = (_Float16)sc;
            p0[j] = h0;
            p1[j] = (_Float16)(sc - (float)h0);
          }
        }
        ph[e][rb] = __builtin_bit_cast(u32x2, p0);
        pl[e][rb] = __builtin_bit_cast(u32x2, p1);
      }
    }
  }
  // ---- c' / h' out: the tiles leave LDS linearly, kPieces lanes per cell
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  {
#pragma unroll
    for (int k = 0; k < kPasses; ++k) {
      const int i = k * 64 + lane_e;
      const int trow = i / kPieces, piece = i - trow * kPieces;
      if (96 * kPieces % 64 == 0 || trow < 96) {
        const uint32_t ro = otab[96 + trow];
        const u32x4 cv = *reinterpret_cast<const u32x4*>(tl0 + i * 4);
        u32x4 hv = cv;
        if (!a.skip_h32) hv = *reinterpret_cast<const u32x4*>(tl1 + i * 4);
        if (ro != kNone) {
          const int off = (int)(ro + colb + (uint32_t)piece * 16u);
          __builtin_amdgcn_raw_buffer_store_b128(cv, co_rs, off, 0, MV_EPI_ST_AUX);
          if (!a.skip_h32) __builtin_amdgcn_raw_buffer_store_b128(hv, ho_rs, off, 0, MV_EPI_ST_AUX);
        }
      }
    }
  }
  // ---- operand planes of h' for the next gate convolution: tile (m >> 5, channel group of
  // 16), k half, 8 channels = one 16-byte vector per cell.  A lane holds 4 of the 8 for each
  // of its three cells; v_permlane32_swap hands the lower half-wave the complete vectors of
  // the e = 0 cells and the upper half-wave those of the e = 1 cells, a second swap the lower
  // half-wave those of the e = 2 cells: 16 bytes per lane, 512 contiguous bytes per half-wave.
  if (planes) {
    const uint32_t mc01 = (uint32_t)(r * HW + (half_e ? cell[1] : cell[0]));
    const uint32_t mc2 = (uint32_t)(r * HW + cell[2]);
    const bool ok01 = half_e ? okc[1] : okc[0];
    const bool ok2 = okc[2] && half_e == 0;
    const size_t KG = (size_t)(C >> 4);
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb) {
      const int c8 = cb * NRB + rb;                          // the vector's 8-channel group
      const size_t grp = (size_t)(c8 >> 1) * 512 + (size_t)(c8 & 1) * 256;
      const size_t o01 = (size_t)(mc01 >> 5) * KG * 512 + grp + (size_t)((int)(mc01 & 31u) * 8);
      const size_t o2 = (size_t)(mc2 >> 5) * KG * 512 + grp + (size_t)((int)(mc2 & 31u) * 8);
#pragma unroll
      for (int pn = 0; pn < (BF16D ? 1 : 2); ++pn) {
        const u32x2 A = pn ? pl[0][rb] : ph[0][rb], B = pn ? pl[1][rb] : ph[1][rb];
        const u32x2 D = pn ? pl[2][rb] : ph[2][rb];
        const u32x2 s0 = __builtin_amdgcn_permlane32_swap(A[0], B[0], false, false);
        const u32x2 s1 = __builtin_amdgcn_permlane32_swap(A[1], B[1], false, false);
        // lower lanes: (own A | partner's A) = e 0, channels 0-3 | 4-7; upper lanes:
        // (partner's B | own B) = e 1, channels 0-3 | 4-7
        const u32x4 v = {s0[0], s1[0], s0[1], s1[1]};
        if (ok01)
          *reinterpret_cast<u32x4*>(q.h16_out + (size_t)pn * q.h16_out_stride + o01) = v;
        const u32x2 t0 = __builtin_amdgcn_permlane32_swap(D[0], D[0], false, false);
        const u32x2 t1 = __builtin_amdgcn_permlane32_swap(D[1], D[1], false, false);
        const u32x4 v2 = {t0[0], t1[0], t0[1], t1[1]};        // lower lanes: e 2, channels 0-3 | 4-7
        if (ok2)
          *reinterpret_cast<u32x4*>(q.h16_out + (size_t)pn * q.h16_out_stride + o2) = v2;
      }
    }
  }
}

template <int WAVES, int NRB, bool HALO, bool BF16D = false>
__global__ __launch_bounds__(WAVES * 64, 2)
void convlstm_step_wino3_kernel(const ConvLstmWinoGroup g) {
  extern __shared__ __attribute__((aligned(16))) f16x8 lds[];
  int block = blockIdx.x;
  int pi = 0;
#pragma unroll
  for (int i = 0; i < kMaxGroup - 1; ++i)
    if (i + 1 < g.n && (int)blockIdx.x >= g.block_end[i]) pi = i + 1;
  if (pi > 0) block -= g.block_end[pi - 1];
  // block -> (column block, row tile), as in convlstm_step_wino_kernel: XCD x holds the
  // ADJACENT column blocks 2x, 2x + 1 of sixteen (the two halves of every 128-byte line of the
  // state tensors at CH = 16) through one L2
  // map_mode 2 / 3 (MV_WINO_MAP, ncb = 16): an XCD holds FOUR / EIGHT column blocks and every
  // second / fourth row tile -- the pre-transformed operands of a row tile are then fetched by 4 /
  // 2 of the 8 L2s instead of all of them, at 2 / 4 times the weight working set per L2
  auto cbmap = [&](int ncb, int& cb, int& mt) {
    if ((g.map_mode == 2 || g.map_mode == 3) && ncb == 16) {
      const int per = g.map_mode == 2 ? 4 : 8;                 // column blocks per XCD
      const int nt = per / 2;                                  // row tiles per block group
      const int grp = block / (16 * nt), w = block - grp * (16 * nt);
      const int xcd = w & 7, j = w >> 3;                       // j: 0 .. per - 1
      cb = per * (xcd % (16 / per)) + j;
      mt = grp * nt + xcd / (16 / per);
    } else if (g.map_mode >= 1 && (ncb & 15) == 0) {
      const int grp = block / 16, w16 = block - grp * 16;      // 16 consecutive blocks
      cb = (grp % (ncb / 16)) * 16 + 2 * (w16 & 7) + (w16 >> 3);
      mt = grp / (ncb / 16);
    } else {
      cb = block % ncb; mt = block / ncb;
    }
  };
  int cb, mt;
  constexpr int CH = Wn3<NRB>::kCh;
  switch (pi) {
    case 0: cbmap(g.p[0].b.f.C / CH, cb, mt); convlstm_wino3_body<WAVES, NRB, HALO, BF16D>(g.p[0], cb, mt, lds); break;
    case 1: cbmap(g.p[1].b.f.C / CH, cb, mt); convlstm_wino3_body<WAVES, NRB, HALO, BF16D>(g.p[1], cb, mt, lds); break;
    case 2: cbmap(g.p[2].b.f.C / CH, cb, mt); convlstm_wino3_body<WAVES, NRB, HALO, BF16D>(g.p[2], cb, mt, lds); break;
    default: cbmap(g.p[3].b.f.C / CH, cb, mt); convlstm_wino3_body<WAVES, NRB, HALO, BF16D>(g.p[3], cb, mt, lds); break;
  }
}

constexpr int kW3Waves = 4, kW3Nrb = 2;     // two 4-wave workgroups per CU

static inline size_t wino3_lds_bytes() {      // 73.5 KB: two workgroups per CU
  return (size_t)2 * (2 * 3 * 2 * kW3Nrb * 64 * 16) + (size_t)kW3Waves * Wn3<kW3Nrb>::kTileFloats * 4 +
         (size_t)kW3Waves * 192 * 4;
}
static inline unsigned convlstm_wino3_blocks(const ConvLstmArgs& a, bool halo, int map_mode = 1) {
  const size_t Q = (size_t)a.rows * ((a.H + 2) / 3) * a.W;
  const size_t triples = (size_t)kW3Waves * (halo ? 30 : 32);
  size_t mtiles = (Q + triples - 1) / triples;
  const unsigned ncb = (unsigned)(a.C / Wn3<kW3Nrb>::kCh);
  if ((map_mode == 2 || map_mode == 3) && ncb == 16) {       // whole block groups (dead tiles idle)
    const size_t nt = map_mode == 2 ? 2 : 4;
    mtiles = (mtiles + nt - 1) / nt * nt;
  }
  return (unsigned)mtiles * ncb;
}

// The F(3,3) form serves a problem when C is a multiple of the channel block, the x operand
// comes as 16-channel planes (or is the 2-channel fp32 chunk) under the FIXED 2^8 scale -- the
// per-tensor exponent of unbounded activations leaves one bit of headroom, the components here
// need three (|V| <= 6 max |d|) -- and the grid has at least three rows.  Any width: one that
// does not divide 32 takes the HALO tiling (30 of 32 lanes owned).
static inline bool wino3_geometry_ok(const ConvLstmArgs& a, const ConvLstm16Args& q) {
  return a.W > 0 && a.C % Wn3<kW3Nrb>::kCh == 0 && (a.Cx % 16 == 0 || a.x_small) && a.H >= 3 &&
         q.x_exp == nullptr;
}
static inline bool wino3_needs_halo(const ConvLstmArgs& a) { return 32 % a.W != 0; }
// The HALO tiling addresses the pre-transformed operands with ONE 32-bit byte offset per lane
// from the buffer's start (a wave's 32 triple-cells start anywhere) and sends the lanes outside
// the sequence to offset 2^31, which must lie BEYOND the buffer: a launch in the halo tiling must
// not hold a problem whose x or h operand has 2 GiB or more (36 x 18 grid, 128 rows x 20 beams,
// 256 channels: 2.8 GB).  The exact tiling rebases its descriptor per wave tile: no such limit.
// The tiling is ONE per launch, so the bound concerns every problem of a halo group, whatever
// its own width (gate_plan.h decides).
static inline bool wino3_halo_addressable(const ConvLstmArgs& a) {
  const size_t lim = (size_t)1 << 31;
  const int cx16 = a.x_small ? 0 : (a.Cx + 15) / 16 * 16;
  return wino3_v_elems(a.rows, a.H, a.W, a.C) * 2 < lim &&
         (cx16 == 0 || wino3_v_elems(a.rows, a.H, a.W, cx16) * 2 < lim);
}

static inline void wino3_init_attributes() {
  static const bool done = [] {
    (void)hipFuncSetAttribute(
        reinterpret_cast<const void*>(convlstm_step_wino3_kernel<kW3Waves, kW3Nrb, false>),
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)wino3_lds_bytes());
    (void)hipFuncSetAttribute(
        reinterpret_cast<const void*>(convlstm_step_wino3_kernel<kW3Waves, kW3Nrb, true>),
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)wino3_lds_bytes());
    return true;
  }();
  (void)done;
}

// ------------------------------------------------------------------ bf16 mode on this tile
// (compute mode 2; body: BF16D).  Pack: [cb][chunk][dy 3][dx 3][rb][lane 64][8] bf16 of the
// kernel itself -- a chunk IS the LDS image of its stage; element e of lane l: A-operand row
// l & 31 = gate (row >> 3), channel cb * 8 nrb + rb * 8 + (row & 7); k = 8 (l >> 5) + e.
static inline size_t bf16t_wpack_elems(int Cx16, int C, int nrb) {   // in halves
  return (size_t)(C / (8 * nrb)) * (size_t)(Cx16 / 16 + C / 16) * 9 * nrb * 64 * 8;
}
__global__ void pack_bf16t_kernel(const float* __restrict__ w, _Float16* __restrict__ out,
                                  int Cx_total, int Cx16, int C, int nrb, size_t total) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int e = idx & 7;
  const int l = (idx >> 3) & 63;
  size_t t = idx >> 9;
  const int rb = (int)(t % nrb); t /= nrb;
  const int tap = (int)(t % 9); t /= 9;                 // dy * 3 + dx
  const int nxc = Cx16 / 16, nch = nxc + C / 16;
  const int chunk = (int)(t % nch), cb = (int)(t / nch);
  const bool is_x = chunk < nxc;
  const int cg = is_x ? chunk : chunk - nxc;
  const int k = 8 * (l >> 5) + e;
  const int cin = (is_x ? 0 : Cx_total) + cg * 16 + k;
  const int row = l & 31;
  const int n = (row >> 3) * C + cb * 8 * nrb + rb * 8 + (row & 7);
  const int Cin = Cx_total + C, N4 = 4 * C;
  out[idx] = bf16_as_half(w[((size_t)tap * Cin + cin) * N4 + n]);
}
static inline size_t bf16t_lds_bytes() {
  return (size_t)2 * (3 * 3 * kW3Nrb * 64 * 16) + (size_t)kW3Waves * Wn3<kW3Nrb>::kTileFloats * 4 +
         (size_t)kW3Waves * 192 * 4;
}
static inline bool bf16t_geometry_ok(const ConvLstmArgs& a, const ConvLstm16Args& q) {
  return a.W > 0 && a.C % Wn3<kW3Nrb>::kCh == 0 && (a.Cx % 16 == 0 || a.x_small) && a.H >= 3 &&
         q.x_exp == nullptr;
}
// One launcher for both kernels of the row-triple tile: F(3,3) on the f16x3 split and, with
// BF16D, the direct bf16 form.  The caller's plan (gate_plan.h) has chosen the tiling -- ONE per
// launch: halo if any problem needs it -- and the block map.  (The F(3,3) attributes are also set
// when the weights are packed, i.e. outside any graph capture.)
template <bool HALO, bool BF16D>
static inline void tile3_launch_one(const ConvLstmWinoGroup& g, unsigned total, hipStream_t stream) {
  const size_t lds = BF16D ? bf16t_lds_bytes() : wino3_lds_bytes();
  if constexpr (BF16D) {
    static const bool attr = [lds] {
      (void)hipFuncSetAttribute(
          reinterpret_cast<const void*>(convlstm_step_wino3_kernel<kW3Waves, kW3Nrb, HALO, true>),
          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      return true;
    }();
    (void)attr;
  } else {
    wino3_init_attributes();
  }
  hipLaunchKernelGGL((convlstm_step_wino3_kernel<kW3Waves, kW3Nrb, HALO, BF16D>), dim3(total),
                     dim3(kW3Waves * 64), lds, stream, g);
}
template <bool BF16D>
static inline void launch_convlstm_tile3_steps(const ConvLstmWinoArgs* probs, int n, bool halo,
                                               int map_mode, hipStream_t stream) {
  ConvLstmWinoGroup g{};
  g.n = n;
  g.map_mode = map_mode;
  unsigned total = 0;
  for (int i = 0; i < n; ++i) {
    g.p[i] = probs[i];
    total += convlstm_wino3_blocks(probs[i].b.f, halo, map_mode);
    g.block_end[i] = (int32_t)total;
  }
  for (int i = n; i < kMaxGroup; ++i) g.block_end[i] = (int32_t)total;
  if (halo) tile3_launch_one<true, BF16D>(g, total, stream);
  else tile3_launch_one<false, BF16D>(g, total, stream);
}
static inline void launch_convlstm_wino3_steps(const ConvLstmWinoArgs* probs, int n, bool halo,
                                               int map_mode, hipStream_t stream) {
  launch_convlstm_tile3_steps<false>(probs, n, halo, map_mode, stream);
}
static inline void launch_convlstm_bf16t_steps(const ConvLstmWinoArgs* probs, int n, bool halo,
                                               int map_mode, hipStream_t stream) {
  launch_convlstm_tile3_steps<true>(probs, n, halo, map_mode, stream);
}

}  // namespace mv
