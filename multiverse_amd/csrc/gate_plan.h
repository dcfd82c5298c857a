// which kernel form a gate-convolution launch takes, and how big what it needs is -- part of the
// ONE translation unit engine.hip (included from there, in order; not a stand-alone header).
//
// Nothing here launches or allocates: these functions answer questions.  The callers
// (engine_setup.h packs, engine_forward.h / engine_train.h launches, engine_ops.h forced variants,
// mv_set_compute_mode and train_alloc for the scratch sizes) ask instead of restating the rules.
#pragma once

namespace {

// ------------------------------------------------------------------ the A/B switches
// Every environment switch that takes part in choosing or shaping a gate launch, read once per
// process (DESIGN.md carries the table).  The decode step's and the chain streams' switches:
// step_plan.h.
struct GateKnobs {
  bool wino, wino3, bf16t, wino_dgrad;      // MV_WINO, MV_WINO3, MV_BF16T, MV_WINO_DGRAD (=0: off)
  // MV_WINO_MAP, block -> column block map; each kernel has its own measured default
  int wino_map_f23;     // 1: the two halves of a 128-byte state line on one XCD
  int wino_map_f33;     // 2: an XCD holds four column blocks and every second row tile (+0.7 %
                        //    greedy and beam-20 against 1, same box; 3 = eight: no better)
  int wino_map_bf16t;   // 2
  bool conv_shift;      // MV_CONV_SHIFT=0: never the DPP column-shift form of the 32-cell bodies
  int conv_map;         // MV_CONV_MAP=1: row tile per XCD (convlstm_f16x3.h step_block_map)
  bool epi_planes;      // MV_EPI_PLANES=0: separate split pass over the fp32 h'
  int dgrad_kslices;    // MV_DGRAD_KSLICES (0 = unset: 4, bf16 1)
  bool transpose3;      // MV_TRANSPOSE3=0: three transposes instead of the fused one
  bool bf16_bwd;        // MV_BF16_BWD=0: the bf16 mode's backward stays on the f16x3 split
  bool bf16_fused_split;  // MV_BF16_FUSED_SPLIT=0: G's bf16 plane from a separate pass
  bool wgrad_splits_set; int wgrad_splits;   // MV_WGRAD_SPLITS
  bool wgrad_wide;      // MV_WGRAD_WIDE=0
  int wgrad_wide_map;   // MV_WGRAD_WIDE_MAP
  int wgrad_wide_splits;  // MV_WGRAD_WIDE_SPLITS (0 = unset)
  bool wgrad_wide_x;    // MV_WGRAD_WIDE_X=1: the x rows on the wide tile too
  bool wgrad_wino, wgrad_wino_bf16;   // MV_WGRAD_WINO, MV_WGRAD_WINO_BF16 (=0: off)
  int wgrad_x_splits;   // MV_WGRAD_X_SPLITS (12)
  int enc_cone;         // MV_ENC_CONE: 0 the class encoder computes every tile of every row; 1 (default)
                        // light cone from kEncConeMinBatch rows on; 2 at any batch size
};

// (the two readers, shared with step_plan.h's switches)
inline int env_num(const char* name, int unset) {
  const char* v = getenv(name);
  return v ? atoi(v) : unset;
}
inline bool env_on(const char* name) { return env_num(name, 1) != 0; }     // off only by NAME=0

inline const GateKnobs& gate_knobs() {
  static const GateKnobs k = [] {
    const auto num = env_num;
    const auto on = env_on;
    GateKnobs g{};
    g.wino = on("MV_WINO"); g.wino3 = on("MV_WINO3"); g.bf16t = on("MV_BF16T");
    g.wino_dgrad = on("MV_WINO_DGRAD");
    g.wino_map_f23 = num("MV_WINO_MAP", 1);
    g.wino_map_f33 = num("MV_WINO_MAP", 2);
    g.wino_map_bf16t = num("MV_WINO_MAP", 2);
    g.conv_shift = on("MV_CONV_SHIFT");
    g.conv_map = num("MV_CONV_MAP", 0);
    g.epi_planes = on("MV_EPI_PLANES");
    g.dgrad_kslices = num("MV_DGRAD_KSLICES", 0);
    g.transpose3 = on("MV_TRANSPOSE3");
    g.bf16_bwd = on("MV_BF16_BWD");
    g.bf16_fused_split = on("MV_BF16_FUSED_SPLIT");
    g.wgrad_splits_set = getenv("MV_WGRAD_SPLITS") != nullptr;
    g.wgrad_splits = num("MV_WGRAD_SPLITS", 0);
    g.wgrad_wide = on("MV_WGRAD_WIDE");
    g.wgrad_wide_map = num("MV_WGRAD_WIDE_MAP", 0);
    g.wgrad_wide_splits = num("MV_WGRAD_WIDE_SPLITS", 0);
    g.wgrad_wide_x = num("MV_WGRAD_WIDE_X", 0) == 1;
    g.wgrad_wino = on("MV_WGRAD_WINO"); g.wgrad_wino_bf16 = on("MV_WGRAD_WINO_BF16");
    g.wgrad_x_splits = num("MV_WGRAD_X_SPLITS", 12);
    g.enc_cone = num("MV_ENC_CONE", 1);
    return g;
  }();
  return k;
}

// ------------------------------------------------------------------ the x operand
// An x operand of up to three channels (the regression encoder's 2) is ONE fp32 chunk of the
// gate GEMM instead of fp16 / bf16 planes; the packs then carry no x part.
inline bool x_is_small(int Cx) { return Cx > 0 && 9 * Cx <= mv::kBK; }
inline int x_chunk16(int Cx) { return x_is_small(Cx) ? 0 : Cx; }
// x passes of the bf16 mode's k-steps and weight pack: an f16x3 split of the x part alone for
// models with unbounded activations (convlstm_f16x3.h xpasses)
inline int bf16_x_passes(int mode, bool dyn_x, bool x_small) {
  return (mode == 2 && dyn_x && !x_small) ? 3 : 1;
}

// ------------------------------------------------------------------ weight packs of a cell
struct CellPacks {
  bool wp16, wpw, wpw3;       // f16x3: direct planes, Winograd F(2,3), F(3,3)
  bool wpb, wpbt;             // bf16: the 32-cell body's plane, the row-triple tile's
  bool wd16, wdw, wdb;        // dgrad (training): f16x3 planes, their F(2,3) form, one bf16 plane
};
// What a cell of `Cx` input and `C` hidden channels carries in a compute mode.  The Winograd
// forms and the row-triple tile want C in whole channel blocks and x as 16-channel planes (or the
// small chunk); the Winograd forms also a kernel without outlier weights (ConvCell::
// wino_numerics_ok); the bf16 row-triple tile a tanh model (unbounded activations keep the
// three-pass x path of the 32-cell body).
inline CellPacks cell_packs(int mode, int activation, int Cx, int C, bool wino_numerics_ok) {
  const GateKnobs& k = gate_knobs();
  const bool blocks_ok = C % mv::kWnCh == 0 && (Cx % 16 == 0 || x_is_small(Cx));
  CellPacks p{};
  p.wp16 = mode == 1;
  p.wpw = mode == 1 && k.wino && blocks_ok && wino_numerics_ok;
  p.wpw3 = p.wpw && k.wino3;
  p.wpb = mode == 2;
  p.wpbt = mode == 2 && k.bf16t && blocks_ok && activation == 0;
  p.wdb = mode == 2 && k.bf16_bwd;
  p.wd16 = mode != 0 && !p.wdb;
  p.wdw = p.wd16 && mode == 1 && k.wino && k.wino_dgrad;
  return p;
}

// ------------------------------------------------------------------ forward
// Halves of ONE pre-transformed F(3,3) operand (rows x H x W cells, Cc channels in 16-channel
// groups); 0 where the form cannot run.  mv_set_compute_mode sizes the slot scratch with it, the
// plan checks the slot scratch against it.
inline size_t wino3_scratch_elems(int rows, int H, int W, int Cc) {
  return H < 3 ? 0 : mv::wino3_v_elems(rows, H, W, (Cc + 15) / 16 * 16);
}
// may an engine in this mode ever launch the F(3,3) form?  (activation 0: no per-tensor x exponent)
inline bool wino3_possible(int mode, int activation) {
  return mode == 1 && gate_knobs().wino && gate_knobs().wino3 && activation == 0;
}

// ------------------------------------------------------------------ light cone of the class encoder
// The class encoder starts from the zero state and its x is one hot cell per row and step (sparse
// x), so outside the cone of the observed cells a row's state equals that of an input-free row.
// Where this answers yes, the encoder problem carries one more row -- that background row -- and
// its h-steps between the first and the last run only the wave tiles the cone touches
// (ConvLstmArgs::cone_*; lists: engine_io.h build_enc_cone).  The lists exist for the F(3,3)
// row-triple kernel in its exact tiling only, so the rule restates what leads there: the f16x3
// mode with the form possible, a grid of whole row triples, whole channel blocks -- and a width
// of exactly 32, where a wave tile IS one (row, triple): narrower grids, whose tiles hold two
// triples or straddle two images, stay dense.  `sparse`: sparse_x_on of the scale; `step_exact`:
// every member of the step's launches passes cone_step_member_ok (one tiling and one form per
// step).  obs_len <= 2 has no step between the first and the last.  In the F(3,3) form the
// cone widens by a whole row TRIPLE per step (build_enc_cone): an observed cell's x reaches up to
// two triples and the step after it up to four, so a grid of fewer than five triples (9 x 16:
// three) would pay for the background row and skip next to nothing: it stays dense.
// The background row adds 1 / batch to every step of a coned encoder, and on the benchmark's feed
// the cone skips 17 % of the h-steps' tiles: from 16 rows on the row costs at most a third of
// that; below, down to batch 1 where it doubles the encoder, the dense encoder stays
// (MV_ENC_CONE=2 cones any batch: the small shapes of the tests).
constexpr int kEncConeMinBatch = 16;
inline bool enc_cone_geometry(int obs_len, int H, int W, int batch) {
  const int k = gate_knobs().enc_cone;
  return k != 0 && (k == 2 || batch >= kEncConeMinBatch) && obs_len >= 3 && H % 3 == 0 &&
         H / 3 >= 5 && W == 32;
}
// a scale whose encoders share the step's launches: exact tiling (no HALO), and the encoder cells
// carry the F(3,3) pack (has_packs: enc_cls and, where it runs, enc_reg)
inline bool cone_step_member_ok(int H, int W, bool has_packs) {
  return H >= 3 && W > 0 && 32 % W == 0 && has_packs;
}
inline bool enc_cone_planned(int mode, int activation, bool sparse, bool step_exact, int obs_len,
                             int H, int W, int C, int batch) {
  return enc_cone_geometry(obs_len, H, W, batch) && sparse && step_exact &&
         wino3_possible(mode, activation) && C % mv::kWnCh == 0;
}
// wave tiles (32 triple-cells) of a coned problem of `rows` rows, the background row included
inline int enc_cone_tiles(int rows, int H, int W) { return (rows * ((H + 2) / 3) * W + 31) / 32; }
// int32 elements of one step's lists: [count | 3 pad | tile list | computed-at-this-step flags]
inline size_t enc_cone_step_elems(int rows, int H, int W) {
  return 4 + 2 * (size_t)enc_cone_tiles(rows, H, W);
}

enum class GateForm { Direct16, Wino2, Wino3, Bf16, Bf16T };
struct ForwardPlan {
  GateForm form = GateForm::Direct16;
  bool halo = false;         // row-triple tile: halo tiling (30 of 32 lanes own a triple-cell)
  bool shift = false;        // 32-cell bodies: DPP column shift (every W divides 32)
  int map_mode = 0;          // the chosen kernel's block map
  int x_passes = 1;          // Bf16: 3 = the three-pass x kernel
  double mfma_factor = 3.0;  // fp16 / bf16 MFMA products ISSUED per executed fp32 product
};
struct ForwardProblem {      // one prepared problem of the group, as the plan sees it
  const mv::ConvLstm16Args* q;
  const ConvCell* cell;
  size_t v3x_cap, v3h_cap;   // the slot's scratch for the pre-transformed operands
};
inline bool has_dense_x(const mv::ConvLstmArgs& a) { return !a.x_small && a.Cx > 0 && !a.sx_corr; }

inline ForwardPlan plan_forward_group(int mode, const ForwardProblem* p, int n) {
  const GateKnobs& k = gate_knobs();
  ForwardPlan pl;
  // the halo tiling is ONE per launch; in it every member's operands must be addressable
  bool halo = false, halo_ok = true, shift = k.conv_shift, x_exp = false;
  for (int i = 0; i < n; ++i) {
    const mv::ConvLstmArgs& a = p[i].q->f;
    halo = halo || mv::wino3_needs_halo(a);
    halo_ok = halo_ok && mv::wino3_halo_addressable(a);
    shift = shift && a.W > 0 && 32 % a.W == 0;
    x_exp = x_exp || p[i].q->x_exp != nullptr;
  }
  const bool tile3_ok = !halo || halo_ok;
  bool wino = mode == 1 && k.wino, wino3 = wino && k.wino3 && tile3_ok;
  bool bf16t = mode == 2 && k.bf16t && tile3_ok;
  for (int i = 0; i < n; ++i) {
    const mv::ConvLstm16Args& q = *p[i].q;
    const mv::ConvLstmArgs& a = q.f;
    wino = wino && mv::wino_geometry_ok(a) && p[i].cell->wpw.p;
    wino3 = wino3 && mv::wino3_geometry_ok(a, q) && p[i].cell->wpw3.p &&
            (a.zero_state || p[i].v3h_cap >= wino3_scratch_elems(a.rows, a.H, a.W, a.C)) &&
            (!has_dense_x(a) || p[i].v3x_cap >= wino3_scratch_elems(a.rows, a.H, a.W, a.Cx));
    bf16t = bf16t && mv::bf16t_geometry_ok(a, q) && p[i].cell->wpbt.p;
  }
  pl.shift = shift;
  pl.map_mode = k.conv_map;
  if (mode == 2) {
    pl.form = bf16t ? GateForm::Bf16T : GateForm::Bf16;
    pl.mfma_factor = 1.0;
    if (bf16t) { pl.halo = halo; pl.map_mode = k.wino_map_bf16t; }
    else pl.x_passes = x_exp ? 3 : 1;
    return pl;
  }
  if (!wino && !wino3) return pl;
  pl.form = wino3 ? GateForm::Wino3 : GateForm::Wino2;
  pl.halo = wino3 && halo;
  pl.map_mode = wino3 ? k.wino_map_f33 : k.wino_map_f23;
  // 3 in the direct form; in a Winograd form 3 * (components * row tiles) / (3 * H) -- partial
  // tiles count (9 rows = 5 pairs: 2.22, not 2), weighted over the group by executed FLOPs
  double num = 0, den = 0;
  for (int i = 0; i < n; ++i) {
    const mv::ConvLstmArgs& a = p[i].q->f;
    const double cx = a.sx_corr ? 0.0 : (double)a.Cx;
    const double fl = (double)a.rows * a.H * a.W * (cx + (a.zero_state ? 0 : a.C));
    // (the halo tiling issues 32 lanes for 30 owned triple-cells)
    const double per = wino3 ? 5.0 * ((a.H + 2) / 3) / a.H * (mv::wino3_needs_halo(a) ? 32.0 / 30.0 : 1.0)
                             : 4.0 * ((a.H + 1) / 2) / a.H;
    num += fl * per; den += fl;
  }
  pl.mfma_factor = den > 0 ? num / den : (wino3 ? 5.0 / 3.0 : 2.0);
  return pl;
}
// a coned problem runs in the exact F(3,3) tiling or not at all (enc_cone_planned promised it)
inline void check_cone_plan(const ForwardPlan& pl, const ForwardProblem* p, int n) {
  for (int i = 0; i < n; ++i)
    MV_REQUIRE(!p[i].q->f.cone_on || (pl.form == GateForm::Wino3 && !pl.halo),
               "internal: a coned class-encoder step was planned outside the exact F(3,3) tiling");
}

// ------------------------------------------------------------------ dgrad
struct DgradPlan {
  bool bf16 = false;          // one bf16 plane per operand (compute mode 2, MV_BF16_BWD)
  bool wino = false;          // the Winograd F(2,3) form (two thirds of the MFMAs)
  bool shift = false;         // direct forms: DPP column shift
  double mfma_factor = 3.0;
  struct Slices { int nks_main, nks_x, n_kslice; } s[mv::kMaxGroup];   // split-K per problem
};
// The F(2,3) dgrad tiling: W divides 32 (DPP shift), row pairs, d h in whole 64-column blocks,
// the reduction (a.C = 4C gate columns here) in eight k slices of whole 16-column chunks.
inline bool wino_dgrad_geometry_ok(const mv::ConvLstmArgs& a) {
  return a.W > 0 && 32 % a.W == 0 && a.H >= 2 && a.out0_cols % 64 == 0 && (a.C / 16) % 8 == 0;
}
// probs: the dgrad problems (convlstm_dgrad_args: h = G, C = 4C); has_wdw: the chain carries the
// Winograd pack
inline DgradPlan plan_dgrad_group(int mode, const mv::ConvLstmArgs* probs, const bool* has_wdw,
                                  int n) {
  const GateKnobs& k = gate_knobs();
  DgradPlan pl;
  pl.bf16 = mode == 2 && k.bf16_bwd;
  pl.wino = mode == 1 && k.wino && k.wino_dgrad;
  pl.shift = k.conv_shift;
  for (int i = 0; i < n; ++i) {
    pl.wino = pl.wino && wino_dgrad_geometry_ok(probs[i]) && has_wdw[i];
    pl.shift = pl.shift && probs[i].W > 0 && 32 % probs[i].W == 0;
  }
  pl.mfma_factor = pl.wino ? 2.0 : (pl.bf16 ? 1.0 : 3.0);
  for (int i = 0; i < n; ++i) {
    const mv::ConvLstmArgs& a = probs[i];
    DgradPlan::Slices& s = pl.s[i];
    s = DgradPlan::Slices{0, 0, 0};
    if (pl.wino) {
      // (d h column block, slice) combos = 8 = the XCDs, the d x blocks a region of their own
      // with eight slices (convlstm_dgrad_wino_kernel)
      const int ncm = a.out0_cols / 64;
      int nkm = std::max(1, 8 / ncm);
      while ((a.C / 16) % nkm != 0) nkm /= 2;
      s.nks_main = nkm;
      s.nks_x = (a.out1 && a.out1_cols > 0) ? 8 : 1;
      continue;
    }
    // split-K over four channel-group ranges (see convlstm16_dgrad_dispatch)
    // (the bf16 dgrad is a third as long: whole-K tiles, no partial sums -- 1 208 vs 1 202 /
    // 1 178 traj/s with 2 / 4 slices at batch 64, profiles/r4u_*)
    const int nstages = 9 * (a.C / 16) / 3;
    const int ks = k.dgrad_kslices > 0 ? k.dgrad_kslices : (pl.bf16 ? 1 : 4);
    if (pl.bf16)
      MV_REQUIRE(nstages % MV_BF16_UNITS == 0, "internal: bf16 dgrad stage count %d", nstages);
    if (ks > 1 && nstages % (2 * ks) == 0) s.n_kslice = ks;
  }
  return pl;
}

// ------------------------------------------------------------------ wgrad
struct WgradPlan {
  bool generic = false;     // --convlstm_kernel other than 3: one deterministic pass, no partials
  bool f16 = false;         // the f16x3 GEMMs on transposed planes (else the fp32 kernel)
  bool one = false;         // ... on ONE fp16 plane per operand (compute mode 2)
  bool wino = false;        // ... in the row-triple form: 15 partial taps on a third of the cells
  bool wide = false;        // ... h rows on the wide tile
  bool wide_x = false;      // ... x rows on the wide tile too
  bool transpose3 = true;   // the three column-shifted copies of an operand from one read
  int map_mode = 0;         // wide tile's block map
  int nsplit = 0;           // splits of the h rows = partial slabs
  int nsplit_x = 0;         // splits of the x rows (<= nsplit)
  int ntaps = 9;
  long long Mtot = 0, Mrow = 0;     // cells, padded to whole 64-cell blocks
  long long Mtot3 = 0, Mrow3 = 0;   // row triples, likewise
  long long Mgemm = 0;              // cells of the GEMMs' reduction
  double mfma_factor = 1.0;
  size_t partial_elems = 0;         // floats the chosen form writes to the partial buffer
  mv::WgradArgs fp32{};             // the fp32 kernel's plan (pointers unset)
};
// force_wino: -1 the planner's choice; 0 / 1 the direct / the row-triple form whatever the switches
// say (mv_op_convlstm_bwd16, which checks wgrad16_wino3_ok itself)
inline WgradPlan plan_wgrad(int mode, int ksize, int R, int H, int W, int Cx, int C,
                            int force_wino = -1) {
  const GateKnobs& k = gate_knobs();
  WgradPlan pl;
  pl.Mtot = (long long)R * H * W;
  pl.Mrow = (pl.Mtot + 63) / 64 * 64;
  pl.Mtot3 = pl.Mtot / 3;
  pl.Mrow3 = (pl.Mtot3 + 63) / 64 * 64;
  pl.Mgemm = pl.Mtot;
  if (ksize != 3) { pl.generic = true; pl.mfma_factor = 0.0; return pl; }
  mv::WgradArgs& wa = pl.fp32;
  wa.R = R; wa.H = H; wa.W = W; wa.Cx = Cx; wa.C = C;
  mv::wgrad_plan(wa, 3072, k.wgrad_splits_set ? &k.wgrad_splits : nullptr);
  pl.nsplit = pl.nsplit_x = wa.nsplit;
  pl.partial_elems = mv::wgrad_partial_elems(wa);
  pl.f16 = mode != 0 && mv::wgrad16_ok(W, C);
  if (!pl.f16) return pl;
  pl.one = mode == 2 && k.bf16_bwd;
  pl.wino = k.wgrad_wino && (k.wgrad_wino_bf16 || !pl.one) && mv::wgrad16_wino3_ok(H);
  if (force_wino >= 0) pl.wino = force_wino == 1;
  pl.transpose3 = k.transpose3;
  if (pl.wino) { pl.ntaps = 15; pl.Mgemm = pl.Mtot3; }
  // the wide tile balances on 7 / 14 / 21 splits; the x rows and the reduction follow its count
  pl.wide = k.wgrad_wide && mv::wgrad16_wide_ok(W, C);
  if (pl.wide) {
    pl.map_mode = mv::wgrad16_wide_map_mode(C, k.wgrad_wide_map);
    pl.nsplit = mv::wgrad16_wide_splits(pl.Mgemm, wa.nsplit, pl.map_mode, k.wgrad_wide_splits);
  }
  pl.wide_x = pl.wide && k.wgrad_wide_x;
  pl.nsplit_x = (pl.wino && Cx > 0) ? mv::wgrad16_x_splits(pl.Mgemm, pl.nsplit, k.wgrad_x_splits)
                                    : pl.nsplit;
  pl.mfma_factor = (pl.one ? 1.0 : 3.0) * (pl.wino ? 5.0 / 9.0 : 1.0);
  pl.partial_elems = (size_t)pl.nsplit * pl.ntaps * (size_t)(Cx + C) * 4 * C;
  return pl;
}

}  // namespace
