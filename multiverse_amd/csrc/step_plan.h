// which form each launch of a decode step takes outside the gate convolution -- the graph
// attention, the decoder tail, the beam / stochastic-beam / sampled selection, the chain pairs --
// and the bounds those forms share.  Part of the ONE translation unit engine.hip (included from
// there right after gate_plan.h; not a stand-alone header).
//
// Nothing here launches or allocates: these functions answer questions.  The launchers
// (engine_setup.h, engine_forward.h), the forwards (engine_forward.h, engine_train.h), mv_create
// and the single-kernel entry points (engine_ops.h) ask instead of restating the rules.
// (tests/test_step_plan_host.py compiles this file alone, on the host, and checks the rules
// against tables written out there.)
#pragma once

#include "row_form.h"

namespace {

// ------------------------------------------------------------------ the A/B switches
// The switches of the decode step and of the chain streams, read once per process with
// gate_plan.h's helpers (DESIGN.md carries the table).  No other csrc file calls getenv for them.
struct StepKnobs {
  int gnn;                  // MV_GNN=v1: one wave per cell; v2: LDS-tiled, one cell per thread
                            // (3, default: the register-blocked third version)
  bool tail_grouped;        // MV_TAIL=v1: hidden2grid convolved in place, separate argmax /
                            // embedding launches (the first-round decoder tail)
  bool train_tail_grouped;  // MV_TRAIN_TAIL=v1: those launches in the training forward alone
  bool beam_step_single;    // MV_BEAM_STEP=v1: the single-launch beam step at every K
  bool beam_shared_first;   // MV_BEAM_SHARED_FIRST=0: the first beam step on B tiled rows per sample
  bool beam_gnn_dedupe;     // MV_BEAM_GNN_DEDUPE=0: the attention after the parent gather, every row
  bool sparse_x;            // MV_SPARSE_X=0: the one-hot decoder / encoder input as a dense embedding
  int chain_streams;        // MV_CHAIN_STREAMS=1: the greedy forward on one stream (default 2)
  bool chain_priority;      // MV_CHAIN_PRIORITY=1: the regression pair's stream at the lowest priority
};

inline const StepKnobs& step_knobs() {
  static const StepKnobs k = [] {
    auto is = [](const char* name, const char* value) {
      const char* v = getenv(name);
      return v && strcmp(v, value) == 0;
    };
    StepKnobs s{};
    s.gnn = is("MV_GNN", "v1") ? 1 : (is("MV_GNN", "v2") ? 2 : 3);
    s.tail_grouped = !is("MV_TAIL", "v1");
    s.train_tail_grouped = !is("MV_TRAIN_TAIL", "v1");
    s.beam_step_single = is("MV_BEAM_STEP", "v1");
    s.beam_shared_first = env_on("MV_BEAM_SHARED_FIRST");
    s.beam_gnn_dedupe = env_on("MV_BEAM_GNN_DEDUPE");
    s.sparse_x = env_on("MV_SPARSE_X");
    s.chain_streams = env_num("MV_CHAIN_STREAMS", 2) == 1 ? 1 : 2;
    s.chain_priority = env_num("MV_CHAIN_PRIORITY", 0) == 1;
    return s;
  }();
  return k;
}

// ------------------------------------------------------------------ one wave holds a row
// beam_rank / sbs_perturb / sample_step / score_step keep a K-cell row in one wave's registers
// (lane l owns k = l + 64 j, j < kBeamRankJ; with_rank_j picks the instantiation).
inline bool row_fits_wave(int K) { return K <= 64 * mv::kBeamRankJ; }
inline void require_row_fits_wave(const char* who, int K) {
  MV_REQUIRE(row_fits_wave(K), "%s: K = %d cells (one wave holds a row of at most %d)", who, K,
             64 * mv::kBeamRankJ);
}

// dynamic LDS of beam_step_kernel: candidates and their parents of a sample's B rows plus the
// reduction scratch.  mv_create and the ops raise the kernels' limit to it (ensure_beam_step_lds).
inline size_t beam_step_lds_bytes(int B, int K) {
  return ((size_t)2 * B * K + 512) * sizeof(float);
}

// ------------------------------------------------------------------ beam step
// RankSelect: the rank count on one wave per (n, b) row over the whole chip, then the per-sample
// selection.  Single: one workgroup per sample does both (any K the LDS holds).  A masked step
// exists in the two-launch form only, whatever MV_BEAM_STEP says: its callers refuse rows that do
// not fit a wave (require_row_fits_wave) before they ask.  `have_cand`: the [N*B, K] scratch of
// the two-launch form exists.
enum class BeamStepForm { Single, RankSelect };
inline BeamStepForm beam_step_form(int K, bool have_cand, bool masked) {
  if (masked) return BeamStepForm::RankSelect;
  return (step_knobs().beam_step_single || !row_fits_wave(K) || !have_cand)
             ? BeamStepForm::Single : BeamStepForm::RankSelect;
}

// ------------------------------------------------------------------ constrained rows
// The form of a constrained step and the rule that picks it: row_form.h.
using mv::RowForm;
using mv::row_form;

// The constraint member of a captured forward's graph key (engine_forward.h run_forward): what a
// captured step bakes in of the four constraints.  Layout codes of the mask and of the bias: 0 not
// set, 1 one plane for every step, 2 a plane per step.  The motion cost: its radius (0 = not set)
// and whether the acc tables are present.  The revisit cost: set or not, and whether it starts from
// the observed cells.  Two different states never share a value; the values themselves mean
// nothing and are never stored.
constexpr int kMotionKeys = 9;   // not set, or a radius with acc absent / present
static_assert(2 * MV_MOTION_MAX_RADIUS < kMotionKeys,
              "graph key: the motion member 2 * radius - 1 + acc must stay below its radix");
inline int constraint_graph_key(int mask_layout, int bias_layout, int radius, bool acc,
                                bool revisit, bool revisit_seed) {
  const int motion = radius > 0 ? 2 * radius - 1 + (acc ? 1 : 0) : 0;
  const int path = revisit ? (revisit_seed ? 2 : 1) : 0;
  return mask_layout + 3 * (bias_layout + 3 * (motion + kMotionKeys * path));
}

// ------------------------------------------------------------------ graph attention (forward)
// PerCell: gnn_attend_kernel, one wave per cell, any shape.  Tiled: gnn_attend_v2_kernel, LDS
// tiles of 32 cells; its tiling wants W <= 32 and C == 256, and it stages ONE 64-channel scene
// chunk, so D <= 64.  Blocked: gnn_attend_v3_kernel, register-blocked; it takes the scene
// channels as no chunk or one whole chunk (D == 0 || D == 64) and addresses h through 32-bit byte
// offsets.  `version_wanted`: 1 / 2 / 3 ask for at most that form, 0 for the MV_GNN knob's.
// `h_bytes_addressed`: bytes of the h operand the caller wants addressable -- the engine passes
// its worst case batch * max(1, beam) * K * C * 4 (one form per engine and scale, whatever a
// step's row count), a single-kernel entry point its actual cells * C * 4.
// Ordered: a launch that carries two jobs takes the weaker of their forms.
enum class GnnForm { PerCell, Tiled, Blocked };
inline GnnForm gnn_form(int version_wanted, int W, int C, int D, size_t h_bytes_addressed) {
  const int ver = version_wanted ? version_wanted : step_knobs().gnn;
  if (ver < 2 || W > 32 || C != 256 || D > 64) return GnnForm::PerCell;
  if (ver >= 3 && (D == 0 || D == 64) && h_bytes_addressed < ((size_t)1 << 32))
    return GnnForm::Blocked;
  return GnnForm::Tiled;
}
inline GnnForm weaker(GnnForm a, GnnForm b) { return a < b ? a : b; }

// ------------------------------------------------------------------ beam decode: attention once per state row
// run_decoders_beam computes h + GNN(h) BEFORE the parent gather, on the state rows that some
// surviving beam continues: the selection marks them in `row_ref`, the attention skips the rest.
// Who takes row_ref (kernels_misc.h): beam_select_kernel, sbs_select_kernel and
// beam_step_kernel write it; gnn_attend_v2_kernel and gnn_attend_v3_kernel read it;
// gnn_attend_kernel has no such argument and computes every row it is given, which is correct
// too, only without the saving.  So every combination would compute the right thing.  The rule
// stays what it has always been all the same -- the two-launch step and an engine that is not
// held on the per-cell attention by MV_GNN=v1 -- and therefore asks the knob, not gnn_form: a
// shape that gnn_form demotes to PerCell (hidden_size != 256, W > 32, D > 64) keeps the dedupe
// order of launches it has today.  A masked step under MV_BEAM_STEP=v1 runs the two-launch form
// (beam_step_form) and likewise keeps today's answer, no dedupe: hence `masked = false` below.
inline bool beam_gnn_dedupe(const mv_config& c, int K, bool shared_first) {
  return step_knobs().beam_gnn_dedupe && shared_first && c.use_gnn &&
         beam_step_form(K, /*have_cand=*/true, /*masked=*/false) == BeamStepForm::RankSelect &&
         step_knobs().gnn >= 2;
}

// ------------------------------------------------------------------ decoder tail
// Grouped: hidden2grid of every chain as one GEMM launch plus one gather / argmax / embedding
// launch (decode_tail.h).  Separate: a hidden2grid convolution per chain, argmax and embedding
// launches of their own.  The grouped tail holds a row's 9 P taps in LDS (K * 2 <= 2048) and
// embeds E <= 512 channels in 16-channel groups.  Config validation already forces
// emb_size % 32 == 0 && emb_size <= 512, so a grid of more than 1024 cells is the only live way
// not to fit.  `Kmax`: the largest enabled scale's cells.
inline bool tail_grouped_fits(int E, int Kmax) {
  return (size_t)Kmax * 2 <= 2048 && E % 16 == 0 && E <= 512;
}
// Inference takes the grouped tail unless MV_TAIL=v1, and run_tail fails where it does not fit
// (the sampled and the scoring forward have no other tail); training falls back to the separate launches
// where it does not fit, or by MV_TRAIN_TAIL=v1.
enum class TailForm { Grouped, Separate };
inline TailForm tail_form(bool training, int E, int Kmax) {
  const StepKnobs& k = step_knobs();
  if (!k.tail_grouped) return TailForm::Separate;
  if (training && !(k.train_tail_grouped && tail_grouped_fits(E, Kmax))) return TailForm::Separate;
  return TailForm::Grouped;
}

// ------------------------------------------------------------------ scene stack
// Proj1x1: scene_proj1x1_mfma_kernel, --scene_conv_kernel 1 with at most 64 output channels.
// Tiled: scene_conv3_s2_tiled_kernel -- k = 3 with exactly the 64 output channels its 16 x 4
// thread map covers, and Ci <= 64: a tap's weights Ci x 64 floats (16 KB) and the 16 pixels'
// inputs stay inside its static LDS.  PerOutput: scene_conv_s2_tanh_kernel, every other shape.
// All three compute the same bits where they overlap.
enum class SceneConvForm { PerOutput, Proj1x1, Tiled };
inline SceneConvForm scene_conv_form(int k, int Ci, int Co) {
  if (k == 1 && Co <= 64) return SceneConvForm::Proj1x1;
  if (k == 3 && Co == 64 && Ci >= 1 && Ci <= 64) return SceneConvForm::Tiled;
  return SceneConvForm::PerOutput;
}

// ------------------------------------------------------------------ chain pairs of the greedy forward
// The four chains of a greedy forward (class / regression x two scales) exchange nothing between
// the scene stage and the end of the decode, and want different things from the chip: a gate
// launch the matrix pipe, the attention / transform / tail kernels HBM and L2.  So the greedy
// inference forward issues them as two chain pairs -- the class chains on the engine's stream,
// the regression chains on a second one -- that meet once per forward: the second stream starts
// after everything queued before the forward (uploads, weight packs), the engine's stream
// continues after both.  The regression pair does not read the scene stage, which thereby runs
// under its first encoder steps.  One stream, in the order of before: no second stream
// (MV_CHAIN_STREAMS=1); profiling (event brackets around overlapped launches time nothing);
// hipGraph capture (a captured fork / join becomes parallel branches of the graph); a beam
// handle; a model with one decoder (no regression chains); the separate decoder tail; batches
// above kChainPairMaxBatch -- measured on one box, alternating fresh processes: batch 64 +0.7 %
// (bf16 mode +2.1 %), batch 256 -2.6 % (the two gate launches of a step run side by side rather
// than against the other pair's small kernels, and at 256 rows a launch of its own per pair costs
// more than the small kernels hide); sizes in between are unmeasured and stay on one stream.
constexpr int kChainPairMaxBatch = 64;
inline bool chain_pairs_planned(const mv_config& c, bool greedy, bool second_stream,
                                bool profiling, bool capturing, bool grouped_tail) {
  return greedy && second_stream && !profiling && !capturing && c.beam_size == 1 &&
         !c.use_single_decoder && grouped_tail && c.batch_size <= kChainPairMaxBatch;
}

}  // namespace
