// The forms of a constrained decode step, and the one rule that picks a step's form.  Plain C++:
// no HIP, compilable on the host alone (tests/test_step_plan_host.py does).  kernels_misc.h takes
// the template parameter of its step kernels from here, step_plan.h the rule.
#pragma once

namespace mv {

// The kernels that hold a row in one wave (beam_rank / sbs_perturb / sample_step) come in five
// forms, each the one before plus one thing; the two occupancy kernels in the first three.
//   Plain   nothing set.
//   Masked  mv_set_cell_mask alone: the in-row predicate is "in row AND allowed" (the `am` bits).
//   Biased  mv_set_cell_bias, with or without a mask: works on the `am` bits (the in-row bits
//           when no mask plane is given) and adds the row's bias plane b[J].
//   Motion  mv_set_motion_cost, with or without a mask and a bias: b is b_eff, the bias (or
//           0.0f) plus the terms each wave derives from its row's path.
//   Path    mv_set_revisit_cost, with or without the three above: b_eff (its motion part only
//           when a motion cost is set) plus rterm, and the row's visited set is stored.
// ONE instantiation per form serves every combination of the optional planes below it.  A
// constrained beam step is a `masked` one to step_plan.h's beam_step_form.
enum class RowForm { Plain, Masked, Biased, Motion, Path };

constexpr RowForm row_form(bool masked, bool biased, bool motion, bool revisit) {
  return revisit ? RowForm::Path
         : motion ? RowForm::Motion
         : biased ? RowForm::Biased
         : masked ? RowForm::Masked : RowForm::Plain;
}

// what a form carries: each implies the ones before it
constexpr bool row_has_bits(RowForm f) { return f >= RowForm::Masked; }    // the allowed bits `am`
constexpr bool row_has_bias(RowForm f) { return f >= RowForm::Biased; }    // the additive b[J]
constexpr bool row_has_motion(RowForm f) { return f >= RowForm::Motion; }  // b from the row's path
constexpr bool row_has_path(RowForm f) { return f == RowForm::Path; }      // the visited set

}  // namespace mv
