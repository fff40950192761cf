// batch_sorted_plan_check.cpp — enumerates plan_batch_sorted (renderer_amd/csrc/batch_plan.hpp) over both LOD modes, both depth
// metrics, every depth_bits, with and without matrices, both census decisions, and checks every launch of a
// mip_batch_draws_sorted call against the selection written out the long way; then the run stage's launches. plan_batch itself
// must not have moved for the entry points it plans. Plain C++, no HIP: built by tests/test_sorted_restatement.py with
// g++ -fsanitize=address,undefined. Prints "SORTED PLAN OK <combinations> <launches>".
#include "../../renderer_amd/csrc/batch_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <initializer_list>

using namespace mip;
using K = BatchKernel;

#define CHECK(cond, ...)                                            \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::printf("FAILED %s:%d %s — ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                                     \
      std::printf("\n");                                            \
      std::exit(1);                                                 \
    }                                                               \
  } while (0)

static K want_count0(bool relative, bool axis) {
  if (relative) return axis ? K::count_sorted_relative_axis : K::count_sorted_relative_radial;
  return axis ? K::count_sorted_distance_axis : K::count_sorted_distance_radial;
}

static K want_scatter0(bool relative, bool axis) {
  if (relative) return axis ? K::scatter_sorted_relative_axis_mid : K::scatter_sorted_relative_radial_mid;
  return axis ? K::scatter_sorted_distance_axis_mid : K::scatter_sorted_distance_radial_mid;
}

static K want_model(bool relative, bool general) {
  if (relative) return general ? K::model_chain_relative_general : K::model_chain_relative;
  return general ? K::model_chain_distance_general : K::model_chain_distance;
}

int main() {
  static_assert(plan_batch_sorted(false, false, 16, false, false).passes == 2, "usable at compile time");
  static_assert(plan_batch_sorted(true, true, 32, true, true).model == K::model_chain_relative_general, "usable at compile time");
  unsigned long long combos = 0, launches = 0;
  for (int relative = 0; relative < 2; ++relative)
    for (int axis = 0; axis < 2; ++axis)
      for (uint32_t bits : {16u, 24u, 32u})
        for (int want = 0; want < 2; ++want)
          for (int general = 0; general < 2; ++general) {
            ++combos;
            const BatchPlan p = plan_batch_sorted(relative != 0, axis != 0, bits, want != 0, general != 0);
            CHECK(p.passes == bits / 8u && p.passes >= 2 && p.passes <= kBatchMaxPasses, "%u bits: %u passes", bits, p.passes);
            CHECK(p.several(), "the key never fits one digit");
            for (uint32_t q = 0; q < p.passes; ++q) {
              const bool last = q + 1 == p.passes;
              CHECK(p.count(q) == (q ? K::count_list : want_count0(relative != 0, axis != 0)), "count, pass %u of %u", q, p.passes);
              CHECK(p.scatter(q) == (!q ? want_scatter0(relative != 0, axis != 0) : last ? K::scatter_list_last : K::scatter_list_mid),
                    "scatter, pass %u of %u", q, p.passes);
              launches += 3;  // count, rowscan, scatter
            }
            CHECK(p.scatter(p.passes - 1) == K::scatter_list_last, "the last pass writes instance_ids (and slot_of)");
            CHECK(p.commands == K::sorted_members, "the members sum stands in the command writer's place");
            CHECK(p.model == (want ? want_model(relative != 0, general != 0) : K::none), "matrices go through slot_of");
            launches += 1 + kBatchRunStageLaunches + (p.model != K::none);
          }
  CHECK(combos == 2 * 2 * 3 * 2 * 2, "every combination");
  // the run stage, in launch order
  static_assert(kBatchRunStageLaunches == 4, "heads, scan, commands, counts");
  CHECK(batch_run_stage(0) == K::run_heads && batch_run_stage(1) == K::rowscan && batch_run_stage(2) == K::run_commands &&
            batch_run_stage(3) == K::run_counts, "the run stage's launches");
  // plan_batch keeps planning the other entry points as it did (tests/native/batch_plan_check.cpp enumerates them)
  CHECK(plan_batch(BatchEntry::ordered, false, 200, true, false).passes == 3 &&
            plan_batch(BatchEntry::ordered, false, 200, true, false).count0 == K::count_ordered_distance &&
            plan_batch(BatchEntry::lods, true, 257, true, true).model == K::model_chain_relative_general &&
            plan_batch(BatchEntry::draws, false, 128, true, false).scatter0 == K::scatter_pick_model, "plan_batch did not move");
  std::printf("SORTED PLAN OK %llu %llu\n", combos, launches);
  return 0;
}
