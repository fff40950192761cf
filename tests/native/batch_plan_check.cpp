// batch_plan_check.cpp — enumerates plan_batch (renderer_amd/csrc/batch_plan.hpp) over every entry point, mode, bucket count
// at the pass boundaries, with and without matrices, both census decisions, and checks every launch of the call against the
// selection written out the long way: the nested conditions api_batch.hip held before the plan existed. Plain C++, no HIP:
// built by tests/test_frame_plan.py with gcc -fsanitize=address,undefined. Prints "BATCH PLAN OK <combinations> <launches>".
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

// ---- the selection as the three entry points used to spell it ----
static K old_count(BatchEntry e, bool relative, uint32_t p) {
  if (p != 0) return K::count_list;
  if (e == BatchEntry::ordered) return relative ? K::count_ordered_relative : K::count_ordered_distance;
  if (e == BatchEntry::draws) return K::count_pick;
  return relative ? K::count_chain_relative : K::count_chain_distance;
}

static K old_scatter(BatchEntry e, bool relative, uint32_t p, bool last, bool stores_model, bool general) {
  if (e == BatchEntry::ordered)
    return p == 0 ? (relative ? K::scatter_ordered_relative_mid : K::scatter_ordered_distance_mid) : last ? K::scatter_list_last : K::scatter_list_mid;
  const int model = !stores_model ? 0 : general ? 2 : 1;
  if (p == 0 && e == BatchEntry::lods) {
    if (relative) {
      if (!last) return K::scatter_chain_relative_mid;
      return model == 0 ? K::scatter_chain_relative_last : model == 2 ? K::scatter_chain_relative_general : K::scatter_chain_relative_model;
    }
    if (!last) return K::scatter_chain_distance_mid;
    return model == 0 ? K::scatter_chain_distance_last : model == 2 ? K::scatter_chain_distance_general : K::scatter_chain_distance_model;
  }
  if (p == 0 && last) return model == 0 ? K::scatter_pick_last : model == 2 ? K::scatter_pick_general : K::scatter_pick_model;
  if (p == 0) return K::scatter_pick_mid;
  return last ? K::scatter_list_last : K::scatter_list_mid;
}

static K old_model(BatchEntry e, bool relative, bool general) {
  if (e == BatchEntry::draws) return general ? K::model_pick_general : K::model_pick;
  if (relative) return general ? K::model_chain_relative_general : K::model_chain_relative;
  return general ? K::model_chain_distance_general : K::model_chain_distance;
}

int main() {
  static_assert(plan_batch(BatchEntry::draws, false, 128, true, false).scatter0 == K::scatter_pick_model, "usable at compile time");
  const unsigned long long buckets[] = {1, 2, 3, 200, 255, 256, 257, 258, 65535, 65536, 65537, 1ull << 24, (1ull << 24) + 1, 0x7fffffffull, 0x80000000ull};
  unsigned long long combos = 0, launches = 0;
  for (BatchEntry e : {BatchEntry::draws, BatchEntry::lods, BatchEntry::ordered})
    for (int relative = 0; relative < 2; ++relative)
      for (unsigned long long b : buckets)
        for (int want_model = 0; want_model < 2; ++want_model)
          for (int general = 0; general < 2; ++general) {
            if (e == BatchEntry::ordered && b > 65536) continue;  // refused before a plan is made
            ++combos;
            const BatchPlan p = plan_batch(e, relative != 0, b, want_model != 0, general != 0);
            // the passes, as the entry points computed them
            uint32_t bits = 1;
            while ((1ull << bits) < b) ++bits;
            CHECK(batch_key_bits(b) == bits && (b == 1 || (1ull << (bits - 1)) < b), "B = %llu: %u bits", b, bits);
            if (e == BatchEntry::ordered) bits += 16;
            CHECK(p.passes == (bits + 7u) / 8u && p.passes >= 1 && p.passes <= kBatchMaxPasses, "B = %llu: %u passes", b, p.passes);
            CHECK(p.several() == (p.passes > 1), "several");
            if (e == BatchEntry::ordered) CHECK(p.passes == (b <= 256 ? 3u : 4u), "ordered: three passes up to 256 buckets, four up to 65 536");
            else CHECK(p.several() == (b > 256), "one pass up to 256 buckets");
            const bool several = p.passes > 1;
            for (uint32_t q = 0; q < p.passes; ++q) {
              const bool last = q + 1 == p.passes;
              const bool stores_model = last && !several && want_model;  // a.batch_model of that pass
              CHECK(p.count(q) == old_count(e, relative != 0, q), "count, pass %u of %u", q, p.passes);
              CHECK(p.scatter(q) == old_scatter(e, relative != 0, q, last, stores_model, general != 0), "scatter, pass %u of %u", q, p.passes);
              launches += 3;
            }
            CHECK(p.commands == (e == BatchEntry::draws ? K::commands_pair : K::commands_chain), "command writer");
            CHECK(p.model == (several && want_model ? old_model(e, relative != 0, general != 0) : K::none), "model kernel");
            CHECK(p.count0 != K::none && p.scatter0 != K::none && p.commands != K::none, "every pass launches something");
            launches += 1 + (p.model != K::none);
          }
  std::printf("BATCH PLAN OK %llu %llu\n", combos, launches);
  return 0;
}
