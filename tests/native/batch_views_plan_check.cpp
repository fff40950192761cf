// batch_views_plan_check.cpp — enumerates plan_batch (renderer_amd/csrc/batch_plan.hpp) for mip_batch_draws_views: every view
// count, both modes, per-view bucket counts B that put the global bucket count n_views x B either side of every pass boundary
// (256, 65 536, 2^24), and the n_views x N capacity rule — against the plan as the header states it: one pass up to 256 global
// buckets, else ceil(key_bits / 8) passes whose later passes are the list kernels and whose last one knows the views' bases.
// Plain C++, no HIP: built by tests/test_views_batch_restatement.py with gcc -fsanitize=address,undefined.
// Prints "VIEWS PLAN OK <combinations> <launches>".
#include "../../renderer_amd/csrc/batch_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <set>

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

int main() {
  static_assert(plan_batch(BatchEntry::views, false, 256, false, false).scatter0 == K::scatter_views_distance_last, "usable at compile time");
  static_assert(plan_batch(BatchEntry::views, true, 257, false, false).passes == 2, "257 global buckets: two passes");
  const unsigned long long boundaries[] = {256, 65536, 1ull << 24};
  unsigned long long combos = 0, launches = 0;
  for (unsigned long long views = 1; views <= 16; ++views) {
    // per-view bucket counts: small ones, and for every boundary the largest B with views x B <= boundary and its neighbours
    std::set<unsigned long long> per_view = {1, 2, 3, 6, 200, 4096, 4097};
    for (unsigned long long edge : boundaries)
      for (long long d = -1; d <= 2; ++d)
        if ((long long)(edge / views) + d >= 1) per_view.insert(edge / views + (unsigned long long)d);
    for (unsigned long long b : per_view)
      for (int relative = 0; relative < 2; ++relative) {
        const unsigned long long g = views * b;  // global buckets
        ++combos;
        const BatchPlan p = plan_batch(BatchEntry::views, relative != 0, g, false, false);
        const uint32_t want_passes = g <= 256 ? 1u : g <= 65536 ? 2u : g <= (1ull << 24) ? 3u : 4u;
        CHECK(p.passes == want_passes, "%llu views x %llu buckets: %u passes", views, b, p.passes);
        CHECK(p.passes == (batch_key_bits(g) + 7u) / 8u, "passes from the key's bits");
        CHECK(p.several() == (g > 256), "one pass up to 256 global buckets");
        CHECK(p.commands == K::commands_views, "the per-view command writer");
        CHECK(p.model == K::none, "no matrices");
        CHECK(p.count0 == (relative ? K::count_views_relative : K::count_views_distance), "count, pass 0");
        for (uint32_t q = 0; q < p.passes; ++q) {
          const bool last = q + 1 == p.passes;
          K want_count = q ? K::count_list : p.count0;
          K want_scatter;
          if (q == 0) want_scatter = relative ? (last ? K::scatter_views_relative_last : K::scatter_views_relative_mid)
                                              : (last ? K::scatter_views_distance_last : K::scatter_views_distance_mid);
          else want_scatter = last ? K::scatter_views_list_last : K::scatter_list_mid;
          CHECK(p.count(q) == want_count, "count, pass %u of %u", q, p.passes);
          CHECK(p.scatter(q) == want_scatter, "scatter, pass %u of %u", q, p.passes);
          launches += 3;
        }
        launches += 1;
        // the flags the other entry points read do not reach this plan
        const BatchPlan other = plan_batch(BatchEntry::views, relative != 0, g, true, true);
        CHECK(other.passes == p.passes && other.scatter0 == p.scatter0 && other.model == K::none, "want_model / general are ignored");
      }
  }
  // the other entry points keep the plain last list pass
  for (BatchEntry e : {BatchEntry::draws, BatchEntry::lods, BatchEntry::ordered})
    CHECK(plan_batch(e, false, 300, false, false).scatter(plan_batch(e, false, 300, false, false).passes - 1) == K::scatter_list_last, "list_last");
  // capacity: n_views x N < 2^32
  CHECK(batch_views_entries_fit(1, 0xffffffffull) && !batch_views_entries_fit(1, 1ull << 32), "one view");
  CHECK(batch_views_entries_fit(16, (1ull << 28) - 1) && !batch_views_entries_fit(16, 1ull << 28), "sixteen views");
  CHECK(batch_views_entries_fit(3, 1431655765ull) && !batch_views_entries_fit(3, 1431655766ull), "three views");
  CHECK(batch_views_entries_fit(16, 0) && batch_views_entries_fit(4, 1000000), "small");
  std::printf("VIEWS PLAN OK %llu %llu\n", combos, launches);
  return 0;
}
