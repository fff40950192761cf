// batch_plan_check.cpp — enumerates plan_batch (renderer_amd/csrc/batch_plan.hpp) over every entry point, mode, bucket count
// at the pass boundaries, with and without matrices, both census decisions, and checks every launch of the call against the
// selection written out the long way: the nested conditions api_batch.hip held before the plan existed. Plain C++, no HIP:
// built by tests/test_frame_plan.py with gcc -fsanitize=address,undefined. Prints "BATCH PLAN OK <combinations> <launches>".
// Then the pass schedule (batch_pass_io, batch_pass_launch, batch_run_stage_list) of every entry point, mip_batch_draws_views
// and mip_batch_draws_sorted included, against the three pass loops api_batch.hip held before it had one pass driver, and the
// schedule's invariants directly. Prints "BATCH SCHEDULE OK <plans> <passes>" in front of the plan's line.
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

// ---- the wiring of a pass as the three drivers used to spell it: their loops, with every buffer named instead of pointed at ----
using G = BatchGrid;
struct OldPass {
  uint32_t shift, totals_row;
  int keys_in, ids_in, keys_out, ids_out;  // index into d_keys / d_ids, -1: nullptr
  bool bucket_hist, instance_ids, slot_of, batch_model;
  K kernel[4];  // count, rowscan, commands (none: not launched), scatter
  G grid[4];
};
enum OldDriver { old_draws, old_sorted, old_views };

static OldPass old_pass(OldDriver d, const BatchPlan& plan, uint32_t p, bool out_batch_model) {
  OldPass a{};
  const bool several = plan.several();
  const bool last = p + 1 == plan.passes;
  a.shift = p * kBatchDigitBits;
  a.totals_row = p;  // a.totals = bs.d_totals + p * kBatchBins
  a.keys_in = p ? (int)((p - 1) & 1u) : -1;
  a.ids_in = p ? (int)((p - 1) & 1u) : -1;
  a.keys_out = last ? -1 : (int)(p & 1u);
  a.ids_out = last ? -1 : (int)(p & 1u);
  a.instance_ids = last;
  switch (d) {
    case old_draws:
      a.bucket_hist = several && p == 0;
      a.slot_of = last && several && out_batch_model;
      a.batch_model = (last && !several) ? out_batch_model : false;
      break;
    case old_sorted:  // a.bucket_hist and a.batch_model stay null inside the passes
      a.slot_of = last && out_batch_model;
      break;
    case old_views:  // a.slot_of and a.batch_model stay null
      a.bucket_hist = several && p == 0;
      break;
  }
  a.kernel[0] = plan.count(p), a.grid[0] = G::tiles;      // launch(ctx, plan.count(p), a.n_tiles, ...)
  a.kernel[1] = K::rowscan, a.grid[1] = G::bins;          // launch(ctx, rowscan, a.n_bins, ...)
  a.kernel[2] = K::none, a.grid[2] = G::one;
  if (p == 0) a.kernel[2] = plan.commands;                // launch(ctx, plan.commands, 1, ...)
  a.kernel[3] = plan.scatter(p), a.grid[3] = G::tiles;    // launch(ctx, plan.scatter(p), a.n_tiles, ...)
  return a;
}

static unsigned long long g_plans = 0, g_passes = 0;

// every field of every pass against the old loop, then the invariants a ping-pong must keep
static void check_schedule(OldDriver d, const BatchPlan& plan, bool want_model, const char* what) {
  const bool with_hist = d != old_sorted;
  ++g_plans;
  uint32_t commands = 0, model_stores = 0, slot_maps = 0;
  for (uint32_t p = 0; p < plan.passes; ++p) {
    ++g_passes;
    const OldPass o = old_pass(d, plan, p, want_model);
    const BatchPassIo io = batch_pass_io(plan, p, want_model, with_hist);
    CHECK(io.shift == o.shift && io.totals_row == o.totals_row, "%s: shift / totals row, pass %u of %u", what, p, plan.passes);
    CHECK(io.list_in == o.keys_in && io.list_in == o.ids_in, "%s: list read, pass %u of %u", what, p, plan.passes);
    CHECK(io.list_out == o.keys_out && io.list_out == o.ids_out, "%s: list written, pass %u of %u", what, p, plan.passes);
    CHECK(io.ids == o.instance_ids && io.slot_of == o.slot_of && io.model == o.batch_model && io.bucket_hist == o.bucket_hist,
          "%s: outputs, pass %u of %u", what, p, plan.passes);
    CHECK(io.commands == (o.kernel[2] != K::none), "%s: commands, pass %u of %u", what, p, plan.passes);
    static_assert(kBatchPassLaunches == 4 && kBatchLaunchCount == 0 && kBatchLaunchRowscan == 1 && kBatchLaunchCommands == 2 && kBatchLaunchScatter == 3,
                  "count, rowscan, commands, scatter");
    for (uint32_t i = 0; i < kBatchPassLaunches; ++i) {
      const BatchLaunch l = batch_pass_launch(plan, p, i);
      CHECK(l.kernel == o.kernel[i] && l.grid == o.grid[i], "%s: launch %u of pass %u of %u", what, i, p, plan.passes);
    }
    // the invariants
    const bool last = p + 1 == plan.passes;
    CHECK(io.shift + kBatchDigitBits <= 32 && io.totals_row < kBatchMaxPasses, "%s: a digit of a 32-bit key, a row of the totals", what);
    CHECK(io.list_in >= -1 && io.list_in <= 1 && io.list_out >= -1 && io.list_out <= 1, "%s: two buffer pairs", what);
    CHECK((p == 0) == (io.list_in < 0) && last == (io.list_out < 0), "%s: pass 0 reads none, the last pass writes none", what);
    if (p) CHECK(io.list_in == batch_pass_io(plan, p - 1, want_model, with_hist).list_out, "%s: pass %u reads what pass %u wrote", what, p, p - 1);
    CHECK(io.list_in < 0 || io.list_in != io.list_out, "%s: pass %u reads and writes the same list", what, p);
    CHECK(io.ids == last, "%s: only the last pass writes ids", what);
    CHECK(!io.slot_of || last, "%s: only the last pass writes the slot map", what);
    CHECK(io.bucket_hist == (with_hist && plan.several() && p == 0), "%s: the histogram is pass 0's, of several", what);
    commands += io.commands;
    model_stores += io.model;
    slot_maps += io.slot_of;
    CHECK(io.commands == (p == 0), "%s: the commands kernel runs on pass 0", what);
  }
  CHECK(commands == 1, "%s: the commands kernel runs exactly once", what);
  // matrices: the single pass, or the model kernel through the slot map, or nobody — by want_model and several() alone
  const bool by_pass = want_model && !plan.several(), by_kernel = want_model && plan.several();
  CHECK(model_stores == (by_pass ? 1u : 0u), "%s: the single pass stores the matrices", what);
  CHECK((plan.model != K::none) == by_kernel && slot_maps == (by_kernel ? 1u : 0u), "%s: the model kernel and its slot map", what);
  if (d == old_sorted) {
    const uint32_t run_list = batch_run_stage_list(plan);
    CHECK(run_list == ((plan.passes - 1) & 1u), "%s: a.slot_bucket = bs.d_keys[(plan.passes - 1) & 1u]", what);
    CHECK((int32_t)run_list != batch_pass_io(plan, plan.passes - 1, want_model, with_hist).list_in, "%s: the run stage overwrites the list the last pass read", what);
    for (uint32_t k = 0; k < kBatchRunStageLaunches; ++k)  // launch(ctx, kernel, kernel == rowscan ? 1u : a.n_tiles, ...)
      CHECK(batch_run_stage_grid(k) == (batch_run_stage(k) == K::rowscan ? G::one : G::tiles), "%s: run stage launch %u", what, k);
  }
}

int main() {
  static_assert(batch_pass_io(plan_batch(BatchEntry::lods, false, 257, true, false), 1, true, true).slot_of, "usable at compile time");
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
            check_schedule(old_draws, p, want_model != 0, "draws / lods / ordered");
          }
  // mip_batch_draws_shard: lods without matrices (its MipBatchOutputs has no batch_model)
  for (int relative = 0; relative < 2; ++relative)
    for (unsigned long long b : buckets)
      for (int general = 0; general < 2; ++general) check_schedule(old_draws, plan_batch(BatchEntry::shard, relative != 0, b, false, general != 0), false, "shard");
  // mip_batch_draws_views: the same list as GLOBAL bucket counts (it holds both sides of every pass edge); never matrices
  for (int relative = 0; relative < 2; ++relative)
    for (unsigned long long b : buckets) check_schedule(old_views, plan_batch(BatchEntry::views, relative != 0, b, false, false), false, "views");
  // mip_batch_draws_sorted
  for (int relative = 0; relative < 2; ++relative)
    for (int axis = 0; axis < 2; ++axis)
      for (uint32_t bits : {16u, 24u, 32u})
        for (int want_model = 0; want_model < 2; ++want_model)
          for (int general = 0; general < 2; ++general)
            check_schedule(old_sorted, plan_batch_sorted(relative != 0, axis != 0, bits, want_model != 0, general != 0), want_model != 0, "sorted");
  CHECK(g_plans == combos + 2 * 15 * 2 + 2 * 15 + 2 * 2 * 3 * 2 * 2, "every plan went through the schedule check");
  std::printf("BATCH SCHEDULE OK %llu %llu\n", g_plans, g_passes);
  std::printf("BATCH PLAN OK %llu %llu\n", combos, launches);
  return 0;
}
