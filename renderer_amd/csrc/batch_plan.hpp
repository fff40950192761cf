// batch_plan.hpp — which kernels a batched-draws call launches: a pure function of the entry point, the policy's mode, the
// bucket count, whether matrices are wanted and the census decision (plan_batch), or, for mip_batch_draws_sorted, of the mode,
// the depth metric, depth_bits, whether matrices are wanted and the census decision (plan_batch_sorted); and what every pass
// of a plan reads, writes and launches (batch_pass_io, batch_pass_launch). Plain C++, no HIP: enumerated on the CPU by
// tests/native/batch_plan_check.cpp, batch_views_plan_check.cpp and batch_sorted_plan_check.cpp. api_batch.hip maps a
// BatchKernel to its instantiation and executes the plan with one pass driver.
#pragma once

#include <cstdint>

namespace mip {

constexpr uint32_t kBatchDigitBits = 8;
constexpr uint32_t kBatchMaxPasses = 4;
constexpr uint32_t kBatchDepthBits = 16;  // D's field of the ordered key (batch_lods_kernel.hpp)
static_assert(kBatchMaxPasses * kBatchDigitBits >= 32, "a 32-bit key takes at most kBatchMaxPasses digits");

// mip_batch_draws, mip_batch_draws_lods, mip_batch_draws_ordered (NEAR / FAR), mip_batch_draws_views, mip_batch_draws_shard,
// mip_batch_draws_sorted (planned by plan_batch_sorted, not plan_batch)
enum class BatchEntry : uint32_t { draws, lods, ordered, views, shard, sorted };

// Every instantiation of the stage (batch_kernel.hpp), by key policy. scatter: `mid` = a pass of several, `last` = the one
// pass, ids only, `model` / `general` = the one pass with matrices (census-selected / general arithmetic).
enum class BatchKernel : uint32_t {
  none,
  count_pick, count_chain_distance, count_chain_relative, count_ordered_distance, count_ordered_relative, count_list,
  scatter_pick_mid, scatter_pick_last, scatter_pick_model, scatter_pick_general,
  scatter_chain_distance_mid, scatter_chain_distance_last, scatter_chain_distance_model, scatter_chain_distance_general,
  scatter_chain_relative_mid, scatter_chain_relative_last, scatter_chain_relative_model, scatter_chain_relative_general,
  scatter_ordered_distance_mid, scatter_ordered_relative_mid,
  scatter_list_mid, scatter_list_last,
  model_pick, model_pick_general, model_chain_distance, model_chain_distance_general, model_chain_relative, model_chain_relative_general,
  rowscan, commands_pair, commands_chain,
  // mip_batch_draws_views (batch_views_kernel.hpp): pass 0 over (instance, view) entries, the last list pass that adds the
  // base of the key's view, the command writer that packs per view
  count_views_distance, count_views_relative,
  scatter_views_distance_mid, scatter_views_distance_last, scatter_views_relative_mid, scatter_views_relative_last,
  scatter_views_list_last, commands_views,
  // mip_batch_draws_shard (batch_merge_kernel.hpp): mip_batch_draws_lods' count / rowscan / scatter with the ids going to the
  // chunk; the epilogue that writes the dense bucket counts and the chunk header in the command writer's place
  commands_shard,
  // mip_batch_draws_sorted (batch_sorted_kernel.hpp): pass 0 under the depth key, by LOD mode and depth metric; the sum that
  // gives the list its length in the command writer's place; the run stage behind the last scatter
  count_sorted_distance_radial, count_sorted_distance_axis, count_sorted_relative_radial, count_sorted_relative_axis,
  scatter_sorted_distance_radial_mid, scatter_sorted_distance_axis_mid, scatter_sorted_relative_radial_mid, scatter_sorted_relative_axis_mid,
  sorted_members, run_heads, run_commands, run_counts,
};

struct BatchPlan {
  uint32_t passes;         // digits of the key
  BatchKernel count0;      // pass 0 forms keys from the instance columns; passes 1.. are the list kernels
  BatchKernel scatter0;
  BatchKernel commands;
  BatchKernel model;       // the matrices of a several-pass frame, through slot_of; none when scatter0 stores them or nobody asked
  BatchKernel list_last;   // the last pass of several: scatter_list_last, or the one that knows the views' bases
  constexpr bool several() const { return passes > 1; }
  constexpr BatchKernel count(uint32_t p) const { return p ? BatchKernel::count_list : count0; }
  constexpr BatchKernel scatter(uint32_t p) const { return !p ? scatter0 : p + 1 == passes ? list_last : BatchKernel::scatter_list_mid; }
};

// ceil(log2(buckets)), at least 1: the bits of a bucket
constexpr uint32_t batch_key_bits(unsigned long long buckets) {
  uint32_t bits = 1;
  while ((1ull << bits) < buckets) ++bits;
  return bits;
}

// mip_batch_draws_views sorts n_views x N (instance, view) entries and keeps their number in a 32-bit word.
constexpr bool batch_views_entries_fit(unsigned long long n_views, unsigned long long n) { return n_views * n < (1ull << 32); }

// `relative`: the policy's mode is MIP_LOD_RELATIVE (ignored by mip_batch_draws, which has no policy). buckets >= 1; for
// BatchEntry::views they are the GLOBAL buckets n_views x B (key = view * B + bucket), and no matrices are stored.
// BatchEntry::shard is BatchEntry::lods without matrices and with the chunk epilogue for a command writer.
constexpr BatchPlan plan_batch(BatchEntry entry, bool relative, unsigned long long buckets, bool want_model, bool general) {
  using K = BatchKernel;
  // rows: pick_lod, the chain under DISTANCE, under RELATIVE
  constexpr K scatter[3][4] = {{K::scatter_pick_mid, K::scatter_pick_last, K::scatter_pick_model, K::scatter_pick_general},
                               {K::scatter_chain_distance_mid, K::scatter_chain_distance_last, K::scatter_chain_distance_model, K::scatter_chain_distance_general},
                               {K::scatter_chain_relative_mid, K::scatter_chain_relative_last, K::scatter_chain_relative_model, K::scatter_chain_relative_general}};
  constexpr K count[3] = {K::count_pick, K::count_chain_distance, K::count_chain_relative};
  constexpr K model[3][2] = {{K::model_pick, K::model_pick_general}, {K::model_chain_distance, K::model_chain_distance_general},
                             {K::model_chain_relative, K::model_chain_relative_general}};
  const bool ordered = entry == BatchEntry::ordered;
  const uint32_t bits = (ordered ? kBatchDepthBits : 0u) + batch_key_bits(buckets);  // ordered: always several passes
  const uint32_t row = entry == BatchEntry::draws ? 0u : relative ? 2u : 1u;
  BatchPlan p{};
  p.passes = (bits + kBatchDigitBits - 1u) / kBatchDigitBits;
  p.commands = entry == BatchEntry::draws ? K::commands_pair : entry == BatchEntry::shard ? K::commands_shard : K::commands_chain;
  p.list_last = K::scatter_list_last;
  if (entry == BatchEntry::views) {
    p.count0 = relative ? K::count_views_relative : K::count_views_distance;
    p.scatter0 = p.several() ? (relative ? K::scatter_views_relative_mid : K::scatter_views_distance_mid)
                             : (relative ? K::scatter_views_relative_last : K::scatter_views_distance_last);
    p.commands = K::commands_views;
    p.list_last = K::scatter_views_list_last;
    p.model = K::none;
    return p;
  }
  if (entry == BatchEntry::shard) want_model = false;
  if (ordered) {
    p.count0 = relative ? K::count_ordered_relative : K::count_ordered_distance;
    p.scatter0 = relative ? K::scatter_ordered_relative_mid : K::scatter_ordered_distance_mid;
  } else {
    p.count0 = count[row];
    p.scatter0 = scatter[row][p.several() ? 0 : !want_model ? 1 : general ? 3 : 2];
  }
  // membership does not depend on the order: the ordered path stores matrices with the chain policy's model kernel
  p.model = p.several() && want_model ? model[row][general ? 1 : 0] : K::none;
  return p;
}

// mip_batch_draws_sorted: the key is D alone, depth_bits (16, 24 or 32) wide, so the sort always takes several passes and the
// matrices go through slot_of with the chain policy's model kernel (membership does not depend on the order). `commands` is
// the sum of pass 0's digit totals: no bucket is counted. `axis`: the metric is MIP_DEPTH_VIEW_AXIS, else MIP_DEPTH_RADIAL.
constexpr BatchPlan plan_batch_sorted(bool relative, bool axis, uint32_t depth_bits, bool want_model, bool general) {
  using K = BatchKernel;
  constexpr K count[2][2] = {{K::count_sorted_distance_radial, K::count_sorted_distance_axis},
                             {K::count_sorted_relative_radial, K::count_sorted_relative_axis}};
  constexpr K scatter[2][2] = {{K::scatter_sorted_distance_radial_mid, K::scatter_sorted_distance_axis_mid},
                               {K::scatter_sorted_relative_radial_mid, K::scatter_sorted_relative_axis_mid}};
  BatchPlan p{};
  p.passes = depth_bits / kBatchDigitBits;
  p.count0 = count[relative][axis];
  p.scatter0 = scatter[relative][axis];
  p.commands = K::sorted_members;
  p.list_last = K::scatter_list_last;
  p.model = !want_model ? K::none
            : relative  ? (general ? K::model_chain_relative_general : K::model_chain_relative)
                        : (general ? K::model_chain_distance_general : K::model_chain_distance);
  return p;
}

// What pass p wires up. The (key, instance) lists ping-pong between two buffer pairs: pass p reads the pair pass p - 1 wrote
// and writes the other one; pass 0 forms its keys from the instance columns and the last pass writes the outputs instead.
// `want_model`: the caller gave batch_model (never for views and shards). `with_bucket_hist`: the command writer counts
// buckets, so pass 0 of several accumulates them (every entry but mip_batch_draws_sorted, whose commands come from runs).
struct BatchPassIo {
  int32_t list_in, list_out;  // the buffer pair read / written: 0, 1 or -1 for none
  bool ids;                   // writes instance_ids
  bool slot_of;               // writes the slot map the model kernel reads
  bool model;                 // stores batch_model itself (the single pass)
  bool bucket_hist;           // accumulates the members per bucket
  bool commands;              // the commands kernel runs behind this pass's rowscan
  uint32_t shift, totals_row; // the digit's shift; the row of the digit totals
};
constexpr BatchPassIo batch_pass_io(const BatchPlan& plan, uint32_t p, bool want_model, bool with_bucket_hist) {
  const bool last = p + 1 == plan.passes;
  BatchPassIo io{};
  io.list_in = p ? (int32_t)((p - 1u) & 1u) : -1;
  io.list_out = last ? -1 : (int32_t)(p & 1u);
  io.ids = last;
  io.slot_of = last && plan.several() && want_model;
  io.model = last && !plan.several() && want_model;
  io.bucket_hist = with_bucket_hist && plan.several() && p == 0;
  io.commands = p == 0;
  io.shift = p * kBatchDigitBits;
  io.totals_row = p;
  return io;
}

// The launches of pass p in order, each with the kind of its grid: one workgroup per tile, per bin, or one. kernel == none:
// not launched (the commands kernel of passes 1..).
enum class BatchGrid : uint32_t { tiles, bins, one };
struct BatchLaunch {
  BatchKernel kernel;
  BatchGrid grid;
};
enum : uint32_t { kBatchLaunchCount, kBatchLaunchRowscan, kBatchLaunchCommands, kBatchLaunchScatter, kBatchPassLaunches };
constexpr BatchLaunch batch_pass_launch(const BatchPlan& plan, uint32_t p, uint32_t i) {
  return i == kBatchLaunchCount     ? BatchLaunch{plan.count(p), BatchGrid::tiles}
         : i == kBatchLaunchRowscan ? BatchLaunch{BatchKernel::rowscan, BatchGrid::bins}
         : i == kBatchLaunchCommands ? BatchLaunch{p == 0 ? plan.commands : BatchKernel::none, BatchGrid::one}
                                     : BatchLaunch{plan.scatter(p), BatchGrid::tiles};
}

// The run stage of mip_batch_draws_sorted, in launch order, behind the last scatter (and in front of the model kernel):
// per-tile head counts, their scan over the tiles (one row), the heads' commands, instanceCount of every command.
constexpr uint32_t kBatchRunStageLaunches = 4;
constexpr BatchKernel batch_run_stage(uint32_t i) {
  constexpr BatchKernel k[kBatchRunStageLaunches] = {BatchKernel::run_heads, BatchKernel::rowscan, BatchKernel::run_commands, BatchKernel::run_counts};
  return k[i];
}
constexpr BatchGrid batch_run_stage_grid(uint32_t i) { return batch_run_stage(i) == BatchKernel::rowscan ? BatchGrid::one : BatchGrid::tiles; }
// The list buffer pair whose keys the run stage may overwrite with the slots' buckets: the one the last pass did not read
// (it read pair (passes - 2) & 1, and wrote none).
constexpr uint32_t batch_run_stage_list(const BatchPlan& plan) { return (plan.passes - 1u) & 1u; }

}  // namespace mip
