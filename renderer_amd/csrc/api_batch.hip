// api_batch.hip — C ABI of the instance pipeline, part 6 of 6: batched draws (extension, not reference behaviour).
// mip_batch_draws bins the members of a visibility bitmap by (mesh, LOD) and writes one instanced command per non-empty
// bucket, the entity ids in slot order and, optionally, the members' model matrices in slot order.
// mip_batch_draws_lods does the same over the whole LOD chain, bucket = lod_base[mesh] + lod, with the caller's thresholds.
// mip_batch_draws_ordered is mip_batch_draws_lods with the members of a bucket nearest first or farthest first.
// mip_batch_draws_views is mip_batch_draws_lods for several views in one call: key = view * B + bucket, one shared instance_ids.
// mip_batch_draws_shard is mip_batch_draws_lods for one shard of a sharded scene: ids and dense bucket counts into a chunk;
// mip_merge_batches merges the all-gathered chunks into the bytes of the unsharded call (batch_merge_kernel.hpp).
// mip_batch_draws_sorted sorts the members of mip_batch_draws_lods by depth across buckets (key = D alone) and writes one
// command per run of equal bucket in the sorted slots (batch_sorted_kernel.hpp: the key policy and the run stage).
// One stage (batch_kernel.hpp) under the key policies of the entry points (batch_kernel.hpp, batch_lods_kernel.hpp,
// batch_views_kernel.hpp, batch_sorted_kernel.hpp); batch_plan.hpp says which instantiation a call launches and what every
// pass reads and writes. The kernels are instantiated here and only here. On the host one function fills the argument fields
// every entry shares (fill_common) and one runs the passes of a plan (run_passes) on one scratch type (ensure_scratch);
// batch_draws, batch_draws_sorted and batch_draws_views keep their checks, their early-outs and their own argument fields.
#include "context.hpp"
#include "batch_views_kernel.hpp"
#include "batch_sorted_kernel.hpp"
#include "batch_merge_kernel.hpp"

static_assert(sizeof(MipSortPolicy) == 28, "MipSortPolicy is part of the ABI");
static_assert(sizeof(MipViewBatchOutputs) == 48, "MipViewBatchOutputs is part of the ABI");
static_assert(sizeof(MipBatchChunkHeader) == mip::kBatchChunkHeaderWords * 4 && MIP_MAX_BATCH_CHUNKS == mip::kMaxBatchChunks,
              "the batch chunk: header and kernels agree");
static_assert(MIP_BATCH_CHUNK_IDS_OFFSET(1) == 32 && MIP_BATCH_CHUNK_IDS_OFFSET(4) == 32 && MIP_BATCH_CHUNK_IDS_OFFSET(5) == 48 &&
              MIP_BATCH_CHUNK_IDS_OFFSET(257) == mip::batch_chunk_ids_offset_words(257) * 4 &&
              MIP_BATCH_CHUNK_BYTES(200, 1000) == mip::batch_chunk_bytes(200, 1000), "the batch chunk: header and plan agree");

namespace mip_host {
namespace {

uint32_t batch_tiles_for(uint32_t n) { return (n + mip::kBatchTile - 1u) / mip::kBatchTile; }

// Room in `bs` for a call over `entries` entries: the tile x bin counts and the digit totals always; with `lists` (a call of
// several passes) the two (key, instance) lists and `hist_words` of bucket histogram; the slot map and the bucket map when asked
// for. Every buffer is kept while it is large enough and replaced by a larger one otherwise (grow, context.hpp), in the order
// a slot's scratch always allocated them.
int32_t ensure_scratch(MipContext* ctx, MipContext::BatchScratch& bs, size_t entries, size_t hist_words, bool lists, bool slot_map,
                       bool bucket_map) {
  if (int32_t rc = grow(ctx, &bs.d_counts, &bs.tiles_cap, batch_tiles_for((uint32_t)entries), (size_t)mip::kBatchBins * 4)) return rc;
  if (!bs.d_totals) MIP_HIP(ctx, hipMalloc(&bs.d_totals, (mip::kBatchMaxPasses * mip::kBatchBins + 1) * 4));
  if (lists && (!bs.d_ids[1] || entries > bs.list_cap)) {  // the four hold the same number of entries: replaced together
    bs.list_cap = 0;
    for (uint32_t** list : {&bs.d_keys[0], &bs.d_ids[0], &bs.d_keys[1], &bs.d_ids[1]}) {
      size_t none = 0;
      if (int32_t rc = grow(ctx, list, &none, entries, 4)) return rc;
    }
    bs.list_cap = entries;
  }
  if (lists)
    if (int32_t rc = grow(ctx, &bs.d_bucket_hist, &bs.hist_cap, hist_words, 4)) return rc;
  if (slot_map)
    if (int32_t rc = grow(ctx, &bs.d_slot_of, &bs.slot_cap, entries, 4)) return rc;
  if (bucket_map)
    if (int32_t rc = grow(ctx, &bs.d_bucket_of, &bs.bucket_cap, entries, 4)) return rc;
  return MIP_OK;
}

// The scratch of frame slot `slot`, asked for the context's capacities: every buffer is allocated once, at first need.
int32_t slot_scratch(MipContext* ctx, uint32_t slot, bool lists, bool slot_map, bool bucket_map, MipContext::BatchScratch*& bs) {
  if (ctx->batch.size() != ctx->slots.size()) ctx->batch.resize(ctx->slots.size());
  bs = &ctx->batch[slot];
  return ensure_scratch(ctx, *bs, instance_cap(ctx), (size_t)(ctx->max_meshes ? ctx->max_meshes : 1) * MIP_MAX_LODS, lists, slot_map, bucket_map);
}

void release_scratch(MipContext::BatchScratch& bs) {
  for (uint32_t* p : {bs.d_counts, bs.d_totals, bs.d_keys[0], bs.d_ids[0], bs.d_keys[1], bs.d_ids[1], bs.d_bucket_hist, bs.d_slot_of, bs.d_bucket_of})
    (void)hipFree(p);
  bs = MipContext::BatchScratch{};
}

// The instantiation behind every name of the plan (batch_plan.hpp).
const void* kernel_address(mip::BatchKernel k) {
  using namespace mip;
  using K = BatchKernel;
  using ChainD = BatchLodChainKey<MIP_LOD_DISTANCE>;
  using ChainR = BatchLodChainKey<MIP_LOD_RELATIVE>;
  using OrderedD = BatchOrderedKey<MIP_LOD_DISTANCE>;
  using OrderedR = BatchOrderedKey<MIP_LOD_RELATIVE>;
  using ViewsD = BatchViewsKey<MIP_LOD_DISTANCE>;
  using ViewsR = BatchViewsKey<MIP_LOD_RELATIVE>;
  switch (k) {
    case K::none: break;
    case K::count_pick: return (const void*)mip_batch_count_kernel<BatchPickLodKey>;
    case K::count_chain_distance: return (const void*)mip_batch_count_kernel<ChainD>;
    case K::count_chain_relative: return (const void*)mip_batch_count_kernel<ChainR>;
    case K::count_ordered_distance: return (const void*)mip_batch_count_kernel<OrderedD>;
    case K::count_ordered_relative: return (const void*)mip_batch_count_kernel<OrderedR>;
    case K::count_list: return (const void*)mip_batch_count_kernel<BatchListKey>;
    case K::scatter_pick_mid: return (const void*)mip_batch_scatter_kernel<BatchPickLodKey, false, 0>;
    case K::scatter_pick_last: return (const void*)mip_batch_scatter_kernel<BatchPickLodKey, true, 0>;
    case K::scatter_pick_model: return (const void*)mip_batch_scatter_kernel<BatchPickLodKey, true, 1>;
    case K::scatter_pick_general: return (const void*)mip_batch_scatter_kernel<BatchPickLodKey, true, 2>;
    case K::scatter_chain_distance_mid: return (const void*)mip_batch_scatter_kernel<ChainD, false, 0>;
    case K::scatter_chain_distance_last: return (const void*)mip_batch_scatter_kernel<ChainD, true, 0>;
    case K::scatter_chain_distance_model: return (const void*)mip_batch_scatter_kernel<ChainD, true, 1>;
    case K::scatter_chain_distance_general: return (const void*)mip_batch_scatter_kernel<ChainD, true, 2>;
    case K::scatter_chain_relative_mid: return (const void*)mip_batch_scatter_kernel<ChainR, false, 0>;
    case K::scatter_chain_relative_last: return (const void*)mip_batch_scatter_kernel<ChainR, true, 0>;
    case K::scatter_chain_relative_model: return (const void*)mip_batch_scatter_kernel<ChainR, true, 1>;
    case K::scatter_chain_relative_general: return (const void*)mip_batch_scatter_kernel<ChainR, true, 2>;
    case K::scatter_ordered_distance_mid: return (const void*)mip_batch_scatter_kernel<OrderedD, false, 0>;
    case K::scatter_ordered_relative_mid: return (const void*)mip_batch_scatter_kernel<OrderedR, false, 0>;
    case K::scatter_list_mid: return (const void*)mip_batch_scatter_kernel<BatchListKey, false, 0>;
    case K::scatter_list_last: return (const void*)mip_batch_scatter_kernel<BatchListKey, true, 0>;
    case K::model_pick: return (const void*)mip_batch_model_kernel<BatchPickLodKey, false>;
    case K::model_pick_general: return (const void*)mip_batch_model_kernel<BatchPickLodKey, true>;
    case K::model_chain_distance: return (const void*)mip_batch_model_kernel<ChainD, false>;
    case K::model_chain_distance_general: return (const void*)mip_batch_model_kernel<ChainD, true>;
    case K::model_chain_relative: return (const void*)mip_batch_model_kernel<ChainR, false>;
    case K::model_chain_relative_general: return (const void*)mip_batch_model_kernel<ChainR, true>;
    case K::rowscan: return (const void*)mip_batch_rowscan_kernel;
    case K::commands_pair: return (const void*)mip_batch_commands_kernel<BatchPairDraw>;
    case K::commands_chain: return (const void*)mip_batch_commands_kernel<BatchChainDraw>;
    case K::count_views_distance: return (const void*)mip_batch_count_kernel<ViewsD>;
    case K::count_views_relative: return (const void*)mip_batch_count_kernel<ViewsR>;
    case K::scatter_views_distance_mid: return (const void*)mip_batch_scatter_kernel<ViewsD, false, 0>;
    case K::scatter_views_distance_last: return (const void*)mip_batch_scatter_kernel<ViewsD, true, 0>;
    case K::scatter_views_relative_mid: return (const void*)mip_batch_scatter_kernel<ViewsR, false, 0>;
    case K::scatter_views_relative_last: return (const void*)mip_batch_scatter_kernel<ViewsR, true, 0>;
    case K::scatter_views_list_last: return (const void*)mip_batch_scatter_kernel<BatchViewsListKey, true, 0>;
    case K::commands_views: return (const void*)mip_batch_view_commands_kernel;
    case K::commands_shard: return (const void*)mip_batch_shard_chunk_kernel;
    case K::count_sorted_distance_radial: return (const void*)mip_batch_count_kernel<BatchSortedKey<MIP_LOD_DISTANCE, MIP_DEPTH_RADIAL>>;
    case K::count_sorted_distance_axis: return (const void*)mip_batch_count_kernel<BatchSortedKey<MIP_LOD_DISTANCE, MIP_DEPTH_VIEW_AXIS>>;
    case K::count_sorted_relative_radial: return (const void*)mip_batch_count_kernel<BatchSortedKey<MIP_LOD_RELATIVE, MIP_DEPTH_RADIAL>>;
    case K::count_sorted_relative_axis: return (const void*)mip_batch_count_kernel<BatchSortedKey<MIP_LOD_RELATIVE, MIP_DEPTH_VIEW_AXIS>>;
    case K::scatter_sorted_distance_radial_mid: return (const void*)mip_batch_scatter_kernel<BatchSortedKey<MIP_LOD_DISTANCE, MIP_DEPTH_RADIAL>, false, 0>;
    case K::scatter_sorted_distance_axis_mid: return (const void*)mip_batch_scatter_kernel<BatchSortedKey<MIP_LOD_DISTANCE, MIP_DEPTH_VIEW_AXIS>, false, 0>;
    case K::scatter_sorted_relative_radial_mid: return (const void*)mip_batch_scatter_kernel<BatchSortedKey<MIP_LOD_RELATIVE, MIP_DEPTH_RADIAL>, false, 0>;
    case K::scatter_sorted_relative_axis_mid: return (const void*)mip_batch_scatter_kernel<BatchSortedKey<MIP_LOD_RELATIVE, MIP_DEPTH_VIEW_AXIS>, false, 0>;
    case K::sorted_members: return (const void*)mip_batch_sorted_members_kernel;
    case K::run_heads: return (const void*)mip_batch_run_heads_kernel;
    case K::run_commands: return (const void*)mip_batch_run_commands_kernel;
    case K::run_counts: return (const void*)mip_batch_run_counts_kernel;
  }
  return nullptr;
}

// `a` is the most derived argument block (OrderedBatchArgs, or ViewBatchArgs for mip_batch_draws_views); every kernel takes
// its own leading part of it (BatchArgs, LodBatchArgs or all of it)
int32_t launch(MipContext* ctx, mip::BatchKernel kernel, uint32_t blocks, hipStream_t stream, mip::LodBatchArgs& a) {
  void* params[] = {&a};
  MIP_HIP(ctx, hipLaunchKernel(kernel_address(kernel), dim3(blocks), dim3(mip::kTile), params, 0, stream));
  MIP_HIP(ctx, hipGetLastError());
  return MIP_OK;
}

uint32_t grid_blocks(mip::BatchGrid grid, const mip::BatchArgs& a) {
  return grid == mip::BatchGrid::tiles ? a.n_tiles : grid == mip::BatchGrid::bins ? a.n_bins : 1u;
}

// The fields every entry point fills the same way, into a zeroed block: the resident columns and tables, the chain under a
// policy, the tile count of `entries`, n_bins, the scratch words and the command and count outputs. frame / bitmap are null
// for mip_batch_draws_views, whose kernels take a camera, a base and a bitmap per view.
void fill_common(MipContext* ctx, mip::LodBatchArgs& a, const MipContext::BatchScratch& bs, const mip::BatchPlan& plan,
                 const MipLodPolicy* policy, const MipFrame* frame, const uint32_t* bitmap, uint32_t entries, unsigned long long buckets,
                 void* batch_cmds, uint32_t* batch_count, uint32_t* instance_count) {
  if (policy) {
    a.chain = ctx->d_mesh_chain;
    a.bucket_lod = ctx->d_bucket_lod;
    std::memcpy(a.switch_sq, policy->switch_sq, sizeof a.switch_sq);
  }
  a.pos = ctx->d_pos; a.rot = ctx->d_rot; a.scale = ctx->d_scale; a.mesh_id = ctx->d_mesh_id;
  a.meshes = ctx->d_meshes; a.mesh_draw = ctx->d_mesh_draw;
  a.bitmap = bitmap;
  a.n = ctx->n;
  a.n_tiles = batch_tiles_for(entries);
  a.n_buckets = (uint32_t)buckets;
  a.n_bins = plan.several() ? mip::kBatchBins : (uint32_t)buckets;
  if (frame) {
    a.first_instance_base = frame->first_instance_base;
    std::memcpy(a.cam, frame->cam_pos, sizeof a.cam);
  }
  a.counts = bs.d_counts;
  a.members = a.members_out = bs.d_totals + mip::kBatchMaxPasses * mip::kBatchBins;
  a.batch_cmds = static_cast<uint32_t*>(batch_cmds);
  a.batch_count = batch_count;
  a.instance_count = instance_count;
#ifdef MIP_DEBUG_STAMPS
  DebugSwitches().tile_order(a.n_tiles, a.debug_tile_mult, a.debug_tile_add);  // as fill_kernel_args (api_frame.hip) permutes the frame's tiles
#endif
}

// The radix passes of `plan` over the block fill_common filled, wired as batch_pass_io says and launched as batch_pass_launch
// says. `a` is the leading part of the caller's most derived block, as launch() takes it. with_bucket_hist: the command
// writer counts buckets, in hist_words words of bs.d_bucket_hist (cleared here); not so for mip_batch_draws_sorted.
// around_count(p, before) runs in front of and behind the count launch of pass p: the caller's own fields of that launch.
template <class AroundCount>
int32_t run_passes(MipContext* ctx, const mip::BatchPlan& plan, const MipContext::BatchScratch& bs, bool with_bucket_hist, size_t hist_words,
                   uint32_t* instance_ids, void* batch_model, hipStream_t stream, mip::LodBatchArgs& a, AroundCount around_count) {
  const bool several = plan.several();
  if (several && with_bucket_hist) MIP_HIP(ctx, hipMemsetAsync(bs.d_bucket_hist, 0, hist_words * 4, stream));
  for (uint32_t p = 0; p < plan.passes; ++p) {
    const mip::BatchPassIo io = mip::batch_pass_io(plan, p, batch_model != nullptr, with_bucket_hist);
    a.shift = io.shift;
    a.totals = bs.d_totals + io.totals_row * mip::kBatchBins;
    a.bucket_hist = io.bucket_hist ? bs.d_bucket_hist : nullptr;
    a.keys_in = io.list_in < 0 ? nullptr : bs.d_keys[io.list_in];
    a.ids_in = io.list_in < 0 ? nullptr : bs.d_ids[io.list_in];
    a.keys_out = io.list_out < 0 ? nullptr : bs.d_keys[io.list_out];
    a.ids_out = io.list_out < 0 ? nullptr : bs.d_ids[io.list_out];
    a.instance_ids = io.ids ? instance_ids : nullptr;
    a.slot_of = io.slot_of ? bs.d_slot_of : nullptr;
    a.batch_model = io.model ? static_cast<float4*>(batch_model) : nullptr;
    auto step = [&](uint32_t i) {
      const mip::BatchLaunch l = mip::batch_pass_launch(plan, p, i);
      return launch(ctx, l.kernel, grid_blocks(l.grid, a), stream, a);
    };
    around_count(p, true);
    if (int32_t rc = step(mip::kBatchLaunchCount)) return rc;
    around_count(p, false);
    if (int32_t rc = step(mip::kBatchLaunchRowscan)) return rc;
    if (io.commands) {  // the scan's epilogue: bucket totals -> commands and counts (and the list's length for later passes)
      a.bucket_totals = !several ? a.totals : with_bucket_hist ? bs.d_bucket_hist : nullptr;
      if (int32_t rc = step(mip::kBatchLaunchCommands)) return rc;
    }
    if (int32_t rc = step(mip::kBatchLaunchScatter)) return rc;
  }
  return MIP_OK;
}

// The matrices of a several-pass call, through slot_of, behind everything else.
int32_t store_models(MipContext* ctx, const mip::BatchPlan& plan, void* batch_model, hipStream_t stream, mip::LodBatchArgs& a) {
  if (plan.model == mip::BatchKernel::none) return MIP_OK;
  a.batch_model = static_cast<float4*>(batch_model);
  return launch(ctx, plan.model, a.n_tiles, stream, a);
}

}  // namespace

void batch_release(MipContext* ctx) {
  for (auto& bs : ctx->batch) release_scratch(bs);
  ctx->batch.clear();
  release_scratch(ctx->view_batch);
  (void)hipFree(ctx->batch_merge.d_words);
  ctx->batch_merge = MipContext::BatchMergeScratch{};
}

namespace {

// The checks the output structs of the family share, in the order every entry point makes them, with the texts of each entry
// point. The alignment rules differ per entry and stay with it.
struct OutputTexts {
  const char *type, *needs_device, *null_outputs;
};
constexpr OutputTexts kDrawsTexts{"MipBatchOutputs", "mip_batch_draws needs MIP_OUT_DEVICE outputs", "batch_cmds/batch_count/instance_ids is NULL"};
constexpr OutputTexts kMergeTexts{"MipBatchOutputs", "mip_merge_batches needs MIP_OUT_DEVICE outputs", "batch_cmds/batch_count/instance_ids is NULL"};
constexpr OutputTexts kViewsTexts{"MipViewBatchOutputs", "mip_batch_draws_views needs MIP_OUT_DEVICE outputs", "batch_cmds/batch_counts/instance_ids is NULL"};
uint32_t reserved_of(const MipBatchOutputs&) { return 0u; }  // (no such field)
uint32_t reserved_of(const MipViewBatchOutputs& out) { return out.reserved; }
const uint32_t* counts_of(const MipBatchOutputs& out) { return out.batch_count; }
const uint32_t* counts_of(const MipViewBatchOutputs& out) { return out.batch_counts; }

template <class Out>
int32_t check_outputs(MipContext* ctx, const Out* out, const OutputTexts& texts) {
  if (out->struct_size != sizeof(Out)) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "%s.struct_size %u != %zu", texts.type, out->struct_size, sizeof(Out));
  if (reserved_of(*out) != 0u) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "%s.reserved is %u, not 0", texts.type, reserved_of(*out));
  if (out->flags & ~(MIP_OUT_DEVICE | MIP_OUT_ASYNC)) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "unknown %s flags 0x%x", texts.type, out->flags);
  if (!(out->flags & MIP_OUT_DEVICE)) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "%s", texts.needs_device);
  if (!out->batch_cmds || !counts_of(*out) || !out->instance_ids) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "%s", texts.null_outputs);
  return MIP_OK;
}

// The argument checks the entry points behind a frame share, and the context's device made current.
int32_t check_call(MipContext* ctx, const MipFrame* frame, const uint32_t* visible_bitmap, const MipBatchOutputs* out) {
  if (!frame || !visible_bitmap || !out) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "frame/visible_bitmap/out is NULL");
  if (int32_t rc = check_outputs(ctx, out, kDrawsTexts)) return rc;
  if ((uintptr_t)out->batch_cmds % 4u != 0u || (uintptr_t)out->batch_model % 16u != 0u)
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "batch_cmds / batch_model is not aligned (4 / 16 bytes)");
  if (!ctx->have_instances || !ctx->have_meshes) return fail(ctx, MIP_ERR_NOT_READY, "instances or mesh table not set");
  if (int32_t rc = bind_device(ctx)) return rc;
  return MIP_OK;
}

// The four entry points. policy == null: mip_batch_draws (pick_lod, bucket = mesh * 2 + lod); else the whole LOD chain, in
// draw order (MIP_BATCH_ORDER_DRAW_INDEX: mip_batch_draws_lods) or by key = bucket << 16 | D (NEAR_FIRST / FAR_FIRST).
// shard_chunk != null: mip_batch_draws_shard — mip_batch_draws_lods with the ids going to the chunk (out->instance_ids points
// at them, out->batch_cmds / batch_count are not written) and the chunk epilogue in the command writer's place.
int32_t batch_draws(MipContext* ctx, const MipFrame* frame, const uint32_t* visible_bitmap, const MipLodPolicy* policy, uint32_t order,
                    const MipBatchOutputs* out, uint32_t* shard_chunk = nullptr, uint32_t shard_ids_capacity = 0) {
  using mip::BatchEntry;
  if (int32_t rc = check_call(ctx, frame, visible_bitmap, out)) return rc;
  if (shard_chunk && shard_ids_capacity < ctx->n)
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "ids_capacity %u < %u resident instances", shard_ids_capacity, ctx->n);
  // behind the frame issued last: a bitmap that frame writes is ordered before these launches without a wait
  const uint32_t slot = ctx->last_slot;
  hipStream_t stream = ctx->slots[slot].stream;
  const uint32_t n = ctx->n;
  const BatchEntry entry = shard_chunk ? BatchEntry::shard
                           : !policy   ? BatchEntry::draws
                                       : order == MIP_BATCH_ORDER_DRAW_INDEX ? BatchEntry::lods : BatchEntry::ordered;
  const unsigned long long buckets = policy ? ctx->lod_buckets : 2ull * ctx->m;
  if (entry == BatchEntry::ordered) {
    if (buckets > mip::kBatchOrderedMaxBuckets)
      return fail(ctx, MIP_ERR_CAPACITY, "%llu buckets: bucket << 16 | depth does not fit a 32-bit key (at most %u)", buckets, mip::kBatchOrderedMaxBuckets);
  } else if (buckets > 0x80000000ull || (policy && ctx->m > 0x20000000u)) {
    return fail(ctx, MIP_ERR_CAPACITY, "%u meshes, %llu buckets: a bucket does not fit a 32-bit key", ctx->m, buckets);
  }

  if (shard_chunk && (n == 0 || buckets == 0)) {  // nothing to bin: the header and B zeros
    mip::ShardBatchArgs z{};
    z.chunk = shard_chunk;
    z.n_buckets = (uint32_t)buckets;
    if (int32_t rc = launch(ctx, mip::BatchKernel::commands_shard, 1, stream, z)) return rc;
    return finish(ctx, stream, (out->flags & MIP_OUT_ASYNC) != 0);
  }
  if (n == 0 || buckets == 0) {  // nothing to bin: two zeros
    MIP_HIP(ctx, hipMemsetAsync(out->batch_count, 0, 4, stream));
    if (out->instance_count) MIP_HIP(ctx, hipMemsetAsync(out->instance_count, 0, 4, stream));
    return finish(ctx, stream, (out->flags & MIP_OUT_ASYNC) != 0);
  }
  // the arithmetic mip_run's `model` comes from: the census decides (frame_plan.hpp, LaunchPlan.general)
  const bool general = ctx->nonfinite_instances != 0 || ctx->force_general;
  const mip::BatchPlan plan = mip::plan_batch(entry, policy && policy->mode == MIP_LOD_RELATIVE, buckets, out->batch_model != nullptr, general);
  MipContext::BatchScratch* bs = nullptr;
  if (int32_t rc = slot_scratch(ctx, slot, plan.several(), plan.several() && out->batch_model, false, bs)) return rc;

  mip::ShardBatchArgs a{};  // the most derived block: every kernel takes its own leading part
  fill_common(ctx, a, *bs, plan, policy, frame, visible_bitmap, n, buckets, out->batch_cmds, out->batch_count, out->instance_count);
  a.chunk = shard_chunk;
  a.depth_flip = order == MIP_BATCH_ORDER_FAR_FIRST ? mip::kBatchDepthMax : 0u;
  if (int32_t rc = run_passes(ctx, plan, *bs, true, (size_t)buckets, out->instance_ids, out->batch_model, stream, a, [](uint32_t, bool) {})) return rc;
  if (int32_t rc = store_models(ctx, plan, out->batch_model, stream, a)) return rc;
  return finish(ctx, stream, (out->flags & MIP_OUT_ASYNC) != 0);
}

}  // namespace

// MipLodPolicy as the header states it (mip_cull_clusters, api_cluster.hip, takes the same policies)
int32_t check_policy(MipContext* ctx, const MipLodPolicy* policy) {
  if (!policy) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "policy is NULL");
  if (policy->struct_size != sizeof(MipLodPolicy))
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "MipLodPolicy.struct_size %u != %zu", policy->struct_size, sizeof(MipLodPolicy));
  if (policy->mode != MIP_LOD_DISTANCE && policy->mode != MIP_LOD_RELATIVE)
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "unknown MipLodPolicy.mode %u", policy->mode);
  for (uint32_t k = 0; k + 1u < MIP_MAX_LODS; ++k) {
    const float t = policy->switch_sq[k];
    if (!(t >= 0.0f)) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "switch_sq[%u] = %g is negative or NaN", k, (double)t);
    if (k && t < policy->switch_sq[k - 1]) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "switch_sq[%u] = %g decreases", k, (double)t);
  }
  return MIP_OK;
}

namespace {

// MipSortPolicy as the header states it
int32_t check_sort(MipContext* ctx, const MipSortPolicy* sort) {
  if (!sort) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "sort is NULL");
  if (sort->struct_size != sizeof(MipSortPolicy))
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "MipSortPolicy.struct_size %u != %zu", sort->struct_size, sizeof(MipSortPolicy));
  if (sort->metric != MIP_DEPTH_RADIAL && sort->metric != MIP_DEPTH_VIEW_AXIS)
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "unknown MipSortPolicy.metric %u", sort->metric);
  if (sort->order != MIP_BATCH_ORDER_NEAR_FIRST && sort->order != MIP_BATCH_ORDER_FAR_FIRST)
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "MipSortPolicy.order %u is neither NEAR_FIRST nor FAR_FIRST", sort->order);
  if (sort->depth_bits != 16u && sort->depth_bits != 24u && sort->depth_bits != 32u)
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "MipSortPolicy.depth_bits %u is not 16, 24 or 32", sort->depth_bits);
  if (sort->metric == MIP_DEPTH_VIEW_AXIS)
    for (uint32_t k = 0; k < 3; ++k)
      if (!std::isfinite(sort->axis[k])) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "MipSortPolicy.axis[%u] = %g is not finite", k, (double)sort->axis[k]);
  return MIP_OK;
}

// mip_batch_draws_sorted: the stage of batch_draws() under BatchSortedKey — depth_bits / 8 passes over D alone, the members sum
// in the command writer's place — then the run stage over the final slots, then the matrices through slot_of.
int32_t batch_draws_sorted(MipContext* ctx, const MipFrame* frame, const uint32_t* visible_bitmap, const MipLodPolicy* policy,
                           const MipSortPolicy* sort, const MipBatchOutputs* out) {
  if (int32_t rc = check_call(ctx, frame, visible_bitmap, out)) return rc;
  const uint32_t slot = ctx->last_slot;
  hipStream_t stream = ctx->slots[slot].stream;
  const uint32_t n = ctx->n;
  const unsigned long long buckets = ctx->lod_buckets;
  if (buckets > 0x80000000ull || ctx->m > 0x20000000u)
    return fail(ctx, MIP_ERR_CAPACITY, "%u meshes, %llu buckets: a bucket does not fit a 32-bit word", ctx->m, buckets);
  const bool async = (out->flags & MIP_OUT_ASYNC) != 0;
  if (n == 0 || buckets == 0) {  // nothing to sort: two zeros
    MIP_HIP(ctx, hipMemsetAsync(out->batch_count, 0, 4, stream));
    if (out->instance_count) MIP_HIP(ctx, hipMemsetAsync(out->instance_count, 0, 4, stream));
    return finish(ctx, stream, async);
  }
  const bool general = ctx->nonfinite_instances != 0 || ctx->force_general;
  const bool axis = sort->metric == MIP_DEPTH_VIEW_AXIS;
  const mip::BatchPlan plan = mip::plan_batch_sorted(policy->mode == MIP_LOD_RELATIVE, axis, sort->depth_bits, out->batch_model != nullptr, general);
  MipContext::BatchScratch* bs = nullptr;
  if (int32_t rc = slot_scratch(ctx, slot, true, out->batch_model != nullptr, true, bs)) return rc;

  mip::SortedBatchArgs a{};
  fill_common(ctx, a, *bs, plan, policy, frame, visible_bitmap, n, buckets, out->batch_cmds, out->batch_count, out->instance_count);
  a.depth_shift = 32u - sort->depth_bits;
  a.depth_flip = sort->order == MIP_BATCH_ORDER_FAR_FIRST ? (axis ? mip::kSortedUmaxAxis : mip::kSortedUmaxRadial) >> a.depth_shift : 0u;
  if (axis) std::memcpy(a.axis, sort->axis, sizeof a.axis);
  // the count of pass 0 stores the buckets; no other launch stores them again
  auto bucket_out = [&](uint32_t p, bool before) { a.bucket_out = (before && p == 0) ? bs->d_bucket_of : nullptr; };
  if (int32_t rc = run_passes(ctx, plan, *bs, false, 0, out->instance_ids, out->batch_model, stream, a, bucket_out)) return rc;
  // the run stage: the tile rows reuse `counts` (row 0), the slots' buckets the list buffer batch_plan.hpp frees for them, and the
  // row's sum — the number of heads — is batch_count
  a.bucket_in = bs->d_bucket_of;
  a.slot_bucket = bs->d_keys[mip::batch_run_stage_list(plan)];
  a.totals = out->batch_count;
  for (uint32_t k = 0; k < mip::kBatchRunStageLaunches; ++k)
    if (int32_t rc = launch(ctx, mip::batch_run_stage(k), grid_blocks(mip::batch_run_stage_grid(k), a), stream, a)) return rc;
  if (int32_t rc = store_models(ctx, plan, out->batch_model, stream, a)) return rc;
  return finish(ctx, stream, async);
}

// mip_batch_draws_views: every check first (a refused call writes nothing), then one sort of the n_views x N (instance, view)
// entries by key = view * B + bucket on the context's first stream, where mip_run_views runs.
int32_t batch_draws_views(MipContext* ctx, const MipFrame* frames, const uint32_t* const* visible_bitmaps, uint32_t n_views,
                          const MipLodPolicy* policy, const MipViewBatchOutputs* out) {
  if (!frames || !visible_bitmaps || !out) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "frames/visible_bitmaps/out is NULL");
  if (int32_t rc = check_outputs(ctx, out, kViewsTexts)) return rc;
  if ((uintptr_t)out->batch_cmds % 4u != 0u) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "batch_cmds is not 4-byte aligned");
  if (n_views == 0 || n_views > MIP_MAX_VIEWS) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "n_views %u outside 1..%u", n_views, (unsigned)MIP_MAX_VIEWS);
  if (!ctx->have_instances || !ctx->have_meshes) return fail(ctx, MIP_ERR_NOT_READY, "instances or mesh table not set");
  const uint32_t n = ctx->n;
  const unsigned long long view_buckets = ctx->lod_buckets, buckets = view_buckets * n_views;
  if (out->cmd_stride < (view_buckets < n ? view_buckets : n))
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "cmd_stride %u < min(B = %llu, N = %u)", out->cmd_stride, view_buckets, n);
  if (!mip::batch_views_entries_fit(n_views, n))
    return fail(ctx, MIP_ERR_CAPACITY, "%u views x %u instances: the entries do not fit a 32-bit count", n_views, n);
  if (buckets > 0x80000000ull || ctx->m > 0x20000000u)
    return fail(ctx, MIP_ERR_CAPACITY, "%u views x %llu buckets: view * B + bucket does not fit a 32-bit key", n_views, view_buckets);
  if (int32_t rc = bind_device(ctx)) return rc;
  hipStream_t stream = ctx->stream;
  const bool async = (out->flags & MIP_OUT_ASYNC) != 0;

  if (n == 0 || view_buckets == 0) {  // nothing to bin: zeros
    MIP_HIP(ctx, hipMemsetAsync(out->batch_counts, 0, (size_t)n_views * 4, stream));
    if (out->view_first_slot) MIP_HIP(ctx, hipMemsetAsync(out->view_first_slot, 0, ((size_t)n_views + 1) * 4, stream));
    return finish(ctx, stream, async);
  }
  const mip::BatchPlan plan = mip::plan_batch(mip::BatchEntry::views, policy->mode == MIP_LOD_RELATIVE, buckets, false, false);
  const bool several = plan.several();
  const uint32_t entries = n_views * n;
  // several passes: copies of the bucket histogram, so that concurrent tiles add to different cache lines; at most 2^20 words
  uint32_t hist_copies = several ? 64u : 1u;
  while (hist_copies > 1u && hist_copies * buckets > (1ull << 20)) hist_copies >>= 1;
  const size_t hist_words = (size_t)hist_copies * (size_t)buckets;
  MipContext::BatchScratch& vs = ctx->view_batch;
  if (int32_t rc = ensure_scratch(ctx, vs, entries, hist_words, several, false, false)) return rc;

  mip::ViewBatchArgs a{};
  fill_common(ctx, a, vs, plan, policy, nullptr, nullptr, entries, buckets, out->batch_cmds, nullptr, nullptr);
  a.n_views = n_views;
  a.view_buckets = (uint32_t)view_buckets;
  a.n_entries = entries;
  a.cmd_stride = out->cmd_stride;
  a.hist_copies = hist_copies;
  for (uint32_t v = 0; v < n_views; ++v) {
    a.view_bitmap[v] = visible_bitmaps[v];
    std::memcpy(a.view_cam[v], frames[v].cam_pos, sizeof a.view_cam[v]);
    a.view_base[v] = frames[v].first_instance_base;
  }
  a.batch_counts = out->batch_counts;
  a.view_first_slot = out->view_first_slot;
  if (int32_t rc = run_passes(ctx, plan, vs, true, hist_words, out->instance_ids, nullptr, stream, a, [](uint32_t, bool) {})) return rc;
  return finish(ctx, stream, async);
}

// mip_merge_batches: every check first (a refused call writes nothing), then the offsets kernel and the gather on the
// context's first stream, where the other merges run.
int32_t merge_batches(MipContext* ctx, const void* chunks, uint32_t n_chunks, uint64_t stride, uint32_t capacity, const MipBatchOutputs* out) {
  if (!chunks || !out) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "chunks/out is NULL");
  if (int32_t rc = check_outputs(ctx, out, kMergeTexts)) return rc;
  if (out->batch_model) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "mip_merge_batches does not merge matrices: batch_model must be NULL");
  if ((uintptr_t)out->batch_cmds % 4u != 0u || (uintptr_t)out->instance_ids % 4u != 0u || (uintptr_t)out->batch_count % 4u != 0u ||
      (uintptr_t)out->instance_count % 4u != 0u)
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "an output is not 4-byte aligned");
  if ((uintptr_t)chunks % 16u != 0u) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "batch chunks must be 16-byte aligned");
  if (n_chunks == 0 || n_chunks > MIP_MAX_BATCH_CHUNKS)
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "n_chunks %u outside 1..%u", n_chunks, (unsigned)MIP_MAX_BATCH_CHUNKS);
  if (!ctx->have_meshes) return fail(ctx, MIP_ERR_NOT_READY, "the chunks are merged against the mesh table: set it first");
  const unsigned long long buckets = ctx->lod_buckets;
  if (stride % 16u != 0u || stride < MIP_BATCH_CHUNK_BYTES(buckets, capacity))
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "a chunk of %llu buckets and %u ids takes %llu bytes: the stride of %llu is smaller, or no multiple of 16",
                buckets, capacity, (unsigned long long)MIP_BATCH_CHUNK_BYTES(buckets, capacity), (unsigned long long)stride);
  if (!mip::batch_merge_table_fits(n_chunks, buckets))
    return fail(ctx, MIP_ERR_CAPACITY, "%u chunks x %llu buckets: the offsets table takes at most 2^24 counts", n_chunks, buckets);
  if (!mip::batch_merge_slots_fit(n_chunks, capacity))
    return fail(ctx, MIP_ERR_CAPACITY, "%u chunks x %u ids: the merged list does not fit a 32-bit count", n_chunks, capacity);
  if (int32_t rc = bind_device(ctx)) return rc;
  hipStream_t stream = ctx->stream;

  const mip::BatchMergePlan plan = mip::plan_batch_merge(n_chunks, buckets, capacity);
  MipContext::BatchMergeScratch& ms = ctx->batch_merge;
  if (int32_t rc = grow(ctx, &ms.d_words, &ms.words_cap, (size_t)plan.scratch_words, 4)) return rc;
  mip::BatchMergeArgs a{};
  a.chunks = static_cast<const unsigned char*>(chunks);
  a.stride = stride;
  a.n_chunks = n_chunks;
  a.n_buckets = (uint32_t)buckets;
  a.capacity = capacity;
  a.ids_offset_words = (uint32_t)mip::batch_chunk_ids_offset_words(buckets);
  a.chain = ctx->d_mesh_chain;
  a.bucket_lod = ctx->d_bucket_lod;
  a.mesh_draw = ctx->d_mesh_draw;
  a.head = ms.d_words;
  a.src_start = ms.d_words + plan.src_start;
  a.seg_dst = ms.d_words + plan.seg_dst;
  a.seg_src = ms.d_words + plan.seg_src;
  a.seg_rank = ms.d_words + plan.seg_rank;
  a.batch_cmds = static_cast<uint32_t*>(out->batch_cmds);
  a.batch_count = out->batch_count;
  a.instance_count = out->instance_count;
  a.instance_ids = out->instance_ids;
  a.error_flag = ctx->d_error;
  hipLaunchKernelGGL(mip::mip_batch_merge_offsets_kernel, dim3(1), dim3(mip::kBatchMergeThreads), 0, stream, a);
  MIP_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(mip::mip_batch_merge_gather_kernel, dim3(plan.gather_blocks), dim3(mip::kBatchMergeThreads), 0, stream, a);
  MIP_HIP(ctx, hipGetLastError());
  return finish(ctx, stream, (out->flags & MIP_OUT_ASYNC) != 0);
}

}  // namespace
}  // namespace mip_host

using namespace mip_host;

extern "C" {

int32_t mip_batch_draws(MipContext* ctx, const MipFrame* frame, const uint32_t* visible_bitmap, const MipBatchOutputs* out) {
  if (!ctx) return MIP_ERR_INVALID_ARGUMENT;
  return batch_draws(ctx, frame, visible_bitmap, nullptr, MIP_BATCH_ORDER_DRAW_INDEX, out);
}

int32_t mip_batch_draws_lods(MipContext* ctx, const MipFrame* frame, const uint32_t* visible_bitmap, const MipLodPolicy* policy,
                             const MipBatchOutputs* out) {
  if (!ctx) return MIP_ERR_INVALID_ARGUMENT;
  if (int32_t rc = check_policy(ctx, policy)) return rc;
  return batch_draws(ctx, frame, visible_bitmap, policy, MIP_BATCH_ORDER_DRAW_INDEX, out);
}

int32_t mip_batch_draws_ordered(MipContext* ctx, const MipFrame* frame, const uint32_t* visible_bitmap, const MipLodPolicy* policy,
                                uint32_t order, const MipBatchOutputs* out) {
  if (!ctx) return MIP_ERR_INVALID_ARGUMENT;
  if (order != MIP_BATCH_ORDER_DRAW_INDEX && order != MIP_BATCH_ORDER_NEAR_FIRST && order != MIP_BATCH_ORDER_FAR_FIRST)
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "unknown order %u", order);
  if (int32_t rc = check_policy(ctx, policy)) return rc;
  return batch_draws(ctx, frame, visible_bitmap, policy, order, out);
}

int32_t mip_batch_draws_sorted(MipContext* ctx, const MipFrame* frame, const uint32_t* visible_bitmap, const MipLodPolicy* policy,
                               const MipSortPolicy* sort, const MipBatchOutputs* out) {
  if (!ctx) return MIP_ERR_INVALID_ARGUMENT;
  if (int32_t rc = check_sort(ctx, sort)) return rc;
  if (int32_t rc = check_policy(ctx, policy)) return rc;
  return batch_draws_sorted(ctx, frame, visible_bitmap, policy, sort, out);
}

int32_t mip_batch_draws_views(MipContext* ctx, const MipFrame* frames, const uint32_t* const* visible_bitmaps, uint32_t n_views,
                              const MipLodPolicy* policy, const MipViewBatchOutputs* out) {
  if (!ctx) return MIP_ERR_INVALID_ARGUMENT;
  if (int32_t rc = check_policy(ctx, policy)) return rc;
  return batch_draws_views(ctx, frames, visible_bitmaps, n_views, policy, out);
}

int32_t mip_batch_draws_shard(MipContext* ctx, const MipFrame* frame, const uint32_t* visible_bitmap, const MipLodPolicy* policy,
                              void* chunk, uint32_t ids_capacity, uint32_t flags) {
  if (!ctx) return MIP_ERR_INVALID_ARGUMENT;
  if (int32_t rc = check_policy(ctx, policy)) return rc;
  if (!chunk) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "chunk is NULL");
  if ((uintptr_t)chunk % 16u != 0u) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "chunk is not 16-byte aligned");
  // the stage's outputs as batch_draws() takes them: the ids of the chunk; no commands, no counts, no matrices
  MipBatchOutputs out{};
  out.struct_size = sizeof(MipBatchOutputs);
  out.flags = flags;
  out.batch_cmds = chunk;                               // (not written: the chunk epilogue takes the command writer's place)
  out.batch_count = static_cast<uint32_t*>(chunk);
  out.instance_ids = reinterpret_cast<uint32_t*>(static_cast<unsigned char*>(chunk) + MIP_BATCH_CHUNK_IDS_OFFSET(ctx->lod_buckets));
  return batch_draws(ctx, frame, visible_bitmap, policy, MIP_BATCH_ORDER_DRAW_INDEX, &out, static_cast<uint32_t*>(chunk), ids_capacity);
}

int32_t mip_merge_batches(MipContext* ctx, const void* chunks, uint32_t n_chunks, uint64_t chunk_stride_bytes, uint32_t chunk_capacity,
                          const MipBatchOutputs* out) {
  if (!ctx) return MIP_ERR_INVALID_ARGUMENT;
  return merge_batches(ctx, chunks, n_chunks, chunk_stride_bytes, chunk_capacity, out);
}

}  // extern "C"
