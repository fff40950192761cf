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
// batch_views_kernel.hpp, batch_sorted_kernel.hpp); batch_plan.hpp says which instantiation a call launches. The kernels are instantiated here and only here.
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

// The slot's scratch, sized from the context's capacities at first use: the tile x bin counts and the digit totals for every
// frame; the (key, instance) lists, the bucket histogram and the slot map only once a frame needs more than one pass.
int32_t ensure_scratch(MipContext* ctx, MipContext::BatchScratch& bs, bool several_passes, bool slot_map) {
  const size_t cap = instance_cap(ctx);
  if (!bs.d_counts) {
    MIP_HIP(ctx, hipMalloc(&bs.d_counts, (size_t)mip::kBatchBins * batch_tiles_for((uint32_t)cap) * 4));
    MIP_HIP(ctx, hipMalloc(&bs.d_totals, (mip::kBatchMaxPasses * mip::kBatchBins + 1) * 4));
  }
  if (several_passes && !bs.d_keys[0]) {
    for (int k = 0; k < 2; ++k) {
      MIP_HIP(ctx, hipMalloc(&bs.d_keys[k], cap * 4));
      MIP_HIP(ctx, hipMalloc(&bs.d_ids[k], cap * 4));
    }
    MIP_HIP(ctx, hipMalloc(&bs.d_bucket_hist, (size_t)(ctx->max_meshes ? ctx->max_meshes : 1) * MIP_MAX_LODS * 4));
  }
  if (several_passes && slot_map && !bs.d_slot_of) MIP_HIP(ctx, hipMalloc(&bs.d_slot_of, cap * 4));
  return MIP_OK;
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

void release_view_scratch(MipContext::ViewBatchScratch& vs) {
  (void)hipFree(vs.d_counts);
  (void)hipFree(vs.d_totals);
  for (int k = 0; k < 2; ++k) {
    (void)hipFree(vs.d_keys[k]);
    (void)hipFree(vs.d_ids[k]);
  }
  (void)hipFree(vs.d_bucket_hist);
  vs = MipContext::ViewBatchScratch{};
}

// mip_batch_draws_views' own scratch, for the entries (n_views x N) and global buckets (n_views x B) of this call: kept while
// it is large enough, replaced by a larger one otherwise (hipFree waits for the work that still reads the old one).
int32_t ensure_view_scratch(MipContext* ctx, MipContext::ViewBatchScratch& vs, size_t entries, size_t buckets, bool several_passes) {
  if (!vs.d_totals) MIP_HIP(ctx, hipMalloc(&vs.d_totals, (mip::kBatchMaxPasses * mip::kBatchBins + 1) * 4));
  if (entries > vs.entries_cap) {
    (void)hipFree(vs.d_counts);
    vs.d_counts = nullptr;
    vs.entries_cap = 0;
    MIP_HIP(ctx, hipMalloc(&vs.d_counts, (size_t)mip::kBatchBins * batch_tiles_for((uint32_t)entries) * 4));
    vs.entries_cap = entries;
  }
  if (several_passes && entries > vs.list_cap) {
    for (int k = 0; k < 2; ++k) {
      (void)hipFree(vs.d_keys[k]);
      (void)hipFree(vs.d_ids[k]);
      vs.d_keys[k] = vs.d_ids[k] = nullptr;
    }
    vs.list_cap = 0;
    for (int k = 0; k < 2; ++k) {
      MIP_HIP(ctx, hipMalloc(&vs.d_keys[k], entries * 4));
      MIP_HIP(ctx, hipMalloc(&vs.d_ids[k], entries * 4));
    }
    vs.list_cap = entries;
  }
  if (several_passes && buckets > vs.hist_cap) {
    (void)hipFree(vs.d_bucket_hist);
    vs.d_bucket_hist = nullptr;
    vs.hist_cap = 0;
    MIP_HIP(ctx, hipMalloc(&vs.d_bucket_hist, buckets * 4));
    vs.hist_cap = buckets;
  }
  return MIP_OK;
}

}  // namespace

void batch_release(MipContext* ctx) {
  for (auto& bs : ctx->batch) {
    (void)hipFree(bs.d_counts);
    (void)hipFree(bs.d_totals);
    for (int k = 0; k < 2; ++k) {
      (void)hipFree(bs.d_keys[k]);
      (void)hipFree(bs.d_ids[k]);
    }
    (void)hipFree(bs.d_bucket_hist);
    (void)hipFree(bs.d_slot_of);
    (void)hipFree(bs.d_bucket_of);
  }
  ctx->batch.clear();
  release_view_scratch(ctx->view_batch);
  (void)hipFree(ctx->batch_merge.d_words);
  ctx->batch_merge = MipContext::BatchMergeScratch{};
}

namespace {

// The argument checks every entry point shares, and the context's device made current.
int32_t check_call(MipContext* ctx, const MipFrame* frame, const uint32_t* visible_bitmap, const MipBatchOutputs* out) {
  if (!frame || !visible_bitmap || !out) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "frame/visible_bitmap/out is NULL");
  if (out->struct_size != sizeof(MipBatchOutputs))
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "MipBatchOutputs.struct_size %u != %zu", out->struct_size, sizeof(MipBatchOutputs));
  if (out->flags & ~(MIP_OUT_DEVICE | MIP_OUT_ASYNC)) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "unknown MipBatchOutputs flags 0x%x", out->flags);
  if (!(out->flags & MIP_OUT_DEVICE)) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "mip_batch_draws needs MIP_OUT_DEVICE outputs");
  if (!out->batch_cmds || !out->batch_count || !out->instance_ids)
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "batch_cmds/batch_count/instance_ids is NULL");
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
  const bool several = plan.several();
  if (ctx->batch.size() != ctx->slots.size()) ctx->batch.resize(ctx->slots.size());
  MipContext::BatchScratch& bs = ctx->batch[slot];
  if (int32_t rc = ensure_scratch(ctx, bs, several, out->batch_model != nullptr)) return rc;

  mip::ShardBatchArgs a{};  // the most derived block: every kernel takes its own leading part
  a.chunk = shard_chunk;
  if (policy) {
    a.chain = ctx->d_mesh_chain;
    a.bucket_lod = ctx->d_bucket_lod;
    std::memcpy(a.switch_sq, policy->switch_sq, sizeof a.switch_sq);
  }
  a.depth_flip = order == MIP_BATCH_ORDER_FAR_FIRST ? mip::kBatchDepthMax : 0u;
  a.pos = ctx->d_pos; a.rot = ctx->d_rot; a.scale = ctx->d_scale; a.mesh_id = ctx->d_mesh_id;
  a.meshes = ctx->d_meshes; a.mesh_draw = ctx->d_mesh_draw;
  a.bitmap = visible_bitmap;
  a.n = n;
  a.n_tiles = batch_tiles_for(n);
  a.n_buckets = (uint32_t)buckets;
  a.n_bins = several ? mip::kBatchBins : (uint32_t)buckets;
  a.first_instance_base = frame->first_instance_base;
  std::memcpy(a.cam, frame->cam_pos, sizeof a.cam);
  a.counts = bs.d_counts;
  a.members = a.members_out = bs.d_totals + mip::kBatchMaxPasses * mip::kBatchBins;
  a.batch_cmds = static_cast<uint32_t*>(out->batch_cmds);
  a.batch_count = out->batch_count;
  a.instance_count = out->instance_count;
#ifdef MIP_DEBUG_STAMPS
  DebugSwitches().tile_order(a.n_tiles, a.debug_tile_mult, a.debug_tile_add);  // as fill_kernel_args (api_frame.hip) permutes the frame's tiles
#endif
  if (several) MIP_HIP(ctx, hipMemsetAsync(bs.d_bucket_hist, 0, (size_t)buckets * 4, stream));

  for (uint32_t p = 0; p < plan.passes; ++p) {
    const bool last = p + 1 == plan.passes;
    a.shift = p * mip::kBatchDigitBits;
    a.totals = bs.d_totals + p * mip::kBatchBins;
    a.bucket_hist = (several && p == 0) ? bs.d_bucket_hist : nullptr;
    a.keys_in = p ? bs.d_keys[(p - 1) & 1u] : nullptr;
    a.ids_in = p ? bs.d_ids[(p - 1) & 1u] : nullptr;
    a.keys_out = last ? nullptr : bs.d_keys[p & 1u];
    a.ids_out = last ? nullptr : bs.d_ids[p & 1u];
    a.instance_ids = last ? out->instance_ids : nullptr;
    a.slot_of = (last && several && out->batch_model) ? bs.d_slot_of : nullptr;
    a.batch_model = (last && !several) ? static_cast<float4*>(out->batch_model) : nullptr;
    if (int32_t rc = launch(ctx, plan.count(p), a.n_tiles, stream, a)) return rc;
    if (int32_t rc = launch(ctx, mip::BatchKernel::rowscan, a.n_bins, stream, a)) return rc;
    if (p == 0) {  // the scan's epilogue: bucket totals -> commands and the two counts (and the list's length for later passes)
      a.bucket_totals = several ? bs.d_bucket_hist : a.totals;
      if (int32_t rc = launch(ctx, plan.commands, 1, stream, a)) return rc;
    }
    if (int32_t rc = launch(ctx, plan.scatter(p), a.n_tiles, stream, a)) return rc;
  }
  if (plan.model != mip::BatchKernel::none) {
    a.batch_model = static_cast<float4*>(out->batch_model);
    if (int32_t rc = launch(ctx, plan.model, a.n_tiles, stream, a)) return rc;
  }
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
  if (ctx->batch.size() != ctx->slots.size()) ctx->batch.resize(ctx->slots.size());
  MipContext::BatchScratch& bs = ctx->batch[slot];
  if (int32_t rc = ensure_scratch(ctx, bs, true, out->batch_model != nullptr)) return rc;
  if (!bs.d_bucket_of) MIP_HIP(ctx, hipMalloc(&bs.d_bucket_of, instance_cap(ctx) * 4));

  mip::SortedBatchArgs a{};
  a.chain = ctx->d_mesh_chain;
  a.bucket_lod = ctx->d_bucket_lod;
  std::memcpy(a.switch_sq, policy->switch_sq, sizeof a.switch_sq);
  a.depth_shift = 32u - sort->depth_bits;
  a.depth_flip = sort->order == MIP_BATCH_ORDER_FAR_FIRST ? (axis ? mip::kSortedUmaxAxis : mip::kSortedUmaxRadial) >> a.depth_shift : 0u;
  if (axis) std::memcpy(a.axis, sort->axis, sizeof a.axis);
  a.pos = ctx->d_pos; a.rot = ctx->d_rot; a.scale = ctx->d_scale; a.mesh_id = ctx->d_mesh_id;
  a.meshes = ctx->d_meshes; a.mesh_draw = ctx->d_mesh_draw;
  a.bitmap = visible_bitmap;
  a.n = n;
  a.n_tiles = batch_tiles_for(n);
  a.n_buckets = (uint32_t)buckets;
  a.n_bins = mip::kBatchBins;
  a.first_instance_base = frame->first_instance_base;
  std::memcpy(a.cam, frame->cam_pos, sizeof a.cam);
  a.counts = bs.d_counts;
  a.members = a.members_out = bs.d_totals + mip::kBatchMaxPasses * mip::kBatchBins;
  a.batch_cmds = static_cast<uint32_t*>(out->batch_cmds);
  a.batch_count = out->batch_count;
  a.instance_count = out->instance_count;
#ifdef MIP_DEBUG_STAMPS
  DebugSwitches().tile_order(a.n_tiles, a.debug_tile_mult, a.debug_tile_add);
#endif

  for (uint32_t p = 0; p < plan.passes; ++p) {
    const bool last = p + 1 == plan.passes;
    a.shift = p * mip::kBatchDigitBits;
    a.totals = bs.d_totals + p * mip::kBatchBins;
    a.keys_in = p ? bs.d_keys[(p - 1) & 1u] : nullptr;
    a.ids_in = p ? bs.d_ids[(p - 1) & 1u] : nullptr;
    a.keys_out = last ? nullptr : bs.d_keys[p & 1u];
    a.ids_out = last ? nullptr : bs.d_ids[p & 1u];
    a.instance_ids = last ? out->instance_ids : nullptr;
    a.slot_of = (last && out->batch_model) ? bs.d_slot_of : nullptr;
    a.bucket_out = p == 0 ? bs.d_bucket_of : nullptr;  // the count of pass 0 stores the buckets; its scatter does not store them again
    if (int32_t rc = launch(ctx, plan.count(p), a.n_tiles, stream, a)) return rc;
    a.bucket_out = nullptr;
    if (int32_t rc = launch(ctx, mip::BatchKernel::rowscan, a.n_bins, stream, a)) return rc;
    if (p == 0)  // the scan's epilogue: the digit totals -> the list's length and instance_count
      if (int32_t rc = launch(ctx, plan.commands, 1, stream, a)) return rc;
    if (int32_t rc = launch(ctx, plan.scatter(p), a.n_tiles, stream, a)) return rc;
  }
  // the run stage: the tile rows reuse `counts` (row 0), the slots' buckets a list buffer the last pass did not read, and the
  // row's sum — the number of heads — is batch_count
  a.bucket_in = bs.d_bucket_of;
  a.slot_bucket = bs.d_keys[(plan.passes - 1) & 1u];
  a.totals = out->batch_count;
  for (uint32_t k = 0; k < mip::kBatchRunStageLaunches; ++k) {
    const mip::BatchKernel kernel = mip::batch_run_stage(k);
    if (int32_t rc = launch(ctx, kernel, kernel == mip::BatchKernel::rowscan ? 1u : a.n_tiles, stream, a)) return rc;
  }
  if (plan.model != mip::BatchKernel::none) {
    a.batch_model = static_cast<float4*>(out->batch_model);
    if (int32_t rc = launch(ctx, plan.model, a.n_tiles, stream, a)) return rc;
  }
  return finish(ctx, stream, async);
}

// mip_batch_draws_views: every check first (a refused call writes nothing), then one sort of the n_views x N (instance, view)
// entries by key = view * B + bucket on the context's first stream, where mip_run_views runs.
int32_t batch_draws_views(MipContext* ctx, const MipFrame* frames, const uint32_t* const* visible_bitmaps, uint32_t n_views,
                          const MipLodPolicy* policy, const MipViewBatchOutputs* out) {
  if (!frames || !visible_bitmaps || !out) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "frames/visible_bitmaps/out is NULL");
  if (out->struct_size != sizeof(MipViewBatchOutputs))
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "MipViewBatchOutputs.struct_size %u != %zu", out->struct_size, sizeof(MipViewBatchOutputs));
  if (out->reserved != 0u) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "MipViewBatchOutputs.reserved is %u, not 0", out->reserved);
  if (out->flags & ~(MIP_OUT_DEVICE | MIP_OUT_ASYNC)) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "unknown MipViewBatchOutputs flags 0x%x", out->flags);
  if (!(out->flags & MIP_OUT_DEVICE)) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "mip_batch_draws_views needs MIP_OUT_DEVICE outputs");
  if (!out->batch_cmds || !out->batch_counts || !out->instance_ids)
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "batch_cmds/batch_counts/instance_ids is NULL");
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
  MipContext::ViewBatchScratch& vs = ctx->view_batch;
  if (int32_t rc = ensure_view_scratch(ctx, vs, entries, hist_words, several)) return rc;

  mip::ViewBatchArgs a{};
  a.chain = ctx->d_mesh_chain;
  a.bucket_lod = ctx->d_bucket_lod;
  std::memcpy(a.switch_sq, policy->switch_sq, sizeof a.switch_sq);
  a.pos = ctx->d_pos; a.rot = ctx->d_rot; a.scale = ctx->d_scale; a.mesh_id = ctx->d_mesh_id;
  a.meshes = ctx->d_meshes; a.mesh_draw = ctx->d_mesh_draw;
  a.n = n;
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
  a.n_tiles = batch_tiles_for(entries);
  a.n_buckets = (uint32_t)buckets;
  a.n_bins = several ? mip::kBatchBins : (uint32_t)buckets;
  a.counts = vs.d_counts;
  a.members = a.members_out = vs.d_totals + mip::kBatchMaxPasses * mip::kBatchBins;
  a.batch_cmds = static_cast<uint32_t*>(out->batch_cmds);
  a.batch_counts = out->batch_counts;
  a.view_first_slot = out->view_first_slot;
#ifdef MIP_DEBUG_STAMPS
  DebugSwitches().tile_order(a.n_tiles, a.debug_tile_mult, a.debug_tile_add);
#endif
  if (several) MIP_HIP(ctx, hipMemsetAsync(vs.d_bucket_hist, 0, hist_words * 4, stream));

  for (uint32_t p = 0; p < plan.passes; ++p) {
    const bool last = p + 1 == plan.passes;
    a.shift = p * mip::kBatchDigitBits;
    a.totals = vs.d_totals + p * mip::kBatchBins;
    a.bucket_hist = (several && p == 0) ? vs.d_bucket_hist : nullptr;
    a.keys_in = p ? vs.d_keys[(p - 1) & 1u] : nullptr;
    a.ids_in = p ? vs.d_ids[(p - 1) & 1u] : nullptr;
    a.keys_out = last ? nullptr : vs.d_keys[p & 1u];
    a.ids_out = last ? nullptr : vs.d_ids[p & 1u];
    a.instance_ids = last ? out->instance_ids : nullptr;
    if (int32_t rc = launch(ctx, plan.count(p), a.n_tiles, stream, a)) return rc;
    if (int32_t rc = launch(ctx, mip::BatchKernel::rowscan, a.n_bins, stream, a)) return rc;
    if (p == 0) {  // global bucket totals -> every view's commands, count and first slot (and the list's length for later passes)
      a.bucket_totals = several ? vs.d_bucket_hist : a.totals;
      if (int32_t rc = launch(ctx, plan.commands, 1, stream, a)) return rc;
    }
    if (int32_t rc = launch(ctx, plan.scatter(p), a.n_tiles, stream, a)) return rc;
  }
  return finish(ctx, stream, async);
}

// mip_merge_batches: every check first (a refused call writes nothing), then the offsets kernel and the gather on the
// context's first stream, where the other merges run.
int32_t merge_batches(MipContext* ctx, const void* chunks, uint32_t n_chunks, uint64_t stride, uint32_t capacity, const MipBatchOutputs* out) {
  if (!chunks || !out) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "chunks/out is NULL");
  if (out->struct_size != sizeof(MipBatchOutputs))
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "MipBatchOutputs.struct_size %u != %zu", out->struct_size, sizeof(MipBatchOutputs));
  if (out->flags & ~(MIP_OUT_DEVICE | MIP_OUT_ASYNC)) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "unknown MipBatchOutputs flags 0x%x", out->flags);
  if (!(out->flags & MIP_OUT_DEVICE)) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "mip_merge_batches needs MIP_OUT_DEVICE outputs");
  if (!out->batch_cmds || !out->batch_count || !out->instance_ids)
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "batch_cmds/batch_count/instance_ids is NULL");
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
  if (plan.scratch_words > ms.words_cap) {  // (hipFree waits for the work that still reads the old one)
    (void)hipFree(ms.d_words);
    ms.d_words = nullptr;
    ms.words_cap = 0;
    MIP_HIP(ctx, hipMalloc(&ms.d_words, (size_t)plan.scratch_words * 4));
    ms.words_cap = (size_t)plan.scratch_words;
  }
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
