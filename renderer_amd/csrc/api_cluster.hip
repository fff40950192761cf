// api_cluster.hip — C ABI of the instance pipeline, part 7 of 7: cluster culling (extension, not reference behaviour).
// mip_build_clusters cuts every level of every mesh into clusters of MIP_CLUSTER_TRIANGLES triangles and builds their boxes on
// the device from the resident geometry; mip_cull_clusters runs the frustum test and (optionally) the Hi-Z test of the
// instance level on every cluster of every member of a bitmap and writes one command per run of surviving clusters;
// mip_cull_clusters_phase is the same call in two phases: FIRST also records the clusters that passed the planes and failed the
// Hi-Z test, SECOND tests exactly those again under a new pyramid; mip_cull_cluster_triangles runs the per-triangle stage's test
// on the triangles of the surviving clusters and writes one culled index stream with the commands into it.
// mip_build_cluster_cones gives every cluster of a valid table a normal cone, and mip_cull_clusters_cone /
// mip_cull_cluster_triangles_cone are the two culls with the cone's back-face test in front of SURVIVES (one new kernel in
// the cull kernel's place; every other launch is the plain call's).
// mip_list_clusters is mip_cull_clusters / mip_cull_clusters_cone with one 16-byte entry per surviving cluster and the arguments
// of one indirect draw in the commands' place (cluster_list_kernel.hpp, cluster_list_plan.hpp: four new kernels behind the cull).
// mip_cull_clusters_views is the frustum test of mip_cull_clusters for several views in one call, on the context's first stream
// with a scratch and a pair of status words of its own (cluster_views_kernel.hpp, cluster_views_plan.hpp).
// mip_list_clusters_views is that call's front with the list's entries behind it, one list and one indirect draw per view, on the
// same stream, scratch and status words (cluster_views_list_kernel.hpp, cluster_views_list_plan.hpp: three new kernels).
// mip_list_clusters_phase is mip_cull_clusters_phase with the list's entries in the commands' place, the list started at an entry
// base read on the device (cluster_list_phase_kernel.hpp, cluster_list_phase_plan.hpp: the front and the list tail of its own).
// mip_list_clusters_views_occluded is mip_list_clusters_views with a depth pyramid per view: one new kernel in the several-view
// cull kernel's place (cluster_views_occluded_kernel.hpp), the same plan, stream, scratch and status words.
// mip_list_cluster_triangles is mip_list_clusters with the per-triangle test behind the cull: an entry per surviving cluster that
// keeps a triangle and its 64-bit triangle mask beside it (cluster_triangle_list_kernel.hpp, cluster_triangle_list_plan.hpp: the
// list's front and word members, then four new kernels).
// cluster_plan.hpp, cluster_triangle_plan.hpp and cluster_cone_plan.hpp hold the arithmetic and the launch plans; the kernels
// (cluster_kernel.hpp, cluster_triangle_kernel.hpp, cluster_cone_kernel.hpp) are instantiated here and only here.
#include "context.hpp"
#include "cluster_kernel.hpp"
#include "cluster_triangle_kernel.hpp"
#include "cluster_cone_kernel.hpp"
#include "cluster_views_kernel.hpp"
#include "cluster_list_kernel.hpp"
#include "cluster_views_list_kernel.hpp"
#include "cluster_list_phase_kernel.hpp"
#include "cluster_views_occluded_kernel.hpp"
#include "cluster_triangle_list_kernel.hpp"

static_assert(sizeof(MipClusterViewOutputs) == 40, "MipClusterViewOutputs is part of the ABI");
static_assert(sizeof(MipClusterOutputs) == 40, "MipClusterOutputs is part of the ABI");
static_assert(sizeof(MipClusterRecord) == 24, "MipClusterRecord is part of the ABI");
static_assert(sizeof(MipClusterTriangleOutputs) == 56, "MipClusterTriangleOutputs is part of the ABI");
static_assert(sizeof(MipClusterCone) == 24, "MipClusterCone is part of the ABI");
static_assert(sizeof(MipClusterEntry) == 16 && sizeof(MipClusterEntry) == sizeof(uint4), "MipClusterEntry is part of the ABI: one 16-byte store");
static_assert(sizeof(MipClusterListOutputs) == 48, "MipClusterListOutputs is part of the ABI");
static_assert(sizeof(MipClusterViewListOutputs) == 48, "MipClusterViewListOutputs is part of the ABI");
static_assert(sizeof(MipClusterPhaseListOutputs) == 56, "MipClusterPhaseListOutputs is part of the ABI");
static_assert(sizeof(MipClusterViewOccludedListOutputs) == 56, "MipClusterViewOccludedListOutputs is part of the ABI");
static_assert(sizeof(MipClusterTriangleListOutputs) == 56, "MipClusterTriangleListOutputs is part of the ABI");
static_assert(mip::kClusterTriangleListStats == mip::kClusterTriangleStats, "words 1 to 5 are mip_cull_cluster_triangles'");
static_assert(sizeof(mip::ClusterConeEntry) == 2 * sizeof(float4), "a cone is the two 16-byte words the kernels load");
static_assert(mip::kClusterFirst == MIP_CLUSTER_PHASE_FIRST && mip::kClusterSecond == MIP_CLUSTER_PHASE_SECOND, "cluster_kernel.hpp restates the header");
static_assert(MIP_CLUSTER_TRIANGLES == mip::kClusterTriangles, "cluster_plan.hpp restates the header");

namespace mip_host {
namespace {

// The status words (pinned, device-visible): two per frame slot. [2 slot] is raised by the asynchronous calls of the slot and
// collected by mip_wait; [2 slot + 1] by a synchronous call, which drains its stream and collects the word itself — so a call
// that fitted is never blamed for another's overflow, and no overflow is reported twice. A word holds a code: the bits
// kClusterStatusCapacity (an overflow) and kClusterStatusDevice (a SECOND call met a record that is not its own).
constexpr uint32_t kStatusWords = 2 * MIP_MAX_FRAMES_IN_FLIGHT;
constexpr const char* kNotItsRecord = "mip_cull_clusters_phase / mip_list_clusters_phase: the record's header names another W or another member count than this SECOND call's: it is not the record of the FIRST call over these members (a zero count is written, stats holds the call's W and members)";

// Every level of every mesh against the host copies of the geometry, as check_geometry (api_frame.hip) checks LODs 0 and 1:
// the level's range inside the uploaded indices, every vertex its triangles name inside the uploaded vertices.
int32_t check_levels(MipContext* ctx) {
  for (uint32_t k = 0; k < ctx->h_meshes.size(); ++k) {
    const MipMesh& m = ctx->h_meshes[k];
    for (uint32_t l = 0; l < m.n_lods; ++l) {
      const uint64_t off = m.index_offset[l], len = m.index_len[l];
      if (off + len > ctx->n_indices)
        return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "mesh %u LOD %u: indices [%llu, %llu) outside the %u uploaded indices", k, l,
                    (unsigned long long)off, (unsigned long long)(off + len), ctx->n_indices);
      const uint64_t used = 3ull * mip::cluster_level_triangles((uint32_t)len);
      uint32_t mx = 0;
      for (uint64_t j = off; j < off + used; ++j) mx = ctx->h_indices[j] > mx ? ctx->h_indices[j] : mx;
      if (used && (m.vertex_offset < 0 || (uint64_t)m.vertex_offset + mx >= ctx->n_vertices))
        return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "mesh %u LOD %u: vertex_offset %d + largest index %u outside the %u uploaded vertices", k, l,
                    m.vertex_offset, mx, ctx->n_vertices);
    }
  }
  return MIP_OK;
}

int32_t build_clusters(MipContext* ctx) {
  if (!ctx->have_meshes || !ctx->have_geometry) return fail(ctx, MIP_ERR_NOT_READY, "mip_build_clusters needs the mesh table and mip_set_geometry");
  if (int32_t rc = check_levels(ctx)) return rc;
  // bucket b = lod_base[mesh] + lod, as mip_set_mesh_table numbers them
  std::vector<uint32_t> base;
  base.reserve((size_t)ctx->lod_buckets + 1);
  unsigned long long total = 0;
  uint32_t max_clusters = 0;
  for (const MipMesh& m : ctx->h_meshes)
    for (uint32_t l = 0; l < m.n_lods; ++l) {
      const uint32_t c = mip::cluster_level_clusters(m.index_len[l]);
      base.push_back((uint32_t)total);
      total += c;
      if (c > max_clusters) max_clusters = c;
      if (total > mip::kClusterMaxTotal) return fail(ctx, MIP_ERR_CAPACITY, "more than 2^31 clusters in the table");
    }
  base.push_back((uint32_t)total);
  if (int32_t rc = bind_device(ctx)) return rc;
  if (int32_t rc = sync_all(ctx)) return rc;  // a cull in flight reads the table this call replaces
  MipContext::ClusterTable& t = ctx->clusters;
  t.valid = false;
  t.cones_valid = false;  // (cones of the table this call replaces)
  if (int32_t rc = grow(ctx, &t.d_boxes, &t.boxes_cap, (size_t)total, 2 * sizeof(float4))) return rc;
  if (int32_t rc = grow(ctx, &t.d_cluster_base, &t.base_cap, base.size(), 4)) return rc;
  MIP_HIP(ctx, hipMemcpyAsync(t.d_cluster_base, base.data(), base.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  if (total) {
    mip::ClusterBuildArgs a{};
    a.vertices = ctx->d_vertices;
    a.indices = ctx->d_indices;
    a.chain = ctx->d_mesh_chain;
    a.mesh_draw = ctx->d_mesh_draw;
    a.bucket_lod = ctx->d_bucket_lod;
    a.cluster_base = t.d_cluster_base;
    a.boxes = t.d_boxes;
    a.n_buckets = (uint32_t)ctx->lod_buckets;
    a.total = (uint32_t)total;
    const uint32_t blocks = (uint32_t)((total + mip::kWaves - 1u) / mip::kWaves);
    hipLaunchKernelGGL(mip::mip_cluster_build_kernel, dim3(blocks), dim3(mip::kClusterThreads), 0, ctx->stream, a);
    MIP_HIP(ctx, hipGetLastError());
  }
  MIP_HIP(ctx, hipStreamSynchronize(ctx->stream));  // `base` is a local; the call is synchronous
  t.total = (uint32_t)total;
  t.max_clusters = max_clusters;
  t.valid = true;
  return MIP_OK;
}

// One cone per cluster of the valid table, from the resident geometry and the table's boxes; synchronous like the table's build.
int32_t build_cluster_cones(MipContext* ctx) {
  MipContext::ClusterTable& t = ctx->clusters;
  if (!t.valid) return fail(ctx, MIP_ERR_NOT_READY, "mip_build_cluster_cones needs a valid cluster table (mip_build_clusters)");
  if (int32_t rc = bind_device(ctx)) return rc;
  if (int32_t rc = sync_all(ctx)) return rc;  // a cull in flight reads the cones this call replaces
  t.cones_valid = false;
  if (int32_t rc = grow(ctx, &t.d_cones, &t.cones_cap, (size_t)t.total, 2 * sizeof(float4))) return rc;
  if (t.total) {
    mip::ClusterConeBuildArgs a{};
    a.b.vertices = ctx->d_vertices;
    a.b.indices = ctx->d_indices;
    a.b.chain = ctx->d_mesh_chain;
    a.b.mesh_draw = ctx->d_mesh_draw;
    a.b.bucket_lod = ctx->d_bucket_lod;
    a.b.cluster_base = t.d_cluster_base;
    a.b.boxes = t.d_boxes;
    a.b.n_buckets = (uint32_t)ctx->lod_buckets;
    a.b.total = t.total;
    a.cones = t.d_cones;
    const uint32_t blocks = (t.total + mip::kWaves - 1u) / mip::kWaves;
    hipLaunchKernelGGL(mip::mip_cluster_cone_build_kernel, dim3(blocks), dim3(mip::kClusterThreads), 0, ctx->stream, a);
    MIP_HIP(ctx, hipGetLastError());
    MIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  t.cones_valid = true;
  return MIP_OK;
}

// What the two cone calls refuse on top of the plain calls' list.
int32_t check_cone(MipContext* ctx, const MipClusterCone* cone) {
  if (!cone) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "cone is NULL");
  if (cone->struct_size != sizeof(MipClusterCone))
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "MipClusterCone.struct_size %u != %zu", cone->struct_size, sizeof(MipClusterCone));
  if (cone->flags) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "unknown MipClusterCone flags 0x%x", cone->flags);
  if (!(cone->facing == 1.0f || cone->facing == -1.0f)) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "MipClusterCone.facing is neither +1 nor -1");
  return MIP_OK;
}

int32_t ensure_scratch(MipContext* ctx, MipContext::ClusterScratch& cs, const mip::ClusterPlan& plan, bool first) {
  const size_t cap = instance_cap(ctx);
  if (!cs.d_instances) {
    MIP_HIP(ctx, hipMalloc(&cs.d_instances, (4 * cap + 1) * 4));
    const size_t tiles = (cap + mip::kClusterInstanceTile - 1) / mip::kClusterInstanceTile;
    MIP_HIP(ctx, hipMalloc(&cs.d_tile_items, tiles * 8));
    MIP_HIP(ctx, hipMalloc(&cs.d_tile_members, tiles * 4));
    MIP_HIP(ctx, hipMalloc(&cs.d_scalars, mip::kClusterScWords * 4));
  }
  if (int32_t rc = grow(ctx, &cs.d_words, &cs.words_cap, (size_t)plan.survive_words, 16)) return rc;
  if (int32_t rc = grow(ctx, &cs.d_tile_heads, &cs.head_tiles_cap, (size_t)plan.head_tiles, 4)) return rc;
  if (int32_t rc = grow(ctx, &cs.d_tile_survivors, &cs.survivor_tiles_cap, (size_t)plan.head_tiles, 4)) return rc;
  if (first)
    if (int32_t rc = grow(ctx, &cs.d_tile_candidates, &cs.candidate_tiles_cap, (size_t)plan.head_tiles, 4)) return rc;
  return MIP_OK;
}

// What mip_cull_cluster_triangles takes on top (cluster_triangle_plan.hpp): 12 bytes per work item of the bound.
int32_t ensure_triangle_scratch(MipContext* ctx, MipContext::ClusterScratch& cs, const mip::ClusterTrianglePlan& plan) {
  if (!cs.d_tri_scalars) MIP_HIP(ctx, hipMalloc(&cs.d_tri_scalars, mip::kClusterTriScWords * 4));
  if (int32_t rc = grow(ctx, &cs.d_triangle_words, &cs.triangle_words_cap, (size_t)plan.triangle_words, 8)) return rc;
  if (int32_t rc = grow(ctx, &cs.d_item_prefix, &cs.item_prefix_cap, (size_t)plan.item_prefixes, 4)) return rc;
  if (int32_t rc = grow(ctx, &cs.d_word_total, &cs.word_total_cap, (size_t)plan.word_totals, 4)) return rc;
  if (int32_t rc = grow(ctx, &cs.d_tile_triangles, &cs.tile_triangles_cap, (size_t)plan.item_tiles, 8)) return rc;
  return MIP_OK;
}

// What mip_list_clusters takes on top (cluster_list_plan.hpp): 8 bytes per 64 work items of the bound.
int32_t ensure_list_scratch(MipContext* ctx, MipContext::ClusterScratch& cs, const mip::ClusterListPlan& plan) {
  if (int32_t rc = grow(ctx, &cs.d_word_member, &cs.word_member_cap, (size_t)plan.words, 4)) return rc;
  if (int32_t rc = grow(ctx, &cs.d_word_rank, &cs.word_rank_cap, (size_t)plan.words, 4)) return rc;
  if (int32_t rc = grow(ctx, &cs.d_list_tiles, &cs.list_tiles_cap, (size_t)plan.list_tiles, 4)) return rc;
  return MIP_OK;
}

// What mip_list_cluster_triangles takes on top of the list's (cluster_triangle_list_plan.hpp): 8 bytes per work item and 8 per
// 64 work items of the bound, and the tile sums. The triangle words and the item tiles' sums are mip_cull_cluster_triangles'.
int32_t ensure_triangle_list_scratch(MipContext* ctx, MipContext::ClusterScratch& cs, const mip::ClusterTriangleListPlan& plan) {
  if (int32_t rc = ensure_list_scratch(ctx, cs, plan.list)) return rc;
  if (int32_t rc = grow(ctx, &cs.d_triangle_words, &cs.triangle_words_cap, (size_t)plan.triangle_words, 8)) return rc;
  if (int32_t rc = grow(ctx, &cs.d_nonempty_words, &cs.nonempty_words_cap, (size_t)plan.nonempty_words, 8)) return rc;
  if (int32_t rc = grow(ctx, &cs.d_tile_triangles, &cs.tile_triangles_cap, (size_t)plan.item_tiles, 8)) return rc;
  if (int32_t rc = grow(ctx, &cs.d_tile_clusters, &cs.tile_clusters_cap, (size_t)plan.cluster_tiles, 4)) return rc;
  return MIP_OK;
}

// The event a SECOND call waits for: behind everything the FIRST call enqueued.
int32_t record_written(MipContext* ctx, hipStream_t stream) {
  if (!ctx->cluster_record_written) MIP_HIP(ctx, hipEventCreateWithFlags(&ctx->cluster_record_written, hipEventDisableTiming));
  MIP_HIP(ctx, hipEventRecord(ctx->cluster_record_written, stream));
  return MIP_OK;
}

template <class Kernel, class Args>
int32_t launch(MipContext* ctx, Kernel kernel, uint32_t blocks, hipStream_t stream, const Args& a) {
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(mip::kClusterThreads), 0, stream, a);
  MIP_HIP(ctx, hipGetLastError());
  return MIP_OK;
}

// Every check first (a refused call writes nothing), then the seven launches on the stream of the frame issued last.
// rec == null: mip_cull_clusters; else a phase of mip_cull_clusters_phase (`phased`: the entry point, which refuses a null rec).
// tri != null: mip_cull_cluster_triangles — `out` holds its leading fields; the triangle test, its scan, the write and the
// commands into the culled stream take the place of the epilogue and the commands kernel (nine launches).
// cone != null (`coned`: the entry point, which refuses a null cone): the cone calls — mip_cluster_cone_cull_kernel in the
// cull kernel's place, nothing else differs.
// list != null: mip_list_clusters — `out` holds its fields under mip_cull_clusters' names; the word members, the count, the
// list's epilogue and the write take the place of heads, epilogue and commands (eight launches). cone may be null or not.
// tlist != null (with `list`, which then holds the fields the two structs share): mip_list_cluster_triangles — the triangle
// test between the word members and the count, and the count, epilogue and write of cluster_triangle_list_kernel.hpp (nine launches).
int32_t cull_clusters(MipContext* ctx, const MipFrame* frame, const uint32_t* visible_bitmap, const MipLodPolicy* policy, const MipOcclusion* occ,
                      const MipClusterOutputs* out, const MipClusterRecord* rec, bool phased, const MipClusterTriangleOutputs* tri = nullptr,
                      const MipClusterCone* cone = nullptr, bool coned = false, const MipClusterListOutputs* list = nullptr,
                      const MipClusterTriangleListOutputs* tlist = nullptr) {
  if (!frame || !visible_bitmap || !out) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "frame/visible_bitmap/out is NULL");
  if (coned)
    if (int32_t rc = check_cone(ctx, cone)) return rc;
  if (out->struct_size != sizeof(MipClusterOutputs))
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "MipClusterOutputs.struct_size %u != %zu", out->struct_size, sizeof(MipClusterOutputs));
  if (out->flags & ~(MIP_OUT_DEVICE | MIP_OUT_ASYNC)) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "unknown MipClusterOutputs flags 0x%x", out->flags);
  if (!(out->flags & MIP_OUT_DEVICE)) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "mip_cull_clusters needs MIP_OUT_DEVICE outputs");
  if (!out->cluster_cmds || !out->cmd_count) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "cluster_cmds/cmd_count is NULL");
  if ((uintptr_t)out->cluster_cmds % 4u != 0u || (uintptr_t)out->cmd_count % 4u != 0u || (uintptr_t)out->stats % 4u != 0u)
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "an output is not 4-byte aligned");
  if (occ) {
    if (occ->struct_size != sizeof(MipOcclusion))
      return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "MipOcclusion.struct_size %u != %zu", occ->struct_size, sizeof(MipOcclusion));
    if (occ->width < 1u || occ->height < 1u || occ->width > MIP_MAX_DEPTH_EXTENT || occ->height > MIP_MAX_DEPTH_EXTENT)
      return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "depth extent %ux%u outside 1..%u", occ->width, occ->height, (unsigned)MIP_MAX_DEPTH_EXTENT);
    if (!occ->pyramid) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "pyramid is NULL");
    if (occ->flags || occ->candidates || occ->occluded_bitmap)
      return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "mip_cull_clusters takes no MipOcclusion flags, candidates or occluded_bitmap");
  }
  if (phased) {
    if (!rec) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "rec is NULL");
    if (rec->struct_size != sizeof(MipClusterRecord))
      return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "MipClusterRecord.struct_size %u != %zu", rec->struct_size, sizeof(MipClusterRecord));
    if (rec->phase != MIP_CLUSTER_PHASE_FIRST && rec->phase != MIP_CLUSTER_PHASE_SECOND)
      return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "unknown MipClusterRecord.phase %u", rec->phase);
    if (!rec->record || (uintptr_t)rec->record % 16u != 0u) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "record is NULL or not 16-byte aligned");
    if (rec->record_bytes < mip::kClusterRecordHeaderBytes) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "record_bytes %llu < 16", (unsigned long long)rec->record_bytes);
    if (!occ) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "mip_cull_clusters_phase needs a MipOcclusion: both phases test against a pyramid");
  }
  const bool first = rec && rec->phase == MIP_CLUSTER_PHASE_FIRST, second = rec && rec->phase == MIP_CLUSTER_PHASE_SECOND;
  if (!ctx->have_instances || !ctx->have_meshes) return fail(ctx, MIP_ERR_NOT_READY, "instances or mesh table not set");
  if (!ctx->clusters.valid) return fail(ctx, MIP_ERR_NOT_READY, "no cluster table, or the mesh table / geometry changed since mip_build_clusters");
  if (cone && !ctx->clusters.cones_valid)
    return fail(ctx, MIP_ERR_NOT_READY, "no cone table, or the cluster table changed since mip_build_cluster_cones");
  if (int32_t rc = bind_device(ctx)) return rc;

  const uint32_t slot = ctx->last_slot;
  hipStream_t stream = ctx->slots[slot].stream;
  const bool async = (out->flags & MIP_OUT_ASYNC) != 0;
  const uint32_t n = ctx->n;
  if (n == 0) {  // nothing to test: zeros
    MIP_HIP(ctx, hipMemsetAsync(out->cmd_count, 0, 4, stream));
    if (out->stats) MIP_HIP(ctx, hipMemsetAsync(out->stats, 0, tri || tlist ? 4 * mip::kClusterTriangleStats : list ? 12 : 16, stream));
    if (list && list->draw_args) {  // {192, 0, 0, 0}
      MIP_HIP(ctx, hipMemsetAsync(list->draw_args, 0, 16, stream));
      MIP_HIP(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(list->draw_args), (int)mip::kClusterListDrawVertices, 1, stream));
    }
    if (first) {
      MIP_HIP(ctx, hipMemsetAsync(rec->record, 0, mip::kClusterRecordHeaderBytes, stream));
      if (int32_t rc = record_written(ctx, stream)) return rc;
    }
    return finish(ctx, stream, async);
  }
  if (!ctx->h_cluster_status) {
    MIP_HIP(ctx, hipHostMalloc(&ctx->h_cluster_status, kStatusWords * 4, hipHostMallocMapped));
    std::memset(ctx->h_cluster_status, 0, kStatusWords * 4);
  }
  const MipContext::ClusterTable& table = ctx->clusters;
  unsigned long long bound = mip::cluster_work_bound(n, table.max_clusters, out->work_capacity);
  if (rec) {  // a W the record has no words for is a work overflow
    const unsigned long long room = mip::cluster_record_items(rec->record_bytes);
    bound = room < bound ? room : bound;
  }
  const mip::ClusterPlan plan = mip::plan_cluster_cull(n, bound);
  if (ctx->cluster_scratch.size() != ctx->slots.size()) ctx->cluster_scratch.resize(ctx->slots.size());
  MipContext::ClusterScratch& cs = ctx->cluster_scratch[slot];
  if (int32_t rc = ensure_scratch(ctx, cs, plan, first)) return rc;
  const mip::ClusterTrianglePlan tri_plan = mip::plan_cluster_triangles(n, bound);
  if (tri)
    if (int32_t rc = ensure_triangle_scratch(ctx, cs, tri_plan)) return rc;
  const mip::ClusterListPlan list_plan = mip::plan_cluster_list(bound);
  const mip::ClusterTriangleListPlan tlist_plan = mip::plan_cluster_triangle_list(bound);
  if (tlist) {
    if (int32_t rc = ensure_triangle_list_scratch(ctx, cs, tlist_plan)) return rc;
  } else if (list) {
    if (int32_t rc = ensure_list_scratch(ctx, cs, list_plan)) return rc;
  }
  if (occ && ctx->next_slot != slot) {
    // a pyramid built for the next run sits on that slot's stream: this call goes behind what that stream holds now
    if (!ctx->cluster_pyramid_ready) MIP_HIP(ctx, hipEventCreateWithFlags(&ctx->cluster_pyramid_ready, hipEventDisableTiming));
    MIP_HIP(ctx, hipEventRecord(ctx->cluster_pyramid_ready, ctx->slots[ctx->next_slot].stream));
    MIP_HIP(ctx, hipStreamWaitEvent(stream, ctx->cluster_pyramid_ready, 0));
  }
  // SECOND goes behind the FIRST call that wrote the record, whichever slot's stream that call ran on
  if (second && ctx->cluster_record_written) MIP_HIP(ctx, hipStreamWaitEvent(stream, ctx->cluster_record_written, 0));

  mip::ClusterArgs a{};
  a.lods.chain = ctx->d_mesh_chain;
  a.lods.bucket_lod = ctx->d_bucket_lod;
  std::memcpy(a.lods.switch_sq, policy->switch_sq, sizeof a.lods.switch_sq);
  a.lods.pos = ctx->d_pos; a.lods.rot = ctx->d_rot; a.lods.scale = ctx->d_scale; a.lods.mesh_id = ctx->d_mesh_id;
  a.lods.meshes = ctx->d_meshes; a.lods.mesh_draw = ctx->d_mesh_draw;
  a.lods.bitmap = visible_bitmap;
  a.lods.n = n;
  a.lods.n_tiles = plan.instance_tiles;
  a.lods.n_buckets = (uint32_t)ctx->lod_buckets;
  a.lods.first_instance_base = frame->first_instance_base;
  std::memcpy(a.lods.cam, frame->cam_pos, sizeof a.lods.cam);
  a.cluster_base = table.d_cluster_base;
  a.boxes = table.d_boxes;
  std::memcpy(a.planes, frame->planes, sizeof a.planes);
  if (occ) {
    std::memcpy(a.pv, occ->pv, sizeof a.pv);
    a.pyramid = static_cast<const float*>(occ->pyramid);
    a.width = occ->width;
    a.height = occ->height;
  }
  a.bound = bound;
  const size_t cap = instance_cap(ctx);
  a.items = cs.d_instances;
  a.bucket = cs.d_instances + cap;
  a.member_inst = cs.d_instances + 2 * cap;
  a.member_first = cs.d_instances + 3 * cap;  // cap + 1 words
  a.tile_items = cs.d_tile_items;
  a.tile_members = cs.d_tile_members;
  a.scalars = cs.d_scalars;
  a.words = static_cast<ulonglong2*>(cs.d_words);
  a.tile_heads = cs.d_tile_heads;
  a.tile_survivors = cs.d_tile_survivors;
  a.cmds = static_cast<uint32_t*>(out->cluster_cmds);
  a.cmd_capacity = out->cmd_capacity;
  a.cmd_count = out->cmd_count;
  a.stats = out->stats;
  if (rec) {
    a.record_header = static_cast<uint32_t*>(rec->record);
    a.record_words = reinterpret_cast<unsigned long long*>(static_cast<char*>(rec->record) + mip::kClusterRecordHeaderBytes);
    a.tile_candidates = cs.d_tile_candidates;
  }
  volatile uint32_t* status = ctx->h_cluster_status + 2u * slot + (async ? 0u : 1u);  // slot < MIP_MAX_FRAMES_IN_FLIGHT
  MIP_HIP(ctx, hipHostGetDevicePointer(reinterpret_cast<void**>(&a.status), const_cast<uint32_t*>(status), 0));
  if (!async) *status = 0;  // (no synchronous call of the slot is in flight: each one drains its stream)
#ifdef MIP_DEBUG_STAMPS
  const DebugSwitches sw;
  sw.tile_order(a.lods.n_tiles, a.lods.debug_tile_mult, a.lods.debug_tile_add);
  a.debug_order = sw.reverse() ? mip::kClusterOrderReverse
                  : (sw.order && std::strcmp(sw.order, "scramble") == 0) ? mip::kClusterOrderScramble : mip::kClusterOrderNone;
#endif
  const bool relative = policy->mode == MIP_LOD_RELATIVE;
  if (int32_t rc = relative ? launch(ctx, mip::mip_cluster_count_kernel<MIP_LOD_RELATIVE>, plan.instance_tiles, stream, a)
                            : launch(ctx, mip::mip_cluster_count_kernel<MIP_LOD_DISTANCE>, plan.instance_tiles, stream, a))
    return rc;
  if (int32_t rc = second ? launch(ctx, mip::mip_cluster_scan_kernel<mip::kClusterSecond>, 1, stream, a)
                          : launch(ctx, mip::mip_cluster_scan_kernel<mip::kClusterPlain>, 1, stream, a))
    return rc;
  if (int32_t rc = launch(ctx, mip::mip_cluster_members_kernel, plan.instance_tiles, stream, a)) return rc;
  mip::ClusterConeArgs ca{};
  if (cone) {
    ca.c = a;
    ca.cones = table.d_cones;
    std::memcpy(ca.eye, cone->eye, sizeof ca.eye);
    ca.facing = cone->facing;
  }
  if (int32_t rc = cone    ? launch(ctx, mip::mip_cluster_cone_cull_kernel, plan.cull_blocks, stream, ca)
                   : second ? launch(ctx, mip::mip_cluster_retest_kernel, plan.retest_blocks, stream, a)
                   : first ? launch(ctx, mip::mip_cluster_cull_kernel<true>, plan.cull_blocks, stream, a)
                           : launch(ctx, mip::mip_cluster_cull_kernel<false>, plan.cull_blocks, stream, a))
    return rc;
  if (!list)  // (the list counts survivors, not heads)
    if (int32_t rc = first ? launch(ctx, mip::mip_cluster_heads_kernel<true>, plan.head_blocks, stream, a)
                           : launch(ctx, mip::mip_cluster_heads_kernel<false>, plan.head_blocks, stream, a))
      return rc;
  if (list) {
    mip::ClusterListArgs la{};
    la.c = a;
    la.word_member = cs.d_word_member;
    la.word_rank = cs.d_word_rank;
    la.list_tiles = cs.d_list_tiles;
    la.entries = static_cast<uint4*>(list->cluster_entries);
    la.entry_capacity = list->entry_capacity;
    la.entry_count = list->entry_count;
    la.draw_args = list->draw_args;
    la.list_stats = list->stats;
    if (int32_t rc = launch(ctx, mip::mip_cluster_list_word_members_kernel, list_plan.word_blocks, stream, la)) return rc;
    if (tlist) {
      mip::ClusterTriangleListArgs ta{};
      ta.l = la;
      ta.vertices = ctx->d_vertices;
      ta.indices = ctx->d_indices;
      ta.vertex_bytes = (unsigned long long)ctx->n_vertices * 12ull;
      ta.geometry_finite = ctx->geometry_finite ? 1u : 0u;
      std::memcpy(ta.pv, frame->pv, sizeof ta.pv);
      ta.triangle_words = cs.d_triangle_words;
      ta.nonempty = cs.d_nonempty_words;
      ta.tile_kept = cs.d_tile_triangles;
      ta.tile_tested = cs.d_tile_triangles + tlist_plan.item_tiles;
      ta.tile_clusters = cs.d_tile_clusters;
      ta.masks = static_cast<unsigned long long*>(tlist->triangle_masks);
      if (int32_t rc = launch(ctx, mip::mip_cluster_triangle_list_test_kernel, tlist_plan.test_blocks, stream, ta)) return rc;
      if (int32_t rc = launch(ctx, mip::mip_cluster_triangle_list_count_kernel, tlist_plan.count_blocks, stream, ta)) return rc;
      if (int32_t rc = launch(ctx, mip::mip_cluster_triangle_list_epilogue_kernel, 1, stream, ta)) return rc;
      if (int32_t rc = launch(ctx, mip::mip_cluster_triangle_list_write_kernel, tlist_plan.write_blocks, stream, ta)) return rc;
    } else {
      if (int32_t rc = launch(ctx, mip::mip_cluster_list_count_kernel, list_plan.word_blocks, stream, la)) return rc;
      if (int32_t rc = launch(ctx, mip::mip_cluster_list_epilogue_kernel, 1, stream, la)) return rc;
      if (int32_t rc = launch(ctx, mip::mip_cluster_list_write_kernel, list_plan.write_blocks, stream, la)) return rc;
    }
  } else if (tri) {
    mip::ClusterTriangleArgs ta{};
    ta.c = a;
    ta.vertices = ctx->d_vertices;
    ta.indices = ctx->d_indices;
    ta.vertex_bytes = (unsigned long long)ctx->n_vertices * 12ull;
    ta.geometry_finite = ctx->geometry_finite ? 1u : 0u;
    std::memcpy(ta.pv, frame->pv, sizeof ta.pv);
    ta.triangle_words = cs.d_triangle_words;
    ta.item_prefix = cs.d_item_prefix;
    ta.word_total = cs.d_word_total;
    ta.tile_kept = cs.d_tile_triangles;
    ta.tile_tested = cs.d_tile_triangles + tri_plan.item_tiles;
    ta.tri_scalars = cs.d_tri_scalars;
    ta.culled_indices = static_cast<uint32_t*>(tri->culled_indices);
    ta.index_capacity = tri->index_capacity;
    if (int32_t rc = launch(ctx, mip::mip_cluster_triangle_test_kernel, tri_plan.test_blocks, stream, ta)) return rc;
    if (int32_t rc = launch(ctx, mip::mip_cluster_triangle_scan_kernel, 1, stream, ta)) return rc;
    if (int32_t rc = launch(ctx, mip::mip_cluster_triangle_write_kernel, tri_plan.write_blocks, stream, ta)) return rc;
    if (int32_t rc = launch(ctx, mip::mip_cluster_triangle_commands_kernel, tri_plan.command_blocks, stream, ta)) return rc;
  } else {
    if (int32_t rc = first ? launch(ctx, mip::mip_cluster_epilogue_kernel<true>, 1, stream, a)
                           : launch(ctx, mip::mip_cluster_epilogue_kernel<false>, 1, stream, a))
      return rc;
    if (int32_t rc = launch(ctx, mip::mip_cluster_commands_kernel, plan.head_blocks, stream, a)) return rc;
  }
  if (first)
    if (int32_t rc = record_written(ctx, stream)) return rc;
  if (int32_t rc = finish(ctx, stream, async)) return rc;
  if (!async && *status) {  // this call's own word, and its stream has drained
    const uint32_t code = *status;
    *status = 0;
    if (code & mip::kClusterStatusDevice) return fail(ctx, MIP_ERR_DEVICE, "%s", kNotItsRecord);
    if (tlist)
      return fail(ctx, MIP_ERR_CAPACITY, "mip_list_cluster_triangles: more entries than entry_capacity (the first entry_capacity entries and masks are written), or more work items than work_capacity / 2^32 - 1 (nothing is written); stats holds the counts");
    if (list)
      return fail(ctx, MIP_ERR_CAPACITY, "mip_list_clusters: more surviving clusters than entry_capacity (the first entry_capacity entries are written), or more work items than work_capacity / 2^32 - 1 (nothing is written); stats holds the counts");
    if (tri)
      return fail(ctx, MIP_ERR_CAPACITY, "mip_cull_cluster_triangles: more surviving indices than index_capacity or 2^32 - 1 (no command and no index is written; stats[4] holds the surviving triangles), more runs than cmd_capacity (the first cmd_capacity commands and the whole stream are written), or more work items than work_capacity / 2^32 - 1 (nothing is written)");
    return fail(ctx, MIP_ERR_CAPACITY, "mip_cull_clusters: more runs than cmd_capacity (the first cmd_capacity commands are written), or more work items than work_capacity / 2^32 - 1 / the record has words for (nothing is written); stats holds the counts");
  }
  return MIP_OK;
}

// ---- mip_cull_clusters_views ----

int32_t ensure_views_scratch(MipContext* ctx, MipContext::ClusterViewScratch& vs, const mip::ClusterViewsPlan& plan) {
  const size_t cap = instance_cap(ctx);
  if (!vs.d_instances) {
    MIP_HIP(ctx, hipMalloc(&vs.d_instances, (4 * cap + 1) * 4));
    MIP_HIP(ctx, hipMalloc(&vs.d_view_mask, cap * 2));
    const size_t tiles = (cap + mip::kClusterInstanceTile - 1) / mip::kClusterInstanceTile;
    MIP_HIP(ctx, hipMalloc(&vs.d_tile_items, tiles * 8));
    MIP_HIP(ctx, hipMalloc(&vs.d_tile_members, tiles * 4));
    MIP_HIP(ctx, hipMalloc(&vs.d_scalars, mip::kClusterScWords * 4));
  }
  if (int32_t rc = grow(ctx, &vs.d_view_words, &vs.words_cap, (size_t)plan.words, 8)) return rc;
  if (int32_t rc = grow(ctx, &vs.d_tile_heads, &vs.head_rows_cap, (size_t)plan.tile_rows, 4)) return rc;
  if (int32_t rc = grow(ctx, &vs.d_tile_survivors, &vs.survivor_rows_cap, (size_t)plan.tile_rows, 4)) return rc;
  return MIP_OK;
}

template <class Kernel>
int32_t launch_views(MipContext* ctx, Kernel kernel, const mip::ClusterViewsLaunch& l, hipStream_t stream, const mip::ClusterViewArgs& a) {
  hipLaunchKernelGGL(kernel, dim3(l.blocks_x, l.blocks_y), dim3(mip::kClusterThreads), 0, stream, a);
  MIP_HIP(ctx, hipGetLastError());
  return MIP_OK;
}

// Every check first (a refused call writes nothing), then the seven launches of the plan on the context's first stream.
int32_t cull_clusters_views(MipContext* ctx, const MipFrame* frames, const uint32_t* const* visible_bitmaps, uint32_t n_views,
                            const MipLodPolicy* policy, const MipClusterViewOutputs* out) {
  if (!frames || !visible_bitmaps || !out) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "frames/visible_bitmaps/out is NULL");
  if (out->struct_size != sizeof(MipClusterViewOutputs))
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "MipClusterViewOutputs.struct_size %u != %zu", out->struct_size, sizeof(MipClusterViewOutputs));
  if (out->flags & ~(MIP_OUT_DEVICE | MIP_OUT_ASYNC)) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "unknown MipClusterViewOutputs flags 0x%x", out->flags);
  if (!(out->flags & MIP_OUT_DEVICE)) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "mip_cull_clusters_views needs MIP_OUT_DEVICE outputs");
  if (!out->cluster_cmds || !out->cmd_counts) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "cluster_cmds/cmd_counts is NULL");
  if ((uintptr_t)out->cluster_cmds % 4u != 0u || (uintptr_t)out->cmd_counts % 4u != 0u || (uintptr_t)out->stats % 4u != 0u)
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "an output is not 4-byte aligned");
  if (n_views == 0 || n_views > MIP_MAX_VIEWS) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "n_views %u outside 1..%u", n_views, (unsigned)MIP_MAX_VIEWS);
  if (!ctx->have_instances || !ctx->have_meshes) return fail(ctx, MIP_ERR_NOT_READY, "instances or mesh table not set");
  if (!ctx->clusters.valid) return fail(ctx, MIP_ERR_NOT_READY, "no cluster table, or the mesh table / geometry changed since mip_build_clusters");
  if (int32_t rc = bind_device(ctx)) return rc;

  hipStream_t stream = ctx->stream;
  const bool async = (out->flags & MIP_OUT_ASYNC) != 0;
  const uint32_t n = ctx->n;
  const size_t stats_bytes = (2 + 2 * (size_t)n_views) * 4;
  if (n == 0) {  // nothing to test: zeros
    MIP_HIP(ctx, hipMemsetAsync(out->cmd_counts, 0, (size_t)n_views * 4, stream));
    if (out->stats) MIP_HIP(ctx, hipMemsetAsync(out->stats, 0, stats_bytes, stream));
    return finish(ctx, stream, async);
  }
  if (!ctx->h_cluster_views_status) {
    MIP_HIP(ctx, hipHostMalloc(&ctx->h_cluster_views_status, 2 * 4, hipHostMallocMapped));
    std::memset(ctx->h_cluster_views_status, 0, 2 * 4);
  }
  const MipContext::ClusterTable& table = ctx->clusters;
  const unsigned long long bound = mip::cluster_work_bound(n, table.max_clusters, out->work_capacity);
  const mip::ClusterViewsPlan plan = mip::plan_cluster_views(n, bound, n_views);
  MipContext::ClusterViewScratch& vs = ctx->cluster_views;
  if (int32_t rc = ensure_views_scratch(ctx, vs, plan)) return rc;

  mip::ClusterViewArgs va{};
  mip::ClusterArgs& a = va.c;
  a.lods.chain = ctx->d_mesh_chain;
  a.lods.bucket_lod = ctx->d_bucket_lod;
  std::memcpy(a.lods.switch_sq, policy->switch_sq, sizeof a.lods.switch_sq);
  a.lods.pos = ctx->d_pos; a.lods.rot = ctx->d_rot; a.lods.scale = ctx->d_scale; a.lods.mesh_id = ctx->d_mesh_id;
  a.lods.meshes = ctx->d_meshes; a.lods.mesh_draw = ctx->d_mesh_draw;
  a.lods.n = n;
  a.lods.n_tiles = plan.one.instance_tiles;
  a.lods.n_buckets = (uint32_t)ctx->lod_buckets;
  std::memcpy(a.lods.cam, frames[0].cam_pos, sizeof a.lods.cam);  // one level for all views
  a.cluster_base = table.d_cluster_base;
  a.boxes = table.d_boxes;
  a.bound = bound;
  const size_t cap = instance_cap(ctx);
  a.items = vs.d_instances;
  a.bucket = vs.d_instances + cap;
  a.member_inst = vs.d_instances + 2 * cap;
  a.member_first = vs.d_instances + 3 * cap;  // cap + 1 words
  a.tile_items = vs.d_tile_items;
  a.tile_members = vs.d_tile_members;
  a.scalars = vs.d_scalars;
  a.tile_heads = vs.d_tile_heads;
  a.tile_survivors = vs.d_tile_survivors;
  a.cmds = static_cast<uint32_t*>(out->cluster_cmds);
  a.cmd_capacity = out->cmd_stride;
  a.cmd_count = out->cmd_counts;
  a.stats = out->stats;
  va.n_views = n_views;
  va.head_tiles = plan.one.head_tiles;
  va.words_stride = plan.one.survive_words;
  va.view_words = vs.d_view_words;
  va.view_mask = vs.d_view_mask;
  for (uint32_t v = 0; v < n_views; ++v) {
    va.view_bitmap[v] = visible_bitmaps[v];
    va.view_base[v] = frames[v].first_instance_base;
    std::memcpy(va.view_planes[v], frames[v].planes, sizeof va.view_planes[v]);
  }
  volatile uint32_t* status = ctx->h_cluster_views_status + (async ? 0u : 1u);
  MIP_HIP(ctx, hipHostGetDevicePointer(reinterpret_cast<void**>(&a.status), const_cast<uint32_t*>(status), 0));
  if (!async) *status = 0;  // (no synchronous call is in flight: each one drains the stream)
#ifdef MIP_DEBUG_STAMPS
  const DebugSwitches sw;
  sw.tile_order(a.lods.n_tiles, a.lods.debug_tile_mult, a.lods.debug_tile_add);
  a.debug_order = sw.reverse() ? mip::kClusterOrderReverse
                  : (sw.order && std::strcmp(sw.order, "scramble") == 0) ? mip::kClusterOrderScramble : mip::kClusterOrderNone;
#endif
  const bool relative = policy->mode == MIP_LOD_RELATIVE;
  for (const mip::ClusterViewsLaunch& l : plan.launches) {
    int32_t rc = MIP_OK;
    switch (l.kernel) {
      case mip::ClusterViewsKernel::count:
        rc = relative ? launch_views(ctx, mip::mip_cluster_views_count_kernel<MIP_LOD_RELATIVE>, l, stream, va)
                      : launch_views(ctx, mip::mip_cluster_views_count_kernel<MIP_LOD_DISTANCE>, l, stream, va);
        break;
      // scan and members are the plain call's instantiations: they read the leading block only
      case mip::ClusterViewsKernel::scan: rc = launch(ctx, mip::mip_cluster_scan_kernel<mip::kClusterPlain>, l.blocks_x, stream, a); break;
      case mip::ClusterViewsKernel::members: rc = launch(ctx, mip::mip_cluster_members_kernel, l.blocks_x, stream, a); break;
      case mip::ClusterViewsKernel::cull: rc = launch_views(ctx, mip::mip_cluster_views_cull_kernel, l, stream, va); break;
      case mip::ClusterViewsKernel::heads: rc = launch_views(ctx, mip::mip_cluster_views_heads_kernel, l, stream, va); break;
      case mip::ClusterViewsKernel::epilogue: rc = launch_views(ctx, mip::mip_cluster_views_epilogue_kernel, l, stream, va); break;
      case mip::ClusterViewsKernel::commands: rc = launch_views(ctx, mip::mip_cluster_views_commands_kernel, l, stream, va); break;
    }
    if (rc) return rc;
  }
  if (int32_t rc = finish(ctx, stream, async)) return rc;
  if (!async && *status) {  // this call's own word, and its stream has drained
    *status = 0;
    return fail(ctx, MIP_ERR_CAPACITY, "mip_cull_clusters_views: a view has more runs than cmd_stride (its first cmd_stride commands are written, the other views are complete), or more work items than work_capacity / 2^32 - 1 (nothing is written); stats holds the counts");
  }
  return MIP_OK;
}

// ---- mip_list_clusters_views ----

// What mip_list_clusters_views takes on top of the several-view scratch (cluster_views_list_plan.hpp): (1 + n_views) x 4 bytes
// per 64 work items of the bound, and n_views rows of list tiles.
int32_t ensure_views_list_scratch(MipContext* ctx, MipContext::ClusterViewScratch& vs, const mip::ClusterViewsListPlan& plan) {
  if (int32_t rc = grow(ctx, &vs.d_word_member, &vs.word_member_cap, (size_t)plan.member_words, 4)) return rc;
  if (int32_t rc = grow(ctx, &vs.d_word_rank, &vs.word_rank_cap, (size_t)plan.rank_words, 4)) return rc;
  if (int32_t rc = grow(ctx, &vs.d_list_tiles, &vs.list_tiles_cap, (size_t)plan.tile_rows, 4)) return rc;
  return MIP_OK;
}

template <class Kernel, class Args>
int32_t launch_grid(MipContext* ctx, Kernel kernel, uint32_t blocks_x, uint32_t blocks_y, hipStream_t stream, const Args& a) {
  hipLaunchKernelGGL(kernel, dim3(blocks_x, blocks_y), dim3(mip::kClusterThreads), 0, stream, a);
  MIP_HIP(ctx, hipGetLastError());
  return MIP_OK;
}

// Every check first (a refused call writes nothing), then the eight launches of the plan on the context's first stream: the
// several-view call's front with its own argument block (filled here as cull_clusters_views fills it — duplicated, so that
// call stays as it is), then the list tail.
int32_t list_clusters_views(MipContext* ctx, const MipFrame* frames, const uint32_t* const* visible_bitmaps, uint32_t n_views,
                            const MipLodPolicy* policy, const MipClusterViewListOutputs* out) {
  if (!frames || !visible_bitmaps || !out) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "frames/visible_bitmaps/out is NULL");
  if (out->struct_size != sizeof(MipClusterViewListOutputs))
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "MipClusterViewListOutputs.struct_size %u != %zu", out->struct_size, sizeof(MipClusterViewListOutputs));
  if (out->flags & ~(MIP_OUT_DEVICE | MIP_OUT_ASYNC)) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "unknown MipClusterViewListOutputs flags 0x%x", out->flags);
  if (!(out->flags & MIP_OUT_DEVICE)) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "mip_list_clusters_views needs MIP_OUT_DEVICE outputs");
  if (!out->cluster_entries || !out->entry_counts) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "cluster_entries/entry_counts is NULL");
  if ((uintptr_t)out->cluster_entries % 16u != 0u) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "cluster_entries is not 16-byte aligned");
  if ((uintptr_t)out->entry_counts % 4u != 0u || (uintptr_t)out->draw_args % 4u != 0u || (uintptr_t)out->stats % 4u != 0u)
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "entry_counts, draw_args or stats is not 4-byte aligned");
  if (n_views == 0 || n_views > MIP_MAX_VIEWS) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "n_views %u outside 1..%u", n_views, (unsigned)MIP_MAX_VIEWS);
  if (!mip::cluster_views_list_fits(n_views, out->entry_stride))
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "n_views %u x entry_stride %u >= 2^32: the last view's firstInstance would not fit", n_views, out->entry_stride);
  if (!ctx->have_instances || !ctx->have_meshes) return fail(ctx, MIP_ERR_NOT_READY, "instances or mesh table not set");
  if (!ctx->clusters.valid) return fail(ctx, MIP_ERR_NOT_READY, "no cluster table, or the mesh table / geometry changed since mip_build_clusters");
  if (int32_t rc = bind_device(ctx)) return rc;

  hipStream_t stream = ctx->stream;
  const bool async = (out->flags & MIP_OUT_ASYNC) != 0;
  const uint32_t n = ctx->n;
  if (n == 0) {  // nothing to test: zero counts, {192, 0, 0, v x entry_stride} per view, zero stats
    MIP_HIP(ctx, hipMemsetAsync(out->entry_counts, 0, (size_t)n_views * 4, stream));
    if (out->stats) MIP_HIP(ctx, hipMemsetAsync(out->stats, 0, (2 + (size_t)n_views) * 4, stream));
    if (out->draw_args) {
      MIP_HIP(ctx, hipMemsetAsync(out->draw_args, 0, (size_t)n_views * 16, stream));
      for (uint32_t v = 0; v < n_views; ++v) {
        MIP_HIP(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(out->draw_args + 4u * v), (int)mip::kClusterListDrawVertices, 1, stream));
        MIP_HIP(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(out->draw_args + 4u * v + 3u),
                                       (int)(uint32_t)mip::cluster_views_list_first(v, out->entry_stride), 1, stream));
      }
    }
    return finish(ctx, stream, async);
  }
  if (!ctx->h_cluster_views_status) {  // the pair both several-view calls share
    MIP_HIP(ctx, hipHostMalloc(&ctx->h_cluster_views_status, 2 * 4, hipHostMallocMapped));
    std::memset(ctx->h_cluster_views_status, 0, 2 * 4);
  }
  const MipContext::ClusterTable& table = ctx->clusters;
  const unsigned long long bound = mip::cluster_work_bound(n, table.max_clusters, out->work_capacity);
  const mip::ClusterViewsListPlan plan = mip::plan_cluster_views_list(n, bound, n_views);
  MipContext::ClusterViewScratch& vs = ctx->cluster_views;
  if (int32_t rc = ensure_views_scratch(ctx, vs, plan.front)) return rc;
  if (int32_t rc = ensure_views_list_scratch(ctx, vs, plan)) return rc;

  mip::ClusterViewsListArgs la{};
  mip::ClusterViewArgs& va = la.v;
  mip::ClusterArgs& a = va.c;
  a.lods.chain = ctx->d_mesh_chain;
  a.lods.bucket_lod = ctx->d_bucket_lod;
  std::memcpy(a.lods.switch_sq, policy->switch_sq, sizeof a.lods.switch_sq);
  a.lods.pos = ctx->d_pos; a.lods.rot = ctx->d_rot; a.lods.scale = ctx->d_scale; a.lods.mesh_id = ctx->d_mesh_id;
  a.lods.meshes = ctx->d_meshes; a.lods.mesh_draw = ctx->d_mesh_draw;
  a.lods.n = n;
  a.lods.n_tiles = plan.front.one.instance_tiles;
  a.lods.n_buckets = (uint32_t)ctx->lod_buckets;
  std::memcpy(a.lods.cam, frames[0].cam_pos, sizeof a.lods.cam);  // one level for all views
  a.cluster_base = table.d_cluster_base;
  a.boxes = table.d_boxes;
  a.bound = bound;
  const size_t cap = instance_cap(ctx);
  a.items = vs.d_instances;
  a.bucket = vs.d_instances + cap;
  a.member_inst = vs.d_instances + 2 * cap;
  a.member_first = vs.d_instances + 3 * cap;  // cap + 1 words
  a.tile_items = vs.d_tile_items;
  a.tile_members = vs.d_tile_members;
  a.scalars = vs.d_scalars;
  va.n_views = n_views;
  va.head_tiles = plan.front.one.head_tiles;
  va.words_stride = plan.front.one.survive_words;
  va.view_words = vs.d_view_words;
  va.view_mask = vs.d_view_mask;
  for (uint32_t v = 0; v < n_views; ++v) {
    va.view_bitmap[v] = visible_bitmaps[v];
    va.view_base[v] = frames[v].first_instance_base;
    std::memcpy(va.view_planes[v], frames[v].planes, sizeof va.view_planes[v]);
  }
  la.word_member = vs.d_word_member;
  la.word_rank = vs.d_word_rank;
  la.list_tiles = vs.d_list_tiles;
  la.rank_stride = plan.list.words;
  la.tile_stride = plan.list.list_tiles;
  la.entries = static_cast<uint4*>(out->cluster_entries);
  la.entry_stride = out->entry_stride;
  la.entry_counts = out->entry_counts;
  la.draw_args = out->draw_args;
  la.list_stats = out->stats;
  volatile uint32_t* status = ctx->h_cluster_views_status + (async ? 0u : 1u);
  MIP_HIP(ctx, hipHostGetDevicePointer(reinterpret_cast<void**>(&a.status), const_cast<uint32_t*>(status), 0));
  if (!async) *status = 0;  // (no synchronous several-view call is in flight: each one drains the stream)
#ifdef MIP_DEBUG_STAMPS
  const DebugSwitches sw;
  sw.tile_order(a.lods.n_tiles, a.lods.debug_tile_mult, a.lods.debug_tile_add);
  a.debug_order = sw.reverse() ? mip::kClusterOrderReverse
                  : (sw.order && std::strcmp(sw.order, "scramble") == 0) ? mip::kClusterOrderScramble : mip::kClusterOrderNone;
#endif
  mip::ClusterListArgs wa{};  // the word-member kernel's: it reads the leading block and writes word_member
  wa.c = a;
  wa.word_member = vs.d_word_member;
  const bool relative = policy->mode == MIP_LOD_RELATIVE;
  for (const mip::ClusterViewsListLaunch& l : plan.launches) {
    int32_t rc = MIP_OK;
    switch (l.kernel) {
      case mip::ClusterViewsListKernel::count:
        rc = relative ? launch_grid(ctx, mip::mip_cluster_views_count_kernel<MIP_LOD_RELATIVE>, l.blocks_x, l.blocks_y, stream, va)
                      : launch_grid(ctx, mip::mip_cluster_views_count_kernel<MIP_LOD_DISTANCE>, l.blocks_x, l.blocks_y, stream, va);
        break;
      case mip::ClusterViewsListKernel::scan: rc = launch(ctx, mip::mip_cluster_scan_kernel<mip::kClusterPlain>, l.blocks_x, stream, a); break;
      case mip::ClusterViewsListKernel::members: rc = launch(ctx, mip::mip_cluster_members_kernel, l.blocks_x, stream, a); break;
      case mip::ClusterViewsListKernel::cull: rc = launch_grid(ctx, mip::mip_cluster_views_cull_kernel, l.blocks_x, l.blocks_y, stream, va); break;
      case mip::ClusterViewsListKernel::word_members: rc = launch(ctx, mip::mip_cluster_list_word_members_kernel, l.blocks_x, stream, wa); break;
      case mip::ClusterViewsListKernel::list_count: rc = launch_grid(ctx, mip::mip_cluster_views_list_count_kernel, l.blocks_x, l.blocks_y, stream, la); break;
      case mip::ClusterViewsListKernel::list_epilogue: rc = launch_grid(ctx, mip::mip_cluster_views_list_epilogue_kernel, l.blocks_x, l.blocks_y, stream, la); break;
      case mip::ClusterViewsListKernel::list_write: rc = launch_grid(ctx, mip::mip_cluster_views_list_write_kernel, l.blocks_x, l.blocks_y, stream, la); break;
    }
    if (rc) return rc;
  }
  if (int32_t rc = finish(ctx, stream, async)) return rc;
  if (!async && *status) {  // this call's own word, and its stream has drained
    *status = 0;
    return fail(ctx, MIP_ERR_CAPACITY, "mip_list_clusters_views: a view has more surviving clusters than entry_stride (its first entry_stride entries are written, the other views are complete), or more work items than work_capacity / 2^32 - 1 (nothing is written); stats holds the counts");
  }
  return MIP_OK;
}

// ---- mip_list_clusters_phase ----

// What mip_list_clusters_phase takes on top of the list's scratch (cluster_list_phase_plan.hpp).
int32_t ensure_list_phase_scratch(MipContext* ctx, MipContext::ClusterScratch& cs, const mip::ClusterListPhasePlan& plan) {
  if (!cs.d_list_phase_scalars) MIP_HIP(ctx, hipMalloc(&cs.d_list_phase_scalars, plan.scalar_words * 4));
  if (plan.first)
    if (int32_t rc = grow(ctx, &cs.d_list_candidates, &cs.list_candidates_cap, (size_t)plan.candidate_rows, 4)) return rc;
  return MIP_OK;
}

// Whether the word at `p` lies inside the `words` words at `at` (either may be null)
bool inside_words(const uint32_t* p, const uint32_t* at, uint32_t words) {
  return p && at && (uintptr_t)p >= (uintptr_t)at && (uintptr_t)p < (uintptr_t)at + 4u * (uintptr_t)words;
}

// Every check first (a refused call writes nothing), then the eight launches of the plan on the stream of the frame issued last:
// mip_cull_clusters_phase's front with the list's tail. The argument block is filled here as cull_clusters fills it —
// duplicated, so that call stays as it is.
int32_t list_clusters_phase(MipContext* ctx, const MipFrame* frame, const uint32_t* visible_bitmap, const MipLodPolicy* policy, const MipOcclusion* occ,
                            const MipClusterPhaseListOutputs* out, const MipClusterRecord* rec) {
  if (!frame || !visible_bitmap || !out) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "frame/visible_bitmap/out is NULL");
  if (out->struct_size != sizeof(MipClusterPhaseListOutputs))
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "MipClusterPhaseListOutputs.struct_size %u != %zu", out->struct_size, sizeof(MipClusterPhaseListOutputs));
  if (out->flags & ~(MIP_OUT_DEVICE | MIP_OUT_ASYNC)) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "unknown MipClusterPhaseListOutputs flags 0x%x", out->flags);
  if (!(out->flags & MIP_OUT_DEVICE)) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "mip_list_clusters_phase needs MIP_OUT_DEVICE outputs");
  if (!out->cluster_entries || !out->entry_count) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "cluster_entries/entry_count is NULL");
  if ((uintptr_t)out->cluster_entries % 16u != 0u) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "cluster_entries is not 16-byte aligned");
  if ((uintptr_t)out->entry_count % 4u != 0u || (uintptr_t)out->draw_args % 4u != 0u || (uintptr_t)out->stats % 4u != 0u || (uintptr_t)out->entry_base % 4u != 0u)
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "entry_count, draw_args, stats or entry_base is not 4-byte aligned");
  if (out->entry_base && (out->entry_base == out->entry_count || inside_words(out->entry_base, out->draw_args, 4) || inside_words(out->entry_base, out->stats, 4)))
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "entry_base is this call's entry_count or lies inside its draw_args or stats");
  if (!occ) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "mip_list_clusters_phase needs a MipOcclusion: both phases test against a pyramid");
  if (occ->struct_size != sizeof(MipOcclusion))
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "MipOcclusion.struct_size %u != %zu", occ->struct_size, sizeof(MipOcclusion));
  if (occ->width < 1u || occ->height < 1u || occ->width > MIP_MAX_DEPTH_EXTENT || occ->height > MIP_MAX_DEPTH_EXTENT)
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "depth extent %ux%u outside 1..%u", occ->width, occ->height, (unsigned)MIP_MAX_DEPTH_EXTENT);
  if (!occ->pyramid) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "pyramid is NULL");
  if (occ->flags || occ->candidates || occ->occluded_bitmap)
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "mip_list_clusters_phase takes no MipOcclusion flags, candidates or occluded_bitmap");
  if (!rec) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "rec is NULL");
  if (rec->struct_size != sizeof(MipClusterRecord))
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "MipClusterRecord.struct_size %u != %zu", rec->struct_size, sizeof(MipClusterRecord));
  if (rec->phase != MIP_CLUSTER_PHASE_FIRST && rec->phase != MIP_CLUSTER_PHASE_SECOND)
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "unknown MipClusterRecord.phase %u", rec->phase);
  if (!rec->record || (uintptr_t)rec->record % 16u != 0u) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "record is NULL or not 16-byte aligned");
  if (rec->record_bytes < mip::kClusterRecordHeaderBytes) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "record_bytes %llu < 16", (unsigned long long)rec->record_bytes);
  const bool first = rec->phase == MIP_CLUSTER_PHASE_FIRST;
  if (!ctx->have_instances || !ctx->have_meshes) return fail(ctx, MIP_ERR_NOT_READY, "instances or mesh table not set");
  if (!ctx->clusters.valid) return fail(ctx, MIP_ERR_NOT_READY, "no cluster table, or the mesh table / geometry changed since mip_build_clusters");
  if (int32_t rc = bind_device(ctx)) return rc;

  const uint32_t slot = ctx->last_slot;
  hipStream_t stream = ctx->slots[slot].stream;
  const bool async = (out->flags & MIP_OUT_ASYNC) != 0;
  const uint32_t n = ctx->n;
  // SECOND goes behind the FIRST call that wrote the record (and its entry_count, which may be this call's entry_base),
  // whichever slot's stream that call ran on
  if (!first && ctx->cluster_record_written) MIP_HIP(ctx, hipStreamWaitEvent(stream, ctx->cluster_record_written, 0));
  if (n == 0) {  // nothing to test: a zero count, {192, 0, 0, b}, zero stats; FIRST: a zero header
    MIP_HIP(ctx, hipMemsetAsync(out->entry_count, 0, 4, stream));
    if (out->stats) MIP_HIP(ctx, hipMemsetAsync(out->stats, 0, 16, stream));
    if (out->draw_args) {
      MIP_HIP(ctx, hipMemsetAsync(out->draw_args, 0, 16, stream));
      MIP_HIP(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(out->draw_args), (int)mip::kClusterListDrawVertices, 1, stream));
      if (out->entry_base) MIP_HIP(ctx, hipMemcpyAsync(out->draw_args + 3, out->entry_base, 4, hipMemcpyDeviceToDevice, stream));  // b, on the device
    }
    if (first) {
      MIP_HIP(ctx, hipMemsetAsync(rec->record, 0, mip::kClusterRecordHeaderBytes, stream));
      if (int32_t rc = record_written(ctx, stream)) return rc;
    }
    return finish(ctx, stream, async);
  }
  if (!ctx->h_cluster_status) {
    MIP_HIP(ctx, hipHostMalloc(&ctx->h_cluster_status, kStatusWords * 4, hipHostMallocMapped));
    std::memset(ctx->h_cluster_status, 0, kStatusWords * 4);
  }
  const MipContext::ClusterTable& table = ctx->clusters;
  unsigned long long bound = mip::cluster_work_bound(n, table.max_clusters, out->work_capacity);
  {  // a W the record has no words for is a work overflow
    const unsigned long long room = mip::cluster_record_items(rec->record_bytes);
    bound = room < bound ? room : bound;
  }
  const mip::ClusterListPhasePlan plan = mip::plan_cluster_list_phase(n, bound, first);
  if (ctx->cluster_scratch.size() != ctx->slots.size()) ctx->cluster_scratch.resize(ctx->slots.size());
  MipContext::ClusterScratch& cs = ctx->cluster_scratch[slot];
  if (int32_t rc = ensure_scratch(ctx, cs, plan.front, false)) return rc;
  if (int32_t rc = ensure_list_scratch(ctx, cs, plan.list)) return rc;
  if (int32_t rc = ensure_list_phase_scratch(ctx, cs, plan)) return rc;
  if (ctx->next_slot != slot) {
    // a pyramid built for the next run sits on that slot's stream: this call goes behind what that stream holds now
    if (!ctx->cluster_pyramid_ready) MIP_HIP(ctx, hipEventCreateWithFlags(&ctx->cluster_pyramid_ready, hipEventDisableTiming));
    MIP_HIP(ctx, hipEventRecord(ctx->cluster_pyramid_ready, ctx->slots[ctx->next_slot].stream));
    MIP_HIP(ctx, hipStreamWaitEvent(stream, ctx->cluster_pyramid_ready, 0));
  }

  mip::ClusterListPhaseArgs pa{};
  mip::ClusterListArgs& la = pa.l;
  mip::ClusterArgs& a = la.c;
  a.lods.chain = ctx->d_mesh_chain;
  a.lods.bucket_lod = ctx->d_bucket_lod;
  std::memcpy(a.lods.switch_sq, policy->switch_sq, sizeof a.lods.switch_sq);
  a.lods.pos = ctx->d_pos; a.lods.rot = ctx->d_rot; a.lods.scale = ctx->d_scale; a.lods.mesh_id = ctx->d_mesh_id;
  a.lods.meshes = ctx->d_meshes; a.lods.mesh_draw = ctx->d_mesh_draw;
  a.lods.bitmap = visible_bitmap;
  a.lods.n = n;
  a.lods.n_tiles = plan.front.instance_tiles;
  a.lods.n_buckets = (uint32_t)ctx->lod_buckets;
  a.lods.first_instance_base = frame->first_instance_base;
  std::memcpy(a.lods.cam, frame->cam_pos, sizeof a.lods.cam);
  a.cluster_base = table.d_cluster_base;
  a.boxes = table.d_boxes;
  if (first) std::memcpy(a.planes, frame->planes, sizeof a.planes);  // SECOND does not read them
  std::memcpy(a.pv, occ->pv, sizeof a.pv);
  a.pyramid = static_cast<const float*>(occ->pyramid);
  a.width = occ->width;
  a.height = occ->height;
  a.bound = bound;
  const size_t cap = instance_cap(ctx);
  a.items = cs.d_instances;
  a.bucket = cs.d_instances + cap;
  a.member_inst = cs.d_instances + 2 * cap;
  a.member_first = cs.d_instances + 3 * cap;  // cap + 1 words
  a.tile_items = cs.d_tile_items;
  a.tile_members = cs.d_tile_members;
  a.scalars = cs.d_scalars;
  a.words = static_cast<ulonglong2*>(cs.d_words);
  a.record_header = static_cast<uint32_t*>(rec->record);
  a.record_words = reinterpret_cast<unsigned long long*>(static_cast<char*>(rec->record) + mip::kClusterRecordHeaderBytes);
  la.word_member = cs.d_word_member;
  la.word_rank = cs.d_word_rank;
  la.list_tiles = cs.d_list_tiles;
  la.entries = static_cast<uint4*>(out->cluster_entries);
  la.entry_capacity = out->entry_capacity;
  la.entry_count = out->entry_count;
  la.draw_args = out->draw_args;
  la.list_stats = out->stats;
  pa.entry_base = out->entry_base;
  pa.list_candidates = cs.d_list_candidates;
  pa.phase_scalars = cs.d_list_phase_scalars;
  volatile uint32_t* status = ctx->h_cluster_status + 2u * slot + (async ? 0u : 1u);  // slot < MIP_MAX_FRAMES_IN_FLIGHT
  MIP_HIP(ctx, hipHostGetDevicePointer(reinterpret_cast<void**>(&a.status), const_cast<uint32_t*>(status), 0));
  if (!async) *status = 0;  // (no synchronous call of the slot is in flight: each one drains its stream)
#ifdef MIP_DEBUG_STAMPS
  const DebugSwitches sw;
  sw.tile_order(a.lods.n_tiles, a.lods.debug_tile_mult, a.lods.debug_tile_add);
  a.debug_order = sw.reverse() ? mip::kClusterOrderReverse
                  : (sw.order && std::strcmp(sw.order, "scramble") == 0) ? mip::kClusterOrderScramble : mip::kClusterOrderNone;
#endif
  const bool relative = policy->mode == MIP_LOD_RELATIVE;
  for (const mip::ClusterListPhaseLaunch& l : plan.launches) {
    int32_t rc = MIP_OK;
    switch (l.kernel) {
      // count, scan and members are mip_cull_clusters_phase's instantiations, word_members is mip_list_clusters': they read
      // the leading blocks only
      case mip::ClusterListPhaseKernel::count:
        rc = relative ? launch(ctx, mip::mip_cluster_count_kernel<MIP_LOD_RELATIVE>, l.blocks, stream, a)
                      : launch(ctx, mip::mip_cluster_count_kernel<MIP_LOD_DISTANCE>, l.blocks, stream, a);
        break;
      case mip::ClusterListPhaseKernel::scan:
        rc = first ? launch(ctx, mip::mip_cluster_scan_kernel<mip::kClusterPlain>, l.blocks, stream, a)
                   : launch(ctx, mip::mip_cluster_scan_kernel<mip::kClusterSecond>, l.blocks, stream, a);
        break;
      case mip::ClusterListPhaseKernel::members: rc = launch(ctx, mip::mip_cluster_members_kernel, l.blocks, stream, a); break;
      case mip::ClusterListPhaseKernel::word_members: rc = launch(ctx, mip::mip_cluster_list_word_members_kernel, l.blocks, stream, la); break;
      case mip::ClusterListPhaseKernel::front:
        rc = first ? launch(ctx, mip::mip_cluster_list_phase_cull_kernel, l.blocks, stream, pa)
                   : launch(ctx, mip::mip_cluster_list_phase_retest_kernel, l.blocks, stream, pa);
        break;
      case mip::ClusterListPhaseKernel::list_count:
        rc = first ? launch(ctx, mip::mip_cluster_list_phase_count_kernel<true>, l.blocks, stream, pa)
                   : launch(ctx, mip::mip_cluster_list_phase_count_kernel<false>, l.blocks, stream, pa);
        break;
      case mip::ClusterListPhaseKernel::list_epilogue:
        rc = first ? launch(ctx, mip::mip_cluster_list_phase_epilogue_kernel<true>, l.blocks, stream, pa)
                   : launch(ctx, mip::mip_cluster_list_phase_epilogue_kernel<false>, l.blocks, stream, pa);
        break;
      case mip::ClusterListPhaseKernel::list_write: rc = launch(ctx, mip::mip_cluster_list_phase_write_kernel, l.blocks, stream, pa); break;
    }
    if (rc) return rc;
  }
  if (first)
    if (int32_t rc = record_written(ctx, stream)) return rc;
  if (int32_t rc = finish(ctx, stream, async)) return rc;
  if (!async && *status) {  // this call's own word, and its stream has drained
    const uint32_t code = *status;
    *status = 0;
    if (code & mip::kClusterStatusDevice)
      return fail(ctx, MIP_ERR_DEVICE, "mip_list_clusters_phase: the record's header names another W or another member count than this SECOND call's: it is not the record of the FIRST call over these members (a zero count is written, stats holds the call's W and members)");
    return fail(ctx, MIP_ERR_CAPACITY, "mip_list_clusters_phase: more surviving clusters than the room behind entry_base (the first `room` entries are written), or more work items than work_capacity / 2^32 - 1 / the record has words for (no entry is written); stats holds the counts");
  }
  return MIP_OK;
}

// ---- mip_list_clusters_views_occluded ----

// Every check first (a refused call writes nothing), then the eight launches of mip_list_clusters_views' plan on the context's
// first stream with mip_cluster_views_cull_occluded_packed_kernel (or, MIP_TUNE_VIEWS_OCCLUDED_PACKED=0, the simple loop of
// mip_cluster_views_cull_occluded_kernel) in the cull kernel's place (with no pyramid in any view the plain
// cull kernel stays: the same words, more waves per SIMD), behind a memset of `hidden`. The
// argument block is filled here as list_clusters_views fills its own — duplicated, so that call stays as it is.
int32_t list_clusters_views_occluded(MipContext* ctx, const MipFrame* frames, const uint32_t* const* visible_bitmaps, const MipOcclusion* const* occs,
                                     uint32_t n_views, const MipLodPolicy* policy, const MipClusterViewOccludedListOutputs* out) {
  if (!frames || !visible_bitmaps || !out) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "frames/visible_bitmaps/out is NULL");
  if (!occs) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "occs is NULL (for no pyramid at all pass an array of NULLs, or call mip_list_clusters_views)");
  if (out->struct_size != sizeof(MipClusterViewOccludedListOutputs))
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "MipClusterViewOccludedListOutputs.struct_size %u != %zu", out->struct_size, sizeof(MipClusterViewOccludedListOutputs));
  if (out->flags & ~(MIP_OUT_DEVICE | MIP_OUT_ASYNC)) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "unknown MipClusterViewOccludedListOutputs flags 0x%x", out->flags);
  if (!(out->flags & MIP_OUT_DEVICE)) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "mip_list_clusters_views_occluded needs MIP_OUT_DEVICE outputs");
  if (!out->cluster_entries || !out->entry_counts) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "cluster_entries/entry_counts is NULL");
  if ((uintptr_t)out->cluster_entries % 16u != 0u) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "cluster_entries is not 16-byte aligned");
  if ((uintptr_t)out->entry_counts % 4u != 0u || (uintptr_t)out->draw_args % 4u != 0u || (uintptr_t)out->stats % 4u != 0u || (uintptr_t)out->hidden % 4u != 0u)
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "entry_counts, draw_args, stats or hidden is not 4-byte aligned");
  if (n_views == 0 || n_views > MIP_MAX_VIEWS) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "n_views %u outside 1..%u", n_views, (unsigned)MIP_MAX_VIEWS);
  if (!mip::cluster_views_list_fits(n_views, out->entry_stride))
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "n_views %u x entry_stride %u >= 2^32: the last view's firstInstance would not fit", n_views, out->entry_stride);
  if (out->hidden)  // either range's first word inside the other: the memset of one would clear words of the other
    for (uint32_t k = 0; k < 3; ++k) {
      const uint32_t* other = k == 0 ? out->stats : k == 1 ? out->draw_args : out->entry_counts;
      const uint32_t words = k == 0 ? 2u + n_views : k == 1 ? 4u * n_views : n_views;
      if (inside_words(out->hidden, other, words) || inside_words(other, out->hidden, n_views))
        return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "hidden lies inside this call's stats, draw_args or entry_counts");
    }
  bool any_pyramid = false;
  for (uint32_t v = 0; v < n_views; ++v) {
    const MipOcclusion* occ = occs[v];
    if (!occ) continue;
    any_pyramid = true;
    if (occ->struct_size != sizeof(MipOcclusion))
      return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "view %u: MipOcclusion.struct_size %u != %zu", v, occ->struct_size, sizeof(MipOcclusion));
    if (occ->width < 1u || occ->height < 1u || occ->width > MIP_MAX_DEPTH_EXTENT || occ->height > MIP_MAX_DEPTH_EXTENT)
      return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "view %u: depth extent %ux%u outside 1..%u", v, occ->width, occ->height, (unsigned)MIP_MAX_DEPTH_EXTENT);
    if (!occ->pyramid) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "view %u: pyramid is NULL", v);
    if (occ->flags || occ->candidates || occ->occluded_bitmap)
      return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "view %u: mip_list_clusters_views_occluded takes no MipOcclusion flags, candidates or occluded_bitmap", v);
  }
  if (!ctx->have_instances || !ctx->have_meshes) return fail(ctx, MIP_ERR_NOT_READY, "instances or mesh table not set");
  if (!ctx->clusters.valid) return fail(ctx, MIP_ERR_NOT_READY, "no cluster table, or the mesh table / geometry changed since mip_build_clusters");
  if (int32_t rc = bind_device(ctx)) return rc;

  hipStream_t stream = ctx->stream;
  const bool async = (out->flags & MIP_OUT_ASYNC) != 0;
  const uint32_t n = ctx->n;
  if (out->hidden) MIP_HIP(ctx, hipMemsetAsync(out->hidden, 0, (size_t)n_views * 4, stream));  // the cull kernel adds to it; N = 0 and a work overflow leave the zeros
  if (n == 0) {  // nothing to test: zero counts, {192, 0, 0, v x entry_stride} per view, zero stats
    MIP_HIP(ctx, hipMemsetAsync(out->entry_counts, 0, (size_t)n_views * 4, stream));
    if (out->stats) MIP_HIP(ctx, hipMemsetAsync(out->stats, 0, (2 + (size_t)n_views) * 4, stream));
    if (out->draw_args) {
      MIP_HIP(ctx, hipMemsetAsync(out->draw_args, 0, (size_t)n_views * 16, stream));
      for (uint32_t v = 0; v < n_views; ++v) {
        MIP_HIP(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(out->draw_args + 4u * v), (int)mip::kClusterListDrawVertices, 1, stream));
        MIP_HIP(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(out->draw_args + 4u * v + 3u),
                                       (int)(uint32_t)mip::cluster_views_list_first(v, out->entry_stride), 1, stream));
      }
    }
    return finish(ctx, stream, async);
  }
  if (!ctx->h_cluster_views_status) {  // the pair the several-view calls share
    MIP_HIP(ctx, hipHostMalloc(&ctx->h_cluster_views_status, 2 * 4, hipHostMallocMapped));
    std::memset(ctx->h_cluster_views_status, 0, 2 * 4);
  }
  const MipContext::ClusterTable& table = ctx->clusters;
  const unsigned long long bound = mip::cluster_work_bound(n, table.max_clusters, out->work_capacity);
  const mip::ClusterViewsListPlan plan = mip::plan_cluster_views_list(n, bound, n_views);
  MipContext::ClusterViewScratch& vs = ctx->cluster_views;
  if (int32_t rc = ensure_views_scratch(ctx, vs, plan.front)) return rc;
  if (int32_t rc = ensure_views_list_scratch(ctx, vs, plan)) return rc;
  if (any_pyramid && ctx->slots[ctx->next_slot].stream != stream) {
    // a pyramid built for the next run sits on that slot's stream: this call goes behind what that stream holds now
    if (!ctx->cluster_pyramid_ready) MIP_HIP(ctx, hipEventCreateWithFlags(&ctx->cluster_pyramid_ready, hipEventDisableTiming));
    MIP_HIP(ctx, hipEventRecord(ctx->cluster_pyramid_ready, ctx->slots[ctx->next_slot].stream));
    MIP_HIP(ctx, hipStreamWaitEvent(stream, ctx->cluster_pyramid_ready, 0));
  }

  mip::ClusterViewsListArgs la{};
  mip::ClusterViewArgs& va = la.v;
  mip::ClusterArgs& a = va.c;
  a.lods.chain = ctx->d_mesh_chain;
  a.lods.bucket_lod = ctx->d_bucket_lod;
  std::memcpy(a.lods.switch_sq, policy->switch_sq, sizeof a.lods.switch_sq);
  a.lods.pos = ctx->d_pos; a.lods.rot = ctx->d_rot; a.lods.scale = ctx->d_scale; a.lods.mesh_id = ctx->d_mesh_id;
  a.lods.meshes = ctx->d_meshes; a.lods.mesh_draw = ctx->d_mesh_draw;
  a.lods.n = n;
  a.lods.n_tiles = plan.front.one.instance_tiles;
  a.lods.n_buckets = (uint32_t)ctx->lod_buckets;
  std::memcpy(a.lods.cam, frames[0].cam_pos, sizeof a.lods.cam);  // one level for all views
  a.cluster_base = table.d_cluster_base;
  a.boxes = table.d_boxes;
  a.bound = bound;
  const size_t cap = instance_cap(ctx);
  a.items = vs.d_instances;
  a.bucket = vs.d_instances + cap;
  a.member_inst = vs.d_instances + 2 * cap;
  a.member_first = vs.d_instances + 3 * cap;  // cap + 1 words
  a.tile_items = vs.d_tile_items;
  a.tile_members = vs.d_tile_members;
  a.scalars = vs.d_scalars;
  va.n_views = n_views;
  va.head_tiles = plan.front.one.head_tiles;
  va.words_stride = plan.front.one.survive_words;
  va.view_words = vs.d_view_words;
  va.view_mask = vs.d_view_mask;
  for (uint32_t v = 0; v < n_views; ++v) {
    va.view_bitmap[v] = visible_bitmaps[v];
    va.view_base[v] = frames[v].first_instance_base;
    std::memcpy(va.view_planes[v], frames[v].planes, sizeof va.view_planes[v]);
  }
  la.word_member = vs.d_word_member;
  la.word_rank = vs.d_word_rank;
  la.list_tiles = vs.d_list_tiles;
  la.rank_stride = plan.list.words;
  la.tile_stride = plan.list.list_tiles;
  la.entries = static_cast<uint4*>(out->cluster_entries);
  la.entry_stride = out->entry_stride;
  la.entry_counts = out->entry_counts;
  la.draw_args = out->draw_args;
  la.list_stats = out->stats;
  volatile uint32_t* status = ctx->h_cluster_views_status + (async ? 0u : 1u);
  MIP_HIP(ctx, hipHostGetDevicePointer(reinterpret_cast<void**>(&a.status), const_cast<uint32_t*>(status), 0));
  if (!async) *status = 0;  // (no synchronous several-view call is in flight: each one drains the stream)
#ifdef MIP_DEBUG_STAMPS
  const DebugSwitches sw;
  sw.tile_order(a.lods.n_tiles, a.lods.debug_tile_mult, a.lods.debug_tile_add);
  a.debug_order = sw.reverse() ? mip::kClusterOrderReverse
                  : (sw.order && std::strcmp(sw.order, "scramble") == 0) ? mip::kClusterOrderScramble : mip::kClusterOrderNone;
#endif
  mip::ClusterListArgs wa{};  // the word-member kernel's: it reads the leading block and writes word_member
  wa.c = a;
  wa.word_member = vs.d_word_member;
  mip::ClusterViewOccludedArgs oa{};  // the cull kernel's: the front's block, then a pyramid per view
  oa.v = va;
  for (uint32_t v = 0; v < n_views; ++v)
    if (const MipOcclusion* occ = occs[v]) {
      std::memcpy(oa.occ[v].pv, occ->pv, sizeof oa.occ[v].pv);
      oa.occ[v].pyramid = static_cast<const float*>(occ->pyramid);
      oa.occ[v].width = occ->width;
      oa.occ[v].height = occ->height;
    }
  oa.hidden = out->hidden;
  const bool relative = policy->mode == MIP_LOD_RELATIVE;
  const char* tune = std::getenv("MIP_TUNE_VIEWS_OCCLUDED_PACKED");  // A/B and tests: 0 = the simple loop; the packed cull kernel is the default
  const bool packed = tune ? std::atoi(tune) != 0 : true;
  const bool always = std::getenv("MIP_TUNE_VIEWS_OCCLUDED_ALWAYS") != nullptr;  // A/B and tests: the occluded kernel even when no view has a pyramid
  for (const mip::ClusterViewsListLaunch& l : plan.launches) {
    int32_t rc = MIP_OK;
    switch (l.kernel) {
      case mip::ClusterViewsListKernel::count:
        rc = relative ? launch_grid(ctx, mip::mip_cluster_views_count_kernel<MIP_LOD_RELATIVE>, l.blocks_x, l.blocks_y, stream, va)
                      : launch_grid(ctx, mip::mip_cluster_views_count_kernel<MIP_LOD_DISTANCE>, l.blocks_x, l.blocks_y, stream, va);
        break;
      case mip::ClusterViewsListKernel::scan: rc = launch(ctx, mip::mip_cluster_scan_kernel<mip::kClusterPlain>, l.blocks_x, stream, a); break;
      case mip::ClusterViewsListKernel::members: rc = launch(ctx, mip::mip_cluster_members_kernel, l.blocks_x, stream, a); break;
      // no pyramid in any view: the plain several-view cull writes the same words (hidden stays the memset's zeros) at five
      // waves per SIMD where the packed kernel holds four and the simple loop three (DESIGN section 36 has the three measured)
      case mip::ClusterViewsListKernel::cull:
        rc = !any_pyramid && !always ? launch_grid(ctx, mip::mip_cluster_views_cull_kernel, l.blocks_x, l.blocks_y, stream, va)
             : packed     ? launch_grid(ctx, mip::mip_cluster_views_cull_occluded_packed_kernel, l.blocks_x, l.blocks_y, stream, oa)
                          : launch_grid(ctx, mip::mip_cluster_views_cull_occluded_kernel, l.blocks_x, l.blocks_y, stream, oa);
        break;
      case mip::ClusterViewsListKernel::word_members: rc = launch(ctx, mip::mip_cluster_list_word_members_kernel, l.blocks_x, stream, wa); break;
      case mip::ClusterViewsListKernel::list_count: rc = launch_grid(ctx, mip::mip_cluster_views_list_count_kernel, l.blocks_x, l.blocks_y, stream, la); break;
      case mip::ClusterViewsListKernel::list_epilogue: rc = launch_grid(ctx, mip::mip_cluster_views_list_epilogue_kernel, l.blocks_x, l.blocks_y, stream, la); break;
      case mip::ClusterViewsListKernel::list_write: rc = launch_grid(ctx, mip::mip_cluster_views_list_write_kernel, l.blocks_x, l.blocks_y, stream, la); break;
    }
    if (rc) return rc;
  }
  if (int32_t rc = finish(ctx, stream, async)) return rc;
  if (!async && *status) {  // this call's own word, and its stream has drained
    *status = 0;
    return fail(ctx, MIP_ERR_CAPACITY, "mip_list_clusters_views_occluded: a view has more surviving clusters than entry_stride (its first entry_stride entries are written, the other views are complete), or more work items than work_capacity / 2^32 - 1 (nothing is written); stats holds the counts");
  }
  return MIP_OK;
}

}  // namespace

// mip_wait, after every stream has drained. An overflow of an asynchronous call is reported when nothing else is: while `rc`
// is another error the words stay as they are, and the mip_wait after it reports the overflow — it is never lost.
int32_t cluster_wait_status(MipContext* ctx, int32_t rc) {
  if (rc != MIP_OK) return rc;
  uint32_t raised = 0;
  if (ctx->h_cluster_status)
    for (uint32_t k = 0; k < kStatusWords; k += 2) {
      raised |= ((volatile uint32_t*)ctx->h_cluster_status)[k];
      ((volatile uint32_t*)ctx->h_cluster_status)[k] = 0;
    }
  if (ctx->h_cluster_views_status) {  // the several-view calls' asynchronous word
    raised |= ((volatile uint32_t*)ctx->h_cluster_views_status)[0];
    ((volatile uint32_t*)ctx->h_cluster_views_status)[0] = 0;
  }
  if (!raised) return MIP_OK;
  if (raised & mip::kClusterStatusDevice) return fail(ctx, MIP_ERR_DEVICE, "asynchronous %s", kNotItsRecord);
  return fail(ctx, MIP_ERR_CAPACITY, "an asynchronous mip_cull_clusters, mip_list_clusters, mip_list_cluster_triangles, mip_list_clusters_phase, mip_cull_clusters_views, mip_list_clusters_views or mip_list_clusters_views_occluded had more runs than cmd_capacity (more surviving clusters than entry_capacity / entry_stride / the room behind entry_base), or more work items than work_capacity / 2^32 - 1; its stats hold the counts");
}

void cluster_release(MipContext* ctx) {
  (void)hipFree(ctx->clusters.d_boxes);
  (void)hipFree(ctx->clusters.d_cluster_base);
  (void)hipFree(ctx->clusters.d_cones);
  ctx->clusters = MipContext::ClusterTable{};
  for (auto& cs : ctx->cluster_scratch) {
    (void)hipFree(cs.d_instances);
    (void)hipFree(cs.d_tile_items);
    (void)hipFree(cs.d_tile_members);
    (void)hipFree(cs.d_scalars);
    (void)hipFree(cs.d_words);
    (void)hipFree(cs.d_tile_heads);
    (void)hipFree(cs.d_tile_survivors);
    (void)hipFree(cs.d_tile_candidates);
    (void)hipFree(cs.d_tri_scalars);
    (void)hipFree(cs.d_triangle_words);
    (void)hipFree(cs.d_item_prefix);
    (void)hipFree(cs.d_word_total);
    (void)hipFree(cs.d_tile_triangles);
    (void)hipFree(cs.d_word_member);
    (void)hipFree(cs.d_word_rank);
    (void)hipFree(cs.d_list_tiles);
    (void)hipFree(cs.d_list_candidates);
    (void)hipFree(cs.d_list_phase_scalars);
    (void)hipFree(cs.d_nonempty_words);
    (void)hipFree(cs.d_tile_clusters);
  }
  ctx->cluster_scratch.clear();
  {
    MipContext::ClusterViewScratch& vs = ctx->cluster_views;
    (void)hipFree(vs.d_instances);
    (void)hipFree(vs.d_view_mask);
    (void)hipFree(vs.d_tile_items);
    (void)hipFree(vs.d_tile_members);
    (void)hipFree(vs.d_scalars);
    (void)hipFree(vs.d_view_words);
    (void)hipFree(vs.d_tile_heads);
    (void)hipFree(vs.d_tile_survivors);
    (void)hipFree(vs.d_word_member);
    (void)hipFree(vs.d_word_rank);
    (void)hipFree(vs.d_list_tiles);
    vs = MipContext::ClusterViewScratch{};
  }
  if (ctx->h_cluster_views_status) (void)hipHostFree(ctx->h_cluster_views_status);
  ctx->h_cluster_views_status = nullptr;
  if (ctx->h_cluster_status) (void)hipHostFree(ctx->h_cluster_status);
  ctx->h_cluster_status = nullptr;
  if (ctx->cluster_pyramid_ready) (void)hipEventDestroy(ctx->cluster_pyramid_ready);
  ctx->cluster_pyramid_ready = nullptr;
  if (ctx->cluster_record_written) (void)hipEventDestroy(ctx->cluster_record_written);
  ctx->cluster_record_written = nullptr;
}

}  // namespace mip_host

using namespace mip_host;

extern "C" {

int32_t mip_build_clusters(MipContext* ctx) {
  if (!ctx) return MIP_ERR_INVALID_ARGUMENT;
  return build_clusters(ctx);
}

uint32_t mip_cluster_count(const MipContext* ctx) { return ctx && ctx->clusters.valid ? ctx->clusters.total : 0u; }

int32_t mip_read_cluster_boxes(MipContext* ctx, float* host_out, uint32_t capacity_clusters) {
  if (!ctx) return MIP_ERR_INVALID_ARGUMENT;
  if (!ctx->clusters.valid) return fail(ctx, MIP_ERR_NOT_READY, "no cluster table, or the mesh table / geometry changed since mip_build_clusters");
  const uint32_t total = ctx->clusters.total;
  if (capacity_clusters < total) return fail(ctx, MIP_ERR_CAPACITY, "%u clusters, room for %u", total, capacity_clusters);
  if (!total) return MIP_OK;
  if (!host_out) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "host_out is NULL");
  if (int32_t rc = bind_device(ctx)) return rc;
  std::vector<float4> boxes((size_t)total * 2);
  MIP_HIP(ctx, hipMemcpy(boxes.data(), ctx->clusters.d_boxes, boxes.size() * sizeof(float4), hipMemcpyDeviceToHost));
  for (size_t g = 0; g < total; ++g) {
    const float4 lo = boxes[2 * g], hi = boxes[2 * g + 1];
    float* o = host_out + 6 * g;
    o[0] = lo.x; o[1] = lo.y; o[2] = lo.z;
    o[3] = hi.x; o[4] = hi.y; o[5] = hi.z;
  }
  return MIP_OK;
}

int32_t mip_build_cluster_cones(MipContext* ctx) {
  if (!ctx) return MIP_ERR_INVALID_ARGUMENT;
  return build_cluster_cones(ctx);
}

int32_t mip_read_cluster_cones(MipContext* ctx, float* host_out, uint32_t capacity_clusters) {
  if (!ctx) return MIP_ERR_INVALID_ARGUMENT;
  if (!ctx->clusters.valid || !ctx->clusters.cones_valid)
    return fail(ctx, MIP_ERR_NOT_READY, "no cone table, or the cluster table changed since mip_build_cluster_cones");
  const uint32_t total = ctx->clusters.total;
  if (capacity_clusters < total) return fail(ctx, MIP_ERR_CAPACITY, "%u clusters, room for %u", total, capacity_clusters);
  if (!total) return MIP_OK;
  if (!host_out) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "host_out is NULL");
  if (int32_t rc = bind_device(ctx)) return rc;
  MIP_HIP(ctx, hipMemcpy(host_out, ctx->clusters.d_cones, (size_t)total * 2 * sizeof(float4), hipMemcpyDeviceToHost));  // 8 floats per cluster, as stored
  return MIP_OK;
}

int32_t mip_cone_from_pv(const float pv[16], MipClusterCone* out) {
  if (!pv || !out) return MIP_ERR_INVALID_ARGUMENT;
  float m[16], eye[3], facing;
  std::memcpy(m, pv, sizeof m);
  if (!mip::cone_from_pv(m, eye, facing)) return MIP_ERR_INVALID_ARGUMENT;
  out->struct_size = sizeof(MipClusterCone);
  out->flags = 0;
  std::memcpy(out->eye, eye, sizeof eye);
  out->facing = facing;
  return MIP_OK;
}

int32_t mip_cull_clusters_cone(MipContext* ctx, const MipFrame* frame, const uint32_t* visible_bitmap, const MipLodPolicy* policy,
                               const MipOcclusion* occ, const MipClusterCone* cone, const MipClusterOutputs* out) {
  if (!ctx) return MIP_ERR_INVALID_ARGUMENT;
  if (int32_t rc = check_policy(ctx, policy)) return rc;
  return cull_clusters(ctx, frame, visible_bitmap, policy, occ, out, nullptr, false, nullptr, cone, true);
}

int32_t mip_cull_clusters(MipContext* ctx, const MipFrame* frame, const uint32_t* visible_bitmap, const MipLodPolicy* policy,
                          const MipOcclusion* occ, const MipClusterOutputs* out) {
  if (!ctx) return MIP_ERR_INVALID_ARGUMENT;
  if (int32_t rc = check_policy(ctx, policy)) return rc;
  return cull_clusters(ctx, frame, visible_bitmap, policy, occ, out, nullptr, false);
}

int32_t mip_cull_clusters_views(MipContext* ctx, const MipFrame* frames, const uint32_t* const* visible_bitmaps, uint32_t n_views,
                                const MipLodPolicy* policy, const MipClusterViewOutputs* out) {
  if (!ctx) return MIP_ERR_INVALID_ARGUMENT;
  if (int32_t rc = check_policy(ctx, policy)) return rc;
  return cull_clusters_views(ctx, frames, visible_bitmaps, n_views, policy, out);
}

int32_t mip_list_clusters_views(MipContext* ctx, const MipFrame* frames, const uint32_t* const* visible_bitmaps, uint32_t n_views,
                                const MipLodPolicy* policy, const MipClusterViewListOutputs* out) {
  if (!ctx) return MIP_ERR_INVALID_ARGUMENT;
  if (int32_t rc = check_policy(ctx, policy)) return rc;
  return list_clusters_views(ctx, frames, visible_bitmaps, n_views, policy, out);
}

int32_t mip_list_clusters_views_occluded(MipContext* ctx, const MipFrame* frames, const uint32_t* const* visible_bitmaps,
                                         const MipOcclusion* const* occs, uint32_t n_views, const MipLodPolicy* policy,
                                         const MipClusterViewOccludedListOutputs* out) {
  if (!ctx) return MIP_ERR_INVALID_ARGUMENT;
  if (int32_t rc = check_policy(ctx, policy)) return rc;
  return list_clusters_views_occluded(ctx, frames, visible_bitmaps, occs, n_views, policy, out);
}

// mip_list_clusters: the checks of its own fields, then the call it shares with mip_cull_clusters / mip_cull_clusters_cone
int32_t mip_list_clusters(MipContext* ctx, const MipFrame* frame, const uint32_t* visible_bitmap, const MipLodPolicy* policy,
                          const MipOcclusion* occ, const MipClusterCone* cone, const MipClusterListOutputs* out) {
  if (!ctx) return MIP_ERR_INVALID_ARGUMENT;
  if (int32_t rc = check_policy(ctx, policy)) return rc;
  if (!out) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "frame/visible_bitmap/out is NULL");
  if (out->struct_size != sizeof(MipClusterListOutputs))
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "MipClusterListOutputs.struct_size %u != %zu", out->struct_size, sizeof(MipClusterListOutputs));
  if (!out->cluster_entries || !out->entry_count) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "cluster_entries/entry_count is NULL");
  if ((uintptr_t)out->cluster_entries % 16u != 0u) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "cluster_entries is not 16-byte aligned");
  // the fields it shares with MipClusterOutputs, checked here so that a refusal names this call and this struct
  if (out->flags & ~(MIP_OUT_DEVICE | MIP_OUT_ASYNC)) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "unknown MipClusterListOutputs flags 0x%x", out->flags);
  if (!(out->flags & MIP_OUT_DEVICE)) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "mip_list_clusters needs MIP_OUT_DEVICE outputs");
  if ((uintptr_t)out->entry_count % 4u != 0u || (uintptr_t)out->draw_args % 4u != 0u || (uintptr_t)out->stats % 4u != 0u)
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "entry_count, draw_args or stats is not 4-byte aligned");
  MipClusterOutputs shared{};  // the fields the two structs share, for the checks and the launches they share
  shared.struct_size = sizeof(MipClusterOutputs);
  shared.flags = out->flags;
  shared.cluster_cmds = out->cluster_entries;
  shared.cmd_capacity = out->entry_capacity;
  shared.work_capacity = out->work_capacity;
  shared.cmd_count = out->entry_count;
  shared.stats = out->stats;
  return cull_clusters(ctx, frame, visible_bitmap, policy, occ, &shared, nullptr, false, nullptr, cone, cone != nullptr, out);
}

// Whether [p, p + bytes) and [q, q + qbytes) share a byte (q may be null: no).
static bool ranges_overlap(const void* p, unsigned long long bytes, const void* q, unsigned long long qbytes) {
  if (!q || !bytes || !qbytes) return false;
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b ? bytes > b - a : qbytes > a - b;
}

// mip_list_cluster_triangles: the checks of its own fields, then the call it shares with mip_list_clusters
int32_t mip_list_cluster_triangles(MipContext* ctx, const MipFrame* frame, const uint32_t* visible_bitmap, const MipLodPolicy* policy,
                                   const MipOcclusion* occ, const MipClusterCone* cone, const MipClusterTriangleListOutputs* out) {
  if (!ctx) return MIP_ERR_INVALID_ARGUMENT;
  if (int32_t rc = check_policy(ctx, policy)) return rc;
  if (!out) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "frame/visible_bitmap/out is NULL");
  if (out->struct_size != sizeof(MipClusterTriangleListOutputs))
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "MipClusterTriangleListOutputs.struct_size %u != %zu", out->struct_size, sizeof(MipClusterTriangleListOutputs));
  if (!out->cluster_entries || !out->entry_count) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "cluster_entries/entry_count is NULL");
  if ((uintptr_t)out->cluster_entries % 16u != 0u) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "cluster_entries is not 16-byte aligned");
  if (!out->triangle_masks || (uintptr_t)out->triangle_masks % 8u != 0u)
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "triangle_masks is NULL or not 8-byte aligned");
  if (out->flags & ~(MIP_OUT_DEVICE | MIP_OUT_ASYNC)) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "unknown MipClusterTriangleListOutputs flags 0x%x", out->flags);
  if (!(out->flags & MIP_OUT_DEVICE)) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "mip_list_cluster_triangles needs MIP_OUT_DEVICE outputs");
  if ((uintptr_t)out->entry_count % 4u != 0u || (uintptr_t)out->draw_args % 4u != 0u || (uintptr_t)out->stats % 4u != 0u)
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "entry_count, draw_args or stats is not 4-byte aligned");
  const unsigned long long mask_bytes = 8ull * out->entry_capacity;
  if (ranges_overlap(out->triangle_masks, mask_bytes, out->cluster_entries, 16ull * out->entry_capacity) ||
      ranges_overlap(out->triangle_masks, mask_bytes, out->entry_count, 4) || ranges_overlap(out->triangle_masks, mask_bytes, out->draw_args, 16) ||
      ranges_overlap(out->triangle_masks, mask_bytes, out->stats, 4ull * mip::kClusterTriangleListStats))
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "triangle_masks overlaps another output");
  MipClusterListOutputs list{};  // the fields it shares with mip_list_clusters, and under them those of mip_cull_clusters
  list.struct_size = sizeof(MipClusterListOutputs);
  list.flags = out->flags;
  list.cluster_entries = out->cluster_entries;
  list.entry_capacity = out->entry_capacity;
  list.work_capacity = out->work_capacity;
  list.entry_count = out->entry_count;
  list.draw_args = out->draw_args;
  list.stats = out->stats;
  MipClusterOutputs shared{};
  shared.struct_size = sizeof(MipClusterOutputs);
  shared.flags = out->flags;
  shared.cluster_cmds = out->cluster_entries;
  shared.cmd_capacity = out->entry_capacity;
  shared.work_capacity = out->work_capacity;
  shared.cmd_count = out->entry_count;
  shared.stats = out->stats;
  return cull_clusters(ctx, frame, visible_bitmap, policy, occ, &shared, nullptr, false, nullptr, cone, cone != nullptr, &list, out);
}

uint64_t mip_cluster_record_bytes(uint64_t work_items) { return mip::cluster_record_bytes(work_items); }

int32_t mip_cull_clusters_phase(MipContext* ctx, const MipFrame* frame, const uint32_t* visible_bitmap, const MipLodPolicy* policy,
                                const MipOcclusion* occ, const MipClusterOutputs* out, const MipClusterRecord* rec) {
  if (!ctx) return MIP_ERR_INVALID_ARGUMENT;
  if (int32_t rc = check_policy(ctx, policy)) return rc;
  return cull_clusters(ctx, frame, visible_bitmap, policy, occ, out, rec, true);
}

int32_t mip_list_clusters_phase(MipContext* ctx, const MipFrame* frame, const uint32_t* visible_bitmap, const MipLodPolicy* policy,
                                const MipOcclusion* occ, const MipClusterPhaseListOutputs* out, const MipClusterRecord* rec) {
  if (!ctx) return MIP_ERR_INVALID_ARGUMENT;
  if (int32_t rc = check_policy(ctx, policy)) return rc;
  return list_clusters_phase(ctx, frame, visible_bitmap, policy, occ, out, rec);
}

// mip_cull_cluster_triangles and its cone form: the checks of the trailing fields, then the call the two structs share
static int32_t cull_cluster_triangles(MipContext* ctx, const MipFrame* frame, const uint32_t* visible_bitmap, const MipLodPolicy* policy,
                               const MipOcclusion* occ, const MipClusterTriangleOutputs* out, const MipClusterCone* cone, bool coned) {
  if (int32_t rc = check_policy(ctx, policy)) return rc;
  if (!out) return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "frame/visible_bitmap/out is NULL");
  if (out->struct_size != sizeof(MipClusterTriangleOutputs))
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "MipClusterTriangleOutputs.struct_size %u != %zu", out->struct_size, sizeof(MipClusterTriangleOutputs));
  if (!out->culled_indices || (uintptr_t)out->culled_indices % 4u != 0u)
    return fail(ctx, MIP_ERR_INVALID_ARGUMENT, "culled_indices is NULL or not 4-byte aligned");
  MipClusterOutputs leading{};  // the fields the two structs share, for the checks and the launches they share
  leading.struct_size = sizeof(MipClusterOutputs);
  leading.flags = out->flags;
  leading.cluster_cmds = out->cluster_cmds;
  leading.cmd_capacity = out->cmd_capacity;
  leading.work_capacity = out->work_capacity;
  leading.cmd_count = out->cmd_count;
  leading.stats = out->stats;
  return cull_clusters(ctx, frame, visible_bitmap, policy, occ, &leading, nullptr, false, out, cone, coned);
}

int32_t mip_cull_cluster_triangles(MipContext* ctx, const MipFrame* frame, const uint32_t* visible_bitmap, const MipLodPolicy* policy,
                                   const MipOcclusion* occ, const MipClusterTriangleOutputs* out) {
  if (!ctx) return MIP_ERR_INVALID_ARGUMENT;
  return cull_cluster_triangles(ctx, frame, visible_bitmap, policy, occ, out, nullptr, false);
}

int32_t mip_cull_cluster_triangles_cone(MipContext* ctx, const MipFrame* frame, const uint32_t* visible_bitmap, const MipLodPolicy* policy,
                                        const MipOcclusion* occ, const MipClusterCone* cone, const MipClusterTriangleOutputs* out) {
  if (!ctx) return MIP_ERR_INVALID_ARGUMENT;
  return cull_cluster_triangles(ctx, frame, visible_bitmap, policy, occ, out, cone, true);
}

}  // extern "C"
