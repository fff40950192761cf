// cluster_kernel.hpp — cluster culling (mip_build_clusters, mip_cull_clusters, mip_cull_clusters_phase; extension, not reference behaviour), gfx950:
// the frustum test and the Hi-Z test of the instance level on every 64-triangle cluster of every member, and one draw
// command per run of surviving clusters. include/mi_instance_pipeline.h specifies it, tests/cluster_restatement.py restates
// it in numpy, cluster_plan.hpp holds the arithmetic that is not a kernel. Instantiated in api_cluster.hip only.
//
//   build      one wave per cluster: lane t folds the three corners of triangle 64 c + t (fminf / fmaxf from +inf / -inf: a NaN
//              is ignored, the result does not depend on the order), six butterfly reductions, lane 0 stores the box
//
// and per call, on one stream:
//
//   count      one tile of 1 024 instances per workgroup: the policy's pick (lod_chain_pick), items(i) = C(bucket) for a
//              member, else 0 -> items[i], bucket[i]; the tile's items (64-bit) and members -> tile_items / tile_members
//   scan       one workgroup: both rows become exclusive prefixes; W and `members`; decides whether the call runs (W < 2^32, W
//              within the bound) — if not, the kernels behind it see W = 0 and the epilogue writes the refusal
//   members    one tile per workgroup: the members packed in draw order — member_first[m] = the first work item of member m,
//              member_inst[m] = its instance; member_first[members] = W. Every member has at least one item, so member_first
//              is strictly increasing and 64 consecutive work items touch at most 64 consecutive members
//   cull       64 work items per wave and round: ONE uniform binary search (the member of the round's first item), the 64
//              entries behind it in the lanes, six shuffles per lane for its own member; the model matrix from the instance
//              columns and the world box of the CLUSTER's box by instance_tiered (the frame kernel's arithmetic, tiers
//              included); coarse_culled; box_occluded. The wave's ballot is the survive word; the ballot of c == 0 is stored
//              beside it (the start word), which spares the two later kernels a search per word
//   heads      one survive word per thread: heads = s & (start | ~(s << 1 | last bit of the word before)), read by the
//              thread itself; per-tile head and survivor counts
//   epilogue   one workgroup: the head counts become exclusive prefixes; cmd_count, stats, the overflow status
//   commands   one tile of 256 words per workgroup, a wave per 64 of them: the words with a head are located as in cull, a
//              head's rank = the tile's prefix + the words before + the lanes below; the run length by scanning the survive
//              words forward, bounded by the clusters the instance has left; guarded by cmd_capacity
//
// The two phases (mip_cull_clusters_phase) are the same seven launches with a compile-time phase:
//
//   FIRST      cull stores a third ballot, passed the planes && occluded, as the record word of its 64 items; heads counts
//              the record's bits beside the survivors; the epilogue writes the record's header
//   SECOND     scan compares the record's header with the call's W and members (a record of another call: W = 0 for the
//              kernels behind it, the device-error bit raised); retest takes cull's place: a wave reads its record word and
//              stores a zero survive word and a zero start word for a zero one — no search, no gather, no arithmetic —
//              and else locates its items, builds their boxes and runs box_occluded alone, the ballot under the record word
//
// The kernels mip_cull_clusters launches are the instantiations of phase 0, the code they had before the phases existed.
//
// No workgroup waits for another and nothing depends on the order workgroups start in. The kernels that walk work items run
// a grid sized for the host's bound on W (capped, cluster_plan.hpp) and loop over the tiles W — read from device memory —
// gives; the diagnostic build permutes the tiles of every kernel.
#pragma once

#include "batch_lods_kernel.hpp"
#include "cluster_plan.hpp"
#define MIP_OCCLUSION_DEVICE_HELPERS_ONLY  // box_occluded; the pyramid kernel stays in api_occlusion.hip
#include "occlusion_kernel.hpp"

#pragma clang fp contract(off)

namespace mip {

static_assert(kClusterThreads == kTile && kClusterInstanceTile == kBatchTile, "the count / members kernels tile as the batch kernels do");
static_assert(kClusterItemTile == kWaves * kBatchRounds * 64u && kClusterHeadTileWords == kTile, "tiles: cluster_plan.hpp and the kernels agree");

// scalars[]: what the scan leaves for the kernels behind it
constexpr uint32_t kClusterScW = 0;        // W, or 0 when the call does not run
constexpr uint32_t kClusterScMembers = 1;
constexpr uint32_t kClusterScWTrue = 2;    // W mod 2^32, whatever was decided
constexpr uint32_t kClusterScRuns = 3;     // 1 when the call runs
constexpr uint32_t kClusterScWords = 4;    // words the scan writes

// the phase a kernel is instantiated for, and the bits of a slot's status word (a code, read by the host)
constexpr uint32_t kClusterPlain = 0, kClusterFirst = 1, kClusterSecond = 2;
constexpr uint32_t kClusterStatusCapacity = 1u, kClusterStatusDevice = 2u;

struct ClusterBuildArgs {
  const float* vertices;
  const uint32_t* indices;
  const MeshChain* chain;
  const MeshDraw* mesh_draw;
  const uint32_t* bucket_lod;    // B words: mesh << 3 | lod
  const uint32_t* cluster_base;  // B + 1 words: the exclusive prefix sum of C, and the total
  float4* boxes;                 // two per cluster: {min xyz, -}, {max xyz, -}
  uint32_t n_buckets, total;
};

struct ClusterArgs {
  LodBatchArgs lods;             // the instance columns, the tables, the bitmap, the policy's thresholds, cam, the base: what lod_chain_pick reads
  const uint32_t* cluster_base;
  const float4* boxes;
  float planes[24];
  float pv[16];
  const float* pyramid;          // or null: the frustum test alone
  uint32_t width, height;
  unsigned long long bound;      // the host's bound on W
  // scratch
  uint32_t* items;               // n: C(bucket_i) of a member, else 0
  uint32_t* bucket;              // n
  uint32_t* member_first;        // n + 1
  uint32_t* member_inst;         // n
  unsigned long long* tile_items;  // instance tiles
  uint32_t* tile_members;
  uint32_t* scalars;             // kClusterScWords
  ulonglong2* words;             // per 64 work items: {survive, start}
  uint32_t* tile_heads;          // head tiles
  uint32_t* tile_survivors;
  // outputs
  uint32_t* cmds;
  uint32_t cmd_capacity;
  uint32_t* cmd_count;
  uint32_t* stats;               // or null
  uint32_t* status;              // the context's device-visible overflow word
  uint32_t debug_order;          // diagnostic build only: kClusterOrder* of the looping grids
  // a two-phase call (appended: the layout in front of them is mip_cull_clusters')
  uint32_t* record_header;       // the caller's record: {W, members, candidates, 0}, or null
  unsigned long long* record_words;  // one per 64 work items behind the header: written by FIRST, read by SECOND
  uint32_t* tile_candidates;     // scratch, head tiles (FIRST)
};

// ---- build ----
__device__ __forceinline__ float cluster_wave_min(float v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v = fminf(v, __shfl_xor(v, m));
  return v;
}
__device__ __forceinline__ float cluster_wave_max(float v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v = fmaxf(v, __shfl_xor(v, m));
  return v;
}

// The bucket a cluster of the table belongs to: the last b with cluster_base[b] <= g (g < total, so C(b) > 0).
__device__ __forceinline__ uint32_t cluster_bucket_of(const uint32_t* cluster_base, uint32_t n_buckets, uint32_t g) {
  uint32_t lo = 0, hi = n_buckets;
  while (hi - lo > 1u) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (cluster_base[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

static __global__ __launch_bounds__(kClusterThreads) __attribute__((unused)) void mip_cluster_build_kernel(const ClusterBuildArgs a) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t g = blockIdx.x * kWaves + wave;
  if (g >= a.total) return;  // (the whole wave)
  const uint32_t b = cluster_bucket_of(a.cluster_base, a.n_buckets, g);
  const uint32_t ml = a.bucket_lod[b];
  const uint32_t mesh = ml >> 3, lod = ml & 7u;
  const MeshChain& ch = a.chain[mesh];
  const uint32_t tris = cluster_level_triangles(ch.index_len[lod]);
  const uint32_t t = (g - a.cluster_base[b]) * kClusterTriangles + lane;
  const float inf = __builtin_inff();
  float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
  if (t < tris) {  // the host checked every index of the level and every vertex behind it (mip_build_clusters)
    const uint32_t* ix = a.indices + (size_t)ch.index_offset[lod] + 3u * (size_t)t;
    const size_t vo = (size_t)a.mesh_draw[mesh].vertex_offset;
#pragma unroll
    for (uint32_t k = 0; k < 3; ++k) {
      const float* v = a.vertices + 3u * (vo + ix[k]);
      const float p[3] = {v[0], v[1], v[2]};
      fold_corner(p, lo, hi);
    }
  }
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {
    lo[ax] = cluster_wave_min(lo[ax]);
    hi[ax] = cluster_wave_max(hi[ax]);
  }
  if (lane == 0u) {
    a.boxes[2u * (size_t)g] = make_float4(lo[0], lo[1], lo[2], 0.0f);
    a.boxes[2u * (size_t)g + 1u] = make_float4(hi[0], hi[1], hi[2], 0.0f);
  }
}

// ---- per call ----

__device__ __forceinline__ uint32_t cluster_loop_tile(const ClusterArgs& a, uint32_t t, uint32_t n_tiles) {
#ifdef MIP_DEBUG_STAMPS
  return cluster_permute_tile(t, n_tiles, a.debug_order);
#else
  return t;
#endif
}

// The slot's status word gains a bit. The calls of a slot are ordered by its stream and a call raises from one thread of one
// kernel at a time; the host clears the word only after the stream has drained: nobody else writes between the load and the store.
__device__ __forceinline__ void cluster_raise(const ClusterArgs& a, uint32_t code) {
  const uint32_t old = __hip_atomic_load(a.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(a.status, old | code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Exclusive scan of one 64-bit value per thread over the workgroup; `total` is the sum. s: kClusterThreads words.
__device__ __forceinline__ unsigned long long cluster_block_scan64(unsigned long long v, unsigned long long* s, unsigned long long& total) {
  const uint32_t tid = threadIdx.x;
  __syncthreads();  // s may still be read from the previous call
  s[tid] = v;
  __syncthreads();
  for (uint32_t off = 1; off < kClusterThreads; off <<= 1) {
    const unsigned long long add = tid >= off ? s[tid - off] : 0ull;
    __syncthreads();
    s[tid] += add;
    __syncthreads();
  }
  total = s[kClusterThreads - 1u];
  return s[tid] - v;
}

// count: items and bucket of every instance of the tile; the tile's sums
template <uint32_t kMode>
__global__ __launch_bounds__(kClusterThreads) void mip_cluster_count_kernel(const ClusterArgs a) {
  __shared__ unsigned long long s_items[kWaves];
  __shared__ uint32_t s_members[kWaves];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t tile = batch_tile(a.lods);
  const uint32_t n = a.lods.n;
  unsigned long long items = 0;
  uint32_t members = 0;
#pragma unroll
  for (uint32_t r = 0; r < kBatchRounds; ++r) {
    const uint32_t idx = batch_index(tile, wave, r, lane);
    const bool active = idx < n;
    const LodChainPick s = lod_chain_pick<kMode>(a.lods, active ? idx : n - 1u, active);
    // a level of one or two indices has no triangle: its instances are no members
    const uint32_t c = s.member ? a.cluster_base[s.bucket + 1u] - a.cluster_base[s.bucket] : 0u;
    if (active) {
      a.items[idx] = c;
      a.bucket[idx] = s.bucket;
    }
    items += (unsigned long long)wave_sum(c & 0xffffu) + ((unsigned long long)wave_sum(c >> 16) << 16);  // C < 2^31: neither half sum wraps
    members += (uint32_t)__popcll(__ballot(c != 0u));
  }
  if (lane == 0u) {
    s_items[wave] = items;
    s_members[wave] = members;
  }
  __syncthreads();
  if (threadIdx.x == 0u) {
    unsigned long long ti = 0;
    uint32_t tm = 0;
#pragma unroll
    for (uint32_t w = 0; w < kWaves; ++w) {
      ti += s_items[w];
      tm += s_members[w];
    }
    a.tile_items[tile] = ti;
    a.tile_members[tile] = tm;
  }
}

// scan: the tiles' sums become exclusive prefixes; W, members, and whether the call runs. One workgroup. SECOND: a record whose
// header names another W or another member count is not this call's — the kernels behind see W = 0, the epilogue zeros.
template <uint32_t kPhase>
__global__ __launch_bounds__(kClusterThreads) void mip_cluster_scan_kernel(const ClusterArgs a) {
  __shared__ unsigned long long s_scan[kClusterThreads];
  const uint32_t n_tiles = a.lods.n_tiles;
  unsigned long long items_before = 0, members_before = 0;
  for (uint32_t first = 0; first < n_tiles; first += kClusterThreads) {
    const uint32_t t = first + threadIdx.x;
    const unsigned long long vi = t < n_tiles ? a.tile_items[t] : 0ull, vm = t < n_tiles ? a.tile_members[t] : 0ull;
    unsigned long long ti, tm;
    const unsigned long long ei = cluster_block_scan64(vi, s_scan, ti);
    const unsigned long long em = cluster_block_scan64(vm, s_scan, tm);
    if (t < n_tiles) {
      a.tile_items[t] = items_before + ei;
      a.tile_members[t] = (uint32_t)(members_before + em);
    }
    items_before += ti;
    members_before += tm;
  }
  if (threadIdx.x == 0u) {
    const bool fits = cluster_work_fits(items_before, a.bound);
    bool runs = fits;
    if constexpr (kPhase == kClusterSecond)
      runs = fits && a.record_header[0] == (uint32_t)items_before && a.record_header[1] == (uint32_t)members_before;
    a.scalars[kClusterScW] = runs ? (uint32_t)items_before : 0u;
    a.scalars[kClusterScRuns] = runs ? 1u : 0u;
    a.scalars[kClusterScMembers] = (uint32_t)members_before;
    a.scalars[kClusterScWTrue] = (uint32_t)items_before;
    a.member_first[(uint32_t)members_before] = (uint32_t)items_before;  // members <= n: the list's end
    if (!fits) cluster_raise(a, kClusterStatusCapacity);
    else if (!runs) cluster_raise(a, kClusterStatusDevice);
  }
}

// members: the tile's members to their slots of the packed list
static __global__ __launch_bounds__(kClusterThreads) __attribute__((unused)) void mip_cluster_members_kernel(const ClusterArgs a) {
  __shared__ uint32_t s_items[kWaves], s_members[kWaves];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t tile = batch_tile(a.lods);
  const uint32_t n = a.lods.n;
  uint32_t first[kBatchRounds], rank[kBatchRounds];
  bool member[kBatchRounds];
  uint32_t w_items = 0, w_members = 0;
#pragma unroll
  for (uint32_t r = 0; r < kBatchRounds; ++r) {
    const uint32_t idx = batch_index(tile, wave, r, lane);
    const uint32_t c = idx < n ? a.items[idx] : 0u;
    member[r] = c != 0u;
    const unsigned long long mask = __ballot(member[r]);
    rank[r] = w_members + lanes_below(mask);
    w_members += (uint32_t)__popcll(mask);
    const uint32_t incl = wave_inclusive_scan(c);  // (wraps only in a call that does not run: nobody reads the list then)
    first[r] = w_items + incl - c;
    w_items += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
  }
  if (lane == 0u) {
    s_items[wave] = w_items;
    s_members[wave] = w_members;
  }
  __syncthreads();
  uint32_t items_before = (uint32_t)a.tile_items[tile], members_before = a.tile_members[tile];
#pragma unroll
  for (uint32_t w = 0; w < kWaves; ++w) {
    items_before += w < wave ? s_items[w] : 0u;
    members_before += w < wave ? s_members[w] : 0u;
  }
#pragma unroll
  for (uint32_t r = 0; r < kBatchRounds; ++r) {
    if (member[r]) {
      const uint32_t m = members_before + rank[r];  // < members <= n
      a.member_first[m] = items_before + first[r];
      a.member_inst[m] = batch_index(tile, wave, r, lane);
    }
  }
}

// Where a work item lives: its member's instance, and its cluster inside the instance's level.
struct ClusterItem {
  uint32_t inst, cluster;
};

// The 64 work items [base, base + 64) of a wave, base a multiple of 64 below W: one uniform binary search for the member of
// `base`, then every lane finds its own among the 64 entries behind it (held one per lane) with six shuffles. A lane whose
// item is at or above W locates `base` instead: its loads stay in bounds and its result is not used. Called by whole waves.
__device__ __forceinline__ ClusterItem cluster_locate(const ClusterArgs& a, uint32_t base, uint32_t lane, uint32_t w_total, uint32_t members) {
  uint32_t lo = 0, hi = members;  // W > 0, so members >= 1 and member_first[0] = 0 <= base
  while (hi - lo > 1u) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    const uint32_t f = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.member_first[mid]);
    if (f <= base) lo = mid; else hi = mid;
  }
  const uint32_t m0 = lo;
  const uint32_t mine = m0 + lane < members ? a.member_first[m0 + lane] : 0xffffffffu;  // strictly increasing; W < 2^32 - 1 <= the filler
  const uint32_t w = base + lane < w_total ? base + lane : base;  // (base <= 2^32 - 64: the sum does not wrap)
  uint32_t j = 0;
#pragma unroll
  for (uint32_t step = 32; step > 0; step >>= 1) {
    const uint32_t at = (uint32_t)__shfl((int)mine, (int)(j + step));  // j + step <= 63
    if (at <= w) j += step;
  }
  const uint32_t first = (uint32_t)__shfl((int)mine, (int)j);
  return {a.member_inst[m0 + j], w - first};
}

// The world box of work item `it`: the model matrix from the instance columns, the CLUSTER's box in the mesh box's place.
// For the retest kernel; cull holds the same lines itself, because calling this from it changed the schedule of the kernel
// mip_cull_clusters launches, which is held to the instructions it had before the phases existed.
__device__ __forceinline__ void cluster_world_box(const ClusterArgs& a, const ClusterItem& it, Instance& inst) {
  const uint32_t i = it.inst;
  const float px = a.lods.pos[3 * (size_t)i + 0], py = a.lods.pos[3 * (size_t)i + 1], pz = a.lods.pos[3 * (size_t)i + 2];
  const float4 q = a.lods.rot[i];
  const float sc = a.lods.scale[i];
  const size_t g = (size_t)a.cluster_base[a.bucket[i]] + it.cluster;
  const float4 b0 = a.boxes[2u * g], b1 = a.boxes[2u * g + 1u];
  MeshEntry mb;  // the cluster's box in the mesh box's place
  mb.min_x = b0.x; mb.min_y = b0.y; mb.min_z = b0.z; mb.len0 = 0u;
  mb.max_x = b1.x; mb.max_y = b1.y; mb.max_z = b1.z; mb.len1 = 0u;
  float rm[3][3];
  quat_to_rotation(q.x, q.y, q.z, q.w, rm);
  struct { const float* box_override; } no_box = {nullptr};
  // always the kernel with the fall-back tiers: a cluster's box may hold anything the vertices hold
  instance_tiered<false, true>(no_box, i, rm, px, py, pz, sc, mb, inst);
}

// cull: both tests on every work item; the survive word and the start word of every 64. kRecord (FIRST): and the record word,
// the items that passed the planes and are occluded.
template <bool kRecord>
__global__ __launch_bounds__(kClusterThreads, 4) void mip_cluster_cull_kernel(const ClusterArgs a) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t w_total = a.scalars[kClusterScW], members = a.scalars[kClusterScMembers];
  const uint32_t n_tiles = cluster_item_tiles(w_total);
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint32_t tile = cluster_loop_tile(a, t, n_tiles);
#pragma unroll 1
    for (uint32_t r = 0; r < kBatchRounds; ++r) {
      const unsigned long long base64 = (unsigned long long)tile * kClusterItemTile + wave * (kBatchRounds * 64u) + r * 64u;
      if (base64 >= w_total) break;  // (the whole wave; the rounds behind it start later still)
      const uint32_t base = (uint32_t)base64;
      const ClusterItem it = cluster_locate(a, base, lane, w_total, members);
      const bool active = base + lane < w_total;
      const uint32_t i = it.inst;
      const float px = a.lods.pos[3 * (size_t)i + 0], py = a.lods.pos[3 * (size_t)i + 1], pz = a.lods.pos[3 * (size_t)i + 2];
      const float4 q = a.lods.rot[i];
      const float sc = a.lods.scale[i];
      const size_t g = (size_t)a.cluster_base[a.bucket[i]] + it.cluster;
      const float4 b0 = a.boxes[2u * g], b1 = a.boxes[2u * g + 1u];
      MeshEntry mb;  // the cluster's box in the mesh box's place
      mb.min_x = b0.x; mb.min_y = b0.y; mb.min_z = b0.z; mb.len0 = 0u;
      mb.max_x = b1.x; mb.max_y = b1.y; mb.max_z = b1.z; mb.len1 = 0u;
      float rm[3][3];
      quat_to_rotation(q.x, q.y, q.z, q.w, rm);
      Instance inst;
      struct { const float* box_override; } no_box = {nullptr};
      // always the kernel with the fall-back tiers: a cluster's box may hold anything the vertices hold
      instance_tiered<false, true>(no_box, i, rm, px, py, pz, sc, mb, inst);
      bool survives = active && !coarse_culled(inst, a.planes);
      [[maybe_unused]] const bool passed = survives;
      if (survives && a.pyramid) survives = !box_occluded(inst.mins, inst.maxs, a.pv, a.pyramid, a.width, a.height);
      const unsigned long long s = __ballot(survives), start = __ballot(active && it.cluster == 0u);
      if (lane == 0u) a.words[base >> 6] = make_ulonglong2(s, start);
      if constexpr (kRecord) {
        const unsigned long long candidates = __ballot(passed && !survives);  // (an item at or above W is not active: its bit is 0)
        if (lane == 0u) a.record_words[base >> 6] = candidates;
      }
    }
  }
}

// retest (SECOND, in cull's place): the Hi-Z test alone, on the items the record names. A wave reads its record word first: a
// zero word is answered with a zero survive word and a zero start word — a head can only be in a non-zero word, and nothing
// else reads a start word.
static __global__ __launch_bounds__(kClusterThreads, 4) __attribute__((unused)) void mip_cluster_retest_kernel(const ClusterArgs a) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t w_total = a.scalars[kClusterScW], members = a.scalars[kClusterScMembers];
  const uint32_t n_tiles = cluster_item_tiles(w_total);
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint32_t tile = cluster_loop_tile(a, t, n_tiles);
#pragma unroll 1
    for (uint32_t r = 0; r < kBatchRounds; ++r) {
      const unsigned long long base64 = (unsigned long long)tile * kClusterItemTile + wave * (kBatchRounds * 64u) + r * 64u;
      if (base64 >= w_total) break;  // (the whole wave; the rounds behind it start later still)
      const uint32_t base = (uint32_t)base64;
      const unsigned long long loaded = a.record_words[base >> 6];  // word < ceil(W / 64): the scan matched W, the host the room
      const unsigned long long candidates = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(loaded >> 32)) << 32) |
                                            (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)loaded);
      if (candidates == 0ull) {  // (the whole wave)
        if (lane == 0u) a.words[base >> 6] = make_ulonglong2(0ull, 0ull);
        continue;
      }
      const ClusterItem it = cluster_locate(a, base, lane, w_total, members);
      const bool active = base + lane < w_total && ((candidates >> lane) & 1ull) != 0ull;
      Instance inst;
      cluster_world_box(a, it, inst);
      const bool survives = active && !box_occluded(inst.mins, inst.maxs, a.pv, a.pyramid, a.width, a.height);
      const unsigned long long s = __ballot(survives), start = __ballot(base + lane < w_total && it.cluster == 0u);
      if (lane == 0u) a.words[base >> 6] = make_ulonglong2(s, start);
    }
  }
}

// The heads among the 64 work items of a word: survivors that start an instance or follow a cluster that does not survive.
__device__ __forceinline__ unsigned long long cluster_head_mask(const ClusterArgs& a, uint32_t word) {
  const ulonglong2 w = a.words[word];
  const unsigned long long before = word ? a.words[word - 1u].x >> 63 : 0ull;  // read by this thread itself
  return w.x & (w.y | ~((w.x << 1) | before));
}

// heads: the head and survivor counts of every tile of 256 words; kRecord (FIRST): and the candidates of the record's words
template <bool kRecord>
__global__ __launch_bounds__(kClusterThreads) void mip_cluster_heads_kernel(const ClusterArgs a) {
  __shared__ uint32_t s_heads[kWaves], s_survivors[kWaves];
  __shared__ uint32_t s_candidates[kRecord ? kWaves : 1u];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t w_total = a.scalars[kClusterScW];
  const uint32_t n_words = cluster_survive_words(w_total), n_tiles = cluster_head_tiles(w_total);
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint32_t tile = cluster_loop_tile(a, t, n_tiles);
    const uint32_t word = tile * kClusterHeadTileWords + threadIdx.x;
    const bool valid = word < n_words;
    const uint32_t heads = wave_sum(valid ? (uint32_t)__popcll(cluster_head_mask(a, word)) : 0u);
    const uint32_t survivors = wave_sum(valid ? (uint32_t)__popcll(a.words[word].x) : 0u);
    if (lane == 0u) {
      s_heads[wave] = heads;
      s_survivors[wave] = survivors;
    }
    if constexpr (kRecord) {
      const uint32_t candidates = wave_sum(valid ? (uint32_t)__popcll(a.record_words[word]) : 0u);
      if (lane == 0u) s_candidates[wave] = candidates;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
      uint32_t th = 0, ts = 0;
#pragma unroll
      for (uint32_t w = 0; w < kWaves; ++w) {
        th += s_heads[w];
        ts += s_survivors[w];
      }
      a.tile_heads[tile] = th;
      a.tile_survivors[tile] = ts;
      if constexpr (kRecord) {
        uint32_t tc = 0;
#pragma unroll
        for (uint32_t w = 0; w < kWaves; ++w) tc += s_candidates[w];
        a.tile_candidates[tile] = tc;
      }
    }
    __syncthreads();  // the sums are free for the next tile
  }
}

// epilogue: the head counts become exclusive prefixes; the count, the stats and the status of the call. One workgroup.
// kRecord (FIRST): and the record's header — {W, members, candidates, 0}, or that of a call that did not run.
template <bool kRecord>
__global__ __launch_bounds__(kClusterThreads) void mip_cluster_epilogue_kernel(const ClusterArgs a) {
  __shared__ uint32_t s_wave[kWaves];
  const uint32_t n_tiles = cluster_head_tiles(a.scalars[kClusterScW]);  // 0 when the call does not run
  uint32_t heads_before = 0, survivors = 0;
  uint32_t candidates = 0;
  for (uint32_t first = 0; first < n_tiles; first += kClusterThreads) {
    const uint32_t t = first + threadIdx.x;
    uint32_t th, ts;
    if constexpr (kRecord) {
      uint32_t tc;
      (void)batch_block_scan(t < n_tiles ? a.tile_candidates[t] : 0u, s_wave, tc);
      candidates += tc;
    }
    const uint32_t excl = batch_block_scan(t < n_tiles ? a.tile_heads[t] : 0u, s_wave, th);
    (void)batch_block_scan(t < n_tiles ? a.tile_survivors[t] : 0u, s_wave, ts);
    if (t < n_tiles) a.tile_heads[t] = heads_before + excl;
    heads_before += th;
    survivors += ts;
  }
  if (threadIdx.x == 0u) {
    *a.cmd_count = heads_before < a.cmd_capacity ? heads_before : a.cmd_capacity;
    if (a.stats) {
      a.stats[0] = heads_before;
      a.stats[1] = survivors;
      a.stats[2] = a.scalars[kClusterScWTrue];
      a.stats[3] = a.scalars[kClusterScMembers];
    }
    if (heads_before > a.cmd_capacity) cluster_raise(a, kClusterStatusCapacity);
    if constexpr (kRecord) {
      const bool runs = a.scalars[kClusterScRuns] != 0u;
      a.record_header[0] = runs ? a.scalars[kClusterScW] : kClusterRecordRefused;
      a.record_header[1] = runs ? a.scalars[kClusterScMembers] : 0u;
      a.record_header[2] = runs ? candidates : 0u;
      a.record_header[3] = 0u;
    }
  }
}

// commands: one per head, in work-item order
static __global__ __launch_bounds__(kClusterThreads) __attribute__((unused)) void mip_cluster_commands_kernel(const ClusterArgs a) {
  __shared__ uint32_t s_wave[kWaves];
  __shared__ uint32_t s_rank[kClusterHeadTileWords];
  __shared__ unsigned long long s_mask[kClusterHeadTileWords];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t w_total = a.scalars[kClusterScW], members = a.scalars[kClusterScMembers];
  const uint32_t n_words = cluster_survive_words(w_total), n_tiles = cluster_head_tiles(w_total);
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint32_t tile = cluster_loop_tile(a, t, n_tiles);
    {
      const uint32_t word = tile * kClusterHeadTileWords + threadIdx.x;
      const unsigned long long mask = word < n_words ? cluster_head_mask(a, word) : 0ull;
      uint32_t unused_total;
      const uint32_t excl = batch_block_scan((uint32_t)__popcll(mask), s_wave, unused_total);
      s_rank[threadIdx.x] = a.tile_heads[tile] + excl;  // the heads in front of this word (epilogue: the tiles before)
      s_mask[threadIdx.x] = mask;
    }
    __syncthreads();
#pragma unroll 1
    for (uint32_t j = 0; j < 64u; ++j) {
      const uint32_t local = wave * 64u + j;
      const unsigned long long stored = s_mask[local];
      const unsigned long long mask = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(stored >> 32)) << 32) |
                                      (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)stored);
      if (mask == 0ull) continue;  // (the whole wave)
      const uint32_t base = (tile * kClusterHeadTileWords + local) * 64u;  // < W: the word holds a survivor
      const ClusterItem it = cluster_locate(a, base, lane, w_total, members);
      const uint32_t rank = s_rank[local] + lanes_below(mask);
      if (((mask >> lane) & 1ull) != 0ull && rank < a.cmd_capacity) {
        const uint32_t ml = a.lods.bucket_lod[a.bucket[it.inst]];
        const uint32_t mesh = ml >> 3, lod = ml & 7u;
        const MeshChain& ch = a.lods.chain[mesh];
        const uint32_t tris = cluster_level_triangles(ch.index_len[lod]);
        const uint32_t limit = cluster_level_clusters(ch.index_len[lod]) - it.cluster;  // clusters the instance has left, this one included
        // the run: this survivor and the survivors straight behind it, inside the instance
        uint32_t run = 0, at = base + lane;
        while (run < limit) {
          const uint32_t bit = at & 63u, room = 64u - bit;
          const unsigned long long rest = ~(a.words[at >> 6].x >> bit);  // the shift brings zeros in: a clear bit below `room`, unless bit == 0
          const uint32_t ones = rest ? (uint32_t)__builtin_ctzll(rest) : 64u;
          const uint32_t take = ones < limit - run ? ones : limit - run;
          run += take;
          at += take;
          if (ones < room) break;  // a cluster that does not survive ends the run
        }
        uint32_t* o = a.cmds + (size_t)rank * kCmdWords;
        o[0] = cluster_run_index_count(it.cluster, run, tris);
        o[1] = 1u;
        o[2] = ch.index_offset[lod] + kClusterIndices * it.cluster;  // the source mesh's own range
        o[3] = (uint32_t)a.lods.mesh_draw[mesh].vertex_offset;
        o[4] = a.lods.first_instance_base + it.inst;
      }
    }
    __syncthreads();  // s_rank / s_mask are free for the next tile
  }
}

}  // namespace mip
