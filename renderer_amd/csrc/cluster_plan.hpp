// cluster_plan.hpp — the arithmetic of cluster culling (mip_build_clusters, mip_cull_clusters, mip_cull_clusters_phase;
// extension, not reference behaviour) that is not a kernel: how a level is cut into clusters, the bound on a call's work items,
// the grids and the scratch a call takes, the tiles a looping grid walks, the permutation the diagnostic build puts on them,
// the index count of a run, the size of a two-phase call's record and the work items a record has room for. Plain C++, no HIP: api_cluster.hip and cluster_kernel.hpp call it, tests/native/cluster_plan_check.cpp enumerates it
// on the CPU over its decision edges.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define MIP_CLUSTER_HD __host__ __device__
#else
#define MIP_CLUSTER_HD
#endif

namespace mip {

constexpr uint32_t kClusterTriangles = 64;                    // MIP_CLUSTER_TRIANGLES: one triangle per lane of the build's wave
constexpr uint32_t kClusterIndices = 3 * kClusterTriangles;   // a cluster's stride in its level's index range
constexpr uint32_t kClusterThreads = 256;                     // every kernel's workgroup: four waves
constexpr uint32_t kClusterInstanceTile = 1024;               // instances per workgroup of the count / members kernels (kBatchTile)
constexpr uint32_t kClusterItemTile = 1024;                   // work items per tile of the cull kernel: a wave takes 4 rounds of 64
constexpr uint32_t kClusterHeadTileWords = 256;               // survive words per tile of the heads / commands kernels: one per thread
constexpr uint32_t kClusterHeadTile = 64 * kClusterHeadTileWords;  // = 16 384 work items
constexpr uint32_t kClusterMaxBlocks = 2048;                  // the looping grids (cull, heads, commands) never launch more
constexpr unsigned long long kClusterMaxTotal = 1ull << 31;   // clusters a table may hold
constexpr unsigned long long kClusterMaxWork = (1ull << 32) - 1ull;  // W of a call that runs: W < 2^32

// T(b) and C(b) of a level of `index_len` indices: a tail of one or two indices belongs to no triangle.
MIP_CLUSTER_HD constexpr uint32_t cluster_level_triangles(uint32_t index_len) { return index_len / 3u; }
MIP_CLUSTER_HD constexpr uint32_t cluster_level_clusters(uint32_t index_len) {
  return (cluster_level_triangles(index_len) + kClusterTriangles - 1u) / kClusterTriangles;
}
// triangles of cluster c of a level of T triangles (c < C): 64, or what is left in the last one
MIP_CLUSTER_HD constexpr uint32_t cluster_triangles(uint32_t c, uint32_t t) {
  return t - c * kClusterTriangles < kClusterTriangles ? t - c * kClusterTriangles : kClusterTriangles;
}
// indexCount of a run of `run` clusters that starts at cluster c of a level of T triangles (c + run <= C)
MIP_CLUSTER_HD constexpr uint32_t cluster_run_index_count(uint32_t c, uint32_t run, uint32_t t) {
  const unsigned long long end = (unsigned long long)(c + run) * kClusterTriangles;
  return 3u * ((end < t ? (uint32_t)end : t) - c * kClusterTriangles);
}

// The bound a call's work items are held to: the caller's, or N x the largest C of the table; never above 2^32 - 1.
constexpr unsigned long long cluster_work_bound(uint32_t n, uint32_t max_clusters, uint32_t work_capacity) {
  const unsigned long long own = (unsigned long long)n * max_clusters;
  const unsigned long long bound = work_capacity ? work_capacity : own;
  return bound < kClusterMaxWork ? bound : kClusterMaxWork;
}
// Whether a call with W work items runs (else MIP_ERR_CAPACITY, no command written): W < 2^32 and within the bound.
MIP_CLUSTER_HD constexpr bool cluster_work_fits(unsigned long long w, unsigned long long bound) { return w <= kClusterMaxWork && w <= bound; }

// The record of a two-phase call (mip_cull_clusters_phase): a 16-byte header, then one 64-bit word per 64 work items.
constexpr unsigned long long kClusterRecordHeaderBytes = 16;
constexpr uint32_t kClusterRecordRefused = 0xFFFFFFFFu;       // the header's W of a FIRST call that did not run: no running call has it
constexpr unsigned long long cluster_record_bytes(unsigned long long work_items) {
  return kClusterRecordHeaderBytes + 8ull * (work_items / 64ull + (work_items % 64ull ? 1ull : 0ull));
}
// The most work items a record of `record_bytes` (>= 16) has words for: the bound a phase call's W is held to besides its own.
constexpr unsigned long long cluster_record_items(unsigned long long record_bytes) {
  const unsigned long long words = (record_bytes - kClusterRecordHeaderBytes) / 8ull;
  return words >= (kClusterMaxWork + 63ull) / 64ull ? kClusterMaxWork : words * 64ull;
}

MIP_CLUSTER_HD constexpr uint32_t cluster_item_tiles(uint32_t w) { return w / kClusterItemTile + (w % kClusterItemTile ? 1u : 0u); }
MIP_CLUSTER_HD constexpr uint32_t cluster_survive_words(uint32_t w) { return w / 64u + (w % 64u ? 1u : 0u); }
MIP_CLUSTER_HD constexpr uint32_t cluster_head_tiles(uint32_t w) { return w / kClusterHeadTile + (w % kClusterHeadTile ? 1u : 0u); }

// What a call launches and allocates: a pure function of N and the bound on W. The grids of the kernels that walk work items
// are sized for the bound, capped at kClusterMaxBlocks, and loop: tile = block, block + grid, ... below the tile count they
// read from device memory.
struct ClusterPlan {
  uint32_t instance_tiles;   // workgroups of the count and members kernels
  uint32_t cull_blocks;      // the cull kernel's grid
  uint32_t retest_blocks;    // the retest kernel's grid (SECOND): it walks the same item tiles
  uint32_t head_blocks;      // the heads and commands kernels' grid
  unsigned long long survive_words;  // 16 bytes each: the survive word and the start word of 64 work items
  uint32_t head_tiles;       // rows of the head counts
  constexpr bool cull_loops() const { return cull_blocks == kClusterMaxBlocks; }
};
constexpr ClusterPlan plan_cluster_cull(uint32_t n, unsigned long long bound) {
  ClusterPlan p{};
  p.instance_tiles = n / kClusterInstanceTile + (n % kClusterInstanceTile ? 1u : 0u);
  if (p.instance_tiles == 0u) p.instance_tiles = 1u;
  const unsigned long long item_tiles = (bound + kClusterItemTile - 1u) / kClusterItemTile;
  const unsigned long long head_tiles = (bound + kClusterHeadTile - 1u) / kClusterHeadTile;
  p.cull_blocks = item_tiles < 1u ? 1u : item_tiles < kClusterMaxBlocks ? (uint32_t)item_tiles : kClusterMaxBlocks;
  p.retest_blocks = p.cull_blocks;
  p.head_blocks = head_tiles < 1u ? 1u : head_tiles < kClusterMaxBlocks ? (uint32_t)head_tiles : kClusterMaxBlocks;
  p.survive_words = (bound + 63u) / 64u;
  p.head_tiles = head_tiles < 1u ? 1u : (uint32_t)head_tiles;
  return p;
}

// The diagnostic build's permutation of the tiles a looping grid walks (never the product): 0 = none, 1 = reversed,
// 2 = scrambled by a prime that does not divide the tile count. A bijection of [0, n_tiles) for every n_tiles >= 1.
constexpr uint32_t kClusterOrderNone = 0, kClusterOrderReverse = 1, kClusterOrderScramble = 2;
MIP_CLUSTER_HD constexpr uint32_t cluster_permute_tile(uint32_t t, uint32_t n_tiles, uint32_t order) {
  if (order == kClusterOrderReverse) return n_tiles - 1u - t;
  if (order == kClusterOrderScramble && n_tiles > 1u) {
    const uint32_t primes[4] = {7919u, 104729u, 1299709u, 15485863u};
    uint32_t mult = 1u;
    for (uint32_t k = 0; k < 4u; ++k)
      if (n_tiles % primes[k] != 0u) { mult = primes[k]; break; }
    return (uint32_t)(((unsigned long long)t * mult + 12345u % n_tiles) % n_tiles);
  }
  return t;
}

}  // namespace mip
