// batch_lods_kernel.hpp — batched draws over the whole LOD chain (mip_batch_draws_lods; extension, not reference behaviour).
//
// The stage is batch_kernel.hpp's — count / rowscan / scatter per 8-bit digit, the list passes above 256 buckets, the
// 1 024-instance tile in rounds of 64 consecutive instances, no workgroup waiting for another — with another key policy:
//
//   lod    = #{ k in [0, n_lods - 1) : q > b_k }           q = |cam - pos|^2 as lod_is_far forms it
//   b_k    = switch_sq[k]                                   MIP_LOD_DISTANCE
//          = switch_sq[k] * ((scale * scale) * diag_sq)     MIP_LOD_RELATIVE, diag_sq = |aabb_max - aabb_min|^2 of the mesh
//   bucket = lod_base[mesh] + lod                           lod_base = exclusive prefix sum of n_lods: B = sum n_lods buckets
//
// in float32, contraction off, every product and sum rounded once (include/mi_instance_pipeline.h states the rule;
// tests/lod_restatement.py restates it in numpy). The per-mesh chain (MeshChain, 64 B, filled by mip_set_mesh_table) is
// gathered as 16-byte pieces: the key takes two (n_lods, lod_base, the six lengths), the command writer all four.
// The DISTANCE key reads neither `scale` nor the mesh box. The mode is a template parameter: no kernel branches on it.
// The list passes and the rowscan do not form keys: mip_batch_draws_lods launches batch_kernel.hpp's own instantiations.
// Instantiated in api_batch.hip only.
#pragma once

#include "batch_kernel.hpp"
#include "mesh_chain.hpp"

#pragma clang fp contract(off)

namespace mip {

constexpr uint32_t kMaxLods = MIP_MAX_LODS;
constexpr uint32_t kLodModeDistance = MIP_LOD_DISTANCE, kLodModeRelative = MIP_LOD_RELATIVE;

static_assert(sizeof(MeshChain::index_len) == kMaxLods * 4, "MeshChain (mesh_chain.hpp) holds MIP_MAX_LODS levels");

struct LodBatchArgs : BatchArgs {
  const MeshChain* chain;        // m
  const uint32_t* bucket_lod;    // B words: mesh << 3 | lod of every bucket (the command writer)
  float switch_sq[kMaxLods - 1];
};

// The bucket of instance il under the policy, or kBatchNone when it is not a member.
template <uint32_t kMode>
struct BatchLodChainKey {
  using Args = LodBatchArgs;
  static __device__ __forceinline__ uint32_t key(const Args& a, uint32_t il, bool active) {
    const uint32_t word = a.bitmap[il >> 5];
    const float px = a.pos[3 * (size_t)il + 0], py = a.pos[3 * (size_t)il + 1], pz = a.pos[3 * (size_t)il + 2];
    const uint32_t mesh = a.mesh_id[il];
    const uint4* piece = reinterpret_cast<const uint4*>(a.chain + mesh);
    const uint4 c0 = piece[0], c1 = piece[1];
    const uint32_t n_lods = c0.x;
    const float dx = a.cam[0] - px, dy = a.cam[1] - py, dz = a.cam[2] - pz;
    const float q = dx * dx + dy * dy + dz * dz;  // (dx*dx + dy*dy) + dz*dz: lod_is_far's expression
    float unit = 1.0f;
    if constexpr (kMode == kLodModeRelative) {
      const MeshEntry mb = load_mesh_entry(a.meshes, mesh);
      const float ex = mb.max_x - mb.min_x, ey = mb.max_y - mb.min_y, ez = mb.max_z - mb.min_z;
      const float diag_sq = ex * ex + ey * ey + ez * ez;
      const float sc = a.scale[il];
      unit = (sc * sc) * diag_sq;
    }
    uint32_t lod = 0;
#pragma unroll
    for (uint32_t k = 0; k + 1u < kMaxLods; ++k) {
      const float b = kMode == kLodModeRelative ? a.switch_sq[k] * unit : a.switch_sq[k];
      lod += (k + 1u < n_lods && q > b) ? 1u : 0u;  // a count; a NaN on either side compares false
    }
    uint32_t len = c0.z;
    len = lod == 1u ? c0.w : len;
    len = lod == 2u ? c1.x : len;
    len = lod == 3u ? c1.y : len;
    len = lod == 4u ? c1.z : len;
    len = lod == 5u ? c1.w : len;
    const bool member = active && ((word >> (il & 31u)) & 1u) != 0u && len > 0u;
    return member ? c0.y + lod : kBatchNone;
  }
};

// ---- count / scatter / model: batch_kernel.hpp's pass 0 (keys from the instance columns), templated on the key policy ----
// The same statements as mip_batch_count_kernel<false>, mip_batch_scatter_kernel<false, kLast, kModel> and
// mip_batch_model_kernel, with Key::key where those call batch_key. They are written out here and not shared with those
// kernels through a common body: routing the existing instantiations through one moved their register allocation, and their
// gfx950 text is pinned. The pin policy keeps the two in step: tests/test_gpu_batch_lods.py compares every output
// buffer of the two entry points byte for byte. batch_tile, batch_index, batch_block_scan and batch_store_models are shared.
template <class Key>
__device__ __forceinline__ uint32_t batch_lods_load_key(const typename Key::Args& a, uint32_t idx) {
  const bool active = idx < a.n;
  return Key::key(a, active ? idx : a.n - 1u, active);
}

template <class Key>
__global__ __launch_bounds__(kTile) void mip_batch_lods_count_kernel(const typename Key::Args a) {
  __shared__ uint32_t s_hist[kBatchBins];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t tile = batch_tile(a);
  s_hist[tid] = 0u;
  __syncthreads();
#pragma unroll
  for (uint32_t r = 0; r < kBatchRounds; ++r) {
    const uint32_t key = batch_lods_load_key<Key>(a, batch_index(tile, wave, r, lane));
    if (key != kBatchNone) {
      atomicAdd(&s_hist[(key >> a.shift) & (kBatchBins - 1u)], 1u);
      if (a.bucket_hist) atomicAdd(&a.bucket_hist[key], 1u);
    }
  }
  __syncthreads();
  if (tid < a.n_bins) a.counts[(size_t)tid * a.n_tiles + tile] = s_hist[tid];
}

// kModel: 0 = no matrices, 1 = census-selected arithmetic, 2 = the tiers of kGeneral (as mip_batch_scatter_kernel)
template <class Key, bool kLast, int kModel>
__global__ __launch_bounds__(kTile) void mip_batch_lods_scatter_kernel(const typename Key::Args a) {
  static_assert(!kModel || kLast, "matrices go out with the one pass that reads the instances in draw order");
  __shared__ uint32_t s_hist[kWaves][kBatchBins];
  __shared__ uint32_t s_wave[kWaves];
  __shared__ __attribute__((aligned(16))) std::conditional_t<kModel != 0, BatchModelStage, uint32_t> s_stage;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t tile = batch_tile(a);
#pragma unroll
  for (uint32_t w = 0; w < kWaves; ++w) s_hist[w][tid] = 0u;
  __syncthreads();

  // rank inside (tile, bin): see mip_batch_scatter_kernel
  uint32_t key[kBatchRounds], rank[kBatchRounds];
#pragma unroll
  for (uint32_t r = 0; r < kBatchRounds; ++r) {
    key[r] = batch_lods_load_key<Key>(a, batch_index(tile, wave, r, lane));
    const bool valid = key[r] != kBatchNone;
    const uint32_t digit = valid ? (key[r] >> a.shift) & (kBatchBins - 1u) : 0u;
    unsigned long long same = __ballot(valid);
#pragma unroll
    for (uint32_t bit = 0; bit < kBatchDigitBits; ++bit) {
      const bool one = ((digit >> bit) & 1u) != 0u;
      const unsigned long long ones = __ballot(one);
      same &= one ? ones : ~ones;
    }
    const uint32_t below = lanes_below(same);
    const uint32_t before = s_hist[wave][digit];
    __builtin_amdgcn_wave_barrier();
    if (valid && below == 0u) s_hist[wave][digit] = before + (uint32_t)__popcll(same);
    __builtin_amdgcn_wave_barrier();
    rank[r] = before + below;
  }
  __syncthreads();

  // thread b: where bin b of this tile starts — digits below b (all tiles), bin b of earlier tiles — then wave by wave
  {
    uint32_t unused_total;
    const uint32_t digits_below = batch_block_scan(tid < a.n_bins ? a.totals[tid] : 0u, s_wave, unused_total);
    uint32_t running = digits_below + (tid < a.n_bins ? a.counts[(size_t)tid * a.n_tiles + tile] : 0u);
#pragma unroll
    for (uint32_t w = 0; w < kWaves; ++w) {
      const uint32_t c = s_hist[w][tid];
      s_hist[w][tid] = running;
      running += c;
    }
  }
  __syncthreads();

#pragma unroll
  for (uint32_t r = 0; r < kBatchRounds; ++r) {
    const uint32_t idx = batch_index(tile, wave, r, lane);
    const bool valid = key[r] != kBatchNone;
    uint32_t slot = kBatchNone;
    if (valid) {
      slot = s_hist[wave][(key[r] >> a.shift) & (kBatchBins - 1u)] + rank[r];
      if constexpr (kLast) {
        a.instance_ids[slot] = a.first_instance_base + idx;
        if (a.slot_of) a.slot_of[idx] = slot;
      } else {
        a.keys_out[slot] = key[r];
        a.ids_out[slot] = idx;
      }
    }
    if constexpr (kModel != 0) batch_store_models<kModel == 2>(a, idx, slot, s_stage);
  }
}

template <class Key, bool kGeneral>
__global__ __launch_bounds__(kTile) void mip_batch_lods_model_kernel(const typename Key::Args a) {
  __shared__ __attribute__((aligned(16))) BatchModelStage s_stage;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t tile = batch_tile(a);
#pragma unroll 1
  for (uint32_t r = 0; r < kBatchRounds; ++r) {
    const uint32_t idx = batch_index(tile, wave, r, lane);
    const bool member = batch_lods_load_key<Key>(a, idx) != kBatchNone;
    batch_store_models<kGeneral>(a, idx, member ? a.slot_of[idx] : kBatchNone, s_stage);
  }
}

// ---- commands: one per non-empty bucket of the chain, ascending, packed; the two counts. One workgroup. ----
static __global__ __launch_bounds__(kTile) __attribute__((unused)) void mip_batch_lods_commands_kernel(const LodBatchArgs a) {
  __shared__ uint32_t s_wave[kWaves];
  uint32_t cmds_before = 0, members_before = 0;
  for (uint32_t first = 0; first < a.n_buckets; first += kTile) {  // (the host refuses more than 2^31 buckets)
    const uint32_t b = first + threadIdx.x;
    const uint32_t c = b < a.n_buckets ? a.bucket_totals[b] : 0u;
    uint32_t chunk_members, chunk_cmds;
    const uint32_t slot = members_before + batch_block_scan(c, s_wave, chunk_members);
    const uint32_t at = cmds_before + batch_block_scan(c ? 1u : 0u, s_wave, chunk_cmds);
    if (c) {
      const uint32_t ml = a.bucket_lod[b];
      const uint32_t mesh = ml >> 3, lod = ml & 7u;
      const MeshChain& ch = a.chain[mesh];
      const MeshDraw md = a.mesh_draw[mesh];
      uint32_t* o = a.batch_cmds + (size_t)at * kCmdWords;
      o[0] = ch.index_len[lod];          // indexCount
      o[1] = c;                          // instanceCount
      o[2] = ch.index_offset[lod];       // firstIndex: the level's own range of the consolidated index buffer
      o[3] = (uint32_t)md.vertex_offset; // vertexOffset
      o[4] = slot;                       // firstInstance: the slot of the bucket's first member
    }
    cmds_before += chunk_cmds;
    members_before += chunk_members;
  }
  if (threadIdx.x == 0) {
    *a.batch_count = cmds_before;
    if (a.instance_count) *a.instance_count = members_before;
    *a.members_out = members_before;
  }
}

}  // namespace mip
