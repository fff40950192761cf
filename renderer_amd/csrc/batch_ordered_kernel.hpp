// batch_ordered_kernel.hpp — depth-ordered batched draws (mip_batch_draws_ordered; extension, not reference behaviour).
//
// mip_batch_draws_lods with the members of a bucket in depth order: the stage's stable radix sort over a 32-bit key
//
//   key = bucket << 16 | D        bucket = lod_base[mesh] + lod under the policy (BatchLodChainKey's rule, B <= 65 536)
//   K   = 0x7F80 if q is NaN, else bits(q) >> 16     q = |cam - pos|^2, the float32 the selection rule compares
//   D   = K (near first)  or  0x7F80 - K (far first)
//
// q is a sum of squares: never negative, so its bit pattern is monotone in its value and K lies in [0, 0x7F80] (+inf), the
// sign, the exponent and seven mantissa bits of q. Equal D keeps draw order because every pass is stable. D <= 0x7F80 and
// bucket <= 0xFFFF, so no key equals kBatchNone.
//
// Pass 0 (the kernels below) forms keys from the instance columns, sorts by the lowest digit of D into a (key, instance) list
// and counts the members per BUCKET (key >> 16) for the command writer; every later digit is batch_kernel.hpp's list pass
// (mip_batch_count_kernel<true>, mip_batch_scatter_kernel<true, ...>), the commands are mip_batch_lods_commands_kernel's and
// the matrices mip_batch_lods_model_kernel's through slot_of: membership does not depend on the order. The sort always takes
// several passes (ceil((16 + key_bits(B)) / 8): three up to 256 buckets, four up to 65 536).
// No workgroup waits for another; nothing depends on the order workgroups start in.
//
// The two kernels are the statements of mip_batch_lods_count_kernel and mip_batch_lods_scatter_kernel<Key, false, 0>, written
// out and not shared with them through a common body, as batch_lods_kernel.hpp explains: the gfx950 text of the existing
// kernels is pinned. Instantiated in api_batch.hip only.
#pragma once

#include "batch_lods_kernel.hpp"

#pragma clang fp contract(off)

namespace mip {

constexpr uint32_t kBatchDepthBits = 16;       // D's field of the key
constexpr uint32_t kBatchDepthMax = 0x7F80u;   // bits(+inf) >> 16: the largest K, and the K of a NaN
constexpr uint32_t kBatchOrderedMaxBuckets = 1u << (32u - kBatchDepthBits);
static_assert((((kBatchOrderedMaxBuckets - 1u) << kBatchDepthBits) | kBatchDepthMax) < kBatchNone, "no key is kBatchNone");

struct OrderedBatchArgs : LodBatchArgs {
  uint32_t depth_flip;  // 0: D = K (near first); kBatchDepthMax: D = kBatchDepthMax - K (far first)
};

// bucket << 16 | D of instance il under the policy and the order, or kBatchNone when it is not a member. The LOD rule is
// BatchLodChainKey<kMode>::key's, statement for statement, so that q is formed once and serves the LOD count and K.
template <uint32_t kMode>
struct BatchOrderedKey {
  using Args = OrderedBatchArgs;
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
    const uint32_t k16 = q != q ? kBatchDepthMax : __float_as_uint(q) >> kBatchDepthBits;  // q >= 0 or NaN: the sign bit is clear otherwise
    const uint32_t depth = a.depth_flip ? a.depth_flip - k16 : k16;                       // a select, no branch
    return member ? ((c0.y + lod) << kBatchDepthBits) | depth : kBatchNone;
  }
};

// ---- pass 0, count: the tile's histogram of the key's lowest digit; the members of every bucket ----
template <class Key>
__global__ __launch_bounds__(kTile) void mip_batch_ordered_count_kernel(const typename Key::Args a) {
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
      atomicAdd(&a.bucket_hist[key >> kBatchDepthBits], 1u);  // < n_buckets: the host sizes bucket_hist for the table
    }
  }
  __syncthreads();
  if (tid < a.n_bins) a.counts[(size_t)tid * a.n_tiles + tile] = s_hist[tid];
}

// ---- pass 0, scatter: every member of the tile to its slot of the (key, instance) list ----
template <class Key>
__global__ __launch_bounds__(kTile) void mip_batch_ordered_scatter_kernel(const typename Key::Args a) {
  __shared__ uint32_t s_hist[kWaves][kBatchBins];
  __shared__ uint32_t s_wave[kWaves];
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
    if (key[r] != kBatchNone) {
      const uint32_t slot = s_hist[wave][(key[r] >> a.shift) & (kBatchBins - 1u)] + rank[r];  // < members <= n
      a.keys_out[slot] = key[r];
      a.ids_out[slot] = idx;
    }
  }
}

}  // namespace mip
