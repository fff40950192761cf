// batch_lods_kernel.hpp — the key policies of batched draws over the whole LOD chain (mip_batch_draws_lods,
// mip_batch_draws_ordered; extension, not reference behaviour). The stage itself is batch_kernel.hpp's.
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
//
// BatchLodChainKey (mip_batch_draws_lods): key = bucket, members of a bucket in draw order.
// BatchOrderedKey (mip_batch_draws_ordered): the members of a bucket in depth order, by the stage's stable sort over
//
//   key = bucket << 16 | D        B <= 65 536
//   K   = 0x7F80 if q is NaN, else bits(q) >> 16     the q the selection rule compares
//   D   = K (near first)  or  0x7F80 - K (far first)
//
// q is a sum of squares: never negative, so its bit pattern is monotone in its value and K lies in [0, 0x7F80] (+inf), the
// sign, the exponent and seven mantissa bits of q. Equal D keeps draw order because every pass is stable. D <= 0x7F80 and
// bucket <= 0xFFFF, so no key equals kBatchNone. Pass 0 sorts by the lowest digit of D and counts the members per BUCKET for
// the command writer; the sort always takes several passes (ceil((16 + key_bits(B)) / 8): three up to 256 buckets, four up to
// 65 536), and the matrices go through slot_of with BatchLodChainKey's model kernel: membership does not depend on the order.
#pragma once

#include "batch_kernel.hpp"
#include "mesh_chain.hpp"

#pragma clang fp contract(off)

namespace mip {

constexpr uint32_t kMaxLods = MIP_MAX_LODS;
constexpr uint32_t kLodModeDistance = MIP_LOD_DISTANCE, kLodModeRelative = MIP_LOD_RELATIVE;
constexpr uint32_t kBatchDepthMax = 0x7F80u;   // bits(+inf) >> 16: the largest K, and the K of a NaN
constexpr uint32_t kBatchOrderedMaxBuckets = 1u << (32u - kBatchDepthBits);
static_assert((((kBatchOrderedMaxBuckets - 1u) << kBatchDepthBits) | kBatchDepthMax) < kBatchNone, "no key is kBatchNone");

static_assert(sizeof(MeshChain::index_len) == kMaxLods * 4, "MeshChain (mesh_chain.hpp) holds MIP_MAX_LODS levels");

struct LodBatchArgs : BatchArgs {
  const MeshChain* chain;        // m
  const uint32_t* bucket_lod;    // B words: mesh << 3 | lod of every bucket (the command writer)
  float switch_sq[kMaxLods - 1];
};

struct OrderedBatchArgs : LodBatchArgs {
  uint32_t depth_flip;  // 0: D = K (near first); kBatchDepthMax: D = kBatchDepthMax - K (far first)
};

// What the policy selects for instance il: its bucket, whether it is a member, and the q the rule compared.
struct LodChainPick {
  uint32_t bucket;
  bool member;
  float q;
};

// `word` is the bitmap word that holds instance il's bit, (cx, cy, cz) the reference point: the frame's own below, a view's in
// batch_views_kernel.hpp.
template <uint32_t kMode>
__device__ __forceinline__ LodChainPick lod_chain_pick(const LodBatchArgs& a, uint32_t il, bool active, uint32_t word, float cx, float cy,
                                                       float cz) {
  const float px = a.pos[3 * (size_t)il + 0], py = a.pos[3 * (size_t)il + 1], pz = a.pos[3 * (size_t)il + 2];
  const uint32_t mesh = a.mesh_id[il];
  const uint4* piece = reinterpret_cast<const uint4*>(a.chain + mesh);
  const uint4 c0 = piece[0], c1 = piece[1];
  const uint32_t n_lods = c0.x;
  const float dx = cx - px, dy = cy - py, dz = cz - pz;
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
  return {c0.y + lod, member, q};
}

template <uint32_t kMode>
__device__ __forceinline__ LodChainPick lod_chain_pick(const LodBatchArgs& a, uint32_t il, bool active) {
  return lod_chain_pick<kMode>(a, il, active, a.bitmap[il >> 5], a.cam[0], a.cam[1], a.cam[2]);
}

// The bucket of instance il under the policy, or kBatchNone when it is not a member.
template <uint32_t kMode>
struct BatchLodChainKey : BatchInstanceKey<BatchLodChainKey<kMode>, LodBatchArgs> {
  static constexpr BatchBucketHist kBucketHist = BatchBucketHist::when_given;  // pass 0 of several
  static __device__ __forceinline__ uint32_t key(const LodBatchArgs& a, uint32_t il, bool active) {
    const LodChainPick s = lod_chain_pick<kMode>(a, il, active);
    return s.member ? s.bucket : kBatchNone;
  }
  static __device__ __forceinline__ uint32_t bucket_of(uint32_t key) { return key; }
};

// bucket << 16 | D of instance il under the policy and the order, or kBatchNone when it is not a member: q is formed once
// and serves the LOD count and K.
template <uint32_t kMode>
struct BatchOrderedKey : BatchInstanceKey<BatchOrderedKey<kMode>, OrderedBatchArgs> {
  static constexpr BatchBucketHist kBucketHist = BatchBucketHist::always;  // pass 0 is the only pass that forms keys
  static __device__ __forceinline__ uint32_t key(const OrderedBatchArgs& a, uint32_t il, bool active) {
    const LodChainPick s = lod_chain_pick<kMode>(a, il, active);
    const float q = s.q;
    const uint32_t k16 = q != q ? kBatchDepthMax : __float_as_uint(q) >> kBatchDepthBits;  // q >= 0 or NaN: the sign bit is clear otherwise
    const uint32_t depth = a.depth_flip ? a.depth_flip - k16 : k16;                       // a select, no branch
    return s.member ? (s.bucket << kBatchDepthBits) | depth : kBatchNone;
  }
  static __device__ __forceinline__ uint32_t bucket_of(uint32_t key) { return key >> kBatchDepthBits; }
};

// The command writer over the chain: bucket -> mesh << 3 | lod (bucket_lod), the level's own range of the consolidated index buffer.
struct BatchChainDraw {
  using Args = LodBatchArgs;
  static __device__ __forceinline__ BatchDraw draw(const LodBatchArgs& a, uint32_t b) {
    const uint32_t ml = a.bucket_lod[b];
    const uint32_t mesh = ml >> 3, lod = ml & 7u;
    const MeshChain& ch = a.chain[mesh];
    const MeshDraw md = a.mesh_draw[mesh];
    return {ch.index_len[lod], ch.index_offset[lod], (uint32_t)md.vertex_offset};
  }
};

}  // namespace mip
