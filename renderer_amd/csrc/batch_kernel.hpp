// batch_kernel.hpp — batched draws (extension, not reference behaviour): one instanced command per (mesh, LOD) bucket.
//
// The members of a frame (visibility bit set and index_len[lod] > 0) are binned, stably, by bucket = mesh_id * 2 + lod:
// a least-significant-digit radix sort with 8-bit digits whose keys are formed from the instance columns exactly as the
// frame kernel forms its command (load_mesh_entry, lod_is_far: instance_kernel.hpp). Per digit, three launches on one stream:
//
//   count    one tile per workgroup: a 256-bin histogram of the tile in LDS -> counts[bin][tile]
//   rowscan  one workgroup per bin: exclusive scan of the bin's row over the tiles, in place; the row's sum -> totals[bin]
//   scatter  one tile per workgroup: a lane's slot = (digits below its own, from totals) + (its bin in earlier tiles, from
//            counts) + (its rank inside tile and bin: ballot match + mbcnt, waves in instance order), so a bin keeps draw order
//
// and one launch of a single workgroup that turns bucket totals into packed commands, batch_count and instance_count.
// No workgroup waits for another; nothing depends on the order workgroups start in.
//
// 2 m <= 256 buckets (every BASELINE configuration): ONE digit, straight from the instance columns to instance_ids (and
// batch_model). More buckets: pass 0 also writes a (key, instance) list, further passes sort that list (its length, the
// member count, is read from device memory; the grid is sized for N), and the matrices are stored by a kernel of their own
// that walks the instances in draw order — the arithmetic tier of a matrix is chosen per 64 consecutive instances
// (instance_tiered), which a pass over a sorted list could not reproduce.
//
// A tile is kBatchTile = 1024 instances: wave w of the workgroup takes instances [256 w, 256 w + 256) of it in four rounds of
// 64 CONSECUTIVE instances, aligned as the frame kernel's waves are — so instance_tiered decides for the same 64 instances as in
// mip_run and batch_model is byte-identical to its `model` output — and four times fewer rows of counts than a 256-instance tile.
//
// The stage is written once, over a KEY POLICY that says where a pass's keys come from:
//
//   Args                     the kernel's argument block: BatchArgs or a struct derived from it (the host fills the most derived one)
//   kFromList                the pass reads the (key, instance) list of the pass before it, not the instance columns
//   kBucketHist              whether count adds every member to bucket_hist[bucket_of(key)]: never / when the pointer is given / always
//   load(a, idx, list_len)   the key of entry idx, or kBatchNone
//   id(a, idx)               the instance behind entry idx
//   bucket_of(key)           the bucket a key belongs to
//
// BatchPickLodKey (mip_batch_draws) and BatchListKey (the later passes of any several-pass sort) are below; the policies over
// the whole LOD chain (mip_batch_draws_lods, mip_batch_draws_ordered) are in batch_lods_kernel.hpp, the policy over several
// views (mip_batch_draws_views) and its command writer in batch_views_kernel.hpp, the policy that sorts by depth across
// buckets (mip_batch_draws_sorted) and the run stage behind it in batch_sorted_kernel.hpp. The command writer takes a
// policy of its own: how a bucket maps to (indexCount, firstIndex, vertexOffset). Instantiated in api_batch.hip only.
#pragma once

#include "batch_plan.hpp"
#include "instance_kernel.hpp"

#pragma clang fp contract(off)

namespace mip {

constexpr uint32_t kBatchRounds = 4;
constexpr uint32_t kBatchTile = kTile * kBatchRounds;
constexpr uint32_t kBatchBins = 256;
constexpr uint32_t kBatchNone = 0xffffffffu;  // the key of an instance that is not a member; a slot that is not stored
static_assert(kTile == 256 && kWaves == 4, "one thread per bin; four waves of four rounds");
static_assert(kBatchBins == 1u << kBatchDigitBits, "one bin per value of a digit");

struct BatchArgs {
  // resident inputs
  const float* pos;
  const float4* rot;
  const float* scale;
  const uint32_t* mesh_id;
  const MeshEntry* meshes;
  const MeshDraw* mesh_draw;
  const uint32_t* bitmap;      // ceil(n / 32) words
  uint32_t n;                  // resident instances
  uint32_t n_tiles;            // tiles of kBatchTile instances = workgroups of count / scatter / model; the row pitch of counts
  uint32_t n_buckets;          // 2 m
  uint32_t n_bins;             // digits of this pass that can occur: n_buckets in the one-pass case, else 256
  uint32_t shift;              // this pass's digit = (key >> shift) & 255
  uint32_t first_instance_base;
  float cam[3];
  // per pass
  uint32_t* counts;            // [n_bins][n_tiles]
  uint32_t* totals;            // [256]
  const uint32_t* members;     // list passes: entries of the list (written by the command kernel)
  const uint32_t* keys_in;     // list passes
  const uint32_t* ids_in;
  uint32_t* keys_out;          // every pass but the last
  uint32_t* ids_out;
  uint32_t* bucket_hist;       // pass 0 of several: members per bucket (device-scope adds), else null
  // outputs
  uint32_t* instance_ids;      // last pass
  uint32_t* slot_of;           // last pass of several, with batch_model: slot of every member, by instance
  float4* batch_model;         // or null
  // command kernel
  const uint32_t* bucket_totals;  // n_buckets words: `totals` (one pass) or `bucket_hist`
  uint32_t* batch_cmds;
  uint32_t* batch_count;
  uint32_t* instance_count;    // or null
  uint32_t* members_out;       // scratch word the list passes read
#ifdef MIP_DEBUG_STAMPS
  uint32_t debug_tile_mult, debug_tile_add;  // diagnostic build only: a permutation of the tiles, as KernelArgs has it
#endif
};

__device__ __forceinline__ uint32_t batch_tile(const BatchArgs& a) {
  uint32_t tile = blockIdx.x;
#ifdef MIP_DEBUG_STAMPS
  if (a.debug_tile_mult) tile = (uint32_t)(((unsigned long long)blockIdx.x * a.debug_tile_mult + a.debug_tile_add) % a.n_tiles);
#endif
  return tile;
}

// Exclusive scan of one value per thread over the 256 threads of a workgroup; `total` is the sum. Two barriers.
__device__ __forceinline__ uint32_t batch_block_scan(uint32_t v, uint32_t* s_wave /* kWaves words */, uint32_t& total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t incl = wave_inclusive_scan(v);
  __syncthreads();  // s_wave may still be read from the previous call
  if (lane == 63u) s_wave[wave] = incl;
  __syncthreads();
  uint32_t before = 0;
  total = 0;
#pragma unroll
  for (uint32_t w = 0; w < kWaves; ++w) {
    const uint32_t s = s_wave[w];
    if (w < wave) before += s;
    total += s;
  }
  return before + incl - v;
}

// Whether pick_lod can return 1 for a mesh: MeshEntry.len1 / MeshDraw.src_offset1 fall back to LOD 0's values for a one-LOD
// mesh, and a two-LOD mesh may hold equal ones, so the tables need one more bit. It travels in MeshDraw's spare fourth word
// (`pad`, filled by mip_set_mesh_table), which no other kernel reads.
__device__ __forceinline__ uint32_t mesh_has_lod1(const MeshDraw& md) { return md.pad; }

// Instance (tile, wave, round, lane) of the tiling described at the top.
__device__ __forceinline__ uint32_t batch_index(uint32_t tile, uint32_t wave, uint32_t round, uint32_t lane) {
  return tile * kBatchTile + wave * (kBatchRounds * 64u) + round * 64u + lane;
}

// What the last scatter adds to an instance to form its entity id. An argument block that holds several views overloads
// this on its own type (batch_views_kernel.hpp): the base is then the one of the key's view.
__device__ __forceinline__ uint32_t batch_first_instance(const BatchArgs& a, uint32_t /*key*/) { return a.first_instance_base; }

// Where count adds a member of `bucket`: bucket_hist[bucket]. An argument block that keeps several copies of the histogram
// (one per residue of the tile number, so that concurrent tiles add to different cache lines) overloads this on its own type.
__device__ __forceinline__ uint32_t batch_hist_index(const BatchArgs&, uint32_t bucket, uint32_t /*tile*/) { return bucket; }

enum class BatchBucketHist { never, when_given, always };

// What the policies that form keys from the instance columns share: Key::key(a, il, active) sees an index in bounds (an idle
// lane loads the last instance, as in the frame kernel), and an entry IS its instance.
template <class Key, class A>
struct BatchInstanceKey {
  using Args = A;
  static constexpr bool kFromList = false;
  static __device__ __forceinline__ uint32_t load(const A& a, uint32_t idx, uint32_t) {
    const bool active = idx < a.n;
    return Key::key(a, active ? idx : a.n - 1u, active);
  }
  static __device__ __forceinline__ uint32_t id(const A&, uint32_t idx) { return idx; }
};

// mip_batch_draws: bucket = mesh_id * 2 + lod, or kBatchNone when instance il is not a member. The LOD and the length are the
// frame kernel's: lod_is_far against the frame's reference point, len1 falling back to LOD 0 for a one-LOD mesh — whose
// bucket is then LOD 0's, as pick_lod returns 0 for it at any distance.
struct BatchPickLodKey : BatchInstanceKey<BatchPickLodKey, BatchArgs> {
  static constexpr BatchBucketHist kBucketHist = BatchBucketHist::when_given;  // pass 0 of several
  static __device__ __forceinline__ uint32_t key(const BatchArgs& a, uint32_t il, bool active) {
    const uint32_t word = a.bitmap[il >> 5];
    const float px = a.pos[3 * (size_t)il + 0], py = a.pos[3 * (size_t)il + 1], pz = a.pos[3 * (size_t)il + 2];
    const uint32_t mesh = a.mesh_id[il];
    const MeshEntry mb = load_mesh_entry(a.meshes, mesh);
    const bool far_lod = lod_is_far(a.cam, px, py, pz);
    const uint32_t len = far_lod ? mb.len1 : mb.len0;
    const uint32_t lod = far_lod ? mesh_has_lod1(a.mesh_draw[mesh]) : 0u;
    const bool member = active && ((word >> (il & 31u)) & 1u) != 0u && len > 0u;
    return member ? mesh * 2u + lod : kBatchNone;
  }
  static __device__ __forceinline__ uint32_t bucket_of(uint32_t key) { return key; }
};

// The later passes of a several-pass sort, under any policy: the (key, instance) list the pass before wrote.
struct BatchListKey {
  using Args = BatchArgs;
  static constexpr bool kFromList = true;
  static constexpr BatchBucketHist kBucketHist = BatchBucketHist::never;  // pass 0 counted the buckets
  static __device__ __forceinline__ uint32_t load(const BatchArgs& a, uint32_t idx, uint32_t list_len) {
    return idx < list_len ? a.keys_in[idx] : kBatchNone;
  }
  static __device__ __forceinline__ uint32_t id(const BatchArgs& a, uint32_t idx) { return a.ids_in[idx]; }
};

// ---- count: the tile's histogram of this pass's digit; pass 0 of several also counts the members of every bucket ----
template <class Key>
__global__ __launch_bounds__(kTile) void mip_batch_count_kernel(const typename Key::Args a) {
  __shared__ uint32_t s_hist[kBatchBins];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t tile = batch_tile(a);
  const uint32_t list_len = Key::kFromList ? *a.members : 0u;
  s_hist[tid] = 0u;
  __syncthreads();
#pragma unroll
  for (uint32_t r = 0; r < kBatchRounds; ++r) {
    const uint32_t key = Key::load(a, batch_index(tile, wave, r, lane), list_len);
    if (key != kBatchNone) {
      atomicAdd(&s_hist[(key >> a.shift) & (kBatchBins - 1u)], 1u);
      if constexpr (Key::kBucketHist == BatchBucketHist::always) {
        atomicAdd(&a.bucket_hist[batch_hist_index(a, Key::bucket_of(key), tile)], 1u);  // < n_buckets: the host sizes bucket_hist for the table
      } else if constexpr (Key::kBucketHist == BatchBucketHist::when_given) {
        if (a.bucket_hist) atomicAdd(&a.bucket_hist[batch_hist_index(a, Key::bucket_of(key), tile)], 1u);
      }
    }
  }
  __syncthreads();
  if (tid < a.n_bins) a.counts[(size_t)tid * a.n_tiles + tile] = s_hist[tid];
}

// ---- rowscan: bin b's counts over the tiles become exclusive prefixes; the bin's total ----
static __global__ __launch_bounds__(kTile) __attribute__((unused)) void mip_batch_rowscan_kernel(const BatchArgs a) {
  __shared__ uint32_t s_wave[kWaves];
  uint32_t* row = a.counts + (size_t)blockIdx.x * a.n_tiles;
  uint32_t carry = 0;
  for (uint32_t first = 0; first < a.n_tiles; first += kTile) {
    const uint32_t t = first + threadIdx.x;
    const uint32_t v = t < a.n_tiles ? row[t] : 0u;
    uint32_t total;
    const uint32_t excl = batch_block_scan(v, s_wave, total);
    if (t < a.n_tiles) row[t] = carry + excl;
    carry += total;
  }
  if (threadIdx.x == 0) a.totals[blockIdx.x] = carry;
}

// What a bucket draws: the command writer's policy maps a bucket to these three words.
struct BatchDraw {
  uint32_t index_count, first_index, vertex_offset;
};

// mip_batch_draws: bucket = mesh * 2 + lod over MeshEntry / MeshDraw.
struct BatchPairDraw {
  using Args = BatchArgs;
  static __device__ __forceinline__ BatchDraw draw(const BatchArgs& a, uint32_t b) {
    const uint32_t mesh = b >> 1;
    const bool far_lod = (b & 1u) != 0u;
    const MeshEntry mb = load_mesh_entry(a.meshes, mesh);
    const MeshDraw md = a.mesh_draw[mesh];
    // firstIndex: the mesh's own range of the consolidated index buffer
    return {far_lod ? mb.len1 : mb.len0, far_lod ? md.src_offset1 : md.src_offset0, (uint32_t)md.vertex_offset};
  }
};

// ---- commands: one per non-empty bucket, ascending, packed; the two counts. One workgroup. ----
template <class Draw>
__global__ __launch_bounds__(kTile) void mip_batch_commands_kernel(const typename Draw::Args a) {
  __shared__ uint32_t s_wave[kWaves];
  uint32_t cmds_before = 0, members_before = 0;
  for (uint32_t first = 0; first < a.n_buckets; first += kTile) {  // (wraps only past 2^32 - 256 buckets: the host refuses those)
    const uint32_t b = first + threadIdx.x;
    const uint32_t c = b < a.n_buckets ? a.bucket_totals[b] : 0u;
    uint32_t chunk_members, chunk_cmds;
    const uint32_t slot = members_before + batch_block_scan(c, s_wave, chunk_members);
    const uint32_t at = cmds_before + batch_block_scan(c ? 1u : 0u, s_wave, chunk_cmds);
    if (c) {
      const BatchDraw d = Draw::draw(a, b);
      uint32_t* o = a.batch_cmds + (size_t)at * kCmdWords;
      o[0] = d.index_count;    // indexCount
      o[1] = c;                // instanceCount
      o[2] = d.first_index;    // firstIndex
      o[3] = d.vertex_offset;  // vertexOffset
      o[4] = slot;             // firstInstance: the slot of the bucket's first member
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

// LDS of the matrix stage: per wave, one round's 64 matrices (rows 0..2, 48-B pitch), NaN bits of row 3, slots.
struct BatchModelStage {
  float mat[kWaves][64 * 12];
  uint32_t row3[kWaves][64];
  uint32_t slot[kWaves][64];
};

// The model matrices of 64 consecutive instances (a wave's round), each stored at its slot (kBatchNone: not stored) as a whole
// 64-byte row: four lanes x 16 B, sixteen rows per store instruction. Called by EVERY lane of the workgroup, members or not:
// the arithmetic tier is the wave's (instance_tiered), as in the frame kernel, and the two barriers are the workgroup's.
template <bool kGeneral>
__device__ __forceinline__ void batch_store_models(const BatchArgs& a, uint32_t idx, uint32_t slot, BatchModelStage& s) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t il = idx < a.n ? idx : a.n - 1u;  // keep the loads of idle lanes in bounds (as the frame kernel does)
  const float px = a.pos[3 * (size_t)il + 0], py = a.pos[3 * (size_t)il + 1], pz = a.pos[3 * (size_t)il + 2];
  const float4 q = a.rot[il];
  const float sc = a.scale[il];
  MeshEntry mb = load_mesh_entry(a.meshes, a.mesh_id[il]);
  float r[3][3];
  quat_to_rotation(q.x, q.y, q.z, q.w, r);
  Instance inst;
  instance_tiered<false, kGeneral>(a, il, r, px, py, pz, sc, mb, inst);
  float4* dst = reinterpret_cast<float4*>(&s.mat[wave][lane * 12u]);
  dst[0] = make_float4(inst.m[0], inst.m[1], inst.m[2], inst.m[3]);
  dst[1] = make_float4(inst.m[4], inst.m[5], inst.m[6], inst.m[7]);
  dst[2] = make_float4(inst.m[8], inst.m[9], inst.m[10], inst.m[11]);
  s.row3[wave][lane] = inst.row3;
  s.slot[wave][lane] = slot;
  __syncthreads();
  const uint32_t col = lane & 3u;
#pragma unroll
  for (uint32_t p = 0; p < 4; ++p) {
    const uint32_t local = 16u * p + (lane >> 2);
    const uint32_t to = s.slot[wave][local];
    if (to != kBatchNone) {
      const float* src = &s.mat[wave][local * 12u];
      float w = (col == 3u) ? 1.0f : 0.0f;  // (store_piece's row 3)
      if constexpr (kGeneral)
        if ((s.row3[wave][local] >> col) & 1u) w = __uint_as_float(0x7fc00000u);
      store_stream16(a.batch_model + (size_t)to * 4 + col, make_float4(src[3u * col], src[3u * col + 1u], src[3u * col + 2u], w));
    }
  }
  __syncthreads();  // the stage is free for the next round
}

// ---- scatter: every member of the tile to its slot of this pass ----
// kLast: the key's last digit — slots are final (instance_ids, slot_of); else the pass writes the next (key, instance) list.
// kModel: 0 = no matrices, 1 = census-selected arithmetic (every resident instance is separable_safe), 2 = the tiers of kGeneral
template <class Key, bool kLast, int kModel>
__global__ __launch_bounds__(kTile) void mip_batch_scatter_kernel(const typename Key::Args a) {
  static_assert(!kModel || (!Key::kFromList && kLast), "matrices go out with the one pass that reads the instances in draw order");
  __shared__ uint32_t s_hist[kWaves][kBatchBins];
  __shared__ uint32_t s_wave[kWaves];
  __shared__ __attribute__((aligned(16))) std::conditional_t<kModel != 0, BatchModelStage, uint32_t> s_stage;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t tile = batch_tile(a);
  const uint32_t list_len = Key::kFromList ? *a.members : 0u;
#pragma unroll
  for (uint32_t w = 0; w < kWaves; ++w) s_hist[w][tid] = 0u;
  __syncthreads();

  // rank inside (tile, bin): the wave's own histogram row counts what its earlier rounds held; the lanes of a round that
  // share a digit find each other by eight ballots, the first of them adds the group to the row
  uint32_t key[kBatchRounds], rank[kBatchRounds];
#pragma unroll
  for (uint32_t r = 0; r < kBatchRounds; ++r) {
    key[r] = Key::load(a, batch_index(tile, wave, r, lane), list_len);
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
      slot = s_hist[wave][(key[r] >> a.shift) & (kBatchBins - 1u)] + rank[r];  // < members <= n
      const uint32_t id = Key::id(a, idx);
      if constexpr (kLast) {
        a.instance_ids[slot] = batch_first_instance(a, key[r]) + id;
        if (a.slot_of) a.slot_of[id] = slot;
      } else {
        a.keys_out[slot] = key[r];
        a.ids_out[slot] = id;
      }
    }
    if constexpr (kModel != 0) batch_store_models<kModel == 2>(a, idx, slot, s_stage);
  }
}

// ---- matrices of a frame that took several passes: the instances in draw order, each member to slot_of[instance] ----
template <class Key, bool kGeneral>
__global__ __launch_bounds__(kTile) void mip_batch_model_kernel(const typename Key::Args a) {
  static_assert(!Key::kFromList, "membership is formed from the instance columns");
  __shared__ __attribute__((aligned(16))) BatchModelStage s_stage;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t tile = batch_tile(a);
#pragma unroll 1
  for (uint32_t r = 0; r < kBatchRounds; ++r) {
    const uint32_t idx = batch_index(tile, wave, r, lane);
    const bool member = Key::load(a, idx, 0u) != kBatchNone;
    batch_store_models<kGeneral>(a, idx, member ? a.slot_of[idx] : kBatchNone, s_stage);
  }
}

}  // namespace mip
