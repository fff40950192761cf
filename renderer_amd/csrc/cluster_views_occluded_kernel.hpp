// cluster_views_occluded_kernel.hpp — mip_list_clusters_views_occluded (the visible-cluster lists for several views in one call,
// a depth pyramid per view; extension, not reference behaviour), gfx950: mip_list_clusters_views with box_occluded behind the
// plane test of every view that brings a pyramid. include/mi_instance_pipeline.h specifies it,
// tests/cluster_views_occluded_restatement.py restates it in numpy; the launch list is cluster_views_list_plan.hpp's, unchanged.
// Instantiated in api_cluster.hip only.
//
// ONE new kernel in the several-view cull kernel's place, in two forms that write the same words: the simple loop below and,
// behind it in this file, the PACKED form the library launches by default (MIP_TUNE_VIEWS_OCCLUDED_PACKED=0 selects the simple
// loop; DESIGN section 36 has both measured). The launches in front of it (count, scan, members) and behind it (word members,
// list count, list epilogue, list write) are mip_list_clusters_views' own and read only the survive planes:
//
//   cull       mip_cluster_views_cull_kernel's shape: 64 work items per wave and round, cluster_locate and cluster_world_box
//              ONCE, the start word once; then the uniform loop over the views. Per view v: a lane is live iff its item is
//              below W and bit v of its instance's mask is set; no live lane: a zero word, no arithmetic. passed = the ballot of
//              live && !coarse_culled against view v's planes. A view with a pyramid and passed != 0: the lanes that passed run
//              box_occluded under view v's pv, pyramid and extents, survive = the ballot of those not occluded; else survive =
//              passed. Lane 0 stores the word. The view's occlusion block (pv, pointer, extents: 80 B) is wave-uniform and
//              comes from the argument block by scalar loads, as the planes do
//   hidden     lane v of every wave adds popcount(passed & ~survive) of view v over the whole grid-stride loop (a select on
//              lane == v: no indexed register array); behind the loop a lane below n_views with a non-zero sum issues ONE
//              atomicAdd to hidden[lane]. Integer adds: the count is exact whatever the order. The host zeroes the n_views
//              words in front of the launches; hidden == null: neither the sums nor the atomics
//
// No workgroup waits for another and nothing depends on the order workgroups start in; the diagnostic build permutes the tiles.
#pragma once

#include "cluster_views_kernel.hpp"

#pragma clang fp contract(off)

namespace mip {

// What box_occluded reads of a view's MipOcclusion; pyramid == null: the view is tested against its planes alone.
struct ClusterViewOcclusion {
  float pv[16];
  const float* pyramid;
  uint32_t width, height;
};
static_assert(sizeof(ClusterViewOcclusion) == 80, "the per-view occlusion block is pv, the pointer and the extents");

struct ClusterViewOccludedArgs {
  ClusterViewArgs v;             // the several-view front's arguments, as its kernels take them
  ClusterViewOcclusion occ[kClusterMaxViews];
  uint32_t* hidden;              // n_views words, zeroed in front of the launch, or null
};
static_assert(sizeof(ClusterViewOccludedArgs) <= 4096, "the cull kernel's arguments exceed the 4 096-byte kernel-argument limit");

// cull, views form with a pyramid per view: the world box once per work item, the plane test once per view with a live lane,
// the Hi-Z test once per view with a pyramid and a lane that passed.
// Three workgroups per CU, where the plain views cull asks for four: box_occluded inside the view loop, with the world box, the
// item and the mask live around it, wants 161 VGPRs; held to the 128 of four workgroups the compiler spills 20 bytes per lane
// to scratch, under either scheduling strategy. No scratch is the requirement here.
static __global__ __launch_bounds__(kClusterThreads, 3) __attribute__((unused)) void mip_cluster_views_cull_occluded_kernel(const ClusterViewOccludedArgs a) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const ClusterArgs& c = a.v.c;
  const uint32_t w_total = c.scalars[kClusterScW], members = c.scalars[kClusterScMembers];
  const uint32_t n_tiles = cluster_item_tiles(w_total);
  const uint32_t n_views = a.v.n_views;
  const bool count_hidden = a.hidden != nullptr;
  uint32_t acc = 0;  // lane v: view v's work items that passed the planes and are occluded, over this wave's rounds
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint32_t tile = cluster_loop_tile(c, t, n_tiles);
#pragma unroll 1
    for (uint32_t r = 0; r < kBatchRounds; ++r) {
      const unsigned long long base64 = (unsigned long long)tile * kClusterItemTile + wave * (kBatchRounds * 64u) + r * 64u;
      if (base64 >= w_total) break;  // (the whole wave; the rounds behind it start later still)
      const uint32_t base = (uint32_t)base64;
      const ClusterItem it = cluster_locate(c, base, lane, w_total, members);
      const bool active = base + lane < w_total;
      Instance inst;
      cluster_world_box(c, it, inst);
      const uint32_t mask = active ? (uint32_t)a.v.view_mask[it.inst] : 0u;
      const size_t word = base >> 6;  // < ceil(W / 64) <= words_stride: the scan held W to the bound the planes are sized by
      const unsigned long long start = __ballot(active && it.cluster == 0u);
      if (lane == 0u) a.v.view_words[word] = start;
#pragma unroll 1
      for (uint32_t v = 0; v < n_views; ++v) {
        const bool live = ((mask >> v) & 1u) != 0u;
        unsigned long long s = 0ull;
        if (__ballot(live) != 0ull) {  // (the whole wave)
          const bool passed = live && !coarse_culled(inst, a.v.view_planes[v]);
          const unsigned long long p = __ballot(passed);
          s = p;
          const ClusterViewOcclusion& o = a.occ[v];  // (uniform: scalar loads)
          if (o.pyramid && p != 0ull) {  // (the whole wave)
            bool survives = passed;
            if (passed) survives = !box_occluded(inst.mins, inst.maxs, o.pv, o.pyramid, o.width, o.height);  // only these lanes project and gather
            s = __ballot(survives);
            if (count_hidden) acc += lane == v ? (uint32_t)__popcll(p & ~s) : 0u;
          }
        }
        if (lane == 0u) a.v.view_words[(size_t)(1u + v) * a.v.words_stride + word] = s;
      }
    }
  }
  if (count_hidden && lane < n_views && acc != 0u) atomicAdd(&a.hidden[lane], acc);
}

// cull, the PACKED variant (MIP_TUNE_VIEWS_OCCLUDED_PACKED=1; DESIGN section 36 has the A/B): the same words and the same
// hidden counts as the kernel above. The view loop runs the plane test alone and notes, per lane, the views with a pyramid
// whose planes it passed; the (lane, view) pairs of the wave's 64 items are then numbered view by view and packed into full
// waves: pair q is tested by lane q mod 64 of chunk q / 64, which fetches the pair's world box from the lane that owns the item
// (six ds_bpermute) and the view's pv, pointer and extents from the argument block — per lane now, so by vector loads. An
// occluded pair sets its item's bit in the wave's word of its view (LDS, atomic or); lane v then forms view v's survive word
// and stores it. Every LDS word is private to one wave and LDS serves a wave's instructions in order: no barrier between waves.
constexpr uint32_t kClusterViewPairs = 64u * kClusterMaxViews;  // pairs of one wave and round at most

static __global__ __launch_bounds__(kClusterThreads, 4) __attribute__((unused)) void mip_cluster_views_cull_occluded_packed_kernel(const ClusterViewOccludedArgs a) {
  __shared__ uint16_t s_pair[kWaves][kClusterViewPairs];            // pair q of the wave: view << 8 | lane
  __shared__ unsigned long long s_occluded[kWaves][kClusterMaxViews];  // per view: the items of the round found occluded
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const ClusterArgs& c = a.v.c;
  const uint32_t w_total = c.scalars[kClusterScW], members = c.scalars[kClusterScMembers];
  const uint32_t n_tiles = cluster_item_tiles(w_total);
  const uint32_t n_views = a.v.n_views;
  const bool count_hidden = a.hidden != nullptr;
  uint32_t acc = 0;  // lane v: view v's work items that passed the planes and are occluded, over this wave's rounds
  if (lane < kClusterMaxViews) s_occluded[wave][lane] = 0ull;
  for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint32_t tile = cluster_loop_tile(c, t, n_tiles);
#pragma unroll 1
    for (uint32_t r = 0; r < kBatchRounds; ++r) {
      const unsigned long long base64 = (unsigned long long)tile * kClusterItemTile + wave * (kBatchRounds * 64u) + r * 64u;
      if (base64 >= w_total) break;  // (the whole wave; the rounds behind it start later still)
      const uint32_t base = (uint32_t)base64;
      const ClusterItem it = cluster_locate(c, base, lane, w_total, members);
      const bool active = base + lane < w_total;
      Instance inst;
      cluster_world_box(c, it, inst);
      const uint32_t mask = active ? (uint32_t)a.v.view_mask[it.inst] : 0u;
      const size_t word = base >> 6;  // < ceil(W / 64) <= words_stride: the scan held W to the bound the planes are sized by
      const unsigned long long start = __ballot(active && it.cluster == 0u);
      if (lane == 0u) a.v.view_words[word] = start;
      // the planes of every view; a view without a pyramid is finished here. Pairs are numbered view by view, lane by lane
      unsigned long long mine = 0ull;  // lane v: view v's passed word, when the view has a pyramid
      uint32_t pairs = 0u;             // (uniform)
#pragma unroll 1
      for (uint32_t v = 0; v < n_views; ++v) {
        const bool live = ((mask >> v) & 1u) != 0u;
        unsigned long long p = 0ull;
        bool passed = false;
        if (__ballot(live) != 0ull) {  // (the whole wave)
          passed = live && !coarse_culled(inst, a.v.view_planes[v]);
          p = __ballot(passed);
        }
        if (a.occ[v].pyramid && p != 0ull) {  // (the whole wave)
          if (passed) s_pair[wave][pairs + lanes_below(p)] = (uint16_t)(v << 8 | lane);  // < 64 (v + 1) <= kClusterViewPairs
          if (lane == v) mine = p;
          pairs += (uint32_t)__popcll(p);
        } else if (lane == 0u) {
          a.v.view_words[(size_t)(1u + v) * a.v.words_stride + word] = p;
        }
      }
      if (pairs == 0u) continue;  // (the whole wave) every view's word is stored: a view with a pyramid and no lane that passed got its zero above
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll 1
      for (uint32_t first = 0; first < pairs; first += 64u) {  // (uniform)
        const bool has = first + lane < pairs;
        const uint32_t pair = has ? (uint32_t)s_pair[wave][first + lane] : lane;  // an idle lane: view 0, its own box, nothing kept
        const uint32_t v = pair >> 8, from = pair & 63u;
        float mins[3], maxs[3];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {  // (called by the whole wave)
          mins[ax] = __shfl(inst.mins[ax], (int)from);
          maxs[ax] = __shfl(inst.maxs[ax], (int)from);
        }
        if (has) {
          const ClusterViewOcclusion& o = a.occ[v];  // v < n_views <= kClusterMaxViews; per lane: vector loads
          float pv[16];
#pragma unroll
          for (int k = 0; k < 16; ++k) pv[k] = o.pv[k];
          if (box_occluded(mins, maxs, pv, o.pyramid, o.width, o.height)) atomicOr(&s_occluded[wave][v], 1ull << from);
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      if (mine != 0ull) {  // lane v of a view with pairs: view v's survive word (lane v < n_views)
        const unsigned long long gone = s_occluded[wave][lane];  // a subset of `mine`
        s_occluded[wave][lane] = 0ull;  // for the next round
        a.v.view_words[(size_t)(1u + lane) * a.v.words_stride + word] = mine & ~gone;
        if (count_hidden) acc += (uint32_t)__popcll(gone);
      }
    }
  }
  if (count_hidden && lane < n_views && acc != 0u) atomicAdd(&a.hidden[lane], acc);
}

}  // namespace mip
