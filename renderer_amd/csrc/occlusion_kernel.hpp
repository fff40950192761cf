// occlusion_kernel.hpp — EXTENSION (not reference behaviour): occlusion culling against a depth pyramid (Hi-Z), gfx950.
//   mip_depth_pyramid_kernel    the max pyramid of a D16_UNORM / D32_SFLOAT depth image in ONE launch
//   mip_occluded_frame_kernel   the commands-first frame kernel with one more keep predicate, built on its tile-tail helpers
//                               (instance_kernel.hpp): a frustum-visible candidate is dropped when its projected world box lies
//                               behind the pyramid's depth
// The test and the pyramid are specified in include/mi_instance_pipeline.h (MipOcclusion) and restated in numpy by
// tests/occlusion_restatement.py; instantiated in api_occlusion.hip only.
#pragma once

#include "instance_kernel.hpp"

#pragma clang fp contract(off)

namespace mip {

constexpr uint32_t kDepthUnorm16 = 0, kDepthFloat32 = 1;
constexpr uint32_t kMaxDepthExtent = 16384;
constexpr uint32_t kPyramidBlock = 64;       // depth pixels per side of one workgroup's block = one texel of level 5
constexpr uint32_t kPyramidBlockLevels = 6;  // levels 0-5 are built by the block's own workgroup
constexpr uint32_t kPyramidTopTexels = 4096; // a level 5 up to this size is reduced in LDS by the last workgroup

// Level k of the pyramid of a W x H image: ceil(W / 2^(k+1)) x ceil(H / 2^(k+1)).
__host__ __device__ constexpr uint32_t pyramid_level_extent(uint32_t side, uint32_t k) { return ((side - 1u) >> (k + 1u)) + 1u; }
// Levels down to 1 x 1 (>= 1 for any image of at least one pixel).
__host__ __device__ constexpr uint32_t pyramid_levels(uint32_t w, uint32_t h) {
  uint32_t k = 0;
  while (pyramid_level_extent(w, k) > 1u || pyramid_level_extent(h, k) > 1u) ++k;
  return k + 1u;
}

struct PyramidArgs {
  const unsigned char* depth;
  float* pyramid;
  uint32_t* counter;            // workgroups of this build that have finished levels 0-5 (one word per frame slot; the last resets it)
  unsigned long long pitch;     // bytes per depth row
  uint32_t width, height, format;
  uint32_t blocks_x, blocks;    // 64 x 64-pixel blocks
  uint32_t levels;
  uint32_t vec;                 // 1: depth and pitch are 16-byte aligned (whole 16-byte rows of pixels are one load)
  uint32_t level_w[16], level_h[16];
  unsigned long long level_off[16];  // in floats
};

// A depth pixel as the pyramid counts it: NaN is 1.0 (cleared), a zero is +0 (so that max is exact in any order).
__device__ __forceinline__ float pyramid_pixel(float v) { return v != v ? 1.0f : v + 0.0f; }

// (cluster_kernel.hpp includes this header for box_occluded alone, under MIP_OCCLUSION_DEVICE_HELPERS_ONLY: the pyramid kernel
// is not a template, so it is defined in api_occlusion.hip's translation unit only)
#ifndef MIP_OCCLUSION_DEVICE_HELPERS_ONLY
// Levels 0-5 of block (bx, by) by its own workgroup (the first level through 16-byte loads where the pitch allows), then — in
// the workgroup that finishes LAST — the levels above from level 5. Texels outside a level hold -inf in LDS: max ignores them.
__global__ __launch_bounds__(256) void mip_depth_pyramid_kernel(const PyramidArgs a) {
  __shared__ float s0[32 * 32];  // level 0 of the block
  __shared__ float s1[16 * 16 + 8 * 8 + 4 * 4 + 2 * 2 + 1];  // levels 1 .. 5 of the block, one after another
  __shared__ float s_top[kPyramidTopTexels];
  __shared__ uint32_t s_last;
  const uint32_t t = threadIdx.x;
  const uint32_t bx = blockIdx.x % a.blocks_x, by = blockIdx.x / a.blocks_x;
  const uint32_t px0 = bx * kPyramidBlock, py0 = by * kPyramidBlock;
  const float kNone = -__builtin_inff();

  // ---- level 0 of the block: 4 texels per thread ----
  if (a.format == kDepthUnorm16) {
    // 8 x 2 pixels per thread: one 16-byte load per row. Max on the integers, converted once (the conversion is monotone).
    const uint32_t tx = t & 7u, ty = t >> 3;
    const uint32_t x = px0 + tx * 8u;
    uint32_t m[4] = {0u, 0u, 0u, 0u};
    bool any[4] = {false, false, false, false};
#pragma unroll
    for (uint32_t r = 0; r < 2; ++r) {
      const uint32_t y = py0 + ty * 2u + r;
      if (y >= a.height) continue;
      const uint16_t* row = reinterpret_cast<const uint16_t*>(a.depth + (size_t)y * a.pitch);
      uint32_t p[8];
      if (a.vec && x + 8u <= a.width) {
        const uint4 w = *reinterpret_cast<const uint4*>(row + x);
        p[0] = w.x & 0xffffu; p[1] = w.x >> 16; p[2] = w.y & 0xffffu; p[3] = w.y >> 16;
        p[4] = w.z & 0xffffu; p[5] = w.z >> 16; p[6] = w.w & 0xffffu; p[7] = w.w >> 16;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) any[j] = true;
      } else {
#pragma unroll
        for (uint32_t e = 0; e < 8; ++e) {
          const bool in = x + e < a.width;
          p[e] = in ? row[x + e] : 0u;
          if (in) any[e >> 1] = true;
        }
      }
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) m[j] = max(m[j], max(p[2 * j], p[2 * j + 1]));
    }
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) s0[ty * 32u + tx * 4u + j] = any[j] ? (float)m[j] / 65535.0f : kNone;
  } else {
    // 4 x 4 pixels per thread: one 16-byte load per row
    const uint32_t tx = t & 15u, ty = t >> 4;
    const uint32_t x = px0 + tx * 4u;
    float m[2][2] = {{kNone, kNone}, {kNone, kNone}};
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
      const uint32_t y = py0 + ty * 4u + r;
      if (y >= a.height) continue;
      const float* row = reinterpret_cast<const float*>(a.depth + (size_t)y * a.pitch);
      float p[4];
      if (a.vec && x + 4u <= a.width) {
        const float4 w = *reinterpret_cast<const float4*>(row + x);
        p[0] = pyramid_pixel(w.x); p[1] = pyramid_pixel(w.y); p[2] = pyramid_pixel(w.z); p[3] = pyramid_pixel(w.w);
      } else {
#pragma unroll
        for (uint32_t e = 0; e < 4; ++e) p[e] = x + e < a.width ? pyramid_pixel(row[x + e]) : kNone;
      }
      m[r >> 1][0] = fmaxf(m[r >> 1][0], fmaxf(p[0], p[1]));
      m[r >> 1][1] = fmaxf(m[r >> 1][1], fmaxf(p[2], p[3]));
    }
#pragma unroll
    for (uint32_t j = 0; j < 2; ++j)
#pragma unroll
      for (uint32_t i = 0; i < 2; ++i) s0[(ty * 2u + j) * 32u + tx * 2u + i] = m[j][i];
  }
  __syncthreads();
  // level 0 out, coalesced rows of 32
#pragma unroll
  for (uint32_t q = 0; q < 4; ++q) {
    const uint32_t idx = t + 256u * q, lx = idx & 31u, ly = idx >> 5;
    const uint32_t gx = bx * 32u + lx, gy = by * 32u + ly;
    if (gx < a.level_w[0] && gy < a.level_h[0]) a.pyramid[a.level_off[0] + (size_t)gy * a.level_w[0] + gx] = s0[idx];
  }

  // ---- levels 1-5 of the block: 16 x 16, 8 x 8, 4 x 4, 2 x 2, 1 x 1 ----
  {
    const float* src = s0;
    uint32_t src_side = 32u, dst_base = 0u;
#pragma unroll
    for (uint32_t k = 1; k < kPyramidBlockLevels; ++k) {
      const uint32_t side = src_side >> 1;
      float v = kNone;
      if (t < side * side) {
        const uint32_t lx = t % side, ly = t / side;
        const float* s = src + (2u * ly) * src_side + 2u * lx;
        v = fmaxf(fmaxf(s[0], s[1]), fmaxf(s[src_side], s[src_side + 1u]));
        const uint32_t gx = bx * side + lx, gy = by * side + ly;
        const bool exists = k < a.levels && gx < a.level_w[k] && gy < a.level_h[k];
        float* dst = &a.pyramid[a.level_off[k] + (size_t)gy * a.level_w[k] + gx];
        if (!exists) v = kNone;
        else if (k == kPyramidBlockLevels - 1u) __hip_atomic_store(dst, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // read by the last workgroup
        else *dst = v;
        s1[dst_base + t] = v;
      }
      __syncthreads();
      src = s1 + dst_base;
      dst_base += side * side;
      src_side = side;
    }
  }
  if (a.levels <= kPyramidBlockLevels) return;  // (then there is one block: W, H <= 64)

  // ---- the last workgroup to get here builds levels 6 .. from level 5 ----
  // The tile prefix's discipline (instance_kernel.hpp): the block's level-5 texel — written by thread 0, the only texel another
  // workgroup reads — is a relaxed agent-scope atomic store (written through to where every XCD sees it: 8 XCDs, their L2s not
  // coherent with each other), complete before the same thread moves the counter; the last workgroup reads level 5 with
  // agent-scope atomic loads. (An agent-scope release FENCE in every workgroup writes back the whole L2 each time: measured,
  // 1080p D16 29.6 us, 2160p f32 118 us.)
  if (t == 0u) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the level-5 store has been acknowledged
    const uint32_t done = __hip_atomic_fetch_add(a.counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = done == a.blocks - 1u ? 1u : 0u;
    if (s_last) __hip_atomic_store(a.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // for the slot's next build
  }
  __syncthreads();
  if (!s_last) return;

  const uint32_t w5 = a.level_w[5], h5 = a.level_h[5];
  if (w5 * h5 <= kPyramidTopTexels && a.level_w[6] * a.level_h[6] <= kPyramidTopTexels / 4u) {
    // level 5 into LDS once; every level above is reduced there and only written out
    for (uint32_t idx = t; idx < w5 * h5; idx += 256u)
      s_top[idx] = __hip_atomic_load(&a.pyramid[a.level_off[5] + idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    uint32_t sw = w5, sh = h5;
    for (uint32_t k = kPyramidBlockLevels; k < a.levels; ++k) {
      const uint32_t dw = a.level_w[k], dh = a.level_h[k];
      float v[kPyramidTopTexels / 4 / 256];  // (level 6 has at most 4096 / 4 texels)
#pragma unroll
      for (uint32_t q = 0; q < kPyramidTopTexels / 4 / 256; ++q) {
        const uint32_t idx = t + 256u * q;
        v[q] = kNone;
        if (idx < dw * dh) {
          const uint32_t x = idx % dw, y = idx / dw;
          const uint32_t x1 = min(2u * x + 1u, sw - 1u), y1 = min(2u * y + 1u, sh - 1u);
          v[q] = fmaxf(fmaxf(s_top[2u * y * sw + 2u * x], s_top[2u * y * sw + x1]), fmaxf(s_top[y1 * sw + 2u * x], s_top[y1 * sw + x1]));
          a.pyramid[a.level_off[k] + idx] = v[q];
        }
      }
      __syncthreads();  // every thread has read level k-1
#pragma unroll
      for (uint32_t q = 0; q < kPyramidTopTexels / 4 / 256; ++q)
        if (t + 256u * q < dw * dh) s_top[t + 256u * q] = v[q];
      __syncthreads();
      sw = dw;
      sh = dh;
    }
  } else {
    // images above 4096 pixels a side: level by level through memory, this workgroup alone
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    for (uint32_t k = kPyramidBlockLevels; k < a.levels; ++k) {
      const uint32_t dw = a.level_w[k], dh = a.level_h[k], sw = a.level_w[k - 1], sh = a.level_h[k - 1];
      const float* src = a.pyramid + a.level_off[k - 1];
      for (uint32_t idx = t; idx < dw * dh; idx += 256u) {
        const uint32_t x = idx % dw, y = idx / dw;
        const uint32_t x1 = min(2u * x + 1u, sw - 1u), y1 = min(2u * y + 1u, sh - 1u);
        const float v = fmaxf(fmaxf(src[(size_t)2u * y * sw + 2u * x], src[(size_t)2u * y * sw + x1]),
                              fmaxf(src[(size_t)y1 * sw + 2u * x], src[(size_t)y1 * sw + x1]));
        a.pyramid[a.level_off[k] + idx] = v;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      __syncthreads();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
  }
}

#endif  // MIP_OCCLUSION_DEVICE_HELPERS_ONLY

// ---------------------------------------------------------------------------------------
// the occluded frame
// ---------------------------------------------------------------------------------------

struct OcclusionArgs {
  KernelArgs k;                  // exactly what the frame kernel of the same mip_run would get (fill_kernel_args)
  const float* pyramid;
  const uint32_t* candidates;    // or null: every instance
  uint32_t* occluded_bitmap;     // or null
  uint32_t candidates_xor;       // 0, or ~0 under MIP_OCC_CANDIDATES_INVERTED
  uint32_t width, height;
  float pv[16];
};

// The occlusion test of include/mi_instance_pipeline.h (steps 1-9) on one world box. true = occluded.
__device__ __forceinline__ bool box_occluded(const float (&mins)[3], const float (&maxs)[3], const float (&pv)[16], const float* pyramid,
                                             uint32_t width, uint32_t height) {
  const float wf = (float)width, hf = (float)height;
  float umin = __builtin_inff(), umax = -__builtin_inff(), vmin = __builtin_inff(), vmax = -__builtin_inff();
  float zmin = __builtin_inff();
  bool ok = true;
#pragma unroll
  for (uint32_t c = 0; c < 8; ++c) {
    const float x = (c & 1u) ? maxs[0] : mins[0], y = (c & 2u) ? maxs[1] : mins[1], z = (c & 4u) ? maxs[2] : mins[2];
    float clip[4];
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) clip[r] = ((pv[r] * x + pv[4 + r] * y) + pv[8 + r] * z) + pv[12 + r];
    const float big = fmaxf(fmaxf(fabsf(clip[0]), fabsf(clip[1])), fmaxf(fabsf(clip[2]), fabsf(clip[3])));
    ok = ok && big <= 3.40282347e+38f && clip[0] == clip[0] && clip[1] == clip[1] && clip[2] == clip[2] && clip[3] > 0.0f;
    const float rw = 1.0f / clip[3];
    const float nx = clip[0] * rw, ny = clip[1] * rw, nz = clip[2] * rw;
    const float u = (nx * 0.5f + 0.5f) * wf;
    const float v = (0.5f - ny * 0.5f) * hf;
    umin = fminf(umin, u); umax = fmaxf(umax, u);
    vmin = fminf(vmin, v); vmax = fmaxf(vmax, v);
    zmin = fminf(zmin, nz);
  }
  if (!ok) return false;
  const int x0 = (int)fminf(fmaxf(floorf(umin), 0.0f), wf - 1.0f), x1 = (int)fminf(fmaxf(floorf(umax), 0.0f), wf - 1.0f);
  const int y0 = (int)fminf(fmaxf(floorf(vmin), 0.0f), hf - 1.0f), y1 = (int)fminf(fmaxf(floorf(vmax), 0.0f), hf - 1.0f);
  uint32_t k = 0;
  size_t off = 0;
  while (((x1 >> (k + 1u)) - (x0 >> (k + 1u))) > 1 || ((y1 >> (k + 1u)) - (y0 >> (k + 1u))) > 1) {
    off += (size_t)pyramid_level_extent(width, k) * pyramid_level_extent(height, k);
    ++k;
  }
  const uint32_t lw = pyramid_level_extent(width, k);
  const float* lvl = pyramid + off;
  const uint32_t tx0 = (uint32_t)x0 >> (k + 1u), tx1 = (uint32_t)x1 >> (k + 1u);
  const uint32_t ty0 = (uint32_t)y0 >> (k + 1u), ty1 = (uint32_t)y1 >> (k + 1u);
  const float d = fmaxf(fmaxf(lvl[(size_t)ty0 * lw + tx0], lvl[(size_t)ty0 * lw + tx1]), fmaxf(lvl[(size_t)ty1 * lw + tx0], lvl[(size_t)ty1 * lw + tx1]));
  return d < 1.0f && zmin > d;
}

// The aggregate {Σ index_len of the kept : 32 | kept commands : 32} of tile u of an occluded frame, computed by ONE wave from
// the tile's inputs with the same predicate as the owner (frustum, candidate, occlusion): resolve_prefix's help.
template <bool kGeneral>
__device__ __forceinline__ unsigned long long help_occluded_aggregate(uint32_t u, uint32_t lane) {
  uint32_t cnt = 0, sum = 0;
#pragma nounroll
  for (uint32_t w = 0; w < kWaves; ++w) {
    // the argument block is fetched again for every 64 instances (an opaque pointer per pass): nothing of it stays alive across
    // the loop — the frame's 24 planes, camera and 16 pv words held across it spilled hundreds of scalar registers
    const auto* oa = cold_kernel_args<OcclusionArgs>();
    const auto* ka = &oa->k;
    float planes[24], cam[3], pv[16];
    cold_frame(ka, planes, cam);
#pragma unroll
    for (int k = 0; k < 16; ++k) pv[k] = oa->pv[k];
    const uint32_t n = ka->n;
    const uint32_t j = u * kTile + w * 64u + lane;
    const bool active = j < n;
    const uint32_t jl = active ? j : n - 1u;
    const float px = ka->pos[3 * (size_t)jl + 0], py = ka->pos[3 * (size_t)jl + 1], pz = ka->pos[3 * (size_t)jl + 2];
    const float4 q = ka->rot[jl];
    const float sc = ka->scale[jl];
    const uint32_t mesh = ka->mesh_id[jl];
    const uint32_t cand_word = oa->candidates ? oa->candidates[jl >> 5] ^ oa->candidates_xor : ~0u;
    MeshEntry mb = load_mesh_entry(ka->meshes, mesh);
    float r[3][3];
    quat_to_rotation(q.x, q.y, q.z, q.w, r);
    Instance inst;
    struct { const float* box_override; } no_box = {nullptr};
    instance_tiered<false, kGeneral>(no_box, jl, r, px, py, pz, sc, mb, inst);
    bool visible = active && !coarse_culled(inst, planes) && ((cand_word >> (jl & 31u)) & 1u);
    if (visible) visible = !box_occluded(inst.mins, inst.maxs, pv, oa->pyramid, oa->width, oa->height);
    const uint32_t len = lod_is_far(cam, px, py, pz) ? mb.len1 : mb.len0;
    cnt += (uint32_t)__popcll(__ballot(visible && len > 0u));
    sum += wave_sum(visible ? len : 0u);
  }
  return ((unsigned long long)sum << 32) | cnt;
}

// One tile of 256 instances per workgroup: the commands-first order of mip_instance_pipeline_kernel<false, kGeneral, 3> with
// its tile tail (instance_kernel.hpp: staging, the one-hop prefix, the copy-out, the matrix / TLAS / box stores). Model matrix,
// world box, frustum test and LOD by the same device functions; then, for the frustum-visible candidates only, the projection
// of the world box and a gather of at most four pyramid texels. The kept instances are compacted with the same prefix
// (publish / resolve / help) — the help applies the same predicate. Matrices, boxes and TLAS rows are written for every
// instance, as mip_run writes them; a second bitmap records the occluded candidates.
// Register bounds: 6 waves per SIMD (80 VGPRs) for the census-selected kernel and 4 for the one with the fall-back tiers — the
// tightest bounds at which neither spills to scratch (the help path, which projects and gathers too, sets the high-water mark).
#ifndef MIP_OCC_WAVES_PER_SIMD
#define MIP_OCC_WAVES_PER_SIMD 6
#endif
template <bool kGeneral>
__global__ __launch_bounds__(kTile, kGeneral ? 4 : MIP_OCC_WAVES_PER_SIMD) void mip_occluded_frame_kernel(const OcclusionArgs oa) {
  const KernelArgs& a = oa.k;
  __shared__ __attribute__((aligned(16))) float s_mat[kTile * 12];
  __shared__ uint32_t s_row3[kTile];
  __shared__ __attribute__((aligned(16))) uint32_t s_cmd[kTile * kCmdLdsWords];
  __shared__ uint32_t s_wave_count[kWaves], s_wave_sum[kWaves];
  __shared__ unsigned long long s_vis[kWaves], s_occ[kWaves];
  __shared__ unsigned long long s_tile_agg;

  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const bool want_cmds = a.cmds != nullptr;
  uint32_t tile = blockIdx.x;
#ifdef MIP_DEBUG_STAMPS
  if (a.debug_tile_mult) tile = (uint32_t)(((unsigned long long)blockIdx.x * a.debug_tile_mult + a.debug_tile_add) % a.n_tiles);
  const bool skip_publish = a.debug_skip_publish_tile == tile + 1u;
#else
  const bool skip_publish = false;
#endif
  const uint32_t tile_first = tile * kTile;
  const uint32_t i = tile_first + tid;
  const uint32_t n = a.n;
  const bool active = i < n;
  const uint32_t il = active ? i : n - 1u;

  const float px = a.pos[3 * (size_t)il + 0], py = a.pos[3 * (size_t)il + 1], pz = a.pos[3 * (size_t)il + 2];
  const float4 q = a.rot[il];
  const float sc = a.scale[il];
  const uint32_t mesh = a.mesh_id[il];
  const uint32_t cand_word = oa.candidates ? oa.candidates[il >> 5] ^ oa.candidates_xor : ~0u;  // one word per 32 lanes
  float planes[24], cam[3];
#pragma unroll
  for (int k = 0; k < 24; ++k) planes[k] = a.planes[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) cam[k] = a.cam[k];
  const uint32_t first_instance_base = a.first_instance_base, first_index_base = a.first_index_base;
  auto help = [lane](uint32_t u) { return help_occluded_aggregate<kGeneral>(u, lane); };

  if (want_cmds) {
    if (tid == 0) s_tile_agg = 0ull;
    __syncthreads();
  }
  MeshEntry mb = load_mesh_entry(a.meshes, mesh);

  float r[3][3];
  quat_to_rotation(q.x, q.y, q.z, q.w, r);
  Instance inst;
  instance_tiered<false, kGeneral>(a, il, r, px, py, pz, sc, mb, inst);

  int32_t vertex_offset_of_mesh = 0;
  if (want_cmds) vertex_offset_of_mesh = a.mesh_draw[mesh].vertex_offset;
  const bool in_frustum = active && !coarse_culled(inst, planes);
  const bool candidate = in_frustum && ((cand_word >> (il & 31u)) & 1u);
  // stage the matrix rows before the occlusion test: only the world box lives across it
  if (a.model || a.tlas_instances) {
    float4* dst = reinterpret_cast<float4*>(&s_mat[tid * 12]);
    dst[0] = make_float4(inst.m[0], inst.m[1], inst.m[2], inst.m[3]);
    dst[1] = make_float4(inst.m[4], inst.m[5], inst.m[6], inst.m[7]);
    dst[2] = make_float4(inst.m[8], inst.m[9], inst.m[10], inst.m[11]);
    s_row3[tid] = inst.row3 | (mesh << 4);
  }
  store_world_aabb(a, i, active, inst);
  bool occluded = false;
  if (candidate) occluded = box_occluded(inst.mins, inst.maxs, oa.pv, oa.pyramid, oa.width, oa.height);  // only these lanes project and gather
  const bool visible = candidate && !occluded;
  const bool far_lod = lod_is_far(cam, px, py, pz);
  const uint32_t len = far_lod ? mb.len1 : mb.len0;
  const bool keep = visible && len > 0u;
  const uint32_t len_vis = visible ? len : 0u;

  const unsigned long long keep_mask = __ballot(keep);
  const unsigned long long vis_mask = __ballot(visible);
  const unsigned long long occ_mask = __ballot(candidate && occluded);
  const uint32_t rank_in_wave = lanes_below(keep_mask);
  const uint32_t incl_sum = wave_inclusive_scan(len_vis);
  if (want_cmds && lane == 63u) {
    const uint32_t wc = (uint32_t)__popcll(keep_mask);
    s_wave_count[wave] = wc;
    s_wave_sum[wave] = incl_sum;
    const unsigned long long mine = ((unsigned long long)incl_sum << 32) | (1ull << kAggArrivalShift) | wc;
    const unsigned long long all = __hip_atomic_fetch_add(&s_tile_agg, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) + mine;
    if (((uint32_t)all >> kAggArrivalShift) == kWaves && !skip_publish) publish_aggregate(a, tile, (uint32_t)all & 0xffffu, (uint32_t)(all >> 32));
  }
  if (lane == 0u) {
    s_vis[wave] = vis_mask;
    s_occ[wave] = occ_mask;
  }

  const PieceStores d = piece_stores(a, tile_first);
  auto store_piece = [&](uint32_t p) { mip::store_piece<kGeneral>(a, d, s_mat, s_row3, tile_first, first_instance_base, lane, p); };
  auto store_bitmaps = [&]() {
    if (lane < 2u * kWaves) {
      const uint32_t word = (tile_first >> 5) + lane;
      if (word < a.bitmap_words) {
        if (a.bitmap) a.bitmap[word] = (uint32_t)(s_vis[lane >> 1] >> (32u * (lane & 1u)));
        if (oa.occluded_bitmap) oa.occluded_bitmap[word] = (uint32_t)(s_occ[lane >> 1] >> (32u * (lane & 1u)));
      }
    }
  };

  __syncthreads();  // staged matrices, wave aggregates and ballots are in LDS
  if (!want_cmds) {
#pragma unroll
    for (uint32_t p = 0; p < 4; ++p) store_piece(wave * 4u + p);
    if (wave == 0) store_bitmaps();
    return;
  }
  uint32_t wave_off_count = 0, wave_off_sum = 0, tile_count = 0, tile_sum = 0;
#pragma unroll
  for (uint32_t w = 0; w < kWaves; ++w) {
    const uint32_t wc = s_wave_count[w], ws = s_wave_sum[w];
    if (w < wave) { wave_off_count += wc; wave_off_sum += ws; }
    tile_count += wc;
    tile_sum += ws;
  }
  if (keep)
    stage_command<0>(a, &s_cmd[(wave_off_count + rank_in_wave) * kCmdLdsWords], len, wave_off_sum + (incl_sum - len_vis),
                     vertex_offset_of_mesh, first_instance_base + i, mesh, far_lod);
  __syncthreads();
  if (wave != 0) {  // waves 1-3: the bulk stores of the whole tile
    const uint32_t p0 = store_run_first(wave), p1 = store_run_first(wave + 1u);
    for (uint32_t p = p0; p < p1; ++p) store_piece(p);
    if (wave == 1) store_bitmaps();
    return;
  }
  // wave 0: the prefix over the earlier tiles, then the commands
  uint32_t base_count = 0, base_sum = 0;
  if (tile > 0) resolve_prefix(a, tile, lane, base_count, base_sum, help, false);
  else note_helps_for_the_host(a, lane);
  if (lane == 0 && tile == a.n_tiles - 1u) {
    *a.draw_count = base_count + tile_count;
    if (a.index_total) *a.index_total = base_sum + tile_sum;
  }
  copy_out_tile<0>(a, s_cmd, lane, base_count, base_sum + first_index_base, tile_count, first_instance_base);
}

}  // namespace mip
