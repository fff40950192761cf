// cluster_cone_kernel.hpp — the normal-cone back-face test of cluster culling (mip_build_cluster_cones, mip_cull_clusters_cone,
// mip_cull_cluster_triangles_cone; extension, not reference behaviour), gfx950. include/mi_instance_pipeline.h specifies it,
// tests/cluster_cone_restatement.py restates it in numpy, cluster_cone_plan.hpp holds the decision and the margin.
// Instantiated in api_cluster.hip only.
//
//   cone build   one wave per cluster, lane t = triangle t, the shape of mip_cluster_build_kernel: the unit normal of the lane's
//                triangle, three butterfly sums for the axis (level j adds the lanes that differ in bit j: float addition is
//                commutative, so every lane holds the same bits), a butterfly minimum of the normals' cosines against the
//                axis, the sphere from the cluster's box; lane 0 stores the 32 bytes
//   cone cull    mip_cluster_cull_kernel with CONE_CULLED in front: two 16-byte loads and cone_culled (cluster_cone_plan.hpp)
//                beside the instance columns the box chain loads anyway. Wave-uniform: a wave none of whose items is left
//                stores its zero survive word and its start word and runs neither instance_tiered nor the planes nor
//                box_occluded. The lines behind the cone are cull's own, copied: the kernels mip_cull_clusters launches
//                keep their instructions (DESIGN sections 27 and 29)
//
// Every other launch of the two cone calls is the kernel the plain calls launch.
#pragma once

#include "cluster_cone_plan.hpp"
#include "cluster_kernel.hpp"

#pragma clang fp contract(off)

namespace mip {

struct ClusterConeBuildArgs {
  ClusterBuildArgs b;   // the geometry, the tables, the boxes (read here), the total
  float4* cones;        // two per cluster: {axis xyz, k}, {centre xyz, r}
};

struct ClusterConeArgs {
  ClusterArgs c;        // mip_cull_clusters' block, untouched
  const float4* cones;
  float eye[3];
  float facing;
};

__device__ __forceinline__ float cluster_wave_sum_butterfly(float v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v = v + __shfl_xor(v, m);
  return v;
}

static __global__ __launch_bounds__(kClusterThreads) __attribute__((unused)) void mip_cluster_cone_build_kernel(const ClusterConeBuildArgs ca) {
  const ClusterBuildArgs& a = ca.b;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t g = blockIdx.x * kWaves + wave;
  if (g >= a.total) return;  // (the whole wave)
  const uint32_t b = cluster_bucket_of(a.cluster_base, a.n_buckets, g);
  const uint32_t ml = a.bucket_lod[b];
  const uint32_t mesh = ml >> 3, lod = ml & 7u;
  const MeshChain& ch = a.chain[mesh];
  const uint32_t tris = cluster_level_triangles(ch.index_len[lod]);
  const uint32_t t = (g - a.cluster_base[b]) * kClusterTriangles + lane;
  const bool present = t < tris;
  const float inf = __builtin_inff();
  float nh[3] = {0.0f, 0.0f, 0.0f};
  bool proper = true;  // (a lane without a triangle spoils nothing)
  if (present) {  // the host checked every index of the level and every vertex behind it (mip_build_clusters)
    const uint32_t* ix = a.indices + (size_t)ch.index_offset[lod] + 3u * (size_t)t;
    const size_t vo = (size_t)a.mesh_draw[mesh].vertex_offset;
    const float* v0 = a.vertices + 3u * (vo + ix[0]);
    const float* v1 = a.vertices + 3u * (vo + ix[1]);
    const float* v2 = a.vertices + 3u * (vo + ix[2]);
    const float e1[3] = {v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]};
    const float e2[3] = {v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]};
    const float n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const float len2 = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
    proper = len2 > 0.0f && len2 < inf;  // (a NaN fails both)
    if (proper) {
      const float len = sqrtf(len2);
      nh[0] = n[0] / len; nh[1] = n[1] / len; nh[2] = n[2] / len;
    }
  }
  const float ax = cluster_wave_sum_butterfly(nh[0]), ay = cluster_wave_sum_butterfly(nh[1]), az = cluster_wave_sum_butterfly(nh[2]);
  const float aa = (ax * ax + ay * ay) + az * az;
  const bool axis_ok = aa > 0.0f && aa < inf;
  const float al = sqrtf(aa);
  const float axis[3] = {ax / al, ay / al, az / al};
  const float cosine = present ? (nh[0] * axis[0] + nh[1] * axis[1]) + nh[2] * axis[2] : inf;
  const float m = cluster_wave_min(cosine);
  const bool cone = __all(proper) && axis_ok && m > kConeSpreadLimit;
  if (lane == 0u) {
    float4 o0 = make_float4(0.0f, 0.0f, 0.0f, inf), o1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (cone) {
      const float4 lo = a.boxes[2u * (size_t)g], hi = a.boxes[2u * (size_t)g + 1u];
      const float hx = (hi.x - lo.x) / 2.0f, hy = (hi.y - lo.y) / 2.0f, hz = (hi.z - lo.z) / 2.0f;
      const float r0 = sqrtf((hx * hx + hy * hy) + hz * hz);
      const float k0 = sqrtf(fmaxf(1.0f - m * m, 0.0f));
      o0 = make_float4(axis[0], axis[1], axis[2], k0 + kConeKMargin);
      o1 = make_float4((hi.x + lo.x) / 2.0f, (hi.y + lo.y) / 2.0f, (hi.z + lo.z) / 2.0f, r0 + r0 * kConeRMargin);
    }
    ca.cones[2u * (size_t)g] = o0;
    ca.cones[2u * (size_t)g + 1u] = o1;
  }
}

// cone cull: CONE_CULLED, then — for a wave that has an item left — both tests of mip_cluster_cull_kernel<false> on the items
// the cone left; the survive word and the start word of every 64.
static __global__ __launch_bounds__(kClusterThreads, 4) __attribute__((unused)) void mip_cluster_cone_cull_kernel(const ClusterConeArgs ca) {
  const ClusterArgs& a = ca.c;
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
      const float4 c0 = ca.cones[2u * g], c1 = ca.cones[2u * g + 1u];
      const ClusterConeEntry cone = {{c0.x, c0.y, c0.z}, c0.w, {c1.x, c1.y, c1.z}, c1.w};
      const float p[3] = {px, py, pz}, quat[4] = {q.x, q.y, q.z, q.w};
      const bool alive = active && !cone_culled(cone, p, quat, sc, ca.eye, ca.facing);
      const unsigned long long start = __ballot(active && it.cluster == 0u);
      if (__ballot(alive) == 0ull) {  // (the whole wave) nothing left for the box chain: no matrix, no planes, no pyramid
        if (lane == 0u) a.words[base >> 6] = make_ulonglong2(0ull, start);
        continue;
      }
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
      bool survives = alive && !coarse_culled(inst, a.planes);
      if (survives && a.pyramid) survives = !box_occluded(inst.mins, inst.maxs, a.pv, a.pyramid, a.width, a.height);
      const unsigned long long s = __ballot(survives);
      if (lane == 0u) a.words[base >> 6] = make_ulonglong2(s, start);
    }
  }
}

}  // namespace mip
