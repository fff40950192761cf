// cluster_cone_plan.hpp — the arithmetic of the normal-cone back-face test of cluster culling (mip_build_cluster_cones,
// mip_cull_clusters_cone, mip_cull_cluster_triangles_cone; extension, not reference behaviour) that is not a kernel: the margin
// that widens a cone, the limits of NO CONE and of the instance GUARD, the per-item decision CONE_CULLED as one literal float
// chain, and the view's side of the test (mip_cone_from_pv: the eye and the facing of a projection, in double). Plain C++, no
// HIP, host + device: api_cluster.hip and cluster_cone_kernel.hpp call it, tests/native/cluster_cone_plan_check.cpp runs it on
// the CPU over its decision edges. include/mi_instance_pipeline.h states every chain of this file in words; DESIGN section 29
// derives the margin. Compile with contraction off: every written operation is one rounding.
#pragma once

#include <cmath>
#include <cstdint>

#include "cluster_plan.hpp"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace mip {

// THE MARGIN. k = sqrtf(1 - m m) + kConeKMargin: absolute, because the error of sin(theta) taken from a
// cosine is sqrt(2 x the cosine's error) near theta = 0 — 2^-7.75 inside the domain — and k <= 1 + 2^-7 makes a relative
// part on top of it pointless. r = r0 + r0 kConeRMargin: relative, it absorbs the rounding of every position of the chain
// (absolute errors of 2^-19 x the largest world coordinate) while that coordinate is at most 2^12 cluster radii.
constexpr float kConeKMargin = 0x1p-7f;
constexpr float kConeRMargin = 0x1p-7f;
constexpr float kConeSpreadLimit = 0.1f;   // m <= this: the normals spread over more than ~84 degrees, NO CONE
constexpr float kConeGuardQuat = 0x1p-20f; // | q.q - 1 | above this: the instance is never cone-culled

// The finite floats: x - x is +0 for them and NaN for +-inf and NaN (no <cmath> classification call on the device).
MIP_CLUSTER_HD inline bool cone_finite(float x) { return x - x == 0.0f; }

// One cone of the table as the two 16-byte words the kernels load.
struct ClusterConeEntry {
  float axis[3], k;     // unit axis, sin(theta) widened; k = +inf: NO CONE (axis, centre and r are zero then)
  float centre[3], r;   // the box's centre and half diagonal, widened
};

// CONE_CULLED(i, c), the header's chain operation by operation. p, q = {i, j, k, w}, s: the instance's columns.
MIP_CLUSTER_HD inline bool cone_culled(const ClusterConeEntry& cone, const float (&p)[3], const float (&q)[4], float s,
                                       const float (&eye)[3], float facing) {
  const float qq = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3];
  const bool guard = s > 0.0f && fabsf(qq - 1.0f) <= kConeGuardQuat;
  // the rotation of nalgebra's UnitQuaternion::to_rotation_matrix (quat_to_rotation, instance_kernel.hpp), rot[row][col]
  const float i = q[0], j = q[1], k = q[2], w = q[3];
  const float ww = w * w, ii = i * i, jj = j * j, kk = k * k;
  const float ij = i * j * 2.0f, wk = w * k * 2.0f, wj = w * j * 2.0f;
  const float ik = i * k * 2.0f, jk = j * k * 2.0f, wi = w * i * 2.0f;
  const float rot[3][3] = {{ww + ii - jj - kk, ij - wk, wj + ik}, {wk + ij, ww - ii + jj - kk, jk - wi}, {ik - wj, wi + jk, ww - ii - jj + kk}};
  float cw[3], aw[3], d[3];
  for (int r = 0; r < 3; ++r) {
    const float m0 = rot[r][0] * s, m1 = rot[r][1] * s, m2 = rot[r][2] * s;   // the model matrix mip_run writes (model_fast)
    cw[r] = ((m0 * cone.centre[0] + m1 * cone.centre[1]) + m2 * cone.centre[2]) + p[r];
    aw[r] = (m0 * cone.axis[0] + m1 * cone.axis[1]) + m2 * cone.axis[2];
    d[r] = cw[r] - eye[r];
  }
  const float da = (d[0] * aw[0] + d[1] * aw[1]) + d[2] * aw[2];
  const float dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
  const float av = facing * da - (s * s) * cone.r;
  const float sk = s * cone.k;
  const float bv = (sk * sk) * dd;
  return guard && av > 0.0f && av * av > bv && cone_finite(av) && cone_finite(bv);
}

// mip_cone_from_pv: rows x, y, w of pv (column-major) are [A | b]; clip = A (x - e), e = -A^-1 b; facing = sign(det A). In
// double, rounded once. false: A is singular or not finite, or e is not a finite float (an orthographic pv has no eye).
inline bool cone_from_pv(const float (&pv)[16], float (&eye)[3], float& facing) {
  const int rows[3] = {0, 1, 3};
  double a[3][3], b[3];
  for (int q = 0; q < 3; ++q) {
    for (int c = 0; c < 3; ++c) a[q][c] = (double)pv[c * 4 + rows[q]];
    b[q] = (double)pv[3 * 4 + rows[q]];
  }
  // the adjugate's rows are the cross products of A's rows
  const double c0[3] = {a[1][1] * a[2][2] - a[1][2] * a[2][1], a[1][2] * a[2][0] - a[1][0] * a[2][2], a[1][0] * a[2][1] - a[1][1] * a[2][0]};
  const double c1[3] = {a[2][1] * a[0][2] - a[2][2] * a[0][1], a[2][2] * a[0][0] - a[2][0] * a[0][2], a[2][0] * a[0][1] - a[2][1] * a[0][0]};
  const double c2[3] = {a[0][1] * a[1][2] - a[0][2] * a[1][1], a[0][2] * a[1][0] - a[0][0] * a[1][2], a[0][0] * a[1][1] - a[0][1] * a[1][0]};
  const double det = a[0][0] * c0[0] + a[0][1] * c0[1] + a[0][2] * c0[2];
  if (!(det - det == 0.0) || det == 0.0) return false;
  for (int r = 0; r < 3; ++r) {
    const double e = -(c0[r] * b[0] + c1[r] * b[1] + c2[r] * b[2]) / det;   // (A^-1)[r][q] = cofactor[q][r] / det
    const float f = (float)e;
    if (!cone_finite(f)) return false;
    eye[r] = f;
  }
  facing = det > 0.0 ? 1.0f : -1.0f;
  return true;
}

}  // namespace mip
