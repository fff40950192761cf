// cluster_cone_plan_check.cpp — renderer_amd/csrc/cluster_cone_plan.hpp on the CPU: the constants, CONE_CULLED on the
// hand-written sheet (tests/cluster_cone_cases.py) and over its decision edges — both facings, the guard's limits, scales
// that are zero, negative, subnormal and infinite, NaN and infinite eyes, NO CONE, the tie Av = 0 — and mip_cone_from_pv's
// arithmetic on a perspective matrix, its y-flip, a mirrored and an orthographic one. Stand-alone: built with
// -fsanitize=address,undefined and -ffp-contract=off by tests/test_cluster_cone_restatement.py. Prints "CLUSTER CONE PLAN OK <checks>".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <limits>

#include "../../renderer_amd/csrc/cluster_cone_plan.hpp"

static long checks = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    ++checks;                                                                \
    if (!(cond)) {                                                           \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);                  \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

using mip::ClusterConeEntry;
using mip::cone_culled;

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  static_assert(mip::kConeKMargin == 0.0078125f && mip::kConeRMargin == 0.0078125f, "the margins DESIGN section 29 derives");
  static_assert(mip::kConeGuardQuat == 1.0f / 1048576.0f && mip::kConeSpreadLimit == 0.1f, "the header's limits");
  static_assert(sizeof(ClusterConeEntry) == 32, "32 bytes per cone");
  CHECK(mip::cone_finite(0.0f) && mip::cone_finite(-3.0e38f) && !mip::cone_finite(inf) && !mip::cone_finite(-inf) && !mip::cone_finite(nan));

  // the sheet: cones of the flat clusters UP / DOWN, an instance at the origin, the eye above it
  const float r0 = std::sqrt(0.5f), r = r0 + r0 * mip::kConeRMargin;
  const ClusterConeEntry up = {{0, 0, 1}, mip::kConeKMargin, {0.5f, 0.5f, 0}, r}, down = {{0, 0, -1}, mip::kConeKMargin, {0.5f, 0.5f, 0}, r};
  const ClusterConeEntry none = {{0, 0, 0}, inf, {0, 0, 0}, 0};
  const float p[3] = {0, 0, 0}, q[4] = {0, 0, 0, 1}, eye[3] = {0.25f, 0.25f, 5.0f};
  CHECK(cone_culled(down, p, q, 1.0f, eye, 1.0f) && !cone_culled(up, p, q, 1.0f, eye, 1.0f));
  CHECK(cone_culled(up, p, q, 1.0f, eye, -1.0f) && !cone_culled(down, p, q, 1.0f, eye, -1.0f));
  CHECK(!cone_culled(none, p, q, 1.0f, eye, 1.0f) && !cone_culled(none, p, q, 1.0f, eye, -1.0f));
  // scale and position: powers of two keep the chain exact; the decision is the same one
  for (float s : {0.25f, 0.5f, 2.0f, 1024.0f}) {
    const float at[3] = {3.0f, -2.0f, 1.0f}, e2[3] = {3.0f + 0.25f * s, -2.0f + 0.25f * s, 1.0f + 5.0f * s};
    CHECK(cone_culled(down, at, q, s, e2, 1.0f) && !cone_culled(up, at, q, s, e2, 1.0f));
  }
  // the guard: s = 0, negative, NaN never cull; under a subnormal s both squares underflow to 0 and Av Av > Bv fails; an
  // infinite s makes Av or Bv infinite or NaN
  for (float s : {0.0f, -0.0f, -1.0f, nan, 1.0e-42f, inf, -inf}) CHECK(!cone_culled(down, p, q, s, eye, 1.0f) && !cone_culled(up, p, q, s, eye, -1.0f));
  // q.q at the guard's limits: w^2 = 1 +- 2^-20 passes, one float beyond fails. qq = w w exactly here.
  {
    const float lim = mip::kConeGuardQuat;
    int passed = 0, failed = 0;
    for (int k = -64; k <= 64; ++k) {
      float w = 1.0f;
      for (int j = 0; j < (k < 0 ? -k : k); ++j) w = std::nextafter(w, k < 0 ? 0.0f : 2.0f);
      const float qs[4] = {0, 0, 0, w};
      const float qq = w * w;
      const bool guard = std::fabs(qq - 1.0f) <= lim;
      CHECK(cone_culled(down, p, qs, 1.0f, eye, 1.0f) == guard);
      (guard ? passed : failed)++;
    }
    CHECK(passed > 4 && failed > 4);
  }
  for (float bad : {nan, inf, -inf}) {
    const float qs[4] = {bad, 0, 0, 1}, e3[3] = {bad, 0.25f, 5.0f}, p3[3] = {0, bad, 0};
    CHECK(!cone_culled(down, p, qs, 1.0f, eye, 1.0f));
    CHECK(!cone_culled(down, p, q, 1.0f, e3, 1.0f) && !cone_culled(up, p, q, 1.0f, e3, -1.0f));
    CHECK(!cone_culled(down, p3, q, 1.0f, eye, 1.0f));
  }
  // the tie: an eye in the cluster's plane at distance r from the centre along the axis... Av = 0 exactly is not > 0
  {
    const ClusterConeEntry flat = {{0, 0, -1}, mip::kConeKMargin, {0, 0, 0}, 1.0f};
    const float e0[3] = {0, 0, 1.0f}, e1[3] = {0, 0, std::nextafter(1.0f, 2.0f)}, e9[3] = {0, 0, 64.0f};
    CHECK(!cone_culled(flat, p, q, 1.0f, e0, 1.0f));   // d.a = 1, Av = 1 - 1 = 0
    CHECK(!cone_culled(flat, p, q, 1.0f, e1, 1.0f));   // Av = 2^-23 > 0, Av^2 = 2^-46 < Bv = 2^-14
    CHECK(cone_culled(flat, p, q, 1.0f, e9, 1.0f));    // Av = 63, Bv = 2^-14 x 4096
  }

  // mip_cone_from_pv: projection x translation(-cam): e = cam, facing = the sign of det A
  {
    const float fx = 1.3f, fy = 2.4f, cam[3] = {0.5f, 1.0f, 2.0f};
    // column-major; clip.x = fx (x - cx), clip.y = fy (y - cy), clip.z = a (z - cz) + b, clip.w = z - cz
    float pv[16] = {fx, 0, 0, 0, 0, fy, 0, 0, 0, 0, 1.001f, 1.0f, -fx * cam[0], -fy * cam[1], -1.001f * cam[2] - 0.1f, -cam[2]};
    float eye3[3], facing;
    CHECK(mip::cone_from_pv(pv, eye3, facing) && facing == 1.0f);
    for (int k = 0; k < 3; ++k) CHECK(std::fabs(eye3[k] - cam[k]) <= 1.0e-6f);
    pv[5] = -fy; pv[13] = fy * cam[1];                       // the y-flip
    CHECK(mip::cone_from_pv(pv, eye3, facing) && facing == -1.0f && std::fabs(eye3[1] - cam[1]) <= 1.0e-6f);
    pv[0] = -fx; pv[12] = fx * cam[0];                       // and mirrored in x: two flips
    CHECK(mip::cone_from_pv(pv, eye3, facing) && facing == 1.0f && std::fabs(eye3[0] - cam[0]) <= 1.0e-6f);
    const float ortho[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};   // w row = (0, 0, 0 | 1): singular
    CHECK(!mip::cone_from_pv(ortho, eye3, facing));
    float bad[16];
    for (int k = 0; k < 16; ++k) bad[k] = pv[k];
    bad[0] = nan;
    CHECK(!mip::cone_from_pv(bad, eye3, facing));
    bad[0] = inf;
    CHECK(!mip::cone_from_pv(bad, eye3, facing));
  }
  std::printf("CLUSTER CONE PLAN OK %ld\n", checks);
  return 0;
}
