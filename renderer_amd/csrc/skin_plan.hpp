// skin_plan.hpp — the integer tables the skinning kernel (skinning_kernel.hpp) walks: which lane holds which (instance,
// joint) pair, and in which order the joints of a skeleton are composed. A PURE function of the parent array, in the style of
// frame_plan.hpp / prefix_tags.hpp. No HIP, no allocation, no I/O — so every table is enumerated on a CPU, under the
// sanitizers, over every legal parent array of up to seven joints and the hierarchy families beyond
// (tests/native/skin_plan_check.cpp, built by tests/test_frame_plan.py). mip_set_skeleton (api_context.hip) copies what
// plan_skeleton returns; plan_frame and enqueue_skinned_bounds take the lane mapping from here. A wrong table is not a
// crash, it is a palette entry composed from the wrong parent.
//
// What the kernel does with them (one lane per (instance, joint) pair, floor(64 / J) instances per wave, four waves):
//   lane -> instance of the wave   g = (lane * inv_joints) >> 16                         must equal lane / J for lane < 64
//   hierarchy, depth d = 1 .. max_depth, thread t < in_block * cnt_d of the workgroup:
//     instance = (t * level_inv[d]) >> 16                                                must equal t / cnt_d for t < 256
//     word     = sorted[level_start[d] + (t - instance * cnt_d)],  joint = word & 0xff, parent = word >> 8
//     G[instance][joint] = G[instance][parent] * L[instance][joint]      — reads and writes of one level share no entry
//   because a joint's parent sits in a strictly earlier level. The kernel keeps level_start[d] | level_inv[d] << 8 in
//   one LDS word: level_start <= 32 takes the low byte, level_inv <= 2^16 the 24 bits above it.
#pragma once

#include <stdint.h>

namespace mip {

constexpr uint32_t kPlanMaxJoints = 32;   // = kMaxJoints = MIP_MAX_JOINTS (static_assert in api_context.hip)
constexpr uint32_t kPlanSkinBlock = 256;  // = kSkinBlock: four waves of 64 lanes

// ceil(2^16 / d): (x * skin_inverse(d)) >> 16 == x / d for every x < 256 and 1 <= d <= 32 (the check program sweeps it)
constexpr uint32_t skin_inverse(uint32_t d) { return (65536u + d - 1u) / d; }
// SkinArgs.inv_joints
constexpr uint32_t skin_inv_joints(uint32_t n_joints) { return skin_inverse(n_joints); }
// instances one workgroup of the skinning kernel poses: four waves of floor(64 / J) — the grid is ceil(n / this)
constexpr uint32_t skin_instances_per_block(uint32_t n_joints) { return (kPlanSkinBlock / 64u) * (64u / n_joints); }
constexpr uint32_t skin_blocks_for(uint32_t n, uint32_t n_joints) {
  return (n + skin_instances_per_block(n_joints) - 1u) / skin_instances_per_block(n_joints);
}
// entry i of the depth order: the i-th joint and its parent (a root carries parent 0 and is never looked up: depth 0 is not walked)
constexpr uint32_t skin_sorted_word(uint32_t joint, int32_t parent) { return joint | ((uint32_t)(parent < 0 ? 0 : parent) << 8); }

struct SkinPlan {
  bool ok = false;                               // false: n_joints outside 1 .. 32, or bad_joint's parent is not -1 or an earlier joint
  uint32_t bad_joint = 0;
  uint32_t n_joints = 0;
  uint32_t max_depth = 0;
  uint32_t depth[kPlanMaxJoints] = {0};          // per joint: 0 for a root
  uint32_t sorted[kPlanMaxJoints] = {0};         // JointEntry.sorted: joints in depth order (stable), skin_sorted_word
  uint8_t level_start[kPlanMaxJoints + 2] = {0}; // depth d owns sorted entries [level_start[d], level_start[d + 1]); n_joints past max_depth
  uint32_t level_inv[kPlanMaxJoints + 1] = {0};  // skin_inverse(joints at depth d); 0 past max_depth
};

inline SkinPlan plan_skeleton(const int32_t* parent, uint32_t n_joints) {
  SkinPlan p;
  if (n_joints == 0 || n_joints > kPlanMaxJoints) return p;
  p.n_joints = n_joints;
  for (uint32_t k = 0; k < n_joints; ++k) {
    if (parent[k] >= (int32_t)k || parent[k] < -1) {
      p.bad_joint = k;
      return p;
    }
    p.depth[k] = parent[k] < 0 ? 0u : p.depth[parent[k]] + 1u;
    if (p.depth[k] > p.max_depth) p.max_depth = p.depth[k];
  }
  // joints in depth order (stable): level d owns sorted entries [level_start[d], level_start[d+1])
  uint32_t at = 0;
  for (uint32_t d = 0; d <= p.max_depth; ++d) {
    p.level_start[d] = (uint8_t)at;
    for (uint32_t k = 0; k < n_joints; ++k)
      if (p.depth[k] == d) p.sorted[at++] = skin_sorted_word(k, parent[k]);
    p.level_inv[d] = skin_inverse(at - p.level_start[d]);
  }
  for (uint32_t d = p.max_depth + 1; d < kPlanMaxJoints + 2; ++d) p.level_start[d] = (uint8_t)at;
  p.ok = true;
  return p;
}

}  // namespace mip
