// skin_plan_check.cpp — runs plan_skeleton (renderer_amd/csrc/skin_plan.hpp) over every legal parent array of up to seven
// joints (1! + 2! + ... + 7! = 5 913) and, for 8 .. 32 joints, over the hierarchy families the GPU tests use (chain, star,
// forest, comb) plus seeded random arrays of three flavours, and checks what skinning_kernel.hpp relies on: the depth order,
// the packed words, the two multiply-shift divisions, and — by replaying the kernel's level walk with integer labels in the
// place of matrices — that every (instance, joint) pair of a workgroup is composed exactly once, from its finished parent.
// Plain C++, no HIP: built by tests/test_frame_plan.py with gcc -fsanitize=address,undefined.
// Prints "SKIN OK <skeletons> <enumerated>".
#include "../../renderer_amd/csrc/skin_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace mip;

#define CHECK(cond, ...)                                                        \
  do {                                                                          \
    if (!(cond)) {                                                              \
      std::printf("FAILED %s:%d %s — ", __FILE__, __LINE__, #cond);             \
      std::printf(__VA_ARGS__);                                                 \
      std::printf("\n");                                                        \
      std::exit(1);                                                             \
    }                                                                           \
  } while (0)

static unsigned long long skeletons = 0, enumerated = 0, walks = 0;

// G = parent's G composed with the joint's own label: not commutative, not associative — a product taken with the wrong
// parent, twice, or before the parent's own product gives another number.
static uint64_t compose(uint64_t parent_g, uint64_t local) { return parent_g * 0x9E3779B97F4A7C15ull + local + 1ull; }
static uint64_t local_label(uint32_t inst, uint32_t joint) { return ((uint64_t)inst << 8) | joint; }

// The kernel's hierarchy phase for one workgroup of `in_block` instances: kPlanSkinBlock threads, one barrier per level, the
// tables read exactly as skinning_kernel.hpp reads them (s_level[d] = level_start[d] | level_inv[d] << 8).
static void replay_walk(const SkinPlan& p, const int32_t* parent, uint32_t in_block) {
  const uint32_t J = p.n_joints;
  std::vector<uint32_t> s_level(kPlanMaxJoints + 2);
  for (uint32_t d = 0; d < kPlanMaxJoints + 2; ++d)
    s_level[d] = (uint32_t)p.level_start[d] | ((d <= kPlanMaxJoints ? p.level_inv[d] : 0u) << 8);
  std::vector<uint32_t> s_sorted(p.sorted, p.sorted + J);   // exactly J words: a look-up past them is an ASan report
  std::vector<uint64_t> s_g((size_t)in_block * J);          // exactly the pairs of this workgroup
  std::vector<uint32_t> written((size_t)in_block * J, 0u);
  for (uint32_t i = 0; i < in_block; ++i)
    for (uint32_t k = 0; k < J; ++k) s_g[(size_t)i * J + k] = local_label(i, k);
  struct Store { size_t at; uint64_t value; };
  std::vector<Store> stores;
  for (uint32_t d = 1; d <= p.max_depth; ++d) {
    const uint32_t lv = s_level.at(d);
    const uint32_t start = lv & 0xffu, cnt = (s_level.at(d + 1) & 0xffu) - start, inv = lv >> 8;
    stores.clear();
    for (uint32_t tid = 0; tid < kPlanSkinBlock; ++tid) {  // every thread reads, then every thread writes: no order inside a level
      if (tid < in_block * cnt) {
        const uint32_t inst_l = (tid * inv) >> 16;
        const uint32_t packed = s_sorted.at(start + (tid - inst_l * cnt));
        const uint32_t k = packed & 0xffu, pk = packed >> 8;
        stores.push_back({(size_t)inst_l * J + k, compose(s_g.at((size_t)inst_l * J + pk), s_g.at((size_t)inst_l * J + k))});
      }
    }
    for (const Store& s : stores) {
      s_g.at(s.at) = s.value;
      ++written.at(s.at);
    }
  }
  // the plain recursion in parent order (the oracle's loop)
  std::vector<uint64_t> g(J);
  for (uint32_t i = 0; i < in_block; ++i)
    for (uint32_t k = 0; k < J; ++k) {
      g[k] = parent[k] < 0 ? local_label(i, k) : compose(g[parent[k]], local_label(i, k));
      CHECK(s_g[(size_t)i * J + k] == g[k], "J %u, %u instances: instance %u joint %u differs from the recursion", J, in_block, i, k);
      CHECK(written[(size_t)i * J + k] == (parent[k] < 0 ? 0u : 1u), "J %u: instance %u joint %u written %u times", J, i, k, written[(size_t)i * J + k]);
    }
  ++walks;
}

static void check_skeleton(const int32_t* parent, uint32_t J) {
  ++skeletons;
  const SkinPlan p = plan_skeleton(parent, J);
  CHECK(p.ok && p.n_joints == J, "a legal skeleton of %u joints was refused at joint %u", J, p.bad_joint);
  // sorted is a permutation of the joints, every word round-trips, and a joint's parent sits in a strictly earlier level
  uint32_t seen = 0, level_of[kPlanMaxJoints];
  for (uint32_t d = 0; d <= p.max_depth; ++d) {
    CHECK(p.level_start[d] < p.level_start[d + 1], "J %u: depth %u is empty", J, d);
    for (uint32_t i = p.level_start[d]; i < p.level_start[d + 1]; ++i) {
      const uint32_t k = p.sorted[i] & 0xffu;
      CHECK(k < J && !(seen >> k & 1u), "J %u: sorted[%u] = joint %u, out of range or twice", J, i, k);
      seen |= 1u << k;
      level_of[k] = d;
      CHECK(p.depth[k] == d, "J %u: joint %u of depth %u sorted into level %u", J, k, p.depth[k], d);
    }
  }
  CHECK(seen == (J == 32u ? 0xffffffffu : (1u << J) - 1u), "J %u: sorted misses a joint (%08x)", J, seen);
  for (uint32_t i = 0; i < J; ++i) {
    const uint32_t k = p.sorted[i] & 0xffu, pk = p.sorted[i] >> 8;
    CHECK(pk == (uint32_t)(parent[k] < 0 ? 0 : parent[k]), "J %u: sorted[%u] carries parent %u of joint %u, not %d", J, i, pk, k, parent[k]);
    CHECK(p.sorted[i] == skin_sorted_word(k, parent[k]), "J %u: sorted[%u] does not round-trip", J, i);
    if (parent[k] >= 0) CHECK(level_of[parent[k]] + 1u == level_of[k], "J %u: joint %u in level %u, its parent in %u", J, k, level_of[k], level_of[parent[k]]);
    else CHECK(level_of[k] == 0u, "J %u: root %u in level %u", J, k, level_of[k]);
    if (i) CHECK(level_of[p.sorted[i - 1] & 0xffu] < level_of[k] || (p.sorted[i - 1] & 0xffu) < k, "J %u: the depth order is not stable at %u", J, i);
  }
  // level_start is monotone, starts at 0 and ends at J; level_inv divides every thread index by the level's joint count
  CHECK(p.level_start[0] == 0u && p.max_depth < J, "J %u: level_start[0] %u, max_depth %u", J, p.level_start[0], p.max_depth);
  for (uint32_t d = 0; d < kPlanMaxJoints + 1; ++d) {
    CHECK(p.level_start[d] <= p.level_start[d + 1] && p.level_start[d + 1] <= J, "J %u: level_start not monotone at %u", J, d);
    if (d > p.max_depth) CHECK(p.level_start[d] == J && p.level_inv[d] == 0u, "J %u: level %u past the deepest is not empty", J, d);
  }
  CHECK(p.level_start[kPlanMaxJoints + 1] == J, "J %u: level_start ends at %u", J, p.level_start[kPlanMaxJoints + 1]);
  for (uint32_t d = 0; d <= p.max_depth; ++d) {
    const uint32_t cnt = (uint32_t)p.level_start[d + 1] - p.level_start[d];
    const uint32_t word = (uint32_t)p.level_start[d] | (p.level_inv[d] << 8);  // the LDS word of the kernel
    CHECK((word & 0xffu) == p.level_start[d] && (word >> 8) == p.level_inv[d] && p.level_inv[d] <= 65536u, "J %u: level word %u does not round-trip", J, d);
    for (uint32_t x = 0; x < kPlanSkinBlock; ++x)
      CHECK(((x * p.level_inv[d]) >> 16) == x / cnt, "J %u depth %u: %u / %u by multiply-shift gives %u", J, d, x, cnt, (x * p.level_inv[d]) >> 16);
  }
  // lane mapping
  const uint32_t ipw = 64u / J, ipb = skin_instances_per_block(J);
  CHECK(ipb == 4u * ipw && ipb * J <= kPlanSkinBlock, "J %u: %u instances per workgroup", J, ipb);
  for (uint32_t lane = 0; lane < 64u; ++lane)
    CHECK(((lane * skin_inv_joints(J)) >> 16) == lane / J, "J %u: lane %u / J by multiply-shift", J, lane);
  for (uint32_t n : {1u, ipb - 1u, ipb, ipb + 1u, 2u * ipb + ipw + 1u, 1000003u})
    if (n) CHECK((unsigned long long)skin_blocks_for(n, J) * ipb >= n && (unsigned long long)(skin_blocks_for(n, J) - 1u) * ipb < n, "J %u: %u workgroups for %u instances", J, skin_blocks_for(n, J), n);
  // the level walk, for a full workgroup, a single instance, and a last wave that is partly full
  replay_walk(p, parent, ipb);
  replay_walk(p, parent, 1u);
  replay_walk(p, parent, ipw > 1u ? ipb - ipw + 1u : ipb - 1u);
}

static void enumerate(int32_t* parent, uint32_t k, uint32_t J) {
  if (k == J) {
    ++enumerated;
    check_skeleton(parent, J);
    return;
  }
  for (int32_t pk = -1; pk < (int32_t)k; ++pk) {
    parent[k] = pk;
    enumerate(parent, k + 1u, J);
  }
}

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint32_t rnd(uint32_t below) {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint32_t)(((rng_state * 0x2545F4914F6CDD1Dull) >> 33) % below);
}

int main() {
  int32_t parent[kPlanMaxJoints];
  for (uint32_t J = 1; J <= 7u; ++J) enumerate(parent, 0u, J);
  CHECK(enumerated == 5913ull, "%llu parent arrays of up to seven joints", enumerated);
  for (uint32_t J = 8; J <= kPlanMaxJoints; ++J) {
    for (uint32_t k = 0; k < J; ++k) parent[k] = (int32_t)k - 1;  // chain
    check_skeleton(parent, J);
    for (uint32_t k = 0; k < J; ++k) parent[k] = k ? 0 : -1;      // star
    check_skeleton(parent, J);
    for (uint32_t k = 0; k < J; ++k) parent[k] = -1;              // forest
    check_skeleton(parent, J);
    for (uint32_t k = 0; k < J; ++k) parent[k] = k >= 2u ? (int32_t)k - 2 : -1;  // comb: two interleaved chains
    check_skeleton(parent, J);
    for (uint32_t rep = 0; rep < 160u; ++rep) {
      const uint32_t flavour = rep % 3u;  // uniform over -1 .. k-1 | deep: one of the last three joints | bushy, a new root now and then
      parent[0] = -1;
      for (uint32_t k = 1; k < J; ++k) {
        if (flavour == 0u) parent[k] = (int32_t)rnd(k + 1u) - 1;
        else if (flavour == 1u) parent[k] = (int32_t)(k - 1u - rnd(k < 3u ? k : 3u));
        else parent[k] = k % 5u == 4u ? (int32_t)rnd(k + 1u) - 1 : (int32_t)rnd(k);
      }
      check_skeleton(parent, J);
    }
  }
  // refusals: a parent that does not precede its child, and joint counts outside 1 .. 32
  for (uint32_t J = 1; J <= kPlanMaxJoints; ++J)
    for (uint32_t bad = 0; bad < J; ++bad)
      for (int32_t value : {(int32_t)bad, (int32_t)bad + 1, -2, 255}) {
        for (uint32_t k = 0; k < J; ++k) parent[k] = (int32_t)k - 1;
        parent[bad] = value;
        const SkinPlan p = plan_skeleton(parent, J);
        CHECK(!p.ok && p.bad_joint == bad, "J %u: parent[%u] = %d accepted", J, bad, value);
      }
  CHECK(!plan_skeleton(parent, 0u).ok && !plan_skeleton(parent, kPlanMaxJoints + 1u).ok, "joint count outside 1 .. 32 accepted");
  std::printf("walks %llu\n", walks);
  std::printf("SKIN OK %llu %llu\n", skeletons, enumerated);
  return 0;
}
