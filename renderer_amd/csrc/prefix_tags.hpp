// prefix_tags.hpp — WHICH tag a launch on a cross-tile prefix state gets, and which of the state's two accumulator buffers
// must be zero before it: a PURE value type, in the style of frame_plan.hpp. No HIP, no allocation, no I/O — so the rule is
// enumerated on a CPU, under the sanitizers, against a model of the device side (tests/native/prefix_tags_check.cpp, built
// by tests/test_frame_plan.py). run_frame, run_views_chunk and run_many_graphed (api_frame.hip) call it and hold no tag
// arithmetic of their own.
//
// The device side (instance_kernel.hpp): a launch with tag t marks every level-0 word and group start it writes with t, and
// it rewrites every one of them that a later launch reads — so the only stale tag a word can hold is the PREVIOUS launch's.
// It adds its tiles into accumulator buffer t & 1, which must be all-zero when it starts, and zeroes the other buffer for
// the launch after it. Hence the two rules of this file: consecutive launches never share a tag, and a launch's tag has the
// parity of the buffer that is zero now. A wrong tag is not a crash, it is wrong command bytes.
//
// Recorded chains (mip_run_many): a chain bakes the G tags base + 1 .. base + G, G even, into its graph. Replaying the same
// tags — also after direct launches ran in between — is sound because
//  - the words then hold the tag of the last launch, which is the chain's own base + G (G >= 2, so not base + 1) or a
//    later launch's tag, handed out after the chain first ran (a recording is replayed at once) and so above base + G;
//  - the buffer the chain's first launch adds into, (base + 1) & 1, is zero: it is the one the chain's last launch zeroed
//    (G is even) when the chain ran last, and when another launch ran last the host zeroes it in front of the replay
//    (chain_needs_zero);
//  - clearing the state (the tag wrap, a new instance count) discards every recorded chain with it (graph_generation).
#pragma once

#include <stdint.h>

#include "frame_plan.hpp"

namespace mip {

// = kMaxEpoch, the largest tag a level-0 word holds beside a tile's count (instance_kernel.hpp; static_assert in context.hpp)
constexpr uint32_t kPlanMaxEpoch = (1u << (32u - (kPlanTile <= 256u ? 9u : (kPlanTile <= 512u ? 10u : 11u)))) - 1u;

struct PrefixTags {
  uint32_t epoch = 0;         // highest tag handed out on this state
  uint32_t last_tag = 0;      // tag of the last launch (what the level-0 words hold now)
  uint32_t zero_buf = 2;      // which accumulator buffer is all-zero now: 0, 1, or 2 = both
  bool status_dirty = false;  // instance count changed: clear the prefix state before the next launch

  // The state must be cleared (device memory zeroed, `cleared()`, recorded chains dropped) before `need` more tags are
  // taken from it: one launch needs 2 (its tag may skip one for parity), a chain of G needs G + 2.
  bool needs_clear(uint32_t need) const { return status_dirty || epoch + need > kPlanMaxEpoch; }
  void cleared() { *this = PrefixTags(); }

  // The tag of one direct launch: the next one, or the one after it when that is what accumulates in the zeroed buffer.
  uint32_t next_tag() {
    uint32_t e = epoch + 1;
    if (zero_buf != 2 && (e & 1u) != zero_buf) ++e;
    epoch = last_tag = e;
    zero_buf = (e & 1u) ^ 1u;
    return e;
  }

  // A chain recorded now bakes the tags chain_base() + 1 .. chain_base() + G (G even). Recording launches nothing and
  // takes nothing from the state: the tags count as handed out once the chain has been replayed.
  uint32_t chain_base() const {
    uint32_t base = epoch > last_tag ? epoch : last_tag;
    if (zero_buf != 2 && ((base + 1) & 1u) != zero_buf) ++base;
    return base;
  }
  static uint32_t chain_tag(uint32_t base, uint32_t j) { return base + 1 + j; }  // of the chain's launch j = 0 .. G - 1
  static uint32_t chain_first_buf(uint32_t base) { return chain_tag(base, 0) & 1u; }
  // A chain whose first tag is the one the words hold now would read them as its own (cannot happen: see above).
  bool chain_replayable(uint32_t base) const { return last_tag != base + 1; }
  // Other launches ran since the chain did: the host zeroes accumulator buffer chain_first_buf(base) in front of the replay.
  bool chain_needs_zero(uint32_t base) const { return zero_buf != 2 && zero_buf != chain_first_buf(base); }
  void chain_replayed(uint32_t base, uint32_t G) {
    last_tag = base + G;
    if (epoch < last_tag) epoch = last_tag;
    zero_buf = chain_first_buf(base);  // G is even: the last launch zeroed the buffer the first one uses
  }
};

}  // namespace mip
