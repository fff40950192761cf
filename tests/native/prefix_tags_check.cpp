// prefix_tags_check.cpp — drives PrefixTags (renderer_amd/csrc/prefix_tags.hpp) through call sequences the way api_frame.hip
// does (direct launches, recorded chains and their replays, clears forced by a new instance count or by the tag wrap) against
// a model of the device side, and checks what the kernels rely on. Plain C++, no HIP: built by tests/test_frame_plan.py with
// gcc -fsanitize=address,undefined. Prints "TAGS OK <sequences> <launches>".
//
// The model (instance_kernel.hpp): the level-0 words hold the tag of the launch that wrote them last; a launch with tag t
// adds into accumulator buffer t & 1, which must be all-zero, and zeroes the other one.
#include "../../renderer_amd/csrc/prefix_tags.hpp"

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

static unsigned long long sequences = 0, launches = 0, clears = 0, bumps = 0, zeroings = 0;

struct Device {
  bool zero[2] = {true, true};
  uint32_t words_tag = 0;
  void clear() { zero[0] = zero[1] = true; words_tag = 0; }
  void launch(uint32_t t) {
    ++launches;
    CHECK(t != 0u && t <= kPlanMaxEpoch, "tag %u outside 1 .. %u", t, kPlanMaxEpoch);
    CHECK(t != words_tag, "tag %u is the one the words hold already: stale words would read as this launch's", t);
    CHECK(zero[t & 1u], "the launch with tag %u adds into accumulator buffer %u, which is not zero", t, t & 1u);
    zero[t & 1u] = false;
    zero[(t & 1u) ^ 1u] = true;
    words_tag = t;
  }
};

// What api_frame.hip keeps around one PrefixTags: the device state it stands for, the generation that invalidates recorded
// chains, and the chains themselves (run_many_graphed: a small LRU, looked up by length here).
struct Host {
  PrefixTags tags;
  Device dev;
  unsigned long long generation = 1;
  uint32_t high = 0;  // highest tag handed out since the last clear
  struct Chain { uint32_t G, base; unsigned long long generation; };
  std::vector<Chain> chains;

  explicit Host(uint32_t epoch_start) { tags.epoch = high = epoch_start; }  // MIP_TEST_EPOCH_START

  void invariants(const char* after) const {
    CHECK(tags.last_tag == dev.words_tag, "after %s: last_tag %u, the words hold %u", after, tags.last_tag, dev.words_tag);
    CHECK(tags.epoch == high && tags.last_tag <= tags.epoch, "after %s: epoch %u, highest tag handed out %u, last %u", after, tags.epoch, high, tags.last_tag);
    if (tags.zero_buf == 2u) CHECK(dev.zero[0] && dev.zero[1], "after %s: zero_buf says both, the model disagrees", after);
    else CHECK(tags.zero_buf < 2u && dev.zero[tags.zero_buf], "after %s: zero_buf %u is not zero in the model", after, tags.zero_buf);
  }
  void clear_if_needed(uint32_t need) {  // clear_prefix_state_if_needed
    if (!tags.needs_clear(need)) {
      CHECK((unsigned long long)high + need <= kPlanMaxEpoch, "no clear, but %u more tags after %u run past the largest tag", need, high);
      return;
    }
    CHECK(tags.status_dirty || (unsigned long long)high + need > kPlanMaxEpoch, "a clear that nothing asked for: %u tags after %u", need, high);
    ++clears;
    dev.clear();
    tags.cleared();
    ++generation;
    high = 0;
    CHECK(tags.epoch == 0u && tags.last_tag == 0u && tags.zero_buf == 2u && !tags.status_dirty, "a cleared state is a new state");
    CHECK(!tags.needs_clear(need), "a cleared state has %u tags", need);
  }
  void direct() {  // run_frame, one view of run_views_chunk
    clear_if_needed(2);
    const uint32_t t = tags.next_tag();
    CHECK(t > high, "tags strictly increase between clears: %u after %u", t, high);
    bumps += t - high - 1u;
    high = t;
    dev.launch(t);
    invariants("a direct launch");
  }
  void chain(uint32_t G, uint32_t rounds) {  // run_many_graphed
    clear_if_needed(G + 2);
    for (size_t i = 0; i < chains.size();)
      if (chains[i].generation != generation) chains.erase(chains.begin() + (long)i);
      else ++i;
    const Chain* c = nullptr;
    for (const Chain& k : chains)
      if (k.G == G) c = &k;
    if (c) CHECK(tags.chain_replayable(c->base), "a recorded chain is replayable until the state is cleared (base %u, last tag %u)", c->base, tags.last_tag);
    if (!c) {
      if (chains.size() >= 4) chains.erase(chains.begin());
      const uint32_t base = tags.chain_base();
      CHECK(PrefixTags::chain_tag(base, 0) > high, "a new chain's tags are fresh: first %u, highest handed out %u", base + 1u, high);
      CHECK(PrefixTags::chain_tag(base, G - 1u) <= kPlanMaxEpoch, "a chain of %u from %u runs past the largest tag", G, base);
      high = PrefixTags::chain_tag(base, G - 1u);
      chains.push_back({G, base, generation});
      c = &chains.back();
    }
    for (uint32_t r = 0; r < rounds; ++r) {
      const uint32_t epoch_before = tags.epoch;
      if (tags.chain_needs_zero(c->base)) {  // the host's memset in front of the replay
        ++zeroings;
        dev.zero[PrefixTags::chain_first_buf(c->base)] = true;
      }
      for (uint32_t j = 0; j < G; ++j) dev.launch(PrefixTags::chain_tag(c->base, j));
      tags.chain_replayed(c->base, G);
      invariants("a replay");
      // ... and as a re-recording would find them: what G direct launches with these tags leave behind
      CHECK(tags.last_tag == c->base + G && tags.zero_buf == (((c->base + G) & 1u) ^ 1u), "a replay ends like its last launch");
      CHECK(tags.epoch == (epoch_before > c->base + G ? epoch_before : c->base + G), "a replay never lowers the highest tag");
      const uint32_t again = tags.chain_base();
      CHECK(again >= tags.epoch && !tags.chain_needs_zero(again) && tags.chain_replayable(again), "a chain recorded behind a replay starts fresh and in the zeroed buffer");
    }
  }
};

// every sequence of `depth` operations out of: direct launch | new instance count | chain of Ga | chain of Gb | chain of Ga, two rounds
static void enumerate(uint32_t start, uint32_t Ga, uint32_t Gb, uint32_t depth) {
  unsigned long long total = 1;
  for (uint32_t d = 0; d < depth; ++d) total *= 5u;
  for (unsigned long long code = 0; code < total; ++code) {
    Host h(start);
    unsigned long long c = code;
    for (uint32_t d = 0; d < depth; ++d, c /= 5u) switch (c % 5u) {
        case 0: h.direct(); break;
        case 1: h.tags.status_dirty = true; break;
        case 2: h.chain(Ga, 1); break;
        case 3: h.chain(Gb, 1); break;
        default: h.chain(Ga, 2); break;
      }
    ++sequences;
  }
}

int main() {
  // chains: every even length up to the default MIP_TUNE_GRAPH_ROUND (64 frames, one frame slot; F slots or a smaller round
  // give shorter ones), beside a short one and, for three of them, the longest; starts (MIP_TEST_EPOCH_START): a fresh state,
  // and every value from which the sequence meets the wrap
  for (uint32_t Ga = 2; Ga <= 64u; Ga += 2)
    for (uint32_t Gb : {2u, 64u}) {
      if (Gb == 64u && Ga != 2u && Ga != 6u && Ga != 62u) continue;
      for (uint32_t start : {0u, 1u, 2u, 1000u, 1001u}) enumerate(start, Ga, Gb, 5);
      for (uint32_t below = 0; below <= Ga + 6u; ++below) enumerate(kPlanMaxEpoch - below, Ga, Gb, 5);
    }
  // a round far above the default (MIP_TUNE_GRAPH_ROUND=4096)
  for (uint32_t below : {0u, 1u, 4095u, 4096u, 4097u, 4098u, 4099u, 8192u, 8195u}) enumerate(kPlanMaxEpoch - below, 4096, 2, 4);
  // long runs through several wraps: direct launches with a chain and a replay of an older chain in between
  for (uint32_t G : {2u, 6u, 64u}) {
    Host h(kPlanMaxEpoch - 100000u);
    for (uint32_t k = 0; k < 300000u; ++k) {
      h.direct();
      if (k % 7u == 3u) h.chain(G, 1 + k % 2u);
      if (k % 11u == 5u) h.chain(2, 1);
    }
  }
  CHECK(clears > 1000 && bumps > 1000 && zeroings > 1000, "the sweep met the wrap (%llu clears), the parity skip (%llu) and the zeroing in front of a replay (%llu)",
        clears, bumps, zeroings);
  std::printf("TAGS OK %llu sequences %llu launches (%llu clears, %llu skipped tags, %llu zeroings)\n", sequences, launches, clears, bumps, zeroings);
  return 0;
}
