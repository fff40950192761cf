// frame_ids_check.cpp — enumerates the width rule of the frame kernel's narrow mesh ids (renderer_amd/csrc/frame_plan.hpp:
// plan_frame_id_bytes, plan_frame_id_mode) and checks what the uploads and the kernel rely on. Plain C++, no HIP: built by
// tests/test_frame_ids_plan.py with gcc -fsanitize=address,undefined. Prints "IDS OK <combinations>".
#include "../../renderer_amd/csrc/frame_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <initializer_list>

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

int main() {
  unsigned long long combos = 0;
  // every capacity up to past the 2-byte rule, and the far end of the range
  auto capacities = [](auto&& f) {
    for (uint32_t cap = 0; cap <= 70000u; ++cap) f(cap);
    for (uint32_t cap : {0x7fffffffu, 0x80000000u, 0xfffffffeu, 0xffffffffu}) f(cap);
  };
  uint32_t last = 1;
  capacities([&](uint32_t cap) {
    const uint32_t bytes = plan_frame_id_bytes(cap);
    CHECK(bytes == 0u || bytes == 1u || bytes == 2u, "max_meshes %u: %u bytes", cap, bytes);
    // the largest id a table of max_meshes entries can hold fits the element (an id is < m <= max_meshes)
    if (bytes && cap) CHECK((uint64_t)(cap - 1u) < (1ull << (8u * bytes)), "max_meshes %u does not fit %u bytes", cap, bytes);
    // ... and it is the narrowest element that does
    if (bytes == 2u) CHECK(cap > 256u, "max_meshes %u would fit one byte", cap);
    if (bytes == 0u) CHECK(cap > 65536u, "max_meshes %u would fit two bytes", cap);
    const uint32_t width = bytes ? bytes : 4u;  // (capacities come in ascending order)
    CHECK(width >= last, "max_meshes %u: the width shrank from %u to %u", cap, last, width);
    last = width;
    CHECK(plan_frame_id_bytes(cap, true) == 0u, "MIP_TUNE_WIDE_IDS: the u32 column");
    ++combos;
    // the mode of every table the context can hold, at the sizes where anything changes
    for (uint32_t m : {0u, 1u, 2u, 255u, 256u, 257u, 65535u, 65536u, 65537u, cap}) {
      if (m > cap) continue;
      for (int wide = 0; wide < 2; ++wide)
        for (int no_one = 0; no_one < 2; ++no_one) {
          const uint32_t b = plan_frame_id_bytes(cap, wide != 0);
          const uint32_t mode = plan_frame_id_mode(m, b, no_one != 0);
          CHECK(mode == kIdsU32 || mode == kIdsOneMesh || mode == kIdsU8 || mode == kIdsU16, "mode %u", mode);
          CHECK((mode == kIdsOneMesh) == (m == 1u && !no_one), "one entry, and only one, is read as a scalar (m %u)", m);
          if (mode != kIdsOneMesh) {
            // the mode names the element the uploads wrote: it follows the context's width, never the table's size
            CHECK(mode == (b == 1u ? kIdsU8 : b == 2u ? kIdsU16 : kIdsU32), "max_meshes %u, m %u: mode %u for %u bytes", cap, m, mode, b);
            if (m) CHECK(mode == kIdsU32 || (uint64_t)(m - 1u) < (1ull << (mode == kIdsU8 ? 8 : 16)), "id %u does not fit mode %u", m - 1u, mode);
          }
          ++combos;
        }
    }
  });
  CHECK(plan_frame_id_bytes(256) == 1u && plan_frame_id_bytes(257) == 2u && plan_frame_id_bytes(65536) == 2u && plan_frame_id_bytes(65537) == 0u,
        "the edges of the rule");
  std::printf("IDS OK %llu\n", combos);
  return 0;
}
