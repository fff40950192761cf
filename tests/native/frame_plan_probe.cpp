// frame_plan_probe.cpp — prints the LaunchPlan plan_frame (renderer_amd/csrc/frame_plan.hpp) gives for one context state and one
// request, as one JSON line per instance count. Plain C++, no HIP: built by tests/plan_boundaries.py with g++, so that the
// boundary sizes the GPU tests run at are READ from the plan and not copied into a table (tests/test_plan_boundaries.py).
//
//   frame_plan_probe key=value ...          (every key optional)
//     cu_count=256 n=1000 n_meshes=64 frame_slots=1 max_lod_tris=0 max_instances=<n> n_joints=0
//     nonfinite=0 force_general=0 force_order=0 tri_chunks_from=0 tri_block_max=65536 tri_parts_max=1024 tri_block_threads=0
//     request=model,bitmap,cmds,aabb,tlas,triangles,skinned,wire,packed,async,host   (cmds implies count and index_total)
//             draw_cmds,count,index_total   (each pointer of the command outputs on its own: every combination, refused ones too)
//     sweep=FIRST:LAST:STEP   instead of n=: one line per n = FIRST, FIRST+STEP, ... <= LAST
//     tri_range_blocks=0 tri_chunk_blocks_per_cu=8
//     rules=TOTAL:N_WAVES:TICKET_SLOTS[:INDEX_COUNT,INDEX_COUNT,...]   instead of a plan: one JSON line with the rules of the range
//             decomposition and of the size-class sort — range_slots(TOTAL, N_WAVES, TICKET_SLOTS), its limits, the commands per
//             ticket of every class, the class of every INDEX_COUNT, and the range grid of the state given so far
// The constants of the prefix structure that are no plan field (tile, level-1 window) are printed with every line.
#include "../../renderer_amd/csrc/frame_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

using namespace mip;

// = kLevel1Window (instance_kernel.hpp, a HIP header this program cannot include; tests/test_plan_boundaries.py compares the two)
static const unsigned kProbeLevel1Window = 64;

static const char* tri_name(TriangleKernel k) {
  switch (k) {
    case TriangleKernel::none: return "none";
    case TriangleKernel::parts: return "parts";
    case TriangleKernel::block: return "block";
    case TriangleKernel::waves: return "waves";
    case TriangleKernel::chunks: return "chunks";
    case TriangleKernel::sorted: return "sorted";
  }
  return "?";
}

static const char* recompact_name(Recompact r) { return r == Recompact::none ? "none" : (r == Recompact::single ? "single" : "wide"); }

static void print_plan(const PlanState& st, const LaunchPlan& p) {
  std::printf("{\"n\": %u, \"status\": %d, \"empty\": %d, \"n_tiles\": %u, \"order\": %d, \"general\": %d, \"box_override\": %d, \"wire\": %d, "
              "\"group_shift\": %u, \"uses_prefix_state\": %d, \"tri\": \"%s\", \"tri_threads\": %u, \"tri_blocks\": %u, \"tri_block_tickets\": %d, \"tri_either_blocks\": %u, "
              "\"recompact\": \"%s\", \"recompact_blocks\": %u, \"skin\": %d, \"tile\": %u, \"level1_window\": %u}\n",
              st.n, (int)p.status, (int)p.empty, p.n_tiles, p.order, (int)p.general, (int)p.box_override, p.wire, p.group_shift, (int)p.uses_prefix_state, tri_name(p.tri),
              p.tri_threads, p.tri_blocks, (int)p.tri_block_tickets, p.tri_either_blocks, recompact_name(p.recompact), p.recompact_blocks,
              (int)p.skin, kPlanTile, kProbeLevel1Window);
}

int main(int argc, char** argv) {
  PlanState st;
  PlanRequest rq;
  st.have_instances = st.have_meshes = st.have_geometry = true;
  st.n_meshes = 64;
  st.n = 1000;
  rq.flags = MIP_OUT_DEVICE;
  bool max_given = false;
  unsigned long first = 0, last = 0, step = 0;
  for (int a = 1; a < argc; ++a) {
    const char* eq = std::strchr(argv[a], '=');
    if (!eq) {
      std::fprintf(stderr, "frame_plan_probe: '%s' is not key=value\n", argv[a]);
      return 2;
    }
    const std::string key(argv[a], eq - argv[a]);
    const char* val = eq + 1;
    const uint32_t u = (uint32_t)std::strtoul(val, nullptr, 10);
    if (key == "cu_count") st.cu_count = u;
    else if (key == "n") st.n = u;
    else if (key == "n_meshes") st.n_meshes = u;
    else if (key == "frame_slots") st.frame_slots = u;
    else if (key == "max_lod_tris") st.max_lod_tris = u;
    else if (key == "max_instances") st.max_instances = u, max_given = true;
    else if (key == "n_joints") st.n_joints = u;
    else if (key == "nonfinite") st.nonfinite = u != 0;
    else if (key == "force_general") st.force_general = u != 0;
    else if (key == "force_order") st.force_order = (int)u;
    else if (key == "tri_chunks_from") st.tri_chunks_from = u;
    else if (key == "tri_block_max") st.tri_block_max = u;
    else if (key == "tri_parts_max") st.tri_parts_max = u;
    else if (key == "tri_block_threads") st.tri_block_threads = u;
    else if (key == "tri_range_blocks") st.tri_range_blocks = u;
    else if (key == "tri_chunk_blocks_per_cu") st.tri_chunk_blocks_per_cu = u;
    else if (key == "rules") {
      unsigned long total = 0, n_waves = 0, ticket_slots = 0;
      int used = 0;
      if (std::sscanf(val, "%lu:%lu:%lu%n", &total, &n_waves, &ticket_slots, &used) != 3 || n_waves == 0) {
        std::fprintf(stderr, "frame_plan_probe: rules=TOTAL:N_WAVES:TICKET_SLOTS[:INDEX_COUNT,...]\n");
        return 2;
      }
      std::printf("{\"range_slots\": %u, \"range_min_slots\": %u, \"range_max_slots\": %u, \"range_blocks\": %u, \"sort_batch\": [",
                  range_slots((uint32_t)total, (uint32_t)n_waves, (uint32_t)ticket_slots), kRangeMinSlots, kRangeMaxSlots,
                  plan_tri_range_blocks(st.cu_count, st.tri_chunk_blocks_per_cu, st.tri_range_blocks));
      for (uint32_t k = 0; k < 32u; ++k) std::printf("%s%u", k ? ", " : "", plan_tri_sort_batch(k));
      std::printf("], \"size_class\": [");
      const char* at = val + used;
      for (bool first_one = true; *at == ':' || *at == ',';) {
        char* end = nullptr;
        const uint32_t index_count = (uint32_t)std::strtoul(at + 1, &end, 10);
        if (end == at + 1) break;
        std::printf("%s%u", first_one ? "" : ", ", tri_size_class(index_count));
        first_one = false;
        at = end;
      }
      std::printf("]}\n");
      return 0;
    }
    else if (key == "sweep") {
      if (std::sscanf(val, "%lu:%lu:%lu", &first, &last, &step) != 3 || step == 0) {
        std::fprintf(stderr, "frame_plan_probe: sweep=FIRST:LAST:STEP\n");
        return 2;
      }
    } else if (key == "request") {
      std::string list(val);
      list += ',';
      for (size_t b = 0, e; (e = list.find(',', b)) != std::string::npos; b = e + 1) {
        const std::string w = list.substr(b, e - b);
        if (w.empty()) continue;
        if (w == "model") rq.model = true;
        else if (w == "bitmap") rq.bitmap = true;
        else if (w == "cmds") rq.cmds = rq.count = rq.index_total = true;
        else if (w == "draw_cmds") rq.cmds = true;
        else if (w == "count") rq.count = true;
        else if (w == "index_total") rq.index_total = true;
        else if (w == "aabb") rq.aabb = true;
        else if (w == "tlas") rq.tlas = true;
        else if (w == "triangles") rq.triangles = true;
        else if (w == "skinned") rq.skinned = true;
        else if (w == "wire") rq.flags |= MIP_OUT_WIRE;
        else if (w == "packed") rq.flags |= MIP_OUT_WIRE | MIP_OUT_WIRE_PACKED;
        else if (w == "async") rq.flags |= MIP_OUT_ASYNC;
        else if (w == "host") rq.flags &= ~(uint32_t)MIP_OUT_DEVICE;
        else {
          std::fprintf(stderr, "frame_plan_probe: unknown request bit '%s'\n", w.c_str());
          return 2;
        }
      }
    } else {
      std::fprintf(stderr, "frame_plan_probe: unknown key '%s'\n", key.c_str());
      return 2;
    }
  }
  if (step == 0) first = last = st.n, step = 1;
  for (unsigned long n = first; n <= last; n += step) {
    st.n = (uint32_t)n;
    if (!max_given) st.max_instances = st.n ? st.n : 1u;
    print_plan(st, plan_frame(st, rq));
  }
  return 0;
}
