// batch_plan_probe.cpp — prints the plan of ONE batched-draws call (renderer_amd/csrc/batch_plan.hpp: plan_batch or
// plan_batch_sorted, batch_pass_io, batch_pass_launch) as a line of JSON, for tests/batch_stage_model.py: the model of the binning
// stage reads the pass count, the shifts, the ping-pong and the kernel kinds from here and restates none of them. Plain C++, no HIP.
//
//   batch_plan_probe <entry: draws|lods|ordered|views|shard> <relative 0|1> <buckets> <want_model 0|1> <general 0|1>
//   batch_plan_probe sorted <relative 0|1> <axis 0|1> <depth_bits> <want_model 0|1> <general 0|1>
#include "../../renderer_amd/csrc/batch_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace mip;
using K = BatchKernel;

// The kinds the model tells apart; every kernel that forms keys from the instance columns is "columns".
static const char* kind(K k) {
  switch (k) {
    case K::none: return "none";
    case K::count_list: return "count_list";
    case K::scatter_list_mid: return "list_mid";
    case K::scatter_list_last: return "list_last";
    case K::scatter_views_list_last: return "views_list_last";
    case K::rowscan: return "rowscan";
    case K::commands_pair: return "pair";
    case K::commands_chain: return "chain";
    case K::commands_views: return "views";
    case K::commands_shard: return "shard";
    case K::sorted_members: return "sorted_members";
    default: return "columns";
  }
}

static const char* grid(BatchGrid g) { return g == BatchGrid::tiles ? "tiles" : g == BatchGrid::bins ? "bins" : "one"; }

int main(int argc, char** argv) {
  if (argc != 6 && argc != 7) return 2;
  const bool sorted = std::strcmp(argv[1], "sorted") == 0;
  if (sorted != (argc == 7)) return 2;
  BatchPlan plan{};
  bool want_model = false;
  if (sorted) {
    want_model = std::atoi(argv[5]) != 0;
    plan = plan_batch_sorted(std::atoi(argv[2]) != 0, std::atoi(argv[3]) != 0, (uint32_t)std::atoi(argv[4]), want_model, std::atoi(argv[6]) != 0);
  } else {
    const char* names[] = {"draws", "lods", "ordered", "views", "shard"};
    int e = -1;
    for (int k = 0; k < 5; ++k)
      if (std::strcmp(argv[1], names[k]) == 0) e = k;
    if (e < 0) return 2;
    want_model = std::atoi(argv[4]) != 0 && e != 3 && e != 4;  // views and shards take no batch_model
    plan = plan_batch((BatchEntry)e, std::atoi(argv[2]) != 0, std::strtoull(argv[3], nullptr, 10), want_model, std::atoi(argv[5]) != 0);
  }
  std::printf("{\"passes\": %u, \"several\": %s, \"digit_bits\": %u, \"model_kernel\": %s, \"pass\": [", plan.passes, plan.several() ? "true" : "false",
              kBatchDigitBits, plan.model != K::none ? "true" : "false");
  for (uint32_t p = 0; p < plan.passes; ++p) {
    const BatchPassIo io = batch_pass_io(plan, p, want_model, !sorted);
    std::printf("%s{\"shift\": %u, \"totals_row\": %u, \"list_in\": %d, \"list_out\": %d, \"ids\": %s, \"slot_of\": %s, \"model\": %s, \"bucket_hist\": %s, "
                "\"commands\": %s, \"launch\": [",
                p ? ", " : "", io.shift, io.totals_row, io.list_in, io.list_out, io.ids ? "true" : "false", io.slot_of ? "true" : "false",
                io.model ? "true" : "false", io.bucket_hist ? "true" : "false", io.commands ? "true" : "false");
    for (uint32_t i = 0; i < kBatchPassLaunches; ++i) {
      const BatchLaunch l = batch_pass_launch(plan, p, i);
      std::printf("%s[\"%s\", \"%s\"]", i ? ", " : "", kind(l.kernel), grid(l.grid));
    }
    std::printf("]}");
  }
  std::printf("]}\n");
  return 0;
}
