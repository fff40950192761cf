// context.hpp — the state behind a MipContext and the helpers the seven host translation units share.
//   api_context.hip   create / destroy, uploads (mesh table, instances, geometry, skeleton, poses), census, diagnostics
//   api_frame.hip     one frame: plan (frame_plan.hpp) -> tag (prefix_tags.hpp) -> launches; the per-triangle stage's host side;
//                     recorded launch graphs; views; light lists; mip_wait
//   api_sharded.hip   shard merges, the collective-library seam, mip_run_sharded and its collective repair
//   api_interop.hip   external memory and external semaphores (row f-2)
//   api_occlusion.hip the occlusion-culling extension: depth pyramid builds, mip_run_occluded (occlusion_kernel.hpp)
//   api_batch.hip     the batched-draws extension: mip_batch_draws, _lods, _ordered, _shard, _sorted and _views — one stage
//                     (batch_kernel.hpp) under the key policies of batch_lods_kernel.hpp, batch_views_kernel.hpp and
//                     batch_sorted_kernel.hpp, planned by batch_plan.hpp and run by one pass driver; mip_merge_batches
//                     (batch_merge_kernel.hpp, batch_merge_plan.hpp)
//   api_cluster.hip   the cluster-culling extension: mip_build_clusters, mip_cull_clusters, mip_cull_clusters_phase (cluster_kernel.hpp, cluster_plan.hpp),
//                     mip_cull_clusters_views (cluster_views_kernel.hpp, cluster_views_plan.hpp)
// (round 3 had all of it in one 2 224-line mip_api.hip)
#pragma once

#include "../../include/mi_instance_pipeline.h"
#include "frame_plan.hpp"
#include "prefix_tags.hpp"
#include "instance_kernel.hpp"  // rows a-1 .. a-7 (the kernel itself is instantiated in api_frame.hip and stages_tu.hip only)
#include "stage_args.hpp"      // argument blocks + launchers of everything built in stages_tu.hip
#include "mesh_chain.hpp"      // the per-mesh LOD chain of mip_batch_draws_lods
#include "batch_merge_plan.hpp" // the shard chunk of batched draws, mip_merge_batches' plan and its two error bits

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types only: the library is opened with dlopen, never linked

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

constexpr uint32_t kHelpWords = mip::kHelpShards + 1;  // MipContext::d_help
constexpr uint32_t kHelpHintWord = 8;                  // of MipContext::h_error (the error words are [0, mip::kErrWords))
constexpr uint32_t kFirstMoverLaunches = 8;            // launches that follow the first-mover rule after a hint
static_assert(kHelpHintWord >= mip::kErrWords, "the hint must not be an error word");

struct MipContext {
  int device = -1;
  uint32_t max_instances = 0, max_meshes = 0, cfg_flags = 0;
  uint32_t n = 0, m = 0;
  bool have_instances = false, have_meshes = false;
  int force_order = 0;         // tuning (MIP_TUNE_ORDER): 1 or 3, 0 = by instance count
  bool force_general = false;  // tuning/tests (MIP_TUNE_FORCE_GENERAL): always launch the kernel with the literal cold path
  // One slot per frame in flight: its own stream and its own cross-tile prefix state, so that
  // consecutive frames may overlap on the device (MipConfig.frames_in_flight).
  struct FrameSlot {
    hipStream_t stream = nullptr;
    bool own_stream = false;
    unsigned long long* d_status = nullptr;  // level-0 granules, accumulators, group starts
    uint32_t* d_scalars = nullptr;           // [0] draw_count, [1] index_total (host-output runs), [2] pre-triangle count, [3] command ticket
    uint32_t* d_tmp_cmds = nullptr;          // per-triangle stage: the instance kernel's list before re-compaction
    uint32_t* d_tmp_src = nullptr;           //                     and each command's source index offset
    unsigned long long* d_tmp_blocks = nullptr;  //                 re-compaction of large frames: one granule per 1024 commands
    uint32_t recompact_epoch = 0;            //                     tag of the last one-launch re-compaction on this slot
    bool tri_ticket_clean = false;           //                     the stage's ticket word (d_scalars + 3) was cleared by the last frame's re-compaction
    bool tri_sort_clean = false;             //                     ... and so was d_tri_sort
    uint32_t* d_tmp_final = nullptr;         //                     parts kernel: each command's final indexCount (never written into the command)
    unsigned long long* d_part_status = nullptr;  //                small frames: one granule per (command, part)
    uint32_t tri_epoch = 0;                  //                     tag of the last parts launch on this slot
    uint32_t* d_chunk_first = nullptr;       // range kernel (round 5): first command of every range of the triangle stream
    unsigned long long* d_chunk_status = nullptr;  //                   one granule per range
    size_t chunks_cap = 0;                   //                         ranges both arrays hold
    uint32_t chunk_epoch = 0;                //                         tag of the last range launch on this slot
    uint32_t* d_tri_order = nullptr;         // large frames: command numbers by descending size class
    uint32_t* d_tri_sort = nullptr;          //               kSortWords words: histogram, positions, tickets (triangle_kernels.hpp)
    float* d_skin_box = nullptr;             // skinned frames: per instance posed mesh-space box {min xyz, -, max xyz, -}
    uint32_t* d_pyramid_counter = nullptr;   // depth pyramid builds on this slot's stream: workgroups done (the last one resets it)
    // recorded launches (mip_run_many): the frames of one replay, read by the kernels (KernelArgs.frame_ring),
    // refreshed before every replay from one of two pinned staging halves
    uint32_t* d_frame_ring = nullptr;
    uint32_t* h_frame_stage = nullptr;
    uint32_t frame_ring_frames = 0, stage_next = 0;
    hipEvent_t stage_free[2] = {nullptr, nullptr};
    mip::PrefixTags tags;       // which tag the next launch on d_status gets (prefix_tags.hpp)
  };
  // mip_run_many replays: per slot one linear hipGraph of `frames` launches with baked tags
  // base_epoch+1 .. base_epoch+frames (see run_many_graphed).
  struct FrameGraph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    uint32_t base_epoch = 0;
  };
  struct GraphSet {
    std::vector<MipOutputs> outs;
    uint32_t first_slot = 0, frames_per_slot = 0;
    uint64_t generation = 0;
    std::vector<FrameGraph> per_slot;
  };
  std::vector<GraphSet> graph_sets;   // small LRU, newest last
  uint64_t graph_generation = 1;      // bumped whenever something a graph bakes in changes
  uint32_t graph_round = 64;          // frames per replay round over all slots (MIP_TUNE_GRAPH_ROUND, 0 = off)
  std::vector<FrameSlot> slots;
  uint32_t next_slot = 0;
  // batched draws (api_batch.hip): the scratch of the pass driver, every buffer allocated at first need and replaced by a
  // larger one when a call asks for more. `batch`: one per frame slot, for the entry points that run behind a frame, always
  // asked for the context's capacities (max_instances entries, MIP_MAX_LODS x max_meshes histogram words), so every buffer
  // is allocated once. `view_batch`: mip_batch_draws_views' own on the first stream, asked for the n_views x N entries and
  // the histogram copies of the call.
  struct BatchScratch {
    uint32_t* d_counts = nullptr;       // [256 bins][tiles of entries] members per (bin, tile), scanned in place
    uint32_t* d_totals = nullptr;       // kBatchMaxPasses x 256 digit totals + the member count
    uint32_t* d_keys[2] = {nullptr, nullptr};  // several passes: the (key, instance) lists between passes
    uint32_t* d_ids[2] = {nullptr, nullptr};
    uint32_t* d_bucket_hist = nullptr;  //   members per bucket (views: per global bucket, in every one of hist_copies copies)
    uint32_t* d_slot_of = nullptr;      //   slot of every member by instance (batch_model)
    uint32_t* d_bucket_of = nullptr;    // mip_batch_draws_sorted: bucket of every member by instance (the run stage)
    size_t tiles_cap = 0, list_cap = 0, hist_cap = 0, slot_cap = 0, bucket_cap = 0;  // tiles d_counts holds, entries of each list, words of d_bucket_hist, entries of the two maps
  };
  std::vector<BatchScratch> batch;
  BatchScratch view_batch;
  // mip_merge_batches (api_batch.hip): the offsets kernel's tables on the first stream (batch_merge_plan.hpp says what they
  // hold), allocated at first use for the n_chunks x B asked for and grown by a larger call
  struct BatchMergeScratch {
    uint32_t* d_words = nullptr;
    size_t words_cap = 0;
  };
  BatchMergeScratch batch_merge;
  // cluster culling (api_cluster.hip): the table mip_build_clusters makes from the resident geometry — stale (valid = false)
  // after mip_set_mesh_table / mip_set_geometry until it is built again — and mip_cull_clusters' scratch per frame slot,
  // allocated at first use and grown by a larger call
  struct ClusterTable {
    float4* d_boxes = nullptr;          // two per cluster, bucket-major: {min xyz, -}, {max xyz, -}
    uint32_t* d_cluster_base = nullptr; // B + 1 words: the exclusive prefix sum of C over the buckets, and the total
    size_t boxes_cap = 0, base_cap = 0; // clusters / words the two hold
    uint32_t total = 0, max_clusters = 0;  // clusters in the table; the largest C of a bucket
    bool valid = false;
    // the normal cones mip_build_cluster_cones makes of a valid table (cluster_cone_plan.hpp): stale with the table
    float4* d_cones = nullptr;          // two per cluster, bucket-major: {axis xyz, k}, {centre xyz, r}
    size_t cones_cap = 0;
    bool cones_valid = false;
  };
  ClusterTable clusters;
  struct ClusterScratch {
    uint32_t* d_instances = nullptr;    // items, bucket, member_first (+1), member_inst: 4 x instance_cap + 1 words
    unsigned long long* d_tile_items = nullptr;  // per instance tile
    uint32_t* d_tile_members = nullptr;
    uint32_t* d_scalars = nullptr;
    void* d_words = nullptr;            // 16 bytes per 64 work items: the survive word and the start word
    uint32_t* d_tile_heads = nullptr;   // per head tile: heads
    uint32_t* d_tile_survivors = nullptr;  //              survivors
    uint32_t* d_tile_candidates = nullptr;  //           the record's candidates (a FIRST call of mip_cull_clusters_phase)
    size_t words_cap = 0, head_tiles_cap = 0, survivor_tiles_cap = 0, candidate_tiles_cap = 0;
    // mip_cull_cluster_triangles (cluster_triangle_plan.hpp): 12 bytes per work item of the call's bound on top
    uint32_t* d_tri_scalars = nullptr;
    unsigned long long* d_triangle_words = nullptr;  // per work item: the ballot of its cluster's surviving triangles
    uint32_t* d_item_prefix = nullptr;  // per work item + 1: the surviving triangles in front of it
    uint32_t* d_word_total = nullptr;   // per survive word: the surviving triangles of its 64 items
    uint32_t* d_tile_triangles = nullptr;  // per item tile: surviving triangles (then their prefix), behind them the tested ones
    size_t triangle_words_cap = 0, item_prefix_cap = 0, word_total_cap = 0, tile_triangles_cap = 0;
    // mip_list_clusters (cluster_list_plan.hpp): 8 bytes per 64 work items of the call's bound on top
    uint32_t* d_word_member = nullptr;  // per survive word: the member of its first work item
    uint32_t* d_word_rank = nullptr;    // per survive word: the survivors of its list tile in front of it
    uint32_t* d_list_tiles = nullptr;   // per list tile: survivors, then their prefix
    size_t word_member_cap = 0, word_rank_cap = 0, list_tiles_cap = 0;
    // mip_list_clusters_phase (cluster_list_phase_plan.hpp) on top of the list's: a row of list tiles and two words
    uint32_t* d_list_candidates = nullptr;  // per list tile: the candidates of its record words (FIRST)
    uint32_t* d_list_phase_scalars = nullptr;  // the entry base and the room, from the epilogue to the write kernel
    size_t list_candidates_cap = 0;
    // mip_list_cluster_triangles (cluster_triangle_list_plan.hpp) on top of the list's; d_triangle_words and d_tile_triangles
    // above are shared with mip_cull_cluster_triangles (one stream per slot: the calls follow each other)
    unsigned long long* d_nonempty_words = nullptr;  // per 64 work items: the surviving items that keep a triangle
    uint32_t* d_tile_clusters = nullptr;  // per list tile: surviving clusters
    size_t nonempty_words_cap = 0, tile_clusters_cap = 0;
  };
  std::vector<ClusterScratch> cluster_scratch;
  // mip_cull_clusters_views (cluster_views_plan.hpp): its own scratch on the first stream, as view_batch is — no frame slot's
  // cluster scratch is touched. Allocated at first use, grown by a larger call.
  struct ClusterViewScratch {
    uint32_t* d_instances = nullptr;    // items, bucket, member_inst, member_first (+1): 4 x instance_cap + 1 words
    uint16_t* d_view_mask = nullptr;    // instance_cap: the views whose bitmap holds the instance
    unsigned long long* d_tile_items = nullptr;  // per instance tile
    uint32_t* d_tile_members = nullptr;
    uint32_t* d_scalars = nullptr;
    unsigned long long* d_view_words = nullptr;  // (1 + n_views) planes of one word per 64 work items: start, then every view's survive words
    uint32_t* d_tile_heads = nullptr;   // n_views rows of head tiles
    uint32_t* d_tile_survivors = nullptr;
    size_t words_cap = 0, head_rows_cap = 0, survivor_rows_cap = 0;
    // mip_list_clusters_views (cluster_views_list_plan.hpp), grown by that call: both several-view calls run on `stream`
    uint32_t* d_word_member = nullptr;  // one plane: per 64 work items, the member of the word's first item
    uint32_t* d_word_rank = nullptr;    // n_views planes
    uint32_t* d_list_tiles = nullptr;   // n_views rows of list tiles
    size_t word_member_cap = 0, word_rank_cap = 0, list_tiles_cap = 0;
  };
  ClusterViewScratch cluster_views;
  uint32_t* h_cluster_views_status = nullptr;  // pinned, device-visible, two words: the code an asynchronous / a synchronous mip_cull_clusters_views or mip_list_clusters_views raised
  uint32_t* h_cluster_status = nullptr;  // pinned, device-visible, two words per frame slot: the code an asynchronous / a synchronous cull of the slot raised
  hipEvent_t cluster_pyramid_ready = nullptr;  // orders a cull behind a pyramid built on another slot's stream
  hipEvent_t cluster_record_written = nullptr;  // behind the last FIRST call of mip_cull_clusters_phase: its SECOND call waits for it, on whichever slot's stream
  std::vector<FrameSlot> view_states;  // mip_run_views: one prefix state per view, all on `stream`
  hipStream_t stream = nullptr;  // = slots[0].stream: uploads, merges, timing
  // resident inputs
  float* d_pos = nullptr;
  float4* d_rot = nullptr;
  float* d_scale = nullptr;
  uint32_t* d_mesh_id = nullptr;
  // the frame kernel's copy of the ids, frame_id_bytes (1 | 2) each: plan_frame_id_bytes(max_meshes), fixed at creation; every
  // upload that writes d_mesh_id writes it too (in the census kernel). 0 / null: max_meshes > 65 536, or
  // MIP_TUNE_WIDE_IDS — the frame kernel reads d_mesh_id like every other kernel
  void* d_frame_ids = nullptr;
  uint32_t frame_id_bytes = 0;
  mip::MeshEntry* d_meshes = nullptr;
  mip::MeshDraw* d_mesh_draw = nullptr;
  mip::MeshChain* d_mesh_chain = nullptr;  // mip_batch_draws_lods: every level of every mesh (filled by mip_set_mesh_table)
  uint32_t* d_bucket_lod = nullptr;        //   mesh << 3 | lod of every (mesh, LOD) bucket, MIP_MAX_LODS x max_meshes words
  unsigned long long lod_buckets = 0;      //   B = sum of n_lods over the table
  unsigned long long* d_blas = nullptr;  // per-mesh BLAS device addresses (optional, row f-4): max_meshes entries, allocated by the first
                                         // mip_set_blas_addresses; zeroed whole by every mip_set_mesh_table (the addresses are the old table's)
  // consolidated geometry for the per-triangle stage (row f-1)
  float* d_vertices = nullptr;
  uint32_t* d_indices = nullptr;
  uint32_t n_vertices = 0, n_indices = 0;
  bool have_geometry = false;
  bool geometry_finite = false;  // every uploaded position is finite (lets the triangle stage skip exact no-ops)
  // host copies kept to check the mesh table against the geometry before the per-triangle stage gathers
  // vertices[vertex_offset + index] and indices[index_offset ..] unchecked on the device
  std::vector<MipMesh> h_meshes;
  std::vector<uint32_t> h_indices;
  int geometry_checked = 0;  // 0 = not yet, 1 = consistent, -1 = inconsistent (message in geometry_error)
  std::string geometry_error;
  // skinned extension (mip_set_skeleton / mip_set_poses / mip_run_skinned)
  mip::JointEntry* d_joints = nullptr;
  uint32_t n_joints = 0, max_joint_depth = 0;
  float joint_box_bound = INFINITY;  // 3 * max |joint_box| + 1, +inf while a joint box holds a non-finite value (SkinArgs.box_bound)
  uint8_t joint_level_start[mip::kMaxJoints + 2] = {0};
  uint32_t joint_level_inv[mip::kMaxJoints + 1] = {0};
  float* d_poses_owned = nullptr;
  const float* d_poses = nullptr;  // owned copy or a borrowed device pointer
  uint32_t poses_n = 0;
  int cu_count = 0;
  // layout of a slot's prefix state (words of 8 bytes)
  size_t status_bytes = 0;
  uint32_t acc1_offset_words = 0, start1_offset_words = 0, helps_seen_offset_words = 0, groups_cap = 0;
  // the frame kernel's first-mover rule (instance_kernel.hpp, KernelArgs.first_mover_rule): followed by the launches that come
  // after a launch whose tile 0 saw new helps (it writes the count to h_error[kHelpHintWord])
  bool no_one_mesh = false;               // MIP_TUNE_NO_ONE_MESH: a one-entry mesh table is gathered from like any other (A/B runs, tests of that path)
  uint32_t first_mover_env = 0;           // MIP_TUNE_FIRST_MOVER=always|never -> 1|2, read at context creation; 0: as the hints say
  uint32_t help_hint_seen = 0;            // the hint word's value when the host last looked
  uint32_t first_mover_launches_left = 0; // launches that still follow the rule
  uint32_t lds_pad = 0;  // tuning only (MIP_TUNE_LDS_PAD): dynamic LDS bytes that cap workgroups per CU
  uint32_t tri_block_threads = 0;  // tuning (MIP_TUNE_TRI_BLOCK_THREADS): 256 / 512 / 1024, 0 = by instance count
  uint32_t tri_block_max = 65536;  // instance counts up to this use the workgroup-per-command triangle kernel
  uint32_t tri_parts_max = 1024;   // instance counts up to this use the parts kernel (16 work items per command), 0 = off
  bool tri_recompact_three_launches = false;  // MIP_TUNE_TRI_RECOMPACT_LAUNCHES=3: round 4's count / scan / scatter instead of the one-launch form (A/B, tests)
  uint32_t tri_ticket_slots = 4096; // long triangle streams: slots per range of the range kernel (MIP_TUNE_TRI_RANGE_SLOTS: 256 .. 8192, whole steps of 64)
  uint32_t tri_range_blocks = 0;   // MIP_TUNE_TRI_RANGE_BLOCKS: workgroups of the range grid and the large-frame stage grid (tests); 0 = the resident grid
  uint32_t tri_chunks_from = 0;    // instance counts from this use the range kernel; MIP_TUNE_TRI_CHUNKS_FROM (4294967295 = never: the round-4 kernels)
  bool tri_no_choice = false;      // tuning (MIP_TUNE_TRI_NO_CHOICE): large frames always take the wave-per-command kernel
  int tri_force_choice = 0;        // tuning (MIP_TUNE_TRI_CHOICE=block|waves): 1 / 2 force the device-side choice of the large-frame grid
  uint32_t tri_batch_from = 65536; // commands from which the ticket-pulling workgroup kernel takes four per ticket (MIP_TUNE_TRI_BATCH_FROM: tests)
                                   // measured (DamagedHelmet entry, frame time parts / workgroup-per-command): 30 instances 14 / 24 us,
                                   // 200: 16 / 25, 1000: 41 / 47, 2000: 67 / 64, 4000: 113 / 83
  uint32_t max_lod_tris = 0;       // largest triangle count of LOD 0 / LOD 1 over the mesh table
  // upload-time census of instances that fail the kernel's finite test (instance_kernel.hpp,
  // finite_magnitude): while it is zero, frames run the kernel without the literal cold path
  uint64_t nonfinite_instances = 0;
  float box_abs = 0.f;  // largest sum of |box coordinates| over the mesh table (the census' overflow bound)
  uint32_t* d_census = nullptr;
  uint32_t* h_error = nullptr;  // pinned, device-visible: error words [0, kErrWords)
  uint32_t* d_help = nullptr;   // device memory, kHelpWords words: helped tile aggregates (MipTimings.prefix_helps = their sum); read back by mip_get_timings
  uint32_t help_base = 0;       // its value at the last mip_reset_timings
  uint32_t* d_error = nullptr;  // device alias of h_error
  uint32_t carried_error_bits = 0;  // error bits a synchronous call saw while asynchronous work was in flight: reported then AND by the next mip_wait
  // staging for MIP_OUT_HOST
  float4* s_model = nullptr;
  uint32_t* s_bitmap = nullptr;
  uint32_t* s_cmds = nullptr;
  float* s_aabb = nullptr;
  // timing
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  MipTimings timings{};
  bool pending_async = false;
  // native sharded exchange (mip_comm_*, mip_run_sharded)
  ncclComm_t comm = nullptr;
  uint32_t comm_rank = 0, comm_world = 0;
  uint32_t shard_cap_max = 0;  // largest max_instances over the ranks: what every rank sizes its chunks by
  uint32_t last_error_bits = 0;
  int shard_wire = 2;          // what mip_run_sharded exchanges: 2 = the packed wire form whenever the largest shard fits it (else 1),
                               // 1 = 8-byte wire records, 0 = 20-byte commands (MIP_TUNE_SHARD_WIRE: A/B and tests)
  int sharded_form = 0;        // the form of the frame in flight (what the send buffer holds; repair_sharded_overflow re-sends it)
  uint32_t* d_send = nullptr;  // this rank's chunk, sized for max_instances commands
  uint32_t* d_recv = nullptr;  // world chunks
  // the last sharded frame, kept so that a tightened chunk that overflowed can be re-gathered at full capacity
  void* sharded_out_cmds = nullptr;
  uint32_t* sharded_out_count = nullptr;
  uint32_t sharded_pending = 0;  // sharded frames enqueued since the last completed wait
  // imported external memory (mip_import_external_fd)
  struct External { hipExternalMemory_t mem; void* ptr; };
  std::vector<External> externals;
  // imported external semaphores (mip_import_external_semaphore_fd); the handle given out is the entry's address
  // Two implementations behind one handle: the HIP runtime's own (hipImportExternalSemaphore: waits and signals
  // execute on the device), or — when the runtime refuses the handle type, as ROCm 7.2 on Linux does — the kernel
  // object itself: the fd of an exported Vulkan semaphore is a DRM sync object on amdgpu, imported on a render node
  // and waited for / signalled by host functions enqueued on the frame's stream (hipLaunchHostFunc).
  struct ExternalSemaphore {
    hipExternalSemaphore_t sem;
    uint32_t kind;
    uint32_t drm_handle;
    // DRM path, stream-value hand-over (api_interop.hip): two pinned, device-visible sequence words —
    // [0] waits granted by the waiter thread (the stream holds a hipStreamWaitValue64 on it),
    // [1] signals reached by the stream (hipStreamWriteValue64; the signaller thread polls it) — and the sequence numbers issued so far
    unsigned long long* words;
    unsigned long long wait_seq, signal_seq;
  };
  std::vector<ExternalSemaphore*> semaphores;
  struct SemaphoreWorkers;             // the two helper threads and their queues (api_interop.hip); created with the first DRM-path semaphore
  SemaphoreWorkers* semaphore_workers = nullptr;
  int drm_fd = -1;  // render node, opened on first use
  uint32_t last_slot = 0;  // slot of the frame issued last (mip_signal_external goes behind it)
  char err[512] = {0};
#ifdef MIP_DEBUG_STAMPS
  unsigned long long* d_stamps = nullptr;
#endif
};

namespace mip_host {

int32_t fail(MipContext* ctx, int32_t code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));

#define MIP_HIP(ctx, call)                                                                    \
  do {                                                                                        \
    hipError_t e_ = (call);                                                                   \
    if (e_ != hipSuccess)                                                                     \
      return mip_host::fail(ctx, e_ == hipErrorOutOfMemory ? MIP_ERR_OUT_OF_MEMORY : MIP_ERR_DEVICE, \
                            "%s failed: %s", #call, hipGetErrorString(e_));                   \
  } while (0)

inline uint32_t tiles_for(uint32_t n) { return (n + mip::kTile - 1) / mip::kTile; }
inline size_t instance_cap(const MipContext* ctx) { return ctx->max_instances ? ctx->max_instances : 1; }  // what per-instance scratch is sized by
static_assert(mip::kPlanTile == mip::kTile && mip::kPlanTriParts == mip::kTriParts && mip::kPlanTriPartMaxT == mip::kTriPartMaxT,
              "frame_plan.hpp restates kernel constants");
static_assert(mip::kPlanMaxEpoch == mip::kMaxEpoch, "prefix_tags.hpp restates the kernel's largest tag");

#ifdef MIP_DEBUG_STAMPS
// The diagnostic build's fault-injection switches (never the product), read from the environment by every launch (a test
// sets them between launches): the outputs must come out byte-identical whatever they say.
//   MIP_DEBUG_TILE_ORDER=reverse|scramble  a permutation tile -> (tile * mult + add) % n_tiles of the tile numbers (workgroups
//                                          then start in an order that is anything but ascending); reverse: the per-triangle
//                                          stage takes its work items from the last one down as well
//   MIP_DEBUG_SKIP_PART=k                  part k of every command (range k of every 16, every fourth re-compaction workgroup)
//                                          never publishes: its successors count it themselves
struct DebugSwitches {
  const char* order = std::getenv("MIP_DEBUG_TILE_ORDER");
  const char* skip = std::getenv("MIP_DEBUG_SKIP_PART");
  bool reverse() const { return order && std::strcmp(order, "reverse") == 0; }
  uint32_t skip_part(uint32_t parts) const { return skip ? (uint32_t)std::atoi(skip) % parts + 1u : 0u; }  // 0 = off
  void tile_order(uint32_t t, uint32_t& mult, uint32_t& add, bool can_scramble = true) const {
    if (t > 1u && reverse()) {
      mult = add = t - 1u;
    } else if (t > 1u && can_scramble && order && std::strcmp(order, "scramble") == 0) {
      static const uint32_t primes[] = {7919u, 104729u, 1299709u, 15485863u};
      for (uint32_t p : primes)
        if (t % p != 0u) { mult = p; break; }  // a prime that does not divide t is coprime to it
      add = 12345u % t;
    }
  }
};
#endif

// Room for `want` elements of `bytes_each` bytes at *p: kept while it is large enough, replaced by a larger allocation otherwise
// (hipFree waits for the work that still reads the old one). *cap is the number of elements *p holds.
template <class T>
int32_t grow(MipContext* ctx, T** p, size_t* cap, size_t want, size_t bytes_each) {
  if (*p && want <= *cap) return MIP_OK;
  (void)hipFree(*p);
  *p = nullptr;
  *cap = 0;
  MIP_HIP(ctx, hipMalloc(reinterpret_cast<void**>(p), (want ? want : 1) * bytes_each));
  *cap = want;
  return MIP_OK;
}

int32_t bind_device(MipContext* ctx);
int32_t sync_all(MipContext* ctx);
// Reads and clears the device-visible error words after streams have drained; runs the collective repair of a sharded
// frame when the merge kernel asked for it (api_sharded.hip).
int32_t check_device_error(MipContext* ctx);
// Number of instances of [first, first + count) that fail the finite test, and (bad_ids != null) how many name a mesh
// outside a table of `m` entries. Synchronous.
// narrow: the kernel also writes the ids of the range into the frame kernel's narrow column (d_frame_ids), where the context has one.
int32_t census(MipContext* ctx, uint32_t first, uint32_t count, uint32_t* out, uint32_t* bad_ids = nullptr, uint32_t m = 0, bool narrow = false);
void drop_graphs(MipContext* ctx);                    // api_frame.hip
// The tail of every entry point that enqueues on `stream`: asynchronous calls leave it to mip_wait, the others drain it.
inline int32_t finish(MipContext* ctx, hipStream_t stream, bool async) {
  if (async) { ctx->pending_async = true; return MIP_OK; }
  MIP_HIP(ctx, hipStreamSynchronize(stream));
  return check_device_error(ctx);
}
int32_t repair_sharded_overflow(MipContext* ctx);     // api_sharded.hip
void comm_release(MipContext* ctx);                   // api_sharded.hip: communicator + buffers, for mip_destroy
void interop_release(MipContext* ctx);                // api_interop.hip: imported memory and semaphores, for mip_destroy
int32_t interop_drain(MipContext* ctx);                // api_interop.hip: every queued signal of an external semaphore has been performed (mip_wait)
// occ != null: the occluded frame kernel (api_occlusion.hip, launch_occluded_frame) takes the frame kernel's place
int32_t run_frame(MipContext* ctx, const MipFrame* frame, const MipOutputs* out, bool skinned, void* palette,
                  const MipOcclusion* occ = nullptr);  // api_frame.hip
void batch_release(MipContext* ctx);                  // api_batch.hip: the batched-draws scratch, for mip_destroy
int32_t check_policy(MipContext* ctx, const MipLodPolicy* policy);  // api_batch.hip: MipLodPolicy as the header states it
void cluster_release(MipContext* ctx);                // api_cluster.hip: the cluster table and the culls' scratch, for mip_destroy
// api_cluster.hip: the status mip_wait returns — `rc`, or MIP_ERR_CAPACITY when an asynchronous mip_cull_clusters overflowed,
// MIP_ERR_DEVICE when an asynchronous SECOND call of mip_cull_clusters_phase met a record that is not its own
int32_t cluster_wait_status(MipContext* ctx, int32_t rc);
int32_t launch_occluded_frame(MipContext* ctx, const MipOcclusion* occ, mip::KernelArgs& a, const mip::LaunchPlan& plan, hipStream_t stream);  // api_occlusion.hip

}  // namespace mip_host
