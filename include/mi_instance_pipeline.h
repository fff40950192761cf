/*
 * mi_instance_pipeline.h — C ABI of the MI355X (gfx950) instance pipeline.
 *
 * One call per frame replaces, for every instance of a scene, this part of
 * farnoy/renderer (paths relative to the reference checkout):
 *
 *   src/ecs.rs:52-64       systems::model_matrix_calculation   M = T(p)·R(q)·S(s)
 *   src/ecs.rs:138-181     systems::aabb_calculation           mesh AABB -> world AABB
 *   src/renderer/systems/cull_pipeline.rs:99-120  coarse_culling   AABB vs 6 planes
 *   src/ecs.rs:117-136     systems::assign_draw_index          draw_index = array index
 *   src/renderer.rs:2266-2288  model_matrices_upload           model[draw_index] = M
 *   src/renderer/systems/cull_pipeline.rs:534-577 cull_pass    per-instance draw command
 *   src/renderer/helpers.rs:3-11  pick_lod                     LOD 1 beyond 10 units
 *   src/shaders/generate_work.comp:61-67          command header fields
 *   src/shaders/compact_draw_stream.comp:34-63    stream compaction + count
 *
 * The reference has no plugin API for this path; the boundary follows the one
 * FFI precedent in the repository, the `vma` crate (vma/src/lib.rs:31-64,
 * src/renderer/device/alloc.rs:192-226): opaque handle, plain #[repr(C)] POD
 * parameter structs, integer status returns (0 = success), out-pointers,
 * explicit create/destroy, no callbacks, nothing unwinds across the boundary.
 *
 * Every entry point is `extern "C"`, takes plain pointers and sizes, and is
 * implemented only by the HIP path: there is no CPU backend behind this ABI.
 * Without a usable gfx950 device mip_create fails with MIP_ERR_NO_DEVICE.
 */
#ifndef MI_INSTANCE_PIPELINE_H
#define MI_INSTANCE_PIPELINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIP_ABI_VERSION 4u

/* ---- status codes (0 = success, negative = error; like VkResult in vma) ---- */
#define MIP_OK 0
#define MIP_ERR_INVALID_ARGUMENT (-1) /* NULL pointer, bad size, mesh id out of range ... */
#define MIP_ERR_NO_DEVICE (-2)        /* no HIP device / not gfx950 / ordinal out of range */
#define MIP_ERR_OUT_OF_MEMORY (-3)    /* hipMalloc failed */
#define MIP_ERR_CAPACITY (-4)         /* more instances / meshes than the context was created for */
#define MIP_ERR_DEVICE (-5)           /* a HIP runtime call failed; see mip_last_error */
#define MIP_ERR_NOT_READY (-6)        /* run before instances / mesh table were set */
#define MIP_ERR_TIMEOUT (-7)          /* a stream-ordered wait for an EXTERNAL semaphore expired (10 s; mip_wait_external). No kernel
                                       * of this library waits for another workgroup to run — a tile whose predecessor has not
                                       * published computes that predecessor's aggregate itself (MipTimings.prefix_helps) — so
                                       * a frame cannot time out, whatever order the hardware starts workgroups in and
                                       * whatever else shares the GPU. (ABI <= 3 reported expired in-kernel waits here.) */

/* ---- MipConfig.flags ---- */
#define MIP_CFG_TIMING 0x1u /* bracket every kernel with hipEvents (mip_get_timings) */
#define MIP_CFG_ORDERED_TILES 0x2u /* accepted and ignored since ABI 4. Up to ABI 3 the default frame kernel relied on the
                                     * hardware starting a launch's workgroups in index order (not guaranteed by HIP, and seen
                                     * to fail when several processes shared one GPU) and this flag selected slower modes that
                                     * did not (tickets: 56 us at 1 M instances; three wait-free launches: 26 us, against 18.5).
                                     * Now EVERY launch is independent of the order workgroups start in: the one-hop look-up of
                                     * a tile's prefix polls a bounded number of times and then computes what is missing itself
                                     * (decoupled look-back with a fallback; renderer_amd/csrc/instance_kernel.hpp). In-order
                                     * dispatch is a performance property only. */

/* ---- MipOutputs.flags ---- */
#define MIP_OUT_HOST 0x0u   /* output pointers are host memory (copied back, synchronous) */
#define MIP_OUT_DEVICE 0x1u /* output pointers are device memory of the context's GPU. The frame runs on the
                              * context's own stream(s) (MipConfig.stream if given): work the caller queued on
                              * OTHER streams for those buffers (a clear, a previous reader) is not waited for —
                              * order it with an event / synchronize, or hand the library that stream */
#define MIP_OUT_ASYNC 0x2u  /* with MIP_OUT_DEVICE: return after enqueue; pair with mip_wait */
#define MIP_OUT_WIRE 0x4u   /* with MIP_OUT_DEVICE and a 16-BYTE ALIGNED draw_cmds: it receives the list in the WIRE form below (8.06 B per
                              * command instead of 20) — what a rank sends through the all-gather; draw_count and
                              * draw_index_total as usual. Not with culled_index_buffer (the wire form carries no
                              * indexCount: it is the mesh table's). mip_merge_wire_lists expands it again. */
#define MIP_OUT_WIRE_PACKED 0x8u /* with MIP_OUT_WIRE: the PACKED wire form below, 4.25 B per command — one 32-bit record
                              * {instance index in the frame | mesh_id << index_bits | lod << 31}. Only while the
                              * context's instance count fits: n <= 1 << mip_wire_index_bits(n_meshes), else
                              * MIP_ERR_INVALID_ARGUMENT. mip_merge_wire_lists_packed expands it. */

/* Largest LOD chain the scene loader can produce: LOD0 + 5 simplified levels
 * (src/renderer/systems/scene_loader.rs:740-753). */
#define MIP_MAX_LODS 6u
#define MIP_MAX_FRAMES_IN_FLIGHT 8u

typedef struct MipContext MipContext; /* opaque; Send + Sync like VmaAllocator */

typedef struct MipConfig {
  uint32_t struct_size;   /* = sizeof(MipConfig); guards ABI drift */
  int32_t device_ordinal; /* HIP device index of this process' GPU */
  uint32_t max_instances; /* capacity; the reference's is 4096 (generate_work.comp:25-27) */
  uint32_t max_meshes;    /* capacity of the mesh table */
  uint32_t flags;         /* MIP_CFG_* */
  /* Frames the caller keeps in flight (0 or 1 = one): each gets its own stream and its own
   * cross-tile prefix state inside the context, and consecutive mip_run calls rotate over
   * them, so frame k+1 may start on the device while frame k drains — what the reference's
   * per-swapchain-image buffers (DoubleBuffered<..>, src/renderer.rs:1225-1249) allow. The
   * caller must give `frames_in_flight` consecutive async runs distinct output buffers.
   * Needs stream == NULL when > 1. */
  uint32_t frames_in_flight;
  void* stream; /* hipStream_t to enqueue on, or NULL for streams owned by the context */
} MipConfig;

/* One entry per distinct mesh. Stands in for GltfMesh.aabb (src/renderer.rs:125),
 * GltfMesh.index_buffers[lod].1 (index_len) and the ConsolidatedMeshBuffers
 * vertex_offsets / index_offsets lookups (cull_pipeline.rs:540-548). */
typedef struct MipMesh {
  float aabb_min[3]; /* mesh-local box, finite */
  float aabb_max[3];
  uint32_t n_lods;                     /* 1..MIP_MAX_LODS */
  uint32_t index_len[MIP_MAX_LODS];    /* indices in LOD k */
  uint32_t index_offset[MIP_MAX_LODS]; /* offset of LOD k in the consolidated index buffer */
  int32_t vertex_offset;               /* offset in the consolidated vertex buffer */
} MipMesh;

/* Byte-identical to VkDrawIndexedIndirectCommand (generate_work.comp:9-15,
 * asserted against ash's struct at src/renderer.rs:178-185). */
typedef struct MipDrawIndexedIndirectCommand {
  uint32_t indexCount;
  uint32_t instanceCount;
  uint32_t firstIndex;
  int32_t vertexOffset;
  uint32_t firstInstance;
} MipDrawIndexedIndirectCommand;

/* Per-frame inputs. Everything else is resident on the device. */
typedef struct MipFrame {
  /* Camera.frustum_planes (src/ecs/camera_controller.rs:15-16): 6 x (nx,ny,nz,d),
   * order left,right,bottom,top,near,far, outward-facing, not normalised
   * (src/ecs.rs:83-90). Produced on the host by project_camera. */
  float planes[24];
  float cam_pos[3];           /* Camera.position, for pick_lod */
  uint32_t first_instance_base; /* added to firstInstance: draw_index of instance 0 of this shard */
  uint32_t first_index_base;    /* added to firstIndex (wrapping u32) */
  /* CameraMatrices.pv = projection * view, column-major (generate_work.comp:29-34). Only read
   * when MipOutputs.culled_index_buffer is set (per-triangle culling). */
  float pv[16];
} MipFrame;

typedef struct MipOutputs {
  /* N x mat4, column-major, 64 B each: the `mat4 model[]` storage buffer
   * (ModelData.model_buffer, src/renderer.rs:1225-1249). May be NULL. */
  void* model;
  /* ceil(N/32) words; bit (i & 31) of word (i >> 5) = !CoarseCulled[i]. May be NULL. */
  uint32_t* visible_bitmap;
  /* Up to N MipDrawIndexedIndirectCommand, compacted, ascending draw_index
   * (IndirectCommandsBuffer). Entries past *draw_count are left untouched. May be NULL
   * only together with draw_count. */
  void* draw_cmds;
  uint32_t* draw_count; /* IndirectCommandsCount.count */
  /* Optional: Σ indexCount over the emitted commands (wrapping u32) = the firstIndex the
   * next appended command would get, relative to first_index_base. Needed when shards
   * of one scene are merged (mip_merge_draw_lists). May be NULL. */
  uint32_t* draw_index_total;
  /* Optional: N x {mins[3], maxs[3]} world AABB as the ECS `AABB` component holds it
   * (src/ecs/components.rs:18-20). May be NULL. Identical to the reference's values AS NUMBERS; the sign
   * of a coordinate that is exactly zero is not specified (the kernel folds the box without enumerating
   * the corners where that is exact — a zero may come out as +0 where the corner loop gives -0 — and which
   * arithmetic tier runs depends on the other instances of the scene). Visibility does not depend on it. */
  void* world_aabb;
  uint32_t flags; /* MIP_OUT_* */
  uint32_t reserved;
  /* Optional (needs MIP_OUT_DEVICE, mip_set_geometry, model and draw_cmds): the culled index
   * stream `uvec3 out_index_buffer[]` (CulledIndexBuffer, generate_work.comp:40-42). When set,
   * every emitted command's triangles go through the per-triangle back-face + x/y frustum test
   * of generate_work.comp:68-200; survivors are appended, in mesh order, at
   * culled_index_buffer[firstIndex ...]; indexCount becomes 3 x survivors and commands without
   * survivors are dropped by the compaction that follows (compact_draw_stream.comp runs after
   * generate_work). firstIndex keeps the reference's layout: the running sum of the full
   * index_len of the earlier commands. */
  void* culled_index_buffer;
  /* Size of culled_index_buffer in indices (u32). Any value is legal, 0 included. When the range
   * [firstIndex, firstIndex + indexCount) of an emitted command (its FULL index count, before the
   * per-triangle test) does not fit:
   *  - the call (mip_wait, for an asynchronous frame) returns MIP_ERR_CAPACITY;
   *  - no word at or behind culled_index_capacity is written;
   *  - the commands that fit keep their bytes and their part of the stream, as if the buffer were
   *    large enough;
   *  - a command that does not fit writes nothing, not even in front of the capacity, and is
   *    absent from the compacted list ("its triangles were dropped"); draw_count counts the
   *    commands that are there, draw_index_total keeps the frame's value;
   *  - the context stays usable: the next frame with a buffer that fits is complete. */
  uint64_t culled_index_capacity;
  /* Optional (needs MIP_OUT_DEVICE): N x VkAccelerationStructureInstanceKHR (64 B), one per
   * instance in draw_index order, as build_acceleration_structures fills them
   * (src/renderer/systems/acceleration_strucures.rs:419-451): transform = rows 0..2 of the model
   * matrix (row-major 3x4), instanceCustomIndex = draw_index, mask = 0xFF, sbt offset 0,
   * flags = TRIANGLE_FACING_CULL_DISABLE, accelerationStructureReference = the mesh's BLAS
   * address (mip_set_blas_addresses; 0 if never set). */
  void* tlas_instances;
} MipOutputs;

typedef struct MipTimings {
  uint64_t runs;              /* mip_run calls timed since create / last reset */
  double last_kernel_ms;      /* hipEvent time of the pipeline kernel of the last run */
  double total_kernel_ms;     /* sum over `runs` */
  double last_merge_ms;       /* same for mip_merge_draw_lists */
  double total_merge_ms;
  uint64_t merges;
  uint64_t graph_frames;      /* frames mip_run_many replayed from recorded launch graphs (counted even without MIP_CFG_TIMING) */
  uint64_t graph_records;     /* times it had to record a new set of graphs */
  uint64_t sharded_retries;   /* sharded frames whose tightened chunk overflowed and were re-gathered at full capacity */
  uint64_t sharded_bytes_sent; /* bytes this rank contributed to the last sharded frame's all-gather */
  uint64_t prefix_helps;      /* tile aggregates a WAITING tile computed itself because their owner had not published within the
                                 patient polls (see MIP_ERR_TIMEOUT): 0 on a GPU this context has to itself; non-zero means the
                                 hardware started workgroups out of order or another tenant held compute units — results are
                                 the same either way. Cumulative since create / mip_reset_timings */
  uint64_t general_launches;  /* frames launched with the kernel that carries the literal path for non-finite
                                 inputs (some resident instance failed the upload-time finite test, or a skinned frame) */
  uint64_t reserved0;         /* (ABI 3: timeout_recoveries) */
} MipTimings;

/* Chunk header used by mip_merge_draw_lists: what each rank contributes to the
 * all-gather in front of its commands. 32 B so the commands stay 16-B aligned. */
typedef struct MipShardHeader {
  uint32_t draw_count;
  uint32_t draw_index_total;
  uint32_t reserved[6];
} MipShardHeader;

/* ---- wire form of a shard's draw list (MIP_OUT_WIRE, mip_merge_wire_lists) ---------------------
 * An emitted command of cull_pass (cull_pipeline.rs:534-577) is determined by its draw_index, its
 * mesh, the LOD picked and its position in the running index sum: indexCount = index_len[lod] and
 * vertexOffset come from the mesh table every rank holds, instanceCount is 1 (generate_work.comp:63).
 * The wire form therefore carries per command the 8-byte record
 *     { firstInstance, mesh_id | lod << 31 }            lod = 0 or 1 (pick_lod, helpers.rs:3-11)
 * in blocks of MIP_WIRE_BLOCK_COMMANDS records, each block behind a 16-byte block header of FOUR
 * words: word q is the firstIndex of the block's record MIP_WIRE_SUB_BLOCK_COMMANDS * q (relative to
 * the shard, plus the frame's first_index_base, as the 20-byte form has it; a word whose record does
 * not exist is unspecified). The firstIndex of the other records is their anchor plus the index_len of
 * the records between the anchor and them. (ABI <= 3 anchored only record 0 of a block; 64-record
 * sub-blocks let one wave of the merge kernel expand its share without talking to the others.)
 * Block b of a list lives at byte b * MIP_WIRE_BLOCK_BYTES of the body; a list cut after any whole
 * number of blocks is a valid shorter list, which is what lets a rank send a tightened slice of it. */
#define MIP_WIRE_BLOCK_COMMANDS 256u
#define MIP_WIRE_SUB_BLOCK_COMMANDS 64u
#define MIP_WIRE_BLOCK_HEADER_BYTES 16u
#define MIP_WIRE_RECORD_BYTES 8u
#define MIP_WIRE_BLOCK_BYTES (MIP_WIRE_BLOCK_HEADER_BYTES + MIP_WIRE_BLOCK_COMMANDS * MIP_WIRE_RECORD_BYTES) /* 2064 */
/* bytes of the body of a wire list with room for `capacity` commands (whole blocks) */
#define MIP_WIRE_BODY_BYTES(capacity) \
  ((((uint64_t)(capacity) + MIP_WIRE_BLOCK_COMMANDS - 1u) / MIP_WIRE_BLOCK_COMMANDS) * MIP_WIRE_BLOCK_BYTES)
/* The PACKED wire form (MIP_OUT_WIRE | MIP_OUT_WIRE_PACKED): ONE 32-bit record per command,
 *     instance_index | mesh_id << index_bits | lod << 31,      instance_index = firstInstance - first_instance_base,
 * in blocks of MIP_WIRE_PACKED_BLOCK_COMMANDS = 64 records, each behind a self-describing 16-byte header
 * {firstIndex of the block's first command, the frame's first_instance_base, index_bits, 0}: 4.25 B per command.
 * index_bits = mip_wire_index_bits(n_meshes) = 31 - ceil(log2(n_meshes)) is what the mesh ids leave of the word, so the
 * form exists for frames of at most 1 << index_bits instances (64 meshes: 33 M; 1 024 meshes: 2 M) — every rank of an
 * exchange derives the same answer from the replicated mesh table and the largest shard. */
#define MIP_WIRE_PACKED_RECORD_BYTES 4u
#define MIP_WIRE_PACKED_BLOCK_COMMANDS 64u
#define MIP_WIRE_PACKED_BLOCK_BYTES (MIP_WIRE_BLOCK_HEADER_BYTES + MIP_WIRE_PACKED_BLOCK_COMMANDS * MIP_WIRE_PACKED_RECORD_BYTES) /* 272 */
#define MIP_WIRE_PACKED_BODY_BYTES(capacity) \
  ((((uint64_t)(capacity) + MIP_WIRE_PACKED_BLOCK_COMMANDS - 1u) / MIP_WIRE_PACKED_BLOCK_COMMANDS) * MIP_WIRE_PACKED_BLOCK_BYTES)
/* bits of a packed record left for the instance index by a mesh table of n_meshes entries (pure function) */
uint32_t mip_wire_index_bits(uint32_t n_meshes);

uint32_t mip_abi_version(void);

/* Create a context on cfg->device_ordinal. Allocates device storage for
 * max_instances / max_meshes. Returns MIP_OK and writes *out, or a negative code
 * (then *out = NULL). Never aborts. */
int32_t mip_create(const MipConfig* cfg, MipContext** out);

/* Frees everything the context owns. NULL is a no-op. */
void mip_destroy(MipContext* ctx);

/* Copy the mesh table to the device (caller keeps its memory). m <= max_meshes.
 * Bounds must be finite and n_lods in 1..MIP_MAX_LODS. If the table is smaller than the one it replaces and a
 * resident instance names a mesh outside it, the instances stop being resident (upload the new scene's
 * next; a frame before that fails with MIP_ERR_NOT_READY): the kernels never gather outside the table.
 * The BLAS addresses belong to the table they were set for: every call CLEARS them (all max_meshes entries, before it
 * returns). MipOutputs.tlas_instances then carries accelerationStructureReference 0 — what it carries while no address
 * was ever set — until mip_set_blas_addresses is called for the new table. */
int32_t mip_set_mesh_table(MipContext* ctx, const MipMesh* meshes, uint32_t m);

/* Upload the instance columns: SoA, tightly packed, draw_index = array index
 * (assign_draw_index for a single-archetype static scene, src/ecs.rs:117-136).
 *   pos_xyz  n x 3 floats   Position(Point3<f32>)
 *   rot_ijkw n x 4 floats   Rotation(UnitQuaternion<f32>), stored [i,j,k,w]; NOT renormalised
 *   scale    n floats       Scale(f32)
 *   mesh_id  n u32          index into the mesh table; every id must be < m
 * Host pointers; copied. Static scenes call this once. n may be 0. */
int32_t mip_set_instances(MipContext* ctx, const float* pos_xyz, const float* rot_ijkw,
                          const float* scale, const uint32_t* mesh_id, uint32_t n);

/* Overwrite a range [first, first + count) of the resident columns (moving entities: the
 * Changed<Position|Rotation|Scale> filter of a bevy query). A NULL column is left as it is.
 * The instance count does not change; first + count must not exceed it. Host pointers; copied
 * after everything in flight has drained. */
int32_t mip_update_instances(MipContext* ctx, uint32_t first, uint32_t count, const float* pos_xyz,
                             const float* rot_ijkw, const float* scale, const uint32_t* mesh_id);

/* Same, from DEVICE pointers of the context's GPU (device-to-device copies). Mesh ids are checked on the
 * device after the copy (the upload-time census reads every instance anyway): an id >= m fails the call with
 * MIP_ERR_INVALID_ARGUMENT and leaves NO instances resident. */
int32_t mip_set_instances_device(MipContext* ctx, const void* pos_xyz, const void* rot_ijkw,
                                 const void* scale, const void* mesh_id, uint32_t n);

/* Per-mesh bottom-level acceleration structure device addresses for MipOutputs.tlas_instances
 * (vkGetAccelerationStructureDeviceAddressKHR per GltfMesh, acceleration_strucures.rs:430-437).
 * m must equal the mesh table's size. Host pointer; copied. Call it AFTER mip_set_mesh_table, and again after every later
 * mip_set_mesh_table: replacing the table clears the addresses (reference 0), whatever the new table's size or contents. */
int32_t mip_set_blas_addresses(MipContext* ctx, const uint64_t* addresses, uint32_t m);

/* Upload the consolidated geometry the per-triangle stage reads (ConsolidatedMeshBuffers'
 * position_buffer and index_buffer, consolidate_mesh_buffers.rs): packed vec3 positions and
 * u32 indices; MipMesh.vertex_offset / index_offset[] index into them. Host pointers; copied. */
int32_t mip_set_geometry(MipContext* ctx, const float* vertex_xyz, uint32_t n_vertices,
                         const uint32_t* indices, uint32_t n_indices);


/* One frame: model matrices, world AABBs, visibility, compacted draw commands.
 * Call from one thread at a time per context. Synchronous on return unless
 * MIP_OUT_ASYNC.
 * Every output pointer of `out` is optional and independent of the others, except that draw_cmds and draw_count go
 * together and draw_index_total needs them; a NULL output is not computed-and-dropped into anything, it is not written.
 * With EVERY pointer NULL the call is valid: it returns MIP_OK, writes nothing (the frame's kernel still runs over the
 * resident instances and stores nothing; it takes no prefix tag) and leaves the context usable — the next frame is what it
 * would have been without it. With no resident instances (n = 0) nothing is launched: draw_count (and draw_index_total)
 * are zeroed, nothing else is touched. */
int32_t mip_run(MipContext* ctx, const MipFrame* frame, const MipOutputs* out);

/* Enqueue `steps` frames back to back from compiled code — the renderer's 'frame: loop
 * (src/main.rs:907-926), in which project_camera (src/ecs.rs:66-91) produces new planes every frame:
 * step k runs frames[k % n_frames] into outputs[k % n_outputs] (give at least frames_in_flight
 * output sets). Every output set must carry MIP_OUT_DEVICE | MIP_OUT_ASYNC. Equivalent to calling
 * mip_run `steps` times; exists so that a host in a scripting language does not pay its per-call
 * overhead per frame, and so that the launches can be recorded once and replayed: when every
 * output set asks for draw commands and none for the per-triangle stage, whole rounds of ~64 frames
 * go out as one hipGraph per frame slot. The graphs are recorded on first use and cached by the
 * OUTPUT sets only — a frame's planes, camera position and bases are not baked into them (each
 * recorded launch reads its frame from a small device-side ring that one copy refreshes per
 * replay), so a moving camera replays the same graphs (MipTimings.graph_records stays put,
 * graph_frames counts the replayed frames); the remainder and every other case are plain mip_run
 * calls. */
int32_t mip_run_many(MipContext* ctx, const MipFrame* frames, uint32_t n_frames, const MipOutputs* outputs,
                     uint32_t n_outputs, uint32_t steps);

/* Row f-4, second consumer — the shadow pass's per-light draw lists
 * (src/renderer/systems/shadow_mapping.rs:405-478: for every light, for every mesh entity,
 * pick_lod(index_buffers, light_position, mesh_position) and cmd_draw_indexed(index_count, 1,
 * 0, 0, draw_index); nothing is culled). For light l and resident instance i
 *   out_cmds[l*n + i] = { index_len[lod], 1, index_offset[lod], vertex_offset,
 *                         first_instance_base + i }
 * over the consolidated buffers (as cull_pass addresses them, cull_pipeline.rs:540-553), so the
 * shadow pass becomes one vkCmdDrawIndexedIndirect(buffer, l*n*20, n, 20) per light.
 * light_pos_xyz: n_lights x 3 host floats, 1 <= n_lights <= MIP_MAX_LIGHTS (the 4x4 shadow atlas,
 * shadow_mapping.rs:24). out_cmds: DEVICE pointer, n_lights * n * 20 bytes. async != 0: returns
 * after enqueueing on the context's stream (mip_wait to finish). */
#define MIP_MAX_LIGHTS 16
int32_t mip_light_draw_lists(MipContext* ctx, const float* light_pos_xyz, uint32_t n_lights,
                             uint32_t first_instance_base, void* out_cmds, int32_t async);

/* ---- Extension: skinned instances (BASELINE config 5) ----------------------------------------
 * NOT a reference behaviour: farnoy/renderer has no skins, joints or animation (SURVEY.md
 * section 8, top table). Specified from glTF 2.0 section 3.7.3 and checked against this repository's
 * oracle, which is itself pinned to a float64 evaluation of that definition within a derived float32
 * rounding bound (tests/float64_reference.py, skinned_reference). One skeleton per context, shared by
 * every instance:
 *   parent[k]        index of the parent joint, < k, or -1 (parents precede children)
 *   inverse_bind     n_joints x 16 floats, column-major mat4 (skin.inverseBindMatrices; rows 0..2 used)
 *   joint_box        n_joints x 6 floats: min xyz, max xyz of the bind-pose vertices weighted to
 *                    joint k, in mesh space (min > max: the joint binds no vertex)
 * 1 <= n_joints <= MIP_MAX_JOINTS. Host pointers; copied. */
#define MIP_MAX_JOINTS 32
#define MIP_POSE_FLOATS 10 /* per joint: translation xyz, rotation quaternion ijkw, scale xyz (the LOCAL TRS) */
int32_t mip_set_skeleton(MipContext* ctx, const int32_t* parent, const float* inverse_bind,
                         const float* joint_box, uint32_t n_joints);

/* The animated pose of every instance: n x n_joints x MIP_POSE_FLOATS floats, instance-major.
 * n must equal the resident instance count. device == 0: host pointer, copied (waits for the frames in
 * flight). device != 0: a DEVICE pointer (8-byte aligned) that is borrowed, not copied; the call does not
 * wait for anything — frames already queued keep the pointer they were launched with, so an animation
 * system can alternate two buffers with frames_in_flight = 2. It keeps each buffer alive and unmodified
 * while a frame that reads it is in flight. A device pointer that is not 8-byte aligned is refused with
 * MIP_ERR_INVALID_ARGUMENT. */
int32_t mip_set_poses(MipContext* ctx, const void* joint_trs, uint32_t n, int32_t device);

/* One frame of skinned instances. Per instance and joint
 *   L_k = T*R*S of the pose, G_k = G_parent * L_k, J_k = G_k * inverse_bind_k   (affine, fp32)
 * the palette (n x n_joints mat4, column-major, DEVICE pointer, may be NULL) receives J_k. It must be
 * 16-byte aligned (it is written in 16-byte stores); one that is not is refused with
 * MIP_ERR_INVALID_ARGUMENT before anything is enqueued. The
 * union over joints of J_k * joint_box_k (8 corners each) is the instance's posed box in mesh
 * space; it takes the place of the mesh table's aabb for that instance, and everything else —
 * model[], world box, frustum test, bitmap, draw commands, count, TLAS rows — is produced from
 * it exactly as mip_run does from GltfMesh.aabb. out must carry MIP_OUT_DEVICE;
 * culled_index_buffer is not supported (the per-triangle stage does not skin vertices). */
int32_t mip_run_skinned(MipContext* ctx, const MipFrame* frame, const MipOutputs* out, void* palette);

/* Several views of the resident instances in ONE launch — per-light culled draw lists (the shadow pass
 * with a frustum per light), cascades, cube faces, stereo. View v is a complete cull_pass with
 * frames[v]'s planes, LOD reference point (cam_pos) and bases, and gives exactly what mip_run would give
 * for that frame: outs[v].visible_bitmap (optional), outs[v].draw_cmds + draw_count (required),
 * outs[v].draw_index_total (optional). The instance data is read once and the model matrix / world box
 * built once for all views; nothing view-independent is written, so model, world_aabb, tlas_instances
 * and culled_index_buffer must be NULL (run the frame's mip_run for those). 1 <= n_views <=
 * MIP_MAX_VIEWS (the 4 x 4 shadow atlas, shadow_mapping.rs:24); four views share a launch, more views
 * are further launches on the same stream. Every output set carries MIP_OUT_DEVICE; the call is
 * asynchronous if outs[0] carries MIP_OUT_ASYNC. Runs on the context's first stream. */
#define MIP_MAX_VIEWS 16
int32_t mip_run_views(MipContext* ctx, const MipFrame* frames, const MipOutputs* outs, uint32_t n_views);

/* ---- Extension: occlusion culling against a depth pyramid (Hi-Z), one and two phases -----------------
 * NOT a reference behaviour: farnoy/renderer renders a depth prepass (DepthRT: D16_UNORM, cleared to 1.0,
 * compare LESS_OR_EQUAL, viewport flipped to y = H, height = -H; src/renderer/systems/depth_pass.rs) but
 * culls nothing against it. Specified here and checked against this repository's own restatement
 * (tests/occlusion_restatement.py) only.
 *
 * PYRAMID (mip_build_depth_pyramid): f32, row-major, levels one after another, level 0 first. Level 0 is
 * ceil(W/2) x ceil(H/2); level k+1 is ceil of half of level k, down to 1 x 1. Texel (x, y) of level k is
 * the max of the depth pixels (px, py) with px >> (k+1) == x and py >> (k+1) == y. A u16 value v counts
 * as (float)v / 65535.0f (correctly rounded), a NaN f32 pixel as 1.0f, and a zero texel is +0.0f: max is
 * exact, so the pyramid is bit-exact whatever the reduction order. mip_depth_pyramid_bytes gives its size.
 * `depth` and `pyramid` are DEVICE pointers of the context's GPU; row_pitch_bytes is a multiple of the
 * element size and at least W of them. The build is enqueued on the stream of the frame slot the context's
 * next mip_run / mip_run_occluded will use, so that run is ordered after it without a wait. async == 0:
 * returns when the pyramid is complete.
 *
 * OCCLUSION TEST (evaluated with contraction off). An instance is OCCLUDED when it passes the frustum
 * test, is a candidate (its bit in `candidates` is set, or clear under MIP_OCC_CANDIDATES_INVERTED; every
 * instance when `candidates` is NULL, which INVERTED does not go with) and fails this test:
 *   1. corner c (0..7) of its world AABB (what world_aabb receives) takes max on x if c&1, on y if c&2, on z if c&4;
 *   2. clip = ((m0*x + m4*y) + m8*z) + m12 per row, m = pv;
 *   3. any clip coordinate non-finite, or any w <= 0: NOT occluded;
 *   4. r = 1.0f / w (correctly rounded), ndc = clip.xyz * r;
 *   5. u = (ndc.x*0.5f + 0.5f) * W, v = (0.5f - ndc.y*0.5f) * H   (the flipped viewport);
 *   6. x0..x1 = floor(min u), floor(max u) over the corners clamped to [0, W-1], y0..y1 the same on v, H; min and max
 *      are fminf / fmaxf folds from +inf / -inf, so a NaN u or v (0 * inf, where w is so small that r overflows) is
 *      ignored and +-inf takes the clamp; if every corner's is NaN the start values stand: x0 = W-1, x1 = 0;
 *   7. k = the smallest level with (x1>>(k+1)) - (x0>>(k+1)) <= 1 and the same for y;
 *   8. d = max of the (at most 4) level-k texels covering the rectangle;
 *   9. occluded iff d < 1.0f and min over corners of ndc.z > d (a texel at 1.0 — cleared — never occludes).
 *
 * mip_run_occluded: every output of MipOutputs is exactly what mip_run gives for the same scene in which
 * every non-candidate and every occluded instance had been frustum-culled — visible_bitmap, draw_cmds /
 * draw_count / draw_index_total (firstIndex sums what is emitted), culled_index_buffer (the per-triangle
 * stage runs over the emitted list); model, world_aabb and tlas_instances are written for every instance.
 * occluded_bitmap (optional) bit i is set iff instance i passed the frustum test, was a candidate and is
 * occluded. `candidates` and `occluded_bitmap` need MIP_OUT_DEVICE. Not with MIP_OUT_WIRE; skinned
 * instances, views, shards and mip_run_many are out of scope.
 *
 * TWO PHASES, composed by the caller:
 *   phase 1  candidates = last frame's visible_bitmap, pyramid = last frame's; draw; rebuild the pyramid
 *            from the new depth (mip_build_depth_pyramid);
 *   phase 2  candidates = phase 1's visible_bitmap with MIP_OCC_CANDIDATES_INVERTED, the new pyramid; draw
 *            with its own draw list and its own culled-index region.
 * The union of the two phases' bitmaps is the next frame's phase-1 candidate set. */
#define MIP_DEPTH_UNORM16 0u /* D16_UNORM, the reference's DepthRT */
#define MIP_DEPTH_FLOAT32 1u /* D32_SFLOAT */
#define MIP_MAX_DEPTH_EXTENT 16384u
#define MIP_OCC_CANDIDATES_INVERTED 0x1u

/* Bytes of the pyramid of a W x H depth image (pure, no device); 0 if a side is 0 or above MIP_MAX_DEPTH_EXTENT. */
uint64_t mip_depth_pyramid_bytes(uint32_t width, uint32_t height);
int32_t mip_build_depth_pyramid(MipContext* ctx, const void* depth, uint32_t width, uint32_t height,
                                uint32_t row_pitch_bytes, uint32_t format, void* pyramid, int32_t async);

typedef struct MipOcclusion {
  uint32_t struct_size;         /* = sizeof(MipOcclusion) */
  uint32_t width, height;       /* of the depth image the pyramid was built from */
  uint32_t flags;               /* MIP_OCC_* */
  const void* pyramid;          /* DEVICE, built by mip_build_depth_pyramid */
  const uint32_t* candidates;   /* optional DEVICE bitmap, ceil(N/32) words; NULL = every instance */
  uint32_t* occluded_bitmap;    /* optional DEVICE output, ceil(N/32) words */
  float pv[16];                 /* projection * view the depth was rendered with, column-major */
} MipOcclusion;                 /* 104 B */

int32_t mip_run_occluded(MipContext* ctx, const MipFrame* frame, const MipOcclusion* occ, const MipOutputs* out);

/* ---- Extension: batched draws — one instanced command per (mesh, LOD), built on the device -------------------
 * NOT a reference behaviour: farnoy/renderer issues one VkDrawIndexedIndirectCommand with instanceCount = 1 per visible
 * entity (generate_work.comp:61-67). Specified here and checked against this repository's own restatement
 * (tests/batch_restatement.py) only. Everything but batch_model is integer, so every byte is determined.
 *
 * MEMBERS: resident instance i < N is a member iff bit i of `visible_bitmap` (DEVICE, ceil(N/32) words, the layout of
 * MipOutputs.visible_bitmap; bits at or above N are ignored) is set AND index_len[lod_i] > 0, where lod_i is what pick_lod
 * gives for frame->cam_pos and the instance's position, exactly as the frame kernel evaluates it (0 or 1; 0 for a mesh with
 * one LOD). With the bitmap of a mip_run of the same frame the members are exactly the firstInstance values of that run's
 * compacted list.
 * BUCKET of a member: mesh_id * 2 + lod; buckets are ordered ascending (mesh-major).
 * SLOTS: the members sorted by (bucket, draw index) — a stable binning. instance_ids[s] = frame->first_instance_base + i for
 * the member in slot s; slots [0, members) are written, nothing at or behind `members` is touched.
 * COMMANDS: one per NON-EMPTY bucket, in ascending bucket order, packed from entry 0:
 *   indexCount = index_len[lod], instanceCount = members of the bucket, firstIndex = index_offset[lod] (the mesh's own range
 *   of the consolidated index buffer: these draws read the source meshes, not a culled stream), vertexOffset =
 *   vertex_offset, firstInstance = the slot of the bucket's first member.
 * Entries at or behind *batch_count are not touched. batch_cmds needs room for min(2 m, N) commands (m = meshes in the table).
 * batch_model (optional): slot s receives exactly the 64 bytes mip_run's `model` output holds for the instance in slot s,
 * non-finite inputs included; no `model` output of any frame is needed for it. Slots at or behind `members` are not touched.
 * A consumer's vertex shader reads entity_id = instance_ids[gl_InstanceIndex] (or, needing only the matrix, model =
 * batch_model[gl_InstanceIndex]) under vkCmdDrawIndexedIndirectCount(batch_cmds, batch_count).
 * frame->planes, first_index_base and pv are not read. N = 0 is legal and writes two zeros.
 *
 * ORDERING: enqueued on the stream of the frame slot the context's most recent mip_run / mip_run_occluded / mip_run_skinned
 * used, so a bitmap that frame writes needs no wait in between. A bitmap from anywhere else — a view of mip_run_views, an OR of
 * two occlusion phases made by the caller, an earlier frame of another slot — needs mip_wait or the caller's own ordering
 * first. Without MIP_OUT_ASYNC the call returns when the outputs are complete. Scratch is per frame slot, so calls behind
 * different frames in flight do not disturb each other; give each its own outputs.
 * ERRORS: NULL ctx / frame / bitmap / batch_cmds / batch_count / instance_ids, a wrong struct_size, a missing MIP_OUT_DEVICE,
 * unknown flags: MIP_ERR_INVALID_ARGUMENT; no instances or no mesh table: MIP_ERR_NOT_READY.
 * OUT OF SCOPE: per-triangle culling of batched draws (culled_index_buffer addresses a per-instance region), mip_run_many /
 * recorded launch graphs, the wire forms. The batches of several shards are merged by mip_batch_draws_shard +
 * mip_merge_batches (below), for mip_batch_draws_lods' buckets and draw order. */
typedef struct MipBatchOutputs {
  uint32_t struct_size;      /* = sizeof(MipBatchOutputs) */
  uint32_t flags;            /* MIP_OUT_DEVICE (required) | MIP_OUT_ASYNC */
  void* batch_cmds;          /* DEVICE: room for min(2 * m, N) MipDrawIndexedIndirectCommand */
  uint32_t* batch_count;     /* DEVICE: number of commands written */
  uint32_t* instance_ids;    /* DEVICE: room for N words; slots [0, members) are written */
  uint32_t* instance_count;  /* DEVICE, optional: members */
  void* batch_model;         /* DEVICE, optional, 16-byte aligned: room for N x 64 B */
} MipBatchOutputs;           /* 48 B */

int32_t mip_batch_draws(MipContext* ctx, const MipFrame* frame, const uint32_t* visible_bitmap, const MipBatchOutputs* out);

/* ---- Extension: batched draws over the whole LOD chain, with a selection rule the caller tunes --------------------
 * mip_batch_draws with every level of MipMesh (up to MIP_MAX_LODS) and a caller's thresholds in pick_lod's place. NOT a
 * reference behaviour; checked against this repository's restatement (tests/lod_restatement.py), byte for byte.
 * The per-instance lists of mip_run, mip_run_views, mip_run_occluded and the wire forms keep pick_lod (LOD 0 or 1), so a
 * frame's own draw list and these batches agree on members only under the pin policy below, not on LOD in general.
 *
 * SELECTION, per instance, in float32 with contraction off, every product and sum rounded once:
 *   d = cam_pos - pos (per component; cam_pos is frame->cam_pos)
 *   q = (d.x*d.x + d.y*d.y) + d.z*d.z                                  (the expression pick_lod's test evaluates)
 *   MIP_LOD_DISTANCE:  b_k = switch_sq[k]
 *   MIP_LOD_RELATIVE:  e = aabb_max - aabb_min of the instance's mesh (per component)
 *                      diag_sq = (e.x*e.x + e.y*e.y) + e.z*e.z
 *                      b_k = switch_sq[k] * ((scale*scale) * diag_sq)
 *   lod = #{ k in [0, n_lods - 1) : q > b_k }
 * lod is a COUNT, not a walk that stops at the first failure. A NaN on either side of a comparison counts as false, so a NaN
 * position or scale selects LOD 0 (as pick_lod does); q = +inf selects the last LOD whose b_k is finite. A mesh with n_lods
 * levels never selects a level at or above n_lods. No square root and no division: every decision can be reproduced bit for
 * bit. switch_sq holds SQUARED metrics: squared distances (DISTANCE), or squared distances in diagonals of the instance's
 * scaled mesh box (RELATIVE).
 * THRESHOLDS: every switch_sq[k] is >= 0 and not NaN, and the five are non-decreasing; +inf is legal and means "never".
 * Anything else is MIP_ERR_INVALID_ARGUMENT.
 * PIN: with mode = MIP_LOD_DISTANCE and switch_sq = {100.00000762939453125f, +inf, +inf, +inf, +inf} (the first value is
 * nextafter(100): sqrt(q) > 10 exactly when q exceeds it) every output is byte-identical to mip_batch_draws on any mesh table.
 *
 * MEMBERS: as mip_batch_draws — bit i of the bitmap is set and index_len[lod_i] > 0 — with lod_i as above.
 * BUCKET of a member: lod_base[mesh_id] + lod, lod_base = the exclusive prefix sum of n_lods over the mesh table; there are
 * B = sum of n_lods buckets, mesh-major, ascending. SLOTS, instance_ids, instance_count, batch_model and the packing of
 * COMMANDS are exactly as mip_batch_draws documents, with indexCount = index_len[lod] and firstIndex = index_offset[lod] of
 * the bucket's level. batch_cmds needs room for min(B, N) commands.
 * ORDERING, ERRORS and OUT OF SCOPE are mip_batch_draws's; a NULL policy, a wrong MipLodPolicy.struct_size and an unknown
 * mode are MIP_ERR_INVALID_ARGUMENT as well. A refused call writes nothing. */
#define MIP_LOD_DISTANCE 0u  /* metric = squared distance from frame->cam_pos to the instance position */
#define MIP_LOD_RELATIVE 1u  /* the same, measured in diagonals of the instance's scaled mesh box */
typedef struct MipLodPolicy {
  uint32_t struct_size;                 /* = sizeof(MipLodPolicy), 28 */
  uint32_t mode;                        /* MIP_LOD_* */
  float switch_sq[MIP_MAX_LODS - 1];    /* LOD k+1 replaces LOD k beyond this SQUARED metric */
} MipLodPolicy;

int32_t mip_batch_draws_lods(MipContext* ctx, const MipFrame* frame, const uint32_t* visible_bitmap,
                             const MipLodPolicy* policy, const MipBatchOutputs* out);

/* ---- Extension: depth-ordered batched draws ------------------------------------------------------------------------
 * mip_batch_draws_lods with a chosen order of the members INSIDE every bucket: nearest first (a depth prepass, the depth a
 * two-phase occlusion pyramid is built from) or farthest first (a blended single-mesh layer). NOT a reference behaviour;
 * checked against this repository's restatement (tests/order_restatement.py), byte for byte.
 *
 * MEMBERS, LOD, BUCKET: exactly mip_batch_draws_lods for the same policy: the members, every member's lod and its bucket
 * lod_base[mesh_id] + lod.
 * COMMANDS AND COUNTS: batch_cmds, batch_count and instance_count are, for every order, the bytes mip_batch_draws_lods
 * writes. The order permutes members only inside a bucket's slot range [firstInstance, firstInstance + instanceCount).
 * DEPTH KEY of instance i, in float32 with contraction off:
 *   d = cam_pos - pos (per component; cam_pos is frame->cam_pos)
 *   q = (d.x*d.x + d.y*d.y) + d.z*d.z          (the q of the selection rule above)
 *   K = 0x7F80 if q is NaN, else bits(q) >> 16 (bits: the float's 32-bit pattern)
 * q is a sum of squares and never negative, so K is monotone (non-decreasing) in q and lies in [0, 0x7F80]; 0x7F80 is the
 * K of q = +inf and of a NaN. K keeps the sign, the exponent and 7 mantissa bits of q: a step of K is at most 1/128 in q,
 * about 0.4 % in distance. Members whose q differ by less may share a K.
 *   D = K            MIP_BATCH_ORDER_NEAR_FIRST
 *   D = 0x7F80 - K   MIP_BATCH_ORDER_FAR_FIRST
 *   D = 0            MIP_BATCH_ORDER_DRAW_INDEX
 * SLOTS: the members sorted by (bucket, D, draw index), ascending. Equal D keeps draw order: the sort is stable. A member
 * whose distance is NaN is last in its bucket under NEAR_FIRST (together with q = +inf, in draw order) and first under
 * FAR_FIRST. instance_ids[s] = first_instance_base + the instance of slot s, batch_model[s] = the 64 bytes mip_run's `model`
 * holds for that instance, and nothing at or behind `members` is touched: all as mip_batch_draws documents.
 * MIP_BATCH_ORDER_DRAW_INDEX is mip_batch_draws_lods, byte for byte in every output.
 * CAPACITY: NEAR_FIRST and FAR_FIRST sort a 32-bit key bucket << 16 | D. With B = sum of n_lods > 65 536 buckets the call
 * returns MIP_ERR_CAPACITY and writes nothing. DRAW_INDEX has the limits of mip_batch_draws_lods.
 * ERRORS: an unknown order is MIP_ERR_INVALID_ARGUMENT. Every other error, the ordering on the stream behind the frame issued
 * last, the scratch per frame slot and the out-of-scope list are mip_batch_draws_lods's. A refused call writes nothing.
 * OUT OF SCOPE, besides that list: sharded scenes, mip_run_many and the per-triangle stage. An order ACROSS buckets and a depth
 * along the view direction are mip_batch_draws_sorted's (below). */
#define MIP_BATCH_ORDER_DRAW_INDEX 0u  /* mip_batch_draws_lods, byte for byte */
#define MIP_BATCH_ORDER_NEAR_FIRST 1u
#define MIP_BATCH_ORDER_FAR_FIRST  2u
int32_t mip_batch_draws_ordered(MipContext* ctx, const MipFrame* frame, const uint32_t* visible_bitmap,
                                const MipLodPolicy* policy, uint32_t order, const MipBatchOutputs* out);

/* ---- Extension: globally depth-sorted batched draws ---------------------------------------------------------------------
 * The transparent pass: the members of mip_batch_draws_lods in ONE depth order across all buckets, and one instanced command
 * per maximal RUN of neighbouring slots that draw the same bucket. A scene with several blended meshes is drawn back to front
 * across meshes (FAR_FIRST), or front to back (NEAR_FIRST), by vkCmdDrawIndexedIndirectCount(batch_cmds, batch_count) as the
 * other batches are. NOT a reference behaviour; checked against this repository's restatement (tests/sorted_restatement.py),
 * byte for byte.
 *
 * MEMBERS, LOD, BUCKET: exactly mip_batch_draws_lods for the same ctx, frame, bitmap and policy: the members, every member's
 * lod and its bucket lod_base[mesh_id] + lod. instance_count holds the bytes that call writes.
 * DEPTH KEY of instance i, in float32 with contraction off, every product and sum rounded once:
 *   MIP_DEPTH_RADIAL:    d = cam_pos - pos; q = (d.x*d.x + d.y*d.y) + d.z*d.z          (the q of the selection rule)
 *                        U = 0x7F800000 if q is NaN, else bits(q);                      Umax = 0x7F800000
 *   MIP_DEPTH_VIEW_AXIS: e = pos - cam_pos; z = (e.x*axis.x + e.y*axis.y) + e.z*axis.z  (axis = MipSortPolicy.axis)
 *                        if z is NaN: U = 0xFF800000 (as +inf); otherwise
 *                        u = 0 if z == 0 (either zero), else bits(z)
 *                        U = u ^ 0x80000000 if the sign bit of u is clear, else ~u;     Umax = 0xFF800000
 * U is monotone (non-decreasing) in q and in z; under VIEW_AXIS it lies in [0x007FFFFF (-inf), 0xFF800000 (+inf)]. `axis`
 * need not be a unit vector: z is then the distance times its length. A zero axis gives z = 0 for every finite e.
 *   s = 32 - depth_bits;  K = U >> s
 *   D = K                MIP_BATCH_ORDER_NEAR_FIRST
 *   D = (Umax >> s) - K  MIP_BATCH_ORDER_FAR_FIRST
 * depth_bits = 16 keeps the sign, the exponent and 7 mantissa bits (a step of about 0.4 % in distance under RADIAL), 24 keeps
 * 15 mantissa bits, 32 the whole float. With RADIAL and depth_bits = 16, D is exactly the D of mip_batch_draws_ordered. No D
 * equals 0xFFFFFFFF. A member whose depth is NaN sorts with +inf: last under NEAR_FIRST, first under FAR_FIRST.
 * SLOTS: the members sorted by (D, draw index), ascending. Equal D keeps draw order: the sort is stable. instance_ids[s] =
 * first_instance_base + the instance of slot s; batch_model[s] (optional) = the 64 bytes mip_run's `model` holds for that
 * instance, as mip_batch_draws_ordered stores them. Nothing at or behind `members` is touched.
 * COMMANDS: b(s) is the bucket of the member in slot s. Slot s is a HEAD if s == 0 or b(s) != b(s-1). Command r belongs to the
 * r-th head, in slot order, packed from entry 0: indexCount, firstIndex and vertexOffset are the ones mip_batch_draws_lods
 * writes for bucket b(head); firstInstance = the head's slot; instanceCount = the distance to the next head, or to `members`
 * for the last head. *batch_count = the number of heads. batch_cmds needs room for N commands: a well-mixed scene has nearly
 * as many runs as members. Entries at or behind *batch_count are not touched. N = 0 writes the two zeros.
 * ORDERING, SCRATCH, ERRORS: the stream behind the frame issued last, the scratch per frame slot and the errors are
 * mip_batch_draws_ordered's. Also MIP_ERR_INVALID_ARGUMENT: a NULL sort, a wrong MipSortPolicy.struct_size, an unknown
 * metric, an order other than NEAR_FIRST / FAR_FIRST (DRAW_INDEX is refused: that is mip_batch_draws_lods), depth_bits not in
 * {16, 24, 32}, a non-finite axis component under VIEW_AXIS (RADIAL ignores axis). The bucket is not part of the key, so there
 * is no 65 536-bucket limit: the bucket limits are those of mip_batch_draws_lods. A refused call writes nothing.
 * OUT OF SCOPE: views, shards, mip_run_many and recorded graphs; a command capacity below N with an overflow status; the
 * per-triangle stage. */
#define MIP_DEPTH_RADIAL    0u  /* q, the squared distance the LOD rule forms */
#define MIP_DEPTH_VIEW_AXIS 1u  /* signed distance along a caller's axis */
typedef struct MipSortPolicy {
  uint32_t struct_size;   /* = sizeof(MipSortPolicy), 28 */
  uint32_t metric;        /* MIP_DEPTH_* */
  uint32_t order;         /* MIP_BATCH_ORDER_NEAR_FIRST | MIP_BATCH_ORDER_FAR_FIRST */
  uint32_t depth_bits;    /* 16, 24 or 32: the leading bits of the key that are sorted */
  float axis[3];          /* VIEW_AXIS: the view direction, need not be unit; ignored by RADIAL */
} MipSortPolicy;

int32_t mip_batch_draws_sorted(MipContext* ctx, const MipFrame* frame, const uint32_t* visible_bitmap,
                               const MipLodPolicy* policy, const MipSortPolicy* sort, const MipBatchOutputs* out);

/* ---- Extension: batched draws for several views in one call -----------------------------------------------------------
 * mip_batch_draws_lods for n_views views of the resident instances — the lights of a shadow pass, cascades, cube faces,
 * stereo — in ONE call that reads the instance columns once. NOT a reference behaviour (farnoy/renderer walks every mesh
 * entity once per light, shadow_mapping.rs:405-478); checked against this repository's restatement
 * (tests/views_batch_restatement.py), byte for byte. Every output is integer, so every byte is determined.
 *
 * VIEWS: 1 <= n_views <= MIP_MAX_VIEWS. View v is frames[v] with visible_bitmaps[v]: `visible_bitmaps` is a HOST array of
 * n_views DEVICE pointers, each a bitmap in the layout mip_batch_draws documents; a NULL entry means every resident instance
 * (the unculled shadow pass). Two views may share a bitmap pointer. cam_pos and first_instance_base are per view; the policy
 * is shared; planes, first_index_base and pv are not read.
 * MEMBERS, LOD, BUCKET, per view: exactly those of mip_batch_draws_lods(ctx, &frames[v], visible_bitmaps[v], policy, ...):
 * bucket = lod_base[mesh_id] + lod, B = sum of n_lods buckets.
 * SLOTS: all members of all views sorted by (view, bucket, draw index) into ONE instance_ids array (room for n_views x N
 * words). view_first_slot[v] (optional, n_views + 1 words) = the number of members of the views before v, and
 * view_first_slot[n_views] = all members. instance_ids[s] = frames[v].first_instance_base + i for the member of view v in
 * slot s. Nothing at or behind the total member count is touched.
 * COMMANDS: view v's commands are entries [v * cmd_stride, v * cmd_stride + batch_counts[v]) of batch_cmds: one per NON-EMPTY
 * bucket of that view, in ascending bucket order, with mip_batch_draws_lods' fields except firstInstance, which is the
 * ABSOLUTE slot in the shared instance_ids (that call's value + view_first_slot[v]). A view without members gets
 * batch_counts[v] = 0. Every entry of a view's range at or behind its count is left untouched. cmd_stride >= min(B, N).
 * A consumer issues vkCmdDrawIndexedIndirectCount(batch_cmds, v * cmd_stride * 20, batch_counts, v * 4, cmd_stride, 20) per
 * view and reads entity_id = instance_ids[gl_InstanceIndex], or model[instance_ids[s] - base] from a frame's `model` output.
 * N = 0 is legal: n_views zero counts and, if asked for, n_views + 1 zero slots.
 *
 * ORDERING: enqueued on the context's first stream, where mip_run_views runs, so bitmaps written by a preceding
 * mip_run_views need no wait in between. Bitmaps from anywhere else — a mip_run of another frame slot, the caller's own
 * kernels — need mip_wait or the caller's ordering first, as documented for mip_batch_draws. Without MIP_OUT_ASYNC the call
 * returns when the outputs are complete. Scratch is the call's own, allocated at first use for the n_views x N asked for
 * (and grown by a later, larger call); it is not the per-slot scratch of mip_batch_draws / _lods / _ordered, so calls of
 * those behind any frame slot and this call do not disturb each other.
 * COST: n_views x B <= 256 sorts in one pass (four launches, whatever n_views); more takes several passes and, at instance
 * counts in the millions, currently longer than one mip_batch_draws_lods call per view (DESIGN.md section 22 has the figures).
 * ERRORS, MIP_ERR_INVALID_ARGUMENT: NULL ctx / frames / visible_bitmaps / policy / out / batch_cmds / batch_counts /
 * instance_ids; a wrong struct_size (MipViewBatchOutputs, MipLodPolicy); reserved != 0; unknown flags; a missing
 * MIP_OUT_DEVICE; n_views out of range; cmd_stride < min(B, N); a policy mip_batch_draws_lods refuses.
 * MIP_ERR_NOT_READY as mip_batch_draws. MIP_ERR_CAPACITY: n_views x N >= 2^32, or n_views x B > 2^31 (view * B + bucket is a
 * 32-bit key). A refused call writes nothing.
 * OUT OF SCOPE: batch_model (read the frame's `model` through instance_ids); the orders of mip_batch_draws_ordered; shards
 * (mip_merge_batches merges one view's chunks); mip_run_many / recorded launch graphs; the per-triangle stage; the wire forms. */
typedef struct MipViewBatchOutputs {
  uint32_t struct_size;      /* = sizeof(MipViewBatchOutputs) */
  uint32_t flags;            /* MIP_OUT_DEVICE (required) | MIP_OUT_ASYNC */
  void* batch_cmds;          /* DEVICE: n_views x cmd_stride MipDrawIndexedIndirectCommand */
  uint32_t cmd_stride;       /* commands reserved per view; >= min(B, N) */
  uint32_t reserved;         /* 0 */
  uint32_t* batch_counts;    /* DEVICE: n_views words: commands written for view v */
  uint32_t* instance_ids;    /* DEVICE: room for n_views x N words, shared by all views */
  uint32_t* view_first_slot; /* DEVICE, optional: n_views + 1 words: first slot of view v; [n_views] = all members */
} MipViewBatchOutputs;       /* 48 B */

int32_t mip_batch_draws_views(MipContext* ctx, const MipFrame* frames, const uint32_t* const* visible_bitmaps,
                              uint32_t n_views, const MipLodPolicy* policy, const MipViewBatchOutputs* out);

/* ---- Extension: batched draws for sharded scenes — shard chunks and their merge ------------------------------------------
 * mip_batch_draws_lods for a scene cut into contiguous draw-index shards (mip_run_sharded,
 * renderer_amd/sharded.py): every rank bins its own shard into a CHUNK (mip_batch_draws_shard), one all-gather moves the
 * chunks, and every rank merges them (mip_merge_batches) into, byte for byte, what ONE mip_batch_draws_lods call writes for
 * the unsharded scene: buckets are mesh-major over a table every rank holds, ids are global (first_instance_base + i), and
 * the shards are ranges in rank order, so (bucket, rank, slot) order is (bucket, draw index) order. NOT a reference
 * behaviour; checked against this repository's restatement (tests/batch_merge_restatement.py). Only integers are
 * involved, so every byte is determined.
 *
 * THE CHUNK, B = sum of n_lods over the mesh table:
 *   MipBatchChunkHeader { members, n_buckets = B, reserved[2] = 0 }     16 B
 *   uint32_t bucket_count[B]        dense, zeros included: batch_cmds is packed, so the bucket of a command cannot be recovered
 *   uint32_t pad[(4 - B % 4) % 4]   zeros: the ids start 16-byte aligned relative to the chunk
 *   uint32_t ids[capacity]          slots [0, members)
 * The ids come last on purpose: a rank always writes its complete chunk into a full-size send buffer and the exchange
 * sends a prefix of it; a tightened chunk that overflows is repaired by gathering again at full capacity. */
typedef struct MipBatchChunkHeader {
  uint32_t members;      /* ids the chunk holds */
  uint32_t n_buckets;    /* B of the emitting rank's mesh table */
  uint32_t reserved[2];  /* 0 */
} MipBatchChunkHeader;   /* 16 B */
#define MIP_MAX_BATCH_CHUNKS 64u
/* byte offset of a chunk's ids, and bytes of a chunk with room for `capacity` ids, for a table of B buckets */
#define MIP_BATCH_CHUNK_IDS_OFFSET(B) \
  ((uint64_t)sizeof(MipBatchChunkHeader) + ((uint64_t)(B) + (4u - (uint64_t)(B) % 4u) % 4u) * 4u)
#define MIP_BATCH_CHUNK_BYTES(B, capacity) (MIP_BATCH_CHUNK_IDS_OFFSET(B) + (uint64_t)(capacity) * 4u)

/* PRODUCER. Members, LOD, bucket and slot order are exactly those of mip_batch_draws_lods for the same ctx, frame,
 * visible_bitmap and policy: ids[0, members) are the bytes that call writes to instance_ids, bucket_count[b] is the number of
 * members of bucket b for every b < B, the header is {members, B, 0, 0} and the pad words are written as 0. Ids at or behind
 * `members` are not touched. `chunk` is a DEVICE pointer, 16-byte aligned, with room for MIP_BATCH_CHUNK_BYTES(B,
 * ids_capacity); ids_capacity >= N resident instances, otherwise MIP_ERR_INVALID_ARGUMENT (cutting a chunk is the exchange's
 * business). flags: MIP_OUT_DEVICE (required) | MIP_OUT_ASYNC. N = 0 writes the header and B zeros. The stream (behind the
 * frame issued last), the per-slot scratch, the policy checks, MIP_ERR_NOT_READY and MIP_ERR_CAPACITY are those of
 * mip_batch_draws_lods. A refused call writes nothing. */
int32_t mip_batch_draws_shard(MipContext* ctx, const MipFrame* frame, const uint32_t* visible_bitmap,
                              const MipLodPolicy* policy, void* chunk, uint32_t ids_capacity, uint32_t flags);

/* CONSUMER. `chunks`: DEVICE memory, 16-byte aligned, holding n_chunks chunks chunk_stride_bytes apart (a multiple of 16,
 * at least MIP_BATCH_CHUNK_BYTES(B, chunk_capacity); whatever an all-gather leaves behind a chunk is ignored), 1 <= n_chunks
 * <= MIP_MAX_BATCH_CHUNKS, in rank order. `out`: batch_model must be NULL, flags MIP_OUT_DEVICE (required) | MIP_OUT_ASYNC.
 * Needs the mesh table only, not instances; enqueued on the context's first stream, like mip_merge_draw_lists.
 * RESULT, with c[r][b] = chunk r's count of bucket b: total[b] = sum over r of c[r][b]; first[b] = the exclusive prefix sum of
 * total; the members of (b, r) go to slots [first[b] + sum over r' < r of c[r'][b], ... + c[r][b]), copied from chunk r's ids at
 * the exclusive prefix of c[r][.]. Commands: one per bucket with total[b] > 0, ascending, packed from entry 0, indexCount /
 * firstIndex / vertexOffset as mip_batch_draws_lods writes them for that bucket from THIS context's table, instanceCount =
 * total[b], firstInstance = first[b]. batch_count and instance_count as that call writes them; nothing at or behind either
 * count is touched. instance_ids needs room for n_chunks x chunk_capacity words and may be only 4-byte aligned; batch_cmds
 * needs room for min(B, n_chunks x chunk_capacity) commands.
 * BAD CHUNKS are decided before anything is copied. A chunk is CORRUPT if n_buckets != B, a reserved word is not 0, or its
 * counts do not sum to `members`: MIP_ERR_DEVICE. If none is corrupt and some chunk has members > chunk_capacity (a tightened
 * chunk overflowed): MIP_ERR_CAPACITY. Either way batch_count and instance_count are written as 0 and batch_cmds and
 * instance_ids are not touched; the status is returned by a synchronous call and by mip_wait for an asynchronous one. The
 * kernels never read outside [chunk, chunk + MIP_BATCH_CHUNK_BYTES(B, chunk_capacity)) and never write outside the room
 * stated above, whatever the words say.
 * REFUSED, nothing written: NULL ctx / chunks / out / batch_cmds / batch_count / instance_ids, a wrong struct_size, unknown
 * flags, a missing MIP_OUT_DEVICE, batch_model != NULL, n_chunks out of range, a misaligned pointer, a stride that is not a
 * multiple of 16 or too small: MIP_ERR_INVALID_ARGUMENT; no mesh table: MIP_ERR_NOT_READY; n_chunks x B > 2^24 or n_chunks x
 * chunk_capacity >= 2^32: MIP_ERR_CAPACITY.
 * OUT OF SCOPE: batch_model across shards (read `model` through the ids on the owning rank, or gather it separately); the
 * depth orders of mip_batch_draws_ordered (a merge of runs sorted by D is a different kernel); views; a native RCCL entry
 * point beside mip_run_sharded (renderer_amd/sharded.py, BatchExchange, is the exchange); mip_run_many / recorded graphs. */
int32_t mip_merge_batches(MipContext* ctx, const void* chunks, uint32_t n_chunks, uint64_t chunk_stride_bytes,
                          uint32_t chunk_capacity, const MipBatchOutputs* out);

/* ---- Extension: cluster culling — the frustum and Hi-Z tests per 64-triangle cluster ----------------------------------
 * The level between whole instances (mip_run, mip_run_occluded) and single triangles (the per-triangle stage): every level
 * of every mesh is cut into clusters of MIP_CLUSTER_TRIANGLES triangles with a box each; per frame, every cluster of every
 * member is tested like an instance and the survivors are drawn by range from the source index buffer. NOT a reference
 * behaviour; checked against this repository's restatement (tests/cluster_restatement.py) only.
 *
 * CLUSTER TABLE (mip_build_clusters). Buckets are mip_batch_draws_lods': b = lod_base[mesh] + lod, B = sum of n_lods. Bucket b
 * has T(b) = floor(index_len[lod] / 3) triangles — triangle t is indices[index_offset[lod] + 3t .. + 3), a tail of one or two
 * indices belongs to no cluster — and C(b) = ceil(T(b) / 64) clusters; cluster c holds triangles [64c, min(64c + 64, T)).
 * Its BOX is, per axis, an fminf / fmaxf fold from +inf / -inf over vertices[vertex_offset + index] of every corner of its
 * triangles: a NaN coordinate is ignored; min and max are exact, so the box is the same numbers in any order of reduction; as
 * with world_aabb the sign of a zero is not specified and nothing downstream depends on it. Boxes are kept bucket-major,
 * cluster c of bucket b at cluster_base[b] + c, cluster_base = the exclusive prefix sum of C. The table is built on the
 * device from the resident geometry, all n_lods levels of every mesh; the call returns when it is complete. It needs the
 * mesh table and mip_set_geometry (MIP_ERR_NOT_READY); every level's range must lie inside the uploaded indices and every
 * vertex its triangles name inside the uploaded vertices (MIP_ERR_INVALID_ARGUMENT, checked on the host); more than 2^31
 * clusters are MIP_ERR_CAPACITY. A later mip_set_mesh_table or mip_set_geometry makes the table STALE: mip_cull_clusters
 * returns MIP_ERR_NOT_READY until it is built again. mip_cluster_count: the clusters of a valid table, else 0.
 * mip_read_cluster_boxes copies 6 floats per cluster (min xyz, max xyz), bucket-major, to HOST memory with room for
 * capacity_clusters of them (fewer than the table holds: MIP_ERR_CAPACITY); it exists so that the build is tested on its own.
 *
 * PER FRAME (mip_cull_clusters). frame, visible_bitmap (DEVICE) and policy (required) are mip_batch_draws_lods'; here
 * frame->planes IS read. occ is NULL or a MipOcclusion of which pyramid, width, height and pv are read; its candidates and
 * occluded_bitmap must be NULL and its flags 0.
 * MEMBERS: instance i is a member iff bit i is set and T(bucket_i) > 0, lod_i selected exactly as mip_batch_draws_lods does.
 * WORK ITEMS: (i, c) for every member i in draw-index order and every c < C(bucket_i) in order; W is their number.
 * SURVIVES(i, c): the world box is what world_aabb would hold for instance i if its mesh box were the cluster's box — the
 * same chain under the instance's model matrix, identical as numbers, non-finite instances and non-finite cluster boxes
 * through the literal chain. The item survives iff that box is not culled by the plane test against frame->planes AND
 * (occ is NULL or the box is not occluded by steps 1-9 of the occlusion test above).
 * COMMANDS: a surviving item is a HEAD if c == 0 or (i, c - 1) does not survive; a run never crosses an instance. One
 * command per head, in (i, c) order, packed from entry 0: indexCount = 3 x the triangles of the run's clusters (the last
 * cluster of a bucket may be short), instanceCount = 1, firstIndex = index_offset[lod] + 192 x c_head (the source mesh's own
 * range, as the batches address it; first_index_base is not read), vertexOffset = the mesh's, firstInstance =
 * first_instance_base + i. An instance whose clusters all survive gets one command with the level's 3 x T indices; one
 * none of whose clusters survive gets none. cmd_count = min(heads, cmd_capacity); entries at or behind it are never touched.
 * stats (optional, 4 words): {heads, surviving clusters, W, members}.
 * OVERFLOW. Heads > cmd_capacity: the first cmd_capacity commands are written exactly as they would be with room, cmd_count =
 * cmd_capacity, stats holds the true values, and the status is MIP_ERR_CAPACITY — from the call, or from mip_wait for an
 * asynchronous one (below). W > work_capacity (0 = the library's own bound, N x the largest C of the table), or W >= 2^32:
 * MIP_ERR_CAPACITY, cmd_count = 0, stats = {0, 0, W mod 2^32, members}, no command written. The context stays usable.
 * WHO REPORTS AN OVERFLOW: a synchronous call returns the status of ITSELF alone, once, whatever else of the context is in
 * flight — an overflow of an earlier asynchronous call is never charged to it. The overflow of an asynchronous call is
 * returned by the next mip_wait that has no other error to return, once for all asynchronous calls since the last such
 * mip_wait; when mip_wait returns another error first, the overflow is kept and the mip_wait after it returns it. Which
 * call overflowed is read from the calls' own cmd_count and stats.
 * N = 0 writes a zero count (and zero stats). REFUSED, nothing written: NULL ctx / frame / bitmap / out / cluster_cmds /
 * cmd_count, a wrong struct_size of any struct, unknown flags, a missing MIP_OUT_DEVICE, a misaligned output, a policy
 * mip_batch_draws_lods refuses, a MipOcclusion with candidates, occluded_bitmap or flags, a depth extent out of range or a
 * NULL pyramid: MIP_ERR_INVALID_ARGUMENT; no instances, no mesh table, no valid cluster table: MIP_ERR_NOT_READY.
 * ORDERING: enqueued on the stream of the frame issued last, like mip_batch_draws; a bitmap that frame writes and a pyramid
 * built (mip_build_depth_pyramid) for the next run need no wait. Scratch is the call's own, per frame slot, allocated at
 * first use and grown by a larger call; with work_capacity = 0 it is sized for N x the largest C (16 bytes per 64 work
 * items), so a scene of large meshes should state its bound.
 * OUT OF SCOPE: shards, skinned instances, mip_run_many and recorded graphs; batch_model. (The per-triangle test on
 * surviving clusters is mip_cull_cluster_triangles; the normal-cone back-face test is mip_cull_clusters_cone; several views
 * in one call are mip_cull_clusters_views; a flat list of the surviving clusters for ONE indirect draw is mip_list_clusters.) */
#define MIP_CLUSTER_TRIANGLES 64u
typedef struct MipClusterOutputs {
  uint32_t struct_size;      /* = sizeof(MipClusterOutputs) */
  uint32_t flags;            /* MIP_OUT_DEVICE (required) | MIP_OUT_ASYNC */
  void* cluster_cmds;        /* DEVICE: room for cmd_capacity MipDrawIndexedIndirectCommand */
  uint32_t cmd_capacity;     /* commands that fit */
  uint32_t work_capacity;    /* the caller's bound on W; 0 = N x the largest C of the table */
  uint32_t* cmd_count;       /* DEVICE: commands written = min(heads, cmd_capacity) */
  uint32_t* stats;           /* DEVICE, optional, 4 words: heads, surviving clusters, W, members */
} MipClusterOutputs;         /* 40 B */

int32_t mip_build_clusters(MipContext* ctx);
uint32_t mip_cluster_count(const MipContext* ctx);
int32_t mip_read_cluster_boxes(MipContext* ctx, float* host_out, uint32_t capacity_clusters);
int32_t mip_cull_clusters(MipContext* ctx, const MipFrame* frame, const uint32_t* visible_bitmap, const MipLodPolicy* policy,
                          const MipOcclusion* occ, const MipClusterOutputs* out);

/* ---- Extension: cluster culling in two phases — record the occluded clusters, test them again -------------------------
 * The only pyramid a frame has when it starts is last frame's. mip_cull_clusters_phase is mip_cull_clusters as two calls around
 * the frame's own depth: FIRST culls against the old pyramid and RECORDS the work items it removed for occlusion alone; after
 * the survivors are drawn and the pyramid is rebuilt, SECOND tests exactly those items against the new pyramid and emits the
 * ones that are visible after all — and nothing that FIRST already drew. NOT a reference behaviour; checked against this
 * repository's restatement (tests/cluster_phase_restatement.py) only. MEMBERS, WORK ITEMS, W, SURVIVES, HEAD and COMMANDS are
 * the words of mip_cull_clusters above; mip_cull_clusters itself is unchanged.
 *
 * THE RECORD: the caller's DEVICE memory, 16-byte aligned, record_bytes of room. A 16-byte header of four words {W, members,
 * candidates, 0}, then ceil(W / 64) 64-bit words: bit j of word k belongs to work item 64 k + j in (i, c) order; bits at or
 * above W are 0. mip_cluster_record_bytes(work_items) = 16 + 8 x ceil(work_items / 64) is its size; pure, no device, no context.
 *
 * FIRST (phase = MIP_CLUSTER_PHASE_FIRST). occ is required, exactly as mip_cull_clusters takes it (a pyramid; candidates,
 * occluded_bitmap NULL; flags 0). cluster_cmds, cmd_count and stats are byte for byte what mip_cull_clusters writes for the
 * same ctx, frame, visible_bitmap, policy, occ and out. The record is written in addition: the bit of work item (i, c) is set
 * iff its world box is NOT culled by the plane test against frame->planes AND is occluded by steps 1-9 of the occlusion test
 * under occ — an item the planes cull is no candidate, whatever the pyramid says. candidates = the number of set bits. A
 * command overflow (heads > cmd_capacity) leaves the record complete and valid. A WORK overflow is mip_cull_clusters' (W >
 * work_capacity or its own bound, W >= 2^32) and also record_bytes < mip_cluster_record_bytes(W): commands, count, stats and
 * status follow mip_cull_clusters' work-overflow rule, the record's header becomes {0xFFFFFFFF, 0, 0, 0} — no running call
 * has that W — and no record word is defined. N = 0: a zero count, zero stats and the header {0, 0, 0, 0}.
 *
 * SECOND (phase = MIP_CLUSTER_PHASE_SECOND). frame (cam_pos and first_instance_base), visible_bitmap and policy are the FIRST
 * call's, and the instance columns, the mesh table and the cluster table are unchanged since that call; occ is the NEW
 * pyramid, required, in the same form. frame->planes is NOT read: a candidate has passed the plane test. MEMBERS, WORK ITEMS
 * and W are formed as always. SURVIVES2(i, c) holds iff the item's record bit is set AND its world box is not occluded by
 * steps 1-9 under occ. HEAD and COMMANDS are mip_cull_clusters' rules with SURVIVES2 in SURVIVES' place: a surviving item is
 * a HEAD if c == 0 or (i, c - 1) does not survive this call — a run that touches a run FIRST drew is still a command of its
 * own. stats = {heads, survivors of this call, W, members}. The command-overflow rule is unchanged; a W that exceeds
 * work_capacity, or that the record_bytes stated to this call have no words for, is the work overflow of mip_cull_clusters.
 * NOT THIS CALL'S RECORD: if the header's W or members differs from the call's, the status is MIP_ERR_DEVICE, cmd_count = 0,
 * stats = {0, 0, W, members} (the call's own) and nothing else is written. The status comes from the call, or from mip_wait
 * for an asynchronous one, by the route of an overflow (WHO REPORTS AN OVERFLOW above, with this code; when asynchronous
 * calls since the last mip_wait raised both, MIP_ERR_DEVICE is the one returned). The context stays usable. This is a sanity
 * check, not proof that nothing moved: a record of another call with the same W and the same member count is accepted, and
 * its bits are then applied to the wrong items. The record is never modified by SECOND. N = 0: a zero count, zero stats.
 *
 * REFUSED, nothing written, MIP_ERR_INVALID_ARGUMENT: everything mip_cull_clusters refuses; a NULL rec or record; a record
 * that is not 16-byte aligned; record_bytes < 16; an unknown phase; a wrong MipClusterRecord.struct_size; a NULL occ.
 * MIP_ERR_NOT_READY as mip_cull_clusters.
 * ORDERING: both calls go on the stream of the frame issued last, as mip_cull_clusters does. A SECOND call normally follows
 * mip_build_depth_pyramid and the phase-2 mip_run_occluded, which with more than one frame in flight is another slot's
 * stream than the FIRST call's: the context orders every SECOND call behind the last FIRST call it was given, on the device;
 * the caller needs no host wait between them.
 * THE FRAME that composes instance phases and cluster phases: (1) mip_run_occluded with last frame's pyramid, then FIRST over
 * its bitmap; (2) draw, rebuild the pyramid; (3) mip_run_occluded with the inverted candidates, then plain mip_cull_clusters
 * over ITS bitmap under the new pyramid (instances phase 1 never saw as visible have no record); (4) SECOND over phase 1's
 * bitmap.
 * OUT OF SCOPE here: the flat list of the visible clusters in two phases (mip_list_clusters_phase below). */
#define MIP_CLUSTER_PHASE_FIRST  1u
#define MIP_CLUSTER_PHASE_SECOND 2u
typedef struct MipClusterRecord {
  uint32_t struct_size;   /* = sizeof(MipClusterRecord) */
  uint32_t phase;         /* MIP_CLUSTER_PHASE_FIRST: written; _SECOND: read */
  void*    record;        /* DEVICE, 16-byte aligned, the caller's */
  uint64_t record_bytes;  /* room behind `record` */
} MipClusterRecord;       /* 24 B */
uint64_t mip_cluster_record_bytes(uint64_t work_items);
int32_t mip_cull_clusters_phase(MipContext* ctx, const MipFrame* frame, const uint32_t* visible_bitmap, const MipLodPolicy* policy,
                                const MipOcclusion* occ, const MipClusterOutputs* out, const MipClusterRecord* rec);

/* ---- Extension: per-triangle culling of surviving clusters — the instance -> cluster -> triangle pipeline ---------------
 * mip_cull_cluster_triangles is mip_cull_clusters followed by the per-triangle stage's test on the triangles of the clusters
 * that survived: instead of ranges of the source index buffer it writes ONE culled index stream and commands into it.
 * NOT a reference behaviour; checked against this repository's restatement (tests/cluster_triangle_restatement.py) only.
 * MEMBERS, WORK ITEMS, W, SURVIVES and HEAD are the words of mip_cull_clusters above; mip_cull_clusters itself is unchanged.
 * frame->planes, frame->pv, frame->cam_pos and frame->first_instance_base are read; frame->first_index_base is not. No
 * `model` buffer is an input.
 *
 * TRI_SURVIVES(i, c, t), for a surviving item (i, c) and a triangle t of cluster c — triangle t of the level is
 * indices[index_offset[lod] + 3t .. + 3) over vertices[vertex_offset + index]: the triangle survives iff the per-triangle
 * stage's test does NOT cull it. clip = pv * (model * vec4(v, 1)) as column combinations left to right, no FMA; culled iff the
 * determinant of the xyw columns is > 0, or all three corners lie beyond one x or y NDC bound. `model` is the sixteen floats
 * mip_run writes to `model` for instance i, non-finite rows included; the call forms it from the instance columns.
 * INDEX STREAM: for every surviving triangle its three source index values, as the per-triangle stage appends them, packed
 * densely from word 0 of culled_indices in (i, c, t) order. Words at or behind 3 x (surviving triangles) are never touched.
 * COMMANDS: one per HEAD, in (i, c) order, at the entry mip_cull_clusters would use: indexCount = 3 x the surviving triangles
 * of the run's clusters, firstIndex = 3 x the surviving triangles of all items in front of the head, instanceCount = 1,
 * vertexOffset = the mesh's, firstInstance = first_instance_base + i. A run none of whose triangles survives KEEPS its command
 * with indexCount = 0, a legal draw that draws nothing. cmd_count = min(heads, cmd_capacity).
 * stats (optional, 6 words): {heads, surviving clusters, W, members, surviving triangles, triangles tested} — tested = the
 * triangles of the surviving clusters; the last two mod 2^32.
 * OVERFLOW, reported as mip_cull_clusters reports (WHO REPORTS AN OVERFLOW above). WORK overflow, as mip_cull_clusters:
 * cmd_count = 0, stats = {0, 0, W mod 2^32, members, 0, 0}, nothing else written. INDEX overflow, 3 x surviving triangles >
 * index_capacity or >= 2^32: MIP_ERR_CAPACITY, cmd_count = 0, no command and no index written, stats holds the true six values
 * — size the buffer by stats[4] and call again. COMMAND overflow: the first cmd_capacity commands exactly as with room, the
 * index stream complete, MIP_ERR_CAPACITY. The context stays usable in every case. N = 0: a zero count and six zero stats.
 * REFUSED, nothing written: everything mip_cull_clusters refuses; a NULL or misaligned culled_indices and a wrong struct_size
 * are MIP_ERR_INVALID_ARGUMENT.
 * ORDERING and scratch are mip_cull_clusters'; the scratch per frame slot is 12 bytes per work item of the bound larger (a
 * triangle word and a prefix per item) — 110 MB at 9.1 M items — so, again, a scene of large meshes should set work_capacity.
 * OUT OF SCOPE: the two-phase record; views, shards and skinned instances; mip_run_many and recorded graphs; first_index_base.
 * Dropping empty runs is mip_list_cluster_triangles' (below): the list form with a triangle mask per entry and no stream. */
typedef struct MipClusterTriangleOutputs {
  uint32_t struct_size;      /* = sizeof(MipClusterTriangleOutputs) */
  uint32_t flags;            /* MIP_OUT_DEVICE (required) | MIP_OUT_ASYNC */
  void* cluster_cmds;        /* DEVICE: room for cmd_capacity MipDrawIndexedIndirectCommand */
  uint32_t cmd_capacity;     /* commands that fit */
  uint32_t work_capacity;    /* the caller's bound on W; 0 = N x the largest C of the table */
  uint32_t* cmd_count;       /* DEVICE: commands written */
  uint32_t* stats;           /* DEVICE, optional, 6 words */
  void* culled_indices;      /* DEVICE, 4-byte aligned: room for index_capacity 32-bit indices */
  uint32_t index_capacity;   /* indices that fit */
} MipClusterTriangleOutputs; /* 56 B */
int32_t mip_cull_cluster_triangles(MipContext* ctx, const MipFrame* frame, const uint32_t* visible_bitmap, const MipLodPolicy* policy,
                                   const MipOcclusion* occ, const MipClusterTriangleOutputs* out);

/* ---- Extension: cluster culling with normal cones — the back-face test per 64-triangle cluster --------------------------
 * The per-triangle stage culls a triangle whose clip-space determinant is > 0 (back-facing). A cluster all of whose triangles
 * are back-facing for a view is found here from 32 bytes, before an index is loaded. NOT a reference behaviour; checked against
 * this repository's restatement (tests/cluster_cone_restatement.py) only. Every entry point above is unchanged.
 * All arithmetic below is float, one rounding per written operation (no FMA), sqrtf and / correctly rounded.
 *
 * THE CONE TABLE (mip_build_cluster_cones): one cone per cluster of a valid cluster table, 8 floats {axis xyz, k, centre xyz, r},
 * bucket-major like the boxes, built on the device from the resident geometry; the call returns when it is complete. For
 * triangle t of the cluster with corners p0, p1, p2 (vertices[vertex_offset + index], in index order):
 *   e1 = p1 - p0, e2 = p2 - p0 (per component); n = (e1.y e2.z - e1.z e2.y, e1.z e2.x - e1.x e2.z, e1.x e2.y - e1.y e2.x);
 *   len2 = (n.x n.x + n.y n.y) + n.z n.z. The triangle is PROPER iff len2 > 0 and len2 < +inf. nh_t = n / sqrtf(len2).
 *   AXIS: A = the sum of nh_t over the cluster, per component, as a fixed butterfly over 64 slots (slot t = triangle t, a slot
 *   without a triangle holds +0): level j = 0..5 replaces every slot v[l] by v[l] + v[l xor 2^j]; float addition is commutative,
 *   so all slots hold the same bits. aa = (A.x A.x + A.y A.y) + A.z A.z; a = A / sqrtf(aa).
 *   SPREAD: m = the minimum over the cluster's triangles of (nh.x a.x + nh.y a.y) + nh.z a.z; k = sqrtf(fmaxf(1 - m m, 0)) + 2^-7.
 *   SPHERE: with lo, hi the cluster's box: centre = (hi + lo) / 2, h = (hi - lo) / 2, r0 = sqrtf((h.x h.x + h.y h.y) + h.z h.z),
 *   r = r0 + r0 x 2^-7.
 *   NO CONE — k = +inf, the other seven floats +0 — when a triangle of the cluster is not PROPER (a zero-area triangle is never
 *   culled by the determinant; NaN and infinite vertices end here), when aa is not > 0 and < +inf, or when m is not > 0.1f.
 * The margins 2^-7 (on k, absolute) and 2^-7 (on r, relative) make the test below conservative against the rounding of the
 * build and of the per-frame chain inside a domain: every triangle has len2 >= 2^-10 (e1.e1)(e2.e2), and the cluster centre's
 * model-space coordinates times s and the instance's position are at most 2^12 s r in magnitude, and s k |d| >= 2^-63 so that no
 * square underflows (DESIGN section 29 derives it; the library does not check the domain).
 * The table needs a valid cluster table (MIP_ERR_NOT_READY) and becomes STALE with it: after mip_set_mesh_table,
 * mip_set_geometry or a new mip_build_clusters the cone calls return MIP_ERR_NOT_READY until it is built again.
 * mip_read_cluster_cones copies the 8 floats per cluster to HOST memory under mip_read_cluster_boxes' rules.
 *
 * THE VIEW (MipClusterCone). eye: the world-space point the view projects from; facing: +1.0f or -1.0f. Write rows x, y, w of
 * a projection pv as [A | b]: clip.xyw = A (x - e) with e = -A^-1 b, and the per-triangle stage's determinant is
 * det(A) x (x0 - e) . n_t; so that stage culls triangle t exactly when facing x n_t . (x0 - e) > 0 with facing = sign(det A).
 * mip_cone_from_pv computes e and facing in double and rounds once; pure host, no context. It returns
 * MIP_ERR_INVALID_ARGUMENT for a NULL argument, a singular or non-finite A, or an eye that is no finite float (an orthographic
 * projection has no eye). The eye of a shadow view is the light; frame->cam_pos stays the LOD rule's reference point.
 *
 * PER FRAME (mip_cull_clusters_cone, mip_cull_cluster_triangles_cone): mip_cull_clusters / mip_cull_cluster_triangles with
 * `cone` in front of `out`. MEMBERS, WORK ITEMS, W, HEAD, COMMANDS, TRI_SURVIVES, the index stream, the stats (4 and 6 words),
 * the three overflow rules, WHO REPORTS AN OVERFLOW, ORDERING and scratch are those calls', with SURVIVES replaced by
 *   SURVIVES_CONE(i, c) = SURVIVES(i, c) AND NOT CONE_CULLED(i, c).
 * CONE_CULLED(i, c), with p, q = (i, j, k, w), s the instance's position, rotation and scale and {a, k, centre, r} the cone:
 *   GUARD: s > 0 and | qq - 1 | <= 2^-20, qq = ((q.i q.i + q.j q.j) + q.k q.k) + q.w q.w. (A non-unit quaternion makes the
 *   matrix no similarity, a non-positive scale flips the winding: such an instance is never cone-culled.)
 *   M[r][c] = R[r][c] x s, R the rotation matrix of the model matrix's chain (nalgebra's to_rotation_matrix): the upper 3 x 3
 *   of the sixteen floats mip_run writes for a finite instance. For r = 0, 1, 2:
 *   cw[r] = ((M[r][0] centre.x + M[r][1] centre.y) + M[r][2] centre.z) + p[r];  aw[r] = (M[r][0] a.x + M[r][1] a.y) + M[r][2] a.z;
 *   d = cw - eye;  da = (d.x aw.x + d.y aw.y) + d.z aw.z;  dd = (d.x d.x + d.y d.y) + d.z d.z;
 *   Av = facing x da - (s s) r;  Bv = ((s k) (s k)) dd.
 *   CONE_CULLED iff GUARD and Av > 0 and Av Av > Bv and Av and Bv are finite.
 * NO CONE (k = +inf), a NaN anywhere, an infinite eye and a non-finite instance all fail a comparison: the item is not
 * cone-culled. This is d . a >= k |d| + r for the cluster's bounding sphere, k = sin(theta), scaled by s and squared; strict
 * comparisons keep the edge-on tie on the surviving side, as det > 0 does.
 * REFUSED, nothing written: everything the plain call refuses; a NULL cone, a wrong MipClusterCone.struct_size, flags != 0, a
 * facing other than +1.0f / -1.0f: MIP_ERR_INVALID_ARGUMENT; no valid cone table: MIP_ERR_NOT_READY.
 * OUT OF SCOPE: a cone form of mip_cull_clusters_phase; orthographic views; apex-form cones and spheres tighter than the box's;
 * views, shards, skinned instances, mip_run_many and recorded graphs. */
typedef struct MipClusterCone {
  uint32_t struct_size;   /* = sizeof(MipClusterCone) */
  uint32_t flags;         /* 0 */
  float eye[3];           /* world-space point the view projects from */
  float facing;           /* +1.0f or -1.0f, nothing else */
} MipClusterCone;         /* 24 B */
int32_t mip_build_cluster_cones(MipContext* ctx);
int32_t mip_read_cluster_cones(MipContext* ctx, float* host_out, uint32_t capacity_clusters);
int32_t mip_cone_from_pv(const float pv[16], MipClusterCone* out);
int32_t mip_cull_clusters_cone(MipContext* ctx, const MipFrame* frame, const uint32_t* visible_bitmap, const MipLodPolicy* policy,
                               const MipOcclusion* occ, const MipClusterCone* cone, const MipClusterOutputs* out);
int32_t mip_cull_cluster_triangles_cone(MipContext* ctx, const MipFrame* frame, const uint32_t* visible_bitmap, const MipLodPolicy* policy,
                                        const MipOcclusion* occ, const MipClusterCone* cone, const MipClusterTriangleOutputs* out);

/* ---- Extension: cluster culling for several views in one call -------------------------------------------------------------
 * mip_cull_clusters (the frustum test, no pyramid) for n_views views of the resident instances — cascades, cube faces, the
 * lights of a shadow pass, stereo eyes — in ONE call: the level, the work items and the world box of every (instance, cluster)
 * are formed once, and only the six planes and the bitmap bit differ per view. NOT a reference behaviour; checked against this
 * repository's restatement (tests/cluster_views_restatement.py), byte for byte. MEMBERS' LOD, WORK ITEMS, the world box, HEAD
 * and the command fields are the words of mip_cull_clusters above; mip_cull_clusters itself is unchanged.
 *
 * VIEWS: 1 <= n_views <= MIP_MAX_VIEWS. frames and visible_bitmaps are as in mip_batch_draws_views: view v is frames[v] with
 * visible_bitmaps[v]; `visible_bitmaps` is a HOST array of n_views DEVICE pointers; a NULL entry means every resident
 * instance; two views may share a pointer. Read per view: planes and first_instance_base.
 * ONE LOD FOR ALL VIEWS: the level of instance i is picked by `policy` from frames[0].cam_pos, exactly as mip_batch_draws_lods
 * picks it; frames[v].cam_pos for v > 0 is NOT read. This differs deliberately from mip_batch_draws_views, which picks a level
 * per view: a shadow caster keeps one level across cascades and faces, and a shared level is what makes a work item, and its
 * world box, common to all views.
 * MEMBERS: instance i is a member iff its bit is set in AT LEAST ONE view's bitmap (a NULL entry counts as set) and
 * T(bucket_i) > 0.
 * WORK ITEMS, W: as in mip_cull_clusters, over these members: (i, c) for every member i in draw-index order and every
 * c < C(bucket_i) in order.
 * SURVIVES_v(i, c): bit i of view v is set, AND the world box — the one mip_cull_clusters defines: same chain, same numbers —
 * is not culled by the plane test against frames[v].planes.
 * HEAD and COMMANDS, per view: mip_cull_clusters' rules with SURVIVES_v in place of SURVIVES; firstInstance =
 * frames[v].first_instance_base + i. View v's commands are entries [v * cmd_stride, v * cmd_stride + cmd_counts[v]) of
 * cluster_cmds; cmd_counts[v] = min(heads_v, cmd_stride); entries at or behind a view's count are never touched.
 * stats (optional, 2 + 2 x n_views words): {W, members, heads_0, survivors_0, heads_1, survivors_1, ...}.
 * THE EQUIVALENCE: let f_v = frames[v] with cam_pos replaced by frames[0].cam_pos. View v's command range, cmd_counts[v],
 * heads_v and survivors_v are byte for byte what mip_cull_clusters(ctx, &f_v, visible_bitmaps[v] (a full bitmap where the entry
 * is NULL), policy, NULL, {cmd_capacity = cmd_stride}) writes, whenever both calls run: an instance outside view v's bitmap
 * has no survivor in view v and therefore no command.
 * OVERFLOW. Some heads_v > cmd_stride: that view gets its first cmd_stride commands exactly as with room, the other views are
 * complete, stats are true, the status is MIP_ERR_CAPACITY. W > work_capacity (0 = the library's own bound, N x the largest C
 * of the table), or W >= 2^32: every count is 0, stats = {W mod 2^32, members, 0, ...}, no command is written,
 * MIP_ERR_CAPACITY. WHO REPORTS is mip_cull_clusters' rule: a synchronous call reports its own overflow, once; an asynchronous
 * call through the next mip_wait that has no other error to return. The call is not tied to a frame slot and has status words
 * of its own: a mip_cull_clusters behind a frame slot is never charged with this call's overflow, nor this call with its.
 * N = 0 writes n_views zero counts (and zero stats).
 * REFUSED, nothing written, MIP_ERR_INVALID_ARGUMENT: NULL ctx / frames / visible_bitmaps / policy / out / cluster_cmds /
 * cmd_counts; a wrong struct_size of either struct; unknown flags; a missing MIP_OUT_DEVICE; a misaligned output (4 bytes);
 * n_views out of range; a policy mip_batch_draws_lods refuses. MIP_ERR_NOT_READY: no instances, no mesh table, or no valid
 * cluster table.
 * ORDERING: enqueued on the context's first stream, where mip_run_views runs, so the bitmaps a preceding mip_run_views writes
 * need no wait. Scratch is the call's own, allocated at first use and grown by a larger call: (1 + n_views) x 8 bytes per 64
 * work items of the bound plus 2 bytes per instance, beside the per-instance lists. No frame slot's cluster scratch is
 * touched: a cluster call behind a frame slot and this call do not disturb each other.
 * OUT OF SCOPE: a pyramid per view (mip_list_clusters_views_occluded below); the two phases; the per-triangle test (one view: mip_list_cluster_triangles below); cones; shards; skinned instances; mip_run_many
 * and recorded graphs. */
typedef struct MipClusterViewOutputs {
  uint32_t struct_size;      /* = sizeof(MipClusterViewOutputs) */
  uint32_t flags;            /* MIP_OUT_DEVICE (required) | MIP_OUT_ASYNC */
  void* cluster_cmds;        /* DEVICE: n_views x cmd_stride MipDrawIndexedIndirectCommand */
  uint32_t cmd_stride;       /* commands reserved per view */
  uint32_t work_capacity;    /* the caller's bound on W (of the union of the views' members); 0 = N x the largest C of the table */
  uint32_t* cmd_counts;      /* DEVICE: n_views words: commands written for view v = min(heads_v, cmd_stride) */
  uint32_t* stats;           /* DEVICE, optional: 2 + 2 x n_views words: W, members, then heads and surviving clusters per view */
} MipClusterViewOutputs;     /* 40 B */

int32_t mip_cull_clusters_views(MipContext* ctx, const MipFrame* frames, const uint32_t* const* visible_bitmaps,
                                uint32_t n_views, const MipLodPolicy* policy, const MipClusterViewOutputs* out);

/* ---- Extension: the visible-cluster list for one indirect draw ------------------------------------------------------------
 * mip_cull_clusters ends in one command per run of surviving clusters. A renderer that culls per cluster rather submits ONE
 * vkCmdDrawIndirect (or one mesh-task dispatch) over a flat list of the visible clusters, and its vertex shader pulls the
 * indices itself. mip_list_clusters is mip_cull_clusters (cone == NULL) or mip_cull_clusters_cone (cone given) with that list
 * in the commands' place: one 16-byte MipClusterEntry per surviving work item, and the arguments of the one draw. NOT a
 * reference behaviour; checked against this repository's restatement (tests/cluster_list_restatement.py) only. MEMBERS, WORK
 * ITEMS, W and SURVIVES are the words of mip_cull_clusters above; every entry point above is unchanged.
 *
 * SURVIVES: with cone == NULL that of mip_cull_clusters (the planes, and the pyramid when occ is given); with a cone that of
 * mip_cull_clusters_cone (the cone test in front of it). frame, visible_bitmap, policy and occ are mip_cull_clusters', cone is
 * mip_cull_clusters_cone's.
 * ENTRIES: one per surviving work item, in (i, c) order, packed from entry 0. instance = first_instance_base + i (wraps as
 * firstInstance does), first_index = index_offset[lod] + 192 x c (the source mesh's own range), vertex_offset = the mesh's,
 * index_count = 3 x the triangles of cluster c (192, or fewer in the last cluster of a level): exactly firstInstance,
 * firstIndex, vertexOffset and indexCount of the command mip_cull_clusters would write for a run of that one cluster. The list
 * is therefore the cluster-by-cluster expansion of the command list of mip_cull_clusters / mip_cull_clusters_cone for the same
 * arguments. entry_count = min(survivors, entry_capacity); entries at or behind it are never touched.
 * draw_args (optional, 4 words): VkDrawIndirectCommand {vertexCount = 192, instanceCount = entry_count, 0, 0}.
 * stats (optional, 3 words): {survivors, W, members}.
 * ENTRY OVERFLOW (survivors > entry_capacity): the first entry_capacity entries are written exactly as they would be with room,
 * entry_count = entry_capacity and draw_args[1] holds the same value, stats holds the true values, and the status is
 * MIP_ERR_CAPACITY, reported by WHO REPORTS AN OVERFLOW of mip_cull_clusters: the same status words, the same mip_wait route.
 * WORK OVERFLOW (W > work_capacity — 0 = the library's own bound, N x the largest C of the table — or W >= 2^32):
 * MIP_ERR_CAPACITY, entry_count = 0, draw_args = {192, 0, 0, 0}, stats = {0, W mod 2^32, members}; nothing else is written
 * and the context stays usable.
 * N = 0 writes a zero count, {192, 0, 0, 0} and zero stats.
 * REFUSED, nothing written: everything mip_cull_clusters refuses (cluster_entries and entry_count in cluster_cmds' and
 * cmd_count's place; draw_args 4-byte aligned like the other words); everything mip_cull_clusters_cone refuses about a
 * non-NULL cone; cluster_entries not 16-byte aligned: MIP_ERR_INVALID_ARGUMENT. MIP_ERR_NOT_READY as for those calls: no
 * instances, no mesh table, a missing or stale cluster table, and with a cone a missing or stale cone table.
 * ORDERING and scratch are mip_cull_clusters': the stream of the frame issued last, scratch per frame slot that grows lazily —
 * 8 bytes per 64 work items of the bound on top of mip_cull_clusters' 16 — and is freed with the rest.
 *
 * THE CONSUMER: vkCmdDrawIndirect(cmd, draw_args, 0, 1, 16) with a triangle-list pipeline and no index buffer bound, and
 *   MipClusterEntry e = entries[gl_InstanceIndex];
 *   if (gl_VertexIndex < e.index_count) { v = vertices[indices[e.first_index + gl_VertexIndex] + e.vertex_offset];
 *                                         model = models[e.instance - first_instance_base]; ... }   // (the subtraction wraps as the sum did)
 *   else gl_Position = vec4(0);   // a degenerate vertex: the triangles of a short last cluster's tail have no area
 * OUT OF SCOPE: the two-phase record and an entry base (mip_list_clusters_phase below); several views in THIS call (mip_list_clusters_views below;
 * commands per view: mip_cull_clusters_views); the per-triangle test (on this list: mip_list_cluster_triangles below; as an
 * index stream with commands: mip_cull_cluster_triangles); shards, skinned instances, mip_run_many and recorded graphs. */
typedef struct MipClusterEntry {
  uint32_t instance;         /* first_instance_base + i (wraps as firstInstance does) */
  uint32_t first_index;      /* index_offset[lod] + 192 x c: the source mesh's own range */
  int32_t vertex_offset;     /* the mesh's */
  uint32_t index_count;      /* 3 x the triangles of cluster c: 192, or fewer in the last cluster of a level */
} MipClusterEntry;           /* 16 B: what a one-cluster command of mip_cull_clusters holds */
typedef struct MipClusterListOutputs {
  uint32_t struct_size;      /* = sizeof(MipClusterListOutputs) */
  uint32_t flags;            /* MIP_OUT_DEVICE (required) | MIP_OUT_ASYNC */
  void* cluster_entries;     /* DEVICE, 16-byte aligned: room for entry_capacity MipClusterEntry */
  uint32_t entry_capacity;   /* entries that fit */
  uint32_t work_capacity;    /* the caller's bound on W; 0 = N x the largest C of the table */
  uint32_t* entry_count;     /* DEVICE: entries written = min(survivors, entry_capacity) */
  uint32_t* draw_args;       /* DEVICE, optional, 4 words: VkDrawIndirectCommand {192, entry_count, 0, 0} */
  uint32_t* stats;           /* DEVICE, optional, 3 words: survivors, W, members */
} MipClusterListOutputs;     /* 48 B */

int32_t mip_list_clusters(MipContext* ctx, const MipFrame* frame, const uint32_t* visible_bitmap, const MipLodPolicy* policy,
                          const MipOcclusion* occ /* or NULL */, const MipClusterCone* cone /* or NULL */,
                          const MipClusterListOutputs* out);

/* ---- Extension: visible-cluster lists for several views in one call --------------------------------------------------------
 * mip_cull_clusters_views with mip_list_clusters' flat list in the commands' place: for n_views views — cascades, cube faces,
 * stereo eyes — ONE call forms the level, the work items and the world box of every (instance, cluster) once, tests them
 * against every view's planes, and writes one list of 16-byte MipClusterEntry and one VkDrawIndirectCommand per view. NOT a
 * reference behaviour; checked against this repository's restatement (tests/cluster_views_list_restatement.py), byte for byte.
 * Every entry point above is unchanged.
 *
 * VIEWS, ONE LOD FOR ALL VIEWS (frames[0].cam_pos), MEMBERS, WORK ITEMS, W and SURVIVES_v are the words of
 * mip_cull_clusters_views, unchanged. There is no pyramid and no cone.
 * ENTRIES: view v's entries are [v * entry_stride, v * entry_stride + entry_counts[v]) of cluster_entries: one
 * MipClusterEntry per work item with SURVIVES_v, in (i, c) order. The fields are mip_list_clusters' with instance =
 * frames[v].first_instance_base + i (wraps as firstInstance does). entry_counts[v] = min(survivors_v, entry_stride); entries
 * at or behind a view's count are never touched.
 * draw_args (optional, n_views x 4 words): draw_args[4v .. 4v+3] = VkDrawIndirectCommand {vertexCount = 192, instanceCount =
 * entry_counts[v], firstVertex = 0, firstInstance = v * entry_stride}. firstInstance is the view's first entry: Vulkan's
 * gl_InstanceIndex includes firstInstance, so every view's shader reads entries[gl_InstanceIndex] from the one buffer.
 * stats (optional, 2 + n_views words): {W, members, survivors_0, survivors_1, ...}.
 * THE CONSUMER: mip_list_clusters' shader, with one vkCmdDrawIndirect(cmd, draw_args, 16 * v, 1, 16) per view into its own
 * target, or one call with drawCount = n_views in a layered pass with gl_DrawID as the view.
 * THE TWO EQUIVALENCES: let f_v = frames[v] with cam_pos replaced by frames[0].cam_pos. (a) View v's entries, entry_counts[v]
 * and survivors_v are byte for byte what mip_list_clusters(ctx, &f_v, visible_bitmaps[v] (a full bitmap where the entry is
 * NULL), policy, NULL, NULL, {entry_capacity = entry_stride}) writes, whenever both calls run. (b) View v's entries are the
 * cluster-by-cluster expansion of view v's command range of mip_cull_clusters_views with the same arguments.
 * ENTRY OVERFLOW (some survivors_v > entry_stride): that view keeps its first entry_stride entries exactly as with room,
 * entry_counts[v] = draw_args[4v+1] = entry_stride, the other views are complete, stats are true, and the status is
 * MIP_ERR_CAPACITY.
 * WORK OVERFLOW (W > work_capacity — 0 = the library's own bound, N x the largest C of the table — or W >= 2^32): every count
 * is 0, draw_args of view v = {192, 0, 0, v * entry_stride}, stats = {W mod 2^32, members, 0, ...}, no entry is written,
 * MIP_ERR_CAPACITY; the context stays usable.
 * WHO REPORTS is mip_cull_clusters_views' rule, on that call's own pair of status words: both several-view calls share the
 * pair. Neither is ever charged to a frame slot's cluster call, nor the other way round.
 * N = 0 writes n_views zero counts, {192, 0, 0, v * entry_stride} per view and zero stats.
 * REFUSED, nothing written, MIP_ERR_INVALID_ARGUMENT: everything mip_cull_clusters_views refuses (cluster_entries,
 * entry_stride and entry_counts in cluster_cmds', cmd_stride's and cmd_counts' places; draw_args 4-byte aligned like the other
 * words); cluster_entries not 16-byte aligned; n_views x entry_stride >= 2^32 (the last view's firstInstance would not fit).
 * MIP_ERR_NOT_READY as for that call.
 * ORDERING: enqueued on the context's first stream, as mip_run_views and mip_cull_clusters_views are. Scratch is the
 * several-view call's own, grown by this call: on top of mip_cull_clusters_views' planes, (1 + n_views) x 4 bytes per 64 work
 * items of the bound. Both several-view calls run on the one stream, so sharing the scratch is ordered.
 * OUT OF SCOPE: a pyramid per view (mip_list_clusters_views_occluded below); cones; the two phases; the per-triangle test (one view: mip_list_cluster_triangles below); one list packed tightly over all views;
 * shards; skinned instances; mip_run_many and recorded graphs. */
typedef struct MipClusterViewListOutputs {
  uint32_t struct_size;      /* = sizeof(MipClusterViewListOutputs) */
  uint32_t flags;            /* MIP_OUT_DEVICE (required) | MIP_OUT_ASYNC */
  void* cluster_entries;     /* DEVICE, 16-byte aligned: n_views x entry_stride MipClusterEntry */
  uint32_t entry_stride;     /* entries reserved per view */
  uint32_t work_capacity;    /* bound on W of the union of the views' members; 0 = N x the largest C */
  uint32_t* entry_counts;    /* DEVICE: n_views words: min(survivors_v, entry_stride) */
  uint32_t* draw_args;       /* DEVICE, optional: n_views x 4 words */
  uint32_t* stats;           /* DEVICE, optional: 2 + n_views words: W, members, survivors_0 ... */
} MipClusterViewListOutputs; /* 48 B */

int32_t mip_list_clusters_views(MipContext* ctx, const MipFrame* frames, const uint32_t* const* visible_bitmaps,
                                uint32_t n_views, const MipLodPolicy* policy, const MipClusterViewListOutputs* out);

/* ---- Extension: visible-cluster lists for several views, a depth pyramid per view ------------------------------------------
 * mip_list_clusters_views with the OCCLUSION TEST behind the plane test of every view that brings a pyramid: a renderer with
 * stereo eyes, cube faces or cascades holds one depth image per view, and ONE call forms the level, the work items and the
 * world box of every (instance, cluster) once, tests them against every view's planes and — for a view with a pyramid —
 * against that view's pyramid, and writes one list of 16-byte MipClusterEntry and one VkDrawIndirectCommand per view. NOT a
 * reference behaviour; checked against this repository's restatement (tests/cluster_views_occluded_restatement.py), byte for
 * byte. Every entry point above is unchanged.
 *
 * BORROWED TERMS: VIEWS, ONE LOD FOR ALL VIEWS (frames[0].cam_pos), MEMBERS (the union of the views' bitmaps, a NULL bitmap
 * counting as every instance), WORK ITEMS, W and the world box are the words of mip_cull_clusters_views, unchanged. A view's
 * pyramid never changes membership, W or the work items.
 * occs: a HOST array of n_views HOST pointers. occs[v] == NULL: view v is tested against its planes alone. A non-NULL entry
 * is read as mip_cull_clusters reads its occ: pyramid, width, height and pv are read; candidates and occluded_bitmap must be
 * NULL and flags 0. Two views may share a pyramid pointer, with the same or different pv.
 * PASSES_v(i, c): bit i of view v is set, AND the shared world box is not culled by the plane test against frames[v].planes
 * (SURVIVES_v of mip_cull_clusters_views).
 * SURVIVES_v(i, c) = PASSES_v(i, c) AND (occs[v] is NULL OR the world box is not occluded under occs[v]). "Occluded" is
 * steps 1-9 of the OCCLUSION TEST above, on the world box, under occs[v]'s pv, pyramid and extents.
 * hidden (optional, n_views words): hidden[v] = the number of work items with PASSES_v and not SURVIVES_v; 0 for a view
 * without a pyramid. An exact integer count whatever the order of execution.
 * ENTRIES, entry_counts, draw_args and stats ({W, members, survivors_0, survivors_1, ...}, 2 + n_views words) are
 * mip_list_clusters_views' rules with this SURVIVES_v; THE CONSUMER is that call's.
 * ENTRY OVERFLOW (some survivors_v > entry_stride): that view keeps its first entry_stride entries exactly as with room,
 * entry_counts[v] = draw_args[4v+1] = entry_stride, the other views are complete, stats and hidden are true, and the status is
 * MIP_ERR_CAPACITY.
 * WORK OVERFLOW (W > work_capacity — 0 = the library's own bound, N x the largest C of the table — or W >= 2^32): every count
 * is 0, draw_args of view v = {192, 0, 0, v * entry_stride}, stats = {W mod 2^32, members, 0, ...}, hidden is all zero, no
 * entry is written, MIP_ERR_CAPACITY; the context stays usable.
 * WHO REPORTS is mip_cull_clusters_views' rule, on the pair of status words both several-view calls already share. None of
 * the several-view calls is ever charged to a frame slot's cluster call, nor the other way round.
 * N = 0 writes n_views zero counts, {192, 0, 0, v * entry_stride} per view, zero stats and zero hidden.
 * THE THREE EQUIVALENCES: let f_v = frames[v] with cam_pos replaced by frames[0].cam_pos. (a) View v's entries,
 * entry_counts[v] and survivors_v are byte for byte what mip_list_clusters(ctx, &f_v, visible_bitmaps[v] (a full bitmap where
 * the entry is NULL), policy, occs[v], NULL, {entry_capacity = entry_stride}) writes, whenever both calls run. (b) With every
 * occs[v] NULL every output is byte for byte mip_list_clusters_views' and hidden is zero. (c) View v's list is a subsequence
 * of the list mip_list_clusters_views writes for view v, and survivors_v + hidden[v] equals that call's survivors_v.
 * REFUSED, nothing written, MIP_ERR_INVALID_ARGUMENT: everything mip_list_clusters_views refuses (n_views x entry_stride >=
 * 2^32 among it); a NULL occs (for no pyramid at all pass an array of NULLs, or use the plain call); any non-NULL entry that
 * mip_cull_clusters would refuse — a wrong struct_size, candidates, occluded_bitmap or flags set, an extent of 0 or above
 * MIP_MAX_DEPTH_EXTENT, a NULL pyramid — and the message names the view; hidden not 4-byte aligned; hidden inside stats,
 * draw_args or entry_counts. MIP_ERR_NOT_READY as for mip_list_clusters_views.
 * ORDERING: enqueued on the context's first stream, as the other several-view calls are. When a non-NULL occs entry exists
 * and the stream of the frame slot the next run takes — where mip_build_depth_pyramid enqueues — is not the first stream, the
 * call goes behind what that stream holds now (an event recorded there, waited for on the device): V pyramids built with
 * mip_build_depth_pyramid (asynchronous) need no mip_wait in front of this call. Scratch is the several-view scratch,
 * unchanged in size: no new plane.
 * OUT OF SCOPE: commands per view under a pyramid; a two-phase record per view; cones; the per-triangle test (one view: mip_list_cluster_triangles below); shards;
 * skinned instances; mip_run_many and recorded graphs. */
typedef struct MipClusterViewOccludedListOutputs {
  uint32_t struct_size;      /* = sizeof(MipClusterViewOccludedListOutputs) */
  uint32_t flags;            /* MIP_OUT_DEVICE (required) | MIP_OUT_ASYNC */
  void* cluster_entries;     /* DEVICE, 16-byte aligned: n_views x entry_stride MipClusterEntry */
  uint32_t entry_stride;     /* entries reserved per view */
  uint32_t work_capacity;    /* bound on W of the union of the views' members; 0 = N x the largest C */
  uint32_t* entry_counts;    /* DEVICE: n_views words: min(survivors_v, entry_stride) */
  uint32_t* draw_args;       /* DEVICE, optional: n_views x 4 words */
  uint32_t* stats;           /* DEVICE, optional: 2 + n_views words: W, members, survivors_0 ... */
  uint32_t* hidden;          /* DEVICE, optional: n_views words: work items that passed view v's planes and are occluded */
} MipClusterViewOccludedListOutputs; /* 56 B */

int32_t mip_list_clusters_views_occluded(MipContext* ctx, const MipFrame* frames, const uint32_t* const* visible_bitmaps,
                                         const MipOcclusion* const* occs, uint32_t n_views, const MipLodPolicy* policy,
                                         const MipClusterViewOccludedListOutputs* out);

/* ---- Extension: the visible-cluster list in two phases ---------------------------------------------------------------------
 * mip_cull_clusters_phase with mip_list_clusters' flat list in the commands' place: FIRST writes one MipClusterEntry per work
 * item that survives under last frame's pyramid and records the items hidden by occlusion alone; SECOND, after the pyramid is
 * rebuilt, writes one entry per recorded item that is visible now — and can append them behind FIRST's entries in the same
 * buffer without the host reading FIRST's count. NOT a reference behaviour; checked against this repository's restatement
 * (tests/cluster_list_phase_restatement.py) only. Every entry point above is unchanged.
 *
 * BORROWED TERMS: MEMBERS, WORK ITEMS, W, SURVIVES, SURVIVES2, THE RECORD (its header, its words, mip_cluster_record_bytes) and
 * the folding of record_bytes into the bound on W are mip_cull_clusters_phase's, unchanged. ENTRIES and their four fields are
 * mip_list_clusters'. frame, visible_bitmap, policy, occ (required) and rec are mip_cull_clusters_phase's.
 * FIRST (rec->phase = MIP_CLUSTER_PHASE_FIRST): one entry per work item with SURVIVES (frame->planes and the pyramid of occ),
 * in (i, c) order. The record is byte for byte what mip_cull_clusters_phase FIRST writes for the same ctx, frame,
 * visible_bitmap, policy, occ and rec, header included. A record written by either call is accepted by SECOND of either call.
 * SECOND (rec->phase = MIP_CLUSTER_PHASE_SECOND): one entry per work item with SURVIVES2 (its record bit is set AND its world
 * box is not occluded under occ, the new pyramid), in (i, c) order. frame->planes is NOT read. The record is never modified.
 * ENTRY BASE: let b = *entry_base, or 0 when entry_base is NULL. b is read ON THE DEVICE when the call's kernels run: behind
 * everything enqueued earlier on that stream, and for SECOND behind the FIRST call (ORDERING). entry_base may therefore be the
 * FIRST call's entry_count. It must not be THIS call's entry_count and must not lie inside this call's draw_args or stats:
 * those are refused. room = entry_capacity - min(b, entry_capacity): entry_capacity counts the BUFFER's entries from entry 0.
 * The entries go to [b, b + entry_count) of cluster_entries, entry_count = min(survivors, room), and nothing outside that
 * range is touched.
 * draw_args (optional, 4 words) = VkDrawIndirectCommand {192, entry_count, 0, b}: firstInstance is the list's first entry, as
 * in mip_list_clusters_views, so the shader reads entries[gl_InstanceIndex]. THE CONSUMER is mip_list_clusters' otherwise.
 * stats (optional, 4 words) = {survivors, W, members, candidates}; candidates is the record header's word: written in FIRST,
 * read in SECOND.
 * ENTRY OVERFLOW (survivors > room): the first `room` entries are written exactly as they would be with room, entry_count =
 * draw_args[1] = room, stats holds the true values, MIP_ERR_CAPACITY. In FIRST the record stays complete and valid.
 * WORK OVERFLOW (as mip_cull_clusters_phase: W > work_capacity or the library's own bound, W >= 2^32, or record_bytes <
 * mip_cluster_record_bytes(W)): MIP_ERR_CAPACITY, entry_count = 0, draw_args = {192, 0, 0, b}, stats = {0, W mod 2^32,
 * members, 0}; no entry is written; FIRST's header becomes {0xFFFFFFFF, 0, 0, 0} and no record word is defined.
 * NOT THIS CALL'S RECORD (SECOND; the header's W or members differs from the call's): MIP_ERR_DEVICE, entry_count = 0,
 * draw_args = {192, 0, 0, b}, stats = {0, W, members, 0} (the call's own); nothing else is written.
 * N = 0: a zero count, {192, 0, 0, b} and zero stats; FIRST writes the header {0, 0, 0, 0}.
 * WHO REPORTS follows mip_cull_clusters: the same per-slot status words, the same mip_wait route (MIP_ERR_DEVICE before
 * MIP_ERR_CAPACITY when asynchronous calls raised both). The context stays usable.
 * REFUSED, nothing written, MIP_ERR_INVALID_ARGUMENT: everything mip_list_clusters (cone == NULL) and mip_cull_clusters_phase
 * refuse (a wrong MipClusterPhaseListOutputs.struct_size in the outputs' place); an entry_base that is this call's entry_count
 * or lies inside its draw_args or stats; an entry_base that is not 4-byte aligned. MIP_ERR_NOT_READY as for those calls.
 * ORDERING: as mip_cull_clusters_phase: both calls go on the stream of the frame issued last; FIRST records the context's
 * record event, SECOND waits for it on the device, so with two frames in flight no host wait is needed between them. Scratch
 * is mip_list_clusters' per frame slot plus one word per list tile.
 * THE FRAME, mip_cull_clusters_phase's four steps with lists: (1) mip_run_occluded with last frame's pyramid, then FIRST over
 * its bitmap with entry_base = NULL; (2) draw FIRST's list, rebuild the pyramid; (3) mip_run_occluded with the inverted
 * candidates, then plain mip_list_clusters over ITS bitmap under the new pyramid into a buffer of its own; (4) SECOND over
 * phase 1's bitmap with entry_base = FIRST's entry_count into FIRST's buffer: one more indirect draw from SECOND's draw_args.
 * OUT OF SCOPE: cones, several views, shards, skinned instances, the per-triangle test (one phase: mip_list_cluster_triangles below), mip_run_many and
 * recorded graphs, and an entry_base for mip_list_clusters. */
typedef struct MipClusterPhaseListOutputs {
  uint32_t struct_size;       /* = sizeof(MipClusterPhaseListOutputs) */
  uint32_t flags;             /* MIP_OUT_DEVICE (required) | MIP_OUT_ASYNC */
  void* cluster_entries;      /* DEVICE, 16-byte aligned: room for entry_capacity MipClusterEntry */
  uint32_t entry_capacity;    /* entries the BUFFER holds, counted from entry 0 */
  uint32_t work_capacity;     /* as MipClusterListOutputs */
  uint32_t* entry_count;      /* DEVICE: entries this call wrote = min(survivors, room) */
  uint32_t* draw_args;        /* DEVICE, optional, 4 words: VkDrawIndirectCommand {192, entry_count, 0, b} */
  uint32_t* stats;            /* DEVICE, optional, 4 words: survivors, W, members, candidates */
  const uint32_t* entry_base; /* DEVICE, optional: the entry this call's list starts at; NULL = 0 */
} MipClusterPhaseListOutputs; /* 56 B */

int32_t mip_list_clusters_phase(MipContext* ctx, const MipFrame* frame, const uint32_t* visible_bitmap, const MipLodPolicy* policy,
                                const MipOcclusion* occ, const MipClusterPhaseListOutputs* out, const MipClusterRecord* rec);

/* ---- Extension: per-triangle masks on the visible-cluster list -------------------------------------------------------------
 * mip_cull_cluster_triangles ends in a dense index stream and commands into it; a consumer of mip_list_clusters' list draws
 * with entries[gl_InstanceIndex] and pulls its own indices, so it wants no stream: it wants, per entry, the 64 bits that say
 * which of the cluster's triangles to emit, and no entry for a cluster that keeps none. mip_list_cluster_triangles is
 * mip_list_clusters with the per-triangle stage's test behind SURVIVES: one MipClusterEntry per surviving work item that keeps a
 * triangle, and beside it one 64-bit TRIANGLE MASK. NOT a reference behaviour; checked against this repository's restatement
 * (tests/cluster_triangle_list_restatement.py) only. Every entry point above is unchanged.
 *
 * MEMBERS, WORK ITEMS, W and SURVIVES are mip_list_clusters' for the same frame, visible_bitmap, policy, occ and cone: the
 * planes, and the pyramid when occ is given; the cone test in front when cone is given.
 * TRI_SURVIVES(i, c, t) is that of mip_cull_cluster_triangles above, unchanged: formed on the matrix mip_run writes for instance
 * i, which the call builds from the instance columns, under frame->pv, the chain with no FMA contraction.
 * MASKS: MASK(i, c) has bit t set iff t is below the triangle count of cluster c (64, or fewer in the last cluster of a level)
 * and TRI_SURVIVES(i, c, t). Bits at or above the triangle count are zero.
 * ENTRIES: one per work item with SURVIVES and MASK != 0, in (i, c) order, packed from entry 0. The four fields are exactly
 * mip_list_clusters' fields, so the entries are a subsequence of that call's list for the same arguments. triangle_masks[k] is
 * the MASK of entry k. entry_count = min(entries, entry_capacity); nothing at or behind entry_count is touched in either array.
 * draw_args (optional, 4 words): VkDrawIndirectCommand {vertexCount = 192, instanceCount = entry_count, 0, 0}.
 * stats (optional, 6 words): {entries, surviving clusters, W, members, surviving triangles, triangles tested}; words 1 to 5 are
 * those of mip_cull_cluster_triangles (with a cone: mip_cull_cluster_triangles_cone) for the same arguments — tested = the
 * triangles of the surviving clusters; the last two mod 2^32.
 * ENTRY OVERFLOW (entries > entry_capacity): the first entry_capacity entries and masks are written exactly as they would be
 * with room, entry_count = entry_capacity and draw_args[1] holds the same value, stats holds the true six values, and the status
 * is MIP_ERR_CAPACITY.
 * WORK OVERFLOW, as mip_list_clusters: MIP_ERR_CAPACITY, entry_count = 0, draw_args = {192, 0, 0, 0},
 * stats = {0, 0, W mod 2^32, members, 0, 0}; nothing else is written and the context stays usable.
 * There is no index overflow: there is no stream. N = 0 writes a zero count, {192, 0, 0, 0} and six zero stats.
 * Both overflows are reported as mip_cull_clusters reports (WHO REPORTS AN OVERFLOW above): the same status words, the same
 * mip_wait route.
 * REFUSED, nothing written: everything mip_list_clusters refuses, what it refuses about a non-NULL cone included; a NULL
 * triangle_masks or one that is not 8-byte aligned; triangle_masks' entry_capacity x 8 bytes overlapping cluster_entries,
 * entry_count, draw_args or stats; a wrong struct_size: MIP_ERR_INVALID_ARGUMENT. MIP_ERR_NOT_READY as for mip_list_clusters.
 * The geometry must be resident (mip_set_geometry), as for mip_cull_cluster_triangles: the cluster table is stale without it.
 * ORDERING and scratch are mip_cull_clusters': the stream of the frame issued last, scratch per frame slot that grows lazily —
 * mip_list_clusters' 8 bytes per 64 work items of the bound, 8 bytes per work item (the triangle word), 8 per 64 work items
 * (which of them are not zero) and a few words per tile — and is freed with the rest.
 *
 * THE CONSUMER: mip_list_clusters' draw and shader, with
 *   uint64_t mask = triangle_masks[gl_InstanceIndex];
 *   if (gl_VertexIndex >= e.index_count || ((mask >> (gl_VertexIndex / 3)) & 1) == 0) gl_Position = vec4(0);   // degenerate
 * in a vertex shader; a mesh shader with one workgroup per entry emits popcount(mask) primitives, the set bits in order.
 * OUT OF SCOPE: a per-entry triangle prefix (a dense stream reconstructed on the device: mip_cull_cluster_triangles writes the
 * stream); the two-phase record; several views; shards; skinned instances; mip_run_many and recorded graphs. */
typedef struct MipClusterTriangleListOutputs {
  uint32_t struct_size;      /* = sizeof(MipClusterTriangleListOutputs) */
  uint32_t flags;            /* MIP_OUT_DEVICE (required) | MIP_OUT_ASYNC */
  void* cluster_entries;     /* DEVICE, 16-byte aligned: room for entry_capacity MipClusterEntry */
  void* triangle_masks;      /* DEVICE, 8-byte aligned: room for entry_capacity uint64_t, mask k beside entry k */
  uint32_t entry_capacity;   /* entries (and masks) that fit */
  uint32_t work_capacity;    /* the caller's bound on W; 0 = N x the largest C of the table */
  uint32_t* entry_count;     /* DEVICE: entries written = min(entries, entry_capacity) */
  uint32_t* draw_args;       /* DEVICE, optional, 4 words: VkDrawIndirectCommand {192, entry_count, 0, 0} */
  uint32_t* stats;           /* DEVICE, optional, 6 words */
} MipClusterTriangleListOutputs; /* 56 B */
int32_t mip_list_cluster_triangles(MipContext* ctx, const MipFrame* frame, const uint32_t* visible_bitmap, const MipLodPolicy* policy,
                                   const MipOcclusion* occ /* or NULL */, const MipClusterCone* cone /* or NULL */,
                                   const MipClusterTriangleListOutputs* out);

/* Block until everything enqueued by this context has finished; reports a
 * deferred error of an async run (MIP_ERR_CAPACITY, MIP_ERR_DEVICE, MIP_ERR_TIMEOUT of an external semaphore).
 * Frames ordered by external semaphores still need this call at a bounded cadence (e.g. every
 * frames_in_flight frames): it is where their errors surface. The MIP_ERR_CAPACITY of an asynchronous
 * mip_cull_clusters, mip_list_clusters, mip_list_cluster_triangles, mip_list_clusters_phase, mip_cull_clusters_views, mip_list_clusters_views or mip_list_clusters_views_occluded (and the MIP_ERR_DEVICE of an asynchronous SECOND call of mip_cull_clusters_phase or mip_list_clusters_phase) is returned
 * when there is no other error to return; otherwise by the mip_wait after. */
int32_t mip_wait(MipContext* ctx);

/* Merge `n_chunks` shard draw lists (each: MipShardHeader followed by its commands,
 * chunks `chunk_stride_bytes` apart, as an all-gather lays them out; DEVICE memory) into
 * one contiguous list in shard order, adding to each shard's firstIndex the
 * draw_index_total of all earlier shards. out_count[0] = total commands,
 * out_count[1] = total indices (so out_count needs room for 2 words). DEVICE pointers. Enqueued on the
 * context's first stream (MipConfig.stream, or frame slot 0's): it is ordered after a frame of the same
 * context only when frames_in_flight == 1 — use one context per frame in flight for sharded frames, as
 * mip_run_sharded and renderer_amd/sharded.py do. Synchronous unless `async` is non-zero.
 * `chunk_capacity` = commands one chunk may carry (0 = what the stride holds): `out_cmds` needs room for
 * n_chunks x chunk_capacity commands, and a chunk whose header count exceeds it is cut there and
 * reported (MIP_ERR_CAPACITY from this call, or from mip_wait for an async one) — the stride is
 * usually rounded up and may physically hold a few commands more than the capacity. */
int32_t mip_merge_draw_lists(MipContext* ctx, const void* chunks, uint32_t n_chunks,
                             uint64_t chunk_stride_bytes, uint32_t chunk_capacity, void* out_cmds,
                             uint32_t* out_count, int32_t async);

/* The same merge for chunks in the WIRE form (each: MipShardHeader followed by a wire body, see
 * MIP_OUT_WIRE): every record is expanded against THIS context's mesh table — which must be the table
 * the emitting ranks ran with; it is replicated by construction — into the 20-byte
 * command, and the result is byte-identical to mip_merge_draw_lists over the 20-byte chunks of the
 * same frames. chunk_stride_bytes >= sizeof(MipShardHeader) + MIP_WIRE_BODY_BYTES(chunk_capacity);
 * chunk_capacity = 0 means what the stride holds in whole blocks. A record whose mesh id is outside the table (a corrupt chunk)
 * is expanded as mesh 0 and reported as MIP_ERR_DEVICE. */
int32_t mip_merge_wire_lists(MipContext* ctx, const void* chunks, uint32_t n_chunks,
                             uint64_t chunk_stride_bytes, uint32_t chunk_capacity, void* out_cmds,
                             uint32_t* out_count, int32_t async);
/* ... and for chunks in the PACKED wire form (MIP_OUT_WIRE_PACKED; chunk_stride_bytes >= sizeof(MipShardHeader) +
 * MIP_WIRE_PACKED_BODY_BYTES(chunk_capacity)). Each block header carries its own index_bits; one that cannot be (> 31)
 * is a corrupt chunk and reported like a bad mesh id. */
int32_t mip_merge_wire_lists_packed(MipContext* ctx, const void* chunks, uint32_t n_chunks,
                                    uint64_t chunk_stride_bytes, uint32_t chunk_capacity, void* out_cmds,
                                    uint32_t* out_count, int32_t async);

/* ---- sharded scenes without a Python host: RCCL straight from the library ------------------
 * librccl.so.1 is opened with dlopen on first use, so single-GPU hosts do not need it. The
 * exchange is the one of SURVEY.md §8e: every rank runs its shard, ONE ncclAllGather moves the
 * fixed-size chunks [MipShardHeader | wire body for chunk_capacity commands: 4.25 B each (packed form; 8.06 B when the
 * largest shard does not fit a packed record) instead of 20, see MIP_OUT_WIRE], the merge kernel expands and concatenates them. Needs a context with one frame in flight. */
#define MIP_COMM_ID_BYTES 128u

/* ncclGetUniqueId: call on one rank, hand the 128 bytes to the others by any means. */
int32_t mip_comm_unique_id(uint8_t out_id[MIP_COMM_ID_BYTES]);
/* ncclCommInitRank on the context's device: collective over all `world` ranks. */
int32_t mip_comm_init(MipContext* ctx, const uint8_t id[MIP_COMM_ID_BYTES], uint32_t rank, uint32_t world);
int32_t mip_comm_destroy(MipContext* ctx);

typedef struct MipShardedOutputs {
  void* model;              /* this rank's shard: n_local x mat4, or NULL */
  uint32_t* visible_bitmap; /* this rank's shard, or NULL */
  void* world_aabb;         /* this rank's shard, or NULL */
  void* draw_cmds;          /* the MERGED global list; room for world x chunk_capacity commands */
  uint32_t* draw_count;     /* [0] merged command count, [1] merged index total */
  uint32_t chunk_capacity;  /* commands each rank contributes at most; 0 = the largest max_instances over the ranks
                               (mip_comm_init settles on it with a 4-byte all-gather, so ranks created for
                               shards of different sizes still exchange chunks of one size).
                               If ANY rank emits more, every rank sees it in the gathered headers and the
                               library repeats the all-gather + merge of that frame once at full capacity
                               (at once for a synchronous call, inside mip_wait for an asynchronous one;
                               MipTimings.sharded_retries counts them): draw_cmds therefore needs room for
                               world x (largest max_instances) commands whenever chunk_capacity is tightened */
  uint32_t flags;           /* MIP_OUT_DEVICE, optionally | MIP_OUT_ASYNC */
} MipShardedOutputs;

/* One frame of a sharded scene on this rank (collective: every rank calls it with the same
 * chunk_capacity). frame->first_instance_base must be the shard's first draw_index. With
 * MIP_OUT_ASYNC and a tightened chunk_capacity call mip_wait before the next sharded frame: the
 * repair of an overflowing frame re-sends this rank's list, which the next frame overwrites
 * (an overflow that can no longer be repaired is reported as MIP_ERR_CAPACITY). */
int32_t mip_run_sharded(MipContext* ctx, const MipFrame* frame, const MipShardedOutputs* out);

/* ---- zero-copy interop with the renderer's own allocations ----------------
 * The reference keeps the buffers this path fills in VMA allocations of its Vulkan device:
 * ModelData.model_buffer (src/renderer.rs:1225-1265), IndirectCommandsBuffer / IndirectCommandsCount
 * (src/renderer/systems/cull_pipeline.rs:70-72,183-220), declared GPU_ONLY by the buffer macro
 * (src/renderer/macros/macros.rs:67-79) on an allocator created without exportable handle types
 * (src/renderer/device/alloc.rs:154-171). Once such a buffer is allocated from a memory block created
 * with VkExportMemoryAllocateInfo{handleTypes = VK_EXTERNAL_MEMORY_HANDLE_TYPE_OPAQUE_FD_BIT} (on amdgpu
 * the fd is a dma-buf; INTEGRATION.md §3 lists the VMA / Vulkan flags) and exported with
 * vkGetMemoryFdKHR, this call maps the same bytes into the context's HIP device:
 * hipImportExternalMemory(OpaqueFd) + hipExternalMemoryGetMappedBuffer. `*out_device_ptr` is then a
 * valid MIP_OUT_DEVICE output pointer (or mip_set_instances_device input) for `size_bytes` bytes.
 * As with cudaImportExternalMemory, a successfully imported fd belongs to the driver: do not use or
 * close it afterwards. Ordering against the Vulkan queue: the semaphore entry points below, or
 * vkQueueWaitIdle / mip_wait at the hand-over points. */
int32_t mip_import_external_fd(MipContext* ctx, int32_t fd, uint64_t size_bytes, void** out_device_ptr);
/* Unmaps a pointer returned by mip_import_external_fd (after mip_wait); mip_destroy releases the rest. */
int32_t mip_release_external(MipContext* ctx, void* device_ptr);

/* ---- the semaphore half of the same interop -------------------------------------------------------
 * The reference orders its passes with TIMELINE semaphores, one per frame-graph pass, signalled and
 * waited with a value derived from the frame number (src/renderer.rs:3757-3861, AutoSemaphores;
 * `ComputeCull` is the pass this library replaces and the graphics submit waits for it). A semaphore
 * created with VkExportSemaphoreCreateInfo{handleTypes = OPAQUE_FD_BIT} (+ VkSemaphoreTypeCreateInfo
 * {TIMELINE}) and exported with vkGetSemaphoreFdKHR is imported here with hipImportExternalSemaphore;
 * the library then takes the place of the ComputeCull submit:
 *
 *   mip_wait_external(ctx, sem_prev, value)   the stream the NEXT frame will run on waits, on the device,
 *                                             until the semaphore reaches `value` (the reader of the
 *                                             buffers this frame overwrites has finished)
 *   mip_run(ctx, frame, outs | MIP_OUT_ASYNC)
 *   mip_signal_external(ctx, sem_cull, value) enqueued behind the frame that was issued LAST: the
 *                                             semaphore reaches `value` when its kernels have finished
 *
 * and the graphics submit lists sem_cull/value as a wait semaphore: no host wait per frame.
 * kind: MIP_SEMAPHORE_TIMELINE (what the reference uses) or MIP_SEMAPHORE_BINARY (`value` ignored).
 * As with memory, a successfully imported fd belongs to the library. Two implementations sit behind the
 * handle: the HIP runtime's (waits and signals execute on the device) when it accepts the handle type, and
 * otherwise — ROCm 7.2 on Linux refuses both: TimelineSemaphoreFd "invalid argument", OpaqueFd "operation
 * not supported" — the kernel object itself: on amdgpu the exported fd IS a DRM sync object, which the
 * library imports on a render node (DRM_IOCTL_SYNCOBJ_FD_TO_HANDLE) and waits for / signals from host
 * functions enqueued on the frame's stream (hipLaunchHostFunc: stream-ordered, no wait on the caller's
 * thread; a wait is bounded at 10 s and then reported by mip_wait as MIP_ERR_TIMEOUT).
 * mip_external_semaphore_on_device tells which one a handle got (1 = HIP runtime, 0 = host functions).
 * Errors: MIP_ERR_INVALID_ARGUMENT for a bad fd / kind / a handle this context did not import;
 * MIP_ERR_DEVICE with the runtime's message when neither path accepts the fd. */
#define MIP_SEMAPHORE_BINARY 0u
#define MIP_SEMAPHORE_TIMELINE 1u
typedef struct MipExternalSemaphore MipExternalSemaphore; /* opaque */
int32_t mip_import_external_semaphore_fd(MipContext* ctx, int32_t fd, uint32_t kind, MipExternalSemaphore** out_semaphore);
int32_t mip_external_semaphore_on_device(MipContext* ctx, MipExternalSemaphore* semaphore);
int32_t mip_wait_external(MipContext* ctx, MipExternalSemaphore* semaphore, uint64_t value);
int32_t mip_signal_external(MipContext* ctx, MipExternalSemaphore* semaphore, uint64_t value);
/* After mip_wait; mip_destroy releases the rest. */
int32_t mip_release_external_semaphore(MipContext* ctx, MipExternalSemaphore* semaphore);

const char* mip_last_error(const MipContext* ctx);
int32_t mip_get_timings(MipContext* ctx, MipTimings* out);  /* touches the device: a blocking 4-byte read of the help counter */
int32_t mip_reset_timings(MipContext* ctx);                /* (the same read: prefix_helps counts from here on, also with frames in flight) */

/* Number of instances currently resident (set by mip_set_instances*). */
uint32_t mip_instance_count(const MipContext* ctx);

#ifdef __cplusplus
}
#endif
#endif /* MI_INSTANCE_PIPELINE_H */
