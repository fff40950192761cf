//! Raw bindings of include/mi_instance_pipeline.h (what bindgen would generate) plus the
//! newtype that makes the context usable as a bevy resource, like `VmaAllocator` in
//! vma/src/lib.rs:31-40.
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_void};

pub const MIP_OK: i32 = 0;
pub const MIP_OUT_HOST: u32 = 0;
pub const MIP_OUT_DEVICE: u32 = 1;
pub const MIP_OUT_ASYNC: u32 = 2;
pub const MIP_OUT_WIRE: u32 = 4;
pub const MIP_OUT_WIRE_PACKED: u32 = 8;
pub const MIP_SEMAPHORE_BINARY: u32 = 0;
pub const MIP_SEMAPHORE_TIMELINE: u32 = 1;
pub const MIP_MAX_LODS: usize = 6;

#[repr(C)]
pub struct MipContext {
    _private: [u8; 0],
}

/// Opaque handle of an imported external semaphore (mip_import_external_semaphore_fd).
#[repr(C)]
pub struct MipExternalSemaphore {
    _private: [u8; 0],
}

#[repr(transparent)]
pub struct Pipeline(pub *mut MipContext);
unsafe impl Send for Pipeline {}
unsafe impl Sync for Pipeline {}

#[repr(C)]
pub struct MipConfig {
    pub struct_size: u32,
    pub device_ordinal: i32,
    pub max_instances: u32,
    pub max_meshes: u32,
    pub flags: u32,
    pub frames_in_flight: u32,
    pub stream: *mut c_void,
}

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct MipMesh {
    pub aabb_min: [f32; 3],
    pub aabb_max: [f32; 3],
    pub n_lods: u32,
    pub index_len: [u32; MIP_MAX_LODS],
    pub index_offset: [u32; MIP_MAX_LODS],
    pub vertex_offset: i32,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct MipDrawIndexedIndirectCommand {
    pub index_count: u32,
    pub instance_count: u32,
    pub first_index: u32,
    pub vertex_offset: i32,
    pub first_instance: u32,
}

#[repr(C)]
pub struct MipFrame {
    pub planes: [f32; 24],
    pub cam_pos: [f32; 3],
    pub first_instance_base: u32,
    pub first_index_base: u32,
    pub pv: [f32; 16],
}

#[repr(C)]
pub struct MipOutputs {
    pub model: *mut c_void,
    pub visible_bitmap: *mut u32,
    pub draw_cmds: *mut c_void,
    pub draw_count: *mut u32,
    pub draw_index_total: *mut u32,
    pub world_aabb: *mut c_void,
    pub flags: u32,
    pub reserved: u32,
    pub culled_index_buffer: *mut c_void,
    pub culled_index_capacity: u64,
    pub tlas_instances: *mut c_void,
}

#[repr(C)]
pub struct MipShardedOutputs {
    pub model: *mut c_void,
    pub visible_bitmap: *mut u32,
    pub world_aabb: *mut c_void,
    pub draw_cmds: *mut c_void,
    pub draw_count: *mut u32,
    pub chunk_capacity: u32,
    pub flags: u32,
}

/// Extension (not a reference behaviour): outputs of the batched draws, device pointers (see the header).
#[repr(C)]
pub struct MipBatchOutputs {
    pub struct_size: u32,
    pub flags: u32,
    pub batch_cmds: *mut c_void,
    pub batch_count: *mut u32,
    pub instance_ids: *mut u32,
    pub instance_count: *mut u32,
    pub batch_model: *mut c_void,
}

pub const MIP_LOD_DISTANCE: u32 = 0;
pub const MIP_LOD_RELATIVE: u32 = 1;

/// The selection rule of mip_batch_draws_lods: LOD k+1 replaces LOD k beyond switch_sq[k], a SQUARED metric.
#[repr(C)]
pub struct MipLodPolicy {
    pub struct_size: u32,
    pub mode: u32,
    pub switch_sq: [f32; 5],
}

/// The order of the members inside a bucket (mip_batch_draws_ordered).
pub const MIP_BATCH_ORDER_DRAW_INDEX: u32 = 0;
pub const MIP_BATCH_ORDER_NEAR_FIRST: u32 = 1;
pub const MIP_BATCH_ORDER_FAR_FIRST: u32 = 2;

/// The depth metric of mip_batch_draws_sorted.
pub const MIP_DEPTH_RADIAL: u32 = 0;
pub const MIP_DEPTH_VIEW_AXIS: u32 = 1;

/// The depth key of mip_batch_draws_sorted: metric, order (NEAR_FIRST / FAR_FIRST), the leading bits that are sorted (16, 24 or
/// 32) and, for MIP_DEPTH_VIEW_AXIS, the view direction.
#[repr(C)]
pub struct MipSortPolicy {
    pub struct_size: u32,
    pub metric: u32,
    pub order: u32,
    pub depth_bits: u32,
    pub axis: [f32; 3],
}

/// What a shard's batch chunk starts with (mip_batch_draws_shard / mip_merge_batches): then `n_buckets` counts, zero words up
/// to a multiple of 16 bytes, and the ids.
#[repr(C)]
pub struct MipBatchChunkHeader {
    pub members: u32,
    pub n_buckets: u32,
    pub reserved: [u32; 2],
}
pub const MIP_MAX_BATCH_CHUNKS: u32 = 64;
/// MIP_BATCH_CHUNK_IDS_OFFSET: bytes in front of the ids of a chunk for a table of `buckets` buckets.
pub const fn mip_batch_chunk_ids_offset(buckets: u64) -> u64 { 16 + (buckets + (4 - buckets % 4) % 4) * 4 }
/// MIP_BATCH_CHUNK_BYTES: bytes of a chunk with room for `capacity` ids.
pub const fn mip_batch_chunk_bytes(buckets: u64, capacity: u64) -> u64 { mip_batch_chunk_ids_offset(buckets) + capacity * 4 }

/// Outputs of mip_batch_draws_views: every view's commands in its own range of `batch_cmds`, one shared `instance_ids`.
#[repr(C)]
pub struct MipViewBatchOutputs {
    pub struct_size: u32,
    pub flags: u32,
    pub batch_cmds: *mut c_void,
    pub cmd_stride: u32,
    pub reserved: u32,
    pub batch_counts: *mut u32,
    pub instance_ids: *mut u32,
    pub view_first_slot: *mut u32,
}

/// Triangles per cluster of mip_build_clusters.
pub const MIP_CLUSTER_TRIANGLES: u32 = 64;

/// Outputs of mip_cull_clusters: one command per run of surviving clusters, device pointers (see the header).
#[repr(C)]
pub struct MipClusterOutputs {
    pub struct_size: u32,
    pub flags: u32,
    pub cluster_cmds: *mut c_void,
    pub cmd_capacity: u32,
    pub work_capacity: u32,
    pub cmd_count: *mut u32,
    pub stats: *mut u32,
}

/// Outputs of mip_cull_clusters_views: view v's commands start at entry v x cmd_stride, device pointers (see the header).
#[repr(C)]
pub struct MipClusterViewOutputs {
    pub struct_size: u32,
    pub flags: u32,
    pub cluster_cmds: *mut c_void,
    pub cmd_stride: u32,
    pub work_capacity: u32,
    pub cmd_counts: *mut u32,
    pub stats: *mut u32,
}

/// Outputs of mip_cull_cluster_triangles: MipClusterOutputs' fields, then the culled index stream (see the header).
#[repr(C)]
pub struct MipClusterTriangleOutputs {
    pub struct_size: u32,
    pub flags: u32,
    pub cluster_cmds: *mut c_void,
    pub cmd_capacity: u32,
    pub work_capacity: u32,
    pub cmd_count: *mut u32,
    pub stats: *mut u32,
    pub culled_indices: *mut c_void,
    pub index_capacity: u32,
}

/// Phases of mip_cull_clusters_phase.
pub const MIP_CLUSTER_PHASE_FIRST: u32 = 1;
pub const MIP_CLUSTER_PHASE_SECOND: u32 = 2;

/// The record of mip_cull_clusters_phase: written by FIRST, read by SECOND; the caller's device memory, 16-byte aligned.
#[repr(C)]
pub struct MipClusterRecord {
    pub struct_size: u32,
    pub phase: u32,
    pub record: *mut c_void,
    pub record_bytes: u64,
}

/// The view's side of the normal-cone back-face test (mip_cull_clusters_cone): the point the view projects from and the
/// sign of its determinant, +1.0 or -1.0. mip_cone_from_pv fills it from a projection.
#[repr(C)]
pub struct MipClusterCone {
    pub struct_size: u32,
    pub flags: u32,
    pub eye: [f32; 3],
    pub facing: f32,
}

/// One entry of mip_list_clusters' list: what a one-cluster command of mip_cull_clusters holds; the vertex shader reads it
/// by gl_InstanceIndex and pulls indices[first_index + gl_VertexIndex] + vertex_offset while gl_VertexIndex < index_count.
#[repr(C)]
pub struct MipClusterEntry {
    pub instance: u32,
    pub first_index: u32,
    pub vertex_offset: i32,
    pub index_count: u32,
}

/// Outputs of mip_list_clusters: the flat list of surviving clusters and the one VkDrawIndirectCommand over it, device
/// pointers (see the header).
#[repr(C)]
pub struct MipClusterListOutputs {
    pub struct_size: u32,
    pub flags: u32,
    pub cluster_entries: *mut c_void,
    pub entry_capacity: u32,
    pub work_capacity: u32,
    pub entry_count: *mut u32,
    pub draw_args: *mut u32,
    pub stats: *mut u32,
}

/// Outputs of mip_list_cluster_triangles: mip_list_clusters' list restricted to the clusters that keep a triangle, and beside
/// entry k the 64-bit mask of its cluster's surviving triangles; six stats words (see the header).
#[repr(C)]
pub struct MipClusterTriangleListOutputs {
    pub struct_size: u32,
    pub flags: u32,
    pub cluster_entries: *mut c_void,
    pub triangle_masks: *mut c_void,
    pub entry_capacity: u32,
    pub work_capacity: u32,
    pub entry_count: *mut u32,
    pub draw_args: *mut u32,
    pub stats: *mut u32,
}

/// Outputs of mip_list_clusters_views: one list of surviving clusters and one VkDrawIndirectCommand per view, device pointers;
/// view v's entries start at entry v x entry_stride, which is also firstInstance of its draw (see the header).
#[repr(C)]
pub struct MipClusterViewListOutputs {
    pub struct_size: u32,
    pub flags: u32,
    pub cluster_entries: *mut c_void,
    pub entry_stride: u32,
    pub work_capacity: u32,
    pub entry_counts: *mut u32,
    pub draw_args: *mut u32,
    pub stats: *mut u32,
}

/// Outputs of mip_list_clusters_views_occluded: MipClusterViewListOutputs' fields and `hidden`, optional, n_views words: per
/// view the work items that passed the view's planes and are occluded under the view's pyramid (see the header).
#[repr(C)]
pub struct MipClusterViewOccludedListOutputs {
    pub struct_size: u32,
    pub flags: u32,
    pub cluster_entries: *mut c_void,
    pub entry_stride: u32,
    pub work_capacity: u32,
    pub entry_counts: *mut u32,
    pub draw_args: *mut u32,
    pub stats: *mut u32,
    pub hidden: *mut u32,
}

/// Outputs of mip_list_clusters_phase: mip_list_clusters' list in two phases. The list starts at entry *entry_base, read on
/// the device (null: 0) — SECOND appends behind FIRST with entry_base = FIRST's entry_count; stats has four words (see the header).
#[repr(C)]
pub struct MipClusterPhaseListOutputs {
    pub struct_size: u32,
    pub flags: u32,
    pub cluster_entries: *mut c_void,
    pub entry_capacity: u32,
    pub work_capacity: u32,
    pub entry_count: *mut u32,
    pub draw_args: *mut u32,
    pub stats: *mut u32,
    pub entry_base: *const u32,
}

/// Per-frame parameters of the occlusion test (mip_cull_clusters reads pyramid, width, height and pv).
#[repr(C)]
pub struct MipOcclusion {
    pub struct_size: u32,
    pub width: u32,
    pub height: u32,
    pub flags: u32,
    pub pyramid: *const c_void,
    pub candidates: *const u32,
    pub occluded_bitmap: *mut u32,
    pub pv: [f32; 16],
}

extern "C" {
    pub fn mip_abi_version() -> u32;
    pub fn mip_create(cfg: *const MipConfig, out: *mut *mut MipContext) -> i32;
    pub fn mip_destroy(ctx: *mut MipContext);
    pub fn mip_set_mesh_table(ctx: *mut MipContext, meshes: *const MipMesh, m: u32) -> i32;
    pub fn mip_set_instances(ctx: *mut MipContext, pos_xyz: *const f32, rot_ijkw: *const f32, scale: *const f32,
                             mesh_id: *const u32, n: u32) -> i32;
    pub fn mip_update_instances(ctx: *mut MipContext, first: u32, count: u32, pos_xyz: *const f32, rot_ijkw: *const f32,
                                scale: *const f32, mesh_id: *const u32) -> i32;
    pub fn mip_set_geometry(ctx: *mut MipContext, vertex_xyz: *const f32, n_vertices: u32, indices: *const u32,
                            n_indices: u32) -> i32;
    pub fn mip_set_blas_addresses(ctx: *mut MipContext, addresses: *const u64, m: u32) -> i32;
    pub fn mip_run(ctx: *mut MipContext, frame: *const MipFrame, out: *const MipOutputs) -> i32;
    /// Step k runs frames[k % n_frames] into outputs[k % n_outputs]; recorded launch graphs do not bake the frame.
    pub fn mip_run_many(ctx: *mut MipContext, frames: *const MipFrame, n_frames: u32, outputs: *const MipOutputs,
                        n_outputs: u32, steps: u32) -> i32;
    pub fn mip_wait(ctx: *mut MipContext) -> i32;
    pub fn mip_merge_draw_lists(ctx: *mut MipContext, chunks: *const c_void, n_chunks: u32, chunk_stride_bytes: u64,
                                chunk_capacity: u32, out_cmds: *mut c_void, out_count: *mut u32, async_: i32) -> i32;
    /// The same merge over chunks in the wire form (MIP_OUT_WIRE: 8-byte records, expanded against the mesh table).
    pub fn mip_merge_wire_lists(ctx: *mut MipContext, chunks: *const c_void, n_chunks: u32, chunk_stride_bytes: u64,
                                chunk_capacity: u32, out_cmds: *mut c_void, out_count: *mut u32, async_: i32) -> i32;
    /// ... and in the packed wire form (MIP_OUT_WIRE_PACKED: one 32-bit record per command).
    pub fn mip_merge_wire_lists_packed(ctx: *mut MipContext, chunks: *const c_void, n_chunks: u32, chunk_stride_bytes: u64,
                                       chunk_capacity: u32, out_cmds: *mut c_void, out_count: *mut u32, async_: i32) -> i32;
    /// Bits of a packed record left for the instance index by a table of `n_meshes` entries.
    pub fn mip_wire_index_bits(n_meshes: u32) -> u32;
    /// Shadow pass (shadow_mapping.rs:405-478): n_lights x n commands, light-major, into device memory.
    pub fn mip_light_draw_lists(ctx: *mut MipContext, light_pos_xyz: *const f32, n_lights: u32, first_instance_base: u32,
                                out_cmds: *mut c_void, async_: i32) -> i32;
    /// Extension (not a reference behaviour): skinned instances, see the header.
    pub fn mip_set_skeleton(ctx: *mut MipContext, parent: *const i32, inverse_bind: *const f32, joint_box: *const f32,
                            n_joints: u32) -> i32;
    pub fn mip_set_poses(ctx: *mut MipContext, joint_trs: *const c_void, n: u32, device: i32) -> i32;
    pub fn mip_run_skinned(ctx: *mut MipContext, frame: *const MipFrame, out: *const MipOutputs, palette: *mut c_void) -> i32;
    /// Up to 4 culled views (per-light lists, cascades) of the resident instances in one launch.
    pub fn mip_run_views(ctx: *mut MipContext, frames: *const MipFrame, outs: *const MipOutputs, n_views: u32) -> i32;
    pub fn mip_comm_unique_id(out_id: *mut u8) -> i32;
    pub fn mip_comm_init(ctx: *mut MipContext, id: *const u8, rank: u32, world: u32) -> i32;
    pub fn mip_comm_destroy(ctx: *mut MipContext) -> i32;
    pub fn mip_run_sharded(ctx: *mut MipContext, frame: *const MipFrame, out: *const MipShardedOutputs) -> i32;
    /// Row f-2: map an fd exported with vkGetMemoryFdKHR (OPAQUE_FD; a dma-buf on amdgpu) into the HIP device.
    pub fn mip_import_external_fd(ctx: *mut MipContext, fd: i32, size_bytes: u64, out_device_ptr: *mut *mut c_void) -> i32;
    pub fn mip_release_external(ctx: *mut MipContext, device_ptr: *mut c_void) -> i32;
    /// Row f-2, the semaphore half: a timeline semaphore exported with vkGetSemaphoreFdKHR (renderer.rs:3757-3861).
    pub fn mip_import_external_semaphore_fd(ctx: *mut MipContext, fd: i32, kind: u32, out_semaphore: *mut *mut MipExternalSemaphore) -> i32;
    /// 1: the HIP runtime imported it (device-side waits); 0: the DRM sync object path (host functions on the stream).
    pub fn mip_external_semaphore_on_device(ctx: *mut MipContext, semaphore: *mut MipExternalSemaphore) -> i32;
    /// The next frame's stream waits on the device until the semaphore reaches `value`.
    pub fn mip_wait_external(ctx: *mut MipContext, semaphore: *mut MipExternalSemaphore, value: u64) -> i32;
    /// Signals `value` behind the frame issued last.
    pub fn mip_signal_external(ctx: *mut MipContext, semaphore: *mut MipExternalSemaphore, value: u64) -> i32;
    pub fn mip_release_external_semaphore(ctx: *mut MipContext, semaphore: *mut MipExternalSemaphore) -> i32;
    /// Extension: one instanced command per (mesh, LOD) bucket over the whole LOD chain, LODs chosen by `policy`.
    pub fn mip_batch_draws_lods(ctx: *mut MipContext, frame: *const MipFrame, visible_bitmap: *const u32,
                                policy: *const MipLodPolicy, out: *const MipBatchOutputs) -> i32;
    /// Extension: mip_batch_draws_lods with the members of every bucket nearest first or farthest first (MIP_BATCH_ORDER_*).
    pub fn mip_batch_draws_ordered(ctx: *mut MipContext, frame: *const MipFrame, visible_bitmap: *const u32,
                                   policy: *const MipLodPolicy, order: u32, out: *const MipBatchOutputs) -> i32;
    /// Extension: the members of mip_batch_draws_lods in one depth order across all buckets, one command per run of equal bucket.
    pub fn mip_batch_draws_sorted(ctx: *mut MipContext, frame: *const MipFrame, visible_bitmap: *const u32,
                                  policy: *const MipLodPolicy, sort: *const MipSortPolicy, out: *const MipBatchOutputs) -> i32;
    /// Extension: mip_batch_draws_lods for up to MIP_MAX_VIEWS views in one call; `visible_bitmaps` is a host array of
    /// `n_views` device pointers (null: every resident instance).
    pub fn mip_batch_draws_views(ctx: *mut MipContext, frames: *const MipFrame, visible_bitmaps: *const *const u32,
                                 n_views: u32, policy: *const MipLodPolicy, out: *const MipViewBatchOutputs) -> i32;
    pub fn mip_batch_draws_shard(ctx: *mut MipContext, frame: *const MipFrame, visible_bitmap: *const u32, policy: *const MipLodPolicy,
                                 chunk: *mut c_void, ids_capacity: u32, flags: u32) -> i32;
    pub fn mip_merge_batches(ctx: *mut MipContext, chunks: *const c_void, n_chunks: u32, chunk_stride_bytes: u64, chunk_capacity: u32,
                             out: *const MipBatchOutputs) -> i32;
    /// Extension: cluster culling. The table of 64-triangle clusters of every level, built on the device from the resident geometry.
    pub fn mip_build_clusters(ctx: *mut MipContext) -> i32;
    pub fn mip_cluster_count(ctx: *const MipContext) -> u32;
    pub fn mip_read_cluster_boxes(ctx: *mut MipContext, host_out: *mut f32, capacity_clusters: u32) -> i32;
    /// The frustum test and (occ non-null) the Hi-Z test per cluster of every member; one command per run of survivors.
    pub fn mip_cull_clusters(ctx: *mut MipContext, frame: *const MipFrame, visible_bitmap: *const u32, policy: *const MipLodPolicy,
                             occ: *const MipOcclusion, out: *const MipClusterOutputs) -> i32;
    /// 16 + 8 x ceil(work_items / 64): the bytes of a record. Pure.
    pub fn mip_cluster_record_bytes(work_items: u64) -> u64;
    /// mip_cull_clusters in two phases: FIRST records the clusters the Hi-Z test alone removed, SECOND tests them again.
    pub fn mip_cull_clusters_phase(ctx: *mut MipContext, frame: *const MipFrame, visible_bitmap: *const u32, policy: *const MipLodPolicy,
                                   occ: *const MipOcclusion, out: *const MipClusterOutputs, rec: *const MipClusterRecord) -> i32;
    /// mip_cull_clusters, then the per-triangle test on the surviving clusters: one culled index stream, commands into it.
    pub fn mip_cull_cluster_triangles(ctx: *mut MipContext, frame: *const MipFrame, visible_bitmap: *const u32, policy: *const MipLodPolicy,
                                      occ: *const MipOcclusion, out: *const MipClusterTriangleOutputs) -> i32;
    /// Extension: normal cones. One cone per cluster of a valid cluster table; stale with that table.
    pub fn mip_build_cluster_cones(ctx: *mut MipContext) -> i32;
    pub fn mip_read_cluster_cones(ctx: *mut MipContext, host_out: *mut f32, capacity_clusters: u32) -> i32;
    /// Pure host: the eye and the facing of a projection (rows x, y, w of pv), in double, rounded once.
    pub fn mip_cone_from_pv(pv: *const f32, out: *mut MipClusterCone) -> i32;
    /// mip_cull_clusters / mip_cull_cluster_triangles with the cone's back-face test in front of the box tests.
    pub fn mip_cull_clusters_cone(ctx: *mut MipContext, frame: *const MipFrame, visible_bitmap: *const u32, policy: *const MipLodPolicy,
                                  occ: *const MipOcclusion, cone: *const MipClusterCone, out: *const MipClusterOutputs) -> i32;
    pub fn mip_cull_cluster_triangles_cone(ctx: *mut MipContext, frame: *const MipFrame, visible_bitmap: *const u32, policy: *const MipLodPolicy,
                                           occ: *const MipOcclusion, cone: *const MipClusterCone, out: *const MipClusterTriangleOutputs) -> i32;
    /// mip_cull_clusters' frustum test for up to MIP_MAX_VIEWS views in one call: one LOD (frames[0].cam_pos) and one world box
    /// per work item for all views, planes and first_instance_base per view; on the first stream, behind mip_run_views.
    pub fn mip_cull_clusters_views(ctx: *mut MipContext, frames: *const MipFrame, visible_bitmaps: *const *const u32,
                                   n_views: u32, policy: *const MipLodPolicy, out: *const MipClusterViewOutputs) -> i32;
    /// mip_cull_clusters (cone null) or mip_cull_clusters_cone with one 16-byte entry per surviving cluster in the commands'
    /// place, and the arguments of the one indirect draw over the list.
    pub fn mip_list_clusters(ctx: *mut MipContext, frame: *const MipFrame, visible_bitmap: *const u32, policy: *const MipLodPolicy,
                             occ: *const MipOcclusion, cone: *const MipClusterCone, out: *const MipClusterListOutputs) -> i32;
    /// mip_cull_clusters_views with mip_list_clusters' entries in the commands' place: one list and one indirect draw per view,
    /// the located work item and three of the four entry fields shared by all views; on the first stream.
    pub fn mip_list_clusters_views(ctx: *mut MipContext, frames: *const MipFrame, visible_bitmaps: *const *const u32,
                                   n_views: u32, policy: *const MipLodPolicy, out: *const MipClusterViewListOutputs) -> i32;
    /// mip_list_clusters_views with a depth pyramid per view: `occs` is a host array of n_views host pointers, null for a view
    /// that is tested against its planes alone; on the first stream, behind pyramids built for the next run.
    pub fn mip_list_clusters_views_occluded(ctx: *mut MipContext, frames: *const MipFrame, visible_bitmaps: *const *const u32,
                                            occs: *const *const MipOcclusion, n_views: u32, policy: *const MipLodPolicy,
                                            out: *const MipClusterViewOccludedListOutputs) -> i32;
    /// mip_cull_clusters_phase with mip_list_clusters' entries in the commands' place: FIRST lists the survivors and writes the
    /// record, SECOND lists the recorded clusters visible under the new pyramid, from entry *out.entry_base on.
    pub fn mip_list_clusters_phase(ctx: *mut MipContext, frame: *const MipFrame, visible_bitmap: *const u32, policy: *const MipLodPolicy,
                                   occ: *const MipOcclusion, out: *const MipClusterPhaseListOutputs, rec: *const MipClusterRecord) -> i32;
    /// mip_list_clusters with the per-triangle test behind the cluster cull: an entry per surviving cluster that keeps a
    /// triangle, its triangle mask beside it; no index stream, no commands, no entry for an empty cluster.
    pub fn mip_list_cluster_triangles(ctx: *mut MipContext, frame: *const MipFrame, visible_bitmap: *const u32, policy: *const MipLodPolicy,
                                      occ: *const MipOcclusion, cone: *const MipClusterCone, out: *const MipClusterTriangleListOutputs) -> i32;
    pub fn mip_last_error(ctx: *const MipContext) -> *const c_char;
    pub fn mip_instance_count(ctx: *const MipContext) -> u32;
}

// Layout guards in the style of src/renderer.rs:178-185 (the C side is checked by tests/test_abi.py)
const _: () = assert!(std::mem::size_of::<MipConfig>() == 32);
const _: () = assert!(std::mem::size_of::<MipMesh>() == 80);
const _: () = assert!(std::mem::size_of::<MipFrame>() == 180);
const _: () = assert!(std::mem::size_of::<MipOutputs>() == 80);
const _: () = assert!(std::mem::size_of::<MipDrawIndexedIndirectCommand>() == 20);
// the extension structs, as array lengths (a mismatch is a type error)
const _: [u8; 48] = [0; std::mem::size_of::<MipBatchOutputs>()];
const _: [u8; 28] = [0; std::mem::size_of::<MipLodPolicy>()];
const _: [u8; 28] = [0; std::mem::size_of::<MipSortPolicy>()];
const _: [u8; 48] = [0; std::mem::size_of::<MipViewBatchOutputs>()];
const _: [u8; 16] = [0; std::mem::size_of::<MipBatchChunkHeader>()];
const _: [u8; 40] = [0; std::mem::size_of::<MipClusterOutputs>()];
const _: [u8; 40] = [0; std::mem::size_of::<MipClusterViewOutputs>()];
const _: [u8; 24] = [0; std::mem::size_of::<MipClusterRecord>()];
const _: [u8; 56] = [0; std::mem::size_of::<MipClusterTriangleOutputs>()];
const _: [u8; 24] = [0; std::mem::size_of::<MipClusterCone>()];
const _: [u8; 16] = [0; std::mem::size_of::<MipClusterEntry>()];
const _: [u8; 48] = [0; std::mem::size_of::<MipClusterListOutputs>()];
const _: [u8; 48] = [0; std::mem::size_of::<MipClusterViewListOutputs>()];
const _: [u8; 56] = [0; std::mem::size_of::<MipClusterPhaseListOutputs>()];
const _: [u8; 56] = [0; std::mem::size_of::<MipClusterViewOccludedListOutputs>()];
const _: [u8; 56] = [0; std::mem::size_of::<MipClusterTriangleListOutputs>()];
const _: [u8; 104] = [0; std::mem::size_of::<MipOcclusion>()];

impl Pipeline {
    /// `panic = "abort"` (Cargo.toml:133,138) makes a panic here as final as in the rest of the renderer.
    pub fn new(max_instances: u32, max_meshes: u32, frames_in_flight: u32) -> Pipeline {
        let cfg = MipConfig { struct_size: std::mem::size_of::<MipConfig>() as u32, device_ordinal: 0, max_instances,
                              max_meshes, flags: 0, frames_in_flight, stream: std::ptr::null_mut() };
        let mut ctx = std::ptr::null_mut();
        let rc = unsafe { mip_create(&cfg, &mut ctx) };
        assert_eq!(rc, MIP_OK, "mip_create failed: {}", rc);
        Pipeline(ctx)
    }
}

impl Drop for Pipeline {
    fn drop(&mut self) {
        unsafe { mip_destroy(self.0) }
    }
}
