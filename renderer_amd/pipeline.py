"""ctypes host wrapper over the C ABI. Mirrors the order the reference's schedule runs the
path in (src/main.rs:780-839 RenderSetup, then cull_pass): upload the ECS columns once,
then one `run` per frame."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (MipBatchOutputs, MipClusterCone, MipClusterListOutputs, MipClusterOutputs, MipClusterPhaseListOutputs, MipClusterRecord, MipClusterTriangleListOutputs, MipClusterTriangleOutputs, MipClusterViewListOutputs, MipClusterViewOccludedListOutputs, MipClusterViewOutputs, MipConfig, MipError, MipFrame, MipLodPolicy, MipOcclusion, MipOutputs, MipShardedOutputs, MipSortPolicy,
                   MipTimings, MipViewBatchOutputs)

MESH_DTYPE = np.dtype(
    [
        ("aabb_min", "<f4", (3,)),
        ("aabb_max", "<f4", (3,)),
        ("n_lods", "<u4"),
        ("index_len", "<u4", (_lib.MIP_MAX_LODS,)),
        ("index_offset", "<u4", (_lib.MIP_MAX_LODS,)),
        ("vertex_offset", "<i4"),
    ]
)
DRAW_CMD_DTYPE = np.dtype(
    [
        ("indexCount", "<u4"),
        ("instanceCount", "<u4"),
        ("firstIndex", "<u4"),
        ("vertexOffset", "<i4"),
        ("firstInstance", "<u4"),
    ]
)
CLUSTER_ENTRY_DTYPE = np.dtype(  # MipClusterEntry: one entry of list_clusters' list
    [
        ("instance", "<u4"),
        ("first_index", "<u4"),
        ("vertex_offset", "<i4"),
        ("index_count", "<u4"),
    ]
)
SHARD_HEADER_BYTES = 32


def wire_form(wire):
    """0 = 20-byte commands, 1 = 8-byte wire records (MIP_OUT_WIRE), 2 = packed 4-byte records (MIP_OUT_WIRE_PACKED).
    Accepts False / True / 1 / 2 / "packed"."""
    if wire in (2, "packed"):
        return 2
    return 1 if wire else 0


def wire_index_bits(n_meshes):
    """mip_wire_index_bits: what a table of n_meshes entries leaves of a packed record for the instance index."""
    mesh_bits = 0
    while mesh_bits < 31 and (1 << mesh_bits) < int(n_meshes):
        mesh_bits += 1
    return 31 - mesh_bits


def wire_body_bytes(capacity, packed=False):
    """MIP_WIRE_BODY_BYTES / MIP_WIRE_PACKED_BODY_BYTES: whole blocks of 256 8-byte records, or of 64 packed 4-byte records,
    each behind a 16-byte block header."""
    per = _lib.MIP_WIRE_PACKED_BLOCK_COMMANDS if packed else _lib.MIP_WIRE_BLOCK_COMMANDS
    blocks = (int(capacity) + per - 1) // per
    return blocks * (_lib.MIP_WIRE_PACKED_BLOCK_BYTES if packed else _lib.MIP_WIRE_BLOCK_BYTES)


def depth_pyramid_layout(width, height):
    """mip_depth_pyramid_bytes as a pure mirror (the occlusion-culling extension): the pyramid of a W x H depth image is f32,
    row-major, level 0 = ceil(W/2) x ceil(H/2), each next level ceil of half the last, down to 1 x 1, stored level 0 first.
    Returns {"sizes": [(w, h), ...], "offsets": [float offset of each level], "bytes": total}; bytes = 0 (no levels) when a
    side is 0 or above MIP_MAX_DEPTH_EXTENT."""
    width, height = int(width), int(height)
    if not (1 <= width <= _lib.MIP_MAX_DEPTH_EXTENT and 1 <= height <= _lib.MIP_MAX_DEPTH_EXTENT):
        return {"sizes": [], "offsets": [], "bytes": 0}
    sizes, offsets, floats = [], [], 0
    k = 0
    while True:
        w, h = ((width - 1) >> (k + 1)) + 1, ((height - 1) >> (k + 1)) + 1
        sizes.append((w, h))
        offsets.append(floats)
        floats += w * h
        if w == 1 and h == 1:
            break
        k += 1
    return {"sizes": sizes, "offsets": offsets, "bytes": floats * 4}


def make_occlusion(width, height, pyramid_ptr, pv, candidates=0, occluded_bitmap=0, inverted=False):
    """A MipOcclusion: the pyramid (device pointer) of a width x height depth image rendered with `pv` (column-major 16 floats);
    optional device bitmaps of candidates and of the occluded instances."""
    o = MipOcclusion()
    o.struct_size = C.sizeof(MipOcclusion)
    o.width, o.height = int(width), int(height)
    o.flags = _lib.MIP_OCC_CANDIDATES_INVERTED if inverted else 0
    o.pyramid = pyramid_ptr or None
    o.candidates = candidates or None
    o.occluded_bitmap = occluded_bitmap or None
    o.pv[:] = np.ascontiguousarray(pv, dtype=np.float32).reshape(16).tolist()
    return o


# mip_batch_draws_lods with this policy is mip_batch_draws, byte for byte: pick_lod's `distance > 10` as a squared threshold
# (nextafter(100) in float32), levels 2.. never
LOD_PIN_SWITCH_SQ = (100.00000762939453125, float("inf"), float("inf"), float("inf"), float("inf"))


def make_lod_policy(mode, switch_sq):
    """A MipLodPolicy: mode MIP_LOD_DISTANCE / MIP_LOD_RELATIVE (or "distance" / "relative") and the five SQUARED thresholds
    (fewer are padded with +inf: those levels are never selected). The values are rounded to float32 here; the library checks them
    (>= 0, not NaN, non-decreasing)."""
    if isinstance(mode, str):
        mode = {"distance": _lib.MIP_LOD_DISTANCE, "relative": _lib.MIP_LOD_RELATIVE}[mode]
    sw = [float(v) for v in np.asarray(switch_sq, dtype=np.float32).reshape(-1)]
    if len(sw) > _lib.MIP_MAX_LODS - 1:
        raise ValueError(f"{len(sw)} thresholds for {_lib.MIP_MAX_LODS} LODs")
    sw += [float("inf")] * (_lib.MIP_MAX_LODS - 1 - len(sw))
    p = MipLodPolicy()
    p.struct_size = C.sizeof(MipLodPolicy)
    p.mode = int(mode)
    p.switch_sq[:] = sw
    return p


def make_sort_policy(metric, order, depth_bits=16, axis=(0.0, 0.0, 0.0)):
    """A MipSortPolicy for batch_draws_sorted: metric MIP_DEPTH_RADIAL / MIP_DEPTH_VIEW_AXIS (or "radial" / "view_axis"), order
    MIP_BATCH_ORDER_NEAR_FIRST / FAR_FIRST (or "near_first" / "far_first"), depth_bits 16, 24 or 32 (the leading bits of the
    depth that are sorted) and, for VIEW_AXIS, the view direction (need not be unit). The library checks the values."""
    if isinstance(metric, str):
        metric = {"radial": _lib.MIP_DEPTH_RADIAL, "view_axis": _lib.MIP_DEPTH_VIEW_AXIS}[metric]
    if isinstance(order, str):
        order = {"near_first": _lib.MIP_BATCH_ORDER_NEAR_FIRST, "far_first": _lib.MIP_BATCH_ORDER_FAR_FIRST}[order]
    p = MipSortPolicy()
    p.struct_size = C.sizeof(MipSortPolicy)
    p.metric = int(metric)
    p.order = int(order)
    p.depth_bits = int(depth_bits)
    p.axis[:] = [float(v) for v in np.asarray(axis, dtype=np.float32).reshape(3)]
    return p


def batch_chunk_ids_offset(n_buckets):
    """MIP_BATCH_CHUNK_IDS_OFFSET: bytes in front of a batch chunk's ids (the 16-byte header, B counts, the pad to 16 bytes)."""
    n_buckets = int(n_buckets)
    return 16 + (n_buckets + (4 - n_buckets % 4) % 4) * 4


def batch_chunk_bytes(n_buckets, capacity):
    """MIP_BATCH_CHUNK_BYTES: bytes of a batch chunk with room for `capacity` ids."""
    return batch_chunk_ids_offset(n_buckets) + int(capacity) * 4


def make_cluster_outputs(cluster_cmds, cmd_capacity, cmd_count, stats=0, work_capacity=0, async_=False):
    """A MipClusterOutputs for cull_clusters: device pointers to room for cmd_capacity commands, to the count and (optional) to
    the four stats words {heads, surviving clusters, W, members}; work_capacity bounds the (instance, cluster) work items of the
    call (0 = N x the largest cluster count of a level, which is also what the call's scratch is sized by)."""
    o = MipClusterOutputs()
    o.struct_size = C.sizeof(MipClusterOutputs)
    o.flags = _lib.MIP_OUT_DEVICE | (_lib.MIP_OUT_ASYNC if async_ else 0)
    o.cluster_cmds = cluster_cmds or None
    o.cmd_capacity = int(cmd_capacity)
    o.work_capacity = int(work_capacity)
    o.cmd_count = cmd_count or None
    o.stats = stats or None
    return o


def make_cluster_list_outputs(cluster_entries, entry_capacity, entry_count, draw_args=0, stats=0, work_capacity=0, async_=False):
    """A MipClusterListOutputs for list_clusters: device pointers to room for entry_capacity 16-byte entries (CLUSTER_ENTRY_DTYPE,
    16-byte aligned), to the count, (optional) to the four words of the one VkDrawIndirectCommand {192, entry_count, 0, 0} and
    (optional) to the three stats words {survivors, W, members}; work_capacity as in make_cluster_outputs."""
    o = MipClusterListOutputs()
    o.struct_size = C.sizeof(MipClusterListOutputs)
    o.flags = _lib.MIP_OUT_DEVICE | (_lib.MIP_OUT_ASYNC if async_ else 0)
    o.cluster_entries = cluster_entries or None
    o.entry_capacity = int(entry_capacity)
    o.work_capacity = int(work_capacity)
    o.entry_count = entry_count or None
    o.draw_args = draw_args or None
    o.stats = stats or None
    return o


def make_cluster_triangle_list_outputs(cluster_entries, triangle_masks, entry_capacity, entry_count, draw_args=0, stats=0, work_capacity=0, async_=False):
    """A MipClusterTriangleListOutputs for list_cluster_triangles: make_cluster_list_outputs' fields, a device pointer to room for
    entry_capacity 64-bit triangle masks (8-byte aligned; mask k goes with entry k) and SIX stats words {entries, surviving
    clusters, W, members, surviving triangles, triangles tested}."""
    o = MipClusterTriangleListOutputs()
    o.struct_size = C.sizeof(MipClusterTriangleListOutputs)
    o.flags = _lib.MIP_OUT_DEVICE | (_lib.MIP_OUT_ASYNC if async_ else 0)
    o.cluster_entries = cluster_entries or None
    o.triangle_masks = triangle_masks or None
    o.entry_capacity = int(entry_capacity)
    o.work_capacity = int(work_capacity)
    o.entry_count = entry_count or None
    o.draw_args = draw_args or None
    o.stats = stats or None
    return o


def make_cluster_phase_list_outputs(cluster_entries, entry_capacity, entry_count, draw_args=0, stats=0, work_capacity=0, async_=False, entry_base=0):
    """A MipClusterPhaseListOutputs for list_clusters_phase: make_cluster_list_outputs' fields — entry_capacity counts the
    BUFFER's entries from entry 0, draw_args becomes {192, entry_count, 0, b}, stats has FOUR words {survivors, W, members,
    candidates} — and entry_base, a device pointer to the word b the list starts at (0 / None: b = 0); it may be the FIRST
    call's entry_count, so that SECOND appends behind FIRST's entries without the host reading the count."""
    o = MipClusterPhaseListOutputs()
    o.struct_size = C.sizeof(MipClusterPhaseListOutputs)
    o.flags = _lib.MIP_OUT_DEVICE | (_lib.MIP_OUT_ASYNC if async_ else 0)
    o.cluster_entries = cluster_entries or None
    o.entry_capacity = int(entry_capacity)
    o.work_capacity = int(work_capacity)
    o.entry_count = entry_count or None
    o.draw_args = draw_args or None
    o.stats = stats or None
    o.entry_base = entry_base or None
    return o


def make_cluster_view_outputs(cluster_cmds, cmd_stride, cmd_counts, stats=0, work_capacity=0, async_=False):
    """A MipClusterViewOutputs for cull_clusters_views: device pointers to room for n_views x cmd_stride commands (view v's
    start at entry v x cmd_stride), to the n_views counts and (optional) to the 2 + 2 x n_views stats words {W, members, then
    heads and surviving clusters per view}; work_capacity bounds the work items of the union of the views' members (0 = N x
    the largest cluster count of a level, which is also what the call's scratch is sized by)."""
    o = MipClusterViewOutputs()
    o.struct_size = C.sizeof(MipClusterViewOutputs)
    o.flags = _lib.MIP_OUT_DEVICE | (_lib.MIP_OUT_ASYNC if async_ else 0)
    o.cluster_cmds = cluster_cmds or None
    o.cmd_stride = int(cmd_stride)
    o.work_capacity = int(work_capacity)
    o.cmd_counts = cmd_counts or None
    o.stats = stats or None
    return o


def make_cluster_view_list_outputs(cluster_entries, entry_stride, entry_counts, draw_args=0, stats=0, work_capacity=0, async_=False):
    """A MipClusterViewListOutputs for list_clusters_views: device pointers to room for n_views x entry_stride 16-byte entries
    (CLUSTER_ENTRY_DTYPE, 16-byte aligned; view v's start at entry v x entry_stride), to the n_views counts, (optional) to the
    n_views x 4 words of one VkDrawIndirectCommand {192, entry_counts[v], 0, v x entry_stride} per view and (optional) to the
    2 + n_views stats words {W, members, then the surviving clusters per view}; work_capacity as in make_cluster_view_outputs."""
    o = MipClusterViewListOutputs()
    o.struct_size = C.sizeof(MipClusterViewListOutputs)
    o.flags = _lib.MIP_OUT_DEVICE | (_lib.MIP_OUT_ASYNC if async_ else 0)
    o.cluster_entries = cluster_entries or None
    o.entry_stride = int(entry_stride)
    o.work_capacity = int(work_capacity)
    o.entry_counts = entry_counts or None
    o.draw_args = draw_args or None
    o.stats = stats or None
    return o


def make_cluster_view_occluded_list_outputs(cluster_entries, entry_stride, entry_counts, draw_args=0, stats=0, hidden=0, work_capacity=0, async_=False):
    """A MipClusterViewOccludedListOutputs for list_clusters_views_occluded: make_cluster_view_list_outputs' fields and
    (optional) a device pointer to the n_views words of `hidden`: per view the work items that passed the view's planes and are
    occluded under the view's pyramid."""
    o = MipClusterViewOccludedListOutputs()
    o.struct_size = C.sizeof(MipClusterViewOccludedListOutputs)
    o.flags = _lib.MIP_OUT_DEVICE | (_lib.MIP_OUT_ASYNC if async_ else 0)
    o.cluster_entries = cluster_entries or None
    o.entry_stride = int(entry_stride)
    o.work_capacity = int(work_capacity)
    o.entry_counts = entry_counts or None
    o.draw_args = draw_args or None
    o.stats = stats or None
    o.hidden = hidden or None
    return o


def make_cluster_triangle_outputs(cluster_cmds, cmd_capacity, cmd_count, culled_indices, index_capacity, stats=0, work_capacity=0, async_=False):
    """A MipClusterTriangleOutputs for cull_cluster_triangles: make_cluster_outputs' fields, a device pointer to room for
    index_capacity 32-bit indices of the culled stream, and (optional) SIX stats words {heads, surviving clusters, W, members,
    surviving triangles, triangles tested}."""
    o = MipClusterTriangleOutputs()
    o.struct_size = C.sizeof(MipClusterTriangleOutputs)
    o.flags = _lib.MIP_OUT_DEVICE | (_lib.MIP_OUT_ASYNC if async_ else 0)
    o.cluster_cmds = cluster_cmds or None
    o.cmd_capacity = int(cmd_capacity)
    o.work_capacity = int(work_capacity)
    o.cmd_count = cmd_count or None
    o.stats = stats or None
    o.culled_indices = culled_indices or None
    o.index_capacity = int(index_capacity)
    return o


def cluster_record_bytes(work_items):
    """mip_cluster_record_bytes: bytes of a two-phase record for `work_items` (instance, cluster) items: a 16-byte header and
    one 64-bit word per 64 items."""
    return 16 + 8 * ((int(work_items) + 63) // 64)


def make_cluster_record(phase, record, record_bytes):
    """A MipClusterRecord for cull_clusters_phase: phase MIP_CLUSTER_PHASE_FIRST / _SECOND (or "first" / "second"), a device
    pointer to the caller's 16-byte aligned record and the room behind it (cluster_record_bytes of the call's bound on W)."""
    if isinstance(phase, str):
        phase = {"first": _lib.MIP_CLUSTER_PHASE_FIRST, "second": _lib.MIP_CLUSTER_PHASE_SECOND}[phase]
    r = MipClusterRecord()
    r.struct_size = C.sizeof(MipClusterRecord)
    r.phase = int(phase)
    r.record = record or None
    r.record_bytes = int(record_bytes)
    return r


def make_cluster_cone(pv=None, eye=None, facing=None):
    """A MipClusterCone for cull_clusters_cone / cull_cluster_triangles_cone: from a projection `pv` (float32[16], column-major)
    through mip_cone_from_pv — the point the view projects from and the sign of its determinant, in double, rounded once; a
    singular (orthographic) or non-finite pv raises MIP_ERR_INVALID_ARGUMENT — or from an explicit `eye` (3 floats; a shadow
    view's is the light) and `facing` (+1 or -1), which also override what pv gives."""
    c = MipClusterCone()
    c.struct_size = C.sizeof(MipClusterCone)
    if pv is not None:
        m = np.ascontiguousarray(np.asarray(pv, np.float32).reshape(16))
        rc = _lib.load_library().mip_cone_from_pv(m.ctypes.data, C.addressof(c))
        if rc != 0:
            raise MipError(rc, "mip_cone_from_pv: rows x, y, w of pv are singular or not finite (an orthographic view has no eye)")
    elif eye is None or facing is None:
        raise ValueError("make_cluster_cone needs pv, or eye and facing")
    if eye is not None:
        c.eye[:] = [float(v) for v in np.asarray(eye, np.float32).reshape(3)]
    if facing is not None:
        c.facing = float(facing)
    return c


def make_frame(planes, cam_pos, first_instance_base=0, first_index_base=0, pv=None):
    f = MipFrame()
    if pv is not None:
        f.pv[:] = np.ascontiguousarray(pv, dtype=np.float32).reshape(16).tolist()
    planes = np.ascontiguousarray(planes, dtype=np.float32).reshape(24)
    cam_pos = np.ascontiguousarray(cam_pos, dtype=np.float32).reshape(3)
    f.planes[:] = planes.tolist()
    f.cam_pos[:] = cam_pos.tolist()
    f.first_instance_base = int(first_instance_base) & 0xFFFFFFFF
    f.first_index_base = int(first_index_base) & 0xFFFFFFFF
    return f


class InstancePipeline:
    """One context on one GPU (one per rank)."""

    def __init__(self, max_instances, max_meshes, device=0, timing=False, stream=None, frames_in_flight=1,
                 ordered_tiles=False):
        self._lib = _lib.load_library()
        self._ctx = C.c_void_p()
        cfg = MipConfig()
        cfg.struct_size = C.sizeof(MipConfig)
        cfg.device_ordinal = int(device)
        cfg.max_instances = int(max_instances)
        cfg.max_meshes = int(max_meshes)
        cfg.flags = (_lib.MIP_CFG_TIMING if timing else 0) | (_lib.MIP_CFG_ORDERED_TILES if ordered_tiles else 0)
        cfg.frames_in_flight = int(frames_in_flight)
        cfg.stream = stream
        rc = self._lib.mip_create(C.byref(cfg), C.byref(self._ctx))
        if rc != 0:
            self._ctx = C.c_void_p()
            raise MipError(rc, "mip_create failed (is there a gfx950 GPU?)")
        self.max_instances = int(max_instances)
        self.n = 0
        self.stream = stream  # the caller's HIP stream handle, or None when the context created its own

    # -- lifetime --
    def close(self):
        if getattr(self, "_ctx", None) and self._ctx.value:
            self._lib.mip_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc):
        if rc != 0:
            msg = self._lib.mip_last_error(self._ctx)
            raise MipError(rc, msg.decode() if msg else "")

    # -- uploads --
    def set_mesh_table(self, meshes):
        meshes = np.ascontiguousarray(meshes, dtype=MESH_DTYPE).reshape(-1)
        self._check(self._lib.mip_set_mesh_table(self._ctx, meshes.ctypes.data, len(meshes)))
        self.n_meshes = len(meshes)

    def set_instances(self, pos_xyz, rot_ijkw, scale, mesh_id):
        pos = np.ascontiguousarray(pos_xyz, dtype=np.float32).reshape(-1, 3)
        rot = np.ascontiguousarray(rot_ijkw, dtype=np.float32).reshape(-1, 4)
        scl = np.ascontiguousarray(scale, dtype=np.float32).reshape(-1)
        mid = np.ascontiguousarray(mesh_id, dtype=np.uint32).reshape(-1)
        n = pos.shape[0]
        if not (rot.shape[0] == n and scl.shape[0] == n and mid.shape[0] == n):
            raise ValueError("instance columns differ in length")
        self._check(self._lib.mip_set_instances(self._ctx, pos.ctypes.data, rot.ctypes.data,
                                                scl.ctypes.data, mid.ctypes.data, n))
        self.n = n

    def set_geometry(self, vertex_xyz, indices):
        """Consolidated position / index buffers for the per-triangle stage."""
        v = np.ascontiguousarray(vertex_xyz, dtype=np.float32).reshape(-1, 3)
        i = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        self._check(self._lib.mip_set_geometry(self._ctx, v.ctypes.data, len(v), i.ctypes.data, len(i)))

    def update_instances(self, first, pos_xyz=None, rot_ijkw=None, scale=None, mesh_id=None):
        """Overwrite a range of the resident columns (None = keep)."""
        cols, count = [], None
        for arr, dtype, width in ((pos_xyz, np.float32, 3), (rot_ijkw, np.float32, 4), (scale, np.float32, 1), (mesh_id, np.uint32, 1)):
            if arr is None:
                cols.append(None)
                continue
            a = np.ascontiguousarray(arr, dtype=dtype).reshape(-1, width)
            if count is not None and len(a) != count:
                raise ValueError("columns differ in length")
            count = len(a)
            cols.append(a)
        ptrs = [c.ctypes.data if c is not None else None for c in cols]
        self._check(self._lib.mip_update_instances(self._ctx, int(first), int(count or 0), *ptrs))

    def set_blas_addresses(self, addresses):
        a = np.ascontiguousarray(addresses, dtype=np.uint64).reshape(-1)
        self._check(self._lib.mip_set_blas_addresses(self._ctx, a.ctypes.data, len(a)))

    def set_instances_device(self, pos_ptr, rot_ptr, scale_ptr, mesh_id_ptr, n):
        self._check(self._lib.mip_set_instances_device(self._ctx, pos_ptr, rot_ptr, scale_ptr,
                                                       mesh_id_ptr, int(n)))
        self.n = int(n)

    # -- per frame --
    def run_host(self, planes, cam_pos, first_instance_base=0, first_index_base=0,
                 want=("model", "visible_bitmap", "draw_cmds", "world_aabb")):
        """Synchronous; results copied back into fresh numpy arrays (PCIe-inclusive)."""
        n = self.n
        frame = make_frame(planes, cam_pos, first_instance_base, first_index_base)
        out = MipOutputs()
        out.flags = _lib.MIP_OUT_HOST
        res = {}
        if "model" in want:
            res["model"] = np.zeros((n, 16), np.float32)
            out.model = res["model"].ctypes.data
        if "visible_bitmap" in want:
            res["visible_bitmap"] = np.zeros((n + 31) // 32, np.uint32)
            out.visible_bitmap = res["visible_bitmap"].ctypes.data
        if "world_aabb" in want:
            res["world_aabb"] = np.zeros((n, 6), np.float32)
            out.world_aabb = res["world_aabb"].ctypes.data
        count = C.c_uint32(0)
        total = C.c_uint32(0)
        cmds = None
        if "draw_cmds" in want:
            cmds = np.zeros(max(n, 1), DRAW_CMD_DTYPE)
            out.draw_cmds = cmds.ctypes.data
            out.draw_count = C.addressof(count)
            out.draw_index_total = C.addressof(total)
        self._check(self._lib.mip_run(self._ctx, C.byref(frame), C.byref(out)))
        if cmds is not None:
            res["draw_cmds"] = cmds[: count.value].copy()
            res["draw_count"] = int(count.value)
            res["draw_index_total"] = int(total.value)
        return res

    def run_device(self, frame, model=0, visible_bitmap=0, draw_cmds=0, draw_count=0,
                   draw_index_total=0, world_aabb=0, async_=False, culled_index_buffer=0, culled_index_capacity=0,
                   tlas_instances=0, wire=False):
        """Device pointers in, nothing copied. `frame` from make_frame(). wire=True: draw_cmds receives the
        wire form of the list (MIP_OUT_WIRE); wire="packed" (or 2): its packed form (MIP_OUT_WIRE_PACKED)."""
        out = MipOutputs()
        form = wire_form(wire)
        out.flags = (_lib.MIP_OUT_DEVICE | (_lib.MIP_OUT_ASYNC if async_ else 0) | (_lib.MIP_OUT_WIRE if form else 0)
                     | (_lib.MIP_OUT_WIRE_PACKED if form == 2 else 0))
        out.model = model or None
        out.visible_bitmap = visible_bitmap or None
        out.draw_cmds = draw_cmds or None
        out.draw_count = draw_count or None
        out.draw_index_total = draw_index_total or None
        out.world_aabb = world_aabb or None
        out.culled_index_buffer = culled_index_buffer or None
        out.culled_index_capacity = int(culled_index_capacity)
        out.tlas_instances = tlas_instances or None
        self._check(self._lib.mip_run(self._ctx, C.byref(frame), C.byref(out)))

    def prepare_outputs(self, model=0, visible_bitmap=0, draw_cmds=0, draw_count=0, draw_index_total=0,
                        world_aabb=0, async_=True, culled_index_buffer=0, culled_index_capacity=0, tlas_instances=0, wire=False):
        """A reusable MipOutputs (device pointers) for run_prepared: keeps the per-frame host cost
        to one foreign call. tlas_instances and wire as run_device takes them."""
        out = MipOutputs()
        form = wire_form(wire)
        out.flags = (_lib.MIP_OUT_DEVICE | (_lib.MIP_OUT_ASYNC if async_ else 0) | (_lib.MIP_OUT_WIRE if form else 0)
                     | (_lib.MIP_OUT_WIRE_PACKED if form == 2 else 0))
        out.model = model or None
        out.visible_bitmap = visible_bitmap or None
        out.draw_cmds = draw_cmds or None
        out.draw_count = draw_count or None
        out.draw_index_total = draw_index_total or None
        out.world_aabb = world_aabb or None
        out.culled_index_buffer = culled_index_buffer or None
        out.culled_index_capacity = int(culled_index_capacity)
        out.tlas_instances = tlas_instances or None
        out._as_parameter_ = C.c_void_p(C.addressof(out))  # lets ctypes pass the struct by address
        return out

    @staticmethod
    def frame_ref(frame):
        """A MipFrame prepared for run_prepared (passed by address)."""
        frame._as_parameter_ = C.c_void_p(C.addressof(frame))
        return frame

    def run_prepared(self, frame, outputs):
        rc = self._lib.mip_run(self._ctx, frame, outputs)
        if rc != 0:
            self._check(rc)

    def run_many(self, frames, prepared_outputs, steps):
        """`steps` frames issued from compiled code: step k runs frames[k % len(frames)] into
        prepared_outputs[k % len(prepared_outputs)]. `frames` is one MipFrame or a sequence of them (a moving
        camera); recorded launch graphs are reused whatever the frames are."""
        if isinstance(frames, MipFrame):
            frames = [frames]
        fr = (MipFrame * len(frames))()
        for k, f in enumerate(frames):
            C.memmove(C.addressof(fr[k]), C.addressof(f), C.sizeof(MipFrame))
        arr = (MipOutputs * len(prepared_outputs))()
        for k, o in enumerate(prepared_outputs):
            C.memmove(C.addressof(arr[k]), C.addressof(o), C.sizeof(MipOutputs))
        rc = self._lib.mip_run_many(self._ctx, C.addressof(fr), len(frames), C.addressof(arr), len(prepared_outputs), int(steps))
        if rc != 0:
            self._check(rc)

    # -- zero-copy interop (row f-2) --
    def import_external_fd(self, fd, size_bytes):
        """Maps memory another API exported as an fd (VK_KHR_external_memory_fd / a dma-buf) into this
        context's device; returns the device pointer. The fd belongs to the driver afterwards."""
        ptr = C.c_void_p()
        self._check(self._lib.mip_import_external_fd(self._ctx, int(fd), int(size_bytes), C.byref(ptr)))
        return ptr.value

    def release_external(self, ptr):
        self._check(self._lib.mip_release_external(self._ctx, ptr))

    def import_external_semaphore_fd(self, fd, timeline=True):
        """Imports a semaphore another API exported as an fd (vkGetSemaphoreFdKHR); returns the opaque handle."""
        h = C.c_void_p()
        kind = _lib.MIP_SEMAPHORE_TIMELINE if timeline is True else (_lib.MIP_SEMAPHORE_BINARY if timeline is False else int(timeline))
        self._check(self._lib.mip_import_external_semaphore_fd(self._ctx, int(fd), kind, C.byref(h)))
        return h.value

    def external_semaphore_on_device(self, semaphore):
        """True: the HIP runtime imported the semaphore (device-side waits/signals); False: the DRM sync object path."""
        rc = self._lib.mip_external_semaphore_on_device(self._ctx, semaphore)
        if rc < 0:
            self._check(rc)
        return bool(rc)

    def wait_external(self, semaphore, value=0):
        """The next frame's stream waits on the device until the semaphore reaches `value`."""
        self._check(self._lib.mip_wait_external(self._ctx, semaphore, int(value)))

    def signal_external(self, semaphore, value=0):
        """Signals the semaphore to `value` behind the frame issued last."""
        self._check(self._lib.mip_signal_external(self._ctx, semaphore, int(value)))

    def release_external_semaphore(self, semaphore):
        self._check(self._lib.mip_release_external_semaphore(self._ctx, semaphore))

    # -- native sharded exchange (RCCL opened by the library itself) --
    @staticmethod
    def comm_unique_id():
        """128 opaque bytes from ncclGetUniqueId; create on one rank, share with the others."""
        buf = (C.c_uint8 * 128)()
        rc = _lib.load_library().mip_comm_unique_id(buf)
        if rc != 0:
            raise MipError(rc, "mip_comm_unique_id failed (is librccl.so.1 loadable?)")
        return bytes(buf)

    def comm_init(self, unique_id, rank, world):
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        self._check(self._lib.mip_comm_init(self._ctx, buf, int(rank), int(world)))

    def comm_destroy(self):
        self._check(self._lib.mip_comm_destroy(self._ctx))

    def run_sharded(self, frame, draw_cmds, draw_count, model=0, visible_bitmap=0, world_aabb=0, chunk_capacity=0,
                    async_=False):
        """Shard kernel -> one ncclAllGather -> merge, all inside the library."""
        out = MipShardedOutputs()
        out.model = model or None
        out.visible_bitmap = visible_bitmap or None
        out.world_aabb = world_aabb or None
        out.draw_cmds = draw_cmds
        out.draw_count = draw_count
        out.chunk_capacity = int(chunk_capacity)
        out.flags = _lib.MIP_OUT_DEVICE | (_lib.MIP_OUT_ASYNC if async_ else 0)
        self._check(self._lib.mip_run_sharded(self._ctx, C.addressof(frame), C.addressof(out)))

    def wait(self):
        self._check(self._lib.mip_wait(self._ctx))

    def merge_draw_lists(self, chunks_ptr, n_chunks, chunk_stride_bytes, out_cmds_ptr, out_count_ptr,
                         async_=False, chunk_capacity=0):
        """chunk_capacity = commands one chunk may carry (out_cmds has room for n_chunks x that); 0 = what
        the stride holds. A chunk whose header count exceeds it is cut and reported (MIP_ERR_CAPACITY)."""
        self._check(self._lib.mip_merge_draw_lists(self._ctx, chunks_ptr, int(n_chunks),
                                                   int(chunk_stride_bytes), int(chunk_capacity), out_cmds_ptr,
                                                   out_count_ptr, 1 if async_ else 0))

    def merge_wire_lists(self, chunks_ptr, n_chunks, chunk_stride_bytes, out_cmds_ptr, out_count_ptr,
                         async_=False, chunk_capacity=0, packed=False):
        """The same merge over chunks in the wire form (MIP_OUT_WIRE; packed=True: MIP_OUT_WIRE_PACKED), expanded against
        this context's mesh table."""
        fn = self._lib.mip_merge_wire_lists_packed if packed else self._lib.mip_merge_wire_lists
        self._check(fn(self._ctx, chunks_ptr, int(n_chunks), int(chunk_stride_bytes), int(chunk_capacity), out_cmds_ptr,
                       out_count_ptr, 1 if async_ else 0))

    # -- extension: skinned instances (BASELINE config 5; not a reference behaviour) --
    def set_skeleton(self, parent, inverse_bind, joint_box):
        parent = np.ascontiguousarray(parent, dtype=np.int32)
        j = len(parent)
        ibm = np.ascontiguousarray(inverse_bind, dtype=np.float32).reshape(j, 16)
        box = np.ascontiguousarray(joint_box, dtype=np.float32).reshape(j, 6)
        self._check(self._lib.mip_set_skeleton(self._ctx, parent.ctypes.data, ibm.ctypes.data, box.ctypes.data, j))
        self._n_joints = j

    def set_poses(self, joint_trs):
        """Host array n x J x 10 (t xyz, q ijkw, s xyz per joint); copied."""
        poses = np.ascontiguousarray(joint_trs, dtype=np.float32)
        n = poses.size // (max(getattr(self, "_n_joints", 0), 1) * 10)
        self._check(self._lib.mip_set_poses(self._ctx, poses.ctypes.data, n, 0))

    def set_poses_device(self, ptr, n):
        """Borrow a device buffer of n x J x 10 floats (not copied)."""
        self._check(self._lib.mip_set_poses(self._ctx, ptr, int(n), 1))

    def run_skinned(self, frame, palette=0, async_=False, **outputs):
        """One frame of skinned instances; outputs as prepare_outputs (device pointers)."""
        out = self.prepare_outputs(async_=async_, **outputs)
        rc = self._lib.mip_run_skinned(self._ctx, C.addressof(frame), C.addressof(out), palette or None)
        if rc != 0:
            self._check(rc)

    def run_views(self, frames, prepared_outputs):
        """Up to 16 views (per-light culled lists, cascades ...) of the resident instances, four per launch:
        frames[v] (make_frame) with prepared_outputs[v] (prepare_outputs: bitmap / draw_cmds / draw_count / index total)."""
        k = len(frames)
        fr = (MipFrame * k)()
        ou = (MipOutputs * k)()
        for v in range(k):
            C.memmove(C.addressof(fr[v]), C.addressof(frames[v]), C.sizeof(MipFrame))
            C.memmove(C.addressof(ou[v]), C.addressof(prepared_outputs[v]), C.sizeof(MipOutputs))
        self._check(self._lib.mip_run_views(self._ctx, C.addressof(fr), C.addressof(ou), k))

    def light_draw_lists(self, light_pos_xyz, out_cmds_ptr, first_instance_base=0, async_=False):
        """Per-light shadow-pass draw lists (shadow_mapping.rs:405-478): n_lights x n commands, light-major,
        into device memory at out_cmds_ptr."""
        lights = np.ascontiguousarray(light_pos_xyz, dtype=np.float32).reshape(-1, 3)
        self._check(self._lib.mip_light_draw_lists(self._ctx, lights.ctypes.data, len(lights), int(first_instance_base),
                                                   out_cmds_ptr, 1 if async_ else 0))

    # -- occlusion culling (extension) --
    def build_depth_pyramid(self, depth_ptr, width, height, pyramid_ptr, row_pitch_bytes=None, format=_lib.MIP_DEPTH_UNORM16,
                            async_=False):
        """The max pyramid of a device depth image (D16_UNORM or D32_SFLOAT) into device memory of
        depth_pyramid_layout(width, height)["bytes"], on the stream the next run / run_occluded will use."""
        if row_pitch_bytes is None:
            row_pitch_bytes = int(width) * (2 if format == _lib.MIP_DEPTH_UNORM16 else 4)
        self._check(self._lib.mip_build_depth_pyramid(self._ctx, depth_ptr or None, int(width), int(height), int(row_pitch_bytes),
                                                      int(format), pyramid_ptr or None, 1 if async_ else 0))

    def run_occluded(self, frame, occlusion, outputs):
        """mip_run_occluded: `frame` from make_frame, `occlusion` from make_occlusion, `outputs` a MipOutputs (prepare_outputs, or
        one built by hand): every output as mip_run gives it for the scene in which the non-candidates and the occluded instances
        had been frustum-culled."""
        self._check(self._lib.mip_run_occluded(self._ctx, C.addressof(frame), C.addressof(occlusion), C.addressof(outputs)))

    # -- batched draws (extension) --
    @staticmethod
    def _batch_outputs(batch_cmds, batch_count, instance_ids, instance_count, batch_model, async_):
        out = MipBatchOutputs()
        out.struct_size = C.sizeof(MipBatchOutputs)
        out.flags = _lib.MIP_OUT_DEVICE | (_lib.MIP_OUT_ASYNC if async_ else 0)
        out.batch_cmds = batch_cmds or None
        out.batch_count = batch_count or None
        out.instance_ids = instance_ids or None
        out.instance_count = instance_count or None
        out.batch_model = batch_model or None
        return out

    def batch_draws(self, frame, visible_bitmap_ptr, *, batch_cmds, batch_count, instance_ids, instance_count=0, batch_model=0,
                    async_=False):
        """mip_batch_draws: one instanced command per non-empty (mesh, LOD) bucket of the members of `visible_bitmap_ptr` (a
        device bitmap in MipOutputs.visible_bitmap's layout), the entity ids in slot order and, optionally, the members' model
        matrices in slot order. Device pointers; enqueued behind the frame this context issued last. `frame` from make_frame
        (its cam_pos and first_instance_base are read)."""
        out = self._batch_outputs(batch_cmds, batch_count, instance_ids, instance_count, batch_model, async_)
        self._check(self._lib.mip_batch_draws(self._ctx, C.addressof(frame), visible_bitmap_ptr or None, C.addressof(out)))

    def batch_draws_lods(self, frame, visible_bitmap_ptr, policy, *, batch_cmds, batch_count, instance_ids, instance_count=0,
                         batch_model=0, async_=False):
        """mip_batch_draws_lods: batch_draws over the whole LOD chain — one instanced command per non-empty (mesh, LOD) bucket,
        bucket = lod_base[mesh] + lod, the LOD chosen by `policy` (make_lod_policy). batch_cmds needs room for
        min(sum of n_lods, N) commands; everything else as batch_draws."""
        out = self._batch_outputs(batch_cmds, batch_count, instance_ids, instance_count, batch_model, async_)
        self._check(self._lib.mip_batch_draws_lods(self._ctx, C.addressof(frame), visible_bitmap_ptr or None, C.addressof(policy),
                                                   C.addressof(out)))

    def batch_draws_ordered(self, frame, visible_bitmap_ptr, policy, order, *, batch_cmds, batch_count, instance_ids, instance_count=0,
                            batch_model=0, async_=False):
        """mip_batch_draws_ordered: batch_draws_lods with the members of every bucket in depth order. `order` is
        MIP_BATCH_ORDER_DRAW_INDEX / NEAR_FIRST / FAR_FIRST (or "draw_index" / "near_first" / "far_first"); the commands and
        counts do not depend on it. The depth key is the squared distance to frame.cam_pos at about 0.4 % resolution, ties in
        draw order. NEAR_FIRST / FAR_FIRST take tables of at most 65 536 buckets (sum of n_lods)."""
        if isinstance(order, str):
            order = {"draw_index": _lib.MIP_BATCH_ORDER_DRAW_INDEX, "near_first": _lib.MIP_BATCH_ORDER_NEAR_FIRST,
                     "far_first": _lib.MIP_BATCH_ORDER_FAR_FIRST}[order]
        out = self._batch_outputs(batch_cmds, batch_count, instance_ids, instance_count, batch_model, async_)
        self._check(self._lib.mip_batch_draws_ordered(self._ctx, C.addressof(frame), visible_bitmap_ptr or None, C.addressof(policy),
                                                      int(order), C.addressof(out)))

    def batch_draws_sorted(self, frame, visible_bitmap_ptr, policy, sort, *, batch_cmds, batch_count, instance_ids, instance_count=0,
                           batch_model=0, async_=False):
        """mip_batch_draws_sorted: the members of batch_draws_lods in one depth order across all buckets (`sort` from
        make_sort_policy: radial or view-axis depth, near or far first, 16 / 24 / 32 key bits; ties in draw order) and one
        instanced command per run of neighbouring slots that draw the same bucket — the transparent pass. batch_cmds needs room
        for N commands; everything else as batch_draws_ordered."""
        out = self._batch_outputs(batch_cmds, batch_count, instance_ids, instance_count, batch_model, async_)
        self._check(self._lib.mip_batch_draws_sorted(self._ctx, C.addressof(frame), visible_bitmap_ptr or None, C.addressof(policy),
                                                     C.addressof(sort), C.addressof(out)))

    def batch_draws_views(self, frames, visible_bitmap_ptrs, policy, *, batch_cmds, cmd_stride, batch_counts, instance_ids,
                          view_first_slot=0, async_=False):
        """mip_batch_draws_views: batch_draws_lods for up to 16 views in one call. frames[v] (make_frame: cam_pos and
        first_instance_base are read) goes with visible_bitmap_ptrs[v], a device bitmap or 0 / None for every resident
        instance. View v's commands are entries [v * cmd_stride, v * cmd_stride + batch_counts[v]) of batch_cmds
        (cmd_stride >= min(sum of n_lods, N)); all views share instance_ids (room for len(frames) x N words), firstInstance is
        the absolute slot there, view_first_slot (len(frames) + 1 words, optional) the first slot of every view. Device
        pointers; enqueued on the context's first stream, behind a run_views."""
        k = len(frames)
        if len(visible_bitmap_ptrs) != k:
            raise ValueError("one bitmap pointer (or None) per frame")
        fr = (MipFrame * max(k, 1))()
        for v in range(k):
            C.memmove(C.addressof(fr[v]), C.addressof(frames[v]), C.sizeof(MipFrame))
        bm = (C.c_void_p * max(k, 1))(*[int(b) if b else None for b in visible_bitmap_ptrs])
        out = MipViewBatchOutputs()
        out.struct_size = C.sizeof(MipViewBatchOutputs)
        out.flags = _lib.MIP_OUT_DEVICE | (_lib.MIP_OUT_ASYNC if async_ else 0)
        out.batch_cmds = batch_cmds or None
        out.cmd_stride = int(cmd_stride)
        out.batch_counts = batch_counts or None
        out.instance_ids = instance_ids or None
        out.view_first_slot = view_first_slot or None
        self._check(self._lib.mip_batch_draws_views(self._ctx, C.addressof(fr), C.addressof(bm), k, C.addressof(policy), C.addressof(out)))

    def batch_draws_shard(self, frame, visible_bitmap_ptr, policy, chunk_ptr, ids_capacity, async_=False):
        """mip_batch_draws_shard: batch_draws_lods of this context's instances — one shard of a sharded scene — into a batch
        chunk at `chunk_ptr` (device memory, 16-byte aligned, batch_chunk_bytes(B, ids_capacity) bytes): the header {members, B,
        0, 0}, the dense per-bucket counts, the ids in slot order. ids_capacity >= the resident instances."""
        flags = _lib.MIP_OUT_DEVICE | (_lib.MIP_OUT_ASYNC if async_ else 0)
        self._check(self._lib.mip_batch_draws_shard(self._ctx, C.addressof(frame), visible_bitmap_ptr or None, C.addressof(policy),
                                                    chunk_ptr or None, int(ids_capacity), flags))

    def merge_batches(self, chunks_ptr, n_chunks, chunk_stride_bytes, chunk_capacity, *, batch_cmds, batch_count, instance_ids,
                      instance_count=0, async_=False):
        """mip_merge_batches: the batch chunks of n_chunks shards (rank order, chunk_stride_bytes apart, as an all-gather lays
        them out) merged into what ONE batch_draws_lods call writes for the unsharded scene. instance_ids needs room for
        n_chunks x chunk_capacity words, batch_cmds for min(B, n_chunks x chunk_capacity) commands. A corrupt chunk is
        MIP_ERR_DEVICE, a chunk with more members than chunk_capacity MIP_ERR_CAPACITY (from wait() for an async call); both
        leave two zero counts and nothing else."""
        out = self._batch_outputs(batch_cmds, batch_count, instance_ids, instance_count, 0, async_)
        self._check(self._lib.mip_merge_batches(self._ctx, chunks_ptr or None, int(n_chunks), int(chunk_stride_bytes), int(chunk_capacity),
                                                C.addressof(out)))

    # -- cluster culling (extension) --
    def build_clusters(self):
        """mip_build_clusters: cuts every level of every mesh into clusters of 64 triangles and builds their boxes on the device
        from the resident geometry (set_mesh_table and set_geometry first; either of them makes the table stale again)."""
        self._check(self._lib.mip_build_clusters(self._ctx))

    def cluster_count(self):
        """Clusters in the table, 0 without a valid one."""
        return int(self._lib.mip_cluster_count(self._ctx))

    def read_cluster_boxes(self):
        """The table's boxes as a (clusters, 6) float32 array (min xyz, max xyz), bucket-major: the build, on its own."""
        boxes = np.zeros((self.cluster_count(), 6), np.float32)
        self._check(self._lib.mip_read_cluster_boxes(self._ctx, boxes.ctypes.data, len(boxes)))
        return boxes

    def cull_clusters(self, frame, visible_bitmap_ptr, policy, outputs, occlusion=None):
        """mip_cull_clusters: the frustum test (frame's planes) and, with `occlusion` (make_occlusion: pyramid, extent and pv),
        the Hi-Z test on every 64-triangle cluster of every member of `visible_bitmap_ptr` under `policy` (make_lod_policy);
        one command per run of surviving clusters of an instance into `outputs` (make_cluster_outputs), drawn from the source
        mesh's own index range. Enqueued behind the frame this context issued last. MIP_ERR_CAPACITY (from wait() for an
        asynchronous call) when the runs do not fit cmd_capacity or the work items exceed work_capacity."""
        self._check(self._lib.mip_cull_clusters(self._ctx, C.addressof(frame), visible_bitmap_ptr or None, C.addressof(policy),
                                                C.addressof(occlusion) if occlusion is not None else None, C.addressof(outputs)))

    def cull_clusters_phase(self, frame, visible_bitmap_ptr, policy, outputs, occlusion, record):
        """mip_cull_clusters_phase: cull_clusters in two phases around the frame's own depth. With a FIRST `record`
        (make_cluster_record) the outputs are cull_clusters' under `occlusion` (last frame's pyramid) and the record names every
        cluster that passed the planes and failed the Hi-Z test; with a SECOND record — the same frame, bitmap and policy,
        `occlusion` the pyramid rebuilt from what phase 1 drew — exactly those clusters are tested again and the ones visible
        now are written, one command per run. The context orders SECOND behind FIRST. MIP_ERR_DEVICE (from wait() for an
        asynchronous call) when the record's header does not match the call's work items and members."""
        self._check(self._lib.mip_cull_clusters_phase(self._ctx, C.addressof(frame), visible_bitmap_ptr or None, C.addressof(policy),
                                                      C.addressof(occlusion) if occlusion is not None else None, C.addressof(outputs),
                                                      C.addressof(record) if record is not None else None))

    def cull_cluster_triangles(self, frame, visible_bitmap_ptr, policy, outputs, occlusion=None):
        """mip_cull_cluster_triangles: cull_clusters, then the per-triangle stage's test (frame's pv) on every triangle of the
        surviving clusters. `outputs` (make_cluster_triangle_outputs) receives the surviving triangles' indices as one dense
        stream and one command per run of surviving clusters into it — a run with no surviving triangle keeps its command with
        indexCount 0. MIP_ERR_CAPACITY (from wait() for an asynchronous call) when the stream does not fit index_capacity
        (nothing is written; stats[4] says how many triangles survive), the runs do not fit cmd_capacity or the work items
        exceed work_capacity."""
        self._check(self._lib.mip_cull_cluster_triangles(self._ctx, C.addressof(frame), visible_bitmap_ptr or None, C.addressof(policy),
                                                         C.addressof(occlusion) if occlusion is not None else None, C.addressof(outputs)))

    def cull_clusters_views(self, frames, visible_bitmap_ptrs, policy, outputs):
        """mip_cull_clusters_views: cull_clusters' frustum test for up to 16 views in one call. frames[v] (make_frame: planes
        and first_instance_base are read; the level of every instance comes from frames[0]'s cam_pos for ALL views) goes with
        visible_bitmap_ptrs[v], a device bitmap or 0 / None for every resident instance. View v's commands are entries
        [v * cmd_stride, v * cmd_stride + cmd_counts[v]) of `outputs` (make_cluster_view_outputs). Enqueued on the context's
        first stream, behind a run_views. MIP_ERR_CAPACITY (from wait() for an asynchronous call) when a view's runs do not
        fit cmd_stride or the work items exceed work_capacity."""
        k = len(frames)
        if len(visible_bitmap_ptrs) != k:
            raise ValueError("one bitmap pointer (or None) per frame")
        fr = (MipFrame * max(k, 1))()
        for v in range(k):
            C.memmove(C.addressof(fr[v]), C.addressof(frames[v]), C.sizeof(MipFrame))
        bm = (C.c_void_p * max(k, 1))(*[int(b) if b else None for b in visible_bitmap_ptrs])
        self._check(self._lib.mip_cull_clusters_views(self._ctx, C.addressof(fr), C.addressof(bm), k, C.addressof(policy), C.addressof(outputs)))

    # -- cluster culling with normal cones (extension) --
    def build_cluster_cones(self):
        """mip_build_cluster_cones: one normal cone per cluster of the valid cluster table (build_clusters first; whatever makes
        that table stale makes the cones stale)."""
        self._check(self._lib.mip_build_cluster_cones(self._ctx))

    def read_cluster_cones(self):
        """The cone table as a (clusters, 8) float32 array {axis xyz, k, centre xyz, r}, bucket-major; k = +inf: no cone."""
        cones = np.zeros((self.cluster_count(), 8), np.float32)
        self._check(self._lib.mip_read_cluster_cones(self._ctx, cones.ctypes.data, len(cones)))
        return cones

    def cull_clusters_cone(self, frame, visible_bitmap_ptr, policy, cone, outputs, occlusion=None):
        """mip_cull_clusters_cone: cull_clusters with the normal-cone back-face test of `cone` (make_cluster_cone) in front: a
        cluster all of whose triangles face away from the cone's eye is removed before its box is tested."""
        self._check(self._lib.mip_cull_clusters_cone(self._ctx, C.addressof(frame), visible_bitmap_ptr or None, C.addressof(policy),
                                                     C.addressof(occlusion) if occlusion is not None else None,
                                                     C.addressof(cone) if cone is not None else None, C.addressof(outputs)))

    def cull_cluster_triangles_cone(self, frame, visible_bitmap_ptr, policy, cone, outputs, occlusion=None):
        """mip_cull_cluster_triangles_cone: cull_cluster_triangles over the clusters cull_clusters_cone leaves. With cone =
        make_cluster_cone(frame's pv) the cone removes only triangles the per-triangle test would cull, up to that test's own
        float rounding on slivers."""
        self._check(self._lib.mip_cull_cluster_triangles_cone(self._ctx, C.addressof(frame), visible_bitmap_ptr or None, C.addressof(policy),
                                                              C.addressof(occlusion) if occlusion is not None else None,
                                                              C.addressof(cone) if cone is not None else None, C.addressof(outputs)))

    # -- the visible-cluster list (extension) --
    def list_clusters(self, frame, visible_bitmap_ptr, policy, outputs, occlusion=None, cone=None):
        """mip_list_clusters: cull_clusters (or, with `cone`, cull_clusters_cone) with a flat list in the commands' place: one
        16-byte entry per surviving cluster, in (instance, cluster) order, and the arguments of the ONE vkCmdDrawIndirect that
        draws them, into `outputs` (make_cluster_list_outputs). The list is the cluster-by-cluster expansion of what
        cull_clusters / cull_clusters_cone write for the same arguments."""
        self._check(self._lib.mip_list_clusters(self._ctx, C.addressof(frame), visible_bitmap_ptr or None, C.addressof(policy),
                                                C.addressof(occlusion) if occlusion is not None else None,
                                                C.addressof(cone) if cone is not None else None, C.addressof(outputs)))

    def list_cluster_triangles(self, frame, visible_bitmap_ptr, policy, outputs, occlusion=None, cone=None):
        """mip_list_cluster_triangles: list_clusters with the per-triangle stage's test (frame's pv) behind the cluster cull.
        `outputs` (make_cluster_triangle_list_outputs) receives one entry per surviving cluster that keeps at least one triangle —
        a subsequence of list_clusters' list — and beside entry k the 64-bit mask of the cluster's surviving triangles: no index
        stream, no commands, and no entry for a cluster whose triangles are all culled. MIP_ERR_CAPACITY (from wait() for an
        asynchronous call) when the entries do not fit entry_capacity or the work items exceed work_capacity."""
        self._check(self._lib.mip_list_cluster_triangles(self._ctx, C.addressof(frame), visible_bitmap_ptr or None, C.addressof(policy),
                                                         C.addressof(occlusion) if occlusion is not None else None,
                                                         C.addressof(cone) if cone is not None else None, C.addressof(outputs)))

    def list_clusters_views(self, frames, visible_bitmap_ptrs, policy, outputs):
        """mip_list_clusters_views: cull_clusters_views with list_clusters' flat list in the commands' place, one list and one
        indirect draw per view. frames and visible_bitmap_ptrs are cull_clusters_views' (one level for ALL views, from
        frames[0]'s cam_pos). View v's entries are [v * entry_stride, v * entry_stride + entry_counts[v]) of `outputs`
        (make_cluster_view_list_outputs), and draw_args[4 v ..] = {192, entry_counts[v], 0, v * entry_stride}. Enqueued on the
        context's first stream, behind a run_views. MIP_ERR_CAPACITY (from wait() for an asynchronous call) when a view's
        survivors do not fit entry_stride or the work items exceed work_capacity."""
        k = len(frames)
        if len(visible_bitmap_ptrs) != k:
            raise ValueError("one bitmap pointer (or None) per frame")
        fr = (MipFrame * max(k, 1))()
        for v in range(k):
            C.memmove(C.addressof(fr[v]), C.addressof(frames[v]), C.sizeof(MipFrame))
        bm = (C.c_void_p * max(k, 1))(*[int(b) if b else None for b in visible_bitmap_ptrs])
        self._check(self._lib.mip_list_clusters_views(self._ctx, C.addressof(fr), C.addressof(bm), k, C.addressof(policy), C.addressof(outputs)))

    def list_clusters_views_occluded(self, frames, visible_bitmap_ptrs, occlusions, policy, outputs):
        """mip_list_clusters_views_occluded: list_clusters_views with a depth pyramid per view. occlusions[v] is a
        make_occlusion(...) (pyramid, extents and pv are read; no candidates, no occluded bitmap, no flags) or None: view v is
        then tested against its planes alone. View v's list is what list_clusters(frames[v] with frames[0]'s cam_pos, ...,
        occlusion=occlusions[v]) writes; `hidden` of `outputs` (make_cluster_view_occluded_list_outputs) counts per view the
        work items that passed the planes and are occluded. Enqueued on the context's first stream, behind a run_views and
        behind pyramids built for the next run: no wait is needed. MIP_ERR_CAPACITY as for list_clusters_views."""
        k = len(frames)
        if len(visible_bitmap_ptrs) != k or len(occlusions) != k:
            raise ValueError("one bitmap pointer (or None) and one occlusion (or None) per frame")
        fr = (MipFrame * max(k, 1))()
        for v in range(k):
            C.memmove(C.addressof(fr[v]), C.addressof(frames[v]), C.sizeof(MipFrame))
        bm = (C.c_void_p * max(k, 1))(*[int(b) if b else None for b in visible_bitmap_ptrs])
        oc = (C.c_void_p * max(k, 1))(*[C.addressof(o) if o is not None else None for o in occlusions])
        self._check(self._lib.mip_list_clusters_views_occluded(self._ctx, C.addressof(fr), C.addressof(bm), C.addressof(oc), k, C.addressof(policy),
                                                               C.addressof(outputs)))

    def list_clusters_phase(self, frame, visible_bitmap_ptr, policy, outputs, occlusion, record):
        """mip_list_clusters_phase: cull_clusters_phase with list_clusters' flat list in the commands' place. With a FIRST
        `record` (make_cluster_record) one entry per cluster that survives under `occlusion` (last frame's pyramid), and the
        record cull_clusters_phase writes; with a SECOND record one entry per recorded cluster that is visible under the new
        `occlusion`. The list starts at entry *entry_base of `outputs` (make_cluster_phase_list_outputs), read on the device:
        with entry_base = FIRST's entry_count SECOND appends behind FIRST's entries. MIP_ERR_CAPACITY / MIP_ERR_DEVICE as for
        list_clusters and cull_clusters_phase (from wait() for an asynchronous call)."""
        self._check(self._lib.mip_list_clusters_phase(self._ctx, C.addressof(frame), visible_bitmap_ptr or None, C.addressof(policy),
                                                      C.addressof(occlusion) if occlusion is not None else None, C.addressof(outputs),
                                                      C.addressof(record) if record is not None else None))

    # -- diagnostics --
    def timings(self):
        t = MipTimings()
        self._check(self._lib.mip_get_timings(self._ctx, C.byref(t)))
        return {k: getattr(t, k) for k, _ in MipTimings._fields_}

    def reset_timings(self):
        self._check(self._lib.mip_reset_timings(self._ctx))
