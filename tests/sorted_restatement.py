"""numpy restatement of globally depth-sorted batched draws (include/mi_instance_pipeline.h, mip_batch_draws_sorted), written
from the header's text: members, LODs and buckets are lod_restatement's; U is the monotone 32-bit image of the float32 depth (q
of the selection rule, or z along the caller's axis), K its leading depth_bits, D = K or (Umax >> s) - K; the slots are the
members sorted stably by D; one command per maximal run of equal bucket in the slots. Returns what
lod_restatement.batch_draws_lods returns, plus `bucket` (of every slot). Not reference behaviour: this file is what the library
is checked against."""
import numpy as np

import lod_restatement as lr
from batch_restatement import bitmap_bits
from renderer_amd.pipeline import DRAW_CMD_DTYPE

F = np.float32
RADIAL, VIEW_AXIS = 0, 1
METRICS = (RADIAL, VIEW_AXIS)
NEAR_FIRST, FAR_FIRST = 1, 2
ORDERS = (NEAR_FIRST, FAR_FIRST)
DEPTH_BITS = (16, 24, 32)
U_MAX = {RADIAL: 0x7F800000, VIEW_AXIS: 0xFF800000}


def check_sort(metric, order, depth_bits, axis):
    """The header's refusals as ValueError (the library's MIP_ERR_INVALID_ARGUMENT); the axis as float32[3]."""
    if metric not in METRICS or order not in ORDERS or depth_bits not in DEPTH_BITS:
        raise ValueError("metric / order / depth_bits")
    ax = np.asarray(axis, F).reshape(3)
    if metric == VIEW_AXIS and not np.isfinite(ax).all():
        raise ValueError("a non-finite axis component")
    return ax


def u_radial(q):
    """U of float32 q values (a sum of squares: never negative): bits(q), 0x7F800000 for a NaN (int64)."""
    q = np.asarray(q, F)
    return np.where(np.isnan(q), U_MAX[RADIAL], q.view(np.uint32).astype(np.int64))


def u_view_axis(z):
    """U of float32 z values (int64): 0xFF800000 for a NaN; else u = 0 for either zero, bits(z) otherwise, and
    U = u ^ 0x80000000 where the sign bit of u is clear, ~u where it is set."""
    z = np.asarray(z, F)
    u = np.where(z == 0, np.uint32(0), z.view(np.uint32)).astype(np.uint32)
    flipped = np.where(u & np.uint32(0x80000000) != 0, ~u, u ^ np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isnan(z), U_MAX[VIEW_AXIS], flipped.astype(np.int64))


def d_of_u(u, metric, order, depth_bits):
    """D of U values (int64): K = U >> s with s = 32 - depth_bits; K near first, (Umax >> s) - K far first."""
    s = 32 - depth_bits
    k = np.asarray(u, np.int64) >> s
    return k if order == NEAR_FIRST else (U_MAX[metric] >> s) - k


def depth_u(pos, cam_pos, metric, axis=(0.0, 0.0, 0.0)):
    """U of every instance: the header's expressions, every product and sum a float32 array operation, rounded once."""
    pos = np.asarray(pos, F).reshape(-1, 3)
    cam = np.asarray(cam_pos, F).reshape(3)
    ax = np.asarray(axis, F).reshape(3)
    with np.errstate(all="ignore"):
        if metric == RADIAL:
            dx, dy, dz = cam[0] - pos[:, 0], cam[1] - pos[:, 1], cam[2] - pos[:, 2]
            q = (dx * dx + dy * dy) + dz * dz
            assert q.dtype == F
            return u_radial(q)
        ex, ey, ez = pos[:, 0] - cam[0], pos[:, 1] - cam[1], pos[:, 2] - cam[2]
        z = (ex * ax[0] + ey * ax[1]) + ez * ax[2]
        assert z.dtype == F
        return u_view_axis(z)


def depth_key(pos, cam_pos, metric, order, depth_bits, axis=(0.0, 0.0, 0.0)):
    ax = check_sort(metric, order, depth_bits, axis)
    return d_of_u(depth_u(pos, cam_pos, metric, ax), metric, order, depth_bits)


def run_commands(bucket, meshes):
    """One command per maximal run of equal bucket in `bucket` (the bucket of every slot): the head's slot, the distance to the
    next head (or to the end), and the three words mip_batch_draws_lods writes for the bucket."""
    bucket = np.asarray(bucket, np.int64)
    members = len(bucket)
    if members == 0:
        return np.zeros(0, DRAW_CMD_DTYPE)
    head = np.ones(members, bool)
    head[1:] = bucket[1:] != bucket[:-1]
    first = np.nonzero(head)[0]
    ends = np.append(first[1:], members)
    base, _ = lr.lod_bases(meshes)
    b = bucket[first]
    b_mesh = np.searchsorted(base, b, side="right") - 1
    b_lod = b - base[b_mesh]
    cmds = np.zeros(len(first), DRAW_CMD_DTYPE)
    cmds["indexCount"] = meshes["index_len"][b_mesh, b_lod]
    cmds["instanceCount"] = ends - first
    cmds["firstIndex"] = meshes["index_offset"][b_mesh, b_lod]
    cmds["vertexOffset"] = meshes["vertex_offset"][b_mesh]
    cmds["firstInstance"] = first
    return cmds


def batch_draws_sorted(pos, scale, mesh_id, meshes, cam_pos, visible_bitmap, mode, switch_sq, metric, order, depth_bits, axis=(0.0, 0.0, 0.0),
                       first_instance_base=0, model=None):
    """Returns dict(cmds, count, ids, members, order (instance of every slot), bucket (of every slot), model (or None), lod)."""
    pos = np.asarray(pos, F).reshape(-1, 3)
    n = len(pos)
    mid = np.asarray(mesh_id, np.uint32).reshape(-1).astype(np.int64)
    d = depth_key(pos, cam_pos, metric, order, depth_bits, axis)
    assert n == 0 or (0 <= d.min() and d.max() < 0xFFFFFFFF)
    lod = lr.select_lods(pos, scale, mesh_id, meshes, cam_pos, mode, switch_sq)
    length = meshes["index_len"][mid, lod] if n else np.zeros(0, np.uint32)
    inst = np.nonzero(bitmap_bits(visible_bitmap, n) & (length > 0))[0]
    base, _ = lr.lod_bases(meshes)
    slots = inst[np.argsort(d[inst], kind="stable")]          # by D; equal D in draw order
    bucket = base[mid[slots]] + lod[slots]
    cmds = run_commands(bucket, meshes)
    ids = ((slots + int(first_instance_base)) & 0xFFFFFFFF).astype(np.uint32)
    return dict(cmds=cmds, count=len(cmds), ids=ids, members=len(slots), order=slots, bucket=bucket, lod=lod,
                model=None if model is None else np.asarray(model).reshape(-1, 16)[slots])
