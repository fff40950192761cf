"""numpy restatement of batched draws over the whole LOD chain (include/mi_instance_pipeline.h, mip_batch_draws_lods), written
from the header's text: the selection rule in float32 with every product and sum rounded once, in the order the header writes
them; bucket = lod_base[mesh] + lod; the slots, commands and ids of mip_batch_draws. Returns what
batch_restatement.batch_draws returns. Not reference behaviour: this file is what the library is checked against."""
import numpy as np

from batch_restatement import bitmap_bits
from renderer_amd.pipeline import DRAW_CMD_DTYPE

F = np.float32
DISTANCE, RELATIVE = 0, 1
N_SWITCH = 5  # MIP_MAX_LODS - 1
INF = float("inf")
PIN_SWITCH_SQ = (100.00000762939453125, INF, INF, INF, INF)  # the header's PIN: mip_batch_draws, byte for byte


def check_policy(mode, switch_sq):
    """The header's THRESHOLDS as float32[5], or ValueError (the library's MIP_ERR_INVALID_ARGUMENT)."""
    sw = np.asarray(switch_sq, F).reshape(-1)
    if mode not in (DISTANCE, RELATIVE) or len(sw) != N_SWITCH:
        raise ValueError("mode / number of thresholds")
    if np.isnan(sw).any() or (sw < 0).any() or (sw[1:] < sw[:-1]).any():
        raise ValueError("thresholds must be >= 0, not NaN and non-decreasing")
    return sw


def select_lods(pos, scale, mesh_id, meshes, cam_pos, mode, switch_sq):
    """lod = #{ k in [0, n_lods - 1) : q > b_k } per instance (int64). Every intermediate is a float32 array: numpy rounds each
    elementwise product and sum once, and the parentheses below are the header's."""
    sw = check_policy(mode, switch_sq)
    pos = np.asarray(pos, F).reshape(-1, 3)
    mesh_id = np.asarray(mesh_id, np.uint32).reshape(-1).astype(np.int64)
    cam = np.asarray(cam_pos, F).reshape(3)
    n_lods = meshes["n_lods"][mesh_id].astype(np.int64)
    with np.errstate(all="ignore"):
        dx, dy, dz = cam[0] - pos[:, 0], cam[1] - pos[:, 1], cam[2] - pos[:, 2]
        q = (dx * dx + dy * dy) + dz * dz
        if mode == RELATIVE:
            e = (np.asarray(meshes["aabb_max"], F) - np.asarray(meshes["aabb_min"], F))[mesh_id]
            diag_sq = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
            s = np.asarray(scale, F).reshape(-1)
            unit = (s * s) * diag_sq
        assert q.dtype == F
        lod = np.zeros(len(pos), np.int64)
        for k in range(N_SWITCH):
            b = sw[k] * unit if mode == RELATIVE else np.full(len(pos), sw[k], F)
            assert b.dtype == F
            lod += ((k < n_lods - 1) & (q > b)).astype(np.int64)   # a comparison with a NaN is False
    return lod


def lod_bases(meshes):
    """Exclusive prefix sum of n_lods over the table (int64[m]) and B, the number of buckets."""
    n_lods = meshes["n_lods"].astype(np.int64)
    ends = np.cumsum(n_lods)
    return ends - n_lods, int(ends[-1]) if len(ends) else 0


def batch_draws_lods(pos, scale, mesh_id, meshes, cam_pos, visible_bitmap, mode, switch_sq, first_instance_base=0, model=None):
    """Returns dict(cmds (DRAW_CMD_DTYPE), count, ids (uint32), members, order (instance of every slot), model (or None), lod
    (the level every instance selects))."""
    pos = np.asarray(pos, F).reshape(-1, 3)
    n = len(pos)
    mesh_id = np.asarray(mesh_id, np.uint32).reshape(-1).astype(np.int64)
    lod = select_lods(pos, scale, mesh_id, meshes, cam_pos, mode, switch_sq)
    length = meshes["index_len"][mesh_id, lod] if n else np.zeros(0, np.uint32)
    member = bitmap_bits(visible_bitmap, n) & (length > 0)
    inst = np.nonzero(member)[0]
    base, _ = lod_bases(meshes)
    bucket = base[mesh_id[inst]] + lod[inst]
    by_bucket = np.argsort(bucket, kind="stable")          # stable: draw order inside a bucket
    order = inst[by_bucket]
    buckets, first_slot, counts = np.unique(bucket[by_bucket], return_index=True, return_counts=True)
    b_mesh = np.searchsorted(base, buckets, side="right") - 1   # the last mesh whose base is <= the bucket (n_lods >= 1)
    b_lod = buckets - base[b_mesh]
    cmds = np.zeros(len(buckets), DRAW_CMD_DTYPE)
    cmds["indexCount"] = meshes["index_len"][b_mesh, b_lod]
    cmds["instanceCount"] = counts
    cmds["firstIndex"] = meshes["index_offset"][b_mesh, b_lod]
    cmds["vertexOffset"] = meshes["vertex_offset"][b_mesh]
    cmds["firstInstance"] = first_slot
    ids = ((order + int(first_instance_base)) & 0xFFFFFFFF).astype(np.uint32)
    return dict(cmds=cmds, count=len(cmds), ids=ids, members=len(order), order=order, lod=lod,
                model=None if model is None else np.asarray(model).reshape(-1, 16)[order])


def per_instance_list(pos, scale, mesh_id, meshes, cam_pos, visible_bitmap, mode, switch_sq, first_instance_base=0):
    """The same frame as one command per member, in draw order (what batch_restatement.expand of the batches must give):
    written as a loop over the instances, sharing only select_lods with batch_draws_lods."""
    pos = np.asarray(pos, F).reshape(-1, 3)
    mesh_id = np.asarray(mesh_id, np.uint32).reshape(-1)
    lod = select_lods(pos, scale, mesh_id, meshes, cam_pos, mode, switch_sq)
    bits = bitmap_bits(visible_bitmap, len(pos))
    rows = []
    for i in range(len(pos)):
        m, l = int(mesh_id[i]), int(lod[i])
        if bits[i] and meshes["index_len"][m, l] > 0:
            rows.append((int(meshes["index_len"][m, l]), 1, int(meshes["index_offset"][m, l]), int(meshes["vertex_offset"][m]),
                         (i + int(first_instance_base)) & 0xFFFFFFFF))
    return np.array(rows, DRAW_CMD_DTYPE) if rows else np.zeros(0, DRAW_CMD_DTYPE)
