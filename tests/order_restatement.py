"""numpy restatement of depth-ordered batched draws (include/mi_instance_pipeline.h, mip_batch_draws_ordered), written from the
header's text: members, LODs and buckets are lod_restatement's; the depth key is bits(q) >> 16 of the float32 q the selection
rule forms, 0x7F80 for a NaN; the slots are the members sorted by (bucket, D, draw index). Returns what
lod_restatement.batch_draws_lods returns. Not reference behaviour: this file is what the library is checked against."""
import numpy as np

import lod_restatement as lr
from batch_restatement import bitmap_bits

F = np.float32
DRAW_INDEX, NEAR_FIRST, FAR_FIRST = 0, 1, 2
ORDERS = (DRAW_INDEX, NEAR_FIRST, FAR_FIRST)
K_MAX = 0x7F80          # bits(+inf) >> 16: the K of q = +inf and of a NaN
MAX_BUCKETS = 1 << 16   # NEAR_FIRST / FAR_FIRST: bucket << 16 | D is a 32-bit key


def k_of_q(q):
    """K of float32 q values (a sum of squares: never negative): bits(q) >> 16, 0x7F80 for a NaN of either sign (int64)."""
    q = np.asarray(q, F)
    k = (q.view(np.uint32) >> np.uint32(16)).astype(np.int64)
    return np.where(np.isnan(q), K_MAX, k)


def depth_key(pos, cam_pos, order):
    """D of every instance (int64): K (NEAR_FIRST), 0x7F80 - K (FAR_FIRST), 0 (DRAW_INDEX). q is the header's expression, every
    product and sum a float32 array operation, rounded once."""
    if order not in ORDERS:
        raise ValueError("order")
    pos = np.asarray(pos, F).reshape(-1, 3)
    cam = np.asarray(cam_pos, F).reshape(3)
    with np.errstate(all="ignore"):
        dx, dy, dz = cam[0] - pos[:, 0], cam[1] - pos[:, 1], cam[2] - pos[:, 2]
        q = (dx * dx + dy * dy) + dz * dz
    assert q.dtype == F
    k = k_of_q(q)
    if order == NEAR_FIRST:
        return k
    if order == FAR_FIRST:
        return K_MAX - k
    return np.zeros(len(pos), np.int64)


def batch_draws_ordered(pos, scale, mesh_id, meshes, cam_pos, visible_bitmap, mode, switch_sq, order, first_instance_base=0, model=None):
    """Returns dict(cmds, count, ids, members, order (instance of every slot), model (or None), lod), as
    lod_restatement.batch_draws_lods. Raises OverflowError where the library returns MIP_ERR_CAPACITY."""
    pos = np.asarray(pos, F).reshape(-1, 3)
    n = len(pos)
    mid = np.asarray(mesh_id, np.uint32).reshape(-1).astype(np.int64)
    base, n_buckets = lr.lod_bases(meshes)
    d = depth_key(pos, cam_pos, order)
    if order != DRAW_INDEX and n_buckets > MAX_BUCKETS:
        raise OverflowError("more than 65 536 buckets")
    # commands, counts, members, LODs: mip_batch_draws_lods's, whatever the order
    res = lr.batch_draws_lods(pos, scale, mesh_id, meshes, cam_pos, visible_bitmap, mode, switch_sq, first_instance_base=first_instance_base)
    lod = res["lod"]
    length = meshes["index_len"][mid, lod] if n else np.zeros(0, np.uint32)
    inst = np.nonzero(bitmap_bits(visible_bitmap, n) & (length > 0))[0]
    bucket = base[mid[inst]] + lod[inst]
    slots = inst[np.lexsort((inst, d[inst], bucket))]   # by bucket, then D, then draw index
    res["order"] = slots
    res["ids"] = ((slots + int(first_instance_base)) & 0xFFFFFFFF).astype(np.uint32)
    res["model"] = None if model is None else np.asarray(model).reshape(-1, 16)[slots]
    return res
