"""numpy restatement of the batched-draws extension (include/mi_instance_pipeline.h, mip_batch_draws): the members of a
visibility bitmap binned, stably, by bucket = mesh_id * 2 + lod; one instanced command per non-empty bucket; the entity ids and
(given a frame's `model`) the matrices in slot order. Not reference behaviour: this file is what the library is checked against."""
import numpy as np

from renderer_amd.pipeline import DRAW_CMD_DTYPE

F = np.float32


def pick_lods(pos, mesh_id, meshes, cam_pos):
    """pick_lod (helpers.rs:3-11) per instance, as orc_pick_lod evaluates it: every product and sum rounded to float32,
    correctly rounded sqrt, `> 10.0` and more than one LOD."""
    pos = np.asarray(pos, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        d = np.asarray(cam_pos, F).reshape(3)[None, :] - pos
        sq = F(0.0) + ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        far = np.sqrt(sq) > F(10.0)
    return (far & (meshes["n_lods"][mesh_id] > 1)).astype(np.int64)


def bitmap_bits(bitmap, n):
    """The first n bits of a bitmap in MipOutputs.visible_bitmap's layout, as booleans (bits at or above n are ignored)."""
    words = np.ascontiguousarray(bitmap, dtype=np.uint32).reshape(-1)
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)


def batch_draws(pos, mesh_id, meshes, cam_pos, visible_bitmap, first_instance_base=0, model=None):
    """Returns dict(cmds (DRAW_CMD_DTYPE), count, ids (uint32), members, order (instance of every slot), model (or None))."""
    pos = np.asarray(pos, F).reshape(-1, 3)
    n = len(pos)
    mesh_id = np.asarray(mesh_id, np.uint32).reshape(-1).astype(np.int64)
    lod = pick_lods(pos, mesh_id, meshes, cam_pos)
    length = meshes["index_len"][mesh_id, lod] if n else np.zeros(0, np.uint32)
    member = bitmap_bits(visible_bitmap, n) & (length > 0)
    inst = np.nonzero(member)[0]
    bucket = mesh_id[inst] * 2 + lod[inst]
    by_bucket = np.argsort(bucket, kind="stable")          # stable: draw order inside a bucket
    order = inst[by_bucket]
    sorted_buckets = bucket[by_bucket]
    buckets, first_slot, counts = np.unique(sorted_buckets, return_index=True, return_counts=True)
    cmds = np.zeros(len(buckets), DRAW_CMD_DTYPE)
    b_mesh, b_lod = buckets // 2, buckets % 2
    cmds["indexCount"] = meshes["index_len"][b_mesh, b_lod]
    cmds["instanceCount"] = counts
    cmds["firstIndex"] = meshes["index_offset"][b_mesh, b_lod]
    cmds["vertexOffset"] = meshes["vertex_offset"][b_mesh]
    cmds["firstInstance"] = first_slot
    ids = ((order + int(first_instance_base)) & 0xFFFFFFFF).astype(np.uint32)
    return dict(cmds=cmds, count=len(cmds), ids=ids, members=len(order), order=order,
                model=None if model is None else np.asarray(model).reshape(-1, 16)[order])


def expand(batches, first_instance_base=0):
    """The batches as per-instance commands (index_len, 1, index_offset[lod], vertex_offset, id), sorted by id: what a
    mip_run's compacted list holds, except that its firstIndex is the running sum and this one is the source offset."""
    c = batches["cmds"]
    out = np.zeros(batches["members"], DRAW_CMD_DTYPE)
    rep = np.repeat(np.arange(len(c)), c["instanceCount"].astype(np.int64))
    out["indexCount"] = c["indexCount"][rep]
    out["instanceCount"] = 1
    out["firstIndex"] = c["firstIndex"][rep]
    out["vertexOffset"] = c["vertexOffset"][rep]
    out["firstInstance"] = batches["ids"]
    return out[np.argsort(out["firstInstance"].astype(np.int64) - int(first_instance_base) & 0xFFFFFFFF, kind="stable")]
