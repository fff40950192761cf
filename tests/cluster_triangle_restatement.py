"""numpy restatement of mip_cull_cluster_triangles (include/mi_instance_pipeline.h), written from the header's text: members,
work items, SURVIVES and heads through tests/cluster_restatement.py, TRI_SURVIVES through numpy_restatement.triangle_culled
under numpy_restatement.model_matrices (the sixteen floats mip_run writes), the index stream, the commands into it, the six
stats and the three overflow rules. Not reference behaviour: this file is what the library is checked against."""
import numpy as np

import cluster_restatement as cr
import numpy_restatement as nr
from renderer_amd.pipeline import DRAW_CMD_DTYPE

F = np.float32
ERR_CAPACITY = cr.ERR_CAPACITY
STATS = 6


def item_triangles(items):
    """Triangles of every work item's cluster: 64, or what the level has left in its last one."""
    t = items["table"]
    tris = t["T"][items["bucket"][items["inst"]]] if len(items["inst"]) else np.zeros(0, np.int64)
    return np.minimum(cr.CLUSTER_TRIANGLES * (items["cluster"] + 1), tris) - cr.CLUSTER_TRIANGLES * items["cluster"]


def surviving_triangles(s, items, survive, vertices, indices, pv):
    """TRI_SURVIVES over every surviving item, in (i, c, t) order: (kept — surviving triangles per work item, 0 for an item that
    does not survive; stream — the source index triples of the surviving triangles, flat)."""
    vertices = np.asarray(vertices, F).reshape(-1, 3)
    indices = np.asarray(indices, np.uint32).reshape(-1)
    t = items["table"]
    kept = np.zeros(items["W"], np.int64)
    chunks = []
    alive = np.nonzero(survive)[0]
    inst = items["inst"][alive]
    pos, rot, scale = np.asarray(s["pos"], F).reshape(-1, 3), np.asarray(s["rot"], F).reshape(-1, 4), np.asarray(s["scale"], F).reshape(-1)
    for i in np.unique(inst):                                   # (ascending: the work items are in instance order)
        own = alive[inst == i]
        b = int(items["bucket"][i])
        k, l, tris = int(t["mesh"][b]), int(t["lod"][b]), int(t["T"][b])
        off = int(s["meshes"]["index_offset"][k, l])
        model = nr.model_matrices(pos[i : i + 1], rot[i : i + 1], scale[i : i + 1])[0]
        first = cr.CLUSTER_TRIANGLES * items["cluster"][own]
        count = np.minimum(first + cr.CLUSTER_TRIANGLES, tris) - first
        which = np.concatenate([np.arange(f, f + c) for f, c in zip(first, count)])
        ix = indices[off : off + 3 * tris].reshape(tris, 3)[which]
        v = vertices[ix.astype(np.int64) + int(s["meshes"]["vertex_offset"][k])]
        keep = ~nr.triangle_culled(model, pv, v)
        kept[own] = np.add.reduceat(keep.astype(np.int64), np.cumsum(count) - count)
        chunks.append(ix[keep].reshape(-1))
    return kept, (np.concatenate(chunks).astype(np.uint32) if chunks else np.zeros(0, np.uint32))


def cull_cluster_triangles(s, boxes, vertices, indices, visible_bitmap, mode, switch_sq, pv, cmd_capacity, index_capacity, work_capacity=0,
                           first_instance_base=0, occlusion=None):
    """What mip_cull_cluster_triangles owes for scene s: dict(status, cmds — the entries written, count — cmd_count, stats — the
    six words, stream — the indices written, and all_cmds / full_stream / kept / items / survive / head for the tests)."""
    c = cr.cull_clusters(s, boxes, visible_bitmap, mode, switch_sq, cmd_capacity=1 << 62, work_capacity=work_capacity,
                         first_instance_base=first_instance_base, occlusion=occlusion)
    none = np.zeros(0, DRAW_CMD_DTYPE)
    empty = np.zeros(0, np.uint32)
    if c["survive"] is None or len(np.asarray(s["mesh_id"]).reshape(-1)) == 0:      # a work overflow, or N = 0
        return dict(status=c["status"], cmds=none, count=0, stats=np.concatenate([c["stats"], np.zeros(2, np.uint32)]), stream=empty,
                    all_cmds=none, full_stream=empty, kept=None, items=c["items"], survive=c["survive"], head=c["head"])
    items, sv, head = c["items"], c["survive"], c["head"]
    kept, stream = surviving_triangles(s, items, sv, vertices, indices, pv)
    tested = int(item_triangles(items)[sv].sum())
    prefix = np.cumsum(kept) - kept
    cmds = c["all_cmds"].copy()                                 # one per head, in (i, c) order: vertexOffset and firstInstance stay
    heads = np.nonzero(head)[0]
    run_of = np.cumsum(head) - 1                                # the run a surviving item belongs to
    per_run = np.bincount(run_of[sv], weights=kept[sv], minlength=len(heads)).astype(np.int64) if len(heads) else np.zeros(0, np.int64)
    cmds["indexCount"] = (3 * per_run) & 0xFFFFFFFF
    cmds["firstIndex"] = (3 * prefix[heads]) & 0xFFFFFFFF
    total = int(kept.sum())
    stats = np.array([len(heads), int(sv.sum()), items["W"], items["members"], total & 0xFFFFFFFF, tested & 0xFFFFFFFF], np.uint32)
    common = dict(stats=stats, all_cmds=cmds, full_stream=stream, kept=kept, items=items, survive=sv, head=head)
    if 3 * total > int(index_capacity) or 3 * total >= 1 << 32:  # the index overflow: the true stats, nothing else
        return dict(status=ERR_CAPACITY, cmds=none, count=0, stream=empty, **common)
    count = min(len(heads), int(cmd_capacity))
    return dict(status=ERR_CAPACITY if len(heads) > int(cmd_capacity) else 0, cmds=cmds[:count], count=count, stream=stream, **common)
