"""numpy restatement of batched draws for several views in one call (include/mi_instance_pipeline.h, mip_batch_draws_views),
written from the header's text: every (view, instance) pair whose instance is a member of the view under
mip_batch_draws_lods' rule gets the key view * B + bucket; the pairs are sorted, stably, by that key into ONE instance_ids
array; every view's commands are packed into the view's own range of batch_cmds with absolute slots as firstInstance.
Built on lod_restatement for the selection rule and the bucket numbering only: the sort over all views is this file's own,
and tests/test_views_batch_restatement.py holds it against lod_restatement.batch_draws_lods view by view.
Not reference behaviour: this file is what the library is checked against."""
import numpy as np

import lod_restatement as lr
from batch_restatement import bitmap_bits
from renderer_amd.pipeline import DRAW_CMD_DTYPE

MAX_VIEWS = 16


def batch_draws_views(pos, scale, mesh_id, meshes, cams, bitmaps, bases, mode, switch_sq):
    """cams: V x 3; bitmaps: V bitmaps (None = every resident instance); bases: V first_instance_base values.
    Returns dict(cmds (a list of V DRAW_CMD_DTYPE arrays), counts (uint32[V]), first_slot (uint32[V + 1]), ids (uint32, all
    views), members, order (the instance of every slot), view (the view of every slot), lod (V x N))."""
    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    n, n_views = len(pos), len(cams)
    if not 1 <= n_views <= MAX_VIEWS or len(bitmaps) != n_views or len(bases) != n_views:
        raise ValueError("1 <= n_views <= 16, one bitmap and one base per view")
    mesh_id = np.asarray(mesh_id, np.uint32).reshape(-1).astype(np.int64)
    lod_base, n_buckets = lr.lod_bases(meshes)
    keys, insts, lods = [], [], np.zeros((n_views, n), np.int64)
    for v in range(n_views):
        lods[v] = lr.select_lods(pos, scale, mesh_id, meshes, cams[v], mode, switch_sq)
        length = meshes["index_len"][mesh_id, lods[v]] if n else np.zeros(0, np.uint32)
        bits = np.ones(n, bool) if bitmaps[v] is None else bitmap_bits(bitmaps[v], n)
        inst = np.nonzero(bits & (length > 0))[0]
        keys.append(v * n_buckets + lod_base[mesh_id[inst]] + lods[v][inst])
        insts.append(inst)
    key, inst = np.concatenate(keys), np.concatenate(insts)           # view-major, draw order inside a view
    by_key = np.argsort(key, kind="stable")                           # (view, bucket, draw index)
    key, order = key[by_key], inst[by_key]
    view = key // n_buckets if n_buckets else key
    base = np.asarray([int(b) for b in bases], np.int64)
    ids = ((order + base[view]) & 0xFFFFFFFF).astype(np.uint32)
    first_slot = np.searchsorted(view, np.arange(n_views + 1)).astype(np.uint32)   # members of the views before v
    groups, first, counts = np.unique(key, return_index=True, return_counts=True)
    g_view, g_bucket = groups // max(n_buckets, 1), groups % max(n_buckets, 1)
    g_mesh = np.searchsorted(lod_base, g_bucket, side="right") - 1
    g_lod = g_bucket - lod_base[g_mesh]
    cmds = np.zeros(len(groups), DRAW_CMD_DTYPE)
    cmds["indexCount"] = meshes["index_len"][g_mesh, g_lod]
    cmds["instanceCount"] = counts
    cmds["firstIndex"] = meshes["index_offset"][g_mesh, g_lod]
    cmds["vertexOffset"] = meshes["vertex_offset"][g_mesh]
    cmds["firstInstance"] = first                                      # the ABSOLUTE slot
    per_view = [cmds[g_view == v] for v in range(n_views)]
    return dict(cmds=per_view, counts=np.array([len(c) for c in per_view], np.uint32), first_slot=first_slot, ids=ids,
                members=len(order), order=order, view=view, lod=lods, n_buckets=n_buckets)


def min_cmd_stride(meshes, n):
    """The smallest legal cmd_stride: min(B, N)."""
    return min(lr.lod_bases(meshes)[1], n)


def fill_outputs(want, n, cmd_stride, sentinel, pad=3, first_slot=True):
    """The four output buffers as a call leaves them when they held `sentinel` in every word before it: batch_cmds
    (n_views x cmd_stride (+ pad) rows of five words), batch_counts (n_views + pad), instance_ids (n_views x N + pad),
    view_first_slot (n_views + 1 + pad; all sentinel when not asked for)."""
    n_views = len(want["cmds"])
    if cmd_stride < min(want["n_buckets"], n):
        raise ValueError("cmd_stride < min(B, N)")
    cmds = np.full((n_views * cmd_stride + pad, 5), sentinel, np.uint32)
    for v, c in enumerate(want["cmds"]):
        cmds[v * cmd_stride: v * cmd_stride + len(c)] = np.ascontiguousarray(c).view(np.uint32).reshape(-1, 5)
    counts = np.full(n_views + pad, sentinel, np.uint32)
    counts[:n_views] = want["counts"]
    ids = np.full(n_views * n + pad, sentinel, np.uint32)
    ids[: want["members"]] = want["ids"]
    slots = np.full(n_views + 1 + pad, sentinel, np.uint32)
    if first_slot:
        slots[: n_views + 1] = want["first_slot"]
    return dict(cmds=cmds, counts=counts, ids=ids, first_slot=slots)
