"""numpy restatement of cluster culling for several views in one call (include/mi_instance_pipeline.h,
mip_cull_clusters_views), written from the header's text: ONE level for all views (frames[0].cam_pos), members from the union
of the views' bitmaps, the work items and their world boxes once, SURVIVES_v = the view's bit AND the plane test against the
view's planes, heads and commands per view by cluster_restatement's rules, the per-view counts, the stats and both overflow
rules. Not reference behaviour: this file is what the library is checked against."""
import numpy as np

import cluster_restatement as cr
import numpy_restatement as nr
from batch_restatement import bitmap_bits
from renderer_amd.pipeline import DRAW_CMD_DTYPE

F = np.float32
ERR_CAPACITY = cr.ERR_CAPACITY


def view_bits(bitmaps, n):
    """(n_views, n) bool: bit i of view v; a None entry counts as set for every resident instance."""
    return np.array([np.ones(n, bool) if b is None else bitmap_bits(b, n) for b in bitmaps], bool).reshape(len(bitmaps), n)


def union_bitmap(bits):
    """The bitmap words of the union of the views' bits."""
    n = bits.shape[1]
    member = bits.any(axis=0)
    words = np.zeros((n + 31) // 32, np.uint32)
    who = np.nonzero(member)[0]
    np.bitwise_or.at(words, who >> 5, np.uint32(1) << (who & 31).astype(np.uint32))
    return words


def cull_clusters_views(s, boxes, view_planes, bitmaps, bases, mode, switch_sq, cmd_stride, work_capacity=0, cam_pos=None):
    """What mip_cull_clusters_views owes for scene s (pos, rot, scale, mesh_id, meshes) under view v = (view_planes[v], bitmaps[v]
    — words or None —, bases[v]); cam_pos = frames[0].cam_pos (default: the scene's). dict(status; cmds — per view the entries
    written; counts — cmd_counts; stats — the 2 + 2 n_views words; heads, survivors per view; items; survive — per view)."""
    n_views = len(view_planes)
    assert len(bitmaps) == n_views == len(bases) and 1 <= n_views <= 16
    n = len(np.asarray(s["mesh_id"]).reshape(-1))
    cam = s["cam_pos"] if cam_pos is None else cam_pos
    empty = np.zeros(0, DRAW_CMD_DTYPE)
    if n == 0:
        return dict(status=0, cmds=[empty] * n_views, counts=np.zeros(n_views, np.uint32), stats=np.zeros(2 + 2 * n_views, np.uint32),
                    heads=[0] * n_views, survivors=[0] * n_views, items=None, survive=None, all_cmds=[empty] * n_views)
    bits = view_bits(bitmaps, n)
    items = cr.work_items(s["pos"], s["scale"], s["mesh_id"], s["meshes"], cam, union_bitmap(bits), mode, switch_sq)
    largest = int(items["table"]["C"].max()) if len(items["table"]["C"]) else 0
    bound = int(work_capacity) if work_capacity else n * largest
    stats = np.zeros(2 + 2 * n_views, np.uint32)
    stats[0], stats[1] = items["W"] & 0xFFFFFFFF, items["members"]
    if items["W"] > bound or items["W"] >= 1 << 32:
        return dict(status=ERR_CAPACITY, cmds=[empty] * n_views, counts=np.zeros(n_views, np.uint32), stats=stats, heads=[0] * n_views,
                    survivors=[0] * n_views, items=items, survive=None, all_cmds=[empty] * n_views)
    status, cmds, all_cmds, counts, heads, survivors, survive = 0, [], [], np.zeros(n_views, np.uint32), [], [], []
    # the world box of a work item is the same numbers for every view: the chain of cluster_restatement.survives, once
    i = items["inst"]
    if len(i):
        model = nr.model_matrices(np.asarray(s["pos"], F).reshape(-1, 3)[i], np.asarray(s["rot"], F).reshape(-1, 4)[i], np.asarray(s["scale"], F).reshape(-1)[i])
        box = np.asarray(boxes, F).reshape(-1, 6)[items["box_index"]]
        mins, maxs = nr.world_aabbs(model, box[:, :3], box[:, 3:])
    for v in range(n_views):
        sv = (~nr.coarse_culled(mins, maxs, view_planes[v]) if len(i) else np.zeros(0, bool)) & bits[v][i]
        c, _ = cr.commands(items, sv, s["meshes"], bases[v])
        count = min(len(c), int(cmd_stride))
        if len(c) > int(cmd_stride):
            status = ERR_CAPACITY
        counts[v] = count
        stats[2 + 2 * v], stats[3 + 2 * v] = len(c), int(sv.sum())
        cmds.append(c[:count])
        all_cmds.append(c)
        heads.append(len(c))
        survivors.append(int(sv.sum()))
        survive.append(sv)
    return dict(status=status, cmds=cmds, counts=counts, stats=stats, heads=heads, survivors=survivors, items=items, survive=survive,
                all_cmds=all_cmds)


def fill_outputs(want, n_views, cmd_stride, sentinel, pad, stats=True):
    """The whole output buffers a call leaves behind when every word was `sentinel` before: dict(cmds — (n_views x cmd_stride +
    pad, 5) uint32, counts — n_views + pad words, stats — 2 + 2 n_views + pad words)."""
    cmds = np.full((n_views * int(cmd_stride) + pad, 5), sentinel, np.uint32)
    for v in range(n_views):
        c = want["cmds"][v]
        if len(c):
            cmds[v * int(cmd_stride): v * int(cmd_stride) + len(c)] = np.ascontiguousarray(c).view(np.uint32).reshape(-1, 5)
    counts = np.full(n_views + pad, sentinel, np.uint32)
    counts[:n_views] = want["counts"]
    st = np.full(2 + 2 * n_views + pad, sentinel, np.uint32)
    if stats:
        st[: 2 + 2 * n_views] = want["stats"]
    return dict(cmds=cmds, counts=counts, stats=st)
