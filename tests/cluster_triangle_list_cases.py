"""Hand-written answers of mip_list_cluster_triangles (include/mi_instance_pipeline.h) for the ten scenes of
tests/cluster_triangle_cases.py (instances at the origin, identity rotation, scale 1, pv = the identity: FRONT survives, BACK is
culled, an OUT cluster never reaches the triangle test — that file derives it), and a DESIGNED geometry whose answer follows by
construction: every cluster of a level is all FRONT, all BACK, OUT or alternating FRONT / BACK, chosen by a character."""
import numpy as np

import cluster_cases as cc
import cluster_triangle_cases as ctc
from renderer_amd.pipeline import CLUSTER_ENTRY_DTYPE, MESH_DTYPE

F = np.float32
FULL = (1 << 64) - 1
EVEN = 0x5555555555555555      # the bits of the FRONT triangles of an alternating cluster: triangle 0 is FRONT
ODD = 0xAAAAAAAAAAAAAAAA


def _want(rows, masks, stats):
    return dict(entries=np.array(rows, CLUSTER_ENTRY_DTYPE) if rows else np.zeros(0, CLUSTER_ENTRY_DTYPE), masks=np.array(masks, np.uint64),
                stats=np.array(stats, np.uint32))


def answers():
    """{scene name of cluster_triangle_cases.cases(): dict(entries — (instance, first_index, vertex_offset, index_count) rows,
    masks, stats — entries, surviving clusters, W, members, surviving triangles, triangles tested)}, written by hand."""
    a = {}
    # one cluster of t FRONT triangles, base 7: one entry, the low t bits
    for t in (1, 63, 64):
        a[f"a cluster of {t}"] = _want([(7, 0, 0, 3 * t)], [(1 << t) - 1], (1, 1, 1, 1, t, t))
    # T = 69 FRONT: clusters of 64 and 5, base 2^32 - 1 + 0
    a["short last cluster"] = _want([(0xFFFFFFFF, 0, 0, 192), (0xFFFFFFFF, 192, 0, 15)], [FULL, 0x1F], (2, 2, 2, 1, 69, 69))
    # T = 70 BACK: both clusters survive their boxes, no triangle survives: NO entry (the command form keeps an empty command)
    a["an empty run"] = _want([], [], (0, 2, 2, 1, 0, 70))
    # FRONT, BACK, FRONT, ...: the even triangles
    a["alternating"] = _want([(0, 0, 0, 192)], [EVEN], (1, 1, 1, 1, 32, 64))
    # FRONT | BACK | FRONT, base 1: three surviving clusters, the middle one has no entry — the entries skip first_index 192
    a["back-facing cluster inside a run"] = _want([(1, 0, 0, 192), (1, 384, 0, 192)], [FULL, FULL], (2, 3, 3, 1, 128, 192))
    # FRONT | OUT | FRONT: the middle cluster does not survive, so it is not tested either
    a["a culled cluster splits the run"] = _want([(1, 0, 0, 192), (1, 384, 0, 192)], [FULL, FULL], (2, 2, 3, 1, 128, 128))
    # instance 0 draws 64 BACK (mesh 0), instance 1 draws 64 FRONT (mesh 1, whose level starts at index 192), base 5
    a["two instances, the first empty"] = _want([(6, 192, 0, 192)], [FULL], (1, 2, 2, 2, 64, 128))
    # det = 0 survives, +TINY is culled, -TINY survives: triangles 0 and 2 of 3
    a["det == 0"] = _want([(0, 0, 0, 9)], [0b101], (1, 1, 1, 1, 2, 3))
    # every clip coordinate is NaN: nothing is culled, all 64 BACK triangles survive; base 2
    a["a non-finite instance"] = _want([(2, 0, 0, 192)], [FULL], (1, 1, 1, 1, 64, 64))
    # the NaN triangle survives, BACK is culled, FRONT survives
    a["a NaN vertex"] = _want([(0, 0, 0, 9)], [0b101], (1, 1, 1, 1, 2, 3))
    return a


KINDS = "FBOA"   # all FRONT, all BACK, OUT (the cluster is outside the frustum), alternating FRONT / BACK from triangle 0


def designed_scene(levels, instance_pattern, base=0, triangles=None, bits=None, mirror=False):
    """levels[k]: the kinds of mesh k's clusters, one character of KINDS each; triangles[k]: the level's triangle count (default
    64 per cluster; fewer makes the last cluster short, and 1 with a one-character level makes a one-triangle cluster);
    instance i draws mesh instance_pattern[i] at the origin; bits: which instances are members (default all). mirror: the
    answer under cluster_triangle_cases.PV_MIRROR, where BACK survives and FRONT is culled. Returns (scene, want): want =
    dict(entries, masks, stats, listed — mip_list_clusters' list for the same arguments), by construction."""
    levels = [np.frombuffer(l.encode(), np.uint8) if isinstance(l, str) else np.asarray(l, np.uint8) for l in levels]
    triangles = [64 * len(l) for l in levels] if triangles is None else list(triangles)
    code_of = np.zeros(256, np.int64)
    for k, ch in enumerate(KINDS):
        code_of[ord(ch)] = k
    triple = np.array([ctc.FRONT, ctc.BACK, cc.OUT], np.uint32)
    meshes = np.zeros(len(levels), MESH_DTYPE)
    chunks, offset = [], 0
    t_first, t_count, t_alive, t_mask, mesh_base, mesh_c = [], [], [], [], [], []
    for k, (l, tris) in enumerate(zip(levels, triangles)):
        c = len(l)
        assert c == (tris + 63) // 64, "a kind per cluster"
        kind = code_of[l]
        tri_kind = kind[np.arange(tris) // 64]
        tri_kind = np.where(tri_kind == 3, np.arange(tris) % 64 % 2, tri_kind)       # alternating: FRONT, BACK, ...
        ix = triple[tri_kind].reshape(-1)
        meshes["aabb_min"][k], meshes["aabb_max"][k] = (0, 0, 0), (1025, 1, 0)
        meshes["n_lods"][k], meshes["index_len"][k, 0], meshes["index_offset"][k, 0] = 1, len(ix), offset
        count = np.minimum(64 * (np.arange(c) + 1), tris) - 64 * np.arange(c)
        full = np.where(count == 64, np.uint64(FULL), (np.uint64(1) << np.minimum(count, 63).astype(np.uint64)) - np.uint64(1))
        front, back = (0, FULL) if mirror else (FULL, 0)
        alt = ODD if mirror else EVEN
        pick = np.array([front, back, 0, alt], np.uint64)[kind]
        mesh_base.append(len(np.concatenate(t_first)) if t_first else 0)
        mesh_c.append(c)
        t_first.append(offset + 192 * np.arange(c))
        t_count.append(count)
        t_alive.append(kind != 2)
        t_mask.append(pick & full)
        chunks.append(ix)
        offset += len(ix)
    inst = np.asarray(instance_pattern, np.int64)
    n = len(inst)
    member = np.array(mesh_c, np.int64)[inst] > 0 if n else np.zeros(0, bool)
    bitmap = np.full((n + 31) // 32, 0xFFFFFFFF, np.uint32)
    if bits is not None:
        bits = np.asarray(bits, bool)
        bitmap = np.zeros((n + 31) // 32, np.uint32)
        np.bitwise_or.at(bitmap, np.nonzero(bits)[0] >> 5, np.uint32(1) << (np.nonzero(bits)[0] & 31).astype(np.uint32))
        member &= bits
    rot = np.zeros((n, 4), F)
    rot[:, 3] = 1.0
    s = dict(n=n, meshes=meshes, vertices=np.array(cc.BASE_VERTICES, F), indices=np.concatenate(chunks) if chunks else np.zeros(0, np.uint32),
             pos=np.zeros((n, 3), F), rot=rot, scale=np.ones(n, F), mesh_id=inst.astype(np.uint32), planes=cc.PLANES, cam_pos=cc.CAM, base=base, bitmap=bitmap)
    # the work items: every cluster of every member, in (i, c) order
    who = np.nonzero(member)[0]
    sizes = np.array(mesh_c, np.int64)[inst[who]]
    w = int(sizes.sum())
    item_inst = np.repeat(who, sizes)
    item_c = np.arange(w) - np.repeat(np.cumsum(sizes) - sizes, sizes)
    flat = np.array(mesh_base, np.int64)[inst[item_inst]] + item_c if w else np.zeros(0, np.int64)
    first, count = np.concatenate(t_first)[flat], np.concatenate(t_count)[flat]
    alive, mask = np.concatenate(t_alive)[flat], np.concatenate(t_mask)[flat]

    def rows(sel):
        e = np.zeros(int(sel.sum()), CLUSTER_ENTRY_DTYPE)
        e["instance"] = ((item_inst[sel] + int(base)) & 0xFFFFFFFF).astype(np.uint32)
        e["first_index"], e["vertex_offset"], e["index_count"] = first[sel], 0, 3 * count[sel]
        return e

    keeps = alive & (mask != 0)
    kept = int(np.unpackbits(np.ascontiguousarray(mask[alive]).view(np.uint8)).sum())
    stats = np.array([int(keeps.sum()), int(alive.sum()), w, len(who), kept & 0xFFFFFFFF, int(count[alive].sum()) & 0xFFFFFFFF], np.uint32)
    return s, dict(entries=rows(keeps), masks=np.ascontiguousarray(mask[keeps]), stats=stats, listed=rows(alive))
