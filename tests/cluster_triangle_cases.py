"""Hand-written scenes for mip_cull_cluster_triangles (include/mi_instance_pipeline.h) with hand-written answers, on the
geometry of tests/cluster_cases.py: instances at the origin, identity rotation, scale 1, the box frustum |x|, |y|, |z| <= 8.

pv is the IDENTITY, so clip = (x, y, z, 1) of the vertex exactly (every product is with 0 or 1) and the determinant of the xyw
columns of corners a, b, c is  ax (by - cy) - bx (ay - cy) + cx (ay - by): twice the signed area in the xy plane, exact for
the small integers used here. The test culls det > 0:
  BACK  (0,0) (1,0) (0,1), vertices 0 1 2:  0 (0 - 1) - 1 (0 - 1) + 0 = +1 > 0: culled.
  FRONT (0,0) (0,1) (1,0), vertices 0 2 1:  0 (1 - 0) - 0 (0 - 0) + 1 (0 - 1) = -1: survives; every corner has |x|, |y| <= 1 = w,
        so no NDC bound rejects it.
  OUT   the triangle at x + 1024, vertices 3 4 5: its CLUSTER is outside the frustum and never reaches the triangle test.
"""
import numpy as np

import cluster_cases as cc
from renderer_amd.pipeline import DRAW_CMD_DTYPE

F = np.float32
PV = np.eye(4, dtype=F).reshape(16)
PV_MIRROR = np.diag(np.array([-1, 1, 1, 1], F)).reshape(16)   # x -> -x: the determinant changes sign, BACK survives and FRONT is culled
FRONT, BACK, OUT = (0, 2, 1), (0, 1, 2), cc.OUT
TINY = float(np.nextafter(F(0), F(1)))                         # the smallest positive float32 (a subnormal)


def _tris(*spec):
    """The indices of a level from (triple, count) pairs, in order."""
    ix = []
    for triple, count in spec:
        ix += list(triple) * count
    return ix


def _want(rows, stats, stream):
    return dict(cmds=np.array(rows, DRAW_CMD_DTYPE) if rows else np.zeros(0, DRAW_CMD_DTYPE), stats=np.array(stats, np.uint32),
                stream=np.array(stream, np.uint32))


def cases():
    """[(name, scene, want)]: want = dict(cmds — every command, in order; stats — heads, surviving clusters, W, members, surviving
    triangles, triangles tested; stream — every index written, in order). The scenes' pv is PV."""
    at0 = (0, (0, 0, 0), 1.0)
    out = []

    # clusters of 1, 63 and 64 triangles, all FRONT: the whole level, 3 T indices from word 0
    for t in (1, 63, 64):
        s = cc._scene([_tris((FRONT, t))], [at0], base=7)
        out.append((f"a cluster of {t}", s, _want([(3 * t, 1, 0, 0, 7)], (1, 1, 1, 1, t, t), FRONT * t)))

    # a short last cluster: T = 64 + 5, two clusters, one run, one command
    s = cc._scene([_tris((FRONT, 69))], [at0], base=0xFFFFFFFF)                      # the base wraps: firstInstance = base + 0
    out.append(("short last cluster", s, _want([(207, 1, 0, 0, 0xFFFFFFFF)], (1, 2, 2, 1, 69, 69), FRONT * 69)))

    # all BACK, T = 70: both clusters survive the box test, no triangle does — the run keeps its command, indexCount = 0
    s = cc._scene([_tris((BACK, 70))], [at0], base=3)
    out.append(("an empty run", s, _want([(0, 1, 0, 0, 3)], (1, 2, 2, 1, 0, 70), [])))

    # alternating FRONT, BACK over one cluster: the 32 FRONT ones, densely
    s = cc._scene([_tris(*[(FRONT, 1), (BACK, 1)] * 32)], [at0])
    out.append(("alternating", s, _want([(96, 1, 0, 0, 0)], (1, 1, 1, 1, 32, 64), FRONT * 32)))

    # a BACK cluster between two FRONT ones: all three survive the box test, so ONE run and ONE command, whose stream skips
    # the middle cluster
    s = cc._scene([_tris((FRONT, 64), (BACK, 64), (FRONT, 64))], [at0], base=1)
    out.append(("back-facing cluster inside a run", s, _want([(384, 1, 0, 0, 1)], (1, 3, 3, 1, 128, 192), FRONT * 128)))

    # an OUT cluster between two FRONT ones: two runs; the second's firstIndex = 3 x the 64 triangles in front of it
    s = cc._scene([_tris((FRONT, 64), (OUT, 64), (FRONT, 64))], [at0], base=1)
    out.append(("a culled cluster splits the run", s, _want([(192, 1, 0, 0, 1), (192, 1, 192, 0, 1)], (2, 2, 3, 1, 128, 128), FRONT * 128)))

    # two instances, the first one's only run is empty: the second's firstIndex is 0. Mesh 1's level starts at index 192.
    s = cc._scene([_tris((BACK, 64)), _tris((FRONT, 64))], [(0, (0, 0, 0), 1.0), (1, (0, 0, 0), 1.0)], base=5)
    out.append(("two instances, the first empty", s, _want([(0, 1, 0, 0, 5), (192, 1, 0, 0, 6)], (2, 2, 2, 2, 64, 128), FRONT * 64)))

    # det == 0 and the floats beside it: corners (0,0) (1,0) (1/2, e). det = 0 (0 - e) - 1 (0 - e) + 1/2 (0 - 0) = e exactly
    # (e times 1 and plus 0 are exact, also for the subnormal e). e = 0: NOT > 0, survives. e = +TINY: culled. e = -TINY: survives.
    extra = [(0.5, 0, 0), (0.5, TINY, 0), (0.5, -TINY, 0)]
    s = cc._scene([_tris(((0, 1, 6), 1), ((0, 1, 7), 1), ((0, 1, 8), 1))], [at0], extra_vertices=extra)
    out.append(("det == 0", s, _want([(6, 1, 0, 0, 0)], (1, 1, 1, 1, 2, 3), [0, 1, 6, 0, 1, 8])))

    # a non-finite instance: scale = NaN makes every entry of rows 0..2 a NaN but the translation, and row 3 (0 x NaN) too.
    # The cluster's world box is the fold's start (every corner is NaN): not culled (tests/cluster_cases.py, "NaN cluster").
    # Every clip coordinate is NaN: det > 0 is false and so is every NDC comparison — all 64 BACK triangles survive.
    s = cc._scene([_tris((BACK, 64))], [(0, (0, 0, 0), cc.NAN)], base=2)
    out.append(("a non-finite instance", s, _want([(192, 1, 0, 0, 2)], (1, 1, 1, 1, 64, 64), BACK * 64)))

    # a NaN vertex (the cluster's box ignores it): the triangle that names it has a NaN determinant and a NaN corner in every
    # NDC test — it survives; beside it BACK is culled and FRONT survives as always
    s = cc._scene([_tris(((0, 1, 6), 1), (BACK, 1), (FRONT, 1))], [at0], extra_vertices=[(cc.NAN, cc.NAN, cc.NAN)])
    out.append(("a NaN vertex", s, _want([(6, 1, 0, 0, 0)], (1, 1, 1, 1, 2, 3), [0, 1, 6, 0, 2, 1])))
    return out


def ladder_want(s, want):
    """What mip_cull_cluster_triangles owes for a scene of cluster_cases.ladder_scene under PV_MIRROR, from mip_cull_clusters'
    answer `want`: every triangle of a surviving cluster is the inside triangle 0 1 2, which survives mirrored — so a command
    keeps its indexCount, its firstIndex becomes the indices of the runs in front, and the stream is 0 1 2 per triangle."""
    cmds = want["cmds"].copy()
    count = cmds["indexCount"].astype(np.int64)
    cmds["firstIndex"] = ((np.cumsum(count) - count) & 0xFFFFFFFF).astype(np.uint32)
    kept = int(count.sum()) // 3
    return dict(cmds=cmds, stats=np.concatenate([want["stats"], np.array([kept, kept], np.uint32)]),
                stream=np.tile(np.array(cc.IN, np.uint32), kept))
