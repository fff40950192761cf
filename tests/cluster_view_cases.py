"""Hand-written scenes for cluster culling of several views in one call (include/mi_instance_pipeline.h,
mip_cull_clusters_views) with hand-written answers, on the LADDER geometry of tests/cluster_cases.py: cluster c of a level is
64 copies of the INSIDE triangle (box [0,1] x [0,1] x [0,0]) or of the OUTSIDE one (the same at x + 1024). Rotation is the
identity, scales are 1 and positions small integers, so every number of the world-box chain is exact.

The views' frusta are exact boxes, six planes each in cluster_cases.PLANES' form (n . centre + d) - extent > 0 <=> outside:
  A  |x| <= 8,        |y| <= 8, |z| <= 8   cluster_cases.PLANES: sees the INSIDE triangle only
  B  |x - 1024| <= 8, |y| <= 8, |z| <= 8   sees the OUTSIDE triangle only
  C  |x| <= 2048,     |y| <= 8, |z| <= 8   sees both
  D  |x + 4096| <= 8, |y| <= 8, |z| <= 8   sees nothing

Also here, so that the CPU and the GPU tests share them without importing each other: the frusta generator of the scene tests
(the scene's own frustum turned about the axes, as tests/test_gpu_batch_views.py turns it) and the per-view bases."""
import numpy as np

import cluster_cases as cc
from renderer_amd.pipeline import DRAW_CMD_DTYPE, MESH_DTYPE

F = np.float32
INF = float("inf")
NAN = float("nan")
DISTANCE = 0   # MIP_LOD_DISTANCE


def _box(x_lo, x_hi):
    p = cc.PLANES.copy().reshape(6, 4)
    p[0, 3], p[1, 3] = -x_hi, x_lo      # (1,0,0,-hi): x - hi > 0 outside; (-1,0,0,lo): lo - x > 0 outside
    return np.ascontiguousarray(p.reshape(-1))


A = cc.PLANES.copy()
B = _box(1016, 1032)
C = _box(-2048, 2048)
D = _box(-4104, -4088)


def bits(n, which):
    """The bitmap words of n instances with the bits of `which` set."""
    words = np.zeros((n + 31) // 32, np.uint32)
    which = np.asarray(which, np.int64).reshape(-1)
    np.bitwise_or.at(words, which >> 5, np.uint32(1) << (which & 31).astype(np.uint32))
    return words


def _rows(rows):
    return np.array(rows, DRAW_CMD_DTYPE) if rows else np.zeros(0, DRAW_CMD_DTYPE)


def _views(planes, bitmaps=None, bases=None, cams=None, switch=cc.PIN):
    k = len(planes)
    return dict(planes=list(planes), bitmaps=list(bitmaps) if bitmaps is not None else [None] * k, bases=list(bases) if bases is not None else [0] * k,
                cams=list(cams) if cams is not None else [cc.CAM.copy() for _ in range(k)], mode=DISTANCE, switch=tuple(switch))


def _two_level_scene():
    """One mesh of two levels: level 0 = two INSIDE clusters (384 indices at 0), level 1 = one (192 indices at 384); one
    instance at the origin."""
    meshes = np.zeros(1, MESH_DTYPE)
    meshes["aabb_min"][0], meshes["aabb_max"][0], meshes["n_lods"][0] = (0, 0, 0), (1025, 1, 0), 2
    meshes["index_len"][0, :2], meshes["index_offset"][0, :2] = (384, 192), (0, 384)
    rot = np.zeros((1, 4), F)
    rot[:, 3] = 1.0
    return dict(n=1, meshes=meshes, vertices=np.array(cc.BASE_VERTICES, F), indices=np.array(list(cc.IN) * (128 + 64), np.uint32),
                pos=np.zeros((1, 3), F), rot=rot, scale=np.ones(1, F), mesh_id=np.zeros(1, np.uint32), planes=cc.PLANES, cam_pos=cc.CAM, base=0,
                bitmap=np.full(1, 0xFFFFFFFF, np.uint32))


def cases():
    """[(name, scene, views, want)]: views = dict(planes, bitmaps — words or None —, bases, cams, mode, switch) per view;
    want = dict(cmds — per view every command in order; stats — W, members, then heads and surviving clusters per view)."""
    out = []

    # one instance of "1010101" (C = 7, T = 448) at the origin under A, B, C, D. A sees clusters 0, 2, 4, 6: four commands of
    # one cluster; B sees 1, 3, 5: three; C sees all seven: ONE command with the level's 3 T = 1 344 indices; D none.
    s = cc._scene([cc._level("1010101", 448)], [(0, (0, 0, 0), 1.0)])
    bases = [7, 100, 0x80000000, 1]
    want = dict(cmds=[_rows([(192, 1, 0, 0, 7), (192, 1, 384, 0, 7), (192, 1, 768, 0, 7), (192, 1, 1152, 0, 7)]),
                      _rows([(192, 1, 192, 0, 100), (192, 1, 576, 0, 100), (192, 1, 960, 0, 100)]),
                      _rows([(1344, 1, 0, 0, 0x80000000)]), _rows([])],
                stats=np.array([7, 1, 4, 4, 3, 3, 1, 7, 0, 0], np.uint32))
    out.append(("four views of one ladder", s, _views([A, B, C, D], bases=bases), want))

    # the same with garbage in the cameras of the views behind the first: frames[v].cam_pos, v > 0, is not read
    cams = [cc.CAM.copy()] + [np.array([NAN, INF, -1e30], F) for _ in range(3)]
    out.append(("garbage cameras behind view 0", s, _views([A, B, C, D], bases=bases, cams=cams), want))

    # two instances of "11" (384 indices), both inside A; bitmaps {0}, {1}, {} and NULL. The view with the empty bitmap has no
    # command; the NULL view draws both (two commands: a run never crosses an instance). View 1's base wraps: 0xFFFFFFFF + 1 = 0.
    s = cc._scene([cc._level("11", 128)], [(0, (0, 0, 0), 1.0), (0, (3, 0, 0), 1.0)])
    want = dict(cmds=[_rows([(384, 1, 0, 0, 9)]), _rows([(384, 1, 0, 0, 0)]), _rows([]), _rows([(384, 1, 0, 0, 20), (384, 1, 0, 0, 21)])],
                stats=np.array([4, 2, 1, 2, 1, 2, 0, 0, 2, 4], np.uint32))
    out.append(("bitmaps {0}, {1}, {}, NULL", s, _views([A, A, A, A], bitmaps=[bits(2, [0]), bits(2, [1]), bits(2, []), None], bases=[9, 0xFFFFFFFF, 5, 20]), want))

    # a third instance with no bit in any view is no member: W = 4 and members = 2, not 6 and 3
    s = cc._scene([cc._level("11", 128)], [(0, (0, 0, 0), 1.0), (0, (3, 0, 0), 1.0), (0, (0, 3, 0), 1.0)])
    want = dict(cmds=[_rows([(384, 1, 0, 0, 9)]), _rows([(384, 1, 0, 0, 0)]), _rows([])], stats=np.array([4, 2, 1, 2, 1, 2, 0, 0], np.uint32))
    out.append(("an instance in no bitmap", s, _views([A, A, A], bitmaps=[bits(3, [0]), bits(3, [1]), bits(3, [])], bases=[9, 0xFFFFFFFF, 5]), want))

    # members 0 and 2 with the non-member between them, under views that see different ladders: "10" at the origin and at
    # (0, 3, 0). A: cluster 0 of both; B: cluster 1 of both; instance 1 (bit nowhere) takes no work item
    s = cc._scene([cc._level("10", 128)], [(0, (0, 0, 0), 1.0), (0, (3, 0, 0), 1.0), (0, (0, 3, 0), 1.0)])
    want = dict(cmds=[_rows([(192, 1, 0, 0, 0), (192, 1, 0, 0, 2)]), _rows([(192, 1, 192, 0, 12)])], stats=np.array([4, 2, 2, 2, 1, 1], np.uint32))
    out.append(("a non-member between two members", s, _views([A, B], bitmaps=[bits(3, [0, 2]), bits(3, [2])], bases=[0, 10]), want))

    # a two-level mesh under a DISTANCE policy with the switch at q = 100: the level comes from frames[0].cam_pos for every
    # view. View 0's camera at the origin (q = 0: level 0), view 1's at z = 100 (q = 10 000: its own camera would pick level 1)
    s = _two_level_scene()
    near, far = np.zeros(3, F), np.array([0, 0, 100], F)
    want = dict(cmds=[_rows([(384, 1, 0, 0, 3)]), _rows([(384, 1, 0, 0, 4)])], stats=np.array([2, 1, 1, 2, 1, 2], np.uint32))
    out.append(("one level for all views: view 0 near", s, _views([A, C], bases=[3, 4], cams=[near, far], switch=(100.0, INF, INF, INF, INF)), want))
    # ... and the other way round: level 1 (one cluster, 192 indices at 384) for both
    want = dict(cmds=[_rows([(192, 1, 384, 0, 3)]), _rows([(192, 1, 384, 0, 4)])], stats=np.array([1, 1, 1, 1, 1, 1], np.uint32))
    out.append(("one level for all views: view 0 far", s, _views([A, C], bases=[3, 4], cams=[far, near], switch=(100.0, INF, INF, INF, INF)), want))
    return out


# ---- ladders under several views, for the structural tests ----

FRUSTUM = {"A": A, "B": B, "C": C, "D": D}


def ladder_views(patterns, instance_pattern, specs):
    """cluster_cases.ladder_scene under several views. specs: per view (frustum — "A" sees the '1' clusters, "B" the '0'
    clusters, "C" every cluster, "D" none —, bits — a bool per instance, or None for a NULL bitmap —, base).
    Returns (scene, views, want): want written down from the patterns — view v's commands are ladder_scene's for the ladders as
    that frustum sees them and that view's bits; W and members are those of the union of the bits."""
    masks = [np.frombuffer(p.encode(), np.uint8) == ord("1") if isinstance(p, str) else np.asarray(p, bool) for p in patterns]
    seen = {"A": masks, "B": [~m for m in masks], "C": [np.ones(len(m), bool) for m in masks], "D": [np.zeros(len(m), bool) for m in masks]}
    inst = np.asarray(instance_pattern, np.int64)
    n = len(inst)
    scene, _ = cc.ladder_scene(masks, inst)
    union = np.zeros(n, bool)
    cmds, stats = [], []
    for kind, b, base in specs:
        b = None if b is None else np.asarray(b, bool)
        _, w = cc.ladder_scene(seen[kind], inst, base=base, bits=b)
        cmds.append(w["cmds"])
        stats += [int(w["stats"][0]), int(w["stats"][1])]
        union |= np.ones(n, bool) if b is None else b
    sizes = np.array([len(m) for m in masks], np.int64)[inst]
    member = union & (sizes > 0)
    views = _views([FRUSTUM[k] for k, _, _ in specs], bitmaps=[None if b is None else bits(n, np.nonzero(np.asarray(b, bool))[0]) for _, b, _ in specs],
                   bases=[base for _, _, base in specs])
    return scene, views, dict(cmds=cmds, stats=np.array([int(sizes[member].sum()), int(member.sum())] + stats, np.uint32))


# ---- the scene tests' views ----

def frusta(planes, n_views):
    """A frustum per view: the scene's own, and the same one turned about the axes (columns swapped, signs flipped) — the
    turns tests/test_gpu_batch_views.py uses."""
    base = np.asarray(planes, F).reshape(6, 4)
    turns = [(0, 1, 2, 1, 1), (2, 1, 0, 1, 1), (0, 1, 2, -1, 1), (2, 1, 0, -1, 1), (0, 2, 1, 1, 1), (0, 1, 2, 1, -1)]
    out = []
    for v in range(n_views):
        a, b, c, sx, sz = turns[v % len(turns)]
        t = base[:, [a, b, c, 3]].copy()
        t[:, 0] *= sx
        t[:, 2] *= sz
        out.append(np.ascontiguousarray(t.reshape(-1)))
    return out


def metric_thresholds(s, mode, levels=6):
    """Five thresholds at the quantiles of the policy's metric over the scene's instances (from the scene's camera): every
    level gets a sixth of them. mode 0 = DISTANCE, 1 = RELATIVE."""
    d = np.asarray(s["cam_pos"], np.float64)[None, :] - s["pos"].astype(np.float64)
    q = (d * d).sum(axis=1)
    if mode == 1:
        e = (s["meshes"]["aabb_max"].astype(np.float64) - s["meshes"]["aabb_min"].astype(np.float64))[s["mesh_id"]]
        q = q / (s["scale"].astype(np.float64) ** 2 * (e * e).sum(axis=1))
    q = np.sort(q)
    if len(q) < levels:
        return (1.0, 2.0, 3.0, 4.0, 5.0) if mode == 0 else (0.1, 0.2, 0.3, 0.4, 0.5)
    return tuple(float(F(v)) for v in np.maximum.accumulate([q[len(q) * k // levels] for k in range(1, levels)]))


def view_cams(s, n_views):
    """frames[v].cam_pos: the scene's for view 0 (the one that is read), somewhere else for the others."""
    rng = np.random.default_rng(n_views)
    return [(np.asarray(s["cam_pos"], F) + (rng.normal(0, 15, 3) if v else 0)).astype(F) for v in range(n_views)]


def view_bases(n_views, n=0):
    """A first_instance_base per view; from view 2 on base + i wraps inside a scene of a few thousand instances. Given the
    scene's n >= 2, the last view's base is 2^32 - n // 2 as well: base + i wraps in the middle of THIS scene, whatever its
    size and however few views the call has."""
    out = [(0x40000000 * v + 1000 * v + 7) & 0xFFFFFFFF if v < 2 else (0xFFFFFFFF - 100 * v) & 0xFFFFFFFF for v in range(n_views)]
    if n >= 2:
        out[-1] = (1 << 32) - n // 2
    return out


# (heads, surviving clusters) of the first six turns for config 3 under "strips", full bitmaps, the pin policy: checked on the
# CPU when the call was specified; n = 257 has W = 9 917 and 257 members, n = 1 025 has W = 34 820
KNOWN = {257: dict(W=9917, members=257, views=[(71, 2581), (81, 3425), (71, 2581), (65, 2539), (4, 255), (65, 2127)]),
         1025: dict(W=34820, members=1025, views=[(278, 9072), (282, 9920), (278, 9072), (262, 7640), (53, 1291), (286, 8460)])}
