"""Scenes built ON the decision edges of cluster culling (include/mi_instance_pipeline.h, mip_cull_clusters): no GPU, no torch.
tests/test_cluster_edge_cases.py proves what is claimed here, tests/test_gpu_cluster_edges.py runs the scenes on the device.

TIGHT GEOMETRY: tight_geometry() turns a mesh table into (table, vertices, indices) whose every cluster box is a CHOSEN box:
every triangle of a cluster is (min corner, max corner, a third corner of the box), so a short last cluster of one triangle
still spans it. vertex_offset is positive and every index range is real.

TRANSFER SCENES: where every cluster box of a mesh is the mesh box, a cluster's world box is the instance's world box, float for
float — a cluster survives exactly when the instance-level test calls the instance visible (and not occluded). The expected
command list is then written down from the instance-level decision (decision_cases.decide, lod_cases.want_edge_lods,
occlusion_restatement.occluded) WITHOUT cluster_restatement: one command (3 T, 1, index_offset[mesh, lod], vertex_offset,
base + i) per member that is visible. The decision catalogue, the six-level chain and the occlusion catalogue are transferred
whole; the nested mesh (the unit box, its half and its double) ties head detection to a frustum edge.

BOX-SOURCED TIER EDGES are new: the arithmetic tier of a work item hangs on the cluster's box, that is on the vertices. The
odd cluster's box is found by bisection on float bits so that an ordinary instance sits on kSeparableLimit / kFiniteLimit, or
holds +-inf, NaN or +-FLT_MAX; expected bytes are cluster_restatement's (the literal chain).

What cannot be built: a cluster box with min > max on an axis out of finite vertices (the fold orders them); a box whose zero
has a chosen sign where vertices hold zeros of both signs (fminf / fmaxf leave it open — the CPU test shows that the decision
is the same for either)."""
import functools

import numpy as np

import decision_cases as dc
import lod_cases as lc
import numpy_restatement as nr
import occlusion_cases as oc
import occlusion_restatement as orr
from renderer_amd.pipeline import DRAW_CMD_DTYPE, MESH_DTYPE

F = np.float32
INF = float("inf")
NAN = float("nan")
FLT_MAX = F(3.4028234663852886e38)
PIN = (100.00000762939453125, INF, INF, INF, INF)   # the pin policy of tests/cluster_cases.py
CLUSTER = 64
UNIT = (-0.5, -0.5, -0.5, 0.5, 0.5, 0.5)


# ---- tight geometry ----

def diagonal(box):
    """The triangle (min corner, max corner, a third corner) of a box (min xyz, max xyz): (3, 3) float32."""
    b = np.asarray(box, F).reshape(6)
    return np.array([b[:3], b[3:], (b[3], b[1], b[2])], F)


def level(boxes, last=CLUSTER, tail=0):
    """One level: a cluster per entry of `boxes` — a box (6 numbers) or the three vertices of its triangle — of 64 triangles,
    the last one of `last`; `tail` more indices that belong to no triangle."""
    assert 1 <= last <= CLUSTER and 0 <= tail < 3 and len(boxes)
    return dict(triangles=[diagonal(b) if np.size(b) == 6 else np.asarray(b, F).reshape(3, 3) for b in boxes], last=int(last), tail=int(tail))


def tight_geometry(table, levels):
    """table: MESH_DTYPE rows whose aabb and n_lods are kept; levels[k][l]: level(...) or None (an empty level) for l < n_lods.
    Returns (table, vertices, indices, want): index_len / index_offset / vertex_offset rewritten, and want (clusters, 6) — the
    box every cluster was built to have, bucket-major as mip_build_clusters numbers them. Vertex 0 belongs to nobody, so every
    vertex_offset is positive; a mesh's indices count from its own first vertex."""
    table = np.array(table, MESH_DTYPE, copy=True)
    table["index_len"], table["index_offset"], table["vertex_offset"] = 0, 0, 0
    vertices, indices, want = [np.full((1, 3), 1.0e30, F)], [], []
    n_vertices, n_indices = 1, 0
    for k in range(len(table)):
        assert len(levels[k]) == int(table["n_lods"][k])
        table["vertex_offset"][k] = n_vertices
        local = 0
        for l, lv in enumerate(levels[k]):
            table["index_offset"][k, l] = n_indices
            if lv is None:
                continue
            ix = []
            for j, tri in enumerate(lv["triangles"]):
                count = lv["last"] if j == len(lv["triangles"]) - 1 else CLUSTER
                ix += [local, local + 1, local + 2] * count
                vertices.append(tri)
                with np.errstate(all="ignore"):
                    want.append(np.concatenate([np.fmin.reduce(np.concatenate([np.full((1, 3), np.inf, F), tri]), axis=0),
                                                np.fmax.reduce(np.concatenate([np.full((1, 3), -np.inf, F), tri]), axis=0)]))
                local += 3
            ix += [0] * lv["tail"]
            table["index_len"][k, l] = len(ix)
            indices += ix
            n_indices += len(ix)
        n_vertices += local
    return table, np.concatenate(vertices).astype(F), np.array(indices, np.uint32), np.array(want, F).reshape(-1, 6)


def level_sizes(table, mesh_id, lod):
    """(T, C) of the level every instance selects."""
    t = table["index_len"][np.asarray(mesh_id, np.int64), np.asarray(lod, np.int64)].astype(np.int64) // 3
    return t, (t + CLUSTER - 1) // CLUSTER


def bits_to_bitmap(bits):
    return orr.bitmap_of(np.asarray(bits, bool)) if len(bits) else np.zeros(0, np.uint32)


def _rows(rows):
    return np.array(rows, DRAW_CMD_DTYPE) if len(rows) else np.zeros(0, DRAW_CMD_DTYPE)


def transfer_commands(table, mesh_id, lod, visible, bits, base=0):
    """The commands and stats mip_cull_clusters owes where every cluster box of a level is the mesh box: for every instance in
    draw order whose bit is set, whose level has a triangle and whose INSTANCE-level decision is `visible`, the whole level in
    one command. dict(cmds, stats — heads, surviving clusters, W, members)."""
    mesh_id, lod = np.asarray(mesh_id, np.int64), np.asarray(lod, np.int64)
    t, c = level_sizes(table, mesh_id, lod)
    member = np.asarray(bits, bool) & (t > 0)
    keep = member & np.asarray(visible, bool)
    rows = [(3 * int(t[i]), 1, int(table["index_offset"][mesh_id[i], lod[i]]), int(table["vertex_offset"][mesh_id[i]]), (int(base) + int(i)) & 0xFFFFFFFF)
            for i in np.nonzero(keep)[0]]
    return dict(cmds=_rows(rows), stats=np.array([int(keep.sum()), int(c[keep].sum()), int(c[member].sum()), int(member.sum())], np.uint32))


def pattern_commands(table, patterns, base=0):
    """One-mesh, one-level scenes whose clusters differ: instance i's clusters survive where patterns[i] holds '1'; one command
    per run of '1's."""
    tris = int(table["index_len"][0, 0]) // 3
    off, vo = int(table["index_offset"][0, 0]), int(table["vertex_offset"][0])
    rows, survivors = [], 0
    for i, p in enumerate(patterns):
        c = 0
        while c < len(p):
            if p[c] != "1":
                c += 1
                continue
            run = 0
            while c + run < len(p) and p[c + run] == "1":
                run += 1
            rows.append((3 * (min(CLUSTER * (c + run), tris) - CLUSTER * c), 1, off + 3 * CLUSTER * c, vo, (int(base) + i) & 0xFFFFFFFF))
            survivors += run
            c += run
    w = sum(len(p) for p in patterns)
    return dict(cmds=_rows(rows), stats=np.array([len(rows), survivors, w, len(patterns)], np.uint32))


# ---- 1. frustum and pin-policy LOD: the decision catalogue, transferred ----

# (clusters, triangles of the last one) of (mesh, lod): LOD 0 and LOD 1 differ, so the LOD ring shows in indexCount, firstIndex
# and in the place of every later command; 1, 2, 3 and 65 clusters; short last clusters. The empty levels of
# decision_cases.MESHES stay empty (mesh 2 LOD 0, mesh 3 LOD 1, mesh 4).
FRUSTUM_LEVELS = {(0, 0): (3, 5), (0, 1): (2, 64), (1, 0): (65, 33), (2, 1): (1, 7), (3, 0): (2, 1)}
FRUSTUM_BASE = 0xFFFFFF00    # wraps inside every scene of more than 256 instances
# Every (case, frame) of decision_cases.RUN_INPUTS, and the views case under its other two frames: in RUN_INPUTS the instance
# whose squared distance is the LOD threshold itself (sq_near_max) draws mesh 4 (both levels empty) or mesh 1 (one level), so
# a wrong LOD comparison would change no command; under view1 it draws mesh 0 and under view3 mesh 2 (LOD 0 empty).
FRUSTUM_INPUTS = dc.RUN_INPUTS + (("views", "view1"), ("views", "view3"))


@functools.lru_cache(maxsize=None)
def frustum_geometry():
    levels = []
    for k in range(len(dc.MESHES)):
        box = np.concatenate([dc.MESHES["aabb_min"][k], dc.MESHES["aabb_max"][k]])
        row = []
        for l in range(int(dc.MESHES["n_lods"][k])):
            assert ((k, l) in FRUSTUM_LEVELS) == (int(dc.MESHES["index_len"][k, l]) > 0)
            row.append(level([box] * FRUSTUM_LEVELS[(k, l)][0], FRUSTUM_LEVELS[(k, l)][1]) if (k, l) in FRUSTUM_LEVELS else None)
        levels.append(row)
    return tight_geometry(dc.MESHES, levels)


def frustum_targets(item_tile):
    """The work-item counts a scene is cut to: one below, at and one above a survive word and the cull kernel's tile."""
    return (63, 64, 65, item_tile - 1, item_tile, item_tile + 1)


def _cut_to(items, src, target):
    """Bits of a layout cut so that the set instances own exactly `target` work items: edge instances keep their bit before
    ordinary ones, earlier instances before later ones, as long as the rest can still make up the sum (a subset sum, its
    reachable totals kept as the bits of an integer). Instances without a work item keep their bit. None if it cannot be done."""
    order = [i for i in range(len(items)) if src[i] >= 0 and items[i]] + [i for i in range(len(items)) if src[i] < 0 and items[i]]
    mask = (1 << (target + 1)) - 1
    behind = [1] * (len(order) + 1)              # behind[k]: the sums the instances order[k:] can make
    for k in range(len(order) - 1, -1, -1):
        behind[k] = (behind[k + 1] | (behind[k + 1] << int(items[order[k]]))) & mask
    if not (behind[0] >> target) & 1:
        return None
    bits = np.asarray(items) == 0
    gap = target
    for k, i in enumerate(order):
        c = int(items[i])
        if c <= gap and (behind[k + 1] >> (gap - c)) & 1:
            bits[i] = True
            gap -= c
    assert gap == 0
    return bits


@functools.lru_cache(maxsize=None)
def frustum_scenes(name, frame, item_tile):
    """[(what, scene, bits, src)] of one (case, frame): the smallest size of decision_cases.SIZES whose layout can be cut to each
    of frustum_targets(), and 513 whole (every bit set)."""
    table = frustum_geometry()[0]
    out = []
    for target in frustum_targets(item_tile) + (None,):
        for n in (dc.SIZES if target is not None else (513,)):
            s, src = dc.layout(name, n, frame)
            s = dict(s, meshes=table)
            items = level_sizes(table, s["mesh_id"], dc.decide(s)["lod"])[1]
            bits = np.ones(n, bool) if target is None else _cut_to(items, src, target) if int(items.sum()) >= target else None
            if bits is not None:
                out.append((f"{name}/{frame} n={n} W={target or 'whole'}", s, bits, src))
                break
        else:
            raise AssertionError((name, frame, target, "no size of the catalogue can be cut to this work-item count"))
    return out


def frustum_want(s, bits, mutant=None, base=FRUSTUM_BASE):
    d = dc.decide(s, mutant)
    return transfer_commands(s["meshes"], s["mesh_id"], d["lod"], d["visible"], bits, base)


@functools.lru_cache(maxsize=None)
def light_scene(light):
    """The catalogue's light case whole (every ring of every light), with light `light` as the LOD reference point and planes
    that accept everything: the ring built around that light sits on the pin policy's threshold. No LOD label is left out."""
    s, src = dc.layout("lights", 513)
    return dict(s, meshes=frustum_geometry()[0], planes=np.zeros(24, F), cam_pos=np.asarray(dc.catalogue()["lights"][light], F)), src


@functools.lru_cache(maxsize=None)
def instance_tier_scenes(kind, placement):
    """decision_cases.tier_scene — an instance whose OWN position or scale sits on a tier limit, in a wave of ordinary ones —
    and its twin, over the tight geometry: ((scene, twin), odd instances). No tier label is left out."""
    s, twin, odd = dc.tier_scene(kind, placement)
    table = frustum_geometry()[0]
    return (dict(s, meshes=table), dict(twin, meshes=table)), odd


# ---- 2. split decisions: the nested mesh ----

NESTED_BOXES = (UNIT, tuple(0.5 * v for v in UNIT), tuple(2.0 * v for v in UNIT))   # the unit box, halved, doubled about the centre
SPLIT_CLASSES = {"tie0": "101", "ulp_in": "101", "edge_in": "101", "ulp_out": "001", "edge_out": "001"}
SPLIT_INPUTS = (("axis", "axis"), ("camera", "camera"))


@functools.lru_cache(maxsize=None)
def nested_geometry():
    table = np.zeros(1, MESH_DTYPE)
    table["aabb_min"], table["aabb_max"], table["n_lods"] = UNIT[:3], UNIT[3:], 1
    return tight_geometry(table, [[level(list(NESTED_BOXES), last=10, tail=2)]])   # (two indices behind the last triangle)


@functools.lru_cache(maxsize=None)
def split_scene(name, frame):
    """(scene, labels): the plane-edge instances of a case (built on unit boxes) drawing the nested mesh, in catalogue order —
    three work items each, so the edge items walk over the lanes."""
    c = dc.case(name)
    labels = [l for l in c["labels"] if l.get("frame") == frame and l["cls"] in SPLIT_CLASSES]
    idx = np.array([l["index"] for l in labels], np.int64)
    planes, cam = dc.catalogue()["frames"][frame]
    s = dict(n=len(idx), pos=np.ascontiguousarray(c["pos"][idx]), rot=np.ascontiguousarray(c["rot"][idx]), scale=np.ascontiguousarray(c["scale"][idx]),
             mesh_id=np.zeros(len(idx), np.uint32), meshes=nested_geometry()[0], planes=np.asarray(planes, F).reshape(24), cam_pos=np.asarray(cam, F).reshape(3))
    return s, labels


def box_decisions(s, box):
    """numpy_restatement's instance-level decision of every instance of s for one mesh-space box: True = not culled."""
    model = nr.model_matrices(s["pos"], s["rot"], s["scale"])
    b = np.tile(np.asarray(box, F).reshape(1, 6), (len(s["scale"]), 1))
    mins, maxs = nr.world_aabbs(model, b[:, :3], b[:, 3:])
    return ~nr.coarse_culled(mins, maxs, s["planes"])


def split_patterns(s, mutant=None):
    """'1' / '0' per nested box and instance, from numpy_restatement (a plane mutant: from decision_cases.decide)."""
    cols = []
    for box in NESTED_BOXES:
        if mutant is None:
            cols.append(box_decisions(s, box))
        else:
            m = s["meshes"].copy()
            m["aabb_min"], m["aabb_max"] = box[:3], box[3:]
            cols.append(dc.decide(dict(s, meshes=m), mutant)["visible"])
    return ["".join("1" if col[i] else "0" for col in cols) for i in range(s["n"])]


# ---- 3. the six-level chain ----

CHAIN_SWITCHES = {"SWITCH": lc.SWITCH, "SWITCH_SHORT": lc.SWITCH_SHORT}
CHAIN_BASE = 40


@functools.lru_cache(maxsize=None)
def chain_geometry():
    """lod_cases.edge_table() with tight geometry: level l has l + 1 clusters (the last one short); level 2 of mesh 2 stays empty."""
    t = lc.edge_table()
    levels = []
    for k in range(len(t)):
        box = np.concatenate([t["aabb_min"][k], t["aabb_max"][k]])
        levels.append([None if int(t["index_len"][k, l]) == 0 else level([box] * (l + 1), last=CLUSTER - 9 * l - k) for l in range(int(t["n_lods"][k]))])
    return tight_geometry(t, levels)


@functools.lru_cache(maxsize=None)
def chain_scene(mode):
    s = lc.edge_scene(mode)
    return dict(s, meshes=chain_geometry()[0], planes=np.zeros(24, F))     # all-accepting planes: no margin is > 0


def chain_want(s, mode, short, lod=None):
    lod = lc.want_edge_lods(s, mode, short) if lod is None else lod
    return transfer_commands(s["meshes"], s["mesh_id"], lod, np.ones(s["n"], bool), np.ones(s["n"], bool), CHAIN_BASE)


# ---- 4. Hi-Z: the occlusion catalogue, transferred ----

OCCLUSION_BASE = 123_456


@functools.lru_cache(maxsize=None)
def occlusion_scene(name):
    """(case, scene, vertices, indices, want_boxes): every edge instance's own mesh as tight geometry of its box (1, 2 or 3
    clusters, short last ones), the four filler meshes with two clusters each."""
    c = oc.case(name)
    m = c["meshes"]
    levels = []
    for k in range(len(m)):
        box = np.concatenate([m["aabb_min"][k], m["aabb_max"][k]])
        j = k - oc.N_FILLER_MESHES
        levels.append([level([box] * 2, last=12) if j < 0 else level([box] * (1 + j % 3), last=(CLUSTER, 1, 17, 33)[j % 4])])
    table, vertices, indices, want = tight_geometry(m, levels)
    return c, dict(oc.scene_of(c), meshes=table), vertices, indices, want


def occlusion_want(c, s, mutant=None):
    """A command iff the instance's world box is not occluded (the planes accept everything)."""
    hidden = oc.mutant_occluded(c["boxes"], c["pv"], c["depth"], mutant) if mutant else \
        orr.occluded(c["boxes"], c["pv"], orr.pyramid_levels(c["depth"]), c["width"], c["height"])
    return transfer_commands(s["meshes"], s["mesh_id"], np.zeros(s["n"], np.int64), ~hidden, np.ones(s["n"], bool), OCCLUSION_BASE)


# ---- 5. box-sourced tier edges ----

TIER_POS = np.array([1.0, 2.0, 3.0], F)
TIER_SMALL = F(2.0 ** -20)
TIER_LIMIT_KINDS = ("sep_below", "sep_at", "fin_below", "fin_at")
TIER_NONFINITE_KINDS = ("inf_max", "inf_both", "nan_axis", "flt_max")
TIER_KINDS = TIER_LIMIT_KINDS + TIER_NONFINITE_KINDS
TIER_PLACEMENTS = {"lane0": (64, 192), "lane63": (63, 192), "pair": (61, 192), "ragged": (128, 134)}   # (ordinary items in front, W)
# closed: |x|, |y|, |z| <= 64. open: x >= -64, y >= -64, z <= 64 — the side the odd box lies on under TIER_ROT stays open.
TIER_FRAMES = {"closed": np.array([1, 0, 0, -64, -1, 0, 0, -64, 0, 1, 0, -64, 0, -1, 0, -64, 0, 0, 1, -64, 0, 0, -1, -64], F),
               "open": np.array([-1, 0, 0, -64, 0, -1, 0, -64, 0, 0, 1, -64, -1, 0, 0, -64, 0, -1, 0, -64, 0, 0, 1, -64], F)}
ORDINARY = UNIT
TIER_BASE = 5


def odd_box(h):
    """The odd cluster's box for half-extent parameter h: far off the origin along x, so a bounded frustum culls it whole."""
    h = F(h)
    return np.array([h * F(0.5), -1, -1, h, 1, 1], F)


def box_abs(box):
    """instance_tiered's sum of the magnitudes of the six box coordinates, in its order, float32."""
    b = np.abs(np.asarray(box, F).reshape(6))
    with np.errstate(all="ignore"):
        return ((((b[0] + b[1]) + b[2]) + b[3]) + b[4]) + b[5]


def box_tier(pos, rot, scale, box):
    """(all_finite, separable) of one work item as instance_tiered decides them, mirrored in float32: box_abs is the CLUSTER's."""
    ba = box_abs(box)
    with np.errstate(all="ignore"):
        all_finite = bool((dc.finite_magnitude(pos, rot, scale)[0] + ba) < dc.FINITE_LIMIT)
        separable = all_finite and bool(dc.separable_bound(pos, rot, scale, ba)[0] < dc.SEPARABLE_LIMIT)
    return all_finite, separable


@functools.lru_cache(maxsize=None)
def tier_half_extents():
    """{kind: h}: the neighbouring float32 pair of h where the ordinary instance (TIER_ROT, TIER_POS, scale 1) drawing
    odd_box(h) crosses kSeparableLimit, and kFiniteLimit — found by bisection on the float's bits."""
    sep = lambda h: box_tier(TIER_POS, dc.TIER_ROT, F(1.0), odd_box(h))[1]
    fin = lambda h: box_tier(TIER_POS, dc.TIER_ROT, F(1.0), odd_box(h))[0]
    a, b = dc._bits_bisect(F(1e30), F(1e37), sep)
    c, d = dc._bits_bisect(F(1e37), F(3.3e38), fin)
    return {"sep_below": a, "sep_at": b, "fin_below": c, "fin_at": d}


def odd_triangle(kind):
    """The three vertices of the odd cluster's triangle."""
    if kind in TIER_LIMIT_KINDS:
        return diagonal(odd_box(tier_half_extents()[kind]))
    m = float(FLT_MAX)
    return np.array({"inf_max": [(1, -1, -1), (INF, 1, 1), (2, 1, -1)],           # +inf on one axis's max only
                     "inf_both": [(-INF, -1, -1), (INF, 1, 1), (0, 0, 0)],         # (-inf, +inf) on one axis
                     "nan_axis": [(NAN, -1, -1), (NAN, 1, 1), (NAN, 0, 0)],        # x keeps the fold's start values (+inf, -inf)
                     "flt_max": [(-m, -m, -m), (m, m, m), (0, 0, 0)]}[kind], F)


@functools.lru_cache(maxsize=None)
def tier_geometry(kind, twin=False):
    """mesh 0: one ordinary cluster; mesh 1: three clusters (the last one short) — odd, ordinary, odd; the twin: all ordinary."""
    table = np.zeros(2, MESH_DTYPE)
    table["aabb_min"], table["aabb_max"], table["n_lods"] = UNIT[:3], UNIT[3:], 1
    odd = diagonal(ORDINARY) if twin else odd_triangle(kind)
    return tight_geometry(table, [[level([ORDINARY])], [level([odd, ORDINARY, odd], last=5)]])


@functools.lru_cache(maxsize=None)
def tier_scene(kind, placement, frame):
    """dict(scene, odd_items, odd_instances): `front` ordinary one-cluster instances, the ordinary instance A (scale 1) and its
    copy B of scale 2^-20 — both draw mesh 1, so the odd work items are front, front + 2 | front + 3, front + 5 — and ordinary
    instances up to W work items. The twin scene is the same instances over tier_geometry(kind, twin=True)."""
    front, w = TIER_PLACEMENTS[placement]
    n = w - 4
    rng = np.random.default_rng(1000 * TIER_KINDS.index(kind) + front)
    pos, rot, scale, _ = dc._fillers(rng, n)
    mesh = np.zeros(n, np.uint32)
    for i, sc in ((front, F(1.0)), (front + 1, TIER_SMALL)):
        pos[i], rot[i], scale[i], mesh[i] = TIER_POS, dc.TIER_ROT, sc, 1
    s = dict(n=n, pos=pos, rot=rot, scale=scale, mesh_id=mesh, meshes=tier_geometry(kind)[0], planes=TIER_FRAMES[frame], cam_pos=np.zeros(3, F))
    return dict(scene=s, odd_items=(front, front + 2, front + 3, front + 5), odd_instances=(front, front + 1))


# ---- mip_build_clusters at the edge of its refusals ----

def refusal_geometry():
    """One mesh, one level of 2 triangles over 6 vertices behind vertex_offset 2, and an index tail of 2 that names a vertex far
    outside: dict(table, vertices, indices). vertex_offset + largest used index = 2 + 5 = 7 = n_vertices - 1."""
    table = np.zeros(1, MESH_DTYPE)
    table["aabb_min"], table["aabb_max"], table["n_lods"] = UNIT[:3], UNIT[3:], 1
    table["index_len"][0, 0], table["index_offset"][0, 0], table["vertex_offset"] = 8, 0, 2
    vertices = np.arange(24, dtype=F).reshape(8, 3)
    return dict(table=table, vertices=vertices, indices=np.array([0, 1, 2, 3, 4, 5, 1 << 30, 1 << 30], np.uint32))
