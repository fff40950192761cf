"""Hand-written scenes for cluster culling in two phases (include/mi_instance_pipeline.h, mip_cull_clusters_phase) with
hand-written answers: the commands of both phases, their stats and the record, none of them taken from a restatement.

GEOMETRY: the tight geometry of tests/cluster_edge_cases.py — every cluster of a level is 64 copies (the last one fewer) of one
triangle that spans a CHOSEN box. Instances sit at the origin with the identity rotation and scale 1, so a cluster's world box
is its box, exactly. pv is the identity: ndc = the box's coordinates, w = 1. The image is 8 x 8: u = (x / 2 + 1 / 2) * 8, v =
(1 / 2 - y / 2) * 8; level 0 of the pyramid is 4 x 4 texels of 2 x 2 pixels.

THE BOXES, by letter:
  V  [ 0.5, 0.75] x [0.25, 0.5] x [0.5, 0.5]   u in [6, 7], v in [2, 3]: texels (3, 1)         — right of every wall: visible
  H  [-0.75, -0.5] x [0.25, 0.5] x [0.5, 0.5]  u in [1, 2], v in [2, 3]: texels (0..1, 1)      — behind the OLD wall only
  S  [-0.75, -0.5] x [-0.5, -0.25] x [0.5, 0.5]  u in [1, 2], v in [5, 6]: texels (0..1, 2..3) — behind the old wall AND the new one
  O  [1024, 1025] x [0, 1] x [0, 0]            outside the frustum |x|, |y|, |z| <= 8 (u clamps to 7: in front of no wall)
OLD pyramid: depth 0.0 (a wall at the near plane) over the left half, pixels x < 4, and 1.0 elsewhere: H and S are occluded (d = 0
< 1, min ndc.z = 0.5 > 0), V is not (d = 1.0 never occludes). CLEAR: 1.0 everywhere — nothing is occluded. QUADRANT: 0.0 over
pixels x < 4, y >= 4 only: S is still occluded, H (texel row 1 = pixel rows 2..3, all 1.0) is not.

THE PLANES OF THE SECOND CALL accept nothing (x >= 4096 only): SECOND must not read them.

One mesh per distinct ladder of letters, one level each; mesh k's indices start where mesh k - 1's end and its vertex_offset is
1 + 3 x (the clusters of the meshes before): tight_geometry keeps vertex 0 for nobody."""
import numpy as np

import cluster_cases as cc
import cluster_edge_cases as ce
from renderer_amd.pipeline import DRAW_CMD_DTYPE, MESH_DTYPE

F = np.float32
BOXES = {"V": (0.5, 0.25, 0.5, 0.75, 0.5, 0.5), "H": (-0.75, 0.25, 0.5, -0.5, 0.5, 0.5), "S": (-0.75, -0.5, 0.5, -0.5, -0.25, 0.5),
         "O": (1024, 0, 0, 1025, 1, 0)}
PLANES = cc.PLANES                                   # |x|, |y|, |z| <= 8
SECOND_PLANES = np.array([-1, 0, 0, 4096] * 6, F)    # -x + 4096 > 0 is outside: everything with x < 4096
WIDTH = HEIGHT = 8
PV = np.eye(4, dtype=F).reshape(16)
PIN = cc.PIN


def _depth(kind):
    d = np.ones((HEIGHT, WIDTH), F)
    if kind == "old":
        d[:, :4] = 0.0
    elif kind == "quadrant":
        d[4:, :4] = 0.0
    else:
        assert kind == "clear"
    return d


def scene(ladders, instances, last=64, base=0):
    """ladders: one string of letters per mesh; instances: the mesh of each; last: triangles of every level's last cluster."""
    table = np.zeros(len(ladders), MESH_DTYPE)
    table["aabb_min"], table["aabb_max"], table["n_lods"] = (-1, -1, -1), (1, 1, 1), 1       # not read (DISTANCE policy)
    table, vertices, indices, want_boxes = ce.tight_geometry(table, [[ce.level([BOXES[ch] for ch in l], last=last)] for l in ladders])
    n = len(instances)
    rot = np.zeros((n, 4), F)
    rot[:, 3] = 1.0
    return dict(n=n, meshes=table, vertices=vertices, indices=indices, want_boxes=want_boxes, pos=np.zeros((n, 3), F), rot=rot, scale=np.ones(n, F),
                mesh_id=np.array(instances, np.uint32), planes=PLANES, second_planes=SECOND_PLANES, cam_pos=np.zeros(3, F), base=base,
                bitmap=np.full((n + 31) // 32, 0xFFFFFFFF, np.uint32), pv=PV, width=WIDTH, height=HEIGHT, old_depth=_depth("old"))


def _cmds(rows):
    return np.array(rows, DRAW_CMD_DTYPE) if rows else np.zeros(0, DRAW_CMD_DTYPE)


def _record(w, members, candidates, words):
    """{W, members, candidates, 0} and the 64-bit words, low half first."""
    out = [w, members, candidates, 0]
    for word in words:
        out += [word & 0xFFFFFFFF, word >> 32]
    return np.array(out, np.uint32)


def _want(first_rows, first_stats, record, second_rows, second_stats, new="clear"):
    """first / second: dict(cmds, stats — heads, survivors, W, members); record: the uint32 words; new_depth: SECOND's image."""
    return dict(first=dict(cmds=_cmds(first_rows), stats=np.array(first_stats, np.uint32)), record=record,
                second=dict(cmds=_cmds(second_rows), stats=np.array(second_stats, np.uint32)), new_depth=_depth(new))


def cases():
    """[(name, scene, want)]. A command is (indexCount, 1, firstIndex, vertexOffset, base + i)."""
    out = []
    ones = (1 << 64) - 1

    # item 0 is the candidate: phase 1 draws clusters 1..2 (384 indices at 192), phase 2 cluster 0
    s = scene(["HVV"], [0], base=7)
    out.append(("a candidate at c = 0", s, _want([(384, 1, 192, 1, 7)], (1, 2, 3, 1), _record(3, 1, 1, [0b001]), [(192, 1, 0, 1, 7)], (1, 1, 3, 1))))

    # the last cluster holds 5 triangles (T = 133): phase 2 draws its 15 indices at 384
    s = scene(["VVH"], [0], last=5, base=7)
    out.append(("a candidate at c = C - 1, short", s, _want([(384, 1, 0, 1, 7)], (1, 2, 3, 1), _record(3, 1, 1, [0b100]), [(15, 1, 384, 1, 7)], (1, 1, 3, 1))))

    # c = 1 of C = 3: phase 1 writes two commands around it, phase 2 one with firstIndex + 192 — a command of its own, though
    # it touches both runs phase 1 drew
    s = scene(["VHV"], [0], base=0xFFFFFFFF)           # the base wraps: firstInstance = base + 0
    out.append(("c = 1 of C = 3", s, _want([(192, 1, 0, 1, 0xFFFFFFFF), (192, 1, 384, 1, 0xFFFFFFFF)], (2, 2, 3, 1), _record(3, 1, 1, [0b010]),
                                          [(192, 1, 192, 1, 0xFFFFFFFF)], (1, 1, 3, 1))))

    # the last item of instance 0 and the first of instance 1 are candidates: neighbours in the work items, TWO commands.
    # mesh 1: indices from 384, vertices from 1 + 3 * 2 = 7
    s = scene(["VH", "HV"], [0, 1], base=9)
    out.append(("candidates meet across an instance boundary", s,
                _want([(192, 1, 0, 1, 9), (192, 1, 384 + 192, 7, 10)], (2, 2, 4, 2), _record(4, 2, 2, [0b0110]),
                      [(192, 1, 192, 1, 9), (192, 1, 384, 7, 10)], (2, 2, 4, 2))))

    # items 63 and 64 of one instance of 66 clusters: a run across two record words
    s = scene(["V" * 63 + "HH" + "V"], [0], base=1)
    out.append(("a run across items 63 | 64", s,
                _want([(192 * 63, 1, 0, 1, 1), (192, 1, 192 * 65, 1, 1)], (2, 64, 66, 1), _record(66, 1, 2, [1 << 63, 1]), [(384, 1, 192 * 63, 1, 1)], (1, 2, 66, 1))))

    # items 0..63 are candidates, 64..127 are not: a full word, then a zero word
    s = scene(["H" * 64 + "V" * 64], [0], base=2)
    out.append(("a whole word, then a zero word", s,
                _want([(192 * 64, 1, 192 * 64, 1, 2)], (1, 64, 128, 1), _record(128, 1, 64, [ones, 0]), [(192 * 64, 1, 0, 1, 2)], (1, 64, 128, 1))))

    # every item of three instances is a candidate: phase 1 draws nothing, phase 2 every level whole
    s = scene(["HH"], [0, 0, 0], last=3, base=3)       # T = 67: 201 indices
    out.append(("every item a candidate", s, _want([], (0, 0, 6, 3), _record(6, 3, 6, [0b111111]), [(201, 1, 0, 1, 3), (201, 1, 0, 1, 4), (201, 1, 0, 1, 5)], (3, 6, 6, 3))))

    # no candidates: the outside cluster is culled by the planes, not occluded — its bit stays clear (mesh 1: indices from 576,
    # vertices from 1 + 3 * 3 = 10)
    s = scene(["VOV", "VV"], [0, 1], base=4)
    out.append(("no candidates", s, _want([(192, 1, 0, 1, 4), (192, 1, 384, 1, 4), (384, 1, 576, 10, 5)], (3, 4, 5, 2), _record(5, 2, 0, [0]), [], (0, 0, 5, 2))))

    # three candidates, the middle one still hidden by the new (quadrant) pyramid: two commands, the last cluster short (7 triangles)
    s = scene(["HSH"], [0], last=7, base=5)
    out.append(("a candidate the new pyramid still hides", s,
                _want([], (0, 0, 3, 1), _record(3, 1, 3, [0b111]), [(192, 1, 0, 1, 5), (21, 1, 384, 1, 5)], (2, 2, 3, 1), new="quadrant")))
    return out


def occlusion_of(s, depth):
    """The restatement's occlusion dict for a scene and an image."""
    import occlusion_restatement as orr
    return dict(pv=s["pv"], levels=orr.pyramid_levels(depth), width=s["width"], height=s["height"])


def _runs(ladder, keep):
    """(first cluster, clusters) of every run of letters of `keep` in a ladder."""
    m = np.array([ch in keep for ch in ladder], bool)
    edge = np.diff(np.concatenate([[0], m.astype(np.int8), [0]]))
    return list(zip(np.nonzero(edge == 1)[0].tolist(), (np.nonzero(edge == -1)[0] - np.nonzero(edge == 1)[0]).tolist()))


def ladder_scene(ladders, instances, base=0, last=64, new="clear"):
    """Ladders of letters for the structural tests. Returns (scene, want) — want as cases() gives it, written down from the
    letters: phase 1 draws the runs of V, the record holds H and S, phase 2 draws the runs of H (and of S under a clear pyramid);
    one command per run per instance, a level's last cluster of `last` triangles."""
    s = scene(ladders, instances, last=last, base=base)
    t = s["meshes"]
    again = "HS" if new == "clear" else "H"
    rows = {"V": [], again: []}
    bits = []
    for i, k in enumerate(instances):
        off, vo, tris = int(t["index_offset"][k, 0]), int(t["vertex_offset"][k]), int(t["index_len"][k, 0]) // 3
        for keep in rows:
            rows[keep] += [(3 * (min(64 * (c + run), tris) - 64 * c), 1, off + 192 * c, vo, (base + i) & 0xFFFFFFFF) for c, run in _runs(ladders[k], keep)]
        bits += [ch in "HS" for ch in ladders[k]]
    bits = np.array(bits, bool)
    w, members = len(bits), len(instances)
    padded = np.zeros(64 * ((w + 63) // 64), np.uint8)
    padded[:w] = bits
    record = np.concatenate([np.array([w, members, int(bits.sum()), 0], np.uint32), np.packbits(padded, bitorder="little").view(np.uint32)])
    count = lambda keep: sum(ladders[k].count(ch) for k in instances for ch in keep)
    return s, dict(first=dict(cmds=_cmds(rows["V"]), stats=np.array([len(rows["V"]), count("V"), w, members], np.uint32)), record=record,
                   second=dict(cmds=_cmds(rows[again]), stats=np.array([len(rows[again]), count(again), w, members], np.uint32)), new_depth=_depth(new))


def filled(w, ladder_of, base=0):
    """W = w work items: instances of 64 clusters, ladder_of(j, 64) for the j-th, and one shorter one."""
    whole, rest = divmod(w, 64)
    ladders, instances = [], []
    for j in range(whole + (1 if rest else 0)):
        l = ladder_of(j, 64 if j < whole else rest)
        if l not in ladders:
            ladders.append(l)
        instances.append(ladders.index(l))
    return ladder_scene(ladders, instances, base=base)
