"""Scenes built ON the decision edges of the path, for every kernel that culls, picks a LOD or an arithmetic tier: a box
against a plane (sd - e exactly 0, a few ulps either side, subnormal, infinite, NaN), a squared distance against the LOD
threshold (the three floats around it, +inf, NaN), and an instance against the two limits that pick a wave's arithmetic
tier. Seeded and deterministic; no GPU, no torch. Every instance that sits on an edge carries a label that says which one,
for which frame (six planes + a LOD reference point) and which plane slot: tests/test_decision_cases.py proves the labels with
tests/numpy_restatement.py, tests/test_gpu_decision_edges.py runs the scenes through the kernels against the oracle.

A CASE is a set of instances over the five-entry mesh table below plus the names of the frames it is run with (the first is
the frame of a mip_run); FRAMES and REFS hold the planes and the reference points by name. layout(case, n) arranges a case
at one of the instance counts SIZES, edge instances first on the first and last lane of every wave and tile."""
import functools

import numpy as np

import float64_reference
import numpy_restatement as nr
from renderer_amd import scene as scene_mod
from renderer_amd.pipeline import MESH_DTYPE

F = np.float32
INF = F(np.inf)
TINY = np.finfo(F).tiny                      # smallest normal float32
U = F(2.0 ** -149)                           # the subnormal unit
SIZES = (1, 63, 64, 65, 255, 256, 257, 513)  # a wave, a tile, two tiles and one: the edges of both
NEAR_MAX = np.nextafter(F(100.0), INF)       # the largest squared distance that is still near: sqrt_rn(q) > 10 <=> q > this
SEPARABLE_LIMIT = F(1.0e37)                  # kSeparableLimit, kFiniteLimit (instance_kernel.hpp)
FINITE_LIMIT = F(3.0e38)
BOX_ABS = F(3.0)                             # sum of |box coordinates| of every mesh of the table: the census and a wave agree
MUTANTS = ("ge_zero", "flush_margin", "flush_inputs", "gt_100", "ge_threshold")
PLANE_MUTANTS = MUTANTS[:3]
IDENTITY = (0.0, 0.0, 0.0, 1.0)


def mesh_table():
    """Unit boxes (a tie is exact by construction) that differ in their LODs, so `visible` and `keep` differ on an edge:
    0: two LODs; 1: ONE LOD (a far instance falls back to LOD 0; the table's second length is a decoy); 2: LOD 0 empty;
    3: LOD 1 empty; 4: both empty."""
    t = np.zeros(5, MESH_DTYPE)
    t["aabb_min"], t["aabb_max"] = -0.5, 0.5
    t["n_lods"] = (2, 1, 2, 2, 2)
    t["index_len"][:, 0] = (36, 36, 0, 36, 0)
    t["index_len"][:, 1] = (18, 99, 18, 0, 0)
    t["index_offset"][:, 0] = (0, 100, 200, 300, 400)
    t["index_offset"][:, 1] = (36, 136, 236, 336, 436)
    t["vertex_offset"] = (0, -7, 24, 1 << 20, -(1 << 31))
    return t


MESHES = mesh_table()
MESHES.setflags(write=False)

# ---- the predicates of instance_tiered and of the upload-time census, mirrored in float32 ----


def rotation(rot):
    """quat_to_rotation (instance_kernel.hpp): (n, 3, 3)."""
    i, j, k, w = (np.asarray(rot, F).reshape(-1, 4)[:, c] for c in range(4))
    two = F(2.0)
    with np.errstate(all="ignore"):
        ww, ii, jj, kk = w * w, i * i, j * j, k * k
        ij, wk, wj = i * j * two, w * k * two, w * j * two
        ik, jk, wi = i * k * two, j * k * two, w * i * two
        r = np.empty((len(i), 3, 3), F)
        r[:, 0, 0] = ww + ii - jj - kk; r[:, 0, 1] = ij - wk; r[:, 0, 2] = wj + ik
        r[:, 1, 0] = wk + ij; r[:, 1, 1] = ww - ii + jj - kk; r[:, 1, 2] = jk - wi
        r[:, 2, 0] = ik - wj; r[:, 2, 1] = wi + jk; r[:, 2, 2] = ww - ii - jj + kk
    return r


def finite_magnitude(pos, rot, scale):
    pos, scale, r = np.asarray(pos, F).reshape(-1, 3), np.asarray(scale, F).reshape(-1), rotation(rot)
    with np.errstate(all="ignore"):
        mag = np.abs(pos[:, 0]) + np.abs(pos[:, 1]) + np.abs(pos[:, 2]) + np.abs(scale)
        for rr in range(3):
            for c in range(3):
                mag = mag + np.abs(r[:, rr, c])
    return mag


def separable_bound(pos, rot, scale, box_abs=BOX_ABS):
    pos, scale, r = np.asarray(pos, F).reshape(-1, 3), np.asarray(scale, F).reshape(-1), rotation(rot)
    with np.errstate(all="ignore"):
        sum_r = np.zeros(len(scale), F)
        for rr in range(3):
            for c in range(3):
                sum_r = sum_r + np.abs(r[:, rr, c])
        return sum_r * np.abs(scale) * F(box_abs) + (np.abs(pos[:, 0]) + np.abs(pos[:, 1]) + np.abs(pos[:, 2]))


def tier(pos, rot, scale):
    """What instance_tiered decides for an instance on its own: 0 the separable fold, 1 the corner enumeration (finite
    inputs that may overflow), 2 the literal chain. A wave takes the highest tier of its 64 lanes."""
    with np.errstate(all="ignore"):
        all_finite = (finite_magnitude(pos, rot, scale) + BOX_ABS) < FINITE_LIMIT
        separable = all_finite & (separable_bound(pos, rot, scale) < SEPARABLE_LIMIT)
    return np.where(separable, 0, np.where(all_finite, 1, 2))


def table_box_abs(meshes):
    """MipContext::box_abs as mip_set_mesh_table computes it: the largest sum of |box coordinate| over the table, every mesh's
    summed in float32 axis by axis, (|min| + |max|) added to the running sum; 0 for an empty table."""
    best = F(0.0)
    for k in range(len(meshes)):
        total = F(0.0)
        for a in range(3):
            total = F(total + F(np.abs(F(meshes["aabb_min"][k][a])) + np.abs(F(meshes["aabb_max"][k][a]))))
        if total > best:
            best = total
    return best


def census_fails(pos, rot, scale, box_abs=BOX_ABS):
    """mip_count_nonfinite_kernel, per instance: True where the instance fails the census under a table whose box_abs this is."""
    with np.errstate(all="ignore"):
        ok = (finite_magnitude(pos, rot, scale) < FINITE_LIMIT) & (separable_bound(pos, rot, scale, box_abs) < SEPARABLE_LIMIT)
    return ~ok


def census_fallbacks(s, box_abs=BOX_ABS):
    """mip_count_nonfinite_kernel: the instances that make the host launch the kernels with the fall-back tiers. box_abs: the
    resident table's (table_box_abs); the default is that of this module's table."""
    return int(census_fails(s["pos"], s["rot"], s["scale"], box_abs).sum())


# ---- the restatement's decisions, and its five mutants ----

def _flush(a):
    a = np.array(a, F, copy=True)
    with np.errstate(all="ignore"):
        a[np.abs(a) < TINY] = 0
    return a


def boxes(s):
    model = nr.model_matrices(s["pos"], s["rot"], s["scale"])
    return nr.world_aabbs(model, s["meshes"]["aabb_min"][s["mesh_id"]], s["meshes"]["aabb_max"][s["mesh_id"]])


def decide(s, mutant=None):
    """visible / far / lod / length / keep of every instance of a scene as the restatement decides them — or as one of the
    likely mistakes would: `sd - e >= 0`, a subnormal margin flushed to zero, subnormal inputs flushed to zero,
    `dist_sq > 100`, `dist_sq >= threshold`. Only this restatement is ever mutated; no wrong kernel is built or run."""
    assert mutant is None or mutant in MUTANTS
    if mutant == "flush_inputs":
        s = dict(s, pos=_flush(s["pos"]), rot=_flush(s["rot"]), scale=_flush(s["scale"]), planes=_flush(s["planes"]), cam_pos=_flush(s["cam_pos"]))
    mins, maxs = boxes(s)
    with np.errstate(all="ignore"):
        m = nr.plane_margins(mins, maxs, np.asarray(s["planes"], F).reshape(24))
        if mutant == "flush_margin":
            m = _flush(m)
        culled = ((m >= 0) if mutant == "ge_zero" else (m > 0)).any(axis=1)
        sq = nr.dist_sq(s["pos"], s["cam_pos"])
        far = (sq > F(100.0)) if mutant == "gt_100" else (sq >= NEAR_MAX) if mutant == "ge_threshold" else nr.lod_is_far(sq)
    lod = (far & (s["meshes"]["n_lods"][s["mesh_id"]] > 1)).astype(np.int64)
    length = s["meshes"]["index_len"][s["mesh_id"], lod]
    return dict(visible=~culled, far=far, lod=lod, length=length, keep=~culled & (length > 0), margins=m, dist_sq=sq)


def flips(s, mutant, indices, planes_matter=True):
    """How many of the instances `indices` of scene s a mutant decides differently (visibility, or the LOD)."""
    a, b = decide(s), decide(s, mutant)
    changed = a["lod"] != b["lod"]
    if planes_matter:
        changed |= a["visible"] != b["visible"]
    return int(changed[np.asarray(indices, np.int64)].sum())


# ---- frames ----

AXIS_PLANES = np.array([1, 0, 0, -4, -1, 0, 0, -4, 0, 2, 0, -8, 0, -0.5, 0, -2, 0, 0, 1, -16, 0, 0, -4, -8], F)
AXIS_TIE = ((0, 4.5), (0, -4.5), (1, 4.5), (1, -4.5), (2, 16.5), (2, -2.5))   # (axis, coordinate) of a unit box tangent to slot p
SUBNORMAL_PLANES = np.array([1, 0, 0, 0, -1, 0, 0, 0, 0, 1, 0, 0, 0, -0.5, 0, 0, 0, 0, 1, 0, 0, 0, -2, 0], F)
SUBNORMAL_SIGN = ((0, 1), (0, -1), (1, 1), (1, -1), (2, 1), (2, -1))
SPECIAL_PLANES = np.array([-0.0, 0.0, 1, -16, np.nan, 0, 0, 0, np.inf, 0, 0, -np.inf, 0, -np.inf, 0, 0, 0, 0, 3.4e38, 0, 0, 0, -1, -8], F)
VIEW_CAMERAS = (dict(cam_pos=(0.5, 1.0, 2.0), q=(0.1, -0.2, 0.05, 0.97), aspect=1.0, fovy_degrees=90.0, near=0.5, far=200.0),
                dict(cam_pos=(6.0, 2.0, -3.0), q=(0.3, 0.6, -0.1, 0.7), aspect=1.5, fovy_degrees=60.0, near=0.25, far=150.0),
                dict(cam_pos=(-5.0, 3.0, 4.0), q=(-0.5, 0.1, 0.4, 0.75), aspect=0.8, fovy_degrees=100.0, near=0.5, far=300.0),
                dict(cam_pos=(1.0, 8.0, 1.0), q=(0.7, 0.0, 0.1, 0.7), aspect=2.0, fovy_degrees=70.0, near=0.1, far=100.0))


def _frames():
    import oracle

    frames = {"axis": (AXIS_PLANES, np.zeros(3, F)),
              "camera": (scene_mod.default_planes(), np.asarray(scene_mod.DEFAULT_CAMERA["cam_pos"], F)),
              "subnormal": (SUBNORMAL_PLANES, np.array([0, 0, 3], F)),
              "special": (SPECIAL_PLANES, np.zeros(3, F))}
    for v, c in enumerate(VIEW_CAMERAS):
        q = np.asarray(c["q"], np.float64)
        q = (q / np.linalg.norm(q)).astype(F)
        cam = np.asarray(c["cam_pos"], F)
        frames[f"view{v}"] = (oracle.project_camera(cam, q, aspect=c["aspect"], fovy_degrees=c["fovy_degrees"], near=c["near"], far=c["far"]), cam)
    return frames


# ---- instance sets ----

class _Set:
    def __init__(self):
        self.pos, self.rot, self.scale, self.mesh, self.labels = [], [], [], [], []

    def add(self, pos, rot, scale, mesh, **label):
        label["index"] = len(self.pos)
        self.pos.append(np.asarray(pos, F).reshape(3)); self.rot.append(np.asarray(rot, F).reshape(4))
        self.scale.append(F(scale)); self.mesh.append(int(mesh)); self.labels.append(label)

    def extend(self, other):
        base = len(self.pos)
        self.pos += other.pos; self.rot += other.rot; self.scale += other.scale; self.mesh += other.mesh
        self.labels += [dict(l, index=l["index"] + base) for l in other.labels]
        return self

    def arrays(self):
        return (np.array(self.pos, F).reshape(-1, 3), np.array(self.rot, F).reshape(-1, 4), np.array(self.scale, F).reshape(-1),
                np.array(self.mesh, np.uint32).reshape(-1))


def _scene(pos, rot, scale, mesh_id, frame, frames):
    planes, cam = frames[frame]
    return dict(n=len(scale), pos=np.ascontiguousarray(pos, F), rot=np.ascontiguousarray(rot, F), scale=np.ascontiguousarray(scale, F),
                mesh_id=np.ascontiguousarray(mesh_id, np.uint32), meshes=MESHES, planes=np.asarray(planes, F).reshape(24), cam_pos=np.asarray(cam, F).reshape(3))


def _step(x, k):
    """x moved k floats up (k < 0: down)."""
    x = F(x)
    for _ in range(abs(int(k))):
        x = np.nextafter(x, INF if k > 0 else -INF)
    return x


def _random_rot(rng, n=None):
    q = rng.normal(size=(n or 1, 4))
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F)
    return q if n else q[0]


def _axis_ties():
    """Unit boxes (scale 1, identity rotation) and boxes of scale 2 tangent to each plane of the axis frame: power-of-two
    coefficients, so every product and sum of the chain is exact and sd - e is 0 by construction; then the centre moved
    +-1 .. +-4 floats along the normal."""
    st = _Set()
    for p, (axis, at) in enumerate(AXIS_TIE):
        for scale in (1.0, 2.0):
            # half extent scale / 2: the tangent centre moves out by (scale - 1) / 2 along the outward normal
            coord = at + np.sign(at) * (scale - 1.0) / 2.0
            for k in ((0, 1, -1, 2, -2, 3, -3, 4, -4) if scale == 1.0 else (0,)):   # (at scale 2 a one-float step can round away)
                pos = np.zeros(3, F)
                pos[axis] = _step(coord, k * (1 if at > 0 else -1))   # k > 0: outwards
                st.add(pos, IDENTITY, scale, 0 if k else (0, 3)[scale == 2.0], cls="tie0" if k == 0 else ("ulp_out" if k > 0 else "ulp_in"),
                       frame="axis", slot=p, k=k)
    return st


def _subnormal():
    """Planes through the origin with power-of-two normals, scales around 2e-39, centres from -1e-45 to 4e-39: sd and e are
    subnormal, sd - e is exact (subnormals are fixed point) and is a non-zero subnormal of either sign, or 0."""
    st = _Set()
    s = F(1427456) * U                       # 2.0003e-39, half = 713728 U
    h = F(713728) * U
    for p, (axis, sign) in enumerate(SUBNORMAL_SIGN):
        for k in (0, 1, -1, 2, -2):
            pos = np.zeros(3, F)
            pos[axis] = F(sign) * (h + F(4 * k) * U)
            st.add(pos, IDENTITY, s, 0, cls="sub_zero" if k == 0 else ("sub_pos" if k > 0 else "sub_neg"), frame="subnormal", slot=p, k=k)
    for x, cls in ((-U, "far_neg"), (F(0), "far_neg"), (U, "far_neg"), (F(4e-39), "far_pos")):   # subnormal margins that are no ties
        st.add((x, 0, 0), IDENTITY, s, 0, cls=cls, frame="subnormal", slot=0, k=None)
    # sd and e normal, their difference subnormal: what a flush of the subtraction's RESULT alone would lose
    for scale, cls in ((F(2.4e-38), "diff_pos"), (F(3.6e-38), "diff_neg")):
        st.add((F(1.5e-38), 0, 0), IDENTITY, scale, 0, cls=cls, frame="subnormal", slot=0, k=None)
    return st


def _nonfinite(frames):
    """Finite inputs whose margin is not finite (against slot 5 of the axis frame, normal (0, 0, -4)), a box whose extent
    overflows so that e = inf * 0 = NaN, and a grid of plain boxes for the frame whose planes hold -0, NaN, +-inf, 3.4e38."""
    st = _Set()
    st.add((0, 0, -1e38), IDENTITY, 2e38, 0, cls="inf_minus_inf", frame="axis", slot=5)
    st.add((0, 0, -1e38), IDENTITY, 1.0, 0, cls="pos_inf", frame="axis", slot=5)
    st.add((0, 0, 1e38), IDENTITY, 1.0, 0, cls="neg_inf", frame="axis", slot=5)
    st.add((0, 0, 0), (0, 0, np.sin(np.pi / 8), np.cos(np.pi / 8)), 3e38, 0, cls="nan_e", frame="axis", slot=0)
    k = 0
    for x in (-1.0, 0.0, 1.0):
        for y in (-1.0, 0.0, 1.0):
            for z in (0.25, 0.5, 0.75, 2.0):
                st.add((x, y, z), IDENTITY, 1.0, k % 5, cls="special_plane", frame="special", slot=None)
                k += 1
    cam = frames["axis"][1]
    st.add((np.nan, cam[1], cam[2]), IDENTITY, 1.0, 0, cls="sq_nan", ref="axis")
    st.add((np.nan, cam[1], cam[2]), IDENTITY, 1.0, 2, cls="sq_nan", ref="axis")
    return st


def _eval_margins(pos, rot, scale, planes, as_distance=False):
    """sd - e of unit boxes per plane slot, float32 chain; as_distance: divided by the normal's length (float64), for the
    builder's "clearly inside" tests only."""
    s = dict(pos=pos, rot=rot, scale=scale, mesh_id=np.zeros(len(scale), np.int64), meshes=MESHES)
    mins, maxs = boxes(s)
    m = nr.plane_margins(mins, maxs, np.asarray(planes, F).reshape(24))
    if as_distance:
        m = m.astype(np.float64) / np.linalg.norm(np.asarray(planes, np.float64).reshape(6, 4)[:, :3], axis=1)[None, :]
    return m


def _forward(rng, planes, cam):
    """A unit direction from the reference point well inside the frustum (found, not derived from a camera convention)."""
    d = rng.normal(size=(4000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pos = (np.asarray(cam, np.float64)[None, :] + 10.0 * d).astype(F)
    m = _eval_margins(pos, np.tile(np.array(IDENTITY, F), (len(pos), 1)), np.ones(len(pos), F), planes, as_distance=True)
    inside = (m < -1.0).all(axis=1)
    assert inside.sum() >= 10
    f = d[inside].mean(axis=0)
    return f / np.linalg.norm(f)


def _decided(pos, rot, scale, planes):
    s = dict(pos=pos, rot=rot, scale=scale, mesh_id=np.zeros(len(scale), np.int64), meshes=MESHES, planes=np.asarray(planes, F).reshape(24))
    return float64_reference.run(s)["decided"]


def _bisected_ties(rng, st, frame, frames, others=(), per_slot=2):
    """For each of the frame's six GENERAL planes: boxes of random rotation and scale moved along the plane's normal until two
    neighbouring float32 positions straddle the float32 chain's decision (`edge_in`: the last not culled by the plane,
    `edge_out`: the first culled), and, where the neighbourhood has one, a position whose sd - e is exactly 0 (`tie0`). The
    other five planes are clearly passed, and the frames `others` clearly decide the instance (float64_reference)."""
    planes, cam = frames[frame]
    fwd = _forward(rng, planes, cam)
    for p in range(6):
        normal = np.asarray(planes[4 * p : 4 * p + 3], np.float64)
        normal /= np.linalg.norm(normal)
        found = {"edge_in": 0, "edge_out": 0, "tie0": 0}
        for attempt in range(12):
            m = 24
            rot, scale = _random_rot(rng, m), rng.uniform(0.5, 2.0, m).astype(F)
            dist = rng.uniform(3.0, 30.0, (m, 1))
            side = rng.normal(size=(m, 3)) * 0.15
            c0 = np.asarray(cam, np.float64)[None, :] + dist * (fwd[None, :] + side)
            ok = (_eval_margins(c0.astype(F), rot, scale, planes, as_distance=True) < -1.0).all(axis=1)
            lo, hi = np.zeros(m), np.full(m, 1.0)
            at = lambda t: (c0 + t[:, None] * normal[None, :]).astype(F)
            for _ in range(14):              # walk out until plane p culls
                out = _eval_margins(at(hi), rot, scale, planes)[:, p] > 0
                hi = np.where(out, hi, hi * 2.0)
            ok &= _eval_margins(at(hi), rot, scale, planes)[:, p] > 0
            for _ in range(44):
                mid = 0.5 * (lo + hi)
                out = _eval_margins(at(mid), rot, scale, planes)[:, p] > 0
                lo, hi = np.where(out, lo, mid), np.where(out, mid, hi)
            p_in, p_out = at(lo), at(hi)
            axis = int(np.argmax(np.abs(normal)))
            for c in np.nonzero(ok)[0]:
                if min(found.values()) >= per_slot:
                    break
                cands = [("edge_in", p_in[c]), ("edge_out", p_out[c])]
                near = np.tile(p_in[c], (33, 1))
                for j in range(33):
                    near[j, axis] = _step(p_in[c, axis], j - 16)
                mz = _eval_margins(near, np.tile(rot[c], (33, 1)), np.full(33, scale[c], F), planes)[:, p]
                zero = np.nonzero(mz == 0)[0]
                if len(zero):
                    cands.append(("tie0", near[zero[len(zero) // 2]]))
                if np.array_equal(p_in[c], p_out[c]):
                    continue
                cp = np.array([x[1] for x in cands], F)
                cr, cs = np.tile(rot[c], (len(cp), 1)), np.full(len(cp), scale[c], F)
                mm = _eval_margins(cp, cr, cs, planes)
                rest = np.delete(_eval_margins(cp, cr, cs, planes, as_distance=True), p, axis=1)
                clear = (rest < -0.05).all(axis=1)
                for o in others:
                    clear &= _decided(cp, cr, cs, frames[o][0])
                if not clear.all():
                    continue
                for (cls, pos), margin in zip(cands, mm[:, p]):
                    if found[cls] < per_slot:
                        found[cls] += 1
                        st.add(pos, rot[c], scale[c], (0, 3, 1)[found[cls] % 3], cls=cls, frame=frame, slot=p, k=None)
            if found["edge_in"] >= per_slot and found["edge_out"] >= per_slot and (found["tie0"] >= 1 or attempt >= 1):
                break
        assert found["edge_in"] and found["edge_out"], (frame, p, found)


LOD_RING = (("sq_lo3", -3), ("sq_lo2", -2), ("sq_lo1", -1), ("sq_100", 0), ("sq_near_max", 1), ("sq_far1", 2), ("sq_far2", 3), ("sq_far3", 4))


def lod_ring_value(cls):
    """The float32 squared distance a ring label stands for: 100 moved k floats."""
    return _step(F(100.0), dict(LOD_RING)[cls])


def _lod_ring(rng, st, ref_name, ref, fwd, offset=0, nan=False):
    """Instances whose float32 squared distance to `ref` is each float from three below 100 to three above the threshold
    (found by search along directions near `fwd`), one on top of the point, one at +inf from finite inputs (a box of scale
    1e20, so that a frustum still sees it) and, on request, one at NaN (a NaN position: near). The mesh rotates through the
    table, so empty LODs and the one-LOD fall-back meet every class."""
    ref64 = np.asarray(ref, np.float64)
    d = fwd[None, :] + rng.normal(size=(6000, 3)) * 0.1
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = 10.0 * (1.0 + rng.uniform(-4e-7, 4e-7, (6000, 1)))
    pos = (ref64[None, :] + r * d).astype(F)
    sq = nr.dist_sq(pos, ref)
    k = offset
    for cls, _ in LOD_RING:
        hit = np.nonzero(sq == lod_ring_value(cls))[0]
        assert len(hit), (ref_name, cls)
        st.add(pos[hit[0]], _random_rot(rng), 1.0, k % 5, cls=cls, ref=ref_name)
        k += 1
    st.add(np.asarray(ref, F), _random_rot(rng), 1.0, k % 5, cls="on_top", ref=ref_name)
    st.add(np.asarray(ref, F) + np.array([2e19, 0, 0], F), IDENTITY, 1e20, (k + 1) % 5, cls="sq_inf", ref=ref_name)
    if nan:
        st.add((np.nan, ref[1], ref[2]), IDENTITY, 1.0, (k + 2) % 5, cls="sq_nan", ref=ref_name)


def ring_classes(nan=False):
    return [c for c, _ in LOD_RING] + ["on_top", "sq_inf"] + (["sq_nan"] if nan else [])


def _fillers(rng, n):
    """Ordinary instances: near the origin, well inside the axis frame, small."""
    return (rng.uniform(-1.0, 1.0, (n, 3)).astype(F), _random_rot(rng, n) if n else np.zeros((0, 4), F), rng.uniform(0.5, 1.5, n).astype(F),
            rng.integers(0, 5, n).astype(np.uint32))


N_LIGHTS = 16


@functools.lru_cache(maxsize=None)
def catalogue():
    """dict(frames, refs, lights, cases): cases[name] = dict(name, pos, rot, scale, mesh_id, labels, frames, fallback)."""
    rng = np.random.default_rng(0xDEC1DE)
    frames = _frames()
    refs = {name: cam for name, (_, cam) in frames.items()}
    lights = rng.uniform(-30.0, 30.0, (N_LIGHTS, 3)).astype(F)
    for l in range(N_LIGHTS):
        refs[f"light{l}"] = lights[l]
    sets = {}
    sets["axis"] = (_axis_ties(), ("axis",))
    cam_set = _Set()
    _bisected_ties(rng, cam_set, "camera", frames)
    _lod_ring(rng, cam_set, "camera", refs["camera"], _forward(rng, *frames["camera"]))
    sets["camera"] = (cam_set, ("camera",))
    view_set = _Set()
    names = tuple(f"view{v}" for v in range(len(VIEW_CAMERAS)))
    for v, name in enumerate(names):
        _bisected_ties(rng, view_set, name, frames, others=[o for o in names if o != name], per_slot=1)
        _lod_ring(rng, view_set, name, refs[name], _forward(rng, *frames[name]), offset=v)
    sets["views"] = (view_set, names)
    sets["subnormal"] = (_subnormal(), ("subnormal",))
    sets["nonfinite"] = (_nonfinite(frames), ("axis", "special"))
    light_set = _Set()
    for l in range(N_LIGHTS):
        _lod_ring(rng, light_set, f"light{l}", lights[l], np.array([0.0, 0.0, 1.0]), offset=l, nan=True)
    sets["lights"] = (light_set, ("camera",))
    union = _Set()
    for name in ("views", "subnormal", "axis", "camera"):
        union.extend(sets[name][0])
    sets["union"] = (union, names + ("subnormal", "axis", "camera"))
    union_nf = _Set().extend(union).extend(sets["nonfinite"][0])
    sets["union_nonfinite"] = (union_nf, ("special", "view1", "subnormal", "axis", "view3"))
    cases = {}
    for name, (st, case_frames) in sets.items():
        pos, rot, scale, mesh = st.arrays()
        case = dict(name=name, pos=pos, rot=rot, scale=scale, mesh_id=mesh, labels=tuple(st.labels), frames=tuple(case_frames))
        case["fallback"] = census_fallbacks(case) > 0
        for a in (pos, rot, scale, mesh):
            a.setflags(write=False)
        cases[name] = case
    return dict(frames=frames, refs=refs, lights=lights, cases=cases)


def case(name):
    return catalogue()["cases"][name]


def scene_of(c, frame=None):
    """The whole case as a scene under one of its frames (default: the first)."""
    return _scene(c["pos"], c["rot"], c["scale"], c["mesh_id"], frame or c["frames"][0], catalogue()["frames"])


# what each kernel is run on: (case, frame) pairs for the kernels that take one frame, (case, frames) for the views kernel
RUN_INPUTS = (("axis", "axis"), ("camera", "camera"), ("views", "view0"), ("views", "view2"), ("subnormal", "subnormal"),
              ("nonfinite", "axis"), ("nonfinite", "special"))
VIEW_INPUTS = ("union", "union_nonfinite")
LIGHT_INPUTS = ("lights",)
KERNEL_INPUTS = {"mip_run": RUN_INPUTS, "run_occluded": RUN_INPUTS, "batch_draws": RUN_INPUTS,
                 "mip_run_views": tuple((c, None) for c in VIEW_INPUTS), "light_draw_lists": tuple((c, None) for c in LIGHT_INPUTS)}


def labelled(c, frame=None, ref=None):
    """Indices of the case's instances built on an edge of this frame's planes / of this reference point."""
    return [l["index"] for l in c["labels"] if (frame is not None and l.get("frame") == frame) or (ref is not None and l.get("ref") == ref)]


def mutant_flips(kernel, mutant):
    """Labelled instances of the kernel's input set that the mutant decides differently, summed over the frames (or the
    lights) the kernel sees them under. A label counts under the frame / reference point it was built for."""
    cat = catalogue()
    total = 0
    for name, frame in KERNEL_INPUTS[kernel]:
        c = cat["cases"][name]
        if kernel == "light_draw_lists":
            for l in range(N_LIGHTS):
                s = dict(scene_of(c), cam_pos=cat["lights"][l])
                total += flips(s, mutant, labelled(c, ref=f"light{l}"), planes_matter=False)
            continue
        for f in ([frame] if frame else c["frames"]):
            idx = labelled(c, frame=f, ref=f)
            if idx:
                total += flips(scene_of(c, f), mutant, idx)
    return total


# ---- a case at one of the instance counts ----

def priority_slots(n):
    """The first and last lane of every wave (and so of every tile) of an n-instance launch, the scene's last instance first
    among them; then every other slot in order."""
    first = [0, n - 1]
    for w in range((n + 63) // 64):
        first += [64 * w, 64 * w + 63]
    seen, out = set(), []
    for i in first + list(range(n)):
        if 0 <= i < n and i not in seen:
            seen.add(i)
            out.append(i)
    return out


@functools.lru_cache(maxsize=None)
def layout(name, n, frame=None):
    """(scene of n instances, src): the case's edge instances on the priority slots (rotated by n, so the sizes put different
    edges first; all of them when n allows), ordinary instances everywhere else. src[i] = index in the case, or -1."""
    c = case(name)
    e = len(c["scale"])
    rng = np.random.default_rng(1000 * n + e)
    pos, rot, scale, mesh = _fillers(rng, n)
    src = np.full(n, -1, np.int64)
    order = np.roll(np.arange(e), -((7 * n) % e))
    for slot, k in zip(priority_slots(n), order):
        src[slot] = k
    put = src >= 0
    pos[put], rot[put], scale[put], mesh[put] = c["pos"][src[put]], c["rot"][src[put]], c["scale"][src[put]], c["mesh_id"][src[put]]
    return _scene(pos, rot, scale, mesh, frame or c["frames"][0], catalogue()["frames"]), src


# ---- tier edges: one odd instance in a wave of ordinary ones, and the twin scene without it ----

def _bits_bisect(lo, hi, below):
    """lo, hi: positive float32 with below(lo) and not below(hi); returns the neighbouring pair where the predicate turns."""
    a, b = int(np.array(lo, F).view(np.uint32)), int(np.array(hi, F).view(np.uint32))
    as_f = lambda k: np.array(k, np.uint32).view(F)[()]
    assert below(as_f(a)) and not below(as_f(b))
    while b - a > 1:
        mid = (a + b) // 2
        if below(as_f(mid)):
            a = mid
        else:
            b = mid
    return as_f(a), as_f(b)


TIER_ROT = np.array([0.18257418, 0.36514837, 0.54772256, 0.73029674], F)   # (1, 2, 3, 4) / sqrt(30)


@functools.lru_cache(maxsize=None)
def tier_edge_instances():
    """{(kind, via): (pos, rot, scale)}; kind: sep_below / sep_at (separable_bound: the last float below 1e37 / the first at or
    above) and fin_below / fin_at (finite_magnitude against 3e38); via: found by bisection on the scale, or on a position."""
    out = {}
    rot = TIER_ROT
    for limit_name, limit, fn, s_range, fixed_scale in (("sep", SEPARABLE_LIMIT, separable_bound, (1e35, 3e37), 3e35),
                                                        ("fin", FINITE_LIMIT, finite_magnitude, (1e38, 3.4e38), 1.0)):
        small = np.array([1.0, 2.0, 3.0], F)
        below = lambda s: bool(fn(small, rot, s)[0] < limit)
        a, b = _bits_bisect(*s_range, below)
        out[(limit_name + "_below", "scale")] = (small, rot, a)
        out[(limit_name + "_at", "scale")] = (small, rot, b)
        p_of = lambda x: np.array([x, 2.0, 3.0], F)
        below = lambda x: bool(fn(p_of(x), rot, fixed_scale)[0] < limit)
        a, b = _bits_bisect(F(limit) / F(16), F(limit), below)
        out[(limit_name + "_below", "pos")] = (p_of(a), rot, F(fixed_scale))
        out[(limit_name + "_at", "pos")] = (p_of(b), rot, F(fixed_scale))
    return out


TIER_KINDS = ("sep_below", "sep_at", "fin_below", "fin_at")
TIER_PLACEMENTS = {"lane0": (257, (64,)), "lane63": (257, (127,)), "pair": (257, (255, 256)), "partial": (255, (254,))}


@functools.lru_cache(maxsize=None)
def tier_scene(kind, placement):
    """(scene, twin, odd): ordinary instances with the odd one(s) of `kind` at the placement's lanes; the twin has ordinary
    instances there too. Default camera frame."""
    n, odd = TIER_PLACEMENTS[placement]
    rng = np.random.default_rng(100_000 * TIER_KINDS.index(kind) + 1000 * n + odd[0])
    pos, rot, scale, mesh = _fillers(rng, n)
    pos[:, 2] += F(6.0)                      # in front of the default camera
    twin = _scene(pos.copy(), rot.copy(), scale.copy(), mesh.copy(), "camera", catalogue()["frames"])
    inst = tier_edge_instances()
    for j, i in enumerate(odd):
        via = ("pos", "scale")[(j + list(TIER_PLACEMENTS).index(placement)) % 2]
        pos[i], rot[i], scale[i] = inst[(kind, via)]
        mesh[i] = 0
    return _scene(pos, rot, scale, mesh, "camera", catalogue()["frames"]), twin, odd


def ordinary_lanes(n, odd):
    """The instances of the waves that hold an odd one, without the odd ones: the lanes that must keep their bytes."""
    waves = sorted({i // 64 for i in odd})
    return np.array([i for w in waves for i in range(64 * w, min(64 * w + 64, n)) if i not in odd], np.int64)
