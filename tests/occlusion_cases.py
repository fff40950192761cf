"""Scenes built ON the edges of the occlusion test (include/mi_instance_pipeline.h, MipOcclusion, steps 1-9) and labelled on
the CPU: no GPU, no torch. tests/test_occlusion_cases.py proves every label with occlusion_restatement.occlusion_terms and
shows on mutants of the restatement that the scenes tell the likely mistakes apart; tests/test_gpu_occlusion_edges.py runs
the scenes through mip_build_depth_pyramid and mip_run_occluded.

A CASE is a scene (pos, rot, scale, mesh_id, meshes, all-accepting planes, cam_pos), a pv, a depth image and, per edge
instance, a label dict(index, cls, side, check): cls names the step of the header the instance sits on, side which side of the
edge, check the terms (occlusion_terms keys and a few derived ones, see verify()) it was built to have. Edge instances have
identity rotation, scale 1 and position 0 and a mesh of their own, so the mesh AABB is the world box: coordinates are either
coarse dyadic numbers or symmetric about 0 (then centre -+ half of the world box is exact), and a depth that must be exact
is a flat box (zmin == zmax). zmin comes from each of the eight corners in turn under eight sheared orthographic pvs
(pv_shear). Under the orthographic pv (the identity: w == 1, u and v exact for power-of-two images) a
pixel position and zmin are arranged through the box; d is arranged through the image (painted pixels) or read off the final
image before zmin is set to d, the float above or the float below. Most geometric members come as a pair: zmin == d (a tie:
not occluded) and zmin one float above d (occluded), so ANY mistake that changes d flips one of the two.

What cannot be built: u or v equal to -0.0 ((t + 0.5) and (0.5 - t) are never -0 in round-to-nearest); a rectangle that
reads the 1 x 1 top level of an image with more than one level-0 texel a side (step 7 stops at a level with at most two
texels a side: test_occlusion_cases.py computes the reachable levels by enumeration); a subnormal w under
scene.default_pv() (w = z - 2 is a multiple of 2^-23 there; the hand-written perspective has them)."""
import functools

import numpy as np

import numpy_restatement as nr
import occlusion_restatement as occ
from renderer_amd import scene as scene_mod
from renderer_amd.pipeline import MESH_DTYPE

F = np.float32
INF = F(np.inf)
U = F(2.0 ** -149)                           # the smallest subnormal
SUB_MAX = np.nextafter(np.finfo(F).tiny, F(0))
TINY = np.finfo(F).tiny                      # the smallest normal
FLT_MAX = occ.FLT_MAX
BELOW_ONE = np.nextafter(F(1.0), F(0))
N = 1243                                     # five tiles of 256, the last one partial
TILE = 256
IDENTITY = (0.0, 0.0, 0.0, 1.0)
CLASSES = ("step3", "step56", "step7", "step8", "step9")
N_FILLER_MESHES = 4

MUTANTS = ("ge_d", "d_le_one", "trunc", "clamp_w", "no_clamp0", "v_not_flipped", "pv_row_major", "w_ge_zero", "flush_w",
           "step7_lt1", "k_minus", "k_plus", "step7_x_only", "lw_floor", "off_floor", "texel00_only", "tx1_dropped", "ty1_dropped",
           "zmax", "u16_65536")
# trunc: floor and truncation differ on (-1, 0) only, and the clamp at 0 of the same step sends both answers to 0 — it is no
# mistake the outputs can show (test_occlusion_cases.py asserts that it changes no term).
EQUIVALENT_MUTANTS = ("trunc",)


def _step(x, k):
    """x moved k floats up (k < 0: down)."""
    x = F(x)
    for _ in range(abs(int(k))):
        x = np.nextafter(x, INF if k > 0 else -INF)
    return x


def pv_ortho():
    return np.eye(4, dtype=F).reshape(16)


def pv_big():
    """A hand-written perspective, column-major: clip.x = 1e38 x - 1e38 y + 2e38, clip.y = FLT_MAX y, clip.z = z + 0.25,
    w = z. Every finite clip.x / w is far outside the image (the clamps of step 6 decide), ndc.z > 1 wherever w > 0 (so
    occluded == ok and d < 1), and the sums overflow where the box says."""
    m = np.zeros(16, F)
    big = F(1e38)
    m[0], m[4], m[12] = big, -big, big * F(2)
    m[5] = FLT_MAX
    m[10], m[14] = 1.0, 0.25
    m[11] = 1.0
    return m


def corner_clips(boxes, pv):
    """clip of the eight corners (n, 8, 4), step 2's chain."""
    b = np.asarray(boxes, F).reshape(-1, 6)
    m = np.asarray(pv, F).reshape(16)
    out = np.empty((len(b), 8, 4), F)
    with np.errstate(all="ignore"):
        for c in range(8):
            x = b[:, 3] if c & 1 else b[:, 0]
            y = b[:, 4] if c & 2 else b[:, 1]
            z = b[:, 5] if c & 4 else b[:, 2]
            for r in range(4):
                out[:, c, r] = ((m[r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r]
    return out


# ---- the restatement again, with one likely mistake switched on ----

def mutant_levels(depth, mutant=None):
    if mutant == "u16_65536" and np.asarray(depth).dtype == np.uint16:
        px = np.asarray(depth).astype(F) / F(65536.0)
        return occ.pyramid_levels(px)
    return occ.pyramid_levels(depth)


def mutant_occluded(world_aabb, pv, depth, mutant=None):
    """occlusion_restatement.occlusion_terms()["occluded"] as a kernel with one mistake would compute it, over the FLAT
    pyramid as the kernel addresses it (level offset and level width computed, reads clipped to the buffer). mutant None is the
    restatement itself (asserted by the CPU test). Only this copy is ever wrong; no wrong kernel is built or run."""
    assert mutant is None or mutant in MUTANTS
    depth = np.asarray(depth)
    height, width = depth.shape
    levels = mutant_levels(depth, mutant)
    flat = occ.pyramid_flat(levels)
    top = len(levels) - 1
    b = np.asarray(world_aabb, F).reshape(-1, 6)
    m = np.asarray(pv, F).reshape(16)
    if mutant == "pv_row_major":
        m = m.reshape(4, 4).T.reshape(16).copy()
    wf, hf = F(width), F(height)
    n = b.shape[0]
    ok = np.ones(n, bool)
    umin, umax = np.full(n, np.inf, F), np.full(n, -np.inf, F)
    vmin, vmax = np.full(n, np.inf, F), np.full(n, -np.inf, F)
    zmin = np.full(n, -np.inf if mutant == "zmax" else np.inf, F)
    with np.errstate(all="ignore"):
        for c in range(8):
            x = b[:, 3] if c & 1 else b[:, 0]
            y = b[:, 4] if c & 2 else b[:, 1]
            z = b[:, 5] if c & 4 else b[:, 2]
            clip = [((m[r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r] for r in range(4)]
            w = clip[3]
            if mutant == "flush_w":
                w = np.where(np.abs(w) < TINY, F(0), w)
            positive = (w >= F(0)) if mutant == "w_ge_zero" else (w > F(0))
            ok &= np.isfinite(clip[0]) & np.isfinite(clip[1]) & np.isfinite(clip[2]) & np.isfinite(clip[3]) & positive
            rw = F(1.0) / w
            nx, ny, nz = clip[0] * rw, clip[1] * rw, clip[2] * rw
            u = (nx * F(0.5) + F(0.5)) * wf
            v = ((F(0.5) + ny * F(0.5)) if mutant == "v_not_flipped" else (F(0.5) - ny * F(0.5))) * hf
            umin, umax = np.fmin(umin, u), np.fmax(umax, u)
            vmin, vmax = np.fmin(vmin, v), np.fmax(vmax, v)
            zmin = np.fmax(zmin, nz) if mutant == "zmax" else np.fmin(zmin, nz)
        whole = np.trunc if mutant == "trunc" else np.floor

        def clamp(a, extent):
            a = whole(a)
            if mutant != "no_clamp0":
                a = np.fmax(a, F(0))
            a = np.fmin(a, F(extent if mutant == "clamp_w" else extent - 1))
            return np.clip(np.where(np.isnan(a), 0, a), -(1 << 30), 1 << 30).astype(np.int64)

        x0, x1, y0, y1 = clamp(umin, width), clamp(umax, width), clamp(vmin, height), clamp(vmax, height)
    k = np.zeros(n, np.int64)
    limit = 0 if mutant == "step7_lt1" else 1
    while True:
        more = (x1 >> (k + 1)) - (x0 >> (k + 1)) > limit
        if mutant != "step7_x_only":
            more |= (y1 >> (k + 1)) - (y0 >> (k + 1)) > limit
        more &= k < top
        if not more.any():
            break
        k += more
    if mutant == "k_minus":
        k = np.maximum(k - 1, 0)
    if mutant == "k_plus":
        k = np.minimum(k + 1, top)
    extent = lambda side, lvl: ((side - 1) >> (lvl + 1)) + 1
    below = (lambda side, lvl: np.maximum(side >> (lvl + 1), 1)) if mutant == "off_floor" else extent
    off = np.zeros(n, np.int64)
    for lvl in range(top):
        off += np.where(k > lvl, below(width, lvl) * below(height, lvl), 0)
    lw = np.maximum(width >> (k + 1), 1) if mutant == "lw_floor" else extent(width, k)
    tx0, tx1, ty0, ty1 = x0 >> (k + 1), x1 >> (k + 1), y0 >> (k + 1), y1 >> (k + 1)
    if mutant in ("texel00_only", "tx1_dropped"):
        tx1 = tx0
    if mutant in ("texel00_only", "ty1_dropped"):
        ty1 = ty0
    read = lambda ty, tx: flat[np.clip(off + ty * lw + tx, 0, len(flat) - 1)]
    d = np.fmax(np.fmax(read(ty0, tx0), read(ty0, tx1)), np.fmax(read(ty1, tx0), read(ty1, tx1)))
    cleared = (d <= F(1.0)) if mutant == "d_le_one" else (d < F(1.0))
    behind = (zmin >= d) if mutant == "ge_d" else (zmin > d)
    return ok & cleared & behind


# ---- building a case ----

def _filler_meshes():
    t = np.zeros(N_FILLER_MESHES, MESH_DTYPE)
    half = np.array([2.0 ** -4, 2.0 ** -3, 2.0 ** -5, 2.0 ** -4], F)
    t["aabb_min"], t["aabb_max"] = -half[:, None], half[:, None]
    t["n_lods"] = 1
    t["index_len"][:, 0] = (36, 12, 0, 60)  # (mesh 2 is empty: visible, no command)
    t["index_offset"][:, 0] = (0, 36, 48, 48)
    t["vertex_offset"] = (0, -7, 24, 1 << 20)
    return t


class _Case:
    def __init__(self, name, width, height, fmt, pv, seed, plain=False):
        self.name, self.width, self.height, self.fmt, self.pv = name, width, height, fmt, np.asarray(pv, F).reshape(16)
        self.rng = np.random.default_rng(seed)
        if fmt == "u16":
            self.depth = self.rng.integers(16384, 49152, (height, width)).astype(np.uint16)
            if not plain:
                self.depth[self.rng.random((height, width)) < 0.03] = 65535
        else:
            self.depth = self.rng.uniform(0.25, 0.75, (height, width)).astype(F)
            if not plain:
                self.depth[self.rng.random((height, width)) < 0.03] = 1.0
                self.depth[self.rng.random((height, width)) < 0.02] = np.nan  # (counts as 1.0)
        self.members = []

    def value(self, v):
        """A depth the image can hold: v for f32, round(v * 65535) for u16 — returns (pixel, float32 depth)."""
        if self.fmt == "u16":
            p = np.uint16(round(float(v) * 65535))
            return p, F(p) / F(65535.0)
        return F(v), F(v) + F(0)

    def paint(self, x, y, v, w=1, h=1):
        self.depth[y : y + h, x : x + w] = v

    def add(self, cls, side, xy, z=("rel", 0), **check):
        """xy: (xlo, xhi, ylo, yhi) of the box; z: ("rel", k) a flat box k floats from d, or ("abs", zlo, zhi)."""
        assert cls in CLASSES
        self.members.append(dict(cls=cls, side=side, xy=tuple(F(c) for c in xy), z=z, check=dict(check)))

    def pair(self, cls, side, xy, **check):
        """zmin == d (a tie: not occluded) and zmin the float above d (occluded, unless the texel is cleared)."""
        self.add(cls, side + "/tie", xy, ("rel", 0), zmin_minus_d=0, **check)
        self.add(cls, side + "/behind", xy, ("rel", 1), zmin_minus_d=1, **check)

    # pixel coordinates to box coordinates under the orthographic pv
    def ndc_x(self, u):
        return F(2.0 * float(u) / self.width - 1.0)

    def ndc_y(self, v):
        return F(1.0 - 2.0 * float(v) / self.height)

    def pixels(self, x0, x1, y0, y1):
        """The box whose rectangle is pixels x0..x1, y0..y1 (corners on the pixel centres; v is flipped)."""
        return (self.ndc_x(x0 + 0.5), self.ndc_x(x1 + 0.5), self.ndc_y(y1 + 0.5), self.ndc_y(y0 + 0.5))

    def x_for_u(self, target):
        """The box coordinate whose u is exactly `target` (searched around the float64 inverse)."""
        x = self.ndc_x(float(target))
        for k in sorted(range(-8, 9), key=abs):
            c = _step(x, k)
            if (c * F(0.5) + F(0.5)) * F(self.width) == F(target):
                return c
        raise AssertionError((self.name, "no box coordinate gives u", target))

    def y_for_v(self, target):
        y = self.ndc_y(float(target))
        for k in sorted(range(-8, 9), key=abs):
            c = _step(y, k)
            if (F(0.5) - c * F(0.5)) * F(self.height) == F(target):
                return c
        raise AssertionError((self.name, "no box coordinate gives v", target))

    def finish(self, filler_pos):
        """Lay the members out, fill the rest, set the depths that hang on d, and label."""
        rng = self.rng
        members = self.members
        e = len(members)
        assert e + 64 <= N, (self.name, e)
        # every class on the first and the last instance of a tile and on lane 0 and lane 63 of a wave inside one
        tiles = (N + TILE - 1) // TILE
        tile_first = [TILE * t for t in range(tiles)]
        tile_last = [min(TILE * t + TILE - 1, N - 1) for t in range(tiles)]
        lane0 = [i for i in range(64, N, 64) if i % TILE]
        lane63 = [i for i in range(63, N - 1, 64) if i % TILE != TILE - 1]
        slot_of = {}
        taken = set()
        present = [c for c in CLASSES if any(mb["cls"] == c for mb in members)]
        for ci, cls in enumerate(present):
            mine = [j for j, mb in enumerate(members) if mb["cls"] == cls]
            wanted = (tile_first[ci % tiles], tile_last[(ci + 2) % tiles], lane0[ci], lane63[-1 - ci])
            for j, slot in zip(mine[:: max(len(mine) // 4, 1)], wanted):
                slot_of[j] = slot
                taken.add(slot)
        free = iter([i for i in rng.permutation(N) if i not in taken])
        for j in range(e):
            if j not in slot_of:
                slot_of[j] = int(next(free))
        filler_meshes = _filler_meshes()
        meshes = np.zeros(N_FILLER_MESHES + e, MESH_DTYPE)
        meshes[:N_FILLER_MESHES] = filler_meshes
        pos = np.asarray(filler_pos(rng, N), F).reshape(N, 3)
        mesh_id = rng.integers(0, N_FILLER_MESHES, N).astype(np.uint32)
        lengths = (36, 3, 0, 96, 18)
        for j, mb in enumerate(members):
            i = slot_of[j]
            pos[i] = 0
            mesh_id[i] = N_FILLER_MESHES + j
            row = meshes[N_FILLER_MESHES + j]
            row["n_lods"] = 1
            row["index_len"][0] = lengths[j % len(lengths)]
            row["index_offset"][0] = 7 * j
            row["vertex_offset"] = j - 50
            mb["index"] = i
        rot = np.tile(np.array(IDENTITY, F), (N, 1))
        scale = np.ones(N, F)
        levels = occ.pyramid_levels(self.depth)

        def boxes_of(zs):
            for j, mb in enumerate(members):
                xlo, xhi, ylo, yhi = mb["xy"]
                meshes["aabb_min"][N_FILLER_MESHES + j] = (xlo, ylo, zs[j][0])
                meshes["aabb_max"][N_FILLER_MESHES + j] = (xhi, yhi, zs[j][1])
            model = nr.model_matrices(pos, rot, scale)
            lo, hi = nr.world_aabbs(model, meshes["aabb_min"][mesh_id], meshes["aabb_max"][mesh_id])
            return np.concatenate([lo, hi], 1)

        idx = np.array([mb["index"] for mb in members], np.int64)
        zs = [(F(0.5), F(0.5)) if mb["z"][0] == "rel" else (F(mb["z"][1]), F(mb["z"][2])) for mb in members]
        d = occ.occlusion_terms(boxes_of(zs)[idx], self.pv, levels, self.width, self.height)["d"]  # (d does not hang on z)
        for j, mb in enumerate(members):
            if mb["z"][0] == "rel":
                zs[j] = (_step(d[j], mb["z"][1]),) * 2
        boxes = boxes_of(zs)
        labels = tuple(dict(index=int(mb["index"]), cls=mb["cls"], side=mb["side"], check=mb["check"]) for mb in members)
        case = dict(name=self.name, n=N, width=self.width, height=self.height, fmt=self.fmt, pv=self.pv, depth=self.depth,
                    pos=pos, rot=rot, scale=scale, mesh_id=mesh_id, meshes=meshes, planes=np.zeros(24, F), cam_pos=np.zeros(3, F),
                    labels=labels, boxes=boxes)
        for a in (self.depth, pos, rot, scale, mesh_id, meshes, boxes, self.pv):
            a.setflags(write=False)
        return case


def _ortho_filler(rng, n):
    return np.stack([rng.uniform(-1.1, 1.1, n), rng.uniform(-1.1, 1.1, n), rng.uniform(0.4, 1.3, n)], 1)


def _geometry_members(c):
    """Steps 5-7 on an orthographic image of any extent: rectangles given in pixels, boxes outside the image, every level step
    7 can select with x, y or both deciding, kept at the level and sent one up."""
    w, h = c.width, c.height
    out_x, out_y = (c.ndc_x(w // 2 + 0.5),) * 2, (c.ndc_y(h // 2 + 0.5),) * 2
    c.pair("step56", "left of the image", (-3.0, -2.0) + out_y, x0=0, x1=0)
    c.pair("step56", "right of the image", (2.0, 3.0) + out_y, x0=w - 1, x1=w - 1)
    c.pair("step56", "above the image", out_x + (2.0, 3.0), y0=0, y1=0)
    c.pair("step56", "below the image", out_x + (-3.0, -2.0), y0=h - 1, y1=h - 1)
    c.pair("step56", "far outside on every side", (-1000.0, 1000.0, -1000.0, 1000.0), x0=0, x1=w - 1, y0=0, y1=h - 1)
    c.pair("step56", "near the top of ndc reads the top rows", out_x + (c.ndc_y(min(1, h - 1) + 0.5), c.ndc_y(0.5)), y0=0, y1=min(1, h - 1))
    c.pair("step56", "near the bottom of ndc reads the bottom rows", out_x + (c.ndc_y(h - 0.5), c.ndc_y(max(h - 2, 0) + 0.5)), y0=max(h - 2, 0), y1=h - 1)
    c.pair("step7", "the whole image", c.pixels(0, w - 1, 0, h - 1), x0=0, x1=w - 1, y0=0, y1=h - 1)
    c.pair("step7", "one pixel: four times the same texel", c.pixels(w - 1, w - 1, h - 1, h - 1), x0=w - 1, x1=w - 1, y0=h - 1, y1=h - 1, k=0)
    c.pair("step8", "the last column and the last row", c.pixels(max(w - 2, 0), w - 1, max(h - 2, 0), h - 1), x1=w - 1, y1=h - 1, k=0)
    c.pair("step8", "the last column, every row", c.pixels(w - 1, w - 1, 0, h - 1), x0=w - 1, x1=w - 1, y0=0, y1=h - 1)
    c.pair("step8", "the last row, every column", c.pixels(0, w - 1, h - 1, h - 1), x0=0, x1=w - 1, y0=h - 1, y1=h - 1)

    def spans(extent):
        """{(k, kind): (p0, p1)}: pixel spans whose step-7 level is k — 'kept' with a texel difference of 1 at k (and 2 one
        level down), 'sent' with a difference of 2 at k - 1, the last place before the end of the image."""
        found = {}
        for p0 in range(extent):
            for p1 in range(p0, extent):
                k = 0
                while (p1 >> (k + 1)) - (p0 >> (k + 1)) > 1:
                    k += 1
                diff = (p1 >> (k + 1)) - (p0 >> (k + 1))
                kind = "kept" if diff == 1 else "flat"
                if k > 0 and (p1 >> k) - (p0 >> k) == 2:
                    kind = "sent"
                found[(k, kind)] = (p0, p1)  # (the last one found: near the end of the image)
                found.setdefault((k, kind, "first"), (p0, p1))
        return found

    sx, sy = spans(w), spans(h)
    one_x, one_y = (w // 3, w // 3), (h // 3, h // 3)
    for (key, (p0, p1)) in sorted(sx.items(), key=str):
        if key[1] != "flat":
            c.pair("step7", f"x alone decides: level {key[0]} {' '.join(key[1:])}", c.pixels(p0, p1, *one_y), x0=p0, x1=p1, k=key[0])
    for (key, (p0, p1)) in sorted(sy.items(), key=str):
        if key[1] != "flat":
            c.pair("step7", f"y alone decides: level {key[0]} {' '.join(key[1:])}", c.pixels(*one_x, p0, p1), y0=p0, y1=p1, k=key[0])
    for k in sorted({key[0] for key in sx} & {key[0] for key in sy}):
        for kind in ("kept", "sent"):
            if (k, kind) in sx and (k, kind) in sy:
                c.pair("step7", f"x and y decide: level {k} {kind}", c.pixels(*sx[(k, kind)], *sy[(k, kind)]), k=k)
    if w >= 5:  # the same width at two alignments
        c.pair("step7", "width 4 aligned: level 0", c.pixels(0, 3, *one_y), x0=0, x1=3, k=0)
        c.pair("step7", "width 4 one pixel on: level 1", c.pixels(1, 4, *one_y), x0=1, x1=4, k=1)
    if h >= 5:
        c.pair("step7", "height 4 aligned: level 0", c.pixels(*one_x, 0, 3), y0=0, y1=3, k=0)
        c.pair("step7", "height 4 one pixel on: level 1", c.pixels(*one_x, 1, 4), y0=1, y1=4, k=1)
    for j in range(12):  # ordinary rectangles all over the image
        a, b = sorted(c.rng.integers(0, w, 2))
        p, q = sorted(c.rng.integers(0, h, 2))
        c.pair("step8", f"rectangle {j}", c.pixels(a, b, p, q), x0=int(a), x1=int(b), y0=int(p), y1=int(q))


def _step9_members(c, x, y):
    """Step 9 on the level-0 texel of pixel (x, y), painted 0.5: zmin on d, beside d, and a thick box around d."""
    c.paint(x & ~1, y & ~1, c.value(0.5)[0], 2, 2)  # (the texel is not a cleared one)
    xy = c.pixels(x, x, y, y)
    c.add("step9", "zmin == d", xy, ("rel", 0), zmin_minus_d=0, occluded=False)
    c.add("step9", "zmin the float above d", xy, ("rel", 1), zmin_minus_d=1, occluded=True)
    c.add("step9", "zmin the float below d", xy, ("rel", -1), zmin_minus_d=-1, occluded=False)
    c.add("step9", "zmin below d, zmax above", xy, ("abs", 0.125, 0.875), occluded=False)


def _painted_texels(c, x_first, y):
    """Step 9 on level-0 texels painted whole: d == 1.0, the float below 1.0, negative, +0 (f32); 65535, 65534, 0, 1 (u16)."""
    fmt = c.fmt
    special = {"d == 1.0": 1.0, "d the float below 1.0": BELOW_ONE, "d negative": -0.25, "d == +0": 0.0} if fmt == "f32" else \
              {"d == 1.0 (65535)": 65535, "d == 65534 / 65535": 65534, "d == +0 (0)": 0, "d == 1 / 65535": 1}
    for j, (side, v) in enumerate(special.items()):
        x = x_first + 4 * j
        c.paint(x, y, np.uint16(v) if fmt == "u16" else F(v), 2, 2)
        if side == "d == +0":
            c.paint(x, y, F(-0.0))  # a -0 pixel beside +0 ones: the texel is +0
        value = F(v) / F(65535.0) if fmt == "u16" else F(v) + F(0)
        xy = c.pixels(x, x + 1, y, y + 1)
        if value == F(1.0):
            c.add("step9", side + ", zmin 2.0", xy, ("abs", 2.0, 2.0), d=value, k=0, occluded=False)
        else:
            c.add("step9", side + ", zmin == d", xy, ("rel", 0), d=value, k=0, zmin_minus_d=0, occluded=False)
            c.add("step9", side + ", zmin the float above", xy, ("rel", 1), d=value, k=0, zmin_minus_d=1, occluded=True)
            c.add("step9", side + ", zmin the float below", xy, ("rel", -1), d=value, k=0, zmin_minus_d=-1, occluded=False)
        if value == BELOW_ONE:
            c.add("step9", side + ", zmin 1.0", xy, ("abs", 1.0, 1.0), d=value, occluded=True)
        if value == F(0):
            c.add("step9", side + ", zmin -0", xy, ("abs", -0.0, -0.0), d=value, occluded=False)
            c.add("step9", side + ", zmin the smallest subnormal", xy, ("abs", U, U), d=value, occluded=True)


def _ortho64(variant):
    """64 x 64 under the orthographic pv: pixel positions are exact. variant 0 .. 3: the texel (variant & 1, variant >> 1) of
    the four holds the maximum of the step-8 members; variants 0 and 2 are f32 images, 1 and 3 u16."""
    fmt = "u16" if variant & 1 else "f32"
    c = _Case(f"ortho64_{fmt}_texel{variant}", 64, 64, fmt, pv_ortho(), 0x0CC0 + variant, plain=True)
    w = h = 64
    jx, jy = variant & 1, variant >> 1
    # the background stays at or below 0.75: the painted maxima are higher
    # ---- step 8: the maximum in texel (jx, jy) of the four, the other three lower ----
    for k, (x0, x1, y0, y1), high in ((0, (9, 10, 9, 10), 0.80), (2, (47, 55, 7, 15), 0.85), (3, (31, 47, 31, 47), 0.90), (4, (0, 63, 0, 63), 0.95)):
        s = k + 1
        tx, ty = (x0 >> s) + jx, (y0 >> s) + jy
        if k == 4:
            px, py = (2, 62)[jx], (2, 62)[jy]  # a corner pixel of the quadrant: in no other member's texels
        else:
            px, py = (tx << s) + (1 << s) // 2, (ty << s) + (1 << s) // 2
        assert px >> s == tx and py >> s == ty
        pixel, value = c.value(high)
        c.paint(px, py, pixel)
        c.pair("step8", f"level {k}: the maximum in texel ({jx}, {jy}) of the four", c.pixels(x0, x1, y0, y1), k=k, d=value, max_texel=(jx, jy))
    _step9_members(c, 40, 20)
    _step9_members(c, 5, 50)
    # ---- steps 5-6: u and v on, and one float either side of, a pixel boundary (boxes symmetric about 0: exact) ----
    rows = (c.ndc_y(30.5), c.ndc_y(12.5))
    cols = (c.ndc_x(12.5), c.ndc_x(30.5))
    for at in (40, 47, 63):
        for k, side in ((0, "on"), (-1, "one float below"), (1, "one float above")):
            target = _step(F(at), k)
            x = c.x_for_u(target)
            c.pair("step56", f"umax {side} {at}, umin mirrored", (-x, x) + rows, umax=target, x1=at - (k < 0), x0=w - at - (k > 0))
            y = c.y_for_v(target)
            c.pair("step56", f"vmax {side} {at}, vmin mirrored", cols + (y, -y), vmax=target, y1=at - (k < 0), y0=h - at - (k > 0))
    c.pair("step56", "u in (-1, 0): floor is -1, clamped to 0", (c.ndc_x(-0.5), c.ndc_x(20.5)) + rows, umin=F(-0.5), x0=0, x1=20)
    c.pair("step56", "v in (-1, 0): floor is -1, clamped to 0", cols + (c.ndc_y(20.5), c.ndc_y(-0.5)), vmin=F(-0.5), y0=0, y1=20)
    c.pair("step56", "umin == 0", (c.ndc_x(0), c.ndc_x(6.5)) + rows, umin=F(0), x0=0, x1=6)
    c.pair("step56", "umax == W - 1", (c.ndc_x(50.5), c.ndc_x(63)) + rows, umax=F(63), x1=63)
    c.pair("step56", "umax == W: clamped to W - 1", (c.ndc_x(50.5), c.ndc_x(64)) + rows, umax=F(64), x1=63)
    c.pair("step56", "vmin == 0", cols + (c.ndc_y(6.5), c.ndc_y(0)), vmin=F(0), y0=0, y1=6)
    c.pair("step56", "vmax == H - 1", cols + (c.ndc_y(63), c.ndc_y(50.5)), vmax=F(63), y1=63)
    c.pair("step56", "vmax == H: clamped to H - 1", cols + (c.ndc_y(64), c.ndc_y(50.5)), vmax=F(64), y1=63)
    c.pair("step56", "umax one pixel outside", (c.ndc_x(60.5), c.ndc_x(64.5)) + rows, x0=60, x1=63)
    c.pair("step56", "vmax one pixel outside", cols + (c.ndc_y(64.5), c.ndc_y(60.5)), y0=60, y1=63)
    _geometry_members(c)
    return c.finish(_ortho_filler)


def _small(width, height, fmt, seed):
    """Images whose levels have odd or rounded-up extents, under the orthographic pv (rectangles from pixel centres)."""
    c = _Case(f"ortho{width}x{height}_{fmt}", width, height, fmt, pv_ortho(), seed)
    _geometry_members(c)
    _step9_members(c, width - 1, height - 1)
    if width >= 40 and height >= 8:
        _painted_texels(c, 20, 2)
    _step9_members(c, 0, 0)
    return c.finish(_ortho_filler)


def _big(fmt):
    """The hand-written perspective pv_big on a 16 x 16 image whose left half is cleared: a finite positive clip.x lands on
    the last column (d < 1), so occluded == ok."""
    c = _Case(f"perspective_big_{fmt}", 16, 16, fmt, pv_big(), 0xB16, plain=True)
    c.depth[:, :8] = c.value(1.0)[0]
    xs = (-1.5, -1.25)   # clip.x = 0.5e38 .. 0.75e38: finite, u far right of the image
    flat = lambda v: (v, v)
    y0 = flat(0.0)
    for side, wv, ok in (("w == +0", F(0.0), False), ("w from z == -0", F(-0.0), False), ("w the smallest subnormal", U, True),
                         ("w the largest subnormal", SUB_MAX, True), ("w the smallest normal, u overflows to +inf", TINY, True),
                         ("w negative", F(-1.0), False), ("w == 1", F(1.0), True)):
        c.add("step3", side, xs + y0, ("abs", wv, wv), ok=ok, occluded=ok, w_is=wv, x0=15 if ok else None, x1=15 if ok else None)
    c.add("step3", "w negative on four corners, positive on four", xs + y0, ("abs", -1.0, 1.0), ok=False, occluded=False)
    c.add("step3", "subnormal w, clip.x == 0 on four corners: u is NaN there", (-2.0, -1.5) + y0, ("abs", U, U), ok=True, occluded=True, clip_x_has=F(0.0), x0=15, x1=15,
          y0=15, y1=0)  # (clip.y == 0 too: v is NaN on every corner, the fold's start values stand)
    c.add("step3", "clip.y == FLT_MAX exactly", (-0.5, -0.25) + flat(1.0), ("abs", 1.0, 1.0), ok=True, occluded=True, clip_y_has=FLT_MAX)
    c.add("step3", "clip.y == +inf", (-0.5, -0.25) + flat(np.nextafter(F(1.0), INF)), ("abs", 1.0, 1.0), ok=False, occluded=False, clip_y_has=INF)
    c.add("step3", "clip.x == +inf in the product", flat(4.0) + y0, ("abs", 1.0, 1.0), ok=False, occluded=False, clip_x_has=INF)
    c.add("step3", "clip.x == -inf in the product", flat(-8.0) + y0, ("abs", 1.0, 1.0), ok=False, occluded=False, clip_x_has=-INF)
    c.add("step3", "clip.x == NaN (inf - inf)", flat(4.0) + flat(4.0), ("abs", 1.0, 1.0), ok=False, occluded=False, clip_x_nan=True)
    c.add("step3", "clip.x overflows in the third addition only", flat(1.5) + y0, ("abs", 1.0, 1.0), ok=False, occluded=False, clip_x_has=INF, third_addition_only=True)
    c.add("step3", "clip.x stays finite in the third addition", flat(1.25) + y0, ("abs", 1.0, 1.0), ok=True, occluded=True, x0=15, x1=15)
    c.add("step3", "u from -inf to +inf: both clamps", (-3.0, -1.5) + y0, ("abs", TINY, TINY), ok=True, x0=0, x1=15, occluded=False)  # (reads a cleared column too)

    def filler(rng, n):
        return np.stack([rng.choice([-1.5, -2.5], n), np.zeros(n), rng.uniform(1.0, 2.0, n)], 1)

    return c.finish(filler)


def _default_perspective():
    """scene.default_pv() (w = z - 2) on a 16 x 8 f32 image of depth -1e30 with six cleared columns: a corner beside w == 0 has
    an enormous negative ndc.z, which still lies behind -1e30."""
    c = _Case("perspective_default", 16, 8, "f32", scene_mod.default_pv(), 0xDEF)
    c.depth[:, :] = F(-1e30)
    c.depth[:, :6] = 1.0
    xs, ys = (0.5, 1.0), (1.5, 2.0)   # right of and above the camera: the last column, the first row
    for side, z, ok in (("w == 0", F(2.0), False), ("w one step negative", _step(F(2.0), -1), False), ("w one step positive", _step(F(2.0), 1), True),
                        ("w == 1", F(3.0), True)):
        c.add("step3", side, xs + ys, ("abs", z, z), ok=ok, occluded=ok, w_is=F(z - F(2.0)), x0=15 if z < 2.5 and ok else None, y0=0 if z < 2.5 and ok else None)
    c.add("step3", "w negative behind the camera", xs + ys, ("abs", -3.0, -2.0), ok=False, occluded=False)
    c.add("step3", "the box straddles the camera plane", xs + ys, ("abs", 0.0, 4.0), ok=False, occluded=False)
    c.add("step9", "d negative, zmin above it", (-0.25, 0.25, 0.75, 1.25), ("abs", 6.0, 7.0), ok=True, occluded=True, d=F(-1e30))

    def filler(rng, n):
        return np.stack([rng.uniform(-8, 8, n), rng.uniform(-2, 4, n), rng.uniform(5, 30, n)], 1)

    return c.finish(filler)


def pv_shear(corner):
    """The orthographic pv with clip.z = +-x/8 +- y/8 +- z/4 + 0.5 (w == 1, every term a dyadic number): the corner that holds
    the smallest ndc.z of ANY box is `corner` (bit 0: the maximum on x, bit 1: on y, bit 2: on z)."""
    m = pv_ortho().copy()
    m[2] = -0.125 if corner & 1 else 0.125
    m[6] = -0.125 if corner & 2 else 0.125
    m[10] = -0.25 if corner & 4 else 0.25
    m[14] = 0.5
    return m


def _corner(corner):
    """zmin taken from one corner in turn: boxes (found by search over coarse dyadic ones) whose d lies between the smallest
    ndc.z and the next one — a fold that misses that corner calls them occluded — and boxes wholly behind d."""
    fmt = "u16" if corner & 1 else "f32"
    c = _Case(f"corner{corner}_{fmt}", 32, 32, fmt, pv_shear(corner), 0xC0 + corner, plain=True)
    rng = c.rng
    n = 4000
    cen = np.round(rng.uniform(-1.0, 1.0, (n, 3)) * 64) / 64
    half = np.round(rng.uniform(0.02, 0.3, (n, 3)) * 64) / 64
    b = np.concatenate([cen - half, cen + half], 1).astype(F)
    t = occ.occlusion_terms(b, c.pv, occ.pyramid_levels(c.depth), c.width, c.height)
    nz = np.sort(corner_clips(b, c.pv)[:, :, 2], axis=1)
    between = np.nonzero((nz[:, 0] <= t["d"]) & (t["d"] < nz[:, 1]))[0]
    behind = np.nonzero(t["d"] < nz[:, 0])[0]
    assert len(between) >= 8 and len(behind) >= 8, (corner, len(between), len(behind))
    for i in between[:8]:
        c.add("step9", f"zmin from corner {corner} alone, d below every other corner", tuple(b[i, [0, 3, 1, 4]]), ("abs", b[i, 2], b[i, 5]),
              zmin_corner=corner, occluded=False)
    for i in behind[:8]:
        c.add("step9", f"zmin from corner {corner}, every corner behind d", tuple(b[i, [0, 3, 1, 4]]), ("abs", b[i, 2], b[i, 5]), zmin_corner=corner, occluded=True)

    def filler(rng, n):
        return np.stack([rng.uniform(-1.1, 1.1, n), rng.uniform(-1.1, 1.1, n), rng.uniform(-1.5, 1.5, n)], 1)

    return c.finish(filler)


SMALL_IMAGES = ((5, 3, "f32"), (53, 37, "u16"), (65, 64, "f32"), (1, 9, "u16"), (9, 1, "f32"), (1, 1, "u16"), (1, 1, "f32"))
_BUILDERS = {f"ortho64_{'u16' if v & 1 else 'f32'}_texel{v}": functools.partial(_ortho64, v) for v in range(4)}
_BUILDERS.update({f"ortho{w}x{h}_{f}": functools.partial(_small, w, h, f, 0x5A11 + 131 * w + h) for w, h, f in SMALL_IMAGES})
_BUILDERS["perspective_big_f32"] = functools.partial(_big, "f32")
_BUILDERS["perspective_big_u16"] = functools.partial(_big, "u16")
_BUILDERS["perspective_default"] = _default_perspective
_BUILDERS.update({f"corner{j}_{'u16' if j & 1 else 'f32'}": functools.partial(_corner, j) for j in range(8)})
NAMES = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    return _BUILDERS[name]()


def scene_of(c):
    return {k: c[k] for k in ("n", "pos", "rot", "scale", "mesh_id", "meshes", "planes", "cam_pos")}


def describe(c, i):
    """The label of instance i of a case, for a failure message."""
    for l in c["labels"]:
        if l["index"] == int(i):
            return f"instance {i} [{l['cls']}: {l['side']}]"
    return f"instance {i} [an ordinary box]"


def _same(a, b):
    a, b = F(a), F(b)
    return (np.isnan(a) and np.isnan(b)) or (a == b and np.signbit(a) == np.signbit(b))


def verify(c, boxes=None):
    """Every label of a case against occlusion_terms over `boxes` (default: the boxes the case was built with; the GPU test
    passes the oracle's world_aabb). Returns the list of failures as strings."""
    boxes = c["boxes"] if boxes is None else np.asarray(boxes, F).reshape(-1, 6)
    levels = occ.pyramid_levels(c["depth"])
    idx = np.array([l["index"] for l in c["labels"]], np.int64)
    t = occ.occlusion_terms(boxes[idx], c["pv"], levels, c["width"], c["height"])
    clips = corner_clips(boxes[idx], c["pv"])
    bad = []
    for j, l in enumerate(c["labels"]):
        for key, want in l["check"].items():
            if want is None:
                continue
            if key in occ.TERMS:
                got = t[key][j]
                good = _same(got, want) if isinstance(got, np.floating) else got == want
            elif key == "zmin_minus_d":
                got = t["zmin"][j]
                good = _same(got, _step(t["d"][j], want)) or (want == 0 and got == t["d"][j])
            elif key == "max_texel":
                s = int(t["k"][j]) + 1
                lvl = levels[int(t["k"][j])]
                four = {(a, b): lvl[(int(t["y0"][j]) >> s) + b, (int(t["x0"][j]) >> s) + a] for a in (0, 1) for b in (0, 1)}
                got = max(four, key=four.get)
                good = got == tuple(want) and sorted(four.values())[-1] > sorted(four.values())[-2] and \
                    (int(t["x1"][j]) >> s) - (int(t["x0"][j]) >> s) == 1 and (int(t["y1"][j]) >> s) - (int(t["y0"][j]) >> s) == 1
            elif key == "zmin_corner":
                nz = clips[j, :, 2] * (F(1.0) / clips[j, :, 3])
                got = int(np.argmin(nz))
                good = got == want and np.sort(nz)[1] > nz[got] == t["zmin"][j] and (t["occluded"][j] or np.sort(nz)[1] > t["d"][j] >= nz[got])
            elif key == "w_is":
                got = clips[j, :, 3]
                good = all(_same(g, want) or (want == 0 and g == 0) for g in got)
            elif key in ("clip_x_has", "clip_y_has"):
                got = clips[j, :, 0 if key == "clip_x_has" else 1]
                good = any(_same(g, want) for g in got)
            elif key == "clip_x_nan":
                got = clips[j, :, 0]
                good = bool(np.isnan(got).any())
            elif key == "third_addition_only":
                b, m = boxes[idx[j]], c["pv"]
                with np.errstate(all="ignore"):
                    got = [(m[0] * x + m[4] * y) + m[8] * z for x in (b[0], b[3]) for y in (b[1], b[4]) for z in (b[2], b[5])]
                good = bool(np.isfinite(got).all()) and bool(np.isinf(clips[j, :, 0]).all())
            else:
                raise KeyError(key)
            if not good:
                bad.append(f"{c['name']}: {describe(c, l['index'])}: {key} is {got!r}, built to be {want!r}")
    return bad


# ---- depth images on the shape edges of mip_depth_pyramid_kernel ----
# (width, height, format, pitch in elements). The kernel works in 64 x 64-pixel blocks: one block returns early, several
# blocks hand levels 6.. to the workgroup that finishes last, which reduces level 5 in LDS when w5 * h5 <= 4096 and
# w6 * h6 <= 1024 and level by level through memory otherwise; a row is read in 16-byte loads (8 u16 / 4 f32 pixels) where the
# pitch and the width allow and pixel by pixel in the tail.

def _pitches(width, fmt):
    """A pitch that keeps every row 16-byte aligned and one that does not (elements)."""
    per16 = 8 if fmt == "u16" else 4
    aligned = -(-width // per16) * per16
    return aligned, aligned + 1


def pyramid_shapes():
    shapes = []
    for w in (63, 64, 65):                      # block count and the early return
        for h in (1, 63, 64, 65):
            shapes += [(w, h, f, w) for f in ("u16", "f32")]
    shapes += [(w, 3, f, w) for w in (127, 128, 129) for f in ("u16", "f32")]
    for fmt, step in (("u16", 8), ("f32", 4)):  # load tails around 64 and 128
        for centre in (64, 128):
            for w in (centre - step - 1, centre - step + 1, centre - 1, centre + 1, centre + step - 1, centre + step + 1):
                shapes += [(w, 5, fmt, p) for p in _pitches(w, fmt)]
    shapes += [(64, 5, "u16", 64), (64, 5, "u16", 65), (128, 5, "f32", 128), (128, 5, "f32", 129)]  # (no tail at all)
    # the LDS / memory branch of the last workgroup: one format each (16 M pixels)
    shapes += [(4096, 4096, "u16", 4096), (4097, 4096, "u16", 4097), (4096, 4097, "u16", 4096), (1088, 15360, "u16", 1088),
               (16384, 1, "f32", 16384), (1, 16384, "f32", 1), (16384, 1, "u16", 16384), (1, 16384, "u16", 1)]
    return shapes


def pyramid_structure(width, height, fmt, pitch):
    """The path mip_depth_pyramid_kernel takes for a shape, from renderer_amd.pipeline.depth_pyramid_layout (never from the
    kernel): a set of class names."""
    from renderer_amd.pipeline import depth_pyramid_layout

    sizes = depth_pyramid_layout(width, height)["sizes"]
    blocks = -(-width // 64) * -(-height // 64)
    out = set()
    if len(sizes) <= 6:
        assert blocks == 1
        out.add("one block, early return")
    else:
        out.add("one block, levels above 5" if blocks == 1 else "several blocks, the last one finishes")
        first = sizes[5][0] * sizes[5][1] <= 4096
        second = sizes[6][0] * sizes[6][1] <= 1024
        out.add("top in LDS" if first and second else "top through memory")
        if first and second and sizes[5][0] * sizes[5][1] == 4096:
            out.add("top in LDS, level 5 exactly 4096 texels")
        if first and not second:
            out.add("top through memory by the second clause alone")
        if not first:
            out.add("top through memory by the first clause")
    per16, size = (8, 2) if fmt == "u16" else (4, 4)
    vec = (pitch * size) % 16 == 0
    out.add(f"{fmt}: 16-byte loads" if vec and width >= per16 else f"{fmt}: no 16-byte loads")
    if vec and width % per16:
        out.add(f"{fmt}: 16-byte loads with a tail")
    if vec and width % per16 == 0:
        out.add(f"{fmt}: 16-byte loads, no tail")
    if not vec:
        out.add(f"{fmt}: pitch not a multiple of 16 bytes")
    return out


PYRAMID_CLASSES = ("one block, early return", "several blocks, the last one finishes", "top in LDS", "top through memory",
                   "top in LDS, level 5 exactly 4096 texels", "top through memory by the second clause alone",
                   "top through memory by the first clause") + tuple(f"{f}: {t}" for f in ("u16", "f32") for t in (
                       "16-byte loads with a tail", "16-byte loads, no tail", "pitch not a multiple of 16 bytes"))
