"""numpy float32 restatement of the occlusion-culling EXTENSION (include/mi_instance_pipeline.h, MipOcclusion): the depth
pyramid, the occlusion test in the header's operation order, and the outputs mip_run_occluded owes — derived from the
oracle's frustum-only frame. Not reference behaviour: the reference renders the depth but culls nothing against it, so
parity here is with this restatement only."""
import numpy as np

F32 = np.float32
FLT_MAX = F32(3.4028234663852886e38)


def pyramid_levels(depth):
    """The max pyramid of a depth image (H x W, uint16 = D16_UNORM or float32 = D32_SFLOAT): a list of float32 levels
    (level 0 = ceil(W/2) x ceil(H/2) ... 1 x 1). u16 v counts as float32(v) / 65535 (correctly rounded), NaN as 1.0, a zero as +0."""
    depth = np.asarray(depth)
    if depth.dtype == np.uint16:
        px = depth.astype(F32) / F32(65535.0)
    else:
        px = depth.astype(F32)
        px = np.where(np.isnan(px), F32(1.0), px) + F32(0.0)
    levels = []
    cur = px
    while True:
        h, w = cur.shape
        ph, pw = h + (h & 1), w + (w & 1)
        pad = np.full((ph, pw), -np.inf, F32)
        pad[:h, :w] = cur
        cur = pad.reshape(ph // 2, 2, pw // 2, 2).max(axis=(1, 3))
        levels.append(cur)
        if cur.shape == (1, 1):
            return levels


def pyramid_flat(levels):
    return np.concatenate([l.reshape(-1) for l in levels]).astype(F32)


TERMS = ("ok", "umin", "umax", "vmin", "vmax", "zmin", "x0", "x1", "y0", "y1", "k", "d", "occluded")


def occlusion_terms(world_aabb, pv, levels, width, height):
    """Steps 1-9 of the header's test for every box (n x 6: min xyz, max xyz), every intermediate term kept: a dict of TERMS —
    ok (step 3), umin .. vmax and zmin (steps 4-5), x0 .. y1 (step 6), k (step 7), d (step 8), occluded (step 9). Same float32
    operations in the same order as the kernel; min / max fold like C fminf / fmaxf (a NaN operand is ignored)."""
    b = np.asarray(world_aabb, F32).reshape(-1, 6)
    m = np.asarray(pv, F32).reshape(16)
    wf, hf = F32(width), F32(height)
    n = b.shape[0]
    ok = np.ones(n, bool)
    umin = np.full(n, np.inf, F32)
    umax = np.full(n, -np.inf, F32)
    vmin = np.full(n, np.inf, F32)
    vmax = np.full(n, -np.inf, F32)
    zmin = np.full(n, np.inf, F32)
    with np.errstate(all="ignore"):
        for c in range(8):
            x = b[:, 3] if c & 1 else b[:, 0]
            y = b[:, 4] if c & 2 else b[:, 1]
            z = b[:, 5] if c & 4 else b[:, 2]
            clip = [((m[r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r] for r in range(4)]
            ok &= np.isfinite(clip[0]) & np.isfinite(clip[1]) & np.isfinite(clip[2]) & np.isfinite(clip[3]) & (clip[3] > F32(0))
            rw = F32(1.0) / clip[3]
            nx, ny, nz = clip[0] * rw, clip[1] * rw, clip[2] * rw
            u = (nx * F32(0.5) + F32(0.5)) * wf
            v = (F32(0.5) - ny * F32(0.5)) * hf
            umin, umax = np.fmin(umin, u), np.fmax(umax, u)
            vmin, vmax = np.fmin(vmin, v), np.fmax(vmax, v)
            zmin = np.fmin(zmin, nz)
        clamp = lambda a, hi: np.fmin(np.fmax(np.floor(a), F32(0)), F32(hi - 1)).astype(np.int64)
        x0, x1, y0, y1 = clamp(umin, width), clamp(umax, width), clamp(vmin, height), clamp(vmax, height)
    k = np.zeros(n, np.int64)
    while True:
        more = ((x1 >> (k + 1)) - (x0 >> (k + 1)) > 1) | ((y1 >> (k + 1)) - (y0 >> (k + 1)) > 1)
        if not more.any():
            break
        k += more
    d = np.empty(n, F32)
    for lvl in np.unique(k):
        sel = k == lvl
        t = levels[lvl]
        s = int(lvl) + 1
        tx0, tx1, ty0, ty1 = x0[sel] >> s, x1[sel] >> s, y0[sel] >> s, y1[sel] >> s
        d[sel] = np.fmax(np.fmax(t[ty0, tx0], t[ty0, tx1]), np.fmax(t[ty1, tx0], t[ty1, tx1]))
    result = ok & (d < F32(1.0)) & (zmin > d)
    return dict(ok=ok, umin=umin, umax=umax, vmin=vmin, vmax=vmax, zmin=zmin, x0=x0, x1=x1, y0=y0, y1=y1, k=k, d=d, occluded=result)


def occluded(world_aabb, pv, levels, width, height):
    """Step 9's answer for every box: True = occluded by the pyramid (the frustum test and the candidate set are the caller's)."""
    return occlusion_terms(world_aabb, pv, levels, width, height)["occluded"]


def bits_of(bitmap, n):
    """bit i of a u32 bitmap as a bool array of n."""
    w = np.asarray(bitmap, np.uint32)
    return ((w[np.arange(n) >> 5] >> (np.arange(n) & 31).astype(np.uint32)) & 1).astype(bool)


def bitmap_of(mask):
    mask = np.asarray(mask, bool)
    words = np.zeros((len(mask) + 31) // 32, np.uint32)
    idx = np.nonzero(mask)[0]
    np.bitwise_or.at(words, idx >> 5, (np.uint32(1) << (idx & 31).astype(np.uint32)))
    return words


def expected(want, n, pv, levels, width, height, candidates=None, inverted=False, first_instance_base=0, first_index_base=0):
    """What mip_run_occluded owes, from the oracle's frustum-only frame `want` (visible_bitmap, world_aabb, draw_cmds of the
    same scene and frame): the non-candidates and the occluded instances culled, their commands removed, firstIndex recomputed
    as first_index_base + the exclusive running sum of indexCount (wrapping u32)."""
    in_frustum = bits_of(want["visible_bitmap"], n)
    cand = np.ones(n, bool) if candidates is None else bits_of(candidates, n) ^ bool(inverted)
    test = in_frustum & cand
    occ = np.zeros(n, bool)
    if test.any():
        occ[test] = occluded(np.asarray(want["world_aabb"]).reshape(-1, 6)[test], pv, levels, width, height)
    visible = test & ~occ
    cmds = want["draw_cmds"][: want["draw_count"]]
    inst = (cmds["firstInstance"].astype(np.int64) - first_instance_base) & 0xFFFFFFFF
    kept = cmds[visible[inst]].copy()
    counts = kept["indexCount"].astype(np.uint64)
    excl = np.concatenate([np.zeros(1, np.uint64), np.cumsum(counts, dtype=np.uint64)[:-1]])[: len(kept)]
    kept["firstIndex"] = ((excl + np.uint64(first_index_base)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return {
        "visible_bitmap": bitmap_of(visible),
        "occluded_bitmap": bitmap_of(occ),
        "draw_cmds": kept,
        "draw_count": int(len(kept)),
        "draw_index_total": int((int(counts.sum()) + 0) & 0xFFFFFFFF),
        "occluded": occ,
        "visible": visible,
        "in_frustum": in_frustum,
    }
