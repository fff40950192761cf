"""numpy restatement of cluster culling with normal cones (include/mi_instance_pipeline.h, mip_build_cluster_cones /
mip_cull_clusters_cone / mip_cull_cluster_triangles_cone), written from the header's text: the cone table operation by
operation in float32, the view's eye and facing in float64, CONE_CULLED, and SURVIVES_CONE in SURVIVES' place of the plain
calls' restatements (tests/cluster_restatement.py, tests/cluster_triangle_restatement.py), which supply everything else.
Also the two properties the scenes are held to: (a) conservative in float64, (b) agreement with the per-triangle stage.
Not reference behaviour: this file is what the library is checked against."""
import numpy as np

import cluster_restatement as cr
import cluster_triangle_restatement as ctr
import numpy_restatement as nr

F = np.float32
K_MARGIN = F(2.0 ** -7)      # on k, absolute
R_MARGIN = F(2.0 ** -7)      # on r, relative
SPREAD_LIMIT = F(0.1)
GUARD_QUAT = F(2.0 ** -20)
ERR_INVALID = -1
NO_CONE = np.array([0, 0, 0, np.inf, 0, 0, 0, 0], F)


def _cluster_corners(meshes, vertices, indices):
    """[(table index g, corners (t, 3, 3) float32)] of every cluster, bucket-major."""
    t = cr.cluster_table(meshes)
    vertices = np.asarray(vertices, F).reshape(-1, 3)
    indices = np.asarray(indices, np.uint32).reshape(-1)
    for b in range(len(t["mesh"])):
        k, l = int(t["mesh"][b]), int(t["lod"][b])
        off, tris = int(meshes["index_offset"][k, l]), int(t["T"][b])
        if tris == 0:
            continue
        corners = vertices[indices[off : off + 3 * tris].astype(np.int64) + int(meshes["vertex_offset"][k])].reshape(tris, 3, 3)
        for c in range(int(t["C"][b])):
            yield int(t["base"][b]) + c, corners[cr.CLUSTER_TRIANGLES * c : cr.CLUSTER_TRIANGLES * (c + 1)]


def _butterfly_sum(v):
    """64 float32 slots: level j replaces v[l] by v[l] + v[l xor 2^j]."""
    lanes = np.arange(64)
    for j in range(6):
        v = v + v[lanes ^ (1 << j)]
    return v[0]


def cluster_cones(meshes, vertices, indices, boxes=None):
    """(total clusters, 8) float32, bucket-major: {axis xyz, k, centre xyz, r}; NO CONE is {0, 0, 0, +inf, 0, 0, 0, 0}."""
    boxes = cr.cluster_boxes(meshes, vertices, indices) if boxes is None else np.asarray(boxes, F).reshape(-1, 6)
    out = np.tile(NO_CONE, (len(boxes), 1))
    two = F(2.0)
    with np.errstate(all="ignore"):
        for g, v in _cluster_corners(meshes, vertices, indices):
            e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
            n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                          e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
            len2 = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
            proper = (len2 > 0) & (len2 < np.inf)
            if not proper.all():
                continue
            nh = n / np.sqrt(len2)[:, None]
            slots = np.zeros((64, 3), F)
            slots[: len(nh)] = nh
            a_sum = np.array([_butterfly_sum(slots[:, ax]) for ax in range(3)], F)
            aa = (a_sum[0] * a_sum[0] + a_sum[1] * a_sum[1]) + a_sum[2] * a_sum[2]
            if not (aa > 0 and aa < np.inf):
                continue
            a = a_sum / np.sqrt(aa)
            m = ((nh[:, 0] * a[0] + nh[:, 1] * a[1]) + nh[:, 2] * a[2]).min()
            if not m > SPREAD_LIMIT:
                continue
            k = np.sqrt(np.fmax(F(1.0) - m * m, F(0.0))) + K_MARGIN
            lo, hi = boxes[g, :3], boxes[g, 3:]
            h = (hi - lo) / two
            r0 = np.sqrt((h[0] * h[0] + h[1] * h[1]) + h[2] * h[2])
            out[g] = np.concatenate([a, [k], (hi + lo) / two, [r0 + r0 * R_MARGIN]]).astype(F)
    return out


def cone_from_pv(pv):
    """mip_cone_from_pv: (status, eye float32[3], facing) — rows x, y, w of pv as [A | b], e = -A^-1 b, facing = sign(det A), in
    float64, rounded once. A different formula from the library's adjugate on purpose: the test compares the rounded results."""
    m = np.asarray(pv, F).reshape(4, 4).T.astype(np.float64)          # column-major storage -> m[row][col]
    a, b = m[[0, 1, 3], :3], m[[0, 1, 3], 3]
    with np.errstate(all="ignore"):
        det = np.linalg.det(a) if np.isfinite(a).all() else np.nan
        if not np.isfinite(det) or det == 0.0 or np.linalg.matrix_rank(a) < 3:
            return ERR_INVALID, None, None
        e = (-np.linalg.solve(a, b)).astype(F)
    if not np.isfinite(e).all():
        return ERR_INVALID, None, None
    return 0, e, 1.0 if det > 0 else -1.0


def rotation_times_scale(rot, scale):
    """M[n, r, c] = R[r][c] x s in float32: R is numpy_restatement.model_matrices' rotation chain."""
    i, j, k, w = (np.asarray(rot, F).reshape(-1, 4)[:, c] for c in range(4))
    s = np.asarray(scale, F).reshape(-1)
    two = F(2.0)
    with np.errstate(all="ignore"):
        ww, ii, jj, kk = w * w, i * i, j * j, k * k
        ij, wk, wj = i * j * two, w * k * two, w * j * two
        ik, jk, wi = i * k * two, j * k * two, w * i * two
        rows = [[ww + ii - jj - kk, ij - wk, wj + ik], [wk + ij, ww - ii + jj - kk, jk - wi], [ik - wj, wi + jk, ww - ii - jj + kk]]
        return np.stack([np.stack([rows[r][c] * s for c in range(3)], axis=1) for r in range(3)], axis=1)


def cone_terms(items, cones, pos, rot, scale, eye, facing):
    """Av, Bv and the GUARD of every work item (float32, float32, bool): the header's chain."""
    i = items["inst"]
    cone = np.asarray(cones, F).reshape(-1, 8)[items["box_index"]]
    p = np.asarray(pos, F).reshape(-1, 3)[i]
    q = np.asarray(rot, F).reshape(-1, 4)[i]
    s = np.asarray(scale, F).reshape(-1)[i]
    eye = np.asarray(eye, F).reshape(3)
    f = F(facing)
    with np.errstate(all="ignore"):
        qq = ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3]
        guard = (s > 0) & (np.abs(qq - F(1.0)) <= GUARD_QUAT)
        m = rotation_times_scale(q, s)
        a, k, c, r = cone[:, :3], cone[:, 3], cone[:, 4:7], cone[:, 7]
        cw = np.stack([((m[:, x, 0] * c[:, 0] + m[:, x, 1] * c[:, 1]) + m[:, x, 2] * c[:, 2]) + p[:, x] for x in range(3)], axis=1)
        aw = np.stack([(m[:, x, 0] * a[:, 0] + m[:, x, 1] * a[:, 1]) + m[:, x, 2] * a[:, 2] for x in range(3)], axis=1)
        d = cw - eye[None, :]
        da = (d[:, 0] * aw[:, 0] + d[:, 1] * aw[:, 1]) + d[:, 2] * aw[:, 2]
        dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        av = f * da - (s * s) * r
        sk = s * k
        bv = (sk * sk) * dd
    return av, bv, guard


def cone_culled(items, cones, pos, rot, scale, eye, facing):
    if len(items["inst"]) == 0:
        return np.zeros(0, bool)
    av, bv, guard = cone_terms(items, cones, pos, rot, scale, eye, facing)
    with np.errstate(all="ignore"):
        return guard & (av > 0) & (av * av > bv) & np.isfinite(av) & np.isfinite(bv)


def _with_cone(s, cones, eye, facing, call):
    """Runs a plain restatement with SURVIVES_CONE in SURVIVES' place; returns its result with `cone_culled` per work item."""
    plain = cr.survives
    seen = {}

    def survives_cone(items, boxes, pos, rot, scale, planes, occlusion=None):
        cc = cone_culled(items, cones, pos, rot, scale, eye, facing)
        seen["cone_culled"] = cc
        return plain(items, boxes, pos, rot, scale, planes, occlusion) & ~cc

    cr.survives = survives_cone
    try:
        out = call()
    finally:
        cr.survives = plain
    out["cone_culled"] = seen.get("cone_culled")
    return out


def cull_clusters_cone(s, boxes, cones, eye, facing, visible_bitmap, mode, switch_sq, cmd_capacity, work_capacity=0, first_instance_base=0, occlusion=None):
    """What mip_cull_clusters_cone owes: cluster_restatement.cull_clusters' dict, and cone_culled per work item."""
    return _with_cone(s, cones, eye, facing, lambda: cr.cull_clusters(s, boxes, visible_bitmap, mode, switch_sq, cmd_capacity, work_capacity,
                                                                      first_instance_base, occlusion))


def cull_cluster_triangles_cone(s, boxes, cones, eye, facing, vertices, indices, visible_bitmap, mode, switch_sq, pv, cmd_capacity, index_capacity,
                                work_capacity=0, first_instance_base=0, occlusion=None):
    """What mip_cull_cluster_triangles_cone owes: cluster_triangle_restatement.cull_cluster_triangles' dict, and cone_culled."""
    return _with_cone(s, cones, eye, facing, lambda: ctr.cull_cluster_triangles(s, boxes, vertices, indices, visible_bitmap, mode, switch_sq, pv,
                                                                                cmd_capacity, index_capacity, work_capacity, first_instance_base,
                                                                                occlusion))


def waves_skipped(survive_before_box, w):
    """Waves (64 consecutive work items) in which the cone leaves no item: the ones the cull kernel answers without a box."""
    alive = np.zeros((w + 63) // 64 * 64, bool)
    alive[:w] = survive_before_box
    return int((~alive.reshape(-1, 64).any(axis=1)).sum())


# ---- the two properties of the scenes ----

def _item_triangles(s, items, vertices, indices, which):
    """Model-space corners (t, 3, 3) of work item `which`'s cluster, and its instance."""
    t = items["table"]
    i, c = int(items["inst"][which]), int(items["cluster"][which])
    b = int(items["bucket"][i])
    k, l, tris = int(t["mesh"][b]), int(t["lod"][b]), int(t["T"][b])
    off = int(s["meshes"]["index_offset"][k, l])
    first, last = cr.CLUSTER_TRIANGLES * c, min(cr.CLUSTER_TRIANGLES * (c + 1), tris)
    ix = np.asarray(indices, np.uint32).reshape(-1)[off + 3 * first : off + 3 * last].reshape(-1, 3)
    return np.asarray(vertices, F).reshape(-1, 3)[ix.astype(np.int64) + int(s["meshes"]["vertex_offset"][k])], i


def property_violations(s, items, culled, vertices, indices, eye, facing, pv=None):
    """(a): the cone-culled items with a triangle whose facing x n_t . (x0 - e) is < 0 in float64 — world corners = the float32
    model matrix mip_run writes applied in float64 to the float32 vertices. (b), with pv: the cone-culled items with a triangle
    numpy_restatement.triangle_culled does not cull. Returns (violations of a, violations of b, items checked)."""
    pos, rot, scale = np.asarray(s["pos"], F).reshape(-1, 3), np.asarray(s["rot"], F).reshape(-1, 4), np.asarray(s["scale"], F).reshape(-1)
    e = np.asarray(eye, F).reshape(3).astype(np.float64)
    bad_a = bad_b = 0
    which = np.nonzero(culled)[0]
    for w in which:
        v, i = _item_triangles(s, items, vertices, indices, w)
        model = nr.model_matrices(pos[i : i + 1], rot[i : i + 1], scale[i : i + 1])[0]
        m = model.astype(np.float64).reshape(4, 4).T                     # m[row][col]
        x = v.astype(np.float64) @ m[:3, :3].T + m[:3, 3]
        n = np.cross(x[:, 1] - x[:, 0], x[:, 2] - x[:, 0])
        side = float(facing) * np.einsum("ij,ij->i", n, x[:, 0] - e)
        bad_a += int((side < 0).any())
        if pv is not None:
            bad_b += int((~nr.triangle_culled(model, pv, v)).any())
    return bad_a, bad_b, len(which)


def in_domain(s, items, cones, vertices, indices):
    """Whether every work item that has a cone lies inside the margin's domain (the header's two conditions)."""
    i = items["inst"]
    cone = np.asarray(cones, F).reshape(-1, 8)[items["box_index"]].astype(np.float64)
    has = np.isfinite(cone[:, 3])
    sc = np.asarray(s["scale"], F).reshape(-1)[i].astype(np.float64)
    p = np.abs(np.asarray(s["pos"], F).reshape(-1, 3)[i].astype(np.float64)).max(axis=1)
    c = np.abs(cone[:, 4:7]).max(axis=1) * sc
    ok = ~has | (np.maximum(p, c) <= 2.0 ** 12 * sc * cone[:, 7])
    shapes = True
    for g, v in _cluster_corners(s["meshes"], vertices, indices):
        v = v.astype(np.float64)
        e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
        n = np.cross(e1, e2)
        if np.isfinite(np.asarray(cones, F).reshape(-1, 8)[g, 3]):
            shapes &= bool(((n * n).sum(1) >= 2.0 ** -10 * (e1 * e1).sum(1) * (e2 * e2).sum(1)).all())
    return bool(ok.all()) and shapes
