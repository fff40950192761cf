"""A second, independent restatement of the reference path in vectorised numpy float32 (one
rounding per elementwise op, no FMA), used only to cross-check the C oracle: same written
operation order, different language, compiler and code shape."""
import numpy as np

F = np.float32


def _gemm(a, b):
    """nalgebra static gemm: out[:,c] = a[:,0]*b[0,c]; then += a[:,k]*b[k,c] (k = 1..3).
    a, b: dict[(r,c)] -> array."""
    out = {}
    for c in range(4):
        for r in range(4):
            y = a[(r, 0)] * b[(0, c)]
            for k in range(1, 4):
                y = a[(r, k)] * b[(k, c)] + y
            out[(r, c)] = y
    return out


def model_matrices(pos, rot, scale):
    n = len(scale)
    i, j, k, w = (rot[:, c].astype(F) for c in range(4))
    two = F(2.0)
    with np.errstate(all="ignore"):
        ww, ii, jj, kk = w * w, i * i, j * j, k * k
        ij, wk, wj = i * j * two, w * k * two, w * j * two
        ik, jk, wi = i * k * two, j * k * two, w * i * two
    zero, one = np.zeros(n, F), np.ones(n, F)
    with np.errstate(all="ignore"):
      R = {(0, 0): ww + ii - jj - kk, (0, 1): ij - wk, (0, 2): wj + ik,
         (1, 0): wk + ij, (1, 1): ww - ii + jj - kk, (1, 2): jk - wi,
         (2, 0): ik - wj, (2, 1): wi + jk, (2, 2): ww - ii - jj + kk}
    Rh = {(r, c): (R[(r, c)] if r < 3 and c < 3 else (one if r == c else zero)) for r in range(4) for c in range(4)}
    T = {(r, c): (one if r == c else zero) for r in range(4) for c in range(4)}
    for r in range(3):
        T[(r, 3)] = pos[:, r].astype(F)
    S = {(r, c): zero for r in range(4) for c in range(4)}
    for d in range(3):
        S[(d, d)] = scale.astype(F)
    S[(3, 3)] = one
    with np.errstate(all="ignore"):
        M = _gemm(_gemm(T, Rh), S)
    out = np.empty((n, 16), F)
    for c in range(4):
        for r in range(4):
            out[:, c * 4 + r] = M[(r, c)]
    return out


def world_aabbs(model, mesh_min, mesh_max):
    """model (n,16) column-major; mesh_min/max (n,3) per instance."""
    n = len(model)
    big = F(3.40282347e38)
    lo = np.full((n, 3), big, F)
    hi = np.full((n, 3), -big, F)
    sel = [(0, 0, 0), (1, 0, 0), (0, 0, 1), (1, 0, 1), (0, 1, 0), (1, 1, 0), (0, 1, 1), (1, 1, 1)]  # (x,y,z) picks
    with np.errstate(all="ignore"):
        for sx, sy, sz in sel:
            x = np.where(sx, mesh_max[:, 0], mesh_min[:, 0]).astype(F)
            y = np.where(sy, mesh_max[:, 1], mesh_min[:, 1]).astype(F)
            z = np.where(sz, mesh_max[:, 2], mesh_min[:, 2]).astype(F)
            t = []
            for r in range(4):
                v = model[:, 0 * 4 + r] * x
                v = model[:, 1 * 4 + r] * y + v
                v = model[:, 2 * 4 + r] * z + v
                v = model[:, 3 * 4 + r] * F(1.0) + v
                t.append(v)
            for a in range(3):
                c = t[a] / t[3]
                lo[:, a] = np.fmin(lo[:, a], c)
                hi[:, a] = np.fmax(hi[:, a], c)
        centre = (hi + lo) / F(2.0)
        half = (hi - lo) / F(2.0)
        return centre - half, centre + half


def plane_terms(mins, maxs, planes):
    """The two operands of the plane test, per instance and plane slot (n, 6): sd, the signed distance of the box centre,
    and e, the box's extent along the normal. The instance is outside plane p when sd - e > 0."""
    with np.errstate(all="ignore"):
        h = (maxs - mins) * F(0.5)
        c = (mins + maxs) * F(0.5)
        sd = np.empty((len(mins), 6), F)
        e = np.empty((len(mins), 6), F)
        for p in range(6):
            nx, ny, nz, d = (F(v) for v in planes[p * 4 : p * 4 + 4])
            e[:, p] = h[:, 0] * np.abs(nx) + h[:, 1] * np.abs(ny) + h[:, 2] * np.abs(nz)
            a0, a1, a2, a3 = nx * c[:, 0], ny * c[:, 1], nz * c[:, 2], d * F(1.0)
            sd[:, p] = (a0 + a2) + (a1 + a3)
    return sd, e


def plane_margins(mins, maxs, planes):
    with np.errstate(all="ignore"):
        sd, e = plane_terms(mins, maxs, planes)
        return sd - e


def coarse_culled(mins, maxs, planes):
    with np.errstate(all="ignore"):
        return (plane_margins(mins, maxs, np.asarray(planes, F).reshape(24)) > 0).any(axis=1)


def dist_sq(pos, ref):
    """norm_squared of (ref - pos) as pick_lod forms it (helpers.rs:3-11), float32."""
    with np.errstate(all="ignore"):
        d = np.asarray(ref).astype(F).reshape(3)[None, :] - np.asarray(pos).astype(F)
        return F(0.0) + ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def lod_is_far(sq):
    with np.errstate(all="ignore"):
        return np.sqrt(sq) > F(10.0)


def draw_commands(pos, mesh_id, culled, meshes, cam_pos, first_instance_base=0, first_index_base=0):
    with np.errstate(all="ignore"):
        d = cam_pos.astype(F)[None, :] - pos.astype(F)
        sq = F(0.0) + ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        far = np.sqrt(sq) > F(10.0)
    n_lods = meshes["n_lods"][mesh_id]
    lod = (far & (n_lods > 1)).astype(np.int64)
    length = meshes["index_len"][mesh_id, lod].astype(np.uint64)
    vis = ~culled
    len_vis = np.where(vis, length, 0)
    first_index = (np.cumsum(len_vis) - len_vis + np.uint64(first_index_base)) & np.uint64(0xFFFFFFFF)
    keep = vis & (length > 0)
    idx = np.nonzero(keep)[0]
    return dict(indexCount=length[idx].astype(np.uint32), firstIndex=first_index[idx].astype(np.uint32),
                vertexOffset=meshes["vertex_offset"][mesh_id[idx]], firstInstance=(idx + first_instance_base).astype(np.uint32),
                total=int(len_vis.sum()) & 0xFFFFFFFF)


def light_draw_lists(pos, mesh_id, meshes, lights, first_instance_base=0):
    """shadow_mapping.rs:405-478: every light x every instance, LOD picked against the light."""
    out = []
    for lp in np.asarray(lights, F).reshape(-1, 3):
        with np.errstate(all="ignore"):
            d = lp[None, :] - pos.astype(F)
            sq = F(0.0) + ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
            far = np.sqrt(sq) > F(10.0)
        lod = (far & (meshes["n_lods"][mesh_id] > 1)).astype(np.int64)
        out.append(np.stack([meshes["index_len"][mesh_id, lod].astype(np.uint32), np.ones(len(pos), np.uint32),
                             meshes["index_offset"][mesh_id, lod].astype(np.uint32),
                             meshes["vertex_offset"][mesh_id].astype(np.int32).view(np.uint32),
                             (np.arange(len(pos)) + first_instance_base).astype(np.uint32)], axis=1))
    return np.stack(out)


def run(s, first_instance_base=0, first_index_base=0):
    model = model_matrices(s["pos"], s["rot"], s["scale"])
    mn = s["meshes"]["aabb_min"][s["mesh_id"]]
    mx = s["meshes"]["aabb_max"][s["mesh_id"]]
    mins, maxs = world_aabbs(model, mn, mx)
    culled = coarse_culled(mins, maxs, s["planes"])
    cmds = draw_commands(s["pos"], s["mesh_id"], culled, s["meshes"], s["cam_pos"], first_instance_base, first_index_base)
    return dict(model=model, world_aabb=np.concatenate([mins, maxs], axis=1), coarse_culled=culled, cmds=cmds)


# ---- row f-1: per-triangle cull + index append (generate_work.comp:68-200) -------------------

def src_index_offsets(pos, mesh_id, culled, meshes, cam_pos):
    """`indexOffset` of every emitted command: the index range of the LOD the frame picked for the instance, for the
    instances that are visible and whose LOD is not empty, in instance order (the order of the command list)."""
    with np.errstate(all="ignore"):
        d = np.asarray(cam_pos).astype(F)[None, :] - pos.astype(F)
        sq = F(0.0) + ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        far = np.sqrt(sq) > F(10.0)
    lod = (far & (meshes["n_lods"][mesh_id] > 1)).astype(np.int64)
    keep = ~np.asarray(culled).astype(bool) & (meshes["index_len"][mesh_id, lod] > 0)
    return meshes["index_offset"][mesh_id, lod][keep].astype(np.uint32)


def _mat4_vec4(m, x, y, z, w):
    """GLSL mat4 * vec4 as the column combination, left to right: m holds 16 scalars or arrays (column-major)."""
    return [((m[0 * 4 + r] * x + m[1 * 4 + r] * y) + m[2 * 4 + r] * z) + m[3 * 4 + r] * w for r in range(4)]


def triangle_culled(model, pv, v):
    """generate_work.comp:137-166 for the triangles v (t, 3 corners, 3) of one instance: True where the shader ends
    with cull == true. float32, one rounding per written operation; `xyz / w` are divisions."""
    m = [F(x) for x in np.asarray(model, F).reshape(16)]
    p = [F(x) for x in np.asarray(pv, F).reshape(16)]
    one = F(1.0)
    with np.errstate(all="ignore"):
        clip = []
        for k in range(3):
            world = _mat4_vec4(m, v[:, k, 0], v[:, k, 1], v[:, k, 2], one)        # model_mat * vec4(v, 1.0)
            clip.append(_mat4_vec4(p, world[0], world[1], world[2], world[3]))    # pv * (...)
        # determinant(mat3(vertex0.xyw, vertex1.xyw, vertex2.xyw)): column k is (x, y, w) of corner k; the cofactor
        # expansion along the first row of columns, m[0][0] * (m[1][1] * m[2][2] - m[2][1] * m[1][2]) - ...
        c = [[clip[k][0], clip[k][1], clip[k][3]] for k in range(3)]
        det = (c[0][0] * (c[1][1] * c[2][2] - c[2][1] * c[1][2]) - c[1][0] * (c[0][1] * c[2][2] - c[2][1] * c[0][2])) \
            + c[2][0] * (c[0][1] * c[1][2] - c[1][1] * c[0][2])
        cull = det > F(0.0)
        ndc_x = [clip[k][0] / clip[k][3] for k in range(3)]
        ndc_y = [clip[k][1] / clip[k][3] for k in range(3)]
        outside = ((ndc_x[0] < -one) & (ndc_x[1] < -one) & (ndc_x[2] < -one)) | ((ndc_x[0] > one) & (ndc_x[1] > one) & (ndc_x[2] > one)) \
            | ((ndc_y[0] < -one) & (ndc_y[1] < -one) & (ndc_y[2] < -one)) | ((ndc_y[0] > one) & (ndc_y[1] > one) & (ndc_y[2] > one))
    return cull | outside    # (the degenerate-triangle test ends in `cull = false`, :166: it decides nothing)


def cull_all_triangles(cmds, src, model, first_instance_base, pv, vertices, indices, out_capacity):
    """The frame's commands through generate_work.comp and compact_draw_stream.comp: for every command the triangles
    index_buffer[indexOffset / 3 + id], id < indexCount / 3, of vertex_buffer[vertexOffset + ix]; the survivors in order
    at out_index_buffer[firstIndex / 3 + k]; indexCount = 3 x survivors; commands without survivors dropped. Returns
    (final commands, the whole output buffer: slots nothing was written to hold 0xFFFFFFFF)."""
    vertices = np.asarray(vertices, F).reshape(-1, 3)
    indices = np.asarray(indices, np.uint32)
    model = np.asarray(model, F).reshape(-1, 16)
    out = np.full(int(out_capacity), 0xFFFFFFFF, np.uint32)
    final = np.array(cmds, copy=True)
    for k in range(len(final)):
        n_tris = int(final["indexCount"][k]) // 3
        s0 = int(src[k]) // 3 * 3
        ix = indices[s0 : s0 + n_tris * 3].reshape(n_tris, 3)
        v = vertices[ix.astype(np.int64) + int(final["vertexOffset"][k])]
        instance = (int(final["firstInstance"][k]) - int(first_instance_base)) & 0xFFFFFFFF
        kept = ix[~triangle_culled(model[instance], pv, v)] if n_tris else ix
        d0 = int(final["firstIndex"][k]) // 3 * 3
        assert d0 + kept.size <= len(out), "the restatement does not model a short output buffer"
        out[d0 : d0 + kept.size] = kept.reshape(-1)
        final["indexCount"][k] = kept.size
    return final[final["indexCount"] != 0], out
