"""A float64 evaluation of the path's FORMULAS (not of its rounding): M = T·R·S, the eight-corner
world AABB, the six-plane test with its margin. Used to show that (a) matrices agree to the north
star's 1e-5 relative tolerance independent of any operation order, and (b) visibility agrees
wherever an instance is not within rounding distance of a plane."""
import numpy as np


def run(s):
    pos = s["pos"].astype(np.float64)
    i, j, k, w = (s["rot"][:, c].astype(np.float64) for c in range(4))
    sc = s["scale"].astype(np.float64)
    n = len(sc)
    R = np.empty((n, 3, 3))
    R[:, 0, 0] = w * w + i * i - j * j - k * k; R[:, 0, 1] = 2 * (i * j - w * k); R[:, 0, 2] = 2 * (w * j + i * k)
    R[:, 1, 0] = 2 * (w * k + i * j); R[:, 1, 1] = w * w - i * i + j * j - k * k; R[:, 1, 2] = 2 * (j * k - w * i)
    R[:, 2, 0] = 2 * (i * k - w * j); R[:, 2, 1] = 2 * (w * i + j * k); R[:, 2, 2] = w * w - i * i - j * j + k * k
    M = np.zeros((n, 4, 4))
    M[:, :3, :3] = R * sc[:, None, None]
    M[:, :3, 3] = pos
    M[:, 3, 3] = 1.0
    mn = s["meshes"]["aabb_min"][s["mesh_id"]].astype(np.float64)
    mx = s["meshes"]["aabb_max"][s["mesh_id"]].astype(np.float64)
    corners = np.stack([np.where(np.array(sel, bool)[None, :], mx, mn)
                        for sel in ((0, 0, 0), (1, 0, 0), (0, 0, 1), (1, 0, 1), (0, 1, 0), (1, 1, 0), (0, 1, 1), (1, 1, 1))], axis=1)
    world = np.einsum("nrc,nkc->nkr", M[:, :3, :3], corners) + M[:, None, :3, 3]
    lo, hi = world.min(axis=1), world.max(axis=1)
    centre, half = (lo + hi) / 2, (hi - lo) / 2
    planes = s["planes"].astype(np.float64).reshape(6, 4)
    margin = (centre @ planes[:, :3].T + planes[:, 3]) - half @ np.abs(planes[:, :3]).T  # s - e per plane, (n, 6)
    scale = np.abs(centre) @ np.abs(planes[:, :3]).T + np.abs(planes[:, 3]) + half @ np.abs(planes[:, :3]).T
    culled = (margin > 0).any(axis=1)
    # an instance is "decided" when no plane's margin is within rounding distance of zero
    decided = (np.abs(margin) > 1e-4 * scale).all(axis=1)
    model_colmajor = M.transpose(0, 2, 1).reshape(n, 16)
    return dict(model=model_colmajor, mins=lo, maxs=hi, culled=culled, decided=decided)


# ---- row f-1: the per-triangle decision (generate_work.comp:137-166) ------------------------------------------------
#
# The forward error bound of the float32 chain, in units of u = 2^-24, against the ABSOLUTE-VALUE evaluation of the same
# expression (every product and sum taken over |pv|, |model|, |v|: cancellation inside the transform is covered).
#   * world = model * vec4(v, 1): a dot product of four terms, 4 multiplications and 3 additions, at most 4 roundings on any
#     term's path: |error| <= 4u |model||v|.
#   * clip = pv * world: the same again over inputs that already carry 4u: (4 + 4)u |pv||model||v| =: 8u A, to first order.
#   * det: a sum of six products of three clip values: 3 x 8u from the factors, 2u from the two multiplications, and at most
#     3u from the subtraction inside the cofactor and the two outer additions: 29u x the permanent-like sum of |.| products.
#   * the bound tests compare x / w with +-1: 8u A_x + 8u A_w from the operands, 1u |w| from the division: <= 9u (A_x + A_w).
# K is the larger of the two, rounded up to a power of two. It is derived, not tuned: a test that fails with it has found
# something.
TRIANGLE_K = 32


def triangle_decisions(model, pv, v, k=TRIANGLE_K):
    """model, pv: float32[16] column-major; v: (t, 3 corners, 3) float32 positions. Returns (culled, decided): the shader's
    decision evaluated in float64 from those float32 inputs, and whether every quantity the decision hangs on is further
    from its threshold than the float32 chain's forward error bound (k u x magnitudes)."""
    u = 2.0 ** -24
    M = np.asarray(model, np.float64).reshape(4, 4).T    # row-major 4x4
    P = np.asarray(pv, np.float64).reshape(4, 4).T
    vh = np.concatenate([np.asarray(v, np.float64), np.ones(v.shape[:2] + (1,))], axis=-1)   # (t, 3, 4)
    with np.errstate(all="ignore"):
        clip = vh @ (P @ M).T                                     # (t, 3, 4)
        mag = np.abs(vh) @ (np.abs(P) @ np.abs(M)).T              # |pv| |model| |v|
        c, a = clip[..., [0, 1, 3]], mag[..., [0, 1, 3]]          # xyw of the three corners: (t, corner, 3)
        det = (c[:, 0, 0] * (c[:, 1, 1] * c[:, 2, 2] - c[:, 2, 1] * c[:, 1, 2]) - c[:, 1, 0] * (c[:, 0, 1] * c[:, 2, 2] - c[:, 2, 1] * c[:, 0, 2])
               + c[:, 2, 0] * (c[:, 0, 1] * c[:, 1, 2] - c[:, 1, 1] * c[:, 0, 2]))
        det_mag = (a[:, 0, 0] * (a[:, 1, 1] * a[:, 2, 2] + a[:, 2, 1] * a[:, 1, 2]) + a[:, 1, 0] * (a[:, 0, 1] * a[:, 2, 2] + a[:, 2, 1] * a[:, 0, 2])
                   + a[:, 2, 0] * (a[:, 0, 1] * a[:, 1, 2] + a[:, 1, 1] * a[:, 0, 2]))
        w = clip[..., 3]
        ndc = clip[..., :2] / w[..., None]                         # (t, corner, 2)
        outside = (ndc < -1.0).all(axis=1).any(axis=1) | (ndc > 1.0).all(axis=1).any(axis=1)
        culled = (det > 0.0) | outside
        sgn = np.where(w < 0.0, -1.0, 1.0)
        margin = np.abs(np.abs(clip[..., :2] * sgn[..., None]) - np.abs(w)[..., None])   # |x sgn w| - |w|: 0 on a bound
        decided = (np.abs(det) > k * u * det_mag) \
            & (margin > k * u * (mag[..., :2] + mag[..., 3:4])).all(axis=(1, 2)) \
            & (np.abs(w) > k * u * mag[..., 3]).all(axis=1) \
            & np.isfinite(clip).all(axis=(1, 2))
    return culled, decided


# ---- extension, BASELINE config 5: the joint palette and the posed box (glTF 2.0 section 3.7.3) ----------------------
#
# skinned_reference evaluates the DEFINITION in float64 from the float32 inputs — L = T R S, G_k = G_parent L_k,
# J_k = G_k IBM_k, the union of the eight transformed corners per non-empty joint box — vectorised over the instances and
# independent of the oracle's loop. Beside every quantity it evaluates the same expression with every term replaced by its
# absolute value: the running bound A of the float32 chain. With u = 2^-24, a float32 evaluation whose terms pass through at
# most k roundings differs from the exact value by at most k u / (1 - k u) * A (Higham, Accuracy and Stability, lemma 3.1):
#   * quaternion -> rotation -> scale: a diagonal entry is four products and three additions, then the scale: at most 8;
#   * every affine product on the path from the root, and the inverse-bind product: (a0 b0 + a1 b1) + a2 b2 (+ a3), a
#     product, two additions and the translation's: 4 per product, over depth_k + 2 products at the most;
#   so k = 4 (depth_k + 2) + 8 for palette entry J_k, and 4 more for a corner J_k (x, y, z, 1). min / max are 1-Lipschitz:
#   a component of the posed box is within the largest of its corners' bounds.
SKIN_U = 2.0 ** -24


def skin_rounding_bound(k, a):
    return (k * SKIN_U) / (1.0 - k * SKIN_U) * a


def _trs_and_bound(poses):
    """poses (n, J, 10) -> L, |L| as (n, J, 3, 4) row-major affine matrices."""
    p = np.asarray(poses, np.float64)
    t, s = p[..., 0:3], p[..., 7:10]
    i, j, k, w = (p[..., 3 + c] for c in range(4))
    R = np.empty(p.shape[:2] + (3, 3))
    A = np.empty_like(R)
    sq = (w * w, i * i, j * j, k * k)
    R[..., 0, 0] = sq[0] + sq[1] - sq[2] - sq[3]; R[..., 1, 1] = sq[0] - sq[1] + sq[2] - sq[3]; R[..., 2, 2] = sq[0] - sq[1] - sq[2] + sq[3]
    R[..., 0, 1] = 2 * (i * j - w * k); R[..., 0, 2] = 2 * (w * j + i * k)
    R[..., 1, 0] = 2 * (w * k + i * j); R[..., 1, 2] = 2 * (j * k - w * i)
    R[..., 2, 0] = 2 * (i * k - w * j); R[..., 2, 1] = 2 * (w * i + j * k)
    A[..., 0, 0] = A[..., 1, 1] = A[..., 2, 2] = sq[0] + sq[1] + sq[2] + sq[3]
    A[..., 0, 1] = A[..., 1, 0] = 2 * (np.abs(i * j) + np.abs(w * k))
    A[..., 0, 2] = A[..., 2, 0] = 2 * (np.abs(w * j) + np.abs(i * k))
    A[..., 1, 2] = A[..., 2, 1] = 2 * (np.abs(j * k) + np.abs(w * i))
    L = np.concatenate([R * s[..., None, :], t[..., :, None]], axis=-1)
    LA = np.concatenate([A * np.abs(s)[..., None, :], np.abs(t)[..., :, None]], axis=-1)
    return L, LA


def _affine(a, b):
    """(.., 3, 4) x (.., 3, 4) as affine transforms (bottom row 0 0 0 1)."""
    out = a[..., :, :3] @ b
    out[..., :, 3] += a[..., :, 3]
    return out


CORNERS = ((0, 1, 2), (3, 1, 2), (0, 1, 5), (3, 1, 5), (0, 4, 2), (3, 4, 2), (0, 4, 5), (3, 4, 5))  # (x, y, z) picks out of min xyz max xyz


def skinned_reference(skeleton, poses):
    """float64: palette (n, J, 3, 4) row-major, posed box (n, 6) = min xyz, max xyz over the non-empty joint boxes (+inf /
    -inf where there is none), and their float32 rounding bounds palette_tol / box_tol, element for element."""
    parent = np.asarray(skeleton["parent"])
    J = len(parent)
    ibm = np.asarray(skeleton["inverse_bind"], np.float64).reshape(J, 4, 4).transpose(0, 2, 1)[:, :3, :]  # column-major mat4 -> rows 0..2
    box = np.asarray(skeleton["joint_box"], np.float64).reshape(J, 6)
    L, LA = _trs_and_bound(poses)
    n = L.shape[0]
    G, GA = L.copy(), LA.copy()
    depth = np.zeros(J, int)
    for k in range(J):
        if parent[k] >= 0:
            depth[k] = depth[parent[k]] + 1
            G[:, k], GA[:, k] = _affine(G[:, parent[k]], L[:, k]), _affine(GA[:, parent[k]], LA[:, k])
    palette = _affine(G, ibm[None])
    palette_a = _affine(GA, np.abs(ibm)[None])
    kk = 4.0 * (depth + 2) + 8.0
    palette_tol = skin_rounding_bound(kk[None, :, None, None], palette_a)
    lo, hi = np.full((n, 3), np.inf), np.full((n, 3), -np.inf)
    tol = np.zeros((n, 3))
    for k in range(J):
        b = box[k]
        if b[0] > b[3] or b[1] > b[4] or b[2] > b[5]:
            continue  # the joint binds no vertex
        for pick in CORNERS:
            c = np.array([b[pick[0]], b[pick[1]], b[pick[2]], 1.0])
            v = palette[:, k] @ c
            lo, hi = np.minimum(lo, v), np.maximum(hi, v)
            tol = np.maximum(tol, skin_rounding_bound(kk[k] + 4.0, palette_a[:, k] @ np.abs(c)))
    return dict(palette=palette, palette_tol=palette_tol, box=np.concatenate([lo, hi], axis=1), box_tol=np.concatenate([tol, tol], axis=1))
