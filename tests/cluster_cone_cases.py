"""Hand-written geometry for the normal cones of cluster culling (include/mi_instance_pipeline.h, mip_build_cluster_cones /
mip_cull_clusters_cone) with hand-written answers.

The SHEET: tests/cluster_cases.py's ladder with the OUTSIDE triangle replaced by the INSIDE triangle wound the other way. Both
lie in the plane z = 0 inside the frustum |x|, |y|, |z| <= 8; cluster '1' is 64 copies of UP (0,0,0) (1,0,0) (0,1,0), normal
(0, 0, +1), cluster '0' 64 copies of DOWN (0,0,0) (0,1,0) (1,0,0), normal (0, 0, -1). Every operation of the build is exact
for them: e1 x e2 = (0, 0, +-1), len2 = 1, the axis sum (0, 0, +-T), aa = T^2, a = (0, 0, +-1), m = 1, k0 = 0. So

    cone = {0, 0, +-1, 2^-7,  0.5, 0.5, 0,  r},  r = r0 + r0 2^-7,  r0 = sqrtf(0.5f)        (box [0,1] x [0,1] x [0,0])

for a cluster of any number of triangles from 1 to 64. Instances sit at the origin with the identity rotation and scale 1, so
cw = centre and aw = a exactly. EYE = (0.25, 0.25, 5): d = (0.25, 0.25, -5), dd = 25.125, d . a = -+5.
  facing +1, cluster DOWN: Av = 5 - r = 4.287..., Bv = 2^-14 x 25.125 = 0.00153...: Av > 0, Av^2 = 18.3 > Bv: CULLED.
  facing +1, cluster UP:   Av = -5 - r < 0: survives.            facing -1: the other way round.
(Check by the stage's rule: DOWN has n = -z, x0 - e = (-0.25, -0.25, -5), n . (x0 - e) = +5 > 0: back-facing for facing +1.)
So under EYE and facing +1 the survive pattern of an instance IS its ladder string, and cluster_cases.ladder_scene's
hand-written commands — one per run of '1's — are the answer; under facing -1 it is the inverted string's.
"""
import numpy as np

import cluster_cases as cc

F = np.float32
INF = float("inf")
NAN = float("nan")
EYE = np.array([0.25, 0.25, 5.0], F)
R_FLAT = F(np.sqrt(F(0.5))) + F(np.sqrt(F(0.5))) * F(2.0 ** -7)         # r0 + r0 2^-7, r0 = sqrtf(0.5f)
K_FLAT = F(2.0 ** -7)                                                  # theta = 0: the margin alone
SHEET_VERTICES = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 0), (0, 1, 0), (1, 0, 0)], F)   # UP = (0, 1, 2), DOWN = (3, 4, 5)
CONE_UP = np.array([0, 0, 1, K_FLAT, 0.5, 0.5, 0, R_FLAT], F)
CONE_DOWN = np.array([0, 0, -1, K_FLAT, 0.5, 0.5, 0, R_FLAT], F)
NO_CONE = np.array([0, 0, 0, INF, 0, 0, 0, 0], F)


def invert(pattern):
    if isinstance(pattern, str):
        return pattern.translate(str.maketrans("01", "10"))
    return ~np.asarray(pattern, bool)


def sheet_scene(patterns, instance_pattern, facing=1.0, base=0, bits=None):
    """(scene, want): ladder_scene over the SHEET. The scene's geometry is the ladder of `patterns` ('1' = UP, '0' = DOWN)
    whatever the facing; want holds the hand-written commands and stats of mip_cull_clusters_cone under EYE and `facing`."""
    s, want = cc.ladder_scene(patterns, instance_pattern, base=base, bits=bits)
    s["vertices"] = SHEET_VERTICES.copy()
    if facing < 0:                                  # the same geometry, the answer of the inverted ladders
        _, want = cc.ladder_scene([invert(p) for p in patterns], instance_pattern, base=base, bits=bits)
    return s, want


def sheet_cones(patterns):
    """The cone table of a sheet scene, written down: one row per cluster, mesh-major."""
    rows = []
    for p in patterns:
        mask = np.frombuffer(p.encode(), np.uint8) == ord("1") if isinstance(p, str) else np.asarray(p, bool)
        rows += [CONE_UP if up else CONE_DOWN for up in mask]
    return np.array(rows, F).reshape(-1, 8)


def table_cases():
    """[(name, scene — cluster_cases._scene's dict, cones — the hand-written table)]: the build on its own."""
    out = []
    # a flat patch of 64 coplanar triangles: theta = 0
    s = cc._scene([cc._level("1", 64)], [(0, (0, 0, 0), 1.0)])
    s["vertices"] = SHEET_VERTICES.copy()
    out.append(("flat patch", s, np.array([CONE_UP], F)))
    # a one-triangle cluster; and short last clusters of 1 triangle behind full ones (T = 65, 129), UP and DOWN
    s = cc._scene([cc._level("1", 1), cc._level("10", 65), cc._level("011", 129)], [(0, (0, 0, 0), 1.0)])
    s["vertices"] = SHEET_VERTICES.copy()
    out.append(("one triangle, short last clusters", s, np.array([CONE_UP, CONE_UP, CONE_DOWN, CONE_DOWN, CONE_UP, CONE_UP], F)))
    # NO CONE: 63 UP and one DOWN triangle (m = -1: the spread is over the limit); 32 UP and 32 DOWN (the axis sum is 0);
    # one zero-area triangle (6, 6, 6) among 63 proper ones; one NaN vertex (7) in one triangle. The cluster behind each has its cone.
    extra = [(0.5, 0.5, 0), (NAN, 0, 0)]
    kinds = {"z": (6, 6, 6), "n": (0, 1, 7)}

    def mixed(first, count):
        ix = []
        for t in range(64):
            ix += list(first if t < count else cc.IN)
        return ix + list(cc.IN) * 64                 # and one whole UP cluster

    levels = [mixed(cc.OUT, 1), mixed(cc.OUT, 32), mixed(kinds["z"], 1), mixed(kinds["n"], 1)]
    s = cc._scene(levels, [(0, (0, 0, 0), 1.0)], extra_vertices=extra)
    s["vertices"] = np.concatenate([SHEET_VERTICES, np.array(extra, F)])
    out.append(("no cone", s, np.array([NO_CONE, CONE_UP] * 4, F)))
    return out


def sphere(longitudes=64, bands=32, radius=2.0, patch=(8, 4)):
    """A UV sphere between latitudes -75 and +75 degrees, wound outwards, listed in patches of 8 x 4 quads (64 triangles: one
    cluster each). Returns (vertices, indices). With the eye at the centre every triangle is back-facing for facing +1 (the
    outward normal points along x0 - e) and front-facing for facing -1; the patches are small enough for their cones to say so."""
    lat = np.radians(np.linspace(-75.0, 75.0, bands + 1))
    lon = np.arange(longitudes) / longitudes * 2 * np.pi
    la, lo = np.meshgrid(lat, lon, indexing="ij")
    v = np.stack([radius * np.cos(la) * np.cos(lo), radius * np.sin(la), radius * np.cos(la) * np.sin(lo)], axis=-1).reshape(-1, 3).astype(F)
    ix = []
    for pj in range(0, bands, patch[1]):
        for pi in range(0, longitudes, patch[0]):
            for j in range(pj, pj + patch[1]):
                for i in range(pi, pi + patch[0]):
                    a, b = j * longitudes + i, j * longitudes + (i + 1) % longitudes
                    c, d = (j + 1) * longitudes + (i + 1) % longitudes, (j + 1) * longitudes + i
                    ix += [a, c, b, a, d, c]         # outward: (b - a) x (c - a) points inwards for this grid, so the other way round
    return v, np.array(ix, np.uint32)


def sphere_scene(instances, radius=2.0):
    """A scene of sphere instances [(position, scale)], identity rotations, inside a wide frustum; one mesh, one level."""
    from renderer_amd.pipeline import MESH_DTYPE

    v, ix = sphere(radius=radius)
    meshes = np.zeros(1, MESH_DTYPE)
    meshes["aabb_min"][0], meshes["aabb_max"][0] = (-radius,) * 3, (radius,) * 3
    meshes["n_lods"][0], meshes["index_len"][0, 0], meshes["index_offset"][0, 0], meshes["vertex_offset"][0] = 1, len(ix), 0, 0
    n = len(instances)
    rot = np.zeros((n, 4), F)
    rot[:, 3] = 1.0
    planes = np.array([1, 0, 0, -64, -1, 0, 0, -64, 0, 1, 0, -64, 0, -1, 0, -64, 0, 0, 1, -64, 0, 0, -1, -64], F)
    return dict(n=n, meshes=meshes, vertices=v, indices=ix, pos=np.array([p for p, _ in instances], F).reshape(n, 3), rot=rot,
                scale=np.array([s for _, s in instances], F), mesh_id=np.zeros(n, np.uint32), planes=planes, cam_pos=cc.CAM, base=0,
                bitmap=np.full((n + 31) // 32, 0xFFFFFFFF, np.uint32))
