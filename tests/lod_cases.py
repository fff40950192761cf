"""Scenes for mip_batch_draws_lods whose answers can be worked out by hand (tests/test_lod_restatement.py checks the
restatement against them; tests/test_gpu_batch_lods.py runs the same scenes on the device), and synthetic mesh tables with a
chosen number of buckets.

The edge scene: camera at the origin, instances on one axis at distance x, so q = x*x is exact; switch_sq = (4, 16, 64, 256, 1024).
  DISTANCE: LOD k+1 replaces LOD k beyond x = 2, 4, 8, 16, 32.
  RELATIVE: box extents (1, 2, 2) -> diag_sq = 9; scale 0.5 -> (scale*scale)*diag_sq = 2.25, b_k = 9, 36, 144, 576, 2304 (all
            exact), so the switches are at x = 3, 6, 12, 24, 48."""
import numpy as np

from renderer_amd.pipeline import MESH_DTYPE

F = np.float32
DISTANCE, RELATIVE = 0, 1
INF = float("inf")
SWITCH = (4.0, 16.0, 64.0, 256.0, 1024.0)
SWITCH_SHORT = (4.0, 16.0, INF, INF, INF)   # levels 3.. are never selected
EDGE_X = {DISTANCE: (2.0, 4.0, 8.0, 16.0, 32.0), RELATIVE: (3.0, 6.0, 12.0, 24.0, 48.0)}


def chain_table(n_lods, seed=1, extents=(1.0, 2.0, 2.0)):
    """A table with the given n_lods per mesh: every level non-empty with a length and offset of its own."""
    n_lods = np.asarray(n_lods, np.int64)
    m = len(n_lods)
    rng = np.random.default_rng(seed)
    t = np.zeros(m, MESH_DTYPE)
    t["aabb_min"] = (0.0, -1.0, -1.0)
    t["aabb_max"] = np.asarray(extents, F) + np.asarray((0.0, -1.0, -1.0), F)
    t["n_lods"] = n_lods
    live = np.arange(6)[None, :] < n_lods[:, None]
    t["index_len"] = np.where(live, rng.integers(1, 20000, (m, 6)) * 3, 0)
    t["index_offset"] = np.where(live, rng.integers(0, 2 ** 31, (m, 6)), 0)
    t["vertex_offset"] = rng.integers(-1000, 2 ** 30, m)
    return t


def table_with_buckets(b, seed=2):
    """A table with exactly `b` buckets: meshes of six levels and one shorter mesh for the remainder (258 = 43 x 6,
    256 = 42 x 6 + 4)."""
    n_lods = [6] * (b // 6) + ([b % 6] if b % 6 else [])
    t = chain_table(n_lods, seed)
    assert int(t["n_lods"].sum()) == b
    return t


def edge_table():
    """mesh 0: six levels; mesh 1: three levels (selection stops at LOD 2); mesh 2: six levels, level 2 of zero length (the
    instances that pick it are no members)."""
    t = chain_table([6, 3, 6], seed=3)
    t["index_len"][2, 2] = 0
    return t


def edge_cases(mode):
    """[(name, pos xyz, scale, LOD a six-level mesh selects under SWITCH, ... under SWITCH_SHORT)], worked out by hand."""
    cases = []
    axes = (np.array([1, 0, 0], F), np.array([-1, 0, 0], F), np.array([0, 1, 0], F), np.array([0, 0, -1], F), np.array([0, -1, 0], F))
    for k, x in enumerate(EDGE_X[mode]):
        x = F(x)
        ax = axes[k]
        cases.append((f"below {k}", ax * np.nextafter(x, F(0)), 0.5, k, min(k, 2)))
        cases.append((f"on {k}", ax * x, 0.5, k, min(k, 2)))                       # q == b_k is NOT beyond it
        cases.append((f"above {k}", ax * np.nextafter(x, F(INF)), 0.5, k + 1, min(k + 1, 2)))
    # x = 5, q = 25: DISTANCE does not read scale: 25 > 4, > 16, not > 64
    at5 = np.array([5, 0, 0], F)
    rel = mode == RELATIVE
    cases.append(("scale 0", at5, 0.0, 5 if rel else 2, 2))            # b_k = 0 (finite thresholds), inf * 0 = NaN (infinite ones)
    cases.append(("scale negative", at5, -0.5, 1 if rel else 2, 1 if rel else 2))   # squared: as 0.5 — 25 > 9, not > 36
    cases.append(("scale subnormal", at5, 1e-42, 5 if rel else 2, 2))  # scale*scale underflows to 0
    cases.append(("scale inf", at5, INF, 0 if rel else 2, 0 if rel else 2))   # b_k = inf
    cases.append(("scale NaN", at5, float("nan"), 0 if rel else 2, 0 if rel else 2))
    for a in range(3):
        p = np.array([5, 5, 5], F)
        p[a] = np.nan
        cases.append((f"NaN position {a}", p, 0.5, 0, 0))
    cases.append(("q overflows", np.array([1e20, 0, 0], F), 0.5, 5, 2))   # q = +inf: the last LOD whose b_k is finite
    cases.append(("position inf", np.array([0, -INF, 0], F), 0.5, 5, 2))
    return cases


def edge_scene(mode, n=1024 + 3 * 64 + 17):
    """n instances (a ragged last tile) over edge_table(): fillers at x = 1 (LOD 0) and the edge cases, cycled over the
    instances on lanes 0 and 63 of every round of 64 and on the last instance. `case` is each instance's case number or -1."""
    cases = edge_cases(mode)
    pos = np.zeros((n, 3), F)
    pos[:, 0] = 1.0
    scale = np.full(n, 0.5, F)
    rot = np.zeros((n, 4), F)
    rot[:, 3] = 1.0
    mesh_id = (np.arange(n) % 3).astype(np.uint32)
    case = np.full(n, -1, np.int64)
    spots = [n - 1] + [i for i in range(n - 1) if i % 64 in (0, 63)]
    assert len(spots) >= len(cases)
    just_beyond = [name for name, *_ in cases].index("above 2")
    for j, i in enumerate(spots):
        c = just_beyond if j == 0 else (j - 1) % len(cases)   # the last instance sits just beyond a switch
        case[i] = c
        pos[i] = cases[c][1]
        scale[i] = cases[c][2]
        mesh_id[i] = 0 if j <= len(cases) else j % 3           # the hand answers are for six levels; later rounds use every mesh
    return dict(n=n, pos=pos, rot=rot, scale=scale, mesh_id=mesh_id, meshes=edge_table(), cam_pos=np.zeros(3, F), case=case)


def want_edge_lods(s, mode, short=False):
    """The hand-worked LOD of every instance of edge_scene: the case's answer for a six-level mesh, stopped at the mesh's
    last level; fillers select LOD 0."""
    cases = edge_cases(mode)
    want6 = np.array([0 if c < 0 else cases[c][4 if short else 3] for c in s["case"]], np.int64)
    return np.minimum(want6, s["meshes"]["n_lods"][s["mesh_id"]].astype(np.int64) - 1)


def all_bits(n):
    return np.full((max(n, 1) + 31) // 32, 0xFFFFFFFF, np.uint32)
