"""Scenes for mip_batch_draws_ordered whose slot orders are written out by hand (tests/test_order_cases.py checks the
restatement against them; tests/test_gpu_batch_ordered.py runs the same scenes on the device).

The first two scenes: camera at the origin, every instance a candidate (a bitmap of ones), a table of one-level meshes, so every
instance selects LOD 0 under any policy and bucket = mesh. K = bits(q) >> 16 of q = |pos|^2 in float32.

edge_scene: n = 1024 + 3 * 64 + 17 instances (a ragged second tile, as lod_cases.edge_scene). Fillers (mesh 0, x = 1) are bucket
0; the cases below (mesh 1) are bucket 1, each once, on the last instance and on lanes 0 and 63 of the first rounds:

  instance  case                       position                      bits(q)       K
  1232      same K, nearer             x = 5                         0x41C80000    0x41C8   (tile 1, the last instance)
     0      zero                       x = 0                         0x00000000    0x0000
    63      subnormal q                x = 2^-70                     0x00000200    0x0000   (q = 2^-140; tied with q = 0)
    64      same K, farther            x = 5.01                      0x41C8CD02    0x41C8   (tile 0: lower draw index, but farther)
   127      below a step of K          x = bits 0x404B0469           0x4120FFFF    0x4120
   128      above a step of K          x = bits 0x404B046A           0x41210000    0x4121
   191      below a power of two       x = nextafter(2, 0)           0x407FFFFE    0x407F
   192      on a power of two          x = 2                         0x40800000    0x4080
   255      q overflows                x = 1e20                      0x7F800000    0x7F80
   256      NaN position               x = NaN                       NaN           0x7F80
   319      largest finite q           (2^64 - 2^40, 2^52, 0)        0x7F7FFFFF    0x7F7F   (x*x = 0x7F7FFFFE, + 2^104 = FLT_MAX)
   320      infinite position          x = -inf                      0x7F800000    0x7F80
   383      NaN in y                   (1, NaN, 0)                   NaN           0x7F80

NEAR_FIRST sorts bucket 1 by K ascending, FAR_FIRST by K descending, equal K in draw order in BOTH — so the zero / subnormal
pair, the same-K pair (64 before 1232 although 1232 is nearer) and the four K = 0x7F80 members keep their draw order under
both orders, and the NaNs are last (near first) or first (far first) together with q = +inf."""
import numpy as np

import lod_cases as lc

F = np.float32
INF = float("inf")
NAN = float("nan")
N_EDGE = 1024 + 3 * 64 + 17


def _from_bits(b):
    return np.array([b], np.uint32).view(F)[0]


# (instance, name, position, bits(q) or None for a NaN, K)
EDGE_CASES = (
    (1232, "same K, nearer", (5.0, 0.0, 0.0), 0x41C80000, 0x41C8),
    (0, "zero", (0.0, 0.0, 0.0), 0x00000000, 0x0000),
    (63, "subnormal q", (2.0 ** -70, 0.0, 0.0), 0x00000200, 0x0000),
    (64, "same K, farther", (5.01, 0.0, 0.0), 0x41C8CD02, 0x41C8),
    (127, "below a step of K", (_from_bits(0x404B0469), 0.0, 0.0), 0x4120FFFF, 0x4120),
    (128, "above a step of K", (_from_bits(0x404B046A), 0.0, 0.0), 0x41210000, 0x4121),
    (191, "below a power of two", (_from_bits(0x3FFFFFFF), 0.0, 0.0), 0x407FFFFE, 0x407F),
    (192, "on a power of two", (2.0, 0.0, 0.0), 0x40800000, 0x4080),
    (255, "q overflows", (1e20, 0.0, 0.0), 0x7F800000, 0x7F80),
    (256, "NaN position", (NAN, 0.0, 0.0), None, 0x7F80),
    (319, "largest finite q", (_from_bits(0x5F7FFFFF), 2.0 ** 52, 0.0), 0x7F7FFFFF, 0x7F7F),
    (320, "infinite position", (-INF, 0.0, 0.0), 0x7F800000, 0x7F80),
    (383, "NaN in y", (1.0, NAN, 0.0), None, 0x7F80),
)

# bucket 1's members in slot order, by instance — worked out from the table above, not computed
EDGE_NEAR_FIRST = (0, 63, 191, 192, 127, 128, 64, 1232, 319, 255, 256, 320, 383)
EDGE_FAR_FIRST = (255, 256, 320, 383, 319, 64, 1232, 128, 127, 192, 191, 0, 63)


def one_level_table(m, seed=4):
    """m meshes of one level each: B = m, bucket = mesh, every policy selects LOD 0."""
    return lc.chain_table([1] * m, seed=seed)


def edge_scene():
    n = N_EDGE
    pos = np.zeros((n, 3), F)
    pos[:, 0] = 1.0
    rot = np.zeros((n, 4), F)
    rot[:, 3] = 1.0
    mesh_id = np.zeros(n, np.uint32)
    for inst, _, p, _, _ in EDGE_CASES:
        pos[inst] = np.asarray(p, F)
        mesh_id[inst] = 1
    return dict(n=n, pos=pos, rot=rot, scale=np.full(n, 0.5, F), mesh_id=mesh_id, meshes=one_level_table(2), cam_pos=np.zeros(3, F))


def want_edge_slots(near_first):
    """The instance of every slot of edge_scene: bucket 0 = the fillers in draw order (one K), then bucket 1 as written above."""
    cases = {c[0] for c in EDGE_CASES}
    fillers = [i for i in range(N_EDGE) if i not in cases]
    return np.array(fillers + list(EDGE_NEAR_FIRST if near_first else EDGE_FAR_FIRST), np.int64)


# ---- ties across a round, a wave and a tile: stability through every pass ----
# One bucket. Three groups by instance % 3: x = 1 (K = 0x3F80), x = 3 (q = 9, K = 0x4110), x = 10 (q = 100, K = 0x42C8); the
# ranges around instance 64 (a round of 64), 256 (a wave's 256), 1024 and 2048 (tiles) are ALL put into the x = 3 group, so
# one tied group has consecutive members on both sides of each boundary. With 1 000+ members the group also crosses the
# 1 024-entry tiles of the (key, instance) list the later passes sort. Near first: group x = 1, then 3, then 10, each in draw
# order; far first: 10, 3, 1, each in draw order.
N_TIES = 3 * 1024 + 37
TIE_X = (1.0, 3.0, 10.0)
TIE_K = (0x3F80, 0x4110, 0x42C8)
TIE_RANGES = ((60, 70), (250, 262), (1018, 1032), (2044, 2052))


def tie_groups():
    g = np.arange(N_TIES) % 3
    for lo, hi in TIE_RANGES:
        g[lo:hi] = 1
    return g


def tie_scene():
    n = N_TIES
    g = tie_groups()
    pos = np.zeros((n, 3), F)
    pos[:, 0] = np.asarray(TIE_X, F)[g]
    rot = np.zeros((n, 4), F)
    rot[:, 3] = 1.0
    return dict(n=n, pos=pos, rot=rot, scale=np.full(n, 0.5, F), mesh_id=np.zeros(n, np.uint32), meshes=one_level_table(1), cam_pos=np.zeros(3, F))


def want_tie_slots(near_first):
    g = tie_groups()
    groups = (0, 1, 2) if near_first else (2, 1, 0)
    return np.concatenate([np.nonzero(g == k)[0] for k in groups]).astype(np.int64)


# ---- one class, different K, in one wave round: what the per-bucket count of pass 0 indexes by ----
# n = 64: one round of one wave. One mesh of two levels, so the buckets are its LODs; under lod_cases.SWITCH at scale 0.5 LOD 1
# starts beyond x = 2 (DISTANCE) or x = 3 (RELATIVE, b_0 = 4 * 2.25 = 9): x <= 2 is bucket 0 and x >= 5 bucket 1 in both modes.
#
#   instance  position   q        bits(q)      K        bucket  NEAR key     FAR key (D = 0x7F80 - K)
#    3        x = 5.5    30.25    0x41F20000   0x41F2   1       0x000141F2   0x00013D8E
#    7        x = 1.25   1.5625   0x3FC80000   0x3FC8   0       0x00003FC8   0x00003FB8
#   40        x = 5      25       0x41C80000   0x41C8   1       0x000141C8   0x00013DB8
#   others    x = 1      1        0x3F800000   0x3F80   0       0x00003F80   0x00004000
#
# Instances 3 and 40 are one bucket and differ only in the key's lowest digit (F2 / C8 near first, 8E / B8 far first);
# instance 7 has instance 40's lowest digit in BOTH orders, from the other bucket. A stage that counted the members of a
# bucket by the whole key, by its lowest digit or by any shift but 16 would not put 62 and 2 into the two commands.
N_DIGIT = 64
DIGIT_CASES = ((3, 5.5, 0x41F20000, 1), (7, 1.25, 0x3FC80000, 0), (40, 5.0, 0x41C80000, 1))   # (instance, x, bits(q), bucket)
DIGIT_FILLER_BITS = 0x3F800000
DIGIT_NEAR_FIRST = tuple(i for i in range(N_DIGIT) if i not in (3, 7, 40)) + (7,) + (40, 3)   # bucket 0: the fillers, then 7; bucket 1: 40, 3
DIGIT_FAR_FIRST = (7,) + tuple(i for i in range(N_DIGIT) if i not in (3, 7, 40)) + (3, 40)     # bucket 0: 7, then the fillers; bucket 1: 3, 40
DIGIT_COUNTS = (62, 2)


def digit_scene():
    n = N_DIGIT
    pos = np.zeros((n, 3), F)
    pos[:, 0] = 1.0
    for inst, x, _, _ in DIGIT_CASES:
        pos[inst, 0] = x
    rot = np.zeros((n, 4), F)
    rot[:, 3] = 1.0
    return dict(n=n, pos=pos, rot=rot, scale=np.full(n, 0.5, F), mesh_id=np.zeros(n, np.uint32), meshes=lc.chain_table([2], seed=5), cam_pos=np.zeros(3, F))


def want_digit_slots(near_first):
    return np.array(DIGIT_NEAR_FIRST if near_first else DIGIT_FAR_FIRST, np.int64)
