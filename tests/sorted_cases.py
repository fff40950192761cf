"""Scenes for mip_batch_draws_sorted whose slot orders and commands are written out by hand (tests/test_sorted_restatement.py
checks the restatement against them; tests/test_gpu_batch_sorted.py runs the same scenes on the device).

Every scene: camera at the origin, every instance a candidate (a bitmap of ones), a table of one-level meshes, so every instance
selects LOD 0 under any policy and bucket = mesh. A command is written here as (mesh, firstInstance, instanceCount).

RADIAL scene (q = |pos|^2, positions on the x axis unless noted; U = bits(q), 0x7F800000 for a NaN):

  instance  mesh  case                      position               U             K16     K24
     0      0     above a 16-bit step       x = bits 0x404B046A    0x41210000    0x4121  0x412100
     1      0     subnormal q               x = 2^-70              0x00000200    0x0000  0x000002
     2      1     NaN position              x = NaN                0x7F800000    0x7F80  0x7F8000
     3      1     above a 24-bit step       x = bits 0x40B51317    0x42001400    0x4200  0x420014
     4      0     above a 32-bit step       x = bits 0x40400002    0x41100003    0x4110  0x411000
     5      0     zero                      x = 0                  0x00000000    0x0000  0x000000
     6      0     q overflows               x = 1e20               0x7F800000    0x7F80  0x7F8000
     7      1     below the 24-bit step     x = bits 0x40B51316    0x420013FF    0x4200  0x420013
     8      1     below the 32-bit step     x = bits 0x40400001    0x41100002    0x4110  0x411000
     9      1     largest finite q          (2^64 - 2^40, 2^52, 0) 0x7F7FFFFF    0x7F7F  0x7F7FFF
    10      1     one                       x = 1                  0x3F800000    0x3F80  0x3F8000
    11      0     below the 16-bit step     x = bits 0x404B0469    0x4120FFFF    0x4120  0x4120FF

In every pair the member ABOVE the step has the lower draw index, so a pair that ties (its step is finer than depth_bits) keeps
draw order and shows above-before-below under NEAR_FIRST; a pair the key resolves shows below-before-above. The subnormal (1) and
zero (5) tie at 16 bits only. NaN (2) and +inf (6) tie always, in draw order, last near first and first far first.
Far first every tie keeps draw order and every resolved pair is above-before-below: the three depth_bits give one order.

VIEW_AXIS scene (axis = (0, 0, 1), positions (0, 0, z), so z is the position's z exactly):

  instance  mesh  z          U             K16
     0      0     -0         0x80000000    0x8000
     1      0     +inf       0xFF800000    0xFF80
     2      1     -1         0x407FFFFF    0x407F
     3      1     +2^-140    0x80000200    0x8000   (K24 = 0x800002)
     4      0     NaN        0xFF800000    0xFF80
     5      1     +0         0x80000000    0x8000
     6      1     -inf       0x007FFFFF    0x007F
     7      1     1          0xBF800000    0xBF80
     8      0     -2^-140    0x7FFFFDFF    0x7FFF

With a ZERO axis z is 0 for the finite positions and NaN (inf * 0) for instances 1, 4 and 6: two tied groups."""
import numpy as np

import lod_cases as lc
import order_cases as oc

F = np.float32
INF = float("inf")
NAN = float("nan")
RADIAL, VIEW_AXIS = 0, 1
NEAR_FIRST, FAR_FIRST = 1, 2


def _from_bits(b):
    return np.array([b], np.uint32).view(F)[0]


def _scene(pos, mesh_id, m):
    pos = np.asarray(pos, F).reshape(-1, 3)
    n = len(pos)
    rot = np.zeros((n, 4), F)
    rot[:, 3] = 1.0
    return dict(n=n, pos=pos, rot=rot, scale=np.full(n, 0.5, F), mesh_id=np.asarray(mesh_id, np.uint32), meshes=oc.one_level_table(m),
                cam_pos=np.zeros(3, F))


# ---- the RADIAL key edges ----
# (position, mesh, U)
RADIAL_CASES = (
    ((_from_bits(0x404B046A), 0.0, 0.0), 0, 0x41210000),
    ((2.0 ** -70, 0.0, 0.0), 0, 0x00000200),
    ((NAN, 0.0, 0.0), 1, 0x7F800000),
    ((_from_bits(0x40B51317), 0.0, 0.0), 1, 0x42001400),
    ((_from_bits(0x40400002), 0.0, 0.0), 0, 0x41100003),
    ((0.0, 0.0, 0.0), 0, 0x00000000),
    ((1e20, 0.0, 0.0), 0, 0x7F800000),
    ((_from_bits(0x40B51316), 0.0, 0.0), 1, 0x420013FF),
    ((_from_bits(0x40400001), 0.0, 0.0), 1, 0x41100002),
    ((_from_bits(0x5F7FFFFF), 2.0 ** 52, 0.0), 1, 0x7F7FFFFF),
    ((1.0, 0.0, 0.0), 1, 0x3F800000),
    ((_from_bits(0x404B0469), 0.0, 0.0), 0, 0x4120FFFF),
)

# {(order, depth_bits): (slots by instance, commands)} — worked out from the table in the docstring, not computed
_RADIAL_FAR = ((2, 6, 9, 3, 7, 0, 11, 4, 8, 10, 1, 5), ((1, 0, 1), (0, 1, 1), (1, 2, 3), (0, 5, 3), (1, 8, 2), (0, 10, 2)))
_RADIAL_NEAR_RUNS = ((0, 0, 2), (1, 2, 1), (0, 3, 1), (1, 4, 1), (0, 5, 2), (1, 7, 4), (0, 11, 1))
RADIAL_WANT = {
    (NEAR_FIRST, 16): ((1, 5, 10, 4, 8, 11, 0, 3, 7, 9, 2, 6), _RADIAL_NEAR_RUNS),
    (NEAR_FIRST, 24): ((5, 1, 10, 4, 8, 11, 0, 7, 3, 9, 2, 6), _RADIAL_NEAR_RUNS),
    (NEAR_FIRST, 32): ((5, 1, 10, 8, 4, 11, 0, 7, 3, 9, 2, 6), ((0, 0, 2), (1, 2, 2), (0, 4, 3), (1, 7, 4), (0, 11, 1))),
    (FAR_FIRST, 16): _RADIAL_FAR,
    (FAR_FIRST, 24): _RADIAL_FAR,
    (FAR_FIRST, 32): _RADIAL_FAR,
}


def radial_scene():
    return _scene([c[0] for c in RADIAL_CASES], [c[1] for c in RADIAL_CASES], 2)


# ---- the VIEW_AXIS key edges ----
VIEW_AXIS_Z = (0.0, 0.0, 1.0)
ZERO_AXIS = (0.0, 0.0, 0.0)
# (z, mesh, U)
AXIS_CASES = (
    (-0.0, 0, 0x80000000),
    (INF, 0, 0xFF800000),
    (-1.0, 1, 0x407FFFFF),
    (2.0 ** -140, 1, 0x80000200),
    (NAN, 0, 0xFF800000),
    (0.0, 1, 0x80000000),
    (-INF, 1, 0x007FFFFF),
    (1.0, 1, 0xBF800000),
    (-(2.0 ** -140), 0, 0x7FFFFDFF),
)
_AXIS_NEAR_RUNS = ((1, 0, 2), (0, 2, 2), (1, 4, 3), (0, 7, 2))
AXIS_WANT = {
    (NEAR_FIRST, 16): ((6, 2, 8, 0, 3, 5, 7, 1, 4), _AXIS_NEAR_RUNS),
    (NEAR_FIRST, 24): ((6, 2, 8, 0, 5, 3, 7, 1, 4), _AXIS_NEAR_RUNS),
    (NEAR_FIRST, 32): ((6, 2, 8, 0, 5, 3, 7, 1, 4), _AXIS_NEAR_RUNS),
    (FAR_FIRST, 16): ((1, 4, 7, 0, 3, 5, 8, 2, 6), ((0, 0, 2), (1, 2, 1), (0, 3, 1), (1, 4, 2), (0, 6, 1), (1, 7, 2))),
    (FAR_FIRST, 24): ((1, 4, 7, 3, 0, 5, 8, 2, 6), ((0, 0, 2), (1, 2, 2), (0, 4, 1), (1, 5, 1), (0, 6, 1), (1, 7, 2))),
    (FAR_FIRST, 32): ((1, 4, 7, 3, 0, 5, 8, 2, 6), ((0, 0, 2), (1, 2, 2), (0, 4, 1), (1, 5, 1), (0, 6, 1), (1, 7, 2))),
}
# the zero axis, any depth_bits: the finite positions (z = 0) in draw order, the non-finite ones (z = NaN) in draw order
ZERO_AXIS_WANT = {
    NEAR_FIRST: ((0, 2, 3, 5, 7, 8, 1, 4, 6), ((0, 0, 1), (1, 1, 4), (0, 5, 3), (1, 8, 1))),
    FAR_FIRST: ((1, 4, 6, 0, 2, 3, 5, 7, 8), ((0, 0, 2), (1, 2, 1), (0, 3, 1), (1, 4, 4), (0, 8, 1))),
}


def axis_scene():
    return _scene([(0.0, 0.0, c[0]) for c in AXIS_CASES], [c[1] for c in AXIS_CASES], 2)


# ---- ties across a round, a wave and a tile (order_cases.tie_scene's positions): stability through every pass ----
# Three tied groups by depth (x = 1, 3, 10); the middle group is mesh 1, the others mesh 0, so the three groups are three runs.
def tie_scene():
    s = oc.tie_scene()
    s["meshes"] = oc.one_level_table(2)
    s["mesh_id"] = (oc.tie_groups() == 1).astype(np.uint32)
    return s


def want_ties(near_first):
    slots = oc.want_tie_slots(near_first)
    c = np.bincount(oc.tie_groups(), minlength=3)
    sizes = (c[0], c[1], c[2]) if near_first else (c[2], c[1], c[0])
    runs = ((0, 0, int(sizes[0])), (1, int(sizes[0]), int(sizes[1])), (0, int(sizes[0] + sizes[1]), int(sizes[2])))
    return slots, runs


# ---- the run stage: every depth ties (one position), so slot order is draw order and mesh_id designs the runs ----
# name -> runs as (mesh, length), in draw order; neighbouring runs differ in mesh. Tiles are 1 024 slots.
RUN_SCENES = {
    "every slot its own run": tuple((i % 2, 1) for i in range(4097)),
    "one run over everything": ((2, 4097),),
    "a head at slot 1023": ((0, 1023), (1, 74)),
    "a head at slot 1024": ((0, 1024), (1, 73)),
    "a head at slot 1025": ((0, 1025), (1, 72)),
    "a run spanning three tiles": ((0, 500), (1, 2600), (2, 50)),
    "a run of one on the last slot": ((1, 2047), (0, 1), (2, 1)),
    "a head on every tile's first slot": ((0, 1024), (1, 1024), (0, 1024), (2, 1024), (1, 1)),
    "a single member": ((1, 1),),
}


def run_scene(runs):
    mesh_id = np.concatenate([np.full(length, mesh, np.uint32) for mesh, length in runs])
    pos = np.zeros((len(mesh_id), 3), F)
    pos[:, 0] = 1.0
    return _scene(pos, mesh_id, 3)


def want_runs(runs):
    """(mesh, firstInstance, instanceCount) of every run, from the lengths as designed."""
    out, first = [], 0
    for mesh, length in runs:
        out.append((mesh, first, length))
        first += length
    return tuple(out)


def last_tile_only(n=2 * 1024 + 300):
    """Members only in the last tile of instances: a bitmap whose bits start at instance 2 048. Meshes alternate in pairs, so
    the 300 members are 150 runs of two in slots 0..299."""
    mesh_id = ((np.arange(n) // 2) % 2).astype(np.uint32)
    pos = np.zeros((n, 3), F)
    pos[:, 0] = 1.0
    s = _scene(pos, mesh_id, 2)
    bits = np.zeros(n, bool)
    bits[2048:] = True
    bitmap = np.packbits(np.pad(bits, (0, (-n) % 32)), bitorder="little").view(np.uint32)
    slots = np.arange(2048, n, dtype=np.int64)
    runs = tuple((int(k % 2), 2 * k, 2) for k in range(150))
    return s, bitmap, slots, runs


def commands(meshes, runs):
    """The runs as commands over a one-level table: bucket = mesh, the three draw words are the mesh's level 0."""
    from renderer_amd.pipeline import DRAW_CMD_DTYPE

    cmds = np.zeros(len(runs), DRAW_CMD_DTYPE)
    for r, (mesh, first, count) in enumerate(runs):
        cmds[r] = (int(meshes["index_len"][mesh, 0]), count, int(meshes["index_offset"][mesh, 0]), int(meshes["vertex_offset"][mesh]), first)
    return cmds
