"""The inputs of the skinning kernel's structure tests (renderer_amd/csrc/skinning_kernel.hpp), built on the CPU,
deterministic and seeded: tests/test_oracle.py pins the oracle on them against float64, tests/test_gpu_skinned_edges.py runs
the kernel on the same arrays.

Skeleton families for a joint count J (the hierarchy is walked level by level through LDS):
  chain   parent[k] = k-1: depth J-1, one joint per level, one barrier each
  star    every joint a child of joint 0: one level of J-1 joints
  forest  all roots: max_depth 0 with J > 1, the walk and the re-read of G are skipped
  comb    parent[k] = k-2: two interleaved chains of two roots: a level's joints are not neighbours of their parents' level
  bushy   test_gpu_skinned._random_skeleton, with its one empty joint box
Sizes for J: with ipw = 64 // J instances per wave and ipb = 4 * ipw per workgroup, the smallest instance counts at which a
lane past the last whole instance of a wave, a partly filled last wave and a last workgroup of one instance all occur.

Guard bands: the kernel folds a joint box without its corners while mag * box_bound < 1e38 holds for every lane of the wave.
One joint box reaches 1e18 and that joint's pose scale runs over five decades, so that a launch holds — all from FINITE
inputs — instances far below the guard, instances above it whose corners are still finite, and instances whose products
overflow."""
import numpy as np

from test_gpu_skinned import _random_poses, _random_skeleton

FAMILIES = ("chain", "star", "forest", "comb", "bushy")
BIG_BOX = 1.0e18
BIG_JOINT = 3
SCALE_RANGE = (1.0e17, 1.0e22)   # five decades: under a random rotation a product with 1e18 overflows for certain only from
                                 # about 6e20 on, and a range that ended at 1e21 left under a tenth of the draws above that


def ipw_ipb(j):
    return 64 // j, 4 * (64 // j)


def sizes(j):
    ipw, ipb = ipw_ipb(j)
    out = []
    for n in (1, ipw, ipw + 1, ipb - 1, ipb, ipb + 1, 2 * ipb + ipw + 1):
        if n > 0 and n not in out:
            out.append(n)
    return out


def _seed(family, j):
    return 7000 + 100 * FAMILIES.index(family) + j


def skeleton(family, j):
    rng = np.random.default_rng(_seed(family, j))
    sk = _random_skeleton(rng, j)          # inverse binds and boxes; its hierarchy is kept for "bushy" only
    if family == "chain":
        parent = np.arange(-1, j - 1)
    elif family == "star":
        parent = np.array([-1] + [0] * (j - 1))
    elif family == "forest":
        parent = np.full(j, -1)
    elif family == "comb":
        parent = np.array([-1, -1] + list(range(j - 2)))[:j]
    else:
        assert family == "bushy", family
        parent = sk["parent"]
    sk["parent"] = np.asarray(parent, np.int32)
    if family != "bushy":                  # every joint binds vertices: each link of a chain reaches the fold
        lo = sk["joint_box"][:, :3]
        sk["joint_box"][:, 3:] = np.maximum(sk["joint_box"][:, 3:], lo + np.float32(0.1))
    return sk


_scene_cache = {}


def instances(n):
    """The first n instances of the mixed scene (prefix-stable generator): transforms, mesh table, camera."""
    from renderer_amd import scene

    if "s" not in _scene_cache:
        _scene_cache["s"] = scene.make_scene(3, n=640)
    s = _scene_cache["s"]
    assert n <= s["n"]
    return dict(s, n=n, pos=s["pos"][:n], rot=s["rot"][:n], scale=s["scale"][:n], mesh_id=s["mesh_id"][:n])


def family_case(family, j):
    """(skeleton, poses) at the largest size of sizes(j); a smaller size takes the first n poses."""
    n = sizes(j)[-1]
    rng = np.random.default_rng(_seed(family, j) + 50_000)
    poses = _random_poses(rng, n, j)
    if family == "chain":                  # 31 links of scale 0.7 .. 1.3 would wander over many decades
        poses[:, :, 7:10] = rng.uniform(0.9, 1.1, (n, j, 3))
    return skeleton(family, j), poses


def guard_skeleton():
    rng = np.random.default_rng(4242)
    parent = np.array([-1, 0, 0, 1, 3], np.int32)       # the big joint has a parent and a child: depth 2, and depth 3 inherits its scale
    ibm = np.tile(np.eye(4, dtype=np.float32).reshape(16), (5, 1))
    ibm[:, 12:15] = rng.uniform(-0.1, 0.1, (5, 3))
    ibm[:, [1, 4, 6, 9]] = rng.uniform(-0.02, 0.02, (5, 4))
    lo = rng.uniform(-1, 0, (5, 3)).astype(np.float32)
    box = np.concatenate([lo, lo + rng.uniform(0.1, 1.0, (5, 3)).astype(np.float32)], axis=1)
    box[BIG_JOINT, 3] = BIG_BOX                         # max x: box_bound = 3e18 + 1
    return dict(parent=parent, inverse_bind=ibm, joint_box=box)


def guard_poses(n, seed=4243):
    """Ordinary poses, except the big joint's scale: log-uniform per instance over SCALE_RANGE. The first 240 instances (five
    workgroups of 48) are sorted by that scale, so whole waves sit on one side of the guard and the waves in between cross it
    in order; the rest stay as drawn, so one wave holds instances of every band."""
    rng = np.random.default_rng(seed)
    poses = _random_poses(rng, n, 5)
    lg = rng.uniform(np.log10(SCALE_RANGE[0]), np.log10(SCALE_RANGE[1]), n)
    lg[:240] = np.sort(lg[:240])
    poses[:, BIG_JOINT, 7:10] = (10.0 ** lg)[:, None] * rng.uniform(0.7, 1.3, (n, 3))
    return poses


def guard_instances(n):
    s = instances(n)
    rot = np.zeros((n, 4), np.float32)
    rot[:, 3] = 1.0
    return dict(s, rot=rot, scale=np.ones(n, np.float32))


def box_bound(sk):
    """SkinArgs.box_bound as mip_set_skeleton computes it (float32)."""
    b = np.asarray(sk["joint_box"], np.float32)
    if not np.isfinite(b).all():
        return np.float32(np.inf)
    return np.float32(3.0) * np.abs(b).max() + np.float32(1.0)


def guard_bands(sk, oracle_result):
    """From the ORACLE's palette and posed boxes: per instance, is it far below the guard (separable), far above it with
    finite boxes (corner), or does its posed box hold a non-finite component (overflow). Asserts that each band holds at
    least a tenth of the instances."""
    pal = oracle_result["palette"].astype(np.float64)                    # (n, J, 16) column-major mat4
    n = pal.shape[0]
    mag = np.abs(pal.reshape(n, -1, 4, 4)[:, :, :, :3]).sum(axis=(2, 3))  # sum |J_k entries| (rows 0..2), per joint
    reach = mag.max(axis=1) * float(box_bound(sk))
    finite = np.isfinite(oracle_result["local_box"]).all(axis=1)
    bands = dict(separable=(reach < 0.5e38) & finite, corner=(reach > 2.0e38) & finite, overflow=~finite)
    for name, mask in bands.items():
        assert mask.sum() * 10 >= n, f"band {name}: {int(mask.sum())} of {n} instances"
    return bands


def nonfinite_box_skeletons():
    """Two skeletons whose box_bound is +inf: a joint box whose maximum is +inf (min <= max holds, 0 * inf is NaN), and one with
    a NaN coordinate (not empty by the > test: its corners are folded and the NaNs ignored)."""
    a, b = guard_skeleton(), guard_skeleton()
    for sk in (a, b):
        sk["joint_box"][BIG_JOINT, 3] = sk["joint_box"][BIG_JOINT, 0] + np.float32(0.5)
    a["joint_box"][2, 4] = np.inf
    b["joint_box"][1, 2] = np.nan
    return dict(inf_max=a, nan_coordinate=b)
