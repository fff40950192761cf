"""Batched draws over the whole LOD chain without a GPU: tests/lod_restatement.py (written from the header's text) against
mip_batch_draws' restatement under the pin policy, against answers worked out by hand (tests/lod_cases.py), and against a
direct per-instance evaluation; the ABI surface of mip_batch_draws_lods."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import batch_restatement as br
import fuzz_scenes
import lod_cases as lc
import lod_restatement as lr
from renderer_amd.pipeline import DRAW_CMD_DTYPE, MESH_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi_instance_pipeline.h")
MODES = (lr.DISTANCE, lr.RELATIVE)


def _random_bitmap(rng, n):
    return rng.integers(0, 1 << 32, (max(n, 1) + 31) // 32, dtype=np.uint64).astype(np.uint32)


def _same(a, b, what):
    assert a["count"] == b["count"] and a["members"] == b["members"], what
    assert a["cmds"].tobytes() == b["cmds"].tobytes(), (what, "commands")
    assert a["ids"].tobytes() == b["ids"].tobytes(), (what, "ids")
    assert np.array_equal(a["order"], b["order"]), what


# ---- the pin: DISTANCE with {nextafter(100), inf, inf, inf, inf} is mip_batch_draws ----

@pytest.mark.parametrize("config,n", [(1, 1024), (2, 5000), (3, 20_000)])
def test_pin_policy_is_batch_draws_on_the_baseline_scenes(config, n):
    from renderer_amd import scene

    s = scene.make_scene(config, n=n)
    rng = np.random.default_rng(config)
    for bitmap in (lc.all_bits(n), _random_bitmap(rng, n)):
        want = br.batch_draws(s["pos"], s["mesh_id"], s["meshes"], s["cam_pos"], bitmap, first_instance_base=7)
        got = lr.batch_draws_lods(s["pos"], s["scale"], s["mesh_id"], s["meshes"], s["cam_pos"], bitmap, lr.DISTANCE, lr.PIN_SWITCH_SQ,
                                  first_instance_base=7)
        _same(got, want, f"config {config}")
        assert got["lod"].max() <= 1
    if config != 1:
        assert got["lod"].min() == 0 and got["lod"].max() == 1   # both sides of the pin are exercised


def test_pin_policy_is_batch_draws_on_fuzzed_scenes(oracle_mod):
    rng = np.random.default_rng(20261018)
    seen_nan = False
    for k in range(30):
        s = fuzz_scenes.random_scene(rng, oracle_mod, n_max=3000)
        n = s["n"]
        seen_nan |= bool(np.isnan(s["pos"]).any())
        bitmap = _random_bitmap(rng, n)
        base = s["first_instance_base"]
        want = br.batch_draws(s["pos"], s["mesh_id"], s["meshes"], s["cam_pos"], bitmap, first_instance_base=base)
        got = lr.batch_draws_lods(s["pos"], s["scale"], s["mesh_id"], s["meshes"], s["cam_pos"], bitmap, lr.DISTANCE, lr.PIN_SWITCH_SQ,
                                  first_instance_base=base)
        _same(got, want, f"fuzz {k}")
    assert seen_nan
    # the pin's first threshold is the library's kLodDistSqThreshold: the float32 behind 100
    assert np.float32(lr.PIN_SWITCH_SQ[0]) == np.nextafter(np.float32(100), np.float32(np.inf))


# ---- monotone along a ray ----

@pytest.mark.parametrize("mode", MODES)
def test_lod_never_decreases_with_distance_along_a_ray(mode):
    rng = np.random.default_rng(5 + mode)
    meshes = lc.chain_table([6, 3, 1, 5, 2], seed=9)
    cam = np.array([3.0, -2.0, 0.5], np.float32)
    for trial in range(20):
        direction = rng.normal(0, 1, 3)
        direction /= np.linalg.norm(direction)
        t = np.sort(np.concatenate([rng.uniform(0, 80, 400), 10.0 ** rng.uniform(-3, 25, 100)]))
        pos = (cam.astype(np.float64)[None, :] + t[:, None] * direction[None, :]).astype(np.float32)
        sw = np.sort(rng.choice([0.0, 1.0, 9.0, 100.0, 400.0, 2500.0, np.inf], 5))
        for mesh in range(len(meshes)):
            mesh_id = np.full(len(t), mesh, np.uint32)
            scale = np.full(len(t), rng.uniform(0.2, 3.0), np.float32)
            lod = lr.select_lods(pos, scale, mesh_id, meshes, cam, mode, sw)
            # q is what the rule compares; along the rounded positions it is the ray's order up to rounding, so sort by q itself
            with np.errstate(over="ignore"):
                d = cam[None, :] - pos
                q = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            assert (np.diff(lod[np.argsort(q, kind="stable")]) >= 0).all(), (mode, trial, mesh)
            assert lod.max() <= meshes["n_lods"][mesh] - 1


# ---- hand-worked answers: every switch, on it and one ulp to either side; special scales and positions ----

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("short", [False, True])
def test_hand_worked_decision_edges(mode, short):
    s = lc.edge_scene(mode)
    sw = lc.SWITCH_SHORT if short else lc.SWITCH
    lod = lr.select_lods(s["pos"], s["scale"], s["mesh_id"], s["meshes"], s["cam_pos"], mode, sw)
    want = lc.want_edge_lods(s, mode, short)
    bad = np.nonzero(lod != want)[0]
    assert len(bad) == 0, [(int(i), lc.edge_cases(mode)[s["case"][i]][0], int(lod[i]), int(want[i])) for i in bad[:8]]
    assert set(s["case"][s["case"] >= 0]) == set(range(len(lc.edge_cases(mode))))       # every case is in the scene
    assert s["case"][s["n"] - 1] >= 0 and s["n"] % 1024 != 0                                # ... one on the ragged tile's last instance
    assert {int(i) % 64 for i in np.nonzero(s["case"] >= 0)[0][:-1]} == {0, 63}
    if not short:
        assert set(lod[s["mesh_id"] == 0]) == set(range(6))                                 # every level is selected
        assert lod[s["mesh_id"] == 1].max() == 2                                            # n_lods = 3 stops at LOD 2


def test_the_thresholds_of_the_edge_scene_are_exact():
    # DISTANCE: x = 2 -> q = 4 = b_0, not beyond; nextafter(2) -> beyond. RELATIVE: (0.5 * 0.5) * 9 = 2.25, b_0 = 4 * 2.25 = 9 = 3 * 3.
    meshes = lc.chain_table([6])
    cam = np.zeros(3, np.float32)
    for mode, xs in lc.EDGE_X.items():
        for k, x in enumerate(xs):
            x = np.float32(x)
            pos = np.array([[np.nextafter(x, np.float32(0)), 0, 0], [x, 0, 0], [np.nextafter(x, np.float32(np.inf)), 0, 0]], np.float32)
            lod = lr.select_lods(pos, np.full(3, 0.5, np.float32), np.zeros(3, np.uint32), meshes, cam, mode, lc.SWITCH)
            assert lod.tolist() == [k, k, k + 1], (mode, k)


def test_clamping_zero_length_middle_level_and_expand():
    """mesh 1 (three levels) stops at LOD 2 whatever the distance; mesh 2's empty level 2 removes exactly the instances that pick
    it; expand() of the batches is the per-instance list: every visible instance with a non-empty level once, sorted by id."""
    for mode in MODES:
        s = lc.edge_scene(mode)
        n = s["n"]
        far = np.zeros((n, 3), np.float32)
        far[:, 0] = 1e6
        lod = lr.select_lods(far, np.full(n, 0.5, np.float32), s["mesh_id"], s["meshes"], s["cam_pos"], mode, lc.SWITCH)
        assert (lod[s["mesh_id"] == 1] == 2).all() and (lod[s["mesh_id"] != 1] == 5).all()
        # rings: x = 1 .. 61 (a period coprime to the three meshes) cycles through every level of every mesh
        ring = s["pos"].copy()
        ring[:, 0] = (1.0 + np.arange(n) % 61).astype(np.float32)
        ring[:, 1:] = 0
        rng = np.random.default_rng(mode)
        for bitmap in (lc.all_bits(n), _random_bitmap(rng, n)):
            b = lr.batch_draws_lods(ring, s["scale"], s["mesh_id"], s["meshes"], s["cam_pos"], bitmap, mode, lc.SWITCH, first_instance_base=100)
            bits = br.bitmap_bits(bitmap, n)
            dropped = bits & (s["mesh_id"] == 2) & (b["lod"] == 2)
            assert dropped.sum() > 0 and b["members"] == int(bits.sum() - dropped.sum())
            assert not np.isin(np.nonzero(dropped)[0], b["order"]).any()
            assert np.array_equal(np.sort(b["order"]), np.nonzero(bits & ~dropped)[0])
            direct = lr.per_instance_list(ring, s["scale"], s["mesh_id"], s["meshes"], s["cam_pos"], bitmap, mode, lc.SWITCH, first_instance_base=100)
            assert br.expand(b, 100).tobytes() == direct.tobytes()
            assert len(np.unique(b["ids"])) == b["members"]
            # buckets are real ones only, mesh-major: no command for mesh 2 LOD 2, at most B commands
            base, B = lr.lod_bases(s["meshes"])
            assert B == 15 and b["count"] == 14
            counts = b["cmds"]["instanceCount"].astype(np.int64)
            assert np.array_equal(b["cmds"]["firstInstance"], np.cumsum(counts) - counts)


def test_known_answer_by_hand():
    meshes = np.zeros(2, MESH_DTYPE)
    meshes["aabb_min"], meshes["aabb_max"] = (0, 0, 0), (1, 2, 2)
    meshes["n_lods"] = [3, 2]
    meshes["index_len"][:, :3] = [[30, 18, 6], [12, 0, 999]]
    meshes["index_offset"][:, :3] = [[0, 30, 48], [54, 66, 7777]]
    meshes["vertex_offset"] = [0, -4]
    #  instance:    0    1    2    3    4    5    6
    x = np.array([1.0, 3.0, 5.0, 1.0, 3.0, 9.0, 5.0], np.float32)
    pos = np.zeros((7, 3), np.float32)
    pos[:, 0] = x
    mesh_id = np.array([0, 0, 0, 1, 1, 0, 0], np.uint32)
    bitmap = np.array([0b0111111], np.uint32)   # instance 6 is culled
    # DISTANCE (4, 16): q = 1, 9, 25, 1, 9, 81, 25 -> LOD 0, 1, 2, 0, 1 (empty: no member), 2, -
    b = lr.batch_draws_lods(pos, np.ones(7, np.float32), mesh_id, meshes, np.zeros(3, np.float32), bitmap, lr.DISTANCE,
                            (4.0, 16.0, 64.0, 256.0, 1024.0), first_instance_base=10)
    want = np.array([(30, 1, 0, 0, 0), (18, 1, 30, 0, 1), (6, 2, 48, 0, 2), (12, 1, 54, -4, 4)], DRAW_CMD_DTYPE)
    assert b["cmds"].tobytes() == want.tobytes() and b["ids"].tolist() == [10, 11, 12, 15, 13] and b["members"] == 5
    # RELATIVE, scale 1: (1 * 1) * 9 = 9 -> b = 36, 144: q = 1, 9, 25 -> LOD 0; q = 81 -> LOD 1
    b = lr.batch_draws_lods(pos, np.ones(7, np.float32), mesh_id, meshes, np.zeros(3, np.float32), bitmap, lr.RELATIVE,
                            (4.0, 16.0, 64.0, 256.0, 1024.0))
    want = np.array([(30, 3, 0, 0, 0), (18, 1, 30, 0, 3), (12, 2, 54, -4, 4)], DRAW_CMD_DTYPE)
    assert b["cmds"].tobytes() == want.tobytes() and b["ids"].tolist() == [0, 1, 2, 5, 3, 4]


def test_policy_checks_of_the_restatement():
    for bad in ((-1.0, 1, 2, 3, 4), (1, 2, 3, 4, float("nan")), (4, 3, 5, 6, 7), (1, 2, 3, 4)):
        with pytest.raises(ValueError):
            lr.check_policy(lr.DISTANCE, bad)
    with pytest.raises(ValueError):
        lr.check_policy(2, lc.SWITCH)
    lr.check_policy(lr.RELATIVE, (0, 0, lr.INF, lr.INF, lr.INF))


# ---- the ABI surface: these fail on a library without the entry point ----

def test_library_exports_mip_batch_draws_lods_and_the_header_states_the_rule():
    import renderer_amd
    from renderer_amd import _lib
    from renderer_amd.pipeline import LOD_PIN_SWITCH_SQ, make_lod_policy

    lib = renderer_amd.load_library()
    assert hasattr(lib, "mip_batch_draws_lods") and "mip_batch_draws_lods" in _lib.EXPORTS
    text = open(HEADER).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int32_t\s+mip_batch_draws_lods\s*\(\s*MipContext\s*\*", header)
    assert re.search(r"typedef\s+struct\s+MipLodPolicy\s*\{", header)
    assert "100.00000762939453125f" in text and "lod = #{ k in [0, n_lods - 1) : q > b_k }" in text
    assert lib.mip_abi_version() == 4   # additive: the ABI version does not move
    assert lib.mip_batch_draws_lods(None, None, None, None, None) == -1
    assert callable(getattr(renderer_amd.InstancePipeline, "batch_draws_lods"))
    p = make_lod_policy("relative", (1.0, 2.0))
    assert p.struct_size == 28 and p.mode == _lib.MIP_LOD_RELATIVE and list(p.switch_sq) == [1.0, 2.0] + [float("inf")] * 3
    assert tuple(np.float32(v) for v in LOD_PIN_SWITCH_SQ) == tuple(np.float32(v) for v in lr.PIN_SWITCH_SQ)


def test_lod_policy_layout_matches_the_header(tmp_path):
    from renderer_amd import _lib

    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "mi_instance_pipeline.h"\nint main(void) {\n'
           '  printf("%zu %zu %zu %zu %u %u", sizeof(MipLodPolicy), offsetof(MipLodPolicy, struct_size), offsetof(MipLodPolicy, mode),\n'
           '         offsetof(MipLodPolicy, switch_sq), MIP_LOD_DISTANCE, MIP_LOD_RELATIVE);\n  return 0;\n}\n')
    c = tmp_path / "t.c"
    c.write_text(src)
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    P = _lib.MipLodPolicy
    assert got == [C.sizeof(P), P.struct_size.offset, P.mode.offset, P.switch_sq.offset, _lib.MIP_LOD_DISTANCE, _lib.MIP_LOD_RELATIVE]
    assert got[0] == 28
