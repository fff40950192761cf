"""The sizes tests/test_gpu_boundaries.py launches at come from plan_frame (tests/plan_boundaries.py over
tests/native/frame_plan_probe.cpp). Here, on the CPU: the list for the 256 CUs of an MI355X is pinned against the table of
thresholds it was written from (if a threshold moves, this says which); the order thresholds scale with the CU count and the
group-size ones do not; every pair the helper yields really straddles; and `truncate_frame` — one oracle run at the largest size
serving every smaller one — equals the oracle's own frame of the prefix byte for byte, and a frame that is one instance or one
firstIndex off is caught by the comparison the GPU tests use."""
import os
import re

import numpy as np
import pytest

import plan_boundaries as pb
from helpers import assert_parity, run_oracle, truncate_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R4 = pb.ROUND4_TRIANGLE_KERNELS


def _changes(request, cu=256, **state):
    return {b.n: b.fields for b in pb.plan_changes(request, cu, **state)}


def test_the_list_at_256_cus_contains_every_threshold_of_the_table():
    """(instances below, instances at) per row of the table in DESIGN §16.1. The per-triangle rows are the round-4 kernels'
    (MIP_TUNE_TRI_CHUNKS_FROM=4294967295: parts / workgroup-per-command / waves); under the default tuning the range kernel takes
    every frame up to 65 536 instances and only the 65 536 / 65 537 row is a plan change — both are pinned."""
    streams, general, commands = _changes(pb.STREAMS), _changes(pb.STREAMS, nonfinite=1), _changes(pb.COMMANDS_ONLY)
    assert streams == {131_073: ("group_shift",), 524_289: ("order", "group_shift")}
    assert general == {131_073: ("group_shift",), 327_681: ("order",), 524_289: ("group_shift",)}
    assert commands == {131_073: ("group_shift",), 524_289: ("group_shift",), 1_114_113: ("order",)}
    assert _changes(pb.SKINNED, n_joints=4) == general           # a skinned frame runs the kernel with the fall-back tiers
    tiles = pb.structure_tiles(pb.STREAMS)
    assert set(tiles) == {16, 512, 544, 2048, 2112, 4160, 4672}
    assert "window edge" in tiles[4160] and tiles[4160].startswith("window edge: 65 groups of 64")
    sizes = pb.boundary_sizes(pb.STREAMS)
    for n in (131_072, 131_073, 524_288, 524_289, 1_064_960, 1_064_961, 4_096, 4_097, 1_064_705):
        assert n in sizes, n
    assert {327_680, 327_681} <= set(pb.boundary_sizes(pb.STREAMS, nonfinite=1))
    assert {1_114_112, 1_114_113} <= set(pb.boundary_sizes(pb.COMMANDS_ONLY))
    # per-triangle stage
    tri_default = _changes(pb.TRIANGLES, max_lod_tris=20_000, hi=70_000)
    assert tri_default == {65_537: ("tri", "recompact")}
    tri_r4 = _changes(pb.TRIANGLES, max_lod_tris=20_000, hi=70_000, tri_chunks_from=R4)
    assert tri_r4 == {1_025: ("tri", "tri_threads"), 3_073: ("tri_threads",), 32_769: ("tri_block_tickets",),
                      65_537: ("tri", "tri_block_tickets", "tri_either", "recompact")}
    # two frame slots: no parts kernel, so 1 024 / 1 025 straddles nothing and 768 / 769 (1024 -> 512 threads) appears
    tri_r4_two = _changes(pb.TRIANGLES, max_lod_tris=20_000, hi=70_000, tri_chunks_from=R4, frame_slots=2)
    assert tri_r4_two == {769: ("tri_threads",), 3_073: ("tri_threads",), 32_769: ("tri_block_tickets",),
                          65_537: ("tri", "tri_block_tickets", "tri_either", "recompact")}
    for lo_n, hi_n in ((768, 769), (1_024, 1_025), (3_072, 3_073), (32_768, 32_769), (65_536, 65_537)):
        in_some = any({lo_n, hi_n} <= set(pb.boundary_sizes(pb.TRIANGLES, hi=70_000, max_lod_tris=20_000, tri_chunks_from=R4, frame_slots=fs))
                      for fs in (1, 2))
        assert in_some, (lo_n, hi_n)
    # the parts kernel is refused by mesh size: 16 x 256 x 8 triangles
    a = pb.plan(1000, pb.TRIANGLES, max_lod_tris=32_768, tri_chunks_from=R4)
    b = pb.plan(1000, pb.TRIANGLES, max_lod_tris=32_769, tri_chunks_from=R4)
    assert (a["tri"], b["tri"], b["tri_threads"]) == ("parts", "block", 512)


@pytest.mark.parametrize("cu", [64, 304])
def test_order_thresholds_scale_with_the_cu_count_and_group_sizes_do_not(cu):
    for request, state, per_cu in ((pb.STREAMS, {}, 8), (pb.STREAMS, {"nonfinite": 1}, 5), (pb.COMMANDS_ONLY, {}, 17)):
        changes = _changes(request, cu, hi=2_000_000, **state)
        order_at = [n for n, f in changes.items() if "order" in f]
        assert order_at == [256 * cu * per_cu + 1], (cu, request, state, changes)
        assert [n for n, f in changes.items() if "group_shift" in f] == [131_073, 524_289]
    assert pb.structure_tiles(pb.STREAMS, cu) == pb.structure_tiles(pb.STREAMS, 256)


def test_every_yielded_pair_has_differing_plans():
    cases = [(pb.STREAMS, {}), (pb.STREAMS, {"nonfinite": 1}), (pb.COMMANDS_ONLY, {}), (pb.SKINNED, {"n_joints": 4}),
             (pb.TRIANGLES, {"max_lod_tris": 20_000}), (pb.TRIANGLES, {"max_lod_tris": 20_000, "tri_chunks_from": R4}),
             (pb.TRIANGLES, {"max_lod_tris": 20_000, "tri_chunks_from": R4, "frame_slots": 2})]
    seen = 0
    for cu in (64, 256, 304):
        for request, state in cases:
            for below, at, fields in pb.straddling_pairs(request, cu, **state):
                assert at == below + 1
                assert set(pb.assert_straddles(below, at, request, cu, fields=fields, **state)) == set(fields)
                seen += 1
    assert seen >= 3 * 20
    with pytest.raises(AssertionError):                          # and a pair that does not straddle is refused
        pb.assert_straddles(131_073, 131_074)
    with pytest.raises(AssertionError):
        pb.assert_straddles(524_288, 524_289, pb.COMMANDS_ONLY, fields=("order",))


def test_probe_constants_are_the_kernels():
    text = open(os.path.join(ROOT, "renderer_amd", "csrc", "instance_kernel.hpp")).read()
    window = int(re.search(r"constexpr uint32_t kLevel1Window = (\d+);", text).group(1))
    p = pb.plan(1)
    assert p["level1_window"] == window and p["tile"] == 256


# ---- truncate_frame ----

def _scene(n, all_visible=False):
    from renderer_amd import scene

    return scene.make_scene(3, n=n, all_visible=all_visible)


def _prefix(s, n):
    return dict(s, n=n, pos=s["pos"][:n], rot=s["rot"][:n], scale=s["scale"][:n], mesh_id=s["mesh_id"][:n])


def _same_frame(got, want, what):
    assert_parity(got, want, what)
    for key in ("model", "world_aabb", "visible_bitmap", "coarse_culled"):
        assert got[key].shape == want[key].shape and got[key].tobytes() == want[key].tobytes(), (what, key)


@pytest.mark.parametrize("all_visible,base,index_base", [(False, 0, 0), (True, 123_456, 0xFFFFFF00)])
def test_truncated_frame_is_the_oracles_frame_of_the_prefix(oracle_mod, all_visible, base, index_base):
    big = 70_000
    s = _scene(big, all_visible)
    s["pos"][300, 1] = np.nan                                    # a non-finite instance inside most prefixes
    s["scale"][5_000] = np.inf
    want = run_oracle(oracle_mod, s, threads=4, first_instance_base=base, first_index_base=index_base)
    for n in (0, 1, 31, 257, 300, 301, 4_097, 65_537, big):
        part = run_oracle(oracle_mod, _prefix(s, n), first_instance_base=base, first_index_base=index_base)
        _same_frame(truncate_frame(want, n, base), part, f"n={n}")
    # the generator is prefix-stable: a scene made at the smaller size IS the prefix
    small = _scene(4_097, all_visible)
    for key in ("pos", "rot", "scale", "mesh_id"):
        assert np.array_equal(small[key], _scene(big, all_visible)[key][:4_097])


def test_a_frame_that_is_off_by_one_is_caught_by_the_gpu_tests_comparison(oracle_mod):
    s = _scene(70_000, all_visible=True)
    base = 1000
    want = run_oracle(oracle_mod, s, threads=4, first_instance_base=base, first_index_base=0xFFFFFF00)
    n = 65_537
    right = truncate_frame(want, n, base)
    assert_parity(truncate_frame(want, n, base), right, "itself")
    for wrong_n in (n - 1, n + 1):
        wrong = truncate_frame(want, wrong_n, base)
        wrong = dict(wrong, model=right["model"], world_aabb=right["world_aabb"])  # only the prefix outputs differ
        if wrong["visible_bitmap"].shape != right["visible_bitmap"].shape:
            wrong["visible_bitmap"] = np.resize(wrong["visible_bitmap"], right["visible_bitmap"].shape)
        with pytest.raises(AssertionError):
            assert_parity(wrong, right, f"n {wrong_n} for {n}")
    # one group's sum missing from every later firstIndex: what a wrong start1 or accumulator gives
    shifted = dict(right, draw_cmds=right["draw_cmds"].copy())
    tail = shifted["draw_cmds"]["firstIndex"][40_000:]
    tail -= shifted["draw_cmds"]["indexCount"][39_999]
    with pytest.raises(AssertionError, match="command bytes"):
        assert_parity(shifted, right, "shifted firstIndex")
    dropped = dict(right, draw_cmds=right["draw_cmds"][:-1], draw_count=right["draw_count"] - 1)
    with pytest.raises(AssertionError, match="draw_count"):
        assert_parity(dropped, right, "dropped command")
    total = dict(right, draw_index_total=(right["draw_index_total"] + 3) & 0xFFFFFFFF)
    with pytest.raises(AssertionError, match="draw_index_total"):
        assert_parity(total, right, "index total")
