"""The designed streams of tests/range_edge_cases.py on the CPU: the oracle decides every designed triangle as designed; the
model of the decomposition (tests/range_model.py) reassembles the hand-written stream for every case; every structural edge the
catalogue promises is hit by a named case; every mutant of the model changes the stream or the counts of a named case. The GPU
side is tests/test_gpu_range_edges.py."""
import numpy as np
import pytest

import range_edge_cases as rc
import range_model as rm


@pytest.fixture(scope="module")
def cat():
    return rc.catalogue()


@pytest.fixture(scope="module")
def ra():
    import renderer_amd

    return renderer_amd


def test_rules_are_read_from_the_plan():
    """The probe prints frame_plan.hpp's rules: limits, whole steps of 64, the class of an index count, the batch of a class
    (known answers — the model never restates them), and the grid MIP_TUNE_TRI_RANGE_BLOCKS sets."""
    r = rc.rules(1000, 4, 256, [0, 2, 3, 5, 6, 3 * 255, 3 * 256, 3 * 257 + 2])
    assert (r["range_slots"], r["range_min_slots"], r["range_max_slots"]) == (256, 256, 8192)
    assert r["size_class"] == [0, 0, 0, 0, 1, 7, 8, 8]
    assert r["sort_batch"][:13] == [16] * 9 + [8, 4, 2, 1] and set(r["sort_batch"][12:]) == {1}
    assert rc.rules(4 * 1639, 4, 8192)["range_slots"] == 1664 and rc.rules(4 * 8192 + 1, 4, 8192)["range_slots"] == 8192
    assert rc.rules(cu_count=256)["range_blocks"] == 2048 and rc.rules(cu_count=256, tri_range_blocks=1)["range_blocks"] == 1
    assert rc.rules(cu_count=256, tri_range_blocks=2049)["range_blocks"] == 2048 and rc.rules(cu_count=4, tri_chunk_blocks_per_cu=5, tri_range_blocks=20)["range_blocks"] == 20


def test_keep_patterns():
    for n in (0, 1, 63, 64, 65, 200):
        assert rc.keep_pattern("all", n).sum() == n and rc.keep_pattern("none", n).sum() == 0
        assert np.nonzero(rc.keep_pattern("alternating", n))[0].tolist() == list(range(0, n, 2))
        assert np.nonzero(rc.keep_pattern("lane63", n))[0].tolist() == list(range(63, n, 64))
        assert np.nonzero(rc.keep_pattern("first", n))[0].tolist() == ([0] if n else [])
        assert np.nonzero(rc.keep_pattern("last", n))[0].tolist() == ([n - 1] if n else [])
    k = rc.keep_pattern("random", 4000, 3)
    assert 1800 < k.sum() < 2200 and not np.array_equal(k, rc.keep_pattern("random", 4000, 4))


def test_the_oracle_decides_every_designed_triangle_as_designed(cat, ra, oracle_mod):
    """Every case through oracle.run + oracle.cull_all_triangles: the frame's commands are the designed stream (every instance
    visible, firstIndex the running sum from first_index_base), and the final commands and the culled stream are the
    hand-written ones — so every triangle of every mesh was decided as its pattern says."""
    table, cases = cat
    meshes, vertices, indices = table.build(ra)
    pv = ra.scene.default_pv()
    seen = set()
    for case in cases.values():
        key = (case.mesh_ids.tobytes(), case.base)
        if key in seen:
            continue
        seen.add(key)
        s = rc.scene_of(ra, meshes, case.mesh_ids)
        base = case.base if case.base < (1 << 28) else case.base % 3 + 6     # (the oracle writes from word 0: a high base is checked modulo its phase)
        r = oracle_mod.run(s["pos"], s["rot"], s["scale"], s["mesh_id"], meshes, s["planes"], s["cam_pos"], first_index_base=base, threads=4)
        st = case.stream
        assert r["draw_count"] == len(st) and r["draw_index_total"] == st.index_total, case.name
        assert np.array_equal(r["draw_cmds"]["indexCount"], st.ic) and np.array_equal(r["draw_cmds"]["firstIndex"], st.first_index - case.base + base), case.name
        full = base + st.index_total + 3
        want_cmds, want_out, _ = oracle_mod.cull_all_triangles(r, s["pos"], s["mesh_id"], meshes, s["cam_pos"], pv, vertices, indices, out_capacity=full)
        final, hand = rm.expected_direct(rm.Stream(st.ic, base), case.keeps, full)
        assert np.array_equal(want_out, hand), case.name
        live = np.nonzero(final)[0]
        assert np.array_equal(want_cmds["indexCount"], final[live]) and np.array_equal(want_cmds["firstInstance"], case.instances[live]), case.name
        if case.status == 0:
            mine = case.expected_cmds(ra)
            mine["firstIndex"] = mine["firstIndex"].astype(np.int64) - case.base + base
            assert mine.tobytes() == want_cmds.tobytes(), case.name


def test_the_model_reassembles_the_hand_written_stream(cat):
    """The decomposition — range map, segments, granules, look-backs, deferred writes — puts every survivor where the design
    says, capacity cases included; S is what the probe says for the stream; the sorted path visits every command once."""
    for case in cat[1].values():
        final, hand = case.expected()
        if case.sorted:
            sort = case.sort()
            assert (sort["visits"] == 1).all() and sort["stale"] == 0, case.name
            lo_n = case.words()
            f2, s2 = rm.sorted_stream(case.stream, case.keeps, case.capacity, sort, window=lo_n)
            assert np.array_equal(f2, final) and np.array_equal(s2, hand), case.name
            starts = sort["start"].tolist() + [len(case.stream)]
            assert sorted(sort["order"][: len(case.stream)].tolist()) == list(range(len(case.stream))), case.name
            for d, first, n_cmds in sort["tickets"]:   # a ticket is commands of ONE class
                assert n_cmds >= 1 and starts[d] <= first and first + n_cmds <= starts[d + 1], (case.name, d, first, n_cmds)
        else:
            d = case.decompose()
            assert np.array_equal(d["final"], final) and np.array_equal(d["stream"], hand), case.name
            assert all(n <= rm.MASK_STEPS for n in d["deferred_steps"].values()), case.name
            assert (d["first"] < len(case.stream)).all(), case.name


def test_every_edge_is_hit_by_a_named_case(cat):
    hit = {}
    for case in cat[1].values():
        if case.tuning == "stage_ranges_256":
            continue
        for e in (case.sort()["edges"] if case.sorted else case.decompose()["edges"]):
            hit.setdefault(e, []).append(case.name)
    missing = [e for e in rc.RANGE_EDGES + rc.SORT_EDGES if e not in hit]
    assert not missing, missing
    # the cases named for an edge hit it
    for name in ("n_ranges=n_waves-1", "n_ranges=n_waves", "n_ranges=n_waves+1"):
        assert hit[name] and any(n.startswith("n_ranges_") for n in hit[name])
    for n in (2, 3, 64, 65, 66, 128, 129, 130):
        assert f"spans_{n}_last_1" in hit[f"spans_{n}_ranges"] and f"spans_{n}_last_S" in hit[f"spans_{n}_ranges"]
    assert "spans_65_last_1" in hit["lookback_of_exactly_one_group"] and "spans_66_last_1" in hit["lookback_last_group_of_one_range"]
    assert "continuing_128_127_steps_at_the_largest_S" in hit["continuing_segment_of_128_steps"]
    for name in rc.LONG_LOOKBACK:
        assert "lookback_in_several_groups" in cat[1][name].decompose()["edges"] or "lookback_of_exactly_one_group" in cat[1][name].decompose()["edges"], name


# the case that kills each mutant (more do; one is named)
KILLED_BY = {
    "ends_here_strict": "boundary_ends_and_lengths",
    "lookback_first_range_ceiling": "spans_2_last_1",
    "lookback_nearest_group_only": "spans_66_last_1",
    "granule_of_first_segment": "spans_3_last_S",
    "prev_end_without_gaps": "gaps_in_front_of_a_crossing_command",
    "range_slots_not_rounded": "continuing_24_25_steps",
    "batch_tail_dropped": "continuing_11_12_13_steps",
    "mask_buffers_aliased": "one_command_of_130_ranges",
    "ticket_past_class_end": "sorted_class_populations_batch+1",
    "class_of_power_of_two_low": "sorted_powers_of_two_k_0_to_14",
    "copy_offsets_ignored": "sorted_more_than_2048_commands",
}


@pytest.mark.parametrize("mutant", rm.MUTANTS)
def test_every_mutant_of_the_model_is_killed_by_a_named_case(cat, mutant):
    """One mistake in the decomposition each: the expected stream, the final counts or the counts of the decomposition (ranges,
    granules, steps; classes, tickets, visits) of the named case change."""
    case = cat[1][KILLED_BY[mutant]]
    if mutant in rm.SORT_MUTANTS:
        good, bad = case.sort(), case.sort(mutant)
        same = all(np.array_equal(good[k], bad[k]) for k in ("start", "visits")) and good["stale"] == bad["stale"] and good["tickets"] == bad["tickets"]
    else:
        good, bad = case.decompose(), case.decompose(mutant)
        same = all(np.array_equal(good[k], bad[k]) for k in ("stream", "final", "granules")) and good["n_ranges"] == bad["n_ranges"] and \
            good["deferred_steps"] == bad["deferred_steps"]
        if mutant != "range_slots_not_rounded":   # these change what the frame ENDS with, not only how it is cut
            assert not (np.array_equal(good["stream"], bad["stream"]) and np.array_equal(good["final"], bad["final"])), mutant
    assert not same, mutant
    assert mutant in KILLED_BY and set(KILLED_BY) == set(rm.MUTANTS)
