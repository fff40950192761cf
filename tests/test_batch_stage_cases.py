"""The designed streams of the binning stage (tests/batch_stage_cases.py) on the CPU: for every case and every entry point it
applies to, three expectations agree byte for byte — by construction from the labels, the numpy restatements (which derive bucket
and depth from the positions by the float32 rules) and the structural model (tests/batch_stage_model.py, whose plans come from
batch_plan.hpp through tests/native/batch_plan_probe.cpp); every named edge is hit and every case hits the edges it claims; every
mutant of the model changes the output of its named case. No GPU."""
import functools

import numpy as np
import pytest

import batch_merge_restatement as bmr
import batch_restatement as br
import batch_stage_cases as bc
import batch_stage_model as sm
import lod_restatement as lr
import order_restatement as orr
import sorted_restatement as sr
import views_batch_restatement as vr

KEYS = {"views": ("cmds", "counts", "first_slot", "ids"), "shard": ("chunk",)}
SINGLE = ("cmds", "count", "ids", "members")
FAMILIES = ("tile", "rowscan", "passes", "writer", "views", "keys")


def _words(cmds):
    return np.ascontiguousarray(cmds).view(np.uint32).reshape(-1, 5)


def whole(want, n, room):
    """A single-view expectation as the buffers a call leaves: `room` command rows and n + 3 ids, a sentinel wherever nothing is written."""
    cmds = np.full((room, 5), bc.SENTINEL, np.uint32)
    cmds[: want["count"]] = _words(want["cmds"])
    ids = np.full(n + 3, bc.SENTINEL, np.uint32)
    ids[: want["members"]] = want["ids"]
    return dict(cmds=cmds, count=want["count"], ids=ids, members=want["members"])


def _room(case, call):
    return (case.n if call.entry == "sorted" else min(case.n_buckets, case.n)) + 3


def by_construction(case, call):
    want = bc.expect(case, call)
    return want if call.entry in KEYS else whole(want, case.n, _room(case, call))


def by_restatement(case, call):
    s, sw = case.scene(), bc.PIN_SWITCH_SQ
    a = (s["pos"], s["scale"], s["mesh_id"], s["meshes"], s["cam"], s["bitmap"], lr.DISTANCE, sw)
    if call.entry == "views":
        v = case.view_spec()
        V = len(v["bucket"])
        want = vr.batch_draws_views(s["pos"], s["scale"], s["mesh_id"], s["meshes"], [case.cam] * V, v["bitmaps"], v["bases"], lr.DISTANCE, sw)
        return vr.fill_outputs(want, case.n, case.cmd_stride(), bc.SENTINEL, 3, first_slot=v["first_slot"])
    if call.entry == "shard":
        return dict(chunk=bmr.shard_chunk(*a, bc.BASE, case.n, fill=bc.SENTINEL))
    if call.entry == "draws":
        want = br.batch_draws(s["pos"], s["mesh_id"], s["meshes"], s["cam"], s["bitmap"], first_instance_base=bc.BASE)
    elif call.entry == "lods":
        want = lr.batch_draws_lods(*a, first_instance_base=bc.BASE)
    elif call.entry == "ordered":
        want = orr.batch_draws_ordered(*a, call.order, first_instance_base=bc.BASE)
    else:
        metric, order, bits, axis = call.sort
        want = sr.batch_draws_sorted(*a, metric, order, bits, axis, first_instance_base=bc.BASE)
    return whole(want, case.n, _room(case, call))


def by_model(case, call, scratch=None, mutant=None):
    kw = dict(base=bc.BASE, want_model=call.model, scratch=scratch, mutant=mutant)
    if call.entry == "views":
        v = case.view_spec()
        kw["views"] = dict(cams=[case.cam] * len(v["bucket"]), bitmaps=v["bitmaps"], bases=v["bases"], stride=case.cmd_stride(), first_slot=v["first_slot"])
    elif call.entry == "shard":
        kw["capacity"] = case.n
    elif call.entry == "ordered":
        kw["order"] = call.order
    elif call.entry == "sorted":
        kw["sort"] = call.sort
    return sm.run(call.entry, case.scene(), **kw)


def differences(a, b, entry):
    return [k for k in KEYS.get(entry, SINGLE) if (a[k].tobytes() != b[k].tobytes() if isinstance(a[k], np.ndarray) else int(a[k]) != int(b[k]))]


@functools.lru_cache(maxsize=None)
def evaluate(name):
    """Every call of the case through the three expectations: the disagreements found (none, if all is well) and the edges hit."""
    case = bc.case(name)
    wrong, edges = [], set()
    for call in case.calls:
        built, restated = by_construction(case, call), by_restatement(case, call)
        modelled, hit = by_model(case, call)
        edges |= hit
        for what, other in (("restatement", restated), ("model", modelled)):
            d = differences(built, other, call.entry)
            if d:
                wrong.append((name, call, what, d))
    return wrong, frozenset(edges)


@functools.lru_cache(maxsize=None)
def sequence_edges():
    """The sequences on one Scratch each (one context, one frame slot): every call still gives the expectation by construction."""
    wrong, edges = [], set()
    for seq in bc.SEQUENCES:
        for call in (bc.LODS, bc.SHARD):
            scratch = sm.Scratch()
            for name in seq:
                case = bc.case(name)
                out, hit = by_model(case, call, scratch=scratch)
                edges |= hit
                if differences(by_construction(case, call), out, call.entry):
                    wrong.append((seq, name, call))
    return wrong, frozenset(edges)


@pytest.mark.parametrize("family", FAMILIES)
def test_three_expectations_agree(family):
    names = [c.name for c in bc.all_cases() if c.family == family]
    assert names
    for name in names:
        wrong, _ = evaluate(name)
        assert not wrong, wrong


def test_the_families_are_the_catalogue():
    assert {c.family for c in bc.all_cases()} == set(FAMILIES)


def test_labels_are_what_the_float32_rules_give():
    """The depth labels against the restatements' own depth functions, member by member (the outputs could agree by accident)."""
    for c in bc.all_cases():
        live = c.bucket >= 0
        for call in c.calls:
            if call.entry == "ordered":
                assert np.array_equal(orr.depth_key(c.pos, c.cam, orr.NEAR_FIRST)[live], c.K[live]), c.name
            if call.entry == "sorted":
                assert np.array_equal(sr.depth_u(c.pos, c.cam, sr.VIEW_AXIS, bc.AXIS)[live], c.U[live]), c.name
    x, k = bc.ordered_x(3, 9)
    assert float(x) == 12.5 and k == 0x431C


def test_sequences_on_one_scratch():
    wrong, edges = sequence_edges()
    assert not wrong, wrong
    assert "stale_keys_behind_members" in edges


def test_every_edge_is_hit():
    hit = set(sequence_edges()[1])
    for c in bc.all_cases():
        hit |= evaluate(c.name)[1]
    assert not set(bc.EDGES) - hit, sorted(set(bc.EDGES) - hit)
    claimed = set().union(*(c.edges for c in bc.all_cases())) | {"stale_keys_behind_members"}
    assert not set(bc.EDGES) - claimed, sorted(set(bc.EDGES) - claimed)     # and by a case that was designed for it


def test_every_case_hits_the_edges_it_claims():
    for c in bc.all_cases():
        missing = c.edges - evaluate(c.name)[1]
        assert not missing, (c.name, sorted(missing))


# every mutant, the case that kills it and the call it is killed through
KILLERS = {
    "match_without_valid": ("bucket_0_beside_clear_bits", bc.LODS),
    "row_reset_every_round": ("bin_in_rounds_0_and_3", bc.LODS),
    "wave_base_skips_previous": ("bin_fills_a_tile", bc.LODS),
    "digits_below_reset_at_seam": ("bins_63_and_64", bc.LODS),
    "rowscan_carry_dropped": ("rowscan_257_tiles", bc.LODS),
    "rowscan_carry_last_nonzero_chunk": ("rowscan_513_tiles", bc.LODS),
    "idle_lane_is_member": ("n1025_last_member", bc.LODS),
    "list_pass_over_n": ("members_1_S257d", bc.LODS),
    "list_pass_reversed_in_tile": ("two_digits_low_equal", bc.LODS),
    "cmds_before_not_carried": ("buckets_255_256", bc.LODS),
    "members_before_not_carried": ("buckets_255_256", bc.LODS),
    "view_first_cmd_current_chunk_only": ("view_in_two_chunks", bc.VIEWS),
    "hist_copy_0_only": ("every_histogram_copy", bc.VIEWS),
    "ordered_bucket_of_is_key": ("ordered_keys", bc.ORDERED_NEAR),
    "far_first_flips_whole_key": ("ordered_keys", bc.ORDERED_FAR),
}


def test_every_mutant_has_a_killer():
    assert set(KILLERS) == set(sm.MUTANTS)


@pytest.mark.parametrize("mutant", sm.MUTANTS)
def test_mutant_is_killed_by_its_named_case(mutant):
    name, call = KILLERS[mutant]
    case = bc.case(name)
    assert call in case.calls
    built = by_construction(case, call)
    plain, _ = by_model(case, call)
    assert not differences(built, plain, call.entry)
    wrong, _ = by_model(case, call, mutant=mutant)
    assert differences(built, wrong, call.entry), (mutant, name)


def test_the_plans_are_the_headers():
    """The probe prints what batch_plan.hpp computes: the pass edges every table of the catalogue was sized for."""
    for buckets, passes in ((1, 1), (256, 1), (257, 2), (65536, 2), (65537, 3)):
        assert sm.plan("lods", 0, buckets, 0, 0)["passes"] == passes
    assert sm.plan("ordered", 0, 65536, 0, 0)["passes"] == 4 and sm.plan("views", 0, 320, 0, 0)["pass"][1]["launch"][3][0] == "views_list_last"
    assert [sm.plan("sorted", 0, 1, b, 0, 0)["passes"] for b in (16, 24, 32)] == [2, 3, 4]
    assert sm.hist_copies_for(True, 320) == 64 and sm.hist_copies_for(False, 320) == 1 and sm.hist_copies_for(True, 1 << 15) == 32
