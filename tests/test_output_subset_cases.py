"""tests/output_subset_cases.py on the CPU: the subsets are exactly what plan_frame accepts, the scene is not vacuous where
the kernel's guards are, the comparison accepts the oracle's own frame for every subset at every size — and rejects every
wrong pipeline of mutants(), for a (subset, size) that the test names. No GPU."""
import numpy as np
import pytest

import output_subset_cases as osc
import plan_boundaries as pb
from cpu_pipeline import OraclePipeline
from renderer_amd.pipeline import make_frame

_frames = {}


def _scene_and_frame(oracle_mod, n):
    if n not in _frames:
        s = osc.subset_scene(n)
        _frames[n] = (s, osc.oracle_frame(oracle_mod, s))
    return _frames[n]


def _run(pipe, s, subset):
    outs = osc.SubsetOutputs(osc.NumpyBackend(), s["n"], subset)
    pipe.run_device(make_frame(s["planes"], s["cam_pos"], first_instance_base=s["base"], first_index_base=s["index_base"]), **outs.pointers())
    return outs


def _pipeline(s):
    p = OraclePipeline(s)
    p.set_blas_addresses(s["blas"])
    return p


def test_there_are_48_subsets_with_distinct_ids():
    assert len(osc.SUBSETS) == 48 and len(set(osc.SUBSETS)) == 48
    assert osc.EMPTY in osc.SUBSETS and osc.ALL in osc.SUBSETS
    ids = [osc.subset_id(s) for s in osc.SUBSETS]
    assert len(set(ids)) == 48 and "none" in ids and "m-t-a-b-c-i" in ids
    assert all(osc.subset_of(i) == s for i, s in zip(ids, osc.SUBSETS))


def test_subsets_are_exactly_what_plan_frame_accepts():
    """All 64 combinations of {model, tlas, aabb, bitmap, draw_cmds + draw_count, draw_index_total} through the probe."""
    accepted = set()
    for combo in osc._all_combinations():
        p = osc.probe_status(osc.plan_request(combo).split(",") if combo else [])
        if p["status"] == 0:
            accepted.add(combo)
    assert accepted == set(osc.SUBSETS), sorted(osc.subset_id(s) for s in accepted ^ set(osc.SUBSETS))
    # draw_cmds and draw_count go together, whatever else is asked for
    for words in (["draw_cmds"], ["count"], ["model", "draw_cmds"], ["bitmap", "count", "index_total"]):
        assert osc.probe_status(words)["status"] != 0, words
    # the probe's own word `cmds` is draw_cmds + count + index_total
    assert pb.plan(1000, "cmds") == pb.plan(1000, osc.plan_request({"cmds", "index_total"}))


def test_both_orders_and_both_prefix_uses_occur_at_the_test_sizes():
    seen = set()
    for n in osc.SIZES:
        for subset in osc.SUBSETS:
            for order in (1, 3):
                p = pb.plan(n, osc.plan_request(subset), force_order=order)
                if n == 0:
                    assert p["empty"] == 1
                    continue
                assert p["order"] == order and p["uses_prefix_state"] == int("cmds" in subset), (n, osc.subset_id(subset), p)
                seen.add((p["order"], p["uses_prefix_state"]))
            own = pb.plan(n, osc.plan_request(subset))
            assert n == 0 or own["order"] == 3           # sizes this small are one generation of workgroups
    assert seen == {(1, 0), (1, 1), (3, 0), (3, 1)}
    assert pb.plan(4129, osc.plan_request(osc.ALL))["n_tiles"] == 17 and pb.plan(4129, osc.plan_request(osc.ALL))["group_shift"] == 4
    assert pb.plan(1000, "model")["tile"] == osc.TILE


@pytest.mark.parametrize("n", list(osc.SIZES))
def test_scene_conditions(oracle_mod, n):
    s, want = _scene_and_frame(oracle_mod, n)
    assert s["n"] == n and len(s["pos"]) == n
    osc.scene_conditions(oracle_mod, s, want)
    if n:   # the unedited instances are make_scene(3)'s
        from renderer_amd import scene

        plain = scene.make_scene(3, n=n)
        edited = {0, 1, 2, n - 1}
        keep = np.array([i not in edited for i in range(n)])
        assert np.array_equal(plain["pos"][keep], s["pos"][keep]) and np.array_equal(plain["mesh_id"][keep], s["mesh_id"][keep])


@pytest.mark.parametrize("n", list(osc.SIZES))
def test_every_subset_passes_through_the_oracle_pipeline(oracle_mod, n):
    s, want = _scene_and_frame(oracle_mod, n)
    pipe = _pipeline(s)
    for subset in osc.SUBSETS:
        outs = _run(pipe, s, subset)
        outs.check(oracle_mod, s, want, n, s["base"], f"oracle pipeline n={n}")
        if n == 0 or not subset:
            for name, b in outs.buf.items():
                assert (b == osc.SENTINEL).all(), (n, name)


def test_wire_forms_pass_through_the_oracle_pipeline(oracle_mod):
    s, want = _scene_and_frame(oracle_mod, 1000)
    pipe = _pipeline(s)
    frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=s["base"], first_index_base=s["index_base"])
    for wire in (True, "packed"):
        outs = osc.SubsetOutputs(osc.NumpyBackend(), 1000, {"cmds", "bitmap"}, wire=wire)
        pipe.run_device(frame, wire=wire, **outs.pointers())
        outs.check(oracle_mod, s, want, 1000, s["base"], f"wire={wire}")


def _kills(oracle_mod, factory, n, subset):
    s, want = _scene_and_frame(oracle_mod, n)
    outs = _run(factory(_pipeline(s)), s, subset)
    try:
        outs.check(oracle_mod, s, want, n, s["base"], "mutant")
    except AssertionError as e:
        return str(e).split("\n")[0]
    return None


@pytest.mark.parametrize("name", [name for name, _ in osc.mutants()])
def test_every_mutant_is_killed(oracle_mod, name):
    factory = dict(osc.mutants())[name]
    killed = {}
    for n in osc.SIZES:
        for subset in osc.SUBSETS:
            why = _kills(oracle_mod, factory, n, subset)
            if why:
                killed[(osc.subset_id(subset), n)] = why
    assert killed, f"no (subset, size) notices: {name}"
    first = sorted(killed, key=lambda k: (k[1], k[0]))[0]
    print(f"[mutant] {name}: killed by {len(killed)} (subset, size) pairs, first {first}: {killed[first]}")
    # the cases that must bite, by name
    expected = {
        "bitmap written only when commands are": ("b", 1),
        "last bitmap word of a ragged tile dropped when there are no commands": ("b", 1000),
        "TLAS rows taken from the matrix of the previous frame when model is NULL": ("t", 1),
        "one row past n written for tlas": ("t", 257),
        "one row past n written for model": ("m", 257),
        "one row past n written for aabb": ("a", 257),
        "draw_index_total written through a NULL request (into the word behind draw_count)": ("c", 1),
        "BLAS address of mesh 0 for every row": ("t", 33),
        "boxes of wave 0 missing when commands are requested": ("a-c", 1),
    }[name]
    assert expected in killed, (name, expected, sorted(killed)[:8])
    # ... and a mutant is wrong only where its name says: the full frame without the mutated output still passes
    untouched = {"bitmap written only when commands are": "m-t-a-b-c-i", "last bitmap word of a ragged tile dropped when there are no commands": "m-t-a-b-c-i",
                 "TLAS rows taken from the matrix of the previous frame when model is NULL": "m-t-a-b-c-i",
                 "draw_index_total written through a NULL request (into the word behind draw_count)": "m-t-a-b-c-i",
                 "boxes of wave 0 missing when commands are requested": "m-t-a-b"}.get(name)
    if untouched:
        assert all((untouched, n) not in killed for n in osc.SIZES), (name, untouched)
