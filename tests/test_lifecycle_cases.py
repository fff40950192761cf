"""The resident-state model (tests/context_model.py) and the lifecycle sequences (tests/lifecycle_cases.py), checked on the CPU:
the model's census is decision_cases' mirror, the sequence that flips the census by the mesh table alone really crosses the limit
with ordinary bytes, the committed walk seeds cover every (operation, probe) pair with few refusals, and every likely mistake
of the library's host side — a mutant of the model, never a wrong library — changes what exactly one named sequence expects."""
import numpy as np
import pytest

import context_model as cm
import decision_cases as dc
import lifecycle_cases as lc

F = np.float32


def _resident(case_or_scene, meshes=dc.MESHES):
    model = cm.ContextModel(len(case_or_scene["scale"]), len(meshes))
    assert model.set_mesh_table(meshes) == cm.OK
    assert model.set_instances(case_or_scene["pos"], case_or_scene["rot"], case_or_scene["scale"], case_or_scene["mesh_id"]) == cm.OK
    return model


def test_the_models_census_is_the_mirror():
    assert dc.table_box_abs(dc.MESHES) == dc.BOX_ABS and dc.table_box_abs(dc.MESHES[:0]) == 0
    some = 0
    for name, c in dc.catalogue()["cases"].items():
        model = _resident(c)
        assert model.nonfinite == dc.census_fallbacks(c) == model.fresh_census(), name
        assert model.fallback == c["fallback"], name
        some += model.fallback
    assert some >= 2
    for kind in dc.TIER_KINDS:
        for placement in dc.TIER_PLACEMENTS:
            s, twin, _ = dc.tier_scene(kind, placement)
            assert _resident(s).fallback == (dc.census_fallbacks(s) > 0) and not _resident(twin).fallback, (kind, placement)
    # the box_abs of a table of its own: the sum is the largest mesh's, in float32, and it is what the mirror is given
    t = lc.table(7)
    sums = [F(sum(abs(float(v)) for v in list(e["aabb_min"]) + list(e["aabb_max"]))) for e in t]
    assert abs(float(dc.table_box_abs(t)) - float(max(sums))) <= 4 * np.spacing(F(max(sums)))
    c = dc.case("nonfinite")
    assert _resident(c, lc.big_boxes()).nonfinite == dc.census_fallbacks(c, dc.table_box_abs(lc.big_boxes()))


def test_the_flip_sequence_crosses_the_limit_with_ordinary_bytes():
    cols, at = lc.flip_instances()
    small, big = dc.table_box_abs(dc.MESHES), dc.table_box_abs(lc.big_boxes())
    assert (float(small), float(big)) == (3.0, 30.0)
    one = {k: v[at:at + 1] for k, v in cols.items()}
    with np.errstate(all="ignore"):
        assert dc.separable_bound(one["pos"], one["rot"], one["scale"], small)[0] < dc.SEPARABLE_LIMIT        # the census-selected kernels
        assert dc.separable_bound(one["pos"], one["rot"], one["scale"], big)[0] >= dc.SEPARABLE_LIMIT         # the fall-back tiers
        assert dc.finite_magnitude(one["pos"], one["rot"], one["scale"])[0] < dc.FINITE_LIMIT
    # a factor from either edge, not a float: a fused or re-associated bound on the device decides the same
    assert 2.0 < float(dc.SEPARABLE_LIMIT) / float(dc.separable_bound(one["pos"], one["rot"], one["scale"], small)[0]) < 5.0
    assert dc.census_fallbacks(cols, small) == 0 and dc.census_fallbacks(cols, big) == 1
    # every world-box corner of every instance under both tables, in float64: finite, and a float32
    rot = dc.rotation(cols["rot"]).astype(np.float64)
    for t in (dc.MESHES, lc.big_boxes()):
        lo, hi = t["aabb_min"][cols["mesh_id"]].astype(np.float64), t["aabb_max"][cols["mesh_id"]].astype(np.float64)
        for corner in range(8):
            p = np.where([(corner >> a) & 1 for a in range(3)], hi, lo)
            world = np.einsum("nij,nj->ni", rot, p) * cols["scale"].astype(np.float64)[:, None] + cols["pos"].astype(np.float64)
            assert np.isfinite(world).all() and np.abs(world).max() < float(np.finfo(F).max) / 100
    # through the model: the table alone moves the census, both ways, and stops moving it once the odd instance is gone
    model, seen = lc.new_model(), []
    for op, kw in lc.sequence("census_by_table"):
        assert model.apply(op, **kw) == cm.OK
        seen.append(model.fallback)
    assert seen == [False, False, True, False, True, False, False]
    assert [op for op, _ in lc.sequence("census_by_table")].count("set_mesh_table") == 5


def test_the_tracked_census_is_the_fresh_count_everywhere():
    for name in lc.SEQUENCES:
        model = lc.new_model()
        for op, kw in lc.sequence(name):
            model.apply(op, **kw)
            assert model.nonfinite == model.fresh_census(), (name, op)
    for seed in lc.WALK_SEEDS:
        model = lc.new_model()
        for op, kw, _ in lc.random_walk(seed):
            model.apply(op, **kw)
            assert model.nonfinite == model.fresh_census(), (seed, op)


def test_the_sequences_meet_what_they_are_named_for():
    codes = {name: [e[0] for e in lc.expectations(name)] for name in lc.SEQUENCES}
    for name in ("census_by_table", "census_by_update", "same_size_swap", "count_down_and_up", "in_flight"):
        assert set(codes[name]) == {cm.OK}, (name, codes[name])
    assert codes["shrink_inside"].count(cm.INVALID) == 1 and codes["blas_across_tables"].count(cm.INVALID) == 1
    assert codes["refused_host_upload"] == [cm.OK, cm.OK, cm.INVALID, cm.OK, cm.INVALID, cm.NOT_READY, cm.OK, cm.CAPACITY]
    assert codes["stranding_shrink"] == [cm.OK, cm.OK, cm.OK, cm.NOT_READY, cm.OK, cm.CAPACITY]
    assert {cm.OK, cm.NOT_READY, cm.INVALID} == set(codes["clusters"])
    # the sizes: every n and m of the two sets occurs in a named sequence
    ns, ms = set(), set()
    for name in lc.SEQUENCES:
        model = lc.new_model()
        for op, kw in lc.sequence(name):
            model.apply(op, **kw)
            ns.add(model.n); ms.add(model.m)
    assert set(lc.N_SET) <= ns and set(lc.M_SET) <= ms, (ns, ms)
    # the shrink reaches one mesh with every instance still resident; the stranding shrink leaves none
    model = lc.new_model()
    for op, kw in lc.sequence("shrink_inside")[:8]:
        model.apply(op, **kw)
    assert (model.m, model.n, model.frame_ready) == (1, 769, True)
    model = lc.new_model()
    for op, kw in lc.sequence("stranding_shrink")[:3]:
        model.apply(op, **kw)
    assert (model.m, model.n, model.frame_ready) == (7, 0, False)
    # the BLAS sequence: ids at or above the old table's size meet no address until the new table has its own
    model, refs = lc.new_model(), []
    for op, kw in lc.sequence("blas_across_tables"):
        model.apply(op, **kw)
        refs.append(None if not model.frame_ready else bool(model.blas_addresses()[model.mesh_id].any()))
    assert refs == [None, None, True, False, False, False, True, False, True]
    assert int(model.mesh_id.min()) >= 7
    # the cluster sequence ends with a valid table and stale cones; it passes through every other combination
    model, states = lc.new_model(), set()
    for op, kw in lc.sequence("clusters"):
        model.apply(op, **kw)
        states.add((model.clusters_valid, model.cones_valid))
    assert states == {(False, False), (True, False), (True, True)} and (model.clusters_valid, model.cones_valid) == (True, False)


def test_walk_seeds_cover_every_pair_with_few_refusals():
    seen = set()
    for seed in lc.WALK_SEEDS:
        walk = lc.random_walk(seed)
        assert len(walk) == 40 and lc.random_walk(seed)[7][0] == walk[7][0]
        pairs, refused = lc.walk_statistics(walk)
        assert 0 < refused <= len(walk) // 4, (seed, refused)      # refusals are part of the contract, and not the whole walk
        seen |= pairs
    want = {(op, probe) for op in cm.OPERATIONS for probe in lc.PROBES}
    assert len(lc.WALK_SEEDS) == 8 and seen == want, sorted(want - seen)


def test_every_mutant_is_told_apart_by_a_named_sequence():
    base = {name: lc.expectations(name) for name in lc.SEQUENCES}
    kills = {mutant: [name for name in lc.SEQUENCES if lc.expectations(name, mutant) != base[name]] for mutant in lc.ALL_MUTANTS}
    table = "\n".join(f"  {mutant:45s} -> {', '.join(names) or 'NOTHING'}" for mutant, names in kills.items())
    assert all(kills.values()), "a mutant no named sequence tells from the contract:\n" + table
    # and no sequence is redundant: each is the ONLY one that tells some mutant apart
    for name in lc.SEQUENCES:
        assert any(names == [name] for names in kills.values()), f"{name} could be removed without losing a mutant:\n" + table
    assert lc.expectations("census_by_table") == base["census_by_table"]     # (deterministic)
