"""The catalogue of decision-edge scenes (tests/decision_cases.py) pinned on the CPU, so that the GPU comparison
(tests/test_gpu_decision_edges.py) cannot pass without exercising anything: every label class exists for every plane slot,
view and reference point; the labelled margins and squared distances are what the labels say (numpy_restatement, float32);
the C oracle and the restatement agree on every case; float64 calls every tie undecided; and five mutants of the restatement
— never of a kernel — each flip labelled instances in every kernel's input set."""
import numpy as np
import pytest

import decision_cases as dc
import float64_reference
import numpy_restatement as nr
from helpers import float_mismatches, run_oracle

F = np.float32
TIE_CLASSES = ("tie0", "ulp_in", "ulp_out", "edge_in", "edge_out", "sub_zero", "sub_pos", "sub_neg")


def _classes(c, **where):
    return {l["cls"] for l in c["labels"] if all(l.get(k) == v for k, v in where.items())}


def test_every_class_for_every_slot_view_and_reference_point():
    cat = dc.catalogue()
    for p in range(6):
        assert _classes(dc.case("axis"), frame="axis", slot=p) == {"tie0", "ulp_in", "ulp_out"}
        assert {l["k"] for l in dc.case("axis")["labels"] if l["slot"] == p} == set(range(-4, 5))
        assert _classes(dc.case("subnormal"), frame="subnormal", slot=p) >= {"sub_zero", "sub_pos", "sub_neg"}
        assert _classes(dc.case("camera"), frame="camera", slot=p) >= {"edge_in", "edge_out"}
        for v in range(4):
            assert _classes(dc.case("views"), frame=f"view{v}", slot=p) >= {"edge_in", "edge_out"}, (v, p)
    assert "tie0" in _classes(dc.case("camera"), frame="camera")
    for v in range(4):
        assert "tie0" in _classes(dc.case("views"), frame=f"view{v}")
        assert _classes(dc.case("views"), ref=f"view{v}") == set(dc.ring_classes())
    assert _classes(dc.case("camera"), ref="camera") == set(dc.ring_classes())
    assert len(cat["lights"]) == 16
    for l in range(16):
        assert _classes(dc.case("lights"), ref=f"light{l}") == set(dc.ring_classes(nan=True))
    assert _classes(dc.case("subnormal")) >= {"diff_pos", "diff_neg"}
    assert _classes(dc.case("nonfinite")) == {"inf_minus_inf", "pos_inf", "neg_inf", "nan_e", "special_plane", "sq_nan"}
    for name in dc.VIEW_INPUTS:                       # the views kernel sees every class of every case it is made of
        assert _classes(dc.case(name)) >= set(TIE_CLASSES) | set(dc.ring_classes())
    # every mesh kind (two LODs, one LOD, LOD 0 / LOD 1 / both empty) meets the threshold floats
    for cls in ("sq_100", "sq_near_max", "sq_far1"):
        assert {int(dc.case("lights")["mesh_id"][l["index"]]) for l in dc.case("lights")["labels"] if l["cls"] == cls} == {0, 1, 2, 3, 4}
    assert len({tuple(v[0].tolist()) for k, v in cat["frames"].items() if k.startswith("view")}) == 4


@pytest.mark.parametrize("name", ["axis", "camera", "views", "subnormal", "nonfinite", "lights"])
def test_labels_say_what_the_float32_chain_computes(name):
    c, cat = dc.case(name), dc.catalogue()
    tiny = dc.TINY
    for frame in {l["frame"] for l in c["labels"] if l.get("frame")}:
        s = dc.scene_of(c, frame)
        mins, maxs = dc.boxes(s)
        with np.errstate(all="ignore"):
            sd, e = nr.plane_terms(mins, maxs, s["planes"])
            m = sd - e
            others_clear = lambda i, p: bool((np.delete(m[i], p) < 0).all())
        for l in c["labels"]:
            if l.get("frame") != frame or l["slot"] is None:
                continue
            i, p, cls = l["index"], l["slot"], l["cls"]
            what = (name, l)
            if cls in ("tie0", "sub_zero"):
                assert m[i, p] == 0 and others_clear(i, p), what
            elif cls in ("ulp_out", "edge_out"):
                assert m[i, p] > 0, what
            elif cls in ("ulp_in", "edge_in"):
                assert m[i, p] <= 0 and others_clear(i, p), what
            if cls in ("ulp_in", "ulp_out"):          # the centre k floats from the tie, outwards (k > 0) or inwards
                tie = [t for t in c["labels"] if t["slot"] == p and t["cls"] == "tie0" and c["scale"][t["index"]] == 1.0][0]
                axis = dc.AXIS_TIE[p][0]
                at = c["pos"][tie["index"], axis]
                assert c["pos"][i, axis] == dc._step(at, l["k"] * (1 if at > 0 else -1)), what
                assert m[i, p] != 0 and np.sign(m[i, p]) == np.sign(l["k"]), what
            if cls.startswith("sub_"):
                assert 0 < abs(sd[i, p]) < tiny and 0 < abs(e[i, p]) < tiny, what
                assert (cls == "sub_pos" and 0 < m[i, p] < tiny) or (cls == "sub_neg" and -tiny < m[i, p] < 0) or (cls == "sub_zero"), what
            if cls.startswith("far_"):
                assert 0 < abs(m[i, p]) < tiny and (m[i, p] > 0) == (cls == "far_pos"), what
            if cls.startswith("diff_"):
                assert abs(sd[i, p]) >= tiny and e[i, p] >= tiny and 0 < abs(m[i, p]) < tiny and (m[i, p] > 0) == (cls == "diff_pos"), what
            if cls == "inf_minus_inf":
                assert sd[i, p] == np.inf and e[i, p] == np.inf and np.isnan(m[i, p]), what
            if cls in ("pos_inf", "neg_inf"):
                assert sd[i, p] == (np.inf if cls == "pos_inf" else -np.inf) and np.isfinite(e[i, p]) and m[i, p] == sd[i, p], what
            if cls == "nan_e":
                assert np.isnan(e[i, p]) and (s["planes"][4 * p : 4 * p + 3] == 0).any() and np.isinf(maxs[i]).any(), what
            if cls in ("inf_minus_inf", "pos_inf", "neg_inf", "nan_e"):
                assert np.isfinite(c["pos"][i]).all() and np.isfinite(c["scale"][i]), what
    special = cat["frames"]["special"][0]
    assert np.isnan(special).any() and np.isposinf(special).any() and np.isneginf(special).any() and (special == F(3.4e38)).any()
    assert np.signbit(special[special == 0]).any() and not np.signbit(special[special == 0]).all()
    for l in c["labels"]:
        if not l.get("ref"):
            continue
        with np.errstate(all="ignore"):
            sq = nr.dist_sq(c["pos"][l["index"]][None, :], cat["refs"][l["ref"]])[0]
            far = bool(nr.lod_is_far(np.array([sq], F))[0])
        cls = l["cls"]
        if cls in dict(dc.LOD_RING):
            assert sq == dc.lod_ring_value(cls), (name, l)
            assert far == (dict(dc.LOD_RING)[cls] >= 2), (name, l)
        elif cls == "on_top":
            assert sq == 0 and not far
        elif cls == "sq_inf":
            assert sq == np.inf and far and np.isfinite(c["pos"][l["index"]]).all()
        elif cls == "sq_nan":
            assert np.isnan(sq) and not far
    assert dc.lod_ring_value("sq_100") == F(100.0) and dc.lod_ring_value("sq_near_max") == dc.NEAR_MAX == np.nextafter(F(100.0), F(np.inf))
    assert dc.lod_ring_value("sq_far1") == np.nextafter(dc.NEAR_MAX, F(np.inf))


def _oracle_equals_restatement(oracle_mod, s, what, base=0, index_base=0):
    want = run_oracle(oracle_mod, s, first_instance_base=base, first_index_base=index_base)
    got = nr.run(s, first_instance_base=base, first_index_base=index_base)
    n = s["n"]
    assert np.array_equal(got["coarse_culled"], want["coarse_culled"].astype(bool)), what
    bits = np.unpackbits(want["visible_bitmap"].view(np.uint8), bitorder="little")[:n].astype(bool)
    assert np.array_equal(bits, ~got["coarse_culled"]), what
    cmds = want["draw_cmds"]
    assert want["draw_count"] == len(got["cmds"]["indexCount"]) and want["draw_index_total"] == got["cmds"]["total"], what
    for field in ("indexCount", "firstIndex", "vertexOffset", "firstInstance"):
        assert np.array_equal(cmds[field], got["cmds"][field]), (what, field)
    assert (cmds["instanceCount"] == 1).all(), what
    assert len(float_mismatches(got["world_aabb"], want["world_aabb"])) == 0, what
    assert len(float_mismatches(got["model"], want["model"])) == 0, what
    return want


def test_oracle_equals_restatement_on_every_case(oracle_mod):
    cat = dc.catalogue()
    for name, c in cat["cases"].items():
        for frame in c["frames"]:
            _oracle_equals_restatement(oracle_mod, dc.scene_of(c, frame), (name, frame), base=5, index_base=0xFFFFFFF0)
    for name, frame in dc.RUN_INPUTS:
        for n in dc.SIZES:
            _oracle_equals_restatement(oracle_mod, dc.layout(name, n, frame)[0], (name, frame, n))
    for kind in dc.TIER_KINDS:
        for placement in dc.TIER_PLACEMENTS:
            s, twin, _ = dc.tier_scene(kind, placement)
            _oracle_equals_restatement(oracle_mod, s, (kind, placement))
            _oracle_equals_restatement(oracle_mod, twin, (kind, placement, "twin"))
    c = dc.case("lights")
    for k in (1, 2, 16):
        want = oracle_mod.light_draw_lists(c["pos"], c["mesh_id"], dc.MESHES, cat["lights"][:k], first_instance_base=3)
        got = nr.light_draw_lists(c["pos"], c["mesh_id"], dc.MESHES, cat["lights"][:k], first_instance_base=3)
        assert want.view(np.uint32).reshape(k, -1, 5).tobytes() == got.astype(np.uint32).tobytes(), k


def test_float64_calls_every_tie_undecided_and_agrees_where_it_decides(oracle_mod):
    """The evidence that the labelled instances sit ON an edge: the float64 evaluation of the formulas cannot decide them, and
    where it can decide an instance the oracle decides the same (the overflow scenes are left out: float64 does not overflow)."""
    seen = 0
    for name, frame in dc.RUN_INPUTS:
        if name == "nonfinite":
            continue
        c = dc.case(name)
        s = dc.scene_of(c, frame)
        ref = float64_reference.run(s)
        want = run_oracle(oracle_mod, s)
        decided = ref["decided"]
        assert np.array_equal(ref["culled"][decided], want["coarse_culled"].astype(bool)[decided]), (name, frame)
        for l in c["labels"]:
            if l.get("frame") == frame and l["cls"] in TIE_CLASSES:
                assert not decided[l["index"]], (name, l)
                seen += 1
            elif l.get("frame", frame) != frame and l["cls"] in TIE_CLASSES:   # another view's tie is CLEARLY in or out of this one
                assert decided[l["index"]], (name, frame, l)
    assert seen > 150


@pytest.mark.parametrize("mutant", dc.MUTANTS)
def test_each_mutant_flips_labelled_instances_in_every_kernels_input_set(mutant):
    """Only the restatement is mutated (decision_cases.decide); no wrong kernel is ever built or run. The shadow lists make
    no plane decision: the three plane mutants cannot change them, and are asserted not to."""
    for kernel in dc.KERNEL_INPUTS:
        count = dc.mutant_flips(kernel, mutant)
        print(f"{mutant}: {count} labelled instances of the input set of {kernel} change")
        if kernel == "light_draw_lists" and mutant in dc.PLANE_MUTANTS:
            assert count == 0
        else:
            assert count > 0, (kernel, mutant)


def test_tier_edges_and_their_twins():
    inst = dc.tier_edge_instances()
    down = lambda x: np.nextafter(F(x), F(0))
    for limit_name, limit, fn in (("sep", dc.SEPARABLE_LIMIT, dc.separable_bound), ("fin", dc.FINITE_LIMIT, dc.finite_magnitude)):
        for via in ("scale", "pos"):
            (pb, rb, sb), (pa, ra_, sa) = inst[(limit_name + "_below", via)], inst[(limit_name + "_at", via)]
            below, at = fn(pb, rb, sb)[0], fn(pa, ra_, sa)[0]
            assert below < limit <= at and np.isfinite(at), (limit_name, via)
            moved = (sb, sa) if via == "scale" else (pb[0], pa[0])
            assert np.nextafter(moved[0], F(np.inf)) == moved[1], (limit_name, via)      # neighbouring inputs
        below, at = fn(*inst[(limit_name + "_below", "pos")])[0], fn(*inst[(limit_name + "_at", "pos")])[0]
        assert below == down(limit) and at == limit, limit_name                          # the last float below, the first at
    expect = {"sep_below": 0, "sep_at": 1, "fin_below": 1, "fin_at": 2}
    for kind in dc.TIER_KINDS:
        for placement, (n, odd) in dc.TIER_PLACEMENTS.items():
            s, twin, odd_ = dc.tier_scene(kind, placement)
            assert odd_ == odd and s["n"] == twin["n"] == n
            t = dc.tier(s["pos"], s["rot"], s["scale"])
            assert (t[list(odd)] == expect[kind]).all() and (np.delete(t, odd) == 0).all(), (kind, placement)
            assert (dc.tier(twin["pos"], twin["rot"], twin["scale"]) == 0).all()
            assert (dc.census_fallbacks(s) > 0) == (kind != "sep_below") and dc.census_fallbacks(twin) == 0
            lanes = dc.ordinary_lanes(n, odd)
            assert len(lanes) == {"lane0": 63, "lane63": 63, "pair": 63, "partial": 62}[placement]
            a, b = nr.run(s), nr.run(twin)
            for key in ("model", "world_aabb"):
                assert a[key][lanes].tobytes() == b[key][lanes].tobytes(), (kind, placement, key)
            da, db = dc.decide(s), dc.decide(twin)
            for key in ("visible", "lod", "length"):
                assert np.array_equal(da[key][lanes], db[key][lanes])
    assert {o % 64 for _, odd in dc.TIER_PLACEMENTS.values() for o in odd} == {0, 63, 62}
    assert dc.TIER_PLACEMENTS["partial"][0] % 64 != 0


def test_layouts_put_edges_on_the_first_and_last_lanes():
    assert dc.SIZES == (1, 63, 64, 65, 255, 256, 257, 513)
    for name, c in dc.catalogue()["cases"].items():
        e = len(c["scale"])
        assert e <= max(dc.SIZES), name
        covered = set()
        for n in dc.SIZES:
            s, src = dc.layout(name, n)
            assert s["n"] == n == len(src)
            placed = src[src >= 0]
            assert len(placed) == min(n, e) and len(set(placed.tolist())) == len(placed)
            for slot in (0, n - 1, 63, 64, 255, 256):
                if slot < n:
                    assert src[slot] >= 0, (name, n, slot)
            put = src >= 0
            assert s["pos"][put].tobytes() == c["pos"][src[put]].tobytes() and np.array_equal(s["mesh_id"][put], c["mesh_id"][src[put]])
            covered |= set(placed.tolist())
            if n >= e:
                assert set(placed.tolist()) == set(range(e))
        assert covered == set(range(e)), name
    # the fillers are ordinary: the separable tier, finite, and clearly decided by float64 in the axis frame
    s, src = dc.layout("axis", 513)
    fill = src < 0
    assert (dc.tier(s["pos"], s["rot"], s["scale"])[fill] == 0).all()
    assert float64_reference.run(s)["decided"][fill].all()


def test_the_catalogue_is_deterministic():
    a = {k: (v["pos"].tobytes(), v["rot"].tobytes(), v["scale"].tobytes()) for k, v in dc.catalogue()["cases"].items()}
    dc.catalogue.cache_clear()
    b = {k: (v["pos"].tobytes(), v["rot"].tobytes(), v["scale"].tobytes()) for k, v in dc.catalogue()["cases"].items()}
    assert a == b
    assert [c["fallback"] for c in (dc.case("axis"), dc.case("camera"), dc.case("views"), dc.case("subnormal"), dc.case("union"))] == [False] * 5
    assert dc.case("nonfinite")["fallback"] and dc.case("union_nonfinite")["fallback"]
