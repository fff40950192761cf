"""The decision-edge catalogue of the per-triangle test (tests/triangle_edge_cases.py) on the CPU: every case is realised bit
for bit, its hand-stated answer is the restatement's and the oracle's, the kernel's division-free predicate agrees, every
mutant is killed under every pv, and the scenes the GPU tests run satisfy their own preconditions."""
from fractions import Fraction

import numpy as np
import pytest

import cluster_cone_restatement as ccr
import cluster_restatement as cr
import cluster_triangle_restatement as ctr
import cluster_cases as cc
import lod_restatement as lr
import numpy_restatement as nr
import renderer_amd
import triangle_edge_cases as te

F = np.float32
GROUP_NAMES = list(te.GROUPS)
PV_NAMES = list(te.PVS)


def _model(group):
    pos, rot, scale = te.instance_arrays(group, 1)
    return nr.model_matrices(pos, rot, scale)[0]


def _realised_clip(group, cs):
    v = np.array([te.realise(group, c.clip[k]) for c in cs for k in range(3)], F).reshape(-1, 3, 3)
    return v, te.clip_of(_model(group), te.PVS[te.PV_OF[group]], v)


def test_the_identity_instance_has_the_identity_matrix_and_the_pvs_have_no_other_entries():
    assert te.bits(_model("pos")).tolist() == te.bits(np.eye(4, dtype=F).reshape(16)).tolist()
    for pv in te.PVS.values():
        assert set(np.abs(pv).tolist()) <= {0.0, 1.0, 4.0}
        assert all(np.signbit(v) for v in pv if v == 0)            # every zero is -0
    assert te.up(te.WSTAR) * (F(1) / te.WSTAR) == F(1) and te.up(te.WSTAR) / te.WSTAR > F(1)


@pytest.mark.parametrize("group", GROUP_NAMES)
def test_every_case_is_realised_bit_for_bit(group):
    cs = te.cases(group) + [te.FILLER_FRONT, te.FILLER_BACK]
    _, clip = _realised_clip(group, cs)
    for c, got in zip(cs, clip):
        for k in range(3):
            want = c.clip[k]
            if np.isnan(want).any():
                assert np.isnan(want).all() and np.isnan(got[k, [0, 1, 3]]).all(), (c.name, k, got[k])
                continue
            assert te.bits(got[k, 3]) == te.bits(want[2]), (c.name, k, "w", got[k], want)
            for a in (0, 1):                                         # x, y: the bits, but for the sign of a zero (module docstring)
                assert te.bits(got[k, a]) == te.bits(want[a]) or (got[k, a] == 0 and want[a] == 0), (c.name, k, "xy"[a], got[k], want)


@pytest.mark.parametrize("group", GROUP_NAMES)
def test_hand_answers_against_the_restatement_and_the_division_free_predicate(group):
    cs = te.cases(group) + [te.FILLER_FRONT, te.FILLER_BACK]
    v, clip = _realised_clip(group, cs)
    hand = np.array([c.kept for c in cs])
    got = ~nr.triangle_culled(_model(group), te.PVS[te.PV_OF[group]], v)
    assert [c.name for c, a, b in zip(cs, hand, got) if a != b] == []
    assert np.array_equal(~te.culled(clip), hand)                   # the switched restatement without a switch
    ndc = np.array([c.cls == "ndc" for c in cs])
    with np.errstate(all="ignore"):
        true_outside = ((clip[..., 0] / clip[..., 3] < -1).all(axis=1) | (clip[..., 0] / clip[..., 3] > 1).all(axis=1)
                        | (clip[..., 1] / clip[..., 3] < -1).all(axis=1) | (clip[..., 1] / clip[..., 3] > 1).all(axis=1))
    assert np.array_equal(te.kernel_ndc_outside(clip), true_outside)       # on every case, whatever its class
    # an NDC case is decided by the bounds alone: its determinant is not > 0 (the families' paper argument)
    assert np.array_equal(~te.kernel_ndc_outside(clip)[ndc], hand[ndc])


def _exact_det(c):
    x, y, w = ([Fraction(float(c.clip[k, a])) for k in range(3)] for a in range(3))
    return x[0] * (y[1] * w[2] - y[2] * w[1]) - x[1] * (y[0] * w[2] - y[2] * w[0]) + x[2] * (y[0] * w[1] - y[1] * w[0])


def test_exact_determinants_of_the_ndc_families():
    """In exact arithmetic: all-on and all-beyond triangles have det == 0 (proportional columns), the two kept families that
    have an area have det < 0 — so they are kept because no bound has all three corners, not by an accident of rounding."""
    seen = 0
    for group in ("pos", "neg", "overflow"):
        for c in te.cases(group):
            if c.cls != "ndc" or not np.isfinite(c.clip).all() or not c.name.startswith("ndc_"):
                continue
            d = _exact_det(c)
            if c.name.endswith("all_on") or c.name.endswith("all_beyond"):
                assert d == 0, c.name
            else:
                assert d < 0, c.name
            seen += 1
    assert seen > 300


@pytest.mark.parametrize("group", GROUP_NAMES)
def test_the_oracle_agrees_with_the_hand_answers(oracle_mod, group):
    for n, nan_vertex in ((1, False), (2, True)):
        sc = te.scene(renderer_amd, group, n, nan_vertex=nan_vertex)
        s = sc["s"]
        r = oracle_mod.run(s["pos"], s["rot"], s["scale"], s["mesh_id"], s["meshes"], s["planes"], s["cam_pos"])
        assert r["draw_count"] == n
        capacity = r["draw_index_total"] + 7
        cmds, out, _ = oracle_mod.cull_all_triangles(r, s["pos"], s["mesh_id"], s["meshes"], s["cam_pos"], sc["pv"], sc["vertices"], sc["indices"],
                                                     out_capacity=capacity)
        counts, want = te.expected_stream(sc, capacity)
        assert cmds["indexCount"].tolist() == counts.tolist()
        assert np.array_equal(out, want), [c.name for c, a in zip(sc["layouts"][0], range(10**6))
                                           if (out[3 * a : 3 * a + 3] != want[3 * a : 3 * a + 3]).any()][:10]
        src = nr.src_index_offsets(s["pos"], s["mesh_id"], r["coarse_culled"], s["meshes"], s["cam_pos"])
        cmds2, out2 = nr.cull_all_triangles(r["draw_cmds"], src, r["model"], 0, sc["pv"], sc["vertices"], sc["indices"], capacity)
        assert cmds2.tobytes() == cmds.tobytes() and np.array_equal(out2, out)


@pytest.mark.parametrize("pv_name", PV_NAMES)
@pytest.mark.parametrize("mutant", te.MUTANTS)
def test_every_mutant_is_killed_under_every_pv(pv_name, mutant):
    killed = []
    for group in GROUP_NAMES:
        if te.PV_OF[group] != pv_name:
            continue
        cs = te.cases(group)
        _, clip = _realised_clip(group, cs)
        got = ~te.mutants[mutant](clip)
        killed += [c.name for c, k in zip(cs, got) if k != c.kept]
    assert killed, (pv_name, mutant)


@pytest.mark.parametrize("pv_name", PV_NAMES)
def test_the_sign_taken_by_comparison_is_caught_on_either_axis(pv_name):
    for axis_cases in (lambda c: c.name.startswith("zero_w_sign_bit") and not c.name.endswith("_on_y"), lambda c: c.name.endswith("decides_kept_on_y")
                       or c.name.endswith("decides_culled_on_y")):
        cs = [c for c in te.cases(pv_name) if axis_cases(c)]
        _, clip = _realised_clip(pv_name, cs)
        assert len(cs) == 2 and (~te.mutants["sign_by_compare"](clip) != np.array([c.kept for c in cs])).all()


def test_every_mesh_is_finite_and_the_nan_corners_come_from_overflow():
    for group in GROUP_NAMES:
        v, _, tris = te.mesh(group, 0)
        assert np.isfinite(v).all(), group
    assert sum(np.isnan(c.clip).any() for c in te.cases("scaled")) == 4


@pytest.mark.parametrize("group", GROUP_NAMES)
def test_mesh_layout(group):
    cs = te.cases(group)
    for rotate in (0, 63):
        v, ix, tris = te.mesh(group, rotate)
        t = len(tris)
        assert t % 64 == 0 and t >= 256 and len(v) == 3 * t and ix.tolist() == list(range(3 * t))
        where = {id(c): k for k, c in enumerate(tris) if c.cls != "filler"}
        assert len(where) == len(cs) and all(id(c) in where for c in cs)          # every case is in the mesh, once
        lanes = {k % 64 for k in where.values()}
        assert {0, 63} <= lanes
        assert any(k < 256 for k in where.values()) and any(k >= 256 for k in where.values())   # both sides of a 256-slot range cut
        kinds = {c.name for c in tris if c.cls == "filler"}
        assert kinds == {"filler_front", "filler_back"}
    a, b = te.layout(group, 0), te.layout(group, 63)
    assert a[0].cls != "filler" and all(b[(k + 63) % len(a)] is a[k] for k in range(len(a)))


@pytest.mark.parametrize("group", GROUP_NAMES)
def test_scene_preconditions(group):
    """Every instance is visible; the cluster restatement tests every triangle of every cluster (every cluster survives, with
    and without cones — none of these meshes has a cone); so no case of any scene is left untested."""
    for (n, first_mesh), nan_vertex in zip(te.SCENES, (False, True, False, True)):
        sc = te.scene(renderer_amd, group, n, nan_vertex=nan_vertex, first_mesh=first_mesh)
        s = sc["s"]
        # finite geometry lets model_is_affine choose triangle_test<true>; one NaN vertex anywhere sends every command down the literal chain
        assert bool(np.isfinite(sc["vertices"]).all()) == (not nan_vertex)
        assert np.isfinite(nr.model_matrices(s["pos"], s["rot"], s["scale"])).all()
        frame = nr.run(s)
        assert not frame["coarse_culled"].any() and len(frame["cmds"]["indexCount"]) == n
        t = len(sc["layouts"][0])
        assert frame["cmds"]["indexCount"].tolist() == [3 * t] * n
        boxes = cr.cluster_boxes(s["meshes"], sc["vertices"], sc["indices"])
        want = ctr.cull_cluster_triangles(s, boxes, sc["vertices"], sc["indices"], s["bitmap"], lr.DISTANCE, cc.PIN, sc["pv"], 1 << 20, 1 << 30)
        assert want["status"] == 0 and want["survive"].all()
        assert int(want["stats"][5]) == n * t                        # triangles tested: all of them — the untested share is zero
        counts, stream = te.expected_stream(sc)
        assert np.array_equal(want["stream"], stream) and int(want["stats"][4]) == len(stream) // 3
        if n == 2:
            cones = ccr.cluster_cones(s["meshes"], sc["vertices"], sc["indices"], boxes)
            assert np.array_equal(te.bits(cones), te.bits(np.tile(ccr.NO_CONE, (len(cones), 1))))
            cone = ccr.cull_cluster_triangles_cone(s, boxes, cones, np.zeros(3, F), 1.0, sc["vertices"], sc["indices"], s["bitmap"], lr.DISTANCE, cc.PIN,
                                                   sc["pv"], 1 << 20, 1 << 30)
            assert np.array_equal(cone["stream"], stream) and cone["stats"].tolist() == want["stats"].tolist()
