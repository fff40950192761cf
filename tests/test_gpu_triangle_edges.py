"""The decision-edge catalogue of the per-triangle test (tests/triangle_edge_cases.py) through every kernel that inlines it:
every decomposition of mip_run's per-triangle stage with finite geometry (every vertex of the catalogue's meshes is finite, NaN
corners come from overflow under the scaled instance: the affine instantiation runs), the same with one NaN vertex appended (the
literal instantiation) at each distinct call site, and mip_cull_cluster_triangles with and without cones. Every comparison is
on bytes; every buffer is filled with a sentinel and compared whole; the expected stream is built twice — by the oracle (or the restatement) and from the hand-stated flags alone.
tests/test_triangle_edge_cases.py checks on the CPU that every case of every scene reaches the triangle test."""
import numpy as np
import pytest

import cluster_cases as cc
import cluster_cone_restatement as ccr
import cluster_restatement as cr
import cluster_triangle_restatement as ctr
import lod_restatement as lr
import test_gpu_batch as T
import test_gpu_cluster_triangles as TT
import test_gpu_clusters as TC
import triangle_edge_cases as te
from renderer_amd.pipeline import make_cluster_cone, make_frame, make_lod_policy
from test_gpu_triangles import SENTINEL, _assert_frame, _Stage
from triangle_variants import MODES, force_variant

pytestmark = pytest.mark.gpu
ra = T.ra   # the module's library fixture
GROUP_NAMES = list(te.GROUPS)
GUARD = 64


def _want(ra, oracle_mod, group, n, first_mesh, nan_vertex=False):
    """The scene, the oracle's frame of it and the hand flags' (a few hundred triangles: rebuilt by every test that needs it)."""
    sc = te.scene(ra, group, n, nan_vertex=nan_vertex, first_mesh=first_mesh)
    s = sc["s"]
    # mip_set_geometry derives geometry_finite from EVERY uploaded position: finite here means the affine chain runs
    assert bool(np.isfinite(sc["vertices"]).all()) == (not nan_vertex)
    r = oracle_mod.run(s["pos"], s["rot"], s["scale"], s["mesh_id"], s["meshes"], s["planes"], s["cam_pos"], want=("model", "coarse_culled", "draw_cmds"))
    capacity = r["draw_index_total"] + 3
    cmds, out, _ = oracle_mod.cull_all_triangles(r, s["pos"], s["mesh_id"], s["meshes"], s["cam_pos"], sc["pv"], sc["vertices"], sc["indices"],
                                                 out_capacity=capacity)
    counts, hand = te.expected_stream(sc, capacity)
    assert r["draw_count"] == n and r["draw_index_total"] == 3 * n * len(sc["layouts"][0])
    assert np.array_equal(out, hand) and cmds["indexCount"].tolist() == counts.tolist()   # (the CPU suite's check, not taken on trust)
    return dict(sc=sc, capacity=capacity, cmds=cmds, out=out, hand=hand, total=r["draw_index_total"])


def _run_scenes(ra, oracle_mod, group, nan_vertex, what):
    """One context: the group's geometry, every scene of te.SCENES in turn (set_instances), two frames each. Returns the frames
    [(status, commands, count, total, whole buffer)] of the second frame of every scene."""
    big = _want(ra, oracle_mod, group, *te.SCENES[-1], nan_vertex)
    frames = []
    with _Stage(ra, big["sc"]["s"], big["sc"]["vertices"], big["sc"]["indices"], big["capacity"] + GUARD) as st:
        for n, first_mesh in te.SCENES:
            w = _want(ra, oracle_mod, group, n, first_mesh, nan_vertex)
            s = w["sc"]["s"]
            assert np.array_equal(w["sc"]["vertices"], big["sc"]["vertices"], equal_nan=True)
            st.p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
            frame = make_frame(s["planes"], s["cam_pos"], pv=w["sc"]["pv"])
            for rep in range(2):
                got = st.run(frame, w["capacity"])
                _assert_frame(got, w["cmds"], w["total"], w["out"], (what, n, first_mesh, rep, "oracle"))
                _assert_frame(got, w["cmds"], w["total"], w["hand"], (what, n, first_mesh, rep, "hand flags"))
            frames.append(got)
    return frames


@pytest.mark.parametrize("group", GROUP_NAMES)
@pytest.mark.parametrize("mode", MODES)
def test_catalogue_through_every_variant_of_the_stage(ra, oracle_mod, monkeypatch, mode, group):
    """Every decomposition x every group (a pv and an instance transform), both rotations of the mesh (as the two meshes of the
    table), 1, 1, 2 and 65 instances: commands, count, total and the whole sentinel-filled buffer against the oracle, and the
    stream against the hand-stated flags. The geometry is finite and every model matrix ends in (0, 0, 0, 1): triangle_test<true>."""
    force_variant(monkeypatch, mode)
    _run_scenes(ra, oracle_mod, group, False, (mode, group))


@pytest.mark.parametrize("group", GROUP_NAMES)
@pytest.mark.parametrize("mode", ["ranges", "block256", "parts", "sorted_waves", "recompact_three_launches"])
def test_literal_chain_writes_the_affine_chain_s_bytes(ra, oracle_mod, monkeypatch, mode, group):
    """One NaN vertex that no index names makes the geometry non-finite: every command takes triangle_test<false>. The
    outputs are the bytes of the finite-geometry run (and the oracle's, and the hand flags') — one mode per distinct call site."""
    force_variant(monkeypatch, mode)
    finite = _run_scenes(ra, oracle_mod, group, False, (mode, group, "affine"))
    literal = _run_scenes(ra, oracle_mod, group, True, (mode, group, "literal"))
    for a, b in zip(finite, literal):
        assert a[0] == b[0] == 0 and a[2:4] == b[2:4]
        assert a[1].tobytes() == b[1].tobytes() and a[4].tobytes() == b[4].tobytes()


@pytest.mark.parametrize("nan_vertex", [False, True])
@pytest.mark.parametrize("group", GROUP_NAMES)
def test_catalogue_through_the_cluster_triangle_calls(ra, group, nan_vertex):
    """mip_cull_cluster_triangles (also with the NaN vertex appended) and mip_cull_cluster_triangles_cone on the same meshes:
    whole buffers against the restatements; for the plain call the triangles tested are ALL triangles and the stream is the
    hand flags'."""
    for n, first_mesh in te.SCENES:
        sc = te.scene(ra, group, n, nan_vertex=nan_vertex, first_mesh=first_mesh)
        s, pv = sc["s"], sc["pv"]
        boxes = cr.cluster_boxes(s["meshes"], sc["vertices"], sc["indices"])
        want = ctr.cull_cluster_triangles(s, boxes, sc["vertices"], sc["indices"], s["bitmap"], lr.DISTANCE, cc.PIN, pv, 1 << 20, 1 << 30)
        counts, hand = te.expected_stream(sc)
        t = len(sc["layouts"][0])
        assert want["status"] == 0 and int(want["stats"][5]) == n * t and np.array_equal(want["stream"], hand)
        policy = make_lod_policy(lr.DISTANCE, cc.PIN)
        frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=0, pv=pv)
        with TC._pipeline(ra, s, sc["vertices"], sc["indices"]) as p:
            out = TT._cull_given(p, s, want, (group, n, "plain"), pv)
            stats, stream = out.result()[1][2:8], out.result()[2]
            assert int(stats[5]) == n * t and int(stats[4]) == len(hand) // 3
            assert np.array_equal(stream[: len(hand)], hand)
            if not nan_vertex:
                p.build_cluster_cones()
                cones = ccr.cluster_cones(s["meshes"], sc["vertices"], sc["indices"], boxes)
                assert np.array_equal(te.bits(p.read_cluster_cones()), te.bits(cones))
                eye = np.zeros(3, np.float32)
                cone_want = ccr.cull_cluster_triangles_cone(s, boxes, cones, eye, 1.0, sc["vertices"], sc["indices"], s["bitmap"], lr.DISTANCE, cc.PIN, pv,
                                                            1 << 20, 1 << 30)
                bm = TC._device_bitmap(s["bitmap"])
                cone_out = TT._Out(len(cone_want["cmds"]), len(cone_want["stream"]))
                p.cull_cluster_triangles_cone(frame, bm.data_ptr(), policy, make_cluster_cone(eye=eye, facing=1.0), cone_out.outputs())
                TT._check(cone_out, cone_want, (group, n, "cone"))
