"""The normal cones of cluster culling on the GPU (include/mi_instance_pipeline.h, mip_build_cluster_cones /
mip_cull_clusters_cone / mip_cull_cluster_triangles_cone): the cone table bit for bit and every byte of the commands, the count,
the stats and the index stream against the numpy restatement (tests/cluster_cone_restatement.py) and the hand-written scenes
(tests/cluster_cone_cases.py); equality with the plain calls where the cone removes nothing; the wave and tile edges of the
cull kernel's skip path, also with reversed and scrambled tiles under the diagnostic library; the decision edges; the three
overflow rules; every new refusal. Every output buffer is filled with a sentinel and compared whole."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_cases as cc
import cluster_cone_cases as ccc
import cluster_cone_restatement as ccr
import cluster_restatement as cr
import lod_restatement as lr
import numpy_restatement as nr
import occlusion_restatement as orr
import test_gpu_batch as T
import test_gpu_batch_lods as TL
import test_gpu_cluster_triangles as TT
import test_gpu_clusters as TC
from renderer_amd import _lib
from renderer_amd.pipeline import make_cluster_cone, make_frame, make_lod_policy, make_occlusion

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SENTINEL = T.SENTINEL
ra = T.ra   # the module's library fixture
NOT_READY, INVALID, CAPACITY = -6, -1, -4
LIGHT = np.array([30.0, 40.0, -20.0], F)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _pipeline(ra, s, vertices, indices, **kw):
    p = TC._pipeline(ra, s, vertices, indices, **kw)
    p.build_cluster_cones()
    return p


def _cull_given(p, s, want, what, eye, facing, cmd_capacity=None, work_capacity=0, async_=False, occ=None):
    """mip_cull_clusters_cone over the scene's own bitmap under the pin policy; the outputs against `want` (cmds, stats)."""
    bm = TC._device_bitmap(s["bitmap"])
    out = TC._Out((len(want["cmds"]) if cmd_capacity is None else cmd_capacity) + 3)
    frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=s["base"])
    p.cull_clusters_cone(frame, bm.data_ptr(), make_lod_policy(lr.DISTANCE, cc.PIN), make_cluster_cone(eye=eye, facing=facing),
                         out.outputs(cmd_capacity, work_capacity, async_), occlusion=occ)
    if async_:
        p.wait()
    TC._check(out, want["cmds"], want["stats"], what)
    return out


# ---- 1. the build ----

def test_built_cones_of_the_hand_written_tables(ra):
    for name, s, cones in ccc.table_cases():
        with _pipeline(ra, s, s["vertices"], s["indices"]) as p:
            got = p.read_cluster_cones()
            assert np.array_equal(_bits(got), _bits(cones)), (name, got)


@pytest.mark.parametrize("ordering", ["rows", "strips", "shuffled", "patches"])
def test_built_cones_equal_the_restatement(ra, ordering):
    s = ra.scene.make_scene(3, n=64)
    vertices, indices = ra.scene.make_geometry(s["meshes"], ordering)
    want = ccr.cluster_cones(s["meshes"], vertices, indices)
    with _pipeline(ra, s, vertices, indices) as p:
        got = p.read_cluster_cones()
    assert got.shape == want.shape == (5771, 8)
    assert np.array_equal(_bits(got), _bits(want)), (ordering, int((_bits(got) != _bits(want)).any(axis=1).sum()))


def test_stale_and_not_ready_rules_and_the_read_capacity(ra):
    name, s, cones = ccc.table_cases()[1]
    with TC._pipeline(ra, s, s["vertices"], s["indices"]) as p:
        lib, ctx = p._lib, p._ctx
        bm = TC._device_bitmap(s["bitmap"])
        out = TC._Out(8)
        frame = make_frame(s["planes"], s["cam_pos"])
        policy, cone = make_lod_policy(lr.DISTANCE, cc.PIN), make_cluster_cone(eye=ccc.EYE, facing=1)

        def not_ready():
            with pytest.raises(ra.MipError) as e:
                p.read_cluster_cones()
            assert e.value.code == NOT_READY
            with pytest.raises(ra.MipError) as e:
                p.cull_clusters_cone(frame, bm.data_ptr(), policy, cone, out.outputs())
            assert e.value.code == NOT_READY and out.untouched()

        not_ready()                                         # a cluster table, no cones yet
        p.build_cluster_cones()
        assert np.array_equal(_bits(p.read_cluster_cones()), _bits(cones))
        host = np.full((len(cones) + 1, 8), 7.0, F)
        assert lib.mip_read_cluster_cones(ctx, host.ctypes.data, len(cones) - 1) == CAPACITY and (host == 7.0).all()
        assert lib.mip_read_cluster_cones(ctx, None, len(cones)) == INVALID
        assert lib.mip_read_cluster_cones(ctx, host.ctypes.data, len(cones)) == 0 and (host[-1] == 7.0).all()
        assert np.array_equal(_bits(host[:-1]), _bits(cones))
        p.build_clusters()                                  # a new cluster table: the cones are stale
        not_ready()
        p.build_cluster_cones()
        p.set_geometry(s["vertices"], s["indices"])         # stale with the table
        with pytest.raises(ra.MipError) as e:
            p.build_cluster_cones()
        assert e.value.code == NOT_READY
        p.build_clusters()
        not_ready()
        p.build_cluster_cones()
        p.set_mesh_table(s["meshes"])
        with pytest.raises(ra.MipError) as e:
            p.build_cluster_cones()
        assert e.value.code == NOT_READY
        p.build_clusters()
        p.build_cluster_cones()
        p.cull_clusters_cone(frame, bm.data_ptr(), policy, cone, out.outputs())
        assert not out.untouched()


# ---- 2. the restatement over config 3; equality with the plain calls ----

def _frame_then_cull(ra, p, s, vertices, indices, boxes, cones, mode, sw, eye, facing, what, wall, base, triangles):
    """mip_run, (the pyramid build,) the cone call over the frame's bitmap with no wait in between; every byte against the
    restatement. Returns (want, the outputs)."""
    import torch

    n = s["n"]
    pv = ra.scene.default_pv()
    f = T._Frame(n)
    frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=base, pv=pv)
    occ = None
    if wall:
        depth = torch.from_numpy(TC._WALL).to(T._dev())
        pyr = torch.full((ra.pipeline.depth_pyramid_layout(64, 32)["bytes"] // 4,), -1.0, dtype=torch.float32, device=T._dev())
        torch.cuda.synchronize()
        occ = make_occlusion(64, 32, pyr.data_ptr(), pv)
    bitmap = orr.bitmap_of(~nr.run(s)["coarse_culled"]) if n else np.zeros(0, np.uint32)
    occlusion = dict(pv=pv, levels=orr.pyramid_levels(TC._WALL), width=64, height=32) if wall else None
    cone = make_cluster_cone(eye=eye, facing=facing)
    if triangles:
        want = ccr.cull_cluster_triangles_cone(s, boxes, cones, eye, facing, vertices, indices, bitmap, mode, sw, pv, max(n, 1) * 8, 1 << 31,
                                               first_instance_base=base, occlusion=occlusion)
        out = TT._Out(max(n, 1) * 8, len(want["stream"]) + 3)
    else:
        want = ccr.cull_clusters_cone(s, boxes, cones, eye, facing, bitmap, mode, sw, max(n, 1) * 8, first_instance_base=base, occlusion=occlusion)
        out = TC._Out(max(n, 1) * 8)
    assert want["status"] == 0, what
    if n:
        p.run_device(frame, async_=True, **f.kwargs())
    if wall:
        p.build_depth_pyramid(depth.data_ptr(), 64, 32, pyr.data_ptr(), format=_lib.MIP_DEPTH_FLOAT32, async_=True)
    if triangles:
        p.cull_cluster_triangles_cone(frame, f.bitmap.data_ptr(), make_lod_policy(mode, sw), cone, out.outputs(async_=True), occlusion=occ)
    else:
        p.cull_clusters_cone(frame, f.bitmap.data_ptr(), make_lod_policy(mode, sw), cone, out.outputs(async_=True), occlusion=occ)
    p.wait()
    assert n == 0 or np.array_equal(f.host_bitmap(), bitmap), (what, "the frame's bitmap")
    if triangles:
        TT._check(out, want, what)
    else:
        TC._check(out, want["cmds"], want["stats"], what)
    return want, out


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 1025])
def test_restatement_over_config_3(ra, n):
    s = TL._sized(ra.scene.make_scene(3, n=max(n, 1)), n)
    vertices, indices = ra.scene.make_geometry(s["meshes"], "patches")
    boxes = cr.cluster_boxes(s["meshes"], vertices, indices)
    cones = ccr.cluster_cones(s["meshes"], vertices, indices, boxes)
    cam = np.asarray(s["cam_pos"], F)
    culled = 0
    with _pipeline(ra, s, vertices, indices) as p:
        # both LOD modes, with and without the wall, both facings, the eye at the camera and at a light; both calls
        for k, (mode, wall, facing, eye) in enumerate([(lr.DISTANCE, False, 1.0, cam), (lr.RELATIVE, True, -1.0, LIGHT),
                                                       (lr.RELATIVE, False, 1.0, LIGHT), (lr.DISTANCE, True, -1.0, cam)]):
            sw = TL._metric_thresholds(s, mode)
            for triangles in ((False, True) if n <= 257 else (k % 2 == 0,)):
                want, _ = _frame_then_cull(ra, p, s, vertices, indices, boxes, cones, mode, sw, eye, facing,
                                           f"n={n} mode={mode} wall={wall} facing={facing} triangles={triangles}", wall, 0xFFFFFFFF - 100, triangles)
                culled += int(want["cone_culled"].sum()) if want["cone_culled"] is not None else 0
        if n == 257:                                       # the known answer (tests/test_cluster_cone_restatement.py), pin policy
            want, _ = _frame_then_cull(ra, p, s, vertices, indices, boxes, cones, lr.DISTANCE, lr.PIN_SWITCH_SQ, cam, 1.0, "pin", False, 0, False)
            assert want["stats"].tolist() == [266, 1971, 3127, 72] and int(want["cone_culled"].sum()) == 731
    assert n < 63 or culled > 0


def test_equality_with_the_plain_calls_where_the_cone_removes_nothing(ra):
    """"shuffled" (12 of 5 771 clusters have a cone, none of them is back-facing here) and an eye that is NaN: the cone calls
    write the plain calls' bytes."""
    s = ra.scene.make_scene(3, n=257)
    vertices, indices = ra.scene.make_geometry(s["meshes"], "shuffled")
    boxes = cr.cluster_boxes(s["meshes"], vertices, indices)
    cones = ccr.cluster_cones(s["meshes"], vertices, indices, boxes)
    pv = ra.scene.default_pv()
    nan_eye = np.array([np.nan, 1.0, 2.0], F)
    with _pipeline(ra, s, vertices, indices) as p:
        for triangles in (False, True):
            want, out = _frame_then_cull(ra, p, s, vertices, indices, boxes, cones, lr.DISTANCE, lr.PIN_SWITCH_SQ, nan_eye, 1.0, "NaN eye", False, 5, triangles)
            assert not want["cone_culled"].any()
            f = T._Frame(257)
            frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=5, pv=pv)
            p.run_device(frame, **f.kwargs())
            policy = make_lod_policy(lr.DISTANCE, lr.PIN_SWITCH_SQ)
            if triangles:
                plain = TT._Out(out.cap, out.room)
                p.cull_cluster_triangles(frame, f.bitmap.data_ptr(), policy, plain.outputs())
            else:
                plain = TC._Out(out.cap)
                p.cull_clusters(frame, f.bitmap.data_ptr(), policy, plain.outputs())
            for a, b in zip(out.result(), plain.result()):
                assert a.tobytes() == b.tobytes(), ("byte for byte", triangles)


def test_the_stream_equals_the_plain_call_s_on_a_property_b_scene(ra):
    """Config 3 under "strips" and the sphere (property (b) holds on both: tests/test_cluster_cone_restatement.py): the cone call's
    index stream and stats[4] are the plain call's, stats[5] — triangles tested — is smaller."""
    pv = ra.scene.default_pv()
    cone = make_cluster_cone(pv)
    scenes = []
    s = ra.scene.make_scene(3, n=257)
    scenes.append(("strips", s, *ra.scene.make_geometry(s["meshes"], "strips"), lr.PIN_SWITCH_SQ))
    sp = ccc.sphere_scene([((0, 1, 12), 1.0), ((3, 2, 9), 0.5)])
    sp["planes"] = s["planes"]
    scenes.append(("sphere", sp, sp["vertices"], sp["indices"], cc.PIN))
    for name, s, vertices, indices, sw in scenes:
        bitmap = orr.bitmap_of(~nr.run(s)["coarse_culled"])
        boxes = cr.cluster_boxes(s["meshes"], vertices, indices)
        cones = ccr.cluster_cones(s["meshes"], vertices, indices, boxes)
        want = ccr.cull_cluster_triangles_cone(s, boxes, cones, np.array(list(cone.eye), F), cone.facing, vertices, indices, bitmap, lr.DISTANCE, sw, pv,
                                               1 << 20, 1 << 31)
        assert want["cone_culled"].any(), name
        with _pipeline(ra, s, vertices, indices) as p:
            bm = TC._device_bitmap(bitmap)
            frame = make_frame(s["planes"], s["cam_pos"], pv=pv)
            policy = make_lod_policy(lr.DISTANCE, sw)
            a, b = TT._Out(len(want["cmds"]), len(want["stream"]) + 64), TT._Out(s["n"] * 8, len(want["stream"]) + 64)
            p.cull_cluster_triangles_cone(frame, bm.data_ptr(), policy, cone, a.outputs())
            p.cull_cluster_triangles(frame, bm.data_ptr(), policy, b.outputs())
            TT._check(a, want, name)
            (_, sa, stream_a), (_, sb, stream_b) = a.result(), b.result()
            assert stream_a.tobytes() == stream_b.tobytes() and sa[6] == sb[6], name
            assert int(sa[7]) < int(sb[7]), (name, int(sa[7]), int(sb[7]))


# ---- 3. hand-written lists ----

@pytest.mark.parametrize("facing", [1.0, -1.0])
def test_two_sided_sheet_ladders(ra, facing):
    for clusters in (1, 2, 3, 63, 64, 65):
        pattern = ("10" * 33)[:clusters]
        s, want = ccc.sheet_scene([pattern, pattern[1:] + "1"], [0, 1, 0], facing=facing, base=11)
        with _pipeline(ra, s, s["vertices"], s["indices"]) as p:
            assert np.array_equal(_bits(p.read_cluster_cones()), _bits(ccc.sheet_cones([pattern, pattern[1:] + "1"])))
            _cull_given(p, s, want, f"C={clusters} facing={facing}", ccc.EYE, facing)


def test_sphere_patches(ra):
    s = ccc.sphere_scene([((0, 0, 0), 1.0)])
    none = dict(cmds=np.zeros(0, cc.DRAW_CMD_DTYPE), stats=[0, 0, 64, 1])
    whole = dict(cmds=np.array([(3 * 4096, 1, 0, 0, 0)], cc.DRAW_CMD_DTYPE), stats=[1, 64, 64, 1])
    boxes = cr.cluster_boxes(s["meshes"], s["vertices"], s["indices"])
    cones = ccr.cluster_cones(s["meshes"], s["vertices"], s["indices"], boxes)
    with _pipeline(ra, s, s["vertices"], s["indices"]) as p:
        assert np.array_equal(_bits(p.read_cluster_cones()), _bits(cones))
        _cull_given(p, s, none, "eye at the centre, facing +1", np.zeros(3, F), 1.0)     # all culled
        _cull_given(p, s, whole, "eye at the centre, facing -1", np.zeros(3, F), -1.0)   # none
        for facing in (1.0, -1.0):
            want = ccr.cull_clusters_cone(s, boxes, cones, np.array([6, 0, 0], F), facing, s["bitmap"], lr.DISTANCE, cc.PIN, 1 << 20)
            assert 8 <= int(want["cone_culled"].sum()) <= 32
            _cull_given(p, s, want, f"eye outside, facing {facing}", np.array([6, 0, 0], F), facing)


# ---- 4. wave and tile edges, by sheet ladders ----

def _filled(w, facing, base):
    """W = w work items of '10' ladders: 8-cluster instances and one shorter one."""
    whole, rest = divmod(w, 8)
    patterns = ["10" * 4] + ([("10" * 4)[:rest]] if rest else [])
    return ccc.sheet_scene(patterns, [0] * whole + ([1] if rest else []), facing=facing, base=base)


def _edge_scenes(part):
    """[(name, scene, want, facing)]. "waves": W one below, at and one above 64 and 1 024 (a survive word, an item tile), a ragged
    last wave; whole waves of culled items between live waves; culled items on lane 0, on lane 63 and across items 63 | 64.
    "grid": one size above the 2 097 152 items from which the cull grid loops, one-cluster instances."""
    out = []
    if part == "grid":
        n = 2048 * 1024 + 1
        inst = (np.arange(n) % 3 == 0).astype(np.int64)              # mesh 1 = DOWN: every third item is culled under facing +1
        out.append(("the grid loops", *ccc.sheet_scene(["1", "0"], inst, facing=1.0, base=3), 1.0))
        return out
    for edge in (64, 1024):
        for w in (edge - 1, edge, edge + 1):
            for facing in (1.0, -1.0):
                out.append((f"W={w} facing={facing}", *_filled(w, facing, base=1), facing))
    out.append(("ragged last wave", *_filled(64 * 3 + 5, 1.0, base=2), 1.0))
    # 64-cluster instances: a live wave, a wave the cone empties, a live wave; then two empty waves at the end; then the same
    # inside one 1 024-item tile border (16 instances per tile: the 17th starts the next tile with an empty wave)
    up, down = "1" * 64, "0" * 64
    for facing in (1.0, -1.0):
        out.append((f"a culled wave between live waves, facing={facing}", *ccc.sheet_scene([up, down], [0, 1, 0, 1, 1], facing=facing, base=4), facing))
        out.append((f"culled waves across a tile border, facing={facing}",
                    *ccc.sheet_scene([up, down], [0] * 15 + [1, 1, 0, 1], facing=facing, base=5), facing))
    # the culled item on lane 0, on lane 63, on both sides of items 63 | 64
    lane0, lane63 = "0" + "1" * 63, "1" * 63 + "0"
    out.append(("culled on lane 0 and lane 63", *ccc.sheet_scene([lane0, lane63], [0, 1, 0], facing=1.0, base=6), 1.0))
    out.append(("culled across 63 | 64", *ccc.sheet_scene([lane63, lane0], [0, 1, 0, 1], facing=1.0, base=7), 1.0))
    return out


def _run_edge_scenes(ra, scenes, with_pyramid=False):
    import torch

    for name, s, want, facing in scenes:
        with _pipeline(ra, s, s["vertices"], s["indices"]) as p:
            _cull_given(p, s, want, name, ccc.EYE, facing, async_=True)
            if with_pyramid:
                # a pyramid that hides nothing (every texel at the far plane under a pv that looks at the sheet from EYE's side):
                # the skip path with the Hi-Z test behind it, the same answer
                pv = ra.scene.default_pv()
                pyr = torch.full((ra.pipeline.depth_pyramid_layout(8, 8)["bytes"] // 4,), 1.0, dtype=torch.float32, device=T._dev())
                torch.cuda.synchronize()
                boxes = cr.cluster_boxes(s["meshes"], s["vertices"], s["indices"])
                cones = ccr.cluster_cones(s["meshes"], s["vertices"], s["indices"], boxes)
                occlusion = dict(pv=pv, levels=orr.pyramid_levels(np.ones((8, 8), F)), width=8, height=8)
                ref = ccr.cull_clusters_cone(s, boxes, cones, ccc.EYE, facing, s["bitmap"], lr.DISTANCE, cc.PIN, 1 << 22, first_instance_base=s["base"],
                                             occlusion=occlusion)
                _cull_given(p, s, ref, name + " under a pyramid", ccc.EYE, facing, occ=make_occlusion(8, 8, pyr.data_ptr(), pv))


EDGE_PARTS = ("waves", "grid")


@pytest.mark.parametrize("part", EDGE_PARTS)
def test_wave_and_tile_edges(ra, part):
    scenes = _edge_scenes(part)
    if part == "waves":
        by_name = {name: want for name, _, want, _ in scenes}
        assert by_name["a culled wave between live waves, facing=1.0"]["stats"].tolist() == [2, 128, 320, 5]
        assert by_name["a culled wave between live waves, facing=-1.0"]["stats"].tolist() == [3, 192, 320, 5]
        assert {int(w["stats"][2]) for w in by_name.values()} >= {63, 64, 65, 1023, 1024, 1025, 197}
    else:
        assert int(scenes[0][2]["stats"][2]) == 2048 * 1024 + 1
    _run_edge_scenes(ra, scenes, with_pyramid=(part == "waves"))


_EDGE_CHILD = r'''
import os, sys
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
os.environ["MIP_LIBRARY"] = os.path.join(root, "renderer_amd", "lib", "libmi_instance_pipeline_dbg.so")
import renderer_amd
import test_gpu_cluster_cones as TK
TK._run_edge_scenes(renderer_amd, TK._edge_scenes(sys.argv[2]))
print("CONE-EDGES-OK")
'''


@pytest.mark.parametrize("part", EDGE_PARTS)
@pytest.mark.parametrize("tiles", ["reverse", "scramble"])
def test_wave_and_tile_edges_in_any_dispatch_order(tiles, part):
    e = dict(os.environ, MIP_DEBUG_TILE_ORDER=tiles)
    out = subprocess.run([sys.executable, "-c", _EDGE_CHILD, ROOT, part], capture_output=True, text=True, timeout=600, env=e)
    assert out.returncode == 0 and "CONE-EDGES-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ---- 5. decision edges ----

def _next(x, up):
    return float(np.nextafter(F(x), F(np.inf if up else -np.inf)))


def test_decision_edges(ra):
    """One mesh of a DOWN and an UP cluster; instances whose columns sit on the guard's limits; eyes on both sides of the float
    where the decision changes, found by bisection on float bits of the restatement's answer. For a cone of the table that float
    is the one of Av Av = Bv: k >= 2^-7 puts it outside Av = 0, whose tie tests/native/cluster_cone_plan_check.cpp holds on the
    same function with a cone of its own."""
    n_w = 24
    w_lo, w_hi = np.sqrt(np.float64(1 - 2.0 ** -20)), np.sqrt(np.float64(1 + 2.0 ** -20))
    ws = [F(1.0)]
    for centre in (w_lo, w_hi):
        x = float(F(centre))
        lo = hi = x
        ws.append(F(x))
        for _ in range(n_w // 4):
            lo, hi = _next(lo, False), _next(hi, True)
            ws += [F(lo), F(hi)]
    scales = [0.0, -0.0, -1.0, 1.0e-42, np.inf, np.nan, 1.0e-20, 0.5, 1.0]
    s, _ = ccc.sheet_scene(["01"], [0] * (len(ws) + len(scales)))
    n = s["n"]
    s["rot"][: len(ws), 3] = ws
    s["scale"][len(ws):] = scales
    boxes = cr.cluster_boxes(s["meshes"], s["vertices"], s["indices"])
    cones = ccr.cluster_cones(s["meshes"], s["vertices"], s["indices"], boxes)

    def answer(eye, facing):
        return ccr.cull_clusters_cone(s, boxes, cones, eye, facing, s["bitmap"], lr.DISTANCE, cc.PIN, 4 * n)

    base = answer(ccc.EYE, 1.0)
    guard_ok = base["cone_culled"].reshape(n, 2)[: len(ws), 0]
    assert guard_ok.any() and not guard_ok.all() and guard_ok[0]                      # both sides of both limits are in the scene
    assert not base["cone_culled"].reshape(n, 2)[len(ws) : len(ws) + 6].any() and base["cone_culled"].reshape(n, 2)[-2:, 0].all()
    # the eye's height at which instance 0's DOWN cluster starts to be culled: bisection on the float's bits
    def culled_at(z):
        return bool(answer(np.array([0.25, 0.25, z], F), 1.0)["cone_culled"][0])

    lo, hi = F(0.5), F(5.0)
    assert not culled_at(lo) and culled_at(hi)
    lo_b, hi_b = int(lo.view(np.uint32)), int(hi.view(np.uint32))
    while hi_b - lo_b > 1:
        mid = (lo_b + hi_b) // 2
        if culled_at(np.array([mid], np.uint32).view(F)[0]):
            hi_b = mid
        else:
            lo_b = mid
    z_out, z_in = (float(np.array([b], np.uint32).view(F)[0]) for b in (lo_b, hi_b))
    eyes = [(ccc.EYE, 1.0), (ccc.EYE, -1.0), ((0.25, 0.25, z_out), 1.0), ((0.25, 0.25, z_in), 1.0), ((0.25, 0.25, -z_in), -1.0),
            ((0.25, 0.25, -z_out), -1.0), ((3.0, -2.0, 0.0), 1.0), ((3.0, -2.0, 0.0), -1.0),           # the eye in the clusters' plane
            ((np.nan, 0.25, 5.0), 1.0), ((0.25, np.inf, 5.0), 1.0), ((0.25, 0.25, -np.inf), -1.0), ((0.25, 0.25, np.inf), 1.0)]
    with _pipeline(ra, s, s["vertices"], s["indices"]) as p:
        for eye, facing in eyes:
            eye = np.array(eye, F)
            want = answer(eye, facing)
            _cull_given(p, s, want, f"eye={eye} facing={facing}", eye, facing)
    assert not answer(np.array([3.0, -2.0, 0.0], F), 1.0)["cone_culled"].any()


def test_non_finite_instances(ra):
    """special_513's instances (tests/golden: special values in every column) over config 3's patches."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "special_513.npz"))
    s = dict(pos=g["pos"], rot=g["rot"], scale=g["scale"], mesh_id=g["mesh_id"], meshes=g["meshes"], planes=g["planes"], cam_pos=g["cam_pos"],
             n=len(g["scale"]))
    vertices, indices = ra.scene.make_geometry(s["meshes"], "patches")
    boxes = cr.cluster_boxes(s["meshes"], vertices, indices)
    cones = ccr.cluster_cones(s["meshes"], vertices, indices, boxes)
    with _pipeline(ra, s, vertices, indices) as p:
        for facing in (1.0, -1.0):
            _frame_then_cull(ra, p, s, vertices, indices, boxes, cones, lr.DISTANCE, lr.PIN_SWITCH_SQ, np.asarray(s["cam_pos"], F), facing,
                             f"special_513 facing={facing}", False, 0, facing > 0)


# ---- 6. one overflow of each kind; every new refusal ----

def test_overflow_rules(ra):
    s = ra.scene.make_scene(3, n=257)
    vertices, indices = ra.scene.make_geometry(s["meshes"], "patches")
    boxes = cr.cluster_boxes(s["meshes"], vertices, indices)
    cones = ccr.cluster_cones(s["meshes"], vertices, indices, boxes)
    pv = ra.scene.default_pv()
    cone = make_cluster_cone(pv)
    eye = np.array(list(cone.eye), F)
    policy = make_lod_policy(lr.DISTANCE, lr.PIN_SWITCH_SQ)
    bitmap = orr.bitmap_of(~nr.run(s)["coarse_culled"])
    full = ccr.cull_clusters_cone(s, boxes, cones, eye, 1.0, bitmap, lr.DISTANCE, lr.PIN_SWITCH_SQ, 1 << 20, first_instance_base=17)
    tri = ccr.cull_cluster_triangles_cone(s, boxes, cones, eye, 1.0, vertices, indices, bitmap, lr.DISTANCE, lr.PIN_SWITCH_SQ, pv, 1 << 20, 1 << 31,
                                          first_instance_base=17)
    heads, w, members = int(full["stats"][0]), int(full["stats"][2]), int(full["stats"][3])
    room = len(tri["stream"])
    with _pipeline(ra, s, vertices, indices) as p:
        bm = TC._device_bitmap(bitmap)
        frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=17, pv=pv)

        def overflows(call):
            with pytest.raises(ra.MipError) as e:
                call()
                p.wait()
            assert e.value.code == CAPACITY
            p.wait()

        for async_ in (False, True):
            out = TC._Out(heads)                # a command overflow: the first commands exactly, the true stats
            overflows(lambda: p.cull_clusters_cone(frame, bm.data_ptr(), policy, cone, out.outputs(cmd_capacity=heads - 1, async_=async_)))
            TC._check(out, full["cmds"], full["stats"], f"cmd_capacity async={async_}", count=heads - 1)
            out = TC._Out(heads)                # a work overflow: the zero count and the refusal's stats
            overflows(lambda: p.cull_clusters_cone(frame, bm.data_ptr(), policy, cone, out.outputs(work_capacity=w - 1, async_=async_)))
            TC._check(out, full["cmds"], [0, 0, w, members], f"work_capacity async={async_}", count=0)
            out = TT._Out(heads, room)          # an index overflow: the true six stats, nothing else
            overflows(lambda: p.cull_cluster_triangles_cone(frame, bm.data_ptr(), policy, cone, out.outputs(index_capacity=room - 3, async_=async_)))
            TT._check(out, tri, f"index_capacity async={async_}", count=0, written=False)
            out = TT._Out(heads, room)          # then a fitting call
            p.cull_cluster_triangles_cone(frame, bm.data_ptr(), policy, cone, out.outputs(async_=async_))
            p.wait()
            TT._check(out, tri, f"fitting async={async_}")


def test_new_refusals_write_nothing(ra):
    s, want = ccc.sheet_scene(["10"], [0, 0], base=3)
    with TC._pipeline(ra, s, s["vertices"], s["indices"]) as p:
        lib, ctx = p._lib, p._ctx
        bm = TC._device_bitmap(s["bitmap"])
        out, tri = TC._Out(4), TT._Out(4, 1024)
        frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=3, pv=ra.scene.default_pv())
        policy = make_lod_policy(lr.DISTANCE, cc.PIN)

        def call(cone, triangles=False, o=None, policy=policy):
            fn = lib.mip_cull_cluster_triangles_cone if triangles else lib.mip_cull_clusters_cone
            o = o if o is not None else (tri.outputs() if triangles else out.outputs())
            return fn(ctx, C.addressof(frame), bm.data_ptr(), C.addressof(policy) if policy is not None else None, None,
                      C.addressof(cone) if cone is not None else None, C.addressof(o))

        def cone(**kw):
            c = make_cluster_cone(eye=ccc.EYE, facing=1)
            for k, v in kw.items():
                setattr(c, k, v)
            return c

        assert call(cone()) == NOT_READY and call(cone(), True) == NOT_READY        # no cone table yet
        p.build_cluster_cones()
        for triangles in (False, True):
            refused = [("NULL cone", call(None, triangles)), ("struct_size", call(cone(struct_size=20), triangles)), ("flags", call(cone(flags=1), triangles)),
                       ("facing 0", call(cone(facing=0.0), triangles)), ("facing 2", call(cone(facing=2.0), triangles)),
                       ("facing NaN", call(cone(facing=float("nan")), triangles)), ("facing -0.5", call(cone(facing=-0.5), triangles)),
                       ("NULL policy", call(cone(), triangles, policy=None))]       # and what the plain calls refuse
            for what, rc in refused:
                assert rc == INVALID, (what, triangles, rc)
        bad = out.outputs()
        bad.struct_size = 36
        assert call(cone(), o=bad) == INVALID
        bad = tri.outputs()
        bad.culled_indices = None
        assert call(cone(), True, o=bad) == INVALID
        assert lib.mip_cull_clusters_cone(None, C.addressof(frame), bm.data_ptr(), C.addressof(policy), None, C.addressof(cone()), C.addressof(out.outputs())) == INVALID
        assert out.untouched() and tri.untouched()
        _cull_given(p, s, want, "after the refusals", ccc.EYE, 1.0)     # the context is usable
