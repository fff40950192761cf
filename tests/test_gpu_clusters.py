"""Cluster culling on the GPU (include/mi_instance_pipeline.h, mip_build_clusters / mip_cull_clusters): the built boxes and every
byte of the commands, the count and the stats against the numpy restatement (tests/cluster_restatement.py) and against the
hand-written scenes (tests/cluster_cases.py); the structural edges of the launch plan (renderer_amd/csrc/cluster_plan.hpp),
also with reversed and scrambled tiles under the diagnostic library; both overflow rules; every refusal. Every output buffer is
filled with a sentinel and compared whole. Not reference behaviour: parity is with the restatement."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_cases as cc
import cluster_restatement as cr
import lod_restatement as lr
import occlusion_restatement as orr
import test_gpu_batch as T
import test_gpu_batch_lods as TL
from renderer_amd import _lib
from renderer_amd.pipeline import MESH_DTYPE, make_cluster_outputs, make_frame, make_lod_policy, make_occlusion

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = T.SENTINEL
ra = T.ra   # the module's library fixture
NOT_READY, INVALID, CAPACITY = -6, -1, -4


class _Out:
    """Device outputs of mip_cull_clusters, filled with a sentinel: room for `cap` commands + 3 entries nobody may touch;
    scal[0] = cmd_count, scal[2:6] = stats."""

    def __init__(self, cap, stats=True):
        import torch

        fill = T._i32(SENTINEL)
        self.cap, self.stats = int(cap), stats
        self.cmds = torch.full((self.cap + 3, 5), fill, dtype=torch.int32, device=T._dev())
        self.scal = torch.full((8,), fill, dtype=torch.int32, device=T._dev())
        torch.cuda.synchronize()

    def outputs(self, cmd_capacity=None, work_capacity=0, async_=False):
        return make_cluster_outputs(self.cmds.data_ptr(), self.cap if cmd_capacity is None else cmd_capacity, self.scal.data_ptr(),
                                    self.scal.data_ptr() + 8 if self.stats else 0, work_capacity=work_capacity, async_=async_)

    def result(self):
        import torch

        torch.cuda.synchronize()
        return self.cmds.cpu().numpy().view(np.uint32), self.scal.cpu().numpy().view(np.uint32)

    def untouched(self):
        cmds, scal = self.result()
        return (cmds == SENTINEL).all() and (scal == SENTINEL).all()


def _check(out, want_cmds, want_stats, what, count=None):
    """The first `count` entries are want_cmds' (all of them unless a capacity cut the list), nothing else was written."""
    cmds, scal = out.result()
    count = len(want_cmds) if count is None else count
    assert int(scal[0]) == count, (what, "cmd_count", int(scal[0]), count)
    assert cmds[:count].tobytes() == np.ascontiguousarray(want_cmds[:count]).tobytes(), (what, "commands")
    assert (cmds[count:] == SENTINEL).all(), (what, "entries at or behind cmd_count were written")
    if out.stats:
        assert scal[2:6].tolist() == [int(v) for v in want_stats], (what, "stats", scal[2:6].tolist(), list(want_stats))
    else:
        assert (scal[2:6] == SENTINEL).all(), what
    assert scal[1] == SENTINEL and (scal[6:] == SENTINEL).all(), what


def _pipeline(ra, s, vertices, indices, **kw):
    p = T._pipeline(ra, s, **kw)
    p.set_geometry(vertices, indices)
    p.build_clusters()
    return p


def _device_bitmap(bitmap):
    import torch

    words = np.ascontiguousarray(bitmap if len(bitmap) else np.zeros(1, np.uint32)).view(np.int32)
    t = torch.from_numpy(words.copy()).to(T._dev())
    torch.cuda.synchronize()
    return t


def _cull_given(p, s, want, what, cmd_capacity=None, work_capacity=0, async_=False, extra=3):
    """mip_cull_clusters over the scene's own bitmap (uploaded) under the pin policy; the outputs against `want`."""
    bm = _device_bitmap(s["bitmap"])
    out = _Out((len(want["cmds"]) if cmd_capacity is None else cmd_capacity) + extra)
    frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=s["base"])
    p.cull_clusters(frame, bm.data_ptr(), make_lod_policy(lr.DISTANCE, cc.PIN), out.outputs(cmd_capacity, work_capacity, async_))
    if async_:
        p.wait()
    _check(out, want["cmds"], want["stats"], what)
    return out


# ---- 1. the build ----

@pytest.mark.parametrize("ordering", ["rows", "strips", "shuffled"])
def test_built_boxes_equal_the_restatement(ra, ordering):
    s = ra.scene.make_scene(3, n=1)
    vertices, indices = ra.scene.make_geometry(s["meshes"], ordering)
    want = cr.cluster_boxes(s["meshes"], vertices, indices)
    with _pipeline(ra, s, vertices, indices) as p:
        assert p.cluster_count() == len(want) > 1000
        got = p.read_cluster_boxes()
    assert got.shape == want.shape and np.array_equal(got, want)   # as numbers: the sign of a zero is not specified


def _edge_table():
    """One mesh, six levels of C = 65, 64, 63, 1 (short), and of two and one indices (no triangle, no cluster)."""
    m = np.zeros(1, MESH_DTYPE)
    m["aabb_min"], m["aabb_max"], m["n_lods"] = (-1, -1, -1), (1, 1, 1), 6
    off = 0
    for l, length in enumerate((192 * 65, 192 * 64, 192 * 63 - 3 * 5, 3 * 59 + 1, 2, 1)):
        m["index_len"][0, l], m["index_offset"][0, l] = length, off
        off += length
    rng = np.random.default_rng(5)
    vertices = rng.uniform(-1, 1, (997, 3)).astype(np.float32)
    vertices[::17, 1] = np.nan                                   # a NaN coordinate is ignored, on its axis alone
    return m, vertices, rng.integers(0, 997, off).astype(np.uint32)


def test_built_boxes_at_the_cluster_count_edges(ra):
    m, vertices, indices = _edge_table()
    s = ra.scene.make_scene(1, n=1)
    s["meshes"] = m
    want = cr.cluster_boxes(m, vertices, indices)
    assert cr.cluster_table(m)["C"].tolist() == [65, 64, 63, 1, 0, 0]
    with _pipeline(ra, s, vertices, indices) as p:
        assert p.cluster_count() == 65 + 64 + 63 + 1
        got = p.read_cluster_boxes()
    assert np.array_equal(got, want) and np.isfinite(got).all()


def test_build_refusals_and_the_stale_table(ra):
    s = ra.scene.make_scene(3, n=64)
    vertices, indices = ra.scene.make_geometry(s["meshes"])
    out = _Out(512)
    frame = make_frame(s["planes"], s["cam_pos"])
    policy = make_lod_policy(lr.DISTANCE, lr.PIN_SWITCH_SQ)
    bm = _device_bitmap(np.full(2, 0xFFFFFFFF, np.uint32))
    with T._pipeline(ra, s) as p:
        with pytest.raises(ra.MipError) as e:                    # no geometry
            p.build_clusters()
        assert e.value.code == NOT_READY and p.cluster_count() == 0
        with pytest.raises(ra.MipError) as e:                    # no table yet
            p.cull_clusters(frame, bm.data_ptr(), policy, out.outputs())
        assert e.value.code == NOT_READY
        p.set_geometry(vertices, indices)
        p.build_clusters()
        count = p.cluster_count()
        p.cull_clusters(frame, bm.data_ptr(), policy, out.outputs())
        # a LOD-3 range outside the indices: refused, and the table the mesh-table upload made stale stays stale
        k = int(np.nonzero(s["meshes"]["n_lods"] >= 4)[0][0])
        bad = s["meshes"].copy()
        bad["index_offset"][k, 3] = len(indices) - 1
        p.set_mesh_table(bad)
        assert p.cluster_count() == 0
        with pytest.raises(ra.MipError) as e:
            p.build_clusters()
        assert e.value.code == INVALID and "LOD 3" in str(e.value) and p.cluster_count() == 0
        # a vertex outside the uploaded vertices
        p.set_mesh_table(s["meshes"])
        p.set_geometry(vertices[: len(vertices) // 2], indices)
        with pytest.raises(ra.MipError) as e:
            p.build_clusters()
        assert e.value.code == INVALID
        # the stale table after set_geometry: not ready until it is built again, and nothing is written
        p.set_geometry(vertices, indices)
        fresh = _Out(512)
        with pytest.raises(ra.MipError) as e:
            p.cull_clusters(frame, bm.data_ptr(), policy, fresh.outputs())
        assert e.value.code == NOT_READY and fresh.untouched() and p.cluster_count() == 0
        with pytest.raises(ra.MipError) as e:
            p.read_cluster_boxes()
        p.build_clusters()
        assert p.cluster_count() == count
        p.cull_clusters(frame, bm.data_ptr(), policy, fresh.outputs())
        a, b = out.result(), fresh.result()
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and int(a[1][0]) > 0


# ---- 2. the restatement over the repository's scenes ----

_WALL = np.ones((32, 64), np.float32)
_WALL[:, :32] = 0.0   # a wall at the near plane over the left half of a 64 x 32 image


def _frame_then_cull(ra, p, s, boxes, mode, sw, what, full_bitmap, wall, base):
    """mip_run, (the pyramid build,) mip_cull_clusters over the frame's bitmap with no wait in between — or over a full bitmap
    uploaded first; every byte against the restatement. Returns the restatement's answer."""
    import torch

    n = s["n"]
    f = T._Frame(n)
    frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=base)
    given = _device_bitmap(np.full((n + 31) // 32, 0xFFFFFFFF, np.uint32)) if full_bitmap else None
    occ = None
    if wall:
        depth = torch.from_numpy(_WALL).to(T._dev())
        pyr = torch.full((ra.pipeline.depth_pyramid_layout(64, 32)["bytes"] // 4,), -1.0, dtype=torch.float32, device=T._dev())
        torch.cuda.synchronize()
        occ = make_occlusion(64, 32, pyr.data_ptr(), ra.scene.default_pv())
    cap = max(n, 1) * 8
    out = _Out(cap)
    if n:
        p.run_device(frame, async_=True, **f.kwargs())
    if wall:
        p.build_depth_pyramid(depth.data_ptr(), 64, 32, pyr.data_ptr(), format=_lib.MIP_DEPTH_FLOAT32, async_=True)
    p.cull_clusters(frame, (given if given is not None else f.bitmap).data_ptr(), make_lod_policy(mode, sw), out.outputs(async_=True), occlusion=occ)
    p.wait()
    bitmap = np.full((n + 31) // 32, 0xFFFFFFFF, np.uint32) if full_bitmap else f.host_bitmap()
    occlusion = dict(pv=ra.scene.default_pv(), levels=orr.pyramid_levels(_WALL), width=64, height=32) if wall else None
    want = cr.cull_clusters(s, boxes, bitmap, mode, sw, cmd_capacity=cap, first_instance_base=base, occlusion=occlusion)
    assert want["status"] == 0, what
    _check(out, want["cmds"], want["stats"], what)
    return want


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 1025, 4097])
def test_restatement_over_config_3(ra, n):
    ordering = "strips" if n == 257 else "rows" if n % 2 else "shuffled"
    s = TL._sized(ra.scene.make_scene(3, n=max(n, 1)), n)
    vertices, indices = ra.scene.make_geometry(s["meshes"], ordering)
    boxes = cr.cluster_boxes(s["meshes"], vertices, indices)
    walled = free = None
    with _pipeline(ra, s, vertices, indices) as p:
        for mode in (lr.DISTANCE, lr.RELATIVE):
            sw = TL._metric_thresholds(s, mode)
            for full_bitmap in (False, True):
                for wall in (False, True):
                    base = (0xFFFFFFFF - n // 2) if full_bitmap else 3      # a base that wraps inside the scene
                    want = _frame_then_cull(ra, p, s, boxes, mode, sw, f"n={n} {ordering} mode={mode} full={full_bitmap} wall={wall}",
                                            full_bitmap, wall, base)
                    if full_bitmap and mode == lr.DISTANCE:
                        walled, free = (want, free) if wall else (walled, want)
        if n == 257:
            # the scene exercises the feature (CPU-checked in tests/test_cluster_restatement.py): the pin policy, the frame's bitmap
            want = _frame_then_cull(ra, p, s, boxes, lr.DISTANCE, lr.PIN_SWITCH_SQ, "n=257 strips pin", False, False, 0)
            heads, survivors, w, members = (int(v) for v in want["stats"])
            assert survivors < w and heads != members
            assert members - len(np.unique(want["items"]["inst"][want["survive"]])) >= 1
    if n >= 257:   # the wall removes clusters, and only removes
        assert 0 < int(walled["stats"][1]) < int(free["stats"][1])


def test_non_finite_instances_take_the_literal_chain(ra):
    """special_513's instances (tests/golden: special values in every column) over config 3's geometry: SURVIVES follows the
    literal chain for every one of them."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "special_513.npz"))
    s = dict(pos=g["pos"], rot=g["rot"], scale=g["scale"], mesh_id=g["mesh_id"], meshes=g["meshes"], planes=g["planes"], cam_pos=g["cam_pos"],
             n=len(g["scale"]))
    assert not np.isfinite(s["pos"]).all()
    vertices, indices = ra.scene.make_geometry(s["meshes"], "strips")
    boxes = cr.cluster_boxes(s["meshes"], vertices, indices)
    with _pipeline(ra, s, vertices, indices) as p:
        for wall in (False, True):
            want = _frame_then_cull(ra, p, s, boxes, lr.DISTANCE, lr.PIN_SWITCH_SQ, f"special_513 wall={wall}", True, wall, 0)
            assert int(want["stats"][2]) > 0


# ---- 3. every hand-written scene, against the hand-written bytes ----

_CASES = cc.cases()


@pytest.mark.parametrize("name,s,want", _CASES, ids=[c[0] for c in _CASES])
def test_hand_cases(ra, name, s, want):
    with _pipeline(ra, s, s["vertices"], s["indices"]) as p:
        _cull_given(p, s, want, name)
        _cull_given(p, s, want, name + ", asynchronous", async_=True)


# ---- 4. structural edges, read from the plan ----

def _plan_sizes(tmp):
    exe = os.path.join(str(tmp), "cluster_plan_sizes")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "native", "cluster_plan_check.cpp"), "-o", exe])
    return json.loads(subprocess.check_output([exe, "sizes"]))


EDGE_PARTS = ("tiles", "cull grid cap", "head grid cap")


def _filled(w, clusters, pattern_of, base):
    """W = w work items: instances of `clusters` clusters and one shorter one. pattern_of(k): the ladder of k clusters."""
    whole, rest = divmod(w, clusters)
    return cc.ladder_scene([pattern_of(clusters)] + ([pattern_of(rest)] if rest else []), [0] * whole + ([1] if rest else []), base=base)


def _edge_scenes(sizes, part):
    """[(name, scene, want)] of one part. "tiles": ladders whose work items, and ladders whose HEADS, fall one below, at and one
    above 64 (a survive word), the item tile and the head tile; runs and heads placed on tile edges. "cull grid cap" / "head grid
    cap": W — and the call's bound on it, work_capacity = W — one below, at and one above the size at which the plan stops
    growing that grid and the grid starts to loop (max_blocks tiles), and well above it under the library's own bound."""
    item, head, blocks = sizes["item_tile"], sizes["head_tile"], sizes["max_blocks"]
    out = []
    if part != "tiles":
        cap = blocks * (item if part == "cull grid cap" else head)
        for w in (cap - 1, cap, cap + 1):
            s, want = _filled(w, 128, lambda k: "1" * k, base=7)       # one run per instance
            s["work_capacity"] = w
            assert int(want["stats"][2]) == w
            out.append((f"{part}: W = bound = {w}", s, want))
        # the library's own bound, two tiles past the cap: 128-cluster instances, the first and last cluster culled
        n = (cap + 2 * (item if part == "cull grid cap" else head)) // 128
        out.append((f"{part}: loops", *cc.ladder_scene(["0" + "1" * 126 + "0"], [0] * n, base=3)))
        return out
    for edge in (64, item, head):
        for w in (edge - 1, edge, edge + 1):
            # W work items of 8-cluster instances and one shorter one: every cluster survives (one head per instance) ...
            out.append((f"W={w} whole", *_filled(w, 8, lambda k: "1" * k, base=1)))
            # ... and alternating: every second work item is a head
            out.append((f"W={w} alternating", *_filled(w, 8, lambda k: ("10" * 4)[:k], base=2)))
        for h in (edge - 1, edge, edge + 1):
            # h HEADS: one-cluster instances (W = h: every bit of a full survive word is a head) ...
            s, want = cc.ladder_scene(["1"], [0] * h, base=9)
            assert int(want["stats"][0]) == h == int(want["stats"][2])
            out.append((f"heads={h}, one cluster each", s, want))
            # ... and in 2 h work items: '10' ladders, four heads per 8-cluster instance and one shorter instance
            s, want = _filled(2 * h, 8, lambda k: ("10" * 4)[:k], base=10)
            assert int(want["stats"][0]) == h and int(want["stats"][2]) == 2 * h
            out.append((f"heads={h} in {2 * h} items", s, want))
    # a run that spans three item tiles and three head tiles, starting in the middle of one
    long_run = np.ones(2 * head + 700, bool)
    long_run[:5] = False
    out.append(("a run over three tiles", *cc.ladder_scene(["1" * 1000, long_run, "101"], [0, 1, 2, 0], base=4)))
    # a head on a tile's first item: the second instance starts at item `item`, the third at item `head`
    out.append(("heads on first items", *cc.ladder_scene(["1" * item, "1" * (head - item), "11"], [0, 1, 2, 2], base=5)))
    # members only in the last instance tile (and only its last instance)
    n = 2 * sizes["instance_tile"] + 1
    bits = np.zeros(n, bool)
    bits[-1] = True
    out.append(("members in the last tile", *cc.ladder_scene(["1101"], [0] * n, base=6, bits=bits)))
    return out


def _run_edge_scenes(ra, scenes):
    for name, s, want in scenes:
        with _pipeline(ra, s, s["vertices"], s["indices"]) as p:
            _cull_given(p, s, want, name, work_capacity=s.get("work_capacity", 0), async_=True)


@pytest.mark.parametrize("part", EDGE_PARTS)
def test_structural_edges(ra, tmp_path, part):
    sizes = _plan_sizes(tmp_path)
    scenes = _edge_scenes(sizes, part)
    by_name = {name: want for name, _, want in scenes}
    if part == "tiles":
        assert by_name["a run over three tiles"]["cmds"]["indexCount"].max() == 192 * (2 * sizes["head_tile"] + 695)
        for edge in (64, sizes["item_tile"], sizes["head_tile"]):
            assert {int(w["stats"][0]) for w in by_name.values()} >= {edge - 1, edge, edge + 1}       # heads on every edge
            assert {int(w["stats"][2]) for w in by_name.values()} >= {edge - 1, edge, edge + 1}       # work items on every edge
    else:
        cap = sizes["max_blocks"] * (sizes["item_tile"] if part == "cull grid cap" else sizes["head_tile"])
        assert [int(w["stats"][2]) for w in by_name.values()][:3] == [cap - 1, cap, cap + 1]
        assert int(by_name[f"{part}: loops"]["stats"][2]) > cap + (sizes["item_tile"] if part == "cull grid cap" else sizes["head_tile"])
    _run_edge_scenes(ra, scenes)


_EDGE_CHILD = r'''
import os, sys
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
os.environ["MIP_LIBRARY"] = os.path.join(root, "renderer_amd", "lib", "libmi_instance_pipeline_dbg.so")
import renderer_amd
import test_gpu_clusters as TC
TC._run_edge_scenes(renderer_amd, TC._edge_scenes(TC._plan_sizes(sys.argv[2]), sys.argv[3]))
print("CLUSTER-EDGES-OK")
'''


@pytest.mark.parametrize("part", EDGE_PARTS)
@pytest.mark.parametrize("tiles", ["reverse", "scramble"])
def test_structural_edges_in_any_dispatch_order(tiles, part, tmp_path):
    e = dict(os.environ, MIP_DEBUG_TILE_ORDER=tiles)
    out = subprocess.run([sys.executable, "-c", _EDGE_CHILD, ROOT, str(tmp_path), part], capture_output=True, text=True, timeout=600, env=e)
    assert out.returncode == 0 and "CLUSTER-EDGES-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ---- 5. overflow ----

@pytest.mark.parametrize("frames_in_flight", [1, 2])
def test_overflow_rules(ra, frames_in_flight):
    s = ra.scene.make_scene(3, n=257)
    vertices, indices = ra.scene.make_geometry(s["meshes"], "strips")
    boxes = cr.cluster_boxes(s["meshes"], vertices, indices)
    policy = make_lod_policy(lr.DISTANCE, lr.PIN_SWITCH_SQ)
    with _pipeline(ra, s, vertices, indices, frames_in_flight=frames_in_flight) as p:
        f = T._Frame(257)
        frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=17)
        p.run_device(frame, **f.kwargs())
        bitmap = f.host_bitmap()
        full = cr.cull_clusters(s, boxes, bitmap, lr.DISTANCE, lr.PIN_SWITCH_SQ, cmd_capacity=1 << 20, first_instance_base=17)
        heads, w, members = int(full["stats"][0]), int(full["stats"][2]), int(full["stats"][3])
        assert heads > 2 and w > heads

        def cull(out, async_=False, **kw):
            if frames_in_flight > 1:   # behind a frame of its own: consecutive calls go to different slots
                p.run_device(frame, async_=True, **f.kwargs())
            p.cull_clusters(frame, f.bitmap.data_ptr(), policy, out.outputs(async_=async_, **kw))

        def overflows(out, async_, **kw):
            """MIP_ERR_CAPACITY once: from the call — also with a frame of the context still in flight — or from mip_wait for an
            asynchronous one; then the context is clean again."""
            with pytest.raises(ra.MipError) as e:
                cull(out, async_, **kw)
                p.wait()
            assert e.value.code == CAPACITY
            p.wait()

        for async_ in (False, True):
            for cap in (heads - 1, 0):          # the first `cap` commands exactly, the true stats, MIP_ERR_CAPACITY
                out = _Out(heads)
                overflows(out, async_, cmd_capacity=cap)
                _check(out, full["cmds"], full["stats"], f"cmd_capacity {cap} async={async_}", count=cap)
            out = _Out(heads)                   # W - 1: nothing but the zero count and the refusal's stats
            overflows(out, async_, work_capacity=w - 1)
            _check(out, full["cmds"], [0, 0, w, members], f"work_capacity W - 1 async={async_}", count=0)
            out = _Out(heads)                   # a fitting call on the same context is complete
            cull(out, async_, cmd_capacity=heads, work_capacity=w)
            p.wait()
            _check(out, full["cmds"], full["stats"], f"fitting call async={async_}")
        if frames_in_flight > 1:
            # two calls in flight behind two frames, the first one overflows: mip_wait reports it, the second is complete
            a, b = _Out(heads), _Out(heads)
            cull(a, True, cmd_capacity=1)
            cull(b, True)
            with pytest.raises(ra.MipError) as e:
                p.wait()
            assert e.value.code == CAPACITY
            _check(a, full["cmds"], full["stats"], "in flight, cut", count=1)
            _check(b, full["cmds"], full["stats"], "in flight, whole")
            p.wait()
            # an asynchronous call overflows; a synchronous call that fits, made before any mip_wait, is NOT charged with it
            # (on the same slot or another): it returns MIP_OK and is complete, and mip_wait reports the first call's overflow once
            for same_slot in (False, True):
                a, b = _Out(heads), _Out(heads)
                cull(a, True, cmd_capacity=1)
                if same_slot:
                    p.cull_clusters(frame, f.bitmap.data_ptr(), policy, b.outputs())
                else:
                    cull(b, False)
                _check(b, full["cmds"], full["stats"], f"a fitting synchronous call behind an overflow, same slot: {same_slot}")
                with pytest.raises(ra.MipError) as e:
                    p.wait()
                assert e.value.code == CAPACITY
                _check(a, full["cmds"], full["stats"], "the overflow behind it", count=1)
                p.wait()


# ---- 6. every refusal writes nothing and leaves the context usable ----

def test_refusals_write_nothing(ra):
    name, s, want = _CASES[0]
    with _pipeline(ra, s, s["vertices"], s["indices"]) as p:
        lib, ctx = p._lib, p._ctx
        bm = _device_bitmap(s["bitmap"])
        out = _Out(4)
        frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=s["base"])
        policy = make_lod_policy(lr.DISTANCE, cc.PIN)
        import torch
        pyr = torch.zeros(64, dtype=torch.float32, device=T._dev())
        torch.cuda.synchronize()

        def call(frame=frame, bitmap=bm.data_ptr(), policy=policy, occ=None, o=None, null_out=False):
            o = o if o is not None else out.outputs()
            return lib.mip_cull_clusters(ctx, C.addressof(frame) if frame is not None else None, bitmap, C.addressof(policy) if policy is not None else None,
                                         C.addressof(occ) if occ is not None else None, None if null_out else C.addressof(o))

        def outputs(**kw):
            o = out.outputs()
            for k, v in kw.items():
                setattr(o, k, v)
            return o

        def occlusion(**kw):
            occ = make_occlusion(8, 8, pyr.data_ptr(), ra.scene.default_pv())
            for k, v in kw.items():
                setattr(occ, k, v)
            return occ

        bad_policy = make_lod_policy(lr.DISTANCE, cc.PIN)
        bad_policy.switch_sq[1] = 1.0           # decreases
        wrong_size = make_lod_policy(lr.DISTANCE, cc.PIN)
        wrong_size.struct_size = 24
        refused = [
            ("NULL frame", call(frame=None)), ("NULL bitmap", call(bitmap=None)), ("NULL policy", call(policy=None)), ("NULL out", call(null_out=True)),
            ("NULL cluster_cmds", call(o=outputs(cluster_cmds=None))), ("NULL cmd_count", call(o=outputs(cmd_count=None))),
            ("struct_size", call(o=outputs(struct_size=36))), ("unknown flags", call(o=outputs(flags=_lib.MIP_OUT_DEVICE | 0x10))),
            ("host outputs", call(o=outputs(flags=0))), ("misaligned", call(o=outputs(cmd_count=out.scal.data_ptr() + 2))),
            ("decreasing thresholds", call(policy=bad_policy)), ("policy struct_size", call(policy=wrong_size)),
            ("occlusion struct_size", call(occ=occlusion(struct_size=100))), ("occlusion flags", call(occ=occlusion(flags=1))),
            ("candidates", call(occ=occlusion(candidates=bm.data_ptr()))), ("occluded_bitmap", call(occ=occlusion(occluded_bitmap=bm.data_ptr()))),
            ("NULL pyramid", call(occ=occlusion(pyramid=None))), ("extent", call(occ=occlusion(width=0))),
            ("extent above the limit", call(occ=occlusion(height=_lib.MIP_MAX_DEPTH_EXTENT + 1))),
        ]
        for what, rc in refused:
            assert rc == INVALID, (what, rc)
        good = out.outputs()
        assert lib.mip_cull_clusters(None, C.addressof(frame), bm.data_ptr(), C.addressof(policy), None, C.addressof(good)) == INVALID
        assert out.untouched()
        _cull_given(p, s, want, name + " after the refusals")     # the context is usable
    # no instances: not ready
    with ra.InstancePipeline(max_instances=4, max_meshes=len(s["meshes"])) as p:
        p.set_mesh_table(s["meshes"])
        p.set_geometry(s["vertices"], s["indices"])
        p.build_clusters()
        fresh = _Out(4)
        with pytest.raises(ra.MipError) as e:
            p.cull_clusters(make_frame(s["planes"], s["cam_pos"]), bm.data_ptr(), policy, fresh.outputs())
        assert e.value.code == NOT_READY and fresh.untouched()
