"""mip_list_cluster_triangles on the GPU (include/mi_instance_pipeline.h): every byte of the entries, the triangle masks, the
count, the draw arguments and the six stats against the numpy restatement (tests/cluster_triangle_list_restatement.py), against
the hand-written answers and the designed geometry (tests/cluster_triangle_list_cases.py), and on the same context against
mip_list_clusters (the entries are a subsequence of its list) and mip_cull_cluster_triangles / _cone (the masks expand into its
stream byte for byte, stats 1 to 5 are equal); the structural edges of the launch plan
(renderer_amd/csrc/cluster_triangle_list_plan.hpp), also with reversed and scrambled tiles under the diagnostic library; two
frames in flight and the calls that share the slot's scratch; both overflow rules; every refusal. Every output buffer is filled
with a sentinel in front and behind and compared whole. Not reference behaviour: parity is with the restatement."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_cases as cc
import cluster_cone_restatement as ccr
import cluster_restatement as cr
import cluster_triangle_cases as ctc
import cluster_triangle_list_cases as ctlc
import cluster_triangle_list_restatement as ctlr
import lod_restatement as lr
import occlusion_restatement as orr
import test_gpu_batch as T
import test_gpu_batch_lods as TL
import test_gpu_cluster_list as TLS
import test_gpu_cluster_triangles as TT
import test_gpu_clusters as TC
from renderer_amd import _lib
from renderer_amd.pipeline import make_cluster_cone, make_cluster_triangle_list_outputs, make_frame, make_lod_policy, make_occlusion

pytestmark = pytest.mark.gpu
ROOT = TC.ROOT
SENTINEL = T.SENTINEL
ra = T.ra   # the module's library fixture
NOT_READY, INVALID, CAPACITY = -6, -1, -4
FRONT_ROWS = 1   # sentinel rows in front of the entries (16 bytes) and of the masks (8 bytes)


class _Out:
    """Device outputs of mip_list_cluster_triangles, filled with a sentinel: room for `cap` entries and masks, a row in front of
    each and 3 rows behind that nobody may touch; scal[1] = entry_count, scal[3:7] = draw_args, scal[8:14] = stats, the words
    between, in front and behind are guards."""

    def __init__(self, cap, args=True, stats=True):
        import torch

        fill = T._i32(SENTINEL)
        self.cap, self.args, self.stats = int(cap), args, stats
        self.entries = torch.full((FRONT_ROWS + self.cap + 3, 4), fill, dtype=torch.int32, device=T._dev())
        self.masks = torch.full((FRONT_ROWS + self.cap + 3, 2), fill, dtype=torch.int32, device=T._dev())
        self.scal = torch.full((16,), fill, dtype=torch.int32, device=T._dev())
        torch.cuda.synchronize()

    def outputs(self, entry_capacity=None, work_capacity=0, async_=False):
        return make_cluster_triangle_list_outputs(self.entries.data_ptr() + 16 * FRONT_ROWS, self.masks.data_ptr() + 8 * FRONT_ROWS,
                                                  self.cap if entry_capacity is None else entry_capacity, self.scal.data_ptr() + 4,
                                                  self.scal.data_ptr() + 12 if self.args else 0, self.scal.data_ptr() + 32 if self.stats else 0,
                                                  work_capacity=work_capacity, async_=async_)

    def result(self):
        import torch

        torch.cuda.synchronize()
        return (self.entries.cpu().numpy().view(np.uint32), np.ascontiguousarray(self.masks.cpu().numpy()).view(np.uint64).reshape(-1),
                self.scal.cpu().numpy().view(np.uint32))

    def written(self):
        """(entries, masks) the call wrote: the first entry_count rows behind the guard."""
        entries, masks, scal = self.result()
        count = int(scal[1])
        return entries[FRONT_ROWS: FRONT_ROWS + count], masks[FRONT_ROWS: FRONT_ROWS + count]

    def untouched(self):
        return all((a.view(np.uint32) == SENTINEL).all() for a in self.result())


SENTINEL64 = (SENTINEL << 32) | SENTINEL


def _check(out, want, what, count=None, stats=None):
    """The first `count` entries and masks are want's (all of them unless a capacity cut the list), the scalars are the count,
    {192, count, 0, 0} and `stats` (want's unless given), and no other word of any buffer was written."""
    entries, masks, scal = out.result()
    count = len(want["entries"]) if count is None else count
    stats = want["stats"] if stats is None else stats
    assert int(scal[1]) == count, (what, "entry_count", int(scal[1]), count)
    if out.args:
        assert scal[3:7].tolist() == [192, count, 0, 0], (what, "draw_args", scal[3:7].tolist())
    else:
        assert (scal[3:7] == SENTINEL).all(), what
    if out.stats:
        assert scal[8:14].tolist() == [int(v) for v in stats], (what, "stats", scal[8:14].tolist(), [int(v) for v in stats])
    else:
        assert (scal[8:14] == SENTINEL).all(), what
    assert scal[0] == SENTINEL and scal[2] == SENTINEL and scal[7] == SENTINEL and (scal[14:] == SENTINEL).all(), (what, "a guard word was written")
    lo, hi = FRONT_ROWS, FRONT_ROWS + count
    assert entries[lo:hi].tobytes() == np.ascontiguousarray(want["entries"][:count]).tobytes(), (what, "entries")
    assert np.array_equal(masks[lo:hi], np.asarray(want["masks"][:count], np.uint64)), (what, "masks")
    assert (entries[:lo] == SENTINEL).all() and (entries[hi:] == SENTINEL).all(), (what, "entries in front of the list or at / behind entry_count were written")
    assert (masks[:lo] == SENTINEL64).all() and (masks[hi:] == SENTINEL64).all(), (what, "masks in front of the list or at / behind entry_count were written")


def _list_given(p, s, want, what, pv=ctc.PV, work_capacity=0, async_=False, args=True, stats=True, extra=0):
    """mip_list_cluster_triangles over the scene's own bitmap (uploaded) under the pin policy, with room for `extra` entries more
    than the answer has; the outputs against `want`."""
    bm = TC._device_bitmap(s["bitmap"])
    out = _Out(len(want["entries"]) + extra, args, stats)
    frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=s["base"], pv=pv)
    p.list_cluster_triangles(frame, bm.data_ptr(), make_lod_policy(lr.DISTANCE, cc.PIN), out.outputs(work_capacity=work_capacity, async_=async_))
    if async_:
        p.wait()
    _check(out, want, what)
    return out


def _against_the_neighbours(p, frame, bitmap_ptr, policy, out, indices, what, occ=None, cone=None):
    """On the same context, for the same arguments: the entries are a subsequence of what mip_list_clusters writes, in its
    order; the masks expand into what mip_cull_cluster_triangles / _cone writes, byte for byte; stats 1 to 5 are that call's."""
    entries, masks = out.written()
    _, _, scal = out.result()
    stats = scal[8:14]
    room = int(stats[1]) + 1
    lst = TLS._Out(room)
    p.list_clusters(frame, bitmap_ptr, policy, lst.outputs(), occlusion=occ, cone=cone)
    rows, lscal = lst.result()
    rows = rows[: int(lscal[0])]
    assert int(lscal[0]) == int(stats[1]), (what, "mip_list_clusters lists the surviving clusters")
    where = {r.tobytes(): k for k, r in enumerate(rows)}
    at = [where.get(e.tobytes(), -1) for e in entries]
    assert all(k >= 0 for k in at) and all(a < b for a, b in zip(at, at[1:])), (what, "not a subsequence of mip_list_clusters' list")
    tri = TT._Out(room, 3 * int(stats[4]))
    if cone is None:
        p.cull_cluster_triangles(frame, bitmap_ptr, policy, tri.outputs(), occlusion=occ)
    else:
        p.cull_cluster_triangles_cone(frame, bitmap_ptr, policy, cone, tri.outputs(), occlusion=occ)
    _, tscal, stream = tri.result()
    assert tscal[3:8].tolist() == stats[1:].tolist(), (what, "stats 1 to 5", tscal[2:8].tolist(), stats.tolist())
    e = np.ascontiguousarray(entries).view(ctlc.CLUSTER_ENTRY_DTYPE).reshape(-1)
    assert ctlr.expand(e, masks, indices).tobytes() == stream[: 3 * int(stats[4])].tobytes(), (what, "the masks do not expand into culled_indices")


# ---- 1. every hand-written scene: synchronous, asynchronous, with each optional output absent ----

_CASES = ctc.cases()
_ANSWERS = ctlc.answers()


@pytest.mark.parametrize("name,s,_tri", _CASES, ids=[c[0] for c in _CASES])
def test_hand_cases(ra, name, s, _tri):
    want = _ANSWERS[name]
    with TC._pipeline(ra, s, s["vertices"], s["indices"]) as p:
        out = _list_given(p, s, want, name, extra=2)
        _list_given(p, s, want, name + ", asynchronous", async_=True)
        _list_given(p, s, want, name + ", no draw_args", args=False)
        _list_given(p, s, want, name + ", no stats", stats=False, async_=True)
        _list_given(p, s, want, name + ", neither", args=False, stats=False)
        frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=s["base"], pv=ctc.PV)
        bm = TC._device_bitmap(s["bitmap"])
        _against_the_neighbours(p, frame, bm.data_ptr(), make_lod_policy(lr.DISTANCE, cc.PIN), out, s["indices"], name)


# ---- 2. the restatement over config 3 ----

def _frame_then_list(ra, p, s, vertices, indices, boxes, mode, sw, what, full_bitmap, wall, base, cone=None, cones=None):
    """mip_run, (the pyramid build,) mip_list_cluster_triangles over the frame's bitmap with no wait in between — or over a full
    bitmap uploaded first; every byte against the restatement, then the neighbours on the same context."""
    import torch

    n = s["n"]
    pv = ra.scene.default_pv()
    f = T._Frame(n)
    frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=base, pv=pv)
    given = TC._device_bitmap(np.full((n + 31) // 32, 0xFFFFFFFF, np.uint32)) if full_bitmap else None
    occ = None
    if wall:
        depth = torch.from_numpy(TC._WALL).to(T._dev())
        pyr = torch.full((ra.pipeline.depth_pyramid_layout(64, 32)["bytes"] // 4,), -1.0, dtype=torch.float32, device=T._dev())
        torch.cuda.synchronize()
        occ = make_occlusion(64, 32, pyr.data_ptr(), pv)
    cap = max(n, 1) * int(cr.cluster_table(s["meshes"])["C"].max())     # every cluster of every instance fits
    out = _Out(cap)
    policy = make_lod_policy(mode, sw)
    bitmap_ptr = (given if given is not None else f.bitmap).data_ptr()
    if n:
        p.run_device(frame, async_=True, **f.kwargs())
    if wall:
        p.build_depth_pyramid(depth.data_ptr(), 64, 32, pyr.data_ptr(), format=_lib.MIP_DEPTH_FLOAT32, async_=True)
    p.list_cluster_triangles(frame, bitmap_ptr, policy, out.outputs(async_=True), occlusion=occ, cone=cone)
    p.wait()
    bitmap = np.full((n + 31) // 32, 0xFFFFFFFF, np.uint32) if full_bitmap else f.host_bitmap()
    occlusion = dict(pv=pv, levels=orr.pyramid_levels(TC._WALL), width=64, height=32) if wall else None
    k = dict(cones=cones, eye=np.array(cone.eye[:], np.float32), facing=float(cone.facing)) if cone is not None else None
    want = ctlr.list_cluster_triangles(s, boxes, vertices, indices, bitmap, mode, sw, pv, cap, first_instance_base=base, occlusion=occlusion, cone=k)
    assert want["status"] == 0, what
    _check(out, want, what)
    if n:
        _against_the_neighbours(p, frame, bitmap_ptr, policy, out, indices, what, occ, cone)
    return want


@pytest.mark.parametrize("coned", [False, True], ids=["no cone", "cone"])
@pytest.mark.parametrize("n", [0, 1, 257, 4097])
def test_restatement_over_config_3(ra, n, coned):
    ordering = "patches" if coned else "strips" if n == 257 else "rows" if n % 2 else "shuffled"
    s = TL._sized(ra.scene.make_scene(3, n=max(n, 1)), n)
    vertices, indices = ra.scene.make_geometry(s["meshes"], ordering)
    boxes = cr.cluster_boxes(s["meshes"], vertices, indices)
    cones = ccr.cluster_cones(s["meshes"], vertices, indices, boxes) if coned else None
    cone = make_cluster_cone(ra.scene.default_pv()) if coned else None
    walled = free = None
    with TC._pipeline(ra, s, vertices, indices) as p:
        if coned:
            p.build_cluster_cones()
        for mode in (lr.DISTANCE, lr.RELATIVE):
            sw = TL._metric_thresholds(s, mode)
            for wall in (False, True):
                full_bitmap = wall != (mode == lr.RELATIVE)                # both bitmaps under both modes and with and without the wall
                base = (0xFFFFFFFF - n // 2) if full_bitmap else 3         # a base that wraps inside the scene
                want = _frame_then_list(ra, p, s, vertices, indices, boxes, mode, sw, f"n={n} {ordering} mode={mode} full={full_bitmap} wall={wall} cone={coned}",
                                        full_bitmap, wall, base, cone, cones)
                if mode == lr.DISTANCE:
                    walled, free = (want, free) if wall else (walled, want)
        if n == 257 and not coned:   # the known answer (tests/test_cluster_triangle_list_restatement.py): the pin policy, the frame's bitmap
            want = _frame_then_list(ra, p, s, vertices, indices, boxes, lr.DISTANCE, lr.PIN_SWITCH_SQ, "n=257 strips pin", False, False, 0)
            assert want["stats"].tolist() == [2581 - 83, 2581, 3127, 72, 78898, 162813]
    if n >= 257:
        assert int(free["stats"][0]) > 0 and int(walled["stats"][0]) > 0


# ---- 3. structural edges: the designed geometry, one-triangle clusters; the sizes are read from the plan ----

def _plan_sizes(tmp):
    exe = os.path.join(str(tmp), "cluster_triangle_list_plan_sizes")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "native", "cluster_triangle_list_plan_check.cpp"), "-o", exe])
    return json.loads(subprocess.check_output([exe, "sizes"]))


EDGE_PARTS = ("tiles", "words", "grid cap")
_ONE = dict(levels=["F", "B", "O"], triangles=[1, 1, 1])     # one-triangle clusters: W = the instances, one work item each
_F, _B, _O = 0, 1, 2


def _one(pattern, base):
    return ctlc.designed_scene(_ONE["levels"], np.asarray(pattern, np.int64), base=base, triangles=_ONE["triangles"])


def _edge_scenes(sizes, part):
    """[(name, scene, want, work_capacity)] of one part, all under the identity pv. "tiles": W one below, at and one above 64, the
    item tile and the list tile, the kinds mixed so that entries, surviving clusters and work items all differ. "words": a zero
    survive word between full ones; a full survive word whose non-empty word is zero between full ones; words in which exactly
    lane 0, exactly lane 63, only lane 0 and only lane 63 keep a triangle or keep none; a short last cluster in the last lane.
    "grid cap": W — and the call's bound on it — one below, at and one above the work items from which the test and write grids
    loop, read from the plan."""
    out = []
    if part == "tiles":
        for edge in (64, sizes["item_tile"], sizes["list_tile"]):
            for w in (edge - 1, edge, edge + 1):
                k = np.arange(w)
                out.append((f"W={w} mixed", *_one(np.where(k % 5 == 1, _B, np.where(k % 7 == 3, _O, _F)), base=1), 0))
                out.append((f"W={w} all keep", *_one(np.full(w, _F), base=0xFFFFFFFF - 5), 0))
        return out
    if part == "words":
        f, b, o = [_F] * 64, [_B] * 64, [_O] * 64
        out.append(("a zero survive word between full ones", *_one(f + o + f, base=2), 0))
        out.append(("a full survive word with a zero non-empty word between full ones", *_one(f + b + f, base=3), 0))
        out.append(("lane 0 empty", *_one(f + [_B] + [_F] * 63 + f, base=4), 0))
        out.append(("lane 63 empty", *_one(f + [_F] * 63 + [_B] + f, base=5), 0))
        out.append(("only lane 0 keeps", *_one(f + [_F] + [_B] * 63 + f, base=6), 0))
        out.append(("only lane 63 keeps", *_one(b + [_B] * 63 + [_F] + b, base=7), 0))
        out.append(("lane 0 culled, lane 63 empty", *_one([_O] + [_F] * 62 + [_B] + [_B] + [_F] * 62 + [_O], base=8), 0))
        # a level of 64 clusters whose last one, work item 63 and 127, holds 5 triangles; alternating and FRONT
        out.append(("a short last cluster in the last lane", *ctlc.designed_scene(["F" * 63 + "A", "B" * 63 + "F"], [0, 1], triangles=[63 * 64 + 5, 63 * 64 + 5], base=9), 0))
        return out
    assert sizes["test_grid_cap"] == sizes["write_grid_cap"] == sizes["max_blocks"] * sizes["item_tile"]
    cap = sizes["test_grid_cap"]
    for w in (cap - 1, cap, cap + 1):
        k = np.arange(w)
        out.append((f"W = bound = {w}", *_one(np.where(k % 3 == 1, _B, np.where(k % 1021 == 7, _O, _F)), base=7), w))
    return out


def _run_edge_scenes(ra, scenes):
    for name, s, want, work_capacity in scenes:
        assert int(want["stats"][2]) > 0
        with TC._pipeline(ra, s, s["vertices"], s["indices"]) as p:
            _list_given(p, s, want, name, work_capacity=work_capacity, async_=True, extra=2)


@pytest.mark.parametrize("part", EDGE_PARTS)
def test_structural_edges(ra, tmp_path, part):
    sizes = _plan_sizes(tmp_path)
    scenes = _edge_scenes(sizes, part)
    if part == "tiles":
        for edge in (64, sizes["item_tile"], sizes["list_tile"]):
            assert {int(w["stats"][2]) for _, _, w, _ in scenes} >= {edge - 1, edge, edge + 1}       # work items on every edge
            assert {int(w["stats"][0]) for _, _, w, _ in scenes} >= {edge - 1, edge, edge + 1}       # entries on every edge
        assert (63, 64, 65, 1023, 1024, 1025, 16383, 16384, 16385) == tuple(sorted({int(w["stats"][2]) for _, _, w, _ in scenes}))
    elif part == "grid cap":
        cap = sizes["max_blocks"] * sizes["item_tile"]
        assert [int(w["stats"][2]) for _, _, w, _ in scenes] == [cap - 1, cap, cap + 1]
    else:
        by = {name: w for name, _, w, _ in scenes}
        assert by["a full survive word with a zero non-empty word between full ones"]["stats"].tolist() == [128, 192, 192, 192, 128, 192]
        assert by["a zero survive word between full ones"]["stats"].tolist() == [128, 128, 192, 192, 128, 128]
        assert by["a short last cluster in the last lane"]["masks"][63] == 0b10101 and by["a short last cluster in the last lane"]["masks"][64] == 0b11111
    _run_edge_scenes(ra, scenes)


_EDGE_CHILD = r'''
import os, sys
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
os.environ["MIP_LIBRARY"] = os.path.join(root, "renderer_amd", "lib", "libmi_instance_pipeline_dbg.so")
import renderer_amd
import test_gpu_cluster_triangle_list as TTL
TTL._run_edge_scenes(renderer_amd, TTL._edge_scenes(TTL._plan_sizes(sys.argv[2]), sys.argv[3]))
print("CLUSTER-TRIANGLE-LIST-EDGES-OK")
'''


@pytest.mark.parametrize("part", EDGE_PARTS)
@pytest.mark.parametrize("tiles", ["reverse", "scramble"])
def test_edges_in_any_dispatch_order(tiles, part, tmp_path):
    e = dict(os.environ, MIP_DEBUG_TILE_ORDER=tiles)
    out = subprocess.run([sys.executable, "-c", _EDGE_CHILD, ROOT, str(tmp_path), part], capture_output=True, text=True, timeout=600, env=e)
    assert out.returncode == 0 and "CLUSTER-TRIANGLE-LIST-EDGES-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ---- 4. context and scheduling; overflow ----

def _config_3(ra):
    s = ra.scene.make_scene(3, n=257)
    vertices, indices = ra.scene.make_geometry(s["meshes"], "strips")
    return s, vertices, indices, cr.cluster_boxes(s["meshes"], vertices, indices)


def test_two_frames_in_flight_and_the_shared_scratch(ra):
    """The call behind two frames in flight, and alternating with mip_list_clusters and mip_cull_cluster_triangles, which use
    the same slot's words, triangle words and tile sums: every call's outputs are whole."""
    s, vertices, indices, boxes = _config_3(ra)
    pv = ra.scene.default_pv()
    policy = make_lod_policy(lr.DISTANCE, lr.PIN_SWITCH_SQ)
    with TC._pipeline(ra, s, vertices, indices, frames_in_flight=2) as p:
        f = T._Frame(257)
        frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=17, pv=pv)
        p.run_device(frame, **f.kwargs())
        want = ctlr.list_cluster_triangles(s, boxes, vertices, indices, f.host_bitmap(), lr.DISTANCE, lr.PIN_SWITCH_SQ, pv, 1 << 20, first_instance_base=17)
        entries = len(want["entries"])
        outs = []
        for _ in range(4):                   # two slots, twice: no wait in between
            p.run_device(frame, async_=True, **f.kwargs())
            outs.append(_Out(entries))
            p.list_cluster_triangles(frame, f.bitmap.data_ptr(), policy, outs[-1].outputs(async_=True))
        p.wait()
        for k, out in enumerate(outs):
            _check(out, want, f"in flight {k}")
        # alternating on one slot with the two calls whose scratch it shares, smaller and larger bounds in turn
        room = int(want["stats"][1]) + 1
        for k in range(3):
            a = _Out(entries)
            p.list_cluster_triangles(frame, f.bitmap.data_ptr(), policy, a.outputs(async_=True, work_capacity=0 if k % 2 else int(want["stats"][2])))
            lst = TLS._Out(room)
            p.list_clusters(frame, f.bitmap.data_ptr(), policy, lst.outputs(async_=True))
            b = _Out(entries)
            p.list_cluster_triangles(frame, f.bitmap.data_ptr(), policy, b.outputs(async_=True))
            tri = TT._Out(room, 3 * int(want["stats"][4]))
            p.cull_cluster_triangles(frame, f.bitmap.data_ptr(), policy, tri.outputs(async_=True))
            c = _Out(entries)
            p.list_cluster_triangles(frame, f.bitmap.data_ptr(), policy, c.outputs(async_=True))
            p.wait()
            for what, out in (("first", a), ("behind mip_list_clusters", b), ("behind mip_cull_cluster_triangles", c)):
                _check(out, want, f"round {k}: {what}")
            _, lscal = lst.result()
            assert int(lscal[0]) == int(want["stats"][1])
            _, tscal, stream = tri.result()
            assert tscal[3:8].tolist() == want["stats"][1:].tolist()
            assert ctlr.expand(want["entries"], want["masks"], indices).tobytes() == stream[: 3 * int(want["stats"][4])].tobytes()


@pytest.mark.parametrize("frames_in_flight", [1, 2])
def test_overflow_rules(ra, frames_in_flight):
    s, vertices, indices, boxes = _config_3(ra)
    pv = ra.scene.default_pv()
    policy = make_lod_policy(lr.DISTANCE, lr.PIN_SWITCH_SQ)
    with TC._pipeline(ra, s, vertices, indices, frames_in_flight=frames_in_flight) as p:
        f = T._Frame(257)
        frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=17, pv=pv)
        p.run_device(frame, **f.kwargs())
        full = ctlr.list_cluster_triangles(s, boxes, vertices, indices, f.host_bitmap(), lr.DISTANCE, lr.PIN_SWITCH_SQ, pv, 1 << 20, first_instance_base=17)
        entries, w, members = int(full["stats"][0]), int(full["stats"][2]), int(full["stats"][3])
        assert full["stats"].tolist() == [2581 - 83, 2581, 3127, 72, 78898, 162813]

        def call(out, async_=False, **kw):
            if frames_in_flight > 1:   # behind a frame of its own: consecutive calls go to different slots
                p.run_device(frame, async_=True, **f.kwargs())
            p.list_cluster_triangles(frame, f.bitmap.data_ptr(), policy, out.outputs(async_=async_, **kw))

        def overflows(out, async_, **kw):
            """MIP_ERR_CAPACITY once: from the call, or from mip_wait for an asynchronous one; then the context is clean again."""
            with pytest.raises(ra.MipError) as e:
                call(out, async_, **kw)
                p.wait()
            assert e.value.code == CAPACITY
            p.wait()

        for async_ in (False, True):
            for cap in (entries - 1, 0):        # the first `cap` entries and masks exactly, the true six stats, MIP_ERR_CAPACITY
                out = _Out(entries)
                overflows(out, async_, entry_capacity=cap)
                _check(out, full, f"entry_capacity {cap} async={async_}", count=cap)
            out = _Out(entries)                 # W - 1: nothing but the zero count, {192, 0, 0, 0} and the refusal's stats
            overflows(out, async_, work_capacity=w - 1)
            _check(out, full, f"work_capacity W - 1 async={async_}", count=0, stats=[0, 0, w, members, 0, 0])
            # a mip_cull_clusters in between is charged with nothing
            cmds = TC._Out(int(full["stats"][1]) + 8)
            p.cull_clusters(frame, f.bitmap.data_ptr(), policy, cmds.outputs())
            p.wait()
            out = _Out(entries)                 # a fitting call on the same context is complete
            call(out, async_, entry_capacity=entries, work_capacity=w)
            p.wait()
            _check(out, full, f"fitting call async={async_}")
        if frames_in_flight > 1:
            # an asynchronous call overflows; a synchronous mip_cull_clusters and a synchronous call of this kind that fit, made
            # before any mip_wait, are NOT charged with it; mip_wait reports it once
            a, b = _Out(entries), _Out(entries)
            call(a, True, entry_capacity=1)
            cmds = TC._Out(int(full["stats"][1]) + 8)
            p.cull_clusters(frame, f.bitmap.data_ptr(), policy, cmds.outputs())
            call(b, False)
            _check(b, full, "a fitting synchronous call behind an overflow")
            with pytest.raises(ra.MipError) as e:
                p.wait()
            assert e.value.code == CAPACITY
            _check(a, full, "the overflow behind it", count=1)
            p.wait()


# ---- 5. every refusal writes nothing and leaves the context usable ----

def test_refusals_write_nothing(ra):
    name, s, _tri = _CASES[[c[0] for c in _CASES].index("short last cluster")]
    want = _ANSWERS[name]
    with TC._pipeline(ra, s, s["vertices"], s["indices"]) as p:
        lib, ctx = p._lib, p._ctx
        bm = TC._device_bitmap(s["bitmap"])
        out = _Out(4)
        frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=s["base"], pv=ctc.PV)
        policy = make_lod_policy(lr.DISTANCE, cc.PIN)
        good_cone = make_cluster_cone(eye=(0, 0, 9), facing=1)
        import torch
        pyr = torch.zeros(64, dtype=torch.float32, device=T._dev())
        torch.cuda.synchronize()

        def call(frame=frame, bitmap=bm.data_ptr(), policy=policy, occ=None, cone=None, o=None, null_out=False):
            o = o if o is not None else out.outputs()
            return lib.mip_list_cluster_triangles(ctx, C.addressof(frame) if frame is not None else None, bitmap, C.addressof(policy) if policy is not None else None,
                                                  C.addressof(occ) if occ is not None else None, C.addressof(cone) if cone is not None else None,
                                                  None if null_out else C.addressof(o))

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

        def cone(**kw):
            c = make_cluster_cone(eye=(0, 0, 9), facing=1)
            for k, v in kw.items():
                setattr(c, k, v)
            return c

        bad_policy = make_lod_policy(lr.DISTANCE, cc.PIN)
        bad_policy.switch_sq[1] = 1.0           # decreases
        wrong_size = make_lod_policy(lr.DISTANCE, cc.PIN)
        wrong_size.struct_size = 24
        e0, m0, s0 = out.entries.data_ptr() + 16 * FRONT_ROWS, out.masks.data_ptr() + 8 * FRONT_ROWS, out.scal.data_ptr()
        refused = [
            ("NULL frame", call(frame=None)), ("NULL bitmap", call(bitmap=None)), ("NULL policy", call(policy=None)), ("NULL out", call(null_out=True)),
            ("NULL cluster_entries", call(o=outputs(cluster_entries=None))), ("NULL entry_count", call(o=outputs(entry_count=None))),
            ("NULL triangle_masks", call(o=outputs(triangle_masks=None))), ("masks 4-byte aligned only", call(o=outputs(triangle_masks=m0 + 4))),
            ("masks overlap the entries", call(o=outputs(triangle_masks=e0 + 16))), ("masks end inside the entries", call(o=outputs(triangle_masks=e0 - 8))),
            ("the entries end inside the masks", call(o=outputs(cluster_entries=m0 - 56))),
            ("masks overlap entry_count", call(o=outputs(entry_count=m0 + 8))), ("masks overlap draw_args", call(o=outputs(draw_args=m0 + 28))),
            ("masks overlap stats", call(o=outputs(stats=m0 - 4))),
            ("struct_size", call(o=outputs(struct_size=48))), ("the list's struct_size", call(o=outputs(struct_size=C.sizeof(_lib.MipClusterListOutputs)))),
            ("unknown flags", call(o=outputs(flags=_lib.MIP_OUT_DEVICE | 0x10))),
            ("host outputs", call(o=outputs(flags=0))), ("misaligned count", call(o=outputs(entry_count=s0 + 6))),
            ("misaligned args", call(o=outputs(draw_args=s0 + 13))), ("misaligned stats", call(o=outputs(stats=s0 + 33))),
            ("entries 4-byte aligned only", call(o=outputs(cluster_entries=e0 + 4))), ("entries 8-byte aligned only", call(o=outputs(cluster_entries=e0 + 8))),
            ("decreasing thresholds", call(policy=bad_policy)), ("policy struct_size", call(policy=wrong_size)),
            ("occlusion struct_size", call(occ=occlusion(struct_size=100))), ("occlusion flags", call(occ=occlusion(flags=1))),
            ("candidates", call(occ=occlusion(candidates=bm.data_ptr()))), ("occluded_bitmap", call(occ=occlusion(occluded_bitmap=bm.data_ptr()))),
            ("NULL pyramid", call(occ=occlusion(pyramid=None))), ("extent", call(occ=occlusion(width=0))),
            ("extent above the limit", call(occ=occlusion(height=_lib.MIP_MAX_DEPTH_EXTENT + 1))),
            ("cone struct_size", call(cone=cone(struct_size=20))), ("cone flags", call(cone=cone(flags=1))), ("cone facing", call(cone=cone(facing=0.5))),
        ]
        for what, rc in refused:
            assert rc == INVALID, (what, rc)
        good = out.outputs()
        assert lib.mip_list_cluster_triangles(None, C.addressof(frame), bm.data_ptr(), C.addressof(policy), None, None, C.addressof(good)) == INVALID
        assert call(cone=good_cone) == NOT_READY        # a cluster table, no cone table
        assert out.untouched()
        _list_given(p, s, want, name + " after the refusals")     # the context is usable, without a cone
        p.build_cluster_cones()
        assert call(cone=good_cone) == 0 and not out.untouched()
        # stale tables: a new cluster table makes the cones stale, new geometry the cluster table
        fresh = _Out(4)
        p.build_clusters()
        assert call(cone=good_cone, o=fresh.outputs()) == NOT_READY and fresh.untouched()
        p.set_geometry(s["vertices"], s["indices"])
        assert call(o=fresh.outputs()) == NOT_READY and call(cone=good_cone, o=fresh.outputs()) == NOT_READY and fresh.untouched()
        p.build_clusters()
        _list_given(p, s, want, name + " after the rebuild")
    # no instances: not ready
    with ra.InstancePipeline(max_instances=4, max_meshes=len(s["meshes"])) as p:
        p.set_mesh_table(s["meshes"])
        p.set_geometry(s["vertices"], s["indices"])
        p.build_clusters()
        fresh = _Out(4)
        with pytest.raises(ra.MipError) as e:
            p.list_cluster_triangles(make_frame(s["planes"], s["cam_pos"], pv=ctc.PV), bm.data_ptr(), policy, fresh.outputs())
        assert e.value.code == NOT_READY and fresh.untouched()
