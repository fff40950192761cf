"""mip_cull_cluster_triangles on the GPU (include/mi_instance_pipeline.h): every byte of the commands, the count, the six stats
and the index stream against the numpy restatement (tests/cluster_triangle_restatement.py) and against the hand-written scenes
(tests/cluster_triangle_cases.py); against mip_run's own per-triangle stage; the structural edges of the launch plan
(renderer_amd/csrc/cluster_triangle_plan.hpp), also with reversed and scrambled tiles under the diagnostic library; the three
overflow rules; every refusal. Every output buffer is filled with a sentinel and compared whole. Not reference behaviour:
parity is with the restatement.

The grid edges are run with one-triangle clusters at the test / write kernels' cap (2 048 tiles of 1 024 items). The commands
kernel's cap (2 048 tiles of 16 384 items, 33.5 M work items) is not run: 33.5 M instances take over a gigabyte of inputs and
many seconds of numpy per case; that kernel's loop is the one mip_cull_clusters' commands kernel has, run past its cap there."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_cases as cc
import cluster_restatement as cr
import cluster_triangle_cases as ctc
import cluster_triangle_restatement as ctr
import lod_restatement as lr
import numpy_restatement as nr
import occlusion_restatement as orr
import test_gpu_batch as T
import test_gpu_batch_lods as TL
import test_gpu_clusters as TC
from renderer_amd import _lib
from renderer_amd.pipeline import DRAW_CMD_DTYPE, MESH_DTYPE, make_cluster_triangle_outputs, make_frame, make_lod_policy, make_occlusion

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = T.SENTINEL
ra = T.ra   # the module's library fixture
NOT_READY, INVALID, CAPACITY = -6, -1, -4


class _Out:
    """Device outputs of mip_cull_cluster_triangles, filled with a sentinel: room for `cap` commands + 3 entries and `room`
    indices + 6 words nobody may touch; scal[0] = cmd_count, scal[2:8] = stats."""

    def __init__(self, cap, room, stats=True):
        import torch

        fill = T._i32(SENTINEL)
        self.cap, self.room, self.stats = int(cap), int(room), stats
        self.cmds = torch.full((self.cap + 3, 5), fill, dtype=torch.int32, device=T._dev())
        self.scal = torch.full((12,), fill, dtype=torch.int32, device=T._dev())
        self.stream = torch.full((self.room + 6,), fill, dtype=torch.int32, device=T._dev())
        torch.cuda.synchronize()

    def outputs(self, cmd_capacity=None, index_capacity=None, work_capacity=0, async_=False):
        return make_cluster_triangle_outputs(self.cmds.data_ptr(), self.cap if cmd_capacity is None else cmd_capacity, self.scal.data_ptr(),
                                             self.stream.data_ptr(), self.room if index_capacity is None else index_capacity,
                                             stats=self.scal.data_ptr() + 8 if self.stats else 0, work_capacity=work_capacity, async_=async_)

    def result(self):
        import torch

        torch.cuda.synchronize()
        return self.cmds.cpu().numpy().view(np.uint32), self.scal.cpu().numpy().view(np.uint32), self.stream.cpu().numpy().view(np.uint32)

    def untouched(self):
        return all((a == SENTINEL).all() for a in self.result())


def _check(out, want, what, count=None, written=True):
    """The first `count` entries are want's commands (all of them unless a capacity cut the list), the stream is want's (nothing
    of it when `written` is false), the stats are want's six words, and nothing else was written."""
    cmds, scal, stream = out.result()
    count = len(want["cmds"]) if count is None else count
    assert int(scal[0]) == count, (what, "cmd_count", int(scal[0]), count)
    assert cmds[:count].tobytes() == np.ascontiguousarray(want["cmds"][:count]).tobytes(), (what, "commands")
    assert (cmds[count:] == SENTINEL).all(), (what, "entries at or behind cmd_count were written")
    if out.stats:
        assert scal[2:8].tolist() == [int(v) for v in want["stats"]], (what, "stats", scal[2:8].tolist(), list(want["stats"]))
    else:
        assert (scal[2:8] == SENTINEL).all(), what
    assert scal[1] == SENTINEL and (scal[8:] == SENTINEL).all(), what
    n = len(want["stream"]) if written else 0
    assert np.array_equal(stream[:n], want["stream"][:n]), (what, "index stream")
    assert (stream[n:] == SENTINEL).all(), (what, "words at or behind the stream's end were written")


def _cull_given(p, s, want, what, pv, cmd_capacity=None, work_capacity=0, async_=False):
    """mip_cull_cluster_triangles over the scene's own bitmap (uploaded) under the pin policy; the outputs against `want`."""
    bm = TC._device_bitmap(s["bitmap"])
    out = _Out(len(want["cmds"]) if cmd_capacity is None else cmd_capacity, len(want["stream"]))
    frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=s["base"], pv=pv)
    p.cull_cluster_triangles(frame, bm.data_ptr(), make_lod_policy(lr.DISTANCE, cc.PIN), out.outputs(work_capacity=work_capacity, async_=async_))
    if async_:
        p.wait()
    _check(out, want, what)
    return out


# ---- 1. the restatement over the repository's scenes; the two device paths ----

def _frame_then_cull(ra, p, s, vertices, indices, boxes, mode, sw, what, wall, base, against_the_stage=False):
    """mip_run, (the pyramid build,) mip_cull_cluster_triangles over the frame's bitmap with no wait in between; every byte
    against the restatement. against_the_stage: the frame also runs the per-triangle stage, and its stream, filtered on the CPU
    to the surviving clusters, is the new call's."""
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
    # the answer first, from the bitmap the frame owes (the frame's own tests pin it): it sizes the buffers
    cpu_frame = nr.run(s) if n else None
    bitmap = orr.bitmap_of(~cpu_frame["coarse_culled"]) if n else np.zeros(0, np.uint32)
    occlusion = dict(pv=pv, levels=orr.pyramid_levels(TC._WALL), width=64, height=32) if wall else None
    want = ctr.cull_cluster_triangles(s, boxes, vertices, indices, bitmap, mode, sw, pv, max(n, 1) * 8, 1 << 31, first_instance_base=base, occlusion=occlusion)
    assert want["status"] == 0, what
    t = cr.cluster_table(s["meshes"])
    room = len(want["stream"]) + 3
    stage_room = int(cpu_frame["cmds"]["total"]) if n else 0
    stage = torch.full((stage_room + 3,), -1, dtype=torch.int32, device=T._dev()) if against_the_stage else None
    out = _Out(max(n, 1) * 8, room)
    if n:
        extra = dict(culled_index_buffer=stage.data_ptr(), culled_index_capacity=stage_room) if against_the_stage else {}
        p.run_device(frame, async_=True, **f.kwargs(), **extra)
    if wall:
        p.build_depth_pyramid(depth.data_ptr(), 64, 32, pyr.data_ptr(), format=_lib.MIP_DEPTH_FLOAT32, async_=True)
    p.cull_cluster_triangles(frame, f.bitmap.data_ptr(), make_lod_policy(mode, sw), out.outputs(async_=True), occlusion=occ)
    p.wait()
    assert n == 0 or np.array_equal(f.host_bitmap(), bitmap), (what, "the frame's bitmap")
    _check(out, want, what)
    if against_the_stage:
        count = int(f.scal[0].item())
        cmds = f.cmds[:count].cpu().numpy().view(np.uint32).reshape(-1).view(DRAW_CMD_DTYPE)
        theirs = stage.cpu().numpy().view(np.uint32)
        items, sv = want["items"], want["survive"]
        filtered = []
        for c in cmds:                                          # the stage's final commands: one per instance with a surviving triangle
            i = (int(c["firstInstance"]) - base) & 0xFFFFFFFF
            b = int(items["bucket"][i])
            k, l, tris = int(t["mesh"][b]), int(t["lod"][b]), int(t["T"][b])
            off = int(s["meshes"]["index_offset"][k, l])
            ix = np.asarray(indices, np.uint32)[off : off + 3 * tris].reshape(tris, 3)
            v = np.asarray(vertices, np.float32).reshape(-1, 3)[ix.astype(np.int64) + int(s["meshes"]["vertex_offset"][k])]
            model = nr.model_matrices(s["pos"][i : i + 1], s["rot"][i : i + 1], s["scale"][i : i + 1])[0]
            keep = ~nr.triangle_culled(model, pv, v)            # which triangles the stage's stream holds: it reproduces the device's bytes
            mine = theirs[int(c["firstIndex"]) : int(c["firstIndex"]) + int(c["indexCount"])]
            assert np.array_equal(ix[keep].reshape(-1), mine), (what, "the per-triangle stage's own stream", i)
            alive = np.zeros(int(t["C"][b]), bool)
            alive[items["cluster"][sv & (items["inst"] == i)]] = True
            filtered.append(ix[keep & alive[np.arange(tris) // 64]].reshape(-1))
        filtered = np.concatenate(filtered) if filtered else np.zeros(0, np.uint32)
        got = out.result()[2][: len(want["stream"])]
        assert np.array_equal(filtered, got) and len(got) > 0, (what, "the two device paths")
    return want


@pytest.mark.parametrize("ordering", ["rows", "strips", "shuffled"])
def test_built_scene_against_the_restatement_and_the_stage(ra, ordering):
    s = ra.scene.make_scene(3, n=257)
    vertices, indices = ra.scene.make_geometry(s["meshes"], ordering)
    boxes = cr.cluster_boxes(s["meshes"], vertices, indices)
    with TC._pipeline(ra, s, vertices, indices) as p:
        for wall in (False, True):
            # the pin policy picks the frame's own levels: the per-triangle stage tests the same triangles
            want = _frame_then_cull(ra, p, s, vertices, indices, boxes, lr.DISTANCE, lr.PIN_SWITCH_SQ, f"{ordering} pin wall={wall}", wall, 0,
                                    against_the_stage=True)
            if ordering == "strips" and not wall:               # the known answer (tests/test_cluster_triangle_restatement.py)
                assert want["stats"].tolist() == [71, 2581, 3127, 72, 78898, 162813] and int((want["cmds"]["indexCount"] == 0).sum()) == 5
            for mode in (lr.DISTANCE, lr.RELATIVE):
                _frame_then_cull(ra, p, s, vertices, indices, boxes, mode, TL._metric_thresholds(s, mode), f"{ordering} mode={mode} wall={wall}", wall,
                                 0xFFFFFFFF - 100)           # a base that wraps inside the scene


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_small_instance_counts(ra, n):
    ordering = "rows" if n % 2 else "shuffled"
    s = TL._sized(ra.scene.make_scene(3, n=max(n, 1)), n)
    vertices, indices = ra.scene.make_geometry(s["meshes"], ordering)
    boxes = cr.cluster_boxes(s["meshes"], vertices, indices)
    with TC._pipeline(ra, s, vertices, indices) as p:
        for wall in (False, True):
            _frame_then_cull(ra, p, s, vertices, indices, boxes, lr.DISTANCE, lr.PIN_SWITCH_SQ, f"n={n} wall={wall}", wall, 3)


def test_non_finite_instances(ra):
    """special_513's instances (tests/golden: special values in every column) over config 3's geometry: the matrix of every one of
    them is the one mip_run writes, NaN rows included."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "special_513.npz"))
    s = dict(pos=g["pos"], rot=g["rot"], scale=g["scale"], mesh_id=g["mesh_id"], meshes=g["meshes"], planes=g["planes"], cam_pos=g["cam_pos"],
             n=len(g["scale"]))
    vertices, indices = ra.scene.make_geometry(s["meshes"], "strips")
    boxes = cr.cluster_boxes(s["meshes"], vertices, indices)
    with TC._pipeline(ra, s, vertices, indices) as p:
        want = _frame_then_cull(ra, p, s, vertices, indices, boxes, lr.DISTANCE, lr.PIN_SWITCH_SQ, "special_513", False, 0)
        assert int(want["stats"][4]) > 0


# ---- 2. every hand-written scene, against the hand-written bytes ----

_CASES = ctc.cases()


@pytest.mark.parametrize("name,s,want", _CASES, ids=[c[0] for c in _CASES])
def test_hand_cases(ra, name, s, want):
    with TC._pipeline(ra, s, s["vertices"], s["indices"]) as p:
        _cull_given(p, s, want, name, ctc.PV)
        _cull_given(p, s, want, name + ", asynchronous", ctc.PV, async_=True)


# ---- 3. structural edges, read from the plan ----

def _plan_sizes(tmp):
    exe = os.path.join(str(tmp), "cluster_triangle_plan_sizes")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "native", "cluster_triangle_plan_check.cpp"), "-o", exe])
    return json.loads(subprocess.check_output([exe, "sizes"]))


def _single_triangles(n, base):
    """n instances of ONE mesh of one triangle (a one-triangle cluster each: W = n); every fifth instance stands outside the
    frustum. Under PV_MIRROR the triangle of a surviving instance survives. Returns (scene, want), want written from the pattern."""
    meshes = np.zeros(1, MESH_DTYPE)
    meshes["aabb_min"][0], meshes["aabb_max"][0], meshes["n_lods"][0], meshes["index_len"][0, 0] = (0, 0, 0), (1, 1, 0), 1, 3
    pos = np.zeros((n, 3), np.float32)
    alive = np.arange(n) % 5 != 0
    pos[~alive, 0] = 2000.0
    rot = np.zeros((n, 4), np.float32)
    rot[:, 3] = 1.0
    s = dict(n=n, meshes=meshes, vertices=np.array(cc.BASE_VERTICES, np.float32), indices=np.array(cc.IN, np.uint32), pos=pos, rot=rot,
             scale=np.ones(n, np.float32), mesh_id=np.zeros(n, np.uint32), planes=cc.PLANES, cam_pos=cc.CAM, base=base,
             bitmap=np.full((n + 31) // 32, 0xFFFFFFFF, np.uint32), work_capacity=n)
    who = np.nonzero(alive)[0]
    cmds = np.zeros(len(who), DRAW_CMD_DTYPE)
    cmds["indexCount"], cmds["instanceCount"], cmds["firstIndex"] = 3, 1, 3 * np.arange(len(who))
    cmds["firstInstance"] = ((who + base) & 0xFFFFFFFF).astype(np.uint32)
    k = len(who)
    return s, dict(cmds=cmds, stats=np.array([k, k, n, n, k, k], np.uint32), stream=np.tile(np.array(cc.IN, np.uint32), k))


EDGE_PARTS = ("tiles", "lanes", "grid cap")


def _edge_scenes(sizes, part):
    """[(name, scene, want)] of one part, all under PV_MIRROR. "tiles": test_gpu_clusters' ladders whose work items and heads fall
    one below, at and one above 64, the item tile and the head tile. "lanes": survivors on lane 0, lane 63 and across the words
    63 | 64; an all-zero survive word between two full ones. "grid cap": W — and the call's bound — one below, at and one above
    the size from which the test and write kernels' grids loop, read from the plan."""
    if part == "tiles":
        return [(name, s, ctc.ladder_want(s, want)) for name, s, want in TC._edge_scenes(sizes, "tiles")]
    if part == "lanes":
        out = []
        for name, patterns, inst in (("lanes 0, 63 | 64", ["1" + "0" * 62 + "11" + "0" * 65], [0]),
                                     ("a zero word between two full ones", ["1" * 64 + "0" * 64 + "1" * 64], [0]),
                                     ("a zero word of whole instances", ["1" * 64, "0" * 32], [0, 1, 1, 0])):
            s, want = cc.ladder_scene(patterns, inst, base=8)
            out.append((name, s, ctc.ladder_want(s, want)))
        return out
    assert sizes["test_grid_cap"] == sizes["write_grid_cap"]
    cap = sizes["test_grid_cap"]
    return [(f"W = bound = {w}", *_single_triangles(w, base=7)) for w in (cap - 1, cap, cap + 1)]


def _run_edge_scenes(ra, scenes):
    for name, s, want in scenes:
        with TC._pipeline(ra, s, s["vertices"], s["indices"]) as p:
            _cull_given(p, s, want, name, ctc.PV_MIRROR, work_capacity=s.get("work_capacity", 0), async_=True)


@pytest.mark.parametrize("part", EDGE_PARTS)
def test_structural_edges(ra, tmp_path, part):
    sizes = _plan_sizes(tmp_path)
    scenes = _edge_scenes(sizes, part)
    if part == "tiles":
        for edge in (64, sizes["item_tile"], sizes["head_tile"]):
            assert {int(w["stats"][0]) for _, _, w in scenes} >= {edge - 1, edge, edge + 1}       # heads on every edge
            assert {int(w["stats"][2]) for _, _, w in scenes} >= {edge - 1, edge, edge + 1}       # work items on every edge
    elif part == "grid cap":
        cap = sizes["max_blocks"] * sizes["item_tile"]
        assert [int(w["stats"][2]) for _, _, w in scenes] == [cap - 1, cap, cap + 1]
    _run_edge_scenes(ra, scenes)


_EDGE_CHILD = r'''
import os, sys
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
os.environ["MIP_LIBRARY"] = os.path.join(root, "renderer_amd", "lib", "libmi_instance_pipeline_dbg.so")
import renderer_amd
import test_gpu_cluster_triangles as TT
TT._run_edge_scenes(renderer_amd, TT._edge_scenes(TT._plan_sizes(sys.argv[2]), sys.argv[3]))
print("CLUSTER-TRIANGLE-EDGES-OK")
'''


@pytest.mark.parametrize("part", EDGE_PARTS)
@pytest.mark.parametrize("tiles", ["reverse", "scramble"])
def test_structural_edges_in_any_dispatch_order(tiles, part, tmp_path):
    e = dict(os.environ, MIP_DEBUG_TILE_ORDER=tiles)
    out = subprocess.run([sys.executable, "-c", _EDGE_CHILD, ROOT, str(tmp_path), part], capture_output=True, text=True, timeout=600, env=e)
    assert out.returncode == 0 and "CLUSTER-TRIANGLE-EDGES-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ---- 4. overflow ----

@pytest.mark.parametrize("frames_in_flight", [1, 2])
def test_overflow_rules(ra, frames_in_flight):
    s = ra.scene.make_scene(3, n=257)
    vertices, indices = ra.scene.make_geometry(s["meshes"], "strips")
    boxes = cr.cluster_boxes(s["meshes"], vertices, indices)
    policy = make_lod_policy(lr.DISTANCE, lr.PIN_SWITCH_SQ)
    pv = ra.scene.default_pv()
    with TC._pipeline(ra, s, vertices, indices, frames_in_flight=frames_in_flight) as p:
        f = T._Frame(257)
        frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=17, pv=pv)
        p.run_device(frame, **f.kwargs())
        full = ctr.cull_cluster_triangles(s, boxes, vertices, indices, f.host_bitmap(), lr.DISTANCE, lr.PIN_SWITCH_SQ, pv, 1 << 20, 1 << 30, first_instance_base=17)
        heads, w, members, total = int(full["stats"][0]), int(full["stats"][2]), int(full["stats"][3]), 3 * int(full["stats"][4])
        assert heads > 2 and w > heads and total == len(full["stream"]) > 3
        refused = dict(full, stats=[0, 0, w, members, 0, 0])

        def cull(out, async_=False, **kw):
            if frames_in_flight > 1:   # behind a frame of its own: consecutive calls go to different slots
                p.run_device(frame, async_=True, **f.kwargs())
            p.cull_cluster_triangles(frame, f.bitmap.data_ptr(), policy, out.outputs(async_=async_, **kw))

        def overflows(out, async_, **kw):
            """MIP_ERR_CAPACITY once: from the call, or from mip_wait for an asynchronous one; then the context is clean again."""
            with pytest.raises(ra.MipError) as e:
                cull(out, async_, **kw)
                p.wait()
            assert e.value.code == CAPACITY
            p.wait()

        for async_ in (False, True):
            for cap in (total - 3, 0):          # the index overflow: a zero count, the true six stats, no command and no index
                out = _Out(heads, total)
                overflows(out, async_, index_capacity=cap)
                _check(out, full, f"index_capacity {cap} async={async_}", count=0, written=False)
            out = _Out(heads, total)            # exactly enough room
            cull(out, async_, index_capacity=total, cmd_capacity=heads, work_capacity=w)
            p.wait()
            _check(out, full, f"index_capacity = total async={async_}")
            for cap in (heads - 1, 0):          # the command overflow: the first `cap` commands exactly, the stream complete
                out = _Out(heads, total)
                overflows(out, async_, cmd_capacity=cap)
                _check(out, full, f"cmd_capacity {cap} async={async_}", count=cap)
            out = _Out(heads, total)            # W - 1: nothing but the zero count and the refusal's stats
            overflows(out, async_, work_capacity=w - 1)
            _check(out, refused, f"work_capacity W - 1 async={async_}", count=0, written=False)
            out = _Out(heads, total)            # a fitting call on the same context is complete
            cull(out, async_)
            p.wait()
            _check(out, full, f"fitting call async={async_}")


# ---- 5. every refusal writes nothing and leaves the context usable ----

def test_refusals_write_nothing(ra):
    name, s, want = _CASES[0]
    with TC._pipeline(ra, s, s["vertices"], s["indices"]) as p:
        lib, ctx = p._lib, p._ctx
        bm = TC._device_bitmap(s["bitmap"])
        out = _Out(4, 64)
        frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=s["base"], pv=ctc.PV)
        policy = make_lod_policy(lr.DISTANCE, cc.PIN)
        import torch
        pyr = torch.zeros(64, dtype=torch.float32, device=T._dev())
        torch.cuda.synchronize()

        def call(frame=frame, bitmap=bm.data_ptr(), policy=policy, occ=None, o=None, null_out=False):
            o = o if o is not None else out.outputs()
            return lib.mip_cull_cluster_triangles(ctx, C.addressof(frame) if frame is not None else None, bitmap,
                                                  C.addressof(policy) if policy is not None else None,
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
            ("NULL culled_indices", call(o=outputs(culled_indices=None))), ("misaligned culled_indices", call(o=outputs(culled_indices=out.stream.data_ptr() + 2))),
            ("struct_size", call(o=outputs(struct_size=40))), ("struct_size + 4", call(o=outputs(struct_size=60))),
            ("NULL frame", call(frame=None)), ("NULL bitmap", call(bitmap=None)), ("NULL policy", call(policy=None)), ("NULL out", call(null_out=True)),
            ("NULL cluster_cmds", call(o=outputs(cluster_cmds=None))), ("NULL cmd_count", call(o=outputs(cmd_count=None))),
            ("unknown flags", call(o=outputs(flags=_lib.MIP_OUT_DEVICE | 0x10))),
            ("host outputs", call(o=outputs(flags=0))), ("misaligned", call(o=outputs(cmd_count=out.scal.data_ptr() + 2))),
            ("misaligned stats", call(o=outputs(stats=out.scal.data_ptr() + 9))),
            ("decreasing thresholds", call(policy=bad_policy)), ("policy struct_size", call(policy=wrong_size)),
            ("occlusion struct_size", call(occ=occlusion(struct_size=100))), ("occlusion flags", call(occ=occlusion(flags=1))),
            ("candidates", call(occ=occlusion(candidates=bm.data_ptr()))), ("occluded_bitmap", call(occ=occlusion(occluded_bitmap=bm.data_ptr()))),
            ("NULL pyramid", call(occ=occlusion(pyramid=None))), ("extent", call(occ=occlusion(width=0))),
            ("extent above the limit", call(occ=occlusion(height=_lib.MIP_MAX_DEPTH_EXTENT + 1))),
        ]
        for what, rc in refused:
            assert rc == INVALID, (what, rc)
        good = out.outputs()
        assert lib.mip_cull_cluster_triangles(None, C.addressof(frame), bm.data_ptr(), C.addressof(policy), None, C.addressof(good)) == INVALID
        assert out.untouched()
        _cull_given(p, s, want, name + " after the refusals", ctc.PV)     # the context is usable
        # a stale table: not ready, nothing written
        p.set_geometry(s["vertices"], s["indices"])
        fresh = _Out(4, 64)
        with pytest.raises(ra.MipError) as e:
            p.cull_cluster_triangles(frame, bm.data_ptr(), policy, fresh.outputs())
        assert e.value.code == NOT_READY and fresh.untouched()
    # no instances: not ready
    with ra.InstancePipeline(max_instances=4, max_meshes=len(s["meshes"])) as p:
        p.set_mesh_table(s["meshes"])
        p.set_geometry(s["vertices"], s["indices"])
        p.build_clusters()
        fresh = _Out(4, 64)
        with pytest.raises(ra.MipError) as e:
            p.cull_cluster_triangles(make_frame(s["planes"], s["cam_pos"], pv=ctc.PV), bm.data_ptr(), policy, fresh.outputs())
        assert e.value.code == NOT_READY and fresh.untouched()
