"""mip_list_clusters on the GPU (include/mi_instance_pipeline.h): every byte of the entries, the count, the draw arguments and
the stats against the numpy restatement (tests/cluster_list_restatement.py), against the hand-written lists
(tests/cluster_list_cases.py) and against the expansion of what mip_cull_clusters / mip_cull_clusters_cone just wrote on the
same context; the structural edges of the launch plan (renderer_amd/csrc/cluster_list_plan.hpp), also with reversed and
scrambled tiles under the diagnostic library; both overflow rules; every refusal. Every output buffer is filled with a sentinel
and compared whole. Not reference behaviour: parity is with the restatement."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_cases as cc
import cluster_cone_restatement as ccr
import cluster_list_cases as clc
import cluster_list_restatement as clr
import cluster_restatement as cr
import lod_restatement as lr
import occlusion_restatement as orr
import test_gpu_batch as T
import test_gpu_batch_lods as TL
import test_gpu_clusters as TC
from renderer_amd import _lib
from renderer_amd.pipeline import DRAW_CMD_DTYPE, make_cluster_cone, make_cluster_list_outputs, make_frame, make_lod_policy, make_occlusion

pytestmark = pytest.mark.gpu
ROOT = TC.ROOT
SENTINEL = T.SENTINEL
ra = T.ra   # the module's library fixture
NOT_READY, INVALID, CAPACITY = -6, -1, -4


class _Out:
    """Device outputs of mip_list_clusters, filled with a sentinel: room for `cap` entries + 3 rows nobody may touch;
    scal[0] = entry_count, scal[2:6] = draw_args, scal[6:9] = stats."""

    def __init__(self, cap, args=True, stats=True):
        import torch

        fill = T._i32(SENTINEL)
        self.cap, self.args, self.stats = int(cap), args, stats
        self.entries = torch.full((self.cap + 3, 4), fill, dtype=torch.int32, device=T._dev())
        self.scal = torch.full((12,), fill, dtype=torch.int32, device=T._dev())
        torch.cuda.synchronize()

    def outputs(self, entry_capacity=None, work_capacity=0, async_=False):
        return make_cluster_list_outputs(self.entries.data_ptr(), self.cap if entry_capacity is None else entry_capacity, self.scal.data_ptr(),
                                         self.scal.data_ptr() + 8 if self.args else 0, self.scal.data_ptr() + 24 if self.stats else 0,
                                         work_capacity=work_capacity, async_=async_)

    def scalars(self):
        import torch

        torch.cuda.synchronize()
        return self.scal.cpu().numpy().view(np.uint32)

    def result(self):
        scal = self.scalars()
        return self.entries.cpu().numpy().view(np.uint32), scal

    def untouched(self):
        entries, scal = self.result()
        return (entries == SENTINEL).all() and (scal == SENTINEL).all()


def _check_scalars(out, count, want_stats, what):
    scal = out.scalars()
    assert int(scal[0]) == count, (what, "entry_count", int(scal[0]), count)
    if out.args:
        assert scal[2:6].tolist() == [192, count, 0, 0], (what, "draw_args", scal[2:6].tolist())
    else:
        assert (scal[2:6] == SENTINEL).all(), what
    if out.stats:
        assert scal[6:9].tolist() == [int(v) for v in want_stats], (what, "stats", scal[6:9].tolist(), list(want_stats))
    else:
        assert (scal[6:9] == SENTINEL).all(), what
    assert scal[1] == SENTINEL and (scal[9:] == SENTINEL).all(), what


def _check(out, want_entries, want_stats, what, count=None):
    """The first `count` entries are want_entries' (all of them unless a capacity cut the list), nothing else was written."""
    count = len(want_entries) if count is None else count
    _check_scalars(out, count, want_stats, what)
    entries, _ = out.result()
    assert entries[:count].tobytes() == np.ascontiguousarray(want_entries[:count]).tobytes(), (what, "entries")
    assert (entries[count:] == SENTINEL).all(), (what, "entries at or behind entry_count were written")


def _list_given(p, s, want, what, entry_capacity=None, work_capacity=0, async_=False, args=True, stats=True):
    """mip_list_clusters over the scene's own bitmap (uploaded) under the pin policy; the outputs against `want`."""
    bm = TC._device_bitmap(s["bitmap"])
    out = _Out(len(want["entries"]) if entry_capacity is None else entry_capacity, args, stats)
    frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=s["base"])
    p.list_clusters(frame, bm.data_ptr(), make_lod_policy(lr.DISTANCE, cc.PIN), out.outputs(entry_capacity, work_capacity, async_))
    if async_:
        p.wait()
    _check(out, want["entries"], want["stats"], what)
    return out


def _commands_then_expanded(p, frame, bitmap_ptr, policy, room, occ=None, cone=None):
    """What mip_cull_clusters / mip_cull_clusters_cone write on this context for the same arguments, expanded into entries."""
    cmds = TC._Out(room)
    if cone is None:
        p.cull_clusters(frame, bitmap_ptr, policy, cmds.outputs(), occlusion=occ)
    else:
        p.cull_clusters_cone(frame, bitmap_ptr, policy, cone, cmds.outputs(), occlusion=occ)
    rows, scal = cmds.result()
    return clr.from_commands(np.ascontiguousarray(rows[: int(scal[0])]).view(DRAW_CMD_DTYPE).reshape(-1), None), scal[2:6]


# ---- 1. every hand-written scene, against the hand-written bytes and against mip_cull_clusters on the same context ----

_CASES = clc.cases()


@pytest.mark.parametrize("name,s,want", _CASES, ids=[c[0] for c in _CASES])
def test_hand_cases(ra, name, s, want):
    with TC._pipeline(ra, s, s["vertices"], s["indices"]) as p:
        _list_given(p, s, want, name)
        _list_given(p, s, want, name + ", asynchronous", async_=True)
        _list_given(p, s, want, name + ", no draw_args", args=False)
        _list_given(p, s, want, name + ", no stats", stats=False, async_=True)
        frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=s["base"])
        bm = TC._device_bitmap(s["bitmap"])
        expanded, stats = _commands_then_expanded(p, frame, bm.data_ptr(), make_lod_policy(lr.DISTANCE, cc.PIN), len(want["entries"]) + 1)
        assert expanded.tobytes() == want["entries"].tobytes() and stats[1:].tolist() == want["stats"].tolist()


# ---- 2. the restatement over the repository's scenes ----

def _frame_then_list(ra, p, s, boxes, mode, sw, what, full_bitmap, wall, base, cone=None, cones=None):
    """mip_run, (the pyramid build,) mip_list_clusters over the frame's bitmap with no wait in between — or over a full bitmap
    uploaded first; every byte against the restatement, and against the expansion of the command call on the same context."""
    import torch

    n = s["n"]
    pv = ra.scene.default_pv()
    f = T._Frame(n)
    frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=base)
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
    p.list_clusters(frame, bitmap_ptr, policy, out.outputs(async_=True), occlusion=occ, cone=cone)
    p.wait()
    bitmap = np.full((n + 31) // 32, 0xFFFFFFFF, np.uint32) if full_bitmap else f.host_bitmap()
    occlusion = dict(pv=pv, levels=orr.pyramid_levels(TC._WALL), width=64, height=32) if wall else None
    k = dict(cones=cones, eye=np.array(cone.eye[:], np.float32), facing=float(cone.facing)) if cone is not None else None
    want = clr.list_clusters(s, boxes, bitmap, mode, sw, cap, first_instance_base=base, occlusion=occlusion, cone=k)
    assert want["status"] == 0, what
    _check(out, want["entries"], want["stats"], what)
    if n:
        expanded, stats = _commands_then_expanded(p, frame, bitmap_ptr, policy, cap, occ, cone)
        assert expanded.tobytes() == want["entries"].tobytes() and stats[1:].tolist() == want["stats"].tolist(), (what, "the command call's expansion")
    return want


@pytest.mark.parametrize("n", [0, 1, 257, 4097])
def test_restatement_over_config_3(ra, n):
    ordering = "strips" if n == 257 else "rows" if n % 2 else "shuffled"
    s = TL._sized(ra.scene.make_scene(3, n=max(n, 1)), n)
    vertices, indices = ra.scene.make_geometry(s["meshes"], ordering)
    boxes = cr.cluster_boxes(s["meshes"], vertices, indices)
    walled = free = None
    with TC._pipeline(ra, s, vertices, indices) as p:
        for mode in (lr.DISTANCE, lr.RELATIVE):
            sw = TL._metric_thresholds(s, mode)
            for full_bitmap, wall in ((False, False), (True, True)) if n > 257 and mode == lr.RELATIVE else ((False, False), (False, True), (True, False), (True, True)):
                base = (0xFFFFFFFF - n // 2) if full_bitmap else 3      # a base that wraps inside the scene
                want = _frame_then_list(ra, p, s, boxes, mode, sw, f"n={n} {ordering} mode={mode} full={full_bitmap} wall={wall}", full_bitmap, wall, base)
                if full_bitmap and mode == lr.DISTANCE:
                    walled, free = (want, free) if wall else (walled, want)
        if n == 257:   # the known answer (tests/test_cluster_list_restatement.py): the pin policy, the frame's bitmap
            want = _frame_then_list(ra, p, s, boxes, lr.DISTANCE, lr.PIN_SWITCH_SQ, "n=257 strips pin", False, False, 0)
            assert want["stats"].tolist() == [2581, 3127, 72]
    if n >= 257:   # the wall removes clusters, and only removes
        assert 0 < int(walled["stats"][0]) < int(free["stats"][0])


def test_with_the_cone_under_patches(ra):
    s = ra.scene.make_scene(3, n=257)
    vertices, indices = ra.scene.make_geometry(s["meshes"], "patches")
    boxes = cr.cluster_boxes(s["meshes"], vertices, indices)
    cones = ccr.cluster_cones(s["meshes"], vertices, indices, boxes)
    cone = make_cluster_cone(ra.scene.default_pv())
    with TC._pipeline(ra, s, vertices, indices) as p:
        p.build_cluster_cones()
        want = _frame_then_list(ra, p, s, boxes, lr.DISTANCE, lr.PIN_SWITCH_SQ, "patches, cone, pin", False, False, 0, cone, cones)
        assert want["stats"].tolist() == [1971, 3127, 72]
        plain = _frame_then_list(ra, p, s, boxes, lr.DISTANCE, lr.PIN_SWITCH_SQ, "patches, no cone", False, False, 0)
        assert int(plain["stats"][0]) > 1971
        sw = TL._metric_thresholds(s, lr.RELATIVE)
        _frame_then_list(ra, p, s, boxes, lr.RELATIVE, sw, "patches, cone, wall, full bitmap", True, True, 0xFFFFFFF0, cone, cones)


def test_non_finite_instances_take_the_literal_chain(ra):
    g = np.load(os.path.join(ROOT, "tests", "golden", "special_513.npz"))
    s = dict(pos=g["pos"], rot=g["rot"], scale=g["scale"], mesh_id=g["mesh_id"], meshes=g["meshes"], planes=g["planes"], cam_pos=g["cam_pos"],
             n=len(g["scale"]))
    vertices, indices = ra.scene.make_geometry(s["meshes"], "strips")
    boxes = cr.cluster_boxes(s["meshes"], vertices, indices)
    with TC._pipeline(ra, s, vertices, indices) as p:
        for wall in (False, True):
            want = _frame_then_list(ra, p, s, boxes, lr.DISTANCE, lr.PIN_SWITCH_SQ, f"special_513 wall={wall}", True, wall, 0)
            assert int(want["stats"][1]) > 0


# ---- 3. structural edges, read from the plan ----

def _plan_sizes(tmp):
    exe = os.path.join(str(tmp), "cluster_list_plan_sizes")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "native", "cluster_list_plan_check.cpp"), "-o", exe])
    return json.loads(subprocess.check_output([exe, "sizes"]))


EDGE_PARTS = ("tiles", "members", "write grid cap", "word grid cap")


def _ladder(patterns, instance_pattern, base=0, bits=None):
    """(scene, want) of a ladder: cluster_cases' scene, cluster_list_cases' closed form."""
    s, _ = cc.ladder_scene(patterns, instance_pattern, base=base, bits=bits)
    entries, stats = clc.ladder_want(patterns, instance_pattern, base=base, bits=bits)
    return s, dict(entries=entries, stats=stats)


def _filled(w, clusters, pattern_of, base):
    """W = w work items: instances of `clusters` clusters and one shorter one. pattern_of(k): the ladder of k clusters."""
    whole, rest = divmod(w, clusters)
    return _ladder([pattern_of(clusters)] + ([pattern_of(rest)] if rest else []), [0] * whole + ([1] if rest else []), base=base)


def _edge_scenes(sizes, part):
    """[(name, scene, want)] of the parts that are compared on the host. "tiles": ladders whose work items, and ladders whose
    SURVIVORS, fall one below, at and one above 64 (a survive word), the item tile and the list tile, all-survive and
    alternating. "members": members whose first item is at 64 k - 1 / 64 k / 64 k + 1, instances of C = 1, 64, 65, 129 across
    words and tiles, 64 members in one word, members only in the last instance tile."""
    item, tile = sizes["item_tile"], sizes["list_tile"]
    out = []
    if part == "tiles":
        for edge in (64, item, tile):
            for w in (edge - 1, edge, edge + 1):
                out.append((f"W={w} whole", *_filled(w, 8, lambda k: "1" * k, base=1)))
                out.append((f"W={w} alternating", *_filled(w, 8, lambda k: ("10" * 4)[:k], base=2)))
            for n in (edge - 1, edge, edge + 1):
                s, want = _filled(2 * n, 8, lambda k: ("10" * 4)[:k], base=10)      # n survivors in 2 n work items
                assert int(want["stats"][0]) == n and int(want["stats"][1]) == 2 * n
                out.append((f"survivors={n} in {2 * n} items", s, want))
                s, want = _ladder(["1"], [0] * n, base=0xFFFFFFFF - 5)              # n survivors, one cluster each; the base wraps
                assert int(want["stats"][0]) == n == int(want["stats"][1])
                out.append((f"survivors={n}, one cluster each", s, want))
        # survivors only in the last word of the third list tile, and only in the first word of the second
        lone = np.zeros(3 * tile, bool)
        lone[-3:] = True
        lone[tile: tile + 2] = True
        out.append(("lone survivors at tile edges", *_ladder([lone], [0], base=4)))
        return out
    # first items at 64 k - 1, 64 k, 64 k + 1 (63, 64, 193, 255 ...), C = 1, 64, 65, 129, every second cluster survives
    alt = lambda k: ("10" * k)[:k]   # noqa: E731
    out.append(("first items around word edges", *_ladder([alt(63), alt(1), alt(64), alt(65), alt(62), alt(3), alt(129)], [0, 1, 2, 3, 4, 5, 5, 6, 6, 3, 2, 6], base=1)))
    out.append(("first items around word edges, all survive", *_ladder(["1" * 63, "1", "1" * 64, "1" * 65, "1" * 62, "111", "1" * 129],
                                                                       [0, 1, 2, 3, 4, 5, 5, 6, 6, 3, 2, 6], base=1)))
    # a member that starts one item before / at / behind a LIST tile's edge
    for d in (-1, 0, 1):
        out.append((f"a member at the list tile's edge {d:+d}", *_ladder(["1" * (tile + d), alt(129), "1"], [0, 1, 2, 1], base=2)))
    # 64 members in every word (C = 1), 200 of them: the window of 64 entries holds the word's last member and no more
    out.append(("64 members in a word", *_ladder(["1"], [0] * 200, base=3)))
    # instances of C = 129 over words and item tiles, the first and last cluster culled
    out.append(("C = 129", *_ladder(["0" + "1" * 127 + "0"], [0] * 40, base=5)))
    # members only in the last instance tile (and only its last instance)
    n = 2 * sizes["instance_tile"] + 1
    bits = np.zeros(n, bool)
    bits[-1] = True
    out.append(("members in the last tile", *_ladder(["1101"], [0] * n, base=6, bits=bits)))
    return out


def _uniform_on_device(n_whole, clusters, lo, hi, rest, base):
    """The closed form of a ladder's list as a device tensor: n_whole instances of mesh 0 (`clusters` clusters, [lo, hi) of them
    survive) and, with rest > 0, one instance of mesh 1 (`rest` clusters, all survive)."""
    import torch

    per = hi - lo
    e = torch.arange(n_whole * per + rest, dtype=torch.int64, device=T._dev())
    whole = e < n_whole * per
    inst = torch.where(whole, e // per, torch.full_like(e, n_whole))
    c = torch.where(whole, lo + e % per, e - n_whole * per)
    want = torch.zeros((len(e), 4), dtype=torch.int64, device=T._dev())
    want[:, 0] = (inst + base) & 0xFFFFFFFF
    want[:, 1] = 192 * c + torch.where(whole, torch.zeros_like(e), torch.full_like(e, 192 * clusters))
    want[:, 3] = 192
    return want.to(torch.int32)


def _cap_scenes(sizes, part):
    """[(name, scene, work_capacity, closed form)]: W — and the call's bound on it, work_capacity = W — one below, at and one
    above the size at which the plan stops growing a looping grid (max_blocks tiles), and two tiles past it under the
    library's own bound with the first and last cluster of every instance culled."""
    step = sizes["item_tile"] if part == "write grid cap" else sizes["list_tile"]
    cap = sizes["max_blocks"] * step
    out = []
    for w in (cap - 1, cap, cap + 1):
        whole, rest = divmod(w, 128)
        s, _ = cc.ladder_scene(["1" * 128] + (["1" * rest] if rest else []), [0] * whole + ([1] if rest else []), base=7)
        out.append((f"{part}: W = bound = {w}", s, w, (whole, 128, 0, 128, rest, 7), [w, w, whole + (1 if rest else 0)]))
    n = (cap + 2 * step) // 128
    s, _ = cc.ladder_scene(["0" + "1" * 126 + "0"], [0] * n, base=3)
    out.append((f"{part}: loops", s, 0, (n, 128, 1, 127, 0, 3), [126 * n, 128 * n, n]))
    return out


def _run_edge_scenes(ra, scenes):
    for name, s, want in scenes:
        with TC._pipeline(ra, s, s["vertices"], s["indices"]) as p:
            _list_given(p, s, want, name, entry_capacity=len(want["entries"]) + 2, async_=True)


def _run_cap_scenes(ra, scenes):
    import torch

    for name, s, work_capacity, form, stats in scenes:
        want = _uniform_on_device(*form)
        assert len(want) == stats[0]
        with TC._pipeline(ra, s, s["vertices"], s["indices"]) as p:
            bm = TC._device_bitmap(s["bitmap"])
            out = _Out(len(want))
            frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=s["base"])
            p.list_clusters(frame, bm.data_ptr(), make_lod_policy(lr.DISTANCE, cc.PIN), out.outputs(work_capacity=work_capacity, async_=True))
            p.wait()
            _check_scalars(out, len(want), stats, name)
            assert torch.equal(out.entries[: len(want)], want), (name, "entries")
            assert bool((out.entries[len(want):] == T._i32(SENTINEL)).all()), (name, "entries behind entry_count were written")
        del out, want


def _run_part(ra, sizes, part):
    if part in ("tiles", "members"):
        _run_edge_scenes(ra, _edge_scenes(sizes, part))
    else:
        _run_cap_scenes(ra, _cap_scenes(sizes, part))


@pytest.mark.parametrize("part", EDGE_PARTS)
def test_structural_edges(ra, tmp_path, part):
    sizes = _plan_sizes(tmp_path)
    if part == "tiles":
        wants = [want for _, _, want in _edge_scenes(sizes, part)]
        for edge in (64, sizes["item_tile"], sizes["list_tile"]):
            assert {int(w["stats"][0]) for w in wants} >= {edge - 1, edge, edge + 1}       # survivors on every edge
            assert {int(w["stats"][1]) for w in wants} >= {edge - 1, edge, edge + 1}       # work items on every edge
    elif part != "members":
        step = sizes["item_tile"] if part == "write grid cap" else sizes["list_tile"]
        cap = sizes["max_blocks"] * step
        scenes = _cap_scenes(sizes, part)
        assert [c[4][1] for c in scenes[:3]] == [cap - 1, cap, cap + 1] and scenes[3][4][1] > cap + step
    _run_part(ra, sizes, part)


_SCENE_PARTS = ("catalogue", "config 3", "cone and special_513")
_EDGE_CHILD = r'''
import os, sys
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
os.environ["MIP_LIBRARY"] = os.path.join(root, "renderer_amd", "lib", "libmi_instance_pipeline_dbg.so")
import renderer_amd
import test_gpu_cluster_list as TLST
if sys.argv[3] in TLST.EDGE_PARTS:
    TLST._run_part(renderer_amd, TLST._plan_sizes(sys.argv[2]), sys.argv[3])
else:
    TLST._run_scenes(renderer_amd, sys.argv[3])
print("CLUSTER-LIST-EDGES-OK")
'''


def _run_scenes(ra, part):
    """The bodies of the tests of sections 1 and 2, whole, on the library `ra` loads: for the run under the diagnostic library."""
    if part == "catalogue":
        for name, s, want in _CASES:
            test_hand_cases(ra, name, s, want)
    elif part == "config 3":
        for n in (0, 1, 257, 4097):
            test_restatement_over_config_3(ra, n)
    else:
        test_with_the_cone_under_patches(ra)
        test_non_finite_instances_take_the_literal_chain(ra)


@pytest.mark.parametrize("part", EDGE_PARTS + _SCENE_PARTS)
@pytest.mark.parametrize("tiles", ["reverse", "scramble"])
def test_everything_in_any_dispatch_order(tiles, part, tmp_path):
    e = dict(os.environ, MIP_DEBUG_TILE_ORDER=tiles)
    out = subprocess.run([sys.executable, "-c", _EDGE_CHILD, ROOT, str(tmp_path), part], capture_output=True, text=True, timeout=600, env=e)
    assert out.returncode == 0 and "CLUSTER-LIST-EDGES-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ---- 4. overflow ----

@pytest.mark.parametrize("frames_in_flight", [1, 2])
def test_overflow_rules(ra, frames_in_flight):
    s = ra.scene.make_scene(3, n=257)
    vertices, indices = ra.scene.make_geometry(s["meshes"], "strips")
    boxes = cr.cluster_boxes(s["meshes"], vertices, indices)
    policy = make_lod_policy(lr.DISTANCE, lr.PIN_SWITCH_SQ)
    with TC._pipeline(ra, s, vertices, indices, frames_in_flight=frames_in_flight) as p:
        f = T._Frame(257)
        frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=17)
        p.run_device(frame, **f.kwargs())
        full = clr.list_clusters(s, boxes, f.host_bitmap(), lr.DISTANCE, lr.PIN_SWITCH_SQ, 1 << 20, first_instance_base=17)
        survivors, w, members = (int(v) for v in full["stats"])
        assert (survivors, w, members) == (2581, 3127, 72)

        def call(out, async_=False, **kw):
            if frames_in_flight > 1:   # behind a frame of its own: consecutive calls go to different slots
                p.run_device(frame, async_=True, **f.kwargs())
            p.list_clusters(frame, f.bitmap.data_ptr(), policy, out.outputs(async_=async_, **kw))

        def overflows(out, async_, **kw):
            """MIP_ERR_CAPACITY once: from the call, or from mip_wait for an asynchronous one; then the context is clean again."""
            with pytest.raises(ra.MipError) as e:
                call(out, async_, **kw)
                p.wait()
            assert e.value.code == CAPACITY
            p.wait()

        for async_ in (False, True):
            for cap in (survivors - 1, 0):      # the first `cap` entries exactly, the true stats, MIP_ERR_CAPACITY
                out = _Out(survivors)
                overflows(out, async_, entry_capacity=cap)
                _check(out, full["entries"], full["stats"], f"entry_capacity {cap} async={async_}", count=cap)
            out = _Out(survivors)               # W - 1: nothing but the zero count, {192, 0, 0, 0} and the refusal's stats
            overflows(out, async_, work_capacity=w - 1)
            _check(out, full["entries"], [0, w, members], f"work_capacity W - 1 async={async_}", count=0)
            out = _Out(survivors)               # a fitting call on the same context is complete
            call(out, async_, entry_capacity=survivors, work_capacity=w)
            p.wait()
            _check(out, full["entries"], full["stats"], f"fitting call async={async_}")
        if frames_in_flight > 1:
            # two calls in flight behind two frames, the first one overflows: mip_wait reports it, the second is complete
            a, b = _Out(survivors), _Out(survivors)
            call(a, True, entry_capacity=1)
            call(b, True)
            with pytest.raises(ra.MipError) as e:
                p.wait()
            assert e.value.code == CAPACITY
            _check(a, full["entries"], full["stats"], "in flight, cut", count=1)
            _check(b, full["entries"], full["stats"], "in flight, whole")
            p.wait()
            # an asynchronous call overflows; a synchronous call that fits, made before any mip_wait, is NOT charged with it
            for same_slot in (False, True):
                a, b = _Out(survivors), _Out(survivors)
                call(a, True, entry_capacity=1)
                if same_slot:
                    p.list_clusters(frame, f.bitmap.data_ptr(), policy, b.outputs())
                else:
                    call(b, False)
                _check(b, full["entries"], full["stats"], f"a fitting synchronous call behind an overflow, same slot: {same_slot}")
                with pytest.raises(ra.MipError) as e:
                    p.wait()
                assert e.value.code == CAPACITY
                _check(a, full["entries"], full["stats"], "the overflow behind it", count=1)
                p.wait()


# ---- 5. every refusal writes nothing and leaves the context usable ----

def test_refusals_write_nothing(ra):
    name, s, want = _CASES[0]
    with TC._pipeline(ra, s, s["vertices"], s["indices"]) as p:
        lib, ctx = p._lib, p._ctx
        bm = TC._device_bitmap(s["bitmap"])
        out = _Out(4)
        frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=s["base"])
        policy = make_lod_policy(lr.DISTANCE, cc.PIN)
        good_cone = make_cluster_cone(eye=(0, 0, 9), facing=1)
        import torch
        pyr = torch.zeros(64, dtype=torch.float32, device=T._dev())
        torch.cuda.synchronize()

        def call(frame=frame, bitmap=bm.data_ptr(), policy=policy, occ=None, cone=None, o=None, null_out=False):
            o = o if o is not None else out.outputs()
            return lib.mip_list_clusters(ctx, C.addressof(frame) if frame is not None else None, bitmap, C.addressof(policy) if policy is not None else None,
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
        refused = [
            ("NULL frame", call(frame=None)), ("NULL bitmap", call(bitmap=None)), ("NULL policy", call(policy=None)), ("NULL out", call(null_out=True)),
            ("NULL cluster_entries", call(o=outputs(cluster_entries=None))), ("NULL entry_count", call(o=outputs(entry_count=None))),
            ("struct_size", call(o=outputs(struct_size=40))), ("unknown flags", call(o=outputs(flags=_lib.MIP_OUT_DEVICE | 0x10))),
            ("host outputs", call(o=outputs(flags=0))), ("misaligned count", call(o=outputs(entry_count=out.scal.data_ptr() + 2))),
            ("misaligned args", call(o=outputs(draw_args=out.scal.data_ptr() + 9))), ("misaligned stats", call(o=outputs(stats=out.scal.data_ptr() + 25))),
            ("entries 4-byte aligned only", call(o=outputs(cluster_entries=out.entries.data_ptr() + 4))),
            ("entries 8-byte aligned only", call(o=outputs(cluster_entries=out.entries.data_ptr() + 8))),
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
        assert lib.mip_list_clusters(None, C.addressof(frame), bm.data_ptr(), C.addressof(policy), None, None, C.addressof(good)) == INVALID
        assert call(cone=good_cone) == NOT_READY        # a cluster table, no cone table
        assert out.untouched()
        _list_given(p, s, want, name + " after the refusals")     # the context is usable, without a cone
        p.build_cluster_cones()
        assert call(cone=good_cone) == 0 and not out.untouched()
        # stale tables: a new cluster table makes the cones stale, new geometry the cluster table
        fresh = _Out(4)
        p.build_clusters()
        assert call(cone=good_cone, o=fresh.outputs()) == NOT_READY and fresh.untouched()
        assert call(o=fresh.outputs()) == 0
        fresh = _Out(4)
        p.set_geometry(s["vertices"], s["indices"])
        assert call(o=fresh.outputs()) == NOT_READY and call(cone=good_cone, o=fresh.outputs()) == NOT_READY and fresh.untouched()
        p.set_mesh_table(s["meshes"])
        assert call(o=fresh.outputs()) == NOT_READY and fresh.untouched()
        p.build_clusters()
        _list_given(p, s, want, name + " after the rebuild")
    # no instances: not ready
    with ra.InstancePipeline(max_instances=4, max_meshes=len(s["meshes"])) as p:
        p.set_mesh_table(s["meshes"])
        p.set_geometry(s["vertices"], s["indices"])
        p.build_clusters()
        fresh = _Out(4)
        with pytest.raises(ra.MipError) as e:
            p.list_clusters(make_frame(s["planes"], s["cam_pos"]), bm.data_ptr(), policy, fresh.outputs())
        assert e.value.code == NOT_READY and fresh.untouched()
