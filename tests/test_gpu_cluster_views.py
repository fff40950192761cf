"""Cluster culling of several views in one call on the GPU (include/mi_instance_pipeline.h, mip_cull_clusters_views): every byte
of every output buffer, whole and sentinel-filled before the call, against the numpy restatement
(tests/cluster_views_restatement.py) AND against one mip_cull_clusters call per view on the same context (THE EQUIVALENCE of
the header); the hand-written scenes (tests/cluster_view_cases.py); ladders on the structural edges of the launch plan
(renderer_amd/csrc/cluster_views_plan.hpp), also with reversed and scrambled tiles under the diagnostic library; both overflow
rules per view and who reports them; the scratch of the call; every refusal. Bitmaps come from a mip_run_views in front of the
call with no wait in between, from a NULL entry, or from one pointer two views with different planes share. Not reference
behaviour: parity is with the restatement."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_restatement as cr
import cluster_view_cases as cv
import cluster_views_restatement as cvr
import lod_restatement as lr
import test_gpu_batch as T
import test_gpu_batch_lods as TL
import test_gpu_clusters as TC
from renderer_amd import _lib
from renderer_amd.pipeline import make_cluster_view_outputs, make_frame, make_lod_policy

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = T.SENTINEL
PAD = 3
ra = T.ra   # the module's library fixture
NOT_READY, INVALID, CAPACITY = -6, -1, -4
MODES = (lr.DISTANCE, lr.RELATIVE)


class _ViewOut:
    """Device outputs of mip_cull_clusters_views, every word a sentinel: n_views x stride commands, the counts and the stats,
    PAD entries nobody may touch behind each."""

    def __init__(self, n_views, stride, stats=True):
        import torch

        fill = T._i32(SENTINEL)
        self.n_views, self.stride, self.stats = n_views, int(stride), stats
        self.cmds = torch.full((n_views * self.stride + PAD, 5), fill, dtype=torch.int32, device=T._dev())
        self.counts = torch.full((n_views + PAD,), fill, dtype=torch.int32, device=T._dev())
        self.st = torch.full((2 + 2 * n_views + PAD,), fill, dtype=torch.int32, device=T._dev())
        torch.cuda.synchronize()

    def outputs(self, cmd_stride=None, work_capacity=0, async_=False):
        return make_cluster_view_outputs(self.cmds.data_ptr(), self.stride if cmd_stride is None else cmd_stride, self.counts.data_ptr(),
                                         self.st.data_ptr() if self.stats else 0, work_capacity=work_capacity, async_=async_)

    def result(self):
        import torch

        torch.cuda.synchronize()
        u = lambda t: t.cpu().numpy().view(np.uint32)   # noqa: E731
        return dict(cmds=u(self.cmds), counts=u(self.counts), stats=u(self.st))

    def check(self, want, what, stride=None):
        """Every buffer whole: what the call owes under `stride` (default: the room of a view), the sentinel everywhere else."""
        stride = self.stride if stride is None else int(stride)
        got, full = self.result(), cvr.fill_outputs(want, self.n_views, stride, SENTINEL, 0, stats=self.stats)
        used = self.n_views * stride
        assert got["counts"][: self.n_views].tolist() == full["counts"].tolist(), (what, "cmd_counts", got["counts"][: self.n_views].tolist(), full["counts"].tolist())
        assert got["stats"][: 2 + 2 * self.n_views].tolist() == full["stats"].tolist(), (what, "stats", got["stats"].tolist(), full["stats"].tolist())
        assert got["cmds"][:used].tobytes() == full["cmds"].tobytes(), (what, "commands")
        assert (got["cmds"][used:] == SENTINEL).all() and (got["counts"][self.n_views:] == SENTINEL).all(), (what, "behind the views' ranges")
        assert (got["stats"][2 + 2 * self.n_views:] == SENTINEL).all(), (what, "behind the stats")
        return got

    def untouched(self):
        got = self.result()
        return all((got[k] == SENTINEL).all() for k in got)


def _hand_want(hand, stride):
    """A hand-written answer (every command of every view, the stats) as the restatement's dict under `stride`."""
    return dict(cmds=[c[:stride] for c in hand["cmds"]], counts=np.array([min(len(c), stride) for c in hand["cmds"]], np.uint32), stats=hand["stats"])


def _plain_per_view(p, planes, cam0, bases, ptrs, n, policy, stride, got, what):
    """THE EQUIVALENCE: one mip_cull_clusters per view on the same context — frames[v] with frames[0]'s camera, the view's own
    bitmap (a full one where the entry is NULL), cmd_capacity = cmd_stride — writes view v's range, count, heads and survivors."""
    ones = TC._device_bitmap(np.full((max(n, 1) + 31) // 32, 0xFFFFFFFF, np.uint32))
    for v in range(len(planes)):
        o = TC._Out(stride, stats=True)
        p.cull_clusters(make_frame(planes[v], cam0, first_instance_base=bases[v]), ptrs[v] or ones.data_ptr(), policy, o.outputs(cmd_capacity=stride))
        cmds, scal = o.result()
        count = int(scal[0])
        assert int(got["counts"][v]) == count, (what, v, "cmd_count of mip_cull_clusters")
        assert got["cmds"][v * stride: v * stride + count].tobytes() == cmds[:count].tobytes(), (what, v, "commands of mip_cull_clusters")
        assert got["stats"][2 + 2 * v: 4 + 2 * v].tolist() == scal[2:4].tolist(), (what, v, "heads and survivors of mip_cull_clusters")


# ---- 1. the restatement and the equivalence over config 3 ----

_SCENES = {}


def _scene(ra, n):
    if n not in _SCENES:
        s = TL._sized(ra.scene.make_scene(3, n=max(n, 1)), n)
        vertices, indices = ra.scene.make_geometry(s["meshes"], "strips")
        _SCENES[n] = (s, vertices, indices, cr.cluster_boxes(s["meshes"], vertices, indices))
    return _SCENES[n]


def _views_call(p, s, boxes, n_views, mode, sw, what, kinds=("culled", "shared", "null"), plain_too=True, work_capacity=0):
    """mip_run_views over the views that take a culled bitmap, then — with no wait — mip_cull_clusters_views over all of them.
    View v's bitmap is kinds[v % len(kinds)]: "culled" (its own view of mip_run_views), "shared" (view 0's pointer, under view
    v's own planes), "null" (every resident instance). The outputs whole against the restatement, then against one
    mip_cull_clusters call per view. The cameras behind view 0 are somewhere else: they are not read. The last view's
    first_instance_base wraps in the middle of the scene (cluster_view_cases.view_bases)."""
    import torch

    n = s["n"]
    cams, frusta, bases = cv.view_cams(s, n_views), cv.frusta(s["planes"], n_views), cv.view_bases(n_views, n)
    frames = [make_frame(frusta[v], cams[v], first_instance_base=bases[v]) for v in range(n_views)]
    kind = [kinds[v % len(kinds)] for v in range(n_views)]
    assert "shared" not in kind or kind[0] == "culled"
    words = (max(n, 1) + 31) // 32
    culled = [v for v in range(n_views) if kind[v] == "culled"]
    bitmaps = torch.zeros((n_views, words), dtype=torch.int32, device=T._dev())
    draw = torch.zeros((max(len(culled), 1), max(n, 1), 5), dtype=torch.int32, device=T._dev())
    scal = torch.zeros((n_views, 2), dtype=torch.int32, device=T._dev())
    ptrs = [bitmaps[v].data_ptr() if kind[v] == "culled" else bitmaps[0].data_ptr() if kind[v] == "shared" else 0 for v in range(n_views)]
    stride = max(n, 1) * 8
    out = _ViewOut(n_views, stride)
    policy = make_lod_policy(mode, sw)
    torch.cuda.synchronize()
    if n and culled:
        prepared = [p.prepare_outputs(visible_bitmap=bitmaps[v].data_ptr(), draw_cmds=draw[k].data_ptr(), draw_count=scal[v].data_ptr(),
                                      draw_index_total=scal[v].data_ptr() + 4) for k, v in enumerate(culled)]
        p.run_views([frames[v] for v in culled], prepared)          # asynchronous: prepare_outputs sets MIP_OUT_ASYNC
    p.cull_clusters_views(frames, ptrs, policy, out.outputs(work_capacity=work_capacity, async_=True))
    p.wait()
    host = bitmaps.cpu().numpy().view(np.uint32)
    host_bm = [None if kind[v] == "null" else host[0] if kind[v] == "shared" else host[v] for v in range(n_views)]
    want = cvr.cull_clusters_views(s, boxes, frusta, host_bm, bases, mode, sw, cmd_stride=stride, work_capacity=work_capacity, cam_pos=cams[0])
    assert want["status"] == 0, what
    got = out.check(want, what)
    if plain_too:
        _plain_per_view(p, frusta, cams[0], bases, ptrs, n, policy, stride, got, what)
    return want


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 1025, 4097])
@pytest.mark.parametrize("n_views", [1, 2, 3, 5, 16])
def test_restatement_and_one_call_per_view_over_config_3(ra, n, n_views):
    s, vertices, indices, boxes = _scene(ra, n)
    with TC._pipeline(ra, s, vertices, indices) as p:
        for mode in MODES:
            want = _views_call(p, s, boxes, n_views, mode, TL._metric_thresholds(s, mode), f"n={n} V={n_views} mode={mode}")
            if n == 0:
                assert (want["stats"] == 0).all() and (want["counts"] == 0).all()
            if n >= 257:
                assert int(want["stats"][0]) > n and max(want["heads"]) > 0
                if n_views >= 2:   # views 0 and 1 share a bitmap pointer and differ by their planes
                    assert want["survive"][0].tolist() != want["survive"][1].tolist()
        if n in cv.KNOWN and n_views == 5:   # the answers pinned on the CPU: full bitmaps, the pin policy
            want = _views_call(p, s, boxes, n_views, lr.DISTANCE, lr.PIN_SWITCH_SQ, f"n={n} known answers", kinds=("null",), plain_too=False)
            assert (int(want["stats"][0]), int(want["stats"][1])) == (cv.KNOWN[n]["W"], cv.KNOWN[n]["members"])
            assert list(zip(want["heads"], want["survivors"])) == cv.KNOWN[n]["views"][:5]


# ---- 2. every hand-written scene, against the hand-written bytes ----

_CASES = cv.cases()


def _given_call(p, s, views, hand, what, async_=False, work_capacity=0, stride=None, plain_too=False):
    """mip_cull_clusters_views over uploaded bitmaps (at rest) and the views' own frames; the outputs whole against `hand`."""
    n_views = len(views["planes"])
    uploaded = [None if b is None else TC._device_bitmap(b) for b in views["bitmaps"]]
    ptrs = [0 if t is None else t.data_ptr() for t in uploaded]
    frames = [make_frame(views["planes"][v], views["cams"][v], first_instance_base=views["bases"][v]) for v in range(n_views)]
    stride = max([len(c) for c in hand["cmds"]] + [1]) if stride is None else stride
    out = _ViewOut(n_views, stride)
    policy = make_lod_policy(views["mode"], views["switch"])
    p.cull_clusters_views(frames, ptrs, policy, out.outputs(work_capacity=work_capacity, async_=async_))
    if async_:
        p.wait()
    got = out.check(_hand_want(hand, stride), what)
    if plain_too:
        _plain_per_view(p, views["planes"], views["cams"][0], views["bases"], ptrs, s["n"], policy, stride, got, what)
    return out


@pytest.mark.parametrize("name,s,views,hand", _CASES, ids=[c[0] for c in _CASES])
def test_hand_cases(ra, name, s, views, hand):
    with TC._pipeline(ra, s, s["vertices"], s["indices"]) as p:
        _given_call(p, s, views, hand, name, plain_too=True)
        _given_call(p, s, views, hand, name + ", asynchronous", async_=True)


# ---- 3. ladders on the structural edges, read from the plan ----

def _plan_sizes(tmp):
    exe = os.path.join(str(tmp), "cluster_views_plan_sizes")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "native", "cluster_views_plan_check.cpp"), "-o", exe])
    return json.loads(subprocess.check_output([exe, "sizes"]))


EDGE_PARTS = ("tiles", "cull grid cap", "head grid cap")


def _filled(w, clusters, pattern_of, specs_of):
    """W = w work items: instances of `clusters` clusters and one shorter one. pattern_of(k): the ladder of k clusters;
    specs_of(n): the views of n instances."""
    whole, rest = divmod(w, clusters)
    n = whole + (1 if rest else 0)
    return cv.ladder_views([pattern_of(clusters)] + ([pattern_of(rest)] if rest else []), [0] * whole + ([1] if rest else []), specs_of(n))


def _edge_scenes(sizes, part):
    """[(name, scene, views, hand)] of one part. "tiles": the ladders the issue lists — W around a survive word and an item tile;
    a view's heads around a head tile while other views have no head in that tile; a wave whose lanes are all outside one view, as
    the first, a middle and the last view; bits that differ between views on lanes 0 and 63 and across items 63 | 64; a run that
    continues over a tile edge in one view and ends there in another. "cull grid cap" / "head grid cap": two views, W — and the
    call's bound on it, work_capacity = W — one below, at and one above the size at which the plan stops growing that grid and it
    starts to loop, and well above it under the library's own bound."""
    item, head, blocks = sizes["item_tile"], sizes["head_tile"], sizes["max_blocks"]
    out = []
    if part != "tiles":
        tile = item if part == "cull grid cap" else head
        cap = blocks * tile
        for w in (cap - 1, cap, cap + 1):
            # view 0 draws every instance whole, view 1 (every cluster too) only every second instance
            s, views, hand = _filled(w, 128, lambda k: "1" * k, lambda n: [("A", None, 7), ("C", np.arange(n) % 2 == 1, 8)])
            s["work_capacity"] = w
            assert int(hand["stats"][0]) == w
            out.append((f"{part}: W = bound = {w}", s, views, hand))
        # the library's own bound, two tiles past the cap: view 0 sees clusters 1 .. 126 of every instance, view 1 the first and the last
        n = (cap + 2 * tile) // 128
        out.append((f"{part}: loops", *cv.ladder_views(["0" + "1" * 126 + "0"], [0] * n, [("A", None, 3), ("B", None, 4)])))
        return out
    every_second = lambda n: np.arange(n) % 2 == 0   # noqa: E731
    for edge in (64, item):
        for w in (edge - 1, edge, edge + 1):
            out.append((f"W={w}", *_filled(w, 8, lambda k: ("10" * 4)[:k], lambda n: [("A", None, 1), ("B", every_second(n), 2), ("C", None, 3), ("D", None, 4)])))
    for h in (head - 1, head, head + 1):
        # h one-cluster instances: view 0 has h heads; views 1 and 2 none at all; view 3 one, on the last item
        last = np.arange(h) == h - 1
        s, views, hand = cv.ladder_views(["1"], [0] * h, [("A", None, 9), ("D", None, 1), ("B", None, 2), ("C", last, 5)])
        assert hand["stats"].tolist() == [h, h, h, h, 0, 0, 0, 0, 1, 1]
        out.append((f"heads={h} in one view, none in that tile in the others", s, views, hand))
    # a wave whose 64 items are all outside one view (instances 64 .. 127 of 256 one-cluster instances): as the first, a middle and the last view
    outside = ~((np.arange(256) >= 64) & (np.arange(256) < 128))
    for at in range(3):
        specs = [("A", None, 10), ("C", None, 20)]
        specs.insert(at, ("A", outside, 30))
        out.append((f"a wave outside view {at}", *cv.ladder_views(["1"], [0] * 256, specs)))
    # ... and a view none of whose waves has a live lane but the last one's last
    out.append(("one live lane in the last wave", *cv.ladder_views(["1"], [0] * 256, [("A", np.arange(256) == 255, 1), ("A", None, 2)])))
    # bits that differ between views on lanes 0, 63 and across items 63 | 64
    pick = lambda *which: np.isin(np.arange(130), which)   # noqa: E731
    out.append(("bits on lanes 0, 63 and items 63 | 64", *cv.ladder_views(["1"], [0] * 130, [("A", pick(0, 63), 1), ("A", pick(63, 64), 2), ("C", pick(64), 3),
                                                                                           ("A", pick(0), 4), ("C", pick(129), 5), ("A", pick(62, 63, 64, 65), 6)])))
    # one instance whose ladder is all ones but for clusters `item` and `head`: view C's run continues over both tile edges,
    # view A's runs end exactly there, view B sees the two clusters alone; a short instance behind it
    long_run = np.ones(head + 700, bool)
    long_run[[item, head]] = False
    out.append(("a run over a tile edge in one view, ending there in another", *cv.ladder_views([long_run, "101"], [0, 1], [("A", None, 4), ("C", None, 5), ("B", None, 6)])))
    # ... and ending one item before / starting one item behind the edges
    other = np.ones(head + 700, bool)
    other[[item - 1, item + 1, head - 1, head + 1]] = False
    out.append(("runs around the tile edges", *cv.ladder_views([other, "101"], [0, 1], [("C", None, 1), ("A", None, 2), ("B", None, 3)])))
    return out


def _run_edge_scenes(ra, scenes):
    for name, s, views, hand in scenes:
        with TC._pipeline(ra, s, s["vertices"], s["indices"]) as p:
            _given_call(p, s, views, hand, name, async_=True, work_capacity=s.get("work_capacity", 0))


@pytest.mark.parametrize("part", EDGE_PARTS)
def test_structural_edges(ra, tmp_path, part):
    sizes = _plan_sizes(tmp_path)
    scenes = _edge_scenes(sizes, part)
    by_name = {name: hand for name, _, _, hand in scenes}
    item, head = sizes["item_tile"], sizes["head_tile"]
    if part == "tiles":
        assert {int(h["stats"][0]) for h in by_name.values()} >= {63, 64, 65, item - 1, item, item + 1}          # work items on every edge
        assert {int(h["stats"][2]) for h in by_name.values()} >= {head - 1, head, head + 1}                       # a view's heads on the head tile's
        run = by_name["a run over a tile edge in one view, ending there in another"]
        assert run["cmds"][1]["indexCount"].tolist() == [192 * (head + 700), 192 * 3]                             # view C: one run over both edges
        assert run["cmds"][0]["indexCount"].tolist()[:3] == [192 * item, 192 * (head - item - 1), 192 * 699]      # view A: runs that end on them
    else:
        tile = item if part == "cull grid cap" else head
        cap = sizes["max_blocks"] * tile
        assert [int(h["stats"][0]) for h in by_name.values()][:3] == [cap - 1, cap, cap + 1]
        assert int(by_name[f"{part}: loops"]["stats"][0]) > cap + tile
    _run_edge_scenes(ra, scenes)


_EDGE_CHILD = r'''
import os, sys
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
os.environ["MIP_LIBRARY"] = os.path.join(root, "renderer_amd", "lib", "libmi_instance_pipeline_dbg.so")
import renderer_amd
import test_gpu_cluster_views as TV
TV._run_edge_scenes(renderer_amd, TV._edge_scenes(TV._plan_sizes(sys.argv[2]), sys.argv[3]))
print("CLUSTER-VIEW-EDGES-OK")
'''


@pytest.mark.parametrize("part", EDGE_PARTS)
@pytest.mark.parametrize("tiles", ["reverse", "scramble"])
def test_structural_edges_in_any_dispatch_order(tiles, part, tmp_path):
    e = dict(os.environ, MIP_DEBUG_TILE_ORDER=tiles)
    out = subprocess.run([sys.executable, "-c", _EDGE_CHILD, ROOT, str(tmp_path), part], capture_output=True, text=True, timeout=600, env=e)
    assert out.returncode == 0 and "CLUSTER-VIEW-EDGES-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ---- 4. overflow: per view, and who reports it ----

def _at_rest(s, frusta, kinds=("culled", "shared", "null")):
    """Bitmaps at rest for the views: the instance boxes against the view's planes (numpy), view 0's again, or none."""
    import numpy_restatement as nr
    import occlusion_restatement as orr

    own = orr.bitmap_of(~nr.run(dict(s, planes=frusta[0]))["coarse_culled"])
    return [None if kinds[v % len(kinds)] == "null" else own if kinds[v % len(kinds)] == "shared" or v == 0
            else orr.bitmap_of(~nr.run(dict(s, planes=frusta[v]))["coarse_culled"]) for v in range(len(frusta))]


def test_overflow_rules(ra):
    s, vertices, indices, boxes = _scene(ra, 257)
    n_views = 3
    frusta, bases = cv.frusta(s["planes"], n_views), cv.view_bases(n_views)
    host_bm = _at_rest(s, frusta)
    full = cvr.cull_clusters_views(s, boxes, frusta, host_bm, bases, lr.DISTANCE, lr.PIN_SWITCH_SQ, cmd_stride=1 << 20)
    heads, w, members = full["heads"], int(full["stats"][0]), int(full["stats"][1])
    big = int(np.argmax(heads))
    assert min(heads) > 2 and heads[big] > min(heads) and w > max(heads)
    room = heads[big]
    policy = make_lod_policy(lr.DISTANCE, lr.PIN_SWITCH_SQ)
    frames = [make_frame(frusta[v], s["cam_pos"], first_instance_base=bases[v]) for v in range(n_views)]
    uploaded = [None if b is None else TC._device_bitmap(b) for b in host_bm]
    ptrs = [0 if t is None else t.data_ptr() for t in uploaded]

    def cut(stride):
        return dict(cmds=[c[:stride] for c in full["all_cmds"]], counts=np.array([min(h, stride) for h in heads], np.uint32), stats=full["stats"])

    refused = dict(cmds=[full["cmds"][0][:0]] * n_views, counts=np.zeros(n_views, np.uint32), stats=np.array([w, members] + [0] * (2 * n_views), np.uint32))
    with TC._pipeline(ra, s, vertices, indices) as p:
        def overflows(out, async_, **kw):
            """MIP_ERR_CAPACITY once: from the call, or from mip_wait for an asynchronous one; then the context is clean again."""
            with pytest.raises(ra.MipError) as e:
                p.cull_clusters_views(frames, ptrs, policy, out.outputs(async_=async_, **kw))
                p.wait()
            assert e.value.code == CAPACITY
            p.wait()

        for async_ in (False, True):
            for stride in (room - 1, 0):        # the largest view is cut at its first `stride` commands, the others are complete where they fit
                out = _ViewOut(n_views, room)
                overflows(out, async_, cmd_stride=stride)
                out.check(cut(stride), f"cmd_stride {stride} async={async_}", stride=stride)
                if stride:
                    assert [int(c) for c in cut(stride)["counts"]] == [min(h, stride) for h in heads] and min(heads) <= stride
            out = _ViewOut(n_views, room)       # W - 1: nothing but the zero counts and the refusal's stats
            overflows(out, async_, work_capacity=w - 1)
            out.check(refused, f"work_capacity W - 1 async={async_}")
            out = _ViewOut(n_views, room)       # a fitting call on the same context is complete
            p.cull_clusters_views(frames, ptrs, policy, out.outputs(cmd_stride=room, work_capacity=w, async_=async_))
            p.wait()
            out.check(cut(room), f"fitting call async={async_}")

        # a synchronous mip_cull_clusters behind a frame slot between two calls: not charged with the asynchronous views call's
        # overflow in front of it, its outputs unchanged; mip_wait then reports that overflow once
        plain_frame = make_frame(frusta[0], s["cam_pos"], first_instance_base=bases[0])
        ref = TC._Out(room)
        p.cull_clusters(plain_frame, ptrs[0], policy, ref.outputs())
        a, b, c = _ViewOut(n_views, room), TC._Out(room), _ViewOut(n_views, room)
        p.cull_clusters_views(frames, ptrs, policy, a.outputs(cmd_stride=1, async_=True))
        p.cull_clusters(plain_frame, ptrs[0], policy, b.outputs())                       # returns MIP_OK
        assert all(x.tobytes() == y.tobytes() for x, y in zip(b.result(), ref.result())) and int(b.result()[1][0]) == heads[0]
        p.cull_clusters_views(frames, ptrs, policy, c.outputs(async_=True))
        with pytest.raises(ra.MipError) as e:
            p.wait()
        assert e.value.code == CAPACITY
        a.check(cut(1), "the overflow in front of the plain call", stride=1)
        c.check(cut(room), "the fitting call behind it")
        p.wait()
        # ... and the other way round: an asynchronous mip_cull_clusters overflows, a synchronous views call that fits is not charged
        a, b = TC._Out(room), _ViewOut(n_views, room)
        p.cull_clusters(plain_frame, ptrs[0], policy, a.outputs(cmd_capacity=1, async_=True))
        p.cull_clusters_views(frames, ptrs, policy, b.outputs())                         # returns MIP_OK
        b.check(cut(room), "a fitting synchronous views call behind a plain overflow")
        with pytest.raises(ra.MipError) as e:
            p.wait()
        assert e.value.code == CAPACITY and int(a.result()[1][0]) == 1
        p.wait()


# ---- 5. the call's own scratch ----

def test_a_larger_call_grows_the_scratch_and_a_smaller_one_reuses_it(ra):
    s, vertices, indices, boxes = _scene(ra, 1025)
    with TC._pipeline(ra, s, vertices, indices) as p:
        w = int(_views_call(p, s, boxes, 1, lr.DISTANCE, lr.PIN_SWITCH_SQ, "scratch, V=1, a tight bound", kinds=("null",), plain_too=False,
                            work_capacity=cv.KNOWN[1025]["W"])["stats"][0])
        assert w == cv.KNOWN[1025]["W"]
        for n_views, work_capacity in ((4, w), (16, 0), (2, w), (16, w), (3, 0)):   # more planes, then the library's bound, then fewer and smaller again
            _views_call(p, s, boxes, n_views, lr.DISTANCE, lr.PIN_SWITCH_SQ, f"scratch, V={n_views} work_capacity={work_capacity}", kinds=("null",),
                        plain_too=n_views == 3, work_capacity=work_capacity)


# ---- 6. every refusal writes nothing and leaves the context usable ----

def test_refusals_write_nothing(ra):
    name, s, views, hand = _CASES[0]
    n_views = len(views["planes"])
    with TC._pipeline(ra, s, s["vertices"], s["indices"]) as p:
        lib, ctx = p._lib, p._ctx
        out = _ViewOut(n_views, 8)
        frames = (_lib.MipFrame * n_views)()
        for v in range(n_views):
            C.memmove(C.addressof(frames[v]), C.addressof(make_frame(views["planes"][v], views["cams"][v], first_instance_base=views["bases"][v])),
                      C.sizeof(_lib.MipFrame))
        bitmaps = (C.c_void_p * n_views)(*[None] * n_views)
        policy = make_lod_policy(views["mode"], views["switch"])

        def outputs(**kw):
            o = out.outputs()
            for k, v in kw.items():
                setattr(o, k, v)
            return o

        def call(o=None, policy=policy, fr=frames, bm=bitmaps, k=n_views, context=ctx):
            o = outputs() if o is None else o
            addr = lambda x: C.addressof(x) if x is not None else None   # noqa: E731
            return lib.mip_cull_clusters_views(context, addr(fr), addr(bm), k, addr(policy), addr(o) if o != "null" else None)

        bad_policy = make_lod_policy(views["mode"], views["switch"])
        bad_policy.switch_sq[1] = 1.0           # decreases
        wrong_size = make_lod_policy(views["mode"], views["switch"])
        wrong_size.struct_size = 24
        bad_mode = make_lod_policy(views["mode"], views["switch"])
        bad_mode.mode = 2
        refused = {
            "NULL ctx": call(context=None), "NULL frames": call(fr=None), "NULL visible_bitmaps": call(bm=None), "NULL policy": call(policy=None),
            "NULL out": call(o="null"), "NULL cluster_cmds": call(outputs(cluster_cmds=None)), "NULL cmd_counts": call(outputs(cmd_counts=None)),
            "struct_size 36": call(outputs(struct_size=36)), "struct_size 48": call(outputs(struct_size=48)),
            "unknown flags": call(outputs(flags=_lib.MIP_OUT_DEVICE | 0x10)), "host outputs": call(outputs(flags=0)),
            "misaligned cmd_counts": call(outputs(cmd_counts=out.counts.data_ptr() + 2)), "misaligned cluster_cmds": call(outputs(cluster_cmds=out.cmds.data_ptr() + 1)),
            "misaligned stats": call(outputs(stats=out.st.data_ptr() + 2)), "zero views": call(k=0), "seventeen views": call(k=17),
            "decreasing thresholds": call(policy=bad_policy), "policy struct_size": call(policy=wrong_size), "policy mode": call(policy=bad_mode),
        }
        assert all(rc == INVALID for rc in refused.values()), refused
        assert lib.mip_last_error(ctx) and out.untouched()
        _given_call(p, s, views, hand, name + " after the refusals")     # the context is usable
    # no instances; no cluster table; a stale one: not ready, nothing written
    fresh = _ViewOut(n_views, 8)
    frames = [make_frame(views["planes"][v], views["cams"][v]) for v in range(n_views)]
    with ra.InstancePipeline(max_instances=4, max_meshes=len(s["meshes"])) as p:
        p.set_mesh_table(s["meshes"])
        p.set_geometry(s["vertices"], s["indices"])
        p.build_clusters()
        with pytest.raises(ra.MipError) as e:
            p.cull_clusters_views(frames, [0] * n_views, policy, fresh.outputs())
        assert e.value.code == NOT_READY and fresh.untouched()
    with T._pipeline(ra, s) as p:
        p.set_geometry(s["vertices"], s["indices"])
        with pytest.raises(ra.MipError) as e:                    # no table yet
            p.cull_clusters_views(frames, [0] * n_views, policy, fresh.outputs())
        assert e.value.code == NOT_READY and fresh.untouched()
        p.build_clusters()
        p.set_geometry(s["vertices"], s["indices"])             # stale again
        with pytest.raises(ra.MipError) as e:
            p.cull_clusters_views(frames, [0] * n_views, policy, fresh.outputs())
        assert e.value.code == NOT_READY and fresh.untouched()
        p.build_clusters()
        _given_call(p, s, views, hand, name + " after the table was built again")
