"""mip_list_clusters_views on the GPU (include/mi_instance_pipeline.h): every byte of every output buffer, whole and
sentinel-filled before the call, against the numpy restatement (tests/cluster_views_list_restatement.py), against the
hand-written lists (tests/cluster_view_list_cases.py), against one mip_list_clusters call per view on the same context
(equivalence (a) of the header) and against the expansion of what mip_cull_clusters_views just wrote on the same context
(equivalence (b)); ladders on the structural edges of the launch plan (renderer_amd/csrc/cluster_views_list_plan.hpp), also
with reversed and scrambled tiles under the diagnostic library; both overflow rules per view and who reports them; the scratch
the two several-view calls share; every refusal. The stride handed to a call leaves PAD entries behind every view's survivors
and the buffer PAD rows behind the last view: nobody may touch them. Not reference behaviour: parity is with the restatement."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_list_restatement as clr
import cluster_restatement as cr
import cluster_view_cases as cv
import cluster_view_list_cases as cvlc
import cluster_views_list_restatement as cvlr
import lod_restatement as lr
import test_gpu_batch as T
import test_gpu_batch_lods as TL
import test_gpu_cluster_list as TLST
import test_gpu_cluster_views as TV
import test_gpu_clusters as TC
from renderer_amd import _lib
from renderer_amd.pipeline import DRAW_CMD_DTYPE, make_cluster_view_list_outputs, make_frame, make_lod_policy

pytestmark = pytest.mark.gpu
ROOT = TC.ROOT
SENTINEL = T.SENTINEL
PAD = 3
ra = T.ra   # the module's library fixture
NOT_READY, INVALID, CAPACITY = -6, -1, -4
MODES = (lr.DISTANCE, lr.RELATIVE)


class _Out:
    """Device outputs of mip_list_clusters_views, every word a sentinel: n_views x stride entries, the counts, the draw
    arguments and the stats, PAD rows / words nobody may touch behind each."""

    def __init__(self, n_views, stride, args=True, stats=True):
        import torch

        fill = T._i32(SENTINEL)
        self.n_views, self.stride, self.args, self.stats = n_views, int(stride), args, stats
        self.entries = torch.full((n_views * self.stride + PAD, 4), fill, dtype=torch.int32, device=T._dev())
        self.counts = torch.full((n_views + PAD,), fill, dtype=torch.int32, device=T._dev())
        self.ar = torch.full((4 * n_views + PAD,), fill, dtype=torch.int32, device=T._dev())
        self.st = torch.full((2 + n_views + PAD,), fill, dtype=torch.int32, device=T._dev())
        torch.cuda.synchronize()

    def outputs(self, entry_stride=None, work_capacity=0, async_=False):
        return make_cluster_view_list_outputs(self.entries.data_ptr(), self.stride if entry_stride is None else entry_stride, self.counts.data_ptr(),
                                              self.ar.data_ptr() if self.args else 0, self.st.data_ptr() if self.stats else 0,
                                              work_capacity=work_capacity, async_=async_)

    def small(self):
        """The counts, the draw arguments and the stats."""
        import torch

        torch.cuda.synchronize()
        u = lambda t: t.cpu().numpy().view(np.uint32)   # noqa: E731
        return dict(counts=u(self.counts), args=u(self.ar), stats=u(self.st))

    def result(self):
        got = self.small()
        got["entries"] = self.entries.cpu().numpy().view(np.uint32)
        return got

    def check_small(self, want, what, stride=None):
        stride = self.stride if stride is None else int(stride)
        got, full = self.small(), cvlr.fill_outputs(dict(want, entries=[e[:0] for e in want["entries"]]), self.n_views, stride, SENTINEL, PAD, self.args, self.stats)
        for k in ("counts", "args", "stats"):
            assert got[k].tolist() == full[k].tolist(), (what, k, got[k].tolist(), full[k].tolist())

    def check(self, want, what, stride=None):
        """Every buffer whole: what the call owes under `stride` (default: the room of a view), the sentinel everywhere else."""
        stride = self.stride if stride is None else int(stride)
        self.check_small(want, what, stride)
        got, full = self.result(), cvlr.fill_outputs(want, self.n_views, stride, SENTINEL, 0)
        used = self.n_views * stride
        assert got["entries"][:used].tobytes() == full["entries"].tobytes(), (what, "entries")
        assert (got["entries"][used:] == SENTINEL).all(), (what, "behind the last view's range")
        return got

    def untouched(self):
        got = self.result()
        return all((got[k] == SENTINEL).all() for k in got)


def _hand_want(hand, stride):
    """A hand-written answer (every entry of every view, the stats) as the restatement's dict under `stride`."""
    counts = np.array([min(len(e), stride) for e in hand["entries"]], np.uint32)
    return dict(entries=[e[:stride] for e in hand["entries"]], counts=counts, args=cvlr.draw_args(counts, stride), stats=hand["stats"])


def _one_list_per_view(p, planes, cam0, bases, ptrs, n, policy, stride, got, what):
    """Equivalence (a): one mip_list_clusters per view on the same context — frames[v] with frames[0]'s camera, the view's own
    bitmap (a full one where the entry is NULL), entry_capacity = entry_stride — writes view v's entries, count and survivors."""
    ones = TC._device_bitmap(np.full((max(n, 1) + 31) // 32, 0xFFFFFFFF, np.uint32))
    for v in range(len(planes)):
        o = TLST._Out(stride)
        p.list_clusters(make_frame(planes[v], cam0, first_instance_base=bases[v]), ptrs[v] or ones.data_ptr(), policy, o.outputs(entry_capacity=stride))
        entries, scal = o.result()
        count = int(scal[0])
        assert int(got["counts"][v]) == count, (what, v, "entry_count of mip_list_clusters")
        assert got["entries"][v * stride: v * stride + count].tobytes() == entries[:count].tobytes(), (what, v, "entries of mip_list_clusters")
        assert int(got["stats"][2 + v]) == int(scal[6]), (what, v, "survivors of mip_list_clusters")
        assert got["args"][4 * v: 4 * v + 4].tolist() == [192, int(scal[3]), 0, v * stride], (what, v, "draw_args")


def _expanded_commands(p, frames, ptrs, policy, n_views, cmd_stride, stride, got, what, work_capacity=0):
    """Equivalence (b): view v's entries are the expansion of view v's command range of mip_cull_clusters_views."""
    o = TV._ViewOut(n_views, cmd_stride)
    p.cull_clusters_views(frames, ptrs, policy, o.outputs(work_capacity=work_capacity))
    r = o.result()
    for v in range(n_views):
        count = int(r["counts"][v])
        assert int(r["stats"][2 + 2 * v]) == count, (what, v, "cmd_stride too small for the comparison")
        cmds = np.ascontiguousarray(r["cmds"][v * cmd_stride: v * cmd_stride + count]).view(DRAW_CMD_DTYPE).reshape(-1)
        e = clr.from_commands(cmds, None)
        assert len(e) == int(got["counts"][v]) == int(r["stats"][3 + 2 * v]), (what, v, "survivors of mip_cull_clusters_views")
        assert got["entries"][v * stride: v * stride + len(e)].tobytes() == e.tobytes(), (what, v, "the expansion of mip_cull_clusters_views' commands")
    assert got["stats"][:2].tolist() == r["stats"][:2].tolist(), (what, "W and members")


# ---- 1. every hand-written scene, against the hand-written bytes ----

_CASES = cvlc.cases()


def _given_call(p, s, views, hand, what, async_=False, work_capacity=0, stride=None, args=True, stats=True, equivalences=False):
    """mip_list_clusters_views over uploaded bitmaps (at rest) and the views' own frames; the outputs whole against `hand`."""
    n_views = len(views["planes"])
    uploaded = [None if b is None else TC._device_bitmap(b) for b in views["bitmaps"]]
    ptrs = [0 if t is None else t.data_ptr() for t in uploaded]
    frames = [make_frame(views["planes"][v], views["cams"][v], first_instance_base=views["bases"][v]) for v in range(n_views)]
    stride = max(len(e) for e in hand["entries"]) + PAD if stride is None else stride
    out = _Out(n_views, stride, args, stats)
    policy = make_lod_policy(views["mode"], views["switch"])
    p.list_clusters_views(frames, ptrs, policy, out.outputs(work_capacity=work_capacity, async_=async_))
    if async_:
        p.wait()
    got = out.check(_hand_want(hand, stride), what)
    if equivalences:
        _one_list_per_view(p, views["planes"], views["cams"][0], views["bases"], ptrs, s["n"], policy, stride, got, what)
        _expanded_commands(p, frames, ptrs, policy, n_views, stride, stride, got, what)
    return out


@pytest.mark.parametrize("name,s,views,hand", _CASES, ids=[c[0] for c in _CASES])
def test_hand_cases(ra, name, s, views, hand):
    with TC._pipeline(ra, s, s["vertices"], s["indices"]) as p:
        _given_call(p, s, views, hand, name, equivalences=True)
        _given_call(p, s, views, hand, name + ", asynchronous", async_=True)
        _given_call(p, s, views, hand, name + ", no draw_args", args=False)
        _given_call(p, s, views, hand, name + ", no stats", stats=False, async_=True)


# ---- 2. the restatement and both equivalences over config 3 ----

def _views_call(p, s, boxes, n_views, mode, sw, what, kinds=("culled", "shared", "null"), equivalences=True, work_capacity=0):
    """mip_run_views over the views that take a culled bitmap, then — with no wait — mip_list_clusters_views over all of them.
    View v's bitmap is kinds[v % len(kinds)]: "culled" (its own view of mip_run_views), "shared" (view 0's pointer, under view
    v's own planes), "null" (every resident instance). The outputs whole against the restatement, then against one
    mip_list_clusters per view and against the expansion of mip_cull_clusters_views' commands, on the same context."""
    import torch

    n = s["n"]
    cams, frusta, bases = cv.view_cams(s, n_views), cv.frusta(s["planes"], n_views), cv.view_bases(n_views, n)
    frames = [make_frame(frusta[v], cams[v], first_instance_base=bases[v]) for v in range(n_views)]
    kind = [kinds[v % len(kinds)] for v in range(n_views)]
    words = (max(n, 1) + 31) // 32
    culled = [v for v in range(n_views) if kind[v] == "culled"]
    bitmaps = torch.zeros((n_views, words), dtype=torch.int32, device=T._dev())
    draw = torch.zeros((max(len(culled), 1), max(n, 1), 5), dtype=torch.int32, device=T._dev())
    scal = torch.zeros((n_views, 2), dtype=torch.int32, device=T._dev())
    ptrs = [bitmaps[v].data_ptr() if kind[v] == "culled" else bitmaps[0].data_ptr() if kind[v] == "shared" else 0 for v in range(n_views)]
    stride = max(n, 1) * int(cr.cluster_table(s["meshes"])["C"].max()) + PAD     # every cluster of every instance fits, and PAD rows
    out = _Out(n_views, stride)
    policy = make_lod_policy(mode, sw)
    torch.cuda.synchronize()
    if n and culled:
        prepared = [p.prepare_outputs(visible_bitmap=bitmaps[v].data_ptr(), draw_cmds=draw[k].data_ptr(), draw_count=scal[v].data_ptr(),
                                      draw_index_total=scal[v].data_ptr() + 4) for k, v in enumerate(culled)]
        p.run_views([frames[v] for v in culled], prepared)          # asynchronous: prepare_outputs sets MIP_OUT_ASYNC
    p.list_clusters_views(frames, ptrs, policy, out.outputs(work_capacity=work_capacity, async_=True))
    p.wait()
    host = bitmaps.cpu().numpy().view(np.uint32)
    host_bm = [None if kind[v] == "null" else host[0] if kind[v] == "shared" else host[v] for v in range(n_views)]
    want = cvlr.list_clusters_views(s, boxes, frusta, host_bm, bases, mode, sw, stride, work_capacity, cam_pos=cams[0])
    assert want["status"] == 0, what
    got = out.check(want, what)
    if equivalences:
        _one_list_per_view(p, frusta, cams[0], bases, ptrs, n, policy, stride, got, what)
        _expanded_commands(p, frames, ptrs, policy, n_views, max(n, 1) * 8, stride, got, what, work_capacity)
    return want


@pytest.mark.parametrize("n", [0, 1, 257, 4097])
@pytest.mark.parametrize("n_views", [1, 2, 5, 16])
def test_restatement_and_both_equivalences_over_config_3(ra, n, n_views):
    s, vertices, indices, boxes = TV._scene(ra, n)
    with TC._pipeline(ra, s, vertices, indices) as p:
        for mode in MODES:
            want = _views_call(p, s, boxes, n_views, mode, TL._metric_thresholds(s, mode), f"n={n} V={n_views} mode={mode}")
            if n == 0:
                assert (want["stats"] == 0).all() and (want["counts"] == 0).all() and (want["args"][:, 0] == 192).all() and want["args"][:, 3].tolist() == sorted(set(want["args"][:, 3].tolist()))
            if n >= 257:
                assert int(want["stats"][0]) > n and max(int(x) for x in want["stats"][2:]) > 0
                if n_views >= 2:   # views 0 and 1 share a bitmap pointer and differ by their planes
                    assert want["survive"][0].tolist() != want["survive"][1].tolist()
        if n in cv.KNOWN and n_views == 5:   # the answers pinned on the CPU: full bitmaps, the pin policy
            want = _views_call(p, s, boxes, n_views, lr.DISTANCE, lr.PIN_SWITCH_SQ, f"n={n} known answers", kinds=("null",), equivalences=False)
            assert want["stats"].tolist() == [cv.KNOWN[n]["W"], cv.KNOWN[n]["members"]] + [sv for _, sv in cv.KNOWN[n]["views"][:5]]


# ---- 3. ladders on the structural edges, read from the plan ----

def _plan_sizes(tmp):
    exe = os.path.join(str(tmp), "cluster_views_list_plan_sizes")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "native", "cluster_views_list_plan_check.cpp"), "-o", exe])
    return json.loads(subprocess.check_output([exe, "sizes"]))


EDGE_PARTS = ("tiles", "members", "write grid cap", "word grid cap")


def _filled(w, clusters, pattern_of, specs_of):
    """W = w work items: instances of `clusters` clusters and one shorter one. pattern_of(k): the ladder of k clusters;
    specs_of(n): the views of n instances."""
    whole, rest = divmod(w, clusters)
    n = whole + (1 if rest else 0)
    return cvlc.ladder_views_list([pattern_of(clusters)] + ([pattern_of(rest)] if rest else []), [0] * whole + ([1] if rest else []), specs_of(n))


def _edge_scenes(sizes, part):
    """[(name, scene, views, hand)] of the parts that are compared on the host. "tiles": W one below, at and one above a survive
    word, an item tile and a list tile under four views that see different clusters; a wave wholly outside one view, as view 0,
    7 and 15 of sixteen; a wave outside every view; a lone survivor on a list tile's edge in one view while the others have
    none in that tile. "members": members whose first item is at 64 k - 1 / 64 k / 64 k + 1, 64 one-cluster members in a word,
    a member across a list tile's edge, members only in the last instance tile."""
    item, tile = sizes["item_tile"], sizes["list_tile"]
    out = []
    every_second = lambda n: np.arange(n) % 2 == 0   # noqa: E731
    if part == "tiles":
        for edge in (64, item, tile):
            for w in (edge - 1, edge, edge + 1):
                out.append((f"W={w}", *_filled(w, 8, lambda k: ("10" * 4)[:k], lambda n: [("A", None, 1), ("B", every_second(n), 2), ("C", None, 0xFFFFFFFF - 5), ("D", None, 4)])))
        # 256 one-cluster instances; instances 64 .. 127 (one wave's 64 items) are outside ONE view of sixteen: the first, a middle, the last
        outside = ~((np.arange(256) >= 64) & (np.arange(256) < 128))
        for at in (0, 7, 15):
            specs = [("A" if v % 2 else "C", None, 10 + v) for v in range(15)]
            specs.insert(at, ("A", outside, 300))
            out.append((f"a wave outside view {at}", *cvlc.ladder_views_list(["1"], [0] * 256, specs)))
        # ... and outside every view: by the bitmap in two of them, by the frustum in the third
        out.append(("a wave outside every view", *cvlc.ladder_views_list(["1"], [0] * 256, [("A", outside, 1), ("D", None, 2), ("C", outside, 3)])))
        # one live lane in the last wave's last item in one view
        out.append(("one live lane in the last wave", *cvlc.ladder_views_list(["1"], [0] * 256, [("A", np.arange(256) == 255, 1), ("A", None, 2)])))
        # three list tiles of one-cluster instances: view 0 has one survivor, the last item of the second tile; view 1 one, the first
        # item of the second tile; view 2 none; view 3 all
        n = 3 * tile
        for at in (tile - 1, tile, 2 * tile - 1, 2 * tile):
            out.append((f"a lone survivor at item {at}", *cvlc.ladder_views_list(["1"], [0] * n, [("A", np.arange(n) == at, 9), ("D", None, 1), ("C", np.arange(n) == at + 1, 2),
                                                                                                 ("B", None, 5)])))
        return out
    alt = lambda k: ("10" * k)[:k]   # noqa: E731
    views = [("A", None, 1), ("B", None, 2), ("C", None, 3)]
    # first items at 64 k - 1, 64 k, 64 k + 1 (63, 64, 193, 255 ...), C = 1, 64, 65, 129
    out.append(("first items around word edges", *cvlc.ladder_views_list([alt(63), alt(1), alt(64), alt(65), alt(62), alt(3), alt(129)], [0, 1, 2, 3, 4, 5, 5, 6, 6, 3, 2, 6], views)))
    # 64 members in every word (C = 1), 200 of them, every second one in view 1 only
    out.append(("64 members in a word", *cvlc.ladder_views_list(["1"], [0] * 200, [("A", None, 3), ("C", every_second(200), 4)])))
    # a member that starts one item before / at / behind a LIST tile's edge
    for d in (-1, 0, 1):
        out.append((f"a member at the list tile's edge {d:+d}", *cvlc.ladder_views_list(["1" * (tile + d), alt(129), "1"], [0, 1, 2, 1], views)))
    # members only in the last instance tile (and only its last instance), in one view; none in the other
    n = 2 * sizes["instance_tile"] + 1
    out.append(("members in the last tile", *cvlc.ladder_views_list(["1101"], [0] * n, [("A", np.arange(n) == n - 1, 6), ("D", np.arange(n) == n - 1, 7)])))
    return out


def _closed_form_on_device(n_whole, clusters, lo, hi, rest, base, first=0, step=1):
    """The closed form of one view's list as a device tensor: instances first, first + step, ... of n_whole instances of mesh 0
    (`clusters` clusters, [lo, hi) of them survive) and, when rest > 0 and the progression reaches it, the one instance of mesh 1
    behind them (`rest` clusters, all survive)."""
    import torch

    per = hi - lo
    picked = len(range(first, n_whole, step))
    tail = rest if rest and (n_whole - first) % step == 0 and n_whole >= first else 0
    e = torch.arange(picked * per + tail, dtype=torch.int64, device=T._dev())
    whole = e < picked * per
    inst = torch.where(whole, first + step * (e // per), torch.full_like(e, n_whole))
    c = torch.where(whole, lo + e % per, e - picked * per)
    want = torch.zeros((len(e), 4), dtype=torch.int64, device=T._dev())
    want[:, 0] = (inst + base) & 0xFFFFFFFF
    want[:, 1] = 192 * c + torch.where(whole, torch.zeros_like(e), torch.full_like(e, 192 * clusters))
    want[:, 3] = 192
    return want.to(torch.int32)


def _cap_scenes(sizes, part):
    """[(name, scene, views, work_capacity, closed forms per view, stats)]: two views — view 0 draws every instance whole, view 1
    every second one — with W, and the call's bound on it, one below, at and one above the size at which the plan stops growing
    the write kernel's grid (max_blocks item tiles), and two tiles past it under the library's own bound with the first and the
    last cluster of every instance seen by view 1 alone. "word grid cap": the same at max_blocks LIST tiles, where the
    word-member and count kernels' grids stop growing."""
    import cluster_cases as cc

    step = sizes["item_tile"] if part == "write grid cap" else sizes["list_tile"]
    cap = sizes["max_blocks"] * step
    out = []
    for w in (cap - 1, cap, cap + 1):
        whole, rest = divmod(w, 128)
        n = whole + (1 if rest else 0)
        s, _ = cc.ladder_scene(["1" * 128] + (["1" * rest] if rest else []), [0] * whole + ([1] if rest else []))
        odd = np.arange(n) % 2 == 1
        views = cv._views([cv.A, cv.C], bitmaps=[None, cv.bits(n, np.nonzero(odd)[0])], bases=[7, 0xFFFFFFF0])
        forms = [(whole, 128, 0, 128, rest, 7), (whole, 128, 0, 128, rest, 0xFFFFFFF0, 1, 2)]
        out.append((f"{part}: W = bound = {w}", s, views, w, forms, [w, n]))
    n = (cap + 2 * step) // 128
    s, _ = cc.ladder_scene(["0" + "1" * 126 + "0"], [0] * n)
    views = cv._views([cv.A, cv.B], bases=[3, 4])
    out.append((f"{part}: loops", s, views, 0, [(n, 128, 1, 127, 0, 3), None], [128 * n, n]))
    return out


def _run_edge_scenes(ra, scenes):
    for name, s, views, hand in scenes:
        with TC._pipeline(ra, s, s["vertices"], s["indices"]) as p:
            _given_call(p, s, views, hand, name, async_=True)


def _run_cap_scenes(ra, scenes):
    import torch

    fill = T._i32(SENTINEL)
    for name, s, views, work_capacity, forms, head in scenes:
        want = [_closed_form_on_device(*f) if f is not None else None for f in forms]
        n_views = len(forms)
        with TC._pipeline(ra, s, s["vertices"], s["indices"]) as p:
            if want[1] is None:   # view B of "0" + "1" * 126 + "0": clusters 0 and 127 of every instance
                e = torch.arange(2 * s["n"], dtype=torch.int64, device=T._dev())
                w1 = torch.zeros((len(e), 4), dtype=torch.int64, device=T._dev())
                w1[:, 0], w1[:, 1], w1[:, 3] = e // 2 + views["bases"][1], 192 * 127 * (e % 2), 192
                want[1] = w1.to(torch.int32)
            stride = max(len(w) for w in want) + PAD
            uploaded = [None if b is None else TC._device_bitmap(b) for b in views["bitmaps"]]
            ptrs = [0 if t is None else t.data_ptr() for t in uploaded]
            frames = [make_frame(views["planes"][v], views["cams"][v], first_instance_base=views["bases"][v]) for v in range(n_views)]
            out = _Out(n_views, stride)
            p.list_clusters_views(frames, ptrs, make_lod_policy(views["mode"], views["switch"]), out.outputs(work_capacity=work_capacity, async_=True))
            p.wait()
            counts = np.array([len(w) for w in want], np.uint32)
            out.check_small(dict(entries=[np.zeros(0, cvlr.CLUSTER_ENTRY_DTYPE)] * n_views, counts=counts, args=cvlr.draw_args(counts, stride),
                                 stats=np.array(head + [len(w) for w in want], np.uint32)), name)
            for v in range(n_views):
                assert torch.equal(out.entries[v * stride: v * stride + len(want[v])], want[v]), (name, v, "entries")
                assert bool((out.entries[v * stride + len(want[v]): (v + 1) * stride] == fill).all()), (name, v, "entries behind the view's count were written")
            assert bool((out.entries[n_views * stride:] == fill).all()), (name, "behind the last view")
        del out, want


def _run_part(ra, sizes, part):
    if part in ("tiles", "members"):
        _run_edge_scenes(ra, _edge_scenes(sizes, part))
    else:
        _run_cap_scenes(ra, _cap_scenes(sizes, part))


@pytest.mark.parametrize("part", EDGE_PARTS)
def test_structural_edges(ra, tmp_path, part):
    sizes = _plan_sizes(tmp_path)
    item, tile = sizes["item_tile"], sizes["list_tile"]
    if part == "tiles":
        hands = {name: hand for name, _, _, hand in _edge_scenes(sizes, part)}
        assert {int(h["stats"][0]) for h in hands.values()} >= {63, 64, 65, item - 1, item, item + 1, tile - 1, tile, tile + 1}   # work items on every edge
        for at in (0, 7, 15):
            h = hands[f"a wave outside view {at}"]
            assert len(h["stats"]) == 18 and int(h["stats"][2 + at]) == 192 and {int(x) for i, x in enumerate(h["stats"][2:]) if i != at} == {256}
        assert hands["a wave outside every view"]["stats"].tolist() == [256, 256, 192, 0, 192]   # members by view 1's NULL bitmap, seen by nobody
        assert hands[f"a lone survivor at item {tile - 1}"]["stats"].tolist() == [3 * tile, 3 * tile, 1, 0, 1, 0]
    elif part != "members":
        step = item if part == "write grid cap" else tile
        cap = sizes["max_blocks"] * step
        scenes = _cap_scenes(sizes, part)
        assert [c[5][0] for c in scenes[:3]] == [cap - 1, cap, cap + 1] and scenes[3][5][0] > cap + step
    _run_part(ra, sizes, part)


_EDGE_CHILD = r'''
import os, sys
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
os.environ["MIP_LIBRARY"] = os.path.join(root, "renderer_amd", "lib", "libmi_instance_pipeline_dbg.so")
import renderer_amd
import test_gpu_cluster_views_list as TVL
TVL._run_part(renderer_amd, TVL._plan_sizes(sys.argv[2]), sys.argv[3])
print("CLUSTER-VIEWS-LIST-EDGES-OK")
'''


@pytest.mark.parametrize("part", EDGE_PARTS)
@pytest.mark.parametrize("tiles", ["reverse", "scramble"])
def test_structural_edges_in_any_dispatch_order(tiles, part, tmp_path):
    e = dict(os.environ, MIP_DEBUG_TILE_ORDER=tiles)
    out = subprocess.run([sys.executable, "-c", _EDGE_CHILD, ROOT, str(tmp_path), part], capture_output=True, text=True, timeout=600, env=e)
    assert out.returncode == 0 and "CLUSTER-VIEWS-LIST-EDGES-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ---- 4. overflow: per view, and who reports it; the scratch both several-view calls share ----

def test_overflow_rules(ra):
    s, vertices, indices, boxes = TV._scene(ra, 257)
    n_views = 3
    frusta, bases = cv.frusta(s["planes"], n_views), cv.view_bases(n_views)
    host_bm = TV._at_rest(s, frusta)
    full = cvlr.list_clusters_views(s, boxes, frusta, host_bm, bases, lr.DISTANCE, lr.PIN_SWITCH_SQ, 1 << 20)
    sv, w, members = [int(x) for x in full["stats"][2:]], int(full["stats"][0]), int(full["stats"][1])
    big = int(np.argmax(sv))
    assert min(sv) > 2 and sv[big] > min(sv) and w > max(sv)
    room = sv[big]
    policy = make_lod_policy(lr.DISTANCE, lr.PIN_SWITCH_SQ)
    frames = [make_frame(frusta[v], s["cam_pos"], first_instance_base=bases[v]) for v in range(n_views)]
    uploaded = [None if b is None else TC._device_bitmap(b) for b in host_bm]
    ptrs = [0 if t is None else t.data_ptr() for t in uploaded]

    def cut(stride):
        counts = np.array([min(x, stride) for x in sv], np.uint32)
        return dict(entries=[e[:stride] for e in full["all_entries"]], counts=counts, args=cvlr.draw_args(counts, stride), stats=full["stats"])

    def refused(stride):
        zero = np.zeros(n_views, np.uint32)
        return dict(entries=[full["entries"][0][:0]] * n_views, counts=zero, args=cvlr.draw_args(zero, stride), stats=np.array([w, members] + [0] * n_views, np.uint32))

    with TC._pipeline(ra, s, vertices, indices) as p:
        def overflows(out, async_, **kw):
            """MIP_ERR_CAPACITY once: from the call, or from mip_wait for an asynchronous one; then the context is clean again."""
            with pytest.raises(ra.MipError) as e:
                p.list_clusters_views(frames, ptrs, policy, out.outputs(async_=async_, **kw))
                p.wait()
            assert e.value.code == CAPACITY
            p.wait()

        for async_ in (False, True):
            for stride in (room - 1, 0):        # the largest view keeps its first `stride` entries, the others are complete where they fit
                out = _Out(n_views, room)
                overflows(out, async_, entry_stride=stride)
                out.check(cut(stride), f"entry_stride {stride} async={async_}", stride=stride)
                if stride:
                    assert min(sv) <= stride
            out = _Out(n_views, room)           # W - 1: nothing but the zero counts, {192, 0, 0, v x stride} and the refusal's stats
            overflows(out, async_, work_capacity=w - 1)
            out.check(refused(room), f"work_capacity W - 1 async={async_}")
            out = _Out(n_views, room)           # a fitting call on the same context is complete
            p.list_clusters_views(frames, ptrs, policy, out.outputs(entry_stride=room, work_capacity=w, async_=async_))
            p.wait()
            out.check(cut(room), f"fitting call async={async_}")

        # a synchronous mip_cull_clusters behind a frame slot between two of these calls: not charged with the asynchronous
        # overflow in front of it, its outputs unchanged; mip_wait then reports that overflow once
        plain_frame = make_frame(frusta[0], s["cam_pos"], first_instance_base=bases[0])
        ref = TC._Out(room)
        p.cull_clusters(plain_frame, ptrs[0], policy, ref.outputs())
        a, b, c = _Out(n_views, room), TC._Out(room), _Out(n_views, room)
        p.list_clusters_views(frames, ptrs, policy, a.outputs(entry_stride=1, async_=True))
        p.cull_clusters(plain_frame, ptrs[0], policy, b.outputs())                       # returns MIP_OK
        assert all(x.tobytes() == y.tobytes() for x, y in zip(b.result(), ref.result()))
        p.list_clusters_views(frames, ptrs, policy, c.outputs(async_=True))
        with pytest.raises(ra.MipError) as e:
            p.wait()
        assert e.value.code == CAPACITY
        a.check(cut(1), "the overflow in front of the plain call", stride=1)
        c.check(cut(room), "the fitting call behind it")
        p.wait()
        # ... and the other way round: an asynchronous mip_cull_clusters overflows, a synchronous call of this kind that fits is not charged
        a, b = TC._Out(room), _Out(n_views, room)
        p.cull_clusters(plain_frame, ptrs[0], policy, a.outputs(cmd_capacity=1, async_=True))
        p.list_clusters_views(frames, ptrs, policy, b.outputs())                         # returns MIP_OK
        b.check(cut(room), "a fitting synchronous call behind a plain overflow")
        with pytest.raises(ra.MipError) as e:
            p.wait()
        assert e.value.code == CAPACITY and int(a.result()[1][0]) == 1
        p.wait()


def test_both_several_view_calls_alternate_on_the_shared_scratch(ra):
    s, vertices, indices, boxes = TV._scene(ra, 1025)
    w = cv.KNOWN[1025]["W"]
    with TC._pipeline(ra, s, vertices, indices) as p:
        # the list call grows the scratch first, then the command call, then more views, the library's own bound, fewer again
        for k, (n_views, work_capacity) in enumerate(((1, w), (4, w), (16, 0), (2, w), (16, w), (3, 0))):
            what = f"alternating, V={n_views} work_capacity={work_capacity}"
            if k % 2 == 0:
                _views_call(p, s, boxes, n_views, lr.DISTANCE, lr.PIN_SWITCH_SQ, "list: " + what, kinds=("null",), equivalences=n_views == 3, work_capacity=work_capacity)
                TV._views_call(p, s, boxes, n_views, lr.DISTANCE, lr.PIN_SWITCH_SQ, "commands: " + what, kinds=("null",), plain_too=False, work_capacity=work_capacity)
            else:
                TV._views_call(p, s, boxes, n_views, lr.DISTANCE, lr.PIN_SWITCH_SQ, "commands: " + what, kinds=("null",), plain_too=False, work_capacity=work_capacity)
                _views_call(p, s, boxes, n_views, lr.DISTANCE, lr.PIN_SWITCH_SQ, "list: " + what, kinds=("null",), equivalences=False, work_capacity=work_capacity)


# ---- 5. every refusal writes nothing and leaves the context usable ----

def test_refusals_write_nothing(ra):
    name, s, views, hand = _CASES[0]
    n_views = len(views["planes"])
    with TC._pipeline(ra, s, s["vertices"], s["indices"]) as p:
        lib, ctx = p._lib, p._ctx
        out = _Out(n_views, 8)
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
            return lib.mip_list_clusters_views(context, addr(fr), addr(bm), k, addr(policy), addr(o) if o != "null" else None)

        bad_policy = make_lod_policy(views["mode"], views["switch"])
        bad_policy.switch_sq[1] = 1.0           # decreases
        wrong_size = make_lod_policy(views["mode"], views["switch"])
        wrong_size.struct_size = 24
        bad_mode = make_lod_policy(views["mode"], views["switch"])
        bad_mode.mode = 2
        refused = {
            "NULL ctx": call(context=None), "NULL frames": call(fr=None), "NULL visible_bitmaps": call(bm=None), "NULL policy": call(policy=None),
            "NULL out": call(o="null"), "NULL cluster_entries": call(outputs(cluster_entries=None)), "NULL entry_counts": call(outputs(entry_counts=None)),
            "struct_size 40": call(outputs(struct_size=40)), "struct_size 56": call(outputs(struct_size=56)),
            "unknown flags": call(outputs(flags=_lib.MIP_OUT_DEVICE | 0x10)), "host outputs": call(outputs(flags=0)),
            "misaligned entry_counts": call(outputs(entry_counts=out.counts.data_ptr() + 2)), "misaligned draw_args": call(outputs(draw_args=out.ar.data_ptr() + 1)),
            "misaligned stats": call(outputs(stats=out.st.data_ptr() + 2)),
            "entries 4-byte aligned only": call(outputs(cluster_entries=out.entries.data_ptr() + 4)),
            "entries 8-byte aligned only": call(outputs(cluster_entries=out.entries.data_ptr() + 8)),
            "zero views": call(k=0), "seventeen views": call(k=17),
            "n_views x entry_stride = 2^32": call(outputs(entry_stride=(1 << 32) // n_views)),
            "n_views x entry_stride above 2^32": call(outputs(entry_stride=0xFFFFFFFF)),
            "decreasing thresholds": call(policy=bad_policy), "policy struct_size": call(policy=wrong_size), "policy mode": call(policy=bad_mode),
        }
        assert n_views == 4 and all(rc == INVALID for rc in refused.values()), refused
        assert lib.mip_last_error(ctx) and out.untouched()
        assert call(outputs(entry_stride=8)) == 0 and not out.untouched()     # the same arguments, nothing wrong with them: taken
        _given_call(p, s, views, hand, name + " after the refusals")     # the context is usable
    # no instances; no cluster table; a stale one: not ready, nothing written
    fresh = _Out(n_views, 8)
    frames = [make_frame(views["planes"][v], views["cams"][v]) for v in range(n_views)]
    with ra.InstancePipeline(max_instances=4, max_meshes=len(s["meshes"])) as p:
        p.set_mesh_table(s["meshes"])
        p.set_geometry(s["vertices"], s["indices"])
        p.build_clusters()
        with pytest.raises(ra.MipError) as e:
            p.list_clusters_views(frames, [0] * n_views, policy, fresh.outputs())
        assert e.value.code == NOT_READY and fresh.untouched()
    with T._pipeline(ra, s) as p:
        p.set_geometry(s["vertices"], s["indices"])
        with pytest.raises(ra.MipError) as e:                    # no table yet
            p.list_clusters_views(frames, [0] * n_views, policy, fresh.outputs())
        assert e.value.code == NOT_READY and fresh.untouched()
        p.build_clusters()
        p.set_geometry(s["vertices"], s["indices"])             # stale again
        with pytest.raises(ra.MipError) as e:
            p.list_clusters_views(frames, [0] * n_views, policy, fresh.outputs())
        assert e.value.code == NOT_READY and fresh.untouched()
        p.build_clusters()
        _given_call(p, s, views, hand, name + " after the rebuild")
