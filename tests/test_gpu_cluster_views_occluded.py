"""mip_list_clusters_views_occluded on the GPU (include/mi_instance_pipeline.h): every byte of every output buffer — the
entries, the counts, the draw arguments, the stats and `hidden`, each whole, sentinel-filled before the call, with sentinel rows
in front of and behind it — against the numpy restatement (tests/cluster_views_occluded_restatement.py), against the
hand-written scenes (tests/cluster_view_occluded_cases.py), against one mip_list_clusters call per view under the view's
pyramid on the same context (equivalence (a) of the header), with no pyramid at all against mip_list_clusters_views byte for
byte (b), and as a subsequence of that call's lists with survivors + hidden = its survivors (c); ladders on the structural
edges of the cull kernel, also with reversed and scrambled tiles under the diagnostic library; pyramids built for the next run
on another stream with no wait; the memset of `hidden`; the scratch the several-view calls share; both overflow rules per view
and who reports them; every refusal. Not reference behaviour: parity is with the restatement."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_restatement as cr
import cluster_view_cases as cv
import cluster_view_occluded_cases as cvoc
import cluster_views_occluded_restatement as cvor
import lod_restatement as lr
import occlusion_restatement as orr
import test_gpu_batch as T
import test_gpu_batch_lods as TL
import test_gpu_cluster_list as TLST
import test_gpu_cluster_phases as TPH
import test_gpu_cluster_views as TV
import test_gpu_cluster_views_list as TVL
import test_gpu_clusters as TC
from renderer_amd import _lib
from renderer_amd.pipeline import make_cluster_view_occluded_list_outputs, make_frame, make_lod_policy, make_occlusion

pytestmark = pytest.mark.gpu
ROOT = TC.ROOT
SENTINEL = T.SENTINEL
PAD = 3      # sentinel rows / words in front of and behind every buffer
ra = T.ra    # the module's library fixture
NOT_READY, INVALID, CAPACITY = -6, -1, -4
MODES = (lr.DISTANCE, lr.RELATIVE)
WALLS = (0, 16, 32)


class _Out:
    """Device outputs of mip_list_clusters_views_occluded, every word a sentinel: n_views x stride entries, the counts, the draw
    arguments, the stats and hidden, PAD rows / words nobody may touch in front of and behind each."""

    def __init__(self, n_views, stride, args=True, stats=True, hidden=True):
        import torch

        fill = T._i32(SENTINEL)
        self.n_views, self.stride, self.args, self.stats, self.hidden = n_views, int(stride), args, stats, hidden
        new = lambda *shape: torch.full(shape, fill, dtype=torch.int32, device=T._dev())   # noqa: E731
        self.entries = new(PAD + n_views * self.stride + PAD, 4)
        self.counts, self.ar, self.st, self.hid = new(PAD + n_views + PAD), new(PAD + 4 * n_views + PAD), new(PAD + 2 + n_views + PAD), new(PAD + n_views + PAD)
        torch.cuda.synchronize()

    def outputs(self, entry_stride=None, work_capacity=0, async_=False):
        at = lambda t, on=True: t.data_ptr() + PAD * t.stride(0) * 4 if on else 0   # noqa: E731
        return make_cluster_view_occluded_list_outputs(at(self.entries), self.stride if entry_stride is None else entry_stride, at(self.counts),
                                                       at(self.ar, self.args), at(self.st, self.stats), at(self.hid, self.hidden),
                                                       work_capacity=work_capacity, async_=async_)

    def result(self):
        import torch

        torch.cuda.synchronize()
        u = lambda t: t.cpu().numpy().view(np.uint32)   # noqa: E731
        return dict(entries=u(self.entries), counts=u(self.counts), args=u(self.ar), stats=u(self.st), hidden=u(self.hid))

    def check(self, want, what, stride=None):
        """Every buffer whole: what the call owes under `stride` (default: the room of a view), the sentinel everywhere else.
        Returns the buffers without their front rows."""
        stride = self.stride if stride is None else int(stride)
        got = self.result()
        full = cvor.fill_outputs(want, self.n_views, stride, SENTINEL, PAD, self.args, self.stats, self.hidden)
        for k in ("counts", "args", "stats", "hidden"):
            assert (got[k][:PAD] == SENTINEL).all(), (what, k, "written in front of the buffer")
            assert got[k][PAD:].tolist() == full[k].tolist(), (what, k, got[k][PAD:].tolist(), full[k].tolist())
        used = self.n_views * stride
        assert (got["entries"][:PAD] == SENTINEL).all(), (what, "written in front of the entries")
        assert got["entries"][PAD: PAD + used].tobytes() == full["entries"][:used].tobytes(), (what, "entries")
        assert (got["entries"][PAD + used:] == SENTINEL).all(), (what, "behind the last view's range")
        return {k: v[PAD:] for k, v in got.items()}

    def untouched(self):
        got = self.result()
        return all((got[k] == SENTINEL).all() for k in got)


class _Images:
    """Depth images on the device and room for their pyramids, by key; build() enqueues every mip_build_depth_pyramid,
    asynchronously; occ(key, pv) is a MipOcclusion over the key's pyramid."""

    def __init__(self, ra, depths):
        self.depths = dict(depths)
        self.pyramids = {k: TPH._Pyramid(ra, np.ascontiguousarray(d, np.float32), np.zeros(16, np.float32)) for k, d in self.depths.items()}

    def build(self, ra, p):
        for q in self.pyramids.values():
            q.build(ra, p)

    def occ(self, key, pv):
        d = self.depths[key]
        return make_occlusion(d.shape[1], d.shape[0], self.pyramids[key].pyr.data_ptr(), pv)


def _one_list_per_view(p, planes, cam0, bases, ptrs, occs, n, policy, stride, got, what):
    """Equivalence (a): one mip_list_clusters per view on the same context — frames[v] with frames[0]'s camera, the view's own
    bitmap (a full one where the entry is NULL), the view's own pyramid, entry_capacity = entry_stride."""
    ones = TC._device_bitmap(np.full((max(n, 1) + 31) // 32, 0xFFFFFFFF, np.uint32))
    for v in range(len(planes)):
        o = TLST._Out(stride)
        p.list_clusters(make_frame(planes[v], cam0, first_instance_base=bases[v]), ptrs[v] or ones.data_ptr(), policy, o.outputs(entry_capacity=stride),
                        occlusion=occs[v])
        entries, scal = o.result()
        count = int(scal[0])
        assert int(got["counts"][v]) == count, (what, v, "entry_count of mip_list_clusters")
        assert got["entries"][v * stride: v * stride + count].tobytes() == entries[:count].tobytes(), (what, v, "entries of mip_list_clusters")
        assert int(got["stats"][2 + v]) == int(scal[6]), (what, v, "survivors of mip_list_clusters")


def _against_the_plain_call(p, frames, ptrs, policy, n_views, stride, got, what, work_capacity=0, again=True):
    """(b) and (c) on the same context: with every occs[v] NULL every buffer is mip_list_clusters_views', byte for byte, and
    hidden is zero; view v's list is a subsequence of that call's, survivors_v + hidden[v] = its survivors_v."""
    plain = TVL._Out(n_views, stride)
    p.list_clusters_views(frames, ptrs, policy, plain.outputs(work_capacity=work_capacity))
    r = plain.result()
    assert got["stats"][:2].tolist() == r["stats"][:2].tolist(), (what, "W and members")
    for v in range(n_views):
        mine = got["entries"][v * stride: v * stride + int(got["counts"][v])]
        theirs = r["entries"][v * stride: v * stride + int(r["counts"][v])]
        it = iter(x.tobytes() for x in theirs)
        assert all(any(x.tobytes() == y for y in it) for x in mine), (what, v, "not a subsequence of mip_list_clusters_views' list")
        assert int(got["stats"][2 + v]) + int(got["hidden"][v]) == int(r["stats"][2 + v]), (what, v, "survivors + hidden")
    if again:
        bare = _Out(n_views, stride)
        p.list_clusters_views_occluded(frames, ptrs, [None] * n_views, policy, bare.outputs(work_capacity=work_capacity))
        b = bare.result()
        for k, theirs in (("entries", r["entries"]), ("counts", r["counts"]), ("args", r["args"]), ("stats", r["stats"])):
            assert b[k][PAD: PAD + len(theirs)].tobytes() == theirs.tobytes(), (what, k, "no pyramid at all: not mip_list_clusters_views' bytes")
        assert b["hidden"][PAD: PAD + n_views].tolist() == [0] * n_views and (b["hidden"][PAD + n_views:] == SENTINEL).all(), (what, "hidden without a pyramid")


# ---- 1. every hand-written scene, against the hand-written bytes ----

_CASES = cvoc.cases()


def _hand_want(hand, stride):
    counts = np.array([min(len(e), stride) for e in hand["entries"]], np.uint32)
    return dict(entries=[e[:stride] for e in hand["entries"]], counts=counts, args=cvor.cvlr.draw_args(counts, stride), stats=hand["stats"], hidden=hand["hidden"])


def _given_call(ra, p, s, views, kinds, hand, what, async_=False, work_capacity=0, stride=None, args=True, stats=True, hidden=True, equivalences=False):
    """The pyramids built asynchronously, then — with no wait — the call over uploaded bitmaps (at rest); the outputs whole
    against `hand`."""
    import torch

    n_views = len(kinds)
    uploaded = [None if b is None else TC._device_bitmap(b) for b in views["bitmaps"]]
    ptrs = [0 if t is None else t.data_ptr() for t in uploaded]
    frames = [make_frame(views["planes"][v], views["cams"][v], first_instance_base=views["bases"][v]) for v in range(n_views)]
    images = _Images(ra, {k: cvoc.OCCLUSIONS[k][1] for k in set(kinds) if k is not None})
    occs = [None if k is None else images.occ(k, cvoc.OCCLUSIONS[k][0]) for k in kinds]
    stride = max(len(e) for e in hand["entries"]) + PAD if stride is None else stride
    out = _Out(n_views, stride, args, stats, hidden)
    policy = make_lod_policy(views["mode"], views["switch"])
    torch.cuda.synchronize()
    images.build(ra, p)
    p.list_clusters_views_occluded(frames, ptrs, occs, policy, out.outputs(work_capacity=work_capacity, async_=async_))
    if async_:
        p.wait()
    got = out.check(_hand_want(hand, stride), what)
    if equivalences:
        _one_list_per_view(p, views["planes"], views["cams"][0], views["bases"], ptrs, occs, s["n"], policy, stride, got, what)
        _against_the_plain_call(p, frames, ptrs, policy, n_views, stride, got, what)
    return out


@pytest.mark.parametrize("name,s,views,kinds,hand", _CASES, ids=[c[0] for c in _CASES])
def test_hand_cases(ra, name, s, views, kinds, hand):
    with TC._pipeline(ra, s, s["vertices"], s["indices"]) as p:
        _given_call(ra, p, s, views, kinds, hand, name, stride=16, equivalences=True)      # room for the plain call's list of the same views
        _given_call(ra, p, s, views, kinds, hand, name + ", asynchronous", async_=True)
        _given_call(ra, p, s, views, kinds, hand, name + ", no draw_args, no hidden", args=False, hidden=False)
        _given_call(ra, p, s, views, kinds, hand, name + ", no stats", stats=False, async_=True)


# ---- 2. the restatement and the three equivalences over config 3 ----

def _wall_images(ra):
    return _Images(ra, {c: cvoc.wall(c) for c in WALLS})


def _views_call(ra, p, s, boxes, n_views, mode, sw, what, kinds=("culled", "shared", "null"), equivalences=True, work_capacity=0, missing=(), images=None):
    """mip_run_views over the views that take a culled bitmap and the pyramid builds, then — with no wait — the call over all
    views. View v's bitmap is kinds[v % len(kinds)] (as in test_gpu_cluster_views_list), its planes the scene's turned, its pv
    the default pv turned the same way, its image the wall at (0, 16, 32)[v % 3]: three pyramids shared by the views, each
    under its own pv; no pyramid for the views in `missing`. The outputs whole against the restatement, then the equivalences
    on the same context."""
    import torch

    n = s["n"]
    cams, frusta, bases = cv.view_cams(s, n_views), cv.frusta(s["planes"], n_views), cv.view_bases(n_views, n)
    pvs = cvor.view_pvs(ra.scene.default_pv(), n_views)
    frames = [make_frame(frusta[v], cams[v], first_instance_base=bases[v]) for v in range(n_views)]
    kind = [kinds[v % len(kinds)] for v in range(n_views)]
    words = (max(n, 1) + 31) // 32
    culled = [v for v in range(n_views) if kind[v] == "culled"]
    bitmaps = torch.zeros((n_views, words), dtype=torch.int32, device=T._dev())
    draw = torch.zeros((max(len(culled), 1), max(n, 1), 5), dtype=torch.int32, device=T._dev())
    scal = torch.zeros((n_views, 2), dtype=torch.int32, device=T._dev())
    ptrs = [bitmaps[v].data_ptr() if kind[v] == "culled" else bitmaps[0].data_ptr() if kind[v] == "shared" else 0 for v in range(n_views)]
    images = images or _wall_images(ra)
    occs = [None if v in missing else images.occ(WALLS[v % 3], pvs[v]) for v in range(n_views)]
    stride = max(n, 1) * int(cr.cluster_table(s["meshes"])["C"].max()) + PAD     # every cluster of every instance fits, and PAD rows
    out = _Out(n_views, stride)
    policy = make_lod_policy(mode, sw)
    torch.cuda.synchronize()
    if n and culled:
        prepared = [p.prepare_outputs(visible_bitmap=bitmaps[v].data_ptr(), draw_cmds=draw[k].data_ptr(), draw_count=scal[v].data_ptr(),
                                      draw_index_total=scal[v].data_ptr() + 4) for k, v in enumerate(culled)]
        p.run_views([frames[v] for v in culled], prepared)          # asynchronous: prepare_outputs sets MIP_OUT_ASYNC
    images.build(ra, p)
    p.list_clusters_views_occluded(frames, ptrs, occs, policy, out.outputs(work_capacity=work_capacity, async_=True))
    p.wait()
    host = bitmaps.cpu().numpy().view(np.uint32)
    host_bm = [None if kind[v] == "null" else host[0] if kind[v] == "shared" else host[v] for v in range(n_views)]
    host_occs = [None if v in missing else dict(pv=pvs[v], levels=orr.pyramid_levels(cvoc.wall(WALLS[v % 3])), width=64, height=32) for v in range(n_views)]
    want = cvor.list_clusters_views_occluded(s, boxes, frusta, host_bm, host_occs, bases, mode, sw, stride, work_capacity, cam_pos=cams[0])
    assert want["status"] == 0, what
    got = out.check(want, what)
    if equivalences:
        _one_list_per_view(p, frusta, cams[0], bases, ptrs, occs, n, policy, stride, got, what)
        _against_the_plain_call(p, frames, ptrs, policy, n_views, stride, got, what, work_capacity)
    return want


@pytest.mark.parametrize("n", [0, 1, 257, 4097])
@pytest.mark.parametrize("n_views", [1, 2, 5, 16])
def test_restatement_and_the_three_equivalences_over_config_3(ra, n, n_views):
    s, vertices, indices, boxes = TV._scene(ra, n)
    with TC._pipeline(ra, s, vertices, indices) as p:
        images = _wall_images(ra)
        for mode in MODES:
            want = _views_call(ra, p, s, boxes, n_views, mode, TL._metric_thresholds(s, mode), f"n={n} V={n_views} mode={mode}", images=images)
            if n == 0:
                assert (want["stats"] == 0).all() and (want["counts"] == 0).all() and (want["hidden"] == 0).all() and (want["args"][:, 0] == 192).all()
            if n >= 257:
                assert int(want["stats"][0]) > n and max(int(x) for x in want["stats"][2:]) > 0 and int(want["hidden"].sum()) > 0
        if n == 257 and n_views == 5:   # the answers pinned on the CPU: full bitmaps, the pin policy; and NULL in the first, a middle, the last slot
            known = [(2581, 970, 1428, 1628), (3425, 1572, 2200, 1853), (2581, 1628, 1428, 970), (2539, 1353, 870, 1206), (255, 84, 86, 171)]
            want = _views_call(ra, p, s, boxes, n_views, lr.DISTANCE, lr.PIN_SWITCH_SQ, "n=257 known answers", kinds=("null",), equivalences=False, images=images)
            assert want["stats"].tolist() == [9917, 257] + [known[v][1 + v % 3] for v in range(5)]
            assert want["hidden"].tolist() == [known[v][0] - known[v][1 + v % 3] for v in range(5)]
            for missing in ((0,), (2,), (4,), (0, 2, 4)):
                mixed = _views_call(ra, p, s, boxes, n_views, lr.DISTANCE, lr.PIN_SWITCH_SQ, f"n=257 no pyramid in {missing}", kinds=("null",), equivalences=False,
                                    missing=missing, images=images)
                assert mixed["stats"][2:].tolist() == [known[v][0] if v in missing else known[v][1 + v % 3] for v in range(5)]


# ---- 3. ladders on the structural edges of the cull kernel ----

def _filled(w, specs_of):
    """W = w work items: instances of "10101010" and one shorter one."""
    whole, rest = divmod(w, 8)
    n = whole + (1 if rest else 0)
    return cvoc.occluded_ladder(["10" * 4] + ([("10" * 4)[:rest]] if rest else []), [0] * whole + ([1] if rest else []), specs_of(n))


def _edge_scenes(sizes):
    """[(name, scene, views, kinds, hand)]: W one below, at and one above a survive word and an item tile under five views with
    different frusta, pyramids and bitmaps; a wave in which no lane passes the planes of the one view that has a pyramid; a
    wave in which exactly lane 0 passes them, and one in which exactly lane 63 does — each with a pyramid that hides that lane
    and with one that does not."""
    item = sizes["item_tile"]
    out = []
    every_second = lambda n: np.arange(n) % 2 == 0   # noqa: E731
    for edge in (64, item):
        for w in (edge - 1, edge, edge + 1):
            out.append((f"W={w}", *_filled(w, lambda n: [("C", "in", None, 1), ("C", None, every_second(n), 2), ("A", "out", None, 0xFFFFFFFF - 5), ("B", "all", None, 4),
                                                         ("C", "none", every_second(n), 9)])))
    # 256 one-cluster instances, four waves of one round: mesh 0 is one INSIDE cluster, mesh 1 one OUTSIDE cluster; frustum A
    # passes the INSIDE ones alone. The second wave (instances 64 .. 127) holds no INSIDE instance, or one in lane 0, or in lane 63
    for name, inside in (("no lane of a wave passes", ()), ("exactly lane 0 passes", (64,)), ("exactly lane 63 passes", (127,))):
        inst = np.zeros(256, np.int64)
        inst[64:128] = 1
        inst[list(inside)] = 0
        for kind in ("in", "out"):          # "in" hides the lanes that passed, "out" none of them
            out.append((f"{name} the planes of the view with the pyramid ({kind})",
                        *cvoc.occluded_ladder(["1", "0"], inst.tolist(), [("C", None, None, 10), ("A", kind, None, 300), ("B", None, None, 20)])))
    # ... and every instance OUTSIDE but one lane: passed is a single bit in the whole grid
    for lane in (0, 63):
        inst = np.ones(128, np.int64)
        inst[64 + lane] = 0
        out.append((f"one lane in the grid passes, lane {lane}", *cvoc.occluded_ladder(["1", "0"], inst.tolist(), [("A", "in", None, 7), ("A", "none", None, 8)])))
    return out


def _run_edge_scenes(ra, sizes):
    for name, s, views, kinds, hand in _edge_scenes(sizes):
        with TC._pipeline(ra, s, s["vertices"], s["indices"]) as p:
            _given_call(ra, p, s, views, kinds, hand, name, async_=True)


def test_structural_edges(ra, tmp_path):
    sizes = TVL._plan_sizes(tmp_path)
    item = sizes["item_tile"]
    hands = {name: hand for name, _, _, _, hand in _edge_scenes(sizes)}
    assert {int(h["stats"][0]) for h in hands.values()} >= {63, 64, 65, item - 1, item, item + 1}
    assert hands["W=64"]["hidden"].tolist() == [32, 0, 0, 32, 0] and hands["W=64"]["stats"].tolist() == [64, 8, 32, 32, 32, 0, 32]
    none = "no lane of a wave passes the planes of the view with the pyramid"
    assert hands[none + " (in)"]["hidden"].tolist() == [0, 192, 0] and hands[none + " (out)"]["stats"].tolist() == [256, 256, 256, 192, 64]
    assert hands["exactly lane 0 passes the planes of the view with the pyramid (in)"]["hidden"].tolist() == [0, 193, 0]
    assert hands["one lane in the grid passes, lane 63"]["hidden"].tolist() == [1, 0] and hands["one lane in the grid passes, lane 63"]["stats"].tolist() == [128, 128, 0, 1]
    _run_edge_scenes(ra, sizes)


_EDGE_CHILD = r'''
import os, sys
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
os.environ["MIP_LIBRARY"] = os.path.join(root, "renderer_amd", "lib", "libmi_instance_pipeline_dbg.so")
import renderer_amd
import test_gpu_cluster_views_list as TVL
import test_gpu_cluster_views_occluded as TVO
TVO._run_edge_scenes(renderer_amd, TVL._plan_sizes(sys.argv[2]))
print("CLUSTER-VIEWS-OCCLUDED-EDGES-OK")
'''


@pytest.mark.parametrize("tiles", ["reverse", "scramble"])
def test_structural_edges_in_any_dispatch_order(tiles, tmp_path):
    e = dict(os.environ, MIP_DEBUG_TILE_ORDER=tiles)
    out = subprocess.run([sys.executable, "-c", _EDGE_CHILD, ROOT, str(tmp_path)], capture_output=True, text=True, timeout=600, env=e)
    assert out.returncode == 0 and "CLUSTER-VIEWS-OCCLUDED-EDGES-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


@pytest.mark.parametrize("packed", ["0", "1"])
def test_both_cull_kernels_with_and_without_a_pyramid(ra, tmp_path, monkeypatch, packed):
    """The library's tuning switches, read per call: the simple-loop kernel and the packed one, each also forced to run when no
    view has a pyramid (by default the plain several-view cull kernel runs then). The hand-written scenes with the
    equivalences — (b) is the all-NULL call byte for byte —, the structural edges and config 3 under sixteen views."""
    monkeypatch.setenv("MIP_TUNE_VIEWS_OCCLUDED_PACKED", packed)
    monkeypatch.setenv("MIP_TUNE_VIEWS_OCCLUDED_ALWAYS", "1")
    for name, s, views, kinds, hand in _CASES:
        with TC._pipeline(ra, s, s["vertices"], s["indices"]) as p:
            _given_call(ra, p, s, views, kinds, hand, f"{name}, packed={packed}", stride=16, equivalences=True)
    _run_edge_scenes(ra, TVL._plan_sizes(tmp_path))
    s, vertices, indices, boxes = TV._scene(ra, 257)
    with TC._pipeline(ra, s, vertices, indices) as p:
        _views_call(ra, p, s, boxes, 16, lr.DISTANCE, lr.PIN_SWITCH_SQ, f"n=257 V=16 packed={packed}")


# ---- 4. pyramids on another stream; the memset of hidden; the shared scratch ----

def _at_rest_call(s, boxes, n_views, stride, work_capacity=0, missing=()):
    """The views of config 3 over NULL bitmaps under the pin policy: (frames, ptrs, pvs, restatement)."""
    frusta, bases = cv.frusta(s["planes"], n_views), cv.view_bases(n_views, s["n"])
    pvs = cvor.view_pvs(np.asarray(s["pv"], np.float32), n_views)
    frames = [make_frame(frusta[v], s["cam_pos"], first_instance_base=bases[v]) for v in range(n_views)]
    host_occs = [None if v in missing else dict(pv=pvs[v], levels=orr.pyramid_levels(cvoc.wall(WALLS[v % 3])), width=64, height=32) for v in range(n_views)]
    want = cvor.list_clusters_views_occluded(s, boxes, frusta, [None] * n_views, host_occs, bases, lr.DISTANCE, lr.PIN_SWITCH_SQ, stride, work_capacity)
    return frames, [0] * n_views, pvs, want


def test_two_frames_in_flight_sixteen_pyramids_and_no_wait(ra):
    """After one mip_run the next run's slot is not slot 0: mip_build_depth_pyramid enqueues on that slot's stream, the call on
    the first stream. Sixteen pyramids of their own are built asynchronously, then the call, with no wait in between."""
    import torch

    s, vertices, indices, boxes = TV._scene(ra, 257)
    s = dict(s, pv=ra.scene.default_pv())
    n_views, stride = 16, 3500
    frames, ptrs, pvs, want = _at_rest_call(s, boxes, n_views, stride)
    assert want["status"] == 0 and min(int(h) for h in want["hidden"]) > 0
    policy = make_lod_policy(lr.DISTANCE, lr.PIN_SWITCH_SQ)
    with TC._pipeline(ra, s, vertices, indices, frames_in_flight=2) as p:
        fr = T._Frame(257)
        images = _Images(ra, {v: cvoc.wall(WALLS[v % 3]) for v in range(n_views)})
        occs = [images.occ(v, pvs[v]) for v in range(n_views)]
        torch.cuda.synchronize()
        for round_ in range(3):                      # the slots alternate: the pyramids sit on slot 1's stream, then slot 0's, then slot 1's
            out = _Out(n_views, stride)
            p.run_device(frames[0], async_=True, **fr.kwargs())
            images.build(ra, p)
            p.list_clusters_views_occluded(frames, ptrs, occs, policy, out.outputs(async_=True))
            p.wait()
            out.check(want, f"sixteen pyramids, round {round_}")
            for q in images.pyramids.values():       # the next round builds them again: a stale pyramid would hide nothing
                q.pyr.fill_(T._i32(0x3F800000))      # 1.0 everywhere
            torch.cuda.synchronize()


def test_hidden_is_cleared_by_every_call_and_not_touched_when_null(ra):
    import torch

    s, vertices, indices, boxes = TV._scene(ra, 257)
    s = dict(s, pv=ra.scene.default_pv())
    n_views, stride = 5, 3500
    frames, ptrs, pvs, want = _at_rest_call(s, boxes, n_views, stride)
    policy = make_lod_policy(lr.DISTANCE, lr.PIN_SWITCH_SQ)
    with TC._pipeline(ra, s, vertices, indices) as p:
        images = _wall_images(ra)
        occs = [images.occ(WALLS[v % 3], pvs[v]) for v in range(n_views)]
        a, b = _Out(n_views, stride), _Out(n_views, stride, hidden=False)
        torch.cuda.synchronize()
        images.build(ra, p)
        # given, NULL, given into the SAME words: without the memset the third call would leave twice the counts
        p.list_clusters_views_occluded(frames, ptrs, occs, policy, a.outputs(async_=True))
        p.list_clusters_views_occluded(frames, ptrs, occs, policy, b.outputs(async_=True))
        p.list_clusters_views_occluded(frames, ptrs, occs, policy, a.outputs(async_=True))
        p.wait()
        a.check(want, "hidden given twice")
        b.check(want, "hidden NULL in between")
        assert min(int(h) for h in want["hidden"]) > 0
        # fewer views into the same words: the words behind n_views stay as they are
        frames3, ptrs3, pvs3, want3 = _at_rest_call(s, boxes, 3, stride)
        p.list_clusters_views_occluded(frames3, ptrs3, occs[:3], policy, a.outputs())
        got = a.result()
        assert got["hidden"][PAD: PAD + 5].tolist() == want3["hidden"].tolist() + want["hidden"][3:].tolist()


def test_the_several_view_calls_alternate_on_the_shared_scratch(ra):
    s, vertices, indices, boxes = TV._scene(ra, 1025)
    w = cv.KNOWN[1025]["W"]
    with TC._pipeline(ra, s, vertices, indices) as p:
        images = _wall_images(ra)
        # this call grows the scratch first, then the list call, then the command call; more views, the library's own bound, fewer again
        for k, (n_views, work_capacity) in enumerate(((1, w), (4, w), (16, 0), (2, w), (16, w), (3, 0))):
            what = f"alternating, V={n_views} work_capacity={work_capacity}"
            mine = lambda: _views_call(ra, p, s, boxes, n_views, lr.DISTANCE, lr.PIN_SWITCH_SQ, "occluded: " + what, kinds=("null",),   # noqa: E731
                                       equivalences=n_views == 3, work_capacity=work_capacity, images=images)
            lists = lambda: TVL._views_call(p, s, boxes, n_views, lr.DISTANCE, lr.PIN_SWITCH_SQ, "list: " + what, kinds=("null",), equivalences=False,   # noqa: E731
                                            work_capacity=work_capacity)
            cmds = lambda: TV._views_call(p, s, boxes, n_views, lr.DISTANCE, lr.PIN_SWITCH_SQ, "commands: " + what, kinds=("null",), plain_too=False,   # noqa: E731
                                          work_capacity=work_capacity)
            for call in ((mine, lists, cmds), (cmds, mine, lists), (lists, cmds, mine))[k % 3]:
                call()


# ---- 5. overflow: per view, and who reports it ----

def test_overflow_rules(ra):
    import torch

    s, vertices, indices, boxes = TV._scene(ra, 257)
    s = dict(s, pv=ra.scene.default_pv())
    n_views = 3
    frames, ptrs, pvs, full = _at_rest_call(s, boxes, n_views, 1 << 20)
    sv, w, members = [int(x) for x in full["stats"][2:]], int(full["stats"][0]), int(full["stats"][1])
    big = int(np.argmax(sv))
    assert min(sv) > 2 and sv[big] > min(sv) and w > max(sv) and min(int(h) for h in full["hidden"]) > 0
    room = sv[big]
    policy = make_lod_policy(lr.DISTANCE, lr.PIN_SWITCH_SQ)

    def cut(stride):
        counts = np.array([min(x, stride) for x in sv], np.uint32)
        return dict(entries=[e[:stride] for e in full["all_entries"]], counts=counts, args=cvor.cvlr.draw_args(counts, stride), stats=full["stats"], hidden=full["hidden"])

    def refused(stride):
        zero = np.zeros(n_views, np.uint32)
        return dict(entries=[full["entries"][0][:0]] * n_views, counts=zero, args=cvor.cvlr.draw_args(zero, stride), stats=np.array([w, members] + [0] * n_views, np.uint32),
                    hidden=zero)

    with TC._pipeline(ra, s, vertices, indices) as p:
        images = _wall_images(ra)
        occs = [images.occ(WALLS[v % 3], pvs[v]) for v in range(n_views)]
        torch.cuda.synchronize()
        images.build(ra, p)
        p.wait()

        def overflows(out, async_, **kw):
            """MIP_ERR_CAPACITY once: from the call, or from mip_wait for an asynchronous one; then the context is clean again."""
            with pytest.raises(ra.MipError) as e:
                p.list_clusters_views_occluded(frames, ptrs, occs, policy, out.outputs(async_=async_, **kw))
                p.wait()
            assert e.value.code == CAPACITY
            p.wait()

        for async_ in (False, True):
            for stride in (room - 1, 0):        # the largest view keeps its first `stride` entries, the others are complete where they fit; hidden is true
                out = _Out(n_views, room)
                overflows(out, async_, entry_stride=stride)
                out.check(cut(stride), f"entry_stride {stride} async={async_}", stride=stride)
                if stride:
                    assert min(sv) <= stride
            out = _Out(n_views, room)           # W - 1: zero counts, {192, 0, 0, v x stride}, the refusal's stats, hidden all zero
            overflows(out, async_, work_capacity=w - 1)
            out.check(refused(room), f"work_capacity W - 1 async={async_}")
            out = _Out(n_views, room)           # a fitting call on the same context is complete
            p.list_clusters_views_occluded(frames, ptrs, occs, policy, out.outputs(entry_stride=room, work_capacity=w, async_=async_))
            p.wait()
            out.check(cut(room), f"fitting call async={async_}")

        # a synchronous mip_cull_clusters behind a frame slot between two of these calls: charged with nothing, its outputs
        # unchanged; mip_wait then reports the overflow in front of it once
        plain_frame = make_frame(cv.frusta(s["planes"], 1)[0], s["cam_pos"], first_instance_base=3)
        ones = TC._device_bitmap(np.full((257 + 31) // 32, 0xFFFFFFFF, np.uint32))
        ref = TC._Out(room)
        p.cull_clusters(plain_frame, ones.data_ptr(), policy, ref.outputs())
        a, b, c = _Out(n_views, room), TC._Out(room), _Out(n_views, room)
        p.list_clusters_views_occluded(frames, ptrs, occs, policy, a.outputs(entry_stride=1, async_=True))
        p.cull_clusters(plain_frame, ones.data_ptr(), policy, b.outputs())                       # returns MIP_OK
        assert all(x.tobytes() == y.tobytes() for x, y in zip(b.result(), ref.result()))
        p.list_clusters_views_occluded(frames, ptrs, occs, policy, c.outputs(async_=True))
        with pytest.raises(ra.MipError) as e:
            p.wait()
        assert e.value.code == CAPACITY
        a.check(cut(1), "the overflow in front of the plain call", stride=1)
        c.check(cut(room), "the fitting call behind it")
        p.wait()
        # ... and the other way round: an asynchronous mip_cull_clusters overflows, a synchronous call of this kind that fits is not charged
        a, b = TC._Out(room), _Out(n_views, room)
        p.cull_clusters(plain_frame, ones.data_ptr(), policy, a.outputs(cmd_capacity=1, async_=True))
        p.list_clusters_views_occluded(frames, ptrs, occs, policy, b.outputs())                  # returns MIP_OK
        b.check(cut(room), "a fitting synchronous call behind a plain overflow")
        with pytest.raises(ra.MipError) as e:
            p.wait()
        assert e.value.code == CAPACITY and int(a.result()[1][0]) == 1
        p.wait()


# ---- 6. every refusal writes nothing and leaves the context usable ----

def test_refusals_write_nothing(ra):
    import torch

    name, s, views, kinds, hand = _CASES[0]
    n_views = len(kinds)
    with TC._pipeline(ra, s, s["vertices"], s["indices"]) as p:
        lib, ctx = p._lib, p._ctx
        out = _Out(n_views, 8)
        frames = (_lib.MipFrame * n_views)()
        made = [make_frame(views["planes"][v], views["cams"][v], first_instance_base=views["bases"][v]) for v in range(n_views)]   # alive while copied
        for v in range(n_views):
            C.memmove(C.addressof(frames[v]), C.addressof(made[v]), C.sizeof(_lib.MipFrame))
        bitmaps = (C.c_void_p * n_views)(*[None] * n_views)
        images = _Images(ra, {k: cvoc.OCCLUSIONS[k][1] for k in set(kinds) if k is not None})
        torch.cuda.synchronize()
        images.build(ra, p)
        p.wait()
        policy = make_lod_policy(views["mode"], views["switch"])
        word = torch.zeros(4, dtype=torch.int32, device=T._dev())

        def occ_array(change=None, at=0):
            """The views' occlusions as the call takes them; change(o) edits the one of view `at` (which has a pyramid)."""
            keep = [None if k is None else images.occ(k, cvoc.OCCLUSIONS[k][0]) for k in kinds]
            if change is not None:
                change(keep[at])
            arr = (C.c_void_p * n_views)(*[C.addressof(o) if o is not None else None for o in keep])
            return arr, keep

        def outputs(**kw):
            o = out.outputs()
            for k, v in kw.items():
                setattr(o, k, v)
            return o

        good_occs, good_keep = occ_array()

        def call(o=None, policy=policy, fr=frames, bm=bitmaps, oc=good_occs, k=n_views, context=ctx):
            o = outputs() if o is None else o
            addr = lambda x: C.addressof(x) if x is not None else None   # noqa: E731
            return lib.mip_list_clusters_views_occluded(context, addr(fr), addr(bm), addr(oc), k, addr(policy), addr(o) if o != "null" else None)

        def with_occ(change, at=0):
            arr, keep = occ_array(change, at)
            rc = call(oc=arr)
            msg = lib.mip_last_error(ctx).decode()
            del keep
            return rc, msg

        bad_policy = make_lod_policy(views["mode"], views["switch"])
        bad_policy.switch_sq[1] = 1.0           # decreases
        good = out.outputs()
        refused = {
            "NULL ctx": call(context=None), "NULL frames": call(fr=None), "NULL visible_bitmaps": call(bm=None), "NULL policy": call(policy=None),
            "NULL occs": call(oc=None),
            "NULL out": call(o="null"), "NULL cluster_entries": call(outputs(cluster_entries=None)), "NULL entry_counts": call(outputs(entry_counts=None)),
            "struct_size 48": call(outputs(struct_size=48)), "struct_size 64": call(outputs(struct_size=64)),
            "unknown flags": call(outputs(flags=_lib.MIP_OUT_DEVICE | 0x10)), "host outputs": call(outputs(flags=0)),
            "misaligned entry_counts": call(outputs(entry_counts=good.entry_counts + 2)), "misaligned draw_args": call(outputs(draw_args=good.draw_args + 1)),
            "misaligned stats": call(outputs(stats=good.stats + 2)), "misaligned hidden": call(outputs(hidden=good.hidden + 2)),
            "entries 8-byte aligned only": call(outputs(cluster_entries=good.cluster_entries + 8)),
            "zero views": call(k=0), "seventeen views": call(k=17),
            "n_views x entry_stride = 2^32": call(outputs(entry_stride=(1 << 32) // 4 if n_views == 4 else -(-(1 << 32) // n_views))),
            "n_views x entry_stride above 2^32": call(outputs(entry_stride=0xFFFFFFFF)),
            "decreasing thresholds": call(policy=bad_policy),
            "hidden is stats' first word": call(outputs(hidden=good.stats)), "hidden is stats' last word": call(outputs(hidden=good.stats + 4 * (1 + n_views))),
            "hidden inside draw_args": call(outputs(hidden=good.draw_args + 4 * (4 * n_views - 1))), "hidden is entry_counts": call(outputs(hidden=good.entry_counts)),
            "hidden inside entry_counts": call(outputs(hidden=good.entry_counts + 4 * (n_views - 1))),
        }
        assert all(rc == INVALID for rc in refused.values()), refused
        # a non-NULL entry that mip_cull_clusters would refuse, in the first and in a later slot: the message names the view
        assert kinds[0] is not None and kinds[2] is not None
        for at in (0, 2):
            for what, change in (("struct_size", lambda o: setattr(o, "struct_size", 96)), ("candidates", lambda o: setattr(o, "candidates", word.data_ptr())),
                                 ("occluded_bitmap", lambda o: setattr(o, "occluded_bitmap", word.data_ptr())), ("flags", lambda o: setattr(o, "flags", 1)),
                                 ("width 0", lambda o: setattr(o, "width", 0)), ("height 0", lambda o: setattr(o, "height", 0)),
                                 ("width above the limit", lambda o: setattr(o, "width", _lib.MIP_MAX_DEPTH_EXTENT + 1)),
                                 ("height above the limit", lambda o: setattr(o, "height", _lib.MIP_MAX_DEPTH_EXTENT + 1)),
                                 ("NULL pyramid", lambda o: setattr(o, "pyramid", None))):
                rc, msg = with_occ(change, at)
                assert rc == INVALID and f"view {at}" in msg, (what, at, rc, msg)
        assert out.untouched()
        # hidden just in front of stats and just behind it is no overlap: taken, and nothing outside the two ranges is written
        arena = torch.full((64,), T._i32(SENTINEL), dtype=torch.int32, device=T._dev())
        stats_at, words = 16, 2 + n_views
        for hidden_at in (stats_at - n_views, stats_at + words):
            arena.fill_(T._i32(SENTINEL))
            torch.cuda.synchronize()
            assert call(outputs(entry_stride=8, stats=arena.data_ptr() + 4 * stats_at, hidden=arena.data_ptr() + 4 * hidden_at)) == 0, hidden_at
            got = arena.cpu().numpy().view(np.uint32)
            assert got[stats_at: stats_at + words].tolist() == hand["stats"].tolist() and got[hidden_at: hidden_at + n_views].tolist() == hand["hidden"].tolist()
            outside = np.ones(64, bool)
            outside[stats_at: stats_at + words] = False
            outside[hidden_at: hidden_at + n_views] = False
            assert (got[outside] == SENTINEL).all(), hidden_at
        assert call(outputs(entry_stride=8)) == 0 and not out.untouched()     # the same arguments, nothing wrong with them: taken
        _given_call(ra, p, s, views, kinds, hand, name + " after the refusals")     # the context is usable
    # no instances; no cluster table; a stale one: not ready, nothing written
    fresh = _Out(n_views, 8)
    frames = [make_frame(views["planes"][v], views["cams"][v]) for v in range(n_views)]
    with ra.InstancePipeline(max_instances=4, max_meshes=len(s["meshes"])) as p:
        p.set_mesh_table(s["meshes"])
        p.set_geometry(s["vertices"], s["indices"])
        p.build_clusters()
        with pytest.raises(ra.MipError) as e:
            p.list_clusters_views_occluded(frames, [0] * n_views, [None] * n_views, policy, fresh.outputs())
        assert e.value.code == NOT_READY and fresh.untouched()
    with T._pipeline(ra, s) as p:
        p.set_geometry(s["vertices"], s["indices"])
        with pytest.raises(ra.MipError) as e:                    # no table yet
            p.list_clusters_views_occluded(frames, [0] * n_views, [None] * n_views, policy, fresh.outputs())
        assert e.value.code == NOT_READY and fresh.untouched()
        p.build_clusters()
        p.set_geometry(s["vertices"], s["indices"])             # stale again
        with pytest.raises(ra.MipError) as e:
            p.list_clusters_views_occluded(frames, [0] * n_views, [None] * n_views, policy, fresh.outputs())
        assert e.value.code == NOT_READY and fresh.untouched()
        p.build_clusters()
        _given_call(ra, p, s, views, kinds, hand, name + " after the rebuild")
