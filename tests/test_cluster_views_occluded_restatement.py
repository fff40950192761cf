"""mip_list_clusters_views_occluded without a GPU (include/mi_instance_pipeline.h): the known survivors of config 3 under
the walls; the hand-written scenes (tests/cluster_view_occluded_cases.py) against the restatement
(tests/cluster_views_occluded_restatement.py); the three equivalences — (a) one cluster_list_restatement.list_clusters per view
under the view's pyramid, (b) cluster_views_list_restatement with no pyramid at all, (c) a subsequence of that call's lists with
survivors + hidden = its survivors — over config 3; mixed, shared and cleared pyramids; both overflow rules per view and the
sentinel behind every count; the struct in C, ctypes and the Rust text; the header, the exports, the Makefile and the C smoke
text; the kernel's argument struct against the kernel-argument limit, compiled; and the likely mistakes of a pyramid per
view, each caught by a named scene."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cluster_list_restatement as clr
import cluster_restatement as cr
import cluster_view_cases as cv
import cluster_view_occluded_cases as cvoc
import cluster_views_list_restatement as cvlr
import cluster_views_occluded_restatement as cvor
import lod_restatement as lr
import numpy_restatement as nr
import occlusion_restatement as orr
import test_cluster_phase_restatement as TP
from renderer_amd import scene
from renderer_amd._lib import MipClusterViewOccludedListOutputs
from renderer_amd.pipeline import make_cluster_view_occluded_list_outputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi_instance_pipeline.h")
CASES = cvoc.cases()
SENTINEL = 0xDEADBEEF
WALLS = (0, 16, 32)

# survivors free / under the wall at 0 / 16 / 32 of the first six turns: config 3, full bitmaps, the pin policy, DISTANCE;
# checked with cluster_restatement.cull_clusters when the call was specified
KNOWN = {
    (257, "strips"): dict(W=9917, views=[(2581, 970, 1428, 1628), (3425, 1572, 2200, 1853), (2581, 1628, 1428, 970), (2539, 1353, 870, 1206),
                                         (255, 84, 86, 171), (2127, 1426, 1435, 703)]),
    (1025, "rows"): dict(W=34820, views=[(9076, 4034, 3782, 5147), (9931, 4319, 5720, 5795), (9076, 5147, 3782, 4034), (7649, 4090, 3756, 3820),
                                         (1293, 517, 884, 780), (8466, 5363, 5180, 3125)]),
}

_SCENES = {}


def _scene_of(n, layout="strips"):
    if (n, layout) not in _SCENES:
        s = scene.make_scene(3, n=n)
        vertices, indices = scene.make_geometry(s["meshes"], layout)
        _SCENES[(n, layout)] = (s, cr.cluster_boxes(s["meshes"], vertices, indices))
    return _SCENES[(n, layout)]


_LEVELS = {c: orr.pyramid_levels(TP.wall_depth(c)) for c in WALLS}
_LEVELS[None] = orr.pyramid_levels(np.ones((32, 64), np.float32))


def _occ(pv, column):
    return dict(pv=pv, levels=_LEVELS[column], width=64, height=32)


def _wall_occs(n_views, columns=None, missing=()):
    """View v: the default pv turned as the view's planes are, the wall at (0, 16, 32)[v % 3] (or columns[v]); None in `missing`."""
    pvs = cvor.view_pvs(scene.default_pv(), n_views)
    return [None if v in missing else _occ(pvs[v], WALLS[v % 3] if columns is None else columns[v]) for v in range(n_views)]


def _bitmaps(s, planes, kinds=("culled", "shared", "null")):
    own, out = {}, []
    for v in range(len(planes)):
        kind = kinds[v % len(kinds)]
        if kind == "null":
            out.append(None)
            continue
        src = 0 if kind == "shared" else v
        if src not in own:
            own[src] = orr.bitmap_of(~nr.run(dict(s, planes=planes[src]))["coarse_culled"])
        out.append(own[src])
    return out


def _is_subsequence(short, long):
    """Whether the rows of `short` are rows of `long` in the same order."""
    a = [r.tobytes() for r in short]
    it = iter(r.tobytes() for r in long)
    return all(any(x == y for y in it) for x in a)


# ---- the turn ----

def test_the_turn_of_pv_matches_the_turn_of_the_planes():
    pv = scene.default_pv()
    pts = np.random.default_rng(5).normal(0, 30, (64, 3))
    assert cvor.TURNS == [(0, 1, 2, 1, 1), (2, 1, 0, 1, 1), (0, 1, 2, -1, 1), (2, 1, 0, -1, 1), (0, 2, 1, 1, 1), (0, 1, 2, 1, -1)]
    planes = np.arange(24, dtype=np.float32) + 1
    for v, (a, b, c, sx, sz) in enumerate(cvor.TURNS):
        t = cvor.view_pvs(pv, v + 1)[v]
        assert sorted(np.abs(t).tolist()) == sorted(np.abs(pv).tolist())          # a permutation and sign flips: no rounding
        # the turned matrix applied to p is the matrix applied to the turned point q: q[a] = sx p.x, q[b] = p.y, q[c] = sz p.z
        q = np.zeros_like(pts)
        q[:, a], q[:, b], q[:, c] = sx * pts[:, 0], pts[:, 1], sz * pts[:, 2]
        m, mt = pv.reshape(4, 4).astype(np.float64), t.reshape(4, 4).astype(np.float64)
        assert np.allclose(pts @ mt[:3] + mt[3], q @ m[:3] + m[3], rtol=1e-12, atol=1e-9), v
        # cluster_view_cases.frusta turns the planes the same way: n' . p = n . q
        turned = planes.reshape(6, 4)[:, [a, b, c, 3]].copy()
        turned[:, 0] *= sx
        turned[:, 2] *= sz
        assert cv.frusta(planes, v + 1)[v].tolist() == turned.reshape(-1).tolist()


# ---- the known answers ----

@pytest.mark.parametrize("n,layout", list(KNOWN))
def test_known_survivors_under_the_walls(n, layout):
    s, boxes = _scene_of(n, layout)
    known = KNOWN[(n, layout)]
    planes = cv.frusta(s["planes"], 6)
    free = [k[0] for k in known["views"]]
    # the walls assigned per view: column (0, 16, 32)[v % 3]
    got = cvor.list_clusters_views_occluded(s, boxes, planes, [None] * 6, _wall_occs(6), [0] * 6, lr.DISTANCE, lr.PIN_SWITCH_SQ, 1 << 20)
    walled = [known["views"][v][1 + v % 3] for v in range(6)]
    assert got["status"] == 0 and got["stats"].tolist() == [known["W"], n] + walled
    assert got["hidden"].tolist() == [f - w for f, w in zip(free, walled)]
    assert all(0 < w < f for f, w in zip(free, walled))                           # no view is vacuous: each keeps some and loses some
    # the existing single-view restatement, view by view, says the same
    full = np.full((n + 31) // 32, 0xFFFFFFFF, np.uint32)
    occs = _wall_occs(6)
    for v in (1, 4):
        one = cr.cull_clusters(dict(s, planes=planes[v]), boxes, full, lr.DISTANCE, lr.PIN_SWITCH_SQ, 1 << 30, occlusion=occs[v])
        assert int(one["stats"][1]) == walled[v] and int(one["stats"][2]) == known["W"]
    if n == 257:                                                                  # the whole table: every view under every wall
        for k, column in enumerate(WALLS):
            got = cvor.list_clusters_views_occluded(s, boxes, planes, [None] * 6, _wall_occs(6, [column] * 6), [0] * 6, lr.DISTANCE, lr.PIN_SWITCH_SQ, 1 << 20)
            assert got["stats"][2:].tolist() == [kv[1 + k] for kv in known["views"]], column
            assert got["hidden"].tolist() == [kv[0] - kv[1 + k] for kv in known["views"]], column
        assert free == [sv for _, sv in cv.KNOWN[257]["views"]]                   # the plain several-view call's pinned survivors


# ---- the hand-written scenes ----

def _owed(s, views, kinds, entry_stride, work_capacity=0, mutant=None):
    boxes = cr.cluster_boxes(s["meshes"], s["vertices"], s["indices"])
    return cvor.list_clusters_views_occluded(s, boxes, views["planes"], views["bitmaps"], [cvoc.occlusion(k) for k in kinds], views["bases"], views["mode"],
                                             views["switch"], entry_stride, work_capacity, cam_pos=views["cams"][0], mutant=mutant)


@pytest.mark.parametrize("name,s,views,kinds,want", CASES, ids=[c[0] for c in CASES])
def test_hand_written_scenes(name, s, views, kinds, want):
    got = _owed(s, views, kinds, 16)
    n_views = len(kinds)
    assert got["status"] == 0 and got["stats"].tolist() == want["stats"].tolist(), (name, got["stats"])
    assert got["hidden"].tolist() == want["hidden"].tolist(), (name, got["hidden"])
    for v in range(n_views):
        assert got["entries"][v].tobytes() == want["entries"][v].tobytes(), (name, v, got["entries"][v], want["entries"][v])
        assert int(got["counts"][v]) == len(want["entries"][v]) and got["args"][v].tolist() == [192, len(want["entries"][v]), 0, 16 * v]
    # (c) against the plain several-view restatement
    boxes = cr.cluster_boxes(s["meshes"], s["vertices"], s["indices"])
    plain = cvlr.list_clusters_views(s, boxes, views["planes"], views["bitmaps"], views["bases"], views["mode"], views["switch"], 16, cam_pos=views["cams"][0])
    assert plain["stats"][:2].tolist() == got["stats"][:2].tolist()
    for v in range(n_views):
        assert _is_subsequence(got["entries"][v], plain["entries"][v]) and int(got["stats"][2 + v]) + int(got["hidden"][v]) == int(plain["stats"][2 + v])


def test_hand_cases_cover_what_they_claim():
    by_name = {c[0]: c for c in CASES}
    middle = by_name["hidden in the middle view only"]
    assert middle[3] == [None, "in", None] and middle[4]["hidden"].tolist() == [0, 4, 0] and [len(e) for e in middle[4]["entries"]] == [7, 3, 7]
    two = by_name["one pyramid under two projections"]
    assert np.array_equal(cvoc.OCCLUSIONS[two[3][0]][1], cvoc.OCCLUSIONS[two[3][1]][1]) and not np.array_equal(cvoc.OCCLUSIONS["all"][0], cvoc.OCCLUSIONS["out"][0])
    assert cvoc.occlusion("small in")["width"] == 32 and cvoc.occlusion("small in")["height"] == 16
    assert (cvoc.OCCLUSIONS["cleared"][1] == 1.0).all()
    member = by_name["a pyramid never adds or removes a member"]
    assert member[1]["n"] == 3 and member[4]["stats"][:2].tolist() == [4, 2] and member[4]["hidden"].tolist() == [1, 0]
    assert TP.wall_depth(16).tobytes() == cvoc.wall(16).tobytes() and TP.wall_depth(0).tobytes() == cvoc.wall(0).tobytes()


def test_the_closed_form_of_a_ladder_under_pyramids():
    patterns = ["1" * 70 + "0" * 3 + "1", "0101" * 40, "", np.arange(200) % 3 == 0]
    inst = [0, 1, 2, 3, 3, 0, 2, 1]
    some = np.array([1, 1, 1, 0, 1, 1, 1, 1], bool)
    specs = [("C", "in", some, 0xFFFFFFFD), ("C", None, None, 5), ("A", "in", None, 9), ("C", "out", ~some, 1), ("B", "none", None, 2), ("C", "all", None, 3)]
    s, views, kinds, want = cvoc.occluded_ladder(patterns, inst, specs)
    got = _owed(s, views, kinds, 1 << 12)
    assert got["status"] == 0 and got["stats"].tolist() == want["stats"].tolist() and got["hidden"].tolist() == want["hidden"].tolist()
    for v in range(len(specs)):
        assert got["entries"][v].tobytes() == want["entries"][v].tobytes(), v
    assert len(want["entries"][2]) == 0 and want["hidden"][2] > 0 and want["hidden"][1] == 0 and want["hidden"][4] == 0
    assert int(want["hidden"][5]) == int(want["stats"][3]) and len(want["entries"][5]) == 0     # "all" hides what the NULL-bitmap view without a pyramid lists


# ---- the three equivalences over the repository's own scenes ----

@pytest.mark.parametrize("n", [257, 1025])
@pytest.mark.parametrize("n_views", [1, 2, 3, 5, 16])
def test_the_three_equivalences(n, n_views):
    s, boxes = _scene_of(n)
    planes, bases, cams = cv.frusta(s["planes"], n_views), cv.view_bases(n_views, n), cv.view_cams(s, n_views)
    bitmaps = _bitmaps(s, planes)
    occs = _wall_occs(n_views)
    full = np.full((n + 31) // 32, 0xFFFFFFFF, np.uint32)
    for mode in (lr.DISTANCE, lr.RELATIVE):
        sw = cv.metric_thresholds(s, mode)
        stride = 40 * n
        got = cvor.list_clusters_views_occluded(s, boxes, planes, bitmaps, occs, bases, mode, sw, stride, cam_pos=cams[0])
        plain = cvlr.list_clusters_views(s, boxes, planes, bitmaps, bases, mode, sw, stride, cam_pos=cams[0])
        assert got["status"] == 0 and int(got["stats"][0]) == got["items"]["W"] > 0
        # a pyramid never changes membership, W or the work items
        assert got["stats"][:2].tolist() == plain["stats"][:2].tolist() and got["items"]["inst"].tobytes() == plain["items"]["inst"].tobytes()
        for v in range(n_views):
            # (a) one mip_list_clusters per view under the view's pyramid, with frames[0]'s camera
            one = clr.list_clusters(dict(s, planes=planes[v], cam_pos=cams[0]), boxes, full if bitmaps[v] is None else bitmaps[v], mode, sw, stride,
                                    first_instance_base=bases[v], occlusion=occs[v])
            assert one["status"] == 0 and got["entries"][v].tobytes() == one["entries"].tobytes(), (n, n_views, mode, v)
            assert int(got["counts"][v]) == one["count"] and int(got["stats"][2 + v]) == int(one["stats"][0])
            assert got["args"][v].tolist() == [192, one["count"], 0, v * stride]
            # (c) a subsequence of the plain several-view list; survivors + hidden = its survivors
            assert _is_subsequence(got["entries"][v], plain["entries"][v]), (n, n_views, mode, v)
            assert int(got["stats"][2 + v]) + int(got["hidden"][v]) == int(plain["stats"][2 + v])
            assert (got["survive"][v] <= plain["survive"][v]).all() and got["passed"][v].tolist() == plain["survive"][v].tolist()
        assert int(got["hidden"].sum()) > 0
        # (b) no pyramid at all: the plain several-view call, byte for byte, and nothing hidden
        bare = cvor.list_clusters_views_occluded(s, boxes, planes, bitmaps, [None] * n_views, bases, mode, sw, stride, cam_pos=cams[0])
        assert bare["hidden"].tolist() == [0] * n_views and bare["status"] == plain["status"] == 0
        fa, fb = cvor.fill_outputs(bare, n_views, stride, SENTINEL, 3), cvlr.fill_outputs(plain, n_views, stride, SENTINEL, 3)
        assert all(fa[k].tobytes() == fb[k].tobytes() for k in fb)


def test_mixed_shared_and_cleared_pyramids():
    s, boxes = _scene_of(257)
    n_views = 5
    planes, bases = cv.frusta(s["planes"], n_views), cv.view_bases(n_views, 257)
    bitmaps = [None] * n_views                  # full bitmaps: every view keeps some clusters and loses some under every wall (KNOWN)
    args = (lr.DISTANCE, lr.PIN_SWITCH_SQ, 1 << 20)
    every = cvor.list_clusters_views_occluded(s, boxes, planes, bitmaps, _wall_occs(n_views), bases, *args)
    plain = cvlr.list_clusters_views(s, boxes, planes, bitmaps, bases, *args)
    assert all(int(h) > 0 for h in every["hidden"])
    # NULL in the first slot, a middle slot, the last slot, and everywhere: that view is the plain call's, the others keep their pyramid
    for missing in ((0,), (2,), (4,), (0, 2, 4), tuple(range(n_views))):
        got = cvor.list_clusters_views_occluded(s, boxes, planes, bitmaps, _wall_occs(n_views, missing=missing), bases, *args)
        for v in range(n_views):
            src = plain if v in missing else every
            assert got["entries"][v].tobytes() == src["entries"][v].tobytes(), (missing, v)
            assert int(got["hidden"][v]) == (0 if v in missing else int(every["hidden"][v]))
    # one pyramid shared by all views, each with its own pv: the wall at 16 (views 0 and 2 mirror each other about it; views 0 and 1 do not)
    shared = cvor.list_clusters_views_occluded(s, boxes, planes, bitmaps, _wall_occs(n_views, [16, 16, 16, 16, 16]), bases, *args)
    pvs = cvor.view_pvs(scene.default_pv(), n_views)
    assert pvs[0].tobytes() != pvs[1].tobytes() and shared["survive"][0].tolist() != shared["survive"][1].tolist()
    full = np.full((257 + 31) // 32, 0xFFFFFFFF, np.uint32)
    for v in (0, 1, 2):
        one = clr.list_clusters(dict(s, planes=planes[v]), boxes, full if bitmaps[v] is None else bitmaps[v], *args, first_instance_base=bases[v],
                                occlusion=_occ(pvs[v], 16))
        assert shared["entries"][v].tobytes() == one["entries"].tobytes()
    # a cleared image, all 1.0: nothing hidden, equal to the plain call
    cleared = cvor.list_clusters_views_occluded(s, boxes, planes, bitmaps, _wall_occs(n_views, [None] * n_views), bases, *args)
    assert cleared["hidden"].tolist() == [0] * n_views and cleared["stats"].tolist() == plain["stats"].tolist()
    assert all(cleared["entries"][v].tobytes() == plain["entries"][v].tobytes() for v in range(n_views))


# ---- the overflow rules, per view; untouched entries keep the sentinel ----

def test_overflow_rules_per_view():
    s, boxes = _scene_of(257)
    planes, bases = cv.frusta(s["planes"], 3), cv.view_bases(3)
    args = (s, boxes, planes, _bitmaps(s, planes), _wall_occs(3), bases, lr.DISTANCE, lr.PIN_SWITCH_SQ)
    full = cvor.list_clusters_views_occluded(*args, 1 << 20)
    sv, w, members = full["stats"][2:].tolist(), int(full["stats"][0]), int(full["stats"][1])
    assert full["status"] == 0 and min(sv) > 2 and len(set(sv)) > 1 and min(full["hidden"]) > 0
    big, small = int(np.argmax(sv)), int(np.argmin(sv))
    # ENTRY OVERFLOW: that view is cut, the others are complete, stats and hidden are true
    stride = sv[big] - 1
    cut = cvor.list_clusters_views_occluded(*args, stride)
    assert cut["status"] == cvor.ERR_CAPACITY and cut["stats"].tolist() == full["stats"].tolist() and cut["hidden"].tolist() == full["hidden"].tolist()
    for v in range(3):
        count = min(sv[v], stride)
        assert int(cut["counts"][v]) == count and cut["entries"][v].tobytes() == full["entries"][v][:count].tobytes()
        assert cut["args"][v].tolist() == [192, count, 0, v * stride]
    assert int(cut["counts"][small]) == sv[small] and int(cut["counts"][big]) == stride
    none = cvor.list_clusters_views_occluded(*args, 0)
    assert none["status"] == cvor.ERR_CAPACITY and none["counts"].tolist() == [0, 0, 0] and none["hidden"].tolist() == full["hidden"].tolist()
    fits = cvor.list_clusters_views_occluded(*args, max(sv), work_capacity=w)
    assert fits["status"] == 0 and all(fits["entries"][v].tobytes() == full["entries"][v].tobytes() for v in range(3))
    # WORK OVERFLOW: zero counts, {192, 0, 0, v x stride}, {W, members, 0, ...}, hidden all zero, no entry
    work = cvor.list_clusters_views_occluded(*args, 1000, work_capacity=w - 1)
    assert work["status"] == cvor.ERR_CAPACITY and work["counts"].tolist() == [0, 0, 0] and all(len(e) == 0 for e in work["entries"])
    assert work["stats"].tolist() == [w, members, 0, 0, 0] and work["hidden"].tolist() == [0, 0, 0]
    assert work["args"].tolist() == [[192, 0, 0, 0], [192, 0, 0, 1000], [192, 0, 0, 2000]]
    # N = 0
    empty = cvor.list_clusters_views_occluded(dict(s, pos=s["pos"][:0], rot=s["rot"][:0], scale=s["scale"][:0], mesh_id=s["mesh_id"][:0]), boxes, planes,
                                              [None] * 3, _wall_occs(3), bases, lr.DISTANCE, lr.PIN_SWITCH_SQ, 4)
    assert empty["status"] == 0 and empty["counts"].tolist() == [0, 0, 0] and empty["stats"].tolist() == [0] * 5 and empty["hidden"].tolist() == [0] * 3
    assert empty["args"].tolist() == [[192, 0, 0, 0], [192, 0, 0, 4], [192, 0, 0, 8]]
    # what sentinel-filled buffers hold afterwards: everything at or behind a count, and every pad, untouched
    filled = cvor.fill_outputs(cut, 3, stride, SENTINEL, 3)
    for v in range(3):
        count = int(cut["counts"][v])
        assert (filled["entries"][v * stride + count: (v + 1) * stride] == SENTINEL).all()
        assert filled["entries"][v * stride: v * stride + count].tobytes() == full["entries"][v][:count].tobytes()
    assert (filled["entries"][3 * stride:] == SENTINEL).all() and (filled["counts"][3:] == SENTINEL).all()
    assert (filled["args"][12:] == SENTINEL).all() and (filled["stats"][5:] == SENTINEL).all()
    assert filled["hidden"][:3].tolist() == full["hidden"].tolist() and (filled["hidden"][3:] == SENTINEL).all()
    off = cvor.fill_outputs(cut, 3, stride, SENTINEL, 3, args=False, stats=False, hidden=False)
    assert (off["args"] == SENTINEL).all() and (off["stats"] == SENTINEL).all() and (off["hidden"] == SENTINEL).all()


# ---- the likely mistakes, each caught by a named scene ----

_KILLED_BY = {
    "pv of slot 0": "one pyramid under two projections", "pyramid of slot 0": "a wall over the inside clusters", "extents of slot 0": "two extents",
    "pyramid before the bitmap bit": "a pyramid never adds or removes a member", "hidden counts lanes outside the view": "a pyramid never adds or removes a member",
    "NULL occlusion hides everything": "hidden in the middle view only", "a pyramid changes the members": "a pyramid never adds or removes a member",
}


def test_every_likely_mistake_is_caught_by_its_scene():
    assert set(_KILLED_BY) == set(cvor.MUTANTS)
    by_name = {c[0]: c for c in CASES}

    def same(got, want, n_views):
        return (got["stats"].tolist() == want["stats"].tolist() and got["hidden"].tolist() == want["hidden"].tolist()
                and all(got["entries"][v].tobytes() == want["entries"][v].tobytes() for v in range(n_views)))

    for mutant, name in _KILLED_BY.items():
        _, s, views, kinds, want = by_name[name]
        assert same(_owed(s, views, kinds, 16), want, len(kinds)), (name, "the header's rule")
        assert not same(_owed(s, views, kinds, 16, mutant=mutant), want, len(kinds)), (mutant, "is not caught by", name)
    # "pyramid before the bitmap bit" leaves every entry as it is and miscounts hidden alone
    _, s, views, kinds, want = by_name["a pyramid never adds or removes a member"]
    wrong = _owed(s, views, kinds, 16, mutant="pyramid before the bitmap bit")
    assert all(wrong["entries"][v].tobytes() == want["entries"][v].tobytes() for v in range(2)) and wrong["hidden"].tolist() == [2, 0]


# ---- the ABI ----

def test_struct_sizes_in_c_ctypes_and_rust(tmp_path):
    from renderer_amd import _lib as L

    O = MipClusterViewOccludedListOutputs
    assert L.MipClusterViewOccludedListOutputs is O
    want = [0, 4, 8, 16, 20, 24, 32, 40, 48]
    assert C.sizeof(O) == 56 and [getattr(O, f).offset for f, _ in O._fields_] == want
    assert [f for f, _ in O._fields_][:8] == [f for f, _ in L.MipClusterViewListOutputs._fields_]      # exactly that struct's fields, then hidden
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "mi_instance_pipeline.h"
    #define O(f) offsetof(MipClusterViewOccludedListOutputs, f)
    int main(void) {
      printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d\n", sizeof(MipClusterViewOccludedListOutputs), O(struct_size), O(flags), O(cluster_entries),
             O(entry_stride), O(work_capacity), O(entry_counts), O(draw_args), O(stats), O(hidden), (int)MIP_ABI_VERSION, (int)MIP_MAX_VIEWS);
      return 0; }'''
    c = tmp_path / "t.c"
    c.write_text(src)
    exe = str(tmp_path / "t")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe])
    assert [int(x) for x in subprocess.check_output([exe]).split()] == [56] + want + [4, 16]
    rust = open(os.path.join(ROOT, "integration", "rust", "mip-sys", "src", "lib.rs")).read()
    body = re.search(r"pub struct MipClusterViewOccludedListOutputs \{(.*?)\}", rust, flags=re.S).group(1)
    assert re.findall(r"pub (\w+): ([^,]+),", body) == [("struct_size", "u32"), ("flags", "u32"), ("cluster_entries", "*mut c_void"), ("entry_stride", "u32"),
                                                        ("work_capacity", "u32"), ("entry_counts", "*mut u32"), ("draw_args", "*mut u32"), ("stats", "*mut u32"),
                                                        ("hidden", "*mut u32")]
    assert "#[repr(C)]" in rust[: rust.index("pub struct MipClusterViewOccludedListOutputs")].rsplit("\n\n", 1)[-1]
    assert "const _: [u8; 56] = [0; std::mem::size_of::<MipClusterViewOccludedListOutputs>()];" in rust


def test_header_exports_and_declarations_agree():
    from renderer_amd import _lib as L
    import renderer_amd

    name = "mip_list_clusters_views_occluded"
    text = open(HEADER).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    rust = open(os.path.join(ROOT, "integration", "rust", "mip-sys", "src", "lib.rs")).read()
    lib = L.load_library()
    assert name in L.EXPORTS and hasattr(lib, name)
    c_args = re.search(name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S).group(1).count(",") + 1
    assert c_args == 7 and len(getattr(lib, name).argtypes) == 7
    assert re.search(r"pub fn " + name + r"\((.*?)\)\s*->", rust, flags=re.S).group(1).count(",") + 1 == 7
    assert re.search(name + r"\([^;]*const MipOcclusion\* const\* occs\s*,\s*uint32_t n_views\s*,\s*const MipLodPolicy\* policy\s*,\s*"
                     r"const MipClusterViewOccludedListOutputs\* out\)", header)
    assert lib.mip_list_clusters_views_occluded(None, None, None, None, 1, None, None) == -1        # without a context: a status code
    assert "#define MIP_ABI_VERSION 4" in text
    # the new section stands behind mip_list_clusters_views' declaration, in front of the two-phase list, and says what the issue lists
    start = text.index("visible-cluster lists for several views, a depth pyramid per view")
    assert text.index("int32_t mip_list_clusters_views(MipContext* ctx") < start < text.index("the visible-cluster list in two phases")
    section = text[start: text.index("} MipClusterViewOccludedListOutputs;")]
    for word in ("BORROWED TERMS", "ONE LOD FOR ALL VIEWS", "MEMBERS", "never changes membership", "HOST array of n_views HOST pointers", "occs[v] == NULL",
                 "share a pyramid pointer", "PASSES_v", "SURVIVES_v", "steps 1-9", "hidden[v]", "exact integer count", "ENTRY OVERFLOW", "WORK OVERFLOW",
                 "hidden is all zero", "WHO REPORTS", "N = 0", "n_views x entry_stride >=", "THE THREE EQUIVALENCES", "(a)", "(b)", "(c)", "subsequence", "REFUSED",
                 "a NULL occs", "names the view", "hidden not 4-byte aligned", "hidden inside stats", "MIP_ERR_NOT_READY", "ORDERING", "no new plane",
                 "OUT OF SCOPE", "a two-phase record per view"):
        assert word in section, word
    for first in ("cluster culling for several views in one call", "visible-cluster lists for several views in one call"):
        lower = text.lower()
        at = lower.index(first)
        scope = text[at: text.index("typedef struct", at)]
        assert "a pyramid per view (mip_list_clusters_views_occluded below)" in scope[scope.index("OUT OF SCOPE"):], first
    wait = text[text.index("/* Block until everything enqueued"): text.index("int32_t mip_wait(MipContext* ctx);")]
    assert name in wait
    assert callable(renderer_amd.make_cluster_view_occluded_list_outputs) and callable(renderer_amd.InstancePipeline.list_clusters_views_occluded)
    assert renderer_amd.make_cluster_view_occluded_list_outputs is make_cluster_view_occluded_list_outputs
    o = make_cluster_view_occluded_list_outputs(16, 5, 32, draw_args=48, stats=64, hidden=80, work_capacity=7, async_=True)
    assert (o.struct_size, o.flags, o.cluster_entries, o.entry_stride, o.work_capacity, o.entry_counts, o.draw_args, o.stats, o.hidden) == \
        (56, L.MIP_OUT_DEVICE | L.MIP_OUT_ASYNC, 16, 5, 7, 32, 48, 64, 80)
    mk = open(os.path.join(ROOT, "renderer_amd", "csrc", "Makefile")).read()
    kernels = re.search(r"^KERNELS := (.*)$", mk, flags=re.M).group(1).split()
    assert "cluster_views_occluded_kernel.hpp" in kernels
    api = open(os.path.join(ROOT, "renderer_amd", "csrc", "api_cluster.hip")).read()
    assert '#include "cluster_views_occluded_kernel.hpp"' in api and "mip::mip_cluster_views_cull_occluded_kernel" in api and "mip::mip_cluster_views_cull_occluded_packed_kernel" in api
    smoke = open(os.path.join(ROOT, "integration", "c", "mip_smoke.c")).read()
    assert "mip_list_clusters_views_occluded(ctx" in smoke


def test_the_argument_struct_fits_the_kernel_argument_limit(tmp_path):
    """The kernel's header carries the static assertion; here it is compiled, and the sizes it is about are printed."""
    src = tmp_path / "args.hip"
    src.write_text(r'''
    #include <cstdio>
    #include "cluster_views_occluded_kernel.hpp"
    static_assert(sizeof(mip::ClusterViewOccludedArgs) <= 4096, "kernel arguments");
    static_assert(sizeof(mip::ClusterViewOccludedArgs) == sizeof(mip::ClusterViewArgs) + 16 * sizeof(mip::ClusterViewOcclusion) + 8, "the front's block, 16 occlusion blocks, hidden");
    int main() { std::printf("%zu %zu %zu\n", sizeof(mip::ClusterViewOccludedArgs), sizeof(mip::ClusterViewArgs), sizeof(mip::ClusterViewOcclusion)); return 0; }
    ''')
    exe = str(tmp_path / "args")
    out = subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O0", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "renderer_amd", "csrc"),
                          "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    whole, front, block = (int(x) for x in subprocess.check_output([exe]).split())
    assert block == 80 and whole == front + 16 * 80 + 8 and whole <= 4096
    text = open(os.path.join(ROOT, "renderer_amd", "csrc", "cluster_views_occluded_kernel.hpp")).read()
    assert "static_assert(sizeof(ClusterViewOccludedArgs) <= 4096" in text
