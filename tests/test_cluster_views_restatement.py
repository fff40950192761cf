"""Cluster culling of several views in one call without a GPU: tests/cluster_views_restatement.py (written from the header's
text) against the hand-written scenes of tests/cluster_view_cases.py; THE EQUIVALENCE with one cluster_restatement.cull_clusters
per view over config 3; known answers pinned when the call was specified; both overflow rules per view and the sentinel
behind every count; the ABI surface of mip_cull_clusters_views (C, ctypes, the Rust text, EXPORTS); the native check of
renderer_amd/csrc/cluster_views_plan.hpp, built with the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cluster_restatement as cr
import cluster_view_cases as cv
import cluster_views_restatement as cvr
import lod_restatement as lr
import numpy_restatement as nr
import occlusion_restatement as orr
from renderer_amd import _lib, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi_instance_pipeline.h")
CASES = cv.cases()
SENTINEL = 0xDEADBEEF


# ---- the hand-written scenes ----

@pytest.mark.parametrize("name,s,views,want", CASES, ids=[c[0] for c in CASES])
def test_hand_cases_against_the_restatement(name, s, views, want):
    boxes = cr.cluster_boxes(s["meshes"], s["vertices"], s["indices"])
    got = cvr.cull_clusters_views(s, boxes, views["planes"], views["bitmaps"], views["bases"], views["mode"], views["switch"], cmd_stride=16,
                                  cam_pos=views["cams"][0])
    assert got["status"] == 0
    assert got["stats"].tolist() == want["stats"].tolist(), (name, got["stats"])
    for v in range(len(views["planes"])):
        assert got["cmds"][v].tobytes() == want["cmds"][v].tobytes(), (name, v, got["cmds"][v], want["cmds"][v])
        assert int(got["counts"][v]) == len(want["cmds"][v])


def test_hand_cases_cover_what_they_claim():
    by_name = {c[0]: c for c in CASES}
    four = by_name["four views of one ladder"]
    assert [len(c) for c in four[3]["cmds"]] == [4, 3, 1, 0] and four[3]["cmds"][2]["indexCount"].tolist() == [3 * 448]
    assert four[3]["stats"].tolist() == [7, 1, 4, 4, 3, 3, 1, 7, 0, 0]
    garbage = by_name["garbage cameras behind view 0"]
    assert all(np.isnan(c[0]) for c in garbage[2]["cams"][1:]) and garbage[3] is four[3]
    nulls = by_name["bitmaps {0}, {1}, {}, NULL"]
    assert nulls[2]["bitmaps"][3] is None and nulls[3]["cmds"][1]["firstInstance"].tolist() == [0]          # 0xFFFFFFFF + 1 wraps
    assert by_name["an instance in no bitmap"][3]["stats"][:2].tolist() == [4, 2] and by_name["an instance in no bitmap"][1]["n"] == 3
    # the two-level mesh: view 1's own camera would pick the other level
    for name, own in (("one level for all views: view 0 near", [0, 1]), ("one level for all views: view 0 far", [1, 0])):
        _, s, views, want = by_name[name]
        picks = [int(lr.select_lods(s["pos"], s["scale"], s["mesh_id"], s["meshes"], cam, views["mode"], views["switch"])[0]) for cam in views["cams"]]
        assert picks == own
        assert len({int(c["firstIndex"][0]) for c in want["cmds"]}) == 1


# ---- THE EQUIVALENCE over the repository's own scenes ----

def _config3(n):
    s = scene.make_scene(3, n=n)
    vertices, indices = scene.make_geometry(s["meshes"], "strips")
    return s, cr.cluster_boxes(s["meshes"], vertices, indices)


_SCENES = {}


def _scene_of(n):
    if n not in _SCENES:
        _SCENES[n] = _config3(n)
    return _SCENES[n]


def _view_bitmap(s, planes):
    """The visibility bitmap a view of mip_run_views writes: the instance boxes against the view's planes."""
    return orr.bitmap_of(~nr.run(dict(s, planes=planes))["coarse_culled"])


def _bitmaps(s, planes, kinds=("culled", "shared", "null")):
    own = {}
    out = []
    for v in range(len(planes)):
        kind = kinds[v % len(kinds)]
        if kind == "null":
            out.append(None)
        else:
            src = 0 if kind == "shared" else v
            if src not in own:
                own[src] = _view_bitmap(s, planes[src])
            out.append(own[src])
    return out


@pytest.mark.parametrize("n", [257, 1025])
@pytest.mark.parametrize("n_views", [1, 2, 3, 5, 16])
def test_equivalence_with_one_call_per_view(n, n_views):
    s, boxes = _scene_of(n)
    planes, bases, cams = cv.frusta(s["planes"], n_views), cv.view_bases(n_views), cv.view_cams(s, n_views)
    bitmaps = _bitmaps(s, planes)
    full = np.full((n + 31) // 32, 0xFFFFFFFF, np.uint32)
    for mode in (lr.DISTANCE, lr.RELATIVE):
        sw = cv.metric_thresholds(s, mode)
        stride = 4 * n
        got = cvr.cull_clusters_views(s, boxes, planes, bitmaps, bases, mode, sw, cmd_stride=stride, cam_pos=cams[0])
        assert got["status"] == 0 and int(got["stats"][0]) == got["items"]["W"] > 0
        union = np.zeros(n, bool)
        for v in range(n_views):
            one = cr.cull_clusters(dict(s, planes=planes[v], cam_pos=cams[0]), boxes, full if bitmaps[v] is None else bitmaps[v], mode, sw,
                                   cmd_capacity=stride, first_instance_base=bases[v])
            assert one["status"] == 0
            assert got["cmds"][v].tobytes() == one["cmds"].tobytes(), (n, n_views, mode, v)
            assert int(got["counts"][v]) == one["count"]
            assert [int(got["stats"][2 + 2 * v]), int(got["stats"][3 + 2 * v])] == one["stats"][:2].tolist(), (n, n_views, mode, v)
            union |= one["items"]["member"]
        assert int(got["stats"][1]) == int(union.sum())                                  # members: the union of the views' members
        if n_views >= 2:   # views 0 and 1 share a pointer and differ by their planes: other instances are drawn
            drawn = [np.unique((got["cmds"][v]["firstInstance"].astype(np.int64) - bases[v]) & 0xFFFFFFFF) for v in (0, 1)]
            assert drawn[0].tolist() != drawn[1].tolist()
        # the level is frames[0]'s: with view 1's camera in view 0's place the answer differs
        if n_views >= 2 and n == 1025:
            other = cvr.cull_clusters_views(s, boxes, planes, bitmaps, bases, mode, sw, cmd_stride=stride, cam_pos=cams[1])
            assert other["stats"].tolist() != got["stats"].tolist()


@pytest.mark.parametrize("n", [257, 1025])
def test_known_answers_full_bitmaps_pin_policy(n):
    s, boxes = _scene_of(n)
    known = cv.KNOWN[n]
    planes = cv.frusta(s["planes"], 6)
    got = cvr.cull_clusters_views(s, boxes, planes, [None] * 6, [0] * 6, lr.DISTANCE, lr.PIN_SWITCH_SQ, cmd_stride=1 << 20)
    assert got["status"] == 0
    assert (int(got["stats"][0]), int(got["stats"][1])) == (known["W"], known["members"])
    assert list(zip(got["heads"], got["survivors"])) == known["views"]
    assert got["stats"][2:].tolist() == [x for pair in known["views"] for x in pair]


# ---- the overflow rules, per view; untouched entries keep the sentinel ----

def test_overflow_rules_per_view():
    s, boxes = _scene_of(257)
    planes, bases = cv.frusta(s["planes"], 3), cv.view_bases(3)
    bitmaps = _bitmaps(s, planes)
    args = (s, boxes, planes, bitmaps, bases, lr.DISTANCE, lr.PIN_SWITCH_SQ)
    full = cvr.cull_clusters_views(*args, cmd_stride=1 << 20)
    heads, w, members = full["heads"], int(full["stats"][0]), int(full["stats"][1])
    assert full["status"] == 0 and min(heads) > 2 and len(set(heads)) > 1
    big, small = int(np.argmax(heads)), int(np.argmin(heads))
    # a stride one below the largest view's heads: that view is cut, the others are complete, the stats are true
    cut = cvr.cull_clusters_views(*args, cmd_stride=heads[big] - 1)
    assert cut["status"] == cvr.ERR_CAPACITY and cut["stats"].tolist() == full["stats"].tolist()
    for v in range(3):
        count = min(heads[v], heads[big] - 1)
        assert int(cut["counts"][v]) == count and cut["cmds"][v].tobytes() == full["cmds"][v][:count].tobytes()
    assert int(cut["counts"][small]) == heads[small]
    none = cvr.cull_clusters_views(*args, cmd_stride=0)
    assert none["status"] == cvr.ERR_CAPACITY and none["counts"].tolist() == [0, 0, 0] and none["stats"].tolist() == full["stats"].tolist()
    fits = cvr.cull_clusters_views(*args, cmd_stride=max(heads), work_capacity=w)
    assert fits["status"] == 0 and all(fits["cmds"][v].tobytes() == full["cmds"][v].tobytes() for v in range(3))
    work = cvr.cull_clusters_views(*args, cmd_stride=1 << 20, work_capacity=w - 1)
    assert work["status"] == cvr.ERR_CAPACITY and work["counts"].tolist() == [0, 0, 0]
    assert work["stats"].tolist() == [w, members, 0, 0, 0, 0, 0, 0] and all(len(c) == 0 for c in work["cmds"])
    empty = cvr.cull_clusters_views(dict(s, pos=s["pos"][:0], rot=s["rot"][:0], scale=s["scale"][:0], mesh_id=s["mesh_id"][:0]), boxes, planes,
                                    [None] * 3, bases, lr.DISTANCE, lr.PIN_SWITCH_SQ, cmd_stride=4)
    assert empty["status"] == 0 and empty["counts"].tolist() == [0, 0, 0] and empty["stats"].tolist() == [0] * 8
    # what a sentinel-filled buffer holds afterwards: every entry at or behind a view's count, and the pad, untouched
    stride = heads[big] - 1
    filled = cvr.fill_outputs(cut, 3, stride, SENTINEL, 3)
    for v in range(3):
        count = int(cut["counts"][v])
        assert (filled["cmds"][v * stride + count: (v + 1) * stride] == SENTINEL).all()
        assert filled["cmds"][v * stride: v * stride + count].tobytes() == full["cmds"][v][:count].tobytes()
    assert (filled["cmds"][3 * stride:] == SENTINEL).all() and (filled["counts"][3:] == SENTINEL).all() and (filled["stats"][8:] == SENTINEL).all()
    assert (cvr.fill_outputs(cut, 3, stride, SENTINEL, 3, stats=False)["stats"] == SENTINEL).all()


# ---- the ABI surface ----

def test_struct_in_c_ctypes_and_rust(tmp_path):
    assert C.sizeof(_lib.MipClusterViewOutputs) == 40
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "mi_instance_pipeline.h"
    int main(void) {
      printf("%zu %zu %zu %zu %zu %zu %zu %u\n", sizeof(MipClusterViewOutputs), offsetof(MipClusterViewOutputs, flags),
             offsetof(MipClusterViewOutputs, cluster_cmds), offsetof(MipClusterViewOutputs, cmd_stride), offsetof(MipClusterViewOutputs, work_capacity),
             offsetof(MipClusterViewOutputs, cmd_counts), offsetof(MipClusterViewOutputs, stats), MIP_MAX_VIEWS);
      return 0;
    }'''
    c = tmp_path / "t.c"
    c.write_text(src)
    exe = str(tmp_path / "t")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe])
    sizes = [int(x) for x in subprocess.check_output([exe]).split()]
    o = _lib.MipClusterViewOutputs
    assert sizes == [C.sizeof(o), o.flags.offset, o.cluster_cmds.offset, o.cmd_stride.offset, o.work_capacity.offset, o.cmd_counts.offset,
                     o.stats.offset, 16]
    rust = open(os.path.join(ROOT, "integration", "rust", "mip-sys", "src", "lib.rs")).read()
    body = re.search(r"pub struct MipClusterViewOutputs \{(.*?)\}", rust, flags=re.S).group(1)
    assert re.findall(r"pub (\w+):", body) == [f for f, _ in o._fields_]
    assert "const _: [u8; 40] = [0; std::mem::size_of::<MipClusterViewOutputs>()];" in rust
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    c_args = re.search(r"mip_cull_clusters_views\s*\(([^;]*?)\)\s*;", header, flags=re.S).group(1).count(",") + 1
    r_args = re.search(r"pub fn mip_cull_clusters_views\((.*?)\)\s*->", rust, flags=re.S).group(1).count(",") + 1
    assert c_args == r_args == 6
    smoke = open(os.path.join(ROOT, "integration", "c", "mip_smoke.c")).read()
    assert "MipClusterViewOutputs" in smoke and "mip_cull_clusters_views(" in smoke


def test_header_and_exports():
    text = open(HEADER).read()
    assert "#define MIP_ABI_VERSION 4u" in text
    assert "mip_cull_clusters_views" in _lib.EXPORTS
    assert re.search(r"\bmip_cull_clusters_views\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    section = text[text.index("Extension: cluster culling for several views"):text.index("MipClusterViewOutputs;")]
    assert "NOT a reference" in section and "frames[0].cam_pos" in section and "THE EQUIVALENCE" in section
    # mip_cull_clusters no longer lists views as out of scope, and points here
    plain = text[text.index("PER FRAME (mip_cull_clusters)"):text.index("#define MIP_CLUSTER_TRIANGLES")]
    scope = plain[plain.index("OUT OF SCOPE"):]
    assert "views" not in scope.split("(")[0] and "mip_cull_clusters_views" in scope
    import renderer_amd
    lib = renderer_amd.load_library()
    assert lib.mip_cull_clusters_views(None, None, None, 0, None, None) == -1


# ---- the plan ----

def test_cluster_views_plan_over_its_decision_edges(tmp_path):
    exe = str(tmp_path / "cluster_views_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "native", "cluster_views_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    last = out.stdout.strip().split("\n")[-1]
    assert last.startswith("CLUSTER VIEWS PLAN OK") and int(last.split()[4]) > 50_000, out.stdout[-2000:]
    sizes = subprocess.check_output([exe, "sizes"])
    assert b'"max_views": 16' in sizes and b'"launches": 7' in sizes
