"""mip_list_clusters_views without a GPU (include/mi_instance_pipeline.h): the hand-written lists
(tests/cluster_view_list_cases.py) against the restatement (tests/cluster_views_list_restatement.py); the two equivalences —
one cluster_list_restatement.list_clusters per view, and the expansion of cluster_views_restatement's commands — over config 3;
both overflow rules per view and the sentinel behind every count; the struct in C, ctypes and the Rust text; the header, the
exports and the Makefile; the plan (renderer_amd/csrc/cluster_views_list_plan.hpp) over its edges under the host sanitizers;
and the likely mistakes of a several-view tail, each caught by a named scene."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cluster_list_restatement as clr
import cluster_restatement as cr
import cluster_view_cases as cv
import cluster_view_list_cases as cvlc
import cluster_views_list_restatement as cvlr
import lod_restatement as lr
import numpy_restatement as nr
import occlusion_restatement as orr
from renderer_amd import scene
from renderer_amd._lib import MipClusterViewListOutputs
from renderer_amd.pipeline import CLUSTER_ENTRY_DTYPE, make_cluster_view_list_outputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi_instance_pipeline.h")
CASES = cvlc.cases()
SENTINEL = 0xDEADBEEF


def _owed(s, views, entry_stride, work_capacity=0):
    boxes = cr.cluster_boxes(s["meshes"], s["vertices"], s["indices"])
    return cvlr.list_clusters_views(s, boxes, views["planes"], views["bitmaps"], views["bases"], views["mode"], views["switch"], entry_stride, work_capacity,
                                    cam_pos=views["cams"][0])


# ---- the hand-written lists ----

@pytest.mark.parametrize("name,s,views,want", CASES, ids=[c[0] for c in CASES])
def test_hand_written_lists(name, s, views, want):
    got = _owed(s, views, 16)
    n_views = len(views["planes"])
    assert got["status"] == 0 and got["stats"].tolist() == want["stats"].tolist(), (name, got["stats"])
    cmds = {c[0]: c[3]["cmds"] for c in cv.cases()}[name]
    for v in range(n_views):
        assert got["entries"][v].tobytes() == want["entries"][v].tobytes(), (name, v, got["entries"][v], want["entries"][v])
        assert int(got["counts"][v]) == len(want["entries"][v])
        assert got["args"][v].tolist() == [192, len(want["entries"][v]), 0, 16 * v]
        # equivalence (b), on the hand-written commands of cluster_view_cases and on the restatement's
        assert clr.from_commands(cmds[v], s["meshes"]).tobytes() == want["entries"][v].tobytes(), (name, v)
        assert clr.from_commands(got["views"]["all_cmds"][v], s["meshes"]).tobytes() == want["entries"][v].tobytes()
    # the launches' steps give the same buffers
    steps = cvlr.entries_by_steps(got["items"], got["survive"], s["meshes"], views["bases"], 16, pad=3)
    filled = cvlr.fill_outputs(got, n_views, 16, SENTINEL, 3)
    written = filled["entries"][:, 3] != SENTINEL
    assert (steps["entries"]["index_count"] != 0xFFFFFFFF).tolist() == written.tolist()
    assert np.ascontiguousarray(steps["entries"]).view(np.uint32).reshape(-1, 4)[written].tobytes() == filled["entries"][written].tobytes()
    assert steps["counts"].tolist() == got["counts"].tolist() and steps["args"].tolist() == got["args"].tolist() and steps["stats"].tolist() == got["stats"].tolist()


def test_hand_cases_cover_what_they_claim():
    by_name = {c[0]: c for c in CASES}
    four = by_name["four views of one ladder"][3]
    assert [len(e) for e in four["entries"]] == [4, 3, 7, 0] and four["stats"].tolist() == [7, 1, 4, 3, 7, 0]
    assert by_name["garbage cameras behind view 0"][3]["entries"] is four["entries"]
    assert all(np.isnan(c[0]) for c in by_name["garbage cameras behind view 0"][2]["cams"][1:])
    nulls = by_name["bitmaps {0}, {1}, {}, NULL"]
    assert nulls[2]["bitmaps"][3] is None and nulls[2]["bases"][1] == 0xFFFFFFFF and nulls[3]["entries"][1]["instance"].tolist() == [0, 0]   # wraps
    assert by_name["an instance in no bitmap"][1]["n"] == 3 and by_name["an instance in no bitmap"][3]["stats"][:2].tolist() == [4, 2]
    assert by_name["a non-member between two members"][3]["entries"][0]["instance"].tolist() == [0, 2]
    assert {int(e["first_index"][0]) for e in by_name["one level for all views: view 0 near"][3]["entries"]} == {0}
    assert {int(e["first_index"][0]) for e in by_name["one level for all views: view 0 far"][3]["entries"]} == {384}


def test_the_closed_form_of_a_ladder_under_several_views():
    patterns = ["1" * 70 + "0" * 3 + "1", "0101" * 40, "", np.arange(200) % 3 == 0]
    inst = [0, 1, 2, 3, 3, 0, 2, 1]
    some = np.array([1, 1, 1, 0, 1, 1, 1, 1], bool)
    s, views, want = cvlc.ladder_views_list(patterns, inst, [("A", some, 0xFFFFFFFD), ("B", None, 5), ("D", None, 9), ("C", ~some, 1)])
    got = _owed(s, views, 1 << 12)
    assert got["status"] == 0 and got["stats"].tolist() == want["stats"].tolist()
    for v in range(4):
        assert got["entries"][v].tobytes() == want["entries"][v].tobytes(), v
    assert len(want["entries"][2]) == 0 and set(want["entries"][3]["instance"].tolist()) == {4}
    assert set(want["entries"][0]["instance"].tolist()) == {0xFFFFFFFD, 0xFFFFFFFE, 1, 2, 4}        # the base wraps inside the scene


# ---- the two equivalences over the repository's own scenes ----

_SCENES = {}


def _scene_of(n):
    if n not in _SCENES:
        s = scene.make_scene(3, n=n)
        vertices, indices = scene.make_geometry(s["meshes"], "strips")
        _SCENES[n] = (s, cr.cluster_boxes(s["meshes"], vertices, indices))
    return _SCENES[n]


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


@pytest.mark.parametrize("n", [257, 1025])
@pytest.mark.parametrize("n_views", [1, 2, 3, 5, 16])
def test_both_equivalences(n, n_views):
    s, boxes = _scene_of(n)
    planes, bases, cams = cv.frusta(s["planes"], n_views), cv.view_bases(n_views, n), cv.view_cams(s, n_views)
    bitmaps = _bitmaps(s, planes)
    full = np.full((n + 31) // 32, 0xFFFFFFFF, np.uint32)
    for mode in (lr.DISTANCE, lr.RELATIVE):
        sw = cv.metric_thresholds(s, mode)
        stride = 40 * n
        got = cvlr.list_clusters_views(s, boxes, planes, bitmaps, bases, mode, sw, stride, cam_pos=cams[0])
        assert got["status"] == 0 and int(got["stats"][0]) == got["items"]["W"] > 0
        for v in range(n_views):
            # (a) one mip_list_clusters per view, with frames[0]'s camera
            one = clr.list_clusters(dict(s, planes=planes[v], cam_pos=cams[0]), boxes, full if bitmaps[v] is None else bitmaps[v], mode, sw, stride,
                                    first_instance_base=bases[v])
            assert one["status"] == 0 and got["entries"][v].tobytes() == one["entries"].tobytes(), (n, n_views, mode, v)
            assert int(got["counts"][v]) == one["count"] and int(got["stats"][2 + v]) == int(one["stats"][0])
            assert got["args"][v].tolist() == [192, one["count"], 0, v * stride]
            # (b) the expansion of the several-view call's commands
            assert got["entries"][v].tobytes() == clr.from_commands(got["views"]["all_cmds"][v], s["meshes"]).tobytes()
            assert int(got["stats"][2 + v]) == got["views"]["survivors"][v]
        assert got["stats"][:2].tolist() == got["views"]["stats"][:2].tolist()
        if n_views >= 2:                     # the last view's base is 2^32 - n / 2: base + i wraps inside the scene
            inst = got["entries"][n_views - 1]["instance"]
            assert ((inst < n) | (inst >= (1 << 32) - n)).all()
            if n_views == 2:
                assert (inst < n).any() and (inst >= (1 << 32) - n).any()
        if n == 257 and n_views in (3, 16):  # the launches' steps, with a small list tile so that the scene spans several
            steps = cvlr.entries_by_steps(got["items"], got["survive"], s["meshes"], bases, stride, tile_words=4, pad=0)
            for v in range(n_views):
                c = int(got["counts"][v])
                assert steps["entries"][v * stride: v * stride + c].tobytes() == got["entries"][v].tobytes()
                assert (steps["entries"]["index_count"][v * stride + c: (v + 1) * stride] == 0xFFFFFFFF).all()
            assert steps["stats"].tolist() == got["stats"].tolist() and steps["args"].tolist() == got["args"].tolist()


def test_known_survivors_of_config_3():
    for n in (257, 1025):
        s, boxes = _scene_of(n)
        known = cv.KNOWN[n]
        got = cvlr.list_clusters_views(s, boxes, cv.frusta(s["planes"], 6), [None] * 6, [0] * 6, lr.DISTANCE, lr.PIN_SWITCH_SQ, 1 << 20)
        assert got["stats"].tolist() == [known["W"], known["members"]] + [sv for _, sv in known["views"]]


# ---- the overflow rules, per view; untouched entries keep the sentinel ----

def test_overflow_rules_per_view():
    s, boxes = _scene_of(257)
    planes, bases = cv.frusta(s["planes"], 3), cv.view_bases(3)
    args = (s, boxes, planes, _bitmaps(s, planes), bases, lr.DISTANCE, lr.PIN_SWITCH_SQ)
    full = cvlr.list_clusters_views(*args, 1 << 20)
    sv, w, members = full["stats"][2:].tolist(), int(full["stats"][0]), int(full["stats"][1])
    assert full["status"] == 0 and min(sv) > 2 and len(set(sv)) > 1
    big, small = int(np.argmax(sv)), int(np.argmin(sv))
    # ENTRY OVERFLOW: a stride one below the largest view's survivors: that view is cut, the others are complete, the stats are true
    stride = sv[big] - 1
    cut = cvlr.list_clusters_views(*args, stride)
    assert cut["status"] == cvlr.ERR_CAPACITY and cut["stats"].tolist() == full["stats"].tolist()
    for v in range(3):
        count = min(sv[v], stride)
        assert int(cut["counts"][v]) == count and cut["entries"][v].tobytes() == full["entries"][v][:count].tobytes()
        assert cut["args"][v].tolist() == [192, count, 0, v * stride]
    assert int(cut["counts"][small]) == sv[small] and int(cut["counts"][big]) == stride
    none = cvlr.list_clusters_views(*args, 0)
    assert none["status"] == cvlr.ERR_CAPACITY and none["counts"].tolist() == [0, 0, 0] and none["stats"].tolist() == full["stats"].tolist()
    assert none["args"].tolist() == [[192, 0, 0, 0]] * 3
    fits = cvlr.list_clusters_views(*args, max(sv), work_capacity=w)      # survivors == stride and W == work_capacity fit
    assert fits["status"] == 0 and all(fits["entries"][v].tobytes() == full["entries"][v].tobytes() for v in range(3))
    # WORK OVERFLOW: zero counts, {192, 0, 0, v x stride}, {W, members, 0, ...}, no entry
    work = cvlr.list_clusters_views(*args, 1000, work_capacity=w - 1)
    assert work["status"] == cvlr.ERR_CAPACITY and work["counts"].tolist() == [0, 0, 0] and all(len(e) == 0 for e in work["entries"])
    assert work["stats"].tolist() == [w, members, 0, 0, 0] and work["args"].tolist() == [[192, 0, 0, 0], [192, 0, 0, 1000], [192, 0, 0, 2000]]
    # N = 0
    empty = cvlr.list_clusters_views(dict(s, pos=s["pos"][:0], rot=s["rot"][:0], scale=s["scale"][:0], mesh_id=s["mesh_id"][:0]), boxes, planes,
                                     [None] * 3, bases, lr.DISTANCE, lr.PIN_SWITCH_SQ, 4)
    assert empty["status"] == 0 and empty["counts"].tolist() == [0, 0, 0] and empty["stats"].tolist() == [0] * 5
    assert empty["args"].tolist() == [[192, 0, 0, 0], [192, 0, 0, 4], [192, 0, 0, 8]]
    # what a sentinel-filled buffer holds afterwards: every entry at or behind a view's count, and the pad, untouched
    filled = cvlr.fill_outputs(cut, 3, stride, SENTINEL, 3)
    for v in range(3):
        count = int(cut["counts"][v])
        assert (filled["entries"][v * stride + count: (v + 1) * stride] == SENTINEL).all()
        assert filled["entries"][v * stride: v * stride + count].tobytes() == full["entries"][v][:count].tobytes()
    assert (filled["entries"][3 * stride:] == SENTINEL).all() and (filled["counts"][3:] == SENTINEL).all()
    assert (filled["args"][12:] == SENTINEL).all() and (filled["stats"][5:] == SENTINEL).all()
    off = cvlr.fill_outputs(cut, 3, stride, SENTINEL, 3, args=False, stats=False)
    assert (off["args"] == SENTINEL).all() and (off["stats"] == SENTINEL).all()
    # the launches' steps cut every view at its own stride
    steps = cvlr.entries_by_steps(cut["items"], cut["survive"], s["meshes"], bases, stride, tile_words=4, pad=3)
    assert np.ascontiguousarray(steps["entries"]).view(np.uint32).reshape(-1, 4)[filled["entries"][:, 3] != SENTINEL].tobytes() == \
        filled["entries"][filled["entries"][:, 3] != SENTINEL].tobytes()
    assert (steps["entries"]["index_count"] != 0xFFFFFFFF).tolist() == (filled["entries"][:, 3] != SENTINEL).tolist()
    assert steps["counts"].tolist() == cut["counts"].tolist()


# ---- the likely mistakes, each caught by a named scene ----

def _mutant_scenes():
    """{name: (scene, views)}; tile_words = 4 makes a list tile 256 items."""
    out = {}
    # three list tiles; the views' survivors differ word by word and tile by tile; a view that sees nothing stands in front of two that do
    s, views, _ = cvlc.ladder_views_list(["1" * 300, "10" * 150, "1" * 250], [0, 1, 2], [("A", None, 5), ("D", None, 6), ("B", None, 0xFFFFFFFF), ("C", None, 9)])
    out["three tiles under A, D, B, C"] = (s, views)
    by_name = {c[0]: c for c in CASES}
    out["four views of one ladder"] = by_name["four views of one ladder"][1:3]
    out["bitmaps {0}, {1}, {}, NULL"] = by_name["bitmaps {0}, {1}, {}, NULL"][1:3]
    return out


_KILLED_BY = {
    "word rank of view 0": "three tiles under A, D, B, C", "tile prefix of view 0": "three tiles under A, D, B, C",
    "base of view 0": "bitmaps {0}, {1}, {}, NULL", "firstInstance left 0": "four views of one ladder", "store offset dropped": "four views of one ladder",
    "cut applied to the sum over views": "four views of one ladder", "clear mask bit writes": "four views of one ladder",
    "zero word ends the view loop": "bitmaps {0}, {1}, {}, NULL", "lanes_below inclusive": "three tiles under A, D, B, C",
    "survivors where the heads were": "four views of one ladder",
}


def test_every_likely_mistake_is_caught_by_its_scene():
    assert set(_KILLED_BY) == set(cvlr.MUTANTS)
    scenes = _mutant_scenes()
    for mutant, name in _KILLED_BY.items():
        s, views = scenes[name]
        got = _owed(s, views, 1 << 12)
        stride = max(int(x) for x in got["stats"][2:]) + 1          # room for one entry more than the largest view's survivors
        got = _owed(s, views, stride)
        assert got["status"] == 0
        n_views = len(views["planes"])
        want = np.zeros(n_views * stride + 2, CLUSTER_ENTRY_DTYPE)
        want["index_count"] = 0xFFFFFFFF
        for v in range(n_views):
            want[v * stride: v * stride + len(got["entries"][v])] = got["entries"][v]
        good = cvlr.entries_by_steps(got["items"], got["survive"], s["meshes"], views["bases"], stride, tile_words=4)
        same = lambda r: (r["entries"].tobytes() == want.tobytes() and r["counts"].tolist() == got["counts"].tolist() and   # noqa: E731
                          r["args"].tolist() == got["args"].tolist() and r["stats"].tolist() == got["stats"].tolist())
        assert same(good), (name, "the header's rule")
        assert not same(cvlr.entries_by_steps(got["items"], got["survive"], s["meshes"], views["bases"], stride, mutant=mutant, tile_words=4)), \
            (mutant, "is not caught by", name)


# ---- the ABI ----

def test_struct_sizes_in_c_ctypes_and_rust(tmp_path):
    from renderer_amd import _lib as L

    O = MipClusterViewListOutputs
    assert L.MipClusterViewListOutputs is O
    want = [0, 4, 8, 16, 20, 24, 32, 40]
    assert C.sizeof(O) == 48 and [getattr(O, f).offset for f, _ in O._fields_] == want
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "mi_instance_pipeline.h"
    #define O(f) offsetof(MipClusterViewListOutputs, f)
    int main(void) {
      printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d\n", sizeof(MipClusterViewListOutputs), O(struct_size), O(flags), O(cluster_entries), O(entry_stride),
             O(work_capacity), O(entry_counts), O(draw_args), O(stats), (int)MIP_ABI_VERSION, (int)MIP_MAX_VIEWS);
      return 0; }'''
    c = tmp_path / "t.c"
    c.write_text(src)
    exe = str(tmp_path / "t")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe])
    assert [int(x) for x in subprocess.check_output([exe]).split()] == [48] + want + [4, 16]
    rust = open(os.path.join(ROOT, "integration", "rust", "mip-sys", "src", "lib.rs")).read()
    body = re.search(r"pub struct MipClusterViewListOutputs \{(.*?)\}", rust, flags=re.S).group(1)
    assert re.findall(r"pub (\w+): ([^,]+),", body) == [("struct_size", "u32"), ("flags", "u32"), ("cluster_entries", "*mut c_void"), ("entry_stride", "u32"),
                                                        ("work_capacity", "u32"), ("entry_counts", "*mut u32"), ("draw_args", "*mut u32"), ("stats", "*mut u32")]
    assert "#[repr(C)]" in rust[: rust.index("pub struct MipClusterViewListOutputs")].rsplit("\n\n", 1)[-1]
    assert "const _: [u8; 48] = [0; std::mem::size_of::<MipClusterViewListOutputs>()];" in rust


def test_header_exports_and_declarations_agree():
    from renderer_amd import _lib as L
    import renderer_amd

    name = "mip_list_clusters_views"
    text = open(HEADER).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    rust = open(os.path.join(ROOT, "integration", "rust", "mip-sys", "src", "lib.rs")).read()
    lib = L.load_library()
    assert name in L.EXPORTS and hasattr(lib, name)
    c_args = re.search(name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S).group(1).count(",") + 1
    assert c_args == 6 and len(getattr(lib, name).argtypes) == 6
    assert re.search(r"pub fn " + name + r"\((.*?)\)\s*->", rust, flags=re.S).group(1).count(",") + 1 == 6
    assert re.search(name + r"\([^;]*uint32_t n_views\s*,\s*const MipLodPolicy\* policy\s*,\s*const MipClusterViewListOutputs\* out\)", header)
    assert lib.mip_list_clusters_views(None, None, None, 1, None, None) == -1        # without a context: a status code
    assert "#define MIP_ABI_VERSION 4" in text
    # the new section stands behind mip_list_clusters' declaration and says what the issue lists
    start = text.index("visible-cluster lists for several views in one call")
    assert start > text.index("int32_t mip_list_clusters(MipContext* ctx")
    section = text[start: text.index("} MipClusterViewListOutputs;")]
    for word in ("ONE LOD FOR ALL VIEWS", "SURVIVES_v", "ENTRIES:", "v * entry_stride", "draw_args", "firstInstance", "gl_InstanceIndex", "THE CONSUMER",
                 "vkCmdDrawIndirect(cmd, draw_args, 16 * v, 1, 16)", "gl_DrawID", "THE TWO EQUIVALENCES", "(a)", "(b)", "ENTRY OVERFLOW", "WORK OVERFLOW",
                 "WHO REPORTS", "N = 0", "REFUSED", "16-byte aligned", "n_views x entry_stride >= 2^32", "MIP_ERR_NOT_READY", "ORDERING", "OUT OF SCOPE",
                 "one list packed tightly over all views"):
        assert word in section, word
    one = text[text.index("the visible-cluster list for one indirect draw"): text.index("} MipClusterEntry;")]
    assert "mip_list_clusters_views" in one[one.index("OUT OF SCOPE"):]
    wait = text[text.index("/* Block until everything enqueued"): text.index("int32_t mip_wait(MipContext* ctx);")]
    assert "mip_list_clusters_views" in wait
    assert callable(renderer_amd.make_cluster_view_list_outputs) and callable(renderer_amd.InstancePipeline.list_clusters_views)
    assert renderer_amd.make_cluster_view_list_outputs is make_cluster_view_list_outputs
    o = make_cluster_view_list_outputs(16, 5, 32, draw_args=48, stats=64, work_capacity=7, async_=True)
    assert (o.struct_size, o.flags, o.cluster_entries, o.entry_stride, o.work_capacity, o.entry_counts, o.draw_args, o.stats) == \
        (48, L.MIP_OUT_DEVICE | L.MIP_OUT_ASYNC, 16, 5, 7, 32, 48, 64)
    mk = open(os.path.join(ROOT, "renderer_amd", "csrc", "Makefile")).read()
    kernels = re.search(r"^KERNELS := (.*)$", mk, flags=re.M).group(1).split()
    assert "cluster_views_list_plan.hpp" in kernels and "cluster_views_list_kernel.hpp" in kernels
    smoke = open(os.path.join(ROOT, "integration", "c", "mip_smoke.c")).read()
    assert "mip_list_clusters_views(ctx" in smoke


def test_views_list_plan_over_its_decision_edges(tmp_path):
    exe = str(tmp_path / "cluster_views_list_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "native", "cluster_views_list_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    last = out.stdout.strip().split("\n")[-1]
    assert last.startswith("CLUSTER VIEWS LIST PLAN OK") and int(last.split()[5]) > 10000, out.stdout[-2000:]
