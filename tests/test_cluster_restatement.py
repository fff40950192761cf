"""Cluster culling without a GPU: tests/cluster_restatement.py (written from the header's text) against the hand-written
scenes of tests/cluster_cases.py, its own properties over config 3 under the three geometry layouts, both overflow rules; the
ABI surface of mip_build_clusters / mip_cull_clusters (C, ctypes, the Rust text, EXPORTS); the native check of
renderer_amd/csrc/cluster_plan.hpp, built with the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cluster_cases as cc
import cluster_restatement as cr
import lod_restatement as lr
import numpy_restatement as nr
import occlusion_restatement as orr
from renderer_amd import _lib, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi_instance_pipeline.h")
CASES = cc.cases()


def _frame_bitmap(s):
    """The visibility bitmap a mip_run of the scene writes (the instance boxes against the planes)."""
    return orr.bitmap_of(~nr.run(s)["coarse_culled"])


def _config3(n, ordering):
    s = scene.make_scene(3, n=n)
    vertices, indices = scene.make_geometry(s["meshes"], ordering)
    return s, cr.cluster_boxes(s["meshes"], vertices, indices)


# ---- the hand-written scenes ----

@pytest.mark.parametrize("name,s,want", CASES, ids=[c[0] for c in CASES])
def test_hand_cases_against_the_restatement(name, s, want):
    boxes = cr.cluster_boxes(s["meshes"], s["vertices"], s["indices"])
    got = cr.cull_clusters(s, boxes, s["bitmap"], lr.DISTANCE, cc.PIN, cmd_capacity=1 << 20, first_instance_base=s["base"])
    assert got["status"] == 0
    assert got["cmds"].tobytes() == want["cmds"].tobytes(), (name, got["cmds"], want["cmds"])
    assert got["stats"].tolist() == want["stats"].tolist(), (name, got["stats"])
    assert got["count"] == len(want["cmds"])


def test_hand_cases_cover_what_they_claim():
    by_name = {c[0]: c for c in CASES}
    assert len(by_name["alternating"][2]["cmds"]) == (7 + 1) // 2
    assert by_name["all survive"][2]["cmds"]["indexCount"].tolist() == [600]           # 3 T
    assert len(by_name["two instances"][2]["cmds"]) == 2
    boxes = cr.cluster_boxes(by_name["tangent"][1]["meshes"], by_name["tangent"][1]["vertices"], by_name["tangent"][1]["indices"])
    assert boxes[0].tolist() == [8, 0, 0, 9, 1, 0] and boxes[1, 0] == np.nextafter(np.float32(8), np.float32(9)) and boxes[1, 3] > 9
    s = by_name["tangent"][1]
    model = nr.model_matrices(s["pos"][[0, 0]], s["rot"][[0, 0]], s["scale"][[0, 0]])
    mins, maxs = nr.world_aabbs(model, boxes[:, :3], boxes[:, 3:])
    margins = nr.plane_margins(mins, maxs, s["planes"])
    assert margins[0, 0] == 0.0 and 0.0 < margins[1, 0] < 1e-6                          # exactly tangent; one float outside
    nan = cr.cluster_boxes(by_name["NaN cluster"][1]["meshes"], by_name["NaN cluster"][1]["vertices"], by_name["NaN cluster"][1]["indices"])
    assert nan[0].tolist() == [np.inf] * 3 + [-np.inf] * 3                             # the fold's start values


# ---- properties over the repository's own scenes ----

@pytest.mark.parametrize("ordering,n", [("strips", 257), ("rows", 1025), ("shuffled", 1025)])
def test_properties_of_the_restatement(ordering, n):
    s, boxes = _config3(n, ordering)
    bitmap = _frame_bitmap(s)
    r = cr.cull_clusters(s, boxes, bitmap, lr.DISTANCE, lr.PIN_SWITCH_SQ, cmd_capacity=1 << 30, first_instance_base=11)
    items, sv, cmds, t = r["items"], r["survive"], r["cmds"], r["items"]["table"]
    assert r["status"] == 0 and items["W"] == len(sv) > 0
    inst = (cmds["firstInstance"].astype(np.int64) - 11) & 0xFFFFFFFF
    # commands tile the survivors: expanding every command's clusters gives exactly the surviving (i, c), in order
    covered = []
    for k in range(len(cmds)):
        i = int(inst[k])
        b = int(items["bucket"][i])
        kmesh, klod = int(t["mesh"][b]), int(t["lod"][b])
        c0, rem = divmod(int(cmds["firstIndex"][k]) - int(s["meshes"]["index_offset"][kmesh, klod]), 192)
        assert rem == 0 and cmds["instanceCount"][k] == 1 and cmds["vertexOffset"][k] == s["meshes"]["vertex_offset"][kmesh]
        tris = int(cmds["indexCount"][k]) // 3
        run = (tris + 63) // 64
        assert int(cmds["indexCount"][k]) == 3 * (min(64 * (c0 + run), int(t["T"][b])) - 64 * c0)
        covered += [(i, c0 + j) for j in range(run)]                                   # a run never crosses an instance: one i
    assert covered == [(int(i), int(c)) for i, c in zip(items["inst"][sv], items["cluster"][sv])]
    # the triangles of the commands are the triangles of the survivors
    b_item = items["bucket"][items["inst"]]
    tri_item = np.minimum(64 * (items["cluster"] + 1), t["T"][b_item]) - 64 * items["cluster"]
    assert int(cmds["indexCount"].astype(np.int64).sum()) // 3 == int(tri_item[sv].sum())
    # an instance the frame culled never appears; no two commands of one instance are neighbours in c
    assert orr.bits_of(bitmap, n)[inst].all()
    assert r["stats"].tolist() == [len(cmds), int(sv.sum()), items["W"], items["members"]]


def test_the_scene_the_gpu_test_relies_on_exercises_the_feature():
    """config 3, n = 257, "strips", the frame's bitmap, the pin policy: survivors < W, members without a survivor, commands !=
    members — what tests/test_gpu_clusters.py asserts of the device's answer for the same scene. (72 members, 3 127 work items,
    2 581 survivors, 71 commands; two members have no surviving cluster and one has two runs.)"""
    s, boxes = _config3(257, "strips")
    r = cr.cull_clusters(s, boxes, _frame_bitmap(s), lr.DISTANCE, lr.PIN_SWITCH_SQ, cmd_capacity=1 << 30)
    heads, survivors, w, members = (int(v) for v in r["stats"])
    assert (members, w, survivors, heads) == (72, 3127, 2581, 71)
    with_survivor = np.unique(r["items"]["inst"][r["survive"]])
    assert members - len(with_survivor) == 2 and survivors < w and heads != members


def test_cluster_boxes_contain_their_triangles_and_tile_the_level():
    s = scene.make_scene(3, n=1)
    vertices, indices = scene.make_geometry(s["meshes"], "strips")
    boxes, t = cr.cluster_boxes(s["meshes"], vertices, indices), cr.cluster_table(s["meshes"])
    assert len(boxes) == int(t["base"][-1]) == int(t["C"].sum()) and len(t["mesh"]) == int(s["meshes"]["n_lods"].sum())
    for b in (0, len(t["mesh"]) // 2, len(t["mesh"]) - 1):
        k, l = int(t["mesh"][b]), int(t["lod"][b])
        off = int(s["meshes"]["index_offset"][k, l])
        v = vertices[indices[off : off + 3 * int(t["T"][b])].astype(np.int64) + int(s["meshes"]["vertex_offset"][k])]
        own = boxes[int(t["base"][b]) : int(t["base"][b + 1])]
        assert np.array_equal(own[:, :3].min(axis=0), v.min(axis=0)) and np.array_equal(own[:, 3:].max(axis=0), v.max(axis=0))


# ---- the overflow rules ----

def test_overflow_rules():
    s, boxes = _config3(257, "strips")
    bitmap = _frame_bitmap(s)
    full = cr.cull_clusters(s, boxes, bitmap, lr.DISTANCE, lr.PIN_SWITCH_SQ, cmd_capacity=1 << 30)
    heads, w = int(full["stats"][0]), int(full["stats"][2])
    cut = cr.cull_clusters(s, boxes, bitmap, lr.DISTANCE, lr.PIN_SWITCH_SQ, cmd_capacity=heads - 1)
    assert cut["status"] == cr.ERR_CAPACITY and cut["count"] == heads - 1 and cut["cmds"].tobytes() == full["cmds"][: heads - 1].tobytes()
    assert cut["stats"].tolist() == full["stats"].tolist()
    none = cr.cull_clusters(s, boxes, bitmap, lr.DISTANCE, lr.PIN_SWITCH_SQ, cmd_capacity=0)
    assert none["status"] == cr.ERR_CAPACITY and none["count"] == 0 and none["stats"].tolist() == full["stats"].tolist()
    fits = cr.cull_clusters(s, boxes, bitmap, lr.DISTANCE, lr.PIN_SWITCH_SQ, cmd_capacity=heads, work_capacity=w)
    assert fits["status"] == 0 and fits["cmds"].tobytes() == full["cmds"].tobytes()
    work = cr.cull_clusters(s, boxes, bitmap, lr.DISTANCE, lr.PIN_SWITCH_SQ, cmd_capacity=1 << 30, work_capacity=w - 1)
    assert work["status"] == cr.ERR_CAPACITY and work["count"] == 0 and work["stats"].tolist() == [0, 0, w, int(full["stats"][3])]
    empty = cr.cull_clusters(dict(s, pos=s["pos"][:0], rot=s["rot"][:0], scale=s["scale"][:0], mesh_id=s["mesh_id"][:0]), boxes, bitmap[:0],
                             lr.DISTANCE, lr.PIN_SWITCH_SQ, cmd_capacity=4)
    assert empty["status"] == 0 and empty["count"] == 0 and empty["stats"].tolist() == [0, 0, 0, 0]


def test_the_pyramid_test_removes_clusters_behind_a_wall():
    s, boxes = _config3(1025, "rows")
    bitmap = _frame_bitmap(s)
    depth = np.ones((32, 64), np.float32)
    depth[:, :32] = 0.0                                                                 # a wall at the near plane over the left half
    occ = dict(pv=scene.default_pv(), levels=orr.pyramid_levels(depth), width=64, height=32)
    free = cr.cull_clusters(s, boxes, bitmap, lr.DISTANCE, lr.PIN_SWITCH_SQ, cmd_capacity=1 << 30)
    walled = cr.cull_clusters(s, boxes, bitmap, lr.DISTANCE, lr.PIN_SWITCH_SQ, cmd_capacity=1 << 30, occlusion=occ)
    assert 0 < int(walled["stats"][1]) < int(free["stats"][1]) and not (walled["survive"] & ~free["survive"]).any()


# ---- the ABI surface ----

def test_structs_in_c_ctypes_and_rust(tmp_path):
    assert C.sizeof(_lib.MipClusterOutputs) == 40 and _lib.MIP_CLUSTER_TRIANGLES == cr.CLUSTER_TRIANGLES == 64
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "mi_instance_pipeline.h"
    int main(void) {
      printf("%zu %zu %zu %zu %zu %zu %zu %u\n", sizeof(MipClusterOutputs), offsetof(MipClusterOutputs, flags), offsetof(MipClusterOutputs, cluster_cmds),
             offsetof(MipClusterOutputs, cmd_capacity), offsetof(MipClusterOutputs, work_capacity), offsetof(MipClusterOutputs, cmd_count),
             offsetof(MipClusterOutputs, stats), MIP_CLUSTER_TRIANGLES);
      return 0;
    }'''
    c = tmp_path / "t.c"
    c.write_text(src)
    exe = str(tmp_path / "t")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe])
    sizes = [int(x) for x in subprocess.check_output([exe]).split()]
    o = _lib.MipClusterOutputs
    assert sizes == [C.sizeof(o), o.flags.offset, o.cluster_cmds.offset, o.cmd_capacity.offset, o.work_capacity.offset, o.cmd_count.offset,
                     o.stats.offset, 64]
    rust = open(os.path.join(ROOT, "integration", "rust", "mip-sys", "src", "lib.rs")).read()
    body = re.search(r"pub struct MipClusterOutputs \{(.*?)\}", rust, flags=re.S).group(1)
    assert re.findall(r"pub (\w+):", body) == [f for f, _ in o._fields_]
    assert "const _: [u8; 40] = [0; std::mem::size_of::<MipClusterOutputs>()];" in rust
    assert "pub const MIP_CLUSTER_TRIANGLES: u32 = 64;" in rust
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for fn in ("mip_build_clusters", "mip_cluster_count", "mip_read_cluster_boxes", "mip_cull_clusters"):
        c_args = re.search(fn + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S).group(1).count(",") + 1
        r_args = re.search(r"pub fn " + fn + r"\((.*?)\)\s*->", rust, flags=re.S).group(1).count(",") + 1
        assert c_args == r_args, (fn, c_args, r_args)


def test_header_and_exports():
    text = open(HEADER).read()
    assert "#define MIP_ABI_VERSION 4u" in text
    for fn in ("mip_build_clusters", "mip_cluster_count", "mip_read_cluster_boxes", "mip_cull_clusters"):
        assert fn in _lib.EXPORTS and re.search(r"\b" + fn + r"\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert "NOT a reference" in text[text.index("Extension: cluster culling"):text.index("MipClusterOutputs;")]
    import renderer_amd
    lib = renderer_amd.load_library()
    assert lib.mip_cluster_count(None) == 0 and lib.mip_build_clusters(None) == -1
    assert lib.mip_read_cluster_boxes(None, None, 0) == -1 and lib.mip_cull_clusters(None, None, None, None, None, None) == -1


# ---- the plan ----

def test_cluster_plan_over_its_decision_edges(tmp_path):
    exe = str(tmp_path / "cluster_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "native", "cluster_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    last = out.stdout.strip().split("\n")[-1]
    assert last.startswith("CLUSTER PLAN OK") and int(last.split()[3]) > 100_000, out.stdout[-2000:]
