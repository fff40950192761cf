"""Cluster culling in two phases without a GPU: tests/cluster_phase_restatement.py (written from the header's text) — its
properties over config 3 under the wall pyramid, the same pyramid again, a cleared one and a moved wall; the hand-written scenes
of tests/cluster_phase_cases.py, byte for byte; the mutants those scenes must tell apart; the ABI surface of
mip_cull_clusters_phase / mip_cluster_record_bytes (C, ctypes, the Rust text, EXPORTS); the native check of what
renderer_amd/csrc/cluster_plan.hpp adds, built with the address and undefined-behaviour sanitizers."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import cluster_phase_cases as pc
import cluster_phase_restatement as pr
import cluster_restatement as cr
import lod_restatement as lr
import numpy_restatement as nr
import occlusion_restatement as orr
from renderer_amd import _lib, scene
from renderer_amd.pipeline import cluster_record_bytes, make_cluster_record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi_instance_pipeline.h")
CASES = pc.cases()
BIG = 1 << 30


def wall_depth(first_column=0):
    """The wall of test_the_pyramid_test_removes_clusters_behind_a_wall — the near plane over 32 of 64 columns — from `first_column` on."""
    depth = np.ones((32, 64), np.float32)
    depth[:, first_column : first_column + 32] = 0.0
    return depth


def occlusion(depth):
    return dict(pv=scene.default_pv(), levels=orr.pyramid_levels(depth), width=depth.shape[1], height=depth.shape[0])


@functools.lru_cache(maxsize=None)
def config3(n, ordering):
    s = scene.make_scene(3, n=n)
    vertices, indices = scene.make_geometry(s["meshes"], ordering)
    bitmap = orr.bitmap_of(~nr.run(s)["coarse_culled"])       # what a mip_run of the scene writes
    return s, cr.cluster_boxes(s["meshes"], vertices, indices), bitmap


def _args(s, boxes, bitmap):
    return (s, boxes, bitmap, lr.DISTANCE, lr.PIN_SWITCH_SQ, BIG)


def _expand(r, s, base=0):
    """The (i, c) every command of a result covers, in order; a run stays inside its instance's level."""
    items, t = r["items"], r["items"]["table"]
    covered = []
    for cmd in r["cmds"]:
        i = (int(cmd["firstInstance"]) - base) & 0xFFFFFFFF
        b = int(items["bucket"][i])
        k, l = int(t["mesh"][b]), int(t["lod"][b])
        c0, rem = divmod(int(cmd["firstIndex"]) - int(s["meshes"]["index_offset"][k, l]), 192)
        run = (int(cmd["indexCount"]) // 3 + 63) // 64
        assert rem == 0 and c0 + run <= int(t["C"][b]), "a run crosses its instance"
        assert int(cmd["indexCount"]) == 3 * (min(64 * (c0 + run), int(t["T"][b])) - 64 * c0)
        covered += [(i, c0 + j) for j in range(run)]
    return covered


# ---- 1. properties over the repository's scenes ----

@pytest.mark.parametrize("ordering,n", [("strips", 257), ("rows", 1025)])
def test_properties_over_config_3(ordering, n):
    s, boxes, bitmap = config3(n, ordering)
    old = occlusion(wall_depth())
    free = cr.cull_clusters(*_args(s, boxes, bitmap))
    walled = cr.cull_clusters(*_args(s, boxes, bitmap), occlusion=old)
    f = pr.first(*_args(s, boxes, bitmap), old)
    # FIRST is mip_cull_clusters, and the record holds what the pyramid alone removed
    assert f["status"] == 0 and f["cmds"].tobytes() == walled["cmds"].tobytes() and f["count"] == walled["count"]
    assert f["stats"].tolist() == walled["stats"].tolist()
    w, members = int(f["stats"][2]), int(f["stats"][3])
    record = f["record"]
    assert record[:4].tolist() == [w, members, int(f["candidates"].sum()), 0] and len(record) == cluster_record_bytes(w) // 4
    assert int(record[2]) == int(free["stats"][1]) - int(walled["stats"][1]) > 0                       # the scene has candidates
    assert np.array_equal(pr.unpack_record(record, w), f["candidates"])
    words = record[4:].view(np.uint64)
    assert (words == 0).any() and (words != 0).any(), "zero words among non-zero ones"
    # SECOND under the same pyramid: every candidate is still hidden
    same = pr.second(*_args(s, boxes, bitmap), old, record)
    assert same["status"] == 0 and same["count"] == 0 and same["stats"].tolist() == [0, 0, w, members]
    # SECOND under a cleared pyramid: exactly the candidates, disjoint from FIRST's, together the survivors without a pyramid
    clear = pr.second(*_args(s, boxes, bitmap), occlusion(np.ones((32, 64), np.float32)), record)
    assert np.array_equal(clear["survive"], f["candidates"]) and not (clear["survive"] & f["survive"]).any()
    assert np.array_equal(clear["survive"] | f["survive"], free["survive"])
    # SECOND under the wall moved by a quarter of the width
    moved = occlusion(wall_depth(16))
    m = pr.second(*_args(s, boxes, bitmap), moved, record)
    mins, maxs = pr.world_boxes(m["items"], boxes, s["pos"], s["rot"], s["scale"])
    hidden_new = orr.occluded(np.concatenate([mins, maxs], axis=1), moved["pv"], moved["levels"], 64, 32)
    assert np.array_equal(m["survive"], f["candidates"] & ~hidden_new) and 0 < int(m["survive"].sum()) < int(f["candidates"].sum())
    covered = _expand(m, s)
    assert covered == [(int(i), int(c)) for i, c in zip(m["items"]["inst"][m["survive"]], m["items"]["cluster"][m["survive"]])]
    assert m["stats"].tolist() == [len(m["cmds"]), int(m["survive"].sum()), w, members]
    # an instance with a phase-2 run strictly inside it: neither its first nor its last cluster
    t = m["items"]["table"]
    inside = 0
    for cmd in m["cmds"]:
        i = int(cmd["firstInstance"])
        b = int(m["items"]["bucket"][i])
        c0 = (int(cmd["firstIndex"]) - int(s["meshes"]["index_offset"][int(t["mesh"][b]), int(t["lod"][b])])) // 192
        run = (int(cmd["indexCount"]) // 3 + 63) // 64
        inside += c0 > 0 and c0 + run < int(t["C"][b])
    assert inside >= 1
    # the planes of a SECOND call are not read
    other = pr.second(dict(s, planes=pc.SECOND_PLANES), boxes, bitmap, lr.DISTANCE, lr.PIN_SWITCH_SQ, BIG, moved, record)
    assert other["cmds"].tobytes() == m["cmds"].tobytes()


def test_overflows_and_the_record_that_is_not_the_calls():
    s, boxes, bitmap = config3(257, "strips")
    old, clear = occlusion(wall_depth()), occlusion(np.ones((32, 64), np.float32))
    f = pr.first(*_args(s, boxes, bitmap), old)
    w, members = int(f["stats"][2]), int(f["stats"][3])
    # FIRST: one word short is a work overflow with the refusal's header; exactly enough runs
    short = pr.first(*_args(s, boxes, bitmap), old, room_bytes=cluster_record_bytes(w) - 8)
    assert short["status"] == pr.ERR_CAPACITY and short["count"] == 0 and short["stats"].tolist() == [0, 0, w, members]
    assert short["record"].tolist() == [0xFFFFFFFF, 0, 0, 0]
    exact = pr.first(*_args(s, boxes, bitmap), old, room_bytes=cluster_record_bytes(w))
    assert exact["status"] == 0 and exact["record"].tobytes() == f["record"].tobytes()
    # a command overflow leaves the record complete
    heads = int(f["stats"][0])
    cut = pr.first(s, boxes, bitmap, lr.DISTANCE, lr.PIN_SWITCH_SQ, heads - 1, old)
    assert cut["status"] == pr.ERR_CAPACITY and cut["count"] == heads - 1 and cut["record"].tobytes() == f["record"].tobytes()
    # SECOND: the command overflow
    full = pr.second(*_args(s, boxes, bitmap), clear, f["record"])
    h2 = int(full["stats"][0])
    assert h2 > 2
    for cap in (h2 - 1, 0):
        c = pr.second(s, boxes, bitmap, lr.DISTANCE, lr.PIN_SWITCH_SQ, cap, clear, f["record"])
        assert c["status"] == pr.ERR_CAPACITY and c["count"] == cap and c["cmds"].tobytes() == full["cmds"][:cap].tobytes()
        assert c["stats"].tolist() == full["stats"].tolist()
    # another bitmap: another W; a bitmap with the same W and another member count
    bits = orr.bits_of(bitmap, 257).copy()
    items = f["items"]
    counts = np.bincount(items["inst"], minlength=257)
    drop = int(items["inst"][0])
    fewer = bits.copy()
    fewer[drop] = False
    r = pr.second(s, boxes, orr.bitmap_of(fewer), lr.DISTANCE, lr.PIN_SWITCH_SQ, BIG, clear, f["record"])
    assert r["status"] == pr.ERR_DEVICE and r["count"] == 0 and r["stats"].tolist() == [0, 0, w - int(counts[drop]), members - 1]
    same_w = same_w_other_members(s, boxes, bitmap)
    r = pr.second(s, boxes, same_w, lr.DISTANCE, lr.PIN_SWITCH_SQ, BIG, clear, f["record"])
    assert r["status"] == pr.ERR_DEVICE and r["count"] == 0 and int(r["stats"][2]) == w and int(r["stats"][3]) != members
    # N = 0
    empty = dict(s, pos=s["pos"][:0], rot=s["rot"][:0], scale=s["scale"][:0], mesh_id=s["mesh_id"][:0])
    e = pr.first(empty, boxes, bitmap[:0], lr.DISTANCE, lr.PIN_SWITCH_SQ, 4, old)
    assert e["status"] == 0 and e["count"] == 0 and e["stats"].tolist() == [0] * 4 and e["record"].tolist() == [0] * 4
    e = pr.second(empty, boxes, bitmap[:0], lr.DISTANCE, lr.PIN_SWITCH_SQ, 4, clear, e["record"])
    assert e["status"] == 0 and e["count"] == 0 and e["stats"].tolist() == [0] * 4


def same_w_other_members(s, boxes, bitmap):
    """A bitmap over the scene with the same W as `bitmap` and another member count: one member of a + b clusters is dropped
    and two instances outside the bitmap, of a and of b clusters, are set."""
    n = len(s["scale"])
    bits = orr.bits_of(bitmap, n).copy()
    every = cr.work_items(s["pos"], s["scale"], s["mesh_id"], s["meshes"], s["cam_pos"], orr.bitmap_of(np.ones(n, bool)), lr.DISTANCE, lr.PIN_SWITCH_SQ)
    c = np.bincount(every["inst"], minlength=n)
    outside = [i for i in range(n) if not bits[i] and c[i] > 0]
    for d in np.nonzero(bits & (c > 1))[0]:
        for a in outside:
            for b in outside:
                if a < b and c[a] + c[b] == c[d]:
                    bits[d], bits[a], bits[b] = False, True, True
                    return orr.bitmap_of(bits)
    raise AssertionError("no such bitmap in this scene")


# ---- 2. the hand-written scenes, byte for byte ----

def _both(s, want, mutant=None):
    """(first, second) of the restatement over a hand-written scene: SECOND under the scene's other planes and new pyramid."""
    boxes = cr.cluster_boxes(s["meshes"], s["vertices"], s["indices"])
    assert np.array_equal(boxes, s["want_boxes"])
    f = pr.first(s, boxes, s["bitmap"], lr.DISTANCE, pc.PIN, BIG, pc.occlusion_of(s, s["old_depth"]), first_instance_base=s["base"],
                 mutant=mutant if mutant and mutant.startswith("record") else None)
    g = pr.second(dict(s, planes=s["second_planes"]), boxes, s["bitmap"], lr.DISTANCE, pc.PIN, BIG, pc.occlusion_of(s, want["new_depth"]), f["record"],
                  first_instance_base=s["base"], mutant=None if mutant and mutant.startswith("record") else mutant, first_survive=f["survive"])
    return f, g


def _bytes(f, g):
    return f["cmds"].tobytes() + f["stats"].tobytes() + f["record"].tobytes() + g["cmds"].tobytes() + g["stats"].tobytes()


def _want_bytes(want):
    return want["first"]["cmds"].tobytes() + want["first"]["stats"].tobytes() + want["record"].tobytes() + want["second"]["cmds"].tobytes() + want["second"]["stats"].tobytes()


@pytest.mark.parametrize("name,s,want", CASES, ids=[c[0] for c in CASES])
def test_hand_cases_against_the_restatement(name, s, want):
    f, g = _both(s, want)
    assert f["status"] == 0 and g["status"] == 0
    assert f["cmds"].tobytes() == want["first"]["cmds"].tobytes(), (name, f["cmds"])
    assert f["stats"].tolist() == want["first"]["stats"].tolist(), (name, f["stats"])
    assert f["record"].tolist() == want["record"].tolist(), (name, f["record"])
    assert g["cmds"].tobytes() == want["second"]["cmds"].tobytes(), (name, g["cmds"])
    assert g["stats"].tolist() == want["second"]["stats"].tolist(), (name, g["stats"])
    # FIRST is the plain call under the old pyramid
    boxes = cr.cluster_boxes(s["meshes"], s["vertices"], s["indices"])
    plain = cr.cull_clusters(s, boxes, s["bitmap"], lr.DISTANCE, pc.PIN, BIG, first_instance_base=s["base"], occlusion=pc.occlusion_of(s, s["old_depth"]))
    assert plain["cmds"].tobytes() == want["first"]["cmds"].tobytes() and plain["stats"].tolist() == want["first"]["stats"].tolist()


def test_hand_cases_cover_what_they_claim():
    by = {c[0]: c for c in CASES}
    assert len(CASES) == 9
    assert len(by["c = 1 of C = 3"][2]["first"]["cmds"]) == 2 and by["c = 1 of C = 3"][2]["second"]["cmds"]["firstIndex"].tolist() == [192]
    assert len(by["candidates meet across an instance boundary"][2]["second"]["cmds"]) == 2
    assert by["a run across items 63 | 64"][2]["record"][4:].tolist() == [0, 1 << 31, 1, 0]
    assert by["a whole word, then a zero word"][2]["record"][4:].tolist() == [0xFFFFFFFF, 0xFFFFFFFF, 0, 0]
    assert int(by["every item a candidate"][2]["record"][2]) == 6 and int(by["no candidates"][2]["record"][2]) == 0
    assert int(by["a candidate the new pyramid still hides"][2]["second"]["stats"][1]) == 2
    # the planes SECOND is given accept nothing
    s = CASES[0][1]
    boxes = cr.cluster_boxes(s["meshes"], s["vertices"], s["indices"])
    items = cr.work_items(s["pos"], s["scale"], s["mesh_id"], s["meshes"], s["cam_pos"], s["bitmap"], lr.DISTANCE, pc.PIN)
    mins, maxs = pr.world_boxes(items, boxes, s["pos"], s["rot"], s["scale"])
    assert nr.coarse_culled(mins, maxs, s["second_planes"]).all() and not nr.coarse_culled(mins, maxs, s["planes"]).any()
    assert np.array_equal(np.concatenate([mins, maxs], axis=1), boxes[items["box_index"]])           # the world box is the cluster's box


# ---- 3. the mutants ----

@pytest.mark.parametrize("mutant", pr.MUTANTS)
def test_every_mutant_changes_a_byte_of_some_scene(mutant):
    changed = [name for name, s, want in CASES if _bytes(*_both(s, want, mutant)) != _want_bytes(want)]
    assert changed, mutant


# ---- 4. the surface and the plan ----

def test_structs_in_c_ctypes_and_rust(tmp_path):
    r = _lib.MipClusterRecord
    assert C.sizeof(r) == 24 and (_lib.MIP_CLUSTER_PHASE_FIRST, _lib.MIP_CLUSTER_PHASE_SECOND) == (1, 2)
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "mi_instance_pipeline.h"
    int main(void) {
      printf("%zu %zu %zu %zu %u %u\n", sizeof(MipClusterRecord), offsetof(MipClusterRecord, phase), offsetof(MipClusterRecord, record),
             offsetof(MipClusterRecord, record_bytes), MIP_CLUSTER_PHASE_FIRST, MIP_CLUSTER_PHASE_SECOND);
      return 0;
    }'''
    c = tmp_path / "t.c"
    c.write_text(src)
    exe = str(tmp_path / "t")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe])
    assert [int(x) for x in subprocess.check_output([exe]).split()] == [C.sizeof(r), r.phase.offset, r.record.offset, r.record_bytes.offset, 1, 2]
    rust = open(os.path.join(ROOT, "integration", "rust", "mip-sys", "src", "lib.rs")).read()
    body = re.search(r"pub struct MipClusterRecord \{(.*?)\}", rust, flags=re.S).group(1)
    assert re.findall(r"pub (\w+):", body) == [f for f, _ in r._fields_]
    assert "const _: [u8; 24] = [0; std::mem::size_of::<MipClusterRecord>()];" in rust
    assert "pub const MIP_CLUSTER_PHASE_FIRST: u32 = 1;" in rust and "pub const MIP_CLUSTER_PHASE_SECOND: u32 = 2;" in rust
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for fn in ("mip_cluster_record_bytes", "mip_cull_clusters_phase"):
        c_args = re.search(fn + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S).group(1).count(",") + 1
        r_args = re.search(r"pub fn " + fn + r"\((.*?)\)\s*->", rust, flags=re.S).group(1).count(",") + 1
        assert c_args == r_args, (fn, c_args, r_args)
    rec = make_cluster_record("second", 0x1000, 4096)
    assert (rec.struct_size, rec.phase, rec.record, rec.record_bytes) == (24, 2, 0x1000, 4096)


def test_header_exports_and_the_record_size():
    text = open(HEADER).read()
    for fn in ("mip_cluster_record_bytes", "mip_cull_clusters_phase"):
        assert fn in _lib.EXPORTS and re.search(r"\b" + fn + r"\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    spec = text[text.index("Extension: cluster culling in two phases"):text.index("MipClusterRecord;")]
    assert "NOT a reference" in spec and "sanity" in spec
    import renderer_amd
    lib = renderer_amd.load_library()
    for w, want in ((0, 16), (1, 24), (64, 24), (65, 32), ((1 << 32) - 1, 16 + 8 * (1 << 26))):
        assert lib.mip_cluster_record_bytes(w) == want == cluster_record_bytes(w) == pr.record_bytes(w), w
    assert lib.mip_cull_clusters_phase(None, None, None, None, None, None, None) == -1


def test_phase_plan_over_its_decision_edges(tmp_path):
    exe = str(tmp_path / "cluster_phase_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "native", "cluster_phase_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    last = out.stdout.strip().split("\n")[-1]
    assert last.startswith("CLUSTER PHASE PLAN OK") and int(last.split()[4]) > 50_000, out.stdout[-2000:]
