"""The visible-cluster list in two phases without a GPU: tests/cluster_list_phase_restatement.py (written from the header's
text) against the hand-written lists of tests/cluster_list_phase_cases.py and against the expansion of
cluster_phase_restatement's commands; its properties over config 3 under the wall, the same wall again, a cleared image and a
moved wall; the base arithmetic; every overflow and mismatch rule and N = 0; the mutants of the by-steps form, each killed by
a named scene; the ABI surface of mip_list_clusters_phase (C, ctypes, the Rust text, the header's words, EXPORTS, KERNELS); the
native check of renderer_amd/csrc/cluster_list_phase_plan.hpp, built with the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cluster_list_phase_cases as lpc
import cluster_list_phase_restatement as lp
import cluster_list_restatement as clr
import cluster_phase_cases as pc
import cluster_phase_restatement as pr
import cluster_restatement as cr
import lod_restatement as lr
import occlusion_restatement as orr
import test_cluster_phase_restatement as CP
from renderer_amd import _lib
from renderer_amd.pipeline import CLUSTER_ENTRY_DTYPE, cluster_record_bytes, make_cluster_phase_list_outputs

ROOT = CP.ROOT
HEADER = CP.HEADER
CASES = lpc.cases()
BIG = 1 << 30


def _hand_args(s):
    boxes = cr.cluster_boxes(s["meshes"], s["vertices"], s["indices"])
    assert np.array_equal(boxes, s["want_boxes"])
    return boxes, (s["bitmap"], lr.DISTANCE, pc.PIN)


def _both(s, want, appended, capacity=BIG):
    """(first, second) of the restatement over a hand-written scene: SECOND under the scene's other planes and new pyramid, at
    base 0 or (appended) at base = FIRST's count."""
    boxes, rest = _hand_args(s)
    f = lp.first(s, boxes, *rest, capacity, pc.occlusion_of(s, s["old_depth"]), first_instance_base=s["base"])
    g = lp.second(dict(s, planes=s["second_planes"]), boxes, *rest, capacity, pc.occlusion_of(s, want["new_depth"]), f["record"],
                  b=f["count"] if appended else 0, first_instance_base=s["base"])
    return f, g


# ---- 1. the hand-written scenes, byte for byte ----

@pytest.mark.parametrize("appended", [False, True], ids=["base 0", "base = FIRST's count"])
@pytest.mark.parametrize("name,s,want", CASES, ids=[c[0] for c in CASES])
def test_hand_cases_against_the_restatement(name, s, want, appended):
    f, g = _both(s, want, appended)
    assert f["status"] == 0 and g["status"] == 0
    n1, n2 = len(want["first"]["entries"]), len(want["second"]["entries"])
    assert f["entries"].tobytes() == want["first"]["entries"].tobytes(), (name, f["entries"])
    assert f["stats"].tolist() == want["first"]["stats"].tolist() and f["count"] == n1 and f["args"].tolist() == [192, n1, 0, 0]
    assert f["record"].tolist() == want["record"].tolist(), (name, f["record"])
    assert g["entries"].tobytes() == want["second"]["entries"].tobytes(), (name, g["entries"])
    b = n1 if appended else 0
    assert g["stats"].tolist() == want["second"]["stats"].tolist() and g["count"] == n2 and g["args"].tolist() == [192, n2, 0, b] and g["b"] == b
    if appended:   # one buffer: FIRST's entries, SECOND's straight behind them
        buf = lp.buffer_of([f, g], n1 + n2)
        assert buf[: n1 + n2].tobytes() == np.concatenate([want["first"]["entries"], want["second"]["entries"]]).tobytes()
        assert (buf["index_count"][n1 + n2:] == 0xFFFFFFFF).all()
    # the by-steps form writes the same buffer, with the library's tile and with a tile of one word
    boxes, rest = _hand_args(s)
    for tile_words in (clr.LIST_TILE_WORDS, 1):
        a = lp.by_steps("first", s, boxes, *rest, n1 + n2, pc.occlusion_of(s, s["old_depth"]), first_instance_base=s["base"], tile_words=tile_words)
        z = lp.by_steps("second", dict(s, planes=s["second_planes"]), boxes, *rest, n1 + n2, pc.occlusion_of(s, want["new_depth"]), b=b, record=a["record"],
                        first_instance_base=s["base"], tile_words=tile_words, buf=a["buf"] if appended else None)
        assert a["record"].tolist() == want["record"].tolist() and a["stats"].tolist() == f["stats"].tolist() and a["args"].tolist() == f["args"].tolist()
        assert z["stats"].tolist() == g["stats"].tolist() and z["args"].tolist() == g["args"].tolist() and z["count"] == g["count"]
        assert z["buf"].tobytes() == (lp.buffer_of([f, g], n1 + n2) if appended else lp.buffer_of([g], n1 + n2)).tobytes()


@pytest.mark.parametrize("name,s,want", CASES, ids=[c[0] for c in CASES])
def test_hand_cases_against_the_expansion_of_the_phase_commands(name, s, want):
    boxes, rest = _hand_args(s)
    f = pr.first(s, boxes, *rest, BIG, pc.occlusion_of(s, s["old_depth"]), first_instance_base=s["base"])
    g = pr.second(dict(s, planes=s["second_planes"]), boxes, *rest, BIG, pc.occlusion_of(s, want["new_depth"]), f["record"], first_instance_base=s["base"])
    assert clr.from_commands(f["cmds"], None).tobytes() == want["first"]["entries"].tobytes()
    assert clr.from_commands(g["cmds"], None).tobytes() == want["second"]["entries"].tobytes()
    assert f["record"].tolist() == want["record"].tolist()
    # FIRST's entries are mip_list_clusters' under the old pyramid
    plain = clr.list_clusters(s, boxes, *rest, BIG, first_instance_base=s["base"], occlusion=pc.occlusion_of(s, s["old_depth"]))
    assert plain["entries"].tobytes() == want["first"]["entries"].tobytes() and plain["stats"].tolist() == want["first"]["stats"][:3].tolist()


def test_hand_cases_cover_what_they_claim():
    by = {c[0]: c[2] for c in CASES}
    assert len(CASES) == 9 and [c[0] for c in pc.cases()].__len__() == 9
    assert by["a candidate at c = C - 1, short"]["second"]["entries"]["index_count"].tolist() == [15]
    assert by["c = 1 of C = 3"]["second"]["entries"]["first_index"].tolist() == [192] and by["c = 1 of C = 3"]["first"]["entries"]["instance"].tolist() == [0xFFFFFFFF] * 2
    assert by["a run across items 63 | 64"]["record"][4:].tolist() == [0, 1 << 31, 1, 0]
    assert by["a full word before a zero word"]["record"][4:].tolist() == [0xFFFFFFFF, 0xFFFFFFFF, 0, 0]
    assert len(by["every item"]["first"]["entries"]) == 0 and len(by["none"]["second"]["entries"]) == 0
    assert by["two instances meet"]["second"]["entries"]["instance"].tolist() == [9, 10]
    assert int(by["a still-hidden candidate between two visible ones"]["second"]["stats"][0]) == 2
    for name, s, want in CASES:   # the scenes are those of cluster_phase_cases, in its order
        assert any(np.array_equal(s["mesh_id"], t["mesh_id"]) and want["record"].tolist() == w["record"].tolist() for _, t, w in pc.cases()), name


# ---- 2. properties over the repository's scenes ----

@pytest.mark.parametrize("ordering,n", [("strips", 257), ("rows", 1025)])
def test_properties_over_config_3(ordering, n):
    s, boxes, bitmap = CP.config3(n, ordering)
    args = (s, boxes, bitmap, lr.DISTANCE, lr.PIN_SWITCH_SQ, BIG)
    old = CP.occlusion(CP.wall_depth())
    f = lp.first(*args, old, first_instance_base=11)
    pf = pr.first(*args, old, first_instance_base=11)
    listed = clr.list_clusters(*args, first_instance_base=11, occlusion=old)
    assert f["status"] == 0 and f["entries"].tobytes() == listed["entries"].tobytes() and f["stats"][:3].tolist() == listed["stats"].tolist()
    assert f["record"].tobytes() == pf["record"].tobytes() and int(f["stats"][3]) == int(pf["record"][2]) > 0
    assert clr.from_commands(pf["cmds"], None).tobytes() == f["entries"].tobytes()
    w, members, candidates = int(f["stats"][1]), int(f["stats"][2]), int(f["stats"][3])
    key = lambda e: set(zip(e["instance"].tolist(), e["first_index"].tolist()))
    # SECOND under the same pyramid is empty
    same = lp.second(*args, old, f["record"], b=f["count"], first_instance_base=11)
    assert same["status"] == 0 and same["count"] == 0 and same["stats"].tolist() == [0, w, members, candidates] and same["args"].tolist() == [192, 0, 0, f["count"]]
    # SECOND under a cleared image yields the candidates; with FIRST's the list without a pyramid
    clear = lp.second(*args, CP.occlusion(np.ones((32, 64), np.float32)), f["record"], b=f["count"], first_instance_base=11)
    assert np.array_equal(clear["survive"], pr.unpack_record(f["record"], w)) and clear["count"] == candidates
    free = clr.list_clusters(*args, first_instance_base=11)
    assert not (key(f["entries"]) & key(clear["entries"])) and key(f["entries"]) | key(clear["entries"]) == key(free["entries"])
    assert len(free["entries"]) == f["count"] + clear["count"]
    # SECOND under the moved wall yields record & ~occluded_new
    moved = CP.occlusion(CP.wall_depth(16))
    m = lp.second(*args, moved, f["record"], b=f["count"], first_instance_base=11)
    mins, maxs = pr.world_boxes(m["items"], boxes, s["pos"], s["rot"], s["scale"])
    hidden_new = orr.occluded(np.concatenate([mins, maxs], axis=1), moved["pv"], moved["levels"], 64, 32)
    assert np.array_equal(m["survive"], pr.unpack_record(f["record"], w) & ~hidden_new) and 0 < m["count"] < candidates
    pm = pr.second(*args, moved, f["record"], first_instance_base=11)
    assert clr.from_commands(pm["cmds"], None).tobytes() == m["entries"].tobytes()
    # the planes of a SECOND call are not read
    other = lp.second(dict(s, planes=pc.SECOND_PLANES), boxes, bitmap, lr.DISTANCE, lr.PIN_SWITCH_SQ, BIG, moved, f["record"], b=f["count"], first_instance_base=11)
    assert other["entries"].tobytes() == m["entries"].tobytes()
    # the by-steps form, FIRST then SECOND appended in one buffer, with two tile sizes
    cap = f["count"] + m["count"]
    for tile_words in (clr.LIST_TILE_WORDS, 3):
        a = lp.by_steps("first", *args[:5], cap, old, first_instance_base=11, tile_words=tile_words)
        z = lp.by_steps("second", *args[:5], cap, moved, b=a["count"], record=a["record"], first_instance_base=11, tile_words=tile_words, buf=a["buf"])
        assert a["record"].tobytes() == f["record"].tobytes() and z["buf"].tobytes() == lp.buffer_of([f, m], cap).tobytes()


def test_base_arithmetic():
    s, boxes, bitmap = CP.config3(257, "strips")
    args = (s, boxes, bitmap, lr.DISTANCE, lr.PIN_SWITCH_SQ)
    old, clear = CP.occlusion(CP.wall_depth()), CP.occlusion(np.ones((32, 64), np.float32))
    f = lp.first(*args, BIG, old)
    full = lp.second(*args, BIG, clear, f["record"])
    survivors = full["count"]
    assert survivors > 3
    cap = survivors + 5
    # b = 0, the last base with room for all, one more, capacity - 1, capacity, capacity + 1, 2^32 - 1
    for b, room in ((0, cap), (5, survivors), (6, survivors - 1), (cap - 1, 1), (cap, 0), (cap + 1, 0), (0xFFFFFFFF, 0)):
        assert lp.room_of(b, cap) == room
        for phase, r in (("second", lp.second(*args, cap, clear, f["record"], b=b)), ("first", lp.first(*args, f["count"] + 5, old, b=b))):
            n_all = len(r["all_entries"])
            want_room = room if phase == "second" else lp.room_of(b, f["count"] + 5)
            count = min(n_all, want_room)
            assert r["count"] == count and r["args"].tolist() == [192, count, 0, b] and r["b"] == b and int(r["stats"][0]) == n_all
            assert r["status"] == (lp.ERR_CAPACITY if n_all > want_room else 0) and r["entries"].tobytes() == r["all_entries"][:count].tobytes()
            if phase == "first":
                assert r["record"].tobytes() == f["record"].tobytes()      # an entry overflow leaves the record whole
        steps = lp.by_steps("second", *args, cap, clear, b=b, record=f["record"])
        want = lp.second(*args, cap, clear, f["record"], b=b)
        assert steps["count"] == want["count"] and steps["args"].tolist() == want["args"].tolist() and steps["buf"].tobytes() == lp.buffer_of([want], cap).tobytes()


def test_overflows_the_record_that_is_not_the_calls_and_no_instances():
    s, boxes, bitmap = CP.config3(257, "strips")
    args = (s, boxes, bitmap, lr.DISTANCE, lr.PIN_SWITCH_SQ)
    old, clear = CP.occlusion(CP.wall_depth()), CP.occlusion(np.ones((32, 64), np.float32))
    f = lp.first(*args, BIG, old)
    w, members, candidates = (int(v) for v in f["stats"][1:])
    # WORK OVERFLOW: a record one word short, a work_capacity one short; exactly enough runs
    for kw in (dict(room_bytes=cluster_record_bytes(w) - 8), dict(work_capacity=w - 1)):
        r = lp.first(*args, BIG, old, b=9, **kw)
        assert r["status"] == lp.ERR_CAPACITY and r["count"] == 0 and r["args"].tolist() == [192, 0, 0, 9] and r["stats"].tolist() == [0, w, members, 0]
        assert r["record"].tolist() == [0xFFFFFFFF, 0, 0, 0] and len(r["entries"]) == 0
        r = lp.second(*args, BIG, clear, f["record"], b=9, **kw)
        assert r["status"] == lp.ERR_CAPACITY and r["count"] == 0 and r["args"].tolist() == [192, 0, 0, 9] and r["stats"].tolist() == [0, w, members, 0]
    exact = lp.first(*args, BIG, old, room_bytes=cluster_record_bytes(w), work_capacity=w)
    assert exact["status"] == 0 and exact["record"].tobytes() == f["record"].tobytes()
    # ENTRY OVERFLOW through the capacity and through the base: true stats, the first `room` entries, the record whole
    n1 = f["count"]
    for cap, b in ((n1 - 1, 0), (n1 + 3, 4), (0, 0), (n1, n1)):
        r = lp.first(*args, cap, old, b=b)
        room = lp.room_of(b, cap)
        assert r["status"] == lp.ERR_CAPACITY and r["count"] == room < n1 and r["stats"].tolist() == f["stats"].tolist()
        assert r["entries"].tobytes() == f["entries"][:room].tobytes() and r["record"].tobytes() == f["record"].tobytes()
    # NOT THIS CALL'S RECORD: another W; the same W and another member count
    bits = orr.bits_of(bitmap, 257).copy()
    bits[int(f["items"]["inst"][0])] = False
    r = lp.second(s, boxes, orr.bitmap_of(bits), lr.DISTANCE, lr.PIN_SWITCH_SQ, BIG, clear, f["record"], b=3)
    assert r["status"] == lp.ERR_DEVICE and r["count"] == 0 and r["args"].tolist() == [192, 0, 0, 3] and r["stats"][0] == 0 and r["stats"][3] == 0
    assert int(r["stats"][1]) != w and int(r["stats"][2]) == members - 1
    r = lp.second(s, boxes, CP.same_w_other_members(s, boxes, bitmap), lr.DISTANCE, lr.PIN_SWITCH_SQ, BIG, clear, f["record"])
    assert r["status"] == lp.ERR_DEVICE and int(r["stats"][1]) == w and int(r["stats"][2]) != members and r["count"] == 0
    # N = 0
    empty = dict(s, pos=s["pos"][:0], rot=s["rot"][:0], scale=s["scale"][:0], mesh_id=s["mesh_id"][:0])
    e = lp.first(empty, boxes, bitmap[:0], lr.DISTANCE, lr.PIN_SWITCH_SQ, 4, old, b=2)
    assert e["status"] == 0 and e["count"] == 0 and e["args"].tolist() == [192, 0, 0, 2] and e["stats"].tolist() == [0] * 4 and e["record"].tolist() == [0] * 4
    e = lp.second(empty, boxes, bitmap[:0], lr.DISTANCE, lr.PIN_SWITCH_SQ, 4, clear, e["record"], b=2)
    assert e["status"] == 0 and e["count"] == 0 and e["args"].tolist() == [192, 0, 0, 2] and e["stats"].tolist() == [0] * 4


# ---- 3. the mutants of the by-steps form ----

def _steps_bytes(s, want, mutant, cut=0):
    """Every byte a frame of the by-steps form leaves — FIRST at base 0, SECOND appended at FIRST's count — in a buffer `cut`
    entries short of both lists."""
    boxes, rest = _hand_args(s)
    cap = max(len(want["first"]["entries"]) + len(want["second"]["entries"]) - cut, 0)
    a = lp.by_steps("first", s, boxes, *rest, cap, pc.occlusion_of(s, s["old_depth"]), first_instance_base=s["base"], mutant=mutant)
    record = a["record"] if a["record"] is not None else np.full(len(want["record"]), 0xAAAAAAAA, np.uint32)   # what the caller's record held
    z = lp.by_steps("second", dict(s, planes=s["second_planes"]), boxes, *rest, cap, pc.occlusion_of(s, want["new_depth"]), b=a["count"], record=want["record"],
                    first_instance_base=s["base"], mutant=mutant, buf=a["buf"])
    return b"".join(x.tobytes() for x in (z["buf"], a["args"], a["stats"], record, z["args"], z["stats"])) + bytes([a["count"] & 255, z["count"] & 255])


KILLED_BY = {   # mutant -> (scene, entries the buffer is short of both lists)
    "base not added to the store": ("a candidate at c = 0", 0),
    "base not in firstInstance": ("a candidate at c = 0", 0),
    "room from capacity alone": ("c = 1 of C = 3", 1),
    "entry_count counted from 0": ("two instances meet", 0),
    "candidates from survive words": ("a candidate at c = 0", 0),
    "header not written on entry overflow": ("a run across items 63 | 64", 10),
    "SECOND tests planes": ("a candidate at c = C - 1, short", 0),
    "SECOND writes an item FIRST drew": ("a full word before a zero word", 0),
    "lanes_below inclusive": ("every item", 0),
    "word skipped by its last rank": ("a still-hidden candidate between two visible ones", 1),
}


@pytest.mark.parametrize("mutant", lp.MUTANTS)
def test_every_mutant_is_killed_by_its_scene(mutant):
    by = {c[0]: c for c in CASES}
    name, cut = KILLED_BY[mutant]
    _, s, want = by[name]
    assert _steps_bytes(s, want, mutant, cut) != _steps_bytes(s, want, None, cut), (mutant, name)
    if cut == 0:   # and the form without a mutant is the hand-written frame
        f, g = _both(s, want, True)
        n = f["count"] + g["count"]
        assert _steps_bytes(s, want, None)[: 16 * (n + 2)] == lp.buffer_of([f, g], n).tobytes()


def test_the_mutants_are_the_issues():
    assert set(KILLED_BY) == set(lp.MUTANTS) and len(lp.MUTANTS) == 10


# ---- 4. the surface and the plan ----

def test_structs_in_c_ctypes_and_rust(tmp_path):
    o = _lib.MipClusterPhaseListOutputs
    names = [f for f, _ in o._fields_]
    assert C.sizeof(o) == 56 and names == ["struct_size", "flags", "cluster_entries", "entry_capacity", "work_capacity", "entry_count", "draw_args", "stats", "entry_base"]
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "mi_instance_pipeline.h"
    int main(void) {
      printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %u\n", sizeof(MipClusterPhaseListOutputs), offsetof(MipClusterPhaseListOutputs, struct_size),
             offsetof(MipClusterPhaseListOutputs, flags), offsetof(MipClusterPhaseListOutputs, cluster_entries), offsetof(MipClusterPhaseListOutputs, entry_capacity),
             offsetof(MipClusterPhaseListOutputs, work_capacity), offsetof(MipClusterPhaseListOutputs, entry_count), offsetof(MipClusterPhaseListOutputs, draw_args),
             offsetof(MipClusterPhaseListOutputs, stats), offsetof(MipClusterPhaseListOutputs, entry_base), MIP_ABI_VERSION);
      return 0;
    }'''
    c = tmp_path / "t.c"
    c.write_text(src)
    exe = str(tmp_path / "t")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe])
    assert [int(x) for x in subprocess.check_output([exe]).split()] == [56] + [getattr(o, f).offset for f in names] + [4]
    rust = open(os.path.join(ROOT, "integration", "rust", "mip-sys", "src", "lib.rs")).read()
    body = re.search(r"pub struct MipClusterPhaseListOutputs \{(.*?)\}", rust, flags=re.S).group(1)
    assert re.findall(r"pub (\w+):", body) == names
    assert "const _: [u8; 56] = [0; std::mem::size_of::<MipClusterPhaseListOutputs>()];" in rust
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    c_args = re.search(r"mip_list_clusters_phase\s*\(([^;]*?)\)\s*;", header, flags=re.S).group(1).count(",") + 1
    r_args = re.search(r"pub fn mip_list_clusters_phase\((.*?)\)\s*->", rust, flags=re.S).group(1).count(",") + 1
    assert c_args == r_args == 7
    made = make_cluster_phase_list_outputs(0x1000, 7, 0x2000, 0x2010, 0x2020, work_capacity=9, async_=True, entry_base=0x3000)
    assert (made.struct_size, made.cluster_entries, made.entry_capacity, made.work_capacity, made.entry_count, made.draw_args, made.stats, made.entry_base) == \
        (56, 0x1000, 7, 9, 0x2000, 0x2010, 0x2020, 0x3000)
    assert made.flags == _lib.MIP_OUT_DEVICE | _lib.MIP_OUT_ASYNC and make_cluster_phase_list_outputs(0x1000, 7, 0x2000).entry_base is None


def test_header_words_exports_and_kernels():
    import renderer_amd

    text = open(HEADER).read()
    assert "mip_list_clusters_phase" in _lib.EXPORTS and re.search(r"\bmip_list_clusters_phase\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    lib = renderer_amd.load_library()
    assert lib.mip_list_clusters_phase(None, None, None, None, None, None, None) == -1     # without a context: a status code
    section = text[text.index("Extension: the visible-cluster list in two phases"): text.index("} MipClusterPhaseListOutputs;")]
    for word in ("NOT a reference", "BORROWED TERMS", "FIRST (", "SECOND (", "byte for byte", "accepted by SECOND of either call", "frame->planes is NOT read",
                 "never modified", "ENTRY BASE", "ON THE DEVICE", "FIRST call's entry_count", "room = entry_capacity - min(b, entry_capacity)", "[b, b + entry_count)",
                 "{192, entry_count, 0, b}", "gl_InstanceIndex", "{survivors, W, members, candidates}", "ENTRY OVERFLOW", "WORK OVERFLOW", "NOT THIS CALL'S RECORD",
                 "N = 0", "WHO REPORTS", "REFUSED", "not 4-byte aligned", "ORDERING", "THE FRAME", "OUT OF SCOPE", "an entry_base for mip_list_clusters"):
        assert word in section, word
    listed = text[text.index("the visible-cluster list for one indirect draw"): text.index("} MipClusterEntry;")]
    phased = text[text.index("Extension: cluster culling in two phases"): text.index("} MipClusterRecord;")]
    wait = text[text.index("Block until everything enqueued"): text.index("int32_t mip_wait(")]
    assert "mip_list_clusters_phase" in listed and "mip_list_clusters_phase" in phased and "mip_list_clusters_phase" in wait
    assert callable(renderer_amd.make_cluster_phase_list_outputs) and callable(renderer_amd.InstancePipeline.list_clusters_phase)
    mk = open(os.path.join(ROOT, "renderer_amd", "csrc", "Makefile")).read()
    kernels = re.search(r"^KERNELS := (.*)$", mk, flags=re.M).group(1).split()
    assert "cluster_list_phase_plan.hpp" in kernels and "cluster_list_phase_kernel.hpp" in kernels
    src = open(os.path.join(ROOT, "renderer_amd", "csrc", "cluster_list_phase_kernel.hpp")).read()
    for kernel in ("mip_cluster_list_phase_count_kernel", "mip_cluster_list_phase_epilogue_kernel", "mip_cluster_list_phase_write_kernel"):
        assert kernel in src, kernel
    assert "__syncthreads_count" not in src and "atomic" not in src.replace("cluster_raise", ""), "no workgroup waits for another"


def test_list_phase_plan_over_its_decision_edges(tmp_path):
    exe = str(tmp_path / "cluster_list_phase_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "native", "cluster_list_phase_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    last = out.stdout.strip().split("\n")[-1]
    assert last.startswith("CLUSTER LIST PHASE PLAN OK") and int(last.split()[5]) > 1000, out.stdout[-2000:]
