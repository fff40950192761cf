"""mip_list_clusters on the CPU (include/mi_instance_pipeline.h): the hand-written lists (tests/cluster_list_cases.py) against
the restatement (tests/cluster_list_restatement.py); the list against the expansion of cluster_restatement's commands on
every scene; the known survivor counts of config 3; both overflow rules; the structs in C, ctypes and the Rust text; the
header and the exports; the plan (renderer_amd/csrc/cluster_list_plan.hpp) over its edges under the host sanitizers; and
the likely mistakes of the rank and locate steps, each caught by a named scene."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cluster_cases as cc
import cluster_cone_restatement as ccr
import cluster_list_cases as clc
import cluster_list_restatement as clr
import cluster_restatement as cr
import lod_restatement as lr
import numpy_restatement as nr
import occlusion_restatement as orr
from renderer_amd.pipeline import CLUSTER_ENTRY_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
_CASES = clc.cases()


def _list(s, entry_capacity=1 << 30, work_capacity=0, base=None, **kw):
    boxes = cr.cluster_boxes(s["meshes"], s["vertices"], s["indices"])
    return clr.list_clusters(s, boxes, s["bitmap"], lr.DISTANCE, cc.PIN, entry_capacity, work_capacity, s["base"] if base is None else base, **kw)


def _triangles(got):
    """The triangles of the surviving work items, from the table."""
    it, t = got["items"], got["items"]["table"]
    sel = np.nonzero(got["survive"])[0]
    b = it["bucket"][it["inst"][sel]]
    return int(np.minimum(t["T"][b] - 64 * it["cluster"][sel], 64).sum())


# ---- the catalogue ----

@pytest.mark.parametrize("name,s,want", _CASES, ids=[c[0] for c in _CASES])
def test_hand_written_lists(name, s, want):
    got = _list(s)
    assert got["status"] == 0 and got["count"] == len(want["entries"])
    assert got["entries"].tobytes() == want["entries"].tobytes(), (name, got["entries"], want["entries"])
    assert got["stats"].tolist() == want["stats"].tolist() and got["args"].tolist() == [192, len(want["entries"]), 0, 0]
    # the list is the expansion of the commands, and of cluster_cases' hand-written commands
    assert clr.from_commands(got["plain"]["all_cmds"], s["meshes"]).tobytes() == want["entries"].tobytes()
    by_name = {c[0]: c[2] for c in cc.cases()}
    assert clr.from_commands(by_name[name]["cmds"], s["meshes"]).tobytes() == want["entries"].tobytes()
    assert int(want["entries"]["index_count"].sum()) // 3 == _triangles(got)
    # the kernels' steps give the same list
    buf, count = clr.entries_by_steps(got["items"], got["survive"], s["meshes"], s["base"], len(want["entries"]))
    assert count == len(want["entries"]) and buf[:count].tobytes() == want["entries"].tobytes() and (buf["index_count"][count:] == 0xFFFFFFFF).all()


def test_the_closed_form_of_a_ladder_is_the_restatement_s_list():
    patterns = ["1" * 70 + "0" * 3 + "1", "0101" * 40, "", np.arange(200) % 3 == 0]
    inst = [0, 1, 2, 3, 3, 0, 2, 1]
    bits = np.array([1, 1, 1, 0, 1, 1, 1, 1], bool)
    s, want_cmds = cc.ladder_scene(patterns, inst, base=0xFFFFFFFD, bits=bits)
    entries, stats = clc.ladder_want(patterns, inst, base=0xFFFFFFFD, bits=bits)
    got = _list(s)
    assert got["all_entries"].tobytes() == entries.tobytes() and got["stats"].tolist() == stats.tolist()
    assert clr.from_commands(want_cmds["cmds"], s["meshes"]).tobytes() == entries.tobytes()
    # the base wraps inside the scene; instance 3 (its bit is clear) and the instances of the empty ladder have no entry
    assert set(entries["instance"].tolist()) == {0xFFFFFFFD, 0xFFFFFFFE, 1, 2, 4}


# ---- config 3 ----

def test_the_known_counts_of_config_3():
    from renderer_amd import scene

    pv = scene.default_pv()
    _, eye, facing = ccr.cone_from_pv(pv)
    s = scene.make_scene(3, n=257)
    bitmap = orr.bitmap_of(~nr.run(s)["coarse_culled"])
    wall = np.ones((32, 64), F)
    wall[:, :32] = 0.0
    occlusion = dict(pv=pv, levels=orr.pyramid_levels(wall), width=64, height=32)
    for ordering, cone, survivors in (("strips", False, 2581), ("strips", True, 2578), ("patches", True, 1971)):
        vertices, indices = scene.make_geometry(s["meshes"], ordering)
        boxes = cr.cluster_boxes(s["meshes"], vertices, indices)
        k = dict(cones=ccr.cluster_cones(s["meshes"], vertices, indices, boxes), eye=eye, facing=facing) if cone else None
        got = clr.list_clusters(s, boxes, bitmap, lr.DISTANCE, lr.PIN_SWITCH_SQ, 1 << 20, first_instance_base=0xFFFFFF80, cone=k)
        assert got["status"] == 0 and got["stats"].tolist() == [survivors, 3127, 72] and got["count"] == survivors
        assert got["args"].tolist() == [192, survivors, 0, 0]
        assert got["entries"].tobytes() == clr.from_commands(got["plain"]["all_cmds"], s["meshes"]).tobytes()
        assert int(got["entries"]["index_count"].sum()) // 3 == _triangles(got)
        assert (got["entries"]["instance"] < 257).any() and (got["entries"]["instance"] >= 0xFFFFFF80).any()   # the base wraps
        buf, count = clr.entries_by_steps(got["items"], got["survive"], s["meshes"], 0xFFFFFF80, survivors, tile_words=4)
        assert count == survivors and buf[:count].tobytes() == got["entries"].tobytes()
        if ordering == "strips" and not cone:
            walled = clr.list_clusters(s, boxes, bitmap, lr.DISTANCE, lr.PIN_SWITCH_SQ, 1 << 20, occlusion=occlusion)
            assert 0 < walled["count"] < survivors
            assert walled["entries"].tobytes() == clr.from_commands(walled["plain"]["all_cmds"], s["meshes"]).tobytes()


# ---- both overflow rules, N = 0 ----

def test_overflow_rules_and_the_empty_scene():
    name, s, want = _CASES[[c[0] for c in _CASES].index("short last cluster")]
    for cap in (3, 0):                      # ENTRY OVERFLOW: the first `cap` entries, the true stats
        got = _list(s, entry_capacity=cap)
        assert got["status"] == clr.ERR_CAPACITY and got["count"] == cap and got["args"].tolist() == [192, cap, 0, 0]
        assert got["entries"].tobytes() == want["entries"][:cap].tobytes() and got["stats"].tolist() == [4, 6, 2]
    got = _list(s, entry_capacity=4)        # survivors == capacity fits
    assert got["status"] == 0 and got["count"] == 4
    got = _list(s, work_capacity=5)         # WORK OVERFLOW: W = 6
    assert got["status"] == clr.ERR_CAPACITY and got["count"] == 0 and len(got["entries"]) == 0
    assert got["args"].tolist() == [192, 0, 0, 0] and got["stats"].tolist() == [0, 6, 2]
    assert _list(s, work_capacity=6)["status"] == 0
    empty = dict(s, pos=np.zeros((0, 3), F), rot=np.zeros((0, 4), F), scale=np.zeros(0, F), mesh_id=np.zeros(0, np.uint32), bitmap=np.zeros(0, np.uint32))
    got = _list(empty)
    assert got["status"] == 0 and got["count"] == 0 and got["args"].tolist() == [192, 0, 0, 0] and got["stats"].tolist() == [0, 0, 0]


# ---- the likely mistakes, each caught by a named scene ----

def _mutant_scenes():
    """{name: scene}: the scenes the mutants are run on; tile_words = 4 makes a list tile 256 items."""
    out = {}
    # survivors in three tiles of 4 words, the middle one with fewer than the others: ranks, tile prefixes, the previous tile's rank
    out["three tiles"] = cc.ladder_scene(["1" * 300, ("10" * 150), "1" * 250], [0, 1, 2], base=5)[0]
    # a short last cluster
    out["short last cluster"] = dict(_CASES[[c[0] for c in _CASES].index("short last cluster")][1])
    # a base that wraps
    out["wrapping base"] = cc.ladder_scene(["11"], [0, 0, 0], base=0xFFFFFFFF)[0]
    # members whose first item is at 64 k - 1, 64 k, 64 k + 1 (k = 1, 2, 3)
    out["first items around word edges"] = cc.ladder_scene(["1" * 63, "1" * 1, "1" * 64, "1" * 65, "1" * 62, "1" * 3], [0, 1, 2, 3, 4, 5, 5], base=1)[0]
    # 64 members in one word: one low is harmless while the 64 entries behind it still hold the word's last member — not here
    out["64 members in a word"] = cc.ladder_scene(["1"], [0] * 200, base=3)[0]
    # W = 65: the last word has one item, all of its other lanes are at or above W
    out["W = 65"] = cc.ladder_scene(["1" * 65], [0], base=2)[0]
    return out


_KILLED_BY = {
    "lanes_below inclusive": "three tiles", "tile prefix dropped": "three tiles", "word rank of the previous tile": "three tiles",
    "index_count always 192": "short last cluster", "base not added": "wrapping base", "base not wrapped": "wrapping base",
    "word_member one low": "64 members in a word", "word_member one high": "first items around word edges",
    "inactive lane writes": "W = 65", "entry at capacity written": "three tiles",
}


def test_every_likely_mistake_is_caught_by_its_scene():
    assert set(_KILLED_BY) == set(clr.MUTANTS)
    scenes = _mutant_scenes()
    for mutant, name in _KILLED_BY.items():
        s = scenes[name]
        got = _list(s)
        # room for one entry more than the survivors — or, for the mistake at the capacity, for one less
        room = len(got["all_entries"]) + (-1 if mutant == "entry at capacity written" else 1)
        written = min(room, len(got["all_entries"]))
        want = np.zeros(room + 2, CLUSTER_ENTRY_DTYPE)
        want["index_count"] = 0xFFFFFFFF
        want[:written] = got["all_entries"][:written]
        buf, count = clr.entries_by_steps(got["items"], got["survive"], s["meshes"], s["base"], room, tile_words=4)
        assert count == written and buf.tobytes() == want.tobytes(), (name, "the header's rule")
        bad, bad_count = clr.entries_by_steps(got["items"], got["survive"], s["meshes"], s["base"], room, mutant=mutant, tile_words=4)
        assert bad.tobytes() != want.tobytes() or bad_count != count, (mutant, "is not caught by", name)
    # word_member's definition on the edge scene: members 1, 2, 3 start at 63, 64, 128; member 4 at 193; member 5 at 255, 6 at 258
    s = scenes["first items around word edges"]
    items = _list(s)["items"]
    first = np.nonzero(items["cluster"] == 0)[0]
    assert first.tolist() == [0, 63, 64, 128, 193, 255, 258] and items["W"] == 261
    assert clr.word_members(first, items["W"]).tolist() == [0, 2, 3, 3, 5]   # item 256 lies in member 5 = [255, 258)


# ---- the ABI ----

def _lib():
    from renderer_amd import _lib as L

    return L.load_library()


def test_struct_sizes_in_c_ctypes_and_rust(tmp_path):
    from renderer_amd import _lib as L

    E, O = L.MipClusterEntry, L.MipClusterListOutputs
    assert C.sizeof(E) == 16 and [getattr(E, f).offset for f, _ in E._fields_] == [0, 4, 8, 12] and CLUSTER_ENTRY_DTYPE.itemsize == 16
    assert [CLUSTER_ENTRY_DTYPE.fields[f][1] for f, _ in E._fields_] == [0, 4, 8, 12] and CLUSTER_ENTRY_DTYPE["vertex_offset"] == np.dtype("<i4")
    want = [0, 4, 8, 16, 20, 24, 32, 40]
    assert C.sizeof(O) == 48 and [getattr(O, f).offset for f, _ in O._fields_] == want
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "mi_instance_pipeline.h"
    #define O(f) offsetof(MipClusterListOutputs, f)
    #define E(f) offsetof(MipClusterEntry, f)
    int main(void) {
      printf("%zu %zu %zu %zu %zu\n", sizeof(MipClusterEntry), E(instance), E(first_index), E(vertex_offset), E(index_count));
      printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d\n", sizeof(MipClusterListOutputs), O(struct_size), O(flags), O(cluster_entries), O(entry_capacity),
             O(work_capacity), O(entry_count), O(draw_args), O(stats), (int)MIP_ABI_VERSION);
      return 0; }'''
    c = tmp_path / "t.c"
    c.write_text(src)
    exe = str(tmp_path / "t")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe])
    assert [int(x) for x in subprocess.check_output([exe]).split()] == [16, 0, 4, 8, 12, 48] + want + [4]
    rust = open(os.path.join(ROOT, "integration", "rust", "mip-sys", "src", "lib.rs")).read()
    body = re.search(r"pub struct MipClusterEntry \{(.*?)\}", rust, flags=re.S).group(1)
    assert re.findall(r"pub (\w+): ([^,]+),", body) == [("instance", "u32"), ("first_index", "u32"), ("vertex_offset", "i32"), ("index_count", "u32")]
    body = re.search(r"pub struct MipClusterListOutputs \{(.*?)\}", rust, flags=re.S).group(1)
    assert re.findall(r"pub (\w+): ([^,]+),", body) == [("struct_size", "u32"), ("flags", "u32"), ("cluster_entries", "*mut c_void"), ("entry_capacity", "u32"),
                                                        ("work_capacity", "u32"), ("entry_count", "*mut u32"), ("draw_args", "*mut u32"), ("stats", "*mut u32")]
    for name, size in (("MipClusterEntry", 16), ("MipClusterListOutputs", 48)):
        assert "#[repr(C)]" in rust[: rust.index("pub struct " + name)].rsplit("\n\n", 1)[-1]
        assert f"const _: [u8; {size}] = [0; std::mem::size_of::<{name}>()];" in rust


def test_header_exports_and_declarations_agree():
    from renderer_amd import _lib as L
    import renderer_amd

    name = "mip_list_clusters"
    text = open(os.path.join(ROOT, "include", "mi_instance_pipeline.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    rust = open(os.path.join(ROOT, "integration", "rust", "mip-sys", "src", "lib.rs")).read()
    lib = _lib()
    assert name in L.EXPORTS and hasattr(lib, name)
    c_args = re.search(name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S).group(1).count(",") + 1
    assert c_args == 7 and len(getattr(lib, name).argtypes) == 7
    assert re.search(r"pub fn " + name + r"\((.*?)\)\s*->", rust, flags=re.S).group(1).count(",") + 1 == 7
    assert re.search(r"mip_list_clusters\([^;]*const MipOcclusion\* occ\s*,\s*const MipClusterCone\* cone\s*,\s*const MipClusterListOutputs\* out\)", header)
    assert lib.mip_list_clusters(None, None, None, None, None, None, None) == -1     # without a context: a status code
    section = text[text.index("the visible-cluster list for one indirect draw"): text.index("} MipClusterEntry;")]
    for word in ("ENTRIES:", "ENTRY OVERFLOW", "WORK OVERFLOW", "N = 0", "REFUSED", "ORDERING", "THE CONSUMER", "vkCmdDrawIndirect", "gl_InstanceIndex",
                 "OUT OF SCOPE", "two-phase record", "several views", "per-triangle test", "shards, skinned instances, mip_run_many and recorded graphs"):
        assert word in section, word
    assert renderer_amd.CLUSTER_ENTRY_DTYPE is CLUSTER_ENTRY_DTYPE and callable(renderer_amd.make_cluster_list_outputs)
    assert callable(renderer_amd.InstancePipeline.list_clusters)
    mk = open(os.path.join(ROOT, "renderer_amd", "csrc", "Makefile")).read()
    kernels = re.search(r"^KERNELS := (.*)$", mk, flags=re.M).group(1).split()
    assert "cluster_list_plan.hpp" in kernels and "cluster_list_kernel.hpp" in kernels


def test_list_plan_over_its_decision_edges(tmp_path):
    exe = str(tmp_path / "cluster_list_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "native", "cluster_list_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    last = out.stdout.strip().split("\n")[-1]
    assert last.startswith("CLUSTER LIST PLAN OK") and int(last.split()[4]) > 10000, out.stdout[-2000:]
