"""mip_list_cluster_triangles on the CPU (include/mi_instance_pipeline.h): the hand-written answers
(tests/cluster_triangle_list_cases.py) against the restatement (tests/cluster_triangle_list_restatement.py); the designed
geometry against it; the equivalences with mip_list_clusters' and mip_cull_cluster_triangles' restatements on config 3; both
overflow rules and N = 0; the struct in C, ctypes and the Rust text, the header words, EXPORTS, KERNELS, the C smoke; the plan
(renderer_amd/csrc/cluster_triangle_list_plan.hpp) over its edges under the host sanitizers; and the likely mistakes, each
caught by a named scene."""
import ctypes as C
import functools
import json
import os
import re
import subprocess

import numpy as np
import pytest

import cluster_cases as cc
import cluster_cone_restatement as ccr
import cluster_list_restatement as clr
import cluster_restatement as cr
import cluster_triangle_cases as ctc
import cluster_triangle_list_cases as ctlc
import cluster_triangle_list_restatement as ctlr
import cluster_triangle_restatement as ctr
import lod_restatement as lr
import numpy_restatement as nr
import occlusion_restatement as orr
from renderer_amd import scene
from renderer_amd.pipeline import CLUSTER_ENTRY_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi_instance_pipeline.h")
F = np.float32
CASES = ctc.cases()
ANSWERS = ctlc.answers()
ROOM = 1 << 30
SENTINEL = 0xC0FFEE11


def _listed(s, pv=ctc.PV, entry_capacity=ROOM, work_capacity=0, mutant=None):
    boxes = cr.cluster_boxes(s["meshes"], s["vertices"], s["indices"])
    return ctlr.list_cluster_triangles(s, boxes, s["vertices"], s["indices"], s["bitmap"], lr.DISTANCE, cc.PIN, pv, entry_capacity, work_capacity,
                                       s["base"], mutant=mutant)


def _same(got, want, what):
    assert got["entries"].tobytes() == want["entries"].tobytes(), (what, got["entries"], want["entries"])
    assert got["masks"].tolist() == want["masks"].tolist(), (what, [hex(int(m)) for m in got["masks"]])
    assert got["stats"].tolist() == want["stats"].tolist(), (what, got["stats"])
    assert got["count"] == len(want["entries"]) and got["args"].tolist() == [192, len(want["entries"]), 0, 0], what


def _buffers(r, capacity):
    """What a call leaves in sentinel-filled buffers of capacity + 2 entries and masks: the words behind the count stay."""
    e = np.full((capacity + 2, 4), SENTINEL, np.uint32)
    m = np.full(capacity + 2, SENTINEL, np.uint64)
    e[: r["count"]] = r["entries"].view(np.uint32).reshape(-1, 4)
    m[: r["count"]] = r["masks"]
    return e, m


# ---- the hand-written answers ----

@pytest.mark.parametrize("name,s,tri_want", CASES, ids=[c[0] for c in CASES])
def test_hand_written_answers(name, s, tri_want):
    want = ANSWERS[name]
    got = _listed(s)
    assert got["status"] == 0
    _same(got, want, name)
    # the entries are a subsequence of mip_list_clusters' list, and expanding them gives mip_cull_cluster_triangles' stream
    keeps = got["item_masks"][got["survive"]] != 0
    assert got["entries"].tobytes() == got["listed"][keeps].tobytes()
    assert ctlr.expand(want["entries"], want["masks"], s["indices"]).tolist() == tri_want["stream"].tolist()
    assert want["stats"][1:].tolist() == tri_want["stats"][1:].tolist()      # words 1 to 5 are the command form's


def test_hand_written_answers_are_the_issue_s():
    assert set(ANSWERS) == {c[0] for c in CASES} and len(CASES) == 12      # ten kinds of scene, "a cluster of t" at three t
    for t in (1, 63, 64):
        a = ANSWERS[f"a cluster of {t}"]
        assert a["entries"].tolist() == [(7, 0, 0, 3 * t)] and a["masks"].tolist() == [2 ** t - 1]
    a = ANSWERS["short last cluster"]
    assert a["masks"].tolist() == [2 ** 64 - 1, 0x1F] and a["entries"]["index_count"].tolist() == [192, 15]
    a = ANSWERS["an empty run"]
    assert len(a["entries"]) == 0 and a["stats"].tolist() == [0, 2, 2, 1, 0, 70]
    assert ANSWERS["alternating"]["masks"].tolist() == [0x5555555555555555]
    a = ANSWERS["back-facing cluster inside a run"]
    assert a["entries"]["first_index"].tolist() == [0, 384] and a["stats"].tolist() == [2, 3, 3, 1, 128, 192]
    a = ANSWERS["two instances, the first empty"]
    assert a["entries"]["instance"].tolist() == [6] and a["entries"]["first_index"].tolist() == [192]
    assert ANSWERS["det == 0"]["masks"].tolist() == [0b101] and ANSWERS["det == 0"]["entries"]["index_count"].tolist() == [9]
    assert ANSWERS["a NaN vertex"]["masks"].tolist() == [0b101]
    assert ANSWERS["a non-finite instance"]["masks"].tolist() == [2 ** 64 - 1]


# ---- the designed geometry ----

def _designed():
    """[(name, scene, want, pv)]: small scenes of the designed geometry, every kind beside every other, short last clusters,
    one-triangle clusters, a member whose bit is clear, a base that wraps."""
    out = []
    for mirror in (False, True):
        pv = ctc.PV_MIRROR if mirror else ctc.PV
        tag = " mirrored" if mirror else ""
        out.append(("every kind beside every other" + tag, *ctlc.designed_scene(["FBOAFFOOBBAAFABOF", "A", "B", "O", ""], [0, 1, 2, 3, 4, 0, 1], base=0xFFFFFFFC, mirror=mirror), pv))
        out.append(("short last clusters" + tag, *ctlc.designed_scene(["FA", "AB", "BF", "F", "A"], [0, 1, 2, 3, 4, 2], triangles=[65, 127, 64 + 63, 5, 3], base=3, mirror=mirror), pv))
        out.append(("one-triangle clusters" + tag, *ctlc.designed_scene(["F", "B", "O", "A"], [0, 1, 2, 3] * 40 + [1] * 70 + [0], triangles=[1, 1, 1, 1], base=9,
                                                                        bits=np.arange(231) % 7 != 3, mirror=mirror), pv))
    return out


_DESIGNED = _designed()


@pytest.mark.parametrize("name,s,want,pv", _DESIGNED, ids=[d[0] for d in _DESIGNED])
def test_designed_geometry_is_the_restatement_s_answer(name, s, want, pv):
    got = _listed(s, pv)
    assert got["status"] == 0
    _same(got, want, name)
    assert got["listed"].tobytes() == want["listed"].tobytes()
    assert len(want["entries"]) > 0 and int(want["stats"][1]) > len(want["entries"])     # some surviving cluster keeps no triangle


def test_designed_geometry_by_hand():
    s, want = ctlc.designed_scene(["FBOA"], [0], triangles=[64 * 3 + 3], base=5)
    assert want["entries"].tolist() == [(5, 0, 0, 192), (5, 576, 0, 9)] and want["masks"].tolist() == [2 ** 64 - 1, 0b101]
    assert want["listed"]["first_index"].tolist() == [0, 192, 576] and want["stats"].tolist() == [2, 3, 4, 1, 66, 131]
    s, want = ctlc.designed_scene(["FBOA"], [0], triangles=[64 * 3 + 3], base=5, mirror=True)
    assert want["entries"].tolist() == [(5, 192, 0, 192), (5, 576, 0, 9)] and want["masks"].tolist() == [2 ** 64 - 1, 0b010]


# ---- the equivalences on config 3 ----

def metric_thresholds(s, mode, levels=6):
    """Five thresholds at the quantiles of the metric over the scene's instances: every level gets a sixth of them."""
    d = np.asarray(s["cam_pos"], np.float64)[None, :] - s["pos"].astype(np.float64)
    q = (d * d).sum(axis=1)
    if mode == lr.RELATIVE:
        e = (s["meshes"]["aabb_max"].astype(np.float64) - s["meshes"]["aabb_min"].astype(np.float64))[s["mesh_id"]]
        q = q / (s["scale"].astype(np.float64) ** 2 * (e * e).sum(axis=1))
    q = np.sort(q)
    return tuple(float(np.float32(v)) for v in np.maximum.accumulate([q[len(q) * k // levels] for k in range(1, levels)]))


@functools.lru_cache(maxsize=None)
def _built(n, ordering):
    s = scene.make_scene(3, n=n)
    vertices, indices = scene.make_geometry(s["meshes"], ordering)
    boxes = cr.cluster_boxes(s["meshes"], vertices, indices)
    bitmap = orr.bitmap_of(~nr.run(s)["coarse_culled"])
    cones = ccr.cluster_cones(s["meshes"], vertices, indices, boxes) if ordering == "patches" else None
    return s, vertices, indices, boxes, bitmap, cones


def _wall():
    depth = np.ones((32, 64), F)
    depth[:, :32] = 0.0
    return dict(pv=scene.default_pv(), levels=orr.pyramid_levels(depth), width=64, height=32)


@pytest.mark.parametrize("cone", [False, True], ids=["no cone", "cone under patches"])
@pytest.mark.parametrize("wall", [False, True], ids=["frustum", "wall"])
@pytest.mark.parametrize("mode", [lr.DISTANCE, lr.RELATIVE], ids=["distance", "relative"])
@pytest.mark.parametrize("n", [257, 1025])
def test_equivalences_on_config_3(n, mode, wall, cone):
    s, vertices, indices, boxes, bitmap, cones = _built(n, "patches" if cone else "strips")
    pv = scene.default_pv()
    sw = metric_thresholds(s, mode)
    occlusion = _wall() if wall else None
    k = None
    if cone:
        _, eye, facing = ccr.cone_from_pv(pv)
        k = dict(cones=cones, eye=eye, facing=facing)
    got = ctlr.list_cluster_triangles(s, boxes, vertices, indices, bitmap, mode, sw, pv, ROOM, first_instance_base=0xFFFFFF80, occlusion=occlusion, cone=k)
    assert got["status"] == 0 and got["count"] == len(got["all_entries"]) > 0
    # the entries are the subsequence of mip_list_clusters' entries where the mask is not zero
    lst = clr.list_clusters(s, boxes, bitmap, mode, sw, ROOM, first_instance_base=0xFFFFFF80, occlusion=occlusion, cone=k)
    per_survivor = got["item_masks"][got["survive"]]
    assert len(per_survivor) == len(lst["entries"])
    assert got["entries"].tobytes() == lst["entries"][per_survivor != 0].tobytes() and got["masks"].tolist() == per_survivor[per_survivor != 0].tolist()
    assert (got["masks"] != 0).all() and 0 < len(got["entries"]) < len(lst["entries"])
    # no bit at or above the triangle count
    counts = got["entries"]["index_count"].astype(np.int64) // 3
    assert ((got["masks"] >> np.minimum(counts, 63).astype(np.uint64) >> (counts == 64).astype(np.uint64)) == 0).all()
    # bit by bit, (entry, mask) expands into the command form's stream; words 1 to 5 of the stats are its words
    if cone:
        tri = ccr.cull_cluster_triangles_cone(s, boxes, cones, k["eye"], k["facing"], vertices, indices, bitmap, mode, sw, pv, ROOM, ROOM,
                                              first_instance_base=0xFFFFFF80, occlusion=occlusion)
    else:
        tri = ctr.cull_cluster_triangles(s, boxes, vertices, indices, bitmap, mode, sw, pv, ROOM, ROOM, first_instance_base=0xFFFFFF80, occlusion=occlusion)
    assert ctlr.expand(got["entries"], got["masks"], indices).tobytes() == tri["full_stream"].tobytes()
    assert got["stats"][1:].tolist() == tri["stats"][1:].tolist() and int(got["stats"][0]) == len(got["entries"])
    assert int(ctlr.popcount64(got["masks"]).sum()) == int(tri["stats"][4])


def test_the_known_answer_of_the_built_scene():
    """config 3, n = 257, "strips", the frame's bitmap, the pin policy: 162 813 triangles tested, 78 898 kept, and the 83
    surviving clusters that keep no triangle (tests/test_cluster_triangle_restatement.py) have no entry."""
    s, vertices, indices, boxes, bitmap, _ = _built(257, "strips")
    got = ctlr.list_cluster_triangles(s, boxes, vertices, indices, bitmap, lr.DISTANCE, lr.PIN_SWITCH_SQ, scene.default_pv(), ROOM)
    assert got["stats"].tolist() == [2581 - 83, 2581, 3127, 72, 78898, 162813]


# ---- both overflow rules, N = 0, the sentinel behind every count ----

def test_overflow_rules_and_the_empty_scene():
    s, want = ctlc.designed_scene(["FBOAF", "A"], [0, 1, 0], triangles=[64 * 4 + 7, 64], base=2)
    full = _listed(s)
    _same(full, want, "with room")
    entries, w, members = len(want["entries"]), int(want["stats"][2]), int(want["stats"][3])
    assert entries == 7 and w == 11
    e_full, m_full = _buffers(full, entries)
    for cap in (entries - 1, 3, 0):               # ENTRY OVERFLOW: the first `cap` entries and masks exactly, the true six stats
        got = _listed(s, entry_capacity=cap)
        assert got["status"] == ctlr.ERR_CAPACITY and got["count"] == cap and got["args"].tolist() == [192, cap, 0, 0]
        assert got["stats"].tolist() == want["stats"].tolist()
        e, m = _buffers(got, cap)
        assert e[:cap].tobytes() == e_full[:cap].tobytes() and m[:cap].tolist() == m_full[:cap].tolist()
        assert (e[cap:] == SENTINEL).all() and (m[cap:] == SENTINEL).all()       # nothing at or behind entry_count
    got = _listed(s, entry_capacity=entries)      # entries == capacity fits
    assert got["status"] == 0 and got["count"] == entries
    got = _listed(s, work_capacity=w - 1)         # WORK OVERFLOW
    assert got["status"] == ctlr.ERR_CAPACITY and got["count"] == 0 and len(got["entries"]) == 0 and len(got["masks"]) == 0
    assert got["args"].tolist() == [192, 0, 0, 0] and got["stats"].tolist() == [0, 0, w, members, 0, 0]
    assert _listed(s, work_capacity=w)["status"] == 0
    empty = dict(s, pos=np.zeros((0, 3), F), rot=np.zeros((0, 4), F), scale=np.zeros(0, F), mesh_id=np.zeros(0, np.uint32), bitmap=np.zeros(0, np.uint32))
    got = _listed(empty)
    assert got["status"] == 0 and got["count"] == 0 and got["args"].tolist() == [192, 0, 0, 0] and got["stats"].tolist() == [0] * 6
    e, m = _buffers(got, 0)
    assert (e == SENTINEL).all() and (m == SENTINEL).all()


# ---- the likely mistakes, each caught by a named scene ----

_KILLED_BY = {
    "bits above the triangle count": "a cluster of 63",
    "entry kept with mask 0": "an empty run",
    "masks by work item": "back-facing cluster inside a run",
    "mask of the next cluster": "short last cluster",
    "pv ignored": "every kind beside every other mirrored",
    "tested over all items": "a culled cluster splits the run",
}


def test_every_likely_mistake_is_caught_by_its_scene():
    assert set(_KILLED_BY) == set(ctlr.MUTANTS)
    scenes = {name: (s, ANSWERS[name], ctc.PV) for name, s, _ in CASES}
    scenes.update({name: (s, want, pv) for name, s, want, pv in _DESIGNED})
    for mutant, name in _KILLED_BY.items():
        s, want, pv = scenes[name]
        _same(_listed(s, pv), want, name)
        bad = _listed(s, pv, mutant=mutant)
        differs = (bad["entries"].tobytes() != want["entries"].tobytes() or bad["masks"].tolist() != want["masks"].tolist() or
                   bad["stats"].tolist() != want["stats"].tolist())
        assert differs, (mutant, "is not caught by", name)


# ---- the ABI surface ----

def _load():
    from renderer_amd import _lib as L

    return L, L.load_library()


def test_struct_in_c_ctypes_and_rust(tmp_path):
    L, _ = _load()
    o = L.MipClusterTriangleListOutputs
    fields = ["struct_size", "flags", "cluster_entries", "triangle_masks", "entry_capacity", "work_capacity", "entry_count", "draw_args", "stats"]
    assert C.sizeof(o) == 56 and [f for f, _t in o._fields_] == fields
    assert [getattr(o, f).offset for f in fields] == [0, 4, 8, 16, 24, 28, 32, 40, 48]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "mi_instance_pipeline.h"\nint main(void) {\n  printf("%zu", sizeof(MipClusterTriangleListOutputs));\n'
    src += "".join(f'  printf(" %zu", offsetof(MipClusterTriangleListOutputs, {f}));\n' for f in fields)
    src += '  printf(" %d\\n", (int)MIP_ABI_VERSION);\n  return 0;\n}\n'
    c = tmp_path / "t.c"
    c.write_text(src)
    exe = str(tmp_path / "t")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe])
    assert [int(x) for x in subprocess.check_output([exe]).split()] == [56, 0, 4, 8, 16, 24, 28, 32, 40, 48, 4]     # MIP_ABI_VERSION stays
    rust = open(os.path.join(ROOT, "integration", "rust", "mip-sys", "src", "lib.rs")).read()
    body = re.search(r"pub struct MipClusterTriangleListOutputs \{(.*?)\}", rust, flags=re.S).group(1)
    assert re.findall(r"pub (\w+): ([^,]+),", body) == [("struct_size", "u32"), ("flags", "u32"), ("cluster_entries", "*mut c_void"), ("triangle_masks", "*mut c_void"),
                                                        ("entry_capacity", "u32"), ("work_capacity", "u32"), ("entry_count", "*mut u32"),
                                                        ("draw_args", "*mut u32"), ("stats", "*mut u32")]
    assert "#[repr(C)]" in rust[: rust.index("pub struct MipClusterTriangleListOutputs")].rsplit("\n\n", 1)[-1]
    assert "const _: [u8; 56] = [0; std::mem::size_of::<MipClusterTriangleListOutputs>()];" in rust


def test_header_exports_and_declarations_agree():
    import renderer_amd

    L, lib = _load()
    name = "mip_list_cluster_triangles"
    text = open(HEADER).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    rust = open(os.path.join(ROOT, "integration", "rust", "mip-sys", "src", "lib.rs")).read()
    assert "#define MIP_ABI_VERSION 4u" in text
    assert name in L.EXPORTS and hasattr(lib, name)
    assert re.search(name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S).group(1).count(",") + 1 == 7 and len(getattr(lib, name).argtypes) == 7
    assert re.search(r"pub fn " + name + r"\((.*?)\)\s*->", rust, flags=re.S).group(1).count(",") + 1 == 7
    assert re.search(name + r"\([^;]*const MipOcclusion\* occ\s*,\s*const MipClusterCone\* cone\s*,\s*const MipClusterTriangleListOutputs\* out\)", header)
    assert lib.mip_list_cluster_triangles(None, None, None, None, None, None, None) == -1      # without a context: a status code
    section = text[text.index("Extension: per-triangle masks on the visible-cluster list"): text.index("} MipClusterTriangleListOutputs;")]
    for word in ("NOT a reference", "TRI_SURVIVES", "MASKS:", "ENTRIES:", "subsequence", "triangle_masks[k]", "ENTRY OVERFLOW", "WORK OVERFLOW", "no index overflow",
                 "N = 0", "REFUSED", "overlapping", "ORDERING", "THE CONSUMER", "popcount(mask)", "gl_VertexIndex / 3", "OUT OF SCOPE", "per-entry triangle prefix",
                 "two-phase record", "several views", "mip_run_many and recorded graphs"):
        assert word in section, word
    # the out-of-scope lines of the two calls this one joins point here
    tri = text[text.index("Extension: per-triangle culling of surviving clusters"): text.index("} MipClusterTriangleOutputs;")]
    assert "dropping empty\n * commands" not in tri and "mip_list_cluster_triangles" in tri
    lst = text[text.index("the visible-cluster list for one indirect draw"): text.index("} MipClusterEntry;")]
    assert "mip_list_cluster_triangles" in lst
    assert "the per-triangle stream" not in text
    assert callable(renderer_amd.make_cluster_triangle_list_outputs) and callable(renderer_amd.InstancePipeline.list_cluster_triangles)
    mk = open(os.path.join(ROOT, "renderer_amd", "csrc", "Makefile")).read()
    kernels = re.search(r"^KERNELS := (.*)$", mk, flags=re.M).group(1).split()
    assert "cluster_triangle_list_plan.hpp" in kernels and "cluster_triangle_list_kernel.hpp" in kernels
    smoke = open(os.path.join(ROOT, "integration", "c", "mip_smoke.c")).read()
    assert "MipClusterTriangleListOutputs" in smoke and "mip_list_cluster_triangles(ctx" in smoke


def test_c_smoke_compiles_against_the_header(tmp_path):
    obj = str(tmp_path / "mip_smoke.o")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(ROOT, "integration", "c", "mip_smoke.c"),
                           "-o", obj])


# ---- the plan ----

def test_plan_over_its_decision_edges(tmp_path):
    exe = str(tmp_path / "cluster_triangle_list_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "native", "cluster_triangle_list_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    last = out.stdout.strip().split("\n")[-1]
    assert last.startswith("CLUSTER TRIANGLE LIST PLAN OK") and int(last.split()[5]) > 1000, out.stdout[-2000:]
    sizes = json.loads(subprocess.check_output([exe, "sizes"]))
    assert sizes["test_grid_cap"] == sizes["write_grid_cap"] == sizes["max_blocks"] * sizes["item_tile"]
    assert sizes["count_grid_cap"] == sizes["max_blocks"] * sizes["list_tile"]
