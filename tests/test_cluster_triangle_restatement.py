"""mip_cull_cluster_triangles without a GPU: tests/cluster_triangle_restatement.py (written from the header's text) against the
hand-written scenes of tests/cluster_triangle_cases.py, the known answer of the scene the GPU tests build on, the existing
per-triangle stage's restatement, its own properties, the three overflow rules; the ABI surface (C, ctypes, the Rust text,
EXPORTS); the native check of renderer_amd/csrc/cluster_triangle_plan.hpp, built with the address and undefined-behaviour
sanitizers."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import cluster_cases as cc
import cluster_restatement as cr
import cluster_triangle_cases as ctc
import cluster_triangle_restatement as ctr
import lod_restatement as lr
import numpy_restatement as nr
import occlusion_restatement as orr
from renderer_amd import _lib, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi_instance_pipeline.h")
CASES = ctc.cases()
ROOM = 1 << 31


@functools.lru_cache(maxsize=None)
def _built(ordering, n=257):
    """config 3, the frame's bitmap, the pin policy, default_pv(): (scene, vertices, indices, boxes, bitmap, the answer)."""
    s = scene.make_scene(3, n=n)
    vertices, indices = scene.make_geometry(s["meshes"], ordering)
    boxes = cr.cluster_boxes(s["meshes"], vertices, indices)
    bitmap = orr.bitmap_of(~nr.run(s)["coarse_culled"])
    r = ctr.cull_cluster_triangles(s, boxes, vertices, indices, bitmap, lr.DISTANCE, lr.PIN_SWITCH_SQ, scene.default_pv(), ROOM, ROOM, first_instance_base=11)
    return s, vertices, indices, boxes, bitmap, r


def _again(ordering, **kw):
    s, vertices, indices, boxes, bitmap, _ = _built(ordering)
    args = dict(cmd_capacity=ROOM, index_capacity=ROOM, first_instance_base=11)
    args.update(kw)
    return ctr.cull_cluster_triangles(s, boxes, vertices, indices, bitmap, lr.DISTANCE, lr.PIN_SWITCH_SQ, scene.default_pv(), **args)


# ---- the hand-written scenes ----

@pytest.mark.parametrize("name,s,want", CASES, ids=[c[0] for c in CASES])
def test_hand_cases_against_the_restatement(name, s, want):
    boxes = cr.cluster_boxes(s["meshes"], s["vertices"], s["indices"])
    got = ctr.cull_cluster_triangles(s, boxes, s["vertices"], s["indices"], s["bitmap"], lr.DISTANCE, cc.PIN, ctc.PV, ROOM, ROOM, first_instance_base=s["base"])
    assert got["status"] == 0
    assert got["cmds"].tobytes() == want["cmds"].tobytes(), (name, got["cmds"], want["cmds"])
    assert got["stats"].tolist() == want["stats"].tolist(), (name, got["stats"])
    assert got["stream"].tolist() == want["stream"].tolist(), name
    assert got["count"] == len(want["cmds"])


def test_hand_cases_cover_what_they_claim():
    by_name = {c[0]: c for c in CASES}
    assert by_name["an empty run"][2]["cmds"]["indexCount"].tolist() == [0] and len(by_name["an empty run"][2]["stream"]) == 0
    assert by_name["two instances, the first empty"][2]["cmds"]["firstIndex"].tolist() == [0, 0]
    assert len(by_name["back-facing cluster inside a run"][2]["cmds"]) == 1 and len(by_name["a culled cluster splits the run"][2]["cmds"]) == 2
    # det == 0: the three determinants are exactly 0, +TINY and -TINY, and TINY is the float beside 0
    s = by_name["det == 0"][1]
    v = s["vertices"][s["indices"].reshape(-1, 3).astype(np.int64)]
    x, y = v[:, :, 0], v[:, :, 1]
    det = x[:, 0] * (y[:, 1] - y[:, 2]) - x[:, 1] * (y[:, 0] - y[:, 2]) + x[:, 2] * (y[:, 0] - y[:, 1])
    assert det.tolist() == [0.0, ctc.TINY, -ctc.TINY] and ctc.TINY == float(np.nextafter(np.float32(0), np.float32(1))) > 0
    model = nr.model_matrices(s["pos"], s["rot"], s["scale"])[0]
    assert nr.triangle_culled(model, ctc.PV, v).tolist() == [False, True, False]
    # the non-finite instance: every entry of the matrix but the translation is NaN, row 3 included
    s = by_name["a non-finite instance"][1]
    model = nr.model_matrices(s["pos"], s["rot"], s["scale"])[0].reshape(4, 4)   # [column][row]
    assert np.isnan(model[:3, :]).all() and model[3].tolist() == [0, 0, 0, 1]
    # the mirrored pv of the structural scenes turns the decision round
    tri = np.array([[(0, 0, 0), (1, 0, 0), (0, 1, 0)]], np.float32)
    eye = np.eye(4, dtype=np.float32).reshape(16)
    assert nr.triangle_culled(eye, ctc.PV, tri).tolist() == [True] and nr.triangle_culled(eye, ctc.PV_MIRROR, tri).tolist() == [False]


def test_ladder_want_is_the_restatements_answer():
    """cluster_triangle_cases.ladder_want, which the structural GPU tests expect, against the restatement on a small ladder."""
    s, want = cc.ladder_scene(["1101", "0110111", "1"], [0, 1, 2, 1, 0], base=4)
    boxes = cr.cluster_boxes(s["meshes"], s["vertices"], s["indices"])
    got = ctr.cull_cluster_triangles(s, boxes, s["vertices"], s["indices"], s["bitmap"], lr.DISTANCE, cc.PIN, ctc.PV_MIRROR, ROOM, ROOM, first_instance_base=4)
    w = ctc.ladder_want(s, want)
    assert got["cmds"].tobytes() == w["cmds"].tobytes() and got["stats"].tolist() == w["stats"].tolist() and got["stream"].tolist() == w["stream"].tolist()
    assert len(w["cmds"]) == 9 and int(w["stats"][4]) == 64 * 17


# ---- the known answer ----

def test_known_answer_of_the_built_scene():
    """config 3, n = 257, "strips", the frame's bitmap, the pin policy, default_pv(): the figures of the issue this feature
    answers, from a script independent of this restatement."""
    r = _built("strips")[5]
    heads, clusters, w, members, kept, tested = (int(v) for v in r["stats"])
    assert (members, w, clusters, heads) == (72, 3127, 2581, 71)
    assert (tested, kept) == (162813, 78898)
    assert int(((r["kept"] == 0) & r["survive"]).sum()) == 83 and int((r["kept"] == 64).sum()) == 6
    assert int((r["cmds"]["indexCount"] == 0).sum()) == 5
    r = _built("rows")[5]
    assert [int(v) for v in r["stats"]] == [72, 2582, 3127, 72, 78924, 162877] and int((r["cmds"]["indexCount"] == 0).sum()) == 6


# ---- agreement with the per-triangle stage's restatement ----

@pytest.mark.parametrize("ordering", ["strips", "rows", "shuffled"])
def test_stream_equals_the_existing_stage_filtered_to_surviving_clusters(ordering):
    """numpy_restatement.cull_all_triangles over the frame's commands: its survivors of each instance, filtered to the triangles
    of that instance's surviving clusters, in order, are the index stream. (Every index_offset of the scene is a multiple of 3:
    the uvec3 rounding of the old stage decides nothing.)"""
    s, vertices, indices, boxes, bitmap, r = _built(ordering)
    assert (s["meshes"]["index_offset"] % 3 == 0).all()
    frame = nr.run(s)
    cmds = np.zeros(len(frame["cmds"]["indexCount"]), [(k, np.uint32) for k in ("indexCount", "firstIndex", "firstInstance")] + [("vertexOffset", np.int64)])
    for k in ("indexCount", "firstIndex", "vertexOffset", "firstInstance"):
        cmds[k] = frame["cmds"][k]
    src = nr.src_index_offsets(s["pos"], s["mesh_id"], frame["coarse_culled"], s["meshes"], s["cam_pos"])
    final, out = nr.cull_all_triangles(cmds, src, frame["model"], 0, scene.default_pv(), vertices, indices, int(frame["cmds"]["total"]))
    old = {int(i): out[int(f) : int(f) + int(c)] for i, f, c in zip(final["firstInstance"], final["firstIndex"], final["indexCount"])}
    items, sv = r["items"], r["survive"]
    t = items["table"]
    expected = []
    for k in range(len(cmds)):
        i = int(cmds["firstInstance"][k])
        b = int(items["bucket"][i])
        n_tris = int(t["T"][b])
        # the pin policy picks the frame's level for every instance: the two stages cut the same triangles
        assert int(s["meshes"]["index_offset"][t["mesh"][b], t["lod"][b]]) == int(src[k]) and 3 * n_tris == int(cmds["indexCount"][k])
        ix = np.asarray(indices, np.uint32)[int(src[k]) : int(src[k]) + 3 * n_tris].reshape(n_tris, 3)
        v = np.asarray(vertices, np.float32).reshape(-1, 3)[ix.astype(np.int64) + int(cmds["vertexOffset"][k])]
        keep = ~nr.triangle_culled(frame["model"][i], scene.default_pv(), v)
        # which triangles the old stage kept: the mask that reproduces its output for this instance
        assert ix[keep].reshape(-1).tolist() == old.get(i, np.zeros(0, np.uint32)).tolist()
        alive = np.zeros(int(t["C"][b]), bool)
        alive[items["cluster"][sv & (items["inst"] == i)]] = True
        expected.append(ix[keep & alive[np.arange(n_tris) // 64]].reshape(-1))
    assert np.concatenate(expected).tolist() == r["stream"].tolist() and len(r["stream"]) == 3 * int(r["stats"][4]) > 0


# ---- properties ----

@pytest.mark.parametrize("ordering", ["strips", "rows", "shuffled"])
def test_properties_of_the_restatement(ordering):
    s, vertices, indices, boxes, bitmap, r = _built(ordering)
    cmds, items, sv, kept = r["cmds"], r["items"], r["survive"], r["kept"]
    count, first = cmds["indexCount"].astype(np.int64), cmds["firstIndex"].astype(np.int64)
    # the commands tile the stream without gap or overlap, in order
    assert first[0] == 0 and (first[1:] == first[:-1] + count[:-1]).all() and first[-1] + count[-1] == len(r["stream"])
    assert int(count.sum()) == 3 * int(r["stats"][4]) == 3 * int(kept.sum()) and (count % 3 == 0).all()
    # one command per head, at the entry mip_cull_clusters uses, with its instance and vertex offset
    plain = cr.cull_clusters(s, boxes, bitmap, lr.DISTANCE, lr.PIN_SWITCH_SQ, cmd_capacity=ROOM, first_instance_base=11)
    assert len(plain["cmds"]) == len(cmds) and r["stats"][:4].tolist() == plain["stats"].tolist()
    for k in ("instanceCount", "vertexOffset", "firstInstance"):
        assert (cmds[k] == plain["cmds"][k]).all()
    assert (count <= plain["cmds"]["indexCount"]).all()
    # every index triple is a source triple of its cluster, in the cluster's order
    t = items["table"]
    at = 0
    triples = r["stream"].reshape(-1, 3)
    for w in np.nonzero(sv)[0]:
        b = int(items["bucket"][items["inst"][w]])
        off = int(s["meshes"]["index_offset"][t["mesh"][b], t["lod"][b]]) + 192 * int(items["cluster"][w])
        n = int(ctr.item_triangles(items)[w])
        source = np.asarray(indices, np.uint32)[off : off + 3 * n].reshape(n, 3)
        mine = triples[at : at + int(kept[w])]
        j = 0
        for row in mine:                                        # a subsequence of the cluster's triangles
            while j < n and not (source[j] == row).all():
                j += 1
            assert j < n, (w, row)
            j += 1
        at += int(kept[w])
    assert at == len(triples)
    assert (kept[~sv] == 0).all() and int(r["stats"][5]) == int(ctr.item_triangles(items)[sv].sum())


def test_the_pyramid_removes_triangles_with_their_clusters():
    s, vertices, indices, boxes, bitmap, free = _built("strips")
    depth = np.ones((32, 64), np.float32)
    depth[:, :32] = 0.0
    occ = dict(pv=scene.default_pv(), levels=orr.pyramid_levels(depth), width=64, height=32)
    walled = _again("strips", occlusion=occ)
    assert 0 < int(walled["stats"][1]) < int(free["stats"][1]) and 0 < int(walled["stats"][5]) < int(free["stats"][5])
    assert int(walled["stats"][4]) <= int(free["stats"][4])


# ---- the overflow rules ----

def test_overflow_rules():
    full = _built("strips")[5]
    heads, w, members, total = int(full["stats"][0]), int(full["stats"][2]), int(full["stats"][3]), 3 * int(full["stats"][4])
    # index overflow: nothing but the zero count and the true six stats
    for cap in (total - 3, total - 1, 0):
        cut = _again("strips", index_capacity=cap)
        assert cut["status"] == ctr.ERR_CAPACITY and cut["count"] == 0 and len(cut["cmds"]) == 0 and len(cut["stream"]) == 0
        assert cut["stats"].tolist() == full["stats"].tolist()
    fits = _again("strips", index_capacity=total, cmd_capacity=heads, work_capacity=w)
    assert fits["status"] == 0 and fits["cmds"].tobytes() == full["cmds"].tobytes() and fits["stream"].tolist() == full["stream"].tolist()
    # command overflow: the first commands exactly, the stream complete
    for cap in (heads - 1, 0):
        cut = _again("strips", cmd_capacity=cap)
        assert cut["status"] == ctr.ERR_CAPACITY and cut["count"] == cap and cut["cmds"].tobytes() == full["cmds"][:cap].tobytes()
        assert cut["stream"].tolist() == full["stream"].tolist() and cut["stats"].tolist() == full["stats"].tolist()
    # work overflow: mip_cull_clusters' rule, six words
    work = _again("strips", work_capacity=w - 1)
    assert work["status"] == ctr.ERR_CAPACITY and work["count"] == 0 and len(work["stream"]) == 0 and work["stats"].tolist() == [0, 0, w, members, 0, 0]
    # an index overflow wins over a command overflow: nothing is written
    both = _again("strips", index_capacity=total - 3, cmd_capacity=1)
    assert both["status"] == ctr.ERR_CAPACITY and both["count"] == 0 and len(both["stream"]) == 0
    s, vertices, indices, boxes, bitmap, _ = _built("strips")
    empty = ctr.cull_cluster_triangles(dict(s, pos=s["pos"][:0], rot=s["rot"][:0], scale=s["scale"][:0], mesh_id=s["mesh_id"][:0]), boxes, vertices, indices,
                                       bitmap[:0], lr.DISTANCE, lr.PIN_SWITCH_SQ, scene.default_pv(), 4, 4)
    assert empty["status"] == 0 and empty["count"] == 0 and empty["stats"].tolist() == [0] * 6


# ---- the ABI surface ----

def test_struct_in_c_ctypes_and_rust(tmp_path):
    o = _lib.MipClusterTriangleOutputs
    assert C.sizeof(o) == 56 and [f for f, _ in o._fields_][:7] == [f for f, _ in _lib.MipClusterOutputs._fields_]
    fields = [f for f, _ in o._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "mi_instance_pipeline.h"\nint main(void) {\n  printf("%zu", sizeof(MipClusterTriangleOutputs));\n'
    src += "".join(f'  printf(" %zu", offsetof(MipClusterTriangleOutputs, {f}));\n' for f in fields[1:])
    src += '  printf(" %zu\\n", offsetof(MipClusterOutputs, stats));\n  return 0;\n}\n'
    c = tmp_path / "t.c"
    c.write_text(src)
    exe = str(tmp_path / "t")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe])
    sizes = [int(x) for x in subprocess.check_output([exe]).split()]
    assert sizes == [C.sizeof(o)] + [getattr(o, f).offset for f in fields[1:]] + [o.stats.offset]      # the leading fields lie as MipClusterOutputs'
    rust = open(os.path.join(ROOT, "integration", "rust", "mip-sys", "src", "lib.rs")).read()
    body = re.search(r"pub struct MipClusterTriangleOutputs \{(.*?)\}", rust, flags=re.S).group(1)
    assert re.findall(r"pub (\w+):", body) == fields
    assert "const _: [u8; 56] = [0; std::mem::size_of::<MipClusterTriangleOutputs>()];" in rust
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    c_args = re.search(r"mip_cull_cluster_triangles\s*\(([^;]*?)\)\s*;", header, flags=re.S).group(1).count(",") + 1
    r_args = re.search(r"pub fn mip_cull_cluster_triangles\((.*?)\)\s*->", rust, flags=re.S).group(1).count(",") + 1
    assert c_args == r_args == 6


def test_header_and_exports():
    text = open(HEADER).read()
    assert "#define MIP_ABI_VERSION 4u" in text
    assert "mip_cull_cluster_triangles" in _lib.EXPORTS
    assert re.search(r"\bmip_cull_cluster_triangles\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    section = text[text.index("Extension: per-triangle culling of surviving clusters"):text.index("MipClusterTriangleOutputs;")]
    assert "NOT a reference" in section and "indexCount = 0" in section and "first_index_base is not" in section
    import renderer_amd
    lib = renderer_amd.load_library()
    assert lib.mip_cull_cluster_triangles(None, None, None, None, None, None) == -1


# ---- the plan ----

def test_cluster_triangle_plan_over_its_decision_edges(tmp_path):
    exe = str(tmp_path / "cluster_triangle_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "native", "cluster_triangle_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    last = out.stdout.strip().split("\n")[-1]
    assert last.startswith("CLUSTER TRIANGLE PLAN OK") and int(last.split()[4]) > 100_000, out.stdout[-2000:]
    sizes = subprocess.check_output([exe, "sizes"])
    import json
    sizes = json.loads(sizes)
    assert sizes["test_grid_cap"] == sizes["write_grid_cap"] == sizes["max_blocks"] * sizes["item_tile"]
    assert sizes["command_grid_cap"] == sizes["max_blocks"] * sizes["head_tile"]
