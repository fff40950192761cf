"""The batched-draws extension without a GPU: tests/batch_restatement.py against the oracle's compacted draw list (the
batches expand to exactly that list), a hand-written known answer, the bitmap's edge cases, and the ABI surface
(include/mi_instance_pipeline.h: MipBatchOutputs, mip_batch_draws)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import batch_restatement as br
import fuzz_scenes
from renderer_amd.pipeline import DRAW_CMD_DTYPE, MESH_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi_instance_pipeline.h")


def _src_index_offsets(oracle, s, culled):
    """orc_src_index_offsets: index_offset[lod] of every emitted command of the oracle's list, in list order."""
    from oracle.oracle import ORC_MESH_DTYPE

    n = s["n"]
    pos = np.ascontiguousarray(s["pos"], np.float32).reshape(-1, 3)
    mesh_id = np.ascontiguousarray(s["mesh_id"], np.uint32)
    meshes = np.ascontiguousarray(s["meshes"], ORC_MESH_DTYPE)
    culled = np.ascontiguousarray(culled, np.uint8)
    cam = np.ascontiguousarray(s["cam_pos"], np.float32).reshape(3)
    src = np.zeros(max(n, 1), np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    oracle.lib().orc_src_index_offsets(C.c_uint32(n), p(pos), p(mesh_id), p(culled), p(meshes), p(cam), p(src))
    return src


def _check_expands_to_the_oracle_list(oracle, s, what):
    base = int(s.get("first_instance_base", 0))
    want = oracle.run(s["pos"], s["rot"], s["scale"], s["mesh_id"], s["meshes"], s["planes"], s["cam_pos"],
                      first_instance_base=base, first_index_base=int(s.get("first_index_base", 0)))
    b = br.batch_draws(s["pos"], s["mesh_id"], s["meshes"], s["cam_pos"], want["visible_bitmap"], first_instance_base=base, model=want["model"])
    lst = want["draw_cmds"]
    assert b["members"] == want["draw_count"] == int(b["cmds"]["instanceCount"].sum()), what
    got = br.expand(b, base)
    for field in ("indexCount", "instanceCount", "vertexOffset", "firstInstance"):
        assert np.array_equal(got[field], lst[field]), (what, field)
    src = _src_index_offsets(oracle, s, want["coarse_culled"])[: want["draw_count"]]
    assert np.array_equal(got["firstIndex"], src), (what, "firstIndex against orc_src_index_offsets")
    counts = b["cmds"]["instanceCount"].astype(np.int64)
    assert np.array_equal(b["cmds"]["firstInstance"], np.cumsum(counts) - counts), what
    assert (counts > 0).all() and b["count"] <= min(2 * len(s["meshes"]), max(s["n"], 0)), what
    # the matrices in slot order are the oracle's, gathered through the ids
    inst = (b["ids"].astype(np.int64) - base) & 0xFFFFFFFF
    assert b["model"].tobytes() == want["model"][inst].tobytes(), what
    return b


@pytest.mark.parametrize("config,n", [(1, 1024), (2, 20_000), (3, 50_000)])
def test_batches_expand_to_the_compacted_list_baseline_configs(oracle_mod, config, n):
    from renderer_amd import scene

    s = scene.make_scene(config, n=n)
    b = _check_expands_to_the_oracle_list(oracle_mod, s, f"config {config}")
    assert 0 < b["count"] <= 2 * len(s["meshes"])


def test_batches_expand_to_the_compacted_list_fuzzed_scenes(oracle_mod):
    rng = np.random.default_rng(20261016)
    seen_empty_lod = seen_one_lod = False
    for k in range(40):
        s = fuzz_scenes.random_scene(rng, oracle_mod, n_max=3000)
        seen_empty_lod |= bool((s["meshes"]["index_len"][:, :2] == 0).any())
        seen_one_lod |= bool((s["meshes"]["n_lods"] == 1).any())
        _check_expands_to_the_oracle_list(oracle_mod, s, f"fuzz {k}")
    assert seen_empty_lod and seen_one_lod


def _known_scene():
    meshes = np.zeros(3, MESH_DTYPE)
    meshes["aabb_min"], meshes["aabb_max"] = -1.0, 1.0
    meshes["n_lods"] = [2, 1, 2]                 # mesh 1 has a single LOD, mesh 2's LOD 1 is empty
    meshes["index_len"][:, :2] = [[36, 12], [60, 999], [24, 0]]
    meshes["index_offset"][:, :2] = [[0, 36], [48, 7777], [108, 132]]
    meshes["vertex_offset"] = [0, 100, -5]
    cam = np.array([0.0, 0.0, 0.0], np.float32)
    #            instance:  0     1     2     3     4     5     6     7     8
    z = np.array([5.0, 15.0, 5.0, 15.0, 5.0, 15.0, 9.0, 10.0, 11.0], np.float32)   # 10.0 itself is NOT beyond the LOD distance
    pos = np.zeros((9, 3), np.float32)
    pos[:, 2] = z
    mesh_id = np.array([0, 0, 1, 1, 2, 2, 0, 0, 0], np.uint32)
    visible = np.array([1, 1, 1, 1, 1, 1, 0, 1, 1], bool)                       # instance 6 is culled
    bitmap = np.array([sum(int(v) << i for i, v in enumerate(visible))], np.uint32)
    return meshes, cam, pos, mesh_id, bitmap


def test_known_answer():
    meshes, cam, pos, mesh_id, bitmap = _known_scene()
    b = br.batch_draws(pos, mesh_id, meshes, cam, bitmap, first_instance_base=1000)
    # buckets: mesh 0 LOD 0 <- 0, 7; mesh 0 LOD 1 <- 1, 8; mesh 1 LOD 0 <- 2, 3 (one LOD: far or not); mesh 2 LOD 0 <- 4;
    # instance 5 picks mesh 2's empty LOD 1 and is no member; instance 6 is culled
    want = np.array([(36, 2, 0, 0, 0), (12, 2, 36, 0, 2), (60, 2, 48, 100, 4), (24, 1, 108, -5, 6)], DRAW_CMD_DTYPE)
    assert b["count"] == 4 and b["members"] == 7
    assert b["cmds"].tobytes() == want.tobytes()
    assert b["ids"].tolist() == [1000, 1007, 1001, 1008, 1002, 1003, 1004]


def test_bits_above_n_and_empty_bitmaps():
    meshes, cam, pos, mesh_id, bitmap = _known_scene()
    a = br.batch_draws(pos, mesh_id, meshes, cam, bitmap)
    b = br.batch_draws(pos, mesh_id, meshes, cam, bitmap | np.uint32(0xFFFFFE00))   # bits 9 .. 31 belong to no instance
    assert a["cmds"].tobytes() == b["cmds"].tobytes() and a["ids"].tobytes() == b["ids"].tobytes() and a["members"] == b["members"]
    z = br.batch_draws(pos, mesh_id, meshes, cam, np.zeros(1, np.uint32))
    assert z["count"] == 0 and z["members"] == 0 and len(z["cmds"]) == 0 and len(z["ids"]) == 0
    e = br.batch_draws(np.zeros((0, 3), np.float32), np.zeros(0, np.uint32), meshes, cam, np.zeros(0, np.uint32))
    assert e["count"] == 0 and e["members"] == 0


# ---- the ABI surface: these fail on a library without the extension ----

def test_library_exports_mip_batch_draws_and_the_header_declares_it():
    import renderer_amd
    from renderer_amd import _lib

    lib = renderer_amd.load_library()
    assert hasattr(lib, "mip_batch_draws")
    assert "mip_batch_draws" in _lib.EXPORTS
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"int32_t\s+mip_batch_draws\s*\(\s*MipContext\s*\*", header)
    assert re.search(r"typedef\s+struct\s+MipBatchOutputs\s*\{", header)
    assert lib.mip_abi_version() == 4   # additive: the ABI version does not move
    assert lib.mip_batch_draws(None, None, None, None) == -1
    assert callable(getattr(renderer_amd.InstancePipeline, "batch_draws"))


def test_batch_outputs_layout_matches_the_header(tmp_path):
    from renderer_amd import _lib

    fields = ("struct_size", "flags", "batch_cmds", "batch_count", "instance_ids", "instance_count", "batch_model")
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "mi_instance_pipeline.h"\nint main(void) {\n'
           '  printf("%zu", sizeof(MipBatchOutputs));\n'
           + "".join(f'  printf(" %zu", offsetof(MipBatchOutputs, {f}));\n' for f in fields) + "  return 0;\n}\n")
    c = tmp_path / "t.c"
    c.write_text(src)
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert sizes[0] == C.sizeof(_lib.MipBatchOutputs) == 48
    assert sizes[1:] == [getattr(_lib.MipBatchOutputs, f).offset for f in fields]
