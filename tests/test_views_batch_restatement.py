"""Batched draws for several views without a GPU: tests/views_batch_restatement.py (written from the header's text) against
lod_restatement.batch_draws_lods view by view, against a scene small enough to check by eye, the sentinel property of the
output buffers, the ABI surface of mip_batch_draws_views, and the launch plan either side of every pass boundary
(tests/native/batch_views_plan_check.cpp, built with the address and undefined-behaviour sanitizers)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lod_cases as lc
import lod_restatement as lr
import views_batch_restatement as vr
from renderer_amd.pipeline import MESH_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (lr.DISTANCE, lr.RELATIVE)
SENTINEL = 0x5A5A5A5A


def _random_bitmap(rng, n):
    return rng.integers(0, 1 << 32, (max(n, 1) + 31) // 32, dtype=np.uint64).astype(np.uint32)


def _scene(rng, n, n_lods):
    meshes = lc.chain_table(n_lods, seed=int(rng.integers(1, 1000)))
    meshes["index_len"][rng.random(meshes["index_len"].shape) < 0.1] = 0     # empty levels: no members
    pos = rng.normal(0, 12, (n, 3)).astype(np.float32)
    scale = rng.uniform(0.2, 3.0, n).astype(np.float32)
    mesh_id = rng.integers(0, len(meshes), n).astype(np.uint32)
    return pos, scale, mesh_id, meshes


def _views(rng, n, n_views):
    cams = rng.normal(0, 10, (n_views, 3)).astype(np.float32)
    bitmaps = [None if v % 3 == 1 else _random_bitmap(rng, n) for v in range(n_views)]
    bases = [int(b) for b in rng.integers(0, 2 ** 32, n_views)]
    return cams, bitmaps, bases


# ---- view v's slice is mip_batch_draws_lods for (frames[v], bitmaps[v]) with firstInstance shifted ----

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n_views", [1, 2, 3, 5, 16])
def test_every_view_is_batch_draws_lods_with_first_instance_shifted(mode, n_views):
    rng = np.random.default_rng(100 * n_views + mode)
    sw = (4.0, 30.0, 90.0, 250.0, 900.0) if mode == lr.DISTANCE else (0.5, 2.0, 9.0, 40.0, 200.0)
    for n in (0, 1, 63, 1000, 1025):
        pos, scale, mesh_id, meshes = _scene(rng, n, [6, 3, 1, 5, 2, 6, 4])
        cams, bitmaps, bases = _views(rng, n, n_views)
        if n_views >= 3:
            bitmaps[2] = np.zeros((max(n, 1) + 31) // 32, np.uint32)    # a view without members between two that have some
        got = vr.batch_draws_views(pos, scale, mesh_id, meshes, cams, bitmaps, bases, mode, sw)
        slot = 0
        for v in range(n_views):
            bm = lc.all_bits(n) if bitmaps[v] is None else bitmaps[v]
            one = lr.batch_draws_lods(pos, scale, mesh_id, meshes, cams[v], bm, mode, sw, first_instance_base=bases[v])
            assert int(got["first_slot"][v]) == slot and int(got["counts"][v]) == one["count"], (n, v)
            shifted = one["cmds"].copy()
            shifted["firstInstance"] += np.uint32(slot)
            assert got["cmds"][v].tobytes() == shifted.tobytes(), (n, v, "commands")
            assert got["ids"][slot: slot + one["members"]].tobytes() == one["ids"].tobytes(), (n, v, "ids")
            assert np.array_equal(got["lod"][v], one["lod"])
            slot += one["members"]
        assert int(got["first_slot"][n_views]) == slot == got["members"] == len(got["ids"])
        if n >= 1000 and n_views >= 2:
            assert got["members"] > 0 and (got["lod"][0] != got["lod"][1]).any()    # the cameras matter
        if n_views >= 3:
            assert got["counts"][2] == 0 and got["first_slot"][2] == got["first_slot"][3]


def test_two_views_that_share_a_bitmap_differ_by_their_cameras_only():
    rng = np.random.default_rng(8)
    pos, scale, mesh_id, meshes = _scene(rng, 500, [6, 6, 6])
    bm = _random_bitmap(rng, 500)
    cams = np.array([[0, 0, 0], [40, 0, 0]], np.float32)
    got = vr.batch_draws_views(pos, scale, mesh_id, meshes, cams, [bm, bm], [0, 0], lr.DISTANCE, (4.0, 30.0, 90.0, 250.0, 900.0))
    assert (got["lod"][0] != got["lod"][1]).any()
    assert got["cmds"][0]["instanceCount"].tolist() != got["cmds"][1]["instanceCount"].tolist()


# ---- a scene small enough to check by eye ----

def _hand_scene():
    """Five instances on the x axis at 1, 3, 1, 5, 0.5 with meshes 0, 0, 1, 1, 0. Mesh 0 has two levels (30 indices at 100,
    12 at 200, vertex offset 7), mesh 1 one (6 at 300, vertex offset -3): B = 3, lod_base = (0, 2). DISTANCE with
    switch_sq[0] = 4: level 1 beyond distance 2."""
    meshes = np.zeros(2, MESH_DTYPE)
    meshes["aabb_min"], meshes["aabb_max"] = -0.5, 0.5
    meshes["n_lods"] = (2, 1)
    meshes["index_len"][0, :2], meshes["index_offset"][0, :2], meshes["vertex_offset"][0] = (30, 12), (100, 200), 7
    meshes["index_len"][1, 0], meshes["index_offset"][1, 0], meshes["vertex_offset"][1] = 6, 300, -3
    pos = np.zeros((5, 3), np.float32)
    pos[:, 0] = (1, 3, 1, 5, 0.5)
    return pos, np.ones(5, np.float32), np.array([0, 0, 1, 1, 0], np.uint32), meshes, (4.0, lr.INF, lr.INF, lr.INF, lr.INF)


def test_two_views_five_instances_by_hand():
    pos, scale, mesh_id, meshes, sw = _hand_scene()
    # view 0: camera at the origin, instances 0, 1, 3, 4 visible, base 100.
    #   q = 1, 9, -, 25, 0.25 -> instance 0: bucket 0; 1: level 1, bucket 1; 3: mesh 1, bucket 2; 4: bucket 0
    #   slots: bucket 0 = (0, 4), bucket 1 = (1), bucket 2 = (3)
    # view 1: nothing visible
    cams = np.array([[0, 0, 0], [4, 0, 0]], np.float32)
    got = vr.batch_draws_views(pos, scale, mesh_id, meshes, cams, [np.array([0b11011], np.uint32), np.array([0], np.uint32)], [100, 200],
                               lr.DISTANCE, sw)
    assert got["counts"].tolist() == [3, 0] and got["first_slot"].tolist() == [0, 4, 4] and got["members"] == 4
    assert got["ids"].tolist() == [100, 104, 101, 103]
    assert got["cmds"][0].tolist() == [(30, 2, 100, 7, 0), (12, 1, 200, 7, 2), (6, 1, 300, -3, 3)] and len(got["cmds"][1]) == 0
    # the same with view 1 unculled (a NULL bitmap), camera at x = 4, base 200:
    #   q = 9, 1, 9, 1, 12.25 -> instance 0: level 1, bucket 1; 1: bucket 0; 2 and 3: bucket 2; 4: level 1, bucket 1
    #   slots behind view 0's four: bucket 0 = (1), bucket 1 = (0, 4), bucket 2 = (2, 3)
    got = vr.batch_draws_views(pos, scale, mesh_id, meshes, cams, [np.array([0b11011], np.uint32), None], [100, 200], lr.DISTANCE, sw)
    assert got["counts"].tolist() == [3, 3] and got["first_slot"].tolist() == [0, 4, 9]
    assert got["ids"].tolist() == [100, 104, 101, 103, 201, 200, 204, 202, 203]
    assert got["cmds"][0].tolist() == [(30, 2, 100, 7, 0), (12, 1, 200, 7, 2), (6, 1, 300, -3, 3)]
    assert got["cmds"][1].tolist() == [(30, 1, 100, 7, 4), (12, 2, 200, 7, 5), (6, 2, 300, -3, 7)]
    # the buffers a call leaves: cmd_stride = min(B, N) = 3, view 1's range starts at entry 3
    out = vr.fill_outputs(got, 5, 3, SENTINEL)
    assert out["cmds"][3].tolist() == [30, 1, 100, 7, 4] and (out["cmds"][6:] == SENTINEL).all()
    assert out["counts"].tolist() == [3, 3] + [SENTINEL] * 3 and out["first_slot"].tolist() == [0, 4, 9] + [SENTINEL] * 3
    assert out["ids"][:9].tolist() == got["ids"].tolist() and (out["ids"][9:] == SENTINEL).all() and len(out["ids"]) == 2 * 5 + 3


# ---- untouched entries keep the sentinel ----

@pytest.mark.parametrize("extra", [0, 5])
def test_entries_behind_a_views_count_and_behind_the_members_keep_the_sentinel(extra):
    rng = np.random.default_rng(3 + extra)
    n, n_views = 300, 4
    pos, scale, mesh_id, meshes = _scene(rng, n, [6, 3, 1, 5])
    cams, bitmaps, bases = _views(rng, n, n_views)
    bitmaps[0] = np.zeros((n + 31) // 32, np.uint32)
    want = vr.batch_draws_views(pos, scale, mesh_id, meshes, cams, bitmaps, bases, lr.RELATIVE, (0.5, 2.0, 9.0, 40.0, 200.0))
    stride = vr.min_cmd_stride(meshes, n) + extra
    assert stride == 15 + extra
    out = vr.fill_outputs(want, n, stride, SENTINEL, first_slot=bool(extra))
    touched = np.zeros(len(out["cmds"]), bool)
    for v in range(n_views):
        k = int(want["counts"][v])
        assert k <= stride
        touched[v * stride: v * stride + k] = True
        assert out["cmds"][v * stride: v * stride + k].tobytes() == want["cmds"][v].tobytes()
    assert (out["cmds"][~touched] == SENTINEL).all() and (out["cmds"][touched] != SENTINEL).any(axis=1).all()
    assert (~touched).sum() > 3 and want["counts"][0] == 0
    assert (out["ids"][want["members"]:] == SENTINEL).all() and want["members"] < n_views * n
    assert (out["first_slot"] == SENTINEL).all() == (not extra)
    with pytest.raises(ValueError):
        vr.fill_outputs(want, n, vr.min_cmd_stride(meshes, n) - 1, SENTINEL)
    with pytest.raises(ValueError):
        vr.batch_draws_views(pos, scale, mesh_id, meshes, cams[:0], [], [], lr.RELATIVE, (0.5, 2.0, 9.0, 40.0, 200.0))
    with pytest.raises(ValueError):
        vr.batch_draws_views(pos, scale, mesh_id, meshes, np.zeros((17, 3)), [None] * 17, [0] * 17, lr.DISTANCE, (1, 2, 3, 4, 5))


# ---- the ABI surface ----

def test_view_batch_outputs_layout_follows_the_header(tmp_path):
    from renderer_amd import _lib

    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "mi_instance_pipeline.h"
    int main(void) {
      printf("%zu %zu %zu %zu %zu %zu %zu %d\n", sizeof(MipViewBatchOutputs), offsetof(MipViewBatchOutputs, batch_cmds),
             offsetof(MipViewBatchOutputs, cmd_stride), offsetof(MipViewBatchOutputs, reserved), offsetof(MipViewBatchOutputs, batch_counts),
             offsetof(MipViewBatchOutputs, instance_ids), offsetof(MipViewBatchOutputs, view_first_slot), MIP_MAX_VIEWS);
      return 0;
    }'''
    c = tmp_path / "t.c"
    c.write_text(src)
    exe = str(tmp_path / "t")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe])
    sizes = [int(x) for x in subprocess.check_output([exe]).split()]
    assert sizes == [48, 8, 16, 20, 24, 32, 40, vr.MAX_VIEWS]
    m = _lib.MipViewBatchOutputs
    assert [C.sizeof(m), m.batch_cmds.offset, m.cmd_stride.offset, m.reserved.offset, m.batch_counts.offset, m.instance_ids.offset,
            m.view_first_slot.offset] == sizes[:7]
    assert "mip_batch_draws_views" in _lib.EXPORTS
    rust = open(os.path.join(ROOT, "integration", "rust", "mip-sys", "src", "lib.rs")).read()
    assert "pub fn mip_batch_draws_views(" in rust and "pub struct MipViewBatchOutputs" in rust


def test_library_exports_batch_draws_views():
    import renderer_amd

    lib = renderer_amd.load_library()
    assert lib.mip_batch_draws_views(None, None, None, 1, None, None) == -1   # a NULL context is a status code, not a crash
    assert lib.mip_abi_version() == 4


# ---- the launch plan ----

def test_views_plan_either_side_of_every_pass_boundary(tmp_path):
    """plan_batch (renderer_amd/csrc/batch_plan.hpp) for BatchEntry::views: passes from n_views x B either side of 256 and
    65 536, the kernels of every pass, the command writer, and the n_views x N capacity rule."""
    exe = str(tmp_path / "batch_views_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "native", "batch_views_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    last = out.stdout.strip().split("\n")[-1]
    assert last.startswith("VIEWS PLAN OK"), out.stdout[-2000:]
    assert int(last.split()[3]) >= 16 * 2 * 12    # every view count, both modes, four per-view bucket counts around each of three boundaries
