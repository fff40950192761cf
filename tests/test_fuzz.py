"""Randomised parity: oracle vs the independent numpy restatement on CPU, HIP path vs oracle on the GPU."""
import numpy as np
import pytest

import numpy_restatement as npr
from fuzz_scenes import random_geometry, random_scene
from helpers import assert_parity, same_floats


@pytest.mark.parametrize("seed", range(12))
def test_oracle_vs_numpy_restatement_random_scenes(oracle_mod, seed):
    rng = np.random.default_rng(1000 + seed)
    s = random_scene(rng, oracle_mod, n_max=3000)
    a = oracle_mod.run(s["pos"], s["rot"], s["scale"], s["mesh_id"], s["meshes"], s["planes"], s["cam_pos"],
                       first_instance_base=s["first_instance_base"], first_index_base=s["first_index_base"])
    b = npr.run(s, first_instance_base=s["first_instance_base"], first_index_base=s["first_index_base"])
    assert same_floats(a["model"], b["model"]) and same_floats(a["world_aabb"], b["world_aabb"])
    assert np.array_equal(a["coarse_culled"].astype(bool), b["coarse_culled"])
    c = a["draw_cmds"]
    assert np.array_equal(c["indexCount"], b["cmds"]["indexCount"]) and np.array_equal(c["firstIndex"], b["cmds"]["firstIndex"])
    assert np.array_equal(c["firstInstance"], b["cmds"]["firstInstance"]) and np.array_equal(c["vertexOffset"], b["cmds"]["vertexOffset"])


def _stage_inputs(seed, s):
    """The scene with the mesh table, geometry and pv of random_geometry, and small bases for the stage."""
    g = random_geometry(np.random.default_rng(5000 + seed), s)
    t = dict(s, meshes=g["meshes"])
    return t, g, int(s["first_instance_base"]), int(seed % 7)


@pytest.mark.parametrize("seed", range(12))
def test_oracle_vs_numpy_restatement_random_scenes_triangle_stage(oracle_mod, seed):
    """Row f-1 on random scenes with random geometry (any winding, index counts of every residue, special values) under the
    random camera's pv: the oracle's final commands, stream and source offsets equal the restatement's."""
    rng = np.random.default_rng(1000 + seed)
    s = random_scene(rng, oracle_mod, n_max=1500)
    t, g, fib, fxb = _stage_inputs(seed, s)
    r = oracle_mod.run(t["pos"], t["rot"], t["scale"], t["mesh_id"], t["meshes"], t["planes"], t["cam_pos"], first_instance_base=fib, first_index_base=fxb)
    capacity = fxb + r["draw_index_total"] + 3
    final, stream, src = oracle_mod.cull_all_triangles(r, t["pos"], t["mesh_id"], t["meshes"], t["cam_pos"], g["pv"], g["vertices"], g["indices"],
                                                       first_instance_base=fib, out_capacity=capacity)
    b = npr.run(t, first_instance_base=fib, first_index_base=fxb)
    src2 = npr.src_index_offsets(t["pos"], t["mesh_id"], b["coarse_culled"], t["meshes"], t["cam_pos"])
    assert np.array_equal(src, src2)
    final2, stream2 = npr.cull_all_triangles(r["draw_cmds"], src2, b["model"], fib, g["pv"], g["vertices"], g["indices"], capacity)
    assert len(final) == len(final2) and final.tobytes() == final2.tobytes()
    assert np.array_equal(stream, stream2)


def test_fuzz_camera_pv_matches_the_default_construction(oracle_mod):
    """camera_pv64 is scene.default_pv() for the default camera (bit for bit), and agrees with the oracle's float32 camera to
    float32 accuracy for random ones."""
    from fuzz_scenes import camera_pv64
    from renderer_amd import scene

    assert camera_pv64(**scene.DEFAULT_CAMERA).tobytes() == scene.default_pv().tobytes()
    rng = np.random.default_rng(3)
    for _ in range(20):
        s = random_scene(rng, oracle_mod, n_max=1)
        c = s["camera"]
        want = oracle_mod.camera_pv(c["cam_pos"], c["cam_rot_ijkw"], c["aspect"], c["fovy_degrees"], c["near"], c["far"])
        assert np.allclose(camera_pv64(**c), want, rtol=1e-4, atol=1e-4 * np.abs(want).max())


def _check_wire_form(ra, p, s, want, what):
    """The same frame emitted in the wire form (MIP_OUT_WIRE) and expanded against the mesh table (the numpy statement of what
    mip_merge_wire_lists does, tests/cpu_pipeline.py) must give the oracle's command bytes — special values, empty LODs, random
    bases and all — and the merge kernel itself must agree (one chunk)."""
    import torch

    from cpu_pipeline import decode_wire, unpack_wire
    from renderer_amd.pipeline import SHARD_HEADER_BYTES, make_frame
    from renderer_amd.sharded import chunk_stride_bytes

    n = s["n"]
    dev = torch.device("cuda", 0)
    frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=s["first_instance_base"], first_index_base=s["first_index_base"])
    for form in (True, "packed"):  # 8-byte records, packed 4-byte records
        stride = chunk_stride_bytes(max(n, 1), wire=form)
        chunk = torch.zeros(stride // 4, dtype=torch.int32, device=dev)
        merged = torch.full((max(n, 1), 5), -1, dtype=torch.int32, device=dev)
        scal = torch.zeros(2, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        base = chunk.data_ptr()
        p.run_device(frame, draw_cmds=base + SHARD_HEADER_BYTES, draw_count=base, draw_index_total=base + 4, wire=form)
        host = chunk.cpu().numpy().view(np.uint32)
        count = int(host[0])
        assert count == want["draw_count"] and int(host[1]) == want["draw_index_total"], (what, form)
        body = host[SHARD_HEADER_BYTES // 4:]
        if form == "packed":
            body = unpack_wire(body, count)
        assert decode_wire(body, count, s["meshes"]).tobytes() == want["draw_cmds"].tobytes(), (what, form)
        p.merge_wire_lists(base, 1, stride, merged.data_ptr(), scal.data_ptr(), chunk_capacity=max(n, 1), packed=form == "packed")
        assert int(scal[0].item()) == count and merged[:count].cpu().numpy().tobytes() == want["draw_cmds"].tobytes(), (what, form)


def _check_triangle_stage(ra, oracle_mod, s, trial):
    """Row f-1 over the random scene: random geometry under the random camera's pv, two frames in a context of its own (the
    second sees the first one's scratch): final commands, count, total and the whole stream against the oracle."""
    import torch

    from renderer_amd.pipeline import make_frame

    t, g, fib, fxb = _stage_inputs(trial, s)
    n = max(t["n"], 1)
    r = oracle_mod.run(t["pos"], t["rot"], t["scale"], t["mesh_id"], t["meshes"], t["planes"], t["cam_pos"], first_instance_base=fib, first_index_base=fxb)
    capacity = fxb + r["draw_index_total"] + 3
    final, stream, _ = oracle_mod.cull_all_triangles(r, t["pos"], t["mesh_id"], t["meshes"], t["cam_pos"], g["pv"], g["vertices"], g["indices"],
                                                     first_instance_base=fib, out_capacity=capacity)
    dev = torch.device("cuda", 0)
    with ra.InstancePipeline(max_instances=n, max_meshes=len(t["meshes"])) as p:
        p.set_mesh_table(t["meshes"])
        p.set_geometry(g["vertices"], g["indices"])
        p.set_instances(t["pos"], t["rot"], t["scale"], t["mesh_id"])
        model = torch.zeros((n, 16), dtype=torch.float32, device=dev)
        cmds = torch.zeros((n, 5), dtype=torch.int32, device=dev)
        scal = torch.zeros(8, dtype=torch.int32, device=dev)
        out = torch.full((capacity + 64,), -1, dtype=torch.int32, device=dev)
        frame = make_frame(t["planes"], t["cam_pos"], first_instance_base=fib, first_index_base=fxb, pv=g["pv"])
        for rep in range(2):
            out.fill_(-1)
            torch.cuda.synchronize()
            p.run_device(frame, model=model.data_ptr(), draw_cmds=cmds.data_ptr(), draw_count=scal.data_ptr(), draw_index_total=scal.data_ptr() + 4,
                         culled_index_buffer=out.data_ptr(), culled_index_capacity=capacity)
            count, total = (int(x) & 0xFFFFFFFF for x in scal[:2].cpu().tolist())
            what = f"trial {trial} n={t['n']} frame {rep}: triangle stage"
            assert count == len(final) and total == r["draw_index_total"], what
            assert cmds[:count].cpu().numpy().tobytes() == final.tobytes(), what
            got = out.cpu().numpy().view(np.uint32)
            assert np.array_equal(got[:capacity], stream) and (got[capacity:] == 0xFFFFFFFF).all(), what


@pytest.mark.gpu
def test_gpu_vs_oracle_random_scenes(oracle_mod):
    import renderer_amd as ra

    rng = np.random.default_rng(77)
    with ra.InstancePipeline(max_instances=20_000, max_meshes=64) as p:
        for trial in range(60):
            s = random_scene(rng, oracle_mod, n_max=20_000 if trial % 10 == 0 else 3000)
            p.set_mesh_table(s["meshes"])
            p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
            got = p.run_host(s["planes"], s["cam_pos"], first_instance_base=s["first_instance_base"],
                             first_index_base=s["first_index_base"])
            want = oracle_mod.run(s["pos"], s["rot"], s["scale"], s["mesh_id"], s["meshes"], s["planes"], s["cam_pos"],
                                  first_instance_base=s["first_instance_base"], first_index_base=s["first_index_base"])
            assert_parity(got, want, f"trial {trial} n={s['n']}")
            _check_wire_form(ra, p, s, want, f"trial {trial} n={s['n']}")
            if trial % 3 == 0:
                _check_triangle_stage(ra, oracle_mod, s, trial)
