"""Row f-1 on the GPU: per-triangle cull + index-stream append (generate_work.comp:68-200) vs the
oracle. Bit-exact final commands, count and culled index stream."""
import numpy as np
import pytest

from triangle_variants import force_variant as _force_variant

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ra():
    import renderer_amd

    renderer_amd.load_library()
    return renderer_amd


def _run_gpu(ra, s, vertices, indices, pv, capacity, frames=1, first_instance_base=0):
    import torch

    from renderer_amd.pipeline import make_frame

    n = s["n"]
    dev = torch.device("cuda", 0)
    with ra.InstancePipeline(max_instances=max(n, 1), max_meshes=len(s["meshes"])) as p:
        p.set_mesh_table(s["meshes"])
        p.set_geometry(vertices, indices)
        p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
        model = torch.zeros((max(n, 1), 16), dtype=torch.float32, device=dev)
        cmds = torch.zeros((max(n, 1), 5), dtype=torch.int32, device=dev)
        scal = torch.zeros(8, dtype=torch.int32, device=dev)
        out = torch.full((capacity,), -1, dtype=torch.int32, device=dev)
        frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=first_instance_base, pv=pv)
        for _ in range(frames):
            out.fill_(-1)
            torch.cuda.synchronize()
            p.run_device(frame, model=model.data_ptr(), draw_cmds=cmds.data_ptr(), draw_count=scal.data_ptr(),
                         draw_index_total=scal.data_ptr() + 4, culled_index_buffer=out.data_ptr(),
                         culled_index_capacity=capacity)
        count, total = (int(x) & 0xFFFFFFFF for x in scal[:2].cpu().tolist())
        got_cmds = cmds[:count].cpu().numpy().view(np.uint32).reshape(-1).view(ra.DRAW_CMD_DTYPE)
        _run_gpu.last_timings = p.timings()
        return got_cmds, count, total, out.cpu().numpy().view(np.uint32)


def _oracle(oracle_mod, s, vertices, indices, pv, capacity, first_instance_base=0):
    r = oracle_mod.run(s["pos"], s["rot"], s["scale"], s["mesh_id"], s["meshes"], s["planes"], s["cam_pos"],
                       first_instance_base=first_instance_base, threads=8)
    cmds, out, _ = oracle_mod.cull_all_triangles(r, s["pos"], s["mesh_id"], s["meshes"], s["cam_pos"], pv, vertices, indices,
                                                 first_instance_base=first_instance_base, out_capacity=capacity)
    return r, cmds, out


# (3, 40 000): above 32 768 instances the workgroup-per-command kernel pulls its commands from the ticket counter
@pytest.mark.parametrize("config,n,allvis", [(1, 1024, False), (2, 4000, False), (3, 20_000, False), (3, 3000, True), (3, 40_000, False)])
def test_triangle_cull_matches_oracle(ra, oracle_mod, config, n, allvis):
    s = ra.scene.make_scene(config, n=n, all_visible=allvis)
    vertices, indices = ra.scene.make_geometry(s["meshes"])
    pv = ra.scene.default_pv()
    r0 = oracle_mod.run(s["pos"], s["rot"], s["scale"], s["mesh_id"], s["meshes"], s["planes"], s["cam_pos"], want=("draw_cmds",))
    capacity = r0["draw_index_total"] + 3
    r, want_cmds, want_out = _oracle(oracle_mod, s, vertices, indices, pv, capacity)
    got_cmds, count, total, got_out = _run_gpu(ra, s, vertices, indices, pv, capacity, frames=2)
    assert count == len(want_cmds) and total == r["draw_index_total"]
    assert got_cmds.tobytes() == want_cmds.tobytes()
    assert np.array_equal(got_out, want_out)
    survivors = int(want_cmds["indexCount"].astype(np.int64).sum())
    assert 0 < survivors < int(r["draw_cmds"]["indexCount"].astype(np.int64).sum())  # something was culled, something survived


@pytest.mark.parametrize("mode", ["ranges", "ranges_ticketed", "ranges_or_sorted_waves", "sorted_waves", "ranges_of_a_large_frame", "recompact_three_launches",
                                  "wave", "wave_only", "tickets", "tickets_x4", "block256", "block512", "block1024", "parts"])
def test_every_triangle_kernel_variant(ra, oracle_mod, monkeypatch, mode):
    """Round 5: the stage is the range kernel (equal ranges of the triangle stream, one per wave, or — long streams — ranges
    of MIP_TUNE_TRI_RANGE_SLOTS pulled from a counter) and, above 65 536 instances, the range kernel or the wave-per-command
    kernel over commands sorted by size class, chosen on the device. The round-4 kernels stay selectable
    (MIP_TUNE_TRI_CHUNKS_FROM=4294967295): sixteen parts per command, a 256/512/1024-thread workgroup per command (dealt by
    a stride, or pulling tickets — one or four commands each), one wave per command in list order. Each variant is forced
    (tuning variables, read by mip_create and at launch) onto the same mixed scene."""
    _force_variant(monkeypatch, mode)
    s = ra.scene.make_scene(3, n=7000)
    s["pos"][11, 1] = np.nan  # one command takes the literal (non-affine) path
    vertices, indices = ra.scene.make_geometry(s["meshes"])
    pv = ra.scene.default_pv()
    r0 = oracle_mod.run(s["pos"], s["rot"], s["scale"], s["mesh_id"], s["meshes"], s["planes"], s["cam_pos"], want=("draw_cmds",))
    capacity = r0["draw_index_total"] + 3
    r, want_cmds, want_out = _oracle(oracle_mod, s, vertices, indices, pv, capacity, first_instance_base=17)
    got_cmds, count, total, got_out = _run_gpu(ra, s, vertices, indices, pv, capacity, frames=2, first_instance_base=17)
    assert count == len(want_cmds) and total == r["draw_index_total"], mode
    assert got_cmds.tobytes() == want_cmds.tobytes(), mode
    assert np.array_equal(got_out, want_out), mode


@pytest.mark.parametrize("ordering", ["rows", "strips", "shuffled"])
@pytest.mark.parametrize("config,n", [(3, 7000), (2, 1500)])
def test_wave_kernel_vertex_ring_on_every_mesh_layout(ra, oracle_mod, monkeypatch, ordering, config, n):
    """The wave-per-command kernel transforms a step's vertex range once into its LDS ring when that is cheaper than
    the per-corner path. The bytes must not depend on which path a step took: the same surfaces listed row by row
    (ranges of a few hundred vertices: ring, window carried from step to step), as first-use-ordered strips (the layout
    of an optimised mesh), and with shuffled triangles (every step spans the mesh: per-corner path), with non-finite
    positions (literal chain), a NaN matrix, tiny meshes whose window runs past their vertices, and the last mesh of
    the consolidated buffer (the ring loads ahead of the indices it has seen: clamped at the buffer's end)."""
    monkeypatch.setenv("MIP_TUNE_TRI_BLOCK_MAX", "0")
    monkeypatch.setenv("MIP_TUNE_TRI_PARTS_MAX", "0")
    monkeypatch.setenv("MIP_TUNE_TRI_CHOICE", "waves")  # (round 5: the large-frame pairing is range kernel | sorted wave-per-command kernel)
    s = ra.scene.make_scene(config, n=n, all_visible=(config == 2))
    s["pos"][11, 1] = np.nan
    vertices, indices = ra.scene.make_geometry(s["meshes"], ordering=ordering)
    pv = ra.scene.default_pv()
    r0 = oracle_mod.run(s["pos"], s["rot"], s["scale"], s["mesh_id"], s["meshes"], s["planes"], s["cam_pos"], want=("draw_cmds",))
    capacity = r0["draw_index_total"] + 3
    for poison in (False, True):
        if poison:  # non-finite positions switch the affine shortcut off for the whole geometry
            vertices = vertices.copy()
            vertices[min(10, len(vertices) - 1), 0] = np.inf
            vertices[len(vertices) // 2, 2] = np.nan
        r, want_cmds, want_out = _oracle(oracle_mod, s, vertices, indices, pv, capacity, first_instance_base=5)
        got_cmds, count, total, got_out = _run_gpu(ra, s, vertices, indices, pv, capacity, frames=2, first_instance_base=5)
        assert count == len(want_cmds) and total == r["draw_index_total"], (ordering, poison)
        assert got_cmds.tobytes() == want_cmds.tobytes(), (ordering, poison)
        assert np.array_equal(got_out, want_out), (ordering, poison)


def test_triangle_cull_special_instances_and_bases(ra, oracle_mod):
    s = ra.scene.make_scene(3, n=2000, all_visible=True)
    s["pos"][5, 0] = np.nan          # NaN model matrix: every comparison is false, so every triangle survives
    s["scale"][7] = 0.0              # degenerate: all vertices coincide
    s["scale"][9] = -1.0             # mirrored: winding flips
    s["rot"][11] = (0, 0, 0, 3.0)    # non-unit quaternion
    vertices, indices = ra.scene.make_geometry(s["meshes"])
    pv = ra.scene.default_pv()
    r0 = oracle_mod.run(s["pos"], s["rot"], s["scale"], s["mesh_id"], s["meshes"], s["planes"], s["cam_pos"], want=("draw_cmds",))
    capacity = r0["draw_index_total"] + 3
    r, want_cmds, want_out = _oracle(oracle_mod, s, vertices, indices, pv, capacity, first_instance_base=1000)
    got_cmds, count, total, got_out = _run_gpu(ra, s, vertices, indices, pv, capacity, first_instance_base=1000)
    assert count == len(want_cmds) and got_cmds.tobytes() == want_cmds.tobytes()
    assert np.array_equal(got_out, want_out)


@pytest.mark.parametrize("range_slots", [None, "256"])
def test_triangle_cull_index_base_and_index_counts_that_are_no_multiple_of_three(ra, oracle_mod, monkeypatch, range_slots):
    """The range kernel numbers the frame's triangles by (firstIndex - first_index_base) / 3: a first_index_base that is no
    multiple of 3, and meshes whose index counts are not (the last one or two indices of a command are no triangle; such
    commands leave unused slots in the stream, and a command of one or two indices has no triangle at all), with one range
    per wave and with 256-slot ranges: bytes equal to the oracle's."""
    import torch

    from renderer_amd.pipeline import make_frame

    if range_slots:
        monkeypatch.setenv("MIP_TUNE_TRI_RANGE_SLOTS", range_slots)
    s = ra.scene.make_scene(3, n=5000)
    meshes = s["meshes"].copy()
    for k in range(len(meshes)):
        for lod in range(int(meshes["n_lods"][k])):
            if (k + lod) % 3 == 1 and meshes["index_len"][k][lod] > 4:
                meshes["index_len"][k][lod] -= 1 + (k % 2)
    meshes["index_len"][5][:] = 2   # commands without a triangle
    meshes["index_len"][9][:] = 1
    s["meshes"] = meshes
    vertices, indices = ra.scene.make_geometry(ra.scene.make_scene(3, n=5000)["meshes"])  # the geometry of the unshortened table
    pv = ra.scene.default_pv()
    base = 5
    r = oracle_mod.run(s["pos"], s["rot"], s["scale"], s["mesh_id"], s["meshes"], s["planes"], s["cam_pos"], first_index_base=base, threads=8)
    capacity = base + r["draw_index_total"] + 3
    want_cmds, want_out, _ = oracle_mod.cull_all_triangles(r, s["pos"], s["mesh_id"], s["meshes"], s["cam_pos"], pv, vertices, indices, out_capacity=capacity)
    dev = torch.device("cuda", 0)
    n = s["n"]
    with ra.InstancePipeline(max_instances=n, max_meshes=len(s["meshes"])) as p:
        p.set_mesh_table(s["meshes"])
        p.set_geometry(vertices, indices)
        p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
        model = torch.zeros((n, 16), dtype=torch.float32, device=dev)
        cmds = torch.zeros((n, 5), dtype=torch.int32, device=dev)
        scal = torch.zeros(8, dtype=torch.int32, device=dev)
        out = torch.full((capacity,), -1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        for _ in range(2):
            out.fill_(-1)
            torch.cuda.synchronize()
            p.run_device(make_frame(s["planes"], s["cam_pos"], first_index_base=base, pv=pv), model=model.data_ptr(), draw_cmds=cmds.data_ptr(),
                         draw_count=scal.data_ptr(), draw_index_total=scal.data_ptr() + 4, culled_index_buffer=out.data_ptr(), culled_index_capacity=capacity)
        count = int(scal[0].item())
        got_cmds = cmds[:count].cpu().numpy().view(np.uint32).reshape(-1).view(ra.DRAW_CMD_DTYPE)
        assert count == len(want_cmds) and got_cmds.tobytes() == want_cmds.tobytes()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want_out)


@pytest.mark.parametrize("large_frame_path", [False, True])
def test_triangle_stage_with_frames_in_flight(ra, oracle_mod, monkeypatch, large_frame_path):
    """Two frame slots, two cameras, asynchronous frames alternating between them: every slot owns its scratch (command list, final
    counts, range map and granules, size-class table and ticket counter), so the culled streams of frames that overlap on the device
    are each the oracle's — with the range kernel alone and with the large-frame pairing (sort kernels + both grids)."""
    import torch

    from renderer_amd.pipeline import make_frame

    if large_frame_path:
        monkeypatch.setenv("MIP_TUNE_TRI_BLOCK_MAX", "0")
    s = ra.scene.make_scene(3, n=6000)
    vertices, indices = ra.scene.make_geometry(s["meshes"])
    pv = ra.scene.default_pv()
    cams = [np.array(c, np.float32) for c in ((0, 1, 2), (5, 1, -20))]
    planes = [s["planes"], oracle_mod.project_camera(cams[1], (0.0, 0.0, 0.0, 1.0))]
    wants = []
    for k in range(2):
        r = oracle_mod.run(s["pos"], s["rot"], s["scale"], s["mesh_id"], s["meshes"], planes[k], cams[k], threads=8)
        cap = r["draw_index_total"] + 3
        wc, wo, _ = oracle_mod.cull_all_triangles(r, s["pos"], s["mesh_id"], s["meshes"], cams[k], pv, vertices, indices, out_capacity=cap)
        wants.append((cap, wc, wo))
    dev = torch.device("cuda", 0)
    n = s["n"]
    with ra.InstancePipeline(max_instances=n, max_meshes=len(s["meshes"]), frames_in_flight=2) as p:
        p.set_mesh_table(s["meshes"])
        p.set_geometry(vertices, indices)
        p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
        bufs = []
        for k in range(2):
            bufs.append(dict(model=torch.zeros((n, 16), dtype=torch.float32, device=dev), cmds=torch.zeros((n, 5), dtype=torch.int32, device=dev),
                             scal=torch.zeros(8, dtype=torch.int32, device=dev), out=torch.full((wants[k][0],), -1, dtype=torch.int32, device=dev)))
        torch.cuda.synchronize()
        for rep in range(6):  # 12 asynchronous frames rotating over the two slots
            for k in range(2):
                b = bufs[k]
                p.run_device(make_frame(planes[k], cams[k], pv=pv), model=b["model"].data_ptr(), draw_cmds=b["cmds"].data_ptr(), draw_count=b["scal"].data_ptr(),
                             draw_index_total=b["scal"].data_ptr() + 4, culled_index_buffer=b["out"].data_ptr(), culled_index_capacity=wants[k][0], async_=True)
        p.wait()
        for k in range(2):
            b = bufs[k]
            count = int(b["scal"][0].item())
            got = b["cmds"][:count].cpu().numpy().view(np.uint32).reshape(-1).view(ra.DRAW_CMD_DTYPE)
            assert count == len(wants[k][1]) and got.tobytes() == wants[k][1].tobytes(), k
            assert np.array_equal(b["out"].cpu().numpy().view(np.uint32), wants[k][2]), k


def test_ranges_of_a_stream_whose_every_command_has_two_indices_too_many(ra, oracle_mod, monkeypatch):
    """One mesh whose index counts are 3 k + 2, every instance visible, an index buffer far larger than the frame needs: the stream is
    then LONGER in slots than instances x triangles of the largest command (the slots are numbered by the running sum of indexCount / 3,
    and every command pushes the later ones up by 2/3 of a slot) — the bound the host sizes the range map by has to allow for that, or
    the last ranges of the frame are never walked."""
    import torch

    from renderer_amd.pipeline import make_frame

    monkeypatch.setenv("MIP_TUNE_TRI_RANGE_SLOTS", "256")
    s = ra.scene.make_scene(2, n=3000, all_visible=True)
    vertices, indices = ra.scene.make_geometry(s["meshes"])
    meshes = s["meshes"].copy()
    for lod in range(int(meshes["n_lods"][0])):
        meshes["index_len"][0][lod] = meshes["index_len"][0][lod] // 3 * 3 - 1   # 3 k + 2
    s["meshes"] = meshes
    pv = ra.scene.default_pv()
    r = oracle_mod.run(s["pos"], s["rot"], s["scale"], s["mesh_id"], s["meshes"], s["planes"], s["cam_pos"], threads=8)
    capacity = 2 * r["draw_index_total"] + 64
    want_cmds, want_out, _ = oracle_mod.cull_all_triangles(r, s["pos"], s["mesh_id"], s["meshes"], s["cam_pos"], pv, vertices, indices, out_capacity=capacity)
    got_cmds, count, total, got_out = _run_gpu(ra, s, vertices, indices, pv, capacity)
    assert count == len(want_cmds) and total == r["draw_index_total"]
    assert got_cmds.tobytes() == want_cmds.tobytes()
    assert np.array_equal(got_out, want_out)


def test_triangle_cull_with_non_finite_positions(ra, oracle_mod):
    """Positions that are not finite switch off the affine shortcut (0 * inf is not 0): the literal
    mat4 * vec4 chain must then reproduce the oracle, including for instances with ordinary matrices."""
    for n in (300, 30_000):  # workgroup-per-command and wave-per-command kernels
        s = ra.scene.make_scene(2, n=n, all_visible=(n == 300))
        vertices, indices = ra.scene.make_geometry(s["meshes"])
        vertices = vertices.copy()
        vertices[10, 0] = np.inf
        vertices[200, 1] = -np.inf
        vertices[3000, 2] = np.nan
        pv = ra.scene.default_pv()
        r0 = oracle_mod.run(s["pos"], s["rot"], s["scale"], s["mesh_id"], s["meshes"], s["planes"], s["cam_pos"], want=("draw_cmds",))
        capacity = r0["draw_index_total"] + 3
        r, want_cmds, want_out = _oracle(oracle_mod, s, vertices, indices, pv, capacity)
        got_cmds, count, total, got_out = _run_gpu(ra, s, vertices, indices, pv, capacity)
        assert count == len(want_cmds) and got_cmds.tobytes() == want_cmds.tobytes(), n
        assert np.array_equal(got_out, want_out), n


def test_triangle_cull_reports_a_short_index_buffer(ra, oracle_mod):
    s = ra.scene.make_scene(2, n=500, all_visible=True)
    vertices, indices = ra.scene.make_geometry(s["meshes"])
    with pytest.raises(ra.MipError) as e:
        _run_gpu(ra, s, vertices, indices, ra.scene.default_pv(), capacity=46356 * 10)
    assert e.value.code == -4
    # and the stage refuses to run without geometry / on host outputs
    import torch

    from renderer_amd.pipeline import make_frame

    with ra.InstancePipeline(max_instances=500, max_meshes=1) as p:
        p.set_mesh_table(s["meshes"])
        p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
        buf = torch.zeros(1024, dtype=torch.int32, device="cuda")
        with pytest.raises(ra.MipError) as e:
            p.run_device(make_frame(s["planes"], s["cam_pos"]), model=buf.data_ptr(), draw_cmds=buf.data_ptr(),
                         draw_count=buf.data_ptr(), culled_index_buffer=buf.data_ptr(), culled_index_capacity=1024)
        assert e.value.code == -6


@pytest.mark.parametrize("config,n", [(2, 100_000), (3, 200_000)])
def test_triangle_cull_at_baseline_sizes(ra, oracle_mod, config, n):
    """Row f-1 at the sizes the bench runs: BASELINE configs[1] in full (100 k instances, 27 k commands, 213 M
    triangles in) and the mixed scene at 200 k (114 M triangles). Above 65 536 instances the library selects
    the one-wave-per-command kernel and the wide re-compaction by itself — nothing is forced here. Every
    final command, the count and the WHOLE culled index stream (gaps included) against the oracle."""
    s = ra.scene.make_scene(config, n=n)
    vertices, indices = ra.scene.make_geometry(s["meshes"])
    pv = ra.scene.default_pv()
    r = oracle_mod.run(s["pos"], s["rot"], s["scale"], s["mesh_id"], s["meshes"], s["planes"], s["cam_pos"], threads=16)
    capacity = r["draw_index_total"] + 3
    assert capacity > 300_000_000  # hundreds of millions of indices: the regime of the bench leg
    want_cmds, want_out, _ = oracle_mod.cull_all_triangles(r, s["pos"], s["mesh_id"], s["meshes"], s["cam_pos"], pv, vertices, indices,
                                                           out_capacity=capacity, threads=16)
    got_cmds, count, total, got_out = _run_gpu(ra, s, vertices, indices, pv, capacity, frames=1)
    assert count == len(want_cmds) and total == r["draw_index_total"]
    assert got_cmds.tobytes() == want_cmds.tobytes()
    assert np.array_equal(got_out, want_out)
    survivors = int(want_cmds["indexCount"].astype(np.int64).sum())
    assert 0.2 < survivors / int(r["draw_cmds"]["indexCount"].astype(np.int64).sum()) < 0.8


@pytest.mark.parametrize("fault", ["reverse", "skip"])
def test_parts_kernel_does_not_depend_on_who_runs_when(oracle_mod, fault):
    """The kernels that cut a command between waves — round 5's range kernel (a range's continuing segment goes behind the
    survivors its command has in the earlier ranges), with one range per wave and with 256-slot ranges pulled from the
    counter, and round 4's parts kernel (16 work items per command) — in the diagnostic build, with the work dealt from the
    LAST item down ("reverse": later ranges start first), and with every 16th range / one part of every command that NEVER
    publishes ("skip": its successors have to count its survivors themselves — MipTimings.prefix_helps says they did): the
    stream still equals the oracle's. No wait depends on another workgroup ever running (rounds 2-3: a bounded wait,
    MIP_ERR_TIMEOUT and the kernel switched off for the context)."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r'''
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
os.environ["MIP_LIBRARY"] = os.path.join(sys.argv[1], "renderer_amd", "lib", "libmi_instance_pipeline_dbg.so")
os.environ["MIP_TUNE_TRI_PARTS_MAX"] = "100000000"
if sys.argv[2] == "reverse":
    os.environ["MIP_DEBUG_TILE_ORDER"] = "reverse"
else:
    os.environ["MIP_DEBUG_SKIP_PART"] = "3"
import numpy as np
import oracle, renderer_amd
from test_gpu_triangles import _oracle, _run_gpu
import torch
for config, n, knobs in ((3, 3000, {}), (2, 700, {}), (3, 3000, {"MIP_TUNE_TRI_RANGE_SLOTS": "256"}), (2, 700, {"MIP_TUNE_TRI_RANGE_SLOTS": "256"}),
                         (3, 9000, {"MIP_TUNE_TRI_BLOCK_MAX": "0"}),   # the large-frame path: the one-launch re-compaction over 9 workgroups, every fourth silent under "skip"
                         (3, 9000, {"MIP_TUNE_TRI_BLOCK_MAX": "0", "MIP_TUNE_TRI_CHOICE": "waves"}),
                         (3, 3000, {"MIP_TUNE_TRI_CHUNKS_FROM": "4294967295"}), (2, 700, {"MIP_TUNE_TRI_CHUNKS_FROM": "4294967295"})):
    for k in ("MIP_TUNE_TRI_RANGE_SLOTS", "MIP_TUNE_TRI_CHUNKS_FROM", "MIP_TUNE_TRI_BLOCK_MAX", "MIP_TUNE_TRI_CHOICE"):
        os.environ.pop(k, None)
    os.environ.update(knobs)   # (read when the context is created)
    s = renderer_amd.scene.make_scene(config, n=n)
    vertices, indices = renderer_amd.scene.make_geometry(s["meshes"])
    pv = renderer_amd.scene.default_pv()
    r0 = oracle.run(s["pos"], s["rot"], s["scale"], s["mesh_id"], s["meshes"], s["planes"], s["cam_pos"], want=("draw_cmds",))
    capacity = r0["draw_index_total"] + 3
    r, want_cmds, want_out = _oracle(oracle, s, vertices, indices, pv, capacity)
    got_cmds, count, total, got_out = _run_gpu(renderer_amd, s, vertices, indices, pv, capacity, frames=2)
    assert count == len(want_cmds), (config, n, knobs, count, len(want_cmds))
    assert got_cmds.tobytes() == want_cmds.tobytes(), (config, n, knobs, "commands", int((got_cmds != want_cmds).sum()))
    assert np.array_equal(got_out, want_out), (config, n, knobs, "index stream", int((got_out != want_out).sum()), int(np.nonzero(got_out != want_out)[0][0]))
    if sys.argv[2] == "skip":   # (in reverse order the predecessors are usually published in time by their own workgroups)
        assert _run_gpu.last_timings["prefix_helps"] > 0, _run_gpu.last_timings
print("PARTS OK")
'''
    out = subprocess.run([sys.executable, "-c", code, root, fault], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "PARTS OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]


# ---- committed fixtures, the overflow contract, degenerate frames ---------------------------------------------------

SENTINEL = 0xFFFFFFFF


class _Stage:
    """One context over a scene and its geometry, with outputs the test owns: the index buffer is allocated at `alloc` words
    whatever capacity a frame is given, so a kernel that ignored the capacity would write into the test's own memory."""

    def __init__(self, ra, s, vertices, indices, alloc, frames_in_flight=1, n_slots=1):
        import torch

        self.ra, self.torch, self.s = ra, torch, s
        n = max(s["n"], 1)
        dev = torch.device("cuda", 0)
        self.p = ra.InstancePipeline(max_instances=n, max_meshes=len(s["meshes"]), frames_in_flight=frames_in_flight)
        self.p.set_mesh_table(s["meshes"])
        self.p.set_geometry(vertices, indices)
        self.p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
        self.bufs = [dict(model=torch.zeros((n, 16), dtype=torch.float32, device=dev), cmds=torch.zeros((n, 5), dtype=torch.int32, device=dev),
                          scal=torch.zeros(8, dtype=torch.int32, device=dev), out=torch.full((alloc,), -1, dtype=torch.int32, device=dev))
                     for _ in range(n_slots)]

    def close(self):
        self.p.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def enqueue(self, frame, capacity, slot=0, async_=False):
        b = self.bufs[slot]
        self.p.run_device(frame, model=b["model"].data_ptr(), draw_cmds=b["cmds"].data_ptr(), draw_count=b["scal"].data_ptr(),
                          draw_index_total=b["scal"].data_ptr() + 4, culled_index_buffer=b["out"].data_ptr(), culled_index_capacity=capacity,
                          async_=async_)

    def read(self, slot=0):
        b = self.bufs[slot]
        count, total = (int(x) & 0xFFFFFFFF for x in b["scal"][:2].cpu().tolist())
        cmds = b["cmds"][:count].cpu().numpy().view(np.uint32).reshape(-1).view(self.ra.DRAW_CMD_DTYPE)
        return cmds, count, total, b["out"].cpu().numpy().view(np.uint32)

    def run(self, frame, capacity, slot=0):
        """One synchronous frame into a freshly sentinel-filled buffer. Returns (status, commands, count, total, whole buffer)."""
        self.bufs[slot]["out"].fill_(-1)
        self.bufs[slot]["cmds"].fill_(0x5A5A5A5A)
        self.torch.cuda.synchronize()
        status = 0
        try:
            self.enqueue(frame, capacity, slot)
        except self.ra.MipError as e:
            status = e.code
        return (status,) + self.read(slot)


def _assert_frame(got, want_cmds, want_total, want_stream, what, status=0):
    g_status, g_cmds, g_count, g_total, g_out = got
    assert g_status == status, (what, g_status)
    assert g_count == len(want_cmds) and g_total == want_total, (what, g_count, len(want_cmds), g_total, want_total)
    assert g_cmds.tobytes() == want_cmds.tobytes(), (what, "commands")
    assert len(g_out) >= len(want_stream)
    assert np.array_equal(g_out[: len(want_stream)], want_stream), (what, "stream", int((g_out[: len(want_stream)] != want_stream).sum()))
    assert (g_out[len(want_stream):] == SENTINEL).all(), (what, "words behind the capacity were written")


@pytest.mark.parametrize("large_frame_path", [False, True])
@pytest.mark.parametrize("name", ["triangles_mixed_300", "triangles_special_24", "triangles_bases_200"])
def test_committed_triangle_fixtures(ra, monkeypatch, name, large_frame_path):
    """tests/golden/ext/triangles_*.npz through mip_run: final commands, count, total and the whole culled stream are the
    committed bytes (which the oracle and the numpy restatement both reproduce: tests/test_oracle.py)."""
    import os

    from renderer_amd.pipeline import make_frame

    if large_frame_path:
        monkeypatch.setenv("MIP_TUNE_TRI_BLOCK_MAX", "0")
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ext", name + ".npz"))
    s = dict(n=len(g["pos"]), pos=g["pos"], rot=g["rot"], scale=g["scale"], mesh_id=g["mesh_id"], meshes=g["meshes"])
    capacity = len(g["culled_stream"])
    frame = make_frame(g["planes"], g["cam_pos"], first_instance_base=int(g["first_instance_base"]), first_index_base=int(g["first_index_base"]), pv=g["pv"])
    with _Stage(ra, s, g["vertices"], g["indices"], capacity + 64) as st:
        for rep in range(2):
            _assert_frame(st.run(frame, capacity), g["final_cmds"], int(g["draw_index_total"]), g["culled_stream"], (name, rep))


_OVERFLOW_SCENE = {}


def _overflow_scene(ra, oracle_mod):
    """The scene of test_every_triangle_kernel_variant, its oracle frame and the three short capacities (computed once)."""
    if not _OVERFLOW_SCENE:
        s = ra.scene.make_scene(3, n=7000)
        s["pos"][11, 1] = np.nan
        vertices, indices = ra.scene.make_geometry(s["meshes"])
        pv = ra.scene.default_pv()
        r0 = oracle_mod.run(s["pos"], s["rot"], s["scale"], s["mesh_id"], s["meshes"], s["planes"], s["cam_pos"], want=("draw_cmds",))
        full = r0["draw_index_total"] + 3
        r, want_cmds, want_out = _oracle(oracle_mod, s, vertices, indices, pv, full, first_instance_base=17)
        frame_cmds = r["draw_cmds"]
        ends = frame_cmds["firstIndex"].astype(np.int64) + frame_cmds["indexCount"].astype(np.int64)
        k = int(np.searchsorted(ends, 0.4 * full))
        assert frame_cmds["indexCount"][k] > 6 and 0 < k < len(frame_cmds) - 1
        caps = {"inside_a_command": int(frame_cmds["firstIndex"][k]) + int(frame_cmds["indexCount"][k]) // 2, "at_a_command_boundary": int(ends[k]), "zero": 0}
        _OVERFLOW_SCENE.update(s=s, vertices=vertices, indices=indices, pv=pv, full=full, r=r, want_cmds=want_cmds, want_out=want_out, ends=ends, caps=caps)
    return _OVERFLOW_SCENE


def _expected_short_frame(o, capacity, alloc):
    """What the contract (include/mi_instance_pipeline.h, culled_index_capacity) leaves of the oracle's frame: the final
    commands whose FRAME range [firstIndex, firstIndex + indexCount) fits, their part of the stream, the sentinel elsewhere."""
    frame_cmds = o["r"]["draw_cmds"]
    fits = o["ends"] <= capacity
    n_fit = int(fits.sum())
    assert fits[:n_fit].all()                                   # the commands ascend in firstIndex: the ones that fit are a prefix
    fitting = set(frame_cmds["firstInstance"][:n_fit].tolist())
    keep = np.array([int(f) in fitting for f in o["want_cmds"]["firstInstance"]], bool)
    cut = int(o["ends"][n_fit - 1]) if n_fit else 0
    stream = np.full(alloc, SENTINEL, np.uint32)
    stream[:cut] = o["want_out"][:cut]
    return o["want_cmds"][keep], stream


@pytest.mark.parametrize("mode", ["ranges", "ranges_ticketed", "ranges_of_a_large_frame", "ranges_or_sorted_waves", "sorted_waves", "recompact_three_launches",
                                  "parts", "block256", "tickets", "wave"])
def test_triangle_overflow_contract(ra, oracle_mod, monkeypatch, mode):
    """culled_index_capacity shorter than the frame needs (include/mi_instance_pipeline.h), on every decomposition: the call
    returns MIP_ERR_CAPACITY; no word at or behind the capacity is written; the commands that fit keep their oracle bytes and
    their part of the stream; the commands that do not fit are absent from the compacted list and write nothing; draw_count
    counts what is there, draw_index_total keeps the frame's value; the context stays usable. The buffer is allocated at the
    full size plus a guard tail throughout, a full-capacity frame runs first (so the slot's scratch holds real counts that
    must not resurface), and a fresh context takes a short frame as its FIRST (so nothing the scratch was allocated with
    resurfaces either)."""
    from renderer_amd.pipeline import make_frame

    _force_variant(monkeypatch, mode)
    o = _overflow_scene(ra, oracle_mod)
    s, full = o["s"], o["full"]
    alloc = full + 4096
    total = o["r"]["draw_index_total"]
    frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=17, pv=o["pv"])
    full_stream = np.concatenate([o["want_out"], np.full(alloc - full, SENTINEL, np.uint32)])
    with _Stage(ra, s, o["vertices"], o["indices"], alloc) as st:
        _assert_frame(st.run(frame, full), o["want_cmds"], total, full_stream, (mode, "full capacity, first"))
        for what, capacity in o["caps"].items():
            want_cmds, want_stream = _expected_short_frame(o, capacity, alloc)
            assert len(want_cmds) < len(o["want_cmds"])
            _assert_frame(st.run(frame, capacity), want_cmds, total, want_stream, (mode, what, capacity), status=-4)
            _assert_frame(st.run(frame, full), o["want_cmds"], total, full_stream, (mode, "full capacity after", what))
    with _Stage(ra, s, o["vertices"], o["indices"], alloc) as st:
        for what in ("zero", "inside_a_command"):
            want_cmds, want_stream = _expected_short_frame(o, o["caps"][what], alloc)
            _assert_frame(st.run(frame, o["caps"][what]), want_cmds, total, want_stream, (mode, "fresh context", what), status=-4)
        _assert_frame(st.run(frame, full), o["want_cmds"], total, full_stream, (mode, "fresh context, full capacity"))


@pytest.mark.parametrize("large_frame_path", [False, True])
def test_triangle_overflow_of_a_frame_in_flight_is_reported_by_wait(ra, oracle_mod, monkeypatch, large_frame_path):
    """Two slots, two asynchronous frames in flight: slot 0's at full capacity, slot 1's with a short buffer. mip_wait returns
    MIP_ERR_CAPACITY; slot 0's frame is the oracle's, slot 1's is what the contract leaves; the next wait is clean."""
    from renderer_amd.pipeline import make_frame

    if large_frame_path:
        monkeypatch.setenv("MIP_TUNE_TRI_BLOCK_MAX", "0")
    o = _overflow_scene(ra, oracle_mod)
    s, full = o["s"], o["full"]
    alloc = full + 4096
    total = o["r"]["draw_index_total"]
    frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=17, pv=o["pv"])
    full_stream = np.concatenate([o["want_out"], np.full(alloc - full, SENTINEL, np.uint32)])
    capacity = o["caps"]["inside_a_command"]
    want_cmds, want_stream = _expected_short_frame(o, capacity, alloc)
    with _Stage(ra, s, o["vertices"], o["indices"], alloc, frames_in_flight=2, n_slots=2) as st:
        for rep in range(2):   # the second round sees the first one's scratch in both slots
            for b in st.bufs:
                b["out"].fill_(-1)
            st.torch.cuda.synchronize()
            st.enqueue(frame, full, slot=0, async_=True)
            st.enqueue(frame, capacity, slot=1, async_=True)
            with pytest.raises(ra.MipError) as e:
                st.p.wait()
            assert e.value.code == -4
            _assert_frame((0,) + st.read(0), o["want_cmds"], total, full_stream, (rep, "the other slot's frame"))
            _assert_frame((0,) + st.read(1), want_cmds, total, want_stream, (rep, "the short frame"))
            st.p.wait()            # reported once
        st.enqueue(frame, full, slot=0, async_=True)
        st.enqueue(frame, full, slot=1, async_=True)
        st.p.wait()
        for k in range(2):
            _assert_frame((0,) + st.read(k), o["want_cmds"], total, full_stream, ("both at full capacity", k))


def _oracle_and_restatement(oracle_mod, s, vertices, indices, pv, capacity):
    """The oracle's frame and final (commands, stream), checked against the numpy restatement's."""
    import numpy_restatement as npr

    r, want_cmds, want_out = _oracle(oracle_mod, s, vertices, indices, pv, capacity)
    src = npr.src_index_offsets(s["pos"], s["mesh_id"], r["coarse_culled"], s["meshes"], s["cam_pos"])
    cmds2, out2 = npr.cull_all_triangles(r["draw_cmds"], src, r["model"], 0, pv, vertices, indices, capacity)
    assert cmds2.tobytes() == want_cmds.tobytes() and np.array_equal(out2, want_out)
    return r, want_cmds, want_out


def _one_triangle_scene(ra, corners):
    """One instance (identity, at the origin) of one mesh of exactly one triangle."""
    meshes = np.zeros(1, ra.MESH_DTYPE)
    c = np.array(corners, np.float32)
    meshes["aabb_min"], meshes["aabb_max"] = c.min(axis=0), c.max(axis=0) + np.float32(0.01)
    meshes["n_lods"] = 1
    meshes["index_len"][0, 0] = 3
    s = dict(n=1, pos=np.zeros((1, 3), np.float32), rot=np.array([[0, 0, 0, 1]], np.float32), scale=np.ones(1, np.float32),
             mesh_id=np.zeros(1, np.uint32), meshes=meshes, planes=ra.scene.default_planes(), cam_pos=np.array([0, 1, 2], np.float32))
    return s, c, np.arange(3, dtype=np.uint32)


@pytest.mark.parametrize("large_frame_path", [False, True])
def test_degenerate_frames_through_the_triangle_stage(ra, oracle_mod, monkeypatch, large_frame_path):
    """Frames that end early in the stage, each twice (the second sees the first one's scratch), each followed by a normal
    frame in the same context, each against the oracle AND the numpy restatement: no instance passes the frustum (no
    command: the stage kernels return on count == 0); commands are emitted but every triangle dies (draw_count 0 after the
    re-compaction, draw_index_total keeps the frame's value); the stream is untouched both times."""
    from renderer_amd.pipeline import make_frame

    if large_frame_path:
        monkeypatch.setenv("MIP_TUNE_TRI_BLOCK_MAX", "0")
    s = ra.scene.make_scene(3, n=3000)
    vertices, indices = ra.scene.make_geometry(s["meshes"])
    pv = ra.scene.default_pv()
    r0 = oracle_mod.run(s["pos"], s["rot"], s["scale"], s["mesh_id"], s["meshes"], s["planes"], s["cam_pos"], want=("draw_cmds",))
    capacity = r0["draw_index_total"] + 3
    alloc = capacity + 64
    r, want_cmds, want_out = _oracle_and_restatement(oracle_mod, s, vertices, indices, pv, capacity)
    normal = make_frame(s["planes"], s["cam_pos"], pv=pv)
    pad = np.full(alloc - capacity, SENTINEL, np.uint32)
    untouched = np.full(alloc, SENTINEL, np.uint32)
    none = np.zeros(0, ra.DRAW_CMD_DTYPE)
    # a camera that looks away from everything: the same frustum 10 000 units up
    away_cam = np.array([0, 10_000, 2], np.float32)
    away_planes = oracle_mod.project_camera(away_cam, (0.0, 0.0, 0.0, 1.0))
    s_away = dict(s, planes=away_planes, cam_pos=away_cam)
    ra_, aw_cmds, aw_out = _oracle_and_restatement(oracle_mod, s_away, vertices, indices, pv, capacity)
    assert ra_["draw_count"] == 0 and len(aw_cmds) == 0 and (aw_out == SENTINEL).all()
    # a pv whose x row is 3 w: clip.x = 3 clip.w for every vertex, NDC.x = 3 > 1 (or NaN): every triangle is culled
    pv_dead = pv.copy().reshape(4, 4)
    pv_dead[:, 0] = 3.0 * pv_dead[:, 3]
    pv_dead = pv_dead.reshape(16)
    rd, dead_cmds, dead_out = _oracle_and_restatement(oracle_mod, s, vertices, indices, pv_dead, capacity)
    assert rd["draw_count"] > 100 and len(dead_cmds) == 0 and (dead_out == SENTINEL).all()
    with _Stage(ra, s, vertices, indices, alloc) as st:
        _assert_frame(st.run(normal, capacity), want_cmds, r["draw_index_total"], np.concatenate([want_out, pad]), "normal, first")
        for rep in range(2):
            _assert_frame(st.run(make_frame(away_planes, away_cam, pv=pv), capacity), none, 0, untouched, ("no instance visible", rep))
        _assert_frame(st.run(normal, capacity), want_cmds, r["draw_index_total"], np.concatenate([want_out, pad]), "normal after an empty frame")
        for rep in range(2):
            _assert_frame(st.run(make_frame(s["planes"], s["cam_pos"], pv=pv_dead), capacity), none, rd["draw_index_total"], untouched, ("every triangle dies", rep))
        _assert_frame(st.run(normal, capacity), want_cmds, r["draw_index_total"], np.concatenate([want_out, pad]), "normal after a frame without survivors")
    with _Stage(ra, s, vertices, indices, alloc) as st:   # a context whose FIRST frames are the degenerate ones
        _assert_frame(st.run(make_frame(away_planes, away_cam, pv=pv), capacity), none, 0, untouched, "no instance visible, fresh context")
        _assert_frame(st.run(make_frame(s["planes"], s["cam_pos"], pv=pv_dead), capacity), none, rd["draw_index_total"], untouched, "every triangle dies, fresh context")
        _assert_frame(st.run(normal, capacity), want_cmds, r["draw_index_total"], np.concatenate([want_out, pad]), "normal after both")


@pytest.mark.parametrize("large_frame_path", [False, True])
def test_one_instance_of_one_triangle(ra, oracle_mod, monkeypatch, large_frame_path):
    """The smallest frame there is: one instance, one mesh of exactly one triangle — kept (front-facing), culled (two corners
    swapped), kept again; against the oracle and the restatement, which the known answers of tests/triangle_cases.py pin."""
    import triangle_cases as tc
    from renderer_amd.pipeline import make_frame

    if large_frame_path:
        monkeypatch.setenv("MIP_TUNE_TRI_BLOCK_MAX", "0")
    pv = ra.scene.default_pv()
    front = tc.tri(0, 1, 12)
    for corners, kept in ((front, True), (tc.swapped(front), False)):
        s, vertices, indices = _one_triangle_scene(ra, corners)
        r, want_cmds, want_out = _oracle_and_restatement(oracle_mod, s, vertices, indices, pv, 6)
        assert r["draw_count"] == 1 and len(want_cmds) == int(kept)
        assert want_out.tolist() == ([0, 1, 2] if kept else [SENTINEL] * 3) + [SENTINEL] * 3
        with _Stage(ra, s, vertices, indices, 64) as st:
            frame = make_frame(s["planes"], s["cam_pos"], pv=pv)
            for rep in range(2):
                _assert_frame(st.run(frame, 6), want_cmds, 3, want_out, (kept, rep))
            _assert_frame(st.run(frame, 3), want_cmds, 3, want_out[:3], (kept, "capacity exactly the frame's"))
