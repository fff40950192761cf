"""The frame kernel's narrow copy of the resident mesh ids (MipContext::d_frame_ids): 1 byte per instance while the context's
max_meshes is at most 256, 2 bytes up to 65 536, the u32 column above that (frame_plan.hpp, plan_frame_id_bytes). Every upload
path fills it; the stores-first order of the frame kernel and its helping path read it (the commands-first order stays on the
u32 column). The bytes of a frame are the test: every case is compared with the oracle on bitmap, count, command bytes, index
total, matrices and boxes (helpers.assert_parity).

These scenes are small, and a small launch takes the commands-first order by itself: MIP_TUNE_ORDER=1 (read when the context is
created) puts them through the stores-first order, the one large launches take; the tests run both.

Mesh tables repeat SEVEN different entries, so that entry k differs from entry k mod 256 and k mod 65 536: an id that lost its
upper bits, or that was read in the wrong width, draws another mesh. Scenes put every instance inside the frustum, so that every
id ends up in a command."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import assert_parity, run_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE, WAVE = 256, 64
WIDTH_EDGES = (1, 2, 255, 256, 257, 65535, 65536, 65537)     # table sizes around the 1-, 2- and 4-byte rules
COUNTS = (1, 63, 64, 65, 255, 256, 257, 513)                 # a wave, a tile, two tiles and one instance, and their neighbours


@pytest.fixture(scope="module")
def ra():
    import renderer_amd

    renderer_amd.load_library()
    return renderer_amd


def pinned_scene(ra, n, m, seed=0):
    """n instances inside the frustum over a table of m meshes; the first and last instance of every wave and tile (and of the
    scene) carry id 0 or m - 1, alternating, the others ids spread over the whole table."""
    s = ra.scene.make_scene(3, n=n, all_visible=True)
    s["meshes"] = np.resize(ra.scene.mixed_mesh_table(7), m)
    ids = ((np.arange(n, dtype=np.uint64) * 2654435761 + seed * 40503) % m).astype(np.uint32)
    edges = sorted({e for b in range(0, n, WAVE) for e in (b, b + WAVE - 1) if e < n} | {0, n - 1})
    for k, e in enumerate(edges):
        ids[e] = 0 if k % 2 == 0 else m - 1
    if n >= 2:
        ids[n - 1] = m - 1
    s["mesh_id"] = ids
    return s


def frame(p, s):
    return p.run_host(s["planes"], s["cam_pos"])


@pytest.fixture(params=("1", "3"))
def order(request, monkeypatch):
    """Both orders of the frame kernel: 1 = stores first (reads the narrow ids), 3 = commands first (reads the u32 column)."""
    monkeypatch.setenv("MIP_TUNE_ORDER", request.param)
    return request.param


@pytest.mark.gpu
@pytest.mark.parametrize("m", WIDTH_EDGES)
def test_table_sizes_at_the_width_edges(ra, oracle_mod, order, m):
    s = pinned_scene(ra, 513, m)
    want = run_oracle(oracle_mod, s)
    assert want["draw_count"] > 400   # the ids reach the commands
    with ra.InstancePipeline(max_instances=513, max_meshes=m) as p:
        p.set_mesh_table(s["meshes"])
        p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
        assert_parity(frame(p, s), want, f"m = {m}, order {order}")


@pytest.mark.gpu
@pytest.mark.parametrize("m", (200, 300, 65537))   # ids in 1, 2 and 4 bytes
@pytest.mark.parametrize("n", COUNTS)
def test_instance_counts_at_the_wave_and_tile_edges(ra, oracle_mod, order, n, m):
    s = pinned_scene(ra, n, m)
    want = run_oracle(oracle_mod, s)
    with ra.InstancePipeline(max_instances=n, max_meshes=m) as p:
        p.set_mesh_table(s["meshes"])
        p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
        assert_parity(frame(p, s), want, f"n = {n}, m = {m}, order {order}")


@pytest.mark.gpu
@pytest.mark.parametrize("max_meshes", (256, 65536))
def test_a_table_smaller_than_the_contexts_width(ra, oracle_mod, order, max_meshes):
    """The width follows max_meshes, not the table: 64 meshes in a context made for 256 / 65 536, then a LARGER table in the same
    context (ids up to max_meshes - 1), in both orders of the frame kernel."""
    with ra.InstancePipeline(max_instances=513, max_meshes=max_meshes) as p:
        for m in (64, max_meshes):
            s = pinned_scene(ra, 513, m)
            p.set_mesh_table(s["meshes"])
            p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
            assert_parity(frame(p, s), run_oracle(oracle_mod, s), f"m = {m} of {max_meshes}, order {order}")


@pytest.mark.gpu
def test_wide_ids_on_request(ra, oracle_mod, monkeypatch):
    """MIP_TUNE_WIDE_IDS (read when the context is created): the stores-first order on the u32 column too, through the same load."""
    monkeypatch.setenv("MIP_TUNE_WIDE_IDS", "1")
    monkeypatch.setenv("MIP_TUNE_ORDER", "1")
    s = pinned_scene(ra, 513, 64)
    with ra.InstancePipeline(max_instances=513, max_meshes=64) as p:
        p.set_mesh_table(s["meshes"])
        p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
        assert_parity(frame(p, s), run_oracle(oracle_mod, s), "u32 ids")


@pytest.mark.gpu
@pytest.mark.parametrize("m", (256, 300))
def test_update_over_an_odd_range_across_a_tile_boundary(ra, oracle_mod, order, m):
    """mip_update_instances over [first, first + count) with first and count odd, across the boundary of tiles 0 and 1 (odd byte
    offsets of a 1-byte column, odd halfword offsets of a 2-byte one): ids alone, then every column. The instances on either
    side of the range keep theirs."""
    s = pinned_scene(ra, 513, m)
    with ra.InstancePipeline(max_instances=513, max_meshes=m) as p:
        p.set_mesh_table(s["meshes"])
        p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
        assert_parity(frame(p, s), run_oracle(oracle_mod, s), "before the update")
        first, count = 251, 11
        new_ids = ((s["mesh_id"][first:first + count].astype(np.uint64) * 7 + 3) % m).astype(np.uint32)
        new_ids[0], new_ids[-1], new_ids[5] = m - 1, 0, m - 1      # 251: m - 1, 256 (a tile's first): m - 1, 261: 0
        assert not np.array_equal(new_ids, s["mesh_id"][first:first + count])
        p.update_instances(first, mesh_id=new_ids)
        s["mesh_id"][first:first + count] = new_ids
        assert_parity(frame(p, s), run_oracle(oracle_mod, s), "ids updated")
        first, count = 255, 3
        other = pinned_scene(ra, 513, m, seed=5)
        for col in ("pos", "rot", "scale", "mesh_id"):
            s[col][first:first + count] = other[col][300:300 + count]
        p.update_instances(first, s["pos"][first:first + count], s["rot"][first:first + count], s["scale"][first:first + count],
                           s["mesh_id"][first:first + count])
        assert_parity(frame(p, s), run_oracle(oracle_mod, s), "every column updated")


@pytest.mark.gpu
@pytest.mark.parametrize("m", (256, 300, 65537))
def test_device_upload_with_an_id_outside_the_table_is_refused(ra, oracle_mod, order, m):
    """mip_set_instances_device checks the ids on the device, in the kernel that narrows them: one id equal to m refuses the
    upload and leaves NO instances resident (a frame is refused too), a valid upload afterwards runs."""
    import torch

    dev = torch.device("cuda", 0)
    s = pinned_scene(ra, 513, m)
    cols = [torch.from_numpy(np.ascontiguousarray(s[c])).to(dev) for c in ("pos", "rot", "scale")]
    bad = s["mesh_id"].copy()
    bad[257] = m
    with ra.InstancePipeline(max_instances=513, max_meshes=m) as p:
        p.set_mesh_table(s["meshes"])
        p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
        ids = torch.from_numpy(bad.view(np.int32)).to(dev)
        torch.cuda.synchronize()
        with pytest.raises(ra.MipError) as refused:
            p.set_instances_device(cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), ids.data_ptr(), 513)
        assert "no instances are resident" in str(refused.value)
        with pytest.raises(ra.MipError):
            frame(p, s)
        ids = torch.from_numpy(s["mesh_id"].view(np.int32)).to(dev)
        torch.cuda.synchronize()
        p.set_instances_device(cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), ids.data_ptr(), 513)
        assert_parity(frame(p, s), run_oracle(oracle_mod, s), f"device upload, m = {m}")


@pytest.mark.gpu
@pytest.mark.parametrize("m", (200, 300))
def test_recorded_launches_before_and_after_an_update(ra, oracle_mod, order, m):
    """mip_run_many replays recorded launches, which bake the kernel's arguments (the id pointer and mode among them) into graph
    nodes: a frame through it, an update of the ids, a frame through it again — each the oracle's."""
    import torch

    from renderer_amd.pipeline import make_frame

    dev = torch.device("cuda", 0)
    n = 513
    s = pinned_scene(ra, n, m)
    with ra.InstancePipeline(max_instances=n, max_meshes=m) as p:
        p.set_mesh_table(s["meshes"])
        p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
        model = torch.zeros((n, 16), dtype=torch.float32, device=dev)
        aabb = torch.zeros((n, 6), dtype=torch.float32, device=dev)
        bitmap = torch.zeros(((n + 31) // 32,), dtype=torch.int32, device=dev)
        cmds = torch.zeros((n, 5), dtype=torch.int32, device=dev)
        scal = torch.zeros(8, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        out = p.prepare_outputs(model=model.data_ptr(), visible_bitmap=bitmap.data_ptr(), draw_cmds=cmds.data_ptr(),
                                draw_count=scal.data_ptr(), draw_index_total=scal.data_ptr() + 4, world_aabb=aabb.data_ptr())

        def replayed():
            p.run_many([make_frame(s["planes"], s["cam_pos"])], [out], 2)
            p.wait()
            count = int(scal[0].item())
            words = cmds[:count].cpu().numpy().view(np.uint32)
            return dict(model=model.cpu().numpy(), world_aabb=aabb.cpu().numpy(), visible_bitmap=bitmap.cpu().numpy().view(np.uint32),
                        draw_cmds=words, draw_count=count, draw_index_total=int(scal[1].item()) & 0xFFFFFFFF)

        assert_parity(replayed(), run_oracle(oracle_mod, s), "replay before the update")
        first, count = 253, 7
        s["mesh_id"][first:first + count] = (m - 1 - s["mesh_id"][first:first + count]).astype(np.uint32)
        p.update_instances(first, mesh_id=s["mesh_id"][first:first + count])
        assert_parity(replayed(), run_oracle(oracle_mod, s), "replay after the update")


_HELP_CHILD = r"""
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
os.environ["MIP_LIBRARY"] = os.path.join(sys.argv[1], "renderer_amd", "lib", "libmi_instance_pipeline_dbg.so")
os.environ["MIP_DEBUG_SKIP_PUBLISH_TILE"] = "1"     # tile 1 never publishes: tile 2 computes its aggregate from the inputs
import numpy as np
import oracle, renderer_amd
from helpers import assert_parity, run_oracle
from test_gpu_narrow_ids import pinned_scene
for m in (1, 200, 300, 65537):
    s = pinned_scene(renderer_amd, 769, m)
    want = run_oracle(oracle, s)
    for order in ("1", "3"):
        os.environ["MIP_TUNE_ORDER"] = order
        with renderer_amd.InstancePipeline(max_instances=769, max_meshes=m) as p:
            p.set_mesh_table(s["meshes"]); p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
            assert_parity(p.run_host(s["planes"], s["cam_pos"]), want, f"helped frame, m = {m}, order {order}")
            helps = p.timings()["prefix_helps"]
            assert helps > 0, (m, order, helps)
print("HELPED OK")
"""


@pytest.mark.gpu
def test_the_helping_path_reads_what_the_owner_reads():
    """Fault injection (the diagnostic build): a tile that never publishes is computed by its successor's wave 0, from the tile's
    inputs — the narrow ids among them, in the mode the owner reads them in (help_tile_aggregate). Tables of 1 (no id is read),
    200 (u8), 300 (u16) and 65 537 (u32) meshes, both orders; the help count says the path ran."""
    out = subprocess.run([sys.executable, "-c", _HELP_CHILD, ROOT], capture_output=True, text=True, timeout=300,
                         env={k: v for k, v in os.environ.items() if k != "MIP_TUNE_ORDER"})
    assert out.returncode == 0 and "HELPED OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
