"""The batched-draws EXTENSION on the GPU (include/mi_instance_pipeline.h, mip_batch_draws): byte equality with the numpy
restatement (tests/batch_restatement.py) behind every kind of frame that writes a visibility bitmap, and batch_model against
the `model` of a mip_run of the same context. Not reference behaviour: parity is with the restatement."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import batch_restatement as br
from renderer_amd.pipeline import DRAW_CMD_DTYPE, MESH_DTYPE, make_frame, make_occlusion

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def ra():
    import renderer_amd

    renderer_amd.load_library()
    return renderer_amd


def _dev():
    import torch

    return torch.device("cuda", 0)


def _pipeline(ra, s, max_meshes=None, **kw):
    p = ra.InstancePipeline(max_instances=max(s["n"], 1), max_meshes=max_meshes or len(s["meshes"]), **kw)
    p.set_mesh_table(s["meshes"])
    p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
    return p


def _i32(v):
    return v - (1 << 32) if v >= 1 << 31 else v


class _Frame:
    """Device outputs of a frame: model, bitmap, commands, count."""

    def __init__(self, n, model=True):
        import torch

        nn = max(n, 1)
        self.n = n
        self.model = torch.zeros((nn, 16), dtype=torch.float32, device=_dev()) if model else None
        self.bitmap = torch.zeros(((nn + 31) // 32,), dtype=torch.int32, device=_dev())
        self.cmds = torch.zeros((nn, 5), dtype=torch.int32, device=_dev())
        self.scal = torch.zeros(8, dtype=torch.int32, device=_dev())
        torch.cuda.synchronize()

    def kwargs(self):
        return dict(model=self.model.data_ptr() if self.model is not None else 0, visible_bitmap=self.bitmap.data_ptr(),
                    draw_cmds=self.cmds.data_ptr(), draw_count=self.scal.data_ptr(), draw_index_total=self.scal.data_ptr() + 4)

    def host_bitmap(self):
        return self.bitmap[: (self.n + 31) // 32].cpu().numpy().view(np.uint32)


class _Batch:
    """Device outputs of mip_batch_draws, filled with a sentinel."""

    def __init__(self, n, n_meshes, model=True, count=True):
        import torch

        nn = max(n, 1)
        self.n = n
        self.cap = max(min(2 * n_meshes, nn), 1) + 3
        fill = _i32(SENTINEL)
        self.cmds = torch.full((self.cap, 5), fill, dtype=torch.int32, device=_dev())
        self.ids = torch.full((nn + 3,), fill, dtype=torch.int32, device=_dev())
        self.scal = torch.full((4,), fill, dtype=torch.int32, device=_dev())
        self.model = torch.full((nn + 3, 16), fill, dtype=torch.int32, device=_dev()) if model else None
        self.count = count
        torch.cuda.synchronize()

    def kwargs(self):
        return dict(batch_cmds=self.cmds.data_ptr(), batch_count=self.scal.data_ptr(), instance_ids=self.ids.data_ptr(),
                    instance_count=self.scal.data_ptr() + 4 if self.count else 0,
                    batch_model=self.model.data_ptr() if self.model is not None else 0)

    def result(self):
        import torch

        torch.cuda.synchronize()
        return dict(cmds=self.cmds.cpu().numpy().view(np.uint32), ids=self.ids.cpu().numpy().view(np.uint32),
                    scal=self.scal.cpu().numpy().view(np.uint32), count_wanted=self.count, model=None if self.model is None else self.model.cpu().numpy().view(np.uint32))


def _check(got, want, what, model_rows=None):
    """Byte equality with the restatement; nothing at or behind count / members is written."""
    count, members = want["count"], want["members"]
    assert int(got["scal"][0]) == count, (what, "batch_count", int(got["scal"][0]), count)
    assert int(got["scal"][1]) == (members if got["count_wanted"] else SENTINEL), (what, "instance_count", int(got["scal"][1]), members)
    assert (got["scal"][2:] == SENTINEL).all(), what
    assert got["cmds"][:count].tobytes() == want["cmds"].tobytes(), (what, "commands")
    assert (got["cmds"][count:] == SENTINEL).all(), (what, "commands behind batch_count were written")
    assert got["ids"][:members].tobytes() == want["ids"].tobytes(), (what, "instance_ids")
    assert (got["ids"][members:] == SENTINEL).all(), (what, "instance_ids behind members were written")
    if got["model"] is not None:
        assert (got["model"][members:] == SENTINEL).all(), (what, "batch_model behind members was written")
        if model_rows is not None:
            assert got["model"][:members].tobytes() == np.ascontiguousarray(model_rows).view(np.uint32).tobytes(), (what, "batch_model")


def _frame_then_batches(ra, p, s, what, base=0, check_list=True):
    """A mip_run and mip_batch_draws over its bitmap with NO wait in between; both against the restatement."""
    n = s["n"]
    f = _Frame(n)
    b = _Batch(n, len(s["meshes"]))
    frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=base)
    p.run_device(frame, async_=True, **f.kwargs())
    p.batch_draws(frame, f.bitmap.data_ptr(), async_=True, **b.kwargs())
    p.wait()
    got = b.result()
    model = f.model[:n].cpu().numpy()
    want = br.batch_draws(s["pos"], s["mesh_id"], s["meshes"], s["cam_pos"], f.host_bitmap(), first_instance_base=base, model=model)
    _check(got, want, what, model_rows=want["model"])
    if check_list:  # the members are exactly the firstInstance values of the frame's compacted list
        k = int(f.scal[0].item())
        lst = f.cmds[:k].cpu().numpy().view(np.uint32)
        assert k == want["members"], what
        assert np.array_equal(np.sort(want["ids"]), lst[:, 4]), what
    return got, want


# ---- 1. the BASELINE configurations at full size ----

@pytest.mark.parametrize("config", [1, 2, 3])
def test_baseline_configs_full_size(ra, config):
    s = ra.scene.make_scene(config)
    with _pipeline(ra, s) as p:
        got, want = _frame_then_batches(ra, p, s, f"config {config}")
        assert 0 < want["count"] <= 2 * len(s["meshes"]) and want["members"] > 0
        # ids only, no instance_count, no matrices: the same ids and commands
        f = _Frame(s["n"], model=False)
        b = _Batch(s["n"], len(s["meshes"]), model=False, count=False)
        frame = make_frame(s["planes"], s["cam_pos"])
        p.run_device(frame, async_=True, **f.kwargs())
        p.batch_draws(frame, f.bitmap.data_ptr(), **b.kwargs())
        _check(b.result(), want, f"config {config}, ids only")


# ---- 2. table sizes (one, two and three digits) and instance counts around the tiles ----

def _table_scene(ra, rng, n, m):
    s = ra.scene.make_scene(3, n=max(n, 1), all_visible=True)
    for k in ("pos", "rot", "scale", "mesh_id"):
        s[k] = s[k][:n].copy()
    s["n"] = n
    meshes = np.zeros(m, MESH_DTYPE)
    meshes["aabb_min"], meshes["aabb_max"] = -0.5, 0.5
    meshes["n_lods"] = rng.integers(1, 4, m)
    meshes["index_len"] = rng.integers(0, 3000, (m, 6)) // 3 * 3
    meshes["index_len"][rng.random((m, 6)) < 0.1] = 0
    meshes["index_offset"] = rng.integers(0, 2 ** 31, (m, 6))
    meshes["vertex_offset"] = rng.integers(-1000, 2 ** 30, m)
    s["meshes"] = meshes
    s["mesh_id"] = rng.integers(0, m, n).astype(np.uint32)
    if n and m > 2:
        s["mesh_id"][rng.integers(0, n, max(n // 8, 1))] = m - 1   # the last bucket is used
    return s


@pytest.mark.parametrize("m,sizes", [(1, (0, 1, 31, 33, 65, 255, 1025, 5000)), (64, (1, 63, 257, 1023, 1024, 4097, 70_001)),
                                     (128, (3000,)), (129, (3000,)), (300, (1, 100, 1500, 33_333)), (40_000, (1, 999, 20_001))])
def test_table_sizes_and_ragged_counts(ra, m, sizes):
    rng = np.random.default_rng(m)
    for n in sizes:
        s = _table_scene(ra, rng, n, m)
        with _pipeline(ra, s) as p:
            got, want = _frame_then_batches(ra, p, s, f"m={m} n={n}", base=int(rng.integers(0, 2 ** 32)))
            if n == 0:
                assert want["count"] == 0 and want["members"] == 0


def test_max_meshes_above_the_table(ra):
    rng = np.random.default_rng(5)
    s = _table_scene(ra, rng, 7000, 90)
    with _pipeline(ra, s, max_meshes=50_000) as p:
        _frame_then_batches(ra, p, s, "table of 90 in a context for 50 000")
        s2 = _table_scene(ra, rng, 7000, 20_000)   # then a three-digit table in the same context
        p.set_mesh_table(s2["meshes"])
        p.set_instances(s2["pos"], s2["rot"], s2["scale"], s2["mesh_id"])
        _frame_then_batches(ra, p, s2, "table of 20 000 in the same context")


# ---- 3. bitmaps of other frames ----

def _ndc_z(view_z):
    n_, f_ = 0.1, 100.0
    return np.float32(f_ / (f_ - n_) - f_ * n_ / ((f_ - n_) * view_z))


def test_bitmaps_of_occluded_frames_and_views(ra):
    import torch

    s = ra.scene.make_scene(3, n=150_000)
    n, m = s["n"], len(s["meshes"])
    w, h = 640, 360
    cleared = np.ones((h, w), np.float32)
    wall = cleared.copy()
    wall[:, : w // 2] = _ndc_z(25.0)   # one occluder: a wall over the left half of the screen, 25 units away
    pv = ra.scene.default_pv()
    with _pipeline(ra, s) as p:
        def pyramid(depth):
            dt = torch.from_numpy(depth).to(_dev())
            pyr = torch.zeros(ra.pipeline.depth_pyramid_layout(w, h)["bytes"] // 4, dtype=torch.float32, device=_dev())
            torch.cuda.synchronize()
            p.build_depth_pyramid(dt.data_ptr(), w, h, pyr.data_ptr(), format=ra._lib.MIP_DEPTH_FLOAT32)
            return pyr

        frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=77)
        bitmaps = {}
        for name, depth in (("cleared", cleared), ("wall", wall)):
            pyr = pyramid(depth)
            f = _Frame(n)
            o = p.prepare_outputs(async_=True, **f.kwargs())
            p.run_occluded(frame, make_occlusion(w, h, pyr.data_ptr(), pv), o)
            b = _Batch(n, m)
            p.batch_draws(frame, f.bitmap.data_ptr(), async_=True, **b.kwargs())   # behind the occluded frame, no wait
            p.wait()
            bitmaps[name] = f.host_bitmap().copy()
            model = f.model[:n].cpu().numpy()
            want = br.batch_draws(s["pos"], s["mesh_id"], s["meshes"], s["cam_pos"], bitmaps[name], first_instance_base=77, model=model)
            _check(b.result(), want, f"occluded frame, {name}", model_rows=want["model"])
            assert int(f.scal[0].item()) == want["members"]
        assert br.bitmap_bits(bitmaps["wall"], n).sum() < br.bitmap_bits(bitmaps["cleared"], n).sum()

        # the OR of two occlusion phases, made by the caller on its own stream: ordered by the caller
        pyr = pyramid(wall)
        rng = np.random.default_rng(8)
        last = torch.from_numpy(rng.integers(0, 1 << 32, (n + 31) // 32, dtype=np.uint64).astype(np.uint32).view(np.int32)).to(_dev())
        ph1, ph2 = _Frame(n), _Frame(n)
        p.run_occluded(frame, make_occlusion(w, h, pyr.data_ptr(), pv, candidates=last.data_ptr()), p.prepare_outputs(async_=False, **ph1.kwargs()))
        p.run_occluded(frame, make_occlusion(w, h, pyr.data_ptr(), pv, candidates=ph1.bitmap.data_ptr(), inverted=True),
                       p.prepare_outputs(async_=False, **ph2.kwargs()))
        both = torch.bitwise_or(ph1.bitmap, ph2.bitmap)
        torch.cuda.synchronize()
        b = _Batch(n, m)
        p.batch_draws(frame, both.data_ptr(), **b.kwargs())
        host = both[: (n + 31) // 32].cpu().numpy().view(np.uint32)
        want = br.batch_draws(s["pos"], s["mesh_id"], s["meshes"], s["cam_pos"], host, first_instance_base=77, model=ph1.model[:n].cpu().numpy())
        _check(b.result(), want, "OR of two phases", model_rows=want["model"])
        assert want["members"] == int(ph1.scal[0].item()) + int(ph2.scal[0].item())

        # a view's bitmap of mip_run_views, after mip_wait; the view's own reference point picks the LODs
        cams = [np.array([0.0, 1.0, 2.0], np.float32), np.array([30.0, 5.0, -20.0], np.float32)]
        views = [_Frame(n, model=False) for _ in cams]
        frames = [make_frame(s["planes"], c, first_instance_base=5 + v) for v, c in enumerate(cams)]
        p.run_views(frames, [p.prepare_outputs(async_=True, **v.kwargs()) for v in views])
        p.wait()
        for v, (view, cam) in enumerate(zip(views, cams)):
            b = _Batch(n, m, model=False)
            p.batch_draws(frames[v], view.bitmap.data_ptr(), **b.kwargs())
            want = br.batch_draws(s["pos"], s["mesh_id"], s["meshes"], cam, view.host_bitmap(), first_instance_base=5 + v)
            _check(b.result(), want, f"view {v}")
            assert want["members"] == int(view.scal[0].item())


# ---- 4. special values: batch_model is the frame's model, in both census states ----

def _special_values():
    return np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1e-38, 3.4e38, -3.4e38,
                     1e19, -1e19, 1e-20, 0.5, 2.0, 10.0, 100.0], dtype=np.float32)


def test_special_values_batch_model_is_the_frames_model(ra):
    import torch

    rng = np.random.default_rng(7)
    sv = _special_values()
    for poisoned in (False, True):
        s = ra.scene.make_scene(3, n=20_000, all_visible=True)
        n = s["n"]
        if poisoned:  # every wave gets a few poisoned lanes: the literal path (whole waves) and its finite lanes
            for col, width in (("pos", 3), ("rot", 4)):
                rows = rng.choice(n, 600, replace=False)
                s[col][rows, rng.integers(0, width, 600)] = rng.choice(sv, 600)
            s["scale"][rng.choice(n, 300, replace=False)] = rng.choice(sv, 300)
        else:         # finite, extreme: huge and denormal scales, products that underflow
            s["scale"][::3] = np.float32(1e-42)
            s["scale"][1::3] = np.float32(1e30)
            s["rot"][::5] *= np.float32(1e-20)
        with _pipeline(ra, s) as p:
            p.reset_timings()
            f = _Frame(n)
            frame = make_frame(s["planes"], s["cam_pos"])
            p.run_device(frame, async_=True, **f.kwargs())
            all_bits = torch.full(((n + 31) // 32,), -1, dtype=torch.int32, device=_dev())   # every instance, visible or not
            torch.cuda.synchronize()
            for bitmap in (f.bitmap, all_bits):
                b = _Batch(n, len(s["meshes"]))
                p.batch_draws(frame, bitmap.data_ptr(), **b.kwargs())
                host = bitmap[: (n + 31) // 32].cpu().numpy().view(np.uint32)
                want = br.batch_draws(s["pos"], s["mesh_id"], s["meshes"], s["cam_pos"], host)
                got = b.result()
                _check(got, want, f"special values, poisoned={poisoned}")
                frame_model = f.model[:n].cpu().numpy().view(np.uint32)
                assert got["model"][: want["members"]].tobytes() == frame_model[got["ids"][: want["members"]]].tobytes(), poisoned
            assert (p.timings()["general_launches"] > 0) == poisoned   # both census states are exercised


# ---- 5. frames in flight ----

def test_two_frames_in_flight_asynchronous(ra):
    s = ra.scene.make_scene(3, n=120_000)
    n, m = s["n"], len(s["meshes"])
    cams = [np.array([0.0, 1.0, 2.0], np.float32), np.array([4.0, 1.0, 30.0], np.float32), np.array([-9.0, 2.0, 11.0], np.float32),
            np.array([0.0, 1.0, 2.0], np.float32)]
    with _pipeline(ra, s, frames_in_flight=2) as p:
        frames = [_Frame(n) for _ in cams]
        batches = [_Batch(n, m) for _ in cams]
        for k, cam in enumerate(cams):   # frame k's batches are enqueued, then frame k+1 and its batches, nothing waits
            fr = make_frame(s["planes"], cam, first_instance_base=k * 1000)
            p.run_device(fr, async_=True, **frames[k].kwargs())
            p.batch_draws(fr, frames[k].bitmap.data_ptr(), async_=True, **batches[k].kwargs())
        p.wait()
        for k, cam in enumerate(cams):
            model = frames[k].model[:n].cpu().numpy()
            want = br.batch_draws(s["pos"], s["mesh_id"], s["meshes"], cam, frames[k].host_bitmap(), first_instance_base=k * 1000, model=model)
            _check(batches[k].result(), want, f"frame {k} in flight", model_rows=want["model"])


# ---- 6. updates move members between buckets ----

def test_updates_move_members_between_buckets(ra):
    s = ra.scene.make_scene(3, n=10_000, all_visible=True)
    with _pipeline(ra, s) as p:
        _, before = _frame_then_batches(ra, p, s, "before the update")
        # instance 17 crosses the LOD distance, instances 100 .. 199 change mesh
        far = np.linalg.norm(s["pos"][17].astype(np.float64) - s["cam_pos"]) > 10.0
        step = np.array([0.0, 0.0, 1.0], np.float32)
        s["pos"][17] = s["cam_pos"] + (step * np.float32(3.0) if far else step * np.float32(40.0))
        p.update_instances(17, pos_xyz=s["pos"][17:18])
        s["mesh_id"][100:200] = (s["mesh_id"][100:200] + 7) % len(s["meshes"])
        p.update_instances(100, mesh_id=s["mesh_id"][100:200])
        _, after = _frame_then_batches(ra, p, s, "after the update", check_list=False)
        assert before["ids"].tobytes() != after["ids"].tobytes()
        s2 = ra.scene.make_scene(3, n=10_000, all_visible=True)   # a re-upload
        s2["mesh_id"][:] = s2["mesh_id"][::-1].copy()
        p.set_instances(s2["pos"], s2["rot"], s2["scale"], s2["mesh_id"])
        _frame_then_batches(ra, p, s2, "after a re-upload")


# ---- 7. bad arguments with a live context ----

def test_bad_arguments_leave_the_context_usable(ra):
    L = ra._lib
    s = ra.scene.make_scene(1, n=2000)
    n = s["n"]
    with ra.InstancePipeline(max_instances=n, max_meshes=4) as p:
        lib, ctx = p._lib, p._ctx
        f, b = _Frame(n), _Batch(n, 1)
        frame = make_frame(s["planes"], s["cam_pos"])

        def outs(**kw):
            o = L.MipBatchOutputs()
            o.struct_size = C.sizeof(L.MipBatchOutputs)
            o.flags = L.MIP_OUT_DEVICE
            o.batch_cmds, o.batch_count, o.instance_ids = b.cmds.data_ptr(), b.scal.data_ptr(), b.ids.data_ptr()
            for k, v in kw.items():
                setattr(o, k, v)
            return o

        def call(fr, bm, o):
            return lib.mip_batch_draws(ctx, C.addressof(fr) if fr is not None else None, bm, C.addressof(o) if o is not None else None)

        assert call(frame, f.bitmap.data_ptr(), outs()) == -6 and lib.mip_last_error(ctx)          # nothing resident yet
        p.set_mesh_table(s["meshes"])
        assert call(frame, f.bitmap.data_ptr(), outs()) == -6                                       # a table, no instances
        p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
        assert lib.mip_batch_draws(None, C.addressof(frame), f.bitmap.data_ptr(), C.addressof(outs())) == -1
        bad = [call(None, f.bitmap.data_ptr(), outs()), call(frame, None, outs()), call(frame, f.bitmap.data_ptr(), None),
               call(frame, f.bitmap.data_ptr(), outs(batch_cmds=None)), call(frame, f.bitmap.data_ptr(), outs(batch_count=None)),
               call(frame, f.bitmap.data_ptr(), outs(instance_ids=None)), call(frame, f.bitmap.data_ptr(), outs(struct_size=40)),
               call(frame, f.bitmap.data_ptr(), outs(flags=0)), call(frame, f.bitmap.data_ptr(), outs(flags=L.MIP_OUT_ASYNC)),
               call(frame, f.bitmap.data_ptr(), outs(flags=L.MIP_OUT_DEVICE | L.MIP_OUT_WIRE)),
               call(frame, f.bitmap.data_ptr(), outs(flags=L.MIP_OUT_DEVICE | 0x100))]
        assert bad == [-1] * len(bad), bad
        assert lib.mip_last_error(ctx)
        assert (b.result()["scal"] == SENTINEL).all()   # none of them wrote anything
        _frame_then_batches(ra, p, s, "after the refused calls")


# ---- 8. any dispatch order (the diagnostic library, a child process) ----

_ORDER_CHILD = r'''
import os, sys
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
os.environ["MIP_LIBRARY"] = os.path.join(root, "renderer_amd", "lib", "libmi_instance_pipeline_dbg.so")
import numpy as np
import renderer_amd
import test_gpu_batch as T
rng = np.random.default_rng(11)
for n, m in ((200_000, 64), (50_000, 300)):
    s = T._table_scene(renderer_amd, rng, n, m) if m != 64 else renderer_amd.scene.make_scene(3, n=n)
    with T._pipeline(renderer_amd, s) as p:
        T._frame_then_batches(renderer_amd, p, s, f"{os.environ.get('MIP_DEBUG_TILE_ORDER')} n={n} m={m}", base=9)
print("ORDER-OK")
'''


@pytest.mark.parametrize("order", ["reverse", "scramble"])
def test_scrambled_dispatch_batched_draws(order):
    e = dict(os.environ, MIP_DEBUG_TILE_ORDER=order)
    out = subprocess.run([sys.executable, "-c", _ORDER_CHILD, ROOT], capture_output=True, text=True, timeout=600, env=e)
    assert out.returncode == 0 and "ORDER-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
