"""The occlusion-culling EXTENSION on the GPU (include/mi_instance_pipeline.h, MipOcclusion): the depth pyramid bit-exact
against the numpy restatement, mip_run_occluded against mip_run (cleared depth, the per-triangle stage) and against the
restatement (occluder scenes, candidates, two phases, frames in flight, fault injection, random scenes). Not reference
behaviour: parity is with tests/occlusion_restatement.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import occlusion_restatement as occ
from helpers import run_oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ra():
    import renderer_amd

    renderer_amd.load_library()
    return renderer_amd


def _dev():
    import torch

    return torch.device("cuda", 0)


def _pipeline(ra, s, **kw):
    p = ra.InstancePipeline(max_instances=max(s["n"], 1), max_meshes=len(s["meshes"]), **kw)
    p.set_mesh_table(s["meshes"])
    p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
    return p


def _build_pyramid(ra, p, depth, pitch_elems=None, async_=False):
    """depth: H x W uint16 or float32 (host). Returns (pyramid tensor, depth tensor) on the device."""
    import torch

    h, w = depth.shape
    fmt = ra._lib.MIP_DEPTH_UNORM16 if depth.dtype == np.uint16 else ra._lib.MIP_DEPTH_FLOAT32
    pitch_elems = pitch_elems or w
    host = np.zeros((h, pitch_elems), depth.dtype)
    host[:, :w] = depth
    dt = torch.from_numpy(host.view(np.int16) if depth.dtype == np.uint16 else host).to(_dev())
    nbytes = ra.pipeline.depth_pyramid_layout(w, h)["bytes"]
    pyr = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=_dev())
    torch.cuda.synchronize()
    p.build_depth_pyramid(dt.data_ptr(), w, h, pyr.data_ptr(), row_pitch_bytes=pitch_elems * depth.itemsize, format=fmt, async_=async_)
    return pyr, dt


class _Outs:
    """Device outputs of one frame (every output of MipOutputs but the per-triangle stage's)."""

    def __init__(self, ra, n, tlas=True, occluded=True):
        import torch

        dev = _dev()
        nn = max(n, 1)
        self.model = torch.zeros((nn, 16), dtype=torch.float32, device=dev)
        self.bitmap = torch.zeros(((nn + 31) // 32,), dtype=torch.int32, device=dev)
        self.occ = torch.full(((nn + 31) // 32,), -1, dtype=torch.int32, device=dev) if occluded else None
        self.cmds = torch.zeros((nn, 5), dtype=torch.int32, device=dev)
        self.scal = torch.zeros(8, dtype=torch.int32, device=dev)
        self.aabb = torch.zeros((nn, 6), dtype=torch.float32, device=dev)
        self.tlas = torch.zeros((nn, 16), dtype=torch.int32, device=dev) if tlas else None
        self.n = n
        o = ra._lib.MipOutputs()
        o.flags = ra._lib.MIP_OUT_DEVICE
        o.model = self.model.data_ptr()
        o.visible_bitmap = self.bitmap.data_ptr()
        o.draw_cmds = self.cmds.data_ptr()
        o.draw_count = self.scal.data_ptr()
        o.draw_index_total = self.scal.data_ptr() + 4
        o.world_aabb = self.aabb.data_ptr()
        o.tlas_instances = self.tlas.data_ptr() if tlas else None
        self.out = o
        torch.cuda.synchronize()

    def asynchronous(self, ra):
        self.out.flags = ra._lib.MIP_OUT_DEVICE | ra._lib.MIP_OUT_ASYNC
        return self

    def result(self):
        import torch

        torch.cuda.synchronize()
        count = int(self.scal[0].item())
        words = (self.n + 31) // 32
        from renderer_amd.pipeline import DRAW_CMD_DTYPE

        r = {
            "model": self.model[: self.n].cpu().numpy(),
            "visible_bitmap": self.bitmap[:words].cpu().numpy().view(np.uint32),
            "draw_cmds": self.cmds[:count].cpu().numpy().view(DRAW_CMD_DTYPE).reshape(-1),
            "draw_count": count,
            "draw_index_total": int(self.scal[1].item()) & 0xFFFFFFFF,
            "world_aabb": self.aabb[: self.n].cpu().numpy(),
        }
        if self.tlas is not None:
            r["tlas"] = self.tlas[: self.n].cpu().numpy()
        if self.occ is not None:
            r["occluded_bitmap"] = self.occ[:words].cpu().numpy().view(np.uint32)
        return r


def _run_occluded(ra, p, s, pyr, w, h, outs, candidates=None, inverted=False, pv=None, frame=None):
    from renderer_amd.pipeline import make_frame, make_occlusion

    pv = ra.scene.default_pv() if pv is None else pv
    frame = frame or make_frame(s["planes"], s["cam_pos"])
    o = make_occlusion(w, h, pyr.data_ptr(), pv, candidates=candidates.data_ptr() if candidates is not None else 0,
                       occluded_bitmap=outs.occ.data_ptr() if outs.occ is not None else 0, inverted=inverted)
    p.run_occluded(frame, o, outs.out)
    return o


def _check_against_restatement(got, want, what):
    assert np.array_equal(got["occluded_bitmap"], want["occluded_bitmap"]), f"{what}: occluded bitmap"
    assert np.array_equal(got["visible_bitmap"], want["visible_bitmap"]), f"{what}: visibility bitmap"
    assert got["draw_count"] == want["draw_count"], f"{what}: draw_count {got['draw_count']} vs {want['draw_count']}"
    assert got["draw_cmds"].tobytes() == want["draw_cmds"].tobytes(), f"{what}: command bytes"
    assert got["draw_index_total"] == want["draw_index_total"], f"{what}: index total"


def _ndc_z(view_z):
    """ndc depth of a point at view distance view_z in the default camera (near 0.1, far 100), float32."""
    n_, f_ = 0.1, 100.0
    return np.float32(f_ / (f_ - n_) - f_ * n_ / ((f_ - n_) * view_z))


def _block_depth(rng, w, h, block, lo=8.0, hi=40.0, cleared=0.05, u16=False):
    """Random block depths (view distances lo .. hi), some blocks cleared."""
    bw, bh = (w + block - 1) // block, (h + block - 1) // block
    z = np.vectorize(_ndc_z)(rng.uniform(lo, hi, (bh, bw))).astype(np.float32)
    z[rng.random(z.shape) < cleared] = 1.0
    d = np.repeat(np.repeat(z, block, 0), block, 1)[:h, :w]
    return np.round(d.astype(np.float64) * 65535).astype(np.uint16) if u16 else d.astype(np.float32)


# ---- 1. the pyramid ----

_PYRAMID_CASES = [(w, h, f) for w, h in [(1, 1), (1, 2), (3, 1), (7, 5), (1920, 1080), (4097, 3)] for f in ("u16", "f32")]
_PYRAMID_CASES += [(16384, 16384, "u16"), (16384, 70, "f32"), (5000, 4099, "f32")]  # (above 4096 a side: levels 6.. through memory)


@pytest.mark.parametrize("w,h,fmt", _PYRAMID_CASES)
def test_pyramid_is_bit_exact(ra, w, h, fmt):
    rng = np.random.default_rng(w * 7 + h)
    s = ra.scene.make_scene(1, n=32)
    if fmt == "u16":
        depth = rng.integers(0, 65536, (h, w), dtype=np.uint16)
    else:
        depth = rng.uniform(-1.0, 1.5, (h, w)).astype(np.float32)
        depth[rng.random((h, w)) < 0.05] = np.nan
        depth[rng.random((h, w)) < 0.02] = -0.0
        depth[rng.random((h, w)) < 0.02] = 1e-42  # subnormals survive
    want = occ.pyramid_flat(occ.pyramid_levels(depth))
    with _pipeline(ra, s) as p:
        pyr, _ = _build_pyramid(ra, p, depth)
        got = pyr.cpu().numpy()
        assert got.view(np.uint32).tobytes() == want.view(np.uint32).tobytes(), np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0][:8]
        if w * h <= 1 << 22:  # a padded pitch (not a multiple of 16 bytes: no 16-byte loads) and an aligned one gives the same
            for pad in (3, 8):
                pyr2, _ = _build_pyramid(ra, p, depth, pitch_elems=w + pad)
                assert pyr2.cpu().numpy().view(np.uint32).tobytes() == want.view(np.uint32).tobytes(), pad


# ---- 2. cleared depth: exactly mip_run ----

@pytest.mark.parametrize("config", [1, 2, 3])
def test_cleared_depth_is_mip_run(ra, config):
    import ctypes as C

    from renderer_amd.pipeline import make_frame

    s = ra.scene.make_scene(config)
    n = s["n"]
    with _pipeline(ra, s) as p:
        p.set_blas_addresses(np.arange(len(s["meshes"]), dtype=np.uint64) * 4096 + 0x10000)
        ref = _Outs(ra, n, occluded=False)
        frame = make_frame(s["planes"], s["cam_pos"])
        p._check(p._lib.mip_run(p._ctx, C.addressof(frame), C.addressof(ref.out)))
        want = ref.result()
        for depth in (np.full((1080, 1920), 65535, np.uint16), np.ones((37, 53), np.float32)):
            pyr, _ = _build_pyramid(ra, p, depth)
            got_o = _Outs(ra, n)
            _run_occluded(ra, p, s, pyr, depth.shape[1], depth.shape[0], got_o)
            got = got_o.result()
            for k in ("model", "visible_bitmap", "draw_cmds", "world_aabb", "tlas"):
                assert got[k].tobytes() == want[k].tobytes(), (config, k)
            assert got["draw_count"] == want["draw_count"] and got["draw_index_total"] == want["draw_index_total"]
            assert not got["occluded_bitmap"].any()


# ---- 3. occluder scenes against the restatement ----

def test_occluder_scenes(ra, oracle_mod):
    s = ra.scene.make_scene(3, n=300_000)
    n = s["n"]
    pv = ra.scene.default_pv()
    want0 = run_oracle(oracle_mod, s, threads=8)
    rng = np.random.default_rng(3)
    w, h = 1920, 1080
    wall = np.full((h, w), 1.0, np.float32)
    wall[:, : w // 2] = _ndc_z(25.0)  # a wall over the left half of the screen, 25 units away
    images = {"wall": wall, "blocks_f32": _block_depth(rng, w, h, 64), "blocks_u16": _block_depth(rng, w, h, 96, u16=True)}
    with _pipeline(ra, s) as p:
        for name, depth in images.items():
            pyr, _ = _build_pyramid(ra, p, depth)
            levels = occ.pyramid_levels(depth)
            outs = _Outs(ra, n)
            _run_occluded(ra, p, s, pyr, w, h, outs)
            got = outs.result()
            want = occ.expected(want0, n, pv, levels, w, h)
            _check_against_restatement(got, want, name)
            vis = int(want["in_frustum"].sum())
            frac = float(want["occluded"].sum()) / vis
            assert 0.1 <= frac <= 0.9, (name, frac)


# ---- 4. candidates and two phases ----

def test_candidates_and_two_phases(ra, oracle_mod):
    import torch

    s = ra.scene.make_scene(3, n=200_000)
    n = s["n"]
    pv = ra.scene.default_pv()
    want0 = run_oracle(oracle_mod, s, threads=8)
    rng = np.random.default_rng(4)
    w, h = 1280, 720
    old, new = _block_depth(rng, w, h, 32), _block_depth(rng, w, h, 20, u16=True)
    old_levels, new_levels = occ.pyramid_levels(old), occ.pyramid_levels(new)
    last_visible = rng.integers(0, 1 << 32, (n + 31) // 32, dtype=np.uint64).astype(np.uint32)
    with _pipeline(ra, s) as p:
        cand = torch.from_numpy(last_visible.view(np.int32)).to(_dev())
        old_pyr, _ = _build_pyramid(ra, p, old)
        for inverted in (False, True):
            outs = _Outs(ra, n)
            _run_occluded(ra, p, s, old_pyr, w, h, outs, candidates=cand, inverted=inverted)
            _check_against_restatement(outs.result(), occ.expected(want0, n, pv, old_levels, w, h, candidates=last_visible, inverted=inverted),
                                       f"candidates inverted={inverted}")
        # a two-phase frame: phase 1 against last frame's visible set and pyramid, phase 2 against the new pyramid for the rest
        ph1 = _Outs(ra, n)
        _run_occluded(ra, p, s, old_pyr, w, h, ph1, candidates=cand)
        new_pyr, _ = _build_pyramid(ra, p, new)
        ph2 = _Outs(ra, n)
        _run_occluded(ra, p, s, new_pyr, w, h, ph2, candidates=ph1.bitmap, inverted=True)
        g1, g2 = ph1.result(), ph2.result()
        w1 = occ.expected(want0, n, pv, old_levels, w, h, candidates=last_visible)
        w2 = occ.expected(want0, n, pv, new_levels, w, h, candidates=w1["visible_bitmap"], inverted=True)
        _check_against_restatement(g1, w1, "phase 1")
        _check_against_restatement(g2, w2, "phase 2")
        # the phases partition what the frame draws: no instance twice, and together every frustum-visible one not occluded by
        # the pyramid it was tested against
        assert not (w1["visible"] & w2["visible"]).any()
        assert ((w1["visible"] | w2["visible"]) <= w1["in_frustum"]).all()
        assert g1["draw_count"] > 0 and g2["draw_count"] > 0


# ---- 5. the per-triangle stage behind it ----

def test_per_triangle_stage_over_the_occluded_list(ra, oracle_mod):
    import torch

    from renderer_amd.pipeline import make_frame

    s = ra.scene.make_scene(3, n=20_000)
    n = s["n"]
    vertices, indices = ra.scene.make_geometry(s["meshes"])
    pv = ra.scene.default_pv()
    want0 = run_oracle(oracle_mod, s, threads=8)
    w, h = 640, 360
    depth = _block_depth(np.random.default_rng(5), w, h, 16)
    occluded = occ.expected(want0, n, pv, occ.pyramid_levels(depth), w, h)["occluded"]
    assert occluded.sum() > 100
    capacity = want0["draw_index_total"] + 3
    dev = _dev()

    def stage(p, run):
        model = torch.zeros((n, 16), dtype=torch.float32, device=dev)
        cmds = torch.zeros((n, 5), dtype=torch.int32, device=dev)
        scal = torch.zeros(8, dtype=torch.int32, device=dev)
        tri = torch.full((capacity,), -1, dtype=torch.int32, device=dev)
        o = ra._lib.MipOutputs()
        o.flags = ra._lib.MIP_OUT_DEVICE
        o.model, o.draw_cmds, o.draw_count, o.draw_index_total = model.data_ptr(), cmds.data_ptr(), scal.data_ptr(), scal.data_ptr() + 4
        o.culled_index_buffer, o.culled_index_capacity = tri.data_ptr(), capacity
        torch.cuda.synchronize()
        run(o)
        torch.cuda.synchronize()
        count = int(scal[0].item())
        return cmds[:count].cpu().numpy().tobytes(), tri.cpu().numpy().tobytes(), count

    frame = make_frame(s["planes"], s["cam_pos"], pv=pv)
    with _pipeline(ra, s) as p:
        p.set_geometry(vertices, indices)
        pyr, _ = _build_pyramid(ra, p, depth)
        from renderer_amd.pipeline import make_occlusion

        o_occ = make_occlusion(w, h, pyr.data_ptr(), pv)
        got = stage(p, lambda o: p.run_occluded(frame, o_occ, o))
        # the same frame by mip_run, the occluded instances moved out of the frustum (behind the camera)
        pos = s["pos"].copy()
        pos[occluded] = (0.0, 1.0, -500.0)
        p.update_instances(0, pos_xyz=pos)
        import ctypes as C

        want = stage(p, lambda o: p._check(p._lib.mip_run(p._ctx, C.addressof(frame), C.addressof(o))))
    assert got[2] == want[2] and got[2] > 0
    assert got[0] == want[0], "commands"
    assert got[1] == want[1], "culled index stream"


# ---- 6. frames in flight ----

def test_frames_in_flight_asynchronous(ra, oracle_mod):
    import torch

    s = ra.scene.make_scene(3, n=300_000)
    n = s["n"]
    pv = ra.scene.default_pv()
    want0 = run_oracle(oracle_mod, s, threads=8)
    rng = np.random.default_rng(6)
    w, h = 1920, 1080
    depths = [_block_depth(rng, w, h, 24, u16=True), _block_depth(rng, w, h, 48)]
    with _pipeline(ra, s, frames_in_flight=2) as p:
        nbytes = ra.pipeline.depth_pyramid_layout(w, h)["bytes"]
        dts = [torch.from_numpy(d.view(np.int16) if d.dtype == np.uint16 else d).to(_dev()) for d in depths]
        pyrs = [torch.zeros(nbytes // 4, dtype=torch.float32, device=_dev()) for _ in range(4)]
        outs = [_Outs(ra, n).asynchronous(ra) for _ in range(4)]
        torch.cuda.synchronize()
        for k in range(4):  # build + run on rotating slots, nothing waited for in between
            d = depths[k % 2]
            fmt = ra._lib.MIP_DEPTH_UNORM16 if d.dtype == np.uint16 else ra._lib.MIP_DEPTH_FLOAT32
            p.build_depth_pyramid(dts[k % 2].data_ptr(), w, h, pyrs[k].data_ptr(), format=fmt, async_=True)
            _run_occluded(ra, p, s, pyrs[k], w, h, outs[k])
        p.wait()
        for k, o in enumerate(outs):
            want = occ.expected(want0, n, pv, occ.pyramid_levels(depths[k % 2]), w, h)
            _check_against_restatement(o.result(), want, f"frame {k}")


# ---- 7. fault injection: any dispatch order, a tile that never publishes ----

_ORDER_CHILD = r"""
import os, sys
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
os.environ["MIP_LIBRARY"] = os.path.join(root, "renderer_amd", "lib", "libmi_instance_pipeline_dbg.so")
import numpy as np
import oracle, renderer_amd
import occlusion_restatement as occ
import test_gpu_occlusion as T
s = renderer_amd.scene.make_scene(3, n=1_000_000)
want0 = oracle.run(s["pos"], s["rot"], s["scale"], s["mesh_id"], s["meshes"], s["planes"], s["cam_pos"], threads=8)
w, h = 1920, 1080
depth = T._block_depth(np.random.default_rng(7), w, h, 32)
want = occ.expected(want0, s["n"], renderer_amd.scene.default_pv(), occ.pyramid_levels(depth), w, h)
with T._pipeline(renderer_amd, s) as p:
    pyr, _ = T._build_pyramid(renderer_amd, p, depth)
    for k in range(2):
        outs = T._Outs(renderer_amd, s["n"])
        T._run_occluded(renderer_amd, p, s, pyr, w, h, outs)
        T._check_against_restatement(outs.result(), want, "frame %d" % k)
    print("HELPS", p.timings()["prefix_helps"])
"""


@pytest.mark.parametrize("env", [{"MIP_DEBUG_TILE_ORDER": "reverse"}, {"MIP_DEBUG_TILE_ORDER": "scramble"}, {"MIP_DEBUG_SKIP_PUBLISH_TILE": "5"}])
def test_scrambled_dispatch_occluded_frames(env):
    e = dict(os.environ, **env)
    out = subprocess.run([sys.executable, "-c", _ORDER_CHILD, ROOT], capture_output=True, text=True, timeout=600, env=e)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    line = [l for l in out.stdout.split("\n") if l.startswith("HELPS")]
    assert line, out.stdout
    helps = int(line[0].split()[1])
    assert helps > 0, env  # the predecessors' aggregates were computed by the help path, with the occlusion predicate


# ---- 8. random scenes ----

def test_gpu_vs_oracle_random_scenes_occluded(ra, oracle_mod):
    import torch

    from renderer_amd.pipeline import make_frame

    rng = np.random.default_rng(8)
    for case in range(50):
        n = int(rng.integers(1, 30_000))
        s = ra.scene.make_scene(3, n=n, first=int(rng.integers(0, 1_000_000)))
        cam = np.array([rng.uniform(-10, 10), rng.uniform(-2, 4), rng.uniform(-10, 5)], np.float32)
        planes = oracle_mod.project_camera(cam, (0.0, 0.0, 0.0, 1.0))
        pv = oracle_mod.camera_pv(cam, (0.0, 0.0, 0.0, 1.0))
        s = dict(s, planes=planes, cam_pos=cam)
        base, ibase = int(rng.integers(0, 1 << 20)), int(rng.integers(0, 1 << 32))
        want0 = run_oracle(oracle_mod, s, threads=8, first_instance_base=base, first_index_base=ibase)
        w, h = int(rng.integers(1, 700)), int(rng.integers(1, 500))
        depth = _block_depth(rng, w, h, int(rng.integers(1, 64)), lo=2.0, hi=40.0, u16=bool(rng.integers(0, 2)))
        if depth.dtype == np.float32 and rng.random() < 0.3:
            depth[rng.random(depth.shape) < 0.05] = np.nan
        use_cand = rng.random() < 0.5
        cand_np = rng.integers(0, 1 << 32, (n + 31) // 32, dtype=np.uint64).astype(np.uint32) if use_cand else None
        inverted = use_cand and bool(rng.integers(0, 2))
        with _pipeline(ra, s) as p:
            pyr, _ = _build_pyramid(ra, p, depth)
            cand = torch.from_numpy(cand_np.view(np.int32)).to(_dev()) if use_cand else None
            outs = _Outs(ra, n)
            _run_occluded(ra, p, s, pyr, w, h, outs, candidates=cand, inverted=inverted, pv=pv,
                          frame=make_frame(planes, cam, first_instance_base=base, first_index_base=ibase))
            got = outs.result()
        want = occ.expected(want0, n, pv, occ.pyramid_levels(depth), w, h, candidates=cand_np, inverted=inverted,
                            first_instance_base=base, first_index_base=ibase)
        _check_against_restatement(got, want, f"case {case} (n {n}, {w}x{h}, candidates {use_cand}, inverted {inverted})")


# ---- bad arguments with a live context ----

def test_bad_arguments_with_a_context(ra):
    import ctypes as C

    import torch

    from renderer_amd.pipeline import make_frame, make_occlusion

    s = ra.scene.make_scene(1, n=100)
    lib = ra.load_library()
    with _pipeline(ra, s) as p:
        pyr = torch.zeros(64, dtype=torch.float32, device=_dev())
        frame = make_frame(s["planes"], s["cam_pos"])
        outs = _Outs(ra, s["n"])

        def rc(**kw):
            o = make_occlusion(8, 8, pyr.data_ptr(), ra.scene.default_pv(), occluded_bitmap=outs.occ.data_ptr())
            out = outs.out
            for k, v in kw.items():
                if k == "out_flags":
                    out = ra._lib.MipOutputs.from_buffer_copy(outs.out)
                    out.flags = v
                else:
                    setattr(o, k, v)
            return lib.mip_run_occluded(p._ctx, C.addressof(frame), C.addressof(o), C.addressof(out))

        assert rc() == 0
        assert rc(struct_size=100) == -1
        assert rc(width=0) == -1 and rc(height=16385) == -1
        assert rc(flags=2) == -1
        assert rc(flags=ra._lib.MIP_OCC_CANDIDATES_INVERTED) == -1  # INVERTED without a candidate bitmap
        assert rc(pyramid=None) == -1
        assert rc(out_flags=ra._lib.MIP_OUT_HOST) == -1  # a device bitmap with host outputs
        assert rc(out_flags=ra._lib.MIP_OUT_DEVICE | ra._lib.MIP_OUT_WIRE) == -1
        assert lib.mip_run_occluded(p._ctx, None, None, None) == -1
        assert lib.mip_build_depth_pyramid(p._ctx, pyr.data_ptr(), 8, 8, 16, 7, pyr.data_ptr(), 0) == -1  # format
        assert lib.mip_build_depth_pyramid(p._ctx, pyr.data_ptr(), 8, 8, 15, 0, pyr.data_ptr(), 0) == -1  # pitch
        assert lib.mip_build_depth_pyramid(p._ctx, pyr.data_ptr(), 0, 8, 16, 0, pyr.data_ptr(), 0) == -1
        assert lib.mip_build_depth_pyramid(p._ctx, None, 8, 8, 16, 0, pyr.data_ptr(), 0) == -1
        # still usable afterwards
        assert rc() == 0
