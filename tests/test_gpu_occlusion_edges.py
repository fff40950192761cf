"""The occlusion-edge catalogue (tests/occlusion_cases.py) through mip_build_depth_pyramid and mip_run_occluded, and the
depth pyramid at every shape where mip_depth_pyramid_kernel changes structure. The expectation is always the numpy
restatement (tests/occlusion_restatement.py) over the oracle's frame, bit for bit; every output is larger than the frame and
holds a sentinel behind it. No wrong kernel is ever run: that the scenes tell the likely mistakes apart is shown on the CPU
(tests/test_occlusion_cases.py). A mismatch names the edge class, the side and the instance."""
import os
import subprocess
import sys

import numpy as np
import pytest

import occlusion_cases as oc
import occlusion_restatement as occ
from helpers import run_oracle
from test_gpu_occlusion import _Outs, _check_against_restatement, _dev, _run_occluded

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5A5A5A5A
SLACK = 16
PYRAMID_SLACK = 64


@pytest.fixture(scope="module")
def ra():
    import renderer_amd

    renderer_amd.load_library()
    return renderer_amd


def _depth_tensor(depth, pitch_elems=None):
    import torch

    h, w = depth.shape
    pitch_elems = pitch_elems or w
    host = np.zeros((h, pitch_elems), depth.dtype)
    host[:, :w] = depth
    return torch.from_numpy(host.view(np.int16) if depth.dtype == np.uint16 else host).to(_dev())


def _pyramid_buffer(ra, w, h):
    import torch

    floats = ra.pipeline.depth_pyramid_layout(w, h)["bytes"] // 4
    assert floats * 4 == ra.load_library().mip_depth_pyramid_bytes(w, h)
    return torch.full((floats + PYRAMID_SLACK,), SENTINEL, dtype=torch.int32, device=_dev())


def _build(ra, p, depth, dt, pyr, pitch_elems=None, async_=False):
    h, w = depth.shape
    fmt = ra._lib.MIP_DEPTH_UNORM16 if depth.dtype == np.uint16 else ra._lib.MIP_DEPTH_FLOAT32
    p.build_depth_pyramid(dt.data_ptr(), w, h, pyr.data_ptr(), row_pitch_bytes=(pitch_elems or w) * depth.itemsize, format=fmt, async_=async_)


def _check_pyramid(pyr, want, what):
    got = pyr.cpu().numpy().view(np.uint32)
    floats = len(want)
    bad = np.nonzero(got[:floats] != want.view(np.uint32))[0]
    assert len(bad) == 0, (what, "texels (flat)", bad[:8].tolist())
    assert (got[floats:] == SENTINEL).all(), (what, "written behind mip_depth_pyramid_bytes")


# ---- the catalogue through the occluded frame ----

def _report(c, got_bits, want_bits, what):
    bad = np.nonzero(got_bits != want_bits)[0]
    assert len(bad) == 0, f"{c['name']} {what}: " + "; ".join(f"{oc.describe(c, i)} is {bool(got_bits[i])}, owed {bool(want_bits[i])}" for i in bad[:8])


def run_case(ra, oracle_mod, c, generals=(0, 1), setenv=None, repeats=1):
    """One catalogue scene: the pyramid bit for bit, then mip_run_occluded without candidates, with a random candidate bitmap
    in both polarities, and with nonzero bases, per value of MIP_TUNE_FORCE_GENERAL."""
    import torch

    from renderer_amd.pipeline import make_frame

    s = oc.scene_of(c)
    n, w, h = c["n"], c["width"], c["height"]
    levels = occ.pyramid_levels(c["depth"])
    bases = ((0, 0), (123_456, 0xFFFFFF00))
    wants = {b: run_oracle(oracle_mod, s, first_instance_base=b[0], first_index_base=b[1]) for b in bases}
    assert oc.verify(c, wants[bases[0]]["world_aabb"]) == []   # the labels hold for the boxes the kernel is owed
    rng = np.random.default_rng(len(c["labels"]))
    cand_np = rng.integers(0, 1 << 32, (n + 31) // 32, dtype=np.uint64).astype(np.uint32)
    labelled = np.array([l["index"] for l in c["labels"]], np.int64)
    cand_bits = occ.bits_of(cand_np, n)
    assert cand_bits[labelled].any() and not cand_bits[labelled].all()
    for general in generals:
        if setenv:
            setenv("MIP_TUNE_FORCE_GENERAL", str(general))
        with ra.InstancePipeline(max_instances=n, max_meshes=len(s["meshes"])) as p:
            p.set_mesh_table(s["meshes"])
            p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
            dt, pyr = _depth_tensor(c["depth"]), _pyramid_buffer(ra, w, h)
            torch.cuda.synchronize()
            _build(ra, p, c["depth"], dt, pyr)
            _check_pyramid(pyr, occ.pyramid_flat(levels), c["name"])
            cand = torch.from_numpy(cand_np.view(np.int32)).to(_dev())
            for candidates, inverted, base in ((None, False, bases[0]), (cand, False, bases[0]), (cand, True, bases[1]), (None, False, bases[1])):
                for _ in range(repeats):
                    what = f"general {general} candidates {candidates is not None} inverted {inverted} bases {base}"
                    outs = _Outs(ra, n + SLACK, tlas=False)
                    outs.n = n
                    for t in (outs.model, outs.bitmap, outs.occ, outs.cmds, outs.scal, outs.aabb):
                        t.view(torch.int32).fill_(SENTINEL)
                    torch.cuda.synchronize()
                    _run_occluded(ra, p, s, pyr, w, h, outs, candidates=candidates, inverted=inverted, pv=c["pv"],
                                  frame=make_frame(s["planes"], s["cam_pos"], first_instance_base=base[0], first_index_base=base[1]))
                    got = outs.result()
                    expect = occ.expected(wants[base], n, c["pv"], levels, w, h, candidates=None if candidates is None else cand_np,
                                          inverted=inverted, first_instance_base=base[0], first_index_base=base[1])
                    _report(c, occ.bits_of(got["occluded_bitmap"], n), expect["occluded"], what + ": occluded bit")
                    _report(c, occ.bits_of(got["visible_bitmap"], n), expect["visible"], what + ": visible bit")
                    _check_against_restatement(got, expect, f"{c['name']} {what}")
                    words = (n + 31) // 32
                    for name_, t, first in (("model", outs.model, n), ("world_aabb", outs.aabb, n), ("commands", outs.cmds, expect["draw_count"]),
                                            ("bitmap", outs.bitmap, words), ("occluded bitmap", outs.occ, words)):
                        assert bool((t.view(torch.int32)[first:] == SENTINEL).all().item()), (c["name"], what, f"{name_} behind the frame was written")
            _check_pyramid(pyr, occ.pyramid_flat(levels), c["name"] + " after the frames")


@pytest.mark.parametrize("name", oc.NAMES)
def test_occluded_frame_on_every_occlusion_edge(ra, oracle_mod, monkeypatch, name):
    run_case(ra, oracle_mod, oc.case(name), setenv=monkeypatch.setenv)


_CHILD = r"""
import os, sys
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
os.environ["MIP_LIBRARY"] = os.path.join(root, "renderer_amd", "lib", "libmi_instance_pipeline_dbg.so")
import oracle, renderer_amd
import occlusion_cases as oc
import test_gpu_occlusion_edges as T
oracle.build()
renderer_amd.load_library()
c = oc.case(sys.argv[2])
os.environ["MIP_DEBUG_TILE_ORDER"] = "scramble"
T.run_case(renderer_amd, oracle, c, generals=(0,), repeats=2)
for tile in range((c["n"] + oc.TILE - 1) // oc.TILE - 1):   # a tile that never publishes: its successors apply the predicate to it
    os.environ["MIP_DEBUG_SKIP_PUBLISH_TILE"] = str(tile)
    T.run_case(renderer_amd, oracle, c, generals=(0,))
print("DONE")
"""


@pytest.mark.parametrize("name", ["ortho64_f32_texel0", "perspective_big_f32"])
def test_scrambled_dispatch_on_the_occlusion_edges(name):
    """The diagnostic library: tiles in a scrambled order, then each tile in turn never publishing its aggregate, so that
    help_occluded_aggregate applies ITS copy of the predicate to every edge instance."""
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT, name], capture_output=True, text=True, timeout=300, env=dict(os.environ))
    assert out.returncode == 0 and "DONE" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]


# ---- the pyramid's shape edges ----

_depths = {}


def _random_depth(w, h, fmt):
    """test_pyramid_is_bit_exact's distributions: every u16 value; f32 in -1 .. 1.5 with NaN, -0 and subnormals."""
    key = (w, h, fmt)
    if key not in _depths:
        rng = np.random.default_rng(w * 7 + h)
        if fmt == "u16":
            depth = rng.integers(0, 65536, (h, w), dtype=np.uint16)
        else:
            depth = rng.uniform(-1.0, 1.5, (h, w)).astype(np.float32)
            depth[rng.random((h, w)) < 0.05] = np.nan
            depth[rng.random((h, w)) < 0.02] = -0.0
            depth[rng.random((h, w)) < 0.02] = 1e-42
        want = occ.pyramid_flat(occ.pyramid_levels(depth))
        depth.setflags(write=False)
        want.setflags(write=False)
        _depths[key] = (depth, want)
    return _depths[key]


@pytest.fixture(scope="module")
def small_pipeline(ra):
    s = ra.scene.make_scene(1, n=32)
    with ra.InstancePipeline(max_instances=32, max_meshes=len(s["meshes"])) as p:
        p.set_mesh_table(s["meshes"])
        p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
        yield p


@pytest.mark.parametrize("w,h,fmt,pitch", oc.pyramid_shapes())
def test_pyramid_at_every_shape_edge(ra, small_pipeline, w, h, fmt, pitch):
    import torch

    depth, want = _random_depth(w, h, fmt)
    dt, pyr = _depth_tensor(depth, pitch), _pyramid_buffer(ra, w, h)
    torch.cuda.synchronize()
    _build(ra, small_pipeline, depth, dt, pyr, pitch)
    _check_pyramid(pyr, want, (w, h, fmt, pitch, sorted(oc.pyramid_structure(w, h, fmt, pitch))))


@pytest.mark.parametrize("frames_in_flight", [1, 2])
def test_builds_back_to_back_on_one_context(ra, frames_in_flight):
    """A multi-block LDS-top shape, a memory-top shape, a one-block shape and the first again, enqueued without a wait in
    between: every build but the first relies on the last workgroup of the one before having reset the slot's counter. With
    two frames in flight an occluded frame behind every build moves the next build to the other slot."""
    import torch

    from renderer_amd.pipeline import make_frame

    shapes = [(200, 130, "f32"), (4097, 4096, "u16"), (40, 30, "u16"), (200, 130, "f32")]
    for w, h, f in shapes[:3]:
        classes = oc.pyramid_structure(w, h, f, w)
        assert ("top in LDS" in classes, "top through memory" in classes, "one block, early return" in classes).count(True) == 1
    s = ra.scene.make_scene(1, n=32)
    with ra.InstancePipeline(max_instances=32, max_meshes=len(s["meshes"]), frames_in_flight=frames_in_flight) as p:
        p.set_mesh_table(s["meshes"])
        p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
        jobs = []
        for w, h, f in shapes:
            depth, want = _random_depth(w, h, f)
            jobs.append((depth, want, _depth_tensor(depth), _pyramid_buffer(ra, w, h), _Outs(ra, s["n"]).asynchronous(ra)))
        torch.cuda.synchronize()
        for round_ in range(2):
            for depth, want, dt, pyr, outs in jobs:
                _build(ra, p, depth, dt, pyr, async_=True)
                if frames_in_flight > 1:
                    _run_occluded(ra, p, s, pyr, depth.shape[1], depth.shape[0], outs, frame=make_frame(s["planes"], s["cam_pos"]))
            p.wait()
            for k, (depth, want, dt, pyr, outs) in enumerate(jobs):
                _check_pyramid(pyr, want, (round_, k, depth.shape))
                pyr.fill_(SENTINEL)
            torch.cuda.synchronize()
