"""The occlusion-culling extension without a GPU: the three entry points are exported, the pyramid size is the Python
mirror's, the public struct has its documented layout, bad arguments are status codes, and the numpy restatement
(tests/occlusion_restatement.py) decides like a float64 computation wherever the float32 rounding cannot matter."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import occlusion_restatement as occ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (1, 2), (3, 1), (7, 5), (1920, 1080), (4097, 3), (16384, 16384)]


def test_library_exports_the_occlusion_entry_points():
    import renderer_amd
    from renderer_amd import _lib

    lib = renderer_amd.load_library()
    for name in ("mip_depth_pyramid_bytes", "mip_build_depth_pyramid", "mip_run_occluded"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS


def test_pyramid_bytes_follow_the_layout():
    import renderer_amd
    from renderer_amd.pipeline import depth_pyramid_layout

    lib = renderer_amd.load_library()
    for w, h in SIZES:
        lay = depth_pyramid_layout(w, h)
        assert lib.mip_depth_pyramid_bytes(w, h) == lay["bytes"] > 0, (w, h)
        # level 0 is ceil(W/2) x ceil(H/2), each next one ceil of half the last, down to 1 x 1, stored one after another
        assert lay["sizes"][0] == ((w + 1) // 2, (h + 1) // 2) and lay["sizes"][-1] == (1, 1)
        for (a, b), (c, d) in zip(lay["sizes"], lay["sizes"][1:]):
            assert (c, d) == ((a + 1) // 2, (b + 1) // 2)
        assert lay["offsets"] == list(np.cumsum([0] + [a * b for a, b in lay["sizes"]])[:-1])
        if w * h <= 1 << 22:  # the restatement's levels have the same shapes
            levels = occ.pyramid_levels(np.zeros((h, w), np.uint16))
            assert [l.shape[::-1] for l in levels] == lay["sizes"]
    assert depth_pyramid_layout(1920, 1080)["sizes"][:3] == [(960, 540), (480, 270), (240, 135)]
    for w, h in [(0, 1), (1, 0), (0, 0), (16385, 1), (1, 16385), (16385, 16385)]:
        assert lib.mip_depth_pyramid_bytes(w, h) == 0 and depth_pyramid_layout(w, h)["bytes"] == 0, (w, h)


def test_occlusion_struct_layout():
    from renderer_amd import _lib

    assert C.sizeof(_lib.MipOcclusion) == 104
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "mi_instance_pipeline.h"
    int main(void) {
      printf("%zu %zu %zu %zu %u %u %u\n", sizeof(MipOcclusion), offsetof(MipOcclusion, pyramid), offsetof(MipOcclusion, occluded_bitmap),
             offsetof(MipOcclusion, pv), MIP_DEPTH_UNORM16, MIP_DEPTH_FLOAT32, MIP_MAX_DEPTH_EXTENT);
      return 0;
    }'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [104, 16, 32, 40, 0, 1, 16384]
    assert _lib.MipOcclusion.pv.offset == 40 and _lib.MipOcclusion.pyramid.offset == 16


def test_bad_arguments_are_status_codes():
    import renderer_amd
    from renderer_amd import _lib
    from renderer_amd.pipeline import make_frame, make_occlusion

    lib = renderer_amd.load_library()
    frame = make_frame(np.zeros(24, np.float32), np.zeros(3, np.float32))
    o = make_occlusion(64, 64, 0x1000, np.eye(4, dtype=np.float32))
    out = _lib.MipOutputs()
    assert lib.mip_run_occluded(None, C.addressof(frame), C.addressof(o), C.addressof(out)) == -1
    assert lib.mip_run_occluded(None, None, None, None) == -1
    o.struct_size = 96
    assert lib.mip_run_occluded(None, C.addressof(frame), C.addressof(o), C.addressof(out)) == -1
    assert lib.mip_build_depth_pyramid(None, None, 64, 64, 128, 0, None, 0) == -1
    assert lib.mip_build_depth_pyramid(None, 0x1000, 64, 64, 128, 0, 0x2000, 0) == -1


def _float64_decision(boxes, pv, levels, width, height):
    """The same test in float64 (the pyramid's texels as they are), with how far each decision is from flipping."""
    m = np.asarray(pv, np.float64).reshape(4, 4, order="F")  # column-major storage
    n = len(boxes)
    corners = np.empty((n, 8, 4))
    for c in range(8):
        corners[:, c, 0] = boxes[:, 3] if c & 1 else boxes[:, 0]
        corners[:, c, 1] = boxes[:, 4] if c & 2 else boxes[:, 1]
        corners[:, c, 2] = boxes[:, 5] if c & 4 else boxes[:, 2]
        corners[:, c, 3] = 1.0
    clip = corners @ m.T
    w = clip[..., 3]
    ndc = clip[..., :3] / w[..., None]
    u = (ndc[..., 0] * 0.5 + 0.5) * width
    v = (0.5 - ndc[..., 1] * 0.5) * height
    margin = np.min(np.abs(w), axis=1)
    ext = [u.min(1), u.max(1), v.min(1), v.max(1)]
    for e in ext:  # distance of each rectangle edge from the next pixel boundary
        margin = np.minimum(margin, np.abs(e - np.round(e)))
    x0, x1 = np.clip(np.floor(ext[0]), 0, width - 1).astype(int), np.clip(np.floor(ext[1]), 0, width - 1).astype(int)
    y0, y1 = np.clip(np.floor(ext[2]), 0, height - 1).astype(int), np.clip(np.floor(ext[3]), 0, height - 1).astype(int)
    zmin = ndc[..., 2].min(1)
    decision = np.zeros(n, bool)
    for i in range(n):
        k = 0
        while (x1[i] >> (k + 1)) - (x0[i] >> (k + 1)) > 1 or (y1[i] >> (k + 1)) - (y0[i] >> (k + 1)) > 1:
            k += 1
        t = levels[k].astype(np.float64)
        s = k + 1
        d = max(t[y0[i] >> s, x0[i] >> s], t[y0[i] >> s, x1[i] >> s], t[y1[i] >> s, x0[i] >> s], t[y1[i] >> s, x1[i] >> s])
        decision[i] = bool((w[i] > 0).all()) and d < 1.0 and zmin[i] > d
        margin[i] = min(margin[i], abs(zmin[i] - d))
    return decision, margin


def test_restatement_decides_like_float64_away_from_the_edges():
    from renderer_amd import scene

    rng = np.random.default_rng(11)
    pv = scene.default_pv()
    width, height = 96, 64
    n = 4000
    centre = np.stack([rng.uniform(-20, 20, n), rng.uniform(-10, 12, n), rng.uniform(3, 60, n)], 1)
    half = rng.uniform(0.05, 3.0, (n, 3))
    boxes = np.concatenate([centre - half, centre + half], 1).astype(np.float32)
    # depths in the range the boxes project to, blocky so that pyramid levels differ
    blocks = rng.uniform(0.93, 0.995, (height // 8, width // 8))
    blocks[rng.random(blocks.shape) < 0.1] = 1.0  # cleared
    depth = np.repeat(np.repeat(blocks, 8, 0), 8, 1).astype(np.float32)
    levels = occ.pyramid_levels(depth)
    got = occ.occluded(boxes, pv, levels, width, height)
    want, margin = _float64_decision(boxes.astype(np.float64), pv, levels, width, height)
    clear = margin > 1e-3
    assert clear.sum() > n // 2, clear.sum()
    assert np.array_equal(got[clear], want[clear]), np.nonzero(got[clear] != want[clear])[0][:10]
    # the sample exercises both answers
    assert 0.1 < got[clear].mean() < 0.9, got[clear].mean()


def test_restatement_pyramid_of_u16_and_nan():
    d16 = np.array([[0, 65535, 1], [2, 3, 4]], np.uint16)
    levels = occ.pyramid_levels(d16)
    assert [l.shape for l in levels] == [(1, 2), (1, 1)]
    assert levels[0][0, 0] == np.float32(1.0) and levels[0][0, 1] == np.float32(4) / np.float32(65535)
    d32 = np.array([[np.nan, 0.25], [-0.0, 0.5]], np.float32)
    l32 = occ.pyramid_levels(d32)
    assert l32[0][0, 0] == np.float32(1.0)
    z = occ.pyramid_levels(np.array([[-0.0]], np.float32))[0]
    assert z[0, 0] == 0 and not np.signbit(z[0, 0])  # a zero texel is +0
    # a cleared image occludes nothing, whatever the boxes
    boxes = np.array([[-1, -1, 5, 1, 1, 6]], np.float32)
    from renderer_amd import scene
    assert not occ.occluded(boxes, scene.default_pv(), occ.pyramid_levels(np.ones((8, 8), np.float32)), 8, 8).any()
