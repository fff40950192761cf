"""Globally depth-sorted batched draws without a GPU: tests/sorted_restatement.py (written from the header's text) — U over the
float32 bit patterns for both metrics, the identity against the ordered restatement, the runs, the hand-written scenes of
tests/sorted_cases.py; the ABI surface of mip_batch_draws_sorted; the native plan check
(tests/native/batch_sorted_plan_check.cpp, built with the address and undefined-behaviour sanitizers)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lod_cases as lc
import lod_restatement as lr
import order_restatement as orr
import sorted_cases as sc
import sorted_restatement as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi_instance_pipeline.h")
F = np.float32
MODES = (lr.DISTANCE, lr.RELATIVE)


def _positive_sweep():
    """Non-negative float32 bit patterns in ascending order of value: 0, subnormals, every exponent at several mantissas with
    the patterns on both sides of the 16- and 24-bit steps nearby, +inf."""
    bits = [0, 1, 2, 0xFF, 0x100, 0x1FF, 0x200, 0xFFFF, 0x10000, 0x10001, 0x7FFFFF]
    for e in range(1, 255):
        for mant in (0, 1, 0xFF, 0x100, 0xFFFF, 0x10000, 0x20FFFF, 0x210000, 0x3FFFFF, 0x400000, 0x7EFFFF, 0x7F0000, 0x7FFFFF):
            bits.append(e << 23 | mant)
    bits.append(0x7F800000)
    return np.array(sorted(set(bits)), np.uint32)


NANS = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF], np.uint32).view(F)


# ---- U, K and D over the bit patterns ----

def test_u_radial_is_monotone_canonical_for_nans_and_equals_the_ordered_key_at_16_bits():
    q = _positive_sweep().view(F)
    assert (np.diff(q.astype(np.float64)) > 0).all()
    u = sr.u_radial(q)
    assert (np.diff(u) > 0).all() and u[0] == 0 and u[-1] == sr.U_MAX[sr.RADIAL] == 0x7F800000
    assert sr.u_radial(NANS).tolist() == [0x7F800000] * len(NANS)
    assert sr.u_radial(np.array([0.0, -0.0], F)).tolist() == [0, 0x80000000]   # (q is a sum of squares: -0 does not occur)
    for bits in sr.DEPTH_BITS:
        near, far = sr.d_of_u(u, sr.RADIAL, sr.NEAR_FIRST, bits), sr.d_of_u(u, sr.RADIAL, sr.FAR_FIRST, bits)
        s = 32 - bits
        assert np.array_equal(near, u >> s) and (np.diff(near) >= 0).all()
        assert np.array_equal(far, (0x7F800000 >> s) - near) and far.min() == 0 and (np.diff(far) <= 0).all()
        assert max(near.max(), far.max()) < 0xFFFFFFFF
    every = np.concatenate([q, NANS])
    assert np.array_equal(sr.d_of_u(sr.u_radial(every), sr.RADIAL, sr.NEAR_FIRST, 16), orr.k_of_q(every))
    assert np.array_equal(sr.d_of_u(sr.u_radial(every), sr.RADIAL, sr.FAR_FIRST, 16), orr.K_MAX - orr.k_of_q(every))


def test_u_view_axis_is_monotone_with_equal_zeros_and_canonical_nans():
    pos = _positive_sweep()
    neg = (pos[::-1] | np.uint32(0x80000000)).astype(np.uint32)          # -inf ... -0
    z = np.concatenate([neg, pos]).view(F)                               # -inf ... -0, +0 ... +inf
    zero = len(neg) - 1
    assert z[zero] == 0 and np.signbit(z[zero]) and z[zero + 1] == 0 and not np.signbit(z[zero + 1])
    u = sr.u_view_axis(z)
    step = np.diff(u)
    assert (step[np.arange(len(step)) != zero] > 0).all() and step[zero] == 0, "strictly monotone, the two zeros equal"
    assert u[zero] == u[zero + 1] == 0x80000000
    assert u[0] == 0x007FFFFF and u[-1] == sr.U_MAX[sr.VIEW_AXIS] == 0xFF800000 and u.min() == 0x007FFFFF and u.max() == 0xFF800000
    assert sr.u_view_axis(NANS).tolist() == [0xFF800000] * len(NANS)
    # the smallest subnormals either side of zero are one step away from it
    assert sr.u_view_axis(np.array([1, 0x80000001], np.uint32).view(F)).tolist() == [0x80000001, 0x7FFFFFFE]
    for bits in sr.DEPTH_BITS:
        s = 32 - bits
        near, far = sr.d_of_u(u, sr.VIEW_AXIS, sr.NEAR_FIRST, bits), sr.d_of_u(u, sr.VIEW_AXIS, sr.FAR_FIRST, bits)
        assert np.array_equal(near, u >> s) and (np.diff(near) >= 0).all()
        assert np.array_equal(far, (0xFF800000 >> s) - near) and far.min() == 0 and far.max() == (0xFF800000 >> s) - (0x007FFFFF >> s)
        assert max(near.max(), far.max()) < 0xFFFFFFFF
        nan_near = sr.d_of_u(sr.u_view_axis(NANS), sr.VIEW_AXIS, sr.NEAR_FIRST, bits)
        assert (nan_near == near[-1]).all(), "a NaN sorts with +inf"


def test_depth_key_through_positions():
    cam = np.array([1.0, -2.0, 0.5], F)
    pos = np.array([[1, -2, 0.5], [4, 2, 0.5], [1e20, 0, 0], [np.nan, 0, 0], [1, -2, -np.inf]], F)
    # (4-1)^2 + (2+2)^2 = 25 = 0x41C80000
    assert sr.depth_key(pos, cam, sr.RADIAL, sr.NEAR_FIRST, 32).tolist() == [0, 0x41C80000, 0x7F800000, 0x7F800000, 0x7F800000]
    assert sr.depth_key(pos, cam, sr.RADIAL, sr.FAR_FIRST, 24).tolist() == [0x7F8000, 0x7F8000 - 0x41C800, 0, 0, 0]
    # along (0, 2, 0): z = 2 * (y + 2) = 0, 8 (0x41000000), 4, NaN, NaN (-inf * 0 in the last term)
    near = sr.depth_key(pos, cam, sr.VIEW_AXIS, sr.NEAR_FIRST, 32, axis=(0, 2, 0))
    assert near.tolist() == [0x80000000, 0xC1000000, 0xC0800000, 0xFF800000, 0xFF800000]
    # the other way: z = -(x - 1) = -0, -3, -1e20, NaN, NaN
    near = sr.depth_key(pos, cam, sr.VIEW_AXIS, sr.NEAR_FIRST, 16, axis=(-1, 0, 0))
    assert near.tolist() == [0x8000, (~0xC0400000 & 0xFFFFFFFF) >> 16, (~int(np.array([-1e20], F).view(np.uint32)[0]) & 0xFFFFFFFF) >> 16, 0xFF80, 0xFF80]
    for bad in (dict(metric=2), dict(order=0), dict(order=3), dict(depth_bits=8), dict(depth_bits=20), dict(axis=(0, np.inf, 0)), dict(axis=(np.nan, 0, 0))):
        kw = dict(metric=sr.VIEW_AXIS, order=sr.NEAR_FIRST, depth_bits=16, axis=(0, 0, 1))
        kw.update(bad)
        with pytest.raises(ValueError):
            sr.depth_key(pos, cam, kw["metric"], kw["order"], kw["depth_bits"], kw["axis"])
    sr.depth_key(pos, cam, sr.RADIAL, sr.NEAR_FIRST, 16, axis=(np.nan, 0, 0))   # RADIAL ignores the axis


# ---- the slots and the runs ----

def _scenes():
    from renderer_amd import scene

    rng = np.random.default_rng(9)
    for config, n in ((2, 3000), (3, 9000)):
        s = scene.make_scene(config, n=n, all_visible=True)
        bitmap = rng.integers(0, 1 << 32, (n + 31) // 32, dtype=np.uint64).astype(np.uint32)
        yield f"config {config}", s, bitmap
    n = 5000   # few buckets, many ties and specials
    s = scene.make_scene(3, n=n, all_visible=True)
    s["meshes"] = lc.chain_table([6, 3, 1], seed=5)
    s["mesh_id"] = rng.integers(0, 3, n).astype(np.uint32)
    s["pos"] = rng.integers(-6, 7, (n, 3)).astype(F) * F(4.0)
    s["pos"][rng.integers(0, n, 40), rng.integers(0, 3, 40)] = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e20], F), 40)
    yield "grid with specials", s, lc.all_bits(n)


def test_radial_16_resorted_by_bucket_is_the_ordered_restatement():
    """The identity: the RADIAL, 16-bit slots re-sorted stably by bucket are mip_batch_draws_ordered's slots."""
    for what, s, bitmap in _scenes():
        for mode in MODES:
            sw = (16.0, 64.0, 256.0, 1024.0, 4096.0) if mode == lr.DISTANCE else (4.0, 16.0, 64.0, 256.0, 1024.0)
            args = (s["pos"], s["scale"], s["mesh_id"], s["meshes"], s["cam_pos"], bitmap, mode, sw)
            for order in sr.ORDERS:
                got = sr.batch_draws_sorted(*args, sr.RADIAL, order, 16, first_instance_base=0xFFFFFF00)
                ref = orr.batch_draws_ordered(*args, order, first_instance_base=0xFFFFFF00)
                again = got["ids"][np.argsort(got["bucket"], kind="stable")]
                assert again.tobytes() == ref["ids"].tobytes(), (what, mode, order)
                assert got["members"] == ref["members"] > 0
                assert np.array_equal(got["lod"], ref["lod"])


def test_runs_tile_the_slots_and_neighbours_differ():
    for what, s, bitmap in _scenes():
        n = s["n"]
        model = np.arange(n * 16, dtype=np.float32).reshape(n, 16)
        args = (s["pos"], s["scale"], s["mesh_id"], s["meshes"], s["cam_pos"], bitmap, lr.RELATIVE, (4.0, 16.0, 64.0, 256.0, 1024.0))
        ref = lr.batch_draws_lods(*args)
        base, _ = lr.lod_bases(s["meshes"])
        seen = set()
        for metric in sr.METRICS:
            for order in sr.ORDERS:
                for bits in sr.DEPTH_BITS:
                    got = sr.batch_draws_sorted(*args, metric, order, bits, axis=(0.3, -0.2, 0.9), first_instance_base=11, model=model)
                    assert got["members"] == ref["members"] and np.array_equal(np.sort(got["order"]), np.sort(ref["order"])), "the same members"
                    assert np.array_equal(got["ids"], ((got["order"] + 11) & 0xFFFFFFFF).astype(np.uint32)) and np.array_equal(got["model"], model[got["order"]])
                    d = sr.depth_key(s["pos"], s["cam_pos"], metric, order, bits, (0.3, -0.2, 0.9))[got["order"]]
                    assert (np.diff(d) >= 0).all() and (np.diff(got["order"])[np.diff(d) == 0] > 0).all(), "by D, ties in draw order"
                    c = got["cmds"]
                    first, count = c["firstInstance"].astype(np.int64), c["instanceCount"].astype(np.int64)
                    assert first[0] == 0 and (count > 0).all() and np.array_equal(first[1:], (first + count)[:-1]) and first[-1] + count[-1] == got["members"]
                    b = base[s["mesh_id"][got["order"]].astype(np.int64)] + got["lod"][got["order"]]
                    assert np.array_equal(b, got["bucket"])
                    heads = b[first]
                    assert (np.diff(heads) != 0).all(), "neighbouring runs differ"
                    assert np.array_equal(np.repeat(heads, count), b), "every run is one bucket"
                    # the three draw words are the ones mip_batch_draws_lods writes for the bucket
                    ref_bucket = base[s["mesh_id"][ref["order"][ref["cmds"]["firstInstance"]]].astype(np.int64)] + ref["lod"][ref["order"][ref["cmds"]["firstInstance"]]]
                    row = {int(k): r for k, r in zip(ref_bucket, ref["cmds"])}
                    for k, r in zip(heads[:200], c[:200]):
                        assert (r["indexCount"], r["firstIndex"], r["vertexOffset"]) == (row[int(k)]["indexCount"], row[int(k)]["firstIndex"], row[int(k)]["vertexOffset"])
                    assert got["count"] == len(c) > ref["count"], (what, "a mixed scene has more runs than buckets")
                    seen.add(got["ids"].tobytes())
        assert len(seen) >= 4, (what, "metric and order change the order (depth_bits need not, on a coarse grid of positions)")


def test_empty_scenes():
    t = lc.chain_table([2, 1])
    z = np.zeros((0, 3), F)
    got = sr.batch_draws_sorted(z, np.zeros(0, F), np.zeros(0, np.uint32), t, np.zeros(3, F), lc.all_bits(0), lr.DISTANCE, lc.SWITCH, sr.RADIAL, sr.NEAR_FIRST, 16)
    assert got["count"] == 0 and got["members"] == 0 and len(got["ids"]) == 0
    pos = np.ones((5, 3), F)
    got = sr.batch_draws_sorted(pos, np.ones(5, F), np.zeros(5, np.uint32), t, np.zeros(3, F), np.zeros(1, np.uint32), lr.DISTANCE, lc.SWITCH, sr.VIEW_AXIS, sr.FAR_FIRST,
                                32, axis=(1, 0, 0))
    assert got["count"] == 0 and got["members"] == 0


def test_no_bucket_limit():
    t = lc.table_with_buckets(65_537)
    pos = np.zeros((4, 3), F)
    m = len(t)
    got = sr.batch_draws_sorted(pos, np.ones(4, F), np.array([m - 1, 0, m - 1, m - 1], np.uint32), t, np.zeros(3, F), lc.all_bits(4), lr.DISTANCE, lc.SWITCH,
                                sr.RADIAL, sr.NEAR_FIRST, 16)
    assert got["members"] == 4 and got["cmds"]["instanceCount"].tolist() == [1, 1, 2] and got["cmds"]["firstInstance"].tolist() == [0, 1, 2]


# ---- the hand-written scenes ----

def _sorted(s, metric, order, bits, axis=(0.0, 0.0, 0.0), bitmap=None, mode=lr.DISTANCE):
    return sr.batch_draws_sorted(s["pos"], s["scale"], s["mesh_id"], s["meshes"], s["cam_pos"], lc.all_bits(s["n"]) if bitmap is None else bitmap, mode,
                                 lc.SWITCH, metric, order, bits, axis=axis, first_instance_base=5)


def _same(got, s, slots, runs, what):
    assert got["order"].tolist() == list(slots), what
    assert got["cmds"].tobytes() == sc.commands(s["meshes"], runs).tobytes(), what
    assert got["ids"].tolist() == [int(i) + 5 for i in slots], what


def test_hand_written_key_edges():
    s = sc.radial_scene()
    assert sr.depth_u(s["pos"], s["cam_pos"], sr.RADIAL).tolist() == [c[2] for c in sc.RADIAL_CASES], "the table's U column"
    for (order, bits), (slots, runs) in sc.RADIAL_WANT.items():
        for mode in MODES:
            _same(_sorted(s, sr.RADIAL, order, bits, mode=mode), s, slots, runs, ("radial", order, bits))
    s = sc.axis_scene()
    assert sr.depth_u(s["pos"], s["cam_pos"], sr.VIEW_AXIS, sc.VIEW_AXIS_Z).tolist() == [c[2] for c in sc.AXIS_CASES]
    for (order, bits), (slots, runs) in sc.AXIS_WANT.items():
        _same(_sorted(s, sr.VIEW_AXIS, order, bits, axis=sc.VIEW_AXIS_Z), s, slots, runs, ("axis", order, bits))
    for order, (slots, runs) in sc.ZERO_AXIS_WANT.items():
        for bits in sr.DEPTH_BITS:
            _same(_sorted(s, sr.VIEW_AXIS, order, bits, axis=sc.ZERO_AXIS), s, slots, runs, ("zero axis", order, bits))


def test_hand_written_ties_and_runs():
    s = sc.tie_scene()
    for order in sr.ORDERS:
        slots, runs = sc.want_ties(order == sr.NEAR_FIRST)
        for bits in sr.DEPTH_BITS:
            _same(_sorted(s, sr.RADIAL, order, bits), s, slots, runs, ("ties", order, bits))
    for name, runs in sc.RUN_SCENES.items():
        s = sc.run_scene(runs)
        assert s["n"] == sum(length for _, length in runs) <= 4097
        for metric, order in ((sr.RADIAL, sr.NEAR_FIRST), (sr.VIEW_AXIS, sr.FAR_FIRST)):
            _same(_sorted(s, metric, order, 16, axis=(0, 1, 0)), s, range(s["n"]), sc.want_runs(runs), name)
    s, bitmap, slots, runs = sc.last_tile_only()
    _same(_sorted(s, sr.RADIAL, sr.FAR_FIRST, 32, bitmap=bitmap), s, slots, runs, "members only in the last tile")


# ---- the ABI surface ----

def test_sort_policy_layout_in_c_ctypes_and_rust(tmp_path):
    from renderer_amd import _lib

    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "mi_instance_pipeline.h"
    int main(void) {
      printf("%zu %zu %zu %zu %zu %zu %u %u\n", sizeof(MipSortPolicy), offsetof(MipSortPolicy, struct_size), offsetof(MipSortPolicy, metric),
             offsetof(MipSortPolicy, order), offsetof(MipSortPolicy, depth_bits), offsetof(MipSortPolicy, axis), MIP_DEPTH_RADIAL, MIP_DEPTH_VIEW_AXIS);
      return 0;
    }'''
    c = tmp_path / "t.c"
    c.write_text(src)
    exe = str(tmp_path / "t")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe])
    sizes = [int(x) for x in subprocess.check_output([exe]).split()]
    assert sizes == [28, 0, 4, 8, 12, 16, sr.RADIAL, sr.VIEW_AXIS]
    m = _lib.MipSortPolicy
    assert [C.sizeof(m), m.struct_size.offset, m.metric.offset, m.order.offset, m.depth_bits.offset, m.axis.offset] == sizes[:6]
    assert (_lib.MIP_DEPTH_RADIAL, _lib.MIP_DEPTH_VIEW_AXIS) == (sr.RADIAL, sr.VIEW_AXIS)
    assert (_lib.MIP_BATCH_ORDER_NEAR_FIRST, _lib.MIP_BATCH_ORDER_FAR_FIRST) == (sr.NEAR_FIRST, sr.FAR_FIRST)
    rust = open(os.path.join(ROOT, "integration", "rust", "mip-sys", "src", "lib.rs")).read()
    body = re.search(r"pub struct MipSortPolicy \{(.*?)\}", rust, flags=re.S).group(1)
    assert re.findall(r"pub (\w+): ([^,]+),", body) == [("struct_size", "u32"), ("metric", "u32"), ("order", "u32"), ("depth_bits", "u32"), ("axis", "[f32; 3]")]
    assert "const _: [u8; 28] = [0; std::mem::size_of::<MipSortPolicy>()];" in rust
    assert "MIP_DEPTH_RADIAL: u32 = 0" in rust and "MIP_DEPTH_VIEW_AXIS: u32 = 1" in rust
    from renderer_amd.pipeline import make_sort_policy

    p = make_sort_policy("view_axis", "far_first", 24, axis=(1, 2, 3))
    assert (p.struct_size, p.metric, p.order, p.depth_bits, list(p.axis)) == (28, 1, 2, 24, [1.0, 2.0, 3.0])


def test_header_declares_mip_batch_draws_sorted_and_the_library_exports_it():
    """Fails on a tree without the entry point."""
    import renderer_amd
    from renderer_amd import _lib

    text = open(HEADER).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int32_t\s+mip_batch_draws_sorted\s*\(\s*MipContext\s*\*", header)
    assert "mip_batch_draws_sorted" in _lib.EXPORTS
    lib = renderer_amd.load_library()
    assert hasattr(lib, "mip_batch_draws_sorted")
    assert lib.mip_batch_draws_sorted(None, None, None, None, None, None) == -1   # a NULL context is a status code, not a crash
    assert lib.mip_abi_version() == 4   # additive: the ABI version does not move
    assert callable(getattr(renderer_amd.InstancePipeline, "batch_draws_sorted"))
    assert "(D, draw index)" in text and "K = U >> s" in text
    rust = open(os.path.join(ROOT, "integration", "rust", "mip-sys", "src", "lib.rs")).read()
    assert "pub fn mip_batch_draws_sorted(" in rust
    # the two entries left mip_batch_draws_ordered's out-of-scope list
    ordered = text[text.index("Extension: depth-ordered batched draws"):text.index("Extension: globally depth-sorted batched draws")]
    assert "one globally depth-sorted per-instance list" not in ordered


# ---- the launch plan ----

def test_sorted_plan_over_every_mode_metric_and_key_width(tmp_path):
    """plan_batch_sorted (renderer_amd/csrc/batch_plan.hpp): depth_bits / 8 passes, pass 0 by mode and metric, the list kernels
    behind it, the members sum, the model kernel, the run stage's four launches."""
    exe = str(tmp_path / "batch_sorted_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "native", "batch_sorted_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    last = out.stdout.strip().split("\n")[-1]
    assert last.startswith("SORTED PLAN OK"), out.stdout[-2000:]
    assert int(last.split()[3]) == 2 * 2 * 3 * 2 * 2
