"""Depth-ordered batched draws without a GPU: tests/order_restatement.py (written from the header's text) — the depth key over
the float32 bit patterns, the slot order against mip_batch_draws_lods' restatement; the ABI surface of mip_batch_draws_ordered."""
import os
import re

import numpy as np
import pytest

import lod_cases as lc
import lod_restatement as lr
import order_restatement as orr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi_instance_pipeline.h")
F = np.float32
MODES = (lr.DISTANCE, lr.RELATIVE)


def _q_sweep():
    """Non-negative float32 bit patterns in ascending order of value: 0, subnormals, every exponent at several mantissas with
    the patterns on both sides of every 16-bit step nearby, +inf."""
    bits = [0, 1, 2, 0x1FF, 0x200, 0xFFFF, 0x10000, 0x10001, 0x7FFFFF]
    for e in range(1, 255):
        for mant in (0, 1, 0xFFFF, 0x10000, 0x20FFFF, 0x210000, 0x3FFFFF, 0x400000, 0x7EFFFF, 0x7F0000, 0x7FFFFF):
            bits.append(e << 23 | mant)
    bits.append(0x7F800000)
    b = np.array(sorted(set(bits)), np.uint32)
    return b.view(F)


def test_k_is_monotone_over_the_float32_patterns_and_tops_out_at_inf():
    q = _q_sweep()
    assert (np.diff(q.astype(np.float64)) > 0).all() and q[0] == 0 and np.isinf(q[-1])
    k = orr.k_of_q(q)
    assert (np.diff(k) >= 0).all()
    assert k[0] == 0 and k[-1] == orr.K_MAX == 0x7F80 and k.max() == 0x7F80 and k.min() == 0
    assert k[q == np.finfo(F).max][0] == 0x7F7F
    # resolution: a step of K is at most 1/128 of q among the normal numbers
    normal = q[(q >= np.finfo(F).tiny) & np.isfinite(q)].astype(np.float64)
    floor = (normal.astype(F).view(np.uint32) & np.uint32(0xFFFF0000)).view(F).astype(np.float64)
    assert ((normal - floor) / normal < 1.0 / 128).all()
    # subnormals below 2^-133 share K = 0 with q = 0
    assert orr.k_of_q(np.array([0.0, 2.0 ** -149, 2.0 ** -140, 2.0 ** -134], F)).tolist() == [0, 0, 0, 0]
    assert orr.k_of_q(np.array([2.0 ** -133], F)).tolist() == [1]


def test_k_is_canonical_for_nans_of_either_sign():
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF], np.uint32).view(F)
    assert np.isnan(nans).all()
    assert orr.k_of_q(nans).tolist() == [0x7F80] * 6


def test_depth_key_through_positions_orders_and_complement():
    # camera off the origin; positions whose q is 0, finite, +inf and NaN
    cam = np.array([1.0, -2.0, 0.5], F)
    pos = np.array([[1, -2, 0.5], [4, 2, 0.5], [1e20, 0, 0], [np.nan, 0, 0], [1, np.inf, 0], [1, -2, -np.inf], [np.inf, -np.inf, 3]], F)
    near = orr.depth_key(pos, cam, orr.NEAR_FIRST)
    # (4-1)^2 + (2+2)^2 = 25 = 0x41C80000
    assert near.tolist() == [0, 0x41C8, 0x7F80, 0x7F80, 0x7F80, 0x7F80, 0x7F80]
    far = orr.depth_key(pos, cam, orr.FAR_FIRST)
    assert np.array_equal(far, 0x7F80 - near) and far.min() == 0 and far.max() == 0x7F80
    assert not orr.depth_key(pos, cam, orr.DRAW_INDEX).any()
    rng = np.random.default_rng(1)
    p = (rng.normal(0, 1, (5000, 3)) * 10.0 ** rng.uniform(-25, 20, (5000, 1))).astype(F)
    near, far = orr.depth_key(p, cam, orr.NEAR_FIRST), orr.depth_key(p, cam, orr.FAR_FIRST)
    assert np.array_equal(near + far, np.full(5000, 0x7F80)) and near.min() >= 0 and near.max() <= 0x7F80
    # non-decreasing in q itself
    with np.errstate(all="ignore"):
        d = cam[None, :] - p
        q = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert (np.diff(near[np.argsort(q, kind="stable")]) >= 0).all()
    with pytest.raises(ValueError):
        orr.depth_key(p, cam, 3)


def _scenes():
    from renderer_amd import scene

    rng = np.random.default_rng(9)
    for config, n in ((2, 3000), (3, 9000)):
        s = scene.make_scene(config, n=n, all_visible=True)
        bitmap = rng.integers(0, 1 << 32, (n + 31) // 32, dtype=np.uint64).astype(np.uint32)
        yield f"config {config}", s, bitmap
    # few buckets, many ties and specials: one mesh family, positions on a coarse grid with NaN / inf sprinkled in
    n = 5000
    s = scene.make_scene(3, n=n, all_visible=True)
    s["meshes"] = lc.chain_table([6, 3, 1], seed=5)
    s["mesh_id"] = rng.integers(0, 3, n).astype(np.uint32)
    s["pos"] = rng.integers(-6, 7, (n, 3)).astype(F) * F(4.0)
    s["pos"][rng.integers(0, n, 40), rng.integers(0, 3, 40)] = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e20], F), 40)
    yield "grid with specials", s, lc.all_bits(n)


def test_slot_order_against_the_lod_restatement():
    for what, s, bitmap in _scenes():
        n = s["n"]
        model = np.arange(n * 16, dtype=np.float32).reshape(n, 16)
        for mode in MODES:
            sw = (16.0, 64.0, 256.0, 1024.0, 4096.0) if mode == lr.DISTANCE else (4.0, 16.0, 64.0, 256.0, 1024.0)
            args = (s["pos"], s["scale"], s["mesh_id"], s["meshes"], s["cam_pos"], bitmap, mode, sw)
            ref = lr.batch_draws_lods(*args, first_instance_base=11, model=model)
            assert ref["members"] > 0 and ref["count"] > 1
            # DRAW_INDEX is mip_batch_draws_lods in every field
            got = orr.batch_draws_ordered(*args, orr.DRAW_INDEX, first_instance_base=11, model=model)
            assert set(got) == set(ref)
            for key in ref:
                assert np.array_equal(np.asarray(got[key]), np.asarray(ref[key]), equal_nan=True) if key != "cmds" else got[key].tobytes() == ref[key].tobytes(), (what, key)
            base, _ = lr.lod_bases(s["meshes"])
            perms = {}
            for order in (orr.NEAR_FIRST, orr.FAR_FIRST):
                got = orr.batch_draws_ordered(*args, order, first_instance_base=11, model=model)
                assert got["cmds"].tobytes() == ref["cmds"].tobytes() and got["count"] == ref["count"] and got["members"] == ref["members"], what
                assert np.array_equal(got["lod"], ref["lod"])
                assert np.array_equal(got["ids"], ((got["order"] + 11) & 0xFFFFFFFF).astype(np.uint32)) and np.array_equal(got["model"], model[got["order"]])
                k = orr.depth_key(s["pos"], s["cam_pos"], orr.NEAR_FIRST)
                moved = 0
                for c in ref["cmds"]:
                    lo, hi = int(c["firstInstance"]), int(c["firstInstance"]) + int(c["instanceCount"])
                    mine, theirs = got["order"][lo:hi], ref["order"][lo:hi]
                    assert np.array_equal(np.sort(mine), theirs), (what, "a bucket's range is a permutation of the same members")
                    kk = k[mine]
                    step = np.diff(kk)
                    assert (step >= 0).all() if order == orr.NEAR_FIRST else (step <= 0).all(), (what, order)
                    assert (np.diff(mine)[step == 0] > 0).all(), (what, "draw index ascends within equal K")
                    moved += int((mine != theirs).sum())
                    b = base[s["mesh_id"][mine].astype(np.int64)] + got["lod"][mine]
                    assert (b == b[0]).all()
                assert moved > 0, (what, "the order changes something")
                perms[order] = got["order"]
            assert not np.array_equal(perms[orr.NEAR_FIRST], perms[orr.FAR_FIRST])


def test_capacity_of_the_restatement():
    t = lc.table_with_buckets(65_537)
    pos = np.zeros((4, 3), F)
    args = (pos, np.ones(4, F), np.zeros(4, np.uint32), t, np.zeros(3, F), lc.all_bits(4), lr.DISTANCE, lc.SWITCH)
    with pytest.raises(OverflowError):
        orr.batch_draws_ordered(*args, orr.NEAR_FIRST)
    with pytest.raises(OverflowError):
        orr.batch_draws_ordered(*args, orr.FAR_FIRST)
    assert orr.batch_draws_ordered(*args, orr.DRAW_INDEX)["members"] == 4
    assert orr.batch_draws_ordered(*args[:3], lc.table_with_buckets(65_536), *args[4:], orr.NEAR_FIRST)["members"] == 4


# ---- the ABI surface: these fail on a library without the entry point ----

def test_library_exports_mip_batch_draws_ordered_and_the_header_states_the_rule():
    import renderer_amd
    from renderer_amd import _lib

    lib = renderer_amd.load_library()
    assert hasattr(lib, "mip_batch_draws_ordered") and "mip_batch_draws_ordered" in _lib.EXPORTS
    text = open(HEADER).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int32_t\s+mip_batch_draws_ordered\s*\(\s*MipContext\s*\*", header)
    for name, value in (("DRAW_INDEX", 0), ("NEAR_FIRST", 1), ("FAR_FIRST", 2)):
        assert re.search(rf"#define\s+MIP_BATCH_ORDER_{name}\s+{value}u", header)
        assert getattr(_lib, f"MIP_BATCH_ORDER_{name}") == value == getattr(orr, name)
    assert "K = 0x7F80 if q is NaN, else bits(q) >> 16" in text and "(bucket, D, draw index)" in text
    assert lib.mip_abi_version() == 4   # additive: the ABI version does not move
    assert lib.mip_batch_draws_ordered(None, None, None, None, 1, None) == -1
    assert callable(getattr(renderer_amd.InstancePipeline, "batch_draws_ordered"))
    rust = open(os.path.join(ROOT, "integration", "rust", "mip-sys", "src", "lib.rs")).read()
    assert "pub fn mip_batch_draws_ordered(" in rust and "MIP_BATCH_ORDER_FAR_FIRST: u32 = 2" in rust
