"""Batched draws for sharded scenes on the CPU (include/mi_instance_pipeline.h, mip_batch_draws_shard / mip_merge_batches): the
numpy restatement (tests/batch_merge_restatement.py) merges the chunks of shard_range shards into exactly what
lod_restatement.batch_draws_lods gives for the whole scene; a scene worked out by hand; every rule for bad chunks; the chunk's
layout in C, ctypes and Rust; the native plan check (tests/native/batch_merge_plan_check.cpp, built with the address and
undefined-behaviour sanitizers). Bytes only."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import batch_merge_cases as bc
import batch_merge_restatement as bm
import lod_cases as lc
import lod_restatement as lr
from batch_restatement import bitmap_bits
from renderer_amd import scene
from renderer_amd.pipeline import DRAW_CMD_DTYPE, MESH_DTYPE, batch_chunk_bytes, batch_chunk_ids_offset
from renderer_amd.sharded import batch_chunk_stride_bytes, shard_range

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 0x5A5A5A5A
SIZES = (0, 1, 5, 65, 1025, 4097)
WORLDS = (1, 2, 3, 8, 64)
BASE = 0xFFFFF800   # the global first_instance_base: the ids of the larger scenes wrap


def pack_bits(bits):
    """A bitmap in MipOutputs.visible_bitmap's layout from booleans."""
    words = (len(bits) + 31) // 32
    padded = np.zeros(words * 32, np.uint8)
    padded[:len(bits)] = bits
    return np.packbits(padded, bitorder="little").view(np.uint32)


def thresholds(s, mode, levels=6):
    """Five thresholds at the quantiles of the metric over the scene's instances (float64 here; the rule itself is float32)."""
    d = np.asarray(s["cam_pos"], np.float64)[None, :] - s["pos"].astype(np.float64)
    q = (d * d).sum(axis=1)
    if mode == lr.RELATIVE:
        e = (s["meshes"]["aabb_max"].astype(np.float64) - s["meshes"]["aabb_min"].astype(np.float64))[s["mesh_id"]]
        q = q / (s["scale"].astype(np.float64) ** 2 * (e * e).sum(axis=1))
    q = np.sort(q)
    if len(q) < levels:
        return (1.0, 2.0, 3.0, 4.0, 5.0) if mode == lr.DISTANCE else (0.1, 0.2, 0.3, 0.4, 0.5)
    return tuple(float(np.float32(v)) for v in np.maximum.accumulate([q[len(q) * k // levels] for k in range(1, levels)]))


def make_scene(kind, n):
    """config 2, config 3, or config 3's instances over a table of ten six-level meshes; `n` instances and a bitmap that culls a third."""
    s = scene.make_scene(3 if kind == "six" else kind, n=max(n, 1))
    for k in ("pos", "rot", "scale", "mesh_id"):
        s[k] = s[k][:n].copy()
    s["n"] = n
    rng = np.random.default_rng(n + 17)
    if kind == "six":
        s["meshes"] = lc.chain_table([6] * 10, seed=4)
        s["mesh_id"] = rng.integers(0, 10, n).astype(np.uint32)
    s["bits"] = rng.random(n) < 0.67
    return s


def shard_chunks(s, world, mode, sw, capacity=None, base=BASE):
    chunks = []
    for rank in range(world):
        lo, hi = shard_range(s["n"], world, rank)
        cap = (hi - lo) if capacity is None else capacity
        chunks.append(bm.shard_chunk(s["pos"][lo:hi], s["scale"][lo:hi], s["mesh_id"][lo:hi], s["meshes"], s["cam_pos"], pack_bits(s["bits"][lo:hi]),
                                     mode, sw, (base + lo) & 0xFFFFFFFF, cap))
    return chunks


def assert_equals_unsharded(out, want, what):
    count, members = want["count"], want["members"]
    assert out["batch_count"] == count and out["instance_count"] == members, what
    assert out["cmds_words"][:count].tobytes() == want["cmds"].tobytes(), what
    assert (out["cmds_words"][count:] == SENT).all(), what
    assert out["ids"][:members].tobytes() == want["ids"].tobytes(), what
    assert (out["ids"][members:] == SENT).all(), what


@pytest.mark.parametrize("kind", [2, 3, "six"])
def test_merged_shards_equal_the_unsharded_scene(kind):
    seen_empty_shard = False
    for n in SIZES:
        s = make_scene(kind, n)
        for mode in (lr.DISTANCE, lr.RELATIVE):
            sw = thresholds(s, mode)
            want = lr.batch_draws_lods(s["pos"], s["scale"], s["mesh_id"], s["meshes"], s["cam_pos"], pack_bits(s["bits"]), mode, sw,
                                       first_instance_base=BASE)
            if n >= 1025:
                assert want["count"] >= 2 and 0 < want["members"] < n
            for world in WORLDS:
                per = max(shard_range(n, world, 0)[1], 0)
                chunks = shard_chunks(s, world, mode, sw, capacity=per)
                seen_empty_shard |= any(shard_range(n, world, r)[0] == shard_range(n, world, r)[1] for r in range(world)) and n > 0
                status, out = bm.merge(chunks, per, s["meshes"], sentinel=SENT)
                assert status == bm.OK
                assert_equals_unsharded(out, want, (kind, n, mode, world))
    assert seen_empty_shard   # N < world: empty shards at the end


def test_two_shards_five_instances_two_meshes_by_hand():
    t = np.zeros(2, MESH_DTYPE)
    t["aabb_min"], t["aabb_max"] = (-1, -1, -1), (1, 1, 1)
    t["n_lods"] = (2, 1)
    t["index_len"][0, :2], t["index_offset"][0, :2] = (30, 12), (0, 30)
    t["index_len"][1, 0], t["index_offset"][1, 0] = 6, 42
    t["vertex_offset"] = (0, 7)
    pos = np.array([[1, 0, 0], [20, 0, 0], [2, 0, 0], [0, 30, 0], [0, 0, 3]], np.float32)
    mesh_id = np.array([1, 0, 0, 0, 1], np.uint32)
    scale = np.ones(5, np.float32)
    cam, sw = np.zeros(3, np.float32), (100.0, lr.INF, lr.INF, lr.INF, lr.INF)
    ones = lc.all_bits
    # shard 0 = instances 0..2: buckets (mesh 0 near, mesh 0 far, mesh 1) hold instance 2, 1, 0; shard 1 = instances 3, 4
    c0 = bm.shard_chunk(pos[:3], scale[:3], mesh_id[:3], t, cam, ones(3), lr.DISTANCE, sw, 10, 3)
    c1 = bm.shard_chunk(pos[3:], scale[3:], mesh_id[3:], t, cam, ones(2), lr.DISTANCE, sw, 13, 3)
    assert c0.tolist() == [3, 3, 0, 0, 1, 1, 1, 0, 12, 11, 10]
    assert c1.tolist() == [2, 3, 0, 0, 0, 1, 1, 0, 13, 14, bm.DEAD_FILL]
    status, out = bm.merge([c0, c1], 3, t, sentinel=SENT)
    assert status == bm.OK and out["batch_count"] == 3 and out["instance_count"] == 5
    assert out["ids"].tolist() == [12, 11, 13, 10, 14, SENT]
    assert out["cmds_words"].tolist() == [[30, 1, 0, 0, 0], [12, 2, 30, 0, 1], [6, 2, 42, 7, 3]]
    whole = lr.batch_draws_lods(pos, scale, mesh_id, t, cam, ones(5), lr.DISTANCE, sw, first_instance_base=10)
    assert_equals_unsharded(out, whole, "by hand")


def test_chunk_layout_in_c_ctypes_and_rust():
    from renderer_amd import _lib

    assert C.sizeof(_lib.MipBatchChunkHeader) == 16 == _lib.MIP_BATCH_CHUNK_HEADER_BYTES and _lib.MIP_MAX_BATCH_CHUNKS == 64 == bm.MAX_CHUNKS
    assert _lib.MipBatchChunkHeader.n_buckets.offset == 4 and _lib.MipBatchChunkHeader.reserved.offset == 8
    buckets = (1, 2, 3, 4, 5, 6, 200, 255, 256, 257, 4097, 262145)
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "mi_instance_pipeline.h"
    int main(void) {
      static const unsigned long long b[] = {%s};
      printf("%%zu %%zu %%zu %%zu %%u\n", sizeof(MipBatchChunkHeader), offsetof(MipBatchChunkHeader, members), offsetof(MipBatchChunkHeader, n_buckets),
             offsetof(MipBatchChunkHeader, reserved), (unsigned)MIP_MAX_BATCH_CHUNKS);
      for (size_t k = 0; k < sizeof b / sizeof b[0]; ++k)
        printf("%%llu %%llu %%llu\n", (unsigned long long)MIP_BATCH_CHUNK_IDS_OFFSET(b[k]), (unsigned long long)MIP_BATCH_CHUNK_BYTES(b[k], 0),
               (unsigned long long)MIP_BATCH_CHUNK_BYTES(b[k], 4294967295u));
      return 0;
    }''' % ", ".join(str(b) for b in buckets)
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        lines = subprocess.check_output([exe]).decode().strip().split("\n")
    assert [int(x) for x in lines[0].split()] == [16, 0, 4, 8, 64]
    for b, line in zip(buckets, lines[1:]):
        off = 16 + (b + 3) // 4 * 16
        assert [int(x) for x in line.split()] == [off, off, off + 4 * 4294967295], b
        assert batch_chunk_ids_offset(b) == off == bm.ids_offset_words(b) * 4 and batch_chunk_bytes(b, 7) == off + 28 == bm.chunk_bytes(b, 7)
    assert batch_chunk_stride_bytes(200, 0) == 1024 and batch_chunk_stride_bytes(200, 52) == 1024 and batch_chunk_stride_bytes(200, 53) == 1280
    assert all(batch_chunk_stride_bytes(b, c) % 256 == 0 and batch_chunk_stride_bytes(b, c) >= batch_chunk_bytes(b, c) for b in buckets for c in (0, 1, 999))
    # the Rust binding: the struct, its size guard in the array-length form, the two functions with the header's argument counts
    rust = open(os.path.join(ROOT, "integration", "rust", "mip-sys", "src", "lib.rs")).read()
    assert re.search(r"pub struct MipBatchChunkHeader \{\s*pub members: u32,\s*pub n_buckets: u32,\s*pub reserved: \[u32; 2\],\s*\}", rust)
    assert "const _: [u8; 16] = [0; std::mem::size_of::<MipBatchChunkHeader>()];" in rust
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mi_instance_pipeline.h")).read(), flags=re.S)
    for fn in ("mip_batch_draws_shard", "mip_merge_batches"):
        c_args = re.search(fn + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S).group(1).count(",") + 1
        r_args = re.search(r"pub fn " + fn + r"\((.*?)\)\s*->", rust, flags=re.S).group(1).count(",") + 1
        assert c_args == r_args, (fn, c_args, r_args)


def test_library_exports_the_two_entry_points():
    import renderer_amd

    lib = renderer_amd.load_library()
    assert lib.mip_batch_draws_shard(None, None, None, None, None, 0, 1) == -1   # a NULL context is a status code, not a crash
    assert lib.mip_merge_batches(None, None, 1, 16, 0, None) == -1
    assert lib.mip_abi_version() == 4


def test_plan_either_side_of_every_boundary(tmp_path):
    exe = str(tmp_path / "batch_merge_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "native", "batch_merge_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    lines = out.stdout.strip().split("\n")
    assert lines[-1].startswith("BATCH MERGE PLAN OK") and int(lines[-1].split()[4]) >= 14 * 8 + 1030 + 6 * 10 * 9, out.stdout[-2000:]
    # the tile sizes the GPU catalogue is built around are the plan's
    assert (int(lines[-3].split()[1]), int(lines[-2].split()[1])) == bc.plan_tiles()


# ---- the synthetic catalogue: what it covers, and the restatement's own properties on it ----

def _catalogue():
    return bc.catalogue(*bc.plan_tiles())


def test_catalogue_covers_what_it_claims():
    cat = _catalogue()
    residues, lengths = set(), set()
    for name, counts in cat.items():
        src = np.cumsum(counts, axis=1) - counts
        total = counts.sum(axis=0)
        first = np.cumsum(total) - total
        dst = first[None, :] + np.cumsum(counts, axis=0) - counts
        live = counts > 0
        if name.startswith("lengths_"):
            residues |= set(zip((src[live] % 4).tolist(), (dst[live] % 4).tolist()))
            lengths |= set(counts.reshape(-1).tolist())
    assert residues == {(a, b) for a in range(4) for b in range(4)}
    assert set(bc.LENGTHS) <= lengths
    one = cat["one_bucket_every_rank"]
    assert (one.sum(axis=0) > 0).sum() == 1 and (one.sum(axis=1) > 0).all()
    for name in ("singles_8x200", "singles_3x4097", "singles_64x200"):
        assert (cat[name].sum(axis=0) == 1).all() and cat[name].max() == 1
    assert cat["empty_everywhere"].sum() == 0
    assert (cat["empty_middle"].sum(axis=1) > 0).tolist() == [True, False, False, False, True]
    assert (cat["empty_ends"].sum(axis=1) > 0).tolist() == [False, True, True, True, False]
    last = cat["bucket_only_in_last_rank"]
    assert last[:-1, 150].sum() == 0 and last[-1, 150] > 0
    bt, gt = bc.plan_tiles()
    assert {f"buckets_{b}" for b in (bt - 1, bt, bt + 1)} <= set(cat) and {f"members_{m}" for m in (gt - 1, gt, gt + 1)} <= set(cat)
    tables = sorted(c.size for n, c in cat.items() if n.startswith("table_"))
    assert tables[0] < gt <= tables[-1] and gt in tables and max(c.shape[0] for c in cat.values()) == 64


@pytest.mark.parametrize("name", sorted(bc.catalogue(256, 2048)))
def test_restatement_on_the_catalogue(name):
    """The merge is a stable sort of (bucket, rank, slot): checked here against a direct construction."""
    counts = _catalogue().get(name)
    if counts is None:
        pytest.fail("the catalogue's names depend on the tile sizes: update the parametrisation's defaults to the plan's")
    case = bc.build(counts, seed=3)
    status, out = bm.merge(case["chunks"], case["capacity"], case["meshes"], sentinel=SENT)
    assert status == bm.OK
    off = bm.ids_offset_words(case["n_buckets"])
    keys, vals = [], []
    for r, w in enumerate(case["chunks"]):
        buckets = np.repeat(np.arange(case["n_buckets"]), counts[r])
        keys.append(buckets)
        vals.append(w[off:off + len(buckets)])
    keys, vals = np.concatenate(keys), np.concatenate(vals)
    order = np.argsort(keys, kind="stable")     # ranks are concatenated in order: stable = (bucket, rank, slot)
    members = len(keys)
    assert out["instance_count"] == members and out["ids"][:members].tobytes() == vals[order].astype(np.uint32).tobytes()
    assert (out["ids"][members:] == SENT).all()
    total = counts.sum(axis=0)
    cmds = out["cmds_words"][:out["batch_count"]].reshape(-1).view(DRAW_CMD_DTYPE)
    assert out["batch_count"] == (total > 0).sum() and cmds["instanceCount"].tolist() == total[total > 0].tolist()
    assert cmds["firstInstance"].tolist() == (np.cumsum(total) - total)[total > 0].tolist()
    length, offset, vertex = bm.bucket_draws(case["meshes"])
    assert cmds["indexCount"].tolist() == length[total > 0].tolist() and cmds["firstIndex"].tolist() == offset[total > 0].tolist()
    assert cmds["vertexOffset"].tolist() == vertex[total > 0].tolist()
    assert (out["cmds_words"][out["batch_count"]:] == SENT).all()


# ---- bad chunks ----

def _assert_untouched(status, out, want_status):
    assert status == want_status
    assert out["batch_count"] == 0 and out["instance_count"] == 0
    assert (out["ids"] == SENT).all() and (out["cmds_words"] == SENT).all()


@pytest.mark.parametrize("kind", bc.CORRUPTIONS)
def test_each_corruption_is_err_device(kind):
    case = bc.build(bc._random(5, 200, 11), seed=5)
    for which in (0, 2, 4):
        chunks = list(case["chunks"])
        chunks[which] = bc.corrupt(chunks[which], kind, 200)
        _assert_untouched(*bm.merge(chunks, case["capacity"], case["meshes"], sentinel=SENT), bm.ERR_DEVICE)


def test_overflow_and_precedence():
    case = bc.build(bc._random(5, 200, 12), seed=6)
    cap = case["capacity"]
    largest = int(np.argmax([int(c[0]) for c in case["chunks"]]))
    for which in (0, 2, 4):
        chunks = list(case["chunks"])
        chunks[which] = bc.overflow(chunks[which], 200, cap - int(chunks[which][0]) + 1)      # members = capacity + 1
        _assert_untouched(*bm.merge(chunks, cap, case["meshes"], sentinel=SENT), bm.ERR_CAPACITY)
        chunks[which] = bc.overflow(case["chunks"][which], 200, cap - int(case["chunks"][which][0]))  # members = capacity: fits
        assert bm.merge(chunks, cap, case["meshes"], sentinel=SENT)[0] == bm.OK
        far = list(case["chunks"])
        far[which] = bc.overflow(far[which], 200, 5 * cap + 7, bucket=199)   # counts whose sum runs past the whole output room
        _assert_untouched(*bm.merge(far, cap, case["meshes"], sentinel=SENT), bm.ERR_CAPACITY)
    # the same chunks at a capacity one below the largest chunk: the tightened-chunk overflow
    _assert_untouched(*bm.merge(case["chunks"], cap - 1, case["meshes"], sentinel=SENT), bm.ERR_CAPACITY)
    # both kinds at once: corrupt wins, whichever comes first
    for corrupt_at, overflow_at in ((0, 4), (4, 0), (2, 2)):
        chunks = list(case["chunks"])
        chunks[overflow_at] = bc.overflow(chunks[overflow_at], 200, cap + 1)
        chunks[corrupt_at] = bc.corrupt(chunks[corrupt_at], "reserved0", 200)
        _assert_untouched(*bm.merge(chunks, cap, case["meshes"], sentinel=SENT), bm.ERR_DEVICE)
    assert largest in range(5)
    # 2^24 counts: refused as MIP_ERR_CAPACITY before anything is looked at
    big = lc.chain_table([1] * 262145)
    assert bm.merge([np.zeros(4, np.uint32)] * 64, 0, big)[0] == bm.ERR_CAPACITY
