"""Synthetic shard chunks for mip_merge_batches (include/mi_instance_pipeline.h), in the manner of merge_cases.py: a case is a
bucket count B and a matrix of counts c[R][B]; the chunks are built on the CPU (batch_merge_restatement.build_chunk) with
0xDEADBEEF in every word the format leaves unspecified — the ids at or behind `members`, the words behind the chunk up to
the stride. The tables are lod_cases.table_with_buckets(B). Used by the CPU tests against the restatement's hand-checkable
properties and by the GPU tests against the restatement."""
import numpy as np

import batch_merge_restatement as bm
import lod_cases as lc

DEAD_FILL = bm.DEAD_FILL
SENTINEL = 0xA5C3F00D   # what the tests fill every output with
SLACK = 64              # sentinel words (ids) / rows (commands) behind the stated room
LENGTHS = [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]


def _lengths_case(src_shift, dst_shift):
    """Two ranks, one bucket per length and rank in turn; bucket 0 moves every later destination by dst_shift (and rank 0's
    sources with it), bucket 1 moves rank 1's sources by src_shift."""
    b = 2 + 2 * len(LENGTHS)
    c = np.zeros((2, b), np.int64)
    c[0, 0] = dst_shift
    c[1, 1] = src_shift
    for k, n in enumerate(LENGTHS):
        c[k % 2, 2 + 2 * k] = n
        c[(k + 1) % 2, 2 + 2 * k] = LENGTHS[(k + 5) % len(LENGTHS)]
        c[(k + 1) % 2, 3 + 2 * k] = n
    return c


def _one_bucket(r, b, which, each):
    c = np.zeros((r, b), np.int64)
    c[:, which] = each
    return c


def _singles(r, b):
    c = np.zeros((r, b), np.int64)
    c[(np.arange(b) * 7 + 3) % r, np.arange(b)] = 1
    return c


def _random(r, b, seed, top=40, empty_ranks=()):
    rng = np.random.default_rng(seed)
    c = rng.integers(0, top, (r, b)) * (rng.random((r, b)) < 0.6)
    c[list(empty_ranks), :] = 0
    return c.astype(np.int64)


def _total(r, b, members, seed):
    """Counts that sum to exactly `members` over all chunks."""
    rng = np.random.default_rng(seed)
    flat = np.bincount(rng.integers(0, r * b, members), minlength=r * b)
    return flat.reshape(r, b).astype(np.int64)


def catalogue(bucket_tile, gather_tile):
    """name -> counts. The two tile sizes are the kernels' (renderer_amd/csrc/batch_merge_plan.hpp), read by the caller."""
    cases = {}
    for s in range(4):
        for d in range(4):
            cases[f"lengths_src{s}_dst{d}"] = _lengths_case(s, d)
    cases["one_bucket_every_rank"] = _one_bucket(8, 200, 37, 300)
    cases["one_bucket_last_bucket"] = _one_bucket(3, 6, 5, 1500)
    cases["singles_8x200"] = _singles(8, 200)
    cases["singles_3x4097"] = _singles(3, 4097)
    cases["singles_64x200"] = _singles(64, 200)         # 12 800 (bucket, rank) cells, 200 one-id segments
    cases["empty_middle"] = _random(5, 200, 1, empty_ranks=(1, 2, 3))
    cases["empty_ends"] = _random(5, 200, 2, empty_ranks=(0, 4))
    cases["empty_everywhere"] = np.zeros((4, 6), np.int64)
    cases["one_chunk"] = _random(1, 200, 3)
    cases["one_chunk_one_bucket"] = _one_bucket(1, 1, 0, 777)
    last = _random(8, 200, 4)
    last[:7, 150] = 0
    last[7, 150] = 9
    cases["bucket_only_in_last_rank"] = last
    cases["sixty_four_ranks"] = _random(64, 6, 5, top=9)
    for b in (bucket_tile - 1, bucket_tile, bucket_tile + 1, 2 * bucket_tile, 2 * bucket_tile + 1):
        cases[f"buckets_{b}"] = _random(3, b, b, top=5)
    for r, b in ((1, gather_tile - 1), (8, gather_tile // 8), (1, gather_tile + 1), (23, (gather_tile - 1) // 23), (3, gather_tile // 3 + 1)):
        cases[f"table_{r}x{b}"] = _random(r, b, r * b, top=4)
    for members in (gather_tile - 1, gather_tile, gather_tile + 1, 3 * gather_tile, 3 * gather_tile + 1):
        cases[f"members_{members}"] = _total(4, 50, members, members)
    cases["members_in_one_tile_many_segments"] = _total(8, gather_tile, gather_tile, 9)
    return cases


def build(counts, seed=0, capacity=None, stride_words=None):
    """Returns dict(meshes, n_buckets, capacity, stride_words, chunks (list of word arrays), buffer (the chunks stride_words apart,
    one array)). capacity defaults to the largest chunk's members, the stride to the chunk rounded up to 16 bytes."""
    counts = np.asarray(counts, np.int64)
    r_n, b = counts.shape
    rng = np.random.default_rng(seed + 1000)
    members = counts.sum(axis=1)
    if capacity is None:
        capacity = int(members.max())
    words = bm.ids_offset_words(b) + capacity
    if stride_words is None:
        stride_words = (words + 3) // 4 * 4
    assert stride_words % 4 == 0 and stride_words >= words
    chunks = [bm.build_chunk(counts[r], rng.integers(0, 2 ** 32, int(members[r]), dtype=np.uint64).astype(np.uint32), capacity,
                             stride_words=stride_words) for r in range(r_n)]
    return dict(meshes=lc.table_with_buckets(b, seed=b % 97 + 1), n_buckets=b, capacity=capacity, stride_words=stride_words, chunks=chunks,
                buffer=np.concatenate(chunks))


CORRUPTIONS = ("n_buckets_low", "n_buckets_high", "reserved0", "reserved1", "members_low", "members_high", "sum_wraps")


def corrupt(chunk, kind, n_buckets):
    """A copy of the chunk's words that breaks one rule of the format."""
    w = np.array(chunk, np.uint32)
    if kind == "n_buckets_low":
        w[1] = n_buckets - 1
    elif kind == "n_buckets_high":
        w[1] = n_buckets + 1
    elif kind == "reserved0":
        w[2] = 1
    elif kind == "reserved1":
        w[3] = 0x80000000
    elif kind == "members_low":
        w[0] = (int(w[0]) - 1) & 0xFFFFFFFF     # (0 members become 2^32 - 1)
    elif kind == "members_high":
        w[0] = int(w[0]) + 1
    elif kind == "sum_wraps":                  # two counts that add 2^32: equal to `members` only in 32-bit arithmetic
        assert n_buckets >= 2
        w[bm.HEADER_WORDS] = int(w[bm.HEADER_WORDS]) + 0x80000000 & 0xFFFFFFFF
        w[bm.HEADER_WORDS + 1] = int(w[bm.HEADER_WORDS + 1]) + 0x80000000 & 0xFFFFFFFF
    else:
        raise KeyError(kind)
    return w


def overflow(chunk, n_buckets, by, bucket=0):
    """A copy whose bucket `bucket` and `members` both grow by `by`: a consistent chunk that holds more than the exchange moved."""
    w = np.array(chunk, np.uint32)
    w[0] = int(w[0]) + by
    w[bm.HEADER_WORDS + bucket] = int(w[bm.HEADER_WORDS + bucket]) + by
    return w


def plan_tiles():
    """(bucket tile, gather tile) of the two merge kernels, read from renderer_amd/csrc/batch_merge_plan.hpp."""
    import os
    import re

    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "renderer_amd", "csrc", "batch_merge_plan.hpp")).read()
    v = {k: int(x) for k, x in re.findall(r"constexpr uint32_t (kBatchMerge(?:Threads|BucketTile|SlotsPerThread)) = (\d+);", text)}
    assert re.search(r"kBatchMergeGatherTile = kBatchMergeThreads \* kBatchMergeSlotsPerThread;", text)
    return v["kBatchMergeBucketTile"], v["kBatchMergeThreads"] * v["kBatchMergeSlotsPerThread"]
