"""Synthetic shard lists for the three merge kernels (mip_merge_draw_lists, mip_merge_wire_lists, mip_merge_wire_lists_packed):
a builder of the all-gather's receive buffer with any per-chunk counts, a plain numpy expectation, the comparison the GPU
tests use, and the catalogue of count vectors both suites walk. No GPU, no torch device, no frame kernel: every byte of the
expectation is integer arithmetic on lists made from a seed. (tests/test_merge_cases.py checks this module on the CPU,
tests/test_gpu_merge.py runs the kernels against it.)"""
import collections
import functools
import zlib

import numpy as np

from cpu_pipeline import (WIRE_BLOCK, WIRE_BLOCK_WORDS, WIRE_PACKED_BLOCK, WIRE_PACKED_BLOCK_WORDS, encode_wire, encode_wire_packed,
                          wire_live_mask)
from renderer_amd.pipeline import DRAW_CMD_DTYPE, MESH_DTYPE, SHARD_HEADER_BYTES, wire_index_bits

FORMS = ("cmds", "wire", "packed")   # 20-byte commands, 8-byte wire records, packed 4-byte records
DEAD_FILL = 0xDEADBEEF
SENTINEL = 0xA5C3F00D                # what the GPU tests fill out_cmds, its slack rows and out_count with
SLACK_ROWS = 64
CMD_WORDS = 5
HEADER_WORDS = SHARD_HEADER_BYTES // 4
MASK = 0xFFFFFFFF

ShardList = collections.namedtuple("ShardList", "cmds mesh far total first_instance_base n_meshes")
Expected = collections.namedtuple("Expected", "commands count index_total overflowed")


# ---- mesh tables ----

def scene_table():
    """The 64-entry table of the mixed scene (index_bits 25)."""
    from renderer_amd import scene

    return scene.make_scene(3, n=1)["meshes"].copy()


def synthetic_table(m, seed=0):
    """m entries: one to four LODs of several lengths, some entries with one LOD, a few zero-length LODs (whose commands the
    frame kernel drops, so shard_list never emits them), negative and positive vertex offsets."""
    rng = np.random.default_rng(0x7AB1E + 1000 * m + seed)
    t = np.zeros(m, MESH_DTYPE)
    t["aabb_min"] = -0.5
    t["aabb_max"] = 0.5
    t["n_lods"] = rng.integers(1, 5, m)
    t["n_lods"][::3] = 1
    if m > 1:
        t["n_lods"][1] = 2
    lens = 3 * rng.integers(1, 40_000, (m, 4))
    lens[:, 1] = 3 * rng.integers(1, 9_000, m)
    t["index_len"][:, :4] = lens * (np.arange(4)[None, :] < t["n_lods"][:, None])
    if m >= 65:
        t["index_len"][7::50, 0] = 0      # LOD 0 empty
        t["index_len"][13::50, 1] = 0     # LOD 1 empty (only means something where n_lods > 1)
    t["index_offset"][:, :4] = np.cumsum(t["index_len"][:, :4].reshape(-1).astype(np.uint64)).reshape(m, 4) & np.uint64(MASK)
    t["vertex_offset"] = rng.integers(-(1 << 31), 1 << 31, m)
    t["vertex_offset"][0] = -7
    t["vertex_offset"][m - 1] = -(1 << 31) if m > 1 else -7
    return t


TABLE_SIZES = {"scene64": 64, "t1": 1, "t2": 2, "t3": 3, "t65": 65, "t1000": 1000}


@functools.lru_cache(maxsize=None)
def table(name):
    t = scene_table() if name == "scene64" else synthetic_table(TABLE_SIZES[name])
    assert len(t) == TABLE_SIZES[name]
    t.setflags(write=False)
    return t


assert [wire_index_bits(TABLE_SIZES[k]) for k in ("t1", "t2", "t3", "scene64", "t65", "t1000")] == [31, 30, 29, 25, 24, 21]


# ---- one shard's list ----

def _emittable(meshes):
    """(mesh, lod bit) pairs the frame kernel can emit: lod 1 only for a mesh that has one, and never a zero-length LOD
    (tests/test_gpu_parity.py test_lod_switch_and_zero_length_meshes: such a command is dropped by the compaction)."""
    pairs = [(k, 0) for k in range(len(meshes)) if meshes["index_len"][k, 0] > 0]
    pairs += [(k, 1) for k in range(len(meshes)) if meshes["n_lods"][k] > 1 and meshes["index_len"][k, 1] > 0]
    return np.array(pairs, np.uint32).reshape(-1, 2)


def shard_list(rng, meshes, count, first_instance_base, first_index_base, last=None):
    """A 20-byte command list as a frame emits it for one shard, with the mesh and lod bit of every command and the shard's
    draw_index_total. `last` = (instance index, mesh, lod bit) forces the final command (the packed extremes)."""
    pairs = _emittable(meshes)
    pick = pairs[rng.integers(0, len(pairs), count)]
    idx = np.cumsum(rng.integers(1, 4, count, dtype=np.int64)) - 1   # strictly ascending instance indices
    if last is not None and count:
        assert count < 2 or int(idx[-2]) < last[0]
        idx[-1] = last[0]
        pick[-1] = (last[1], last[2])
        assert meshes["index_len"][last[1], last[2]] > 0 and (last[2] == 0 or meshes["n_lods"][last[1]] > 1)
    mesh, far = pick[:, 0].copy(), pick[:, 1].copy()
    lens = meshes["index_len"][mesh, far].astype(np.uint64)
    run = np.cumsum(lens)
    cmds = np.zeros(count, DRAW_CMD_DTYPE)
    cmds["indexCount"] = lens
    cmds["instanceCount"] = 1
    cmds["firstIndex"] = (np.uint64(first_index_base & MASK) + run - lens) & np.uint64(MASK)
    cmds["vertexOffset"] = meshes["vertex_offset"][mesh]
    cmds["firstInstance"] = (idx + (first_instance_base & MASK)) & MASK
    total = int(run[-1]) & MASK if count else 0
    return ShardList(cmds, mesh, far, total, first_instance_base & MASK, len(meshes))


# ---- the receive buffer ----

def body_bytes(capacity, form):
    if form == "cmds":
        return capacity * 20
    per, words = (WIRE_PACKED_BLOCK, WIRE_PACKED_BLOCK_WORDS) if form == "packed" else (WIRE_BLOCK, WIRE_BLOCK_WORDS)
    return (capacity + per - 1) // per * words * 4


def stride_for(capacity, form):
    """What an exchange sizes a chunk to: header + body for `capacity` commands, rounded up to 256 bytes."""
    return (SHARD_HEADER_BYTES + body_bytes(capacity, form) + 255) // 256 * 256


def build_chunks(lists, totals, form, capacity, stride=None, dead_fill=DEAD_FILL, header_counts=None):
    """The all-gather's receive buffer as uint32 words: per chunk a 32-byte MipShardHeader {count, index total, 6 reserved}
    and the body in `form`. A list longer than the stride holds travels cut to what fits (a tightened slice) while its header
    still says the full count; header_counts[k] replaces that count (a corrupt header). Every word the header file calls
    unspecified — record slots at or behind the count, anchors of sub-blocks without records, the body behind the last block,
    the reserved header words — holds dead_fill."""
    assert form in FORMS
    stride = stride_for(capacity, form) if stride is None else stride
    assert stride % 4 == 0 and stride >= SHARD_HEADER_BYTES
    sw = stride // 4
    buf = np.full(len(lists) * sw, dead_fill & MASK, np.uint32)
    room = sw - HEADER_WORDS
    for k, l in enumerate(lists):
        n = len(l.cmds)
        chunk = buf[k * sw:(k + 1) * sw]
        chunk[0] = n if header_counts is None or header_counts[k] is None else header_counts[k]
        chunk[1] = totals[k] & MASK
        if form == "cmds":
            words, live = l.cmds.view(np.uint32).reshape(-1), np.ones(n * CMD_WORDS, bool)
            room_k = room // CMD_WORDS * CMD_WORDS
        elif form == "wire":
            words, live = encode_wire(l.cmds, l.mesh, l.far), wire_live_mask(n)
            room_k = room // WIRE_BLOCK_WORDS * WIRE_BLOCK_WORDS
        else:
            words = encode_wire_packed(l.cmds, l.mesh, l.far, l.first_instance_base, l.n_meshes)
            live = wire_live_mask(n, packed=True)
            room_k = room // WIRE_PACKED_BLOCK_WORDS * WIRE_PACKED_BLOCK_WORDS
        words, live = words[:room_k], live[:room_k]
        body = chunk[HEADER_WORDS:HEADER_WORDS + len(words)]
        body[live] = words[live]
    return buf


def body_of(buf, k, stride):
    return buf[k * stride // 4 + HEADER_WORDS:(k + 1) * stride // 4]


# ---- the expectation ----

def expected_merge(lists, totals, capacity):
    """Plain numpy, independent of the oracle: the lists cut at the capacity and concatenated, each chunk's firstIndex rebased
    by the wrapping sum of the FULL totals of the chunks in front of it (the kernels add the header totals, not the totals of
    what survived the cut)."""
    parts, base, overflowed = [], 0, False
    for l, t in zip(lists, totals):
        cmds = l.cmds if isinstance(l, ShardList) else l
        keep = min(len(cmds), capacity)
        overflowed |= len(cmds) > capacity
        part = np.array(cmds[:keep], DRAW_CMD_DTYPE)
        part["firstIndex"] = (part["firstIndex"].astype(np.uint64) + np.uint64(base)) & np.uint64(MASK)
        parts.append(part)
        base = (base + (int(t) & MASK)) & MASK
    commands = np.concatenate(parts) if parts else np.zeros(0, DRAW_CMD_DTYPE)
    return Expected(commands, len(commands), base, bool(overflowed))


def assert_merge(out_words, out_count, want, what=""):
    """The GPU tests' comparison. out_words = the whole destination as uint32 words (merged list, then every row that was
    allocated behind it, all pre-filled with SENTINEL); out_count = the two words {commands, indices}."""
    out_words = np.asarray(out_words, np.uint32).reshape(-1)
    count, total = int(out_count[0]) & MASK, int(out_count[1]) & MASK
    assert count == want.count, f"{what}: merged count {count}, expected {want.count}"
    assert total == want.index_total, f"{what}: index total {total:#x}, expected {want.index_total:#x}"
    got = out_words[:count * CMD_WORDS].reshape(-1, CMD_WORDS)
    ref = want.commands.view(np.uint32).reshape(-1, CMD_WORDS)
    if got.tobytes() != ref.tobytes():
        row = int(np.argmax((got != ref).any(axis=1)))
        raise AssertionError(f"{what}: command {row} of {count} is {got[row].tolist()}, expected {ref[row].tolist()}")
    behind = out_words[count * CMD_WORDS:]
    assert len(behind) >= SLACK_ROWS * CMD_WORDS, f"{what}: the destination has no slack rows to check"
    if not np.all(behind == SENTINEL):
        word = count * CMD_WORDS + int(np.argmax(behind != SENTINEL))
        raise AssertionError(f"{what}: word {word} (row {word // CMD_WORDS}) behind the merged count {count} was written")


# ---- the catalogue ----

SINGLE = [0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512, 513, 1279, 1280, 1281]
ALIGN_C0 = list(range(0, 9)) + list(range(252, 261))
N_CHUNKS = [1, 2, 3, 7, 8, 9, 31, 32, 33, 63, 64]
WRAP_BASE = 0xFFFFFF00


def _ragged(name, n):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    counts = rng.integers(0, 701, n)
    counts[rng.random(n) < 0.2] = 0
    return [int(c) for c in counts]


def _catalogue():
    c = collections.OrderedDict()
    for n in SINGLE:
        c[f"single-{n}"] = dict(counts=[n])
    for c0 in ALIGN_C0:  # 5 * count_base mod 4 takes every residue for the chunk that starts mid-quad; the 7 is a head- or tail-only round
        c[f"align-{c0}"] = dict(counts=[c0, 300, 7])
    c["empty-all"] = dict(counts=[0] * 5)
    for n in (1, 65, 300):
        c[f"empty-between-{n}"] = dict(counts=[0, n, 0, 0, n, 0])
    c["empty-but-last-of-64"] = dict(counts=[0] * 63 + [333])
    c["empty-but-first-of-64"] = dict(counts=[333] + [0] * 63)
    for n in N_CHUNKS:
        c[f"chunks-{n}"] = dict(counts=_ragged(f"chunks-{n}", n))
    # firstIndex wraps u32 inside chunk 0 (the base is 256 short of 2^32), between chunks (the rebase of chunks 1.. wraps on top of
    # the wrapped base) and in out_count[1]: header totals as much larger shards would report them
    c["wrap-inside-a-chunk"] = dict(counts=[200], first_index_base=WRAP_BASE)
    c["wrap-between-chunks"] = dict(counts=[130, 0, 70, 257], first_index_base=WRAP_BASE, totals=[0x7FFFFFF0, 0x12345678, 0x7FFFFFF0, 0x90000000])
    c["wrap-in-the-index-total"] = dict(counts=[5, 64, 3], first_index_base=WRAP_BASE, totals=[0xFFFFFFFF, 0xFFFFFFFF, 2])
    # packed extremes: the last command of every chunk carries the largest instance index the table's index_bits allow with
    # the table's last (mesh, lod) pair — every bit of the record's index field is set; and a base next to 2^32
    c["packed-largest-index"] = dict(counts=[1, 64, 129], largest_index=True)
    c["packed-base-wraps"] = dict(counts=[70, 300], first_instance_base=0xFFFFFFF0)
    c["packed-largest-index-and-base-wraps"] = dict(counts=[257, 2], largest_index=True, first_instance_base=0xFFFFFFFE)
    return c


CATALOGUE = _catalogue()


def family(name):
    return name.split("-")[0]


def make_lists(tbl, counts, seed, first_instance_base=1000, first_index_base=77, largest_index=False):
    """One ShardList per count, as the shards of one frame: each shard's instances follow the previous shard's."""
    rng = np.random.default_rng(seed)
    lists, base = [], first_instance_base
    pairs = _emittable(tbl)
    for n in counts:
        last = None
        if largest_index and n:
            last = ((1 << wire_index_bits(len(tbl))) - 1, int(pairs[-1, 0]), int(pairs[-1, 1]))
        l = shard_list(rng, tbl, n, base, first_index_base, last=last)
        lists.append(l)
        base = (base + 3 * n + 5) & MASK
    return lists


@functools.lru_cache(maxsize=256)
def case(name, table_name):
    """(lists, totals) of a catalogue entry against a table; deterministic."""
    spec = CATALOGUE[name]
    tbl = table(table_name)
    lists = make_lists(tbl, spec["counts"], zlib.crc32(f"{name}/{table_name}".encode()),
                       first_instance_base=spec.get("first_instance_base", 1000), first_index_base=spec.get("first_index_base", 77),
                       largest_index=spec.get("largest_index", False))
    totals = spec.get("totals") or [l.total for l in lists]
    return lists, [int(t) for t in totals]


def capacity_of(lists):
    return max(1, max(len(l.cmds) for l in lists))


# ---- capacity cuts ----

CUT_CAPACITIES = [100, 257, 1000, 256, 1024]


def cut_case(capacity, which, position):
    """The capacity cuts both suites run: a count of capacity - 1, capacity, capacity + 1 or a header of 0xFFFFFFFF, in a chunk
    of its own ("alone") or in chunk 3 of 6 ("middle"). Returns (lists, totals, header_counts)."""
    tbl = table("scene64")
    n = {"minus1": capacity - 1, "exact": capacity, "plus1": capacity + 1, "ffffffff": capacity + 9}[which]
    counts = [n] if position == "alone" else [min(40, capacity), 0, capacity, n, 17, min(300, capacity)]
    lists = make_lists(tbl, counts, 1000 * capacity + len(which) + len(position))
    header = [None] * len(counts)
    if which == "ffffffff":
        header[counts.index(n) if position == "alone" else 3] = 0xFFFFFFFF
    return lists, [l.total for l in lists], header
