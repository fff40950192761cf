"""numpy restatement of batched draws for sharded scenes (include/mi_instance_pipeline.h, mip_batch_draws_shard and
mip_merge_batches), written from the header's text: the chunk {members, B, 0, 0 | bucket_count[B] | pad | ids}, and the merge of
R chunks in rank order into commands, counts and ids. Only integers. Not reference behaviour: this file is what the library is
checked against. Words the header leaves untouched stay at the caller's sentinel."""
import numpy as np

import lod_restatement as lr
from renderer_amd.pipeline import DRAW_CMD_DTYPE

HEADER_WORDS = 4
MAX_CHUNKS = 64
MAX_TABLE = 1 << 24
OK, ERR_CAPACITY, ERR_DEVICE = 0, -4, -5
DEAD_FILL = 0xDEADBEEF


def ids_offset_words(n_buckets):
    """MIP_BATCH_CHUNK_IDS_OFFSET(B) / 4: the header, B counts, the pad that makes the ids start at a multiple of 16 bytes."""
    return HEADER_WORDS + n_buckets + (4 - n_buckets % 4) % 4


def chunk_bytes(n_buckets, capacity):
    return (ids_offset_words(n_buckets) + capacity) * 4


def build_chunk(bucket_count, ids, capacity, members=None, n_buckets=None, reserved=(0, 0), fill=DEAD_FILL, stride_words=None):
    """A chunk as uint32 words: `stride_words` of them (default: exactly the chunk), every word the format leaves unspecified —
    the ids at or behind `members`, the words behind the chunk — at `fill`. members / n_buckets / reserved override what the
    counts and ids imply (corrupt chunks)."""
    bucket_count = np.asarray(bucket_count, np.uint32).reshape(-1)
    ids = np.asarray(ids, np.uint32).reshape(-1)
    b = len(bucket_count)
    off = ids_offset_words(b)
    words = off + capacity
    out = np.full(max(stride_words or words, words), fill, np.uint32)
    out[0] = len(ids) if members is None else members
    out[1] = b if n_buckets is None else n_buckets
    out[2], out[3] = reserved
    out[HEADER_WORDS:HEADER_WORDS + b] = bucket_count
    out[HEADER_WORDS + b:off] = 0
    keep = min(len(ids), capacity)
    out[off:off + keep] = ids[:keep]
    return out


def shard_chunk(pos, scale, mesh_id, meshes, cam_pos, visible_bitmap, mode, switch_sq, first_instance_base, capacity, **kw):
    """The chunk mip_batch_draws_shard writes for a shard: lod_restatement.batch_draws_lods of the shard, its ids, and the
    dense member count of every bucket."""
    r = lr.batch_draws_lods(pos, scale, mesh_id, meshes, cam_pos, visible_bitmap, mode, switch_sq, first_instance_base=first_instance_base)
    base, n_buckets = lr.lod_bases(meshes)
    inst = r["order"]
    bucket = base[np.asarray(mesh_id, np.uint32).reshape(-1).astype(np.int64)[inst]] + r["lod"][inst]
    counts = np.bincount(bucket, minlength=n_buckets).astype(np.uint32)
    assert np.array_equal(bucket, np.sort(bucket, kind="stable")) and int(counts.sum()) == r["members"]
    return build_chunk(counts, r["ids"], capacity, **kw)


def bucket_draws(meshes):
    """(indexCount, firstIndex, vertexOffset) of every bucket of the table, in bucket order."""
    base, n_buckets = lr.lod_bases(meshes)
    b = np.arange(n_buckets)
    mesh = np.searchsorted(base, b, side="right") - 1
    lod = b - base[mesh]
    return meshes["index_len"][mesh, lod], meshes["index_offset"][mesh, lod], meshes["vertex_offset"][mesh]


def merge(chunks, capacity, meshes, sentinel=0x5A5A5A5A, ids_room=None, cmds_room=None):
    """chunks: R arrays of uint32 words (at least chunk_bytes(B, capacity) / 4 each), rank order. Returns (status, dict(cmds_words
    (rows of 5 uint32), batch_count, ids, instance_count)) with room for R x capacity ids and min(B, R x capacity) commands
    (or the rooms given), every untouched word at `sentinel`."""
    r_n = len(chunks)
    _, n_buckets = lr.lod_bases(meshes)
    assert 1 <= r_n <= MAX_CHUNKS
    if r_n * n_buckets > MAX_TABLE:
        return ERR_CAPACITY, None
    slots = r_n * capacity
    ids = np.full(slots if ids_room is None else ids_room, sentinel, np.uint32)
    cmds = np.full((min(n_buckets, slots) if cmds_room is None else cmds_room, 5), sentinel, np.uint32)
    off = ids_offset_words(n_buckets)
    c = np.zeros((r_n, n_buckets), np.uint64)
    corrupt = overflow = False
    for r, w in enumerate(chunks):
        w = np.asarray(w, np.uint32)
        c[r] = w[HEADER_WORDS:HEADER_WORDS + n_buckets]
        if int(w[1]) != n_buckets or int(w[2]) != 0 or int(w[3]) != 0 or int(c[r].sum()) != int(w[0]):
            corrupt = True
        elif int(w[0]) > capacity:
            overflow = True
    if corrupt or overflow:
        return (ERR_DEVICE if corrupt else ERR_CAPACITY), dict(cmds_words=cmds, batch_count=0, ids=ids, instance_count=0)
    c = c.astype(np.int64)
    total = c.sum(axis=0)
    first = np.cumsum(total) - total
    src = np.cumsum(c, axis=1) - c                  # where bucket b's ids start in chunk r
    before = np.cumsum(c, axis=0) - c               # members of bucket b in the chunks in front of r
    for b in np.nonzero(total)[0]:
        for r in np.nonzero(c[:, b])[0]:
            to = first[b] + before[r, b]
            ids[to:to + c[r, b]] = np.asarray(chunks[r], np.uint32)[off + src[r, b]:off + src[r, b] + c[r, b]]
    live = np.nonzero(total)[0]
    length, offset, vertex = bucket_draws(meshes)
    rows = np.zeros(len(live), DRAW_CMD_DTYPE)
    rows["indexCount"], rows["instanceCount"], rows["firstIndex"] = length[live], total[live], offset[live]
    rows["vertexOffset"], rows["firstInstance"] = vertex[live], first[live]
    cmds[:len(live)] = rows.view(np.uint32).reshape(-1, 5)
    return OK, dict(cmds_words=cmds, batch_count=len(live), ids=ids, instance_count=int(total.sum()))
