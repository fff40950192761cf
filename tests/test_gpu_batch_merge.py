"""Batched draws for sharded scenes on the GPU (include/mi_instance_pipeline.h, mip_batch_draws_shard / mip_merge_batches): the
chunk a shard emits against mip_batch_draws_lods on the same context and the restatement (tests/batch_merge_restatement.py);
the merge of shard_range shards against ONE mip_batch_draws_lods call on a context that holds the whole scene and against the
restatement; a synthetic catalogue of chunks (tests/batch_merge_cases.py); bad chunks; refusals. One GPU: every shard call
writes its chunk straight into the receive buffer at rank x stride. Bytes only: every buffer is filled with a sentinel and
compared whole, slack included."""
import ctypes as C

import numpy as np
import pytest

import batch_merge_cases as bc
import batch_merge_restatement as bm
import lod_cases as lc
import lod_restatement as lr
import test_gpu_batch as T
from renderer_amd.pipeline import batch_chunk_bytes, batch_chunk_ids_offset, make_frame, make_lod_policy
from renderer_amd.sharded import batch_chunk_stride_bytes, shard_range
from test_batch_merge_restatement import pack_bits, thresholds
from test_gpu_batch_lods import _batch, _buckets, _sized

pytestmark = pytest.mark.gpu
ra = T.ra
SENT = bc.SENTINEL
SLACK = bc.SLACK
MODES = (lr.DISTANCE, lr.RELATIVE)
SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 4097)
BASE = 0xFFFFF800


def _dev_words(words):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(words, np.uint32).view(np.int32)).to(T._dev())
    torch.cuda.synchronize()
    return t


def _host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32)


class _Merged:
    """Device outputs of mip_merge_batches with the stated room plus slack, at the sentinel; instance_ids `ids_skew` bytes behind a
    256-byte boundary."""

    def __init__(self, n_buckets, n_chunks, capacity, ids_skew=0):
        self.ids_room, self.cmds_room, self.skew = n_chunks * capacity, min(n_buckets, n_chunks * capacity), ids_skew // 4
        self.ids = _dev_words(np.full(self.skew + self.ids_room + SLACK, SENT, np.uint32))
        self.cmds = _dev_words(np.full((self.cmds_room + SLACK, 5), SENT, np.uint32))
        self.scal = _dev_words(np.full(4, SENT, np.uint32))
        assert self.ids.data_ptr() % 256 == 0

    def kwargs(self, count=True):
        return dict(batch_cmds=self.cmds.data_ptr(), batch_count=self.scal.data_ptr(), instance_ids=self.ids.data_ptr() + 4 * self.skew,
                    instance_count=self.scal.data_ptr() + 4 if count else 0)

    def check(self, want, what, count=True):
        """`want` from bm.merge(..., sentinel=SENT): equal word for word, the slack and the words in front of a skewed list included."""
        ids, cmds, scal = _host(self.ids), _host(self.cmds), _host(self.scal)
        assert int(scal[0]) == want["batch_count"], (what, "batch_count", int(scal[0]), want["batch_count"])
        assert int(scal[1]) == (want["instance_count"] if count else SENT), (what, "instance_count", int(scal[1]))
        assert (scal[2:] == SENT).all(), what
        assert (ids[:self.skew] == SENT).all() and (ids[self.skew + self.ids_room:] == SENT).all(), (what, "ids outside the room")
        assert ids[self.skew:self.skew + self.ids_room].tobytes() == want["ids"].tobytes(), (what, "instance_ids")
        assert cmds[:self.cmds_room].tobytes() == want["cmds_words"].tobytes(), (what, "batch_cmds")
        assert (cmds[self.cmds_room:] == SENT).all(), (what, "commands outside the room")


def _merge_pipeline(ra, meshes):
    """A context that can merge: the mesh table only, max_instances = 1."""
    p = ra.InstancePipeline(max_instances=1, max_meshes=len(meshes))
    p.set_mesh_table(meshes)
    return p


def _chunk_buffer(n_buckets, capacity, slack_words=SLACK):
    return _dev_words(np.full(batch_chunk_bytes(n_buckets, capacity) // 4 + slack_words, SENT, np.uint32))


# ---- 1. the producer ----

def _shard_against_lods(p, s, mode, sw, what, base=BASE, extra=0, bitmap=None):
    """mip_run, then mip_batch_draws_lods and mip_batch_draws_shard over its bitmap, nothing waits in between; the chunk against
    that call's outputs and against the restatement, whole."""
    n, b = s["n"], _buckets(s["meshes"])
    f, lods = T._Frame(n), _batch(n, s["meshes"], model=False)
    chunk = _chunk_buffer(b, n + extra)
    frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=base)
    policy = make_lod_policy(mode, sw)
    given = _dev_words(bitmap) if bitmap is not None else None
    bm_ptr = (given if given is not None else f.bitmap).data_ptr()
    p.run_device(frame, async_=True, **f.kwargs())
    p.batch_draws_lods(frame, bm_ptr, policy, async_=True, **lods.kwargs())
    p.batch_draws_shard(frame, bm_ptr, policy, chunk.data_ptr(), n + extra, async_=True)
    p.wait()
    host_bitmap = f.host_bitmap() if bitmap is None else bitmap
    want = bm.shard_chunk(s["pos"], s["scale"], s["mesh_id"], s["meshes"], s["cam_pos"], host_bitmap, mode, sw, base, n + extra, fill=SENT,
                          stride_words=batch_chunk_bytes(b, n + extra) // 4 + SLACK)
    got = _host(chunk)
    assert got.tobytes() == want.tobytes(), (what, "chunk", np.nonzero(got != want)[0][:8])
    # the same members as the call beside it: its ids, and its commands' instance counts are the non-zero bucket counts
    r = lods.result()
    members, count = int(r["scal"][1]), int(r["scal"][0])
    off = batch_chunk_ids_offset(b) // 4
    assert int(got[0]) == members and got[off:off + members].tobytes() == r["ids"][:members].tobytes(), what
    counts = got[4:4 + b]
    assert counts[counts > 0].tolist() == r["cmds"][:count, 1].tolist(), what
    return want


@pytest.mark.parametrize("config", [2, 3])
def test_chunk_of_a_shard_at_every_size(ra, config):
    for k, n in enumerate(SIZES):
        s = _sized(ra.scene.make_scene(config, n=max(n, 1)), n)
        with T._pipeline(ra, s) as p:
            for mode in MODES:
                want = _shard_against_lods(p, s, mode, thresholds(s, mode), f"config {config} n={n} mode={mode}", extra=(0, 5)[(k + mode) % 2])
                if n == 0:
                    assert want[:4].tolist() == [0, _buckets(s["meshes"]), 0, 0] and not want[4:4 + _buckets(s["meshes"])].any()


@pytest.mark.parametrize("buckets", [1, 2, 6, 200, 255, 256, 257, 4097])
def test_chunk_at_every_bucket_count(ra, buckets):
    n = 3000
    rng = np.random.default_rng(buckets)
    s = ra.scene.make_scene(3, n=n, all_visible=True)
    s["meshes"] = lc.table_with_buckets(buckets, seed=buckets)
    m = len(s["meshes"])
    s["mesh_id"] = rng.integers(0, m, n).astype(np.uint32)
    s["mesh_id"][:50] = m - 1
    with T._pipeline(ra, s) as p:
        for mode in MODES:
            bits = pack_bits(rng.random(n) < 0.8)
            want = _shard_against_lods(p, s, mode, thresholds(s, mode), f"B={buckets} mode={mode}", extra=buckets % 3, bitmap=bits)
            assert int(want[0]) > 0


def test_chunks_of_two_frames_in_flight(ra):
    s = ra.scene.make_scene(3, n=20_000)
    n, b = s["n"], _buckets(s["meshes"])
    cams = [np.array([0.0, 1.0, 2.0], np.float32), np.array([4.0, 1.0, 30.0], np.float32), np.array([-9.0, 2.0, 11.0], np.float32)]
    with T._pipeline(ra, s, frames_in_flight=2) as p:
        frames, chunks = [T._Frame(n) for _ in cams], [_chunk_buffer(b, n) for _ in cams]
        for k, cam in enumerate(cams):
            fr = make_frame(s["planes"], cam, first_instance_base=k * 1000)
            p.run_device(fr, async_=True, **frames[k].kwargs())
            p.batch_draws_shard(fr, frames[k].bitmap.data_ptr(), make_lod_policy(k % 2, thresholds(s, k % 2)), chunks[k].data_ptr(), n, async_=True)
        p.wait()
        seen = set()
        for k, cam in enumerate(cams):
            want = bm.shard_chunk(s["pos"], s["scale"], s["mesh_id"], s["meshes"], cam, frames[k].host_bitmap(), k % 2, thresholds(s, k % 2),
                                  k * 1000, n, fill=SENT, stride_words=batch_chunk_bytes(b, n) // 4 + SLACK)
            assert _host(chunks[k]).tobytes() == want.tobytes(), k
            seen.add(want.tobytes())
        assert len(seen) == len(cams)


def test_refused_shard_calls_write_nothing(ra):
    L = ra._lib
    s = ra.scene.make_scene(2, n=2000, all_visible=True)
    n, b = s["n"], _buckets(s["meshes"])
    with T._pipeline(ra, s) as p:
        lib, ctx = p._lib, p._ctx
        f, chunk = T._Frame(n), _chunk_buffer(b, n)
        frame = make_frame(s["planes"], s["cam_pos"])
        p.run_device(frame, **f.kwargs())
        good = make_lod_policy(lr.DISTANCE, lc.SWITCH)
        bad_mode = make_lod_policy(lr.DISTANCE, lc.SWITCH)
        bad_mode.mode = 2
        decreasing = make_lod_policy(lr.DISTANCE, lc.SWITCH)
        decreasing.switch_sq[2] = 1.0

        def call(fr=frame, bitmap=f.bitmap.data_ptr(), policy=good, ptr=chunk.data_ptr(), cap=n, flags=L.MIP_OUT_DEVICE, c=ctx):
            return lib.mip_batch_draws_shard(c, C.addressof(fr) if fr is not None else None, bitmap, C.addressof(policy) if policy is not None else None,
                                             ptr, cap, flags)

        bad = {"NULL ctx": call(c=None), "NULL frame": call(fr=None), "NULL bitmap": call(bitmap=None), "NULL policy": call(policy=None),
               "NULL chunk": call(ptr=None), "chunk + 4": call(ptr=chunk.data_ptr() + 4), "chunk + 8": call(ptr=chunk.data_ptr() + 8),
               "ids_capacity N - 1": call(cap=n - 1), "ids_capacity 0": call(cap=0), "no MIP_OUT_DEVICE": call(flags=L.MIP_OUT_ASYNC),
               "host flags": call(flags=0), "unknown flag": call(flags=L.MIP_OUT_DEVICE | 0x40), "wire flag": call(flags=L.MIP_OUT_DEVICE | L.MIP_OUT_WIRE),
               "mode 2": call(policy=bad_mode), "decreasing": call(policy=decreasing)}
        assert all(v == -1 for v in bad.values()), bad
        assert (_host(chunk) == SENT).all()
        assert call() == 0 and int(_host(chunk)[1]) == b
    with ra.InstancePipeline(max_instances=16, max_meshes=4) as q:      # no instances, no table: MIP_ERR_NOT_READY
        chunk = _chunk_buffer(6, 16)
        frame = make_frame(s["planes"], s["cam_pos"])
        rc = q._lib.mip_batch_draws_shard(q._ctx, C.addressof(frame), chunk.data_ptr(), C.addressof(good), chunk.data_ptr(), 16, L.MIP_OUT_DEVICE)
        assert rc == -6 and (_host(chunk) == SENT).all()


# ---- 2. identity: the merged shards are the unsharded call, byte for byte ----

@pytest.mark.parametrize("world", [1, 2, 3, 8, 64])
def test_merged_shards_equal_one_call_on_the_whole_scene(ra, world):
    for n in SIZES:
        s = _sized(ra.scene.make_scene(3, n=max(n, 1)), n)
        b = _buckets(s["meshes"])
        per = shard_range(n, world, 0)[1]
        stride = batch_chunk_stride_bytes(b, per)
        with T._pipeline(ra, s) as whole, ra.InstancePipeline(max_instances=max(per, 1), max_meshes=len(s["meshes"])) as shard, \
                _merge_pipeline(ra, s["meshes"]) as merger:
            shard.set_mesh_table(s["meshes"])
            f = T._Frame(n)
            frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=BASE)
            whole.run_device(frame, **f.kwargs())       # the global bitmap: a frame of the whole scene
            bits = np.unpackbits(f.host_bitmap().view(np.uint8), bitorder="little")[:n].astype(bool) if n else np.zeros(0, bool)
            for mode in MODES:
                sw = thresholds(s, mode)
                policy = make_lod_policy(mode, sw)
                lods = _batch(n, s["meshes"], model=False)
                whole.batch_draws_lods(frame, f.bitmap.data_ptr(), policy, **lods.kwargs())
                recv = _dev_words(np.full(world * stride // 4, bc.DEAD_FILL, np.uint32))
                chunks = []
                for rank in range(world):      # one context takes every shard in turn: the bitmap is cut at the shard's bounds
                    lo, hi = shard_range(n, world, rank)
                    shard.set_instances(s["pos"][lo:hi], s["rot"][lo:hi], s["scale"][lo:hi], s["mesh_id"][lo:hi])
                    cut = _dev_words(np.concatenate([pack_bits(bits[lo:hi]), np.zeros(1, np.uint32)]))
                    sf = make_frame(s["planes"], s["cam_pos"], first_instance_base=(BASE + lo) & 0xFFFFFFFF)
                    shard.batch_draws_shard(sf, cut.data_ptr(), policy, recv.data_ptr() + rank * stride, per)
                    chunks.append(bm.shard_chunk(s["pos"][lo:hi], s["scale"][lo:hi], s["mesh_id"][lo:hi], s["meshes"], s["cam_pos"], pack_bits(bits[lo:hi]),
                                                 mode, sw, (BASE + lo) & 0xFFFFFFFF, per, stride_words=stride // 4))
                assert _host(recv).tobytes() == np.concatenate(chunks).tobytes(), (world, n, mode, "the gathered chunks")
                out = _Merged(b, world, per)
                merger.merge_batches(recv.data_ptr(), world, stride, per, **out.kwargs())
                status, want = bm.merge(chunks, per, s["meshes"], sentinel=SENT)
                assert status == bm.OK
                out.check(want, (world, n, mode))
                # ... and against the one call on the whole scene
                r = lods.result()
                count, members = int(r["scal"][0]), int(r["scal"][1])
                assert (count, members) == (want["batch_count"], want["instance_count"]), (world, n, mode)
                assert r["cmds"][:count].tobytes() == _host(out.cmds)[:count].tobytes(), (world, n, mode, "commands")
                assert r["ids"][:members].tobytes() == _host(out.ids)[:members].tobytes(), (world, n, mode, "ids")
                if n >= 1023:
                    assert count > 6 and 0 < members < n


# ---- 3. the synthetic catalogue ----

def _run_case(ra, pipes, name, counts, k):
    """Variant k of a case: instance_ids 0 / 4 / 8 / 12 bytes behind a 256-byte boundary; every other case a stride above the
    minimum with dead words behind the chunk; every third a capacity below what the stride has room for; every other one
    asynchronous."""
    skew = 4 * (k % 4)
    roomy_stride, short_capacity, async_ = k % 2 == 1, k % 3 == 2, (k // 2) % 2 == 1
    members = counts.sum(axis=1)
    capacity = int(members.max())
    b = counts.shape[1]
    words = bm.ids_offset_words(b) + capacity + (9 if short_capacity else 0)
    stride_words = (words + 3) // 4 * 4 + (16 * (k % 5 + 1) if roomy_stride else 0)
    case = bc.build(counts, seed=k, capacity=capacity, stride_words=stride_words)
    if b not in pipes:
        pipes[b] = _merge_pipeline(ra, case["meshes"])
    p = pipes[b]
    recv = _dev_words(case["buffer"])
    out = _Merged(b, len(counts), capacity, ids_skew=skew)
    p.merge_batches(recv.data_ptr(), len(counts), stride_words * 4, capacity, async_=async_, **out.kwargs(count=k % 7 != 6))
    if async_:
        p.wait()
    status, want = bm.merge(case["chunks"], capacity, case["meshes"], sentinel=SENT)
    assert status == bm.OK
    out.check(want, (name, k), count=k % 7 != 6)
    assert _host(recv).tobytes() == case["buffer"].tobytes(), (name, "the chunks were written")


@pytest.mark.parametrize("family", ["lengths", "rest"])
def test_synthetic_catalogue(ra, family):
    cat = bc.catalogue(*bc.plan_tiles())
    names = [n for n in sorted(cat) if n.startswith("lengths_") == (family == "lengths")]
    assert len(names) >= 16
    pipes = {}
    try:
        for k, name in enumerate(names):
            _run_case(ra, pipes, name, cat[name], k)
            if family == "lengths":   # every length at every skew of the output list
                _run_case(ra, pipes, name, cat[name], k + 1)
    finally:
        for p in pipes.values():
            p.close()


# ---- 4. bad chunks ----

def _bad(ra, p, case, chunks, want_code, what, async_):
    from renderer_amd import MipError

    recv = _dev_words(np.concatenate(chunks))
    out = _Merged(case["n_buckets"], len(chunks), case["capacity"], ids_skew=4)
    with pytest.raises(MipError) as e:
        p.merge_batches(recv.data_ptr(), len(chunks), case["stride_words"] * 4, case["capacity"], async_=async_, **out.kwargs())
        if async_:
            p.wait()
    assert e.value.code == want_code, (what, e.value.code)
    status, want = bm.merge(chunks, case["capacity"], case["meshes"], sentinel=SENT)
    assert status == want_code and want["batch_count"] == 0 and want["instance_count"] == 0
    out.check(want, what)     # two zeros, every other word at the sentinel
    p.wait()                  # the error was reported once


def test_bad_chunks_leave_two_zeros_and_nothing_else(ra):
    counts = bc._random(5, 200, 11)
    case = bc.build(counts, seed=5)
    cap = case["capacity"]
    with _merge_pipeline(ra, case["meshes"]) as p:
        k = 0
        for kind in bc.CORRUPTIONS:
            for which in (0, 2, 4):
                chunks = list(case["chunks"])
                chunks[which] = bc.corrupt(chunks[which], kind, 200)
                _bad(ra, p, case, chunks, bm.ERR_DEVICE, (kind, which), async_=k % 2 == 1)
                k += 1
        for which in (0, 2, 4):
            chunks = list(case["chunks"])
            chunks[which] = bc.overflow(chunks[which], 200, cap - int(chunks[which][0]) + 1)          # overflow by one
            _bad(ra, p, case, chunks, bm.ERR_CAPACITY, ("overflow by one", which), async_=which == 2)
            far = list(case["chunks"])
            far[which] = bc.overflow(far[which], 200, 5 * cap + 7, bucket=199)                           # counts past the whole output room
            _bad(ra, p, case, far, bm.ERR_CAPACITY, ("past the room", which), async_=which == 0)
            huge = list(case["chunks"])
            huge[which] = bc.overflow(huge[which], 200, 0xFFFF0000, bucket=which)                        # ... by almost 2^32
            _bad(ra, p, case, huge, bm.ERR_CAPACITY, ("almost 2^32", which), async_=False)
        for corrupt_at, overflow_at in ((0, 4), (4, 0), (2, 2)):                                         # both kinds at once: corrupt wins
            chunks = list(case["chunks"])
            chunks[overflow_at] = bc.overflow(chunks[overflow_at], 200, cap + 1)
            chunks[corrupt_at] = bc.corrupt(chunks[corrupt_at], "reserved0", 200)
            _bad(ra, p, case, chunks, bm.ERR_DEVICE, ("both", corrupt_at, overflow_at), async_=corrupt_at == 4)
        # the context is as good as before
        out = _Merged(200, 5, cap)
        p.merge_batches(_dev_words(case["buffer"]).data_ptr(), 5, case["stride_words"] * 4, cap, **out.kwargs())
        out.check(bm.merge(case["chunks"], cap, case["meshes"], sentinel=SENT)[1], "after the bad chunks")


# ---- 5. refusals ----

def test_refused_merges_write_nothing(ra):
    L = ra._lib
    case = bc.build(bc._random(3, 200, 13), seed=7)
    cap, stride = case["capacity"], case["stride_words"] * 4
    with _merge_pipeline(ra, case["meshes"]) as p:
        lib, ctx = p._lib, p._ctx
        recv = _dev_words(case["buffer"])
        out = _Merged(200, 3, cap)
        model = _dev_words(np.full(16, SENT, np.uint32))

        def outputs(**kw):
            o = L.MipBatchOutputs()
            o.struct_size = C.sizeof(L.MipBatchOutputs)
            o.flags = L.MIP_OUT_DEVICE
            o.batch_cmds, o.batch_count, o.instance_ids, o.instance_count = out.cmds.data_ptr(), out.scal.data_ptr(), out.ids.data_ptr(), out.scal.data_ptr() + 4
            for key, v in kw.items():
                setattr(o, key, v)
            return o

        def call(o=None, chunks=recv.data_ptr(), n=3, st=stride, capacity=cap, c=ctx, null_out=False):
            o = o or outputs()
            return lib.mip_merge_batches(c, chunks, n, st, capacity, None if null_out else C.addressof(o))

        bad = {"NULL ctx": call(c=None), "NULL chunks": call(chunks=None), "NULL out": call(null_out=True),
               "struct_size": call(outputs(struct_size=40)), "unknown flag": call(outputs(flags=L.MIP_OUT_DEVICE | 0x10)),
               "no MIP_OUT_DEVICE": call(outputs(flags=L.MIP_OUT_ASYNC)), "NULL cmds": call(outputs(batch_cmds=None)),
               "NULL count": call(outputs(batch_count=None)), "NULL ids": call(outputs(instance_ids=None)),
               "batch_model": call(outputs(batch_model=model.data_ptr())), "ids + 2": call(outputs(instance_ids=out.ids.data_ptr() + 2)),
               "cmds + 1": call(outputs(batch_cmds=out.cmds.data_ptr() + 1)), "chunks + 4": call(chunks=recv.data_ptr() + 4),
               "chunks + 8": call(chunks=recv.data_ptr() + 8), "no chunks": call(n=0), "65 chunks": call(n=65),
               "stride + 4": call(st=stride + 4), "stride + 8": call(st=stride + 8), "stride - 16": call(st=batch_chunk_bytes(200, cap) // 16 * 16 - 16),
               "capacity above the stride": call(capacity=cap + 8)}
        assert all(v == -1 for v in bad.values()), bad
        assert lib.mip_last_error(ctx)
        assert call(capacity=1 << 31, st=1 << 40, n=2) == -4      # 2 x 2^31 ids: the merged list does not fit a 32-bit count
        out.check(dict(batch_count=SENT, instance_count=SENT, ids=np.full(out.ids_room, SENT, np.uint32),
                       cmds_words=np.full((out.cmds_room, 5), SENT, np.uint32)), "refused calls")
        assert call() == 0
        out.check(bm.merge(case["chunks"], cap, case["meshes"], sentinel=SENT)[1], "after the refused calls")
    with ra.InstancePipeline(max_instances=1, max_meshes=4) as q:     # no mesh table
        o = outputs()
        assert q._lib.mip_merge_batches(q._ctx, recv.data_ptr(), 3, stride, cap, C.addressof(o)) == -6


def test_more_than_2_24_counts_are_refused(ra):
    meshes = lc.chain_table([1] * 262_145)
    b = 262_145
    stride = batch_chunk_bytes(b, 0)
    with _merge_pipeline(ra, meshes) as p:
        words = np.zeros((64, stride // 4), np.uint32)
        words[:, 1] = b                                                       # 64 good chunks without members
        recv = _dev_words(words.reshape(-1))
        out = _Merged(b, 64, 1)
        from renderer_amd import MipError

        with pytest.raises(MipError) as e:
            p.merge_batches(recv.data_ptr(), 64, stride, 0, **out.kwargs())
        assert e.value.code == -4
        assert (_host(out.scal) == SENT).all() and (_host(out.ids) == SENT).all() and (_host(out.cmds) == SENT).all()
        small = _Merged(b, 63, 0)
        p.merge_batches(recv.data_ptr(), 63, stride, 0, **small.kwargs())     # 63 x 262 145 < 2^24: zero members, two zeros
        assert _host(small.scal)[:2].tolist() == [0, 0]
