"""One batched-draws scratch serving different entry points in turn (renderer_amd/csrc/api_batch.hip: ensure_scratch, run_passes).
Every frame slot has ONE scratch object whose buffers are allocated at first need — the counts by the first call, the lists by
the first call of several passes, the slot map by the first such call with matrices, the bucket map by the first sorted call —
and mip_batch_draws_views has one of the same type that grows with the call. The other batch suites run every entry point in
a context of its own; here one context runs all of them in sequence, forwards and backwards, at N = 1025 (a full 1024-entry
tile and a ragged one) over a one-pass table (config 3's 200 buckets) and a two-pass one (257 buckets), and every output
buffer of every call — whole, sentinel padding included — equals the bytes of the same call on a fresh context and the numpy
restatement's. Not reference behaviour."""
import os
import subprocess
import sys

import numpy as np
import pytest

import batch_merge_restatement as bm
import batch_restatement as br
import lod_cases as lc
import lod_restatement as lr
import order_restatement as orr
import sorted_restatement as sr
import test_gpu_batch as T
import test_gpu_batch_lods as TL
import test_gpu_batch_merge as TM
import test_gpu_batch_sorted as TS
import test_gpu_batch_views as TV
import views_batch_restatement as vr
from renderer_amd.pipeline import batch_chunk_bytes, make_frame, make_lod_policy, make_sort_policy

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ra = T.ra   # the module's library fixture
N = 1025
BASE = 0xFFFFFC00   # first_instance_base: the ids wrap


def _scenes(ra):
    """The same resident instances under the two tables: their mesh ids name a mesh of either."""
    s = ra.scene.make_scene(3, n=N, all_visible=True)
    two_pass = lc.table_with_buckets(257, seed=5)
    assert TL._buckets(s["meshes"]) == 200 and TL._buckets(two_pass) == 257 and len(two_pass) <= len(s["meshes"])
    rng = np.random.default_rng(1025)
    s["mesh_id"] = rng.integers(0, len(two_pass), N).astype(np.uint32)
    s["mesh_id"][[0, N - 1]] = (len(two_pass) - 1, 0)   # the last bucket is used, and by the first instance
    return {"one pass": s, "two passes": dict(s, meshes=two_pass)}


def _framed(p, s, call, batch):
    """mip_run, then call(frame, bitmap pointer) with no wait in between; the batch's buffers, the frame's bitmap and model."""
    f = T._Frame(N)
    frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=BASE)
    p.run_device(frame, async_=True, **f.kwargs())
    call(frame, f.bitmap.data_ptr())
    p.wait()
    return batch.result(), f.host_bitmap(), f.model[:N].cpu().numpy()


def _buffers(got):
    return {k: got[k] for k in ("cmds", "ids", "scal", "model") if got[k] is not None}


def _lods(p, s, what, model):
    sw = TL._metric_thresholds(s, lr.RELATIVE)
    b = TL._batch(N, s["meshes"], model=model)
    got, bitmap, frame_model = _framed(p, s, lambda fr, bm_ptr: p.batch_draws_lods(fr, bm_ptr, make_lod_policy(lr.RELATIVE, sw), async_=True, **b.kwargs()), b)
    want = lr.batch_draws_lods(s["pos"], s["scale"], s["mesh_id"], s["meshes"], s["cam_pos"], bitmap, lr.RELATIVE, sw, first_instance_base=BASE, model=frame_model)
    T._check(got, want, what, model_rows=want["model"] if model else None)
    assert want["members"] == N
    return _buffers(got)


def _sorted(p, s, what):
    sw = TL._metric_thresholds(s, lr.DISTANCE)
    b = TS._batch(N)
    sort = (sr.VIEW_AXIS, sr.FAR_FIRST, 32)
    got, bitmap, frame_model = _framed(p, s, lambda fr, bm_ptr: p.batch_draws_sorted(fr, bm_ptr, make_lod_policy(lr.DISTANCE, sw), make_sort_policy(*sort, TS.AXIS),
                                                                                     async_=True, **b.kwargs()), b)
    want = sr.batch_draws_sorted(s["pos"], s["scale"], s["mesh_id"], s["meshes"], s["cam_pos"], bitmap, lr.DISTANCE, sw, *sort, axis=TS.AXIS,
                                 first_instance_base=BASE, model=frame_model)
    T._check(got, want, what, model_rows=want["model"])
    return _buffers(got)


def _ordered(p, s, what):
    sw = TL._metric_thresholds(s, lr.DISTANCE)
    b = TL._batch(N, s["meshes"])
    got, bitmap, frame_model = _framed(p, s, lambda fr, bm_ptr: p.batch_draws_ordered(fr, bm_ptr, make_lod_policy(lr.DISTANCE, sw), orr.FAR_FIRST, async_=True,
                                                                                      **b.kwargs()), b)
    want = orr.batch_draws_ordered(s["pos"], s["scale"], s["mesh_id"], s["meshes"], s["cam_pos"], bitmap, lr.DISTANCE, sw, orr.FAR_FIRST,
                                   first_instance_base=BASE, model=frame_model)
    T._check(got, want, what, model_rows=want["model"])
    return _buffers(got)


def _draws(p, s, what):
    b = T._Batch(N, len(s["meshes"]))
    got, bitmap, frame_model = _framed(p, s, lambda fr, bm_ptr: p.batch_draws(fr, bm_ptr, async_=True, **b.kwargs()), b)
    want = br.batch_draws(s["pos"], s["mesh_id"], s["meshes"], s["cam_pos"], bitmap, first_instance_base=BASE, model=frame_model)
    T._check(got, want, what, model_rows=want["model"])
    return _buffers(got)


class _Chunk:
    def __init__(self, buckets):
        self.words = TM._chunk_buffer(buckets, N)

    def result(self):
        return TM._host(self.words)


def _shard(p, s, what):
    sw = TL._metric_thresholds(s, lr.DISTANCE)
    buckets = TL._buckets(s["meshes"])
    chunk = _Chunk(buckets)
    got, bitmap, _ = _framed(p, s, lambda fr, bm_ptr: p.batch_draws_shard(fr, bm_ptr, make_lod_policy(lr.DISTANCE, sw), chunk.words.data_ptr(), N, async_=True), chunk)
    want = bm.shard_chunk(s["pos"], s["scale"], s["mesh_id"], s["meshes"], s["cam_pos"], bitmap, lr.DISTANCE, sw, BASE, N, fill=TM.SENT,
                          stride_words=batch_chunk_bytes(buckets, N) // 4 + TM.SLACK)
    assert got.tobytes() == want.tobytes(), (what, "chunk", np.nonzero(got != want)[0][:8])
    return {"chunk": got}


def _views(p, s, what, n_views):
    """View v's bitmap: every resident instance (null) for odd v, bits of its own for even v; a camera and a base per view."""
    sw = TL._metric_thresholds(s, lr.DISTANCE)
    rng = np.random.default_rng(n_views)
    cams = TV._cams(s, n_views)
    bases = [(0x40000000 * v + 1000 * v + 7) & 0xFFFFFFFF for v in range(n_views)]
    frames = [make_frame(s["planes"], cams[v], first_instance_base=bases[v]) for v in range(n_views)]
    host = [None if v % 2 else rng.integers(0, 2 ** 32, (N + 31) // 32, dtype=np.uint32) for v in range(n_views)]
    dev = [None if h is None else TV._upload(h) for h in host]
    out = TV._ViewBatch(N, n_views, vr.min_cmd_stride(s["meshes"], N) + 2)
    p.batch_draws_views(frames, [0 if d is None else d.data_ptr() for d in dev], make_lod_policy(lr.DISTANCE, sw), async_=True, **out.kwargs())
    p.wait()
    want = vr.batch_draws_views(s["pos"], s["scale"], s["mesh_id"], s["meshes"], cams, host, bases, lr.DISTANCE, sw)
    assert want["members"] > N * (n_views // 2)
    return out.check(want, what)


# (name, table, call): the order puts every first allocation behind calls that did not need it — the lists, the slot map and the
# bucket map behind a one-pass call; the views' growth behind its first size and in front of a smaller one
STEPS = (
    ("lods, ids only, one pass", "one pass", lambda p, s, w: _lods(p, s, w, model=False)),
    ("sorted, matrices, 32 bits", "one pass", _sorted),
    ("ordered, far first", "one pass", _ordered),
    ("draws, matrices", "two passes", _draws),
    ("shard", "two passes", _shard),
    ("views, 2", "two passes", lambda p, s, w: _views(p, s, w, 2)),
    ("views, 5 (grows)", "two passes", lambda p, s, w: _views(p, s, w, 5)),
    ("views, 2 again (reuses)", "two passes", lambda p, s, w: _views(p, s, w, 2)),
    ("lods, matrices, two passes", "two passes", lambda p, s, w: _lods(p, s, w, model=True)),
)
_fresh = {}


def _fresh_results(ra, scenes):
    """Every step on a context of its own, once: what the steps of a shared context must reproduce."""
    if not _fresh:
        for name, table, step in STEPS:
            with T._pipeline(ra, scenes[table], max_meshes=len(scenes["one pass"]["meshes"])) as p:
                _fresh[name] = step(p, scenes[table], f"fresh context: {name}")
    return _fresh


def _sequence(ra, scenes, steps, frames_in_flight, what):
    """The steps on ONE context, the table changed under the resident instances where a step asks for the other one."""
    want = _fresh_results(ra, scenes)
    table = steps[0][1]
    with T._pipeline(ra, scenes[table], max_meshes=len(scenes["one pass"]["meshes"]), frames_in_flight=frames_in_flight) as p:
        for name, step_table, step in steps:
            if step_table != table:
                table = step_table
                p.set_mesh_table(scenes[table]["meshes"])
            got = step(p, scenes[table], f"{what}: {name}")
            assert got.keys() == want[name].keys(), (what, name)
            for key in got:
                assert got[key].tobytes() == want[name][key].tobytes(), (what, name, key, "differs from the fresh context's")


@pytest.mark.parametrize("frames_in_flight", [1, 2])
def test_one_scratch_serves_every_entry_point_in_turn(ra, frames_in_flight):
    scenes = _scenes(ra)
    _sequence(ra, scenes, STEPS, frames_in_flight, f"forwards, {frames_in_flight} in flight")
    _sequence(ra, scenes, STEPS[::-1], frames_in_flight, f"backwards, {frames_in_flight} in flight")


_ORDER_CHILD = r'''
import os, sys
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
os.environ["MIP_LIBRARY"] = os.path.join(root, "renderer_amd", "lib", "libmi_instance_pipeline_dbg.so")
import renderer_amd
import test_gpu_batch_scratch as S
S._sequence(renderer_amd, S._scenes(renderer_amd), S.STEPS, 2, os.environ.get("MIP_DEBUG_TILE_ORDER"))
print("SCRATCH-OK")
'''


def test_scrambled_dispatch_one_scratch_in_turn():
    e = dict(os.environ, MIP_DEBUG_TILE_ORDER="scramble")
    out = subprocess.run([sys.executable, "-c", _ORDER_CHILD, ROOT], capture_output=True, text=True, timeout=600, env=e)
    assert out.returncode == 0 and "SCRATCH-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
