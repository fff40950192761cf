"""The designed member streams of the binning stage (tests/batch_stage_cases.py) on the GPU: every case through every entry point
it applies to — mip_batch_draws, _lods (with and without batch_model), _ordered, _sorted, _views and _shard — one context per
table, the host bitmap uploaded by the test. Every output buffer is sentinel-filled and compared whole, byte for byte, with the
expectation BY CONSTRUCTION (from the case's labels; tests/test_batch_stage_cases.py ties it to the numpy restatements and to the
structural model on the CPU); batch_model against the `model` rows of a mip_run of the same context in slot order;
mip_batch_draws_views against one mip_batch_draws_lods call per view. Not reference behaviour."""
import os
import subprocess
import sys

import numpy as np
import pytest

import batch_stage_cases as bc
import test_gpu_batch as T
import test_gpu_batch_views as TV
from renderer_amd.pipeline import batch_chunk_bytes, make_frame, make_lod_policy, make_sort_policy

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLACK = 8
ra = T.ra   # the module's library fixture


def _upload(words):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32)).to(T._dev())
    torch.cuda.synchronize()
    return t


def _host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32)


def _policy():
    return make_lod_policy(bc.DISTANCE, bc.PIN_SWITCH_SQ)


def _frame(ra, case, base=bc.BASE):
    return make_frame(ra.scene.default_planes(), case.cam, first_instance_base=base)


def _batch(case, call):
    """Room for min(B, N) commands (N for the sorted call, where every member may be a run of its own), + 3 sentinel rows."""
    return T._Batch(case.n, case.n if call.entry == "sorted" else (case.n_buckets + 1) // 2, model=call.model)


def _single(p, case, call, frame, bitmap_ptr, b, async_=False):
    kw = dict(async_=async_, **b.kwargs())
    if call.entry == "draws":
        p.batch_draws(frame, bitmap_ptr, **kw)
    elif call.entry == "lods":
        p.batch_draws_lods(frame, bitmap_ptr, _policy(), **kw)
    elif call.entry == "ordered":
        p.batch_draws_ordered(frame, bitmap_ptr, _policy(), call.order, **kw)
    else:
        metric, order, bits, axis = call.sort
        p.batch_draws_sorted(frame, bitmap_ptr, _policy(), make_sort_policy(metric, order, bits, axis), **kw)


def _views(p, ra, case, what):
    """mip_batch_draws_views, every buffer whole; then one mip_batch_draws_lods call per view on the same context."""
    v = case.view_spec()
    V, n, stride = len(v["bucket"]), case.n, case.cmd_stride()
    frames = [_frame(ra, case, base=v["bases"][k]) for k in range(V)]
    bitmaps = [_upload(w) for w in v["bitmaps"]]
    out = TV._ViewBatch(n, V, stride, v["first_slot"])
    p.batch_draws_views(frames, [t.data_ptr() for t in bitmaps], _policy(), **out.kwargs())
    got, want = out.result(), bc.expect_views(case)
    for key in ("counts", "first_slot", "cmds", "ids"):
        assert got[key].tobytes() == want[key].tobytes(), (what, key, np.nonzero(got[key].reshape(-1) != want[key].reshape(-1))[0][:8])
    slot = 0
    for k in range(V):
        b = T._Batch(n, (case.n_buckets + 1) // 2, model=False)
        p.batch_draws_lods(frames[k], bitmaps[k].data_ptr(), _policy(), **b.kwargs())
        one = b.result()
        count, members = int(one["scal"][0]), int(one["scal"][1])
        shifted = one["cmds"][:count].copy()
        shifted[:, 4] += np.uint32(slot)
        assert int(got["counts"][k]) == count, (what, k)
        assert got["cmds"][k * stride: k * stride + count].tobytes() == shifted.tobytes(), (what, k, "commands of mip_batch_draws_lods")
        assert got["ids"][slot: slot + members].tobytes() == one["ids"][:members].tobytes(), (what, k, "ids of mip_batch_draws_lods")
        slot += members
    assert slot == want["members"], what


def _run_case(ra, p, case):
    """The case resident on context p: every call it lists."""
    p.set_instances(case.pos, case.rot, case.scale, case.mesh_id)
    frame = _frame(ra, case)
    bitmap = _upload(case.bitmap)
    frame_model = None
    if any(c.model for c in case.calls):          # the rows batch_model must hold, from a mip_run of the same context
        f = T._Frame(case.n)
        p.run_device(frame, **f.kwargs())
        frame_model = f.model[: case.n].cpu().numpy()
    for call in case.calls:
        what = f"{case.name} {call}"
        if call.entry == "views":
            _views(p, ra, case, what)
        elif call.entry == "shard":
            words = batch_chunk_bytes(case.n_buckets, case.n) // 4
            chunk = _upload(np.full(words + SLACK, bc.SENTINEL, np.uint32))
            p.batch_draws_shard(frame, bitmap.data_ptr(), _policy(), chunk.data_ptr(), case.n)
            got, want = _host(chunk), np.r_[bc.expect(case, call)["chunk"], np.full(SLACK, bc.SENTINEL, np.uint32)]
            assert got.tobytes() == want.tobytes(), (what, np.nonzero(got != want)[0][:8])
        else:
            b = _batch(case, call)
            _single(p, case, call, frame, bitmap.data_ptr(), b)
            want = bc.expect(case, call)
            T._check(b.result(), want, what, model_rows=frame_model[want["order"]] if call.model else None)


def _run_family(ra, family):
    """Every case of the family, one context per table."""
    cases = [c for c in bc.all_cases() if c.family == family]
    assert cases
    for tname in sorted({c.table_name for c in cases}):
        mine = [c for c in cases if c.table_name == tname]
        with ra.InstancePipeline(max_instances=max(c.n for c in mine), max_meshes=len(bc.table(tname))) as p:
            p.set_mesh_table(bc.table(tname))
            for c in mine:
                _run_case(ra, p, c)
    return len(cases)


@pytest.mark.parametrize("family", ["tile", "rowscan", "passes", "writer", "views", "keys"])
def test_designed_streams_by_edge_family(ra, family):
    assert _run_family(ra, family) > 0


@pytest.mark.parametrize("sequence", range(len(bc.SEQUENCES)))
def test_few_members_behind_many_on_one_context(ra, sequence):
    """Two frames in flight; a frame, then a call with many members and one with few on the frame's slot, nothing waits: the list
    buffers of the second call hold the first call's keys past `members`. Checked after one wait at the end."""
    names = bc.SEQUENCES[sequence]
    cases = [bc.case(nm) for nm in names]
    first = cases[0]
    assert all(np.array_equal(c.mesh_id, first.mesh_id) and np.array_equal(c.pos, first.pos) for c in cases)   # one set of instances, five bitmaps
    call = bc.LODS_MODEL
    with ra.InstancePipeline(max_instances=first.n, max_meshes=len(first.table), frames_in_flight=2) as p:
        p.set_mesh_table(first.table)
        p.set_instances(first.pos, first.rot, first.scale, first.mesh_id)
        frame = _frame(ra, first)
        bitmaps = [_upload(c.bitmap) for c in cases]
        order = [0, 1, 2, 3, 4, 1, 0, 3]          # per frame: all then one, 1 025 then none, 1 023 then one, all then none
        frames, batches = [], [_batch(cases[k], call) for k in order]
        for at in range(0, len(order), 2):
            frames.append(T._Frame(first.n))
            p.run_device(frame, async_=True, **frames[-1].kwargs())
            for j in (at, at + 1):
                _single(p, cases[order[j]], call, frame, bitmaps[order[j]].data_ptr(), batches[j], async_=True)
        p.wait()
        frame_model = frames[0].model[: first.n].cpu().numpy()
        for j, k in enumerate(order):
            want = bc.expect(cases[k], call)
            T._check(batches[j].result(), want, f"call {j}: {names[k]}", model_rows=frame_model[want["order"]])


# ---- any dispatch order (the diagnostic library, a child process) ----

_ORDER_CHILD = r'''
import os, sys
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
os.environ["MIP_LIBRARY"] = os.path.join(root, "renderer_amd", "lib", "libmi_instance_pipeline_dbg.so")
import renderer_amd
renderer_amd.load_library()
import test_gpu_batch_stage as S
for family in ("tile", "rowscan", "views"):
    print(family, S._run_family(renderer_amd, family), flush=True)
print("ORDER-OK")
'''


@pytest.mark.parametrize("order", ["reverse", "scramble"])
def test_scrambled_dispatch_batch_stage(order):
    e = dict(os.environ, MIP_DEBUG_TILE_ORDER=order)
    out = subprocess.run([sys.executable, "-c", _ORDER_CHILD, ROOT], capture_output=True, text=True, timeout=600, env=e)
    assert out.returncode == 0 and "ORDER-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
