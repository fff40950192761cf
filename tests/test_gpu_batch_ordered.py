"""Depth-ordered batched draws on the GPU (include/mi_instance_pipeline.h, mip_batch_draws_ordered): byte equality with
mip_batch_draws_lods (DRAW_INDEX in every buffer; commands and counts under any order), with the numpy restatement
(tests/order_restatement.py), with the slot orders written out by hand (tests/order_cases.py), and of batch_model with the
`model` of a mip_run of the same context. Not reference behaviour."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import lod_cases as lc
import lod_restatement as lr
import order_cases as oc
import order_restatement as orr
import test_gpu_batch as T
import test_gpu_batch_lods as TL
from renderer_amd.pipeline import LOD_PIN_SWITCH_SQ, make_frame, make_lod_policy

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (lr.DISTANCE, lr.RELATIVE)
ORDERS = (orr.NEAR_FIRST, orr.FAR_FIRST)
ra = T.ra   # the module's library fixture


def _frame_then_ordered(p, s, mode, sw, order, what, base=0, model=True, count=True, bitmap=None, want_slots=None):
    """mip_run, then mip_batch_draws_ordered over its bitmap with no wait in between (or over `bitmap`, a host array uploaded
    first); the outputs against the restatement, batch_model against the frame's model."""
    import torch

    n = s["n"]
    f = T._Frame(n)
    b = TL._batch(n, s["meshes"], model=model, count=count)
    frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=base)
    given = None
    if bitmap is not None:
        given = torch.from_numpy(np.ascontiguousarray(bitmap).view(np.int32)).to(T._dev())
        torch.cuda.synchronize()
    p.run_device(frame, async_=True, **f.kwargs())
    p.batch_draws_ordered(frame, (given if given is not None else f.bitmap).data_ptr(), make_lod_policy(mode, sw), order, async_=True, **b.kwargs())
    p.wait()
    host = f.host_bitmap() if bitmap is None else bitmap
    frame_model = f.model[:n].cpu().numpy() if n else np.zeros((0, 16), np.float32)
    want = orr.batch_draws_ordered(s["pos"], s["scale"], s["mesh_id"], s["meshes"], s["cam_pos"], host, mode, sw, order,
                                   first_instance_base=base, model=frame_model)
    if want_slots is not None:   # the hand-written order, not the restatement's
        assert want["order"].tolist() == want_slots.tolist(), what
        want["ids"] = ((want_slots + base) & 0xFFFFFFFF).astype(np.uint32)
        want["model"] = frame_model[want_slots]
    T._check(b.result(), want, what, model_rows=want["model"] if model else None)
    return want


# ---- 1. the pin: DRAW_INDEX is mip_batch_draws_lods, buffer for buffer; no order changes commands or counts ----

@pytest.mark.parametrize("config,n", [(3, 20_000), (2, 4097)])
def test_draw_index_is_batch_draws_lods_and_orders_keep_commands(ra, config, n):
    s = ra.scene.make_scene(config, n=n)
    with T._pipeline(ra, s) as p:
        f = T._Frame(n)
        frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=31)
        p.run_device(frame, **f.kwargs())
        for what, mode, sw in (("pin", lr.DISTANCE, LOD_PIN_SWITCH_SQ), ("six levels", lr.RELATIVE, TL._metric_thresholds(s, lr.RELATIVE))):
            policy = make_lod_policy(mode, sw)
            old = TL._batch(n, s["meshes"])
            p.batch_draws_lods(frame, f.bitmap.data_ptr(), policy, **old.kwargs())
            a = old.result()
            assert int(a["scal"][1]) > 0 and int(a["scal"][0]) > 1
            members = int(a["scal"][1])
            for order in orr.ORDERS:
                new = TL._batch(n, s["meshes"])
                p.batch_draws_ordered(frame, f.bitmap.data_ptr(), policy, order, **new.kwargs())
                b = new.result()
                for key in ("cmds", "scal") + (("ids", "model") if order == orr.DRAW_INDEX else ()):
                    assert a[key].tobytes() == b[key].tobytes(), (config, what, order, key)
                if order != orr.DRAW_INDEX:
                    assert a["ids"].tobytes() != b["ids"].tobytes(), (config, what, order)
                    assert np.array_equal(np.sort(a["ids"][:members]), np.sort(b["ids"][:members]))
                    assert (b["ids"][members:] == T.SENTINEL).all() and (b["model"][members:] == T.SENTINEL).all()
                assert b["model"][:members].tobytes() == f.model[:n].cpu().numpy().view(np.uint32)[b["ids"][:members] - 31].tobytes()


# ---- 2. the restatement: both LOD modes x both orders, around the rounds and the tiles ----

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("order", ORDERS)
def test_restatement_both_modes_both_orders(ra, mode, order):
    for n in (0, 1, 63, 65, 1023, 1024, 1025, 4097):
        visible = ra.scene.make_scene(3, n=max(n, 1), all_visible=True)
        culled = ra.scene.make_scene(3, n=max(n, 1))
        for s, name in ((TL._sized(visible, n), "all visible"), (TL._sized(culled, n), "the frame's bitmap")):
            with T._pipeline(ra, s) as p:
                sw = TL._metric_thresholds(s, mode)
                what = f"n={n} mode={mode} order={order} {name}"
                want = _frame_then_ordered(p, s, mode, sw, order, what, base=n + 7)
                _frame_then_ordered(p, s, mode, sw, order, what + ", ids only", base=n + 7, model=False, count=False)
                if n == 0:
                    assert want["count"] == 0 and want["members"] == 0
                if name == "all visible" and n:
                    assert want["members"] == n    # the member list crosses the list passes' tile at 1 024 / 1 025


# ---- 3. bucket counts: three passes, four passes, a key that uses all 32 bits; capacity ----

def _bucket_scene(ra, buckets, n=5000):
    rng = np.random.default_rng(buckets)
    s = ra.scene.make_scene(3, n=n, all_visible=True)
    s["meshes"] = lc.table_with_buckets(buckets, seed=buckets)
    m = len(s["meshes"])
    s["mesh_id"] = rng.integers(0, m, n).astype(np.uint32)
    s["mesh_id"][rng.integers(0, n, 200)] = m - 1          # the last bucket is used
    s["mesh_id"][rng.integers(0, n, 200)] = 0
    return s, rng


@pytest.mark.parametrize("buckets", [1, 255, 256, 257, 65_535, 65_536])
def test_bucket_count_edges(ra, buckets):
    s, rng = _bucket_scene(ra, buckets)
    with T._pipeline(ra, s) as p:
        for mode, order in ((lr.DISTANCE, orr.NEAR_FIRST), (lr.RELATIVE, orr.FAR_FIRST), (lr.DISTANCE, orr.FAR_FIRST)):
            # thresholds that put members into the last level of the last mesh: the last bucket is used
            sw = TL._metric_thresholds(s, mode)
            want = _frame_then_ordered(p, s, mode, sw, order, f"B={buckets} mode={mode} order={order}", base=int(rng.integers(0, 2 ** 32)))
            base, b_total = lr.lod_bases(s["meshes"])
            assert b_total == buckets and want["members"] > 0
            used = base[s["mesh_id"][want["order"]].astype(np.int64)] + want["lod"][want["order"]]
            assert used.max() == buckets - 1, "the last bucket has members"


def test_more_buckets_than_the_key_holds(ra):
    s, rng = _bucket_scene(ra, 65_537)
    n = s["n"]
    with T._pipeline(ra, s) as p:
        f, b = T._Frame(n), TL._batch(n, s["meshes"])
        frame = make_frame(s["planes"], s["cam_pos"])
        p.run_device(frame, **f.kwargs())
        sw = TL._metric_thresholds(s, lr.DISTANCE)
        for order in ORDERS:
            with pytest.raises(ra.pipeline.MipError) as e:
                p.batch_draws_ordered(frame, f.bitmap.data_ptr(), make_lod_policy(lr.DISTANCE, sw), order, **b.kwargs())
            assert e.value.code == -4   # MIP_ERR_CAPACITY
        got = b.result()
        for key in ("cmds", "ids", "scal", "model"):
            assert (got[key] == T.SENTINEL).all(), key
        p.batch_draws_ordered(frame, f.bitmap.data_ptr(), make_lod_policy(lr.DISTANCE, sw), orr.DRAW_INDEX, **b.kwargs())
        want = lr.batch_draws_lods(s["pos"], s["scale"], s["mesh_id"], s["meshes"], s["cam_pos"], f.host_bitmap(), lr.DISTANCE, sw,
                                   model=f.model[:n].cpu().numpy())
        T._check(b.result(), want, "B = 65 537, DRAW_INDEX", model_rows=want["model"])


# ---- 4. decision edges: the hand-written slot orders ----

@pytest.mark.parametrize("order", ORDERS)
def test_decision_edges_on_the_device(ra, order):
    """Every instance is a candidate (a bitmap of ones, uploaded by the test): a frustum would cull the NaN and infinite
    positions whose place in the order is the point."""
    near = order == orr.NEAR_FIRST
    for name, s, slots in (("edges", oc.edge_scene(), oc.want_edge_slots(near)), ("ties", oc.tie_scene(), oc.want_tie_slots(near))):
        s["planes"] = ra.scene.default_planes()
        with T._pipeline(ra, s) as p:
            for mode in MODES:
                _frame_then_ordered(p, s, mode, lc.SWITCH, order, f"{name} mode={mode} order={order}", base=5, bitmap=lc.all_bits(s["n"]),
                                    want_slots=slots)
            if name == "edges":
                assert p.timings()["general_launches"] > 0   # the non-finite instances put batch_model on the literal path


@pytest.mark.parametrize("order", ORDERS)
def test_one_bucket_two_depths_in_one_wave_round(ra, order):
    """order_cases.digit_scene: 64 instances of one two-level mesh, two members of bucket 1 whose keys differ only in the lowest
    digit and a member of bucket 0 that shares that digit with one of them. The two commands hold 62 and 2 members only if the
    count of pass 0 indexes its per-bucket histogram by key >> 16."""
    s = oc.digit_scene()
    s["planes"] = ra.scene.default_planes()
    slots = oc.want_digit_slots(order == orr.NEAR_FIRST)
    with T._pipeline(ra, s) as p:
        for mode in MODES:
            want = _frame_then_ordered(p, s, mode, lc.SWITCH, order, f"digit mode={mode} order={order}", base=5, bitmap=lc.all_bits(s["n"]),
                                       want_slots=slots)
            assert want["cmds"]["instanceCount"].tolist() == list(oc.DIGIT_COUNTS) and want["cmds"]["firstInstance"].tolist() == [0, 62]


# ---- 5. any dispatch order (the diagnostic library, a child process); a non-finite scene ----

_ORDER_CHILD = r'''
import os, sys
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
os.environ["MIP_LIBRARY"] = os.path.join(root, "renderer_amd", "lib", "libmi_instance_pipeline_dbg.so")
import numpy as np
import renderer_amd
import order_restatement as orr
import test_gpu_batch_lods as TL
import test_gpu_batch_ordered as TO
import test_gpu_batch as T
n = 20_000   # twenty tiles, B = 200: three passes
s = renderer_amd.scene.make_scene(3, n=n, all_visible=True)
with T._pipeline(renderer_amd, s) as p:
    for mode, order in ((0, orr.NEAR_FIRST), (1, orr.FAR_FIRST)):
        TO._frame_then_ordered(p, s, mode, TL._metric_thresholds(s, mode), order, f"{os.environ.get('MIP_DEBUG_TILE_ORDER')} mode={mode} order={order}", base=9)
print("ORDER-OK")
'''


@pytest.mark.parametrize("tiles", ["reverse", "scramble"])
def test_scrambled_dispatch_batched_draws_ordered(tiles):
    e = dict(os.environ, MIP_DEBUG_TILE_ORDER=tiles)
    out = subprocess.run([sys.executable, "-c", _ORDER_CHILD, ROOT], capture_output=True, text=True, timeout=600, env=e)
    assert out.returncode == 0 and "ORDER-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


def test_non_finite_instances_general_matrices(ra):
    """special_513's instances (tests/golden: special values in every column): the `general` matrix arithmetic of batch_model
    is the frame's `model`, whatever slot a member lands in."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "special_513.npz"))
    s = dict(pos=g["pos"], rot=g["rot"], scale=g["scale"], mesh_id=g["mesh_id"], meshes=g["meshes"], planes=g["planes"], cam_pos=g["cam_pos"],
             n=len(g["scale"]))
    n = s["n"]
    assert n == 513 and not np.isfinite(s["pos"]).all()
    with T._pipeline(ra, s) as p:
        p.reset_timings()
        for order in ORDERS:
            for mode in MODES:
                _frame_then_ordered(p, s, mode, lc.SWITCH, order, f"special_513 mode={mode} order={order}", base=3, bitmap=lc.all_bits(n))
        assert p.timings()["general_launches"] > 0


# ---- 6. bad arguments with a live context ----

def test_bad_arguments_are_refused_and_leave_the_context_usable(ra):
    L = ra._lib
    s = ra.scene.make_scene(2, n=2000, all_visible=True)
    n = s["n"]
    with ra.InstancePipeline(max_instances=n, max_meshes=len(s["meshes"])) as p:
        lib, ctx = p._lib, p._ctx
        f, b = T._Frame(n), TL._batch(n, s["meshes"])
        frame = make_frame(s["planes"], s["cam_pos"])

        def outs(**kw):
            o = L.MipBatchOutputs()
            o.struct_size = C.sizeof(L.MipBatchOutputs)
            o.flags = L.MIP_OUT_DEVICE
            o.batch_cmds, o.batch_count, o.instance_ids = b.cmds.data_ptr(), b.scal.data_ptr(), b.ids.data_ptr()
            o.instance_count, o.batch_model = b.scal.data_ptr() + 4, b.model.data_ptr()
            for k, v in kw.items():
                setattr(o, k, v)
            return o

        def policy(size=None):
            q = make_lod_policy(lr.DISTANCE, lc.SWITCH)
            if size is not None:
                q.struct_size = size
            return q

        def call(pol, order, o):
            return lib.mip_batch_draws_ordered(ctx, C.addressof(frame), f.bitmap.data_ptr(), C.addressof(pol) if pol is not None else None, order,
                                               C.addressof(o))

        assert call(policy(), orr.NEAR_FIRST, outs()) == -6 and lib.mip_last_error(ctx)       # MIP_ERR_NOT_READY: nothing resident
        p.set_mesh_table(s["meshes"])
        assert call(policy(), orr.FAR_FIRST, outs()) == -6                                    # a table, no instances
        p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
        p.run_device(frame, **f.kwargs())
        bad = {"order 3": call(policy(), 3, outs()), "order 0xffffffff": call(policy(), 0xFFFFFFFF, outs()),
               "NULL policy": call(None, orr.NEAR_FIRST, outs()), "NULL policy, draw index": call(None, orr.DRAW_INDEX, outs()),
               "policy struct_size 24": call(policy(24), orr.NEAR_FIRST, outs()), "outputs struct_size 40": call(policy(), orr.FAR_FIRST, outs(struct_size=40)),
               "no MIP_OUT_DEVICE": call(policy(), orr.NEAR_FIRST, outs(flags=0)), "only MIP_OUT_ASYNC": call(policy(), orr.FAR_FIRST, outs(flags=L.MIP_OUT_ASYNC))}
        assert all(v == -1 for v in bad.values()), bad
        assert lib.mip_batch_draws_ordered(None, C.addressof(frame), f.bitmap.data_ptr(), C.addressof(policy()), 1, C.addressof(outs())) == -1
        got = b.result()
        for key in ("cmds", "ids", "scal", "model"):
            assert (got[key] == T.SENTINEL).all(), key   # none of them wrote anything
        for order in ORDERS:
            _frame_then_ordered(p, s, lr.DISTANCE, TL._metric_thresholds(s, lr.DISTANCE), order, f"after the refused calls, order={order}")


# ---- 7. two frames in flight, each with its own camera, order and outputs ----

def test_two_frames_in_flight(ra):
    s = ra.scene.make_scene(3, n=30_000, all_visible=True)
    n = s["n"]
    cams = [np.array([0.0, 1.0, 2.0], np.float32), np.array([4.0, 1.0, 30.0], np.float32)]
    sw = TL._metric_thresholds(s, lr.DISTANCE)
    with T._pipeline(ra, s, frames_in_flight=2) as p:
        frames = [T._Frame(n) for _ in cams]
        batches = [TL._batch(n, s["meshes"]) for _ in cams]
        for k, cam in enumerate(cams):   # frame k and its batches are enqueued, then frame k + 1 and its batches; nothing waits
            fr = make_frame(s["planes"], cam, first_instance_base=k * 1000)
            p.run_device(fr, async_=True, **frames[k].kwargs())
            p.batch_draws_ordered(fr, frames[k].bitmap.data_ptr(), make_lod_policy(lr.DISTANCE, sw), ORDERS[k], async_=True, **batches[k].kwargs())
        p.wait()
        seen = set()
        for k, cam in enumerate(cams):
            want = orr.batch_draws_ordered(s["pos"], s["scale"], s["mesh_id"], s["meshes"], cam, frames[k].host_bitmap(), lr.DISTANCE, sw, ORDERS[k],
                                           first_instance_base=k * 1000, model=frames[k].model[:n].cpu().numpy())
            T._check(batches[k].result(), want, f"frame {k} in flight", model_rows=want["model"])
            seen.add(want["ids"].tobytes())
        assert len(seen) == len(cams)
