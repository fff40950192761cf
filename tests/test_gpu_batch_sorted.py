"""Globally depth-sorted batched draws on the GPU (include/mi_instance_pipeline.h, mip_batch_draws_sorted): byte equality with the
numpy restatement (tests/sorted_restatement.py), with mip_batch_draws_ordered on the same context (the RADIAL, 16-bit slots
re-sorted by bucket), with the slot orders and commands written out by hand (tests/sorted_cases.py), and of batch_model with the
`model` of a mip_run of the same context. Every output buffer is sentinel-filled and compared whole. Not reference behaviour."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import lod_cases as lc
import lod_restatement as lr
import order_restatement as orr
import sorted_cases as sc
import sorted_restatement as sr
import test_gpu_batch as T
import test_gpu_batch_lods as TL
import test_gpu_batch_ordered as TO
from renderer_amd.pipeline import make_frame, make_lod_policy, make_sort_policy

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (lr.DISTANCE, lr.RELATIVE)
AXIS = (0.3, -0.2, 0.9)   # not a unit vector
ra = T.ra   # the module's library fixture


def _batch(n, **kw):
    """Device outputs with room for N commands (+ 3 sentinel entries): every member may be a run of its own."""
    return T._Batch(n, max(n, 1), **kw)


def _frame_then_sorted(p, s, mode, sw, metric, order, bits, what, axis=AXIS, base=0, model=True, count=True, bitmap=None, hand=None):
    """mip_run, then mip_batch_draws_sorted over its bitmap with no wait in between (or over `bitmap`, a host array uploaded
    first); the outputs against the restatement (and, with hand = (slots, runs), against the hand-written answer), batch_model
    against the frame's model."""
    import torch

    n = s["n"]
    f = T._Frame(n)
    b = _batch(n, model=model, count=count)
    frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=base)
    given = None
    if bitmap is not None:
        given = torch.from_numpy(np.ascontiguousarray(bitmap).view(np.int32)).to(T._dev())
        torch.cuda.synchronize()
    p.run_device(frame, async_=True, **f.kwargs())
    p.batch_draws_sorted(frame, (given if given is not None else f.bitmap).data_ptr(), make_lod_policy(mode, sw), make_sort_policy(metric, order, bits, axis),
                         async_=True, **b.kwargs())
    p.wait()
    host = f.host_bitmap() if bitmap is None else bitmap
    frame_model = f.model[:n].cpu().numpy() if n else np.zeros((0, 16), np.float32)
    want = sr.batch_draws_sorted(s["pos"], s["scale"], s["mesh_id"], s["meshes"], s["cam_pos"], host, mode, sw, metric, order, bits, axis=axis,
                                 first_instance_base=base, model=frame_model)
    if hand is not None:   # the hand-written answer, not the restatement's
        slots, runs = hand
        slots = np.asarray(list(slots), np.int64)
        assert want["order"].tolist() == slots.tolist(), what
        want = dict(want, cmds=sc.commands(s["meshes"], runs), count=len(runs), members=len(slots), ids=((slots + base) & 0xFFFFFFFF).astype(np.uint32),
                    model=frame_model[slots])
    T._check(b.result(), want, what, model_rows=want["model"] if model else None)
    return want


# ---- 1. the restatement: both metrics x both orders x every key width x both LOD modes, around the rounds and the tiles ----

@pytest.mark.parametrize("bits", sr.DEPTH_BITS)
@pytest.mark.parametrize("order", sr.ORDERS)
@pytest.mark.parametrize("metric", sr.METRICS)
def test_restatement_every_metric_order_and_key_width(ra, metric, order, bits):
    runs = members = 0
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 4097):
        s = TL._sized(ra.scene.make_scene(3, n=max(n, 1)), n)
        with T._pipeline(ra, s) as p:
            for mode in MODES:
                sw = TL._metric_thresholds(s, mode)
                what = f"n={n} mode={mode} metric={metric} order={order} bits={bits}"
                want = _frame_then_sorted(p, s, mode, sw, metric, order, bits, what + ", the frame's bitmap")
                _frame_then_sorted(p, s, mode, sw, metric, order, bits, what + ", ids only", model=False, count=False)
                full = _frame_then_sorted(p, s, mode, sw, metric, order, bits, what + ", every bit, a base that wraps", base=2 ** 32 - 1 - n // 2,
                                          bitmap=lc.all_bits(n))
                if n == 0:
                    assert want["count"] == 0 and want["members"] == 0 and full["count"] == 0
                else:
                    assert full["members"] == n   # (every level of config 3's tables has indices)
                runs, members = runs + full["count"], members + full["members"]
    print(f"metric={metric} order={order} bits={bits}: {members} members -> {runs} runs")   # (reported: DESIGN.md section 24)


# ---- 2. the identity against mip_batch_draws_ordered on the same context ----

@pytest.mark.parametrize("order", sr.ORDERS)
def test_radial_16_resorted_by_bucket_is_batch_draws_ordered(ra, order):
    n = 4097
    s = ra.scene.make_scene(3, n=n)
    base, _ = lr.lod_bases(s["meshes"])
    with T._pipeline(ra, s) as p:
        f = T._Frame(n)
        frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=31)
        p.run_device(frame, **f.kwargs())
        for mode in MODES:
            sw = TL._metric_thresholds(s, mode)
            old, new = TL._batch(n, s["meshes"]), _batch(n)
            p.batch_draws_ordered(frame, f.bitmap.data_ptr(), make_lod_policy(mode, sw), order, **old.kwargs())
            p.batch_draws_sorted(frame, f.bitmap.data_ptr(), make_lod_policy(mode, sw), make_sort_policy(sr.RADIAL, order, 16), **new.kwargs())
            a, b = old.result(), new.result()
            members = int(a["scal"][1])
            assert members > 0 and int(b["scal"][1]) == members and int(b["scal"][0]) > int(a["scal"][0])
            inst = (b["ids"][:members] - np.uint32(31)).astype(np.int64)
            lod = lr.select_lods(s["pos"], s["scale"], s["mesh_id"], s["meshes"], s["cam_pos"], mode, sw)
            bucket = base[s["mesh_id"][inst].astype(np.int64)] + lod[inst]
            assert b["ids"][:members][np.argsort(bucket, kind="stable")].tobytes() == a["ids"][:members].tobytes(), (mode, order)
            assert (b["ids"][members:] == T.SENTINEL).all()


@pytest.mark.parametrize("order", sr.ORDERS)
def test_one_mesh_one_lod_is_batch_draws_ordered_byte_for_byte(ra, order):
    n = 2049
    s = ra.scene.make_scene(3, n=n)
    s["meshes"] = lc.chain_table([1], seed=7)
    s["mesh_id"] = np.zeros(n, np.uint32)
    with T._pipeline(ra, s) as p:
        f = T._Frame(n)
        frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=9)
        p.run_device(frame, **f.kwargs())
        old, new = T._Batch(n, n), _batch(n)   # the same capacities: the buffers are compared whole
        p.batch_draws_ordered(frame, f.bitmap.data_ptr(), make_lod_policy(lr.DISTANCE, lc.SWITCH), order, **old.kwargs())
        p.batch_draws_sorted(frame, f.bitmap.data_ptr(), make_lod_policy(lr.DISTANCE, lc.SWITCH), make_sort_policy(sr.RADIAL, order, 16), **new.kwargs())
        a, b = old.result(), new.result()
        assert int(a["scal"][0]) == 1 and int(a["scal"][1]) > 0
        for key in ("cmds", "ids", "scal", "model"):
            assert a[key].tobytes() == b[key].tobytes(), key


# ---- 3. the run stage: designed runs, every depth tied ----

@pytest.mark.parametrize("name", list(sc.RUN_SCENES))
def test_run_stage_edges(ra, name):
    runs = sc.RUN_SCENES[name]
    s = sc.run_scene(runs)
    s["planes"] = ra.scene.default_planes()
    n = s["n"]
    with T._pipeline(ra, s) as p:
        for metric, order, bits in ((sr.RADIAL, sr.NEAR_FIRST, 16), (sr.VIEW_AXIS, sr.FAR_FIRST, 32)):
            _frame_then_sorted(p, s, lr.DISTANCE, lc.SWITCH, metric, order, bits, f"{name} metric={metric}", axis=(0, 1, 0), base=5, bitmap=lc.all_bits(n),
                               hand=(range(n), sc.want_runs(runs)))


def test_members_only_in_the_last_tile(ra):
    s, bitmap, slots, runs = sc.last_tile_only()
    s["planes"] = ra.scene.default_planes()
    with T._pipeline(ra, s) as p:
        _frame_then_sorted(p, s, lr.DISTANCE, lc.SWITCH, sr.RADIAL, sr.FAR_FIRST, 32, "last tile only", base=5, bitmap=bitmap, hand=(slots, runs))
        none = np.zeros_like(bitmap)   # resident instances, no member: two zeros, nothing else
        want = _frame_then_sorted(p, s, lr.DISTANCE, lc.SWITCH, sr.RADIAL, sr.NEAR_FIRST, 16, "no member", bitmap=none)
        assert want["count"] == 0 and want["members"] == 0


# ---- 4. key edges: the hand-written slot orders and commands ----

@pytest.mark.parametrize("order", sr.ORDERS)
def test_key_edges_on_the_device(ra, order):
    """Every instance is a candidate (a bitmap of ones, uploaded by the test): a frustum would cull the NaN and infinite
    positions whose place in the order is the point."""
    s = sc.radial_scene()
    s["planes"] = ra.scene.default_planes()
    with T._pipeline(ra, s) as p:
        for bits in sr.DEPTH_BITS:
            for mode in MODES:
                _frame_then_sorted(p, s, mode, lc.SWITCH, sr.RADIAL, order, bits, f"radial edges order={order} bits={bits} mode={mode}", base=5,
                                   bitmap=lc.all_bits(s["n"]), hand=sc.RADIAL_WANT[(order, bits)])
        assert p.timings()["general_launches"] > 0   # the non-finite instances put batch_model on the literal path
    s = sc.axis_scene()
    s["planes"] = ra.scene.default_planes()
    with T._pipeline(ra, s) as p:
        for bits in sr.DEPTH_BITS:
            _frame_then_sorted(p, s, lr.DISTANCE, lc.SWITCH, sr.VIEW_AXIS, order, bits, f"axis edges order={order} bits={bits}", axis=sc.VIEW_AXIS_Z, base=5,
                               bitmap=lc.all_bits(s["n"]), hand=sc.AXIS_WANT[(order, bits)])
            _frame_then_sorted(p, s, lr.RELATIVE, lc.SWITCH, sr.VIEW_AXIS, order, bits, f"zero axis order={order} bits={bits}", axis=sc.ZERO_AXIS, base=5,
                               bitmap=lc.all_bits(s["n"]), hand=sc.ZERO_AXIS_WANT[order])


@pytest.mark.parametrize("order", sr.ORDERS)
def test_tied_groups_across_a_round_a_wave_and_a_tile(ra, order):
    s = sc.tie_scene()
    s["planes"] = ra.scene.default_planes()
    with T._pipeline(ra, s) as p:
        for bits in sr.DEPTH_BITS:
            _frame_then_sorted(p, s, lr.DISTANCE, lc.SWITCH, sr.RADIAL, order, bits, f"ties order={order} bits={bits}", base=5, bitmap=lc.all_bits(s["n"]),
                               hand=sc.want_ties(order == sr.NEAR_FIRST))


# ---- 5. bucket counts: no limit from the key ----

@pytest.mark.parametrize("buckets", [1, 257, 65_537])
def test_bucket_counts(ra, buckets):
    s, rng = TO._bucket_scene(ra, buckets)
    with T._pipeline(ra, s) as p:
        for mode, metric, order, bits in ((lr.DISTANCE, sr.RADIAL, sr.NEAR_FIRST, 16), (lr.RELATIVE, sr.VIEW_AXIS, sr.FAR_FIRST, 32)):
            want = _frame_then_sorted(p, s, mode, TL._metric_thresholds(s, mode), metric, order, bits, f"B={buckets} mode={mode} metric={metric}",
                                      base=int(rng.integers(0, 2 ** 32)))
            assert lr.lod_bases(s["meshes"])[1] == buckets and want["members"] > 0 and want["bucket"].max() == buckets - 1
        if buckets > orr.MAX_BUCKETS:   # where mip_batch_draws_ordered refuses
            n = s["n"]
            f, b = T._Frame(n), TL._batch(n, s["meshes"])
            frame = make_frame(s["planes"], s["cam_pos"])
            p.run_device(frame, **f.kwargs())
            with pytest.raises(ra.pipeline.MipError) as e:
                p.batch_draws_ordered(frame, f.bitmap.data_ptr(), make_lod_policy(lr.DISTANCE, lc.SWITCH), orr.NEAR_FIRST, **b.kwargs())
            assert e.value.code == -4   # MIP_ERR_CAPACITY


# ---- 6. any dispatch order (the diagnostic library, a child process); a non-finite scene ----

_SORTED_CHILD = r'''
import os, sys
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
os.environ["MIP_LIBRARY"] = os.path.join(root, "renderer_amd", "lib", "libmi_instance_pipeline_dbg.so")
import numpy as np
import renderer_amd
import sorted_restatement as sr
import test_gpu_batch_lods as TL
import test_gpu_batch_sorted as TS
import test_gpu_batch as T
n = 20_000   # twenty tiles of instances, of slots and (nearly) of commands
s = renderer_amd.scene.make_scene(3, n=n, all_visible=True)
with T._pipeline(renderer_amd, s) as p:
    for mode, metric, order, bits in ((0, sr.RADIAL, sr.NEAR_FIRST, 16), (1, sr.VIEW_AXIS, sr.FAR_FIRST, 32), (0, sr.RADIAL, sr.FAR_FIRST, 24)):
        want = TS._frame_then_sorted(p, s, mode, TL._metric_thresholds(s, mode), metric, order, bits,
                                     f"{os.environ.get('MIP_DEBUG_TILE_ORDER')} mode={mode} metric={metric} order={order} bits={bits}", base=9)
        assert want["count"] > 10_000
print("SORTED-OK")
'''


@pytest.mark.parametrize("tiles", ["reverse", "scramble"])
def test_scrambled_dispatch_batched_draws_sorted(tiles):
    e = dict(os.environ, MIP_DEBUG_TILE_ORDER=tiles)
    out = subprocess.run([sys.executable, "-c", _SORTED_CHILD, ROOT], capture_output=True, text=True, timeout=600, env=e)
    assert out.returncode == 0 and "SORTED-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


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
        for metric in sr.METRICS:
            for order in sr.ORDERS:
                for mode, bits in ((lr.DISTANCE, 16), (lr.RELATIVE, 32)):
                    _frame_then_sorted(p, s, mode, lc.SWITCH, metric, order, bits, f"special_513 metric={metric} order={order} mode={mode}", base=3,
                                       bitmap=lc.all_bits(n))
        assert p.timings()["general_launches"] > 0


# ---- 7. bad arguments with a live context ----

def test_bad_arguments_are_refused_and_leave_the_context_usable(ra):
    L = ra._lib
    s = ra.scene.make_scene(2, n=2000, all_visible=True)
    n = s["n"]
    with ra.InstancePipeline(max_instances=n, max_meshes=len(s["meshes"])) as p:
        lib, ctx = p._lib, p._ctx
        f, b = T._Frame(n), _batch(n)
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

        def sort(metric=sr.VIEW_AXIS, order=sr.NEAR_FIRST, bits=16, axis=AXIS, size=None):
            q = make_sort_policy(metric, order, bits, axis)
            if size is not None:
                q.struct_size = size
            return q

        def call(pol, srt, o):
            return lib.mip_batch_draws_sorted(ctx, C.addressof(frame), f.bitmap.data_ptr(), C.addressof(pol) if pol is not None else None,
                                              C.addressof(srt) if srt is not None else None, C.addressof(o))

        assert call(policy(), sort(), outs()) == -6 and lib.mip_last_error(ctx)       # MIP_ERR_NOT_READY: nothing resident
        p.set_mesh_table(s["meshes"])
        assert call(policy(), sort(), outs()) == -6                                   # a table, no instances
        p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
        p.run_device(frame, **f.kwargs())
        inf, nan = float("inf"), float("nan")
        bad = {"NULL sort": call(policy(), None, outs()), "sort struct_size 24": call(policy(), sort(size=24), outs()),
               "sort struct_size 32": call(policy(), sort(size=32), outs()), "metric 2": call(policy(), sort(metric=2), outs()),
               "metric 0xffffffff": call(policy(), sort(metric=0xFFFFFFFF), outs()), "order DRAW_INDEX": call(policy(), sort(order=0), outs()),
               "order 3": call(policy(), sort(order=3), outs()), "depth_bits 0": call(policy(), sort(bits=0), outs()),
               "depth_bits 8": call(policy(), sort(bits=8), outs()), "depth_bits 20": call(policy(), sort(bits=20), outs()),
               "depth_bits 40": call(policy(), sort(bits=40), outs()), "axis inf": call(policy(), sort(axis=(0, inf, 0)), outs()),
               "axis -inf": call(policy(), sort(axis=(-inf, 0, 1)), outs()), "axis NaN": call(policy(), sort(axis=(0, 0, nan)), outs()),
               "NULL policy": call(None, sort(), outs()), "policy struct_size 24": call(policy(24), sort(), outs()),
               "outputs struct_size 40": call(policy(), sort(), outs(struct_size=40)), "no MIP_OUT_DEVICE": call(policy(), sort(), outs(flags=0)),
               "NULL batch_cmds": call(policy(), sort(), outs(batch_cmds=None))}
        assert all(v == -1 for v in bad.values()), bad
        assert lib.mip_batch_draws_sorted(None, C.addressof(frame), f.bitmap.data_ptr(), C.addressof(policy()), C.addressof(sort()), C.addressof(outs())) == -1
        got = b.result()
        for key in ("cmds", "ids", "scal", "model"):
            assert (got[key] == T.SENTINEL).all(), key   # none of them wrote anything
        assert call(policy(), sort(metric=sr.RADIAL, axis=(nan, inf, 0)), outs()) == 0   # RADIAL ignores the axis
        for metric, order in ((sr.RADIAL, sr.FAR_FIRST), (sr.VIEW_AXIS, sr.NEAR_FIRST)):
            _frame_then_sorted(p, s, lr.DISTANCE, TL._metric_thresholds(s, lr.DISTANCE), metric, order, 24, f"after the refused calls, metric={metric}")


# ---- 8. two frames in flight, each with its own camera, sort and outputs ----

def test_two_frames_in_flight(ra):
    s = ra.scene.make_scene(3, n=30_000, all_visible=True)
    n = s["n"]
    cams = [np.array([0.0, 1.0, 2.0], np.float32), np.array([4.0, 1.0, 30.0], np.float32)]
    sorts = [(sr.RADIAL, sr.FAR_FIRST, 24), (sr.VIEW_AXIS, sr.NEAR_FIRST, 32)]
    sw = TL._metric_thresholds(s, lr.DISTANCE)
    with T._pipeline(ra, s, frames_in_flight=2) as p:
        frames = [T._Frame(n) for _ in cams]
        batches = [_batch(n) for _ in cams]
        for k, cam in enumerate(cams):   # frame k and its batches are enqueued, then frame k + 1 and its batches; nothing waits
            fr = make_frame(s["planes"], cam, first_instance_base=k * 1000)
            p.run_device(fr, async_=True, **frames[k].kwargs())
            p.batch_draws_sorted(fr, frames[k].bitmap.data_ptr(), make_lod_policy(lr.DISTANCE, sw), make_sort_policy(*sorts[k], AXIS), async_=True,
                                 **batches[k].kwargs())
        p.wait()
        seen = set()
        for k, cam in enumerate(cams):
            want = sr.batch_draws_sorted(s["pos"], s["scale"], s["mesh_id"], s["meshes"], cam, frames[k].host_bitmap(), lr.DISTANCE, sw, *sorts[k], axis=AXIS,
                                         first_instance_base=k * 1000, model=frames[k].model[:n].cpu().numpy())
            T._check(batches[k].result(), want, f"frame {k} in flight", model_rows=want["model"])
            seen.add(want["ids"].tobytes())
        assert len(seen) == len(cams)
