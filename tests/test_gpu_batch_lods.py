"""Batched draws over the whole LOD chain on the GPU (include/mi_instance_pipeline.h, mip_batch_draws_lods): byte equality with
the numpy restatement (tests/lod_restatement.py), with mip_batch_draws under the pin policy, and of batch_model with the
`model` of a mip_run of the same context. The bitmaps are those of a mip_run of the same context, enqueued in front of the
call with no wait in between, except where a test says otherwise. Not reference behaviour."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import lod_cases as lc
import lod_restatement as lr
import test_gpu_batch as T
from renderer_amd.pipeline import LOD_PIN_SWITCH_SQ, make_frame, make_lod_policy

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (lr.DISTANCE, lr.RELATIVE)
ra = T.ra   # the module's library fixture


def _buckets(meshes):
    return int(meshes["n_lods"].sum())


def _batch(n, meshes, **kw):
    """Device outputs with room for min(B, N) commands (+ 3 sentinel entries), as T._Batch sizes them from 2 m."""
    return T._Batch(n, (_buckets(meshes) + 1) // 2, **kw)


def _metric_thresholds(s, mode, levels=6):
    """Five thresholds at the quantiles of the metric over the scene's instances: every level gets a sixth of them."""
    d = np.asarray(s["cam_pos"], np.float64)[None, :] - s["pos"].astype(np.float64)
    q = (d * d).sum(axis=1)
    if mode == lr.RELATIVE:
        e = (s["meshes"]["aabb_max"].astype(np.float64) - s["meshes"]["aabb_min"].astype(np.float64))[s["mesh_id"]]
        q = q / (s["scale"].astype(np.float64) ** 2 * (e * e).sum(axis=1))
    q = np.sort(q)
    if len(q) < levels:
        return (1.0, 2.0, 3.0, 4.0, 5.0) if mode == lr.DISTANCE else (0.1, 0.2, 0.3, 0.4, 0.5)
    return tuple(float(np.float32(v)) for v in np.maximum.accumulate([q[len(q) * k // levels] for k in range(1, levels)]))


def _frame_then_lods(p, s, mode, sw, what, base=0, model=True, count=True, frame_out=None, bitmap=None):
    """mip_run, then mip_batch_draws_lods over its bitmap with no wait in between (or over `bitmap`, a host array uploaded
    first); the outputs against the restatement, batch_model against the frame's model."""
    import torch

    n = s["n"]
    f = frame_out or T._Frame(n)
    b = _batch(n, s["meshes"], model=model, count=count)
    frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=base)
    given = None
    if bitmap is not None:
        given = torch.from_numpy(np.ascontiguousarray(bitmap).view(np.int32)).to(T._dev())
        torch.cuda.synchronize()
    p.run_device(frame, async_=True, **f.kwargs())
    p.batch_draws_lods(frame, (given if given is not None else f.bitmap).data_ptr(), make_lod_policy(mode, sw), async_=True, **b.kwargs())
    p.wait()
    host = f.host_bitmap() if bitmap is None else bitmap
    frame_model = f.model[:n].cpu().numpy() if n else np.zeros((0, 16), np.float32)
    want = lr.batch_draws_lods(s["pos"], s["scale"], s["mesh_id"], s["meshes"], s["cam_pos"], host, mode, sw, first_instance_base=base,
                               model=frame_model)
    T._check(b.result(), want, what, model_rows=want["model"] if model else None)
    return want


def _sized(s, n):
    for k in ("pos", "rot", "scale", "mesh_id"):
        s[k] = s[k][:n].copy()
    s["n"] = n
    return s


# ---- 1. the pin policy is mip_batch_draws, buffer for buffer ----

@pytest.mark.parametrize("config,n", [(3, 20_000), (2, 4097)])
def test_pin_policy_equals_batch_draws_on_the_device(ra, config, n):
    s = ra.scene.make_scene(config, n=n)
    with T._pipeline(ra, s) as p:
        f = T._Frame(n)
        frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=31)
        old, new = _batch(n, s["meshes"]), _batch(n, s["meshes"])
        p.run_device(frame, async_=True, **f.kwargs())
        p.batch_draws(frame, f.bitmap.data_ptr(), async_=True, **old.kwargs())
        p.batch_draws_lods(frame, f.bitmap.data_ptr(), make_lod_policy(lr.DISTANCE, LOD_PIN_SWITCH_SQ), async_=True, **new.kwargs())
        p.wait()
        a, b = old.result(), new.result()
        assert int(a["scal"][1]) > 0 and int(a["scal"][0]) > 1
        for key in ("cmds", "ids", "scal", "model"):
            assert a[key].tobytes() == b[key].tobytes(), (config, key)
        members = int(a["scal"][1])
        assert a["model"][:members].tobytes() == f.model[:n].cpu().numpy().view(np.uint32)[a["ids"][:members] - 31].tobytes()


# ---- 2. the whole chain, both modes, around the tiles ----

@pytest.mark.parametrize("config", [2, 3])
def test_whole_chain_both_modes(ra, config):
    for n in (0, 1, 63, 65, 1023, 1025, 4097):
        s = _sized(ra.scene.make_scene(config, n=max(n, 1), all_visible=True), n)
        with T._pipeline(ra, s) as p:
            for mode in MODES:
                sw = _metric_thresholds(s, mode)
                want = _frame_then_lods(p, s, mode, sw, f"config {config} n={n} mode={mode}", base=n)
                if n >= 1023:   # the thresholds put members in every level
                    hist = np.bincount(want["lod"][want["order"]], minlength=6)
                    assert (hist > 0).all(), (config, n, mode, hist)
                _frame_then_lods(p, s, mode, sw, f"config {config} n={n} mode={mode}, ids only", base=n, model=False, count=False)
                if n == 0:
                    assert want["count"] == 0 and want["members"] == 0


# ---- 3. bucket counts where the launch plan changes: one pass up to 256, two up to 65 536, three above ----

@pytest.mark.parametrize("buckets", [1, 6, 255, 256, 257, 258, 65_535, 65_536, 65_537, 65_540])
def test_bucket_count_edges(ra, buckets):
    n = 5000
    rng = np.random.default_rng(buckets)
    s = ra.scene.make_scene(3, n=n, all_visible=True)
    s["meshes"] = lc.table_with_buckets(buckets, seed=buckets)
    m = len(s["meshes"])
    s["mesh_id"] = rng.integers(0, m, n).astype(np.uint32)
    s["mesh_id"][rng.integers(0, n, 200)] = m - 1          # the last bucket is used
    s["mesh_id"][rng.integers(0, n, 200)] = 0
    roomy = buckets == 257                                  # one case: a context with room for far more meshes than the table has
    with T._pipeline(ra, s, max_meshes=30_000 if roomy else None) as p:
        for mode in MODES:
            sw = _metric_thresholds(s, mode)
            want = _frame_then_lods(p, s, mode, sw, f"B={buckets} mode={mode}", base=int(rng.integers(0, 2 ** 32)), model=True)
            assert want["count"] <= min(buckets, n)
            lods = want["lod"][want["order"]]
            assert lods.max() == s["meshes"]["n_lods"].max() - 1 and want["members"] > 0


# ---- 4. decision edges: hand-worked scenes on lanes 0 and 63 of a round and on a ragged tile's last instance ----

@pytest.mark.parametrize("mode", MODES)
def test_decision_edges_on_the_device(ra, mode):
    """Every instance is a candidate here (a bitmap of ones, uploaded by the test): a frustum would cull the NaN and infinite
    positions whose LOD is the point. On and one ulp to either side of every switch, scale 0 / negative / subnormal / inf / NaN,
    a NaN in each position component, q overflowing to +inf; the restatement's LODs are checked against the hand-worked ones."""
    s = lc.edge_scene(mode)
    s["planes"] = ra.scene.default_planes()
    n = s["n"]
    with T._pipeline(ra, s) as p:
        for short, sw in ((False, lc.SWITCH), (True, lc.SWITCH_SHORT)):
            want = _frame_then_lods(p, s, mode, sw, f"edges mode={mode} short={short}", base=5, bitmap=lc.all_bits(n))
            assert np.array_equal(want["lod"], lc.want_edge_lods(s, mode, short))
            assert want["members"] == n - int(((s["mesh_id"] == 2) & (want["lod"] == 2)).sum())   # the empty middle level
        assert p.timings()["general_launches"] > 0   # the non-finite instances put batch_model on the literal path


# ---- 5. tables that change under resident instances; updates that move members across levels ----

def test_tables_change_under_resident_instances(ra):
    s = ra.scene.make_scene(3, n=6000, all_visible=True)
    rng = np.random.default_rng(3)
    with T._pipeline(ra, s, max_meshes=64) as p:
        sw = _metric_thresholds(s, lr.DISTANCE)
        first = _frame_then_lods(p, s, lr.DISTANCE, sw, "B = 200")
        assert _buckets(s["meshes"]) == 200
        for n_lods in (1, 6):        # the same meshes with chains of one level (B = 64), then six (B = 384: two passes)
            t = s["meshes"].copy()
            t["n_lods"] = n_lods
            grown = np.arange(6)[None, :] >= s["meshes"]["n_lods"][:, None]
            t["index_len"] = np.where(grown, rng.integers(1, 500, (64, 6)) * 3, t["index_len"])
            t["index_offset"] = np.where(grown, rng.integers(0, 2 ** 31, (64, 6)), t["index_offset"])
            live = np.arange(6)[None, :] < n_lods
            t["index_len"], t["index_offset"] = np.where(live, t["index_len"], 0), np.where(live, t["index_offset"], 0)
            s["meshes"] = t
            p.set_mesh_table(t)      # the instances stay resident
            for mode in MODES:
                want = _frame_then_lods(p, s, mode, _metric_thresholds(s, mode) if mode else sw, f"B = {64 * n_lods} mode={mode}")
                assert want["lod"].max() == n_lods - 1
        # instances 1000 .. 1999 move to twice their distance from the camera: members cross levels
        before = _frame_then_lods(p, s, lr.DISTANCE, sw, "before the update", bitmap=lc.all_bits(6000))
        s["pos"][1000:2000] = (s["cam_pos"] + 2 * (s["pos"][1000:2000] - s["cam_pos"])).astype(np.float32)
        p.update_instances(1000, pos_xyz=s["pos"][1000:2000])
        after = _frame_then_lods(p, s, lr.DISTANCE, sw, "after the update", bitmap=lc.all_bits(6000))
        assert (after["lod"][1000:2000] >= before["lod"][1000:2000]).all() and (after["lod"][1000:2000] > before["lod"][1000:2000]).any()
        assert first["members"] > 0


# ---- 6. two frames in flight, each with its own outputs and policy ----

def test_two_frames_in_flight_with_different_policies(ra):
    s = ra.scene.make_scene(3, n=30_000, all_visible=True)
    n = s["n"]
    cams = [np.array([0.0, 1.0, 2.0], np.float32), np.array([4.0, 1.0, 30.0], np.float32), np.array([-9.0, 2.0, 11.0], np.float32),
            np.array([0.0, 1.0, 2.0], np.float32)]
    policies = [(lr.DISTANCE, _metric_thresholds(s, lr.DISTANCE)), (lr.RELATIVE, _metric_thresholds(s, lr.RELATIVE)),
                (lr.DISTANCE, LOD_PIN_SWITCH_SQ), (lr.RELATIVE, (0.0, 50.0, 50.0, lr.INF, lr.INF))]
    with T._pipeline(ra, s, frames_in_flight=2) as p:
        frames = [T._Frame(n) for _ in cams]
        batches = [_batch(n, s["meshes"]) for _ in cams]
        for k, cam in enumerate(cams):   # frame k and its batches are enqueued, then frame k + 1 and its batches; nothing waits
            fr = make_frame(s["planes"], cam, first_instance_base=k * 1000)
            p.run_device(fr, async_=True, **frames[k].kwargs())
            p.batch_draws_lods(fr, frames[k].bitmap.data_ptr(), make_lod_policy(*policies[k]), async_=True, **batches[k].kwargs())
        p.wait()
        seen = set()
        for k, cam in enumerate(cams):
            want = lr.batch_draws_lods(s["pos"], s["scale"], s["mesh_id"], s["meshes"], cam, frames[k].host_bitmap(), policies[k][0],
                                       policies[k][1], first_instance_base=k * 1000, model=frames[k].model[:n].cpu().numpy())
            T._check(batches[k].result(), want, f"frame {k} in flight", model_rows=want["model"])
            seen.add(want["cmds"].tobytes())
        assert len(seen) == len(cams)


# ---- 7. bad arguments with a live context ----

def test_bad_policies_are_refused_and_leave_the_context_usable(ra):
    L = ra._lib
    s = ra.scene.make_scene(2, n=2000, all_visible=True)
    n = s["n"]
    with T._pipeline(ra, s) as p:
        lib, ctx = p._lib, p._ctx
        f, b = T._Frame(n), _batch(n, s["meshes"])
        frame = make_frame(s["planes"], s["cam_pos"])
        p.run_device(frame, **f.kwargs())
        o = L.MipBatchOutputs()
        o.struct_size = C.sizeof(L.MipBatchOutputs)
        o.flags = L.MIP_OUT_DEVICE
        o.batch_cmds, o.batch_count, o.instance_ids = b.cmds.data_ptr(), b.scal.data_ptr(), b.ids.data_ptr()
        o.instance_count, o.batch_model = b.scal.data_ptr() + 4, b.model.data_ptr()

        def call(policy, fr=frame, bm=f.bitmap.data_ptr(), out=o):
            return lib.mip_batch_draws_lods(ctx, C.addressof(fr) if fr is not None else None, bm, C.addressof(policy) if policy is not None else None,
                                            C.addressof(out) if out is not None else None)

        def policy(sw=lc.SWITCH, mode=lr.DISTANCE, size=None):
            q = make_lod_policy(mode, (0.0,) * 5)
            q.switch_sq[:] = [float(v) for v in sw]   # unchecked: what a C caller could pass
            if size is not None:
                q.struct_size = size
            return q

        nan = float("nan")
        bad = {"NULL policy": call(None), "struct_size 24": call(policy(size=24)), "struct_size 32": call(policy(size=32)),
               "mode 2": call(policy(mode=2)), "mode 0xffffffff": call(policy(mode=0xFFFFFFFF)),
               "decreasing": call(policy((4, 16, 15.999, 256, 1024))), "decreasing from inf": call(policy((4, lr.INF, 1e30, lr.INF, lr.INF))),
               "negative": call(policy((-1e-30, 16, 64, 256, 1024))), "minus inf": call(policy((-lr.INF, 0, 0, 0, 0))),
               "NaN first": call(policy((nan, 16, 64, 256, 1024))), "NaN last": call(policy((4, 16, 64, 256, nan))),
               "NULL frame": call(policy(), fr=None), "NULL bitmap": call(policy(), bm=None), "NULL outputs": call(policy(), out=None)}
        assert all(v == -1 for v in bad.values()), bad
        assert lib.mip_batch_draws_lods(None, C.addressof(frame), f.bitmap.data_ptr(), C.addressof(policy()), C.addressof(o)) == -1
        assert lib.mip_last_error(ctx)
        got = b.result()
        for key in ("cmds", "ids", "scal", "model"):
            assert (got[key] == T.SENTINEL).all(), key   # none of them wrote anything
        # accepted: +inf anywhere from some level on, zeros, equal values; then a good call against the restatement
        assert call(policy((0, 0, 0, 0, 0))) == 0 and call(policy((lr.INF,) * 5)) == 0 and call(policy((-0.0, 7, 7, lr.INF, lr.INF), mode=1)) == 0
        for mode in MODES:
            _frame_then_lods(p, s, mode, _metric_thresholds(s, mode), f"after the refused calls, mode={mode}")


# ---- 8. any dispatch order (the diagnostic library, a child process) ----

_ORDER_CHILD = r'''
import os, sys
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
os.environ["MIP_LIBRARY"] = os.path.join(root, "renderer_amd", "lib", "libmi_instance_pipeline_dbg.so")
import numpy as np
import renderer_amd
import lod_cases as lc
import test_gpu_batch as T
import test_gpu_batch_lods as TL
rng = np.random.default_rng(12)
for n, buckets in ((50_000, 200), (20_000, 258)):   # one pass; two passes (the matrices by the kernel of their own)
    s = renderer_amd.scene.make_scene(3, n=n, all_visible=True)
    if buckets != 200:
        s["meshes"] = lc.table_with_buckets(buckets)
        s["mesh_id"] = rng.integers(0, len(s["meshes"]), n).astype(np.uint32)
    assert TL._buckets(s["meshes"]) == buckets
    with T._pipeline(renderer_amd, s) as p:
        for mode in TL.MODES:
            TL._frame_then_lods(p, s, mode, TL._metric_thresholds(s, mode), f"{os.environ.get('MIP_DEBUG_TILE_ORDER')} n={n} B={buckets} mode={mode}", base=9)
print("ORDER-OK")
'''


@pytest.mark.parametrize("order", ["reverse", "scramble"])
def test_scrambled_dispatch_batched_draws_lods(order):
    e = dict(os.environ, MIP_DEBUG_TILE_ORDER=order)
    out = subprocess.run([sys.executable, "-c", _ORDER_CHILD, ROOT], capture_output=True, text=True, timeout=600, env=e)
    assert out.returncode == 0 and "ORDER-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
