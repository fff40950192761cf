"""Batched draws for several views in one call on the GPU (include/mi_instance_pipeline.h, mip_batch_draws_views): byte
equality of every output buffer, whole and sentinel-filled before the call, with the numpy restatement
(tests/views_batch_restatement.py) AND with one mip_batch_draws_lods call per view on the same library. Bitmaps come from a
mip_run_views of the same frames, enqueued in front of the call with no wait in between, from a NULL entry (every resident
instance) or from one bitmap two views share. Not reference behaviour."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import lod_cases as lc
import lod_restatement as lr
import test_gpu_batch as T
import test_gpu_batch_lods as TL
import views_batch_restatement as vr
from renderer_amd.pipeline import make_frame, make_lod_policy

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (lr.DISTANCE, lr.RELATIVE)
SENTINEL = T.SENTINEL
PAD = 3
ra = T.ra   # the module's library fixture


def _full(*shape):
    import torch

    return torch.full(shape, T._i32(SENTINEL), dtype=torch.int32, device=T._dev())


class _ViewBatch:
    """Device outputs of mip_batch_draws_views, every word a sentinel, PAD entries behind each."""

    def __init__(self, n, n_views, stride, first_slot=True):
        self.cmds, self.counts = _full(n_views * stride + PAD, 5), _full(n_views + PAD)
        self.ids, self.slots = _full(n_views * n + PAD), _full(n_views + 1 + PAD)
        self.n, self.stride, self.first_slot = n, stride, first_slot

    def kwargs(self):
        return dict(batch_cmds=self.cmds.data_ptr(), cmd_stride=self.stride, batch_counts=self.counts.data_ptr(),
                    instance_ids=self.ids.data_ptr(), view_first_slot=self.slots.data_ptr() if self.first_slot else 0)

    def result(self):
        import torch

        torch.cuda.synchronize()
        u = lambda t: t.cpu().numpy().view(np.uint32)   # noqa: E731
        return dict(cmds=u(self.cmds), counts=u(self.counts), ids=u(self.ids), first_slot=u(self.slots))

    def check(self, want, what):
        """Every buffer whole against the restatement's: what is written, and the sentinel everywhere else."""
        got, full = self.result(), vr.fill_outputs(want, self.n, self.stride, SENTINEL, PAD, first_slot=self.first_slot)
        for key in ("counts", "first_slot", "cmds", "ids"):
            assert got[key].tobytes() == full[key].tobytes(), (what, key)
        return got

    def untouched(self):
        got = self.result()
        return all((got[k] == SENTINEL).all() for k in got)


def _frusta(planes, n_views):
    """A frustum per view: the scene's own, and the same one turned about the axes (columns swapped, signs flipped)."""
    base = np.asarray(planes, np.float32).reshape(6, 4)
    turns = [(0, 1, 2, 1, 1), (2, 1, 0, 1, 1), (0, 1, 2, -1, 1), (2, 1, 0, -1, 1), (0, 2, 1, 1, 1), (0, 1, 2, 1, -1)]
    out = []
    for v in range(n_views):
        a, b, c, sx, sz = turns[v % len(turns)]
        t = base[:, [a, b, c, 3]].copy()
        t[:, 0] *= sx
        t[:, 2] *= sz
        out.append(np.ascontiguousarray(t.reshape(-1)))
    return out


def _cams(s, n_views):
    rng = np.random.default_rng(n_views)
    return [(np.asarray(s["cam_pos"], np.float32) + (rng.normal(0, 15, 3) if v else 0)).astype(np.float32) for v in range(n_views)]


def _upload(words):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).to(T._dev())
    torch.cuda.synchronize()
    return t


def _views_call(p, s, n_views, mode, sw, what, kinds=("culled", "null", "shared"), stride_extra=0, first_slot=True, lods_too=True,
                given=None):
    """mip_run_views over the views that take a culled bitmap, then — with no wait — mip_batch_draws_views over all of them.
    View v's bitmap is kinds[v % len(kinds)]: "culled" (its own view of mip_run_views), "null" (every resident instance),
    "shared" (view 0's pointer, with view v's own camera), "given" (given[v], uploaded and synchronised first).
    The outputs against the restatement, whole; then against one mip_batch_draws_lods call per view."""
    import torch

    n = s["n"]
    cams, frusta = _cams(s, n_views), _frusta(s["planes"], n_views)
    bases = [(0x40000000 * v + 1000 * v + 7) & 0xFFFFFFFF for v in range(n_views)]
    frames = [make_frame(frusta[v], cams[v], first_instance_base=bases[v]) for v in range(n_views)]
    kind = [kinds[v % len(kinds)] for v in range(n_views)]
    assert "shared" not in kind or kind[0] == "culled"
    words = (max(n, 1) + 31) // 32
    culled = [v for v in range(n_views) if kind[v] == "culled"]
    bitmaps = torch.zeros((n_views, words), dtype=torch.int32, device=T._dev())
    draw = torch.zeros((max(len(culled), 1), max(n, 1), 5), dtype=torch.int32, device=T._dev())
    scal = torch.zeros((n_views, 2), dtype=torch.int32, device=T._dev())
    uploaded = {v: _upload(given[v]) for v in range(n_views) if kind[v] == "given"}
    ptrs = [bitmaps[v].data_ptr() if kind[v] == "culled" else bitmaps[0].data_ptr() if kind[v] == "shared"
            else uploaded[v].data_ptr() if kind[v] == "given" else 0 for v in range(n_views)]
    stride = vr.min_cmd_stride(s["meshes"], n) + stride_extra
    out = _ViewBatch(n, n_views, stride, first_slot)
    policy = make_lod_policy(mode, sw)
    torch.cuda.synchronize()
    if n and culled:
        prepared = [p.prepare_outputs(visible_bitmap=bitmaps[v].data_ptr(), draw_cmds=draw[k].data_ptr(), draw_count=scal[v].data_ptr(),
                                      draw_index_total=scal[v].data_ptr() + 4) for k, v in enumerate(culled)]
        p.run_views([frames[v] for v in culled], prepared)          # asynchronous: prepare_outputs sets MIP_OUT_ASYNC
    p.batch_draws_views(frames, ptrs, policy, async_=True, **out.kwargs())
    p.wait()
    host = bitmaps.cpu().numpy().view(np.uint32)
    host_bm = [None if kind[v] == "null" else host[0] if kind[v] == "shared" else given[v] if kind[v] == "given" else host[v]
               for v in range(n_views)]
    want = vr.batch_draws_views(s["pos"], s["scale"], s["mesh_id"], s["meshes"], cams, host_bm, bases, mode, sw)
    got = out.check(want, what)
    if lods_too:   # V separate mip_batch_draws_lods calls on the same build
        ones = _upload(lc.all_bits(n))
        slot = 0
        for v in range(n_views):
            b = TL._batch(n, s["meshes"], model=False)
            p.batch_draws_lods(frames[v], ptrs[v] or ones.data_ptr(), policy, **b.kwargs())
            one = b.result()
            count, members = int(one["scal"][0]), int(one["scal"][1])
            assert int(got["counts"][v]) == count and slot == int(want["first_slot"][v]), (what, v)
            shifted = one["cmds"][:count].copy()
            shifted[:, 4] += np.uint32(slot)
            assert got["cmds"][v * stride: v * stride + count].tobytes() == shifted.tobytes(), (what, v, "commands of mip_batch_draws_lods")
            assert got["ids"][slot: slot + members].tobytes() == one["ids"][:members].tobytes(), (what, v, "ids of mip_batch_draws_lods")
            slot += members
        assert slot == want["members"]
    return want


def _scene(ra, n, table=None, seed=0, config=3):
    s = TL._sized(ra.scene.make_scene(config, n=max(n, 1)), n)
    if table is not None:
        s["meshes"] = table
        rng = np.random.default_rng(seed + n)
        s["mesh_id"] = rng.integers(0, len(table), n).astype(np.uint32)
        if n > 2:
            s["mesh_id"][[0, n - 1]] = (len(table) - 1, 0)     # the first and the last bucket are used
    return s


# ---- 1. instance counts around the waves and tiles x view counts, both modes, every kind of bitmap ----

SIZES = (0, 1, 63, 64, 65, 1000, 1023, 1024, 1025, 4097)


@pytest.mark.parametrize("n_views", [1, 2, 3, 5, 16])
def test_sizes_and_view_counts_against_restatement_and_separate_calls(ra, n_views):
    """B = 200 (config 3's table): one pass for one view, two passes from two views on; B = 17: one pass up to 15 views, two
    for 16. N = 1 000 with three views puts a view boundary inside a tile of entries."""
    small = lc.chain_table([6, 3, 1, 5, 2], seed=4)
    members = 0
    for n in SIZES:
        for table in (None, small):
            s = _scene(ra, n, table)
            with T._pipeline(ra, s) as p:
                for mode in MODES:
                    sw = TL._metric_thresholds(s, mode)
                    want = _views_call(p, s, n_views, mode, sw, f"V={n_views} n={n} B={TL._buckets(s['meshes'])} mode={mode}")
                    members += want["members"]
                    if n == 0:
                        assert want["members"] == 0 and (want["counts"] == 0).all() and (want["first_slot"] == 0).all()
                    if n >= 1000 and n_views >= 3:   # views 0 and 2 share a bitmap pointer and differ by their cameras
                        assert (want["lod"][0] != want["lod"][2]).any()
                        assert want["cmds"][0].tobytes() != want["cmds"][2].tobytes()
    assert members > 0


# ---- 2. global bucket counts n_views x B where the launch plan changes, at small N ----

@pytest.mark.parametrize("n_views,n_lods", [(5, [1] * 51), (3, [1] * 85), (16, [1] * 16), (2, [1] * 128), (1, [1] * 257), (2, [1] * 129),
                                            (16, [1] * 4096), (16, [1] * 4097), (2, [6] * 21), (3, [6] * 15), (16, [6] * 683)])
def test_pass_boundaries(ra, n_views, n_lods):
    """One-level tables with n_views x B = 255, 255, 256, 256, 257, 258; sixteen views of 4 096 / 4 097 buckets (65 536: two
    passes, 65 552: three); six-level tables with 252 (one pass), 270 (two) and 65 568 (three) global buckets."""
    n = 3000
    s = _scene(ra, n, lc.chain_table(n_lods, seed=len(n_lods)), seed=n_views)
    with T._pipeline(ra, s) as p:
        for mode in MODES:
            sw = TL._metric_thresholds(s, mode)
            want = _views_call(p, s, n_views, mode, sw, f"V={n_views} B={len(n_lods)}x{n_lods[0]} mode={mode}", lods_too=n_views <= 5)
            assert want["members"] > 0 and want["lod"].max() == n_lods[0] - 1
            for v in range(1, n_views, 3):   # the unculled views draw instance 0's mesh, the last of the table: the view's last bucket
                assert want["cmds"][v]["firstIndex"][-1] in s["meshes"]["index_offset"][-1]


# ---- 3. edge cases ----

def test_empty_views_and_command_strides(ra):
    n = 1000
    s = _scene(ra, n, lc.chain_table([6, 3, 1, 5, 2], seed=4))
    zero, rng = np.zeros((n + 31) // 32, np.uint32), np.random.default_rng(1)
    some = [rng.integers(0, 1 << 32, (n + 31) // 32, dtype=np.uint64).astype(np.uint32) for _ in range(3)]
    sw = TL._metric_thresholds(s, lr.DISTANCE)
    with T._pipeline(ra, s) as p:
        # a view with no members between two that have some: n = 1 000, three views, a view boundary inside a tile
        want = _views_call(p, s, 3, lr.DISTANCE, sw, "empty view in the middle", kinds=("given",), given=[some[0], zero, some[1]])
        assert want["counts"][1] == 0 and want["counts"][0] > 0 and want["counts"][2] > 0
        assert want["first_slot"][1] == want["first_slot"][2] > 0
        # the first and the last view empty
        want = _views_call(p, s, 4, lr.RELATIVE, TL._metric_thresholds(s, lr.RELATIVE), "empty views at both ends", kinds=("given",),
                           given=[zero, some[0], some[2], zero])
        assert want["counts"].tolist()[0] == 0 and want["counts"].tolist()[3] == 0 and want["members"] > 0
        # all views empty
        for n_views in (1, 5):
            want = _views_call(p, s, n_views, lr.DISTANCE, sw, "all views empty", kinds=("given",), given=[zero] * n_views)
            assert want["members"] == 0 and (want["counts"] == 0).all()
        # cmd_stride == min(B, N) (every other test) and larger; view_first_slot not asked for
        for extra, first_slot in ((1, True), (40, False)):
            want = _views_call(p, s, 5, lr.DISTANCE, sw, f"cmd_stride + {extra}", stride_extra=extra, first_slot=first_slot, lods_too=first_slot)
            assert want["members"] > 0
    # N < B: cmd_stride = N
    s = _scene(ra, 9, lc.chain_table([6, 3, 1, 5, 2], seed=4))
    assert vr.min_cmd_stride(s["meshes"], 9) == 9
    with T._pipeline(ra, s) as p:
        _views_call(p, s, 3, lr.DISTANCE, TL._metric_thresholds(s, lr.DISTANCE), "N < B", kinds=("null",))


def test_a_larger_call_grows_the_scratch_and_a_smaller_one_reuses_it(ra):
    s = _scene(ra, 5000, lc.chain_table([6] * 50, seed=2))
    sw = TL._metric_thresholds(s, lr.DISTANCE)
    with T._pipeline(ra, s) as p:
        for n_views in (1, 4, 16, 2):   # one pass, then two with ever more entries and buckets, then fewer again
            _views_call(p, s, n_views, lr.DISTANCE, sw, f"scratch, V={n_views}", lods_too=False)


# ---- 4. two frames in flight and a mip_batch_draws_lods call behind slot 1, interleaved ----

def test_two_frames_in_flight_interleaved_with_batch_draws_lods(ra):
    import torch

    s = _scene(ra, 20_000)
    n, n_views = s["n"], 4
    sw = TL._metric_thresholds(s, lr.DISTANCE)
    policy = make_lod_policy(lr.DISTANCE, sw)
    cams, bases = _cams(s, n_views), [11, 22, 33, 44]
    with T._pipeline(ra, s, frames_in_flight=2) as p:
        frames = [T._Frame(n) for _ in range(3)]
        batches = [TL._batch(n, s["meshes"], model=False) for _ in range(3)]
        outs = [_ViewBatch(n, n_views, vr.min_cmd_stride(s["meshes"], n)) for _ in range(2)]
        vframes = [make_frame(s["planes"], cams[v], first_instance_base=bases[v]) for v in range(n_views)]
        fcams = [np.array([0.0, 1.0, 2.0], np.float32), np.array([4.0, 1.0, 30.0], np.float32), np.array([-9.0, 2.0, 11.0], np.float32)]
        torch.cuda.synchronize()
        for k in range(3):   # frame k (slots 0, 1, 0) and its batches, a views call after frames 0 and 1; nothing waits
            fr = make_frame(s["planes"], fcams[k], first_instance_base=k * 1000)
            p.run_device(fr, async_=True, **frames[k].kwargs())
            p.batch_draws_lods(fr, frames[k].bitmap.data_ptr(), policy, async_=True, **batches[k].kwargs())
            if k < 2:
                p.batch_draws_views(vframes, [0] * n_views, policy, async_=True, **outs[k].kwargs())
        p.wait()
        for k in range(3):
            want = lr.batch_draws_lods(s["pos"], s["scale"], s["mesh_id"], s["meshes"], fcams[k], frames[k].host_bitmap(), lr.DISTANCE, sw,
                                       first_instance_base=k * 1000)
            T._check(batches[k].result(), want, f"mip_batch_draws_lods behind frame {k}")
        want = vr.batch_draws_views(s["pos"], s["scale"], s["mesh_id"], s["meshes"], cams, [None] * n_views, bases, lr.DISTANCE, sw)
        for k in range(2):
            outs[k].check(want, f"views call {k} between frames in flight")


# ---- 5. refused arguments: status codes, and every output still a sentinel ----

def test_refused_arguments_write_nothing_and_leave_the_context_usable(ra):
    L = ra._lib
    s = _scene(ra, 2000, lc.chain_table([6, 3, 1, 5, 2], seed=4))
    n, n_views = s["n"], 3
    stride = vr.min_cmd_stride(s["meshes"], n)
    with T._pipeline(ra, s) as p:
        lib, ctx = p._lib, p._ctx
        out = _ViewBatch(n, n_views, stride)
        frames = (L.MipFrame * n_views)()
        for v in range(n_views):
            C.memmove(C.addressof(frames[v]), C.addressof(make_frame(s["planes"], s["cam_pos"], first_instance_base=v)), C.sizeof(L.MipFrame))
        bitmaps = (C.c_void_p * n_views)(None, None, None)
        good_policy = make_lod_policy(lr.DISTANCE, lc.SWITCH)

        def outputs(**kw):
            o = L.MipViewBatchOutputs()
            o.struct_size, o.flags = C.sizeof(L.MipViewBatchOutputs), L.MIP_OUT_DEVICE
            o.batch_cmds, o.cmd_stride, o.batch_counts = out.cmds.data_ptr(), stride, out.counts.data_ptr()
            o.instance_ids, o.view_first_slot = out.ids.data_ptr(), out.slots.data_ptr()
            for k, v in kw.items():
                setattr(o, k, v)
            return o

        def call(o=None, policy=good_policy, fr=frames, bm=bitmaps, views=n_views, context=ctx):
            o = outputs() if o is None else o
            addr = lambda x: C.addressof(x) if x is not None else None   # noqa: E731
            return lib.mip_batch_draws_views(context, addr(fr), addr(bm), views, addr(policy), addr(o) if o != "null" else None)

        def policy(sw=lc.SWITCH, mode=lr.DISTANCE, size=None):
            q = make_lod_policy(mode, (0.0,) * 5)
            q.switch_sq[:] = [float(v) for v in sw]
            if size is not None:
                q.struct_size = size
            return q

        bad = {"NULL ctx": call(context=None), "NULL frames": call(fr=None), "NULL bitmaps": call(bm=None), "NULL policy": call(policy=None),
               "NULL out": call(o="null"), "NULL batch_cmds": call(outputs(batch_cmds=None)), "NULL batch_counts": call(outputs(batch_counts=None)),
               "NULL instance_ids": call(outputs(instance_ids=None)), "struct_size 40": call(outputs(struct_size=40)),
               "struct_size 56": call(outputs(struct_size=56)), "reserved": call(outputs(reserved=1)), "unknown flag": call(outputs(flags=L.MIP_OUT_DEVICE | 0x4000)),
               "no MIP_OUT_DEVICE": call(outputs(flags=0)), "zero views": call(views=0), "seventeen views": call(views=17),
               "cmd_stride short": call(outputs(cmd_stride=stride - 1)), "cmd_stride 0": call(outputs(cmd_stride=0)),
               "policy size": call(policy=policy(size=24)), "policy mode": call(policy=policy(mode=2)),
               "policy decreasing": call(policy=policy((4, 16, 15.999, 256, 1024))), "policy NaN": call(policy=policy((float("nan"), 16, 64, 256, 1024))),
               "policy negative": call(policy=policy((-1.0, 16, 64, 256, 1024)))}
        assert all(v == -1 for v in bad.values()), bad
        assert lib.mip_last_error(ctx)
        assert out.untouched()
        # MIP_ERR_NOT_READY: a context without instances
        with ra.InstancePipeline(max_instances=16, max_meshes=4) as q:
            assert call(context=q._ctx) == -6 and out.untouched()
        # accepted afterwards, against the restatement
        _views_call(p, s, n_views, lr.DISTANCE, TL._metric_thresholds(s, lr.DISTANCE), "after the refused calls")


# ---- 6. any dispatch order (the diagnostic library, a child process) ----

_ORDER_CHILD = r'''
import os, sys
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
os.environ["MIP_LIBRARY"] = os.path.join(root, "renderer_amd", "lib", "libmi_instance_pipeline_dbg.so")
import renderer_amd
import lod_cases as lc
import test_gpu_batch as T
import test_gpu_batch_lods as TL
import test_gpu_batch_views as TV
order = os.environ.get("MIP_DEBUG_TILE_ORDER")
for n, n_lods, n_views in ((20_000, [6, 3, 1, 5, 2], 5), (9_000, [6] * 43, 3), (3_000, [1] * 4097, 16)):   # one, two and three passes
    s = TV._scene(renderer_amd, n, lc.chain_table(n_lods, seed=7))
    with T._pipeline(renderer_amd, s) as p:
        for mode in TV.MODES:
            TV._views_call(p, s, n_views, mode, TL._metric_thresholds(s, mode), f"{order} n={n} V={n_views} mode={mode}", lods_too=False)
print("ORDER-OK")
'''


@pytest.mark.parametrize("order", ["reverse", "scramble"])
def test_scrambled_dispatch_batched_draws_views(order):
    e = dict(os.environ, MIP_DEBUG_TILE_ORDER=order)
    out = subprocess.run([sys.executable, "-c", _ORDER_CHILD, ROOT], capture_output=True, text=True, timeout=600, env=e)
    assert out.returncode == 0 and "ORDER-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
