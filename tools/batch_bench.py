#!/usr/bin/env python3
"""GPU time of the batched-draws stage (mip_batch_draws) beside the frame it follows: HIP events on the launch stream around
BATCH back-to-back repetitions, median of samples, one JSON line per leg.

  (a) mip_run with every output of the flagship frame (model, bitmap, commands, count, index total): the yardstick
  (b) mip_run with model = NULL  +  mip_batch_draws with batch_model
  (c) (a)  +  mip_batch_draws with ids only
  (s) mip_batch_draws alone, ids only / with batch_model (over the bitmap of (a))
  (copy) a device-to-device copy of 256 MB: the measured ceiling the fractions refer to
  (m) mip_batch_draws alone over a table of 300 meshes at 100 k instances: 600 buckets, the several-pass path (a (key,
      instance) list, the per-bucket histogram, the matrices through slot_of), ids only / with batch_model

  python tools/batch_bench.py [n ...] [--samples 40] [--out profiles/batch_draws_bench.jsonl]

--lods: the LOD-chain stage (mip_batch_draws_lods) alone, over the bitmap of (a), beside mip_batch_draws on the same scene:
the pin policy (the same buckets and outputs as mip_batch_draws), a DISTANCE and a RELATIVE policy that use every level, each
with ids only and with batch_model.

  python tools/batch_bench.py --lods [--out profiles/batch_draws_lods_bench.jsonl]

--ordered: the depth-ordered stage (mip_batch_draws_ordered, NEAR_FIRST and FAR_FIRST) beside mip_batch_draws_lods of the same
build under the two example policies, each with ids only and with batch_model.

  python tools/batch_bench.py --ordered [--out profiles/batch_draws_ordered_bench.jsonl]

--views: mip_batch_draws_views for V = 4 views in one call beside its yardsticks of the same session: four
mip_batch_draws_lods calls (one per view, back to back, no wait in between: the bitmaps are at rest here, which favours the
four calls — behind a mip_run_views the caller would have to wait first) and, for the unculled case, mip_light_draw_lists
with four lights. Culled bitmaps come from one mip_run_views of the four frames; the unculled case passes NULL bitmaps
(a bitmap of ones to mip_batch_draws_lods). A library without the entry point (the parent commit's) runs the yardsticks only.

  python tools/batch_bench.py --views [--out profiles/batch_draws_views_bench.jsonl]

--sharded: batched draws of a sharded scene on ONE GPU: the scene as 8 contiguous shards (config 3 at 1 M, config 2 at 100 k;
culled by the scene's frustum, and unculled), every shard's chunk written straight into the receive buffer. Times
mip_batch_draws_shard beside mip_batch_draws_lods on the same shard, and mip_merge_batches beside two yardsticks of the same
process: a device-to-device copy of the same members x 4 bytes, and mip_merge_wire_lists_packed over the same frame's eight
draw lists. No all-gather is timed: no box with more than one GPU.

  python tools/batch_bench.py --sharded [--out profiles/batch_merge_bench.jsonl]

--sorted: the globally depth-sorted stage (mip_batch_draws_sorted, FAR_FIRST: RADIAL at 16, 24 and 32 key bits, VIEW_AXIS at 32)
beside mip_batch_draws_ordered FAR_FIRST of the same build and policy, each with ids only and with batch_model. The run stage
alone is not a leg: its four kernels are read from a kernel trace of this leg (rocprofv3 --kernel-trace --stats).

  python tools/batch_bench.py --sorted [--out profiles/batch_sorted_bench.jsonl]

--parent-library PATH (any of the first four): the SAME legs on another build of the library (the parent commit's) as the yardstick,
in the same session. A library is loaded once per process, so the tool then only starts children of itself, one after the
other: the parent build, this build, the parent build again. Every row says which (`library`); the two parent runs give each
leg's noise band: the larger of the difference of its two parent medians and its parent p90 - median."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TBS = 8.0  # MI355X HBM3E


def measure(st, fn, batch=20, samples=40, warm=3):
    import numpy as np
    import torch

    for _ in range(warm * batch):
        fn()
    st.synchronize()
    out = []
    for _ in range(samples):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(batch):
            fn()
        e1.record(st)
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / batch * 1e3)
    us = np.array(out)
    return dict(median_us=round(float(np.median(us)), 3), min_us=round(float(us.min()), 3), p90_us=round(float(np.percentile(us, 90)), 3))


def bench(n, emit, samples=40, library="this build"):
    import numpy as np
    import torch

    import renderer_amd
    from renderer_amd import scene
    from renderer_amd.pipeline import make_frame

    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream()
    config = 2 if n <= 100_000 else 3
    s = scene.make_scene(config, n=n)
    m = len(s["meshes"])
    with torch.cuda.stream(st):
        p = renderer_amd.InstancePipeline(n, m, stream=st.cuda_stream)
        p.set_mesh_table(s["meshes"])
        p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
        model = torch.empty((n, 16), dtype=torch.float32, device=dev)
        bitmap = torch.zeros((n + 31) // 32 + 1, dtype=torch.int32, device=dev)
        cmds = torch.empty((n, 5), dtype=torch.int32, device=dev)
        scal = torch.zeros(8, dtype=torch.int32, device=dev)
        b_cmds = torch.empty((2 * m, 5), dtype=torch.int32, device=dev)
        b_ids = torch.empty(n, dtype=torch.int32, device=dev)
        b_scal = torch.zeros(8, dtype=torch.int32, device=dev)
        b_model = torch.empty((n, 16), dtype=torch.float32, device=dev)
        src = torch.empty(64 << 20, dtype=torch.int32, device=dev)
        dst = torch.empty_like(src)
        torch.cuda.synchronize()
        frame = p.frame_ref(make_frame(s["planes"], s["cam_pos"]))
        common = dict(visible_bitmap=bitmap.data_ptr(), draw_cmds=cmds.data_ptr(), draw_count=scal.data_ptr(), draw_index_total=scal.data_ptr() + 4)
        full = p.prepare_outputs(model=model.data_ptr(), **common)
        no_model = p.prepare_outputs(**common)
        ids_only = dict(batch_cmds=b_cmds.data_ptr(), batch_count=b_scal.data_ptr(), instance_ids=b_ids.data_ptr(),
                        instance_count=b_scal.data_ptr() + 4, async_=True)
        with_model = dict(ids_only, batch_model=b_model.data_ptr())

        def leg_a():
            p.run_prepared(frame, full)

        def leg_b():
            p.run_prepared(frame, no_model)
            p.batch_draws(frame, bitmap.data_ptr(), **with_model)

        def leg_c():
            p.run_prepared(frame, full)
            p.batch_draws(frame, bitmap.data_ptr(), **ids_only)

        leg_a()
        p.wait()
        copy = measure(st, lambda: dst.copy_(src), batch=5, samples=20)
        copy_tbs = 2 * src.numel() * 4 / 1e6 / copy["median_us"]
        emit(dict(leg="copy", library=library, bytes=2 * src.numel() * 4, tb_per_s=round(copy_tbs, 3), **copy))
        legs = [("a: mip_run, every output", leg_a, None), ("b: mip_run without model + batch_draws with batch_model", leg_b, None),
                ("c: mip_run, every output + batch_draws ids only", leg_c, None),
                ("s: batch_draws ids only, alone", lambda: p.batch_draws(frame, bitmap.data_ptr(), **ids_only), False),
                ("s: batch_draws with batch_model, alone", lambda: p.batch_draws(frame, bitmap.data_ptr(), **with_model), True)]
        for name, fn, stage_model in legs:
            r = measure(st, fn, samples=samples)
            p.wait()
            draws, batches, members = int(scal[0].item()), int(b_scal[0].item()), int(b_scal[1].item())
            row = dict(leg=name, library=library, n=n, config=config, meshes=m, draw_count=draws, batch_count=batches, members=members, **r)
            if stage_model is not None:  # the stage's algorithmic bytes (one pass): bitmap + mesh_id + pos read, ids written; rot + scale read, matrices written
                v = members / n
                per_instance = 0.125 + 16 + 4 * v + ((20 + 64 * v) if stage_model else 0)
                tbs = per_instance * n / 1e6 / r["median_us"]
                row.update(member_fraction=round(v, 4), algorithmic_bytes_per_instance=round(per_instance, 2), tb_per_s=round(tbs, 3),
                           of_peak=round(tbs / PEAK_TBS, 3), of_copy=round(tbs / copy_tbs, 3))
            emit(row)
        p.close()


def bench_several(emit, samples=40, library="this build", n=100_000, m=300):
    """Leg (m): a table of m > 128 meshes, built as tests/test_gpu_batch.py builds its many-mesh scenes."""
    import numpy as np
    import torch

    import renderer_amd
    from renderer_amd import scene
    from renderer_amd.pipeline import MESH_DTYPE, make_frame

    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream()
    rng = np.random.default_rng(m)
    s = scene.make_scene(3, n=n, all_visible=True)
    meshes = np.zeros(m, MESH_DTYPE)
    meshes["aabb_min"], meshes["aabb_max"] = -0.5, 0.5
    meshes["n_lods"] = rng.integers(1, 4, m)
    meshes["index_len"] = rng.integers(0, 3000, (m, 6)) // 3 * 3
    meshes["index_len"][rng.random((m, 6)) < 0.1] = 0
    meshes["index_offset"] = rng.integers(0, 2 ** 31, (m, 6))
    meshes["vertex_offset"] = rng.integers(-1000, 2 ** 30, m)
    mesh_id = rng.integers(0, m, n).astype(np.uint32)
    mesh_id[rng.integers(0, n, n // 8)] = m - 1   # the last bucket is used
    with torch.cuda.stream(st):
        p = renderer_amd.InstancePipeline(n, m, stream=st.cuda_stream)
        p.set_mesh_table(meshes)
        p.set_instances(s["pos"], s["rot"], s["scale"], mesh_id)
        bitmap = torch.zeros((n + 31) // 32 + 1, dtype=torch.int32, device=dev)
        cmds = torch.empty((n, 5), dtype=torch.int32, device=dev)
        scal = torch.zeros(8, dtype=torch.int32, device=dev)
        b_cmds = torch.empty((2 * m, 5), dtype=torch.int32, device=dev)
        b_ids = torch.empty(n, dtype=torch.int32, device=dev)
        b_scal = torch.zeros(8, dtype=torch.int32, device=dev)
        b_model = torch.empty((n, 16), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        frame = p.frame_ref(make_frame(s["planes"], s["cam_pos"]))
        p.run_prepared(frame, p.prepare_outputs(visible_bitmap=bitmap.data_ptr(), draw_cmds=cmds.data_ptr(), draw_count=scal.data_ptr(),
                                                draw_index_total=scal.data_ptr() + 4))
        p.wait()
        ids_only = dict(batch_cmds=b_cmds.data_ptr(), batch_count=b_scal.data_ptr(), instance_ids=b_ids.data_ptr(),
                        instance_count=b_scal.data_ptr() + 4, async_=True)
        with_model = dict(ids_only, batch_model=b_model.data_ptr())
        for outs, what in ((ids_only, "ids only"), (with_model, "with batch_model")):
            r = measure(st, lambda: p.batch_draws(frame, bitmap.data_ptr(), **outs), samples=samples)
            p.wait()
            emit(dict(leg=f"m: batch_draws {what}, {m} meshes (several passes)", library=library, n=n, config=3, meshes=m, buckets=2 * m,
                      batch_count=int(b_scal[0].item()), members=int(b_scal[1].item()), **r))
        p.close()


# example policies of the --lods leg (squared metrics): every level of a six-level chain is used in configs 2 and 3
LODS_DISTANCE_SQ = (100.0, 400.0, 1600.0, 3600.0, 6400.0)   # switches at 10, 20, 40, 60, 80 units
LODS_RELATIVE_SQ = (9.0, 36.0, 144.0, 400.0, 900.0)         # switches at 3, 6, 12, 20, 30 box diagonals


def bench_lods(n, emit, samples=40, library="this build"):
    import torch

    import renderer_amd
    from renderer_amd import scene
    from renderer_amd.pipeline import make_frame

    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream()
    config = 2 if n <= 100_000 else 3
    s = scene.make_scene(config, n=n)
    m = len(s["meshes"])
    buckets = int(s["meshes"]["n_lods"].sum())
    with torch.cuda.stream(st):
        p = renderer_amd.InstancePipeline(n, m, stream=st.cuda_stream)
        p.set_mesh_table(s["meshes"])
        p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
        bitmap = torch.zeros((n + 31) // 32 + 1, dtype=torch.int32, device=dev)
        cmds = torch.empty((n, 5), dtype=torch.int32, device=dev)
        scal = torch.zeros(8, dtype=torch.int32, device=dev)
        b_cmds = torch.empty((max(2 * m, buckets), 5), dtype=torch.int32, device=dev)
        b_ids = torch.empty(n, dtype=torch.int32, device=dev)
        b_scal = torch.zeros(8, dtype=torch.int32, device=dev)
        b_model = torch.empty((n, 16), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        frame = p.frame_ref(make_frame(s["planes"], s["cam_pos"]))
        p.run_prepared(frame, p.prepare_outputs(visible_bitmap=bitmap.data_ptr(), draw_cmds=cmds.data_ptr(), draw_count=scal.data_ptr(),
                                                draw_index_total=scal.data_ptr() + 4))
        p.wait()
        ids_only = dict(batch_cmds=b_cmds.data_ptr(), batch_count=b_scal.data_ptr(), instance_ids=b_ids.data_ptr(),
                        instance_count=b_scal.data_ptr() + 4, async_=True)
        with_model = dict(ids_only, batch_model=b_model.data_ptr())
        from renderer_amd.pipeline import LOD_PIN_SWITCH_SQ, make_lod_policy

        legs = [("batch_draws", None), ("batch_draws_lods, pin policy", make_lod_policy("distance", LOD_PIN_SWITCH_SQ)),
                ("batch_draws_lods, DISTANCE", make_lod_policy("distance", LODS_DISTANCE_SQ)),
                ("batch_draws_lods, RELATIVE", make_lod_policy("relative", LODS_RELATIVE_SQ))]
        for name, policy in legs:
            for outs, what in ((ids_only, "ids only"), (with_model, "with batch_model")):
                if policy is None:
                    fn = lambda: p.batch_draws(frame, bitmap.data_ptr(), **outs)
                else:
                    fn = lambda: p.batch_draws_lods(frame, bitmap.data_ptr(), policy, **outs)
                r = measure(st, fn, samples=samples)
                p.wait()
                emit(dict(leg=f"lods: {name}, {what}", library=library, n=n, config=config, meshes=m, buckets=2 * m if policy is None else buckets,
                          batch_count=int(b_scal[0].item()), members=int(b_scal[1].item()), **r))
        p.close()


def bench_ordered(n, emit, samples=40, library="this build"):
    import torch

    import renderer_amd
    from renderer_amd import _lib, scene
    from renderer_amd.pipeline import make_frame, make_lod_policy

    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream()
    config = 2 if n <= 100_000 else 3
    s = scene.make_scene(config, n=n)
    m = len(s["meshes"])
    buckets = int(s["meshes"]["n_lods"].sum())
    with torch.cuda.stream(st):
        p = renderer_amd.InstancePipeline(n, m, stream=st.cuda_stream)
        p.set_mesh_table(s["meshes"])
        p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
        bitmap = torch.zeros((n + 31) // 32 + 1, dtype=torch.int32, device=dev)
        cmds = torch.empty((n, 5), dtype=torch.int32, device=dev)
        scal = torch.zeros(8, dtype=torch.int32, device=dev)
        b_cmds = torch.empty((buckets, 5), dtype=torch.int32, device=dev)
        b_ids = torch.empty(n, dtype=torch.int32, device=dev)
        b_scal = torch.zeros(8, dtype=torch.int32, device=dev)
        b_model = torch.empty((n, 16), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        frame = p.frame_ref(make_frame(s["planes"], s["cam_pos"]))
        p.run_prepared(frame, p.prepare_outputs(visible_bitmap=bitmap.data_ptr(), draw_cmds=cmds.data_ptr(), draw_count=scal.data_ptr(),
                                                draw_index_total=scal.data_ptr() + 4))
        p.wait()
        ids_only = dict(batch_cmds=b_cmds.data_ptr(), batch_count=b_scal.data_ptr(), instance_ids=b_ids.data_ptr(),
                        instance_count=b_scal.data_ptr() + 4, async_=True)
        with_model = dict(ids_only, batch_model=b_model.data_ptr())
        orders = [("batch_draws_lods", None), ("batch_draws_ordered NEAR_FIRST", _lib.MIP_BATCH_ORDER_NEAR_FIRST),
                  ("batch_draws_ordered FAR_FIRST", _lib.MIP_BATCH_ORDER_FAR_FIRST)]
        for pname, policy in (("DISTANCE", make_lod_policy("distance", LODS_DISTANCE_SQ)), ("RELATIVE", make_lod_policy("relative", LODS_RELATIVE_SQ))):
            for name, order in orders:
                for outs, what in ((ids_only, "ids only"), (with_model, "with batch_model")):
                    if order is None:
                        fn = lambda: p.batch_draws_lods(frame, bitmap.data_ptr(), policy, **outs)
                    else:
                        fn = lambda: p.batch_draws_ordered(frame, bitmap.data_ptr(), policy, order, **outs)
                    r = measure(st, fn, samples=samples)
                    p.wait()
                    emit(dict(leg=f"ordered: {name}, {pname}, {what}", library=library, n=n, config=config, meshes=m, buckets=buckets,
                              batch_count=int(b_scal[0].item()), members=int(b_scal[1].item()), **r))
        p.close()


def bench_sorted(n, emit, samples=40, library="this build"):
    import numpy as np
    import torch

    import renderer_amd
    from renderer_amd import _lib, scene
    from renderer_amd.pipeline import make_frame, make_lod_policy, make_sort_policy

    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream()
    config = 2 if n <= 100_000 else 3
    s = scene.make_scene(config, n=n)
    m = len(s["meshes"])
    buckets = int(s["meshes"]["n_lods"].sum())
    with torch.cuda.stream(st):
        p = renderer_amd.InstancePipeline(n, m, stream=st.cuda_stream)
        p.set_mesh_table(s["meshes"])
        p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
        bitmap = torch.zeros((n + 31) // 32 + 1, dtype=torch.int32, device=dev)
        cmds = torch.empty((n, 5), dtype=torch.int32, device=dev)
        scal = torch.zeros(8, dtype=torch.int32, device=dev)
        b_cmds = torch.empty((n, 5), dtype=torch.int32, device=dev)   # a run per member at worst
        b_ids = torch.empty(n, dtype=torch.int32, device=dev)
        b_scal = torch.zeros(8, dtype=torch.int32, device=dev)
        b_model = torch.empty((n, 16), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        frame = p.frame_ref(make_frame(s["planes"], s["cam_pos"]))
        p.run_prepared(frame, p.prepare_outputs(visible_bitmap=bitmap.data_ptr(), draw_cmds=cmds.data_ptr(), draw_count=scal.data_ptr(),
                                                draw_index_total=scal.data_ptr() + 4))
        p.wait()
        ids_only = dict(batch_cmds=b_cmds.data_ptr(), batch_count=b_scal.data_ptr(), instance_ids=b_ids.data_ptr(),
                        instance_count=b_scal.data_ptr() + 4, async_=True)
        with_model = dict(ids_only, batch_model=b_model.data_ptr())
        policy = make_lod_policy("distance", LODS_DISTANCE_SQ)
        far = _lib.MIP_BATCH_ORDER_FAR_FIRST
        axis = -np.asarray(s["cam_pos"], np.float32)   # towards the origin of the scene
        legs = [("batch_draws_ordered FAR_FIRST", None)]
        legs += [(f"batch_draws_sorted FAR_FIRST RADIAL {bits} bits", make_sort_policy("radial", far, bits)) for bits in (16, 24, 32)]
        legs += [("batch_draws_sorted FAR_FIRST VIEW_AXIS 32 bits", make_sort_policy("view_axis", far, 32, axis))]
        for name, sort in legs:
            for outs, what in ((ids_only, "ids only"), (with_model, "with batch_model")):
                if sort is None:
                    fn = lambda: p.batch_draws_ordered(frame, bitmap.data_ptr(), policy, far, **outs)
                else:
                    fn = lambda: p.batch_draws_sorted(frame, bitmap.data_ptr(), policy, sort, **outs)
                r = measure(st, fn, samples=samples)
                p.wait()
                emit(dict(leg=f"sorted: {name}, DISTANCE, {what}", library=library, n=n, config=config, meshes=m, buckets=buckets,
                          batch_count=int(b_scal[0].item()), members=int(b_scal[1].item()), **r))
        p.close()


def view_frusta(planes, n_views):
    """A frustum per view: the scene's own and the same one turned about the axes (columns swapped, signs flipped)."""
    import numpy as np

    base = np.asarray(planes, np.float32).reshape(6, 4)
    turns = [(0, 1, 2, 1, 1), (2, 1, 0, 1, 1), (0, 1, 2, -1, 1), (2, 1, 0, -1, 1)]
    out = []
    for v in range(n_views):
        a, b, c, sx, sz = turns[v % len(turns)]
        t = base[:, [a, b, c, 3]].copy()
        t[:, 0] *= sx
        t[:, 2] *= sz
        out.append(np.ascontiguousarray(t.reshape(-1)))
    return out


def bench_views(n, emit, samples=40, library="this build", n_views=4):
    import numpy as np
    import torch

    import renderer_amd
    from renderer_amd import scene
    from renderer_amd.pipeline import make_frame, make_lod_policy

    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream()
    config = 2 if n <= 100_000 else 3
    s = scene.make_scene(config, n=n)
    m = len(s["meshes"])
    buckets = int(s["meshes"]["n_lods"].sum())
    stride = min(buckets, n)
    cam = np.asarray(s["cam_pos"], np.float32)
    cams = [cam + np.asarray(d, np.float32) for d in ((0, 0, 0), (25, 0, 0), (0, 0, -25), (-20, 5, 20))][:n_views]
    with torch.cuda.stream(st):
        p = renderer_amd.InstancePipeline(n, m, stream=st.cuda_stream)
        p.set_mesh_table(s["meshes"])
        p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
        words = (n + 31) // 32 + 1
        bitmaps = torch.zeros((n_views, words), dtype=torch.int32, device=dev)
        ones = torch.full((words,), -1, dtype=torch.int32, device=dev)
        cmds = torch.empty((n_views, n, 5), dtype=torch.int32, device=dev)
        scal = torch.zeros((n_views, 2), dtype=torch.int32, device=dev)
        one_cmds = torch.empty((n_views, stride, 5), dtype=torch.int32, device=dev)      # four calls: a set of outputs per view
        one_ids = torch.empty((n_views, n), dtype=torch.int32, device=dev)
        one_scal = torch.zeros((n_views, 2), dtype=torch.int32, device=dev)
        v_cmds = torch.empty((n_views * stride, 5), dtype=torch.int32, device=dev)        # one call
        v_ids = torch.empty(n_views * n, dtype=torch.int32, device=dev)
        v_counts = torch.zeros(n_views, dtype=torch.int32, device=dev)
        v_slots = torch.zeros(n_views + 1, dtype=torch.int32, device=dev)
        light_cmds = torch.empty((n_views * n, 5), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        frames = [make_frame(f, c, first_instance_base=v * n) for v, (f, c) in enumerate(zip(view_frusta(s["planes"], n_views), cams))]
        p.run_views(frames, [p.prepare_outputs(visible_bitmap=bitmaps[v].data_ptr(), draw_cmds=cmds[v].data_ptr(), draw_count=scal[v].data_ptr(),
                                               draw_index_total=scal[v].data_ptr() + 4) for v in range(n_views)])
        p.wait()
        listed = [int(x) for x in scal[:, 0].cpu()]      # per-instance commands per view: what mip_run_views hands a consumer today
        policy = make_lod_policy("distance", LODS_DISTANCE_SQ)
        one_out = [dict(batch_cmds=one_cmds[v].data_ptr(), batch_count=one_scal[v].data_ptr(), instance_ids=one_ids[v].data_ptr(),
                        instance_count=one_scal[v].data_ptr() + 4, async_=True) for v in range(n_views)]
        views_out = dict(batch_cmds=v_cmds.data_ptr(), cmd_stride=stride, batch_counts=v_counts.data_ptr(), instance_ids=v_ids.data_ptr(),
                         view_first_slot=v_slots.data_ptr(), async_=True)
        have_views = hasattr(p._lib, "mip_batch_draws_views")
        lights = np.stack(cams)

        def four_calls(ptrs):
            def fn():
                for v in range(n_views):
                    p.batch_draws_lods(frames[v], ptrs[v], policy, **one_out[v])
            return fn

        culled_ptrs, ones_ptrs = [bitmaps[v].data_ptr() for v in range(n_views)], [ones.data_ptr()] * n_views
        legs = [("culled", f"{n_views} x batch_draws_lods", four_calls(culled_ptrs), "four"),
                ("unculled", f"{n_views} x batch_draws_lods", four_calls(ones_ptrs), "four"),
                ("unculled", f"light_draw_lists, {n_views} lights", lambda: p.light_draw_lists(lights, light_cmds.data_ptr(), async_=True), "lights")]
        if have_views:
            legs += [("culled", "batch_draws_views", lambda: p.batch_draws_views(frames, culled_ptrs, policy, **views_out), "one"),
                     ("unculled", "batch_draws_views", lambda: p.batch_draws_views(frames, [0] * n_views, policy, **views_out), "one")]
        for case, name, fn, kind in legs:
            r = measure(st, fn, samples=samples)
            p.wait()
            row = dict(leg=f"views: {name}, {case}", library=library, n=n, config=config, meshes=m, views=n_views, buckets=buckets, **r)
            if kind == "four":
                row.update(draws_per_view_before=listed if case == "culled" else [n] * n_views, draws_per_view_after=[int(x) for x in one_scal[:, 0].cpu()],
                           members_per_view=[int(x) for x in one_scal[:, 1].cpu()])
            elif kind == "one":
                slots = [int(x) for x in v_slots.cpu()]
                row.update(draws_per_view_before=listed if case == "culled" else [n] * n_views, draws_per_view_after=[int(x) for x in v_counts.cpu()],
                           members_per_view=[b - a for a, b in zip(slots, slots[1:])])
            else:
                row.update(commands=n_views * n, command_bytes=n_views * n * 20)
            emit(row)
        p.close()


def bench_sharded(n, emit, samples=40, library="this build", world=8):
    import numpy as np
    import torch

    import renderer_amd
    from renderer_amd import scene
    from renderer_amd.pipeline import make_frame, make_lod_policy
    from renderer_amd.sharded import batch_chunk_stride_bytes, chunk_stride_bytes, shard_range

    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream()
    config = 2 if n <= 100_000 else 3
    policy = make_lod_policy("distance", LODS_DISTANCE_SQ)
    for culled in (True, False):
        s = scene.make_scene(config, n=n, all_visible=not culled)
        m = len(s["meshes"])
        buckets = int(s["meshes"]["n_lods"].sum())
        per = shard_range(n, world, 0)[1]
        stride, wire_stride = batch_chunk_stride_bytes(buckets, per), chunk_stride_bytes(per, "packed")
        with torch.cuda.stream(st):
            p = renderer_amd.InstancePipeline(per, m, stream=st.cuda_stream)
            p.set_mesh_table(s["meshes"])
            recv = torch.zeros(world * stride // 4, dtype=torch.int32, device=dev)
            wire_recv = torch.zeros(world * wire_stride // 4, dtype=torch.int32, device=dev)
            bitmap = torch.zeros((per + 31) // 32 + 1, dtype=torch.int32, device=dev)
            m_cmds = torch.empty((max(buckets, 1), 5), dtype=torch.int32, device=dev)
            m_ids = torch.empty(world * per, dtype=torch.int32, device=dev)
            m_scal = torch.zeros(8, dtype=torch.int32, device=dev)
            l_cmds = torch.empty((world * per, 5), dtype=torch.int32, device=dev)
            l_scal = torch.zeros(8, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            for rank in range(world):   # the last shard stays resident: the shard call is timed on it
                lo, hi = shard_range(n, world, rank)
                p.set_instances(s["pos"][lo:hi], s["rot"][lo:hi], s["scale"][lo:hi], s["mesh_id"][lo:hi])
                frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=lo)
                w = wire_recv.data_ptr() + rank * wire_stride
                p.run_device(frame, visible_bitmap=bitmap.data_ptr(), draw_cmds=w + 32, draw_count=w, draw_index_total=w + 4, wire=2)
                p.batch_draws_shard(frame, bitmap.data_ptr(), policy, recv.data_ptr() + rank * stride, per)
            members = int(recv.view(world, stride // 4)[:, 0].sum().item())
            draws = int(wire_recv.view(world, wire_stride // 4)[:, 0].sum().item())
            row = dict(library=library, n=n, config=config, world=world, culled=culled, buckets=buckets, shard_instances=per, members=members)

            outs = dict(batch_cmds=m_cmds.data_ptr(), batch_count=m_scal.data_ptr(), instance_ids=m_ids.data_ptr(), instance_count=m_scal.data_ptr() + 4)
            r = measure(st, lambda: p.batch_draws_lods(frame, bitmap.data_ptr(), policy, async_=True, **outs), samples=samples)
            p.wait()
            emit(dict(leg="sharded: batch_draws_lods on one shard, ids only", **row, **r))
            scratch_chunk = torch.empty(stride // 4, dtype=torch.int32, device=dev)
            r = measure(st, lambda: p.batch_draws_shard(frame, bitmap.data_ptr(), policy, scratch_chunk.data_ptr(), per, async_=True), samples=samples)
            p.wait()
            emit(dict(leg="sharded: batch_draws_shard on one shard", shard_members=int(scratch_chunk[0].item()), **row, **r))

            r = measure(st, lambda: p.merge_batches(recv.data_ptr(), world, stride, per, async_=True, **outs), samples=samples)
            p.wait()
            assert int(m_scal[1].item()) == members
            emit(dict(leg="sharded: merge_batches", batch_count=int(m_scal[0].item()), bytes_moved=8 * members, **row, **r))
            src = torch.empty(max(members, 1), dtype=torch.int32, device=dev)
            dst = torch.empty(max(members, 1), dtype=torch.int32, device=dev)
            r = measure(st, lambda: dst.copy_(src), samples=samples)
            emit(dict(leg="sharded: device-to-device copy of members x 4 bytes", bytes_moved=8 * members, **row, **r))
            r = measure(st, lambda: p.merge_wire_lists(wire_recv.data_ptr(), world, wire_stride, l_cmds.data_ptr(), l_scal.data_ptr(), async_=True,
                                                       chunk_capacity=per, packed=True), samples=samples)
            p.wait()
            assert int(l_scal[0].item()) == draws
            emit(dict(leg="sharded: merge_wire_lists_packed of the same frame's draw lists", draws=draws, bytes_moved=draws * 24, **row, **r))
            p.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", nargs="*", type=int, default=[1_000_000, 100_000])
    ap.add_argument("--samples", type=int, default=40)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    ap.add_argument("--lods", action="store_true", help="the mip_batch_draws_lods legs instead of (a) .. (s)")
    ap.add_argument("--ordered", action="store_true", help="the mip_batch_draws_ordered legs instead of (a) .. (s)")
    ap.add_argument("--sorted", action="store_true", help="the mip_batch_draws_sorted legs beside mip_batch_draws_ordered instead of (a) .. (s)")
    ap.add_argument("--views", action="store_true", help="the mip_batch_draws_views legs (V = 4) and their yardsticks instead of (a) .. (s)")
    ap.add_argument("--sharded", action="store_true", help="mip_batch_draws_shard and mip_merge_batches over 8 shards, and their yardsticks")
    ap.add_argument("--parent-library", default=None, help="also run the same legs on this build of the library: the yardstick (child processes)")
    ap.add_argument("--library-label", default="this build", help=argparse.SUPPRESS)  # a child's rows: which library it loaded
    a = ap.parse_args()

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    if a.parent_library:  # a library is loaded once per process (MIP_LIBRARY, renderer_amd/_lib.py): this process starts children and never opens the GPU
        import subprocess

        cmd = [sys.executable, os.path.abspath(__file__)] + [str(n) for n in a.n] + ["--samples", str(a.samples)]
        cmd += (["--lods"] if a.lods else []) + (["--ordered"] if a.ordered else []) + (["--sorted"] if a.sorted else []) + (["--views"] if a.views else []) + (["--out", a.out] if a.out else [])
        parent = dict(os.environ, MIP_LIBRARY=os.path.abspath(a.parent_library))
        for label, env in (("parent commit, first run", parent), ("this build", os.environ), ("parent commit, last run", parent)):
            subprocess.run(cmd + ["--library-label", label], check=True, env=env)
        return
    for n in a.n:
        if a.sharded:
            bench_sharded(n, emit, a.samples, library=a.library_label)
        elif a.views:
            bench_views(n, emit, a.samples, library=a.library_label)
        elif a.ordered:
            bench_ordered(n, emit, a.samples, library=a.library_label)
        elif a.sorted:
            bench_sorted(n, emit, a.samples, library=a.library_label)
        elif a.lods:
            bench_lods(n, emit, a.samples, library=a.library_label)
        else:
            bench(n, emit, a.samples, library=a.library_label)
    if not (a.ordered or a.lods or a.sorted or a.views or a.sharded):
        bench_several(emit, a.samples, library=a.library_label)


if __name__ == "__main__":
    main()
