#!/usr/bin/env python3
"""GPU time of mip_list_cluster_triangles beside the three calls it stands between, by the method of tools/cluster_bench.py:
HIP events on the launch stream around 20 back-to-back calls, the median of at least 20 samples, one JSON line per leg. The
four legs ALTERNATE sample by sample in one process, so that all see the same clocks:

  1. mip_list_cluster_triangles                 entries and a 64-bit triangle mask per entry
  2. mip_cull_cluster_triangles                 the dense index stream and commands into it
  3. mip_run with culled_index_buffer           the frame and the per-triangle stage
  4. mip_list_clusters                          the list without the triangle test

Config 3 at 1 M instances and config 2 at 100 k; scene.make_geometry "strips" and "patches"; the frustum alone and with the
wall of tools/cluster_bench.py; the bitmap of a mip_run of the scene, the pin policy. Every row of legs 1 and 2 carries W, the
surviving clusters, what was written, the triangles tested and kept, and tested / time as a rate for the whole call.

  python tools/cluster_triangle_list_bench.py [--samples 20] [--out profiles/cluster_triangle_list_bench.jsonl]

--once CONFIG: one warm call of legs 1, 2 and 4 per scene and nothing else, for a kernel trace of its own
(rocprofv3 --kernel-trace --stats -- python tools/cluster_triangle_list_bench.py --once 3)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from tools.cluster_bench import WALL  # noqa: E402
from tools.cluster_list_bench import BATCH, summary  # noqa: E402


def one_sample(st, fn):
    """The GPU time of BATCH back-to-back calls, per call, in microseconds."""
    import torch

    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(BATCH):
        fn()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1) / BATCH * 1e3


def bench(config, emit, samples=20, once=False, orderings=("strips", "patches")):
    import numpy as np
    import torch

    import renderer_amd
    from renderer_amd import _lib, scene
    from renderer_amd.pipeline import (LOD_PIN_SWITCH_SQ, depth_pyramid_layout, make_cluster_list_outputs, make_cluster_triangle_list_outputs,
                                       make_cluster_triangle_outputs, make_frame, make_lod_policy, make_occlusion)

    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream()
    s = scene.make_scene(config)
    n, m = s["n"], len(s["meshes"])
    pv = scene.default_pv()
    for ordering in orderings:
        vertices, indices = scene.make_geometry(s["meshes"], ordering)
        with torch.cuda.stream(st):
            p = renderer_amd.InstancePipeline(n, m, stream=st.cuda_stream)
            p.set_mesh_table(s["meshes"])
            p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
            p.set_geometry(vertices, indices)
            p.build_clusters()
            bitmap = torch.zeros((n + 31) // 32 + 1, dtype=torch.int32, device=dev)
            cmds = torch.empty((n, 5), dtype=torch.int32, device=dev)
            scal = torch.zeros(8, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            frame = make_frame(s["planes"], s["cam_pos"], pv=pv)
            p.run_device(frame, visible_bitmap=bitmap.data_ptr(), draw_cmds=cmds.data_ptr(), draw_count=scal.data_ptr(), draw_index_total=scal.data_ptr() + 4)
            members, index_total = (int(v) for v in scal[:2].cpu().numpy().view(np.uint32))
            policy = make_lod_policy(_lib.MIP_LOD_DISTANCE, LOD_PIN_SWITCH_SQ)
            largest = int(((s["meshes"]["index_len"] // 3 + 63) // 64).max())
            work = min(members * largest, (1 << 32) - 1)
            depth = torch.ones((WALL[1], WALL[0]), dtype=torch.float32, device=dev)
            depth[:, : WALL[0] // 2] = 0.0
            pyramid = torch.empty(depth_pyramid_layout(*WALL)["bytes"] // 4, dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            p.build_depth_pyramid(depth.data_ptr(), WALL[0], WALL[1], pyramid.data_ptr(), format=_lib.MIP_DEPTH_FLOAT32)
            occ = make_occlusion(WALL[0], WALL[1], pyramid.data_ptr(), pv)
            # leg 3: the frame with the per-triangle stage, outputs of its own
            t_bitmap = torch.zeros_like(bitmap)
            t_cmds = torch.empty((n, 5), dtype=torch.int32, device=dev)
            t_scal = torch.zeros(8, dtype=torch.int32, device=dev)
            t_out = torch.empty(index_total + 3, dtype=torch.int32, device=dev)
            model = torch.empty((n, 16), dtype=torch.float32, device=dev)
            # legs 1, 2 and 4
            entries = torch.empty((work, 4), dtype=torch.int32, device=dev)
            masks = torch.empty((work, 2), dtype=torch.int32, device=dev)
            tl_scal = torch.zeros(16, dtype=torch.int32, device=dev)
            c_cmds = torch.empty(((work + members) // 2 + 1, 5), dtype=torch.int32, device=dev)   # a member of C clusters has at most ceil(C / 2) runs
            c_scal = torch.zeros(8, dtype=torch.int32, device=dev)
            stream = torch.empty(index_total + 3, dtype=torch.int32, device=dev)
            l_entries = torch.empty((work, 4), dtype=torch.int32, device=dev)
            l_scal = torch.zeros(12, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            masked = make_cluster_triangle_list_outputs(entries.data_ptr(), masks.data_ptr(), work, tl_scal.data_ptr(), tl_scal.data_ptr() + 8,
                                                        tl_scal.data_ptr() + 24, work_capacity=work, async_=True)
            streamed = make_cluster_triangle_outputs(c_cmds.data_ptr(), len(c_cmds), c_scal.data_ptr(), stream.data_ptr(), index_total,
                                                     stats=c_scal.data_ptr() + 8, work_capacity=work, async_=True)
            listed = make_cluster_list_outputs(l_entries.data_ptr(), work, l_scal.data_ptr(), l_scal.data_ptr() + 8, l_scal.data_ptr() + 24,
                                               work_capacity=work, async_=True)
            bm = bitmap.data_ptr()
            run_stage = lambda: p.run_device(frame, model=model.data_ptr(), visible_bitmap=t_bitmap.data_ptr(), draw_cmds=t_cmds.data_ptr(),   # noqa: E731
                                             draw_count=t_scal.data_ptr(), draw_index_total=t_scal.data_ptr() + 4, culled_index_buffer=t_out.data_ptr(),
                                             culled_index_capacity=index_total, async_=True)
            for what, walled in (("frustum", False), ("frustum + pyramid", True)):
                o = occ if walled else None
                calls = [("mip_list_cluster_triangles", lambda o=o: p.list_cluster_triangles(frame, bm, policy, masked, occlusion=o)),
                         ("mip_cull_cluster_triangles", lambda o=o: p.cull_cluster_triangles(frame, bm, policy, streamed, occlusion=o)),
                         ("mip_run with culled_index_buffer (frame + per-triangle stage)", run_stage),
                         ("mip_list_clusters", lambda o=o: p.list_clusters(frame, bm, policy, listed, occlusion=o))]
                for name, fn in calls:
                    if not (once and name.startswith("mip_run")):
                        fn()
                p.wait()
                t_stats = [int(v) for v in tl_scal[6:12].cpu().numpy().view(np.uint32)]
                c_stats = [int(v) for v in c_scal[2:8].cpu().numpy().view(np.uint32)]
                l_stats = [int(v) for v in l_scal[6:9].cpu().numpy().view(np.uint32)]
                assert t_stats[1:] == c_stats[1:] and l_stats == [t_stats[1], t_stats[2], t_stats[3]] and int(tl_scal[0].item()) == t_stats[0]
                common = dict(config=config, n=n, ordering=ordering, test=what, W=t_stats[2], members=t_stats[3], surviving_clusters=t_stats[1])
                rows = [dict(leg=calls[0][0], entries=t_stats[0], triangles_kept=t_stats[4], triangles_tested=t_stats[5], bytes_written=24 * t_stats[0], **common),
                        dict(leg=calls[1][0], commands=c_stats[0], triangles_kept=c_stats[4], triangles_tested=c_stats[5],
                             bytes_written=20 * c_stats[0] + 12 * c_stats[4], **common),
                        dict(leg=calls[2][0], triangles_tested=index_total // 3, **common),
                        dict(leg=calls[3][0], entries=l_stats[0], bytes_written=16 * l_stats[0], **common)]
                if not once:
                    us = [[] for _ in calls]
                    for _, fn in calls:                        # warm
                        for _ in range(2 * BATCH):
                            fn()
                    st.synchronize()
                    for _ in range(max(samples, 20)):          # the legs alternate sample by sample
                        for which, (_, fn) in enumerate(calls):
                            us[which].append(one_sample(st, fn))
                    p.wait()
                    for row, series in zip(rows, us):
                        row.update(summary(series))
                    for row in rows[:2]:
                        row["triangles_tested_per_s"] = float(f"{row['triangles_tested'] / (row['median_us'] * 1e-6):.4g}")
                    rows[0]["over_cull_cluster_triangles"] = round(rows[0]["median_us"] / rows[1]["median_us"], 4)
                    rows[0]["over_run_with_stage"] = round(rows[0]["median_us"] / rows[2]["median_us"], 4)
                    rows[0]["over_list_clusters"] = round(rows[0]["median_us"] / rows[3]["median_us"], 4)
                for row in rows:
                    if not (once and row["leg"].startswith("mip_run")):
                        emit(row)
            p.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_triangle_list_bench.jsonl"))
    ap.add_argument("--once", type=int, default=0, metavar="CONFIG")
    ap.add_argument("--configs", default="3,2")
    ap.add_argument("--orderings", default="strips,patches")
    args = ap.parse_args()
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    orderings = tuple(args.orderings.split(","))
    if args.once:
        bench(args.once, emit, once=True, orderings=orderings[:1])
        return
    for config in (int(c) for c in args.configs.split(",")):
        bench(config, emit, samples=args.samples, orderings=orderings)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
