#!/usr/bin/env python3
"""GPU time of mip_list_clusters beside the command call it replaces (mip_cull_clusters, or mip_cull_clusters_cone with a
cone), by the method of tools/cluster_bench.py: HIP events on the launch stream around 20 back-to-back calls, the median of 40
samples, one JSON line per leg. The two calls of a leg ALTERNATE in one session — 10 samples of one, 10 of the other, four
times — so that both see the same clocks. Legs: the frustum alone, the frustum and the wall pyramid of tools/cluster_bench.py
(both over scene.make_geometry("strips")), and the frustum with the cone of default_pv over "patches"; over the bitmap of a
mip_run of the scene, under the pin policy. Config 3 at 1 M instances and config 2 at 100 k. Every row carries the survivors,
the commands or entries written, W, the members and the bytes the call's last kernel has to write (commands x 20 B, entries x
16 B), with the time a 4 TB/s device needs to move them.

  python tools/cluster_list_bench.py [--samples 40] [--out profiles/cluster_list_bench.jsonl]

--once CONFIG: one warm call of each leg's two calls and nothing else, for a kernel trace of its own
(rocprofv3 --kernel-trace --stats -- python tools/cluster_list_bench.py --once 3)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from tools.cluster_bench import WALL  # noqa: E402

BATCH = 20
MOVE_BYTES_PER_US = 4.0e6   # 4 TB/s: the yardstick for the bytes the write kernel moves, not a measurement


def sample(st, fn, samples):
    """`samples` times: the GPU time of BATCH back-to-back calls, per call, in microseconds."""
    import torch

    out = []
    for _ in range(samples):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(BATCH):
            fn()
        e1.record(st)
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / BATCH * 1e3)
    return out


def summary(us):
    import numpy as np

    us = np.array(us)
    return dict(median_us=round(float(np.median(us)), 3), min_us=round(float(us.min()), 3), p90_us=round(float(np.percentile(us, 90)), 3), samples=len(us))


def bench(config, emit, samples=40, once=False):
    import numpy as np
    import torch

    import renderer_amd
    from renderer_amd import _lib, scene
    from renderer_amd.pipeline import (LOD_PIN_SWITCH_SQ, depth_pyramid_layout, make_cluster_cone, make_cluster_list_outputs, make_cluster_outputs,
                                       make_frame, make_lod_policy, make_occlusion)

    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream()
    s = scene.make_scene(config)
    n, m = s["n"], len(s["meshes"])
    pv = scene.default_pv()
    for ordering, legs in (("strips", (("frustum", False, False), ("frustum + pyramid", True, False))), ("patches", (("frustum + cone", False, True),))):
        vertices, indices = scene.make_geometry(s["meshes"], ordering)
        with torch.cuda.stream(st):
            p = renderer_amd.InstancePipeline(n, m, stream=st.cuda_stream)
            p.set_mesh_table(s["meshes"])
            p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
            p.set_geometry(vertices, indices)
            p.build_clusters()
            p.build_cluster_cones()
            bitmap = torch.zeros((n + 31) // 32 + 1, dtype=torch.int32, device=dev)
            cmds = torch.empty((n, 5), dtype=torch.int32, device=dev)
            scal = torch.zeros(8, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            frame = make_frame(s["planes"], s["cam_pos"], pv=pv)
            p.run_device(frame, visible_bitmap=bitmap.data_ptr(), draw_cmds=cmds.data_ptr(), draw_count=scal.data_ptr(), draw_index_total=scal.data_ptr() + 4)
            members = int(scal[:1].cpu().numpy().view(np.uint32)[0])
            policy = make_lod_policy(_lib.MIP_LOD_DISTANCE, LOD_PIN_SWITCH_SQ)
            largest = int(((s["meshes"]["index_len"] // 3 + 63) // 64).max())
            work = min(members * largest, (1 << 32) - 1)
            depth = torch.ones((WALL[1], WALL[0]), dtype=torch.float32, device=dev)
            depth[:, : WALL[0] // 2] = 0.0
            pyramid = torch.empty(depth_pyramid_layout(*WALL)["bytes"] // 4, dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            p.build_depth_pyramid(depth.data_ptr(), WALL[0], WALL[1], pyramid.data_ptr(), format=_lib.MIP_DEPTH_FLOAT32)
            occ = make_occlusion(WALL[0], WALL[1], pyramid.data_ptr(), pv)
            cone = make_cluster_cone(pv)
            c_cmds = torch.empty(((work + members) // 2 + 1, 5), dtype=torch.int32, device=dev)   # a member of C clusters has at most ceil(C / 2) runs
            c_scal = torch.zeros(8, dtype=torch.int32, device=dev)
            entries = torch.empty((work, 4), dtype=torch.int32, device=dev)
            l_scal = torch.zeros(12, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            plain = make_cluster_outputs(c_cmds.data_ptr(), len(c_cmds), c_scal.data_ptr(), c_scal.data_ptr() + 8, work_capacity=work, async_=True)
            listed = make_cluster_list_outputs(entries.data_ptr(), work, l_scal.data_ptr(), l_scal.data_ptr() + 8, l_scal.data_ptr() + 24,
                                               work_capacity=work, async_=True)
            bm = bitmap.data_ptr()
            for what, walled, coned in legs:
                o, k = (occ if walled else None), (cone if coned else None)
                if coned:
                    command_call = lambda o=o, k=k: p.cull_clusters_cone(frame, bm, policy, k, plain, occlusion=o)   # noqa: E731
                else:
                    command_call = lambda o=o: p.cull_clusters(frame, bm, policy, plain, occlusion=o)   # noqa: E731
                list_call = lambda o=o, k=k: p.list_clusters(frame, bm, policy, listed, occlusion=o, cone=k)   # noqa: E731
                command_call()
                list_call()
                p.wait()
                heads, survivors, w, mem = (int(v) for v in c_scal[2:6].cpu().numpy().view(np.uint32))
                count, l_survivors, l_w, l_mem = (int(v) for v in l_scal[[0, 6, 7, 8]].cpu().numpy().view(np.uint32))
                assert (l_survivors, l_w, l_mem) == (survivors, w, mem) and count == survivors
                common = dict(config=config, n=n, ordering=ordering, test=what, survivors=survivors, W=w, members=mem)
                rows = [dict(leg=("mip_cull_clusters_cone" if coned else "mip_cull_clusters"), written=heads, bytes_written=20 * heads, **common),
                        dict(leg="mip_list_clusters", written=count, bytes_written=16 * count, **common)]
                for row in rows:
                    row["move_us_at_4TBps"] = round(row["bytes_written"] / MOVE_BYTES_PER_US, 3)
                if not once:
                    us = ([], [])
                    for fn in (command_call, list_call):       # warm
                        for _ in range(3 * BATCH):
                            fn()
                    st.synchronize()
                    for _ in range(4):                         # alternate: 4 x (samples / 4) of each
                        for which, fn in enumerate((command_call, list_call)):
                            us[which].extend(sample(st, fn, max(samples // 4, 1)))
                    p.wait()
                    for row, series in zip(rows, us):
                        row.update(summary(series))
                    rows[1]["list_over_commands"] = round(rows[1]["median_us"] / rows[0]["median_us"], 4)
                for row in rows:
                    emit(row)
            p.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samples", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_list_bench.jsonl"))
    ap.add_argument("--once", type=int, default=0, metavar="CONFIG")
    ap.add_argument("--configs", default="3,2")
    args = ap.parse_args()
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    if args.once:
        bench(args.once, emit, once=True)
        return
    for config in (int(c) for c in args.configs.split(",")):
        bench(config, emit, samples=args.samples)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
