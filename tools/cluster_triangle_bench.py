#!/usr/bin/env python3
"""GPU time of mip_cull_cluster_triangles beside the two stages it connects, on the same inputs and by the method of
tools/cluster_bench.py (HIP events on the launch stream around BATCH back-to-back repetitions, median of samples, one JSON line
per leg): mip_cull_clusters over the same bitmap, and mip_run with culled_index_buffer (the per-triangle stage) over the same
scene and layout. Config 3 at 1 M instances and config 2 at 100 k, the bitmap of a mip_run of the scene, the pin policy,
scene.make_geometry("strips"); with and without the wall of tools/cluster_bench.py. Every row of the new call carries W, the
surviving clusters, the commands, the triangles tested and kept.

  python tools/cluster_triangle_bench.py [--samples 40] [--out profiles/cluster_triangles_bench.jsonl]

--once CONFIG: one warm call of each leg and nothing else, for a kernel trace of its own
(rocprofv3 --kernel-trace --stats -- python tools/cluster_triangle_bench.py --once 3).
--stage-only: the mip_run leg alone — run it with MIP_LIBRARY set to another build of the library (and --label naming it, --append
to keep the rows already written) for an A/B of that stage."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.batch_bench import measure  # noqa: E402
from tools.cluster_bench import WALL  # noqa: E402


def bench(config, emit, samples=40, once=False, stage_only=False, label="this build"):
    import numpy as np
    import torch

    import renderer_amd
    from renderer_amd import _lib, scene
    from renderer_amd.pipeline import (LOD_PIN_SWITCH_SQ, depth_pyramid_layout, make_cluster_outputs, make_cluster_triangle_outputs, make_frame,
                                       make_lod_policy, make_occlusion)

    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream()
    s = scene.make_scene(config)
    n, m = s["n"], len(s["meshes"])
    vertices, indices = scene.make_geometry(s["meshes"], "strips")
    pv = scene.default_pv()
    with torch.cuda.stream(st):
        p = renderer_amd.InstancePipeline(n, m, stream=st.cuda_stream)
        p.set_mesh_table(s["meshes"])
        p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
        p.set_geometry(vertices, indices)
        bitmap = torch.zeros((n + 31) // 32 + 1, dtype=torch.int32, device=dev)
        cmds = torch.empty((n, 5), dtype=torch.int32, device=dev)
        scal = torch.zeros(8, dtype=torch.int32, device=dev)
        model = torch.empty((n, 16), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        frame = make_frame(s["planes"], s["cam_pos"], pv=pv)
        p.run_device(frame, visible_bitmap=bitmap.data_ptr(), draw_cmds=cmds.data_ptr(), draw_count=scal.data_ptr(), draw_index_total=scal.data_ptr() + 4)
        members, index_total = (int(v) for v in scal[:2].cpu().numpy().view(np.uint32))
        legs = []

        # the per-triangle stage of mip_run, every triangle of every visible instance (its commands and its bitmap go to buffers of its own)
        t_cmds = torch.empty((n, 5), dtype=torch.int32, device=dev)
        t_bitmap = torch.zeros_like(bitmap)
        t_scal = torch.zeros(8, dtype=torch.int32, device=dev)
        t_out = torch.empty(index_total + 3, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        run_stage = lambda: p.run_device(frame, model=model.data_ptr(), visible_bitmap=t_bitmap.data_ptr(), draw_cmds=t_cmds.data_ptr(),
                                         draw_count=t_scal.data_ptr(), draw_index_total=t_scal.data_ptr() + 4, culled_index_buffer=t_out.data_ptr(),
                                         culled_index_capacity=index_total, async_=True)
        stage_row = lambda: dict(triangles_tested=index_total // 3, commands=int(t_scal[0].item()),
                                 triangles_kept=int(t_cmds[: int(t_scal[0].item()), 0].to(torch.int64).sum().item()) // 3)
        legs.append(("mip_run with culled_index_buffer (frame + per-triangle stage)", run_stage, stage_row))

        if not stage_only:
            policy = make_lod_policy(_lib.MIP_LOD_DISTANCE, LOD_PIN_SWITCH_SQ)
            p.build_clusters()
            largest = int(((s["meshes"]["index_len"] // 3 + 63) // 64).max())
            work = min(members * largest, (1 << 32) - 1)
            depth = torch.ones((WALL[1], WALL[0]), dtype=torch.float32, device=dev)
            depth[:, : WALL[0] // 2] = 0.0
            pyramid = torch.empty(depth_pyramid_layout(*WALL)["bytes"] // 4, dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            p.build_depth_pyramid(depth.data_ptr(), WALL[0], WALL[1], pyramid.data_ptr(), format=_lib.MIP_DEPTH_FLOAT32)
            occ = make_occlusion(WALL[0], WALL[1], pyramid.data_ptr(), pv)
            c_cmds = torch.empty((8 * max(members, 1), 5), dtype=torch.int32, device=dev)
            c_scal = torch.zeros(12, dtype=torch.int32, device=dev)
            plain = make_cluster_outputs(c_cmds.data_ptr(), len(c_cmds), c_scal.data_ptr(), c_scal.data_ptr() + 8, work_capacity=work, async_=True)
            # the stream's size is the call's to tell: a first call without room overflows and leaves the count in stats[4]
            no_room = torch.empty(1, dtype=torch.int32, device=dev)
            try:
                p.cull_cluster_triangles(frame, bitmap.data_ptr(), policy,
                                         make_cluster_triangle_outputs(c_cmds.data_ptr(), len(c_cmds), c_scal.data_ptr(), no_room.data_ptr(), 0,
                                                                       stats=c_scal.data_ptr() + 8, work_capacity=work))
            except renderer_amd.MipError:
                pass
            room = 3 * int(c_scal[6:7].cpu().numpy().view(np.uint32)[0])
            stream = torch.empty(room + 3, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            tri = make_cluster_triangle_outputs(c_cmds.data_ptr(), len(c_cmds), c_scal.data_ptr(), stream.data_ptr(), room, stats=c_scal.data_ptr() + 8,
                                                work_capacity=work, async_=True)

            def cluster_row(six):
                v = [int(x) for x in c_scal[2:8].cpu().numpy().view(np.uint32)]
                row = dict(commands=v[0], survivors=v[1], W=v[2], members=v[3])
                if six:
                    row.update(triangles_kept=v[4], triangles_tested=v[5])
                return row

            for what, o in (("frustum", None), ("frustum + pyramid", occ)):
                legs.append((f"mip_cull_clusters, {what}", (lambda o=o: p.cull_clusters(frame, bitmap.data_ptr(), policy, plain, occlusion=o)),
                             lambda: cluster_row(False)))
                legs.append((f"mip_cull_cluster_triangles, {what}", (lambda o=o: p.cull_cluster_triangles(frame, bitmap.data_ptr(), policy, tri, occlusion=o)),
                             lambda: cluster_row(True)))
        for name, fn, describe in legs:
            fn()
            p.wait()
            row = dict(leg=name, config=config, n=n, library=label)
            row.update(describe())
            if not once:
                row.update(measure(st, fn, samples=samples))
                p.wait()
            emit(row)
        p.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samples", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_triangles_bench.jsonl"))
    ap.add_argument("--once", type=int, default=0, metavar="CONFIG")
    ap.add_argument("--stage-only", action="store_true", help="the mip_run leg alone (for an A/B of that stage with MIP_LIBRARY)")
    ap.add_argument("--label", default="this build", help="the `library` field of every row (name the build MIP_LIBRARY selects)")
    ap.add_argument("--append", action="store_true", help="append to --out")
    args = ap.parse_args()
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    if args.once:
        bench(args.once, emit, once=True, stage_only=args.stage_only, label=args.label)
        return
    for config in (3, 2):
        bench(config, emit, samples=args.samples, stage_only=args.stage_only, label=args.label)
    with open(args.out, "a" if args.append else "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
