#!/usr/bin/env python3
"""GPU time of the two cone calls beside the plain calls they extend, by the method of tools/cluster_triangle_bench.py (HIP
events on the launch stream around 20 back-to-back calls, median of samples, one JSON line per leg): mip_cull_clusters against
mip_cull_clusters_cone and mip_cull_cluster_triangles against mip_cull_cluster_triangles_cone over the bitmap of a mip_run of
the scene, under the pin policy, with the frustum alone and with the wall of tools/cluster_bench.py, for
scene.make_geometry("strips") and ("patches"); beside them mip_run with culled_index_buffer (the per-triangle stage). Config 3 at
1 M instances and config 2 at 100 k. Every cone row carries the clusters that have a cone, the work items the cone removes,
the waves of 64 items it empties (the cull kernel answers those without a box), the survivors, the commands and the triangles
tested and kept; a row of its own carries the build time of the cone table.

The items the cone removes and the waves it empties are not outputs of the library: they come from the numpy restatement
(tests/cluster_cone_restatement.py) over the call's own work items, in slices.

  python tools/cluster_cone_bench.py [--samples 20] [--out profiles/cluster_cones_bench.jsonl]

--once CONFIG: one warm call of each leg under "patches" and nothing else, for a kernel trace of its own
(rocprofv3 --kernel-trace --stats -- python tools/cluster_cone_bench.py --once 3).
--stage-only: the mip_run leg alone — run it with MIP_LIBRARY set to another build of the library (and --label naming it, --append
to keep the rows already written) for an A/B of that stage."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from tools.batch_bench import measure  # noqa: E402
from tools.cluster_bench import WALL  # noqa: E402


def cone_census(s, cones, bitmap, eye, facing, switch_sq):
    """(items the cone removes, waves it empties, W) by the restatement, 1 M work items at a time."""
    import numpy as np

    import cluster_cone_restatement as ccr
    import cluster_restatement as cr
    import lod_restatement as lr

    items = cr.work_items(s["pos"], s["scale"], s["mesh_id"], s["meshes"], s["cam_pos"], bitmap, lr.DISTANCE, switch_sq)
    w = items["W"]
    culled = np.zeros(w, bool)
    for lo in range(0, w, 1 << 20):
        part = dict(items, inst=items["inst"][lo : lo + (1 << 20)], box_index=items["box_index"][lo : lo + (1 << 20)])
        culled[lo : lo + (1 << 20)] = ccr.cone_culled(part, cones, s["pos"], s["rot"], s["scale"], eye, facing)
    return int(culled.sum()), ccr.waves_skipped(~culled, w), w


def bench(config, ordering, emit, samples=20, once=False, stage_only=False, label="this build"):
    import numpy as np
    import torch

    import renderer_amd
    from renderer_amd import _lib, scene
    from renderer_amd.pipeline import (LOD_PIN_SWITCH_SQ, depth_pyramid_layout, make_cluster_cone, make_cluster_outputs,
                                       make_cluster_triangle_outputs, make_frame, make_lod_policy, make_occlusion)

    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream()
    s = scene.make_scene(config)
    n, m = s["n"], len(s["meshes"])
    vertices, indices = scene.make_geometry(s["meshes"], ordering)
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
        common = dict(config=config, n=n, ordering=ordering, library=label)

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
            builds = []
            for _ in range(5):
                t0 = time.perf_counter()
                p.build_cluster_cones()                       # synchronous: the call returns when the table is complete
                builds.append((time.perf_counter() - t0) * 1e6)
            cones = p.read_cluster_cones()
            with_cone = int(np.isfinite(cones[:, 3]).sum())
            cone = make_cluster_cone(pv)
            removed, emptied, w = (0, 0, 0) if once else cone_census(s, cones, bitmap[: (n + 31) // 32].cpu().numpy().view(np.uint32),
                                                                     np.array(list(cone.eye), np.float32), cone.facing, LOD_PIN_SWITCH_SQ)
            emit(dict(leg="mip_build_cluster_cones (host time of the synchronous call)", clusters=len(cones), clusters_with_cone=with_cone,
                      median_us=round(float(np.median(builds)), 1), min_us=round(float(min(builds)), 1), **common))
            largest = int(((s["meshes"]["index_len"] // 3 + 63) // 64).max())
            work = min(members * largest, (1 << 32) - 1)
            depth = torch.ones((WALL[1], WALL[0]), dtype=torch.float32, device=dev)
            depth[:, : WALL[0] // 2] = 0.0
            pyramid = torch.empty(depth_pyramid_layout(*WALL)["bytes"] // 4, dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            p.build_depth_pyramid(depth.data_ptr(), WALL[0], WALL[1], pyramid.data_ptr(), format=_lib.MIP_DEPTH_FLOAT32)
            occ = make_occlusion(WALL[0], WALL[1], pyramid.data_ptr(), pv)
            # the cone cuts runs apart: a member of C clusters has at most ceil(C / 2) runs, so this is always room
            c_cmds = torch.empty(((work + members) // 2 + 1, 5), dtype=torch.int32, device=dev)
            c_scal = torch.zeros(12, dtype=torch.int32, device=dev)
            plain = make_cluster_outputs(c_cmds.data_ptr(), len(c_cmds), c_scal.data_ptr(), c_scal.data_ptr() + 8, work_capacity=work, async_=True)
            no_room = torch.empty(1, dtype=torch.int32, device=dev)
            try:   # the stream's size is the plain call's to tell (the cone call's is never larger)
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

            def cluster_row(six, coned):
                v = [int(x) for x in c_scal[2:8].cpu().numpy().view(np.uint32)]
                row = dict(commands=v[0], survivors=v[1], W=v[2], members=v[3])
                if six:
                    row.update(triangles_kept=v[4], triangles_tested=v[5])
                if coned:
                    row.update(clusters_with_cone=with_cone, items_cone_culled=removed, waves_skipped=emptied, waves=(w + 63) // 64)
                return row

            bm = bitmap.data_ptr()
            for what, o in (("frustum", None), ("frustum + pyramid", occ)):
                legs.append((f"mip_cull_clusters, {what}", (lambda o=o: p.cull_clusters(frame, bm, policy, plain, occlusion=o)), lambda: cluster_row(False, False)))
                legs.append((f"mip_cull_clusters_cone, {what}", (lambda o=o: p.cull_clusters_cone(frame, bm, policy, cone, plain, occlusion=o)),
                             lambda: cluster_row(False, True)))
                legs.append((f"mip_cull_cluster_triangles, {what}", (lambda o=o: p.cull_cluster_triangles(frame, bm, policy, tri, occlusion=o)),
                             lambda: cluster_row(True, False)))
                legs.append((f"mip_cull_cluster_triangles_cone, {what}", (lambda o=o: p.cull_cluster_triangles_cone(frame, bm, policy, cone, tri, occlusion=o)),
                             lambda: cluster_row(True, True)))
        for name, fn, describe in legs:
            fn()
            p.wait()
            row = dict(leg=name, **common)
            row.update(describe())
            if not once:
                row.update(measure(st, fn, samples=samples))
                p.wait()
            emit(row)
        p.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_cones_bench.jsonl"))
    ap.add_argument("--once", type=int, default=0, metavar="CONFIG")
    ap.add_argument("--configs", default="3,2")
    ap.add_argument("--orderings", default="strips,patches")
    ap.add_argument("--stage-only", action="store_true", help="the mip_run leg alone (for an A/B of that stage with MIP_LIBRARY)")
    ap.add_argument("--label", default="this build", help="the `library` field of every row (name the build MIP_LIBRARY selects)")
    ap.add_argument("--append", action="store_true", help="append to --out")
    args = ap.parse_args()
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    if args.once:
        bench(args.once, "patches", emit, once=True, stage_only=args.stage_only, label=args.label)
        return
    for config in (int(c) for c in args.configs.split(",")):
        for ordering in args.orderings.split(","):
            bench(config, ordering, emit, samples=args.samples, stage_only=args.stage_only, label=args.label)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
