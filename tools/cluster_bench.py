#!/usr/bin/env python3
"""GPU time of the cluster-culling stage (mip_cull_clusters) beside mip_batch_draws_lods on the same bitmap — the yardstick for
a stage that reads the same instance columns: HIP events on the launch stream around BATCH back-to-back repetitions, median of
samples, one JSON line per leg. Config 3 at 1 M instances and config 2 at 100 k, the bitmap of a mip_run of the scene, the
pin policy, scene.make_geometry("strips"); with and without a depth pyramid (a wall at the near plane over the left half of a
1024 x 512 image, built by mip_build_depth_pyramid). Every row carries W, the surviving clusters and the commands of its run.

  python tools/cluster_bench.py [--samples 40] [--out profiles/cluster_cull_bench.jsonl]

--once CONFIG: one warm call of each leg and nothing else, for a kernel trace of its own
(rocprofv3 --kernel-trace --stats -- python tools/cluster_bench.py --once 3).

--phases: the legs of mip_cull_clusters_phase instead (default --out profiles/cluster_phases_bench.jsonl), same scenes, same
method: FIRST against mip_cull_clusters under the same wall, alternating twice; SECOND under (a) the same wall — every
candidate tested, none drawn —, (b) a cleared image, (c) the wall moved by 1/16 of the width — sparse disocclusion —, each
beside the yardstick, a full mip_cull_clusters under that new pyramid, which is what a caller without a record must run (and
which draws again what phase 1 drew). With --once CONFIG: one warm call of each of these legs."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.batch_bench import measure  # noqa: E402

WALL = (1024, 512)


def bench(config, emit, samples=40, once=False):
    import numpy as np
    import torch

    import renderer_amd
    from renderer_amd import _lib, scene
    from renderer_amd.pipeline import (LOD_PIN_SWITCH_SQ, depth_pyramid_layout, make_cluster_outputs, make_frame, make_lod_policy,
                                       make_occlusion)

    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream()
    s = scene.make_scene(config)
    n, m = s["n"], len(s["meshes"])
    vertices, indices = scene.make_geometry(s["meshes"], "strips")
    with torch.cuda.stream(st):
        p = renderer_amd.InstancePipeline(n, m, stream=st.cuda_stream)
        p.set_mesh_table(s["meshes"])
        p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
        p.set_geometry(vertices, indices)
        p.build_clusters()
        largest = int(((s["meshes"]["index_len"] // 3 + 63) // 64).max())
        bitmap = torch.zeros((n + 31) // 32 + 1, dtype=torch.int32, device=dev)
        cmds = torch.empty((n, 5), dtype=torch.int32, device=dev)
        scal = torch.zeros(8, dtype=torch.int32, device=dev)
        b_cmds = torch.empty((int(s["meshes"]["n_lods"].sum()), 5), dtype=torch.int32, device=dev)
        b_ids = torch.empty(n, dtype=torch.int32, device=dev)
        b_scal = torch.zeros(8, dtype=torch.int32, device=dev)
        depth = torch.ones((WALL[1], WALL[0]), dtype=torch.float32, device=dev)
        depth[:, : WALL[0] // 2] = 0.0
        pyramid = torch.empty(depth_pyramid_layout(*WALL)["bytes"] // 4, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        frame = make_frame(s["planes"], s["cam_pos"])
        policy = make_lod_policy(_lib.MIP_LOD_DISTANCE, LOD_PIN_SWITCH_SQ)
        p.run_device(frame, visible_bitmap=bitmap.data_ptr(), draw_cmds=cmds.data_ptr(), draw_count=scal.data_ptr(), draw_index_total=scal.data_ptr() + 4)
        p.build_depth_pyramid(depth.data_ptr(), WALL[0], WALL[1], pyramid.data_ptr(), format=_lib.MIP_DEPTH_FLOAT32)
        members = int(scal[0].item())
        # the call's scratch is sized by work_capacity: the members' own bound, not N x the largest C
        c_cmds = torch.empty((8 * max(members, 1), 5), dtype=torch.int32, device=dev)
        c_scal = torch.zeros(8, dtype=torch.int32, device=dev)
        out = make_cluster_outputs(c_cmds.data_ptr(), len(c_cmds), c_scal.data_ptr(), c_scal.data_ptr() + 8,
                                   work_capacity=min(members * largest, (1 << 32) - 1), async_=True)
        occ = make_occlusion(WALL[0], WALL[1], pyramid.data_ptr(), scene.default_pv())
        legs = [("mip_batch_draws_lods, ids only (yardstick)",
                 lambda: p.batch_draws_lods(frame, bitmap.data_ptr(), policy, batch_cmds=b_cmds.data_ptr(), batch_count=b_scal.data_ptr(),
                                            instance_ids=b_ids.data_ptr(), instance_count=b_scal.data_ptr() + 4, async_=True), False),
                ("mip_cull_clusters, frustum", lambda: p.cull_clusters(frame, bitmap.data_ptr(), policy, out), True),
                ("mip_cull_clusters, frustum + pyramid", lambda: p.cull_clusters(frame, bitmap.data_ptr(), policy, out, occlusion=occ), True)]
        for name, fn, clusters in legs:
            fn()
            p.wait()
            row = dict(leg=name, config=config, n=n, members=members)
            if clusters:
                heads, survivors, w, mem = (int(v) for v in c_scal[2:6].cpu().numpy().view(np.uint32))
                row.update(W=w, survivors=survivors, commands=heads, members=mem, clusters_in_table=p.cluster_count())
            if not once:
                row.update(measure(st, fn, samples=samples))
                p.wait()
            emit(row)
        p.close()


def bench_phases(config, emit, samples=40, once=False):
    import numpy as np
    import torch

    import renderer_amd
    from renderer_amd import _lib, scene
    from renderer_amd.pipeline import (LOD_PIN_SWITCH_SQ, cluster_record_bytes, depth_pyramid_layout, make_cluster_outputs, make_cluster_record,
                                       make_frame, make_lod_policy, make_occlusion)

    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream()
    s = scene.make_scene(config)
    n, m = s["n"], len(s["meshes"])
    vertices, indices = scene.make_geometry(s["meshes"], "strips")
    with torch.cuda.stream(st):
        p = renderer_amd.InstancePipeline(n, m, stream=st.cuda_stream)
        p.set_mesh_table(s["meshes"])
        p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
        p.set_geometry(vertices, indices)
        p.build_clusters()
        largest = int(((s["meshes"]["index_len"] // 3 + 63) // 64).max())
        bitmap = torch.zeros((n + 31) // 32 + 1, dtype=torch.int32, device=dev)
        cmds = torch.empty((n, 5), dtype=torch.int32, device=dev)
        scal = torch.zeros(8, dtype=torch.int32, device=dev)
        frame = make_frame(s["planes"], s["cam_pos"])
        policy = make_lod_policy(_lib.MIP_LOD_DISTANCE, LOD_PIN_SWITCH_SQ)
        p.run_device(frame, visible_bitmap=bitmap.data_ptr(), draw_cmds=cmds.data_ptr(), draw_count=scal.data_ptr(), draw_index_total=scal.data_ptr() + 4)
        members = int(scal[0].item())
        work = min(members * largest, (1 << 32) - 1)
        pv = scene.default_pv()

        def pyramid(first_column):
            """The wall over half the width from `first_column` on (None: a cleared image), as a built pyramid."""
            depth = torch.ones((WALL[1], WALL[0]), dtype=torch.float32, device=dev)
            if first_column is not None:
                depth[:, first_column : first_column + WALL[0] // 2] = 0.0
            pyr = torch.empty(depth_pyramid_layout(*WALL)["bytes"] // 4, dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            p.build_depth_pyramid(depth.data_ptr(), WALL[0], WALL[1], pyr.data_ptr(), format=_lib.MIP_DEPTH_FLOAT32)
            return pyr, make_occlusion(WALL[0], WALL[1], pyr.data_ptr(), pv)

        old = pyramid(0)
        new = {"(a) the same wall": old, "(b) a cleared image": pyramid(None), "(c) the wall moved by 1/16 of the width": pyramid(WALL[0] // 16)}
        c_cmds = torch.empty((8 * max(members, 1), 5), dtype=torch.int32, device=dev)
        c_scal = torch.zeros(8, dtype=torch.int32, device=dev)
        out = make_cluster_outputs(c_cmds.data_ptr(), len(c_cmds), c_scal.data_ptr(), c_scal.data_ptr() + 8, work_capacity=work, async_=True)
        room = cluster_record_bytes(work)
        record = torch.zeros(room // 4, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        first, second = make_cluster_record("first", record.data_ptr(), room), make_cluster_record("second", record.data_ptr(), room)
        plain = lambda occ: (lambda: p.cull_clusters(frame, bitmap.data_ptr(), policy, out, occlusion=occ))
        run_first = lambda: p.cull_clusters_phase(frame, bitmap.data_ptr(), policy, out, old[1], first)
        legs = []
        for round_ in (1, 2):
            legs += [(f"mip_cull_clusters, the wall (round {round_})", plain(old[1])), (f"FIRST, the wall (round {round_})", run_first)]
        for name, (_, occ) in new.items():
            legs += [(f"SECOND {name}", (lambda occ=occ: p.cull_clusters_phase(frame, bitmap.data_ptr(), policy, out, occ, second))),
                     (f"yardstick: mip_cull_clusters {name}", plain(occ))]
        run_first()
        p.wait()
        candidates = int(record[2].item())
        for name, fn in legs:
            fn()
            p.wait()
            heads, survivors, w, mem = (int(v) for v in c_scal[2:6].cpu().numpy().view(np.uint32))
            row = dict(leg=name, config=config, n=n, members=mem, W=w, survivors=survivors, commands=heads, candidates=candidates, record_bytes=cluster_record_bytes(w))
            if not once:
                row.update(measure(st, fn, samples=samples))
                p.wait()
            emit(row)
        p.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samples", type=int, default=40)
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", type=int, default=0, metavar="CONFIG")
    ap.add_argument("--phases", action="store_true", help="the legs of mip_cull_clusters_phase")
    args = ap.parse_args()
    run = bench_phases if args.phases else bench
    args.out = args.out or os.path.join(ROOT, "profiles", "cluster_phases_bench.jsonl" if args.phases else "cluster_cull_bench.jsonl")
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    if args.once:
        run(args.once, emit, once=True)
        return
    for config in (3, 2):
        run(config, emit, samples=args.samples)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
