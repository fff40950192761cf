#!/usr/bin/env python3
"""GPU time of the two-phase visible-cluster list (mip_list_clusters_phase) beside the command call of the same phase
(mip_cull_clusters_phase) and, for FIRST, beside mip_list_clusters under the same pyramid, by the method of
tools/cluster_bench.py and tools/cluster_list_bench.py: HIP events on the launch stream around 20 back-to-back calls, the median
of 40 samples, one JSON line per leg. The calls of a row ALTERNATE in one process — 10 samples of one, 10 of the next, four
times — so that all see the same clocks; the bitmap is the one a mip_run of the scene wrote and stays at rest. Rows: FIRST under
the wall pyramid of tools/cluster_bench.py; SECOND over FIRST's record (a) under the same wall, (b) under a cleared image, (c)
under the wall moved by 1/16 of the width. SECOND's list call appends behind FIRST's entries through FIRST's entry_count.
Config 3 at 1 M instances and config 2 at 100 k, "strips" geometry, the pin policy.

  python tools/cluster_list_phase_bench.py [--samples 40] [--out profiles/cluster_list_phase_bench.jsonl]

--once CONFIG: one warm call of every leg and nothing else, for a kernel trace of its own
(rocprofv3 --kernel-trace --stats -- python tools/cluster_list_phase_bench.py --once 3).

FRONTS names the fronts of the list call a row is measured with: (label, environment variable that selects it, or None). The
shipped library has one front; a measurement build that keeps a second one behind an environment variable read per call is
measured by adding it here (DESIGN section 34 did so for the composed front before removing it)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from tools.cluster_bench import WALL  # noqa: E402
from tools.cluster_list_bench import BATCH, sample, summary  # noqa: E402

FRONTS = (("search-free", None),)


def _front(env):
    """Select a front for the calls that follow."""
    for _, e in FRONTS:
        if e:
            os.environ.pop(e, None)
    if env:
        os.environ[env] = "1"


def bench(config, emit, samples=40, once=False):
    import numpy as np
    import torch

    import renderer_amd
    from renderer_amd import _lib, scene
    from renderer_amd.pipeline import (LOD_PIN_SWITCH_SQ, cluster_record_bytes, depth_pyramid_layout, make_cluster_list_outputs, make_cluster_outputs,
                                       make_cluster_phase_list_outputs, make_cluster_record, make_frame, make_lod_policy, make_occlusion)

    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream()
    s = scene.make_scene(config)
    n, m = s["n"], len(s["meshes"])
    pv = scene.default_pv()
    vertices, indices = scene.make_geometry(s["meshes"], "strips")
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
        members = int(scal[:1].cpu().numpy().view(np.uint32)[0])
        policy = make_lod_policy(_lib.MIP_LOD_DISTANCE, LOD_PIN_SWITCH_SQ)
        largest = int(((s["meshes"]["index_len"] // 3 + 63) // 64).max())
        work = min(members * largest, (1 << 32) - 1)

        def pyramid_of(first_column):
            depth = torch.ones((WALL[1], WALL[0]), dtype=torch.float32, device=dev)
            if first_column is not None:
                depth[:, first_column: first_column + WALL[0] // 2] = 0.0
            pyramid = torch.empty(depth_pyramid_layout(*WALL)["bytes"] // 4, dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            p.build_depth_pyramid(depth.data_ptr(), WALL[0], WALL[1], pyramid.data_ptr(), format=_lib.MIP_DEPTH_FLOAT32)
            return pyramid, make_occlusion(WALL[0], WALL[1], pyramid.data_ptr(), pv)

        old = pyramid_of(0)
        seconds = (("SECOND (a) the same wall", old), ("SECOND (b) a cleared image", pyramid_of(None)), ("SECOND (c) the wall moved by 1/16", pyramid_of(WALL[0] // 16)))
        c_cmds = torch.empty(((work + members) // 2 + 1, 5), dtype=torch.int32, device=dev)   # a member of C clusters has at most ceil(C / 2) runs
        c_scal = torch.zeros(8, dtype=torch.int32, device=dev)
        entries = torch.empty((work, 4), dtype=torch.int32, device=dev)    # FIRST's and SECOND's lists never hold more than W entries together
        plain_entries = torch.empty((work, 4), dtype=torch.int32, device=dev)
        l_scal = torch.zeros(36, dtype=torch.int32, device=dev)            # [0:12] FIRST, [12:24] SECOND, [24:36] mip_list_clusters
        record = torch.zeros(cluster_record_bytes(work) // 4, dtype=torch.int32, device=dev)
        c_record = torch.zeros(cluster_record_bytes(work) // 4, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        sp = l_scal.data_ptr()
        commands = make_cluster_outputs(c_cmds.data_ptr(), len(c_cmds), c_scal.data_ptr(), c_scal.data_ptr() + 8, work_capacity=work, async_=True)
        listed = make_cluster_list_outputs(plain_entries.data_ptr(), work, sp + 96, sp + 104, sp + 120, work_capacity=work, async_=True)
        first_out = make_cluster_phase_list_outputs(entries.data_ptr(), work, sp, sp + 8, sp + 24, work_capacity=work, async_=True)
        second_out = make_cluster_phase_list_outputs(entries.data_ptr(), work, sp + 48, sp + 56, sp + 72, work_capacity=work, async_=True, entry_base=sp)
        rec = lambda buf, phase: make_cluster_record(phase, buf.data_ptr(), 4 * len(buf))   # noqa: E731
        bm = bitmap.data_ptr()

        def measure(row_name, legs, read):
            """legs: [(leg, front env or None, fn)]; read(): dict of the row's counts, after one warm call of every leg."""
            for _, env, fn in legs:
                _front(env)
                fn()
            p.wait()
            common = dict(config=config, n=n, row=row_name, **read())
            rows = [dict(leg=leg, **common) for leg, _, _ in legs]
            if not once:
                us = [[] for _ in legs]
                for _, env, fn in legs:       # warm
                    _front(env)
                    for _ in range(3 * BATCH):
                        fn()
                st.synchronize()
                for _ in range(4):            # alternate: 4 x (samples / 4) of each
                    for which, (_, env, fn) in enumerate(legs):
                        _front(env)
                        us[which].extend(sample(st, fn, max(samples // 4, 1)))
                p.wait()
                for row, series in zip(rows, us):
                    row.update(summary(series))
                for row in rows[1:]:
                    row["over_the_command_call"] = round(row["median_us"] / rows[0]["median_us"], 4)
            _front(None)
            for row in rows:
                emit(row)

        u32 = lambda t: [int(v) for v in t.cpu().numpy().view(np.uint32)]   # noqa: E731

        def read_first():
            heads, survivors, w, mem = u32(c_scal[2:6])
            count, l_survivors, l_w, l_mem, candidates = u32(l_scal[[0, 6, 7, 8, 9]])
            assert (l_survivors, l_w, l_mem) == (survivors, w, mem) and count == survivors and u32(l_scal[[24, 30]]) == [survivors, survivors]
            assert u32(record[:4]) == [w, mem, candidates, 0] == u32(c_record[:4])
            return dict(W=w, members=mem, survivors=survivors, candidates=candidates, commands=heads, command_bytes=20 * heads, entry_bytes=16 * count)

        legs = [("mip_cull_clusters_phase FIRST", None, lambda: p.cull_clusters_phase(frame, bm, policy, commands, old[1], rec(c_record, "first"))),
                ("mip_list_clusters, the same pyramid", None, lambda: p.list_clusters(frame, bm, policy, listed, occlusion=old[1]))]
        legs += [(f"mip_list_clusters_phase FIRST, {label} front", env, lambda: p.list_clusters_phase(frame, bm, policy, first_out, old[1], rec(record, "first")))
                 for label, env in FRONTS]
        measure("FIRST", legs, read_first)
        for row_name, (_, occ) in seconds:
            def read_second():
                heads, survivors, w, mem = u32(c_scal[2:6])
                count, base, l_survivors, l_w, l_mem, candidates = u32(l_scal[[12, 17, 18, 19, 20, 21]])
                assert (l_survivors, l_w, l_mem) == (survivors, w, mem) and count == survivors and base == u32(l_scal[:1])[0]
                return dict(W=w, members=mem, survivors=survivors, candidates=candidates, entry_base=base, commands=heads, command_bytes=20 * heads,
                            entry_bytes=16 * count)

            legs = [("mip_cull_clusters_phase SECOND", None, lambda occ=occ: p.cull_clusters_phase(frame, bm, policy, commands, occ, rec(c_record, "second")))]
            legs += [(f"mip_list_clusters_phase SECOND, {label} front", env, lambda occ=occ: p.list_clusters_phase(frame, bm, policy, second_out, occ, rec(record, "second")))
                     for label, env in FRONTS]
            measure(row_name, legs, read_second)
        p.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samples", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_list_phase_bench.jsonl"))
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
