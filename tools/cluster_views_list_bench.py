#!/usr/bin/env python3
"""GPU time of the visible-cluster lists for several views in one call (mip_list_clusters_views) beside the two calls it
combines: HIP events on the launch stream around BATCH back-to-back repetitions, the legs ALTERNATING sample by sample within
one process, median of the samples, one JSON line per leg. Config 3 at 1 M instances and config 2 at 100 k,
scene.make_geometry("strips"), the pin policy; V = 4 and V = 16 views, the scene's frustum turned about the axes (the turns of
tests/cluster_view_cases.py); bitmaps culled (one mip_run_views per four views, at rest when the legs run) or NULL: the rows of
tools/cluster_views_bench.py. Legs:

  (a) mip_cull_clusters_views            the yardstick: the several-view call with its commands tail
  (b) mip_list_clusters_views            one list and one indirect draw per view
  (c) V x mip_list_clusters              one call per view on bitmaps at rest (a full bitmap where (b) takes NULL)

Every row carries W, the members, the per-view survivors, the entries written and their bytes.

  python tools/cluster_views_list_bench.py [--samples 40] [--out profiles/cluster_views_list_bench.jsonl] [--parent-library PATH]

--parent-library: leg (a) also through that library (a build of the parent commit), in fresh child processes that set
MIP_LIBRARY, alternating with this build's: parent, this build, parent, this build.
--yardstick-only: leg (a) alone (what the children run).
--once CONFIG: one warm call of each leg at V = 16 and nothing else, for a kernel trace of its own
(rocprofv3 --kernel-trace --stats -- python tools/cluster_views_list_bench.py --once 3)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.cluster_views_bench import frusta  # noqa: E402

BATCH = 20


def measure_alternating(st, legs, samples=40, warm=3):
    """{name: dict(median_us, min_us, p90_us)}: per sample every leg once, BATCH back-to-back calls between two events."""
    import numpy as np
    import torch

    for _, fn in legs:
        for _ in range(warm * BATCH):
            fn()
    st.synchronize()
    times = {name: [] for name, _ in legs}
    for _ in range(samples):
        for name, fn in legs:
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(BATCH):
                fn()
            e1.record(st)
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / BATCH * 1e3)
    out = {}
    for name, us in times.items():
        us = np.array(us)
        out[name] = dict(median_us=round(float(np.median(us)), 3), min_us=round(float(us.min()), 3), p90_us=round(float(np.percentile(us, 90)), 3))
    return out


def bench(config, emit, samples=40, once=False, yardstick_only=False, library="this build", view_counts=(4, 16)):
    import numpy as np
    import torch

    import renderer_amd
    from renderer_amd import _lib, scene
    from renderer_amd.pipeline import LOD_PIN_SWITCH_SQ, make_cluster_view_outputs, make_frame, make_lod_policy

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
        policy = make_lod_policy(_lib.MIP_LOD_DISTANCE, LOD_PIN_SWITCH_SQ)
        words = (n + 31) // 32 + 1
        full = torch.full((words,), -1, dtype=torch.int32, device=dev)
        for n_views in ((16,) if once else view_counts):
            planes = frusta(s["planes"], n_views)
            frames = [make_frame(planes[v], s["cam_pos"], first_instance_base=1000 * v) for v in range(n_views)]
            bitmaps = torch.zeros((n_views, words), dtype=torch.int32, device=dev)
            draw = torch.empty((4, n, 5), dtype=torch.int32, device=dev)
            scal = torch.zeros((n_views, 2), dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            for first in range(0, n_views, 4):   # the culled bitmaps, at rest before any leg runs
                group = list(range(first, min(first + 4, n_views)))
                prepared = [p.prepare_outputs(visible_bitmap=bitmaps[v].data_ptr(), draw_cmds=draw[k].data_ptr(), draw_count=scal[v].data_ptr(),
                                              draw_index_total=scal[v].data_ptr() + 4) for k, v in enumerate(group)]
                p.run_views([frames[v] for v in group], prepared)
                p.wait()
            visible = [int(c) for c in scal[:, 0].cpu().numpy()]
            host = bitmaps.cpu().numpy().view(np.uint32)
            union = int(np.unpackbits(np.bitwise_or.reduce(host, axis=0).view(np.uint8)).sum())
            for kind in ("culled", "NULL"):
                members = union if kind == "culled" else n
                work = min(members * largest, (1 << 32) - 1)
                cmd_stride = 2 * max(max(visible) if kind == "culled" else n, 1)   # heads are about a quarter of the members
                ptrs = [bitmaps[v].data_ptr() if kind == "culled" else 0 for v in range(n_views)]
                one_ptrs = [bitmaps[v].data_ptr() if kind == "culled" else full.data_ptr() for v in range(n_views)]
                cmds = torch.empty((n_views * cmd_stride, 5), dtype=torch.int32, device=dev)
                counts = torch.zeros(n_views, dtype=torch.int32, device=dev)
                stats = torch.zeros(2 + 2 * n_views, dtype=torch.int32, device=dev)
                torch.cuda.synchronize()
                views_out = make_cluster_view_outputs(cmds.data_ptr(), cmd_stride, counts.data_ptr(), stats.data_ptr(), work_capacity=work, async_=True)
                p.cull_clusters_views(frames, ptrs, policy, views_out)    # the survivors per view size the lists
                p.wait()
                st_host = stats.cpu().numpy().view(np.uint32)
                survivors = [int(x) for x in st_host[3::2]]
                row0 = dict(library=library, config=config, n=n, views=n_views, bitmaps=kind, W=int(st_host[0]), members=int(st_host[1]), survivors=survivors)
                legs = [("(a) mip_cull_clusters_views", lambda: p.cull_clusters_views(frames, ptrs, policy, views_out))]
                extra = {"(a) mip_cull_clusters_views": dict(heads=[int(x) for x in st_host[2::2]])}
                if not yardstick_only:
                    from renderer_amd.pipeline import make_cluster_list_outputs, make_cluster_view_list_outputs

                    stride = max(max(survivors), 1)
                    entries = torch.empty((n_views * stride, 4), dtype=torch.int32, device=dev)
                    list_counts = torch.zeros(n_views, dtype=torch.int32, device=dev)
                    args = torch.zeros((n_views, 4), dtype=torch.int32, device=dev)
                    list_stats = torch.zeros(2 + n_views, dtype=torch.int32, device=dev)
                    one_stats = torch.zeros((n_views, 3), dtype=torch.int32, device=dev)
                    one_args = torch.zeros((n_views, 4), dtype=torch.int32, device=dev)
                    torch.cuda.synchronize()
                    list_out = make_cluster_view_list_outputs(entries.data_ptr(), stride, list_counts.data_ptr(), args.data_ptr(), list_stats.data_ptr(),
                                                              work_capacity=work, async_=True)
                    ones = [make_cluster_list_outputs(entries[v * stride].data_ptr(), stride, list_counts[v].data_ptr(), one_args[v].data_ptr(),
                                                      one_stats[v].data_ptr(), work_capacity=work, async_=True) for v in range(n_views)]

                    def one_per_view():
                        for v in range(n_views):
                            p.list_clusters(frames[v], one_ptrs[v], policy, ones[v])

                    legs.append(("(b) mip_list_clusters_views", lambda: p.list_clusters_views(frames, ptrs, policy, list_out)))
                    legs.append((f"(c) {n_views} x mip_list_clusters", one_per_view))
                    written = sum(survivors)
                    for name, _ in legs[1:]:
                        extra[name] = dict(entry_stride=stride, entries=written, entry_bytes=16 * written)
                for _, fn in legs:
                    fn()
                p.wait()
                if not yardstick_only:   # the legs agree before they are timed
                    assert list_stats.cpu().numpy().view(np.uint32)[2:].tolist() == survivors, "mip_list_clusters_views' survivors"
                    assert one_stats.cpu().numpy().view(np.uint32)[:, 0].tolist() == survivors, "mip_list_clusters' survivors"
                times = {} if once else measure_alternating(st, legs, samples=samples)
                p.wait()
                for name, _ in legs:
                    row = dict(leg=name, **row0, **extra[name], **times.get(name, {}))
                    if "entry_bytes" in row and "median_us" in row:
                        row["entry_TB_per_s_of_the_call"] = round(row["entry_bytes"] / row["median_us"] * 1e-6, 4)
                    emit(row)
        p.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samples", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_views_list_bench.jsonl"))
    ap.add_argument("--once", type=int, default=0, metavar="CONFIG")
    ap.add_argument("--configs", default="3,2")
    ap.add_argument("--parent-library", default=None)
    ap.add_argument("--yardstick-only", action="store_true")
    ap.add_argument("--label", default="this build")
    args = ap.parse_args()
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    if args.once:
        bench(args.once, emit, once=True)
        return
    configs = [int(c) for c in args.configs.split(",")]
    if args.yardstick_only:
        for config in configs:
            bench(config, emit, samples=args.samples, yardstick_only=True, library=args.label)
        return
    if args.parent_library:   # leg (a) through the parent's library and this build, alternating, each in a fresh child process
        for round_ in (1, 2):
            for label, lib in ((f"parent (round {round_})", args.parent_library), (f"this build (round {round_})", None)):
                env = dict(os.environ)
                if lib:
                    env["MIP_LIBRARY"] = os.path.abspath(lib)
                else:
                    env.pop("MIP_LIBRARY", None)
                child = subprocess.run([sys.executable, os.path.abspath(__file__), "--yardstick-only", "--samples", str(args.samples), "--configs", args.configs,
                                        "--label", label], env=env, capture_output=True, text=True, check=True)
                for line in child.stdout.splitlines():
                    if line.startswith("{"):
                        emit(json.loads(line))
    for config in configs:
        bench(config, emit, samples=args.samples)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
