#!/usr/bin/env python3
"""GPU time of the visible-cluster lists for several views with a depth pyramid per view
(mip_list_clusters_views_occluded) beside what a renderer had before it: HIP events on the launch stream around BATCH
back-to-back repetitions, the legs ALTERNATING sample by sample within one process, median of the samples, one JSON line per
leg. Config 3 at 1 M instances and config 2 at 100 k, scene.make_geometry("strips"), the pin policy; V = 4 and V = 16 views,
the scene's frustum turned about the axes (the turns of tests/cluster_view_cases.py); bitmaps culled (one mip_run_views per
four views, at rest when the legs run) or NULL: the rows of tools/cluster_views_list_bench.py. View v's depth image is the
64 x 32 wall of the tests — the near plane over columns [c, c + 32), c = (0, 16, 32)[v % 3] — in a pyramid of its own, under
scene.default_pv() turned as the view's planes are. Legs:

  (i)         mip_list_clusters_views_occluded   a wall pyramid per view, `hidden` given; the library's default cull kernel (packed)
  (i-alt)     the same call                      the other cull kernel (the simple loop), through MIP_TUNE_VIEWS_OCCLUDED_PACKED
  (ii)        V x mip_list_clusters(occ)         the yardstick: one call per view with the same occ, on bitmaps at rest (a full
                                                 bitmap where (i) takes NULL)
  (iii)       mip_list_clusters_views            no pyramid: what the pyramid leg of (i) costs on top
  (iv)        mip_list_clusters_views_occluded   every occs[v] NULL: must read as (iii) (the host launches the plain cull kernel)
  (iv-simple) the same, forced through the simple-loop occluded kernel (MIP_TUNE_VIEWS_OCCLUDED_ALWAYS): what a view without a
  (iv-packed) pyramid costs inside each occluded kernel
  (iii')      mip_list_clusters_views again      the same call as (iii) in the same session: the noise (iv) is read against

Every row carries W, the members, the per-view survivors with and without the pyramids, hidden, the entries written and
their bytes.

  python tools/cluster_views_occluded_bench.py [--samples 40] [--out profiles/cluster_views_occluded_bench.jsonl]

--once CONFIG: one warm call of legs (i), (i-alt), (ii) and (iii) at V = 16 over NULL bitmaps and nothing else, for a kernel trace of
its own (rocprofv3 --kernel-trace --stats -- python tools/cluster_views_occluded_bench.py --once 3)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.cluster_views_bench import frusta  # noqa: E402
from tools.cluster_views_list_bench import measure_alternating  # noqa: E402

TURNS = [(0, 1, 2, 1, 1), (2, 1, 0, 1, 1), (0, 1, 2, -1, 1), (2, 1, 0, -1, 1), (0, 2, 1, 1, 1), (0, 1, 2, 1, -1)]   # those of frusta()
WALLS = (0, 16, 32)
DEFAULT_PACKED = "1"   # the library's default cull kernel: "1" packed, "0" the simple loop (api_cluster.hip)


def turned_pv(pv, turn):
    """pv (column-major storage) turned as frusta() turns the planes: columns [a, b, c, 3], column 0 times sx, column 2 times sz."""
    import numpy as np

    a, b, c, sx, sz = turn
    t = np.asarray(pv, np.float32).reshape(4, 4)[[a, b, c, 3]].copy()
    t[0] *= sx
    t[2] *= sz
    return np.ascontiguousarray(t.reshape(16))


def bench(config, emit, samples=40, once=False, view_counts=(4, 16)):
    import numpy as np
    import torch

    import renderer_amd
    from renderer_amd import _lib, scene
    from renderer_amd.pipeline import (LOD_PIN_SWITCH_SQ, depth_pyramid_layout, make_cluster_list_outputs, make_cluster_view_list_outputs,
                                       make_cluster_view_occluded_list_outputs, make_frame, make_lod_policy, make_occlusion)

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
        pyramid_floats = depth_pyramid_layout(64, 32)["bytes"] // 4
        probe = np.arange(24, dtype=np.float32) + 1   # TURNS are frusta()'s: the planes and the pv of a view turn together
        for v, (ta, tb, tc, sx, sz) in enumerate(TURNS):
            want = probe.reshape(6, 4)[:, [ta, tb, tc, 3]].copy()
            want[:, 0] *= sx
            want[:, 2] *= sz
            assert np.asarray(frusta(probe, v + 1)[v], np.float32).reshape(-1).tolist() == want.reshape(-1).tolist(), "TURNS differ from frusta()"
        for n_views in ((16,) if once else view_counts):
            planes = frusta(s["planes"], n_views)
            frames = [make_frame(planes[v], s["cam_pos"], first_instance_base=1000 * v) for v in range(n_views)]
            # a depth image and a pyramid of its own per view, built once and at rest when the legs run
            depth = torch.ones((n_views, 32, 64), dtype=torch.float32, device=dev)
            for v in range(n_views):
                depth[v, :, WALLS[v % 3]: WALLS[v % 3] + 32] = 0.0
            pyramids = torch.zeros((n_views, pyramid_floats), dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            for v in range(n_views):
                p.build_depth_pyramid(depth[v].data_ptr(), 64, 32, pyramids[v].data_ptr(), format=_lib.MIP_DEPTH_FLOAT32, async_=True)
            p.wait()
            occs = [make_occlusion(64, 32, pyramids[v].data_ptr(), turned_pv(scene.default_pv(), TURNS[v % len(TURNS)])) for v in range(n_views)]
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
            host = bitmaps.cpu().numpy().view(np.uint32)
            union = int(np.unpackbits(np.bitwise_or.reduce(host, axis=0).view(np.uint8)).sum())
            for kind in (("NULL",) if once else ("culled", "NULL")):
                members = union if kind == "culled" else n
                work = min(members * largest, (1 << 32) - 1)
                ptrs = [bitmaps[v].data_ptr() if kind == "culled" else 0 for v in range(n_views)]
                one_ptrs = [bitmaps[v].data_ptr() if kind == "culled" else full.data_ptr() for v in range(n_views)]
                # the plain several-view call first: its survivors size the lists
                probe_stats = torch.zeros(2 + n_views, dtype=torch.int32, device=dev)
                probe_counts = torch.zeros(n_views, dtype=torch.int32, device=dev)
                probe_entries = torch.empty((16, 4), dtype=torch.int32, device=dev)
                torch.cuda.synchronize()
                try:
                    p.list_clusters_views(frames, ptrs, policy, make_cluster_view_list_outputs(probe_entries.data_ptr(), 1, probe_counts.data_ptr(), 0,
                                                                                              probe_stats.data_ptr(), work_capacity=work))
                except renderer_amd.MipError:   # an entry overflow, expected: the stats are true
                    pass
                st_host = probe_stats.cpu().numpy().view(np.uint32)
                free = [int(x) for x in st_host[2:]]
                stride = max(max(free), 1)
                entries = torch.empty((n_views * stride, 4), dtype=torch.int32, device=dev)
                counts = torch.zeros(n_views, dtype=torch.int32, device=dev)
                args = torch.zeros((n_views, 4), dtype=torch.int32, device=dev)
                stats = torch.zeros(2 + n_views, dtype=torch.int32, device=dev)
                hidden = torch.zeros(n_views, dtype=torch.int32, device=dev)
                bare_stats = torch.zeros(2 + n_views, dtype=torch.int32, device=dev)
                plain_stats = torch.zeros(2 + n_views, dtype=torch.int32, device=dev)
                one_stats = torch.zeros((n_views, 3), dtype=torch.int32, device=dev)
                one_args = torch.zeros((n_views, 4), dtype=torch.int32, device=dev)
                torch.cuda.synchronize()
                occluded_out = make_cluster_view_occluded_list_outputs(entries.data_ptr(), stride, counts.data_ptr(), args.data_ptr(), stats.data_ptr(),
                                                                       hidden.data_ptr(), work_capacity=work, async_=True)
                bare_out = make_cluster_view_occluded_list_outputs(entries.data_ptr(), stride, counts.data_ptr(), args.data_ptr(), bare_stats.data_ptr(),
                                                                   0, work_capacity=work, async_=True)
                plain_out = make_cluster_view_list_outputs(entries.data_ptr(), stride, counts.data_ptr(), args.data_ptr(), plain_stats.data_ptr(),
                                                           work_capacity=work, async_=True)
                ones = [make_cluster_list_outputs(entries[v * stride].data_ptr(), stride, counts[v].data_ptr(), one_args[v].data_ptr(),
                                                  one_stats[v].data_ptr(), work_capacity=work, async_=True) for v in range(n_views)]
                none = [None] * n_views

                def one_per_view():
                    for v in range(n_views):
                        p.list_clusters(frames[v], one_ptrs[v], policy, ones[v], occlusion=occs[v])

                def tuned(packed, always, occlusions, out):
                    """The call under the library's tuning switches (read per call): the packed cull kernel or the simple loop,
                    and the occluded kernel even when no view has a pyramid."""
                    def call():
                        os.environ["MIP_TUNE_VIEWS_OCCLUDED_PACKED"] = packed
                        if always:
                            os.environ["MIP_TUNE_VIEWS_OCCLUDED_ALWAYS"] = "1"
                        else:
                            os.environ.pop("MIP_TUNE_VIEWS_OCCLUDED_ALWAYS", None)
                        p.list_clusters_views_occluded(frames, ptrs, occlusions, policy, out)
                    return call

                legs = [("(i) mip_list_clusters_views_occluded", tuned(DEFAULT_PACKED, False, occs, occluded_out)),
                        ("(i-alt) the same, the other cull kernel (%s)" % ("simple loop" if DEFAULT_PACKED == "1" else "packed"),
                         tuned("0" if DEFAULT_PACKED == "1" else "1", False, occs, occluded_out)),
                        (f"(ii) {n_views} x mip_list_clusters(occ)", one_per_view),
                        ("(iii) mip_list_clusters_views", lambda: p.list_clusters_views(frames, ptrs, policy, plain_out))]
                if not once:
                    legs += [("(iv) mip_list_clusters_views_occluded, no pyramid", tuned(DEFAULT_PACKED, False, none, bare_out)),
                             ("(iv-simple) no pyramid, forced through the simple-loop occluded kernel", tuned("0", True, none, bare_out)),
                             ("(iv-packed) no pyramid, forced through the packed occluded kernel", tuned("1", True, none, bare_out)),
                             ("(iii') mip_list_clusters_views again", lambda: p.list_clusters_views(frames, ptrs, policy, plain_out))]
                for _, fn in legs:
                    fn()
                p.wait()
                walled = [int(x) for x in stats.cpu().numpy().view(np.uint32)[2:]]
                gone = [int(x) for x in hidden.cpu().numpy().view(np.uint32)]
                # the legs agree before they are timed
                assert one_stats.cpu().numpy().view(np.uint32)[:, 0].tolist() == walled, "mip_list_clusters' survivors under the pyramids"
                assert plain_stats.cpu().numpy().view(np.uint32)[2:].tolist() == free, "mip_list_clusters_views' survivors"
                assert [a + b for a, b in zip(walled, gone)] == free, "survivors + hidden"
                if not once:
                    assert bare_stats.cpu().numpy().view(np.uint32).tolist() == plain_stats.cpu().numpy().view(np.uint32).tolist(), "no pyramid: the plain call's stats"
                row0 = dict(library="this build", config=config, n=n, views=n_views, bitmaps=kind, W=int(st_host[0]), members=int(st_host[1]),
                            survivors_without_pyramids=free, entry_stride=stride)
                times = {} if once else measure_alternating(st, legs, samples=samples)
                p.wait()
                for name, _ in legs:
                    under = name.startswith(("(i)", "(i-alt)", "(ii)"))   # the legs that test against the pyramids
                    written = sum(walled) if under else sum(free)
                    row = dict(leg=name, **row0, survivors=walled if under else free, hidden=gone if under else [0] * n_views,
                               entries=written, entry_bytes=16 * written, **times.get(name, {}))
                    emit(row)
                if times:
                    t = {name.split(" ")[0]: times[name]["median_us"] for name, _ in legs}
                    emit(dict(leg="ratios", config=config, n=n, views=n_views, bitmaps=kind,
                              one_call_over_V_calls=round(t["(i)"] / t["(ii)"], 4), other_kernel_over_this=round(t["(i-alt)"] / t["(i)"], 4),
                              pyramid_leg_us=round(t["(i)"] - t["(iii)"], 3), no_pyramid_over_plain=round(t["(iv)"] / t["(iii)"], 4),
                              no_pyramid_through_simple_over_plain=round(t["(iv-simple)"] / t["(iii)"], 4),
                              no_pyramid_through_packed_over_plain=round(t["(iv-packed)"] / t["(iii)"], 4),
                              plain_again_over_plain=round(t["(iii')"] / t["(iii)"], 4)))
        p.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samples", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_views_occluded_bench.jsonl"))
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
    for config in [int(c) for c in args.configs.split(",")]:
        bench(config, emit, samples=args.samples)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
