"""The several-view edge scenes (tests/view_edge_cases.py) through mip_cull_clusters_views and mip_batch_draws_views: the
decision catalogue under every rotation of its frames (every frame in slot 0, in a middle slot and in slot 15), the LOD rings of
the four view cameras, the six-level chain with one edge view among far ones, split decisions, instance- and box-sourced tier
edges and the sixteen distinct mask bits. Every output buffer is filled with a sentinel and compared whole — commands, counts,
stats, ids, first slots and the PAD entries behind each — against an expectation written from the instance-level decision
(never from a restatement of the views calls, never from anything a GPU computed); then against one mip_cull_clusters /
mip_batch_draws_lods call per view on the same context. Synchronously, asynchronously and, where the bits are the views' own
visibility, behind mip_run_views on the same stream with no wait in between; each set once more under the diagnostic library
with scrambled tiles. No wrong kernel is ever run: that the scenes tell the likely mistakes apart is shown on the CPU
(tests/test_view_edge_cases.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_edge_cases as ce
import decision_cases as dc
import lod_cases as lc
import test_gpu_batch as T
import test_gpu_batch_lods as TL
import test_gpu_batch_views as TBV
import test_gpu_cluster_edges as TE
import test_gpu_cluster_views as TV
import test_gpu_clusters as TC
import view_edge_cases as ve
import views_batch_restatement as vr
from renderer_amd.pipeline import make_frame, make_lod_policy

pytestmark = pytest.mark.gpu
ROOT = TC.ROOT
ra = T.ra   # the module's library fixture
ALL = ("sync", "async", "behind")


# ---- mip_cull_clusters_views ----

def _open(ra, c, max_instances):
    table, vertices, indices, boxes = c["geometry"]
    if boxes is not None:
        return TE._context(ra, table, vertices, indices, boxes, max_instances)
    p = ra.InstancePipeline(max_instances=max_instances, max_meshes=len(table))
    p.set_mesh_table(table)
    p.set_geometry(vertices, indices)
    p.build_clusters()
    return p


def _frames(c):
    return [make_frame(c["planes"][v], c["cams"][v], first_instance_base=c["bases"][v]) for v in range(len(c["planes"]))]


def _uploaded(c):
    """One device bitmap per key of c["ptr"]: views with one key share the pointer."""
    held = {k: TC._device_bitmap(ce.bits_to_bitmap(c["bits"][k])) for k in sorted(set(c["ptr"]) - {None})}
    return held, [0 if k is None else held[k].data_ptr() for k in c["ptr"]]


def _cluster_call(p, c, how, plain):
    """One call over the uploaded scene: "sync" / "async" over bitmaps at rest, "behind" over the bitmaps a mip_run_views of the
    views' own frames writes in front of it on the same stream. The outputs whole, then one mip_cull_clusters per view."""
    import torch

    n, n_views, what = c["s"]["n"], len(c["planes"]), f"{c['name']} {how}"
    frames, policy = _frames(c), make_lod_policy(c["mode"], c["switch"])
    stride = max([len(x) for x in c["want"]["cmds"]] + [1])         # the largest view fills its range to the last entry
    out = TV._ViewOut(n_views, stride)
    if how == "behind":
        culled = [v for v in range(n_views) if c["ptr"][v] == v]
        bitmaps = torch.zeros((n_views, (n + 31) // 32), dtype=torch.int32, device=T._dev())
        draw = torch.zeros((max(len(culled), 1), n, 5), dtype=torch.int32, device=T._dev())
        scal = torch.zeros((n_views, 2), dtype=torch.int32, device=T._dev())
        ptrs = [0 if k is None else bitmaps[k].data_ptr() for k in c["ptr"]]
        torch.cuda.synchronize()
        if culled:
            prepared = [p.prepare_outputs(visible_bitmap=bitmaps[v].data_ptr(), draw_cmds=draw[j].data_ptr(), draw_count=scal[v].data_ptr(),
                                          draw_index_total=scal[v].data_ptr() + 4) for j, v in enumerate(culled)]
            p.run_views([frames[v] for v in culled], prepared)      # asynchronous: prepare_outputs sets MIP_OUT_ASYNC
        p.cull_clusters_views(frames, ptrs, policy, out.outputs(async_=True))
        p.wait()
        host = bitmaps.cpu().numpy().view(np.uint32)
        for v in culled:
            assert np.array_equal(host[v], ce.bits_to_bitmap(c["bits"][v])), (what, v, "the view's own bitmap")
    else:
        held, ptrs = _uploaded(c)
        p.cull_clusters_views(frames, ptrs, policy, out.outputs(async_=how == "async"))
        if how == "async":
            p.wait()
    got = out.check(c["want"], what)
    if plain:
        TV._plain_per_view(p, c["planes"], c["cams"][0], c["bases"], ptrs, n, policy, stride, got, what)
    return got, stride


def run_cluster(ra, calls, hows=ALL, plain=True):
    """Every call in every form (the "behind" form where the bits are the views' own visibility), one context per geometry.
    Returns {name: (the buffers of the last form, cmd_stride)}."""
    out, p, key = {}, None, None
    n_max = max(c["s"]["n"] for c in calls)
    try:
        for c in calls:
            if key != id(c["geometry"][0]):
                if p is not None:
                    p.close()
                p, key = _open(ra, c, n_max), id(c["geometry"][0])
            TE._upload(p, c["s"])
            for j, how in enumerate(h for h in hows if h != "behind" or c["own_bits"]):
                out[c["name"]] = _cluster_call(p, c, how, plain and j == 0)
    finally:
        if p is not None:
            p.close()
    return out


@pytest.mark.parametrize("n_views", ["k", 16])
@pytest.mark.parametrize("case", dc.VIEW_INPUTS)
def test_catalogue_through_every_view_slot(ra, case, n_views):
    """Every size of decision_cases.SIZES under one rotation, every rotation at 257 and 513 instances."""
    n_views = len(dc.case(case)["frames"]) if n_views == "k" else n_views
    calls = [ve.frustum_call(*k) for k in ve.frustum_keys() if k[0] == case and k[2] == n_views]
    assert {c["s"]["n"] for c in calls} == set(dc.SIZES) and {c["r"] for c in calls if c["s"]["n"] == 513} == set(range(len(dc.case(case)["frames"])))
    run_cluster(ra, calls)


def test_lod_rings_are_decided_by_the_camera_of_slot_0(ra):
    run_cluster(ra, ve.calls("lod"))


@pytest.mark.parametrize("mode", [lc.DISTANCE, lc.RELATIVE])
def test_chain_follows_slot_0(ra, mode):
    run_cluster(ra, [ve.chain_call(*k) for k in ve.chain_keys() if k[0] == mode])


def test_split_decisions_beside_a_view_that_sees_everything_and_one_that_sees_nothing(ra):
    run_cluster(ra, ve.calls("split"))


def test_instance_tier_edges_under_every_views_planes(ra):
    run_cluster(ra, [ve.tier_instance_call(*k) for k in ve.tier_instance_keys()])


def _without_odd(result, c, v, odd):
    """View v's commands on the device, without those of the instances that own an odd item."""
    got, stride = result
    rows = got["cmds"][v * stride: v * stride + int(c["want"]["counts"][v])]
    return rows[~np.isin(rows[:, 4] - np.uint32(c["bases"][v]), odd)]


@pytest.mark.parametrize("kind", ce.TIER_KINDS)
def test_box_tier_edges_hold_for_every_view(ra, kind):
    keys = ve.tier_box_keys(kind)
    got = run_cluster(ra, [ve.tier_box_call(*k) for k in keys])
    # the instances that own no odd item: the device's commands are byte-identical in the twin, view by view
    for k in keys:
        odd, twin = ve.tier_box_call(*k), ve.tier_box_call(*k[:3], True)
        if k[3]:
            continue
        for v in range(len(odd["planes"])):
            mine = _without_odd(got[odd["name"]], odd, v, odd["odd_instances"])
            assert mine.tobytes() == _without_odd(got[twin["name"]], twin, v, odd["odd_instances"]).tobytes() and len(mine) > 100, (odd["name"], v)


def test_sixteen_distinct_mask_bits(ra):
    run_cluster(ra, ve.calls("mask"))


# ---- mip_batch_draws_views ----

def _batch_call(p, c, lods_too):
    """The call (asynchronous) over uploaded bitmaps; the four buffers whole; then one mip_batch_draws_lods per view."""
    s, n_views, what = c["s"], len(c["planes"]), c["name"]
    n = s["n"]
    frames, policy = _frames(c), make_lod_policy(c["mode"], c["switch"])
    held, ptrs = _uploaded(c)
    stride = vr.min_cmd_stride(s["meshes"], n)
    out = TBV._ViewBatch(n, n_views, stride)
    p.batch_draws_views(frames, ptrs, policy, async_=True, **out.kwargs())
    p.wait()
    want = c["want"]
    got = out.check(want, what)
    if lods_too:
        ones = TBV._upload(lc.all_bits(n))
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


def run_batch(ra, calls, lods_too=True):
    p, key = None, None
    n_max = max(c["s"]["n"] for c in calls)
    try:
        for c in calls:
            table = c["s"]["meshes"]
            if key != id(table):
                if p is not None:
                    p.close()
                p, key = ra.InstancePipeline(max_instances=n_max, max_meshes=len(table)), id(table)
                p.set_mesh_table(table)
            TE._upload(p, c["s"])
            _batch_call(p, c, lods_too)
    finally:
        if p is not None:
            p.close()


@pytest.mark.parametrize("padded", [False, True], ids=["one pass", "several passes"])
@pytest.mark.parametrize("which", ve.BATCH_SETS)
def test_batch_views_levels_per_view(ra, which, padded):
    calls = [c for c in ve.batch_calls(which) if c["padded"] == padded]
    assert calls and all((len(c["planes"]) * c["want"]["n_buckets"] > 256) == padded for c in calls)
    run_batch(ra, calls)


# ---- each set under the diagnostic library, tiles scrambled: asynchronous form only ----

def run_set(ra, which):
    if which == "batch":
        for b in ve.BATCH_SETS:
            run_batch(ra, ve.batch_calls(b), lods_too=False)
    else:
        run_cluster(ra, ve.calls(which), hows=("async",), plain=False)


_CHILD = r'''
import os, sys
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
os.environ["MIP_LIBRARY"] = os.path.join(root, "renderer_amd", "lib", "libmi_instance_pipeline_dbg.so")
import renderer_amd
import test_gpu_view_edges as VE
renderer_amd.load_library()
VE.run_set(renderer_amd, sys.argv[2])
print("VIEW-EDGE-SET-OK")
'''


@pytest.mark.parametrize("which", ve.SETS + ("batch",))
def test_edge_sets_in_any_dispatch_order(which):
    e = dict(os.environ, MIP_DEBUG_TILE_ORDER="scramble")
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT, which], capture_output=True, text=True, timeout=600, env=e)
    assert out.returncode == 0 and "VIEW-EDGE-SET-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
