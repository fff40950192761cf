"""The cluster-culling edge scenes (tests/cluster_edge_cases.py) through mip_build_clusters and mip_cull_clusters: the built
boxes as numbers, then every byte of the commands, the count and the stats, synchronously and asynchronously — the frustum set
also behind mip_run on the same stream over the frame's own bitmap, the Hi-Z set behind mip_build_depth_pyramid — and each set
once more under the diagnostic library with scrambled tiles. The expectation of a transfer scene is written down from the
instance-level decision (never from cluster_restatement, never from anything a GPU computed); the tier edges are owed the
restatement's literal chain. Every output buffer is filled with a sentinel and compared whole. mip_build_clusters' refusals at
their own edge. No wrong kernel is ever run: that the scenes tell the likely mistakes apart is shown on the CPU
(tests/test_cluster_edge_cases.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_edge_cases as ce
import cluster_restatement as cr
import decision_cases as dc
import lod_cases as lc
import lod_restatement as lr
import occlusion_cases as oc
import test_gpu_batch as T
import test_gpu_clusters as TC
import test_gpu_occlusion_edges as OE
from renderer_amd.pipeline import make_frame, make_lod_policy, make_occlusion

pytestmark = pytest.mark.gpu
ROOT = TC.ROOT
ra = T.ra   # the module's library fixture
INVALID = TC.INVALID
BOTH = (False, True)


def _context(ra, table, vertices, indices, want_boxes, max_instances):
    """A context over a tight geometry whose built boxes are the chosen ones (as numbers: the sign of a zero is not specified)."""
    p = ra.InstancePipeline(max_instances=max_instances, max_meshes=len(table))
    p.set_mesh_table(table)
    p.set_geometry(vertices, indices)
    p.build_clusters()
    got = p.read_cluster_boxes()
    assert got.shape == want_boxes.shape and np.array_equal(got, want_boxes), "built boxes"
    return p


def _upload(p, s):
    p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])


def _cull(p, s, want, what, mode, switch_sq, base, bits, async_, occlusion=None):
    """mip_cull_clusters over an uploaded bitmap; every output word against `want`. Returns the commands written."""
    bm = TC._device_bitmap(ce.bits_to_bitmap(bits))
    out = TC._Out(len(want["cmds"]) + 3)
    frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=base)
    p.cull_clusters(frame, bm.data_ptr(), make_lod_policy(mode, switch_sq), out.outputs(async_=async_), occlusion=occlusion)
    if async_:
        p.wait()
    TC._check(out, want["cmds"], want["stats"], f"{what} async={async_}")
    return out.result()[0][: len(want["cmds"])]


# ---- 1. the frustum set ----

def run_frustum(ra, name, frame, item_tile, asyncs=BOTH):
    table, vertices, indices, boxes = ce.frustum_geometry()
    with _context(ra, table, vertices, indices, boxes, max(dc.SIZES)) as p:
        for what, s, bits, src in ce.frustum_scenes(name, frame, item_tile):
            _upload(p, s)
            want = ce.frustum_want(s, bits)
            for async_ in asyncs:
                _cull(p, s, want, what, lr.DISTANCE, ce.PIN, ce.FRUSTUM_BASE, bits, async_)
            # behind mip_run on the same stream, no wait in between, over the frame's own bitmap
            n = s["n"]
            f = T._Frame(n)
            fr = make_frame(s["planes"], s["cam_pos"], first_instance_base=ce.FRUSTUM_BASE)
            visible = dc.decide(s)["visible"]
            want = ce.frustum_want(s, visible)
            out = TC._Out(len(want["cmds"]) + 3)
            p.run_device(fr, async_=True, **f.kwargs())
            p.cull_clusters(fr, f.bitmap.data_ptr(), make_lod_policy(lr.DISTANCE, ce.PIN), out.outputs(async_=True))
            p.wait()
            assert np.array_equal(f.host_bitmap(), ce.bits_to_bitmap(visible)), (what, "the frame's bitmap")
            TC._check(out, want["cmds"], want["stats"], what + " behind mip_run")


@pytest.mark.parametrize("name,frame", ce.FRUSTUM_INPUTS, ids=[f"{c}-{f}" for c, f in ce.FRUSTUM_INPUTS])
def test_frustum_and_pin_lod_edges(ra, tmp_path, name, frame):
    run_frustum(ra, name, frame, TC._plan_sizes(tmp_path)["item_tile"])


def run_lights_and_instance_tiers(ra, asyncs=BOTH):
    """The ring of every light with the light as the reference point, and the instances whose own position or scale sits on a
    tier limit (decision_cases.tier_scene) with their twins, over the frustum set's geometry."""
    table, vertices, indices, boxes = ce.frustum_geometry()
    with _context(ra, table, vertices, indices, boxes, max(dc.SIZES)) as p:
        scenes = [(f"light {light}", ce.light_scene(light)[0]) for light in range(dc.N_LIGHTS)]
        for kind in dc.TIER_KINDS:
            for placement in dc.TIER_PLACEMENTS:
                pair, odd = ce.instance_tier_scenes(kind, placement)
                scenes += [(f"instance tier {kind} {placement} twin={twin}", s) for twin, s in enumerate(pair)]
        for what, s in scenes:
            _upload(p, s)
            bits = np.ones(s["n"], bool)
            want = ce.frustum_want(s, bits)
            for async_ in asyncs:
                _cull(p, s, want, what, lr.DISTANCE, ce.PIN, ce.FRUSTUM_BASE, bits, async_)


def test_light_rings_and_instance_tier_edges(ra):
    run_lights_and_instance_tiers(ra)


# ---- 2. split decisions ----

def run_split(ra, name, frame, asyncs=BOTH):
    table, vertices, indices, boxes = ce.nested_geometry()
    s, labels = ce.split_scene(name, frame)
    want = ce.pattern_commands(table, ce.split_patterns(s), 9)
    with _context(ra, table, vertices, indices, boxes, s["n"]) as p:
        _upload(p, s)
        for async_ in asyncs:
            _cull(p, s, want, f"split {name}/{frame}", lr.DISTANCE, ce.PIN, 9, np.ones(s["n"], bool), async_)


@pytest.mark.parametrize("name,frame", ce.SPLIT_INPUTS)
def test_split_decisions_on_the_nested_mesh(ra, name, frame):
    run_split(ra, name, frame)


# ---- 3. the six-level chain ----

def run_chain(ra, mode, asyncs=BOTH):
    table, vertices, indices, boxes = ce.chain_geometry()
    s = ce.chain_scene(mode)
    with _context(ra, table, vertices, indices, boxes, s["n"]) as p:
        _upload(p, s)
        for short, sw in ((False, lc.SWITCH), (True, lc.SWITCH_SHORT)):
            want = ce.chain_want(s, mode, short)
            for async_ in asyncs:
                _cull(p, s, want, f"chain mode={mode} short={short}", mode, sw, ce.CHAIN_BASE, np.ones(s["n"], bool), async_)


@pytest.mark.parametrize("mode", [lc.DISTANCE, lc.RELATIVE])
def test_six_level_chain_edges(ra, mode):
    run_chain(ra, mode)


# ---- 4. Hi-Z ----

def run_occlusion(ra, name, asyncs=BOTH):
    import torch

    c, s, vertices, indices, boxes = ce.occlusion_scene(name)
    want = ce.occlusion_want(c, s)
    w, h = c["width"], c["height"]
    with _context(ra, s["meshes"], vertices, indices, boxes, s["n"]) as p:
        _upload(p, s)
        dt, pyr = OE._depth_tensor(c["depth"]), OE._pyramid_buffer(ra, w, h)
        torch.cuda.synchronize()
        occlusion = make_occlusion(w, h, pyr.data_ptr(), c["pv"])
        for async_ in asyncs:
            OE._build(ra, p, c["depth"], dt, pyr, async_=True)           # the cull follows on the same stream, no wait in between
            _cull(p, s, want, f"Hi-Z {name}", lr.DISTANCE, ce.PIN, ce.OCCLUSION_BASE, np.ones(s["n"], bool), async_, occlusion=occlusion)
        p.wait()


@pytest.mark.parametrize("name", oc.NAMES)
def test_hi_z_edges(ra, name):
    run_occlusion(ra, name)


# ---- 5. box-sourced tier edges ----

def run_tier(ra, kind, asyncs=BOTH):
    got = {}
    n_max = max(w for _, w in ce.TIER_PLACEMENTS.values())
    for twin in (False, True):
        table, vertices, indices, boxes = ce.tier_geometry(kind, twin)
        restated = cr.cluster_boxes(table, vertices, indices)
        with _context(ra, table, vertices, indices, boxes, n_max) as p:
            for placement in ce.TIER_PLACEMENTS:
                for frame in ce.TIER_FRAMES:
                    t = ce.tier_scene(kind, placement, frame)
                    s = dict(t["scene"], meshes=table)
                    bits = np.ones(s["n"], bool)
                    r = cr.cull_clusters(s, restated, ce.bits_to_bitmap(bits), lr.DISTANCE, ce.PIN, cmd_capacity=1 << 30, first_instance_base=ce.TIER_BASE)
                    assert r["status"] == 0
                    _upload(p, s)
                    for async_ in asyncs:
                        cmds = _cull(p, s, r, f"tier {kind} {placement} {frame} twin={twin}", lr.DISTANCE, ce.PIN, ce.TIER_BASE, bits, async_)
                    got[(placement, frame, twin)] = (cmds, t["odd_instances"])
    # the instances that own no odd item: the device's commands are byte-identical in the twin
    for (placement, frame, twin), (cmds, odd) in got.items():
        if not twin:
            other = got[(placement, frame, True)][0]
            mine = lambda x: x[~np.isin(x[:, 4] - np.uint32(ce.TIER_BASE), odd)]
            assert mine(cmds).tobytes() == mine(other).tobytes() and len(mine(cmds)) > 100, (kind, placement, frame)


@pytest.mark.parametrize("kind", ce.TIER_KINDS)
def test_box_sourced_tier_edges(ra, kind):
    run_tier(ra, kind)


# ---- each set under the diagnostic library, tiles scrambled ----

def run_set(ra, which, item_tile):
    if which == "frustum":
        for name, frame in ce.FRUSTUM_INPUTS:
            run_frustum(ra, name, frame, item_tile, asyncs=(True,))
        run_lights_and_instance_tiers(ra, asyncs=(True,))
    elif which == "split":
        for name, frame in ce.SPLIT_INPUTS:
            run_split(ra, name, frame, asyncs=(True,))
    elif which == "chain":
        for mode in (lc.DISTANCE, lc.RELATIVE):
            run_chain(ra, mode, asyncs=(True,))
    elif which == "hi-z":
        for name in oc.NAMES:
            run_occlusion(ra, name, asyncs=(True,))
    elif which == "tier":
        for kind in ce.TIER_KINDS:
            run_tier(ra, kind, asyncs=(True,))
    else:
        raise KeyError(which)


SETS = ("frustum", "split", "chain", "hi-z", "tier")

_CHILD = r'''
import os, sys
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
os.environ["MIP_LIBRARY"] = os.path.join(root, "renderer_amd", "lib", "libmi_instance_pipeline_dbg.so")
import renderer_amd
import test_gpu_clusters as TC
import test_gpu_cluster_edges as TE
renderer_amd.load_library()
TE.run_set(renderer_amd, sys.argv[3], TC._plan_sizes(sys.argv[2])["item_tile"])
print("CLUSTER-EDGE-SET-OK")
'''


@pytest.mark.parametrize("which", SETS)
def test_edge_sets_in_any_dispatch_order(which, tmp_path):
    e = dict(os.environ, MIP_DEBUG_TILE_ORDER="scramble")
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(tmp_path), which], capture_output=True, text=True, timeout=600, env=e)
    assert out.returncode == 0 and "CLUSTER-EDGE-SET-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ---- mip_build_clusters: the refusals at their own edge ----

def test_build_refusals_at_their_own_edge(ra):
    g = ce.refusal_geometry()
    table, vertices, indices = g["table"], g["vertices"], g["indices"]
    want = cr.cluster_boxes(table, vertices, indices)
    with ra.InstancePipeline(max_instances=4, max_meshes=1) as p:
        p.set_mesh_table(table)
        # vertex_offset + largest used index == n_vertices - 1: accepted, the boxes are right — and the index tail (8 % 3 = 2
        # trailing indices, far out of range) belongs to no cluster, so it is not checked
        p.set_geometry(vertices, indices)
        p.build_clusters()
        assert p.cluster_count() == 1 and np.array_equal(p.read_cluster_boxes(), want)
        # == n_vertices: refused, and no table is left behind
        p.set_geometry(vertices[:-1], indices)
        with pytest.raises(ra.MipError) as e:
            p.build_clusters()
        assert e.value.code == INVALID and "vertex_offset" in str(e.value) and p.cluster_count() == 0
        # the same index out of range INSIDE the triangles: refused
        inside = indices.copy()
        inside[5] = indices[-1]
        p.set_geometry(vertices, inside)
        with pytest.raises(ra.MipError) as e:
            p.build_clusters()
        assert e.value.code == INVALID and p.cluster_count() == 0
        # vertex_offset < 0: refused, whatever the indices
        negative = table.copy()
        negative["vertex_offset"] = -1
        p.set_mesh_table(negative)
        p.set_geometry(vertices, indices)
        with pytest.raises(ra.MipError) as e:
            p.build_clusters()
        assert e.value.code == INVALID and "vertex_offset -1" in str(e.value) and p.cluster_count() == 0
        # and the context is usable again
        p.set_mesh_table(table)
        p.build_clusters()
        assert np.array_equal(p.read_cluster_boxes(), want)
