"""Cluster culling in two phases on the GPU (include/mi_instance_pipeline.h, mip_cull_clusters_phase): every byte of both phases'
commands, counts and stats and of the record against the hand-written scenes (tests/cluster_phase_cases.py), the numpy
restatement (tests/cluster_phase_restatement.py) over config 3 under three new pyramids, the structural edges of W, the
occlusion test's own decision edges, the overflow and not-its-record contracts, every refusal, and two frames in flight with no
host wait; the scenes once more under the diagnostic library with reversed and scrambled tiles. Every buffer — the record
included — is filled with a sentinel and compared whole. Not reference behaviour: parity is with the restatement."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_edge_cases as ce
import cluster_phase_cases as pc
import cluster_phase_restatement as pr
import cluster_restatement as cr
import lod_restatement as lr
import numpy_restatement as nr
import occlusion_cases as oc
import occlusion_restatement as orr
import test_gpu_batch as T
import test_gpu_batch_lods as TL
import test_gpu_clusters as TC
import test_gpu_occlusion as TO
import test_gpu_occlusion_edges as OE
from renderer_amd import _lib
from renderer_amd.pipeline import cluster_record_bytes, make_cluster_record, make_frame, make_lod_policy, make_occlusion

pytestmark = pytest.mark.gpu
ROOT = TC.ROOT
SENTINEL = T.SENTINEL
ra = T.ra   # the module's library fixture
INVALID, CAPACITY, DEVICE = -1, -4, -5
GUARD = 6   # sentinel words behind the record's room
BOTH = (False, True)


class _Record:
    """The caller's record on the device, filled with a sentinel: room for `w` work items and GUARD words nobody may touch."""

    def __init__(self, w):
        import torch

        self.bytes = cluster_record_bytes(w)
        self.buf = torch.full((self.bytes // 4 + GUARD,), T._i32(SENTINEL), dtype=torch.int32, device=T._dev())
        torch.cuda.synchronize()

    def arg(self, phase, room=None):
        return make_cluster_record(phase, self.buf.data_ptr(), self.bytes if room is None else room)

    def words(self):
        import torch

        torch.cuda.synchronize()
        return self.buf.cpu().numpy().view(np.uint32)

    def check(self, want, what):
        """The first len(want) words are `want`, every word behind them is the sentinel."""
        got = self.words()
        assert got[: len(want)].tolist() == np.asarray(want, np.uint32).tolist(), (what, "record", got[:8].tolist(), np.asarray(want)[:8].tolist())
        assert (got[len(want):] == SENTINEL).all(), (what, "written behind the record")


class _Pyramid:
    """A depth image on the device and room for its pyramid; build() enqueues mip_build_depth_pyramid, asynchronously."""

    def __init__(self, ra, depth, pv):
        self.depth = depth
        self.dt, self.pyr = OE._depth_tensor(depth), OE._pyramid_buffer(ra, depth.shape[1], depth.shape[0])
        self.occ = make_occlusion(depth.shape[1], depth.shape[0], self.pyr.data_ptr(), pv)

    def build(self, ra, p):
        OE._build(ra, p, self.depth, self.dt, self.pyr, async_=True)
        return self.occ


def _phase(p, frame, bitmap, policy, occ, rec, want, what, cmd_capacity=None, work_capacity=0, async_=False, expect=0, count=None):
    """One mip_cull_clusters_phase call; the commands, the count and the stats against want (dict(cmds, stats))."""
    out = TC._Out((len(want["cmds"]) if cmd_capacity is None else cmd_capacity) + 3)
    raised = 0
    try:
        p.cull_clusters_phase(frame, bitmap, policy, out.outputs(cmd_capacity, work_capacity, async_), occ, rec)
        if async_:
            p.wait()
    except Exception as e:   # MipError of the library under test (the product's or the diagnostic one's)
        raised = e.code
    assert raised == expect, (what, raised, expect)
    if expect:
        p.wait()              # reported once
    TC._check(out, want["cmds"], want["stats"], what, count=count)
    return out


def run_scene(ra, p, s, want, what, asyncs=BOTH, mode=lr.DISTANCE, switch_sq=pc.PIN):
    """FIRST under the scene's old pyramid, SECOND under its new one and under planes that accept nothing, the pyramid builds
    and the calls with no wait in between; both calls' outputs and the record whole."""
    import torch

    bm = TC._device_bitmap(s["bitmap"])
    old, new = _Pyramid(ra, s["old_depth"], s["pv"]), _Pyramid(ra, want["new_depth"], s["pv"])
    torch.cuda.synchronize()
    policy = make_lod_policy(mode, switch_sq)
    f1 = make_frame(s["planes"], s["cam_pos"], first_instance_base=s["base"])
    f2 = make_frame(s.get("second_planes", s["planes"]), s["cam_pos"], first_instance_base=s["base"])
    for async_ in asyncs:
        rec = _Record(int(want["first"]["stats"][2]))
        _phase(p, f1, bm.data_ptr(), policy, old.build(ra, p), rec.arg("first"), want["first"], what + " FIRST", async_=async_)
        rec.check(want["record"], what + " FIRST")
        _phase(p, f2, bm.data_ptr(), policy, new.build(ra, p), rec.arg("second"), want["second"], what + " SECOND", async_=async_)
        rec.check(want["record"], what + " SECOND leaves the record alone")
    p.wait()


# ---- 1. the scenes of the CPU tests ----

_CASES = pc.cases()


def run_hand_cases(ra, asyncs=BOTH):
    for name, s, want in _CASES:
        with TC._pipeline(ra, s, s["vertices"], s["indices"]) as p:
            run_scene(ra, p, s, want, name, asyncs)


@pytest.mark.parametrize("name,s,want", _CASES, ids=[c[0] for c in _CASES])
def test_hand_cases(ra, name, s, want):
    with TC._pipeline(ra, s, s["vertices"], s["indices"]) as p:
        run_scene(ra, p, s, want, name)


def _wall(first_column):
    depth = np.ones((32, 64), np.float32)
    if first_column is not None:
        depth[:, first_column : first_column + 32] = 0.0
    return depth


def run_config_3(ra, n, asyncs=(True,)):
    """config 3 under the wall; SECOND under the same wall, a cleared image and the wall moved by a quarter of the width."""
    ordering = "strips" if n == 257 else "rows" if n % 2 else "shuffled"
    s = TL._sized(ra.scene.make_scene(3, n=max(n, 1)), n)
    vertices, indices = ra.scene.make_geometry(s["meshes"], ordering)
    boxes = cr.cluster_boxes(s["meshes"], vertices, indices)
    bitmap = orr.bitmap_of(~nr.run(s)["coarse_culled"]) if n else np.zeros(0, np.uint32)
    pv = ra.scene.default_pv()
    occ_of = lambda depth: dict(pv=pv, levels=orr.pyramid_levels(depth), width=64, height=32)
    base = 0xFFFFFFFF - n // 2                        # wraps inside the scene
    args = (s, boxes, bitmap, lr.DISTANCE, lr.PIN_SWITCH_SQ, 1 << 30)
    f = pr.first(*args, occ_of(_wall(0)), first_instance_base=base)
    scene = dict(s, bitmap=bitmap, base=base, pv=pv, old_depth=_wall(0), second_planes=pc.SECOND_PLANES)
    survivors = []
    with TC._pipeline(ra, s, vertices, indices) as p:
        for column in (0, None, 16):
            g = pr.second(*args, occ_of(_wall(column)), f["record"], first_instance_base=base)
            assert f["status"] == 0 and g["status"] == 0
            run_scene(ra, p, scene, dict(first=f, second=g, record=f["record"], new_depth=_wall(column)), f"config 3 n={n} wall at {column}", asyncs,
                      switch_sq=lr.PIN_SWITCH_SQ)
            survivors.append(int(g["stats"][1]))
    if n >= 257:
        assert survivors[0] == 0 < survivors[2] < survivors[1] == int(f["record"][2])


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 4097])
def test_restatement_over_config_3(ra, n):
    run_config_3(ra, n)


# ---- 2. the edges of W ----

def _edge_scenes(sizes):
    """[(name, scene, want)]: W one below, at and one above a record word, the item tile and the head tile, every item a candidate
    and alternating candidate words; three item tiles of which only the last holds candidates."""
    out = []
    for edge in (64, sizes["item_tile"], sizes["head_tile"]):
        for w in (edge - 1, edge, edge + 1):
            out.append((f"W={w}, every item a candidate", *pc.filled(w, lambda j, k: "H" * k, base=1)))
            out.append((f"W={w}, alternating candidate words", *pc.filled(w, lambda j, k: ("H" if j % 2 == 0 else "V") * k, base=2)))
    per = sizes["item_tile"] // 64
    out.append(("candidates in the last of three item tiles", *pc.filled(3 * sizes["item_tile"], lambda j, k: ("H" if j >= 2 * per else "V") * k, base=3)))
    return out


def run_edge_scenes(ra, sizes):
    for name, s, want in _edge_scenes(sizes):
        assert int(want["first"]["stats"][2]) == len(pr.unpack_record(want["record"], int(want["record"][0])))
        with TC._pipeline(ra, s, s["vertices"], s["indices"]) as p:
            run_scene(ra, p, s, want, name, asyncs=(True,))


def test_w_edges(ra, tmp_path):
    sizes = TC._plan_sizes(tmp_path)
    by = {name: want for name, _, want in _edge_scenes(sizes)}
    for edge in (64, sizes["item_tile"], sizes["head_tile"]):
        assert {int(w["record"][0]) for w in by.values()} >= {edge - 1, edge, edge + 1}
    last = by["candidates in the last of three item tiles"]["record"][4:].view(np.uint64)
    assert (last[: 2 * sizes["item_tile"] // 64] == 0).all() and (last[2 * sizes["item_tile"] // 64 :] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
    run_edge_scenes(ra, sizes)


# ---- 3. all of it in any dispatch order ----

_CHILD = r'''
import os, sys
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
os.environ["MIP_LIBRARY"] = os.path.join(root, "renderer_amd", "lib", "libmi_instance_pipeline_dbg.so")
import renderer_amd
import test_gpu_clusters as TC
import test_gpu_cluster_phases as TP
renderer_amd.load_library()
if sys.argv[3] == "hand":
    TP.run_hand_cases(renderer_amd, asyncs=(True,))
elif sys.argv[3] == "config 3":
    for n in (0, 1, 63, 64, 65, 257, 4097):
        TP.run_config_3(renderer_amd, n)
else:
    TP.run_edge_scenes(renderer_amd, TC._plan_sizes(sys.argv[2]))
print("CLUSTER-PHASES-OK")
'''


@pytest.mark.parametrize("which", ["hand", "config 3", "W edges"])
@pytest.mark.parametrize("tiles", ["reverse", "scramble"])
def test_in_any_dispatch_order(tiles, which, tmp_path):
    e = dict(os.environ, MIP_DEBUG_TILE_ORDER=tiles)
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(tmp_path), which], capture_output=True, text=True, timeout=600, env=e)
    assert out.returncode == 0 and "CLUSTER-PHASES-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ---- 4. the occlusion test's decision edges ----

@pytest.mark.parametrize("name", oc.NAMES)
def test_decision_edges(ra, name):
    """FIRST under an all-0.0 image: everything the test can occlude becomes a candidate. SECOND under the case's own image:
    the case's written survivors among the candidates. Expectations from the instance-level decision (a cluster's box is its
    mesh's box), never from a cluster restatement."""
    import torch

    c, s, vertices, indices, boxes = ce.occlusion_scene(name)
    w, h = c["width"], c["height"]
    zeros = np.zeros((h, w), np.float32)
    candidate = orr.occluded(c["boxes"], c["pv"], orr.pyramid_levels(zeros), w, h)
    hidden = orr.occluded(c["boxes"], c["pv"], orr.pyramid_levels(c["depth"]), w, h)
    lod, every = np.zeros(s["n"], np.int64), np.ones(s["n"], bool)
    want = dict(first=ce.transfer_commands(s["meshes"], s["mesh_id"], lod, ~candidate, every, ce.OCCLUSION_BASE),
                second=ce.transfer_commands(s["meshes"], s["mesh_id"], lod, candidate & ~hidden, every, ce.OCCLUSION_BASE), new_depth=c["depth"])
    clusters = ce.level_sizes(s["meshes"], s["mesh_id"], lod)[1]
    want["record"] = pr.pack_record(int(clusters.sum()), int((clusters > 0).sum()), np.repeat(candidate, clusters))
    assert candidate.any() and (candidate & ~hidden).any()
    scene = dict(s, bitmap=ce.bits_to_bitmap(every), base=ce.OCCLUSION_BASE, pv=c["pv"], old_depth=zeros)
    with TE_context(ra, s, vertices, indices, boxes) as p:
        run_scene(ra, p, scene, want, f"decision edges {name}")
    torch.cuda.synchronize()


def TE_context(ra, s, vertices, indices, boxes):
    p = ra.InstancePipeline(max_instances=s["n"], max_meshes=len(s["meshes"]))
    p.set_mesh_table(s["meshes"])
    p.set_geometry(vertices, indices)
    p.build_clusters()
    assert np.array_equal(p.read_cluster_boxes(), boxes), "built boxes"
    p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
    return p


# ---- 5. contracts ----

def _contract_scene(ra):
    s = ra.scene.make_scene(3, n=257)
    vertices, indices = ra.scene.make_geometry(s["meshes"], "strips")
    boxes = cr.cluster_boxes(s["meshes"], vertices, indices)
    bitmap = orr.bitmap_of(~nr.run(s)["coarse_culled"])
    pv = ra.scene.default_pv()
    occ_of = lambda depth: dict(pv=pv, levels=orr.pyramid_levels(depth), width=64, height=32)
    return s, vertices, indices, boxes, bitmap, pv, occ_of


@pytest.mark.parametrize("frames_in_flight", [1, 2])
def test_overflows_and_a_record_that_is_not_the_calls(ra, frames_in_flight):
    import torch
    import test_cluster_phase_restatement as CPU

    s, vertices, indices, boxes, bitmap, pv, occ_of = _contract_scene(ra)
    args = (s, boxes, bitmap, lr.DISTANCE, lr.PIN_SWITCH_SQ)
    f = pr.first(*args, 1 << 30, occ_of(_wall(0)), first_instance_base=17)
    g = pr.second(*args, 1 << 30, occ_of(_wall(None)), f["record"], first_instance_base=17)
    w, members, heads2 = int(f["stats"][2]), int(f["stats"][3]), int(g["stats"][0])
    assert heads2 > 2
    fewer = orr.bits_of(bitmap, 257).copy()
    fewer[int(f["items"]["inst"][0])] = False
    other_w = orr.bitmap_of(fewer)
    other_members = CPU.same_w_other_members(s, boxes, bitmap)
    policy = make_lod_policy(lr.DISTANCE, lr.PIN_SWITCH_SQ)
    frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=17)
    with TC._pipeline(ra, s, vertices, indices, frames_in_flight=frames_in_flight) as p:
        old, clear = _Pyramid(ra, _wall(0), pv), _Pyramid(ra, _wall(None), pv)
        bm, bm_w, bm_m = TC._device_bitmap(bitmap), TC._device_bitmap(other_w), TC._device_bitmap(other_members)
        fr = T._Frame(257)
        torch.cuda.synchronize()
        occ_old, occ_new = old.build(ra, p), clear.build(ra, p)
        p.wait()

        def turn():
            if frames_in_flight > 1:       # behind a frame of its own: consecutive calls go to different slots
                p.run_device(frame, async_=True, **fr.kwargs())

        for async_ in BOTH:
            # FIRST: a record one word short is a work overflow — the refusal's header and nothing behind it; exact room runs
            rec = _Record(w)
            turn()
            _phase(p, frame, bm.data_ptr(), policy, occ_old, rec.arg("first", rec.bytes - 8), dict(cmds=f["cmds"], stats=[0, 0, w, members]),
                   f"a record one word short async={async_}", cmd_capacity=len(f["cmds"]), async_=async_, expect=CAPACITY, count=0)
            rec.check([0xFFFFFFFF, 0, 0, 0], "a record one word short")
            turn()
            _phase(p, frame, bm.data_ptr(), policy, occ_old, rec.arg("first"), f, f"a record of exactly W async={async_}", async_=async_)
            rec.check(f["record"], "a record of exactly W")
            # FIRST: a command overflow leaves the record complete
            rec2 = _Record(w)
            turn()
            _phase(p, frame, bm.data_ptr(), policy, occ_old, rec2.arg("first"), dict(cmds=f["cmds"], stats=f["stats"]), f"FIRST cut async={async_}",
                   cmd_capacity=len(f["cmds"]) - 1, async_=async_, expect=CAPACITY, count=len(f["cmds"]) - 1)
            rec2.check(f["record"], "the record of a FIRST call whose commands overflowed")
            # SECOND: the command overflow
            for cap in (heads2 - 1, 0):
                turn()
                _phase(p, frame, bm.data_ptr(), policy, occ_new, rec.arg("second"), dict(cmds=g["all_cmds"], stats=g["stats"]),
                       f"SECOND cmd_capacity {cap} async={async_}", cmd_capacity=cap, async_=async_, expect=CAPACITY, count=cap)
            # SECOND with another bitmap: another W; the same W and another member count
            for what, other, bits in (("another W", bm_w, other_w), ("another member count", bm_m, other_members)):
                items = cr.work_items(s["pos"], s["scale"], s["mesh_id"], s["meshes"], s["cam_pos"], bits, lr.DISTANCE, lr.PIN_SWITCH_SQ)
                assert (items["W"] != w) == (what == "another W") and items["members"] != members
                turn()
                _phase(p, frame, other.data_ptr(), policy, occ_new, rec.arg("second"), dict(cmds=g["all_cmds"], stats=[0, 0, items["W"], items["members"]]),
                       f"SECOND, {what} async={async_}", cmd_capacity=heads2, async_=async_, expect=DEVICE, count=0)
            # then a fitting call: complete, and the record is as FIRST left it
            turn()
            _phase(p, frame, bm.data_ptr(), policy, occ_new, rec.arg("second"), g, f"a fitting SECOND call async={async_}", async_=async_)
            rec.check(f["record"], "the record behind every SECOND call")
        # mip_cull_clusters after a FIRST call on the same slot returns its usual bytes
        plain = cr.cull_clusters(*args, 1 << 30, first_instance_base=17, occlusion=occ_of(_wall(0)))
        out = TC._Out(len(plain["cmds"]) + 3)
        p.cull_clusters(frame, bm.data_ptr(), policy, out.outputs(), occlusion=occ_old)
        TC._check(out, plain["cmds"], plain["stats"], "mip_cull_clusters behind a FIRST call")
        assert plain["cmds"].tobytes() == f["cmds"].tobytes()


def test_refusals_write_nothing(ra):
    import torch

    name, s, want = _CASES[0]
    with TC._pipeline(ra, s, s["vertices"], s["indices"]) as p:
        lib, ctx = p._lib, p._ctx
        bm = TC._device_bitmap(s["bitmap"])
        out, rec = TC._Out(4), _Record(3)
        frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=s["base"])
        policy = make_lod_policy(lr.DISTANCE, pc.PIN)
        pyr = torch.zeros(64, dtype=torch.float32, device=T._dev())
        torch.cuda.synchronize()
        good_occ = make_occlusion(8, 8, pyr.data_ptr(), s["pv"])

        def call(frame=frame, bitmap=bm.data_ptr(), policy=policy, occ=good_occ, o=None, r=None, null_out=False, null_rec=False):
            o = o if o is not None else out.outputs()
            r = r if r is not None else rec.arg("first")
            return lib.mip_cull_clusters_phase(ctx, C.addressof(frame) if frame is not None else None, bitmap, C.addressof(policy) if policy is not None else None,
                                               C.addressof(occ) if occ is not None else None, None if null_out else C.addressof(o),
                                               None if null_rec else C.addressof(r))

        def changed(make, **kw):
            x = make()
            for k, v in kw.items():
                setattr(x, k, v)
            return x

        outputs = lambda **kw: changed(out.outputs, **kw)
        record = lambda **kw: changed(lambda: rec.arg("first"), **kw)
        occlusion = lambda **kw: changed(lambda: make_occlusion(8, 8, pyr.data_ptr(), s["pv"]), **kw)
        bad_policy = make_lod_policy(lr.DISTANCE, pc.PIN)
        bad_policy.switch_sq[1] = 1.0           # decreases
        refused = [
            # everything mip_cull_clusters refuses
            ("NULL frame", call(frame=None)), ("NULL bitmap", call(bitmap=None)), ("NULL policy", call(policy=None)), ("NULL out", call(null_out=True)),
            ("NULL cluster_cmds", call(o=outputs(cluster_cmds=None))), ("NULL cmd_count", call(o=outputs(cmd_count=None))),
            ("struct_size", call(o=outputs(struct_size=36))), ("unknown flags", call(o=outputs(flags=_lib.MIP_OUT_DEVICE | 0x10))),
            ("host outputs", call(o=outputs(flags=0))), ("misaligned", call(o=outputs(cmd_count=out.scal.data_ptr() + 2))),
            ("decreasing thresholds", call(policy=bad_policy)),
            ("occlusion struct_size", call(occ=occlusion(struct_size=100))), ("occlusion flags", call(occ=occlusion(flags=1))),
            ("candidates", call(occ=occlusion(candidates=bm.data_ptr()))), ("occluded_bitmap", call(occ=occlusion(occluded_bitmap=bm.data_ptr()))),
            ("NULL pyramid", call(occ=occlusion(pyramid=None))), ("extent", call(occ=occlusion(width=0))),
            # and the record's own
            ("NULL rec", call(null_rec=True)), ("NULL record", call(r=record(record=None))), ("misaligned record", call(r=record(record=rec.buf.data_ptr() + 8))),
            ("record_bytes 15", call(r=record(record_bytes=15))), ("record_bytes 0", call(r=record(record_bytes=0))),
            ("phase 0", call(r=record(phase=0))), ("phase 3", call(r=record(phase=3))), ("record struct_size", call(r=record(struct_size=16))),
            ("NULL occ", call(occ=None)), ("NULL occ, SECOND", call(occ=None, r=record(phase=2))),
        ]
        for what, rc in refused:
            assert rc == INVALID, (what, rc)
        assert lib.mip_cull_clusters_phase(None, C.addressof(frame), bm.data_ptr(), C.addressof(policy), C.addressof(good_occ), None, None) == INVALID
        assert out.untouched() and (rec.words() == SENTINEL).all()
        run_scene(ra, p, s, want, name + " after the refusals")       # the context is usable


# ---- 6. two frames in flight ----

def test_two_frames_in_flight_without_a_host_wait(ra):
    """FIRST, mip_build_depth_pyramid, mip_run_occluded (the slot advances), SECOND — the SECOND call runs on another stream
    than the FIRST call that writes its record, and nothing waits on the host in between."""
    import torch

    s, vertices, indices, boxes, bitmap, pv, occ_of = _contract_scene(ra)
    args = (s, boxes, bitmap, lr.DISTANCE, lr.PIN_SWITCH_SQ, 1 << 30)
    f = pr.first(*args, occ_of(_wall(0)), first_instance_base=5)
    g = pr.second(*args, occ_of(_wall(16)), f["record"], first_instance_base=5)
    policy = make_lod_policy(lr.DISTANCE, lr.PIN_SWITCH_SQ)
    frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=5)
    with TC._pipeline(ra, s, vertices, indices, frames_in_flight=2) as p:
        old, moved = _Pyramid(ra, _wall(0), pv), _Pyramid(ra, _wall(16), pv)
        bm = TC._device_bitmap(bitmap)
        fr, outs = T._Frame(257), TO._Outs(ra, 257)
        outs.out.flags |= _lib.MIP_OUT_ASYNC
        torch.cuda.synchronize()
        occ_old = old.build(ra, p)
        p.wait()
        for round_ in range(3):
            rec = _Record(int(f["stats"][2]))
            o1, o2 = TC._Out(len(f["cmds"]) + 3), TC._Out(len(g["cmds"]) + 3)
            p.run_device(frame, async_=True, **fr.kwargs())
            p.cull_clusters_phase(frame, bm.data_ptr(), policy, o1.outputs(async_=True), occ_old, rec.arg("first"))
            occ_new = moved.build(ra, p)
            p.run_occluded(frame, occ_new, outs.out)
            p.cull_clusters_phase(frame, bm.data_ptr(), policy, o2.outputs(async_=True), occ_new, rec.arg("second"))
            p.wait()
            TC._check(o1, f["cmds"], f["stats"], f"FIRST, round {round_}")
            TC._check(o2, g["cmds"], g["stats"], f"SECOND on the other slot, round {round_}")
            rec.check(f["record"], f"round {round_}")
        assert int(g["stats"][1]) > 0
