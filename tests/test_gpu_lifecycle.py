"""ONE context through table swaps, updates and re-uploads (tests/lifecycle_cases.py), with the resident-state model
(tests/context_model.py) beside it: every step's return code is the model's, and after every step the consumers of the resident
state — mip_run in both orders, the packed wire form, recorded launches prepared once for the whole sequence, mip_run_views, a
TLAS frame, mip_light_draw_lists, mip_batch_draws_lods with batch_model, mip_run_occluded on an open pyramid, and in the
sequences with geometry mip_cull_clusters / mip_cull_clusters_cone — write what the oracle and the restatements give for
model.scene(), or are refused and write nothing. general_launches follows the model's census state frame by frame. The
expectation never comes from a GPU. Buffers are larger than the frame and hold a sentinel.

The transitions, the mutant table and the wall time of this file on its own: DESIGN.md §15.3b."""
import numpy as np
import pytest

import cluster_cone_restatement as ccr
import cluster_restatement as cr
import context_model as cm
import decision_cases as dc
import lifecycle_cases as lc
import lod_restatement as lr
import occlusion_restatement as occ
from helpers import float_mismatches, run_oracle

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A5A5A5A
SLACK = 16
CAP = lc.MAX_INSTANCES
BASE, INDEX_BASE = 123, 0xFFFFFF00            # firstIndex wraps inside the list
VIEW_BASES = ((7, 0), (1007, 0xFFFFFF01))
LIGHTS = np.array([[3.0, 4.0, 30.0], [-20.0, 1.0, 60.0]], np.float32)
DEPTH = np.ones((37, 53), np.float32)         # a cleared depth image: nothing is occluded
FRAME_PROBES = ("run", "wire_packed", "run_many", "run_views", "tlas", "light_draw_lists", "batch_draws_lods", "run_occluded")
CLUSTER_PROBES = ("cull_clusters", "cull_clusters_cone")
COUNTS_GENERAL = ("run", "wire_packed", "run_views", "tlas", "run_occluded")     # one launch each, counted by general_launches
assert set(FRAME_PROBES + CLUSTER_PROBES) == set(lc.PROBES)


@pytest.fixture(scope="module")
def ra():
    import renderer_amd

    renderer_amd.load_library()
    return renderer_amd


@pytest.fixture(params=("1", "3"))
def order(request, monkeypatch):
    """Both orders of the frame kernel (MIP_TUNE_ORDER is read when the context is created)."""
    monkeypatch.setenv("MIP_TUNE_ORDER", request.param)
    return request.param


def _dev():
    import torch

    return torch.device("cuda", 0)


def _full(*dims):
    import torch

    return torch.full(dims, SENTINEL, dtype=torch.int32, device=_dev())


def _words(t):
    return t.cpu().numpy().view(np.uint32)


def _second_view(oracle_mod):
    c = dc.VIEW_CAMERAS[0]
    q = np.asarray(c["q"], np.float64)
    cam = np.asarray(c["cam_pos"], np.float32)
    planes = oracle_mod.project_camera(cam, (q / np.linalg.norm(q)).astype(np.float32), aspect=c["aspect"], fovy_degrees=c["fovy_degrees"],
                                       near=c["near"], far=c["far"])
    return planes, cam


def oracle_frame(oracle_mod, s, base=BASE, index_base=INDEX_BASE):
    """The oracle's frame of a scene; of no instances, the empty frame."""
    if s["n"] == 0:
        from renderer_amd.pipeline import DRAW_CMD_DTYPE

        return dict(model=np.zeros((0, 16), np.float32), world_aabb=np.zeros((0, 6), np.float32), visible_bitmap=np.zeros(0, np.uint32),
                    draw_cmds=np.zeros(0, DRAW_CMD_DTYPE), draw_count=0, draw_index_total=0)
    return run_oracle(oracle_mod, s, first_instance_base=base, first_index_base=index_base)


class _Frame:
    """Device outputs of one frame, SLACK sentinel rows behind the largest frame of the context."""

    def __init__(self, tlas=True):
        self.model, self.aabb, self.cmds = _full(CAP + SLACK, 16), _full(CAP + SLACK, 6), _full(CAP + SLACK, 5)
        self.bitmap, self.scal = _full((CAP + 31) // 32 + SLACK), _full(8)
        self.tlas = _full(CAP + SLACK, 16) if tlas else None

    def tensors(self):
        return [t for t in (self.model, self.aabb, self.cmds, self.bitmap, self.scal, self.tlas) if t is not None]

    def refill(self):
        import torch

        for t in self.tensors():
            t.fill_(SENTINEL)
        torch.cuda.synchronize()

    def pointers(self, tlas=False):
        d = dict(model=self.model.data_ptr(), visible_bitmap=self.bitmap.data_ptr(), draw_cmds=self.cmds.data_ptr(), draw_count=self.scal.data_ptr(),
                 draw_index_total=self.scal.data_ptr() + 4, world_aabb=self.aabb.data_ptr())
        if tlas:
            d["tlas_instances"] = self.tlas.data_ptr()
        return d

    def untouched(self):
        import torch

        torch.cuda.synchronize()
        return all(bool((t == SENTINEL).all().item()) for t in self.tensors())

    def check(self, oracle_mod, s, want, what, tlas=None, streams=True, base=BASE):
        """Everything helpers.assert_parity compares, the sentinels behind it, and (tlas: the per-mesh addresses) the TLAS rows."""
        import torch

        torch.cuda.synchronize()
        n, words = s["n"], (s["n"] + 31) // 32
        scal = _words(self.scal)
        assert (int(scal[0]), int(scal[1])) == (want["draw_count"], want["draw_index_total"]), (what, "count / index total", scal[:2].tolist(), want["draw_count"], want["draw_index_total"])
        assert (scal[2:] == SENTINEL).all(), what
        count = want["draw_count"]
        cmds = _words(self.cmds)
        assert cmds[:count].tobytes() == want["draw_cmds"].tobytes(), (what, "command bytes")
        assert (cmds[count:] == SENTINEL).all(), (what, "a command row behind draw_count was written")
        bitmap = _words(self.bitmap)
        assert np.array_equal(bitmap[:words], want["visible_bitmap"]), (what, "visibility bitmap")
        assert (bitmap[words:] == SENTINEL).all(), (what, "a bitmap word behind the last instance was written")
        for name, t, key in (("model", self.model, "model"), ("world_aabb", self.aabb, "world_aabb")):
            rows = _words(t)
            if streams:
                mm = float_mismatches(rows[:n].view(np.float32), want[key])
                assert len(mm) == 0, (what, f"{len(mm)} {name} entries differ, first {mm[:4].tolist()}")
            assert (rows[n if streams else 0:] == SENTINEL).all(), (what, f"a {name} row behind instance {n} was written")
        if self.tlas is not None:
            rows = _words(self.tlas)
            if tlas is not None:
                expect = oracle_mod.tlas_instances(want["model"], s["mesh_id"], tlas, first_instance_base=base) if n else np.zeros((0, 16), np.uint32)
                assert np.array_equal(rows[:n, 14:], expect[:, 14:]), (what, "accelerationStructureReference", rows[:n, 14:][:4].tolist(), expect[:4, 14:].tolist())
                assert np.array_equal(rows[:n, 12:14], expect[:, 12:14]), (what, "TLAS index / mask / flags words")
                assert len(float_mismatches(rows[:n, :12].view(np.float32), expect[:, :12].view(np.float32))) == 0, (what, "TLAS matrices")
            assert (rows[n if tlas is not None else 0:] == SENTINEL).all(), (what, "a TLAS row that is not the frame's was written")


class _Driver:
    """One InstancePipeline and one model, step by step."""

    def __init__(self, ra, oracle_mod, what, max_meshes=lc.MAX_MESHES, frames_in_flight=1, wire=True, clusters=False):
        from renderer_amd.pipeline import make_frame, wire_body_bytes

        self.ra, self.oracle, self.what, self.wire, self.clusters = ra, oracle_mod, what, wire, clusters
        self.model = lc.new_model(max_meshes=max_meshes)
        self.p = ra.InstancePipeline(max_instances=lc.MAX_INSTANCES, max_meshes=max_meshes, frames_in_flight=frames_in_flight)
        self.pv = ra.scene.default_pv()
        self.frame = make_frame(self.model.planes, self.model.cam_pos, first_instance_base=BASE, first_index_base=INDEX_BASE, pv=self.pv)
        self.view_inputs = [(self.model.planes, self.model.cam_pos), _second_view(oracle_mod)]
        self.view_frames = [make_frame(pl, cam, first_instance_base=b, first_index_base=ib) for (pl, cam), (b, ib) in zip(self.view_inputs, VIEW_BASES)]
        self.outs, self.flight = _Frame(), _Frame()
        self.body = _full(wire_body_bytes(CAP, packed=True) // 4 + SLACK)
        self.lights = _full(1 + len(LIGHTS) * CAP + SLACK, 5)
        self.views = [_Frame(tlas=False) for _ in VIEW_BASES]
        # recorded launches: the outputs are prepared ONCE, so a recording lives across the steps until the library drops it
        self.many = [_Frame(tlas=False) for _ in range(frames_in_flight)]      # one per frame slot: frames of two slots overlap
        self.many_outs = [self.p.prepare_outputs(**o.pointers()) for o in self.many]
        self.pyramid = None
        self.levels = occ.pyramid_levels(DEPTH)
        self.step = 0
        self.want = None
        self.log = []

    def close(self):
        self.p.close()

    # ---- the expectation ----

    def scene(self):
        return self.model.scene()

    def frame_want(self):
        if self.want is None:
            self.want = oracle_frame(self.oracle, self.scene())
        return self.want

    def where(self, probe):
        return f"{self.what}, step {self.step} {self.log[-1] if self.log else ''}, {probe} (graph_records {self.p.timings()['graph_records']})"

    # ---- a step ----

    def apply(self, op, kw):
        """The call on the library and on the model: the same return code."""
        import torch

        p, keep = self.p, []
        want_rc = self.model.apply(op, **kw)
        self.want = None
        self.step += 1
        self.log.append(f"{op} -> {want_rc}")
        try:
            if op == "set_mesh_table":
                p.set_mesh_table(kw["meshes"])
            elif op == "set_instances":
                p.set_instances(kw["pos"], kw["rot"], kw["scale"], kw["mesh_id"])
            elif op == "set_instances_device":
                keep = [torch.from_numpy(np.ascontiguousarray(kw[c]).view(np.int32).reshape(-1).copy()).to(_dev()) for c in ("pos", "rot", "scale", "mesh_id")]
                torch.cuda.synchronize()
                p.set_instances_device(*[t.data_ptr() for t in keep], len(kw["mesh_id"]))
            elif op == "update_instances":
                p.update_instances(kw["first"], pos_xyz=kw.get("pos"), rot_ijkw=kw.get("rot"), scale=kw.get("scale"), mesh_id=kw.get("mesh_id"))
            elif op == "set_blas_addresses":
                p.set_blas_addresses(kw["addresses"])
            elif op == "set_geometry":
                p.set_geometry(kw["vertices"], kw["indices"])
            elif op == "build_clusters":
                p.build_clusters()
            else:
                assert op == "build_cluster_cones", op
                p.build_cluster_cones()
            got_rc = cm.OK
        except self.ra.MipError as e:
            got_rc = e.code
        assert got_rc == want_rc, (self.where("the call itself"), got_rc, want_rc)
        assert p._lib.mip_instance_count(p._ctx) == self.model.n, self.where("mip_instance_count")

    def refused(self, call, outs, probe):
        """A call the state refuses: MIP_ERR_NOT_READY, and not a byte of its outputs is written."""
        with pytest.raises(self.ra.MipError) as e:
            call()
        assert e.value.code == cm.NOT_READY, (self.where(probe), e.value.code)
        assert outs.untouched(), (self.where(probe), "a refused call wrote to its outputs")

    def census(self, probe, before):
        rose = self.p.timings()["general_launches"] - before
        expect = 1 if self.model.fallback and self.model.n else 0
        assert rose == expect, (self.where(probe), f"general_launches rose by {rose}, the model's census state says {expect}")

    def probe(self, name):
        before = self.p.timings()["general_launches"]
        getattr(self, "probe_" + name)()
        if name in COUNTS_GENERAL and self.model.frame_ready:
            self.census(name, before)

    def probe_all(self):
        for name in FRAME_PROBES + (CLUSTER_PROBES if self.clusters else ()):
            if name == "wire_packed" and not self.wire:
                continue
            self.probe(name)

    # ---- the probes ----

    def _run(self, probe, tlas):
        o = self.outs
        o.refill()
        call = lambda: self.p.run_device(self.frame, **o.pointers(tlas=tlas))
        if not self.model.frame_ready:
            return self.refused(call, o, probe)
        call()
        o.check(self.oracle, self.scene(), self.frame_want(), self.where(probe), tlas=self.model.blas_addresses() if tlas else None)

    def probe_run(self):
        self._run("run", False)

    def probe_tlas(self):
        self._run("tlas", True)

    def probe_wire_packed(self):
        import torch

        from cpu_pipeline import decode_wire, unpack_wire

        o, s = self.outs, self.scene()
        o.refill()
        self.body.fill_(SENTINEL)
        torch.cuda.synchronize()
        call = lambda: self.p.run_device(self.frame, visible_bitmap=o.bitmap.data_ptr(), draw_cmds=self.body.data_ptr(), draw_count=o.scal.data_ptr(),
                                         draw_index_total=o.scal.data_ptr() + 4, wire="packed")
        where = self.where("wire_packed")
        if not self.model.frame_ready:
            self.refused(call, o, "wire_packed")
            assert bool((self.body == SENTINEL).all().item()), (where, "a refused call wrote to the wire body")
            return
        call()
        want = self.frame_want()
        scal, body, count = _words(o.scal), _words(self.body), want["draw_count"]
        assert (int(scal[0]), int(scal[1])) == (count, want["draw_index_total"]), (where, scal[:2].tolist())
        blocks = (count + 63) // 64
        assert (body[blocks * 68:] == SENTINEL).all(), (where, "a word behind the list's last block was written")
        headers = body[: blocks * 68].reshape(blocks, 68)[:, :4]
        assert (headers[:, 2] == self.model.index_bits).all() and (headers[:, 1] == BASE).all(), (where, "block headers", headers[:2].tolist(), self.model.index_bits)
        cmds = decode_wire(unpack_wire(body, count), count, s["meshes"]) if count else want["draw_cmds"][:0]
        assert np.ascontiguousarray(cmds).tobytes() == want["draw_cmds"].tobytes(), (where, "the decoded list")
        assert np.array_equal(_words(o.bitmap)[: (s["n"] + 31) // 32], want["visible_bitmap"]), (where, "visibility bitmap")

    def probe_run_many(self):
        for o in self.many:
            o.refill()
        call = lambda: (self.p.run_many([self.frame], self.many_outs, 64), self.p.wait())
        if not self.model.frame_ready:
            self.refused(call, self.many[0], "run_many")
            assert self.many[-1].untouched()
            return
        call()
        for o in self.many:
            o.check(self.oracle, self.scene(), self.frame_want(), self.where("run_many"))

    def probe_run_views(self):
        import torch

        for v in self.views:
            v.refill()
        prepared = [self.p.prepare_outputs(draw_cmds=v.cmds.data_ptr(), draw_count=v.scal.data_ptr(), draw_index_total=v.scal.data_ptr() + 4,
                                           visible_bitmap=v.bitmap.data_ptr(), async_=False) for v in self.views]
        call = lambda: self.p.run_views(self.view_frames, prepared)
        if not self.model.frame_ready:
            self.refused(call, self.views[0], "run_views")
            assert self.views[1].untouched()
            return
        call()
        torch.cuda.synchronize()
        s = self.scene()
        for k, (v, (planes, cam), (base, index_base)) in enumerate(zip(self.views, self.view_inputs, VIEW_BASES)):
            want = self.frame_want() if (k == 0 and (base, index_base) == (BASE, INDEX_BASE)) else \
                oracle_frame(self.oracle, dict(s, planes=planes, cam_pos=cam), base, index_base)
            v.check(self.oracle, s, want, self.where(f"run_views, view {k}"), streams=False, base=base)

    def probe_light_draw_lists(self):
        import torch

        self.lights.fill_(SENTINEL)
        torch.cuda.synchronize()
        where = self.where("light_draw_lists")
        try:
            self.p.light_draw_lists(LIGHTS, self.lights.data_ptr() + 20, first_instance_base=3)      # rows 4-byte aligned only
            assert self.model.frame_ready, (where, "a call the model refuses succeeded")
        except self.ra.MipError as e:
            assert not self.model.frame_ready and e.code == cm.NOT_READY, (where, e.code)
        s, rows = self.scene(), _words(self.lights)
        k = len(LIGHTS) * s["n"] if self.model.frame_ready else 0
        if k:
            want = self.oracle.light_draw_lists(s["pos"], s["mesh_id"], s["meshes"], LIGHTS, first_instance_base=3)
            assert rows[1 : 1 + k].tobytes() == want.tobytes(), where
        assert (rows[:1] == SENTINEL).all() and (rows[1 + k :] == SENTINEL).all(), (where, "a row that is not the lists' was written")

    def probe_batch_draws_lods(self):
        import torch

        import test_gpu_batch as T
        import test_gpu_batch_lods as TL
        from renderer_amd.pipeline import make_lod_policy

        s, where = self.scene(), self.where("batch_draws_lods")
        n = s["n"]
        meshes = s["meshes"] if len(s["meshes"]) else lc.table(1)
        b = TL._batch(n, meshes)
        if not self.model.frame_ready:
            bitmap = torch.zeros(4, dtype=torch.int32, device=_dev())
            torch.cuda.synchronize()
            with pytest.raises(self.ra.MipError) as e:
                self.p.batch_draws_lods(self.frame, bitmap.data_ptr(), make_lod_policy(lr.DISTANCE, lr.PIN_SWITCH_SQ), **b.kwargs())
            got = b.result()
            assert e.value.code == cm.NOT_READY and all((got[k] == SENTINEL).all() for k in ("cmds", "ids", "scal", "model")), where
            return
        want_frame = self.frame_want()
        sw = TL._metric_thresholds(s, lr.DISTANCE)
        bitmap = torch.from_numpy(np.concatenate([want_frame["visible_bitmap"], np.full(SLACK, SENTINEL, np.uint32)]).view(np.int32)).to(_dev())
        torch.cuda.synchronize()
        self.p.batch_draws_lods(self.frame, bitmap.data_ptr(), make_lod_policy(lr.DISTANCE, sw), **b.kwargs())
        want = lr.batch_draws_lods(s["pos"], s["scale"], s["mesh_id"], s["meshes"], s["cam_pos"], want_frame["visible_bitmap"], lr.DISTANCE, sw,
                                   first_instance_base=BASE, model=want_frame["model"])
        got = b.result()
        T._check(got, want, where)
        if want["members"]:                   # the arithmetic tier batch_model comes from follows the census: the oracle's matrices, as numbers
            mm = float_mismatches(got["model"][: want["members"]].view(np.float32), want["model"])
            assert len(mm) == 0, (where, f"{len(mm)} batch_model entries differ")

    def probe_run_occluded(self):
        import torch

        from test_gpu_occlusion import _Outs as OccOuts, _build_pyramid, _check_against_restatement, _run_occluded

        s, where = self.scene(), self.where("run_occluded")
        n = s["n"]
        if self.pyramid is None:
            self.pyramid, _ = _build_pyramid(self.ra, self.p, DEPTH)
            self.p.wait()
        outs = OccOuts(self.ra, n + SLACK, tlas=False)
        outs.n = n
        filled = (outs.model, outs.bitmap, outs.occ, outs.cmds, outs.scal, outs.aabb)
        for t in filled:
            t.view(torch.int32).fill_(SENTINEL)
        torch.cuda.synchronize()
        call = lambda: _run_occluded(self.ra, self.p, s, self.pyramid, DEPTH.shape[1], DEPTH.shape[0], outs, pv=self.pv, frame=self.frame)
        if not self.model.frame_ready:
            with pytest.raises(self.ra.MipError) as e:
                call()
            torch.cuda.synchronize()
            assert e.value.code == cm.NOT_READY and all(bool((t.view(torch.int32) == SENTINEL).all().item()) for t in filled), where
            return
        call()
        want = self.frame_want()
        if n == 0:
            torch.cuda.synchronize()
            assert _words(outs.scal)[:2].tolist() == [0, 0], where
            return
        got = outs.result()
        expect = occ.expected(want, n, self.pv, self.levels, DEPTH.shape[1], DEPTH.shape[0], first_instance_base=BASE, first_index_base=INDEX_BASE)
        assert not expect["occluded"].any() and expect["draw_count"] == want["draw_count"], where
        _check_against_restatement(got, expect, where)
        for key in ("model", "world_aabb"):
            assert len(float_mismatches(got[key], want[key])) == 0, (where, key)
        words = (n + 31) // 32
        for what, t, first in (("model", outs.model, n), ("world_aabb", outs.aabb, n), ("commands", outs.cmds, want["draw_count"]), ("bitmap", outs.bitmap, words),
                               ("occluded bitmap", outs.occ, words)):
            assert bool((t.view(torch.int32)[first:] == SENTINEL).all().item()), (where, f"{what} behind the frame was written")

    def _cull(self, cone):
        import test_gpu_batch_lods as TL
        import test_gpu_clusters as TC
        from renderer_amd.pipeline import make_cluster_cone, make_lod_policy

        probe = "cull_clusters_cone" if cone else "cull_clusters"
        s, where, m = self.scene(), self.where(probe), self.model
        n = s["n"]
        cap = max(n, 1) * 8
        out = TC._Out(cap)
        eye = np.asarray(m.cam_pos, np.float32)
        view_cone = make_cluster_cone(eye=eye, facing=1.0)
        ready = m.cull_status(cone) == cm.OK
        bits = self.frame_want()["visible_bitmap"] if m.frame_ready else np.zeros(0, np.uint32)
        bm = TC._device_bitmap(bits)
        sw = TL._metric_thresholds(s, lr.DISTANCE) if ready else lr.PIN_SWITCH_SQ
        policy = make_lod_policy(lr.DISTANCE, sw)
        call = (lambda: self.p.cull_clusters_cone(self.frame, bm.data_ptr(), policy, view_cone, out.outputs())) if cone else \
               (lambda: self.p.cull_clusters(self.frame, bm.data_ptr(), policy, out.outputs()))
        if not ready:
            return self.refused(call, out, probe)
        boxes = cr.cluster_boxes(s["meshes"], m.vertices, m.indices)
        if cone:
            cones = ccr.cluster_cones(s["meshes"], m.vertices, m.indices, boxes)
            want = ccr.cull_clusters_cone(s, boxes, cones, eye, 1.0, bits, lr.DISTANCE, sw, cap, first_instance_base=BASE)
        else:
            want = cr.cull_clusters(s, boxes, bits, lr.DISTANCE, sw, cmd_capacity=cap, first_instance_base=BASE)
        assert want["status"] == 0, where
        call()
        TC._check(out, want["cmds"], want["stats"], where)

    def probe_cull_clusters(self):
        self._cull(False)

    def probe_cull_clusters_cone(self):
        self._cull(True)

    # ---- a step behind a frame in flight ----

    def apply_behind_a_frame(self, op, kw):
        """MIP_OUT_ASYNC frame, the mutating call with no wait in between, mip_wait: the frame delivers the OLD state's bytes."""
        if not self.model.frame_ready:
            return self.apply(op, kw)
        s, want, addresses = self.scene(), self.frame_want(), self.model.blas_addresses()
        s = dict(s, **{c: s[c].copy() for c in ("pos", "rot", "scale", "mesh_id")})
        self.flight.refill()
        self.p.run_device(self.frame, async_=True, **self.flight.pointers(tlas=True))
        self.apply(op, kw)
        self.p.wait()
        self.flight.check(self.oracle, s, want, self.where("the frame in flight across the call"), tlas=addresses)


def _run_sequence(ra, oracle_mod, name, what, **kw):
    in_flight = name in lc.IN_FLIGHT
    d = _Driver(ra, oracle_mod, what, frames_in_flight=2 if in_flight else 1, clusters=name in ("clusters", "in_flight"), **kw)
    try:
        for op, args in lc.sequence(name):
            (d.apply_behind_a_frame if in_flight else d.apply)(op, args)
            d.probe_all()
    finally:
        d.close()


@pytest.mark.parametrize("name", list(lc.SEQUENCES))
def test_named_sequence(ra, oracle_mod, order, name):
    """One named sequence on one context, every probe after every step; the packed wire form with the stores-first order."""
    _run_sequence(ra, oracle_mod, name, f"{name}, order {order}", wire=order == "1")


@pytest.mark.parametrize("name", ["shrink_inside", "census_by_update", "count_down_and_up"])
def test_named_sequence_with_ids_in_the_u32_column(ra, oracle_mod, monkeypatch, name):
    """max_meshes = 65 537: no narrow id column, the stores-first order reads the u32 ids the updates and re-uploads write."""
    monkeypatch.setenv("MIP_TUNE_ORDER", "1")
    _run_sequence(ra, oracle_mod, name, f"{name}, max_meshes {lc.WIDE_MAX_MESHES}", max_meshes=lc.WIDE_MAX_MESHES)


@pytest.mark.parametrize("seed", lc.WALK_SEEDS)
def test_random_walk(ra, oracle_mod, monkeypatch, seed):
    """A seeded walk of 40 steps, refusals included; behind every step the one probe the walk drew, and a plain frame."""
    monkeypatch.setenv("MIP_TUNE_ORDER", "1" if seed % 2 == 0 else "3")
    d = _Driver(ra, oracle_mod, f"walk {seed}", clusters=True)
    try:
        for op, args, probe in lc.random_walk(seed):
            d.apply(op, args)
            d.probe(probe)
            if probe != "run":
                d.probe("run")
    finally:
        d.close()
