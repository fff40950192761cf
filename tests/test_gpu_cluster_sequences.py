"""ONE context through every kind of cluster call in every order (tests/cluster_sequence_cases.py): the eleven entry points and
phases share a scratch per frame slot, a several-view scratch, two pairs of status words and the event behind a FIRST call, and
every other cluster test makes a context per scene. Here the preceding calls are the poison: each call step's return code and
EVERY output buffer — commands, entries and the culled index stream, counts, draw arguments and stats, the record with its guard
words, the words in front of an entry base and behind a count — is compared whole against what the numpy restatements give for
that step alone. With two frames in flight an asynchronous frame sits in front of every call step and rotates the slot, so that
both slots' scratches collect different histories; its visible bitmap is compared too. The expectation never comes from a GPU.

What each sequence guards and what is left to the per-call tests: DESIGN.md, "Cluster calls in sequence"."""
import numpy as np
import pytest

import cluster_sequence_cases as sq
import numpy_restatement as nr
import occlusion_restatement as orr
import test_gpu_batch as T
import test_gpu_cluster_list as TLST
import test_gpu_cluster_list_phases as TLP
import test_gpu_cluster_phases as TP
import test_gpu_cluster_triangles as TT
import test_gpu_cluster_views as TV
import test_gpu_cluster_views_list as TVL
import test_gpu_clusters as TC
from renderer_amd.pipeline import make_cluster_cone, make_frame, make_lod_policy

pytestmark = pytest.mark.gpu
ra = T.ra   # the module's library fixture
assert (sq.SENTINEL, sq.GUARD_ROWS, sq.PAD, sq.RECORD_GUARD, sq.BLOCK) == (T.SENTINEL, TLP.GUARD, TV.PAD, TP.GUARD, TLP.BLOCK) and TVL.PAD == TV.PAD
COUNT_FIELD = {"views": "cmd_counts", "list_views": "entry_counts", "list": "entry_count", "list_phase.FIRST": "entry_count", "list_phase.SECOND": "entry_count"}


class _Driver:
    """One InstancePipeline and what the steps of one sequence leave beside it: the resident scene's bitmaps, the two pyramids,
    the records and list buffers of the FIRST steps, the asynchronous steps whose status a wait step collects."""

    def __init__(self, ra, p, name, frames_in_flight):
        import torch

        self.ra, self.p, self.name, self.frames = ra, p, name, frames_in_flight
        self.old, self.new = TP._Pyramid(ra, sq.DEPTH["old"], sq.PV), TP._Pyramid(ra, sq.DEPTH["new"], sq.PV)
        torch.cuda.synchronize()
        self.occ = dict(old=self.old.build(ra, p), new=self.new.build(ra, p))     # built once: no step writes a pyramid
        p.wait()
        self.sc, self.records, self.pending, self.units = None, {}, [], []

    # ---- state steps ----

    def switch(self, name):
        self.p.wait()
        self.sc = sc = sq.scene(name)
        s = sc["s"]
        self.p.set_mesh_table(s["meshes"])
        self.p.set_geometry(sc["vertices"], sc["indices"])
        self.p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
        self.build()
        self.bm = [TC._device_bitmap(b) for b in sc["bitmaps"]]
        self.records = {}
        self.fr = T._Frame(s["n"], model=False)
        self.frame_bitmap = orr.bitmap_of(~nr.run(s)["coarse_culled"]) if s["n"] else None
        self.policy = make_lod_policy(sq.MODE, sc["switch"])
        self.cone = make_cluster_cone(eye=sc["eye"], facing=sc["facing"])

    def build(self):
        self.p.build_clusters()
        self.p.build_cluster_cones()

    def turn(self):
        """With two frames in flight: an asynchronous frame of the resident scene, so that the next call meets the other slot."""
        s = self.sc["s"]
        if self.frames < 2 or s["n"] == 0:
            return False
        import torch

        self.fr.bitmap.zero_()
        torch.cuda.synchronize()
        self.p.run_device(make_frame(s["planes"], s["cam_pos"]), async_=True, **self.fr.kwargs())
        return True

    # ---- a call step ----

    def launch(self, e):
        """The step's buffers, filled with the sentinel, and the call on them: (its code, {name: tensor})."""
        st, sizes, unit, s = e["step"], e["sizes"], e["unit"], self.sc["s"]
        p, async_ = self.p, st["async_"]
        frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=st["fib"], pv=sq.PV)
        bm = self.bm[st["bm"]].data_ptr()
        occ = self.occ["old"] if (st["pyramid"] and unit in sq.TAKES_PYRAMID) or unit in sq.FIRSTS else self.occ["new"] if unit in sq.SECONDS else None
        rec = None
        if unit in sq.FIRSTS:
            rec = TP._Record(e["w"])
            if not e.get("refused"):
                self.records[st["rec"]] = dict(rec=rec)
        elif unit in sq.SECONDS:
            rec = self.records[st["rec"]]["rec"]
        if unit in ("cull", "cull_cone", "phase.FIRST", "phase.SECOND"):
            out = TC._Out(sizes["cap"])
            o, tensors = out.outputs(sizes["arg"], sizes["work"], async_), dict(cmds=out.cmds, scal=out.scal)
            if unit == "cull":
                fn = lambda: p.cull_clusters(frame, bm, self.policy, o, occlusion=occ)   # noqa: E731
            elif unit == "cull_cone":
                fn = lambda: p.cull_clusters_cone(frame, bm, self.policy, self.cone, o, occlusion=occ)   # noqa: E731
            else:
                arg = rec.arg("first" if unit == "phase.FIRST" else "second")
                fn = lambda: p.cull_clusters_phase(frame, bm, self.policy, o, occ, arg)   # noqa: E731
        elif unit in ("tri", "tri_cone"):
            out = TT._Out(sizes["cap"], sizes["room"])
            o, tensors = out.outputs(cmd_capacity=sizes["arg"], work_capacity=sizes["work"], async_=async_), dict(cmds=out.cmds, scal=out.scal, stream=out.stream)
            if unit == "tri":
                fn = lambda: p.cull_cluster_triangles(frame, bm, self.policy, o, occlusion=occ)   # noqa: E731
            else:
                fn = lambda: p.cull_cluster_triangles_cone(frame, bm, self.policy, self.cone, o, occlusion=occ)   # noqa: E731
        elif unit == "list":
            out = TLST._Out(sizes["cap"])
            o, tensors = out.outputs(sizes["arg"], sizes["work"], async_), dict(entries=out.entries, scal=out.scal)
            fn = lambda: p.list_clusters(frame, bm, self.policy, o, occlusion=occ, cone=self.cone if st["cone"] else None)   # noqa: E731
        elif unit in sq.SEVERAL:
            v = e["views"]
            k = 17 if st["refuse"] == "views17" else sizes["n_views"]          # the seventeenth view is the sixteenth again
            pick = [min(i, sizes["n_views"] - 1) for i in range(k)]
            frames = [make_frame(v["planes"][i], v["cams"][i], first_instance_base=v["bases"][i]) for i in pick]
            ptrs = [0 if v["bitmaps"][i] is None else self.bm[v["bitmaps"][i]].data_ptr() for i in pick]
            if unit == "views":
                out = TV._ViewOut(sizes["n_views"], sizes["stride"])
                tensors = dict(cmds=out.cmds, counts=out.counts, stats=out.st)
                o = out.outputs(sizes["arg"], sizes["work"], async_)
                fn = lambda: p.cull_clusters_views(frames, ptrs, self.policy, o)   # noqa: E731
            else:
                out = TVL._Out(sizes["n_views"], sizes["stride"])
                tensors = dict(entries=out.entries, counts=out.counts, args=out.ar, stats=out.st)
                o = out.outputs(sizes["arg"], sizes["work"], async_)
                fn = lambda: p.list_clusters_views(frames, ptrs, self.policy, o)   # noqa: E731
        else:
            call_no, appended = sizes["call"], unit == "list_phase.SECOND" and st["base"] == "count"
            buf = self.records[st["rec"]]["buf"] if appended else TLP._Buf(sizes["cap"], calls=2)
            if unit == "list_phase.FIRST" and not e.get("refused"):
                self.records[st["rec"]]["buf"] = buf
            if not appended and st["base"] != "null":
                buf.set_word(call_no, sizes["b"])
            base = buf.ptr(0, 0) if appended else 0 if st["base"] == "null" else buf.ptr(call_no, 10)
            o = buf.outputs(call_no, entry_capacity=sizes["arg"], entry_base=base, work_capacity=sizes["work"], async_=async_)
            tensors = dict(entries=buf.entries, scal=buf.scal)
            arg = rec.arg("first" if unit == "list_phase.FIRST" else "second")
            fn = lambda: p.list_clusters_phase(frame, bm, self.policy, o, occ, arg)   # noqa: E731
        if rec is not None:
            tensors["record"] = rec.buf
        if st["refuse"] == "misaligned":
            field = COUNT_FIELD.get(unit, "cmd_count")
            setattr(o, field, getattr(o, field) + 2)
        return self.code(fn), tensors

    def code(self, fn):
        try:
            fn()
        except self.ra.MipError as err:
            return err.code
        return 0

    def where(self, k, e):
        return (f"{self.name}[{k}] frames_in_flight={self.frames} scene={e['scene']} unit={e['unit']} behind {self.units[-3:-1]} "
                f"{ {f: e['step'][f] for f in ('async_', 'pyramid', 'work', 'cap', 'fib', 'cone', 'n_views', 'bm', 'rec', 'base', 'refuse')} }")

    def compare(self, k, e, tensors, turned):
        """One device-to-host copy of everything the step could have written, then every buffer whole."""
        import torch

        names = list(tensors)
        flat = [tensors[n].reshape(-1) for n in names] + ([self.fr.bitmap] if turned else [])
        torch.cuda.synchronize()
        host = torch.cat(flat).cpu().numpy().view(np.uint32)
        at = 0
        for n in names:
            want = e["images"][n].reshape(-1)
            got = host[at: at + len(want)]
            assert tensors[n].numel() == len(want), (self.where(k, e), n, "size", tensors[n].numel(), len(want))
            if got.tobytes() != want.tobytes():
                bad = np.nonzero(got != want)[0]
                raise AssertionError((self.where(k, e), n, "first differing word", int(bad[0]), hex(int(got[bad[0]])), hex(int(want[bad[0]])), "words", len(bad)))
            at += len(want)
        if turned:
            got = host[at: at + len(self.frame_bitmap)]
            assert got.tolist() == self.frame_bitmap.tolist(), (self.where(k, e), "the visible bitmap of the frame in front of the step")

    def step(self, k, e):
        self.units.append(e["unit"])
        st = e["step"]
        turned = self.turn()
        code, tensors = self.launch(e)
        if st["defer"]:
            assert code == 0, (self.where(k, e), "an asynchronous call returned", code)
            self.pending.append((k, e, tensors, turned))
            return
        if st["async_"]:
            code = code or self.code(self.p.wait)
        assert code == e["status"], (self.where(k, e), "status", code, e["status"])
        if code and not self.pending:
            self.p.wait()                     # reported once
        self.compare(k, e, tensors, turned)

    def wait(self, k, expect):
        code = self.code(self.p.wait)
        last = self.pending[-1][1] if self.pending else None
        assert code == expect, (f"{self.name}[{k}] frames_in_flight={self.frames}", "mip_wait behind", last and self.where(self.pending[-1][0], last), code, expect)
        for j, e, tensors, turned in self.pending:
            assert e["status"] == expect, (self.where(j, e), "the sequence collects another status than the step owes")
            self.compare(j, e, tensors, turned)
        self.pending = []


def run_sequence(ra, name, frames_in_flight, expectations=None):
    steps = sq.sequence(name)
    ex = sq.expectations(steps, frames_in_flight=frames_in_flight) if expectations is None else expectations
    with ra.InstancePipeline(max_instances=sq.max_instances(), max_meshes=len(sq.scene("M")["s"]["meshes"]), frames_in_flight=frames_in_flight) as p:
        d = _Driver(ra, p, name, frames_in_flight)
        for k, (st, e) in enumerate(zip(steps, ex)):
            if st["op"] == "scene":
                d.switch(st["scene"])
            elif st["op"] == "set_geometry":      # the cluster table goes stale
                p.wait()
                p.set_geometry(d.sc["vertices"], d.sc["indices"])
            elif st["op"] == "build":
                d.build()
            elif st["op"] == "wait":
                d.wait(k, st["expect"])
            else:
                d.step(k, e)
        assert not d.pending
        p.wait()


@pytest.mark.parametrize("frames_in_flight", [1, 2])
@pytest.mark.parametrize("name", list(sq.SEQUENCES))
def test_sequence(ra, name, frames_in_flight):
    run_sequence(ra, name, frames_in_flight)
