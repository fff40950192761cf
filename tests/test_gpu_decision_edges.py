"""The decision-edge catalogue (tests/decision_cases.py) through every kernel that culls, picks a LOD or an arithmetic tier:
mip_run (both orders, both census states), mip_run_views (view_culled, its own LOD test), mip_light_draw_lists (a third LOD
test), mip_run_occluded and mip_batch_draws (their own instantiations of instance_tiered / coarse_culled / lod_is_far). The
instance counts are the edges of a wave and a tile (1 ... 513); the edge instances sit on the first and last lanes. The
expectation is always the oracle (for the two extensions: their restatements over the oracle's frame), byte for byte — model
and world_aabb as numbers — and never anything a GPU computed. Outputs are larger than the frame and hold a sentinel.
No wrong kernel is ever run here: that these scenes tell the likely mistakes apart is shown on the CPU, on mutants of the
restatement (tests/test_decision_cases.py)."""
import numpy as np
import pytest

import batch_restatement as br
import decision_cases as dc
import occlusion_restatement as occ
import plan_boundaries as pb
from helpers import float_mismatches, run_oracle

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A5A5A5A
SLACK = 16
N_MAX = max(dc.SIZES)


@pytest.fixture(scope="module")
def ra():
    import renderer_amd

    renderer_amd.load_library()
    return renderer_amd


def _dev():
    import torch

    return torch.device("cuda", 0)


def _full(*dims):
    import torch

    return torch.full(dims, SENTINEL, dtype=torch.int32, device=_dev())


_wants = {}


def _want(oracle_mod, key, s, base=0, index_base=0):
    """The oracle's frame of a catalogue scene, computed once per (scene, bases) and shared by the tests."""
    key = (key, base, index_base)
    if key not in _wants:
        w = run_oracle(oracle_mod, s, first_instance_base=base, first_index_base=index_base)
        for v in w.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _wants[key] = w
    return _wants[key]


def _context(ra, **kw):
    p = ra.InstancePipeline(max_instances=N_MAX, max_meshes=len(dc.MESHES), **kw)
    p.set_mesh_table(dc.MESHES)
    return p


def _upload(p, s):
    p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])


def _frame(s, base=0, index_base=0):
    from renderer_amd.pipeline import make_frame

    return make_frame(s["planes"], s["cam_pos"], first_instance_base=base, first_index_base=index_base)


def _run_scenes():
    for name, frame in dc.RUN_INPUTS:
        for n in dc.SIZES:
            yield (name, frame, n), dc.layout(name, n, frame)[0]


# ---- mip_run ----

@pytest.mark.parametrize("general", [0, 1])
@pytest.mark.parametrize("order", [1, 3])
def test_frame_kernel_on_every_edge(ra, oracle_mod, monkeypatch, order, general):
    """Every case at every size; the tier-edge scenes and their twins: the 63 ordinary lanes of a wave keep their outputs
    whichever tier the odd lane makes the wave take. general = 0 leaves the kernel to the census: the scenes with fall-back
    instances then still run the kernel with the fall-back tiers, and general_launches says so."""
    from test_gpu_boundaries import _Outs

    monkeypatch.setenv("MIP_TUNE_ORDER", str(order))
    monkeypatch.setenv("MIP_TUNE_FORCE_GENERAL", str(general))
    base, index_base = 123_456, 0xFFFFFF00
    outs = _Outs(ra, N_MAX, pb.STREAMS)
    with _context(ra) as p:
        def one(key, s):
            want = _want(oracle_mod, key, s, base, index_base)
            _upload(p, s)
            outs.refill()
            before = p.timings()["general_launches"]
            outs.run(p, _frame(s, base, index_base))
            outs.check(oracle_mod, s, want, s["n"], base, f"{key} order {order} general {general}")
            assert p.timings()["general_launches"] - before == (1 if general or dc.census_fallbacks(s) else 0), key
            return want

        fallbacks = 0
        for key, s in _run_scenes():
            one(key, s)
            fallbacks += dc.census_fallbacks(s) > 0
        assert fallbacks >= len(dc.SIZES)       # (a one-instance layout need not hold a fall-back instance)
        for kind in dc.TIER_KINDS:
            for placement in dc.TIER_PLACEMENTS:
                s, twin, odd = dc.tier_scene(kind, placement)
                n = s["n"]
                lanes = dc.ordinary_lanes(n, odd)
                got = {}
                for which, scene in (("odd", s), ("twin", twin)):
                    want = one((kind, placement, which), scene)
                    words = outs.bitmap[: (n + 31) // 32].cpu().numpy().view(np.uint32)
                    cmds = outs.cmds[: want["draw_count"]].cpu().numpy().view(np.uint32)
                    mine = cmds[np.isin(cmds[:, 4] - np.uint32(base), lanes.astype(np.uint32))]
                    got[which] = dict(model=outs.model[:n].cpu().numpy().view(np.float32)[lanes], aabb=outs.aabb[:n].cpu().numpy().view(np.float32)[lanes],
                                      tlas=outs.tlas[:n].cpu().numpy().view(np.uint32)[lanes][:, 12:], visible=br.bitmap_bits(words, n)[lanes],
                                      cmds=mine[:, [0, 1, 3, 4]])
                what = (kind, placement, order, general)
                for key in ("model", "aabb"):
                    assert len(float_mismatches(got["odd"][key], got["twin"][key])) == 0, (what, key)
                for key in ("tlas", "visible", "cmds"):
                    assert np.array_equal(got["odd"][key], got["twin"][key]), (what, key)


# ---- mip_run_views ----

class _ViewOuts:
    def __init__(self, with_bitmap=True):
        self.cmds, self.scal, self.bitmap = _full(N_MAX + SLACK, 5), _full(8), _full((N_MAX + 31) // 32 + SLACK)
        self.with_bitmap = with_bitmap

    def refill(self):
        for t in (self.cmds, self.scal, self.bitmap):
            t.fill_(SENTINEL)

    def prepared(self, p):
        return p.prepare_outputs(draw_cmds=self.cmds.data_ptr(), draw_count=self.scal.data_ptr(), draw_index_total=self.scal.data_ptr() + 4,
                                 visible_bitmap=self.bitmap.data_ptr() if self.with_bitmap else 0, async_=False)

    def check(self, ra, want, n, what):
        count, total = (int(x) & 0xFFFFFFFF for x in self.scal[:2].cpu().tolist())
        assert (count, total) == (want["draw_count"], want["draw_index_total"]), (what, count, total)
        rows = self.cmds.cpu().numpy().view(np.uint32)
        assert rows[:count].tobytes() == want["draw_cmds"].tobytes(), (what, "command bytes")
        assert (rows[count:] == SENTINEL).all(), (what, "a command row behind draw_count was written")
        assert (self.scal[2:].cpu().numpy().view(np.uint32) == SENTINEL).all(), what
        words = self.bitmap.cpu().numpy().view(np.uint32)
        k = (n + 31) // 32 if self.with_bitmap else 0
        assert np.array_equal(words[:k], want["visible_bitmap"][:k]), (what, "visibility bitmap")
        assert (words[k:] == SENTINEL).all(), (what, "a bitmap word that is not the view's was written")


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("name", dc.VIEW_INPUTS)
def test_views_kernel_on_every_edge(ra, oracle_mod, name, k):
    """k views of one launch (5: two launches), each with its own planes, its own LOD reference point and its own bases; the
    frames rotate with the size, so the views' tie sets, the subnormal planes, the axis planes and the planes with -0, NaN,
    +-inf and 3.4e38 all pass through every view slot. Without a bitmap at two of the sizes."""
    import torch

    c = dc.case(name)
    sets = [_ViewOuts() for _ in range(k)]
    with _context(ra) as p:
        for j, n in enumerate(dc.SIZES):
            s0 = dc.layout(name, n)[0]
            frames = [c["frames"][(j + v) % len(c["frames"])] for v in range(k)]
            _upload(p, s0)
            for with_bitmap in ((True, False) if n in (65, 257) else (True,)):
                fr, prepared, wants = [], [], []
                for v, f in enumerate(frames):
                    s = dc.layout(name, n, f)[0]
                    base, index_base = 1000 * v + 7, (0xFFFFFF00 + v) & 0xFFFFFFFF
                    wants.append(_want(oracle_mod, (name, f, n), s, base, index_base))
                    fr.append(_frame(s, base, index_base))
                    sets[v].with_bitmap = with_bitmap
                    sets[v].refill()
                    prepared.append(sets[v].prepared(p))
                torch.cuda.synchronize()
                for rep in range(2):
                    p.run_views(fr, prepared)
                p.wait()
                torch.cuda.synchronize()
                for v, f in enumerate(frames):
                    sets[v].check(ra, wants[v], n, f"{name} n={n} view {v} of {k} = {f} bitmap={with_bitmap}")
        assert (p.timings()["general_launches"] > 0) == c["fallback"], name   # the census picks the instantiation


# ---- mip_light_draw_lists ----

@pytest.mark.parametrize("n_lights", [1, 2, 16])
def test_light_lists_on_every_lod_edge(ra, oracle_mod, n_lights):
    """Every light has its own ring of instances on the floats around the LOD threshold, one on top of it, one at +inf and one
    at NaN. n = 64 and 256 run the 16-byte-aligned instantiation, the other sizes the unaligned one; then a destination that is
    only 4-byte aligned."""
    import torch

    lights = dc.catalogue()["lights"][:n_lights]
    with _context(ra) as p:
        for n in dc.SIZES:
            s = dc.layout("lights", n)[0]
            want = oracle_mod.light_draw_lists(s["pos"], s["mesh_id"], dc.MESHES, lights, first_instance_base=3)
            _upload(p, s)
            out = _full(1 + n_lights * n + SLACK, 5)
            torch.cuda.synchronize()
            for offset in (0, 20):            # 20 bytes: the rows start 4-byte aligned only
                out.fill_(SENTINEL)
                torch.cuda.synchronize()
                p.light_draw_lists(lights, out.data_ptr() + offset, first_instance_base=3)
                rows = out.cpu().numpy().view(np.uint32)
                first = offset // 20
                assert rows[first : first + n_lights * n].tobytes() == want.tobytes(), (n, n_lights, offset)
                assert (rows[:first] == SENTINEL).all() and (rows[first + n_lights * n :] == SENTINEL).all(), (n, n_lights, offset)
    assert {n % 4 == 0 for n in dc.SIZES} == {True, False}


# ---- mip_run_occluded ----

def test_occluded_frame_kernel_on_every_edge(ra, oracle_mod):
    """A cleared depth pyramid occludes nothing and every instance is a candidate: the frame must be the oracle's, through
    occlusion_restatement.expected — the frustum, LOD and tier decisions of this kernel's own instantiation."""
    import torch

    from test_gpu_occlusion import _Outs as OccOuts, _build_pyramid, _check_against_restatement, _run_occluded

    depth = np.ones((37, 53), np.float32)
    levels = occ.pyramid_levels(depth)
    pv = ra.scene.default_pv()
    with _context(ra) as p:
        pyr, _ = _build_pyramid(ra, p, depth)
        p.wait()
        for key, s in _run_scenes():
            n = s["n"]
            want = _want(oracle_mod, key, s)
            _upload(p, s)
            outs = OccOuts(ra, n + SLACK, tlas=False)
            outs.n = n
            for t in (outs.model, outs.bitmap, outs.occ, outs.cmds, outs.scal, outs.aabb):
                t.view(torch.int32).fill_(SENTINEL)
            torch.cuda.synchronize()
            _run_occluded(ra, p, s, pyr, depth.shape[1], depth.shape[0], outs, pv=pv, frame=_frame(s))
            got = outs.result()
            expect = occ.expected(want, n, pv, levels, depth.shape[1], depth.shape[0])
            assert not expect["occluded"].any() and expect["draw_count"] == want["draw_count"]
            _check_against_restatement(got, expect, key)
            for name_, rows in (("model", got["model"]), ("world_aabb", got["world_aabb"])):
                assert len(float_mismatches(rows, want[name_])) == 0, (key, name_)
            words = (n + 31) // 32
            for name_, t, first in (("model", outs.model, n), ("world_aabb", outs.aabb, n), ("commands", outs.cmds, want["draw_count"]),
                                    ("bitmap", outs.bitmap, words), ("occluded bitmap", outs.occ, words)):
                assert bool((t.view(torch.int32)[first:] == SENTINEL).all().item()), (key, f"{name_} behind the frame was written")


# ---- mip_batch_draws ----

@pytest.mark.parametrize("general", [0, 1])
def test_batched_draws_on_every_edge(ra, oracle_mod, monkeypatch, general):
    """Over the ORACLE's bitmap of the edge frame (uploaded, not produced by a kernel): the bucket of every member — so the
    LOD this kernel picks for it — the ids in slot order, and batch_model against the oracle's matrices, as numbers."""
    import torch

    from test_gpu_batch import _Batch, _check

    monkeypatch.setenv("MIP_TUNE_FORCE_GENERAL", str(general))
    base = 77
    with _context(ra) as p:
        for key, s in _run_scenes():
            n = s["n"]
            want_frame = _want(oracle_mod, key, s)
            _upload(p, s)
            bitmap = torch.from_numpy(np.concatenate([want_frame["visible_bitmap"], np.full(SLACK, SENTINEL, np.uint32)]).view(np.int32)).to(_dev())
            b = _Batch(n, len(dc.MESHES))
            torch.cuda.synchronize()
            p.batch_draws(_frame(s, base), bitmap.data_ptr(), **b.kwargs())
            got = b.result()
            want = br.batch_draws(s["pos"], s["mesh_id"], dc.MESHES, s["cam_pos"], want_frame["visible_bitmap"], first_instance_base=base,
                                  model=want_frame["model"])
            what = (key, general)
            _check(got, want, what)
            rows = got["model"][: want["members"]].view(np.float32)
            assert len(float_mismatches(rows, want["model"])) == 0, (what, "batch_model")
            # the LOD of every member, spelled out: the restatement's pick, and the oracle's command for the same instance
            lod = br.pick_lods(s["pos"], s["mesh_id"], dc.MESHES, s["cam_pos"])
            per_instance = br.expand(dict(cmds=got["cmds"][: want["count"]].reshape(-1).view(br.DRAW_CMD_DTYPE), members=want["members"],
                                          ids=got["ids"][: want["members"]]), base)
            inst = (per_instance["firstInstance"].astype(np.int64) - base) & 0xFFFFFFFF
            assert np.array_equal(per_instance["indexCount"], dc.MESHES["index_len"][s["mesh_id"][inst], lod[inst]]), what
            assert np.array_equal(per_instance["indexCount"], want_frame["draw_cmds"]["indexCount"]), what
            assert np.array_equal(inst, want_frame["draw_cmds"]["firstInstance"]), what
