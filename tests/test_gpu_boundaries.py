"""Every user of the cross-tile prefix, launched at the instance counts where its launch plan or the prefix structure
changes: group size 16 -> 32 -> 64 tiles, commands-first -> stores-first order (three thresholds, by request shape), the first
launch whose last tile starts from start1 instead of summing every earlier group, exactly full / one-tile last groups, and the
per-triangle stage's thresholds. The sizes are READ from plan_frame (tests/plan_boundaries.py) for this device's CU count;
every pair is asserted to straddle. The expectation is always the oracle: ONE run at the largest size, truncated
(helpers.truncate_frame, proven on the CPU in tests/test_plan_boundaries.py). Buffers are larger than the frame and filled with
a sentinel: nothing behind the last bitmap word, the last command or the last instance's row may be written.
No wrong kernel is ever run here: that the comparisons bite is shown on the CPU (test_plan_boundaries.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import plan_boundaries as pb
from helpers import assert_parity, float_mismatches, truncate_frame

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_MAX = 1_200_000
SENTINEL = 0x5A5A5A5A
SLACK = 64                                   # rows / words behind the frame that must keep the sentinel
BASES = (123_456, 0xFFFFFF00)                # first_instance_base, first_index_base: firstIndex wraps inside the list


@pytest.fixture(scope="module")
def ra():
    import renderer_amd

    renderer_amd.load_library()
    return renderer_amd


@pytest.fixture(scope="module")
def cu():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _dev():
    import torch

    return torch.device("cuda", 0)


# ---- one oracle run per scene variant, kept while consecutive tests use it ----

_cache = {}


def _variant(ra, oracle_mod, name, n_max=N_MAX):
    """name: default | all_visible | nonfinite (default camera, one NaN position early in the scene) | bases (all visible,
    instance and index bases). Returns (scene, oracle frame at n_max, instance base, index base)."""
    key = (name, n_max)
    if key not in _cache:
        _cache.clear()                       # 1.2 M x 150 B per frame: one at a time
        s = ra.scene.make_scene(3, n=n_max, all_visible=name in ("all_visible", "bases"))
        if name == "nonfinite":
            s["pos"][7, 1] = np.nan
        base, index_base = BASES if name == "bases" else (0, 0)
        want = oracle_mod.run(s["pos"], s["rot"], s["scale"], s["mesh_id"], s["meshes"], s["planes"], s["cam_pos"], threads=8,
                              first_instance_base=base, first_index_base=index_base)
        _cache[key] = (s, want, base, index_base)
    return _cache[key]


def _upload(p, s, n):
    p.set_instances(s["pos"][:n], s["rot"][:n], s["scale"][:n], s["mesh_id"][:n])


class _Outs:
    """Device outputs of one frame with SLACK sentinel rows behind them. shape: pb.STREAMS or pb.COMMANDS_ONLY."""

    def __init__(self, ra, capacity, shape, wire=False):
        import torch

        from renderer_amd.pipeline import wire_body_bytes

        def full(*dims):
            return torch.full(dims, SENTINEL, dtype=torch.int32, device=_dev())

        self.ra, self.capacity, self.streams, self.wire = ra, capacity, shape == pb.STREAMS, wire
        self.bitmap = full((capacity + 31) // 32 + SLACK)
        self.cmds = full(wire_body_bytes(capacity, packed=False) // 4 + SLACK) if wire else full(capacity + SLACK, 5)
        self.scal = full(8)
        self.model = full(capacity + SLACK, 16) if self.streams else None
        self.aabb = full(capacity + SLACK, 6) if self.streams else None
        self.tlas = full(capacity + SLACK, 16) if self.streams else None
        torch.cuda.synchronize()

    def pointers(self):
        d = dict(visible_bitmap=self.bitmap.data_ptr(), draw_cmds=self.cmds.data_ptr(), draw_count=self.scal.data_ptr(),
                 draw_index_total=self.scal.data_ptr() + 4)
        if self.streams:
            d.update(model=self.model.data_ptr(), world_aabb=self.aabb.data_ptr())
        return d

    def run(self, p, frame, async_=False):
        kw = self.pointers()
        if self.streams:
            kw["tlas_instances"] = self.tlas.data_ptr()
        p.run_device(frame, async_=async_, wire=self.wire, **kw)

    def refill(self):
        import torch

        for t in (self.bitmap, self.cmds, self.scal, self.model, self.aabb, self.tlas):
            if t is not None:
                t.fill_(SENTINEL)
        torch.cuda.synchronize()

    def check(self, oracle_mod, s, want, n, base, what):
        """`want`: the oracle's frame of the first n instances. Everything test_ragged_sizes compares, plus the sentinels."""
        import torch

        from cpu_pipeline import decode_wire, unpack_wire

        torch.cuda.synchronize()
        words = (n + 31) // 32
        count, total = (int(x) & 0xFFFFFFFF for x in self.scal[:2].cpu().tolist())
        assert count == want["draw_count"], f"{what}: draw_count {count} vs {want['draw_count']}"
        assert count <= self.capacity

        def untouched(t, first):             # compared on the device: only the frame's own rows are copied back
            return bool((t[first:] == SENTINEL).all().item())

        if self.wire:
            body = self.cmds.cpu().numpy().view(np.uint32)
            flat = decode_wire(unpack_wire(body, count), count, s["meshes"]) if self.wire == "packed" else decode_wire(body, count, s["meshes"])
            cmds = np.ascontiguousarray(flat).view(self.ra.DRAW_CMD_DTYPE).reshape(-1)
        else:
            cmds = self.cmds[:count].cpu().numpy().view(np.uint32).reshape(-1).view(self.ra.DRAW_CMD_DTYPE)
            assert untouched(self.cmds, count), f"{what}: a command row behind draw_count was written"
        assert untouched(self.bitmap, words), f"{what}: a bitmap word behind the last instance was written"
        got = dict(visible_bitmap=self.bitmap[:words].cpu().numpy().view(np.uint32), draw_cmds=cmds, draw_count=count, draw_index_total=total)
        if self.streams:
            for name, t in (("model", self.model), ("world_aabb", self.aabb), ("tlas", self.tlas)):
                assert untouched(t, n), f"{what}: a {name} row behind instance {n} was written"
                rows = t[:n].cpu().numpy().view(np.uint32)
                got[name] = rows.view(np.float32) if name != "tlas" else rows
        assert_parity(got, want, what)
        if self.streams:
            rows = oracle_mod.tlas_instances(want["model"], s["mesh_id"][:n], None, first_instance_base=base)
            assert np.array_equal(got["tlas"][:, 12:], rows[:, 12:]), f"{what}: TLAS index / mask / address words"
            mm = float_mismatches(got["tlas"][:, :12].view(np.float32), rows[:, :12].view(np.float32))
            assert len(mm) == 0, f"{what}: {len(mm)} TLAS matrix entries differ"


def _frame(s, base, index_base):
    from renderer_amd.pipeline import make_frame

    return make_frame(s["planes"], s["cam_pos"], first_instance_base=base, first_index_base=index_base)


def _one_size(ra, oracle_mod, variant, shape, n, what, wire=False, expect_order=None, cu=None):
    """A fresh context with max_instances = n, three launches (both parities of the accumulators), checked each time."""
    s, big, base, index_base = _variant(ra, oracle_mod, variant)
    want = truncate_frame(big, n, base)
    outs = _Outs(ra, n, shape, wire=wire)
    with ra.InstancePipeline(max_instances=n, max_meshes=len(s["meshes"])) as p:
        p.set_mesh_table(s["meshes"])
        _upload(p, s, n)
        for rep in range(3):
            if rep:
                outs.refill()
            outs.run(p, _frame(s, base, index_base))
            outs.check(oracle_mod, s, want, n, base, f"{what} n={n} launch {rep}")
        assert p.timings()["general_launches"] == (3 if variant == "nonfinite" else 0), what
    if variant in ("all_visible", "bases"):
        assert want["draw_count"] == n      # every tile publishes a full count


# ---- a. the frame kernel at every boundary size ----

_SHAPES = {"streams": (pb.STREAMS, "default", {}), "streams_all_visible": (pb.STREAMS, "bases", {}),
           "commands_only": (pb.COMMANDS_ONLY, "default", {}), "commands_only_all_visible": (pb.COMMANDS_ONLY, "all_visible", {}),
           "nonfinite": (pb.STREAMS, "nonfinite", {"nonfinite": 1})}


# Measured (profiles/gpu_suite_plan_boundaries.txt): with the sizes one tile SHORT of every full-group / window tile count in it too,
# the module added 59 s to a 107 s suite — more than a third — so the sweep keeps, per boundary tile count T, {one instance in the
# last tile, full} at T and at T + 1. The other tests of the module are not thinned.
_THIN_SWEEP = True


def _sweep_cases():
    # collected without a GPU: the ids use the 256 CUs of an MI355X; the test recomputes the list for the device and runs
    # the size only if the device's list has it too (the order thresholds scale with the CU count)
    cases = []
    for name, (shape, variant, state) in _SHAPES.items():
        for n in pb.boundary_sizes(shape, 256, hi=N_MAX, thin=_THIN_SWEEP, **state):
            cases.append(pytest.param(name, n, id=f"{name}-{n}"))
    return cases


_device_sizes = {}


def _sizes_here(name, cu):
    if (name, cu) not in _device_sizes:
        shape, _, state = _SHAPES[name]
        _device_sizes[(name, cu)] = pb.boundary_sizes(shape, cu, hi=N_MAX, thin=_THIN_SWEEP, **state)
    return _device_sizes[(name, cu)]


@pytest.mark.parametrize("name,n", _sweep_cases())
def test_frame_kernel_at_plan_boundaries(ra, oracle_mod, cu, name, n):
    shape, variant, state = _SHAPES[name]
    sizes = _sizes_here(name, cu)
    if n not in sizes:
        pytest.skip(f"{n} is a boundary size at 256 CUs, not at the {cu} of this device")
    why = sizes[n]
    if "changes at" in why:                  # a plan change: the pair around it really straddles on this device
        at = int(why.rsplit(" ", 1)[1])
        pb.assert_straddles(at - 1, at, shape, cu, **state)
    _one_size(ra, oracle_mod, variant, shape, n, f"{name} ({why})", cu=cu)


# ---- b. both orders on both sides of the order thresholds ----

def _order_sizes():
    out = []
    for name, at in (("nonfinite", 327_681), ("streams", 524_289), ("commands_only", 1_114_113)):
        for n in (at - 256, at - 1, at, at + 255):
            out.append(pytest.param(name, at, n, id=f"{name}-{n}"))
    return out


@pytest.mark.parametrize("order", [1, 3])
@pytest.mark.parametrize("name,at,n", _order_sizes())
def test_both_orders_on_both_sides_of_the_order_thresholds(ra, oracle_mod, cu, monkeypatch, name, at, n, order):
    shape, variant, state = _SHAPES[name]
    try:
        pb.assert_straddles(at - 1, at, shape, cu, fields=("order",), **state)
    except AssertionError as e:
        if cu == 256:
            raise
        pytest.skip(f"the order threshold scales with the CU count: {e}")
    forced = pb.plan(n, shape, cu, force_order=order, **state)
    assert forced["order"] == order
    monkeypatch.setenv("MIP_TUNE_ORDER", str(order))
    _one_size(ra, oracle_mod, variant, shape, n, f"{name} order {order}")


# ---- c. one context across group sizes ----

def _alternating_sizes(cu):
    """Boundary sizes ordered so that consecutive launches alternate group_shift 6, 4, 5, 6, 5, 4 ..."""
    by_shift = {4: [], 5: [], 6: []}
    for n in pb.boundary_sizes(pb.STREAMS, cu, hi=N_MAX, thin=True):
        by_shift[pb.plan(n, pb.STREAMS, cu, max_instances=N_MAX)["group_shift"]].append(n)
    for v in by_shift.values():
        v.sort(reverse=True)
    assert all(by_shift.values()), by_shift
    order, k = [], 0
    pattern = (6, 4, 5, 6, 5, 4)
    while any(by_shift.values()):
        shift = pattern[k % len(pattern)]
        k += 1
        if by_shift[shift]:
            order.append(by_shift[shift].pop(0))
        elif k > 10_000:
            break
    return order + order[-2::-1]             # largest -> smallest -> largest


@pytest.mark.parametrize("mode", ["synchronous", "two_frames_in_flight", "run_many"])
def test_one_context_across_group_sizes(ra, oracle_mod, cu, monkeypatch, mode):
    """groups_cap comes from max_instances, group_shift from the resident n: accumulators, start1 words and parity buffers
    written under one group size lie underneath the launches of another."""
    import torch

    s, big, base, index_base = _variant(ra, oracle_mod, "bases")
    sizes = _alternating_sizes(cu)
    shifts = [pb.plan(n, pb.STREAMS, cu, max_instances=N_MAX)["group_shift"] for n in sizes]
    assert {4, 5, 6} <= set(shifts) and sum(a != b for a, b in zip(shifts, shifts[1:])) >= len(shifts) // 2, shifts
    slots = 1 if mode == "synchronous" else 2
    monkeypatch.setenv("MIP_TUNE_GRAPH_ROUND", "4")   # (read when the context is created) a round = 4 frames: 2 per frame slot
    sets = [_Outs(ra, N_MAX, pb.COMMANDS_ONLY) for _ in range(slots)]
    frame = _frame(s, base, index_base)
    with ra.InstancePipeline(max_instances=N_MAX, max_meshes=len(s["meshes"]), frames_in_flight=slots) as p:
        p.set_mesh_table(s["meshes"])
        prepared = [p.prepare_outputs(**o.pointers()) for o in sets]
        for n in sizes:
            want = truncate_frame(big, n, base)
            _upload(p, s, n)
            for o in sets:
                o.refill()
            if mode == "synchronous":
                for rep in range(3):
                    sets[0].run(p, frame)
                    sets[0].check(oracle_mod, s, want, n, base, f"one context n={n} launch {rep}")
                    sets[0].refill()
                continue
            if mode == "two_frames_in_flight":
                for rep in range(3):
                    sets[rep % 2].run(p, frame, async_=True)
            else:
                p.run_many(frame, prepared, 6)   # one round from recorded graphs (re-recorded: the instance count changed) + two single launches
            p.wait()
            torch.cuda.synchronize()
            for k, o in enumerate(sets):
                o.check(oracle_mod, s, want, n, base, f"{mode} n={n} slot {k}")
        if mode == "run_many":
            assert p.timings()["graph_frames"] >= 4 * len(sizes) // 2, p.timings()


# ---- d. the other users of the prefix at the group-size and window sizes ----

def _structure_sizes(cu, hi=N_MAX):
    """256 T (the last group exactly full) and 256 T + 1 (one instance in a new group / beyond the window) per structure tile count."""
    tiles = pb.structure_tiles(pb.COMMANDS_ONLY, cu, hi)
    return sorted({n for t in tiles for n in (256 * t, 256 * t + 1)})


def test_views_each_with_its_own_prefix_state(ra, oracle_mod, cu):
    import torch

    from renderer_amd.pipeline import make_frame

    s = ra.scene.make_scene(3, n=N_MAX)
    cams = [np.array(c, np.float32) for c in ((0, 1, 2), (5, 1, 2), (-3, 2, 8), (0, 1, 30))]
    bases = [(0, 0), (1000, 0xFFFFF000), (7, 77), (0, 1 << 31)]
    wants = [oracle_mod.run(s["pos"], s["rot"], s["scale"], s["mesh_id"], s["meshes"], s["planes"], cam, threads=8,
                            first_instance_base=b, first_index_base=ib, want=("draw_cmds", "visible_bitmap")) for cam, (b, ib) in zip(cams, bases)]
    sets = [_Outs(ra, N_MAX, pb.COMMANDS_ONLY) for _ in cams]
    frames = [make_frame(s["planes"], cam, first_instance_base=b, first_index_base=ib) for cam, (b, ib) in zip(cams, bases)]
    with ra.InstancePipeline(max_instances=N_MAX, max_meshes=len(s["meshes"])) as p:
        p.set_mesh_table(s["meshes"])
        prepared = [p.prepare_outputs(async_=False, **o.pointers()) for o in sets]
        for n in _structure_sizes(cu):
            _upload(p, s, n)
            for o in sets:
                o.refill()
            for rep in range(2):
                p.run_views(frames, prepared)
            p.wait()
            for v, o in enumerate(sets):
                o.check(oracle_mod, s, truncate_frame(wants[v], n, bases[v][0]), n, bases[v][0], f"view {v} n={n}")


@pytest.mark.parametrize("wire", [True, "packed"], ids=["wire", "packed"])
def test_wire_forms_at_group_and_window_sizes(ra, oracle_mod, cu, wire):
    for n in _structure_sizes(cu):
        _one_size(ra, oracle_mod, "all_visible", pb.COMMANDS_ONLY, n, f"wire={wire}", wire=wire)


def test_occluded_frames_at_group_and_window_sizes(ra, oracle_mod, cu):
    import occlusion_restatement as occ
    from test_gpu_occlusion import _Outs as OccOuts, _block_depth, _build_pyramid, _check_against_restatement, _run_occluded

    s, big, _, _ = _variant(ra, oracle_mod, "default")
    pv = ra.scene.default_pv()
    w, h = 640, 360
    depth = _block_depth(np.random.default_rng(11), w, h, 40)
    levels = occ.pyramid_levels(depth)
    with ra.InstancePipeline(max_instances=N_MAX, max_meshes=len(s["meshes"])) as p:
        p.set_mesh_table(s["meshes"])
        pyr, _ = _build_pyramid(ra, p, depth)
        for n in _structure_sizes(cu):
            _upload(p, s, n)
            outs = OccOuts(ra, n, tlas=False)
            for rep in range(2):
                _run_occluded(ra, p, s, pyr, w, h, outs)
            want = occ.expected(truncate_frame(big, n), n, pv, levels, w, h)
            _check_against_restatement(outs.result(), want, f"occluded n={n}")
            assert 0 < want["occluded"].sum() < want["in_frustum"].sum()


def test_skinned_frame_at_its_order_threshold(ra, oracle_mod, cu):
    import torch

    from test_gpu_skinned import _check, _random_poses, _random_skeleton

    j = 2
    at = [b.n for b in pb.plan_changes(pb.SKINNED, cu, hi=N_MAX, n_joints=j) if "order" in b.fields][0]
    pb.assert_straddles(at - 1, at, pb.SKINNED, cu, fields=("order",), n_joints=j)
    rng = np.random.default_rng(5)
    s = ra.scene.make_scene(3, n=at)
    sk, poses = _random_skeleton(rng, j), _random_poses(rng, at, j)
    with ra.InstancePipeline(max_instances=at, max_meshes=len(s["meshes"])) as p:
        p.set_mesh_table(s["meshes"])
        p.set_skeleton(sk["parent"], sk["inverse_bind"], sk["joint_box"])
        for n in (at - 1, at):
            want = oracle_mod.run_skinned(s["pos"][:n], s["rot"][:n], s["scale"][:n], s["mesh_id"][:n], s["meshes"], sk, poses[:n],
                                          s["planes"], s["cam_pos"], first_instance_base=7, first_index_base=0xFFFFFF00)
            _upload(p, s, n)
            p.set_poses(poses[:n])
            outs = _Outs(ra, n, pb.STREAMS)
            palette = torch.zeros((n, j, 16), dtype=torch.float32, device=_dev())
            torch.cuda.synchronize()
            kw = outs.pointers()
            for rep in range(2):
                p.run_skinned(_frame(s, 7, 0xFFFFFF00), palette=palette.data_ptr(), **kw)
            p.wait()
            count, total = (int(x) & 0xFFFFFFFF for x in outs.scal[:2].cpu().tolist())
            rows = outs.cmds.cpu().numpy().view(np.uint32)
            assert (rows[count:] == SENTINEL).all() and (outs.model.cpu().numpy().view(np.uint32)[n:] == SENTINEL).all()
            got = dict(model=outs.model[:n].cpu().numpy().view(np.float32), palette=palette.cpu().numpy(),
                       world_aabb=outs.aabb[:n].cpu().numpy().view(np.float32), draw_count=count, draw_index_total=total,
                       visible_bitmap=outs.bitmap[:(n + 31) // 32].cpu().numpy().view(np.uint32),
                       draw_cmds=rows[:count].reshape(-1).view(ra.DRAW_CMD_DTYPE))
            _check(got, want, f"skinned n={n}")


# ---- e. the per-triangle stage at its thresholds ----

_geometry = {}


def _config3_geometry(ra, meshes):
    if "g" not in _geometry:
        _geometry["g"] = ra.scene.make_geometry(meshes)
    return _geometry["g"]


_TRI_PAIRS = [(768, 769), (1_024, 1_025), (3_072, 3_073), (32_768, 32_769), (65_536, 65_537)]


def _triangle_frame(ra, oracle_mod, s, n, vertices, indices, slots, what):
    import torch

    from renderer_amd.pipeline import make_frame

    pv = ra.scene.default_pv()
    r = oracle_mod.run(s["pos"][:n], s["rot"][:n], s["scale"][:n], s["mesh_id"][:n], s["meshes"], s["planes"], s["cam_pos"],
                       first_instance_base=17, threads=8)
    capacity = r["draw_index_total"] + 3
    want_cmds, want_out, _ = oracle_mod.cull_all_triangles(r, s["pos"][:n], s["mesh_id"][:n], s["meshes"], s["cam_pos"], pv, vertices, indices,
                                                           first_instance_base=17, out_capacity=capacity)
    dev = _dev()
    with ra.InstancePipeline(max_instances=n, max_meshes=len(s["meshes"]), frames_in_flight=slots) as p:
        p.set_mesh_table(s["meshes"])
        p.set_geometry(vertices, indices)
        _upload(p, s, n)
        sets = []
        for _ in range(slots):
            sets.append((torch.zeros((n, 16), dtype=torch.float32, device=dev), torch.full((n + SLACK, 5), SENTINEL, dtype=torch.int32, device=dev),
                         torch.zeros(8, dtype=torch.int32, device=dev), torch.full((capacity + SLACK,), -1, dtype=torch.int32, device=dev)))
        torch.cuda.synchronize()
        frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=17, pv=pv)
        for rep in range(2 * slots):
            model, cmds, scal, out = sets[rep % slots]
            p.run_device(frame, model=model.data_ptr(), draw_cmds=cmds.data_ptr(), draw_count=scal.data_ptr(), draw_index_total=scal.data_ptr() + 4,
                         culled_index_buffer=out.data_ptr(), culled_index_capacity=capacity, async_=slots > 1)
        p.wait()
        torch.cuda.synchronize()
        for k, (model, cmds, scal, out) in enumerate(sets):
            count, total = (int(x) & 0xFFFFFFFF for x in scal[:2].cpu().tolist())
            assert count == len(want_cmds) and total == r["draw_index_total"], (what, k)   # (the total of an overflowing frame would differ: the overflow word)
            rows = cmds.cpu().numpy().view(np.uint32)
            assert rows[:count].reshape(-1).view(ra.DRAW_CMD_DTYPE).tobytes() == want_cmds.tobytes(), (what, k)
            assert (rows[count:] == SENTINEL).all(), (what, k)
            stream = out.cpu().numpy().view(np.uint32)
            assert np.array_equal(stream[:capacity], want_out) and (stream[capacity:] == 0xFFFFFFFF).all(), (what, k)


@pytest.mark.parametrize("slots", [1, 2])
@pytest.mark.parametrize("tuning", ["default", "round4_kernels"])
@pytest.mark.parametrize("below,above", _TRI_PAIRS)
def test_triangle_stage_at_its_thresholds(ra, oracle_mod, cu, monkeypatch, below, above, tuning, slots):
    """Default tuning: the range kernel takes every frame up to 65 536 instances, so only 65 536 / 65 537 (range kernel ->
    range-or-sorted-waves, re-compaction single -> wide) is a plan change, and the probe is asserted to say exactly that. The
    thresholds 768 / 1 024 / 3 072 / 32 768 belong to the round-4 kernels, which stay selectable
    (MIP_TUNE_TRI_CHUNKS_FROM=4294967295): with them every pair straddles — except 1 024 / 1 025 with two frame slots (no parts
    kernel) and 768 / 769 with one (the parts kernel has both sides)."""
    s = ra.scene.make_scene(3, n=above)
    max_lod_tris = int((s["meshes"]["index_len"][:, :2] // 3).max())
    state = dict(max_lod_tris=max_lod_tris, frame_slots=slots)
    if tuning == "round4_kernels":
        monkeypatch.setenv("MIP_TUNE_TRI_CHUNKS_FROM", "4294967295")
        state["tri_chunks_from"] = pb.ROUND4_TRIANGLE_KERNELS
    a, b = pb.plan(below, pb.TRIANGLES, cu, **state), pb.plan(above, pb.TRIANGLES, cu, **state)
    same = (tuning == "default" and below != 65_536) or (tuning == "round4_kernels" and (below, slots) in ((1_024, 2), (768, 1)))
    assert (pb.differing_fields(a, b) == ()) == same, (a, b)
    vertices, indices = _config3_geometry(ra, s["meshes"])
    for n in (below, above):
        _triangle_frame(ra, oracle_mod, s, n, vertices, indices, slots, f"{tuning} slots={slots} n={n}")


@pytest.mark.parametrize("tris", [32_768, 32_769])
def test_parts_kernel_is_refused_by_mesh_size(ra, oracle_mod, cu, monkeypatch, tris):
    monkeypatch.setenv("MIP_TUNE_TRI_CHUNKS_FROM", "4294967295")
    n = 1000
    want_kernel = "parts" if tris == 32_768 else "block"
    assert pb.plan(n, pb.TRIANGLES, cu, max_lod_tris=tris, tri_chunks_from=pb.ROUND4_TRIANGLE_KERNELS)["tri"] == want_kernel
    s = ra.scene.make_scene(1, n=n)
    m = s["meshes"].copy()
    m["n_lods"] = 1
    m["index_len"][0, 0] = 3 * tris
    m["index_offset"][0, 0] = 0
    s = dict(s, meshes=m)
    vertices, indices = ra.scene.make_geometry(m)
    _triangle_frame(ra, oracle_mod, s, n, vertices, indices, 1, f"{tris} triangles")


# ---- f. any dispatch order at a boundary (diagnostic library, one child process at a time) ----

_ORDER_CHILD = r"""
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
os.environ["MIP_LIBRARY"] = os.path.join(sys.argv[1], "renderer_amd", "lib", "libmi_instance_pipeline_dbg.so")
import numpy as np, torch
import oracle, renderer_amd
import test_gpu_boundaries as tb
oracle.build()
sizes = [int(x) for x in sys.argv[2].split(",")]
helps = []
for n in sizes:
    with_help = []
    for shape in (tb.pb.STREAMS, tb.pb.COMMANDS_ONLY):
        s, big, base, index_base = tb._variant(renderer_amd, oracle, "bases", max(sizes))
        want = tb.truncate_frame(big, n, base)
        outs = tb._Outs(renderer_amd, n, shape)
        with renderer_amd.InstancePipeline(max_instances=n, max_meshes=len(s["meshes"])) as p:
            p.set_mesh_table(s["meshes"]); tb._upload(p, s, n)
            for rep in range(4):   # (launches that had to help make the ones after the next follow the first-mover rule: both kinds run)
                if rep: outs.refill()
                outs.run(p, tb._frame(s, base, index_base))
                outs.check(oracle, s, want, n, base, f"scrambled n={n} launch {rep}")
            helps.append(p.timings()["prefix_helps"])
print("HELPS", " ".join(str(h) for h in helps))
"""


@pytest.mark.parametrize("first_mover", [None, "always"])
def test_any_dispatch_order_at_plan_boundaries(cu, first_mover):
    """Tiles numbered by a scrambled permutation of the workgroup index: the help path and the first-mover rule across a
    group-size change (524 289) and across the window edge (1 064 961)."""
    from helpers import report_timing_property

    sizes = [524_289, 1_064_961]
    pb.assert_straddles(524_288, 524_289, pb.STREAMS, cu, fields=("group_shift",))
    assert pb.structure_tiles(pb.STREAMS, cu)[1_064_960 // 256].startswith("window edge")
    env = dict(os.environ, MIP_DEBUG_TILE_ORDER="scramble")
    env.pop("MIP_TUNE_ORDER", None)
    env.pop("MIP_TUNE_FIRST_MOVER", None)
    if first_mover:
        env["MIP_TUNE_FIRST_MOVER"] = first_mover
    out = subprocess.run([sys.executable, "-c", _ORDER_CHILD, ROOT, ",".join(str(n) for n in sizes)], capture_output=True, text=True,
                         timeout=600, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    line = [l for l in out.stdout.split("\n") if l.startswith("HELPS")]
    assert line, out.stdout
    helps = [int(x) for x in line[0].split()[1:]]
    report_timing_property(f"scrambled tiles at {sizes}: helps", helps, "> 0 each", all(h > 0 for h in helps))
