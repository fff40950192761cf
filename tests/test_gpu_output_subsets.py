"""Every valid subset of a frame's outputs (tests/output_subset_cases.py: 48 of them, the empty one included) through every
instantiation of the frame kernels: both orders x both arithmetic tiers at the sizes where a guard can fail, the wire forms,
every mesh-id width, one context that alternates subsets, host outputs, mip_run_many, and the other frame entry points
(skinned, occluded, views, the per-triangle stage). The expectation is always the oracle (or, for the extensions, the
restatement the other GPU modules use); every buffer has sentinel rows in front and behind; every comparison is exact.
That the comparison bites is shown on the CPU (tests/test_output_subset_cases.py): no wrong kernel is run here."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import output_subset_cases as osc
import plan_boundaries as pb

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ra():
    import renderer_amd

    renderer_amd.load_library()
    return renderer_amd


@pytest.fixture(scope="module")
def cu():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


_scenes = {}


def _scene(oracle_mod, n, nonfinite=False, **kw):
    """(scene, oracle frame): computed once, shared, never changed."""
    key = (n, nonfinite, tuple(sorted(kw.items())))
    if key not in _scenes:
        s = osc.subset_scene(n, **kw)
        if nonfinite:
            s["pos"][7, 1] = np.nan
        _scenes[key] = (s, osc.oracle_frame(oracle_mod, s))
    return _scenes[key]


def _frame(s, cam_pos=None, base=None, index_base=None, pv=None, planes=None):
    from renderer_amd.pipeline import make_frame

    return make_frame(s["planes"] if planes is None else planes, s["cam_pos"] if cam_pos is None else cam_pos, first_instance_base=s["base"] if base is None else base,
                      first_index_base=s["index_base"] if index_base is None else index_base, pv=pv)


def _pipeline(ra, s, **kw):
    p = ra.InstancePipeline(max_instances=max(s["n"], 1), max_meshes=kw.pop("max_meshes", len(s["meshes"])), **kw)
    p.set_mesh_table(s["meshes"])
    p.set_blas_addresses(s["blas"])
    p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
    return p


def _set_tuning(monkeypatch, order=None, general=0, **env):
    for key in ("MIP_TUNE_ORDER", "MIP_TUNE_FORCE_GENERAL", "MIP_TUNE_WIDE_IDS", "MIP_TUNE_FIRST_MOVER", "MIP_TUNE_NO_ONE_MESH"):
        monkeypatch.delenv(key, raising=False)
    if order:
        monkeypatch.setenv("MIP_TUNE_ORDER", str(order))
    if general:
        monkeypatch.setenv("MIP_TUNE_FORCE_GENERAL", "1")
    for key, value in env.items():
        monkeypatch.setenv(key, value)


def _sweep_one_size(ra, oracle_mod, s, want, subsets, what, launches=2, wire=False):
    """One context, one allocation of every output; every subset `launches` times with a refill in between. Returns the
    number of frame-kernel launches (an empty scene launches nothing) and the context's timings."""
    n = s["n"]
    outs = osc.SubsetOutputs(osc.TorchBackend(), n, osc.ALL, wire=wire)
    frame = _frame(s)
    launched = 0
    with _pipeline(ra, s) as p:
        for subset in subsets:
            outs.request(subset)
            for rep in range(launches):
                outs.refill()
                p.run_device(frame, wire=wire, **outs.pointers())
                outs.check(oracle_mod, s, want, n, s["base"], f"{what} n={n} launch {rep}")
                launched += 1 if n else 0
        return launched, p.timings()


# ---- a. every subset at every size, both orders, both arithmetic tiers ----

@pytest.mark.parametrize("general", [0, 1], ids=["fast", "general"])
@pytest.mark.parametrize("order", [1, 3], ids=["stores_first", "commands_first"])
def test_every_subset_at_every_size(ra, oracle_mod, cu, monkeypatch, order, general):
    _set_tuning(monkeypatch, order, general)
    for n in osc.SIZES:
        s, want = _scene(oracle_mod, n)
        for subset in (osc.ALL, frozenset({"bitmap"}), frozenset({"cmds"})) if n else ():
            plan = pb.plan(n, osc.plan_request(subset), cu, force_order=order, force_general=general)
            assert plan["order"] == order and plan["general"] == general and plan["uses_prefix_state"] == int("cmds" in subset)
        launched, t = _sweep_one_size(ra, oracle_mod, s, want, osc.SUBSETS, f"order {order} general {general}")
        assert t["general_launches"] == (launched if general else 0), (n, t["general_launches"], launched)
    if general:   # a genuinely non-finite instance: the row-3 NaN bits of the kGeneral kernels carry something
        for n in (33, 1000):
            s, want = _scene(oracle_mod, n, nonfinite=True)
            assert np.isnan(want["model"][7]).any() and not np.isnan(want["model"][8]).any()
            launched, t = _sweep_one_size(ra, oracle_mod, s, want, osc.SUBSETS, f"order {order} NaN at instance 7", launches=1)
            assert t["general_launches"] == launched


def test_a_nonfinite_instance_selects_the_general_kernel_for_every_subset(ra, oracle_mod, monkeypatch):
    """Without MIP_TUNE_FORCE_GENERAL: the upload census alone sends every subset to the general kernel."""
    _set_tuning(monkeypatch)
    s, want = _scene(oracle_mod, 1000, nonfinite=True)
    launched, t = _sweep_one_size(ra, oracle_mod, s, want, osc.SUBSETS, "census", launches=1)
    assert t["general_launches"] == launched == len(osc.SUBSETS)


def test_the_comparison_bites_on_device_buffers(ra, oracle_mod, monkeypatch):
    """The mutants are run on the CPU only; here the same check, reading DEVICE buffers of a right frame, must reject an
    expectation that is off by one bit in any output, and a word poked into any buffer's slack. No wrong kernel runs."""
    import torch

    _set_tuning(monkeypatch)
    n = 1000
    s, want = _scene(oracle_mod, n)
    outs = osc.SubsetOutputs(osc.TorchBackend(), n, osc.ALL)
    with _pipeline(ra, s) as p:
        p.run_device(_frame(s), **outs.pointers())
    outs.check(oracle_mod, s, want, n, s["base"], "right frame")

    def rejected(wrong):
        with pytest.raises(AssertionError):
            outs.check(oracle_mod, s, wrong, n, s["base"], "wrong expectation")

    for key, where in (("model", (n - 1, 13)), ("world_aabb", (n - 1, 5)), ("tlas", (n - 1, 14)), ("tlas", (n - 1, 3)), ("visible_bitmap", (n - 1) // 32)):
        wrong = dict(want, **{key: want[key].copy()})
        wrong[key].view(np.uint32)[where] ^= np.uint32(1)
        rejected(wrong)
    cmds = want["draw_cmds"].copy()
    cmds["firstIndex"][-1] ^= np.uint32(1)
    rejected(dict(want, draw_cmds=cmds))
    rejected(dict(want, draw_count=want["draw_count"] - 1, draw_cmds=want["draw_cmds"][:-1]))   # the last row is then behind the list
    rejected(dict(want, draw_index_total=want["draw_index_total"] ^ 1))
    for name, b in list(outs.buf.items()) + [("scalars", outs.scal)]:
        for word in (0, len(b) - 1) if name != "scalars" else (osc.COUNT_WORD + 1,):
            kept = int(b[word].item())
            b[word] = 7
            torch.cuda.synchronize()
            rejected(want)
            b[word] = kept
    outs.check(oracle_mod, s, want, n, s["base"], "right frame again")


# ---- b. wire forms ----

@pytest.mark.parametrize("order", [1, 3], ids=["stores_first", "commands_first"])
@pytest.mark.parametrize("wire", [True, "packed"], ids=["wire", "packed"])
def test_wire_forms_with_every_subset(ra, oracle_mod, monkeypatch, wire, order):
    _set_tuning(monkeypatch, order)
    subsets = [s for s in osc.SUBSETS if "cmds" in s]
    assert len(subsets) == 32
    for n in (1000, 4129):
        s, want = _scene(oracle_mod, n)
        _sweep_one_size(ra, oracle_mod, s, want, subsets, f"wire={wire} order {order}", launches=1, wire=wire)


# ---- c. every width of the frame kernel's mesh ids ----

_ID_SUBSETS = [frozenset(x) for x in ({"tlas"}, {"tlas", "cmds"}, {"model"}, {"aabb", "bitmap"}, {"cmds"}, osc.ALL)]
_ID_TABLES = {"one_mesh": (1, {}), "u8": (64, {}), "u16": (300, {}), "u32": (70_000, {}), "u32_by_env": (64, {"MIP_TUNE_WIDE_IDS": "1"})}


@pytest.mark.parametrize("order", [1, 3], ids=["stores_first", "commands_first"])
@pytest.mark.parametrize("table", list(_ID_TABLES))
def test_id_widths(ra, oracle_mod, monkeypatch, table, order):
    n_meshes, env = _ID_TABLES[table]
    _set_tuning(monkeypatch, order, **env)
    n = 1000
    s, want = _scene(oracle_mod, n, n_meshes=n_meshes, top_mesh_in_last_tile=True)
    top = n_meshes - 1
    last_tile = s["mesh_id"][(n - 1) // osc.TILE * osc.TILE:]
    assert len(s["meshes"]) == n_meshes and (last_tile == top).sum() >= 3 and s["mesh_id"][n - 1] == top
    assert len(set(s["blas"].tolist())) == n_meshes
    assert (want["tlas"][s["mesh_id"] == top, 14] == np.uint32(int(s["blas"][top]) & 0xFFFFFFFF)).all()
    if n_meshes > 64:
        assert len(np.unique(s["mesh_id"])) > 64 and int(s["mesh_id"].max()) == top
    drawn = (want["draw_cmds"]["firstInstance"] - np.uint32(s["base"])).astype(np.int64)
    assert n - 1 in drawn
    _sweep_one_size(ra, oracle_mod, s, want, _ID_SUBSETS, f"{table} order {order}")


# ---- d. one context, alternating subsets ----

_SEQUENCE = [osc.ALL, frozenset({"bitmap"}), frozenset({"cmds", "index_total"}), frozenset({"model"}), frozenset({"tlas", "aabb"}),
             frozenset({"cmds"}), osc.ALL, osc.EMPTY, osc.ALL]


@pytest.mark.parametrize("order", [None, 1, 3], ids=["plan_order", "stores_first", "commands_first"])
@pytest.mark.parametrize("slots", [1, 2])
def test_one_context_alternating_subsets(ra, oracle_mod, monkeypatch, slots, order):
    """A command-less frame takes no tag and does not touch the prefix state: the frames with commands around it come out
    right, on one slot and with two frames in flight (every frame into buffers of its own, checked after one wait)."""
    _set_tuning(monkeypatch, order)
    be = osc.TorchBackend()
    for n in (1000, 4129):
        s, want = _scene(oracle_mod, n)
        frame = _frame(s)
        with _pipeline(ra, s, frames_in_flight=slots) as p:
            for rnd in range(2):   # twice: the second round starts on the state the first one left
                sets = [osc.SubsetOutputs(be, n, subset) for subset in _SEQUENCE]
                for k, o in enumerate(sets):
                    p.run_device(frame, async_=slots > 1, **o.pointers())
                    if slots == 1:
                        o.check(oracle_mod, s, want, n, s["base"], f"n={n} round {rnd} frame {k}")
                if slots > 1:
                    p.wait()
                    for k, o in enumerate(sets):
                        o.check(oracle_mod, s, want, n, s["base"], f"n={n} two slots, round {rnd} frame {k}")


# ---- the empty subset: MIP_OK, nothing written, context usable ----

@pytest.mark.parametrize("n", [0, 1000])
def test_a_frame_without_outputs_is_ok_and_writes_nothing(ra, oracle_mod, monkeypatch, n):
    _set_tuning(monkeypatch)
    s, want = _scene(oracle_mod, n)
    outs = osc.SubsetOutputs(osc.TorchBackend(), n, osc.ALL)
    frame = _frame(s)
    with _pipeline(ra, s) as p:
        out = ra._lib.MipOutputs()
        out.flags = ra._lib.MIP_OUT_DEVICE
        for flags in (ra._lib.MIP_OUT_DEVICE, ra._lib.MIP_OUT_DEVICE | ra._lib.MIP_OUT_ASYNC, ra._lib.MIP_OUT_HOST):
            out.flags = flags
            assert p._lib.mip_run(p._ctx, C.byref(frame), C.byref(out)) == 0     # MIP_OK
            p.wait()
            outs.untouched(f"a frame without outputs (flags {flags})")
        p.run_device(frame, **outs.pointers())                                # the next full frame is right
        outs.check(oracle_mod, s, want, n, s["base"], f"full frame after empty ones n={n}")


# ---- e. host outputs ----

def _run_host(ra, p, frame, outs):
    out = ra._lib.MipOutputs()
    out.flags = ra._lib.MIP_OUT_HOST
    kw = outs.pointers()
    out.model = kw["model"] or None
    out.visible_bitmap = kw["visible_bitmap"] or None
    out.world_aabb = kw["world_aabb"] or None
    out.draw_cmds = kw["draw_cmds"] or None
    out.draw_count = kw["draw_count"] or None
    out.draw_index_total = kw["draw_index_total"] or None
    out.tlas_instances = kw["tlas_instances"] or None
    return p._lib.mip_run(p._ctx, C.byref(frame), C.byref(out))


@pytest.mark.parametrize("n", [0, 33, 1000])
def test_host_outputs_subset_by_subset(ra, oracle_mod, monkeypatch, n):
    """MIP_OUT_HOST through mip_run itself (run_host cannot ask for commands without draw_index_total): the staging buffers
    are allocated per pointer, subset by subset on a fresh context, then used again in the reverse order."""
    _set_tuning(monkeypatch)
    s, want = _scene(oracle_mod, n)
    subsets = [x for x in osc.SUBSETS if "tlas" not in x]
    assert len(subsets) == 24
    frame = _frame(s)
    be = osc.NumpyBackend()
    with _pipeline(ra, s) as p:
        for direction, seq in (("forward", subsets), ("reverse", subsets[::-1])):
            for subset in seq:
                outs = osc.SubsetOutputs(be, n, subset)
                assert _run_host(ra, p, frame, outs) == 0, p._lib.mip_last_error(p._ctx)
                outs.check(oracle_mod, s, want, n, s["base"], f"host outputs {direction} n={n}")
        for subset in (frozenset({"tlas"}), osc.ALL):   # TLAS rows need device outputs: refused, nothing written
            outs = osc.SubsetOutputs(be, n, subset)
            assert _run_host(ra, p, frame, outs) == -1, "MIP_ERR_INVALID_ARGUMENT"
            outs.untouched(f"refused host frame [{osc.subset_id(subset)}]")
        outs = osc.SubsetOutputs(be, n, osc.ALL - {"tlas"})
        assert _run_host(ra, p, frame, outs) == 0
        outs.check(oracle_mod, s, want, n, s["base"], "host outputs after a refused frame")


# ---- f. mip_run_many ----

_MANY = {"cmds": {"cmds"}, "cmds_tlas_aabb": {"cmds", "tlas", "aabb"}, "model_bitmap": {"model", "bitmap"}, "cmds_model_total": {"cmds", "model", "index_total"}}


@pytest.mark.parametrize("kind", list(_MANY))
def test_run_many_with_partial_output_sets(ra, oracle_mod, monkeypatch, kind):
    """Two output sets per frame slot, 130 steps (rounds of recorded graphs and a remainder where every set asks for commands;
    plain calls otherwise), two cameras: every set holds the frame of the camera that wrote it last."""
    from helpers import report_timing_property

    _set_tuning(monkeypatch)
    subset, slots, steps, n = frozenset(_MANY[kind]), 2, 130, 4129
    s, _ = _scene(oracle_mod, n)
    cams = [s["cam_pos"], np.array((3.0, 2.0, -5.0), np.float32)]
    bases = [(s["base"], s["index_base"]), (77, 0x80000000)]
    planes = [oracle_mod.project_camera(cam_pos=c) for c in cams]
    wants = [osc.oracle_frame(oracle_mod, s, cam_pos=c, base=b, index_base=ib, planes=pl) for c, (b, ib), pl in zip(cams, bases, planes)]
    assert wants[0]["draw_count"] != wants[1]["draw_count"] and not np.array_equal(wants[0]["visible_bitmap"], wants[1]["visible_bitmap"])
    frames = [_frame(s, cam_pos=c, base=b, index_base=ib, planes=pl) for c, (b, ib), pl in zip(cams, bases, planes)]
    be = osc.TorchBackend()
    sets = [osc.SubsetOutputs(be, n, subset) for _ in range(2 * slots)]
    with _pipeline(ra, s, frames_in_flight=slots) as p:
        prepared = [p.prepare_outputs(**o.pointers()) for o in sets]
        for rnd in range(2):
            for o in sets:
                o.refill()
            p.run_many(frames, prepared, steps)
            p.wait()
            for j, o in enumerate(sets):
                last = max(k for k in range(steps) if k % len(sets) == j)
                cam = last % len(frames)
                o.check(oracle_mod, s, wants[cam], n, bases[cam][0], f"run_many {kind} round {rnd} set {j} (step {last}, camera {cam})")
        t = p.timings()
        report_timing_property(f"run_many {kind}: graph_records / graph_frames", (t["graph_records"], t["graph_frames"]),
                               "graphs only where every set has commands", (t["graph_frames"] > 0) == ("cmds" in subset))


# ---- g. the other frame entry points ----

def _skeleton_and_poses(n, j=3):
    from test_gpu_skinned import _random_poses, _random_skeleton

    rng = np.random.default_rng(5)
    return _random_skeleton(rng, j), _random_poses(rng, n, j)


@pytest.mark.parametrize("n", [1000, 4129])
def test_skinned_frames_with_every_subset(ra, oracle_mod, monkeypatch, n):
    import torch

    from helpers import float_mismatches

    _set_tuning(monkeypatch)
    s, _ = _scene(oracle_mod, n)
    j = 3
    sk, poses = _skeleton_and_poses(n, j)
    want = oracle_mod.run_skinned(s["pos"], s["rot"], s["scale"], s["mesh_id"], s["meshes"], sk, poses, s["planes"], s["cam_pos"],
                                  first_instance_base=s["base"], first_index_base=s["index_base"])
    want["tlas"] = oracle_mod.tlas_instances(want["model"], s["mesh_id"], s["blas"], first_instance_base=s["base"])
    assert 0 < want["draw_count"] < n
    outs = osc.SubsetOutputs(osc.TorchBackend(), n, osc.ALL)
    palette = torch.full(((n + 2 * osc.SLACK) * j * 16,), osc.SENTINEL, dtype=torch.int32, device=torch.device("cuda", 0))
    front = osc.SLACK * j * 16
    frame = _frame(s)
    with _pipeline(ra, s) as p:
        p.set_skeleton(sk["parent"], sk["inverse_bind"], sk["joint_box"])
        p.set_poses(poses)
        for subset in osc.SUBSETS:
            for with_palette in (True, False):
                outs.request(subset).refill()
                palette.fill_(osc.SENTINEL)
                torch.cuda.synchronize()
                p.run_skinned(frame, palette=palette.data_ptr() + 4 * front if with_palette else 0, **outs.pointers())
                what = f"skinned n={n} palette={with_palette}"
                outs.check(oracle_mod, s, want, n, s["base"], what)
                words = palette.cpu().numpy().view(np.uint32)
                own = words[front:front + n * j * 16]
                assert (words[:front] == osc.SENTINEL).all() and (words[front + n * j * 16:] == osc.SENTINEL).all(), f"{what}: palette slack"
                if with_palette:
                    mm = float_mismatches(own.view(np.float32).reshape(n, j, 16), want["palette"])
                    assert len(mm) == 0, f"{what} [{osc.subset_id(subset)}]: {len(mm)} palette entries differ"
                else:
                    assert (own == osc.SENTINEL).all(), f"{what}: palette written through a NULL pointer"


def _occluder_depth(w, h):
    """Random block depths, and an occluder at view distance 20 over the middle of the image: it hides the far instance n - 1
    (at distance 38) and not the near instance 0 (at distance 6)."""
    from test_gpu_occlusion import _block_depth, _ndc_z

    depth = _block_depth(np.random.default_rng(11), w, h, 40)
    depth[h // 4: 3 * h // 4, w // 4: 3 * w // 4] = _ndc_z(20.0)
    return depth


@pytest.mark.parametrize("n", [1000, 4129])
def test_occluded_frames_with_every_subset(ra, oracle_mod, monkeypatch, n):
    import torch

    import occlusion_restatement as occ
    from renderer_amd.pipeline import make_occlusion
    from test_gpu_occlusion import _build_pyramid

    _set_tuning(monkeypatch)
    s, frustum = _scene(oracle_mod, n)
    pv = ra.scene.default_pv()
    w, h = 640, 360
    depth = _occluder_depth(w, h)
    e = occ.expected(frustum, n, pv, occ.pyramid_levels(depth), w, h, first_instance_base=s["base"], first_index_base=s["index_base"])
    assert e["occluded"][n - 1] and not e["occluded"][0] and e["visible"][0]
    assert 0 < e["occluded"].sum() < e["in_frustum"].sum()
    want = dict(frustum, visible_bitmap=e["visible_bitmap"], draw_cmds=e["draw_cmds"], draw_count=e["draw_count"], draw_index_total=e["draw_index_total"])
    words = (n + 31) // 32
    outs = osc.SubsetOutputs(osc.TorchBackend(), n, osc.ALL)
    occluded = torch.full((words + 2 * osc.SLACK,), osc.SENTINEL, dtype=torch.int32, device=torch.device("cuda", 0))
    frame = _frame(s)
    with _pipeline(ra, s) as p:
        pyr, _ = _build_pyramid(ra, p, depth)
        for subset in osc.SUBSETS:
            for with_bitmap in (True, False):
                outs.request(subset).refill()
                occluded.fill_(osc.SENTINEL)
                torch.cuda.synchronize()
                kw = outs.pointers()
                out = p.prepare_outputs(async_=False, **kw)
                o = make_occlusion(w, h, pyr.data_ptr(), pv, occluded_bitmap=occluded.data_ptr() + 4 * osc.SLACK if with_bitmap else 0)
                p.run_occluded(frame, o, out)
                what = f"occluded n={n} occluded_bitmap={with_bitmap}"
                outs.check(oracle_mod, s, want, n, s["base"], what)
                got = occluded.cpu().numpy().view(np.uint32)
                assert (got[:osc.SLACK] == osc.SENTINEL).all() and (got[osc.SLACK + words:] == osc.SENTINEL).all(), f"{what}: occluded bitmap slack"
                own = got[osc.SLACK:osc.SLACK + words]
                if with_bitmap:
                    assert np.array_equal(own, e["occluded_bitmap"]), f"{what} [{osc.subset_id(subset)}]: occluded bitmap"
                else:
                    assert (own == osc.SENTINEL).all()


@pytest.mark.parametrize("n", [1000, 4129])
def test_views_with_their_own_optional_outputs(ra, oracle_mod, monkeypatch, n):
    """Five views = two launches; bitmap and index total differ per view. A view without a bitmap must not write through a
    neighbour's pointer: every buffer's sentinels are checked."""
    _set_tuning(monkeypatch)
    s, _ = _scene(oracle_mod, n)
    extras = [{"bitmap", "index_total"}, {"bitmap"}, {"index_total"}, set(), {"bitmap", "index_total"}]
    cams = [np.array(c, np.float32) for c in ((0, 1, 2), (5, 1, 2), (-3, 2, 8), (0, 1, 30), (1, 0, -4))]
    bases = [(s["base"], s["index_base"]), (1000, 0xFFFFF000), (7, 77), (0, 1 << 31), (5, 0xFFFFFFFF)]
    planes = [oracle_mod.project_camera(cam_pos=c) for c in cams]
    wants = [osc.oracle_frame(oracle_mod, s, cam_pos=c, base=b, index_base=ib, planes=pl) for c, (b, ib), pl in zip(cams, bases, planes)]
    assert len({w["visible_bitmap"].tobytes() for w in wants}) == len(wants) and all(w["draw_count"] > 0 for w in wants)
    be = osc.TorchBackend()
    sets = [osc.SubsetOutputs(be, n, frozenset({"cmds"} | x)) for x in extras]
    frames = [_frame(s, cam_pos=c, base=b, index_base=ib, planes=pl) for c, (b, ib), pl in zip(cams, bases, planes)]
    with _pipeline(ra, s) as p:
        prepared = [p.prepare_outputs(async_=False, **{k: v for k, v in o.pointers().items() if k not in ("model", "world_aabb", "tlas_instances")}) for o in sets]
        for rep in range(3):
            for o in sets:
                o.refill()
            p.run_views(frames, prepared)
            p.wait()
            for v, o in enumerate(sets):
                o.check(oracle_mod, s, wants[v], n, bases[v][0], f"view {v} n={n} call {rep}")


_geometry = {}


def test_triangle_stage_with_every_optional_output(ra, oracle_mod, monkeypatch):
    """model + draw_cmds + culled_index_buffer, and every subset of {bitmap, aabb, tlas, index_total} beside them."""
    import itertools

    import torch

    _set_tuning(monkeypatch)
    n, base = 1000, 17
    s, _ = _scene(oracle_mod, n)
    pv = ra.scene.default_pv()
    r = osc.oracle_frame(oracle_mod, s, base=base, index_base=0)
    vertices, indices = ra.scene.make_geometry(s["meshes"])
    capacity = r["draw_index_total"] + 3
    want_cmds, want_stream, _ = oracle_mod.cull_all_triangles(r, s["pos"], s["mesh_id"], s["meshes"], s["cam_pos"], pv, vertices, indices,
                                                              first_instance_base=base, out_capacity=capacity)
    want = dict(r, draw_cmds=want_cmds, draw_count=len(want_cmds))
    assert 0 < len(want_cmds) <= r["draw_count"] and int(want_cmds["indexCount"].sum()) < int(r["draw_cmds"]["indexCount"].sum())
    outs = osc.SubsetOutputs(osc.TorchBackend(), n, osc.ALL)
    stream = torch.full((capacity + osc.SLACK,), -1, dtype=torch.int32, device=torch.device("cuda", 0))
    frame = _frame(s, base=base, index_base=0, pv=pv)
    with _pipeline(ra, s) as p:
        p.set_geometry(vertices, indices)
        for k in range(5):
            for extra in itertools.combinations(("bitmap", "aabb", "tlas", "index_total"), k):
                outs.request(frozenset({"model", "cmds"} | set(extra))).refill()
                stream.fill_(-1)
                torch.cuda.synchronize()
                p.run_device(frame, culled_index_buffer=stream.data_ptr(), culled_index_capacity=capacity, **outs.pointers())
                what = f"triangle stage + {extra}"
                outs.check(oracle_mod, s, want, n, base, what)
                got = stream.cpu().numpy().view(np.uint32)
                assert np.array_equal(got[:capacity], want_stream) and (got[capacity:] == 0xFFFFFFFF).all(), what


# ---- h. any dispatch order (diagnostic library, one child process at a time) ----

_ORDER_CHILD = r"""
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
os.environ["MIP_LIBRARY"] = os.path.join(sys.argv[1], "renderer_amd", "lib", "libmi_instance_pipeline_dbg.so")
import oracle, renderer_amd
import output_subset_cases as osc
import test_gpu_output_subsets as t
oracle.build()
n = int(sys.argv[2])
helps = []
for order in (1, 3):
    os.environ["MIP_TUNE_ORDER"] = str(order)
    s, want = t._scene(oracle, n)
    launched, timings = t._sweep_one_size(renderer_amd, oracle, s, want, osc.SUBSETS, f"scrambled order {order}", launches=4)
    helps.append(timings["prefix_helps"])
print("HELPS", " ".join(str(h) for h in helps))
"""


@pytest.mark.parametrize("first_mover", [None, "always"])
def test_any_dispatch_order_with_every_subset(first_mover):
    """Tiles numbered by a scrambled permutation of the workgroup index: whoever runs first, every subset's frame is the same."""
    from helpers import report_timing_property

    n = 4129
    env = dict(os.environ, MIP_DEBUG_TILE_ORDER="scramble")
    for key in ("MIP_TUNE_ORDER", "MIP_TUNE_FIRST_MOVER", "MIP_TUNE_FORCE_GENERAL", "MIP_TUNE_WIDE_IDS"):
        env.pop(key, None)
    if first_mover:
        env["MIP_TUNE_FIRST_MOVER"] = first_mover
    out = subprocess.run([sys.executable, "-c", _ORDER_CHILD, ROOT, str(n)], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    line = [l for l in out.stdout.split("\n") if l.startswith("HELPS")]
    assert line, out.stdout
    helps = [int(x) for x in line[0].split()[1:]]
    report_timing_property(f"scrambled tiles, every subset at {n}: helps per order", helps, "reported only", True)
