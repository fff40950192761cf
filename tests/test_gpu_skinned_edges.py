"""The skinning kernel (renderer_amd/csrc/skinning_kernel.hpp) at the shapes its own structure singles out: every joint
count at every edge of its lane mapping, the hierarchy families, the guard of the separable box fold from finite inputs, a
NULL palette, two frames in flight at one workgroup and one instance. The inputs come from tests/skinned_cases.py;
tests/test_oracle.py shows that the oracle is the float64 definition up to float32 rounding on the same arrays, so the
expectation here is the oracle, bit for bit in the integers and number for number in the floats. Every device output
carries SLACK sentinel rows (or words) behind it that must survive: the palette leaves the kernel re-packed to 1 KiB per
store instruction, and a store past the last instance is invisible in a buffer of exactly n rows."""
import numpy as np
import pytest

import skinned_cases as sc
from test_gpu_skinned import _check

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
SLACK = 64
BASES = (123_456, 0xFFFFFF00)   # first_instance_base, first_index_base: firstIndex wraps inside the list


@pytest.fixture(scope="module")
def ra():
    import renderer_amd

    renderer_amd.load_library()
    return renderer_amd


def _dev():
    import torch

    return torch.device("cuda", 0)


class _Outs:
    """Device outputs of one skinned frame of n instances and j joints, each with SLACK sentinel rows / words behind it."""

    def __init__(self, n, j, palette=True):
        import torch

        def full(*dims):
            return torch.full(dims, SENTINEL, dtype=torch.int32, device=_dev())

        self.n, self.j = n, j
        self.palette = full(n + SLACK, j, 16) if palette else None
        self.model, self.aabb, self.cmds = full(n + SLACK, 16), full(n + SLACK, 6), full(n + SLACK, 5)
        self.bitmap = full((n + 31) // 32 + SLACK)
        self.scal = full(8)
        torch.cuda.synchronize()  # torch fills on its own stream; the library's streams do not wait for it

    def pointers(self):
        return dict(model=self.model.data_ptr(), visible_bitmap=self.bitmap.data_ptr(), draw_cmds=self.cmds.data_ptr(),
                    draw_count=self.scal.data_ptr(), draw_index_total=self.scal.data_ptr() + 4, world_aabb=self.aabb.data_ptr())

    def result(self, ra, what):
        """The frame as _check wants it, after asserting that nothing behind it was written."""
        n, words = self.n, (self.n + 31) // 32
        count, total = (int(x) & 0xFFFFFFFF for x in self.scal[:2].cpu().tolist())
        assert count <= n, f"{what}: draw_count {count} > n {n}"
        rows = self.cmds.cpu().numpy().view(np.uint32)
        model, aabb, bitmap = (x.cpu().numpy().view(np.uint32) for x in (self.model, self.aabb, self.bitmap))
        assert (rows[count:] == SENTINEL).all(), f"{what}: a command row behind the list was written"
        assert (model[n:] == SENTINEL).all(), f"{what}: a model row behind the frame was written"
        assert (aabb[n:] == SENTINEL).all(), f"{what}: a world-box row behind the frame was written"
        assert (bitmap[words:] == SENTINEL).all(), f"{what}: a bitmap word behind the frame was written"
        got = dict(model=model[:n].view(np.float32), world_aabb=aabb[:n].view(np.float32), visible_bitmap=bitmap[:words].copy(),
                   draw_count=count, draw_index_total=total, draw_cmds=rows[:count].reshape(-1).view(ra.DRAW_CMD_DTYPE))
        if self.palette is not None:
            pal = self.palette.cpu().numpy().view(np.uint32)
            assert (pal[n:] == SENTINEL).all(), f"{what}: a palette row behind the last instance was written"
            got["palette"] = pal[:n].view(np.float32)
        return got


def _want(oracle_mod, s, sk, poses, bases=BASES):
    return oracle_mod.run_skinned(s["pos"], s["rot"], s["scale"], s["mesh_id"], s["meshes"], sk, poses, s["planes"], s["cam_pos"],
                                  first_instance_base=bases[0], first_index_base=bases[1])


def _frame(s, bases=BASES):
    from renderer_amd.pipeline import make_frame

    return make_frame(s["planes"], s["cam_pos"], first_instance_base=bases[0], first_index_base=bases[1])


def _run_on(ra, p, s, poses, j, device_poses=False, palette=True):
    """Instances, poses and one skinned frame on a context whose mesh table and skeleton are set."""
    import torch

    n = s["n"]
    p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
    held = None
    if device_poses:
        held = torch.from_numpy(np.ascontiguousarray(poses)).to(_dev())
        torch.cuda.synchronize()
        p.set_poses_device(held.data_ptr(), n)
    else:
        p.set_poses(poses)
    outs = _Outs(n, j, palette=palette)
    p.run_skinned(_frame(s), palette=outs.palette.data_ptr() if palette else 0, **outs.pointers())
    p.wait()
    del held
    return outs


def _context(ra, s, sk, n_max, **kw):
    p = ra.InstancePipeline(max_instances=n_max, max_meshes=len(s["meshes"]), **kw)
    p.set_mesh_table(s["meshes"])
    p.set_skeleton(sk["parent"], sk["inverse_bind"], sk["joint_box"])
    return p


def _compare(got, want, what, palette=True):
    if not palette:
        got = dict(got, palette=want["palette"])
    _check(got, want, what)


@pytest.mark.parametrize("j", range(1, 33))
def test_every_joint_count_at_every_block_edge(ra, oracle_mod, j):
    """J = 1 .. 32 (the lane mapping is a multiply-shift by ceil(2^16 / J); `valid`, `pair` and `in_block` all hang on J) at
    1, ipw, ipw + 1, ipb - 1, ipb, ipb + 1 and 2 ipb + ipw + 1 instances: a lane past the last whole instance of a wave, a
    partly filled last wave, a last workgroup of one instance. Host poses for odd J, device poses for even J."""
    sk, poses = sc.family_case("bushy", j)
    sizes = sc.sizes(j)
    with _context(ra, sc.instances(sizes[-1]), sk, sizes[-1]) as p:
        for n in sizes:
            s = sc.instances(n)
            want = _want(oracle_mod, s, sk, poses[:n])
            got = _run_on(ra, p, s, poses[:n], j, device_poses=(j % 2 == 0)).result(ra, f"J={j} n={n}")
            _compare(got, want, f"J={j} n={n}")


@pytest.mark.parametrize("family", ["chain", "star", "forest", "comb"])
@pytest.mark.parametrize("j", [2, 3, 5, 8, 21, 22, 32])
def test_every_hierarchy_family(ra, oracle_mod, j, family):
    """chain: depth J - 1, one joint and one barrier per level; star: one level of J - 1 joints, in_block * cnt close to 256;
    forest: max_depth 0 with J > 1; comb: levels whose joints are not their parents' neighbours."""
    sk, poses = sc.family_case(family, j)
    ipw, ipb = sc.ipw_ipb(j)
    sizes = (ipb + 1, 2 * ipb + ipw + 1)
    with _context(ra, sc.instances(sizes[-1]), sk, sizes[-1]) as p:
        for n in sizes:
            s = sc.instances(n)
            want = _want(oracle_mod, s, sk, poses[:n])
            got = _run_on(ra, p, s, poses[:n], j, device_poses=(j % 2 == 1)).result(ra, f"{family} J={j} n={n}")
            _compare(got, want, f"{family} J={j} n={n}")


def test_guard_bands_from_finite_inputs(ra, oracle_mod):
    """The three bands of the separable fold's guard in ONE launch (tests/skinned_cases.py): whole waves below the guard, waves
    that cross it, and waves that hold instances of every band. Inputs are finite throughout; instances of the two finite
    bands must come out finite on the GPU as well."""
    n = 600
    sk, poses, s = sc.guard_skeleton(), sc.guard_poses(n), sc.guard_instances(n)
    want = _want(oracle_mod, s, sk, poses)
    bands = sc.guard_bands(sk, want)
    with _context(ra, s, sk, n) as p:
        outs = _run_on(ra, p, s, poses, 5)
        got = outs.result(ra, "guard bands")
        _compare(got, want, "guard bands")
        finite_band = bands["separable"] | bands["corner"]
        assert np.isfinite(got["world_aabb"][finite_band]).all() and np.isfinite(got["palette"][finite_band]).all()
        with np.errstate(over="ignore"):   # overflow band: a product of the big joint's x column with the big coordinate does overflow
            reach = got["palette"].reshape(n, 5, 16)[:, sc.BIG_JOINT, 0:3] * np.float32(sc.BIG_BOX)
        assert np.isinf(reach[bands["overflow"]]).any(axis=1).all() and np.isfinite(reach[finite_band]).all()


@pytest.mark.parametrize("which", ["inf_max", "nan_coordinate"])
def test_non_finite_joint_boxes(ra, oracle_mod, which):
    """box_bound = +inf (where 0 * inf is NaN, so a zero palette entry cannot pass the guard): a joint box whose maximum is
    +inf, and one with a NaN coordinate, which the > test does not call empty."""
    sk = sc.nonfinite_box_skeletons()[which]
    n = sc.sizes(5)[-1]
    s, poses = sc.instances(n), sc.guard_poses(600)[:n]
    poses[7, :, 7:10] = 0.0    # zero scales: palette entries that are exactly zero meet the infinite bound
    want = _want(oracle_mod, s, sk, poses)
    with _context(ra, s, sk, n) as p:
        _compare(_run_on(ra, p, s, poses, 5, device_poses=True).result(ra, which), want, which)


def test_null_palette_gives_the_same_frame(ra, oracle_mod):
    """palette = NULL skips the staging through LDS and the stores; boxes, bitmap and commands must not notice."""
    j = 7
    sk, poses = sc.family_case("comb", j)
    n = sc.sizes(j)[-1]
    s = sc.instances(n)
    want = _want(oracle_mod, s, sk, poses)
    with _context(ra, s, sk, n) as p:
        got = _run_on(ra, p, s, poses, j, palette=False).result(ra, "NULL palette")
        _compare(got, want, "NULL palette", palette=False)
        _compare(_run_on(ra, p, s, poses, j).result(ra, "palette after NULL"), want, "palette after NULL")


def test_two_frames_in_flight_over_a_chain_of_32(ra, oracle_mod):
    """Alternating device pose buffers, frames queued without waiting on two frame slots, at n = ipb + 1 = 9: two
    workgroups, the second with one instance, 31 levels each."""
    import torch

    j = 32
    sk, poses_a = sc.family_case("chain", j)
    n = sc.ipw_ipb(j)[1] + 1
    s = sc.instances(n)
    poses_a = np.ascontiguousarray(poses_a[:n])
    poses_b = np.ascontiguousarray(sc.family_case("comb", j)[1][:n])   # other values, same layout
    wants = [_want(oracle_mod, s, sk, x) for x in (poses_a, poses_b)]
    assert len(np.argwhere(wants[0]["palette"] != wants[1]["palette"])) > n * j
    with _context(ra, s, sk, n, frames_in_flight=2) as p:
        p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
        bufs = [torch.from_numpy(x).to(_dev()) for x in (poses_a, poses_b)]
        outs = [_Outs(n, j), _Outs(n, j)]
        frame = _frame(s)
        for k in range(8):  # A, B, A, B ... queued without waiting
            p.set_poses_device(bufs[k % 2].data_ptr(), n)
            p.run_skinned(frame, palette=outs[k % 2].palette.data_ptr(), async_=True, **outs[k % 2].pointers())
        p.wait()
        for k in range(2):
            _compare(outs[k].result(ra, f"in flight, buffer {k}"), wants[k], f"in flight, buffer {k}")


def test_misaligned_pointers_are_refused_before_anything_is_enqueued(ra, oracle_mod):
    """The palette leaves in 16-byte stores, device poses arrive in 8-byte loads (include/mi_instance_pipeline.h): a pointer
    that is not so aligned is MIP_ERR_INVALID_ARGUMENT — no kernel ever runs on it — and the context stays usable."""
    import torch

    j = 3
    sk, poses = sc.family_case("star", j)
    n = sc.ipw_ipb(j)[1] + 1
    s = sc.instances(n)
    poses = np.ascontiguousarray(poses[:n])
    want = _want(oracle_mod, s, sk, poses)
    with _context(ra, s, sk, n) as p:
        p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
        p.set_poses(poses)
        outs = _Outs(n, j)
        for off in (4, 8, 12):
            with pytest.raises(ra.MipError) as e:
                p.run_skinned(_frame(s), palette=outs.palette.data_ptr() + off, **outs.pointers())
            assert e.value.code == -1 and "16-byte" in str(e.value)
        dposes = torch.from_numpy(np.concatenate([poses.reshape(-1), np.zeros(2, np.float32)])).to(_dev())
        torch.cuda.synchronize()
        with pytest.raises(ra.MipError) as e:
            p.set_poses_device(dposes.data_ptr() + 4, n)
        assert e.value.code == -1 and "8-byte" in str(e.value)
        p.wait()
        for buf in (outs.palette, outs.model, outs.aabb, outs.cmds, outs.bitmap, outs.scal):   # nothing ran
            assert (buf.cpu().numpy().view(np.uint32) == SENTINEL).all()
        # the refused calls changed nothing: the host poses set before them are still the resident ones
        p.run_skinned(_frame(s), palette=outs.palette.data_ptr(), **outs.pointers())
        p.wait()
        _compare(outs.result(ra, "after the refusals"), want, "after the refusals")
        p.set_poses_device(dposes.data_ptr() + 8, n)   # 8-byte aligned, not 16: legal
        dposes[2:] = torch.from_numpy(poses.reshape(-1)).to(_dev())
        torch.cuda.synchronize()
        outs = _Outs(n, j)
        p.run_skinned(_frame(s), palette=outs.palette.data_ptr(), **outs.pointers())
        p.wait()
        _compare(outs.result(ra, "poses at an 8-byte offset"), want, "poses at an 8-byte offset")
