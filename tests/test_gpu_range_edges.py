"""The designed streams of tests/range_edge_cases.py through mip_run with culled_index_buffer: the range kernel (and the range
body inside the large-frame stage kernel) and the size-class sort in front of the wave-per-command body, with the grid pinned to
one workgroup (MIP_TUNE_TRI_RANGE_BLOCKS=1: four waves) so that a few thousand triangles reach every cut edge — both dealing
modes, every S from 256 to 8 192, look-backs over more than two groups of 64 ranges, full mask buffers, every batch size of the
sort. Commands, draw_count, draw_index_total and the WHOLE sentinel-filled index buffer go against the hand-written expectation
(which tests/test_range_edge_cases.py ties to the oracle and to the model of the decomposition) and against the oracle run here;
every case runs two frames. One context serves all cases of a tuning."""
import os
import subprocess
import sys

import numpy as np
import pytest

import range_edge_cases as rc
import range_model as rm

pytestmark = pytest.mark.gpu
GUARD = 64   # (Case.words allocates this many sentinel words behind the capacity)


@pytest.fixture(scope="module")
def ra():
    import renderer_amd

    renderer_amd.load_library()
    return renderer_amd


_BUILT = {}


def built(ra):
    """(mesh table, cases, meshes, vertices, indices) — the geometry is built once."""
    if not _BUILT:
        table, cases = rc.catalogue()
        _BUILT["v"] = (table, cases) + table.build(ra)
    return _BUILT["v"]


_ORACLE = {}


def oracle_frame(ra, oracle_mod, case):
    """The oracle's final commands and stream of a case that it can express (a buffer from word 0 that fits), computed once per stream."""
    if case.status != 0 or case.words()[0] != 0:
        return None
    key = (case.mesh_ids.tobytes(), case.base)
    if key not in _ORACLE:
        _, _, meshes, vertices, indices = built(ra)
        s = rc.scene_of(ra, meshes, case.mesh_ids)
        r = oracle_mod.run(s["pos"], s["rot"], s["scale"], s["mesh_id"], meshes, s["planes"], s["cam_pos"], first_index_base=case.base, threads=4)
        cmds, out, _ = oracle_mod.cull_all_triangles(r, s["pos"], s["mesh_id"], meshes, s["cam_pos"], ra.scene.default_pv(), vertices, indices,
                                                     out_capacity=case.words()[1])
        _ORACLE[key] = (r["draw_index_total"], cmds, out)
    return _ORACLE[key]


class Context:
    """One context under a tuning (the variables are read by mip_create), with outputs the test owns."""

    def __init__(self, ra, tuning, names, frames_in_flight=1):
        import torch

        self.ra, self.torch = ra, torch
        _, cases, meshes, vertices, indices = built(ra)
        self.cases = [cases[n] for n in names]
        n = max(len(c.mesh_ids) for c in self.cases)
        words = max(c.words()[1] for c in self.cases)
        saved = {k: os.environ.get(k) for k in rc.TUNING_VARIABLES}
        try:
            for k in rc.TUNING_VARIABLES:
                os.environ.pop(k, None)
            os.environ.update(rc.TUNINGS[tuning])
            self.p = ra.InstancePipeline(max_instances=n, max_meshes=len(meshes), frames_in_flight=frames_in_flight)
        finally:
            for k, v in saved.items():
                os.environ.pop(k, None)
                if v is not None:
                    os.environ[k] = v
        self.meshes = meshes
        self.p.set_mesh_table(meshes)
        self.p.set_geometry(vertices, indices)
        dev = torch.device("cuda", 0)
        self.bufs = [dict(model=torch.zeros((n, 16), dtype=torch.float32, device=dev), cmds=torch.zeros((n, 5), dtype=torch.int32, device=dev),
                          scal=torch.zeros(8, dtype=torch.int32, device=dev), out=torch.full((words,), -1, dtype=torch.int32, device=dev))
                     for _ in range(frames_in_flight)]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.p.close()

    def run(self, case, slot=0):
        """One synchronous frame of the case into sentinel-filled buffers: (status, commands, count, total, the allocated words)."""
        from renderer_amd.pipeline import make_frame

        s = rc.scene_of(self.ra, self.meshes, case.mesh_ids)
        self.p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
        b = self.bufs[slot]
        b["out"].fill_(-1)
        b["cmds"].fill_(0x5A5A5A5A)
        b["scal"].fill_(0x5A5A5A5A)
        self.torch.cuda.synchronize()
        lo, words = case.words()
        assert words <= b["out"].numel() and lo * 4 < b["out"].data_ptr()
        frame = make_frame(s["planes"], s["cam_pos"], first_index_base=case.base, pv=self.ra.scene.default_pv())
        status = 0
        try:
            # (a first_index_base that no buffer reaches from word 0: the buffer's word `lo` is the allocation's first)
            self.p.run_device(frame, model=b["model"].data_ptr(), draw_cmds=b["cmds"].data_ptr(), draw_count=b["scal"].data_ptr(),
                              draw_index_total=b["scal"].data_ptr() + 4, culled_index_buffer=b["out"].data_ptr() - 4 * lo,
                              culled_index_capacity=case.capacity)
        except self.ra.MipError as e:
            status = e.code
        count, total = (int(x) & 0xFFFFFFFF for x in b["scal"][:2].cpu().tolist())
        assert count <= len(case.mesh_ids)
        cmds = b["cmds"][:count].cpu().numpy().view(np.uint32).reshape(-1).view(self.ra.DRAW_CMD_DTYPE)
        return status, cmds, count, total, b["out"].cpu().numpy().view(np.uint32)


def check(ra, oracle_mod, case, got, what):
    status, cmds, count, total, out = got
    _, hand = case.expected()
    want_cmds = case.expected_cmds(ra)
    assert status == case.status, (what, status)
    assert count == len(want_cmds) and total == case.stream.index_total, (what, count, len(want_cmds), total, case.stream.index_total)
    assert cmds.tobytes() == want_cmds.tobytes(), (what, "commands", np.nonzero(cmds["indexCount"] != want_cmds["indexCount"])[0][:8].tolist())
    wrong = np.nonzero(out[: len(hand)] != hand)[0]
    assert len(wrong) == 0, (what, "stream", len(wrong), wrong[:4].tolist(), out[wrong[:4]].tolist(), hand[wrong[:4]].tolist())
    assert (out[len(hand):] == rm.SENTINEL).all(), (what, "words behind the frame's allocation were written")
    if case.status:   # no word at or behind the capacity
        assert (out[case.capacity - case.words()[0]:] == rm.SENTINEL).all(), what
    o = oracle_frame(ra, oracle_mod, case) if oracle_mod is not None else None
    if o is not None:
        assert total == o[0] and cmds.tobytes() == o[1].tobytes() and np.array_equal(out[: len(o[2])], o[2]), (what, "oracle")


def run_cases(ra, oracle_mod, tuning, names, frames=2, frames_in_flight=1):
    """The named cases in order on one context; returns its timings."""
    with Context(ra, tuning, names, frames_in_flight) as ctx:
        turn = 0
        for case in ctx.cases:
            for rep in range(frames):
                check(ra, oracle_mod, case, ctx.run(case, slot=turn % frames_in_flight), (tuning, case.name, rep))
                turn += 1
        return ctx.p.timings()


@pytest.mark.parametrize("tuning", ["ranges_256", "ranges_8192", "stage_ranges_256"])
def test_range_cases(ra, oracle_mod, tuning):
    """Every designed stream of the tuning, two frames each, on one context: the range kernel with S = 256 (both dealing modes),
    with S between the limits and at 8 192, and the range body inside mip_triangle_stage_kernel on the S = 256 streams."""
    names = [c.name for c in rc.cases_of(tuning)]
    assert len(names) >= 3
    run_cases(ra, oracle_mod, tuning, names)


def test_sorted_cases(ra, oracle_mod):
    """The size-class sort and the tickets of the wave-per-command body: powers of two and their neighbours, one class, every class,
    class populations around every batch size, more than 2 048 commands (a histogram copy serves two workgroups)."""
    run_cases(ra, oracle_mod, "sorted", [c.name for c in rc.cases_of("sorted")])


@pytest.mark.parametrize("k", range(len(rc.SEQUENCES)))
def test_sequences_on_one_context(ra, oracle_mod, k):
    """Streams of different lengths back to back on one frame slot (A, B, A ...: a granule, a range-map entry or a sort word of
    the previous frame must not be taken), then one frame each on a context of two slots, where the slots alternate."""
    tuning, names = rc.SEQUENCES[k]
    run_cases(ra, oracle_mod, tuning, names, frames=1)
    a, b = names[0], names[1]
    run_cases(ra, oracle_mod, tuning, [a, b, b, a, a, b, a], frames=1, frames_in_flight=2)


def child(fault):
    """In a child process under the diagnostic library: ranges dealt from the last one down ("reverse"), or every 16th range
    never publishing ("skip": the look-backs count those ranges themselves, in the nearest and in a later group of 64)."""
    import renderer_amd

    renderer_amd.load_library()
    helps = 0
    t = run_cases(renderer_amd, None, "ranges_256", rc.LONG_LOOKBACK)
    helps += t["prefix_helps"]
    for tuning, names in rc.SEQUENCES[:2]:
        t = run_cases(renderer_amd, None, tuning, names, frames=1)
        helps += t["prefix_helps"] if fault == "skip" else 0
        if fault == "skip":
            assert t["prefix_helps"] > 0, (tuning, t)
    if fault == "skip":
        assert helps > 0
    print("RANGE EDGES OK", fault, helps)


@pytest.mark.parametrize("fault", ["reverse", "skip"])
def test_long_look_backs_do_not_depend_on_who_runs_when(fault):
    """The cases whose look-back spans one group of 64 ranges or more, and the sequences, under the diagnostic library with the
    ranges dealt in reverse and with silent ranges (the switches of test_parts_kernel_does_not_depend_on_who_runs_when): the
    frames are still the hand-written ones, and under "skip" MipTimings.prefix_helps says ranges were counted by their successors."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r'''
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
os.environ["MIP_LIBRARY"] = os.path.join(sys.argv[1], "renderer_amd", "lib", "libmi_instance_pipeline_dbg.so")
if sys.argv[2] == "reverse":
    os.environ["MIP_DEBUG_TILE_ORDER"] = "reverse"
else:
    os.environ["MIP_DEBUG_SKIP_PART"] = "3"
import test_gpu_range_edges
test_gpu_range_edges.child(sys.argv[2])
'''
    out = subprocess.run([sys.executable, "-c", code, root, fault], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "RANGE EDGES OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
