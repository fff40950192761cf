"""The visible-cluster list in two phases on the GPU (include/mi_instance_pipeline.h, mip_list_clusters_phase): every byte of both
phases' entries, counts, draw arguments and stats and of the record against the hand-written lists
(tests/cluster_list_phase_cases.py), against the numpy restatement (tests/cluster_list_phase_restatement.py) over config 3 under
three new pyramids, and on the same context against mip_cull_clusters_phase (its commands expanded, its record byte for byte,
each call's SECOND over the other's record) and mip_list_clusters; the structural edges of the launch plan
(renderer_amd/csrc/cluster_list_phase_plan.hpp), also with reversed and scrambled tiles under the diagnostic library; the base
arithmetic through the capacity and through the base, the overflow and not-its-record contracts, every refusal, and the frame
with two frames in flight and no host wait. Every buffer — the entries in front of the base and behind the count, the record
and its guard words, the scalar words — is filled with a sentinel and compared whole. Not reference behaviour: parity is with
the restatement."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_list_phase_cases as lpc
import cluster_list_phase_restatement as lp
import cluster_list_restatement as clr
import cluster_phase_cases as pc
import cluster_phase_restatement as pr
import cluster_restatement as cr
import lod_restatement as lr
import numpy_restatement as nr
import occlusion_restatement as orr
import test_gpu_batch as T
import test_gpu_batch_lods as TL
import test_gpu_cluster_list as TLST
import test_gpu_cluster_phases as TP
import test_gpu_clusters as TC
import test_gpu_occlusion as TO
from renderer_amd import _lib
from renderer_amd.pipeline import (CLUSTER_ENTRY_DTYPE, DRAW_CMD_DTYPE, make_cluster_phase_list_outputs, make_frame, make_lod_policy,
                                   make_occlusion)

pytestmark = pytest.mark.gpu
ROOT = TC.ROOT
SENTINEL = T.SENTINEL
ra = T.ra   # the module's library fixture
NOT_READY, INVALID, CAPACITY, DEVICE = -6, -1, -4, -5
BOTH = (False, True)
BLOCK = 12   # scalar words per call: [0] entry_count, [2:6] draw_args, [6:10] stats, [10] a word for the base; [1], [11] nobody's
GUARD = 3    # sentinel entries behind the buffer's capacity


class _Buf:
    """One entry buffer of `cap` entries (+ GUARD nobody may touch) and the scalar blocks of up to three calls into it, all
    filled with a sentinel."""

    def __init__(self, cap, calls=2):
        import torch

        fill = T._i32(SENTINEL)
        self.cap = int(cap)
        self.entries = torch.full((self.cap + GUARD, 4), fill, dtype=torch.int32, device=T._dev())
        self.scal = torch.full((BLOCK * calls,), fill, dtype=torch.int32, device=T._dev())
        self.word = {}          # call -> the value its base word was given
        torch.cuda.synchronize()

    def ptr(self, call, word):
        return self.scal.data_ptr() + 4 * (BLOCK * call + word)

    def set_word(self, call, value):
        import torch

        self.scal[BLOCK * call + 10] = T._i32(value)
        self.word[call] = int(value)
        torch.cuda.synchronize()

    def outputs(self, call, entry_capacity=None, entry_base=0, args=True, stats=True, work_capacity=0, async_=False):
        return make_cluster_phase_list_outputs(self.entries.data_ptr(), self.cap if entry_capacity is None else entry_capacity, self.ptr(call, 0),
                                               self.ptr(call, 2) if args else 0, self.ptr(call, 6) if stats else 0, work_capacity=work_capacity,
                                               async_=async_, entry_base=entry_base)

    def scalars(self):
        import torch

        torch.cuda.synchronize()
        return self.scal.cpu().numpy().view(np.uint32)

    def rows(self):
        import torch

        torch.cuda.synchronize()
        return self.entries.cpu().numpy().view(np.uint32)

    def check_call(self, call, count, b, stats, what, args=True, has_stats=True):
        """The call's block, whole: the count, {192, count, 0, b}, the four stats words, its base word as it was given."""
        blk = self.scalars()[BLOCK * call: BLOCK * (call + 1)]
        want = np.full(BLOCK, SENTINEL, np.uint32)
        want[0] = count
        if args:
            want[2:6] = [192, count, 0, b]
        if has_stats:
            want[6:10] = [int(v) for v in stats]
        if call in self.word:
            want[10] = self.word[call]
        assert blk.tolist() == want.tolist(), (what, "scalars", blk.tolist(), want.tolist())

    def check_entries(self, lists, what):
        """lists: [(b, entries written)] — everything else is still the sentinel: in front of a base, behind a count, the guard."""
        want = np.full((self.cap + GUARD, 4), SENTINEL, np.uint32)
        for b, entries in lists:
            if len(entries):
                want[b: b + len(entries)] = np.ascontiguousarray(entries).view(np.uint32).reshape(-1, 4)
        got = self.rows()
        if got.tobytes() != want.tobytes():
            bad = np.nonzero((got != want).any(axis=1))[0]
            raise AssertionError((what, "entries", "first differing row", int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist(), "rows", len(bad)))

    def untouched(self):
        want = np.full(len(self.scal), SENTINEL, np.uint32)
        for call, value in self.word.items():
            want[BLOCK * call + 10] = value
        return (self.rows() == SENTINEL).all() and self.scalars().tolist() == want.tolist()


def _call(p, frame, bitmap_ptr, policy, o, occ, rec, async_, expect=0, what=""):
    """One mip_list_clusters_phase call; its status, from the call or from mip_wait for an asynchronous one, reported once."""
    raised = 0
    try:
        p.list_clusters_phase(frame, bitmap_ptr, policy, o, occ, rec)
        if async_ and expect:
            p.wait()
    except Exception as e:   # MipError of the library under test (the product's or the diagnostic one's)
        raised = e.code
    assert raised == expect, (what, raised, expect)
    if expect:
        p.wait()              # reported once


def _stats4(want, phase):
    """{survivors, W, members, candidates} of a hand-written want (lists) or of a phase-command want (heads, survivors, W, members)."""
    st = [int(v) for v in want[phase]["stats"]]
    return st if "entries" in want[phase] else [st[1], st[2], st[3], int(want["record"][2])]


def _entries(want, phase):
    return want[phase]["entries"] if "entries" in want[phase] else clr.from_commands(want[phase]["cmds"], None)


def run_scene(ra, p, s, want, what, asyncs=BOTH, mode=lr.DISTANCE, switch_sq=pc.PIN, bases=("count", "word 0", "null"), subsets=((True, True),)):
    """FIRST under the scene's old pyramid at base NULL, SECOND under its new one and under planes that accept nothing, the
    pyramid builds and the calls with no wait in between. bases: "count" — SECOND appends behind FIRST through FIRST's own
    entry_count; "word 0" — both calls read a word holding 0, SECOND into a buffer of its own; "null" — entry_base NULL."""
    import torch

    bm = TC._device_bitmap(s["bitmap"])
    old, new = TP._Pyramid(ra, s["old_depth"], s["pv"]), TP._Pyramid(ra, want["new_depth"], s["pv"])
    torch.cuda.synchronize()
    policy = make_lod_policy(mode, switch_sq)
    f1 = make_frame(s["planes"], s["cam_pos"], first_instance_base=s["base"])
    f2 = make_frame(s.get("second_planes", s["planes"]), s["cam_pos"], first_instance_base=s["base"])
    e1, e2 = _entries(want, "first"), _entries(want, "second")
    st1, st2 = _stats4(want, "first"), _stats4(want, "second")
    n1, n2 = len(e1), len(e2)
    for async_ in asyncs:
        for base in bases:
            for args, stats in subsets:
                tag = f"{what} async={async_} base={base} args={args} stats={stats}"
                rec = TP._Record(st1[1])
                appended = base == "count"
                a = _Buf(n1 + n2 if appended else n1)
                z = a if appended else _Buf(n2)
                if base == "word 0":
                    a.set_word(0, 0)
                    z.set_word(1, 0)
                first_base = a.ptr(0, 10) if base == "word 0" else 0
                second_base = a.ptr(0, 0) if appended else z.ptr(1, 10) if base == "word 0" else 0
                _call(p, f1, bm.data_ptr(), policy, a.outputs(0, entry_base=first_base, args=args, stats=stats, async_=async_), old.build(ra, p), rec.arg("first"), async_)
                _call(p, f2, bm.data_ptr(), policy, z.outputs(1, entry_base=second_base, args=args, stats=stats, async_=async_), new.build(ra, p), rec.arg("second"), async_)
                p.wait()
                rec.check(want["record"], tag)
                b = n1 if appended else 0
                a.check_call(0, n1, 0, st1, tag + " FIRST", args, stats)
                z.check_call(1, n2, b, st2, tag + " SECOND", args, stats)
                if appended:
                    a.check_entries([(0, e1), (n1, e2)], tag)
                else:
                    a.check_entries([(0, e1)], tag + " FIRST")
                    z.check_entries([(0, e2)], tag + " SECOND")


# ---- 1. the hand-written scenes ----

_CASES = lpc.cases()


def run_hand_cases(ra, asyncs=BOTH, subsets=((True, True), (False, True), (True, False), (False, False))):
    for name, s, want in _CASES:
        with TC._pipeline(ra, s, s["vertices"], s["indices"]) as p:
            run_scene(ra, p, s, want, name, asyncs, subsets=subsets)


@pytest.mark.parametrize("name,s,want", _CASES, ids=[c[0] for c in _CASES])
def test_hand_cases(ra, name, s, want):
    with TC._pipeline(ra, s, s["vertices"], s["indices"]) as p:
        run_scene(ra, p, s, want, name)
        run_scene(ra, p, s, want, name, asyncs=(True,), bases=("count",), subsets=((False, True), (True, False), (False, False)))


# ---- 2. the restatement over config 3, and the other calls on the same context ----

def _commands(p, frame, bitmap_ptr, policy, occ, rec, room):
    """What mip_cull_clusters_phase writes on this context for the same arguments, expanded into entries; its stats."""
    out = TC._Out(room)
    p.cull_clusters_phase(frame, bitmap_ptr, policy, out.outputs(), occ, rec)
    rows, scal = out.result()
    return clr.from_commands(np.ascontiguousarray(rows[: int(scal[0])]).view(DRAW_CMD_DTYPE).reshape(-1), None), scal[2:6]


def run_config_3(ra, n, mode, asyncs=(True,)):
    """config 3 under the wall; SECOND under the same wall, a cleared image and the wall moved by a quarter of the width,
    appended behind FIRST in one buffer; then the same against mip_cull_clusters_phase and mip_list_clusters on the context."""
    ordering = "strips" if n == 257 else "rows" if n % 2 else "shuffled"
    s = TL._sized(ra.scene.make_scene(3, n=max(n, 1)), n)
    vertices, indices = ra.scene.make_geometry(s["meshes"], ordering)
    boxes = cr.cluster_boxes(s["meshes"], vertices, indices)
    bitmap = orr.bitmap_of(~nr.run(s)["coarse_culled"]) if n else np.zeros(0, np.uint32)
    pv = ra.scene.default_pv()
    occ_of = lambda depth: dict(pv=pv, levels=orr.pyramid_levels(depth), width=64, height=32)   # noqa: E731
    base = 0xFFFFFFFF - n // 2                        # wraps inside the scene
    sw = TL._metric_thresholds(s, mode) if mode == lr.RELATIVE else lr.PIN_SWITCH_SQ
    args = (s, boxes, bitmap, mode, sw, 1 << 30)
    f = lp.first(*args, occ_of(TP._wall(0)), first_instance_base=base)
    scene = dict(s, bitmap=bitmap, base=base, pv=pv, old_depth=TP._wall(0), second_planes=pc.SECOND_PLANES)
    survivors = []
    with TC._pipeline(ra, s, vertices, indices) as p:
        for column in (0, None, 16):
            g = lp.second(*args, occ_of(TP._wall(column)), f["record"], b=f["count"], first_instance_base=base)
            assert f["status"] == 0 and g["status"] == 0
            want = dict(first=f, second=g, record=f["record"], new_depth=TP._wall(column))
            run_scene(ra, p, scene, want, f"config 3 n={n} mode={mode} wall at {column}", asyncs, mode, sw, bases=("count",))
            survivors.append(int(g["stats"][0]))
            if n and column == 16:
                _against_the_other_calls(ra, p, scene, want, mode, sw)
    if n >= 257:
        assert survivors[0] == 0 < survivors[2] < survivors[1] == int(f["record"][2])


def _against_the_other_calls(ra, p, s, want, mode, sw):
    import torch

    bm = TC._device_bitmap(s["bitmap"])
    old, new = TP._Pyramid(ra, s["old_depth"], s["pv"]), TP._Pyramid(ra, want["new_depth"], s["pv"])
    torch.cuda.synchronize()
    occ_old, occ_new = old.build(ra, p), new.build(ra, p)
    p.wait()
    policy = make_lod_policy(mode, sw)
    frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=s["base"])
    f, g = want["first"], want["second"]
    n1, n2, w = f["count"], g["count"], int(f["stats"][1])
    # mip_cull_clusters_phase on this context: its commands expanded are the lists, its record is the list call's byte for byte
    rec_c = TP._Record(w)
    e1, s1 = _commands(p, frame, bm.data_ptr(), policy, occ_old, rec_c.arg("first"), n1 + 1)
    e2, s2 = _commands(p, frame, bm.data_ptr(), policy, occ_new, rec_c.arg("second"), n2 + 1)
    assert e1.tobytes() == f["entries"].tobytes() and e2.tobytes() == g["entries"].tobytes(), "the command call's expansion"
    assert s1[1:].tolist() == f["stats"][:3].tolist() and s2[1:].tolist() == g["stats"][:3].tolist()
    rec_c.check(want["record"], "mip_cull_clusters_phase's record")
    rec_l = TP._Record(w)
    a = _Buf(n1 + n2)
    _call(p, frame, bm.data_ptr(), policy, a.outputs(0), occ_old, rec_l.arg("first"), False)
    assert rec_l.words().tobytes() == rec_c.words().tobytes(), "the two calls' records"
    # mip_list_clusters under the old pyramid writes FIRST's entries
    plain = TLST._Out(n1)
    p.list_clusters(frame, bm.data_ptr(), policy, plain.outputs(), occlusion=occ_old)
    TLST._check(plain, f["entries"], f["stats"][:3], "mip_list_clusters under the old pyramid")
    # cross-acceptance: this call's SECOND over the command call's record, appended; the command call's SECOND over this call's
    _call(p, frame, bm.data_ptr(), policy, a.outputs(1, entry_base=a.ptr(0, 0)), occ_new, rec_c.arg("second"), False)
    a.check_call(0, n1, 0, f["stats"], "FIRST")
    a.check_call(1, n2, n1, g["stats"], "SECOND over mip_cull_clusters_phase's record")
    a.check_entries([(0, f["entries"]), (n1, g["entries"])], "SECOND over mip_cull_clusters_phase's record")
    e2, s2 = _commands(p, frame, bm.data_ptr(), policy, occ_new, rec_l.arg("second"), n2 + 1)
    assert e2.tobytes() == g["entries"].tobytes() and s2[1:].tolist() == g["stats"][:3].tolist(), "mip_cull_clusters_phase SECOND over this call's record"
    rec_l.check(want["record"], "the record behind both SECOND calls")


@pytest.mark.parametrize("mode", [lr.DISTANCE, lr.RELATIVE], ids=["distance", "relative"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 4097])
def test_restatement_over_config_3(ra, n, mode):
    run_config_3(ra, n, mode)


# ---- 3. sizes read from the plans ----

def _plan_sizes(tmp):
    exe = os.path.join(str(tmp), "cluster_list_phase_plan_sizes")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "native", "cluster_list_phase_plan_check.cpp"), "-o", exe])
    return json.loads(subprocess.check_output([exe, "sizes"]))


EDGE_PARTS = ("W edges", "members")


def _edge_scenes(sizes, part):
    """[(name, scene, want)] — want as cluster_phase_cases.ladder_scene writes it down from the letters. "W edges": W one below,
    at and one above a word, the item tile and the list tile, every item a candidate and alternating candidate words; three item
    tiles of which only the last holds candidates; lone SECOND survivors on each side of a list-tile edge. "members": members
    whose first item is at 64 k - 1 / 64 k / 64 k + 1 (the search-free locate's edge), C = 1, 64, 65 and 129, 64 one-cluster
    members in a word."""
    item, tile = sizes["item_tile"], sizes["list_tile"]
    out = []
    if part == "W edges":
        for edge in (64, item, tile):
            for w in (edge - 1, edge, edge + 1):
                out.append((f"W={w}, every item a candidate", *pc.filled(w, lambda j, k: "H" * k, base=1)))
                out.append((f"W={w}, alternating candidate words", *pc.filled(w, lambda j, k: ("H" if j % 2 == 0 else "V") * k, base=2)))
        per = item // 64
        out.append(("candidates in the last of three item tiles", *pc.filled(3 * item, lambda j, k: ("H" if j >= 2 * per else "V") * k, base=3)))
        at = tile // 64   # the instance that starts the second list tile
        lone = lambda j, k: "V" * 63 + "H" if j == at - 1 else "H" + "V" * 63 if j == at else "V" * k   # noqa: E731
        out.append(("lone SECOND survivors on each side of a list-tile edge", *pc.filled(2 * tile, lone, base=4)))
        return out
    alt = lambda k, first="H": (("HV" if first == "H" else "VH") * k)[:k]   # noqa: E731
    ladders = [alt(63), alt(1), alt(64), alt(65), alt(62, "V"), alt(3), alt(129, "V")]
    out.append(("first items around word edges", *pc.ladder_scene(ladders, [0, 1, 2, 3, 4, 5, 5, 6, 6, 3, 2, 6, 1, 0, 1], base=1)))
    out.append(("first items around word edges, every item a candidate", *pc.ladder_scene(["H" * 63, "H", "H" * 64, "H" * 65, "H" * 62, "HHH", "H" * 129],
                                                                                        [0, 1, 2, 3, 4, 5, 5, 6, 6, 3, 2, 6], base=1)))
    out.append(("64 one-cluster members in a word", *pc.ladder_scene(["H", "V"], [0, 1, 1, 0, 0] * 40, base=3)))
    out.append(("C = 129 over words and item tiles", *pc.ladder_scene(["V" + "H" * 127 + "V"], [0] * 40, base=5, last=9)))
    return out


def run_edge_scenes(ra, sizes, part):
    for name, s, want in _edge_scenes(sizes, part):
        assert int(want["first"]["stats"][2]) == len(pr.unpack_record(want["record"], int(want["record"][0])))
        with TC._pipeline(ra, s, s["vertices"], s["indices"]) as p:
            run_scene(ra, p, s, want, name, asyncs=(True,), bases=("count",))


@pytest.mark.parametrize("part", EDGE_PARTS)
def test_sizes_read_from_the_plans(ra, tmp_path, part):
    sizes = _plan_sizes(tmp_path)
    scenes = _edge_scenes(sizes, part)
    if part == "W edges":
        for edge in (64, sizes["item_tile"], sizes["list_tile"]):
            assert {int(w["record"][0]) for _, _, w in scenes} >= {edge - 1, edge, edge + 1}
        lone = scenes[-1][2]
        bits = np.nonzero(pr.unpack_record(lone["record"], int(lone["record"][0])))[0]
        assert bits.tolist() == [sizes["list_tile"] - 1, sizes["list_tile"]]
    else:
        firsts = np.cumsum([0] + [len(l) for l in (63 * "x", "x", 64 * "x", 65 * "x")])
        assert {int(v) % 64 for v in firsts} >= {0, 63, 1}   # 0, 63, 64, 128, 193: on, one before and one behind a word edge
    run_edge_scenes(ra, sizes, part)


# ---- 4. all of it in any dispatch order, under the diagnostic library ----

_CHILD = r'''
import os, sys
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
os.environ["MIP_LIBRARY"] = os.path.join(root, "renderer_amd", "lib", "libmi_instance_pipeline_dbg.so")
import renderer_amd
import lod_restatement as lr
import test_gpu_cluster_list_phases as TLP
renderer_amd.load_library()
if sys.argv[3] == "hand":
    TLP.run_hand_cases(renderer_amd, asyncs=(True,), subsets=((True, True),))
elif sys.argv[3] == "config 3":
    for n in (0, 1, 63, 64, 65, 257, 4097):
        TLP.run_config_3(renderer_amd, n, lr.DISTANCE)
else:
    TLP.run_edge_scenes(renderer_amd, TLP._plan_sizes(sys.argv[2]), sys.argv[3])
print("CLUSTER-LIST-PHASES-OK")
'''


@pytest.mark.parametrize("which", ("hand", "config 3") + EDGE_PARTS)
@pytest.mark.parametrize("tiles", ["reverse", "scramble"])
def test_in_any_dispatch_order(tiles, which, tmp_path):
    e = dict(os.environ, MIP_DEBUG_TILE_ORDER=tiles)
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(tmp_path), which], capture_output=True, text=True, timeout=600, env=e)
    assert out.returncode == 0 and "CLUSTER-LIST-PHASES-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ---- 5. contracts (the release library only) ----

@pytest.mark.parametrize("frames_in_flight", [1, 2])
def test_overflows_bases_and_a_record_that_is_not_the_calls(ra, frames_in_flight):
    import torch
    import test_cluster_phase_restatement as CPU

    s, vertices, indices, boxes, bitmap, pv, occ_of = TP._contract_scene(ra)
    args = (s, boxes, bitmap, lr.DISTANCE, lr.PIN_SWITCH_SQ)
    old_o, clear_o = occ_of(TP._wall(0)), occ_of(TP._wall(None))
    f = lp.first(*args, 1 << 30, old_o, first_instance_base=17)
    g = lp.second(*args, 1 << 30, clear_o, f["record"], first_instance_base=17)
    n1, n2, w, members, candidates = f["count"], g["count"], int(f["stats"][1]), int(f["stats"][2]), int(f["stats"][3])
    assert n1 > 2 and n2 > 2
    fewer = orr.bits_of(bitmap, 257).copy()
    fewer[int(f["items"]["inst"][0])] = False
    other_w = orr.bitmap_of(fewer)
    other_members = CPU.same_w_other_members(s, boxes, bitmap)
    policy = make_lod_policy(lr.DISTANCE, lr.PIN_SWITCH_SQ)
    frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=17)
    with TC._pipeline(ra, s, vertices, indices, frames_in_flight=frames_in_flight) as p:
        old, clear = TP._Pyramid(ra, TP._wall(0), pv), TP._Pyramid(ra, TP._wall(None), pv)
        bm, bm_w, bm_m = TC._device_bitmap(bitmap), TC._device_bitmap(other_w), TC._device_bitmap(other_members)
        fr = T._Frame(257)
        torch.cuda.synchronize()
        occ_old, occ_new = old.build(ra, p), clear.build(ra, p)
        p.wait()

        def turn():
            if frames_in_flight > 1:       # behind a frame of its own: consecutive calls go to different slots
                p.run_device(frame, async_=True, **fr.kwargs())

        for async_ in BOTH:
            tag = f"async={async_}"
            # FIRST: a record one word short is a work overflow — zeros, {192, 0, 0, b}, the refusal's header; exact room runs
            rec = TP._Record(w)
            a = _Buf(n1 + n2)
            a.set_word(0, 5)
            turn()
            _call(p, frame, bm.data_ptr(), policy, a.outputs(0, entry_base=a.ptr(0, 10), async_=async_), occ_old, rec.arg("first", rec.bytes - 8), async_, CAPACITY, tag)
            a.check_call(0, 0, 5, [0, w, members, 0], "a record one word short " + tag)
            a.check_entries([], "a record one word short " + tag)
            rec.check([0xFFFFFFFF, 0, 0, 0], "a record one word short")
            a = _Buf(n1 + n2)
            turn()
            _call(p, frame, bm.data_ptr(), policy, a.outputs(0, async_=async_), occ_old, rec.arg("first"), async_, 0, tag)
            p.wait()
            a.check_call(0, n1, 0, f["stats"], "a record of exactly W " + tag)
            rec.check(f["record"], "a record of exactly W")
            # FIRST: an entry overflow, through the capacity and through the base, leaves the record whole
            for cap, b in ((n1 - 1, 0), (n1 + 3, 4), (0, 0), (n1, n1), (n1, n1 + 1), (n1, 0xFFFFFFFF)):
                rec2 = TP._Record(w)
                c = _Buf(max(cap, 1))
                c.set_word(0, b)
                room = lp.room_of(b, cap)
                turn()
                _call(p, frame, bm.data_ptr(), policy, c.outputs(0, entry_capacity=cap, entry_base=c.ptr(0, 10), async_=async_), occ_old, rec2.arg("first"), async_,
                      CAPACITY, f"FIRST cut cap={cap} b={b} {tag}")
                c.check_call(0, room, b, f["stats"], f"FIRST cut cap={cap} b={b} {tag}")
                c.check_entries([(b, f["entries"][:room])] if room else [], f"FIRST cut cap={cap} b={b} {tag}")
                rec2.check(f["record"], "the record of a FIRST call whose entries overflowed")
            # SECOND appended behind FIRST: room = survivors - 1 and 0 through the capacity; then b >= capacity
            for cap in (n1 + n2 - 1, n1):
                z = _Buf(cap)
                rec3 = TP._Record(w)
                turn()
                _call(p, frame, bm.data_ptr(), policy, z.outputs(0, async_=async_), occ_old, rec3.arg("first"), async_, 0, tag)
                turn()
                _call(p, frame, bm.data_ptr(), policy, z.outputs(1, entry_base=z.ptr(0, 0), async_=async_), occ_new, rec3.arg("second"), async_, CAPACITY,
                      f"SECOND cut cap={cap} {tag}")
                z.check_call(0, n1, 0, f["stats"], f"FIRST in front of a cut SECOND {tag}")
                z.check_call(1, cap - n1, n1, g["stats"], f"SECOND cut cap={cap} {tag}")
                z.check_entries([(0, f["entries"]), (n1, g["entries"][: cap - n1])], f"SECOND cut cap={cap} {tag}")
            # SECOND with another bitmap: another W; the same W and another member count — MIP_ERR_DEVICE, reported once
            for what, other, bits in (("another W", bm_w, other_w), ("another member count", bm_m, other_members)):
                items = cr.work_items(s["pos"], s["scale"], s["mesh_id"], s["meshes"], s["cam_pos"], bits, lr.DISTANCE, lr.PIN_SWITCH_SQ)
                assert (items["W"] != w) == (what == "another W") and items["members"] != members
                z = _Buf(n2)
                z.set_word(1, 2)
                turn()
                _call(p, frame, other.data_ptr(), policy, z.outputs(1, entry_base=z.ptr(1, 10), async_=async_), occ_new, rec.arg("second"), async_, DEVICE, f"{what} {tag}")
                z.check_call(1, 0, 2, [0, items["W"], items["members"], 0], f"SECOND, {what} {tag}")
                z.check_entries([], f"SECOND, {what} {tag}")
            # then a fitting call: complete, and the record is as FIRST left it
            z = _Buf(n2 + 2)
            z.set_word(1, 2)
            turn()
            _call(p, frame, bm.data_ptr(), policy, z.outputs(1, entry_base=z.ptr(1, 10), async_=async_), occ_new, rec.arg("second"), async_, 0, tag)
            p.wait()
            z.check_call(1, n2, 2, g["stats"], "a fitting SECOND call " + tag)
            z.check_entries([(2, g["entries"])], "a fitting SECOND call " + tag)
            rec.check(f["record"], "the record behind every SECOND call")
        # mip_list_clusters and mip_cull_clusters_phase behind these calls on the same slot return their usual bytes
        plain = clr.list_clusters(*args, 1 << 30, first_instance_base=17, occlusion=old_o)
        out = TLST._Out(len(plain["entries"]))
        p.list_clusters(frame, bm.data_ptr(), policy, out.outputs(), occlusion=occ_old)
        TLST._check(out, plain["entries"], plain["stats"], "mip_list_clusters behind the phase calls")
        assert plain["entries"].tobytes() == f["entries"].tobytes()
        pf = pr.first(*args, 1 << 30, old_o, first_instance_base=17)
        rec4 = TP._Record(w)
        TP._phase(p, frame, bm.data_ptr(), policy, occ_old, rec4.arg("first"), pf, "mip_cull_clusters_phase behind the phase list calls")
        rec4.check(f["record"], "mip_cull_clusters_phase behind the phase list calls")


def test_refusals_write_nothing(ra):
    import torch

    name, s, want = _CASES[0]
    with TC._pipeline(ra, s, s["vertices"], s["indices"]) as p:
        lib, ctx = p._lib, p._ctx
        bm = TC._device_bitmap(s["bitmap"])
        out, rec = _Buf(4), TP._Record(3)
        frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=s["base"])
        policy = make_lod_policy(lr.DISTANCE, pc.PIN)
        pyr = torch.zeros(64, dtype=torch.float32, device=T._dev())
        torch.cuda.synchronize()
        good_occ = make_occlusion(8, 8, pyr.data_ptr(), s["pv"])

        def call(frame=frame, bitmap=bm.data_ptr(), policy=policy, occ=good_occ, o=None, r=None, null_out=False, null_rec=False):
            o = o if o is not None else out.outputs(0)
            r = r if r is not None else rec.arg("first")
            return lib.mip_list_clusters_phase(ctx, C.addressof(frame) if frame is not None else None, bitmap, C.addressof(policy) if policy is not None else None,
                                               C.addressof(occ) if occ is not None else None, None if null_out else C.addressof(o),
                                               None if null_rec else C.addressof(r))

        def changed(make, **kw):
            x = make()
            for k, v in kw.items():
                setattr(x, k, v)
            return x

        outputs = lambda **kw: changed(lambda: out.outputs(0), **kw)   # noqa: E731
        record = lambda **kw: changed(lambda: rec.arg("first"), **kw)   # noqa: E731
        occlusion = lambda **kw: changed(lambda: make_occlusion(8, 8, pyr.data_ptr(), s["pv"]), **kw)   # noqa: E731
        bad_policy = make_lod_policy(lr.DISTANCE, pc.PIN)
        bad_policy.switch_sq[1] = 1.0           # decreases
        refused = [
            # everything mip_list_clusters (cone NULL) refuses
            ("NULL frame", call(frame=None)), ("NULL bitmap", call(bitmap=None)), ("NULL policy", call(policy=None)), ("NULL out", call(null_out=True)),
            ("NULL cluster_entries", call(o=outputs(cluster_entries=None))), ("NULL entry_count", call(o=outputs(entry_count=None))),
            ("struct_size", call(o=outputs(struct_size=48))), ("unknown flags", call(o=outputs(flags=_lib.MIP_OUT_DEVICE | 0x10))),
            ("host outputs", call(o=outputs(flags=0))), ("misaligned count", call(o=outputs(entry_count=out.ptr(0, 0) + 2))),
            ("misaligned args", call(o=outputs(draw_args=out.ptr(0, 2) + 1))), ("misaligned stats", call(o=outputs(stats=out.ptr(0, 6) + 1))),
            ("entries 4 bytes off", call(o=outputs(cluster_entries=out.entries.data_ptr() + 4))),
            ("entries 8 bytes off", call(o=outputs(cluster_entries=out.entries.data_ptr() + 8))),
            ("decreasing thresholds", call(policy=bad_policy)),
            ("occlusion struct_size", call(occ=occlusion(struct_size=100))), ("occlusion flags", call(occ=occlusion(flags=1))),
            ("candidates", call(occ=occlusion(candidates=bm.data_ptr()))), ("occluded_bitmap", call(occ=occlusion(occluded_bitmap=bm.data_ptr()))),
            ("NULL pyramid", call(occ=occlusion(pyramid=None))), ("extent", call(occ=occlusion(width=0))),
            # everything mip_cull_clusters_phase refuses about the record
            ("NULL rec", call(null_rec=True)), ("NULL record", call(r=record(record=None))), ("misaligned record", call(r=record(record=rec.buf.data_ptr() + 8))),
            ("record_bytes 15", call(r=record(record_bytes=15))), ("record_bytes 0", call(r=record(record_bytes=0))),
            ("phase 0", call(r=record(phase=0))), ("phase 3", call(r=record(phase=3))), ("record struct_size", call(r=record(struct_size=16))),
            ("NULL occ", call(occ=None)), ("NULL occ, SECOND", call(occ=None, r=record(phase=2))),
            # and the base's own
            ("entry_base misaligned", call(o=outputs(entry_base=out.ptr(0, 10) + 2))), ("entry_base is entry_count", call(o=outputs(entry_base=out.ptr(0, 0)))),
            ("entry_base is draw_args[0]", call(o=outputs(entry_base=out.ptr(0, 2)))), ("entry_base is draw_args[3]", call(o=outputs(entry_base=out.ptr(0, 5)))),
            ("entry_base is stats[0]", call(o=outputs(entry_base=out.ptr(0, 6)))), ("entry_base is stats[3]", call(o=outputs(entry_base=out.ptr(0, 9)))),
        ]
        for what, rc in refused:
            assert rc == INVALID, (what, rc)
        assert lib.mip_list_clusters_phase(None, C.addressof(frame), bm.data_ptr(), C.addressof(policy), C.addressof(good_occ), None, None) == INVALID
        assert out.untouched() and (rec.words() == SENTINEL).all()
        run_scene(ra, p, s, want, name + " after the refusals", bases=("count",))       # the context is usable
        # the three not-ready states: a stale cluster table after new geometry, after a new mesh table; no instances
        p.set_geometry(s["vertices"], s["indices"])
        assert call() == NOT_READY
        p.build_clusters()
        p.set_mesh_table(s["meshes"])
        assert call() == NOT_READY and out.untouched() and (rec.words() == SENTINEL).all()
        p.build_clusters()
        run_scene(ra, p, s, want, name + " after the rebuild", asyncs=(True,), bases=("count",))
    with ra.InstancePipeline(max_instances=4, max_meshes=len(s["meshes"])) as p:
        p.set_mesh_table(s["meshes"])
        p.set_geometry(s["vertices"], s["indices"])
        p.build_clusters()
        fresh, rec = _Buf(4), TP._Record(3)
        with pytest.raises(ra.MipError) as e:
            p.list_clusters_phase(frame, bm.data_ptr(), policy, fresh.outputs(0), good_occ, rec.arg("first"))
        assert e.value.code == NOT_READY and fresh.untouched() and (rec.words() == SENTINEL).all()


# ---- 6. the frame ----

def test_the_frame_with_two_frames_in_flight_and_no_host_wait(ra):
    """FIRST, mip_build_depth_pyramid, mip_run_occluded (the slot advances), SECOND with entry_base = FIRST's entry_count — the
    SECOND call runs on another stream than the FIRST call that writes its record and its base, and nothing waits on the host."""
    import torch

    s, vertices, indices, boxes, bitmap, pv, occ_of = TP._contract_scene(ra)
    args = (s, boxes, bitmap, lr.DISTANCE, lr.PIN_SWITCH_SQ, 1 << 30)
    f = lp.first(*args, occ_of(TP._wall(0)), first_instance_base=5)
    g = lp.second(*args, occ_of(TP._wall(16)), f["record"], b=f["count"], first_instance_base=5)
    n1, n2 = f["count"], g["count"]
    assert n1 > 0 and n2 > 0
    policy = make_lod_policy(lr.DISTANCE, lr.PIN_SWITCH_SQ)
    frame = make_frame(s["planes"], s["cam_pos"], first_instance_base=5)
    with TC._pipeline(ra, s, vertices, indices, frames_in_flight=2) as p:
        old, moved = TP._Pyramid(ra, TP._wall(0), pv), TP._Pyramid(ra, TP._wall(16), pv)
        bm = TC._device_bitmap(bitmap)
        fr, outs = T._Frame(257), TO._Outs(ra, 257)
        outs.out.flags |= _lib.MIP_OUT_ASYNC
        torch.cuda.synchronize()
        occ_old = old.build(ra, p)
        p.wait()
        for round_ in range(3):
            rec = TP._Record(int(f["stats"][1]))
            a = _Buf(n1 + n2)
            p.run_device(frame, async_=True, **fr.kwargs())
            p.list_clusters_phase(frame, bm.data_ptr(), policy, a.outputs(0, async_=True), occ_old, rec.arg("first"))
            occ_new = moved.build(ra, p)
            p.run_occluded(frame, occ_new, outs.out)
            p.list_clusters_phase(frame, bm.data_ptr(), policy, a.outputs(1, entry_base=a.ptr(0, 0), async_=True), occ_new, rec.arg("second"))
            p.wait()
            a.check_call(0, n1, 0, f["stats"], f"FIRST, round {round_}")
            a.check_call(1, n2, n1, g["stats"], f"SECOND on the other slot, round {round_}")
            a.check_entries([(0, f["entries"]), (n1, g["entries"])], f"round {round_}")
            rec.check(f["record"], f"round {round_}")
