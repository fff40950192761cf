"""The several-view edge scenes (tests/view_edge_cases.py) without a GPU: every expectation written from the instance-level
decision equals the numpy restatement of the call (tests/cluster_views_restatement.py, tests/views_batch_restatement.py) on
every call of every set — two independent descriptions —, every rotation puts a labelled edge instance into the first, a middle
and the last slot, the rules of the module's docstring hold, and each likely mistake of the code AROUND the shared device
functions changes the expected bytes of a call NAMED here. No wrong kernel is built or run: only the expectation writer's
hooks or the restatement's inputs and outputs are mutated."""
import numpy as np
import pytest

import cluster_edge_cases as ce
import cluster_restatement as cr
import cluster_view_cases as cv
import cluster_views_restatement as cvr
import decision_cases as dc
import lod_cases as lc
import view_edge_cases as ve
import views_batch_restatement as vr

F = np.float32
_BOXES = {}


def _boxes(c):
    table, vertices, indices, _ = c["geometry"]
    if id(table) not in _BOXES:
        _BOXES[id(table)] = (table, cr.cluster_boxes(table, vertices, indices))     # (the table is kept: its id stays its own)
    return _BOXES[id(table)][1]


def _restated(c, bits=None):
    bits = c["bits"] if bits is None else bits
    r = cvr.cull_clusters_views(c["s"], _boxes(c), c["planes"], [None if b is None else ce.bits_to_bitmap(b) for b in bits], c["bases"], c["mode"], c["switch"],
                                cmd_stride=1 << 30, cam_pos=c["cams"][0])
    assert r["status"] == 0, c["name"]
    return r


def _batch_restated(c):
    s = c["s"]
    return vr.batch_draws_views(s["pos"], s["scale"], s["mesh_id"], s["meshes"], c["cams"], [None if b is None else ce.bits_to_bitmap(b) for b in c["bits"]],
                                c["bases"], c["mode"], c["switch"])


def _same(got, want):
    return len(got["cmds"]) == len(want["cmds"]) and all(a.tobytes() == b.tobytes() for a, b in zip(got["cmds"], want["cmds"])) and \
        [int(x) for x in got["stats"]] == [int(x) for x in want["stats"]]


def _batch_same(got, want):
    return _same(dict(got, stats=got["first_slot"]), dict(want, stats=want["first_slot"])) and got["ids"].tobytes() == want["ids"].tobytes() and \
        got["counts"].tolist() == want["counts"].tolist() and got["members"] == want["members"]


# ---- the two descriptions agree, on every call: none is skipped ----

@pytest.mark.parametrize("which", ve.SETS)
def test_every_expectation_equals_the_restatement(which):
    calls = ve.calls(which)
    assert len(calls) >= {"frustum": 72, "lod": 8, "chain": 12, "split": 6, "tier": 224, "mask": 2}[which]
    for c in calls:
        assert _same(_restated(c), c["want"]), c["name"]


@pytest.mark.parametrize("which", ve.BATCH_SETS)
def test_every_batch_expectation_equals_the_restatement(which):
    calls = ve.batch_calls(which)
    assert len(calls) >= {"frustum": 144, "lod": 16, "chain": 24}[which] and {c["padded"] for c in calls} == {False, True}
    for c in calls:
        assert _batch_same(_batch_restated(c), c["want"]), c["name"]
        assert (len(c["planes"]) * c["want"]["n_buckets"] > 256) == c["padded"], c["name"]      # one pass | several


def test_a_padded_table_moves_offsets_only():
    one, several = ve.batch_frustum_call("union", 2, 16, 513, False), ve.batch_frustum_call("union", 2, 16, 513, True)
    assert np.array_equal(one["s"]["mesh_id"], several["s"]["mesh_id"]) and len(several["s"]["meshes"]) > len(one["s"]["meshes"])
    assert several["s"]["mesh_id"].max() < len(dc.MESHES)                                       # no instance references a padding mesh
    assert _batch_same(one["want"], dict(several["want"], n_buckets=one["want"]["n_buckets"]))  # every decision unchanged: the same bytes


# ---- slot coverage ----

def test_rotations_put_every_frame_into_every_slot():
    for case in dc.VIEW_INPUTS:
        frames = dc.case(case)["frames"]
        for n_views in (len(frames), 16):
            lists = ve.rotations(case, n_views)
            for slot in (0, n_views // 2, n_views - 1) + ((8, 15) if n_views == 16 else ()):
                assert {l[slot] for l in lists} == set(frames), (case, n_views, slot)
    assert ve.bases(16)[0] == ce.FRUSTUM_BASE and 0x80000000 in ve.bases(16) and len(set(ve.bases(16))) == 16


def test_every_rotation_has_a_labelled_edge_instance_in_the_first_a_middle_and_the_last_slot():
    """At the sizes every rotation runs at, and for the LOD set: a label built for the frame of slot 0, of the middle slot and
    of the last slot is among the instances, with its bit set in that view; with sixteen views every slot 8 .. 15
    has one."""
    seen, live_at = 0, set()
    for c in ve.calls("frustum") + ve.calls("lod"):
        if c["s"]["n"] not in ve.ROTATION_SIZES:
            continue
        n_views = len(c["names"])
        for slot in sorted({0, n_views // 2, n_views - 1} | (set(range(8, 16)) if n_views == 16 else set())):
            idx = ve.edge_labels(c, slot)
            live = [i for i in idx if c["bits"][slot] is None or c["bits"][slot][i]]
            # (a view that shares view 0's pointer holds view 0's visible instances: its own frame's edge instances are resident,
            # their bits need not be set; the first, the middle and the last slot never share)
            assert idx and (live or c["kinds"][slot] == "shared") and (live or slot not in (0, n_views // 2, n_views - 1)), (c["name"], slot, c["names"][slot])
            seen += 1
            if live:
                live_at.add((c["case"], n_views, slot, c["names"][slot]))
    assert seen > 300
    # ... and every frame of a case meets the first, a middle and the last slot with such an instance's bit SET, in some rotation
    for case in dc.VIEW_INPUTS + ("views",):
        frames = dc.case(case)["frames"]
        for n_views in (len(frames), 16):
            for slot in (0, n_views // 2, n_views - 1):
                assert {f for f in frames if (case, n_views, slot, f) in live_at} == set(frames), (case, n_views, slot)
    kinds = [ve.kinds(16, r) for r in range(7)]                             # a NULL and a given bitmap in each of the three slots, every kind in between
    assert all({k[v] for k in kinds} == {"null", "given"} for v in (0, 8, 15)) and {k[9] for k in kinds} == set(ve.KINDS)


# ---- the rules of the docstring ----

def test_lod_ownership_only_the_ring_of_slot_0_is_live():
    ring = dict(dc.LOD_RING)
    case = dc.case("views")
    for c in ve.calls("lod"):
        n, names = c["s"]["n"], c["names"]
        sq0 = ve._decision("views", n, names[0], names[0])["dist_sq"]
        for v in range(4):
            own = ve._decision("views", n, names[0], names[v])
            flips = 0
            for l in case["labels"]:
                if l.get("ref") != names[v]:
                    continue
                i = int(np.nonzero(c["src"] == l["index"])[0][0])
                if l["cls"] in ring:
                    assert own["dist_sq"][i] == dc.lod_ring_value(l["cls"])                    # live under its own camera ...
                    assert (v == 0) == (F(99.0) < sq0[i] < F(101.0)), (c["name"], v, l)         # ... and under slot 0's only if it is slot 0's
                flips += int(own["lod"][i] != ve._decision("views", n, names[0], names[0])["lod"][i])
            assert (flips > 0) == (v > 0), (c["name"], v)                                       # a ring picked by the wrong camera shows
    # the batch call: view v's members sit at view v's own levels
    b = ve.batch_frustum_call("views", 1, 4, 257, False, "lod")
    lods = [ve._decision("views", 257, b["names"][0], f)["lod"] for f in b["names"]]
    assert len({l.tobytes() for l in lods}) == 4
    assert _batch_same(b["want"], ve.batch_want(dc.MESHES, b["s"]["mesh_id"], lods, b["bits"], b["bases"]))


@pytest.mark.parametrize("mode", [lc.DISTANCE, lc.RELATIVE])
def test_chain_rules(mode):
    s = ce.chain_scene(mode)
    for short in (False, True):
        far, near = ve.far_lods(s, mode, short), lc.want_edge_lods(s, mode, short)
        top = np.minimum(2 if short else 5, s["meshes"]["n_lods"][s["mesh_id"]].astype(np.int64) - 1)
        assert ((far == top) | (far == 0)).all() and (far != near).sum() > 100 and 0 < (far != top).sum() < 200
        for slot in ve.CHAIN_SLOTS:
            c = ve.chain_call(mode, short, slot)
            assert [np.array_equal(cam, np.zeros(3, F)) for cam in c["cams"]] == [v == slot for v in range(16)]
            # the cluster call: every view has the levels of slot 0 — the commands differ by the base and the bits only
            lod = near if slot == 0 else far
            for v in (0, 7, 15):
                bits = np.ones(s["n"], bool) if c["bits"][v] is None else c["bits"][v]
                assert c["want"]["cmds"][v].tobytes() == ce.transfer_commands(s["meshes"], s["mesh_id"], lod, bits, bits, c["bases"][v])["cmds"].tobytes()
            if slot == 0:                                                   # cluster_edge_cases.chain_want, moved to the view's base
                moved = ce.chain_want(s, mode, short)["cmds"].copy()
                moved["firstInstance"] = (moved["firstInstance"].astype(np.int64) - ce.CHAIN_BASE + c["bases"][0]) & 0xFFFFFFFF
                assert c["want"]["cmds"][0].tobytes() == moved.tobytes()
            # the batch call: the edge view alone has the chain scene's levels
            lods = ve.chain_batch_lods(c)
            assert all(np.array_equal(lods[v], near if v == slot else far) for v in range(16))


def test_split_and_mask_answers():
    for key in ve.split_keys():
        c = ve.split_call(*key)
        s, table = c["s"], c["geometry"][0]
        for v, o in enumerate(c["order"]):
            got = c["want"]["cmds"][v]
            if o == "none":
                assert len(got) == 0
            if o == "all":
                assert len(got) == s["n"] and (got["indexCount"] == 3 * (int(table["index_len"][0, 0]) // 3)).all()
            if o == "edge":
                assert got.tobytes() == ce.pattern_commands(table, ce.split_patterns(s), c["bases"][v])["cmds"].tobytes() and 0 < len(got) < 2 * s["n"]
        assert c["want"]["stats"][:2].tolist() == [3 * s["n"], s["n"]]
        assert ce.box_decisions(dict(s, planes=ve.EVERYTHING), ce.NESTED_BOXES[2]).all() and not ce.box_decisions(dict(s, planes=ve.NOTHING), ce.NESTED_BOXES[2]).any()
    for layout in ve.MASK_LAYOUTS:
        c = ve.mask_call(layout)
        specs = [("A", c["bits"][v], c["bases"][v]) for v in range(16)]
        _, _, ladder = cv.ladder_views(["1"], [0] * 33, specs)              # the hand-written answer is the ladder's
        assert _same(dict(cmds=ladder["cmds"], stats=ladder["stats"]), c["want"]), layout
        masks = sum(np.asarray(c["bits"][v], np.int64) << v for v in range(16))
        assert len(set(masks[:32].tolist()) - {0}) == 16 and int(masks[32]) == 0xFFFF and ((masks == 0).sum() == 1) == (layout != "every bit")


def test_box_tier_twins():
    for kind in ce.TIER_KINDS:
        for placement in ce.TIER_PLACEMENTS:
            for views in ve.TIER_LISTS:
                odd, twin = ve.tier_box_call(kind, placement, views, False), ve.tier_box_call(kind, placement, views, True)
                for v in range(len(odd["planes"])):
                    mine = ve.without_odd(odd["want"]["cmds"][v], odd["bases"][v], odd["odd_instances"])
                    assert mine.tobytes() == ve.without_odd(twin["want"]["cmds"][v], twin["bases"][v], odd["odd_instances"]).tobytes() and len(mine) > 100


# ---- the likely mistakes, each killed by a NAMED call ----

def _no_wrap(want, c):
    """base + i saturating instead of wrapping: the expectation writer's last step, mutated."""
    out = []
    for v, cmds in enumerate(want["cmds"]):
        cmds = cmds.copy()
        i = (cmds["firstInstance"].astype(np.int64) - int(c["bases"][v])) & 0xFFFFFFFF
        cmds["firstInstance"] = np.minimum(int(c["bases"][v]) + i, 0xFFFFFFFF)
        out.append(cmds)
    return dict(want, cmds=out)


def _stale_words(c):
    """View v inherits view v - 1's survive word for every 64-item word that holds no member of view v: the restatement's
    survive flags rewritten, its own command writer run on them."""
    r = _restated(c)
    items, n = r["items"], c["s"]["n"]
    word = np.arange(items["W"]) >> 6
    cmds, stats, before = [], r["stats"].copy(), None
    for v, sv in enumerate(r["survive"]):
        sv = sv.copy()
        if before is not None:
            live = (np.ones(n, bool) if c["bits"][v] is None else c["bits"][v])[items["inst"]]
            dead = ~np.isin(word, word[live])
            sv[dead] = before[dead]
        out, _ = cr.commands(items, sv, c["s"]["meshes"], c["bases"][v])
        cmds.append(out)
        stats[2 + 2 * v], stats[3 + 2 * v] = len(out), int(sv.sum())
        before = sv
    return dict(cmds=cmds, stats=stats)


def _zeros(c):
    return np.zeros(c["s"]["n"], bool)


U16 = lambda r, n: ve.frustum_call("union", r, 16, n)                       # noqa: E731
NAMED = {
    "view 0's planes for every view": (lambda: U16(0, 513), lambda c: ve.frustum_want(c, planes=[0] * 16)),
    "view v + 1's planes": (lambda: ve.frustum_call("union", 3, 7, 257), lambda c: ve.frustum_want(c, planes=[(v + 1) % 7 for v in range(7)])),
    "view v - 1's planes": (lambda: ve.frustum_call("union_nonfinite", 1, 5, 513), lambda c: ve.frustum_want(c, planes=[(v - 1) % 5 for v in range(5)])),
    "level from frames[v].cam_pos": (lambda: ve.frustum_call("views", 2, 4, 257, set_="lod"), lambda c: ve.frustum_want(c, lod_cams=list(range(4)))),
    "gt_100 on the level pick": (lambda: ve.frustum_call("views", 1, 16, 257, set_="lod"), lambda c: ve.frustum_want(c, lod_mutant="gt_100")),
    "ge_threshold on the level pick": (lambda: ve.frustum_call("views", 3, 16, 257, set_="lod"), lambda c: ve.frustum_want(c, lod_mutant="ge_threshold")),
    "the mask cut to 8 bits": (lambda: ve.mask_call("every bit"), lambda c: _restated(c, bits=[b if v < 8 else _zeros(c) for v, b in enumerate(c["bits"])])),
    "bit 15 lost": (lambda: ve.mask_call("every bit"), lambda c: _restated(c, bits=[b if v < 15 else _zeros(c) for v, b in enumerate(c["bits"])])),
    "bit v from view 0's bitmap": (lambda: ve.mask_call("an instance in no view"), lambda c: _restated(c, bits=[c["bits"][0]] * 16)),
    "a NULL bitmap read as empty": (lambda: U16(2, 257), lambda c: _restated(c, bits=[_zeros(c) if b is None else b for b in c["bits"]])),
    "W and members from view 0's bits": (lambda: U16(1, 513), lambda c: ve.frustum_want(c, union=c["bits"][0])),
    "view 0's base for every view": (lambda: U16(0, 257), lambda c: ve.frustum_want(c, bases_=[c["bases"][0]] * 16)),
    "the base added without wrap-around": (lambda: U16(0, 513), lambda c: _no_wrap(c["want"], c)),
    "a stale survive word": (lambda: U16(1, 513), _stale_words),
}


@pytest.mark.parametrize("mistake", list(NAMED))
def test_named_call_kills(mistake):
    build, mutate = NAMED[mistake]
    c = build()
    assert _same(_restated(c), c["want"]) and not _same(mutate(c), c["want"]), (mistake, c["name"])


def test_no_wrap_shows_only_above_256_instances_under_the_wrapping_base():
    for n in (255, 256):
        c = U16(ve.ALL_SIZES_ROTATION["union"], n)
        assert _same(_no_wrap(c["want"], c), c["want"]), n
    c = U16(0, 513)
    changed = [v for v in range(16) if _no_wrap(c["want"], c)["cmds"][v].tobytes() != c["want"]["cmds"][v].tobytes()]
    assert changed == [0] and c["bases"][0] == ce.FRUSTUM_BASE


# one plane mutant in ONE slot — slot 0, a middle one and 15 —, under the rotation that puts a frame with such an edge there
PLANE_SLOT_KILLS = {("ge_zero", 0): ("union", 5, 16, 513), ("ge_zero", 8): ("union", 4, 16, 513), ("ge_zero", 15): ("union", 4, 16, 513),
                    ("flush_margin", 0): ("union", 4, 16, 513), ("flush_margin", 8): ("union", 3, 16, 513), ("flush_margin", 15): ("union", 3, 16, 513),
                    ("flush_inputs", 0): ("union", 4, 16, 513), ("flush_inputs", 8): ("union", 3, 16, 513), ("flush_inputs", 15): ("union", 3, 16, 513)}


@pytest.mark.parametrize("mutant,slot", list(PLANE_SLOT_KILLS))
def test_a_plane_mutant_in_one_slot_is_killed(mutant, slot):
    c = ve.frustum_call(*PLANE_SLOT_KILLS[(mutant, slot)])
    got = ve.frustum_want(c, plane_mutant={slot: mutant})
    assert not _same(got, c["want"]), (mutant, slot, c["name"])
    assert [v for v in range(16) if got["cmds"][v].tobytes() != c["want"]["cmds"][v].tobytes()] == [slot]     # and in that slot only


BATCH_NAMED = {
    "level from frames[0].cam_pos": (("views", 1, 4, 257, False, "lod"), lambda c: ve.batch_frustum_want(c, lod_cams=[0] * 4)),
    "gt_100 on the level pick": (("views", 0, 16, 257, False, "lod"), lambda c: ve.batch_frustum_want(c, lod_mutant="gt_100")),
    "ge_threshold on the level pick": (("views", 2, 16, 257, True, "lod"), lambda c: ve.batch_frustum_want(c, lod_mutant="ge_threshold")),
    "view 0's base for every view": (("union", 2, 16, 257, True), lambda c: ve.batch_frustum_want(c, bases_=[c["bases"][0]] * 16)),
}


@pytest.mark.parametrize("mistake", list(BATCH_NAMED))
def test_named_batch_call_kills(mistake):
    key, mutate = BATCH_NAMED[mistake]
    c = ve.batch_frustum_call(*key)
    assert _batch_same(_batch_restated(c), c["want"]) and not _batch_same(mutate(c), c["want"]), (mistake, c["name"])
    if "level from" in mistake:                                             # every view behind view 0 shows it, each on its own ring
        got = mutate(c)
        assert all(got["cmds"][v].tobytes() != c["want"]["cmds"][v].tobytes() for v in range(1, 4))
