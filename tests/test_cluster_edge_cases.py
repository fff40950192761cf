"""The cluster-culling edge scenes (tests/cluster_edge_cases.py) without a GPU: the tight geometry builds the chosen boxes; the
transfer scenes hold every label of the catalogues they come from, put edge instances on the lanes that matter and tell the
likely mistakes apart; tests/cluster_restatement.py reproduces every independently written command list; the tier edges sit
where they claim, both answers occur and the float64 reference agrees wherever it is decided."""
import json
import os
import subprocess

import numpy as np
import pytest

import cluster_edge_cases as ce
import cluster_restatement as cr
import decision_cases as dc
import float64_reference
import lod_cases as lc
import lod_restatement as lr
import numpy_restatement as nr
import occlusion_cases as oc
import occlusion_restatement as orr

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# Labels that cannot be built as tight geometry, by name, with the reason. The cap is zero plane, LOD and tier labels and at most
# two occlusion labels; none is needed.
NOT_TRANSFERRED = {}


@pytest.fixture(scope="module")
def item_tile(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "cluster_plan_sizes")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "native", "cluster_plan_check.cpp"), "-o", exe])
    return int(json.loads(subprocess.check_output([exe, "sizes"]))["item_tile"])


def _same(got, want, what):
    assert got["cmds"].tobytes() == want["cmds"].tobytes(), (what, "commands")
    assert [int(v) for v in got["stats"]] == [int(v) for v in want["stats"]], (what, "stats", got["stats"], want["stats"])


def _restated(s, boxes, bits, mode, switch_sq, base, occlusion=None):
    r = cr.cull_clusters(s, boxes, ce.bits_to_bitmap(bits), mode, switch_sq, cmd_capacity=1 << 30, first_instance_base=base, occlusion=occlusion)
    assert r["status"] == 0
    return r


def _differs(a, b):
    return a["cmds"].tobytes() != b["cmds"].tobytes()


# ---- tight geometry ----

def _zero_sign_variants(box):
    """The box, and — where an axis holds zeros of both signs — every way the fold may sign them."""
    box = np.asarray(box, F).reshape(6)
    out = [box]
    for ax in range(3):
        lo, hi = box[ax], box[ax + 3]
        if lo == 0 and hi == 0 and np.signbit(lo) != np.signbit(hi):
            more = []
            for b in out:
                for zl in (F(0.0), F(-0.0)):
                    for zh in (F(0.0), F(-0.0)):
                        v = b.copy()
                        v[ax], v[ax + 3] = zl, zh
                        more.append(v)
            out = more
    return out


def _geometries():
    yield "frustum", ce.frustum_geometry()
    yield "nested", ce.nested_geometry()
    yield "chain", ce.chain_geometry()
    for name in oc.NAMES:
        c, s, vertices, indices, want = ce.occlusion_scene(name)
        yield name, (s["meshes"], vertices, indices, want)
    for kind in ce.TIER_KINDS:
        for twin in (False, True):
            yield f"tier {kind} twin={twin}", ce.tier_geometry(kind, twin)


def test_tight_geometry_builds_the_chosen_boxes():
    counts = set()
    for what, (table, vertices, indices, want) in _geometries():
        assert (table["vertex_offset"] > 0).all(), what
        t = cr.cluster_table(table)
        assert int(t["base"][-1]) == len(want), what
        for k in range(len(table)):      # real ranges: inside the indices, every vertex inside the vertices
            for l in range(int(table["n_lods"][k])):
                off, length = int(table["index_offset"][k, l]), int(table["index_len"][k, l])
                assert off + length <= len(indices) and (length == 0 or int(table["vertex_offset"][k]) + int(indices[off : off + length].max()) < len(vertices)), what
        got = cr.cluster_boxes(table, vertices, indices)
        assert got.shape == want.shape and np.array_equal(got, want, equal_nan=True), what      # as numbers
        counts |= {int(c) for c in t["C"]}
        short = t["T"][t["C"] > 0] % 64 != 0
        assert short.any(), what                                                               # a short last cluster
    assert counts >= {0, 1, 2, 3, 65}


def test_the_intended_boxes_are_the_catalogues():
    table, _, _, want = ce.frustum_geometry()
    t = cr.cluster_table(table)
    for b in range(len(t["mesh"])):
        k = int(t["mesh"][b])
        own = want[int(t["base"][b]) : int(t["base"][b + 1])]
        assert (own == np.concatenate([dc.MESHES["aabb_min"][k], dc.MESHES["aabb_max"][k]])[None, :]).all()
    live = np.arange(2)[None, :] < dc.MESHES["n_lods"][:, None]                         # the n_lods pattern and the empty levels are kept
    assert np.array_equal(table["n_lods"], dc.MESHES["n_lods"])
    assert np.array_equal((table["index_len"][:, :2] > 0) & live, (dc.MESHES["index_len"][:, :2] > 0) & live)
    c = cr.level_clusters(table["index_len"])
    assert c[0, 0] != c[0, 1] and table["index_offset"][0, 0] != table["index_offset"][0, 1]   # the LOD shows in the command
    for name in oc.NAMES:
        c, s, vertices, indices, want = ce.occlusion_scene(name)
        t = cr.cluster_table(s["meshes"])
        for b in range(len(t["mesh"])):
            k = int(t["mesh"][b])
            own = want[int(t["base"][b]) : int(t["base"][b + 1])]
            assert len(own) >= 1 and (own.view(np.uint32) == np.concatenate([c["meshes"]["aabb_min"][k], c["meshes"]["aabb_max"][k]]).view(np.uint32)[None, :]).all(), name


def test_a_zero_of_either_sign_decides_the_same():
    """Where a box holds zeros of both signs on an axis the fold may return either: the restatement's decision must not hang on
    it. Every such box of every geometry is decided under every sign, for the instances that draw it."""
    seen = 0
    for name in oc.NAMES:
        c, s, vertices, indices, want = ce.occlusion_scene(name)
        levels = orr.pyramid_levels(c["depth"])
        t = cr.cluster_table(s["meshes"])
        for b in range(len(t["mesh"])):
            variants = _zero_sign_variants(want[int(t["base"][b])])
            if len(variants) == 1:
                continue
            seen += 1
            inst = np.nonzero(s["mesh_id"] == t["mesh"][b])[0]
            answers = set()
            for v in variants:
                model = nr.model_matrices(s["pos"][inst], s["rot"][inst], s["scale"][inst])
                box = np.tile(v[None, :], (len(inst), 1))
                mins, maxs = nr.world_aabbs(model, box[:, :3], box[:, 3:])
                answers.add(tuple(orr.occluded(np.concatenate([mins, maxs], 1), c["pv"], levels, c["width"], c["height"]).tolist()))
            assert len(answers) == 1, (name, b)
    for what, (table, vertices, indices, want) in (("frustum", ce.frustum_geometry()), ("nested", ce.nested_geometry()), ("chain", ce.chain_geometry())):
        assert all(len(_zero_sign_variants(b)) == 1 for b in want), what
    print("boxes with zeros of both signs:", seen)


# ---- the frustum set ----

def _frustum_all(item_tile):
    for name, frame in ce.FRUSTUM_INPUTS:
        for what, s, bits, src in ce.frustum_scenes(name, frame, item_tile):
            yield name, frame, what, s, bits, src


def test_frustum_scenes_hit_their_sizes_and_hold_every_label(item_tile):
    for name, frame in ce.FRUSTUM_INPUTS:
        scenes = ce.frustum_scenes(name, frame, item_tile)
        table = scenes[0][1]["meshes"]
        got = []
        for what, s, bits, src in scenes:
            items = cr.work_items(s["pos"], s["scale"], s["mesh_id"], table, s["cam_pos"], ce.bits_to_bitmap(bits), lr.DISTANCE, ce.PIN)
            got.append(items["W"])
        assert tuple(got[:-1]) == ce.frustum_targets(item_tile), (name, frame, got)
        what, s, bits, src = scenes[-1]
        assert s["n"] == 513 and bits.all() and set(src[src >= 0].tolist()) == set(range(len(dc.case(name)["scale"]))), (name, frame)   # no label left out
    assert NOT_TRANSFERRED == {}


def test_frustum_edge_instances_on_the_lanes_that_matter(item_tile):
    """From cluster_restatement.work_items: labelled edge instances own work items on lane 0, on lane 63, and straddle a wave
    boundary (items 63 | 64 of a wave pair) — also among the instances of at most three clusters."""
    lane0 = lane63 = straddle = small_straddle = 0
    for name, frame, what, s, bits, src in _frustum_all(item_tile):
        labelled = set(dc.labelled(dc.case(name), frame=frame, ref=frame))
        items = cr.work_items(s["pos"], s["scale"], s["mesh_id"], s["meshes"], s["cam_pos"], ce.bits_to_bitmap(bits), lr.DISTANCE, ce.PIN)
        edge = np.array([int(src[i]) in labelled for i in items["inst"]], bool)
        lane = np.arange(items["W"]) & 63
        lane0 += int((edge & (lane == 0)).sum())
        lane63 += int((edge & (lane == 63)).sum())
        same = items["inst"][1:] == items["inst"][:-1]
        cross = edge[1:] & same & (lane[1:] == 0)
        straddle += int(cross.sum())
        counts = np.bincount(items["inst"], minlength=s["n"])
        small_straddle += int((cross & (counts[items["inst"][1:]] <= 3)).sum())
    assert lane0 > 0 and lane63 > 0 and straddle > 0 and small_straddle > 0, (lane0, lane63, straddle, small_straddle)


def test_the_restatement_reproduces_the_frustum_set(item_tile):
    table, vertices, indices, _ = ce.frustum_geometry()
    boxes = cr.cluster_boxes(table, vertices, indices)
    for name, frame, what, s, bits, src in _frustum_all(item_tile):
        want = ce.frustum_want(s, bits)
        _same(_restated(s, boxes, bits, lr.DISTANCE, ce.PIN, ce.FRUSTUM_BASE), want, what)
        visible = dc.decide(s)["visible"]                                   # the frame's own bitmap
        _same(_restated(s, boxes, visible, lr.DISTANCE, ce.PIN, ce.FRUSTUM_BASE), ce.frustum_want(s, visible), what + " frame bitmap")


def test_frustum_set_tells_the_mutants_apart(item_tile):
    flipped = {m: 0 for m in dc.MUTANTS}
    for name, frame, what, s, bits, src in _frustum_all(item_tile):
        want = ce.frustum_want(s, bits)
        for m in dc.MUTANTS:
            flipped[m] += _differs(want, ce.frustum_want(s, bits, m))
    print("frustum set, scenes whose expected commands a mutant changes:", flipped)
    assert all(v > 0 for v in flipped.values()), flipped


def test_every_light_ring_and_every_instance_tier_edge_is_transferred():
    """The labels RUN_INPUTS does not reach: the ring of every light (the light as the reference point), and the instances whose
    own position or scale sits on a tier limit. The restatement reproduces the written lists; the LOD mutants show."""
    table, vertices, indices, _ = ce.frustum_geometry()
    boxes = cr.cluster_boxes(table, vertices, indices)
    c = dc.case("lights")
    flipped = {"gt_100": 0, "ge_threshold": 0}
    for light in range(dc.N_LIGHTS):
        s, src = ce.light_scene(light)
        assert set(src[src >= 0].tolist()) == set(range(len(c["scale"])))
        ring = [l for l in c["labels"] if l["ref"] == f"light{light}"]
        assert {l["cls"] for l in ring} == set(dc.ring_classes(nan=True))
        sq = dc.decide(s)["dist_sq"]
        for l in ring:                                                      # the ring sits where its label says, for this light
            if l["cls"] in dict(dc.LOD_RING):
                assert sq[np.nonzero(src == l["index"])[0][0]] == dc.lod_ring_value(l["cls"]), (light, l)
        bits = np.ones(s["n"], bool)
        want = ce.frustum_want(s, bits)
        _same(_restated(s, boxes, bits, lr.DISTANCE, ce.PIN, ce.FRUSTUM_BASE), want, ("light", light))
        for m in flipped:
            flipped[m] += _differs(want, ce.frustum_want(s, bits, m))
    print("light rings, scenes whose expected commands a mutant changes:", flipped)
    assert all(v > 0 for v in flipped.values()), flipped
    for kind in dc.TIER_KINDS:
        for placement in dc.TIER_PLACEMENTS:
            scenes, odd = ce.instance_tier_scenes(kind, placement)
            for s in scenes:
                bits = np.ones(s["n"], bool)
                _same(_restated(s, boxes, bits, lr.DISTANCE, ce.PIN, ce.FRUSTUM_BASE), ce.frustum_want(s, bits), (kind, placement))
            assert (dc.tier(scenes[0]["pos"][list(odd)], scenes[0]["rot"][list(odd)], scenes[0]["scale"][list(odd)]) ==
                    {"sep_below": 0, "sep_at": 1, "fin_below": 1, "fin_at": 2}[kind]).all()


# ---- split decisions ----

@pytest.mark.parametrize("name,frame", ce.SPLIT_INPUTS)
def test_split_decisions(name, frame):
    s, labels = ce.split_scene(name, frame)
    patterns = ce.split_patterns(s)
    assert {l["cls"] for l in labels} >= ({"tie0", "ulp_in", "ulp_out"} if name == "axis" else {"edge_in", "edge_out"})
    assert {l["slot"] for l in labels} == set(range(6))
    for l, p in zip(labels, patterns):
        assert p == ce.SPLIT_CLASSES[l["cls"]], (l, p)
    # the half and the double box are DECIDED, far from their own edge: only the unit box sits on it
    for box, want in ((ce.NESTED_BOXES[1], False), (ce.NESTED_BOXES[2], True)):
        m = s["meshes"].copy()
        m["aabb_min"], m["aabb_max"] = box[:3], box[3:]
        ref = float64_reference.run(dict(s, meshes=m))
        assert ref["decided"].all() and (~ref["culled"] == want).all(), box
    table, vertices, indices, _ = ce.nested_geometry()
    want = ce.pattern_commands(table, patterns, 9)
    assert len(want["cmds"]) == 2 * sum(p == "101" for p in patterns) + sum(p == "001" for p in patterns)
    _same(_restated(s, cr.cluster_boxes(table, vertices, indices), np.ones(s["n"], bool), lr.DISTANCE, ce.PIN, 9), want, (name, frame))
    # `sd - e >= 0` turns every tie's 1 0 1 into 0 0 1: one command less per tie
    assert any(l["cls"] == "tie0" for l in labels)
    assert _differs(want, ce.pattern_commands(table, ce.split_patterns(s, "ge_zero"), 9))


# ---- the six-level chain ----

@pytest.mark.parametrize("mode", [lc.DISTANCE, lc.RELATIVE])
def test_chain_scenes(mode):
    table, vertices, indices, _ = ce.chain_geometry()
    assert cr.cluster_table(table)["C"].tolist() == [1, 2, 3, 4, 5, 6, 1, 2, 3, 1, 2, 0, 4, 5, 6]
    boxes = cr.cluster_boxes(table, vertices, indices)
    s = ce.chain_scene(mode)
    for short, sw in ((False, lc.SWITCH), (True, lc.SWITCH_SHORT)):
        lod = lc.want_edge_lods(s, mode, short)
        assert set(lod.tolist()) == ({0, 1, 2} if short else {0, 1, 2, 3, 4, 5})
        want = ce.chain_want(s, mode, short)
        empty = (s["mesh_id"] == 2) & (lod == 2)
        assert empty.any() and int(want["stats"][3]) == s["n"] - int(empty.sum()) == len(want["cmds"])
        _same(_restated(s, boxes, np.ones(s["n"], bool), mode, sw, ce.CHAIN_BASE), want, (mode, short))
        # an off-by-one pick of one instance shifts every later command
        other = lod.copy()
        i = int(np.nonzero((s["case"] >= 0) & (s["mesh_id"] == 0))[0][3])
        other[i] = (other[i] + 1) % 3
        assert _differs(want, ce.chain_want(s, mode, short, other))


# ---- Hi-Z ----

def test_occlusion_catalogue_is_transferred_whole_and_restated():
    labels = 0
    for name in oc.NAMES:
        c, s, vertices, indices, _ = ce.occlusion_scene(name)
        t, _ = ce.level_sizes(s["meshes"], s["mesh_id"], np.zeros(s["n"], np.int64))
        assert (t > 0).all(), name                                          # every instance is a member: no label is left out
        labels += len(c["labels"])
        want = ce.occlusion_want(c, s)
        hidden = orr.occluded(c["boxes"], c["pv"], orr.pyramid_levels(c["depth"]), c["width"], c["height"])
        idx = np.array([l["index"] for l in c["labels"]], np.int64)
        assert len(want["cmds"]) == int((~hidden).sum()) and set(idx[~hidden[idx]] + ce.OCCLUSION_BASE) <= set(want["cmds"]["firstInstance"].tolist())
        occlusion = dict(pv=c["pv"], levels=orr.pyramid_levels(c["depth"]), width=c["width"], height=c["height"])
        got = _restated(s, cr.cluster_boxes(s["meshes"], vertices, indices), np.ones(s["n"], bool), lr.DISTANCE, ce.PIN, ce.OCCLUSION_BASE, occlusion)
        _same(got, want, name)
    assert labels > 1000 and NOT_TRANSFERRED == {}


def test_occlusion_set_tells_the_mutants_apart():
    flipped = {}
    for m in oc.MUTANTS:
        if m in oc.EQUIVALENT_MUTANTS:
            continue
        flipped[m] = 0
        for name in oc.NAMES:
            c, s, *_ = ce.occlusion_scene(name)
            flipped[m] += _differs(ce.occlusion_want(c, s), ce.occlusion_want(c, s, m))
    print("occlusion set, cases whose expected commands a mutant changes:", flipped)
    assert all(v > 0 for v in flipped.values()), flipped


# ---- box-sourced tier edges ----

def test_tier_half_extents_sit_on_the_limits():
    """The BUILT cluster box of every limit kind: the last float below / the first at or above each limit for the ordinary
    instance; the copy of scale 2^-20 is separable wherever it is finite."""
    h = ce.tier_half_extents()
    up = lambda x: np.nextafter(F(x), F(np.inf))
    assert up(h["sep_below"]) == h["sep_at"] and up(h["fin_below"]) == h["fin_at"]
    want = {"sep_below": (True, True), "sep_at": (True, False), "fin_below": (True, False), "fin_at": (False, False)}
    small = {"sep_below": (True, True), "sep_at": (True, True), "fin_below": (True, True), "fin_at": (False, False)}
    for kind in ce.TIER_LIMIT_KINDS:
        table, vertices, indices, _ = ce.tier_geometry(kind)
        built = cr.cluster_boxes(table, vertices, indices)
        assert np.array_equal(built[1], ce.odd_box(h[kind])) and np.array_equal(built[3], built[1]) and np.array_equal(built[2], np.array(ce.ORDINARY, F))
        assert ce.box_tier(ce.TIER_POS, dc.TIER_ROT, F(1.0), built[1]) == want[kind], kind
        assert ce.box_tier(ce.TIER_POS, dc.TIER_ROT, ce.TIER_SMALL, built[1]) == small[kind], kind
        assert ce.box_tier(ce.TIER_POS, dc.TIER_ROT, F(1.0), built[2]) == (True, True)
    for kind in ce.TIER_NONFINITE_KINDS:
        table, vertices, indices, _ = ce.tier_geometry(kind)
        built = cr.cluster_boxes(table, vertices, indices)
        assert ce.box_tier(ce.TIER_POS, dc.TIER_ROT, F(1.0), built[1]) == (False, False), kind
    inf = np.inf
    first = lambda kind: cr.cluster_boxes(*ce.tier_geometry(kind)[:3])[1].tolist()
    assert first("inf_max") == [1, -1, -1, inf, 1, 1] and first("inf_both") == [-inf, -1, -1, inf, 1, 1]
    assert first("nan_axis") == [inf, -1, -1, -inf, 1, 1] and first("flt_max") == [-float(ce.FLT_MAX)] * 3 + [float(ce.FLT_MAX)] * 3
    assert dc.rotation(dc.TIER_ROT)[0, 0, 1] != 0                           # not the identity


def _tier_restated(kind, placement, frame, twin):
    t = ce.tier_scene(kind, placement, frame)
    table, vertices, indices, _ = ce.tier_geometry(kind, twin)
    s = dict(t["scene"], meshes=table)
    return t, s, _restated(s, cr.cluster_boxes(table, vertices, indices), np.ones(s["n"], bool), lr.DISTANCE, ce.PIN, ce.TIER_BASE)


def test_tier_scenes_place_the_odd_items_and_both_answers_occur():
    answers = {kind: set() for kind in ce.TIER_KINDS}
    against_float64 = {kind: 0 for kind in ce.TIER_KINDS}
    for kind in ce.TIER_KINDS:
        for placement, (front, w) in ce.TIER_PLACEMENTS.items():
            for frame in ce.TIER_FRAMES:
                t, s, r = _tier_restated(kind, placement, frame, False)
                _, s2, r2 = _tier_restated(kind, placement, frame, True)
                items = r["items"]
                assert items["W"] == w == r2["items"]["W"] and np.array_equal(items["inst"], r2["items"]["inst"])
                odd = np.array(t["odd_items"])
                assert set(items["inst"][odd].tolist()) == set(t["odd_instances"]) and items["cluster"][odd].tolist() == [0, 2, 0, 2]
                lanes = (odd & 63).tolist()
                if placement == "lane0":
                    assert lanes[0] == 0 and odd[0] == 64
                if placement == "lane63":
                    assert lanes[0] == 63
                if placement == "pair":
                    assert (odd[1], odd[2]) == (63, 64)
                if placement == "ragged":
                    assert w % 64 and odd[0] // 64 == (w - 1) // 64
                answers[kind] |= set(r["survive"][odd].tolist())
                assert r2["survive"].all()                                  # the twin: every cluster is ordinary and inside
                ordinary = np.ones(w, bool)
                ordinary[[i for i in range(w) if items["inst"][i] in t["odd_instances"]]] = False
                assert r["survive"][ordinary].all()
                # the commands of the instances that own no odd item: byte-identical in the twin
                base = ce.TIER_BASE
                mine = lambda x: x["cmds"][~np.isin(x["cmds"]["firstInstance"] - base, t["odd_instances"])]
                assert mine(r).tobytes() == mine(r2).tobytes() and len(mine(r)) == s["n"] - 2
                # every finite odd item: the float64 reference's decision wherever it is decided
                boxes = cr.cluster_boxes(s["meshes"], *ce.tier_geometry(kind)[1:3])
                for it in odd:
                    i = int(items["inst"][it])
                    box = boxes[int(items["box_index"][it])]
                    model = nr.model_matrices(s["pos"][[i]], s["rot"][[i]], s["scale"][[i]])
                    mins, maxs = nr.world_aabbs(model, box[None, :3], box[None, 3:])
                    if not (np.isfinite(box).all() and np.isfinite(mins).all() and np.isfinite(maxs).all()):
                        continue
                    m = s["meshes"][:1].copy()
                    m["aabb_min"], m["aabb_max"] = box[:3], box[3:]
                    ref = float64_reference.run(dict(pos=s["pos"][[i]], rot=s["rot"][[i]], scale=s["scale"][[i]], mesh_id=np.zeros(1, np.int64), meshes=m,
                                                     planes=s["planes"]))
                    if ref["decided"][0]:
                        against_float64[kind] += 1
                        assert bool(r["survive"][it]) == (not ref["culled"][0]), (kind, placement, frame, int(it))
    print("tier edges, answers of the odd items:", {k: sorted(v) for k, v in answers.items()})
    for kind in ce.TIER_LIMIT_KINDS:
        assert answers[kind] == {True, False}, (kind, answers[kind])
        assert against_float64[kind] >= 2 * len(ce.TIER_PLACEMENTS) * len(ce.TIER_FRAMES), (kind, against_float64)   # not vacuous
    assert set().union(*answers.values()) == {True, False}


def test_refusal_geometry_is_on_its_edge():
    g = ce.refusal_geometry()
    used = g["indices"][: 3 * (int(g["table"]["index_len"][0, 0]) // 3)]
    assert int(g["table"]["vertex_offset"][0]) + int(used.max()) == len(g["vertices"]) - 1
    assert int(g["indices"][len(used):].min()) > len(g["vertices"])        # only the tail points out of range
    assert cr.cluster_boxes(g["table"], g["vertices"], g["indices"]).tolist() == [[6, 7, 8, 21, 22, 23]]
