"""The occlusion-edge catalogue (tests/occlusion_cases.py) without a GPU: every label is what occlusion_terms computes (over
the catalogue's boxes and over the oracle's world_aabb, which are the same bits), every class is there on both sides of its
edge and on the lanes and tile ends, every likely mistake — written as a mutant of the restatement, never as a kernel —
flips a labelled instance in an f32 and in a u16 scene, the float64 computation agrees wherever it calls a case decided and
calls every tie undecided, and every structural class of mip_depth_pyramid_kernel has a shape."""
import numpy as np
import pytest

import occlusion_cases as oc
import occlusion_restatement as occ
from helpers import run_oracle
from test_occlusion_host import _float64_decision


def _terms(c):
    return occ.occlusion_terms(c["boxes"], c["pv"], occ.pyramid_levels(c["depth"]), c["width"], c["height"])


def _labelled(c):
    return np.array([l["index"] for l in c["labels"]], np.int64)


@pytest.mark.parametrize("name", oc.NAMES)
def test_every_label_is_what_the_restatement_computes(name, oracle_mod):
    c = oc.case(name)
    assert oc.verify(c) == []
    want = run_oracle(oracle_mod, oc.scene_of(c))
    boxes = np.asarray(want["world_aabb"], np.float32).reshape(-1, 6)
    assert boxes.view(np.uint32).tobytes() == c["boxes"].view(np.uint32).tobytes(), "the oracle's world boxes are the catalogue's"
    assert occ.bits_of(want["visible_bitmap"], c["n"]).all(), "the planes accept every instance"
    assert oc.verify(c, boxes) == []


def test_catalogue_is_deterministic():
    for name in oc.NAMES:
        a, b = oc.case(name), oc._BUILDERS[name]()
        for key in ("depth", "pos", "rot", "scale", "mesh_id", "meshes", "boxes", "pv"):
            assert a[key].tobytes() == b[key].tobytes(), (name, key)
        assert a["labels"] == b["labels"], name


# (class, words of the side): every edge the catalogue is owed, on both sides
SIDES = [
    ("step3", "w == +0"), ("step3", "z == -0"), ("step3", "smallest subnormal"), ("step3", "largest subnormal"), ("step3", "smallest normal"),
    ("step3", "w negative"), ("step3", "w == 1"), ("step3", "w one step negative"), ("step3", "w one step positive"), ("step3", "w == 0"),
    ("step3", "FLT_MAX exactly"), ("step3", "clip.y == +inf"), ("step3", "clip.x == +inf"), ("step3", "clip.x == -inf"), ("step3", "NaN (inf - inf)"),
    ("step3", "third addition only"), ("step3", "stays finite in the third addition"), ("step3", "u is NaN"), ("step3", "both clamps"),
    ("step56", "umax on 40"), ("step56", "umax one float below 40"), ("step56", "umax one float above 40"), ("step56", "vmax on 47"),
    ("step56", "vmax one float below 63"), ("step56", "vmax one float above 63"), ("step56", "u in (-1, 0)"), ("step56", "v in (-1, 0)"),
    ("step56", "umin == 0"), ("step56", "umax == W - 1"), ("step56", "umax == W:"), ("step56", "vmin == 0"), ("step56", "vmax == H - 1"),
    ("step56", "vmax == H:"), ("step56", "left of the image"), ("step56", "right of the image"), ("step56", "above the image"),
    ("step56", "below the image"), ("step56", "far outside"), ("step56", "reads the top rows"), ("step56", "reads the bottom rows"),
    ("step7", "the whole image"), ("step7", "four times the same texel"), ("step7", "x alone decides"), ("step7", "y alone decides"),
    ("step7", "x and y decide"), ("step7", "width 4 aligned"), ("step7", "width 4 one pixel on"), ("step7", "height 4 one pixel on"),
    ("step8", "the maximum in texel (0, 0)"), ("step8", "the maximum in texel (1, 0)"), ("step8", "the maximum in texel (0, 1)"),
    ("step8", "the maximum in texel (1, 1)"), ("step8", "the last column and the last row"), ("step8", "the last column, every row"),
    ("step8", "the last row, every column"),
    ("step9", "zmin == d"), ("step9", "zmin the float above"), ("step9", "zmin the float below"), ("step9", "d == 1.0, zmin 2.0"),
    ("step9", "d the float below 1.0, zmin 1.0"), ("step9", "d the float below 1.0, zmin == d"), ("step9", "d negative"), ("step9", "d == +0, zmin -0"),
    ("step9", "d == +0, zmin the smallest subnormal"), ("step9", "zmin below d, zmax above"), ("step9", "d == 1.0 (65535)"),
    ("step9", "d == 65534 / 65535, zmin == d"), ("step9", "d == 65534 / 65535, zmin the float above"), ("step9", "d == +0 (0), zmin == d"),
    ("step9", "d == 1 / 65535, zmin the float below"), ("step9", "d == 1 / 65535, zmin the float above"),
] + [("step9", f"zmin from corner {j} alone") for j in range(8)] + [("step9", f"zmin from corner {j}, every corner behind") for j in range(8)]


def test_every_class_is_present_on_both_sides():
    seen = {(l["cls"], l["side"]) for name in oc.NAMES for l in oc.case(name)["labels"]}
    for cls, words in SIDES:
        assert any(c == cls and words in side for c, side in seen), (cls, words)
    for cls in oc.CLASSES:  # both answers in every class; ties and their neighbours in every geometric one
        answers = set()
        for name in oc.NAMES:
            c = oc.case(name)
            t = _terms(c)
            answers |= {bool(t["occluded"][l["index"]]) for l in c["labels"] if l["cls"] == cls}
        assert answers == {False, True}, cls
    for name in oc.NAMES:
        c = oc.case(name)
        assert c["name"] == name and c["n"] >= 3 * oc.TILE and 900 <= c["n"] <= 1300
        assert all((l["side"] + "/").count("/") <= 2 for l in c["labels"])


def _reachable_levels(extent_x, extent_y):
    def per_axis(extent):
        ks = set()
        for p0 in range(extent):
            for p1 in range(p0, extent):
                k = 0
                while (p1 >> (k + 1)) - (p0 >> (k + 1)) > 1:
                    k += 1
                ks.add(k)
        return ks

    return {max(a, b) for a in per_axis(extent_x) for b in per_axis(extent_y)}


@pytest.mark.parametrize("name", [n for n in oc.NAMES if n.startswith("ortho")])
def test_every_reachable_level_and_every_ragged_edge_is_read(name):
    """Step 7 on every level a rectangle of this image can select (the 1 x 1 top is one of them only when level 0 has at
    most two texels a side), and step 8 on the last column and the last row of every such level."""
    c = oc.case(name)
    t = _terms(c)
    idx = _labelled(c)
    sizes = [l.shape[::-1] for l in occ.pyramid_levels(c["depth"])]
    reachable = _reachable_levels(c["width"], c["height"])
    assert set(t["k"][idx]) == reachable, (name, sorted(reachable))
    assert (len(sizes) - 1 in reachable) == (sizes[0][0] <= 2 and sizes[0][1] <= 2), name
    for k in reachable:
        at = idx[t["k"][idx] == k]
        lw, lh = sizes[k]
        assert ((t["x1"][at] >> (k + 1)) == lw - 1).any() and ((t["y1"][at] >> (k + 1)) == lh - 1).any(), (name, k)
        assert ((t["x0"][at] >> (k + 1)) == 0).any() and ((t["y0"][at] >> (k + 1)) == 0).any(), (name, k)
    if "texel" in name:  # every level a rectangle can select here: kept with a texel difference of 1, sent on with 2
        sides = {l["side"] for l in c["labels"] if l["cls"] == "step7"}
        for k in sorted(reachable):
            for axis in ("x alone decides", "y alone decides", "x and y decide"):
                assert any(f"{axis}: level {k} kept" in s for s in sides), (axis, k)
                assert k == 0 or any(f"{axis}: level {k} sent" in s for s in sides), (axis, k)


def test_layout_puts_every_class_on_the_lanes_and_tile_ends():
    kinds_seen = {cls: set() for cls in oc.CLASSES}
    for name in oc.NAMES:
        c = oc.case(name)
        n = c["n"]
        t = _terms(c)
        idx = _labelled(c)
        assert len(set(idx)) == len(idx)
        by_class = {}
        for l in c["labels"]:
            i = l["index"]
            kinds = set()
            if i % oc.TILE == 0:
                kinds.add("first of a tile")
            if i % oc.TILE == oc.TILE - 1 or i == n - 1:
                kinds.add("last of a tile")
            if i % 64 == 0:
                kinds.add("lane 0")
            if i % 64 == 63:
                kinds.add("lane 63")
            by_class.setdefault(l["cls"], []).append(kinds)
        for cls, kinds in by_class.items():
            got = set().union(*kinds)
            kinds_seen[cls] |= got
            if len(kinds) >= 4:
                assert got == {"first of a tile", "last of a tile", "lane 0", "lane 63"}, (name, cls, got)
        # the ordinary boxes around them keep both bitmaps from being all 0 or all 1, tile by tile
        filler = np.ones(n, bool)
        filler[idx] = False
        for first in range(0, n, oc.TILE):
            tile = slice(first, min(first + oc.TILE, n))
            occluded = t["occluded"][tile][filler[tile]]
            assert 0 < occluded.sum() < len(occluded), (name, first)
    for cls, got in kinds_seen.items():
        assert len(got) == 4, (cls, got)


@pytest.mark.parametrize("mutant", oc.MUTANTS)
def test_the_catalogue_tells_the_mistake_apart(mutant):
    """The mistake changes the occluded bit of a LABELLED instance in an f32 scene and in a u16 scene (u16 / 65536: a u16
    scene). Truncation for floor changes nothing anywhere: the clamp at 0 hides the only interval where the two differ."""
    flipped = {"f32": [], "u16": []}
    for name in oc.NAMES:
        c = oc.case(name)
        right = oc.mutant_occluded(c["boxes"], c["pv"], c["depth"])
        assert np.array_equal(right, _terms(c)["occluded"]), name   # the copy without a mistake IS the restatement
        wrong = oc.mutant_occluded(c["boxes"], c["pv"], c["depth"], mutant)
        idx = _labelled(c)
        flipped[c["fmt"]] += [oc.describe(c, i) for i in idx[right[idx] != wrong[idx]]]
        if mutant in oc.EQUIVALENT_MUTANTS:
            assert np.array_equal(right, wrong), name
    if mutant in oc.EQUIVALENT_MUTANTS:
        t = _terms(oc.case("ortho64_f32_texel0"))
        assert ((t["umin"] > -1) & (t["umin"] < 0)).any() and ((t["vmin"] > -1) & (t["vmin"] < 0)).any()  # (the interval is there)
        return
    assert flipped["u16"], mutant
    if mutant != "u16_65536":
        assert flipped["f32"], mutant


@pytest.mark.parametrize("name", oc.NAMES)
def test_float64_agrees_where_it_decides_and_calls_every_tie_undecided(name):
    c = oc.case(name)
    levels = occ.pyramid_levels(c["depth"])
    t = occ.occlusion_terms(c["boxes"], c["pv"], levels, c["width"], c["height"])
    clips = oc.corner_clips(c["boxes"], c["pv"])
    usable = np.isfinite(clips).all(axis=(1, 2)) & (clips[:, :, 3] != 0).all(axis=1)  # (a w of 0 or a non-finite clip: margin 0)
    want, margin = np.zeros(c["n"], bool), np.zeros(c["n"])
    with np.errstate(all="ignore"):
        want[usable], margin[usable] = _float64_decision(c["boxes"][usable].astype(np.float64), c["pv"], levels, c["width"], c["height"])
    decided = margin > 1e-3
    assert np.array_equal(t["occluded"][decided], want[decided]), [oc.describe(c, i) for i in np.nonzero(decided & (t["occluded"] != want))[0][:8]]
    for l in c["labels"]:
        if l["check"].get("zmin_minus_d") is not None or abs(float(l["check"].get("w_is", 1.0))) < 1e-3:
            assert not decided[l["index"]], oc.describe(c, l["index"])
    if name.startswith("ortho") and c["width"] > 1:
        assert decided.sum() > 100, (name, int(decided.sum()))  # the ordinary boxes


# ---- the depth pyramid's shapes ----

def test_every_structural_class_of_the_pyramid_kernel_has_a_shape():
    shapes = oc.pyramid_shapes()
    assert len(set(shapes)) == len(shapes)
    have = {}
    for s in shapes:
        for cls in oc.pyramid_structure(*s):
            have.setdefault(cls, []).append(s)
    for cls in oc.PYRAMID_CLASSES:
        assert have.get(cls), cls
    first = lambda cls: have[cls][0][:2]
    assert (4096, 4096) in [s[:2] for s in have["top in LDS, level 5 exactly 4096 texels"]]
    assert {(4097, 4096), (4096, 4097)} <= {s[:2] for s in have["top through memory by the first clause"]}
    assert first("top through memory by the second clause alone") == (1088, 15360)
    assert {(63, 1), (64, 64)} <= {s[:2] for s in have["one block, early return"]} and (65, 1) in [s[:2] for s in have["several blocks, the last one finishes"]]
    assert max(w * h for w, h, _, _ in shapes) == 4097 * 4096
    for w, h, fmt, pitch in shapes:
        assert pitch >= w
