"""numpy restatement of mip_list_clusters_views_occluded (include/mi_instance_pipeline.h), written from the header's text:
mip_list_clusters_views with a depth pyramid per view. MEMBERS, WORK ITEMS and W are cluster_views_restatement's (the union of
the views' bitmaps; a pyramid never changes them), SURVIVES of a view's planes and pyramid is cluster_restatement.survives
masked by the view's bits, the entry fields are cluster_list_restatement.entries_of's and draw_args
cluster_views_list_restatement's: imported and not restated. `hidden` is counted here. Each step can be replaced by a likely
mistake (MUTANTS) so that the tests can show which scene catches it. Not reference behaviour: this file is what the library
is checked against."""
import numpy as np

import cluster_list_restatement as clr
import cluster_restatement as cr
import cluster_views_list_restatement as cvlr
import cluster_views_restatement as cvr
from renderer_amd.pipeline import CLUSTER_ENTRY_DTYPE

ERR_CAPACITY = cvr.ERR_CAPACITY
MUTANTS = ("pv of slot 0", "pyramid of slot 0", "extents of slot 0", "pyramid before the bitmap bit", "hidden counts lanes outside the view",
           "NULL occlusion hides everything", "a pyramid changes the members")


def turned_pv(pv, turn):
    """pv (16 floats, column-major storage) under one of cluster_view_cases.frusta's turns (a, b, c, sx, sz): as a (4, 4) array
    of the storage — row j is column j of the matrix, the coefficients of world coordinate j — rows [a, b, c, 3], row 0 times
    sx, row 2 times sz. Exact: a permutation and sign flips."""
    a, b, c, sx, sz = turn
    t = np.asarray(pv, np.float32).reshape(4, 4)[[a, b, c, 3]].copy()
    t[0] *= sx
    t[2] *= sz
    return np.ascontiguousarray(t.reshape(16))


TURNS = [(0, 1, 2, 1, 1), (2, 1, 0, 1, 1), (0, 1, 2, -1, 1), (2, 1, 0, -1, 1), (0, 2, 1, 1, 1), (0, 1, 2, 1, -1)]   # cluster_view_cases.frusta's


def view_pvs(pv, n_views):
    """View v's pv: `pv` turned as cluster_view_cases.frusta turns the planes of view v."""
    return [turned_pv(pv, TURNS[v % len(TURNS)]) for v in range(n_views)]


def list_clusters_views_occluded(s, boxes, view_planes, bitmaps, occlusions, bases, mode, switch_sq, entry_stride, work_capacity=0, cam_pos=None,
                                 mutant=None):
    """What mip_list_clusters_views_occluded owes for scene s under view v = (view_planes[v], bitmaps[v] — words or None —,
    occlusions[v] — dict(pv, levels, width, height) or None —, bases[v]); cam_pos = frames[0].cam_pos (default: the scene's).
    dict(status; entries — per view the ones written; counts; args — (n_views, 4); stats — 2 + n_views words; hidden — n_views
    words; all_entries; items; survive, passed — per view). mutant: one of MUTANTS, or None for the header's rule."""
    assert mutant is None or mutant in MUTANTS
    n_views = len(view_planes)
    assert len(bitmaps) == len(occlusions) == len(bases) == n_views and 1 <= n_views <= 16 and n_views * int(entry_stride) < 1 << 32
    n = len(np.asarray(s["mesh_id"]).reshape(-1))
    cam = s["cam_pos"] if cam_pos is None else cam_pos
    none = np.zeros(0, CLUSTER_ENTRY_DTYPE)
    zero = np.zeros(n_views, np.uint32)
    stats = np.zeros(2 + n_views, np.uint32)
    if n == 0:                                                    # N = 0
        return dict(status=0, entries=[none] * n_views, counts=zero, args=cvlr.draw_args(zero, entry_stride), stats=stats, hidden=zero.copy(),
                    all_entries=[none] * n_views, items=None, survive=None, passed=None)
    bits = cvr.view_bits(bitmaps, n)
    member_bits = bits
    if mutant == "a pyramid changes the members":                 # a view with a pyramid adds nothing to the union
        member_bits = np.array([b if o is None else np.zeros(n, bool) for b, o in zip(bits, occlusions)], bool).reshape(n_views, n)
    items = cr.work_items(s["pos"], s["scale"], s["mesh_id"], s["meshes"], cam, cvr.union_bitmap(member_bits), mode, switch_sq)
    largest = int(items["table"]["C"].max()) if len(items["table"]["C"]) else 0
    bound = int(work_capacity) if work_capacity else n * largest
    stats[0], stats[1] = items["W"] & 0xFFFFFFFF, items["members"]
    if items["W"] > bound or items["W"] >= 1 << 32:               # WORK OVERFLOW
        return dict(status=ERR_CAPACITY, entries=[none] * n_views, counts=zero, args=cvlr.draw_args(zero, entry_stride), stats=stats, hidden=zero.copy(),
                    all_entries=[none] * n_views, items=items, survive=None, passed=None)
    every, survive, passed, hidden = [], [], [], np.zeros(n_views, np.uint32)
    for v in range(n_views):
        occ = occlusions[v]
        if occ is not None:
            src = occlusions[0] if occlusions[0] is not None else occ
            occ = dict(occ)
            if mutant == "pv of slot 0":
                occ["pv"] = src["pv"]
            if mutant == "pyramid of slot 0":
                occ["levels"] = src["levels"]
            if mutant == "extents of slot 0":
                occ["width"], occ["height"] = src["width"], src["height"]
        in_view = bits[v][items["inst"]]
        # PASSES_v: the view's bit AND the plane test; SURVIVES_v: AND not occluded under the view's pyramid
        by_planes = cr.survives(items, boxes, s["pos"], s["rot"], s["scale"], view_planes[v])
        by_both = by_planes.copy()
        if occ is not None and by_planes.any():                   # survives(..., planes_v, occlusion_v), on the items that can still change
            sub = dict(items, inst=items["inst"][by_planes], box_index=items["box_index"][by_planes])
            by_both[by_planes] = cr.survives(sub, boxes, s["pos"], s["rot"], s["scale"], view_planes[v], occ)
        if occ is None and mutant == "NULL occlusion hides everything":
            by_both = np.zeros_like(by_planes)
        p, sv = by_planes & in_view, by_both & in_view
        if mutant == "pyramid before the bitmap bit":             # the lanes outside the view ran the test too, and were counted
            hidden[v] = int((by_planes & ~by_both).sum())
        elif mutant == "hidden counts lanes outside the view":    # every lane that did not survive
            hidden[v] = int((~sv).sum()) if occ is not None else 0
        else:
            hidden[v] = int((p & ~sv).sum())
        passed.append(p)
        survive.append(sv)
        every.append(clr.entries_of(items, sv, s["meshes"], bases[v]))
    counts = np.array([min(len(e), int(entry_stride)) for e in every], np.uint32)
    stats[2:] = [len(e) for e in every]
    status = ERR_CAPACITY if any(len(e) > int(entry_stride) for e in every) else 0
    return dict(status=status, entries=[e[:c] for e, c in zip(every, counts)], counts=counts, args=cvlr.draw_args(counts, entry_stride), stats=stats,
                hidden=hidden, all_entries=every, items=items, survive=survive, passed=passed)


def fill_outputs(want, n_views, entry_stride, sentinel, pad, args=True, stats=True, hidden=True):
    """The whole output buffers a call leaves behind when every word was `sentinel` before:
    cluster_views_list_restatement.fill_outputs' four, and hidden — n_views + pad words."""
    out = cvlr.fill_outputs(want, n_views, entry_stride, sentinel, pad, args, stats)
    h = np.full(n_views + pad, sentinel, np.uint32)
    if hidden:
        h[:n_views] = want["hidden"]
    out["hidden"] = h
    return out
