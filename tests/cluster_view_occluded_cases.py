"""Hand-written scenes for mip_list_clusters_views_occluded (include/mi_instance_pipeline.h) on the LADDER geometry of
tests/cluster_cases.py under the box frusta A, B, C, D of tests/cluster_view_cases.py, with depth images and projections under
which every number of the occlusion test is exact:

  P    clip = (x / 2048, y / 8, 0.5, 1): on a 64 x 32 image the INSIDE triangle's box ([0,1] x [0,1] at the origin) lands in
       column 32, the OUTSIDE one (x + 1024) in column 48, rows 14 .. 16, at depth 0.5. On a 32 x 16 image: columns 16 and 24.
  P2   clip = ((x - 1024) / 2048, y / 8, 0.5, 1): INSIDE in column 16, OUTSIDE in column 32.
An instance a few units away from the origin stays in the same pair of columns (level 0 of a pyramid is 2 x 2 texels).

The images are tests/test_cluster_phase_restatement.wall_depth's walls — 0.0 (the near plane: whatever lies behind is hidden)
over 32 of 64 columns from `first_column` on, 1.0 (nothing) elsewhere:

  "in"       P  under the wall at 16 (columns 16 .. 47): hides the INSIDE clusters, shows the OUTSIDE ones
  "out"      P2 under the wall at 32 (columns 32 .. 63): hides the OUTSIDE clusters, shows the INSIDE ones
  "all"      P  under the wall at 32: hides both
  "none"     P  under the wall at 0 (columns 0 .. 31): a pyramid that hides nothing
  "cleared"  P  under an image of 1.0: nothing hidden
  "small in" P  under a 32 x 16 image with 0.0 over columns 16 .. 23: hides INSIDE, shows OUTSIDE — other extents
  None       no pyramid: the planes alone
"""
import numpy as np

import cluster_cases as cc
import cluster_view_cases as cvc
import cluster_view_list_cases as cvlc
import occlusion_restatement as orr
from renderer_amd.pipeline import CLUSTER_ENTRY_DTYPE

F = np.float32
# column-major storage: four floats per column
P = np.array([1 / 2048, 0, 0, 0, 0, 1 / 8, 0, 0, 0, 0, 0, 0, 0, 0, 0.5, 1], F)
P2 = np.array([1 / 2048, 0, 0, 0, 0, 1 / 8, 0, 0, 0, 0, 0, 0, -0.5, 0, 0.5, 1], F)


def wall(first_column, width=64, height=32, columns=32):
    """test_cluster_phase_restatement.wall_depth for the default extents; first_column None: a cleared image."""
    depth = np.ones((height, width), F)
    if first_column is not None:
        depth[:, first_column: first_column + columns] = 0.0
    return depth


OCCLUSIONS = {"in": (P, wall(16)), "out": (P2, wall(32)), "all": (P, wall(32)), "none": (P, wall(0)), "cleared": (P, wall(None)),
              "small in": (P, wall(16, 32, 16, 8))}
# which clusters a kind hides: (INSIDE, OUTSIDE)
HIDES = {None: (False, False), "in": (True, False), "out": (False, True), "all": (True, True), "none": (False, False), "cleared": (False, False),
         "small in": (True, False)}
SEES = {"A": (True, False), "B": (False, True), "C": (True, True), "D": (False, False)}
_KIND_OF = {v: k for k, v in SEES.items()}


def occlusion(kind):
    """What the restatement takes for an occlusion kind: dict(pv, levels, width, height, depth), or None."""
    if kind is None:
        return None
    pv, depth = OCCLUSIONS[kind]
    return dict(pv=pv, levels=orr.pyramid_levels(depth), width=depth.shape[1], height=depth.shape[0], depth=depth)


def _rows(rows):
    return np.array(rows, CLUSTER_ENTRY_DTYPE) if rows else np.zeros(0, CLUSTER_ENTRY_DTYPE)


def _clusters(base, which):
    return _rows([(base, 192 * c, 0, 192) for c in which])


def cases():
    """[(name, scene, views, kinds, want)]: views as cluster_view_cases.cases() gives them, kinds — one occlusion kind per
    view —, want = dict(entries — per view every entry in order; stats — W, members, survivors per view; hidden — per view).
    Every answer is typed by hand from the table in this module's docstring."""
    out = []
    # ONE instance of "1010101" (C = 7; INSIDE clusters 0, 2, 4, 6, OUTSIDE 1, 3, 5) at the origin.
    s = cc._scene([cc._level("1010101", 448)], [(0, (0, 0, 0), 1.0)])
    # view 0: sees all, the wall hides the INSIDE four: 1, 3, 5 are left, 4 hidden. View 1, no pyramid: all seven. View 2 sees
    # the INSIDE four and the wall hides them all. View 3: a pyramid that hides nothing. View 4 sees the OUTSIDE three, all hidden.
    want = dict(entries=[_clusters(7, [1, 3, 5]), _clusters(100, range(7)), _rows([]), _clusters(0x80000000, range(7)), _rows([])],
                stats=np.array([7, 1, 3, 7, 0, 7, 0], np.uint32), hidden=np.array([4, 0, 4, 0, 3], np.uint32))
    out.append(("a wall over the inside clusters", s, cvc._views([cvc.C, cvc.C, cvc.A, cvc.C, cvc.B], bases=[7, 100, 5, 0x80000000, 9]),
                ["in", None, "in", "none", "all"], want))
    # the same wall in ONE view of three that are otherwise the same: only that view loses clusters
    want = dict(entries=[_clusters(1, range(7)), _clusters(2, [1, 3, 5]), _clusters(3, range(7))], stats=np.array([7, 1, 7, 3, 7], np.uint32),
                hidden=np.array([0, 4, 0], np.uint32))
    out.append(("hidden in the middle view only", s, cvc._views([cvc.C, cvc.C, cvc.C], bases=[1, 2, 3]), [None, "in", None], want))
    # one pyramid (the wall at 32) under two projections: P puts both triangles behind it, P2 the OUTSIDE one alone
    want = dict(entries=[_rows([]), _clusters(2, [0, 2, 4, 6])], stats=np.array([7, 1, 0, 4], np.uint32), hidden=np.array([7, 3], np.uint32))
    out.append(("one pyramid under two projections", s, cvc._views([cvc.C, cvc.C], bases=[1, 2]), ["all", "out"], want))
    # two images of different extents: 32 x 16 in slot 0 (hides INSIDE), 64 x 32 in slot 1 (hides both)
    want = dict(entries=[_clusters(1, [1, 3, 5]), _rows([])], stats=np.array([7, 1, 3, 0], np.uint32), hidden=np.array([4, 7], np.uint32))
    out.append(("two extents", s, cvc._views([cvc.C, cvc.C], bases=[1, 2]), ["small in", "all"], want))
    # a cleared image: nothing hidden
    want = dict(entries=[_clusters(5, [0, 2, 4, 6]), _clusters(6, range(7))], stats=np.array([7, 1, 4, 7], np.uint32), hidden=np.array([0, 0], np.uint32))
    out.append(("a cleared image", s, cvc._views([cvc.A, cvc.C], bases=[5, 6]), ["cleared", "cleared"], want))
    # "10" at the origin, at (3, 0, 0) and at (0, 3, 0). View 0, with the wall over INSIDE, holds instance 0 alone; view 1, no
    # pyramid, instance 2 alone; instance 1 is in no bitmap. Members {0, 2}: W = 4. View 0: cluster 1 of instance 0 survives,
    # cluster 0 is hidden — instance 2's cluster 0 is behind the wall too, but it is not in view 0: hidden[0] = 1, not 2.
    s3 = cc._scene([cc._level("10", 128)], [(0, (0, 0, 0), 1.0), (0, (3, 0, 0), 1.0), (0, (0, 3, 0), 1.0)])
    want = dict(entries=[_rows([(0, 192, 0, 192)]), _rows([(12, 0, 0, 192), (12, 192, 0, 192)])], stats=np.array([4, 2, 1, 2], np.uint32),
                hidden=np.array([1, 0], np.uint32))
    out.append(("a pyramid never adds or removes a member", s3, cvc._views([cvc.C, cvc.C], bitmaps=[cvc.bits(3, [0]), cvc.bits(3, [2])], bases=[0, 10]),
                ["in", None], want))
    return out


def occluded_ladder(patterns, instance_pattern, specs):
    """cluster_view_list_cases.ladder_views_list under a pyramid per view. specs: per view (frustum — "A", "B", "C" or "D" —,
    occlusion kind, bits — a bool per instance, or None for a NULL bitmap —, base). Returns (scene, views, kinds, want): the
    views carry the frusta as given; want is written down from the patterns: a view's entries are the ladder's list as the
    frustum sees it WITHOUT the clusters its kind hides, hidden[v] the clusters of the view's instances that the frustum sees
    and the kind hides; W and members those of the union of the bits."""
    masks = [np.frombuffer(p.encode(), np.uint8) == ord("1") if isinstance(p, str) else np.asarray(p, bool) for p in patterns]
    inst = np.asarray(instance_pattern, np.int64)
    scene, views, _ = cvlc.ladder_views_list(patterns, instance_pattern, [(f, b, base) for f, _, b, base in specs])
    left = []
    hidden = []
    for f, kind, b, base in specs:
        sees, hides = SEES[f], HIDES[kind]
        after = (sees[0] and not hides[0], sees[1] and not hides[1])
        left.append((_KIND_OF[after], b, base))
        gone = (sees[0] and hides[0], sees[1] and hides[1])
        per_mesh = np.array([int(gone[0]) * int(m.sum()) + int(gone[1]) * int((~m).sum()) for m in masks], np.int64)
        bit = np.ones(len(inst), bool) if b is None else np.asarray(b, bool)
        hidden.append(int(per_mesh[inst[bit]].sum()) if len(inst) else 0)
    _, _, want = cvlc.ladder_views_list(patterns, instance_pattern, left)
    return scene, views, [k for _, k, _, _ in specs], dict(entries=want["entries"], stats=want["stats"], hidden=np.array(hidden, np.uint32))
