"""Hand-written lists for mip_list_clusters_views (include/mi_instance_pipeline.h) on the scenes and views of
tests/cluster_view_cases.py (the LADDER geometry under the box frusta A, B, C, D): per view every entry in order, typed by hand
from the header's ENTRIES rule — {frames[v].first_instance_base + i (wraps), index_offset + 192 c, vertex_offset, 3 x the
cluster's triangles} — and the stats {W, members, survivors per view}. Also the closed form of a ladder under several views for
the structural tests."""
import numpy as np

import cluster_list_cases as clc
import cluster_view_cases as cvc
from renderer_amd.pipeline import CLUSTER_ENTRY_DTYPE


def _rows(rows):
    return np.array(rows, CLUSTER_ENTRY_DTYPE) if rows else np.zeros(0, CLUSTER_ENTRY_DTYPE)


_FOUR = dict(entries=[_rows([(7, 0, 0, 192), (7, 384, 0, 192), (7, 768, 0, 192), (7, 1152, 0, 192)]),          # A: clusters 0, 2, 4, 6
                      _rows([(100, 192, 0, 192), (100, 576, 0, 192), (100, 960, 0, 192)]),                       # B: clusters 1, 3, 5
                      _rows([(0x80000000, 192 * c, 0, 192) for c in range(7)]),                                   # C: all seven (T = 448: the last is whole)
                      _rows([])],                                                                                 # D: none
             stats=[7, 1, 4, 3, 7, 0])

# name -> (per view every entry, stats)
_LISTS = {
    "four views of one ladder": _FOUR,
    "garbage cameras behind view 0": _FOUR,
    # two instances of "11"; bitmaps {0}, {1}, {} and NULL; bases 9, 0xFFFFFFFF (+ 1 wraps to 0), 5, 20
    "bitmaps {0}, {1}, {}, NULL": dict(entries=[_rows([(9, 0, 0, 192), (9, 192, 0, 192)]), _rows([(0, 0, 0, 192), (0, 192, 0, 192)]), _rows([]),
                                                _rows([(20, 0, 0, 192), (20, 192, 0, 192), (21, 0, 0, 192), (21, 192, 0, 192)])],
                                       stats=[4, 2, 2, 2, 0, 4]),
    "an instance in no bitmap": dict(entries=[_rows([(9, 0, 0, 192), (9, 192, 0, 192)]), _rows([(0, 0, 0, 192), (0, 192, 0, 192)]), _rows([])],
                                     stats=[4, 2, 2, 2, 0]),
    # "10" at instances 0 and 2 (1 has no bit): A sees cluster 0 of both, B (bit of instance 2 only, base 10) cluster 1 of instance 2
    "a non-member between two members": dict(entries=[_rows([(0, 0, 0, 192), (2, 0, 0, 192)]), _rows([(12, 192, 0, 192)])], stats=[4, 2, 2, 1]),
    # level 0 (two clusters at index 0) for both views: frames[0].cam_pos is near
    "one level for all views: view 0 near": dict(entries=[_rows([(3, 0, 0, 192), (3, 192, 0, 192)]), _rows([(4, 0, 0, 192), (4, 192, 0, 192)])],
                                                 stats=[2, 1, 2, 2]),
    # level 1 (one cluster at index 384) for both
    "one level for all views: view 0 far": dict(entries=[_rows([(3, 384, 0, 192)]), _rows([(4, 384, 0, 192)])], stats=[1, 1, 1, 1]),
}


def cases():
    """[(name, scene, views, want)]: scene and views are cluster_view_cases.cases()'; want = dict(entries — per view every
    entry in order; stats — W, members, then the surviving clusters per view)."""
    out = []
    for name, s, views, _ in cvc.cases():
        w = _LISTS[name]
        out.append((name, s, views, dict(entries=w["entries"], stats=np.array(w["stats"], np.uint32))))
    assert len(out) == len(_LISTS)
    return out


def ladder_views_list(patterns, instance_pattern, specs):
    """cluster_view_cases.ladder_views with lists in the commands' place: (scene, views, want), want = dict(entries — per view
    cluster_list_cases.ladder_want of the ladders as the view's frustum sees them under the view's bits and base; stats)."""
    scene, views, cmds_want = cvc.ladder_views(patterns, instance_pattern, specs)
    masks = [np.frombuffer(p.encode(), np.uint8) == ord("1") if isinstance(p, str) else np.asarray(p, bool) for p in patterns]
    seen = {"A": masks, "B": [~m for m in masks], "C": [np.ones(len(m), bool) for m in masks], "D": [np.zeros(len(m), bool) for m in masks]}
    entries, survivors = [], []
    for kind, b, base in specs:
        # the closed form of one list over the ladders as the view's frustum sees them: every cluster keeps its place in its level
        e, _ = clc.ladder_want(seen[kind], instance_pattern, base=base, bits=None if b is None else np.asarray(b, bool))
        entries.append(e)
        survivors.append(len(e))
    return scene, views, dict(entries=entries, stats=np.array([int(cmds_want["stats"][0]), int(cmds_want["stats"][1])] + survivors, np.uint32))
