"""Hand-written lists for the visible-cluster list in two phases (include/mi_instance_pipeline.h, mip_list_clusters_phase): the
nine scenes of tests/cluster_phase_cases.py — its geometry, boxes, pyramids and planes, described there — with the ENTRIES of
both phases, their four stats words and the record written down by hand, none of them taken from a restatement. An entry is
(instance = base + i, first_index = the level's offset + 192 c, vertex_offset, index_count = 192 or 3 x the triangles of a
short last cluster). Every scene is meant to be run twice: SECOND at base 0 into a buffer of its own, and SECOND at base =
FIRST's count behind FIRST's entries (appended)."""
import numpy as np

import cluster_phase_cases as pc
from renderer_amd.pipeline import CLUSTER_ENTRY_DTYPE


def _entries(rows):
    return np.array(rows, CLUSTER_ENTRY_DTYPE) if rows else np.zeros(0, CLUSTER_ENTRY_DTYPE)


def _want(first_rows, first_stats, record, second_rows, second_stats, new="clear"):
    """first / second: dict(entries, stats — survivors, W, members, candidates); record: the uint32 words; new_depth: SECOND's image."""
    return dict(first=dict(entries=_entries(first_rows), stats=np.array(first_stats, np.uint32)), record=record,
                second=dict(entries=_entries(second_rows), stats=np.array(second_stats, np.uint32)), new_depth=pc._depth(new))


def cases():
    """[(name, scene, want)]."""
    out = []
    ones = (1 << 64) - 1

    # HVV: item 0 is the candidate; FIRST lists clusters 1 and 2, SECOND cluster 0
    s = pc.scene(["HVV"], [0], base=7)
    out.append(("a candidate at c = 0", s, _want([(7, 192, 1, 192), (7, 384, 1, 192)], (2, 3, 1, 1), pc._record(3, 1, 1, [0b001]), [(7, 0, 1, 192)], (1, 3, 1, 1))))

    # VVH, the last cluster of 5 triangles: SECOND's one entry has 15 indices at 384
    s = pc.scene(["VVH"], [0], last=5, base=7)
    out.append(("a candidate at c = C - 1, short", s,
                _want([(7, 0, 1, 192), (7, 192, 1, 192)], (2, 3, 1, 1), pc._record(3, 1, 1, [0b100]), [(7, 384, 1, 15)], (1, 3, 1, 1))))

    # VHV: FIRST lists clusters 0 and 2, SECOND cluster 1; the base wraps: instance = base + 0
    s = pc.scene(["VHV"], [0], base=0xFFFFFFFF)
    out.append(("c = 1 of C = 3", s, _want([(0xFFFFFFFF, 0, 1, 192), (0xFFFFFFFF, 384, 1, 192)], (2, 3, 1, 1), pc._record(3, 1, 1, [0b010]),
                                          [(0xFFFFFFFF, 192, 1, 192)], (1, 3, 1, 1))))

    # VH | HV: the last item of instance 0 and the first of instance 1 are candidates. mesh 1: indices from 384, vertices from 7
    s = pc.scene(["VH", "HV"], [0, 1], base=9)
    out.append(("two instances meet", s, _want([(9, 0, 1, 192), (10, 576, 7, 192)], (2, 4, 2, 2), pc._record(4, 2, 2, [0b0110]),
                                              [(9, 192, 1, 192), (10, 384, 7, 192)], (2, 4, 2, 2))))

    # items 63 and 64 of one instance of 66 clusters: two record words, two entries next to each other in SECOND's list
    s = pc.scene(["V" * 63 + "HH" + "V"], [0], base=1)
    out.append(("a run across items 63 | 64", s,
                _want([(1, 192 * c, 1, 192) for c in range(63)] + [(1, 192 * 65, 1, 192)], (64, 66, 1, 2), pc._record(66, 1, 2, [1 << 63, 1]),
                      [(1, 192 * 63, 1, 192), (1, 192 * 64, 1, 192)], (2, 66, 1, 2))))

    # items 0..63 are candidates, 64..127 are not: a full word, then a zero word
    s = pc.scene(["H" * 64 + "V" * 64], [0], base=2)
    out.append(("a full word before a zero word", s,
                _want([(2, 192 * c, 1, 192) for c in range(64, 128)], (64, 128, 1, 64), pc._record(128, 1, 64, [ones, 0]),
                      [(2, 192 * c, 1, 192) for c in range(64)], (64, 128, 1, 64))))

    # every item of three instances is a candidate (T = 67: the second cluster holds 3 triangles): FIRST lists nothing
    s = pc.scene(["HH"], [0, 0, 0], last=3, base=3)
    out.append(("every item", s, _want([], (0, 6, 3, 6), pc._record(6, 3, 6, [0b111111]),
                                       [(3, 0, 1, 192), (3, 192, 1, 9), (4, 0, 1, 192), (4, 192, 1, 9), (5, 0, 1, 192), (5, 192, 1, 9)], (6, 6, 3, 6))))

    # no candidates: the outside cluster is culled by the planes, not occluded. mesh 1: indices from 576, vertices from 10
    s = pc.scene(["VOV", "VV"], [0, 1], base=4)
    out.append(("none", s, _want([(4, 0, 1, 192), (4, 384, 1, 192), (5, 576, 10, 192), (5, 768, 10, 192)], (4, 5, 2, 0), pc._record(5, 2, 0, [0]), [], (0, 5, 2, 0))))

    # three candidates, the middle one still hidden by the new (quadrant) pyramid; the last cluster holds 7 triangles
    s = pc.scene(["HSH"], [0], last=7, base=5)
    out.append(("a still-hidden candidate between two visible ones", s,
                _want([], (0, 3, 1, 3), pc._record(3, 1, 3, [0b111]), [(5, 0, 1, 192), (5, 384, 1, 21)], (2, 3, 1, 3), new="quadrant")))
    return out
