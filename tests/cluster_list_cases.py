"""Hand-written answers of mip_list_clusters (include/mi_instance_pipeline.h) for the ladder scenes of cluster_cases.py: the
scenes are cluster_cases', imported; the lists below are typed in from the survive patterns those scenes are built from, one
entry (instance, first_index, vertex_offset, index_count) per '1' of a pattern, by the header's ENTRIES rule — not derived
from cluster_cases' commands. stats = (survivors, W, members)."""
import numpy as np

import cluster_cases as cc
from renderer_amd.pipeline import CLUSTER_ENTRY_DTYPE

WRAP = 0xFFFFFFFF
LEVEL = 24960            # the indices of one 130-cluster level of "single survivors"

_LISTS = {
    # "1111", T = 200: three whole clusters and the last with 200 - 192 = 8 triangles; base 7
    "all survive": ([(7, 0, 0, 192), (7, 192, 0, 192), (7, 384, 0, 192), (7, 576, 0, 24)], (4, 4, 1)),
    # "0000"
    "none survives": ([], (0, 4, 1)),
    # "1010101": c = 0, 2, 4, 6; the base 0xFFFFFFFF + instance 0 does not wrap yet
    "alternating": ([(WRAP, 0, 0, 192), (WRAP, 384, 0, 192), (WRAP, 768, 0, 192), (WRAP, 1152, 0, 192)], (4, 7, 1)),
    # one '1' at c = 0 / 63 / 64 / 129 of mesh 0 / 1 / 2 / 3; base 100
    "single survivors": ([(100, 0, 0, 192), (101, LEVEL + 192 * 63, 0, 192), (102, 2 * LEVEL + 192 * 64, 0, 192), (103, 3 * LEVEL + 192 * 129, 0, 192)],
                         (4, 520, 4)),
    # T = 129: "111" — the third cluster holds one triangle; "001" in the level behind it (387 indices further)
    "short last cluster": ([(0, 0, 0, 192), (0, 192, 0, 192), (0, 384, 0, 3), (1, 387 + 384, 0, 3)], (4, 6, 2)),
    # T = 65 twice ("11": 64 triangles and one), levels at 0 and 196; the instance in between draws the level without a triangle
    "index tails": ([(5, 0, 0, 192), (5, 192, 0, 3), (7, 196, 0, 192), (7, 196 + 192, 0, 3)], (4, 4, 2)),
    # "11" drawn by two instances; base 9
    "two instances": ([(9, 0, 0, 192), (9, 192, 0, 192), (10, 0, 0, 192), (10, 192, 0, 192)], (4, 4, 2)),
    # the tangent cluster survives, the one a float further out does not
    "tangent": ([(0, 0, 0, 192)], (1, 2, 1)),
    # the NaN cluster survives, the outside cluster behind it does not
    "NaN cluster": ([(0, 0, 0, 192)], (1, 2, 1)),
}


def cases():
    """[(name, scene, want)]: want = dict(entries — every entry, in order; stats — survivors, W, members)."""
    out = []
    for name, s, _ in cc.cases():
        rows, stats = _LISTS[name]
        out.append((name, s, dict(entries=np.array(rows, CLUSTER_ENTRY_DTYPE) if rows else np.zeros(0, CLUSTER_ENTRY_DTYPE), stats=np.array(stats, np.uint32))))
    assert len(out) == len(_LISTS)
    return out


def ladder_want(patterns, instance_pattern, base=0, bits=None):
    """The closed form of the list of cluster_cases.ladder_scene(patterns, instance_pattern, base, bits) — whole clusters only,
    mesh k's level behind the levels before it: (entries, stats)."""
    masks = [np.frombuffer(p.encode(), np.uint8) == ord("1") if isinstance(p, str) else np.asarray(p, bool) for p in patterns]
    sizes = np.array([len(m) for m in masks], np.int64)
    offset = np.cumsum(192 * sizes) - 192 * sizes
    inst = np.asarray(instance_pattern, np.int64)
    member = sizes[inst] > 0
    if bits is not None:
        member &= np.asarray(bits, bool)
    who = np.nonzero(member)[0]
    per_mesh = [np.nonzero(m)[0] for m in masks]
    counts = np.array([len(per_mesh[k]) for k in inst[who]], np.int64)
    entries = np.zeros(int(counts.sum()), CLUSTER_ENTRY_DTYPE)
    if len(entries):
        entries["instance"] = ((np.repeat(who, counts) + int(base)) & WRAP).astype(np.uint32)
        entries["first_index"] = np.concatenate([offset[k] + 192 * per_mesh[k] for k in inst[who]])
        entries["index_count"] = 192
    return entries, np.array([len(entries), int(sizes[inst[who]].sum()), len(who)], np.uint32)
