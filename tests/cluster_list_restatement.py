"""numpy restatement of mip_list_clusters (include/mi_instance_pipeline.h), written from the header's text: the list of
surviving work items as 16-byte entries, the count, the draw arguments, the stats and both overflow rules. MEMBERS, WORK ITEMS
and SURVIVES are cluster_restatement's (and cluster_cone_restatement's with a cone), imported and not restated. The list is
built the way the header's kernels are described — word members, ranks per 64 work items, tiles — so that each step can be
replaced by a likely mistake (MUTANTS) and the tests can show which scene catches it; from_commands is the other way round:
the cluster-by-cluster expansion of a command list. Not reference behaviour: this file is what the library is checked against."""
import numpy as np

import cluster_cone_restatement as ccr
import cluster_restatement as cr
from renderer_amd.pipeline import CLUSTER_ENTRY_DTYPE

F = np.float32
ERR_CAPACITY = cr.ERR_CAPACITY
DRAW_VERTICES = 192      # draw_args[0]: 3 x MIP_CLUSTER_TRIANGLES
LIST_TILE_WORDS = 256    # kClusterListTileWords: a choice of the library's the result does not depend on
MUTANTS = ("lanes_below inclusive", "tile prefix dropped", "word rank of the previous tile", "index_count always 192", "base not added",
           "base not wrapped", "word_member one low", "word_member one high", "inactive lane writes", "entry at capacity written")


def entries_of(items, survive, meshes, first_instance_base=0):
    """One entry per surviving work item, in (i, c) order: the header's ENTRIES, vectorised."""
    sel = np.nonzero(np.asarray(survive, bool))[0]
    t = items["table"]
    i, c = items["inst"][sel], items["cluster"][sel]
    b = items["bucket"][i] if len(sel) else np.zeros(0, np.int64)
    k, l = t["mesh"][b], t["lod"][b]
    out = np.zeros(len(sel), CLUSTER_ENTRY_DTYPE)
    out["instance"] = ((i + int(first_instance_base)) & 0xFFFFFFFF).astype(np.uint32)
    out["first_index"] = ((meshes["index_offset"][k, l].astype(np.int64) + 192 * c) & 0xFFFFFFFF).astype(np.uint32)
    out["vertex_offset"] = meshes["vertex_offset"][k]
    out["index_count"] = 3 * np.minimum(t["T"][b] - 64 * c, 64)
    return out


def word_members(member_first, w):
    """word_member[k] for k < ceil(W / 64): the member m with member_first[m] <= 64 k < member_first[m + 1]."""
    return np.searchsorted(np.asarray(member_first, np.int64), 64 * np.arange((w + 63) // 64, dtype=np.int64), side="right") - 1


def entries_by_steps(items, survive, meshes, first_instance_base, entry_capacity, mutant=None, tile_words=LIST_TILE_WORDS):
    """The list as the kernels build it, word by word: (buffer of entry_capacity + 2 entries — unwritten ones stay zero with
    index_count 0xFFFFFFFF — and the count). mutant: one of MUTANTS, or None for the header's rule."""
    assert mutant is None or mutant in MUTANTS
    w = items["W"]
    t = items["table"]
    survive = np.asarray(survive, bool)
    inst_of_member = np.nonzero(items["member"])[0]
    sizes = t["C"][items["bucket"][inst_of_member]]
    member_first = np.concatenate([np.cumsum(sizes) - sizes, [w]]).astype(np.int64)
    wm = word_members(member_first[:-1], w)
    n_words = (w + 63) // 64
    padded = np.zeros(n_words * 64, bool)
    padded[:w] = survive
    if mutant == "inactive lane writes" and w % 64:
        padded[w:] = True                                        # the lanes at or above W are not masked out
    per_word = padded.reshape(n_words, 64).sum(axis=1)
    tile = np.arange(n_words) // tile_words
    tile_total = np.bincount(tile, per_word, minlength=(n_words + tile_words - 1) // tile_words).astype(np.int64)
    tile_prefix = np.cumsum(tile_total) - tile_total
    word_rank = np.cumsum(per_word) - per_word - tile_prefix[tile] if n_words else np.zeros(0, np.int64)
    buf = np.zeros(int(entry_capacity) + 2, CLUSTER_ENTRY_DTYPE)
    buf["index_count"] = 0xFFFFFFFF
    base = int(first_instance_base)
    for k in range(n_words):
        if per_word[k] == 0:
            continue
        m0 = int(wm[k]) + {"word_member one low": -1, "word_member one high": 1}.get(mutant, 0)
        m0 = min(max(m0, 0), len(inst_of_member) - 1)
        before = int(word_rank[k])
        if mutant == "word rank of the previous tile" and tile[k] > 0:
            before = int(word_rank[k - tile_words])
        if mutant != "tile prefix dropped":
            before += int(tile_prefix[tile[k]])
        bits = padded[64 * k: 64 * k + 64]
        for lane in np.nonzero(bits)[0]:
            item = 64 * k + int(lane) if 64 * k + int(lane) < w else 64 * k   # (at or above W only under the mutant: it locates the word's first item)
            rank = before + int(bits[:lane + (1 if mutant == "lanes_below inclusive" else 0)].sum())
            if rank > int(entry_capacity) or (rank == int(entry_capacity) and mutant != "entry at capacity written") or rank >= len(buf):
                continue
            # the lane's member: the last of the 64 entries behind m0 whose first item is <= item (the six shuffles)
            window = member_first[m0: min(m0 + 64, len(inst_of_member))]
            j = max(int(np.searchsorted(window, item, side="right")) - 1, 0)
            i, c = int(inst_of_member[m0 + j]), item - int(window[j])
            b = int(items["bucket"][i])
            mesh, lod = int(t["mesh"][b]), int(t["lod"][b])
            instance = i if mutant == "base not added" else i + base
            buf[rank] = (instance & 0xFFFFFFFF if mutant != "base not wrapped" else min(instance, 0xFFFFFFFF),
                         (int(meshes["index_offset"][mesh, lod]) + 192 * c) & 0xFFFFFFFF, int(meshes["vertex_offset"][mesh]),
                         192 if mutant == "index_count always 192" else 3 * min(int(t["T"][b]) - 64 * c, 64))
    return buf, min(int(padded.sum()) if mutant == "inactive lane writes" else int(survive.sum()), int(entry_capacity))


def from_commands(cmds, meshes):
    """The expansion of a command list of mip_cull_clusters into entries: a command of a run of r clusters becomes r entries,
    192 indices apart, the last one with what is left of indexCount. `meshes` is not read: a command carries all an entry holds."""
    cmds = np.asarray(cmds)
    r = (cmds["indexCount"].astype(np.int64) + 191) // 192
    which = np.repeat(np.arange(len(cmds)), r)
    j = np.arange(int(r.sum()), dtype=np.int64) - np.repeat(np.cumsum(r) - r, r)
    out = np.zeros(len(which), CLUSTER_ENTRY_DTYPE)
    out["instance"] = cmds["firstInstance"][which]
    out["first_index"] = ((cmds["firstIndex"][which].astype(np.int64) + 192 * j) & 0xFFFFFFFF).astype(np.uint32)
    out["vertex_offset"] = cmds["vertexOffset"][which]
    out["index_count"] = np.minimum(cmds["indexCount"][which].astype(np.int64) - 192 * j, 192)
    return out


def list_clusters(s, boxes, visible_bitmap, mode, switch_sq, entry_capacity, work_capacity=0, first_instance_base=0, occlusion=None, cone=None):
    """What mip_list_clusters owes for scene s: dict(status, entries — the ones written, count — entry_count, args — draw_args,
    stats — {survivors, W, members}, all_entries, items, survive). cone: None, or dict(cones, eye, facing) for SURVIVES of
    mip_cull_clusters_cone."""
    if cone is None:
        plain = cr.cull_clusters(s, boxes, visible_bitmap, mode, switch_sq, 1 << 40, work_capacity, first_instance_base, occlusion)
    else:
        plain = ccr.cull_clusters_cone(s, boxes, cone["cones"], cone["eye"], cone["facing"], visible_bitmap, mode, switch_sq, 1 << 40, work_capacity,
                                       first_instance_base, occlusion)
    items = plain["items"]
    none = np.zeros(0, CLUSTER_ENTRY_DTYPE)
    if len(np.asarray(s["mesh_id"]).reshape(-1)) == 0:            # N = 0: a zero count, {192, 0, 0, 0}, zero stats
        return dict(status=0, entries=none, count=0, args=np.array([DRAW_VERTICES, 0, 0, 0], np.uint32), stats=np.zeros(3, np.uint32), all_entries=none,
                    items=items, survive=np.zeros(0, bool))
    if plain["status"] == ERR_CAPACITY and plain["survive"] is None:   # WORK OVERFLOW
        return dict(status=ERR_CAPACITY, entries=none, count=0, args=np.array([DRAW_VERTICES, 0, 0, 0], np.uint32),
                    stats=np.array([0, items["W"] & 0xFFFFFFFF, items["members"]], np.uint32), all_entries=none, items=items, survive=None)
    sv = plain["survive"]
    entries = entries_of(items, sv, s["meshes"], first_instance_base)
    count = min(len(entries), int(entry_capacity))
    return dict(status=ERR_CAPACITY if len(entries) > int(entry_capacity) else 0, entries=entries[:count], count=count,
                args=np.array([DRAW_VERTICES, count, 0, 0], np.uint32), stats=np.array([len(entries), items["W"], items["members"]], np.uint32),
                all_entries=entries, items=items, survive=sv, plain=plain)
