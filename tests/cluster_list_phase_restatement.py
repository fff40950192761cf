"""numpy restatement of mip_list_clusters_phase (include/mi_instance_pipeline.h), written from the header's text: FIRST — one
entry per work item with SURVIVES and mip_cull_clusters_phase's record —, SECOND — one entry per work item with SURVIVES2 —,
the entry base b, the room behind it, the draw arguments {192, count, 0, b}, the four stats words, both overflow rules, the
record that is not the call's and N = 0. MEMBERS, WORK ITEMS, SURVIVES, SURVIVES2 and the record are cluster_phase_restatement's,
the entries cluster_list_restatement's: imported, not restated. by_steps is the same call the way the header's kernels are
described — survive words, ranks per word, tiles, a base and a room — so that each step can be replaced by a likely mistake
(MUTANTS) and the tests can show which scene catches it. Not reference behaviour: this file is what the library is checked
against."""
import numpy as np

import cluster_list_restatement as clr
import cluster_phase_restatement as pr
import numpy_restatement as nr
from renderer_amd.pipeline import CLUSTER_ENTRY_DTYPE

ERR_CAPACITY = pr.ERR_CAPACITY
ERR_DEVICE = pr.ERR_DEVICE
DRAW_VERTICES = clr.DRAW_VERTICES
MUTANTS = ("base not added to the store", "base not in firstInstance", "room from capacity alone", "entry_count counted from 0",
           "candidates from survive words", "header not written on entry overflow", "SECOND tests planes", "SECOND writes an item FIRST drew",
           "lanes_below inclusive", "word skipped by its last rank")
_NONE = np.zeros(0, CLUSTER_ENTRY_DTYPE)


def room_of(b, entry_capacity):
    """room = entry_capacity - min(b, entry_capacity)."""
    return int(entry_capacity) - min(int(b), int(entry_capacity))


def _refused(b, w, members, status, record=None):
    """A call that writes no entry: a zero count, {192, 0, 0, b}, {0, W mod 2^32, members, 0}."""
    out = dict(status=status, entries=_NONE, count=0, args=np.array([DRAW_VERTICES, 0, 0, b], np.uint32),
               stats=np.array([0, w & 0xFFFFFFFF, members, 0], np.uint32), all_entries=_NONE, survive=None, b=b)
    if record is not None:
        out["record"] = record
    return out


def _listed(survive, items, meshes, first_instance_base, b, entry_capacity, candidates):
    entries = clr.entries_of(items, survive, meshes, first_instance_base)
    room = room_of(b, entry_capacity)
    count = min(len(entries), room)
    return dict(status=ERR_CAPACITY if len(entries) > room else 0, entries=entries[:count], count=count,
                args=np.array([DRAW_VERTICES, count, 0, b], np.uint32), stats=np.array([len(entries), items["W"], items["members"], candidates], np.uint32),
                all_entries=entries, survive=np.asarray(survive, bool), items=items, b=b, room=room)


def first(s, boxes, visible_bitmap, mode, switch_sq, entry_capacity, occlusion, b=0, room_bytes=None, work_capacity=0, first_instance_base=0):
    """What a FIRST call owes with *entry_base = b: dict(status, entries — the ones written, they go to [b, b + count) —, count,
    args, stats, record — the uint32 words the call leaves in the caller's record, as cluster_phase_restatement.first —,
    all_entries, survive, b)."""
    b = int(b) & 0xFFFFFFFF
    f = pr.first(s, boxes, visible_bitmap, mode, switch_sq, 1 << 40, occlusion, room_bytes, work_capacity, first_instance_base)
    items = f["items"]
    if len(np.asarray(s["mesh_id"]).reshape(-1)) == 0:                 # N = 0: zero count, {192, 0, 0, b}, zero stats, a zero header
        return dict(_refused(b, 0, 0, 0, f["record"]), survive=np.zeros(0, bool), items=items)
    if f["survive"] is None:                                          # WORK OVERFLOW: the refusal's header
        return dict(_refused(b, items["W"], items["members"], ERR_CAPACITY, f["record"]), items=items)
    return dict(_listed(f["survive"], items, s["meshes"], first_instance_base, b, entry_capacity, int(f["record"][2])), record=f["record"])


def second(s, boxes, visible_bitmap, mode, switch_sq, entry_capacity, occlusion, record, b=0, room_bytes=None, work_capacity=0, first_instance_base=0):
    """What a SECOND call owes under the new `occlusion` for a record (uint32 words) with *entry_base = b. s["planes"] is not
    read; the record is not modified."""
    b = int(b) & 0xFFFFFFFF
    g = pr.second(s, boxes, visible_bitmap, mode, switch_sq, 1 << 40, occlusion, record, room_bytes, work_capacity, first_instance_base)
    items = g["items"]
    if len(np.asarray(s["mesh_id"]).reshape(-1)) == 0:
        return dict(_refused(b, 0, 0, 0), survive=np.zeros(0, bool), items=items)
    if g["survive"] is None:                                          # WORK OVERFLOW, or NOT THIS CALL'S RECORD
        return dict(_refused(b, items["W"], items["members"], g["status"]), items=items)
    return _listed(g["survive"], items, s["meshes"], first_instance_base, b, entry_capacity, int(np.asarray(record, np.uint32)[2]))


def buffer_of(results, entry_capacity, guard=2):
    """The caller's buffer after `results` (dicts of first / second, in call order): entry_capacity + guard entries, the ones no
    call wrote zero with index_count 0xFFFFFFFF (as by_steps leaves them)."""
    buf = np.zeros(int(entry_capacity) + guard, CLUSTER_ENTRY_DTYPE)
    buf["index_count"] = 0xFFFFFFFF
    for r in results:
        buf[r["b"]: r["b"] + r["count"]] = r["entries"]
    return buf


# ---- the call by steps ----

def by_steps(phase, s, boxes, visible_bitmap, mode, switch_sq, entry_capacity, occlusion, b=0, record=None, first_instance_base=0, mutant=None,
             tile_words=clr.LIST_TILE_WORDS, buf=None):
    """A call that runs (N > 0, no work overflow, in SECOND the call's own record), the way the kernels are described:
    dict(buf — the caller's buffer of entry_capacity + 2 entries behind the call, see buffer_of —, count, args, stats, record —
    FIRST: the words written, or None when the header was not —). phase: "first" / "second". mutant: one of MUTANTS, or None
    for the header's rule."""
    assert mutant is None or mutant in MUTANTS
    items = pr.cr.work_items(s["pos"], s["scale"], s["mesh_id"], s["meshes"], s["cam_pos"], visible_bitmap, mode, switch_sq)
    w, members, t = items["W"], items["members"], items["table"]
    meshes = s["meshes"]
    mins, maxs = pr.world_boxes(items, boxes, s["pos"], s["rot"], s["scale"])
    hidden = pr._occluded(mins, maxs, occlusion) if w else np.zeros(0, bool)
    passed = ~nr.coarse_culled(mins, maxs, s["planes"]) if w else np.zeros(0, bool)
    if phase == "first":
        survive, bits = passed & ~hidden, passed & hidden
    else:
        bits = pr.unpack_record(record, w)
        survive = bits & ~hidden
        if mutant == "SECOND tests planes":
            survive &= passed
        if mutant == "SECOND writes an item FIRST drew":
            survive = ~hidden                                          # the record bit is not asked
    # the front's words
    n_words = (w + 63) // 64
    padded = np.zeros(n_words * 64, bool)
    padded[:w] = survive
    record_padded = np.zeros(n_words * 64, bool)
    record_padded[:w] = bits
    per_word = padded.reshape(n_words, 64).sum(axis=1)
    # count: ranks inside the tile, the tile's survivors; FIRST: the tile's candidates
    tile = np.arange(n_words) // tile_words
    n_tiles = (n_words + tile_words - 1) // tile_words
    tile_total = np.bincount(tile, per_word, minlength=n_tiles).astype(np.int64)
    counted = padded if mutant == "candidates from survive words" else record_padded
    tile_candidates = np.bincount(tile, counted.reshape(n_words, 64).sum(axis=1), minlength=n_tiles).astype(np.int64)
    word_rank = np.cumsum(per_word) - per_word - (np.cumsum(tile_total) - tile_total)[tile] if n_words else np.zeros(0, np.int64)
    # epilogue
    tile_prefix = np.cumsum(tile_total) - tile_total
    survivors = int(tile_total.sum())
    b = int(b) & 0xFFFFFFFF
    cap = int(entry_capacity)
    room = cap if mutant == "room from capacity alone" else cap - min(b, cap)
    count = min(survivors, room)
    if mutant == "entry_count counted from 0":
        count = min(b + survivors, cap)                                # the list's end, not its length
    candidates = int(tile_candidates.sum()) if phase == "first" else int(np.asarray(record, np.uint32)[2])
    args = np.array([DRAW_VERTICES, count, 0, 0 if mutant == "base not in firstInstance" else b], np.uint32)
    stats = np.array([survivors, w, members, candidates], np.uint32)
    written = None
    if phase == "first" and not (mutant == "header not written on entry overflow" and survivors > room):
        written = pr.pack_record(w, members, bits)
        written[2] = candidates
    # write
    if buf is None:
        buf = np.zeros(cap + 2, CLUSTER_ENTRY_DTYPE)
        buf["index_count"] = 0xFFFFFFFF
    inst_of_member = np.nonzero(items["member"])[0]
    sizes = t["C"][items["bucket"][inst_of_member]]
    member_first = np.concatenate([np.cumsum(sizes) - sizes, [w]]).astype(np.int64)
    wm = clr.word_members(member_first[:-1], w)
    for k in range(n_words):
        if per_word[k] == 0:
            continue
        before = int(tile_prefix[tile[k]] + word_rank[k])
        if (before + int(per_word[k]) - 1 if mutant == "word skipped by its last rank" else before) >= room:
            continue
        m0 = int(wm[k])
        lanes = padded[64 * k: 64 * k + 64]
        for lane in np.nonzero(lanes)[0]:
            item = 64 * k + int(lane)
            rank = before + int(lanes[:lane + (1 if mutant == "lanes_below inclusive" else 0)].sum())
            at = rank if mutant == "base not added to the store" else b + rank
            if rank >= room or at >= len(buf):
                continue
            window = member_first[m0: min(m0 + 64, len(inst_of_member))]
            j = int(np.searchsorted(window, item, side="right")) - 1
            i, c = int(inst_of_member[m0 + j]), item - int(window[j])
            bk = int(items["bucket"][i])
            mesh, lod = int(t["mesh"][bk]), int(t["lod"][bk])
            buf[at] = ((i + int(first_instance_base)) & 0xFFFFFFFF, (int(meshes["index_offset"][mesh, lod]) + 192 * c) & 0xFFFFFFFF,
                       int(meshes["vertex_offset"][mesh]), 3 * min(int(t["T"][bk]) - 64 * c, 64))
    return dict(buf=buf, count=count, args=args, stats=stats, record=written, survive=survive)
