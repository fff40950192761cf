"""numpy restatement of mip_list_clusters_views (include/mi_instance_pipeline.h), written from the header's text: one list of
16-byte entries, one count, one VkDrawIndirectCommand and one stats word per view, and both overflow rules. MEMBERS, WORK ITEMS,
W and SURVIVES_v are cluster_views_restatement's, the entry fields are cluster_list_restatement.entries_of's: imported and not
restated. entries_by_steps builds the lists the way the header's launches are described — word members once, word ranks and
tile prefixes per view, then the write with its loop over the views — so that each step can be replaced by a likely mistake
(MUTANTS) and the tests can show which scene catches it. Not reference behaviour: this file is what the library is checked
against."""
import numpy as np

import cluster_list_restatement as clr
import cluster_views_restatement as cvr
from renderer_amd.pipeline import CLUSTER_ENTRY_DTYPE

ERR_CAPACITY = cvr.ERR_CAPACITY
DRAW_VERTICES = clr.DRAW_VERTICES
LIST_TILE_WORDS = clr.LIST_TILE_WORDS
MUTANTS = ("word rank of view 0", "tile prefix of view 0", "base of view 0", "firstInstance left 0", "store offset dropped",
           "cut applied to the sum over views", "clear mask bit writes", "zero word ends the view loop", "lanes_below inclusive",
           "survivors where the heads were")


def draw_args(counts, entry_stride):
    """draw_args: {192, entry_counts[v], 0, v x entry_stride} per view."""
    out = np.zeros((len(counts), 4), np.uint32)
    out[:, 0] = DRAW_VERTICES
    out[:, 1] = counts
    out[:, 3] = [(v * int(entry_stride)) & 0xFFFFFFFF for v in range(len(counts))]
    return out


def list_clusters_views(s, boxes, view_planes, bitmaps, bases, mode, switch_sq, entry_stride, work_capacity=0, cam_pos=None):
    """What mip_list_clusters_views owes for scene s under view v = (view_planes[v], bitmaps[v] — words or None —, bases[v]);
    cam_pos = frames[0].cam_pos (default: the scene's). dict(status; entries — per view the ones written; counts —
    entry_counts; args — (n_views, 4) draw_args; stats — the 2 + n_views words; all_entries — per view every survivor's; items;
    survive — per view; views — cluster_views_restatement's answer with room for every command)."""
    n_views = len(view_planes)
    assert n_views * int(entry_stride) < 1 << 32
    views = cvr.cull_clusters_views(s, boxes, view_planes, bitmaps, bases, mode, switch_sq, 1 << 40, work_capacity, cam_pos)
    none = np.zeros(0, CLUSTER_ENTRY_DTYPE)
    zero = np.zeros(n_views, np.uint32)
    stats = np.zeros(2 + n_views, np.uint32)
    if views["items"] is None:                                    # N = 0
        return dict(status=0, entries=[none] * n_views, counts=zero, args=draw_args(zero, entry_stride), stats=stats, all_entries=[none] * n_views,
                    items=None, survive=None, views=views)
    stats[:2] = views["stats"][:2]
    if views["survive"] is None:                                  # WORK OVERFLOW
        return dict(status=ERR_CAPACITY, entries=[none] * n_views, counts=zero, args=draw_args(zero, entry_stride), stats=stats,
                    all_entries=[none] * n_views, items=views["items"], survive=None, views=views)
    every = [clr.entries_of(views["items"], views["survive"][v], s["meshes"], bases[v]) for v in range(n_views)]
    counts = np.array([min(len(e), int(entry_stride)) for e in every], np.uint32)
    stats[2:] = [len(e) for e in every]
    status = ERR_CAPACITY if any(len(e) > int(entry_stride) for e in every) else 0
    return dict(status=status, entries=[e[:c] for e, c in zip(every, counts)], counts=counts, args=draw_args(counts, entry_stride), stats=stats,
                all_entries=every, items=views["items"], survive=views["survive"], views=views)


def fill_outputs(want, n_views, entry_stride, sentinel, pad, args=True, stats=True):
    """The whole output buffers a call leaves behind when every word was `sentinel` before: dict(entries — (n_views x
    entry_stride + pad, 4) uint32, counts — n_views + pad words, args — 4 n_views + pad words, stats — 2 + n_views + pad)."""
    entries = np.full((n_views * int(entry_stride) + pad, 4), sentinel, np.uint32)
    for v in range(n_views):
        e = want["entries"][v]
        if len(e):
            entries[v * int(entry_stride): v * int(entry_stride) + len(e)] = np.ascontiguousarray(e).view(np.uint32).reshape(-1, 4)
    counts = np.full(n_views + pad, sentinel, np.uint32)
    counts[:n_views] = want["counts"]
    ar = np.full(4 * n_views + pad, sentinel, np.uint32)
    if args:
        ar[: 4 * n_views] = want["args"].reshape(-1)
    st = np.full(2 + n_views + pad, sentinel, np.uint32)
    if stats:
        st[: 2 + n_views] = want["stats"]
    return dict(entries=entries, counts=counts, args=ar, stats=st)


def entries_by_steps(items, survive, meshes, bases, entry_stride, mutant=None, tile_words=LIST_TILE_WORDS, pad=2):
    """The call as its launches build it: dict(entries — a buffer of n_views x entry_stride + pad entries, unwritten ones zero
    with index_count 0xFFFFFFFF; counts; args; stats). mutant: one of MUTANTS, or None for the header's rule."""
    assert mutant is None or mutant in MUTANTS
    n_views, stride = len(survive), int(entry_stride)
    w, t = items["W"], items["table"]
    inst_of_member = np.nonzero(items["member"])[0]
    sizes = t["C"][items["bucket"][inst_of_member]]
    member_first = np.concatenate([np.cumsum(sizes) - sizes, [w]]).astype(np.int64)
    n_words = (w + 63) // 64
    # word members: ONCE for all views
    wm = clr.word_members(member_first[:-1], w)
    # count and epilogue: per view the rank of every word inside its tile, and the tiles' exclusive prefixes
    words, word_rank, tile_prefix, survivors = [], [], [], []
    tile = np.arange(n_words) // tile_words
    n_tiles = (n_words + tile_words - 1) // tile_words
    for v in range(n_views):
        padded = np.zeros(n_words * 64, bool)
        padded[:w] = np.asarray(survive[v], bool)
        per_word = padded.reshape(n_words, 64).sum(axis=1)
        total = np.bincount(tile, per_word, minlength=n_tiles).astype(np.int64)
        prefix = np.cumsum(total) - total
        words.append(padded.reshape(n_words, 64))
        tile_prefix.append(prefix)
        word_rank.append(np.cumsum(per_word) - per_word - prefix[tile] if n_words else np.zeros(0, np.int64))
        survivors.append(int(per_word.sum()))
    if mutant == "cut applied to the sum over views":
        counts = np.array([max(min(stride - sum(survivors[:v]), survivors[v]), 0) for v in range(n_views)], np.uint32)
    else:
        counts = np.minimum(survivors, stride).astype(np.uint32)
    args = draw_args(counts, 0 if mutant == "firstInstance left 0" else stride)
    if mutant == "survivors where the heads were":                # mip_cull_clusters_views' layout: two words per view
        stats = np.zeros(2 + 2 * n_views, np.uint32)
        stats[2::2] = survivors
        stats = stats[: 2 + n_views]
    else:
        stats = np.array([0, 0] + survivors, np.uint32)
    stats[0], stats[1] = w & 0xFFFFFFFF, items["members"]
    # write
    buf = np.zeros(n_views * stride + pad, CLUSTER_ENTRY_DTYPE)
    buf["index_count"] = 0xFFFFFFFF
    for k in range(n_words):
        union = np.zeros(64, bool)
        for v in range(n_views):
            union |= words[v][k]
        if not union.any():
            continue
        m0 = int(wm[k])
        window = member_first[m0: min(m0 + 64, len(inst_of_member))]
        fields = {}
        for lane in np.nonzero(union)[0]:                         # the located item and the three fields all views share
            item = 64 * k + int(lane)
            j = int(np.searchsorted(window, item, side="right")) - 1
            i, c = int(inst_of_member[m0 + j]), item - int(window[j])
            b = int(items["bucket"][i])
            mesh, lod = int(t["mesh"][b]), int(t["lod"][b])
            fields[int(lane)] = (i, (int(meshes["index_offset"][mesh, lod]) + 192 * c) & 0xFFFFFFFF, int(meshes["vertex_offset"][mesh]),
                                 3 * min(int(t["T"][b]) - 64 * c, 64))
        for v in range(n_views):
            bits = words[v][k]
            if not bits.any():
                if mutant == "zero word ends the view loop":
                    break
                continue
            before = int(tile_prefix[0 if mutant == "tile prefix of view 0" else v][tile[k]]) + int(word_rank[0 if mutant == "word rank of view 0" else v][k])
            if before >= stride:
                continue
            offset = 0 if mutant == "store offset dropped" else v * stride
            base = int(bases[0 if mutant == "base of view 0" else v])
            for lane in np.nonzero(union if mutant == "clear mask bit writes" else bits)[0]:
                rank = before + int(bits[: lane + (1 if mutant == "lanes_below inclusive" else 0)].sum())
                limit = stride - offset if mutant == "cut applied to the sum over views" else stride
                if rank >= limit or offset + rank >= len(buf):
                    continue
                i, first_index, vertex_offset, index_count = fields[int(lane)]
                buf[offset + rank] = ((i + base) & 0xFFFFFFFF, first_index, vertex_offset, index_count)
    return dict(entries=buf, counts=counts, args=args, stats=stats)
