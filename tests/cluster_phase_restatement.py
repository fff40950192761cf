"""numpy restatement of cluster culling in two phases (include/mi_instance_pipeline.h, mip_cull_clusters_phase), written from
the header's text: the record (header and words), FIRST — mip_cull_clusters' outputs and the candidates —, SECOND — SURVIVES2,
heads and commands over it, the record that is not the call's — and both work-overflow rules. Members, work items and commands
are cluster_restatement's, the plane test numpy_restatement's, steps 1-9 occlusion_restatement's. `mutant` switches one likely
mistake on (tests/test_cluster_phase_restatement.py shows that the hand-written scenes tell each of them apart). Not reference
behaviour: this file is what the library is checked against."""
import numpy as np

import cluster_restatement as cr
import numpy_restatement as nr
import occlusion_restatement as orr
from renderer_amd.pipeline import DRAW_CMD_DTYPE

F = np.float32
ERR_CAPACITY = cr.ERR_CAPACITY
ERR_DEVICE = -5          # MIP_ERR_DEVICE
REFUSED = 0xFFFFFFFF     # the header's W of a FIRST call that did not run
MUTANTS = ("record_frustum_culled", "record_without_occlusion", "second_tests_planes", "heads_over_union", "no_start_word")


def record_bytes(work_items):
    """mip_cluster_record_bytes."""
    return 16 + 8 * ((int(work_items) + 63) // 64)


def pack_record(w, members, bits):
    """The record as uint32 words: {W, members, candidates, 0}, then ceil(W / 64) 64-bit words, bit j of word k = item 64 k + j."""
    bits = np.asarray(bits, bool)
    assert len(bits) == w
    padded = np.zeros(64 * ((w + 63) // 64), np.uint8)
    padded[:w] = bits
    words = np.packbits(padded, bitorder="little").view(np.uint32) if w else np.zeros(0, np.uint32)
    return np.concatenate([np.array([w, members, int(bits.sum()), 0], np.uint32), words])


def unpack_record(record, w):
    """The bits of the first w work items of a record."""
    words = np.ascontiguousarray(np.asarray(record, np.uint32)[4 : 4 + 2 * ((w + 63) // 64)])
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:w].astype(bool) if w else np.zeros(0, bool)


def world_boxes(items, boxes, pos, rot, scale):
    """(mins, maxs) of every work item's world box: the cluster's box under the instance's model matrix (the literal chain)."""
    i = items["inst"]
    model = nr.model_matrices(np.asarray(pos, F).reshape(-1, 3)[i], np.asarray(rot, F).reshape(-1, 4)[i], np.asarray(scale, F).reshape(-1)[i])
    box = np.asarray(boxes, F).reshape(-1, 6)[items["box_index"]]
    return nr.world_aabbs(model, box[:, :3], box[:, 3:])


def _occluded(mins, maxs, occlusion):
    return orr.occluded(np.concatenate([mins, maxs], axis=1), occlusion["pv"], occlusion["levels"], occlusion["width"], occlusion["height"])


def _bound(s, items, work_capacity, room_bytes):
    """The bound W is held to: the caller's or N x the largest C, and the work items the record has words for."""
    n = len(np.asarray(s["mesh_id"]).reshape(-1))
    largest = int(items["table"]["C"].max()) if len(items["table"]["C"]) else 0
    bound = int(work_capacity) if work_capacity else n * largest
    return min(bound, 64 * ((int(room_bytes) - 16) // 8), (1 << 32) - 1)


def _work_overflow(items):
    return dict(status=ERR_CAPACITY, cmds=np.zeros(0, DRAW_CMD_DTYPE), count=0, stats=np.array([0, 0, items["W"] & 0xFFFFFFFF, items["members"]], np.uint32),
                items=items, survive=None)


def first(s, boxes, visible_bitmap, mode, switch_sq, cmd_capacity, occlusion, room_bytes=None, work_capacity=0, first_instance_base=0, mutant=None):
    """What a FIRST call owes: cluster_restatement.cull_clusters' dict (status, cmds, count, stats, items, survive) and `record`,
    the uint32 words the call leaves in the caller's record: four for a call that did not run or had N = 0 (no word behind the
    header is defined then), else the whole record. room_bytes: record_bytes as the caller states it (default: exactly enough)."""
    items = cr.work_items(s["pos"], s["scale"], s["mesh_id"], s["meshes"], s["cam_pos"], visible_bitmap, mode, switch_sq)
    n = len(np.asarray(s["mesh_id"]).reshape(-1))
    room = record_bytes(items["W"]) if room_bytes is None else int(room_bytes)
    if n and items["W"] > _bound(s, items, work_capacity, room):
        return dict(_work_overflow(items), record=np.array([REFUSED, 0, 0, 0], np.uint32))
    r = cr.cull_clusters(s, boxes, visible_bitmap, mode, switch_sq, cmd_capacity, work_capacity, first_instance_base, occlusion)
    if n == 0:
        return dict(r, record=np.zeros(4, np.uint32))
    mins, maxs = world_boxes(items, boxes, s["pos"], s["rot"], s["scale"])
    passed = ~nr.coarse_culled(mins, maxs, s["planes"]) if items["W"] else np.zeros(0, bool)
    hidden = _occluded(mins, maxs, occlusion) if items["W"] else np.zeros(0, bool)
    bits = passed & hidden                       # NOT culled by the plane test AND occluded
    if mutant == "record_frustum_culled":
        bits = hidden | ~passed
    elif mutant == "record_without_occlusion":
        bits = passed
    assert mutant or np.array_equal(r["survive"], passed & ~hidden)
    return dict(r, record=pack_record(items["W"], items["members"], bits), candidates=bits)


def second(s, boxes, visible_bitmap, mode, switch_sq, cmd_capacity, occlusion, record, room_bytes=None, work_capacity=0, first_instance_base=0,
           mutant=None, first_survive=None):
    """What a SECOND call owes under the new `occlusion` for a record (uint32 words): dict(status, cmds, count, stats, items,
    survive). s["planes"] is not read. first_survive: FIRST's survivors, for the heads_over_union mutant alone."""
    items = cr.work_items(s["pos"], s["scale"], s["mesh_id"], s["meshes"], s["cam_pos"], visible_bitmap, mode, switch_sq)
    n = len(np.asarray(s["mesh_id"]).reshape(-1))
    w, members = items["W"], items["members"]
    none = np.zeros(0, DRAW_CMD_DTYPE)
    if n == 0:
        return dict(status=0, cmds=none, count=0, stats=np.zeros(4, np.uint32), items=items, survive=np.zeros(0, bool), all_cmds=none)
    room = 4 * len(record) if room_bytes is None else int(room_bytes)
    if w > _bound(s, items, work_capacity, room):
        return dict(_work_overflow(items), all_cmds=none)
    record = np.asarray(record, np.uint32)
    if int(record[0]) != w or int(record[1]) != members:     # not this call's record
        return dict(status=ERR_DEVICE, cmds=none, count=0, stats=np.array([0, 0, w, members], np.uint32), items=items, survive=None, all_cmds=none)
    bits = unpack_record(record, w)
    sv = np.zeros(w, bool)
    if bits.any():
        mins, maxs = world_boxes(items, boxes, s["pos"], s["rot"], s["scale"])
        sv[bits] = ~_occluded(mins[bits], maxs[bits], occlusion)
        if mutant == "second_tests_planes":
            sv &= ~nr.coarse_culled(mins, maxs, s["planes"])
    cmds, head = cr.commands(items, sv, s["meshes"], first_instance_base)
    if mutant in ("heads_over_union", "no_start_word"):
        drawn = sv | np.asarray(first_survive, bool) if mutant == "heads_over_union" else sv
        before = np.concatenate([np.zeros(1, bool), drawn[:-1]]) if w else np.zeros(0, bool)
        wrong = sv & (((items["cluster"] == 0) & (mutant != "no_start_word")) | ~before)
        assert not (wrong & ~head).any()
        cmds, head = cmds[wrong[head]], wrong
    heads = len(cmds)
    count = min(heads, int(cmd_capacity))
    return dict(status=ERR_CAPACITY if heads > int(cmd_capacity) else 0, cmds=cmds[:count], count=count,
                stats=np.array([heads, int(sv.sum()), w, members], np.uint32), items=items, survive=sv, head=head, all_cmds=cmds)
