"""A CPU model of how the binning stage of the batched-draws family DECOMPOSES a call (renderer_amd/csrc/batch_kernel.hpp and the
key policies and command writers beside it): batch_index, the tile histogram with its store guard, rowscan in chunks of 256 tiles
with a carry, the scatter's rank (the match by `valid` and eight digit bits, the per-wave rows over four rounds, digits_below as a
256-wide block scan, the wave bases), the list passes that read `members` entries, the ping-pong of the (key, instance) lists, the
command writers in chunks of 256 buckets (pair, chain, views with s_view_cmd / s_view_slot and the histogram copies, the shard
epilogue) and mip_batch_sorted_members_kernel. The pass count, the shifts, the ping-pong and the kernel kinds are READ from
batch_plan.hpp through tests/native/batch_plan_probe.cpp and never restated. The float32 rules that turn instance columns into
(member, bucket, depth) are the restatements' (lod_restatement, order_restatement, sorted_restatement, batch_restatement): this
model is about the decomposition behind them. Every entry returns its outputs and the set of named structural EDGES the call
touched, detected from the data. Every MUTANT — one mistake in the decomposition each — changes the output of a named case
(tests/test_batch_stage_cases.py). No GPU."""
import functools
import hashlib
import json
import os
import subprocess
import tempfile

import numpy as np

import batch_restatement as br
import lod_restatement as lr
import order_restatement as orr
import sorted_restatement as sr

NONE = 0xFFFFFFFF        # kBatchNone
LANES, ROUNDS, WAVES = 64, 4, 4
TILE = LANES * ROUNDS * WAVES      # kBatchTile
BINS = 256               # kBatchBins
CHUNK = 256              # kTile: tiles per step of rowscan, buckets per step of a command writer
CMD_WORDS = 5
SENTINEL = 0x5A5A5A5A
STALE = 0                # what a list buffer holds before anything wrote it: unknown on the device; here a VALID key, so a read shows

MUTANTS = ("match_without_valid", "row_reset_every_round", "wave_base_skips_previous", "digits_below_reset_at_seam",
           "rowscan_carry_dropped", "rowscan_carry_last_nonzero_chunk", "idle_lane_is_member", "list_pass_over_n", "list_pass_reversed_in_tile",
           "cmds_before_not_carried", "members_before_not_carried", "view_first_cmd_current_chunk_only", "hist_copy_0_only",
           "ordered_bucket_of_is_key", "far_first_flips_whole_key")

_HERE = os.path.dirname(os.path.abspath(__file__))
_PROBE_SRC = os.path.join(_HERE, "native", "batch_plan_probe.cpp")
_PLAN_HPP = os.path.join(os.path.dirname(_HERE), "renderer_amd", "csrc", "batch_plan.hpp")
_exe = None


def probe_exe():
    global _exe
    if _exe is None:
        text = open(_PROBE_SRC, "rb").read() + open(_PLAN_HPP, "rb").read()
        exe = os.path.join(tempfile.gettempdir(), f"mip_batch_plan_probe_{os.getuid()}_{hashlib.sha1(text).hexdigest()[:16]}")
        if not os.path.exists(exe):
            tmp = f"{exe}.{os.getpid()}"
            subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", _PROBE_SRC, "-o", tmp])
            os.replace(tmp, exe)
        _exe = exe
    return _exe


@functools.lru_cache(maxsize=None)
def plan(*args):
    """plan("lods", relative, buckets, want_model, general) or plan("sorted", relative, axis, depth_bits, want_model, general)."""
    out = subprocess.run([probe_exe()] + [str(int(a)) if not isinstance(a, str) else a for a in args], capture_output=True, text=True, timeout=120, check=True)
    p = json.loads(out.stdout)
    assert p["digit_bits"] == 8 and BINS == 1 << p["digit_bits"]
    return p


def hist_copies_for(several, buckets):
    """api_batch.hip, batch_draws_views ("several passes: copies of the bucket histogram ... at most 2^20 words"): 64 copies,
    halved while copies x buckets > 2^20; one copy for a single pass."""
    copies = 64 if several else 1
    while copies > 1 and copies * buckets > (1 << 20):
        copies >>= 1
    return copies


def batch_index(tile, wave, rnd, lane):
    """Instance (tile, wave, round, lane): wave w takes [256 w, 256 w + 256) of the tile in four rounds of 64 consecutive ones."""
    return tile * TILE + wave * (ROUNDS * LANES) + rnd * LANES + lane


def _rank_in_group(gid):
    """For every element, how many EARLIER elements hold the same gid (what a ballot match and lanes_below give a lane)."""
    order = np.argsort(gid, kind="stable")
    sg = gid[order]
    at = np.arange(len(sg))
    first = np.maximum.accumulate(np.where(np.r_[True, sg[1:] != sg[:-1]], at, 0)) if len(sg) else at
    rank = np.empty(len(gid), np.int64)
    rank[order] = at - first
    return rank


class Scratch:
    """The two (key, instance) list buffer pairs of a frame slot, kept from call to call as MipContext::BatchScratch keeps them."""

    def __init__(self):
        self.keys = [np.zeros(0, np.uint32), np.zeros(0, np.uint32)]
        self.ids = [np.zeros(0, np.uint32), np.zeros(0, np.uint32)]
        self.last_members = None

    def ensure(self, entries):
        if entries > len(self.keys[0]):
            self.keys = [np.full(entries, STALE, np.uint32) for _ in range(2)]
            self.ids = [np.full(entries, STALE, np.uint32) for _ in range(2)]
            self.last_members = None


class _Stage:
    """count / rowscan / scatter over the passes of one plan."""

    def __init__(self, p, n_entries, n_bins, scratch, mutant, edges):
        assert mutant is None or mutant in MUTANTS
        self.p, self.n_entries, self.n_bins, self.mutant, self.edges = p, int(n_entries), int(n_bins), mutant, edges
        self.n_tiles = -(-self.n_entries // TILE)
        self.scratch = scratch or Scratch()
        if p["several"]:
            self.scratch.ensure(self.n_entries)
        self.padded = self.n_tiles * TILE
        # the tiling the kernels use, checked once against batch_index
        idx = np.arange(self.padded)
        self.tile, self.wave, self.rnd = idx // TILE, (idx // (ROUNDS * LANES)) % WAVES, (idx // LANES) % ROUNDS
        assert np.array_equal(batch_index(self.tile, self.wave, self.rnd, idx % LANES), idx)

    # ---- the keys of a pass, one per lane of every tile ----
    def column_keys(self, keys0):
        k = np.full(self.padded, NONE, np.uint32)
        k[: self.n_entries] = keys0
        if self.mutant == "idle_lane_is_member":   # an idle lane loads the last entry (in bounds) and forgets that it is idle
            k[self.n_entries:] = keys0[-1]
        if self.padded > self.n_entries:
            self.edges.add("idle_lanes_behind_member" if keys0[-1] != NONE else "idle_lanes_behind_nonmember")
        else:
            self.edges.add("no_idle_lanes")
        return k, np.arange(self.padded, dtype=np.int64)

    def list_keys(self, pair, members):
        list_len = self.n_entries if self.mutant == "list_pass_over_n" else members
        k = np.full(self.padded, NONE, np.uint32)
        k[:list_len] = self.scratch.keys[pair][:list_len]
        ids = np.zeros(self.padded, np.int64)
        ids[: self.n_entries] = self.scratch.ids[pair][: self.n_entries]
        if members % LANES:
            self.edges.add("list_len_inside_a_round")
        if -(-members // TILE) < self.n_tiles:
            self.edges.add("list_tiles_beyond_members_idle")
        return k, ids

    # ---- count ----
    def count(self, k, shift):
        valid = k != NONE
        digit = ((k >> np.uint32(shift)) & np.uint32(BINS - 1)).astype(np.int64)
        hist = np.bincount(self.tile[valid] * BINS + digit[valid], minlength=self.n_tiles * BINS).reshape(self.n_tiles, BINS)
        return hist[:, : self.n_bins].T.copy()     # `if (tid < a.n_bins)`: counts[bin][tile]

    # ---- rowscan ----
    def rowscan(self, counts, note):
        out = np.zeros_like(counts)
        carry = np.zeros(counts.shape[0], np.int64)
        chunk_totals = []
        for first in range(0, self.n_tiles, CHUNK):
            v = counts[:, first: first + CHUNK]
            total = v.sum(axis=1)
            if self.mutant == "rowscan_carry_dropped":
                carry[:] = 0
            out[:, first: first + CHUNK] = carry[:, None] + (np.cumsum(v, axis=1) - v)
            carry = np.where(total > 0, total, carry) if self.mutant == "rowscan_carry_last_nonzero_chunk" else carry + total
            chunk_totals.append(total)
        if note:
            ct = np.array(chunk_totals).T                      # [bin][chunk]
            live = counts.sum(axis=1) > 0
            if self.n_tiles in (1, 255, 256, 257, 512, 513):
                self.edges.add(f"n_tiles={self.n_tiles}")
            if ct.shape[1] >= 2:
                if (live & (ct[:, 0] == 0)).any():
                    self.edges.add("bin_first_chunk_zero")
                if (live & (ct[:, 0] > 0) & (ct[:, 1] == 0)).any():
                    self.edges.add("bin_second_chunk_zero")
            nz = counts > 0
            for b in np.nonzero(live)[0]:
                tiles = set(np.nonzero(nz[b])[0].tolist())
                if tiles == {0, 256}:
                    self.edges.add("bin_in_tile_0_and_256_only")
                if tiles == {255} and self.n_tiles > 256:
                    self.edges.add("bin_in_tile_255_only")
                if tiles == {self.n_tiles - 1} and self.n_tiles > 1:
                    self.edges.add("bin_in_last_tile_only")
        return out, carry

    # ---- scatter: the slot of every lane (valid lanes only are stored) ----
    def scatter(self, k, shift, scanned, totals, from_list, kinds=None):
        m, T = self.mutant, self.n_tiles
        valid = k != NONE
        digit = np.where(valid, (k >> np.uint32(shift)) & np.uint32(BINS - 1), 0).astype(np.int64)
        rounds = np.arange(self.padded) // LANES                     # (tile, wave, round), flat
        # the match: `same` starts as ballot(valid) and is narrowed by the eight digit bits
        part = np.ones(self.padded, bool) if m == "match_without_valid" else valid
        gid = rounds * BINS + digit
        below = np.zeros(self.padded, np.int64)
        below[part] = _rank_in_group(gid[part])
        size = np.bincount(gid[part], minlength=T * WAVES * ROUNDS * BINS)
        lead = part & (below == 0) & valid                           # `if (valid && below == 0u)`: the first of the group adds it to the row
        added = np.zeros(T * WAVES * ROUNDS * BINS, np.int64)
        added[gid[lead]] = size[gid[lead]]
        added = added.reshape(T * WAVES, ROUNDS, BINS)
        before = np.cumsum(added, axis=1) - added                    # the wave's own row: what its earlier rounds held
        wave_count = added.sum(axis=1)
        if m == "row_reset_every_round":
            before = np.zeros_like(added)
            wave_count = added[:, ROUNDS - 1, :]
        rank = before.reshape(-1)[gid] + below
        # digits_below: a 256-wide block scan of the digit totals, wave by wave
        t = np.zeros(BINS, np.int64)
        t[: self.n_bins] = totals
        w = t.reshape(WAVES, LANES)
        incl = np.cumsum(w, axis=1)
        seam = np.cumsum(incl[:, -1]) - incl[:, -1]
        if m == "digits_below_reset_at_seam":
            seam[:] = 0
        digits_below = (seam[:, None] + incl - w).reshape(BINS)
        start = np.zeros((T, BINS), np.int64)
        start[:, : self.n_bins] = scanned.T
        start += digits_below[None, :]
        cw = wave_count.reshape(T, WAVES, BINS)
        excl = np.cumsum(cw, axis=1) - cw
        if m == "wave_base_skips_previous":
            excl[:, 1:, :] -= cw[:, :-1, :]
        base = start[:, None, :] + excl
        slot = base.reshape(-1)[(self.tile * WAVES + self.wave) * BINS + digit] + rank
        if from_list and m == "list_pass_reversed_in_tile":
            ts, tc = start.reshape(-1)[self.tile * BINS + digit], cw.sum(axis=1).reshape(-1)[self.tile * BINS + digit]
            slot = ts + (tc - 1 - (slot - ts))
        if not from_list:
            self._placement_edges(valid, digit, added, cw, kinds)
        return valid, slot

    def _placement_edges(self, valid, digit, added, cw, kinds):
        e, T = self.edges, self.n_tiles
        per_round = (added > 0).sum(axis=2)                          # distinct digits per (wave, round)
        if (added.max(axis=2) == LANES).any():
            e.add("round_of_one_digit")
        if (per_round == LANES).any():
            e.add("round_of_64_digits")
        used = np.unique(digit[valid])
        if len(used) == 2 and (used[0] ^ used[1]) in (1, 128):
            e.add("digits_differ_in_bit_0_only" if (used[0] ^ used[1]) == 1 else "digits_differ_in_bit_7_only")
        for a, b in ((63, 64), (127, 128), (191, 192), (0, 255)):
            if set(used.tolist()) == {a, b}:
                e.add(f"only_bins_{a}_and_{b}")
        if kinds is not None:                                        # 1: a clear bitmap bit, 2: a dead mesh with its bit set
            v2, d2, k2 = valid.reshape(-1, LANES), digit.reshape(-1, LANES), np.zeros(self.padded, np.int64)
            k2[: len(kinds)] = kinds
            k2 = k2.reshape(-1, LANES)
            zero_after = v2[:, 1:] & (d2[:, 1:] == 0)
            for kind, name in ((1, "clear_bit_beside_bucket_0"), (2, "dead_mesh_beside_bucket_0")):
                if (zero_after & (k2[:, :-1] == kind)).sum() >= LANES // 2 - 1:
                    e.add(name)
        r = added > 0
        if (r[:, 0] & r[:, 3] & ~r[:, 1] & ~r[:, 2]).any():
            e.add("bin_in_rounds_0_and_3_only")
        wv = cw > 0
        if (wv[:, 0] & wv[:, 3] & ~wv[:, 1] & ~wv[:, 2]).any():
            e.add("bin_in_waves_0_and_3_only")
        if (cw.sum(axis=1) == TILE).any():
            e.add("bin_fills_a_tile")
        tile_members = cw.sum(axis=(1, 2))
        live = np.nonzero(tile_members)[0]
        if len(live) and (tile_members[live[0]: live[-1] + 1] == 0).any():
            e.add("empty_tile_between_tiles")

    # ---- the passes ----
    def run(self, keys0, id_of_entry, kinds, bucket_hist_of, members_of, first_instance):
        """keys0: the key of every entry of pass 0 (NONE: not a member). id_of_entry(idx): Key::id. bucket_hist_of(keys, tiles):
        what pass 0 of several adds to the bucket histogram (None: no histogram). members_of(totals0, hist): the word the command
        kernel leaves for the list passes. first_instance(keys): what the last scatter adds to an id. Returns ids (uint32 written
        slots, by slot), slot_of (or None), the totals of pass 0, the histogram."""
        p, sc = self.p, self.scratch
        members, hist, totals0, out_ids, slot_of = None, None, None, {}, None
        for n, io in enumerate(p["pass"]):
            kinds_launch = [l[0] for l in io["launch"]]
            assert kinds_launch[1] == "rowscan" and (kinds_launch[2] != "none") == io["commands"] == (n == 0)
            from_list = io["list_in"] >= 0
            assert from_list == (n > 0) and (kinds_launch[0] == "count_list") == from_list
            assert kinds_launch[3] == ("columns" if n == 0 else "list_mid" if not io["ids"] else kinds_launch[3])
            assert not from_list or not io["ids"] or kinds_launch[3] in ("list_last", "views_list_last")
            k, ids = self.list_keys(io["list_in"], members) if from_list else self.column_keys(keys0)
            if not from_list:
                ids = id_of_entry(ids)
            counts = self.count(k, io["shift"])
            if io["bucket_hist"]:
                valid = k != NONE
                hist = bucket_hist_of(k[valid], self.tile[valid])
            scanned, totals = self.rowscan(counts, note=n == 0)
            if n == 0:
                totals0 = totals
                members = members_of(totals0, hist)
            valid, slot = self.scatter(k, io["shift"], scanned, totals, from_list, kinds if n == 0 else None)
            at = slot[valid]
            if io["ids"]:
                out_ids = dict(slots=at, values=((first_instance(k[valid]) + ids[valid]) & 0xFFFFFFFF).astype(np.uint32))
                if io["slot_of"]:
                    slot_of = dict(ids=ids[valid], slots=at)
            else:
                keep = (at >= 0) & (at < len(sc.keys[io["list_out"]]))       # (a mutant may run off the list: the model stops there)
                sc.keys[io["list_out"]][at[keep]] = k[valid][keep]
                sc.ids[io["list_out"]][at[keep]] = ids[valid][keep].astype(np.uint32)
        if p["several"]:
            if sc.last_members is not None and sc.last_members > members:
                self.edges.add("stale_keys_behind_members")
            sc.last_members = members
        return out_ids, slot_of, totals0, hist, members


def _ids_buffer(out_ids, room):
    """instance_ids as the call leaves a buffer of `room` sentinel words."""
    buf = np.full(room, SENTINEL, np.uint32)
    if out_ids:
        keep = (out_ids["slots"] >= 0) & (out_ids["slots"] < room)
        buf[out_ids["slots"][keep]] = out_ids["values"][keep]
    return buf


# ---- command writers ----

def chain_draw(meshes, b):
    base, _ = lr.lod_bases(meshes)
    mesh = np.searchsorted(base, b, side="right") - 1       # bucket_lod: mesh << 3 | lod of every bucket
    lod = b - base[mesh]
    return meshes["index_len"][mesh, lod], meshes["index_offset"][mesh, lod], meshes["vertex_offset"][mesh]


def pair_draw(meshes, b):
    assert (meshes["n_lods"] == 2).all(), "the model's pair writer takes two-level meshes (len1 / src_offset1 are the level's own)"
    mesh, far = b >> 1, b & 1
    return meshes["index_len"][mesh, far], meshes["index_offset"][mesh, far], meshes["vertex_offset"][mesh]


def _rows(draw, meshes, b, c, slot):
    rows = np.zeros((len(b), CMD_WORDS), np.uint32)
    ic, fi, vo = draw(meshes, b)
    rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4] = ic, c, fi, vo.astype(np.int64) & 0xFFFFFFFF, slot
    return rows


def commands(bucket_totals, n_buckets, draw, meshes, room, mutant, edges):
    """mip_batch_commands_kernel: 256 buckets per step, two block scans, two carries. Returns (cmds buffer, count, members)."""
    buf = np.full((room, CMD_WORDS), SENTINEL, np.uint32)
    cmds_before = members_before = 0
    chunk_members = []
    for first in range(0, n_buckets, CHUNK):
        c = np.asarray(bucket_totals[first: first + CHUNK], np.int64)
        live = c > 0
        if mutant == "cmds_before_not_carried":
            cmds_before = 0
        if mutant == "members_before_not_carried":
            members_before = 0
        slot = members_before + np.cumsum(c) - c
        at = cmds_before + np.cumsum(live) - live
        rows = _rows(draw, meshes, first + np.nonzero(live)[0], c[live], slot[live])
        keep = at[live] < room
        buf[at[live][keep]] = rows[keep]
        cmds_before += int(live.sum())
        members_before += int(c.sum())
        chunk_members.append(int(c.sum()))
    _writer_edges(np.asarray(bucket_totals[:n_buckets], np.int64), chunk_members, edges)
    return buf, cmds_before, members_before


def _writer_edges(c, chunk_members, edges):
    live = set(np.nonzero(c)[0].tolist())
    n = len(c)
    for a in (255, 511, 65535):
        if live == {a, a + 1}:
            edges.add(f"only_buckets_{a}_and_{a + 1}")
        if {a, a + 1} <= live:
            edges.add(f"buckets_{a}_and_{a + 1}_used")
    if n > 1 and live == {n - 1}:
        edges.add("only_the_last_bucket")
    if n - 1 in live:
        edges.add("last_bucket_used")
    if n >= 513 and (c == 1).all():
        edges.add("every_bucket_one_member")
    nz = [k for k, v in enumerate(chunk_members) if v]
    if nz and any(v == 0 for v in chunk_members[nz[0]: nz[-1] + 1]):
        edges.add("empty_bucket_chunk_between_chunks")


def view_commands(hist, copies, n_views, view_buckets, stride, meshes, want_first_slot, mutant, edges, pad=3):
    """mip_batch_view_commands_kernel. hist: [copies][n_views x B]. Returns dict(cmds, counts, first_slot) as whole buffers."""
    n_buckets = n_views * view_buckets
    buf = np.full((n_views * stride + pad, CMD_WORDS), SENTINEL, np.uint32)
    s_cmd, s_slot = np.zeros(n_views + 1, np.int64), np.zeros(n_views + 1, np.int64)
    cmds_before = members_before = 0
    hist = np.asarray(hist, np.int64).reshape(copies, n_buckets)
    total = hist[0] if mutant == "hist_copy_0_only" else hist.sum(axis=0)
    for first in range(0, n_buckets, CHUNK):
        g = np.arange(first, min(first + CHUNK, n_buckets))
        c = total[g]
        v, live = g // view_buckets, c > 0
        b = g - v * view_buckets
        slot = members_before + np.cumsum(c) - c
        at = cmds_before + np.cumsum(live) - live
        if mutant == "view_first_cmd_current_chunk_only":
            s_cmd[:] = cmds_before
        s_cmd[v[b == 0]], s_slot[v[b == 0]] = at[b == 0], slot[b == 0]
        rows = _rows(chain_draw, meshes, b[live], c[live], slot[live])
        to = v[live] * stride + (at[live] - s_cmd[v[live]])
        keep = (to >= 0) & (to < len(buf))
        buf[to[keep]] = rows[keep]
        cmds_before += int(live.sum())
        members_before += int(c.sum())
    s_cmd[n_views], s_slot[n_views] = cmds_before, members_before
    counts = np.full(n_views + pad, SENTINEL, np.uint32)
    counts[:n_views] = ((s_cmd[1:] - s_cmd[:-1]) & 0xFFFFFFFF).astype(np.uint32)
    first_slot = np.full(n_views + 1 + pad, SENTINEL, np.uint32)
    if want_first_slot:
        first_slot[: n_views + 1] = s_slot
    # edges
    per_view = total.reshape(n_views, view_buckets)
    empty = per_view.sum(axis=1) == 0
    if n_views >= 3 and not empty.all():
        if empty[0]:
            edges.add("empty_view_first")
        if empty[-1]:
            edges.add("empty_view_last")
        if empty[1:-1].any():
            edges.add("empty_view_in_the_middle")
    if n_views > 1 and view_buckets % CHUNK == 0 or (n_views > 1 and CHUNK % view_buckets == 0 and view_buckets * n_views > CHUNK):
        edges.add(f"view_boundary_on_a_chunk_boundary_B={view_buckets}")
    for vv in range(n_views):
        nzb = np.nonzero(per_view[vv])[0]
        if len(nzb) and (vv * view_buckets + nzb[0]) // CHUNK >= (vv * view_buckets) // CHUNK + 2:
            edges.add("view_first_members_two_chunks_later")
    edges.add(f"n_views={n_views}")
    if copies == 64:
        if (hist.sum(axis=1) > 0).all():
            edges.add("every_histogram_copy_used")
        if ((hist[63] > 0) & (hist[:63].sum(axis=0) == 0)).any():
            edges.add("only_copy_63_for_a_bucket")
    edges.add("view_first_slot_given" if want_first_slot else "view_first_slot_null")
    return dict(cmds=buf, counts=counts, first_slot=first_slot), members_before


def shard_chunk(bucket_totals, n_buckets, ids_buffer):
    """mip_batch_shard_chunk_kernel in the command writer's place: the header, the dense counts, the pad; the ids behind them."""
    padded = n_buckets + (4 - n_buckets % 4) % 4
    counts = np.zeros(padded, np.uint32)
    counts[:n_buckets] = bucket_totals[:n_buckets]
    members = int(counts.sum())
    return np.concatenate([np.array([members, n_buckets, 0, 0], np.uint32), counts, ids_buffer]), members


# ---- the entry points ----

def _member_kinds(bits, length):
    """0: member; 1: the bitmap bit is clear; 2: the bit is set and the level has no indices (a dead mesh)."""
    return np.where(~bits, 1, np.where(length > 0, 0, 2))


def _chain_keys(s, cam, bitmap):
    n = len(s["mesh_id"])
    mid = s["mesh_id"].astype(np.int64)
    lod = lr.select_lods(s["pos"], s["scale"], mid, s["meshes"], cam, lr.DISTANCE, s["switch_sq"])
    bits = np.ones(n, bool) if bitmap is None else br.bitmap_bits(bitmap, n)
    kinds = _member_kinds(bits, s["meshes"]["index_len"][mid, lod])
    base, n_buckets = lr.lod_bases(s["meshes"])
    return np.where(kinds == 0, base[mid] + lod, -1), kinds, n_buckets


def _key_words(bucket_or_minus_one, key):
    return np.where(bucket_or_minus_one >= 0, key, NONE).astype(np.uint32)


def run(entry, s, *, base=0, want_model=False, order=None, sort=None, views=None, capacity=None, scratch=None, mutant=None):
    """One call of `entry` ("draws", "lods", "ordered", "views", "shard", "sorted") over the scene dict s (pos, scale, mesh_id,
    meshes, bitmap, cam, switch_sq). Returns (outputs, edges). outputs: cmds (count x 5 words), count, ids, members for the
    single-view entries (+ slot_of when the plan writes it); the whole buffers of mip_batch_draws_views; the chunk's words."""
    edges = set()
    n = len(s["mesh_id"])
    mid = s["mesh_id"].astype(np.int64)
    meshes = s["meshes"]
    general = not (np.isfinite(s["pos"]).all() and np.isfinite(s["scale"]).all())
    if n in (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049):
        edges.add(f"N={n}")

    if entry == "views":
        cams, bitmaps, bases, stride, want_first_slot = views["cams"], views["bitmaps"], views["bases"], views["stride"], views["first_slot"]
        V = len(cams)
        per_view = [_chain_keys(s, cams[v], bitmaps[v]) for v in range(V)]
        B = per_view[0][2]
        p = plan("views", 0, V * B, 0, 0)
        copies = hist_copies_for(p["several"], V * B)
        bucket = np.stack([pv[0] for pv in per_view], axis=1).reshape(-1)          # entry e = i * V + v
        kinds = np.stack([pv[1] for pv in per_view], axis=1).reshape(-1)
        view = np.tile(np.arange(V), n)
        keys0 = _key_words(bucket, view * B + bucket)
        n_buckets = V * B
        stage = _Stage(p, V * n, BINS if p["several"] else n_buckets, scratch, mutant, edges)
        bases_a = np.asarray([int(b) for b in bases], np.int64)

        def hist_of(keys, tiles):
            h = np.zeros(copies * n_buckets, np.int64)
            np.add.at(h, (tiles & (copies - 1)) * n_buckets + keys.astype(np.int64), 1)
            return h

        holder = {}

        def members_of(totals0, hist):
            h = hist if p["several"] else np.asarray(totals0, np.int64)
            holder["out"], members = view_commands(h, copies, V, B, stride, meshes, want_first_slot, mutant, edges)
            return members

        out_ids, _, _, _, members = stage.run(keys0, lambda idx: idx // V, kinds, hist_of, members_of, lambda k: bases_a[k.astype(np.int64) // B])
        out = holder["out"]
        out["ids"] = _ids_buffer(out_ids, V * n + 3)
        if out_ids and ((bases_a[:, None] + np.arange(n)[None, :]) > 0xFFFFFFFF).any() and len(set(bases)) == V:
            edges.add("distinct_bases_one_wraps")
        _multi_pass_edges(p, keys0, edges)
        return out, edges

    if entry == "draws":
        lod = br.pick_lods(s["pos"], mid, meshes, s["cam"])
        bits = br.bitmap_bits(s["bitmap"], n)
        kinds = _member_kinds(bits, meshes["index_len"][mid, lod])
        bucket = np.where(kinds == 0, mid * 2 + lod, -1)
        n_buckets = 2 * len(meshes)
        keys0, draw = _key_words(bucket, bucket), pair_draw
        p = plan("draws", 0, n_buckets, want_model, general)
    else:
        bucket, kinds, n_buckets = _chain_keys(s, s["cam"], s["bitmap"])
        keys0, draw = _key_words(bucket, bucket), chain_draw
        if entry in ("lods", "shard"):
            p = plan(entry, 0, n_buckets, want_model, general)
        elif entry == "ordered":
            assert order in (orr.NEAR_FIRST, orr.FAR_FIRST)
            p = plan("ordered", 0, n_buckets, want_model, general)
            k16 = orr.depth_key(s["pos"], s["cam"], orr.NEAR_FIRST)
            flip = orr.K_MAX if order == orr.FAR_FIRST else 0
            depth = flip - k16 if flip else k16
            key = (bucket << 16) | depth
            if mutant == "far_first_flips_whole_key" and flip:
                key = (((n_buckets - 1) << 16) | flip) - ((bucket << 16) | k16)
            keys0 = _key_words(bucket, key)
            _ordered_edges(bucket, depth, k16, s, keys0, order, edges)
        else:
            assert entry == "sorted"
            metric, sorder, depth_bits, axis = sort
            p = plan("sorted", 0, metric == sr.VIEW_AXIS, depth_bits, want_model, general)
            u = sr.depth_u(s["pos"], s["cam"], metric, axis)
            shift = 32 - depth_bits
            kk = u >> shift
            depth = (sr.U_MAX[metric] >> shift) - kk if sorder == sr.FAR_FIRST else kk
            keys0 = _key_words(bucket, depth)
            _sorted_edges(u[bucket >= 0], depth[bucket >= 0], s, depth_bits, edges)

    several = p["several"]
    stage = _Stage(p, n, BINS if several else n_buckets, scratch, mutant, edges)
    if not several and n_buckets in (1, 2, 255, 256) and bucket[0] == n_buckets - 1 and (bucket == n_buckets - 1).sum() == 1:
        edges.add(f"n_bins={n_buckets}_last_bucket_by_instance_0_only")
    ordered_key = entry == "ordered"
    holder = {}
    room = min(n_buckets, n) + 3

    def hist_of(keys, tiles):
        b = keys.astype(np.int64) >> 16 if ordered_key and mutant != "ordered_bucket_of_is_key" else keys.astype(np.int64)
        return np.bincount(b[b < n_buckets], minlength=n_buckets)     # (the mutant's adds land far outside the histogram: the model drops them)

    def members_of(totals0, hist):
        kind = p["pass"][0]["launch"][2][0]
        if kind == "sorted_members":                                   # the sum of pass 0's 256 digit totals
            holder["members"] = int(np.asarray(totals0).sum())
            return holder["members"]
        h = hist if several else np.asarray(totals0, np.int64)
        assert kind == {"draws": "pair", "shard": "shard"}.get(entry, "chain")
        if kind == "shard":
            holder["totals"] = h
            return int(h.sum())
        holder["cmds"], holder["count"], holder["members"] = commands(h, n_buckets, draw, meshes, room, mutant, edges)
        return holder["members"]

    out_ids, slot_of, _, _, members = stage.run(keys0, lambda idx: idx, kinds, hist_of, members_of, lambda k: np.int64(int(base) & 0xFFFFFFFF))
    _multi_pass_edges(p, keys0, edges)
    if several and n == 2049:
        live = int((keys0 != NONE).sum())
        if live in (0, 1, 1023, 1024, 1025, n):
            edges.add(f"members={'N' if live == n else live}_of_2049")
    if entry == "shard":
        _writer_edges(np.asarray(holder["totals"][:n_buckets], np.int64), [int(np.asarray(holder["totals"][f: f + CHUNK]).sum()) for f in range(0, n_buckets, CHUNK)], edges)
        chunk, members = shard_chunk(holder["totals"], n_buckets, _ids_buffer(out_ids, capacity))
        return dict(chunk=chunk), edges
    ids = _ids_buffer(out_ids, n + 3)
    if entry == "sorted":                                              # the run stage (not this model's subject): one command per run
        members = holder["members"]
        order_of = ((ids[:members].astype(np.int64) - int(base)) & 0xFFFFFFFF)
        sb = bucket[order_of[order_of < n]]
        heads = [k for k in range(len(sb)) if k == 0 or sb[k] != sb[k - 1]]
        cmds = np.full((n + 3, CMD_WORDS), SENTINEL, np.uint32)
        if heads:
            cmds[: len(heads)] = _rows(chain_draw, meshes, sb[heads], np.diff(heads + [len(sb)]), np.asarray(heads, np.int64))
        out = dict(cmds=cmds, count=len(heads), ids=ids, members=members)
    else:
        out = dict(cmds=holder["cmds"], count=holder["count"], ids=ids, members=holder["members"])
    if slot_of is not None:
        out["slot_of"] = slot_of
        edges.add("slot_of_for_the_model_kernel")
    return out, edges


def _multi_pass_edges(p, keys0, edges):
    live = keys0[keys0 != NONE].astype(np.int64)
    if not p["several"] or len(live) == 0:
        return
    digits = [np.unique((live >> io["shift"]) & 255) for io in p["pass"]]
    edges.add(f"passes={p['passes']}")
    if len(digits[0]) == 1 and any(len(d) > 1 for d in digits[1:]):
        edges.add(f"low_digit_equal_high_digits_differ_passes={p['passes']}")
    if len(digits[0]) > 1 and all(len(d) == 1 for d in digits[1:]):
        edges.add(f"high_digits_equal_low_digit_differs_passes={p['passes']}")


def _ordered_edges(bucket, depth, k16, s, keys0, order, edges):
    live = bucket >= 0
    tag = "near" if order == orr.NEAR_FIRST else "far"
    nan = np.isnan(s["pos"]).any(axis=1)
    if (live & (k16 == 0)).any():
        edges.add(f"K=0_{tag}_first")
    if (live & (k16 == orr.K_MAX) & ~nan).any():
        edges.add(f"K=0x7F80_{tag}_first")
    if (live & nan).any():
        edges.add(f"K_of_NaN_{tag}_first")
    if (keys0 == 0xFFFF7F80).any():
        edges.add("largest_ordered_key")
    pairs = set(zip(bucket[live].tolist(), depth[live].tolist()))
    by_d, by_b = {}, {}
    for b, d in pairs:
        by_d.setdefault(d, set()).add(b)
        by_b.setdefault(b, set()).add(d)
    if any(len(v) > 1 for v in by_d.values()):
        edges.add("two_buckets_same_D")
    for ds in by_b.values():
        ds = sorted(ds)
        if len(ds) == 2 and (ds[0] ^ ds[1]) < 256:
            edges.add("one_bucket_D_differs_in_digit_0_only")
        if len(ds) == 2 and (ds[0] ^ ds[1]) & 0xFF == 0:
            edges.add("one_bucket_D_differs_in_digit_1_only")


def _sorted_edges(u, depth, s, depth_bits, edges):
    ds = np.unique(depth)
    if len(ds) == 2:
        x = int(ds[0] ^ ds[1])
        for k in range(depth_bits // 8):
            if x and x & ~(0xFF << (8 * k)) == 0:
                edges.add(f"sorted_D_differs_in_digit_{k}_only_bits={depth_bits}")
    if len(np.unique(u)) > len(ds):
        edges.add(f"sorted_ties_below_the_sorted_bits_bits={depth_bits}")
    x = s["pos"][:, 0]
    special = {0x007FFFFF, 0x7FFFFFFE, 0x80000000, 0x80000001, 0xFF800000}
    if special <= set(u.tolist()) and np.isnan(x).any() and (np.signbit(x) & (x == 0)).any() and (~np.signbit(x) & (x == 0)).any():
        edges.add(f"sorted_zeros_subnormals_infinities_nan_bits={depth_bits}")
