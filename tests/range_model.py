"""A CPU model of how the per-triangle stage DECOMPOSES a frame's triangle stream (renderer_amd/csrc/triangle_kernels.hpp): the range
kernel — range -> first command map, segments, which segment of which range continues a command, granules, look-backs, steps per
deferred write, final_index_count — and the size-class sort in front of the wave-per-command body — class order, histogram copies,
tickets and batches. It is given the commands' index counts, first_index_base, S and n_waves (S is READ from frame_plan.hpp through
tests/native/frame_plan_probe.cpp: tests/range_edge_cases.py) and every triangle's keep decision, reassembles the culled stream
from them, and says which structural EDGES the stream hits. `expected_direct` states the same stream without any decomposition;
the two agree for every case (tests/test_range_edge_cases.py), and every MUTANT — one mistake in the decomposition each — changes
the stream or the counts of a named case. No GPU."""
import numpy as np

U32 = np.uint32
SENTINEL = 0xFFFFFFFF
STEP = 64            # triangles per step of a walk
BATCH = 12           # steps per batch of the deferred write (kBatch)
MASK_STEPS = 128     # keep masks per wave and buffer (kRangeMaskSteps)
GROUP = 64           # granules per round trip of the look-back
SORT_COPIES = 8      # histogram copies of the size-class sort (kSortCopies)
SORT_BLOCK = 256     # commands per workgroup of the sort kernels

RANGE_MUTANTS = ("ends_here_strict", "lookback_first_range_ceiling", "lookback_nearest_group_only", "granule_of_first_segment",
                 "prev_end_without_gaps", "range_slots_not_rounded", "batch_tail_dropped", "mask_buffers_aliased")
SORT_MUTANTS = ("ticket_past_class_end", "class_of_power_of_two_low", "copy_offsets_ignored")
MUTANTS = RANGE_MUTANTS + SORT_MUTANTS


def range_slots_unrounded(total, n_waves, ticket_slots, min_slots):
    """The mutant of range_slots that forgets the whole steps of 64 (the rule itself is read from the probe, never restated)."""
    one = -(-total // n_waves)
    if one <= ticket_slots:
        return max(one, min_slots)
    return ticket_slots


class Stream:
    """The commands of one frame as the instance kernel emits them: index counts in list order, firstIndex their running sum from
    first_index_base on; command c owns the slots [slot0, slot0 + index_count // 3)."""

    def __init__(self, index_counts, base):
        self.ic = np.asarray(index_counts, np.int64)
        self.base = int(base)
        self.first_index = self.base + np.concatenate([[0], np.cumsum(self.ic)[:-1]]) if len(self.ic) else np.zeros(0, np.int64)
        assert len(self.ic) == 0 or int(self.first_index[-1] + self.ic[-1]) <= 0xFFFFFFFF, "the catalogue's streams never wrap firstIndex"
        self.n_tris = self.ic // 3
        self.slot0 = (self.first_index - self.base) // 3
        self.end = self.slot0 + self.n_tris
        self.total = int(self.end[-1]) if len(self.ic) else 0       # stream_slots: from the LAST command
        self.index_total = int(self.ic.sum())

    def __len__(self):
        return len(self.ic)


def _buffer(capacity, window):
    """The index buffer as the model keeps it: (words, first word) — the whole buffer, or the `window` (first word, words) of it."""
    lo, n = window if window is not None else (0, capacity)
    return np.full(int(n), SENTINEL, np.int64), int(lo)


def _write(buf, first_index, position, tris, origin=0):
    """Survivors `tris` (triangle numbers of the mesh: triangle t names vertices 3 t .. 3 t + 2) from the command's place on."""
    at = (int(first_index) // 3 + int(position)) * 3 - origin
    assert at >= 0
    t = np.asarray(tris, np.int64)
    words = (3 * t[:, None] + np.arange(3)[None, :]).reshape(-1)[: max(len(buf) - at, 0)]   # (a mutant may run off the buffer: the model stops there)
    buf[at : at + len(words)] = words


def expected_direct(stream, keeps, capacity, window=None):
    """From the design alone, no decomposition: (final index count per command, the whole buffer of `alloc` words). A command
    whose frame range does not fit `capacity` writes nothing and ends with no indices (include/mi_instance_pipeline.h)."""
    buf, origin = _buffer(capacity, window)
    final = np.zeros(len(stream), np.int64)
    for c in range(len(stream)):
        if int(stream.first_index[c] + stream.ic[c]) > capacity:
            continue
        kept = np.nonzero(keeps[c])[0]
        final[c] = 3 * len(kept)
        _write(buf, stream.first_index[c], 0, kept, origin)
    return final, buf.astype(U32)


def range_first_cmd(stream, S, n_ranges, mutant=None):
    """mip_triangle_prepare_kernel: command c takes every range whose first slot lies in [end of c - 1, end of c) (a later
    command's store wins where a mutant lets two claim one range: the model runs the threads in order)."""
    first = np.full(n_ranges, len(stream), np.int64)
    dense_end = np.cumsum(stream.n_tris)
    for c in range(len(stream)):
        prev_end = 0 if c == 0 else int(stream.end[c - 1])
        if mutant == "prev_end_without_gaps" and c:
            prev_end = int(dense_end[c - 1])
        for b in range(-(-prev_end // S), min(-(-int(stream.end[c]) // S), n_ranges)):
            first[b] = c
    return first


def decompose(stream, keeps, S, n_waves, capacity, window=None, mutant=None):
    """triangle_ranges_body over the whole stream. Returns a dict: n_ranges, first (range -> first command), segments (per range:
    [(command, t_begin, t_end, ends_here, continues)]), granules, lookbacks (per continuing segment: range -> the groups of ranges
    it sums, nearest first), deferred_steps (range -> steps of its deferred write), final (final_index_count), stream (the
    whole buffer), edges (names)."""
    assert mutant is None or mutant in RANGE_MUTANTS
    total = stream.total
    n_ranges = -(-total // S) if len(stream) else 0
    first = range_first_cmd(stream, S, n_ranges, mutant)
    buf, origin = _buffer(capacity, window)
    final = np.zeros(len(stream), np.int64)      # (commands without a triangle, and commands that do not fit: the map kernel's zero)
    fits = [int(stream.first_index[c] + stream.ic[c]) <= capacity for c in range(len(stream))]
    segments, granules, pending = [], np.zeros(n_ranges, np.int64), {}
    first_survivors = np.zeros(n_ranges, np.int64)
    edges = set()
    for b in range(n_ranges):
        lo, hi = b * S, (b + 1) * S
        segs, last, first_seen = [], 0, None
        c = int(first[b])
        while c < len(stream):
            s0, nt = int(stream.slot0[c]), int(stream.n_tris[c])
            if s0 >= hi:
                break
            seg_lo, seg_hi = max(s0, lo), min(s0 + nt, hi)
            ends_here = s0 + nt < hi if mutant == "ends_here_strict" else s0 + nt <= hi
            if seg_lo < seg_hi:
                t_begin, t_end = seg_lo - s0, seg_hi - s0
                kept = np.nonzero(keeps[c][t_begin:t_end])[0] + t_begin
                continues = t_begin > 0
                segs.append((c, t_begin, t_end, ends_here, continues))
                if continues:
                    pending[b] = dict(c=c, t_begin=t_begin, t_end=t_end, ends=ends_here, kept=kept)
                else:
                    if fits[c]:
                        _write(buf, stream.first_index[c], 0, kept, origin)
                    if ends_here:
                        final[c] = 3 * len(kept) if fits[c] else 0
                last = len(kept)
                if first_seen is None:
                    first_seen = len(kept)
            if not ends_here:
                break
            c += 1
        segments.append(segs)
        granules[b] = last
        first_survivors[b] = first_seen or 0
    published = first_survivors if mutant == "granule_of_first_segment" else granules
    # which wave walks which range, for the one thing that depends on it (the two mask buffers): the static ranges, then the
    # tickets in order, dealt round robin — one schedule of many, all of which write the same stream unless the buffers alias
    wave_ranges = [[b for b in range(n_ranges) if b % n_waves == w] for w in range(n_waves)]
    lookbacks, deferred_steps = {}, {}
    for b, p in sorted(pending.items()):
        c = p["c"]
        s0 = int(stream.slot0[c])
        b0 = -(-s0 // S) if mutant == "lookback_first_range_ceiling" else s0 // S
        groups, hi = [], b
        while hi > b0:
            lo = hi - GROUP if hi - b0 > GROUP else b0
            groups.append(list(range(lo, hi)))
            hi = lo
            if mutant == "lookback_nearest_group_only":
                break
        lookbacks[b] = groups
        prefix = int(sum(published[j] for g in groups for j in g))
        n = p["t_end"] - p["t_begin"]
        n_steps = -(-n // STEP)
        deferred_steps[b] = n_steps
        kept = p["kept"]
        if mutant == "batch_tail_dropped" and n_steps % BATCH:
            kept = kept[kept < p["t_begin"] + (n_steps // BATCH) * BATCH * STEP]
        if mutant == "mask_buffers_aliased":
            mine = wave_ranges[b % n_waves]
            later = [x for x in mine if x > b]
            if later and later[0] in pending:   # the wave's next range has tested ITS continuing segment into the same buffer
                q = pending[later[0]]
                other = np.zeros(n_steps * STEP, bool)
                m = np.zeros(-(-(q["t_end"] - q["t_begin"]) // STEP) * STEP, bool)
                m[q["kept"] - q["t_begin"]] = True
                other[: min(len(other), len(m))] = m[: len(other)]
                other[n:] = False
                kept = np.nonzero(other)[0] + p["t_begin"]
        if fits[c]:
            _write(buf, stream.first_index[c], prefix, kept[: len(p["kept"])], origin)   # (the region descriptor spans p.survivors triangles)
        if p["ends"]:
            final[c] = 3 * (prefix + len(p["kept"])) if fits[c] else 0
    out = dict(S=S, n_ranges=n_ranges, first=first, segments=segments, granules=granules, lookbacks=lookbacks, deferred_steps=deferred_steps,
               final=final, stream=buf.astype(U32), wave_ranges=wave_ranges, pending=sorted(pending))
    out["edges"] = edges | range_edges(stream, keeps, out, n_waves, capacity)
    return out


def range_edges(stream, keeps, d, n_waves, capacity):
    """The structural edges a decomposed stream hits, by name (tests/range_edge_cases.EDGES lists every name there is)."""
    S, n_ranges = d["S"], d["n_ranges"]
    e = {f"S={S}", f"base={'0' if stream.base == 0 else ('high' if stream.base > 0xF0000000 else 'odd')}"}
    for c in range(len(stream)):
        s0, nt, end = int(stream.slot0[c]), int(stream.n_tris[c]), int(stream.end[c])
        if nt == 0:
            continue
        aligned = "aligned" if s0 % S == 0 else "misaligned"
        for k, name in ((0, "on"), (S - 1, "one_short_of"), (1, "one_past")):
            if end % S == k:
                e.add(f"command_ends_{name}_a_boundary")
        if s0 % S == 0:
            e.add("command_starts_on_a_boundary")
        for k, name in ((S, "S"), (S - 1, "S-1"), (S + 1, "S+1")):
            if nt == k:
                e.add(f"command_of_{name}_{aligned}")
        spans = (end - 1) // S - s0 // S + 1
        if spans >= 2:
            e.add(f"spans_{spans}_ranges")
            last = end - ((end - 1) // S) * S
            if last == 1:
                e.add("last_segment_of_1")
            if last == S:
                e.add("last_segment_of_S")
        if not keeps[c].any() and 0 < c < len(stream) - 1 and keeps[c - 1].any() and keeps[c + 1].any():
            e.add("command_without_survivor_between_kept_neighbours")
    if len(stream) == 1:
        nt = int(stream.n_tris[0])
        e.add("one_command_" + ("shorter_than_a_range" if nt < S else "of_one_range" if nt == S else f"of_{-(-nt // S)}_ranges"))
    for b, groups in d["lookbacks"].items():
        n = sum(len(g) for g in groups)
        e.add("lookback_in_one_group" if n < GROUP else "lookback_of_exactly_one_group" if n == GROUP else "lookback_in_several_groups")
        if len(groups) > 1 and len(groups[-1]) == 1:
            e.add("lookback_last_group_of_one_range")
    for b, segs in enumerate(d["segments"]):
        for (c, t_begin, t_end, ends, continues) in segs:
            if continues:
                n = t_end - t_begin
                e.add(f"continuing_segment_of_{n}_triangles")
                e.add(f"continuing_segment_of_{-(-n // STEP)}_steps")
                if b == n_ranges - 1 or (n_ranges <= n_waves):
                    e.add("pending_segment_written_in_the_iteration_that_walks_nothing")
        if segs and d["granules"][b] == 0:
            e.add("granule_0")
        if d["granules"][b] == S:
            e.add("granule_S")
    for mine in d["wave_ranges"]:
        for x, y in zip(mine, mine[1:]):
            if x in d["lookbacks"] and y in d["lookbacks"]:
                e.add("both_mask_buffers_live")
    if len(stream):
        for k, name in ((n_waves - 1, "n_waves-1"), (n_waves, "n_waves"), (n_waves + 1, "n_waves+1")):
            if n_ranges == k:
                e.add(f"n_ranges={name}")
        e.add("one_range_per_wave" if n_ranges <= n_waves else "ranges_pulled_from_the_counter")
    # runs of commands without a triangle, and the slot gaps that index counts 3 k + 1 / 3 k + 2 leave
    zero = stream.n_tris == 0
    for c in np.nonzero(zero)[0]:
        e.add(f"command_of_{int(stream.ic[c])}_indices")     # (1 or 2: a mesh without an index emits no command)
    c = 0
    while c < len(stream):
        if not zero[c]:
            c += 1
            continue
        c1 = c
        while c1 < len(stream) and zero[c1]:
            c1 += 1
        lo = int(stream.end[c - 1]) if c else 0                      # the slots the run's indices skip: [lo, hi)
        hi = int(stream.slot0[c1]) if c1 < len(stream) else int(stream.end[-1])
        if lo % S == 0 and c1 < len(stream):
            e.add("zero_triangle_run_at_a_range_start")
        if lo // S != hi // S and lo % S and hi % S:
            e.add("zero_triangle_run_across_a_boundary")
        if any(lo <= b * S and (b + 1) * S <= hi for b in range(n_ranges)):
            e.add("zero_triangle_run_over_a_whole_range")
        c = c1
    for c in range(len(stream) - 1):
        r = int(stream.ic[c]) % 3
        if r and stream.n_tris[c] and int(stream.end[c]) % S == 0 and int(stream.slot0[c + 1]) > int(stream.end[c]):   # the gap holds the boundary
            e.add(f"index_count_3k+{r}_in_front_of_a_boundary")
    if len(stream) and capacity < int(stream.first_index[-1] + stream.ic[-1]):
        unfit = [c for c in range(len(stream)) if int(stream.first_index[c] + stream.ic[c]) > capacity]
        c = unfit[0]
        if int(stream.slot0[c]) // S != (int(stream.end[c]) - 1) // S:
            e.add("overflow_of_a_continuing_command")
        if c == len(stream) - 1 and c > 0 and int(stream.slot0[c]) // S == int(stream.slot0[c - 1]) // S and int(stream.slot0[c]) % S:
            e.add("overflow_of_the_last_command_to_start_in_a_range")
    return e


# ---- the size-class sort in front of the wave-per-command body ---------------------------------------------------------------

def sort_decompose(index_counts, classes, batch_of_class, mutant=None):
    """triangle_sort_count_part + mip_triangle_sort_scatter_kernel + the ticket loop of triangle_waves_body. `classes`: the size
    class of every command and `batch_of_class`: commands per ticket of every class — both READ through the probe. Returns
    dict(start — position of rank d's class (largest first), order — the sorted list under one arrival order (by command
    number inside a copy), tickets [(rank, first, n_cmds)], visits — how often every command is walked, stale — places of
    `order` nobody wrote, edges)."""
    assert mutant is None or mutant in SORT_MUTANTS
    ic = np.asarray(index_counts, np.int64)
    count = len(ic)
    k_of = np.asarray(classes, np.int64).copy()
    if mutant == "class_of_power_of_two_low":
        nt = ic // 3
        pow2 = (nt > 1) & ((nt & (nt - 1)) == 0)
        k_of[pow2] -= 1
    copy_of = (np.arange(count) // SORT_BLOCK) % SORT_COPIES
    hist = np.zeros((SORT_COPIES, 32), np.int64)
    for c in range(count):
        hist[copy_of[c], k_of[c]] += 1
    total = hist.sum(axis=0)
    start, tickets_upto, batch = np.zeros(32, np.int64), np.zeros(32, np.int64), np.zeros(32, np.int64)
    at = upto = 0
    for d in range(32):                     # rank d: class 31 - d
        k = 31 - d
        batch[d] = batch_of_class[k]
        start[d] = at
        at += total[k]
        upto += -(-total[k] // batch[d])
        tickets_upto[d] = upto
    order = np.full(count + 64, -1, np.int64)   # (room behind the list: a mutant ticket may look there)
    cursor = np.zeros((SORT_COPIES, 32), np.int64)
    for c in range(count):                   # arrival order: by command number
        k, q = k_of[c], copy_of[c]
        below = 0 if mutant == "copy_offsets_ignored" else hist[:q, k].sum()
        order[start[31 - k] + below + cursor[q, k]] = c
        cursor[q, k] += 1
    tickets, visits = [], np.zeros(count, np.int64)
    stale = 0
    for ticket in range(int(tickets_upto[31])):
        d = int(np.searchsorted(tickets_upto[:31], ticket, side="right"))
        before = int(tickets_upto[d - 1]) if d else 0
        class_end = int(start[d + 1]) if d < 31 else count
        first = int(start[d]) + (ticket - before) * int(batch[d])
        n_cmds = int(batch[d]) if mutant == "ticket_past_class_end" else min(class_end - first, int(batch[d]))
        tickets.append((d, first, n_cmds))
        for c in order[first : first + n_cmds]:
            if c < 0:
                stale += 1
            else:
                visits[c] += 1
    pop = {int(k): int(total[k]) for k in range(32) if total[k]}
    edges = {f"class_{k}_occupied" for k in pop}
    for k, n in pop.items():
        b = int(batch_of_class[k])
        for want, name in ((b - 1, "batch-1"), (b, "batch"), (b + 1, "batch+1"), (2 * b + 1, "2batch+1")):
            if n == want and n > 0:
                edges.add(f"class_population_{name}_at_batch_{b}")
    if len(pop) == 1:
        edges.add("frame_of_a_single_class")
    if all(k in pop for k in range(17)):
        edges.add("every_class_0_to_16_occupied")
    if count > SORT_COPIES * SORT_BLOCK:
        edges.add("one_histogram_copy_serves_two_workgroups")
    if count and (ic < 3).any():
        edges.add("zero_triangle_commands_share_class_0")
    nt = ic // 3
    for k in range(17):
        for v, name in (((1 << k) - 1, "2^k-1"), (1 << k, "2^k"), ((1 << k) + 1, "2^k+1")):
            if (nt == v).any():
                edges.add(f"command_of_{name}_k={k}")
    return dict(start=start, batch=batch, order=order, tickets=tickets, visits=visits, stale=stale, population=pop, edges=edges)


def sorted_stream(stream, keeps, capacity, sort, window=None):
    """What the wave-per-command body over the sorted list leaves: every VISITED command's survivors (a command nobody visits
    keeps what the scratch held: reported as final -1)."""
    buf, origin = _buffer(capacity, window)
    final = np.full(len(stream), -1, np.int64)
    for c in np.nonzero(sort["visits"])[0]:
        if int(stream.first_index[c] + stream.ic[c]) > capacity:
            final[c] = 0
            continue
        kept = np.nonzero(keeps[c])[0]
        final[c] = 3 * len(kept)
        _write(buf, stream.first_index[c], 0, kept, origin)
    return final, buf.astype(U32)
