"""Designed triangle streams for the range kernel and the size-class sort of the per-triangle stage, placed on every cut edge
(tests/range_model.py names them; tests/test_range_edge_cases.py asserts on the CPU that every name is hit and every mutant of
the model is killed; tests/test_gpu_range_edges.py runs them through mip_run).

The fixture: ONE mesh table of single-LOD meshes whose index_len is chosen per mesh, one geometry, every instance at identity,
in view and visible — so a command stream is just a mesh_id array, and one context serves every case through set_instances.
Triangle t of a mesh uses vertices 3 t .. 3 t + 2 of the mesh's own: a small front-facing triangle inside the frustum (kept), or
the same with two corners swapped (culled). The keep decision of every triangle is therefore DESIGNED (PATTERNS); the oracle
agrees (test_range_edge_cases.py), so the expectations are hand-written and the oracle's at once.

Sizes are derived from S as the probe (tests/native/frame_plan_probe.cpp) prints it; the cases pin n_waves with
MIP_TUNE_TRI_RANGE_BLOCKS=1 (four waves) and never look at the CU count."""
import copy
import json
import subprocess

import numpy as np

import plan_boundaries as pb
import range_model as rm
import triangle_cases as tc

F, U32 = np.float32, np.uint32
N_WAVES = 4                      # MIP_TUNE_TRI_RANGE_BLOCKS=1: one workgroup of four waves
PATTERNS = ("all", "none", "alternating", "lane63", "first", "last", "random")

# the contexts the cases run in (tuning variables, read by mip_create)
TUNINGS = {
    "ranges_256": {"MIP_TUNE_TRI_RANGE_BLOCKS": "1", "MIP_TUNE_TRI_RANGE_SLOTS": "256"},
    "ranges_8192": {"MIP_TUNE_TRI_RANGE_BLOCKS": "1", "MIP_TUNE_TRI_RANGE_SLOTS": "8192"},
    # the large-frame stage kernel (one grid, either body): its range body forced, and its wave-per-command body over the sorted list
    "stage_ranges_256": {"MIP_TUNE_TRI_RANGE_BLOCKS": "1", "MIP_TUNE_TRI_RANGE_SLOTS": "256", "MIP_TUNE_TRI_BLOCK_MAX": "0", "MIP_TUNE_TRI_CHOICE": "block"},
    "sorted": {"MIP_TUNE_TRI_RANGE_BLOCKS": "1", "MIP_TUNE_TRI_BLOCK_MAX": "0", "MIP_TUNE_TRI_CHOICE": "waves"},
}
TICKET_SLOTS = {"ranges_256": 256, "ranges_8192": 8192, "stage_ranges_256": 256, "sorted": 4096}
TUNING_VARIABLES = sorted({k for t in TUNINGS.values() for k in t})


def rules(total=0, n_waves=N_WAVES, ticket_slots=4096, index_counts=(), **state):
    """The probe's rules line: range_slots(total, n_waves, ticket_slots), its limits, the batch of every class, the class of
    every index count (asked in pieces: a command line has its limits)."""
    out = None
    ics = [int(x) for x in index_counts]
    classes = []
    for at in range(0, max(len(ics), 1), 2000):
        piece = ics[at : at + 2000]
        arg = f"rules={int(total)}:{int(n_waves)}:{int(ticket_slots)}" + (":" + ",".join(map(str, piece)) if piece else "")
        res = subprocess.run([pb.probe_exe()] + [f"{k}={v}" for k, v in state.items()] + [arg], capture_output=True, text=True, timeout=120, check=True)
        out = json.loads(res.stdout)
        classes += out["size_class"]
    out["size_class"] = classes
    return out


def keep_pattern(name, n, seed=0):
    """The designed decision of every triangle of a mesh of n triangles."""
    k = np.zeros(n, bool)
    if name == "all":
        k[:] = True
    elif name == "alternating":
        k[::2] = True
    elif name == "lane63":
        k[63::64] = True
    elif name == "first":
        k[:1] = True
    elif name == "last":
        k[-1:] = True
    elif name == "random":
        k[:] = np.random.default_rng(1000 + seed).random(n) < 0.5
    else:
        assert name == "none", name
    return k


class MeshTable:
    """Meshes by (index_len, pattern, seed), registered as the cases ask for them."""

    def __init__(self):
        self.keys, self.ids = [], {}

    def mesh(self, index_len, pattern="random", seed=0):
        assert pattern in PATTERNS
        key = (int(index_len), pattern, int(seed) if pattern == "random" else 0)
        if key not in self.ids:
            self.ids[key] = len(self.keys)
            self.keys.append(key)
        return self.ids[key]

    def vertex_offset(self, mesh_id):
        return sum(-(-k[0] // 3) * 3 for k in self.keys[:mesh_id])

    def index_len(self, mesh_id):
        return self.keys[mesh_id][0]

    def keep(self, mesh_id):
        n, pattern, seed = self.keys[mesh_id]
        return keep_pattern(pattern, n // 3, seed)

    def build(self, ra):
        """(mesh table, vertices, indices): mesh m's indices are 0 .. index_len - 1 over its own vertices; every mesh starts at
        a multiple of 3 in both buffers (a triangle is read at index_offset / 3 + t)."""
        kept_tri = np.array(tc.tri(0, 1, 12), F)
        culled_tri = np.array(tc.swapped(tc.tri(0, 1, 12)), F)
        meshes = np.zeros(len(self.keys), ra.MESH_DTYPE)
        vs, ixs = [], []
        v_off = 0
        for m, (n, pattern, seed) in enumerate(self.keys):
            keep = self.keep(m)
            v = np.where(keep[:, None, None], kept_tri[None], culled_tri[None]).reshape(-1, 3)
            room = -(-n // 3) * 3
            v = np.concatenate([v, np.tile(kept_tri[:1], (room - 3 * (n // 3), 1))]).astype(F)   # (the one or two indices behind the last triangle)
            meshes["aabb_min"][m], meshes["aabb_max"][m] = (-1, -1, -1), (1, 1, 1)
            meshes["n_lods"][m], meshes["index_len"][m, 0], meshes["index_offset"][m, 0], meshes["vertex_offset"][m] = 1, n, v_off, v_off
            vs.append(v), ixs.append(np.arange(room, dtype=U32))
            v_off += room
        vs.append(np.array(kept_tri[:1], F))   # (never empty)
        return meshes, np.concatenate(vs), np.concatenate(ixs + [np.zeros(1, U32)])


def scene_of(ra, meshes, mesh_ids):
    """The scene of one stream: identity instances under planes nothing fails."""
    n = len(mesh_ids)
    return dict(n=n, pos=np.zeros((n, 3), F), rot=np.tile(np.array([0, 0, 0, 1], F), (n, 1)), scale=np.ones(n, F),
                mesh_id=np.asarray(mesh_ids, U32), meshes=meshes, planes=np.tile(np.array([0, 0, 0, -1], F), 6), cam_pos=np.zeros(3, F))


class Case:
    def __init__(self, name, tuning, table, commands, base=0, short_by=None):
        """commands: [(triangles or ("ic", index count), pattern)]; short_by: the capacity is the frame's end minus this."""
        self.name, self.tuning, self.table, self.base = name, tuning, table, int(base)
        ids = []
        for k, (size, pattern) in enumerate(commands):
            ic = int(size[1]) if isinstance(size, tuple) else 3 * int(size)
            ids.append(table.mesh(ic, pattern, seed=k % 7))
        self.mesh_ids = np.array(ids, U32)                                # one instance per entry ...
        # ... and one command per instance whose mesh has an index at all (the first compaction keeps indexCount > 0: an instance
        # of an index-less mesh is in the scene and emits nothing)
        self.instances = np.array([i for i, m in enumerate(ids) if table.index_len(m) > 0], np.int64)
        self.cmd_meshes = self.mesh_ids[self.instances] if len(ids) else self.mesh_ids
        self.stream = rm.Stream([table.index_len(m) for m in self.cmd_meshes], base)
        self.end = self.base + self.stream.index_total                    # the frame's end in the index buffer
        self.capacity = self.end + 3 if short_by is None else self.end - int(short_by)
        self.status = 0 if short_by is None else -4
        self.sorted = tuning == "sorted"
        self.S = None if self.sorted else rules(self.stream.total, N_WAVES, TICKET_SLOTS[tuning])["range_slots"]

    @property
    def keeps(self):
        return [self.table.keep(m) for m in self.cmd_meshes]

    def words(self):
        """(lowest word of the index buffer the frame may touch, words to allocate from there): the whole buffer from word 0, or,
        for a first_index_base that no test could allocate up to, the frame's own part."""
        lo = 0 if self.base < (1 << 28) else self.base // 3 * 3
        return lo, max(self.end, self.capacity) - lo + 64

    def decompose(self, mutant=None):
        lo, n = self.words()
        S = self.S
        if mutant == "range_slots_not_rounded":
            r = rules()
            S = rm.range_slots_unrounded(self.stream.total, N_WAVES, TICKET_SLOTS[self.tuning], r["range_min_slots"])
        return rm.decompose(self.stream, self.keeps, S, N_WAVES, self.capacity, window=(lo, n), mutant=None if mutant == "range_slots_not_rounded" else mutant)

    def sort(self, mutant=None):
        r = rules(index_counts=self.stream.ic)
        return rm.sort_decompose(self.stream.ic, r["size_class"], r["sort_batch"], mutant)

    def expected(self):
        """(final index count per command, the buffer from words()[0] on) — hand-written from the design."""
        lo, n = self.words()
        return rm.expected_direct(self.stream, self.keeps, self.capacity, window=(lo, n))

    def expected_cmds(self, ra, first_instance_base=0):
        """The compacted list the frame ends with."""
        final, _ = self.expected()
        live = np.nonzero(final)[0]
        cmds = np.zeros(len(live), ra.DRAW_CMD_DTYPE)
        cmds["indexCount"] = final[live]
        cmds["instanceCount"] = 1
        cmds["firstIndex"] = self.stream.first_index[live]
        cmds["vertexOffset"] = [self.table.vertex_offset(int(self.cmd_meshes[c])) for c in live]
        cmds["firstInstance"] = first_instance_base + self.instances[live]
        return cmds


def _spanning(S, spans, last):
    """[head, the command, tail]: the command starts at slot 100 and spans `spans` ranges, its last segment of `last` triangles."""
    return [(100, "all"), ((spans - 1) * S + last - 100, "random"), (50, "alternating")]


def build_catalogue():
    """Every case, by name. S256 / S8192: the limits of range_slots as the probe prints them."""
    r = rules()
    lo_S, hi_S, batch = r["range_min_slots"], r["range_max_slots"], r["sort_batch"]
    t = MeshTable()
    cases = []

    def add(name, commands, tuning="ranges_256", **kw):
        cases.append(Case(name, tuning, t, commands, **kw))

    S = lo_S
    # ---- where a command ends and starts relative to a boundary; commands of S - 1, S, S + 1 triangles, aligned and not ----
    add("boundary_ends_and_lengths", [(S, "random"), (S - 1, "random"), (1, "all"), (S + 1, "random"), (100, "alternating"), (S, "random"), (S - 1, "lane63"),
                                      (S + 1, "random"), (S - 103, "all"), (S, "all"), (7, "first")])
    add("boundary_ends_and_lengths_base_5", [(S, "random"), (S - 1, "random"), (1, "all"), (S + 1, "random"), (100, "alternating"), (S, "random"), (S - 1, "lane63"),
                                             (S + 1, "random"), (S - 103, "all"), (S, "all"), (7, "first")], base=5)
    # ---- a command over 2 .. 130 ranges: the look-back in one, exactly one and several groups of 64 ----
    for spans in (2, 3, 64, 65, 66, 128, 129, 130):
        add(f"spans_{spans}_last_1", _spanning(S, spans, 1))
        add(f"spans_{spans}_last_S", _spanning(S, spans, S))
    # ---- continuing segments of 1, 63, 64 and 65 triangles ----
    add("continuing_1_63_64_65", [(200, "random"), (S - 200 + 1, "random"), (S - 1 + 63, "random"), (S - 63 + 64, "lane63"), (S - 64 + 65, "random"), (30, "last")])
    # ---- n_ranges = n_waves - 1, n_waves, n_waves + 1; every range but the first continues a command ----
    for k, name in ((N_WAVES - 1, "n_waves-1"), (N_WAVES, "n_waves"), (N_WAVES + 1, "n_waves+1")):
        add(f"n_ranges_{name}", [(150, "random")] + [(S, "random")] * (k - 1) + [(S - 150 - 9, "alternating")])
    # ---- commands of 0, 1 and 2 indices; index counts 3 k + 1 and 3 k + 2 ----
    nothing = [(("ic", 0), "none"), (("ic", 1), "none"), (("ic", 2), "none")]
    add("zero_runs_at_a_range_start", nothing + [(S - 1, "random")] + nothing * 2 + [(100, "random")] + nothing + [(S - 100 - 3, "all"), (40, "random")] + nothing)
    add("zero_run_across_a_boundary", [(200, "random")] + [(("ic", 2), "none")] * 120 + [(300, "random"), (20, "all")])
    add("zero_run_over_a_whole_range", [(100, "random")] + [(("ic", 2), "none")] * ((3 * (2 * S - 100) + 30) // 2) + [(300, "random"), (20, "all")])
    for rem in (1, 2):
        add(f"index_count_3k+{rem}_gap_holds_the_boundary", [(("ic", 3 * 100 + 2), "random"), (("ic", 3 * (S - 100) + rem), "random"), (300, "random"), (("ic", 3 * 55 + rem), "all"), (150, "random")])
    add("gaps_in_front_of_a_crossing_command", [(("ic", 3 * 10 + 2), "random")] * 60 + [(160, "random"), (50, "all")], base=5)
    # ---- first_index_base within 3 S of the end of 32 bits (the stream ends below it) ----
    add("base_near_the_end_of_32_bits", [(100, "random"), (("ic", 3 * 60 + 2), "all"), (80, "alternating")], base=(1 << 32) - 3 * S + 9)
    # ---- one command alone ----
    add("one_command_shorter_than_a_range", [(100, "random")])
    add("one_command_of_one_range", [(S, "random")])
    add("one_command_of_130_ranges", [(130 * S, "random")])
    # ---- granules of 0 and S; a command without a survivor between kept neighbours ----
    add("granules_0_and_S", [(100, "all"), (S - 100 + 2 * S + 44, "all"), (300, "none"), (100, "all"), (20, "none"), (77, "all"), (2 * S, "none"), (5, "last")])
    # ---- capacity: the command that does not fit continues from an earlier range / is the last to start in its range ----
    add("overflow_of_a_continuing_command", [(100, "random"), (300, "random"), (200, "random")], short_by=1)
    add("overflow_of_the_last_command_to_start", [(300, "random"), (100, "random"), (50, "all")], short_by=1)

    # ---- S between the limits (one range per wave): continuing segments of 11, 12, 13, 24, 25 steps ----
    S = 26 * 64
    add("continuing_11_12_13_steps", [(1000, "random"), (S - 1000 + 700, "random"), (2 * S - (S + 700) + 768, "random"), (3 * S - (2 * S + 768) + 832, "lane63"),
                                      (4 * S - (3 * S + 832), "random")], tuning="ranges_8192")
    add("continuing_24_25_steps", [(100, "all"), (S - 100 + 1536, "random"), (2 * S - (S + 1536) + 1600, "random"), (4 * S - (2 * S + 1600) - 100, "random")], tuning="ranges_8192")
    # ---- S at its upper limit: continuing segments of 128 and 127 steps (a full mask buffer, a full batch tail) ----
    S = hi_S
    add("continuing_128_127_steps_at_the_largest_S", [(64, "all"), (S - 64 + S + 8100, "random"), (5000, "random"), (5000, "alternating")], tuning="ranges_8192")

    # ---- the range body inside the large-frame stage kernel: the same streams ----
    for c in [c for c in cases if c.tuning == "ranges_256"]:
        twin = copy.copy(c)
        twin.name, twin.tuning = "stage:" + c.name, "stage_ranges_256"
        cases.append(twin)

    # ---- the size-class sort ----
    for name, ks in (("k_0_to_14", range(0, 15)), ("k_15", (15,)), ("k_16", (16,))):
        add(f"sorted_powers_of_two_{name}", [(n, "random") for k in ks for n in ((1 << k) - 1, 1 << k, (1 << k) + 1)], tuning="sorted")
    add("sorted_single_class", [(40 + (7 * k) % 24, "random") for k in range(37)], tuning="sorted")
    add("sorted_every_class_0_to_16", [(1 << k, "random") for k in (3, 16, 0, 9, 12, 1, 15, 5, 10, 2, 14, 7, 11, 4, 13, 6, 8)], tuning="sorted")
    class_of_batch = {b: min(k for k in range(17) if batch[k] == b) for b in (16, 8, 4, 2, 1)}
    for name, pop in (("batch-1", lambda b: b - 1), ("batch", lambda b: b), ("batch+1", lambda b: b + 1), ("2batch+1", lambda b: 2 * b + 1)):
        commands = []
        for b, k in class_of_batch.items():
            commands += [((1 << k) + (j % 3 if k else 0), "random") for j in range(pop(b))]
        order = np.random.default_rng(5).permutation(len(commands))
        add(f"sorted_class_populations_{name}", [commands[j] for j in order], tuning="sorted")
    add("sorted_more_than_2048_commands", [(("ic", (k * 37) % 120), "random") for k in range(8 * 256 + 261)], tuning="sorted")
    return t, cases


_CATALOGUE = None


def catalogue():
    """(mesh table, {name: case}) — built once."""
    global _CATALOGUE
    if _CATALOGUE is None:
        t, cases = build_catalogue()
        assert len({c.name for c in cases}) == len(cases)
        _CATALOGUE = (t, {c.name: c for c in cases})
    return _CATALOGUE


def cases_of(tuning):
    return [c for c in catalogue()[1].values() if c.tuning == tuning]


# Sequences on one context: streams of different lengths back to back (a granule or a sort word left by the previous frame must
# not be taken): (tuning, [case names])
SEQUENCES = [
    ("ranges_256", ["spans_130_last_1", "continuing_1_63_64_65", "spans_130_last_1", "one_command_shorter_than_a_range", "spans_66_last_S", "granules_0_and_S"]),
    ("stage_ranges_256", ["stage:spans_130_last_1", "stage:continuing_1_63_64_65", "stage:spans_130_last_1"]),
    ("sorted", ["sorted_more_than_2048_commands", "sorted_single_class", "sorted_more_than_2048_commands", "sorted_class_populations_2batch+1", "sorted_single_class"]),
    # a context whose FIRST frame overflows (its range map is sized by the short buffer), complete frames between and after the
    # short ones: the context stays usable, and nothing an overflowed frame left resurfaces
    ("ranges_256", ["overflow_of_a_continuing_command", "spans_3_last_S", "overflow_of_the_last_command_to_start", "spans_130_last_1",
                    "overflow_of_a_continuing_command", "granules_0_and_S"]),
]
LONG_LOOKBACK = [f"spans_{n}_last_{last}" for n in (65, 66, 128, 129, 130) for last in ("1", "S")] + ["one_command_of_130_ranges"]

# every edge the catalogue must hit (range_model.range_edges / sort_decompose name them)
RANGE_EDGES = (
    ["command_ends_on_a_boundary", "command_ends_one_short_of_a_boundary", "command_ends_one_past_a_boundary", "command_starts_on_a_boundary"]
    + [f"command_of_{n}_{a}" for n in ("S", "S-1", "S+1") for a in ("aligned", "misaligned")]
    + [f"spans_{n}_ranges" for n in (2, 3, 64, 65, 66, 128, 129, 130)] + ["last_segment_of_1", "last_segment_of_S"]
    + ["lookback_in_one_group", "lookback_of_exactly_one_group", "lookback_in_several_groups", "lookback_last_group_of_one_range"]
    + [f"continuing_segment_of_{n}_triangles" for n in (1, 63, 64, 65)] + [f"continuing_segment_of_{n}_steps" for n in (11, 12, 13, 24, 25, 127, 128)]
    + ["both_mask_buffers_live", "n_ranges=n_waves-1", "n_ranges=n_waves", "n_ranges=n_waves+1", "one_range_per_wave", "ranges_pulled_from_the_counter",
       "pending_segment_written_in_the_iteration_that_walks_nothing"]
    + ["command_of_1_indices", "command_of_2_indices", "zero_triangle_run_at_a_range_start", "zero_triangle_run_across_a_boundary",
       "zero_triangle_run_over_a_whole_range", "index_count_3k+1_in_front_of_a_boundary", "index_count_3k+2_in_front_of_a_boundary"]
    + ["base=0", "base=odd", "base=high", "S=256", "S=1664", "S=8192"]
    + ["one_command_shorter_than_a_range", "one_command_of_one_range", "one_command_of_130_ranges"]
    + ["granule_0", "granule_S", "command_without_survivor_between_kept_neighbours", "overflow_of_a_continuing_command",
       "overflow_of_the_last_command_to_start_in_a_range"])
SORT_EDGES = (
    [f"command_of_{n}_k={k}" for k in range(17) for n in ("2^k-1", "2^k", "2^k+1")] + [f"class_{k}_occupied" for k in range(17)]
    + ["frame_of_a_single_class", "every_class_0_to_16_occupied", "one_histogram_copy_serves_two_workgroups", "zero_triangle_commands_share_class_0"]
    + [f"class_population_{p}_at_batch_{b}" for b in (16, 8, 4, 2, 1) for p in ("batch-1", "batch", "batch+1", "2batch+1") if not (b == 1 and p == "batch-1")])
