"""Designed member streams for the binning stage of the batched-draws family (renderer_amd/csrc/batch_kernel.hpp: count, rowscan,
scatter, a command writer) and, for every stream and entry point, the expectation BY CONSTRUCTION.

A case is a name, a table and pos / scale / mesh_id / a host bitmap that realise the case's own LABELS: bucket[i] (-1: not a
member, through a clear bitmap bit or a dead mesh with index_len 0), and for the depth-keyed calls K[i] (mip_batch_draws_ordered)
or the full 32-bit U[i] (mip_batch_draws_sorted). The generator writes the labels and then positions that realise them; nothing
here derives a label from a position. Tables hold single-level meshes (bucket == mesh_id) with index_len = 3 (k + 1) and
index_offset / vertex_offset distinct per mesh, or two-level meshes (bucket = 2 mesh + lod, the far bit realised by x = 100
against pick_lod's distance of 10) for mip_batch_draws. cam = 0, pos = (x, 0, 0), identity rotation, scale 1:

    ordered   x = (16 + j) / 16 * 2^a, so q = x * x = (16 + j)^2 * 2^(2a - 8) is exact and K = bits(q) >> 16 follows from (a, j)
              in integers (ordered_x); x = inf gives K = 0x7F80, x = NaN gives 0x7F80 too
    sorted    MIP_DEPTH_VIEW_AXIS with axis (1, 0, 0): z == x exactly, so x = from_bits(unflip(U)) realises any U (sorted_x)

The expectation by construction is Python's `sorted` over (bucket, i), (bucket, D, i), (D, i) or (view, bucket, i) of the labels
and one command per run of equal bucket in that order, its three table words read from the table row of the labelled bucket. No
numpy sort, none of the restatements' code. tests/test_batch_stage_cases.py holds it against the numpy restatements (which derive
bucket and depth from the positions by the float32 rules) and against tests/batch_stage_model.py, byte for byte;
tests/test_gpu_batch_stage.py holds the library against it. EDGES names every structural edge; every case claims the ones it was
designed for, and the model says which ones a call really touched."""
import functools
from collections import namedtuple

import numpy as np

from renderer_amd.pipeline import MESH_DTYPE

M32 = 0xFFFFFFFF
SENTINEL = 0x5A5A5A5A
PIN_SWITCH_SQ = (100.00000762939453125, float("inf"), float("inf"), float("inf"), float("inf"))   # mip_batch_draws' own rule
DISTANCE = 0
DRAW_INDEX, NEAR_FIRST, FAR_FIRST = 0, 1, 2
RADIAL, VIEW_AXIS = 0, 1
AXIS = (1.0, 0.0, 0.0)
K_MAX = 0x7F80
U_MAX_AXIS = 0xFF800000
K_ONE, U_ONE = 0x3F80, 0xBF800000        # of x = 1: every case that is not about depth keys
BASE = 0xFFFFFFF0                        # first_instance_base: ids wrap from instance 16 on
TILE = 1024
SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)

Call = namedtuple("Call", "entry model order sort", defaults=(False, None, None))
LODS, LODS_MODEL, SHARD, DRAWS, DRAWS_MODEL = Call("lods"), Call("lods", True), Call("shard"), Call("draws"), Call("draws", True)
ORDERED_NEAR, ORDERED_FAR = Call("ordered", False, NEAR_FIRST), Call("ordered", False, FAR_FIRST)
VIEWS = Call("views")


def sorted_call(order, bits):
    return Call("sorted", False, None, (VIEW_AXIS, order, bits, AXIS))


STAGE_CALLS = (LODS_MODEL, LODS, SHARD, ORDERED_NEAR, sorted_call(NEAR_FIRST, 16), VIEWS)

# ---- the edges: one list; tests/test_batch_stage_cases.py asserts that every one is hit and that every claim holds ----
EDGES = tuple(
    [f"N={n}" for n in SIZES] + ["idle_lanes_behind_member", "idle_lanes_behind_nonmember", "no_idle_lanes"]
    + ["round_of_one_digit", "round_of_64_digits", "digits_differ_in_bit_0_only", "digits_differ_in_bit_7_only",
       "clear_bit_beside_bucket_0", "dead_mesh_beside_bucket_0", "bin_in_rounds_0_and_3_only", "bin_in_waves_0_and_3_only",
       "bin_fills_a_tile", "empty_tile_between_tiles", "only_bins_63_and_64", "only_bins_127_and_128", "only_bins_191_and_192",
       "only_bins_0_and_255"]
    + [f"n_bins={b}_last_bucket_by_instance_0_only" for b in (1, 2, 255, 256)]
    + [f"n_tiles={t}" for t in (1, 255, 256, 257, 512, 513)]
    + ["bin_in_tile_0_and_256_only", "bin_in_tile_255_only", "bin_in_last_tile_only", "bin_first_chunk_zero", "bin_second_chunk_zero"]
    + ["passes=2", "passes=3", "passes=4", "low_digit_equal_high_digits_differ_passes=2", "high_digits_equal_low_digit_differs_passes=2",
       "low_digit_equal_high_digits_differ_passes=3", "high_digits_equal_low_digit_differs_passes=3",
       "only_buckets_255_and_256", "only_buckets_65535_and_65536", "buckets_255_and_256_used", "buckets_65535_and_65536_used", "last_bucket_used"]
    + [f"members={k}_of_2049" for k in (0, 1, 1023, 1024, 1025, "N")]
    + ["list_len_inside_a_round", "list_tiles_beyond_members_idle", "stale_keys_behind_members", "slot_of_for_the_model_kernel"]
    + ["only_buckets_511_and_512", "only_the_last_bucket", "every_bucket_one_member", "empty_bucket_chunk_between_chunks"]
    + [f"view_boundary_on_a_chunk_boundary_B={b}" for b in (128, 256, 512)]
    + ["view_first_members_two_chunks_later", "empty_view_first", "empty_view_in_the_middle", "empty_view_last"]
    + [f"n_views={v}" for v in (1, 2, 3, 15, 16)]
    + ["every_histogram_copy_used", "only_copy_63_for_a_bucket", "distinct_bases_one_wraps", "view_first_slot_given", "view_first_slot_null"]
    + [f"K=0_{t}_first" for t in ("near", "far")] + [f"K=0x7F80_{t}_first" for t in ("near", "far")] + [f"K_of_NaN_{t}_first" for t in ("near", "far")]
    + ["largest_ordered_key", "two_buckets_same_D", "one_bucket_D_differs_in_digit_0_only", "one_bucket_D_differs_in_digit_1_only"]
    + [f"sorted_D_differs_in_digit_{k}_only_bits={b}" for b in (16, 24, 32) for k in range(b // 8)]
    + ["sorted_ties_below_the_sorted_bits_bits=16", "sorted_ties_below_the_sorted_bits_bits=24"]
    + [f"sorted_zeros_subnormals_infinities_nan_bits={b}" for b in (16, 24, 32)])


# ---- tables ----

@functools.lru_cache(maxsize=None)
def table(name):
    """"S<m>": m single-level meshes; "S<m>d": the same with mesh 5 dead; "P<m>" / "P<m>d": two-level meshes. Bucket b of a table
    draws index_len 3 (b + 1); every offset is distinct."""
    levels = 1 if name[0] == "S" else 2
    dead = name.endswith("d")
    m = int(name[1:].rstrip("d"))
    t = np.zeros(m, MESH_DTYPE)
    t["aabb_min"], t["aabb_max"] = -0.5, 0.5
    t["n_lods"] = levels
    k = np.arange(m, dtype=np.int64)
    for lod in range(levels):
        t["index_len"][:, lod] = 3 * (levels * k + lod + 1)
        t["index_offset"][:, lod] = 1000 + 64 * k + 2_000_000 * lod
    t["vertex_offset"] = 3 * k - 100
    if dead:
        t["index_len"][5] = 0
    t.setflags(write=False)
    return t


def table_levels(name):
    return 1 if name[0] == "S" else 2


def dead_mesh(name):
    return 5 if name.endswith("d") else None


# ---- labels -> positions ----

def _f32(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


def ordered_x(a, j):
    """(x, K): x = (16 + j) / 16 * 2^a; q = x * x = (16 + j)^2 / 256 * 4^a exactly, so K = bits(q) >> 16 in integers."""
    assert 0 <= j < 16 and -40 <= a <= 40
    sq = (16 + j) ** 2
    exponent, top7 = (2 * a + 127, (sq - 256) // 2) if sq < 512 else (2 * a + 128, (sq - 512) // 4)
    return np.float32((16 + j) * 2.0 ** (a - 4)), (exponent << 7) | top7


def sorted_x(u):
    """x with U(x) == u under MIP_DEPTH_VIEW_AXIS, axis (1, 0, 0), cam 0: U = bits ^ 0x80000000 (sign clear), ~bits (sign set)."""
    assert 0 <= u <= U_MAX_AXIS and u != 0x7FFFFFFF      # (0x7FFFFFFF would be -0, whose U is +0's)
    return _f32(u ^ 0x80000000 if u & 0x80000000 else ~u & M32)


class Case:
    """One stream. bucket / non_kind are the labels (non_kind: 1 a clear bit, 2 a dead mesh with its bit set); K / U the depth
    labels; x realises them. views: dict(bucket=[V label arrays], bases, first_slot) for the several-view cases."""

    def __init__(self, name, family, table_name, bucket, non_kind=None, calls=STAGE_CALLS, edges=(), K=None, U=None, x=None, views=None,
                 far_x=True):
        self.name, self.family, self.table_name, self.calls, self.edges = name, family, table_name, tuple(calls), frozenset(edges)
        assert self.edges <= set(EDGES), self.edges - set(EDGES)
        self.table, self.levels = table(table_name), table_levels(table_name)
        self.bucket = np.asarray(bucket, np.int64)
        n = self.n = len(self.bucket)
        self.n_buckets = len(self.table) * self.levels
        assert n >= 1 and self.bucket.max(initial=-1) < self.n_buckets
        kind = np.ones(n, np.int64) if non_kind is None else np.asarray(non_kind, np.int64)
        self.non_kind = np.where(self.bucket >= 0, 0, kind)
        dead = dead_mesh(table_name)
        assert dead is not None or not (self.non_kind == 2).any()
        assert dead is None or not (self.bucket // self.levels == dead).any(), "a member of a dead mesh"
        live = [k for k in range(len(self.table)) if k != dead]
        i = np.arange(n)
        other = np.asarray(live, np.int64)[(i * 7) % len(live)]         # the mesh of an instance whose bit is clear
        self.mesh_id = np.where(self.bucket >= 0, self.bucket // self.levels, np.where(self.non_kind == 2, dead if dead is not None else 0, other)).astype(np.uint32)
        bits = self.non_kind != 1
        self.bitmap = np.packbits(np.r_[bits, np.zeros(-n % 32, bool)], bitorder="little").view(np.uint32).copy()
        self.K = np.full(n, K_ONE, np.int64) if K is None else np.asarray(K, np.int64)
        self.U = np.full(n, U_ONE, np.int64) if U is None else np.asarray(U, np.int64)
        xs = np.ones(n, np.float32) if x is None else np.asarray(x, np.float32)
        if self.levels == 2 and x is None:                                # the far bit of a pair bucket: beyond pick_lod's distance
            xs = np.where((self.bucket >= 0) & (self.bucket % 2 == 1), np.float32(100.0), np.float32(1.0)).astype(np.float32)
        self.pos = np.zeros((n, 3), np.float32)
        self.pos[:, 0] = xs
        self.scale = np.ones(n, np.float32)
        self.rot = np.zeros((n, 4), np.float32)
        self.rot[:, 3] = 1.0
        self.cam = np.zeros(3, np.float32)
        self.views = views
        if views is not None:
            for b in views["bucket"]:       # a view's non-members are clear bits of the view's own bitmap (or the shared dead mesh)
                b = np.asarray(b)
                assert len(b) == n and ((b < 0) | (b // self.levels == self.mesh_id)).all()

    def scene(self):
        return dict(n=self.n, pos=self.pos, rot=self.rot, scale=self.scale, mesh_id=self.mesh_id, meshes=self.table, bitmap=self.bitmap,
                    cam=self.cam, cam_pos=self.cam, switch_sq=PIN_SWITCH_SQ)

    # -- the several-view form of the case: its own, or the one view every single-view case is --
    def view_spec(self):
        if self.views is None:
            return dict(bucket=[self.bucket], bitmaps=[self.bitmap], bases=[BASE], first_slot=True)
        v = dict(self.views)
        v["bitmaps"] = [np.packbits(np.r_[np.asarray(b) >= 0, np.zeros(-self.n % 32, bool)], bitorder="little").view(np.uint32).copy() for b in v["bucket"]]
        return v

    def cmd_stride(self):
        return min(self.n_buckets, self.n)


# ---- the expectation by construction ----

def _row(case, b):
    mesh, lod = divmod(int(b), case.levels)
    t = case.table
    return int(t["index_len"][mesh, lod]), int(t["index_offset"][mesh, lod]), int(t["vertex_offset"][mesh]) & M32


def _runs(case, slot_buckets, first_slot=0):
    """One command per run of equal bucket: [indexCount, instanceCount, firstIndex, vertexOffset, firstInstance]."""
    rows = []
    for s, b in enumerate(slot_buckets):
        if s and b == slot_buckets[s - 1]:
            rows[-1][1] += 1
        else:
            ic, fi, vo = _row(case, b)
            rows.append([ic, 1, fi, vo, first_slot + s])
    return np.asarray(rows, np.uint32).reshape(-1, 5)


def sorted_d(case, sort):
    _, order, bits, _ = sort
    shift = 32 - bits
    return [(U_MAX_AXIS >> shift) - (int(u) >> shift) if order == FAR_FIRST else int(u) >> shift for u in case.U]


def ordered_d(case, order):
    return [K_MAX - int(k) if order == FAR_FIRST else int(k) for k in case.K]


def expect(case, call, base=BASE):
    """What `call` writes for `case`, from the labels alone. Single-view entries: dict(cmds rows, count, ids, members); shard:
    dict(chunk words for `capacity` = N ids, sentinel behind the members); views: expect_views."""
    if call.entry == "views":
        return expect_views(case)
    b = case.bucket
    members = [i for i in range(case.n) if b[i] >= 0]
    if call.entry == "ordered":
        d = ordered_d(case, call.order)
        order = [i for _, _, i in sorted((int(b[i]), d[i], i) for i in members)]
    elif call.entry == "sorted":
        d = sorted_d(case, call.sort)
        order = [i for _, i in sorted((d[i], i) for i in members)]
    else:
        order = [i for _, i in sorted((int(b[i]), i) for i in members)]
    ids = np.asarray([(i + base) & M32 for i in order], np.uint32)
    slot_buckets = [int(b[i]) for i in order]
    if call.entry == "shard":
        counts = [0] * (case.n_buckets + (4 - case.n_buckets % 4) % 4)
        for sb in slot_buckets:
            counts[sb] += 1
        tail = np.full(case.n, SENTINEL, np.uint32)
        tail[: len(ids)] = ids
        return dict(chunk=np.concatenate([np.asarray([len(ids), case.n_buckets, 0, 0] + counts, np.uint32), tail]))
    cmds = _runs(case, slot_buckets)
    return dict(cmds=cmds, count=len(cmds), ids=ids, members=len(ids), order=np.asarray(order, np.int64))


def expect_views(case, pad=3):
    """The four buffers of mip_batch_draws_views, whole, every unwritten word a sentinel."""
    v = case.view_spec()
    V, n, stride = len(v["bucket"]), case.n, case.cmd_stride()
    triples = sorted((view, int(bv[i]), i) for view, bv in enumerate(v["bucket"]) for i in range(n) if bv[i] >= 0)
    ids = np.full(V * n + pad, SENTINEL, np.uint32)
    ids[: len(triples)] = [(i + v["bases"][view]) & M32 for view, _, i in triples]
    cmds = np.full((V * stride + pad, 5), SENTINEL, np.uint32)
    counts = np.full(V + pad, SENTINEL, np.uint32)
    first_slot = np.full(V + 1 + pad, SENTINEL, np.uint32)
    slot = 0
    for view in range(V):
        mine = [bk for vw, bk, _ in triples if vw == view]
        rows = _runs(case, mine, first_slot=slot)
        cmds[view * stride: view * stride + len(rows)] = rows
        counts[view] = len(rows)
        if v["first_slot"]:
            first_slot[view] = slot
        slot += len(mine)
    if v["first_slot"]:
        first_slot[V] = slot
    return dict(cmds=cmds, counts=counts, ids=ids, first_slot=first_slot, members=slot)


# ---- the catalogue ----

def _spread(n, buckets, skip=()):
    """Instance i in bucket buckets[(5 i) % len]: a fixed, repeating walk over the buckets."""
    bs = [b for b in buckets if b not in skip]
    return np.asarray([bs[(5 * i) % len(bs)] for i in range(n)], np.int64)


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = []

    def add(*a, **kw):
        cases.append(Case(*a, **kw))

    live256 = [b for b in range(256) if b != 5]

    # ---- count / scatter inside a tile: N around the lanes, waves and tiles, the last instance a member or not ----
    for n in SIZES:
        for last in ("member", "nonmember"):
            b = _spread(n, live256)
            kind = np.ones(n, np.int64)
            for i in range(n):
                if i % 11 == 3:
                    b[i] = -1
                elif i % 13 == 6:
                    b[i], kind[i] = -1, 2
            b[n - 1] = 9 if last == "member" else -1
            idle = "no_idle_lanes" if n % TILE == 0 else f"idle_lanes_behind_{last}"
            add(f"n{n}_last_{last}", "tile", "S256d", b, kind, edges=[f"N={n}", idle] + (["n_tiles=1"] if n <= TILE else []))

    def rounds(n, fill=-1):
        return np.full(n, fill, np.int64)

    b = rounds(1024)
    b[0:64] = 7                                   # wave 0, round 0: one digit
    b[64:128] = np.arange(100, 164)               # wave 0, round 1: 64 digits
    add("one_digit_and_64_digits", "tile", "S256d", b, edges=["round_of_one_digit", "round_of_64_digits"])
    add("digits_bit_0", "tile", "S256d", np.where(np.arange(1500) % 3 == 0, 6, 7), edges=["digits_differ_in_bit_0_only"])
    add("digits_bit_7", "tile", "S256d", np.where(np.arange(1500) % 3 == 0, 3, 131), edges=["digits_differ_in_bit_7_only"])
    alt = np.where(np.arange(1100) % 2 == 0, 0, -1)
    add("bucket_0_beside_clear_bits", "tile", "S256d", alt, np.full(1100, 1), edges=["clear_bit_beside_bucket_0"])
    add("bucket_0_beside_dead_meshes", "tile", "S256d", alt, np.full(1100, 2), edges=["dead_mesh_beside_bucket_0"])
    b = rounds(1024, 10)
    b[256:320] = 9                                # wave 1: bucket 9 in round 0 ...
    b[448:512] = 9                                # ... and round 3, bucket 10 in between
    add("bin_in_rounds_0_and_3", "tile", "S256d", b, edges=["bin_in_rounds_0_and_3_only"])
    b = rounds(1024, 10)
    b[0:256:3] = 9                                # waves 0 and 3 hold bucket 9, waves 1 and 2 do not
    b[768:1024:2] = 9
    add("bin_in_waves_0_and_3", "tile", "S256d", b, edges=["bin_in_waves_0_and_3_only"])
    b = _spread(3072, live256)
    b[1024:2048] = 42
    add("bin_fills_a_tile", "tile", "S256d", b, edges=["bin_fills_a_tile", "no_idle_lanes"])
    kind = np.where(np.arange(3072) % 2 == 0, 1, 2)
    b = _spread(3072, live256)
    b[1024:2048] = -1
    add("empty_tile_between", "tile", "S256d", b, kind, edges=["empty_tile_between_tiles"])
    for lo, hi in ((63, 64), (127, 128), (191, 192), (0, 255)):
        add(f"bins_{lo}_and_{hi}", "tile", "S256d", np.where(np.arange(700) % 3 == 1, lo, hi), edges=[f"only_bins_{lo}_and_{hi}"])
    for m in (1, 2, 255, 256):
        b = _spread(300, range(max(m - 1, 1))) if m > 1 else rounds(300)
        b[0] = m - 1                              # the last bucket is used, and only by instance 0
        add(f"n_bins_{m}", "tile", f"S{m}", b, calls=(LODS_MODEL, LODS, SHARD, VIEWS), edges=[f"n_bins={m}_last_bucket_by_instance_0_only", "last_bucket_used"])

    # ---- the same placements through the pair policy (mip_batch_draws; the chain policy under the pin thresholds agrees) ----
    pair_calls = (DRAWS_MODEL, DRAWS, LODS)
    b = _spread(2049, [k for k in range(256) if k // 2 != 5])
    b[::7] = -1
    add("pair_2049", "tile", "P128d", b, np.where(np.arange(2049) % 14 == 0, 2, 1), calls=pair_calls, edges=["N=2049", "last_bucket_used"])

    # ---- rowscan: 255 .. 513 tiles; a sparse stream, every member placed ----
    for tiles in (255, 256, 257, 512, 513):
        n, last = (tiles - 1) * TILE + 1, tiles - 1                    # the last tile holds ONE instance
        b = rounds(n)
        at = lambda t, k: t * TILE + (37 * t + k) % TILE               # noqa: E731  (a place in a full tile)
        b[[at(t, 0) for t in range(last)]] = 7                         # bin 7: a member in every full tile
        b[at(0, 1)] = 1                                                # bin 1: tile 0 (and tile 256, below)
        b[at(10, 1)] = 6                                               # bin 6: tile 10 only
        edges = [f"n_tiles={tiles}"]
        if tiles == 257:                                               # tile 256 is the last tile: its one instance is bin 1's
            b[n - 1] = 1
            b[at(255, 2)] = 2                                          # bin 2: tile 255 only
            edges += ["bin_in_tile_0_and_256_only", "bin_in_tile_255_only", "bin_second_chunk_zero"]
        else:
            b[n - 1] = 3                                               # bin 3: the last tile only
            edges += ["bin_in_last_tile_only"]
        if tiles > 257:
            b[at(256, 1)] = 1
            b[at(255, 2)] = 2
            b[[at(300, 3), at(400, 3)]] = 4                            # bin 4: nothing in the first chunk of 256 tiles
            edges += ["bin_in_tile_0_and_256_only", "bin_in_tile_255_only", "bin_first_chunk_zero", "bin_second_chunk_zero"]
        add(f"rowscan_{tiles}_tiles", "rowscan", "S256d", b, calls=(LODS, SHARD), edges=edges)

    # ---- several passes: two and three digits ----
    live257 = [k for k in range(257) if k != 5]
    n = 2049
    add("two_digits_low_equal", "passes", "S257d", np.where(np.arange(n) % 2 == 0, 0, 256),
        edges=["passes=2", "low_digit_equal_high_digits_differ_passes=2", "last_bucket_used", "slot_of_for_the_model_kernel"])
    add("two_digits_high_equal", "passes", "S257d", _spread(n, range(1, 201), skip=(5,)), edges=["high_digits_equal_low_digit_differs_passes=2"])
    add("buckets_255_256", "passes", "S257d", np.where(np.arange(n) % 3 == 0, 256, 255), edges=["only_buckets_255_and_256", "buckets_255_and_256_used", "last_bucket_used"])
    three = (LODS_MODEL, LODS, SHARD, VIEWS)
    add("three_digits_low_equal", "passes", "S65537d", np.asarray([0, 256, 65536])[np.arange(n) % 3], calls=three,
        edges=["passes=3", "low_digit_equal_high_digits_differ_passes=3", "last_bucket_used"])
    add("three_digits_high_equal", "passes", "S65537d", _spread(n, range(256), skip=(5,)), calls=three, edges=["high_digits_equal_low_digit_differs_passes=3"])
    add("buckets_65535_65536", "passes", "S65537d", np.where(np.arange(n) % 3 == 0, 65536, 65535), calls=three,
        edges=["only_buckets_65535_and_65536", "buckets_65535_and_65536_used", "last_bucket_used"])
    # members = 0, 1, 1 023, 1 024, 1 025 and N of 2 049 instances: the SAME instances under different bitmaps (so one context
    # runs a call with few members directly behind one with many: test sequences below)
    for tname, buckets, calls in (("S257d", live257, STAGE_CALLS), ("S65537d", [k * 257 % 65537 for k in range(1, 600) if k * 257 % 65537 != 5] + [65536], three)):
        full = _spread(n, buckets)
        walk = [(i * 1031) % n for i in range(n)]                      # a fixed permutation: which instances a bitmap keeps
        for m in (0, 1, 1023, 1024, 1025, n):
            b = np.full(n, -1, np.int64)
            keep = walk[:m]
            b[keep] = full[keep]
            c = Case(f"members_{m}_{tname}", "passes", tname, b, calls=calls,
                     edges=([f"members={'N' if m == n else m}_of_2049"] + (["list_len_inside_a_round"] if m % 64 else []) + (["list_tiles_beyond_members_idle"] if m <= 1024 else [])))
            c.mesh_id = np.asarray(full, np.uint32)                      # every instance keeps its mesh; the bitmap alone decides
            cases.append(c)

    # ---- command writers: chain and shard (S tables), pair (P513: 1 026 buckets) ----
    writer = (LODS, SHARD, VIEWS)
    add("every_bucket_one_member", "writer", "S513", (np.arange(513) * 2) % 513, calls=writer, edges=["every_bucket_one_member", "last_bucket_used"])
    add("only_buckets_511_512", "writer", "S1025d", np.where(np.arange(900) % 4 == 0, 511, 512), calls=writer, edges=["only_buckets_511_and_512"])
    add("only_the_last_bucket", "writer", "S1025d", np.where(np.arange(900) % 4 == 0, -1, 1024), calls=writer, edges=["only_the_last_bucket", "last_bucket_used"])
    add("empty_chunk_between", "writer", "S1025d", np.asarray([3, 700, 1024, 700, 3])[np.arange(900) % 5], calls=writer, edges=["empty_bucket_chunk_between_chunks"])
    add("pair_only_255_256", "writer", "P513", np.where(np.arange(900) % 4 == 0, 255, 256), calls=pair_calls, edges=["only_buckets_255_and_256"])
    add("pair_only_511_512", "writer", "P513", np.where(np.arange(900) % 4 == 0, 511, 512), calls=pair_calls, edges=["only_buckets_511_and_512"])
    add("pair_only_the_last", "writer", "P513", np.where(np.arange(900) % 4 == 0, -1, 1025), calls=pair_calls, edges=["only_the_last_bucket"])
    add("pair_every_bucket", "writer", "P513", (np.arange(1026) * 5) % 1026, calls=pair_calls, edges=["every_bucket_one_member"])
    add("pair_empty_chunk_between", "writer", "P513", np.asarray([3, 700, 1025, 700, 2])[np.arange(900) % 5], calls=pair_calls, edges=["empty_bucket_chunk_between_chunks"])

    # ---- the several-view command writer and key policy ----
    def views_case(name, tname, per_view, edges, first_slot=True, family="views"):
        V, n = len(per_view), len(per_view[0])
        bases = [1000 * v + 7 for v in range(V)]
        bases[-1] = BASE
        first = np.asarray(per_view[0], np.int64)
        c = Case(name, family, tname, first, calls=(VIEWS,), edges=list(edges) + [f"n_views={V}"] * (V in (1, 2, 3, 15, 16)) + (["distinct_bases_one_wraps"] if V > 1 and n > 16 else []) +
                 ["view_first_slot_given" if first_slot else "view_first_slot_null"],
                 views=None)
        mesh = np.full(n, -1, np.int64)                                  # every view labels an instance with the same mesh or not at all
        for bv in per_view:
            bv = np.asarray(bv, np.int64)
            assert ((mesh < 0) | (bv < 0) | (mesh == bv)).all()
            mesh = np.where(bv >= 0, bv, mesh)
        live = [k for k in range(len(c.table)) if k != dead_mesh(tname)]
        c.mesh_id = np.where(mesh >= 0, mesh, np.asarray(live)[(np.arange(n) * 7) % len(live)]).astype(np.uint32)
        c.views = dict(bucket=[np.asarray(bv, np.int64) for bv in per_view], bases=bases, first_slot=first_slot)
        cases.append(c)

    n = 400
    s20 = [k for k in range(20) if k != 5]
    walk20 = _spread(n, s20)
    for V, fs in ((1, True), (2, False), (3, True), (15, True), (16, False)):
        # three views, every instance a member of each: the entries of instance 21 are split across a round (63 | 64, 65), of
        # instance 85 across a wave (255 | 256, 257), of instance 341 across a tile (1 023 | 1 024, 1 025)
        per = [walk20 if V == 3 else np.where((np.arange(n) + v) % (v + 2) == 0, -1, walk20) for v in range(V)]
        views_case(f"views_{V}", "S20d", per, ["passes=2"] if V * 20 > 256 else [], first_slot=fs)
    for B, V in ((128, 3), (256, 2), (512, 2)):
        wb = _spread(n, range(B))
        views_case(f"view_boundary_B{B}", f"S{B}", [np.where(np.arange(n) % (v + 3) == 0, -1, wb) for v in range(V)], [f"view_boundary_on_a_chunk_boundary_B={B}"])
    i = np.arange(n)
    views_case("view_two_chunks_later", "S600", [np.where(i % 2 == 0, 0, 599), np.where(i % 2 == 1, 599, -1)], ["view_first_members_two_chunks_later"])
    views_case("view_in_two_chunks", "S600", [np.where(i % 4 == 0, 0, np.where(i % 4 == 2, 1, 599)), np.where(i % 4 == 1, 599, np.where(i % 4 == 2, 1, -1))], [])
    none = np.full(n, -1, np.int64)
    views_case("empty_views_first_middle_last", "S20d", [none, walk20, none, np.where(i % 3 == 0, -1, walk20), none],
               ["empty_view_first", "empty_view_in_the_middle", "empty_view_last"])
    # 66 tiles of entries (16 views x 4 161 instances); ONE member in one tile of every residue of 64, each in a bucket of its own
    n, V = 4161, 16
    per = [np.full(n, -1, np.int64) for _ in range(V)]
    for r in range(64):
        t = 64 if r == 0 else 65 if r == 1 else r
        inst = 4160 if t == 65 else t * 64 + 3
        per[t % 16][inst] = s20[t % 19]
    views_case("every_histogram_copy", "S20d", per, ["every_histogram_copy_used", "only_copy_63_for_a_bucket", "passes=2"])
    # rowscan through entries: 16 views x 16 385 instances = 257 tiles of entries
    n = 16385
    per = [np.full(n, -1, np.int64) for _ in range(V)]
    per[0][[0, 16384]] = 1                                             # key 1: tiles 0 and 256 only
    per[1][255 * 64 + 5] = 2                                           # key 22: tile 255 only
    per[7][16384] = 1                                                  # key 141: the last tile only, its first chunk zero
    per[15][np.arange(9, 16384, 192)] = 19                             # key 319: every third tile of the first chunk
    views_case("views_rowscan_257_tiles", "S20d", per, ["n_tiles=257", "bin_in_tile_0_and_256_only", "bin_in_tile_255_only", "bin_in_last_tile_only",
                                                       "bin_first_chunk_zero", "bin_second_chunk_zero", "passes=2"], family="rowscan")

    # ---- depth keys through the shared passes ----
    # ordered: (bucket, (a, j) or "zero" / "inf" / "nan") per instance, repeated
    pattern = [(65535, "inf"), (65535, "zero"), (7, (1, 0)), (8, (1, 0)), (9, (1, 0)), (9, (1, 1)), (10, (1, 0)), (10, (2, 0)), (65535, "nan"), (7, "nan"),
               (300, (3, 9)), (8, "zero"), (300, "inf")]
    n = 650
    b, K, x = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.float32)
    for i in range(n):
        b[i], what = pattern[i % len(pattern)]
        x[i], K[i] = (0.0, 0) if what == "zero" else (np.inf, K_MAX) if what == "inf" else (np.nan, K_MAX) if what == "nan" else ordered_x(*what)
    b[3::26] = -1
    add("ordered_keys", "keys", "S65536d", b, K=K, x=x, calls=(ORDERED_NEAR, ORDERED_FAR, Call("ordered", True, FAR_FIRST)),
        edges=["passes=4", "largest_ordered_key", "two_buckets_same_D", "one_bucket_D_differs_in_digit_0_only", "one_bucket_D_differs_in_digit_1_only",
               "slot_of_for_the_model_kernel"] + [f"{k}_{t}_first" for k in ("K=0", "K=0x7F80", "K_of_NaN") for t in ("near", "far")])
    # sorted: two U values that differ in one byte of U; what that means for D depends on depth_bits
    s300 = [k for k in range(300) if k != 5]
    n = 600
    every = tuple(sorted_call(o, bits) for bits in (16, 24, 32) for o in (NEAR_FIRST, FAR_FIRST))
    for byte in range(4):
        u0 = 0xC0A08040
        U = np.where((np.arange(n) * 7) % 5 < 2, u0, u0 ^ (0x11 << (8 * byte)))
        edges = [f"sorted_D_differs_in_digit_{byte - (32 - bits) // 8}_only_bits={bits}" for bits in (16, 24, 32) if byte >= (32 - bits) // 8]
        edges += [f"sorted_ties_below_the_sorted_bits_bits={bits}" for bits in (16, 24) if byte < (32 - bits) // 8]
        bk = _spread(n, s300)
        bk[5::17] = -1
        add(f"sorted_byte_{byte}", "keys", "S300d", bk, U=U, x=[sorted_x(int(u)) for u in U], calls=every, edges=edges)
    special = [(0x80000000, _f32(0x00000000)), (0x80000000, _f32(0x80000000)), (0x80000001, _f32(0x00000001)), (0x7FFFFFFE, _f32(0x80000001)),
               (0xFF800000, np.float32(np.inf)), (0x007FFFFF, np.float32(-np.inf)), (0xFF800000, np.float32(np.nan)), (0xC0A08040, sorted_x(0xC0A08040)),
               (0x3F5F7FBF, sorted_x(0x3F5F7FBF))]
    U = [special[(i * 4) % len(special)][0] for i in range(n)]
    x = [special[(i * 4) % len(special)][1] for i in range(n)]
    add("sorted_special_values", "keys", "S300d", _spread(n, s300), U=U, x=x, calls=every, edges=[f"sorted_zeros_subnormals_infinities_nan_bits={b}" for b in (16, 24, 32)])

    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    return tuple(cases)


def case(name):
    return {c.name: c for c in all_cases()}[name]


# One context, one frame slot: a call with few members directly behind a call with many (the list buffers hold stale keys past
# `members`), for the two- and the three-digit table.
SEQUENCES = (("members_2049_S257d", "members_1_S257d", "members_1025_S257d", "members_0_S257d", "members_1023_S257d"),
             ("members_2049_S65537d", "members_1_S65537d", "members_1024_S65537d", "members_0_S65537d", "members_1025_S65537d"))
