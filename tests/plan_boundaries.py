"""Instance counts at which a frame's launch plan, or the structure of the cross-tile prefix, changes — READ from plan_frame
(renderer_amd/csrc/frame_plan.hpp) through tests/native/frame_plan_probe.cpp, not kept in a table: when a threshold moves,
the sizes the GPU tests run at (tests/test_gpu_boundaries.py) move with it and tests/test_plan_boundaries.py says what moved.
No GPU, no HIP: the probe is built with g++ into the temporary directory, once per source text."""
import hashlib
import json
import os
import subprocess
import tempfile
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_PROBE_SRC = os.path.join(ROOT, "tests", "native", "frame_plan_probe.cpp")
_PLAN_HPP = os.path.join(ROOT, "renderer_amd", "csrc", "frame_plan.hpp")

# what "the plan differs" means (LaunchPlan fields as the probe prints them; tri_either_blocks only as "> 0": its value is the grid)
PLAN_FIELDS = ("order", "general", "group_shift", "tri", "tri_threads", "tri_block_tickets", "tri_either", "recompact")

# request shapes of the GPU tests (the probe's request= words)
STREAMS = "model,bitmap,cmds,aabb,tlas"          # streams per-instance outputs: matrices, boxes, TLAS rows
COMMANDS_ONLY = "bitmap,cmds"                    # cull + commands: nothing per instance but a bit
TRIANGLES = "model,cmds,triangles"               # the per-triangle stage behind the frame kernel
SKINNED = "model,bitmap,cmds,aabb,skinned"
ROUND4_TRIANGLE_KERNELS = 0xFFFFFFFF             # tri_chunks_from = MIP_TUNE_TRI_CHUNKS_FROM=4294967295: parts / block / waves

Boundary = namedtuple("Boundary", "n fields")    # plan(n) differs from plan(n - 1) in `fields`

_exe = None


def probe_exe():
    global _exe
    if _exe is None:
        text = open(_PROBE_SRC, "rb").read() + open(_PLAN_HPP, "rb").read()
        exe = os.path.join(tempfile.gettempdir(), f"mip_frame_plan_probe_{os.getuid()}_{hashlib.sha1(text).hexdigest()[:16]}")
        if not os.path.exists(exe):
            tmp = f"{exe}.{os.getpid()}"
            subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", _PROBE_SRC, "-o", tmp])
            os.replace(tmp, exe)
        _exe = exe
    return _exe


def _probe(args):
    out = subprocess.run([probe_exe()] + [f"{k}={v}" for k, v in args.items()], capture_output=True, text=True, timeout=120, check=True)
    plans = [json.loads(line) for line in out.stdout.splitlines() if line]
    for p in plans:
        assert p["status"] == 0, p
        p["tri_either"] = p["tri_either_blocks"] > 0
    return plans


def plan(n, request=STREAMS, cu_count=256, **state):
    """The LaunchPlan of one frame, as a dict. state: the probe's keys (frame_slots, max_lod_tris, nonfinite, force_order,
    max_instances, tri_chunks_from, n_joints ...)."""
    return _probe(dict(state, n=int(n), request=request, cu_count=int(cu_count)))[0]


def plan_key(p):
    return tuple(p[f] for f in PLAN_FIELDS)


def differing_fields(a, b):
    return tuple(f for f in PLAN_FIELDS if a[f] != b[f])


def plan_changes(request=STREAMS, cu_count=256, lo=1, hi=1_200_000, **state):
    """Every n in (lo, hi] whose plan differs from that of n - 1. Searched tile by tile (the plan depends on n through n_tiles:
    256 T and 256 T + 1 are compared for every T), and, for a request with the per-triangle stage, instance by instance below
    70 000 (its thresholds are instance counts)."""
    found = {}
    tile = plan(1, request, cu_count, **state)["tile"]
    first = (lo // tile) * tile + 1                      # n = tile * T + 1: the first size of T + 1 tiles
    sweep = _probe(dict(state, request=request, cu_count=int(cu_count), sweep=f"{first}:{hi}:{tile}"))
    for before, after in zip(sweep, sweep[1:]):          # `before` has the plan of every size of its tile count, tile * T included
        d = differing_fields(before, after)
        if d and lo < after["n"] <= hi:
            found[after["n"]] = d
    if "triangles" in request.split(","):
        top = min(hi, 70_000)
        sweep = _probe(dict(state, request=request, cu_count=int(cu_count), sweep=f"{max(lo, 1)}:{top}:1"))
        for before, after in zip(sweep, sweep[1:]):
            d = differing_fields(before, after)
            if d:
                found[after["n"]] = tuple(sorted(set(found.get(after["n"], ()) + d), key=PLAN_FIELDS.index))
    return [Boundary(n, found[n]) for n in sorted(found)]


def group_shift_regimes(request=STREAMS, cu_count=256, hi=1_200_000, **state):
    """[(group_shift, first tile count, last tile count)] over the launches of 1 .. hi instances."""
    tile = plan(1, request, cu_count, **state)["tile"]
    sweep = _probe(dict(state, request=request, cu_count=int(cu_count), sweep=f"1:{hi}:{tile}"))
    regimes = []
    for p in sweep:
        if regimes and regimes[-1][0] == p["group_shift"]:
            regimes[-1][2] = p["n_tiles"]
        else:
            regimes.append([p["group_shift"], p["n_tiles"], p["n_tiles"]])
    return [tuple(r) for r in regimes]


def structure_tiles(request=STREAMS, cu_count=256, hi=1_200_000, **state):
    """Tile counts at which the prefix structure changes although no plan field does: {T: reason}. For each group size 2^s in
    force, the first and the last multiple T = k 2^s inside its regime (the last group is exactly full; T + 1: the last group
    holds one tile; T - 1: one tile short) — k = 1 where a one-group launch is in the regime —, and the window edge: the first
    launch whose last tile does not sum all earlier groups but starts from start1 (kLevel1Window + 1 groups of the largest size)."""
    tiles = {}
    regimes = group_shift_regimes(request, cu_count, hi, **state)
    for s, t_first, t_last in regimes:
        g = 1 << s
        k_first = max(1, -(-(t_first + 1) // g))         # k g - 1 >= t_first
        k_last = (t_last - 1) // g                       # k g + 1 <= t_last ...
        if (s, t_first, t_last) != regimes[-1]:
            k_last = t_last // g                         # ... but below the next regime T + 1 is the boundary itself
        for k in sorted({k_first, k_last}):
            if k >= 1 and k * g - 1 >= max(t_first, 1):
                tiles[k * g] = f"{k} full group{'s' if k > 1 else ''} of {g} tiles (group_shift {s})"
    window = plan(1, request, cu_count, **state)["level1_window"]
    s, t_first, t_last = regimes[-1]
    edge = (window + 1) << s
    if t_first <= edge - 1 and edge + 1 <= t_last:
        tiles[edge] = f"window edge: {window + 1} groups of {1 << s} tiles, the next tile starts from start1"
    return tiles


def sizes_of_tile_count(t, tile=256, boundary=False):
    """One instance in the last tile, a full last tile — and, where `t` itself is the boundary, the first size beyond it."""
    return [tile * t - (tile - 1), tile * t] + ([tile * t + 1] if boundary else [])


def boundary_sizes(request=STREAMS, cu_count=256, lo=1, hi=1_200_000, thin=False, **state):
    """{n: reason} — every instance count the GPU tests launch for this request shape: around every plan change, and around every
    structure tile count (T - 1, T, T + 1 tiles). thin: only {one instance in the last tile, full} at T and T + 1."""
    tile = plan(1, request, cu_count, **state)["tile"]
    sizes = {}

    def add(n, why):
        if lo <= n <= hi:
            sizes.setdefault(n, why)

    for b in plan_changes(request, cu_count, lo, hi, **state):
        why = f"{'/'.join(b.fields)} changes at {b.n}"
        if (b.n - 1) % tile == 0:                         # a tile-count threshold: T = (n - 1) / tile is the boundary
            t = (b.n - 1) // tile
            for n in sizes_of_tile_count(t, tile, boundary=True):
                add(n, why)
            add(tile * (t + 1), why)
        else:
            add(b.n - 1, why)
            add(b.n, why)
    for t, why in sorted(structure_tiles(request, cu_count, hi, **state).items()):
        if not thin:
            for n in sizes_of_tile_count(t - 1, tile):
                add(n, f"one tile short of: {why}")
        for n in sizes_of_tile_count(t, tile, boundary=True):
            add(n, why)
        add(tile * (t + 1), f"one tile beyond: {why}")
    return dict(sorted(sizes.items()))


def straddling_pairs(request=STREAMS, cu_count=256, lo=1, hi=1_200_000, **state):
    """[(n - 1, n, fields)] for every plan change."""
    return [(b.n - 1, b.n, b.fields) for b in plan_changes(request, cu_count, lo, hi, **state)]


def assert_straddles(n_below, n_above, request=STREAMS, cu_count=256, fields=None, **state):
    """The two sizes really get different plans (in `fields`, if given) — a boundary test that stopped straddling must fail."""
    a, b = plan(n_below, request, cu_count, **state), plan(n_above, request, cu_count, **state)
    d = differing_fields(a, b)
    assert d, f"{n_below} and {n_above} instances get the same plan at {cu_count} CUs ({request}, {state}): {plan_key(a)}"
    if fields:
        assert set(fields) <= set(d), f"{n_below} / {n_above}: expected {fields} to differ, only {d} do"
    return d
