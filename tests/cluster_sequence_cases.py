"""Sequences of cluster calls for ONE context (include/mi_instance_pipeline.h, the eleven entry points and phases of the cluster
family): the calls share a scratch per frame slot, a several-view scratch, two pairs of status words and the event behind a
FIRST call ("Cluster calls in sequence"), and every per-call test makes a context of its own. A sequence is a list of
steps — a state step switches the resident scene and rebuilds the cluster table and the cones, a call step names one of the
eleven UNITS and its parameters —; expectations() gives, per step, the return code and EVERY output buffer whole (the sentinel
where the call writes nothing), computed by the numpy restatements of the calls and never by a GPU.
tests/test_gpu_cluster_sequences.py applies the steps to one InstancePipeline; tests/test_cluster_sequence_cases.py checks the
sequences themselves on the CPU and shows that each expectation MUTANT — a stale input of the kind a shared scratch would
supply — changes the expected bytes of every unit it applies to. Seeded and deterministic; no GPU, no torch.

The buffer layouts are those of the per-call GPU tests' helpers (test_gpu_clusters._Out, test_gpu_cluster_triangles._Out,
test_gpu_cluster_views._ViewOut, test_gpu_cluster_views_list._Out, test_gpu_cluster_list._Out, test_gpu_cluster_list_phases._Buf,
test_gpu_cluster_phases._Record): GUARD_ROWS rows, PAD words, RECORD_GUARD words nobody may touch."""
import functools

import numpy as np

import cluster_cone_restatement as ccr
import cluster_list_phase_restatement as lp
import cluster_list_restatement as clr
import cluster_phase_restatement as pr
import cluster_restatement as cr
import cluster_triangle_restatement as ctr
import cluster_view_cases as cv
import cluster_views_list_restatement as cvlr
import cluster_views_restatement as cvr
import lifecycle_cases as lc
import lod_restatement as lr
import occlusion_restatement as orr
from renderer_amd import scene as scene_mod

SENTINEL = 0x5A5A5A5A
UNITS = ("cull", "cull_cone", "tri", "tri_cone", "views", "list", "list_views", "phase.FIRST", "phase.SECOND", "list_phase.FIRST",
         "list_phase.SECOND")
SEVERAL = ("views", "list_views")                     # the units that share the several-view scratch and its status words
SINGLE = tuple(u for u in UNITS if u not in SEVERAL)  # the units that share the slot's scratch and its status words
FIRSTS, SECONDS = ("phase.FIRST", "list_phase.FIRST"), ("phase.SECOND", "list_phase.SECOND")
TAKES_PYRAMID = ("cull", "cull_cone", "tri", "tri_cone", "list")      # optional there; the phase units need one, the view units take none
CONE_UNITS = ("cull_cone", "tri_cone", "list")
OK, INVALID, CAPACITY, DEVICE, NOT_READY = 0, -1, -4, -5, -6
ROOM = 5            # rows / words a buffer holds beyond everything the call could write
GUARD_ROWS, PAD, RECORD_GUARD, BLOCK = 3, 3, 6, 12
LARGE = 1 << 18     # a work_capacity above every bound a call of these scenes has by itself
MODE = lr.DISTANCE
MUTANTS = ("previous_scene", "previous_parameters", "stale_boxes", "stale_cones", "stale_record", "stale_bitmap", "other_slots_history")


def group(unit):
    return "several-view" if unit in SEVERAL else "single-view"


# ---- scenes ----

def _columns(n, variant, seed):
    base = scene_mod.make_scene(3, n=1)
    cols = lc.instances(n, len(lc.geometry_table(variant)), seed=seed)
    return dict(cols, meshes=lc.geometry_table(variant), planes=base["planes"], cam_pos=base["cam_pos"], n=n)


def _w_of(n):
    s = _columns(n, 1, 3)
    bits = _bitmaps(s)[0]
    return cr.work_items(s["pos"], s["scale"], s["mesh_id"], s["meshes"], s["cam_pos"], bits, MODE, _switch(1))["W"]


def _bitmaps(s):
    """Two bitmaps of a scene: every instance — the planes cull the clusters of those outside the frustum — but every 7th
    (every 5th), whose bit is cleared."""
    n = s["n"]
    if n == 0:
        return [np.zeros(0, np.uint32)] * 2
    out = []
    for k in (7, 5):
        bits = np.ones(n, bool)
        bits[k - 2::k] = False
        out.append(orr.bitmap_of(bits))
    return out


@functools.lru_cache(maxsize=None)
def _switch(variant):
    """The policy's thresholds: the pin policy of the hand-written cluster scenes with its first switch moved out to 60 units
    from the camera, so that most instances draw level 0 and the far ones level 1."""
    return (3600.0,) + tuple(float(v) for v in lr.PIN_SWITCH_SQ[1:])


@functools.lru_cache(maxsize=None)
def n_of_l():
    """The smallest n over geometry_table(1) whose W (first bitmap) exceeds 16 384: two head tiles and two list tiles."""
    lo, hi = 769, 1 << 14
    assert _w_of(lo) <= 16384 < _w_of(hi)
    while hi - lo > 1:           # W grows with n: instances(n) is a prefix of instances(n + 1) but for the wave-edge ids
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if _w_of(mid) <= 16384 else (lo, mid)
    return hi


SCENE_NAMES = ("S", "M", "L", "Z")
_SHAPE = dict(S=(0, 65), M=(1, 769), L=(1, None), Z=(1, 0))
PV = scene_mod.default_pv()


def _wall(first_column):
    depth = np.ones((32, 64), np.float32)
    if first_column is not None:
        depth[:, first_column: first_column + 32] = 0.0
    return depth


DEPTH = dict(old=_wall(0), new=_wall(16))     # the phase units' old and new images; "old" is the optional pyramid of the others


@functools.lru_cache(maxsize=None)
def occlusion(which):
    return dict(pv=PV, levels=orr.pyramid_levels(DEPTH[which]), width=64, height=32)


@functools.lru_cache(maxsize=None)
def scene(name):
    variant, n = _SHAPE[name]
    n = n_of_l() if n is None else n
    s = _columns(n, variant, 3)
    vertices, indices = lc.geometry(variant)
    boxes = cr.cluster_boxes(s["meshes"], vertices, indices)
    cones = ccr.cluster_cones(s["meshes"], vertices, indices, boxes)
    return dict(name=name, variant=variant, s=s, vertices=vertices, indices=indices, boxes=boxes, cones=cones, bitmaps=_bitmaps(s),
                switch=_switch(variant), eye=np.asarray(s["cam_pos"], np.float32), facing=1.0,
                max_clusters=int(cr.cluster_table(s["meshes"])["C"].max()))


def max_instances():
    return scene("L")["s"]["n"]


# ---- steps ----

def switch(name):
    return dict(op="scene", scene=name)


def call(unit, **kw):
    """A call step. async_; pyramid (TAKES_PYRAMID); work: "zero" / "exact" (W) / "short" (W - 1) / "large"; cap: "room" /
    "exact" / "short" (one entry too few); fib: first_instance_base; cone (list); n_views; bm: which of the scene's bitmaps;
    rec: the record's name (phase units); base (list_phase): "null", "count" (SECOND behind FIRST through FIRST's entry_count)
    or the value of the word; defer: an asynchronous call whose status a later wait step collects; refuse: "stale" (no step,
    the state does it), "misaligned" or "views17"."""
    step = dict(op="call", unit=unit, async_=False, pyramid=False, work="zero", cap="room", fib=0, cone=False, n_views=3, bm=0, rec=None,
                base="null", defer=False, refuse=None)
    assert set(kw) <= set(step), kw
    step.update(kw)
    assert (step["rec"] is not None) == (unit in FIRSTS + SECONDS), step
    return step


def wait(expect):
    return dict(op="wait", expect=expect)


# ---- what one call owes ----

def _key(v):
    return v if not isinstance(v, np.ndarray) else (v.shape, v.tobytes())


def _rows(img, rows, at=0):
    if len(rows):
        r = np.ascontiguousarray(rows).view(np.uint32).reshape(len(rows), -1)
        img[at: at + len(r)] = r
    return img


def _full(shape):
    return np.full(shape, SENTINEL, np.uint32)


SHORTCUT = True     # tests/test_cluster_sequence_cases.py switches it off to show that it changes nothing


def _same_as_full(p, w, work):
    """A call with room for everything and a bound W fits owes what the call with no bound of its own and unlimited room owes:
    every restatement reads work_capacity in one comparison with W and a capacity in one with its count. Saves the second
    evaluation, which for the triangle units over L costs a second."""
    return SHORTCUT and p["cap"] == "room" and (work == 0 or w <= work) and p["unit"] != "list_views"   # whose draw_args hold the stride


def _resolve(p, w, full_count):
    work = dict(zero=0, exact=w, short=max(w - 1, 1), large=LARGE)[p["work"]]
    cap = dict(room=full_count + ROOM, exact=full_count, short=max(full_count - 1, 0))[p["cap"]]
    return work, cap


_FULL = {}


def _once(memo, f):
    """The call with unlimited room and no bound of its own, once per everything else it depends on (`memo`, from _cached)."""
    if memo is None:
        return f()
    if memo not in _FULL:
        _FULL[memo] = f()
    return _FULL[memo]


def compute(sc, p, record=None, first=None, boxes=None, cones=None, bitmaps=None, memo=None):
    """One call of unit p["unit"] over scene sc (boxes / cones / bitmaps: in their place, for the mutants). record: the words
    a SECOND call reads; first: the FIRST step's answer (list_phase.SECOND with base "count"). Returns dict(status, images —
    every buffer of the step, whole, by name —, sizes — what the driver allocates —, record — a FIRST call's words —, w, bound)."""
    unit, s = p["unit"], sc["s"]
    boxes = sc["boxes"] if boxes is None else boxes
    cones = sc["cones"] if cones is None else cones
    bitmaps = sc["bitmaps"] if bitmaps is None else bitmaps
    bitmap, fib, sw = bitmaps[p["bm"]], p["fib"], sc["switch"]
    occ = occlusion("old") if (p["pyramid"] and unit in TAKES_PYRAMID) or unit in FIRSTS else occlusion("new") if unit in SECONDS else None
    n, big = s["n"], 1 << 30
    cone = dict(cones=cones, eye=sc["eye"], facing=sc["facing"]) if (unit in ("cull_cone", "tri_cone") or (unit == "list" and p["cone"])) else None

    if unit in SEVERAL:
        nv = p["n_views"]
        planes, cams = cv.frusta(s["planes"], nv), cv.view_cams(s, nv)
        bases = [(b + fib) & 0xFFFFFFFF for b in cv.view_bases(nv, n)]
        view_bm = [None if v % 3 == 2 else bitmaps[(p["bm"] + v) % 2] for v in range(nv)]
        f = cvr.cull_clusters_views if unit == "views" else cvlr.list_clusters_views
        run = lambda stride, work: f(s, boxes, planes, view_bm, bases, MODE, sw, stride, work, cams[0])   # noqa: E731
        full = _once(memo, lambda: run(1 << 24, 0))
        w = int(full["stats"][0])
        most = max([len(c) for c in full["all_cmds" if unit == "views" else "all_entries"]] + [0])
        work, stride = _resolve(p, w, most)
        want = full if _same_as_full(p, w, work) else run(stride, work)
        phys = most + ROOM
        fill = cvr.fill_outputs if unit == "views" else cvlr.fill_outputs
        part = fill(want, nv, stride, SENTINEL, 0)
        width = 5 if unit == "views" else 4
        main = "cmds" if unit == "views" else "entries"
        images = {main: _full((nv * phys + PAD, width))}
        images[main][: nv * stride] = part[main]
        for k in part:
            if k != main:
                images[k] = np.concatenate([part[k], _full(PAD)])
        return dict(status=want["status"], images=images, sizes=dict(n_views=nv, stride=phys, arg=stride, work=work), w=w, bound=work or n * sc["max_clusters"],
                    items=full["items"], survive=full["survive"],
                    views=dict(planes=planes, cams=cams, bases=bases, bitmaps=[None if b is None else (p["bm"] + v) % 2 for v, b in enumerate(view_bm)]))

    items = cr.work_items(s["pos"], s["scale"], s["mesh_id"], s["meshes"], s["cam_pos"], bitmap, MODE, sw)
    w = items["W"]
    out = dict(w=w)

    if unit in ("cull", "cull_cone", "phase.FIRST", "phase.SECOND"):
        if unit == "cull":
            run = lambda cap, work: cr.cull_clusters(s, boxes, bitmap, MODE, sw, cap, work, fib, occ)   # noqa: E731
        elif unit == "cull_cone":
            run = lambda cap, work: ccr.cull_clusters_cone(s, boxes, cone["cones"], cone["eye"], cone["facing"], bitmap, MODE, sw, cap, work, fib, occ)   # noqa: E731
        elif unit == "phase.FIRST":
            run = lambda cap, work: pr.first(s, boxes, bitmap, MODE, sw, cap, occ, p["room_bytes"], work, fib)   # noqa: E731
        else:
            run = lambda cap, work: pr.second(s, boxes, bitmap, MODE, sw, cap, occ, record, p["room_bytes"], work, fib)   # noqa: E731
        full = _once(memo, lambda: run(big, 0))
        heads = len(full["all_cmds"])
        work, cap = _resolve(p, w, heads)
        want = full if _same_as_full(p, w, work) else run(cap, work)
        scal = _full(8)
        scal[0], scal[2:6] = want["count"], want["stats"]
        out.update(status=want["status"], images=dict(cmds=_rows(_full((heads + ROOM + GUARD_ROWS, 5)), want["cmds"]), scal=scal),
                   sizes=dict(cap=heads + ROOM, arg=cap, work=work))
    elif unit in ("tri", "tri_cone"):
        if unit == "tri":
            run = lambda cap, work: ctr.cull_cluster_triangles(s, boxes, sc["vertices"], sc["indices"], bitmap, MODE, sw, PV, cap, 1 << 31, work, fib, occ)   # noqa: E731
        else:
            run = lambda cap, work: ccr.cull_cluster_triangles_cone(s, boxes, cone["cones"], cone["eye"], cone["facing"], sc["vertices"], sc["indices"], bitmap,   # noqa: E731
                                                                    MODE, sw, PV, cap, 1 << 31, work, fib, occ)
        full = _once(memo, lambda: run(big, 0))
        heads, room = len(full["all_cmds"]), len(full["full_stream"]) + ROOM
        work, cap = _resolve(p, w, heads)
        want = full if _same_as_full(p, w, work) else run(cap, work)
        scal = _full(12)
        scal[0], scal[2:8] = want["count"], want["stats"]
        stream = _full(room + 6)
        stream[: len(want["stream"])] = want["stream"]
        out.update(status=want["status"], images=dict(cmds=_rows(_full((heads + ROOM + GUARD_ROWS, 5)), want["cmds"]), scal=scal, stream=stream),
                   sizes=dict(cap=heads + ROOM, room=room, arg=cap, work=work))
    elif unit == "list":
        run = lambda cap, work: clr.list_clusters(s, boxes, bitmap, MODE, sw, cap, work, fib, occ, cone)   # noqa: E731
        full = _once(memo, lambda: run(big, 0))
        survivors = len(full["all_entries"])
        work, cap = _resolve(p, w, survivors)
        want = full if _same_as_full(p, w, work) else run(cap, work)
        scal = _full(12)
        scal[0], scal[2:6], scal[6:9] = want["count"], want["args"], want["stats"]
        out.update(status=want["status"], images=dict(entries=_rows(_full((survivors + ROOM + GUARD_ROWS, 4)), want["entries"]), scal=scal),
                   sizes=dict(cap=survivors + ROOM, arg=cap, work=work))
    else:   # list_phase.FIRST / list_phase.SECOND: one buffer of two scalar blocks; SECOND with base "count" writes into FIRST's
        appended = unit == "list_phase.SECOND" and p["base"] == "count"
        b = first["count"] if appended else 0 if p["base"] == "null" else int(p["base"])
        if unit == "list_phase.FIRST":
            run = lambda cap, work: lp.first(s, boxes, bitmap, MODE, sw, cap, occ, b, p["room_bytes"], work, fib)   # noqa: E731
        else:
            run = lambda cap, work: lp.second(s, boxes, bitmap, MODE, sw, cap, occ, record, b, p["room_bytes"], work, fib)   # noqa: E731
        full = _once(memo, lambda: run(big, 0))
        survivors = len(full["all_entries"])
        work = _resolve(p, w, 0)[0]
        cap = b + dict(room=survivors + ROOM, exact=survivors, short=max(survivors - 1, 0))[p["cap"]]
        if appended:
            cap = min(cap, first["sizes"]["cap"])
        want = full if _same_as_full(p, w, work) and not b else run(cap, work)
        call_no = 1 if unit == "list_phase.SECOND" else 0
        if appended:
            entries, scal, phys = first["images"]["entries"].copy(), first["images"]["scal"].copy(), first["sizes"]["cap"]
        else:
            # FIRST leaves room for everything a SECOND call can append: the candidates
            phys = b + survivors + (int(full["stats"][3]) if unit == "list_phase.FIRST" else 0) + ROOM
            entries, scal = _full((phys + GUARD_ROWS, 4)), _full(2 * BLOCK)
            if p["base"] != "null":
                scal[BLOCK * call_no + 10] = b
        _rows(entries, want["entries"], b)
        blk = scal[BLOCK * call_no: BLOCK * (call_no + 1)]
        blk[0], blk[2:6], blk[6:10] = want["count"], want["args"], want["stats"]
        out.update(status=want["status"], images=dict(entries=entries, scal=scal), sizes=dict(cap=phys, arg=cap, work=work, b=b, call=call_no), count=want["count"])
    out.update(items=items, survive=full["survive"])
    if unit in FIRSTS + SECONDS:
        room = pr.record_bytes(w) if p["room_bytes"] is None else p["room_bytes"]
        if unit in FIRSTS:      # the caller's record: room for exactly W work items; a SECOND step's is its FIRST step's (expectations)
            words = _full(room // 4 + RECORD_GUARD)
            words[: len(want["record"])] = want["record"]
            out["images"]["record"] = words
            out["record"] = want["record"]
        out["bound"] = min(work or n * sc["max_clusters"], 64 * ((room - 16) // 8))
    else:
        out["bound"] = work or n * sc["max_clusters"]
    return out


_CACHE = {}


def _cached(sc, p, record=None, first=None, **stale):
    """compute(), once per distinct (scene, unit, parameters, record, buffer in front) — and per stale input of a mutant."""
    ignore = ("async_", "defer", "op", "rec", "refuse")
    key = (sc["name"], tuple((k, p[k]) for k in sorted(p) if k not in ignore), None if record is None else record.tobytes(),
           None if first is None else (first["images"]["entries"].tobytes(), first["images"]["scal"].tobytes()),
           tuple((k, tuple(_key(x) for x in v) if isinstance(v, list) else _key(v)) for k, v in sorted(stale.items())))
    if key not in _CACHE:
        memo = (key[0], tuple(kv for kv in key[1] if kv[0] not in ("work", "cap"))) + key[2:]
        _CACHE[key] = compute(sc, p, record, first, memo=memo, **stale)
    return _CACHE[key]


def _untouched(answer):
    """A refused call: the buffers of the call it would have been, every word the sentinel."""
    return {k: _full(v.shape) for k, v in answer["images"].items()}


# ---- a sequence's expectations ----

def expectations(steps, mutant=None, frames_in_flight=2, mutate=("S", "M", "Z")):
    """Per step: None for a state step; dict(status) for a wait step; for a call step dict(status, images, sizes, unit, scene,
    step — the step with its record resolved —, applies — whether `mutant` had something else to put in). With a mutant the
    images are what a library with that stale read would leave, in the steps over the scenes of `mutate`."""
    out, scene_now, scene_before, stale = [], None, None, False
    records, last_of_unit, history = {}, {}, []        # record name -> dict(words, before, first); unit -> the unit's last step
    latest_record = None
    for k, st in enumerate(steps):
        if st["op"] == "scene":
            scene_before, scene_now, stale = scene_now, st["scene"], False
            records, latest_record = {}, None
            out.append(None)
            continue
        if st["op"] == "set_geometry":
            stale = True
            out.append(None)
            continue
        if st["op"] == "build":
            stale = False
            out.append(None)
            continue
        if st["op"] == "wait":
            out.append(dict(status=st["expect"]))
            continue
        unit, sc = st["unit"], scene(scene_now)
        p = dict(st, room_bytes=None, n_views=min(st["n_views"], 16))
        record = first = image = None
        if unit in SECONDS:
            r = records[st["rec"]]
            record, image, first = r["words"], r["image"], r["first"] if st["base"] == "count" else None
            assert st["base"] != "count" or (r["first"] is not None and not r["appended"]), (k, "nothing to append behind")
            p["room_bytes"] = 4 * (len(image) - RECORD_GUARD)
        true = _cached(sc, p, record, first)            # the bookkeeping (records, buffers in front) follows the right answer
        refused = bool(st["refuse"]) or stale
        answer, applies = true, False
        if refused:
            answer = dict(true, status=NOT_READY if stale else INVALID, images=_untouched(true), refused=True)
        elif scene_now not in mutate or (mutant in ("previous_scene", "stale_boxes", "stale_cones") and scene_before not in mutate):
            pass                                        # a mutant is evaluated over the small scenes alone: over L one costs seconds
        elif mutant == "previous_scene" and scene_before is not None and st["base"] != "count":
            answer, applies = _cached(dict(scene(scene_before), name=scene_now + "<-" + scene_before), p, record, first), True
        elif mutant in ("stale_boxes", "stale_cones") and scene_before is not None:
            which = "boxes" if mutant == "stale_boxes" else "cones"
            old = scene(scene_before)[which]
            applies = mutant == "stale_boxes" or unit in ("cull_cone", "tri_cone") or (unit == "list" and st["cone"])
            if applies:
                answer = _cached(sc, p, record, first, **{which: np.resize(old, sc[which].shape)})
        elif mutant == "stale_bitmap":
            answer, applies = _cached(sc, p, record, first, bitmaps=sc["bitmaps"][::-1]), True
        elif mutant == "previous_parameters" and unit in last_of_unit:
            was = last_of_unit[unit]
            fields = ("cap", "fib") + (("base",) if was["base"] != "count" and st["base"] != "count" else ())
            answer, applies = _cached(sc, dict(p, **{f: was[f] for f in fields}), record, first), True
        elif mutant == "stale_record" and unit in SECONDS and r["before"] is not None:
            answer, applies = _cached(sc, p, r["before"], first), True
        elif mutant == "other_slots_history":
            other = [h for h in history if h["unit"] == unit and not h.get("refused") and (frames_in_flight == 1 or h["slot"] != len(history) % 2)]
            if other:
                answer, applies = dict(true, status=other[-1]["true"]["status"], images=other[-1]["true"]["images"]), True
        if unit in SECONDS:                             # the caller's record holds what its FIRST call wrote, whatever the call read
            answer = dict(answer, images=dict(answer["images"], record=image))
        if not refused:
            if unit in FIRSTS:
                records[st["rec"]] = dict(words=true["record"], image=true["images"]["record"], before=latest_record,
                                          first=true if unit == "list_phase.FIRST" else None, appended=False)
                latest_record = true["record"]
            elif unit == "list_phase.SECOND" and st["base"] == "count":
                records[st["rec"]]["appended"] = True
            last_of_unit[unit] = st
        e = dict(answer, unit=unit, scene=scene_now, step=p, applies=applies, slot=len(history) % 2, true=true)
        history.append(e)
        out.append(e)
    return out


def differs(a, b):
    return a["status"] != b["status"] or any(a["images"][k].shape != b["images"][k].shape or a["images"][k].tobytes() != b["images"][k].tobytes() for k in a["images"])


# ---- the sequences ----

def _rng(name):
    return np.random.default_rng(int.from_bytes(name.encode(), "little") % (1 << 32))


def _varied(rng, unit, k, **fixed):
    """Parameters drawn for step k of a walk: every step of a unit differs from the unit's last one in fib and bm."""
    kw = dict(async_=bool(rng.integers(2)), pyramid=bool(rng.integers(2)), work=("zero", "exact", "large")[int(rng.integers(3))],
              cap=("room", "exact")[int(rng.integers(2))], fib=(0, 17, 0xFFFFFFF0, 123456)[k % 4], bm=(k // 2) % 2, cone=bool(rng.integers(2)),
              n_views=(1, 3, 16)[int(rng.integers(3))])
    kw.update(fixed)
    if unit == "list_phase.FIRST" and "base" not in kw:
        kw["base"] = ("null", 0, 3)[int(rng.integers(3))]
    return kw


def _euler(rng):
    """A closed walk over the complete digraph of the units with its loops: every ordered pair once (Hierholzer, seeded)."""
    left = {u: list(rng.permutation(len(UNITS))) for u in UNITS}
    stack, walk = [UNITS[int(rng.integers(len(UNITS)))]], []
    while stack:
        u = stack[-1]
        if left[u]:
            stack.append(UNITS[left[u].pop()])
        else:
            walk.append(stack.pop())
    return walk[::-1]


class _Records:
    """Names the records of a walk: a FIRST step opens one, a SECOND step reads the latest one a SECOND call may still append to
    (base "count", once per record) or any live one."""

    def __init__(self, rng):
        self.rng, self.live, self.k = rng, [], 0

    def reset(self):
        self.live = []

    def first(self, unit, bm, base):
        self.k += 1
        self.live.append(dict(name=f"r{self.k}", bm=bm, list=unit == "list_phase.FIRST", base=base, appended=False))
        return self.live[-1]["name"]

    def second(self, unit):
        """(rec, bm, base) for a SECOND step: the record's own bitmap — another one is the not-its-record case."""
        r = self.live[-1 - int(self.rng.integers(min(len(self.live), 3)))]
        base = "null"
        if unit == "list_phase.SECOND":
            if r["list"] and r["base"] in ("null", 0) and not r["appended"]:
                base, r["appended"] = "count", True
            else:
                base = int(self.rng.integers(4))
        return r["name"], r["bm"], base


def _walk(rng, units, scene_name, start=0, **fixed):
    recs, steps = _Records(rng), [switch(scene_name)]
    for k, unit in enumerate(units, start):
        kw = _varied(rng, unit, k, **fixed)
        if unit in FIRSTS:
            kw["rec"] = recs.first(unit, kw["bm"], kw.get("base", "null"))
        elif unit in SECONDS:
            kw["rec"], kw["bm"], kw["base"] = recs.second(unit)
        steps.append(call(unit, **kw))
    return steps


def every_pair():
    rng = _rng("every_pair")
    return _walk(rng, ["phase.FIRST", "list_phase.FIRST"] + _euler(rng), "M")


def across_phases():
    rng, steps, k = _rng("across_phases"), [], 0
    for which, name in enumerate(("S", "M")):
        steps.append(switch(name))
        for x in UNITS[which::2] + UNITS[1 - which::2]:
            for opener in FIRSTS:
                closer = opener.replace("FIRST", "SECOND")
                for order in ((0, 1), (1, 0)) if x in FIRSTS and x != opener else ((0, 1),):
                    k += 1
                    a, c = f"a{k}", f"x{k}"
                    base = dict(base="null") if opener == "list_phase.FIRST" else {}
                    steps.append(call(opener, **_varied(rng, opener, k, rec=a, bm=k % 2, **base)))
                    tail = [call(closer, **_varied(rng, closer, k, rec=a, bm=k % 2, base="count" if closer == "list_phase.SECOND" else "null"))]
                    if x in FIRSTS:
                        xbase = dict(base="null") if x == "list_phase.FIRST" else {}
                        steps.append(call(x, **_varied(rng, x, k + 1, rec=c, bm=(k + 1) % 2, **xbase)))
                        xc = x.replace("FIRST", "SECOND")
                        tail.append(call(xc, **_varied(rng, xc, k + 1, rec=c, bm=(k + 1) % 2, base="count" if xc == "list_phase.SECOND" else "null")))
                    elif x in SECONDS:     # a SECOND call between a FIRST and its SECOND: over the same record, at a base of its own
                        steps.append(call(x, **_varied(rng, x, k + 1, rec=a, bm=k % 2, base=2 if x == "list_phase.SECOND" else "null")))
                    else:
                        steps.append(call(x, **_varied(rng, x, k + 1)))
                    steps += [tail[i] for i in order[: len(tail)]]
    return steps


BOUNDS_ORDER = ("L", "S", "M", "Z", "S", "L")


def bounds_down_and_up():
    rng, steps, k = _rng("bounds_down_and_up"), [], 0
    for work in ("zero", "exact", "large"):
        for visit, name in enumerate(BOUNDS_ORDER):
            order = [UNITS[i] for i in rng.permutation(len(UNITS))]
            for f in FIRSTS:      # a SECOND unit behind the FIRST of its entry point
                s2 = f.replace("FIRST", "SECOND")
                i, j = order.index(f), order.index(s2)
                if j < i:
                    order[i], order[j] = s2, f
            k += 1
            # the parameters of a visit depend on the scene's name alone, so that both visits of L share their expectations
            fixed = dict(work=work, n_views=dict(S=16, M=3, L=3, Z=1)[name], fib=dict(S=17, M=0xFFFFFFF0, L=123456, Z=0)[name], bm=visit % 2 if name == "S" else 0,
                         cap="room" if name in "LZ" else ("room", "exact")[k % 2], **(dict(pyramid=False, cone=False, async_=True) if name == "L" else {}))
            recs, part = _Records(rng), [switch(name)]
            for unit in order:
                kw = _varied(rng, unit, k, **fixed)
                if unit in FIRSTS:
                    kw["rec"] = recs.first(unit, kw["bm"], kw.get("base", "null"))
                else:
                    if unit in SECONDS:
                        kw["rec"], kw["bm"], kw["base"] = recs.second(unit)
                part.append(call(unit, **kw))
            steps += part
    return steps


def _other(unit, same_group, k):
    pool = [u for u in (SEVERAL if (unit in SEVERAL) == same_group else SINGLE) if u != unit and u not in SECONDS]
    return pool[k % len(pool)]


def overflow_isolation():
    """Per X: [X asynchronous and overflowing, Y synchronous and fitting, wait -> MIP_ERR_CAPACITY, wait -> MIP_OK] with Y of
    X's status-word group and of the other one; the mirror [X asynchronous and fitting, Y synchronous and overflowing, wait]."""
    steps, k = [switch("S")], 0

    def with_record(unit, tag, **kw):
        if unit in FIRSTS:
            return [call(unit, rec=tag, **kw)]
        if unit in SECONDS:
            first = unit.replace("SECOND", "FIRST")
            return [call(first, rec=tag, bm=kw.get("bm", 0), fib=9), call(unit, rec=tag, **kw)]
        return [call(unit, **kw)]

    for x in UNITS:
        for same_group in (True, False):
            k += 1
            short = dict(cap="short") if k % 2 else dict(work="short")
            y = _other(x, same_group, k)
            steps += with_record(x, f"x{k}", async_=True, defer=True, fib=k, bm=k % 2, n_views=(1, 3, 16)[k % 3], **short)
            steps += with_record(y, f"y{k}", fib=k + 100, bm=(k + 1) % 2, pyramid=bool(k % 2), n_views=(3, 16, 1)[k % 3])
            steps += [wait(CAPACITY), wait(OK)]
            short = dict(work="short") if k % 2 else dict(cap="short")
            steps += with_record(x, f"mx{k}", async_=True, defer=True, fib=k + 200, bm=k % 2, cap="exact", n_views=(16, 1, 3)[k % 3])
            steps += with_record(y, f"my{k}", fib=k + 300, bm=(k + 1) % 2, **short)
            steps += [wait(OK)]
    return steps


def refused_in_between():
    """[a good call, a refused call of another kind, a good call of a third kind], per refusal and per unit it applies to."""
    steps, k = [switch("S")], 0

    def good(unit, tag):
        kw = dict(fib=k, bm=k % 2, async_=bool(k % 2))
        if unit in FIRSTS:
            return [call(unit, rec=tag, **kw)]
        return [call(unit, **kw)]

    plain = [u for u in UNITS if u not in SECONDS]
    for i, x in enumerate(UNITS):
        for refusal in ("stale", "misaligned") + (("views17",) if x in SEVERAL else ()) + (("not its record",) if x in SECONDS else ()):
            k += 1
            before, after = [u for u in plain if u != x][k % (len(plain) - 1)], [u for u in plain if u != x][(k + 4) % (len(plain) - 1)]
            steps += good(before, f"b{k}")
            rec = {}
            if x in FIRSTS:
                rec = dict(rec=f"x{k}")
            elif x in SECONDS:     # its FIRST ran, and fitted, over the state the refusal meets — or over the other bitmap
                steps.append(call(x.replace("SECOND", "FIRST"), rec=f"x{k}", bm=k % 2, fib=k))
                rec = dict(rec=f"x{k}")
            if refusal == "stale":
                steps += [dict(op="set_geometry"), call(x, fib=k, bm=k % 2, **rec), dict(op="build")]
            elif refusal == "not its record":
                steps.append(call(x, fib=k, bm=1 - k % 2, async_=bool(i % 2), **rec))
            else:
                steps.append(call(x, fib=k, bm=k % 2, refuse=refusal, n_views=17 if refusal == "views17" else 3, **rec))
            steps += good(after, f"a{k}")
    return steps


SEQUENCES = dict(every_pair=every_pair, across_phases=across_phases, bounds_down_and_up=bounds_down_and_up, overflow_isolation=overflow_isolation,
                 refused_in_between=refused_in_between)


@functools.lru_cache(maxsize=None)
def sequence(name):
    return tuple(SEQUENCES[name]())


def calls(steps):
    return [st for st in steps if st["op"] == "call"]
