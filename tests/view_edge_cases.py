"""Decision-edge scenes for the two calls that take several views at once (include/mi_instance_pipeline.h,
mip_cull_clusters_views and mip_batch_draws_views): no GPU, no torch, no new arithmetic. The scenes are the catalogues of
tests/decision_cases.py, tests/cluster_edge_cases.py and tests/lod_cases.py; what is new is WHERE a frame sits in the call.
tests/test_view_edge_cases.py proves what is claimed here, tests/test_gpu_view_edges.py runs the calls on the device.

A CALL is dict(set, name, s — the scene —, geometry — (table, vertices, indices, boxes) —, names — the frame of every view —,
planes, cams, bases, bits — a bool per instance and view, or None for a NULL bitmap —, ptr — which view's bitmap a view points
at, or None: two views with one key share ONE device pointer —, mode, switch, want — dict(cmds per view, counts, stats)).
An expectation is written from the instance-level decision (decision_cases.decide, lod_cases.want_edge_lods,
cluster_edge_cases.split_patterns) through cluster_edge_cases.transfer_commands / pattern_commands, never from
cluster_views_restatement, views_batch_restatement or a GPU; only the box-sourced tier set is owed cluster_restatement's
literal chain, per view.

THE RULES, each derivable by hand and asserted on the CPU:
  planes   view v's commands are the instances whose bit v is set and that view v's OWN planes do not cull
  level    mip_cull_clusters_views: ONE level per instance for all views, from the camera of slot 0. Of the four LOD rings of the
           `views` case only the ring around slot 0's camera is live; the other three are decided by slot 0's camera as well,
           and clearly (they are ten units from another point). mip_batch_draws_views: view v's level from view v's own camera:
           every ring is live in the view it was built around, and only there
  chain    one view carries the chain scene's camera (the origin), the others a camera 3e5 away: from there every squared
           distance exceeds every finite threshold, so an instance takes the LAST level its mesh and the policy allow — 5, or 2
           under SWITCH_SHORT, stopped at n_lods - 1 — unless its distance is NaN (a NaN position: level 0) or, under RELATIVE,
           its threshold is +inf or NaN (scale inf, scale NaN: level 0). The cluster call follows slot 0: the chain scene's
           levels in every view when the edge camera is in slot 0, the far levels in every view otherwise. The batch call has
           the chain scene's levels in the edge view and the far levels in every other view
  members  W and members come from the union of the views' bits; a NULL bitmap is all ones; a shared pointer gives view v the
           bits of view 0 under view v's planes
  base     firstInstance = (first_instance_base of view v + i) mod 2^32: slot 0 carries cluster_edge_cases.FRUSTUM_BASE, which
           wraps above 256 instances, one slot 0x80000000"""
import functools

import numpy as np

import cluster_cases as cc
import cluster_edge_cases as ce
import cluster_restatement as cr
import cluster_view_cases as cv
import decision_cases as dc
import lod_cases as lc

F = np.float32
DISTANCE, RELATIVE = lc.DISTANCE, lc.RELATIVE
KINDS = ("null", "given", "shared")
ALL_SIZES_ROTATION = {"union": 2, "union_nonfinite": 1}      # the rotation that runs at every size of decision_cases.SIZES
ROTATION_SIZES = (257, 513)                                  # every rotation runs at these
FAR = 3.0e5


# ---- a. slot rotations ----

def rotations(case, n_views):
    """The view lists of a case with frames f_0 .. f_{k-1}: rotation r puts f_{(v + r) mod k} into slot v, so over the k
    rotations every frame occupies every slot — slot 0, every middle slot and the last one, slots 8 .. 15 included when
    n_views = 16 repeats the list."""
    f = dc.case(case)["frames"]
    return [tuple(f[(v + r) % len(f)] for v in range(n_views)) for r in range(len(f))]


def bases(n_views):
    """first_instance_base per view: slot 0 wraps above 256 instances, the middle slot is 0x80000000, the rest small."""
    out = [1000 * v + 7 for v in range(n_views)]
    out[0] = ce.FRUSTUM_BASE
    if n_views > 1:
        out[n_views // 2] = 0x80000000
    return out


def kinds(n_views, r):
    """The kind of every view's bitmap under rotation r: "null", "given" (the view's own visible bits) or "shared" (view 0's
    pointer — a NULL one where view 0 is NULL — under this view's planes). The first, the middle and the last slot alternate
    between NULL and their own bits from one rotation to the next (the middle one out of step), so the edge instances of the
    frame there can have their bits set; the other slots rotate through all three kinds."""
    named = {0: 0, n_views // 2: 1, n_views - 1: 0}
    return [("null", "given")[(v + r + named[v]) % 2] if v in named else KINDS[(v + r) % 3] for v in range(n_views)]


def _pointers(kind):
    """ptr[v]: the view whose bits view v's pointer holds, or None."""
    first = None if kind[0] == "null" else 0
    return [first if v == 0 or k == "shared" else None if k == "null" else v for v, k in enumerate(kind)]


def _finish(c):
    n_views = len(c["planes"])
    assert len(c["cams"]) == len(c["bases"]) == len(c["bits"]) == len(c["ptr"]) == n_views and 1 <= n_views <= 16
    c["want"]["counts"] = np.array([len(x) for x in c["want"]["cmds"]], np.uint32)
    return c


def _stats(per, whole):
    """{W, members, heads_v, survivors_v ...} from transfer_commands / pattern_commands stats (heads, survivors, W, members)."""
    out = [int(whole["stats"][2]), int(whole["stats"][3])]
    for w in per:
        out += [int(w["stats"][0]), int(w["stats"][1])]
    return np.array(out, np.uint32)


# ---- b, c. transfer sets: the decision catalogue under rotated frames ----

@functools.lru_cache(maxsize=None)
def _decision(case, n, planes_frame, cam_frame, mutant=None):
    s = dc.layout(case, n)[0]
    fr = dc.catalogue()["frames"]
    return dc.decide(dict(s, planes=np.asarray(fr[planes_frame][0], F).reshape(24), cam_pos=np.asarray(fr[cam_frame][1], F).reshape(3)), mutant)


def transfer_want(table, mesh_id, lods, visible, bits, bases_, union=None):
    """The views call's answer where every cluster box of a level is the mesh box: view v's commands are
    cluster_edge_cases.transfer_commands of (lods[v], visible[v], bits[v], bases_[v]); W and members those of the union of the
    bits under lods[0]. For mip_cull_clusters_views every lods[v] is the same array."""
    n = len(mesh_id)
    b = [np.ones(n, bool) if x is None else np.asarray(x, bool) for x in bits]
    per = [ce.transfer_commands(table, mesh_id, lods[v], visible[v], b[v], bases_[v]) for v in range(len(b))]
    u = np.logical_or.reduce(b) if union is None else union
    whole = ce.transfer_commands(table, mesh_id, lods[0], np.zeros(n, bool), u)
    return dict(cmds=[w["cmds"] for w in per], stats=_stats(per, whole))


def frustum_want(c, planes=None, lod_cams=None, plane_mutant=None, lod_mutant=None, bits=None, union=None, bases_=None):
    """The expectation of a catalogue call, and the hooks the CPU test mutates it through: planes[v] / lod_cams[v] — the SLOT
    whose planes / camera view v uses (default v / 0) —, plane_mutant — {slot: a decision_cases.PLANE_MUTANTS name} —,
    lod_mutant, and other bits, union bits or bases."""
    case, n, names = c["case"], c["s"]["n"], c["names"]
    n_views = len(names)
    lods = [_decision(case, n, names[0], names[0 if lod_cams is None else lod_cams[v]], lod_mutant)["lod"] for v in range(n_views)]
    visible = [_decision(case, n, names[v if planes is None else planes[v]], names[0], (plane_mutant or {}).get(v))["visible"] for v in range(n_views)]
    return transfer_want(c["s"]["meshes"], c["s"]["mesh_id"], lods, visible, c["bits"] if bits is None else bits,
                         c["bases"] if bases_ is None else bases_, union)


@functools.lru_cache(maxsize=None)
def frustum_call(case, r, n_views, n, set_="frustum"):
    """The catalogue case at n instances over cluster_edge_cases.frustum_geometry(), under rotation r of its frames."""
    names = rotations(case, n_views)[r]
    s, src = dc.layout(case, n)
    fr = dc.catalogue()["frames"]
    kind = kinds(n_views, r)
    ptr = _pointers(kind)
    own = [_decision(case, n, f, names[0])["visible"] for f in names]
    c = dict(set=set_, name=f"{set_} {case} r={r} V={n_views} n={n}", case=case, r=r, s=dict(s, meshes=ce.frustum_geometry()[0]), src=src,
             geometry=ce.frustum_geometry(), names=names, planes=[np.asarray(fr[f][0], F).reshape(24) for f in names],
             cams=[np.asarray(fr[f][1], F).reshape(3) for f in names], bases=bases(n_views), kinds=kind, ptr=ptr,
             bits=[None if k is None else own[k] for k in ptr], own_bits=True, mode=DISTANCE, switch=ce.PIN)
    c["want"] = frustum_want(c)
    return _finish(c)


def frustum_keys():
    """(case, rotation, n_views, n): one rotation of each case at every size, every rotation at 257 and 513; n_views = k and 16."""
    out = []
    for case in dc.VIEW_INPUTS:
        k = len(dc.case(case)["frames"])
        for n_views in (k, 16):
            out += [(case, ALL_SIZES_ROTATION[case], n_views, n) for n in dc.SIZES if n not in ROTATION_SIZES]
            out += [(case, r, n_views, n) for r in range(k) for n in ROTATION_SIZES]
    return out


def lod_keys():
    """The `views` case — a LOD ring around each of the four view cameras — under every rotation; 4 and 16 views."""
    return [("views", r, n_views, 257) for n_views in (4, 16) for r in range(4)]


def edge_labels(c, v):
    """The instances of a catalogue call that carry a label built for the frame of slot v (its planes or its camera)."""
    idx = set(dc.labelled(dc.case(c["case"]), frame=c["names"][v], ref=c["names"][v]))
    return [i for i in range(c["s"]["n"]) if int(c["src"][i]) in idx]


# ---- c. the six-level chain: one edge view among far ones ----

CHAIN_SLOTS = (0, 7, 15)


def far_lods(s, mode, short):
    """The level every instance of the chain scene takes from a camera 3e5 away (the docstring's chain rule)."""
    cases = lc.edge_cases(mode)
    top = 2 if short else 5
    out = np.full(s["n"], top, np.int64)
    for i, k in enumerate(s["case"]):
        name = cases[k][0] if k >= 0 else ""
        if name.startswith("NaN position") or (mode == RELATIVE and name in ("scale inf", "scale NaN")):
            out[i] = 0
    return np.minimum(out, s["meshes"]["n_lods"][s["mesh_id"]].astype(np.int64) - 1)


def chain_cams(edge_slot, n_views=16):
    return [np.zeros(3, F) if v == edge_slot else np.array([0.0, 1000.0 * v, FAR], F) for v in range(n_views)]


@functools.lru_cache(maxsize=None)
def chain_call(mode, short, edge_slot, n_views=16):
    s = ce.chain_scene(mode)
    n = s["n"]
    every = np.ones(n, bool)
    lod = lc.want_edge_lods(s, mode, short) if edge_slot == 0 else far_lods(s, mode, short)     # all views follow slot 0
    half = np.arange(n) % 2 == 0
    bits = [None if v % 3 else half if v == 3 else every for v in range(n_views)]               # NULL, all ones, and one view of every second instance
    c = dict(set="chain", name=f"chain mode={mode} short={short} edge view {edge_slot}", s=s, geometry=ce.chain_geometry(), names=None,
             planes=[np.zeros(24, F)] * n_views, cams=chain_cams(edge_slot, n_views), bases=bases(n_views), ptr=[None if b is None else v for v, b in enumerate(bits)],
             bits=bits, own_bits=False, mode=mode, switch=lc.SWITCH_SHORT if short else lc.SWITCH, short=short, edge_slot=edge_slot)
    c["want"] = transfer_want(s["meshes"], s["mesh_id"], [lod] * n_views, [every] * n_views, bits, c["bases"])
    return _finish(c)


def chain_keys():
    return [(mode, short, slot) for mode in (DISTANCE, RELATIVE) for short in (False, True) for slot in CHAIN_SLOTS]


# ---- d. split decisions ----

BIG = 2.0 ** 20


def _cube(x_lo, x_hi, half):
    """Six planes in cluster_cases.PLANES' form: x in [x_lo, x_hi], |y| <= half, |z| <= half (cluster_view_cases' C and D, scaled)."""
    p = cc.PLANES.copy().reshape(6, 4)
    p[:, 3] = -half
    p[0, 3], p[1, 3] = -x_hi, x_lo
    return np.ascontiguousarray(p.reshape(-1))


EVERYTHING = _cube(-BIG, BIG, BIG)               # cv.C at the scene's scale: no instance is further than a few hundred units out
NOTHING = _cube(-2 * BIG - 8, -2 * BIG + 8, 8)   # cv.D
SPLIT_ORDERS = (("edge", "all", "none"), ("all", "edge", "none"), ("none", "all", "edge"))


@functools.lru_cache(maxsize=None)
def split_call(name, frame, order):
    s, labels = ce.split_scene(name, frame)
    table = ce.nested_geometry()[0]
    n = s["n"]
    patterns = {"edge": ce.split_patterns(s), "all": ["111"] * n, "none": ["000"] * n}
    planes = {"edge": s["planes"], "all": EVERYTHING, "none": NOTHING}
    b = bases(3)
    per = [ce.pattern_commands(table, patterns[o], b[v]) for v, o in enumerate(order)]
    c = dict(set="split", name=f"split {name}/{frame} {'-'.join(order)}", s=s, geometry=ce.nested_geometry(), names=None, planes=[planes[o] for o in order],
             cams=[s["cam_pos"]] * 3, bases=b, ptr=[None] * 3, bits=[None] * 3, own_bits=False, mode=DISTANCE, switch=ce.PIN, order=order,
             want=dict(cmds=[w["cmds"] for w in per], stats=_stats(per, per[0])))
    return _finish(c)


def split_keys():
    return [(name, frame, order) for name, frame in ce.SPLIT_INPUTS for order in SPLIT_ORDERS]


# ---- e. tier edges ----

@functools.lru_cache(maxsize=None)
def tier_instance_call(kind, placement, twin, r):
    """cluster_edge_cases.instance_tier_scenes under rotation r of the `union` frames: the tier of a work item is decided once,
    from the instance, and must hold under every view's planes."""
    s = ce.instance_tier_scenes(kind, placement)[0][twin]
    names = rotations("union", 7)[r]
    fr = dc.catalogue()["frames"]
    planes = [np.asarray(fr[f][0], F).reshape(24) for f in names]
    cams = [np.asarray(fr[f][1], F).reshape(3) for f in names]
    lod = dc.decide(dict(s, cam_pos=cams[0]))["lod"]
    visible = [dc.decide(dict(s, planes=p))["visible"] for p in planes]
    c = dict(set="tier", name=f"instance tier {kind} {placement} twin={twin} r={r}", s=s, geometry=ce.frustum_geometry(), names=names, planes=planes, cams=cams,
             bases=bases(7), ptr=[None] * 7, bits=[None] * 7, own_bits=False, mode=DISTANCE, switch=ce.PIN)
    c["want"] = transfer_want(s["meshes"], s["mesh_id"], [lod] * 7, visible, c["bits"], c["bases"])
    return _finish(c)


def tier_instance_keys():
    out = []
    for kind in dc.TIER_KINDS:
        for placement in dc.TIER_PLACEMENTS:
            for twin in (0, 1):
                out.append((kind, placement, twin, len(out) // 2 % 7))
    return out


TIER_LISTS = {"closed-open": ("closed", "open"), "open-closed": ("open", "closed"), "sixteen": ("closed", "open") * 8}


@functools.lru_cache(maxsize=None)
def tier_box_call(kind, placement, views, twin):
    """cluster_edge_cases.tier_scene — the tier hangs on the CLUSTER's box — with both TIER_FRAMES as views of one call. Owed
    cluster_restatement.cull_clusters per view: the literal chain."""
    frames = TIER_LISTS[views]
    table, vertices, indices, want_boxes = ce.tier_geometry(kind, twin)
    t = ce.tier_scene(kind, placement, frames[0])
    s = dict(t["scene"], meshes=table)
    boxes = cr.cluster_boxes(table, vertices, indices)
    b = bases(len(frames))
    full = ce.bits_to_bitmap(np.ones(s["n"], bool))
    per = [cr.cull_clusters(dict(s, planes=ce.TIER_FRAMES[f]), boxes, full, DISTANCE, ce.PIN, cmd_capacity=1 << 30, first_instance_base=b[v])
           for v, f in enumerate(frames)]
    assert all(r["status"] == 0 for r in per)
    c = dict(set="tier", name=f"box tier {kind} {placement} {views} twin={twin}", s=s, geometry=(table, vertices, indices, want_boxes), names=frames,
             planes=[ce.TIER_FRAMES[f] for f in frames], cams=[s["cam_pos"]] * len(frames), bases=b, ptr=[None] * len(frames), bits=[None] * len(frames),
             own_bits=False, mode=DISTANCE, switch=ce.PIN, odd_instances=t["odd_instances"],
             want=dict(cmds=[r["cmds"] for r in per], stats=_stats(per, per[0])))
    return _finish(c)


def tier_box_keys(kind=None):
    return [(k, placement, views, twin) for k in (ce.TIER_KINDS if kind is None else (kind,)) for twin in (False, True) for placement in ce.TIER_PLACEMENTS
            for views in TIER_LISTS]


def without_odd(cmds, base, odd):
    """The commands of the instances that own no odd item."""
    return cmds[~np.isin((cmds["firstInstance"].astype(np.int64) - int(base)) & 0xFFFFFFFF, odd)]


# ---- f. mask edges: sixteen views with sixteen distinct bits, written by hand ----

MASK_LAYOUTS = ("every bit", "an instance in no view")


@functools.lru_cache(maxsize=None)
def mask_call(layout):
    """33 one-cluster instances of the ladder "1" (192 indices at 0) under sixteen views of frustum A, which sees the cluster.
    Instance i < 32 is a member of view i mod 16 only, instance 32 of all sixteen: view v draws v, v + 16 and 32 — three
    commands, three heads, three survivors; W = members = 33. The other layout takes instance 5 out of view 5, its only view:
    view 5 draws 21 and 32, W = members = 32."""
    s, _ = cc.ladder_scene(["1"], [0] * 33)
    b = bases(16)
    gone = 5 if layout == "an instance in no view" else None
    bits, cmds, stats = [], [], [33 - (gone is not None)] * 2
    for v in range(16):
        who = [i for i in (v, v + 16, 32) if i != gone]
        bits.append(np.isin(np.arange(33), who))
        cmds.append(cv._rows([(192, 1, 0, 0, (b[v] + i) & 0xFFFFFFFF) for i in who]))
        stats += [len(who), len(who)]
    c = dict(set="mask", name=f"mask {layout}", s=s, geometry=(s["meshes"], s["vertices"], s["indices"], None), names=None, planes=[cv.A] * 16,
             cams=[cc.CAM.copy()] * 16, bases=b, ptr=list(range(16)), bits=bits, own_bits=False, mode=DISTANCE, switch=cc.PIN,
             want=dict(cmds=cmds, stats=np.array(stats, np.uint32)))
    return _finish(c)


# ---- every call of a set ----

SETS = ("frustum", "lod", "chain", "split", "tier", "mask")


def calls(which):
    if which == "frustum":
        return [frustum_call(*k) for k in frustum_keys()]
    if which == "lod":
        return [frustum_call(*k, set_="lod") for k in lod_keys()]
    if which == "chain":
        return [chain_call(*k) for k in chain_keys()]
    if which == "split":
        return [split_call(*k) for k in split_keys()]
    if which == "tier":
        return [tier_instance_call(*k) for k in tier_instance_keys()] + [tier_box_call(*k) for k in tier_box_keys()]
    if which == "mask":
        return [mask_call(k) for k in MASK_LAYOUTS]
    raise KeyError(which)


# ---- mip_batch_draws_views: bucket membership from the same decisions ----

def padded_table(table, n_views):
    """The table with one-level meshes behind it that no instance references, until n_views x B > 256: the call takes several
    passes; mesh ids and decisions are unchanged, only lod_base and the command offsets move."""
    extra = max(0, 256 // n_views + 1 - int(table["n_lods"].sum()))
    pad = np.zeros(extra, table.dtype)
    pad["aabb_min"], pad["aabb_max"], pad["n_lods"] = -0.5, 0.5, 1
    pad["index_len"][:, 0] = 3 * (1 + np.arange(extra))
    pad["index_offset"][:, 0] = 5000 + 10 * np.arange(extra)
    pad["vertex_offset"] = 1 + np.arange(extra)
    return np.concatenate([np.asarray(table), pad])


def batch_want(table, mesh_id, lods, bits, bases_):
    """What mip_batch_draws_views owes, from the decisions: instance i is a member of view v iff bit v is set and the level
    lods[v][i] of its mesh has indices; per view and bucket (mesh-major, level-minor) one command whose firstInstance is the
    absolute slot; instance_ids = base_v + i (mod 2^32), view-major, bucket-major, draw order inside a bucket."""
    mesh_id = np.asarray(mesh_id, np.int64)
    n, n_lods = len(mesh_id), table["n_lods"].astype(np.int64)
    ids, cmds, first_slot = [], [], []
    for v in range(len(bits)):
        first_slot.append(len(ids))
        lod = np.asarray(lods[v], np.int64)
        member = (np.ones(n, bool) if bits[v] is None else np.asarray(bits[v], bool)) & (table["index_len"][mesh_id, lod] > 0)
        rows = []
        for k in range(len(table)):
            for l in range(int(n_lods[k])):
                who = np.nonzero(member & (mesh_id == k) & (lod == l))[0]
                if len(who):
                    rows.append((int(table["index_len"][k, l]), len(who), int(table["index_offset"][k, l]), int(table["vertex_offset"][k]), len(ids)))
                    ids += [(int(bases_[v]) + int(i)) & 0xFFFFFFFF for i in who]
        cmds.append(ce._rows(rows))
    first_slot.append(len(ids))
    return dict(cmds=cmds, counts=np.array([len(c) for c in cmds], np.uint32), first_slot=np.array(first_slot, np.uint32), ids=np.array(ids, np.uint32),
                members=len(ids), n_buckets=int(n_lods.sum()))


def batch_frustum_want(c, lod_cams=None, lod_mutant=None, bases_=None, table=None):
    """The batch expectation of a catalogue call: view v's level from the camera of slot lod_cams[v] (default: its own)."""
    case, n, names = c["case"], c["s"]["n"], c["names"]
    lods = [_decision(case, n, names[0], names[v if lod_cams is None else lod_cams[v]], lod_mutant)["lod"] for v in range(len(names))]
    return batch_want(c["s"]["meshes"] if table is None else table, c["s"]["mesh_id"], lods, c["bits"], c["bases"] if bases_ is None else bases_)


@functools.lru_cache(maxsize=None)
def batch_table(kind, n_views, padded):
    """The mesh table of a batch call — decision_cases.MESHES or the chain's — as ONE array per (kind, n_views, padded)."""
    table = dc.MESHES if kind == "decision" else ce.chain_geometry()[0]
    return padded_table(table, n_views) if padded else np.asarray(table)


def _batch(c, kind, padded, want):
    t = batch_table(kind, len(c["planes"]), padded)
    assert (len(c["planes"]) * int(t["n_lods"].sum()) > 256) == padded
    b = dict(c, set="batch " + c["set"], name=f"batch {c['name']} padded={padded}", s=dict(c["s"], meshes=t), padded=padded, geometry=None)
    b["want"] = want(b)
    return b


@functools.lru_cache(maxsize=None)
def batch_frustum_call(case, r, n_views, n, padded, set_="frustum"):
    """The catalogue call through mip_batch_draws_views over decision_cases.MESHES: membership by the same bitmaps, levels per view."""
    return _batch(frustum_call(case, r, n_views, n, set_), "decision", padded, batch_frustum_want)


def chain_batch_lods(c):
    s = c["s"]
    return [lc.want_edge_lods(s, c["mode"], c["short"]) if v == c["edge_slot"] else far_lods(s, c["mode"], c["short"]) for v in range(len(c["planes"]))]


@functools.lru_cache(maxsize=None)
def batch_chain_call(mode, short, edge_slot, padded):
    return _batch(chain_call(mode, short, edge_slot), "chain", padded,
                  lambda b: batch_want(b["s"]["meshes"], b["s"]["mesh_id"], chain_batch_lods(b), b["bits"], b["bases"]))


def batch_calls(which):
    """The batch calls of a set, one pass and several: "frustum" (every call of frustum_keys()), "lod", "chain"."""
    out = []
    for padded in (False, True):
        if which == "frustum":
            out += [batch_frustum_call(*k, padded) for k in frustum_keys()]
        elif which == "lod":
            out += [batch_frustum_call(*k, padded, set_="lod") for k in lod_keys()]
        elif which == "chain":
            out += [batch_chain_call(*k, padded) for k in chain_keys()]
        else:
            raise KeyError(which)
    return out


BATCH_SETS = ("frustum", "lod", "chain")
