"""Sequences of mutating calls for ONE context (tests/context_model.py holds the contract): named sequences, one per transition
that api_context.hip handles with cached host state, and seeded random walks over the same small input sets. A sequence is a
list of steps (operation, arguments[, probe]); tests/test_gpu_lifecycle.py applies every step to an InstancePipeline and to the
model and compares what the next consumers write with the oracle / the restatements of model.scene();
tests/test_lifecycle_cases.py checks the sequences themselves on the CPU, and shows which sequence tells which likely mistake
(context_model.MUTANTS and the two below) from the contract. Seeded and deterministic; no GPU, no torch.

Sizes: n from N_SET (a tile is 256 instances, a wave 64), m from M_SET (one entry: scalar id; up to 256: u8; above: u16 — the
width of the narrow id column follows max_meshes, the id MODE of a launch follows m), one context of MAX_INSTANCES x MAX_MESHES;
WIDE_MAX_MESHES is the context whose ids stay in the u32 column."""
import functools
import hashlib

import numpy as np

import context_model as cm
import decision_cases as dc
import numpy_restatement as nr
from renderer_amd import scene as scene_mod
from renderer_amd.pipeline import MESH_DTYPE

F = np.float32
MAX_INSTANCES, MAX_MESHES, WIDE_MAX_MESHES = 769, 300, 65537
N_SET = (0, 1, 255, 256, 257, 513, 769)
M_SET = (1, 2, 7, 200, 300)
UPDATE_RANGES = ((251, 11), (255, 3), (0, 1), (63, 2), (509, 4))   # odd first and count across a tile (and a wave) boundary
PROBES = ("run", "wire_packed", "run_many", "run_views", "tlas", "light_draw_lists", "batch_draws_lods", "run_occluded", "cull_clusters",
          "cull_clusters_cone")
# two mistakes no ContextModel flag can make: they are mistakes of the expectation itself
EXTRA_MUTANTS = ("count_kept_when_it_goes_down", "frame_in_flight_sees_the_new_state")
ALL_MUTANTS = cm.MUTANTS + EXTRA_MUTANTS


# ---- inputs ----

def table(m, variant=0):
    """m entries repeating SEVEN different meshes (entry k differs from entry k mod 256), rotated by `variant`: the same size with
    other contents."""
    return np.resize(np.roll(scene_mod.mixed_mesh_table(7), -variant), m)


def instances(n, m, seed=0):
    """The four columns of n instances over a table of m meshes: the first and last instance of every wave carry id 0 or m - 1,
    the others ids spread over the table (tests/test_gpu_narrow_ids.py, pinned_scene); every second seed inside the frustum."""
    s = scene_mod.make_scene(3, n=max(n, 1), first=1000 * seed, all_visible=seed % 2 == 0)
    ids = ((np.arange(n, dtype=np.uint64) * 2654435761 + seed * 40503) % m).astype(np.uint32)
    edges = sorted({e for b in range(0, n, 64) for e in (b, b + 63) if e < n} | ({0, n - 1} if n else set()))
    for k, e in enumerate(edges):
        ids[e] = 0 if k % 2 == 0 else m - 1
    if n >= 2:
        ids[n - 1] = m - 1
    return dict(pos=s["pos"][:n].copy(), rot=s["rot"][:n].copy(), scale=s["scale"][:n].copy(), mesh_id=ids)


def rows(cols, first, count):
    return {k: v[first:first + count].copy() for k, v in cols.items()}


def blas(m, salt=0):
    return (np.arange(m, dtype=np.uint64) << np.uint64(20)) + np.uint64(0xABC0000000 + 0x1000 * salt)


def geometry_table(variant=0):
    """Four (variant 1: five) small meshes with geometry of their own, a few dozen clusters of 64 triangles: every level's range
    and vertices are disjoint, so make_geometry lays them out as the table says."""
    lens = (((1200, 600, 300), (390,), (960, 480), (210, 60)), ((990, 330), (1500, 750, 375, 186), (192,), (600, 300), (96,)))[variant]
    t = np.zeros(len(lens), MESH_DTYPE)
    boxes = np.roll(scene_mod.mixed_mesh_table(7), variant)[:len(lens)]
    t["aabb_min"], t["aabb_max"] = boxes["aabb_min"], boxes["aabb_max"]
    off = voff = 0
    for k, chain in enumerate(lens):
        t["n_lods"][k] = len(chain)
        for l, length in enumerate(chain):
            t["index_len"][k, l], t["index_offset"][k, l] = length, off
            off += length
        t["vertex_offset"][k] = voff
        voff += max(chain[0] // 3, 9)
    return t


@functools.lru_cache(maxsize=None)
def geometry(variant=0):
    v, i = scene_mod.make_geometry(geometry_table(variant), "patches")
    v.setflags(write=False); i.setflags(write=False)
    return v, i


# ---- the census flipped by the table alone ----

def big_boxes():
    """decision_cases' table with every box ten times larger and a sixth entry: another size, box_abs 30 instead of 3."""
    t = np.concatenate([dc.MESHES, dc.MESHES[:1]])
    t["aabb_min"] *= F(10.0); t["aabb_max"] *= F(10.0)
    return t


@functools.lru_cache(maxsize=None)
def flip_scale():
    """A scale for an instance at the origin with the identity rotation whose separable_bound is below kSeparableLimit under
    decision_cases' table and above it under big_boxes(): the geometric mean of the two scales at which the bound meets the limit
    (found by bisection on the mirror, not assumed)."""
    edges = []
    for t in (dc.MESHES, big_boxes()):
        box_abs = dc.table_box_abs(t)
        below = lambda s: bool(dc.separable_bound(np.zeros(3, F), dc.IDENTITY, s, box_abs)[0] < dc.SEPARABLE_LIMIT)
        edges.append(float(dc._bits_bisect(F(1e30), F(3e38), below)[0]))
    small_table_edge, big_table_edge = edges
    assert big_table_edge < small_table_edge
    return F(np.sqrt(small_table_edge * big_table_edge))


def flip_instances(n=257, at=256):
    """Ordinary instances (decision_cases' fillers, in front of the default camera) and, alone in the last tile, the odd one."""
    pos, rot, scale, mesh = dc._fillers(np.random.default_rng(0xF11B), n)
    pos[:, 2] += F(6.0)
    pos[at], rot[at], scale[at], mesh[at] = 0.0, dc.IDENTITY, flip_scale(), 0
    return dict(pos=pos, rot=rot, scale=scale, mesh_id=mesh), at


# ---- named sequences ----

def _upload(cols, device=False):
    return ("set_instances_device" if device else "set_instances", dict(cols))


def _update(first, count, **cols):
    return ("update_instances", dict(first=first, count=count, **cols))


def _census_by_table():
    cols, at = flip_instances()
    plain = dict(cols, scale=cols["scale"].copy())
    plain["scale"][at] = 1.0                  # the same scene without the odd instance: the tables no longer move the census
    return [("set_mesh_table", dict(meshes=dc.MESHES)), _upload(cols), ("set_mesh_table", dict(meshes=big_boxes())),
            ("set_mesh_table", dict(meshes=dc.MESHES)), ("set_mesh_table", dict(meshes=big_boxes())),
            _upload(plain), ("set_mesh_table", dict(meshes=dc.MESHES))]


def _census_by_update():
    cols = instances(513, 7, seed=2)
    good = rows(cols, 255, 3)
    bad = rows(cols, 255, 3)
    bad["pos"][0, 1], bad["scale"][2] = np.nan, np.inf          # instances 255 and 257: two tiles
    return [("set_mesh_table", dict(meshes=table(7))), _upload(cols), _update(255, 3, pos=bad["pos"], scale=bad["scale"]),
            _update(255, 1, pos=good["pos"][:1]), _update(257, 1, scale=good["scale"][2:]), _update(256, 0),
            _update(251, 11, **rows(instances(513, 7, seed=4), 300, 11))]


def _same_size_swap():
    return [("set_mesh_table", dict(meshes=table(7))), _upload(instances(513, 7, seed=2)), ("set_mesh_table", dict(meshes=table(7, 3))),
            ("set_mesh_table", dict(meshes=table(200))), _upload(instances(769, 200, seed=4)), ("set_mesh_table", dict(meshes=table(200, 5))),
            ("set_mesh_table", dict(meshes=table(200, 5)))]


def _shrink_inside():
    cols = instances(769, 2, seed=2)
    zeros = np.zeros(769, np.uint32)
    return [("set_mesh_table", dict(meshes=table(300))), _upload(cols), ("set_mesh_table", dict(meshes=table(200))),
            ("set_mesh_table", dict(meshes=table(7))), _update(0, 1, mesh_id=np.full(1, 7, np.uint32)), ("set_mesh_table", dict(meshes=table(2))),
            _update(0, 769, mesh_id=zeros), ("set_mesh_table", dict(meshes=table(1))), ("set_mesh_table", dict(meshes=table(300, 1))), _update(251, 11, mesh_id=np.arange(289, 300, dtype=np.uint32))]


def _blas_across_tables():
    cols = instances(257, 7, seed=2)
    high = ((np.arange(257, dtype=np.uint32) * 7) % 57 + 7).astype(np.uint32)             # every id >= 7
    return [("set_mesh_table", dict(meshes=table(7))), ("set_blas_addresses", dict(addresses=blas(7))), _upload(cols),
            ("set_mesh_table", dict(meshes=table(64))), _update(0, 257, mesh_id=high), ("set_blas_addresses", dict(addresses=blas(7))),
            ("set_blas_addresses", dict(addresses=blas(64, 1))), ("set_mesh_table", dict(meshes=table(64))),
            ("set_blas_addresses", dict(addresses=blas(64, 2)))]


def _count_down_and_up():
    steps = [("set_mesh_table", dict(meshes=table(7)))]
    for k, n in enumerate((769, 513, 257, 256, 255, 1, 0, 1, 769, 0, 513)):
        steps.append(_upload(instances(n, 7, seed=2 * k), device=k % 3 == 2))
    return steps


def _refused_host_upload():
    cols = instances(513, 7, seed=2)
    bad = instances(257, 7, seed=4)
    bad["mesh_id"][256] = 7
    return [("set_mesh_table", dict(meshes=table(7))), _upload(cols), _upload(bad), _update(255, 3, **rows(bad, 10, 3)),
            _upload(bad, device=True), _update(0, 1, **rows(cols, 0, 1)), _upload(instances(769, 7, seed=6), device=True),
            _upload(instances(770, 7, seed=6))]


def _stranding_shrink():
    return [("set_mesh_table", dict(meshes=table(200))), _upload(instances(513, 200, seed=2)), ("set_mesh_table", dict(meshes=table(7))),
            _update(0, 1, **rows(instances(1, 7), 0, 1)), _upload(instances(513, 7, seed=4)), ("set_mesh_table", dict(meshes=table(301)))]


def _clusters():
    cols = instances(257, 4, seed=2)
    return [("set_mesh_table", dict(meshes=geometry_table(0))), _upload(cols), ("build_clusters", {}),
            ("set_geometry", dict(vertices=geometry(0)[0], indices=geometry(0)[1])), ("build_cluster_cones", {}), ("build_clusters", {}),
            ("build_cluster_cones", {}), ("set_geometry", dict(vertices=geometry(0)[0], indices=geometry(0)[1])), ("build_clusters", {}),
            ("build_cluster_cones", {}), ("set_mesh_table", dict(meshes=geometry_table(1))), ("build_clusters", {}),
            ("set_geometry", dict(vertices=geometry(1)[0], indices=geometry(1)[1])), ("build_clusters", {}), ("build_cluster_cones", {}),
            ("build_clusters", {})]


def _in_flight():
    """Every mutating call behind a frame that was launched asynchronously and not waited for (frames_in_flight = 2)."""
    cols = instances(513, 4, seed=2)
    return [("set_mesh_table", dict(meshes=geometry_table(0))), _upload(cols), ("set_geometry", dict(vertices=geometry(0)[0], indices=geometry(0)[1])),
            ("build_clusters", {}), ("build_cluster_cones", {}), _update(251, 11, **rows(instances(513, 4, seed=4), 100, 11)),
            _upload(instances(769, 4, seed=6)), ("set_mesh_table", dict(meshes=table(64))), ("set_blas_addresses", dict(addresses=blas(64))),
            _upload(instances(769, 64, seed=8), device=True), _update(0, 769, mesh_id=instances(769, 64, seed=10)["mesh_id"])]


SEQUENCES = {"census_by_table": _census_by_table, "census_by_update": _census_by_update, "same_size_swap": _same_size_swap,
             "shrink_inside": _shrink_inside, "blas_across_tables": _blas_across_tables, "count_down_and_up": _count_down_and_up,
             "refused_host_upload": _refused_host_upload, "stranding_shrink": _stranding_shrink, "clusters": _clusters, "in_flight": _in_flight}
IN_FLIGHT = ("in_flight",)                    # the sequences the driver runs with a frame in flight in front of every step


@functools.lru_cache(maxsize=None)
def sequence(name):
    return tuple(SEQUENCES[name]())


# ---- what a sequence expects, as digests (the CPU's view of "the expected bytes or the expected return code") ----

def digest(model):
    """Everything the probes compare, of the model's present state: the statuses, the census state and the frame's bytes
    (numpy restatement) with the TLAS rows' address words."""
    head = (model.frame_ready, model.fallback, model.cull_status(), model.cull_status(cone=True))
    if not model.frame_ready or model.n == 0:
        return head + (model.n,)
    s = model.scene()
    if int(s["mesh_id"].max()) >= len(s["meshes"]):
        return head + (model.n, "an id outside the table: the kernels gather whatever lies behind it")
    h = hashlib.sha256()
    want = nr.run(s)
    for a in (want["model"], want["world_aabb"], want["coarse_culled"], *(want["cmds"][k] for k in ("indexCount", "firstIndex", "vertexOffset", "firstInstance")),
              model.blas_addresses()[s["mesh_id"]]):
        h.update(np.ascontiguousarray(a).tobytes())
    return head + (model.n, h.hexdigest())


class _StaleTail(cm.ContextModel):
    """count_kept_when_it_goes_down: an upload of fewer instances leaves n, and the old instances behind the new ones, as they were."""

    def _upload(self, pos, rot, scale, mesh_id, device):
        old = None if not self.have_instances else (self.n, self.pos, self.rot, self.scale, self.mesh_id)
        rc = super()._upload(pos, rot, scale, mesh_id, device)
        if rc == cm.OK and old and self.n < old[0]:
            k = self.n
            self.pos, self.rot, self.scale, self.mesh_id = (np.concatenate([new, was[k:]]) for new, was in zip((self.pos, self.rot, self.scale, self.mesh_id), old[1:]))
            self.n = old[0]
            self.nonfinite = self._count()
        return rc


def new_model(mutant=None, max_meshes=MAX_MESHES):
    if mutant == "count_kept_when_it_goes_down":
        return _StaleTail(MAX_INSTANCES, max_meshes)
    return cm.ContextModel(MAX_INSTANCES, max_meshes, mutant=mutant if mutant in cm.MUTANTS else None)


def expectations(name, mutant=None):
    """Per step of a named sequence: (return code, [what the frame in flight must deliver,] the state's digest)."""
    model = new_model(mutant)
    out = []
    for op, kw in sequence(name):
        before = digest(model) if name in IN_FLIGHT and model.frame_ready else None
        rc = model.apply(op, **kw)
        after = digest(model)
        if before is not None:
            out.append((rc, after if mutant == "frame_in_flight_sees_the_new_state" and model.frame_ready else before, after))
        else:
            out.append((rc, after))
    return out


# ---- seeded random walks ----

WALK_SEEDS = (16, 24, 51, 74, 158, 245, 258, 275)   # chosen by search: see tests/test_lifecycle_cases.py for what they must satisfy
_WALK_TABLES = tuple(("table", m, v) for m in M_SET for v in (0, 3)) + (("geometry", 4, 0), ("geometry", 5, 1))
_OP_WEIGHTS = dict(set_mesh_table=2.0, set_instances=2.0, set_instances_device=1.5, update_instances=2.5, set_blas_addresses=1.5, set_geometry=1.0,
                   build_clusters=1.5, build_cluster_cones=1.5)
REFUSE = 0.08                                 # how often a step asks for something the contract refuses, on purpose


def _walk_table(kind, m, v):
    return geometry_table(v) if kind == "geometry" else table(m, v)


def random_walk(seed, steps=40):
    """`steps` steps (operation, arguments, probe): operations and arguments drawn from the small sets above THROUGH the model, so
    that most steps are valid in the state they meet; a step the contract refuses — drawn on purpose (REFUSE) or met by chance —
    stays in the walk. The probe is the one consumer the driver runs directly behind the step."""
    rng = np.random.default_rng(0x11FEC0DE + seed)
    model = new_model()
    ops, weights = list(_OP_WEIGHTS), np.array(list(_OP_WEIGHTS.values()))
    out = []
    for k in range(steps):
        op = "set_mesh_table" if k == 0 else "set_instances" if k == 1 else ops[rng.choice(len(ops), p=weights / weights.sum())]
        refuse = k > 1 and rng.random() < REFUSE
        salt = int(rng.integers(1, 50))
        # a call the state would refuse by itself is mostly replaced by the call that mends the state
        if not refuse and rng.random() < 0.9:
            if op in ("update_instances", "set_instances", "set_instances_device") and not model.have_meshes:
                op = "set_mesh_table"
            elif op == "update_instances" and not model.have_instances:
                op = "set_instances"
            elif op == "build_cluster_cones" and not model.clusters_valid:
                op = "build_clusters"
            if op == "build_clusters" and not model.have_geometry:
                op = "set_geometry"
        if op == "set_mesh_table":
            fits = [t for t in _WALK_TABLES if not model.have_instances or model.n == 0 or t[1] > int(model.mesh_id.max())]
            pick = _WALK_TABLES if refuse or rng.random() < 0.1 else fits          # (a stranding shrink: MIP_OK, nothing resident)
            # towards a table the resident geometry fits, while there is one: the cluster calls need it
            geo = [t for t in pick if t[0] == "geometry"]
            pick = geo if geo and model.have_geometry and rng.random() < 0.5 else pick
            kind, m, v = pick[rng.integers(len(pick))]
            kw = dict(meshes=table(MAX_MESHES + 1) if refuse and rng.random() < 0.3 else _walk_table(kind, m, v))
        elif op in ("set_instances", "set_instances_device"):
            n = int(rng.choice(N_SET))
            cols = instances(n, max(model.m, 1), seed=salt)
            if refuse and n:
                cols["mesh_id"][int(rng.integers(n))] = model.m
            elif refuse:
                cols = instances(MAX_INSTANCES + 1, max(model.m, 1), seed=salt)
            kw = cols
        elif op == "update_instances":
            usable = [r for r in UPDATE_RANGES if r[0] + r[1] <= model.n] or [(0, 0)]
            first, count = usable[rng.integers(len(usable))]
            if rng.random() < 0.1:
                count = 0
            if refuse:
                first = model.n
                count = max(count, 1)
            src = rows(instances(MAX_INSTANCES, max(model.m, 1), seed=salt), 300, count)
            names = [c for c in ("pos", "rot", "scale", "mesh_id") if rng.random() < 0.5] or ["mesh_id"]
            if rng.random() < 0.15 and count and "pos" in names:
                src["pos"][0, 0] = np.nan                                          # the census moves
            kw = dict(first=first, count=count, **{c: src[c] for c in names})
        elif op == "set_blas_addresses":
            kw = dict(addresses=blas(model.m + 1 if refuse else model.m, salt))
        elif op == "set_geometry":
            v = int(rng.integers(2))
            # mostly the geometry the resident table was made for, while it is one of the two
            for t in (0, 1):
                if len(model.meshes) == len(geometry_table(t)) and np.array_equal(model.meshes, geometry_table(t)) and rng.random() < 0.8:
                    v = t
            kw = dict(vertices=geometry(v)[0], indices=geometry(v)[1])
        else:
            kw = {}
        model.apply(op, **kw)
        out.append((op, kw, PROBES[rng.integers(len(PROBES))]))
    return out


def walk_statistics(walk):
    """(the (operation, probe) pairs of a walk, the steps the model expects to be refused)."""
    model = new_model()
    refused = sum(model.apply(op, **kw) != cm.OK for op, kw, _ in walk)
    return {(op, probe) for op, _, probe in walk}, refused
