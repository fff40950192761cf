"""A pure model of what a MipContext holds between calls, as include/mi_instance_pipeline.h promises it: the mesh table, the four
instance columns and n, have_meshes / have_instances, the BLAS addresses, the geometry, whether the cluster table and the cones
are valid, and the census state the next frame must see. No GPU, no library: numpy and the float32 census mirror of
tests/decision_cases.py (census_fails under the table's own box_abs, table_box_abs).

One method per mutating call. Each returns the status the header names for the call (OK or a MIP_ERR_* code) and applies the
header's state change — also for the two outcomes that change state without uploading what was asked: a device upload with an
id outside the table (MIP_ERR_INVALID_ARGUMENT, nothing resident afterwards) and a smaller table that strands a resident id
(MIP_OK, nothing resident afterwards). A refused HOST upload changes nothing: its ids are checked before any copy.

scene() is what the oracle and the numpy restatements take: a consumer's expected bytes are always those of model.scene().

MUTANTS names the likely mistakes of the library's host side. ContextModel(mutant=...) makes that one mistake and nothing
else; tests/test_lifecycle_cases.py shows that every one of them changes what some named sequence expects. Only this model is
ever mutated: no wrong library is built or run."""
import numpy as np

import decision_cases as dc
from renderer_amd import scene as scene_mod
from renderer_amd.pipeline import MESH_DTYPE, wire_index_bits

OK, INVALID, CAPACITY, NOT_READY = 0, -1, -4, -6
MAX_LODS = MESH_DTYPE["index_len"].shape[0]
MUTANTS = ("census_not_recounted", "census_not_decremented", "table_contents_kept", "m_kept_on_shrink", "blas_kept",
           "instances_kept_when_stranded", "instances_dropped_by_refused_host_upload", "clusters_kept_across_set_geometry")
OPERATIONS = ("set_mesh_table", "set_instances", "set_instances_device", "update_instances", "set_blas_addresses", "set_geometry",
              "build_clusters", "build_cluster_cones")
_COLUMNS = (("pos", np.float32, 3), ("rot", np.float32, 4), ("scale", np.float32, 1), ("mesh_id", np.uint32, 1))


def _column(a, dtype, width):
    a = np.array(a, dtype=dtype, copy=True)
    return a.reshape(-1, width) if width > 1 else a.reshape(-1)


class ContextModel:
    def __init__(self, max_instances, max_meshes, mutant=None, planes=None, cam_pos=None):
        assert mutant is None or mutant in MUTANTS, mutant
        self.max_instances, self.max_meshes, self.mutant = int(max_instances), int(max_meshes), mutant
        self.planes = scene_mod.default_planes() if planes is None else np.asarray(planes, np.float32).reshape(24)
        self.cam_pos = np.asarray(scene_mod.DEFAULT_CAMERA["cam_pos"] if cam_pos is None else cam_pos, np.float32).reshape(3)
        self.meshes = np.zeros(0, MESH_DTYPE)
        self.m = 0                               # the table size the id checks, the address check and the wire form go by
        self.have_meshes = self.have_instances = False
        self.n = 0
        self.pos, self.rot, self.scale, self.mesh_id = (_column([], d, w) for _, d, w in _COLUMNS)
        self.blas = None                         # None: reference 0 for every mesh
        self.vertices = self.indices = None
        self.have_geometry = self.clusters_valid = self.cones_valid = False
        self.box_abs = np.float32(0.0)
        self.nonfinite = 0                       # the census count, kept the way the header's calls keep it

    # ---- what the next consumer must see ----

    def scene(self):
        return dict(n=self.n, pos=self.pos, rot=self.rot, scale=self.scale, mesh_id=self.mesh_id, meshes=self.meshes, planes=self.planes,
                    cam_pos=self.cam_pos)

    @property
    def frame_ready(self):
        """False: a frame (and every call over the resident instances) is MIP_ERR_NOT_READY."""
        return self.have_meshes and self.have_instances

    @property
    def fallback(self):
        """True: the next launch over the resident instances is the kernel with the fall-back tiers."""
        return self.have_instances and self.nonfinite != 0

    @property
    def index_bits(self):
        return wire_index_bits(self.m)

    def blas_addresses(self):
        """Per mesh of the resident table, as the TLAS rows carry them: zeros while none are set for THIS table."""
        out = np.zeros(len(self.meshes), np.uint64)
        if self.blas is not None:                # (other lengths only under a mutant: what lies behind the old addresses is anything)
            out[:] = np.uint64(0xFFFFFFFFFFFFFFFF)
            k = min(len(out), len(self.blas))
            out[:k] = self.blas[:k]
        return out

    def fresh_census(self):
        """The census counted from nothing: what `nonfinite` must equal while instances are resident."""
        return int(dc.census_fails(self.pos, self.rot, self.scale, self.box_abs).sum()) if self.have_instances else 0

    def cull_status(self, cone=False):
        """What mip_cull_clusters (cone: mip_cull_clusters_cone) returns before it looks at anything else."""
        if not self.frame_ready or not self.clusters_valid or (cone and not self.cones_valid):
            return NOT_READY
        return OK

    # ---- the calls ----

    def apply(self, op, **kw):
        assert op in OPERATIONS, op
        return getattr(self, op)(**kw)

    def _drop_instances(self):
        self.have_instances, self.n = False, 0
        self.pos, self.rot, self.scale, self.mesh_id = (_column([], d, w) for _, d, w in _COLUMNS)

    def _count(self, first=0, count=None):
        stop = self.n if count is None else first + count
        return int(dc.census_fails(self.pos[first:stop], self.rot[first:stop], self.scale[first:stop], self.box_abs).sum())

    def set_mesh_table(self, meshes):
        meshes = np.array(meshes, dtype=MESH_DTYPE, copy=True).reshape(-1)
        m = len(meshes)
        if m > self.max_meshes:
            return CAPACITY
        if m and (((meshes["n_lods"] < 1) | (meshes["n_lods"] > MAX_LODS)).any() or not np.isfinite(meshes["aabb_min"]).all()
                  or not np.isfinite(meshes["aabb_max"]).all()):
            return INVALID
        if self.have_instances and self.have_meshes and m < self.m and self.n and int(self.mesh_id.max()) >= m \
                and self.mutant != "instances_kept_when_stranded":
            self._drop_instances()               # a new scene: table first, instances next
            self.nonfinite = 0
        same_size = self.have_meshes and m == self.m
        if not (self.mutant == "table_contents_kept" and same_size):
            self.meshes = meshes
        if not (self.mutant == "m_kept_on_shrink" and self.have_meshes and m < self.m):
            self.m = m
        self.have_meshes = True
        self.clusters_valid = self.cones_valid = False
        if self.mutant != "blas_kept":
            self.blas = None
        box_abs = dc.table_box_abs(meshes)
        if box_abs != self.box_abs:
            self.box_abs = box_abs
            if self.have_instances and self.mutant != "census_not_recounted":
                self.nonfinite = self._count()
        return OK

    def _upload(self, pos, rot, scale, mesh_id, device):
        if not self.have_meshes:
            return NOT_READY
        cols = [_column(a, d, w) for a, (_, d, w) in zip((pos, rot, scale, mesh_id), _COLUMNS)]
        n = len(cols[3])
        assert all(len(c) == n for c in cols)
        bad_ids = n and int(cols[3].max()) >= self.m
        if bad_ids and not device:               # checked on the host before any copy: the old scene stays as it is
            if self.mutant == "instances_dropped_by_refused_host_upload":
                self._drop_instances()
            return INVALID
        if n > self.max_instances:
            return CAPACITY
        if bad_ids:                              # found on the device, after the copies: nothing is resident
            self._drop_instances()
            return INVALID
        self.pos, self.rot, self.scale, self.mesh_id = cols
        self.n, self.have_instances = n, True
        self.nonfinite = self._count()
        return OK

    def set_instances(self, pos, rot, scale, mesh_id):
        return self._upload(pos, rot, scale, mesh_id, device=False)

    def set_instances_device(self, pos, rot, scale, mesh_id):
        return self._upload(pos, rot, scale, mesh_id, device=True)

    def update_instances(self, first, count, pos=None, rot=None, scale=None, mesh_id=None):
        if not self.have_instances:
            return NOT_READY
        first, count = int(first), int(count)
        if first + count > self.n:
            return INVALID
        given = {}
        for (name, d, w), a in zip(_COLUMNS, (pos, rot, scale, mesh_id)):
            if a is not None:
                given[name] = _column(a, d, w)
                assert len(given[name]) == count, name
        if "mesh_id" in given and count and int(given["mesh_id"].max()) >= self.m:
            return INVALID
        if count:
            before = self._count(first, count)
            for name, a in given.items():
                getattr(self, name)[first:first + count] = a
            after = self._count(first, count)
            if self.mutant == "census_not_decremented":
                before = min(before, after)
            self.nonfinite = self.nonfinite - before + after
        return OK

    def set_blas_addresses(self, addresses):
        addresses = np.array(addresses, dtype=np.uint64, copy=True).reshape(-1)
        if not self.have_meshes or len(addresses) != self.m:
            return INVALID
        self.blas = addresses
        return OK

    def set_geometry(self, vertices, indices):
        self.vertices = np.array(vertices, dtype=np.float32, copy=True).reshape(-1, 3)
        self.indices = np.array(indices, dtype=np.uint32, copy=True).reshape(-1)
        self.have_geometry = True
        if self.mutant != "clusters_kept_across_set_geometry":
            self.clusters_valid = self.cones_valid = False
        return OK

    def _levels_fit(self):
        """Every level's range inside the indices, every vertex its whole triangles name inside the vertices."""
        for k in range(len(self.meshes)):
            mesh = self.meshes[k]
            for l in range(int(mesh["n_lods"])):
                off, length = int(mesh["index_offset"][l]), int(mesh["index_len"][l])
                if off + length > len(self.indices):
                    return False
                used = length // 3 * 3
                if used:
                    vo = int(mesh["vertex_offset"])
                    if vo < 0 or vo + int(self.indices[off:off + used].max()) >= len(self.vertices):
                        return False
        return True

    def build_clusters(self):
        if not self.have_meshes or not self.have_geometry:
            return NOT_READY
        if not self._levels_fit():
            return INVALID
        self.clusters_valid, self.cones_valid = True, False
        return OK

    def build_cluster_cones(self):
        if not self.clusters_valid:
            return NOT_READY
        self.cones_valid = True
        return OK
