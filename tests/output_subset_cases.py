"""Every valid subset of a frame's six outputs (MipOutputs: model, tlas_instances, world_aabb, visible_bitmap, draw_cmds +
draw_count, draw_index_total), the scene and the sizes they are run at, the buffers they are run into, and wrong pipelines
that the comparison must catch. Pure Python: no GPU, no HIP. tests/test_output_subset_cases.py proves on the CPU that the
comparison bites (every mutant is killed); tests/test_gpu_output_subsets.py runs the same comparison on the kernels.

The frame kernel (renderer_amd/csrc/instance_kernel.hpp) leaves through a different exit, stages or does not stage its
matrices, and stores its boxes and bitmap words from different waves, depending on WHICH outputs are NULL; plan_frame
(frame_plan.hpp) picks the order and whether the launch takes a prefix tag from the same subset."""
import ctypes as C
import itertools
import json
import subprocess

import numpy as np

NAMES = ("model", "tlas", "aabb", "bitmap", "cmds", "index_total")
_LETTER = dict(model="m", tlas="t", aabb="a", bitmap="b", cmds="c", index_total="i")
# run_device's keyword of every output ("cmds" also carries draw_count)
KEYWORD = dict(model="model", tlas="tlas_instances", aabb="world_aabb", bitmap="visible_bitmap", cmds="draw_cmds",
               index_total="draw_index_total")


def _all_combinations():
    return [frozenset(n for n, bit in zip(NAMES, bits) if bit) for bits in itertools.product((0, 1), repeat=len(NAMES))]


# draw_index_total only beside draw_cmds: 32 subsets without it + 16 with both = 48, the empty one among them
SUBSETS = [s for s in _all_combinations() if "index_total" not in s or "cmds" in s]
EMPTY = frozenset()
ALL = frozenset(NAMES)


def subset_id(subset):
    return "-".join(_LETTER[n] for n in NAMES if n in subset) or "none"


def subset_of(text):
    """'m-t-c' or 'model,cmds' -> the frozenset."""
    by_letter = {v: k for k, v in _LETTER.items()}
    if text in ("", "none"):
        return EMPTY
    return frozenset(by_letter.get(w, w) for w in text.replace(",", "-").split("-"))


def plan_request(subset, *extra):
    """The request= string of tests/native/frame_plan_probe.cpp for a subset (draw_cmds always goes with draw_count; the
    probe's own word `cmds` would add draw_index_total too)."""
    words = [n for n in ("model", "tlas", "aabb", "bitmap") if n in subset]
    if "cmds" in subset:
        words += ["draw_cmds", "count"]
    if "index_total" in subset:
        words.append("index_total")
    return ",".join(words + list(extra))


def probe_status(words, n=1000, **state):
    """plan_frame's verdict on ANY combination of request words, valid or not: the probe's JSON line (status != 0: refused)."""
    import plan_boundaries as pb

    args = dict(state, n=int(n), request=",".join(words))
    out = subprocess.run([pb.probe_exe()] + [f"{k}={v}" for k, v in args.items()], capture_output=True, text=True, timeout=60, check=True)
    return json.loads(out.stdout.splitlines()[0])


# ---- sizes: the smallest at which each guard of the kernel can fail ----
SIZES = {
    0: "counts zeroed, nothing else touched",
    1: "a single lane",
    33: "two bitmap words; the third 16-matrix piece holds one row",
    257: "two tiles, the last one with one instance, one predecessor in the prefix",
    1000: "ragged last tile of 232 instances: a piece cut in half, a last bitmap word of 8 bits",
    4129: "17 tiles: the last tile is the first of a second level-1 group (group_shift 4)",
}
TILE = 256

INSTANCE_BASE = 123_456
INDEX_BASE = 0xFFFFFFF0            # the second command's firstIndex has wrapped past 2^32
# where the edited instances stand (camera at (0, 1, 2), looking down +z; LOD 1 beyond a distance of 10)
_NEAR = (0.0, 1.0, 8.0)
_FAR = (0.5, 1.5, 40.0)


def blas_addresses(n_meshes):
    """Distinct per mesh, both 32-bit halves non-zero and distinct per mesh."""
    k = np.arange(n_meshes, dtype=np.uint64)
    return ((np.uint64(0x1000) + k) << np.uint64(32)) | (np.uint64(0xA0000000) + np.uint64(0x100) * k)


def subset_scene(n, n_meshes=None, top_mesh_in_last_tile=False):
    """The first n instances of scene.make_scene(3), edited so that the frame is not vacuous where the kernel's guards are
    (the unedited scene: nothing visible at n = 1, the one instance of the second tile culled at n = 257, draw_count equal to
    the visible count everywhere because no level is empty):
      instance 0     near, a two-LOD mesh: visible, LOD 0;          instance n - 1  far, a two-LOD mesh: visible, LOD 1
      instance 1     far, a mesh whose LOD 1 is EMPTY: visible, no command (n >= 33)
      instance 2     far, a one-LOD mesh: visible, LOD 0 from beyond the LOD switch (n >= 33)
    n_meshes: a table of that many entries instead of the 64 (entries repeat the 64 with a shifted vertex_offset; ids are
    spread over the whole table); top_mesh_in_last_tile: instances of the highest id in the last tile."""
    from renderer_amd import scene

    n = int(n)
    s = scene.make_scene(3, n=max(n, 1))
    meshes = s["meshes"].copy()
    if n_meshes is not None and n_meshes != len(meshes):
        reps = -(-n_meshes // len(meshes))
        big = np.tile(meshes, reps)[:n_meshes].copy()
        big["vertex_offset"] = big["vertex_offset"] + (np.arange(n_meshes) // len(meshes)).astype(np.int32) * 7
        ids = s["mesh_id"].astype(np.uint64)
        if n_meshes > len(meshes):   # spread the ids over the whole table, entry k + 64 j is a copy of entry k
            spread = (np.arange(len(ids), dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(reps)
            ids = np.minimum(ids + spread * np.uint64(len(meshes)), np.uint64(n_meshes - 1))
        else:
            ids = ids % np.uint64(n_meshes)
        s["mesh_id"] = ids.astype(np.uint32)
        meshes = big
    two = np.nonzero((meshes["n_lods"] >= 2) & (meshes["index_len"][:, 0] > 0) & (meshes["index_len"][:, 1] > 0))[0]
    one = np.nonzero((meshes["n_lods"] == 1) & (meshes["index_len"][:, 0] > 0))[0]
    if len(meshes) >= 4:
        assert len(two) >= 3 and len(one) >= 1, "the mixed table has meshes of one and of several LODs"
        hollow = int(two[2])
        meshes["index_len"][hollow, 1] = 0          # a visible instance beyond the LOD switch draws nothing
        s["hollow_mesh"] = hollow
    for key in ("pos", "rot", "scale", "mesh_id"):
        s[key] = s[key][:n].copy()
    if n >= 1:
        s["pos"][0] = _NEAR
        if len(meshes) >= 4:
            s["mesh_id"][0] = two[0]
    if n >= 33 and len(meshes) >= 4:
        s["pos"][1] = _FAR
        s["mesh_id"][1] = hollow
        s["pos"][2] = (-0.5, 0.5, 45.0)
        s["mesh_id"][2] = one[0]
    if n >= 2:
        s["pos"][n - 1] = _FAR
        if len(meshes) >= 4:
            s["mesh_id"][n - 1] = two[1]
    if top_mesh_in_last_tile and n >= 8:
        first = ((n - 1) // TILE) * TILE
        for i in sorted({first, max(first, n - 5), n - 1}):
            s["mesh_id"][i] = len(meshes) - 1
            s["pos"][i] = (0.25 * (i - first) / TILE, 1.0, 30.0)
    s.update(n=n, meshes=meshes, blas=blas_addresses(len(meshes)), base=INSTANCE_BASE, index_base=INDEX_BASE)
    return s


def oracle_frame(oracle_mod, s, cam_pos=None, base=None, index_base=None, planes=None):
    """The oracle's frame of a subset_scene (n = 0 included: two zero counts and empty arrays), with the TLAS rows."""
    n = s["n"]
    base = s["base"] if base is None else base
    index_base = s["index_base"] if index_base is None else index_base
    if n == 0:
        from renderer_amd.pipeline import DRAW_CMD_DTYPE

        return dict(model=np.zeros((0, 16), np.float32), world_aabb=np.zeros((0, 6), np.float32), visible_bitmap=np.zeros(0, np.uint32),
                    draw_cmds=np.zeros(0, DRAW_CMD_DTYPE), draw_count=0, draw_index_total=0, tlas=np.zeros((0, 16), np.uint32),
                    coarse_culled=np.zeros(0, np.uint8))
    want = oracle_mod.run(s["pos"], s["rot"], s["scale"], s["mesh_id"], s["meshes"], s["planes"] if planes is None else planes, s["cam_pos"] if cam_pos is None else cam_pos,
                          first_instance_base=base, first_index_base=index_base)
    want["tlas"] = oracle_mod.tlas_instances(want["model"], s["mesh_id"], s["blas"], first_instance_base=base)
    return want


def scene_conditions(oracle_mod, s, want):
    """Asserts that the frame exercises what subset_scene promises (module docstring of the scene)."""
    from helpers import popcount_bitmap

    n = s["n"]
    assert s["base"] != 0 and s["index_base"] != 0
    blas = s["blas"]
    assert len(set(blas.tolist())) == len(blas) and (blas >> np.uint64(32)).all() and (blas & np.uint64(0xFFFFFFFF)).all()
    assert len(set((blas & np.uint64(0xFFFFFFFF)).tolist())) == len(blas) and len(set((blas >> np.uint64(32)).tolist())) == len(blas)
    if n == 0:
        return
    cmds = want["draw_cmds"]
    drawn = (cmds["firstInstance"] - np.uint32(s["base"])).astype(np.int64)
    bits = np.unpackbits(want["visible_bitmap"].view(np.uint8), bitorder="little")
    for i in {0, n - 1}:
        assert bits[i] and i in drawn, f"n={n}: instance {i} is visible and emits a command"
    if n < 33:
        return
    assert popcount_bitmap(want["visible_bitmap"]) > want["draw_count"], f"n={n}: a visible instance draws an empty level"
    assert bits[1] and 1 not in drawn
    meshes, ids = s["meshes"], s["mesh_id"][drawn]
    far = np.array([oracle_mod.pick_lod(2, s["cam_pos"], s["pos"][i]) for i in drawn], bool)
    lod1 = far & (meshes["n_lods"][ids] > 1)
    assert lod1.any() and (~far).any(), f"n={n}: both LODs occur among the commands"
    assert (cmds["indexCount"][lod1] == meshes["index_len"][ids[lod1], 1]).all()
    assert (far & (meshes["n_lods"][ids] == 1)).any(), f"n={n}: a one-LOD mesh is seen from beyond the LOD switch"
    first = cmds["firstIndex"].astype(np.int64)
    assert (first[1:] < first[:-1]).sum() == 1 and first[0] == s["index_base"], f"n={n}: firstIndex wraps past 2^32 inside the list"


# ---- buffers ----
SENTINEL = 0x5A5A5A5A
SLACK = 64                    # sentinel rows / words in front of and behind every buffer
_ROW_WORDS = dict(model=16, tlas=16, aabb=6, bitmap=1, cmds=5)
# scalar words: draw_count and draw_index_total are NOT neighbours, so a total written through a NULL request shows
SCALAR_WORDS, COUNT_WORD, TOTAL_WORD = 8, 2, 5


class NumpyBackend:
    """Host memory: the CPU pipelines of the tests, and MIP_OUT_HOST outputs."""

    def full(self, words):
        return np.full(words, SENTINEL, np.uint32)

    def ptr(self, buf):
        return buf.ctypes.data

    def read(self, buf):
        return buf.copy()

    def fill(self, buf):
        buf[:] = SENTINEL

    def sync(self):
        pass


class TorchBackend:
    """Device memory of cuda:0."""

    def __init__(self):
        import torch

        self.torch, self.dev = torch, torch.device("cuda", 0)

    def full(self, words):
        return self.torch.full((words,), SENTINEL, dtype=self.torch.int32, device=self.dev)

    def ptr(self, buf):
        return buf.data_ptr()

    def read(self, buf):
        return buf.cpu().numpy().view(np.uint32)

    def fill(self, buf):
        buf.fill_(SENTINEL)

    def sync(self):
        self.torch.cuda.synchronize()


class SubsetOutputs:
    """One buffer per requested output of `subset`, for frames of up to `capacity` instances: SLACK sentinel rows in front
    (every front is a multiple of 256 bytes, so the 16-byte stores of matrices, TLAS rows and wire blocks stay aligned) and
    behind. Outputs outside `subset` have no buffer and a 0 pointer. wire: False | True | "packed" (draw_cmds in a wire form).
    request(active) narrows what the next frames ask for to a part of `subset` — one allocation serves a loop over subsets —:
    the buffers of the outputs left out get a 0 pointer too, and check() wants every word of them intact."""

    def __init__(self, backend, capacity, subset, wire=False):
        from renderer_amd.pipeline import wire_body_bytes

        self.be, self.capacity, self.subset, self.wire = backend, int(capacity), frozenset(subset), wire
        self.active = self.subset
        self.front, self.buf = {}, {}
        for name in ("model", "tlas", "aabb", "bitmap", "cmds"):
            if name not in self.subset:
                continue
            rows = (self.capacity + 31) // 32 if name == "bitmap" else max(self.capacity, 1)
            words = rows * _ROW_WORDS[name]
            if name == "cmds" and wire:
                words = wire_body_bytes(max(self.capacity, 1), packed=wire == "packed") // 4
            self.front[name] = SLACK * _ROW_WORDS[name] if name != "bitmap" else SLACK
            assert (self.front[name] * 4) % 256 == 0
            self.buf[name] = backend.full(self.front[name] + words + SLACK * _ROW_WORDS[name])
        self.scal = backend.full(SCALAR_WORDS)
        backend.sync()

    def request(self, active):
        active = frozenset(active)
        assert active <= self.subset, (subset_id(active), subset_id(self.subset))
        self.active = active
        return self

    def address(self, name):
        return self.be.ptr(self.buf[name]) + 4 * self.front[name]

    def pointers(self):
        """run_device's keywords; unrequested outputs are 0."""
        d = {KEYWORD[name]: (self.address(name) if name in self.active else 0) for name in ("model", "tlas", "aabb", "bitmap", "cmds")}
        d["draw_count"] = self.be.ptr(self.scal) + 4 * COUNT_WORD if "cmds" in self.active else 0
        d["draw_index_total"] = self.be.ptr(self.scal) + 4 * TOTAL_WORD if "index_total" in self.active else 0
        return d

    def refill(self):
        for b in self.buf.values():
            self.be.fill(b)
        self.be.fill(self.scal)
        self.be.sync()

    def untouched(self, what="nothing"):
        """No word of any buffer was written."""
        self.be.sync()
        for name, b in self.buf.items():
            assert (self.be.read(b) == SENTINEL).all(), f"{what}: {name} was written"
        assert (self.be.read(self.scal) == SENTINEL).all(), f"{what}: a scalar word was written"

    def check(self, oracle_mod, scene, want, n, base, what):
        """Requested outputs against the oracle's frame `want` of the scene's n instances: integers and commands byte for byte,
        matrices, boxes and TLAS transform words identical as numbers, TLAS index / mask / address words exactly (against
        want["tlas"], or oracle.tlas_instances with the scene's BLAS addresses) — and every sentinel word in front of and
        behind what the frame owns, command rows behind draw_count included, an unrequested draw_index_total and the scalar
        words beside draw_count."""
        from cpu_pipeline import decode_wire, unpack_wire
        from helpers import float_mismatches
        from renderer_amd.pipeline import DRAW_CMD_DTYPE, wire_body_bytes

        self.be.sync()
        what = f"{what} [{subset_id(self.active)}]"
        sub = self.active
        assert n <= self.capacity
        for name, b in self.buf.items():
            if name not in sub:
                assert (self.be.read(b) == SENTINEL).all(), f"{what}: {name} was not requested and was written"

        def split(name, owned_words):
            all_words = self.be.read(self.buf[name])
            f = self.front[name]
            assert (all_words[:f] == SENTINEL).all(), f"{what}: {name}: a word in front of the buffer was written"
            behind = all_words[f + owned_words:]
            bad = np.nonzero(behind != SENTINEL)[0]
            assert len(bad) == 0, f"{what}: {name}: word {int(bad[0])} behind the frame's {owned_words} words was written"
            return all_words[f:f + owned_words]

        scal = self.be.read(self.scal)
        quiet = [w for w in range(SCALAR_WORDS) if not ((w == COUNT_WORD and "cmds" in sub) or (w == TOTAL_WORD and "index_total" in sub))]
        for w in quiet:
            assert scal[w] == SENTINEL, f"{what}: scalar word {w} was written (draw_count is word {COUNT_WORD}, draw_index_total word {TOTAL_WORD})"
        if "cmds" in sub:
            count = int(scal[COUNT_WORD])
            assert count == want["draw_count"], f"{what}: draw_count {count} vs {want['draw_count']}"
            if "index_total" in sub:
                assert int(scal[TOTAL_WORD]) == want["draw_index_total"], f"{what}: draw_index_total {int(scal[TOTAL_WORD])} vs {want['draw_index_total']}"
            if self.wire:
                packed = self.wire == "packed"
                body = split("cmds", wire_body_bytes(max(self.capacity, 1), packed=packed) // 4)
                got = decode_wire(unpack_wire(body, count) if packed else body, count, scene["meshes"])
            else:
                got = split("cmds", count * 5).view(DRAW_CMD_DTYPE)
            assert got.tobytes() == want["draw_cmds"].tobytes(), f"{what}: draw command bytes"
        if "bitmap" in sub:
            got = split("bitmap", (n + 31) // 32)
            assert np.array_equal(got, want["visible_bitmap"]), f"{what}: visibility bitmap"
        if "model" in sub:
            mm = float_mismatches(split("model", n * 16).view(np.float32).reshape(n, 16), want["model"])
            assert len(mm) == 0, f"{what}: {len(mm)} model matrix entries differ, first {mm[:4].tolist()}"
        if "aabb" in sub:
            mm = float_mismatches(split("aabb", n * 6).view(np.float32).reshape(n, 6), want["world_aabb"])
            assert len(mm) == 0, f"{what}: {len(mm)} world AABB entries differ, first {mm[:4].tolist()}"
        if "tlas" in sub:
            got = split("tlas", n * 16).reshape(n, 16)
            rows = want["tlas"] if "tlas" in want else oracle_mod.tlas_instances(want["model"], scene["mesh_id"][:n], scene["blas"], first_instance_base=base)
            bad = np.nonzero((got[:, 12:] != rows[:, 12:]).any(axis=1))[0]
            assert len(bad) == 0, f"{what}: TLAS index / mask / address words of {len(bad)} rows, first row {int(bad[0])}: {got[bad[0], 12:].tolist()} vs {rows[bad[0], 12:].tolist()}"
            mm = float_mismatches(got[:, :12].view(np.float32), rows[:, :12].view(np.float32))
            assert len(mm) == 0, f"{what}: {len(mm)} TLAS transform entries differ, first {mm[:4].tolist()}"


# ---- wrong pipelines (CPU only: they patch the outputs of a pipeline that writes host memory) ----

def _words(ptr, count):
    return np.frombuffer((C.c_uint32 * count).from_address(ptr), dtype=np.uint32)


class _Mutant:
    """A pipeline that runs `inner` and then does one thing wrong. `inner`: run_device(frame, **pointers), .n, .blas."""

    name = "?"

    def __init__(self, inner):
        self.inner, self.n = inner, inner.n

    def run_device(self, frame, **kw):
        self.inner.run_device(frame, **kw)


class BitmapOnlyWithCommands(_Mutant):
    name = "bitmap written only when commands are"

    def run_device(self, frame, **kw):
        if not kw.get("draw_cmds"):
            kw = dict(kw, visible_bitmap=0)
        self.inner.run_device(frame, **kw)


class LastBitmapWordDropped(_Mutant):
    name = "last bitmap word of a ragged tile dropped when there are no commands"

    def run_device(self, frame, **kw):
        n, bitmap = self.n, kw.get("visible_bitmap")
        ragged = bitmap and not kw.get("draw_cmds") and n % TILE
        if ragged:
            last = _words(bitmap + 4 * ((n + 31) // 32 - 1), 1)
            before = int(last[0])
        self.inner.run_device(frame, **kw)
        if ragged:
            last[0] = before


class TlasFromStaleStaging(_Mutant):
    name = "TLAS rows taken from the matrix of the previous frame when model is NULL"

    def __init__(self, inner):
        super().__init__(inner)
        self.staged = np.zeros((max(self.n, 1), 16), np.uint32)     # what a frame with model left in the staging area

    def run_device(self, frame, **kw):
        self.inner.run_device(frame, **kw)
        n, tlas = self.n, kw.get("tlas_instances")
        if kw.get("model") and n:
            self.staged[:n] = _words(kw["model"], n * 16).reshape(n, 16)
        elif tlas and n:
            rows = _words(tlas, n * 16).reshape(n, 16)
            rows[:, :12] = self.staged[:n].reshape(n, 4, 4)[:, :, :3].transpose(0, 2, 1).reshape(n, 12)


class RowPastTheEnd(_Mutant):
    def __init__(self, inner, which):
        super().__init__(inner)
        self.which = which
        self.name = f"one row past n written for {which}"

    def run_device(self, frame, **kw):
        self.inner.run_device(frame, **kw)
        ptr, n, w = kw.get(KEYWORD[self.which]), self.n, _ROW_WORDS[self.which]
        if ptr and n:
            rows = _words(ptr, (n + 1) * w)
            rows[n * w:] = rows[(n - 1) * w:n * w]


class TotalThroughNull(_Mutant):
    name = "draw_index_total written through a NULL request (into the word behind draw_count)"

    def run_device(self, frame, **kw):
        self.inner.run_device(frame, **kw)
        if kw.get("draw_cmds") and not kw.get("draw_index_total"):
            _words(kw["draw_count"], 2)[1] = 7


class BlasOfMeshZero(_Mutant):
    name = "BLAS address of mesh 0 for every row"

    def run_device(self, frame, **kw):
        self.inner.run_device(frame, **kw)
        n, tlas = self.n, kw.get("tlas_instances")
        if tlas and n:
            rows = _words(tlas, n * 16).reshape(n, 16)
            rows[:, 14] = np.uint32(int(self.inner.blas[0]) & 0xFFFFFFFF)
            rows[:, 15] = np.uint32(int(self.inner.blas[0]) >> 32)


class BoxesOfWaveZeroMissing(_Mutant):
    name = "boxes of wave 0 missing when commands are requested"

    def run_device(self, frame, **kw):
        self.inner.run_device(frame, **kw)
        n, aabb = self.n, kw.get("world_aabb")
        if aabb and kw.get("draw_cmds") and n:
            rows = _words(aabb, n * 6).reshape(n, 6)
            rows[np.arange(n) % TILE < 64] = SENTINEL


def mutants():
    """[(name, factory)]: factory(pipeline) -> a pipeline that is wrong in the named way."""
    out = [(cls.name, cls) for cls in (BitmapOnlyWithCommands, LastBitmapWordDropped, TlasFromStaleStaging, TotalThroughNull, BlasOfMeshZero,
                                       BoxesOfWaveZeroMissing)]
    for which in ("tlas", "model", "aabb"):
        out.append((f"one row past n written for {which}", lambda inner, which=which: RowPastTheEnd(inner, which)))
    return out
