"""Row f-1 on the CPU: is the oracle of the per-triangle stage (orc_cull_triangles, orc_cull_all_triangles,
orc_src_index_offsets) what generate_work.comp:68-200 says? Three answers, none of which reads the oracle's own output as
truth: the numpy float32 restatement (bit equality), hand-built known answers, and the decision evaluated in float64 on
every triangle that rounding cannot decide."""
import ctypes as C

import numpy as np
import pytest

import float64_reference as f64
import numpy_restatement as npr
import triangle_cases as tc
from renderer_amd import scene


def _frame(oracle_mod, s, threads=None, **bases):
    return oracle_mod.run(s["pos"], s["rot"], s["scale"], s["mesh_id"], s["meshes"], s["planes"], s["cam_pos"], threads=threads, **bases)


def assert_oracle_equals_restatement(oracle_mod, s, vertices, indices, pv, first_instance_base=0, first_index_base=0, what=""):
    """Frame -> src offsets -> per-triangle cull -> re-compaction, by the oracle (1 and 8 threads) and by the restatement:
    commands (bytes), count, the WHOLE stream (untouched slots included) and the source offsets."""
    r = _frame(oracle_mod, s, first_instance_base=first_instance_base, first_index_base=first_index_base)
    capacity = first_index_base + r["draw_index_total"] + 3
    src = npr.src_index_offsets(s["pos"], s["mesh_id"], r["coarse_culled"], s["meshes"], s["cam_pos"])
    want_cmds, want_out = npr.cull_all_triangles(r["draw_cmds"], src, r["model"], first_instance_base, pv, vertices, indices, capacity)
    for threads in (1, 8):
        cmds, out, got_src = oracle_mod.cull_all_triangles(r, s["pos"], s["mesh_id"], s["meshes"], s["cam_pos"], pv, vertices, indices,
                                                           first_instance_base=first_instance_base, out_capacity=capacity, threads=threads)
        assert np.array_equal(got_src, src), (what, threads, "src_index_offset")
        assert len(cmds) == len(want_cmds), (what, threads, len(cmds), len(want_cmds))
        assert cmds.tobytes() == want_cmds.tobytes(), (what, threads, "final commands")
        assert np.array_equal(out, want_out), (what, threads, "culled stream", int((out != want_out).sum()))
    return r, want_cmds, want_out


@pytest.mark.parametrize("config,n", [(1, 1024), (2, 60), (3, 1500)])
@pytest.mark.parametrize("all_visible", [False, True])
def test_oracle_equals_restatement_on_the_configs(oracle_mod, config, n, all_visible):
    s = scene.make_scene(config, n=n, all_visible=all_visible)
    vertices, indices = scene.make_geometry(s["meshes"])
    r, cmds, out = assert_oracle_equals_restatement(oracle_mod, s, vertices, indices, scene.default_pv(), what=(config, n, all_visible))
    survivors = int(cmds["indexCount"].astype(np.int64).sum())
    assert 0 < survivors < int(r["draw_cmds"]["indexCount"].astype(np.int64).sum())   # something was culled, something survived


@pytest.mark.parametrize("ordering", ["rows", "strips", "shuffled"])
def test_oracle_equals_restatement_on_every_mesh_layout(oracle_mod, ordering):
    for config, n in ((3, 700), (2, 40)):
        s = scene.make_scene(config, n=n, all_visible=(config == 2))
        s["pos"][11, 1] = np.nan
        vertices, indices = scene.make_geometry(s["meshes"], ordering=ordering)
        assert_oracle_equals_restatement(oracle_mod, s, vertices, indices, scene.default_pv(), first_instance_base=5, what=(ordering, config))


def special_instances_scene(n=400):
    """The instances of test_gpu_triangles.py::test_triangle_cull_special_instances_and_bases."""
    s = scene.make_scene(3, n=n, all_visible=True)
    s["pos"][5, 0] = np.nan          # NaN model matrix: every comparison is false, so every triangle survives
    s["scale"][7] = 0.0              # degenerate: all vertices coincide
    s["scale"][9] = -1.0             # mirrored: winding flips
    s["rot"][11] = (0, 0, 0, 3.0)    # non-unit quaternion
    return s


def test_oracle_equals_restatement_special_instances_and_instance_base(oracle_mod):
    s = special_instances_scene()
    vertices, indices = scene.make_geometry(s["meshes"])
    r, cmds, out = assert_oracle_equals_restatement(oracle_mod, s, vertices, indices, scene.default_pv(), first_instance_base=1000)
    by_instance = {int(c["firstInstance"]) - 1000: int(c["indexCount"]) for c in cmds}
    frame = {int(c["firstInstance"]) - 1000: int(c["indexCount"]) for c in r["draw_cmds"]}
    assert by_instance[5] == frame[5] // 3 * 3     # NaN matrix: nothing is culled
    assert by_instance[7] == frame[7] // 3 * 3     # zero scale: det = 0, every corner at the instance's (visible) position


def shortened_index_counts(meshes):
    """The table of test_gpu_triangles.py::test_triangle_cull_index_base_and_index_counts_that_are_no_multiple_of_three:
    index counts of 3k+1 and 3k+2, and commands of 2 and 1 indices."""
    meshes = meshes.copy()
    for k in range(len(meshes)):
        for lod in range(int(meshes["n_lods"][k])):
            if (k + lod) % 3 == 1 and meshes["index_len"][k][lod] > 4:
                meshes["index_len"][k][lod] -= 1 + (k % 2)
    meshes["index_len"][5][:] = 2
    meshes["index_len"][9][:] = 1
    return meshes


def test_oracle_equals_restatement_index_base_and_counts_that_are_no_multiple_of_three(oracle_mod):
    s = scene.make_scene(3, n=1200)
    vertices, indices = scene.make_geometry(s["meshes"])   # the geometry of the unshortened table
    s["meshes"] = shortened_index_counts(s["meshes"])
    lens = s["meshes"]["index_len"]
    assert (lens % 3 == 1).any() and (lens % 3 == 2).any()
    r, cmds, out = assert_oracle_equals_restatement(oracle_mod, s, vertices, indices, scene.default_pv(), first_index_base=5)
    assert (r["draw_cmds"]["firstIndex"] % 3 != 0).any() and (r["draw_cmds"]["indexCount"] < 3).any()
    assert not (cmds["indexCount"] % 3).any()


def test_oracle_equals_restatement_non_finite_positions(oracle_mod):
    s = scene.make_scene(2, n=50, all_visible=True)
    vertices, indices = scene.make_geometry(s["meshes"])
    vertices = vertices.copy()
    vertices[10, 0] = np.inf
    vertices[200, 1] = -np.inf
    vertices[3000, 2] = np.nan
    assert_oracle_equals_restatement(oracle_mod, s, vertices, indices, scene.default_pv())


# ---- known answers ---------------------------------------------------------------------------------------------------

def oracle_keeps(oracle_mod, model, pv, vertices, indices, src=0, vertex_offset=0, n_tris=None):
    """The oracle's decision per triangle: every triangle as a command of its own (3 indices at slot t), so that a kept
    triangle is a written slot and a culled one an untouched slot."""
    indices = np.ascontiguousarray(indices, np.uint32)
    vertices = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    n_tris = len(indices) // 3 if n_tris is None else n_tris
    cmds = np.zeros(n_tris, oracle_mod.DRAW_CMD_DTYPE)
    cmds["indexCount"] = 3
    cmds["instanceCount"] = 1
    cmds["firstIndex"] = 3 * np.arange(n_tris)
    cmds["vertexOffset"] = vertex_offset
    srcs = (src // 3 * 3 + 3 * np.arange(n_tris)).astype(np.uint32)
    out = np.full(3 * n_tris, 0xFFFFFFFF, np.uint32)
    model = np.ascontiguousarray(model, np.float32).reshape(1, 16)
    pv = np.ascontiguousarray(pv, np.float32).reshape(16)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    count = oracle_mod.lib().orc_cull_all_triangles(p(cmds), C.c_uint32(n_tris), p(srcs), p(model), C.c_uint32(0), p(pv), p(vertices), p(indices),
                                                    p(out), C.c_uint32(1))
    kept = out.reshape(n_tris, 3)[:, 0] != 0xFFFFFFFF
    assert count == int(kept.sum())
    assert np.array_equal(out.reshape(n_tris, 3)[kept], indices[srcs[0] : srcs[0] + 3 * n_tris].reshape(n_tris, 3)[kept])
    return kept


IDENTITY = np.eye(4, dtype=np.float32).reshape(16)


def test_known_answers(oracle_mod):
    """The per-triangle test against answers derived from the shader's text (tests/triangle_cases.py has the derivation:
    which winding `det > 0` culls under this projection, where the x / y bounds lie, that z is never tested, what w < 0 and
    w = 0 do to the formulas, NaN, zero area). Identity model, default pv. The expected column is written by hand; the
    oracle, the restatement and the float64 evaluation each have to give it."""
    vertices, indices = tc.case_mesh()
    pv = scene.default_pv()
    want = np.array([kept for _, _, kept, _ in tc.CASES])
    names = [name for name, _, _, _ in tc.CASES]
    got = oracle_keeps(oracle_mod, IDENTITY, pv, vertices, indices)
    assert got.tolist() == want.tolist(), [n for n, g, w in zip(names, got, want) if g != w]
    v = vertices[indices.astype(np.int64)].reshape(-1, 3, 3)
    assert (~npr.triangle_culled(IDENTITY, pv, v)).tolist() == want.tolist()
    culled64, decided = f64.triangle_decisions(IDENTITY, pv, v)
    finite = np.array([np.isfinite(np.array(corners, np.float64)).all() for _, corners, _, _ in tc.CASES])
    assert (~culled64)[finite].tolist() == want[finite].tolist()
    # the clear-cut cases are far from every threshold; the ones built ON a threshold (w = 0, zero area) are not "decided"
    clear = [names.index(n) for n in ("front_ccw_on_screen", "front_two_corners_swapped", "left_of_frustum", "above_frustum", "straddles_x_bound",
                                      "beyond_far_plane", "behind_camera_swapped", "behind_camera_left_swapped")]
    assert decided[clear].all() and not decided[names.index("zero_area")] and not decided[names.index("one_corner_w_zero_inside")]


def test_known_answers_hand_arithmetic():
    """The numbers the case table quotes, recomputed in float64 from the camera's definition alone (no pv array, no code
    under test): a = 1 / (2 tan 35 deg), clip = (a x, 2a (y - 1), z - 2)."""
    a = 1.0 / (2.0 * np.tan(np.radians(35.0)))
    pv = scene.default_pv().astype(np.float64).reshape(4, 4).T
    want = np.array([[a, 0, 0, 0], [0, 2 * a, 0, -2 * a], [0, 0, 0, 0], [0, 0, 1, -2]])
    assert np.allclose(pv[[0, 1, 3]], want[[0, 1, 3]], rtol=1e-7, atol=1e-7)   # rows x, y, w (z is never used)
    cases = {name: (np.array(corners, np.float64), kept) for name, corners, kept, _ in tc.CASES}

    def clip(p):
        return np.stack([a * p[:, 0], 2 * a * (p[:, 1] - 1.0), p[:, 2] - 2.0], axis=1)   # x, y, w

    def hand(p):
        c = clip(p)
        det = np.linalg.det(c.T)    # columns = the corners' xyw
        with np.errstate(all="ignore"):
            ndc = c[:, :2] / c[:, 2:3]
        out = any((ndc[:, k] < -1).all() or (ndc[:, k] > 1).all() for k in range(2))
        return det, ndc, not (det > 0 or out)

    for name, (p, kept) in cases.items():
        if not np.isfinite(p).all():
            continue
        det, ndc, k = hand(p)
        assert k == kept, (name, det, ndc)
    assert hand(cases["front_ccw_on_screen"][0])[0] < 0 < hand(cases["front_two_corners_swapped"][0])[0]
    assert np.allclose(hand(cases["straddles_x_bound"][0])[1][:, 0], [0.964, 1.035, 1.107], atol=1e-3)
    assert hand(cases["zero_area"][0])[0] == 0.0


def test_known_answers_mirrored_instance(oracle_mod):
    """Scale -1 with a half turn about y is the reflection y -> 2 - y: the decision of the front-facing triangle and of its
    swapped twin flip against the identity's."""
    model = oracle_mod.model_matrix(tc.MIRROR_INSTANCE["pos"], tc.MIRROR_INSTANCE["rot"], tc.MIRROR_INSTANCE["scale"])
    assert np.array_equal(model.reshape(4, 4).T, np.array([[1, 0, 0, 0], [0, -1, 0, 2], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32))
    vertices, indices = tc.case_mesh(tc.MIRROR_CASES)
    pv = scene.default_pv()
    want = [kept for _, _, kept, _ in tc.MIRROR_CASES]
    assert oracle_keeps(oracle_mod, model, pv, vertices, indices).tolist() == want
    assert oracle_keeps(oracle_mod, IDENTITY, pv, vertices, indices).tolist() == [not k for k in want]
    v = vertices[indices.astype(np.int64)].reshape(-1, 3, 3)
    assert (~npr.triangle_culled(model, pv, v)).tolist() == want
    assert (~f64.triangle_decisions(model, pv, v)[0]).tolist() == want


def test_survivors_land_at_first_index_over_three_and_sources_follow_the_lod(oracle_mod):
    """Placement, by hand: two commands over one mesh whose two LODs hold DIFFERENT triangles. The far instance must read
    LOD 1's range (src = index_offset[1]), its survivors go to out[firstIndex / 3 * 3 ...] in order, indexCount = 3 x
    survivors; a command whose only triangle is culled disappears."""
    front, back = tc.tri(0, 1, 0), tc.swapped(tc.tri(0, 1, 0))   # around the instance's origin
    vertices = np.array(front + back, np.float32)                # vertices 0-2 front-facing, 3-5 back-facing
    # LOD 0 (indices 0..8): front, back, front.   LOD 1 (indices 9..14): back, front
    indices = np.array([0, 1, 2, 3, 4, 5, 0, 1, 2, 3, 4, 5, 0, 1, 2], np.uint32)
    meshes = np.zeros(1, oracle_mod.ORC_MESH_DTYPE)
    meshes["aabb_min"], meshes["aabb_max"] = (-1, 0, -0.1), (1, 3, 0.1)
    meshes["n_lods"] = 2
    meshes["index_len"][0, :2] = (9, 6)
    meshes["index_offset"][0, :2] = (0, 9)
    pos = np.array([[0, 0, 8], [0, 0, 30]], np.float32)          # distance 6.1 (LOD 0) and 28 (LOD 1) from the camera at (0, 1, 2)
    s = dict(pos=pos, rot=np.array([[0, 0, 0, 1]] * 2, np.float32), scale=np.ones(2, np.float32), mesh_id=np.zeros(2, np.uint32),
             meshes=meshes, planes=scene.default_planes(), cam_pos=np.array([0, 1, 2], np.float32))
    r = _frame(oracle_mod, s, first_index_base=7)
    assert r["draw_cmds"]["indexCount"].tolist() == [9, 6] and r["draw_cmds"]["firstIndex"].tolist() == [7, 16]
    cmds, out, src = oracle_mod.cull_all_triangles(r, pos, s["mesh_id"], meshes, s["cam_pos"], scene.default_pv(), vertices, indices, out_capacity=24)
    assert src.tolist() == [0, 9]
    assert npr.src_index_offsets(pos, s["mesh_id"], r["coarse_culled"], meshes, s["cam_pos"]).tolist() == [0, 9]
    assert cmds["indexCount"].tolist() == [6, 3] and cmds["firstIndex"].tolist() == [7, 16]
    want = np.full(24, 0xFFFFFFFF, np.uint32)
    want[6:12] = [0, 1, 2, 0, 1, 2]     # 7 / 3 = 2: slot 2 = words 6..; LOD 0's two front-facing triangles, in order
    want[15:18] = [0, 1, 2]             # 16 / 3 = 5: words 15..; LOD 1's one front-facing triangle
    assert out.tolist() == want.tolist()


# ---- float64 ---------------------------------------------------------------------------------------------------------

def _decisions(oracle_mod, s, vertices, indices, pv):
    """Per command of the frame: the oracle's keep flags, the float64 decision and `decided`, concatenated."""
    r = _frame(oracle_mod, s)
    src = npr.src_index_offsets(s["pos"], s["mesh_id"], r["coarse_culled"], s["meshes"], s["cam_pos"])
    keeps, culled64, decided = [], [], []
    for c, so in zip(r["draw_cmds"], src):
        n_tris = int(c["indexCount"]) // 3
        keeps.append(oracle_keeps(oracle_mod, r["model"][int(c["firstInstance"])], pv, vertices, indices, src=int(so), vertex_offset=int(c["vertexOffset"]),
                                  n_tris=n_tris))
        ix = indices[int(so) // 3 * 3 : int(so) // 3 * 3 + 3 * n_tris].reshape(n_tris, 3).astype(np.int64) + int(c["vertexOffset"])
        c64, dec = f64.triangle_decisions(r["model"][int(c["firstInstance"])], pv, vertices[ix])
        culled64.append(c64)
        decided.append(dec)
    return np.concatenate(keeps), np.concatenate(culled64), np.concatenate(decided)


def test_oracle_against_float64_decisions_box_scene(oracle_mod):
    """Config 1 (box, 1 024 instances): wherever the float32 chain's forward error bound (float64_reference.TRIANGLE_K,
    derived from its operation count) cannot reach a threshold, the oracle's keep / cull IS the float64 decision — no
    exception — and that covers at least 0.95 of the scene's triangles (a condition of the test: below it the test would be
    vacuous and fails)."""
    s = scene.make_scene(1)
    vertices, indices = scene.make_geometry(s["meshes"])
    keep, culled64, decided = _decisions(oracle_mod, s, vertices, indices, scene.default_pv())
    share = decided.mean()
    wrong = int((keep[decided] == culled64[decided]).sum())
    print(f"box scene: {len(keep)} triangles, decided {share:.4f} at K = {f64.TRIANGLE_K}, disagreements among decided {wrong}, among all {int((keep == culled64).sum())}")
    assert len(keep) > 3000
    assert wrong == 0
    assert share >= 0.95


@pytest.mark.parametrize("config,n", [(2, 60), (3, 1500)])
def test_oracle_against_float64_decisions_dense_meshes(oracle_mod, config, n):
    """The dense synthetic meshes: distant sub-pixel triangles, most of them within rounding distance of det = 0 — the decided
    share is printed, not asserted; among the decided ones there is no disagreement."""
    s = scene.make_scene(config, n=n, all_visible=(config == 2))
    vertices, indices = scene.make_geometry(s["meshes"])
    keep, culled64, decided = _decisions(oracle_mod, s, vertices, indices, scene.default_pv())
    wrong = int((keep[decided] == culled64[decided]).sum())
    print(f"config {config} n={n}: {len(keep)} triangles, decided {decided.mean():.4f} at K = {f64.TRIANGLE_K}, disagreements among decided {wrong}, "
          f"among all {int((keep == culled64).sum())}")
    assert decided.any()
    assert wrong == 0
