"""The normal cones of cluster culling without a GPU: the restatement (tests/cluster_cone_restatement.py) against the hand-written
tables and command lists (tests/cluster_cone_cases.py); mip_cone_from_pv through the library (it needs no device); the struct
in C, ctypes and the Rust text; header, EXPORTS and declarations; the plan check under ASan + UBSan; and the two properties
the margin is held to — (a) conservative in float64, (b) agreement with the per-triangle stage — with zero tolerance."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cluster_cases as cc
import cluster_cone_cases as ccc
import cluster_cone_restatement as ccr
import cluster_restatement as cr
import cluster_triangle_restatement as ctr
import lod_restatement as lr
import numpy_restatement as nr
import occlusion_restatement as orr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- the build ----

@pytest.mark.parametrize("name,s,cones", ccc.table_cases(), ids=[c[0] for c in ccc.table_cases()])
def test_hand_written_cone_tables(name, s, cones):
    got = ccr.cluster_cones(s["meshes"], s["vertices"], s["indices"])
    assert np.array_equal(_bits(got), _bits(cones)), (name, got, cones)


def test_flat_cone_is_the_margin_alone():
    assert ccc.K_FLAT == ccr.K_MARGIN == F(2.0 ** -7) and ccr.R_MARGIN == F(2.0 ** -7)
    assert ccc.R_FLAT == F(0.7126310467720032)          # sqrtf(0.5f) (1 + 2^-7), rounded twice


def test_shuffled_levels_and_the_known_counts_of_config_3():
    """Clusters with a cone under the four layouts of config 3's geometry: a shuffled level's clusters span the mesh, a strip
    runs around the torus's small circle; only patches bound their normals."""
    from renderer_amd import scene

    s = scene.make_scene(3, n=257)
    counts = {}
    for ordering in ("rows", "strips", "shuffled", "patches"):
        vertices, indices = scene.make_geometry(s["meshes"], ordering)
        cones = ccr.cluster_cones(s["meshes"], vertices, indices)
        counts[ordering] = int(np.isfinite(cones[:, 3]).sum())
        assert len(cones) == 5771
        none = ~np.isfinite(cones[:, 3])
        assert np.array_equal(_bits(cones[none]), _bits(np.tile(ccc.NO_CONE, (int(none.sum()), 1))))
    assert counts == {"rows": 21, "strips": 99, "shuffled": 12, "patches": 4107}, counts


# ---- the hand-written lists ----

@pytest.mark.parametrize("clusters", [1, 2, 3, 63, 64, 65])
@pytest.mark.parametrize("facing", [1.0, -1.0])
def test_two_sided_sheet_ladders(clusters, facing):
    pattern = ("10" * 33)[:clusters]
    s, want = ccc.sheet_scene([pattern, pattern[1:] + "1"], [0, 1, 0], facing=facing, base=11)
    cones = ccr.cluster_cones(s["meshes"], s["vertices"], s["indices"])
    assert np.array_equal(_bits(cones), _bits(ccc.sheet_cones([pattern, pattern[1:] + "1"])))
    boxes = cr.cluster_boxes(s["meshes"], s["vertices"], s["indices"])
    got = ccr.cull_clusters_cone(s, boxes, cones, ccc.EYE, facing, s["bitmap"], lr.DISTANCE, cc.PIN, 1 << 20, first_instance_base=11)
    assert got["status"] == 0 and got["cmds"].tobytes() == want["cmds"].tobytes(), (clusters, facing)
    assert got["stats"].tolist() == want["stats"].tolist()
    # the plain call draws every cluster: the frustum removes none of them
    plain = cr.cull_clusters(s, boxes, s["bitmap"], lr.DISTANCE, cc.PIN, 1 << 20, first_instance_base=11)
    assert int(plain["stats"][1]) == int(plain["stats"][2]) == 3 * clusters


def _sphere_run(eye, facing, instances=(((0, 0, 0), 1.0),)):
    s = ccc.sphere_scene(list(instances))
    boxes = cr.cluster_boxes(s["meshes"], s["vertices"], s["indices"])
    cones = ccr.cluster_cones(s["meshes"], s["vertices"], s["indices"], boxes)
    got = ccr.cull_clusters_cone(s, boxes, cones, eye, facing, s["bitmap"], lr.DISTANCE, cc.PIN, 1 << 20)
    return s, cones, got


def test_sphere_patches():
    s, cones, got = _sphere_run(np.zeros(3, F), 1.0)
    assert len(cones) == 64 and np.isfinite(cones[:, 3]).all()
    # the eye at the centre: every outward triangle is back-facing for facing +1, none for -1
    assert got["stats"].tolist() == [0, 0, 64, 1] and got["cone_culled"].all()
    s, cones, got = _sphere_run(np.zeros(3, F), -1.0)
    assert got["stats"].tolist() == [1, 64, 64, 1] and not got["cone_culled"].any()
    # the eye outside, three radii away: the far side goes — less than half, the cone is conservative
    s, cones, got = _sphere_run(np.array([6, 0, 0], F), 1.0)
    culled = int(got["cone_culled"].sum())
    assert 16 <= culled <= 32, culled
    s, cones, other = _sphere_run(np.array([6, 0, 0], F), -1.0)
    assert not (got["cone_culled"] & other["cone_culled"]).any()     # no cluster is back-facing for both windings
    assert 8 <= int(other["cone_culled"].sum()) <= 32


# ---- the two properties ----

def _properties(s, vertices, indices, eye, facing, pv, bitmap, mode=lr.DISTANCE, sw=None):
    boxes = cr.cluster_boxes(s["meshes"], vertices, indices)
    cones = ccr.cluster_cones(s["meshes"], vertices, indices, boxes)
    got = ccr.cull_clusters_cone(s, boxes, cones, eye, facing, bitmap, mode, lr.PIN_SWITCH_SQ if sw is None else sw, 1 << 30)
    a, b, checked = ccr.property_violations(s, got["items"], got["cone_culled"], vertices, indices, eye, facing, pv)
    return a, b, checked, got, cones


def test_property_a_conservative_in_float64_and_b_agreement_with_the_stage():
    from renderer_amd import scene

    pv = scene.default_pv()
    status, eye, facing = ccr.cone_from_pv(pv)
    assert status == 0 and facing == 1.0
    s = scene.make_scene(3, n=257)
    bitmap = orr.bitmap_of(~nr.run(s)["coarse_culled"])
    # config 3, strips: (a) and (b); the known answer under the pin policy
    vertices, indices = scene.make_geometry(s["meshes"], "strips")
    a, b, checked, got, cones = _properties(s, vertices, indices, eye, facing, pv, bitmap)
    assert (a, b, checked) == (0, 0, 3)
    assert int(np.isfinite(cones[:, 3]).sum()) == 99 and got["stats"].tolist() == [71, 2578, 3127, 72]
    assert ccr.in_domain(s, got["items"], cones, vertices, indices)
    # config 3, patches: (a) with both windings and with the eye at a light; (b) is NOT a property of this scene — its
    # stretched torus has slivers whose float determinant keeps a mathematically back-facing triangle
    vertices, indices = scene.make_geometry(s["meshes"], "patches")
    a, b, checked, got, cones = _properties(s, vertices, indices, eye, 1.0, None, bitmap)
    assert (a, checked) == (0, 731), (a, checked, got["stats"].tolist())
    assert got["stats"].tolist() == [266, 1971, 3127, 72]
    assert ccr.in_domain(s, got["items"], cones, vertices, indices)
    a, b, checked, got, cones = _properties(s, vertices, indices, eye, -1.0, None, bitmap)
    assert a == 0 and checked > 600
    a, b, checked, got, cones = _properties(s, vertices, indices, np.array([30.0, 40.0, -20.0], F), 1.0, None, bitmap)
    assert a == 0 and checked > 300
    # the sphere and the sheet: (a) and (b) under a projection of their own eye
    for scene_eye in (np.array([6, 0, 0], F), np.array([0.5, 7, 1], F)):
        own_pv = pv.copy().reshape(4, 4)
        own_pv[3] = (pv.reshape(4, 4)[:3] * -(scene_eye - eye)[:, None]).sum(axis=0) + pv.reshape(4, 4)[3]   # pv x translate(eye - scene_eye)
        own_pv = own_pv.reshape(16)
        status, e2, f2 = ccr.cone_from_pv(own_pv)
        assert status == 0 and f2 == 1.0 and np.allclose(e2, scene_eye, atol=1e-5)
        sp = ccc.sphere_scene([((0, 0, 0), 1.0), ((1, 2, -3), 0.5)])
        a, b, checked, got, cones = _properties(sp, sp["vertices"], sp["indices"], e2, f2, own_pv, sp["bitmap"], sw=cc.PIN)
        assert (a, b) == (0, 0) and checked >= 30
    own_pv = pv.copy().reshape(4, 4)
    own_pv[3] = (pv.reshape(4, 4)[:3] * -(ccc.EYE - eye)[:, None]).sum(axis=0) + pv.reshape(4, 4)[3]
    status, e2, f2 = ccr.cone_from_pv(own_pv.reshape(16))
    sh, _ = ccc.sheet_scene(["10" * 32 + "1"], [0, 0])
    a, b, checked, got, cones = _properties(sh, sh["vertices"], sh["indices"], e2, f2, own_pv.reshape(16), sh["bitmap"], sw=cc.PIN)
    assert (a, b, checked) == (0, 0, 64)


def test_the_stream_of_the_cone_call_is_the_plain_call_s_on_a_property_b_scene():
    """Where (b) holds, the cone removes only triangles the per-triangle test removes: the same index stream, fewer tested."""
    from renderer_amd import scene

    pv = scene.default_pv()
    _, eye, facing = ccr.cone_from_pv(pv)
    s = scene.make_scene(3, n=257)
    bitmap = orr.bitmap_of(~nr.run(s)["coarse_culled"])
    vertices, indices = scene.make_geometry(s["meshes"], "strips")
    boxes = cr.cluster_boxes(s["meshes"], vertices, indices)
    cones = ccr.cluster_cones(s["meshes"], vertices, indices, boxes)
    plain = ctr.cull_cluster_triangles(s, boxes, vertices, indices, bitmap, lr.DISTANCE, lr.PIN_SWITCH_SQ, pv, 1 << 20, 1 << 31)
    cone = ccr.cull_cluster_triangles_cone(s, boxes, cones, eye, facing, vertices, indices, bitmap, lr.DISTANCE, lr.PIN_SWITCH_SQ, pv, 1 << 20, 1 << 31)
    assert np.array_equal(plain["stream"], cone["stream"]) and plain["stats"][4] == cone["stats"][4]
    assert int(cone["stats"][5]) < int(plain["stats"][5])
    assert plain["stats"].tolist() == [71, 2581, 3127, 72, 78898, 162813] and cone["stats"].tolist()[:4] == [71, 2578, 3127, 72]


# ---- the view ----

def _lib():
    import renderer_amd
    return renderer_amd.load_library()


def _from_pv(pv):
    from renderer_amd import _lib as L

    c = L.MipClusterCone()
    m = np.ascontiguousarray(pv, F)
    rc = _lib().mip_cone_from_pv(m.ctypes.data, C.addressof(c))
    return rc, np.array(list(c.eye), F), float(c.facing), c


def test_cone_from_pv():
    from renderer_amd import scene
    from renderer_amd.pipeline import make_cluster_cone
    import renderer_amd

    pv = scene.default_pv()
    rc, eye, facing, c = _from_pv(pv)
    assert rc == 0 and facing == 1.0 and c.struct_size == 24 and c.flags == 0
    assert np.array_equal(eye, np.asarray(scene.DEFAULT_CAMERA["cam_pos"], F))           # the eye is the camera
    want = ccr.cone_from_pv(pv)
    assert want[0] == 0 and np.array_equal(_bits(want[1]), _bits(eye)) and want[2] == facing
    flip = pv.copy().reshape(4, 4)
    flip[:, 1] *= -1                                    # row y of the column-major matrix
    rc, eye2, facing2, _ = _from_pv(flip.reshape(16))
    assert rc == 0 and facing2 == -1.0 and np.array_equal(eye2, eye)
    mirror = flip.copy()
    mirror[:, 0] *= -1                                  # and row x: two flips
    rc, eye3, facing3, _ = _from_pv(mirror.reshape(16))
    assert rc == 0 and facing3 == 1.0 and np.array_equal(eye3, eye)
    ortho = np.eye(4, dtype=F)
    ortho[0, 0], ortho[1, 1], ortho[3, 2] = 0.1, 0.2, -0.3
    assert _from_pv(ortho.reshape(16))[0] == -1 and ccr.cone_from_pv(ortho.reshape(16))[0] == -1
    for bad in (np.nan, np.inf):
        broken = pv.copy()
        broken[0] = bad
        assert _from_pv(broken)[0] == -1 and ccr.cone_from_pv(broken)[0] == -1
    assert _lib().mip_cone_from_pv(None, None) == -1 and _lib().mip_cone_from_pv(pv.ctypes.data, None) == -1
    # the Python side
    c = make_cluster_cone(pv)
    assert list(c.eye) == list(eye) and c.facing == 1.0
    c = make_cluster_cone(pv, eye=(1, 2, 3), facing=-1)
    assert list(c.eye) == [1.0, 2.0, 3.0] and c.facing == -1.0
    c = make_cluster_cone(eye=(4, 5, 6), facing=1)
    assert list(c.eye) == [4.0, 5.0, 6.0] and c.struct_size == 24
    with pytest.raises(renderer_amd.MipError):
        make_cluster_cone(ortho.reshape(16))
    with pytest.raises(ValueError):
        make_cluster_cone(eye=(1, 2, 3))


# ---- the ABI ----

def test_struct_sizes_in_c_ctypes_and_rust(tmp_path):
    from renderer_amd import _lib as L

    assert C.sizeof(L.MipClusterCone) == 24 and L.MipClusterCone.eye.offset == 8 and L.MipClusterCone.facing.offset == 20
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "mi_instance_pipeline.h"
    int main(void) { printf("%zu %zu %zu\n", sizeof(MipClusterCone), offsetof(MipClusterCone, eye), offsetof(MipClusterCone, facing)); return 0; }'''
    c = tmp_path / "t.c"
    c.write_text(src)
    exe = str(tmp_path / "t")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe])
    assert [int(x) for x in subprocess.check_output([exe]).split()] == [24, 8, 20]
    rust = open(os.path.join(ROOT, "integration", "rust", "mip-sys", "src", "lib.rs")).read()
    body = re.search(r"pub struct MipClusterCone \{(.*?)\}", rust, flags=re.S).group(1)
    assert re.findall(r"pub (\w+): ([^,]+),", body) == [("struct_size", "u32"), ("flags", "u32"), ("eye", "[f32; 3]"), ("facing", "f32")]
    assert "#[repr(C)]" in rust[: rust.index("pub struct MipClusterCone")].rsplit("\n\n", 1)[-1]


def test_header_exports_and_declarations_agree():
    from renderer_amd import _lib as L

    names = ["mip_build_cluster_cones", "mip_read_cluster_cones", "mip_cone_from_pv", "mip_cull_clusters_cone", "mip_cull_cluster_triangles_cone"]
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mi_instance_pipeline.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "integration", "rust", "mip-sys", "src", "lib.rs")).read()
    lib = _lib()
    for name in names:
        assert name in L.EXPORTS and hasattr(lib, name)
        c_args = re.search(name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S).group(1).count(",") + 1
        assert len(getattr(lib, name).argtypes) == c_args, name
        r_args = re.search(r"pub fn " + name + r"\((.*?)\)\s*->", rust, flags=re.S).group(1).count(",") + 1
        assert r_args == c_args, name
    # the cone sits in front of `out`, as the header says
    assert re.search(r"mip_cull_clusters_cone\([^;]*const MipClusterCone\* cone, const MipClusterOutputs\* out\)", header)
    assert re.search(r"mip_cull_cluster_triangles_cone\([^;]*const MipClusterCone\* cone, const MipClusterTriangleOutputs\* out\)", header)
    # without a context every entry point is a status code
    assert lib.mip_build_cluster_cones(None) == -1 and lib.mip_read_cluster_cones(None, None, 0) == -1
    assert lib.mip_cull_clusters_cone(None, None, None, None, None, None, None) == -1
    assert lib.mip_cull_cluster_triangles_cone(None, None, None, None, None, None, None) == -1
    # the cone left the header's OUT OF SCOPE lists
    text = open(os.path.join(ROOT, "include", "mi_instance_pipeline.h")).read()
    for m in re.finditer(r"OUT OF SCOPE:[^/]*?\*/", text, flags=re.S):
        assert "normal-cone back-face test (" not in m.group(0)


def test_cone_plan_over_its_decision_edges(tmp_path):
    exe = str(tmp_path / "cluster_cone_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "native", "cluster_cone_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    last = out.stdout.strip().split("\n")[-1]
    assert last.startswith("CLUSTER CONE PLAN OK") and int(last.split()[4]) > 150, out.stdout[-2000:]


def test_the_matrix_of_cone_culled_is_the_one_mip_run_writes():
    """rotation_times_scale against numpy_restatement.model_matrices on finite instances: the same nine floats."""
    from renderer_amd import scene

    s = scene.make_scene(3, n=1025)
    model = nr.model_matrices(s["pos"], s["rot"], s["scale"]).reshape(-1, 4, 4)     # [n][col][row]
    m = ccr.rotation_times_scale(s["rot"], s["scale"])                               # [n][row][col]
    assert np.array_equal(_bits(model[:, :3, :3].transpose(0, 2, 1)), _bits(m))
