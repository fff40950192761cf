"""Random scene generator for the fuzz tests: arbitrary cameras (planes from the oracle's
project_camera), mesh tables with empty LODs, special floating-point values sprinkled over every
input column, random shard bases."""
import numpy as np

from renderer_amd.pipeline import MESH_DTYPE

SPECIAL = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1e-38, 3.4e38, -3.4e38, 1e19, -1e19,
                    1e-20, 0.5, 2.0, 10.0, 100.0, 16777216.0], dtype=np.float32)


def random_scene(rng, oracle, n_max=5000, special_rate=0.02):
    n = int(rng.integers(0, n_max + 1))
    m = int(rng.integers(1, 40))
    meshes = np.zeros(m, MESH_DTYPE)
    centre = rng.uniform(-1, 1, (m, 3))
    half = rng.uniform(0.01, 3, (m, 3))
    meshes["aabb_min"] = (centre - half).astype(np.float32)
    meshes["aabb_max"] = (centre + half).astype(np.float32)
    meshes["n_lods"] = rng.integers(1, 7, m)
    meshes["index_len"] = rng.integers(0, 70000, (m, 6)) // 3 * 3
    meshes["index_len"][rng.random((m, 6)) < 0.1] = 0          # empty LODs: dropped by compaction
    meshes["index_offset"] = rng.integers(0, 2 ** 31, (m, 6))
    meshes["vertex_offset"] = rng.integers(-1000, 2 ** 30, m)
    spread = float(rng.choice([5.0, 40.0, 200.0]))
    pos = rng.normal(0, spread, (n, 3)).astype(np.float32)
    rot = rng.normal(0, 1, (n, 4)).astype(np.float32)
    if rng.random() < 0.7:
        rot /= np.maximum(np.linalg.norm(rot, axis=1, keepdims=True), 1e-6).astype(np.float32)   # mostly unit quaternions
    scale = rng.uniform(-1, 3, n).astype(np.float32)
    mesh_id = rng.integers(0, m, n).astype(np.uint32)
    for arr in (pos, rot):
        hit = rng.random(arr.shape) < special_rate
        arr[hit] = rng.choice(SPECIAL, int(hit.sum()))
    hit = rng.random(n) < special_rate
    scale[hit] = rng.choice(SPECIAL, int(hit.sum()))
    cam_pos = rng.normal(0, 10, 3).astype(np.float32)
    q = rng.normal(0, 1, 4)
    q /= np.linalg.norm(q)
    camera = (float(rng.uniform(0.5, 3)), float(rng.uniform(20, 120)), float(rng.uniform(0.01, 1)), float(rng.uniform(10, 1000)))
    planes = oracle.project_camera(cam_pos, q.astype(np.float32), aspect=camera[0], fovy_degrees=camera[1], near=camera[2], far=camera[3])
    if rng.random() < 0.2:   # degenerate planes too: zeros, NaN, huge
        planes[rng.integers(0, 24, 3)] = rng.choice(SPECIAL, 3)
    return dict(n=n, pos=pos, rot=rot, scale=scale, mesh_id=mesh_id, meshes=meshes, planes=planes, cam_pos=cam_pos,
                first_instance_base=int(rng.integers(0, 2 ** 32)), first_index_base=int(rng.integers(0, 2 ** 32)),
                camera=dict(cam_pos=cam_pos.astype(np.float64), cam_rot_ijkw=q, aspect=camera[0], fovy_degrees=camera[1], near=camera[2], far=camera[3]))


def camera_pv64(cam_pos, cam_rot_ijkw, aspect, fovy_degrees, near, far):
    """projection * view of a camera, float32[16] column-major, computed in float64 and rounded once — the construction
    of scene.default_pv() for any camera (glm::perspective_lh_zo x glm::look_at_lh along the rotated +z, up the rotated +y)."""
    i, j, k, w = np.asarray(cam_rot_ijkw, np.float64) / np.linalg.norm(cam_rot_ijkw)
    R = np.array([[1 - 2 * (j * j + k * k), 2 * (i * j - w * k), 2 * (w * j + i * k)],
                  [2 * (w * k + i * j), 1 - 2 * (i * i + k * k), 2 * (j * k - w * i)],
                  [2 * (i * k - w * j), 2 * (w * i + j * k), 1 - 2 * (i * i + j * j)]])
    z, up = R[:, 2], R[:, 1]
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    view = np.eye(4)
    view[:3, :3] = np.stack([x, y, z])
    view[:3, 3] = -view[:3, :3] @ np.asarray(cam_pos, np.float64)
    t = np.tan(np.radians(fovy_degrees) / 2.0)
    proj = np.zeros((4, 4))
    proj[0, 0] = 1.0 / (aspect * t)
    proj[1, 1] = 1.0 / t
    proj[2, 2] = far / (far - near)
    proj[2, 3] = -(far * near) / (far - near)
    proj[3, 2] = 1.0
    return (proj @ view).T.astype(np.float32).reshape(16)


def random_geometry(rng, s):
    """Geometry for the per-triangle stage over a random scene (its own generator: the scene's stream is not disturbed):
    the scene's mesh table with index ranges and vertex offsets that a small consolidated buffer backs — index counts that
    are no multiple of 3 and of 1 or 2, empty LODs, ranges that start at no multiple of 3, vertex offsets below the mesh's first vertex, random
    triangles (any winding, any size against the box), special values among the positions of some scenes — and the
    camera's pv. Returns dict(meshes, vertices, indices, pv)."""
    meshes = s["meshes"].copy()
    m = len(meshes)
    n_idx = 0
    v_chunks = []
    i_chunks = []
    n_vtx = 0
    for k in range(m):
        vc = int(rng.integers(3, 60))
        lo, hi = meshes["aabb_min"][k].astype(np.float64), meshes["aabb_max"][k].astype(np.float64)
        v_chunks.append((lo + rng.random((vc, 3)) * (hi - lo)).astype(np.float32))
        shift = int(rng.integers(0, 8)) if n_vtx >= 8 else 0      # vertexOffset below the mesh's first vertex, indices shifted up
        meshes["vertex_offset"][k] = n_vtx - shift
        for lod in range(6):
            length = int(rng.integers(0, 400))
            if rng.random() < 0.1:
                length = int(rng.integers(0, 3))
            # indexOffset / 3 rounds down: a range that starts at no multiple of 3 is read from up to two indices earlier.
            # Those are filler indices of this mesh's own first vertex, so every index the stage can read names a vertex
            # of the buffer.
            gap = 2 + int(rng.integers(0, 3))
            i_chunks.append(np.full(gap, shift, np.uint32))
            n_idx += gap
            meshes["index_offset"][k][lod] = n_idx
            meshes["index_len"][k][lod] = length
            n_idx += length
            i_chunks.append((rng.integers(0, vc, length) + shift).astype(np.uint32))
        n_vtx += vc
    vertices = np.concatenate(v_chunks)
    if rng.random() < 0.3:
        hit = rng.random(vertices.shape) < 0.01
        vertices[hit] = rng.choice(SPECIAL, int(hit.sum()))
    return dict(meshes=meshes, vertices=vertices, indices=np.concatenate(i_chunks), pv=camera_pv64(**s["camera"]))
