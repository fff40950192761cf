#!/usr/bin/env python3
"""Generates tests/golden/*.npz from the C oracle (TEST INFRASTRUCTURE).

The reference has no tests, fixtures or golden vectors for this path and cannot be built
or run here (nightly Rust, un-vendored crates), so these vectors are produced by the
oracle itself: they pin the oracle against regressions / toolchain differences and give the
GPU tests committed expected outputs, but they are NOT outputs of the reference (parity
unpinned — see oracle/mip_oracle.h).

    python oracle/gen_golden.py          # rewrites tests/golden/
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import oracle  # noqa: E402
from renderer_amd import scene  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def special_scene(n=513):
    """Hand-built edge cases followed by random filler."""
    s = scene.make_scene(3, n=n, all_visible=True)
    pos, rot, scl, mid = s["pos"], s["rot"], s["scale"], s["mesh_id"]
    m = s["meshes"]
    m["index_len"][5, 0] = 0  # a mesh whose LOD0 is empty: dropped by compaction when near
    r = np.float32(np.sqrt(0.5))
    cases = [
        # pos, rot[i,j,k,w], scale, mesh
        ((1, 2, 30), (0, 0, 0, 1), 1.0, 0),                 # identity: M = T
        ((0, 1, 40), (0, r, 0, r), 2.0, 1),                 # 90 degrees about +Y, scale 2
        ((30, 20, -40.1), (0, 0, 0, 1), 1.0, 2),            # a reference light position (main.rs:369)
        ((0.1, 17, 0.1), (0, 0, 0, 1), 1.0, 3),             # the other one (main.rs:378)
        ((0, 1, 50), (0, 0, 0, 1), 0.0, 4),                 # zero scale
        ((0, 1, 50), (0, 0, 0, 2), 1.0, 4),                 # non-unit quaternion (not renormalised)
        ((np.nan, 1, 50), (0, 0, 0, 1), 1.0, 4),            # NaN position => visible
        ((0, 1, 50), (np.inf, 0, 0, 1), 1.0, 4),            # inf in the quaternion
        ((0, 1, 50), (0, 0, 0, 1), np.inf, 4),              # inf scale
        ((0, 1, 50), (0, 0, 0, 1), np.nan, 4),              # NaN scale
        ((np.inf, 1, 50), (0, 0, 0, 1), 1.0, 4),            # inf position
        ((0, 1, 5), (0, 0, 0, 1), 1.0, 5),                  # near (LOD 0) with an empty LOD 0 => no command
        ((0, 1, 12), (0, 0, 0, 1), 1.0, 0),                 # distance exactly 10 from the camera => LOD 0
        ((0, 1, np.nextafter(np.float32(12), np.float32(13))), (0, 0, 0, 1), 1.0, 0),  # just beyond => LOD 1
        ((0, 1, -50), (0, 0, 0, 1), 1.0, 0),                # behind the camera: culled
        ((0, 1, 1e-42), (1e-20, 1e-20, 0, 1), 1e-38, 0),    # denormals
    ]
    for k, (p, q, sc, me) in enumerate(cases):
        pos[k] = p
        rot[k] = q
        scl[k] = sc
        mid[k] = me
    return s


def dump(name, s, **extra):
    r = oracle.run(s["pos"], s["rot"], s["scale"], s["mesh_id"], s["meshes"], s["planes"], s["cam_pos"], **extra)
    np.savez_compressed(
        os.path.join(OUT, name + ".npz"),
        pos=s["pos"], rot=s["rot"], scale=s["scale"], mesh_id=s["mesh_id"], meshes=s["meshes"],
        planes=s["planes"], cam_pos=s["cam_pos"],
        first_instance_base=np.uint32(extra.get("first_instance_base", 0)),
        first_index_base=np.uint32(extra.get("first_index_base", 0)),
        model=r["model"], world_aabb=r["world_aabb"], visible_bitmap=r["visible_bitmap"],
        coarse_culled=r["coarse_culled"], draw_cmds=r["draw_cmds"],
        draw_count=np.uint32(r["draw_count"]), draw_index_total=np.uint32(r["draw_index_total"]),
    )
    print(f"{name}: n={s['n']} visible={int((1 - r['coarse_culled']).sum())} cmds={r['draw_count']}")


def dump_skinned(name, s):
    """Extension fixtures (tests/golden/ext/): the skinned frame, inputs + oracle outputs."""
    sk = s["skeleton"]
    r = oracle.run_skinned(s["pos"], s["rot"], s["scale"], s["mesh_id"], s["meshes"], sk, s["poses"], s["planes"], s["cam_pos"])
    np.savez_compressed(
        os.path.join(OUT, "ext", name + ".npz"),
        pos=s["pos"], rot=s["rot"], scale=s["scale"], mesh_id=s["mesh_id"], meshes=s["meshes"], planes=s["planes"], cam_pos=s["cam_pos"],
        parent=sk["parent"], inverse_bind=sk["inverse_bind"], joint_box=sk["joint_box"], poses=s["poses"],
        palette=r["palette"], local_box=r["local_box"], model=r["model"], world_aabb=r["world_aabb"],
        visible_bitmap=r["visible_bitmap"], draw_cmds=r["draw_cmds"], draw_count=np.uint32(r["draw_count"]),
        draw_index_total=np.uint32(r["draw_index_total"]),
    )
    print(f"ext/{name}: n={s['n']} cmds={r['draw_count']}")


def dump_lights(name, s, lights, first_instance_base):
    """Extension fixtures: the shadow pass's per-light draw lists (row f-4)."""
    lists = oracle.light_draw_lists(s["pos"], s["mesh_id"], s["meshes"], lights, first_instance_base=first_instance_base)
    np.savez_compressed(os.path.join(OUT, "ext", name + ".npz"), pos=s["pos"], rot=s["rot"], scale=s["scale"], mesh_id=s["mesh_id"],
                        meshes=s["meshes"], lights=lights, first_instance_base=np.uint32(first_instance_base), lists=lists)
    print(f"ext/{name}: n={s['n']} lights={len(lights)}")


def dump_wire(name, golden_name):
    """Extension fixture: the WIRE form (include/mi_instance_pipeline.h, MIP_OUT_WIRE) of a committed golden frame's draw
    list, from the numpy statement of the format in tests/cpu_pipeline.py — pins the byte layout the kernels speak."""
    sys.path.insert(0, os.path.join(os.path.dirname(OUT)))
    from cpu_pipeline import encode_wire, encode_wire_packed

    g = np.load(os.path.join(OUT, golden_name + ".npz"))
    cmds = g["draw_cmds"]
    inst = (cmds["firstInstance"] - np.uint32(g["first_instance_base"])).astype(np.int64)
    far = np.array([oracle.pick_lod(2, g["cam_pos"], g["pos"][i]) for i in inst], np.uint32)
    body = encode_wire(cmds, g["mesh_id"][inst], far)
    body_packed = encode_wire_packed(cmds, g["mesh_id"][inst], far, g["first_instance_base"], len(g["meshes"]))  # MIP_OUT_WIRE_PACKED
    np.savez_compressed(os.path.join(OUT, "ext", name + ".npz"), source=np.array(golden_name), body=body, body_packed=body_packed,
                        draw_count=np.uint32(len(cmds)), draw_index_total=g["draw_index_total"])
    print(f"ext/{name}: {len(cmds)} commands -> {body.nbytes} wire bytes ({body.nbytes / max(len(cmds), 1):.2f} B per command)")


def dump_triangles(name, s, vertices, indices, pv, first_instance_base=0, first_index_base=0):
    """Extension fixtures for row f-1 (the per-triangle stage): the frame's inputs with geometry and pv, the frame's command
    list, the source index offsets, and the oracle's final commands and WHOLE culled stream (untouched slots = 0xFFFFFFFF)."""
    r = oracle.run(s["pos"], s["rot"], s["scale"], s["mesh_id"], s["meshes"], s["planes"], s["cam_pos"],
                   first_instance_base=first_instance_base, first_index_base=first_index_base)
    capacity = first_index_base + r["draw_index_total"] + 3
    final, stream, src = oracle.cull_all_triangles(r, s["pos"], s["mesh_id"], s["meshes"], s["cam_pos"], pv, vertices, indices,
                                                   first_instance_base=first_instance_base, out_capacity=capacity, threads=1)
    path = os.path.join(OUT, "ext", name + ".npz")
    np.savez_compressed(
        path, pos=s["pos"], rot=s["rot"], scale=s["scale"], mesh_id=s["mesh_id"], meshes=s["meshes"], planes=s["planes"], cam_pos=s["cam_pos"],
        pv=np.asarray(pv, np.float32), first_instance_base=np.uint32(first_instance_base), first_index_base=np.uint32(first_index_base),
        vertices=np.asarray(vertices, np.float32), indices=np.asarray(indices, np.uint32),
        draw_cmds=r["draw_cmds"], draw_count=np.uint32(r["draw_count"]), draw_index_total=np.uint32(r["draw_index_total"]),
        src_index_offset=src, final_cmds=final, final_count=np.uint32(len(final)), culled_stream=stream,
    )
    print(f"ext/{name}: n={s['n']} cmds={r['draw_count']} -> {len(final)}, indices {int(r['draw_cmds']['indexCount'].sum())} -> "
          f"{int(final['indexCount'].sum())}, {os.path.getsize(path)} bytes")


def small_mesh_table(m=8, max_len0=600):
    """The first m meshes of the mixed table with their LOD chains rebuilt from at most max_len0 indices and the offsets
    repacked: the same boxes and LOD structure over geometry of a few thousand indices."""
    t = scene.mixed_mesh_table()[:m].copy()
    index_off = vertex_off = 0
    for k in range(m):
        len0 = min(int(t["index_len"][k, 0]), max_len0 - 30 * k) // 3 * 3
        lens = scene._lod_chain(len0)[: int(t["n_lods"][k])]
        t["n_lods"][k] = len(lens)
        t["index_len"][k] = 0
        t["index_offset"][k] = 0
        for j, l in enumerate(lens):
            t["index_len"][k, j] = l
            t["index_offset"][k, j] = index_off
            index_off += l
        t["vertex_offset"][k] = vertex_off
        vertex_off += max(len0 // 3, 9)
    return t


def triangle_scenes():
    """(name, scene, vertices, indices, pv, bases) of the three committed row f-1 fixtures."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import triangle_cases as tc

    pv = scene.default_pv()
    out = []
    # a mixed scene over a reduced mesh table
    s = scene.make_scene(3, n=300)
    s["meshes"] = small_mesh_table()
    s["mesh_id"] = (s["mesh_id"] % len(s["meshes"])).astype(np.uint32)
    out.append(("triangles_mixed_300", s, *scene.make_geometry(s["meshes"]), pv, {}))
    # the known-answer triangles as mesh 0 (identity instance 0, mirrored instance 1) + special instances of a small mesh
    s = scene.make_scene(3, n=24, all_visible=True)
    table = small_mesh_table(2, 300)
    kv, ki = tc.case_mesh(tc.CASES + tc.MIRROR_CASES)
    finite = kv[np.isfinite(kv).all(axis=1)]
    table["aabb_min"][0], table["aabb_max"][0] = finite.min(axis=0), finite.max(axis=0)
    table["n_lods"][0] = 1
    table["index_len"][0], table["index_offset"][0] = 0, 0
    table["index_len"][0, 0] = len(ki)
    alone = table[1:2].copy()                         # mesh 1's torus on its own, then placed behind the case mesh
    n1 = int(alone["n_lods"][0])
    alone["index_offset"][0, :n1] -= alone["index_offset"][0, 0]
    alone["vertex_offset"][0] = 0
    gv, gi = scene.make_geometry(alone)
    table["vertex_offset"][1] = len(kv)
    table["index_offset"][1, :n1] = alone["index_offset"][0, :n1] + len(ki)
    vertices = np.concatenate([kv, gv])
    indices = np.concatenate([ki, gi])
    s["meshes"] = table
    s["mesh_id"][:] = 1
    s["mesh_id"][:2] = 0
    s["pos"][0], s["rot"][0], s["scale"][0] = (0, 0, 0), (0, 0, 0, 1), 1.0
    s["pos"][1], s["rot"][1], s["scale"][1] = tc.MIRROR_INSTANCE["pos"], tc.MIRROR_INSTANCE["rot"], tc.MIRROR_INSTANCE["scale"]
    s["pos"][5, 0] = np.nan
    s["scale"][7] = 0.0
    s["scale"][9] = -1.0
    s["rot"][11] = (0, 0, 0, 3.0)
    s["scale"][13] = np.inf
    out.append(("triangles_special_24", s, vertices, indices, pv, {}))
    # bases != 0, index counts of 3k+1, 3k+2, 2 and 1
    s = scene.make_scene(3, n=200, all_visible=True)
    s["meshes"] = small_mesh_table()
    s["mesh_id"] = (s["mesh_id"] % len(s["meshes"])).astype(np.uint32)
    vertices, indices = scene.make_geometry(s["meshes"])
    m = s["meshes"]
    for k in range(len(m)):
        for lod in range(int(m["n_lods"][k])):
            if (k + lod) % 3 == 1 and m["index_len"][k][lod] > 4:
                m["index_len"][k][lod] -= 1 + (k % 2)
    m["index_len"][5][: int(m["n_lods"][5])] = 2
    m["index_len"][6][: int(m["n_lods"][6])] = 1
    out.append(("triangles_bases_200", s, vertices, indices, pv, dict(first_instance_base=1000, first_index_base=5)))
    return out


def main():
    os.makedirs(os.path.join(OUT, "ext"), exist_ok=True)
    oracle.build()
    sk_scene = scene.make_skinned_scene(301)
    sk_scene["poses"][7, 3, 0] = np.nan      # a NaN joint translation
    sk_scene["poses"][9, :, 7:10] = 0.0      # zero joint scales
    sk_scene["pos"][11] = np.nan             # NaN instance position
    dump_skinned("skinned_301", sk_scene)
    lit = scene.make_scene(3, n=1001)
    lit["pos"][5] = np.nan
    dump_lights("lights_1001", lit, np.array([[30, 20, -40.1], [0.1, 17, 0.1], [0, 0, 0], lit["pos"][17]], np.float32), 4)
    dump("box_1024", scene.make_scene(1))  # BASELINE config 1, full outputs
    for n in (1, 63, 64, 65, 257):
        dump(f"mixed_{n}", scene.make_scene(3, n=n, all_visible=(n < 100)))
    dump("mixed_4097_bases", scene.make_scene(3, n=4097), first_instance_base=1000, first_index_base=0xFFFFF000)
    dump("helmet_2000", scene.make_scene(2, n=2000))
    dump("special_513", special_scene())
    np.save(os.path.join(OUT, "default_planes.npy"), scene.default_planes())
    dump_wire("wire_4097_bases", "mixed_4097_bases")
    for name, s, vertices, indices, pv, bases in triangle_scenes():
        dump_triangles(name, s, vertices, indices, pv, **bases)


if __name__ == "__main__":
    main()
