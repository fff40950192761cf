#!/usr/bin/env python3
"""occlusion_bench.py — the occlusion-culling extension's timings (include/mi_instance_pipeline.h, MipOcclusion).

  python tools/occlusion_bench.py [--samples S] [--steps K] [--out FILE]

The context launches on torch's current stream, so that HIP events recorded there bracket its launches (as bench.py
does). Every leg: K back-to-back launches per sample, median over S samples of a sample's time / K.

  pyramid_1080p_u16_us     mip_build_depth_pyramid, 1920 x 1080 D16_UNORM
  pyramid_2160p_f32_us     mip_build_depth_pyramid, 3840 x 2160 D32_SFLOAT
  run_1m_us                mip_run, BASELINE config 3 (mixed scene, 1 M instances), model + bitmap + commands
  run_occluded_1m_us       mip_run_occluded, same scene and outputs, + the occluded bitmap, against a 1080p pyramid of
                           random 24-pixel blocks of depth (view distances 8 .. 40, 5 % of the blocks cleared)
  occluded_over_run        run_occluded_1m_us / run_1m_us

Prints one JSON line (with the source hash of the kernels it measured); --out appends it to FILE.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def source_hash():
    h = hashlib.sha256()
    for f in ("occlusion_kernel.hpp", "api_occlusion.hip", "instance_kernel.hpp", "api_frame.hip"):
        h.update(open(os.path.join(ROOT, "renderer_amd", "csrc", f), "rb").read())
    return h.hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import renderer_amd
    from renderer_amd import _lib, scene
    from renderer_amd.pipeline import depth_pyramid_layout, make_frame, make_occlusion
    from test_gpu_occlusion import _block_depth

    dev = torch.device("cuda", 0)
    ts = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(ts)

    def timed(fn):
        for _ in range(args.steps * 3):
            fn()
        ts.synchronize()
        per = []
        for _ in range(args.samples):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ts)
            for _ in range(args.steps):
                fn()
            e1.record(ts)
            e1.synchronize()
            per.append(e0.elapsed_time(e1) * 1000.0 / args.steps)
        return float(np.median(per))

    s = scene.make_scene(3)
    n = s["n"]
    res = {"metric": "occlusion extension timings (us per launch, median)", "source_hash": source_hash(), "n": n}
    with renderer_amd.InstancePipeline(max_instances=n, max_meshes=len(s["meshes"]), stream=ts.cuda_stream) as p:
        p.set_mesh_table(s["meshes"])
        p.set_instances(s["pos"], s["rot"], s["scale"], s["mesh_id"])
        rng = np.random.default_rng(1)
        pyramids = {}
        for name, (w, h, u16) in {"pyramid_1080p_u16_us": (1920, 1080, True), "pyramid_2160p_f32_us": (3840, 2160, False)}.items():
            depth = _block_depth(rng, w, h, 24, u16=u16)
            dt = torch.from_numpy(depth.view(np.int16) if u16 else depth).to(dev)
            pyr = torch.zeros(depth_pyramid_layout(w, h)["bytes"] // 4, dtype=torch.float32, device=dev)
            fmt = _lib.MIP_DEPTH_UNORM16 if u16 else _lib.MIP_DEPTH_FLOAT32
            ts.synchronize()
            res[name] = timed(lambda: p.build_depth_pyramid(dt.data_ptr(), w, h, pyr.data_ptr(), format=fmt, async_=True))
            pyramids[name] = (pyr, dt, w, h)
        pyr, _, w, h = pyramids["pyramid_1080p_u16_us"]
        model = torch.zeros((n, 16), dtype=torch.float32, device=dev)
        bitmap = torch.zeros((n + 31) // 32, dtype=torch.int32, device=dev)
        occ_bitmap = torch.zeros((n + 31) // 32, dtype=torch.int32, device=dev)
        cmds = torch.zeros((n, 5), dtype=torch.int32, device=dev)
        scal = torch.zeros(8, dtype=torch.int32, device=dev)
        ts.synchronize()
        out = p.prepare_outputs(model=model.data_ptr(), visible_bitmap=bitmap.data_ptr(), draw_cmds=cmds.data_ptr(),
                                draw_count=scal.data_ptr(), draw_index_total=scal.data_ptr() + 4)
        frame = p.frame_ref(make_frame(s["planes"], s["cam_pos"]))
        o = make_occlusion(w, h, pyr.data_ptr(), scene.default_pv(), occluded_bitmap=occ_bitmap.data_ptr())
        res["run_1m_us"] = timed(lambda: p.run_prepared(frame, out))
        res["run_occluded_1m_us"] = timed(lambda: p.run_occluded(frame, o, out))
        p.wait()
        vis = int(np.unpackbits(bitmap.cpu().numpy().view(np.uint8)).sum())
        occd = int(np.unpackbits(occ_bitmap.cpu().numpy().view(np.uint8)).sum())
        res["occluded_over_run"] = res["run_occluded_1m_us"] / res["run_1m_us"]
        res["drawn"] = vis
        res["occluded"] = occd
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
