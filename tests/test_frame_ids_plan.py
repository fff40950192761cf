"""The width rule of the frame kernel's narrow mesh ids (renderer_amd/csrc/frame_plan.hpp: plan_frame_id_bytes,
plan_frame_id_mode) is a pure function, so it is enumerated on the CPU, under AddressSanitizer + UBSan, in the style of
test_frame_plan.py: every max_meshes up to past the 2-byte rule, every table size at which the mode can change. A wrong width
on the GPU is not a crash, it is another mesh's draw."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_id_width_rule_over_every_capacity(tmp_path):
    exe = str(tmp_path / "frame_ids_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "native", "frame_ids_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    last = out.stdout.strip().split("\n")[-1]
    assert last.startswith("IDS OK"), out.stdout[-2000:]
    assert int(last.split()[2]) > 1_000_000  # the sweep really ran


def test_the_uploads_and_the_launch_take_the_width_from_the_rule():
    """api_context.hip sizes and fills the narrow column by the rule, api_frame.hip picks the kernel's mode by it: neither
    decides a width of its own."""
    ctx = open(os.path.join(ROOT, "renderer_amd", "csrc", "api_context.hip")).read()
    frame = open(os.path.join(ROOT, "renderer_amd", "csrc", "api_frame.hip")).read()
    assert "mip::plan_frame_id_bytes(ctx->max_meshes" in ctx
    assert "mip::plan_frame_id_mode(ctx->m, plan.order == 1 ? ctx->frame_id_bytes : 0u" in frame
