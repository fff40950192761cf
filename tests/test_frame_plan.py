"""plan_frame (renderer_amd/csrc/frame_plan.hpp) — the library's whole per-frame decision table: which instantiation of the
frame kernel, which triangle kernel over which grid, which scratch — is a pure function, so it is enumerated HERE, on the
CPU, under AddressSanitizer + UBSan, over every combination of context state and requested outputs (VERDICT round 3, item 7:
"no host-side unit can run without a GPU"). api_frame.hip executes the plan and decides nothing itself."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_frame_invariants_over_every_combination(tmp_path):
    exe = str(tmp_path / "frame_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "native", "frame_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    last = out.stdout.strip().split("\n")[-1]
    assert last.startswith("PLAN OK"), out.stdout[-2000:]
    assert int(last.split()[2]) > 5_000_000  # the sweep really ran


def test_prefix_tag_rule_over_call_sequences(tmp_path):
    """PrefixTags (renderer_amd/csrc/prefix_tags.hpp), the rule that hands out the tags of the cross-tile prefix state: direct
    launches, recorded chains of every even length and their replays, clears forced by a new instance count, starts up to the
    tag wrap — against a model of the two accumulator buffers. A wrong tag on the GPU is not a crash, it is wrong command bytes."""
    exe = str(tmp_path / "prefix_tags_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "native", "prefix_tags_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    last = out.stdout.strip().split("\n")[-1]
    assert last.startswith("TAGS OK"), out.stdout[-2000:]
    assert int(last.split()[2]) > 4_000_000  # the sweep really ran


def test_skin_plan_tables_over_every_small_skeleton(tmp_path):
    """plan_skeleton (renderer_amd/csrc/skin_plan.hpp), the integer tables the skinning kernel walks: every legal parent array
    of up to seven joints, the hierarchy families of tests/skinned_cases.py and seeded random arrays for 8 .. 32 joints — the
    depth order, the packed words, both multiply-shift divisions, and the kernel's level walk replayed with integer labels
    against the parent-order recursion. A wrong table on the GPU is not a crash, it is a joint composed with the wrong parent."""
    exe = str(tmp_path / "skin_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "native", "skin_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    last = out.stdout.strip().split("\n")[-1]
    assert last.startswith("SKIN OK"), out.stdout[-2000:]
    assert int(last.split()[3]) == 5913               # every legal parent array of 1 .. 7 joints
    assert int(last.split()[2]) >= 5913 + 25 * 164    # 8 .. 32 joints: four families + 160 random arrays each: the sweep really ran


def test_batch_plan_selects_the_kernels_the_entry_points_selected(tmp_path):
    """plan_batch (renderer_amd/csrc/batch_plan.hpp), which instantiation of the batched-draws stage every launch of a call is:
    every entry point, mode, bucket count at the pass boundaries, with and without matrices, both census decisions — against the
    nested conditions the three entry points held before they shared one plan. A wrong entry is another key policy's kernel.
    Then the pass schedule (batch_pass_io, batch_pass_launch, batch_run_stage_list) of every plan, views and sorted included,
    against the three pass loops the host held before it had one pass driver, and its invariants: a wrong ping-pong index is
    a pass that reads the list it writes."""
    exe = str(tmp_path / "batch_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "native", "batch_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    last = out.stdout.strip().split("\n")[-1]
    assert last.startswith("BATCH PLAN OK"), out.stdout[-2000:]
    assert int(last.split()[3]) == 2 * 2 * 15 * 4 + 2 * 10 * 4   # draws and lods at 15 bucket counts, ordered at the 10 it accepts
    schedule = out.stdout.strip().split("\n")[-2]
    assert schedule.startswith("BATCH SCHEDULE OK"), out.stdout[-2000:]
    # the plans above, shard and views at the 15 bucket counts, sorted at 3 key widths x mode x metric x matrices x census
    assert int(schedule.split()[3]) == 2 * 2 * 15 * 4 + 2 * 10 * 4 + 2 * 15 * 2 + 2 * 15 + 2 * 2 * 3 * 2 * 2


def test_plan_header_has_no_hip_dependency():
    """frame_plan.hpp, prefix_tags.hpp, skin_plan.hpp and batch_plan.hpp must stay compilable by a plain host compiler: that is
    what keeps the decision tables, the tag rule and the skeleton tables testable here."""
    for header in ("frame_plan.hpp", "prefix_tags.hpp", "skin_plan.hpp", "batch_plan.hpp"):
        text = open(os.path.join(ROOT, "renderer_amd", "csrc", header)).read()
        assert "hip/" not in text and "__device__" not in text and "__global__" not in text, header
    api = open(os.path.join(ROOT, "renderer_amd", "csrc", "api_frame.hip")).read()
    # the launch code takes the kernel, the grids and the scratch from the plan
    for field in ("plan.n_tiles", "plan.tri_blocks", "plan.recompact_blocks", "plan.skin_blocks", "frame_kernel_of(plan, ", "plan.need_tri_scratch",
                  "plan.need_part_status", "plan.need_chunk_scratch"):
        assert field in api, field
