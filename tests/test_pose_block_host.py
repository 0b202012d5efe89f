"""The host plumbing shared by the launchers of k_pose_opt (ygz_slam_amd/csrc/pose_block.h) without a device: tests/cpp/pose_block_host.cpp
includes that header alone, is built with AddressSanitizer and UBSan (no recovery) and run as a program.  It checks ygz_pose_params_ok at
the defaults, at every exact limit and one past it, on chi2 of 0, below 0, NaN and infinity and on a NaN min_rel_decrease; ygz_all_finite on
an empty and a finite range and with a NaN or an infinity first, in the middle and last; YgzPoseBlock for 1 and 65 frames of 1 and 768
cells (every offset a multiple of 256, strictly increasing in the documented order, the end against plain arithmetic, copy_results into
buffers of exactly the documented sizes, absent outputs skipped); and ygz_distinct_slot on the slots 3, 1, 3, 0, 1.  The entry points' own
ladders are held by the GPU suites."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "ygz_slam_amd", "csrc")


def test_pose_block_under_sanitizers(tmp_path):
    exe = str(tmp_path / "pose_block_host")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "pose_block_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout[-3000:], r.stderr[-3000:])


def test_the_header_needs_no_hip_and_is_the_only_copy():
    h = open(os.path.join(CSRC, "pose_block.h")).read()
    includes = [line for line in h.splitlines() if line.startswith("#include")]
    assert not any("hip/" in line or "ygz_internal" in line for line in includes), includes
    mk = open(os.path.join(CSRC, "Makefile")).read()
    # every object depends on every header of csrc/, pose_block.h and slot_pose_dev.h among them
    assert "$(wildcard *.h)" in mk[mk.index("build/%.o:"):].split("\n")[0] and os.path.exists(os.path.join(CSRC, "slot_pose_dev.h"))
    # one range check, one finiteness check, one rotation rule under csrc/ (bow.hip keeps its own, held to the oracle)
    texts = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h"))}
    assert not any("isfinite(q.chi2_mono)" in t for t in texts.values())
    assert [f for f, t in texts.items() if "_finite(const double" in t] == ["pose_block.h"]
    assert [f for f, t in texts.items() if "max3 = max2" in t and f != "bow.hip"] == ["slot_pose_dev.h"]
    assert texts["slot_pose_dev.h"].count("int max1 = 0, max2 = 0, max3 = 0") == 1
    assert sum(t.count("r * (1.0f / 30)") for t in texts.values()) == 1
