"""YgzBlobLayout (ygz_slam_amd/csrc/ygz_blob.h), the offsets of the packed blocks of the upload / launch / copy-back entry points, without a
device: tests/cpp/blob_layout_host.cpp includes that header alone, is built with AddressSanitizer and UBSan (no recovery) and run as a program.
It checks the offsets against the recurrence x = o; o = round_up_256(o + bytes) for sizes 0, 1, 255, 256, 257 and a mix, that an absent array
takes no room, that every offset is a multiple of 256, that an overflowing size marks the layout bad instead of wrapping, and the totals of
the PnP, culling and keyframe-database blocks, restated in the program, at their smallest cases and at their capacities against plain
arithmetic.  The entry points' own ladders are held by the GPU suites."""
import os
import subprocess

from conftest import ROOT


def test_blob_layout_under_sanitizers(tmp_path):
    exe = str(tmp_path / "blob_layout_host")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + os.path.join(ROOT, "ygz_slam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "blob_layout_host.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout[-3000:], r.stderr[-3000:])


def test_the_header_needs_no_hip():
    h = open(os.path.join(ROOT, "ygz_slam_amd", "csrc", "ygz_blob.h")).read()
    assert "hip" not in "".join(line for line in h.splitlines() if line.startswith("#include"))
    mk = open(os.path.join(ROOT, "ygz_slam_amd", "csrc", "Makefile")).read()
    assert "$(wildcard *.h)" in mk[mk.index("build/%.o:"):].split("\n")[0]             # every object depends on every header of csrc/, this one among them
