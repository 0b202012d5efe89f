"""The host-only logic of the resident map without a device: tests/cpp/rmap_host.cpp, a stand-alone program with its own main that includes
ygz_slam_amd/csrc/rmap_host.h -- the header ygz_hip_map_upload, ygz_hip_map_update and ygz_hip_stereo_local_map_resident check and lay out with
-- compiled with g++ -fsanitize=address,undefined and run directly.  The duplicate and range test of a delta equals a brute-force one on crafted
and random index lists, every refusal of a delta and of an upload is hit once, the three layouts neither overlap nor overflow unseen, and the
sanitizers see nothing."""
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rmap_host") / "rmap_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", os.path.join(ROOT, "tests", "cpp", "rmap_host.cpp"), "-o", out])
    return out


@pytest.mark.parametrize("mode", ("rows", "delta", "arrays", "layout"))
def test_mode_passes_under_the_sanitizers(exe, mode):
    r = subprocess.run([exe, mode], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == 1 and lines[0].startswith(mode + " ok ") and int(lines[0].split()[-1]) > 10, r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_usage(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stderr


def test_the_header_is_plain_cpp():
    text = open(os.path.join(ROOT, "ygz_slam_amd", "csrc", "rmap_host.h")).read()
    assert "hip_runtime" not in text and "ygz_internal.h" not in text and "__global__" not in text
    hip = open(os.path.join(ROOT, "ygz_slam_amd", "csrc", "rmap.hip")).read()
    assert '#include "rmap_host.h"' in hip and "ygz_rmap_check_arrays(" in hip and "ygz_rmap_check_delta(" in hip
    assert "RmapStore" in hip and "RmapCall" in hip and "RmapDelta" in hip and "ygz_rmap_grown(" in hip
