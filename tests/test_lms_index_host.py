"""The keyframe-major index of the local-map selection on the host, without a device: tests/cpp/lms_index_host.cpp, a stand-alone program with
its own main that includes ygz_slam_amd/csrc/lms_index.h -- the header ygz_hip_local_map_select builds its index with -- compiled with
g++ -fsanitize=address,undefined and run directly.  On the map of every case of tests/lms_ref.py (lists of 0 to 256 observations, keyframes of
0 to 257 features, shared (keyframe, feature) pairs, 1 to 4096 keyframes) the index equals a brute-force build, and the sanitizers see no write
past an array that has exactly its size."""
import os
import subprocess

import numpy as np

import lms_ref as lr
from conftest import ROOT


def test_index_equals_brute_force_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "lms_index_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", os.path.join(ROOT, "tests", "cpp", "lms_index_host.cpp"), "-o", exe])
    cases = lr.cases()
    files = []
    for name in sorted(cases):
        c = cases[name]
        path = str(tmp_path / (name + ".bin"))
        np.concatenate([[len(c["off"]) - 1, c["K"]], c["off"], c["kf"], c["feat"]]).astype(np.int32).tofile(path)
        files.append(path)
    r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.split("\n")[:-1]
    assert lines == ["%s.bin ok %d" % (name, len(cases[name]["kf"])) for name in sorted(cases)], r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    # the cases are ragged: empty lists, empty keyframes and a shared (keyframe, feature) are among them
    assert any((np.diff(c["off"]) == 0).any() for c in cases.values())
    c = cases["shared_feature"]
    assert len(set(zip(c["kf"].tolist(), c["feat"].tolist()))) < len(c["kf"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stderr
