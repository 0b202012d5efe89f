"""Matcher::FindDirectProjection's memo on the host, without a device: tests/cpp/fdp_memo_host.cpp, written against include/ygz only, compiles and
links with -Wl,--no-undefined against both libraries and runs.  A map point with no observation in the keyframe asked about is "no projection" and
leaves its _obs as it was; a Frame destroyed after the Runtime (static destruction) does not touch the Runtime or its memo."""
import os
import subprocess

from conftest import ROOT

PKG = os.path.join(ROOT, "ygz_slam_amd")


def test_fdp_memo_host_program(tmp_path):
    assert os.path.exists(os.path.join(PKG, "libygz_host.so")), "libygz_host.so is not built (run __graft_entry__.build())"
    exe = str(tmp_path / "fdp_memo_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "fdp_memo_host.cpp"), "-o", exe, "-L", PKG, "-lygz_host", "-lygz_hip",
                           "-Wl,--no-undefined", "-Wl,-rpath," + PKG])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    assert r.stdout.split() == ["miss", "0", "0", "1"], r.stdout          # returned false, no entry for the keyframe asked about, the other one kept
