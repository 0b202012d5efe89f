"""LoopClosing::ReplaceMapPoint on the host, without a device: tests/cpp/fuse_host.cpp, a stand-alone program written against include/ygz
only, compiles and links with -Wl,--no-undefined against both libraries and runs.  It builds a handful of frames, features and map points by
hand: disjoint keyframes, a shared keyframe (the feature loses its point), from == into, counters summed, `from` bad and empty, and the
_obs <-> _mappoint invariant afterwards."""
import os
import subprocess

from conftest import ROOT

PKG = os.path.join(ROOT, "ygz_slam_amd")

CHECKS = ["disjoint_moved", "disjoint_kept", "counters_summed", "from_bad_and_empty", "disjoint_invariant", "shared_keeps_own",
          "shared_feature_loses_point", "shared_other_moves", "shared_from_bad_and_empty", "shared_counters_summed", "shared_invariant",
          "same_point_untouched", "null_untouched", "same_invariant", "chain", "chain_invariant"]


def test_replace_map_point_host_program(tmp_path):
    assert os.path.exists(os.path.join(PKG, "libygz_host.so")), "libygz_host.so is not built (run __graft_entry__.build())"
    exe = str(tmp_path / "fuse_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "fuse_host.cpp"), "-o", exe, "-L", PKG, "-lygz_host", "-lygz_hip",
                           "-Wl,--no-undefined", "-Wl,-rpath," + PKG])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    assert r.stdout.split("\n")[:-1] == [c + " ok" for c in CHECKS], r.stdout
