"""What the host surfaces share (ygz_slam_amd/host/surface_share.h), without a device: tests/cpp/share_host.cpp, a stand-alone program,
compiles and links with -Wl,--no-undefined against both libraries and runs.  On frames, features and map points built by hand: the feature
arrays of a slot (level -1 counts as 0, depth 0 and -1 are no depth, the angle is a float), the keypoint arrays (a feature without 32
descriptor bytes refuses the frame), the point-set arrays (an unobserved point is left out, the four arrays stay in step), the write-back of a
pose optimisation (bitwise World2Camera under a non-identity pose), and the slot loader's refusals, which come before the runtime is reached:
the program never initialises a device."""
import os
import subprocess

from conftest import ROOT

PKG = os.path.join(ROOT, "ygz_slam_amd")

CHECKS = ["features_in_step", "features_pixels", "features_level_clamped", "features_has_depth", "features_angle_float", "keypoints_gathered",
          "keypoints_refuse_no_descriptor", "keypoints_refuse_short_descriptor", "append_refuses_unobserved", "append_in_step", "append_values",
          "append_search_struct", "good_once", "verdict_outlier", "verdict_inlier", "loader_refuses_null_frame", "loader_refuses_null_feature",
          "loader_refuses_overfull", "loader_touched_nothing"]


def test_surface_share_host_program(tmp_path):
    assert os.path.exists(os.path.join(PKG, "libygz_host.so")), "libygz_host.so is not built (run __graft_entry__.build())"
    exe = str(tmp_path / "share_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(PKG, "host"), os.path.join(ROOT, "tests", "cpp", "share_host.cpp"), "-o", exe, "-L", PKG,
                           "-lygz_host", "-lygz_hip", "-Wl,--no-undefined", "-Wl,-rpath," + PKG])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    assert r.stdout.split("\n")[:-1] == [c + " ok" for c in CHECKS], r.stdout
