"""KeyFrameCulling::SetBadFlag on the host, without a device: tests/cpp/cull_host.cpp, a stand-alone program written against include/ygz
only, compiles and links with -Wl,--no-undefined against both libraries and runs.  It builds a handful of frames, features and map points by
hand: the observation is erased, a point that drops under min_obs goes bad and releases its other feature, the connections go on both sides,
a second call is a no-op, min_obs = 0 and 3, stale and bad points are only let go."""
import os
import subprocess

from conftest import ROOT

PKG = os.path.join(ROOT, "ygz_slam_amd")

CHECKS = ["observation_erased", "survivor_point_stays", "point_under_min_obs_goes_bad", "other_feature_released", "feature_without_point_untouched",
          "keyframe_bad", "own_connections_cleared", "connections_removed_on_both_sides", "survivors_stay_connected",
          "one_sided_connection_named_by_the_keyframe", "invariant", "second_call_is_a_no_op", "one_sided_through_a_shared_point",
          "min_obs_0_keeps_points", "min_obs_3_kills_a_point_of_one", "stale_and_bad_points_let_go"]


def test_set_bad_flag_host_program(tmp_path):
    assert os.path.exists(os.path.join(PKG, "libygz_host.so")), "libygz_host.so is not built (run __graft_entry__.build())"
    exe = str(tmp_path / "cull_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "cull_host.cpp"), "-o", exe, "-L", PKG, "-lygz_host", "-lygz_hip",
                           "-Wl,--no-undefined", "-Wl,-rpath," + PKG])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    assert r.stdout.split("\n")[:-1] == [c + " ok" for c in CHECKS], r.stdout
