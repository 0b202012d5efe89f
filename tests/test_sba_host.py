"""ygz::BundleAdjuster's problem gathering and outlier erasure on the host, without a device and under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/cpp/sba_host.cpp, a stand-alone program with its own main written against include/ygz only, is compiled
together with ygz_slam_amd/host/ygz_sba.cpp with -fsanitize=address,undefined (the two libraries it links are not instrumented) and run.  It
builds keyframes, features and map points by hand: which keyframes become poses and which of them are fixed, which points and edges enter
and in which order, where a stereo edge arises, what is refused, and that an erasure takes the observation away on both sides and nothing
else."""
import os
import subprocess

from conftest import ROOT

PKG = os.path.join(ROOT, "ygz_slam_amd")

CHECKS = ["null_keyframe_refused", "local_poses_by_id_with_the_observers_fixed", "points_by_keyframe_id_then_feature_index",
          "point_with_one_edge_left_out_and_counted", "bad_point_and_bad_keyframe_give_no_edge", "stereo_edges_where_the_keyframe_has_a_right_column",
          "edges_name_their_features", "cleared_right_columns_give_mono_edges", "flags_of_another_length_refused",
          "outlier_observations_erased_on_both_sides", "nothing_else_changes", "second_erasure_is_a_no_op",
          "global_poses_once_each_by_id_the_first_fixed", "without_right_columns_every_edge_is_mono",
          "local_without_observers_fixes_the_smallest_free_keyframe", "free_keyframe_without_an_edge_refused"]


def test_gather_and_erase_host_program_under_sanitizers(tmp_path):
    assert os.path.exists(os.path.join(PKG, "libygz_host.so")), "libygz_host.so is not built (run __graft_entry__.build())"
    exe = str(tmp_path / "sba_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "sba_host.cpp"),
                           os.path.join(PKG, "host", "ygz_sba.cpp"), "-o", exe, "-L", PKG, "-lygz_host", "-lygz_hip", "-Wl,--no-undefined",
                           "-Wl,-rpath," + PKG])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.split("\n")[:-1] == [c + " ok" for c in CHECKS], r.stdout
