"""Subprocess driver of tests/test_gpu_cull_surface.py: runs tests/cpp/cull_surface.cpp (loaded with ctypes) -- ygz::KeyFrameCulling on a map
built by hand, against a plain host loop over the same map -- and writes its checks to an .npz file.
Usage: cull_driver.py <libcull_surface.so> <out.npz>.  Test infrastructure, never imported by the package."""
import ctypes
import sys

import numpy as np

# the checks of cull_run, in its order
CHECKS = ["redundancy_equals_the_host_loop", "redundancy_changes_nothing", "first_and_protected_keyframes_are_redundant", "culls_some_keeps_some",
          "cull_equals_the_host_loop", "points_were_killed", "features_and_points_agree", "no_good_point_names_a_bad_keyframe",
          "culled_keyframes_are_disconnected", "database_shrank_by_the_culled", "stats", "update_covisibility_reproduces_the_weights",
          "first_and_protected_keyframes_survive", "poses_and_positions_bit_unchanged", "ref_keyframes_repointed", "second_cull_equals_the_host_loop",
          "universe_of_five_is_left_alone", "level_slack_1_equals_the_host_loop", "outside_observers_count", "min_obs_0_kills_nothing"]
INFO = ["culled", "points_killed", "universe", "points", "observations", "culled_second_round", "culled_slack_1", "culled_of_three", "universe_of_three"]


def run(lib):
    checks, info = np.zeros(32), np.zeros(16)
    lib.cull_run.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    rc = lib.cull_run(checks.ctypes.data_as(ctypes.c_void_p), info.ctypes.data_as(ctypes.c_void_p))
    return rc, checks, info


if __name__ == "__main__":
    rc, checks, info = run(ctypes.CDLL(sys.argv[1]))
    np.savez(sys.argv[2], rc=rc, checks=checks, info=info)
    print(dict(zip(INFO, info[:len(INFO)].astype(int).tolist())))
    sys.exit(int(rc))
