"""ygz::LocalMapSelector on the MI355X, through tests/cpp/lms_surface.cpp in a subprocess under a time limit.  The same small map is built
twice by hand: six keyframes with their _cov_keyframes (one list holds a null), keyframe 24 bad, sixteen map points (one bad), four tracked
frames of which two see the same keyframes, one carries a point twice and the bad point, and one has no map point.  On one copy
StereoTracker::LocalKeyFrames runs frame by frame; on the other ONE LocalMapSelector::Select runs.  The lists are equal keyframe by keyframe,
_ref_keyframe is equal, `points` is the set rule of DESIGN.md section 28 applied to the list (std::set, first occurrence first, computed in the
program), `prior` is each feature's position in it, two frames with equal lists hold the same objects, and nothing else on frames, points or
keyframes moves."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu

CHECKS = ["call_answers_every_frame", "return_value", "lists_equal_keyframe_by_keyframe", "ref_keyframe_equal", "points_equal_the_set_rule",
          "prior_is_the_position_in_the_set", "voters_counted", "list_of_frame_0", "bad_keyframe_is_ref_and_not_listed", "frame_without_points",
          "equal_lists_share_one_object", "bad_point_is_in_no_set", "nothing_else_moves", "stats", "single_frame_call_equals_its_batch_entry",
          "no_frame_fails", "null_frame_fails", "too_many_neighbours_fails", "dangling_observation_dropped"]


def test_one_select_equals_local_keyframes_frame_by_frame(tmp_path):
    from test_lms_surface_build import build_program
    exe = build_program(str(tmp_path))
    r = subprocess.run([exe, "run"], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.split("\n")[:-1] == [c + " ok" for c in CHECKS], r.stdout
