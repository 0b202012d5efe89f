"""ygz::LocalMapTracker on the MI355X, through tests/cpp/lmt_surface.cpp in a subprocess under a time limit.  The small map of
tests/cpp/lms_surface.cpp is built twice with what tracking needs (pictures, poses, positions, descriptors, depths), plus one point whose
reference observation has no descriptor and one observation whose feature does not point back.  On one copy LocalMapSelector::Select and then
StereoLocalMap::TrackLocalMap run; on the other ONE LocalMapTracker::Track.  Both copies end equal: _TCW bitwise, every feature's _mappoint,
_bad and _depth, every point's _cnt_visible, _cnt_found and _track_in_view, _ref_keyframe, and the per-frame results.  The attributes the class
sent are bit-equal to Matcher::PointAttributes point by point, the descriptor-less point is in no list and is counted, and nothing else
moves."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu

CHECKS = ["copies_start_equal", "select_answers", "host_route_answers", "track_answers_every_frame", "return_value", "state_equal_on_both_copies",
          "results_equal", "ref_voters_cut_equal", "the_case_is_about_something", "attributes_bit_equal_to_point_attributes",
          "descriptorless_point_is_in_no_list_and_counted", "stats", "keyframes_do_not_move", "no_frame_fails", "null_frame_fails",
          "repeated_frame_fails"]


def test_one_track_equals_select_then_track_local_map(tmp_path):
    from test_lmt_surface_build import build_program
    exe = build_program(str(tmp_path))
    r = subprocess.run([exe, "run"], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.split("\n")[:-1] == [c + " ok" for c in CHECKS], r.stdout
