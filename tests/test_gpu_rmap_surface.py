"""ygz::ResidentMap on the MI355X, through tests/cpp/rmap_surface.cpp in a subprocess under a time limit.  The map of tests/cpp/lmt_surface.cpp
is built twice: on one copy ONE LocalMapTracker::Track runs, on the other ResidentMap::Upload of the six keyframes and ONE ResidentMap::Track.
Both copies end equal: _TCW bitwise, every feature's _mappoint, _bad and _depth, every point's _cnt_visible, _cnt_found and _track_in_view,
_ref_keyframe, and the per-frame results.  Then three points and one keyframe move and one point turns bad: Upload before the move, Update
and Track on one copy equal a fresh Upload and Track on another."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu

CHECKS = ["copies_start_equal", "tracker_answers", "track_before_upload_fails", "upload", "track_answers_every_frame", "return_value",
          "state_equal_on_both_copies", "results_equal", "the_case_is_about_something", "stats", "keyframes_do_not_move", "no_frame_fails",
          "null_frame_fails", "repeated_frame_fails", "upload_of_nothing_fails_and_keeps_the_map", "upload_before_the_move",
          "update_pushes_and_skips", "fresh_upload_after_the_move", "update_then_track_equals_upload_then_track",
          "the_update_case_is_about_something"]


def test_resident_route_equals_the_tracker_and_update_equals_upload(tmp_path):
    from test_rmap_surface_build import build_program
    exe = build_program(str(tmp_path))
    r = subprocess.run([exe, "run"], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.split("\n")[:-1] == [c + " ok" for c in CHECKS], r.stdout
