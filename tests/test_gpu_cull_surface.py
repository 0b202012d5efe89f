"""ygz::KeyFrameCulling on the MI355X (include/ygz/Algorithm/KeyFrameCulling.h) on a map built by hand -- fourteen keyframes along a line, the
middle ones redundant, _obs, levels, connections, a reference chain and an attached KeyFrameDatabase -- against a plain host loop over _obs that
tests/cpp/cull_surface.cpp codes independently: Redundancy gives its counts and changes nothing; Cull culls the same keyframes in the same
order and kills the same points; afterwards the map is consistent, the database shrank, the edited weights are what UpdateCovisibility
recounts, the first frame and a protected keyframe survive, a universe of five keyframes is left alone, and no pose or position moved.  The
program runs in a subprocess under a time limit (tests/cull_driver.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from cull_driver import CHECKS, INFO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from test_cull_surface_build import build_program
    d = tmp_path_factory.mktemp("cull_gpu")
    so = build_program(str(d))
    out = os.path.join(str(d), "cull.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cull_driver.py"), so, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return np.load(out)


@pytest.mark.parametrize("name", CHECKS)
def test_check(run, name):
    assert run["checks"][CHECKS.index(name)] == 1, dict(zip(INFO, run["info"].tolist()))


def test_the_map_is_about_something(run):
    """keyframes were culled in both rounds and under every option, points died, and the universe of three candidates is the whole line"""
    info = dict(zip(INFO, run["info"].astype(int).tolist()))
    assert info["universe"] == 14 and info["culled"] >= 2 and info["points_killed"] >= 2 and info["observations"] > 60 * 14
    assert info["culled_slack_1"] >= 1 and info["culled_of_three"] >= 1 and info["universe_of_three"] > 3
