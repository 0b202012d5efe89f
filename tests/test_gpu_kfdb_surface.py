"""ygz::KeyFrameDatabase on the MI355X (include/ygz/Algorithm/KeyFrameDatabase.h) on the scenes of the loop-closing and relocalisation
tests: the hits of Query equal common words counted and Frame::_vocab->score called per keyframe, the score as bits, for every keyframe;
DetectLoop with every field of its Stats, ComputeSim3's outcome, and Relocalize's outcome, pose and Stats are identical, bit for bit, with a
database attached, with none, and with one that holds only every second keyframe; Add and Erase return what the header says.  The program
runs in a subprocess under a time limit (tests/kfdb_driver.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

CONSISTENCY_TH = 3


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from test_kfdb_surface_build import build_program
    d = tmp_path_factory.mktemp("kfdb_gpu")
    so = build_program(str(d))
    out = os.path.join(str(d), "kfdb.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "kfdb_driver.py"), so, out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return np.load(out)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_the_scene_still_detects_its_loop(run):
    """the comparison below is about something: the loop is found on the (consistency_th + 1)-th revisit keyframe and relocalisation succeeds"""
    o = run["loop0"][:int(run["n_rev"])]
    assert (o[:CONSISTENCY_TH, 0] == 0).all() and o[CONSISTENCY_TH, 0] == 1 and o[CONSISTENCY_TH, 1] == 1, o[:, :3]
    assert (o[:CONSISTENCY_TH + 1, 21] >= 1).all()                   # candidates on every revisit keyframe up to the loop
    assert (run["reloc0"][:-1, 0] == 1).all() and run["reloc0"][-1, 0] == 0


@pytest.mark.parametrize("mode", [1, 2])
def test_detect_loop_and_compute_sim3_are_identical(run, mode):
    a, b = run["loop0"][:, :200], run["loop%d" % mode][:, :200]
    bad = np.argwhere(_bits(a) != _bits(b))
    assert len(bad) == 0, (bad[:8].tolist(), [(a[tuple(x)], b[tuple(x)]) for x in bad[:8]])


@pytest.mark.parametrize("mode", [1, 2])
def test_relocalize_is_identical(run, mode):
    a, b = run["reloc0"][:, :30], run["reloc%d" % mode][:, :30]
    bad = np.argwhere(_bits(a) != _bits(b))
    assert len(bad) == 0, (bad[:8].tolist(), [(a[tuple(x)], b[tuple(x)]) for x in bad[:8]])


def test_query_hits_equal_the_host_functions(run):
    for mode in (1, 2):
        o = run["loop%d" % mode]
        assert (o[:, 202] == 1).all(), (mode, o[:, 200:204])
        assert (o[:, 201] >= 1).all()                                # every keyframe shares words with some keyframe held
        r = run["reloc%d" % mode]
        assert (r[:, 30] == 1).all() and (r[:-1, 31] >= 1).all(), (mode, r[:, 30:32])
    full, half = run["loop1"][:, 203], run["loop2"][:, 203]
    assert (full == run["loop1"][:, 200] + 1).all()                  # every keyframe up to this one
    assert (half == np.floor(run["loop2"][:, 200] / 2) + 1).all()    # the even ids


def test_add_and_erase_return_values(run):
    c = run["checks"]
    assert (c[:12] == 1).all(), c[:12]
