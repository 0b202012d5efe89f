"""The next step's head (pyramid, early LK images, extractor) beside the LK launch that is still at the tail of the main stream, and the
two sets of LK working images that make it possible (ygz_internal.h: klt_tail / head_aside / klt_set).

Two frame sets: A is a synthetic sequence, B another texture seed with inverted intensities, so a stale or clobbered working image cannot
pass by luck.  Every comparison is bit for bit.  References are fresh contexts with overlap DISABLED (one stream, one image set: the path the
oracle tests anchor): either one that only ever saw the frames in question (`_only`), or -- where the call sequence itself is the case, e.g.
LK started again from its own result -- one that plays the same calls.  uploads wait for everything (they are full joins), so the scripts that
must have LK still in flight when the next head starts place the upload of the next frames in front of that LK launch ("pre", "upload", "klt").

Whether a flip happened is visible through the existing ABI: every context has one spare slot outside the pair table whose framed copy is
built once ("spare"); a flip marks the framed copies of all slots it does not rebuild as missing, so download_framed_level of the spare slot
("probe") gives None after a flip and the image otherwise.  The probe is itself an ordinary entry point and ends the overlap, so it stands
behind the reads.  _play returns (what the "read" ops saw, what the probes saw).

Shapes: 320 x 240 with batch 4 and batch 2 (pairs 0<->1: every slot is both reference and current, one flip touches every buffer LK reads),
and 64 x 48, whose LK pyramid stops after two levels (klt_prep_levels < 5).  That size yields few keypoints (tracks of a pair = keypoints of its
reference frame: A 3 and 2, B 2 and 0), so there the guard against an empty case asks for a track in every pair of A -- whose LK is the one that
runs beside the next head -- and in one pair of B; at 320 x 240 for 20 in every pair."""
import functools
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu

I7 = np.array([0, 0, 0, 1.0, 0, 0, 0])
SHAPES = [(320, 240, 4), (320, 240, 2), (64, 48, 2)]


@functools.lru_cache(maxsize=None)
def _frames(name, w, h, n):
    from ygz_slam_amd import synth
    seq = synth.Sequence(n, w, h, seed=5 if name == "A" else 23, step=0.3)
    fr = [seq.frame(i).copy() for i in range(n)]
    if name == "B":
        fr = [255 - f for f in fr]
    return fr, [seq.depth(i).copy() for i in range(n)]


def _play(lib, script, w, h, n, overlap):
    """runs the ops of `script` on a fresh context; returns what the "read_*" ops saw, in order"""
    ctx = lib.HipContext(width=w, height=h, levels=3, max_frames=n + 1)      # slot n: the spare slot of the flip probe
    q, t = list(range(n)), [(i - 1) % n for i in range(n)]
    out, probes, st = [], [], {}

    def upload(name, slots):
        for s in slots:
            ctx.upload_bgr(s, _frames(name, w, h, n)[0][s])

    def depths(name):
        for s in range(n):
            px = ctx.get_keypoints(s)["px"]
            d = _frames(name, w, h, n)[1][s][px[:, 1].astype(int), px[:, 0].astype(int)].astype(np.float64)
            ctx.set_keypoint_depths(s, d, np.ones(len(d), np.uint8))

    def head(prepare=True):
        ctx.build_pyramid(0, n, from_bgr=True)
        if prepare:
            ctx.track_klt_prepare()
        ctx.detect(0, n)

    def pre():
        ctx.track_reload(True); ctx.track_sparse_align(); ctx.match_slots_again(1); ctx.track_direct()

    def read_klt():
        return [tuple(a.tobytes() for a in ctx.track_get_klt(p)) for p in range(n)]

    for op in script:
        arg = op.split()[1] if " " in op else None
        op = op.split()[0]
        if op == "setup":                       # frames `arg` resident, pair tables and track sets loaded, then the overlap setting under test
            upload(arg, range(n)); head(False); depths(arg)
            ctx.match_slots(q, t, 1)
            ctx.track_begin(q, t, np.tile(I7, (n, 1)), np.tile(I7, (n, 1)), predict=True)
            ctx.set_overlap(overlap)
            kp = ctx.get_keypoints(0)                # candidates of the single-frame calls below (any valid pixels do)
            d = _frames(arg, w, h, n)[1][0][kp["px"][:, 1].astype(int), kp["px"][:, 0].astype(int)].astype(np.float64)
            P = ctx.params
            st["px"], st["level"] = kp["px"], kp["level"]
            st["gray"] = [ctx.download_level(s, 0) for s in range(n)]
        elif op == "regray":                        # the pyramids and keypoints of `arg` again, from gray uploads: valid pyramids while the BGR store holds other frames
            for s in range(n):
                ctx.upload_gray(s, st["gray"][s])
            ctx.build_pyramid(0, n, from_bgr=False); ctx.detect(0, n)
            st["pw"] = np.stack([(kp["px"][:, 0] - P.cx) * d / P.fx, (kp["px"][:, 1] - P.cy) * d / P.fy, d], 1)
        elif op == "spare":                         # a partial rebuild: never a flip
            ctx.upload_bgr(n, _frames("A", w, h, n)[0][0]); ctx.build_pyramid(n, 1, from_bgr=True)
        elif op == "probe":
            probes.append(ctx.download_framed_level(n, 0) is not None)
        elif op == "fdp_begin":                     # queued on the main stream, not waited for: reads the levels of slots 0 and 1
            m = len(st["px"])
            st["n_fdp"] = ctx.find_direct_projection_mp_begin(1, I7, [0], [I7], np.zeros(m, np.int32), st["pw"], st["px"], st["level"])
        elif op == "fdp_end":
            out.append(tuple(v.tobytes() for _, v in sorted(ctx.find_direct_projection_mp_end(st["n_fdp"]).items())))
        elif op == "align2d":                       # reads level 0 of slot 1 on the main stream
            m = min(64, len(st["px"]))
            pwb = np.random.default_rng(3).integers(0, 256, (m, 100)).astype(np.uint8)
            out.append(tuple(np.ascontiguousarray(a).tobytes() for a in ctx.align2d(1, 0, pwb, st["px"][:m])))
        elif op == "upload":
            upload(arg, range(n))
        elif op == "upload01":
            upload(arg, range(2))
        elif op == "upload_async":
            ctx.upload_bgr_batch(0, np.stack(_frames(arg, w, h, n)[0]), wait=False)
        elif op == "depths":
            depths(arg)
        elif op == "head":
            head(True)
        elif op == "head_noprep":
            head(False)
        elif op == "build":
            ctx.build_pyramid(0, n, from_bgr=True)
        elif op == "build01":
            ctx.build_pyramid(0, 2, from_bgr=True)
        elif op == "pre":
            pre()
        elif op == "klt":
            ctx.track_klt()
        elif op == "tail":
            pre(); ctx.track_klt()
        elif op == "read_klt":
            out.append(read_klt())
        elif op == "read_all":
            kps = [tuple(v.tobytes() for _, v in sorted(ctx.get_keypoints(s).items())) for s in range(n)]
            prs = []
            for p in range(n):
                nm, T, its = ctx.track_get_pose(p)
                prs.append((tuple(a.tobytes() for a in ctx.get_matches(p)), tuple(a.tobytes() for a in ctx.track_get_direct(p)), nm, T.tobytes(), tuple(its)))
            out.append((kps, prs, read_klt()))
        else:
            raise ValueError(op)
    ctx.close()
    return out, probes


_REF = {}


def _only(lib, name, w, h, n):
    """one step on a context that only ever saw frame set `name`, overlap disabled: (keypoints, per-pair outputs, LK)"""
    k = (name, w, h, n)
    if k not in _REF:
        _REF[k] = _play(lib, ["setup " + name, "head", "tail", "read_all"], w, h, n, False)[0][0]
    return _REF[k]


# step(A) with B's upload in front of its LK launch, then B's head while that LK is in flight; LK of A is read only afterwards
T1_STAGED = ["setup A", "head", "tail", "spare", "probe", "head", "pre", "upload B", "klt", "head", "read_klt", "probe", "depths B", "tail", "read_all"]
# the same with the upload behind the step (asynchronous, but a full join: the head then follows LK on the main stream)
T1_PLAIN = ["setup A", "head", "tail", "spare", "probe", "head", "tail", "upload_async B", "head", "read_klt", "probe", "depths B", "tail", "read_all"]


@pytest.mark.parametrize("w,h,n", SHAPES)
@pytest.mark.parametrize("script", [T1_STAGED, T1_PLAIN], ids=["staged", "plain"])
def test_lk_keeps_its_images_while_the_next_head_runs(hip_lib, script, w, h, n):
    (klt_a, all_b), probes = _play(hip_lib, script, w, h, n, True)
    ref_a, ref_b = _only(hip_lib, "A", w, h, n), _only(hip_lib, "B", w, h, n)
    n_a, n_b = [len(p[0]) // 8 for p in ref_a[2]], [len(p[0]) // 8 for p in ref_b[2]]      # tracks per pair: the case is not empty
    print("tracks per pair", n_a, n_b, "probes", probes)
    assert (min(n_a) >= 20 and min(n_b) >= 20) if w >= 320 else (min(n_a) >= 1 and max(n_b) >= 1)
    assert probes == [True, script is not T1_STAGED], "a flip happens exactly where LK is still the tail of the main stream when the head starts"
    assert klt_a == ref_a[2], "LK of A changed by the head of B"
    assert all_b[0] == ref_b[0], "keypoints of B"
    assert all_b[1] == ref_b[1], "matches / direct projection / alignment pose of B"
    assert all_b[2] == ref_b[2], "LK of B"


# set selection is by state, not by count; the value is the script's reference: ("only", frame set) or "same" (the same calls, overlap disabled)
T2 = {"a_build_twice": (["setup A", "head", "pre", "upload B", "klt", "build", "build", "klt", "read_klt"], "same"),
      "b_klt_three_times": (["setup A", "head", "tail", "klt", "klt", "read_klt"], "same"),
      "c_no_prepare": (["setup A", "head", "pre", "upload B", "klt", "head_noprep", "depths B", "tail", "read_all"], ("only", "B")),
      "d_steps_a_b_a": (["setup A", "head", "pre", "upload B", "klt", "head", "depths B", "pre", "upload A", "klt", "head", "read_klt", "depths A", "tail",
                         "read_all"], ("only", "A"))}


@pytest.mark.parametrize("case", sorted(T2))
def test_set_selection_is_by_state(hip_lib, case):
    w, h, n = SHAPES[0]
    script, ref = T2[case]
    got = _play(hip_lib, script, w, h, n, True)[0]
    if ref == "same":
        assert got == _play(hip_lib, script, w, h, n, False)[0]
    else:
        assert got[-1] == _only(hip_lib, ref[1], w, h, n)
    if case == "d_steps_a_b_a":
        assert got[0] == _only(hip_lib, "B", w, h, n)[2], "LK of the middle step (B), read after the third head"


def test_partial_rebuild(hip_lib):
    """after step(A) only slots 0-1 are rebuilt from B: no flip, LK then reads B in slots 0-1 and A in slots 2-3 (the reference plays the same calls on one
    stream and one image set, where that is what the buffers hold)"""
    w, h, n = SHAPES[0]
    script = ["setup A", "head", "pre", "upload01 B", "klt", "build01", "klt", "read_klt"]
    got = _play(hip_lib, script, w, h, n, True)[0]
    assert got == _play(hip_lib, script, w, h, n, False)[0]
    assert got[0] != _play(hip_lib, ["setup A", "head", "tail", "klt", "read_klt"], w, h, n, False)[0][0], "the rebuilt slots must matter"


# entry points that read the levels on the main stream without a join of their own: they must come behind a head that runs aside, and a head must
# come behind them.  (b) is queued, not waited for, between LK and the rebuild of every slot; (a) follows a flip.
T5 = {"a_align2d_behind_a_flip": (["setup A", "head", "tail", "spare", "probe", "head", "pre", "upload B", "klt", "build", "align2d", "probe"], [True, False]),
      "b_fdp_begin_in_front_of_a_rebuild": (["setup A", "head", "tail", "spare", "probe", "upload B", "regray", "pre", "klt", "fdp_begin", "build", "fdp_end", "probe"],
                                            [True, True])}


@pytest.mark.parametrize("case", sorted(T5))
def test_unjoined_readers_of_the_levels(hip_lib, case):
    w, h, n = SHAPES[0]
    script, flips = T5[case]
    got, probes = _play(hip_lib, script, w, h, n, True)
    ref, ref_probes = _play(hip_lib, script, w, h, n, False)
    assert probes == flips and ref_probes == [True, True]
    assert got == ref


def test_overlap_off_and_switch_off(hip_lib, tmp_path):
    """the sequence of the first test with overlap disabled, and in a child process with YGZ_KLT_ASIDE=0 (read once per process): identical bytes.
    (The context has no allocated-bytes accounting, so that the second image set stays unallocated is not asserted.)"""
    w, h, n = SHAPES[0]
    ref, probes = _play(hip_lib, T1_STAGED, w, h, n, True)
    assert probes == [True, False]
    assert _play(hip_lib, T1_STAGED, w, h, n, False) == (ref, [True, True])      # no flip: the second image set is never asked for
    path = str(tmp_path / "switch_off.pkl")
    env = dict(os.environ); env["YGZ_KLT_ASIDE"] = "0"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert pickle.load(open(path, "rb")) == (ref, [True, True])


if __name__ == "__main__":
    from ygz_slam_amd import _lib
    pickle.dump(_play(_lib, T1_STAGED, *SHAPES[0], True), open(sys.argv[1], "wb"))
