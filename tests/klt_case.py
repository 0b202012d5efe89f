"""The fixed input of tests/test_gpu_klt_bitexact.py (and tools/make_klt_golden.py, which wrote its fixture): two VGA frame pairs of
the benchmark's seeded batch (bench.py build_inputs, rank 0: frames 1 -> 0 and 2 -> 1), tracked by k_klt3 (the 21 x 21 window) twice:
  batched  the resident batched path of the step (ygz_hip_track_klt): the initial guess is the reference pixel itself;
  shifted  the same reference keypoints through ygz_hip_klt_track (the same kernel, one pair per launch) with use_initial_flow and
           initial guesses moved by a seeded offset of up to 2 pixels per axis, so that the iterations start away from the answer."""
import numpy as np

from ygz_slam_amd import synth

W, H, LEVELS = 640, 480, 3
CUR, REF = [1, 2], [0, 1]


def frames(n=3):
    """the first n frames of bench.py's batch: same texture, trajectory and render seeds (a prefix of the trajectory does not
    depend on its length)"""
    tex = synth.make_texture(1, W, H)
    poses = synth.trajectory(n, 11, 0.25)
    poses[0] = [0, 0, 0, 1, 0, 0, 0]
    rendered = [synth.render(tex[0], tex[1], poses[i], W, H, 1.0, 1000 + i) for i in range(n)]
    return np.stack([synth.gray_to_bgr(im, i) for i, (im, _) in enumerate(rendered)]), poses, np.stack([d for _, d in rendered])


def put(out, tag, res):
    pts, st, err = res
    out[tag + "pts"] = np.asarray(pts, np.float32)
    out[tag + "status"] = np.asarray(st, np.uint8)
    out[tag + "err"] = np.asarray(err, np.float32)


def track(lib):
    """{"<batched or shifted>_<pair>_{pts,status,err}": array} from one context"""
    bgr, poses, depths = frames()
    ctx = lib.HipContext(width=W, height=H, levels=LEVELS, max_frames=len(bgr))
    try:
        for s in range(len(bgr)):
            ctx.upload_bgr(s, bgr[s])
        ctx.build_pyramid(0, len(bgr), from_bgr=True)
        ctx.detect(0, len(bgr))
        for s in range(len(bgr)):
            px = ctx.get_keypoints(s)["px"]
            d = depths[s][px[:, 1].astype(np.int64), px[:, 0].astype(np.int64)]
            ctx.set_keypoint_depths(s, d, np.ones(len(d), np.uint8))
        out = {}
        ctx.track_begin(CUR, REF, poses[CUR], poses[REF], predict=False)
        ctx.track_klt()
        for p in range(len(CUR)):
            put(out, "batched_%d_" % p, ctx.track_get_klt(p))
        rng = np.random.default_rng(17)
        for p, (c, r) in enumerate(zip(CUR, REF)):
            pts = ctx.get_keypoints(r)["px"].astype(np.float32)
            init = pts + rng.uniform(-2.0, 2.0, pts.shape).astype(np.float32)
            put(out, "shifted_%d_" % p, ctx.klt_track(r, c, pts, init))
        return out
    finally:
        ctx.close()
