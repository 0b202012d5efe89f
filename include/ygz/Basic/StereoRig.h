// ygz/Basic/StereoRig.h -- ygz::StereoRig: two cameras on a bar, as they come (two lenses, a relative rotation, a baseline that is not exactly
// along x), in front of the stereo chain that assumes rectified pictures (StereoMatcher, PoseOptimizer, BundleAdjuster).  Nothing in the
// reference, which is monocular.  Rectify() computes the rig's two rotations (ygz_hip_stereo_rectify: cv::stereoRectify's method) and sets
// the two rectifying maps of the process-wide context; InitPair() is Frame::InitFrame for the two frames of a pair through those maps
// (ygz_hip_build_pyramid_rectified, ygz_slam_amd/csrc/rectify.hip; the spec is DESIGN.md section 23 and tests/rect_ref.c).  Both rectified
// pictures are seen by Frame's one camera (the configuration's), so bf = fx * Baseline().
//
// Error conventions of the other surfaces: a failed call logs and returns false, only a missing device throws.  One thread at a time.
#ifndef YGZ_STEREO_RIG_H_
#define YGZ_STEREO_RIG_H_

#include "ygz/Basic/Common.h"
#include "ygz/Basic/Frame.h"

namespace ygz
{

class StereoRig
{
public:
    struct Lens { double fx = 0, fy = 0, cx = 0, cy = 0, k1 = 0, k2 = 0, p1 = 0, p2 = 0, k3 = 0; };
    struct Calibration {
        Lens left, right;
        double R[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 };      // X_right = R X_left + T (OpenCV's convention), row-major
        double T[3] = { -0.1, 0, 0 };
        int border_value = 0;                              // gray value of what a picture does not cover
    };

    explicit StereoRig(const Calibration &calibration) : _calibration(calibration) {}

    // the two rotations and both maps, once; false (and a log line) when the rig is refused: see ygz_hip_stereo_rectify, ygz_hip_set_rectification
    bool Rectify();
    bool Rectified() const { return _rectified; }

    // rotations (row-major) that turn the left and the right camera's rays into the rectified frame; metres between the rectified cameras
    const double *R1() const { return _R1; }
    const double *R2() const { return _R2; }
    double Baseline() const { return _baseline; }
    double bf() const;                                     // fx of the context's camera times Baseline()

    // What InitFrame does, for both frames of a pair, through the rectifying maps: _color (CV_8UC3 or CV_8UC1, both alike) goes up, level 0 is the
    // rectified gray, the pyramid follows; one device call when the two frames got neighbouring slots, two otherwise.  The frames belong to
    // the rig from then on: one that loses its slot and comes back from _color is rectified again, one that comes back from its fetched
    // _pyramid[0] is uploaded as it is, and Frame's destructor (or a plain InitFrame) ends the membership.
    bool InitPair(Frame *left, Frame *right);

private:
    Calibration _calibration;
    bool _rectified = false;
    double _R1[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 }, _R2[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 }, _baseline = 0;
};

}

#endif // YGZ_STEREO_RIG_H_
