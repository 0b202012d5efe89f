// ygz/Algorithm/StereoMatcher.h -- ygz::StereoMatcher: the depth of a left frame's features from a rectified stereo pair.  Nothing in the
// reference, which is monocular: this is ORB-SLAM2's Frame::ComputeStereoMatches on this data model -- a row-band descriptor search among the
// right frame's features, an 11 x 11 SAD search over +-5 columns at the feature's pyramid level, a parabola fit for the sub-pixel column and a
// median rule on the SAD values -- as one device call (ygz_hip_stereo_match, ygz_slam_amd/csrc/stereo.hip; the spec is DESIGN.md section 19
// and tests/stereo_ref.c).  The pictures are rectified: epipolar lines are image rows, and both frames are seen by Frame's one camera.
//
// A map built from such depths has metric scale: set LoopClosing::Options::_fix_scale = true for it.
// Error conventions of the other surfaces: a failed call logs and returns 0, only a missing device throws.  One thread at a time.
#ifndef YGZ_STEREO_MATCHER_H_
#define YGZ_STEREO_MATCHER_H_

#include "ygz/Basic.h"

namespace ygz
{

class StereoMatcher
{
public:
    struct Options {
        double _baseline = 0.1;         // metres between the two cameras
        double _min_disparity = 0;      // level-0 pixels
        double _max_disparity = 0;      // 0: the camera's fx
        int _th_dist = 75;              // a best descriptor distance at or above this is no match
    } _options;

    StereoMatcher() {}
    explicit StereoMatcher(const Options &options) : _options(options) {}

    // Both frames have had InitFrame (an evicted one is uploaded again); the keypoints are _features' _pixel, _level and _desc of both.
    // Feature::_depth of every left feature that was matched (status YGZ_STEREO_OK) is set, the others' are left alone; u_right, when
    // given, receives the sub-pixel column in the right picture per left feature (-1 where there is no match).  Returns the number set.
    int ComputeStereoMatches(Frame *left, Frame *right, std::vector<double> *u_right = nullptr);

    // per left feature of the last call: YGZ_STEREO_OK .. YGZ_STEREO_MEDIAN (include/ygz_hip.h)
    const std::vector<int> &GetStatus() const { return _status; }

private:
    std::vector<int> _status;
};

}

#endif // YGZ_STEREO_MATCHER_H_
