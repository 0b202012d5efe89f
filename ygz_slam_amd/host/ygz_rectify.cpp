// ygz::StereoRig (include/ygz/Basic/StereoRig.h) over ygz_hip_stereo_rectify, ygz_hip_set_rectification and ygz_hip_build_pyramid_rectified
// (ygz_slam_amd/csrc/rectify.hip).  Which frame belongs to which rig camera is the Runtime's table (Runtime::SetRigCamera): the re-upload of
// an evicted frame takes the same path there.  Error conventions of the other surfaces: a failed call logs and returns false, only a missing
// device throws.
#include "ygz/Basic/StereoRig.h"
#include "ygz/hip/Runtime.h"
#include "ygz_hip.h"

namespace ygz {

bool StereoRig::Rectify()
{
    _rectified = false;
    if (!hip::check(ygz_hip_stereo_rectify(_calibration.R, _calibration.T, _R1, _R2, &_baseline), "stereo_rectify")) return false;
    ygz_hip_ctx *c = hip::Runtime::Get().ctx();
    const Lens *lens[YGZ_RECT_CAMERAS] = { &_calibration.left, &_calibration.right };
    const double *rot[YGZ_RECT_CAMERAS] = { _R1, _R2 };
    for (int k = 0; k < YGZ_RECT_CAMERAS; ++k) {
        ygz_rectify_params p;
        if (!hip::check(ygz_hip_default_rectify_params(c, &p), "default_rectify_params")) return false;
        const Lens &l = *lens[k];
        p.lens.k1 = l.k1; p.lens.k2 = l.k2; p.lens.p1 = l.p1; p.lens.p2 = l.p2; p.lens.k3 = l.k3;
        p.lens.fx = l.fx; p.lens.fy = l.fy; p.lens.cx = l.cx; p.lens.cy = l.cy; p.lens.border_value = _calibration.border_value;
        for (int i = 0; i < 9; ++i) p.R[i] = rot[k][i];
        if (!hip::check(ygz_hip_set_rectification(c, k, &p), "set_rectification")) return false;
    }
    _rectified = true;
    return true;
}

double StereoRig::bf() const
{
    ygz_rectify_params p;
    if (!hip::check(ygz_hip_default_rectify_params(hip::Runtime::Get().ctx(), &p), "default_rectify_params")) return 0;
    return p.lens.fx * _baseline;                          // the default lens is the context's camera
}

bool StereoRig::InitPair(Frame *left, Frame *right)
{
    if (!left || !right || left == right) { LOG(ERROR) << "StereoRig::InitPair: two different frames are needed" << endl; return false; }
    if (!_rectified) { LOG(ERROR) << "StereoRig::InitPair: Rectify() has not succeeded" << endl; return false; }
    hip::Runtime &rt = hip::Runtime::Get();
    ygz_hip_ctx *c = rt.ctx();
    int w = 0, h = 0;
    ygz_hip_level_size(c, 0, &w, &h);
    Frame *f[2] = { left, right };
    for (int k = 0; k < 2; ++k) { rt.Release(f[k]); f[k]->_pyramid.clear(); }
    for (int k = 0; k < 2; ++k)
        if (f[k]->_color.empty() || f[k]->_color.cols != w || f[k]->_color.rows != h || f[k]->_color.channels() != left->_color.channels()) {
            LOG(ERROR) << "StereoRig::InitPair: _color (" << f[k]->_color.cols << " x " << f[k]->_color.rows << ") does not match image.width/height ("
                       << w << " x " << h << ") or the other frame's channels; no pyramid" << endl;
            return false;
        }
    const int bgr = left->_color.channels() == 3;
    int slot[2];
    for (int k = 0; k < 2; ++k) slot[k] = rt.Resident(f[k]);                          // no pyramid yet: slot only
    bool ok = slot[0] >= 0 && slot[1] >= 0 && left->_hip_slot == slot[0];            // (the second took the first one's slot: fewer than two slots)
    if (!ok) LOG(ERROR) << "StereoRig::InitPair: the two frames are not resident together" << endl;
    for (int k = 0; k < 2 && ok; ++k) {
        rt.SetRigCamera(f[k], k);
        const cv::Mat &im = f[k]->_color;
        ok = hip::check(bgr ? ygz_hip_upload_bgr(c, slot[k], im.data, (int)im.step) : ygz_hip_upload_gray(c, slot[k], im.data, (int)im.step), "upload");
    }
    if (ok) {
        if (slot[1] == slot[0] + 1 || slot[0] == slot[1] + 1) {                       // neighbours: both cameras in one launch
            const uint8_t cams[2] = { (uint8_t)(slot[0] < slot[1] ? 0 : 1), (uint8_t)(slot[0] < slot[1] ? 1 : 0) };
            ok = hip::check(ygz_hip_build_pyramid_rectified(c, slot[0] < slot[1] ? slot[0] : slot[1], 2, bgr, cams), "build_pyramid_rectified");
        } else {
            for (int k = 0; k < 2 && ok; ++k) {
                const uint8_t cam = (uint8_t)k;
                ok = hip::check(ygz_hip_build_pyramid_rectified(c, slot[k], 1, bgr, &cam), "build_pyramid_rectified");
            }
        }
    }
    if (!ok) { rt.Release(left); rt.Release(right); return false; }
    for (int k = 0; k < 2; ++k) f[k]->_pyramid.reset(f[k], (size_t)f[k]->_option._pyramid_level);      // levels are fetched when somebody indexes them
    return true;
}

}  // namespace ygz
