// ygz::Initializer (include/ygz/Algorithm/Initializer.h) over ygz_hip_initialize: the reference's TryInitialize (src/Algorithm/Initializer.cpp:9-87)
// as one device call -- sample sets, 200 H and 200 F hypotheses with their scores, the model choice and the reconstruction
// (ygz_slam_amd/csrc/init.hip).  Error conventions of the other surfaces: a failed call logs and returns false, only a missing device throws.
#include "ygz/Algorithm/Initializer.h"
#include "ygz/hip/Runtime.h"
#include "ygz_hip.h"
#include <cmath>

namespace Sophus {
// SO3(const Matrix3d &) = Eigen::Quaterniond(const Matrix3d &): the trace branch, else the largest diagonal (on the device
// ygz_quat_from_matrix of csrc/posemath_dev.h, restated in tests/init_ref.c; what ygz_hip_initialize returns as T21)
SO3::SO3(const Matrix3d &R)
{
    const double *m = R.m;
    const double tr = m[0] + m[4] + m[8];
    if (tr > 0) {
        double t = std::sqrt(tr + 1.0);
        q_[3] = 0.5 * t;
        t = 0.5 / t;
        q_[0] = (m[2 * 3 + 1] - m[1 * 3 + 2]) * t;
        q_[1] = (m[0 * 3 + 2] - m[2 * 3 + 0]) * t;
        q_[2] = (m[1 * 3 + 0] - m[0 * 3 + 1]) * t;
    } else {
        int i = 0;
        if (m[4] > m[0]) i = 1;
        if (m[8] > m[i * 3 + i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        double t = std::sqrt(m[i * 3 + i] - m[j * 3 + j] - m[k * 3 + k] + 1.0);
        q_[i] = 0.5 * t;
        t = 0.5 / t;
        q_[3] = (m[k * 3 + j] - m[j * 3 + k]) * t;
        q_[j] = (m[j * 3 + i] + m[i * 3 + j]) * t;
        q_[k] = (m[k * 3 + i] + m[i * 3 + k]) * t;
    }
}
}  // namespace Sophus

namespace ygz {

bool Initializer::TryInitialize(vector<Vector2d> &px1, vector<Vector2d> &px2, Frame *ref, Frame *curr)
{
    assert(px1.size() == px2.size());
    _ref = ref; _curr = curr;
    const int n = (int)px1.size();
    _inliers = vector<bool>(px1.size(), true);
    if (px2.size() != px1.size()) { LOG(ERROR) << "Initializer::TryInitialize: " << px1.size() << " and " << px2.size() << " pixels" << endl; return false; }
    const PinholeCamera *cam = Frame::GetCamera();
    if (!cam) { LOG(ERROR) << "Initializer::TryInitialize: no camera (Frame::SetCamera)" << endl; return false; }
    const Matrix3d K = cam->GetCameraMatrix();
    const double K4[4] = { K(0, 0), K(1, 1), K(0, 2), K(1, 2) };
    ygz_init_params prm;
    prm.sigma = _options._sigma; prm.sigma2 = _options._sigma2; prm.max_iter = _options._max_iter;
    prm.min_parallax = _options._min_parallex; prm.min_triangulated = _options._min_triangulated_pts; prm.good_point_ratio_h = _options.good_point_ratio_H;
    vector<double> a(2 * (size_t)n), b(2 * (size_t)n), p3d(3 * (size_t)n);
    vector<uint8_t> tri((size_t)n);
    for (int i = 0; i < n; ++i) { a[2 * i] = px1[i][0]; a[2 * i + 1] = px1[i][1]; b[2 * i] = px2[i][0]; b[2 * i + 1] = px2[i][1]; }
    ygz_init_result res;
    if (!hip::check(ygz_hip_initialize(hip::Runtime::Get().ctx(), a.data(), b.data(), n, K4, &prm, &res, p3d.data(), tri.data()), "initialize"))
        return false;
    Matrix3d R21;
    for (int k = 0; k < 9; ++k) R21.m[k] = res.R21[k];
    _T21 = SE3(R21, Vector3d(res.t21[0], res.t21[1], res.t21[2]));     // :79
    if (!res.success) return false;
    _inliers.assign((size_t)n, false);
    _pts_triangulated.assign((size_t)n, Vector3d());
    for (int i = 0; i < n; ++i) {
        _inliers[i] = tri[i] != 0;
        _pts_triangulated[i] = Vector3d(p3d[3 * i], p3d[3 * i + 1], p3d[3 * i + 2]);
    }
    return true;
}

}  // namespace ygz
