// ygz/Algorithm/Initializer.h -- ygz::Initializer, the reference's monocular initialisation (include/ygz/Algorithm/Initializer.h,
// src/Algorithm/Initializer.cpp): the public surface as the reference declares it, the work on the GPU through ygz_hip_initialize
// (H / F RANSAC, model choice and reconstruction in one call; ygz_slam_amd/host/ygz_init.cpp).  Private members are this project's.
#ifndef YGZ_INITIALIZER_H_
#define YGZ_INITIALIZER_H_

#include "ygz/Basic.h"

namespace ygz
{

class Initializer
{
public:
    // px1 / px2: matched pixels of the reference and the current frame; true when a motion was accepted (Initializer.cpp:9-87)
    bool TryInitialize(vector<Vector2d> &px1, vector<Vector2d> &px2, Frame *ref, Frame *curr);

    SE3 GetT21() const { return _T21; }

    // the triangulated points (reference-camera coordinates) and which of them are good (the reference's spelling)
    void GetTriangluatedPoints(vector<Vector3d> &pts_3d, vector<bool> &inliers)
    {
        pts_3d = _pts_triangulated;
        inliers = _inliers;
    }

    struct Option
    {
        float _sigma = 2.0;
        float _sigma2 = 4.0;
        int _max_iter = 200;
        double _min_parallex = 1.0;
        int _min_triangulated_pts = 8;
        double good_point_ratio_H = 0.9;
    } _options;

private:
    vector<bool> _inliers;
    vector<Vector3d> _pts_triangulated;
    SE3 _T21;
    Frame *_ref = nullptr;
    Frame *_curr = nullptr;
};

}

#endif // YGZ_INITIALIZER_H_
