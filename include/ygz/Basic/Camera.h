// ygz::PinholeCamera -- same surface as include/ygz/Basic/Camera.h:10-112 (float intrinsics, double maths).
#ifndef YGZ_CAMERA_H_
#define YGZ_CAMERA_H_
#include "ygz/Basic/Common.h"
#include "ygz/Basic/Config.h"
namespace ygz {
class PinholeCamera {
public:
    PinholeCamera()
    {
        _fx = Config::Get<float>("camera.fx"); _fy = Config::Get<float>("camera.fy");
        _cx = Config::Get<float>("camera.cx"); _cy = Config::Get<float>("camera.cy");
        _k1 = Config::Get<float>("camera.k1"); _k2 = Config::Get<float>("camera.k2");
        _p1 = Config::Get<float>("camera.p1"); _p2 = Config::Get<float>("camera.p2");
        _f = (_fx + _fy) / 2;
    }
    inline Vector3d World2Camera(const Vector3d &p_w, const SE3 &T_c_w) { return T_c_w * p_w; }
    inline Vector3d Camera2World(const Vector3d &p_c, const SE3 &T_c_w) { return T_c_w.inverse() * p_c; }
    inline Vector2d Camera2Pixel(const Vector3d &p_c) { return Vector2d(_fx * p_c[0] / p_c[2] + _cx, _fy * p_c[1] / p_c[2] + _cy); }
    inline Vector3d Pixel2Camera(const Vector2d &p_p, double depth = 1) { return Vector3d((p_p[0] - _cx) * depth / _fx, (p_p[1] - _cy) * depth / _fy, depth); }
    inline Vector2d Pixel2Camera2D(const Vector2d &p_p) { return Vector2d((p_p[0] - _cx) / _fx, (p_p[1] - _cy) / _fy); }
    inline Vector3d Pixel2World(const Vector2d &p_p, const SE3 &T_c_w, double depth = 1) { return Camera2World(Pixel2Camera(p_p, depth), T_c_w); }
    Vector2d World2Pixel(const Vector3d &p_w, const SE3 &T_c_w) { return Camera2Pixel(World2Camera(p_w, T_c_w)); }
    inline float fx() const { return _fx; }
    inline float fy() const { return _fy; }
    inline float cx() const { return _cx; }
    inline float cy() const { return _cy; }
    inline float focal() const { return _f; }
    // the lens coefficients of camera.k1, k2, p1, p2 (0 when the configuration has none)
    inline float k1() const { return _k1; }
    inline float k2() const { return _k2; }
    inline float p1() const { return _p1; }
    inline float p2() const { return _p2; }
    inline bool HasDistortion() const { return _k1 != 0 || _k2 != 0 || _p1 != 0 || _p2 != 0; }
    // Brown-Conrady on normalised coordinates, k3 = 0: the model Frame::InitFrame undistorts level 0 with (ygz_hip_set_undistortion, the order and
    // parentheses of tests/undist_ref.c).  Not the reference's UndistortPoint, whose tangential terms are not Brown-Conrady's
    inline Vector2d DistortPoint(const Vector2d &p) const
    {
        const double k1 = _k1, k2 = _k2, p1 = _p1, p2 = _p2, x = p[0], y = p[1];
        const double x2 = x * x, y2 = y * y, r2 = x2 + y2, xy2 = 2.0 * (x * y);
        const double kr = 1.0 + ((0.0 * r2 + k2) * r2 + k1) * r2;
        return Vector2d((x * kr + p1 * xy2) + p2 * (r2 + 2.0 * x2), (y * kr + p1 * (r2 + 2.0 * y2)) + p2 * xy2);
    }
    inline Matrix3d GetCameraMatrix() const                     // Camera.h:28-34
    { Matrix3d m; m(0, 0) = _fx; m(0, 2) = _cx; m(1, 1) = _fy; m(1, 2) = _cy; m(2, 2) = 1; return m; }
protected:
    float _fx, _fy, _cx, _cy, _f;
    float _k1, _k2, _p1, _p2;
};
}
#endif
