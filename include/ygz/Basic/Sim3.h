// ygz/Basic/Sim3.h -- ygz::Sim3, a similarity X -> s (R X) + t over the SO3 / Vector3d of Common.h.  Nothing in the reference (its loop closing
// is empty); the type came with ygz::LoopClosing and lives here so that Matcher.h can name it (SearchBySim3, SearchByProjection).
#ifndef YGZ_SIM3_H_
#define YGZ_SIM3_H_
#include "ygz/Basic/Common.h"
namespace ygz
{

// a similarity: X -> s (R X) + t
struct Sim3
{
    SO3 R;
    Vector3d t = Vector3d(0, 0, 0);
    double s = 1.0;

    Sim3() {}
    Sim3(const SO3 &R_, const Vector3d &t_, double s_) : R(R_), t(t_), s(s_) {}
    explicit Sim3(const SE3 &T) : R(T.so3()), t(T.translation()), s(1.0) {}

    Vector3d operator*(const Vector3d &p) const { return s * (R * p) + t; }
    Sim3 operator*(const Sim3 &o) const { return Sim3(R * o.R, s * (R * o.t) + t, s * o.s); }
    Sim3 operator*(const SE3 &T) const { return *this * Sim3(T); }
    Sim3 inverse() const { const SO3 Ri = R.inverse(); return Sim3(Ri, -(1.0 / s) * (Ri * t), 1.0 / s); }
    // qx qy qz qw tx ty tz s: SE3::to7's order, then the scale (the layout of ygz_sim3_result's S12 and of ygz_proj_problem's S)
    void to8(double out[8]) const
    { for (int i = 0; i < 4; ++i) out[i] = R.q_[i]; for (int i = 0; i < 3; ++i) out[4 + i] = t[i]; out[7] = s; }
    static Sim3 from8(const double in[8])
    { Sim3 S; for (int i = 0; i < 4; ++i) S.R.q_[i] = in[i]; for (int i = 0; i < 3; ++i) S.t[i] = in[4 + i]; S.s = in[7]; return S; }
};

}
#endif // YGZ_SIM3_H_
