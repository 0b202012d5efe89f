// ygz::Initializer used the way src/Module/VisualOdometry.cpp:121-151 uses it: TryInitialize, GetT21, GetTriangluatedPoints, then
// ba::TwoViewBACeres on the result.  Written against include/ygz only.  Usage: init_surface <input> where the input holds n, then n lines
// "u1 v1 u2 v2"; prints "ok <ret>", T21 (qx qy qz qw tx ty tz) and the n points "x y z inlier" as the Initializer handed them out
// (before the two-view BA), then "ba <translation norm>".  Built and run by tests/test_gpu_initializer.py (recipe in test_init_surface_build.py).
#include "ygz/Basic.h"
#include "ygz/Algorithm.h"
#include <cstdio>
using namespace ygz;

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    int n = 0;
    if (fscanf(f, "%d", &n) != 1) return 2;
    vector<Vector2d> pixels_ref(n), pixels_curr(n);
    for (int i = 0; i < n; ++i)
        if (fscanf(f, "%lf %lf %lf %lf", &pixels_ref[i][0], &pixels_ref[i][1], &pixels_curr[i][0], &pixels_curr[i][1]) != 4) return 2;
    fclose(f);
    PinholeCamera *cam = new PinholeCamera();
    Frame::SetCamera(cam);
    Frame *ref = new Frame(), *curr = new Frame();
    Initializer *init = new Initializer();
    init->_options._max_iter = 200;
    bool init_success = init->TryInitialize(pixels_ref, pixels_curr, ref, curr);
    printf("ok %d\n", init_success ? 1 : 0);
    SE3 T21 = init->GetT21();
    double T[7];
    T21.to7(T);
    for (int k = 0; k < 7; ++k) printf("%.17g%c", T[k], k < 6 ? ' ' : '\n');
    vector<Vector3d> pts_ref_triangulated;
    vector<bool> inliers;
    init->GetTriangluatedPoints(pts_ref_triangulated, inliers);
    for (size_t i = 0; i < pts_ref_triangulated.size(); ++i)
        printf("%.17g %.17g %.17g %d\n", pts_ref_triangulated[i][0], pts_ref_triangulated[i][1], pts_ref_triangulated[i][2], inliers[i] ? 1 : 0);
    if (init_success) {
        ba::TwoViewBACeres(ref->_TCW, T21, pixels_ref, pixels_curr, inliers, pts_ref_triangulated);
        printf("ba %.17g\n", T21.translation().norm());
    }
    delete init; delete ref; delete curr; delete cam;
    return 0;
}
