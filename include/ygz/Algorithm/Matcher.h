// ygz::Matcher -- same surface as include/ygz/Algorithm/Matcher.h:15-152.  Brute-force matching is offered as
// BruteForceMatch (what test/test_orb_match.cpp:86-93 does with cv::BFMatcher).  The BoW-guided searches run on the GPU
// against the vocabulary loaded through ORBVocabulary::loadFromBinaryFile (the reference does not ship vocab/ORBvoc.bin).
#ifndef YGZ_MATCHER_H_
#define YGZ_MATCHER_H_
#include "ygz/Basic/Common.h"
#include "ygz/Basic/Sim3.h"
namespace ygz {
struct Frame;
struct MapPoint;
struct Feature;
class SparseImgAlign;
struct DMatch { int queryIdx = -1, trainIdx = -1; float distance = 0; };
class Matcher {
public:
    struct Options {
        int th_high = 100, th_low = 50;
        float knnRatio = 0.9f;
        bool checkOrientation = false;
        float initMatchRatio = 3.0f;
        int init_low = 30, init_high = 80;
        double _max_alignment_motion = 0.2;
        double _epipolar_dsqr = 1e-4;
    } _options;
    static const int HISTO_LENGTH = 30;
    Matcher();
    ~Matcher();
    void SetTCR(const SE3 &TCR) { _TCR_esti = TCR; }
    static int DescriptorDistance(const cv::Mat &a, const cv::Mat &b);                      // Matcher.cpp:30-43
    int CheckFrameDescriptors(Frame *frame1, Frame *frame2, list<pair<int, int>> &matches);  // Matcher.cpp:45-84
    int SearchByBoW(Frame *kf1, Frame *kf2, map<int, int> &matches);                          // Matcher.cpp:196-292
    int SearchForTriangulation(Frame *kf1, Frame *kf2, const Matrix3d &E12, vector<pair<int, int>> &matched_points,
                               const bool &onlyStereo = false);                               // Matcher.cpp:86-193
    // cv::BFMatcher(NORM_HAMMING, crossCheck).match(frame1 descriptors, frame2 descriptors) on the GPU
    int BruteForceMatch(Frame *frame1, Frame *frame2, vector<DMatch> &matches, bool cross_check = true);
    bool FindDirectProjection(Frame *ref, Frame *curr, MapPoint *mp, Vector2d &px_curr, int &search_level);   // Matcher.cpp:356-383
    bool FindDirectProjection(Frame *ref, Frame *curr, Feature *fea_ref, Vector2d &px_curr, int &search_level); // Matcher.cpp:385-417
    // the same for many features of `ref` in one launch (what LocalMapping::ProjectMapPoints loops over)
    int FindDirectProjectionBatch(Frame *ref, Frame *curr, const vector<Feature *> &fea_ref, vector<Vector2d> &px_curr,
                                  vector<int> &search_level, vector<bool> &ok);
    // LocalMapping::FindCandidates + ProjectMapPoints (src/Module/LocalMapping.cpp:47-120) in one launch: projects the local map
    // points into `current`, refines every co-visible observation with FindDirectProjection (MapPoint overload) and appends one
    // new Feature per matched map point to current->_features; side effects as the reference (_track_in_view = false when out
    // of view, _cnt_visible++ when in view).  Candidates are visited per map point in _obs (keyframe id) order -- the
    // reference's order is the heap-address order of a std::map<Feature*, ...>.  Returns the number of matched points.
    int ProjectMapPoints(Frame *current, const std::set<Frame *> &local_keyframes, const std::set<MapPoint *> &local_map_points);
    bool SparseImageAlignment(Frame *ref, Frame *current);                                  // Matcher.cpp:468-492

    // ---- descriptor searches guided by projection -- nothing in the reference; ORB-SLAM2's ORBmatcher::SearchByProjection(pKF, Scw, ...),
    // SearchBySim3 and Fuse(pKF, Scw, ...) over one device primitive (ygz_hip_search_by_projection).  A map point's
    // attributes are derived on the host, once per call (PointAttributes):
    //   descriptor  _distinctive_desc when it holds 32 bytes, else the descriptor of the reference observation = the _obs entry of the lowest
    //               key with a non-null feature and frame;
    //   dmax        |P - O_ref| 2^level_ref (the reference observation's camera centre and pyramid level);
    //   normal      the mean over _obs, in key order, of the unit rays (P - O_k) / |P - O_k|, not renormalised (ORB-SLAM2's UpdateNormalAndDepth);
    //   a point with no usable observation is skipped.
    struct PointAttr { uint8_t desc[32]; double dmax = 0; Vector3d normal = Vector3d(0, 0, 0); };
    static bool PointAttributes(const MapPoint *mp, PointAttr &out);
    // points projected into kf with (R, t / s, 1) of Scw, the viewing-angle test, Hamming distance <= 50 (ORB-SLAM2's TH_LOW, not _options.th_low) and the claim: `matched`
    // has one entry per feature of kf, its non-null entries mark taken keypoints; points that are bad or already in `matched` are skipped.
    // Fills `matched`, returns the number of new matches.
    int SearchByProjection(Frame *kf, const Sim3 &Scw, const vector<MapPoint *> &points, vector<MapPoint *> &matched, float th);
    // kf1's map points into kf2 with S21 * T_1w and kf2's into kf1 with S12 * T_2w (the scale is kept) in one device call: no viewing-angle
    // test, Hamming distance <= 100 (TH_HIGH), no claim; the sources skipped are the features already in matches12 (one entry per feature
    // of kf1: a map point of kf2 or nullptr) on side 1 and their map points' features on side 2; a target keypoint needs a good map point;
    // a pair is added when both directions agree.  Returns the number of pairs added.
    int SearchBySim3(Frame *kf1, Frame *kf2, vector<MapPoint *> &matches12, const Sim3 &S12, float th);
    // which feature of each keyframe a point would merge into (what ORB-SLAM2's Fuse decides, without acting on it): one problem per
    // keyframe with (R, t / s, 1) of Scw[k], the viewing-angle test, Hamming distance <= 50, no claim; points that are bad or already
    // observed by that keyframe are skipped.  feature_of_point[k][i] = feature index of kfs[k] or -1.  Read-only; returns the number of
    // (keyframe, point) hits.
    int SearchFuseCandidates(const vector<Frame *> &kfs, const vector<Sim3> &Scw, const vector<MapPoint *> &points, float th,
                             vector<vector<int>> &feature_of_point);
    // ORB-SLAM2's MapPoint::ComputeDistinctiveDescriptors for many points in one device call (ygz_hip_distinctive_descriptors, DESIGN.md
    // section 14; the reference ships MapPoint::ComputeDistinctiveDesc commented out).  Per good point the observations are the _obs entries
    // in key order whose feature is non-null and holds a continuous 32-byte _desc; _distinctive_desc becomes a 1 x 32 CV_8UC1 copy of the
    // one with the smallest median distance to the others (the first of equals).  Points with no such observation, or with more than 256,
    // keep _distinctive_desc as it is.  Returns the number of points set.
    int ComputeDistinctiveDescriptors(const vector<MapPoint *> &points);
    SE3 GetTCR() const { return _TCR_esti; }
private:
    SparseImgAlign *_align;
    SE3 _TCR_esti;
    // the last SearchForTriangulation of this object (frames and matched feature index pairs): what the Feature overload of FindDirectProjection speculates
    // on when LocalMapping::CreateNewMapPoints calls it once per matched pair (src/Module/LocalMapping.cpp:398-447)
    Frame *_tri_kf1 = nullptr, *_tri_kf2 = nullptr;
    vector<pair<int, int>> _tri_pairs;
};
}
#endif
