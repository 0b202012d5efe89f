// ygz/Algorithm/LoopClosing.h -- ygz::LoopClosing: loop detection.  The reference leaves the stage empty: LocalMapping.cpp:330 ends each
// keyframe with "put this keyframe into the loop-detection queue" and no code, and include/ygz/loop_closing.h is an empty `class LoopClosing {}`.
// This class takes that name and follows ORB-SLAM2's LoopClosing::DetectLoop (BoW candidates, KeyFrameDatabase::DetectLoopCandidates, the
// covisibility-group consistency) and LoopClosing::ComputeSim3 (SearchByBoW per candidate, then Sim3 RANSAC and the 7-dof refinement of every
// candidate in one device call, ygz_hip_sim3_ransac) with its second half, SearchLoopMapPoints: the accepted candidate's pairs widened by
// Matcher::SearchBySim3, then the map points of the loop keyframe's neighbourhood pulled in by Matcher::SearchByProjection, and the "enough
// matches in total" decision.  Those three detect only: no pose, map point, feature, observation or connection changes
// (ygz_slam_amd/host/ygz_loop.cpp).  CorrectLoop is the correcting half of ORB-SLAM2's LoopClosing::CorrectLoop: the Sim3 of the accepted loop
// is propagated to the current keyframe's neighbourhood, a Sim3 pose graph over the keyframes (Optimizer::OptimizeEssentialGraph's edges) is
// optimised in one device call (ygz_hip_pose_graph_optimize), and the keyframe poses and map points are rewritten from the result
// (ygz_slam_amd/host/ygz_correct.cpp).  FuseLoop is the rest of ORB-SLAM2's CorrectLoop up to its global BA: the
// duplicated map points of the revisited region are fused into the old ones (the current keyframe's matches, then Matcher::
// SearchFuseCandidates over the corrected neighbourhood), the surviving points' distinctive descriptors are recomputed
// (Matcher::ComputeDistinctiveDescriptors, ygz_hip_distinctive_descriptors) and the covisibility of every keyframe it touched is recounted
// (UpdateCovisibility, ygz_hip_covisibility) -- ygz_slam_amd/host/ygz_fuse.cpp.  The new connections are not fed back into the pose
// graph.  GlobalBundleAdjustment is what ORB-SLAM2's CorrectLoop ends with, RunGlobalBundleAdjustment, as a synchronous
// call: every keyframe pose and every map point with two observations or more against all of their observations in one device call
// (ygz_hip_global_ba: Levenberg-Marquardt, the points marginalised, conjugate gradients on the camera system) --
// ygz_slam_amd/host/ygz_gba.cpp.  It needs no loop state and may be called at any time.  The integration is in INTEGRATION.md.
// SetKeyFrameDatabase is optional: with a ygz::KeyFrameDatabase attached DetectLoop takes its BoW scores and common-word counts from one device
// query instead of one host walk per keyframe; every result is the same bit for bit (ygz/Algorithm/KeyFrameDatabase.h).
#ifndef YGZ_LOOP_CLOSING_H_
#define YGZ_LOOP_CLOSING_H_

#include "ygz/Basic.h"
#include "ygz/Basic/Sim3.h"
#include "ygz/Algorithm/Matcher.h"
#include <set>

namespace ygz
{

class KeyFrameDatabase;

// ygz::Sim3 is defined in ygz/Basic/Sim3.h (Matcher.h names it too) and exposed here as before:
//   struct Sim3 { SO3 R; Vector3d t; double s; Sim3(); Sim3(R, t, s); explicit Sim3(const SE3 &);
//                 Vector3d operator*(const Vector3d &) const; Sim3 operator*(const Sim3 &) const; Sim3 operator*(const SE3 &) const;
//                 Sim3 inverse() const; void to8(double out[8]) const; static Sim3 from8(const double in[8]); };

class LoopClosing
{
public:
    struct Option
    {
        int _min_kf_gap = 10;                   // keyframes after the last accepted loop (and after id 0) before another is detected
        int _consistency_th = 3;                // consecutive consistent detections a candidate needs
        double _min_common_words_ratio = 0.8;   // shared words above this fraction of the largest count
        double _acc_score_ratio = 0.75;         // group scores above this fraction of the best
        int _acc_covisibles = 10;               // covisibles of a candidate that join its group score
        float _knn_ratio = 0.75f;               // SearchByBoW's ratio
        int _min_bow_matches = 20;              // map-point pairs a candidate needs before RANSAC
        int _ransac_iterations = 300;           // ORB-SLAM2 LoopClosing::ComputeSim3 / Optimizer::OptimizeSim3's values
        double _ransac_chi2 = 9.210;
        int _min_inliers = 20;
        double _refine_chi2 = 10;
        bool _fix_scale = false;                // true for stereo / RGB-D maps
        int _min_total_matches = 40;            // matches of the current keyframe SearchLoopMapPoints needs to accept the loop
        float _sim3_search_th = 7.5f;           // SearchBySim3's window, level-0 pixels
        float _projection_search_th = 10.0f;    // SearchByProjection's
        int _min_essential_weight = 100;        // CorrectLoop: connected pairs with at least this weight get an edge (ORB-SLAM2's minFeat)
        float _fuse_search_th = 4.0f;           // FuseLoop: SearchFuseCandidates' window, level-0 pixels (ORB-SLAM2's SearchAndFuse)
        int _gba_iterations = 10;               // GlobalBundleAdjustment: LM iterations (ORB-SLAM2's RunGlobalBundleAdjustment)
        double _gba_huber_delta = 5.991;        // its Huber width in pixels (sqrt of ORB-SLAM2's thHuber2D squared: g2o's setDelta); <= 0: no kernel
    } _option;

    struct Stats
    {
        double min_score = 0;                   // minScore of the last DetectLoop
        vector<unsigned long> candidates;       // the group representatives of the last DetectLoop, by keyframe id
        vector<double> acc_scores;              // their group scores
        vector<int> consistency;                // their consistency (the largest over the previous groups they extend; 0 for a new group)
        vector<unsigned long> consistent;       // the enough-consistent ones, by keyframe id
        vector<int> bow_pairs;                  // per enough-consistent candidate: the map-point pairs of SearchByBoW (last ComputeSim3)
        vector<int> ransac_inliers;             // per enough-consistent candidate: -1 when it did not reach the device
        vector<int> refined_inliers;            // likewise
        int sim3_added = 0;                     // last SearchLoopMapPoints: pairs SearchBySim3 added to the refined inliers
        int projection_added = 0;               // matches SearchByProjection added from the loop map points
        int total_matches = 0;                  // features of the current keyframe with a loop map point
        // the last CorrectLoop
        int correct_vertices = 0;               // keyframes in the pose graph
        int correct_tree_edges = 0;             // one per keyframe with a connected keyframe of smaller id
        int correct_covisibility_edges = 0;     // connected pairs of weight >= _min_essential_weight without a tree edge
        int correct_loop_edges = 0;             // 1
        vector<unsigned long> correct_left_out; // keyframes given that have no edge: untouched
        int correct_points_moved = 0;
        struct PoseGraphResult                  // ygz_pgo_result's fields
        {
            int status = 0, lm_iterations = 0, n_solves = 0, cg_iterations_total = 0, cg_capped = 0;
            double cost_initial = 0, cost_final = 0, lambda = 0;
        } pose_graph;
        // the last FuseLoop
        int fuse_current_replaced = 0;          // step 1: points of the current keyframe replaced by their loop map point
        int fuse_current_added = 0;             // step 1: loop map points given to a feature without a good point
        int fuse_targets = 0;                   // keyframes SearchFuseCandidates looked into
        int fuse_hits = 0;                      // its (keyframe, point) hits
        int fuse_replaced = 0;                  // step 3: points replaced
        int fuse_added = 0;                     // step 3: observations added
        int fuse_conflicts = 0;                 // matches and hits skipped: the loop point is already observed there, or is bad, or the feature holds another loop point
        int fuse_descriptors = 0;               // points whose _distinctive_desc was set
        int fuse_rows = 0;                      // keyframes whose covisibility was rewritten
        // the last GlobalBundleAdjustment
        int gba_poses = 0;                      // keyframes in the problem (the one with the smallest id is fixed)
        int gba_points = 0;                     // map points in it
        int gba_edges = 0;                      // observations
        int gba_points_left_out = 0;            // good map points with fewer than 2 observations among the poses: untouched
        struct GlobalBAResult                   // ygz_gba_result's fields
        {
            int status = 0, lm_iterations = 0, n_solves = 0, cg_iterations_total = 0, cg_capped = 0;
            double cost_initial = 0, cost_final = 0, lambda = 0;
        } global_ba;
    };

    // one action of FuseLoop: feature `feature` of keyframe `keyframe_id` now observes loop map point `loop_point_id`; `replaced_point_id`
    // is the point it held before (now bad), -1 when it held none
    struct FusedPair { unsigned long keyframe_id; int feature; unsigned long loop_point_id; long replaced_point_id; };

    // the pose graph of the last CorrectLoop that reached the solver, as it was handed over and as it came back
    struct PoseGraph
    {
        vector<unsigned long> keyframe_ids;     // per vertex, ascending
        vector<double> S, S_out;                // [N][8] qx qy qz qw tx ty tz s, world -> camera
        vector<uint8_t> fixed;                  // [N]
        vector<int32_t> edges;                  // [E][2] vertex indices (i, j)
        vector<double> M;                       // [E][8] ~ S_j o S_i^-1
    };

    // the problem of the last GlobalBundleAdjustment that reached the solver, as it was handed over and as it came back
    struct BundleProblem
    {
        vector<unsigned long> keyframe_ids;     // per pose, ascending
        vector<unsigned long> point_ids;        // per point, in the order of rule 2
        vector<double> poses, poses_out;        // [N][7] qx qy qz qw tx ty tz, world -> camera
        vector<uint8_t> fixed;                  // [N]
        vector<double> points, points_out;      // [L][3]
        vector<int32_t> edge_pose, edge_point;  // [E]
        vector<double> obs;                     // [E][2]
        double K4[4] = { 0, 0, 0, 0 };          // fx fy cx cy
        double huber_delta = 0;
    };

    // Optional, null by default: where DetectLoop computes, never what.  With a database attached the scores of step 2 and the common-word
    // counts and scores of step 3 come from ONE KeyFrameDatabase::Query of kf->_bow_vec for every keyframe the database holds, and from the host
    // functions, as without it, for every other keyframe (and for all of them when the query fails).  Every filter stays where it is and sees
    // the same numbers, so every return value, Stats field and later stage is identical with, without, or with a partly filled database --
    // provided the database holds each keyframe's current _bow_vec (it stores the vector as of Add).  Not owned; it outlives its use here.
    void SetKeyFrameDatabase(KeyFrameDatabase *db) { _kfdb = db; }
    KeyFrameDatabase *GetKeyFrameDatabase() const { return _kfdb; }

    // kf: a keyframe of the map with its covisibility (_connected_keyframe_weights); true when some loop candidate is consistent enough
    bool DetectLoop(Frame *kf, const vector<Frame *> &keyframes);
    bool DetectLoop(Frame *kf);             // every keyframe registered in Memory
    // the geometric check of the last DetectLoop's candidates; true when one of them is accepted
    bool ComputeSim3();
    // valid after a ComputeSim3() that returned true: GetMatches() seeds a per-feature match vector of the current keyframe,
    // SearchBySim3(current, matched, ..., S12, 7.5) widens it, the good map points of the matched keyframe and of its connected keyframes
    // (keyframes in _keyframe_id order, features in index order, each point once) are the loop map points, SearchByProjection(current, S_cw,
    // loop points, ..., 10) pulls them in; true when the matches reach _min_total_matches.  Changes nothing in the map.
    bool SearchLoopMapPoints();
    // valid once after a ComputeSim3() that returned true (SearchLoopMapPoints is not needed); otherwise false and nothing changes, a second
    // call for the same loop included.  Ties go by _keyframe_id, never by address.
    //  vertices: the keyframes given that are not bad, by id; one without an edge is left out and untouched (Stats::correct_left_out)
    //  estimate: the current keyframe GetCorrectedPose(); each keyframe connected to it (but the matched one) Sim3(T_iw T_wc) o S_cw; the
    //            others Sim3(T_iw)
    //  edges (i, j) with M = Sim3(T_jw T_iw^-1) of the poses before the correction; a pair is connected with the larger of the two weights
    //            the keyframes hold for each other: per keyframe i its connected keyframe j of smaller id with the largest weight (ties: the
    //            smaller id) -- no fallback to the previous id; then every connected pair of weight >= _min_essential_weight without such an
    //            edge, i the larger id; last the loop edge current -> matched with M = Sim3(T_mw) o S_cw^-1
    //  fixed:    the matched keyframe; _fix_scale is passed on
    //  one ygz_hip_pose_graph_optimize call; on an error or status failed: false, the map untouched
    //  poses:    T_iw <- (R, t / s) of every vertex but the fixed one
    //  points:   keyframes by id, features by index, each good point once: its reference keyframe r is that of the _obs entry with the lowest
    //            key that has a feature whose frame is a vertex (Matcher::PointAttributes' rule); P <- S_rw^-1 (T_rw P) with the new S_rw and
    //            the old T_rw, unless S_rw did not change; a point without such an entry stays
    bool CorrectLoop(const vector<Frame *> &keyframes);
    bool CorrectLoop();                     // every keyframe registered in Memory
    const PoseGraph &GetPoseGraph() const { return _pose_graph; }

    // ORB-SLAM2's MapPoint::Replace on this data model; pure host code.  Nothing happens when the two are equal or either is null.  For each
    // (id, f) of from->_obs in key order: when into->_obs has no entry for id, f->_mappoint = into and into->_obs[id] = f; otherwise
    // f->_mappoint = nullptr.  into's _cnt_found and _cnt_visible grow by from's; from->_bad = true and from->_obs is cleared.  Nothing is deleted.
    static void ReplaceMapPoint(MapPoint *from, MapPoint *into);
    // recounts the covisibility of `rows` on the device (ygz_hip_covisibility, in chunks of rows when rows x K is above its cell cap).  The
    // universe is the keyframes given that are not bad, once each, by id; the points are the good map points of their features, each once; a
    // point's list is its _obs keys that belong to the universe.  Each row keyframe of the universe is rewritten by Frame::UpdateConnections'
    // rules: nothing changes when it shares nothing; _connected_keyframe_weights holds every non-zero count; _cov_keyframes / _cov_weights the
    // counts >= 15, heaviest first, equal weights by the smaller id; when no count reaches 15 the single largest (the smaller id of equals),
    // and that keyframe gets AddConnection.  Returns the rows rewritten.
    int UpdateCovisibility(const vector<Frame *> &rows, const vector<Frame *> &keyframes);
    // valid once, after a CorrectLoop that returned true for a loop on which SearchLoopMapPoints() ran before that correction (afterwards the
    // revisit run's camera frames are rescaled and SearchLoopMapPoints can no longer run); in every other case false and nothing changes, a
    // second call for the same loop included.  Poses and point positions are never touched.
    //  1. current keyframe: for each feature i with GetCurrentMatchedPoints()[i] = L, L good, in index order: L already observed by the
    //     current keyframe -> a conflict; the feature's point q good and q != L -> ReplaceMapPoint(q, L); no good point -> the observation is added
    //  2. targets: the current keyframe and the keyframes connected to it (the larger of the two weights, as CorrectLoop) that are among the
    //     keyframes given, not bad, not the matched keyframe and not connected to it, by id; one SearchFuseCandidates(targets, Sim3(T_kw),
    //     GetLoopMapPoints(), _fuse_search_th) with the corrected poses at scale 1
    //  3. hits: keyframes by id, points by index, each re-checked against the map as it is now: L bad or already observed by k -> a conflict;
    //     the feature's point q null or bad -> the observation is added; q = L -> nothing; q itself a loop map point -> a conflict (left to local
    //     mapping); otherwise ReplaceMapPoint(q, L)
    //  4. Matcher::ComputeDistinctiveDescriptors over every loop map point that gained an observation, one device call
    //  5. UpdateCovisibility(touched, keyframes): the keyframes in which some feature's _mappoint changed and those that observe a point
    //     that gained an observation, by id
    bool FuseLoop(const vector<Frame *> &keyframes);
    bool FuseLoop();                        // every keyframe registered in Memory
    const vector<FusedPair> &GetFusedPairs() const { return _fused; }   // every action of the last FuseLoop, in order

    // callable at any time, no loop state needed.  Ties go by _keyframe_id, never by address.
    //  1. poses: the keyframes given that are not bad, once each, by id; the one with the smallest id is fixed (ORB-SLAM2's keyframe 0)
    //  2. points: the good map points of their features, keyframes by id, features by index, each point once; a point's edges are its _obs
    //     entries in key order whose feature is non-null and whose frame is a pose; the pixel is Feature::_pixel, the camera Frame::GetCamera()
    //  3. a point with fewer than 2 such edges is left out and untouched (Stats::gba_points_left_out)
    //  4. a free pose left without any edge: false, nothing changed
    //  5. one ygz_hip_global_ba call with _gba_iterations and _gba_huber_delta; on an error or status failed: false, the map untouched
    //  6. _TCW of every free pose and _pos_world of every included point are rewritten from the result; the fixed keyframe keeps its bits
    //  7. nothing else changes: no observation, no _bad flag, no covisibility, no outlier removal
    bool GlobalBundleAdjustment(const vector<Frame *> &keyframes);
    bool GlobalBundleAdjustment();          // every keyframe registered in Memory
    const BundleProblem &GetBundleProblem() const { return _bundle; }

    Frame *GetMatchedKeyframe() const { return _matched; }
    const Sim3 &GetSim3() const { return _S12; }                      // loop keyframe's camera -> current keyframe's camera
    const Sim3 &GetCorrectedPose() const { return _Scw; }             // S12 * T_2w
    const vector<pair<MapPoint *, MapPoint *>> &GetMatches() const { return _matches; }   // (current, loop) refined inlier pairs
    const vector<MapPoint *> &GetCurrentMatchedPoints() const { return _current_matched; }   // per feature of the current keyframe: its loop map point or nullptr (last SearchLoopMapPoints)
    const vector<MapPoint *> &GetLoopMapPoints() const { return _loop_points; }             // the loop map points it searched
    const Stats &GetStats() const { return _stats; }

private:
    typedef pair<std::set<unsigned long>, int> ConsistentGroup;      // keyframe ids, consistency
    vector<ConsistentGroup> _consistent_groups;
    vector<Frame *> _enough_consistent;
    map<unsigned long, double> _acc_score;
    Frame *_current = nullptr;
    unsigned long _last_loop_kf_id = 0;
    Matcher _matcher;
    KeyFrameDatabase *_kfdb = nullptr;
    Frame *_matched = nullptr;
    Sim3 _S12, _Scw;
    vector<pair<MapPoint *, MapPoint *>> _matches;
    vector<MapPoint *> _current_matched, _loop_points;
    bool _correctable = false;                                        // an accepted loop that no CorrectLoop has used yet
    bool _searched = false;                                           // SearchLoopMapPoints ran for that loop, before its correction
    bool _fusable = false;                                            // a corrected loop with such a search that no FuseLoop has used yet
    vector<FusedPair> _fused;
    PoseGraph _pose_graph;
    BundleProblem _bundle;
    Stats _stats;
};

}

#endif // YGZ_LOOP_CLOSING_H_
