// ygz/Algorithm/Relocalizer.h -- ygz::Relocalizer: the way out of VO_LOST.  Nothing in the reference: it fills the stub at
// src/Module/VisualOdometry.cpp:101-104 ("try relocalization"), in the manner of ORB-SLAM2's Tracking::Relocalization -- BoW keyframe
// retrieval, Matcher::SearchByBoW against each candidate, P3P RANSAC of all candidates in one device call (ygz_hip_pnp_ransac), then
// ba::OptimizeCurrentPoseOnly on the inliers (ygz_slam_amd/host/ygz_reloc.cpp; the integration is in INTEGRATION.md).
// SetKeyFrameDatabase is optional: with a ygz::KeyFrameDatabase attached the retrieval's BoW scores come from one device query instead of one
// host walk per keyframe; every result is the same bit for bit (ygz/Algorithm/KeyFrameDatabase.h).
#ifndef YGZ_RELOCALIZER_H_
#define YGZ_RELOCALIZER_H_

#include "ygz/Basic.h"
#include "ygz/Algorithm/FeatureDetector.h"
#include "ygz/Algorithm/Matcher.h"

namespace ygz
{

class KeyFrameDatabase;

class Relocalizer
{
public:
    struct Option
    {
        int _max_candidates = 5;            // keyframes tried, best BoW score first (at most YGZ_PNP_MAX_PROBLEMS)
        double _min_score_ratio = 0.75;     // a candidate scores at least this fraction of the best score (and above 0)
        int _min_bow_matches = 15;          // SearchByBoW matches with a map point that a candidate needs
        int _ransac_iterations = 300;       // ORB-SLAM2 Tracking::Relocalization's values
        double _ransac_chi2 = 5.991;
        int _min_ransac_inliers = 10;
        int _min_final_inliers = 50;        // features left after the pose-only BA
        float _knn_ratio = 0.75f;           // SearchByBoW's ratio (the Matcher's own reads matcher.knnRatio through Get<int>: 0)
    } _option;

    struct Stats
    {
        int candidates = 0, pnp_problems = 0, ransac_inliers = 0, final_inliers = 0;
        vector<int> bow_matches;            // per candidate, in candidate order
    };

    // current: a frame after InitFrame() that holds no features yet; true when its pose was recovered against one of the keyframes.  On
    // success current->_features are the RANSAC inliers (map point set, after the pose-only BA), _TCW the refined pose and _ref_keyframe
    // the keyframe; on failure the features, _TCW and the map are as they were.  _bow_vec / _feature_vec are left empty in every case.
    bool Relocalize(Frame *current, const vector<Frame *> &keyframes);
    bool Relocalize(Frame *current);        // every keyframe registered in Memory

    // Optional, null by default: where Relocalize computes, never what.  With a database attached the BoW scores of the retrieval come from ONE
    // KeyFrameDatabase::Query of the frame's BoW vector for every keyframe the database holds, and from Vocabulary::score, as without it, for
    // every other keyframe (and for all of them when the query fails).  Every filter stays where it is and sees the same numbers: the outcome,
    // the pose and the Stats are identical with, without, or with a partly filled database -- provided the database holds each keyframe's
    // current _bow_vec (it stores the vector as of Add).  Not owned; it outlives its use here.
    void SetKeyFrameDatabase(KeyFrameDatabase *db) { _kfdb = db; }
    KeyFrameDatabase *GetKeyFrameDatabase() const { return _kfdb; }

    Frame *GetMatchedKeyframe() const { return _matched; }
    const Stats &GetStats() const { return _stats; }

private:
    KeyFrameDatabase *_kfdb = nullptr;
    FeatureDetector _detector;
    Matcher _matcher;
    Frame *_matched = nullptr;
    Stats _stats;
};

}

#endif // YGZ_RELOCALIZER_H_
