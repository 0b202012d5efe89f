// The BoW keyframe retrieval that ygz::Relocalizer and ygz::StereoRelocalizer share (retrieval.cpp).  Private to libygz_host.so like
// surface_share.h.  Host code; an attached ygz::KeyFrameDatabase answers with one device query.
#ifndef YGZ_HOST_RETRIEVAL_H_
#define YGZ_HOST_RETRIEVAL_H_
#include "ygz/Basic.h"
namespace ygz {
class KeyFrameDatabase;
namespace hip {
struct Retrieved { Frame *kf; double score; };
// the keyframes (null, _bad and `current` itself left out) whose _bow_vec scores above 0 against current->_bow_vec, best first, ties by
// keyframe id; at most max_candidates of them, each with at least min_score_ratio of the best score.  With a database (may be null, and only
// for a vocabulary with L1 scoring) the scores of the keyframes it holds come from ONE KeyFrameDatabase::Query, the others from
// Vocabulary::score: the same numbers
void bow_candidates(const Frame *current, const std::vector<Frame *> &keyframes, KeyFrameDatabase *db, int max_candidates,
                    double min_score_ratio, std::vector<Retrieved> &out);
}
}
#endif
