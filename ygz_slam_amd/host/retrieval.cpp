// hip::bow_candidates (retrieval.h): step 3 of ygz::Relocalizer::Relocalize, as it stood in ygz_reloc.cpp, for that class and for
// ygz::StereoRelocalizer::Candidates.
#include "retrieval.h"
#include "ygz/Algorithm/KeyFrameDatabase.h"
#include <algorithm>
#include <map>

namespace ygz {
namespace hip {

void bow_candidates(const Frame *current, const std::vector<Frame *> &keyframes, KeyFrameDatabase *db, int max_candidates,
                    double min_score_ratio, std::vector<Retrieved> &out)
{
    out.clear();
    // (an attached database answers for the keyframes it holds with one device query: the same numbers, KeyFrameDatabase.h)
    std::map<const Frame *, double> db_score;
    std::vector<KeyFrameDatabase::Hit> hits;
    const bool from_db = db && Frame::_vocab->scoring_ == 0 && db->Query(current->_bow_vec, hits);
    for (const KeyFrameDatabase::Hit &h : hits) db_score[h.kf] = h.score;
    for (Frame *kf : keyframes) {
        if (!kf || kf->_bad || kf == current) continue;
        Retrieved c;
        c.kf = kf;
        if (from_db && db->Has(kf)) {
            auto it = db_score.find(kf);
            c.score = it != db_score.end() ? it->second : -0.0 / 2.0;             // no shared word: what Vocabulary::score returns
        } else
            c.score = Frame::_vocab->score(current->_bow_vec, kf->_bow_vec);
        if (c.score > 0) out.push_back(c);
    }
    std::sort(out.begin(), out.end(), [](const Retrieved &a, const Retrieved &b) {
        return a.score != b.score ? a.score > b.score : a.kf->_keyframe_id < b.kf->_keyframe_id; });
    if (!out.empty()) {
        const double floor = min_score_ratio * out[0].score;
        size_t keep = 0;
        const size_t cap = (size_t)std::max(0, max_candidates);
        while (keep < out.size() && keep < cap && out[keep].score >= floor) ++keep;
        out.resize(keep);
    }
}

}  // namespace hip
}  // namespace ygz
