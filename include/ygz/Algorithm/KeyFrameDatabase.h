// ygz/Algorithm/KeyFrameDatabase.h -- ygz::KeyFrameDatabase: the BoW vectors of the map's keyframes resident in HBM and the place-recognition
// query that starts relocalisation and loop detection.  Nothing in the reference (its relocalisation and loop detection are stubs); it follows
// ORB-SLAM2's KeyFrameDatabase on this data model, without the inverted file: one device call (ygz_hip_kfdb_query) gives the number of common
// words and the L1 score (DBoW3::L1Scoring::score, what DBoW3::Vocabulary::score returns) of up to 64 query vectors against every keyframe
// held, bit-identical to common words counted and Vocabulary::score called per keyframe on the host (ygz_slam_amd/host/ygz_kfdb.cpp).
//
// Attaching one to LoopClosing or Relocalizer (SetKeyFrameDatabase) is optional and changes no result, only where the scores are computed.
// The database holds each keyframe's _bow_vec AS OF Add: a caller that recomputes a keyframe's _bow_vec calls Erase and Add again, and a
// keyframe that is deleted or set bad is erased first.  Ties go by _keyframe_id, never by address.  Error conventions of the
// other surfaces: a failed call logs and returns false or 0, only a missing device throws.  One thread at a time, like every class surface.
#ifndef YGZ_KEYFRAME_DATABASE_H_
#define YGZ_KEYFRAME_DATABASE_H_

#include "ygz/Basic.h"

struct ygz_kfdb;

namespace ygz
{

class KeyFrameDatabase
{
public:
    struct Hit { Frame *kf; int common; double score; };

    KeyFrameDatabase() {}
    ~KeyFrameDatabase();
    KeyFrameDatabase(const KeyFrameDatabase &) = delete;
    KeyFrameDatabase &operator=(const KeyFrameDatabase &) = delete;

    // stores kf->_bow_vec as it is now (ComputeBoW() first when it is empty).  false, with nothing changed: a null or bad keyframe, one already
    // held, a vector still empty after ComputeBoW(), a vector of more than YGZ_KFDB_MAX_WORDS (8192) words, a database that has taken
    // YGZ_KFDB_MAX_ENTRIES (4096) keyframes since its last Clear (an Erase gives no row back).
    bool Add(Frame *kf);
    bool Erase(Frame *kf);                          // false when kf is not held
    void Clear();                                   // forgets every keyframe; the row count starts again
    size_t Size() const { return _entry.size(); }   // keyframes held
    bool Has(const Frame *kf) const { return _entry.count(kf) != 0; }

    // every keyframe held that shares at least one word with v, by _keyframe_id: common = the shared words, score = Vocabulary::score(v, the
    // stored vector).  A keyframe held that is not among the hits shares nothing: Vocabulary::score would give 0 (as -0.0).  false (hits
    // empty) when the device call fails or v has more than 8192 words; an empty database answers true with no hits and no device call.
    bool Query(const DBoW3::BowVector &v, vector<Hit> &hits);
    // the same for many vectors, 64 per device call (larger batches go in chunks); hits[i] belongs to vs[i]; a null vector is refused
    bool Query(const vector<const DBoW3::BowVector *> &vs, vector<vector<Hit>> &hits);

private:
    ygz_kfdb *_db = nullptr;                        // created by the first Add
    map<const Frame *, int> _entry;                 // keyframe -> row (lookups only: nothing is ordered by it)
    vector<Frame *> _row;                           // row -> keyframe, nullptr once erased
};

}

#endif // YGZ_KEYFRAME_DATABASE_H_
