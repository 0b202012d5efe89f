// ygz::KeyFrameDatabase (include/ygz/Algorithm/KeyFrameDatabase.h): nothing in the reference; ORB-SLAM2's KeyFrameDatabase on this data model
// over the device store of ygz_slam_amd/csrc/kfdb.hip.  A keyframe's BoW vector goes up once (ygz_hip_kfdb_add); a query is one
// ygz_hip_kfdb_query call for up to YGZ_KFDB_MAX_QUERIES vectors.  Error conventions of the other surfaces: a failed call logs and returns
// false, only a missing device throws.
#include "ygz/Algorithm/KeyFrameDatabase.h"
#include "ygz/hip/Runtime.h"
#include "ygz_hip.h"
#include <algorithm>

namespace ygz {

namespace {
// a BowVector as the ABI's arrays, appended; false when a word does not fit the ABI's int32
bool append(const DBoW3::BowVector &v, vector<int32_t> &word, vector<double> &weight)
{
    for (const auto &kv : v) {
        if (kv.first > 0x7FFFFFFFu) return false;
        word.push_back((int32_t)kv.first);
        weight.push_back(kv.second);
    }
    return true;
}
}

KeyFrameDatabase::~KeyFrameDatabase()
{
    if (_db) ygz_hip_kfdb_destroy(_db);
}

bool KeyFrameDatabase::Add(Frame *kf)
{
    if (!kf || kf->_bad || Has(kf)) return false;
    if (kf->_bow_vec.empty()) kf->ComputeBoW();
    if (kf->_bow_vec.empty() || kf->_bow_vec.size() > (size_t)YGZ_KFDB_MAX_WORDS || _row.size() >= (size_t)YGZ_KFDB_MAX_ENTRIES) return false;
    vector<int32_t> word;
    vector<double> weight;
    if (!append(kf->_bow_vec, word, weight)) {
        LOG(ERROR) << "KeyFrameDatabase::Add: a word id above 2^31 - 1" << endl;
        return false;
    }
    if (!_db && !hip::check(ygz_hip_kfdb_create(hip::Runtime::Get().ctx(), &_db), "kfdb_create")) return false;
    int32_t entry = -1;
    if (!hip::check(ygz_hip_kfdb_add(_db, word.data(), weight.data(), (int)word.size(), &entry), "kfdb_add")) return false;
    if ((size_t)entry != _row.size()) {                          // cannot happen: the rows are counted on both sides
        LOG(ERROR) << "KeyFrameDatabase::Add: row " << entry << " where " << _row.size() << " was expected" << endl;
        (void)ygz_hip_kfdb_erase(_db, entry);
        return false;
    }
    _row.push_back(kf);
    _entry[kf] = entry;
    return true;
}

bool KeyFrameDatabase::Erase(Frame *kf)
{
    auto it = _entry.find(kf);
    if (it == _entry.end()) return false;
    const bool ok = hip::check(ygz_hip_kfdb_erase(_db, it->second), "kfdb_erase");
    _row[it->second] = nullptr;
    _entry.erase(it);
    return ok;
}

void KeyFrameDatabase::Clear()
{
    if (_db) (void)hip::check(ygz_hip_kfdb_clear(_db), "kfdb_clear");
    _entry.clear();
    _row.clear();
}

bool KeyFrameDatabase::Query(const DBoW3::BowVector &v, vector<Hit> &hits)
{
    vector<vector<Hit>> all;
    const bool ok = Query(vector<const DBoW3::BowVector *>(1, &v), all);
    hits.clear();
    if (ok) hits.swap(all[0]);
    return ok;
}

bool KeyFrameDatabase::Query(const vector<const DBoW3::BowVector *> &vs, vector<vector<Hit>> &hits)
{
    hits.clear();
    for (const DBoW3::BowVector *v : vs)
        if (!v || v->size() > (size_t)YGZ_KFDB_MAX_WORDS) {
            LOG(ERROR) << "KeyFrameDatabase::Query: a null vector or one of more than " << YGZ_KFDB_MAX_WORDS << " words" << endl;
            return false;
        }
    hits.resize(vs.size());
    if (_entry.empty() || vs.empty()) return true;
    const size_t E = _row.size();
    vector<int32_t> off, word, common;
    vector<double> weight, score;
    for (size_t first = 0; first < vs.size(); first += YGZ_KFDB_MAX_QUERIES) {
        const size_t n = std::min(vs.size() - first, (size_t)YGZ_KFDB_MAX_QUERIES);
        off.assign(1, 0); word.clear(); weight.clear();
        for (size_t q = 0; q < n; ++q) {
            if (!append(*vs[first + q], word, weight)) {
                LOG(ERROR) << "KeyFrameDatabase::Query: a word id above 2^31 - 1" << endl;
                hits.clear();
                return false;
            }
            off.push_back((int32_t)word.size());
        }
        if (word.empty()) { word.push_back(0); weight.push_back(0.0); }          // every vector empty: the arrays must still exist
        common.assign(n * E, 0); score.assign(n * E, 0.0);
        if (!hip::check(ygz_hip_kfdb_query(_db, (int)n, off.data(), word.data(), weight.data(), common.data(), score.data()), "kfdb_query")) {
            hits.clear();
            return false;
        }
        for (size_t q = 0; q < n; ++q) {
            vector<Hit> &h = hits[first + q];
            for (size_t e = 0; e < E; ++e)
                if (_row[e] && common[q * E + e] > 0) h.push_back(Hit{ _row[e], common[q * E + e], score[q * E + e] });
            std::stable_sort(h.begin(), h.end(), [](const Hit &a, const Hit &b) { return a.kf->_keyframe_id < b.kf->_keyframe_id; });
        }
    }
    return true;
}

}  // namespace ygz
