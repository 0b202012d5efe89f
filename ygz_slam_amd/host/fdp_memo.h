// ygz::hip::FdpMemo -- Matcher::FindDirectProjection behind its per-candidate callers (fdp_memo.cpp).  Private to libygz_host.so: one instance,
// a member of the Runtime (Runtime::Fdp()), used by one thread at a time like the rest of the Runtime.
#ifndef YGZ_HOST_FDP_MEMO_H_
#define YGZ_HOST_FDP_MEMO_H_
#include "ygz/Basic.h"
#include "ygz/hip/Runtime.h"
#include <limits>
namespace ygz {
namespace hip {
class FdpMemo {
public:
    FdpMemo();
    // the two overloads of Matcher::FindDirectProjection: true = answered from the memo (px_curr, search_level, ok written), false = the caller takes
    // the n = 1 launch.  obs: the map point's observation in `ref`; tri_pairs: the pairs of the Matcher's last SearchForTriangulation(ref, curr, ...)
    bool answer_mp(Frame *ref, Frame *curr, const MapPoint *mp, const Feature *obs, Vector2d &px_curr, int &search_level, bool &ok);
    bool answer_feat(Frame *ref, Frame *curr, const Feature *fea_ref, const vector<pair<int, int>> &tri_pairs, Vector2d &px_curr, int &search_level, bool &ok);
    // Matcher::SparseImageAlignment: whether the next frame's launch will be queued; the wait hook that gathers its candidates (user: the current
    // Frame); the launch itself, once the pose is known
    bool prelaunch_wanted(Frame *curr) const; static void pregather_hook(void *curr); void prelaunch(Frame *curr);
    void forget(const Frame *f);                       // a frame that is (re)initialised or deleted takes every answer that involves it along
    void clear();
    FdpMemoStats st;
    bool enabled;                                      // YGZ_FDP_MEMO (default 1), SetFdpSpeculation
    bool bypass = false;                               // calls take the n = 1 launch and leave the memo alone (A/B inside one loop)

private:
    struct Ref { Frame *f; double T[7]; };
    struct Entry {                                     // inputs (compared on every look-up) and answers of one candidate
        const Frame *ref; const void *key;             // key: the MapPoint (MapPoint overload) or the reference Feature (Feature overload)
        double a[3];                                   // mp->_pos_world | (fea->_depth, 0, 0)
        double px_ref[2]; int32_t level;
        double px_in[2] = { std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::quiet_NaN() };   // the prediction answered (no call equals NaN)
        double px_out[2] = { 0, 0 }; int32_t sl = 0; uint8_t ok = 0;
        Entry(const Frame *r, const void *k, const double *a3, const double *px, int32_t lvl)
            : ref(r), key(k), a{ a3[0], a3[1], a3[2] }, px_ref{ px[0], px[1] }, level(lvl) {}
        void answer(const double *in, const double *out, int32_t s, uint8_t o) { px_in[0] = in[0]; px_in[1] = in[1]; px_out[0] = out[0]; px_out[1] = out[1]; sl = s; ok = o; }
    };
    struct Answers {                                   // what one launch hands back per candidate
        std::vector<uint8_t> vis, ok; std::vector<double> proj, out; std::vector<int32_t> sl;
        explicit Answers(size_t n) : vis(n), ok(n), proj(2 * n), out(2 * n), sl(n) {}
    };
    struct Gathered {                                  // the candidates of some keyframes: everything a launch needs except the current frame's pose
        std::vector<Frame *> kfs; std::vector<int32_t> kf_slot; std::vector<double> kf_T;
        std::vector<int32_t> ck, cl; std::vector<double> pos, cpx;
        std::vector<Entry> ent; std::vector<int32_t> tab;   // their table entries (inputs only); the hash table over them when built ahead (pregather)
        void reset() { kfs.clear(); kf_slot.clear(); kf_T.clear(); ck.clear(); cl.clear(); pos.clear(); cpx.clear(); ent.clear(); tab.clear(); }
    };

    void begin(Frame *c); void restart(Frame *c); bool valid_for(const Frame *c) const; void note_asked(Frame *f);
    const Ref *unmoved(const std::vector<Ref> &v, const Frame *f, Frame *c);
    static void build_table(const std::vector<Entry> &ent, std::vector<int32_t> &tab);
    const Entry *find(const Frame *ref, const void *key) const;
    bool serve(const Ref *R, const void *key, const double a[3], const Feature *obs, Vector2d &px_curr, int &search_level, bool &ok);
    void absorb(std::vector<Entry> &ent, const Answers &A, std::vector<int32_t> *tab = nullptr);
    void gather(const Frame *curr, const std::vector<Frame *> &batch, bool skip_covered, Gathered &G) const;
    void pregather(Frame *curr, const std::vector<Frame *> &batch);
    void launch(Frame *curr, Gathered &G, bool defer);
    void collect();
    void speculate_feat(Frame *ref, Frame *curr, const vector<pair<int, int>> &pairs);

    Frame *curr = nullptr;
    double T_cur[7];
    std::vector<Ref> refs;                             // keyframes whose map-point candidates are in the table (MapPoint overload)
    std::vector<Ref> feat_refs;                        // keyframes whose triangulation candidates are in the table (Feature overload)
    std::vector<Entry> entries;
    std::vector<int32_t> table;                        // open addressing over (ref, key), -1 = free
    std::vector<Frame *> asked, asked_prev;            // keyframes the calls of this / the previous current frame named
    // a speculative launch that has been queued (ygz_hip_find_direct_projection_mp_begin) and not collected yet: its entries and their table
    struct Pending { std::vector<Entry> ent; std::vector<int32_t> tab; } pend;
    // candidates gathered while Matcher::SparseImageAlignment waited for its kernel (ygz_hip_set_wait_hook), for the launch that follows it
    struct Pre : Gathered { Frame *curr = nullptr; std::vector<Frame *> batch; bool valid = false; } pre;
};
}
}
#endif
