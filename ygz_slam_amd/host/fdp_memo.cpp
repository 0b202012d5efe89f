// FindDirectProjection behind its per-candidate callers.
// LocalMapping::ProjectMapPoints calls Matcher::FindDirectProjection once per candidate (src/Module/LocalMapping.cpp:88-118, 1000-3800 calls per
// frame) and CreateNewMapPoints once per matched feature pair (:447).  One call = upload, launch, download, synchronise: ~40 us, i.e. tens of
// milliseconds per frame.  FindDirectProjection is a pure function of (both images, both poses, the reference observation, the map point's
// position / the feature's depth, the prediction), so the first call of a current frame that misses runs ONE launch over every candidate the caller
// can be expected to ask about (below) and keeps the answers; the calls that follow are a table look-up.  An answer is handed out only when every
// input of the call equals the memoised one BIT FOR BIT -- anything else takes the n = 1 launch --, so results are identical to n = 1 calls
// (tests/test_gpu_surface.py: the per-candidate loop with YGZ_FDP_MEMO=0 against the default).
//
// What is speculated, MapPoint overload: for the keyframe `ref` of the call and every keyframe the previous current frame asked about, every
// feature of the keyframe that observes a good map point (mp->_obs[ref->_keyframe_id]), with the prediction FindCandidates makes
// (Camera2Pixel(World2Camera(mp->_pos_world, curr->_TCW)), LocalMapping.cpp:58-59, evaluated by the launch itself and compared with the caller's).
// A keyframe that was not covered gets its own launch on its first miss.  Feature overload: the matches the same Matcher object's last
// SearchForTriangulation(ref, curr, ...) returned, with the depth and prediction CreateNewMapPoints forms from them (LocalMapping.cpp:416-446).
#include "fdp_memo.h"
#include "ygz/Algorithm.h"
#include "ygz_hip.h"
#include <chrono>
#include <cstdlib>
#include <cstring>

namespace ygz {
namespace hip {
namespace {
inline bool same7(const SE3 &T, const double t7[7])
{ return memcmp(T.so3_.q_, t7, 32) == 0 && memcmp(T.t_, t7 + 4, 24) == 0; }
inline bool env_on(const char *name, bool dflt) { const char *e = getenv(name); return e ? atoi(e) != 0 : dflt; }
inline size_t hash(const Frame *ref, const void *key)
{ uint64_t h = (uint64_t)(uintptr_t)key * 0x9E3779B97F4A7C15ull ^ (uint64_t)(uintptr_t)ref * 0xC2B2AE3D27D4EB4Full; return (size_t)(h ^ (h >> 29)); }
template <class R> const R *ref_in(const std::vector<R> &v, const Frame *f) { for (const R &r : v) if (r.f == f) return &r; return nullptr; }
// adds the wall time of its scope to a total in milliseconds
struct ScopedMs {
    double &acc; std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    ~ScopedMs() { acc += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};
}  // namespace

FdpMemo::FdpMemo() : enabled(env_on("YGZ_FDP_MEMO", true)) {}
void FdpMemo::clear() { curr = nullptr; refs.clear(); feat_refs.clear(); entries.clear(); table.clear(); pend.ent.clear(); }   // (pre survives: it belongs to the frame about to begin)
void FdpMemo::restart(Frame *c) { clear(); curr = c; c->_TCW.to7(T_cur); }
// a new current frame (or the same one with another pose): the answers of the last one are void, the keyframes it named are the guess
void FdpMemo::begin(Frame *c) { if (!asked.empty()) asked_prev.swap(asked); asked.clear(); restart(c); }
bool FdpMemo::valid_for(const Frame *c) const { return curr == c && same7(c->_TCW, T_cur); }
// the Ref of keyframe f in v; a keyframe that moved since it was speculated on (local BA) voids every answer: the memo restarts for c
const FdpMemo::Ref *FdpMemo::unmoved(const std::vector<Ref> &v, const Frame *f, Frame *c)
{
    const Ref *R = ref_in(v, f);
    if (R && !same7(f->_TCW, R->T)) { restart(c); R = nullptr; }
    return R;
}
void FdpMemo::note_asked(Frame *f) { for (Frame *a : asked) if (a == f) return; asked.push_back(f); }
void FdpMemo::forget(const Frame *f)
{
    for (std::vector<Frame *> *v : { &asked, &asked_prev }) v->erase(std::remove(v->begin(), v->end(), f), v->end());
    pre.valid = false;
    if (curr == f || ref_in(refs, f) || ref_in(feat_refs, f)) clear();
}

void FdpMemo::build_table(const std::vector<Entry> &ent, std::vector<int32_t> &tab)
{
    size_t cap = 64;
    while (cap < 2 * ent.size() + 2) cap <<= 1;
    tab.assign(cap, -1);
    for (size_t i = 0; i < ent.size(); ++i) {
        size_t h = hash(ent[i].ref, ent[i].key) & (cap - 1);
        while (tab[h] >= 0) h = (h + 1) & (cap - 1);
        tab[h] = (int32_t)i;
    }
}
const FdpMemo::Entry *FdpMemo::find(const Frame *ref, const void *key) const
{
    if (table.empty()) return nullptr;
    const size_t mask = table.size() - 1;
    for (size_t h = hash(ref, key) & mask; table[h] >= 0; h = (h + 1) & mask) {
        const Entry &e = entries[table[h]];
        if (e.ref == ref && e.key == key) return &e;
    }
    return nullptr;
}
// the one look-up of both overloads: the answer memoised for (R's keyframe, key) when the call's inputs equal the speculated ones bit for bit -- a (the map
// point's position | the feature's depth, 0, 0), the observation's pixel and level, the caller's prediction
bool FdpMemo::serve(const Ref *R, const void *key, const double a[3], const Feature *obs, Vector2d &px_curr, int &search_level, bool &ok)
{
    const Entry *e = R ? find(R->f, key) : nullptr;
    if (!(e && e->a[0] == a[0] && e->a[1] == a[1] && e->a[2] == a[2] && e->px_ref[0] == obs->_pixel[0] && e->px_ref[1] == obs->_pixel[1]
          && e->level == obs->_level && e->px_in[0] == px_curr[0] && e->px_in[1] == px_curr[1])) {
        st.single++;
        return false;
    }
    st.hits++;
    px_curr = Vector2d(e->px_out[0], e->px_out[1]); search_level = e->sl; ok = e->ok != 0;
    return true;
}

// the answers of one launch over the candidates `ent` become entries of the table.  tab: the hash table over all of `ent`, built ahead -- adopted when the
// memo holds nothing yet (a candidate FindCandidates drops keeps its NaN prediction); otherwise only the candidates in view are appended
void FdpMemo::absorb(std::vector<Entry> &ent, const Answers &A, std::vector<int32_t> *tab)
{
    st.launches++; st.speculated += ent.size();
    for (size_t i = 0; i < ent.size(); ++i)
        if (A.vis[i]) ent[i].answer(&A.proj[2 * i], &A.out[2 * i], A.sl[i], A.ok[i]);    // FindCandidates drops the others (LocalMapping.cpp:60-63): nobody asks
    if (tab && entries.empty()) { entries.swap(ent); table.swap(*tab); return; }
    entries.reserve(entries.size() + ent.size());
    for (size_t i = 0; i < ent.size(); ++i) if (A.vis[i]) entries.push_back(ent[i]);
    build_table(entries, table);
}
// pure host work, no call into the context: every observation of a good map point in the keyframes of `batch` that hold an image (`skip_covered`: and
// are not in the table yet), with the keyframes' poses and the HBM slots they sit in as of now
void FdpMemo::gather(const Frame *curr, const std::vector<Frame *> &batch, bool skip_covered, Gathered &G) const
{
    G.reset();
    const int levels = curr->_option._pyramid_level;
    for (Frame *r : batch)
        if (r != curr && !r->_pyramid.empty() && !(skip_covered && ref_in(refs, r)) && std::find(G.kfs.begin(), G.kfs.end(), r) == G.kfs.end()) G.kfs.push_back(r);
    for (size_t k = 0; k < G.kfs.size(); ++k) {
        Frame *r = G.kfs[k];
        G.kf_slot.push_back(r->_hip_slot); double t7[7]; r->_TCW.to7(t7); G.kf_T.insert(G.kf_T.end(), t7, t7 + 7);
        const size_t n0 = r->_features.size();
        G.ck.reserve(G.ck.size() + n0); G.cl.reserve(G.cl.size() + n0); G.pos.reserve(G.pos.size() + 3 * n0); G.cpx.reserve(G.cpx.size() + 2 * n0); G.ent.reserve(G.ent.size() + n0);
        for (const Feature *f : r->_features) {
            const MapPoint *mp = f->_mappoint;
            if (!mp || mp->_bad) continue;
            // (whether f is the Feature the method reads, mp->_obs[ref->_keyframe_id] (Matcher.cpp:361), is settled at look-up time by comparing
            // pixel and level: a tree look-up per feature here was a third of the gather)
            if (f->_level < 0 || f->_level >= levels) continue;
            G.ck.push_back((int32_t)k); G.cl.push_back(f->_level);
            G.pos.push_back(mp->_pos_world[0]); G.pos.push_back(mp->_pos_world[1]); G.pos.push_back(mp->_pos_world[2]);
            G.cpx.push_back(f->_pixel[0]); G.cpx.push_back(f->_pixel[1]);
            G.ent.emplace_back(r, mp, mp->_pos_world.data(), f->_pixel.data(), f->_level);
        }
    }
}
// the gathered candidates against `curr` in one launch, into the memo.  defer: the launch is queued and collected at the first look-up (the caller's own
// FindCandidates runs in between)
void FdpMemo::launch(Frame *curr, Gathered &G, bool defer)
{
    Runtime &rt = Runtime::Get();
    if (G.kfs.empty() || curr->_pyramid.empty()) return;
    const int cs = rt.Resident(curr);
    for (size_t k = 0; k < G.kfs.size(); ++k) if (rt.Resident(G.kfs[k]) != G.kf_slot[k] || G.kf_slot[k] < 0) return;   // (not resident when gathered, or more keyframes than HBM slots: no speculation)
    if (curr->_hip_slot != cs) return;
    for (size_t k = 0; k < G.kfs.size(); ++k) if (G.kfs[k]->_hip_slot != G.kf_slot[k]) return;
    const size_t first_ref = refs.size();
    for (size_t k = 0; k < G.kfs.size(); ++k) { Ref R; R.f = G.kfs[k]; memcpy(R.T, &G.kf_T[7 * k], 56); refs.push_back(R); }
    const int n = (int)G.ck.size();
    if (n == 0) return;
    if (defer) {
        if (ygz_hip_find_direct_projection_mp_begin(rt.ctx(), cs, T_cur, (int)G.kfs.size(), G.kf_slot.data(), G.kf_T.data(), n, G.ck.data(), G.pos.data(), G.cpx.data(),
                                                    G.cl.data()) != YGZ_OK) { refs.resize(first_ref); return; }
        pend.ent.swap(G.ent); pend.tab.swap(G.tab);
        return;
    }
    Answers A(n);
    if (ygz_hip_find_direct_projection_mp(rt.ctx(), cs, T_cur, (int)G.kfs.size(), G.kf_slot.data(), G.kf_T.data(), n, G.ck.data(), G.pos.data(), G.cpx.data(),
                                          G.cl.data(), nullptr, A.vis.data(), A.proj.data(), A.ok.data(), A.out.data(), A.sl.data()) != YGZ_OK) {
        refs.resize(first_ref);                                        // nothing learnt; the calls take the n = 1 path (and report the error there)
        return;
    }
    absorb(G.ent, A);
}
// the queued launch, waited for and turned into table entries (first look-up of the frame)
void FdpMemo::collect()
{
    ScopedMs clock{ st.speculate_ms };
    Answers A(pend.ent.size());
    if (ygz_hip_find_direct_projection_mp_end(Runtime::Get().ctx(), (int)pend.ent.size(), A.vis.data(), A.proj.data(), A.ok.data(), A.out.data(), A.sl.data()) == YGZ_OK)
        absorb(pend.ent, A, &pend.tab);
    else refs.clear();                         // (another _begin took its place, or the run failed): nothing learnt -- the queued launch is the frame's first
    pend.ent.clear();
}

// Queue the frame's speculative launch as soon as its pose is known -- the end of Matcher::SparseImageAlignment -- when the previous current frame was
// served per candidate (an unchanged caller: Tracker -> LocalMapping::TrackLocalMap, LocalMapping.cpp:24-33).  LocalMapping::FindCandidates (0.2 ms of the
// caller's std::map work per frame) then runs while the device evaluates the candidates; a caller that changes the pose afterwards, or asks about other
// keyframes, falls back to the launch at its first call.  The candidates are gathered, and their table built, by the wait hook of the alignment
// (called by ygz_hip_sparse_align between its launch and its wait): they do not depend on the pose being estimated.
void FdpMemo::pregather(Frame *curr, const std::vector<Frame *> &batch)
{
    pre.valid = false; pre.curr = curr; pre.batch = batch;
    gather(curr, pre.batch, false, pre);
    build_table(pre.ent, pre.tab);
    pre.valid = true;
}
void FdpMemo::pregather_hook(void *curr)
{ FdpMemo &M = Runtime::Get().Fdp(); ScopedMs clock{ M.st.speculate_ms }; M.pregather(static_cast<Frame *>(curr), M.asked); }
bool FdpMemo::prelaunch_wanted(Frame *curr) const { return enabled && !bypass && !asked.empty() && !valid_for(curr); }
void FdpMemo::prelaunch(Frame *curr)
{
    if (!prelaunch_wanted(curr)) { pre.valid = false; return; }
    ScopedMs clock{ st.speculate_ms };
    begin(curr);
    if (!(pre.valid && pre.curr == curr && pre.batch == asked_prev)) pregather(curr, asked_prev);   // (the hook did not run: now)
    pre.valid = false;
    launch(curr, pre, true);
}

// Feature overload: the pairs the same Matcher's last SearchForTriangulation(ref, curr, ...) returned, with the depth and prediction
// LocalMapping::CreateNewMapPoints forms from them before it calls (src/Module/LocalMapping.cpp:405-447): both features without a map point, rays not
// parallel (cos < 0.9998), DepthFromTriangulation(T12^-1, pt1, pt2) positive -> fea1->_depth = depth1, prediction = fea2->_pixel.  One launch; a call is
// answered only if its feature, depth and prediction equal the speculated ones bit for bit.
void FdpMemo::speculate_feat(Frame *ref, Frame *curr, const vector<pair<int, int>> &pairs)
{
    ScopedMs clock{ st.speculate_ms };
    Runtime &rt = Runtime::Get();
    PinholeCamera *cam = Frame::_camera;
    Ref R; R.f = ref; ref->_TCW.to7(R.T);
    feat_refs.push_back(R);
    if (!cam || pairs.empty() || ref->_pyramid.empty() || curr->_pyramid.empty()) return;
    const int levels = curr->_option._pyramid_level;
    const SE3 T12 = ref->_TCW * curr->_TCW.inverse(), T21 = T12.inverse();
    std::vector<Entry> ent; std::vector<double> pr, dep, pc; std::vector<int32_t> lvl;
    for (const auto &pq : pairs) {
        if (pq.first < 0 || pq.second < 0 || pq.first >= (int)ref->_features.size() || pq.second >= (int)curr->_features.size()) continue;
        const Feature *fea1 = ref->_features[pq.first], *fea2 = curr->_features[pq.second];
        if (fea1->_mappoint || fea2->_mappoint || fea1->_level < 0 || fea1->_level >= levels) continue;
        const Vector3d pt1 = cam->Pixel2Camera(fea1->_pixel), pt2 = cam->Pixel2Camera(fea2->_pixel);
        if (pt1.dot(pt2) / (pt1.norm() * pt2.norm()) >= 0.9998) continue;
        double d1 = 0, d2 = 0;
        if (!cvutils::DepthFromTriangulation(T21, pt1, pt2, d1, d2) || d1 < 0 || d2 < 0) continue;
        const double a[3] = { d1, 0, 0 }; ent.emplace_back(ref, fea1, a, fea1->_pixel.data(), fea1->_level);
        dep.push_back(d1); lvl.push_back(fea1->_level);
        pr.push_back(fea1->_pixel[0]); pr.push_back(fea1->_pixel[1]); pc.push_back(fea2->_pixel[0]); pc.push_back(fea2->_pixel[1]);
    }
    const int n = (int)ent.size();
    if (n == 0) return;
    ygz_align_pair pair;
    pair.ref_slot = rt.Resident(ref); pair.cur_slot = rt.Resident(curr);
    if (ref->_hip_slot != pair.ref_slot || pair.ref_slot < 0 || pair.cur_slot < 0) return;
    memcpy(pair.T_ref, R.T, 56); memcpy(pair.T_cur, T_cur, 56);
    Answers A(n); A.vis.assign(n, 1); A.proj = pc; A.out = pc;                  // every pair is asked about; out: in/out, the prediction first
    if (ygz_hip_find_direct_projection(rt.ctx(), &pair, pr.data(), dep.data(), lvl.data(), A.out.data(), A.sl.data(), A.ok.data(), n) != YGZ_OK) return;
    absorb(ent, A);
}

bool FdpMemo::answer_mp(Frame *ref, Frame *curr, const MapPoint *mp, const Feature *obs, Vector2d &px_curr, int &search_level, bool &ok)
{
    if (!enabled || bypass) return false;
    if (!valid_for(curr)) begin(curr);
    if (!pend.ent.empty()) collect();                                  // the launch Matcher::SparseImageAlignment queued for this frame
    note_asked(ref);
    const Ref *R = unmoved(refs, ref, curr);
    if (!R) {                                                          // a keyframe not covered yet: its own launch (with the previous frame's, if the table is empty)
        ScopedMs clock{ st.speculate_ms };
        std::vector<Frame *> batch(1, ref);
        if (refs.empty()) batch.insert(batch.end(), asked_prev.begin(), asked_prev.end());
        Gathered G;
        gather(curr, batch, true, G);
        launch(curr, G, false);
        R = ref_in(refs, ref);
    }
    return serve(R, mp, mp->_pos_world.data(), obs, px_curr, search_level, ok);
}
bool FdpMemo::answer_feat(Frame *ref, Frame *curr, const Feature *fea_ref, const vector<pair<int, int>> &tri_pairs, Vector2d &px_curr, int &search_level, bool &ok)
{
    if (!enabled || bypass) return false;
    if (!valid_for(curr)) begin(curr);
    const Ref *R = unmoved(feat_refs, ref, curr);
    if (!R) { speculate_feat(ref, curr, tri_pairs); R = ref_in(feat_refs, ref); }
    const double a[3] = { fea_ref->_depth, 0, 0 };
    return serve(R, fea_ref, a, fea_ref, px_curr, search_level, ok);
}

void SetFdpSpeculation(bool on) { FdpMemo &M = Runtime::Get().Fdp(); M.enabled = on; if (!on) M.clear(); }
void SetFdpBypass(bool on) { Runtime::Get().Fdp().bypass = on; }
FdpMemoStats GetFdpMemoStats() { return Runtime::Get().Fdp().st; }
void ResetFdpMemoStats() { Runtime::Get().Fdp().st = FdpMemoStats(); }
}  // namespace hip
}  // namespace ygz
