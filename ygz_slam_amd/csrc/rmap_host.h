// The host-only logic of the resident map (rmap.hip): the check list of an upload, the validation of a delta (range,
// duplicates, finiteness) and the layouts of the map's three buffers.  Plain C++ without a HIP header: a host program can include it
// (tests/cpp/rmap_host.cpp drives it under the sanitizers).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "../../include/ygz_hip.h"
#include "ygz_blob.h"
#include "pose_block.h"                          // ygz_all_finite: the one finiteness check under csrc/
#include "lms_index.h"

// The checks of ygz_hip_map_upload before the context's: those of ygz_hip_local_map_select on the map's side, then those of
// ygz_hip_map_point_attributes, then those of ygz_hip_stereo_local_map_indexed on the map, each in its own order.  n_obs and n_rows are set
// once the offsets are known to be sound.
inline int ygz_rmap_check_arrays(const ygz_map_arrays *m, int *n_obs, int *n_rows)
{
    if (!m) return YGZ_E_INVALID;
    // selection
    if (!m->kf_bad || !m->offsets || !m->kf || !m->feat || (m->n_cov > 0 && !m->cov)) return YGZ_E_INVALID;
    if (m->n_keyframes < 1 || m->n_cov < 0 || m->n_points < 1) return YGZ_E_INVALID;
    if (m->n_keyframes > YGZ_LMS_MAX_KEYFRAMES || m->n_cov > YGZ_LMS_MAX_COV) return YGZ_E_CAPACITY;
    if (m->offsets[0] != 0) return YGZ_E_INVALID;
    bool big = false;
    for (int p = 0; p < m->n_points; ++p) {
        if (m->offsets[p + 1] < m->offsets[p]) return YGZ_E_INVALID;
        big = big || m->offsets[p + 1] - m->offsets[p] > YGZ_MAP_MAX_OBS_PER_POINT;
    }
    if (big || m->offsets[m->n_points] > YGZ_MAP_MAX_OBS) return YGZ_E_CAPACITY;
    for (int p = 0; p < m->n_points; ++p)
        for (int g = m->offsets[p]; g < m->offsets[p + 1]; ++g)
            if (m->kf[g] < 0 || m->kf[g] >= m->n_keyframes || (g > m->offsets[p] && m->kf[g] <= m->kf[g - 1]) || m->feat[g] < 0 ||
                m->feat[g] >= YGZ_LMS_FEAT_END)
                return YGZ_E_INVALID;
    for (size_t i = 0; i < (size_t)m->n_keyframes * (size_t)m->n_cov; ++i)
        if (m->cov[i] < -1 || m->cov[i] >= m->n_keyframes) return YGZ_E_INVALID;
    // attributes
    if (!m->centre || !m->pw || !m->a_offsets || !m->a_kf || !m->a_level || m->n_centres < 1) return YGZ_E_INVALID;
    if (m->n_centres > YGZ_MAP_MAX_KEYFRAMES || m->n_points > YGZ_MPA_MAX_POINTS) return YGZ_E_CAPACITY;
    if (m->a_offsets[0] != 0) return YGZ_E_INVALID;
    big = false;
    for (int p = 0; p < m->n_points; ++p) {
        if (m->a_offsets[p + 1] < m->a_offsets[p]) return YGZ_E_INVALID;
        big = big || m->a_offsets[p + 1] - m->a_offsets[p] > YGZ_MAP_MAX_OBS_PER_POINT;
    }
    if (big || m->a_offsets[m->n_points] > YGZ_MAP_MAX_OBS) return YGZ_E_CAPACITY;
    const int rows = m->a_offsets[m->n_points];
    for (int e = 0; e < rows; ++e)
        if (m->a_kf[e] < 0 || m->a_kf[e] >= m->n_centres || m->a_level[e] > 30) return YGZ_E_INVALID;
    if (!ygz_all_finite(m->centre, 3 * (size_t)m->n_centres) || !ygz_all_finite(m->pw, 3 * (size_t)m->n_points)) return YGZ_E_INVALID;
    // tracking: the points were checked above, the attributes are computed and finite by construction
    if (!m->pt_desc) return YGZ_E_INVALID;
    *n_obs = m->offsets[m->n_points];
    *n_rows = rows;
    return YGZ_OK;
}

// the rows of one array of a delta: every index in [0, limit) and none twice.  `seen` is the caller's, any size; it is left all zero
inline bool ygz_rmap_rows_ok(int n, const int32_t *idx, int limit, std::vector<uint8_t> &seen)
{
    if (n < 0 || (n > 0 && !idx)) return false;
    if ((int)seen.size() < limit) seen.assign((size_t)limit, 0);
    bool ok = true;
    int done = 0;
    for (; done < n && ok; ++done) {
        const int32_t i = idx[done];
        if (i < 0 || i >= limit || seen[(size_t)i]) { ok = false; break; }
        seen[(size_t)i] = 1;
    }
    for (int k = 0; k < done; ++k) seen[(size_t)idx[k]] = 0;             // the failing entry set nothing, or what an earlier one set
    return ok;
}

// the whole delta of ygz_hip_map_update against a map of P points, K keyframes and Kc centres
inline int ygz_rmap_check_delta(int P, int K, int Kc, int n_pt, const int32_t *pt_idx, const double *pw, int n_kf, const int32_t *kf_idx,
                                const uint8_t *kf_bad, int n_c, const int32_t *c_idx, const double *centre)
{
    std::vector<uint8_t> seen;
    if (!ygz_rmap_rows_ok(n_pt, pt_idx, P, seen) || !ygz_rmap_rows_ok(n_kf, kf_idx, K, seen) || !ygz_rmap_rows_ok(n_c, c_idx, Kc, seen))
        return YGZ_E_INVALID;
    if ((n_kf > 0 && !kf_bad) || (n_c > 0 && !centre)) return YGZ_E_INVALID;
    if (pw && !ygz_all_finite(pw, 3 * (size_t)n_pt)) return YGZ_E_INVALID;
    if (n_c > 0 && !ygz_all_finite(centre, 3 * (size_t)n_c)) return YGZ_E_INVALID;
    return YGZ_OK;
}

// ---- the layouts.  Offsets in bytes, every array at a multiple of 256 (YgzBlobLayout); a bad() layout overflowed
// the map itself: [0, in_end) goes up, [o_dmax, end) is written by k_mpa_attr
struct RmapStore {
    size_t o_kbad, o_pbad, o_has, o_cov, o_off, o_obs, o_koff, o_kpt, o_centre, o_pw, o_aoff, o_akf, o_alv, o_desc, in_end, o_dmax, o_nrm, o_state, end;
    bool bad;
    RmapStore(size_t K, size_t C, size_t P, size_t N, size_t Kc, size_t R)
    {
        YgzBlobLayout L;
        o_kbad = L.add(K); o_pbad = L.add(P); o_has = L.add(P); o_cov = L.add_n<int32_t>(K * C); o_off = L.add_n<int32_t>(P + 1);
        o_obs = L.add_n<int32_t>(N); o_koff = L.add_n<int32_t>(K + 1); o_kpt = L.add_n<int32_t>(N); o_centre = L.add_n<double>(3 * Kc);
        o_pw = L.add_n<double>(3 * P); o_aoff = L.add_n<int32_t>(P + 1); o_akf = L.add_n<int32_t>(R); o_alv = L.add_n<int32_t>(R);
        o_desc = L.add(32 * P); in_end = L.end;
        o_dmax = L.add_n<double>(P); o_nrm = L.add_n<double>(3 * P); o_state = L.add_n<int32_t>(P); end = L.end;
        bad = L.bad();
    }
};

// the rows of a delta: everything goes up
struct RmapDelta {
    size_t o_pidx, o_pw, o_desc, o_pbad, o_has, o_kidx, o_kbad, o_cidx, o_centre, end;
    bool bad;
    RmapDelta(size_t n_pt, bool pw, bool desc, bool pbad, bool has, size_t n_kf, size_t n_c)
    {
        YgzBlobLayout L;
        o_pidx = L.add_n<int32_t>(n_pt); o_pw = L.add_n<double>(pw ? 3 * n_pt : 0); o_desc = L.add(desc ? 32 * n_pt : 0);
        o_pbad = L.add(pbad ? n_pt : 0); o_has = L.add(has ? n_pt : 0); o_kidx = L.add_n<int32_t>(n_kf); o_kbad = L.add(n_kf);
        o_cidx = L.add_n<int32_t>(n_c); o_centre = L.add_n<double>(3 * n_c); end = L.end;
        bad = L.bad();
    }
};

// the selection and filter side of one resident tracking call: [0, in_end) goes up, [o_ref, back_end(..)) comes back, the rest stays
struct RmapCall {
    size_t o_foff, o_fpt, in_end, o_ref, o_nvot, o_nloc, o_npt, o_ncut, o_nrem, o_lkf, o_lpt, small_end, o_prior, prior_end, o_votes, out_end;
    size_t o_npt0, o_lpt0, o_fprior, o_rank, o_cnt, o_start, o_lft, o_moved, end;
    bool bad;
    RmapCall(size_t F, size_t K, size_t E, size_t MP, size_t cells)
    {
        YgzBlobLayout L;
        o_foff = L.add_n<int32_t>(F + 1); o_fpt = L.add_n<int32_t>(E); in_end = L.end;
        o_ref = L.add_n<int32_t>(F); o_nvot = L.add_n<int32_t>(F); o_nloc = L.add_n<int32_t>(F); o_npt = L.add_n<int32_t>(F);
        o_ncut = L.add_n<int32_t>(F); o_nrem = L.add_n<int32_t>(F); o_lkf = L.add_n<int32_t>(F * K); o_lpt = L.add_n<int32_t>(F * MP);
        small_end = L.end; o_prior = L.add_n<int32_t>(F * cells); prior_end = L.end; o_votes = L.add_n<int32_t>(F * K); out_end = L.end;
        o_npt0 = L.add_n<int32_t>(F); o_lpt0 = L.add_n<int32_t>(F * MP); o_fprior = L.add_n<int32_t>(E); o_rank = L.add_n<uint16_t>(F * K);
        o_cnt = L.add_n<int32_t>(F * K); o_start = L.add_n<int32_t>(F * (K + 1)); o_lft = L.add_n<int32_t>(F * MP);
        o_moved = L.add_n<int32_t>(F * MP); end = L.end;
        bad = L.bad();
    }
    size_t back_end(bool votes, bool prior) const { return votes ? out_end : prior ? prior_end : small_end; }
};

// ygz_scratch's growth rule: a quarter more than asked for, and 256 bytes
inline size_t ygz_rmap_grown(size_t bytes) { return bytes + bytes / 4 + 256; }
