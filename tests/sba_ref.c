/* sba_ref.c -- restatement of the stereo bundle adjustment (ygz_slam_amd/csrc/sba.hip): the yardstick of tests/test_sba_ref.py and
 * tests/test_gpu_sba.py, and the frozen spec of DESIGN.md section 22.  The solver is gba_ref.c's (included below, unchanged): the same
 * Levenberg-Marquardt rules, the same Schur-complement PCG, the same summation orders.  New here are the edge model -- mono (u, v) and stereo
 * (u, v, uR) edges, the information 4^-level, g2o's Huber kernel on chi2 -- and the rounds: a round runs the LM loop from the current
 * estimate over the active edges, then every present edge is classified by a fresh evaluation without kernel.  Test infrastructure: plain
 * C99, built by tests/sba_ref.py with -O2 -ffp-contract=off -fno-fast-math, never linked into the product.  Only + - * / and sqrt.
 *
 *  - an absent edge (kind 0) or an inactive one (an outlier of the last classification) keeps its slot in every list and contributes exact
 *    zeros: residual, weight, cost term, both Jacobian blocks and Hpl are 0.0; it is never tested for being defined;
 *  - rows 0 and 1 of an edge are gb_edge_terms' in its operation order; a stereo edge adds r2 = uR - ((fx (x / z) + cx) - bf / z) with the
 *    Jacobian rows J2 = J0 + (-e y, e x, 0, 0, 0, -e) for the pose and J2 = J0 - e R[2][.] for the point, e = (bf / z) / z;
 *  - chi2 = w (r0^2 + r1^2) for a mono edge and w ((r0^2 + r1^2) + r2^2) for a stereo one; the stored weight is rho' w;
 *  - Hpl = weight ((J0^T J0 + J1^T J1) + J2^T J2), for a mono edge the two-row expression alone; the sums of Hll, bl, Hpp and bp add the
 *    third row's product of every edge, which is +0.0 for a mono one and changes no bit of a sum that starts at +0.0. */
#include "gba_ref.c"

#define SB_MAX_ROUNDS 4

/* the layouts of ygz_sba_params and ygz_sba_result (include/ygz_hip.h) */
typedef struct {
    int32_t max_iterations, max_trials, cg_max_iterations, cg_batch;
    double  cg_tol, min_rel_decrease;
    double  baseline, chi2_mono, chi2_stereo;
    int32_t rounds, robust_rounds, iterations[SB_MAX_ROUNDS];
} sb_params;

typedef struct {
    double  cost_initial[SB_MAX_ROUNDS], cost_final[SB_MAX_ROUNDS], lambda[SB_MAX_ROUNDS];
    int32_t rounds_run, launches;            /* launches: a count of the device's host driver, 0 here */
    int32_t status[SB_MAX_ROUNDS], lm_iterations[SB_MAX_ROUNDS], n_solves[SB_MAX_ROUNDS], cg_iterations[SB_MAX_ROUNDS], cg_capped[SB_MAX_ROUNDS],
            inliers[SB_MAX_ROUNDS];
} sb_result;

typedef struct {
    int n, nl, ne;
    const double *poses, *points, *obs;      /* [N][7], [L][3], [E][3] */
    const uint8_t *fixed;
    const int32_t *edge_pose, *edge_point;
    const uint8_t *kind;                     /* [E] 0 absent, 1 mono, 2 stereo */
    const int32_t *level;                    /* [E] */
    double fx, fy, cx, cy;
} sb_problem;

/* ---- one edge ------------------------------------------------------------------------------------------------------------------ */
/* on the device: ygz_level_weight (ygz_slam_amd/csrc/posemath_dev.h) */
double sb_weight(int level) { return 1.0 / (double)(1 << (2 * level)); }

/* r [3] (r2 = 0.0 for a mono edge), R and P; 0 when the edge is rejected */
int sb_residual(const double *T, const double *X, const double *ob, const double *K, double bf, int kind, double *R, double *P, double *r)
{
    r[2] = 0.0;
    if (!gb_residual(T, X, ob, K, R, P, r)) return 0;
    if (kind != 2) return 1;
    r[2] = ob[2] - ((K[0] * (P[0] / P[2]) + K[2]) - bf / P[2]);
    return fabs(r[2]) <= GB_DMAX;
}

double sb_chi2(const double *r, int kind, double w)
{
    double e2 = r[0] * r[0] + r[1] * r[1];
    if (kind == 2) e2 = e2 + r[2] * r[2];
    return w * e2;
}

/* g2o's RobustKernelHuber on chi2: d2 = delta^2 is chi2_mono or chi2_stereo */
void sb_robust(double chi2, int on, double d2, double delta, double *rho0, double *rho1)
{
    *rho0 = chi2; *rho1 = 1.0;
    if (on && chi2 > d2) {
        const double s = sqrt(chi2);
        *rho0 = 2.0 * s * delta - d2;
        *rho1 = delta / s;
    }
}

/* residual r [3], stored weight, cost term rho, Jp [3][6], Jl [3][3]; 0 (and zeros) when the edge is rejected.  d2 / delta: the edge kind's */
int sb_edge_terms(const double *T, const double *X, const double *ob, const double *K, double bf, int kind, int level, int robust, double d2,
                  double delta, double *r, double *wgt, double *rho, double *Jp, double *Jl)
{
    double R[9], P[3], w0, rho0;
    int ok = gb_edge_terms(T, X, ob, K, 0.0, r, &w0, &rho0, Jp, Jl);          /* rows 0 and 1 */
    r[2] = 0.0;
    for (int k = 0; k < 6; ++k) Jp[12 + k] = 0.0;
    for (int k = 0; k < 3; ++k) Jl[6 + k] = 0.0;
    if (ok) ok = sb_residual(T, X, ob, K, bf, kind, R, P, r);
    if (!ok) {
        r[0] = 0.0; r[1] = 0.0; r[2] = 0.0; *wgt = 0.0; *rho = 0.0;
        for (int k = 0; k < 18; ++k) Jp[k] = 0.0;
        for (int k = 0; k < 9; ++k) Jl[k] = 0.0;
        return 0;
    }
    if (kind == 2) {
        const double x = P[0], y = P[1], z = P[2], e = (bf / z) / z;
        Jp[12] = Jp[0] - e * y; Jp[13] = Jp[1] + e * x; Jp[14] = Jp[2]; Jp[15] = Jp[3]; Jp[16] = Jp[4]; Jp[17] = Jp[5] - e;
        for (int k = 0; k < 3; ++k) Jl[6 + k] = Jl[k] - e * R[6 + k];
    }
    const double w = sb_weight(level);
    double rho1;
    sb_robust(sb_chi2(r, kind, w), robust, d2, delta, rho, &rho1);
    *wgt = rho1 * w;
    return 1;
}

/* Hpl = weight Jp^T Jl, 6x3 row-major */
void sb_hpl(const double *Jp, const double *Jl, double wgt, int kind, double *H)
{
    for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 3; ++b) {
            const double two = Jp[a] * Jl[b] + Jp[6 + a] * Jl[3 + b];
            H[3 * a + b] = kind == 2 ? wgt * (two + Jp[12 + a] * Jl[6 + b]) : wgt * two;
        }
}

/* ---- the work ---------------------------------------------------------------------------------------------------------------------- */
typedef struct {
    gb_work W;                               /* gba_ref.c's, whose res, Jp and Jl stay unused */
    sb_problem pb;
    double bf, d2m, d2s, dm, ds;
    int robust;
    uint8_t *active;                         /* [E] */
    double *res, *Jp, *Jl;                   /* [E][3], [E][18], [E][9] */
} sb_work;

static void sb_zero_edge(sb_work *S, int e)
{
    gb_work *W = &S->W;
    for (int k = 0; k < 3; ++k) S->res[3 * (size_t)e + k] = 0.0;
    for (int k = 0; k < 18; ++k) S->Jp[18 * (size_t)e + k] = 0.0;
    for (int k = 0; k < 9; ++k) S->Jl[9 * (size_t)e + k] = 0.0;
    for (int k = 0; k < 18; ++k) W->Hpl[18 * (size_t)e + k] = 0.0;
    W->w[e] = 0.0; W->term[e] = 0.0;
}

/* residuals, weights, Jacobian blocks, Hpl and the cost at (T, X) over the active edges; 0 when an active edge is rejected */
static int sb_linearize_edges(sb_work *S, const double *T, const double *X, double *cost)
{
    gb_work *W = &S->W;
    const sb_problem *pb = &S->pb;
    int ok = 1;
    for (int e = 0; e < pb->ne; ++e) {
        if (!S->active[e]) { sb_zero_edge(S, e); continue; }
        const int kind = pb->kind[e];
        ok &= sb_edge_terms(T + 7 * pb->edge_pose[e], X + 3 * pb->edge_point[e], pb->obs + 3 * (size_t)e, W->K, S->bf, kind, pb->level[e], S->robust,
                            kind == 2 ? S->d2s : S->d2m, kind == 2 ? S->ds : S->dm, S->res + 3 * (size_t)e, W->w + e, W->term + e,
                            S->Jp + 18 * (size_t)e, S->Jl + 9 * (size_t)e);
        sb_hpl(S->Jp + 18 * (size_t)e, S->Jl + 9 * (size_t)e, W->w[e], kind, W->Hpl + 18 * (size_t)e);
    }
    *cost = gb_sum2(W->term, pb->ne);
    return ok && fabs(*cost) <= GB_DMAX;
}

/* the cost alone at (T, X) */
static int sb_cost(sb_work *S, const double *T, const double *X, double *cost)
{
    gb_work *W = &S->W;
    const sb_problem *pb = &S->pb;
    int ok = 1;
    for (int e = 0; e < pb->ne; ++e) {
        double R[9], P[3], r[3], rho1;
        W->term[e] = 0.0;
        if (!S->active[e]) continue;
        const int kind = pb->kind[e];
        if (!sb_residual(T + 7 * pb->edge_pose[e], X + 3 * pb->edge_point[e], pb->obs + 3 * (size_t)e, W->K, S->bf, kind, R, P, r)) { ok = 0; continue; }
        sb_robust(sb_chi2(r, kind, sb_weight(pb->level[e])), S->robust, kind == 2 ? S->d2s : S->d2m, kind == 2 ? S->ds : S->dm, W->term + e, &rho1);
    }
    *cost = gb_sum2(W->term, pb->ne);
    return ok && fabs(*cost) <= GB_DMAX;
}

/* gb_gather_system with three rows */
static void sb_gather_system(sb_work *S)
{
    gb_work *W = &S->W;
    const sb_problem *pb = &S->pb;
    for (int l = 0; l < pb->nl; ++l) {
        double h[6], g[3];
        for (int k = 0; k < 6; ++k) h[k] = 0.0;
        for (int k = 0; k < 3; ++k) g[k] = 0.0;
        for (int s = W->pt_off[l]; s < W->pt_off[l + 1]; ++s) {
            const int e = W->pt_adj[s];
            const double *J = S->Jl + 9 * (size_t)e, *r = S->res + 3 * (size_t)e, w = W->w[e];
            int m = 0;
            for (int a = 0; a < 3; ++a) {
                for (int b = a; b < 3; ++b) h[m++] += w * ((J[a] * J[b] + J[3 + a] * J[3 + b]) + J[6 + a] * J[6 + b]);
                g[a] += w * ((J[a] * r[0] + J[3 + a] * r[1]) + J[6 + a] * r[2]);
            }
        }
        for (int k = 0; k < 6; ++k) W->Hll[6 * (size_t)l + k] = h[k];
        for (int k = 0; k < 3; ++k) W->bl[3 * (size_t)l + k] = -g[k];
    }
    for (int v = 0; v < pb->n; ++v) {
        if (pb->fixed[v]) continue;
        double lane[27][GB_LANES];
        for (int ln = 0; ln < GB_LANES; ++ln) {
            double acc[27];
            for (int k = 0; k < 27; ++k) acc[k] = 0.0;
            for (int s = W->ps_off[v] + ln; s < W->ps_off[v + 1]; s += GB_LANES) {
                const int e = W->ps_adj[s];
                const double *J = S->Jp + 18 * (size_t)e, *r = S->res + 3 * (size_t)e, w = W->w[e];
                int m = 0;
                for (int a = 0; a < 6; ++a) {
                    for (int b = a; b < 6; ++b) acc[m++] += w * ((J[a] * J[b] + J[6 + a] * J[6 + b]) + J[12 + a] * J[12 + b]);
                    acc[21 + a] += w * ((J[a] * r[0] + J[6 + a] * r[1]) + J[12 + a] * r[2]);
                }
            }
            for (int k = 0; k < 27; ++k) lane[k][ln] = acc[k];
        }
        for (int k = 0; k < 21; ++k) W->Hpp[21 * v + k] = gb_tree(lane[k]);
        for (int k = 0; k < 6; ++k) W->bp[6 * v + k] = -gb_tree(lane[21 + k]);
    }
}

/* every present edge at (T, X) by a fresh evaluation without kernel; returns the inliers */
static int sb_classify(const sb_work *S, const double *T, const double *X, uint8_t *outlier, double *chi2)
{
    const sb_problem *pb = &S->pb;
    int inliers = 0;
    for (int e = 0; e < pb->ne; ++e) {
        const int kind = pb->kind[e];
        double R[9], P[3], r[3];
        if (kind == 0) { outlier[e] = 0; chi2[e] = -1.0; continue; }
        if (!sb_residual(T + 7 * pb->edge_pose[e], X + 3 * pb->edge_point[e], pb->obs + 3 * (size_t)e, S->W.K, S->bf, kind, R, P, r)) {
            outlier[e] = 1; chi2[e] = 0.0; continue;
        }
        const double c = sb_chi2(r, kind, sb_weight(pb->level[e]));
        outlier[e] = c > (kind == 2 ? S->d2s : S->d2m);
        chi2[e] = c;
        inliers += !outlier[e];
    }
    return inliers;
}

static void sb_work_init(sb_work *S, const sb_problem *pb, const sb_params *prm)
{
    memset(S, 0, sizeof *S);
    S->pb = *pb;
    gb_problem g;
    memset(&g, 0, sizeof g);
    g.n = pb->n; g.nl = pb->nl; g.ne = pb->ne; g.poses = pb->poses; g.points = pb->points; g.fixed = pb->fixed; g.edge_pose = pb->edge_pose;
    g.edge_point = pb->edge_point; g.fx = pb->fx; g.fy = pb->fy; g.cx = pb->cx; g.cy = pb->cy;
    gb_work_init(&S->W, &g);
    const size_t E = (size_t)pb->ne;
    S->bf = pb->fx * prm->baseline;
    S->d2m = prm->chi2_mono; S->d2s = prm->chi2_stereo; S->dm = sqrt(prm->chi2_mono); S->ds = sqrt(prm->chi2_stereo);
    S->active = (uint8_t *)calloc(E, 1);
    S->res = (double *)calloc(3 * E, sizeof(double)); S->Jp = (double *)calloc(18 * E, sizeof(double)); S->Jl = (double *)calloc(9 * E, sizeof(double));
}

static void sb_work_free(sb_work *S)
{
    gb_work_free(&S->W);
    free(S->active); free(S->res); free(S->Jp); free(S->Jl);
}

/* the stage: the linearisation at the input, every present edge active, the kernel on iff robust_rounds > 0.  res [E][3], w [E], Jp [E][18],
 * Jl [E][9], Hpp [N][21], bp [N][6], Hll [L][6], bl [L][3]; each may be NULL.  Returns 1 when every present edge is defined */
int sb_linearize(const sb_problem *pb, const sb_params *prm, double *res, double *w, double *Jp, double *Jl, double *Hpp, double *bp, double *Hll,
                 double *bl, double *cost)
{
    sb_work S;
    sb_work_init(&S, pb, prm);
    const size_t N = (size_t)pb->n, L = (size_t)pb->nl, E = (size_t)pb->ne;
    for (size_t e = 0; e < E; ++e) S.active[e] = pb->kind[e] != 0;
    S.robust = prm->robust_rounds > 0;
    const int ok = sb_linearize_edges(&S, S.W.T, S.W.X, cost);
    sb_gather_system(&S);
    if (res) memcpy(res, S.res, sizeof(double) * 3 * E);
    if (w) memcpy(w, S.W.w, sizeof(double) * E);
    if (Jp) memcpy(Jp, S.Jp, sizeof(double) * 18 * E);
    if (Jl) memcpy(Jl, S.Jl, sizeof(double) * 9 * E);
    if (Hpp) memcpy(Hpp, S.W.Hpp, sizeof(double) * 21 * N);
    if (bp) memcpy(bp, S.W.bp, sizeof(double) * 6 * N);
    if (Hll) memcpy(Hll, S.W.Hll, sizeof(double) * 6 * L);
    if (bl) memcpy(bl, S.W.bl, sizeof(double) * 3 * L);
    sb_work_free(&S);
    return ok;
}

/* the whole call; outlier [E] and chi2 [E] receive the last classification */
void sb_optimize(const sb_problem *pb, const sb_params *prm, double *poses_out, double *points_out, uint8_t *outlier, double *chi2, sb_result *out)
{
    sb_work S;
    sb_work_init(&S, pb, prm);
    gb_work *W = &S.W;
    memset(out, 0, sizeof *out);
    const size_t N = (size_t)pb->n, L = (size_t)pb->nl;
    int n_free = 0;
    for (int v = 0; v < pb->n; ++v) n_free += !pb->fixed[v];
    int cap = prm->cg_max_iterations;
    if (cap <= 0) cap = 6 * n_free < GB_CG_CAP ? 6 * n_free : GB_CG_CAP;
    for (int e = 0; e < pb->ne; ++e) outlier[e] = 0;

    for (int round = 0; round < prm->rounds; ++round) {
        for (int e = 0; e < pb->ne; ++e) S.active[e] = pb->kind[e] != 0 && !(round > 0 && outlier[e]);
        S.robust = round < prm->robust_rounds;
        /* gb_optimize's loop, from the current estimate, the counters of this round */
        double lambda = 0.0, ni = 2.0, currentChi = 0.0;
        int status = GB_MAX_ITERATIONS;
        for (int it = 0; it < prm->iterations[round]; ++it) {
            double cost;
            const int lin_ok = sb_linearize_edges(&S, W->T, W->X, &cost);
            if (it == 0) {
                if (!lin_ok) { status = GB_FAILED; break; }
                out->cost_initial[round] = cost;
            }
            currentChi = cost;
            sb_gather_system(&S);
            if (it == 0) {
                double mx = 0.0;
                for (int v = 0; v < pb->n; ++v) {
                    if (pb->fixed[v]) continue;
                    int m = 0;
                    for (int a = 0; a < 6; ++a) { const double h = fabs(W->Hpp[21 * v + m]); if (h > mx) mx = h; m += 6 - a; }
                }
                for (int l = 0; l < pb->nl; ++l) {
                    const int dg[3] = { 0, 3, 5 };
                    for (int a = 0; a < 3; ++a) { const double h = fabs(W->Hll[6 * (size_t)l + dg[a]]); if (h > mx) mx = h; }
                }
                lambda = 1e-5 * mx; ni = 2.0;
            }
            double rho = 0.0;
            int qmax = 0, converged = 0;
            do {
                int ok = gb_trial_system(W, lambda);
                double tempChi = GB_DMAX, scale = 0.0;
                if (ok) {
                    int capped = 0;
                    out->cg_iterations[round] += gb_cg(W, lambda, prm->cg_tol, cap, &capped);
                    out->cg_capped[round] += capped;
                    ++out->n_solves[round];
                    scale = gb_update(W, lambda);
                    ok = sb_cost(&S, W->Tn, W->Xn, &tempChi);
                    if (!ok) { tempChi = GB_DMAX; scale = 0.0; }
                }
                scale += 1e-3;
                rho = (currentChi - tempChi) / scale;
                if (!(fabs(rho) <= GB_DMAX)) rho = -1.0;
                if (ok && rho > 0) {
                    const double u = 2.0 * rho - 1.0;
                    double alpha = 1.0 - u * u * u;
                    if (alpha > 2.0 / 3.0) alpha = 2.0 / 3.0;
                    lambda = lambda * (alpha > 1.0 / 3.0 ? alpha : 1.0 / 3.0);
                    ni = 2.0;
                    converged = currentChi - tempChi <= prm->min_rel_decrease * currentChi;
                    currentChi = tempChi;
                    memcpy(W->T, W->Tn, sizeof(double) * 7 * N);
                    memcpy(W->X, W->Xn, sizeof(double) * 3 * L);
                } else {
                    lambda = lambda * ni; ni = ni * 2.0;
                    if (!(fabs(lambda) <= GB_DMAX)) break;
                }
                ++qmax;
            } while (rho < 0 && qmax < prm->max_trials);
            ++out->lm_iterations[round];
            if (qmax == prm->max_trials || rho == 0 || !(fabs(lambda) <= GB_DMAX)) { status = GB_STALLED; break; }
            if (converged) { status = GB_CONVERGED; break; }
        }
        out->status[round] = status;
        out->cost_final[round] = status == GB_FAILED ? 0.0 : currentChi;
        if (status == GB_FAILED) out->cost_initial[round] = 0.0;
        out->lambda[round] = lambda;
        out->inliers[round] = sb_classify(&S, W->T, W->X, outlier, chi2);
        out->rounds_run = round + 1;
        if (status == GB_FAILED) break;
    }
    memcpy(poses_out, W->T, sizeof(double) * 7 * N);                 /* a FAILED round moved nothing */
    memcpy(points_out, W->X, sizeof(double) * 3 * L);
    sb_work_free(&S);
}
