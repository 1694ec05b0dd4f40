// orbhip_pnp.hip — PnPsolver::iterate (PnPsolver.cc:165-258) for one solver or one round of several, in four launches: every drawn hypothesis of every
// problem is solved by EPnP (compute_pose, :477-525) and checked against all correspondences (CheckInliers, :308-339); the loop's bookkeeping over
// the counts gives the distinct best masks the loop can meet; each is refined (Refine, :260-305: EPnP over the mask's set bits, CheckInliers over all
// n); the first hypothesis, in order, whose then-current mask refines with more than min_inliers ends the call.  The arithmetic is DESIGN.md H18,
// restated in tests/pnp_model.py: +, -, *, / and sqrt in double, one rounding each, in the order written here; CheckInliers' mixed float and double.
//
//   k_pnp_hyp       one wave per (hypothesis, problem): pnp_epnp over the four drawn correspondences, then the check.
//   k_pnp_select    one wave per problem: 64 counts a pass, a prefix maximum by shuffles.  Lists the candidates: the carried-in mask if a hypothesis
//                   reaches the minimum before the first new maximum, then every strict new maximum that reaches the minimum.
//   k_pnp_refine    one wave per (candidate, problem): pnp_epnp over the set bits of the candidate's mask, then the check.
//   k_pnp_finish    one wave per problem: the first candidate, in order, with more than min_inliers refined inliers; the result record and the masks.
//
// pnp_epnp is one routine for both: a sum over the correspondences of a set is taken as 64 partial sums - partial l adds the set's positions
// l, l + 64, .. in rising order, from 0.0 - and the tree (p[l] + p[l ^ 32]), then ^ 16 .. ^ 1 (addition commutes, so every lane ends with lane 0's
// bits).  A position is the rank in the quadruple for a hypothesis and the correspondence's index for a mask; positions outside the set add nothing.
// The 12 x 12 and 3 x 3 eigenproblems are orbhip_jacobi_eigen_wave on LDS (2.8 KB a workgroup); the 6 x 10 system, the three beta solves,
// Gauss-Newton and the 3 x 3 singular value decomposition run uniformly on all lanes.
// No device state survives a call, no floating-point atomics, every loop is bounded by n, n_hyp or a constant whatever the numbers are: a non-finite
// pose fails every comparison and has 0 inliers.
#include "orbhip_ctx.h"
#include "orbhip_jacobi.h"
#include "orbhip_hestenes.h"

#define PNP_MAX_HYP 4096
#define PNP_REC 16                     // doubles per record: R[9] t[3] count(int) pad pad pad

struct PnpResult { int n_consumed, returned, best, best_inliers, refined_inliers, n_cand, ok_cand, pad; float best_Tcw[16], refined_Tcw[16]; };
struct PnpDev {
    const orbhip_pnp_corr* corr; const int* quads; const unsigned long long* mask_in; double* hyp; unsigned long long* mask;
    int* cand; int* cand_at; double* ref; unsigned long long* ref_mask; PnpResult* res; unsigned char* best_mask; unsigned char* refined_mask;
    int n, n_hyp, words, min_inliers, best_in, cand_cap;
    float K[4];
};
struct PnpLds { double A[12][12], V[12][12], L[6][10]; int ord[12]; };
// the correspondences of one EPnP: positions 0 .. range-1, of which those with their mask bit set (all, without a mask) take part; position r is
// correspondence list[r] (r itself, without a list); m of them in all, `first` the first
struct PnpSet { const orbhip_pnp_corr* corr; const int* list; const unsigned long long* mask; int range, m, first; };

template <int K, typename F> __device__ __forceinline__ void pnp_reduce(const PnpSet& S, int lane, double (&acc)[K], F f)
{
#pragma unroll
    for (int k = 0; k < K; k++) acc[k] = 0.0;
    for (int r = lane; r < S.range; r += 64) {
        if (S.mask && !((S.mask[r >> 6] >> (r & 63)) & 1ull)) continue;
        double v[K];
        f(S.corr[S.list ? S.list[r] : r], v);
#pragma unroll
        for (int k = 0; k < K; k++) acc[k] = acc[k] + v[k];
    }
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int k = 0; k < K; k++) acc[k] = acc[k] + __shfl_xor(acc[k], d);
    }
}

// lane 0 orders the diagonal of A descending by insertion with a strict `>` (equal values keep their index order); a barrier follows
template <int N> __device__ static void pnp_sort_desc(double (*A)[N], int* ord, int lane)
{
    if (lane == 0) {
        for (int i = 0; i < N; i++) ord[i] = i;
        for (int i = 1; i < N; i++)
            for (int j = i; j > 0 && A[ord[j]][ord[j]] > A[ord[j - 1]][ord[j - 1]]; j--) { const int o = ord[j]; ord[j] = ord[j - 1]; ord[j - 1] = o; }
    }
    __syncthreads();
}

__device__ __forceinline__ double pnp_dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// compute_barycentric_coordinates, one point
__device__ __forceinline__ void pnp_alphas(const orbhip_pnp_corr& c, const double ci[9], const double c0[3], double a[4])
{
    const double d0 = (double)c.Xw[0] - c0[0], d1 = (double)c.Xw[1] - c0[1], d2 = (double)c.Xw[2] - c0[2];
#pragma unroll
    for (int j = 0; j < 3; j++) a[1 + j] = (ci[3 * j] * d0 + ci[3 * j + 1] * d1) + ci[3 * j + 2] * d2;
    a[0] = ((1.0 - a[1]) - a[2]) - a[3];
}

// qr_solve (PnPsolver.cc:860-950) on a 6 x NC system, A row-major: Householder, b <- Q^T b, back substitution.  A zero column (eta == 0) leaves x as
// it is.  eta is the largest |A[i][k]| over rows k .. 4, as the reference's loop reads it (it tests the entry before it steps to the next).
template <int NC> __device__ static void pnp_qr_solve(double* A, double* b, double* x)
{
    double A1[NC], A2[NC];
    for (int k = 0; k < NC; k++) {
        double eta = fabs(A[k * NC + k]);
        for (int i = k + 1; i < 6; i++) { const double elt = fabs(A[(i - 1) * NC + k]); if (eta < elt) eta = elt; }
        if (eta == 0.0) return;
        const double inv_eta = 1.0 / eta;
        double sum = 0.0;
        for (int i = k; i < 6; i++) { A[i * NC + k] = A[i * NC + k] * inv_eta; sum = sum + A[i * NC + k] * A[i * NC + k]; }
        double sigma = sqrt(sum);
        if (A[k * NC + k] < 0.0) sigma = -sigma;
        A[k * NC + k] = A[k * NC + k] + sigma;
        A1[k] = sigma * A[k * NC + k];
        A2[k] = -eta * sigma;
        for (int j = k + 1; j < NC; j++) {
            double s2 = 0.0;
            for (int i = k; i < 6; i++) s2 = s2 + A[i * NC + k] * A[i * NC + j];
            const double tau = s2 / A1[k];
            for (int i = k; i < 6; i++) A[i * NC + j] = A[i * NC + j] - tau * A[i * NC + k];
        }
    }
    for (int j = 0; j < NC; j++) {
        double tau = 0.0;
        for (int i = j; i < 6; i++) tau = tau + A[i * NC + j] * b[i];
        tau = tau / A1[j];
        for (int i = j; i < 6; i++) b[i] = b[i] - tau * A[i * NC + j];
    }
    x[NC - 1] = b[NC - 1] / A2[NC - 1];
    for (int i = NC - 2; i >= 0; i--) {
        double sum = 0.0;
        for (int j = i + 1; j < NC; j++) sum = sum + A[i * NC + j] * x[j];
        x[i] = (b[i] - sum) / A2[i];
    }
}

// the three find_betas_approx_*: columns of L_6x10, qr_solve from x = 0, the reference's sign rules
__device__ static void pnp_betas_approx(int which, const double (*L)[10], const double rho[6], double betas[4])
{
    double a[30], b[6], x[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < 6; i++) b[i] = rho[i];
    if (which == 1) {
        for (int i = 0; i < 6; i++) { a[4 * i] = L[i][0]; a[4 * i + 1] = L[i][1]; a[4 * i + 2] = L[i][3]; a[4 * i + 3] = L[i][6]; }
        pnp_qr_solve<4>(a, b, x);
        if (x[0] < 0.0) { betas[0] = sqrt(-x[0]); betas[1] = -x[1] / betas[0]; betas[2] = -x[2] / betas[0]; betas[3] = -x[3] / betas[0]; }
        else { betas[0] = sqrt(x[0]); betas[1] = x[1] / betas[0]; betas[2] = x[2] / betas[0]; betas[3] = x[3] / betas[0]; }
        return;
    }
    if (which == 2) {
        for (int i = 0; i < 6; i++) { a[3 * i] = L[i][0]; a[3 * i + 1] = L[i][1]; a[3 * i + 2] = L[i][2]; }
        pnp_qr_solve<3>(a, b, x);
    } else {
        for (int i = 0; i < 6; i++) for (int j = 0; j < 5; j++) a[5 * i + j] = L[i][j];
        pnp_qr_solve<5>(a, b, x);
    }
    if (x[0] < 0.0) { betas[0] = sqrt(-x[0]); betas[1] = x[2] < 0.0 ? sqrt(-x[2]) : 0.0; }
    else { betas[0] = sqrt(x[0]); betas[1] = x[2] > 0.0 ? sqrt(x[2]) : 0.0; }
    if (x[1] < 0.0) betas[0] = -betas[0];
    betas[2] = which == 3 ? x[3] / betas[0] : 0.0;
    betas[3] = 0.0;
}

// gauss_newton: five steps; x starts at 0 and a step that meets a zero column keeps the previous x
__device__ static void pnp_gauss_newton(const double (*L)[10], const double rho[6], double betas[4])
{
    double x[4] = {0.0, 0.0, 0.0, 0.0};
    for (int it = 0; it < 5; it++) {
        double a[24], b[6];
        const double b0 = betas[0], b1 = betas[1], b2 = betas[2], b3 = betas[3];
        for (int i = 0; i < 6; i++) {
            const double* r = L[i];
            a[4 * i] = (((2.0 * r[0]) * b0 + r[1] * b1) + r[3] * b2) + r[6] * b3;
            a[4 * i + 1] = ((r[1] * b0 + (2.0 * r[2]) * b1) + r[4] * b2) + r[7] * b3;
            a[4 * i + 2] = ((r[3] * b0 + r[4] * b1) + (2.0 * r[5]) * b2) + r[8] * b3;
            a[4 * i + 3] = ((r[6] * b0 + r[7] * b1) + r[8] * b2) + (2.0 * r[9]) * b3;
            b[i] = rho[i] - ((((((((((r[0] * b0) * b0 + (r[1] * b0) * b1) + (r[2] * b1) * b1) + (r[3] * b0) * b2) + (r[4] * b1) * b2) + (r[5] * b2) * b2) +
                                 (r[6] * b0) * b3) + (r[7] * b1) * b3) + (r[8] * b2) * b3) + (r[9] * b3) * b3);
        }
        pnp_qr_solve<4>(a, b, x);
        for (int i = 0; i < 4; i++) betas[i] = betas[i] + x[i];
    }
}

// R = U V^T of ABt = U S V^T by the one-sided (Hestenes) Jacobi of orbhip_hestenes.h, then the reference's det < 0 row flip
__device__ static void pnp_rotation(const double abt[9], double R[9])
{
    double U[3][3], V[3][3], sw[3];      // [column][row]
    orbhip_hestenes3(abt, U, V, sw);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) R[3 * i + j] = (U[0][i] * V[0][j] + U[1][i] * V[1][j]) + U[2][i] * V[2][j];
    const double det = ((((((R[0] * R[4]) * R[8] + (R[1] * R[5]) * R[6]) + (R[2] * R[3]) * R[7]) - (R[2] * R[4]) * R[6]) - (R[1] * R[3]) * R[8]) - (R[0] * R[5]) * R[7]);
    if (det < 0.0) { R[6] = -R[6]; R[7] = -R[7]; R[8] = -R[8]; }
}

// compute_pose.  Every lane returns the same R, t.  The workgroup is one wave; barriers are passed by all lanes.
__device__ static void pnp_epnp(const PnpSet& S, double fu, double fv, double uc, double vc, PnpLds& sh, int lane, double R[9], double t[3])
{
    const double dm = (double)S.m;
    // choose_control_points: the centroid (also pw0 of estimate_R_and_t: the same sum and division), PW0^T PW0, its eigenvectors
    double c0[3], cws[4][3];
    {
        double a[3];
        pnp_reduce<3>(S, lane, a, [](const orbhip_pnp_corr& c, double (&v)[3]) { v[0] = (double)c.Xw[0]; v[1] = (double)c.Xw[1]; v[2] = (double)c.Xw[2]; });
        c0[0] = a[0] / dm; c0[1] = a[1] / dm; c0[2] = a[2] / dm;
    }
    double (*A3)[3] = reinterpret_cast<double (*)[3]>(&sh.A[0][0]);
    double (*V3)[3] = reinterpret_cast<double (*)[3]>(&sh.V[0][0]);
    {
        double a[6];
        pnp_reduce<6>(S, lane, a, [&](const orbhip_pnp_corr& c, double (&v)[6]) {
            const double d0 = (double)c.Xw[0] - c0[0], d1 = (double)c.Xw[1] - c0[1], d2 = (double)c.Xw[2] - c0[2];
            v[0] = d0 * d0; v[1] = d0 * d1; v[2] = d0 * d2; v[3] = d1 * d1; v[4] = d1 * d2; v[5] = d2 * d2;
        });
        __syncthreads();
        if (lane == 0) { A3[0][0] = a[0]; A3[0][1] = a[1]; A3[0][2] = a[2]; A3[1][0] = a[1]; A3[1][1] = a[3]; A3[1][2] = a[4]; A3[2][0] = a[2]; A3[2][1] = a[4]; A3[2][2] = a[5]; }
        __syncthreads();
    }
    orbhip_jacobi_eigen_wave<3>(A3, V3, lane);
    pnp_sort_desc<3>(A3, sh.ord, lane);
#pragma unroll
    for (int j = 0; j < 3; j++) cws[0][j] = c0[j];
#pragma unroll
    for (int i = 1; i < 4; i++) {
        const int o = sh.ord[i - 1];
        double dc = A3[o][o];
        if (dc < 0.0) dc = 0.0;
        const double k = sqrt(dc / dm);
#pragma unroll
        for (int j = 0; j < 3; j++) cws[i][j] = c0[j] + k * V3[j][o];
    }
    __syncthreads();
    // compute_barycentric_coordinates: CC^-1 by cofactors over the determinant
    double ci[9];
    {
        double cc[9];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 1; j < 4; j++) cc[3 * i + j - 1] = cws[j][i] - cws[0][i];
        const double m00 = cc[4] * cc[8] - cc[5] * cc[7], m01 = cc[3] * cc[8] - cc[5] * cc[6], m02 = cc[3] * cc[7] - cc[4] * cc[6];
        const double det = (cc[0] * m00 - cc[1] * m01) + cc[2] * m02;
        ci[0] = m00 / det; ci[1] = (cc[2] * cc[7] - cc[1] * cc[8]) / det; ci[2] = (cc[1] * cc[5] - cc[2] * cc[4]) / det;
        ci[3] = (cc[5] * cc[6] - cc[3] * cc[8]) / det; ci[4] = (cc[0] * cc[8] - cc[2] * cc[6]) / det; ci[5] = (cc[2] * cc[3] - cc[0] * cc[5]) / det;
        ci[6] = m02 / det; ci[7] = (cc[1] * cc[6] - cc[0] * cc[7]) / det; ci[8] = (cc[0] * cc[4] - cc[1] * cc[3]) / det;
    }
    // M^T M, a row a pass: entry (a, b) sums M1[a] M1[b] + M2[a] M2[b] over the points (fill_M's two rows of a point)
    for (int a = 0; a < 12; a++) {
        double row[12];
        pnp_reduce<12>(S, lane, row, [&](const orbhip_pnp_corr& c, double (&v)[12]) {
            double as[4], M1[12], M2[12];
            pnp_alphas(c, ci, c0, as);
            const double du = uc - (double)c.u, dv = vc - (double)c.v;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                M1[3 * i] = as[i] * fu; M1[3 * i + 1] = 0.0; M1[3 * i + 2] = as[i] * du;
                M2[3 * i] = 0.0; M2[3 * i + 1] = as[i] * fv; M2[3 * i + 2] = as[i] * dv;
            }
            double m1a = M1[0], m2a = M2[0];
#pragma unroll
            for (int b = 1; b < 12; b++) if (b == a) { m1a = M1[b]; m2a = M2[b]; }
#pragma unroll
            for (int b = 0; b < 12; b++) v[b] = m1a * M1[b] + m2a * M2[b];
        });
        if (lane < 12) {
            double x = row[0];
#pragma unroll
            for (int b = 1; b < 12; b++) if (b == lane) x = row[b];
            sh.A[a][lane] = x;
        }
    }
    __syncthreads();
    orbhip_jacobi_eigen_wave<12>(sh.A, sh.V, lane);
    pnp_sort_desc<12>(sh.A, sh.ord, lane);
    // the four null vectors v[i] = ut row 11 - i, into rows 0 .. 3 of A (the eigenvalues are no longer needed)
    double vk[4] = {0.0, 0.0, 0.0, 0.0};
    if (lane < 12) {
#pragma unroll
        for (int i = 0; i < 4; i++) vk[i] = sh.V[lane][sh.ord[11 - i]];
    }
    __syncthreads();
    if (lane < 12) {
#pragma unroll
        for (int i = 0; i < 4; i++) sh.A[i][lane] = vk[i];
    }
    __syncthreads();
    const double (*v)[12] = sh.A;
    // compute_L_6x10: lane i < 6 fills row i
    if (lane < 6) {
        const int pa = lane < 3 ? 0 : lane < 5 ? 1 : 2, pb = lane < 3 ? lane + 1 : lane < 5 ? lane - 1 : 3;
        double dv[4][3];
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int k = 0; k < 3; k++) dv[i][k] = v[i][3 * pa + k] - v[i][3 * pb + k];
        double* row = sh.L[lane];
        row[0] = pnp_dot3(dv[0], dv[0]); row[1] = 2.0 * pnp_dot3(dv[0], dv[1]); row[2] = pnp_dot3(dv[1], dv[1]);
        row[3] = 2.0 * pnp_dot3(dv[0], dv[2]); row[4] = 2.0 * pnp_dot3(dv[1], dv[2]); row[5] = pnp_dot3(dv[2], dv[2]);
        row[6] = 2.0 * pnp_dot3(dv[0], dv[3]); row[7] = 2.0 * pnp_dot3(dv[1], dv[3]); row[8] = 2.0 * pnp_dot3(dv[2], dv[3]); row[9] = pnp_dot3(dv[3], dv[3]);
    }
    __syncthreads();
    double rho[6];
    {
        const int pa[6] = {0, 0, 0, 1, 1, 2}, pb[6] = {1, 2, 3, 2, 3, 3};
#pragma unroll
        for (int i = 0; i < 6; i++) {
            const double d0 = cws[pa[i]][0] - cws[pb[i]][0], d1 = cws[pa[i]][1] - cws[pb[i]][1], d2 = cws[pa[i]][2] - cws[pb[i]][2];
            rho[i] = (d0 * d0 + d1 * d1) + d2 * d2;
        }
    }
    double best_err = 0.0;
    for (int which = 1; which <= 3; which++) {
        double betas[4];
        pnp_betas_approx(which, sh.L, rho, betas);
        pnp_gauss_newton(sh.L, rho, betas);
        // compute_ccs, solve_for_sign on the first point's pcs[2] (the sign goes into ccs; every pcs below is taken from the signed ccs)
        double ccs[4][3];
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int k = 0; k < 3; k++) {
                double s = 0.0;
#pragma unroll
                for (int i = 0; i < 4; i++) s = s + betas[i] * v[i][3 * j + k];
                ccs[j][k] = s;
            }
        if (S.m > 0) {
            double as[4];
            pnp_alphas(S.corr[S.first], ci, c0, as);
            const double pc2 = ((as[0] * ccs[0][2] + as[1] * ccs[1][2]) + as[2] * ccs[2][2]) + as[3] * ccs[3][2];
            if (pc2 < 0.0) {
#pragma unroll
                for (int j = 0; j < 4; j++)
#pragma unroll
                    for (int k = 0; k < 3; k++) ccs[j][k] = -ccs[j][k];
            }
        }
        // estimate_R_and_t
        double pc0[3], abt[9], Rc[9], tc[3];
        {
            double a[3];
            pnp_reduce<3>(S, lane, a, [&](const orbhip_pnp_corr& c, double (&o)[3]) {
                double as[4];
                pnp_alphas(c, ci, c0, as);
#pragma unroll
                for (int j = 0; j < 3; j++) o[j] = ((as[0] * ccs[0][j] + as[1] * ccs[1][j]) + as[2] * ccs[2][j]) + as[3] * ccs[3][j];
            });
            pc0[0] = a[0] / dm; pc0[1] = a[1] / dm; pc0[2] = a[2] / dm;
        }
        pnp_reduce<9>(S, lane, abt, [&](const orbhip_pnp_corr& c, double (&o)[9]) {
            double as[4];
            pnp_alphas(c, ci, c0, as);
            const double w0 = (double)c.Xw[0] - c0[0], w1 = (double)c.Xw[1] - c0[1], w2 = (double)c.Xw[2] - c0[2];
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const double pc = ((as[0] * ccs[0][j] + as[1] * ccs[1][j]) + as[2] * ccs[2][j]) + as[3] * ccs[3][j];
                const double d = pc - pc0[j];
                o[3 * j] = d * w0; o[3 * j + 1] = d * w1; o[3 * j + 2] = d * w2;
            }
        });
        pnp_rotation(abt, Rc);
#pragma unroll
        for (int i = 0; i < 3; i++) tc[i] = pc0[i] - pnp_dot3(Rc + 3 * i, c0);
        // reprojection_error
        double e[1];
        pnp_reduce<1>(S, lane, e, [&](const orbhip_pnp_corr& c, double (&o)[1]) {
            const double pw[3] = {(double)c.Xw[0], (double)c.Xw[1], (double)c.Xw[2]};
            const double Xc = pnp_dot3(Rc, pw) + tc[0], Yc = pnp_dot3(Rc + 3, pw) + tc[1], inv_Zc = 1.0 / (pnp_dot3(Rc + 6, pw) + tc[2]);
            const double ue = uc + (fu * Xc) * inv_Zc, ve = vc + (fv * Yc) * inv_Zc;
            const double du = (double)c.u - ue, dv = (double)c.v - ve;
            o[0] = sqrt(du * du + dv * dv);
        });
        const double err = e[0] / dm;
        if (which == 1 || err < best_err) {
            best_err = err;
#pragma unroll
            for (int k = 0; k < 9; k++) R[k] = Rc[k];
            t[0] = tc[0]; t[1] = tc[1]; t[2] = tc[2];
        }
    }
    __syncthreads();
}

// CheckInliers over all n: mask words and the count (every lane returns it)
__device__ static int pnp_check(const PnpDev& Q, const double R[9], const double t[3], double fu, double fv, double uc, double vc, unsigned long long* mask, int lane)
{
    int count = 0;
    for (int base = 0; base < Q.n; base += 64) {
        const int i = base + lane;
        bool in = false;
        if (i < Q.n) {
            const orbhip_pnp_corr c = Q.corr[i];
            const double x = (double)c.Xw[0], y = (double)c.Xw[1], z = (double)c.Xw[2];
            const float Xc = (float)(((R[0] * x + R[1] * y) + R[2] * z) + t[0]);
            const float Yc = (float)(((R[3] * x + R[4] * y) + R[5] * z) + t[1]);
            const float invZc = (float)(1.0 / (((R[6] * x + R[7] * y) + R[8] * z) + t[2]));
            const double ue = uc + (fu * (double)Xc) * (double)invZc, ve = vc + (fv * (double)Yc) * (double)invZc;
            const float distX = (float)((double)c.u - ue), distY = (float)((double)c.v - ve);
            const float error2 = distX * distX + distY * distY;
            in = error2 < c.max_error;
        }
        const unsigned long long m = __ballot(in);
        if (lane == 0) mask[base >> 6] = m;
        count += __popcll(m);
    }
    return count;
}

__device__ __forceinline__ void pnp_store(double* o, const double R[9], const double t[3], int count)
{
#pragma unroll
    for (int k = 0; k < 9; k++) o[k] = R[k];
    o[9] = t[0]; o[10] = t[1]; o[11] = t[2];
    reinterpret_cast<int*>(o + 12)[0] = count; reinterpret_cast<int*>(o + 12)[1] = 0;
    o[13] = 0.0; o[14] = 0.0; o[15] = 0.0;
}

__global__ __launch_bounds__(64) void k_pnp_hyp(const PnpDev* problems)
{
    __shared__ PnpLds sh;
    const PnpDev& Q = problems[blockIdx.y];
    const int h = blockIdx.x, lane = threadIdx.x;
    if (h >= Q.n_hyp) return;
    const double fu = (double)Q.K[0], fv = (double)Q.K[1], uc = (double)Q.K[2], vc = (double)Q.K[3];
    const int* quad = Q.quads + 4 * h;                                         // checked by the host: 0 .. n - 1, distinct
    const PnpSet S = {Q.corr, quad, nullptr, 4, 4, quad[0]};
    double R[9], t[3];
    pnp_epnp(S, fu, fv, uc, vc, sh, lane, R, t);
    const int count = pnp_check(Q, R, t, fu, fv, uc, vc, Q.mask + (size_t)h * Q.words, lane);
    if (lane == 0) pnp_store(Q.hyp + (size_t)h * PNP_REC, R, t, count);
}

// cand[j]: the hypothesis whose mask candidate j is (-1: the carried-in mask); cand_at[j]: the hypothesis at which the loop first refines it
__global__ __launch_bounds__(64) void k_pnp_select(const PnpDev* problems)
{
    const PnpDev& Q = problems[blockIdx.x];
    const int lane = threadIdx.x, nh = Q.n_hyp, mi = Q.min_inliers;
    int run = Q.best_in, ncand = 0;
    bool seen_new = false, seen_carried = false;
    for (int base = 0; base < nh; base += 64) {
        const int h = base + lane;
        int c = h < nh ? reinterpret_cast<const int*>(Q.hyp + (size_t)h * PNP_REC + 12)[0] : -1;
        if (c < mi) c = -1;                                                    // below the minimum a hypothesis does nothing
        int incl = c;
        for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(incl, d); if (lane >= d) incl = max(incl, o); }
        int before = __shfl_up(incl, 1);
        before = lane == 0 ? run : max(run, before);
        const bool reach = c >= 0, is_new = reach && c > before;
        const unsigned long long new_m = __ballot(is_new), reach_m = __ballot(reach);
        const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
        if (!seen_new && !seen_carried && reach_m) {
            const int l = __ffsll((long long)reach_m) - 1;                         // the first to reach the minimum: does it stand on the carried-in mask?
            if (!((new_m >> l) & 1ull)) { if (lane == 0) { Q.cand[0] = -1; Q.cand_at[0] = base + l; } ncand = 1; seen_carried = true; }
        }
        if (is_new) { const int j = ncand + __popcll(new_m & below); Q.cand[j] = h; Q.cand_at[j] = h; }
        ncand += __popcll(new_m);
        if (new_m) seen_new = true;
        run = max(run, __shfl(incl, 63));
    }
    if (lane == 0) { Q.res->n_cand = ncand; Q.res->best_inliers = run; }
}

__global__ __launch_bounds__(64) void k_pnp_refine(const PnpDev* problems)
{
    __shared__ PnpLds sh;
    const PnpDev& Q = problems[blockIdx.y];
    const int j = blockIdx.x, lane = threadIdx.x;
    if (j >= Q.res->n_cand) return;
    const int src = Q.cand[j];
    const unsigned long long* mask = src < 0 ? Q.mask_in : Q.mask + (size_t)src * Q.words;
    int m = 0, first = Q.n;
    for (int w = lane; w < Q.words; w += 64) { const unsigned long long x = mask[w]; m += __popcll(x); if (x && first == Q.n) first = 64 * w + __ffsll((long long)x) - 1; }
    for (int d = 32; d >= 1; d >>= 1) { m += __shfl_xor(m, d); first = min(first, __shfl_xor(first, d)); }
    const double fu = (double)Q.K[0], fv = (double)Q.K[1], uc = (double)Q.K[2], vc = (double)Q.K[3];
    const PnpSet S = {Q.corr, nullptr, mask, Q.n, m, first < Q.n ? first : 0};
    double R[9], t[3];
    pnp_epnp(S, fu, fv, uc, vc, sh, lane, R, t);
    const int count = pnp_check(Q, R, t, fu, fv, uc, vc, Q.ref_mask + (size_t)j * Q.words, lane);
    if (lane == 0) pnp_store(Q.ref + (size_t)j * PNP_REC, R, t, count);
}

__device__ static void pnp_tcw(const double* o, float T[16])
{
    for (int i = 0; i < 3; i++) { for (int k = 0; k < 3; k++) T[4 * i + k] = (float)o[3 * i + k]; T[4 * i + 3] = (float)o[9 + i]; }
    T[12] = 0.0f; T[13] = 0.0f; T[14] = 0.0f; T[15] = 1.0f;
}

__global__ __launch_bounds__(64) void k_pnp_finish(const PnpDev* problems)
{
    const PnpDev& Q = problems[blockIdx.x];
    const int lane = threadIdx.x, n = Q.n, ncand = Q.res->n_cand;
    int ok = ncand;                                                            // the first candidate whose refine succeeds
    for (int base = 0; base < ncand; base += 64) {
        const int j = base + lane;
        const bool good = j < ncand && reinterpret_cast<const int*>(Q.ref + (size_t)j * PNP_REC + 12)[0] > Q.min_inliers;
        const unsigned long long m = __ballot(good);
        if (m) { ok = base + __ffsll((long long)m) - 1; break; }
    }
    const int last = ok < ncand ? ok : ncand - 1;                                // the last candidate the loop met
    const int best = last >= 0 ? Q.cand[last] : -1;                             // -1: none, or only the carried-in mask
    if (best >= 0) {
        const unsigned long long* mask = Q.mask + (size_t)best * Q.words;
        for (int i = lane; i < n; i += 64) Q.best_mask[i] = (unsigned char)((mask[i >> 6] >> (i & 63)) & 1ull);
    }
    if (ok < ncand) {
        const unsigned long long* mask = Q.ref_mask + (size_t)ok * Q.words;
        for (int i = lane; i < n; i += 64) Q.refined_mask[i] = (unsigned char)((mask[i >> 6] >> (i & 63)) & 1ull);
    }
    if (lane == 0) {
        PnpResult& r = *Q.res;
        r.returned = ok < ncand ? Q.cand_at[ok] : -1;
        r.n_consumed = ok < ncand ? r.returned + 1 : Q.n_hyp;
        r.best = best; r.ok_cand = ok < ncand ? ok : -1;
        if (best >= 0) { const double* o = Q.hyp + (size_t)best * PNP_REC; r.best_inliers = reinterpret_cast<const int*>(o + 12)[0]; pnp_tcw(o, r.best_Tcw); }
        else r.best_inliers = Q.best_in;
        if (ok < ncand) { const double* o = Q.ref + (size_t)ok * PNP_REC; r.refined_inliers = reinterpret_cast<const int*>(o + 12)[0]; pnp_tcw(o, r.refined_Tcw); }
        else r.refined_inliers = 0;
    }
}

// ---------------------------------------------------------------------------------------------- host
static inline bool pnp_live(const orbhip_pnp_problem& Q) { return Q.n >= 4 && Q.n >= Q.min_inliers && Q.n_hyp > 0; }
static inline int pnp_cand_cap(const orbhip_pnp_problem& Q) { return std::min(Q.n_hyp, Q.n + 1) + 1; }     // strict maxima rise within 0 .. n; one carried-in mask

static orbhip_status pnp_problems(int device, int nproblems, orbhip_pnp_problem* problems, const char* who)
{
    OrbApiTimer api_timer;
    std::vector<int> live;
    int max_hyp = 0, max_cand = 0;
    for (int p = 0; p < nproblems; p++) {
        orbhip_pnp_problem& Q = problems[p];
        if (Q.n < 0 || Q.n_hyp < 0 || Q.min_inliers < 0 || Q.best_inliers_in < 0) return fail(ORBHIP_ERR_INVALID, "%s: problem %d: negative size", who, p);
        if (Q.n_hyp > PNP_MAX_HYP) return fail(ORBHIP_ERR_INVALID, "%s: problem %d: %d hypotheses, at most %d a call", who, p, Q.n_hyp, PNP_MAX_HYP);
        if (!pnp_live(Q)) continue;
        if (!Q.corr || !Q.quads || !Q.best_mask || !Q.refined_mask) return fail(ORBHIP_ERR_INVALID, "%s: problem %d: null pointer", who, p);
        if (Q.best_inliers_in > 0 && !Q.best_mask_in) return fail(ORBHIP_ERR_INVALID, "%s: problem %d: best_inliers_in = %d without best_mask_in", who, p, Q.best_inliers_in);
        if (Q.ref_cap < 0) return fail(ORBHIP_ERR_INVALID, "%s: problem %d: negative ref_cap", who, p);
        for (int h = 0; h < Q.n_hyp; h++) {
            const int32_t* q = Q.quads + 4 * h;
            for (int a = 0; a < 4; a++) {
                if (q[a] < 0 || q[a] >= Q.n) return fail(ORBHIP_ERR_INVALID, "%s: problem %d: hypothesis %d draws an index outside 0..%d", who, p, h, Q.n - 1);
                for (int b = 0; b < a; b++) if (q[a] == q[b]) return fail(ORBHIP_ERR_INVALID, "%s: problem %d: hypothesis %d draws an index twice", who, p, h);
            }
        }
    }
    for (int p = 0; p < nproblems; p++) {
        orbhip_pnp_problem& Q = problems[p];
        Q.n_consumed = 0; Q.returned = -1; Q.best = -1;
        if (pnp_live(Q)) { live.push_back(p); max_hyp = std::max(max_hyp, Q.n_hyp); max_cand = std::max(max_cand, pnp_cand_cap(Q)); }
    }
    if (live.empty()) return ORBHIP_OK;
    if (!device_present()) return fail(ORBHIP_ERR_HIP, "no HIP device available: no CPU fallback");
    HIPCHK(hipSetDevice(device));
    const hipStream_t s = orbhip_thread_stream(device);
    const int NL = (int)live.size();
    std::vector<PnpDev> hP(NL); std::vector<PnpResult> hA(NL);
    std::vector<std::vector<unsigned char> > hBest(NL), hRefined(NL);
    std::vector<std::vector<unsigned long long> > hMaskIn(NL), hRefMask(NL);
    std::vector<std::vector<double> > hHyp(NL), hRef(NL);
    std::vector<std::vector<int> > hCand(NL);
    PnpDev* dP = nullptr; PnpResult* dA = nullptr;
    std::vector<orbhip_pnp_corr*> dcorr(NL, nullptr); std::vector<int*> dquad(NL, nullptr), dcand(NL, nullptr), dat(NL, nullptr);
    std::vector<double*> dhyp(NL, nullptr), dref(NL, nullptr);
    std::vector<unsigned long long*> dmask(NL, nullptr), dmin(NL, nullptr), drmask(NL, nullptr); std::vector<unsigned char*> dbest(NL, nullptr), drefined(NL, nullptr);
    for (int k = 0; k < NL; k++) {
        const orbhip_pnp_problem& Q = problems[live[k]];
        const size_t words = ((size_t)Q.n + 63) / 64, cap = (size_t)pnp_cand_cap(Q);
        hBest[k].resize((size_t)Q.n); hRefined[k].resize((size_t)Q.n);
        hMaskIn[k].assign(words, 0ull);                                         // mvbBestInliers as words (all clear while mnBestInliers is 0)
        if (Q.best_inliers_in > 0) for (int i = 0; i < Q.n; i++) if (Q.best_mask_in[i]) hMaskIn[k][(size_t)i >> 6] |= 1ull << (i & 63);
        if (Q.hyp_R || Q.hyp_t || Q.hyp_count) hHyp[k].resize((size_t)Q.n_hyp * PNP_REC);
        if (Q.ref_cap > 0) { hRef[k].resize(cap * PNP_REC); hCand[k].resize(cap); if (Q.ref_mask) hRefMask[k].resize(cap * words); }
    }
    const hipError_t e = arena_call(device, s, [&](Arena& A) {
        A.io(&dP, (size_t)NL, (const PnpDev*)hP.data(), (size_t)NL);
        for (int k = 0; k < NL; k++) {
            const orbhip_pnp_problem& Q = problems[live[k]];
            A.io(&dcorr[k], (size_t)Q.n, Q.corr, (size_t)Q.n);
            A.io(&dquad[k], (size_t)Q.n_hyp * 4, (const int*)Q.quads, (size_t)Q.n_hyp * 4);
            A.io(&dmin[k], hMaskIn[k].size(), (const unsigned long long*)hMaskIn[k].data(), hMaskIn[k].size());
        }
        A.io(&dA, (size_t)NL, (const PnpResult*)nullptr, 0, hA.data(), (size_t)NL);
        for (int k = 0; k < NL; k++) {
            const orbhip_pnp_problem& Q = problems[live[k]];
            A.io(&dbest[k], (size_t)Q.n, (const unsigned char*)nullptr, 0, hBest[k].data(), (size_t)Q.n);
            A.io(&drefined[k], (size_t)Q.n, (const unsigned char*)nullptr, 0, hRefined[k].data(), (size_t)Q.n);
        }
        for (int k = 0; k < NL; k++) {                                          // the optional outputs and the scratch: behind what every call downloads
            const orbhip_pnp_problem& Q = problems[live[k]];
            const size_t words = ((size_t)Q.n + 63) / 64, cap = (size_t)pnp_cand_cap(Q);
            A.io(&dhyp[k], (size_t)Q.n_hyp * PNP_REC, (const double*)nullptr, 0, hHyp[k].empty() ? (double*)nullptr : hHyp[k].data(), hHyp[k].size());
            A.io(&dmask[k], (size_t)Q.n_hyp * words, (const unsigned long long*)nullptr, 0, (unsigned long long*)Q.hyp_mask, Q.hyp_mask ? (size_t)Q.n_hyp * words : 0);
            A.io(&dcand[k], cap, (const int*)nullptr, 0, hCand[k].empty() ? (int*)nullptr : hCand[k].data(), hCand[k].size());
            A.io(&dat[k], cap, (const int*)nullptr, 0);
            A.io(&dref[k], cap * PNP_REC, (const double*)nullptr, 0, hRef[k].empty() ? (double*)nullptr : hRef[k].data(), hRef[k].size());
            A.io(&drmask[k], cap * words, (const unsigned long long*)nullptr, 0, hRefMask[k].empty() ? (unsigned long long*)nullptr : hRefMask[k].data(), hRefMask[k].size());
        }
        for (int k = 0; k < NL; k++) {                                          // (hP is read when the arena is uploaded, after this pass has filled in the addresses)
            const orbhip_pnp_problem& Q = problems[live[k]]; PnpDev& D = hP[k];
            D.corr = dcorr[k]; D.quads = dquad[k]; D.mask_in = dmin[k]; D.hyp = dhyp[k]; D.mask = dmask[k]; D.cand = dcand[k]; D.cand_at = dat[k];
            D.ref = dref[k]; D.ref_mask = drmask[k]; D.res = dA ? dA + k : nullptr; D.best_mask = dbest[k]; D.refined_mask = drefined[k];
            D.n = Q.n; D.n_hyp = Q.n_hyp; D.words = (Q.n + 63) / 64; D.min_inliers = Q.min_inliers; D.best_in = Q.best_inliers_in; D.cand_cap = pnp_cand_cap(Q);
            memcpy(D.K, Q.K, sizeof D.K);
        }
    }, [&] {
        hipLaunchKernelGGL(k_pnp_hyp, dim3(max_hyp, NL, 1), dim3(64, 1, 1), 0, s, (const PnpDev*)dP);
        hipLaunchKernelGGL(k_pnp_select, dim3(NL, 1, 1), dim3(64, 1, 1), 0, s, (const PnpDev*)dP);
        hipLaunchKernelGGL(k_pnp_refine, dim3(max_cand, NL, 1), dim3(64, 1, 1), 0, s, (const PnpDev*)dP);
        hipLaunchKernelGGL(k_pnp_finish, dim3(NL, 1, 1), dim3(64, 1, 1), 0, s, (const PnpDev*)dP);
    });
    if (e != hipSuccess) return fail(ORBHIP_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    for (int k = 0; k < NL; k++) {
        orbhip_pnp_problem& Q = problems[live[k]]; const PnpResult& r = hA[k];
        const size_t words = ((size_t)Q.n + 63) / 64;
        Q.n_consumed = r.n_consumed; Q.returned = r.returned; Q.best = r.best; Q.best_inliers_out = r.best_inliers; Q.refined_inliers = r.refined_inliers;
        if (r.best >= 0) { memcpy(Q.best_Tcw, r.best_Tcw, sizeof Q.best_Tcw); memcpy(Q.best_mask, hBest[k].data(), (size_t)Q.n); }
        if (r.returned >= 0) { memcpy(Q.refined_Tcw, r.refined_Tcw, sizeof Q.refined_Tcw); memcpy(Q.refined_mask, hRefined[k].data(), (size_t)Q.n); }
        for (int h = 0; h < Q.n_hyp && !hHyp[k].empty(); h++) {
            const double* o = hHyp[k].data() + (size_t)h * PNP_REC;
            if (Q.hyp_R) memcpy(Q.hyp_R + 9 * (size_t)h, o, 9 * sizeof(double));
            if (Q.hyp_t) memcpy(Q.hyp_t + 3 * (size_t)h, o + 9, 3 * sizeof(double));
            if (Q.hyp_count) memcpy(Q.hyp_count + h, o + 12, sizeof(int32_t));
        }
        Q.n_ref = Q.ref_cap <= 0 ? 0 : r.ok_cand >= 0 ? r.ok_cand + 1 : r.n_cand;     // the refines the loop made: up to the one that returned
        for (int j = 0; j < std::min(Q.n_ref, Q.ref_cap); j++) {
            const double* o = hRef[k].data() + (size_t)j * PNP_REC;
            if (Q.ref_hyp) Q.ref_hyp[j] = hCand[k][j];
            if (Q.ref_R) memcpy(Q.ref_R + 9 * (size_t)j, o, 9 * sizeof(double));
            if (Q.ref_t) memcpy(Q.ref_t + 3 * (size_t)j, o + 9, 3 * sizeof(double));
            if (Q.ref_count) memcpy(Q.ref_count + j, o + 12, sizeof(int32_t));
            if (Q.ref_mask) memcpy(Q.ref_mask + words * (size_t)j, hRefMask[k].data() + words * (size_t)j, words * sizeof(uint64_t));
        }
    }
    return ORBHIP_OK;
}

extern "C" orbhip_status orbhip_pnp_iterate_batch(int device, int nproblems, orbhip_pnp_problem* problems)
{
    if (nproblems < 0 || (nproblems > 0 && !problems)) return fail(ORBHIP_ERR_INVALID, "pnp_iterate_batch: bad argument");
    return pnp_problems(device, nproblems, problems, "pnp_iterate_batch");
}

extern "C" orbhip_status orbhip_pnp_iterate(int device, orbhip_pnp_problem* problem)
{
    if (!problem) return fail(ORBHIP_ERR_INVALID, "pnp_iterate: null problem");
    return pnp_problems(device, 1, problem, "pnp_iterate");
}

#ifdef ORBHIP_TEST_HOOKS      // the CPU emulation build only: the serial template and the cooperative form of the Jacobi routine on one 12 x 12 matrix
__global__ void k_pnp_test_jacobi(const double* A, double* out)
{
    __shared__ PnpLds sh;
    const int lane = threadIdx.x;
    for (int e = lane; e < 144; e += 64) sh.A[e / 12][e % 12] = A[e];
    __syncthreads();
    orbhip_jacobi_eigen_wave<12>(sh.A, sh.V, lane);
    for (int e = lane; e < 144; e += 64) { out[e] = sh.A[e / 12][e % 12]; out[144 + e] = sh.V[e / 12][e % 12]; }
    if (lane == 0) {
        double As[12][12], Vs[12][12], w[12];
        for (int e = 0; e < 144; e++) As[e / 12][e % 12] = A[e];
        orbhip_jacobi_eigen<12>(As, Vs, w);
        for (int e = 0; e < 144; e++) { out[288 + e] = e / 12 == e % 12 ? w[e / 12] : As[e / 12][e % 12]; out[432 + e] = Vs[e / 12][e % 12]; }
    }
}
// out: 4 x 144 doubles - A and V of the cooperative form, then of the serial template
extern "C" void orbhip_test_jacobi12(const double* A, double* out)
{
    hipLaunchKernelGGL(k_pnp_test_jacobi, dim3(1, 1, 1), dim3(64, 1, 1), 0, 0, A, out);
}
#endif
