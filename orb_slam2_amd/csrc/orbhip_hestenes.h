// orbhip_hestenes.h — M = U diag(s) V^T of a 3 x 3 in double by a one-sided (Hestenes) Jacobi, inside a kernel; one thread does the whole matrix.
// Shared by PnPsolver's estimate_R_and_t (orbhip_pnp.hip) and Initializer's three 3 x 3 decompositions (orbhip_init.hip, H19 (4)).
//
// The statement, as tests/pnp_model.py restates it (hestenes) - every operation is one IEEE double +, -, *, / or sqrt, in this order:
//   G = M W, W = I; the columns of G are made orthogonal pair by pair, (0,1) (0,2) (1,2), W collects the rotations:
//     alpha = g_p . g_p, beta = g_q . g_q, gamma = g_p . g_q (each (a0 b0 + a1 b1) + a2 b2); nothing to do if gamma == 0 or
//     |gamma| <= ORBHIP_HEST_EPS sqrt(alpha beta)
//     zeta = (beta - alpha) / (2 gamma); t = 1 / (2 zeta) if |zeta| > 1e150, else sign(zeta) / (|zeta| + sqrt(zeta zeta + 1)); c = 1 / sqrt(t t + 1), s = t c
//     (x_p, x_q) <- (c x_p - s x_q, s x_p + c x_q) on the columns of G and of W
//   at most ORBHIP_HEST_SWEEPS sweeps; a sweep that rotates nothing ends the loop
//   singular values are the column norms, sorted descending by insertion with a strict `>` (equal values keep their index order);
//   U's column is g / s, V's column is w; where s_3 <= ORBHIP_HEST_RANK_TOL s_1 (rank 2) the third columns are the cross products of the first two.
// U, V: [column][row].  A non-finite entry makes every comparison false: the loops end at their constant bounds.
#ifndef ORBHIP_HESTENES_H
#define ORBHIP_HESTENES_H

#define ORBHIP_HEST_SWEEPS 30
#define ORBHIP_HEST_EPS 1e-15
#define ORBHIP_HEST_RANK_TOL 1e-12

__device__ __forceinline__ double orbhip_hest_dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ void orbhip_hest_rot2(double c, double s, double& xp, double& xq) { const double a = xp, b = xq; xp = c * a - s * b; xq = s * a + c * b; }
__device__ __forceinline__ void orbhip_hest_cross(const double a[3], const double b[3], double o[3])
{
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}

// M row-major
__device__ static void orbhip_hestenes3(const double M[9], double U[3][3], double V[3][3], double sw[3])
{
    double G[3][3], W[3][3];      // [column][row]
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int r = 0; r < 3; r++) { G[c][r] = M[3 * r + c]; W[c][r] = r == c ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < ORBHIP_HEST_SWEEPS; sweep++) {
        bool rotated = false;
#pragma unroll
        for (int pair = 0; pair < 3; pair++) {
            const int p = pair == 2 ? 1 : 0, q = pair == 0 ? 1 : 2;
            const double alpha = orbhip_hest_dot3(G[p], G[p]), beta = orbhip_hest_dot3(G[q], G[q]), gamma = orbhip_hest_dot3(G[p], G[q]);
            if (gamma == 0.0) continue;
            if (fabs(gamma) <= ORBHIP_HEST_EPS * sqrt(alpha * beta)) continue;
            rotated = true;
            const double zeta = (beta - alpha) / (2.0 * gamma);
            double t;
            if (fabs(zeta) > 1e150) t = 1.0 / (2.0 * zeta);
            else { t = 1.0 / (fabs(zeta) + sqrt(zeta * zeta + 1.0)); if (zeta < 0.0) t = -t; }
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
            for (int k = 0; k < 3; k++) { orbhip_hest_rot2(c, s, G[p][k], G[q][k]); orbhip_hest_rot2(c, s, W[p][k], W[q][k]); }
        }
        if (!rotated) break;
    }
    double sg[3];
#pragma unroll
    for (int c = 0; c < 3; c++) sg[c] = sqrt(orbhip_hest_dot3(G[c], G[c]));
    int o0 = 0, o1 = 1, o2 = 2;                                                 // insertion by strict `>`
    if (sg[o1] > sg[o0]) { const int t = o0; o0 = o1; o1 = t; }
    if (sg[o2] > sg[o1]) { const int t = o1; o1 = o2; o2 = t; if (sg[o1] > sg[o0]) { const int u = o0; o0 = o1; o1 = u; } }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const int o = c == 0 ? o0 : c == 1 ? o1 : o2;
        const double sv = o == 0 ? sg[0] : o == 1 ? sg[1] : sg[2];
        sw[c] = sv;
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const double g = o == 0 ? G[0][r] : o == 1 ? G[1][r] : G[2][r], w = o == 0 ? W[0][r] : o == 1 ? W[1][r] : W[2][r];
            U[c][r] = g / sv; V[c][r] = w;
        }
    }
    if (!(sw[2] > ORBHIP_HEST_RANK_TOL * sw[0])) { orbhip_hest_cross(U[0], U[1], U[2]); orbhip_hest_cross(V[0], V[1], V[2]); }
}
#endif
