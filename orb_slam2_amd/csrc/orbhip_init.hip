// orbhip_init.hip — Initializer::Initialize (Initializer.cc:44-121) for one candidate frame pair or several, in four launches: both RANSACs
// (FindHomography :124-172, FindFundamental :175-223), the model choice RH = SH / (SH + SF) > 0.40, ReconstructH (:572-732) or ReconstructF
// (:470-570) with CheckRT (:798-907) and Triangulate (:734-747) for every motion hypothesis, and the final selection rules.  The arithmetic is
// DESIGN.md H19, restated in tests/init_model.py: float wherever the reference holds a CV_32F Mat or a float, every OpenCV primitive by its stated
// replacement.
//
//   k_init_hyp       one wave per (set, model, problem): gathers the 8 drawn matches, builds A (16 x 9 for H, 8 x 9 for F) in float and A^T A in
//                    double in LDS, runs the cooperative Jacobi, takes the eigenvector of the smallest eigenvalue, denormalises (H: and inverts;
//                    F: rank-2 projection first), then scores all matches 64 at a time: ballot words for the mask, 64 float partials and the
//                    fixed tree for the score.
//   k_init_select    one wave per problem: the first strict maximum of each model, RH, the masks as bytes, N, and the 8 (H) or 4 (F) motion
//                    hypotheses of the chosen model with their K [R | t] and camera centre.
//   k_init_check_rt  one thread per (motion hypothesis, match): Triangulate with the per-thread 4 x 4 Jacobi, then CheckRT's tests.
//   k_init_finish    one workgroup of eight waves per problem, a wave per motion hypothesis: nGood and the order statistic min(50, nGood - 1) of the
//                    accepted cosines by a 32-step selection on their ordered bit patterns; then thread 0 applies the selection rules and all
//                    threads write the per-match outputs.
// acos never runs on the device: the host turns min_parallax into the two cosine thresholds the rules need (init_cos_threshold).
// No device state survives a call, no floating-point atomics, every loop is bounded by n, n_sets or a constant whatever the numbers are.
#include "orbhip_ctx.h"
#include "orbhip_jacobi.h"
#include "orbhip_hestenes.h"
#include <cmath>

#define INIT_MAX_N 8192
#define INIT_MAX_SETS 4096
#define INIT_HREC 12                   // floats per hypothesis record: M[9] score pad pad
#define INIT_MREC 32                   // floats per motion hypothesis: R[9] t[3] P2[12] O2[3] pad

struct InitResult {
    int returned, model, best_h, best_f, n_mot, best_mot, N, pad;
    float SH, SF, H21[9], F21[9], R21[9], t21[3], mot_cos[8]; int mot_good[8];
};
struct InitDev {
    const float4* matches; const int* sets; float* hyp; unsigned long long* mask; InitResult* res; float* mot; float* cosb; float* p3; unsigned char* st;
    unsigned char* mask_h; unsigned char* mask_f; float* p3d; unsigned char* tri;
    int n, n_sets, words, mode, min_tri, pad;
    float K[4], sigma, norm1[4], norm2[4], min_par, cos_gt, cos_ge;
};
struct InitLds { double A[9][9], V[9][9]; float M[16][9]; };

// one entry of a CV_32F product with inner length 3: mode 0 sums the products in double from 0 and rounds once, mode 1 sums
// them in float
__device__ __forceinline__ double in_dotd(float a0, float a1, float a2, float b0, float b1, float b2)
{
    double s = 0.0;
    s += (double)a0 * (double)b0; s += (double)a1 * (double)b1; s += (double)a2 * (double)b2;
    return s;
}
__device__ __forceinline__ float in_dotf(float a0, float a1, float a2, float b0, float b1, float b2)
{
    float t0 = a0 * b0;
    t0 = t0 + a1 * b1; t0 = t0 + a2 * b2;
    return t0;
}
__device__ __forceinline__ float in_mul(int mode, float a0, float a1, float a2, float b0, float b1, float b2)
{
    return mode == 1 ? in_dotf(a0, a1, a2, b0, b1, b2) : (float)in_dotd(a0, a1, a2, b0, b1, b2);
}
// `R*x + t` as one expression, as orbhip_sim3.hip treats it
__device__ __forceinline__ float in_affine(int mode, float a0, float a1, float a2, float b0, float b1, float b2, float t)
{
    if (mode == 1) return (float)((double)in_dotf(a0, a1, a2, b0, b1, b2) + (double)t);
    return (float)in_dotd(a0, a1, a2, b0, b1, b2) + t;
}
// C = A B, 3 x 3 row-major.  A product that carries a transposition flag is called with mode 0 (the generic kernel: the double sum in both modes)
__device__ static void in_mm3(int mode, const float A[9], const float B[9], float C[9])
{
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) C[3 * i + j] = in_mul(mode, A[3 * i], A[3 * i + 1], A[3 * i + 2], B[j], B[3 + j], B[6 + j]);
}
__device__ __forceinline__ void in_mv3(int mode, const float A[9], const float x[3], float y[3])
{
#pragma unroll
    for (int i = 0; i < 3; i++) y[i] = in_mul(mode, A[3 * i], A[3 * i + 1], A[3 * i + 2], x[0], x[1], x[2]);
}
__device__ __forceinline__ void in_t3(const float A[9], float T[9])
{
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) T[3 * i + j] = A[3 * j + i];
}
__device__ __forceinline__ float in_sqrt(float x) { return (float)sqrt((double)x); }
// cv::norm of three floats: the square root of the double sum of squares from 0.0, in double
__device__ __forceinline__ double in_norm3(const float a[3]) { return sqrt(in_dotd(a[0], a[1], a[2], a[0], a[1], a[2])); }

// Mat::inv() of a 3 x 3: cofactors over the determinant in double, rounded to float
__device__ static void in_inv3(const float m[9], float o[9])
{
    double c[9];
#pragma unroll
    for (int k = 0; k < 9; k++) c[k] = (double)m[k];
    const double m00 = c[4] * c[8] - c[5] * c[7], m01 = c[3] * c[8] - c[5] * c[6], m02 = c[3] * c[7] - c[4] * c[6];
    const double det = (c[0] * m00 - c[1] * m01) + c[2] * m02;
    o[0] = (float)(m00 / det); o[1] = (float)((c[2] * c[7] - c[1] * c[8]) / det); o[2] = (float)((c[1] * c[5] - c[2] * c[4]) / det);
    o[3] = (float)((c[5] * c[6] - c[3] * c[8]) / det); o[4] = (float)((c[0] * c[8] - c[2] * c[6]) / det); o[5] = (float)((c[2] * c[3] - c[0] * c[5]) / det);
    o[6] = (float)(m02 / det); o[7] = (float)((c[1] * c[6] - c[0] * c[7]) / det); o[8] = (float)((c[0] * c[4] - c[1] * c[3]) / det);
}
__device__ __forceinline__ double in_det3(const float m[9])
{
    const double c0 = m[0], c1 = m[1], c2 = m[2], c3 = m[3], c4 = m[4], c5 = m[5], c6 = m[6], c7 = m[7], c8 = m[8];
    const double m00 = c4 * c8 - c5 * c7, m01 = c3 * c8 - c5 * c6, m02 = c3 * c7 - c4 * c6;
    return (c0 * m00 - c1 * m01) + c2 * m02;
}

// M = U diag(w) V^T of a 3 x 3: the Hestenes form of orbhip_hestenes.h (H18 (5)) on the widened matrix; U, w, V rounded to float (row-major, column c
// the c-th vector)
__device__ static void in_svd3(const float M[9], float Uo[9], float wo[3], float Vo[9])
{
    double Md[9], U[3][3], V[3][3], sw[3];      // [column][row]
#pragma unroll
    for (int k = 0; k < 9; k++) Md[k] = (double)M[k];
    orbhip_hestenes3(Md, U, V, sw);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        wo[c] = (float)sw[c];
#pragma unroll
        for (int r = 0; r < 3; r++) { Uo[3 * r + c] = (float)U[c][r]; Vo[3 * r + c] = (float)V[c][r]; }
    }
}

// CheckHomography's two terms of one match: returns bIn, adds to the lane's partial as the reference adds to score
__device__ __forceinline__ bool in_score_h(const float H[9], const float Hi[9], float u1, float v1, float u2, float v2, float invS, float& part)
{
    const float th = 5.991f;
    bool in = true;
    const float w2 = (float)(1.0 / (double)((Hi[6] * u2 + Hi[7] * v2) + Hi[8]));
    const float u2in1 = ((Hi[0] * u2 + Hi[1] * v2) + Hi[2]) * w2, v2in1 = ((Hi[3] * u2 + Hi[4] * v2) + Hi[5]) * w2;
    const float sq1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
    const float chi1 = sq1 * invS;
    if (chi1 > th) in = false; else part = part + (th - chi1);
    const float w1 = (float)(1.0 / (double)((H[6] * u1 + H[7] * v1) + H[8]));
    const float u1in2 = ((H[0] * u1 + H[1] * v1) + H[2]) * w1, v1in2 = ((H[3] * u1 + H[4] * v1) + H[5]) * w1;
    const float sq2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
    const float chi2 = sq2 * invS;
    if (chi2 > th) in = false; else part = part + (th - chi2);
    return in;
}
// CheckFundamental's
__device__ __forceinline__ bool in_score_f(const float F[9], float u1, float v1, float u2, float v2, float invS, float& part)
{
    const float th = 3.841f, thScore = 5.991f;
    bool in = true;
    const float a2 = (F[0] * u1 + F[1] * v1) + F[2], b2 = (F[3] * u1 + F[4] * v1) + F[5], c2 = (F[6] * u1 + F[7] * v1) + F[8];
    const float num2 = (a2 * u2 + b2 * v2) + c2;
    const float sq1 = (num2 * num2) / (a2 * a2 + b2 * b2);
    const float chi1 = sq1 * invS;
    if (chi1 > th) in = false; else part = part + (thScore - chi1);
    const float a1 = (F[0] * u2 + F[3] * v2) + F[6], b1 = (F[1] * u2 + F[4] * v2) + F[7], c1 = (F[2] * u2 + F[5] * v2) + F[8];
    const float num1 = (a1 * u1 + b1 * v1) + c1;
    const float sq2 = (num1 * num1) / (a1 * a1 + b1 * b1);
    const float chi2 = sq2 * invS;
    if (chi2 > th) in = false; else part = part + (thScore - chi2);
    return in;
}

__global__ __launch_bounds__(64) void k_init_hyp(const InitDev* problems)
{
    __shared__ InitLds sh;
    const InitDev& Q = problems[blockIdx.y];
    const int h = blockIdx.x >> 1, isF = blockIdx.x & 1, lane = threadIdx.x, n = Q.n, mode = Q.mode;
    if (h >= Q.n_sets) return;
    const int rows = isF ? 8 : 16;
    const float m1x = Q.norm1[0], m1y = Q.norm1[1], s1x = Q.norm1[2], s1y = Q.norm1[3], m2x = Q.norm2[0], m2y = Q.norm2[1], s2x = Q.norm2[2], s2y = Q.norm2[3];
    if (lane < rows) {
        const int j = isF ? lane : lane >> 1;
        const float4 m = Q.matches[Q.sets[8 * h + j]];                            // checked by the host: 0 .. n - 1
        const float u1 = (m.x - m1x) * s1x, v1 = (m.y - m1y) * s1y, u2 = (m.z - m2x) * s2x, v2 = (m.w - m2y) * s2y;
        float* r = sh.M[lane];
        if (isF) { r[0] = u2 * u1; r[1] = u2 * v1; r[2] = u2; r[3] = v2 * u1; r[4] = v2 * v1; r[5] = v2; r[6] = u1; r[7] = v1; r[8] = 1.0f; }
        else if (!(lane & 1)) { r[0] = 0.0f; r[1] = 0.0f; r[2] = 0.0f; r[3] = -u1; r[4] = -v1; r[5] = -1.0f; r[6] = v2 * u1; r[7] = v2 * v1; r[8] = v2; }
        else { r[0] = u1; r[1] = v1; r[2] = 1.0f; r[3] = 0.0f; r[4] = 0.0f; r[5] = 0.0f; r[6] = -(u2 * u1); r[7] = -(u2 * v1); r[8] = -u2; }
    }
    __syncthreads();
    for (int e = lane; e < 81; e += 64) {
        const int a = e / 9, b = e % 9;
        double s = 0.0;
        for (int r = 0; r < rows; r++) s += (double)sh.M[r][a] * (double)sh.M[r][b];
        sh.A[a][b] = s;
    }
    __syncthreads();
    orbhip_jacobi_eigen_wave<9>(sh.A, sh.V, lane);
    int best = 0;                                                              // the first index strictly smaller than every earlier one
    for (int i = 1; i < 9; i++) if (sh.A[i][i] < sh.A[best][best]) best = i;
    float v[9];
    for (int k = 0; k < 9; k++) v[k] = (float)sh.V[k][best];
    const float T1[9] = {s1x, 0.0f, (-m1x) * s1x, 0.0f, s1y, (-m1y) * s1y, 0.0f, 0.0f, 1.0f};
    const float T2[9] = {s2x, 0.0f, (-m2x) * s2x, 0.0f, s2y, (-m2y) * s2y, 0.0f, 0.0f, 1.0f};
    float Mx[9], Hi[9], tmp[9];
    if (isF) {
        float U[9], w[3], V[9], D[9], Vt[9], UD[9], Fn[9], T2t[9];
        in_svd3(v, U, w, V);
        w[2] = 0.0f;
#pragma unroll
        for (int k = 0; k < 9; k++) D[k] = 0.0f;
        D[0] = w[0]; D[4] = w[1]; D[8] = w[2];
        in_t3(V, Vt); in_t3(T2, T2t);
        in_mm3(mode, U, D, UD); in_mm3(mode, UD, Vt, Fn);
        in_mm3(mode, T2t, Fn, tmp); in_mm3(mode, tmp, T1, Mx);
    } else {
        float T2inv[9];
        in_inv3(T2, T2inv);
        in_mm3(mode, T2inv, v, tmp); in_mm3(mode, tmp, T1, Mx);
        in_inv3(Mx, Hi);
    }
    const float invS = (float)(1.0 / (double)(Q.sigma * Q.sigma));
    unsigned long long* mask = Q.mask + ((size_t)isF * Q.n_sets + h) * Q.words;
    float part = 0.0f;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        bool in = false;
        if (i < n) {
            const float4 m = Q.matches[i];
            in = isF ? in_score_f(Mx, m.x, m.y, m.z, m.w, invS, part) : in_score_h(Mx, Hi, m.x, m.y, m.z, m.w, invS, part);
        }
        const unsigned long long b = __ballot(in);
        if (lane == 0) mask[base >> 6] = b;
    }
    for (int d = 32; d >= 1; d >>= 1) part = part + __shfl_xor(part, d);
    if (lane == 0) {
        float* o = Q.hyp + ((size_t)isF * Q.n_sets + h) * INIT_HREC;
#pragma unroll
        for (int k = 0; k < 9; k++) o[k] = Mx[k];
        o[9] = part; o[10] = 0.0f; o[11] = 0.0f;
    }
}

// one motion hypothesis: R, t, P2 = K [R | t], O2 = -R^T t
__device__ static void in_store_motion(float* o, int mode, const float K[4], const float R[9], const float t[3])
{
    const float Km[9] = {K[0], 0.0f, K[2], 0.0f, K[1], K[3], 0.0f, 0.0f, 1.0f};
#pragma unroll
    for (int k = 0; k < 9; k++) o[k] = R[k];
    o[9] = t[0]; o[10] = t[1]; o[11] = t[2];
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) o[12 + 4 * r + c] = in_mul(mode, Km[3 * r], Km[3 * r + 1], Km[3 * r + 2], R[c], R[3 + c], R[6 + c]);
        o[12 + 4 * r + 3] = in_mul(mode, Km[3 * r], Km[3 * r + 1], Km[3 * r + 2], t[0], t[1], t[2]);
    }
#pragma unroll
    for (int r = 0; r < 3; r++) o[24 + r] = -(float)in_dotd(R[r], R[3 + r], R[6 + r], t[0], t[1], t[2]);       // a transposition flag: the generic kernel
    for (int k = 27; k < INIT_MREC; k++) o[k] = 0.0f;
}

// ReconstructH up to the eight (R, t); false: the d1/d2, d2/d3 early return
__device__ static bool in_motions_h(const InitDev& Q, const float H21[9], bool write)
{
    const int mode = Q.mode;
    const float Km[9] = {Q.K[0], 0.0f, Q.K[2], 0.0f, Q.K[1], Q.K[3], 0.0f, 0.0f, 1.0f};
    float invK[9], tmp[9], A[9], U[9], w[3], V[9], Vt[9];
    in_inv3(Km, invK);
    in_mm3(mode, invK, H21, tmp); in_mm3(mode, tmp, Km, A);
    in_svd3(A, U, w, V);
    in_t3(V, Vt);
    const float s = (float)(in_det3(U) * in_det3(Vt));
    const float d1 = w[0], d2 = w[1], d3 = w[2];
    if ((double)(d1 / d2) < 1.00001 || (double)(d2 / d3) < 1.00001) return false;
    const float aux1 = in_sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3)), aux3 = in_sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
    const float aux_st = in_sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2), ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
    const float aux_sp = in_sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2), cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
    float sU[9];
#pragma unroll
    for (int k = 0; k < 9; k++) sU[k] = s * U[k];
    for (int i = 0; i < 8; i++) {
        const int j = i & 3;
        const float x1 = j < 2 ? aux1 : -aux1, x3 = (j & 1) ? -aux3 : aux3;
        const bool flip = j == 1 || j == 2;
        float Rp[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f}, tp[3];
        if (i < 4) {
            const float st = flip ? -aux_st : aux_st;
            Rp[0] = ctheta; Rp[2] = -st; Rp[6] = st; Rp[8] = ctheta;
            tp[0] = x1 * (d1 - d3); tp[1] = 0.0f * (d1 - d3); tp[2] = (-x3) * (d1 - d3);
        } else {
            const float sp = flip ? -aux_sp : aux_sp;
            Rp[0] = cphi; Rp[2] = sp; Rp[4] = -1.0f; Rp[6] = sp; Rp[8] = -cphi;
            tp[0] = x1 * (d1 + d3); tp[1] = 0.0f * (d1 + d3); tp[2] = x3 * (d1 + d3);
        }
        float R[9], t[3];
        in_mm3(mode, sU, Rp, tmp); in_mm3(mode, tmp, Vt, R);
        in_mv3(mode, U, tp, t);
        const float nrm = (float)in_norm3(t);
        t[0] = t[0] / nrm; t[1] = t[1] / nrm; t[2] = t[2] / nrm;
        if (write) in_store_motion(Q.mot + i * INIT_MREC, mode, Q.K, R, t);
    }
    return true;
}

// ReconstructF up to the four (R, t)
__device__ static void in_motions_f(const InitDev& Q, const float F21[9], bool write)
{
    const int mode = Q.mode;
    const float Km[9] = {Q.K[0], 0.0f, Q.K[2], 0.0f, Q.K[1], Q.K[3], 0.0f, 0.0f, 1.0f};
    const float W[9] = {0.0f, -1.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    float Kt[9], Wt[9], tmp[9], E[9], U[9], w[3], V[9], Vt[9], R1[9], R2[9], t[3];
    in_t3(Km, Kt); in_t3(W, Wt);
    in_mm3(0, Kt, F21, tmp);                                                    // K.t() * F21: a transposition flag
    in_mm3(mode, tmp, Km, E);
    in_svd3(E, U, w, V);
    in_t3(V, Vt);
    t[0] = U[2]; t[1] = U[5]; t[2] = U[8];
    const float nrm = (float)in_norm3(t);
    t[0] = t[0] / nrm; t[1] = t[1] / nrm; t[2] = t[2] / nrm;
    in_mm3(mode, U, W, tmp); in_mm3(mode, tmp, Vt, R1);
    if (in_det3(R1) < 0.0) { for (int k = 0; k < 9; k++) R1[k] = -R1[k]; }
    in_mm3(0, U, Wt, tmp);                                                      // u * W.t(): a transposition flag
    in_mm3(mode, tmp, Vt, R2);
    if (in_det3(R2) < 0.0) { for (int k = 0; k < 9; k++) R2[k] = -R2[k]; }
    const float t2[3] = {-t[0], -t[1], -t[2]};
    if (write) {
        in_store_motion(Q.mot + 0 * INIT_MREC, mode, Q.K, R1, t);
        in_store_motion(Q.mot + 1 * INIT_MREC, mode, Q.K, R2, t);
        in_store_motion(Q.mot + 2 * INIT_MREC, mode, Q.K, R1, t2);
        in_store_motion(Q.mot + 3 * INIT_MREC, mode, Q.K, R2, t2);
    }
}

__global__ __launch_bounds__(64) void k_init_select(const InitDev* problems)
{
    const InitDev& Q = problems[blockIdx.x];
    const int lane = threadIdx.x, ns = Q.n_sets, n = Q.n;
    float S[2]; int best[2];
    for (int m = 0; m < 2; m++) {
        const float* rec = Q.hyp + (size_t)m * ns * INIT_HREC;
        float mx = 0.0f;                                                       // currentScore > score from 0.0f: a NaN never wins
        for (int h = lane; h < ns; h += 64) { const float s = rec[(size_t)h * INIT_HREC + 9]; if (s > mx) mx = s; }
        for (int d = 32; d >= 1; d >>= 1) { const float o = __shfl_xor(mx, d); if (o > mx) mx = o; }
        int first = 0x7fffffff;
        if (mx > 0.0f) for (int h = lane; h < ns; h += 64) { if (rec[(size_t)h * INIT_HREC + 9] == mx) { first = h; break; } }
        for (int d = 32; d >= 1; d >>= 1) first = min(first, __shfl_xor(first, d));
        S[m] = mx; best[m] = first == 0x7fffffff ? -1 : first;
    }
    const float RH = S[0] / (S[0] + S[1]);
    int model = (double)RH > 0.40 ? 0 : 1;
    if (best[model] < 0) model = -1;
    for (int m = 0; m < 2; m++) {
        unsigned char* out = m ? Q.mask_f : Q.mask_h;
        const unsigned long long* mask = Q.mask + ((size_t)m * ns + (best[m] < 0 ? 0 : best[m])) * Q.words;
        for (int i = lane; i < n; i += 64) out[i] = best[m] < 0 ? (unsigned char)0 : (unsigned char)((mask[i >> 6] >> (i & 63)) & 1ull);
    }
    int N = 0;
    if (model >= 0) {
        const unsigned long long* mask = Q.mask + ((size_t)model * ns + best[model]) * Q.words;
        for (int w = lane; w < Q.words; w += 64) N += __popcll(mask[w]);
        for (int d = 32; d >= 1; d >>= 1) N += __shfl_xor(N, d);
    }
    float Mh[9], Mf[9];
    for (int k = 0; k < 9; k++) {
        Mh[k] = best[0] < 0 ? 0.0f : Q.hyp[(size_t)best[0] * INIT_HREC + k];
        Mf[k] = best[1] < 0 ? 0.0f : Q.hyp[((size_t)ns + best[1]) * INIT_HREC + k];
    }
    int n_mot = 0;
    if (model == 0) { if (in_motions_h(Q, Mh, lane == 0)) n_mot = 8; }      // else: the d1/d2, d2/d3 return, nothing to check
    else if (model == 1) { in_motions_f(Q, Mf, lane == 0); n_mot = 4; }
    if (lane == 0) {
        InitResult& r = *Q.res;
        r.returned = 0; r.model = model; r.best_h = best[0]; r.best_f = best[1]; r.n_mot = n_mot; r.best_mot = -1; r.N = N; r.pad = 0;
        r.SH = S[0]; r.SF = S[1];
        for (int k = 0; k < 9; k++) { r.H21[k] = Mh[k]; r.F21[k] = Mf[k]; r.R21[k] = 0.0f; }
        r.t21[0] = 0.0f; r.t21[1] = 0.0f; r.t21[2] = 0.0f;
        for (int k = 0; k < 8; k++) { r.mot_cos[k] = 0.0f; r.mot_good[k] = 0; }
    }
}

// one (motion hypothesis, match): status bit 0 = counted in nGood, bit 1 = vbGood
__global__ __launch_bounds__(64) void k_init_check_rt(const InitDev* problems)
{
    const InitDev& Q = problems[blockIdx.z];
    const int mot = blockIdx.x, i = blockIdx.y * 64 + threadIdx.x, n = Q.n, mode = Q.mode;
    const InitResult& res = *Q.res;
    if (mot >= res.n_mot || i >= n) return;
    const size_t slot = (size_t)mot * n + i;
    unsigned char status = 0;
    float cosP = 0.0f, p[3] = {0.0f, 0.0f, 0.0f};
    const unsigned long long* mask = Q.mask + ((size_t)res.model * Q.n_sets + (res.model ? res.best_f : res.best_h)) * Q.words;
    if ((mask[i >> 6] >> (i & 63)) & 1ull) {
        const float* M = Q.mot + mot * INIT_MREC;
        const float fx = Q.K[0], fy = Q.K[1], cx = Q.K[2], cy = Q.K[3];
        const float4 m = Q.matches[i];
        const float P1[12] = {fx, 0.0f, cx, 0.0f, 0.0f, fy, cy, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f};
        float Ar[4][4];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            Ar[0][c] = m.x * P1[8 + c] - P1[c]; Ar[1][c] = m.y * P1[8 + c] - P1[4 + c];
            Ar[2][c] = m.z * M[12 + 8 + c] - M[12 + c]; Ar[3][c] = m.w * M[12 + 8 + c] - M[12 + 4 + c];
        }
        double A[4][4], V[4][4], w[4];
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int b = 0; b < 4; b++) {
                double s = 0.0;
#pragma unroll
                for (int r = 0; r < 4; r++) s += (double)Ar[r][a] * (double)Ar[r][b];
                A[a][b] = s;
            }
        orbhip_jacobi_eigen<4>(A, V, w);
        int best = 0;
#pragma unroll
        for (int k = 1; k < 4; k++) if (w[k] < w[best]) best = k;
        float x[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            double e = V[k][0];
#pragma unroll
            for (int c = 1; c < 4; c++) if (c == best) e = V[k][c];
            x[k] = (float)e;
        }
        const float q[3] = {x[0] / x[3], x[1] / x[3], x[2] / x[3]};
        if (__builtin_isfinite(q[0]) && __builtin_isfinite(q[1]) && __builtin_isfinite(q[2])) {
            const float O2[3] = {M[24], M[25], M[26]};
            const float n1[3] = {q[0] - 0.0f, q[1] - 0.0f, q[2] - 0.0f}, n2[3] = {q[0] - O2[0], q[1] - O2[1], q[2] - O2[2]};
            const float dist1 = (float)in_norm3(n1), dist2 = (float)in_norm3(n2);
            const float cp = (float)(in_dotd(n1[0], n1[1], n1[2], n2[0], n2[1], n2[2]) / (double)(dist1 * dist2));
            const bool par = (double)cp < 0.99998;
            bool ok = !(q[2] <= 0.0f && par);
            float q2[3];
#pragma unroll
            for (int r = 0; r < 3; r++) q2[r] = in_affine(mode, M[3 * r], M[3 * r + 1], M[3 * r + 2], q[0], q[1], q[2], M[9 + r]);
            if (q2[2] <= 0.0f && par) ok = false;
            const float th2 = (float)(4.0 * (double)(Q.sigma * Q.sigma));
            const float invZ1 = (float)(1.0 / (double)q[2]);
            const float im1x = (fx * q[0]) * invZ1 + cx, im1y = (fy * q[1]) * invZ1 + cy;
            const float e1 = (im1x - m.x) * (im1x - m.x) + (im1y - m.y) * (im1y - m.y);
            if (e1 > th2) ok = false;
            const float invZ2 = (float)(1.0 / (double)q2[2]);
            const float im2x = (fx * q2[0]) * invZ2 + cx, im2y = (fy * q2[1]) * invZ2 + cy;
            const float e2 = (im2x - m.z) * (im2x - m.z) + (im2y - m.w) * (im2y - m.w);
            if (e2 > th2) ok = false;
            if (ok) { status = par ? 3 : 1; cosP = cp; p[0] = q[0]; p[1] = q[1]; p[2] = q[2]; }
        }
    }
    Q.st[slot] = status; Q.cosb[slot] = cosP;
    Q.p3[3 * slot] = p[0]; Q.p3[3 * slot + 1] = p[1]; Q.p3[3 * slot + 2] = p[2];
}

// a float's bit pattern as an unsigned key in the order of the values
__device__ __forceinline__ unsigned in_key(float f) { const unsigned u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float in_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__global__ __launch_bounds__(512) void k_init_finish(const InitDev* problems)
{
    __shared__ int s_good[8], s_sel[2];
    __shared__ float s_cos[8];
    const InitDev& Q = problems[blockIdx.x];
    InitResult& res = *Q.res;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, n = Q.n, n_mot = res.n_mot, model = res.model;
    {
        int good = 0;
        unsigned key = 0;
        if (wave < n_mot) {
            const unsigned char* st = Q.st + (size_t)wave * n;
            const float* cb = Q.cosb + (size_t)wave * n;
            for (int i = lane; i < n; i += 64) good += st[i] & 1;
            for (int d = 32; d >= 1; d >>= 1) good += __shfl_xor(good, d);
            if (good > 0) {
                const int k = min(50, good - 1);                                 // the k-th smallest: the largest T with fewer than k + 1 keys below it
                for (int bit = 31; bit >= 0; bit--) {
                    const unsigned cand = key | (1u << bit);
                    int cnt = 0;
                    for (int i = lane; i < n; i += 64) cnt += (st[i] & 1) && in_key(cb[i]) < cand;
                    for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d);
                    if (cnt <= k) key = cand;
                }
            }
        }
        if (lane == 0 && wave < 8) { s_good[wave] = good; s_cos[wave] = good > 0 ? in_unkey(key) : 0.0f; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int ret = 0, best = -1;
        bool pgt[8], pge[8];
        for (int k = 0; k < 8; k++) {
            const float c = s_cos[k];
            pgt[k] = s_good[k] > 0 ? (c >= -1.0f && c <= Q.cos_gt) : (0.0f > Q.min_par);
            pge[k] = s_good[k] > 0 ? (c >= -1.0f && c <= Q.cos_ge) : (0.0f >= Q.min_par);
        }
        const int N = res.N;
        if (model == 1 && n_mot == 4) {
            int maxGood = s_good[0];
            for (int k = 1; k < 4; k++) maxGood = max(maxGood, s_good[k]);
            const int nMinGood = max((int)(0.9 * (double)N), Q.min_tri);
            int nsimilar = 0;
            for (int k = 0; k < 4; k++) if ((double)s_good[k] > 0.7 * (double)maxGood) nsimilar++;
            if (!(maxGood < nMinGood || nsimilar > 1)) {
                for (int k = 0; k < 4; k++) if (s_good[k] == maxGood) { best = k; ret = pgt[k] ? 1 : 0; break; }     // the else-if chain: the first equal arm only
            }
        } else if (model == 0 && n_mot == 8) {
            int bestGood = 0, second = 0;
            for (int k = 0; k < 8; k++) {
                const int g = s_good[k];
                if (g > bestGood) { second = bestGood; bestGood = g; best = k; }
                else if (g > second) second = g;
            }
            ret = best >= 0 && (double)second < 0.75 * (double)bestGood && pge[best] && bestGood > Q.min_tri && (double)bestGood > 0.9 * (double)N;
        }
        res.returned = ret; res.best_mot = best;
        for (int k = 0; k < 8; k++) { res.mot_cos[k] = s_cos[k]; res.mot_good[k] = s_good[k]; }
        if (ret) {
            const float* M = Q.mot + best * INIT_MREC;
            for (int k = 0; k < 9; k++) res.R21[k] = M[k];
            res.t21[0] = M[9]; res.t21[1] = M[10]; res.t21[2] = M[11];
        }
        s_sel[0] = ret; s_sel[1] = best;
    }
    __syncthreads();
    const int ret = s_sel[0], best = s_sel[1];
    for (int i = threadIdx.x; i < n; i += 512) {
        float p[3] = {0.0f, 0.0f, 0.0f};
        unsigned char tr = 0;
        if (ret) {
            const size_t slot = (size_t)best * n + i;
            const unsigned char status = Q.st[slot];
            if (status & 1) { p[0] = Q.p3[3 * slot]; p[1] = Q.p3[3 * slot + 1]; p[2] = Q.p3[3 * slot + 2]; }
            tr = (status >> 1) & 1;
        }
        Q.p3d[3 * i] = p[0]; Q.p3d[3 * i + 1] = p[1]; Q.p3d[3 * i + 2] = p[2]; Q.tri[i] = tr;
    }
}

// ---------------------------------------------------------------------------------------------- host
// CheckRT's `parallax = acos(cos)*180/CV_PI` (:901) with the host's libm: acos of a float, times 180 in float, over CV_PI in double
static float init_parallax(float c) { return (float)((double)(std::acos(c) * 180) / 3.1415926535897932384626433832795); }
static unsigned init_hkey(float f) { unsigned u; memcpy(&u, &f, 4); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
static float init_hunkey(unsigned k) { const unsigned u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k; float f; memcpy(&f, &u, 4); return f; }
// the largest cosine in [-1, 1] whose parallax passes `> min_parallax` (or `>=`): parallax falls as the cosine rises, so the device's comparison of a
// cosine in [-1, 1] against this threshold is the reference's comparison of its parallax.  -2: no cosine passes.
// PRECONDITION (stated in include/orbhip.h): the host's acosf does not rise anywhere on [-1, 1]; the bisection finds ONE boundary.
static float init_cos_threshold(float min_parallax, bool or_equal)
{
    auto pass = [&](float c) { const float p = init_parallax(c); return or_equal ? p >= min_parallax : p > min_parallax; };
    if (!pass(-1.0f)) return -2.0f;
    if (pass(1.0f)) return 1.0f;
    unsigned lo = init_hkey(-1.0f), hi = init_hkey(1.0f);                        // pass(lo), !pass(hi)
    while (hi - lo > 1) { const unsigned mid = lo + (hi - lo) / 2; if (pass(init_hunkey(mid))) lo = mid; else hi = mid; }
    return init_hunkey(lo);
}

static orbhip_status init_problems(int device, int nproblems, orbhip_init_problem* problems, const char* who)
{
    OrbApiTimer api_timer;
    int max_sets = 0, max_n = 0;
    for (int p = 0; p < nproblems; p++) {
        const orbhip_init_problem& Q = problems[p];
        if (Q.gemm_mode == 2) return fail(ORBHIP_ERR_UNSUPPORTED, "%s: problem %d: gemm_mode 2 cannot be served: every product is per hypothesis on the device (DESIGN.md H19)", who, p);
        if (Q.gemm_mode != 0 && Q.gemm_mode != 1) return fail(ORBHIP_ERR_INVALID, "%s: problem %d: gemm_mode %d", who, p, Q.gemm_mode);
        if (Q.n < 8) return fail(ORBHIP_ERR_INVALID, "%s: problem %d: %d matches, a minimal set needs 8", who, p, Q.n);
        if (Q.n > INIT_MAX_N) return fail(ORBHIP_ERR_INVALID, "%s: problem %d: %d matches, at most %d a call", who, p, Q.n, INIT_MAX_N);
        if (Q.n_sets < 1 || Q.n_sets > INIT_MAX_SETS) return fail(ORBHIP_ERR_INVALID, "%s: problem %d: %d sets, 1 to %d a call", who, p, Q.n_sets, INIT_MAX_SETS);
        if (!Q.matches || !Q.sets || !Q.mask_h || !Q.mask_f || !Q.p3d || !Q.triangulated) return fail(ORBHIP_ERR_INVALID, "%s: problem %d: null pointer", who, p);
        for (int k = 0; k < 8 * Q.n_sets; k++)
            if (Q.sets[k] < 0 || Q.sets[k] >= Q.n) return fail(ORBHIP_ERR_INVALID, "%s: problem %d: set %d draws an index outside 0..%d", who, p, k / 8, Q.n - 1);
        max_sets = std::max(max_sets, Q.n_sets); max_n = std::max(max_n, Q.n);
    }
    if (nproblems == 0) return ORBHIP_OK;
    if (!device_present()) return fail(ORBHIP_ERR_HIP, "no HIP device available: no CPU fallback");
    HIPCHK(hipSetDevice(device));
    const hipStream_t s = orbhip_thread_stream(device);
    const int NL = nproblems;
    std::vector<InitDev> hP(NL); std::vector<InitResult> hA(NL);
    std::vector<std::vector<float> > hHyp(NL), hMot(NL);
    InitDev* dP = nullptr; InitResult* dA = nullptr;
    std::vector<float4*> dmatch(NL, nullptr); std::vector<int*> dsets(NL, nullptr);
    std::vector<float*> dhyp(NL, nullptr), dmot(NL, nullptr), dcos(NL, nullptr), dp3(NL, nullptr), dp3d(NL, nullptr);
    std::vector<unsigned long long*> dmask(NL, nullptr);
    std::vector<unsigned char*> dst(NL, nullptr), dmh(NL, nullptr), dmf(NL, nullptr), dtri(NL, nullptr);
    for (int k = 0; k < NL; k++) {
        const orbhip_init_problem& Q = problems[k];
        if (Q.hyp_score || Q.hyp_M) hHyp[k].resize((size_t)2 * Q.n_sets * INIT_HREC);
        if (Q.mot_R || Q.mot_t) hMot[k].resize((size_t)8 * INIT_MREC);
    }
    const hipError_t e = arena_call(device, s, [&](Arena& A) {
        A.io(&dP, (size_t)NL, (const InitDev*)hP.data(), (size_t)NL);
        for (int k = 0; k < NL; k++) {
            const orbhip_init_problem& Q = problems[k];
            A.io(&dmatch[k], (size_t)Q.n, reinterpret_cast<const float4*>(Q.matches), (size_t)Q.n);
            A.io(&dsets[k], (size_t)Q.n_sets * 8, (const int*)Q.sets, (size_t)Q.n_sets * 8);
        }
        A.io(&dA, (size_t)NL, (const InitResult*)nullptr, 0, hA.data(), (size_t)NL);
        for (int k = 0; k < NL; k++) {
            const orbhip_init_problem& Q = problems[k];
            A.io(&dmh[k], (size_t)Q.n, (const unsigned char*)nullptr, 0, (unsigned char*)Q.mask_h, (size_t)Q.n);
            A.io(&dmf[k], (size_t)Q.n, (const unsigned char*)nullptr, 0, (unsigned char*)Q.mask_f, (size_t)Q.n);
            A.io(&dp3d[k], (size_t)Q.n * 3, (const float*)nullptr, 0, (float*)Q.p3d, (size_t)Q.n * 3);
            A.io(&dtri[k], (size_t)Q.n, (const unsigned char*)nullptr, 0, (unsigned char*)Q.triangulated, (size_t)Q.n);
        }
        for (int k = 0; k < NL; k++) {                                          // the optional outputs and the scratch: behind what every call downloads
            const orbhip_init_problem& Q = problems[k];
            const size_t words = ((size_t)Q.n + 63) / 64;
            A.io(&dhyp[k], (size_t)2 * Q.n_sets * INIT_HREC, (const float*)nullptr, 0, hHyp[k].empty() ? (float*)nullptr : hHyp[k].data(), hHyp[k].size());
            A.io(&dmot[k], (size_t)8 * INIT_MREC, (const float*)nullptr, 0, hMot[k].empty() ? (float*)nullptr : hMot[k].data(), hMot[k].size());
            A.io(&dmask[k], (size_t)2 * Q.n_sets * words, (const unsigned long long*)nullptr, 0);
            A.io(&dcos[k], (size_t)8 * Q.n, (const float*)nullptr, 0);
            A.io(&dp3[k], (size_t)24 * Q.n, (const float*)nullptr, 0);
            A.io(&dst[k], (size_t)8 * Q.n, (const unsigned char*)nullptr, 0);
        }
        for (int k = 0; k < NL; k++) {                                          // (hP is read when the arena is uploaded, after this pass has filled in the addresses)
            const orbhip_init_problem& Q = problems[k]; InitDev& D = hP[k];
            D.matches = dmatch[k]; D.sets = dsets[k]; D.hyp = dhyp[k]; D.mask = dmask[k]; D.res = dA ? dA + k : nullptr; D.mot = dmot[k]; D.cosb = dcos[k];
            D.p3 = dp3[k]; D.st = dst[k]; D.mask_h = dmh[k]; D.mask_f = dmf[k]; D.p3d = dp3d[k]; D.tri = dtri[k];
            D.n = Q.n; D.n_sets = Q.n_sets; D.words = (Q.n + 63) / 64; D.mode = Q.gemm_mode; D.min_tri = Q.min_triangulated; D.pad = 0;
            memcpy(D.K, Q.K, sizeof D.K); D.sigma = Q.sigma; memcpy(D.norm1, Q.norm1, sizeof D.norm1); memcpy(D.norm2, Q.norm2, sizeof D.norm2);
            D.min_par = Q.min_parallax; D.cos_gt = init_cos_threshold(Q.min_parallax, false); D.cos_ge = init_cos_threshold(Q.min_parallax, true);
        }
    }, [&] {
        hipLaunchKernelGGL(k_init_hyp, dim3(2 * max_sets, NL, 1), dim3(64, 1, 1), 0, s, (const InitDev*)dP);
        hipLaunchKernelGGL(k_init_select, dim3(NL, 1, 1), dim3(64, 1, 1), 0, s, (const InitDev*)dP);
        hipLaunchKernelGGL(k_init_check_rt, dim3(8, (max_n + 63) / 64, NL), dim3(64, 1, 1), 0, s, (const InitDev*)dP);
        hipLaunchKernelGGL(k_init_finish, dim3(NL, 1, 1), dim3(512, 1, 1), 0, s, (const InitDev*)dP);
    });
    if (e != hipSuccess) return fail(ORBHIP_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    for (int k = 0; k < NL; k++) {
        orbhip_init_problem& Q = problems[k]; const InitResult& r = hA[k];
        Q.returned = r.returned; Q.model = r.model; Q.best_h = r.best_h; Q.best_f = r.best_f; Q.n_mot = r.n_mot; Q.best_mot = r.best_mot;
        Q.SH = r.SH; Q.SF = r.SF;
        memcpy(Q.H21, r.H21, sizeof Q.H21); memcpy(Q.F21, r.F21, sizeof Q.F21); memcpy(Q.R21, r.R21, sizeof Q.R21); memcpy(Q.t21, r.t21, sizeof Q.t21);
        memcpy(Q.mot_cos, r.mot_cos, sizeof Q.mot_cos); memcpy(Q.mot_good, r.mot_good, sizeof Q.mot_good);
        for (int h = 0; h < 2 * Q.n_sets && !hHyp[k].empty(); h++) {
            const float* o = hHyp[k].data() + (size_t)h * INIT_HREC;
            if (Q.hyp_M) memcpy(Q.hyp_M + 9 * (size_t)h, o, 9 * sizeof(float));
            if (Q.hyp_score) Q.hyp_score[h] = o[9];
        }
        for (int j = 0; j < 8 && !hMot[k].empty(); j++) {                       // rows past n_mot: zero
            const float* o = hMot[k].data() + (size_t)j * INIT_MREC;
            if (Q.mot_R) { if (j < r.n_mot) memcpy(Q.mot_R + 9 * j, o, 9 * sizeof(float)); else memset(Q.mot_R + 9 * j, 0, 9 * sizeof(float)); }
            if (Q.mot_t) { if (j < r.n_mot) memcpy(Q.mot_t + 3 * j, o + 9, 3 * sizeof(float)); else memset(Q.mot_t + 3 * j, 0, 3 * sizeof(float)); }
        }
    }
    return ORBHIP_OK;
}

extern "C" orbhip_status orbhip_init_reconstruct_batch(int device, int nproblems, orbhip_init_problem* problems)
{
    if (nproblems < 0 || (nproblems > 0 && !problems)) return fail(ORBHIP_ERR_INVALID, "init_reconstruct_batch: bad argument");
    return init_problems(device, nproblems, problems, "init_reconstruct_batch");
}

extern "C" orbhip_status orbhip_init_reconstruct(int device, orbhip_init_problem* problem)
{
    if (!problem) return fail(ORBHIP_ERR_INVALID, "init_reconstruct: null problem");
    return init_problems(device, 1, problem, "init_reconstruct");
}
