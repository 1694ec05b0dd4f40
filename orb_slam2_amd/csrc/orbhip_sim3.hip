// orbhip_sim3.hip — Sim3Solver::iterate (Sim3Solver.cc:140-207) for one solver or one round of several, in two launches: every drawn hypothesis of every
// problem is solved (ComputeSim3, :226-337) and checked against all correspondences (CheckInliers / Project, :340-403) at once, then the RANSAC loop's
// bookkeeping (`>= best` is a new best, `> min_inliers` on a new best returns) is replayed over the counts in hypothesis order.  The arithmetic is
// DESIGN.md H17, restated in tests/sim3_model.py: float wherever the reference holds a CV_32F Mat or a float member, double in between.
//
//   k_sim3_hyp      one wave per (hypothesis, problem).  Horn's closed form from the three drawn correspondences runs uniformly on all 64 lanes (a wave
//                   executes it once either way; nothing has to be broadcast): centroids, M, the 4 x 4 N, its largest eigenvector by cyclic Jacobi
//                   (orbhip_jacobi.h), angle-axis, Rodrigues, scale, translation, T12 and T21.  The lanes then stride over the problem's correspondences
//                   (32 bytes each, contiguous by lane), project both ways, recompute the image points and integer thresholds of FromCameraToImage and
//                   the constructor (one division against two more streams of loads), test both errors and ballot; lane 0 stores the 64-bit mask words
//                   and the record R12 | t12 | s12 | count.
//   k_sim3_select   one wave per problem: 64 counts a pass, a prefix maximum by shuffles, two ballots.  Writes the fixed result record and expands the
//                   best hypothesis' mask to one byte per correspondence.
// No device state survives a call, no floating-point atomics, every loop is bounded by n, n_hyp or a constant, whatever the numbers are: a non-finite
// hypothesis fails every comparison and has 0 inliers, as in the reference.
#include "orbhip_ctx.h"
#include "orbhip_jacobi.h"
#include <cfloat>

#define S3_MAX_HYP 4096
#define S3_REC 16                      // floats per hypothesis record: R12[9] t12[3] s12 count(int) pad pad

struct Sim3Result { int n_consumed, returned, best, best_inliers; float T12[16], R12[9], t12[3], s12; int pad[3]; };
struct Sim3Dev {
    const orbhip_sim3_corr* corr; const int* triples; float* hyp; unsigned long long* mask; Sim3Result* res; unsigned char* inliers;
    int n, n_hyp, words, fix_scale, gemm_mode, min_inliers, best_in, pad;
    float K1[4], K2[4];
};

// one entry of a CV_32F product with inner length 3: mode 0 sums the products in double from 0 and rounds once (include/cvlite,
// cv::gemm's generic kernel), mode 1 sums them in float (cv::gemm's small-matrix path)
__device__ __forceinline__ double s3_dot_d(float a0, float a1, float a2, float b0, float b1, float b2)
{
    double s = 0.0;
    s += (double)a0 * (double)b0; s += (double)a1 * (double)b1; s += (double)a2 * (double)b2;
    return s;
}
__device__ __forceinline__ float s3_dot_f(float a0, float a1, float a2, float b0, float b1, float b2)
{
    float t0 = a0 * b0;
    t0 = t0 + a1 * b1; t0 = t0 + a2 * b2;
    return t0;
}
__device__ __forceinline__ float s3_mul(int mode, float a0, float a1, float a2, float b0, float b1, float b2)
{
    return mode == 1 ? s3_dot_f(a0, a1, a2, b0, b1, b2) : (float)s3_dot_d(a0, a1, a2, b0, b1, b2);
}
// `R*x + t` as one expression: mode 0 adds t in float after the rounding, mode 1 folds it in (alpha = beta = 1, in double)
__device__ __forceinline__ float s3_affine(int mode, float a0, float a1, float a2, float b0, float b1, float b2, float t)
{
    if (mode == 1) return (float)((double)s3_dot_f(a0, a1, a2, b0, b1, b2) + (double)t);
    return (float)s3_dot_d(a0, a1, a2, b0, b1, b2) + t;
}

// ComputeCentroid: C = cv::reduce(P, 1, SUM) / 3; Pr.col(i) = P.col(i) - C.  P[r][i]: coordinate r of point i.
__device__ __forceinline__ void s3_centroid(const float P[3][3], float Pr[3][3], float C[3])
{
#pragma unroll
    for (int r = 0; r < 3; r++) {
        C[r] = ((P[r][0] + P[r][1]) + P[r][2]) / 3.0f;
#pragma unroll
        for (int i = 0; i < 3; i++) Pr[r][i] = P[r][i] - C[r];
    }
}

// ComputeSim3 up to mt12i
__device__ static void s3_horn(const float P1[3][3], const float P2[3][3], int fix_scale, int mode, float R[9], float t[3], float& s12)
{
    float Pr1[3][3], Pr2[3][3], O1[3], O2[3], M[3][3];
    s3_centroid(P1, Pr1, O1);
    s3_centroid(P2, Pr2, O2);
    // M = Pr2 * Pr1.t(): the product carries a transposition flag, which the small-matrix path excludes - the generic kernel in both modes
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) M[r][c] = (float)s3_dot_d(Pr2[r][0], Pr2[r][1], Pr2[r][2], Pr1[c][0], Pr1[c][1], Pr1[c][2]);
    // N11 .. N44: float expressions (both operands are float), held in doubles, stored to a CV_32F Mat: the values are the float expressions'
    const float N11 = M[0][0] + M[1][1] + M[2][2], N12 = M[1][2] - M[2][1], N13 = M[2][0] - M[0][2], N14 = M[0][1] - M[1][0];
    const float N22 = M[0][0] - M[1][1] - M[2][2], N23 = M[0][1] + M[1][0], N24 = M[2][0] + M[0][2];
    const float N33 = -M[0][0] + M[1][1] - M[2][2], N34 = M[1][2] + M[2][1], N44 = -M[0][0] - M[1][1] + M[2][2];
    double A[4][4] = {{N11, N12, N13, N14}, {N12, N22, N23, N24}, {N13, N23, N33, N34}, {N14, N24, N34, N44}}, V[4][4], w[4], qd[4];
    orbhip_jacobi_eigen<4>(A, V, w);
    orbhip_jacobi_largest<4>(V, w, qd);
    if (qd[0] < 0.0) { qd[0] = -qd[0]; qd[1] = -qd[1]; qd[2] = -qd[2]; qd[3] = -qd[3]; }          // q and -q are the same rotation, not the same bits
    const float q0 = (float)qd[0], v0 = (float)qd[1], v1 = (float)qd[2], v2 = (float)qd[3];     // evec is CV_32F
    double nrm = 0.0;
    nrm += (double)v0 * (double)v0; nrm += (double)v1 * (double)v1; nrm += (double)v2 * (double)v2;
    nrm = sqrt(nrm);
    const double ang = atan2(nrm, (double)q0);
    const float f2a = (float)(2.0 * ang), fn = (float)nrm;                                      // vec = 2*ang*vec/norm(vec)
    const float r0 = (f2a * v0) / fn, r1 = (f2a * v1) / fn, r2 = (f2a * v2) / fn;
    // cv::Rodrigues, vector to matrix
    const double rx = (double)r0, ry = (double)r1, rz = (double)r2;
    const double theta = sqrt(rx * rx + ry * ry + rz * rz);
    if (theta < DBL_EPSILON) {
#pragma unroll
        for (int k = 0; k < 9; k++) R[k] = k % 4 == 0 ? 1.0f : 0.0f;
    } else {
        const double c = cos(theta), s = sin(theta), c1 = 1.0 - c, itheta = 1.0 / theta;
        const double k[3] = {rx * itheta, ry * itheta, rz * itheta};
        const double X[9] = {0.0, -k[2], k[1], k[2], 0.0, -k[0], -k[1], k[0], 0.0};
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) R[3 * i + j] = (float)((c * (i == j ? 1.0 : 0.0) + c1 * (k[i] * k[j])) + s * X[3 * i + j]);
    }
    // P3 = mR12i * Pr2; the scale
    if (!fix_scale) {
        double nom = 0.0, den = 0.0;
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int i = 0; i < 3; i++) {
                const float p3 = s3_mul(mode, R[3 * r], R[3 * r + 1], R[3 * r + 2], Pr2[0][i], Pr2[1][i], Pr2[2][i]);
                nom += (double)Pr1[r][i] * (double)p3;
                den += (double)(p3 * p3);
            }
        s12 = (float)(nom / den);
    } else s12 = 1.0f;
    // mt12i = O1 - ms12i*mR12i*O2
#pragma unroll
    for (int r = 0; r < 3; r++) {
        if (mode == 1) t[r] = (float)((double)s3_dot_f(R[3 * r], R[3 * r + 1], R[3 * r + 2], O2[0], O2[1], O2[2]) * (-(double)s12) + (double)O1[r]);
        else t[r] = O1[r] - (float)s3_dot_d(s12 * R[3 * r], s12 * R[3 * r + 1], s12 * R[3 * r + 2], O2[0], O2[1], O2[2]);
    }
}

// Steps 8.1 and 8.2: the 3 x 4 tops of mT12i and mT21i (A[4r + c]; column 3 is the translation)
__device__ __forceinline__ void s3_transforms(const float R[9], const float t[3], float s12, int mode, float T12[12], float T21[12])
{
    const float inv = (float)(1.0 / (double)s12);
    float sRinv[9];
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) { T12[4 * r + c] = s12 * R[3 * r + c]; sRinv[3 * r + c] = inv * R[3 * c + r]; T21[4 * r + c] = sRinv[3 * r + c]; }
        T12[4 * r + 3] = t[r];
    }
#pragma unroll
    for (int r = 0; r < 3; r++) T21[4 * r + 3] = -s3_mul(mode, sRinv[3 * r], sRinv[3 * r + 1], sRinv[3 * r + 2], t[0], t[1], t[2]);       // tinv = -sRinv*mt12i
}

// Project: P3Dc = Rcw*X + tcw; invz = 1/z; (fx x invz + cx, fy y invz + cy).  FromCameraToImage is the same on the point itself.
__device__ __forceinline__ void s3_image(float X, float Y, float Z, const float K[4], float& u, float& v)
{
    const float invz = 1.0f / Z;
    const float x = X * invz, y = Y * invz;
    u = K[0] * x + K[2]; v = K[1] * y + K[3];
}
__device__ __forceinline__ void s3_project(const float T[12], int mode, float X, float Y, float Z, const float K[4], float& u, float& v)
{
    const float x = s3_affine(mode, T[0], T[1], T[2], X, Y, Z, T[3]);
    const float y = s3_affine(mode, T[4], T[5], T[6], X, Y, Z, T[7]);
    const float z = s3_affine(mode, T[8], T[9], T[10], X, Y, Z, T[11]);
    s3_image(x, y, z, K, u, v);
}
// err = dist.dot(dist) (double sum, to float) < (float)(size_t)(9.210 * sigma2)
__device__ __forceinline__ bool s3_within(float u0, float v0, float u1, float v1, float sigma2)
{
    const float du = u0 - u1, dv = v0 - v1;
    double e = 0.0;
    e += (double)du * (double)du; e += (double)dv * (double)dv;
    const float thr = (float)(unsigned long long)(9.210 * (double)sigma2);
    return (float)e < thr;
}

__global__ __launch_bounds__(64) void k_sim3_hyp(const Sim3Dev* problems)
{
    const Sim3Dev& Q = problems[blockIdx.y];
    const int h = blockIdx.x, lane = threadIdx.x, n = Q.n, mode = Q.gemm_mode;
    if (h >= Q.n_hyp) return;
    float P1[3][3], P2[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int idx = Q.triples[3 * h + i];                                  // checked by the host: 0 .. n - 1
        const orbhip_sim3_corr c = Q.corr[idx];
        P1[0][i] = c.X1[0]; P1[1][i] = c.X1[1]; P1[2][i] = c.X1[2];
        P2[0][i] = c.X2[0]; P2[1][i] = c.X2[1]; P2[2][i] = c.X2[2];
    }
    float R[9], t[3], s12, T12[12], T21[12];
    s3_horn(P1, P2, Q.fix_scale, mode, R, t, s12);
    s3_transforms(R, t, s12, mode, T12, T21);
    const float K1[4] = {Q.K1[0], Q.K1[1], Q.K1[2], Q.K1[3]}, K2[4] = {Q.K2[0], Q.K2[1], Q.K2[2], Q.K2[3]};
    unsigned long long* mask = Q.mask + (size_t)h * Q.words;
    int count = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        bool in = false;
        if (i < n) {
            const float4* p = reinterpret_cast<const float4*>(Q.corr + i);
            const float4 a = p[0], b = p[1];                                    // X1 = a.xyz, X2 = a.w b.xy, sigma2_1 = b.z, sigma2_2 = b.w
            float u11, v11, u22, v22, u21, v21, u12, v12;
            s3_image(a.x, a.y, a.z, K1, u11, v11);                              // mvP1im1
            s3_image(a.w, b.x, b.y, K2, u22, v22);                              // mvP2im2
            s3_project(T12, mode, a.w, b.x, b.y, K1, u21, v21);                 // vP2im1
            s3_project(T21, mode, a.x, a.y, a.z, K2, u12, v12);                 // vP1im2
            const bool e1 = s3_within(u11, v11, u21, v21, b.z), e2 = s3_within(u12, v12, u22, v22, b.w);
            in = e1 && e2;
        }
        const unsigned long long m = __ballot(in);
        if (lane == 0) mask[base >> 6] = m;
        count += __popcll(m);
    }
    if (lane == 0) {
        float* o = Q.hyp + (size_t)h * S3_REC;
#pragma unroll
        for (int k = 0; k < 9; k++) o[k] = R[k];
        o[9] = t[0]; o[10] = t[1]; o[11] = t[2]; o[12] = s12;
        reinterpret_cast<int*>(o)[13] = count;
    }
}

__global__ __launch_bounds__(64) void k_sim3_select(const Sim3Dev* problems)
{
    const Sim3Dev& Q = problems[blockIdx.x];
    const int lane = threadIdx.x, nh = Q.n_hyp, n = Q.n;
    int run = Q.best_in, best = -1, returned = -1, consumed = nh;               // run: mnBestInliers before the hypothesis at hand
    for (int base = 0; base < nh; base += 64) {
        const int h = base + lane;
        const int c = h < nh ? reinterpret_cast<const int*>(Q.hyp + (size_t)h * S3_REC)[13] : -1;
        int incl = c;                                                          // inclusive prefix maximum over the lanes
        for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(incl, d); if (lane >= d) incl = max(incl, o); }
        int before = __shfl_up(incl, 1);
        before = lane == 0 ? run : max(run, before);
        const bool is_new = h < nh && c >= before;
        const unsigned long long new_m = __ballot(is_new), ret_m = __ballot(is_new && c > Q.min_inliers);
        if (ret_m) {
            const int l = __ffsll((long long)ret_m) - 1;
            returned = best = base + l; consumed = returned + 1;
            run = __shfl(c, l);
            break;
        }
        if (new_m) { const int l = 63 - __clzll((long long)new_m); best = base + l; }
        run = max(run, __shfl(incl, 63));
    }
    if (best >= 0) {
        const unsigned long long* mask = Q.mask + (size_t)best * Q.words;
        for (int i = lane; i < n; i += 64) Q.inliers[i] = (unsigned char)((mask[i >> 6] >> (i & 63)) & 1ull);
    }
    if (lane == 0) {
        Sim3Result& r = *Q.res;
        r.n_consumed = consumed; r.returned = returned; r.best = best; r.best_inliers = run;
        if (best >= 0) {
            const float* o = Q.hyp + (size_t)best * S3_REC;
            const float s12 = o[12];
            for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) { r.T12[4 * i + j] = s12 * o[3 * i + j]; r.R12[3 * i + j] = o[3 * i + j]; } r.T12[4 * i + 3] = o[9 + i]; r.t12[i] = o[9 + i]; }
            r.T12[12] = 0.0f; r.T12[13] = 0.0f; r.T12[14] = 0.0f; r.T12[15] = 1.0f;
            r.s12 = s12;
        }
    }
}

// ---------------------------------------------------------------------------------------------- host
static orbhip_status sim3_problems(int device, int nproblems, orbhip_sim3_problem* problems, const char* who)
{
    OrbApiTimer api_timer;
    std::vector<int> live;
    int max_hyp = 0;
    for (int p = 0; p < nproblems; p++) {
        orbhip_sim3_problem& Q = problems[p];
        if (Q.n < 0 || Q.n_hyp < 0) return fail(ORBHIP_ERR_INVALID, "%s: problem %d: negative size", who, p);
        if (Q.n_hyp > S3_MAX_HYP) return fail(ORBHIP_ERR_INVALID, "%s: problem %d: %d hypotheses, at most %d a call", who, p, Q.n_hyp, S3_MAX_HYP);
        if (Q.gemm_mode == 2) return fail(ORBHIP_ERR_UNSUPPORTED, "%s: problem %d: gemm_mode 2 cannot be served: every product is per hypothesis on the device (DESIGN.md H17)", who, p);
        if (Q.gemm_mode != 0 && Q.gemm_mode != 1) return fail(ORBHIP_ERR_INVALID, "%s: problem %d: gemm_mode %d", who, p, Q.gemm_mode);
        if (Q.n < 3 || Q.n_hyp == 0) continue;
        if (!Q.corr || !Q.triples || !Q.inliers) return fail(ORBHIP_ERR_INVALID, "%s: problem %d: null pointer", who, p);
        for (int h = 0; h < Q.n_hyp; h++) {
            const int32_t a = Q.triples[3 * h], b = Q.triples[3 * h + 1], c = Q.triples[3 * h + 2];
            if (a < 0 || a >= Q.n || b < 0 || b >= Q.n || c < 0 || c >= Q.n) return fail(ORBHIP_ERR_INVALID, "%s: problem %d: hypothesis %d draws an index outside 0..%d", who, p, h, Q.n - 1);
            if (a == b || a == c || b == c) return fail(ORBHIP_ERR_INVALID, "%s: problem %d: hypothesis %d draws an index twice", who, p, h);
        }
    }
    for (int p = 0; p < nproblems; p++) {
        orbhip_sim3_problem& Q = problems[p];
        Q.n_consumed = 0; Q.returned = -1; Q.best = -1;
        if (Q.n >= 3 && Q.n_hyp > 0) { live.push_back(p); max_hyp = std::max(max_hyp, Q.n_hyp); }
    }
    if (live.empty()) return ORBHIP_OK;
    if (!device_present()) return fail(ORBHIP_ERR_HIP, "no HIP device available: no CPU fallback");
    HIPCHK(hipSetDevice(device));
    const hipStream_t s = orbhip_thread_stream(device);
    const int NL = (int)live.size();
    std::vector<Sim3Dev> hP(NL); std::vector<Sim3Result> hA(NL);
    std::vector<std::vector<unsigned char> > hIn(NL);
    std::vector<std::vector<float> > hHyp(NL);
    Sim3Dev* dP = nullptr; Sim3Result* dA = nullptr;
    std::vector<orbhip_sim3_corr*> dcorr(NL, nullptr); std::vector<int*> dtri(NL, nullptr); std::vector<float*> dhyp(NL, nullptr);
    std::vector<unsigned long long*> dmask(NL, nullptr); std::vector<unsigned char*> din(NL, nullptr);
    for (int k = 0; k < NL; k++) {
        const orbhip_sim3_problem& Q = problems[live[k]];
        hIn[k].resize((size_t)Q.n);
        if (Q.hyp_R || Q.hyp_t || Q.hyp_s || Q.hyp_count) hHyp[k].resize((size_t)Q.n_hyp * S3_REC);
    }
    const hipError_t e = arena_call(device, s, [&](Arena& A) {
        A.io(&dP, (size_t)NL, (const Sim3Dev*)hP.data(), (size_t)NL);
        for (int k = 0; k < NL; k++) {
            const orbhip_sim3_problem& Q = problems[live[k]];
            A.io(&dcorr[k], (size_t)Q.n, Q.corr, (size_t)Q.n);
            A.io(&dtri[k], (size_t)Q.n_hyp * 3, (const int*)Q.triples, (size_t)Q.n_hyp * 3);
        }
        A.io(&dA, (size_t)NL, (const Sim3Result*)nullptr, 0, hA.data(), (size_t)NL);
        for (int k = 0; k < NL; k++) {
            const orbhip_sim3_problem& Q = problems[live[k]];
            const size_t words = ((size_t)Q.n + 63) / 64;
            A.io(&din[k], (size_t)Q.n, (const unsigned char*)nullptr, 0, hIn[k].data(), (size_t)Q.n);
            A.io(&dhyp[k], (size_t)Q.n_hyp * S3_REC, (const float*)nullptr, 0, hHyp[k].empty() ? (float*)nullptr : hHyp[k].data(), hHyp[k].size());
            A.io(&dmask[k], (size_t)Q.n_hyp * words, (const unsigned long long*)nullptr, 0, (unsigned long long*)Q.hyp_mask, Q.hyp_mask ? (size_t)Q.n_hyp * words : 0);
        }
        for (int k = 0; k < NL; k++) {                                          // (hP is read when the arena is uploaded, after this pass has filled in the addresses)
            const orbhip_sim3_problem& Q = problems[live[k]]; Sim3Dev& D = hP[k];
            D.corr = dcorr[k]; D.triples = dtri[k]; D.hyp = dhyp[k]; D.mask = dmask[k]; D.res = dA ? dA + k : nullptr; D.inliers = din[k];
            D.n = Q.n; D.n_hyp = Q.n_hyp; D.words = (Q.n + 63) / 64; D.fix_scale = Q.fix_scale ? 1 : 0; D.gemm_mode = Q.gemm_mode;
            D.min_inliers = Q.min_inliers; D.best_in = Q.best_inliers_in; D.pad = 0;
            memcpy(D.K1, Q.K1, sizeof D.K1); memcpy(D.K2, Q.K2, sizeof D.K2);
        }
    }, [&] {
        hipLaunchKernelGGL(k_sim3_hyp, dim3(max_hyp, NL, 1), dim3(64, 1, 1), 0, s, (const Sim3Dev*)dP);
        hipLaunchKernelGGL(k_sim3_select, dim3(NL, 1, 1), dim3(64, 1, 1), 0, s, (const Sim3Dev*)dP);
    });
    if (e != hipSuccess) return fail(ORBHIP_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    for (int k = 0; k < NL; k++) {
        orbhip_sim3_problem& Q = problems[live[k]]; const Sim3Result& r = hA[k];
        Q.n_consumed = r.n_consumed; Q.returned = r.returned; Q.best = r.best; Q.best_inliers_out = r.best_inliers;
        if (r.best >= 0) {
            memcpy(Q.T12, r.T12, sizeof Q.T12); memcpy(Q.R12, r.R12, sizeof Q.R12); memcpy(Q.t12, r.t12, sizeof Q.t12); Q.s12 = r.s12;
            memcpy(Q.inliers, hIn[k].data(), (size_t)Q.n);
        }
        for (int h = 0; h < Q.n_hyp && !hHyp[k].empty(); h++) {
            const float* o = hHyp[k].data() + (size_t)h * S3_REC;
            if (Q.hyp_R) memcpy(Q.hyp_R + 9 * (size_t)h, o, 9 * sizeof(float));
            if (Q.hyp_t) memcpy(Q.hyp_t + 3 * (size_t)h, o + 9, 3 * sizeof(float));
            if (Q.hyp_s) Q.hyp_s[h] = o[12];
            if (Q.hyp_count) memcpy(Q.hyp_count + h, o + 13, sizeof(int32_t));
        }
    }
    return ORBHIP_OK;
}

extern "C" orbhip_status orbhip_sim3_iterate_batch(int device, int nproblems, orbhip_sim3_problem* problems)
{
    if (nproblems < 0 || (nproblems > 0 && !problems)) return fail(ORBHIP_ERR_INVALID, "sim3_iterate_batch: bad argument");
    return sim3_problems(device, nproblems, problems, "sim3_iterate_batch");
}

extern "C" orbhip_status orbhip_sim3_iterate(int device, orbhip_sim3_problem* problem)
{
    if (!problem) return fail(ORBHIP_ERR_INVALID, "sim3_iterate: null problem");
    return sim3_problems(device, 1, problem, "sim3_iterate");
}
