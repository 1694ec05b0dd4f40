// orbhip_sim3_opt.hip — Optimizer::OptimizeSim3 (Optimizer.cc:1046-1241) in one launch: one free Sim(3) vertex, for each of n matched pairs a forward edge
// (EdgeSim3ProjectXYZ: X2 through S12 into camera 1) and an inverse edge (EdgeInverseSim3ProjectXYZ: X1 through S12^-1 into camera 2), Huber kernel on both in
// both phases, optimize(5), removal of every pair with either chi2 > th2, optimize(10) or optimize(5), second check - as g2o runs them
// (OptimizationAlgorithmLevenberg::solve, SparseOptimizer::optimize, BaseBinaryEdge::linearizeOplus / constructQuadraticForm with a fixed first vertex,
// RobustKernelHuber, LinearSolverDense, Sim3, VertexSim3Expmap).  Everything is double; the pairs and the cameras are float.
//
//   numerical Jacobians  the two edge types have no linearizeOplus of their own, so g2o differentiates them: column d = (e(Sim3(+1e-9 e_d) * estimate) -
//                     e(Sim3(-1e-9 e_d) * estimate)) / 2e-9.  The 14 perturbed estimates and their inverses are the same for every edge: 14 threads compute
//                     one each per evaluation and publish them through LDS (s_xf), beside the estimate and its inverse that thread 0 publishes.  A last-bit
//                     difference in a perturbed transform is multiplied by 5e8, hence -ffp-contract=off for this file and no re-association anywhere.
//   k_sim3_opt<T>     one workgroup of T threads per problem, both phases.  Thread t owns pairs t, t + T, ...  A SYSTEM evaluation: every thread walks its
//                     live pairs, 15 map + project + cam_map per edge, the 2 x 7 Jacobians, the Huber weight, and keeps S3O_SUMS = 36 running sums - the 28
//                     upper entries of H, the 7 of b, rho_0; a CHI evaluation keeps rho_0 alone (2 maps per pair).  Sums are added across the wave by a
//                     shuffle butterfly, written per wave to LDS and added across waves by thread 0 in a fixed tree: the order of every addition follows
//                     from n and T alone.  Thread 0 is the LM driver: accept / reject, lambda, the 7 x 7 LDL^T solve, Sim3(x) * estimate.
//   when the system is built   AFTER ACCEPTANCE (S3O_SYSTEM_EVERY_TRIAL = 0, the shipped choice): a trial evaluates chi2 alone and every iteration starts
//                     with one system evaluation at the estimate, as g2o itself does.  The other choice (= 1: every trial a system evaluation, an accepted
//                     trial's system reused as in k_pose_opt) gives the same bits - g2o rebuilds the system at the same estimate - and is kept behind the macro
//                     for tools/sim3_opt_rate.py, which measured both (profiles/sim3_opt_rate.json).
//   per-pair state    one byte: removed.  In LDS while the problem is staged (copied to the caller's array at the end), in that array itself beyond.  The
//                     checks read the errors the phase's last computeActiveErrors left (S3oState::last: the rejected trial's estimate if the phase ended on
//                     one); linearizeOplus restores _error, so the differentiation does not disturb them.  Errors are recomputed there, not stored.
//                     Pairs are staged in LDS up to S3O_STAGE_MAX (48 bytes each) and read through L2 beyond.
//   fixed scale       oplusImpl zeroes update[6] before Sim3(update): both perturbations of column 6 are the estimate itself, the column is exactly 0, H66 is
//                     lambda alone, and the scale keeps its bits (exp(0) * s).
// No loop depends on the data for its bound: 2 phases x 10 iterations x 10 trials, each a compile-time limit.  No floating-point atomics.
#include "orbhip_ctx.h"
#include <cfloat>

#define S3O_SUMS 36
#define S3O_STAGE_MAX 1024             // pairs staged in LDS: 48 KB of the 160 KB, so that three problems of a batch can share a CU; loop candidates have a few hundred pairs
#ifndef S3O_T
#define S3O_T 256                      // threads per workgroup: the measured choice among 64, 128, 256 and 512; a compile-time constant
#endif
#ifndef S3O_SYSTEM_EVERY_TRIAL
#define S3O_SYSTEM_EVERY_TRIAL 0
#endif
#define S3O_NXF 30                     // published transforms: estimate, inverse, then for k = 2d + (minus ? 1 : 0): perturbed [2 + 2k], its inverse [3 + 2k]

struct S3o { double qx, qy, qz, qw, tx, ty, tz, s; };                         // g2o::Sim3: r (NOT normalised), t, s
struct Sim3OptProblem {
    const orbhip_sim3_pair* pairs; unsigned char* removed; double* S12_out; int* n_inliers;
    int n, fix_scale; float th2; float cam[8]; double S12[8];
};
// thread 0's state between two evaluations (LDS), and what it publishes to the workgroup
struct S3oState {
    S3o cur, trial, last;              // the estimate; the trial just evaluated; the estimate of the phase's last computeActiveErrors
    double H[28], b[7], chi;           // the system and activeRobustChi2 at cur
    double x[7];                       // the solver's x (a failed solve leaves it as it was; oplusImpl zeroes x[6] under fix_scale)
    double lambda, ni, ini_chi;
    int n_bad_steps, ok2, more_trials, more_iters, n_bad, n_in;
};

__device__ __forceinline__ int s3o_idx(int j, int k) { return j * 7 - j * (j - 1) / 2 + (k - j); }     // (j <= k) of the 28 upper entries, row by row

// Eigen: Quaternion(Matrix3) - no normalisation follows it in Sim3
__device__ static void s3o_quat_of_matrix(const double m[9], S3o& P)
{
    double t = m[0] + m[4] + m[8], q[4];
    if (t > 0.0) {
        t = sqrt(t + 1.0); q[3] = 0.5 * t; t = 0.5 / t;
        q[0] = (m[7] - m[5]) * t; q[1] = (m[2] - m[6]) * t; q[2] = (m[3] - m[1]) * t;
    } else {
        int i = 0;
        if (m[4] > m[0]) i = 1;
        if (m[8] > m[i * 4]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = sqrt(m[i * 4] - m[j * 4] - m[k * 4] + 1.0);
        q[i] = 0.5 * t; t = 0.5 / t;
        q[3] = (m[k * 3 + j] - m[j * 3 + k]) * t; q[j] = (m[j * 3 + i] + m[i * 3 + j]) * t; q[k] = (m[k * 3 + i] + m[i * 3 + k]) * t;
    }
    P.qx = q[0]; P.qy = q[1]; P.qz = q[2]; P.qw = q[3];
}
// Eigen: Quaternion * Vector3
__device__ __forceinline__ void s3o_rotate(double qx, double qy, double qz, double qw, double X, double Y, double Z, double& x, double& y, double& z)
{
    double ux = qy * Z - qz * Y, uy = qz * X - qx * Z, uz = qx * Y - qy * X;
    ux += ux; uy += uy; uz += uz;
    x = X + qw * ux + (qy * uz - qz * uy);
    y = Y + qw * uy + (qz * ux - qx * uz);
    z = Z + qw * uz + (qx * uy - qy * ux);
}
// Sim3::map: s * (r * xyz) + t
__device__ __forceinline__ void s3o_map(const S3o& S, double X, double Y, double Z, double& x, double& y, double& z)
{
    s3o_rotate(S.qx, S.qy, S.qz, S.qw, X, Y, Z, x, y, z);
    x = S.s * x + S.tx; y = S.s * y + S.ty; z = S.s * z + S.tz;
}
// Sim3::inverse: Sim3(r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s)
__device__ static void s3o_inverse(const S3o& S, S3o& I)
{
    const double k = -1.0 / S.s;
    double x, y, z;
    s3o_rotate(-S.qx, -S.qy, -S.qz, S.qw, k * S.tx, k * S.ty, k * S.tz, x, y, z);
    I.qx = -S.qx; I.qy = -S.qy; I.qz = -S.qz; I.qw = S.qw; I.tx = x; I.ty = y; I.tz = z; I.s = 1.0 / S.s;
}
// Sim3(const Vector7d& update): omega | upsilon | sigma, four branches
__device__ static void s3o_exp(const double* u, S3o& E)
{
    const double ox = u[0], oy = u[1], oz = u[2], sigma = u[6];
    const double theta = sqrt(ox * ox + oy * oy + oz * oz);
    const double O[9] = {0.0, -oz, oy, oz, 0.0, -ox, -oy, ox, 0.0};
    double O2[9], R[9], A, B, C;
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) O2[i * 3 + j] = O[i * 3] * O[j] + O[i * 3 + 1] * O[3 + j] + O[i * 3 + 2] * O[6 + j];
    const double s = exp(sigma), eps = 0.00001;
    const bool small_theta = theta < eps;
    double sn = 0.0, cs = 0.0;
    if (!small_theta) { sn = sin(theta); cs = cos(theta); }
    if (fabs(sigma) < eps) {
        C = 1.0;
        if (small_theta) { A = 1.0 / 2.0; B = 1.0 / 6.0; }
        else { const double theta2 = theta * theta; A = (1.0 - cs) / theta2; B = (theta - sn) / (theta2 * theta); }
    } else {
        C = (s - 1.0) / sigma;
        if (small_theta) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1.0) * s + 1.0) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1.0) * s) / (sigma2 * sigma);
        } else {
            const double a = s * sn, b = s * cs, theta2 = theta * theta, sigma2 = sigma * sigma, c = theta2 + sigma2;
            A = (a * sigma + (1.0 - b) * theta) / (theta * c);
            B = (C - ((b - 1.0) * sigma + a * theta) / c) * 1.0 / theta2;
        }
    }
    if (small_theta) for (int i = 0; i < 9; i++) R[i] = ((i % 4 == 0 ? 1.0 : 0.0) + O[i]) + O2[i];
    else {
        const double a = sn / theta, c = (1.0 - cs) / (theta * theta);
        for (int i = 0; i < 9; i++) R[i] = ((i % 4 == 0 ? 1.0 : 0.0) + a * O[i]) + c * O2[i];
    }
    s3o_quat_of_matrix(R, E);
    double W[9];
    for (int i = 0; i < 9; i++) W[i] = (A * O[i] + B * O2[i]) + C * (i % 4 == 0 ? 1.0 : 0.0);
    E.tx = W[0] * u[3] + W[1] * u[4] + W[2] * u[5]; E.ty = W[3] * u[3] + W[4] * u[4] + W[5] * u[5]; E.tz = W[6] * u[3] + W[7] * u[4] + W[8] * u[5];
    E.s = s;
}
// VertexSim3Expmap::oplusImpl: (fix_scale: update[6] = 0, in the caller's array); Sim3(update) * estimate.  operator*: r = r1 * r2, t = s1 * (r1 * t2) + t1, s = s1 * s2
__device__ static void s3o_oplus(double* u, int fix_scale, const S3o& est, S3o& out)
{
    if (fix_scale) u[6] = 0.0;
    S3o E;
    s3o_exp(u, E);
    double rx, ry, rz;
    s3o_rotate(E.qx, E.qy, E.qz, E.qw, est.tx, est.ty, est.tz, rx, ry, rz);
    S3o r;
    r.qw = E.qw * est.qw - E.qx * est.qx - E.qy * est.qy - E.qz * est.qz;
    r.qx = E.qw * est.qx + E.qx * est.qw + E.qy * est.qz - E.qz * est.qy;
    r.qy = E.qw * est.qy + E.qy * est.qw + E.qz * est.qx - E.qx * est.qz;
    r.qz = E.qw * est.qz + E.qz * est.qw + E.qx * est.qy - E.qy * est.qx;
    r.tx = E.s * rx + E.tx; r.ty = E.s * ry + E.ty; r.tz = E.s * rz + E.tz;
    r.s = E.s * est.s;
    out = r;
}
// LinearSolverDense: (H + lambda I) x = b by LDL^T; a negative pivot is "not positive": x stays as it was
__device__ static int s3o_solve(const double* H, const double* b, double lambda, double* x)
{
    double L[7][7], d[7], y[7];
    for (int j = 0; j < 7; j++) {
        double s = H[s3o_idx(j, j)] + lambda;
        for (int k = 0; k < j; k++) s -= L[j][k] * L[j][k] * d[k];
        d[j] = s;
        if (s < 0.0) return 0;
        for (int i = j + 1; i < 7; i++) {
            double v = H[s3o_idx(j, i)];
            for (int k = 0; k < j; k++) v -= L[i][k] * L[j][k] * d[k];
            L[i][j] = v / s;
        }
    }
    for (int i = 0; i < 7; i++) { double v = b[i]; for (int k = 0; k < i; k++) v -= L[i][k] * y[k]; y[i] = v; }
    for (int i = 6; i >= 0; i--) { double v = y[i] / d[i]; for (int k = i + 1; k < 7; k++) v -= L[k][i] * x[k]; x[i] = v; }
    return 1;
}

// the two computeError()s: obs - cam_map(project(S.map(X)))
__device__ __forceinline__ void s3o_error(const S3o& S, double X, double Y, double Z, double u, double v, double fx, double fy, double cx, double cy, double& e0, double& e1)
{
    double x, y, z;
    s3o_map(S, X, Y, Z, x, y, z);
    e0 = u - (x / z * fx + cx);
    e1 = v - (y / z * fy + cy);
}
__device__ __forceinline__ double s3o_chi2(double e0, double e1, double w) { return e0 * (w * e0) + e1 * (w * e1); }

// One edge into the sums: error at xf[0] (the caller passes the table for a forward edge, the table + 1 for an inverse edge: a transform's inverse follows it),
// the Huber weight and, with SYSTEM, the numerical Jacobian from xf[2 + 4 d] (plus) and xf[4 + 4 d] (minus)
template <bool SYSTEM> __device__ __forceinline__ void s3o_edge(const S3o* xf, double X, double Y, double Z, double u, double v, double w,
                                                               double fx, double fy, double cx, double cy, double delta, double* acc)
{
    double e0, e1;
    s3o_error(xf[0], X, Y, Z, u, v, fx, fy, cx, cy, e0, e1);
    const double chi2 = s3o_chi2(e0, e1, w), dsqr = delta * delta;
    double rho0 = chi2, rho1 = 1.0;
    if (!(chi2 <= dsqr)) { const double sq = sqrt(chi2); rho0 = 2.0 * sq * delta - dsqr; rho1 = delta / sq; }      // RobustKernelHuber::robustify
    if constexpr (SYSTEM) {
        const double scalar = 1.0 / (2 * 1e-9);
        double J0[7], J1[7];
#pragma unroll
        for (int d = 0; d < 7; d++) {
            double p0, p1, m0, m1;
            s3o_error(xf[2 + 4 * d], X, Y, Z, u, v, fx, fy, cx, cy, p0, p1);
            s3o_error(xf[4 + 4 * d], X, Y, Z, u, v, fx, fy, cx, cy, m0, m1);
            J0[d] = scalar * (p0 - m0); J1[d] = scalar * (p1 - m1);
        }
        const double wr = rho1 * w, we0 = w * e0, we1 = w * e1;                  // robustInformation: rho_1 Omega
        int idx = 0;
#pragma unroll
        for (int j = 0; j < 7; j++) {
            const double a0 = J0[j] * wr, a1 = J1[j] * wr;
#pragma unroll
            for (int k = j; k < 7; k++, idx++) acc[idx] += a0 * J0[k] + a1 * J1[k];
            acc[28 + j] += rho1 * (J0[j] * we0 + J1[j] * we1);                   // b -= rho_1 J^T Omega e: summed here, negated by thread 0
        }
        acc[35] += rho0;
    } else acc[0] += rho0;
}

// One evaluation: thread `tid` of T adds its live pairs into acc (SYSTEM: 36 sums, rho_0 last; otherwise rho_0 alone in acc[0]) - forward edge, then inverse edge
template <int T, bool SYSTEM> __device__ __forceinline__ void s3o_accumulate(const orbhip_sim3_pair* pairs, const unsigned char* removed, int n, int tid, const S3o* xf,
                                                                            const double* cam, double delta, double* acc)
{
    for (int k = 0; k < (SYSTEM ? S3O_SUMS : 1); k++) acc[k] = 0.0;
    for (int i = tid; i < n; i += T) {
        if (removed[i]) continue;
        const orbhip_sim3_pair p = pairs[i];
#pragma unroll 1
        for (int side = 0; side < 2; side++) {                                  // one body for both edges, and the transforms read where they are used: hoisted out of the
            int at = side;                                                     // loops, the 30 transforms alone are 480 registers
            asm volatile("" : "+v"(at));
            const float* X = side ? p.X1 : p.X2;
            const double* c = cam + 4 * side;
            s3o_edge<SYSTEM>(xf + at, (double)X[0], (double)X[1], (double)X[2], (double)(side ? p.u2 : p.u1), (double)(side ? p.v2 : p.v1),
                             (double)(side ? p.inv_sigma2_2 : p.inv_sigma2_1), c[0], c[1], c[2], c[3], delta, acc);
        }
    }
}

// The workgroup's sums in s_part[0], for thread 0 ONLY: the barrier lies before thread 0's tree, none after it.  A caller must pass a __syncthreads before
// any thread writes s_part again or reads what thread 0 derives from the sums.
template <int T, int K> __device__ __forceinline__ void s3o_reduce(const double* acc, double (*s_part)[S3O_SUMS], int tid)
{
    const int lane = tid & 63, w = tid >> 6;
#pragma unroll
    for (int k = 0; k < K; k++) {
        double v = acc[k];
        for (int m = 32; m; m >>= 1) v += __shfl_xor(v, m);
        if (lane == 0) s_part[w][k] = v;
    }
    __syncthreads();
    if (tid == 0)
        for (int s = 1; s < T / 64; s <<= 1)
            for (int a = 0; a + s < T / 64; a += 2 * s)
                for (int k = 0; k < K; k++) s_part[a][k] += s_part[a + s][k];
}

// thread 0 has written the estimate to evaluate at to xf[0] and its inverse to xf[1], and a barrier has passed; with SYSTEM threads 0..13 add the perturbed estimates.
// Ends with the sums in s_part[0] for thread 0 (see s3o_reduce): SYSTEM H | b (to be negated) | rho_0, otherwise rho_0 in s_part[0][0].
template <int T, bool SYSTEM> __device__ __forceinline__ void s3o_evaluate(const orbhip_sim3_pair* pairs, const unsigned char* removed, int n, int tid, S3o* xf, int fix_scale,
                                                                          const double* cam, double delta, double (*s_part)[S3O_SUMS])
{
    double acc[SYSTEM ? S3O_SUMS : 1];
    if constexpr (SYSTEM) {
        if (tid < 14) {                                                        // linearizeOplus: push, oplus(+-delta e_d), ..., pop
            double add[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            add[tid >> 1] = (tid & 1) ? -1e-9 : 1e-9;
            S3o P, I;
            s3o_oplus(add, fix_scale, xf[0], P);
            s3o_inverse(P, I);
            xf[2 + 2 * tid] = P; xf[3 + 2 * tid] = I;
        }
        __syncthreads();
    }
    s3o_accumulate<T, SYSTEM>(pairs, removed, n, tid, xf, cam, delta, acc);
    s3o_reduce<T, SYSTEM ? S3O_SUMS : 1>(acc, s_part, tid);
}

template <int T> __global__ __launch_bounds__(T) void k_sim3_opt(const Sim3OptProblem* problems)
{
    HIP_DYNAMIC_SHARED(orbhip_sim3_pair, s_pairs)
    __shared__ double s_part[T / 64][S3O_SUMS];
    __shared__ S3oState S;
    __shared__ S3o s_xf[S3O_NXF];
    __shared__ double s_cam[8];
    __shared__ unsigned char s_removed[S3O_STAGE_MAX];                          // the pairs' flags while the problem is staged (a thread reads and writes its own pairs' only)
    const int tid = threadIdx.x;
    const Sim3OptProblem& Q = problems[blockIdx.x];
    const int n = Q.n, fix_scale = Q.fix_scale;
    const double th2 = (double)Q.th2, delta = (double)(float)sqrt((double)Q.th2);        // const float deltaHuber = sqrt(th2)
    unsigned char* removed = Q.removed;
    const orbhip_sim3_pair* pairs = Q.pairs;
    if (n <= S3O_STAGE_MAX) {
        const float* src = reinterpret_cast<const float*>(Q.pairs); float* dst = reinterpret_cast<float*>(s_pairs);
        for (int t = tid; t < n * 12; t += T) dst[t] = src[t];
        pairs = s_pairs; removed = s_removed;
    }
    for (int i = tid; i < n; i += T) removed[i] = 0;
    if (tid < 8) s_cam[tid] = (double)Q.cam[tid];
    if (tid == 0) {
        S.cur.qx = Q.S12[0]; S.cur.qy = Q.S12[1]; S.cur.qz = Q.S12[2]; S.cur.qw = Q.S12[3]; S.cur.tx = Q.S12[4]; S.cur.ty = Q.S12[5]; S.cur.tz = Q.S12[6]; S.cur.s = Q.S12[7];
        S.n_bad = 0; S.n_in = 0;
    }
    __syncthreads();

    for (int phase = 0; phase < 2; phase++) {
        const int iterations = phase == 0 ? 5 : S.n_bad > 0 ? 10 : 5;          // nMoreIterations
        if (tid == 0) {
            S.last = S.cur;
            for (int k = 0; k < 7; k++) S.x[k] = 0.0;
            s_xf[0] = S.cur; s3o_inverse(S.cur, s_xf[1]);
        }
        __syncthreads();
        bool have_system = false;                                              // (uniform) the sums at cur are in S.H, S.b, S.chi
        for (int it = 0; it < 10; it++) {
            if (it >= iterations) break;
            if (!have_system) {                                                // computeActiveErrors, activeRobustChi2 and buildSystem at the estimate (s_xf[0], s_xf[1])
                s3o_evaluate<T, true>(pairs, removed, n, tid, s_xf, fix_scale, s_cam, delta, s_part);
                if (tid == 0) {
                    for (int k = 0; k < 28; k++) S.H[k] = s_part[0][k];
                    for (int k = 0; k < 7; k++) S.b[k] = -s_part[0][28 + k];
                    S.chi = s_part[0][35];
                }
            }
            if (tid == 0) {
                S.last = S.cur; S.ini_chi = S.chi;
                if (it == 0) {
                    double mx = 0.0;
                    for (int j = 0; j < 7; j++) mx = fmax(fabs(S.H[s3o_idx(j, j)]), mx);
                    S.lambda = 1e-5 * mx; S.ni = 2.0; S.n_bad_steps = 0;
                }
            }
            for (int q = 0; q < 10; q++) {
                if (tid == 0) {
                    S.ok2 = s3o_solve(S.H, S.b, S.lambda, S.x);
                    s3o_oplus(S.x, fix_scale, S.cur, S.trial);
                    S.last = S.trial;
                    s_xf[0] = S.trial; s3o_inverse(S.trial, s_xf[1]);
                }
                __syncthreads();
                s3o_evaluate<T, S3O_SYSTEM_EVERY_TRIAL != 0>(pairs, removed, n, tid, s_xf, fix_scale, s_cam, delta, s_part);
                if (tid == 0) {
                    double temp_chi = s_part[0][S3O_SYSTEM_EVERY_TRIAL ? 35 : 0];
                    if (!S.ok2) temp_chi = DBL_MAX;
                    double rho = S.chi - temp_chi, scale = 0.0;
                    for (int j = 0; j < 7; j++) scale += S.x[j] * (S.lambda * S.x[j] + S.b[j]);
                    scale += 1e-3;
                    rho /= scale;
                    const bool accepted = rho > 0.0 && __builtin_isfinite(temp_chi);
                    if (accepted) {
                        double alpha = 1.0 - pow(2.0 * rho - 1.0, 3.0);
                        alpha = fmin(alpha, 2.0 / 3.0);
                        S.lambda *= fmax(1.0 / 3.0, alpha);
                        S.ni = 2.0; S.chi = temp_chi; S.cur = S.trial;
#if S3O_SYSTEM_EVERY_TRIAL
                        for (int k = 0; k < 28; k++) S.H[k] = s_part[0][k];
                        for (int k = 0; k < 7; k++) S.b[k] = -s_part[0][28 + k];
#endif
                    } else {
                        S.lambda *= S.ni; S.ni *= 2.0;                           // pop(): the estimate is restored, the edges' errors are not
                    }
                    S.more_trials = rho < 0.0 && q + 1 < 10;
                    if (!S.more_trials) {
                        bool go = !(q + 1 == 10 || rho == 0.0);
                        if (go) {
                            if ((S.ini_chi - S.chi) * 1e3 < S.ini_chi) S.n_bad_steps++; else S.n_bad_steps = 0;
                            if (S.n_bad_steps >= 3) go = false;
                        }
                        S.more_iters = go;
                        if (!S3O_SYSTEM_EVERY_TRIAL && go && it + 1 < iterations) { s_xf[0] = S.cur; s3o_inverse(S.cur, s_xf[1]); }      // the next iteration's system is built at the estimate
                    }
                }
                __syncthreads();
                if (!S.more_trials) break;
            }
            have_system = S3O_SYSTEM_EVERY_TRIAL != 0;
            if (!S.more_iters) break;
        }
        // the check: a pair goes as a whole if either edge's chi2, at the estimate of the phase's last computeActiveErrors, exceeds th2
        __syncthreads();
        S3o L = S.last, Li;
        s3o_inverse(L, Li);
        int bad = 0, in = 0;
        for (int i = tid; i < n; i += T) {
            if (removed[i]) continue;
            const orbhip_sim3_pair p = pairs[i];
            double e0, e1;
            s3o_error(L, (double)p.X2[0], (double)p.X2[1], (double)p.X2[2], (double)p.u1, (double)p.v1, s_cam[0], s_cam[1], s_cam[2], s_cam[3], e0, e1);
            const double c12 = s3o_chi2(e0, e1, (double)p.inv_sigma2_1);
            s3o_error(Li, (double)p.X1[0], (double)p.X1[1], (double)p.X1[2], (double)p.u2, (double)p.v2, s_cam[4], s_cam[5], s_cam[6], s_cam[7], e0, e1);
            const double c21 = s3o_chi2(e0, e1, (double)p.inv_sigma2_2);
            const int out = c12 > th2 || c21 > th2;
            removed[i] = (unsigned char)out; bad += out; in += !out;
        }
        for (int m = 32; m; m >>= 1) { bad += __shfl_xor(bad, m); in += __shfl_xor(in, m); }
        if (tid == 0) S.n_in = 0;
        __syncthreads();
        if ((tid & 63) == 0) { if (phase == 0 && bad) atomicAdd(&S.n_bad, bad); if (in) atomicAdd(&S.n_in, in); }      // n_bad: nBad, the first check's alone
        __syncthreads();
        if (n - S.n_bad < 10) break;                                           // nCorrespondences - nBad < 10: return 0, g2oS12 untouched
    }
    if (removed == s_removed) for (int i = tid; i < n; i += T) Q.removed[i] = s_removed[i];
    if (tid == 0) {
        const bool early = n - S.n_bad < 10;
        double* o = Q.S12_out;
        if (early) for (int k = 0; k < 8; k++) o[k] = Q.S12[k];
        else { o[0] = S.cur.qx; o[1] = S.cur.qy; o[2] = S.cur.qz; o[3] = S.cur.qw; o[4] = S.cur.tx; o[5] = S.cur.ty; o[6] = S.cur.tz; o[7] = S.cur.s; }
        *Q.n_inliers = early ? 0 : S.n_in;
    }
}

// ---------------------------------------------------------------------------------------------- host
// Every problem of a call in one pass: ONE arena (the problem table, every live problem's pairs, then every answer), one copy each way, one launch.
// Problems with n == 0 are answered here: 0 inliers, nothing else written.
static orbhip_status sim3_optimize_problems(int device, int nproblems, orbhip_sim3_opt_problem* problems, const char* who)
{
    OrbApiTimer api_timer;
    std::vector<int> live;
    int max_n = 0;
    for (int p = 0; p < nproblems; p++) {
        orbhip_sim3_opt_problem& Q = problems[p];
        if (Q.n < 0 || (Q.n > 0 && (!Q.pairs || !Q.removed))) return fail(ORBHIP_ERR_INVALID, "bad argument in problem %d", p);
        Q.n_inliers = 0;
        if (Q.n >= 1) { live.push_back(p); max_n = std::max(max_n, Q.n); }
    }
    if (live.empty()) return ORBHIP_OK;
    if (!device_present()) return fail(ORBHIP_ERR_HIP, "no HIP device available: no CPU fallback");
    HIPCHK(hipSetDevice(device));
    const hipStream_t s = orbhip_thread_stream(device);
    const int NL = (int)live.size();
    struct Answer { double S12[8]; int n_inliers; int pad; };
    std::vector<Sim3OptProblem> hP(NL); std::vector<Answer> hA(NL);
    Sim3OptProblem* dP = nullptr; Answer* dA = nullptr;
    std::vector<orbhip_sim3_pair*> dpairs(NL, nullptr); std::vector<unsigned char*> dflag(NL, nullptr);
    const hipError_t e = arena_call(device, s, [&](Arena& A) {
        A.io(&dP, (size_t)NL, (const Sim3OptProblem*)hP.data(), (size_t)NL);
        for (int k = 0; k < NL; k++) { const orbhip_sim3_opt_problem& Q = problems[live[k]]; A.io(&dpairs[k], (size_t)Q.n, Q.pairs, (size_t)Q.n); }
        A.io(&dA, (size_t)NL, (const Answer*)nullptr, 0, hA.data(), (size_t)NL);
        for (int k = 0; k < NL; k++) { const orbhip_sim3_opt_problem& Q = problems[live[k]]; A.io(&dflag[k], (size_t)Q.n, (const unsigned char*)nullptr, 0, (unsigned char*)Q.removed, (size_t)Q.n); }
        for (int k = 0; k < NL; k++) {                                          // (hP is read when the arena is uploaded, after this pass has filled in the addresses)
            const orbhip_sim3_opt_problem& Q = problems[live[k]]; Sim3OptProblem& D = hP[k];
            D.pairs = dpairs[k]; D.removed = dflag[k]; D.S12_out = dA ? dA[k].S12 : nullptr; D.n_inliers = dA ? &dA[k].n_inliers : nullptr;
            D.n = Q.n; D.fix_scale = Q.fix_scale != 0; D.th2 = Q.th2;
            memcpy(D.cam, &Q.cam, sizeof D.cam); memcpy(D.S12, Q.S12_in, sizeof D.S12);
        }
    }, [&] {
        const size_t lds = (size_t)std::min(max_n, S3O_STAGE_MAX) * sizeof(orbhip_sim3_pair);
        hipLaunchKernelGGL(k_sim3_opt<S3O_T>, dim3(NL, 1, 1), dim3(S3O_T, 1, 1), lds, s, (const Sim3OptProblem*)dP);
    });
    if (e != hipSuccess) return fail(ORBHIP_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    for (int k = 0; k < NL; k++) { orbhip_sim3_opt_problem& Q = problems[live[k]]; memcpy(Q.S12_out, hA[k].S12, sizeof Q.S12_out); Q.n_inliers = hA[k].n_inliers; }
    return ORBHIP_OK;
}

extern "C" orbhip_status orbhip_sim3_optimize_batch(int device, int nproblems, orbhip_sim3_opt_problem* problems)
{
    if (nproblems < 0 || (nproblems > 0 && !problems)) return fail(ORBHIP_ERR_INVALID, "bad argument");
    return sim3_optimize_problems(device, nproblems, problems, "sim3_optimize_batch");
}
extern "C" orbhip_status orbhip_sim3_optimize(int device, orbhip_sim3_opt_problem* problem)
{
    if (!problem) return fail(ORBHIP_ERR_INVALID, "bad argument");
    return sim3_optimize_problems(device, 1, problem, "sim3_optimize");
}
