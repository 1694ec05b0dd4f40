// orbhip_pose_opt.hip — Optimizer::PoseOptimization (Optimizer.cc:239-451) in one launch: one SE(3) vertex, n unary edges (monocular 2-D, stereo 3-D),
// four rounds of at most ten Levenberg-Marquardt iterations of at most ten trials, as g2o runs them (OptimizationAlgorithmLevenberg::solve,
// SparseOptimizer::optimize, BaseUnaryEdge::constructQuadraticForm, RobustKernelHuber, LinearSolverDense, SE3Quat).  Everything is double; inputs are float.
//
//   k_pose_opt<T>     one workgroup of T threads per problem, all four rounds.  Thread t owns edges t, t + T, ...  One EVALUATION at a pose: every thread walks its
//                     active edges (error, analytic Jacobian, Huber weight) and keeps PO_SUMS = 28 running sums - the 21 upper entries of H, the 6 of b, rho_0;
//                     the sums are added across the wave by a shuffle butterfly, written per wave to LDS and added across waves by thread 0 in a fixed tree: the
//                     order of every addition follows from n and T alone, so a problem gives the same bits alone, repeated, or at any slot of a batch.
//                     Thread 0 then does what g2o does between two computeActiveErrors(): accept / reject, lambda, the 6 x 6 LDL^T solve, exp(x) * estimate,
//                     and publishes the next trial pose and two "go on" flags through LDS.  Every trial evaluates H and b along with chi2: an accepted trial's
//                     system IS the next iteration's (g2o rebuilds it at the same estimate), a rejected one's is dropped.
//   per-edge state    one byte: the outlier flag = the edge's level, in LDS while the problem is staged (copied to the caller's `outlier` array at the end) and
//                     in that array itself beyond.  An edge's error is a pure function of
//                     the pose, so the "_error the last computeActiveErrors left" that the classification reads for a level-0 edge is recomputed at the pose of the
//                     round's last evaluation (PoState::last: the rejected trial's if the round ended on one) - no error vector is stored.  The observations
//                     are staged in LDS up to PO_STAGE_MAX edges (28 bytes each) and read through L2 beyond.
//   k_pose_gather     the frame form: observations from the resident undistorted key points, right columns and the context's 1 / sigma^2 table.
// No loop depends on the data for its bound: 4 rounds x 10 iterations x 10 trials, each a compile-time limit.  No floating-point atomics.
#include "orbhip_ctx.h"
#include <cfloat>

#define PO_SUMS 28
#define PO_STAGE_MAX 2048              // edges whose observations are staged in LDS (56 KB)
#ifndef PO_T
#define PO_T 256                       // threads per workgroup: the measured choice among 64, 128, 256 and 512; a compile-time constant
#endif

struct PoPose { double qx, qy, qz, qw, tx, ty, tz; };                         // SE3Quat: _r (unit quaternion, w >= 0), _t
struct PoseOptProblem {
    const orbhip_pose_obs* obs; unsigned char* outlier; float* Tcw_out; int* n_inliers;
    int n; float fx, fy, cx, cy, bf; float Tcw[16];
};
// thread 0's state between two evaluations (LDS), and what it publishes to the workgroup
struct PoState {
    PoPose init, cur, trial, last;     // Converter::toSE3Quat(mTcw); the estimate; the trial just evaluated; the pose of the round's last computeActiveErrors
    double H[21], b[6], chi;           // the system and activeRobustChi2 at cur
    double x[6];                       // the solver's x (a failed solve leaves it as it was)
    double lambda, ni, ini_chi;
    int n_bad_steps, ok2, more_trials, more_iters, n_active, n_bad;
};

__device__ __forceinline__ int po_idx(int j, int k) { return j * 6 - j * (j - 1) / 2 + (k - j); }      // (j <= k) of the 21 upper entries, row by row

// Eigen: Quaternion(Matrix3), Quaternion * Vector3, Quaternion * Quaternion, toRotationMatrix, SE3Quat::normalizeRotation
__device__ static void po_quat_of_matrix(const double m[9], PoPose& P)
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
__device__ static void po_normalize_rotation(PoPose& P)
{
    if (P.qw < 0.0) { P.qx = -P.qx; P.qy = -P.qy; P.qz = -P.qz; P.qw = -P.qw; }
    const double nrm = sqrt(P.qx * P.qx + P.qy * P.qy + P.qz * P.qz + P.qw * P.qw);
    P.qx /= nrm; P.qy /= nrm; P.qz /= nrm; P.qw /= nrm;
}
__device__ __forceinline__ void po_rotate(const PoPose& P, double X, double Y, double Z, double& x, double& y, double& z)
{
    double ux = P.qy * Z - P.qz * Y, uy = P.qz * X - P.qx * Z, uz = P.qx * Y - P.qy * X;      // uv = q.vec x v; uv += uv; v + w uv + q.vec x uv
    ux += ux; uy += uy; uz += uz;
    x = X + P.qw * ux + (P.qy * uz - P.qz * uy);
    y = Y + P.qw * uy + (P.qz * ux - P.qx * uz);
    z = Z + P.qw * uz + (P.qx * uy - P.qy * ux);
}
__device__ static void po_rotation_matrix(const PoPose& P, double R[9])
{
    const double tx = 2.0 * P.qx, ty = 2.0 * P.qy, tz = 2.0 * P.qz, twx = tx * P.qw, twy = ty * P.qw, twz = tz * P.qw;
    const double txx = tx * P.qx, txy = ty * P.qx, txz = tz * P.qx, tyy = ty * P.qy, tyz = tz * P.qy, tzz = tz * P.qz;
    R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1.0 - (txx + tyy);
}
// Converter::toSE3Quat: the float entries widened, SE3Quat(R, t)
__device__ static void po_pose_of_matrix(const float* T, PoPose& P)
{
    const double R[9] = {(double)T[0], (double)T[1], (double)T[2], (double)T[4], (double)T[5], (double)T[6], (double)T[8], (double)T[9], (double)T[10]};
    po_quat_of_matrix(R, P); P.tx = (double)T[3]; P.ty = (double)T[7]; P.tz = (double)T[11];
    po_normalize_rotation(P);
}
// VertexSE3Expmap::oplusImpl: SE3Quat::exp(update) * estimate (update = omega | upsilon)
__device__ static void po_oplus(const double* u, const PoPose& est, PoPose& out)
{
    const double ox = u[0], oy = u[1], oz = u[2];
    const double theta = sqrt(ox * ox + oy * oy + oz * oz);
    const double O[9] = {0.0, -oz, oy, oz, 0.0, -ox, -oy, ox, 0.0};
    double O2[9], R[9], V[9];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) O2[i * 3 + j] = O[i * 3] * O[j] + O[i * 3 + 1] * O[3 + j] + O[i * 3 + 2] * O[6 + j];
    if (theta < 0.00001) {
        for (int i = 0; i < 9; i++) { R[i] = ((i % 4 == 0 ? 1.0 : 0.0) + O[i]) + O2[i]; V[i] = R[i]; }
    } else {
        const double a = sin(theta) / theta, c = (1.0 - cos(theta)) / (theta * theta), d = (theta - sin(theta)) / pow(theta, 3.0);
        for (int i = 0; i < 9; i++) {
            const double I = i % 4 == 0 ? 1.0 : 0.0;
            R[i] = (I + a * O[i]) + c * O2[i];
            V[i] = (I + c * O[i]) + d * O2[i];
        }
    }
    PoPose E;
    po_quat_of_matrix(R, E);
    E.tx = V[0] * u[3] + V[1] * u[4] + V[2] * u[5]; E.ty = V[3] * u[3] + V[4] * u[4] + V[5] * u[5]; E.tz = V[6] * u[3] + V[7] * u[4] + V[8] * u[5];
    po_normalize_rotation(E);
    // SE3Quat::operator*: t = t1 + r1 * t2; r = r1 * r2; normalizeRotation
    double rx, ry, rz;
    po_rotate(E, est.tx, est.ty, est.tz, rx, ry, rz);
    out.tx = E.tx + rx; out.ty = E.ty + ry; out.tz = E.tz + rz;
    out.qw = E.qw * est.qw - E.qx * est.qx - E.qy * est.qy - E.qz * est.qz;
    out.qx = E.qw * est.qx + E.qx * est.qw + E.qy * est.qz - E.qz * est.qy;
    out.qy = E.qw * est.qy + E.qy * est.qw + E.qz * est.qx - E.qx * est.qz;
    out.qz = E.qw * est.qz + E.qz * est.qw + E.qx * est.qy - E.qy * est.qx;
    po_normalize_rotation(out);
}
// LinearSolverDense: (H + lambda I) x = b by LDL^T; a negative pivot is "not positive": x stays as it was
__device__ static int po_solve(const double* H, const double* b, double lambda, double* x)
{
    double L[6][6], d[6], y[6];
    for (int j = 0; j < 6; j++) {
        double s = H[po_idx(j, j)] + lambda;
        for (int k = 0; k < j; k++) s -= L[j][k] * L[j][k] * d[k];
        d[j] = s;
        if (s < 0.0) return 0;
        for (int i = j + 1; i < 6; i++) {
            double v = H[po_idx(j, i)];
            for (int k = 0; k < j; k++) v -= L[i][k] * L[j][k] * d[k];
            L[i][j] = v / s;
        }
    }
    for (int i = 0; i < 6; i++) { double v = b[i]; for (int k = 0; k < i; k++) v -= L[i][k] * y[k]; y[i] = v; }
    for (int i = 5; i >= 0; i--) { double v = y[i] / d[i]; for (int k = i + 1; k < 6; k++) v -= L[k][i] * x[k]; x[i] = v; }
    return 1;
}

// computeError of the two ...OnlyPose edges at pose P; returns chi2 = e . (Omega e).  (x, y, z) = estimate.map(Xw)
__device__ __forceinline__ double po_error(const orbhip_pose_obs& o, const PoPose& P, double fx, double fy, double cx, double cy, double bf,
                                           double& x, double& y, double& z, double e[3], bool& stereo)
{
    po_rotate(P, (double)o.X, (double)o.Y, (double)o.Z, x, y, z);
    x += P.tx; y += P.ty; z += P.tz;
    const double w = (double)o.inv_sigma2;
    stereo = !(o.u_right < 0.0f);
    if (!stereo) {
        e[0] = (double)o.u - (x / z * fx + cx);
        e[1] = (double)o.v - (y / z * fy + cy);
        e[2] = 0.0;
        return e[0] * (w * e[0]) + e[1] * (w * e[1]);
    }
    const double invz = (double)(float)(1.0 / z);                             // `const float invz = 1.0f/trans_xyz[2]` (types_six_dof_expmap.cpp:300)
    const double pu = x * invz * fx + cx;
    e[0] = (double)o.u - pu;
    e[1] = (double)o.v - (y * invz * fy + cy);
    e[2] = (double)o.u_right - (pu - bf * invz);
    return e[0] * (w * e[0]) + e[1] * (w * e[1]) + e[2] * (w * e[2]);
}

// One evaluation: thread `tid` of T adds its level-0 edges into acc
template <int T> __device__ __forceinline__ void po_accumulate(const orbhip_pose_obs* obs, const unsigned char* level, int n, int tid, const PoPose& P,
                                                               double fx, double fy, double cx, double cy, double bf, bool robust, double acc[PO_SUMS])
{
    const double delta_mono = (double)(float)sqrt(5.991), delta_stereo = (double)(float)sqrt(7.815);
    for (int k = 0; k < PO_SUMS; k++) acc[k] = 0.0;
    for (int i = tid; i < n; i += T) {
        if (level[i]) continue;
        const orbhip_pose_obs o = obs[i];
        double x, y, z, e[3]; bool stereo;
        const double chi2 = po_error(o, P, fx, fy, cx, cy, bf, x, y, z, e, stereo);
        double rho0 = chi2, rho1 = 1.0;
        if (robust) {                                                          // RobustKernelHuber::robustify
            const double delta = stereo ? delta_stereo : delta_mono, dsqr = delta * delta;
            if (!(chi2 <= dsqr)) { const double sq = sqrt(chi2); rho0 = 2.0 * sq * delta - dsqr; rho1 = delta / sq; }
        }
        const double invz = 1.0 / z, invz_2 = invz * invz;                      // linearizeOplus
        double A[3][6];
        A[0][0] = x * y * invz_2 * fx; A[0][1] = -(1.0 + (x * x * invz_2)) * fx; A[0][2] = y * invz * fx; A[0][3] = -invz * fx; A[0][4] = 0.0; A[0][5] = x * invz_2 * fx;
        A[1][0] = (1.0 + y * y * invz_2) * fy; A[1][1] = -x * y * invz_2 * fy; A[1][2] = -x * invz * fy; A[1][3] = 0.0; A[1][4] = -invz * fy; A[1][5] = y * invz_2 * fy;
        A[2][0] = A[0][0] - bf * y * invz_2; A[2][1] = A[0][1] + bf * x * invz_2; A[2][2] = A[0][2]; A[2][3] = A[0][3]; A[2][4] = 0.0; A[2][5] = A[0][5] - bf * invz_2;
        const double w = (double)o.inv_sigma2, wr = rho1 * w;                   // robustInformation: rho_1 Omega (the second-order term is commented out there)
        const double we0 = w * e[0], we1 = w * e[1], we2 = w * e[2];
        int idx = 0;
#pragma unroll
        for (int j = 0; j < 6; j++) {
            const double a0 = A[0][j] * wr, a1 = A[1][j] * wr, a2 = A[2][j] * wr;
#pragma unroll
            for (int k = j; k < 6; k++, idx++) {
                double t = a0 * A[0][k] + a1 * A[1][k];
                if (stereo) t += a2 * A[2][k];
                acc[idx] += t;
            }
            double g = A[0][j] * we0 + A[1][j] * we1;
            if (stereo) g += A[2][j] * we2;
            acc[21 + j] += rho1 * g;                                           // b -= rho_1 A^T Omega e: summed here, negated by thread 0
        }
        acc[27] += rho0;
    }
}

// The workgroup's sums in s_part[0], for thread 0 ONLY: the barrier lies before thread 0's tree, none after it.  A caller must pass a __syncthreads before
// any thread writes s_part again (the next po_reduce) or reads what thread 0 derives from the sums - every call below is followed by one.
template <int T> __device__ __forceinline__ void po_reduce(double acc[PO_SUMS], double (*s_part)[PO_SUMS], int tid)
{
    const int lane = tid & 63, w = tid >> 6;
#pragma unroll
    for (int k = 0; k < PO_SUMS; k++) {
        double v = acc[k];
        for (int m = 32; m; m >>= 1) v += __shfl_xor(v, m);
        if (lane == 0) s_part[w][k] = v;
    }
    __syncthreads();
    if (tid == 0)
        for (int s = 1; s < T / 64; s <<= 1)
            for (int a = 0; a + s < T / 64; a += 2 * s)
                for (int k = 0; k < PO_SUMS; k++) s_part[a][k] += s_part[a + s][k];
}

template <int T> __global__ __launch_bounds__(T) void k_pose_opt(const PoseOptProblem* problems)
{
    HIP_DYNAMIC_SHARED(orbhip_pose_obs, s_obs)
    __shared__ double s_part[T / 64][PO_SUMS];
    __shared__ PoState S;
    __shared__ unsigned char s_level[PO_STAGE_MAX];                             // the edges' levels while the problem is staged (a thread reads and writes its own edges' only)
    const int tid = threadIdx.x;
    const PoseOptProblem& Q = problems[blockIdx.x];
    const int n = Q.n;
    const double fx = (double)Q.fx, fy = (double)Q.fy, cx = (double)Q.cx, cy = (double)Q.cy, bf = (double)Q.bf;
    unsigned char* level = Q.outlier;
    const orbhip_pose_obs* obs = Q.obs;
    if (n <= PO_STAGE_MAX) {
        const float* src = reinterpret_cast<const float*>(Q.obs); float* dst = reinterpret_cast<float*>(s_obs);
        for (int t = tid; t < n * 7; t += T) dst[t] = src[t];
        obs = s_obs; level = s_level;
    }
    for (int i = tid; i < n; i += T) level[i] = 0;                              // pFrame->mvbOutlier[i] = false
    if (tid == 0) { po_pose_of_matrix(Q.Tcw, S.init); S.n_active = n; S.n_bad = 0; }
    double acc[PO_SUMS];

    for (int round = 0; round < 4; round++) {
        const bool robust = round < 3;                                         // e->setRobustKernel(0) after round index 2
        if (tid == 0) { S.cur = S.init; S.last = S.init; S.n_bad = 0; }        // vSE3->setEstimate(Converter::toSE3Quat(pFrame->mTcw))
        __syncthreads();
        if (S.n_active > 0) {                                                  // no level-0 edge: optimize() returns at once
            po_accumulate<T>(obs, level, n, tid, S.cur, fx, fy, cx, cy, bf, robust, acc);
            po_reduce<T>(acc, s_part, tid);
            if (tid == 0) {
                for (int k = 0; k < 21; k++) S.H[k] = s_part[0][k];
                for (int k = 0; k < 6; k++) { S.b[k] = -s_part[0][21 + k]; S.x[k] = 0.0; }
                S.chi = s_part[0][27];
            }
            for (int it = 0; it < 10; it++) {
                if (tid == 0) {                                                // solve(it): errors and system at the estimate are the ones held
                    S.last = S.cur; S.ini_chi = S.chi;
                    if (it == 0) {
                        double mx = 0.0;
                        for (int j = 0; j < 6; j++) mx = fmax(fabs(S.H[po_idx(j, j)]), mx);
                        S.lambda = 1e-5 * mx; S.ni = 2.0; S.n_bad_steps = 0;
                    }
                }
                for (int q = 0; q < 10; q++) {
                    if (tid == 0) {
                        S.ok2 = po_solve(S.H, S.b, S.lambda, S.x);
                        po_oplus(S.x, S.cur, S.trial);
                        S.last = S.trial;
                    }
                    __syncthreads();
                    po_accumulate<T>(obs, level, n, tid, S.trial, fx, fy, cx, cy, bf, robust, acc);
                    po_reduce<T>(acc, s_part, tid);
                    if (tid == 0) {
                        double temp_chi = s_part[0][27];
                        if (!S.ok2) temp_chi = DBL_MAX;
                        double rho = S.chi - temp_chi, scale = 0.0;
                        for (int j = 0; j < 6; j++) scale += S.x[j] * (S.lambda * S.x[j] + S.b[j]);
                        scale += 1e-3;
                        rho /= scale;
                        if (rho > 0.0 && __builtin_isfinite(temp_chi)) {
                            double alpha = 1.0 - pow(2.0 * rho - 1.0, 3.0);
                            alpha = fmin(alpha, 2.0 / 3.0);
                            S.lambda *= fmax(1.0 / 3.0, alpha);
                            S.ni = 2.0; S.chi = temp_chi; S.cur = S.trial;
                            for (int k = 0; k < 21; k++) S.H[k] = s_part[0][k];
                            for (int k = 0; k < 6; k++) S.b[k] = -s_part[0][21 + k];
                        } else {
                            S.lambda *= S.ni; S.ni *= 2.0;                       // pop(): the estimate is restored, the edges' errors are not
                        }
                        S.more_trials = rho < 0.0 && q + 1 < 10;
                        if (!S.more_trials) {
                            bool go = !(q + 1 == 10 || rho == 0.0);
                            if (go) {
                                if ((S.ini_chi - S.chi) * 1e3 < S.ini_chi) S.n_bad_steps++; else S.n_bad_steps = 0;
                                if (S.n_bad_steps >= 3) go = false;
                            }
                            S.more_iters = go;
                        }
                    }
                    __syncthreads();
                    if (!S.more_trials) break;
                }
                if (!S.more_iters) break;
            }
        }
        // classification: an outlier's error is computed afresh at the estimate, a level-0 edge's is the one the round's last evaluation left
        __syncthreads();
        int bad = 0;
        for (int i = tid; i < n; i += T) {
            const orbhip_pose_obs o = obs[i];
            double x, y, z, e[3]; bool stereo;
            const float chi2 = (float)po_error(o, level[i] ? S.cur : S.last, fx, fy, cx, cy, bf, x, y, z, e, stereo);
            const int out = stereo ? chi2 > 7.815f : chi2 > 5.991f;
            level[i] = (unsigned char)out; bad += out;
        }
        for (int m = 32; m; m >>= 1) bad += __shfl_xor(bad, m);
        if ((tid & 63) == 0 && bad) atomicAdd(&S.n_bad, bad);
        __syncthreads();
        if (tid == 0) S.n_active = n - S.n_bad;
        if (n < 10) break;                                                     // optimizer.edges().size() < 10
    }
    if (level == s_level) for (int i = tid; i < n; i += T) Q.outlier[i] = s_level[i];
    __syncthreads();
    if (tid == 0) {                                                            // Converter::toCvMat(SE3Quat): to_homogeneous_matrix rounded to float
        double R[9]; po_rotation_matrix(S.cur, R);
        float* o = Q.Tcw_out;
        for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) o[i * 4 + j] = (float)R[i * 3 + j]; }
        o[3] = (float)S.cur.tx; o[7] = (float)S.cur.ty; o[11] = (float)S.cur.tz; o[12] = 0.0f; o[13] = 0.0f; o[14] = 0.0f; o[15] = 1.0f;
        *Q.n_inliers = n - S.n_bad;
    }
}

// the frame form's observations: key point idx[i] of the resident frame (undistorted), its right column, 1 / sigma^2 of its octave, the caller's point
__global__ __launch_bounds__(256) void k_pose_gather(const orbhip_keypoint* kp, const float* u_right, const float* inv_sigma2, int nlevels,
                                                     const int* idx, const float* xyz, int m, orbhip_pose_obs* out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const int f = idx[i];
    const orbhip_keypoint k = kp[f];
    const int oct = k.octave < 0 ? 0 : k.octave >= nlevels ? nlevels - 1 : k.octave;
    orbhip_pose_obs o;
    o.u = k.x; o.v = k.y; o.u_right = u_right ? u_right[f] : -1.0f; o.inv_sigma2 = inv_sigma2[oct];
    o.X = xyz[3 * i]; o.Y = xyz[3 * i + 1]; o.Z = xyz[3 * i + 2];
    out[i] = o;
}

// ---------------------------------------------------------------------------------------------- host
static void launch_pose_opt(const PoseOptProblem* d_problems, int nlive, int max_n, hipStream_t s)
{
    const size_t lds = (size_t)std::min(std::max(max_n, 1), PO_STAGE_MAX) * sizeof(orbhip_pose_obs);
    hipLaunchKernelGGL(k_pose_opt<PO_T>, dim3(nlive, 1, 1), dim3(PO_T, 1, 1), lds, s, d_problems);
}

// what the frame form adds to a problem: its observations are gathered on the device from a context's resident frame
struct PoseFrameSource { const orbhip_keypoint* kp; const float* u_right; const float* inv_sigma2; int nlevels; const int32_t* idx; const float* xyz; };

// Every problem of a call in one pass: ONE arena (the problem table, every live problem's inputs, then every answer), one copy each way, one launch of
// k_pose_opt over the table.  Problems with fewer than 3 observations are answered here: 0 inliers, pose and flags untouched.
static orbhip_status pose_optimization_problems(int device, hipStream_t stream, bool own_stream, int nproblems, orbhip_pose_problem* problems, const PoseFrameSource* src, const char* who)
{
    OrbApiTimer api_timer;
    std::vector<int> live;
    int max_n = 0;
    for (int p = 0; p < nproblems; p++) {
        orbhip_pose_problem& Q = problems[p];
        if (Q.n < 0 || (Q.n > 0 && ((!src && !Q.obs) || !Q.outlier))) return nproblems > 1 || !own_stream ? fail(ORBHIP_ERR_INVALID, "bad argument in problem %d", p) : fail(ORBHIP_ERR_INVALID, "bad argument");
        Q.n_inliers = 0;
        if (Q.n >= 3) { live.push_back(p); max_n = std::max(max_n, Q.n); }
    }
    if (live.empty()) return ORBHIP_OK;
    if (own_stream && !device_present()) return fail(ORBHIP_ERR_HIP, "no HIP device available: no CPU fallback");
    HIPCHK(hipSetDevice(device));
    const hipStream_t s = own_stream ? orbhip_thread_stream(device) : stream;
    const int NL = (int)live.size();
    struct Answer { float Tcw[16]; int n_inliers; int pad[3]; };
    std::vector<PoseOptProblem> hP(NL); std::vector<Answer> hA(NL);
    PoseOptProblem* dP = nullptr; Answer* dA = nullptr; float* dis2 = nullptr; int* didx = nullptr; float* dxyz = nullptr;
    std::vector<orbhip_pose_obs*> dobs(NL, nullptr); std::vector<unsigned char*> dflag(NL, nullptr);
    const hipError_t e = arena_call(device, s, [&](Arena& A) {
        A.io(&dP, (size_t)NL, (const PoseOptProblem*)hP.data(), (size_t)NL);
        for (int k = 0; k < NL; k++) {
            const orbhip_pose_problem& Q = problems[live[k]];
            if (src) {                                                          // (the frame form is one problem)
                A.io(&dis2, (size_t)src->nlevels, src->inv_sigma2, (size_t)src->nlevels);
                A.io(&didx, (size_t)Q.n, (const int*)src->idx, (size_t)Q.n);
                A.io(&dxyz, (size_t)Q.n * 3, src->xyz, (size_t)Q.n * 3);
            } else A.io(&dobs[k], (size_t)Q.n, Q.obs, (size_t)Q.n);
        }
        A.io(&dA, (size_t)NL, (const Answer*)nullptr, 0, hA.data(), (size_t)NL);
        for (int k = 0; k < NL; k++) { const orbhip_pose_problem& Q = problems[live[k]]; A.io(&dflag[k], (size_t)Q.n, (const unsigned char*)nullptr, 0, (unsigned char*)Q.outlier, (size_t)Q.n); }
        if (src) A.take(&dobs[0], (size_t)problems[live[0]].n);
        for (int k = 0; k < NL; k++) {                                          // (hP is read when the arena is uploaded, after this pass has filled in the addresses)
            const orbhip_pose_problem& Q = problems[live[k]]; PoseOptProblem& D = hP[k];
            D.obs = dobs[k]; D.outlier = dflag[k]; D.Tcw_out = dA ? dA[k].Tcw : nullptr; D.n_inliers = dA ? &dA[k].n_inliers : nullptr;
            D.n = Q.n; D.fx = Q.cam.fx; D.fy = Q.cam.fy; D.cx = Q.cam.cx; D.cy = Q.cam.cy; D.bf = Q.cam.bf;
            memcpy(D.Tcw, Q.Tcw_in, sizeof D.Tcw);
        }
    }, [&] {
        if (src) {
            const int m = problems[live[0]].n;
            hipLaunchKernelGGL(k_pose_gather, dim3((m + 255) / 256, 1, 1), dim3(256, 1, 1), 0, s, src->kp, src->u_right, (const float*)dis2, src->nlevels, (const int*)didx, (const float*)dxyz, m, dobs[0]);
        }
        launch_pose_opt(dP, NL, max_n, s);
    });
    if (e != hipSuccess) return fail(ORBHIP_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    for (int k = 0; k < NL; k++) { orbhip_pose_problem& Q = problems[live[k]]; memcpy(Q.Tcw_out, hA[k].Tcw, sizeof Q.Tcw_out); Q.n_inliers = hA[k].n_inliers; }
    return ORBHIP_OK;
}

extern "C" orbhip_status orbhip_pose_optimization_batch(int device, int nproblems, orbhip_pose_problem* problems)
{
    if (nproblems < 0 || (nproblems > 0 && !problems)) return fail(ORBHIP_ERR_INVALID, "bad argument");
    return pose_optimization_problems(device, nullptr, true, nproblems, problems, nullptr, "pose_optimization_batch");
}

static orbhip_status one_problem(orbhip_pose_problem* Q, const orbhip_pose_camera* cam, const float* Tcw_in, int n, float* Tcw_out, uint8_t* outlier, int* n_inliers)
{
    if (!cam || !Tcw_in || !Tcw_out || !n_inliers || n < 0 || (n > 0 && !outlier)) return fail(ORBHIP_ERR_INVALID, "bad argument");
    memset(Q, 0, sizeof *Q);
    Q->cam = *cam; memcpy(Q->Tcw_in, Tcw_in, sizeof Q->Tcw_in); Q->n = n; Q->outlier = outlier;
    *n_inliers = 0;
    return ORBHIP_OK;
}
extern "C" orbhip_status orbhip_pose_optimization(int device, const orbhip_pose_camera* cam, const float* Tcw_in, const orbhip_pose_obs* obs, int n,
                                                  float* Tcw_out, uint8_t* outlier, int* n_inliers)
{
    orbhip_pose_problem Q;
    orbhip_status st = one_problem(&Q, cam, Tcw_in, n, Tcw_out, outlier, n_inliers); if (st != ORBHIP_OK) return st;
    if (n > 0 && !obs) return fail(ORBHIP_ERR_INVALID, "bad argument");
    Q.obs = obs;
    st = pose_optimization_problems(device, nullptr, true, 1, &Q, nullptr, "pose_optimization"); if (st != ORBHIP_OK) return st;
    if (n >= 3) { memcpy(Tcw_out, Q.Tcw_out, sizeof Q.Tcw_out); *n_inliers = Q.n_inliers; }
    return ORBHIP_OK;
}
extern "C" orbhip_status orbhip_pose_optimization_frame(orbhip_ctx* c, int frame, const orbhip_pose_camera* cam, const float* Tcw_in, const int32_t* idx, const float* xyz, int m,
                                                        float* Tcw_out, uint8_t* outlier, int* n_inliers)
{
    if (!c) return fail(ORBHIP_ERR_INVALID, "null context");
    if (frame < 0 || frame >= c->last_nimg) return fail(ORBHIP_ERR_INVALID, "frame %d outside the %d frames of the last extraction", frame, c->last_nimg);
    orbhip_pose_problem Q;
    orbhip_status st = one_problem(&Q, cam, Tcw_in, m, Tcw_out, outlier, n_inliers); if (st != ORBHIP_OK) return st;
    if (m > 0 && (!idx || !xyz)) return fail(ORBHIP_ERR_INVALID, "bad argument");
    int nkp = c->out_cap;                                                       // the frame's key point count: what the host has seen, or read from the device once the extraction is complete
    if (c->last_n_valid && frame < (int)c->last_n.size()) nkp = c->last_n[frame];
    else if (m > 0) {
        st = orbhip_sync(c); if (st != ORBHIP_OK) return st;
        HIPCHK(hipSetDevice(c->cfg.device));
        HIPCHK(hipMemcpy(&nkp, c->d_out_n[c->cur] + frame, sizeof(int), hipMemcpyDeviceToHost));
    }
    for (int i = 0; i < m; i++) if (idx[i] < 0 || idx[i] >= nkp) return fail(ORBHIP_ERR_INVALID, "key point index %d at %d outside 0..%d", idx[i], i, nkp - 1);
    const PoseFrameSource src = {(c->distorted ? c->d_out_kpun : c->d_out_kp)[c->cur] + (size_t)frame * c->out_cap,
                                 c->d_last_uright ? c->d_last_uright + (size_t)frame * c->out_cap : nullptr, c->is2.data(), c->L, idx, xyz};
    st = pose_optimization_problems(c->cfg.device, c->stream, false, 1, &Q, &src, "pose_optimization_frame"); if (st != ORBHIP_OK) return st;
    if (m >= 3) { memcpy(Tcw_out, Q.Tcw_out, sizeof Q.Tcw_out); *n_inliers = Q.n_inliers; }
    return ORBHIP_OK;
}
