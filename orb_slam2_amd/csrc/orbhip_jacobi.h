// orbhip_jacobi.h — eigen-decomposition of a small real symmetric matrix inside a kernel: cyclic Jacobi in double, for N x N with N <= 12
// (Sim3Solver's 4 x 4 quaternion matrix today; EPnP's 12 x 12 M^T M later).  One thread does the whole matrix; nothing is shared.
//
// The statement, as tests/sim3_model.py restates it - every operation is one IEEE double +, -, *, / or sqrt, in this order:
//   sweep = 0 .. ORBHIP_JACOBI_SWEEPS - 1 (a compile-time bound; the sweep loop ends early once every off-diagonal entry is exactly 0)
//     pairs (p, q), p < q, row by row: (0,1) (0,2) .. (0,N-1) (1,2) ..
//       apq = A[p][q]; nothing to do if apq == 0
//       g = 100 |apq|; if |A[p][p]| + g == |A[p][p]| and |A[q][q]| + g == |A[q][q]|: A[p][q] = A[q][p] = 0, next pair   (Rutishauser's negligibility test)
//       theta = (A[q][q] - A[p][p]) / (2 apq)
//       t = 1 / (2 theta)                                   if |theta| > 1e150   (theta * theta would overflow)
//           sign(theta) / (|theta| + sqrt(theta * theta + 1))  otherwise             (sign(0) = +1)
//       c = 1 / sqrt(t * t + 1), s = t * c
//       columns p and q of A, then rows p and q of A, then columns p and q of V:  (x_p, x_q) <- (c x_p - s x_q, s x_p + c x_q)
//       A[p][q] = A[q][p] = 0
//   w[i] = A[i][i]; column i of V is its eigenvector.  Nothing is sorted: the caller picks what it needs (orbhip_jacobi_largest).
// A non-finite entry makes every comparison above false, so the rotations go on and spread it: all loops still end at their constant bounds.
#ifndef ORBHIP_JACOBI_H
#define ORBHIP_JACOBI_H

#ifndef ORBHIP_JACOBI_SWEEPS
#define ORBHIP_JACOBI_SWEEPS 24
#endif

template <int N> __device__ static void orbhip_jacobi_eigen(double (&A)[N][N], double (&V)[N][N], double (&w)[N])
{
    static_assert(N >= 2 && N <= 12, "orbhip_jacobi_eigen: 2 <= N <= 12");
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int j = 0; j < N; j++) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < ORBHIP_JACOBI_SWEEPS; sweep++) {
        double off = 0.0;
#pragma unroll
        for (int p = 0; p < N; p++)
#pragma unroll
            for (int q = p + 1; q < N; q++) off += fabs(A[p][q]);
        if (off == 0.0) break;
#pragma unroll
        for (int p = 0; p < N - 1; p++) {
#pragma unroll
            for (int q = p + 1; q < N; q++) {
                const double apq = A[p][q];
                if (apq == 0.0) continue;
                const double g = 100.0 * fabs(apq), app = fabs(A[p][p]), aqq = fabs(A[q][q]);
                if (app + g == app && aqq + g == aqq) { A[p][q] = 0.0; A[q][p] = 0.0; continue; }
                const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                double t;
                if (fabs(theta) > 1e150) t = 1.0 / (2.0 * theta);
                else { t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0)); if (theta < 0.0) t = -t; }
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                for (int k = 0; k < N; k++) { const double xp = A[k][p], xq = A[k][q]; A[k][p] = c * xp - s * xq; A[k][q] = s * xp + c * xq; }
#pragma unroll
                for (int k = 0; k < N; k++) { const double xp = A[p][k], xq = A[q][k]; A[p][k] = c * xp - s * xq; A[q][k] = s * xp + c * xq; }
#pragma unroll
                for (int k = 0; k < N; k++) { const double xp = V[k][p], xq = V[k][q]; V[k][p] = c * xp - s * xq; V[k][q] = s * xp + c * xq; }
                A[p][q] = 0.0; A[q][p] = 0.0;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < N; i++) w[i] = A[i][i];
}

// The cooperative form (PnPsolver's 12 x 12 M^T M and 3 x 3 PW0^T PW0, orbhip_pnp.hip): A and V lie in LDS and one workgroup of one wave (64 threads) does
// the matrix together.  Every lane reads the pair's three entries and computes the same c and s (a wave executes that once whichever lanes take part,
// so nothing is broadcast); lanes 0 .. N-1 then turn the columns of A, lanes 16 .. 16+N-1 the columns of V beside them, and after a barrier lanes
// 0 .. N-1 the rows of A.  Pair order, negligibility test, sweep bound and every rounding are those of the statement above, so A's diagonal and V
// end with the bits of orbhip_jacobi_eigen<N> (asserted under emulation, tests/test_pnp_emu.py).  Every branch is uniform: all lanes read the same
// values.  PRECONDITION: the workgroup is exactly one wave of 64 threads, `lane` = threadIdx.x (the stride 64 and the split into lanes 0 .. N-1 and
// 16 .. 16+N-1 assume it; a larger block would race on A).  The caller has filled A and passed a barrier; on return a barrier has been passed and
// w[i] = A[i][i].
template <int N> __device__ static void orbhip_jacobi_eigen_wave(double (*A)[N], double (*V)[N], int lane)
{
    static_assert(N >= 2 && N <= 12, "orbhip_jacobi_eigen_wave: 2 <= N <= 12");
    for (int e = lane; e < N * N; e += 64) V[e / N][e % N] = e / N == e % N ? 1.0 : 0.0;
    __syncthreads();
    for (int sweep = 0; sweep < ORBHIP_JACOBI_SWEEPS; sweep++) {
        double off = 0.0;
        for (int p = 0; p < N; p++)
            for (int q = p + 1; q < N; q++) off += fabs(A[p][q]);
        if (off == 0.0) break;
        for (int p = 0; p < N - 1; p++) {
            for (int q = p + 1; q < N; q++) {
                const double apq = A[p][q];
                if (apq == 0.0) continue;
                const double dpp = A[p][p], dqq = A[q][q];
                const double g = 100.0 * fabs(apq), app = fabs(dpp), aqq = fabs(dqq);
                __syncthreads();                                                // every lane has read the pair before anyone writes
                if (app + g == app && aqq + g == aqq) {
                    if (lane == 0) { A[p][q] = 0.0; A[q][p] = 0.0; }
                    __syncthreads();
                    continue;
                }
                const double theta = (dqq - dpp) / (2.0 * apq);
                double t;
                if (fabs(theta) > 1e150) t = 1.0 / (2.0 * theta);
                else { t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0)); if (theta < 0.0) t = -t; }
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                if (lane < N) { const int k = lane; const double xp = A[k][p], xq = A[k][q]; A[k][p] = c * xp - s * xq; A[k][q] = s * xp + c * xq; }
                else if (lane >= 16 && lane < 16 + N) { const int k = lane - 16; const double xp = V[k][p], xq = V[k][q]; V[k][p] = c * xp - s * xq; V[k][q] = s * xp + c * xq; }
                __syncthreads();
                if (lane < N) {
                    const int k = lane; const double xp = A[p][k], xq = A[q][k];
                    A[p][k] = k == q ? 0.0 : c * xp - s * xq; A[q][k] = k == p ? 0.0 : s * xp + c * xq;     // A[p][q] = A[q][p] = 0
                }
                __syncthreads();
            }
        }
    }
}

// the eigenvector of the largest eigenvalue: the first index whose eigenvalue is strictly larger than every earlier one (index 0 if none compares)
template <int N> __device__ static void orbhip_jacobi_largest(const double (&V)[N][N], const double (&w)[N], double (&v)[N])
{
    int best = 0;
#pragma unroll
    for (int i = 1; i < N; i++) if (w[i] > w[best]) best = i;
#pragma unroll
    for (int k = 0; k < N; k++) {
        double x = V[k][0];
#pragma unroll
        for (int i = 1; i < N; i++) if (i == best) x = V[k][i];
        v[k] = x;
    }
}
#endif
