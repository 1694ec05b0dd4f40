// Drives ORB_SLAM2::Sim3Solver (include/Sim3Solver.h, orb_slam2_amd/cpp/Sim3Solver.cc) on stand-in key frames - iterate(5) rounds, find, IterateBatch,
// the getters - and compares with the C ABI called directly on the same correspondences and the same triples: matrices, inlier flags, counts and
// bNoMore must be equal bit for bit.  The Random stand-in logs every RandomInt call; the expected side replays the log, so the number and the order
// (the ranges 0..N-1, 0..N-2, 0..N-3 per hypothesis) of the calls are asserted too, including the queue an early return leaves.
// Stand-alone: it links the library named on its build line and prints "sim3_cpp ok".  With ORBHIP_GEMM_MODE=2 in the environment the constructor
// must throw.  Lines "maxits N minInliers maxIterations -> v" report SetRansacParameters for the Python side to compare with the model.
#include "Sim3Solver.h"
#include "KeyFrame.h"
#include "MapPoint.h"
#include "ORBextractor.h"
#include "Random.h"
#include "orbhip.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <vector>

using namespace ORB_SLAM2;

static unsigned long long g_state = 0x9E3779B97F4A7C15ull;
static double uniform() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (double)(g_state >> 11) / 9007199254740992.0; }
static double normal() { double s = 0; for (int i = 0; i < 12; i++) s += uniform(); return s - 6.0; }
static size_t g_logpos = 0;
static int g_mode = 0;

struct Probe : public Sim3Solver {                     // the protected state the test reads
    Probe(KeyFrame* a, KeyFrame* b, const std::vector<MapPoint*>& m, bool fix) : Sim3Solver(a, b, m, fix) {}
    using Sim3Solver::mRansacMaxIts; using Sim3Solver::mnIterations; using Sim3Solver::mqDrawn; using Sim3Solver::N; using Sim3Solver::mvCorr;
};

struct Scene { KeyFrame kf1, kf2; std::vector<std::unique_ptr<MapPoint> > points; std::vector<MapPoint*> matched; };

static void rot_y(cv::Mat& R, double a) { const float m[9] = {(float)std::cos(a), 0, (float)std::sin(a), 0, 1, 0, (float)-std::sin(a), 0, (float)std::cos(a)}; for (int i = 0; i < 9; i++) R.at<float>(i / 3, i % 3) = m[i]; }

// nkp key points in each frame; the true similarity X1c = s Rz(0.3) X2c + t; `wrong` = share of gross mismatches
static void make_scene(Scene& S, int nkp, double s, double wrong)
{
    const float K1[4] = {520.9f, 521.0f, 325.1f, 249.7f}, K2[4] = {517.3f, 516.5f, 318.6f, 255.3f};
    KeyFrame* kf[2] = {&S.kf1, &S.kf2};
    for (int f = 0; f < 2; f++) {
        const float* K = f ? K2 : K1;
        kf[f]->mK = cv::Mat::eye(3, 3, CV_32F);
        kf[f]->mK.at<float>(0, 0) = K[0]; kf[f]->mK.at<float>(1, 1) = K[1]; kf[f]->mK.at<float>(0, 2) = K[2]; kf[f]->mK.at<float>(1, 2) = K[3];
        kf[f]->mvLevelSigma2.resize(8);
        float sf = 1.0f;
        for (int l = 0; l < 8; l++) { kf[f]->mvLevelSigma2[l] = sf * sf; sf = (float)(sf * 1.2); }
        kf[f]->mvKeysUn.resize(nkp); kf[f]->mvpMapPoints.assign(nkp, (MapPoint*)0);
        for (int i = 0; i < nkp; i++) kf[f]->mvKeysUn[i].octave = (int)(8 * uniform()) & 7;
        rot_y(kf[f]->mRcw, f ? -0.15 : 0.1);
        kf[f]->mtcw.at<float>(0) = f ? -0.4f : 0.3f; kf[f]->mtcw.at<float>(1) = f ? 0.1f : -0.2f; kf[f]->mtcw.at<float>(2) = f ? 0.2f : 0.5f;
    }
    S.matched.assign(nkp, (MapPoint*)0);
    const double c = std::cos(0.3), sn = std::sin(0.3), t[3] = {0.2, -0.1, 0.3};
    for (int i = 0; i < nkp; i++) {
        const double z = 2 + 10 * uniform(), X1[3] = {(30 + 580 * uniform() - K1[2]) / K1[0] * z, (30 + 420 * uniform() - K1[3]) / K1[1] * z, z};
        const double d[3] = {(X1[0] - t[0]) / s, (X1[1] - t[1]) / s, (X1[2] - t[2]) / s};
        double X2[3] = {c * d[0] + sn * d[1], -sn * d[0] + c * d[1], d[2]};       // Rz^T d
        const int j = nkp - 1 - i;
        const double sig = std::pow(1.2, S.kf2.mvKeysUn[j].octave);
        X2[0] += 0.5 * sig * normal() * X2[2] / K2[0]; X2[1] += 0.5 * sig * normal() * X2[2] / K2[1];
        if (uniform() < wrong) { X2[0] += normal(); X2[1] += normal(); X2[2] += normal(); }
        const double* Xc[2] = {X1, X2};
        MapPoint* mp[2];
        for (int f = 0; f < 2; f++) {                                           // world = Rcw^T (Xc - tcw)
            const cv::Mat& R = kf[f]->mRcw; const cv::Mat& tc = kf[f]->mtcw;
            double q[3], w[3];
            for (int r = 0; r < 3; r++) q[r] = Xc[f][r] - tc.at<float>(r);
            for (int r = 0; r < 3; r++) w[r] = R.at<float>(0, r) * q[0] + R.at<float>(1, r) * q[1] + R.at<float>(2, r) * q[2];
            S.points.push_back(std::unique_ptr<MapPoint>(new MapPoint((float)w[0], (float)w[1], (float)w[2], kf[f], f ? j : i)));
            mp[f] = S.points.back().get();
        }
        if (i % 9 != 4) S.kf1.mvpMapPoints[i] = mp[0];                          // key points of frame 1 without a map point
        if (i % 5 != 2) S.matched[i] = mp[1];                                   // ... without a match
        if (i % 11 == 7) mp[1]->mbBad = true;
        if (i % 13 == 6) mp[1]->mpKF = &S.kf1;                                  // a match the second key frame does not observe
        S.kf2.mvpMapPoints[j] = mp[1];
    }
}

// the expected side: the class's state around direct calls of the C ABI
struct Expect {
    std::vector<orbhip_sim3_corr> corr; std::vector<int> index1; std::deque<int> queue;
    int mN1, N, its, best_in, maxIts, minInl, fix; float K1[4], K2[4];
    bool has_best; float T[16], R[9], t[3], s;
};
struct Answer { bool has_T; float T[16]; bool noMore; std::vector<bool> inl; int nInl; };

static int max_its(int N, double prob, int minInl, int maxIts)
{
    int n;
    if (minInl == N) n = 1;
    else if (N == 0) n = -2147483647 - 1;
    else { const float eps = (float)minInl / N; const double x = std::ceil(std::log(1 - prob) / std::log(1 - std::pow((double)eps, 3.0))); n = (std::isfinite(x) && x >= -2147483648.0 && x < 2147483648.0) ? (int)x : -2147483647 - 1; }
    return std::max(1, std::min(n, maxIts));
}

static void gather(Scene& S, bool fix, Expect& E)
{
    E.corr.clear(); E.index1.clear(); E.queue.clear();
    E.mN1 = (int)S.matched.size();
    const cv::Mat R1 = S.kf1.GetRotation(), t1 = S.kf1.GetTranslation(), R2 = S.kf2.GetRotation(), t2 = S.kf2.GetTranslation();
    for (int i = 0; i < E.mN1; i++) {
        MapPoint* a = S.kf1.mvpMapPoints[i]; MapPoint* b = S.matched[i];
        if (!a || !b || a->isBad() || b->isBad()) continue;
        const int i1 = a->GetIndexInKeyFrame(&S.kf1), i2 = b->GetIndexInKeyFrame(&S.kf2);
        if (i1 < 0 || i2 < 0) continue;
        const cv::Mat X1 = R1 * a->GetWorldPos() + t1, X2 = R2 * b->GetWorldPos() + t2;
        orbhip_sim3_corr c;
        for (int r = 0; r < 3; r++) { c.X1[r] = X1.at<float>(r); c.X2[r] = X2.at<float>(r); }
        c.sigma2_1 = S.kf1.mvLevelSigma2[S.kf1.mvKeysUn[i1].octave]; c.sigma2_2 = S.kf2.mvLevelSigma2[S.kf2.mvKeysUn[i2].octave];
        E.corr.push_back(c); E.index1.push_back(i);
    }
    E.N = (int)E.corr.size(); E.its = 0; E.best_in = 0; E.fix = fix; E.has_best = false;
    const cv::Mat &A = S.kf1.mK, &B = S.kf2.mK;
    E.K1[0] = A.at<float>(0, 0); E.K1[1] = A.at<float>(1, 1); E.K1[2] = A.at<float>(0, 2); E.K1[3] = A.at<float>(1, 2);
    E.K2[0] = B.at<float>(0, 0); E.K2[1] = B.at<float>(1, 1); E.K2[2] = B.at<float>(0, 2); E.K2[3] = B.at<float>(1, 2);
    E.minInl = 6; E.maxIts = max_its(E.N, 0.99, 6, 300);
}

// the triples of one call: queued ones first, the rest replayed from the Random log (which asserts the calls' ranges)
static int take(Expect& E, int n, std::vector<int32_t>& tri)
{
    const int need = std::max(0, std::min(n, E.maxIts - E.its));
    tri.clear();
    while ((int)tri.size() < 3 * need && !E.queue.empty()) { tri.push_back(E.queue.front()); E.queue.pop_front(); }
    const std::vector<DUtils::Random::Call>& log = DUtils::Random::Log();
    while ((int)tri.size() < 3 * need) {
        std::vector<int> avail(E.N);
        for (int i = 0; i < E.N; i++) avail[i] = i;
        for (int k = 0; k < 3; k++) {
            if (g_logpos >= log.size()) { std::printf("RandomInt was called %d times, more were expected\n", (int)log.size()); return -1; }
            const DUtils::Random::Call& c = log[g_logpos++];
            if (c.min != 0 || c.max != (int)avail.size() - 1) { std::printf("RandomInt call %d has the range %d..%d, expected 0..%d\n", (int)g_logpos - 1, c.min, c.max, (int)avail.size() - 1); return -1; }
            tri.push_back(avail[c.value]); avail[c.value] = avail.back(); avail.pop_back();
        }
    }
    return need;
}

static int step(Expect& E, int n, Answer& A)
{
    A.has_T = false; A.noMore = false; A.inl.assign(E.mN1, false); A.nInl = 0;
    if (E.N < E.minInl || E.N < 3) { A.noMore = true; return 0; }
    std::vector<int32_t> tri;
    const int need = take(E, n, tri);
    if (need < 0) return 1;
    std::vector<uint8_t> inl(E.N + 1, 9);
    orbhip_sim3_problem Q;
    std::memset(&Q, 0, sizeof Q);
    std::memcpy(Q.K1, E.K1, sizeof Q.K1); std::memcpy(Q.K2, E.K2, sizeof Q.K2);
    Q.corr = &E.corr[0]; Q.n = E.N; Q.fix_scale = E.fix; Q.gemm_mode = g_mode; Q.triples = tri.empty() ? 0 : &tri[0]; Q.n_hyp = need;
    Q.min_inliers = E.minInl; Q.best_inliers_in = E.best_in; Q.inliers = &inl[0];
    if (orbhip_sim3_iterate(0, &Q) != ORBHIP_OK) { std::printf("orbhip_sim3_iterate: %s\n", orbhip_last_error()); return 2; }
    if (inl[E.N] != 9) { std::printf("the C ABI wrote past its inlier flags\n"); return 1; }
    E.its += Q.n_consumed;
    for (int k = (int)tri.size() - 1; k >= 3 * Q.n_consumed; k--) E.queue.push_front(tri[k]);
    if (Q.best >= 0) {
        E.has_best = true; E.best_in = Q.best_inliers_out;
        std::memcpy(E.T, Q.T12, sizeof E.T); std::memcpy(E.R, Q.R12, sizeof E.R); std::memcpy(E.t, Q.t12, sizeof E.t); E.s = Q.s12;
        if (Q.returned >= 0) {
            A.has_T = true; std::memcpy(A.T, Q.T12, sizeof A.T); A.nInl = Q.best_inliers_out;
            for (int i = 0; i < E.N; i++) if (inl[i]) A.inl[E.index1[i]] = true;
            return 0;
        }
    }
    A.noMore = E.its >= E.maxIts;
    return 0;
}

static bool same_mat(const cv::Mat& m, const float* want, int rows, int cols)
{
    if (m.rows != rows || m.cols != cols) return false;
    for (int r = 0; r < rows; r++) for (int c = 0; c < cols; c++) { const float a = m.at<float>(r, c); if (std::memcmp(&a, want + r * cols + c, 4)) return false; }
    return true;
}

static int compare(const char* what, const cv::Mat& T, bool noMore, const std::vector<bool>& inl, int nInl, const Answer& A)
{
    if (T.empty() == A.has_T) { std::printf("%s: a matrix was %sreturned, the C ABI says otherwise\n", what, T.empty() ? "not " : ""); return 1; }
    if (A.has_T && !same_mat(T, A.T, 4, 4)) { std::printf("%s: T12 differs from the C ABI's\n", what); return 1; }
    if (noMore != A.noMore || nInl != A.nInl || inl != A.inl) { std::printf("%s: bNoMore %d/%d, nInliers %d/%d, flags %s\n", what, (int)noMore, (int)A.noMore, nInl, A.nInl, inl == A.inl ? "equal" : "differ"); return 1; }
    if (g_logpos != DUtils::Random::Log().size()) { std::printf("%s: RandomInt was called %d times, %d were expected\n", what, (int)DUtils::Random::Log().size(), (int)g_logpos); return 1; }
    return 0;
}

static int getters(const char* what, Sim3Solver& S, const Expect& E)
{
    if (!E.has_best) return 0;
    if (!same_mat(S.GetEstimatedRotation(), E.R, 3, 3) || !same_mat(S.GetEstimatedTranslation(), E.t, 3, 1) || S.GetEstimatedScale() != E.s) { std::printf("%s: the getters differ from the C ABI's best\n", what); return 1; }
    return 0;
}

int main()
{
    if (const char* e = std::getenv("ORBHIP_GEMM_MODE")) g_mode = std::atoi(e);
    {
        Scene S; make_scene(S, 40, 1.0, 0.2);
        if (g_mode == 2) {
            try { Probe P(&S.kf1, &S.kf2, S.matched, true); }
            catch (const ORBhipError& e) { std::printf("sim3_cpp ok: gemm mode 2 refused at construction (%s)\n", e.what()); return 0; }
            std::printf("gemm mode 2 must be refused at construction\n"); return 1;
        }
    }
    try {
        // A: rounds of iterate(5) with the default parameters until the solver returns; then one more round, which starts with the queued triples
        Scene SA; make_scene(SA, 260, 1.0, 0.25);
        Expect EA; gather(SA, true, EA);
        Probe A(&SA.kf1, &SA.kf2, SA.matched, true);
        if (A.N != EA.N || EA.N < 100 || EA.N > 200) { std::printf("A: %d correspondences, the direct filter keeps %d\n", A.N, EA.N); return 1; }
        A.SetRansacParameters(0.99, 20, 300); EA.minInl = 20; EA.maxIts = max_its(EA.N, 0.99, 20, 300); EA.its = 0;
        if (A.mRansacMaxIts != EA.maxIts) { std::printf("A: mRansacMaxIts %d, expected %d\n", A.mRansacMaxIts, EA.maxIts); return 1; }
        int rounds = 0, queued = 0;
        for (;;) {
            bool noMore; std::vector<bool> inl; int nInl; Answer W;
            const cv::Mat T = A.iterate(5, noMore, inl, nInl);
            if (step(EA, 5, W) || compare("A", T, noMore, inl, nInl, W) || getters("A", A, EA)) return 1;
            if (A.mnIterations != EA.its || A.mqDrawn.size() != EA.queue.size()) { std::printf("A: %d iterations, %d queued; expected %d, %d\n", A.mnIterations, (int)A.mqDrawn.size(), EA.its, (int)EA.queue.size()); return 1; }
            rounds++;
            if (!T.empty()) { queued = (int)EA.queue.size(); if (nInl <= 20 || (int)inl.size() != 260) { std::printf("A: returned with %d inliers\n", nInl); return 1; } break; }
            if (noMore || rounds > 60) { std::printf("A: no return in %d rounds\n", rounds); return 1; }
        }
        if (queued == 0 || queued % 3) { std::printf("A: the return left %d queued indices; the scene must leave some (a multiple of 3)\n", queued); return 1; }
        {
            const size_t before = DUtils::Random::Log().size();
            bool noMore; std::vector<bool> inl; int nInl; Answer W;
            const cv::Mat T = A.iterate(5, noMore, inl, nInl);
            if (step(EA, 5, W) || compare("A after the return", T, noMore, inl, nInl, W) || getters("A after the return", A, EA)) return 1;
            if ((int)(DUtils::Random::Log().size() - before) != 15 - queued) { std::printf("A: %d calls after the return, expected %d\n", (int)(DUtils::Random::Log().size() - before), 15 - queued); return 1; }
        }
        // B: find() with a free scale on a scene of scale 1.3
        Scene SB; make_scene(SB, 120, 1.3, 0.2);
        Expect EB; gather(SB, false, EB);
        Probe B(&SB.kf1, &SB.kf2, SB.matched, false);
        {
            std::vector<bool> inl; int nInl; Answer W;
            const cv::Mat T = B.find(inl, nInl);
            if (step(EB, EB.maxIts, W) || compare("B", T, false, inl, nInl, W) || getters("B", B, EB)) return 1;
            if (T.empty() || std::fabs(B.GetEstimatedScale() - 1.3f) > 0.1f) { std::printf("B: find() did not recover the scale (%g)\n", B.GetEstimatedScale()); return 1; }
        }
        // C: mostly wrong matches, 60 inliers asked for, at most 7 iterations: 5 + 2, then no more - the second round has fewer iterations left than asked
        Scene SC; make_scene(SC, 260, 1.0, 0.8);
        Expect EC; gather(SC, true, EC);
        Probe Cs(&SC.kf1, &SC.kf2, SC.matched, true);
        Cs.SetRansacParameters(0.99, 60, 7); EC.minInl = 60; EC.maxIts = max_its(EC.N, 0.99, 60, 7);
        if (Cs.mRansacMaxIts != 7 || EC.maxIts != 7) { std::printf("C: mRansacMaxIts %d\n", Cs.mRansacMaxIts); return 1; }
        for (int r = 0; r < 3; r++) {
            const size_t before = DUtils::Random::Log().size();
            bool noMore; std::vector<bool> inl; int nInl; Answer W;
            const cv::Mat T = Cs.iterate(5, noMore, inl, nInl);
            if (step(EC, 5, W) || compare("C", T, noMore, inl, nInl, W) || getters("C", Cs, EC)) return 1;
            const int calls = (int)(DUtils::Random::Log().size() - before), want[3] = {15, 6, 0};
            if (!T.empty() || noMore != (r >= 1) || calls != want[r]) { std::printf("C round %d: %d calls, bNoMore %d\n", r, calls, (int)noMore); return 1; }
        }
        // D: IterateBatch over {NULL, S1, S2, NULL, S3 (two correspondences)}, two rounds, against solvers run alone on the same draws
        Scene S1; make_scene(S1, 200, 1.0, 0.5);
        Scene S2; make_scene(S2, 90, 1.3, 0.3);
        Scene S3; make_scene(S3, 3, 1.0, 0.0);
        Expect E1, E2, E3; gather(S1, true, E1); gather(S2, false, E2); gather(S3, true, E3);
        Probe P1(&S1.kf1, &S1.kf2, S1.matched, true), P2(&S2.kf1, &S2.kf2, S2.matched, false), P3(&S3.kf1, &S3.kf2, S3.matched, true);
        P1.SetRansacParameters(0.99, 70, 300); E1.minInl = 70; E1.maxIts = max_its(E1.N, 0.99, 70, 300);
        P2.SetRansacParameters(0.99, 20, 300); E2.minInl = 20; E2.maxIts = max_its(E2.N, 0.99, 20, 300);
        if (E3.N >= 3) { std::printf("D: the short scene keeps %d correspondences\n", E3.N); return 1; }
        std::vector<Sim3Solver*> list;
        list.push_back(0); list.push_back(&P1); list.push_back(&P2); list.push_back(0); list.push_back(&P3);
        for (int r = 0; r < 2; r++) {
            std::vector<cv::Mat> vT; std::vector<bool> vNoMore; std::vector<std::vector<bool> > vInl; std::vector<int> vn;
            Sim3Solver::IterateBatch(list, 5, vT, vNoMore, vInl, vn);
            if (vT.size() != 5 || vNoMore.size() != 5 || vInl.size() != 5 || vn.size() != 5) { std::printf("D: output sizes\n"); return 1; }
            if (!vT[0].empty() || vNoMore[0] || !vInl[0].empty() || vn[0] || !vT[3].empty() || vNoMore[3]) { std::printf("D: NULL entries must be skipped\n"); return 1; }
            Answer W1, W2, W3;
            if (step(E1, 5, W1) || step(E2, 5, W2) || step(E3, 5, W3)) return 1;
            if (compare("D solver 1", vT[1], vNoMore[1], vInl[1], vn[1], W1) || compare("D solver 2", vT[2], vNoMore[2], vInl[2], vn[2], W2) ||
                compare("D short solver", vT[4], vNoMore[4], vInl[4], vn[4], W3)) return 1;
            if (getters("D solver 1", P1, E1) || getters("D solver 2", P2, E2)) return 1;
            if (!W3.noMore || (int)vInl[4].size() != 3) { std::printf("D: the short solver must report bNoMore\n"); return 1; }
        }
        // SetRansacParameters on its own, for the model to compare: also epsilon >= 1 and the degenerate sizes
        const int table[8][3] = {{150, 20, 300}, {150, 6, 300}, {64, 40, 13}, {10, 10, 300}, {10, 11, 300}, {10, 20, 300}, {260, 1, 300}, {100, 0, 50}};
        for (int k = 0; k < 8; k++) {
            Scene S; make_scene(S, 5, 1.0, 0.0);
            Probe P(&S.kf1, &S.kf2, S.matched, true);
            P.mvCorr.assign(8 * (size_t)table[k][0], 1.0f);                      // (only the number of correspondences matters here)
            P.SetRansacParameters(0.99, table[k][1], table[k][2]);
            if (P.mRansacMaxIts != max_its(table[k][0], 0.99, table[k][1], table[k][2])) { std::printf("SetRansacParameters(%d, %d, %d) gives %d\n", table[k][0], table[k][1], table[k][2], P.mRansacMaxIts); return 1; }
            std::printf("maxits %d %d %d -> %d\n", table[k][0], table[k][1], table[k][2], P.mRansacMaxIts);
        }
        {
            Scene S; make_scene(S, 5, 1.0, 0.0);
            std::vector<MapPoint*> none(5, (MapPoint*)0);
            Probe P(&S.kf1, &S.kf2, none, true);                                // N == 0
            bool noMore = false; std::vector<bool> inl; int nInl = -1;
            const size_t before = DUtils::Random::Log().size();
            if (P.N != 0 || P.mRansacMaxIts != 1 || !P.iterate(5, noMore, inl, nInl).empty() || !noMore || nInl != 0 || inl.size() != 5 || DUtils::Random::Log().size() != before) { std::printf("N == 0: mRansacMaxIts %d\n", P.mRansacMaxIts); return 1; }
            std::printf("maxits 0 6 300 -> %d\n", P.mRansacMaxIts);
        }
        std::printf("sim3_cpp ok: gemm mode %d, A returned after %d rounds with %d indices queued, %d RandomInt calls in all\n", g_mode, rounds, queued, (int)DUtils::Random::Log().size());
    } catch (const std::exception& e) { std::printf("Sim3Solver: %s\n", e.what()); return 2; }
    return 0;
}
