// Drives ORB_SLAM2::OptimizeSim3Device (include/Sim3Optimizer.h, orb_slam2_amd/cpp/Sim3Optimizer.cc) on stand-in key frames and a stand-in Sim3 type,
// single and batched, and compares with the C ABI called directly on pairs gathered here: S12, the matches set to NULL and the return values must be
// equal bit for bit.  The scenes contain every skip of the member's set-up loop: no match, no map point in pKF1, either point bad, the matched point not
// observed in pKF2.  Stand-alone: it links the library named on its build line (the emulation build in the CPU suite, liborbhip.so on the device) and
// prints "sim3_opt_cpp ok".
#include "Sim3Optimizer.h"
#include "KeyFrame.h"
#include "MapPoint.h"
#include "Sim3Stub.h"
#include "orbhip.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

using namespace ORB_SLAM2;

static unsigned long long g_state = 0x9E3779B97F4A7C15ull;
static double uniform() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (double)(g_state >> 11) / 9007199254740992.0; }
static double normal() { double s = 0; for (int i = 0; i < 12; i++) s += uniform(); return s - 6.0; }

static void rot_y(double a, double R[9]) { const double m[9] = {std::cos(a), 0, std::sin(a), 0, 1, 0, -std::sin(a), 0, std::cos(a)}; memcpy(R, m, sizeof m); }
static void set_pose(KeyFrame& kf, double yaw, double tx, double ty, double tz)
{
    double R[9]; rot_y(yaw, R);
    for (int i = 0; i < 9; i++) kf.mRcw.at<float>(i / 3, i % 3) = (float)R[i];
    kf.mtcw.at<float>(0) = (float)tx; kf.mtcw.at<float>(1) = (float)ty; kf.mtcw.at<float>(2) = (float)tz;
}
static void set_camera(KeyFrame& kf, float fx, float fy, float cx, float cy, int nkp)
{
    kf.mK = cv::Mat::eye(3, 3, CV_32F);
    kf.mK.at<float>(0, 0) = fx; kf.mK.at<float>(1, 1) = fy; kf.mK.at<float>(0, 2) = cx; kf.mK.at<float>(1, 2) = cy;
    kf.mvInvLevelSigma2.resize(8);
    float sf = 1.0f;
    for (int l = 0; l < 8; l++) { kf.mvInvLevelSigma2[l] = 1.0f / (sf * sf); sf = (float)(sf * 1.2); }
    kf.mvKeysUn.resize(nkp); kf.mvpMapPoints.assign(nkp, (MapPoint*)0);
}
// world position of a camera-frame point: R^T (Xc - t), the pose read back from the key frame's float matrices
static MapPoint* add_point(std::vector<std::unique_ptr<MapPoint> >& store, KeyFrame& kf, const double Xc[3], KeyFrame* observer, int idx)
{
    double w[3];
    for (int c = 0; c < 3; c++) { w[c] = 0; for (int r = 0; r < 3; r++) w[c] += (double)kf.mRcw.at<float>(r, c) * (Xc[r] - (double)kf.mtcw.at<float>(r)); }
    store.push_back(std::unique_ptr<MapPoint>(new MapPoint((float)w[0], (float)w[1], (float)w[2], observer, idx)));
    return store.back().get();
}

struct Candidate { KeyFrame kf2; std::vector<MapPoint*> matches; StubSim3 S12; double s, yaw, t[3]; };
struct Scene { KeyFrame kf1, other; std::vector<std::unique_ptr<MapPoint> > points; std::vector<std::unique_ptr<Candidate> > cands; std::vector<double> X1c; };

static void make_kf1(Scene& S, int nkp)
{
    set_camera(S.kf1, 520.9f, 521.0f, 325.1f, 249.7f, nkp);
    set_pose(S.kf1, 0.1, 0.3, -0.2, 0.5);
    S.X1c.resize(3 * nkp);
    for (int i = 0; i < nkp; i++) {
        const double z = 4 + 8 * uniform(), X[3] = {(30 + 580 * uniform() - 325.1) / 520.9 * z, (30 + 420 * uniform() - 249.7) / 521.0 * z, z};
        memcpy(&S.X1c[3 * i], X, sizeof X);
        cv::KeyPoint& k = S.kf1.mvKeysUn[i];
        k.octave = (int)(8 * uniform()) & 7;
        const double sigma = std::pow(1.2, k.octave);
        k.pt.x = (float)(X[0] / z * 520.9 + 325.1 + sigma * normal()); k.pt.y = (float)(X[1] / z * 521.0 + 249.7 + sigma * normal());
        if (i % 11 == 3) continue;                                             // no map point in pKF1
        S.kf1.mvpMapPoints[i] = add_point(S.points, S.kf1, X, &S.kf1, i);
        if (i % 13 == 4) S.kf1.mvpMapPoints[i]->mbBad = true;
    }
}
// a candidate key frame: X1c = s Ry(yaw) X2c + t; key point i2 = nkp - 1 - i of kf2 observes the point matched to key point i of kf1
static Candidate& add_candidate(Scene& S, double s, double yaw, double tx, double ty, double tz, double wrong)
{
    const int nkp = (int)S.kf1.mvKeysUn.size();
    S.cands.push_back(std::unique_ptr<Candidate>(new Candidate()));
    Candidate& C = *S.cands.back();
    C.s = s; C.yaw = yaw; C.t[0] = tx; C.t[1] = ty; C.t[2] = tz;
    set_camera(C.kf2, 458.6f, 457.3f, 367.2f, 248.4f, nkp);
    set_pose(C.kf2, -0.15, -0.4, 0.1, 0.2);
    C.matches.assign(nkp, (MapPoint*)0);
    double R[9]; rot_y(yaw, R);
    for (int i = 0; i < nkp; i++) {
        const double* X1 = &S.X1c[3 * i];
        const double d[3] = {(X1[0] - tx) / s, (X1[1] - ty) / s, (X1[2] - tz) / s};
        double X2[3];
        for (int c = 0; c < 3; c++) X2[c] = R[c] * d[0] + R[3 + c] * d[1] + R[6 + c] * d[2];        // R^T d
        const int i2 = nkp - 1 - i;
        cv::KeyPoint& k = C.kf2.mvKeysUn[i2];
        k.octave = (int)(8 * uniform()) & 7;
        const double sigma = std::pow(1.2, k.octave);
        k.pt.x = (float)(X2[0] / X2[2] * 458.6 + 367.2 + sigma * normal()); k.pt.y = (float)(X2[1] / X2[2] * 457.3 + 248.4 + sigma * normal());
        if (uniform() < wrong) { k.pt.x += 45.0f; k.pt.y -= 30.0f; }
        if (i % 5 == 0) continue;                                              // no match
        MapPoint* p = add_point(S.points, C.kf2, X2, i % 19 == 6 ? &S.other : &C.kf2, i2);          // i % 19 == 6: not observed in pKF2, i2 < 0
        if (i % 17 == 5) p->mbBad = true;
        C.matches[i] = p;
    }
    // the initial S12: the true one, perturbed; the quaternion of a rotation about y
    const double a = yaw + 0.02;
    C.S12.r.v[0] = 0.0; C.S12.r.v[1] = std::sin(a / 2); C.S12.r.v[2] = 0.0; C.S12.r.v[3] = std::cos(a / 2);
    C.S12.t.v[0] = tx + 0.04; C.S12.t.v[1] = ty - 0.03; C.S12.t.v[2] = tz + 0.05; C.S12.s = s * 1.02;
    C.S12.writes = 0;
    return C;
}

struct Direct { std::vector<orbhip_sim3_pair> pairs; std::vector<int> index; std::vector<uint8_t> removed; orbhip_sim3_opt_problem Q; };

// the member's set-up loop, written again here
static int direct(KeyFrame& kf1, Candidate& C, float th2, bool fix, Direct& D)
{
    D.pairs.clear(); D.index.clear();
    const cv::Mat R1w = kf1.GetRotation(), t1w = kf1.GetTranslation(), R2w = C.kf2.GetRotation(), t2w = C.kf2.GetTranslation();
    for (size_t i = 0; i < C.matches.size(); i++) {
        MapPoint* p1 = kf1.mvpMapPoints[i]; MapPoint* p2 = C.matches[i];
        if (!p2 || !p1 || p1->isBad() || p2->isBad()) continue;
        const int i2 = p2->GetIndexInKeyFrame(&C.kf2);
        if (i2 < 0) continue;
        const cv::Mat X1 = R1w * p1->GetWorldPos() + t1w, X2 = R2w * p2->GetWorldPos() + t2w;
        const cv::KeyPoint &k1 = kf1.mvKeysUn[i], &k2 = C.kf2.mvKeysUn[i2];
        orbhip_sim3_pair p = {k1.pt.x, k1.pt.y, kf1.mvInvLevelSigma2[k1.octave], k2.pt.x, k2.pt.y, C.kf2.mvInvLevelSigma2[k2.octave],
                              {X1.at<float>(0), X1.at<float>(1), X1.at<float>(2)}, {X2.at<float>(0), X2.at<float>(1), X2.at<float>(2)}};
        D.pairs.push_back(p); D.index.push_back((int)i);
    }
    D.removed.assign(D.pairs.size() + 1, 9);
    orbhip_sim3_opt_problem& Q = D.Q;
    memset(&Q, 0, sizeof Q);
    const orbhip_sim3_cameras cam = {kf1.mK.at<float>(0, 0), kf1.mK.at<float>(1, 1), kf1.mK.at<float>(0, 2), kf1.mK.at<float>(1, 2),
                                     C.kf2.mK.at<float>(0, 0), C.kf2.mK.at<float>(1, 1), C.kf2.mK.at<float>(0, 2), C.kf2.mK.at<float>(1, 2)};
    Q.cam = cam;
    for (int k = 0; k < 4; k++) Q.S12_in[k] = C.S12.r.v[k];
    for (int k = 0; k < 3; k++) Q.S12_in[4 + k] = C.S12.t.v[k];
    Q.S12_in[7] = C.S12.s;
    memcpy(Q.S12_out, Q.S12_in, sizeof Q.S12_out);
    Q.pairs = D.pairs.empty() ? 0 : &D.pairs[0]; Q.n = (int)D.pairs.size(); Q.th2 = th2; Q.fix_scale = fix; Q.removed = &D.removed[0]; Q.n_inliers = -1;
    return orbhip_sim3_optimize(0, &Q);
}

// after the drop-in ran on C (its matches and S12 updated) against what the direct call left in D, computed BEFORE from the same inputs
static int check(const char* what, const Candidate& C, const std::vector<MapPoint*>& before, const Direct& D, int returned, int expect_pairs)
{
    if ((int)D.pairs.size() != expect_pairs) { std::printf("%s: %d pairs gathered, %d expected\n", what, (int)D.pairs.size(), expect_pairs); return 1; }
    if (returned != D.Q.n_inliers) { std::printf("%s: returned %d, the C ABI %d\n", what, returned, D.Q.n_inliers); return 1; }
    double got[8];
    for (int k = 0; k < 4; k++) got[k] = C.S12.r.v[k];
    for (int k = 0; k < 3; k++) got[4 + k] = C.S12.t.v[k];
    got[7] = C.S12.s;
    if (memcmp(got, D.Q.S12_out, sizeof got)) { std::printf("%s: S12 differs from the C ABI's\n", what); return 1; }
    std::vector<MapPoint*> want = before;
    int nremoved = 0;
    for (size_t e = 0; e < D.pairs.size(); e++) if (D.removed[e] == 1) { want[D.index[e]] = 0; nremoved++; } else if (D.removed[e] != 0) { std::printf("%s: flag %d\n", what, D.removed[e]); return 1; }
    if (D.removed[D.pairs.size()] != 9) { std::printf("%s: a flag past the n-th was written\n", what); return 1; }
    if (want != C.matches) { std::printf("%s: the matches set to NULL differ\n", what); return 1; }
    std::printf("%s: %d pairs, %d removed, %d inliers\n", what, (int)D.pairs.size(), nremoved, returned);
    return 0;
}

static int count_pairs(int nkp)
{
    int n = 0;
    for (int i = 0; i < nkp; i++) if (!(i % 5 == 0 || i % 11 == 3 || i % 13 == 4 || i % 17 == 5 || i % 19 == 6)) n++;
    return n;
}

int main()
{
    int bad = 0;
    {   // single calls: the scale free and fixed
        Scene S; make_kf1(S, 160);
        for (int fix = 0; fix < 2; fix++) {
            Candidate& C = add_candidate(S, fix ? 1.0 : 1.3, 0.3, 0.2, -0.1, 0.3, 0.15);
            if (fix) C.S12.s = 1.0;
            Direct D;
            if (direct(S.kf1, C, 10.0f, fix != 0, D) != ORBHIP_OK) { std::printf("direct: %s\n", orbhip_last_error()); return 1; }
            const std::vector<MapPoint*> before = C.matches;
            const int n = OptimizeSim3Device(&S.kf1, &C.kf2, C.matches, C.S12, 10.0f, fix != 0);
            bad += check(fix ? "single, fixed scale" : "single", C, before, D, n, count_pairs(160));
            if (n < 20 || C.S12.writes == 0) { std::printf("single: %d inliers, %d writes: the scene should converge\n", n, C.S12.writes); bad++; }
            if (fix && C.S12.s != 1.0) { std::printf("fixed scale: the scale moved\n"); bad++; }
        }
    }
    {   // fewer than 10 pairs: the member returns 0 and leaves g2oS12 alone
        Scene S; make_kf1(S, 14);
        Candidate& C = add_candidate(S, 1.1, 0.2, 0.1, 0.1, -0.2, 0.0);
        Direct D;
        if (direct(S.kf1, C, 10.0f, false, D) != ORBHIP_OK) { std::printf("direct: %s\n", orbhip_last_error()); return 1; }
        const std::vector<MapPoint*> before = C.matches;
        const int n = OptimizeSim3Device(&S.kf1, &C.kf2, C.matches, C.S12, 10.0f, false);
        bad += check("early return", C, before, D, n, count_pairs(14));
        if (n != 0 || C.S12.writes != 0 || count_pairs(14) >= 10) { std::printf("early return: %d returned, %d writes to S12\n", n, C.S12.writes); bad++; }
    }
    {   // a batch: three candidates of different sizes of similarity, a NULL one among them, against the single calls
        Scene S; make_kf1(S, 120);
        const double par[3][5] = {{0.7, -0.25, 0.3, 0.2, 0.1}, {1.0, 0.1, -0.2, 0.1, 0.4}, {1.6, 0.35, 0.1, -0.3, -0.2}};
        std::vector<Sim3OptCandidate<StubSim3> > v;
        std::vector<Direct> D(3);
        std::vector<std::vector<MapPoint*> > before(3);
        for (int k = 0; k < 3; k++) {
            Candidate& C = add_candidate(S, par[k][0], par[k][1], par[k][2], par[k][3], par[k][4], 0.1 * k);
            if (direct(S.kf1, C, 10.0f, false, D[k]) != ORBHIP_OK) { std::printf("direct: %s\n", orbhip_last_error()); return 1; }
            before[k] = C.matches;
            if (k == 1) { const Sim3OptCandidate<StubSim3> none = {0, 0, 0}; v.push_back(none); }
            const Sim3OptCandidate<StubSim3> c = {&C.kf2, &C.matches, &C.S12};
            v.push_back(c);
        }
        const std::vector<int> n = OptimizeSim3Device(&S.kf1, v, 10.0f, false);
        if (n.size() != 4 || n[1] != 0) { std::printf("batch: %d results, the NULL candidate returned %d\n", (int)n.size(), n.size() > 1 ? n[1] : -1); bad++; }
        else for (int k = 0; k < 3; k++) bad += check("batch", *S.cands[k], before[k], D[k], n[k < 1 ? k : k + 1], count_pairs(120));
        const std::vector<Sim3OptCandidate<StubSim3> > empty;
        if (!OptimizeSim3Device(&S.kf1, empty, 10.0f, false).empty()) { std::printf("empty batch\n"); bad++; }
    }
    if (bad) { std::printf("sim3_opt_cpp: %d failures\n", bad); return 1; }
    std::printf("sim3_opt_cpp ok\n");
    return 0;
}
