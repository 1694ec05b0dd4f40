// Sim3Solver.h — ORB_SLAM2::Sim3Solver (include/Sim3Solver.h, src/Sim3Solver.cc of the reference) with the RANSAC loop on the device
// (orbhip_sim3_iterate / orbhip_sim3_iterate_batch, include/orbhip.h).  Same public signatures; INTEGRATION.md step 3n.
//
// The constructor is the reference's: it filters the correspondences (both map points present and good, both seen in their key frame), computes
// `Rcw*Xw + tcw` with the caller's own cv::Mat - exact by construction whatever the linked OpenCV does - and keeps sigma^2 of each key point's level.
// It probes how the linked cv::Mat rounds `R*x + t` (orbhip_probe_gemm_mode) and throws ORBhipError where the answer is mode 2:
// every product of the solver is per hypothesis on the device, so there is nothing the caller could evaluate instead.
//
// iterate(n) needs min(n, mRansacMaxIts - mnIterations) hypotheses.  It takes queued triples first and draws the rest with
// DUtils::Random::RandomInt and the reference's swap-remove over mvAllIndices, three per hypothesis, then makes ONE device call for all of them.
// THE ONE DEVIATION: the reference draws a hypothesis only once the one before has failed to return.  Here the draws of a call are made up front, so
// after an early return at hypothesis `returned`, up to 3 * (n - returned - 1) more values of rand() have been taken than the reference would have
// taken.  Those triples are not lost: they stay queued for this solver's next call (a triple depends only on N).
//
// SetRansacParameters: where the reference's expression for the iteration count is not finite or does not fit an int, or N == 0 (epsilon >= 1 gives
// the log of a negative number), the conversion to int is undefined; x86 gives INT_MIN, so mRansacMaxIts = max(1, min(INT_MIN, maxIterations)) = 1,
// and that is what this class computes on every machine.  With N < 3, iterate returns an empty Mat with bNoMore = true (the reference would index an
// empty vector in its draw).
#ifndef SIM3SOLVER_H
#define SIM3SOLVER_H

#include <opencv2/opencv.hpp>
#include <deque>
#include <vector>

#include "KeyFrame.h"

namespace ORB_SLAM2
{

class Sim3Solver
{
public:

    Sim3Solver(KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<MapPoint*> &vpMatched12, const bool bFixScale = true);

    void SetRansacParameters(double probability = 0.99, int minInliers = 6 , int maxIterations = 300);

    cv::Mat find(std::vector<bool> &vbInliers12, int &nInliers);

    cv::Mat iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers);

    cv::Mat GetEstimatedRotation();
    cv::Mat GetEstimatedTranslation();
    float GetEstimatedScale();

    // One round of LoopClosing::ComputeSim3's candidate loop in one device call: element i of the outputs is what
    // vpSolvers[i]->iterate(nIterations, ...) gives from the same draws, bit for bit.  NULL entries are skipped (an empty Mat, bNoMore false, no
    // inliers); draws are made in vector order.
    static void IterateBatch(const std::vector<Sim3Solver*> &vpSolvers, int nIterations, std::vector<cv::Mat> &vScm, std::vector<bool> &vbNoMore,
                             std::vector<std::vector<bool> > &vvbInliers, std::vector<int> &vnInliers);

protected:

    struct Round;                                       // one call's problem record and the buffers it points to (Sim3Solver.cc)
    bool Prepare(int nIterations, Round &round);        // false: iterate returns before its loop (N < mRansacMinInliers or N < 3)
    cv::Mat Absorb(const Round &round, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers);

    // the filtered correspondences, as the device reads them: X3Dc1 | X3Dc2 | sigma^2 of level 1 | of level 2, 8 floats each
    std::vector<float> mvCorr;
    std::vector<size_t> mvnIndices1;

    int N;
    int mN1;

    // Current Ransac State
    int mnIterations;
    std::vector<bool> mvbBestInliers;
    int mnBestInliers;
    cv::Mat mBestT12;
    cv::Mat mBestRotation;
    cv::Mat mBestTranslation;
    float mBestScale;

    bool mbFixScale;
    int mnGemmMode;

    // Indices for random selection, and the triples drawn but not yet consumed
    std::vector<size_t> mvAllIndices;
    std::deque<int> mqDrawn;

    double mRansacProb;
    int mRansacMinInliers;
    int mRansacMaxIts;

    // Calibration: fx, fy, cx, cy
    float mK1[4];
    float mK2[4];
};

} //namespace ORB_SLAM

#endif // SIM3SOLVER_H
