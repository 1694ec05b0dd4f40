// PnPsolver.h — ORB_SLAM2::PnPsolver (include/PnPsolver.h, src/PnPsolver.cc of the reference) with the RANSAC loop, EPnP, CheckInliers and Refine on
// the device (orbhip_pnp_iterate / orbhip_pnp_iterate_batch, include/orbhip.h).  Same public signatures; INTEGRATION.md step 3o.
//
// The constructor is the reference's: it keeps, for every match whose map point is present and good, the undistorted key point, sigma^2 of its
// level and the point's world position.  The EPnP members of the reference (compute_pose, choose_control_points, find_betas_approx_*, gauss_newton,
// qr_solve, ...) are NOT kept: that arithmetic runs on the device, as DESIGN.md H18 states it.
//
// iterate(n) needs max(n, mRansacMaxIts - mnIterations) hypotheses: the reference's loop is `while(mnIterations<mRansacMaxIts ||
// nCurrentIterations<nIterations)`, an OR.  It takes queued quadruples first and draws the rest with DUtils::Random::RandomInt and the reference's
// swap-remove over mvAllIndices, four per hypothesis, then makes ONE device call for all of them (one per 4096 hypotheses on longer runs; the best
// count, mask and pose carry over between them).
// THE ONE DEVIATION: the reference draws a hypothesis only once the one before has failed to return.  Here the draws of a call are made up front, so
// after an early return at hypothesis `returned`, up to 4 * (n - returned - 1) more values of rand() have been taken than the reference would have
// taken.  Those quadruples are not lost: they stay queued for this solver's next call (a quadruple depends only on N).
//
// SetRansacParameters reproduces the reference's arithmetic (`int nMinInliers = N*mRansacEpsilon` as a float product truncated, both clamps, epsilon
// raised to (float)minInliers/N).  Where the reference's expression for the iteration count is not finite or does not fit an int, or N == 0
// (epsilon >= 1 gives the log of a negative number), the conversion to int is undefined; x86 gives INT_MIN, so mRansacMaxIts = max(1, min(INT_MIN,
// maxIterations)) = 1, and that is what this class computes on every machine.  minSet must be 4, which every caller in the reference passes: the
// device solves EPnP from quadruples, and another value throws ORBhipError.
#ifndef PNPSOLVER_H
#define PNPSOLVER_H

#include <opencv2/core/core.hpp>
#include <deque>
#include <vector>

#include "MapPoint.h"
#include "Frame.h"

namespace ORB_SLAM2
{

class PnPsolver {
 public:
  PnPsolver(const Frame &F, const std::vector<MapPoint*> &vpMapPointMatches);

  ~PnPsolver();

  void SetRansacParameters(double probability = 0.99, int minInliers = 8 , int maxIterations = 300, int minSet = 4, float epsilon = 0.4,
                           float th2 = 5.991);

  cv::Mat find(std::vector<bool> &vbInliers, int &nInliers);

  cv::Mat iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers);

  // One round of Tracking::Relocalization's candidate loop in one device call (one per 4096 hypotheses of the longest run): element i of the
  // outputs is what vpSolvers[i]->iterate(nIterations, ...) gives from the same draws, bit for bit.  NULL entries are skipped (an empty Mat, bNoMore
  // false, no inliers); draws are made in vector order.
  static void IterateBatch(const std::vector<PnPsolver*> &vpSolvers, int nIterations, std::vector<cv::Mat> &vTcw, std::vector<bool> &vbNoMore,
                           std::vector<std::vector<bool> > &vvbInliers, std::vector<int> &vnInliers);

 protected:

  struct Round;                                     // one call's quadruples, problem record and the buffers it points to (PnPsolver.cc)
  bool Prepare(int nIterations, Round &round);      // false: iterate returns before its loop (N < mRansacMinInliers)
  bool NextPart(Round &round);                      // the record of the next device call; false: every hypothesis of the call is consumed
  bool Absorb(Round &round, std::vector<bool> &vbInliers, int &nInliers);      // true: a refine succeeded, round.result is mRefinedTcw
  cv::Mat Finish(bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers);  // what iterate does after its loop

  // the correspondences, as the device reads them: mvP3Dw | mvP2D | mvMaxError, 6 floats each
  std::vector<float> mvCorr;
  std::vector<float> mvSigma2;
  std::vector<size_t> mvKeyPointIndices;
  size_t mnMatches;                                 // vpMapPointMatches.size()

  // Current Ransac State
  int mnIterations;
  std::vector<unsigned char> mvbBestInliers;
  int mnBestInliers;
  cv::Mat mBestTcw;

  // Number of Correspondences
  int N;

  // Indices for random selection [0 .. N-1], and the quadruples drawn but not yet consumed
  std::vector<size_t> mvAllIndices;
  std::deque<int> mqDrawn;

  double mRansacProb;
  int mRansacMinInliers;
  int mRansacMaxIts;
  float mRansacEpsilon;
  int mRansacMinSet;

  // Calibration: fx, fy, cx, cy
  float mK[4];
};

} //namespace ORB_SLAM

#endif //PNPSOLVER_H
