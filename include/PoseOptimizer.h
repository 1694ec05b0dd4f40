// PoseOptimizer.h — Optimizer::PoseOptimization (Optimizer.cc:239-451) on the device (orbhip_pose_optimization, include/orbhip.h).
// Same contract as the reference's member: reads pFrame->mvpMapPoints, mvKeysUn, mvuRight, mvInvLevelSigma2, fx, fy, cx, cy, mbf and mTcw, writes
// mvbOutlier for every index that has a map point, calls pFrame->SetPose and returns the number of inliers.  To use it, forward the member:
//     int Optimizer::PoseOptimization(Frame *pFrame) { return PoseOptimizationDevice(pFrame); }
// (INTEGRATION.md step 3m).  A failed device call throws ORBhipError.
#ifndef POSEOPTIMIZER_H
#define POSEOPTIMIZER_H

#include <vector>

namespace ORB_SLAM2
{

class Frame;

int PoseOptimizationDevice(Frame* pFrame);

// Several frames in one device call (Tracking::Relocalization's candidates): element i of the result is what PoseOptimizationDevice(vpFrames[i])
// returns, bit for bit; NULL elements are skipped (0).
std::vector<int> PoseOptimizationDevice(const std::vector<Frame*> &vpFrames);

} // namespace ORB_SLAM2

#endif // POSEOPTIMIZER_H
