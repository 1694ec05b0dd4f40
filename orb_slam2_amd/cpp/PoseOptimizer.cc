// PoseOptimizer.cc — Optimizer::PoseOptimization (Optimizer.cc:239-451) as one device call per frame, or one per list of frames
// (orbhip_pose_optimization / orbhip_pose_optimization_batch, include/orbhip.h).  Declared in include/PoseOptimizer.h.
//
// The host part is the member's own set-up loop (Optimizer.cc:277-361): under MapPoint::mGlobalMutex every index with a map point becomes one observation -
// the undistorted key point, mvuRight (negative: monocular), mvInvLevelSigma2 of its octave and the point's position from GetWorldPos(), which takes
// MapPoint::mMutexPos as the matchers' gathers do - and its mvbOutlier is cleared.  With fewer than 3 observations the member returns 0 there; so does this.
// Everything after (four rounds of Levenberg-Marquardt, the classification, the final pose) runs on the device.
#include "PoseOptimizer.h"
#include "Frame.h"
#include "MapPoint.h"
#include "ORBextractor.h"   // ORBhipError
#include "orbhip.h"

#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>

using namespace std;

namespace ORB_SLAM2
{

namespace
{

struct FrameProblem
{
    vector<orbhip_pose_obs> vObs;
    vector<size_t> vnIndex;          // the frame index of every observation
    vector<uint8_t> vOutlier;
    orbhip_pose_problem problem;
};

int Device()
{
    static const int device = getenv("ORBHIP_DEVICE") ? atoi(getenv("ORBHIP_DEVICE")) : 0;      // read once per process, like ORBmatcher.cc
    return device;
}

void Gather(Frame* pFrame, FrameProblem &P)
{
    const int N = pFrame->N;
    P.vObs.clear(); P.vnIndex.clear();
    P.vObs.reserve(N); P.vnIndex.reserve(N);
    {
    unique_lock<mutex> lock(MapPoint::mGlobalMutex);
    for(int i=0; i<N; i++)
    {
        MapPoint* pMP = pFrame->mvpMapPoints[i];
        if(!pMP) continue;
        pFrame->mvbOutlier[i] = false;
        const cv::KeyPoint &kpUn = pFrame->mvKeysUn[i];
        const cv::Mat Xw = pMP->GetWorldPos();
        orbhip_pose_obs o;
        o.u = kpUn.pt.x; o.v = kpUn.pt.y; o.u_right = pFrame->mvuRight[i];
        o.inv_sigma2 = pFrame->mvInvLevelSigma2[kpUn.octave];
        o.X = Xw.at<float>(0); o.Y = Xw.at<float>(1); o.Z = Xw.at<float>(2);
        P.vObs.push_back(o);
        P.vnIndex.push_back(i);
    }
    }
    P.vOutlier.assign(P.vObs.size(), 0);
    orbhip_pose_problem &Q = P.problem;
    memset(&Q, 0, sizeof Q);
    Q.cam.fx = pFrame->fx; Q.cam.fy = pFrame->fy; Q.cam.cx = pFrame->cx; Q.cam.cy = pFrame->cy; Q.cam.bf = pFrame->mbf;
    for(int r=0; r<4; r++)
        for(int c=0; c<4; c++)
            Q.Tcw_in[4*r+c] = pFrame->mTcw.at<float>(r,c);
    Q.n = (int)P.vObs.size();
}

// the pointers are set once the problem lies where it stays
void Bind(FrameProblem &P)
{
    P.problem.obs = P.vObs.empty() ? NULL : &P.vObs[0];
    P.problem.outlier = P.vOutlier.empty() ? NULL : &P.vOutlier[0];
}

int Scatter(Frame* pFrame, const FrameProblem &P)
{
    if(P.problem.n<3)
        return 0;
    for(size_t k=0; k<P.vnIndex.size(); k++)
        pFrame->mvbOutlier[P.vnIndex[k]] = P.vOutlier[k]!=0;
    cv::Mat pose(4,4,CV_32F);
    for(int r=0; r<4; r++)
        for(int c=0; c<4; c++)
            pose.at<float>(r,c) = P.problem.Tcw_out[4*r+c];
    pFrame->SetPose(pose);
    return P.problem.n_inliers;
}

} // namespace

int PoseOptimizationDevice(Frame* pFrame)
{
    FrameProblem P;
    Gather(pFrame, P);
    Bind(P);
    if(orbhip_pose_optimization_batch(Device(), 1, &P.problem)!=ORBHIP_OK)
        throw ORBhipError(string("PoseOptimizationDevice: ") + orbhip_last_error());
    return Scatter(pFrame, P);
}

vector<int> PoseOptimizationDevice(const vector<Frame*> &vpFrames)
{
    vector<int> vnInliers(vpFrames.size(), 0);
    vector<FrameProblem> vP(vpFrames.size());
    vector<orbhip_pose_problem> vQ;
    vector<size_t> vnFrame;
    for(size_t f=0; f<vpFrames.size(); f++)
        if(vpFrames[f])
            Gather(vpFrames[f], vP[f]);
    for(size_t f=0; f<vpFrames.size(); f++)
    {
        if(!vpFrames[f]) continue;
        Bind(vP[f]);
        vQ.push_back(vP[f].problem);
        vnFrame.push_back(f);
    }
    if(vQ.empty())
        return vnInliers;
    if(orbhip_pose_optimization_batch(Device(), (int)vQ.size(), &vQ[0])!=ORBHIP_OK)
        throw ORBhipError(string("PoseOptimizationDevice: ") + orbhip_last_error());
    for(size_t k=0; k<vQ.size(); k++)
    {
        vP[vnFrame[k]].problem = vQ[k];
        vnInliers[vnFrame[k]] = Scatter(vpFrames[vnFrame[k]], vP[vnFrame[k]]);
    }
    return vnInliers;
}

} // namespace ORB_SLAM2
