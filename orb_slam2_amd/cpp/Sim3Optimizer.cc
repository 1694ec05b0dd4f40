// Sim3Optimizer.cc — Optimizer::OptimizeSim3 (Optimizer.cc:1046-1241) as one device call per candidate, or one per list of candidates
// (orbhip_sim3_optimize_batch, include/orbhip.h).  Declared in include/Sim3Optimizer.h.
//
// The host part is the member's own set-up loop (Optimizer.cc:1085-1178): every index with a match whose two map points exist, are not bad and whose
// second point is observed in pKF2 becomes one pair - the two undistorted key points, mvInvLevelSigma2 of their octaves and the two camera-frame points
// P3D1c = R1w*P3D1w + t1w and P3D2c = R2w*P3D2w + t2w in cv::Mat's float arithmetic - and its index is kept (vnIndexEdge).  Everything after (both
// optimisations, both checks) runs on the device; the removed pairs' matches are set to NULL here.
#include "Sim3Optimizer.h"
#include "KeyFrame.h"
#include "MapPoint.h"
#include "ORBextractor.h"   // ORBhipError
#include "orbhip.h"

#include <cstdlib>
#include <cstring>
#include <string>

using namespace std;

namespace ORB_SLAM2
{

namespace
{

struct TaskProblem
{
    vector<orbhip_sim3_pair> vPairs;
    vector<size_t> vnIndexEdge;
    vector<uint8_t> vRemoved;
};

int Device()
{
    static const int device = getenv("ORBHIP_DEVICE") ? atoi(getenv("ORBHIP_DEVICE")) : 0;      // read once per process, like ORBmatcher.cc
    return device;
}

void Gather(KeyFrame* pKF1, KeyFrame* pKF2, const vector<MapPoint*> &vpMatches1, TaskProblem &P, orbhip_sim3_opt_problem &Q)
{
    const cv::Mat &K1 = pKF1->mK;
    const cv::Mat &K2 = pKF2->mK;
    const cv::Mat R1w = pKF1->GetRotation();
    const cv::Mat t1w = pKF1->GetTranslation();
    const cv::Mat R2w = pKF2->GetRotation();
    const cv::Mat t2w = pKF2->GetTranslation();

    Q.cam.fx1 = K1.at<float>(0,0); Q.cam.fy1 = K1.at<float>(1,1); Q.cam.cx1 = K1.at<float>(0,2); Q.cam.cy1 = K1.at<float>(1,2);
    Q.cam.fx2 = K2.at<float>(0,0); Q.cam.fy2 = K2.at<float>(1,1); Q.cam.cx2 = K2.at<float>(0,2); Q.cam.cy2 = K2.at<float>(1,2);

    const int N = vpMatches1.size();
    const vector<MapPoint*> vpMapPoints1 = pKF1->GetMapPointMatches();
    P.vPairs.reserve(N); P.vnIndexEdge.reserve(N);

    for(int i=0; i<N; i++)
    {
        if(!vpMatches1[i])
            continue;

        MapPoint* pMP1 = vpMapPoints1[i];
        MapPoint* pMP2 = vpMatches1[i];

        const int i2 = pMP2->GetIndexInKeyFrame(pKF2);

        if(!pMP1 || !pMP2)
            continue;
        if(pMP1->isBad() || pMP2->isBad() || i2<0)
            continue;

        cv::Mat P3D1w = pMP1->GetWorldPos();
        cv::Mat P3D1c = R1w*P3D1w + t1w;
        cv::Mat P3D2w = pMP2->GetWorldPos();
        cv::Mat P3D2c = R2w*P3D2w + t2w;

        const cv::KeyPoint &kpUn1 = pKF1->mvKeysUn[i];
        const cv::KeyPoint &kpUn2 = pKF2->mvKeysUn[i2];

        orbhip_sim3_pair p;
        p.u1 = kpUn1.pt.x; p.v1 = kpUn1.pt.y; p.inv_sigma2_1 = pKF1->mvInvLevelSigma2[kpUn1.octave];
        p.u2 = kpUn2.pt.x; p.v2 = kpUn2.pt.y; p.inv_sigma2_2 = pKF2->mvInvLevelSigma2[kpUn2.octave];
        for(int k=0; k<3; k++)
        {
            p.X1[k] = P3D1c.at<float>(k);
            p.X2[k] = P3D2c.at<float>(k);
        }
        P.vPairs.push_back(p);
        P.vnIndexEdge.push_back(i);
    }
    P.vRemoved.assign(P.vPairs.size(), 0);
    Q.n = (int)P.vPairs.size();
}

} // namespace

void OptimizeSim3DeviceTasks(KeyFrame* pKF1, vector<Sim3OptTask> &vTasks, float th2, bool bFixScale)
{
    vector<TaskProblem> vP(vTasks.size());
    vector<orbhip_sim3_opt_problem> vQ;
    vector<size_t> vnTask;
    for(size_t k=0; k<vTasks.size(); k++)
    {
        Sim3OptTask &T = vTasks[k];
        T.bWritten = false; T.nInliers = 0;
        if(!T.pKF2 || !T.pvpMatches1)
            continue;
        orbhip_sim3_opt_problem Q;
        memset(&Q, 0, sizeof Q);
        Gather(pKF1, T.pKF2, *T.pvpMatches1, vP[k], Q);
        memcpy(Q.S12_in, T.S12, sizeof Q.S12_in);
        memcpy(Q.S12_out, T.S12, sizeof Q.S12_out);
        Q.th2 = th2; Q.fix_scale = bFixScale ? 1 : 0;
        vQ.push_back(Q);
        vnTask.push_back(k);
    }
    for(size_t j=0; j<vQ.size(); j++)       // the pointers are set once every problem lies where it stays
    {
        TaskProblem &P = vP[vnTask[j]];
        vQ[j].pairs = P.vPairs.empty() ? NULL : &P.vPairs[0];
        vQ[j].removed = P.vRemoved.empty() ? NULL : &P.vRemoved[0];
    }
    if(vQ.empty())
        return;
    if(orbhip_sim3_optimize_batch(Device(), (int)vQ.size(), &vQ[0])!=ORBHIP_OK)
        throw ORBhipError(string("OptimizeSim3Device: ") + orbhip_last_error());
    for(size_t j=0; j<vQ.size(); j++)
    {
        Sim3OptTask &T = vTasks[vnTask[j]];
        const TaskProblem &P = vP[vnTask[j]];
        for(size_t e=0; e<P.vnIndexEdge.size(); e++)
            if(P.vRemoved[e])
                (*T.pvpMatches1)[P.vnIndexEdge[e]] = static_cast<MapPoint*>(NULL);
        T.nInliers = vQ[j].n_inliers;
        // The member writes g2oS12 after the second check only; on its early return S12_out is S12_in bit for bit (include/orbhip.h).  The caller's
        // S12 is touched only where the bits differ: never where the member leaves g2oS12 alone, and where it would store the same bits nothing is lost.
        T.bWritten = memcmp(vQ[j].S12_out, vQ[j].S12_in, sizeof vQ[j].S12_out)!=0;
        memcpy(T.S12, vQ[j].S12_out, sizeof T.S12);
    }
}

} // namespace ORB_SLAM2
