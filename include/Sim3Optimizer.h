// Sim3Optimizer.h — Optimizer::OptimizeSim3 (Optimizer.cc:1046-1241) on the device (orbhip_sim3_optimize, include/orbhip.h).
// Same contract as the reference's member: reads pKF1->GetMapPointMatches(), mvKeysUn, mvInvLevelSigma2, mK and the poses of both key frames, the
// matched points' positions and their indices in pKF2; sets vpMatches1[i] = NULL for every pair either check removes; returns the number of inliers and
// writes S12 only where the member writes g2oS12 (not on its early `return 0`).  The reference's signature carries a g2o::Sim3&; this file does not
// include g2o, so the Sim3 type is a template parameter that needs the accessors g2o::Sim3 has: rotation().coeffs() (x, y, z, w), translation(), scale().
// To use it, forward the member:
//     int Optimizer::OptimizeSim3(KeyFrame *pKF1, KeyFrame *pKF2, std::vector<MapPoint *> &vpMatches1, g2o::Sim3 &g2oS12, const float th2, const bool bFixScale)
//     { return OptimizeSim3Device(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale); }
// A failed device call throws ORBhipError.
#ifndef SIM3OPTIMIZER_H
#define SIM3OPTIMIZER_H

#include <cstddef>
#include <vector>

namespace ORB_SLAM2
{

class KeyFrame;
class MapPoint;

// One candidate of a batch: S12 as qx qy qz qw tx ty tz s going in; coming out, the result and whether the member would have written g2oS12.
struct Sim3OptTask
{
    KeyFrame* pKF2;
    std::vector<MapPoint*>* pvpMatches1;
    double S12[8];
    bool bWritten;
    int nInliers;
};

// All tasks against pKF1 in one device call; element i is what a single call on task i gives, bit for bit.  Tasks with a NULL pKF2 or match vector are skipped (0).
void OptimizeSim3DeviceTasks(KeyFrame* pKF1, std::vector<Sim3OptTask> &vTasks, float th2, bool bFixScale);

template <class Sim3T>
void Sim3ToTask(const Sim3T &S12, Sim3OptTask &task)
{
    for(int i=0; i<4; i++) task.S12[i] = S12.rotation().coeffs()[i];
    for(int i=0; i<3; i++) task.S12[4+i] = S12.translation()[i];
    task.S12[7] = S12.scale();
}

template <class Sim3T>
void TaskToSim3(const Sim3OptTask &task, Sim3T &S12)
{
    if(!task.bWritten)
        return;
    for(int i=0; i<4; i++) S12.rotation().coeffs()[i] = task.S12[i];
    for(int i=0; i<3; i++) S12.translation()[i] = task.S12[4+i];
    S12.scale() = task.S12[7];
}

template <class Sim3T>
int OptimizeSim3Device(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*> &vpMatches1, Sim3T &S12, float th2, bool bFixScale)
{
    std::vector<Sim3OptTask> vTasks(1);
    vTasks[0].pKF2 = pKF2; vTasks[0].pvpMatches1 = &vpMatches1;
    Sim3ToTask(S12, vTasks[0]);
    OptimizeSim3DeviceTasks(pKF1, vTasks, th2, bFixScale);
    TaskToSim3(vTasks[0], S12);
    return vTasks[0].nInliers;
}

// One round of LoopClosing::ComputeSim3's candidates (after Sim3Solver::IterateBatch and SearchBySim3): element i of the result is what
// OptimizeSim3Device(pKF1, candidate i) returns, its matches and its S12 are updated in the same way.
template <class Sim3T>
struct Sim3OptCandidate
{
    KeyFrame* pKF2;
    std::vector<MapPoint*>* pvpMatches1;
    Sim3T* pS12;
};

template <class Sim3T>
std::vector<int> OptimizeSim3Device(KeyFrame* pKF1, const std::vector<Sim3OptCandidate<Sim3T> > &vCandidates, float th2, bool bFixScale)
{
    std::vector<Sim3OptTask> vTasks(vCandidates.size());
    for(size_t k=0; k<vCandidates.size(); k++)
    {
        vTasks[k].pKF2 = vCandidates[k].pS12 ? vCandidates[k].pKF2 : NULL;
        vTasks[k].pvpMatches1 = vCandidates[k].pvpMatches1;
        if(vCandidates[k].pS12)
            Sim3ToTask(*vCandidates[k].pS12, vTasks[k]);
    }
    OptimizeSim3DeviceTasks(pKF1, vTasks, th2, bFixScale);
    std::vector<int> vnInliers(vCandidates.size(), 0);
    for(size_t k=0; k<vCandidates.size(); k++)
    {
        if(vCandidates[k].pS12)
            TaskToSim3(vTasks[k], *vCandidates[k].pS12);
        vnInliers[k] = vTasks[k].nInliers;
    }
    return vnInliers;
}

} // namespace ORB_SLAM2

#endif // SIM3OPTIMIZER_H
