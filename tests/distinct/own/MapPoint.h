// Test-owned stand-in for ORB_SLAM2's MapPoint.h, for the builds that have no reference checkout (tests/test_distinctive_dropin_cpp.py with
// -DDISTINCT_STUB_OWN_MAPPOINT): the fields orb_slam2_amd/cpp/MapPointBatch.cc reaches, the friend line integration/apply_dropin.py adds to the real header,
// and the few members tests/distinct/mp_stub.cpp builds a point with.  It has no ComputeDistinctiveDescriptors: only the batch form runs against it.
#ifndef MAPPOINT_H
#define MAPPOINT_H
#define ORBHIP_MAPPOINT_FRIEND 1
#include "KeyFrame.h"
#include "Frame.h"
#include "Map.h"
#include <map>
#include <mutex>
#include <opencv2/core/core.hpp>
namespace ORB_SLAM2
{
class MapPoint
{
    friend class ORBmatcher;
public:
    MapPoint(const cv::Mat &, Map*, Frame* pFrame, const int &idxF) : mbBad(false) { pFrame->mDescriptors.row(idxF).copyTo(mDescriptor); }
    void AddObservation(KeyFrame* pKF, size_t idx) { std::unique_lock<std::mutex> lock(mMutexFeatures); if(!mObservations.count(pKF)) mObservations[pKF] = idx; }
    void SetBadFlag() { std::unique_lock<std::mutex> lock(mMutexFeatures); mbBad = true; mObservations.clear(); }
    cv::Mat GetDescriptor() { std::unique_lock<std::mutex> lock(mMutexFeatures); return mDescriptor.clone(); }
protected:
    std::map<KeyFrame*,size_t> mObservations;
    cv::Mat mDescriptor;
    bool mbBad;
    std::mutex mMutexFeatures;
};
}
#endif
