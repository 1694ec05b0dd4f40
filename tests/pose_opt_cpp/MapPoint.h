// Test-owned stand-in for ORB_SLAM2's MapPoint.h: a position behind mMutexPos and the global mutex the optimiser's set-up loop holds.
#ifndef MAPPOINT_H
#define MAPPOINT_H
#include <mutex>
#include <opencv2/core/core.hpp>
namespace ORB_SLAM2
{
class MapPoint
{
public:
    MapPoint(float x, float y, float z) : mWorldPos(3, 1, CV_32F), nReads(0) { mWorldPos.at<float>(0) = x; mWorldPos.at<float>(1) = y; mWorldPos.at<float>(2) = z; }
    cv::Mat GetWorldPos() { std::unique_lock<std::mutex> lock(mMutexPos); nReads++; return mWorldPos.clone(); }
    static std::mutex mGlobalMutex;
    int nReads;            // (test only) positions were taken through GetWorldPos()
protected:
    cv::Mat mWorldPos;
    std::mutex mMutexPos;
};
}
#endif
