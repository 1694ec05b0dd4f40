// Test-owned stand-in for ORB_SLAM2's MapPoint.h: a position and a bad flag.
#ifndef MAPPOINT_H
#define MAPPOINT_H
#include <opencv2/core/core.hpp>
namespace ORB_SLAM2
{
class MapPoint
{
public:
    MapPoint(float x, float y, float z) : mWorldPos(3, 1, CV_32F), mbBad(false)
    { mWorldPos.at<float>(0) = x; mWorldPos.at<float>(1) = y; mWorldPos.at<float>(2) = z; }
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    bool isBad() { return mbBad; }
    cv::Mat mWorldPos;
    bool mbBad;
};
}
#endif
