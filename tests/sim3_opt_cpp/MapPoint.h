// Test-owned stand-in for ORB_SLAM2's MapPoint.h: a position, a bad flag and the index of the point in the one key frame that observes it.
#ifndef MAPPOINT_H
#define MAPPOINT_H
#include <opencv2/core/core.hpp>
namespace ORB_SLAM2
{
class KeyFrame;
class MapPoint
{
public:
    MapPoint(float x, float y, float z, KeyFrame* pKF, int idx) : mWorldPos(3, 1, CV_32F), mbBad(false), mpKF(pKF), mnIdx(idx)
    { mWorldPos.at<float>(0) = x; mWorldPos.at<float>(1) = y; mWorldPos.at<float>(2) = z; }
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    bool isBad() { return mbBad; }
    int GetIndexInKeyFrame(KeyFrame* pKF) { return pKF == mpKF ? mnIdx : -1; }
    cv::Mat mWorldPos;
    bool mbBad;
    KeyFrame* mpKF;
    int mnIdx;
};
}
#endif
