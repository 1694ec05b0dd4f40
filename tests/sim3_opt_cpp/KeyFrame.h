// Test-owned stand-in for ORB_SLAM2's KeyFrame.h: the members OptimizeSim3Device reads (orb_slam2_amd/cpp/Sim3Optimizer.cc).
#ifndef KEYFRAME_H
#define KEYFRAME_H
#include <vector>
#include <opencv2/core/core.hpp>
#include <opencv2/features2d/features2d.hpp>
namespace ORB_SLAM2
{
class MapPoint;
class KeyFrame
{
public:
    KeyFrame() : mK(3, 3, CV_32F), mRcw(3, 3, CV_32F), mtcw(3, 1, CV_32F) {}
    std::vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
    cv::Mat GetRotation() { return mRcw.clone(); }
    cv::Mat GetTranslation() { return mtcw.clone(); }
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvInvLevelSigma2;
    cv::Mat mK;
    std::vector<MapPoint*> mvpMapPoints;
    cv::Mat mRcw, mtcw;
};
}
#endif
