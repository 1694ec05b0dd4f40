// Test-owned stand-in for ORB_SLAM2's Frame.h: the members MapPoint's frame constructor and PredictScale read (see KeyFrame.h beside it).
#ifndef FRAME_H
#define FRAME_H
#include <vector>
#include <opencv2/core/core.hpp>
#include <opencv2/features2d/features2d.hpp>
namespace ORB_SLAM2
{
class MapPoint; class KeyFrame;
class Frame
{
public:
    Frame() : mnId(0), mnScaleLevels(1), mfLogScaleFactor(1.0f) {}
    cv::Mat GetCameraCenter() { return cv::Mat(cv::Mat::zeros(3, 1, CV_32F)); }
    long unsigned int mnId;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvScaleFactors;
    int mnScaleLevels; float mfLogScaleFactor;
    cv::Mat mDescriptors;
};
}
#endif
