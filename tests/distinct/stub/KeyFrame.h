// Test-owned stand-in for ORB_SLAM2's KeyFrame.h: what src/MapPoint.cc and orb_slam2_amd/cpp/MapPointBatch.cc need of a key frame, nothing else
// (tests/golden/make_golden_distinct.py, tests/test_distinctive_dropin_cpp.py; the C interface that drives them: tests/distinct/mp_stub.cpp).
#ifndef KEYFRAME_H
#define KEYFRAME_H
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <map>
#include <mutex>
#include <vector>
#include <opencv2/core/core.hpp>
#include <opencv2/features2d/features2d.hpp>
using namespace std;      // the reference's own headers bring std into scope, and its src/MapPoint.cc relies on it (unique_lock<mutex>, vector, map)
namespace ORB_SLAM2
{
class MapPoint; class Map; class Frame;
class KeyFrame
{
public:
    KeyFrame() : mnId(0), mnFrameId(0), mnScaleLevels(1), mfLogScaleFactor(1.0f), mbBad(false) {}
    bool isBad() { return mbBad; }
    void EraseMapPointMatch(const size_t &) {}
    void ReplaceMapPointMatch(const size_t &, MapPoint*) {}
    cv::Mat GetCameraCenter() { return cv::Mat(cv::Mat::zeros(3, 1, CV_32F)); }
    long unsigned int mnId, mnFrameId;
    std::vector<float> mvuRight;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvScaleFactors;
    int mnScaleLevels; float mfLogScaleFactor;
    cv::Mat mDescriptors;
    bool mbBad;
};
}
#endif
