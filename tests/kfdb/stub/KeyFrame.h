// Test-owned stand-in for ORB_SLAM2's KeyFrame.h: what orb_slam2_amd/cpp/KeyFrameDatabase.cc needs of a key frame, nothing else
// (tests/test_kfdb_dropin_cpp.py; members defined in tests/kfdb/kf_stub.cpp).
#ifndef KEYFRAME_H
#define KEYFRAME_H
#include <set>
#include <vector>
#include "ORBVocabulary.h"
namespace ORB_SLAM2
{
class Frame; class Map; class KeyFrameDatabase;
class KeyFrame
{
public:
    KeyFrame(Frame &F, Map* pMap, KeyFrameDatabase* pKFDB);
    void AddConnection(KeyFrame* pKF, const int &weight);
    std::set<KeyFrame*> GetConnectedKeyFrames();
    std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int &N);
    static long unsigned int nNextId;
    long unsigned int mnId;
    DBoW2::BowVector mBowVec;
protected:
    std::set<KeyFrame*> mspConnected;
    std::vector<KeyFrame*> mvpOrderedConnectedKeyFrames;
};
}
#endif
