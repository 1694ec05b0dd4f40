// Test-owned stand-in for ORB_SLAM2's Frame.h (see KeyFrame.h beside it)
#ifndef FRAME_H
#define FRAME_H
#include "ORBVocabulary.h"
namespace ORB_SLAM2
{
class Frame
{
public:
    Frame();
    long unsigned int mnId;
    DBoW2::BowVector mBowVec;
};
}
#endif
