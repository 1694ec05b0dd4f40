// Test-owned stand-in for ORB_SLAM2's Map.h: the lock MapPoint's constructors take and the call its SetBadFlag makes (see KeyFrame.h beside it).
#ifndef MAP_H
#define MAP_H
#include <mutex>
namespace ORB_SLAM2
{
class MapPoint;
class Map
{
public:
    void EraseMapPoint(MapPoint*) {}
    std::mutex mMutexPointCreation;
};
}
#endif
