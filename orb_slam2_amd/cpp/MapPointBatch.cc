// MapPointBatch.cc — MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:242-307) for a whole list of map points as ONE device call
// (orbhip_distinctive_descriptors, include/orbhip.h).  Declared in include/ORBmatcherBatch.h; integration/apply_dropin.py installs this file as
// src/MapPointBatch.cc beside src/ORBmatcher.cc (add it to the library's sources in CMakeLists.txt); INTEGRATION.md section 2-3k shows the two LocalMapping
// loops that call it.  A translation unit of its own: it needs MapPoint, KeyFrame and the one friend line in include/MapPoint.h, nothing else of the tree.
//
// Per point it does what the member does, in the member's order: under mMutexFeatures it leaves a bad point alone and copies mObservations; it walks the copy
// in the map's own order - std::map<KeyFrame*,size_t>: by key-frame address, as the member's iterator does - and gathers row mit->second of every key frame
// that is not bad; a point with nothing gathered is left alone.  The device picks the row with the least median distance (first among equals: the order just
// walked, so ties break as the member breaks them in this process); the chosen row is cloned into mDescriptor under mMutexFeatures.
#include "ORBmatcher.h"
#include "ORBmatcherBatch.h"
#include "ORBextractor.h"   // ORBhipError
#include "orbhip.h"

#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#ifndef ORBHIP_MAPPOINT_FRIEND
#error "include/MapPoint.h needs `friend class ORBmatcher;` (integration/apply_dropin.py adds it and defines ORBHIP_MAPPOINT_FRIEND): the batch reads mObservations and writes mDescriptor in place"
#endif

using namespace std;

namespace ORB_SLAM2
{

// the nested type the friend line in include/MapPoint.h reaches (like ORBmatcher::Access in ORBmatcher.cc)
struct ORBmatcher::DistinctAccess
{
    // MapPoint.cc:249-254: false = the member returns here (bad point)
    static inline bool Observations(MapPoint* pMP, map<KeyFrame*,size_t> &observations)
    {
        unique_lock<mutex> lock1(pMP->mMutexFeatures);
        if(pMP->mbBad) return false;
        observations = pMP->mObservations;
        return true;
    }
    // MapPoint.cc:303-306
    static inline void SetDescriptor(MapPoint* pMP, const cv::Mat &row)
    {
        unique_lock<mutex> lock(pMP->mMutexFeatures);
        pMP->mDescriptor = row.clone();
    }
};

void ComputeDistinctiveDescriptorsBatch(const vector<MapPoint*> &vpMapPoints)
{
    static const int device = getenv("ORBHIP_DEVICE") ? atoi(getenv("ORBHIP_DEVICE")) : 0;      // read once per process, like ORBmatcher.cc
    vector<MapPoint*> vpLive;               // the points the member would reach its distance table with
    vector<cv::Mat> vDescriptors;           // their observed rows, group after group (headers that share the key frames' data, as in the member)
    vector<int32_t> vOffsets(1, 0);
    vector<unsigned char> vBytes;
    map<KeyFrame*,size_t> observations;
    for(size_t i=0; i<vpMapPoints.size(); i++)
    {
        MapPoint* pMP = vpMapPoints[i];
        if(!pMP) continue;
        if(!ORBmatcher::DistinctAccess::Observations(pMP, observations)) continue;
        if(observations.empty()) continue;
        const size_t nBefore = vDescriptors.size();
        for(map<KeyFrame*,size_t>::iterator mit=observations.begin(), mend=observations.end(); mit!=mend; mit++)
        {
            KeyFrame* pKF = mit->first;
            if(!pKF->isBad())
                vDescriptors.push_back(pKF->mDescriptors.row(mit->second));
        }
        if(vDescriptors.size()==nBefore) continue;
        vpLive.push_back(pMP);
        vOffsets.push_back((int32_t)vDescriptors.size());
    }
    if(vpLive.empty()) return;
    vBytes.resize(vDescriptors.size()*32);
    for(size_t d=0; d<vDescriptors.size(); d++) memcpy(&vBytes[32*d], vDescriptors[d].ptr<unsigned char>(), 32);
    vector<int32_t> vBest(vpLive.size(), 0);
    if(orbhip_distinctive_descriptors(device, &vBytes[0], &vOffsets[0], (int)vpLive.size(), &vBest[0], NULL)!=ORBHIP_OK)
        throw ORBhipError(string("ComputeDistinctiveDescriptorsBatch: ") + orbhip_last_error());
    for(size_t p=0; p<vpLive.size(); p++)
        ORBmatcher::DistinctAccess::SetDescriptor(vpLive[p], vDescriptors[vOffsets[p]+vBest[p]]);
}

} // namespace ORB_SLAM2
