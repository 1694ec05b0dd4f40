// kf_stub.cpp — the key frames of the KeyFrameDatabase tests, and a C interface that plays a script of database calls.
// Two builds:
//  * beside ORB_SLAM2's own src/KeyFrameDatabase.cc and headers (tests/golden/make_golden_kfdb.py): this file defines the few KeyFrame / Frame members that
//    translation unit needs - the constructors, GetConnectedKeyFrames and GetBestCovisibilityKeyFrames from lists that AddConnection fills, and the zero
//    initial value of the six query fields (KeyFrame.cc:35 leaves the two scores uninitialised);
//  * with -DKFDB_STUB_OWN_TYPES and tests/kfdb/stub/ on the include path (tests/test_kfdb_dropin_cpp.py): the same members for the stand-in classes there,
//    beside this repository's orb_slam2_amd/cpp/KeyFrameDatabase.cc.
#include "KeyFrame.h"
#include "Frame.h"
#include "KeyFrameDatabase.h"
#include <cstdint>
#include <cstring>

namespace ORB_SLAM2
{
long unsigned int KeyFrame::nNextId = 0;

#ifdef KFDB_STUB_OWN_TYPES
KeyFrame::KeyFrame(Frame &F, Map*, KeyFrameDatabase*) : mnId(nNextId++), mBowVec(F.mBowVec) {}
void KeyFrame::AddConnection(KeyFrame* pKF, const int &weight) { mspConnected.insert(pKF); if (weight > 0) mvpOrderedConnectedKeyFrames.push_back(pKF); }
std::set<KeyFrame*> KeyFrame::GetConnectedKeyFrames() { return mspConnected; }
#else
KeyFrame::KeyFrame(Frame &F, Map* pMap, KeyFrameDatabase* pKFDB) :
    mnFrameId(F.mnId), mTimeStamp(0), mnGridCols(0), mnGridRows(0), mfGridElementWidthInv(0), mfGridElementHeightInv(0),
    mnTrackReferenceForFrame(0), mnFuseTargetForKF(0), mnBALocalForKF(0), mnBAFixedForKF(0),
    mnLoopQuery(0), mnLoopWords(0), mLoopScore(0.0f), mnRelocQuery(0), mnRelocWords(0), mRelocScore(0.0f), mnBAGlobalForKF(0),
    fx(0), fy(0), cx(0), cy(0), invfx(0), invfy(0), mbf(0), mb(0), mThDepth(0), N(0), mBowVec(F.mBowVec),
    mnScaleLevels(0), mfScaleFactor(0), mfLogScaleFactor(0), mnMinX(0), mnMinY(0), mnMaxX(0), mnMaxY(0),
    mpKeyFrameDB(pKFDB), mpORBvocabulary(NULL), mbFirstConnection(true), mpParent(NULL), mbNotErase(false), mbToBeErased(false), mbBad(false), mHalfBaseline(0), mpMap(pMap)
{
    mnId = nNextId++;
}
void KeyFrame::AddConnection(KeyFrame* pKF, const int &weight) { mConnectedKeyFrameWeights[pKF] = weight; if (weight > 0) mvpOrderedConnectedKeyFrames.push_back(pKF); }
std::set<KeyFrame*> KeyFrame::GetConnectedKeyFrames()
{
    std::set<KeyFrame*> s;
    for (std::map<KeyFrame*, int>::iterator it = mConnectedKeyFrameWeights.begin(); it != mConnectedKeyFrameWeights.end(); ++it) s.insert(it->first);
    return s;
}
#endif
std::vector<KeyFrame*> KeyFrame::GetBestCovisibilityKeyFrames(const int &N)
{
    if ((int)mvpOrderedConnectedKeyFrames.size() < N) return mvpOrderedConnectedKeyFrames;
    return std::vector<KeyFrame*>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + N);
}
Frame::Frame() {}
}

using namespace ORB_SLAM2;

static void fill(DBoW2::BowVector& v, const uint32_t* id, const double* val, int n)
{
    v.clear();
    for (int i = 0; i < n; i++) v.insert(v.end(), std::make_pair(id[i], val[i]));
}
static int deliver(const std::vector<KeyFrame*>& r, void** out, int cap)
{
    for (int i = 0; i < (int)r.size() && i < cap; i++) out[i] = r[i];
    return (int)r.size();
}

extern "C" {
void* kfs_voc(const char* path) { ORBVocabulary* v = new ORBVocabulary(); if (!v->loadFromTextFile(path)) { delete v; return NULL; } return v; }
void* kfs_db(void* voc) { return new KeyFrameDatabase(*static_cast<ORBVocabulary*>(voc)); }
void kfs_db_free(void* db) { delete static_cast<KeyFrameDatabase*>(db); }
void* kfs_kf(uint64_t id, const uint32_t* bid, const double* bval, int n)
{
    Frame F; F.mnId = id; fill(F.mBowVec, bid, bval, n);
    KeyFrame* kf = new KeyFrame(F, NULL, NULL);
    kf->mnId = id;
    return kf;
}
void kfs_connect(void* kf, void* other, int weight) { static_cast<KeyFrame*>(kf)->AddConnection(static_cast<KeyFrame*>(other), weight); }
void kfs_add(void* db, void* kf) { static_cast<KeyFrameDatabase*>(db)->add(static_cast<KeyFrame*>(kf)); }
void kfs_erase(void* db, void* kf) { static_cast<KeyFrameDatabase*>(db)->erase(static_cast<KeyFrame*>(kf)); }
void kfs_clear(void* db) { static_cast<KeyFrameDatabase*>(db)->clear(); }
int kfs_loop(void* db, void* kf, float min_score, void** out, int cap) { return deliver(static_cast<KeyFrameDatabase*>(db)->DetectLoopCandidates(static_cast<KeyFrame*>(kf), min_score), out, cap); }
int kfs_reloc(void* db, uint64_t id, const uint32_t* bid, const double* bval, int n, void** out, int cap)
{
    Frame F; F.mnId = id; fill(F.mBowVec, bid, bval, n);
    return deliver(static_cast<KeyFrameDatabase*>(db)->DetectRelocalizationCandidates(&F), out, cap);
}
#ifndef KFDB_STUB_OWN_TYPES
// {mnRelocQuery, mnLoopQuery}, {mnRelocWords, mnLoopWords}, {mRelocScore, mLoopScore}
void kfs_fields(void* kf, uint64_t* query, int32_t* words, float* score)
{
    KeyFrame* k = static_cast<KeyFrame*>(kf);
    query[0] = k->mnRelocQuery; query[1] = k->mnLoopQuery; words[0] = k->mnRelocWords; words[1] = k->mnLoopWords; score[0] = k->mRelocScore; score[1] = k->mLoopScore;
}
#endif
}
