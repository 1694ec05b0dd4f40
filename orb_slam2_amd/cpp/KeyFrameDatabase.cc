// KeyFrameDatabase.cc — ORB_SLAM2::KeyFrameDatabase on liborbhip.so (see include/KeyFrameDatabase.h).  The reference's inverted file and its walks are
// replaced by the device key-frame database of include/orbhip.h: both queries are gather -> ONE device call (orbhip_kfdb_query: the shared-word scan,
// the scores, the hit list in the reference's order) -> GetBestCovisibilityKeyFrames(10) per hit -> orbhip_kfdb_select (the covisibility accumulation).
// The vector overload of DetectRelocalizationCandidates does the same for a batch of frames with orbhip_kfdb_query_batch / _select_batch.
#include "KeyFrameDatabase.h"
#include "ORBextractor.h"
#include "orbhip.h"
#include <string>

namespace ORB_SLAM2
{

static void orbhip_check(orbhip_status st, const char* what)
{
    if (st != ORBHIP_OK) throw ORBhipError(std::string("KeyFrameDatabase::") + what + ": " + orbhip_last_error());
}

static void FlattenBow(const DBoW2::BowVector &bow, std::vector<uint32_t> &id, std::vector<double> &val)
{
    id.clear(); val.clear(); id.reserve(bow.size()); val.reserve(bow.size());
    for (DBoW2::BowVector::const_iterator it = bow.begin(); it != bow.end(); ++it) { id.push_back(it->first); val.push_back(it->second); }
}

// A database is created scoring L1_NORM (0, what ORBvoc.txt declares) and follows the vocabulary's scoring object from there
KeyFrameDatabase::KeyFrameDatabase(const ORBVocabulary &voc) : mpVoc(&voc), mpDb(NULL), mnScoring(0)
{
    int device = 0;
    if (const char* dev = getenv("ORBHIP_DEVICE")) device = atoi(dev);
    orbhip_check(orbhip_kfdb_create(&mpDb, device, (int)voc.size(), 0), "KeyFrameDatabase");
    try { FollowVocabularyScoring(); }
    catch (...) { orbhip_kfdb_destroy(mpDb); mpDb = NULL; throw; }      // (a KL vocabulary: the destructor of a half-built object does not run)
}

void KeyFrameDatabase::FollowVocabularyScoring()
{
    static const char* const names[] = {"L1_NORM", "L2_NORM", "CHI_SQUARE", "KL", "BHATTACHARYYA", "DOT_PRODUCT"};
    const int scoring = (int)mpVoc->getScoringType();
    std::unique_lock<std::mutex> lock(mMutex);
    if (scoring == mnScoring) return;
    const orbhip_status st = orbhip_kfdb_set_scoring(mpDb, scoring);
    if (st != ORBHIP_OK)
        throw ORBhipError(std::string("KeyFrameDatabase: the vocabulary's scoring ") + (scoring >= 0 && scoring <= 5 ? names[scoring] : "?") + ": " + orbhip_last_error());
    mnScoring = scoring;
}

KeyFrameDatabase::~KeyFrameDatabase() { if (mpDb) orbhip_kfdb_destroy(mpDb); }

void KeyFrameDatabase::add(KeyFrame *pKF)
{
    std::vector<uint32_t> id; std::vector<double> val;
    FlattenBow(pKF->mBowVec, id, val);
    std::unique_lock<std::mutex> lock(mMutex);
    int slot = -1;
    orbhip_check(orbhip_kfdb_add(mpDb, id.empty() ? NULL : &id[0], val.empty() ? NULL : &val[0], (int)id.size(), &slot), "add");
    if ((size_t)slot >= mvpKeyFrameOf.size()) mvpKeyFrameOf.resize((size_t)slot + 1, static_cast<KeyFrame*>(NULL));
    mvpKeyFrameOf[slot] = pKF;
    mSlotOf[pKF] = slot;
}

void KeyFrameDatabase::erase(KeyFrame* pKF)
{
    std::unique_lock<std::mutex> lock(mMutex);
    std::map<KeyFrame*, int>::iterator it = mSlotOf.find(pKF);
    if (it == mSlotOf.end()) return;                                  // (the reference's erase of an unknown key frame finds nothing in any list)
    orbhip_check(orbhip_kfdb_erase(mpDb, it->second), "erase");
    mvpKeyFrameOf[it->second] = NULL;
    mSlotOf.erase(it);
}

void KeyFrameDatabase::clear()
{
    std::unique_lock<std::mutex> lock(mMutex);
    orbhip_check(orbhip_kfdb_clear(mpDb), "clear");
    mSlotOf.clear(); mvpKeyFrameOf.clear();
}

std::vector<KeyFrame*> KeyFrameDatabase::Detect(int kind, unsigned long long qid, const DBoW2::BowVector &bow, const std::set<KeyFrame*> &sConnected, float minScore)
{
    FollowVocabularyScoring();
    std::vector<uint32_t> id; std::vector<double> val;
    FlattenBow(bow, id, val);
    std::vector<int32_t> vExcluded; int nCap = 0;
    {
        std::unique_lock<std::mutex> lock(mMutex);
        for (std::set<KeyFrame*>::const_iterator sit = sConnected.begin(); sit != sConnected.end(); ++sit) {
            std::map<KeyFrame*, int>::const_iterator it = mSlotOf.find(*sit);
            if (it != mSlotOf.end()) vExcluded.push_back(it->second);
        }
        nCap = (int)mSlotOf.size();
    }
    std::vector<orbhip_kfdb_hit> vHits((size_t)nCap + 1);
    int nHits = 0, nSharing = 0, nMinCommon = 0;
    std::unique_lock<std::mutex> lockQuery(mMutexQuery);
    orbhip_status st = orbhip_kfdb_query(mpDb, kind, qid, id.empty() ? NULL : &id[0], val.empty() ? NULL : &val[0], (int)id.size(),
                                         vExcluded.empty() ? NULL : &vExcluded[0], (int)vExcluded.size(), minScore, &vHits[0], (int)vHits.size(), &nHits, &nSharing, &nMinCommon);
    lockQuery.unlock();
    if (st == ORBHIP_ERR_CAPACITY) nHits = (int)vHits.size();       // key frames were added since the count was taken: the first ones in the reference's order are kept
    else orbhip_check(st, "query");
    if (nHits == 0) return std::vector<KeyFrame*>();

    // the hits' key frames (under the mapping's lock), then their best covisibles (under the key frames' own mutexes), then the neighbours' slots
    std::vector<KeyFrame*> vpHit((size_t)nHits, static_cast<KeyFrame*>(NULL));
    {
        std::unique_lock<std::mutex> lock(mMutex);
        for (int i = 0; i < nHits; i++) if ((size_t)vHits[i].slot < mvpKeyFrameOf.size()) vpHit[i] = mvpKeyFrameOf[vHits[i].slot];
    }
    std::vector<std::vector<KeyFrame*> > vvpNeighs((size_t)nHits);
    for (int i = 0; i < nHits; i++) if (vpHit[i]) vvpNeighs[i] = vpHit[i]->GetBestCovisibilityKeyFrames(10);
    std::vector<int32_t> vOff((size_t)nHits + 1, 0), vNeighSlot;
    std::vector<KeyFrame*> vpOut;
    {
        std::unique_lock<std::mutex> lock(mMutex);
        for (int i = 0; i < nHits; i++) {
            for (size_t j = 0; j < vvpNeighs[i].size(); j++) {
                std::map<KeyFrame*, int>::const_iterator it = mSlotOf.find(vvpNeighs[i][j]);
                vNeighSlot.push_back(it != mSlotOf.end() ? it->second : -1);
            }
            vOff[i + 1] = (int32_t)vNeighSlot.size();
        }
    }
    std::vector<int32_t> vOutSlot((size_t)nHits + 1);
    int nOut = 0;
    orbhip_check(orbhip_kfdb_select(mpDb, kind, qid, nMinCommon, minScore, &vHits[0], nHits, &vOff[0], vNeighSlot.empty() ? NULL : &vNeighSlot[0],
                                    &vOutSlot[0], (int)vOutSlot.size(), &nOut), "select");
    {
        std::unique_lock<std::mutex> lock(mMutex);
        vpOut.reserve((size_t)nOut);
        for (int i = 0; i < nOut; i++) if ((size_t)vOutSlot[i] < mvpKeyFrameOf.size() && mvpKeyFrameOf[vOutSlot[i]]) vpOut.push_back(mvpKeyFrameOf[vOutSlot[i]]);
    }
    return vpOut;
}

std::vector<KeyFrame*> KeyFrameDatabase::DetectLoopCandidates(KeyFrame* pKF, float minScore)
{
    return Detect(ORBHIP_KFDB_LOOP, pKF->mnId, pKF->mBowVec, pKF->GetConnectedKeyFrames(), minScore);
}

std::vector<KeyFrame*> KeyFrameDatabase::DetectRelocalizationCandidates(Frame *F)
{
    return Detect(ORBHIP_KFDB_RELOC, F->mnId, F->mBowVec, std::set<KeyFrame*>(), 0.0f);
}

std::vector<std::vector<KeyFrame*> > KeyFrameDatabase::DetectRelocalizationCandidates(const std::vector<Frame*> &vpF)
{
    const int nQ = (int)vpF.size();
    std::vector<std::vector<KeyFrame*> > vvpOut((size_t)nQ);
    if (nQ == 0) return vvpOut;
    FollowVocabularyScoring();
    std::vector<uint64_t> vQid((size_t)nQ);
    std::vector<int32_t> vBowOff((size_t)nQ + 1, 0);
    std::vector<uint32_t> id, vId; std::vector<double> val, vVal;
    for (int i = 0; i < nQ; i++) {
        vQid[i] = vpF[i]->mnId;
        FlattenBow(vpF[i]->mBowVec, id, val);
        vId.insert(vId.end(), id.begin(), id.end()); vVal.insert(vVal.end(), val.begin(), val.end());
        vBowOff[i + 1] = (int32_t)vId.size();
    }
    std::vector<int32_t> vHitOff((size_t)nQ + 1, 0);
    uint64_t nToken = 0;
    std::unique_lock<std::mutex> lockQuery(mMutexQuery);            // until the selections: a later query would supersede the snapshot
    orbhip_check(orbhip_kfdb_query_batch(mpDb, ORBHIP_KFDB_RELOC, nQ, &vQid[0], &vBowOff[0], vId.empty() ? NULL : &vId[0], vVal.empty() ? NULL : &vVal[0], NULL, NULL, NULL,
                                         &vHitOff[0], NULL, NULL, NULL, 0, &nToken), "query_batch");
    const int nHits = vHitOff[nQ];
    if (nHits == 0) return vvpOut;
    std::vector<orbhip_kfdb_hit> vHits((size_t)nHits);
    orbhip_check(orbhip_kfdb_batch_hits(mpDb, nToken, 0, nQ, &vHits[0], nHits), "batch_hits");

    // as the single member: the hits' key frames, their best covisibles (under the key frames' own mutexes), the neighbours' slots
    std::vector<KeyFrame*> vpHit((size_t)nHits, static_cast<KeyFrame*>(NULL));
    {
        std::unique_lock<std::mutex> lock(mMutex);
        for (int i = 0; i < nHits; i++) if ((size_t)vHits[i].slot < mvpKeyFrameOf.size()) vpHit[i] = mvpKeyFrameOf[vHits[i].slot];
    }
    std::vector<std::vector<KeyFrame*> > vvpNeighs((size_t)nHits);
    for (int i = 0; i < nHits; i++) if (vpHit[i]) vvpNeighs[i] = vpHit[i]->GetBestCovisibilityKeyFrames(10);
    std::vector<int32_t> vOff((size_t)nHits + 1, 0), vNeighSlot;
    {
        std::unique_lock<std::mutex> lock(mMutex);
        for (int i = 0; i < nHits; i++) {
            for (size_t j = 0; j < vvpNeighs[i].size(); j++) {
                std::map<KeyFrame*, int>::const_iterator it = mSlotOf.find(vvpNeighs[i][j]);
                vNeighSlot.push_back(it != mSlotOf.end() ? it->second : -1);
            }
            vOff[i + 1] = (int32_t)vNeighSlot.size();
        }
    }
    std::vector<int32_t> vOutSlot((size_t)nHits + 1), vOutOff((size_t)nQ + 1, 0);
    orbhip_check(orbhip_kfdb_select_batch(mpDb, nToken, ORBHIP_KFDB_RELOC, &vHits[0], &vHitOff[0], &vOff[0], vNeighSlot.empty() ? NULL : &vNeighSlot[0],
                                          &vOutSlot[0], &vOutOff[0], (int)vOutSlot.size()), "select_batch");
    lockQuery.unlock();
    std::unique_lock<std::mutex> lock(mMutex);
    for (int q = 0; q < nQ; q++)
        for (int i = vOutOff[q]; i < vOutOff[q + 1]; i++)
            if ((size_t)vOutSlot[i] < mvpKeyFrameOf.size() && mvpKeyFrameOf[vOutSlot[i]]) vvpOut[q].push_back(mvpKeyFrameOf[vOutSlot[i]]);
    return vvpOut;
}

} //namespace ORB_SLAM
