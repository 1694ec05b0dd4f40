// KeyFrameDatabase.h — ORB_SLAM2::KeyFrameDatabase on liborbhip.so: the reference's public signatures (include/KeyFrameDatabase.h:45-60 there) over
// the device key-frame database of include/orbhip.h (orbhip_kfdb_*).  The key frames' BowVectors live in device memory, one slot per key frame; this
// class keeps the slot <-> KeyFrame* mapping.  The per-key-frame query fields (mnLoopQuery, mnLoopWords, mLoopScore, mnRelocQuery, mnRelocWords,
// mRelocScore), which no file of ORB_SLAM2 outside KeyFrameDatabase.cc reads, live in the database and not in the KeyFrame.
// Scores are those of the vocabulary's own scoring object (ORBVocabulary::getScoringType, read at the constructor and at every Detect as the reference
// calls mpVoc->score there): L1_NORM, L2_NORM, CHI_SQUARE, BHATTACHARYYA or DOT_PRODUCT.  A KL vocabulary throws ORBhipError.
#ifndef KEYFRAMEDATABASE_H
#define KEYFRAMEDATABASE_H

#include <vector>
#include <list>
#include <set>
#include <map>
#include <mutex>

#include "KeyFrame.h"
#include "Frame.h"
#include "ORBVocabulary.h"

struct orbhip_kfdb;

namespace ORB_SLAM2
{

class KeyFrame;
class Frame;

class KeyFrameDatabase
{
public:

    KeyFrameDatabase(const ORBVocabulary &voc);
    ~KeyFrameDatabase();

    void add(KeyFrame* pKF);

    void erase(KeyFrame* pKF);

    void clear();

    // Loop Detection
    std::vector<KeyFrame *> DetectLoopCandidates(KeyFrame* pKF, float minScore);

    // Relocalization
    std::vector<KeyFrame*> DetectRelocalizationCandidates(Frame* F);

    // Relocalization of a batch of frames: ONE device call for the queries (orbhip_kfdb_query_batch), the hits' best covisibles, ONE for the
    // selections.  Result [i] is what DetectRelocalizationCandidates(vpF[i]) returns when the frames are asked one after another in this order.
    std::vector<std::vector<KeyFrame*> > DetectRelocalizationCandidates(const std::vector<Frame*> &vpF);

protected:

    // one device query (kind: ORBHIP_KFDB_RELOC / ORBHIP_KFDB_LOOP), the hits' best covisibles, the covisibility selection
    std::vector<KeyFrame*> Detect(int kind, unsigned long long qid, const DBoW2::BowVector &bow, const std::set<KeyFrame*> &sConnected, float minScore);

    // makes the device database score as mpVoc does now; calls the device only when that changed
    void FollowVocabularyScoring();

    // Associated vocabulary
    const ORBVocabulary* mpVoc;

    // The device database; which key frame each of its slots holds
    orbhip_kfdb* mpDb;
    int mnScoring;                       // what mpDb scores with (under mMutex)
    std::map<KeyFrame*, int> mSlotOf;
    std::vector<KeyFrame*> mvpKeyFrameOf;

    // Mutex (the slot mapping; the device database has its own lock)
    std::mutex mMutex;

    // Held over a device query; the batched form holds it until its selections are done, since any later query supersedes a batch's snapshot
    std::mutex mMutexQuery;

private:
    KeyFrameDatabase(const KeyFrameDatabase&);
    KeyFrameDatabase& operator=(const KeyFrameDatabase&);
};

} //namespace ORB_SLAM

#endif
