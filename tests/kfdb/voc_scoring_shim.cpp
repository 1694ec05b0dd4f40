// voc_scoring_shim.cpp — the ORBVocabulary members that tests/kfdb/kf_stub.cpp's C interface does not reach, for tests/test_kfdb_scoring_dropin_cpp.py:
// the scoring accessors, saveToTextFile, and a KeyFrameDatabase constructor whose exception comes back as a message.  Built beside kf_stub.cpp.
#include "KeyFrame.h"
#include "Frame.h"
#include "KeyFrameDatabase.h"
#include "ORBextractor.h"
#include <cstdio>
#include <cstring>

using namespace ORB_SLAM2;

extern "C" {
// -> 0, or 1 with what() in msg
int kfs_voc_set_scoring(void* voc, int scoring, char* msg, int cap)
{
    try { static_cast<ORBVocabulary*>(voc)->setScoringType((DBoW2::ScoringType)scoring); return 0; }
    catch (const ORBhipError& e) { snprintf(msg, (size_t)cap, "%s", e.what()); return 1; }
}
// {getScoringType, getWeightingType, getBranchingFactor, getDepthLevels}
void kfs_voc_get(void* voc, int* out)
{
    const ORBVocabulary* v = static_cast<const ORBVocabulary*>(voc);
    out[0] = (int)v->getScoringType(); out[1] = (int)v->getWeightingType(); out[2] = v->getBranchingFactor(); out[3] = v->getDepthLevels();
}
void kfs_voc_save(void* voc, const char* path) { static_cast<ORBVocabulary*>(voc)->saveToTextFile(path); }
void kfs_voc_free(void* voc) { delete static_cast<ORBVocabulary*>(voc); }
// new KeyFrameDatabase(voc), or NULL with what() in msg
void* kfs_db_try(void* voc, char* msg, int cap)
{
    try { return new KeyFrameDatabase(*static_cast<ORBVocabulary*>(voc)); }
    catch (const ORBhipError& e) { snprintf(msg, (size_t)cap, "%s", e.what()); return NULL; }
}
}
