// kf_batch_stub.cpp — the driver of the batched relocalisation query of this repository's KeyFrameDatabase (the vector overload of
// DetectRelocalizationCandidates); compiled beside kf_stub.cpp, which defines the key frames and the rest of the C interface.
#include "KeyFrame.h"
#include "Frame.h"
#include "KeyFrameDatabase.h"
#include <cstdint>
#include <vector>

using namespace ORB_SLAM2;

extern "C" {
// query i: id qid[i], BowVector (bid, bval)[bow_off[i] .. bow_off[i+1]); its candidates are out[out_off[i] .. out_off[i+1]) where they fit into cap
int kfs_reloc_batch(void* db, int nq, const uint64_t* qid, const int32_t* bow_off, const uint32_t* bid, const double* bval, void** out, int32_t* out_off, int cap)
{
    std::vector<Frame> frames((size_t)nq);
    std::vector<Frame*> vpF((size_t)nq);
    for (int i = 0; i < nq; i++) {
        frames[i].mnId = qid[i];
        for (int j = bow_off[i]; j < bow_off[i + 1]; j++) frames[i].mBowVec.insert(frames[i].mBowVec.end(), std::make_pair(bid[j], bval[j]));
        vpF[i] = &frames[i];
    }
    const std::vector<std::vector<KeyFrame*> > r = static_cast<KeyFrameDatabase*>(db)->DetectRelocalizationCandidates(vpF);
    int n = 0;
    out_off[0] = 0;
    for (int i = 0; i < nq; i++) {
        for (size_t j = 0; j < r[i].size(); j++, n++) if (n < cap) out[n] = r[i][j];
        out_off[i + 1] = n;
    }
    return (int)r.size();
}
}
