// ref_train.cpp — the reference's own TemplatedVocabulary::create behind a C interface, for tests/voc_train_harness.py.  Compiled together with the reference's
// DBoW2 sources where they lie (never into this repository); nothing of the reference is changed.
//
// The reference draws its k-means++ centres from rand() in depth-first order, seeded from the clock: not a function of its input.  initiateClusters is
// virtual (TemplatedVocabulary.h:380), so the subclass below reseeds the stream for every node from the node's own key and then calls the
// reference's initiateClustersKMpp.  DUtils::Random::SeedRandOnce(0) before create(): otherwise the first initiateClustersKMpp (:847) would reseed from the
// clock after the override's seed.
#include <chrono>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include "DBoW2/FORB.h"
#include "DBoW2/TemplatedVocabulary.h"
#include "DUtils/Random.h"

typedef DBoW2::TemplatedVocabulary<DBoW2::FORB::TDescriptor, DBoW2::FORB> Base;

struct TrainVoc : Base {
    uint32_t base = 0;
    std::map<const cv::Mat*, uint32_t> flat;                                  // a training feature -> its index in training order
    void initiateClusters(const std::vector<pDescriptor>& d, std::vector<cv::Mat>& clusters) const override
    {
        const uint32_t first = flat.at(d[0]), n = (uint32_t)d.size();
        DUtils::Random::SeedRand((int)((base ^ (first * 0x9E3779B1u) ^ (n * 0x85EBCA6Bu)) & 0x7fffffffu));
        initiateClustersKMpp(d, clusters);
    }
    size_t nnodes() const { return m_nodes.size(); }
    void tree(int* parent, uint8_t* leaf, uint8_t* desc, double* weight) const
    {
        for (size_t i = 0; i < m_nodes.size(); i++) {
            const Node& n = m_nodes[i];
            parent[i] = (int)n.parent; leaf[i] = i > 0 && n.isLeaf(); weight[i] = n.weight;
            if (i > 0) memcpy(desc + i * 32, n.descriptor.data, 32); else memset(desc, 0, 32);
        }
    }
    DBoW2::WordId word(const cv::Mat& f) const { DBoW2::WordId w; transform(f, w); return w; }
};

struct Run { TrainVoc voc; std::vector<std::vector<cv::Mat> > feats; double seconds = 0; };

extern "C" {

void* vt_ref_create(const uint8_t* desc, const int* counts, int nimages, int k, int L, int weighting, int scoring, uint32_t seed)
{
    Run* r = new Run();
    r->feats.resize(nimages);
    size_t off = 0;
    for (int i = 0; i < nimages; i++) {
        r->feats[i].resize(counts[i]);
        for (int j = 0; j < counts[i]; j++, off++) { r->feats[i][j].create(1, 32, CV_8U); memcpy(r->feats[i][j].data, desc + off * 32, 32); }
    }
    uint32_t idx = 0;
    for (size_t i = 0; i < r->feats.size(); i++) for (size_t j = 0; j < r->feats[i].size(); j++) r->voc.flat[&r->feats[i][j]] = idx++;
    r->voc.base = seed;
    DUtils::Random::SeedRandOnce(0);
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    r->voc.create(r->feats, k, L, (DBoW2::WeightingType)weighting, (DBoW2::ScoringType)scoring);
    r->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return r;
}
void vt_ref_free(void* h) { delete (Run*)h; }
double vt_ref_seconds(void* h) { return ((Run*)h)->seconds; }
int vt_ref_nodes(void* h) { return (int)((Run*)h)->voc.nnodes(); }
int vt_ref_words(void* h) { return (int)((Run*)h)->voc.size(); }
void vt_ref_tree(void* h, int* parent, uint8_t* leaf, uint8_t* desc, double* weight) { ((Run*)h)->voc.tree(parent, leaf, desc, weight); }
void vt_ref_after(void* h, uint8_t* out)
{
    Run* r = (Run*)h; size_t off = 0;
    for (size_t i = 0; i < r->feats.size(); i++) for (size_t j = 0; j < r->feats[i].size(); j++, off++) memcpy(out + off * 32, r->feats[i][j].data, 32);
}
// Ni as setNodeWeights counts it (:962-983), by the reference's own per-feature transform
void vt_ref_word_docs(void* h, int* ni)
{
    Run* r = (Run*)h;
    const size_t nw = r->voc.size();
    for (size_t w = 0; w < nw; w++) ni[w] = 0;
    std::vector<char> counted(nw);
    for (size_t i = 0; i < r->feats.size(); i++) {
        std::fill(counted.begin(), counted.end(), 0);
        for (size_t j = 0; j < r->feats[i].size(); j++) { const DBoW2::WordId w = r->voc.word(r->feats[i][j]); if (!counted[w]) { counted[w] = 1; ni[w]++; } }
    }
}
void vt_ref_save(void* h, const char* path) { ((Run*)h)->voc.saveToTextFile(path); }

}  // extern "C"
