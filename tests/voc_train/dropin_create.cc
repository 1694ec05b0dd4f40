// dropin_create.cc — a stand-alone caller of ORB_SLAM2::ORBVocabulary::create / saveToTextFile (include/ORBVocabulary.h), for tests/test_voc_train_dropin_cpp.py.
//   dropin_create <input> <k> <L> <weighting> <scoring> <seed> <saved vocabulary> <features after>
// input: int32 nimages, int32 counts[nimages], then the descriptors (32 bytes each), image after image.  The program builds the reference's argument
// (vector<vector<cv::Mat>>, a Mat of its own per descriptor), calls create, writes the Mats' bytes as create left them, saves the vocabulary, loads it again
// and checks what a caller would: sizes, that a refused create throws and leaves the vocabulary in place, that saving without a vocabulary throws.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "ORBVocabulary.h"
#include "ORBextractor.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "dropin_create: %s failed (line %d)\n", #c, __LINE__); return 1; } } while (0)

int main(int argc, char** argv)
{
    if (argc != 9) { fprintf(stderr, "usage: dropin_create input k L weighting scoring seed voc_out features_out\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    CHECK(f);
    int nimages = 0;
    CHECK(fread(&nimages, 4, 1, f) == 1);
    std::vector<int> counts(nimages);
    CHECK(nimages == 0 || fread(&counts[0], 4, nimages, f) == (size_t)nimages);
    std::vector<std::vector<cv::Mat> > feats(nimages);
    size_t total = 0;
    for (int i = 0; i < nimages; i++) {
        feats[i].resize(counts[i]);
        for (int j = 0; j < counts[i]; j++, total++) { feats[i][j].create(1, 32, CV_8U); CHECK(fread(feats[i][j].data, 32, 1, f) == 1); }
    }
    fclose(f);
    const int k = atoi(argv[2]), L = atoi(argv[3]);
    ORB_SLAM2::ORBVocabulary voc;
    bool threw = false;
    try { voc.saveToTextFile(argv[7]); } catch (const ORB_SLAM2::ORBhipError&) { threw = true; }
    CHECK(threw && voc.empty());
    voc.SetTrainingSeed((unsigned)strtoul(argv[6], NULL, 10));
    voc.create(feats, k, L, (DBoW2::WeightingType)atoi(argv[4]), (DBoW2::ScoringType)atoi(argv[5]));
    const unsigned nwords = voc.size();
    CHECK(total == 0 || nwords > 0);
    f = fopen(argv[8], "wb");
    CHECK(f);
    for (int i = 0; i < nimages; i++) for (int j = 0; j < counts[i]; j++) CHECK(fwrite(feats[i][j].data, 32, 1, f) == 1);      // the caller's own Mats
    fclose(f);
    voc.saveToTextFile(argv[7]);
    threw = false;
    try { voc.create(feats, 1, L); } catch (const ORB_SLAM2::ORBhipError& e) { threw = strstr(e.what(), "k = 1") != NULL; }
    CHECK(threw && voc.size() == nwords);                                     // a refused create leaves the vocabulary as it was
    ORB_SLAM2::ORBVocabulary again;
    CHECK(again.loadFromTextFile(argv[7]) && again.size() == nwords);
    if (total > 0) {
        DBoW2::BowVector a, b; DBoW2::FeatureVector fa, fb;
        voc.transform(feats[nimages - 1].empty() ? feats[0] : feats[nimages - 1], a, fa, 1);
        again.transform(feats[nimages - 1].empty() ? feats[0] : feats[nimages - 1], b, fb, 1);
        CHECK(a.size() == b.size() && fa.size() == fb.size());
        DBoW2::BowVector::const_iterator ia = a.begin(), ib = b.begin();
        for (; ia != a.end(); ++ia, ++ib) CHECK(ia->first == ib->first);
    }
    printf("dropin_create ok: %u words\n", nwords);
    return 0;
}
