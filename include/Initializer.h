// Initializer.h — ORB_SLAM2::Initializer (include/Initializer.h, src/Initializer.cc of the reference) with both RANSACs, the model choice, the motion
// hypotheses, CheckRT / Triangulate and the selection rules on the device (orbhip_init_reconstruct / orbhip_init_reconstruct_batch,
// include/orbhip.h).  Same public signatures; INTEGRATION.md step 3p.
//
// The host keeps what cannot move without changing bits: the draws (DUtils::Random::SeedRandOnce(0), RandomInt and the reference's swap-remove over a
// fresh copy of the indices per set), Normalize's two serial float passes over ALL key points of each frame, and the scatter of the per-match
// results to mvMatches12[i].first.  The reference's private solver members (FindHomography, ComputeH21, CheckRT, ...) and its pair of std::threads are
// NOT kept: that arithmetic runs in one device call, as DESIGN.md H19 states it.
//
// TWO DEVIATIONS: with fewer than 8 matches the reference reads back() of an empty vector; Initialize returns false before any draw.  Where no
// hypothesis of the chosen model scores above 0 the reference hands an empty Mat to the reconstruction and OpenCV throws; Initialize returns false
// with empty R21 and t21.
// THE DRAWS AND rand(): the sets come from the C library's rand(), seeded once a process, as in the reference.  rand() belongs to the whole process.
// Where the HIP runtime is loaded it takes values of rand() itself between device calls (observed on an MI355X: the first Initialize of a process draws
// the reference's sets from seed 0, later ones do not), so from the second call on the sets are valid draws but not the ones the reference would have
// drawn at that point of its stream.  Under the CPU emulation of the kernels the whole stream is the reference's.
// A cv::Mat whose `R*x+t` rounds in neither known way (gemm mode 2, include/orbhip_gemm_probe.h) makes the constructor throw ORBhipError.
#ifndef INITIALIZER_H
#define INITIALIZER_H

#include <opencv2/opencv.hpp>
#include <utility>
#include <vector>

#include "Frame.h"

namespace ORB_SLAM2
{

// Monocular initialisation only: stereo and RGB-D tracking never construct one.
class Initializer
{
    typedef std::pair<int,int> Match;

public:

    // keeps the reference frame's undistorted key points and calibration
    Initializer(const Frame &ReferenceFrame, float sigma = 1.0, int iterations = 200);

    // One device call: H and F by RANSAC over the same sets, the model choice, motion and structure.  vP3D and vbTriangulated are indexed by the
    // reference frame's key points.
    bool Initialize(const Frame &CurrentFrame, const std::vector<int> &vMatches12,
                    cv::Mat &R21, cv::Mat &t21, std::vector<cv::Point3f> &vP3D, std::vector<bool> &vbTriangulated);

    // Several candidate frame pairs in ONE device call: element i of the outputs is what vpInitializers[i]->Initialize(*vpCurrentFrames[i],
    // vvMatches12[i], ...) gives from the same draws, bit for bit.  NULL initialisers (or frames) are skipped: false, their outputs untouched.
    // Draws are made in vector order.
    static void InitializeBatch(const std::vector<Initializer*> &vpInitializers, const std::vector<const Frame*> &vpCurrentFrames,
                                const std::vector<std::vector<int> > &vvMatches12, std::vector<cv::Mat> &vR21, std::vector<cv::Mat> &vt21,
                                std::vector<std::vector<cv::Point3f> > &vvP3D, std::vector<std::vector<bool> > &vvbTriangulated, std::vector<bool> &vbOk);

protected:

    struct Call;                                                        // one call's problem record and the buffers it points to (Initializer.cc)
    bool Prepare(const Frame &CurrentFrame, const std::vector<int> &vMatches12, Call &call);      // false: fewer than 8 matches
    bool Absorb(const Call &call, cv::Mat &R21, cv::Mat &t21, std::vector<cv::Point3f> &vP3D, std::vector<bool> &vbTriangulated);

    std::vector<cv::KeyPoint> mvKeys1;                  // frame 1 (reference), undistorted
    std::vector<cv::KeyPoint> mvKeys2;                  // frame 2 (current) of the last call
    std::vector<Match> mvMatches12;                     // (index in frame 1, index in frame 2), rising in the first
    std::vector<bool> mvbMatched1;
    cv::Mat mK;
    float mSigma, mSigma2;
    int mMaxIterations;                                 // sets per model
    std::vector<std::vector<size_t> > mvSets;           // the sets of the last call
    int mnGemmMode;
};

} //namespace ORB_SLAM

#endif // INITIALIZER_H
