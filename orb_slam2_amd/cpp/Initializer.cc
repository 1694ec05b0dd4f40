// Initializer.cc — ORB_SLAM2::Initializer with FindHomography, FindFundamental, the model choice, ReconstructH / ReconstructF, CheckRT and Triangulate
// on the device: one call of orbhip_init_reconstruct per Initialize(), one call of orbhip_init_reconstruct_batch per InitializeBatch().  Declared in
// include/Initializer.h, which states the two deviations from the reference.
//
// The host part is the reference's constructor (Initializer.cc:33-42), the match list and the draws of Initialize (:44-97), Normalize's sums
// (:749-781) and the scatter of CheckRT's per-match results to mvMatches12[i].first (:843, :889, :893).
#include "Initializer.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>

#include "ORBextractor.h"   // ORBhipError
#include "orbhip.h"
#include "orbhip_gemm_probe.h"

#if defined(__has_include)
#if __has_include("Thirdparty/DBoW2/DUtils/Random.h")
#include "Thirdparty/DBoW2/DUtils/Random.h"
#else
#include "Random.h"
#endif
#else
#include "Thirdparty/DBoW2/DUtils/Random.h"
#endif

using namespace std;

namespace ORB_SLAM2
{

namespace
{

int Device()
{
    static const int device = getenv("ORBHIP_DEVICE") ? atoi(getenv("ORBHIP_DEVICE")) : 0;      // read once per process, like ORBmatcher.cc
    return device;
}

int GemmMode()
{
    static const int mode = orbhip_probe_gemm_mode<cv::Mat>(CV_32F);
    return mode;
}

// One axis of Normalize (:749-781): the mean and the reciprocal of the mean absolute deviation of one coordinate over every key point.  Both sums
// are serial float sums in index order - their bits depend on that order - and the reciprocal is a double division rounded to float.
void AxisStats(const vector<cv::KeyPoint> &vKeys, float cv::Point2f::*axis, float &mean, float &scale)
{
    const int nKeys = vKeys.size();
    float sum = 0;
    for(int i=0; i<nKeys; i++)
        sum += vKeys[i].pt.*axis;
    mean = sum/nKeys;

    float dev = 0;
    for(int i=0; i<nKeys; i++)
    {
        const float centred = vKeys[i].pt.*axis - mean;
        dev += std::fabs(centred);
    }
    dev = dev/nKeys;
    scale = 1.0/dev;
}

// meanX, meanY, sX, sY as the device reads them
void NormalizeSums(const vector<cv::KeyPoint> &vKeys, float out[4])
{
    AxisStats(vKeys,&cv::Point2f::x,out[0],out[2]);
    AxisStats(vKeys,&cv::Point2f::y,out[1],out[3]);
}

} // namespace

struct Initializer::Call
{
    vector<float> vMatches;         // u1 v1 u2 v2 of pair i in mvMatches12 order
    vector<int32_t> vSets;
    vector<uint8_t> vMaskH, vMaskF, vTriangulated;
    vector<float> vP3D;
    orbhip_init_problem problem;
};

Initializer::Initializer(const Frame &ReferenceFrame, float sigma, int iterations):
    mvKeys1(ReferenceFrame.mvKeysUn), mK(ReferenceFrame.mK.clone()), mSigma(sigma), mSigma2(sigma*sigma), mMaxIterations(iterations), mnGemmMode(GemmMode())
{
    if(mnGemmMode==2)
        throw ORBhipError("Initializer: the linked cv::Mat rounds R*x+t in neither of the two known ways (gemm mode 2), and every product of the initialiser is per hypothesis on the device");
}

bool Initializer::Prepare(const Frame &CurrentFrame, const vector<int> &vMatches12, Call &call)
{
    mvKeys2 = CurrentFrame.mvKeysUn;

    // the pairs (index in frame 1, index in frame 2), in rising order of the first: the order every per-match buffer of the call follows
    mvMatches12.clear();
    mvbMatched1.assign(mvKeys1.size(),false);
    for(size_t i1=0; i1<vMatches12.size(); i1++)
    {
        const int i2 = vMatches12[i1];
        if(i2<0)
            continue;
        mvMatches12.push_back(Match(i1,i2));
        mvbMatched1[i1] = true;
    }

    const int N = mvMatches12.size();
    if(N<8)
        return false;               // before any draw: the generator's stream is left where it was

    // The draws (:68-97): seeded once a process; each set starts from all N indices, takes the one at a drawn position and moves the last
    // still-available index into its place, eight times.  8 * mMaxIterations values of RandomInt, with ranges 0..N-1 down to 0..N-8 per set.
    DUtils::Random::SeedRandOnce(0);
    mvSets.assign(mMaxIterations,vector<size_t>(8,0));
    call.vSets.resize(8*(size_t)mMaxIterations);
    vector<int32_t> vPool(N);
    for(int it=0; it<mMaxIterations; it++)
    {
        for(int i=0; i<N; i++)
            vPool[i] = i;
        for(int j=0, nLeft=N; j<8; j++, nLeft--)
        {
            const int pos = DUtils::Random::RandomInt(0,nLeft-1);
            mvSets[it][j] = vPool[pos];
            call.vSets[8*it+j] = vPool[pos];
            vPool[pos] = vPool[nLeft-1];
        }
    }

    call.vMatches.resize(4*(size_t)N);
    for(int i=0; i<N; i++)
    {
        const cv::Point2f &p1 = mvKeys1[mvMatches12[i].first].pt;
        const cv::Point2f &p2 = mvKeys2[mvMatches12[i].second].pt;
        float *pm = &call.vMatches[4*(size_t)i];
        pm[0] = p1.x; pm[1] = p1.y; pm[2] = p2.x; pm[3] = p2.y;
    }
    call.vMaskH.assign(N,0);
    call.vMaskF.assign(N,0);
    call.vTriangulated.assign(N,0);
    call.vP3D.assign(3*(size_t)N,0.0f);

    orbhip_init_problem &Q = call.problem;
    memset(&Q,0,sizeof(Q));
    Q.K[0] = mK.at<float>(0,0);
    Q.K[1] = mK.at<float>(1,1);
    Q.K[2] = mK.at<float>(0,2);
    Q.K[3] = mK.at<float>(1,2);
    Q.sigma = mSigma;
    NormalizeSums(mvKeys1,Q.norm1);
    NormalizeSums(mvKeys2,Q.norm2);
    Q.matches = call.vMatches.data();
    Q.n = N;
    Q.sets = call.vSets.data();
    Q.n_sets = mMaxIterations;
    Q.min_parallax = 1.0;           // Initialize passes 1.0 and 50 to ReconstructH / ReconstructF
    Q.min_triangulated = 50;
    Q.gemm_mode = mnGemmMode;
    Q.mask_h = call.vMaskH.data();
    Q.mask_f = call.vMaskF.data();
    Q.p3d = call.vP3D.data();
    Q.triangulated = call.vTriangulated.data();
    return true;
}

bool Initializer::Absorb(const Call &call, cv::Mat &R21, cv::Mat &t21, vector<cv::Point3f> &vP3D, vector<bool> &vbTriangulated)
{
    const orbhip_init_problem &Q = call.problem;
    if(!Q.returned)
    {
        if(Q.model!=0)              // ReconstructF empties both before its tests; so does the call without a model
        {
            R21 = cv::Mat();
            t21 = cv::Mat();
        }
        return false;
    }

    R21 = cv::Mat(3,3,CV_32F);
    t21 = cv::Mat(3,1,CV_32F);
    for(int r=0; r<3; r++)
    {
        for(int c=0; c<3; c++)
            R21.at<float>(r,c) = Q.R21[3*r+c];
        t21.at<float>(r) = Q.t21[r];
    }

    // the reference indexes both outputs by the key point of frame 1 (:843, :889, :893); the device answers per match
    vP3D = vector<cv::Point3f>(mvKeys1.size());
    vbTriangulated = vector<bool>(mvKeys1.size(),false);
    for(size_t i=0, iend=mvMatches12.size(); i<iend; i++)
    {
        const int first = mvMatches12[i].first;
        if(call.vTriangulated[i])
            vbTriangulated[first] = true;
        vP3D[first] = cv::Point3f(call.vP3D[3*i],call.vP3D[3*i+1],call.vP3D[3*i+2]);      // zero where CheckRT assigned nothing
    }
    return true;
}

bool Initializer::Initialize(const Frame &CurrentFrame, const vector<int> &vMatches12, cv::Mat &R21, cv::Mat &t21,
                             vector<cv::Point3f> &vP3D, vector<bool> &vbTriangulated)
{
    Call call;
    if(!Prepare(CurrentFrame,vMatches12,call))
        return false;
    if(orbhip_init_reconstruct(Device(),&call.problem)!=ORBHIP_OK)
        throw ORBhipError(string("Initializer::Initialize: ")+orbhip_last_error());
    return Absorb(call,R21,t21,vP3D,vbTriangulated);
}

void Initializer::InitializeBatch(const vector<Initializer*> &vpInitializers, const vector<const Frame*> &vpCurrentFrames,
                                  const vector<vector<int> > &vvMatches12, vector<cv::Mat> &vR21, vector<cv::Mat> &vt21,
                                  vector<vector<cv::Point3f> > &vvP3D, vector<vector<bool> > &vvbTriangulated, vector<bool> &vbOk)
{
    const size_t n = vpInitializers.size();
    vR21.resize(n);
    vt21.resize(n);
    vvP3D.resize(n);
    vvbTriangulated.resize(n);
    vbOk.assign(n,false);

    vector<Call> vCalls(n);
    vector<size_t> vLive;
    for(size_t i=0; i<n; i++)
    {
        if(!vpInitializers[i] || i>=vpCurrentFrames.size() || !vpCurrentFrames[i] || i>=vvMatches12.size())
            continue;
        if(vpInitializers[i]->Prepare(*vpCurrentFrames[i],vvMatches12[i],vCalls[i]))
            vLive.push_back(i);
    }
    if(vLive.empty())
        return;

    vector<orbhip_init_problem> vProblems(vLive.size());
    for(size_t k=0; k<vLive.size(); k++)
        vProblems[k] = vCalls[vLive[k]].problem;
    if(orbhip_init_reconstruct_batch(Device(),vProblems.size(),vProblems.data())!=ORBHIP_OK)
        throw ORBhipError(string("Initializer::InitializeBatch: ")+orbhip_last_error());
    for(size_t k=0; k<vLive.size(); k++)
    {
        const size_t i = vLive[k];
        vCalls[i].problem = vProblems[k];
        vbOk[i] = vpInitializers[i]->Absorb(vCalls[i],vR21[i],vt21[i],vvP3D[i],vvbTriangulated[i]);
    }
}

} //namespace ORB_SLAM
