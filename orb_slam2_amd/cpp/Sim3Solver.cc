// Sim3Solver.cc — ORB_SLAM2::Sim3Solver with ComputeSim3, CheckInliers and the RANSAC bookkeeping of iterate() on the device: one call of
// orbhip_sim3_iterate per iterate() / find(), one call of orbhip_sim3_iterate_batch per IterateBatch().  Declared in include/Sim3Solver.h, which
// states the one deviation from the reference (draws made up front, kept in a queue after an early return).
//
// The host part is the reference's constructor (Sim3Solver.cc:37-112), SetRansacParameters (:114-138) and the draw of iterate() (:163-177).
#include "Sim3Solver.h"

#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>

#include "KeyFrame.h"
#include "MapPoint.h"
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

} // namespace

struct Sim3Solver::Round
{
    vector<int32_t> vTriples;
    vector<uint8_t> vInliers;
    orbhip_sim3_problem problem;
};

Sim3Solver::Sim3Solver(KeyFrame *pKF1, KeyFrame *pKF2, const vector<MapPoint *> &vpMatched12, const bool bFixScale):
    mnIterations(0), mnBestInliers(0), mBestScale(0.0f), mbFixScale(bFixScale), mnGemmMode(GemmMode())
{
    if(mnGemmMode==2)
        throw ORBhipError("Sim3Solver: the linked cv::Mat rounds R*x+t in neither of the two known ways (gemm mode 2), and every product of the solver is per hypothesis on the device");

    vector<MapPoint*> vpKeyFrameMP1 = pKF1->GetMapPointMatches();

    mN1 = vpMatched12.size();

    mvnIndices1.reserve(mN1);
    mvCorr.reserve(8*(size_t)mN1);

    cv::Mat Rcw1 = pKF1->GetRotation();
    cv::Mat tcw1 = pKF1->GetTranslation();
    cv::Mat Rcw2 = pKF2->GetRotation();
    cv::Mat tcw2 = pKF2->GetTranslation();

    mvAllIndices.reserve(mN1);

    size_t idx=0;
    for(int i1=0; i1<mN1; i1++)
    {
        if(vpMatched12[i1])
        {
            MapPoint* pMP1 = vpKeyFrameMP1[i1];
            MapPoint* pMP2 = vpMatched12[i1];

            if(!pMP1)
                continue;

            if(pMP1->isBad() || pMP2->isBad())
                continue;

            int indexKF1 = pMP1->GetIndexInKeyFrame(pKF1);
            int indexKF2 = pMP2->GetIndexInKeyFrame(pKF2);

            if(indexKF1<0 || indexKF2<0)
                continue;

            const cv::KeyPoint &kp1 = pKF1->mvKeysUn[indexKF1];
            const cv::KeyPoint &kp2 = pKF2->mvKeysUn[indexKF2];

            const float sigmaSquare1 = pKF1->mvLevelSigma2[kp1.octave];
            const float sigmaSquare2 = pKF2->mvLevelSigma2[kp2.octave];

            mvnIndices1.push_back(i1);

            cv::Mat X3D1w = pMP1->GetWorldPos();
            cv::Mat X3D1c = Rcw1*X3D1w+tcw1;

            cv::Mat X3D2w = pMP2->GetWorldPos();
            cv::Mat X3D2c = Rcw2*X3D2w+tcw2;

            for(int r=0; r<3; r++)
                mvCorr.push_back(X3D1c.at<float>(r));
            for(int r=0; r<3; r++)
                mvCorr.push_back(X3D2c.at<float>(r));
            mvCorr.push_back(sigmaSquare1);         // the device forms (float)(size_t)(9.210*sigma^2): mvnMaxError1/2
            mvCorr.push_back(sigmaSquare2);

            mvAllIndices.push_back(idx);
            idx++;
        }
    }

    const cv::Mat &K1 = pKF1->mK;
    const cv::Mat &K2 = pKF2->mK;
    mK1[0] = K1.at<float>(0,0); mK1[1] = K1.at<float>(1,1); mK1[2] = K1.at<float>(0,2); mK1[3] = K1.at<float>(1,2);
    mK2[0] = K2.at<float>(0,0); mK2[1] = K2.at<float>(1,1); mK2[2] = K2.at<float>(0,2); mK2[3] = K2.at<float>(1,2);

    SetRansacParameters();
}

void Sim3Solver::SetRansacParameters(double probability, int minInliers, int maxIterations)
{
    mRansacProb = probability;
    mRansacMinInliers = minInliers;
    mRansacMaxIts = maxIterations;

    N = mvCorr.size()/8; // number of correspondences

    // Set RANSAC iterations according to probability, epsilon, and max iterations
    int nIterations;

    if(mRansacMinInliers==N)
        nIterations=1;
    else if(N==0)
        nIterations=INT_MIN;
    else
    {
        // Adjust Parameters according to number of correspondences
        float epsilon = (float)mRansacMinInliers/N;
        const double x = ceil(log(1-mRansacProb)/log(1-pow(epsilon,3)));
        nIterations = (std::isfinite(x) && x>=-2147483648.0 && x<2147483648.0) ? (int)x : INT_MIN;    // x86's answer where the conversion is undefined
    }

    mRansacMaxIts = max(1,min(nIterations,mRansacMaxIts));

    mnIterations = 0;
}

bool Sim3Solver::Prepare(int nIterations, Round &round)
{
    if(N<mRansacMinInliers || N<3)
        return false;

    const int nNeeded = max(0,min(nIterations,mRansacMaxIts-mnIterations));

    round.vTriples.clear();
    round.vTriples.reserve(3*(size_t)nNeeded);
    while((int)round.vTriples.size()<3*nNeeded && !mqDrawn.empty())
    {
        round.vTriples.push_back(mqDrawn.front());
        mqDrawn.pop_front();
    }

    vector<size_t> vAvailableIndices;
    while((int)round.vTriples.size()<3*nNeeded)
    {
        vAvailableIndices = mvAllIndices;

        // Get min set of points
        for(short i = 0; i < 3; ++i)
        {
            int randi = DUtils::Random::RandomInt(0, vAvailableIndices.size()-1);

            int idx = vAvailableIndices[randi];

            round.vTriples.push_back(idx);

            vAvailableIndices[randi] = vAvailableIndices.back();
            vAvailableIndices.pop_back();
        }
    }

    round.vInliers.assign(N, 0);

    orbhip_sim3_problem &Q = round.problem;
    memset(&Q, 0, sizeof Q);
    memcpy(Q.K1, mK1, sizeof Q.K1);
    memcpy(Q.K2, mK2, sizeof Q.K2);
    Q.n = N;
    Q.fix_scale = mbFixScale ? 1 : 0;
    Q.gemm_mode = mnGemmMode;
    Q.n_hyp = nNeeded;
    Q.min_inliers = mRansacMinInliers;
    Q.best_inliers_in = mnBestInliers;
    return true;
}

cv::Mat Sim3Solver::Absorb(const Round &round, bool &bNoMore, vector<bool> &vbInliers, int &nInliers)
{
    const orbhip_sim3_problem &Q = round.problem;

    mnIterations += Q.n_consumed;

    // the triples the device did not consume go back to the head of the queue, in their order
    for(int k=(int)round.vTriples.size()-1; k>=3*Q.n_consumed; k--)
        mqDrawn.push_front(round.vTriples[k]);

    if(Q.best>=0)
    {
        mvbBestInliers.assign(N,false);
        for(int i=0; i<N; i++)
            mvbBestInliers[i] = round.vInliers[i]!=0;
        mnBestInliers = Q.best_inliers_out;
        mBestT12 = cv::Mat(4,4,CV_32F);
        mBestRotation = cv::Mat(3,3,CV_32F);
        mBestTranslation = cv::Mat(3,1,CV_32F);
        for(int r=0; r<4; r++)
            for(int c=0; c<4; c++)
                mBestT12.at<float>(r,c) = Q.T12[4*r+c];
        for(int r=0; r<3; r++)
        {
            for(int c=0; c<3; c++)
                mBestRotation.at<float>(r,c) = Q.R12[3*r+c];
            mBestTranslation.at<float>(r,0) = Q.t12[r];
        }
        mBestScale = Q.s12;

        if(Q.returned>=0)
        {
            nInliers = mnBestInliers;
            for(int i=0; i<N; i++)
                if(mvbBestInliers[i])
                    vbInliers[mvnIndices1[i]] = true;
            return mBestT12;
        }
    }

    if(mnIterations>=mRansacMaxIts)
        bNoMore=true;

    return cv::Mat();
}

cv::Mat Sim3Solver::iterate(int nIterations, bool &bNoMore, vector<bool> &vbInliers, int &nInliers)
{
    bNoMore = false;
    vbInliers = vector<bool>(mN1,false);
    nInliers=0;

    Round round;
    if(!Prepare(nIterations, round))
    {
        bNoMore = true;
        return cv::Mat();
    }
    orbhip_sim3_problem &Q = round.problem;
    Q.corr = reinterpret_cast<const orbhip_sim3_corr*>(&mvCorr[0]);
    Q.triples = round.vTriples.empty() ? NULL : &round.vTriples[0];
    Q.inliers = &round.vInliers[0];

    if(orbhip_sim3_iterate(Device(), &Q)!=ORBHIP_OK)
        throw ORBhipError(string("Sim3Solver::iterate: ") + orbhip_last_error());

    return Absorb(round, bNoMore, vbInliers, nInliers);
}

cv::Mat Sim3Solver::find(vector<bool> &vbInliers12, int &nInliers)
{
    bool bFlag;
    return iterate(mRansacMaxIts,bFlag,vbInliers12,nInliers);
}

void Sim3Solver::IterateBatch(const vector<Sim3Solver*> &vpSolvers, int nIterations, vector<cv::Mat> &vScm, vector<bool> &vbNoMore,
                              vector<vector<bool> > &vvbInliers, vector<int> &vnInliers)
{
    const size_t nSolvers = vpSolvers.size();
    vScm.assign(nSolvers, cv::Mat());
    vbNoMore.assign(nSolvers, false);
    vvbInliers.assign(nSolvers, vector<bool>());
    vnInliers.assign(nSolvers, 0);

    vector<Round> vRounds(nSolvers);
    vector<size_t> vnLive;
    for(size_t i=0; i<nSolvers; i++)
    {
        Sim3Solver* pSolver = vpSolvers[i];
        if(!pSolver)
            continue;
        vvbInliers[i] = vector<bool>(pSolver->mN1,false);
        if(!pSolver->Prepare(nIterations, vRounds[i]))
        {
            vbNoMore[i] = true;
            continue;
        }
        vnLive.push_back(i);
    }
    if(vnLive.empty())
        return;

    vector<orbhip_sim3_problem> vProblems(vnLive.size());
    for(size_t k=0; k<vnLive.size(); k++)
    {
        Round &round = vRounds[vnLive[k]];
        orbhip_sim3_problem &Q = round.problem;
        Q.corr = reinterpret_cast<const orbhip_sim3_corr*>(&vpSolvers[vnLive[k]]->mvCorr[0]);
        Q.triples = round.vTriples.empty() ? NULL : &round.vTriples[0];
        Q.inliers = &round.vInliers[0];
        vProblems[k] = Q;
    }

    if(orbhip_sim3_iterate_batch(Device(), (int)vProblems.size(), &vProblems[0])!=ORBHIP_OK)
        throw ORBhipError(string("Sim3Solver::IterateBatch: ") + orbhip_last_error());

    for(size_t k=0; k<vnLive.size(); k++)
    {
        const size_t i = vnLive[k];
        vRounds[i].problem = vProblems[k];
        bool bNoMore = false;
        int nInliers = 0;
        vScm[i] = vpSolvers[i]->Absorb(vRounds[i], bNoMore, vvbInliers[i], nInliers);
        vbNoMore[i] = bNoMore;
        vnInliers[i] = nInliers;
    }
}

cv::Mat Sim3Solver::GetEstimatedRotation()
{
    return mBestRotation.clone();
}

cv::Mat Sim3Solver::GetEstimatedTranslation()
{
    return mBestTranslation.clone();
}

float Sim3Solver::GetEstimatedScale()
{
    return mBestScale;
}

} //namespace ORB_SLAM
