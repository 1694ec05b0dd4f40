// PnPsolver.cc — ORB_SLAM2::PnPsolver with compute_pose (EPnP), CheckInliers, Refine and the RANSAC bookkeeping of iterate() on the device: one call
// of orbhip_pnp_iterate per 4096 hypotheses of an iterate() / find(), one call of orbhip_pnp_iterate_batch per such part of an IterateBatch().
// Declared in include/PnPsolver.h, which states the one deviation from the reference (draws made up front, kept in a queue after an early return).
//
// The host part is the reference's constructor (PnPsolver.cc:67-110), SetRansacParameters (:121-157), the draw of iterate() (:188-201) and what
// iterate() does after its loop (:241-257).
#include "PnPsolver.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>

#include "ORBextractor.h"   // ORBhipError
#include "orbhip.h"

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

const int kMaxHypotheses = 4096;      // of one device call (include/orbhip.h)

int Device()
{
    static const int device = getenv("ORBHIP_DEVICE") ? atoi(getenv("ORBHIP_DEVICE")) : 0;      // read once per process, like ORBmatcher.cc
    return device;
}

cv::Mat ToMat(const float T[16])
{
    cv::Mat M(4,4,CV_32F);
    for(int r=0; r<4; r++)
        for(int c=0; c<4; c++)
            M.at<float>(r,c) = T[4*r+c];
    return M;
}

} // namespace

struct PnPsolver::Round
{
    vector<int32_t> vQuads;         // every quadruple of the call
    size_t nPos;                    // hypotheses already handed to the device
    vector<uint8_t> vBestIn, vBest, vRefined;
    orbhip_pnp_problem problem;
    cv::Mat result;
    Round() : nPos(0) {}
};

PnPsolver::PnPsolver(const Frame &F, const vector<MapPoint*> &vpMapPointMatches):
    mnMatches(vpMapPointMatches.size()), mnIterations(0), mnBestInliers(0), N(0)
{
    mvCorr.reserve(6*F.mvpMapPoints.size());
    mvSigma2.reserve(F.mvpMapPoints.size());
    mvKeyPointIndices.reserve(F.mvpMapPoints.size());
    mvAllIndices.reserve(F.mvpMapPoints.size());

    int idx=0;
    for(size_t i=0, iend=vpMapPointMatches.size(); i<iend; i++)
    {
        MapPoint* pMP = vpMapPointMatches[i];

        if(pMP)
        {
            if(!pMP->isBad())
            {
                const cv::KeyPoint &kp = F.mvKeysUn[i];

                cv::Mat Pos = pMP->GetWorldPos();
                mvCorr.push_back(Pos.at<float>(0));
                mvCorr.push_back(Pos.at<float>(1));
                mvCorr.push_back(Pos.at<float>(2));
                mvCorr.push_back(kp.pt.x);
                mvCorr.push_back(kp.pt.y);
                mvCorr.push_back(0.0f);                 // mvMaxError: SetRansacParameters

                mvSigma2.push_back(F.mvLevelSigma2[kp.octave]);

                mvKeyPointIndices.push_back(i);
                mvAllIndices.push_back(idx);

                idx++;
            }
        }
    }

    // Set camera calibration parameters
    mK[0] = F.fx;
    mK[1] = F.fy;
    mK[2] = F.cx;
    mK[3] = F.cy;

    SetRansacParameters();
}

PnPsolver::~PnPsolver()
{
}

void PnPsolver::SetRansacParameters(double probability, int minInliers, int maxIterations, int minSet, float epsilon, float th2)
{
    if(minSet!=4)
        throw ORBhipError("PnPsolver::SetRansacParameters: minSet must be 4 - the device solves EPnP from quadruples");

    mRansacProb = probability;
    mRansacMinInliers = minInliers;
    mRansacMaxIts = maxIterations;
    mRansacEpsilon = epsilon;
    mRansacMinSet = minSet;

    N = mvSigma2.size(); // number of correspondences

    // Adjust Parameters according to number of correspondences
    int nMinInliers = N*mRansacEpsilon;
    if(nMinInliers<mRansacMinInliers)
        nMinInliers=mRansacMinInliers;
    if(nMinInliers<minSet)
        nMinInliers=minSet;
    mRansacMinInliers = nMinInliers;

    if(N>0 && mRansacEpsilon<(float)mRansacMinInliers/N)
        mRansacEpsilon=(float)mRansacMinInliers/N;

    // Set RANSAC iterations according to probability, epsilon, and max iterations
    int nIterations;

    if(mRansacMinInliers==N)
        nIterations=1;
    else if(N==0)
        nIterations=INT_MIN;
    else
    {
        const double x = ceil(log(1-mRansacProb)/log(1-pow(mRansacEpsilon,3)));
        nIterations = (std::isfinite(x) && x>=-2147483648.0 && x<2147483648.0) ? (int)x : INT_MIN;    // x86's answer where the conversion is undefined
    }

    mRansacMaxIts = max(1,min(nIterations,mRansacMaxIts));

    for(size_t i=0; i<mvSigma2.size(); i++)
        mvCorr[6*i+5] = mvSigma2[i]*th2;
}

bool PnPsolver::Prepare(int nIterations, Round &round)
{
    if(N<mRansacMinInliers)
        return false;

    // while(mnIterations<mRansacMaxIts || nCurrentIterations<nIterations)
    const int nNeeded = max(0,max(nIterations,mRansacMaxIts-mnIterations));

    round.nPos = 0;
    round.vQuads.clear();
    round.vQuads.reserve(4*(size_t)nNeeded);
    while(round.vQuads.size()<4*(size_t)nNeeded && !mqDrawn.empty())
    {
        round.vQuads.push_back(mqDrawn.front());
        mqDrawn.pop_front();
    }

    vector<size_t> vAvailableIndices;
    while(round.vQuads.size()<4*(size_t)nNeeded)
    {
        vAvailableIndices = mvAllIndices;

        // Get min set of points
        for(short i = 0; i < mRansacMinSet; ++i)
        {
            int randi = DUtils::Random::RandomInt(0, vAvailableIndices.size()-1);

            int idx = vAvailableIndices[randi];

            round.vQuads.push_back(idx);

            vAvailableIndices[randi] = vAvailableIndices.back();
            vAvailableIndices.pop_back();
        }
    }

    round.vBest.assign(N, 0);
    round.vRefined.assign(N, 0);
    return true;
}

bool PnPsolver::NextPart(Round &round)
{
    const size_t nLeft = round.vQuads.size()/4 - round.nPos;
    if(nLeft==0)
        return false;

    round.vBestIn = mvbBestInliers;

    orbhip_pnp_problem &Q = round.problem;
    memset(&Q, 0, sizeof Q);
    memcpy(Q.K, mK, sizeof Q.K);
    Q.corr = reinterpret_cast<const orbhip_pnp_corr*>(&mvCorr[0]);
    Q.n = N;
    Q.quads = &round.vQuads[4*round.nPos];
    Q.n_hyp = (int)min<size_t>(nLeft, kMaxHypotheses);
    Q.min_inliers = mRansacMinInliers;
    Q.best_inliers_in = mnBestInliers;
    Q.best_mask_in = mnBestInliers>0 ? &round.vBestIn[0] : NULL;
    Q.best_mask = &round.vBest[0];
    Q.refined_mask = &round.vRefined[0];
    return true;
}

bool PnPsolver::Absorb(Round &round, vector<bool> &vbInliers, int &nInliers)
{
    const orbhip_pnp_problem &Q = round.problem;

    mnIterations += Q.n_consumed;

    if(Q.best>=0)
    {
        mvbBestInliers = round.vBest;
        mnBestInliers = Q.best_inliers_out;
        mBestTcw = ToMat(Q.best_Tcw);
    }

    if(Q.returned>=0)
    {
        // the quadruples the device did not consume go back to the head of the queue, in their order
        for(size_t k=round.vQuads.size(); k>4*(round.nPos+Q.n_consumed); k--)
            mqDrawn.push_front(round.vQuads[k-1]);

        nInliers = Q.refined_inliers;
        vbInliers = vector<bool>(mnMatches,false);
        for(int i=0; i<N; i++)
        {
            if(round.vRefined[i])
                vbInliers[mvKeyPointIndices[i]] = true;
        }
        round.result = ToMat(Q.refined_Tcw);
        return true;
    }

    round.nPos += Q.n_hyp;
    return false;
}

cv::Mat PnPsolver::Finish(bool &bNoMore, vector<bool> &vbInliers, int &nInliers)
{
    if(mnIterations>=mRansacMaxIts)
    {
        bNoMore=true;
        if(mnBestInliers>=mRansacMinInliers)
        {
            nInliers=mnBestInliers;
            vbInliers = vector<bool>(mnMatches,false);
            for(int i=0; i<N; i++)
            {
                if(mvbBestInliers[i])
                    vbInliers[mvKeyPointIndices[i]] = true;
            }
            return mBestTcw.clone();
        }
    }

    return cv::Mat();
}

cv::Mat PnPsolver::iterate(int nIterations, bool &bNoMore, vector<bool> &vbInliers, int &nInliers)
{
    bNoMore = false;
    vbInliers.clear();
    nInliers=0;

    Round round;
    if(!Prepare(nIterations, round))
    {
        bNoMore = true;
        return cv::Mat();
    }

    while(NextPart(round))
    {
        if(orbhip_pnp_iterate(Device(), &round.problem)!=ORBHIP_OK)
            throw ORBhipError(string("PnPsolver::iterate: ") + orbhip_last_error());

        if(Absorb(round, vbInliers, nInliers))
            return round.result;
    }

    return Finish(bNoMore, vbInliers, nInliers);
}

cv::Mat PnPsolver::find(vector<bool> &vbInliers, int &nInliers)
{
    bool bFlag;
    return iterate(mRansacMaxIts,bFlag,vbInliers,nInliers);
}

void PnPsolver::IterateBatch(const vector<PnPsolver*> &vpSolvers, int nIterations, vector<cv::Mat> &vTcw, vector<bool> &vbNoMore,
                             vector<vector<bool> > &vvbInliers, vector<int> &vnInliers)
{
    const size_t nSolvers = vpSolvers.size();
    vTcw.assign(nSolvers, cv::Mat());
    vbNoMore.assign(nSolvers, false);
    vvbInliers.assign(nSolvers, vector<bool>());
    vnInliers.assign(nSolvers, 0);

    vector<Round> vRounds(nSolvers);
    vector<size_t> vnOpen;                      // solvers still inside their loop
    for(size_t i=0; i<nSolvers; i++)
    {
        PnPsolver* pSolver = vpSolvers[i];
        if(!pSolver)
            continue;
        if(!pSolver->Prepare(nIterations, vRounds[i]))
        {
            vbNoMore[i] = true;
            continue;
        }
        vnOpen.push_back(i);
    }

    vector<bool> vbReturned(nSolvers,false);
    const vector<size_t> vnPrepared = vnOpen;
    while(!vnOpen.empty())
    {
        vector<size_t> vnLive;
        vector<orbhip_pnp_problem> vProblems;
        for(size_t k=0; k<vnOpen.size(); k++)
        {
            const size_t i = vnOpen[k];
            if(vpSolvers[i]->NextPart(vRounds[i]))
            {
                vnLive.push_back(i);
                vProblems.push_back(vRounds[i].problem);
            }
        }
        if(vnLive.empty())
            break;

        if(orbhip_pnp_iterate_batch(Device(), (int)vProblems.size(), &vProblems[0])!=ORBHIP_OK)
            throw ORBhipError(string("PnPsolver::IterateBatch: ") + orbhip_last_error());

        vnOpen.clear();
        for(size_t k=0; k<vnLive.size(); k++)
        {
            const size_t i = vnLive[k];
            vRounds[i].problem = vProblems[k];
            int nInliers = 0;
            if(vpSolvers[i]->Absorb(vRounds[i], vvbInliers[i], nInliers))
            {
                vTcw[i] = vRounds[i].result;
                vnInliers[i] = nInliers;
                vbReturned[i] = true;
            }
            else
                vnOpen.push_back(i);
        }
    }

    for(size_t k=0; k<vnPrepared.size(); k++)
    {
        const size_t i = vnPrepared[k];
        if(vbReturned[i])
            continue;
        bool bNoMore = false;
        int nInliers = 0;
        vTcw[i] = vpSolvers[i]->Finish(bNoMore, vvbInliers[i], nInliers);
        vbNoMore[i] = bNoMore;
        vnInliers[i] = nInliers;
    }
}

} //namespace ORB_SLAM
