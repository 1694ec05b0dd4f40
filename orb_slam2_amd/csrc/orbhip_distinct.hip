// orbhip_distinct.hip — MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:242-307) for a whole key frame's map points in one device call.
//
// A map point's observations are a GROUP of 32-byte descriptors.  The reference fills the group's N x N table of Hamming distances, sorts every row,
// takes element (size_t)(0.5*(N-1)) of the sorted row as the row's median and keeps the FIRST row with the strictly smallest median (MapPoint.cc:272-301).
// Here no table and no sorted row exist in memory:
//   k_distinct_small   groups of up to DS_SMALL_MAX = 64 descriptors, one wavefront per group, four groups per workgroup.  Lane i holds descriptor i;
//                      descriptor j reaches every lane by v_readlane (j is wave-uniform); row i lives in lane i's registers; its k-th smallest value is the
//                      largest v with |{j : d(i,j) < v}| <= k, found bit by bit (9 steps over 0..511); the winner is the wave minimum of median << 6 | lane.
//   k_distinct_large   larger groups, one workgroup per group.  The descriptors are staged in LDS as two planes of 16 bytes (conflict-free ds_read_b128)
//                      while the group has at most DL_STAGE_MAX = 1024 of them, and read through L2 otherwise.  Rows are dealt to the four wavefronts; a
//                      wavefront counts its row into its own 257-bin histogram in LDS, finds the bin that holds rank k by a wave scan, and clears the
//                      bins again.  The winner is the minimum of median << 32 | row: reduced in the wave, then one LDS atomicMin per wavefront.
// Which form a group takes is decided from its size alone: the small kernel skips the large groups, the host lists them for the large kernel.
#include "orbhip_ctx.h"

#define DS_T 256                       // k_distinct_small: four wavefronts = four groups per workgroup
#define DS_SMALL_MAX 64                // largest group of the one-wavefront form
#define DL_T 256                       // k_distinct_large: four wavefronts share one group
#define DL_STAGE_MAX 1024              // largest group whose descriptors are staged in LDS (32 KB)
#define DL_HSTRIDE 260                 // ints between the wavefronts' histograms: 257 bins, rounded up to 16 bytes

struct DistinctParams {
    const uint4* desc;                 // total x 2: descriptor d is desc[2d], desc[2d + 1]
    const int* off;                    // npoints + 1
    int npoints;
    const int* large;                  // groups of more than DS_SMALL_MAX descriptors (the large kernel's work list)
    int2* out;                         // per group {best index, best median}; {-1, -1} for an empty group
};

__device__ __forceinline__ int distinct_distance(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1)
{
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w)
         + __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

__global__ __launch_bounds__(DS_T) void k_distinct_small(DistinctParams P)
{
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * (DS_T / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (g >= P.npoints) return;                                               // (whole waves; the kernel has no barrier)
    const int o = __builtin_amdgcn_readfirstlane(P.off[g]), n = __builtin_amdgcn_readfirstlane(P.off[g + 1]) - o;
    if (n > DS_SMALL_MAX) return;                                             // k_distinct_large's
    if (n <= 0) { if (lane == 0) { int2 r; r.x = -1; r.y = -1; P.out[g] = r; } return; }
    uint4 a = {0u, 0u, 0u, 0u}, b = a;
    if (lane < n) { const uint4* p = P.desc + (size_t)(o + lane) * 2; a = p[0]; b = p[1]; }
    const int v[8] = {(int)a.x, (int)a.y, (int)a.z, (int)a.w, (int)b.x, (int)b.y, (int)b.z, (int)b.w};
    // row `lane` of the table, one register per column (every index below is a constant once the loops are unrolled); columns from n on hold 512 and
    // never count.  Eight columns at a time, so that a group of a few descriptors does not pay for 64.
    int d[DS_SMALL_MAX];
#pragma unroll
    for (int j = 0; j < DS_SMALL_MAX; j++) d[j] = 512;
#pragma unroll
    for (int c = 0; c < DS_SMALL_MAX / 8; c++)
        if (c * 8 < n) {
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int j = c * 8 + u;
                int s = 0;
#pragma unroll
                for (int q = 0; q < 8; q++) s += __popc((unsigned)(v[q] ^ __builtin_amdgcn_readlane(v[q], j)));
                d[j] = j < n ? s : 512;
            }
        }
    // vDists[0.5*(N-1)] of the sorted row = its k-th smallest value x: the largest v with #(d < v) <= k (v = x + 1 already counts k + 1)
    const int k = (n - 1) >> 1;
    int med = 0;
#pragma unroll 1
    for (int bit = 256; bit; bit >>= 1) {
        const int cand = med + bit;
        int cnt = 0;
#pragma unroll
        for (int c = 0; c < DS_SMALL_MAX / 8; c++)
            if (c * 8 < n) {
#pragma unroll
                for (int u = 0; u < 8; u++) cnt += d[c * 8 + u] < cand;
            }
        if (cnt <= k) med = cand;
    }
    // median < BestMedian in row order: the least median, and among equal ones the first row
    int key = lane < n ? (med << 6 | lane) : 0x7fffffff;
    for (int m = 32; m; m >>= 1) { const int t = __shfl_xor(key, m); key = t < key ? t : key; }
    if (lane == 0) { int2 r; r.x = key & 63; r.y = key >> 6; P.out[g] = r; }
}

// the wavefront's LDS accesses before this point are done before those after it (LDS serves one wavefront's instructions in order; this keeps the compiler from reordering them)
__device__ __forceinline__ void distinct_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// rows w, w + 4, ... of one group by wavefront w: lo[j] | hi[j] is descriptor j (LDS planes, or the group's own place in global memory with stride 2)
template <int STRIDE, typename Ptr> __device__ __forceinline__ unsigned long long distinct_rows(Ptr lo, Ptr hi, int n, int w, int lane, int* hist)
{
    const int k = (n - 1) >> 1;
    unsigned long long best = ~0ull;
    for (int i = w; i < n; i += DL_T / 64) {
        const uint4 a0 = lo[(size_t)i * STRIDE], a1 = hi[(size_t)i * STRIDE];
        for (int j = lane; j < n; j += 64) atomicAdd(&hist[distinct_distance(a0, a1, lo[(size_t)j * STRIDE], hi[(size_t)j * STRIDE])], 1);
        distinct_wave_sync();
        // lane l owns bins 4l .. 4l+3; bin 256 (complementary descriptors) is what remains above them
        const int4 h = *reinterpret_cast<const int4*>(hist + 4 * lane);
        const int s = h.x + h.y + h.z + h.w;
        int incl = s;
        for (int m = 1; m < 64; m <<= 1) { const int t = __shfl_up(incl, m); if (lane >= m) incl += t; }
        const unsigned long long reached = __ballot(incl > k);                // lanes at or behind the bin that holds rank k
        int med = 256;
        if (reached) {
            int c = incl - s + h.x, bin = 4 * lane;
            if (c <= k) { c += h.y; bin++; if (c <= k) { c += h.z; bin++; if (c <= k) bin++; } }
            med = __shfl(bin, __ffsll((long long)reached) - 1);
        }
        int4 z; z.x = z.y = z.z = z.w = 0;
        *reinterpret_cast<int4*>(hist + 4 * lane) = z;
        if (lane == 0) hist[256] = 0;
        distinct_wave_sync();
        const unsigned long long key = (unsigned long long)med << 32 | (unsigned)i;
        best = key < best ? key : best;
    }
    return best;
}

__global__ __launch_bounds__(DL_T) void k_distinct_large(DistinctParams P)
{
    HIP_DYNAMIC_SHARED(uint4, s_desc)                                         // [2][n]: first and second half of every descriptor (n <= DL_STAGE_MAX)
    __shared__ __attribute__((aligned(16))) int s_hist[DL_T / 64][DL_HSTRIDE];
    __shared__ unsigned long long s_best;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = P.large[blockIdx.x];
    const int o = P.off[g], n = P.off[g + 1] - o;
    const uint4* gd = P.desc + (size_t)o * 2;
    const bool staged = n <= DL_STAGE_MAX;
    if (staged) for (int t = tid; t < 2 * n; t += DL_T) s_desc[(t & 1) * n + (t >> 1)] = gd[t];
    for (int b = lane; b < DL_HSTRIDE; b += 64) s_hist[w][b] = 0;
    if (tid == 0) s_best = ~0ull;
    __syncthreads();
    const unsigned long long best = staged ? distinct_rows<1>(s_desc, s_desc + n, n, w, lane, s_hist[w])
                                           : distinct_rows<2>(gd, gd + 1, n, w, lane, s_hist[w]);
    if (lane == 0) atomicMin(&s_best, best);                                  // (the same value in every lane: the wave has reduced it)
    __syncthreads();
    if (tid == 0) { int2 r; r.x = (int)(s_best & 0xffffffffu); r.y = (int)(s_best >> 32); P.out[g] = r; }
}

// ---------------------------------------------------------------------------------------------- host
extern "C" orbhip_status orbhip_distinctive_descriptors(int device, const uint8_t* desc, const int32_t* offsets, int npoints, int32_t* best_index, int32_t* best_median)
{
    OrbApiTimer api_timer;
    if (npoints == 0) return ORBHIP_OK;
    if (npoints < 0 || !offsets || !best_index) return fail(ORBHIP_ERR_INVALID, "bad argument");
    if (offsets[0] != 0) return fail(ORBHIP_ERR_INVALID, "offsets[0] is %d, not 0", offsets[0]);
    std::vector<int> large; int stage = 0;
    for (int g = 0; g < npoints; g++) {
        const long long n = (long long)offsets[g + 1] - offsets[g];
        if (n < 0) return fail(ORBHIP_ERR_INVALID, "offsets decrease at group %d (%d after %d)", g, offsets[g + 1], offsets[g]);
        if (n > DS_SMALL_MAX) { large.push_back(g); if (n <= DL_STAGE_MAX) stage = std::max(stage, (int)n); }
    }
    const size_t total = (size_t)offsets[npoints], nlarge = large.size();
    if (total > 0 && !desc) return fail(ORBHIP_ERR_INVALID, "bad argument");
    if (!device_present()) return fail(ORBHIP_ERR_HIP, "no HIP device available: no CPU fallback");
    HIPCHK(hipSetDevice(device));
    const hipStream_t s = orbhip_thread_stream(device);
    std::vector<int2> out(npoints);
    uint8_t* dd = nullptr; int *doff = nullptr, *dlarge = nullptr; int2* dout = nullptr;
    const hipError_t e = arena_call(device, s, [&](Arena& A) {
        A.io(&dd, total * 32, desc, total * 32);
        A.io(&doff, (size_t)npoints + 1, (const int*)offsets, (size_t)npoints + 1);
        A.io(&dlarge, nlarge, (const int*)large.data(), nlarge);
        A.io(&dout, (size_t)npoints, (const int2*)nullptr, 0, out.data(), (size_t)npoints);
    }, [&] {
        DistinctParams P; P.desc = reinterpret_cast<const uint4*>(dd); P.off = doff; P.npoints = npoints; P.large = dlarge; P.out = dout;
        hipLaunchKernelGGL(k_distinct_small, dim3((npoints + DS_T / 64 - 1) / (DS_T / 64), 1, 1), dim3(DS_T, 1, 1), 0, s, P);
        if (nlarge) hipLaunchKernelGGL(k_distinct_large, dim3((unsigned)nlarge, 1, 1), dim3(DL_T, 1, 1), (size_t)std::max(stage, 1) * 32, s, P);
    });
    if (e != hipSuccess) return fail(ORBHIP_ERR_HIP, "distinctive_descriptors: %s", hipGetErrorString(e));
    for (int g = 0; g < npoints; g++) { best_index[g] = out[g].x; if (best_median) best_median[g] = out[g].y; }
    return ORBHIP_OK;
}
