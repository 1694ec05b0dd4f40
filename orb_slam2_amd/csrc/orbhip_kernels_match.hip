// orbhip_kernels_match.hip — gfx950 kernels of the matcher side (replaces the Hamming / Frame-to-Frame part of
// src/ORBmatcher.cc and the Frame feature grid it reads).
//
//   k_hamming_nn / k_hamming_merge   brute-force 256-bit Hamming NN, queries in registers, DB rows broadcast from LDS,
//                                    __popcll on 4 x u64 per pair (ORBmatcher::DescriptorDistance, ORBmatcher.cc:1647-1663;
//                                    best/second idiom :102-114, :447-456).  Integer-VALU bound (v_xor + v_bcnt); small databases.
//   k_hamming_nn_fp4b                the same scan as +-1 FP4 products on the matrix cores (databases from 32 K rows on)
//   k_match_grid                     Frame::AssignFeaturesToGrid (Frame.cc:230-245, 382-392): 64x48 buckets, keypoint order
//   k_match_candidates               Frame::GetFeaturesInArea (Frame.cc:327-380) in canonical order + all Hamming distances,
//                                    a row of 16 lanes per previous-frame keypoint, four key points per wavefront; also records each
//                                    key point's four best candidates.  A candidate is named by its position in the bucket table.
//   k_match_select                   the order-dependent part of SearchForInitialization (ORBmatcher.cc:418-517): one
//                                    wavefront (= workgroup) per camera slot decides 64 key points per step from those records (a
//                                    candidate is skipped once matched at a distance <= the query's), rescans the rare key point whose
//                                    records are used up, then rotation histogram, ComputeThreeMaxima (:1601-1642), vbPrevMatched update.
//                                    Per-feature tables by table position: 2 x level-0 key points of F2 + level-0 key points of F1 words.
#include "orbhip_internal.h"
#include <cstdlib>
#include <cstring>
#include <type_traits>

#define WAVE 64
#define IMAX 0x7fffffff

// ------------------------------------------------------------------------------------------------ brute-force NN
#define NN_T 256
#define NN_QPT 4                       // queries held in registers per thread
#define NN_ROWS 256                    // DB rows staged in LDS per step (8 KB)
#define NN_CHUNK 8192                  // DB rows per workgroup

struct NNPart { int best, second; long long idx; };

__global__ __launch_bounds__(NN_T) void k_hamming_nn(const unsigned long long* q, int nq, const unsigned long long* db, long long ndb,
                                                     long long base, NNPart* parts, int nchunks)
{
    __shared__ unsigned long long s_db[NN_ROWS * 4];
    const int tid = threadIdx.x, chunk = blockIdx.y;
    const int q0 = (blockIdx.x * NN_T + tid) * NN_QPT;
    unsigned long long qa[NN_QPT][4];
    // per query: the two smallest keys (distance << 13 | row-in-chunk).  Keys are unique and ordered like (distance, index), so
    //   best' = min(best, x);  second' = min(second, max(best, x))
    // is exactly the matcher's `if (d < best) {second = best; best = d;} else if (d < second) second = d` with lowest-index ties.
    unsigned kb[NN_QPT], ks[NN_QPT];
#pragma unroll
    for (int k = 0; k < NN_QPT; k++) {
        const int qi = min(q0 + k, nq - 1);
#pragma unroll
        for (int w = 0; w < 4; w++) qa[k][w] = q[(long long)qi * 4 + w];
        kb[k] = 0xffffffffu; ks[k] = 0xffffffffu;
    }
    const long long row0 = (long long)chunk * NN_CHUNK;
    const long long row1 = min(row0 + (long long)NN_CHUNK, ndb);
    for (long long r = row0; r < row1; r += NN_ROWS) {
        const int nr = (int)min((long long)NN_ROWS, row1 - r);
        __syncthreads();
        for (int i = tid; i < nr * 4; i += NN_T) s_db[i] = db[r * 4 + i];
        __syncthreads();
        const unsigned jbase = (unsigned)(r - row0);
        for (int j = 0; j < nr; j++) {
            const unsigned long long d0 = s_db[4 * j], d1 = s_db[4 * j + 1], d2 = s_db[4 * j + 2], d3 = s_db[4 * j + 3];   // LDS broadcast
#pragma unroll
            for (int k = 0; k < NN_QPT; k++) {
                const unsigned d = (unsigned)(__popcll(qa[k][0] ^ d0) + __popcll(qa[k][1] ^ d1) + __popcll(qa[k][2] ^ d2) + __popcll(qa[k][3] ^ d3));
                const unsigned x = (d << 13) | (jbase + j);
                ks[k] = min(ks[k], max(kb[k], x));
                kb[k] = min(kb[k], x);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NN_QPT; k++)
        if (q0 + k < nq) {
            NNPart p;
            p.best = kb[k] == 0xffffffffu ? IMAX : (int)(kb[k] >> 13);
            p.second = ks[k] == 0xffffffffu ? IMAX : (int)(ks[k] >> 13);
            p.idx = kb[k] == 0xffffffffu ? -1 : row0 + (long long)(kb[k] & 0x1fffu) + base;
            parts[(long long)(q0 + k) * nchunks + chunk] = p;
        }
}

// ---- the same scan on the FP4 matrix path (gfx950: v_mfma_scale_f32_32x32x64_f8f6f4).  With descriptor bits as +-1, <a, b> = 256 - 2 * Hamming(a, b), and
// +-1 is exact in E2M1 (+1 = 0x2, -1 = 0xA; bit k of a byte -> nibble k: s_tab).  A descriptor is 256 nibbles = 8 x 16 bytes, a tile of 32 DB rows 4 KB:
// [dword d of the row = 2 kb + h][row i] x 16 bytes.  Lane (j, h) of a wave holds query j of a 32-query tile as B operands, K block kb = dword 2 kb + h of
// the query, with the SAME sign as the rows (set bit -> +1), and reads row j of the tile as A operands, the same dwords.  The rows' block scale is 2^0
// (E8M0 127), the queries' 2^6 (133): a matching bit contributes +64, a differing one -64, and with C = 0 an accumulator is the similarity
// sim = 64 (256 - 2 d) = 16384 - 128 d  of (row, query) - an integer of magnitude <= 2^14, exact in f32.  The result leaves with lane = query, register reg =
// DB row (reg & 3) + 8 (reg >> 2) + 4 h of the tile.
// KEYS.  A kept (tile, query tile) turns its similarities into the keys  d << 7 | row-in-tile = 16384 + row - sim  as floats.  Positive floats order like
// their bit patterns: the v_min3 / v_med3 tournament runs on the raw registers and only the two winners are converted, into chunk keys
// d << LCH | row-in-chunk, and merged into the query's running pair  second = min(second, max(best, key)), best = min(best, key)  exactly as in
// k_hamming_nn, whose partial format and merge kernel are reused.  THRESHOLD: a tile matters to a query only if it holds a similarity ABOVE thr[t], i.e. a
// distance strictly below the running second best - a later row at that distance has a larger key than it (rows ascend).
typedef int nn_v4i __attribute__((vector_size(16)));
typedef int nn_v8i __attribute__((vector_size(32)));
typedef float nn_v16f __attribute__((vector_size(64)));
// SEEDED SCAN.  A query's FINAL second-best distance is at most the second-best distance over ANY subset of the rows; seed[q] (nullptr: none) carries that
// bound from a first pass over the database's head (rows 0 .. 2^15, k_hamming_seed).  A workgroup whose rows all lie BEHIND the head starts its threshold
// at the bound instead of at "nothing seen yet": a tile can only matter if it holds a distance strictly below the bound (a row AT the bound loses the tie
// to the head's rows, which have lower indices) - so the skip works from a chunk's first tile on.
// EXP: `db` is the database EXPANDED in device memory (k_nn_expand: 128 B per row, 4 KB per tile of 32 rows in exactly the layout of the LDS tile), so
// staging a tile is ONE 16-byte LDS-DMA per thread - no registers, no byte -> E2M1 table, no VALU - requested a whole superstep ahead.  Without it the
// rows are loaded a superstep ahead and expanded through s_tab into LDS just before the barrier.
// HAND-ORDERED SUPERSTEP.  Left to itself hipcc gathers the sixteen matrix instructions of a tile back to back, with the threshold tests and the tile's
// operand reads (+ their lgkmcnt(0)) in front of them, so a wave's matrix pipe idles while it tests and waits.  Here a whole superstep of NN_FP4B_TPB tiles
// is ONE asm statement whose text is generated (tools/gen_nn_fp4_block.py -> nn_fp4_block.inc): matrix instruction, two or three v_max3_f32 of a tile
// finished long before, matrix instruction, ...; the next tile's operands are read a half tile ahead.  The statement owns its accumulators (registers it
// clobbers), so nothing of a tile outlives it except ONE scalar: bit 8 t + u = tile u may matter to query tile t.  Those rare pairs are recomputed - four
// matrix instructions - and folded in by compiled code behind the statement, while the superstep's tiles are still in LDS.  A threshold is therefore up
// to one superstep stale: it only ever keeps more, never fewer.  Partial supersteps and the ragged tile take the compiled per-tile path.  hipcc must NOT
// spill across the statement: a reload in front of it comes with `s_waitcnt vmcnt(0)`, i.e. waits for the prefetch issued just before - hence one
// tile-operand set, the lane's LDS address and the scales made inside the statement, and addresses rebuilt at their (rare) uses instead of kept (check:
// no scratch_ access between the loop's barriers).
#include "nn_fp4_block.inc"
#define NN_SHARE_EVERY 16                // supersteps between two reads of the shared bounds (a power of two)
// SHARED BOUNDS.  `share` (nullptr: none) = two words per query: share[q] the smallest, share[nq + q] the second smallest distance among the head's best
// pair (k_hamming_seed) and EVERY row any workgroup has found below its threshold since.  A row at distance d is OFFERED with two non-returning atomics,
// atomicMin(best, d) and atomicMin(second, max(d, b)), b = the best as last read by the offering lane: b is the distance of some OTHER row, so max(d, b) is
// at least the second smallest of two real rows - `second` never falls below the final second-best distance.  (The exact exchange
// `old = atomicMin(best, d); atomicMin(second, max(old, d))` was built first: its returned value is a round trip of microseconds in front of the
// workgroup's barrier and cost more than the bounds won.)  A tile whose distances all EXCEED some second best S holds neither the final best, nor the
// final second best, nor a row tied with either - whichever rows S came from - so S + 1 is a threshold for everybody.  A workgroup re-reads the pair of
// its queries every NN_SHARE_EVERY-th superstep by LDS-DMA with sc1 (device scope: a plain load is served from the reading XCD's L2, which the other
// XCDs' atomics never reach), requested at a superstep's start and taken behind its barrier: the thresholds follow the best pair found ANYWHERE.  Under
// the head's bound alone one (tile, query tile) in twenty-three is kept and recomputed, with the shared bounds one in five hundred.  The filter only
// decides which tiles are looked at: the answers do not depend on the order the workgroups run in (tests/test_parity_match.py:
// test_brute_force_nn_ties_across_chunks).
template <int LCH, bool EXP> __global__ __launch_bounds__(256, 2) void k_hamming_nn_fp4b(const unsigned* q, int nq, const unsigned* db, long long ndb, long long base, NNPart* parts, int nchunks,
                                                                                     const int* seed, int* share, long long rows0, int chrows, int part0)
{
    constexpr int QT = 4, TPB = NN_FP4B_TPB;
    static_assert(TPB <= 8, "the keep mask has eight bits per query tile");
    __shared__ unsigned s_tab[256];                                    // byte -> its 8 bits as E2M1 nibbles (bit k -> nibble k): set = +1 (0x2), clear = -1 (0xA)
    __shared__ __attribute__((aligned(16))) unsigned s_a[2][TPB * 1024];   // the superstep's TPB tiles, double-buffered
    __shared__ int s_bnd[4][2 * QT][64];                               // the queries' shared pairs as last read: [wave][t] the second best, [wave][QT + t] the best
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bx = blockIdx.x, by = blockIdx.y;
    {
        unsigned e = 0;
#pragma unroll
        for (int t = 0; t < 8; t++) e |= (((tid >> t) & 1) ? 0x2u : 0xAu) << (4 * t);
        s_tab[tid] = e;
    }
    __syncthreads();
    const int j = lane & 31, h = lane >> 5;
    constexpr int QG = 4 * QT * 32;
    nn_v4i B[QT][4];
    int qidx[QT];
#pragma unroll
    for (int t = 0; t < QT; t++) {
        qidx[t] = bx * QG + (wave * QT + t) * 32 + j;
        const unsigned* qp = q + (long long)min(qidx[t], nq - 1) * 8;
#pragma unroll
        for (int kb = 0; kb < 4; kb++) {
            const unsigned w = qp[2 * kb + h];
            B[t][kb] = nn_v4i{(int)s_tab[w & 0xff], (int)s_tab[(w >> 8) & 0xff], (int)s_tab[(w >> 16) & 0xff], (int)s_tab[w >> 24]};
        }
    }
    unsigned kbest[QT], ksec[QT]; float thr[QT];
#pragma unroll
    for (int t = 0; t < QT; t++) {
        kbest[t] = 0xffffffffu; ksec[t] = 0xffffffffu; thr[t] = -3.0e38f;
        if (seed) { const int sd2 = seed[min(qidx[t], nq - 1)]; if (sd2 >= 0 && sd2 <= 256) thr[t] = (float)(16384 - 128 * sd2); }
    }
    int* const bound = share;
    auto bounds_request = [&]() {      // (aux 16 = sc1: device-scope reads - a plain one is served from this XCD's L2, which the other XCDs' atomics never reach)
#pragma unroll
        for (int t = 0; t < QT; t++) {
            int qc = min(qidx[t], nq - 1);
            asm volatile("" : "+v"(qc));                               // (rebuilt at every request: as eight loop-invariant pointers the addresses were spilled around the superstep)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(share + nq + qc), (__attribute__((address_space(3))) void*)&s_bnd[wave][t][0], 4, 0, 16);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(share + qc), (__attribute__((address_space(3))) void*)&s_bnd[wave][QT + t][0], 4, 0, 16);
        }
    };
    auto bounds_take = [&]() {
#pragma unroll
        for (int t = 0; t < QT; t++) { const int sd2 = s_bnd[wave][t][lane]; if (sd2 >= 0 && sd2 <= 256) thr[t] = fmaxf(thr[t], (float)(16384 - 128 * (sd2 + 1))); }
    };
    constexpr int CH = 1 << LCH;
    // rows [rows0 + by * chrows, + chrows) are this workgroup's: chrows <= CH (the keys pack a row-in-chunk into LCH bits) and a multiple of 32 (tiles of the
    // expanded database); the launcher sizes it so that the launch fills the chip's workgroup slots a whole number of times (below)
    const long long row0 = rows0 + (long long)by * chrows;
    const int nrows = (int)min((long long)chrows, ndb - row0);
    const int ntiles = (nrows + 31) >> 5;
    const int sr = tid & 31, sd = tid >> 5;                            // staging role: row sr of the tile, dword sd of that row
    unsigned wnext[TPB];
    auto fetch = [&](int sup) {
#pragma unroll
        for (int u = 0; u < TPB; u++) { const int r = (sup * TPB + u) * 32 + sr; wnext[u] = r < nrows ? db[(row0 + r) * 8 + sd] : 0u; }
    };
    auto expand = [&](int buf) {
#pragma unroll
        for (int u = 0; u < TPB; u++) {
            const unsigned w = wnext[u];
            *reinterpret_cast<uint4*>(s_a[buf] + u * 1024 + (sd * 32 + sr) * 4) = uint4{s_tab[w & 0xff], s_tab[(w >> 8) & 0xff], s_tab[(w >> 16) & 0xff], s_tab[w >> 24]};
        }
    };
    auto stage_dma = [&](int sup, int buf) {                           // thread tid: bytes [16 tid, 16 tid + 16) of each 4 KB tile (wave w: the tile's w-th KB)
#pragma unroll
        for (int u = 0; u < TPB; u++) {
            const int tile = sup * TPB + u;
            if (tile < ntiles)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(db + ((row0 >> 5) + tile) * 1024 + tid * 4),
                                                 (__attribute__((address_space(3))) void*)(s_a[buf] + u * 1024 + wave * 256), 16, 0, 0);
        }
    };
    const nn_v16f czero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const float off_h = (float)(4 * h);
    auto top2_of3 = [](unsigned a, unsigned b, unsigned c, unsigned& lo, unsigned& mid) { lo = min(min(a, b), c); mid = max(min(a, b), min(max(a, b), c)); };
    auto merge2 = [](unsigned& b, unsigned& s2, unsigned ob, unsigned os) { s2 = min(min(s2, os), max(b, ob)); b = min(b, ob); };
    // the similarities of one (tile, query tile): four matrix instructions (compiled: the kept pairs and the per-tile path)
    auto products1 = [&](const unsigned* ta, const nn_v4i (&b)[4]) -> nn_v16f {
        nn_v16f d = czero;
#pragma unroll
        for (int kb = 0; kb < 4; kb++) {      // (A, B, C, format of A = FP4, format of B = FP4, scale A: byte 0 of 127 = 2^0, scale B: byte 0 of 133 = 2^6)
            const uint4 a4 = *reinterpret_cast<const uint4*>(ta + ((2 * kb + h) * 32 + j) * 4);
            d = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(nn_v8i{(int)a4.x, (int)a4.y, (int)a4.z, (int)a4.w, 0, 0, 0, 0}, nn_v8i{b[kb][0], b[kb][1], b[kb][2], b[kb][3], 0, 0, 0, 0}, d, 4, 4, 0, 127, 0, 133);
        }
        return d;
    };
    // the threshold test of one query tile: does ANY lane see a similarity above its threshold in this tile?  (eight v_max3_f32, a compare, a ballot)
    auto test1 = [&](int t, const nn_v16f& x) -> bool {
        const float m0 = fmaxf(fmaxf(x[0], x[1]), x[2]), m1 = fmaxf(fmaxf(x[3], x[4]), x[5]), m2 = fmaxf(fmaxf(x[6], x[7]), x[8]), m3 = fmaxf(fmaxf(x[9], x[10]), x[11]), m4 = fmaxf(fmaxf(x[12], x[13]), x[14]);
        const float mx = fmaxf(fmaxf(fmaxf(m0, m1), m2), fmaxf(fmaxf(m3, m4), x[15]));
        return __ballot(mx > thr[t]) != 0;
    };
    // a kept (tile, query tile): keys, tournament, the running pair and threshold (KEYS above); `ragged`: rows past the end get distance 511 and lose
    auto tournament1 = [&](int tile, int t, const nn_v16f& a, bool ragged) {
        const unsigned tbase = (unsigned)tile * 32u;
        unsigned x[16];
#pragma unroll
        for (int reg = 0; reg < 16; reg++) {
            const int rbase = (reg & 3) + 8 * (reg >> 2);
            x[reg] = __float_as_uint(((float)(16384 + rbase) - a[reg]) + off_h);
            if (ragged && tile * 32 + rbase + 4 * h >= nrows) x[reg] = __float_as_uint((float)((511 << 7) + rbase) + off_h);
        }
        unsigned b, s2;
        top2_of3(x[0], x[1], x[2], b, s2);
#pragma unroll
        for (int g = 1; g < 5; g++) { unsigned lo, mid; top2_of3(x[3 * g], x[3 * g + 1], x[3 * g + 2], lo, mid); merge2(b, s2, lo, mid); }
        merge2(b, s2, x[15], 0x7f7fffffu);                                                                  // (the largest finite float's bits: loses to every key)
        const unsigned bi = (unsigned)__uint_as_float(b), si = (unsigned)__uint_as_float(s2);               // the two winners back to integers: d << 7 | r
        const unsigned kb1 = ((bi >> 7) << LCH) + (bi & 127u) + tbase, ks1 = ((si >> 7) << LCH) + (si & 127u) + tbase;      // chunk keys d << LCH | (tile * 32 + r)
        if (share && qidx[t] < nq) {
            // this lane's two best rows of the tile, offered if they beat its threshold (SHARED BOUNDS above): b = the best AS LAST READ, or the tile's other row
            const int d1 = (int)(bi >> 7), d2 = (int)(si >> 7), bstar = s_bnd[wave][QT + t][lane];
            int qc = qidx[t];
            asm volatile("" : "+v"(qc));
            if (d1 <= 256 && (float)(16384 - 128 * d1) > thr[t]) { atomicMin(share + qc, d1); atomicMin(share + nq + qc, max(d1, bstar)); }
            if (d2 <= 256 && (float)(16384 - 128 * d2) > thr[t]) atomicMin(share + nq + qc, d2);                 // (the tile's other row is no farther)
        }
        merge2(kbest[t], ksec[t], kb1, ks1);
        // (a never-set second best gives a threshold below every similarity; a seeded threshold is never lowered)
        thr[t] = fmaxf(thr[t], 16384.0f - 128.0f * (float)(ksec[t] >> LCH));
    };
    // one whole superstep: which (tile u, query tile t) hold a similarity above the query tile's threshold - bit 8 t + u
    auto superstep = [&](const unsigned* ta) -> unsigned {
#if defined(__HIP_DEVICE_COMPILE__) && __HIP_DEVICE_COMPILE__
        unsigned keep, stmp;
        const unsigned addr = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long long)(__attribute__((address_space(3))) const void*)ta);
        asm volatile(NN_FP4B_BODY
                     : "=&s"(keep), "=&s"(stmp)
                     : "v"(B[0][0]), "v"(B[0][1]), "v"(B[0][2]), "v"(B[0][3]), "v"(B[1][0]), "v"(B[1][1]), "v"(B[1][2]), "v"(B[1][3]),
                       "v"(B[2][0]), "v"(B[2][1]), "v"(B[2][2]), "v"(B[2][3]), "v"(B[3][0]), "v"(B[3][1]), "v"(B[3][2]), "v"(B[3][3]),
                       "v"(thr[0]), "v"(thr[1]), "v"(thr[2]), "v"(thr[3]), "s"(addr)
                     : "memory", "vcc", "scc", NN_FP4B_CLOBBERS);
        return keep;
#else
        unsigned keep = 0;                                            // (the CPU emulation of the test suite: the same mask from the compiled pieces)
        for (int u = 0; u < TPB; u++)
            for (int t = 0; t < QT; t++) if (test1(t, products1(ta + u * 1024, B[t]))) keep |= 1u << (8 * t + u);
        return keep;
#endif
    };
    if (bound) bounds_request();                                       // what the others have found so far, with the first tiles
    if constexpr (EXP) stage_dma(0, 0); else { fetch(0); expand(0); }
    __builtin_amdgcn_s_waitcnt(0x0f70);                                // (vmcnt(0))
    __syncthreads();
    if (bound) bounds_take();
    const int nfull = nrows >> 5, nsuper = (ntiles + TPB - 1) / TPB;
    bool pending = false;
    for (int sup = 0; sup < nsuper; sup++) {
        const int buf = sup & 1, tile0 = sup * TPB;
        if (pending) bounds_take();                                                                         // (requested at the start of the superstep before, landed before its barrier)
        pending = false;
        if (sup + 1 < nsuper) { if constexpr (EXP) stage_dma(sup + 1, buf ^ 1); else fetch(sup + 1); }      // (everybody left that buffer at the barrier of the superstep before)
        // every NN_SHARE_EVERY-th superstep, the workgroups out of step with each other: the reads are device-scope (they go past the L2) and all workgroups of a
        // query group read the same few lines - once per superstep they queued on those lines' memory channel (5.1 ms against 3.3 for the scan without them)
        if (bound && sup + 1 < nsuper && ((sup + by) & (NN_SHARE_EVERY - 1)) == 0) { bounds_request(); pending = true; }
        if (tile0 + TPB <= nfull) {                                                                         // a superstep of whole tiles: the hand-ordered statement
            const unsigned keep = superstep(s_a[buf]);
            if (__builtin_expect(keep != 0, 0))                                                             // (rare: the hint keeps hipcc from spilling around the statement)
#pragma unroll
            for (int t = 0; t < QT; t++) {
                unsigned m = (keep >> (8 * t)) & 0xffu;
                while (m) {
                    const int u = __builtin_ctz(m); m &= m - 1;
                    tournament1(tile0 + u, t, products1(s_a[buf] + u * 1024, B[t]), false);
                }
            }
        } else {
            for (int u = 0; u < TPB; u++) {
                const int tile = tile0 + u;
                if (tile >= ntiles) break;
#pragma unroll
                for (int t = 0; t < QT; t++) {
                    const nn_v16f d = products1(s_a[buf] + u * 1024, B[t]);
                    if (tile >= nfull || test1(t, d)) tournament1(tile, t, d, tile >= nfull);
                }
            }
        }
        if (sup + 1 < nsuper) { if constexpr (!EXP) expand(buf ^ 1); __builtin_amdgcn_s_waitcnt(0x0f70); }      // (vmcnt(0): the next tiles and the bounds have landed)
        __syncthreads();
    }
#pragma unroll
    for (int t = 0; t < QT; t++) {      // a query's rows were split over its two lanes (j, 0) and (j, 1): fold, then one partial per (query, chunk)
        const unsigned ob = (unsigned)__shfl_xor((int)kbest[t], 32), os = (unsigned)__shfl_xor((int)ksec[t], 32);
        const unsigned b = min(kbest[t], ob), s2 = min(min(ksec[t], os), max(kbest[t], ob));
        if (h == 0 && qidx[t] < nq) {
            NNPart p;
            p.best = (b >> LCH) > 256u ? IMAX : (int)(b >> LCH);       // never-set keys and the ragged tile's filler rows carry a distance above 256
            p.second = (s2 >> LCH) > 256u ? IMAX : (int)(s2 >> LCH);
            p.idx = (b >> LCH) > 256u ? -1 : row0 + (long long)(b & (unsigned)(CH - 1)) + base;
            parts[(long long)qidx[t] * nchunks + part0 + by] = p;
        }
    }
}
// The database as the FP4 scan reads it (orbhip_nn_expand_device): tile T = rows 32 T .. 32 T + 31 as 4 KB, [dword d of the row][row i] x 16 bytes = the eight
// E2M1 nibbles of each of the dword's four bytes - byte for byte what k_hamming_nn_fp4b's `expand` writes into LDS from the bit form.  Rows past the end: zeros (never a winner:
// the scan's ragged tile masks them).  One thread per (tile, d, i).
__global__ __launch_bounds__(256) void k_nn_expand(const unsigned* db, long long ndb, uint4* out, long long ntiles)
{
    __shared__ unsigned s_tab[256];
    {
        unsigned e = 0;
#pragma unroll
        for (int t = 0; t < 8; t++) e |= (((threadIdx.x >> t) & 1) ? 0x2u : 0xAu) << (4 * t);
        s_tab[threadIdx.x] = e;
    }
    __syncthreads();
    const long long tile = blockIdx.x;
    if (tile >= ntiles) return;
    const int i = threadIdx.x & 31, d = threadIdx.x >> 5;
    const long long row = tile * 32 + i;
    const unsigned w = row < ndb ? db[row * 8 + d] : 0u;
    out[tile * 256 + d * 32 + i] = row < ndb ? uint4{s_tab[w & 0xff], s_tab[(w >> 8) & 0xff], s_tab[(w >> 16) & 0xff], s_tab[w >> 24]} : uint4{0u, 0u, 0u, 0u};
}
size_t orbhip_nn_expanded_bytes(long long ndb) { return (size_t)((ndb + 31) / 32) * 4096; }
void orbhip_launch_nn_expand(const uint8_t* d_db, long long ndb, uint8_t* d_out, hipStream_t s)
{
    const long long ntiles = (ndb + 31) / 32;
    if (ntiles > 0) hipLaunchKernelGGL(k_nn_expand, dim3((unsigned)ntiles, 1, 1), dim3(256, 1, 1), 0, s, (const unsigned*)d_db, ndb, (uint4*)d_out, ntiles);
}

// second-best distance over the head's partials of every query: the seed of the main pass (a head with fewer than two rows in reach gives none)
__global__ __launch_bounds__(256) void k_hamming_seed(const NNPart* parts, int nq, int stride, int nhead, int* seed, int* share)
{   // share (nullptr: none): the shared best / second-best pair of k_hamming_nn_fp4b starts as the head's.
    // One wavefront per query, a lane per head partial (one thread per query walked its 64 partials one load latency after the other: 30 us of a 3.7 ms query)
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int qi = blockIdx.x * 4 + wave;
    if (qi >= nq) return;
    int b = IMAX, s2 = IMAX;
    for (int c = lane; c < nhead; c += 64) { const NNPart p = parts[(long long)qi * stride + c]; s2 = min(min(s2, p.second), max(b, p.best)); b = min(b, p.best); }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {                 // the two smallest of the union: only the distances matter here, not which row
        const int ob = __shfl_xor(b, off), os = __shfl_xor(s2, off);
        s2 = min(min(s2, os), max(b, ob)); b = min(b, ob);
    }
    if (lane == 0) {
        seed[qi] = s2 == IMAX ? -1 : s2;
        if (share) { share[qi] = b == IMAX ? (1 << 20) : b; share[nq + qi] = s2 == IMAX ? (1 << 20) : s2; }      // (none: above every distance, and atomicMin can still lower it)
    }
}

// fold the per-chunk partials of one query in ascending DB order: stable arg-min + second smallest of the multiset
__device__ __forceinline__ void nn_combine(int& b, long long& i, int& s, int rb, long long ri, int rs)
{
    if (rb < b) { s = min(b, rs); b = rb; i = ri; } else { s = min(s, rb); }
}
__global__ __launch_bounds__(256) void k_hamming_merge(const NNPart* parts, int nq, int nchunks, long long* best_idx, int* best_dist, int* second_dist)
{
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int qi = blockIdx.x * 4 + wave;
    if (qi >= nq) return;
    int b = IMAX, s = IMAX; long long i = -1;
    const int per = (nchunks + 63) / 64;                     // contiguous runs per lane keep the index order
    for (int c = lane * per; c < min((lane + 1) * per, nchunks); c++) { const NNPart p = parts[(long long)qi * nchunks + c]; nn_combine(b, i, s, p.best, p.idx, p.second); }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {                 // lanes hold ascending index ranges; combine neighbours left-to-right
        const int rb = __shfl_down(b, off), rs = __shfl_down(s, off); const long long ri = __shfl_down(i, off);
        if (((lane & (2 * off - 1)) == 0) && lane + off < 64) nn_combine(b, i, s, rb, ri, rs);
    }
    if (lane == 0) { best_idx[qi] = i; best_dist[qi] = b; second_dist[qi] = s; }
}

// workspace for the partials lives in a small per-thread cache owned by the API layer

bool orbhip_launch_hamming_nn(const uint8_t* d_q, int nq, const uint8_t* d_db, long long ndb, long long base,
                              long long* d_best_idx, int* d_best_dist, int* d_second, hipStream_t s, const uint8_t* d_dbx)
{   // d_dbx: the same database expanded by orbhip_launch_nn_expand (nullptr: none) - taken by the FP4 scan
    if (nq <= 0) return true;
    const int nchunks = (int)max(1LL, (ndb + NN_CHUNK - 1) / NN_CHUNK);
    NNPart* parts = (NNPart*)orbhip_nn_workspace(sizeof(NNPart) * (size_t)nq * nchunks, s);
    if (!parts) return false;                                    // the caller reports it: results would be left unwritten
    // the matrix-core scan from a few chunks on (below that a call is latency, not throughput).  ORBHIP_NN=valu (measurement: tools/db_query_rate.py) keeps
    // the popcount kernel at any size; any other value names no form: the default scans, said once on stderr.  (Read per call: a scan is at least a
    // hundred microseconds, and tests switch forms inside one process.)
    const char* e = getenv("ORBHIP_NN");
    const bool valu = e && !strcmp(e, "valu");
    if (e && *e && !valu) {
        static bool said = false;
        if (!said) { said = true; fprintf(stderr, "orbhip: ORBHIP_NN=%s names no scan form (valu is the only one); the default scan is used\n", e); }
    }
    if (valu || ndb < 4 * NN_CHUNK) {
        const int qblocks = (nq + NN_T * NN_QPT - 1) / (NN_T * NN_QPT);
        hipLaunchKernelGGL(k_hamming_nn, dim3(qblocks, nchunks, 1), dim3(NN_T, 1, 1), 0, s, (const unsigned long long*)d_q, nq,
                           (const unsigned long long*)d_db, ndb, base, parts, nchunks);
        hipLaunchKernelGGL(k_hamming_merge, dim3((nq + 3) / 4, 1, 1), dim3(256, 1, 1), 0, s, (const NNPart*)parts, nq, nchunks, d_best_idx, d_best_dist, d_second);
        return true;
    }
    // The FP4 scan in two passes: the head = the first 2^15 rows as 64 sub-chunks of 512 rows (256 workgroups, sixteen tiles each - a chunk of 2^15 rows takes
    // ONE workgroup a millisecond); behind it, if the database is longer, k_hamming_seed merges the head's second-best distance per query into the bound the
    // main pass scans the rest of the database under.  Partials: [64 head sub-chunks][main chunks].
    constexpr long long head = 1LL << 15;
    const int qg = 4 * 4 * 32;                                   // queries per workgroup: four wavefronts of four query tiles
    int chrows = 1 << 15, nmain = 0;
    if (ndb > head) {
        // ROWS PER WORKGROUP of the main pass.  Every workgroup does the same work, so a launch runs in rounds of (2 x CUs) workgroups: 609 chunks of 2^15
        // rows x 4 query groups = 2436 workgroups on 512 slots took five rounds with the last one three quarters empty.  The rows behind the head are split
        // into the number of chunks that fills a whole number of rounds instead (a multiple of 256 rows, at most 2^15, at least 2048: a short database is
        // spread over the chip instead of scanned by a handful of workgroups).
        static int ncu_of[64];                                             // (a benign race: every writer stores the same value)
        int dev = 0; (void)hipGetDevice(&dev); dev = std::min(std::max(dev, 0), 63);
        if (!ncu_of[dev]) { hipDeviceProp_t pr; ncu_of[dev] = hipGetDeviceProperties(&pr, dev) == hipSuccess ? std::max(1, pr.multiProcessorCount) : 256; }
        const long long M = ndb - head, nqg = (nq + qg - 1) / qg, slots = 2LL * ncu_of[dev];
        const long long rounds = std::max(1LL, (M * nqg + 32768LL * slots - 1) / (32768LL * slots));
        const long long want = std::max(1LL, rounds * slots / nqg);
        long long cr = ((M + want - 1) / want + 255) / 256 * 256;
        cr = std::min(32768LL, std::max(2048LL, cr));
        chrows = (int)cr; nmain = (int)((M + cr - 1) / cr);
    }
    const int nhead = 64, stride = nhead + nmain;
    NNPart* p2 = (NNPart*)orbhip_nn_workspace(sizeof(NNPart) * (size_t)nq * stride + sizeof(int) * (size_t)nq * 3, s);
    if (!p2) return false;
    parts = p2;
    int* seed = reinterpret_cast<int*>(p2 + (size_t)nq * stride);
    int* share = seed + nq;                                                // [nq] best, [nq] second best: k_hamming_nn_fp4b's shared bounds
    const dim3 grid_h((nq + qg - 1) / qg, nhead, 1), grid_m((nq + qg - 1) / qg, nmain, 1), block(256, 1, 1);
    if (d_dbx) hipLaunchKernelGGL((k_hamming_nn_fp4b<9, true>), grid_h, block, 0, s, (const unsigned*)d_q, nq, (const unsigned*)d_dbx, head, base, parts, stride, (const int*)nullptr, (int*)nullptr, 0LL, 512, 0);
    else hipLaunchKernelGGL((k_hamming_nn_fp4b<9, false>), grid_h, block, 0, s, (const unsigned*)d_q, nq, (const unsigned*)d_db, head, base, parts, stride, (const int*)nullptr, (int*)nullptr, 0LL, 512, 0);
    if (nmain > 0) {
        hipLaunchKernelGGL(k_hamming_seed, dim3((nq + 3) / 4, 1, 1), dim3(256, 1, 1), 0, s, (const NNPart*)parts, nq, stride, nhead, seed, share);
        if (d_dbx) hipLaunchKernelGGL((k_hamming_nn_fp4b<15, true>), grid_m, block, 0, s, (const unsigned*)d_q, nq, (const unsigned*)d_dbx, ndb, base, parts, stride, (const int*)seed, share, head, chrows, nhead);
        else hipLaunchKernelGGL((k_hamming_nn_fp4b<15, false>), grid_m, block, 0, s, (const unsigned*)d_q, nq, (const unsigned*)d_db, ndb, base, parts, stride, (const int*)seed, share, head, chrows, nhead);
    }
    hipLaunchKernelGGL(k_hamming_merge, dim3((nq + 3) / 4, 1, 1), dim3(256, 1, 1), 0, s, (const NNPart*)parts, nq, stride, d_best_idx, d_best_dist, d_second);
    return true;
}

// ------------------------------------------------------------------------------------------------ frame grid
// Frame::AssignFeaturesToGrid on the current frame F2.  posX = round((x-mnMinX)*inv) — `round`, not floor (Frame.cc:384-385).
// One workgroup per frame, everything between the first read of the key points and the last write of the table in LDS: cell of every key point
// (u16), 3072 counters, the bucket table itself.  A frame's grid is latency, not work - as one launch among three of a single-frame search it
// used to cost 37 us of dependent global-memory round trips (per-cell insertion sort and key point gathers in HBM); now the key points are read
// once, coalesced, and the table is written once.
__device__ __forceinline__ int mg_wave_incl_scan(int v, int lane)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const int t = __shfl_up(v, off); if (lane >= off) v += t; }
    return v;
}
__device__ __forceinline__ int mg_cell(const orbhip_keypoint& k, const MatchParams& M, float gwInv, float ghInv)
{
    if (!(M.grid_all_levels || k.octave == 0)) return 0xFFFF;
    const int px = (int)roundf(__fmul_rn(__fsub_rn(k.x, M.min_x), gwInv)), py = (int)roundf(__fmul_rn(__fsub_rn(k.y, M.min_y), ghInv));
    return (px < 0 || px >= ORBHIP_GRID_COLS || py < 0 || py >= ORBHIP_GRID_ROWS) ? 0xFFFF : px * ORBHIP_GRID_ROWS + py;
}
__global__ __launch_bounds__(256) void k_match_grid(MatchParams M, float gwInv, float ghInv)
{
    HIP_DYNAMIC_SHARED(int, lds)
    int* s_cnt = lds;                                                    // [CELLS + 1] counters, then cursors
    int* s_items = s_cnt + ORBHIP_GRID_CELLS + 1;                         // [cap] bucket table (key point indices)
    unsigned short* s_cell = reinterpret_cast<unsigned short*>(s_items + M.cap);      // [cap] cell of key point i (0xFFFF: not in the grid)
    __shared__ int s_wsum[4];
    const int slot = blockIdx.x + M.slot0, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n2 = min(M.n2[slot], M.cap);
    const orbhip_keypoint* kp = M.kp2 + (long long)slot * M.cap;
    int* gstart = M.grid_start + (long long)slot * (ORBHIP_GRID_CELLS + 1);
    int* gitems = M.grid_items + (long long)slot * M.cap;
    float2* gxy = M.grid_xy + (long long)slot * M.cap;
    for (int c = tid; c <= ORBHIP_GRID_CELLS; c += 256) s_cnt[c] = 0;
    __syncthreads();
    // Only level-0 keypoints can ever be returned by GetFeaturesInArea(.., minLevel 0, maxLevel 0) (Frame.cc:362-370), and
    // filtering a cell keeps the relative order of its entries, so the buckets are built from level-0 keypoints only.
    for (int i = tid; i < n2; i += 256) {
        const int cell = mg_cell(kp[i], M, gwInv, ghInv);
        if (cell != 0xFFFF) atomicAdd(&s_cnt[cell], 1);
        s_cell[i] = (unsigned short)cell;
    }
    __syncthreads();
    // exclusive scan of 3072 counters: 12 consecutive ones per thread, a shuffle scan per wave, the four wave totals through LDS
    const int per = ORBHIP_GRID_CELLS / 256;
    int sum = 0;
    for (int k = 0; k < per; k++) sum += s_cnt[tid * per + k];
    const int incl = mg_wave_incl_scan(sum, lane);
    if (lane == 63) s_wsum[wave] = incl;
    __syncthreads();
    int run = incl - sum;
    for (int w = 0; w < wave; w++) run += s_wsum[w];
    for (int k = 0; k < per; k++) { const int v = s_cnt[tid * per + k]; s_cnt[tid * per + k] = run; gstart[tid * per + k] = run; run += v; }
    if (tid == 255) { gstart[ORBHIP_GRID_CELLS] = run; s_cnt[ORBHIP_GRID_CELLS] = run; }
    __syncthreads();
    const int total = s_cnt[ORBHIP_GRID_CELLS];
    __syncthreads();
    for (int i = tid; i < n2; i += 256) { const int cell = s_cell[i]; if (cell != 0xFFFF) s_items[atomicAdd(&s_cnt[cell], 1)] = i; }
    __syncthreads();
    // cells are tiny: restore keypoint order inside each cell (mGrid[x][y].push_back(i) for ascending i); after the scatter s_cnt[c] is the END of
    // cell c, which is where cell c + 1 starts
    for (int c = tid; c < ORBHIP_GRID_CELLS; c += 256) {
        const int a = c ? s_cnt[c - 1] : 0, b = s_cnt[c];
        for (int i = a + 1; i < b; i++) { const int v = s_items[i]; int j = i - 1; while (j >= a && s_items[j] > v) { s_items[j + 1] = s_items[j]; j--; } s_items[j + 1] = v; }
    }
    __syncthreads();
    for (int t = tid; t < total; t += 256) { const int i = s_items[t]; gitems[t] = i; const orbhip_keypoint k = kp[i]; float2 xy; xy.x = k.x; xy.y = k.y; gxy[t] = xy; }
}

// The same table for frames whose capacity does not fit the LDS form (12 KB + 6 bytes per key point: from ~23 000 key points per frame): counters and
// cursors in LDS, the bucket table built in place in global memory, the cell of a key point computed twice instead of kept.
__global__ __launch_bounds__(256) void k_match_grid_big(MatchParams M, float gwInv, float ghInv)
{
    __shared__ int s_cnt[ORBHIP_GRID_CELLS + 1];
    __shared__ int s_wsum[4];
    const int slot = blockIdx.x + M.slot0, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n2 = min(M.n2[slot], M.cap);
    const orbhip_keypoint* kp = M.kp2 + (long long)slot * M.cap;
    int* gstart = M.grid_start + (long long)slot * (ORBHIP_GRID_CELLS + 1);
    int* gitems = M.grid_items + (long long)slot * M.cap;
    float2* gxy = M.grid_xy + (long long)slot * M.cap;
    for (int c = tid; c <= ORBHIP_GRID_CELLS; c += 256) s_cnt[c] = 0;
    __syncthreads();
    for (int i = tid; i < n2; i += 256) { const int cell = mg_cell(kp[i], M, gwInv, ghInv); if (cell != 0xFFFF) atomicAdd(&s_cnt[cell], 1); }
    __syncthreads();
    const int per = ORBHIP_GRID_CELLS / 256;
    int sum = 0;
    for (int k = 0; k < per; k++) sum += s_cnt[tid * per + k];
    const int incl = mg_wave_incl_scan(sum, lane);
    if (lane == 63) s_wsum[wave] = incl;
    __syncthreads();
    int run = incl - sum;
    for (int w = 0; w < wave; w++) run += s_wsum[w];
    for (int k = 0; k < per; k++) { const int v = s_cnt[tid * per + k]; s_cnt[tid * per + k] = run; gstart[tid * per + k] = run; run += v; }
    if (tid == 255) { gstart[ORBHIP_GRID_CELLS] = run; s_cnt[ORBHIP_GRID_CELLS] = run; }
    __syncthreads();
    const int total = s_cnt[ORBHIP_GRID_CELLS];
    __syncthreads();
    for (int i = tid; i < n2; i += 256) { const int cell = mg_cell(kp[i], M, gwInv, ghInv); if (cell != 0xFFFF) gitems[atomicAdd(&s_cnt[cell], 1)] = i; }
    __threadfence_block();
    __syncthreads();
    for (int c = tid; c < ORBHIP_GRID_CELLS; c += 256) {                 // key point order inside each cell (see k_match_grid)
        const int a = c ? s_cnt[c - 1] : 0, b = s_cnt[c];
        for (int i = a + 1; i < b; i++) { const int v = gitems[i]; int j = i - 1; while (j >= a && gitems[j] > v) { gitems[j + 1] = gitems[j]; j--; } gitems[j + 1] = v; }
    }
    __threadfence_block();
    __syncthreads();
    for (int t = tid; t < total; t += 256) { const orbhip_keypoint k = kp[gitems[t]]; float2 xy; xy.x = k.x; xy.y = k.y; gxy[t] = xy; }
}

size_t orbhip_match_grid_lds(int cap) { return sizeof(int) * (ORBHIP_GRID_CELLS + 1 + (size_t)cap) + sizeof(unsigned short) * ((size_t)cap + 2); }

void orbhip_launch_match_grid(const MatchParams& M, int nslots, hipStream_t s)
{
    const float gwInv = (float)ORBHIP_GRID_COLS / (float)(M.max_x - M.min_x), ghInv = (float)ORBHIP_GRID_ROWS / (float)(M.max_y - M.min_y);   // Frame.cc:101-102
    size_t lds_max = (size_t)150 * 1024;
#ifdef ORBHIP_TEST_HOOKS      // the CPU emulation build only: small frames through the large-frame form
    if (const char* e = getenv("ORBHIP_TEST_MATCH_GRID_LDS_MAX")) lds_max = (size_t)atol(e);
#endif
    if (orbhip_match_grid_lds(M.cap) <= lds_max) hipLaunchKernelGGL(k_match_grid, dim3(nslots, 1, 1), dim3(256, 1, 1), orbhip_match_grid_lds(M.cap), s, M, gwInv, ghInv);
    else hipLaunchKernelGGL(k_match_grid_big, dim3(nslots, 1, 1), dim3(256, 1, 1), 0, s, M, gwInv, ghInv);
}

// ------------------------------------------------------------------------------------------------ candidates
// For the j-th level-0 keypoint of the previous frame: F2.GetFeaturesInArea(prev.x, prev.y, window, 0, 0) in the
// reference's order (ix outer, iy inner, keypoint order inside a cell) + DescriptorDistance to each candidate.
//
// The bucket table written by k_match_grid lists F2's (level-0) keypoints in exactly that order: by cell ix*ROWS+iy, then by
// index.  GetFeaturesInArea visits the cells [floor((x-r)/w) .. ceil((x+r)/w)] x [..] and keeps keypoints with |dx| < r and
// |dy| < r (Frame.cc:327-380); a keypoint that passes the distance test always lies in a visited cell (its cell is
// round(kx/w), and floor(a) <= round(v) <= ceil(b) for a < v < b; the sub-ulp slack of the float subtraction is far below
// the 0.5 of the rounding), so the result is the sub-sequence of the whole table that passes the distance test.  The
// table is scanned (coalesced, several loads in flight at once) instead of walking ~300 mostly empty cells with dependent
// loads; ballot ranks keep the order.
// wave64 minimum with DPP row shifts / broadcasts (6 dependent 4-cycle VALU steps); result broadcast from lane 63
__device__ __forceinline__ int wave_min_dpp(int v)
{
    v = min(v, __builtin_amdgcn_update_dpp(IMAX, v, 0x111, 0xf, 0xf, false));      // row_shr:1
    v = min(v, __builtin_amdgcn_update_dpp(IMAX, v, 0x112, 0xf, 0xf, false));      // row_shr:2
    v = min(v, __builtin_amdgcn_update_dpp(IMAX, v, 0x114, 0xf, 0xe, false));      // row_shr:4
    v = min(v, __builtin_amdgcn_update_dpp(IMAX, v, 0x118, 0xf, 0xc, false));      // row_shr:8 -> lane 15 of each row = row minimum
    v = min(v, __builtin_amdgcn_update_dpp(IMAX, v, 0x142, 0xa, 0xf, false));      // row_bcast:15 into rows 1 and 3
    v = min(v, __builtin_amdgcn_update_dpp(IMAX, v, 0x143, 0xc, 0xf, false));      // row_bcast:31 into rows 2 and 3 -> lane 63 = wave minimum
    return __builtin_amdgcn_readlane(v, 63);
}

#define MS_K 4                          // best candidates recorded per query (under the initial state: nothing matched yet)
#define MS_REC (MS_K + 1)               // + one word: more candidates exist
#define MS_NONE 0xFFFFFFFFu
#define MC_CHUNKS 4
#define MC_KPW 4                        // key points per wavefront: one per DPP row of 16 lanes
// minimum over the 16 lanes of a DPP row, in every lane of the row (4 dependent VALU steps; every row of the wave on its own)
__device__ __forceinline__ int row_min_dpp(int v)
{
    v = min(v, __builtin_amdgcn_update_dpp(IMAX, v, 0xB1, 0xf, 0xf, false));       // quad_perm:[1,0,3,2]
    v = min(v, __builtin_amdgcn_update_dpp(IMAX, v, 0x4E, 0xf, 0xf, false));       // quad_perm:[2,3,0,1] -> quad minimum
    v = min(v, __builtin_amdgcn_update_dpp(IMAX, v, 0x141, 0xf, 0xf, false));      // row_half_mirror -> minimum of 8
    v = min(v, __builtin_amdgcn_update_dpp(IMAX, v, 0x128, 0xf, 0xf, false));      // row_ror:8 -> row minimum
    return v;
}
// A wavefront takes four consecutive level-0 key points of F1, one per row of 16 lanes: the run of a key point is about two 64-entry passes long, and a
// whole wave per key point spent most of its instructions on per-wave overhead (load guards of eight chunks, the six-step wave minimum four times
// over, the setup chain).  A row walks its own run 16 entries at a time, in table order; rows are masked individually and the loop ends when
// every row is done.  Nothing else changes: list positions `pos`, the clamp at cand_stride, the records.
__global__ __launch_bounds__(256) void k_match_candidates(MatchParams M, float gwInv, float ghInv)
{
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, slot = blockIdx.y + M.slot0;
    const int row = lane >> 4, rl = lane & 15;
    const int n1l = min(M.n1_lvl0[slot * M.lvl_stride], M.lvl0_cap);
    if ((blockIdx.x * 4 + wave) * MC_KPW >= n1l) return;                       // (the whole wave)
    const bool live = (blockIdx.x * 4 + wave) * MC_KPW + row < n1l;            // a ragged last wave: its idle rows go along with an empty run
    const int j1 = live ? (blockIdx.x * 4 + wave) * MC_KPW + row : n1l - 1;
    const int i1 = M.list1 ? M.list1[(long long)slot * M.lvl0_cap + j1] : j1;   // level-major extractor output: level 0 = indices [0, n_lvl0)
    const int* gitems = M.grid_items + (long long)slot * M.cap;
    const float2* gxy = M.grid_xy + (long long)slot * M.cap;
    unsigned* cand = M.cand + ((long long)slot * M.lvl0_cap + j1) * M.cand_stride;
    const orbhip_keypoint* kp1 = M.kp1 + (long long)slot * M.cap;
    const float x = M.prev_from_kp1 ? kp1[i1].x : M.prev[((long long)slot * M.cap + i1) * 2];
    const float y = M.prev_from_kp1 ? kp1[i1].y : M.prev[((long long)slot * M.cap + i1) * 2 + 1];
    const float r = (float)M.window;
    const unsigned long long* d1 = (const unsigned long long*)(M.desc1 + ((long long)slot * M.cap + i1) * 32);
    const unsigned long long q0 = d1[0], q1 = d1[1], q2 = d1[2], q3 = d1[3];
    const unsigned below = (1u << rl) - 1u;
    int nc = 0;
    int tk[MS_K]; unsigned te[MS_K]; int nsel = 0;          // this lane's MS_K smallest (distance, list position) keys + their records
#pragma unroll
    for (int k = 0; k < MS_K; k++) { tk[k] = IMAX; te[k] = MS_NONE; }
    // The table is ordered by grid column first, so the entries of the columns the window can reach are ONE contiguous run of it: the columns
    // GetFeaturesInArea visits (Frame.cc:333-343: floor((x - mnMinX - r) inv) .. ceil((x - mnMinX + r) inv)), widened by one on either side (far
    // more than the float slack of that arithmetic).  A key point outside the run fails |dx| < r, so scanning the run alone gives the same
    // sub-sequence as scanning the whole table: at the metric's window (100 px of 1241) that is a fifth of it.
    const int* gstart = M.grid_start + (long long)slot * (ORBHIP_GRID_CELLS + 1);
    const float cl = __fmul_rn(__fsub_rn(__fsub_rn(x, M.min_x), r), gwInv), ch = __fmul_rn(__fadd_rn(__fsub_rn(x, M.min_x), r), gwInv);
    // (the comparisons are written so that a NaN position scans the whole table, like the distance test it would fail everywhere)
    const int col_lo = cl >= 1.0f ? (int)fminf(floorf(cl) - 1.0f, (float)ORBHIP_GRID_COLS) : 0;
    const int col_hi = ch < (float)(ORBHIP_GRID_COLS - 2) ? (int)fmaxf(ceilf(ch) + 2.0f, 0.0f) : ORBHIP_GRID_COLS;       // one past the last column scanned
    // (tab_cap: what k_match_select's tables hold - the callers size it by F2's level-0 key points, which is all the table can list)
    const int t_lo = min(gstart[min(col_lo, col_hi) * ORBHIP_GRID_ROWS], M.tab_cap), t_hi = live ? min(gstart[col_hi * ORBHIP_GRID_ROWS], M.tab_cap) : 0;
    for (int tb = t_lo + rl; __ballot(tb - rl < t_hi) != 0ull; tb += 16 * MC_CHUNKS) {
        float2 k[MC_CHUNKS]; int it[MC_CHUNKS];
#pragma unroll
        for (int c = 0; c < MC_CHUNKS; c++) {
            const int t = tb + 16 * c;
            k[c].x = 0.0f; k[c].y = 0.0f; it[c] = 0;
            if (t < t_hi) { k[c] = gxy[t]; it[c] = gitems[t]; }
        }
#pragma unroll
        for (int c = 0; c < MC_CHUNKS; c++) {
            const int t = tb + 16 * c;
            const bool ok = t < t_hi && fabsf(__fsub_rn(k[c].x, x)) < r && fabsf(__fsub_rn(k[c].y, y)) < r;    // Frame.cc:367-371
            const unsigned long long m = __ballot(ok);
            if (m == 0) continue;
            const unsigned mr = (unsigned)(m >> (16 * row)) & 0xFFFFu;          // this row's lanes
            const int pos = nc + __popc(mr & below);
            if (ok && pos < M.cand_stride) {
                const unsigned long long* d2 = (const unsigned long long*)(M.desc2 + ((long long)slot * M.cap + it[c]) * 32);
                const int dist = __popcll(q0 ^ d2[0]) + __popcll(q1 ^ d2[1]) + __popcll(q2 ^ d2[2]) + __popcll(q3 ^ d2[3]);
                unsigned rec = (unsigned)t | ((unsigned)dist << 20);       // table position | DescriptorDistance (ORBmatcher.cc:442)
                cand[pos] = rec;
                int key = (dist << 20) | pos;
                nsel++;
#pragma unroll
                for (int k = 0; k < MS_K; k++) if (key < tk[k]) { const int tkk = tk[k]; const unsigned tee = te[k]; tk[k] = key; te[k] = rec; key = tkk; rec = tee; }   // sorted insert
            }
            nc += __popc(mr);
        }
    }
    nc = min(nc, M.cand_stride);
    if (live && rl == 0) M.ncand[(long long)slot * M.lvl0_cap + j1] = nc;
    // The best / second-best update of the reference (ORBmatcher.cc:447-456) ends with the two smallest (distance, list position)
    // keys among the candidates it does not skip.  Record the MS_K smallest of the whole list: k_match_select takes the first two
    // that are not skipped at its turn.  Keys hold the list position, so a row's minimum lives in exactly one of its lanes: that lane writes
    // its record and drops it.
    unsigned* top = M.top + ((long long)slot * M.lvl0_cap + j1) * MS_REC;
    int popped = 0, nrec = 0;
#pragma unroll
    for (int r = 0; r < MS_K; r++) {
        const int m = row_min_dpp(tk[0]);
        if (m != IMAX) nrec = r + 1;
        if (m != IMAX && tk[0] == m) {
            if (live) top[r] = te[0];
            popped++;
#pragma unroll
            for (int k = 0; k + 1 < MS_K; k++) { tk[k] = tk[k + 1]; te[k] = te[k + 1]; }
            tk[MS_K - 1] = IMAX; te[MS_K - 1] = MS_NONE;
        }
    }
    const bool more = ((unsigned)(__ballot(nsel > popped) >> (16 * row)) & 0xFFFFu) != 0u;
    if (live && rl >= nrec && rl < MS_K) top[rl] = MS_NONE;
    if (live && rl == MS_K) top[MS_K] = more ? 1u : 0u;
}

void orbhip_launch_match_candidates(const MatchParams& M, int nslots, hipStream_t s)
{
    const float gwInv = (float)ORBHIP_GRID_COLS / (float)(M.max_x - M.min_x), ghInv = (float)ORBHIP_GRID_ROWS / (float)(M.max_y - M.min_y);
    hipLaunchKernelGGL(k_match_candidates, dim3((M.lvl0_cap + 4 * MC_KPW - 1) / (4 * MC_KPW), nslots, 1), dim3(256, 1, 1), 0, s, M, gwInv, ghInv);
}

// ------------------------------------------------------------------------------------------------ select

#define MS_T 64

// One wavefront (a 64-thread workgroup) per camera slot: it initialises the slot's tables and then resolves the order-dependent loop over F1's
// level-0 keypoints, 64 of them per step, from the MS_K records k_match_candidates left per key point (see the loop).
//
// A feature of F2 is named by its POSITION t in the slot's bucket table (k_match_grid), not by its key point index: only the table's entries
// (octave-0 key points inside the grid) can ever be candidates, so the per-feature state has tab_cap entries, not cap, whatever the order of F2's
// key points; results are mapped back through grid_items / grid_xy where they are written.  Per slot:
//   s_mdm[t]    vMatchedDistance[i2] << 21 | (vnMatches21[i2] + 1)      written together on every accept; distance MS_MD_NONE = nothing matched yet
//   s_stamp[t]  lowest undecided query that wants to claim feature t
//   s_acc[j1]   ((t + 1) << 6) | alive << 5 | rotation bin              the feature query j1 accepted (a query decides once); alive = not stolen since
//   s_hist      rotation histogram + the three maxima
// 2 tab_cap + lvl0_cap + 38 words: 5.4 KB at 2000 features on 1241x376, so the workgroup fits beside the extraction kernels it runs next to (k_fast_cells
// fills a CU's LDS exactly; tables of cap entries - 40 KB - displaced two or three of its workgroups per slot, profiles/matcher_beside_extraction.txt).
// The angles are not staged: rotHist only counts (ORBmatcher.cc:470-480 pushes, nothing pops when a match is stolen), so the bin of every accepted
// pair is computed after the loop, all queries in parallel, from the key point records in memory.  The candidate lists (t | dist<<20, canonical
// order) and their counts stay in HBM/L2 and are only read for the rare key point whose records are used up.
#define MS_MD_NONE 0x3FF
#define MS_J_MASK 0x1FFFFF
__device__ __forceinline__ int orbhip_match_select_ints_d(int tab_cap, int lvl0_cap) { return 2 * tab_cap + lvl0_cap + ORBHIP_HISTO_LENGTH + 8; }
// BIG: the per-slot tables in device memory (M.big_ws) instead of LDS, for frames of more level-0 key points than the LDS holds (the reference takes any
// nFeatures, Tracking.cc:113-125).  Same statements on volatile global words (one wave resolves the loop: program order is the order), see proj_select_body<BIG>.
template <bool BIG> __device__ __forceinline__ void match_select_body(const MatchParams& M)
{
    typedef typename std::conditional<BIG, volatile int, int>::type TI;
    const int slot = blockIdx.x + M.slot0, lane = threadIdx.x;
    const int n1 = M.n1[slot];
    const int n1l = min(M.n1_lvl0[slot * M.lvl_stride], M.lvl0_cap);
    const int* list1 = M.list1 ? M.list1 + (long long)slot * M.lvl0_cap : nullptr;
    const int nt = min(M.grid_start[(long long)slot * (ORBHIP_GRID_CELLS + 1) + ORBHIP_GRID_CELLS], M.tab_cap);
    HIP_DYNAMIC_SHARED(int, lds)
    TI* s_mdm = BIG ? M.big_ws + (long long)slot * (long long)orbhip_match_select_ints_d(M.tab_cap, M.lvl0_cap) : lds;
    TI* s_stamp = s_mdm + M.tab_cap;
    TI* s_acc = s_stamp + M.tab_cap;
    TI* s_hist = s_acc + M.lvl0_cap;        // [HISTO_LENGTH] + misc
    auto amin = [](TI* p, int v) { atomicMin(const_cast<int*>(p), v); };
    auto aadd = [](TI* p, int v) { atomicAdd(const_cast<int*>(p), v); };
    const orbhip_keypoint* kp1 = M.kp1 + (long long)slot * M.cap;
    const orbhip_keypoint* kp2 = M.kp2 + (long long)slot * M.cap;
    const int* gitems = M.grid_items + (long long)slot * M.cap;
    const float2* gxy = M.grid_xy + (long long)slot * M.cap;
    const int* ncand = M.ncand + (long long)slot * M.lvl0_cap;
    int* m12 = M.matches12 + (long long)slot * M.cap;
    float* prev = M.prev + (long long)slot * M.cap * 2;
    const unsigned* cand0 = M.cand + (long long)slot * M.lvl0_cap * M.cand_stride;
    const unsigned* top0 = M.top + (long long)slot * M.lvl0_cap * MS_REC;
    for (int t = lane; t < nt; t += MS_T) { s_mdm[t] = MS_MD_NONE << 21; s_stamp[t] = IMAX; }
    for (int i = lane; i < n1l; i += MS_T) s_acc[i] = 0;
    for (int i = lane; i < ORBHIP_HISTO_LENGTH + 8; i += MS_T) s_hist[i] = 0;
    for (int i = lane; i < n1; i += MS_T) { m12[i] = -1; if (M.prev_from_kp1) { prev[2 * i] = kp1[i].x; prev[2 * i + 1] = kp1[i].y; } }
    __syncthreads();
    auto matched_dist = [&](int t) -> int { return s_mdm[t] >> 21; };                          // vMatchedDistance
    auto accept_match = [&](int j1, int t, int dist) {                                          // :463-467
        const int old = (s_mdm[t] & MS_J_MASK) - 1;
        if (old >= 0) s_acc[old] = s_acc[old] & ~32;
        s_acc[j1] = ((t + 1) << 6) | 32; s_mdm[t] = (dist << 21) | (j1 + 1);
    };
    // 64 previous-frame key points per step.  A candidate is skipped once it is matched at a distance <= this query's
    // (vMatchedDistance only ever decreases), so a query's best / second-best are the first two recorded candidates that are
    // not skipped when its turn comes.  All lanes decide at once; a lane one of whose relevant records an earlier, still
    // undecided lane wants to claim (atomicMin stamp) waits for the next iteration; only a query whose records are used up
    // while its list holds more is rescanned from the list.
    for (int jb = 0; jb < n1l; jb += 64) {
        const int j1 = jb + lane;
        const bool inb = j1 < n1l;
        int ei[MS_K], ed[MS_K]; int nk = 0;
        const bool any = inb && ncand[j1] != 0;
#pragma unroll
        for (int k = 0; k < MS_K; k++) {
            const unsigned t = any ? top0[(long long)j1 * MS_REC + k] : MS_NONE;
            ei[k] = (int)(t & 0xFFFFFu); ed[k] = (int)((t >> 20) & 0x1FFu);
            if (t != MS_NONE) nk = k + 1;
        }
        const bool more = nk > 0 && top0[(long long)j1 * MS_REC + MS_K] != 0u;
        int stamped = -1;
        unsigned long long todo = __ballot(nk > 0);
        while (todo) {
            const bool mine = (todo >> lane) & 1ull;
            const int lowest = __ffsll((long long)todo) - 1;
            int a = -1, b = -1;
#pragma unroll
            for (int k = 0; k < MS_K; k++)
                if (mine && k < nk && b < 0 && !(matched_dist(ei[k]) <= ed[k])) { if (a < 0) a = k; else b = k; }      // :444-445
            const int ia = a >= 0 ? ei[a] : 0, da = a >= 0 ? ed[a] : IMAX, db = b >= 0 ? ed[b] : IMAX;
            const bool exhausted = mine && more && b < 0;
            const bool accept = mine && !exhausted && a >= 0 && da <= ORBHIP_TH_LOW && (float)da < __fmul_rn((float)db, M.nnratio);    // :459-461
            const int want = accept ? ia : -1;
            if (stamped >= 0 && stamped != want && s_stamp[stamped] == j1) s_stamp[stamped] = IMAX;       // withdraw an outdated claim
            __builtin_amdgcn_wave_barrier();
            if (want >= 0) amin(&s_stamp[want], j1);
            stamped = want;
            __builtin_amdgcn_wave_barrier();
            bool unsure = false;
            const int last = b >= 0 ? b : nk - 1;
#pragma unroll
            for (int k = 0; k < MS_K; k++)
                if (mine && lane != lowest && k <= last && !(matched_dist(ei[k]) <= ed[k]) && s_stamp[ei[k]] < j1) unsure = true;
            const unsigned long long bad = __ballot(unsure || exhausted);
            const int first_bad = bad ? __ffsll((long long)bad) - 1 : 64;
            const unsigned long long commit = first_bad == 64 ? todo : (todo & ((1ull << first_bad) - 1ull));
            const bool win = ((commit >> lane) & 1ull) && accept;
            if (win) {                                                                  // claimed features are distinct within one commit
                accept_match(j1, ia, da);
                if (s_stamp[ia] == j1) s_stamp[ia] = IMAX;                              // a decided claim lives in vMatchedDistance
                stamped = -1;
            }
            __builtin_amdgcn_wave_barrier();
            todo &= ~commit;
            if (first_bad == 64) break;
            if (first_bad != lowest || !((__ballot(exhausted) >> first_bad) & 1ull)) continue;
            // rescan the list of key point jb + first_bad against the current state
            todo &= ~(1ull << first_bad);
            if (lane == first_bad && stamped >= 0 && s_stamp[stamped] == j1) s_stamp[stamped] = IMAX;
            const int js = jb + first_bad, nc = ncand[js];
            const unsigned* cand = cand0 + (long long)js * M.cand_stride;
            int best = IMAX, second = IMAX, bidx = -1;
            for (int cb = 0; cb < nc; cb += 64) {
                const int c = cb + lane;
                const unsigned e = c < nc ? cand[c] : 0u;
                const int t = (int)(e & 0xFFFFFu), dist = (int)(e >> 20);
                const bool valid = c < nc && !(matched_dist(t) <= dist);              // :444-445
                // smallest (distance, lane) key by a DPP min network: strict '<' means the first candidate with the minimum
                // wins (:447-452); the runner-up is the minimum with that lane masked out
                const int key = valid ? ((dist << 6) | lane) : IMAX;
                const int k1 = wave_min_dpp(key);
                if (k1 == IMAX) continue;
                const int first = k1 & 63, wmin = k1 >> 6, ci = __builtin_amdgcn_readlane(t, first);
                const int k2 = wave_min_dpp(lane == first ? IMAX : key);
                const int wsec = k2 == IMAX ? IMAX : (k2 >> 6);
                if (wmin < best) { second = min(best, wsec); best = wmin; bidx = ci; } else second = min(second, wmin);
            }
            if (best <= ORBHIP_TH_LOW && (float)best < __fmul_rn((float)second, M.nnratio)) {      // :459-461
                if (lane == 0) accept_match(js, bidx, best);
            }
            __builtin_amdgcn_wave_barrier();                     // lane 0's updates are read by the whole wave next
        }
    }
    __builtin_amdgcn_wave_barrier();
    // nmatches of the reference (++ on accept, -- on steal :463-467 and on rotation reject :504-508) == final count of set entries
    if (M.check_ori) {
        const float factor = 1.0f / ORBHIP_HISTO_LENGTH;
        for (int j = lane; j < n1l; j += 64) {                    // rotHist[bin].push_back(i1) of every accept (:470-480), stolen later or not
            const int w = s_acc[j];
            if (w == 0) continue;
            float rot = __fsub_rn(kp1[list1 ? list1[j] : j].angle, kp2[gitems[(w >> 6) - 1]].angle);
            if (rot < 0.0f) rot = __fadd_rn(rot, 360.0f);
            int bin = (int)roundf(__fmul_rn(rot, factor));
            if (bin == ORBHIP_HISTO_LENGTH) bin = 0;
            bin = min(max(bin, 0), ORBHIP_HISTO_LENGTH - 1);
            s_acc[j] = w | bin; aadd(&s_hist[bin], 1);
        }
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) {                                          // ComputeThreeMaxima (:1601-1642)
            int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
            for (int i = 0; i < ORBHIP_HISTO_LENGTH; i++) {
                const int s = s_hist[i];
                if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
                else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
                else if (s > max3) { max3 = s; ind3 = i; }
            }
            if ((float)max2 < __fmul_rn(0.1f, (float)max1)) { ind2 = -1; ind3 = -1; }
            else if ((float)max3 < __fmul_rn(0.1f, (float)max1)) { ind3 = -1; }
            s_hist[ORBHIP_HISTO_LENGTH] = ind1; s_hist[ORBHIP_HISTO_LENGTH + 1] = ind2; s_hist[ORBHIP_HISTO_LENGTH + 2] = ind3;
        }
        __builtin_amdgcn_wave_barrier();
    }
    const int ind1 = s_hist[ORBHIP_HISTO_LENGTH], ind2 = s_hist[ORBHIP_HISTO_LENGTH + 1], ind3 = s_hist[ORBHIP_HISTO_LENGTH + 2];
    int cnt = 0;
    for (int j = lane; j < n1l; j += 64) {
        const int w = s_acc[j], b = w & 31;
        if (!(w & 32) || (M.check_ori && b != ind1 && b != ind2 && b != ind3)) continue;
        const int t = (w >> 6) - 1, i1 = list1 ? list1[j] : j;
        const float2 xy = gxy[t];                                                     // the key point's own x, y (k_match_grid)
        cnt++; m12[i1] = gitems[t]; prev[2 * i1] = xy.x; prev[2 * i1 + 1] = xy.y;     // :515-517
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off);
    if (lane == 0) M.nmatches[slot] = cnt;
}

__global__ __launch_bounds__(MS_T) void k_match_select(MatchParams M) { match_select_body<false>(M); }
__global__ __launch_bounds__(MS_T) void k_match_select_big(MatchParams M) { match_select_body<true>(M); }

#define MS_LDS_BUDGET (158 * 1024)
size_t orbhip_match_select_ints(int tab_cap, int lvl0_cap) { return (size_t)2 * tab_cap + (size_t)lvl0_cap + ORBHIP_HISTO_LENGTH + 8; }
bool orbhip_match_select_big(int tab_cap, int lvl0_cap)
{
    const char* env = getenv("ORBHIP_SELECT_BIG");                       // tests: 1 = the device-memory form at any size (read per call: tests switch inside one process)
    const bool force = env && env[0] == '1';
    return force || sizeof(int) * orbhip_match_select_ints(tab_cap, lvl0_cap) > MS_LDS_BUDGET;
}
void orbhip_launch_match_select(const MatchParams& M, int nslots, hipStream_t s)
{
    if (M.big_ws) hipLaunchKernelGGL(k_match_select_big, dim3(nslots, 1, 1), dim3(MS_T, 1, 1), 0, s, M);
    else hipLaunchKernelGGL(k_match_select, dim3(nslots, 1, 1), dim3(MS_T, 1, 1), sizeof(int) * orbhip_match_select_ints(M.tab_cap, M.lvl0_cap), s, M);
}
