// orbhip_kfdb.hip — KeyFrameDatabase on the device: the loop and relocalisation queries of ORB_SLAM2 (src/KeyFrameDatabase.cc) as a forward scan.
//
// The reference keeps an inverted file (one std::list<KeyFrame*> per word) and walks the lists of the query's words.  What that walk produces is a
// function of three things per key frame: how many words it shares with the query, which shared word comes first, and when it was added (words are
// visited ascending, each list is in add order and erase() keeps it).  So no list exists here.  The store is a forward store: every key frame's
// BowVector lies as one range of a word-id arena (u32) and a weight arena (f64); a query is
//   k_kfdb_scan    one wavefront per key frame: its words are looked up in the query's sorted id list (LDS, bisection) -> shared-word count, first
//                  shared word and the score, bit for bit the vocabulary's scoring object (ScoringObject.cpp:23-311; L1, L2, chi-square, Bhattacharyya,
//                  dot product: one instantiation each, orbhip_kfdb_set_scoring chooses): the terms in ascending word order in ONE dependent f64
//                  chain from 0
//   k_kfdb_select  one workgroup: the per-key-frame state rule of KeyFrameDatabase.cc:86-104 / :207-222 (mnRelocQuery, mnRelocWords, mRelocScore and
//                  the mnLoop* fields live here, per slot and kind), maxCommonWords, minCommonWords = (int)(max * 0.8f), the compaction of the key frames
//                  above it, their order (first shared word << 32 | add sequence) and the hit list (lScoreAndMatch)
// The covisibility accumulation (:144-196, :258-308) needs the caller's neighbour lists and is host arithmetic (orbhip_kfdb_select).
// One lock per database, held for a whole entry: the reference's mMutex (add from LocalMapping, the queries from LoopClosing and Tracking).
// Batches of queries (orbhip_kfdb_query_batch and its companions) have kernels of their own in the second half of this file.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <utility>
#include <vector>
#include <algorithm>
#include "../../include/orbhip.h"
#include "orbhip_internal.h"

#define KFCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return orbhip_set_error(ORBHIP_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)
#define KFDB_MAX_WORDS 8192            // BOW_MAX_FEATURES (orbhip_bow.hip): a BowVector has at most one word per feature

struct KfSlot { unsigned long long off; unsigned n, seq, live, pad; };      // range [off, off + n) of both arenas, add sequence number, live flag
struct KfState { unsigned long long query; int words; float score; };       // mnRelocQuery / mnRelocWords / mRelocScore (or the mnLoop* fields) of one key frame

// ------------------------------------------------------------------------------------------------ k_kfdb_scan
struct KfScanParams {
    const uint32_t* ids; const double* vals; const KfSlot* slots;
    const int* list; int n;                                  // wave w scans slot list[w] (list == nullptr: slot w), n waves in all
    const uint32_t* q_id; const double* q_val;               // the query's BowVector, ascending ids
    const int* q_n_dev; int q_n, q_cap;                      // its length: read on the device (a resident frame's nbow) or given; q_cap entries of LDS
    int* cnt; uint32_t* first; double* score;                // per wave: shared words, first shared word, score
};

__device__ __forceinline__ double kf_readlane(double v, int lane)             // lane is wave-uniform: two v_readlane_b32
{
    int h[2]; memcpy(h, &v, 8);
    h[0] = __builtin_amdgcn_readlane(h[0], lane); h[1] = __builtin_amdgcn_readlane(h[1], lane);
    double r; memcpy(&r, h, 8); return r;
}

// The term a shared word adds to the chain (vi the query's weight, wi the key frame's) and what becomes of the sum: SC is DBoW2's ScoringType
// (0 L1_NORM :23-68, 1 L2_NORM :73-119, 2 CHI_SQUARE :124-188, 4 BHATTACHARYYA :243-282, 5 DOT_PRODUCT :287-311).  Every operation rounds once, to nearest.
template <int SC> __device__ __forceinline__ double kf_term(double vi, double wi)
{
    if constexpr (SC == 0) return __dsub_rn(__dsub_rn(fabs(__dsub_rn(vi, wi)), fabs(vi)), fabs(wi));
    else if constexpr (SC == 2) { const double d = __dadd_rn(vi, wi); return d != 0.0 ? __ddiv_rn(__dmul_rn(vi, wi), d) : 0.0; }      // (s + 0.0 == s: s is never -0.0)
    else if constexpr (SC == 4) return __dsqrt_rn(__dmul_rn(vi, wi));
    else return __dmul_rn(vi, wi);
}
template <int SC> __device__ __forceinline__ double kf_result(double s)
{
    if constexpr (SC == 0) return -s / 2.0;
    else if constexpr (SC == 1) return s >= 1 ? 1.0 : __dsub_rn(1.0, __dsqrt_rn(__dsub_rn(1.0, s)));
    else if constexpr (SC == 2) return __dmul_rn(2.0, s);
    else return s;
}

#define KS_T 256                       // four wavefronts share one staged copy of the query's ids
template <int SC> __global__ __launch_bounds__(KS_T) void k_kfdb_scan(KfScanParams P)
{
    HIP_DYNAMIC_SHARED(uint32_t, q)
    const int tid = threadIdx.x, lane = tid & 63;
    int nq = P.q_n_dev ? *P.q_n_dev : P.q_n;
    nq = nq < 0 ? 0 : nq > P.q_cap ? P.q_cap : nq;
    for (int i = tid; i < nq; i += KS_T) q[i] = P.q_id[i];
    __syncthreads();
    const int w = blockIdx.x * (KS_T / 64) + (tid >> 6);
    if (w >= P.n) return;                                                     // (whole waves, after the kernel's only barrier)
    const KfSlot S = P.slots[P.list ? P.list[w] : w];
    int top = 0;                                                              // largest power of two <= nq: the bisection's first step
    if (nq > 0) top = 1 << (31 - __clz(nq));
    int cnt = 0; uint32_t first = 0xffffffffu; double s = 0.0;
    if (S.live && nq > 0 && S.n > 0) {
        const uint32_t* kid = P.ids + S.off; const double* kval = P.vals + S.off;
        uint32_t id_next = (unsigned)lane < S.n ? kid[lane] : 0xffffffffu;
        for (unsigned base = 0; base < S.n; base += 64) {
            const unsigned i = base + lane; const bool in = i < S.n;
            const uint32_t id = id_next;
            id_next = i + 64 < S.n ? kid[i + 64] : 0xffffffffu;               // the next chunk's ids are on their way while this one is searched
            int pos = 0;                                                      // number of query ids below `id` (lower bound), the same steps in every lane
            for (int st = top; st; st >>= 1) { const int p = pos + st; if (p <= nq && q[p - 1] < id) pos = p; }
            const bool hit = in && pos < nq && q[pos] == id;
            double term = 0.0;
            if (hit) {                                                        // score(query, key frame): vi the query's weight, wi the key frame's; both loads leave together
                const double wi = kval[i], vi = P.q_val[pos];
                term = kf_term<SC>(vi, wi);
            }
            unsigned long long m = __ballot(hit);
            if (m) {
                if (cnt == 0) first = (uint32_t)__builtin_amdgcn_readlane((int)id, __ffsll((long long)m) - 1);
                cnt += __popcll(m);
                // the shared pairs of this chunk in word order (the set bits ascending), added to the ONE chain that runs through every chunk of the key frame
                while (m) { const int l = __ffsll((long long)m) - 1; m &= m - 1; s = __dadd_rn(s, kf_readlane(term, l)); }
            }
        }
    }
    if (lane == 0) { P.cnt[w] = cnt; P.first[w] = first; P.score[w] = kf_result<SC>(s); }
}

// ------------------------------------------------------------------------------------------------ k_kfdb_select
struct KfSelectParams {
    const KfSlot* slots; KfState* state; int nslots;         // state: this kind's
    const int* cnt; const uint32_t* first; const double* score;      // k_kfdb_scan's answers, per slot
    const int* excl; int nexcl;                              // LOOP: the slots connected to the querying key frame, ascending
    int kind; unsigned long long qid; float min_score;
    int* flag;                                               // [nslots] words of a listed key frame, 0 otherwise
    unsigned long long* keys; int* pay; int cap2;            // sort workspace for more than KSEL_LDS listed key frames, cap2 a power of two >= nslots
    orbhip_kfdb_hit* hits; int* meta;                        // hit list in the reference's order; meta = {nhits, nsharing, min_common}
};

#define KSEL_T 1024                    // slots per pass
#define KSEL_LDS 4096                  // listed key frames whose sort fits the LDS (12 bytes each)

// bitonic sort of n2 (a power of two) unique keys with a payload, by the whole workgroup
template <typename KP, typename PP> __device__ __forceinline__ void kf_bitonic(KP keys, PP pay, int n2, int tid)
{
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (n2 >> 1); t += KSEL_T) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const unsigned long long a = keys[i], b = keys[l];
                if ((a > b) == ((i & k) == 0) && a != b) { keys[i] = b; keys[l] = a; const int pa = pay[i]; pay[i] = pay[l]; pay[l] = pa; }
            }
            __syncthreads();
        }
}

__global__ __launch_bounds__(KSEL_T) void k_kfdb_select(KfSelectParams P)
{
    __shared__ int s_max, s_nlist, s_nhit;
    __shared__ unsigned long long s_key[KSEL_LDS];
    __shared__ int s_pay[KSEL_LDS];
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) { s_max = 0; s_nlist = 0; s_nhit = 0; }
    __syncthreads();
    // pass 1: the state rule; a slot is one thread's alone
    int lmax = 0, nl = 0;
    for (int b = 0; b < P.nslots; b += KSEL_T) {
        const int i = b + tid;
        if (i >= P.nslots) break;
        int listed = 0;
        const int c = P.slots[i].live ? P.cnt[i] : 0;
        if (c >= 1) {
            KfState st = P.state[i];
            if (st.query == P.qid) st.words += c;                                                 // met before under this query id: counts on, not listed again
            else {
                bool excluded = false;
                if (P.kind == ORBHIP_KFDB_LOOP && P.nexcl > 0) {
                    int lo = 0, hi = P.nexcl;
                    while (lo < hi) { const int mid = (lo + hi) >> 1; if (P.excl[mid] < i) lo = mid + 1; else hi = mid; }
                    excluded = lo < P.nexcl && P.excl[lo] == i;
                }
                if (excluded) st.words = 1;                                                       // every shared word resets the count to 0 and adds one
                else { st.query = P.qid; st.words = c; listed = c; }
            }
            P.state[i].query = st.query; P.state[i].words = st.words;
        }
        P.flag[i] = listed;
        lmax = max(lmax, listed); nl += listed != 0;
    }
    for (int o = 32; o; o >>= 1) { lmax = max(lmax, __shfl_xor(lmax, o)); nl += __shfl_xor(nl, o); }
    if (lane == 0 && nl) { atomicMax(&s_max, lmax); atomicAdd(&s_nlist, nl); }
    __syncthreads();
    const int nlist = s_nlist;
    const int minc = (int)__fmul_rn((float)s_max, 0.8f);                                          // int minCommonWords = maxCommonWords*0.8f;
    const bool in_lds = nlist <= KSEL_LDS;
    // pass 2: score and compact the listed key frames above minCommonWords (any order: they are sorted next)
    for (int b = 0; b < P.nslots; b += KSEL_T) {                                                  // (whole waves leave together: KSEL_T is a multiple of 64)
        const int i = b + tid;
        bool hit = false; unsigned long long key = 0;
        if (i < P.nslots && P.flag[i] > minc) {
            const float sf = (float)P.score[i];
            P.state[i].score = sf;                                                                // written for every scored key frame ...
            hit = P.kind == ORBHIP_KFDB_RELOC || sf >= P.min_score;                               // ... listed only above minScore (LOOP)
            key = ((unsigned long long)P.first[i] << 32) | P.slots[i].seq;
        }
        const unsigned long long m = __ballot(hit);
        if (m) {
            const int leader = __ffsll((long long)m) - 1;
            int base = 0;
            if (lane == leader) base = atomicAdd(&s_nhit, (int)__popcll(m));                      // one LDS atomic per wave
            base = __builtin_amdgcn_readlane(base, leader);
            const int pos = base + (int)__popcll(m & ((1ull << lane) - 1ull));
            if (hit) { if (in_lds) { s_key[pos] = key; s_pay[pos] = i; } else { P.keys[pos] = key; P.pay[pos] = i; } }
        }
    }
    __syncthreads();
    const int n = s_nhit;
    int n2 = 1; while (n2 < n) n2 <<= 1;
    if (in_lds) {
        for (int t = n + tid; t < n2; t += KSEL_T) { s_key[t] = ~0ull; s_pay[t] = 0; }
        __syncthreads();
        kf_bitonic(s_key, s_pay, n2, tid);
        for (int t = tid; t < n; t += KSEL_T) { const int slot = s_pay[t]; orbhip_kfdb_hit h; h.slot = slot; h.words = P.flag[slot]; h.score = (float)P.score[slot]; P.hits[t] = h; }
    } else {
        for (int t = n + tid; t < n2; t += KSEL_T) { P.keys[t] = ~0ull; P.pay[t] = 0; }
        __syncthreads();
        kf_bitonic(P.keys, P.pay, n2, tid);
        for (int t = tid; t < n; t += KSEL_T) { const int slot = P.pay[t]; orbhip_kfdb_hit h; h.slot = slot; h.words = P.flag[slot]; h.score = (float)P.score[slot]; P.hits[t] = h; }
    }
    if (tid == 0) { P.meta[0] = n; P.meta[1] = nlist; P.meta[2] = nlist ? minc : 0; }
}

// the state of the named slots (list[i] < 0: zeros), for orbhip_kfdb_select's neighbour lists
__global__ __launch_bounds__(256) void k_kfdb_gather(const KfState* state, const int* list, int n, KfState* out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int slot = list[i];
    unsigned long long query = 0; int words = 0; float score = 0.0f;
    if (slot >= 0) { query = state[slot].query; words = state[slot].words; score = state[slot].score; }
    out[i].query = query; out[i].words = words; out[i].score = score;
}

// ------------------------------------------------------------------------------------------------ host side
struct KfBatch;
static void kf_batch_free(KfBatch* b);
static void kf_batch_supersede(KfBatch* b);

struct orbhip_kfdb {
    int device = 0, nwords = 0, scoring = 0;                 // scoring: DBoW2's ScoringType of the next query (orbhip_kfdb_set_scoring)
    std::mutex m;
    // forward store: both arenas grow together by doubling; erased ranges are reused first-fit
    uint32_t* d_ids = nullptr; double* d_vals = nullptr; size_t arena_cap = 0, arena_end = 0;
    std::vector<std::pair<size_t, size_t>> holes;            // (offset, length)
    KfSlot* d_slots = nullptr; KfState* d_state[2] = {nullptr, nullptr}; int slot_cap = 0, nslots = 0, nlive = 0; unsigned next_seq = 0;      // slot_cap: a power of two
    std::vector<KfSlot> h_slots; std::vector<int> free_slots;
    // per-query workspace (sized with the slot arrays), the query's BowVector, slot lists
    int* d_cnt = nullptr; uint32_t* d_first = nullptr; double* d_score = nullptr; int* d_flag = nullptr; unsigned long long* d_keys = nullptr; int* d_pay = nullptr;
    orbhip_kfdb_hit* d_hits = nullptr; int* d_meta = nullptr; uint32_t* d_qid = nullptr; double* d_qval = nullptr;
    int* d_list = nullptr; size_t list_cap = 0; KfState* d_gather = nullptr; size_t gather_cap = 0;
    uint64_t batch_tokens = 0; KfBatch* batch = nullptr;                           // the batched queries' workspace and snapshot (below), made by the first orbhip_kfdb_query_batch
};

static void kf_free(void* p) { if (p) (void)hipFree(p); }
template <typename T> static hipError_t kf_grow(T** p, size_t* cap, size_t need)      // contents are not kept
{
    if (need <= *cap) return hipSuccess;
    kf_free(*p); *p = nullptr; *cap = 0;
    const size_t nc = std::max<size_t>(need + need / 2, 256);
    const hipError_t e = orbhip_dmalloc((void**)p, nc * sizeof(T));
    if (e == hipSuccess) *cap = nc;
    return e;
}
// a larger array with the first `keep` elements of the old one (the caller has drained every stream that used it: all entries are synchronous)
template <typename T> static hipError_t kf_regrow(T** p, size_t keep, size_t ncap)
{
    T* np = nullptr;
    hipError_t e = orbhip_dmalloc((void**)&np, std::max<size_t>(ncap, 1) * sizeof(T)); if (e != hipSuccess) return e;
    if (keep && *p) { e = hipMemcpy(np, *p, keep * sizeof(T), hipMemcpyDeviceToDevice); if (e != hipSuccess) { (void)hipFree(np); return e; } }
    kf_free(*p); *p = np;
    return hipSuccess;
}

static orbhip_status kf_ensure_slots(orbhip_kfdb* db, int need)
{
    if (need <= db->slot_cap) return ORBHIP_OK;
    int nc = std::max(db->slot_cap, 64); while (nc < need) nc *= 2;
    const size_t keep = (size_t)db->nslots, C = (size_t)nc;
    KFCHK(kf_regrow(&db->d_slots, keep, C)); KFCHK(kf_regrow(&db->d_state[0], keep, C)); KFCHK(kf_regrow(&db->d_state[1], keep, C));
    KFCHK(kf_regrow(&db->d_cnt, 0, C)); KFCHK(kf_regrow(&db->d_first, 0, C)); KFCHK(kf_regrow(&db->d_score, 0, C)); KFCHK(kf_regrow(&db->d_flag, 0, C));
    KFCHK(kf_regrow(&db->d_keys, 0, C)); KFCHK(kf_regrow(&db->d_pay, 0, C)); KFCHK(kf_regrow(&db->d_hits, 0, C));
    db->slot_cap = nc;
    return ORBHIP_OK;
}

static bool kf_ascending(const uint32_t* id, int n, int nwords)
{
    for (int i = 0; i < n; i++) if (id[i] >= (uint32_t)nwords || (i && id[i] <= id[i - 1])) return false;
    return true;
}

extern "C" orbhip_status orbhip_kfdb_create(orbhip_kfdb** out, int device, int nwords, int scoring)
{
    if (!out || nwords < 0) return orbhip_set_error(ORBHIP_ERR_INVALID, "bad argument");
    *out = nullptr;
    if (scoring != 0) return orbhip_set_error(ORBHIP_ERR_UNSUPPORTED, "key-frame database: scoring %d (only 0, L1_NORM, runs on the device: it is what ORBvoc.txt declares, and KL needs a log with no bit-exact device form)", scoring);
    KFCHK(hipSetDevice(device));
    orbhip_kfdb* db = new orbhip_kfdb(); db->device = device; db->nwords = nwords;
    hipError_t e = orbhip_dmalloc((void**)&db->d_meta, 4 * sizeof(int));
    if (e == hipSuccess) e = orbhip_dmalloc((void**)&db->d_qid, KFDB_MAX_WORDS * sizeof(uint32_t));
    if (e == hipSuccess) e = orbhip_dmalloc((void**)&db->d_qval, KFDB_MAX_WORDS * sizeof(double));
    if (e != hipSuccess) { orbhip_kfdb_destroy(db); return orbhip_set_error(ORBHIP_ERR_HIP, "key-frame database: %s", hipGetErrorString(e)); }
    *out = db;
    return ORBHIP_OK;
}

extern "C" void orbhip_kfdb_destroy(orbhip_kfdb* db)
{
    if (!db) return;
    (void)hipSetDevice(db->device);
    void* ptrs[] = {db->d_ids, db->d_vals, db->d_slots, db->d_state[0], db->d_state[1], db->d_cnt, db->d_first, db->d_score, db->d_flag, db->d_keys, db->d_pay, db->d_hits,
                    db->d_meta, db->d_qid, db->d_qval, db->d_list, db->d_gather};
    for (void* p : ptrs) kf_free(p);
    kf_batch_free(db->batch);
    delete db;
}

extern "C" orbhip_status orbhip_kfdb_clear(orbhip_kfdb* db)
{
    if (!db) return orbhip_set_error(ORBHIP_ERR_INVALID, "null database");
    std::lock_guard<std::mutex> lock(db->m);
    db->nslots = 0; db->nlive = 0; db->arena_end = 0; db->holes.clear(); db->h_slots.clear(); db->free_slots.clear();
    kf_batch_supersede(db->batch);
    return ORBHIP_OK;
}

// The scoring object of every later query: what the reference reads from the vocabulary at query time (KeyFrameDatabase.cc:133,249 call mpVoc->score).
// Scores that earlier queries left in the key frames' state stay, as mRelocScore / mLoopScore do.
extern "C" orbhip_status orbhip_kfdb_set_scoring(orbhip_kfdb* db, int scoring)
{
    if (!db) return orbhip_set_error(ORBHIP_ERR_INVALID, "null database");
    if (scoring < 0 || scoring > 5) return orbhip_set_error(ORBHIP_ERR_INVALID, "key-frame database: scoring %d outside 0..5", scoring);
    if (scoring == 3) return orbhip_set_error(ORBHIP_ERR_UNSUPPORTED, "key-frame database: scoring 3 (KL): its sum runs over the query's words that the key frame LACKS and needs a log, "
                                              "and as a divergence it grows with dissimilarity, so the database's higher-is-better selection means nothing under it");
    std::lock_guard<std::mutex> lock(db->m);
    db->scoring = scoring;
    return ORBHIP_OK;
}

extern "C" int orbhip_kfdb_get_scoring(orbhip_kfdb* db)
{
    if (!db) return 0;
    std::lock_guard<std::mutex> lock(db->m);
    return db->scoring;
}

extern "C" int orbhip_kfdb_size(orbhip_kfdb* db)
{
    if (!db) return 0;
    std::lock_guard<std::mutex> lock(db->m);
    return db->nlive;
}

extern "C" orbhip_status orbhip_kfdb_add(orbhip_kfdb* db, const uint32_t* bow_id, const double* bow_val, int nbow, int* slot_out)
{
    OrbApiTimer api_timer;
    if (!db || !slot_out || nbow < 0 || (nbow > 0 && (!bow_id || !bow_val))) return orbhip_set_error(ORBHIP_ERR_INVALID, "bad argument");
    *slot_out = -1;
    if (nbow > KFDB_MAX_WORDS) return orbhip_set_error(ORBHIP_ERR_UNSUPPORTED, "a BowVector of %d words (at most %d)", nbow, KFDB_MAX_WORDS);
    if (!kf_ascending(bow_id, nbow, db->nwords)) return orbhip_set_error(ORBHIP_ERR_INVALID, "BowVector ids must ascend and lie below %d", db->nwords);
    std::lock_guard<std::mutex> lock(db->m);
    KFCHK(hipSetDevice(db->device));
    hipStream_t s = orbhip_thread_stream(db->device);
    // a range of the arenas: an erased one that is large enough, else the end
    size_t off = db->arena_end; bool from_hole = false;
    for (size_t h = 0; h < db->holes.size() && nbow > 0; h++)
        if (db->holes[h].second >= (size_t)nbow) {
            off = db->holes[h].first; from_hole = true;
            if (db->holes[h].second == (size_t)nbow) db->holes.erase(db->holes.begin() + h); else { db->holes[h].first += nbow; db->holes[h].second -= nbow; }
            break;
        }
    if (!from_hole && off + nbow > db->arena_cap) {
        size_t nc = std::max<size_t>(db->arena_cap, 4096); while (nc < off + nbow) nc *= 2;
        KFCHK(kf_regrow(&db->d_ids, db->arena_end, nc)); KFCHK(kf_regrow(&db->d_vals, db->arena_end, nc));
        db->arena_cap = nc;
    }
    const int slot = db->free_slots.empty() ? db->nslots : db->free_slots.back();
    const orbhip_status st = kf_ensure_slots(db, slot + 1); if (st != ORBHIP_OK) return st;
    KfSlot S; S.off = off; S.n = (unsigned)nbow; S.seq = db->next_seq; S.live = 1; S.pad = 0;
    if (nbow > 0) {
        KFCHK(hipMemcpyAsync(db->d_ids + off, bow_id, (size_t)nbow * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        KFCHK(hipMemcpyAsync(db->d_vals + off, bow_val, (size_t)nbow * sizeof(double), hipMemcpyHostToDevice, s));
    }
    KFCHK(hipMemcpyAsync(db->d_slots + slot, &S, sizeof S, hipMemcpyHostToDevice, s));
    for (int k = 0; k < 2; k++) KFCHK(hipMemsetAsync(db->d_state[k] + slot, 0, sizeof(KfState), s));      // query 0, words 0, score 0.0f
    KFCHK(hipStreamSynchronize(s));
    // committed: the host's books follow
    if (!from_hole) db->arena_end = off + nbow;
    if (db->free_slots.empty()) { db->nslots++; db->h_slots.push_back(S); } else { db->free_slots.pop_back(); db->h_slots[slot] = S; }
    db->next_seq++; db->nlive++;
    *slot_out = slot;
    return ORBHIP_OK;
}

static bool kf_live(const orbhip_kfdb* db, int slot) { return slot >= 0 && slot < db->nslots && db->h_slots[slot].live; }

extern "C" orbhip_status orbhip_kfdb_erase(orbhip_kfdb* db, int slot)
{
    OrbApiTimer api_timer;
    if (!db) return orbhip_set_error(ORBHIP_ERR_INVALID, "null database");
    std::lock_guard<std::mutex> lock(db->m);
    if (!kf_live(db, slot)) return orbhip_set_error(ORBHIP_ERR_INVALID, "slot %d holds no key frame", slot);
    KFCHK(hipSetDevice(db->device));
    hipStream_t s = orbhip_thread_stream(db->device);
    KfSlot S = db->h_slots[slot]; S.live = 0;
    KFCHK(hipMemcpyAsync(db->d_slots + slot, &S, sizeof S, hipMemcpyHostToDevice, s));
    KFCHK(hipStreamSynchronize(s));
    if (S.n) db->holes.push_back(std::make_pair((size_t)S.off, (size_t)S.n));
    db->h_slots[slot] = S; db->free_slots.push_back(slot); db->nlive--;
    return ORBHIP_OK;
}

static void kf_launch_scan(orbhip_kfdb* db, const int* d_list, int n, const uint32_t* d_qid, const double* d_qval, const int* d_qn, int qn, int qcap, hipStream_t s)
{
    KfScanParams P; memset(&P, 0, sizeof P);
    P.ids = db->d_ids; P.vals = db->d_vals; P.slots = db->d_slots; P.list = d_list; P.n = n;
    P.q_id = d_qid; P.q_val = d_qval; P.q_n_dev = d_qn; P.q_n = qn; P.q_cap = qcap;
    P.cnt = db->d_cnt; P.first = db->d_first; P.score = db->d_score;
    const dim3 g((n + KS_T / 64 - 1) / (KS_T / 64), 1, 1), b(KS_T, 1, 1); const size_t lds = (size_t)std::max(qcap, 1) * sizeof(uint32_t);
    switch (db->scoring) {
    case 1: hipLaunchKernelGGL(k_kfdb_scan<1>, g, b, lds, s, P); break;
    case 2: hipLaunchKernelGGL(k_kfdb_scan<2>, g, b, lds, s, P); break;
    case 4: hipLaunchKernelGGL(k_kfdb_scan<4>, g, b, lds, s, P); break;
    case 5: hipLaunchKernelGGL(k_kfdb_scan<5>, g, b, lds, s, P); break;
    default: hipLaunchKernelGGL(k_kfdb_scan<0>, g, b, lds, s, P); break;
    }
}

// scan + select + download on stream s, the database's lock held; the query's BowVector is on the device already
static orbhip_status kf_query_core(orbhip_kfdb* db, int kind, unsigned long long qid, const uint32_t* d_qid, const double* d_qval, const int* d_qn, int qn, int qcap,
                                   const int* excl, int nexcl, float min_score, orbhip_kfdb_hit* hits, int cap, int* nhits, int* nsharing, int* min_common, hipStream_t s)
{
    *nhits = 0; if (nsharing) *nsharing = 0; if (min_common) *min_common = 0;
    kf_batch_supersede(db->batch);                                            // a batch's snapshot describes the state its own queries left
    if (db->nslots == 0) return ORBHIP_OK;
    int ne = 0;
    if (kind == ORBHIP_KFDB_LOOP && nexcl > 0) {
        std::vector<int> e; e.reserve((size_t)nexcl);
        for (int i = 0; i < nexcl; i++) if (excl[i] >= 0 && excl[i] < db->nslots) e.push_back(excl[i]);
        std::sort(e.begin(), e.end()); e.erase(std::unique(e.begin(), e.end()), e.end());
        ne = (int)e.size();
        KFCHK(kf_grow(&db->d_list, &db->list_cap, (size_t)ne));
        if (ne) { KFCHK(hipMemcpyAsync(db->d_list, e.data(), (size_t)ne * sizeof(int), hipMemcpyHostToDevice, s)); KFCHK(hipStreamSynchronize(s)); }      // (e leaves scope)
    }
    kf_launch_scan(db, nullptr, db->nslots, d_qid, d_qval, d_qn, qn, qcap, s);
    KfSelectParams Q; memset(&Q, 0, sizeof Q);
    Q.slots = db->d_slots; Q.state = db->d_state[kind]; Q.nslots = db->nslots; Q.cnt = db->d_cnt; Q.first = db->d_first; Q.score = db->d_score;
    Q.excl = db->d_list; Q.nexcl = ne; Q.kind = kind; Q.qid = qid; Q.min_score = min_score;
    Q.flag = db->d_flag; Q.keys = db->d_keys; Q.pay = db->d_pay; Q.cap2 = db->slot_cap; Q.hits = db->d_hits; Q.meta = db->d_meta;
    hipLaunchKernelGGL(k_kfdb_select, dim3(1, 1, 1), dim3(KSEL_T, 1, 1), 0, s, Q);
    KFCHK(hipGetLastError());
    int meta[3] = {0, 0, 0};
    KFCHK(hipMemcpyAsync(meta, db->d_meta, sizeof meta, hipMemcpyDeviceToHost, s));
    KFCHK(hipStreamSynchronize(s));
    if (meta[0] < 0 || meta[0] > db->nslots) return orbhip_set_error(ORBHIP_ERR_HIP, "key-frame database: %d hits among %d slots", meta[0], db->nslots);
    const int ncopy = std::min(meta[0], cap);
    if (ncopy > 0) { KFCHK(hipMemcpyAsync(hits, db->d_hits, (size_t)ncopy * sizeof(orbhip_kfdb_hit), hipMemcpyDeviceToHost, s)); KFCHK(hipStreamSynchronize(s)); }
    *nhits = meta[0]; if (nsharing) *nsharing = meta[1]; if (min_common) *min_common = meta[2];
    if (meta[0] > cap) return orbhip_set_error(ORBHIP_ERR_CAPACITY, "key-frame database: %d hits, room for %d (the key frames' state is that of the completed query)", meta[0], cap);
    return ORBHIP_OK;
}

static orbhip_status kf_upload_query(orbhip_kfdb* db, const uint32_t* bow_id, const double* bow_val, int nbow, hipStream_t s)
{
    if (nbow > KFDB_MAX_WORDS) return orbhip_set_error(ORBHIP_ERR_UNSUPPORTED, "a BowVector of %d words (at most %d)", nbow, KFDB_MAX_WORDS);
    if (!kf_ascending(bow_id, nbow, db->nwords)) return orbhip_set_error(ORBHIP_ERR_INVALID, "BowVector ids must ascend and lie below %d", db->nwords);
    if (nbow > 0) {
        KFCHK(hipMemcpyAsync(db->d_qid, bow_id, (size_t)nbow * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        KFCHK(hipMemcpyAsync(db->d_qval, bow_val, (size_t)nbow * sizeof(double), hipMemcpyHostToDevice, s));
    }
    return ORBHIP_OK;
}

extern "C" orbhip_status orbhip_kfdb_query(orbhip_kfdb* db, int kind, uint64_t qid, const uint32_t* bow_id, const double* bow_val, int nbow,
                                           const int32_t* excluded_slots, int nexcluded, float min_score,
                                           orbhip_kfdb_hit* hits, int cap, int* nhits, int* nsharing, int* min_common)
{
    OrbApiTimer api_timer;
    if (!db || !nhits || nbow < 0 || cap < 0 || nexcluded < 0 || (kind != ORBHIP_KFDB_RELOC && kind != ORBHIP_KFDB_LOOP) || (nbow > 0 && (!bow_id || !bow_val)) ||
        (cap > 0 && !hits) || (nexcluded > 0 && !excluded_slots))
        return orbhip_set_error(ORBHIP_ERR_INVALID, "bad argument");
    std::lock_guard<std::mutex> lock(db->m);
    KFCHK(hipSetDevice(db->device));
    hipStream_t s = orbhip_thread_stream(db->device);
    const orbhip_status st = kf_upload_query(db, bow_id, bow_val, nbow, s); if (st != ORBHIP_OK) return st;
    return kf_query_core(db, kind, qid, db->d_qid, db->d_qval, nullptr, nbow, nbow, excluded_slots, nexcluded, min_score, hits, cap, nhits, nsharing, min_common, s);
}

extern "C" orbhip_status orbhip_kfdb_query_frame(orbhip_kfdb* db, int kind, uint64_t qid, orbhip_ctx* ctx, orbhip_voc* voc, int frame,
                                                 const int32_t* excluded_slots, int nexcluded, float min_score,
                                                 orbhip_kfdb_hit* hits, int cap, int* nhits, int* nsharing, int* min_common)
{
    OrbApiTimer api_timer;
    if (!db || !ctx || !voc || !nhits || cap < 0 || nexcluded < 0 || (kind != ORBHIP_KFDB_RELOC && kind != ORBHIP_KFDB_LOOP) || (cap > 0 && !hits) || (nexcluded > 0 && !excluded_slots))
        return orbhip_set_error(ORBHIP_ERR_INVALID, "bad argument");
    const uint32_t* d_id = nullptr; const double* d_val = nullptr; const int* d_n = nullptr; int qcap = 0, device = 0, nwords = 0; hipStream_t s = nullptr;
    const orbhip_status st = orbhip_bow_resident(ctx, voc, frame, &d_id, &d_val, &d_n, &qcap, &device, &nwords, &s); if (st != ORBHIP_OK) return st;
    if (device != db->device || nwords != db->nwords) return orbhip_set_error(ORBHIP_ERR_INVALID, "database for %d words on device %d, vocabulary of %d words on device %d", db->nwords, db->device, nwords, device);
    std::lock_guard<std::mutex> lock(db->m);
    KFCHK(hipSetDevice(db->device));
    return kf_query_core(db, kind, qid, d_id, d_val, d_n, 0, std::min(qcap, KFDB_MAX_WORDS), excluded_slots, nexcluded, min_score, hits, cap, nhits, nsharing, min_common, s);     // on the extractor's stream: behind orbhip_compute_bow
}

extern "C" orbhip_status orbhip_kfdb_state(orbhip_kfdb* db, int kind, int slot, uint64_t* query, int* words, float* score)
{
    if (!db || (kind != ORBHIP_KFDB_RELOC && kind != ORBHIP_KFDB_LOOP)) return orbhip_set_error(ORBHIP_ERR_INVALID, "bad argument");
    std::lock_guard<std::mutex> lock(db->m);
    if (!kf_live(db, slot)) return orbhip_set_error(ORBHIP_ERR_INVALID, "slot %d holds no key frame", slot);
    KFCHK(hipSetDevice(db->device));
    hipStream_t s = orbhip_thread_stream(db->device);
    KfState st;
    KFCHK(hipMemcpyAsync(&st, db->d_state[kind] + slot, sizeof st, hipMemcpyDeviceToHost, s));
    KFCHK(hipStreamSynchronize(s));
    if (query) *query = st.query;
    if (words) *words = st.words;
    if (score) *score = st.score;
    return ORBHIP_OK;
}

extern "C" orbhip_status orbhip_kfdb_scores(orbhip_kfdb* db, const uint32_t* bow_id, const double* bow_val, int nbow, const int32_t* slots, int n, double* scores)
{
    OrbApiTimer api_timer;
    if (!db || nbow < 0 || n < 0 || (nbow > 0 && (!bow_id || !bow_val)) || (n > 0 && (!slots || !scores))) return orbhip_set_error(ORBHIP_ERR_INVALID, "bad argument");
    std::lock_guard<std::mutex> lock(db->m);
    for (int i = 0; i < n; i++) if (!kf_live(db, slots[i])) return orbhip_set_error(ORBHIP_ERR_INVALID, "slot %d holds no key frame", slots[i]);
    KFCHK(hipSetDevice(db->device));
    hipStream_t s = orbhip_thread_stream(db->device);
    const orbhip_status st = kf_upload_query(db, bow_id, bow_val, nbow, s); if (st != ORBHIP_OK) return st;
    for (int o = 0; o < n; o += db->slot_cap) {                                   // (one launch unless key frames are named more often than the database has slots)
        const int m = std::min(n - o, db->slot_cap);
        KFCHK(kf_grow(&db->d_list, &db->list_cap, (size_t)m));
        KFCHK(hipMemcpyAsync(db->d_list, slots + o, (size_t)m * sizeof(int), hipMemcpyHostToDevice, s));
        kf_launch_scan(db, db->d_list, m, db->d_qid, db->d_qval, nullptr, nbow, nbow, s);
        KFCHK(hipGetLastError());
        KFCHK(hipMemcpyAsync(scores + o, db->d_score, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, s));
        KFCHK(hipStreamSynchronize(s));
    }
    return ORBHIP_OK;
}

// The covisibility accumulation over gathered neighbour states: list[j] the neighbour's slot (< 0: not in the database), ns[j] its state, j as neigh_off counts
static void kf_select_host(int kind, unsigned long long qid, int min_common, float min_score, const orbhip_kfdb_hit* hits, int nhits,
                           const int32_t* neigh_off, const int* list, const KfState* ns, int nslots, std::vector<int>& picked)
{
    std::vector<float> acc((size_t)nhits); std::vector<int> best((size_t)nhits);
    float best_acc = kind == ORBHIP_KFDB_LOOP ? min_score : 0.0f;
    for (int i = 0; i < nhits; i++) {
        float best_score = hits[i].score, a = hits[i].score; int best_slot = hits[i].slot;
        for (int j = neigh_off[i]; j < neigh_off[i + 1]; j++) {
            if (list[j] < 0) continue;
            const KfState& st = ns[j];
            if (st.query != qid) continue;
            if (kind == ORBHIP_KFDB_LOOP && !(st.words > min_common)) continue;
            a += st.score;
            if (st.score > best_score) { best_slot = list[j]; best_score = st.score; }
        }
        acc[i] = a; best[i] = best_slot;
        if (a > best_acc) best_acc = a;
    }
    const float retain = 0.75f * best_acc;
    picked.clear(); std::vector<char> seen((size_t)nslots, 0);                             // first occurrence wins (spAlreadyAddedKF)
    for (int i = 0; i < nhits; i++)
        if (acc[i] > retain && !seen[best[i]]) { seen[best[i]] = 1; picked.push_back(best[i]); }
}

// The covisibility accumulation (KeyFrameDatabase.cc:144-196 LOOP, :258-308 RELOC): f32 sums in neighbour order over the state the query left.
extern "C" orbhip_status orbhip_kfdb_select(orbhip_kfdb* db, int kind, uint64_t qid, int min_common, float min_score, const orbhip_kfdb_hit* hits, int nhits,
                                            const int32_t* neigh_off, const int32_t* neigh_slot, int32_t* out_slots, int cap, int* nout)
{
    OrbApiTimer api_timer;
    if (!db || !nout || nhits < 0 || cap < 0 || (kind != ORBHIP_KFDB_RELOC && kind != ORBHIP_KFDB_LOOP) || (nhits > 0 && (!hits || !neigh_off)) || (cap > 0 && !out_slots))
        return orbhip_set_error(ORBHIP_ERR_INVALID, "bad argument");
    *nout = 0;
    if (nhits == 0) return ORBHIP_OK;
    const int nn = neigh_off[nhits];
    if (neigh_off[0] != 0 || nn < 0 || (nn > 0 && !neigh_slot)) return orbhip_set_error(ORBHIP_ERR_INVALID, "bad neighbour lists");
    for (int i = 0; i < nhits; i++) if (neigh_off[i + 1] < neigh_off[i]) return orbhip_set_error(ORBHIP_ERR_INVALID, "bad neighbour lists");
    std::vector<KfState> ns((size_t)nn);
    std::vector<int> list((size_t)nn);
    int nslots = 0;
    {
        std::lock_guard<std::mutex> lock(db->m);
        nslots = db->nslots;
        for (int i = 0; i < nhits; i++) if (hits[i].slot < 0 || hits[i].slot >= nslots) return orbhip_set_error(ORBHIP_ERR_INVALID, "hit %d names slot %d", i, hits[i].slot);
        for (int j = 0; j < nn; j++) list[j] = kf_live(db, neigh_slot[j]) ? neigh_slot[j] : -1;      // a neighbour that is not in the database was never met by a query
        if (nn > 0) {
            KFCHK(hipSetDevice(db->device));
            hipStream_t s = orbhip_thread_stream(db->device);
            KFCHK(kf_grow(&db->d_list, &db->list_cap, (size_t)nn)); KFCHK(kf_grow(&db->d_gather, &db->gather_cap, (size_t)nn));
            KFCHK(hipMemcpyAsync(db->d_list, list.data(), (size_t)nn * sizeof(int), hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(k_kfdb_gather, dim3((nn + 255) / 256, 1, 1), dim3(256, 1, 1), 0, s, db->d_state[kind], db->d_list, nn, db->d_gather);
            KFCHK(hipGetLastError());
            KFCHK(hipMemcpyAsync(ns.data(), db->d_gather, (size_t)nn * sizeof(KfState), hipMemcpyDeviceToHost, s));
            KFCHK(hipStreamSynchronize(s));
        }
    }
    std::vector<int> picked;
    kf_select_host(kind, qid, min_common, min_score, hits, nhits, neigh_off, list.data(), ns.data(), nslots, picked);
    *nout = (int)picked.size();
    if (*nout > cap) return orbhip_set_error(ORBHIP_ERR_CAPACITY, "key-frame database: %d candidates, room for %d", *nout, cap);
    for (size_t i = 0; i < picked.size(); i++) out_slots[i] = picked[i];
    return ORBHIP_OK;
}

// ================================================================================================ batched queries
// orbhip_kfdb_query_batch / _query_frames answer nq queries in order under one hold of the lock with a fixed number of launches:
//   k_kfdb_scan_batch   a workgroup stages a TILE of queries' id lists in LDS (the host plans the tiles: at most KB_TQ queries and KB_IDS ids) and its four waves
//                       own a key frame each, several in turn; per (query, key frame) the count, the first shared word and the score of k_kfdb_scan, into
//                       [query][slot] matrices.  Tiles are the fast grid index, so the workgroups that read one key frame run together and its words come from HBM once.
//   k_kfdb_walk_words   one thread per slot steps through the queries in order with {query, words} in registers: k_kfdb_select's rule; the listed words
//                       replace the counts, the per-query maximum and listed count are reduced, and the snapshot's {query == qid, words} are written
//   k_kfdb_walk_score   the same walk for the score once every query's minCommonWords is known; snapshot's score, per-query hit counts
//   k_kfdb_sort_batch   one workgroup per query: compaction of its hits, their order, the hit list at its CSR offset
// The SNAPSHOT is, per (query, slot), the slot's state right after that query; orbhip_kfdb_select_batch gathers the neighbours' states from it.
#define KB_TQ 16                       // queries a tile holds at most
#define KB_IDS 8192                    // ids a tile holds at most (32 KiB of LDS: one query of KFDB_MAX_WORDS always fits)
#define KB_MAX_CELLS (1ll << 27)       // nq x slot capacity; 25 bytes of workspace per cell
#define KB_U 8                         // queries a walk loads ahead of its dependent chain

struct KfBq { long long id_off, val_off; int n, pad; };      // a query: byte offsets of its ids and weights from the batch's two base pointers, its length

struct KfBscanParams {
    const uint32_t* ids; const double* vals; const KfSlot* slots; int nslots;
    const uint32_t* q_id; const double* q_val; const KfBq* q;          // base pointers and the queries
    const int* tile_q0; int ntiles;                                     // tile t holds the queries [tile_q0[t], tile_q0[t + 1])
    int groups, gpb;                                                    // groups of four slots in all, groups per workgroup
    size_t stride;                                                      // row length of the matrices
    int* cnt; uint32_t* first; double* score;
};

template <int SC> __global__ __launch_bounds__(KS_T) void k_kfdb_scan_batch(KfBscanParams P)
{
    HIP_DYNAMIC_SHARED(uint32_t, q)
    __shared__ int s_off[KB_TQ + 1];
    __shared__ long long s_val[KB_TQ];
    const int tid = threadIdx.x, lane = tid & 63;
    const int tile = blockIdx.x % P.ntiles, gb = blockIdx.x / P.ntiles;
    const int q0 = P.tile_q0[tile], T = P.tile_q0[tile + 1] - q0;
    if (tid == 0) {
        int o = 0;
        for (int t = 0; t < T; t++) { s_off[t] = o; o += P.q[q0 + t].n; s_val[t] = P.q[q0 + t].val_off; }
        s_off[T] = o;
    }
    __syncthreads();
    for (int t = 0; t < T; t++) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(P.q_id) + P.q[q0 + t].id_off);
        const int o = s_off[t], n = s_off[t + 1] - o;
        for (int i = tid; i < n; i += KS_T) q[o + i] = src[i];
    }
    __syncthreads();
    for (int g = gb * P.gpb; g < (gb + 1) * P.gpb && g < P.groups; g++) {     // (whole waves, no barrier below)
        const int w = g * (KS_T / 64) + (tid >> 6);
        if (w >= P.nslots) break;
        const KfSlot S = P.slots[w];
        const uint32_t* kid = P.ids + S.off; const double* kval = P.vals + S.off;
        const bool any = S.live && S.n > 0;
        const uint32_t id0 = any && (unsigned)lane < S.n ? kid[lane] : 0xffffffffu;     // the first chunk's ids stay in a register for every query of the tile
        for (int t = 0; t < T; t++) {
            const uint32_t* ql = q + s_off[t]; const int nq = s_off[t + 1] - s_off[t];
            const double* qval = reinterpret_cast<const double*>(reinterpret_cast<const char*>(P.q_val) + s_val[t]);
            int top = 0;
            if (nq > 0) top = 1 << (31 - __clz(nq));
            int cnt = 0; uint32_t first = 0xffffffffu; double s = 0.0;
            if (any && nq > 0) {
                uint32_t id_next = id0;
                for (unsigned base = 0; base < S.n; base += 64) {
                    const unsigned i = base + lane; const bool in = i < S.n;
                    const uint32_t id = id_next;
                    id_next = i + 64 < S.n ? kid[i + 64] : 0xffffffffu;       // (after the tile's first query these come from the cache)
                    int pos = 0;
                    for (int st = top; st; st >>= 1) { const int p = pos + st; if (p <= nq && ql[p - 1] < id) pos = p; }
                    const bool hit = in && pos < nq && ql[pos] == id;
                    double term = 0.0;
                    if (hit) { const double wi = kval[i], vi = qval[pos]; term = kf_term<SC>(vi, wi); }
                    unsigned long long m = __ballot(hit);
                    if (m) {
                        if (cnt == 0) first = (uint32_t)__builtin_amdgcn_readlane((int)id, __ffsll((long long)m) - 1);
                        cnt += __popcll(m);
                        while (m) { const int l = __ffsll((long long)m) - 1; m &= m - 1; s = __dadd_rn(s, kf_readlane(term, l)); }      // ONE chain, ascending words
                    }
                }
            }
            if (lane == 0) { const size_t c = (size_t)(q0 + t) * P.stride + (size_t)w; P.cnt[c] = cnt; P.first[c] = first; P.score[c] = kf_result<SC>(s); }
        }
    }
}

struct KfBwalkParams {
    const KfSlot* slots; KfState* state; int nslots, nq, kind; size_t stride;
    const unsigned long long* qid; const float* min_score;
    const int* excl_off; const int* excl;                    // LOOP: per query the excluded slots, ascending
    int* cnt;                                                // in: shared words; out: words of a listed key frame, 0 otherwise
    const double* score;
    int* qmax; int* qnlist; int* qnhit;                      // per query
    int* s_words; float* s_score; unsigned char* s_match;    // the snapshot
};

__global__ __launch_bounds__(256) void k_kfdb_walk_words(KfBwalkParams P)
{
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    const bool in = i < P.nslots;
    const size_t col = in ? (size_t)i : 0;
    const bool live = in && P.slots[col].live;
    unsigned long long query = P.state[col].query; int words = P.state[col].words;
    for (int qb = 0; qb < P.nq; qb += KB_U) {
        int c[KB_U];
#pragma unroll
        for (int u = 0; u < KB_U; u++) c[u] = (live && qb + u < P.nq) ? P.cnt[(size_t)(qb + u) * P.stride + col] : 0;
#pragma unroll
        for (int u = 0; u < KB_U; u++) {
            const int qi = qb + u;
            if (qi >= P.nq) break;                                                                // (uniform)
            const unsigned long long qid = P.qid[qi];
            int listed = 0;
            if (c[u] >= 1) {
                if (query == qid) words += c[u];
                else {
                    bool excluded = false;
                    if (P.kind == ORBHIP_KFDB_LOOP) {
                        int lo = P.excl_off[qi]; const int end = P.excl_off[qi + 1]; int hi = end;
                        while (lo < hi) { const int mid = (lo + hi) >> 1; if (P.excl[mid] < i) lo = mid + 1; else hi = mid; }
                        excluded = lo < end && P.excl[lo] == i;
                    }
                    if (excluded) words = 1;
                    else { query = qid; words = c[u]; listed = c[u]; }
                }
            }
            if (in) {
                const size_t cell = (size_t)qi * P.stride + col;
                P.cnt[cell] = listed; P.s_words[cell] = words; P.s_match[cell] = query == qid;
            }
            int lmax = listed, nl = listed != 0;
            for (int o = 32; o; o >>= 1) { lmax = max(lmax, __shfl_xor(lmax, o)); nl += __shfl_xor(nl, o); }
            if (lane == 0 && nl) { atomicMax(&P.qmax[qi], lmax); atomicAdd(&P.qnlist[qi], nl); }
        }
    }
    if (in) { P.state[col].query = query; P.state[col].words = words; }
}

__global__ __launch_bounds__(256) void k_kfdb_walk_score(KfBwalkParams P)
{
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    const bool in = i < P.nslots;
    const size_t col = in ? (size_t)i : 0;
    float score = P.state[col].score;
    for (int qb = 0; qb < P.nq; qb += KB_U) {
        int l[KB_U];
#pragma unroll
        for (int u = 0; u < KB_U; u++) l[u] = (in && qb + u < P.nq) ? P.cnt[(size_t)(qb + u) * P.stride + col] : 0;
#pragma unroll
        for (int u = 0; u < KB_U; u++) {
            const int qi = qb + u;
            if (qi >= P.nq) break;
            const int minc = (int)__fmul_rn((float)P.qmax[qi], 0.8f);
            const size_t cell = (size_t)qi * P.stride + col;
            bool hit = false;
            if (l[u] > minc) { score = (float)P.score[cell]; hit = P.kind == ORBHIP_KFDB_RELOC || score >= P.min_score[qi]; }
            if (in) P.s_score[cell] = score;
            const unsigned long long m = __ballot(hit);
            if (lane == 0 && m) atomicAdd(&P.qnhit[qi], (int)__popcll(m));
        }
    }
    if (in) P.state[col].score = score;
}

struct KfBsortParams {
    const KfSlot* slots; int nslots, kind; size_t stride;
    const int* cnt; const uint32_t* first; const double* score;      // cnt: the listed words
    const float* min_score; const int* qmax; const int* qnhit;
    const int* hit_off; const long long* key_off;            // per query: where its hits go; where its sort workspace lies (< 0: the LDS)
    unsigned long long* keys; int* pay; orbhip_kfdb_hit* hits;
};

__global__ __launch_bounds__(KSEL_T) void k_kfdb_sort_batch(KfBsortParams P)
{
    __shared__ int s_nhit;
    __shared__ unsigned long long s_key[KSEL_LDS];
    __shared__ int s_pay[KSEL_LDS];
    const int tid = threadIdx.x, lane = tid & 63, qi = blockIdx.x;
    const int n = P.qnhit[qi];
    if (n == 0) return;                                                                           // (the whole workgroup)
    if (tid == 0) s_nhit = 0;
    __syncthreads();
    const int minc = (int)__fmul_rn((float)P.qmax[qi], 0.8f);
    const float min_score = P.min_score[qi];
    const long long ko = P.key_off[qi];
    const bool in_lds = ko < 0;
    unsigned long long* gkey = P.keys + (in_lds ? 0 : ko); int* gpay = P.pay + (in_lds ? 0 : ko);
    const int* cnt = P.cnt + (size_t)qi * P.stride; const uint32_t* first = P.first + (size_t)qi * P.stride; const double* score = P.score + (size_t)qi * P.stride;
    for (int b = 0; b < P.nslots; b += KSEL_T) {
        const int i = b + tid;
        bool hit = false; unsigned long long key = 0;
        if (i < P.nslots && cnt[i] > minc) {
            hit = P.kind == ORBHIP_KFDB_RELOC || (float)score[i] >= min_score;
            key = ((unsigned long long)first[i] << 32) | P.slots[i].seq;
        }
        const unsigned long long m = __ballot(hit);
        if (m) {
            const int leader = __ffsll((long long)m) - 1;
            int base = 0;
            if (lane == leader) base = atomicAdd(&s_nhit, (int)__popcll(m));
            base = __builtin_amdgcn_readlane(base, leader);
            const int pos = base + (int)__popcll(m & ((1ull << lane) - 1ull));
            if (hit && pos < n) { if (in_lds) { s_key[pos] = key; s_pay[pos] = i; } else { gkey[pos] = key; gpay[pos] = i; } }
        }
    }
    __syncthreads();
    int n2 = 1; while (n2 < n) n2 <<= 1;
    orbhip_kfdb_hit* out = P.hits + P.hit_off[qi];
    if (in_lds) {
        for (int t = n + tid; t < n2; t += KSEL_T) { s_key[t] = ~0ull; s_pay[t] = 0; }
        __syncthreads();
        kf_bitonic(s_key, s_pay, n2, tid);
        for (int t = tid; t < n; t += KSEL_T) { const int slot = s_pay[t]; orbhip_kfdb_hit h; h.slot = slot; h.words = cnt[slot]; h.score = (float)score[slot]; out[t] = h; }
    } else {
        for (int t = n + tid; t < n2; t += KSEL_T) { gkey[t] = ~0ull; gpay[t] = 0; }
        __syncthreads();
        kf_bitonic(gkey, gpay, n2, tid);
        for (int t = tid; t < n; t += KSEL_T) { const int slot = gpay[t]; orbhip_kfdb_hit h; h.slot = slot; h.words = cnt[slot]; h.score = (float)score[slot]; out[t] = h; }
    }
}

// the snapshot's cells named by list (cell index, < 0: zeros) as KfState: query = 1 where the slot's query was the cell's query id
__global__ __launch_bounds__(256) void k_kfdb_gather_batch(const int* s_words, const float* s_score, const unsigned char* s_match, const long long* list, int n, KfState* out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long cell = list[i];
    unsigned long long query = 0; int words = 0; float score = 0.0f;
    if (cell >= 0) { query = s_match[cell]; words = s_words[cell]; score = s_score[cell]; }
    out[i].query = query; out[i].words = words; out[i].score = score;
}

struct KfBatch {
    // workspace: the matrices, the per-query arrays, the uploaded batch
    int* d_cnt = nullptr; uint32_t* d_first = nullptr; double* d_score = nullptr; int* d_swords = nullptr; float* d_sscore = nullptr; unsigned char* d_smatch = nullptr; size_t cells = 0;
    int* d_meta = nullptr; size_t meta_cap = 0;                                                  // qmax, qnlist, qnhit: nq each
    uint32_t* d_qid = nullptr; size_t qid_cap = 0; double* d_qval = nullptr; size_t qval_cap = 0;
    KfBq* d_q = nullptr; size_t q_cap = 0; int* d_tile = nullptr; size_t tile_cap = 0; unsigned long long* d_qids = nullptr; size_t qids_cap = 0; float* d_minscore = nullptr; size_t minscore_cap = 0;
    int* d_excl_off = nullptr; size_t excl_off_cap = 0; int* d_excl = nullptr; size_t excl_cap = 0; int* d_lens = nullptr; size_t lens_cap = 0;
    int* d_hit_off = nullptr; size_t hit_off_cap = 0; long long* d_key_off = nullptr; size_t key_off_cap = 0;
    unsigned long long* d_keys = nullptr; size_t keys_cap = 0; int* d_pay = nullptr; size_t pay_cap = 0; orbhip_kfdb_hit* d_hits = nullptr; size_t hits_cap = 0;
    long long* d_cells = nullptr; size_t cells_cap = 0; KfState* d_gather = nullptr; size_t gather_cap = 0;
    // the snapshot's books
    bool valid = false; uint64_t token = 0; int kind = 0, nq = 0, nslots = 0; size_t stride = 0; unsigned next_seq = 0;
    std::vector<unsigned long long> qid; std::vector<float> min_score; std::vector<int> min_common, hit_off;
};

static void kf_batch_free(KfBatch* b)
{
    if (!b) return;
    void* ptrs[] = {b->d_cnt, b->d_first, b->d_score, b->d_swords, b->d_sscore, b->d_smatch, b->d_meta, b->d_qid, b->d_qval, b->d_q, b->d_tile, b->d_qids, b->d_minscore, b->d_excl_off, b->d_excl,
                    b->d_lens, b->d_hit_off, b->d_key_off, b->d_keys, b->d_pay, b->d_hits, b->d_cells, b->d_gather};
    for (void* p : ptrs) kf_free(p);
    delete b;
}
static void kf_batch_supersede(KfBatch* b) { if (b) b->valid = false; }

template <typename T> static hipError_t kf_fit(T** p, size_t* cap, size_t need)                  // exactly `need` elements when the array is too small (the matrices are large)
{
    if (need <= *cap) return hipSuccess;
    kf_free(*p); *p = nullptr; *cap = 0;
    const hipError_t e = orbhip_dmalloc((void**)p, need * sizeof(T));
    if (e == hipSuccess) *cap = need;
    return e;
}
template <typename T> static hipError_t kf_put(T** p, size_t* cap, const std::vector<T>& v, hipStream_t s)      // v stays until the stream is drained
{
    hipError_t e = kf_grow(p, cap, std::max<size_t>(v.size(), 1)); if (e != hipSuccess) return e;
    if (!v.empty()) e = hipMemcpyAsync(*p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s);
    return e;
}

// The batch on stream s, the database's lock held: the queries' BowVectors are on the device (ids at q_id + bq[i].id_off, weights at q_val + bq[i].val_off).
static orbhip_status kf_batch_core(orbhip_kfdb* db, int kind, int nq, const uint64_t* qids, const uint32_t* d_qid, const double* d_qval, const std::vector<KfBq>& bq,
                                   const int32_t* excl_off, const int32_t* excl_slot, const float* min_score,
                                   int32_t* hit_off, int32_t* nsharing, int32_t* min_common, orbhip_kfdb_hit* hits, int cap, uint64_t* token, hipStream_t s)
{
    KfBatch* B = db->batch;
    B->valid = false;
    const int nslots = db->nslots; const size_t stride = ((size_t)nslots + 63) & ~(size_t)63, cells = (size_t)nq * stride;
    B->qid.assign(qids, qids + nq);
    B->min_score.assign((size_t)nq, 0.0f); if (kind == ORBHIP_KFDB_LOOP) B->min_score.assign(min_score, min_score + nq);
    B->min_common.assign((size_t)nq, 0); B->hit_off.assign((size_t)nq + 1, 0);
    std::vector<int> meta((size_t)3 * nq, 0);
    if (nslots > 0) {
        // the tiles: consecutive queries while their ids fit
        std::vector<int> tile(1, 0); int ids = 0, maxids = 1;
        for (int i = 0; i < nq; i++) {
            if (i > tile.back() && (i - tile.back() == KB_TQ || ids + bq[i].n > KB_IDS)) { tile.push_back(i); ids = 0; }
            ids += bq[i].n; maxids = std::max(maxids, ids);
        }
        tile.push_back(nq);
        const int ntiles = (int)tile.size() - 1;
        std::vector<int> eoff((size_t)nq + 1, 0), excl;
        if (kind == ORBHIP_KFDB_LOOP)
            for (int i = 0; i < nq; i++) {
                const size_t b = excl.size();
                for (int j = excl_off[i]; j < excl_off[i + 1]; j++) if (excl_slot[j] >= 0 && excl_slot[j] < nslots) excl.push_back(excl_slot[j]);
                std::sort(excl.begin() + b, excl.end()); excl.erase(std::unique(excl.begin() + b, excl.end()), excl.end());
                eoff[i + 1] = (int)excl.size();
            }
        if (cells > B->cells) {                                           // the six matrices grow together
            size_t c[6] = {0, 0, 0, 0, 0, 0}; B->cells = 0;
            KFCHK(kf_fit(&B->d_cnt, &c[0], cells)); KFCHK(kf_fit(&B->d_first, &c[1], cells)); KFCHK(kf_fit(&B->d_score, &c[2], cells));
            KFCHK(kf_fit(&B->d_swords, &c[3], cells)); KFCHK(kf_fit(&B->d_sscore, &c[4], cells)); KFCHK(kf_fit(&B->d_smatch, &c[5], cells));
            B->cells = cells;
        }
        std::vector<unsigned long long> q64(qids, qids + nq);
        KFCHK(kf_put(&B->d_q, &B->q_cap, bq, s)); KFCHK(kf_put(&B->d_tile, &B->tile_cap, tile, s)); KFCHK(kf_put(&B->d_qids, &B->qids_cap, q64, s));
        KFCHK(kf_put(&B->d_minscore, &B->minscore_cap, B->min_score, s)); KFCHK(kf_put(&B->d_excl_off, &B->excl_off_cap, eoff, s)); KFCHK(kf_put(&B->d_excl, &B->excl_cap, excl, s));
        KFCHK(kf_grow(&B->d_meta, &B->meta_cap, meta.size()));
        KFCHK(hipMemsetAsync(B->d_meta, 0, meta.size() * sizeof(int), s));
        KfBscanParams P; memset(&P, 0, sizeof P);
        P.ids = db->d_ids; P.vals = db->d_vals; P.slots = db->d_slots; P.nslots = nslots; P.q_id = d_qid; P.q_val = d_qval; P.q = B->d_q; P.tile_q0 = B->d_tile; P.ntiles = ntiles;
        P.groups = (nslots + KS_T / 64 - 1) / (KS_T / 64);
        P.gpb = (int)std::min<long long>(16, std::max<long long>(1, (long long)P.groups * ntiles / 8192));      // enough workgroups to fill the device, then fewer stagings of the tile
        P.stride = stride; P.cnt = B->d_cnt; P.first = B->d_first; P.score = B->d_score;
        const long long nblocks = (long long)((P.groups + P.gpb - 1) / P.gpb) * ntiles;
        if (nblocks > 0x7fffffffll) return orbhip_set_error(ORBHIP_ERR_UNSUPPORTED, "key-frame database: a batch of %lld workgroups", nblocks);
        const dim3 g((unsigned)nblocks, 1, 1), b(KS_T, 1, 1); const size_t lds = (size_t)maxids * sizeof(uint32_t);
        switch (db->scoring) {
        case 1: hipLaunchKernelGGL(k_kfdb_scan_batch<1>, g, b, lds, s, P); break;
        case 2: hipLaunchKernelGGL(k_kfdb_scan_batch<2>, g, b, lds, s, P); break;
        case 4: hipLaunchKernelGGL(k_kfdb_scan_batch<4>, g, b, lds, s, P); break;
        case 5: hipLaunchKernelGGL(k_kfdb_scan_batch<5>, g, b, lds, s, P); break;
        default: hipLaunchKernelGGL(k_kfdb_scan_batch<0>, g, b, lds, s, P); break;
        }
        KFCHK(hipGetLastError());
        KfBwalkParams W; memset(&W, 0, sizeof W);
        W.slots = db->d_slots; W.state = db->d_state[kind]; W.nslots = nslots; W.nq = nq; W.kind = kind; W.stride = stride; W.qid = B->d_qids; W.min_score = B->d_minscore;
        W.excl_off = B->d_excl_off; W.excl = B->d_excl; W.cnt = B->d_cnt; W.score = B->d_score; W.qmax = B->d_meta; W.qnlist = B->d_meta + nq; W.qnhit = B->d_meta + 2 * (size_t)nq;
        W.s_words = B->d_swords; W.s_score = B->d_sscore; W.s_match = B->d_smatch;
        const dim3 wg((unsigned)((nslots + 255) / 256), 1, 1), wb(256, 1, 1);
        hipLaunchKernelGGL(k_kfdb_walk_words, wg, wb, 0, s, W);
        hipLaunchKernelGGL(k_kfdb_walk_score, wg, wb, 0, s, W);
        KFCHK(hipGetLastError());
        KFCHK(hipMemcpyAsync(meta.data(), B->d_meta, meta.size() * sizeof(int), hipMemcpyDeviceToHost, s));
        KFCHK(hipStreamSynchronize(s));                                   // the key frames' state is that of the completed batch from here on
        std::vector<long long> koff((size_t)nq, -1); long long nkeys = 0;
        for (int i = 0; i < nq; i++) {
            const int nh = meta[2 * (size_t)nq + i];
            if (nh < 0 || nh > nslots) return orbhip_set_error(ORBHIP_ERR_HIP, "key-frame database: %d hits among %d slots", nh, nslots);
            B->hit_off[i + 1] = B->hit_off[i] + nh;
            B->min_common[i] = meta[(size_t)nq + i] ? (int)((float)meta[i] * 0.8f) : 0;
            if (nh > KSEL_LDS) { koff[i] = nkeys; long long n2 = 1; while (n2 < nh) n2 <<= 1; nkeys += n2; }
        }
        const int total = B->hit_off[nq];
        if (total > 0) {
            KFCHK(kf_put(&B->d_hit_off, &B->hit_off_cap, B->hit_off, s)); KFCHK(kf_put(&B->d_key_off, &B->key_off_cap, koff, s));
            KFCHK(kf_grow(&B->d_keys, &B->keys_cap, (size_t)std::max<long long>(nkeys, 1))); KFCHK(kf_grow(&B->d_pay, &B->pay_cap, (size_t)std::max<long long>(nkeys, 1)));
            KFCHK(kf_grow(&B->d_hits, &B->hits_cap, (size_t)total));
            KfBsortParams Q; memset(&Q, 0, sizeof Q);
            Q.slots = db->d_slots; Q.nslots = nslots; Q.kind = kind; Q.stride = stride; Q.cnt = B->d_cnt; Q.first = B->d_first; Q.score = B->d_score; Q.min_score = B->d_minscore;
            Q.qmax = B->d_meta; Q.qnhit = B->d_meta + 2 * (size_t)nq; Q.hit_off = B->d_hit_off; Q.key_off = B->d_key_off; Q.keys = B->d_keys; Q.pay = B->d_pay; Q.hits = B->d_hits;
            hipLaunchKernelGGL(k_kfdb_sort_batch, dim3((unsigned)nq, 1, 1), dim3(KSEL_T, 1, 1), 0, s, Q);
            KFCHK(hipGetLastError());
            if (hits && cap >= total) KFCHK(hipMemcpyAsync(hits, B->d_hits, (size_t)total * sizeof(orbhip_kfdb_hit), hipMemcpyDeviceToHost, s));
            KFCHK(hipStreamSynchronize(s));
        }
    }
    for (int i = 0; i <= nq; i++) hit_off[i] = B->hit_off[i];
    for (int i = 0; i < nq; i++) { if (nsharing) nsharing[i] = meta[(size_t)nq + i]; if (min_common) min_common[i] = B->min_common[i]; }
    B->kind = kind; B->nq = nq; B->nslots = nslots; B->stride = stride; B->next_seq = db->next_seq; B->token = ++db->batch_tokens; B->valid = true;
    *token = B->token;
    if (hits && cap < B->hit_off[nq])
        return orbhip_set_error(ORBHIP_ERR_CAPACITY, "key-frame database: %d hits, room for %d (the key frames' state is that of the completed batch; orbhip_kfdb_batch_hits delivers)", B->hit_off[nq], cap);
    return ORBHIP_OK;
}

static orbhip_status kf_batch_args(orbhip_kfdb* db, int kind, int nq, const uint64_t* qids, const int32_t* excl_off, const int32_t* excl_slot, const float* min_score,
                                   int32_t* hit_off, int cap, uint64_t* token)
{
    if (!db || !token || nq < 0 || cap < 0 || (kind != ORBHIP_KFDB_RELOC && kind != ORBHIP_KFDB_LOOP) || !hit_off || (nq > 0 && !qids))
        return orbhip_set_error(ORBHIP_ERR_INVALID, "bad argument");
    if (kind == ORBHIP_KFDB_LOOP && nq > 0) {
        if (!excl_off || !min_score || excl_off[0] != 0) return orbhip_set_error(ORBHIP_ERR_INVALID, "a LOOP batch needs excluded lists and minimum scores");
        for (int i = 0; i < nq; i++) if (excl_off[i + 1] < excl_off[i]) return orbhip_set_error(ORBHIP_ERR_INVALID, "bad excluded lists");
        if (excl_off[nq] > 0 && !excl_slot) return orbhip_set_error(ORBHIP_ERR_INVALID, "bad excluded lists");
    }
    return ORBHIP_OK;
}

static orbhip_status kf_batch_room(orbhip_kfdb* db, int nq)       // the lock held
{
    if ((long long)nq * (long long)std::max(db->slot_cap, 64) > KB_MAX_CELLS)
        return orbhip_set_error(ORBHIP_ERR_UNSUPPORTED, "key-frame database: %d queries x %d slots exceed %lld cells: split the batch", nq, std::max(db->slot_cap, 64), (long long)KB_MAX_CELLS);
    if (!db->batch) db->batch = new KfBatch();
    return ORBHIP_OK;
}

extern "C" orbhip_status orbhip_kfdb_query_batch(orbhip_kfdb* db, int kind, int nq, const uint64_t* qids, const int32_t* bow_off, const uint32_t* bow_id, const double* bow_val,
                                                 const int32_t* excl_off, const int32_t* excl_slot, const float* min_score,
                                                 int32_t* hit_off, int32_t* nsharing, int32_t* min_common, orbhip_kfdb_hit* hits, int cap, uint64_t* batch_token)
{
    OrbApiTimer api_timer;
    orbhip_status st = kf_batch_args(db, kind, nq, qids, excl_off, excl_slot, min_score, hit_off, cap, batch_token); if (st != ORBHIP_OK) return st;
    *batch_token = 0; hit_off[0] = 0;
    if (nq == 0) return ORBHIP_OK;
    if (!bow_off || bow_off[0] < 0) return orbhip_set_error(ORBHIP_ERR_INVALID, "bad argument");
    std::lock_guard<std::mutex> lock(db->m);
    st = kf_batch_room(db, nq); if (st != ORBHIP_OK) return st;
    for (int i = 0; i < nq; i++) {
        const long long n = (long long)bow_off[i + 1] - bow_off[i];
        if (n < 0 || (n > 0 && (!bow_id || !bow_val))) return orbhip_set_error(ORBHIP_ERR_INVALID, "bad argument");
        if (n > KFDB_MAX_WORDS) return orbhip_set_error(ORBHIP_ERR_UNSUPPORTED, "query %d: a BowVector of %lld words (at most %d)", i, n, KFDB_MAX_WORDS);
        if (!kf_ascending(bow_id + bow_off[i], (int)n, db->nwords)) return orbhip_set_error(ORBHIP_ERR_INVALID, "query %d: BowVector ids must ascend and lie below %d", i, db->nwords);
    }
    KFCHK(hipSetDevice(db->device));
    hipStream_t s = orbhip_thread_stream(db->device);
    KfBatch* B = db->batch;
    const size_t b0 = (size_t)bow_off[0], nb = (size_t)bow_off[nq] - b0;
    std::vector<KfBq> bq((size_t)nq);
    for (int i = 0; i < nq; i++) { bq[i].id_off = (long long)((size_t)bow_off[i] - b0) * 4; bq[i].val_off = (long long)((size_t)bow_off[i] - b0) * 8; bq[i].n = bow_off[i + 1] - bow_off[i]; bq[i].pad = 0; }
    KFCHK(kf_grow(&B->d_qid, &B->qid_cap, std::max<size_t>(nb, 1))); KFCHK(kf_grow(&B->d_qval, &B->qval_cap, std::max<size_t>(nb, 1)));
    if (nb > 0) {
        KFCHK(hipMemcpyAsync(B->d_qid, bow_id + b0, nb * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        KFCHK(hipMemcpyAsync(B->d_qval, bow_val + b0, nb * sizeof(double), hipMemcpyHostToDevice, s));
    }
    return kf_batch_core(db, kind, nq, qids, B->d_qid, B->d_qval, bq, excl_off, excl_slot, min_score, hit_off, nsharing, min_common, hits, cap, batch_token, s);
}

extern "C" orbhip_status orbhip_kfdb_query_frames(orbhip_kfdb* db, int kind, const uint64_t* qids, orbhip_ctx* ctx, orbhip_voc* voc, int first_frame, int nq,
                                                  const int32_t* excl_off, const int32_t* excl_slot, const float* min_score,
                                                  int32_t* hit_off, int32_t* nsharing, int32_t* min_common, orbhip_kfdb_hit* hits, int cap, uint64_t* batch_token)
{
    OrbApiTimer api_timer;
    orbhip_status st = kf_batch_args(db, kind, nq, qids, excl_off, excl_slot, min_score, hit_off, cap, batch_token); if (st != ORBHIP_OK) return st;
    if (!ctx || !voc) return orbhip_set_error(ORBHIP_ERR_INVALID, "bad argument");
    *batch_token = 0; hit_off[0] = 0;
    if (nq == 0) return ORBHIP_OK;
    const uint32_t* d_id0 = nullptr; const double* d_val0 = nullptr; const int* d_n0 = nullptr; int qcap = 0, device = 0, nwords = 0; hipStream_t s = nullptr;
    std::vector<KfBq> bq((size_t)nq);
    long long n_pitch = 0;
    for (int i = 0; i < nq; i++) {
        const uint32_t* d_id = nullptr; const double* d_val = nullptr; const int* d_n = nullptr;
        st = orbhip_bow_resident(ctx, voc, first_frame + i, &d_id, &d_val, &d_n, &qcap, &device, &nwords, &s); if (st != ORBHIP_OK) return st;
        if (i == 0) { d_id0 = d_id; d_val0 = d_val; d_n0 = d_n; }
        bq[i].id_off = reinterpret_cast<const char*>(d_id) - reinterpret_cast<const char*>(d_id0); bq[i].val_off = reinterpret_cast<const char*>(d_val) - reinterpret_cast<const char*>(d_val0);
        bq[i].n = 0; bq[i].pad = 0;
        if (i == 1) n_pitch = reinterpret_cast<const char*>(d_n) - reinterpret_cast<const char*>(d_n0);
    }
    if (device != db->device || nwords != db->nwords) return orbhip_set_error(ORBHIP_ERR_INVALID, "database for %d words on device %d, vocabulary of %d words on device %d", db->nwords, db->device, nwords, device);
    std::lock_guard<std::mutex> lock(db->m);
    st = kf_batch_room(db, nq); if (st != ORBHIP_OK) return st;
    KFCHK(hipSetDevice(db->device));
    std::vector<int> lens((size_t)nq, 0);                                 // the tiles are planned on the host: one download of nq lengths, no BowVector travels
    KFCHK(hipMemcpy2DAsync(lens.data(), sizeof(int), d_n0, nq > 1 ? (size_t)n_pitch : sizeof(int), sizeof(int), (size_t)nq, hipMemcpyDeviceToHost, s));
    KFCHK(hipStreamSynchronize(s));
    for (int i = 0; i < nq; i++) bq[i].n = std::max(0, std::min(lens[i], std::min(qcap, KFDB_MAX_WORDS)));
    return kf_batch_core(db, kind, nq, qids, d_id0, d_val0, bq, excl_off, excl_slot, min_score, hit_off, nsharing, min_common, hits, cap, batch_token, s);     // on the extractor's stream: behind orbhip_compute_bow
}

static orbhip_status kf_batch_token(orbhip_kfdb* db, uint64_t token)      // the lock held
{
    if (!db->batch || !db->batch->valid || db->batch->token != token || token == 0)
        return orbhip_set_error(ORBHIP_ERR_INVALID, "key-frame database: batch token %llu is superseded (a later query or clear) or was never given", (unsigned long long)token);
    return ORBHIP_OK;
}

extern "C" orbhip_status orbhip_kfdb_batch_hits(orbhip_kfdb* db, uint64_t batch_token, int first_query, int nqueries, orbhip_kfdb_hit* hits, int cap)
{
    OrbApiTimer api_timer;
    if (!db || first_query < 0 || nqueries < 0 || cap < 0 || (cap > 0 && !hits)) return orbhip_set_error(ORBHIP_ERR_INVALID, "bad argument");
    std::lock_guard<std::mutex> lock(db->m);
    const orbhip_status st = kf_batch_token(db, batch_token); if (st != ORBHIP_OK) return st;
    KfBatch* B = db->batch;
    if ((long long)first_query + nqueries > B->nq) return orbhip_set_error(ORBHIP_ERR_INVALID, "queries %d..%d of a batch of %d", first_query, first_query + nqueries, B->nq);
    const int o = B->hit_off[first_query], n = B->hit_off[first_query + nqueries] - o;
    if (n > cap) return orbhip_set_error(ORBHIP_ERR_CAPACITY, "key-frame database: %d hits, room for %d", n, cap);
    if (n == 0) return ORBHIP_OK;
    KFCHK(hipSetDevice(db->device));
    hipStream_t s = orbhip_thread_stream(db->device);
    KFCHK(hipMemcpyAsync(hits, B->d_hits + o, (size_t)n * sizeof(orbhip_kfdb_hit), hipMemcpyDeviceToHost, s));
    KFCHK(hipStreamSynchronize(s));
    return ORBHIP_OK;
}

// orbhip_kfdb_select for every query of the batch, each over the states its neighbours had right after that query (the snapshot)
extern "C" orbhip_status orbhip_kfdb_select_batch(orbhip_kfdb* db, uint64_t batch_token, int kind, const orbhip_kfdb_hit* hits, const int32_t* hit_off,
                                                  const int32_t* neigh_off, const int32_t* neigh_slot, int32_t* out_slots, int32_t* out_off, int cap)
{
    OrbApiTimer api_timer;
    if (!db || !hit_off || !out_off || cap < 0 || (kind != ORBHIP_KFDB_RELOC && kind != ORBHIP_KFDB_LOOP) || (cap > 0 && !out_slots)) return orbhip_set_error(ORBHIP_ERR_INVALID, "bad argument");
    std::vector<int> list; std::vector<KfState> ns; std::vector<unsigned long long> qid; std::vector<float> min_score; std::vector<int> min_common;
    int nq = 0, nslots = 0, nh = 0;
    {
        std::lock_guard<std::mutex> lock(db->m);
        const orbhip_status st = kf_batch_token(db, batch_token); if (st != ORBHIP_OK) return st;
        KfBatch* B = db->batch;
        if (kind != B->kind) return orbhip_set_error(ORBHIP_ERR_INVALID, "the batch was of kind %d", B->kind);
        nq = B->nq; nslots = db->nslots; qid = B->qid; min_score = B->min_score; min_common = B->min_common;
        if (hit_off[0] != 0) return orbhip_set_error(ORBHIP_ERR_INVALID, "bad hit offsets");
        for (int i = 0; i < nq; i++) if (hit_off[i + 1] < hit_off[i]) return orbhip_set_error(ORBHIP_ERR_INVALID, "bad hit offsets");
        nh = hit_off[nq];
        if (nh > 0 && (!hits || !neigh_off)) return orbhip_set_error(ORBHIP_ERR_INVALID, "bad argument");
        const int nn = nh > 0 ? neigh_off[nh] : 0;
        if (nh > 0 && (neigh_off[0] != 0 || nn < 0 || (nn > 0 && !neigh_slot))) return orbhip_set_error(ORBHIP_ERR_INVALID, "bad neighbour lists");
        for (int i = 0; i < nh; i++) {
            if (neigh_off[i + 1] < neigh_off[i]) return orbhip_set_error(ORBHIP_ERR_INVALID, "bad neighbour lists");
            if (hits[i].slot < 0 || hits[i].slot >= nslots) return orbhip_set_error(ORBHIP_ERR_INVALID, "hit %d names slot %d", i, hits[i].slot);
        }
        list.resize((size_t)nn); ns.resize((size_t)nn);
        std::vector<long long> cell((size_t)nn);
        for (int q = 0; q < nq; q++)
            for (int i = hit_off[q]; i < hit_off[q + 1]; i++)
                for (int j = neigh_off[i]; j < neigh_off[i + 1]; j++) {
                    const int sl = neigh_slot[j];
                    list[j] = kf_live(db, sl) ? sl : -1;                                          // liveness as it is now, as orbhip_kfdb_select reads it
                    // a key frame added since the batch was never met by it: the zero state of a new slot
                    cell[j] = (list[j] >= 0 && sl < B->nslots && db->h_slots[sl].seq < B->next_seq) ? (long long)((size_t)q * B->stride + (size_t)sl) : -1;
                }
        if (nn > 0) {
            KFCHK(hipSetDevice(db->device));
            hipStream_t s = orbhip_thread_stream(db->device);
            KFCHK(kf_grow(&B->d_cells, &B->cells_cap, (size_t)nn)); KFCHK(kf_grow(&B->d_gather, &B->gather_cap, (size_t)nn));
            KFCHK(hipMemcpyAsync(B->d_cells, cell.data(), (size_t)nn * sizeof(long long), hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(k_kfdb_gather_batch, dim3((nn + 255) / 256, 1, 1), dim3(256, 1, 1), 0, s, B->d_swords, B->d_sscore, B->d_smatch, B->d_cells, nn, B->d_gather);
            KFCHK(hipGetLastError());
            KFCHK(hipMemcpyAsync(ns.data(), B->d_gather, (size_t)nn * sizeof(KfState), hipMemcpyDeviceToHost, s));
            KFCHK(hipStreamSynchronize(s));
        }
        for (int q = 0; q < nq; q++)
            for (int i = hit_off[q]; i < hit_off[q + 1]; i++)
                for (int j = neigh_off[i]; j < neigh_off[i + 1]; j++) {
                    if (cell[j] < 0) ns[j].query = 0; else ns[j].query = ns[j].query ? qid[q] : ~qid[q];      // (a new slot's query field is 0)
                }
    }
    std::vector<int> picked; int total = 0; bool fits = true;
    out_off[0] = 0;
    for (int q = 0; q < nq; q++) {
        const int h0 = hit_off[q], n = hit_off[q + 1] - h0;
        picked.clear();
        if (n > 0) kf_select_host(kind, qid[q], min_common[q], min_score[q], hits + h0, n, neigh_off + h0, list.data(), ns.data(), nslots, picked);
        if ((long long)total + (long long)picked.size() > cap) fits = false;
        if (fits) for (size_t i = 0; i < picked.size(); i++) out_slots[total + (int)i] = picked[i];
        total += (int)picked.size(); out_off[q + 1] = total;
    }
    if (!fits) return orbhip_set_error(ORBHIP_ERR_CAPACITY, "key-frame database: %d candidates, room for %d", total, cap);
    return ORBHIP_OK;
}
