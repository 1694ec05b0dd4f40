// orbhip_voc_train.hip — DBoW2's TemplatedVocabulary::create (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:558-616, :642-996) on gfx950.
//
// The reference is a depth-first recursion: HKmeansStep clusters a node's features with k-means++ seeding (:833-913) and Lloyd passes whose "mean" is the
// per-bit majority (FORB::meanValue, FORB.cpp:28-77), makes a child per cluster and recurses.  Sibling nodes own disjoint features, so here ALL nodes of a level
// run at once and the host walks the levels.  Everything that decides anything is an integer (Hamming distances, their u64 sums, bit counts), except the two
// f64 operations of the k-means++ cut (one division, one product, each rounded once: vt_cut), so the tree is the reference's bit for bit once the random
// stream is pinned per node (glibc's rand() restated in vt_rand_nth, reseeded for every node from the node's own key).
//
// Reference behaviour that is kept on purpose:
//   - a centre is a shallow copy of a training feature (clusters.push_back(*pfeatures[i])), and meanValue of a group of >= 2 writes the mean into that
//     buffer: training features are overwritten, permanently, and a node's descriptor is whatever its feature slot holds when create() ends.  A group of
//     exactly 1 replaces the centre by a clone: the alias ends.  A centre here is "feature slot f" (cent >= 0) or "own buffer" (cent == -1).
//   - inside a node the means of clusters 0 .. k-1 are computed one after the other, each reading the features as the earlier ones left them.  Counting
//     every cluster's bits BEFORE any mean is written is the same thing: the only features a pass writes are the aliased ones, feature f of cluster c at
//     step c; f holds exactly centre c's bytes whenever features are assigned (they share the buffer), so its distance to centre c is 0 and the first
//     minimum puts it into a cluster c' <= c, whose sum the reference takes before step c writes.  No cluster ever reads a byte this pass has written.
//
// Layout: idx[] lists the features node-major, in training order inside a node (stable).  A node's range is cut into chunks of at most VT_CHUNK positions;
// the per-feature kernels take a workgroup per chunk, the per-node ones a workgroup per node.
//   k_vt_seed_first / k_vt_seed_dist / k_vt_seed_pick   k-means++: first centre, min-distance update against the newest centre, u64 sum + first prefix >= cut
//   k_vt_assign     nearest centre (first minimum), per-feature cluster, changed flag per node
//   k_vt_count      per chunk: the chunk's descriptors staged in LDS, thread t owns bit t of all clusters' counters (LDS, no atomics); a node of one chunk is
//                   finished from LDS (vt_finalize), a node of several adds its chunks' counters into a table in device memory that only such nodes have
//                   (at most M / VT_CHUNK of them: k bytes per feature), finished by k_vt_mean_big
//   k_vt_hist / k_vt_scatter   the stable partition of a node's range by cluster at the end of a level (bases prefix-summed on the host, which needs the
//                   group sizes anyway to lay out the next level)
//   k_vt_docs       Ni of a word: features whose walk (k_bow_descend) ends in it and that are the first of their image to do so
#include "orbhip_ctx.h"
#include <climits>

#define VT_T 256
#define VT_CHUNK 1024                  // positions per chunk: 32 KB of descriptors + 32 KB of counters in LDS
#define VT_MAXK 32
#define VT_MAX_PASSES 512              // Lloyd passes of one level before the call gives up (the reference has no bound)

struct VtNode { int start, n, chunk0, nchunks, big; uint32_t seed; };      // big: the node's slot in the several-chunk counter table, or -1
struct VtChunk { int node, start, n; };

struct VtParams {
    uint32_t* desc;                    // [M][8] the features, overwritten like the reference's
    const int* idx; int* idx_out;      // [M] node-major feature indices; the next level's
    const VtNode* nodes; const VtChunk* chunks; const int* bignodes; int nnodes, nchunks, k;
    int* ncl; int* used;               // [node] centres so far; draws consumed
    int* cent; uint32_t* own;          // [node][k] feature slot or -1; [node][k][8] the centre's own buffer
    int* mind; uint8_t* asg;           // [position] k-means++ distance to the nearest centre; cluster
    int* active; int* changed;         // [node]
    uint32_t* bigcnt; int* biggs;      // [big][k][256], [big][k]
    int* chunk_cnt; const int* chunk_base;      // [chunk][k]
    int* stat;                         // [0] nodes that go on, [1] smallest node with an empty cluster
    int round, first_pass;
};

// the nth value (from 0) rand() returns after srand(seed): glibc's TYPE_3 additive feedback generator, r[i] = r[i-31] + r[i-3], started with 31 words of the
// 16807 Lehmer sequence, 310 values discarded, the top 31 bits returned (RAND_MAX = 2147483647)
__host__ __device__ inline uint32_t vt_rand_nth(uint32_t seed, int nth)
{
    uint32_t r[34];
    int32_t w = seed ? (int32_t)seed : 1;
    r[0] = (uint32_t)w;
    for (int i = 1; i < 31; i++) {
        const int32_t hi = w / 127773, lo = w % 127773;
        w = 16807 * lo - 2836 * hi;
        if (w < 0) w += 2147483647;
        r[i] = (uint32_t)w;
    }
    r[31] = r[0]; r[32] = r[1]; r[33] = r[2];
    const int last = 344 + nth;
    for (int i = 34; i <= last; i++) r[i % 34] = r[(i - 31) % 34] + r[(i - 3) % 34];
    return r[last % 34] >> 1;
}
// DUtils::Random::RandomValue<double>(0, dist_sum): one division, one product ("* (max - min) + min" with min = 0 is exact)
__host__ __device__ inline double vt_cut(uint32_t r, unsigned long long dist_sum) { const double u = (double)r / 2147483647.0; return u * (double)dist_sum; }

__device__ __forceinline__ int vt_distance(const uint32_t* a, const uint32_t* b)
{
    int d = 0;
#pragma unroll
    for (int w = 0; w < 8; w++) d += __popc(a[w] ^ b[w]);
    return d;
}

// :855-858  the first centre: RandomInt(0, n - 1) = int(rand() / (RAND_MAX + 1.0) * n)
__global__ __launch_bounds__(VT_T) void k_vt_seed_first(VtParams P)
{
    const int node = blockIdx.x * VT_T + threadIdx.x;
    if (node >= P.nnodes) return;
    const VtNode N = P.nodes[node];
    const uint32_t r = vt_rand_nth(N.seed, 0);
    const int i0 = (int)(((double)r / 2147483648.0) * (double)N.n);
    P.cent[(size_t)node * P.k] = P.idx[N.start + i0];
    P.ncl[node] = 1; P.used[node] = 1; P.active[node] = 1; P.changed[node] = 0;
}

// :860-880  distances to the newest centre (round - 1): all of them in round 1, afterwards only where the distance is still > 0 and gets smaller
__global__ __launch_bounds__(VT_T) void k_vt_seed_dist(VtParams P)
{
    const VtChunk C = P.chunks[blockIdx.x];
    if (P.ncl[C.node] != P.round) return;                                     // the node stopped early (dist_sum == 0)
    const int slot = P.cent[(size_t)C.node * P.k + P.round - 1];
    uint32_t c[8];
#pragma unroll
    for (int w = 0; w < 8; w++) c[w] = P.desc[(size_t)slot * 8 + w];
    for (int i = threadIdx.x; i < C.n; i += VT_T) {
        const int p = C.start + i;
        const int old = P.round == 1 ? INT_MAX : P.mind[p];
        if (old > 0) {
            uint32_t f[8];
            const uint32_t* src = P.desc + (size_t)P.idx[p] * 8;
#pragma unroll
            for (int w = 0; w < 8; w++) f[w] = src[w];
            const int d = vt_distance(f, c);
            if (d < old) P.mind[p] = d;
        }
    }
}

// :883-909  dist_sum, the cut, the first feature whose running sum reaches it.  One workgroup per node; thread t owns a contiguous piece of the node.
__global__ __launch_bounds__(VT_T) void k_vt_seed_pick(VtParams P)
{
    __shared__ unsigned long long s_sum[VT_T];
    __shared__ double s_cut;
    __shared__ int s_pick;
    const int node = blockIdx.x, t = threadIdx.x;
    if (P.ncl[node] != P.round) return;
    const VtNode N = P.nodes[node];
    const int per = (N.n + VT_T - 1) / VT_T, lo = min(t * per, N.n), hi = min(lo + per, N.n);
    const int* md = P.mind + N.start;
    unsigned long long sum = 0;
    for (int i = lo; i < hi; i++) sum += (unsigned long long)md[i];
    s_sum[t] = sum;
    if (t == 0) s_pick = N.n - 1;                                             // :900-901
    __syncthreads();
    unsigned long long base = 0, total = 0;
    for (int u = 0; u < VT_T; u++) { const unsigned long long v = s_sum[u]; total += v; if (u < t) base += v; }
    if (total == 0) return;                                                   // :907-909: the node keeps the centres it has
    if (t == 0) {
        int u = P.used[node]; double cut;
        do { cut = vt_cut(vt_rand_nth(N.seed, u++), total); } while (cut == 0.0);      // :887-891
        P.used[node] = u; s_cut = cut;
    }
    __syncthreads();
    const double cut = s_cut;
    unsigned long long run = base;
    for (int i = lo; i < hi; i++) {
        run += (unsigned long long)md[i];
        if ((double)run >= cut) { atomicMin(&s_pick, i); break; }             // integers below 2^53: the conversion is exact
    }
    __syncthreads();
    if (t == 0) { P.cent[(size_t)node * P.k + P.round] = P.idx[N.start + s_pick]; P.ncl[node] = P.round + 1; }
}

// :730-751  nearest centre, the first among equals
__global__ __launch_bounds__(VT_T) void k_vt_assign(VtParams P)
{
    __shared__ uint32_t s_c[VT_MAXK * 8];
    __shared__ int s_changed;
    const VtChunk C = P.chunks[blockIdx.x];
    if (!P.active[C.node]) return;
    const int nc = P.ncl[C.node], t = threadIdx.x;
    if (t < nc * 8) {
        const size_t ci = (size_t)C.node * P.k + (t >> 3);
        const int slot = P.cent[ci];
        s_c[t] = slot >= 0 ? P.desc[(size_t)slot * 8 + (t & 7)] : P.own[ci * 8 + (t & 7)];
    }
    if (t == 0) s_changed = 0;
    __syncthreads();
    int ch = 0;
    for (int i = t; i < C.n; i += VT_T) {
        const int p = C.start + i;
        const uint32_t* src = P.desc + (size_t)P.idx[p] * 8;
        uint32_t f[8];
#pragma unroll
        for (int w = 0; w < 8; w++) f[w] = src[w];
        int best = vt_distance(f, s_c), bc = 0;
        for (int c = 1; c < nc; c++) { const int d = vt_distance(f, s_c + c * 8); if (d < best) { best = d; bc = c; } }
        if (P.first_pass || P.asg[p] != bc) ch = 1;
        P.asg[p] = (uint8_t)bc;
    }
    if (ch) atomicOr(&s_changed, 1);
    __syncthreads();
    if (t == 0 && s_changed) atomicOr(&P.changed[C.node], 1);
}

// FORB::meanValue for the clusters of one node, in cluster order, by one workgroup: thread t owns bit t (word t / 32, bit t % 32 of the descriptor read as
// eight little-endian words; the reference's "bit 7 - i % 8 of byte i / 8" is the same bit under another name, and every bit is decided on its own).
// cnt[c][256]: set bits of cluster c's group, gs[c]: its size.  Returns false when a group is empty.
__device__ __forceinline__ bool vt_finalize(const VtParams& P, int node, const uint32_t* cnt, const int* gs)
{
    const int t = threadIdx.x, nc = P.ncl[node], wi = t >> 5;
    for (int c = 0; c < nc; c++) {
        const int n = gs[c];
        if (n == 0) { if (t == 0) atomicMin(&P.stat[1], node); return false; }
        const uint32_t need = n >= 2 ? (uint32_t)(n / 2 + n % 2) : 1u;            // a group of one: the clone's bits are the counters themselves
        const uint32_t bit = cnt[c * 256 + t] >= need;
        const unsigned long long m = __ballot(bit);
        const uint32_t word = (t & 32) ? (uint32_t)(m >> 32) : (uint32_t)m;
        const size_t ci = (size_t)node * P.k + c;
        const int slot = n >= 2 ? P.cent[ci] : -1;
        if ((t & 31) == 0) {
            if (slot >= 0) P.desc[(size_t)slot * 8 + wi] = word;                   // Mat::zeros into the buffer the centre shares with feature `slot`
            else P.own[ci * 8 + wi] = word;
        }
        if (t == 0 && n < 2) P.cent[ci] = -1;                                      // descriptors[0]->clone(): the alias ends
    }
    return true;
}

// :694-717  the bit counts of every cluster of the chunk's node
__global__ __launch_bounds__(VT_T) void k_vt_count(VtParams P)
{
    __shared__ uint32_t s_cnt[VT_MAXK * 256];
    __shared__ uint32_t s_d[VT_CHUNK * 8];
    __shared__ uint8_t s_a[VT_CHUNK];
    __shared__ int s_gs[VT_MAXK];
    const VtChunk C = P.chunks[blockIdx.x];
    if (!P.active[C.node]) return;
    const VtNode N = P.nodes[C.node];
    const int nc = P.ncl[C.node], t = threadIdx.x;
    for (int c = 0; c < nc; c++) s_cnt[c * 256 + t] = 0;
    if (t < VT_MAXK) s_gs[t] = 0;
    __syncthreads();
    for (int i = t; i < C.n * 8; i += VT_T) s_d[i] = P.desc[(size_t)P.idx[C.start + (i >> 3)] * 8 + (i & 7)];
    for (int i = t; i < C.n; i += VT_T) { const uint8_t a = P.asg[C.start + i]; s_a[i] = a; atomicAdd(&s_gs[a], 1); }
    __syncthreads();
    const int wi = t >> 5, sh = t & 31;
    for (int m = 0; m < C.n; m++) s_cnt[s_a[m] * 256 + t] += (s_d[m * 8 + wi] >> sh) & 1u;
    __syncthreads();
    if (N.nchunks == 1) { vt_finalize(P, C.node, s_cnt, s_gs); return; }
    for (int c = 0; c < nc; c++) { const uint32_t v = s_cnt[c * 256 + t]; if (v) atomicAdd(&P.bigcnt[((size_t)N.big * P.k + c) * 256 + t], v); }
    if (t < nc && s_gs[t]) atomicAdd(&P.biggs[(size_t)N.big * P.k + t], s_gs[t]);
}

// the nodes of several chunks: means from the table k_vt_count added up, which is cleared for the next pass
__global__ __launch_bounds__(VT_T) void k_vt_mean_big(VtParams P)
{
    const int node = P.bignodes[blockIdx.x], t = threadIdx.x;
    if (!P.active[node]) return;
    const int big = P.nodes[node].big, nc = P.ncl[node];
    uint32_t* cnt = P.bigcnt + (size_t)big * P.k * 256; int* gs = P.biggs + (size_t)big * P.k;
    vt_finalize(P, node, cnt, gs);
    __syncthreads();
    for (int c = 0; c < nc; c++) cnt[c * 256 + t] = 0;
    if (t < nc) gs[t] = 0;
}

// :756-779  a node goes on while an assignment changed (the pass right after seeding always counts as changed)
__global__ __launch_bounds__(VT_T) void k_vt_pass_end(VtParams P)
{
    const int node = blockIdx.x * VT_T + threadIdx.x;
    if (node >= P.nnodes || !P.active[node]) return;
    if (P.changed[node]) { P.changed[node] = 0; atomicAdd(&P.stat[0], 1); } else P.active[node] = 0;
}

__global__ __launch_bounds__(VT_T) void k_vt_hist(VtParams P)
{
    __shared__ int s_gs[VT_MAXK];
    const VtChunk C = P.chunks[blockIdx.x];
    const int t = threadIdx.x;
    if (t < VT_MAXK) s_gs[t] = 0;
    __syncthreads();
    for (int i = t; i < C.n; i += VT_T) atomicAdd(&s_gs[P.asg[C.start + i]], 1);
    __syncthreads();
    if (t < P.k) P.chunk_cnt[(size_t)blockIdx.x * P.k + t] = s_gs[t];
}

// groups keep training order (:749, :804-811): one wavefront per chunk, lane c keeps cluster c's next free position
__global__ __launch_bounds__(64) void k_vt_scatter(VtParams P)
{
    const VtChunk C = P.chunks[blockIdx.x];
    const int lane = threadIdx.x, nc = P.ncl[C.node];
    int next = lane < P.k ? P.chunk_base[(size_t)blockIdx.x * P.k + lane] : 0;
    for (int tile = 0; tile < C.n; tile += 64) {
        const int i = tile + lane; const bool valid = i < C.n;
        const int a = valid ? (int)P.asg[C.start + i] : -1, fi = valid ? P.idx[C.start + i] : 0;
        for (int c = 0; c < nc; c++) {
            const unsigned long long m = __ballot(a == c);
            const int base = __shfl(next, c);
            if (a == c) P.idx_out[base + __popcll(m & ((1ull << lane) - 1ull))] = fi;
            if (lane == c) next += __popcll(m);
        }
    }
}

// :962-983  a feature counts for its word when no earlier feature of its image walks to the same word (img_off: nimages + 1 ascending)
__global__ __launch_bounds__(VT_T) void k_vt_docs(const uint32_t* word, const int* img_off, int nimages, int n, int* ni)
{
    const int i = blockIdx.x * VT_T + threadIdx.x;
    if (i >= n) return;
    int lo = 0, hi = nimages;                                                 // the last image that starts at or before i
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (img_off[mid] <= i) lo = mid; else hi = mid; }
    const uint32_t w = word[i];
    for (int j = img_off[lo]; j < i; j++) if (word[j] == w) return;
    atomicAdd(&ni[w], 1);
}

// ---------------------------------------------------------------------------------------------- host
namespace {
struct VtMem {                                                                 // the call's device memory and events
    std::vector<void*> ptrs; std::vector<hipEvent_t> events;
    template <typename T> hipError_t get(T** p, size_t count) { *p = nullptr; const hipError_t e = orbhip_dmalloc((void**)p, std::max<size_t>(count, 1) * sizeof(T)); if (e == hipSuccess) ptrs.push_back(*p); return e; }
    ~VtMem() { for (void* p : ptrs) (void)hipFree(p); for (hipEvent_t e : events) (void)hipEventDestroy(e); }
};
struct VtTree {                                                                // handles in creation order; a node's children are neighbours
    std::vector<int> parent, slot, own, c0, nc;                                // slot: the feature a descriptor aliases, or -1 and own = its place in own_desc
    std::vector<uint8_t> own_desc;
    int add(int p, int s, int o) { parent.push_back(p); slot.push_back(s); own.push_back(o); c0.push_back(0); nc.push_back(0); return (int)parent.size() - 1; }
};
struct VtWork { int handle, start, n; };
thread_local std::vector<double> vt_level_ms;
}

extern "C" int orbhip_voc_create_level_ms(double* ms, int cap)
{
    const int n = (int)vt_level_ms.size();
    for (int i = 0; i < n && i < cap; i++) ms[i] = vt_level_ms[i];
    return n ? n - 1 : 0;
}

extern "C" orbhip_status orbhip_voc_create(orbhip_voc** out, int device, const uint8_t* desc, const int32_t* image_counts, int nimages, int k, int L,
                                           int weighting, int scoring, uint32_t seed, uint8_t* desc_after, int32_t* word_docs)
{
    OrbApiTimer api_timer;
    if (!out) return fail(ORBHIP_ERR_INVALID, "null argument");
    *out = nullptr;
    if (nimages < 0 || (nimages > 0 && !image_counts)) return fail(ORBHIP_ERR_INVALID, "bad argument");
    if (weighting < 0 || weighting > 3 || scoring < 0 || scoring > 5) return fail(ORBHIP_ERR_INVALID, "weighting %d (0..3) or scoring %d (0..5) out of range", weighting, scoring);
    if (k < 2 || k > VT_MAXK) return fail(ORBHIP_ERR_UNSUPPORTED, "branching factor k = %d (2..%d)", k, VT_MAXK);
    if (L < 1 || L > 10) return fail(ORBHIP_ERR_UNSUPPORTED, "depth L = %d (1..10)", L);
    std::vector<int> img_off(nimages + 1, 0);
    long long total = 0;
    for (int i = 0; i < nimages; i++) {
        if (image_counts[i] < 0) return fail(ORBHIP_ERR_INVALID, "image %d has %d features", i, image_counts[i]);
        total += image_counts[i];
        if (total > INT_MAX / 32) return fail(ORBHIP_ERR_UNSUPPORTED, "more than %d training features", INT_MAX / 32);
        img_off[i + 1] = (int)total;
    }
    const int M = (int)total;
    if (M > 0 && !desc) return fail(ORBHIP_ERR_INVALID, "bad argument");
    if (!device_present()) return fail(ORBHIP_ERR_HIP, "no HIP device available: no CPU fallback");
    HIPCHK(hipSetDevice(device));
    const hipStream_t s = orbhip_thread_stream(device);
    vt_level_ms.assign(1, 0.0);

    VtTree T; T.add(0, -1, -1);                                               // the root: no descriptor
    T.own_desc.assign(32, 0); T.own[0] = 0;
    VtMem mem;
    VtParams P; memset(&P, 0, sizeof P);
    uint8_t* d_desc = nullptr;
    std::vector<int> hidx(M);
    for (int i = 0; i < M; i++) hidx[i] = i;
    std::vector<VtWork> work;
    if (M > 0) work.push_back(VtWork{0, 0, M});                               // :645
    const int NN = M / (k + 1) + 1, NC = M / VT_CHUNK + NN, NB = M / VT_CHUNK + 1;      // nodes of more than k features, their chunks, those of several chunks
    int *d_idx[2] = {nullptr, nullptr}, *d_bignodes = nullptr, *d_chunk_base = nullptr; VtNode* d_nodes = nullptr; VtChunk* d_chunks = nullptr;
    if (M > k) {
        HIPCHK(mem.get(&d_desc, (size_t)M * 32)); HIPCHK(mem.get(&d_idx[0], M)); HIPCHK(mem.get(&d_idx[1], M));
        HIPCHK(mem.get(&d_nodes, NN)); HIPCHK(mem.get(&d_chunks, NC)); HIPCHK(mem.get(&d_bignodes, NB)); HIPCHK(mem.get(&d_chunk_base, (size_t)NC * k));
        HIPCHK(mem.get(&P.ncl, NN)); HIPCHK(mem.get(&P.used, NN)); HIPCHK(mem.get(&P.cent, (size_t)NN * k)); HIPCHK(mem.get(&P.own, (size_t)NN * k * 8));
        HIPCHK(mem.get(&P.mind, M)); HIPCHK(mem.get(&P.asg, M)); HIPCHK(mem.get(&P.active, NN)); HIPCHK(mem.get(&P.changed, NN));
        HIPCHK(mem.get(&P.bigcnt, (size_t)NB * k * 256)); HIPCHK(mem.get(&P.biggs, (size_t)NB * k)); HIPCHK(mem.get(&P.chunk_cnt, (size_t)NC * k)); HIPCHK(mem.get(&P.stat, 2));
        HIPCHK(hipMemcpyAsync(d_desc, desc, (size_t)M * 32, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_idx[0], hidx.data(), (size_t)M * 4, hipMemcpyHostToDevice, s));
        P.desc = reinterpret_cast<uint32_t*>(d_desc); P.nodes = d_nodes; P.chunks = d_chunks; P.bignodes = d_bignodes; P.chunk_base = d_chunk_base; P.k = k;
    }
    int cur = 0;
    for (int level = 1; level <= L && !work.empty(); level++) {
        // ---- this level's nodes: those of at most k features make one child per feature (:660-670), the others run k-means
        std::vector<VtNode> nodes; std::vector<VtChunk> chunks; std::vector<int> bignodes, handles;
        for (const VtWork& w : work) {
            if (w.n <= k) {
                T.c0[w.handle] = (int)T.parent.size(); T.nc[w.handle] = w.n;
                for (int i = 0; i < w.n; i++) T.add(w.handle, hidx[w.start + i], -1);
                continue;
            }
            VtNode N; N.start = w.start; N.n = w.n; N.chunk0 = (int)chunks.size(); N.nchunks = (w.n + VT_CHUNK - 1) / VT_CHUNK; N.big = -1;
            N.seed = (seed ^ ((uint32_t)hidx[w.start] * 0x9E3779B1u) ^ ((uint32_t)w.n * 0x85EBCA6Bu)) & 0x7fffffffu;
            if (N.nchunks > 1) { N.big = (int)bignodes.size(); bignodes.push_back((int)nodes.size()); }
            for (int c = 0; c < N.nchunks; c++) chunks.push_back(VtChunk{(int)nodes.size(), w.start + c * VT_CHUNK, std::min(VT_CHUNK, w.n - c * VT_CHUNK)});
            nodes.push_back(N); handles.push_back(w.handle);
        }
        work.clear();
        const int nn = (int)nodes.size(), nch = (int)chunks.size(), nbig = (int)bignodes.size();
        if (nn == 0) break;
        if (nn > NN || nch > NC || nbig > NB) return fail(ORBHIP_ERR_HIP, "orbhip_voc_create: level %d outgrew its tables", level);
        hipEvent_t ea, eb; HIPCHK(hipEventCreate(&ea)); mem.events.push_back(ea); HIPCHK(hipEventCreate(&eb)); mem.events.push_back(eb);
        HIPCHK(hipEventRecord(ea, s));
        HIPCHK(hipMemcpyAsync(d_nodes, nodes.data(), (size_t)nn * sizeof(VtNode), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_chunks, chunks.data(), (size_t)nch * sizeof(VtChunk), hipMemcpyHostToDevice, s));
        if (nbig) {
            HIPCHK(hipMemcpyAsync(d_bignodes, bignodes.data(), (size_t)nbig * 4, hipMemcpyHostToDevice, s));
            HIPCHK(hipMemsetAsync(P.bigcnt, 0, (size_t)nbig * k * 256 * 4, s)); HIPCHK(hipMemsetAsync(P.biggs, 0, (size_t)nbig * k * 4, s));
        }
        P.idx = d_idx[cur]; P.idx_out = d_idx[cur ^ 1]; P.nnodes = nn; P.nchunks = nch;
        const dim3 gn((nn + VT_T - 1) / VT_T), gc(nch), gb(nbig), bt(VT_T);
        // ---- k-means++ (:833-913)
        hipLaunchKernelGGL(k_vt_seed_first, gn, bt, 0, s, P);
        for (int c = 1; c < k; c++) {
            P.round = c;
            hipLaunchKernelGGL(k_vt_seed_dist, gc, bt, 0, s, P);
            hipLaunchKernelGGL(k_vt_seed_pick, dim3(nn), bt, 0, s, P);
        }
        // ---- Lloyd passes (:681-781)
        P.first_pass = 1;
        hipLaunchKernelGGL(k_vt_assign, gc, bt, 0, s, P);
        P.first_pass = 0;
        int pass = 0, stat[2] = {0, INT_MAX};
        for (;; pass++) {
            if (pass == VT_MAX_PASSES) {
                (void)hipStreamSynchronize(s);
                return fail(ORBHIP_ERR_UNSUPPORTED, "orbhip_voc_create: k-means of level %d has not settled after %d passes (%d nodes still change)", level, VT_MAX_PASSES, stat[0]);
            }
            stat[0] = 0; stat[1] = INT_MAX;
            HIPCHK(hipMemcpyAsync(P.stat, stat, sizeof stat, hipMemcpyHostToDevice, s));
            if (pass > 0) {
                hipLaunchKernelGGL(k_vt_count, gc, bt, 0, s, P);
                if (nbig) hipLaunchKernelGGL(k_vt_mean_big, gb, bt, 0, s, P);
                hipLaunchKernelGGL(k_vt_assign, gc, bt, 0, s, P);
            }
            hipLaunchKernelGGL(k_vt_pass_end, gn, bt, 0, s, P);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(stat, P.stat, sizeof stat, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            if (stat[1] != INT_MAX) {
                const VtNode& N = nodes[stat[1]];
                return fail(ORBHIP_ERR_UNSUPPORTED, "orbhip_voc_create: a cluster of the node at level %d that starts at feature %d (%d features) lost all its features in pass %d; "
                            "the reference dereferences a null pointer here", level, hidx[N.start], N.n, pass);
            }
            if (stat[0] == 0) break;
        }
        // ---- the groups, in training order, become the next level's nodes
        std::vector<int> ncl(nn), cent((size_t)nn * k), ccnt((size_t)nch * k), cbase((size_t)nch * k);
        const size_t own0 = T.own_desc.size() / 32;
        T.own_desc.resize((own0 + (size_t)nn * k) * 32);
        hipLaunchKernelGGL(k_vt_hist, gc, bt, 0, s, P);
        HIPCHK(hipMemcpyAsync(ncl.data(), P.ncl, (size_t)nn * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(cent.data(), P.cent, (size_t)nn * k * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(ccnt.data(), P.chunk_cnt, (size_t)nch * k * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&T.own_desc[own0 * 32], P.own, (size_t)nn * k * 32, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        std::vector<VtWork> next;
        for (int nd = 0; nd < nn; nd++) {
            const VtNode& N = nodes[nd];
            const int h = handles[nd];
            T.c0[h] = (int)T.parent.size(); T.nc[h] = ncl[nd];
            int at = N.start;
            for (int c = 0; c < ncl[nd]; c++) {
                int gs = 0;
                for (int ch = 0; ch < N.nchunks; ch++) { cbase[(size_t)(N.chunk0 + ch) * k + c] = at + gs; gs += ccnt[(size_t)(N.chunk0 + ch) * k + c]; }
                const int sl = cent[(size_t)nd * k + c];
                const int child = T.add(h, sl, sl >= 0 ? -1 : (int)(own0 + (size_t)nd * k + c));
                if (gs > 1 && level < L) next.push_back(VtWork{child, at, gs});                  // :796-817
                at += gs;
            }
        }
        HIPCHK(hipMemcpyAsync(d_chunk_base, cbase.data(), (size_t)nch * k * 4, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_vt_scatter, gc, dim3(64), 0, s, P);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(eb, s));
        if (!next.empty()) HIPCHK(hipMemcpyAsync(hidx.data(), P.idx_out, (size_t)M * 4, hipMemcpyDeviceToHost, s));      // (positions outside this level's nodes are never read again)
        HIPCHK(hipStreamSynchronize(s));
        float ms = 0.f; HIPCHK(hipEventElapsedTime(&ms, ea, eb)); vt_level_ms.push_back(ms);
        cur ^= 1;
        work.swap(next);
    }

    // ---- the features as the reference leaves them; node ids in the reference's depth-first order (:786-817): a node's children take the next ids when it is visited
    std::vector<uint8_t> after;
    if (M > 0) {
        after.resize((size_t)M * 32);
        if (d_desc) { HIPCHK(hipMemcpyAsync(after.data(), d_desc, (size_t)M * 32, hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s)); }
        else memcpy(after.data(), desc, (size_t)M * 32);
    }
    const int nn = (int)T.parent.size();
    std::vector<int> id(nn, 0);
    {
        int next = 1;
        std::vector<std::pair<int, int>> st;
        for (int i = 0; i < T.nc[0]; i++) id[T.c0[0] + i] = next++;
        st.push_back(std::make_pair(0, 0));
        while (!st.empty()) {
            const int h = st.back().first, i = st.back().second;
            if (i == T.nc[h]) { st.pop_back(); continue; }
            st.back().second++;
            const int c = T.c0[h] + i;
            if (T.nc[c] > 0) { for (int j = 0; j < T.nc[c]; j++) id[T.c0[c] + j] = next++; st.push_back(std::make_pair(c, 0)); }
        }
    }
    std::vector<int> parent(nn, 0); std::vector<uint8_t> leaf(nn, 0), ndesc((size_t)nn * 32, 0); std::vector<double> weight(nn, 0.0);
    for (int h = 1; h < nn; h++) {
        const int i = id[h];
        parent[i] = id[T.parent[h]]; leaf[i] = T.nc[h] == 0;
        memcpy(&ndesc[(size_t)i * 32], T.slot[h] >= 0 ? &after[(size_t)T.slot[h] * 32] : &T.own_desc[(size_t)T.own[h] * 32], 32);
    }
    std::vector<int> word_node; word_node.reserve(nn);
    for (int i = 1; i < nn; i++) if (leaf[i]) word_node.push_back(i);
    const int nwords = (int)word_node.size();

    // ---- setNodeWeights (:943-996): Ni over the features as they are now; the walk is k_bow_descend's, through a vocabulary without weights
    std::vector<int> ni(std::max(nwords, 1), 0);
    if (nwords > 0 && M > 0) {
        orbhip_voc* tmp = nullptr;
        orbhip_status st = orbhip_voc_from_tree(&tmp, device, k, L, scoring, weighting, nn, parent.data(), leaf.data(), ndesc.data(), weight.data());
        if (st != ORBHIP_OK) return st;
        hipError_t e = hipSuccess; uint32_t *d_word = nullptr, *d_node = nullptr; double* d_weight = nullptr; int *d_off = nullptr, *d_ni = nullptr; hipEvent_t ea = nullptr, eb = nullptr;
        if (!d_desc) { e = mem.get(&d_desc, (size_t)M * 32); if (e == hipSuccess) e = hipMemcpyAsync(d_desc, desc, (size_t)M * 32, hipMemcpyHostToDevice, s); }
        if (e == hipSuccess) e = mem.get(&d_word, M); if (e == hipSuccess) e = mem.get(&d_node, M); if (e == hipSuccess) e = mem.get(&d_weight, M);
        if (e == hipSuccess) e = mem.get(&d_off, (size_t)nimages + 1); if (e == hipSuccess) e = mem.get(&d_ni, nwords);
        if (e == hipSuccess) e = hipEventCreate(&ea); if (e == hipSuccess) { mem.events.push_back(ea); e = hipEventCreate(&eb); } if (e == hipSuccess) mem.events.push_back(eb);
        if (e == hipSuccess) e = hipMemcpyAsync(d_off, img_off.data(), ((size_t)nimages + 1) * 4, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemsetAsync(d_ni, 0, (size_t)nwords * 4, s);
        if (e == hipSuccess) e = hipEventRecord(ea, s);
        if (e == hipSuccess) st = orbhip_voc_words_resident(tmp, d_desc, M, d_word, d_weight, d_node, s);
        if (e == hipSuccess && st == ORBHIP_OK) {
            hipLaunchKernelGGL(k_vt_docs, dim3((M + VT_T - 1) / VT_T), dim3(VT_T), 0, s, d_word, d_off, nimages, M, d_ni);
            e = hipGetLastError();
            if (e == hipSuccess) e = hipEventRecord(eb, s);
            if (e == hipSuccess) e = hipMemcpyAsync(ni.data(), d_ni, (size_t)nwords * 4, hipMemcpyDeviceToHost, s);
        }
        const hipError_t e2 = hipStreamSynchronize(s);
        float ms = 0.f; if (e == hipSuccess && e2 == hipSuccess && st == ORBHIP_OK && hipEventElapsedTime(&ms, ea, eb) == hipSuccess) vt_level_ms[0] = ms;
        orbhip_voc_destroy(tmp);
        if (st != ORBHIP_OK) return st;
        if (e != hipSuccess || e2 != hipSuccess) return fail(ORBHIP_ERR_HIP, "orbhip_voc_create: %s", hipGetErrorString(e != hipSuccess ? e : e2));
    }
    for (int w = 0; w < nwords; w++) {
        if (weighting == 1 || weighting == 3) weight[word_node[w]] = 1.0;                                             // TF, BINARY
        else if (ni[w] > 0) weight[word_node[w]] = std::log((double)(unsigned)nimages / (double)(unsigned)ni[w]);     // a word no walk reaches keeps 0 (:988-991)
    }
    const orbhip_status st = orbhip_voc_from_tree(out, device, k, L, scoring, weighting, nn, parent.data(), leaf.data(), ndesc.data(), weight.data());
    if (st != ORBHIP_OK) return st;
    if (desc_after && M > 0) memcpy(desc_after, after.data(), (size_t)M * 32);
    if (word_docs) for (int w = 0; w < nwords; w++) word_docs[w] = ni[w];
    return ORBHIP_OK;
}
