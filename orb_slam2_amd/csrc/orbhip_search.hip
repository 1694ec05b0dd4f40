// orbhip_search.hip — host side of the matcher searches of liborbhip.so.  The projection-guided and the best-in-window search have ONE routine each that takes a
// list of slots and does the whole call (search_by_projection_slots, search_best_in_window_slots): every entry point - one frame as host arrays or resident on a
// context, batch, shared - checks its own arguments, states them as slots and calls it; orbhip_project_best_in_window_held searches a slot the shared call left.
// Then the stateless matcher entry points and the relocalisation candidates.  Kernels: orbhip_kernels_proj.hip, orbhip_kernels_match.hip.
#include "orbhip_ctx.h"

// Frame::AssignFeaturesToGrid over ALL key points of nslots frames kp[slot][cap] (counts d_n[slot]) into the tables at [slot]: k_match_grid with grid_all_levels
void launch_feature_grid(const orbhip_keypoint* kp, const int* d_n, int cap, const orbhip_bounds& b, int* grid_start, int* grid_items, float2* grid_xy,
                         int nslots, int slot0, hipStream_t s)
{
    MatchParams M; memset(&M, 0, sizeof M);
    M.kp2 = kp; M.n2 = d_n; M.cap = cap; M.min_x = b.min_x; M.min_y = b.min_y; M.max_x = b.max_x; M.max_y = b.max_y;
    M.grid_start = grid_start; M.grid_items = grid_items; M.grid_xy = grid_xy; M.grid_all_levels = 1; M.slot0 = slot0;
    orbhip_launch_match_grid(M, nslots, s);
}

// ---------------------------------------------------------------------------------------------- projection-guided search
static bool projection_ok(const orbhip_projection* P)
{
    const int kind = P ? P->kind & ~ORBHIP_FP_CONTRACT : -1;          // the kind, optionally with the fused-arithmetic flag; any other bit is invalid
    return P && kind >= ORBHIP_PROJ_LAST_FRAME && kind <= ORBHIP_PROJ_SIM3 && P->gemm_mode >= 0 && P->gemm_mode <= 2 && P->nlevels >= 1 && P->nlevels <= ORBHIP_MAX_PROJ_LEVELS;
}
// ORBHIP_FP_CONTRACT in proj->kind selects the fused kernels; the device copy carries the bare kind (the kernels compare it)
static bool fp_contract_of(const orbhip_projection* P) { return P && (P->kind & ORBHIP_FP_CONTRACT); }
static orbhip_projection bare_projection(const orbhip_projection& P) { orbhip_projection Q = P; Q.kind &= ~ORBHIP_FP_CONTRACT; return Q; }
template <typename Query> static void gated_out(Query* q, int np) { if (q) for (int i = 0; i < np; i++) { memset(&q[i], 0, sizeof q[i]); q[i].radius = -1.0f; } }
static void no_match(int32_t* best_idx, int32_t* best_dist, int nq) { for (int i = 0; i < nq; i++) { best_idx[i] = -1; best_dist[i] = 256; } }
// a host input the kernels only read: laid out like Arena::io, its device copy handed back as a pointer to const
template <typename T> static void arena_in(Arena& A, const T** p, const T* src, size_t count) { T* d = nullptr; A.io(&d, count, src, count); *p = d; }

// The frame a single-frame search looks in: host arrays that travel in the call's arena (host_frame), or a frame of a context's last extraction
// that is still on the device (frame_args), of which only the queries travel.
struct SearchFrame {
    int device; hipStream_t stream;             // a context's stream; host arrays use the calling thread's, taken once the device is set
    int n; orbhip_bounds bounds; bool on_host;
    const orbhip_keypoint* kps; const uint8_t* desc; const float* u_right;      // host or device pointers (u_right may be nullptr)
    const int* grid_start = nullptr; const int* grid_items = nullptr; const float2* grid_xy = nullptr;      // the frame's grid, already on the device; nullptr: the search builds it
    bool* want_grid = nullptr;                  // set when the search runs: the context then builds the grid behind each single-image extraction
};
static orbhip_status host_frame(int device, const orbhip_keypoint* kps, const uint8_t* desc, const float* u_right, int n, const orbhip_bounds* bounds, SearchFrame* F)
{
    if (n < 0 || (n > 0 && (!kps || !desc)) || !bounds || !(bounds->max_x > bounds->min_x) || !(bounds->max_y > bounds->min_y)) return fail(ORBHIP_ERR_INVALID, "bad argument");
    *F = SearchFrame{device, nullptr, n, *bounds, true, kps, desc, u_right};
    return ORBHIP_OK;
}
// key points (mvKeysUn with a distorted camera attached), descriptors and - if asked for - mvuRight of the last stereo / RGB-D step are read where the extraction left them
static orbhip_status frame_args(orbhip_ctx* c, int frame, int n, int use_u_right, SearchFrame* F)
{
    if (!c) return fail(ORBHIP_ERR_INVALID, "null context");
    if (frame < 0 || frame >= c->last_nimg) return fail(ORBHIP_ERR_INVALID, "frame %d outside the %d frames of the last extraction", frame, c->last_nimg);
    if (n < 0 || n > c->out_cap) return fail(ORBHIP_ERR_INVALID, "n %d outside 0..%d", n, c->out_cap);
    if (use_u_right && !c->d_last_uright) return fail(ORBHIP_ERR_INVALID, "no mvuRight on the device: run orbhip_compute_stereo_matches / orbhip_compute_stereo_from_rgbd on this context first");
    *F = SearchFrame{c->cfg.device, c->stream, n, c->bounds, false, (c->distorted ? c->d_out_kpun : c->d_out_kp)[c->cur] + (size_t)frame * c->out_cap,
                     c->d_out_desc[c->cur] + (size_t)frame * c->out_cap * 32, use_u_right ? c->d_last_uright + (size_t)frame * c->out_cap : nullptr};
    // the grid of this frame was built behind its extraction (frame epilogue, same stream): take it; from now on it always will be
    if (frame == 0 && c->fgrid_valid && c->fgrid_cur == c->cur && c->last_n_valid && c->last_n[0] == n) { F->grid_start = c->d_fgrid_start; F->grid_items = c->d_fgrid_items; F->grid_xy = c->d_fgrid_xy; }
    if (c->last_nimg == 1 || c->pair_mode) F->want_grid = &c->want_fgrid;
    return ORBHIP_OK;
}

// One frame (slot) of a projection-guided search call: queries given, or (points != nullptr) derived on the device from nq map points under *proj
// (orbhip_project_search_*: k_proj_candidates also writes them to queries_out, if asked for)
struct ProjSlotIn {
    SearchFrame F; const uint8_t* blocked;                                              // blocked: optional
    const orbhip_proj_query* queries; const uint8_t* query_desc; int nq;
    const orbhip_projection* proj; const orbhip_map_point* points; orbhip_proj_query* queries_out;
    int32_t* feature_query; int* nmatches;
};
// where a slot's arrays lie on the device
struct ProjDev {
    const orbhip_keypoint* kp; const uint8_t* desc; const float* u_right; const int* grid_start; const int* grid_items; const float2* grid_xy;
    orbhip_proj_query* q; const uint8_t* qdesc; const orbhip_map_point* pts; const orbhip_projection* proj; const unsigned char* blocked;
    int* feature_query; int* nmatches; unsigned* cand; int* ncand; unsigned* top; int* events; int* big_ws;
};
// the slot's block of the table the kernels read (the only place that fills one)
static ProjParams proj_block(const ProjSlotIn& S, const ProjDev& D, int mode, float nnratio, int th_high, int check_ori)
{
    const orbhip_bounds& b = S.F.bounds;
    ProjParams J; memset(&J, 0, sizeof J);
    J.kp = D.kp; J.desc = D.desc; J.u_right = D.u_right; J.n = S.F.n; J.min_x = b.min_x; J.min_y = b.min_y; J.max_x = b.max_x; J.max_y = b.max_y;
    J.gw_inv = (float)ORBHIP_GRID_COLS / (float)(b.max_x - b.min_x); J.gh_inv = (float)ORBHIP_GRID_ROWS / (float)(b.max_y - b.min_y);      // as orbhip_launch_match_grid lays the grid out
    J.grid_start = D.grid_start; J.grid_items = D.grid_items; J.grid_xy = D.grid_xy;
    J.q = D.q; J.qdesc = D.qdesc; J.nq = S.nq; J.pts = D.pts; J.proj = D.proj; J.q_out = D.q;
    J.cand = D.cand; J.ncand = D.ncand; J.cand_stride = S.F.n; J.top = D.top;
    J.blocked_in = D.blocked; J.blocked_out = nullptr; J.feature_query = D.feature_query; J.nmatches = D.nmatches; J.events = D.events;
    J.mode = mode; J.nnratio = nnratio; J.th_high = th_high; J.check_ori = check_ori; J.big_ws = D.big_ws;
    return J;
}

// (ORBHIP_RECORD / TestRecord, the emulation-only capture of the calls below: orbhip_internal.h)

// The entry point behind a call of the two slot routines.  ONE_FRAME: one slot, which may be a resident frame - the call then runs on its context's stream, with
// the grid built behind its extraction if that is ready; BATCH: the _batch entry points, slots of host arrays; SHARED: orbhip_project_best_in_window_shared
enum SlotForm { ONE_FRAME, BATCH, SHARED };

// Every slot of a call in one pass, a one-frame call being one slot: ONE arena - the parameter table, each live slot's inputs at their own size, then every answer
// (what the download carries back: no input lies between two answers), then the kernels' work space - one copy each way, one launch of each kernel over the table
// (the order-dependent one runs a workgroup per slot).
static orbhip_status search_by_projection_slots(int nslots, ProjSlotIn* slots, int mode, float nnratio, int th_high, int check_ori, SlotForm form)
{
    OrbApiTimer api_timer;
    const bool batch = form == BATCH;
    if (mode != 0 && mode != 1) return fail(ORBHIP_ERR_INVALID, "bad argument");
    std::vector<int> live;
    int cap = 1, qcap = 1;
    for (int s = 0; s < nslots; s++) {
        const ProjSlotIn& S = slots[s]; const int n = S.F.n;
        if (n < 0 || S.nq < 0 || !S.nmatches || (n > 0 && (!S.F.kps || !S.F.desc || !S.feature_query)) || (S.nq > 0 && ((!S.queries && !S.points) || !S.query_desc)) || (S.points && !projection_ok(S.proj)))
            return batch ? fail(ORBHIP_ERR_INVALID, "bad argument in slot %d", s) : fail(ORBHIP_ERR_INVALID, "bad argument");
        *S.nmatches = 0;
        for (int i = 0; i < n; i++) S.feature_query[i] = -1;
        if (S.points) gated_out(S.queries_out, S.nq);
        cap = std::max(cap, n); qcap = std::max(qcap, S.nq);
        if (n > 0 && S.nq > 0) live.push_back(s);
    }
    if (live.empty()) return ORBHIP_OK;
    const SearchFrame& F0 = slots[live[0]].F;
    if (F0.on_host && cap >= (1 << 19)) return fail(ORBHIP_ERR_UNSUPPORTED, "too many features");
    if (batch && (size_t)nslots * qcap * cap * sizeof(unsigned) > ((size_t)2 << 30)) return fail(ORBHIP_ERR_UNSUPPORTED, "candidate lists of %d slots x %d queries x %d features exceed 2 GB: split the batch", nslots, qcap, cap);
    if (F0.on_host && !device_present()) return fail(ORBHIP_ERR_HIP, "no HIP device available: no CPU fallback");
    HIPCHK(hipSetDevice(F0.device));
    const hipStream_t ts = F0.on_host ? orbhip_thread_stream(F0.device) : F0.stream;
    const int NL = (int)live.size();
    const bool fc = fp_contract_of(slots[live[0]].proj);                               // (only a one-frame call brings points)
    int max_n = 1, max_nq = 1;                                                         // the launch is sized by the slots with work (cap / qcap above: the preconditions' view of all slots)
    for (int k = 0; k < NL; k++) { max_n = std::max(max_n, slots[live[k]].F.n); max_nq = std::max(max_nq, slots[live[k]].nq); }
    // the select kernel's per-feature tables in device memory: for every slot or for none.  orbhip_launch_proj asks the same question of the same max_n (and reads
    // ORBHIP_SELECT_BIG again): the two answers must agree, or a kernel finds no big_ws / sizes its LDS for none
    const bool big = orbhip_proj_select_big(max_n);
    std::vector<ProjParams> hJ(NL); std::vector<ProjDev> D(NL); std::vector<int> hn(NL), hnm(NL, 0);
    std::vector<orbhip_projection> hP(NL);                                             // the slots' projections as the device reads them (bare kind)
    std::vector<size_t> noff(NL + 1, 0), qoff(NL + 1, 0), coff(NL + 1, 0);             // the slots' places in the shared work arrays: features, queries, candidates before them
    for (int k = 0; k < NL; k++) {
        const ProjSlotIn& S = slots[live[k]];
        hn[k] = S.F.n; if (S.points) hP[k] = bare_projection(*S.proj);
        noff[k + 1] = noff[k] + (size_t)S.F.n; qoff[k + 1] = qoff[k] + (size_t)S.nq; coff[k + 1] = coff[k] + (size_t)S.nq * S.F.n;
    }
    ProjParams* dJ = nullptr; int *dn = nullptr, *dnm = nullptr, *dgs = nullptr, *dgi = nullptr, *dnc = nullptr, *dev = nullptr, *dbig = nullptr; float2* dgxy = nullptr; unsigned *dcand = nullptr, *dtop = nullptr;
    const hipError_t e = arena_call(F0.device, ts, [&](Arena& A) {
        A.io(&dJ, (size_t)NL, (const ProjParams*)hJ.data(), (size_t)NL);
        A.io(&dn, (size_t)NL, (const int*)hn.data(), (size_t)NL);
        for (int k = 0; k < NL; k++) {                                                  // every slot's inputs ...
            const ProjSlotIn& S = slots[live[k]]; ProjDev& d = D[k]; const size_t n = (size_t)S.F.n, nq = (size_t)S.nq;
            d.kp = S.F.kps; d.desc = S.F.desc; d.u_right = S.F.u_right;                 // (host arrays: replaced by their copies)
            if (S.F.on_host) { arena_in(A, &d.kp, S.F.kps, n); arena_in(A, &d.desc, S.F.desc, n * 32); if (S.F.u_right) arena_in(A, &d.u_right, S.F.u_right, n); }
            arena_in(A, &d.qdesc, S.query_desc, nq * 32);
            if (S.points) { arena_in(A, &d.pts, S.points, nq); arena_in(A, &d.proj, &hP[k], 1); }
            else A.io(&d.q, nq, S.queries, nq);
            if (S.blocked) arena_in(A, &d.blocked, S.blocked, n);
        }
        A.io(&dnm, (size_t)NL, (const int*)nullptr, 0, hnm.data(), (size_t)NL);        // ... then every answer: the match counts (k_proj_select writes every slot's), feature_query, the derived queries
        for (int k = 0; k < NL; k++) A.io(&D[k].feature_query, (size_t)hn[k], (const int*)nullptr, 0, slots[live[k]].feature_query, (size_t)hn[k]);
        for (int k = 0; k < NL; k++) { const ProjSlotIn& S = slots[live[k]]; if (S.points) A.io(&D[k].q, (size_t)S.nq, (const orbhip_proj_query*)nullptr, 0, S.queries_out, S.queries_out ? (size_t)S.nq : 0); }
        A.take(&dgs, (size_t)NL * (ORBHIP_GRID_CELLS + 1)); A.take(&dgi, noff[NL]); A.take(&dgxy, noff[NL]); A.take(&dnc, qoff[NL]); A.take(&dev, qoff[NL]);
        A.take(&dcand, coff[NL]); A.take(&dtop, qoff[NL] * 5);
        if (big) A.take(&dbig, 4 * noff[NL]);
        for (int k = 0; k < NL; k++) {                                                  // (hJ is read when the arena is uploaded, after this pass has filled in the addresses)
            const ProjSlotIn& S = slots[live[k]]; ProjDev& d = D[k];
            const bool own = !S.F.grid_start;                                           // the slot does not bring its grid: built below
            d.grid_start = own ? dgs + (size_t)k * (ORBHIP_GRID_CELLS + 1) : S.F.grid_start; d.grid_items = own ? dgi + noff[k] : S.F.grid_items; d.grid_xy = own ? dgxy + noff[k] : S.F.grid_xy;
            d.nmatches = dnm + k; d.ncand = dnc + qoff[k]; d.events = dev + qoff[k]; d.cand = dcand + coff[k]; d.top = dtop + qoff[k] * 5; d.big_ws = big ? dbig + 4 * noff[k] : nullptr;
            hJ[k] = proj_block(S, d, mode, nnratio, th_high, check_ori);
        }
    }, [&] {
        for (int k = 0; k < NL; k++) {                                                  // Frame::AssignFeaturesToGrid of every slot that needs it
            const SearchFrame& F = slots[live[k]].F;
            if (!F.grid_start) launch_feature_grid(D[k].kp, dn + k, F.n, F.bounds, dgs + (size_t)k * (ORBHIP_GRID_CELLS + 1), dgi + noff[k], dgxy + noff[k], 1, 0, ts);
            if (F.want_grid) *F.want_grid = true;
        }
        orbhip_launch_proj(dJ, NL, max_nq, max_n, ts, fc);
    });
    if (e != hipSuccess) {
        for (int k = 0; k < NL; k++) { const ProjSlotIn& S = slots[live[k]]; for (int i = 0; i < S.F.n; i++) S.feature_query[i] = -1; if (S.points) gated_out(S.queries_out, S.nq); }
        return fail(ORBHIP_ERR_HIP, "%s: %s", batch ? "search_by_projection_batch" : F0.on_host ? "search_by_projection" : "search_by_projection_frame", hipGetErrorString(e));
    }
    for (int k = 0; k < NL; k++) *slots[live[k]].nmatches = hnm[k];
    ORBHIP_RECORD(if (!batch) for (int k = 0; k < NL; k++) {
        const ProjSlotIn& S = slots[live[k]]; const SearchFrame& F = S.F;
        if (!S.points) continue;
        TestRecord R(1); const float par[2] = {nnratio, (float)0}; const int ipar[3] = {th_high, check_ori, hnm[k]};
        R.put(F.kps, F.n); R.put(F.desc, (size_t)F.n * 32); R.put(F.u_right, F.n); R.put(S.blocked, F.n); R.put(&F.bounds, 1); R.put(S.proj, 1); R.put(S.points, S.nq); R.put(S.query_desc, (size_t)S.nq * 32);
        R.put(par, 2); R.put(ipar, 3); R.put(S.feature_query, F.n);
    });
    return ORBHIP_OK;
}
// one frame: queries given (P == nullptr) or derived on the device from map points under *P (orbhip_project_search_*): `queries` is then nullptr and nq = the point count
static orbhip_status search_by_projection(const SearchFrame& F, const uint8_t* blocked, const orbhip_proj_query* queries, const uint8_t* query_desc, int nq,
                                          const orbhip_projection* P, const orbhip_map_point* points, orbhip_proj_query* queries_out,
                                          int mode, float nnratio, int th_high, int check_ori, int32_t* feature_query, int* nmatches)
{
    ProjSlotIn S{F, blocked, queries, query_desc, nq, P, points, queries_out, feature_query, nmatches};
    return search_by_projection_slots(1, &S, mode, nnratio, th_high, check_ori, ONE_FRAME);
}
extern "C" orbhip_status orbhip_search_by_projection_bounds(int device, const orbhip_keypoint* kps, const uint8_t* desc, const float* u_right,
                                                     const uint8_t* blocked, int n, const orbhip_bounds* bounds,
                                                     const orbhip_proj_query* queries, const uint8_t* query_desc, int nq,
                                                     int mode, float nnratio, int th_high, int check_ori, int32_t* feature_query, int* nmatches)
{
    SearchFrame F; const orbhip_status st = host_frame(device, kps, desc, u_right, n, bounds, &F); if (st != ORBHIP_OK) return st;
    return search_by_projection(F, blocked, queries, query_desc, nq, nullptr, nullptr, nullptr, mode, nnratio, th_high, check_ori, feature_query, nmatches);
}
extern "C" orbhip_status orbhip_project_search_bounds(int device, const orbhip_keypoint* kps, const uint8_t* desc, const float* u_right, const uint8_t* blocked, int n, const orbhip_bounds* bounds,
                                                      const orbhip_projection* proj, const orbhip_map_point* points, const uint8_t* point_desc, int np,
                                                      float nnratio, int th_high, int check_ori, int32_t* feature_query, int* nmatches, orbhip_proj_query* queries_out)
{
    SearchFrame F; const orbhip_status st = host_frame(device, kps, desc, u_right, n, bounds, &F); if (st != ORBHIP_OK) return st;
    return search_by_projection(F, blocked, nullptr, point_desc, np, np > 0 ? proj : nullptr, np > 0 ? points : nullptr, queries_out, 1, nnratio, th_high, check_ori, feature_query, nmatches);
}
extern "C" orbhip_status orbhip_search_by_projection_frame(orbhip_ctx* c, int frame, int n, int use_u_right, const uint8_t* blocked,
                                                           const orbhip_proj_query* queries, const uint8_t* query_desc, int nq,
                                                           int mode, float nnratio, int th_high, int check_ori, int32_t* feature_query, int* nmatches)
{
    if (nq > 0 && !queries) return fail(ORBHIP_ERR_INVALID, "bad argument");
    SearchFrame F; const orbhip_status st = frame_args(c, frame, n, use_u_right, &F); if (st != ORBHIP_OK) return st;
    return search_by_projection(F, blocked, queries, query_desc, nq, nullptr, nullptr, nullptr, mode, nnratio, th_high, check_ori, feature_query, nmatches);
}
extern "C" orbhip_status orbhip_project_search_frame(orbhip_ctx* c, int frame, int n, int use_u_right, const uint8_t* blocked,
                                                     const orbhip_projection* proj, const orbhip_map_point* points, const uint8_t* point_desc, int np,
                                                     float nnratio, int th_high, int check_ori, int32_t* feature_query, int* nmatches, orbhip_proj_query* queries_out)
{
    if (np > 0 && (!points || !proj)) return fail(ORBHIP_ERR_INVALID, "bad argument");
    SearchFrame F; const orbhip_status st = frame_args(c, frame, n, use_u_right, &F); if (st != ORBHIP_OK) return st;
    return search_by_projection(F, blocked, nullptr, point_desc, np, np > 0 ? proj : nullptr, np > 0 ? points : nullptr, queries_out, 1, nnratio, th_high, check_ori, feature_query, nmatches);
}

// Several frames in one pass: the slots of the C ABI as slots of the routine above (one bounds for all)
extern "C" orbhip_status orbhip_search_by_projection_batch(int device, int nslots, orbhip_proj_slot* slots, const orbhip_bounds* bounds,
                                                           int mode, float nnratio, int th_high, int check_ori)
{
    if (nslots < 0 || (nslots > 0 && !slots) || !bounds || !(bounds->max_x > bounds->min_x) || !(bounds->max_y > bounds->min_y) || (mode != 0 && mode != 1))
        return fail(ORBHIP_ERR_INVALID, "bad argument");
    std::vector<ProjSlotIn> in((size_t)nslots);
    for (int s = 0; s < nslots; s++) {
        orbhip_proj_slot& S = slots[s];
        in[s] = ProjSlotIn{SearchFrame{device, nullptr, S.n, *bounds, true, S.kps, S.desc, S.u_right}, S.blocked, S.queries, S.query_desc, S.nq, nullptr, nullptr, nullptr, S.feature_query, &S.nmatches};
    }
    return search_by_projection_slots(nslots, in.data(), mode, nnratio, th_high, check_ori, BATCH);
}
// One key frame (slot) of a best-in-window search call; inv_level_sigma2 / nlevels: mvInvLevelSigma2 of the frame's extractor (a context's frame: its own).
// Queries given, or (points != nullptr) derived on the device from nq map points under *proj (orbhip_project_best_in_window_*), written to queries_out if asked for.
struct BestSlotIn {
    SearchFrame F; const float* inv_level_sigma2; int nlevels;
    const orbhip_best_query* queries; const uint8_t* query_desc; int nq; const orbhip_projection* proj; const orbhip_map_point* points; orbhip_best_query* queries_out;
    int32_t* best_idx; int32_t* best_dist;
};
// where a slot's arrays lie on the device
struct BestDev {
    const orbhip_keypoint* kp; const uint8_t* desc; const float* u_right; const float* inv_level_sigma2; const int* grid_start; const int* grid_items; const float2* grid_xy;      // the key frame: what a held slot keeps
    const orbhip_best_query* q; const uint8_t* qdesc; const orbhip_map_point* pts; const orbhip_projection* proj; const unsigned long long* skip; orbhip_best_query* q_out; int* best_idx; int* best_dist;
};
// the slot's block of the table the kernels read (the only place that fills one)
static BestParams best_block(const BestDev& D, const orbhip_bounds& b, int nq, int chi2_gate, int skip_bit)
{
    BestParams B; memset(&B, 0, sizeof B);
    B.kp = D.kp; B.desc = D.desc; B.u_right = D.u_right; B.inv_level_sigma2 = D.inv_level_sigma2; B.grid_start = D.grid_start; B.grid_items = D.grid_items; B.grid_xy = D.grid_xy;
    B.q = D.q; B.qdesc = D.qdesc; B.nq = nq; B.chi2_gate = chi2_gate; B.pts = D.pts; B.proj = D.proj; B.q_out = D.q_out; B.best_idx = D.best_idx; B.best_dist = D.best_dist;
    B.min_x = b.min_x; B.gw_inv = (float)ORBHIP_GRID_COLS / (float)(b.max_x - b.min_x);      // as orbhip_launch_match_grid lays the grid out
    B.skip = D.skip; B.skip_bit = skip_bit;
    return B;
}
// the slots orbhip_project_best_in_window_shared left in the calling thread's scratch (valid while orbhip_tl_held_valid, orbhip_api.hip)
static thread_local struct HeldSlots { int device = -1; size_t floor = 0; std::vector<BestDev> D; std::vector<orbhip_bounds> bounds; std::vector<int> live_of_slot; } g_held;

// Every key frame of a call in one pass (Fuse over all targets), a one-frame call being one slot: [slot][cap] key point / grid blocks in one arena; the feature grids
// of all slots are built by ONE k_match_grid launch when the slots share their image bounds (key frames of one camera do), the searches by one launch over all queries.
// SHARED: every slot's queries are slots[0]'s (points / query_desc / nq: uploaded once); skip: see orbhip_project_best_in_window_shared
static orbhip_status search_best_in_window_slots(int device, int nslots, BestSlotIn* slots, int chi2_gate, SlotForm form, const uint64_t* skip)
{
    OrbApiTimer api_timer;
    const bool shared = form == SHARED;
    if (shared) {
        orbhip_tl_held_valid = false;                                                   // whatever an earlier call left held is not THIS call's (also when nothing is live below)
        if (nslots > 64) return fail(ORBHIP_ERR_INVALID, "at most 64 slots share one set of points");
        for (int s = 1; s < nslots; s++)
            if (slots[s].nq != slots[0].nq || (slots[0].nq > 0 && (slots[s].points != slots[0].points || slots[s].query_desc != slots[0].query_desc || !slots[s].points)))        // (no points: nothing to name)
                return fail(ORBHIP_ERR_INVALID, "slot %d does not name slot 0's points", s);
    }
    std::vector<int> live;
    int cap = 1, fc = -1;                                    // fc: the slots' ORBHIP_FP_CONTRACT (one launch: every slot with points must agree)
    for (int s = 0; s < nslots; s++) {
        BestSlotIn& S = slots[s]; const orbhip_bounds& b = S.F.bounds;
        if (S.F.n < 0 || S.nq < 0 || (S.nq > 0 && ((!S.queries && !S.points) || !S.query_desc || !S.best_idx || !S.best_dist)) || (S.F.n > 0 && (!S.F.kps || !S.F.desc)) ||
            !(b.max_x > b.min_x) || !(b.max_y > b.min_y) || (chi2_gate && (!S.inv_level_sigma2 || S.nlevels < 1)) || (S.nq > 0 && S.points && !projection_ok(S.proj)))
            return form == ONE_FRAME ? fail(ORBHIP_ERR_INVALID, "bad argument") : fail(ORBHIP_ERR_INVALID, "bad argument in slot %d", s);
        if (S.nq > 0 && S.points) {
            if (fc >= 0 && fc != (int)fp_contract_of(S.proj)) return fail(ORBHIP_ERR_INVALID, "slot %d: the slots of one call mix ORBHIP_FP_CONTRACT and its absence", s);
            fc = fp_contract_of(S.proj);
        }
        no_match(S.best_idx, S.best_dist, S.nq);
        if (S.points) gated_out(S.queries_out, S.nq);
        if (S.F.n == 0 || S.nq == 0) continue;
        live.push_back(s); cap = std::max(cap, S.F.n);
    }
    if (live.empty()) {
        if (shared) {                                                                   // held: a slot without key points answers -1 / 256; one whose key frame never travelled (no points were offered) cannot answer (-2)
            g_held.device = device; g_held.floor = 0; g_held.D.clear(); g_held.bounds.clear(); g_held.live_of_slot.assign((size_t)nslots, -1);
            for (int s = 0; s < nslots; s++) if (slots[s].F.n > 0) g_held.live_of_slot[(size_t)s] = -2;
            orbhip_tl_held_valid = true;
        }
        return ORBHIP_OK;
    }
    const SearchFrame& F0 = slots[live[0]].F;
    if (F0.on_host && !device_present()) return fail(ORBHIP_ERR_HIP, "no HIP device available: no CPU fallback");
    HIPCHK(hipSetDevice(device));
    const hipStream_t ts = F0.on_host ? orbhip_thread_stream(device) : F0.stream;
    cap = (cap + 63) & ~63;                                  // 64 key points = 7 x 256 bytes: the arena's 256-byte blocks then lie exactly cap records apart ([slot][cap])
    const int NL = (int)live.size(); const size_t C = (size_t)cap;
    const bool ready = F0.grid_start != nullptr;             // (one slot: a resident frame whose grid was built behind its extraction)
    bool same_bounds = true;
    for (int k = 1; k < NL; k++) same_bounds = same_bounds && !memcmp(&slots[live[k]].F.bounds, &F0.bounds, sizeof(orbhip_bounds));
    std::vector<BestParams> hB(NL); std::vector<BestDev> D(NL); std::vector<int> pref(NL + 1, 0), hn(NL);
    std::vector<orbhip_projection> hP(NL);                   // the slots' projections as the device reads them (bare kind)
    for (int k = 0; k < NL; k++) if (slots[live[k]].points) hP[k] = bare_projection(*slots[live[k]].proj);
    for (int k = 0; k < NL; k++) { pref[k + 1] = pref[k] + (slots[live[k]].nq + 3) / 4; hn[k] = slots[live[k]].F.n; }
    BestParams* dB = nullptr; int *dpref = nullptr, *dn = nullptr, *dgs = nullptr, *dgi = nullptr; float2* dgxy = nullptr;
    size_t held_floor = 0;
    const hipError_t e = arena_call(device, ts, [&](Arena& A) {
        A.io(&dB, (size_t)NL, (const BestParams*)hB.data(), (size_t)NL);
        A.io(&dpref, (size_t)NL + 1, (const int*)pref.data(), (size_t)NL + 1);
        A.io(&dn, (size_t)NL, (const int*)hn.data(), (size_t)NL);
        for (int k = 0; k < NL; k++) {                                                  // [slot][cap] key points first: k_match_grid indexes them by slot
            const SearchFrame& F = slots[live[k]].F;
            D[k].kp = F.kps;                                                            // (host arrays: replaced by their copies, here and below)
            if (F.on_host) { orbhip_keypoint* dk = nullptr; A.io(&dk, C, F.kps, (size_t)F.n); D[k].kp = dk; }
        }
        for (int k = 0; k < NL; k++) {                                                  // every slot's inputs ...
            const BestSlotIn& S = slots[live[k]]; const SearchFrame& F = S.F; BestDev& d = D[k]; const size_t n = (size_t)F.n, nq = (size_t)S.nq;
            d.desc = F.desc; d.u_right = F.u_right;
            if (F.on_host) { arena_in(A, &d.desc, F.desc, n * 32); if (F.u_right) arena_in(A, &d.u_right, F.u_right, n); }
            if (shared) {
                if (k == 0) {
                    arena_in(A, &d.qdesc, S.query_desc, nq * 32); arena_in(A, &d.pts, S.points, nq);
                    if (skip) arena_in(A, &d.skip, reinterpret_cast<const unsigned long long*>(skip), nq);
                }
                d.qdesc = D[0].qdesc; d.pts = D[0].pts; d.skip = D[0].skip; arena_in(A, &d.proj, &hP[k], 1);
            } else {
                arena_in(A, &d.qdesc, S.query_desc, nq * 32);
                if (S.points) { arena_in(A, &d.pts, S.points, nq); arena_in(A, &d.proj, &hP[k], 1); }
                else arena_in(A, &d.q, S.queries, nq);
            }
            if (S.inv_level_sigma2 && S.nlevels > 0) arena_in(A, &d.inv_level_sigma2, S.inv_level_sigma2, (size_t)S.nlevels);
        }
        for (int k = 0; k < NL; k++) {                                                  // ... then every slot's answers, contiguous: the download is one small copy
            const BestSlotIn& S = slots[live[k]];
            A.io(&D[k].best_idx, (size_t)S.nq, (const int*)nullptr, 0, S.best_idx, (size_t)S.nq); A.io(&D[k].best_dist, (size_t)S.nq, (const int*)nullptr, 0, S.best_dist, (size_t)S.nq);
            if (S.points && S.queries_out) A.io(&D[k].q_out, (size_t)S.nq, (const orbhip_best_query*)nullptr, 0, S.queries_out, (size_t)S.nq);
        }
        if (!ready) { A.take(&dgs, (size_t)NL * (ORBHIP_GRID_CELLS + 1)); A.take(&dgi, NL * C); A.take(&dgxy, NL * C); }
        for (int k = 0; k < NL; k++) {                                                  // (hB is read when the arena is uploaded, after this pass has filled in the addresses)
            const BestSlotIn& S = slots[live[k]]; BestDev& d = D[k];
            d.grid_start = ready ? S.F.grid_start : dgs + (size_t)k * (ORBHIP_GRID_CELLS + 1); d.grid_items = ready ? S.F.grid_items : dgi + k * C; d.grid_xy = ready ? S.F.grid_xy : dgxy + k * C;
            hB[k] = best_block(d, S.F.bounds, S.nq, chi2_gate, live[k]);
        }
        if (shared) {                                                                   // room for the held entry's block and queries behind everything: it never reallocates
            held_floor = A.off; uint8_t* pad = nullptr; A.take(&pad, (size_t)slots[live[0]].nq * (sizeof(orbhip_map_point) + 32 + 8) + 4096 + 512);
        }
    }, [&] {
        if (!ready) for (int k = 0; k < (same_bounds ? 1 : NL); k++) launch_feature_grid(D[0].kp, dn, cap, slots[live[k]].F.bounds, dgs, dgi, dgxy, same_bounds ? NL : 1, k, ts);
        for (int k = 0; k < NL; k++) if (slots[live[k]].F.want_grid) *slots[live[k]].F.want_grid = true;
        orbhip_launch_best_in_window(dB, dpref, NL, pref[NL], ts, fc == 1);
    });
    if (e != hipSuccess) {
        for (int k = 0; k < NL; k++) { const BestSlotIn& S = slots[live[k]]; no_match(S.best_idx, S.best_dist, S.nq); if (S.points) gated_out(S.queries_out, S.nq); }
        return fail(ORBHIP_ERR_HIP, "%s: %s", form != ONE_FRAME ? "search_best_in_window_batch" : F0.on_host ? "search_best_in_window" : "search_best_in_window_frame", hipGetErrorString(e));
    }
    ORBHIP_RECORD(if (form == BATCH) for (int k = 0; k < NL; k++) {
        const BestSlotIn& S = slots[live[k]]; const SearchFrame& F = S.F;
        if (!S.points) continue;
        TestRecord R(2); const int ipar[1] = {chi2_gate};
        R.put(F.kps, F.n); R.put(F.desc, (size_t)F.n * 32); R.put(F.u_right, F.n); R.put(&F.bounds, 1); R.put(S.inv_level_sigma2, S.nlevels); R.put(S.proj, 1);
        R.put(S.points, S.nq); R.put(S.query_desc, (size_t)S.nq * 32); R.put(ipar, 1); R.put(S.best_idx, S.nq); R.put(S.best_dist, S.nq);
    });
    if (shared) {                                                                       // the slots stay where they are for orbhip_project_best_in_window_held
        g_held.device = device; g_held.floor = held_floor; g_held.D = D; g_held.bounds.resize((size_t)NL); g_held.live_of_slot.assign((size_t)nslots, -1);
        for (int k = 0; k < NL; k++) { g_held.bounds[(size_t)k] = slots[live[k]].F.bounds; g_held.live_of_slot[(size_t)live[k]] = k; }
        orbhip_tl_held_valid = true;
    }
    return ORBHIP_OK;
}
// one frame: queries given (P == nullptr) or derived on the device from map points under *P
static orbhip_status search_best_in_window(const SearchFrame& F, const float* inv_level_sigma2, int nlevels, const orbhip_best_query* queries, const uint8_t* query_desc, int nq,
                                           const orbhip_projection* P, const orbhip_map_point* points, orbhip_best_query* queries_out,
                                           int chi2_gate, int32_t* best_idx, int32_t* best_dist)
{
    BestSlotIn S{F, inv_level_sigma2, nlevels, queries, query_desc, nq, P, points, queries_out, best_idx, best_dist};
    return search_best_in_window_slots(F.device, 1, &S, chi2_gate, ONE_FRAME, nullptr);
}
extern "C" orbhip_status orbhip_search_best_in_window_bounds(int device, const orbhip_keypoint* kps, const uint8_t* desc, const float* u_right, int n, const orbhip_bounds* bounds,
                                                      const float* inv_level_sigma2, int nlevels, const orbhip_best_query* queries, const uint8_t* query_desc, int nq,
                                                      int chi2_gate, int32_t* best_idx, int32_t* best_dist)
{
    SearchFrame F; const orbhip_status st = host_frame(device, kps, desc, u_right, n, bounds, &F); if (st != ORBHIP_OK) return st;
    return search_best_in_window(F, inv_level_sigma2, nlevels, queries, query_desc, nq, nullptr, nullptr, nullptr, chi2_gate, best_idx, best_dist);
}
extern "C" orbhip_status orbhip_project_best_in_window_bounds(int device, const orbhip_keypoint* kps, const uint8_t* desc, const float* u_right, int n, const orbhip_bounds* bounds,
                                                              const float* inv_level_sigma2, int nlevels, const orbhip_projection* proj, const orbhip_map_point* points, const uint8_t* point_desc, int np,
                                                              int chi2_gate, int32_t* best_idx, int32_t* best_dist, orbhip_best_query* queries_out)
{
    SearchFrame F; const orbhip_status st = host_frame(device, kps, desc, u_right, n, bounds, &F); if (st != ORBHIP_OK) return st;
    return search_best_in_window(F, inv_level_sigma2, nlevels, nullptr, point_desc, np, np > 0 ? proj : nullptr, np > 0 ? points : nullptr, queries_out, chi2_gate, best_idx, best_dist);
}
extern "C" orbhip_status orbhip_search_best_in_window_frame(orbhip_ctx* c, int frame, int n, int use_u_right, const orbhip_best_query* queries, const uint8_t* query_desc, int nq,
                                                            int chi2_gate, int32_t* best_idx, int32_t* best_dist)
{
    SearchFrame F; const orbhip_status st = frame_args(c, frame, n, use_u_right, &F); if (st != ORBHIP_OK) return st;
    return search_best_in_window(F, c->is2.data(), c->L, queries, query_desc, nq, nullptr, nullptr, nullptr, chi2_gate, best_idx, best_dist);
}

// One slot of the calling thread's last orbhip_project_best_in_window_shared call searched again with other points: its key frame, descriptors and
// grid table are still in the thread's scratch - only the points travel, with a table of one block, above what is held (ORBmatcher.cc's FuseBatch: the points
// whose descriptor an earlier target's MapPoint::Replace changed, MapPoint.cc:177-215)
extern "C" orbhip_status orbhip_project_best_in_window_held(int device, int slot, const orbhip_projection* proj, const orbhip_map_point* points, const uint8_t* point_desc, int np,
                                                            int chi2_gate, int32_t* best_idx, int32_t* best_dist)
{
    OrbApiTimer api_timer;
    if (np < 0 || (np > 0 && (!points || !point_desc || !best_idx || !best_dist || !projection_ok(proj)))) return fail(ORBHIP_ERR_INVALID, "bad argument");
    if (!orbhip_tl_held_valid || g_held.device != device || slot < 0 || slot >= (int)g_held.live_of_slot.size())
        return fail(ORBHIP_ERR_INVALID, "no held slot %d: the calling thread's last scratch-using call was not orbhip_project_best_in_window_shared on this device", slot);
    no_match(best_idx, best_dist, np);
    const int k = g_held.live_of_slot[(size_t)slot];
    if (k == -2) return fail(ORBHIP_ERR_INVALID, "held slot %d: its key frame did not travel (the shared call offered no points)", slot);
    if (k < 0 || np == 0) return ORBHIP_OK;                                             // (a slot without key points or a call without points: nothing to search)
    HIPCHK(hipSetDevice(device));
    hipStream_t ts = orbhip_thread_stream(device);
    BestDev d = g_held.D[(size_t)k]; d.q = nullptr; d.q_out = nullptr; d.skip = nullptr;      // the held key frame, this call's points
    BestParams hB; BestParams* dB = nullptr; int* dpref = nullptr;
    const int pref[2] = {0, (np + 3) / 4};
    const orbhip_projection hP = bare_projection(*proj);
    const hipError_t e = arena_call(device, ts, [&](Arena& A) {
        A.io(&dB, 1, (const BestParams*)&hB, 1); A.io(&dpref, 2, pref, 2);
        arena_in(A, &d.qdesc, point_desc, (size_t)np * 32); arena_in(A, &d.pts, points, (size_t)np); arena_in(A, &d.proj, &hP, 1);
        A.io(&d.best_idx, (size_t)np, (const int*)nullptr, 0, best_idx, (size_t)np); A.io(&d.best_dist, (size_t)np, (const int*)nullptr, 0, best_dist, (size_t)np);
        hB = best_block(d, g_held.bounds[(size_t)k], np, chi2_gate, 0);
    }, [&] { orbhip_launch_best_in_window(dB, dpref, 1, pref[1], ts, fp_contract_of(proj)); }, g_held.floor);
    if (e == hipErrorOutOfMemory) return fail(ORBHIP_ERR_INVALID, "the held scratch has no room for %d points", np);      // (the caller falls back to the full entry)
    if (e != hipSuccess) { no_match(best_idx, best_dist, np); return fail(ORBHIP_ERR_HIP, "project_best_in_window_held: %s", hipGetErrorString(e)); }
    return ORBHIP_OK;
}
extern "C" orbhip_status orbhip_search_best_in_window_batch(int device, int nslots, orbhip_best_slot* slots, int chi2_gate)
{
    if (nslots < 0 || (nslots > 0 && !slots)) return fail(ORBHIP_ERR_INVALID, "bad argument");
    std::vector<BestSlotIn> in((size_t)nslots);
    for (int s = 0; s < nslots; s++) {
        const orbhip_best_slot& S = slots[s];
        if (S.nq > 0 && !S.queries) return fail(ORBHIP_ERR_INVALID, "bad argument in slot %d", s);
        in[s] = BestSlotIn{SearchFrame{device, nullptr, S.n, S.bounds, true, S.kps, S.desc, S.u_right}, S.inv_level_sigma2, S.nlevels, S.queries, S.query_desc, S.nq, nullptr, nullptr, nullptr, S.best_idx, S.best_dist};
    }
    return search_best_in_window_slots(device, nslots, in.data(), chi2_gate, BATCH, nullptr);
}
// orbhip_project_best_in_window_batch / _shared: the slots' points projected on the device
static orbhip_status project_best_in_window_slots(int device, int nslots, const orbhip_project_best_slot* slots, int chi2_gate, SlotForm form, const uint64_t* skip)
{
    if (nslots < 0 || (nslots > 0 && !slots)) return fail(ORBHIP_ERR_INVALID, "bad argument");
    std::vector<BestSlotIn> in((size_t)nslots);
    for (int s = 0; s < nslots; s++) {
        const orbhip_project_best_slot& S = slots[s];
        if (S.np > 0 && (!S.points || !S.proj)) return fail(ORBHIP_ERR_INVALID, "bad argument in slot %d", s);
        in[s] = BestSlotIn{SearchFrame{device, nullptr, S.n, S.bounds, true, S.kps, S.desc, S.u_right}, S.inv_level_sigma2, S.nlevels, nullptr, S.point_desc, S.np, S.np > 0 ? S.proj : nullptr, S.np > 0 ? S.points : nullptr, nullptr, S.best_idx, S.best_dist};
    }
    return search_best_in_window_slots(device, nslots, in.data(), chi2_gate, form, skip);
}
extern "C" orbhip_status orbhip_project_best_in_window_batch(int device, int nslots, orbhip_project_best_slot* slots, int chi2_gate)
{
    return project_best_in_window_slots(device, nslots, slots, chi2_gate, BATCH, nullptr);
}
extern "C" orbhip_status orbhip_project_best_in_window_shared(int device, int nslots, orbhip_project_best_slot* slots, const uint64_t* skip, int chi2_gate)
{
    return project_best_in_window_slots(device, nslots, slots, chi2_gate, SHARED, skip);
}

// ---------------------------------------------------------------------------------------------- stateless matcher entry points
extern "C" int orbhip_descriptor_distance(const uint8_t* a, const uint8_t* b)
{
    unsigned long long x[4], y[4]; memcpy(x, a, 32); memcpy(y, b, 32);
    return __builtin_popcountll(x[0] ^ y[0]) + __builtin_popcountll(x[1] ^ y[1]) + __builtin_popcountll(x[2] ^ y[2]) + __builtin_popcountll(x[3] ^ y[3]);
}

extern "C" orbhip_status orbhip_hamming_nn_device(void* stream, const uint8_t* d_q, int nq, const uint8_t* d_db, int64_t ndb, int64_t base,
                                                  int64_t* d_best_idx, int32_t* d_best_dist, int32_t* d_second)
{
    if (nq < 0 || ndb < 0 || (nq > 0 && (!d_q || !d_best_idx || !d_best_dist || !d_second)) || (ndb > 0 && !d_db)) return fail(ORBHIP_ERR_INVALID, "bad argument");
    if (!orbhip_launch_hamming_nn(d_q, nq, d_db, ndb, base, (long long*)d_best_idx, d_best_dist, d_second, (hipStream_t)stream)) return fail(ORBHIP_ERR_HIP, "hamming_nn: no device memory for the scan partials");
    HIPCHK(hipGetLastError());
    return ORBHIP_OK;
}

// A database that is queried many times (a key frame database: BASELINE.json config 5) expanded ONCE into the form the FP4 scan multiplies - 128 bytes per row
// instead of 32 - so that a query stages tiles by LDS-DMA instead of expanding every row again for every 512 queries (include/orbhip.h)
extern "C" size_t orbhip_nn_expanded_size(int64_t ndb) { return ndb < 0 ? 0 : orbhip_nn_expanded_bytes(ndb); }
extern "C" orbhip_status orbhip_nn_expand_device(void* stream, const uint8_t* d_db, int64_t ndb, uint8_t* d_expanded)
{
    if (ndb < 0 || (ndb > 0 && (!d_db || !d_expanded))) return fail(ORBHIP_ERR_INVALID, "bad argument");
    if (((uintptr_t)d_expanded & 15) != 0) return fail(ORBHIP_ERR_INVALID, "the expanded database must be 16-byte aligned");
    orbhip_launch_nn_expand(d_db, ndb, d_expanded, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return ORBHIP_OK;
}
extern "C" orbhip_status orbhip_hamming_nn_device_expanded(void* stream, const uint8_t* d_q, int nq, const uint8_t* d_db, const uint8_t* d_expanded, int64_t ndb, int64_t base,
                                                           int64_t* d_best_idx, int32_t* d_best_dist, int32_t* d_second)
{
    if (nq < 0 || ndb < 0 || (nq > 0 && (!d_q || !d_best_idx || !d_best_dist || !d_second)) || (ndb > 0 && (!d_db || !d_expanded))) return fail(ORBHIP_ERR_INVALID, "bad argument");
    if (!orbhip_launch_hamming_nn(d_q, nq, d_db, ndb, base, (long long*)d_best_idx, d_best_dist, d_second, (hipStream_t)stream, d_expanded)) return fail(ORBHIP_ERR_HIP, "hamming_nn: no device memory for the scan partials");
    HIPCHK(hipGetLastError());
    return ORBHIP_OK;
}

extern "C" orbhip_status orbhip_hamming_nn(int device, const uint8_t* q, int nq, const uint8_t* db, int64_t ndb, int64_t base,
                                           int64_t* best_idx, int32_t* best_dist, int32_t* second_dist)
{
    if (nq < 0 || ndb < 0 || (nq > 0 && (!q || !best_idx || !best_dist || !second_dist)) || (ndb > 0 && !db)) return fail(ORBHIP_ERR_INVALID, "bad argument");
    if (nq == 0) return ORBHIP_OK;
    if (!device_present()) return fail(ORBHIP_ERR_HIP, "no HIP device available: no CPU fallback");
    HIPCHK(hipSetDevice(device));
    uint8_t *dq = nullptr, *ddb = nullptr; long long* dbi = nullptr; int *dbd = nullptr, *dsd = nullptr;
    orbhip_status st = ORBHIP_OK;
    hipError_t e = hipSuccess;
    if (e == hipSuccess) e = orbhip_dmalloc((void**)&dq, (size_t)nq * 32);
    if (e == hipSuccess) e = orbhip_dmalloc((void**)&ddb, std::max<size_t>((size_t)ndb * 32, 32));
    if (e == hipSuccess) e = orbhip_dmalloc((void**)&dbi, (size_t)nq * 8);
    if (e == hipSuccess) e = orbhip_dmalloc((void**)&dbd, (size_t)nq * 4);
    if (e == hipSuccess) e = orbhip_dmalloc((void**)&dsd, (size_t)nq * 4);
    if (e == hipSuccess) e = hipMemcpy(dq, q, (size_t)nq * 32, hipMemcpyHostToDevice);
    if (e == hipSuccess && ndb > 0) e = hipMemcpy(ddb, db, (size_t)ndb * 32, hipMemcpyHostToDevice);
    if (e == hipSuccess) { e = orbhip_launch_hamming_nn(dq, nq, ddb, ndb, base, dbi, dbd, dsd, nullptr) ? hipGetLastError() : hipErrorOutOfMemory; }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(best_idx, dbi, (size_t)nq * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(best_dist, dbd, (size_t)nq * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(second_dist, dsd, (size_t)nq * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) st = fail(ORBHIP_ERR_HIP, "hamming_nn: %s", hipGetErrorString(e));
    (void)hipFree(dq); (void)hipFree(ddb); (void)hipFree(dbi); (void)hipFree(dbd); (void)hipFree(dsd);
    return st;
}

extern "C" orbhip_status orbhip_search_for_initialization_bounds(int device, const orbhip_keypoint* kps1, const uint8_t* desc1, int n1,
                                                          const orbhip_keypoint* kps2, const uint8_t* desc2, int n2, const orbhip_bounds* bounds,
                                                          float* prev_matched, int32_t* matches12, int window, float nnratio, int check_ori, int* nmatches)
{
    OrbApiTimer api_timer;
    if (n1 < 0 || n2 < 0 || !nmatches || (n1 > 0 && (!kps1 || !desc1 || !prev_matched || !matches12)) || (n2 > 0 && (!kps2 || !desc2)) || !bounds || !(bounds->max_x > bounds->min_x) || !(bounds->max_y > bounds->min_y))
        return fail(ORBHIP_ERR_INVALID, "bad argument");
    *nmatches = 0;
    for (int i = 0; i < n1; i++) matches12[i] = -1;
    if (n1 == 0) return ORBHIP_OK;
    if (!device_present()) return fail(ORBHIP_ERR_HIP, "no HIP device available: no CPU fallback");
    HIPCHK(hipSetDevice(device));
    hipStream_t ts = orbhip_thread_stream(device);
    // Frame members flattened: level-0 keypoints of F1 in index order (the loop at ORBmatcher.cc:418-423 skips the rest)
    std::vector<int> list1; for (int i = 0; i < n1; i++) if (kps1[i].octave <= 0) list1.push_back(i);
    int n2l0 = 0; for (int i = 0; i < n2; i++) n2l0 += kps2[i].octave == 0;
    const int cap = std::max(std::max(n1, n2), 1), l0cap = std::max((int)list1.size(), 1), cstride = std::max(n2l0, 1);
    orbhip_keypoint *dk1 = nullptr, *dk2 = nullptr; uint8_t *dd1 = nullptr, *dd2 = nullptr; int *dn = nullptr, *dlist = nullptr, *dgs = nullptr, *dgi = nullptr, *dnc = nullptr, *dm12 = nullptr, *dbig = nullptr; float2* dgxy = nullptr;
    unsigned* dcand = nullptr; unsigned* dtop = nullptr; float* dprev = nullptr;
    const int hn[4] = {n1, n2, (int)list1.size(), 0}; int hres[4] = {0, 0, 0, 0};
    const hipError_t e = arena_call(device, ts, [&](Arena& A) {
        A.io(&dk1, cap, kps1, n1); A.io(&dk2, cap, kps2, n2); A.io(&dd1, (size_t)cap * 32, desc1, (size_t)n1 * 32); A.io(&dd2, (size_t)cap * 32, desc2, (size_t)n2 * 32);
        A.io(&dlist, l0cap, (const int*)list1.data(), list1.size());
        A.io(&dn, 8, hn, 4, hres, 4);                          // counts in, [3] = nmatches out
        A.io(&dprev, (size_t)cap * 2, (const float*)prev_matched, (size_t)n1 * 2, prev_matched, (size_t)n1 * 2);
        A.io(&dm12, cap, (const int*)nullptr, 0, matches12, n1);
        A.take(&dgs, ORBHIP_GRID_CELLS + 1); A.take(&dgi, cap); A.take(&dgxy, cap); A.take(&dnc, l0cap);
        A.take(&dcand, (size_t)l0cap * cstride); A.take(&dtop, (size_t)l0cap * 5);
        if (orbhip_match_select_big(cstride, l0cap)) A.take(&dbig, orbhip_match_select_ints(cstride, l0cap));      // the select kernel's tables when they do not fit LDS
    }, [&] {
        MatchParams M; memset(&M, 0, sizeof M);
        M.kp1 = dk1; M.desc1 = dd1; M.n1 = dn; M.n1_lvl0 = dn + 2; M.kp2 = dk2; M.desc2 = dd2; M.n2 = dn + 1; M.lvl_stride = 0; M.list1 = dlist; M.prev_from_kp1 = 0;
        M.cap = cap; M.min_x = bounds->min_x; M.min_y = bounds->min_y; M.max_x = bounds->max_x; M.max_y = bounds->max_y; M.grid_start = dgs; M.grid_items = dgi; M.grid_xy = dgxy; M.cand = dcand; M.top = dtop; M.ncand = dnc; M.cand_stride = cstride; M.lvl0_cap = l0cap; M.tab_cap = cstride;      // the table lists F2's octave-0 key points inside the grid: at most n2l0
        M.prev = dprev; M.matches12 = dm12; M.nmatches = dn + 3; M.window = window; M.nnratio = nnratio; M.check_ori = check_ori; M.big_ws = dbig;
        orbhip_launch_match_grid(M, 1, ts); orbhip_launch_match_candidates(M, 1, ts); orbhip_launch_match_select(M, 1, ts);
    });
    if (e != hipSuccess) return fail(ORBHIP_ERR_HIP, "search_for_initialization: %s", hipGetErrorString(e));
    *nmatches = hres[3];
    return ORBHIP_OK;
}

// the im_w / im_h forms: an undistorted camera, mnMinX = mnMinY = 0, mnMaxX = cols, mnMaxY = rows (Frame.cc:455-463)
static bool whole_image(int im_w, int im_h, orbhip_bounds* b) { if (im_w < 1 || im_h < 1) return false; b->min_x = 0.0f; b->min_y = 0.0f; b->max_x = (float)im_w; b->max_y = (float)im_h; return true; }
extern "C" orbhip_status orbhip_search_by_projection(int device, const orbhip_keypoint* kps, const uint8_t* desc, const float* u_right, const uint8_t* blocked, int n,
                                                     int im_w, int im_h, const orbhip_proj_query* queries, const uint8_t* query_desc, int nq,
                                                     int mode, float nnratio, int th_high, int check_ori, int32_t* feature_query, int* nmatches)
{
    orbhip_bounds b; if (!whole_image(im_w, im_h, &b)) return fail(ORBHIP_ERR_INVALID, "bad argument");
    return orbhip_search_by_projection_bounds(device, kps, desc, u_right, blocked, n, &b, queries, query_desc, nq, mode, nnratio, th_high, check_ori, feature_query, nmatches);
}
extern "C" orbhip_status orbhip_search_best_in_window(int device, const orbhip_keypoint* kps, const uint8_t* desc, const float* u_right, int n, int im_w, int im_h,
                                                      const float* inv_level_sigma2, int nlevels, const orbhip_best_query* queries, const uint8_t* query_desc, int nq,
                                                      int chi2_gate, int32_t* best_idx, int32_t* best_dist)
{
    orbhip_bounds b; if (!whole_image(im_w, im_h, &b)) return fail(ORBHIP_ERR_INVALID, "bad argument");
    return orbhip_search_best_in_window_bounds(device, kps, desc, u_right, n, &b, inv_level_sigma2, nlevels, queries, query_desc, nq, chi2_gate, best_idx, best_dist);
}
extern "C" orbhip_status orbhip_search_for_initialization(int device, const orbhip_keypoint* kps1, const uint8_t* desc1, int n1,
                                                          const orbhip_keypoint* kps2, const uint8_t* desc2, int n2, int im_w, int im_h,
                                                          float* prev_matched, int32_t* matches12, int window, float nnratio, int check_ori, int* nmatches)
{
    orbhip_bounds b; if (!whole_image(im_w, im_h, &b)) return fail(ORBHIP_ERR_INVALID, "bad argument");
    return orbhip_search_for_initialization_bounds(device, kps1, desc1, n1, kps2, desc2, n2, &b, prev_matched, matches12, window, nnratio, check_ori, nmatches);
}

// ---------------------------------------------------------------------------------------------- relocalisation candidates
// Stands where Tracking::Relocalization asks KeyFrameDatabase::DetectRelocalizationCandidates for key frames that share words with the
// frame (Tracking.cc:1344-1348, KeyFrameDatabase.cc:199-309): here the evidence is the brute-force nearest neighbour of every query
// descriptor over the descriptors of ALL key frames (BASELINE.json config 5), filtered with the matcher's own acceptance idiom
// (distance threshold + ratio to the second best, ORBmatcher.cc:102-114), one vote per accepted descriptor for the owning key frame.
// MapPoint::PredictScale as a table (include/orbhip.h): level_ratio[i] = the smallest positive float ratio the caller's own expression maps to a level > i.
// Host arithmetic only (the caller's libm through level_of); the device compares ratios against the table (pj_predict_scale).
extern "C" orbhip_status orbhip_predict_scale_table(int (*level_of)(float ratio, void* user), void* user, int nlevels, float* level_ratio)
{
    if (!level_of || !level_ratio || nlevels < 1 || nlevels > ORBHIP_MAX_PROJ_LEVELS) return fail(ORBHIP_ERR_INVALID, "bad argument");
    auto as_float = [](uint32_t b) { float f; memcpy(&f, &b, 4); return f; };
    const float inf = as_float(0x7f800000u);
    for (int i = 0; i < ORBHIP_MAX_PROJ_LEVELS; i++) level_ratio[i] = inf;
    for (int i = 0; i + 1 < nlevels; i++) {
        auto above = [&](uint32_t b) { return level_of(as_float(b), user) > i; };
        uint32_t lo = 1u, hi = 0x7f7fffffu;                                  // smallest denormal .. largest finite float: positive floats order like their bits
        if (!above(hi)) continue;                                            // no finite ratio reaches level i + 1
        if (above(lo)) { level_ratio[i] = as_float(lo); continue; }
        while (hi - lo > 1u) { const uint32_t mid = lo + (hi - lo) / 2u; if (above(mid)) hi = mid; else lo = mid; }
        for (uint32_t d = 1; d <= 64u; d++) {                                 // a step function: nothing above the threshold falls back, nothing below reaches over
            if (hi + d <= 0x7f7fffffu && !above(hi + d)) return fail(ORBHIP_ERR_UNSUPPORTED, "PredictScale is not monotone in the distance ratio near %.9g (level %d)", (double)as_float(hi), i + 1);
            if (lo >= d && lo - d >= 1u && above(lo - d)) return fail(ORBHIP_ERR_UNSUPPORTED, "PredictScale is not monotone in the distance ratio near %.9g (level %d)", (double)as_float(hi), i + 1);
        }
        level_ratio[i] = as_float(hi);
    }
    return ORBHIP_OK;
}

extern "C" orbhip_status orbhip_reloc_candidates(const int64_t* best_idx, const int32_t* best_dist, const int32_t* second_dist, int nq,
                                                 const int32_t* row_keyframe, int64_t ndb, int nkf, int th_dist, float ratio,
                                                 int top_k, int32_t* kf_out, int32_t* votes_out, int* nout)
{
    if (nq < 0 || ndb < 0 || nkf < 0 || top_k < 0 || !nout || (nq > 0 && (!best_idx || !best_dist || !second_dist)) || (ndb > 0 && !row_keyframe) || (top_k > 0 && (!kf_out || !votes_out)))
        return fail(ORBHIP_ERR_INVALID, "bad argument");
    *nout = 0;
    std::vector<int> votes((size_t)std::max(nkf, 1), 0);
    for (int i = 0; i < nq; i++) {
        const int64_t r = best_idx[i];
        if (r < 0 || r >= ndb) continue;
        if (best_dist[i] > th_dist) continue;
        if (!((float)best_dist[i] < ratio * (float)second_dist[i])) continue;
        const int kf = row_keyframe[r];
        if (kf < 0 || kf >= nkf) return fail(ORBHIP_ERR_INVALID, "row %lld belongs to key frame %d outside 0..%d", (long long)r, kf, nkf - 1);
        votes[kf]++;
    }
    std::vector<int> order; order.reserve(nkf);
    for (int k = 0; k < nkf; k++) if (votes[k] > 0) order.push_back(k);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return votes[a] > votes[b]; });      // ties keep ascending key frame id
    const int m = std::min<int>(top_k, (int)order.size());
    for (int i = 0; i < m; i++) { kf_out[i] = order[i]; votes_out[i] = votes[order[i]]; }
    *nout = m;
    return ORBHIP_OK;
}
