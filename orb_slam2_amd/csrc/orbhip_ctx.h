// orbhip_ctx.h — the extractor context and what the host translation units share (orbhip_api.hip, orbhip_host_path.hip, orbhip_search.hip,
// orbhip_frame.hip, the host half of orbhip_distinct.hip).  Host code only: no kernel reads it.
#pragma once
#include "orbhip_internal.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include <algorithm>

// the one error setter is orbhip_set_error (orbhip_api.hip, declared in orbhip_internal.h); the host files spell it fail(...).
// (a macro: include this header after the standard ones)
#define fail orbhip_set_error
#define HIPCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail(ORBHIP_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)

static inline int cvRoundF(float v) { return (int)lrintf(v); }         // round-half-even, like cvRound
static inline int cvRoundD(double v) { return (int)lrint(v); }
static inline int cvFloorF(float v) { int i = (int)v; return i - (i > v); }
static inline short satShort(int v) { return (short)(v < -32768 ? -32768 : v > 32767 ? 32767 : v); }

enum { K_PYRAMID = 0, K_FAST, K_BLUR, K_QUADTREE, K_DESCRIBE, K_MGRID, K_MCAND, K_MSELECT, K_UNDISTORT, K_REMAP, K_COUNT };

struct ProfSpan { int k; hipEvent_t a, b; int counts; };

// One batch of the pipelined host-buffer path (orbhip_submit / orbhip_collect, orbhip_extract_batch): its own pinned input mirror,
// device input planes and pinned output mirrors, so that up to ORBHIP_RING batches are in flight; a batch is cut into chunks of
// camera slots and chunk k+1 uploads while chunk k computes and chunk k-1 downloads.
#define ORBHIP_RING 3
#define ORBHIP_MAX_CHUNKS 16
struct HostSet {
    uint8_t* d_packed = nullptr; size_t packed_bytes = 0;     // pinned caller images land here as they are (rows `stride` apart) and are re-pitched on the device
    uint8_t* d_in = nullptr; uint8_t* h_in = nullptr; orbhip_keypoint* h_kp = nullptr; uint8_t* h_desc = nullptr; int* h_n = nullptr; bool owned = false;
    uint8_t* h_block = nullptr;                               // h_n | h_kp | h_desc are parts of this one pinned allocation (same layout as the device block)
    bool busy = false; int ticket = -1, nimg = 0, out_buf = -1, nchunks = 0, chunk_f0[ORBHIP_MAX_CHUNKS + 1] = {0};
    hipEvent_t ev_h2d[ORBHIP_MAX_CHUNKS] = {nullptr}, ev_k[ORBHIP_MAX_CHUNKS] = {nullptr}, ev_d2h[ORBHIP_MAX_CHUNKS] = {nullptr};
    // outputs that went straight into the caller's pinned buffers by DMA (nothing left to copy at collect time)
    orbhip_keypoint* direct_kp = nullptr; uint8_t* direct_desc = nullptr; int direct_cap = 0;
};

struct orbhip_ctx {
    orbhip_config cfg; int L = 0, B = 0, fp_contract = 0;
    std::vector<LevelGeom> geom; std::vector<float> sf, isf, s2, is2; std::vector<int> nfeat;
    std::vector<CellDesc> cells; std::vector<TileDesc> blur_tiles; std::vector<BlurRun> blur_runs; std::vector<int2> xtab, ytab; std::vector<PyrGroup> xgrp; std::vector<char> pyr_staged;
    int gk[4] = {0, 0, 0, 0};
    hipStream_t stream = nullptr; bool own_stream = false;
    std::vector<hipStream_t> xstreams; std::vector<hipEvent_t> xevents; hipEvent_t ev_fork = nullptr;     // extra streams of a multi-stream context
    int fc_maxpw = 0, fc_maxph = 0;
    long long plane_frame_bytes = 0, blur_frame_bytes = 0, cand_slots_per_frame = 0, qt_per_frame = 0; int lvl_kp_per_frame = 0, out_cap = 0, qt_maxn = 0, qt_maxcells = 0, lvl0_cap = 0;
    // device
    LevelGeom* d_geom = nullptr; CellDesc* d_cells = nullptr; TileDesc* d_tiles = nullptr; BlurRun* d_runs = nullptr; int2* d_xtab = nullptr; int2* d_ytab = nullptr; float* d_pattern = nullptr; int4* d_fc_dma = nullptr; int fc_np = 0; PyrGroup* d_xgrp = nullptr; unsigned* d_ic_mask = nullptr; int4* d_blur_band = nullptr; bool blur_mfma = true; bool blur_strip_ok = true;
    uint8_t* d_pyr = nullptr; uint8_t* d_blur = nullptr; int* d_cell_count = nullptr; unsigned* d_cell_cand = nullptr;
    unsigned* d_qt_val = nullptr; unsigned* d_qt_code = nullptr; int* d_qt_node = nullptr; unsigned* d_lvl_kp = nullptr;
    // outputs are triple-buffered: batch t writes buffer t%3 while the matcher of batch t-1 (own stream) still reads buffers (t-1)%3 and (t-2)%3
    int* d_lvl_n[3] = {nullptr, nullptr, nullptr}; orbhip_keypoint* d_out_kp[3] = {nullptr, nullptr, nullptr}; uint8_t* d_out_desc[3] = {nullptr, nullptr, nullptr}; int* d_out_n[3] = {nullptr, nullptr, nullptr};
    // the three output arrays of a buffer are carved from ONE allocation ([counts | key points | descriptors], 256-byte aligned parts): the whole
    // result of a small batch is one device-to-host copy instead of three (a single-frame call spent 60 us between its second and third copy)
    uint8_t* d_out_block[3] = {nullptr, nullptr, nullptr}; size_t out_off_kp = 0, out_off_desc = 0, out_block_bytes = 0; uint8_t* h_block = nullptr;
    hipStream_t bstream = nullptr, bstream_host = nullptr; hipEvent_t ev_pyr = nullptr, ev_blur = nullptr;      // blur runs beside FAST + quadtree (independent until describe)
    // k_pyramid_cascade (every level in one launch, used for a handful of frames): per level the column ranges of each tile column and the row ranges of
    // each tile row, LDS layout sizes; pc_ok = the context's shape fits
    short2* d_pc_xr = nullptr; short2* d_pc_yr = nullptr; int pc_ntx = 0, pc_nty = 0, pc_buf0 = 0, pc_buf1 = 0, pc_xcap = 0, pc_ycap = 0; bool pc_ok = false;
    hipStream_t mstream = nullptr; hipEvent_t ev_extract = nullptr; hipEvent_t ev_match[3] = {nullptr, nullptr, nullptr}; bool match_pending[3] = {false, false, false};
    int cur = 0; int last_nimg = 0; bool last_matched = false; bool last_from_host = false;
    // Frame epilogues.  ORB_SLAM2 calls one image at a time and follows every extraction with the same steps (Frame.cc:61-117, Tracking.cc:867-928,
    // 1143-1193): the right image's row table for ComputeStereoMatches, the 64x48 feature grid for the projection searches.  Both depend on
    // nothing but the extraction's own results, so once a context has seen such a follow-up it enqueues them BEHIND the result download of every
    // single-image call: they run while the host is still copying key points out, and the follow-up call finds them done instead of launching
    // them on its critical path (18 us each of a stereo frame's ~0.9 ms).  Learned per context (a monocular extractor never pays for a row table).
    bool want_fgrid = false, want_rrows = false, fgrid_valid = false, rrows_valid = false; int fgrid_cur = -1, rrows_cur = -1;
    int* d_fgrid_start = nullptr; int* d_fgrid_items = nullptr; float2* d_fgrid_xy = nullptr; int* d_rrow_start = nullptr; int* d_rrow_items = nullptr; int rrow_cap = 0;
    hipEvent_t ev_epilogue = nullptr;
    bool pair_mode = false; float* h_st = nullptr; hipEvent_t ev_stereo = nullptr;           // the last call was orbhip_extract_stereo: slot 0 = the frame (left image), slot 1 = its right image; pinned mirror of [mvuRight | mvDepth]
    std::vector<int> last_n; bool last_n_valid = false;      // key point counts of the last call as already delivered to the host (the call's results were waited for)
    // host-buffer API staging: one contiguous device input buffer + pinned host mirrors (single bulk copies instead of per-frame pageable copies)
    bool serial = false;      // ORBHIP_SERIAL=1 (profiling aid): every kernel on the main stream, nothing overlaps - per-kernel times are standalone times
    uint8_t* d_in = nullptr; uint8_t* h_in = nullptr; uint8_t* d_col = nullptr; uint8_t* h_col = nullptr; size_t col_bytes = 0; orbhip_keypoint* h_kp = nullptr; uint8_t* h_desc = nullptr; int* h_n = nullptr; int in_pitch = 0;
    // stereo (Frame::ComputeStereoMatches): level-0 source of the last call + lazily allocated workspace on the LEFT context
    const uint8_t* last_img0 = nullptr; long long last_img0_fstride = 0; int last_img0_pitch = 0;
    int* d_st_rowstart = nullptr; int* d_st_rowitems = nullptr; int st_rowcap = 0; float* d_st_u = nullptr; float* d_st_depth = nullptr; int* d_st_sad = nullptr;
    // matcher workspace
    int* d_grid_start = nullptr; int* d_grid_items = nullptr; float2* d_grid_xy = nullptr; unsigned* d_cand = nullptr; unsigned* d_top = nullptr; int* d_ncand = nullptr; float* d_prev = nullptr; int* d_m12 = nullptr; int* d_nm = nullptr;
    // camera geometry: undistorted key points of a distorted camera, rectification maps of a raw stereo camera
    orbhip_bounds bounds = {0, 0, 0, 0}; bool distorted = false; CameraD cam = {}; orbhip_keypoint* d_out_kpun[3] = {nullptr, nullptr, nullptr}; orbhip_keypoint* h_kpun = nullptr;
    int* d_map_x = nullptr; int* d_map_y = nullptr; int src_w = 0, src_h = 0, raw_pitch = 0; uint8_t* d_raw = nullptr; uint8_t* h_raw = nullptr; uint8_t* d_depth = nullptr; size_t depth_bytes = 0; const float* d_last_uright = nullptr; float* d_ucols = nullptr; int* d_match_ws = nullptr; float* h_ucols = nullptr; hipEvent_t ev_ucols = nullptr; bool ucols_pending = false;   // mvuRight [slot][out_cap] of the last stereo / RGB-D step
    // pipelined host-buffer path
    HostSet sets[ORBHIP_RING]; hipStream_t hstream = nullptr, dstream = nullptr; int next_ticket = 0, oldest_ticket = 0, ticket_set[ORBHIP_RING] = {0, 0, 0}; const uint8_t* last_d_in = nullptr; bool plane0_dirty = false;   // plane0_dirty: set 0's level-0 plane was last written by an un-ticketed entry (colour / rectify)
    // profiling
    bool prof = false; std::vector<ProfSpan> pending; std::vector<hipEvent_t> pool; double tot_ms[K_COUNT] = {0}; long long launches[K_COUNT] = {0};
};

// ---------------------------------------------------------------------------------------------- profiling spans
static hipEvent_t prof_event(orbhip_ctx* c)
{
    if (!c->pool.empty()) { hipEvent_t e = c->pool.back(); c->pool.pop_back(); return e; }
    hipEvent_t e = nullptr; (void)hipEventCreate(&e); return e;
}
struct ProfScope {       // counts = 0: a further part of a kernel that is launched in pieces (its time adds up, the launch count does not)
    orbhip_ctx* c; int k; hipStream_t s; int counts; hipEvent_t a = nullptr, b = nullptr;
    ProfScope(orbhip_ctx* c_, int k_, hipStream_t s_, int counts_ = 1) : c(c_), k(k_), s(s_), counts(counts_) { if (c->prof) { a = prof_event(c); b = prof_event(c); (void)hipEventRecord(a, s); } }
    ~ProfScope() { if (c->prof) { (void)hipEventRecord(b, s); c->pending.push_back(ProfSpan{k, a, b, counts}); } }
};

// ---------------------------------------------------------------------------------------------- small helpers
template <typename T> static hipError_t dalloc(T** p, size_t count) { return orbhip_dmalloc((void**)p, std::max<size_t>(count, 1) * sizeof(T)); }
static bool device_present() { int n = 0; return hipGetDeviceCount(&n) == hipSuccess && n >= 1; }

// One matcher call on the calling thread's arena: lay it out (above floor, see arena_layout), upload its inputs, launch, download its answers.
// After a failure the stream is synchronised: never leave a copy in flight on the per-thread mirrors.
template <typename Layout, typename Launch> static hipError_t arena_call(int device, hipStream_t s, Layout layout, Launch launch, size_t floor = 0)
{
    hipError_t e = arena_layout(device, layout, floor);
    if (e == hipSuccess) e = arena_upload(s);
    if (e == hipSuccess) { launch(); e = hipGetLastError(); }
    if (e == hipSuccess) e = arena_download(s);
    if (e != hipSuccess) (void)hipStreamSynchronize(s);
    return e;
}

// ---------------------------------------------------------------------------------------------- functions that one host file defines and another calls
// (hidden: they are not part of the library's dynamic symbol table)
#pragma GCC visibility push(hidden)
// orbhip_api.hip
void prof_collect(orbhip_ctx* c);
ExtractParams make_params(orbhip_ctx* c, const uint8_t* d_img0, long long frame_stride, int row_stride);
orbhip_status pipeline_frames(orbhip_ctx* c, ExtractParams& P, int f0, int nf, hipStream_t s, bool own_blur_stream, bool host_path = false);
orbhip_status begin_batch(orbhip_ctx* c, const uint8_t* d_img0, long long frame_stride, int row_stride);
orbhip_status run_pipeline(orbhip_ctx* c, int nimg, const uint8_t* d_img0, long long frame_stride, int row_stride,
                           int match_prev, int window, float nnratio, int check_ori);
orbhip_status ensure_host_staging(orbhip_ctx* c, bool input);
orbhip_status mirrors_free(const orbhip_ctx* c, const char* who);
// orbhip_host_path.hip
orbhip_status frame_epilogues(orbhip_ctx* c, hipStream_t s);
orbhip_status submit_impl(orbhip_ctx* c, int nimg, const uint8_t* const* imgs, int stride, orbhip_keypoint* direct_kp, uint8_t* direct_desc, int direct_cap, int* ticket);
orbhip_status collect_flat(orbhip_ctx* c, int ticket, orbhip_keypoint* kps, uint8_t* desc, int cap, int* n_out);
// orbhip_search.hip
void launch_feature_grid(const orbhip_keypoint* kp, const int* d_n, int cap, const orbhip_bounds& b, int* grid_start, int* grid_items, float2* grid_xy,
                         int nslots, int slot0, hipStream_t s);
// orbhip_frame.hip
int stereo_row_cap(const orbhip_ctx* c);
StereoSide stereo_side(orbhip_ctx* c);
#pragma GCC visibility pop
