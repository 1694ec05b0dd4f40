// orbhip_api.hip — the extractor context of liborbhip.so (include/orbhip.h): last-error string, per-thread caches and arena, context creation,
// the extraction pipeline, fetch, profiling.  The rest of the host side: orbhip_host_path.hip (host-buffer path), orbhip_search.hip (matcher
// searches), orbhip_frame.hip (stereo, camera geometry); what they share is in orbhip_ctx.h.
//
// Host side of the drop-in: what ORBextractor::ORBextractor computes once (scale tables, features per level,
// ORBextractor.cc:410-470) plus everything the reference recomputes per frame although it only depends on the image
// size (level sizes :1111-1112, FAST cell grid :773-806, cv::resize coefficient tables, Gaussian kernel) is computed
// here at context creation and uploaded; per call the host only enqueues kernels on the context's HIP stream.
// Float expressions mirror the reference's types step by step (file built with -ffp-contract=off).
#include <cstdarg>
#include <unistd.h>
#include <sys/syscall.h>
#include "orbhip_ctx.h"

static thread_local std::string g_err;
orbhip_status orbhip_set_error(orbhip_status st, const char* fmt, ...)      // the one error setter (the host files' fail(): orbhip_ctx.h)
{
    char buf[512]; va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    g_err = buf; return st;
}

static const char* kKernelNames[K_COUNT] = {"k_pyramid_level", "k_fast_cells", "k_blur", "k_quadtree", "k_describe",
                                            "k_match_grid", "k_match_candidates", "k_match_select", "k_undistort_keys", "k_remap"};

static const signed char kPatternHost[256 * 4] = {
#include "brief_pattern_31.inc"
};

// ---------------------------------------------------------------------------------------------- profiling helpers
void prof_collect(orbhip_ctx* c)
{
    for (auto& s : c->pending) {
        (void)hipEventSynchronize(s.b);
        float ms = 0; (void)hipEventElapsedTime(&ms, s.a, s.b);
        c->tot_ms[s.k] += ms; c->launches[s.k] += s.counts;
        c->pool.push_back(s.a); c->pool.push_back(s.b);
    }
    c->pending.clear();
}

// ---------------------------------------------------------------------------------------------- creation
// Per-thread, grow-only device scratch for the host-pointer matcher entry points: one hipMalloc the first time (or when a call
// needs more), none afterwards — hipMalloc / hipFree cost more than the kernels of a single-frame call.  (Arena: orbhip_internal.h)
thread_local void* orbhip_tl_scratch = nullptr; thread_local size_t orbhip_tl_scratch_bytes = 0; thread_local int orbhip_tl_scratch_dev = -1;
thread_local std::vector<OrbXfer> orbhip_tl_xfers;           // host <-> arena transfers of the call being laid out
// What orbhip_project_best_in_window_shared left in the calling thread's scratch - every slot's key frame, grid table and parameter block - for
// orbhip_project_best_in_window_held: valid until the thread's next ordinary layout (arena_layout with floor 0) or orbhip_thread_release
thread_local bool orbhip_tl_held_valid = false;
#define g_scratch orbhip_tl_scratch
#define g_scratch_bytes orbhip_tl_scratch_bytes
#define g_scratch_dev orbhip_tl_scratch_dev
#define g_xfers orbhip_tl_xfers
typedef OrbXfer Xfer;
static thread_local uint8_t* g_hstage = nullptr; static thread_local size_t g_hstage_bytes = 0;      // pinned mirror of the arena's host-visible head
// The stream of the calling thread's stateless matcher calls: its own, non-blocking.  (They used to share the NULL stream: Tracking's, LocalMapping's
// and LoopClosing's calls then queue behind each other on the device and every hipStreamSynchronize waits for all three.)
static thread_local hipStream_t g_tstream = nullptr; static thread_local int g_tstream_dev = -1;
hipStream_t orbhip_thread_stream(int device)
{
    orbhip_touch_thread_caches();
    if (g_tstream && g_tstream_dev == device) return g_tstream;
    if (g_tstream) { (void)hipSetDevice(g_tstream_dev); (void)hipStreamSynchronize(g_tstream); (void)hipStreamDestroy(g_tstream); g_tstream = nullptr; (void)hipSetDevice(device); }
    if (hipStreamCreateWithFlags(&g_tstream, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); g_tstream = nullptr; g_tstream_dev = -1; return nullptr; }   // the NULL stream still works
    g_tstream_dev = device;
    return g_tstream;
}
static hipError_t hstage_reserve(size_t bytes)
{
    orbhip_touch_thread_caches();
    if (g_hstage_bytes >= bytes) return hipSuccess;
    if (g_hstage) (void)hipHostFree(g_hstage);
    g_hstage = nullptr; g_hstage_bytes = 0;
    const hipError_t e = hipHostMalloc((void**)&g_hstage, bytes + bytes / 4, hipHostMallocDefault);
    if (e == hipSuccess) g_hstage_bytes = bytes + bytes / 4;
    return e;
}
// The per-thread caches above (and the brute-force / BoW matcher workspaces) belong to the thread that made the calls: a worker thread that
// exits gives them back (thread_local holder below), any thread may do so explicitly with orbhip_thread_release().  The main thread's are
// left to process exit: its thread-local destructors run while the interpreter / runtime that loaded this library is already unwinding.
static thread_local void* g_nn_ws = nullptr; static thread_local size_t g_nn_ws_bytes = 0; static thread_local int g_nn_ws_dev = -1; static thread_local hipStream_t g_nn_ws_stream = nullptr;
extern "C" void orbhip_thread_release(void)
{
    int cur = -1; (void)hipGetDevice(&cur);
    if (g_scratch) { (void)hipSetDevice(g_scratch_dev); (void)hipDeviceSynchronize(); (void)hipFree(g_scratch); }
    g_scratch = nullptr; g_scratch_bytes = 0; g_scratch_dev = -1; orbhip_tl_held_valid = false;
    if (g_tstream) { (void)hipSetDevice(g_tstream_dev); (void)hipStreamSynchronize(g_tstream); (void)hipStreamDestroy(g_tstream); }
    g_tstream = nullptr; g_tstream_dev = -1;
    if (g_hstage) (void)hipHostFree(g_hstage);
    g_hstage = nullptr; g_hstage_bytes = 0;
    if (g_nn_ws) { (void)hipSetDevice(g_nn_ws_dev); (void)hipDeviceSynchronize(); (void)hipFree(g_nn_ws); }
    g_nn_ws = nullptr; g_nn_ws_bytes = 0; g_nn_ws_dev = -1; g_nn_ws_stream = nullptr;
    if (cur >= 0) (void)hipSetDevice(cur);
    (void)hipGetLastError();
}
namespace { struct ThreadCacheHolder { ~ThreadCacheHolder() { if ((long)syscall(SYS_gettid) != (long)getpid()) orbhip_thread_release(); } }; }
static thread_local ThreadCacheHolder g_cache_holder;
void orbhip_touch_thread_caches() { (void)&g_cache_holder; }

// Partials of the brute-force scan: a per-thread, grow-only buffer tied to the device it was allocated on and to the stream that used it
// last (a second stream of the same thread waits for the first before it reuses the buffer).
void* orbhip_nn_workspace(size_t bytes, hipStream_t s)
{
    orbhip_touch_thread_caches();
    int dev = -1; if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    if (g_nn_ws && g_nn_ws_dev == dev && g_nn_ws_stream != s) (void)hipStreamSynchronize(g_nn_ws_stream);
    if (g_nn_ws_dev != dev || bytes > g_nn_ws_bytes) {
        if (g_nn_ws) { const int cur = dev; (void)hipSetDevice(g_nn_ws_dev); (void)hipStreamSynchronize(g_nn_ws_stream); (void)hipFree(g_nn_ws); (void)hipSetDevice(cur); g_nn_ws = nullptr; g_nn_ws_bytes = 0; }
        if (orbhip_dmalloc(&g_nn_ws, bytes) != hipSuccess) { (void)hipGetLastError(); g_nn_ws = nullptr; g_nn_ws_dev = -1; return nullptr; }
        g_nn_ws_bytes = bytes; g_nn_ws_dev = dev;
    }
    g_nn_ws_stream = s;
    return g_nn_ws;
}

// One pageable->pinned gather on the host and ONE host-to-device copy for all inputs of a call (a hipMemcpy per array costs more
// than the kernels of a single-frame matcher call); likewise one device-to-host copy for all outputs.
hipError_t arena_upload(hipStream_t s)
{
    size_t hi = 0;
    for (const Xfer& x : g_xfers) hi = std::max(hi, x.off + std::max(x.bytes_in, x.bytes_out));
    hipError_t e = hstage_reserve(hi); if (e != hipSuccess) return e;
    size_t in_lo = (size_t)-1, in_hi = 0;
    for (const Xfer& x : g_xfers) if (x.src) { memcpy(g_hstage + x.off, x.src, x.bytes_in); in_lo = std::min(in_lo, x.off); in_hi = std::max(in_hi, x.off + x.bytes_in); }
    if (!in_hi) return hipSuccess;
    in_lo &= ~(size_t)255;                                    // (a layout above a floor leaves what lies below it alone)
    return orbhip_copy_async(static_cast<uint8_t*>(g_scratch) + in_lo, g_hstage + in_lo, in_hi - in_lo, hipMemcpyHostToDevice, s);
}
hipError_t arena_download(hipStream_t s)
{
    size_t lo = (size_t)-1, hi = 0;
    for (const Xfer& x : g_xfers) if (x.dst) { lo = std::min(lo, x.off); hi = std::max(hi, x.off + x.bytes_out); }
    if (hi == 0) return hipStreamSynchronize(s);
    hipError_t e = orbhip_copy_async(g_hstage + (lo & ~(size_t)255), static_cast<uint8_t*>(g_scratch) + (lo & ~(size_t)255), hi - (lo & ~(size_t)255), hipMemcpyDeviceToHost, s); if (e != hipSuccess) return e;
    e = hipStreamSynchronize(s); if (e != hipSuccess) return e;
    for (const Xfer& x : g_xfers) if (x.dst) memcpy(x.dst, g_hstage + x.off, x.bytes_out);
    return hipSuccess;
}
hipError_t orbhip_arena_reserve(int device, size_t bytes)
{
    if (g_scratch_dev != device || g_scratch_bytes < bytes) {
        if (g_scratch) { (void)hipSetDevice(g_scratch_dev); (void)hipFree(g_scratch); (void)hipSetDevice(device); }
        g_scratch = nullptr; g_scratch_bytes = 0;
        const hipError_t e = orbhip_dmalloc(&g_scratch, bytes + bytes / 4);
        if (e != hipSuccess) return e;
        g_scratch_bytes = bytes + bytes / 4; g_scratch_dev = device;
    }
    return hipSuccess;
}
template <typename T> static hipError_t upload(T** p, const std::vector<T>& v)
{
    hipError_t e = dalloc(p, v.size()); if (e != hipSuccess) return e;
    return v.empty() ? hipSuccess : hipMemcpy(*p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}

static void build_resize_table(int sw, int dw, std::vector<int2>& tab)   // cv::resize coefficient tables (OpenCV 3.2 imgwarp.cpp)
{
    const double inv_scale = (double)dw / sw, scale = 1. / inv_scale;
    for (int dx = 0; dx < dw; dx++) {
        float fx = (float)((dx + 0.5) * scale - 0.5);
        int sx = cvFloorF(fx);
        fx -= sx;
        if (sx < 0) { fx = 0; sx = 0; }
        if (sx >= sw - 1) { fx = 0; sx = sw - 1; }
        const int a0 = satShort(cvRoundF((1.f - fx) * 2048.f)), a1 = satShort(cvRoundF(fx * 2048.f));
        int2 e; e.x = sx; e.y = (a0 & 0xffff) | (a1 << 16);
        tab.push_back(e);
    }
}
static void build_yresize_table(int sh, int dh, std::vector<int2>& tab)  // rows are clipped in the kernel, weights are not reset
{
    const double inv_scale = (double)dh / sh, scale = 1. / inv_scale;
    for (int dy = 0; dy < dh; dy++) {
        float fy = (float)((dy + 0.5) * scale - 0.5);
        int sy = cvFloorF(fy);
        fy -= sy;
        const int b0 = satShort(cvRoundF((1.f - fy) * 2048.f)), b1 = satShort(cvRoundF(fy * 2048.f));
        int2 e; e.x = sy; e.y = (b0 & 0xffff) | (b1 << 16);
        tab.push_back(e);
    }
}

// k_pyramid_cascade's rectangles.  A workgroup owns a TW x TH tile of the last level; the rectangle of level l-1 it needs is the source footprint of its
// rectangle of level l (first column aligned down to 4), widened where necessary so that the rectangles of all tiles cover level l-1 completely (a
// level's last columns / rows need not be referenced by the next level).  Columns and rows are independent: one table per tile column, one per tile row.
static hipError_t build_cascade(orbhip_ctx* c)
{
    c->pc_ok = false;
    const int L = c->L;
    if (L < 2 || L > ORBHIP_MAX_LEVELS) return hipSuccess;
    for (int l = 1; l < L; l++) if (c->pyr_staged[l] != 2) return hipSuccess;       // the kernel computes four pixels at a time from PyrGroup entries (scale factors below ~1.6)
    int TW = 32, TH = 16;      // measured on MI355X at 1241 x 376 / 8 levels, ms per call: 32x16 0.139-0.142, 64x8 0.140-0.141, 16x8 0.139-0.142, 32x8 0.141-0.142, 16x16 0.141-0.145 (seven launches: 0.158-0.162; 64x16 and larger exceed the kernel's 256 table entries per workgroup and fall back to them)
    if (const char* e = getenv("ORBHIP_PC_TILE")) { int w = 0, h = 0; if (sscanf(e, "%dx%d", &w, &h) == 2 && w >= 4 && h >= 1 && w % 4 == 0) { TW = w; TH = h; } else if (*e == '0') return hipSuccess; }
    const LevelGeom& gl = c->geom[L - 1];
    const int ntx = (gl.w + TW - 1) / TW, nty = (gl.h + TH - 1) / TH;
    std::vector<short2> xr((size_t)L * ntx), yr((size_t)L * nty);
    for (int t = 0; t < ntx; t++) xr[(size_t)(L - 1) * ntx + t] = short2{(short)(t * TW), (short)(std::min((t + 1) * TW, gl.w) - 1)};
    for (int t = 0; t < nty; t++) yr[(size_t)(L - 1) * nty + t] = short2{(short)(t * TH), (short)(std::min((t + 1) * TH, gl.h) - 1)};
    for (int l = L - 1; l >= 1; l--) {
        const LevelGeom& g = c->geom[l];
        if (g.src_w > 32767 || g.src_h > 32767) return hipSuccess;
        const int2* xt = c->xtab.data() + g.xtab_off; const int2* yt = c->ytab.data() + g.ytab_off;
        short2* sx = &xr[(size_t)(l - 1) * ntx]; short2* sy = &yr[(size_t)(l - 1) * nty];
        // (a rectangle's columns are computed in groups of 4 from its first one: the pixels up to the end of the last group are computed - and stored - too)
        for (int t = 0; t < ntx; t++) { short2& r = xr[(size_t)l * ntx + t]; r.y = (short)std::min(r.x + 4 * (((r.y - r.x) >> 2) + 1) - 1, g.w - 1); }
        for (int t = 0; t < ntx; t++) { const short2 r = xr[(size_t)l * ntx + t]; sx[t] = short2{(short)(xt[r.x].x & ~3), (short)std::min(xt[r.y].x + 1, g.src_w - 1)}; }
        for (int t = 0; t < nty; t++) { const short2 r = yr[(size_t)l * nty + t]; sy[t] = short2{(short)std::min(std::max(yt[r.x].x, 0), g.src_h - 1), (short)std::min(std::max(yt[r.y].x + 1, 0), g.src_h - 1)}; }
        sx[0].x = 0; sx[ntx - 1].y = (short)(g.src_w - 1); sy[0].x = 0; sy[nty - 1].y = (short)(g.src_h - 1);
        for (int t = 0; t + 1 < ntx; t++) sx[t].y = std::max<short>(sx[t].y, (short)(sx[t + 1].x - 1));
        for (int t = 0; t + 1 < nty; t++) sy[t].y = std::max<short>(sy[t].y, (short)(sy[t + 1].x - 1));
    }
    // LDS: the widest x tallest rectangle of the even levels | of the odd levels (the last level is not kept) | the tables
    auto xbytes = [&](int l, int t) { const short2 r = xr[(size_t)l * ntx + t]; return 4 * (((r.y - r.x) >> 2) + 1); };
    auto yrows = [&](int l, int t) { const short2 r = yr[(size_t)l * nty + t]; return r.y - r.x + 1; };
    int buf[2] = {16, 16}, xcap = 0, ycap = 0;
    for (int l = 0; l + 1 < L; l++) {
        int mx = 0, my = 0;
        for (int t = 0; t < ntx; t++) mx = std::max(mx, xbytes(l, t));
        for (int t = 0; t < nty; t++) my = std::max(my, yrows(l, t));
        buf[l & 1] = std::max(buf[l & 1], (mx * my + 16 + 15) & ~15);        // + 16: a group reads the three dwords from its first tap's on, used or not
    }
    for (int t = 0; t < ntx; t++) { int n = 0; for (int l = 1; l < L; l++) n += xbytes(l, t) / 4; xcap = std::max(xcap, n); }        // PyrGroup entries
    for (int t = 0; t < nty; t++) { int n = 0; for (int l = 1; l < L; l++) n += yrows(l, t); ycap = std::max(ycap, n); }
    {   // level 0 too (it has no footprint to take, but its last group is staged whole)
        const LevelGeom& g0 = c->geom[0];
        for (int t = 0; t < ntx; t++) { short2& r = xr[t]; r.y = (short)std::min(r.x + 4 * (((r.y - r.x) >> 2) + 1) - 1, g0.w - 1); }
    }
    int r0max = 0; for (int tx = 0; tx < ntx; tx++) for (int ty = 0; ty < nty; ty++) r0max = std::max(r0max, xbytes(0, tx) / 4 * yrows(0, ty));
    if ((size_t)buf[0] + buf[1] + (size_t)xcap * sizeof(PyrGroup) + (size_t)ycap * sizeof(int2) > 60 * 1024 || xcap > 256 || ycap > 512 || r0max > 4096) return hipSuccess;      // (k_pyramid_cascade's PC_GIT / PC_YIT / PC_RIT)
    // self-check before the tables are used: every level covered without a gap, and every tap of every pixel a workgroup computes (whole 4-pixel groups)
    // inside the rectangle it holds of the level below.  A table that fails is not used (the level kernels run instead).
    for (int l = 0; l < L; l++) {
        const LevelGeom& g = c->geom[l];
        int next = 0;
        for (int t = 0; t < ntx; t++) { const short2 r = xr[(size_t)l * ntx + t]; if (r.x > next || r.y < r.x || (r.x & 3)) return hipSuccess; next = std::max(next, r.y + 1); }
        if (next < g.w) return hipSuccess;
        next = 0;
        for (int t = 0; t < nty; t++) { const short2 r = yr[(size_t)l * nty + t]; if (r.x > next || r.y < r.x) return hipSuccess; next = std::max(next, r.y + 1); }
        if (next < g.h) return hipSuccess;
        if (l == 0) continue;
        const int2* xt = c->xtab.data() + g.xtab_off; const int2* yt = c->ytab.data() + g.ytab_off;
        for (int t = 0; t < ntx; t++) {
            const short2 r = xr[(size_t)l * ntx + t], sr = xr[(size_t)(l - 1) * ntx + t];
            const int sx_last = std::min(sr.x + xbytes(l - 1, t) - 1, g.src_w - 1);            // last source column the workgroup holds
            for (int x = r.x; x <= std::min(r.x + xbytes(l, t) - 1, g.w - 1); x++) { const int a = xt[x].x, b = std::min(a + 1, g.src_w - 1); if (a < sr.x || b > sx_last) return hipSuccess; }
        }
        for (int t = 0; t < nty; t++) {
            const short2 r = yr[(size_t)l * nty + t], sr = yr[(size_t)(l - 1) * nty + t];
            for (int y = r.x; y <= r.y; y++) { const int a = std::min(std::max(yt[y].x, 0), g.src_h - 1), b = std::min(std::max(yt[y].x + 1, 0), g.src_h - 1); if (a < sr.x || b > sr.y) return hipSuccess; }
        }
    }
    hipError_t e = upload(&c->d_pc_xr, xr); if (e != hipSuccess) return e;
    e = upload(&c->d_pc_yr, yr); if (e != hipSuccess) return e;
    c->pc_ntx = ntx; c->pc_nty = nty; c->pc_buf0 = buf[0]; c->pc_buf1 = buf[1]; c->pc_xcap = xcap; c->pc_ycap = ycap; c->pc_ok = true;
    return hipSuccess;
}

extern "C" int orbhip_pyramid_cascade_tiles(const orbhip_ctx* c) { return c && c->pc_ok ? c->pc_ntx * c->pc_nty : 0; }
extern "C" const char* orbhip_version(void) { return "orbhip 0.2 (gfx950)"; }
thread_local double orbhip_tl_api_ms = 0; thread_local int orbhip_tl_api_depth = 0;
extern "C" double orbhip_thread_api_ms(int reset) { const double v = orbhip_tl_api_ms; if (reset) orbhip_tl_api_ms = 0; return v; }
extern "C" int orbhip_device_count(void) { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; } return n; }
extern "C" const char* orbhip_last_error(void) { return g_err.c_str(); }

extern "C" void orbhip_destroy(orbhip_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->cfg.device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    orbhip_bow_forget_ctx(c);                                      // BoW workspaces the vocabularies keep for this context (they ran on c->stream)
    if (c->mstream) { (void)hipStreamSynchronize(c->mstream); (void)hipStreamDestroy(c->mstream); }
    if (c->bstream) { (void)hipStreamSynchronize(c->bstream); (void)hipStreamDestroy(c->bstream); }
    if (c->bstream_host) { (void)hipStreamSynchronize(c->bstream_host); (void)hipStreamDestroy(c->bstream_host); }
    if (c->d_pc_xr) (void)hipFree(c->d_pc_xr);
    if (c->d_pc_yr) (void)hipFree(c->d_pc_yr);
    if (c->ev_pyr) (void)hipEventDestroy(c->ev_pyr);
    if (c->ev_blur) (void)hipEventDestroy(c->ev_blur);
    if (c->ev_extract) (void)hipEventDestroy(c->ev_extract);
    for (auto e : c->ev_match) if (e) (void)hipEventDestroy(e);
    for (auto xs : c->xstreams) { (void)hipStreamSynchronize(xs); (void)hipStreamDestroy(xs); }
    for (auto e : c->xevents) (void)hipEventDestroy(e);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    prof_collect(c);
    for (auto e : c->pool) (void)hipEventDestroy(e);
    void* ptrs[] = {c->d_blur_band, c->d_ic_mask, c->d_xgrp, c->d_fc_dma, c->d_geom, c->d_cells, c->d_tiles, c->d_runs, c->d_xtab, c->d_ytab, c->d_pattern, c->d_pyr, c->d_blur, c->d_cell_count, c->d_cell_cand,
                    c->d_qt_val, c->d_qt_code, c->d_qt_node, c->d_lvl_kp, c->d_lvl_n[0], c->d_lvl_n[1], c->d_lvl_n[2], c->d_out_block[0], c->d_out_block[1], c->d_out_block[2], c->d_grid_start, c->d_grid_items, c->d_grid_xy, c->d_cand, c->d_top, c->d_ncand,
                    c->d_prev, c->d_m12, c->d_nm};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    { void* ep[] = {c->d_fgrid_start, c->d_fgrid_items, c->d_fgrid_xy, c->d_rrow_start, c->d_rrow_items}; for (void* q : ep) if (q) (void)hipFree(q); if (c->ev_epilogue) (void)hipEventDestroy(c->ev_epilogue); if (c->h_st) (void)hipHostFree(c->h_st); if (c->d_ucols) (void)hipFree(c->d_ucols); if (c->d_match_ws) (void)hipFree(c->d_match_ws); if (c->h_ucols) (void)hipHostFree(c->h_ucols); if (c->ev_ucols) (void)hipEventDestroy(c->ev_ucols); if (c->ev_stereo) (void)hipEventDestroy(c->ev_stereo); }
    { void* st[] = {c->d_st_rowstart, c->d_st_rowitems, c->d_st_u /* | d_st_depth */, c->d_st_sad}; for (void* q : st) if (q) (void)hipFree(q); }
    for (auto& hs : c->sets) {
        for (int k = 0; k < ORBHIP_MAX_CHUNKS; k++) { if (hs.ev_h2d[k]) (void)hipEventDestroy(hs.ev_h2d[k]); if (hs.ev_k[k]) (void)hipEventDestroy(hs.ev_k[k]); if (hs.ev_d2h[k]) (void)hipEventDestroy(hs.ev_d2h[k]); }
        if (hs.d_packed) (void)hipFree(hs.d_packed);
        if (hs.owned) { if (hs.d_in) (void)hipFree(hs.d_in); if (hs.h_in) (void)hipHostFree(hs.h_in); if (hs.h_block) (void)hipHostFree(hs.h_block); }
    }
    if (c->hstream) { (void)hipStreamSynchronize(c->hstream); (void)hipStreamDestroy(c->hstream); }
    if (c->dstream) { (void)hipStreamSynchronize(c->dstream); (void)hipStreamDestroy(c->dstream); }
    if (c->d_in) (void)hipFree(c->d_in);
    if (c->h_in) (void)hipHostFree(c->h_in);
    if (c->d_col) (void)hipFree(c->d_col);
    if (c->h_col) (void)hipHostFree(c->h_col);
    { void* g[] = {c->d_out_kpun[0], c->d_out_kpun[1], c->d_out_kpun[2], c->d_map_x, c->d_map_y, c->d_raw, c->d_depth}; for (void* q : g) if (q) (void)hipFree(q); }
    if (c->h_kpun) (void)hipHostFree(c->h_kpun);
    if (c->h_raw) (void)hipHostFree(c->h_raw);
    if (c->h_block) (void)hipHostFree(c->h_block);             // h_n | h_kp | h_desc
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

// LDS row stride of a k_fast_cells patch: 4 * (groups + 2) bytes cover every window read; 48 bytes for the usual 37-px cells puts the
// eight rows a wave reads at once on each LDS bank exactly twice (the minimum for 64 lanes x 4 bytes)
static int fc_pstride(const orbhip_ctx* c)
{
    return (c->fc_maxpw + 8 + 3) & ~3;
}

extern "C" orbhip_status orbhip_create(orbhip_ctx** out, const orbhip_config* cfg)
{
    if (!out || !cfg) return fail(ORBHIP_ERR_INVALID, "null argument");
    *out = nullptr;
    if (cfg->nfeatures < 0 || cfg->nlevels < 1 || cfg->nlevels > ORBHIP_MAX_LEVELS || cfg->scale_factor <= 1.0f || cfg->max_batch < 1 ||
        cfg->width < 1 || cfg->height < 1)
        return fail(ORBHIP_ERR_INVALID, "bad configuration (nfeatures %d, nlevels %d, scale %f, %dx%d, batch %d)", cfg->nfeatures, cfg->nlevels,
                    cfg->scale_factor, cfg->width, cfg->height, cfg->max_batch);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(ORBHIP_ERR_HIP, "no HIP device available: the ORB front-end has no CPU fallback");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(ORBHIP_ERR_INVALID, "device %d out of range (%d devices)", cfg->device, ndev);
    HIPCHK(hipSetDevice(cfg->device));

    orbhip_ctx* c = new orbhip_ctx; c->cfg = *cfg; c->L = cfg->nlevels; c->B = cfg->max_batch;
    c->bounds.max_x = (float)cfg->width; c->bounds.max_y = (float)cfg->height;       // undistorted camera until orbhip_set_camera says otherwise
    const int L = c->L;
    // ---- ORBextractor::ORBextractor (ORBextractor.cc:410-446): double scaleFactor member initialised from the float argument
    const double scaleFactor = (double)cfg->scale_factor;
    c->sf.assign(L, 1.0f); c->s2.assign(L, 1.0f); c->isf.assign(L, 1.0f); c->is2.assign(L, 1.0f); c->nfeat.assign(L, 0);
    for (int i = 1; i < L; i++) { c->sf[i] = (float)(c->sf[i - 1] * scaleFactor); c->s2[i] = c->sf[i] * c->sf[i]; }
    for (int i = 0; i < L; i++) { c->isf[i] = 1.0f / c->sf[i]; c->is2[i] = 1.0f / c->s2[i]; }
    {
        float factor = (float)(1.0f / scaleFactor);
        float nDesired = cfg->nfeatures * (1 - factor) / (1 - (float)pow((double)factor, (double)L));
        int sum = 0;
        for (int l = 0; l < L - 1; l++) { c->nfeat[l] = cvRoundF(nDesired); sum += c->nfeat[l]; nDesired *= factor; }
        c->nfeat[L - 1] = std::max(cfg->nfeatures - sum, 0);
    }
    // ---- Gaussian kernel of cv::GaussianBlur(7x7, sigma 2) in 8-bit fixed point (getGaussianKernel + convertTo(CV_32S, 256))
    {
        float cf[7]; double sum = 0; const double scale2X = -0.5 / (2.0 * 2.0);
        for (int i = 0; i < 7; i++) { double x = i - 3.0; cf[i] = (float)std::exp(scale2X * x * x); sum += cf[i]; }
        sum = 1. / sum;
        for (int i = 0; i < 4; i++) c->gk[i] = cvRoundF((float)(cf[3 + i] * sum) * 256.f);      // centre, +-1, +-2, +-3
        { const char* e = getenv("ORBHIP_BLUR"); c->blur_mfma = !(e && strcmp(e, "valu") == 0); }       // ORBHIP_BLUR=valu: the all-VALU blur kernel instead of k_blur_mfma
        if (c->gk[0] > 127 || c->gk[0] + 2 * (c->gk[1] + c->gk[2] + c->gk[3]) != 257) c->blur_mfma = false;     // the i8 form assumes these taps
    }
    // ---- per level geometry (ORBextractor.cc:1111-1112, 773-806, 543-545)
    c->geom.resize(L);
    long long plane_off = 0, blur_off = 0, cand_off = 0; int kp_off = 0;
    for (int l = 0; l < L; l++) {
        LevelGeom& g = c->geom[l]; memset(&g, 0, sizeof g);
        g.w = cvRoundF((float)cfg->width * c->isf[l]); g.h = cvRoundF((float)cfg->height * c->isf[l]);
        if (g.w < 32 + 30 || g.h < 32 + 30 || g.w > 4095 || g.h > 4095) { const int gw = g.w, gh = g.h; delete c; return fail(ORBHIP_ERR_UNSUPPORTED, "level %d is %dx%d: supported level sizes are 62..4095 px per side (the reference divides by zero below 30 px of interior)", l, gw, gh); }
        g.pitch = (g.w + 63) & ~63; g.plane_off = (int)plane_off; plane_off += (long long)g.pitch * g.h;
        g.blur_tpr = orbhip_blur_tiles_per_row(g.w); g.blur_off = (int)blur_off; blur_off += (long long)g.blur_tpr * orbhip_blur_tile_rows(g.h) * ORBHIP_BT_BYTES;     // the blurred level as 32x4 tiles
        g.maxBorderX = g.w - ORBHIP_EDGE; g.maxBorderY = g.h - ORBHIP_EDGE;
        const float width = (float)(g.maxBorderX - ORBHIP_EDGE), height = (float)(g.maxBorderY - ORBHIP_EDGE), W = 30;
        g.nCols = (int)(width / W); g.nRows = (int)(height / W);
        g.wCell = (int)ceil(width / g.nCols); g.hCell = (int)ceil(height / g.nRows);
        if (g.wCell > 59 || g.hCell > 59) { const int cw = g.wCell, ch = g.hCell; delete c; return fail(ORBHIP_ERR_UNSUPPORTED, "cell %dx%d too large", cw, ch); }
        g.cell_first = (int)c->cells.size(); g.ncells = g.nCols * g.nRows;
        g.cand_total_off = (int)cand_off;
        for (int i = 0; i < g.nRows; i++) {
            const float iniY = ORBHIP_EDGE + i * g.hCell; float maxY = iniY + g.hCell + 6;
            const bool skipY = iniY >= g.maxBorderY - 3;
            if (maxY > g.maxBorderY) maxY = (float)g.maxBorderY;
            for (int j = 0; j < g.nCols; j++) {
                const float iniX = ORBHIP_EDGE + j * g.wCell; float maxX = iniX + g.wCell + 6;
                const bool skipX = iniX >= g.maxBorderX - 6;
                if (maxX > g.maxBorderX) maxX = (float)g.maxBorderX;
                CellDesc cd; memset(&cd, 0, sizeof cd);
                cd.level = (short)l; cd.skipped = (skipX || skipY) ? 1 : 0;
                cd.iniX = (short)iniX; cd.iniY = (short)iniY; cd.maxX = (short)maxX; cd.maxY = (short)maxY;
                cd.shiftX = (short)(j * g.wCell); cd.shiftY = (short)(i * g.hCell);
                const int cw = std::max((int)maxX - (int)iniX - 6, 0), ch = std::max((int)maxY - (int)iniY - 6, 0);
                cd.cand_cap = cd.skipped ? 0 : ((cw + 1) / 2) * ((ch + 1) / 2);       // strict 3x3 maxima are never 8-adjacent
                if (!cd.skipped) { c->fc_maxpw = std::max(c->fc_maxpw, (int)maxX - (int)iniX); c->fc_maxph = std::max(c->fc_maxph, (int)maxY - (int)iniY); }
                { const int ng = std::max((cw + 3) / 4, 1); cd.inv_ng = (65536 + ng - 1) / ng; }
                cd.cand_idx = (int)cand_off; cand_off += cd.cand_cap;
                c->cells.push_back(cd);
            }
        }
        g.cand_total_cap = (int)(cand_off - g.cand_total_off);
        g.nfeat = c->nfeat[l];
        g.nIni = (int)roundf((float)(g.maxBorderX - ORBHIP_EDGE) / (g.maxBorderY - ORBHIP_EDGE));
        if (g.nIni < 1) { delete c; return fail(ORBHIP_ERR_UNSUPPORTED, "portrait image: the reference quadtree has zero root nodes (ORBextractor.cc:543-545 divides by zero)"); }
        g.hX = (float)(g.maxBorderX - ORBHIP_EDGE) / g.nIni;
        g.kp_cap = std::max(g.nfeat + 3, 4 * g.nIni); g.kp_off = kp_off; kp_off += g.kp_cap;
        g.scale = c->sf[l]; g.kp_size = (float)(int)(31 * c->sf[l]); g.inv_scale = c->isf[l];   // scaledPatchSize (:837)
        c->qt_maxn = std::max(c->qt_maxn, g.kp_cap); c->qt_maxcells = std::max(c->qt_maxcells, g.ncells);
        if (g.ncells > 65535 || g.kp_cap > 16383) { delete c; return fail(ORBHIP_ERR_UNSUPPORTED, "level %d: too many cells / features for the quadtree scan", l); }
        if (l > 0) {
            g.src_w = c->geom[l - 1].w; g.src_h = c->geom[l - 1].h;
            g.xtab_off = (int)c->xtab.size(); build_resize_table(g.src_w, g.w, c->xtab);
            g.ytab_off = (int)c->ytab.size(); build_yresize_table(g.src_h, g.h, c->ytab);
            // does every output tile's source footprint fit the LDS stage of k_pyramid_level?
            const int tw = orbhip_pyramid_tile_w(), th = orbhip_pyramid_tile_h(); bool fits = true;
            for (int x0 = 0; x0 < g.w; x0 += tw) { const int xl = std::min(x0 + tw - 1, g.w - 1); const int a = c->xtab[g.xtab_off + x0].x & ~3, b = std::min(c->xtab[g.xtab_off + xl].x + 1, g.src_w - 1); fits = fits && orbhip_pyramid_tile_fits(b - a + 1, 1); }
            for (int y0 = 0; y0 < g.h; y0 += th) { const int yl = std::min(y0 + th - 1, g.h - 1); const int a = std::min(std::max(c->ytab[g.ytab_off + y0].x, 0), g.src_h - 1), b = std::min(std::max(c->ytab[g.ytab_off + yl].x + 1, 0), g.src_h - 1); fits = fits && orbhip_pyramid_tile_fits(1, b - a + 1); }
            c->pyr_staged.resize(L, 0); c->pyr_staged[l] = fits ? 1 : 0;
            // 4-pixel groups (k_pyramid_level_g): usable when every group's taps lie within 8 source bytes of its first tap and the three
            // dwords a thread reads stay inside the staged row
            g.xgrp_off = (int)c->xgrp.size(); bool grouped = fits;
            for (int x4 = 0; x4 < g.w; x4 += 4) {
                PyrGroup G; memset(&G, 0, sizeof G);
                G.sx0 = c->xtab[g.xtab_off + x4].x;
                for (int k = 0; k < 4; k++) {
                    const int2 e = c->xtab[g.xtab_off + std::min(x4 + k, g.w - 1)];
                    const int o0 = e.x - G.sx0, o1 = std::min(e.x + 1, g.src_w - 1) - G.sx0;
                    if (o0 < 0 || o1 < 0 || o0 > 7 || o1 > 7) grouped = false;
                    G.sel[k] = (unsigned)(o0 & 7) | (0x0cu << 8) | ((unsigned)(o1 & 7) << 16) | (0x0cu << 24);
                    G.coef[k] = (unsigned)e.y;
                }
                const int sxa = c->xtab[g.xtab_off + (x4 / tw) * tw].x & ~3;
                if (((G.sx0 - sxa) >> 2) + 2 >= orbhip_pyramid_tile_dwords()) grouped = false;
                c->xgrp.push_back(G);
            }
            if (grouped) c->pyr_staged[l] = 2;
        }
        const int btw = c->blur_mfma ? orbhip_blur_mfma_tile_w() : 128, bth = c->blur_mfma ? orbhip_blur_mfma_tile_h() : 32;     // k_blur_mfma / k_blur workgroup tile
        for (int y0 = 0; y0 < g.h; y0 += bth) for (int x0 = 0; x0 < g.w; x0 += btw) { TileDesc t; t.level = (short)l; t.x0 = (short)x0; t.y0 = (short)y0; t.pad = 0; c->blur_tiles.push_back(t); }
        if (c->blur_mfma) {   // k_blur_strip's work units: the tiles of a column strip in runs of orbhip_blur_strip_tiles(), top to bottom
            const int nt = orbhip_blur_strip_tiles(), gy = (g.h + bth - 1) / bth;
            for (int ty = 0; ty < gy; ty += nt) for (int x0 = 0; x0 < g.w; x0 += btw) { BlurRun r; r.level = (short)l; r.x0 = (short)x0; r.y0 = (short)(ty * bth); r.n = (short)std::min(nt, gy - ty); c->blur_runs.push_back(r); }
            if (g.w < 8) c->blur_strip_ok = false;      // (its border patch reads the row's last eight columns from the staged tile)
        }
    }
    c->plane_frame_bytes = (plane_off + 255) & ~255LL; c->blur_frame_bytes = (blur_off + 255) & ~255LL; c->cand_slots_per_frame = cand_off; c->qt_per_frame = cand_off;
    c->lvl_kp_per_frame = kp_off; c->out_cap = kp_off; c->lvl0_cap = c->geom[0].kp_cap;
    if (cand_off >= (1 << 24)) { delete c; return fail(ORBHIP_ERR_UNSUPPORTED, "too many candidate slots"); }
    if (orbhip_quadtree_lds_bytes(c->qt_maxn, c->qt_maxcells) > 150 * 1024) { const int qn = c->qt_maxn; delete c; return fail(ORBHIP_ERR_UNSUPPORTED, "nfeatures too large for the LDS quadtree (%d nodes)", qn); }

    // ---- device
    // Stream priorities: the main stream gets the highest, the blur's stream - tens of thousands of independent tiles - and the matcher's stream the
    // lowest, so that the quadtree's few long workgroups on the main stream are always dispatched before the blur tiles they run beside
    // (profiles/r05_exp_stream_priorities.jsonl).  The host-buffer path's blur stream has no priority (pipeline_frames).
    int prio_lo = 0, prio_hi = 0; (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);      // (numerically: lo = least urgent, hi = most urgent)
    if (cfg->stream) c->stream = (hipStream_t)cfg->stream;
    else {
        hipError_t e = hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, prio_hi);
        if (e != hipSuccess) { delete c; return fail(ORBHIP_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e)); } c->own_stream = true;
    }
    for (int i = 1; i < std::min(cfg->num_streams, cfg->max_batch); i++) {
        hipStream_t xs = nullptr; hipEvent_t xe = nullptr;
        if (hipStreamCreateWithFlags(&xs, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&xe, hipEventDisableTiming) != hipSuccess) { orbhip_destroy(c); return fail(ORBHIP_ERR_HIP, "extra stream creation failed"); }
        c->xstreams.push_back(xs); c->xevents.push_back(xe);
    }
    if (!c->xstreams.empty() && hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess) { orbhip_destroy(c); return fail(ORBHIP_ERR_HIP, "event creation failed"); }
    { const char* e = getenv("ORBHIP_SERIAL"); c->serial = e && e[0] == '1'; }
    {   // the matcher runs on its own stream so that it overlaps the next batch's extraction
        bool ok = hipStreamCreateWithPriority(&c->mstream, hipStreamNonBlocking, prio_lo) == hipSuccess &&
                  hipEventCreateWithFlags(&c->ev_extract, hipEventDisableTiming) == hipSuccess &&
                  hipStreamCreateWithPriority(&c->bstream, hipStreamNonBlocking, prio_lo) == hipSuccess &&
                  hipStreamCreateWithFlags(&c->bstream_host, hipStreamNonBlocking) == hipSuccess &&
                  hipEventCreateWithFlags(&c->ev_pyr, hipEventDisableTiming) == hipSuccess &&
                  hipEventCreateWithFlags(&c->ev_blur, hipEventDisableTiming) == hipSuccess;
        for (int k = 0; k < 3 && ok; k++) ok = hipEventCreateWithFlags(&c->ev_match[k], hipEventDisableTiming) == hipSuccess;
        if (!ok) { orbhip_destroy(c); return fail(ORBHIP_ERR_HIP, "match stream creation failed"); }
    }
    const size_t B = (size_t)c->B;
    std::vector<float> pat(1024);                                      // k_describe reads [component x0 y0 x1 y1][round][lane]: test 64 r + lane
    for (int t = 0; t < 256; t++) for (int k = 0; k < 4; k++) pat[(k * 4 + (t >> 6)) * 64 + (t & 63)] = kPatternHost[4 * t + k];
    hipError_t e = hipSuccess;
#define TRY(x) do { if (e == hipSuccess) e = (x); } while (0)
    TRY(upload(&c->d_geom, c->geom)); TRY(upload(&c->d_cells, c->cells)); TRY(upload(&c->d_tiles, c->blur_tiles)); if (!c->blur_runs.empty()) TRY(upload(&c->d_runs, c->blur_runs));
    TRY(upload(&c->d_xtab, c->xtab)); TRY(upload(&c->d_ytab, c->ytab)); TRY(upload(&c->d_xgrp, c->xgrp)); TRY(upload(&c->d_pattern, pat));
    TRY(build_cascade(c));
    if (c->blur_mfma) {   // k_blur_mfma: the two band (Toeplitz) matrices of the 7-tap filter laid out as B operands of v_mfma_i32_32x32x32_i8
        const int tap[7] = {c->gk[3], c->gk[2], c->gk[1], c->gk[0], c->gk[1], c->gk[2], c->gk[3]};
        std::vector<int4> band(3 * 64); signed char* bb = reinterpret_cast<signed char*>(band.data());
        for (int l = 0; l < 64; l++) for (int b = 0; b < 16; b++) {
            const int j = l & 31, hh = l >> 5;
            const int t1 = 16 * hh + b - j - 1, t2 = 32 + 16 * hh + b - j - 1;                 // source column x0 - 4 + k feeds output column x0 + j with tap k - j - 1
            const int r = (b & 3) + 8 * (b >> 2) + 4 * hh, tv = r - j;                         // source row y0 - 3 + r (the register / lane-half order of the first product's result)
            bb[(0 * 64 + l) * 16 + b] = (signed char)((t1 >= 0 && t1 <= 6) ? tap[t1] : 0);
            bb[(1 * 64 + l) * 16 + b] = (signed char)((t2 >= 0 && t2 <= 6) ? tap[t2] : 0);
            bb[(2 * 64 + l) * 16 + b] = (signed char)((tv >= 0 && tv <= 6 && j < 26) ? tap[tv] : 0);
        }
        TRY(upload(&c->d_blur_band, band));
    }
    {   // circular patch of IC_Angle as byte masks over 32 rows x 8 dwords (byte b of dword d = column 4d + b - 15); umax as ORBextractor.cc:452-469 computes it
        int umax[16]; const int vmax = (int)floor(15 * sqrt(2.0) / 2 + 1), vmin = (int)ceil(15 * sqrt(2.0) / 2);
        for (int v = 0; v <= vmax; v++) umax[v] = cvRoundF((float)sqrt(225.0 - (double)v * v));
        for (int v = 15, v0 = 0; v >= vmin; --v) { while (umax[v0] == umax[v0 + 1]) ++v0; umax[v] = v0; ++v0; }
        std::vector<unsigned> mask(8 * 64, 0u);                       // k_describe: pass q, lane l = (row 4q + l / 16, dword l % 16 of the row from column -15 on)
        for (int q = 0; q < 8; q++) for (int l = 0; l < 64; l++) for (int b = 0; b < 4; b++) {
            const int r = 4 * q + (l >> 4), d = l & 15, v = r - 15, uu = 4 * d + b - 15;
            if (r <= 30 && d <= 7 && abs(uu) <= 15 && abs(uu) <= umax[abs(v)]) mask[q * 64 + l] |= 0xffu << (8 * b);
        }
        TRY(upload(&c->d_ic_mask, mask));
    }
    {   // k_fast_cells stages a cell's sub-image by LDS-DMA: pass k, lane l fills patch dword 64k + l = (row, column) in the PS-strided LDS layout
        const int psd = fc_pstride(c) / 4, nd = psd * std::max(c->fc_maxph, 1);
        c->fc_np = (nd + 63) / 64;
        const int np8 = (c->fc_np + 7) & ~7;
        std::vector<int4> tab((size_t)(np8 / 4) * 2 * 64);
        for (int k = 0; k < np8; k++) for (int l = 0; l < 64; l++) {
            const int pos = 64 * k + l, row = pos / psd, col4 = 4 * (pos % psd);
            int* r = &tab[(size_t)((k >> 2) * 2) * 64 + l].x; int* d = &tab[(size_t)((k >> 2) * 2 + 1) * 64 + l].x;
            r[k & 3] = row; d[k & 3] = col4;
        }
        TRY(upload(&c->d_fc_dma, tab));
    }
    TRY(dalloc(&c->d_pyr, B * c->plane_frame_bytes + 256)); TRY(dalloc(&c->d_blur, B * c->blur_frame_bytes + 256));
    TRY(dalloc(&c->d_cell_count, B * c->cells.size())); TRY(dalloc(&c->d_cell_cand, B * c->cand_slots_per_frame));
    TRY(dalloc(&c->d_qt_val, B * c->qt_per_frame)); TRY(dalloc(&c->d_qt_code, B * c->qt_per_frame)); TRY(dalloc(&c->d_qt_node, B * c->qt_per_frame));
    TRY(dalloc(&c->d_lvl_kp, B * c->lvl_kp_per_frame));
    for (int k = 0; k < 3; k++) {
        TRY(dalloc(&c->d_lvl_n[k], B * L));
        c->out_off_kp = (B * sizeof(int) + 255) & ~(size_t)255; c->out_off_desc = c->out_off_kp + ((B * c->out_cap * sizeof(orbhip_keypoint) + 255) & ~(size_t)255);
        c->out_block_bytes = c->out_off_desc + B * c->out_cap * 32;
        TRY(dalloc(&c->d_out_block[k], c->out_block_bytes));
        if (e == hipSuccess) { c->d_out_n[k] = reinterpret_cast<int*>(c->d_out_block[k]); c->d_out_kp[k] = reinterpret_cast<orbhip_keypoint*>(c->d_out_block[k] + c->out_off_kp); c->d_out_desc[k] = c->d_out_block[k] + c->out_off_desc; }
        if (e == hipSuccess) e = hipMemset(c->d_lvl_n[k], 0, B * L * sizeof(int));
        if (e == hipSuccess) e = hipMemset(c->d_out_n[k], 0, B * sizeof(int));
    }
    TRY(dalloc(&c->d_grid_start, B * (ORBHIP_GRID_CELLS + 1))); TRY(dalloc(&c->d_grid_items, B * c->out_cap)); TRY(dalloc(&c->d_grid_xy, B * c->out_cap));
    TRY(dalloc(&c->d_cand, B * c->lvl0_cap * (size_t)c->lvl0_cap)); TRY(dalloc(&c->d_ncand, B * c->lvl0_cap)); TRY(dalloc(&c->d_top, B * c->lvl0_cap * (size_t)5));
    TRY(dalloc(&c->d_prev, B * c->out_cap * 2)); TRY(dalloc(&c->d_m12, B * c->out_cap)); TRY(dalloc(&c->d_nm, B));
#undef TRY
    if (e != hipSuccess) { fail(ORBHIP_ERR_HIP, "device allocation failed: %s", hipGetErrorString(e)); orbhip_destroy(c); return ORBHIP_ERR_HIP; }
    *out = c;
    return ORBHIP_OK;
}

extern "C" int orbhip_keypoint_capacity(const orbhip_ctx* c) { return c ? c->out_cap : 0; }

extern "C" orbhip_status orbhip_get_scale_tables(const orbhip_ctx* c, float* sf, float* isf, float* s2, float* is2, int32_t* fpl)
{
    if (!c) return fail(ORBHIP_ERR_INVALID, "null context");
    for (int i = 0; i < c->L; i++) { if (sf) sf[i] = c->sf[i]; if (isf) isf[i] = c->isf[i]; if (s2) s2[i] = c->s2[i]; if (is2) is2[i] = c->is2[i]; if (fpl) fpl[i] = c->nfeat[i]; }
    return ORBHIP_OK;
}
extern "C" orbhip_status orbhip_level_size(const orbhip_ctx* c, int level, int* w, int* h)
{
    if (!c || level < 0 || level >= c->L) return fail(ORBHIP_ERR_INVALID, "bad level");
    if (w) *w = c->geom[level].w; if (h) *h = c->geom[level].h;
    return ORBHIP_OK;
}

extern "C" orbhip_status orbhip_set_blur_rounding(orbhip_ctx* c, int mode)
{
    if (!c || (mode != 0 && mode != 1)) return fail(ORBHIP_ERR_INVALID, "blur_round_mode is 0 (generic C++) or 1 (x86 SSE2 build)");
    c->cfg.blur_round_mode = mode;          // read when the next call's kernel parameters are laid out
    return ORBHIP_OK;
}

extern "C" orbhip_status orbhip_set_fp_contract(orbhip_ctx* c, int mode)
{
    if (!c || (mode != 0 && mode != 1)) return fail(ORBHIP_ERR_INVALID, "fp_contract is 0 (two roundings) or 1 (gcc's fused forms)");
    c->fp_contract = mode;
    return ORBHIP_OK;
}

// ---------------------------------------------------------------------------------------------- pipeline
ExtractParams make_params(orbhip_ctx* c, const uint8_t* d_img0, long long frame_stride, int row_stride)
{
    ExtractParams P; memset(&P, 0, sizeof P);
    P.geom = c->d_geom; P.nlevels = c->L;
    P.img0 = d_img0; P.img0_frame_stride = frame_stride; P.img0_pitch = row_stride;
    P.pyr = c->d_pyr; P.blur = c->d_blur; P.plane_frame_bytes = c->plane_frame_bytes; P.blur_frame_bytes = c->blur_frame_bytes;
    P.cells = c->d_cells; P.ncells_total = (int)c->cells.size();
    P.cell_count = c->d_cell_count; P.cell_cand = c->d_cell_cand; P.cand_slots_per_frame = c->cand_slots_per_frame;
    P.qt_val = c->d_qt_val; P.qt_code = c->d_qt_code; P.qt_node = c->d_qt_node; P.qt_per_frame = c->qt_per_frame;
    P.lvl_kp = c->d_lvl_kp; P.lvl_kp_per_frame = c->lvl_kp_per_frame; P.lvl_n = c->d_lvl_n[c->cur];
    P.out_kp = c->d_out_kp[c->cur]; P.out_desc = c->d_out_desc[c->cur]; P.out_n = c->d_out_n[c->cur]; P.out_cap = c->out_cap;
    P.blur_tiles = c->d_tiles; P.nblur_tiles = (int)c->blur_tiles.size(); P.blur_band = c->blur_mfma ? c->d_blur_band : nullptr;
    if (c->blur_mfma && c->blur_strip_ok) { P.blur_runs = c->d_runs; P.nblur_runs = (int)c->blur_runs.size(); }
    P.xtab = c->d_xtab; P.ytab = c->d_ytab; P.xgrp = c->d_xgrp; P.patternf = c->d_pattern; P.ic_mask = c->d_ic_mask;
    P.pc_xr = c->d_pc_xr; P.pc_yr = c->d_pc_yr; P.pc_ntx = c->pc_ntx; P.pc_nty = c->pc_nty; P.pc_buf0 = c->pc_buf0; P.pc_buf1 = c->pc_buf1; P.pc_xcap = c->pc_xcap; P.pc_ycap = c->pc_ycap;
    P.iniTh = std::min(std::max(c->cfg.ini_th_fast, 0), 255); P.minTh = std::min(std::max(c->cfg.min_th_fast, 0), 255);      // cv::FAST clamps its threshold to [0, 255] (OpenCV 3.2 fast.cpp, FAST_t)
    P.blur_round_mode = c->cfg.blur_round_mode; P.fp_contract = c->fp_contract;
    P.qt_maxn = c->qt_maxn; P.qt_maxcells = c->qt_maxcells; P.qt_scr = orbhip_quadtree_scr(c->qt_maxn, c->qt_maxcells);
    P.fc_pstride = fc_pstride(c); P.fc_prows = c->fc_maxph; P.fc_np = c->fc_np; P.fc_pbytes = 256 * c->fc_np; P.fc_dma = c->d_fc_dma; P.fc_sstride = 4 + 4 * ((std::max(c->fc_maxpw - 6, 0) + 3) / 4); P.fc_srows = std::max(c->fc_maxph - 6, 0) + 2;
    P.fc_listcap = 2 * ((std::max(c->fc_maxpw - 6, 0) + 3) / 4) * std::max(c->fc_maxph - 6, 0);       // pixel pairs of the largest cell
    return P;
}

// levels 1 .. L-1, each from the one before: seven dependent launches for a batch (fewer were tried and lost there: the small levels in one launch of one
// workgroup per frame, 0.27 -> 0.54 ms at B = 256; docs/ROUND_LOG.md), ONE launch for up to eight frames, where the seven cost 35 us of pure latency
static void launch_pyramid(orbhip_ctx* c, const ExtractParams& P, int nf, hipStream_t s)
{
    if (nf <= 8 && c->pc_ok) { orbhip_launch_pyramid_cascade(P, nf, s); return; }      // a handful of frames: one launch for all levels (k_pyramid_cascade)
    for (int l = 1; l < c->L; l++) orbhip_launch_pyramid_level(P, l, c->geom[l].w, c->geom[l].h, (int)c->pyr_staged[l], nf, s);
}

// pyramid -> FAST -> quadtree -> describe for camera slots [f0, f0 + nf) on stream s.  With own_blur_stream (and more than a handful of frames)
// the blur - independent of FAST and the quadtree until the descriptor kernel - runs on the context's second stream beside the quadtree, whose
// workgroups are latency-bound (barriers, one workgroup per (frame, level)); every throughput kernel is alone on the GPU, so its HIP-event time
// in a timed region is its own (bench.py's roofline object relies on that).  Other placements of the second stream landed within 1.3 % of this
// one and are gone from the code (docs/ROUND_LOG.md, round 3 "schedules").
orbhip_status pipeline_frames(orbhip_ctx* c, ExtractParams& P, int f0, int nf, hipStream_t s, bool own_blur_stream, bool host_path)
{
    if (nf <= 0) return ORBHIP_OK;
    P.frame0 = f0;
    { ProfScope ps(c, K_PYRAMID, s); launch_pyramid(c, P, nf, s); }
    { ProfScope ps(c, K_FAST, s); orbhip_launch_fast_cells(P, nf, s); }
    if (own_blur_stream && nf > 8 && !c->serial) {      // (a handful of frames: the two event hops of the second stream cost more than the blur's 11 us - a single-frame call lost 75 us in them)
        // (the host-buffer pipeline keeps a blur stream WITHOUT a priority: with the lowest one its pinned path fell from 110 k to 85 k frames/s - the blur of
        // chunk k starved beside the copies of chunks k - 1 and k + 1, profiles/r05_exp_host_path_stream_priorities.jsonl)
        hipStream_t bs = host_path ? c->bstream_host : c->bstream;
        HIPCHK(hipEventRecord(c->ev_pyr, s)); HIPCHK(hipStreamWaitEvent(bs, c->ev_pyr, 0));
        { ProfScope ps(c, K_QUADTREE, s); orbhip_launch_quadtree(P, nf, s); }
        { ProfScope ps(c, K_BLUR, bs); orbhip_launch_blur(P, c->gk, nf, bs); }
        HIPCHK(hipEventRecord(c->ev_blur, bs));
        HIPCHK(hipStreamWaitEvent(s, c->ev_blur, 0));
    } else if (nf <= 8 && P.blur_band && !c->serial && orbhip_quadtree_lds_bytes(c->qt_maxn, c->qt_maxcells) + orbhip_blur_quadtree_static_lds() <= 160 * 1024) {        // (the blur's tile is static LDS beside the quadtree's dynamic block)
        // a handful of frames: one launch for both (the quadtree's few long workgroups beside the blur's tiles); its time is booked on the quadtree
        ProfScope ps(c, K_QUADTREE, s); orbhip_launch_blur_quadtree(P, nf, s);
    } else {
        { ProfScope ps(c, K_BLUR, s); orbhip_launch_blur(P, c->gk, nf, s); }
        { ProfScope ps(c, K_QUADTREE, s); orbhip_launch_quadtree(P, nf, s); }
    }
    { ProfScope ps(c, K_DESCRIBE, s); orbhip_launch_describe(P, nf, s); }
    if (c->distorted) {   // Frame::UndistortKeyPoints (Frame.cc:404-434) behind the descriptor kernel: mvKeysUn stays in HBM beside mvKeys
        ProfScope ps(c, K_UNDISTORT, s);
        orbhip_launch_undistort_keys(c->cam, c->d_out_kp[c->cur] + (size_t)f0 * c->out_cap, c->d_out_n[c->cur] + f0, c->d_out_kpun[c->cur] + (size_t)f0 * c->out_cap, c->out_cap, nf, s);
    }
    return ORBHIP_OK;
}

// a new batch: rotate the output buffers and make the main stream wait for the matcher that still reads the buffer about to be overwritten
orbhip_status begin_batch(orbhip_ctx* c, const uint8_t* d_img0, long long frame_stride, int row_stride)
{
    HIPCHK(hipSetDevice(c->cfg.device));
    c->cur = (c->cur + 1) % 3;
    const int cur = c->cur;
    c->last_img0 = d_img0; c->last_img0_fstride = frame_stride; c->last_img0_pitch = row_stride; c->d_last_uright = nullptr; c->last_n_valid = false; c->fgrid_valid = false; c->rrows_valid = false;
    // the buffer about to be overwritten was the "previous frame" of the matcher launched two calls ago
    for (int k = 0; k < 3; k++) if (c->match_pending[k] && (k == (cur + 1) % 3)) { HIPCHK(hipStreamWaitEvent(c->stream, c->ev_match[k], 0)); c->match_pending[k] = false; }
    // ... or may still be downloading (a submitted batch that has not been collected while un-ticketed calls rotate the buffers)
    for (auto& hs : c->sets) if (hs.busy && hs.out_buf == cur && hs.nchunks > 0) HIPCHK(hipStreamWaitEvent(c->stream, hs.ev_d2h[hs.nchunks - 1], 0));
    return ORBHIP_OK;
}

orbhip_status run_pipeline(orbhip_ctx* c, int nimg, const uint8_t* d_img0, long long frame_stride, int row_stride,
                           int match_prev, int window, float nnratio, int check_ori)
{
    orbhip_status st = begin_batch(c, d_img0, frame_stride, row_stride); if (st != ORBHIP_OK) return st;
    const int cur = c->cur, prev = (cur + 2) % 3;
    // camera slots are independent: optionally split the batch into groups, one HIP stream each
    const int ngroups = std::min((int)c->xstreams.size() + 1, nimg);
    ExtractParams P = make_params(c, d_img0, frame_stride, row_stride);
    if (ngroups > 1) { HIPCHK(hipEventRecord(c->ev_fork, c->stream)); }
    for (int gi = 0; gi < ngroups; gi++) {
        const int f0 = (int)((long long)nimg * gi / ngroups), f1 = (int)((long long)nimg * (gi + 1) / ngroups), nf = f1 - f0;
        hipStream_t s = gi == 0 ? c->stream : c->xstreams[gi - 1];
        if (gi > 0) HIPCHK(hipStreamWaitEvent(s, c->ev_fork, 0));
        if (nf <= 0) continue;
        st = pipeline_frames(c, P, f0, nf, s, ngroups == 1); if (st != ORBHIP_OK) return st;
        if (gi > 0) { HIPCHK(hipEventRecord(c->xevents[gi - 1], s)); HIPCHK(hipStreamWaitEvent(c->stream, c->xevents[gi - 1], 0)); }
    }
    if (match_prev) {
        MatchParams M; memset(&M, 0, sizeof M);
        // the matcher reads mvKeysUn of both frames (ORBmatcher.cc:418, 443 via GetFeaturesInArea)
        M.kp1 = c->distorted ? c->d_out_kpun[prev] : c->d_out_kp[prev]; M.desc1 = c->d_out_desc[prev]; M.n1 = c->d_out_n[prev]; M.n1_lvl0 = c->d_lvl_n[prev];
        M.kp2 = c->distorted ? c->d_out_kpun[cur] : c->d_out_kp[cur]; M.desc2 = c->d_out_desc[cur]; M.n2 = c->d_out_n[cur];
        M.lvl_stride = c->L; M.list1 = nullptr; M.prev_from_kp1 = 1;
        M.cap = c->out_cap; M.min_x = c->bounds.min_x; M.min_y = c->bounds.min_y; M.max_x = c->bounds.max_x; M.max_y = c->bounds.max_y;
        M.grid_start = c->d_grid_start; M.grid_items = c->d_grid_items; M.grid_xy = c->d_grid_xy; M.cand = c->d_cand; M.top = c->d_top; M.ncand = c->d_ncand; M.cand_stride = c->lvl0_cap; M.lvl0_cap = c->lvl0_cap; M.tab_cap = c->lvl0_cap;      // (level 0 of a frame holds at most lvl0_cap key points)
        M.prev = c->d_prev; M.matches12 = c->d_m12; M.nmatches = c->d_nm; M.window = window; M.nnratio = nnratio; M.check_ori = check_ori; M.slot0 = 0;
        if (orbhip_match_select_big(c->lvl0_cap, c->lvl0_cap)) {     // level-0 key points beyond what LDS holds: the select kernel's tables in device memory, [slot][...], allocated at the first matched call
            if (!c->d_match_ws) HIPCHK(dalloc(&c->d_match_ws, (size_t)c->B * orbhip_match_select_ints(c->lvl0_cap, c->lvl0_cap)));
            M.big_ws = c->d_match_ws;
        }
        // matcher of this batch on its own stream: latency-bound (one wave per slot), overlaps the next call's extraction
        hipStream_t ms = c->serial ? c->stream : c->mstream;
        HIPCHK(hipEventRecord(c->ev_extract, c->stream));
        HIPCHK(hipStreamWaitEvent(ms, c->ev_extract, 0));
        { ProfScope ps(c, K_MGRID, ms); orbhip_launch_match_grid(M, nimg, ms); }
        { ProfScope ps(c, K_MCAND, ms); orbhip_launch_match_candidates(M, nimg, ms); }
        { ProfScope ps(c, K_MSELECT, ms); orbhip_launch_match_select(M, nimg, ms); }
        HIPCHK(hipEventRecord(c->ev_match[cur], ms));
        c->match_pending[cur] = true;
    }
    c->last_matched = match_prev != 0;
    c->last_nimg = nimg;
    HIPCHK(hipGetLastError());
    return ORBHIP_OK;
}

extern "C" orbhip_status orbhip_extract_device(orbhip_ctx* c, int nimg, const uint8_t* d_imgs, size_t frame_stride, int row_stride,
                                               int match_prev, int window, float nnratio, int check_ori)
{
    if (!c || !d_imgs) return fail(ORBHIP_ERR_INVALID, "null argument");
    if (nimg < 1 || nimg > c->B) return fail(ORBHIP_ERR_INVALID, "nimg %d outside 1..%d", nimg, c->B);
    if (row_stride < c->cfg.width) return fail(ORBHIP_ERR_INVALID, "row stride %d < width %d", row_stride, c->cfg.width);
    c->last_from_host = false;
    return run_pipeline(c, nimg, d_imgs, (long long)frame_stride, row_stride, match_prev, window, nnratio, check_ori);
}

void orbhip_internal_outputs(orbhip_ctx* c, const uint8_t** d_desc, const int** d_n, int* cap, int* last_nimg, int* device, hipStream_t* s)
{   // where the last extraction left its descriptors (orbhip_bow.hip reads them in place)
    *d_desc = c->d_out_desc[c->cur]; *d_n = c->d_out_n[c->cur]; *cap = c->out_cap; *last_nimg = c->last_nimg; *device = c->cfg.device; *s = c->stream;
}

extern "C" orbhip_status orbhip_sync(orbhip_ctx* c)
{
    if (!c) return fail(ORBHIP_ERR_INVALID, "null context");
    HIPCHK(hipSetDevice(c->cfg.device));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (auto xs : c->xstreams) HIPCHK(hipStreamSynchronize(xs));
    if (c->mstream) HIPCHK(hipStreamSynchronize(c->mstream));
    if (c->bstream) HIPCHK(hipStreamSynchronize(c->bstream));
    if (c->bstream_host) HIPCHK(hipStreamSynchronize(c->bstream_host));
    if (c->hstream) HIPCHK(hipStreamSynchronize(c->hstream));
    if (c->dstream) HIPCHK(hipStreamSynchronize(c->dstream));
    prof_collect(c);
    return ORBHIP_OK;
}

orbhip_status ensure_host_staging(orbhip_ctx* c, bool input)
{
    const size_t B = (size_t)c->B;
    if (!c->h_n) {
        HIPCHK(hipHostMalloc((void**)&c->h_block, c->out_block_bytes, hipHostMallocDefault));
        c->h_n = reinterpret_cast<int*>(c->h_block); c->h_kp = reinterpret_cast<orbhip_keypoint*>(c->h_block + c->out_off_kp); c->h_desc = c->h_block + c->out_off_desc;
    }
    if (input && !c->d_in) {
        c->in_pitch = c->geom[0].pitch;
        const size_t bytes = B * (size_t)c->in_pitch * c->cfg.height + 256;
        HIPCHK(orbhip_dmalloc((void**)&c->d_in, bytes));
        HIPCHK(hipHostMalloc((void**)&c->h_in, bytes, hipHostMallocDefault));
    }
    return ORBHIP_OK;
}

// The un-ticketed host entry points (orbhip_fetch*, the colour / rectify batch calls, the stereo calls) download into the context's OWN pinned
// mirrors - which are also staging set 0 of the ticketed path: while a submitted batch is still in flight they would overwrite (or read) what
// its collect is about to deliver.  They refuse instead, like orbhip_extract_batch does.
orbhip_status mirrors_free(const orbhip_ctx* c, const char* who)
{
    if (c->oldest_ticket != c->next_ticket) return fail(ORBHIP_ERR_INVALID, "%s with %d submitted batch(es) still in flight: collect them first", who, c->next_ticket - c->oldest_ticket);
    return ORBHIP_OK;
}
static orbhip_status enqueue_fetch(orbhip_ctx* c, int nimg, bool want_kp, bool want_desc)
{   // bulk device-to-host copies into the pinned mirrors, ordered after the extraction on the context's stream
    { const orbhip_status st = mirrors_free(c, "a fetch into the context's mirrors"); if (st != ORBHIP_OK) return st; }
    // (orbhip_copy_async: a kernel for a few frames' worth, the DMA engines beyond 2 MB)
    HIPCHK(orbhip_copy_async(c->h_n, c->d_out_n[c->cur], nimg * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (want_kp) HIPCHK(orbhip_copy_async(c->h_kp, c->d_out_kp[c->cur], (size_t)nimg * c->out_cap * sizeof(orbhip_keypoint), hipMemcpyDeviceToHost, c->stream));
    if (want_desc) HIPCHK(orbhip_copy_async(c->h_desc, c->d_out_desc[c->cur], (size_t)nimg * c->out_cap * 32, hipMemcpyDeviceToHost, c->stream));
    return ORBHIP_OK;
}
static orbhip_status finish_fetch(orbhip_ctx* c, int nimg, orbhip_keypoint* kps, uint8_t* desc, int cap, int* n_out)
{
    bool overflow = false;
    c->last_n.assign(c->h_n, c->h_n + nimg); c->last_n_valid = nimg == c->last_nimg;
    for (int f = 0; f < nimg; f++) {
        const int n = c->h_n[f];
        n_out[f] = n;
        const int m = std::min(n, cap);
        if (n > cap) overflow = true;
        if (m > 0 && kps) memcpy(kps + (size_t)f * cap, c->h_kp + (size_t)f * c->out_cap, (size_t)m * sizeof(orbhip_keypoint));
        if (m > 0 && desc) memcpy(desc + (size_t)f * cap * 32, c->h_desc + (size_t)f * c->out_cap * 32, (size_t)m * 32);
    }
    return overflow ? fail(ORBHIP_ERR_CAPACITY, "keypoint buffer too small") : ORBHIP_OK;
}

extern "C" orbhip_status orbhip_fetch(orbhip_ctx* c, int nimg, orbhip_keypoint* kps, uint8_t* desc, int cap, int* n_out)
{
    if (!c || !n_out) return fail(ORBHIP_ERR_INVALID, "null argument");
    if (nimg < 1 || nimg > c->last_nimg) return fail(ORBHIP_ERR_INVALID, "nimg %d but the last call processed %d frames", nimg, c->last_nimg);
    HIPCHK(hipSetDevice(c->cfg.device));
    orbhip_status st = ensure_host_staging(c, false); if (st != ORBHIP_OK) return st;
    st = enqueue_fetch(c, nimg, kps != nullptr, desc != nullptr); if (st != ORBHIP_OK) return st;
    st = orbhip_sync(c); if (st != ORBHIP_OK) return st;
    return finish_fetch(c, nimg, kps, desc, cap, n_out);
}

extern "C" orbhip_status orbhip_fetch_matches(orbhip_ctx* c, int nimg, int32_t* matches12, int cap1, int32_t* n1_out, int32_t* nmatches)
{
    if (!c) return fail(ORBHIP_ERR_INVALID, "null context");
    if (!c->last_matched) return fail(ORBHIP_ERR_INVALID, "the last call did not run the matcher");
    if (nimg < 1 || nimg > c->last_nimg) return fail(ORBHIP_ERR_INVALID, "bad nimg");
    orbhip_status st = orbhip_sync(c); if (st != ORBHIP_OK) return st;
    std::vector<int> n1(nimg);
    HIPCHK(hipMemcpy(n1.data(), c->d_out_n[(c->cur + 2) % 3], nimg * sizeof(int), hipMemcpyDeviceToHost));
    if (nmatches) HIPCHK(hipMemcpy(nmatches, c->d_nm, nimg * sizeof(int), hipMemcpyDeviceToHost));
    for (int f = 0; f < nimg; f++) {
        if (n1_out) n1_out[f] = n1[f];
        const int m = std::min(n1[f], cap1);
        if (m > 0 && matches12) HIPCHK(hipMemcpy(matches12 + (size_t)f * cap1, c->d_m12 + (size_t)f * c->out_cap, (size_t)m * sizeof(int), hipMemcpyDeviceToHost));
    }
    return ORBHIP_OK;
}

// ---------------------------------------------------------------------------------------------- measurement
extern "C" orbhip_status orbhip_profile_enable(orbhip_ctx* c, int on) { if (!c) return fail(ORBHIP_ERR_INVALID, "null context"); c->prof = on != 0; return ORBHIP_OK; }
extern "C" int orbhip_profile_num_kernels(const orbhip_ctx*) { return K_COUNT; }
extern "C" orbhip_status orbhip_profile_get(orbhip_ctx* c, int k, const char** name, double* total_ms, int64_t* launches)
{
    if (!c || k < 0 || k >= K_COUNT) return fail(ORBHIP_ERR_INVALID, "bad kernel index");
    prof_collect(c);
    if (name) *name = kKernelNames[k]; if (total_ms) *total_ms = c->tot_ms[k]; if (launches) *launches = c->launches[k];
    return ORBHIP_OK;
}
extern "C" orbhip_status orbhip_profile_reset(orbhip_ctx* c)
{
    if (!c) return fail(ORBHIP_ERR_INVALID, "null context");
    prof_collect(c);
    for (int k = 0; k < K_COUNT; k++) { c->tot_ms[k] = 0; c->launches[k] = 0; }
    return ORBHIP_OK;
}
extern "C" int64_t orbhip_algorithmic_bytes_per_frame(const orbhip_ctx* c)
{   // B(W,H,N) = P0 + (SP-P0) + (SP-P7) + SP + 2*SP + N*(749+512) + N*(28+32)      
    if (!c) return 0;
    long long SP = 0; for (auto& g : c->geom) SP += (long long)g.w * g.h;
    const long long P0 = (long long)c->geom[0].w * c->geom[0].h, PL = (long long)c->geom[c->L - 1].w * c->geom[c->L - 1].h, N = c->cfg.nfeatures;
    return P0 + (SP - P0) + (SP - PL) + SP + 2 * SP + N * (749 + 512) + N * (28 + 32);
}
extern "C" int64_t orbhip_algorithmic_bytes_per_frame_kernel(const orbhip_ctx* c, int k)
{   // the terms of B(W,H,N) attributed to the kernel that moves them
    if (!c) return 0;
    long long SP = 0; for (auto& g : c->geom) SP += (long long)g.w * g.h;
    const long long P0 = (long long)c->geom[0].w * c->geom[0].h, PL = (long long)c->geom[c->L - 1].w * c->geom[c->L - 1].h, N = c->cfg.nfeatures;
    switch (k) {
        case K_PYRAMID: return (SP - PL) + (SP - P0);
        case K_FAST: return SP;
        case K_BLUR: return 2 * SP;
        case K_DESCRIBE: return N * (749 + 512) + N * (28 + 32);
        default: return 0;
    }
}
