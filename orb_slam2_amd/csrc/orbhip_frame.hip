// orbhip_frame.hip — host side of what ORB_SLAM2's Frame does with an extraction's results in liborbhip.so: stereo matching and camera geometry
// (undistortion, RGB-D, rectification maps).  Kernels: orbhip_kernels_stereo.hip, orbhip_kernels_geom.hip.
#include "orbhip_ctx.h"

// ---------------------------------------------------------------------------------------------- stereo
// k_stereo_rows drops items beyond this bound (`if (p < T.row_cap)`); none exists: a key point enters ceil(y+r) - floor(y-r) + 1 < 2r + 3 <= ceil(4*sf[L-1]) + 3 rows, a frame has at most out_cap
int stereo_row_cap(const orbhip_ctx* c) { return c->out_cap * ((int)ceilf(4.0f * c->sf[c->L - 1]) + 3); }      // rows [floor(y-r), ceil(y+r)], r = 2*scale
StereoSide stereo_side(orbhip_ctx* c)
{
    StereoSide S; memset(&S, 0, sizeof S);
    S.kp = c->d_out_kp[c->cur]; S.desc = c->d_out_desc[c->cur]; S.n = c->d_out_n[c->cur];
    S.img0 = c->last_img0; S.img0_frame_stride = c->last_img0_fstride; S.img0_pitch = c->last_img0_pitch;
    S.pyr = c->d_pyr; S.plane_frame_bytes = c->plane_frame_bytes;
    return S;
}

extern "C" orbhip_status orbhip_compute_stereo_matches(orbhip_ctx* l, orbhip_ctx* r, int nimg, float mbf, float mb, float* u_right, float* depth, int cap)
{
    OrbApiTimer api_timer;
    if (!l || !r || !u_right || !depth) return fail(ORBHIP_ERR_INVALID, "null argument");
    if (l->cfg.device != r->cfg.device || l->cfg.width != r->cfg.width || l->cfg.height != r->cfg.height || l->L != r->L ||
        l->cfg.scale_factor != r->cfg.scale_factor || l->out_cap != r->out_cap)
        return fail(ORBHIP_ERR_INVALID, "left and right contexts must share device, image size, levels and scale factor");
    if (nimg < 1 || nimg > l->last_nimg || nimg > r->last_nimg) return fail(ORBHIP_ERR_INVALID, "nimg %d but the last calls processed %d / %d frames", nimg, l->last_nimg, r->last_nimg);
    if (!(mb > 0) || !(mbf > 0)) return fail(ORBHIP_ERR_INVALID, "mbf and mb must be positive");
    if (l->out_cap >= 65536) return fail(ORBHIP_ERR_UNSUPPORTED, "too many keypoints per frame for the stereo matcher");
    HIPCHK(hipSetDevice(l->cfg.device));
    // the right frame's results must be complete (left work is stream-ordered): they are if its caller already holds them
    orbhip_status st = ORBHIP_OK;
    if (!r->last_n_valid) { st = orbhip_sync(r); if (st != ORBHIP_OK) return st; }
    const size_t B = (size_t)l->B;
    if (!l->d_st_rowstart) {
        l->st_rowcap = stereo_row_cap(l);
        hipError_t e = hipSuccess;
        if (e == hipSuccess) e = dalloc(&l->d_st_rowstart, B * (l->cfg.height + 1));
        if (e == hipSuccess) e = dalloc(&l->d_st_rowitems, B * (size_t)l->st_rowcap);
        if (e == hipSuccess) e = dalloc(&l->d_st_u, 2 * B * l->out_cap);           // [mvuRight | mvDepth]: one allocation, one download when the call fills the context
        if (e == hipSuccess) l->d_st_depth = l->d_st_u + B * l->out_cap;
        if (e == hipSuccess) e = dalloc(&l->d_st_sad, B * l->out_cap);
        if (e != hipSuccess) return fail(ORBHIP_ERR_HIP, "stereo workspace allocation failed: %s", hipGetErrorString(e));
    }
    StereoParams T; memset(&T, 0, sizeof T);
    T.geom = l->d_geom; T.L = stereo_side(l); T.R = stereo_side(r);
    T.cap = l->out_cap; T.im_h = l->cfg.height;
    T.row_start = l->d_st_rowstart; T.row_items = l->d_st_rowitems; T.row_cap = l->st_rowcap;
    // the right context built its frame's row table behind its own extraction (frame epilogue): take it; from now on it always will
    const bool rows_ready = nimg == 1 && r->rrows_valid && r->rrows_cur == r->cur;
    if (rows_ready) { T.row_start = r->d_rrow_start; T.row_items = r->d_rrow_items; T.row_cap = r->rrow_cap; HIPCHK(hipStreamWaitEvent(l->stream, r->ev_epilogue, 0)); }
    if (nimg == 1) r->want_rrows = true;
    T.u_right = l->d_st_u; T.depth = l->d_st_depth; T.sad = l->d_st_sad; l->d_last_uright = l->d_st_u;
    T.mbf = mbf; T.maxD = mbf / mb;                                                 // minZ = mb, maxD = mbf/minZ (Frame.cc:496-498)
    orbhip_launch_stereo(T, nimg, l->out_cap, l->stream, rows_ready);
    HIPCHK(hipGetLastError());
    st = ensure_host_staging(l, false); if (st != ORBHIP_OK) return st;
    { const orbhip_status stf = mirrors_free(l, "orbhip_compute_stereo_matches"); if (stf != ORBHIP_OK) return stf; }
    const bool know_n = l->last_n_valid && (int)l->last_n.size() >= nimg;
    if (!know_n) HIPCHK(hipMemcpyAsync(l->h_n, l->d_out_n[l->cur], nimg * sizeof(int), hipMemcpyDeviceToHost, l->stream));
    float* hu = reinterpret_cast<float*>(l->h_kp); float* hd = hu + (size_t)nimg * l->out_cap;       // pinned mirror reused (28 B/keypoint >= 8 B)
    if ((size_t)nimg == B) HIPCHK(orbhip_copy_async(hu, l->d_st_u, 2 * B * l->out_cap * sizeof(float), hipMemcpyDeviceToHost, l->stream));
    else {
        HIPCHK(hipMemcpyAsync(hu, l->d_st_u, (size_t)nimg * l->out_cap * sizeof(float), hipMemcpyDeviceToHost, l->stream));
        HIPCHK(hipMemcpyAsync(hd, l->d_st_depth, (size_t)nimg * l->out_cap * sizeof(float), hipMemcpyDeviceToHost, l->stream));
    }
    HIPCHK(hipStreamSynchronize(l->stream));
    if (l->prof) prof_collect(l);
    for (int f = 0; f < nimg; f++) {
        const int m = std::min(know_n ? l->last_n[f] : l->h_n[f], cap);
        for (int i = 0; i < cap; i++) { u_right[(size_t)f * cap + i] = -1.0f; depth[(size_t)f * cap + i] = -1.0f; }
        if (m > 0) { memcpy(u_right + (size_t)f * cap, hu + (size_t)f * l->out_cap, m * sizeof(float)); memcpy(depth + (size_t)f * cap, hd + (size_t)f * l->out_cap, m * sizeof(float)); }
    }
    return ORBHIP_OK;
}

// The stereo pair as ONE call (include/orbhip.h): both images through one context with two camera slots - one staging copy + upload, one launch
// chain for both frames, the stereo matcher (slot 0 against slot 1) and the frame's feature grid queued behind it on the same stream; the host copies
// the key points out while the stereo kernels run, then picks up mvuRight / mvDepth.
extern "C" orbhip_status orbhip_extract_stereo(orbhip_ctx* c, const uint8_t* img_left, const uint8_t* img_right, int stride, orbhip_keypoint* kps, uint8_t* desc, int cap, int* n_out,
                                               float mbf, float mb, float* u_right, float* depth)
{
    OrbApiTimer api_timer;
    if (!c || !n_out || !u_right || !depth || cap < 0) return fail(ORBHIP_ERR_INVALID, "null argument");
    if (c->B < 2) return fail(ORBHIP_ERR_INVALID, "orbhip_extract_stereo needs a context with max_batch >= 2 (this one has %d)", c->B);
    if (!(mb > 0) || !(mbf > 0)) return fail(ORBHIP_ERR_INVALID, "mbf and mb must be positive");
    if (c->out_cap >= 65536) return fail(ORBHIP_ERR_UNSUPPORTED, "too many keypoints per frame for the stereo matcher");
    n_out[0] = n_out[1] = 0;
    for (int i = 0; i < cap; i++) { u_right[i] = -1.0f; depth[i] = -1.0f; }
    if (!img_left || !img_right) return ORBHIP_OK;                      // an empty image: the reference's operator() returns silently, the frame has no features
    if (c->oldest_ticket != c->next_ticket) return fail(ORBHIP_ERR_INVALID, "orbhip_extract_stereo with %d submitted batches still in flight: collect them first", c->next_ticket - c->oldest_ticket);
    HIPCHK(hipSetDevice(c->cfg.device));
    const size_t B = (size_t)c->B, oc = (size_t)c->out_cap;
    if (!c->d_st_rowstart) {
        c->st_rowcap = stereo_row_cap(c);
        hipError_t e = hipSuccess;
        if (e == hipSuccess) e = dalloc(&c->d_st_rowstart, B * (c->cfg.height + 1));
        if (e == hipSuccess) e = dalloc(&c->d_st_rowitems, B * (size_t)c->st_rowcap);
        if (e == hipSuccess) e = dalloc(&c->d_st_u, 2 * B * oc);
        if (e == hipSuccess) c->d_st_depth = c->d_st_u + B * oc;
        if (e == hipSuccess) e = dalloc(&c->d_st_sad, B * oc);
        if (e != hipSuccess) return fail(ORBHIP_ERR_HIP, "stereo workspace allocation failed: %s", hipGetErrorString(e));
    }
    if (!c->h_st) HIPCHK(hipHostMalloc((void**)&c->h_st, (B + 1) * oc * sizeof(float), hipHostMallocDefault));
    const uint8_t* imgs[2] = {img_left, img_right};
    int ticket = -1;
    orbhip_status st = submit_impl(c, 2, imgs, stride, nullptr, nullptr, 0, &ticket); if (st != ORBHIP_OK) return st;
    c->pair_mode = true;
    // slot 0 against slot 1 of this context
    StereoParams T; memset(&T, 0, sizeof T);
    T.geom = c->d_geom; T.L = stereo_side(c); T.R = stereo_side(c);
    T.R.kp += oc; T.R.desc += oc * 32; T.R.n += 1; T.R.img0 += T.R.img0_frame_stride; T.R.pyr += T.R.plane_frame_bytes;
    T.cap = c->out_cap; T.im_h = c->cfg.height; T.row_start = c->d_st_rowstart; T.row_items = c->d_st_rowitems; T.row_cap = c->st_rowcap;
    T.u_right = c->d_st_u; T.depth = c->d_st_depth; T.sad = c->d_st_sad; c->d_last_uright = c->d_st_u;
    T.mbf = mbf; T.maxD = mbf / mb;
    orbhip_launch_stereo(T, 1, c->out_cap, c->stream, false);
    hipError_t e = hipGetLastError();
    // [mvuRight of slot 0 .. mvDepth of slot 0]: ONE copy of (B + 1) * out_cap floats (slot 1's unused mvuRight rides along), then an event: the host waits for
    // that, not for the stream - the frame's feature grid (an epilogue of the searches to come, 20 us) is queued behind it and is nobody's business yet
    if (!c->ev_stereo) { if (hipEventCreateWithFlags(&c->ev_stereo, hipEventDisableTiming) != hipSuccess) e = hipErrorOutOfMemory; }
    if (e == hipSuccess) e = orbhip_copy_async(c->h_st, c->d_st_u, (B + 1) * oc * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipEventRecord(c->ev_stereo, c->stream);
    if (e == hipSuccess && c->want_fgrid) { const bool rr = c->want_rrows; c->want_rrows = false; const orbhip_status se = frame_epilogues(c, c->stream); c->want_rrows = rr; if (se != ORBHIP_OK) e = hipErrorInvalidValue; }
    // key points + descriptors of both images (waits for the result block only: the stereo kernels are still running)
    st = collect_flat(c, ticket, kps, desc, cap, n_out);
    const hipError_t es = e == hipSuccess ? hipEventSynchronize(c->ev_stereo) : hipStreamSynchronize(c->stream);
    if (c->prof) prof_collect(c);
    if (e != hipSuccess || es != hipSuccess) return fail(ORBHIP_ERR_HIP, "extract_stereo: %s", hipGetErrorString(e != hipSuccess ? e : es));
    if (st != ORBHIP_OK && st != ORBHIP_ERR_CAPACITY) return st;
    const int m = std::min(n_out[0], cap);
    if (m > 0) { memcpy(u_right, c->h_st, (size_t)m * sizeof(float)); memcpy(depth, c->h_st + B * oc, (size_t)m * sizeof(float)); }
    return st;
}

// ---------------------------------------------------------------------------------------------- camera geometry
static bool camera_ok(const orbhip_camera* cam) { return cam && cam->fx != 0.0f && cam->fy != 0.0f; }
static CameraD widen(const orbhip_camera& k)
{   // cvUndistortPoints converts the CV_32F mK / mDistCoef to double and forms ifx = 1./fx on the host
    CameraD C; C.fx = k.fx; C.fy = k.fy; C.cx = k.cx; C.cy = k.cy; C.ifx = 1. / C.fx; C.ify = 1. / C.fy; C.k1 = k.k1; C.k2 = k.k2; C.p1 = k.p1; C.p2 = k.p2; C.k3 = k.k3;
    return C;
}
extern "C" orbhip_status orbhip_undistort_points(int device, const orbhip_camera* cam, const float* xy, int n, float* xy_out)
{
    OrbApiTimer api_timer;
    if (!camera_ok(cam) || n < 0 || (n > 0 && (!xy || !xy_out))) return fail(ORBHIP_ERR_INVALID, "bad argument");
    if (n == 0) return ORBHIP_OK;
    if (!device_present()) return fail(ORBHIP_ERR_HIP, "no HIP device available: no CPU fallback");
    HIPCHK(hipSetDevice(device));
    hipStream_t ts = orbhip_thread_stream(device);
    float *din = nullptr, *dout = nullptr;
    HIPCHK(arena_layout(device, [&](Arena& A) { A.take(&din, (size_t)n * 2); A.take(&dout, (size_t)n * 2); }));
    HIPCHK(hipMemcpyAsync(din, xy, (size_t)n * 2 * sizeof(float), hipMemcpyHostToDevice, ts));
    orbhip_launch_undistort_points(widen(*cam), din, n, dout, ts);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(xy_out, dout, (size_t)n * 2 * sizeof(float), hipMemcpyDeviceToHost, ts));
    HIPCHK(hipStreamSynchronize(ts));
    return ORBHIP_OK;
}
extern "C" orbhip_status orbhip_image_bounds(int device, const orbhip_camera* cam, int im_w, int im_h, orbhip_bounds* out)
{
    OrbApiTimer api_timer;
    if (!camera_ok(cam) || !out || im_w < 1 || im_h < 1) return fail(ORBHIP_ERR_INVALID, "bad argument");
    if (cam->k1 == 0.0f) { out->min_x = 0.0f; out->max_x = (float)im_w; out->min_y = 0.0f; out->max_y = (float)im_h; return ORBHIP_OK; }     // Frame.cc:455-463
    const float corners[8] = {0.0f, 0.0f, (float)im_w, 0.0f, 0.0f, (float)im_h, (float)im_w, (float)im_h};                                 // Frame.cc:440-444
    float m[8];
    const orbhip_status st = orbhip_undistort_points(device, cam, corners, 4, m); if (st != ORBHIP_OK) return st;
    out->min_x = std::min(m[0], m[4]); out->max_x = std::max(m[2], m[6]); out->min_y = std::min(m[1], m[3]); out->max_y = std::max(m[5], m[7]);   // Frame.cc:451-454
    return ORBHIP_OK;
}
extern "C" orbhip_status orbhip_set_camera(orbhip_ctx* c, const orbhip_camera* cam)
{
    if (!c || (cam && !camera_ok(cam))) return fail(ORBHIP_ERR_INVALID, "bad argument");
    orbhip_status st = orbhip_sync(c); if (st != ORBHIP_OK) return st;
    const bool distorted = cam && cam->k1 != 0.0f;                        // if(mDistCoef.at<float>(0)==0.0) mvKeysUn = mvKeys  (Frame.cc:406-410)
    orbhip_bounds b = {0.0f, 0.0f, (float)c->cfg.width, (float)c->cfg.height};
    if (distorted) {
        st = orbhip_image_bounds(c->cfg.device, cam, c->cfg.width, c->cfg.height, &b); if (st != ORBHIP_OK) return st;
        if (!(b.max_x > b.min_x) || !(b.max_y > b.min_y)) return fail(ORBHIP_ERR_INVALID, "the distortion model folds the image corners (bounds %g..%g x %g..%g)", b.min_x, b.max_x, b.min_y, b.max_y);
        for (int k = 0; k < 3; k++) if (!c->d_out_kpun[k]) HIPCHK(dalloc(&c->d_out_kpun[k], (size_t)c->B * c->out_cap));
        c->cam = widen(*cam);
    }
    c->distorted = distorted; c->bounds = b;
    // frames extracted under the previous camera are no "previous frame" for the matcher any more
    for (int k = 0; k < 3; k++) { HIPCHK(hipMemsetAsync(c->d_out_n[k], 0, (size_t)c->B * sizeof(int), c->stream)); HIPCHK(hipMemsetAsync(c->d_lvl_n[k], 0, (size_t)c->B * c->L * sizeof(int), c->stream)); }
    c->last_nimg = 0; c->last_matched = false;
    return orbhip_sync(c);
}
extern "C" orbhip_status orbhip_get_bounds(const orbhip_ctx* c, orbhip_bounds* out)
{
    if (!c || !out) return fail(ORBHIP_ERR_INVALID, "null argument");
    *out = c->bounds; return ORBHIP_OK;
}
extern "C" orbhip_status orbhip_fetch_undistorted(orbhip_ctx* c, int nimg, orbhip_keypoint* kps_un, int cap)
{
    OrbApiTimer api_timer;
    if (!c || !kps_un || cap < 0) return fail(ORBHIP_ERR_INVALID, "bad argument");
    if (nimg < 1 || nimg > c->last_nimg) return fail(ORBHIP_ERR_INVALID, "nimg %d but the last call processed %d frames", nimg, c->last_nimg);
    HIPCHK(hipSetDevice(c->cfg.device));
    orbhip_status st = ensure_host_staging(c, false); if (st != ORBHIP_OK) return st;
    if (!c->h_kpun) HIPCHK(hipHostMalloc((void**)&c->h_kpun, (size_t)c->B * c->out_cap * sizeof(orbhip_keypoint), hipHostMallocDefault));
    { const orbhip_status stf = mirrors_free(c, "orbhip_fetch_undistorted"); if (stf != ORBHIP_OK) return stf; }
    HIPCHK(orbhip_copy_async(c->h_n, c->d_out_n[c->cur], nimg * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(orbhip_copy_async(c->h_kpun, (c->distorted ? c->d_out_kpun : c->d_out_kp)[c->cur], (size_t)nimg * c->out_cap * sizeof(orbhip_keypoint), hipMemcpyDeviceToHost, c->stream));
    st = orbhip_sync(c); if (st != ORBHIP_OK) return st;
    bool overflow = false;
    for (int f = 0; f < nimg; f++) {
        const int m = std::min(c->h_n[f], cap);
        if (c->h_n[f] > cap) overflow = true;
        if (m > 0) memcpy(kps_un + (size_t)f * cap, c->h_kpun + (size_t)f * c->out_cap, (size_t)m * sizeof(orbhip_keypoint));
    }
    return overflow ? fail(ORBHIP_ERR_CAPACITY, "keypoint buffer too small") : ORBHIP_OK;
}

// Frame::ComputeStereoFromRGBD (Frame.cc:643-665) on the key points the last extraction left in HBM
extern "C" orbhip_status orbhip_compute_stereo_from_rgbd(orbhip_ctx* c, int nimg, const void* const* depth_maps, int stride_bytes, int depth_type, float depth_factor,
                                                         float mbf, float* u_right, float* depth, int cap)
{
    OrbApiTimer api_timer;
    if (!c || !depth_maps || !u_right || !depth || cap < 0 || (depth_type != 0 && depth_type != 1)) return fail(ORBHIP_ERR_INVALID, "bad argument");
    if (nimg < 1 || nimg > c->last_nimg) return fail(ORBHIP_ERR_INVALID, "nimg %d but the last call processed %d frames", nimg, c->last_nimg);
    const int esz = depth_type == 0 ? 4 : 2, W = c->cfg.width, H = c->cfg.height;
    if (stride_bytes < W * esz) return fail(ORBHIP_ERR_INVALID, "depth row stride %d < %d", stride_bytes, W * esz);
    HIPCHK(hipSetDevice(c->cfg.device));
    const size_t pitch = ((size_t)W * 4 + 63) & ~(size_t)63, fbytes = pitch * H, need = (size_t)c->B * fbytes + (size_t)2 * c->B * c->out_cap * sizeof(float);
    if (c->depth_bytes < need) { if (c->d_depth) (void)hipFree(c->d_depth); c->d_depth = nullptr; c->depth_bytes = 0; HIPCHK(orbhip_dmalloc((void**)&c->d_depth, need)); c->depth_bytes = need; }
    float* d_u = (float*)(c->d_depth + (size_t)c->B * fbytes); float* d_z = d_u + (size_t)c->B * c->out_cap; c->d_last_uright = d_u;
    for (int f = 0; f < nimg; f++) {
        if (!depth_maps[f]) return fail(ORBHIP_ERR_INVALID, "depth map %d is null", f);
        HIPCHK(hipMemcpy2DAsync(c->d_depth + f * fbytes, pitch, depth_maps[f], (size_t)stride_bytes, (size_t)W * esz, H, hipMemcpyHostToDevice, c->stream));
    }
    const int convert = (std::fabs(depth_factor - 1.0f) > 1e-5f) || depth_type != 0;          // Tracking.cc:226
    orbhip_launch_stereo_from_rgbd(c->d_out_kp[c->cur], (c->distorted ? c->d_out_kpun : c->d_out_kp)[c->cur], c->d_out_n[c->cur], c->out_cap, c->d_depth, (long long)fbytes,
                                   (int)pitch, depth_type, convert, depth_factor, mbf, d_u, d_z, nimg, c->stream);
    HIPCHK(hipGetLastError());
    orbhip_status st = ensure_host_staging(c, false); if (st != ORBHIP_OK) return st;
    { const orbhip_status stf = mirrors_free(c, "orbhip_compute_stereo_from_rgbd"); if (stf != ORBHIP_OK) return stf; }
    HIPCHK(hipMemcpyAsync(c->h_n, c->d_out_n[c->cur], nimg * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    st = orbhip_sync(c); if (st != ORBHIP_OK) return st;
    for (int f = 0; f < nimg; f++) {
        const int m = std::min(c->h_n[f], cap);
        if (m > 0) {
            HIPCHK(hipMemcpy(u_right + (size_t)f * cap, d_u + (size_t)f * c->out_cap, (size_t)m * sizeof(float), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(depth + (size_t)f * cap, d_z + (size_t)f * c->out_cap, (size_t)m * sizeof(float), hipMemcpyDeviceToHost));
        }
    }
    return ORBHIP_OK;
}

// mvuRight computed by the caller (Frame::ComputeStereoFromRGBD's own loop, Frame.cc:643-665: N samples of a depth map that lives in host memory) handed to
// the frame that is still on the device, so that the resident searches' right-coordinate test (ORBmatcher.cc:1418-1424, 96-101) reads it in HBM: N floats travel,
// not the depth map.  Asynchronous on the context's stream; the values are copied before the call returns.
extern "C" orbhip_status orbhip_set_stereo_columns(orbhip_ctx* c, int frame, const float* u_right, int n)
{
    OrbApiTimer api_timer;
    if (!c || (!u_right && n > 0)) return fail(ORBHIP_ERR_INVALID, "null argument");
    if (frame < 0 || frame >= c->last_nimg) return fail(ORBHIP_ERR_INVALID, "frame %d outside the %d frames of the last extraction", frame, c->last_nimg);
    if (n < 0 || n > c->out_cap) return fail(ORBHIP_ERR_INVALID, "n %d outside 0..%d", n, c->out_cap);
    HIPCHK(hipSetDevice(c->cfg.device));
    const size_t total = (size_t)c->B * c->out_cap;
    if (!c->d_ucols) {
        HIPCHK(orbhip_dmalloc((void**)&c->d_ucols, total * sizeof(float)));
        HIPCHK(hipHostMalloc((void**)&c->h_ucols, total * sizeof(float), hipHostMallocDefault));
        HIPCHK(hipEventCreateWithFlags(&c->ev_ucols, hipEventDisableTiming));
    }
    if (c->ucols_pending) { HIPCHK(hipEventSynchronize(c->ev_ucols)); c->ucols_pending = false; }      // the pinned block is free again
    if (c->d_last_uright != c->d_ucols) {
        // the block becomes the extraction's mvuRight for EVERY frame: the other frames keep the columns a stereo / RGB-D step left for them, or read
        // "no right coordinate" (-1, Frame.cc:468) - never whatever the allocation held
        if (c->d_last_uright) HIPCHK(orbhip_copy_async(c->d_ucols, c->d_last_uright, total * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
        else HIPCHK(hipMemsetD32Async((hipDeviceptr_t)c->d_ucols, 0xBF800000, total, c->stream));
    }
    if (n > 0) {
        memcpy(c->h_ucols + (size_t)frame * c->out_cap, u_right, (size_t)n * sizeof(float));
        HIPCHK(orbhip_copy_async(c->d_ucols + (size_t)frame * c->out_cap, c->h_ucols + (size_t)frame * c->out_cap, (size_t)n * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipEventRecord(c->ev_ucols, c->stream)); c->ucols_pending = true;
    }
    c->d_last_uright = c->d_ucols;
    return ORBHIP_OK;
}

// Rectification of raw stereo frames (stereo_euroc.cc:136-137): remapped on the device into the context's level-0 plane
extern "C" orbhip_status orbhip_set_rectification(orbhip_ctx* c, const float* map_x, const float* map_y, int src_w, int src_h)
{
    if (!c) return fail(ORBHIP_ERR_INVALID, "null context");
    orbhip_status st = orbhip_sync(c); if (st != ORBHIP_OK) return st;
    if (!map_x) { c->src_w = c->src_h = 0; return ORBHIP_OK; }
    if (!map_y || src_w < 1 || src_h < 1 || src_w > 32767 || src_h > 32767) return fail(ORBHIP_ERR_INVALID, "bad argument");
    HIPCHK(hipSetDevice(c->cfg.device));
    const int qp = (c->cfg.width + 3) & ~3;
    const size_t n = (size_t)qp * c->cfg.height;
    if (!c->d_map_x) { HIPCHK(dalloc(&c->d_map_x, n)); HIPCHK(dalloc(&c->d_map_y, n)); }
    // cv::remap converts the float maps to 5 fractional bits for every image (RemapInvoker: cvRound(map * INTER_TAB_SIZE)); the maps of
    // a camera never change, so the table is built here once.  cvRound = cvtss2si: round-half-even, INT_MIN when out of range / NaN.
    std::vector<int> q(2 * n, 0);
    for (int y = 0; y < c->cfg.height; y++)
        for (int x = 0; x < c->cfg.width; x++) {
            const float vx = map_x[(size_t)y * c->cfg.width + x] * 32.0f, vy = map_y[(size_t)y * c->cfg.width + x] * 32.0f;
            q[(size_t)y * qp + x] = std::fabs(vx) < 2147483648.0f ? (int)lrintf(vx) : INT32_MIN;
            q[n + (size_t)y * qp + x] = std::fabs(vy) < 2147483648.0f ? (int)lrintf(vy) : INT32_MIN;
        }
    HIPCHK(hipMemcpy(c->d_map_x, q.data(), n * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->d_map_y, q.data() + n, n * sizeof(int), hipMemcpyHostToDevice));
    if (c->d_raw && (src_w != c->src_w || src_h != c->src_h)) { (void)hipFree(c->d_raw); (void)hipHostFree(c->h_raw); c->d_raw = nullptr; c->h_raw = nullptr; }
    c->src_w = src_w; c->src_h = src_h; c->raw_pitch = (src_w + 63) & ~63;
    return ORBHIP_OK;
}
