// window_gather_probe.hip — what does k_describe's blurred window cost to gather from a plane stored as 32-column x 4-row tiles (one tile =
// one aligned 128-byte line), against today's row-major plane?  Same shape as the window timing of tools/lds_dma_b128_probe.hip: 4096
// workgroups x 4 waves x 200 gathers around random centres of a 1280 x 384 image, every gather waited for before the next.
//   (a) row-major plane, 7 dword LDS-DMA passes over 37 rows x 48 bytes (12-dword LDS rows)          - k_describe today
//   (b) tiled plane, 10 passes of one tile row each (4 image rows x 64 bytes), 64-byte LDS row stride - 2 tile columns, 3 when the window needs them
//   (c) as (b) with every gather forced onto the 3-tile-column span (64 bytes starting 16 bytes into a tile)
// Each form runs on one plane (everything L2-resident) and on 1024 planes (480 MB: nothing stays), three times each.  Before the timing a
// one-workgroup kernel checks that forms (b) and (c) leave the row-major window in LDS that the address function promises.
// Build: hipcc --offload-arch=gfx950 -O2 tools/window_gather_probe.hip -o tools/window_gather_probe
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
typedef const __attribute__((address_space(1))) void* gptr;
typedef __attribute__((address_space(3))) void* lptr;
typedef const __attribute__((address_space(1))) unsigned char* gbytes;
#define W 1280
#define H 384
#define TPR (W / 32)                    // tiles per row
#define PLANE (W * H)
__host__ __device__ inline unsigned tiled_off(unsigned x, unsigned y) { return ((y >> 2) * TPR + (x >> 5)) * 128u + (y & 3u) * 32u + (x & 31u); }
__host__ __device__ inline unsigned char pixel(unsigned x, unsigned y, unsigned f) { return (unsigned char)(x * 37u + y * 11u + (x >> 5) * 5u + (y >> 2) * 3u + f * 7u + 1u); }

__device__ __forceinline__ gbytes uniform_ptr(const unsigned char* p)
{
    const unsigned long long a = (unsigned long long)p;
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)a), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(a >> 32));
    return (gbytes)(((unsigned long long)hi << 32) | lo);
}
// one window into `win` (2560 bytes).  FORM 0: (a); 1: (b); 2: (c).  cx, cy wave-uniform; returns the LDS byte offset of (cx - 18, cy - 18)
template <int FORM> __device__ __forceinline__ unsigned gather(gbytes plane, int cx, int cy, int lane, unsigned* win, const int* wrow, const int* wcol)
{
    if (FORM == 0) {
        const unsigned base = (unsigned)((cy - 18) * W + ((cx - 18) & ~3));
#pragma unroll
        for (int k = 0; k < 7; k++) __builtin_amdgcn_global_load_lds((gptr)(plane + (base + __umul24((unsigned)wrow[k], (unsigned)W) + (unsigned)wcol[k])), (lptr)(win + 64 * k), 4, 0, 0);
        return (unsigned)((cx - 18) & 3);
    } else {
        const int x0 = cx - 18, y0 = cy - 18;
        const bool three = FORM == 2 || (x0 & 31) > 27;
        // first staged column: tile-aligned, or 16 bytes into a tile.  (FORM 2 off the real straddling alignments: the last span that starts 16 bytes
        // into a tile at or below x0; it misses the window's last columns when x0 - xs > 27 - the cost is what is measured, and k_check skips those)
        const int xs = three ? max(((x0 - 16) & ~31) + 16, 16) : (x0 & ~31);
        const unsigned tbase = (unsigned)(((y0 >> 2) * TPR + (xs >> 5)) * 128);
        const unsigned c = (three ? 16u : 0u) + 4u * (unsigned)(lane & 15);
        const unsigned loff = (c >> 5) * 128u + (unsigned)(lane >> 4) * 32u + (c & 31u);
        gbytes p = plane + tbase;
#pragma unroll
        for (int k = 0; k < 10; k++) { __builtin_amdgcn_global_load_lds((gptr)(p + loff), (lptr)(win + 64 * k), 4, 0, 0); p += TPR * 128; }
        return (unsigned)((y0 & 3) * 64 + (x0 - xs));
    }
}
__device__ __forceinline__ void pass_tables(int lane, int* wrow, int* wcol)
{
#pragma unroll
    for (int k = 0; k < 7; k++) { const int pos = 64 * k + lane, row = (pos * 5462) >> 16; wrow[k] = min(row, 36); wcol[k] = 4 * (pos - 12 * row); }
}
template <int FORM> __global__ __launch_bounds__(256) void k_time(const unsigned char* img, int nplanes, int iters, unsigned* sink)
{
    __shared__ unsigned lds[4][640];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int wrow[7], wcol[7]; pass_tables(lane, wrow, wcol);
    gbytes plane = uniform_ptr(img + (size_t)(blockIdx.x % nplanes) * PLANE);
    unsigned acc = 0;
    unsigned s = blockIdx.x * 2654435761u + wave * 40503u + 12345u;
    for (int it = 0; it < iters; it++) {
        s = s * 1664525u + 1013904223u;
        const int cx = __builtin_amdgcn_readfirstlane(32 + (s >> 8) % (W - 128)), cy = __builtin_amdgcn_readfirstlane(32 + (s >> 20) % (H - 96));
        gather<FORM>(plane, cx, cy, lane, lds[wave], wrow, wcol);
        __builtin_amdgcn_s_waitcnt(0x0f70);
        acc += lds[wave][lane];
    }
    sink[blockIdx.x * 256 + threadIdx.x] = acc;
}
// correctness of the tiled forms: every byte of the 37 x 37 window, read where k_describe would read it, against pixel()
template <int FORM> __global__ __launch_bounds__(64) void k_check(const unsigned char* img, int ncentres, unsigned* bad)
{
    __shared__ unsigned lds[640];
    const int lane = threadIdx.x;
    int wrow[7], wcol[7]; pass_tables(lane, wrow, wcol);
    gbytes plane = uniform_ptr(img);
    unsigned nbad = 0, s = 99u + blockIdx.x;
    for (int it = 0; it < ncentres; it++) {
        s = s * 1664525u + 1013904223u;
        // the borders k_describe may reach: cx - 18 >= 0 ... cx + 18 < W, the same for rows; every eighth centre sits on one
        int cx = 18 + (s >> 8) % (W - 36), cy = 18 + (s >> 20) % (H - 36);
        if ((it & 7) == 0) cx = (it & 8) ? W - 19 : 18;
        if ((it & 7) == 1) cy = (it & 8) ? H - 19 : 18;
        cx = __builtin_amdgcn_readfirstlane(cx); cy = __builtin_amdgcn_readfirstlane(cy);
        if (FORM == 2) { const int x0 = cx - 18, xs = ((x0 - 16) & ~31) + 16; if (x0 < 16 || xs + 64 > W || x0 - xs > 27) continue; }     // (c)'s forced span leaves the plane or the window there; (b) never takes it there
        const unsigned o = gather<FORM>(plane, cx, cy, lane, lds, wrow, wcol);
        __builtin_amdgcn_s_waitcnt(0x0f70);
        __builtin_amdgcn_wave_barrier();
        const unsigned char* w8 = reinterpret_cast<const unsigned char*>(lds) + o;
        for (int i = lane; i < 37 * 37; i += 64) { const int r = i / 37, c = i - 37 * r; if (w8[(r << 6) + c] != pixel(cx - 18 + c, cy - 18 + r, 0)) nbad++; }
        __builtin_amdgcn_wave_barrier();
    }
    atomicAdd(bad, nbad);
}
#define CHECK(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) { printf("%s failed: %s\n", #call, hipGetErrorString(e_)); return 1; } } while (0)
int main()
{
    const int NP = 1024;
    std::vector<unsigned char> rowmajor(PLANE), tiled(PLANE);
    for (unsigned y = 0; y < H; y++) for (unsigned x = 0; x < W; x++) { rowmajor[y * W + x] = pixel(x, y, 0); tiled[tiled_off(x, y)] = pixel(x, y, 0); }
    unsigned char *d_row, *d_tiled; unsigned *sink, *bad;
    CHECK(hipMalloc(&d_row, (size_t)PLANE * NP)); CHECK(hipMalloc(&d_tiled, (size_t)PLANE * NP));
    CHECK(hipMalloc(&sink, 4096 * 256 * 4)); CHECK(hipMalloc(&bad, 4));
    for (int f = 0; f < NP; f++) {      // the same plane everywhere: the timing needs the footprint, the check reads plane 0
        CHECK(hipMemcpyAsync(d_row + (size_t)f * PLANE, f ? d_row : rowmajor.data(), PLANE, f ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, 0));
        CHECK(hipMemcpyAsync(d_tiled + (size_t)f * PLANE, f ? d_tiled : tiled.data(), PLANE, f ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, 0));
    }
    CHECK(hipDeviceSynchronize());
    int wrong = 0;
    for (int form = 1; form < 3; form++) {
        CHECK(hipMemset(bad, 0, 4));
        if (form == 1) hipLaunchKernelGGL(k_check<1>, dim3(64), dim3(64), 0, 0, d_tiled, 256, bad);
        else hipLaunchKernelGGL(k_check<2>, dim3(64), dim3(64), 0, 0, d_tiled, 256, bad);
        unsigned nb = 0; CHECK(hipMemcpy(&nb, bad, 4, hipMemcpyDeviceToHost));
        printf("check (%c): %u wrong window bytes over 64 x 256 centres: %s\n", form == 1 ? 'b' : 'c', nb, nb ? "MISMATCH" : "ok");
        wrong += nb != 0;
    }
    if (hipDeviceSynchronize() != hipSuccess || wrong) { printf("tiled gather: NOT as assumed, no timing\n"); return 1; }
    hipEvent_t e0, e1; CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    const char* names[3] = {"(a) row-major, 7 passes", "(b) 32x4 tiles, 10 passes", "(c) as (b), 3 tile columns forced"};
    for (int np : {1, NP}) for (int form = 0; form < 3; form++) for (int rep = 0; rep < 4; rep++) {
        const unsigned char* img = form == 0 ? d_row : d_tiled;
        CHECK(hipEventRecord(e0));
        if (form == 0) hipLaunchKernelGGL(k_time<0>, dim3(4096), dim3(256), 0, 0, img, np, 200, sink);
        if (form == 1) hipLaunchKernelGGL(k_time<1>, dim3(4096), dim3(256), 0, 0, img, np, 200, sink);
        if (form == 2) hipLaunchKernelGGL(k_time<2>, dim3(4096), dim3(256), 0, 0, img, np, 200, sink);
        CHECK(hipEventRecord(e1));
        if (hipEventSynchronize(e1) != hipSuccess) { printf("kernel failed\n"); return 1; }
        float ms; CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (rep) printf("%-34s %4d plane%s run %d: %.3f ms = %.1f cycles of a CU per gather at 2.4 GHz\n", names[form], np, np > 1 ? "s" : " ", rep, ms, ms * 1e6 / (4096.0 * 4 * 200) * 256 * 2.4);
    }
    return 0;
}
