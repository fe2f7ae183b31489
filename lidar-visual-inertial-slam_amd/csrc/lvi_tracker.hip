// feature_tracker hot path for gfx950 behind the C-ABI:
//   cv::calcOpticalFlowPyrLK(cur, forw, pts, …, Size(21,21), 3)   feature_tracker.cpp:113
//   cv::goodFeaturesToTrack(forw, n_pts, N, 0.01, MIN_DIST, mask)  feature_tracker.cpp:166
//
// LK: the pyramids of the two resident images are built once per image (pyrDown, integer exact).
// One wavefront per feature walks the levels top→0 inside ONE launch: the 24x24 source tile of the
// previous level is staged in LDS, Scharr derivatives are formed on the fly for that tile only
// (OpenCV differentiates the whole level), the 21x21 patch and its gradient live in registers
// (7 pixels per lane), and every Newton step re-stages the 22x22 target tile and reduces the two
// mismatch sums across the wave.  All patch arithmetic is OpenCV's fixed point (W_BITS = 14) with
// exact int64 sums (the aarch64 build of OpenCV, which is what the reference's Jetson runs), so the
// result does not depend on reduction order and matches the CPU restatement bit for bit.
//
// GFTT: min-eigenvalue map (Sobel 3x3 → products → 3x3 box, f64 box accumulation as cv::boxFilter),
// masked max (order-encoded atomicMax), threshold + 3x3 non-maximum test + ordered compaction,
// stable radix sort by value (descending, ties by higher address first), and the sequential
// minimum-distance pick done by one wavefront with ballot-resolved conflicts.
#include <algorithm>

#include "lvi_mei.hpp"
#include "lvi_sort.hpp"
#include "../../include/lvi_tbatch.h"

namespace lvi {

namespace {

constexpr int MAX_LEVELS = 8;
constexpr int LK_WIN_MAX = 21;

struct Level { uint8_t* px; int w, h; };
struct Pyr { Level lv[MAX_LEVELS]; int top; };

__device__ __forceinline__ int reflect101(int p, int len)
{
    if (len == 1) return 0;
    while (p < 0 || p >= len) p = (p < 0) ? -p : 2 * len - 2 - p;
    return p;
}

// ------------------------------------------------------------------------------------------- pyrDown
__device__ __forceinline__ void pyrdown_body(const uint8_t* __restrict__ src, int sw, int sh, uint8_t* __restrict__ dst, int dw, int dh)
{
    const int x = blockIdx.x * 32 + (threadIdx.x & 31);
    const int y = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x >= dw || y >= dh) return;
    int sum = 0;
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const int sy = reflect101(2 * y + j - 2, sh);
        const uint8_t* row = src + (size_t)sy * sw;
        const int r = row[reflect101(2 * x - 2, sw)] + 4 * row[reflect101(2 * x - 1, sw)] + 6 * row[2 * x < sw ? 2 * x : reflect101(2 * x, sw)]
                    + 4 * row[reflect101(2 * x + 1, sw)] + row[reflect101(2 * x + 2, sw)];
        sum += (j == 0 || j == 4) ? r : (j == 2 ? 6 * r : 4 * r);
    }
    dst[(size_t)y * dw + x] = (uint8_t)((sum + 128) >> 8);
}
// Every tracker kernel has ONE entry: the slot in blockIdx.z, one by-value table of per-slot argument blocks per launch (as
// lvi_scan.hip's B_.a[blockIdx.z]).  A zeroed block is a slot that sits the call out; the grid is sized for the largest slot, and a
// workgroup beyond its own slot's extent returns at once (uniform per workgroup).  A set of one slot (a single handle) launches the
// entry's instantiation for a table of ONE block, grid.z = 1: the eight-block table cost lk_track, gftt_sortpick and gftt_mineig
// 0.2 - 0.7 us each against arguments passed directly, the one-block table is those arguments.
template <class T, int N = LVI_TRACKER_MAX_BATCH> struct TBatch { T a[N]; };
template <class T, int N> __device__ __forceinline__ const T& slot_args(const TBatch<T, N>& B) { return B.a[N == 1 ? 0 : blockIdx.z]; }
#define LVI_TBATCH_FITS(T) static_assert(sizeof(TBatch<T>) <= 4096, #T ": the per-slot table exceeds the 4 KB kernel-argument limit")
struct PyrArgs { const uint8_t* src; uint8_t* dst; int sw, sh, dw, dh; };
LVI_TBATCH_FITS(PyrArgs);
template <int N>
__global__ __launch_bounds__(256) void pyrdown_kernel(TBatch<PyrArgs, N> B_)
{
    const PyrArgs& a = slot_args(B_);
    if ((int)blockIdx.x * 32 >= a.dw || (int)blockIdx.y * 8 >= a.dh) return;
    pyrdown_body(a.src, a.sw, a.sh, a.dst, a.dw, a.dh);
}

// ------------------------------------------------------------------------------------------- LK
struct LkArgs {
    Pyr prev, next;
    const float* prev_xy; float* next_xy; uint8_t* status; float* err;
    float* h_next_xy; uint8_t* h_status; float* h_err;     // host-mapped mirrors of the three results (nullptr: none): get_lk reads them after one wait, no copy commands
    int n, win, max_level, max_count;
    double epsilon; float min_eig;
};

#define LVI_DESCALE(x, n) (((x) + (1 << ((n)-1))) >> (n))
__device__ __forceinline__ int cv_floor(float v) { const int i = (int)v; return i - (i > v); }
__device__ __forceinline__ int cv_round(float v) { return __float2int_rn(v); }

// ---------------------------------------------------------------------------------------------
// f-2  cv::CLAHE::apply, CV_8UC1 (OpenCV imgproc/src/clahe.cpp).  clahe_lut: one workgroup per tile — LDS
// histogram, clip + redistribution evaluated per bin (the serial residual loop hits bins 0, step, 2·step, …),
// inclusive scan, lut = saturate(cvRound(sum * lutScale)).  clahe_interp: one thread per pixel, the f32 blend of
// the four surrounding tile LUTs in the reference's operation order (the library is built -ffp-contract=off).
// ---------------------------------------------------------------------------------------------
struct ClaheArgs {
    const uint8_t* src; uint8_t* dst; uint8_t* lut;
    int W, H, tilesX, tilesY, tw, th, clipLimit; float lutScale;
};

LVI_TBATCH_FITS(ClaheArgs);
template <int N>
__global__ __launch_bounds__(1024) void clahe_lut_kernel(TBatch<ClaheArgs, N> B_)
{
    const ClaheArgs& a = slot_args(B_);
    if ((int)blockIdx.x >= a.tilesX * a.tilesY) return;
    // 1024 threads per tile, four pixels per load, one histogram per wavefront (a tile of the 1280 x 720 frame is 14 400 pixels: 256
    // threads reading bytes one by one into ONE histogram were 32 us of the node's frame — 64 workgroups, 56 dependent rounds each)
    __shared__ int whist[16][256];
    __shared__ int ws[17];
    const int k = blockIdx.x, tx = k % a.tilesX, ty = k / a.tilesX, tid = threadIdx.x, wv = tid >> 6;
    for (int i = tid; i < 16 * 256; i += 1024) (&whist[0][0])[i] = 0;
    __syncthreads();
    const int area = a.tw * a.th;
    const int x0 = tx * a.tw, y0 = ty * a.th;
    const bool vec = (a.tw & 3) == 0 && (a.W & 3) == 0 && x0 + a.tw <= a.W && y0 + a.th <= a.H;     // (x0 is then a multiple of 4 as well)
    if (vec) {
        const int qw = a.tw >> 2, nq = qw * a.th;
        constexpr int NL = 4;
        for (int q0 = tid; q0 < nq; q0 += NL * 1024) {
            unsigned v[NL];
#pragma unroll
            for (int u = 0; u < NL; u++) {
                const int q = min(q0 + u * 1024, nq - 1);
                v[u] = *reinterpret_cast<const unsigned*>(a.src + (size_t)(y0 + q / qw) * a.W + x0 + 4 * (q % qw));
            }
#pragma unroll
            for (int u = 0; u < NL; u++) {
                if (q0 + u * 1024 >= nq) continue;
                atomicAdd(&whist[wv][v[u] & 255u], 1); atomicAdd(&whist[wv][(v[u] >> 8) & 255u], 1);
                atomicAdd(&whist[wv][(v[u] >> 16) & 255u], 1); atomicAdd(&whist[wv][v[u] >> 24], 1);
            }
        }
    } else {
        for (int idx = tid; idx < area; idx += 1024) {
            const int x = x0 + idx % a.tw, y = y0 + idx / a.tw;
            // right / bottom extension of images that are not a multiple of the tile grid: BORDER_REFLECT_101
            const int sx = x < a.W ? x : reflect101(x, a.W), sy = y < a.H ? y : reflect101(y, a.H);
            atomicAdd(&whist[wv][a.src[(size_t)sy * a.W + sx]], 1);
        }
    }
    __syncthreads();
    // bins live in the first 256 threads; the others contribute zeros to the two scans (every thread reaches every barrier)
    int hv = 0;
    if (tid < 256) {
#pragma unroll
        for (int q = 0; q < 16; q++) hv += whist[q][tid];
    }
    if (a.clipLimit > 0) {
        const int excess = max(hv - a.clipLimit, 0);
        hv = min(hv, a.clipLimit);
        int clipped;
        (void)block_excl_scan<1024>(excess, ws, &clipped);
        const int redistBatch = clipped / 256;
        const int residual = clipped - redistBatch * 256;
        if (tid < 256) {
            hv += redistBatch;
            if (residual != 0) {
                const int step = max(256 / residual, 1);
                if (tid % step == 0 && tid / step < residual) hv++;
            }
        }
    }
    int tot;
    const int sum = block_excl_scan<1024>(hv, ws, &tot) + hv;
    const int v = cv_round((float)sum * a.lutScale);
    if (tid >= 256) return;
    a.lut[(size_t)k * 256 + tid] = (uint8_t)min(max(v, 0), 255);
}

template <int N>
__global__ __launch_bounds__(256) void clahe_interp_kernel(TBatch<ClaheArgs, N> B_)
{
    const ClaheArgs& a = slot_args(B_);
    if ((int)blockIdx.x * 64 >= a.W || (int)blockIdx.y * 4 >= a.H) return;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.W || y >= a.H) return;
    const float inv_tw = 1.0f / a.tw, inv_th = 1.0f / a.th;
    const float tyf = (float)y * inv_th - 0.5f;
    int ty1 = cv_floor(tyf), ty2 = ty1 + 1;
    const float ya = tyf - (float)ty1, ya1 = 1.0f - ya;
    ty1 = max(ty1, 0); ty2 = min(ty2, a.tilesY - 1);
    const float txf = (float)x * inv_tw - 0.5f;
    int tx1 = cv_floor(txf), tx2 = tx1 + 1;
    const float xa = txf - (float)tx1, xa1 = 1.0f - xa;
    tx1 = max(tx1, 0); tx2 = min(tx2, a.tilesX - 1);
    const int srcVal = a.src[(size_t)y * a.W + x];
    const uint8_t* p1 = a.lut + (size_t)ty1 * a.tilesX * 256;
    const uint8_t* p2 = a.lut + (size_t)ty2 * a.tilesX * 256;
    const int ind1 = tx1 * 256 + srcVal, ind2 = tx2 * 256 + srcVal;
    const float res = ((float)p1[ind1] * xa1 + (float)p1[ind2] * xa) * ya1 + ((float)p2[ind1] * xa1 + (float)p2[ind2] * xa) * ya;
    a.dst[(size_t)y * a.W + x] = (uint8_t)min(max(cv_round(res), 0), 255);
}

// ---------------------------------------------------------------------------------------------
// f-3  CataCamera::liftProjective with the 8-step recursive distortion model + (b.x/b.z, b.y/b.z) → Point2f
// (CataCamera.cc:556-626, 766-783; feature_tracker.cpp:306-309).  All in double, one thread per point.
// ---------------------------------------------------------------------------------------------
// (the device function lives in lvi_mei.hpp: the keyframe describer of lvi_kf.hip compiles the same code)
__device__ __forceinline__ void mei_undistort_body(const lvi_mei_params& c, const float* __restrict__ xy, int n, float* __restrict__ out, const int* __restrict__ n_dev)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (n_dev) n = min(n, *n_dev);                  // (the count of a device-side concatenation)
    if (i >= n) return;
    mei_lift_normalized(c, xy[2 * i], xy[2 * i + 1], out[2 * i], out[2 * i + 1]);
}
struct MeiArgs { lvi_mei_params c; const float* xy; float* out; const int* n_dev; int n; };
LVI_TBATCH_FITS(MeiArgs);
template <int N>
__global__ __launch_bounds__(64) void mei_undistort_kernel(TBatch<MeiArgs, N> B_)
{
    const MeiArgs& a = slot_args(B_);
    if ((int)blockIdx.x * 64 >= a.n) return;
    mei_undistort_body(a.c, a.xy, a.n, a.out, a.n_dev);
}

// setMask (feature_tracker.cpp:36-69): mask = 255, then cv::circle(mask, pt, MIN_DIST, 0, -1) around every kept point.  The
// filled circle is OpenCV's midpoint raster (FillCircle): row cy +- dy spans cx +- dx and row cy +- dx spans cx +- dy for the
// (dx, dy) the integer error recurrence visits; hw[j] = the widest of the spans of row offset j.  One thread per (circle, row).
struct CircleArgs { uint8_t* mask; int w, h; const float* centers; int n; int radius; };
LVI_TBATCH_FITS(CircleArgs);
template <int N>
__global__ __launch_bounds__(256) void mask_fill_kernel(TBatch<CircleArgs, N> B_)
{
    const CircleArgs& a = slot_args(B_);
    if (!a.mask || (size_t)blockIdx.x * 256 * 16 >= (size_t)a.w * a.h) return;
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 16;
    if (i + 16 <= (size_t)a.w * a.h) *reinterpret_cast<uint4*>(a.mask + i) = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
    else for (size_t k = i; k < (size_t)a.w * a.h; k++) a.mask[k] = 255;
}
template <int N>
__global__ __launch_bounds__(64) void mask_circles_kernel(TBatch<CircleArgs, N> B_)
{
    const CircleArgs& a = slot_args(B_);
    if (!a.mask || (int)blockIdx.x >= a.n) return;
    __shared__ int hw[128];
    const int r = a.radius;
    if (threadIdx.x == 0) {
        for (int j = 0; j <= r; j++) hw[j] = -1;
        int err = 0, dx = r, dy = 0, plus = 1, minus = (r << 1) - 1;
        while (dx >= dy) {
            hw[dy] = max(hw[dy], dx); hw[dx] = max(hw[dx], dy);
            dy++;
            err += plus; plus += 2;
            const int m = (err <= 0) - 1;
            err -= minus & m; dx += m; minus -= m & 2;
        }
    }
    __syncthreads();
    const int c = blockIdx.x;
    if (c >= a.n) return;
    const int cx = (int)rintf(a.centers[2 * c]), cy = (int)rintf(a.centers[2 * c + 1]);      // Mat::at(Point2f) / cv::circle round the centre (cvRound)
    for (int j = threadIdx.x; j <= 2 * r; j += 64) {
        const int off = j - r, y = cy + off, half = hw[off < 0 ? -off : off];
        if (y < 0 || y >= a.h || half < 0) continue;
        const int x0 = max(cx - half, 0), x1 = min(cx + half, a.w - 1);
        for (int x = x0; x <= x1; x++) a.mask[(size_t)y * a.w + x] = 0;
    }
}

// undistortedPoints over [the kept points (host) ; the corners goodFeaturesToTrack just found (device)]: cur_pts of the next frame
__device__ __forceinline__ void frame_concat_body(const float* __restrict__ kept, int n_kept, const float* __restrict__ found, const int* __restrict__ n_found,
                                                  const int* __restrict__ n_cand, int with_gftt, int cap, float* __restrict__ all_xy, int* __restrict__ d_hdr,
                                                  int* __restrict__ h_hdr, float* __restrict__ h_new)
{
    // kept: the caller's points in pinned host memory (read in place); h_hdr / h_new: the frame's result block in pinned host memory —
    // {n_new (or the pick kernel's negative code), n_cand, n_all}, then the new corners: the frame end is kernels and one wait
    const int nraw = with_gftt ? *n_found : 0;
    const int nf = min(max(nraw, 0), cap);
    const int n = min(n_kept + nf, cap);
    for (int i = threadIdx.x; i < n; i += 64) {
        const float* src = i < n_kept ? kept + 2 * i : found + 2 * (i - n_kept);
        const float x = src[0], y = src[1];
        all_xy[2 * i] = x; all_xy[2 * i + 1] = y;
        if (i >= n_kept) { h_new[2 * (i - n_kept)] = x; h_new[2 * (i - n_kept) + 1] = y; }
    }
    if (threadIdx.x == 0) { d_hdr[2] = n; h_hdr[0] = nraw; h_hdr[1] = with_gftt ? *n_cand : 0; h_hdr[2] = n; }
}
struct ConcatArgs { const float* kept; const float* found; const int* n_found; const int* n_cand; float* all_xy; int* d_hdr; int* h_hdr; float* h_new; int n_kept, with_gftt, cap; };
LVI_TBATCH_FITS(ConcatArgs);
template <int N>
__global__ __launch_bounds__(64) void frame_concat_kernel(TBatch<ConcatArgs, N> B_)
{
    const ConcatArgs& a = slot_args(B_);
    if (!a.d_hdr) return;
    frame_concat_body(a.kept, a.n_kept, a.found, a.n_found, a.n_cand, a.with_gftt, a.cap, a.all_xy, a.d_hdr, a.h_hdr, a.h_new);
}
LVI_TBATCH_FITS(LkArgs);               // two 8-level Pyr: 360 bytes per slot
template <int N>
__global__ __launch_bounds__(64) void lk_kernel(TBatch<LkArgs, N> B_)
{
    const LkArgs& a = slot_args(B_);     // (a workgroup past its slot's n returns below, first thing)
    constexpr int TW = LK_WIN_MAX + 3;             // 24: source tile (window + 1 for bilinear + 1 on each side for Scharr)
    constexpr int DW = LK_WIN_MAX + 1;             // 22: derivative / target tile
    constexpr int NPX = (LK_WIN_MAX * LK_WIN_MAX + 63) / 64;   // 7 window pixels per lane
    __shared__ uint8_t sI[TW * TW];
    __shared__ short sD[DW * DW * 2];
    // target image: a region of JW x JW pixels around the window stays in LDS across the iterations of a level (the window moves
    // by a fraction of a pixel per iteration: reloading its 22 x 22 tile from L2 every iteration was most of the kernel's 80 us)
    constexpr int JR = 8, JW = DW + 2 * JR;
    __shared__ uint8_t sJ[JW * JW];
    int jx0 = 0, jy0 = 0; bool jvalid = false;     // absolute coordinates of sJ[0] in the level (uniform over the wavefront)
    const int f = blockIdx.x, l = threadIdx.x;
    if (f >= a.n) return;
    const int win = a.win;
    const float halfWin = (win - 1) * 0.5f;
    // window pixels of this lane, (row, column), once: `win` is a run-time value and an integer division costs ~40 instructions
    // (lanes beyond the window take pixel (0, 0) and are masked out: no branch inside the pixel loops, so that the LDS reads
    // of all seven pixels are in flight together — one wavefront per workgroup has nothing else to hide their latency)
    int wy[NPX], wx[NPX]; bool wv[NPX];
#pragma unroll
    for (int j = 0; j < NPX; j++) { const int p = l + 64 * j; wv[j] = p < win * win; wy[j] = wv[j] ? p / win : 0; wx[j] = wv[j] ? p - wy[j] * win : 0; }
    const float px0 = a.prev_xy[2 * f], py0 = a.prev_xy[2 * f + 1];
    float outx = 0.f, outy = 0.f, errv = 0.f;
    bool st = true;
    const int W_BITS = 14;
    const float FLT_SCALE = 1.f / (1 << 20);

    for (int level = a.max_level; level >= 0; level--) {
        const Level I = a.prev.lv[level], J = a.next.lv[level];
        jvalid = false;
        // make the window [inx, inx + DW) x [iny, iny + DW) of the target level resident; returns the offset of its corner in sJ
        constexpr int NJ = (JW * JW + 63) / 64;
        // all loads of a lane are issued before the first one is stored (a loop of load, wait, store was 23 round trips to L2)
        auto region_issue = [&](int x0, int y0, uint8_t (&rj)[NJ]) {
            if (x0 >= 0 && y0 >= 0 && x0 + JW <= J.w && y0 + JW <= J.h) {                  // interior: no border arithmetic
                const uint8_t* __restrict__ src = J.px + (size_t)y0 * J.w + x0;
#pragma unroll
                for (int k = 0; k < NJ; k++) { const int t = l + 64 * k, ty = t / JW, tx = t - ty * JW; rj[k] = t < JW * JW ? src[ty * J.w + tx] : (uint8_t)0; }
            } else {
#pragma unroll
                for (int k = 0; k < NJ; k++) {
                    const int t = l + 64 * k, ty = t / JW, tx = t - ty * JW;
                    rj[k] = t < JW * JW ? J.px[(size_t)reflect101(y0 + ty, J.h) * J.w + reflect101(x0 + tx, J.w)] : (uint8_t)0;
                }
            }
        };
        auto region_commit = [&](int x0, int y0, const uint8_t (&rj)[NJ]) {
#pragma unroll
            for (int k = 0; k < NJ; k++) { const int t = l + 64 * k; if (t < JW * JW) sJ[t] = rj[k]; }
            jx0 = x0; jy0 = y0; jvalid = true;
        };
        // make the window [inx, inx + DW) x [iny, iny + DW) of the target level resident; returns the offset of its corner in sJ
        auto target_window = [&](int inx, int iny) {
            if (!(jvalid && inx >= jx0 && inx + DW <= jx0 + JW && iny >= jy0 && iny + DW <= jy0 + JW)) {
                __syncthreads();
                uint8_t rj[NJ];
                region_issue(inx - JR, iny - JR, rj);
                region_commit(inx - JR, iny - JR, rj);
                __syncthreads();
            }
            return (iny - jy0) * JW + (inx - jx0);
        };
        float prevx = px0 * (float)(1. / (1 << level)), prevy = py0 * (float)(1. / (1 << level));
        float nextx, nexty;
        if (level == a.max_level) { nextx = prevx; nexty = prevy; }
        else { nextx = outx * 2.f; nexty = outy * 2.f; }
        outx = nextx; outy = nexty;
        prevx -= halfWin; prevy -= halfWin;
        const int ipx = cv_floor(prevx), ipy = cv_floor(prevy);
        if (ipx < -win || ipx >= I.w || ipy < -win || ipy >= I.h) {
            if (level == 0) { st = false; errv = 0.f; }
            continue;
        }
        // ---- stage the source tile (REFLECT_101 border of the pyramid level) and its Scharr derivatives
        __syncthreads();
        {
            constexpr int NI = (TW * TW + 63) / 64;
            uint8_t ri[NI];
            if (ipx >= 1 && ipy >= 1 && ipx - 1 + TW <= I.w && ipy - 1 + TW <= I.h) {      // interior: no border arithmetic
                const uint8_t* __restrict__ src = I.px + (size_t)(ipy - 1) * I.w + (ipx - 1);
#pragma unroll
                for (int k = 0; k < NI; k++) { const int t = l + 64 * k, ty = t / TW, tx = t - ty * TW; ri[k] = t < TW * TW ? src[ty * I.w + tx] : (uint8_t)0; }
            } else {
#pragma unroll
                for (int k = 0; k < NI; k++) {
                    const int t = l + 64 * k, ty = t / TW, tx = t - ty * TW;
                    ri[k] = t < TW * TW ? I.px[(size_t)reflect101(ipy - 1 + ty, I.h) * I.w + reflect101(ipx - 1 + tx, I.w)] : (uint8_t)0;
                }
            }
#pragma unroll
            for (int k = 0; k < NI; k++) { const int t = l + 64 * k; if (t < TW * TW) sI[t] = ri[k]; }
        }
        __syncthreads();
        {
            constexpr int ND = (DW * DW + 63) / 64;
            short gxs[ND], gys[ND];
#pragma unroll
            for (int k = 0; k < ND; k++) {
                const int t = min(l + 64 * k, DW * DW - 1);
                const int dy_ = t / DW, dx_ = t - dy_ * DW;
                const int X = ipx + dx_, Y = ipy + dy_;
                const uint8_t* c = &sI[(dy_ + 1) * TW + (dx_ + 1)];
                const int p00 = c[-TW - 1], p01 = c[-TW], p02 = c[-TW + 1], p10 = c[-1], p12 = c[1], p20 = c[TW - 1], p21 = c[TW], p22 = c[TW + 1];
                const bool in = X >= 0 && X < I.w && Y >= 0 && Y < I.h;             // the derivative image is zero outside the level
                gxs[k] = in ? (short)(((p02 + p22) * 3 + p12 * 10) - ((p00 + p20) * 3 + p10 * 10)) : (short)0;
                gys[k] = in ? (short)(((p20 - p00) + (p22 - p02)) * 3 + (p21 - p01) * 10) : (short)0;
            }
#pragma unroll
            for (int k = 0; k < ND; k++) { const int t = l + 64 * k; if (t < DW * DW) { sD[2 * t] = gxs[k]; sD[2 * t + 1] = gys[k]; } }
        }
        __syncthreads();
        float aa = prevx - ipx, bb = prevy - ipy;
        int iw00 = cv_round((1.f - aa) * (1.f - bb) * (1 << W_BITS));
        int iw01 = cv_round(aa * (1.f - bb) * (1 << W_BITS));
        int iw10 = cv_round((1.f - aa) * bb * (1 << W_BITS));
        int iw11 = (1 << W_BITS) - iw00 - iw01 - iw10;
        short Iw[NPX], Ix[NPX], Iy[NPX];
        long long sA11 = 0, sA12 = 0, sA22 = 0;
#pragma unroll
        for (int j = 0; j < NPX; j++) {
            const int y = wy[j], x = wx[j];
            const uint8_t* s = &sI[(y + 1) * TW + (x + 1)];
            const short* d = &sD[2 * (y * DW + x)];
            const int ival = wv[j] ? LVI_DESCALE(s[0] * iw00 + s[1] * iw01 + s[TW] * iw10 + s[TW + 1] * iw11, W_BITS - 5) : 0;
            const int ixval = wv[j] ? LVI_DESCALE(d[0] * iw00 + d[2] * iw01 + d[2 * DW] * iw10 + d[2 * DW + 2] * iw11, W_BITS) : 0;
            const int iyval = wv[j] ? LVI_DESCALE(d[1] * iw00 + d[3] * iw01 + d[2 * DW + 1] * iw10 + d[2 * DW + 3] * iw11, W_BITS) : 0;
            Iw[j] = (short)ival; Ix[j] = (short)ixval; Iy[j] = (short)iyval;
            sA11 += ixval * ixval; sA12 += ixval * iyval; sA22 += iyval * iyval;
        }
        sA11 = wave_sum_i64(sA11); sA12 = wave_sum_i64(sA12); sA22 = wave_sum_i64(sA22);
        const float A11 = (float)sA11 * FLT_SCALE, A12 = (float)sA12 * FLT_SCALE, A22 = (float)sA22 * FLT_SCALE;
        float D = A11 * A22 - A12 * A12;
        const float minEig = (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) / (2 * win * win);
        if (minEig < a.min_eig || D < 1.1920929e-7f) {
            if (level == 0) st = false;
            continue;
        }
        D = 1.f / D;
        nextx -= halfWin; nexty -= halfWin;
        float pdx = 0.f, pdy = 0.f;
        for (int j = 0; j < a.max_count; j++) {
            const int inx = cv_floor(nextx), iny = cv_floor(nexty);
            if (inx < -win || inx >= J.w || iny < -win || iny >= J.h) {
                if (level == 0) st = false;
                break;
            }
            const int jo = target_window(inx, iny);
            aa = nextx - inx; bb = nexty - iny;
            iw00 = cv_round((1.f - aa) * (1.f - bb) * (1 << W_BITS));
            iw01 = cv_round(aa * (1.f - bb) * (1 << W_BITS));
            iw10 = cv_round((1.f - aa) * bb * (1 << W_BITS));
            iw11 = (1 << W_BITS) - iw00 - iw01 - iw10;
            long long ib1 = 0, ib2 = 0;
#pragma unroll
            for (int q = 0; q < NPX; q++) {
                const uint8_t* s = &sJ[jo + wy[q] * JW + wx[q]];          // a lane beyond the window reads pixel (0, 0): its Ix = Iy = 0
                const int diff = LVI_DESCALE(s[0] * iw00 + s[1] * iw01 + s[JW] * iw10 + s[JW + 1] * iw11, W_BITS - 5) - Iw[q];
                ib1 += diff * Ix[q]; ib2 += diff * Iy[q];
            }
            ib1 = wave_sum_i64(ib1); ib2 = wave_sum_i64(ib2);
            const float b1 = (float)ib1 * FLT_SCALE, b2 = (float)ib2 * FLT_SCALE;
            const float dx = (float)((A12 * b2 - A22 * b1) * D);
            const float dy = (float)((A12 * b1 - A11 * b2) * D);
            nextx += dx; nexty += dy;
            outx = nextx + halfWin; outy = nexty + halfWin;
            if ((double)dx * dx + (double)dy * dy <= a.epsilon) break;
            if (j > 0 && fabsf(dx + pdx) < 0.01 && fabsf(dy + pdy) < 0.01) {
                outx -= dx * 0.5f; outy -= dy * 0.5f;
                break;
            }
            pdx = dx; pdy = dy;
        }
        if (st && level == 0) {
            const float nx = outx - halfWin, ny = outy - halfWin;
            const int inx = cv_floor(nx), iny = cv_floor(ny);
            if (inx < -win || inx >= J.w || iny < -win || iny >= J.h) { st = false; continue; }
            const int jo = target_window(inx, iny);
            aa = nx - inx; bb = ny - iny;
            iw00 = cv_round((1.f - aa) * (1.f - bb) * (1 << W_BITS));
            iw01 = cv_round(aa * (1.f - bb) * (1 << W_BITS));
            iw10 = cv_round((1.f - aa) * bb * (1 << W_BITS));
            iw11 = (1 << W_BITS) - iw00 - iw01 - iw10;
            int esum = 0;                                  // |diff| are integers; the f32 sum of OpenCV is exact (< 2^24)
#pragma unroll
            for (int q = 0; q < NPX; q++) {
                const uint8_t* s = &sJ[jo + wy[q] * JW + wx[q]];
                const int diff = LVI_DESCALE(s[0] * iw00 + s[1] * iw01 + s[JW] * iw10 + s[JW + 1] * iw11, W_BITS - 5) - Iw[q];
                esum += wv[q] ? abs(diff) : 0;
            }
            esum = wave_sum(esum);
            errv = (float)esum * 1.f / (32 * win * win);
        }
    }
    if (l == 0) {
        a.next_xy[2 * f] = outx; a.next_xy[2 * f + 1] = outy;
        a.status[f] = st ? 1 : 0; a.err[f] = errv;
        if (a.h_next_xy) { a.h_next_xy[2 * f] = outx; a.h_next_xy[2 * f + 1] = outy; a.h_status[f] = st ? 1 : 0; a.h_err[f] = errv; }
    }
}

// ------------------------------------------------------------------------------------------- GFTT
struct GfttArgs {
    const uint8_t* img; const uint8_t* mask; int w, h;
    float* eig; unsigned* maxord; float* thr;
    unsigned* maxPartial;            // [npartial] one per workgroup of mineig_kernel, rows of gx (the slot's own layout, not the grid's)
    int gx, npartial, nblk;          // the sizes derived from w, h (gftt_args): mineig's workgroups per row and in all, tiles of CAND_TILE pixels
    int* blockCnt; int* total;
    unsigned *keysA, *valsA;
    int *d_n, *d_nbits;
    double quality;
};

__device__ __forceinline__ void sobel_at(const uint8_t* img, int w, int h, int x, int y, float k0, float k1, float& Dx, float& Dy)
{
    // evaluated at in-image (x,y); neighbours through REFLECT_101
    const int xm = reflect101(x - 1, w), xp = reflect101(x + 1, w), ym = reflect101(y - 1, h), yp = reflect101(y + 1, h);
    const uint8_t *r0 = img + (size_t)ym * w, *r1 = img + (size_t)y * w, *r2 = img + (size_t)yp * w;
    const float a0 = r0[xm], a1 = r0[x], a2 = r0[xp], b0 = r1[xm], b2 = r1[xp], c0 = r2[xm], c1 = r2[x], c2 = r2[xp];
    // dx: row [-1 0 1] exact, column [1 2 1]*scale:  (S0 + S2)*k1 + S1*k0
    const float S0 = a2 - a0, S1 = b2 - b0, S2 = c2 - c0;
    const float u = (S0 + S2) * k1, v = S1 * k0;
    Dx = u + v;
    // dy: row [1 2 1]*scale: S[0]*k0 + (S[-1]+S[1])*k1, column [-1 0 1]
    const float t0 = a1 * k0, t1 = (a0 + a2) * k1, rs0 = t0 + t1;
    const float t2 = c1 * k0, t3 = (c0 + c2) * k1, rs2 = t2 + t3;
    Dy = rs2 - rs0;
}

// Tile of 32 x 8 output pixels: the Sobel products of the 34 x 10 pixels under the 3x3 box are computed ONCE into
// LDS (the first version recomputed them nine times per pixel), then every thread adds its nine in the reference's
// order (rows, then columns, in double).  The masked maximum goes to one partial per workgroup; gftt_thr folds them
// (14 400 wavefronts hitting one atomicMax address cost ~0.16 ms: same-address atomics serialise).
LVI_TBATCH_FITS(GfttArgs);
template <int N>
__global__ __launch_bounds__(256) void mineig_kernel(TBatch<GfttArgs, N> B_)
{
    const GfttArgs& a = slot_args(B_);
    if ((int)blockIdx.x * 32 >= a.w || (int)blockIdx.y * 8 >= a.h) return;
    constexpr int TW = 34, TH = 10;
    __shared__ float sxx[TH][TW], sxy[TH][TW], syy[TH][TW];
    __shared__ unsigned smax[4];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int x0 = blockIdx.x * 32, y0 = blockIdx.y * 8;
    const double scale = 1.0 / (4.0 * 3.0 * 255.0);
    const float k1 = (float)(1.0 * scale), k0 = (float)(2.0 * scale);
    for (int e = threadIdx.x; e < TW * TH; e += 256) {
        const int ex = e % TW, ey = e / TW;
        // the box reads pixel reflect101(x + i), reflect101(y + j); Sobel is evaluated at that in-image pixel
        const int px = reflect101(x0 - 1 + ex, a.w), py = reflect101(y0 - 1 + ey, a.h);
        float dx, dy;
        sobel_at(a.img, a.w, a.h, px, py, k0, k1, dx, dy);
        sxx[ey][ex] = dx * dx; sxy[ey][ex] = dx * dy; syy[ey][ex] = dy * dy;
    }
    __syncthreads();
    const int x = x0 + tx, y = y0 + ty;
    float val = 0.f; const bool in = (x < a.w && y < a.h);
    if (in) {
        double s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
        for (int j = 0; j < 3; j++)
#pragma unroll
            for (int i = 0; i < 3; i++) { s0 += sxx[ty + j][tx + i]; s1 += sxy[ty + j][tx + i]; s2 += syy[ty + j][tx + i]; }
        const float A = (float)s0 * 0.5f, B = (float)s1, C = (float)s2 * 0.5f;
        const float t = (A - C) * (A - C), u = B * B;
        val = (A + C) - sqrtf(t + u);
        a.eig[(size_t)y * a.w + x] = val;
    }
    // masked maximum (minMaxLoc with mask)
    const bool counted = in && (!a.mask || a.mask[(size_t)y * a.w + x]);
    unsigned o = counted ? f2ord(val) : 0u;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) { const unsigned t = __shfl_xor(o, s, 64); o = t > o ? t : o; }
    if (lane_id() == 0) smax[wave_id()] = o;
    __syncthreads();
    if (threadIdx.x == 0) a.maxPartial[blockIdx.y * a.gx + blockIdx.x] = max(max(smax[0], smax[1]), max(smax[2], smax[3]));
}

// quality threshold = max over the (masked) min-eigenvalue image x qualityLevel (featureselect.cpp): the fold of mineig's per-workgroup
// maxima.  Every workgroup of gftt_count folds the few thousand partial maxima itself (a separate one-workgroup launch was 4.6 us of
// the node's frame); its first workgroup leaves the result for gftt_emit and the debug views.
__device__ __forceinline__ float gftt_threshold(const GfttArgs& a, unsigned* smax)
{
    unsigned o = 0u;
    for (int i = threadIdx.x; i < a.npartial; i += 256) o = max(o, a.maxPartial[i]);
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) { const unsigned t = __shfl_xor(o, s, 64); o = t > o ? t : o; }
    if (lane_id() == 0) smax[wave_id()] = o;
    __syncthreads();
    o = max(max(smax[0], smax[1]), max(smax[2], smax[3]));
    const double maxVal = o ? (double)ord2f(o) : 0.0;
    const float thr = (float)(maxVal * a.quality);
    if (blockIdx.x == 0 && threadIdx.x == 0) { *a.maxord = o; *a.thr = thr; }
    return thr;
}

__device__ __forceinline__ bool gftt_is_cand(const GfttArgs& a, int x, int y, float thr)
{
    // the 3 x 3 neighbourhood and the mask byte are loaded unconditionally (coordinates clamped into the interior) and tested
    // afterwards: with the tests in between, a pixel was up to ten round trips in a row
    if (a.w < 3 || a.h < 3) return false;          // no interior (candidates are 1..size-2): the clamp below would leave the image
    const int xc = min(max(x, 1), a.w - 2), yc = min(max(y, 1), a.h - 2);
    const float* e = a.eig + (size_t)yc * a.w + xc;
    float nv[9];
#pragma unroll
    for (int j = -1; j <= 1; j++)
#pragma unroll
        for (int i = -1; i <= 1; i++) nv[(j + 1) * 3 + (i + 1)] = e[j * a.w + i];
    const uint8_t mk = a.mask ? a.mask[(size_t)yc * a.w + xc] : (uint8_t)1;
    if (x < 1 || y < 1 || x >= a.w - 1 || y >= a.h - 1) return false;
    const float val = nv[4];
    if (!(val > thr) || val == 0.f || !mk) return false;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 9; k++) ok = ok && !(nv[k] > thr && nv[k] > val);
    return ok;
}

constexpr int CAND_TILE = 1024;
template <int N>
__global__ __launch_bounds__(256) void gftt_count_kernel(TBatch<GfttArgs, N> B_)
{
    const GfttArgs& a = slot_args(B_);
    if ((int)blockIdx.x >= a.nblk) return;
    __shared__ unsigned smax[4];
    const float thr = gftt_threshold(a, smax);
    const int base = blockIdx.x * CAND_TILE;
    int c = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) { const int p = base + threadIdx.x * 4 + j; if (p < a.w * a.h && gftt_is_cand(a, p % a.w, p / a.w, thr)) c++; }
    __shared__ int ws[8];
    int tot;
    block_excl_scan<256>(c, ws, &tot);
    if (threadIdx.x == 0) a.blockCnt[blockIdx.x] = tot;
}
// ordered compaction; the prefix over the (<= a few thousand) per-tile counts is folded by every workgroup itself (the one-workgroup
// scan launch in between was 4.8 us of the node's frame)
template <int N>
__global__ __launch_bounds__(256) void gftt_emit_kernel(TBatch<GfttArgs, N> B_)
{
    const GfttArgs& a = slot_args(B_);
    if ((int)blockIdx.x >= a.nblk) return;
    const float thr = *a.thr;
    __shared__ int ws[8];
    int bef = 0, all = 0;
    for (int i = threadIdx.x; i < a.nblk; i += 256) { const int v = a.blockCnt[i]; all += v; bef += i < (int)blockIdx.x ? v : 0; }
    int total, before;
    (void)block_excl_scan<256>(all, ws, &total);
    (void)block_excl_scan<256>(bef, ws, &before);
    if (blockIdx.x == 0 && threadIdx.x == 0) { *a.total = total; a.d_n[0] = total; a.d_nbits[0] = 32; }
    const int base = blockIdx.x * CAND_TILE;
    bool h[4]; int c = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) { const int p = base + threadIdx.x * 4 + j; h[j] = (p < a.w * a.h) && gftt_is_cand(a, p % a.w, p / a.w, thr); c += h[j]; }
    int r = before + block_excl_scan<256>(c, ws, nullptr);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (!h[j]) continue;
        const int p = base + threadIdx.x * 4 + j;
        // emit in DESCENDING address order: the stable sort by value then keeps "higher address first" among ties
        const int pos = total - 1 - r++;
        a.keysA[pos] = ~__float_as_uint(a.eig[p]);          // eig > 0 here: ascending ~bits = descending value
        a.valsA[pos] = (unsigned)p;
    }
}

struct PickArgs {
    const unsigned *keysA;
    const unsigned *valsA, *valsB; const int* d_nbits; const int* total;
    int w, h, max_corners, cap; double min_dist;
    float* out_xy; int* out_n; int* ncand;
    long long* dbg;                  // [8] phase stamps of the LDS form (diagnostics; may be null)
};

// sequential minimum-distance selection (featureselect.cpp), one wavefront, ballot-resolved.  A candidate is compared with
// the accepted corners of the 3 x 3 grid cells around it (cell = min_dist, as OpenCV's own grid): the cells keep up to four
// accepted indices each in LDS (corners at least min_dist apart: two fit a cell), so a candidate reads a handful of entries
// instead of walking all accepted corners; a fifth corner in one cell, or a grid beyond the LDS budget, falls back to that walk.
// SORTLDS = false: the candidates arrive sorted (12-launch radix sort), one wavefront picks.
// SORTLDS = true: ONE workgroup of 1024 threads.  The greedy pick consumes candidates in descending value order and stops at the
// quota (MAX_CNT - tracked: tens of corners), so only the strongest few thousand are ever looked at: the workgroup takes a
// 1024-bin histogram of the values, cuts a band of at most GFTT_BAND candidates off its top, sorts THAT band in LDS (bitonic;
// keys = ~value bits, then ~address: descending value, higher address first among equal values — cv::goodFeaturesToTrack's
// greaterThanPtr order — and unique), lets its first wavefront pick from it, and goes on to the next band only if the quota is
// not met.  One launch instead of thirteen; any number of candidates.  A value bin that alone exceeds the band (thousands of
// exactly equal values) or an accepted list beyond the LDS tables reports -2: the host runs the radix form for that frame.
constexpr int GFTT_BAND = 1024;                   // one candidate per thread: the band is ordered by counting, for every key, the keys below it
template <bool SORTLDS>
__device__ __forceinline__ void gftt_pick_body(const PickArgs& a)
{
    constexpr int ACC_MAX = SORTLDS ? 2048 : 4096, GRID_MAX = SORTLDS ? 4096 : 8192, CELL_CAP = 4;
    constexpr int NT = SORTLDS ? 1024 : 64;
    __shared__ short ax[ACC_MAX], ay[ACC_MAX], acx[ACC_MAX], acy[ACC_MAX];      // accepted corners and their grid cells (no division in the inner loop)
    __shared__ unsigned gcnt[GRID_MAX];                                          // (words: the accepted corners of a batch enter their cells together, through atomics)
    __shared__ unsigned short gent[GRID_MAX * CELL_CAP];
    __shared__ unsigned long long band[SORTLDS ? GFTT_BAND : 1];
    __shared__ unsigned hist[SORTLDS ? 1024 : 1], hsub[SORTLDS ? 8 * 1024 : 1];      // hsub: eight copies (lane & 7) — weak candidates crowd the last bins
    __shared__ int ws[NT / 64 + 1];
    __shared__ unsigned s_kmin, s_kmax;
    __shared__ int s_lo, s_hi, s_state;                   // the band's bin range [lo, hi); 0 = go on | 1 = finished | 2 = redo in the radix form
    const int total = *a.total;
    const unsigned* vals = rs_result_in_B(a.d_nbits[0]) ? a.valsB : a.valsA;
    const int l = threadIdx.x;
    if (l == 0) { *a.ncand = total; s_state = 0; s_lo = 0; s_hi = 0; s_kmin = 0xFFFFFFFFu; s_kmax = 0u; }
    const bool filter = a.min_dist >= 1.0;
    const int cell = filter ? (int)rint(a.min_dist) : 1;
    const double md2 = a.min_dist * a.min_dist;
    const int gw = (a.w + cell - 1) / cell, gh = (a.h + cell - 1) / cell;
    bool grid = filter && gw * gh <= GRID_MAX;
    if (grid) for (int c = l; c < gw * gh; c += NT) gcnt[c] = 0;
    if (SORTLDS) for (int b = l; b < 8 * 1024; b += NT) hsub[b] = 0u;
    __syncthreads();
    int shift = 0;
    constexpr int KPT = SORTLDS ? 16 : 1;
    unsigned kreg[KPT];
    long long tq[6] = {0, 0, 0, 0, 0, 0}; int nbands = 0;
    if (SORTLDS && l == 0) tq[0] = clock64();
    if (SORTLDS) {
        // range of the value keys, then the histogram (keys ascend as values descend: bin 0 holds the strongest)
        // (the first KPT keys of a thread stay in registers for all three passes — range, histogram, band placement; one round of
        // loads, all in flight together: 14 k candidates were 14 dependent round trips per pass)
        unsigned kmn = 0xFFFFFFFFu, kmx = 0u;
#pragma unroll
        for (int j = 0; j < KPT; j++) kreg[j] = a.keysA[min(l + j * NT, max(total - 1, 0))];
#pragma unroll
        for (int j = 0; j < KPT; j++) if (l + j * NT < total) { kmn = min(kmn, kreg[j]); kmx = max(kmx, kreg[j]); }
        for (int i = l + KPT * NT; i < total; i += NT) { const unsigned k = a.keysA[i]; kmn = min(kmn, k); kmx = max(kmx, k); }
        atomicMin(&s_kmin, kmn); atomicMax(&s_kmax, kmx);
        __syncthreads();
        while (((s_kmax - s_kmin) >> shift) >= 1024u) shift++;
#pragma unroll
        for (int j = 0; j < KPT; j++) if (l + j * NT < total) atomicAdd(&hsub[(l & 7) * 1024 + ((kreg[j] - s_kmin) >> shift)], 1u);
        for (int i = l + KPT * NT; i < total; i += NT) atomicAdd(&hsub[(l & 7) * 1024 + ((a.keysA[i] - s_kmin) >> shift)], 1u);
        __syncthreads();
        { unsigned v = 0u;
#pragma unroll
          for (int c = 0; c < 8; c++) v += hsub[c * 1024 + l];
          // inclusive prefix over the bins (thread = bin): hist[b] = candidates in bins 0 .. b
          int tot; const int ex = block_excl_scan<1024>((int)v, ws, &tot); hist[l] = (unsigned)ex + v; }
        __syncthreads();
        if (l == 0) tq[1] = clock64();
    }
    int nacc = 0;
    // one corner past the capacity is enough to know the result does not fit (it is counted, not stored)
    const int limit = (a.max_corners > 0) ? min(a.max_corners, a.cap + 1) : a.cap + 1;
    bool overflow = false;
    for (;;) {
        int count = total;                                   // the radix form: one "band" = every candidate, already in order
        if (SORTLDS) {
            // the next band: bins [lo, hi) with at most GFTT_BAND candidates, at least one bin (thread = bin, hist = inclusive prefix)
            {
                const int lo = s_hi;                              // (read by every thread before thread 0 rewrites it below the barrier)
                const unsigned before = lo > 0 ? hist[lo - 1] : 0u;
                const bool fits = l >= lo && hist[l] - before <= (unsigned)GFTT_BAND;
                const unsigned long long mk = __ballot(fits);     // bins are monotone: the fitting ones form a prefix of [lo, 1024)
                if ((l & 63) == 0) ws[l >> 6] = __popcll(mk);
                __syncthreads();
                if (l == 0) {
                    int nfit = 0;
                    for (int q = 0; q < NT / 64; q++) nfit += ws[q];
                    int hi = lo + nfit;
                    if (total == 0 || lo >= 1024) s_state = 1;
                    else if (nfit == 0) { hi = lo + 1; s_state = 2; }     // one bin of (nearly) equal values is larger than the band
                    s_lo = lo; s_hi = hi;
                }
            }
            __syncthreads();
            if (s_state) break;
            const unsigned lo = (unsigned)s_lo, hi = (unsigned)s_hi;
            const unsigned before = lo > 0 ? hist[lo - 1] : 0u;      // candidates in the bins above this band's
            if (l == 0) tq[2] -= clock64();
            nbands += l == 0 ? 1 : 0;
            // counting sort by bin (the bins ARE value order): a key goes to its bin's segment of the band, any place inside it …
            for (unsigned b = lo + (unsigned)l; b < hi; b += NT) hsub[b] = 0u;          // (hsub[0 .. 1024) serves as the bins' cursors now)
            __syncthreads();
            auto place = [&](unsigned k, int i) {
                const unsigned b = (k - s_kmin) >> shift;
                if (b >= lo && b < hi) {
                    const unsigned seg = (b > 0 ? hist[b - 1] : 0u) - before;
                    band[seg + atomicAdd(&hsub[b], 1u)] = ((unsigned long long)k << 32) | (unsigned long long)(0xFFFFFFFFu - a.valsA[i]);
                }
            };
#pragma unroll
            for (int j = 0; j < KPT; j++) if (l + j * NT < total) place(kreg[j], l + j * NT);
            for (int i = l + KPT * NT; i < total; i += NT) place(a.keysA[i], i);
            __syncthreads();
            count = (int)(hist[hi - 1] - before);
            {   // … and is then ranked among the few keys of its own bin (unique keys: the count of smaller ones is its place)
                unsigned long long mine = ~0ull; int place = 0;
                if (l < count) {
                    mine = band[l];
                    const unsigned b = ((unsigned)(mine >> 32) - s_kmin) >> shift;
                    const int s0 = (int)((b > 0 ? hist[b - 1] : 0u) - before), s1 = (int)(hist[b] - before);
                    int r = 0;
                    for (int j = s0; j < s1; j++) r += band[j] < mine ? 1 : 0;
                    place = s0 + r;
                }
                __syncthreads();
                if (l < count) band[place] = mine;
                __syncthreads();
            }
            if (l == 0) { const long long t = clock64(); tq[2] += t; tq[3] -= t; }
        }
        if (l < 64) {
            auto cand = [&](int i) -> unsigned { return SORTLDS ? 0xFFFFFFFFu - (unsigned)band[i] : vals[i]; };
            unsigned pnext = l < count ? cand(l) : 0u;       // the next batch's candidates are in flight while this one is resolved
            for (int base = 0; base < count && nacc < limit; base += 64) {
                const int i = base + l;
                bool alive = i < count;
                int x = 0, y = 0;
                const int p = (int)pnext;
                pnext = i + 64 < count ? cand(i + 64) : 0u;
                if (alive) { y = p / a.w; x = p - y * a.w; }
                const int xc = x / cell, yc = y / cell;
                if (alive && filter) {
                    if (grid) {
                        for (int dyc = -1; dyc <= 1 && alive; dyc++) {
                            const int cy = yc + dyc;
                            if (cy < 0 || cy >= gh) continue;
                            for (int dxc = -1; dxc <= 1 && alive; dxc++) {
                                const int cx = xc + dxc;
                                if (cx < 0 || cx >= gw) continue;
                                const int c = cy * gw + cx, n = min((int)gcnt[c], CELL_CAP);
                                for (int e = 0; e < n; e++) {
                                    const int k = gent[c * CELL_CAP + e];
                                    const float dx = (float)(x - ax[k]), dy = (float)(y - ay[k]);
                                    if ((double)(dx * dx + dy * dy) < md2) { alive = false; break; }
                                }
                            }
                        }
                    } else {
                        for (int k = 0; k < nacc; k++) {
                            const int dxc = acx[k] - xc, dyc = acy[k] - yc;
                            if (dxc < -1 || dxc > 1 || dyc < -1 || dyc > 1) continue;
                            const float dx = (float)(x - ax[k]), dy = (float)(y - ay[k]);
                            if ((double)(dx * dx + dy * dy) < md2) { alive = false; break; }
                        }
                    }
                }
                // accept rounds in registers: the strongest surviving lane is accepted, the lanes within min_dist of it drop out (a corner
                // that close always lies in a neighbouring cell, so the plain distance test equals the grid's) — no LDS inside the loop
                // (a table update per round was ~1 000 cycles: 68 us for 150 corners)
                uint64_t m = __ballot(alive), accm = 0ull;
                const int nacc0 = nacc;
                while (m && nacc < limit) {
                    const int first = __ffsll((long long)m) - 1;
                    const int fx = __builtin_amdgcn_readlane(x, first), fy = __builtin_amdgcn_readlane(y, first);      // `first` is wave-uniform: scalar reads
                    accm |= 1ull << first;
                    nacc++;
                    if (l == first) alive = false;
                    if (alive && filter) {
                        const float dx = (float)(x - fx), dy = (float)(y - fy);
                        if ((double)(dx * dx + dy * dy) < md2) alive = false;
                    }
                    m = __ballot(alive);
                    if (nacc >= ACC_MAX && filter) { overflow = true; break; }
                }
                // … then the batch's accepted corners enter the tables together (their order inside a cell does not matter)
                bool full = false;
                if ((accm >> l) & 1ull) {
                    const int k = nacc0 + __popcll(accm & ((1ull << l) - 1ull));
                    if (k < ACC_MAX) { ax[k] = (short)x; ay[k] = (short)y; acx[k] = (short)xc; acy[k] = (short)yc; }
                    if (k < a.cap) { a.out_xy[2 * k] = (float)x; a.out_xy[2 * k + 1] = (float)y; }
                    if (grid) {
                        const int c = yc * gw + xc;
                        const unsigned n = k < ACC_MAX ? atomicAdd(&gcnt[c], 1u) : (unsigned)CELL_CAP;
                        if (n < (unsigned)CELL_CAP) gent[c * CELL_CAP + n] = (unsigned short)k;
                        else full = true;
                    }
                }
                if (__ballot(full)) grid = false;                   // a fifth corner in one cell: from here on the walk over all accepted corners
                if (overflow) break;
                __threadfence_block(); __builtin_amdgcn_wave_barrier();      // one wavefront: its LDS operations complete in order
            }
            if (SORTLDS && l == 0) tq[3] += clock64();
            if (SORTLDS && l == 0 && (overflow || nacc >= limit)) s_state = overflow ? 2 : 1;
        }
        if (!SORTLDS) break;
        __syncthreads();
        if (s_state) break;
    }
    if (l == 0) *a.out_n = SORTLDS ? (s_state == 2 ? -2 : nacc) : (overflow ? -1 : nacc);
    if (SORTLDS && l == 0 && a.dbg) { a.dbg[0] = tq[1] - tq[0]; a.dbg[1] = tq[2]; a.dbg[2] = tq[3]; a.dbg[3] = clock64() - tq[0]; a.dbg[4] = nbands; a.dbg[5] = total; a.dbg[6] = nacc; }
}
// the radix form: one slot per launch by design (the sort in front of it is per slot)
__global__ __launch_bounds__(64) void gftt_pick_kernel(PickArgs a) { gftt_pick_body<false>(a); }
LVI_TBATCH_FITS(PickArgs);
// the LDS form: one 1024-thread workgroup per slot, each on its own CU (its ~108 KB of LDS leave room for one)
template <int N>
__global__ __launch_bounds__(1024) void gftt_sortpick_kernel(TBatch<PickArgs, N> B_)
{
    const PickArgs& a = slot_args(B_);
    if (N > 1 && !a.total) return;     // (a set of one launches this kernel only for its slot)
    gftt_pick_body<true>(a);
}

}  // namespace

}  // namespace lvi

using namespace lvi;

constexpr int CLAHE_MAX_TILES = 64;

struct lvi_tracker {
    lvi_tracker_params P;
    int device = 0;
    Ctx ctx; Profiler prof; Arena arena;
    Pyr pyr[2];                 // [cur, forw]
    int cur = 0, forw = 1;
    int w = 0, h = 0;
    bool have_forw = false, have_cur = false, have_lk = false, have_gftt = false, have_mask = false;
    uint8_t* d_stage = nullptr;
    float *d_cur_xy = nullptr, *d_forw_xy = nullptr, *d_err = nullptr; uint8_t* d_status = nullptr; int n_pts = 0;
    uint8_t* d_mask = nullptr; float* d_eig = nullptr; unsigned* d_maxord = nullptr; unsigned* d_maxPartial = nullptr; float* d_thr = nullptr;
    int *d_blockCnt = nullptr, *d_total = nullptr, *d_n = nullptr, *d_nbits = nullptr, *d_out_n = nullptr, *d_ncand = nullptr;
    float* d_gftt_xy = nullptr;
    SortPlan sort;
    int gftt_n = 0, gftt_ncand = 0;
    bool gftt_force_radix = false;     // LVI_GFTT_RADIX=1 at create: always the 12-launch radix sort + one-wavefront pick (tests: same corners)
    bool gftt_pending = false; int gftt_pending_max = 0;       // lvi_tracker_run_gftt_async enqueued, result not fetched yet
    float* d_centers = nullptr; float* h_centers[2] = {nullptr, nullptr}; hipEvent_t ev_centers[2] = {nullptr, nullptr}; int centers_slot = 0;
    float* d_frame_out = nullptr;      // [4 + 2 F + 2 F] one block: {n_new, n_cand, n_all, 0}, the new corners, the undistorted points of [kept ; new]
    float* h_frame_out = nullptr;      // pinned mirror
    float* d_all_xy = nullptr;         // [2 F] kept ++ new
    long long* d_dbg = nullptr;        // [8] phase stamps of gftt_sortpick (LVI_TDBG_SORTPICK_CYCLES)
    // f-2 / f-3
    uint8_t *d_eq = nullptr, *d_lut = nullptr; float *d_un_in = nullptr, *d_un_out = nullptr;
    bool equalize = false; double clahe_clip = 3.0; int clahe_tx = 8, clahe_ty = 8;
    // pinned staging for incoming frames: the caller's (pageable) image is copied here on the host and goes to the
    // device from pinned memory — measured: the runtime's own handling of a pageable 0.9 MB source costs up to 1 ms per
    // frame in a process with many GPU mappings, and the call had to wait for it before returning
    uint8_t* h_frame[2] = {nullptr, nullptr}; hipEvent_t ev_frame[2] = {nullptr, nullptr}; int frame_slot = 0;
    float* h_pts[2] = {nullptr, nullptr}; hipEvent_t ev_pts[2] = {nullptr, nullptr}; int pts_slot = 0;      // the same for cur_pts (set_points only)
    float* h_kept[2] = {nullptr, nullptr}; hipEvent_t ev_kept[2] = {nullptr, nullptr}; int kept_slot = 0;   // the kept points of finish_frame: a pair of
                                                                                                           // its own, so it never overwrites run_lk's points
    // Small inputs and results do not travel through copy commands (a 1 KB hipMemcpyAsync is a 4 us blit kernel on the stream, and the node
    // path had eleven of them per frame): kernels read the caller's points / circle centres in place from the pinned slots above and
    // write the LK results and the frame's result block into pinned host memory; the host waits once and reads.
    const float* cur_src = nullptr; int cur_slot = -1;       // points of the next run_lk (a pinned slot; its event is recorded behind the kernel that reads it)
    float* h_lk = nullptr;                                   // [2 F] forw_xy, [F] err, [F bytes] status
};

namespace {

template <class AR>
void tracker_layout(AR& ar, lvi_tracker& t)
{
    const int W = t.P.max_width, H = t.P.max_height;
    for (int s = 0; s < 2; s++) {
        int w = W, h = H;
        for (int l = 0; l <= t.P.lk_max_level; l++) {
            t.pyr[s].lv[l].px = ar.template alloc<uint8_t>((size_t)w * h);
            w = (w + 1) / 2; h = (h + 1) / 2;
        }
    }
    const int F = std::max(t.P.max_features, 64);
    t.d_cur_xy = ar.template alloc<float>(2 * (size_t)F); t.d_forw_xy = ar.template alloc<float>(2 * (size_t)F);
    t.d_err = ar.template alloc<float>(F); t.d_status = ar.template alloc<uint8_t>(F);
    t.d_mask = ar.template alloc<uint8_t>((size_t)W * H); t.d_eig = ar.template alloc<float>((size_t)W * H);
    t.d_maxord = ar.template alloc<unsigned>(1); t.d_thr = ar.template alloc<float>(1);
    t.d_maxPartial = ar.template alloc<unsigned>((size_t)div_up(W, 32) * div_up(H, 8));
    t.d_blockCnt = ar.template alloc<int>(div_up(W * H, CAND_TILE) + 1);
    t.d_total = ar.template alloc<int>(1); t.d_n = ar.template alloc<int>(1); t.d_nbits = ar.template alloc<int>(1);
    t.d_out_n = ar.template alloc<int>(1); t.d_ncand = ar.template alloc<int>(1);
    t.d_gftt_xy = ar.template alloc<float>(2 * (size_t)F);
    t.sort.allocate(ar, 1, W * H, RS_ITEMS_SMALL);
    t.d_stage = ar.template alloc<uint8_t>((size_t)W * H); t.d_eq = ar.template alloc<uint8_t>((size_t)W * H);
    t.d_lut = ar.template alloc<uint8_t>((size_t)CLAHE_MAX_TILES * CLAHE_MAX_TILES * 256);
    t.d_un_in = ar.template alloc<float>(2 * (size_t)F); t.d_un_out = ar.template alloc<float>(2 * (size_t)F);
    t.d_centers = ar.template alloc<float>(2 * (size_t)F); t.d_all_xy = ar.template alloc<float>(2 * (size_t)F);
    t.d_frame_out = ar.template alloc<float>(4 + 4 * (size_t)F);
    t.d_dbg = ar.template alloc<long long>(8);
}

// A set of tracker states that every stage serves with ONE launch (the image side's counterpart of lvi_lidar.hpp's Slots): the
// slots of an lvi_tbatch, or a single handle as a set of one.  c: the stream and the profiler the set's launches go through.
struct TSlots {
    const Ctx& c; lvi_tracker* t; int n;             // t[0 .. n), n = 1 .. LVI_TRACKER_MAX_BATCH
    lvi_tracker& operator[](int s) const { return t[s]; }
    TSlots one(int s) const { return TSlots{c, t + s, 1}; }
    template <class T>
    void launch(const char* name, double bytes, void (*k1)(TBatch<T, 1>), void (*kn)(TBatch<T>), dim3 grid, int threads, const TBatch<T>& B) const
    {
        grid.z = (unsigned)n;
        if (n == 1) {
            const TBatch<T, 1> B1{{B.a[0]}};
            LVI_LAUNCH(c, name, bytes, hipLaunchKernelGGL(k1, grid, dim3(threads), 0, c.stream, B1));
        } else {
            LVI_LAUNCH(c, name, bytes, hipLaunchKernelGGL(kn, grid, dim3(threads), 0, c.stream, B));
        }
    }
};
// one launch of a kernel entry for the set S: its one-block instantiation for a set of one slot
#define LVI_TLAUNCH(S, name, bytes, kernel, grid, threads, B) (S).launch(name, bytes, kernel<1>, kernel<LVI_TRACKER_MAX_BATCH>, grid, threads, B)
const bool TAKE_ALL[LVI_TRACKER_MAX_BATCH] = {true, true, true, true, true, true, true, true};
static_assert(LVI_TRACKER_MAX_BATCH == 8, "TAKE_ALL names every slot");

// the pinned double slots: the other buffer of the pair, free once the command that read it two uses ago is through.  The caller
// fills it and records ev[slot] behind the command that reads it.
template <class T>
T* pinned_next(T* const (&h)[2], const hipEvent_t (&ev)[2], int& slot)
{
    slot ^= 1;
    LVI_HIP(hipEventSynchronize(ev[slot]));
    return h[slot];
}

// src (w x h, dense) → dst equalised; both device buffers of the handle
ClaheArgs clahe_args(lvi_tracker& t, const uint8_t* src, uint8_t* dst, int w, int h, double clip, int tilesX, int tilesY)
{
    int extW = w, extH = h;
    if (w % tilesX != 0 || h % tilesY != 0) { extW = w + (tilesX - (w % tilesX)); extH = h + (tilesY - (h % tilesY)); }   // copyMakeBorder quirk: both sides grow
    ClaheArgs a{};
    a.src = src; a.dst = dst; a.lut = t.d_lut; a.W = w; a.H = h; a.tilesX = tilesX; a.tilesY = tilesY;
    a.tw = extW / tilesX; a.th = extH / tilesY;
    const int area = a.tw * a.th;
    a.lutScale = static_cast<float>(255) / area;
    a.clipLimit = 0;
    if (clip > 0.0) a.clipLimit = std::max(static_cast<int>(clip * area / 256), 1);
    return a;
}
// the filled blocks of B are w x h images with one tile grid
void run_clahe(const TSlots& S, const TBatch<ClaheArgs>& B, int ntile, int w, int h, double px)
{
    LVI_TLAUNCH(S, "clahe_lut", px, clahe_lut_kernel, dim3(ntile), 1024, B);
    LVI_TLAUNCH(S, "clahe_interp", 2.0 * px, clahe_interp_kernel, dim3(div_up(w, 64), div_up(h, 4)), 256, B);
}

// the levels of the pyramid of a w x h image (buildOpticalFlowPyramid's early return included), without the launches
void plan_pyramid(Pyr& p, int w, int h, const lvi_tracker_params& P)
{
    p.lv[0].w = w; p.lv[0].h = h;
    p.top = P.lk_max_level;
    for (int level = 0; level <= P.lk_max_level; level++) {
        if (level != 0) { p.lv[level].w = (p.lv[level - 1].w + 1) / 2; p.lv[level].h = (p.lv[level - 1].h + 1) / 2; }
        w = (w + 1) / 2; h = (h + 1) / 2;
        if (w <= P.lk_win || h <= P.lk_win) { p.top = level; break; }
    }
}
// the pyramids of the slots of `take` over their level-0 images: one launch per level; a slot whose pyramid ends early has a zeroed
// block in the deeper launches
void build_pyramids(const TSlots& S, const bool* take, bool cur_side)
{
    int maxtop = 0;
    for (int s = 0; s < S.n; s++) {
        if (!take[s]) continue;
        lvi_tracker& t = S[s];
        Pyr& p = t.pyr[cur_side ? t.cur : t.forw];
        plan_pyramid(p, t.w, t.h, t.P);
        maxtop = std::max(maxtop, p.top);
    }
    for (int level = 1; level <= maxtop; level++) {
        TBatch<PyrArgs> B{};
        int gx = 0, gy = 0; double bytes = 0;
        for (int s = 0; s < S.n; s++) {
            if (!take[s]) continue;
            lvi_tracker& t = S[s];
            const Pyr& p = t.pyr[cur_side ? t.cur : t.forw];
            if (level > p.top) continue;
            B.a[s] = PyrArgs{p.lv[level - 1].px, p.lv[level].px, p.lv[level - 1].w, p.lv[level - 1].h, p.lv[level].w, p.lv[level].h};
            gx = std::max(gx, div_up(p.lv[level].w, 32)); gy = std::max(gy, div_up(p.lv[level].h, 8));
            bytes += (double)p.lv[level - 1].w * p.lv[level - 1].h + (double)p.lv[level].w * p.lv[level].h;
        }
        LVI_TLAUNCH(S, "pyrdown", bytes, pyrdown_kernel, dim3(gx, gy), 256, B);
    }
}

int32_t check_tracker_params(const lvi_tracker_params* p)
{
    if (p->lk_win < 3 || (p->lk_win & 1) == 0 || p->lk_win > LK_WIN_MAX || p->lk_max_level < 0 || p->lk_max_level >= MAX_LEVELS)
        return fail(LVI_ERR_INVALID_ARG, "bad LK parameters (odd window <= 21, maxLevel 0..7)");
    if (p->max_width <= 0 || p->max_height <= 0 || p->max_features <= 0 || p->max_features > 4096) return fail(LVI_ERR_INVALID_ARG, "bad capacities");
    return LVI_OK;
}

// the pinned staging buffers of one tracker state, their events recorded on its stream
void tracker_host_alloc(lvi_tracker* t)
{
    for (int s = 0; s < 2; s++) {
        LVI_HIP(hipHostMalloc((void**)&t->h_frame[s], (size_t)t->P.max_width * t->P.max_height, hipHostMallocDefault));
        LVI_HIP(hipEventCreateWithFlags(&t->ev_frame[s], hipEventDisableTiming));
        LVI_HIP(hipEventRecord(t->ev_frame[s], t->ctx.stream));
        LVI_HIP(hipHostMalloc((void**)&t->h_centers[s], sizeof(float) * 2 * (size_t)std::max(t->P.max_features, 64), hipHostMallocDefault));
        LVI_HIP(hipEventCreateWithFlags(&t->ev_centers[s], hipEventDisableTiming));
        LVI_HIP(hipEventRecord(t->ev_centers[s], t->ctx.stream));
        LVI_HIP(hipHostMalloc((void**)&t->h_pts[s], sizeof(float) * 2 * (size_t)std::max(t->P.max_features, 64), hipHostMallocDefault));
        LVI_HIP(hipEventCreateWithFlags(&t->ev_pts[s], hipEventDisableTiming));
        LVI_HIP(hipEventRecord(t->ev_pts[s], t->ctx.stream));
        LVI_HIP(hipHostMalloc((void**)&t->h_kept[s], sizeof(float) * 2 * (size_t)std::max(t->P.max_features, 64), hipHostMallocDefault));
        LVI_HIP(hipEventCreateWithFlags(&t->ev_kept[s], hipEventDisableTiming));
        LVI_HIP(hipEventRecord(t->ev_kept[s], t->ctx.stream));
    }
    LVI_HIP(hipHostMalloc((void**)&t->h_frame_out, sizeof(float) * (4 + 4 * (size_t)std::max(t->P.max_features, 64)), hipHostMallocDefault));
    LVI_HIP(hipHostMalloc((void**)&t->h_lk, sizeof(float) * 4 * (size_t)std::max(t->P.max_features, 64), hipHostMallocDefault));
}
void tracker_host_free(lvi_tracker* t)
{
    for (int s = 0; s < 2; s++) {
        if (t->h_frame[s]) (void)hipHostFree(t->h_frame[s]);
        if (t->ev_frame[s]) (void)hipEventDestroy(t->ev_frame[s]);
        if (t->h_pts[s]) (void)hipHostFree(t->h_pts[s]);
        if (t->h_centers[s]) (void)hipHostFree(t->h_centers[s]);
        if (t->ev_centers[s]) (void)hipEventDestroy(t->ev_centers[s]);
        if (t->ev_pts[s]) (void)hipEventDestroy(t->ev_pts[s]);
        if (t->h_kept[s]) (void)hipHostFree(t->h_kept[s]);
        if (t->ev_kept[s]) (void)hipEventDestroy(t->ev_kept[s]);
    }
    if (t->h_frame_out) (void)hipHostFree(t->h_frame_out);
    if (t->h_lk) (void)hipHostFree(t->h_lk);
}

// ---------------------------------------------------------------------------------------------
// The stages.  Each is written once, for a set of slots; the entry points below check their arguments and hand over a set of one
// (lvi_tracker_*) or of S (lvi_tbatch_*) slots.  A slot that sits a call out is skipped by its mask or its negative count.
// ---------------------------------------------------------------------------------------------
// one image per slot of `take`: staging copy, optional CLAHE, the forw pyramid; a slot's first image (or a new size) is its cur image too
void stage_push(const TSlots& S, const uint8_t* const* imgs, const bool* take, int w, int h, int stride)
{
    bool first[LVI_TRACKER_MAX_BATCH] = {}, any_first = false;
    for (int s = 0; s < S.n; s++) {
        if (!take[s]) continue;
        lvi_tracker& t = S[s];
        if (t.have_forw && (w != t.w || h != t.h)) { t.have_forw = t.have_cur = false; }
        if (t.have_forw) { std::swap(t.cur, t.forw); t.have_cur = true; }     // cur_img = forw_img (:203), this slot's own rotation
        first[s] = !t.have_forw; any_first = any_first || first[s];
        t.w = w; t.h = h;
        uint8_t* stage = pinned_next(t.h_frame, t.ev_frame, t.frame_slot);    // (waits for the copy that used this buffer two frames ago)
        for (int y = 0; y < h; y++) std::memcpy(stage + (size_t)y * w, imgs[s] + (size_t)y * stride, (size_t)w);
        uint8_t* dst0 = t.equalize ? t.d_stage : t.pyr[t.forw].lv[0].px;
        LVI_HIP(hipMemcpyAsync(dst0, stage, (size_t)w * h, hipMemcpyHostToDevice, S.c.stream));
        LVI_HIP(hipEventRecord(t.ev_frame[t.frame_slot], S.c.stream));
    }
    if (S[0].equalize) {                                                       // readImage's EQUALIZE branch (:86-90), all slots alike
        TBatch<ClaheArgs> B{};
        int ntile = 0; double px = 0;
        for (int s = 0; s < S.n; s++) {
            if (!take[s]) continue;
            lvi_tracker& t = S[s];
            B.a[s] = clahe_args(t, t.d_stage, t.pyr[t.forw].lv[0].px, w, h, t.clahe_clip, t.clahe_tx, t.clahe_ty);
            ntile = B.a[s].tilesX * B.a[s].tilesY; px += (double)w * h;
        }
        run_clahe(S, B, ntile, w, h, px);
    }
    build_pyramids(S, take, false);
    if (any_first) {                                                           // prev = cur = forw = img (:94-97)
        for (int s = 0; s < S.n; s++) {
            if (!first[s]) continue;
            lvi_tracker& t = S[s];
            LVI_HIP(hipMemcpyAsync(t.pyr[t.cur].lv[0].px, t.pyr[t.forw].lv[0].px, (size_t)w * h, hipMemcpyDeviceToDevice, S.c.stream));
        }
        build_pyramids(S, first, true);
    }
    // no stream sync: the caller's buffers were consumed by the host copies above
    for (int s = 0; s < S.n; s++) {
        if (!take[s]) continue;
        lvi_tracker& t = S[s];
        if (first[s]) t.have_cur = true;
        t.have_forw = true; t.have_lk = false; t.have_gftt = false;
    }
}

void stage_set_points(const TSlots& S, const float* const* cur_xy, const int32_t* n)
{
    for (int s = 0; s < S.n; s++) {
        if (n[s] < 0) continue;
        lvi_tracker& t = S[s];
        if (n[s]) {
            float* dst = pinned_next(t.h_pts, t.ev_pts, t.pts_slot);
            std::memcpy(dst, cur_xy[s], sizeof(float) * 2 * (size_t)n[s]);
            t.cur_src = dst; t.cur_slot = t.pts_slot;                          // lk_kernel reads them in place
        }
        t.n_pts = n[s]; t.have_lk = false;
    }
}

// LK for the slots of `take`, each from its last set_points; true if a kernel was launched
bool stage_run_lk(const TSlots& S, const bool* take)
{
    TBatch<LkArgs> B{};
    int nmax = 0; double bytes = 0;
    for (int s = 0; s < S.n; s++) {
        if (!take[s]) continue;
        lvi_tracker& t = S[s];
        LkArgs& a = B.a[s];
        a.prev = t.pyr[t.cur]; a.next = t.pyr[t.forw];
        const size_t F = (size_t)std::max(t.P.max_features, 64);
        a.prev_xy = t.cur_src ? t.cur_src : t.d_cur_xy; a.next_xy = t.d_forw_xy; a.status = t.d_status; a.err = t.d_err;
        a.h_next_xy = t.h_lk; a.h_err = t.h_lk + 2 * F; a.h_status = reinterpret_cast<uint8_t*>(t.h_lk + 3 * F);
        a.n = t.n_pts; a.win = t.P.lk_win; a.max_level = std::min(a.prev.top, a.next.top);
        a.max_count = std::min(std::max(t.P.lk_max_iters, 0), 100);
        const double eps = std::min(std::max(t.P.lk_eps, 0.), 10.);
        a.epsilon = eps * eps; a.min_eig = t.P.lk_min_eig_threshold;
        nmax = std::max(nmax, a.n);
        bytes += (double)a.n * (a.max_level + 1) * (24.0 * 24 + 22.0 * 22 * 4);
    }
    if (nmax > 0) {
        LVI_TLAUNCH(S, "lk_track", bytes, lk_kernel, dim3(nmax), 64, B);
        for (int s = 0; s < S.n; s++) {
            lvi_tracker& t = S[s];                                             // the points' slot is free again once this kernel has read it
            if (take[s] && t.n_pts > 0 && t.cur_slot >= 0) LVI_HIP(hipEventRecord(t.ev_pts[t.cur_slot], S.c.stream));
        }
    }
    for (int s = 0; s < S.n; s++) if (take[s]) S[s].have_lk = true;
    return nmax > 0;
}

// the results lk_kernel wrote into the slot's pinned block; wait: the stream has not been waited for since run_lk
int32_t get_lk(const Ctx& c, lvi_tracker* t, bool wait, float* forw_xy, uint8_t* status, float* err, int32_t capacity, int32_t* n)
{
    if (!t->have_lk) return fail(LVI_ERR_STATE, "LK not run");
    *n = t->n_pts;
    if (capacity < *n) return fail(LVI_ERR_CAPACITY, "capacity too small");
    return guarded(t->device, [&]() -> int32_t {
        const int m = *n;
        const size_t F = (size_t)std::max(t->P.max_features, 64);
        if (wait) LVI_HIP(hipStreamSynchronize(c.stream));
        if (m && forw_xy) std::memcpy(forw_xy, t->h_lk, sizeof(float) * 2 * (size_t)m);
        if (m && err) std::memcpy(err, t->h_lk + 2 * F, sizeof(float) * (size_t)m);
        if (m && status) std::memcpy(status, t->h_lk + 3 * F, (size_t)m);
        return LVI_OK;
    });
}

// setMask's raster half for the slots with n[s] >= 0
void stage_mask_circles(const TSlots& S, const float* const* centers_xy, const int32_t* n, int radius)
{
    TBatch<CircleArgs> B{};
    bool read[LVI_TRACKER_MAX_BATCH] = {}; int nmax = 0, gfill = 0; double px = 0;
    for (int s = 0; s < S.n; s++) {
        if (n[s] < 0) continue;
        lvi_tracker& t = S[s];
        B.a[s] = CircleArgs{t.d_mask, t.w, t.h, t.d_centers, n[s], radius};
        if (n[s]) {
            float* dst = pinned_next(t.h_centers, t.ev_centers, t.centers_slot);
            std::memcpy(dst, centers_xy[s], sizeof(float) * 2 * (size_t)n[s]);
            B.a[s].centers = dst; read[s] = true;                               // read in place (pinned host memory)
        }
        nmax = std::max(nmax, n[s]); gfill = std::max(gfill, div_up(div_up(t.w * t.h, 16), 256)); px += (double)t.w * t.h;
    }
    LVI_TLAUNCH(S, "mask_fill", px, mask_fill_kernel, dim3(gfill), 256, B);
    if (nmax) {
        LVI_TLAUNCH(S, "mask_circles", 0, mask_circles_kernel, dim3(nmax), 64, B);
        for (int s = 0; s < S.n; s++) if (read[s]) LVI_HIP(hipEventRecord(S[s].ev_centers[S[s].centers_slot], S.c.stream));
    }
    for (int s = 0; s < S.n; s++) if (n[s] >= 0) S[s].have_mask = true;
}

GfttArgs gftt_args(lvi_tracker& t)
{
    GfttArgs a{};
    a.img = t.pyr[t.forw].lv[0].px; a.mask = t.have_mask ? t.d_mask : nullptr; a.w = t.w; a.h = t.h;
    a.gx = div_up(t.w, 32); a.npartial = a.gx * div_up(t.h, 8); a.nblk = div_up(t.w * t.h, CAND_TILE);
    a.eig = t.d_eig; a.maxord = t.d_maxord; a.maxPartial = t.d_maxPartial; a.thr = t.d_thr; a.blockCnt = t.d_blockCnt; a.total = t.d_total;
    a.keysA = t.sort.keysA; a.valsA = t.sort.valsA; a.d_n = t.d_n; a.d_nbits = t.d_nbits; a.quality = t.P.gftt_quality;
    return a;
}
PickArgs pick_args(lvi_tracker& t, int32_t max_corners)
{
    PickArgs p{};
    p.keysA = t.sort.keysA; p.valsA = t.sort.valsA; p.valsB = t.sort.valsB; p.d_nbits = t.d_nbits; p.total = t.d_total;
    p.w = t.w; p.h = t.h; p.max_corners = max_corners; p.cap = t.P.max_features; p.min_dist = t.P.min_dist;
    p.out_xy = t.d_gftt_xy; p.out_n = t.d_out_n; p.ncand = t.d_ncand; p.dbg = t.d_dbg;
    return p;
}
// goodFeaturesToTrack on forw for the slots of `take`, enqueued only.  lds_form: the candidates of every slot are sorted and picked
// by ONE workgroup in LDS (a slot beyond what that form holds reports -2 in d_out_n and is redone in the radix form by whoever
// fetches the result).  The radix form (12-launch sort + one-wavefront pick) runs slot by slot: the rare path is not batched.
void enqueue_gftt(const TSlots& S, const bool* take, const int32_t* max_corners, bool lds_form)
{
    if (!lds_form && S.n > 1) {
        for (int s = 0; s < S.n; s++) if (take[s]) enqueue_gftt(S.one(s), TAKE_ALL, max_corners + s, false);
        return;
    }
    TBatch<GfttArgs> G{}; TBatch<PickArgs> K{};
    int gx = 0, gy = 0, nblk = 0; double npx = 0;
    for (int s = 0; s < S.n; s++) {
        if (!take[s]) continue;
        G.a[s] = gftt_args(S[s]); K.a[s] = pick_args(S[s], max_corners[s]);
        gx = std::max(gx, G.a[s].gx); gy = std::max(gy, div_up(G.a[s].h, 8)); nblk = std::max(nblk, G.a[s].nblk);
        npx += (double)G.a[s].w * G.a[s].h;
    }
    LVI_TLAUNCH(S, "gftt_mineig", 6.0 * npx, mineig_kernel, dim3(gx, gy), 256, G);
    LVI_TLAUNCH(S, "gftt_count", 5.0 * npx, gftt_count_kernel, dim3(nblk), 256, G);
    LVI_TLAUNCH(S, "gftt_emit", 5.0 * npx, gftt_emit_kernel, dim3(nblk), 256, G);
    if (lds_form) {
        LVI_TLAUNCH(S, "gftt_sortpick", 0, gftt_sortpick_kernel, dim3(1), 1024, K);
    } else {
        lvi_tracker& t = S[0];
        radix_sort_pairs(S.c, t.sort, t.d_n, t.d_nbits, 4, "gftt", 0.02 * npx);
        LVI_LAUNCH(S.c, "gftt_pick", 0, hipLaunchKernelGGL(gftt_pick_kernel, dim3(1), dim3(64), 0, S.c.stream, K.a[0]));
    }
}

void stage_gftt_async(const TSlots& S, const bool* take, const int32_t* max_corners)
{
    enqueue_gftt(S, take, max_corners, !S[0].gftt_force_radix);       // LVI_GFTT_RADIX=1: every slot through the radix form
    for (int s = 0; s < S.n; s++) {
        if (!take[s]) continue;
        lvi_tracker& t = S[s];
        t.gftt_pending = true; t.gftt_pending_max = max_corners[s]; t.have_gftt = false;
    }
}

// The frame end of the slots with n_kept[s] >= 0: [kept ; the corners of a pending run_gftt_async] and their undistorted points,
// two kernels that write into pinned host memory and ONE wait.  A slot beyond the LDS form (-2) is redone alone in the radix form
// on its own state, its two frame-end kernels run again (the kept points are still in the pinned slot the first attempt read) and
// a second wait follows; the other slots' results stand.  redone: bit s = slot s was redone.  A capacity error found in a slot's
// result is returned after every slot has been served (the last one, if several).
int32_t stage_frame_end(const TSlots& S, const lvi_mei_params* cams, const float* const* kept_xy, const int32_t* n_kept,
                        float* const* new_xy, int32_t new_capacity, int32_t* n_new, float* const* un_xy, int32_t& redone)
{
    const int F = S[0].P.max_features;
    TBatch<ConcatArgs> C{}; TBatch<MeiArgs> M{};
    bool with_gftt[LVI_TRACKER_MAX_BATCH] = {}, read[LVI_TRACKER_MAX_BATCH] = {};
    for (int s = 0; s < S.n; s++) {
        if (n_kept[s] < 0) continue;
        lvi_tracker& t = S[s];
        with_gftt[s] = t.gftt_pending;
        const float* kept_src = t.d_un_in;
        if (n_kept[s]) {
            float* dst = pinned_next(t.h_kept, t.ev_kept, t.kept_slot);
            std::memcpy(dst, kept_xy[s], sizeof(float) * 2 * (size_t)n_kept[s]);
            kept_src = dst; read[s] = true;                                     // read in place
        }
        int* d_hdr = reinterpret_cast<int*>(t.d_frame_out);
        C.a[s] = ConcatArgs{kept_src, t.d_gftt_xy, t.d_out_n, t.d_ncand, t.d_all_xy, d_hdr, reinterpret_cast<int*>(t.h_frame_out), t.h_frame_out + 4,
                            n_kept[s], with_gftt[s] ? 1 : 0, F};
        if (cams) M.a[s] = MeiArgs{cams[s], t.d_all_xy, t.h_frame_out + 4 + 2 * (size_t)F, d_hdr + 2, F};
    }
    auto frame_end_kernels = [&](const TSlots& Q, const TBatch<ConcatArgs>& Cq, const TBatch<MeiArgs>& Mq, const bool* readq) {
        LVI_TLAUNCH(Q, "frame_concat", 0, frame_concat_kernel, dim3(1), 64, Cq);
        for (int s = 0; s < Q.n; s++) if (readq[s]) LVI_HIP(hipEventRecord(Q[s].ev_kept[Q[s].kept_slot], Q.c.stream));
        if (cams) LVI_TLAUNCH(Q, "mei_undistort", 16.0 * F, mei_undistort_kernel, dim3(div_up(F, 64)), 64, Mq);
    };
    frame_end_kernels(S, C, M, read);
    LVI_HIP(hipStreamSynchronize(S.c.stream));                      // the ONE wait of the frame end, all slots
    redone = 0;
    for (int s = 0; s < S.n; s++) {
        if (n_kept[s] < 0 || !with_gftt[s]) continue;
        lvi_tracker& t = S[s];
        if (reinterpret_cast<const int*>(t.h_frame_out)[0] != -2) continue;
        redone |= 1 << s;
        enqueue_gftt(S.one(s), TAKE_ALL, &t.gftt_pending_max, false);
        TBatch<ConcatArgs> C1{}; TBatch<MeiArgs> M1{};
        C1.a[0] = C.a[s]; M1.a[0] = M.a[s];
        frame_end_kernels(S.one(s), C1, M1, read + s);
    }
    if (redone) LVI_HIP(hipStreamSynchronize(S.c.stream));
    int32_t rc = LVI_OK;
    for (int s = 0; s < S.n; s++) {
        if (n_kept[s] < 0) continue;
        lvi_tracker& t = S[s];
        const int* hdr = reinterpret_cast<const int*>(t.h_frame_out);
        t.gftt_pending = false;
        const int nn = with_gftt[s] ? hdr[0] : 0;
        if (nn < 0) { rc = fail(LVI_ERR_CAPACITY, "more corners than the pick kernel's accepted-list capacity"); continue; }
        if (nn > F || n_kept[s] + nn > F) { rc = fail(LVI_ERR_CAPACITY, "more corners than max_features"); continue; }
        if (nn > new_capacity) { rc = fail(LVI_ERR_CAPACITY, "capacity too small"); continue; }
        n_new[s] = nn;
        if (with_gftt[s]) { t.gftt_n = nn; t.gftt_ncand = hdr[1]; t.have_gftt = true; }
        if (nn && new_xy && new_xy[s]) std::memcpy(new_xy[s], t.h_frame_out + 4, sizeof(float) * 2 * (size_t)nn);
        if (cams && un_xy && un_xy[s]) std::memcpy(un_xy[s], t.h_frame_out + 4 + 2 * (size_t)F, sizeof(float) * 2 * (size_t)(n_kept[s] + nn));
    }
    return rc;
}

TSlots one_slot(lvi_tracker* t) { return TSlots{t->ctx, t, 1}; }

}  // namespace

extern "C" {

void lvi_tracker_params_default(lvi_tracker_params* p)
{
    memset(p, 0, sizeof(*p));
    p->max_width = 1280; p->max_height = 720; p->max_cnt = 150; p->min_dist = 20.0;
    p->lk_win = 21; p->lk_max_level = 3; p->lk_max_iters = 30; p->lk_eps = 0.01; p->lk_min_eig_threshold = 1e-4f;
    p->gftt_quality = 0.01; p->max_features = 1024;
}

int32_t lvi_tracker_create(const lvi_tracker_params* p, int32_t device, lvi_tracker** out)
{
    if (!p || !out) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (const int32_t bad = check_tracker_params(p)) return bad;
    if (const int32_t bad = check_device(device)) return bad;
    lvi_tracker* t = new lvi_tracker();
    t->P = *p; t->device = device;
    { const char* e = getenv("LVI_GFTT_RADIX"); t->gftt_force_radix = e && e[0] == '1'; }
    int32_t st = guarded(t->device, [&]() -> int32_t {
        LVI_HIP(hipStreamCreateWithFlags(&t->ctx.stream, hipStreamNonBlocking));
        t->ctx.prof = &t->prof;
        ArenaSizer sz; tracker_layout(sz, *t);
        t->arena.init(sz.used + (1 << 16));
        tracker_layout(t->arena, *t);
        LVI_HIP(hipMemsetAsync(t->arena.base, 0, t->arena.size, t->ctx.stream));
        tracker_host_alloc(t);
        LVI_HIP(hipStreamSynchronize(t->ctx.stream));
        return LVI_OK;
    });
    if (st != LVI_OK) { lvi_tracker_destroy(t); return st; }
    *out = t;
    return LVI_OK;
}

void lvi_tracker_destroy(lvi_tracker* t)
{
    if (!t) return;
    (void)hipSetDevice(t->device);
    if (t->ctx.stream) (void)hipStreamSynchronize(t->ctx.stream);
    t->prof.collect();
    t->arena.release();
    tracker_host_free(t);
    if (t->ctx.stream) (void)hipStreamDestroy(t->ctx.stream);
    delete t;
}

int32_t lvi_tracker_sync(lvi_tracker* t)
{
    if (!t) return fail(LVI_ERR_INVALID_ARG, "null handle");
    return guarded(t->device, [&]() -> int32_t { LVI_HIP(hipStreamSynchronize(t->ctx.stream)); return LVI_OK; });
}

int32_t lvi_tracker_push_image(lvi_tracker* t, const uint8_t* img, int32_t w, int32_t h, int32_t stride)
{
    if (!t || !img || w <= 0 || h <= 0 || stride < w) return fail(LVI_ERR_INVALID_ARG, "bad image");
    if (w > t->P.max_width || h > t->P.max_height) return fail(LVI_ERR_CAPACITY, "image exceeds capacity");
    return guarded(t->device, [&]() -> int32_t { stage_push(one_slot(t), &img, TAKE_ALL, w, h, stride); return LVI_OK; });
}

int32_t lvi_clahe(lvi_tracker* t, const uint8_t* img, int32_t w, int32_t h, int32_t stride, double clip_limit, int32_t tiles_x, int32_t tiles_y,
                  uint8_t* out, int32_t out_stride)
{
    if (!t || !img || !out || w <= 0 || h <= 0 || stride < w || out_stride < w) return fail(LVI_ERR_INVALID_ARG, "bad image");
    if (tiles_x < 1 || tiles_y < 1 || tiles_x > CLAHE_MAX_TILES || tiles_y > CLAHE_MAX_TILES) return fail(LVI_ERR_INVALID_ARG, "bad tile grid");
    if (w > t->P.max_width || h > t->P.max_height) return fail(LVI_ERR_CAPACITY, "image exceeds capacity");
    return guarded(t->device, [&]() -> int32_t {
        LVI_HIP(hipMemcpy2DAsync(t->d_stage, (size_t)w, img, (size_t)stride, (size_t)w, (size_t)h, hipMemcpyHostToDevice, t->ctx.stream));
        TBatch<ClaheArgs> B{};
        B.a[0] = clahe_args(*t, t->d_stage, t->d_eq, w, h, clip_limit, tiles_x, tiles_y);
        run_clahe(one_slot(t), B, tiles_x * tiles_y, w, h, (double)w * h);
        LVI_HIP(hipMemcpy2DAsync(out, (size_t)out_stride, t->d_eq, (size_t)w, (size_t)w, (size_t)h, hipMemcpyDeviceToHost, t->ctx.stream));
        LVI_HIP(hipStreamSynchronize(t->ctx.stream));
        return LVI_OK;
    });
}

int32_t lvi_tracker_set_equalize(lvi_tracker* t, int32_t on, double clip_limit, int32_t tiles_x, int32_t tiles_y)
{
    if (!t) return fail(LVI_ERR_INVALID_ARG, "null handle");
    if (on && (tiles_x < 1 || tiles_y < 1 || tiles_x > CLAHE_MAX_TILES || tiles_y > CLAHE_MAX_TILES)) return fail(LVI_ERR_INVALID_ARG, "bad tile grid");
    t->equalize = on != 0; t->clahe_clip = clip_limit; t->clahe_tx = tiles_x; t->clahe_ty = tiles_y;
    return LVI_OK;
}

int32_t lvi_undistort_points(lvi_tracker* t, const lvi_mei_params* cam, const float* xy, int32_t n, float* un_xy)
{
    if (!t || !cam || n < 0 || (n > 0 && (!xy || !un_xy))) return fail(LVI_ERR_INVALID_ARG, "bad arguments");
    if (n > t->P.max_features) return fail(LVI_ERR_CAPACITY, "too many points");
    if (n == 0) return LVI_OK;
    return guarded(t->device, [&]() -> int32_t {
        LVI_HIP(hipMemcpyAsync(t->d_un_in, xy, sizeof(float) * 2 * n, hipMemcpyHostToDevice, t->ctx.stream));
        TBatch<MeiArgs> M{};
        M.a[0] = MeiArgs{*cam, t->d_un_in, t->d_un_out, nullptr, n};
        LVI_TLAUNCH(one_slot(t), "mei_undistort", 16.0 * n, mei_undistort_kernel, dim3(div_up(n, 64)), 64, M);
        LVI_HIP(hipMemcpyAsync(un_xy, t->d_un_out, sizeof(float) * 2 * n, hipMemcpyDeviceToHost, t->ctx.stream));
        LVI_HIP(hipStreamSynchronize(t->ctx.stream));
        return LVI_OK;
    });
}

int32_t lvi_tracker_set_points(lvi_tracker* t, const float* cur_xy, int32_t n)
{
    if (!t || n < 0 || (n > 0 && !cur_xy)) return fail(LVI_ERR_INVALID_ARG, "bad points");
    if (n > t->P.max_features) return fail(LVI_ERR_CAPACITY, "too many points");
    return guarded(t->device, [&]() -> int32_t { stage_set_points(one_slot(t), &cur_xy, &n); return LVI_OK; });
}

int32_t lvi_tracker_run_lk(lvi_tracker* t)
{
    if (!t || !t->have_forw || !t->have_cur) return fail(LVI_ERR_STATE, "no image pair");
    return guarded(t->device, [&]() -> int32_t { stage_run_lk(one_slot(t), TAKE_ALL); return LVI_OK; });     // (again with the last points, if called again)
}

int32_t lvi_tracker_get_lk(lvi_tracker* t, float* forw_xy, uint8_t* status, float* err, int32_t capacity, int32_t* n)
{
    if (!t || !n) return fail(LVI_ERR_INVALID_ARG, "null argument");
    return get_lk(t->ctx, t, true, forw_xy, status, err, capacity, n);
}

int32_t lvi_tracker_set_mask(lvi_tracker* t, const uint8_t* mask, int32_t w, int32_t h, int32_t stride)
{
    if (!t) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (!mask) { t->have_mask = false; return LVI_OK; }
    if (!t->have_forw || w != t->w || h != t->h || stride < w) return fail(LVI_ERR_INVALID_ARG, "mask size mismatch");
    return guarded(t->device, [&]() -> int32_t {
        LVI_HIP(hipMemcpy2DAsync(t->d_mask, (size_t)w, mask, (size_t)stride, (size_t)w, (size_t)h, hipMemcpyHostToDevice, t->ctx.stream));
        LVI_HIP(hipStreamSynchronize(t->ctx.stream));
        t->have_mask = true;
        return LVI_OK;
    });
}

int32_t lvi_tracker_run_gftt(lvi_tracker* t, int32_t max_corners)
{
    if (!t || !t->have_forw) return fail(LVI_ERR_STATE, "no image");
    return guarded(t->device, [&]() -> int32_t {
        int res[2] = {0, 0};
        for (int attempt = 0; attempt < 2; attempt++) {
            enqueue_gftt(one_slot(t), TAKE_ALL, &max_corners, attempt == 0 && !t->gftt_force_radix);
            LVI_HIP(hipMemcpyAsync(&res[0], t->d_out_n, sizeof(int), hipMemcpyDeviceToHost, t->ctx.stream));
            LVI_HIP(hipMemcpyAsync(&res[1], t->d_ncand, sizeof(int), hipMemcpyDeviceToHost, t->ctx.stream));
            LVI_HIP(hipStreamSynchronize(t->ctx.stream));
            if (res[0] != -2) break;                        // -2: more candidates than the LDS form holds -> once more, radix form
        }
        t->gftt_pending = false;
        if (res[0] < 0) return fail(LVI_ERR_CAPACITY, "more corners than the pick kernel's accepted-list capacity");
        if (res[0] > t->P.max_features) return fail(LVI_ERR_CAPACITY, "more corners than max_features");
        t->gftt_n = res[0]; t->gftt_ncand = res[1]; t->have_gftt = true;
        return LVI_OK;
    });
}

int32_t lvi_tracker_set_mask_circles(lvi_tracker* t, const float* centers_xy, int32_t n, int32_t radius)
{
    if (!t || n < 0 || (n > 0 && !centers_xy) || radius < 0 || radius > 120) return fail(LVI_ERR_INVALID_ARG, "bad circle list");
    if (!t->have_forw) return fail(LVI_ERR_STATE, "no image");
    if (n > t->P.max_features) return fail(LVI_ERR_CAPACITY, "too many circles");
    return guarded(t->device, [&]() -> int32_t { stage_mask_circles(one_slot(t), &centers_xy, &n, radius); return LVI_OK; });
}

int32_t lvi_tracker_run_gftt_async(lvi_tracker* t, int32_t max_corners)
{
    if (!t || !t->have_forw) return fail(LVI_ERR_STATE, "no image");
    return guarded(t->device, [&]() -> int32_t { stage_gftt_async(one_slot(t), TAKE_ALL, &max_corners); return LVI_OK; });
}

int32_t lvi_tracker_finish_frame(lvi_tracker* t, const lvi_mei_params* cam, const float* kept_xy, int32_t n_kept,
                                 float* new_xy, int32_t new_capacity, int32_t* n_new, float* un_xy)
{
    if (!t || n_kept < 0 || (n_kept > 0 && !kept_xy) || !n_new) return fail(LVI_ERR_INVALID_ARG, "bad arguments");
    if (n_kept > t->P.max_features) return fail(LVI_ERR_CAPACITY, "too many points");
    return guarded(t->device, [&]() -> int32_t {
        int32_t redone;
        return stage_frame_end(one_slot(t), cam, &kept_xy, &n_kept, &new_xy, new_capacity, n_new, &un_xy, redone);
    });
}

int32_t lvi_tracker_get_gftt(lvi_tracker* t, float* xy, int32_t capacity, int32_t* n)
{
    if (!t || !n) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (!t->have_gftt) return fail(LVI_ERR_STATE, "GFTT not run");
    *n = t->gftt_n;
    if (capacity < *n) return fail(LVI_ERR_CAPACITY, "capacity too small");
    return guarded(t->device, [&]() -> int32_t {
        if (*n && xy) LVI_HIP(hipMemcpyAsync(xy, t->d_gftt_xy, sizeof(float) * 2 * *n, hipMemcpyDeviceToHost, t->ctx.stream));
        LVI_HIP(hipStreamSynchronize(t->ctx.stream));
        return LVI_OK;
    });
}

int32_t lvi_lk_track(lvi_tracker* t, const uint8_t* prev, const uint8_t* next, int32_t w, int32_t h, int32_t stride,
                     const float* prev_xy, int32_t n, float* next_xy, uint8_t* status, float* err)
{
    if (!t || !prev || !next || n < 0) return fail(LVI_ERR_INVALID_ARG, "bad arguments");
    t->have_forw = false; t->have_cur = false;
    int32_t st = lvi_tracker_push_image(t, prev, w, h, stride); if (st) return st;
    st = lvi_tracker_push_image(t, next, w, h, stride); if (st) return st;
    st = lvi_tracker_set_points(t, prev_xy, n); if (st) return st;
    st = lvi_tracker_run_lk(t); if (st) return st;
    int32_t m = 0;
    return lvi_tracker_get_lk(t, next_xy, status, err, n, &m);
}

int32_t lvi_good_features(lvi_tracker* t, const uint8_t* img, const uint8_t* mask, int32_t w, int32_t h, int32_t stride,
                          int32_t max_corners, double quality, double min_dist, float* xy, int32_t xy_capacity, int32_t* n_out)
{
    if (!t || !img || !n_out) return fail(LVI_ERR_INVALID_ARG, "bad arguments");
    t->have_forw = false; t->have_cur = false;
    int32_t st = lvi_tracker_push_image(t, img, w, h, stride); if (st) return st;
    st = lvi_tracker_set_mask(t, mask, w, h, stride); if (st) return st;
    const double q0 = t->P.gftt_quality, d0 = t->P.min_dist;
    t->P.gftt_quality = quality; t->P.min_dist = min_dist;
    st = lvi_tracker_run_gftt(t, max_corners);
    t->P.gftt_quality = q0; t->P.min_dist = d0;
    if (st) return st;
    return lvi_tracker_get_gftt(t, xy, xy_capacity, n_out);
}

int32_t lvi_tracker_debug_get(lvi_tracker* t, int32_t what, void* dst, int64_t cap, int64_t* n_bytes)
{
    if (!t) return fail(LVI_ERR_INVALID_ARG, "null handle");
    return guarded(t->device, [&]() -> int32_t {
        const void* src = nullptr; int64_t bytes = 0; int32_t host_val = 0; bool host = false;
        switch (what) {
            case LVI_TDBG_PYRAMID_L1: case LVI_TDBG_PYRAMID_L2: case LVI_TDBG_PYRAMID_L3: {
                const int l = what - LVI_TDBG_PYRAMID_L1 + 1;
                if (!t->have_forw || l > t->pyr[t->forw].top) return fail(LVI_ERR_STATE, "level not built");
                src = t->pyr[t->forw].lv[l].px; bytes = (int64_t)t->pyr[t->forw].lv[l].w * t->pyr[t->forw].lv[l].h;
                break;
            }
            case LVI_TDBG_MINEIG:
                if (!t->have_gftt) return fail(LVI_ERR_STATE, "GFTT not run");
                src = t->d_eig; bytes = (int64_t)t->w * t->h * 4;
                break;
            case LVI_TDBG_GFTT_NCAND:
                if (!t->have_gftt) return fail(LVI_ERR_STATE, "GFTT not run");
                host = true; host_val = t->gftt_ncand; bytes = 4;
                break;
            case 7:                                  // phase stamps of gftt_sortpick (diagnostics, HIP only)
                src = t->d_dbg; bytes = 64;
                break;
            case LVI_TDBG_MASK:
                if (!t->have_mask || !t->have_forw) return fail(LVI_ERR_STATE, "no mask");
                src = t->d_mask; bytes = (int64_t)t->w * t->h;
                break;
            default: return fail(LVI_ERR_INVALID_ARG, "unknown debug item");
        }
        if (n_bytes) *n_bytes = bytes;
        if (!dst) return LVI_OK;
        if (cap < bytes) return fail(LVI_ERR_CAPACITY, "debug buffer too small");
        if (host) { memcpy(dst, &host_val, 4); return LVI_OK; }
        LVI_HIP(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToHost, t->ctx.stream));
        LVI_HIP(hipStreamSynchronize(t->ctx.stream));
        return LVI_OK;
    });
}

}  // extern "C"

namespace {
int32_t prof_enable_impl(int device, Ctx& c, Profiler& p, int32_t on)
{
    return guarded(device, [&]() -> int32_t { LVI_HIP(hipStreamSynchronize(c.stream)); p.collect(); p.on = on != 0; return LVI_OK; });
}
int32_t prof_reset_impl(int device, Ctx& c, Profiler& p)
{
    return guarded(device, [&]() -> int32_t { LVI_HIP(hipStreamSynchronize(c.stream)); p.reset(); return LVI_OK; });
}
int32_t prof_read_impl(int device, Ctx& c, Profiler& p, lvi_kernel_stat* stats, int32_t capacity, int32_t* n)
{
    return guarded(device, [&]() -> int32_t {
        LVI_HIP(hipStreamSynchronize(c.stream)); p.collect();
        int k = 0;
        for (size_t i = 0; i < p.names.size(); i++) {
            if (!p.launches[i]) continue;
            if (k < capacity && stats) {
                memset(&stats[k], 0, sizeof(stats[k]));
                strncpy(stats[k].name, p.names[i].c_str(), sizeof(stats[k].name) - 1);
                stats[k].launches = p.launches[i]; stats[k].total_ms = p.total_ms[i]; stats[k].bytes_alg = p.bytes[i];
            }
            k++;
        }
        *n = std::min(k, capacity);
        return LVI_OK;
    });
}
}  // namespace

extern "C" {

int32_t lvi_tracker_prof_enable(lvi_tracker* t, int32_t on)
{
    if (!t) return fail(LVI_ERR_INVALID_ARG, "null handle");
    return prof_enable_impl(t->device, t->ctx, t->prof, on);
}
int32_t lvi_tracker_prof_reset(lvi_tracker* t)
{
    if (!t) return fail(LVI_ERR_INVALID_ARG, "null handle");
    return prof_reset_impl(t->device, t->ctx, t->prof);
}
int32_t lvi_tracker_prof_read(lvi_tracker* t, lvi_kernel_stat* stats, int32_t capacity, int32_t* n)
{
    if (!t || !n) return fail(LVI_ERR_INVALID_ARG, "null argument");
    return prof_read_impl(t->device, t->ctx, t->prof, stats, capacity, n);
}

}  // extern "C"

// =============================================================================================
// lvi_tbatch (include/lvi_tbatch.h): up to 8 tracker states in one arena on one stream, every stage one launch for all
// slots.  A slot IS an lvi_tracker state (same buffers, same pinned double slots, same flags) whose launches go through the
// handle's stream and profiler.  Every call checks its tables for all slots and runs the stage routine of the single handle
// over the set of its S slots; what the handle adds is which slots set_points armed and whether an LK result is awaited.
// =============================================================================================
struct lvi_tbatch {
    lvi_tracker_params P;
    int device = 0, S = 0;
    Ctx ctx; Profiler prof; Arena arena;
    lvi_tracker slot[LVI_TRACKER_MAX_BATCH];
    bool armed[LVI_TRACKER_MAX_BATCH] = {};        // set_points since the slot's last run_lk
    bool lk_in_flight = false;                     // run_lk enqueued, the stream not waited for yet (get_lk waits once)
    int32_t redo_mask = 0;                         // LVI_TBDBG_REDO_MASK
};

namespace {

TSlots all_slots(lvi_tbatch* b) { return TSlots{b->ctx, b->slot, b->S}; }
int32_t bad_slot(const lvi_tbatch* b, int32_t slot) { return !b || slot < 0 || slot >= b->S; }

}  // namespace

extern "C" {

int32_t lvi_tbatch_abi_version(void) { return LVI_TBATCH_ABI_VERSION; }

int32_t lvi_tbatch_create(const lvi_tracker_params* p, int32_t slots, int32_t device, lvi_tbatch** out)
{
    if (!p || !out) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (slots < 1 || slots > LVI_TRACKER_MAX_BATCH) return fail(LVI_ERR_INVALID_ARG, "slots must be 1..LVI_TRACKER_MAX_BATCH");
    if (const int32_t bad = check_tracker_params(p)) return bad;
    if (const int32_t bad = check_device(device)) return bad;
    lvi_tbatch* b = new lvi_tbatch();
    b->P = *p; b->device = device; b->S = slots;
    const char* e = getenv("LVI_GFTT_RADIX");
    for (int s = 0; s < slots; s++) { b->slot[s].P = *p; b->slot[s].device = device; b->slot[s].gftt_force_radix = e && e[0] == '1'; }
    int32_t st = guarded(device, [&]() -> int32_t {
        LVI_HIP(hipStreamCreateWithFlags(&b->ctx.stream, hipStreamNonBlocking));
        b->ctx.prof = &b->prof;
        ArenaSizer sz;
        for (int s = 0; s < slots; s++) tracker_layout(sz, b->slot[s]);
        b->arena.init(sz.used + (1 << 16));
        for (int s = 0; s < slots; s++) tracker_layout(b->arena, b->slot[s]);
        LVI_HIP(hipMemsetAsync(b->arena.base, 0, b->arena.size, b->ctx.stream));
        for (int s = 0; s < slots; s++) { b->slot[s].ctx = b->ctx; tracker_host_alloc(&b->slot[s]); }
        LVI_HIP(hipStreamSynchronize(b->ctx.stream));
        return LVI_OK;
    });
    if (st != LVI_OK) { lvi_tbatch_destroy(b); return st; }
    *out = b;
    return LVI_OK;
}

void lvi_tbatch_destroy(lvi_tbatch* b)
{
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->ctx.stream) (void)hipStreamSynchronize(b->ctx.stream);
    b->prof.collect();
    b->arena.release();
    for (int s = 0; s < b->S; s++) tracker_host_free(&b->slot[s]);
    if (b->ctx.stream) (void)hipStreamDestroy(b->ctx.stream);
    delete b;
}

int32_t lvi_tbatch_sync(lvi_tbatch* b)
{
    if (!b) return fail(LVI_ERR_INVALID_ARG, "null handle");
    return guarded(b->device, [&]() -> int32_t { LVI_HIP(hipStreamSynchronize(b->ctx.stream)); b->lk_in_flight = false; return LVI_OK; });
}

int32_t lvi_tbatch_set_equalize(lvi_tbatch* b, int32_t on, double clip_limit, int32_t tiles_x, int32_t tiles_y)
{
    if (!b) return fail(LVI_ERR_INVALID_ARG, "null handle");
    if (on && (tiles_x < 1 || tiles_y < 1 || tiles_x > CLAHE_MAX_TILES || tiles_y > CLAHE_MAX_TILES)) return fail(LVI_ERR_INVALID_ARG, "bad tile grid");
    for (int s = 0; s < b->S; s++) { lvi_tracker& t = b->slot[s]; t.equalize = on != 0; t.clahe_clip = clip_limit; t.clahe_tx = tiles_x; t.clahe_ty = tiles_y; }
    return LVI_OK;
}

int32_t lvi_tbatch_push_images(lvi_tbatch* b, const uint8_t* const* imgs, int32_t w, int32_t h, int32_t stride)
{
    if (!b || !imgs || w <= 0 || h <= 0 || stride < w) return fail(LVI_ERR_INVALID_ARG, "bad image table");
    if (w > b->P.max_width || h > b->P.max_height) return fail(LVI_ERR_CAPACITY, "image exceeds capacity");
    bool take[LVI_TRACKER_MAX_BATCH] = {}, any = false;
    for (int s = 0; s < b->S; s++) { take[s] = imgs[s] != nullptr; any = any || take[s]; }
    if (!any) return LVI_OK;
    return guarded(b->device, [&]() -> int32_t { stage_push(all_slots(b), imgs, take, w, h, stride); return LVI_OK; });
}

int32_t lvi_tbatch_set_points(lvi_tbatch* b, const float* const* cur_xy, const int32_t* n)
{
    if (!b || !n) return fail(LVI_ERR_INVALID_ARG, "null argument");
    for (int s = 0; s < b->S; s++) {
        if (n[s] > 0 && (!cur_xy || !cur_xy[s])) return fail(LVI_ERR_INVALID_ARG, "bad points");
        if (n[s] > b->P.max_features) return fail(LVI_ERR_CAPACITY, "too many points");
    }
    return guarded(b->device, [&]() -> int32_t {
        stage_set_points(all_slots(b), cur_xy, n);
        for (int s = 0; s < b->S; s++) if (n[s] >= 0) b->armed[s] = true;
        return LVI_OK;
    });
}

int32_t lvi_tbatch_run_lk(lvi_tbatch* b)
{
    if (!b) return fail(LVI_ERR_INVALID_ARG, "null handle");
    for (int s = 0; s < b->S; s++)
        if (b->armed[s] && (!b->slot[s].have_forw || !b->slot[s].have_cur)) return fail(LVI_ERR_STATE, "no image pair");
    return guarded(b->device, [&]() -> int32_t {
        if (stage_run_lk(all_slots(b), b->armed)) b->lk_in_flight = true;       // only the slots armed by set_points: no re-run
        for (int s = 0; s < b->S; s++) b->armed[s] = false;
        return LVI_OK;
    });
}

int32_t lvi_tbatch_get_lk(lvi_tbatch* b, int32_t slot, float* forw_xy, uint8_t* status, float* err, int32_t capacity, int32_t* n)
{
    if (bad_slot(b, slot) || !n) return fail(LVI_ERR_INVALID_ARG, "bad slot or null argument");
    const int32_t st = get_lk(b->ctx, &b->slot[slot], b->lk_in_flight, forw_xy, status, err, capacity, n);       // the one wait for all slots
    if (st == LVI_OK) b->lk_in_flight = false;
    return st;
}

int32_t lvi_tbatch_set_mask_circles(lvi_tbatch* b, const float* const* centers_xy, const int32_t* n, int32_t radius)
{
    if (!b || !n || radius < 0 || radius > 120) return fail(LVI_ERR_INVALID_ARG, "bad circle table");
    bool any = false;
    for (int s = 0; s < b->S; s++) {
        if (n[s] > 0 && (!centers_xy || !centers_xy[s])) return fail(LVI_ERR_INVALID_ARG, "bad circle list");
        if (n[s] >= 0 && !b->slot[s].have_forw) return fail(LVI_ERR_STATE, "no image");
        if (n[s] > b->P.max_features) return fail(LVI_ERR_CAPACITY, "too many circles");
        any = any || n[s] >= 0;
    }
    if (!any) return LVI_OK;
    return guarded(b->device, [&]() -> int32_t { stage_mask_circles(all_slots(b), centers_xy, n, radius); return LVI_OK; });
}

int32_t lvi_tbatch_run_gftt_async(lvi_tbatch* b, const int32_t* max_corners)
{
    if (!b || !max_corners) return fail(LVI_ERR_INVALID_ARG, "null argument");
    bool take[LVI_TRACKER_MAX_BATCH] = {}, any = false;
    for (int s = 0; s < b->S; s++) {
        take[s] = max_corners[s] >= 0;
        if (take[s] && !b->slot[s].have_forw) return fail(LVI_ERR_STATE, "no image");
        any = any || take[s];
    }
    if (!any) return LVI_OK;
    return guarded(b->device, [&]() -> int32_t { stage_gftt_async(all_slots(b), take, max_corners); return LVI_OK; });
}

int32_t lvi_tbatch_finish_frame(lvi_tbatch* b, const lvi_mei_params* cams, const float* const* kept_xy, const int32_t* n_kept,
                                float* const* new_xy, int32_t new_capacity, int32_t* n_new, float* const* un_xy)
{
    if (!b || !n_kept || !n_new) return fail(LVI_ERR_INVALID_ARG, "bad arguments");
    bool any = false;
    for (int s = 0; s < b->S; s++) {
        if (n_kept[s] > 0 && (!kept_xy || !kept_xy[s])) return fail(LVI_ERR_INVALID_ARG, "bad kept points");
        if (n_kept[s] > b->P.max_features) return fail(LVI_ERR_CAPACITY, "too many points");
        any = any || n_kept[s] >= 0;
    }
    if (!any) return LVI_OK;
    return guarded(b->device, [&]() -> int32_t {
        const int32_t rc = stage_frame_end(all_slots(b), cams, kept_xy, n_kept, new_xy, new_capacity, n_new, un_xy, b->redo_mask);
        b->lk_in_flight = false;                                       // (the frame end waited for the stream)
        return rc;
    });
}

int32_t lvi_tbatch_debug_get(lvi_tbatch* b, int32_t slot, int32_t what, void* dst, int64_t cap, int64_t* n_bytes)
{
    if (!b) return fail(LVI_ERR_INVALID_ARG, "null handle");
    if (what == LVI_TBDBG_REDO_MASK) {
        if (n_bytes) *n_bytes = 4;
        if (!dst) return LVI_OK;
        if (cap < 4) return fail(LVI_ERR_CAPACITY, "debug buffer too small");
        memcpy(dst, &b->redo_mask, 4);
        return LVI_OK;
    }
    if (bad_slot(b, slot)) return fail(LVI_ERR_INVALID_ARG, "slot out of range");
    return lvi_tracker_debug_get(&b->slot[slot], what, dst, cap, n_bytes);      // (the slot's stream is the handle's)
}

int32_t lvi_tbatch_prof_enable(lvi_tbatch* b, int32_t on)
{
    if (!b) return fail(LVI_ERR_INVALID_ARG, "null handle");
    return prof_enable_impl(b->device, b->ctx, b->prof, on);
}
int32_t lvi_tbatch_prof_reset(lvi_tbatch* b)
{
    if (!b) return fail(LVI_ERR_INVALID_ARG, "null handle");
    return prof_reset_impl(b->device, b->ctx, b->prof);
}
int32_t lvi_tbatch_prof_read(lvi_tbatch* b, lvi_kernel_stat* stats, int32_t capacity, int32_t* n)
{
    if (!b || !n) return fail(LVI_ERR_INVALID_ARG, "null argument");
    return prof_read_impl(b->device, b->ctx, b->prof, stats, capacity, n);
}

}  // extern "C"
