// pose_graph keyframes on the GPU (include/lvi_kf.h; the contract is DESIGN §14): the image work of the KeyFrame
// constructor (keyframe.cpp:14-73) and findConnection's descriptor search (:81-131, 266-271).
//
//   kf_blur        GaussianBlur(9x9, sigma 2) of OpenCV's fixed-point path, fused: one LDS tile with a 4-pixel halo
//                  (reflect-101), the u16 horizontal pass kept in LDS, the image read once and written once
//   kf_fast_score  FAST-9/16 score map (u8) from an LDS tile with a 3-pixel halo
//   kf_nms<0>      3x3 non-max suppression, one wavefront per image row: the row's corner count
//   kf_row_scan    exclusive scan of the row counts; the totals go to a device counter the later launches read
//   kf_nms<1>      the same test again, writing (x, y) at row offset + rank in the row: row-major, no atomics
//   kf_brief       one wavefront per point (window points and FAST keypoints in one launch): lane l of round r tests
//                  pair 64 r + l, the 64-wide ballot is word r
//   kf_norm        keypoints_norm through the tracker's MEI lift (lvi_mei.hpp)
//   kf_match       one workgroup per window descriptor: XOR + popcount against every old descriptor, packed
//                  (dist << 32 | index) minimum per thread, then over the wavefront, then through LDS
//
// Everything but kf_norm is integer arithmetic (the BRIEF coordinates are one f32 addition and a truncation), so the
// results equal tests/kfdesc_ref.py bit for bit.
#include "lvi_mei.hpp"
#include "lvi_kf_store.hpp"

using namespace lvi;

namespace {

constexpr int TILE_W = 64, TILE_H = 16;      // output tile of the two stencil kernels: 256 threads, 4 rows per thread
constexpr int BLUR_R = 4, FAST_R = 3;
constexpr int MAX_SIDE = 8192;

// BORDER_REFLECT_101; the final clamp only matters for halo pixels that no in-image output reads (partial tiles)
__device__ __forceinline__ int reflect101(int i, int n)
{
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * (n - 1) - i : i;
    return min(max(i, 0), n - 1);
}

// 8.8 fixed-point Gaussian weights of ksize 9, sigma 2 (tests/kfdesc_ref.py derives them; they sum to 256)
#define LVI_KF_GAUSS(f, r) (7 * f(r, 0) + 17 * f(r, 1) + 32 * f(r, 2) + 46 * f(r, 3) + 52 * f(r, 4) + 46 * f(r, 5) + 32 * f(r, 6) + 17 * f(r, 7) + 7 * f(r, 8))

__global__ __launch_bounds__(256) void kf_blur_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int w, int h)
{
    __shared__ uint8_t s_src[TILE_H + 2 * BLUR_R][TILE_W + 2 * BLUR_R];
    __shared__ uint16_t s_h[TILE_H + 2 * BLUR_R][TILE_W];
    const int x0 = blockIdx.x * TILE_W, y0 = blockIdx.y * TILE_H;
    constexpr int SW = TILE_W + 2 * BLUR_R, SH = TILE_H + 2 * BLUR_R;
    for (int i = threadIdx.x; i < SW * SH; i += 256) {
        const int r = i / SW, c = i % SW;
        s_src[r][c] = src[(size_t)reflect101(y0 - BLUR_R + r, h) * w + reflect101(x0 - BLUR_R + c, w)];
    }
    __syncthreads();
    const int col = threadIdx.x & 63, grp = threadIdx.x >> 6;
    // horizontal: 24 rows of 64, 6 rows per thread; 255 * 256 fits u16
#define KF_TAP_SRC(r, k) (int)s_src[r][col + k]
#pragma unroll
    for (int j = 0; j < SH / 4; j++) {
        const int r = grp * (SH / 4) + j;
        s_h[r][col] = (uint16_t)LVI_KF_GAUSS(KF_TAP_SRC, r);
    }
#undef KF_TAP_SRC
    __syncthreads();
    // vertical: u32 accumulation, rounded back to u8
    const int x = x0 + col;
#define KF_TAP_ROW(r, k) (unsigned)s_h[r + k][col]
#pragma unroll
    for (int j = 0; j < TILE_H / 4; j++) {
        const int r = grp * (TILE_H / 4) + j, y = y0 + r;
        const unsigned v = LVI_KF_GAUSS(KF_TAP_ROW, r);
        if (x < w && y < h) dst[(size_t)y * w + x] = (uint8_t)((v + 32768u) >> 16);
    }
#undef KF_TAP_ROW
}

// FAST-9/16 score of one pixel: d[k] = v - p_k over the circle; best = max over the 16 arcs of 9 contiguous pixels of
// min(d) and of min(-d); a corner iff best > t, its score best - 1.  This closed form equals OpenCV's cornerScore<16>
// (the largest threshold at which the pixel is still a corner) without its early-exit loop.
__device__ __forceinline__ int fast_score_px(const int (&d)[16])
{
    constexpr int T = LVI_KF_FAST_T;
    // early reject (changes no score): every arc of 9 holds pixel k or pixel k + 8, so an arc brighter (darker) than
    // v by more than t needs one of each opposite pair to be so
    const bool dark_ring = max(d[0], d[8]) > T && max(d[4], d[12]) > T;        // ring darker than the centre: d > t
    const bool bright_ring = min(d[0], d[8]) < -T && min(d[4], d[12]) < -T;
    if (!dark_ring && !bright_ring) return 0;
    int lo2[16], lo4[16], lo8[16], hi2[16], hi4[16], hi8[16];
#pragma unroll
    for (int k = 0; k < 16; k++) { lo2[k] = min(d[k], d[(k + 1) & 15]); hi2[k] = max(d[k], d[(k + 1) & 15]); }
#pragma unroll
    for (int k = 0; k < 16; k++) { lo4[k] = min(lo2[k], lo2[(k + 2) & 15]); hi4[k] = max(hi2[k], hi2[(k + 2) & 15]); }
#pragma unroll
    for (int k = 0; k < 16; k++) { lo8[k] = min(lo4[k], lo4[(k + 4) & 15]); hi8[k] = max(hi4[k], hi4[(k + 4) & 15]); }
    int best = -256;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        best = max(best, min(lo8[k], d[(k + 8) & 15]));                         // min of d over the arc k .. k + 8
        best = max(best, -max(hi8[k], d[(k + 8) & 15]));                        // min of -d
    }
    return best > T ? best - 1 : 0;
}

__global__ __launch_bounds__(256) void kf_fast_score_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ score, int w, int h)
{
    constexpr int SW = TILE_W + 2 * FAST_R + 2, SH = TILE_H + 2 * FAST_R;       // rows padded to 72 bytes
    __shared__ uint8_t s[SH][SW];
    const int x0 = blockIdx.x * TILE_W, y0 = blockIdx.y * TILE_H;
    for (int i = threadIdx.x; i < SW * SH; i += 256) {
        const int r = i / SW, c = i % SW;
        // clamped: a pixel whose circle leaves the image scores 0 whatever is read here
        s[r][c] = src[(size_t)min(max(y0 - FAST_R + r, 0), h - 1) * w + min(max(x0 - FAST_R + c, 0), w - 1)];
    }
    __syncthreads();
    const int col = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int x = x0 + col;
#pragma unroll
    for (int j = 0; j < TILE_H / 4; j++) {
        const int r = grp * (TILE_H / 4) + j, y = y0 + r;
        int sc = 0;
        if (x >= FAST_R && x < w - FAST_R && y >= FAST_R && y < h - FAST_R) {
            const int cy = r + FAST_R, cx = col + FAST_R;
            const int v = s[cy][cx];
            const int d[16] = {v - s[cy + 3][cx],     v - s[cy + 3][cx + 1], v - s[cy + 2][cx + 2], v - s[cy + 1][cx + 3],
                               v - s[cy][cx + 3],     v - s[cy - 1][cx + 3], v - s[cy - 2][cx + 2], v - s[cy - 3][cx + 1],
                               v - s[cy - 3][cx],     v - s[cy - 3][cx - 1], v - s[cy - 2][cx - 2], v - s[cy - 1][cx - 3],
                               v - s[cy][cx - 3],     v - s[cy + 1][cx - 3], v - s[cy + 2][cx - 2], v - s[cy + 3][cx - 1]};
            sc = fast_score_px(d);
        }
        if (x < w && y < h) score[(size_t)y * w + x] = (uint8_t)sc;
    }
}

// non-max suppression, one wavefront per row.  WRITE = false: rows[y] = the row's corner count.  WRITE = true: rows[y]
// is the row's exclusive offset; corner number offset + rank goes to kp_xy when below max_kp.  A corner has x, y at
// least 3 pixels inside the image (every other score is 0), so its 8 neighbours exist.
template <bool WRITE>
__global__ __launch_bounds__(256) void kf_nms_kernel(const uint8_t* __restrict__ score, int w, int h, int* __restrict__ rows, float2* __restrict__ kp_xy, int max_kp)
{
    const int y = blockIdx.x * 4 + wave_id(), lane = lane_id();
    if (y >= h) return;                                                          // the whole wavefront
    int cnt = WRITE ? rows[y] : 0;
    if (y >= FAST_R && y < h - FAST_R) {
        for (int xb = 0; xb < w; xb += LVI_WAVE) {
            const int x = xb + lane;
            bool keep = false;
            if (x >= FAST_R && x < w - FAST_R) {
                const uint8_t* p = score + (size_t)y * w + x;
                const int s = p[0];
                if (s > 0) keep = s > p[-1] && s > p[1] && s > p[-w - 1] && s > p[-w] && s > p[-w + 1] && s > p[w - 1] && s > p[w] && s > p[w + 1];
            }
            const uint64_t m = __ballot(keep);
            if (WRITE && keep) {
                const int pos = cnt + __popcll(m & lanemask_lt());
                if (pos < max_kp) kp_xy[pos] = make_float2((float)x, (float)y);
            }
            cnt += __popcll(m);
        }
    }
    if (!WRITE && lane == 0) rows[y] = cnt;
}

// counters[0] = corners found, counters[1] = corners stored
__global__ __launch_bounds__(1024) void kf_row_scan_kernel(const int* __restrict__ row_count, int* __restrict__ row_off, int h, int max_kp, int* __restrict__ counters)
{
    __shared__ int ws[1024 / 64 + 1];
    int carry = 0;
    for (int b = 0; b < h; b += 1024) {
        const int i = b + threadIdx.x;
        int total;
        const int ex = block_excl_scan<1024>(i < h ? row_count[i] : 0, ws, &total);
        if (i < h) row_off[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) { counters[0] = carry; counters[1] = min(carry, max_kp); }
}

struct BriefArgs {
    const uint8_t* blur; int w, h;
    const int* pattern;            // [256] (x1, y1, x2, y2) as four signed bytes
    const float* win_xy; int n_window;
    const float* kp_xy; const int* counters;
    ulonglong2 *win_desc, *kp_desc;
};

__global__ __launch_bounds__(256) void kf_brief_kernel(BriefArgs a)
{
    __shared__ int s_pat[LVI_KF_PAIRS];
    s_pat[threadIdx.x] = a.pattern[threadIdx.x];
    __syncthreads();
    const int p = blockIdx.x * 4 + wave_id(), lane = lane_id();
    const float* xy;
    ulonglong2* out;
    if (p < a.n_window) { xy = a.win_xy + 2 * p; out = a.win_desc + 2 * (size_t)p; }
    else {
        const int k = p - a.n_window;
        if (k >= a.counters[1]) return;                                          // the whole wavefront; no barrier follows
        xy = a.kp_xy + 2 * k; out = a.kp_desc + 2 * (size_t)k;
    }
    const float px = xy[0], py = xy[1], fw = (float)a.w, fh = (float)a.h;
    uint64_t word[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int pk = s_pat[64 * r + lane];
        // f32 sums; tested against (-1, W) before the cast so that no out-of-range (or NaN) cast is evaluated
        const float sx1 = px + (float)(signed char)(pk & 0xFF), sy1 = py + (float)(signed char)((pk >> 8) & 0xFF);
        const float sx2 = px + (float)(signed char)((pk >> 16) & 0xFF), sy2 = py + (float)(signed char)((pk >> 24) & 0xFF);
        bool bit = false;
        if (sx1 > -1.f && sx1 < fw && sy1 > -1.f && sy1 < fh && sx2 > -1.f && sx2 < fw && sy2 > -1.f && sy2 < fh) {
            const int X1 = (int)sx1, Y1 = (int)sy1, X2 = (int)sx2, Y2 = (int)sy2;     // towards zero: -0.4 reads pixel 0
            bit = a.blur[(size_t)Y1 * a.w + X1] < a.blur[(size_t)Y2 * a.w + X2];
        }
        word[r] = __ballot(bit);
    }
    if (lane == 0) { out[0] = make_ulonglong2(word[0], word[1]); out[1] = make_ulonglong2(word[2], word[3]); }
}

__global__ __launch_bounds__(64) void kf_norm_kernel(lvi_mei_params c, const float* __restrict__ kp_xy, const int* __restrict__ counters, float* __restrict__ out)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= counters[1]) return;
    mei_lift_normalized(c, kp_xy[2 * i], kp_xy[2 * i + 1], out[2 * i], out[2 * i + 1]);
}

// searchInAera for window descriptor blockIdx.x: the smallest (dist, index) pair, ties to the lowest index
__global__ __launch_bounds__(256) void kf_match_kernel(const ulonglong2* __restrict__ win_desc, const ulonglong2* __restrict__ old_desc, int m,
                                                       int* __restrict__ index_out, int* __restrict__ dist_out, uint8_t* __restrict__ status_out)
{
    __shared__ unsigned long long s_key[4];
    const int q = blockIdx.x;
    const ulonglong2 a0 = win_desc[2 * (size_t)q], a1 = win_desc[2 * (size_t)q + 1];
    unsigned long long best = ((unsigned long long)LVI_KF_MATCH_START << 32) | 0xFFFFFFFFull;
    for (int j = threadIdx.x; j < m; j += 256) {
        const ulonglong2 b0 = old_desc[2 * (size_t)j], b1 = old_desc[2 * (size_t)j + 1];
        const int d = __popcll(a0.x ^ b0.x) + __popcll(a0.y ^ b0.y) + __popcll(a1.x ^ b1.x) + __popcll(a1.y ^ b1.y);
        const unsigned long long key = ((unsigned long long)d << 32) | (unsigned)j;
        best = key < best ? key : best;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long t = __shfl_xor(best, o, 64); best = t < best ? t : best; }
    if (lane_id() == 0) s_key[wave_id()] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; k++) best = s_key[k] < best ? s_key[k] : best;
        const int d = (int)(best >> 32);
        const bool found = d < LVI_KF_MATCH_START;                               // bestDist starts at 128, strict <
        index_out[q] = found ? (int)(unsigned)best : -1;
        dist_out[q] = found ? d : LVI_KF_MATCH_START;
        status_out[q] = found && d < LVI_KF_MATCH_ACCEPT ? 1 : 0;
    }
}

struct Slot {
    bool valid = false;
    int n_kp = 0, n_win = 0;
    float *kp_xy = nullptr, *kp_norm = nullptr, *win_xy = nullptr;
    ulonglong2 *kp_desc = nullptr, *win_desc = nullptr;
    uint64_t generation = 0;               // bumped by every call that changes the slot (lvi_kf_store.hpp)
};

}  // namespace

// ---------------------------------------------------------------------------------------------- the handle
struct lvi_kf : Handle {
    int W = 0, H = 0, K = 0, Wn = 0, S = 0;
    char* d_in = nullptr;                  // window xy [Wn][2] | image (tightly packed)
    char* h_in = nullptr;                  // pinned mirror of d_in
    size_t off_img = 0, in_bytes = 0;
    uint8_t *d_blur = nullptr, *d_score = nullptr;
    int *d_row_count = nullptr, *d_row_off = nullptr, *d_counters = nullptr, *d_pattern = nullptr;
    char* d_match = nullptr;               // index [Wn] i32 | dist [Wn] i32 | status [Wn] u8
    char* h_out = nullptr;                 // pinned: counters [2] | the match block
    size_t match_bytes = 0;
    std::vector<Slot> slots;
    int last_w = 0, last_h = 0;

    template <class A, class B> void layout(A& a, B& pin)
    {
        alloc_pair(a, pin, d_in, h_in, in_bytes);
        h_out = pin.template alloc<char>(256 + match_bytes);
        d_blur = a.template alloc<uint8_t>((size_t)W * H);
        d_score = a.template alloc<uint8_t>((size_t)W * H);
        d_row_count = a.template alloc<int>(H);
        d_row_off = a.template alloc<int>(H);
        d_counters = a.template alloc<int>(2);
        d_pattern = a.template alloc<int>(LVI_KF_PAIRS);
        d_match = a.template alloc<char>(match_bytes);
        for (Slot& s : slots) {
            s.kp_xy = a.template alloc<float>(2 * (size_t)K);
            s.kp_norm = a.template alloc<float>(2 * (size_t)K);
            s.kp_desc = a.template alloc<ulonglong2>(2 * (size_t)K);
            s.win_xy = a.template alloc<float>(2 * (size_t)Wn);
            s.win_desc = a.template alloc<ulonglong2>(2 * (size_t)Wn);
        }
    }
};

namespace {

Slot* slot_of(lvi_kf* h, int32_t slot) { return h && slot >= 0 && slot < h->S ? &h->slots[slot] : nullptr; }

}  // namespace

namespace lvi {

bool kf_store_view(lvi_kf* h, KfStoreView* out)
{
    if (!h) return false;
    out->device = h->device; out->max_keypoints = h->K; out->stream = h->stream;
    return true;
}

bool kf_slot_view(lvi_kf* h, int32_t slot, KfSlotView* out)
{
    const Slot* s = slot_of(h, slot);
    if (!s) return false;
    out->valid = s->valid; out->n_kp = s->n_kp; out->kp_desc = s->kp_desc; out->generation = s->generation;
    return true;
}

}  // namespace lvi

extern "C" {

int32_t lvi_kf_abi_version(void) { return LVI_KF_ABI_VERSION; }

int32_t lvi_kf_create(int32_t device, int32_t max_width, int32_t max_height, int32_t max_keypoints, int32_t max_window, int32_t max_keyframes,
                      const int32_t* x1, const int32_t* y1, const int32_t* x2, const int32_t* y2, lvi_kf** out)
{
    if (!out) return fail(LVI_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (!x1 || !y1 || !x2 || !y2) return fail(LVI_ERR_INVALID_ARG, "null pattern");
    if (max_width < LVI_KF_MIN_SIDE || max_height < LVI_KF_MIN_SIDE || max_width > MAX_SIDE || max_height > MAX_SIDE)
        return fail(LVI_ERR_INVALID_ARG, "max_width / max_height must be 16..8192");
    if (max_keypoints < 1 || max_keypoints > (1 << 24) || max_window < 1 || max_window > (1 << 20) || max_keyframes < 1 || max_keyframes > (1 << 16))
        return fail(LVI_ERR_INVALID_ARG, "max_keypoints, max_window and max_keyframes must be positive (and at most 2^24, 2^20, 2^16)");
    int pattern[LVI_KF_PAIRS];
    for (int i = 0; i < LVI_KF_PAIRS; i++) {
        const int v[4] = {x1[i], y1[i], x2[i], y2[i]};
        for (int k = 0; k < 4; k++)
            if (v[k] < -LVI_KF_PATTERN_MAX || v[k] > LVI_KF_PATTERN_MAX) return fail(LVI_ERR_INVALID_ARG, "pattern offset beyond +-24");
        pattern[i] = (v[0] & 0xFF) | ((v[1] & 0xFF) << 8) | ((v[2] & 0xFF) << 16) | ((v[3] & 0xFF) << 24);
    }
    return create_handle(device, out, lvi_kf_destroy,
        [&](lvi_kf* h) {
            h->W = max_width; h->H = max_height; h->K = max_keypoints; h->Wn = max_window; h->S = max_keyframes;
            h->slots.resize(max_keyframes);
            h->off_img = align256(sizeof(float) * 2 * (size_t)h->Wn);
            h->in_bytes = h->off_img + (size_t)h->W * h->H;
            h->match_bytes = 9 * (size_t)h->Wn;
        },
        [&](lvi_kf* h) -> int32_t {
            h->open(device, [&](auto& dev, auto& pin) { h->layout(dev, pin); });
            LVI_HIP(hipMemcpyAsync(h->d_pattern, pattern, sizeof(pattern), hipMemcpyHostToDevice, h->stream));
            LVI_HIP(hipStreamSynchronize(h->stream));
            return LVI_OK;
        });
}

void lvi_kf_destroy(lvi_kf* h)
{
    if (!h) return;
    h->close();
    delete h;
}

int32_t lvi_kf_describe(lvi_kf* h, int32_t slot, const uint8_t* img, int32_t w, int32_t hgt, int32_t stride, const float* window_xy, int32_t n_window,
                        const lvi_mei_params* cam, lvi_kf_info* info_out)
{
    Slot* s = slot_of(h, slot);
    if (!s || !img) return fail(LVI_ERR_INVALID_ARG, "null handle or image, or slot out of range");
    if (w < LVI_KF_MIN_SIDE || hgt < LVI_KF_MIN_SIDE) return fail(LVI_ERR_INVALID_ARG, "image smaller than 16x16");
    if (w > h->W || hgt > h->H) return fail(LVI_ERR_INVALID_ARG, "image larger than the handle's capacity");
    if (stride < w) return fail(LVI_ERR_INVALID_ARG, "stride < width");
    if (n_window < 0 || n_window > h->Wn) return fail(LVI_ERR_INVALID_ARG, "n_window must be 0..max_window");
    if (n_window > 0 && !window_xy) return fail(LVI_ERR_INVALID_ARG, "null window points");
    return guarded(h->device, [&]() -> int32_t {
        if (n_window > 0) std::memcpy(h->h_in, window_xy, sizeof(float) * 2 * (size_t)n_window);
        uint8_t* stage = reinterpret_cast<uint8_t*>(h->h_in + h->off_img);
        for (int y = 0; y < hgt; y++) std::memcpy(stage + (size_t)y * w, img + (size_t)y * stride, (size_t)w);
        LVI_HIP(hipMemcpyAsync(h->d_in, h->h_in, h->off_img + (size_t)w * hgt, hipMemcpyHostToDevice, h->stream));
        const uint8_t* d_img = reinterpret_cast<const uint8_t*>(h->d_in + h->off_img);
        const float* d_win = reinterpret_cast<const float*>(h->d_in);
        s->valid = false; s->generation++;
        const dim3 tiles(div_up(w, TILE_W), div_up(hgt, TILE_H));
        hipLaunchKernelGGL(kf_blur_kernel, tiles, dim3(256), 0, h->stream, d_img, h->d_blur, w, hgt);
        LVI_HIP(hipGetLastError());
        hipLaunchKernelGGL(kf_fast_score_kernel, tiles, dim3(256), 0, h->stream, d_img, h->d_score, w, hgt);
        LVI_HIP(hipGetLastError());
        hipLaunchKernelGGL(kf_nms_kernel<false>, dim3(div_up(hgt, 4)), dim3(256), 0, h->stream, h->d_score, w, hgt, h->d_row_count, (float2*)nullptr, h->K);
        LVI_HIP(hipGetLastError());
        hipLaunchKernelGGL(kf_row_scan_kernel, dim3(1), dim3(1024), 0, h->stream, h->d_row_count, h->d_row_off, hgt, h->K, h->d_counters);
        LVI_HIP(hipGetLastError());
        hipLaunchKernelGGL(kf_nms_kernel<true>, dim3(div_up(hgt, 4)), dim3(256), 0, h->stream, h->d_score, w, hgt, h->d_row_off, reinterpret_cast<float2*>(s->kp_xy), h->K);
        LVI_HIP(hipGetLastError());
        if (n_window > 0) LVI_HIP(hipMemcpyAsync(s->win_xy, d_win, sizeof(float) * 2 * (size_t)n_window, hipMemcpyDeviceToDevice, h->stream));
        // the keypoint count is only known on the device: one wavefront per possible keypoint, the surplus leaves at once
        BriefArgs ba{h->d_blur, w, hgt, h->d_pattern, d_win, n_window, s->kp_xy, h->d_counters, s->win_desc, s->kp_desc};
        hipLaunchKernelGGL(kf_brief_kernel, dim3(div_up(n_window + h->K, 4)), dim3(256), 0, h->stream, ba);
        LVI_HIP(hipGetLastError());
        if (cam) {
            hipLaunchKernelGGL(kf_norm_kernel, dim3(div_up(h->K, 64)), dim3(64), 0, h->stream, *cam, s->kp_xy, h->d_counters, s->kp_norm);
            LVI_HIP(hipGetLastError());
        } else {
            LVI_HIP(hipMemsetAsync(s->kp_norm, 0, sizeof(float) * 2 * (size_t)h->K, h->stream));
        }
        LVI_HIP(hipMemcpyAsync(h->h_out, h->d_counters, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        LVI_HIP(hipStreamSynchronize(h->stream));
        const int* c = reinterpret_cast<const int*>(h->h_out);
        s->valid = true; s->n_kp = c[1]; s->n_win = n_window;
        h->last_w = w; h->last_h = hgt;
        if (info_out) { info_out->n_keypoints_found = c[0]; info_out->n_keypoints_stored = c[1]; info_out->n_window = n_window; info_out->reserved = 0; }
        return c[0] > c[1] ? LVI_KF_TRUNCATED : LVI_OK;
    });
}

int32_t lvi_kf_get(lvi_kf* h, int32_t slot, int32_t counts[2], float* kp_xy, float* kp_norm, uint64_t* kp_desc, float* win_xy, uint64_t* win_desc)
{
    Slot* s = slot_of(h, slot);
    if (!s) return fail(LVI_ERR_INVALID_ARG, "null handle or slot out of range");
    if (!s->valid) return fail(LVI_ERR_INVALID_ARG, "empty slot");
    return guarded(h->device, [&]() -> int32_t {
        if (counts) { counts[0] = s->n_kp; counts[1] = s->n_win; }
        const size_t k = (size_t)s->n_kp, n = (size_t)s->n_win;
        bool any = false;
        auto down = [&](void* dst, const void* src, size_t bytes) {
            if (!dst || !bytes) return;
            LVI_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
            any = true;
        };
        down(kp_xy, s->kp_xy, 8 * k); down(kp_norm, s->kp_norm, 8 * k); down(kp_desc, s->kp_desc, 32 * k);
        down(win_xy, s->win_xy, 8 * n); down(win_desc, s->win_desc, 32 * n);
        if (any) LVI_HIP(hipStreamSynchronize(h->stream));                    // a count query never waits
        return LVI_OK;
    });
}

int32_t lvi_kf_put(lvi_kf* h, int32_t slot, int32_t n_keypoints, const float* kp_xy, const float* kp_norm, const uint64_t* kp_desc, int32_t n_window,
                   const float* win_xy, const uint64_t* win_desc)
{
    Slot* s = slot_of(h, slot);
    if (!s) return fail(LVI_ERR_INVALID_ARG, "null handle or slot out of range");
    if (n_keypoints < 0 || n_keypoints > h->K || n_window < 0 || n_window > h->Wn) return fail(LVI_ERR_INVALID_ARG, "counts beyond the handle's capacity");
    return guarded(h->device, [&]() -> int32_t {
        const size_t k = (size_t)n_keypoints, n = (size_t)n_window;
        s->valid = false; s->generation++;
        auto up = [&](void* dst, const void* src, size_t bytes) {
            if (!bytes) return;
            if (src) LVI_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream));
            else LVI_HIP(hipMemsetAsync(dst, 0, bytes, h->stream));
        };
        up(s->kp_xy, kp_xy, 8 * k); up(s->kp_norm, kp_norm, 8 * k); up(s->kp_desc, kp_desc, 32 * k);
        up(s->win_xy, win_xy, 8 * n); up(s->win_desc, win_desc, 32 * n);
        LVI_HIP(hipStreamSynchronize(h->stream));
        s->valid = true; s->n_kp = n_keypoints; s->n_win = n_window;
        return LVI_OK;
    });
}

int32_t lvi_kf_release(lvi_kf* h, int32_t slot)
{
    Slot* s = slot_of(h, slot);
    if (!s) return fail(LVI_ERR_INVALID_ARG, "null handle or slot out of range");
    s->valid = false; s->n_kp = 0; s->n_win = 0; s->generation++;
    return LVI_OK;
}

int32_t lvi_kf_match(lvi_kf* h, int32_t cur_slot, int32_t old_slot, uint8_t* status_out, int32_t* index_out, int32_t* dist_out)
{
    Slot *c = slot_of(h, cur_slot), *o = slot_of(h, old_slot);
    if (!c || !o) return fail(LVI_ERR_INVALID_ARG, "null handle or slot out of range");
    if (!c->valid || !o->valid) return fail(LVI_ERR_INVALID_ARG, "empty or released slot");
    const int n = c->n_win;
    if (n == 0) return LVI_OK;
    return guarded(h->device, [&]() -> int32_t {
        int* d_index = reinterpret_cast<int*>(h->d_match);
        int* d_dist = d_index + h->Wn;
        uint8_t* d_status = reinterpret_cast<uint8_t*>(d_dist + h->Wn);
        hipLaunchKernelGGL(kf_match_kernel, dim3(n), dim3(256), 0, h->stream, c->win_desc, o->kp_desc, o->n_kp, d_index, d_dist, d_status);
        LVI_HIP(hipGetLastError());
        char* hm = h->h_out + 256;
        LVI_HIP(hipMemcpyAsync(hm, h->d_match, 8 * (size_t)h->Wn + (size_t)n, hipMemcpyDeviceToHost, h->stream));
        LVI_HIP(hipStreamSynchronize(h->stream));
        if (index_out) std::memcpy(index_out, hm, 4 * (size_t)n);
        if (dist_out) std::memcpy(dist_out, hm + 4 * (size_t)h->Wn, 4 * (size_t)n);
        if (status_out) std::memcpy(status_out, hm + 8 * (size_t)h->Wn, (size_t)n);
        return LVI_OK;
    });
}

int32_t lvi_kf_debug_maps(lvi_kf* h, uint8_t* blur, uint8_t* score, int32_t wh_out[2])
{
    if (!h) return fail(LVI_ERR_INVALID_ARG, "null handle");
    if (h->last_w == 0) return fail(LVI_ERR_STATE, "no describe yet");
    return guarded(h->device, [&]() -> int32_t {
        const size_t n = (size_t)h->last_w * h->last_h;
        if (wh_out) { wh_out[0] = h->last_w; wh_out[1] = h->last_h; }
        if (blur) LVI_HIP(hipMemcpyAsync(blur, h->d_blur, n, hipMemcpyDeviceToHost, h->stream));
        if (score) LVI_HIP(hipMemcpyAsync(score, h->d_score, n, hipMemcpyDeviceToHost, h->stream));
        LVI_HIP(hipStreamSynchronize(h->stream));
        return LVI_OK;
    });
}

}  // extern "C"
