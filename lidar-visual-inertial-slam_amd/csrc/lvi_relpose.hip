// lvi_relpose.hip — the initial two-view pose of vins_estimator's visual initialisation on the device (include/lvi_relpose.h,
// DESIGN §30).
//
// Two kernels.  relpose_cheirality runs on a grid of (point chunk, candidate), one wavefront per workgroup: every lane
// decomposes E itself (a few hundred flops on the same bits: the same candidates in every workgroup and on the host), then
// one lane per (point, candidate) runs the serial code of lvi_relpose_math.hpp: the 4 x 4 matrix of triangulatePoints, its
// null vector by lvi_fman_math::svd_null_vector and the four comparisons.  A lane writes its mask byte; the workgroup's
// count is the popcount of a ballot.  relpose_pick runs on one wavefront: it sums the counts (integers: their order is
// free), chooses, and writes the pose, the four candidates and the chosen mask.
//
// One call = one upload of the points and the mask (E and the threshold travel as kernel arguments), two launches, one
// download of the record and the five masks, one wait.
#include <cmath>
#include <cstring>

#include "../../include/lvi_relpose.h"
#include "lvi_dev.hpp"
#include "lvi_relpose_math.hpp"

using namespace lvi;
namespace rm = lvi_relpose_math;

static_assert(LVI_RELPOSE_DEGENERATE == rm::FLAG_DEGENERATE, "the flag of lvi_relpose_math.hpp");
static_assert(LVI_RELPOSE_CHUNK == 64, "one wavefront per chunk");
static_assert(sizeof(lvi_relpose_pose) == 8 * 15 + 4 * 8 && sizeof(rm::Pose) == sizeof(lvi_relpose_pose), "lvi_relpose_pose layout");

namespace {

constexpr int CHUNK = LVI_RELPOSE_CHUNK, CAND = rm::CANDIDATES;

struct Args {
    double E[9];
    double dist;
    int32_t n, chunks;
};

// what one call downloads: the record, then chosen [n] and masks [4][n] behind it
struct Out {
    lvi_relpose_pose pose;
    double cand[CAND][12];
};

__global__ __launch_bounds__(CHUNK) void relpose_cheirality(Args a, const float* __restrict__ pts, const uint8_t* __restrict__ in_mask,
                                                           uint8_t* __restrict__ masks, int32_t* __restrict__ counts)
{
    const int c = blockIdx.y, k = blockIdx.x * CHUNK + threadIdx.x;
    rm::Decomp D;
    rm::decompose(a.E, D);
    int bit = 0;
    if (k < a.n && !D.degenerate) {
        double P[3][4];
        rm::candidate(D, c, P);
        const lvi_f4 p = *(const lvi_f4*)(pts + 4 * (size_t)k);
        bit = rm::cheirality(P, (double)p.x, (double)p.y, (double)p.z, (double)p.w, a.dist) && in_mask[k] != 0;
    }
    if (k < a.n) masks[(size_t)c * a.n + k] = (uint8_t)bit;
    const uint64_t b = __ballot(bit);
    if (threadIdx.x == 0) counts[c * a.chunks + blockIdx.x] = __popcll(b);
}

__global__ __launch_bounds__(LVI_WAVE) void relpose_pick(Args a, const int32_t* __restrict__ counts, const uint8_t* __restrict__ masks,
                                                        Out* __restrict__ out, uint8_t* __restrict__ chosen_mask)
{
    const int lane = threadIdx.x;
    int good[CAND];
    for (int c = 0; c < CAND; c++) {
        int s = 0;
        for (int j = lane; j < a.chunks; j += LVI_WAVE) s += counts[c * a.chunks + j];
        good[c] = wave_sum(s);
    }
    const int ch = rm::choose(good);
    for (int k = lane; k < a.n; k += LVI_WAVE) chosen_mask[k] = masks[(size_t)ch * a.n + k];
    if (lane == 0) {
        rm::Decomp D;
        rm::decompose(a.E, D);
        for (int c = 0; c < CAND; c++) rm::candidate_record(D, c, out->cand[c]);
        rm::Pose p;
        rm::fill_pose(D, good, p);
        *reinterpret_cast<rm::Pose*>(&out->pose) = p;             // the same fields in the same order
    }
}

size_t out_bytes(int n) { return sizeof(Out) + (size_t)(CAND + 1) * n; }

}  // namespace

struct lvi_relpose : Handle {
    int max_points = 0, max_iters = 0;
    lvi_relpose_params P{};
    lvi_fmat* fmat = nullptr;
    float* d_pts = nullptr;                                     // one upload: pts [n][4] then mask [n], packed
    char* d_out = nullptr; int32_t* d_counts = nullptr;         // Out | chosen [n] | masks [4][n]
    char* h_up = nullptr; char* h_down = nullptr;               // pinned
    // the last recover that succeeded
    bool have_last = false; int last_n = 0;
    Out last{}; std::vector<uint8_t> last_masks;
    // solve's scratch
    std::vector<float> p1, p2; std::vector<uint8_t> status, mask;
};

namespace {

template <class A, class B> void carve(A& a, B& pin, lvi_relpose* h)
{
    const size_t mp = (size_t)h->max_points;
    h->d_pts = reinterpret_cast<float*>(a.template alloc<char>(17 * mp));
    h->d_out = a.template alloc<char>(out_bytes((int)mp));
    h->d_counts = a.template alloc<int32_t>((size_t)CAND * div_up((int)mp, CHUNK));
    h->h_up = pin.template alloc<char>(17 * mp);
    h->h_down = pin.template alloc<char>(out_bytes((int)mp));
}

void identity_result(lvi_relpose_result* r)
{
    std::memset(r, 0, sizeof(*r));
    r->Rotation[0] = r->Rotation[4] = r->Rotation[8] = 1.;
}

}  // namespace

extern "C" {

int32_t lvi_relpose_abi_version(void) { return LVI_RELPOSE_ABI_VERSION; }

void lvi_relpose_params_default(lvi_relpose_params* p)
{
    if (!p) return;
    p->threshold = 0.3 / 460; p->confidence = 0.99; p->distance_thresh = 50.0;
}

int32_t lvi_relpose_create(int32_t device, int32_t max_points, int32_t max_iters, lvi_relpose** out)
{
    if (!out) return fail(LVI_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (max_points < LVI_RELPOSE_MIN_POINTS || max_points > LVI_FMAT_MAX_POINTS)
        return fail(LVI_ERR_INVALID_ARG, "max_points is outside LVI_RELPOSE_MIN_POINTS..LVI_FMAT_MAX_POINTS");
    if (max_iters < 1 || max_iters > LVI_FMAT_MAX_ITERS) return fail(LVI_ERR_INVALID_ARG, "max_iters is outside 1..LVI_FMAT_MAX_ITERS");
    return create_handle(device, out, lvi_relpose_destroy,
        [&](lvi_relpose* h) { h->max_points = max_points; h->max_iters = max_iters; h->device = device; lvi_relpose_params_default(&h->P); },
        [&](lvi_relpose* h) -> int32_t {
            h->open(device, [&](auto& dev, auto& pin) { carve(dev, pin, h); });
            h->p1.resize(2 * (size_t)max_points); h->p2.resize(2 * (size_t)max_points); h->status.resize((size_t)max_points);
            return lvi_fmat_create(device, max_points, max_iters, &h->fmat);
        });
}

void lvi_relpose_destroy(lvi_relpose* h)
{
    if (!h) return;
    if (h->fmat) lvi_fmat_destroy(h->fmat);
    h->close();
    delete h;
}

int32_t lvi_relpose_set_params(lvi_relpose* h, const lvi_relpose_params* p)
{
    if (!h || !p) return fail(LVI_ERR_INVALID_ARG, "null argument");
    const double v[3] = {p->threshold, p->confidence, p->distance_thresh};
    if (!finite_n(v, 3) || !(p->threshold > 0) || !(p->confidence > 0 && p->confidence < 1) || !(p->distance_thresh > 0))
        return fail(LVI_ERR_INVALID_ARG, "the parameters must be finite, threshold > 0, 0 < confidence < 1, distance_thresh > 0");
    h->P = *p;
    return LVI_OK;
}

double lvi_relpose_average_parallax(const double* pairs, int32_t n) { return (pairs && n > 0) ? rm::average_parallax(pairs, n) : 0.; }

lvi_fmat* lvi_relpose_fmat(lvi_relpose* h) { return h ? h->fmat : nullptr; }

int32_t lvi_relpose_recover(lvi_relpose* h, const double* E, const float* pts1_xy, const float* pts2_xy, int32_t n, uint8_t* mask_inout, double distance_thresh,
                            lvi_relpose_pose* pose)
{
    if (!h || !E || !pts1_xy || !pts2_xy || !pose) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (n < 1 || n > h->max_points) return fail(LVI_ERR_INVALID_ARG, "n is outside 1..max_points");
    if (!std::isfinite(distance_thresh) || !(distance_thresh > 0)) return fail(LVI_ERR_INVALID_ARG, "distance_thresh must be finite and > 0");
    return guarded(h->device, [&]() -> int32_t {
        Args a;
        for (int k = 0; k < 9; k++) a.E[k] = E[k];
        a.dist = distance_thresh; a.n = n; a.chunks = div_up(n, CHUNK);
        float* up = reinterpret_cast<float*>(h->h_up);
        for (int k = 0; k < n; k++) {
            up[4 * k] = pts1_xy[2 * k]; up[4 * k + 1] = pts1_xy[2 * k + 1];
            up[4 * k + 2] = pts2_xy[2 * k]; up[4 * k + 3] = pts2_xy[2 * k + 1];
        }
        uint8_t* um = reinterpret_cast<uint8_t*>(h->h_up) + 16 * (size_t)n;
        for (int k = 0; k < n; k++) um[k] = mask_inout ? (mask_inout[k] != 0) : 1;
        LVI_HIP(hipMemcpyAsync(h->d_pts, h->h_up, 17 * (size_t)n, hipMemcpyHostToDevice, h->stream));
        const uint8_t* d_inmask = reinterpret_cast<const uint8_t*>(h->d_pts) + 16 * (size_t)n;
        Out* d_o = reinterpret_cast<Out*>(h->d_out);
        uint8_t* d_chosen = reinterpret_cast<uint8_t*>(h->d_out) + sizeof(Out);
        uint8_t* d_masks = d_chosen + n;
        hipLaunchKernelGGL(relpose_cheirality, dim3(a.chunks, CAND), dim3(CHUNK), 0, h->stream, a, h->d_pts, d_inmask, d_masks, h->d_counts);
        LVI_HIP(hipGetLastError());
        hipLaunchKernelGGL(relpose_pick, dim3(1), dim3(LVI_WAVE), 0, h->stream, a, h->d_counts, d_masks, d_o, d_chosen);
        LVI_HIP(hipGetLastError());
        LVI_HIP(hipMemcpyAsync(h->h_down, h->d_out, out_bytes(n), hipMemcpyDeviceToHost, h->stream));
        LVI_HIP(hipStreamSynchronize(h->stream));
        std::memcpy(&h->last, h->h_down, sizeof(Out));
        const uint8_t* dn = reinterpret_cast<const uint8_t*>(h->h_down) + sizeof(Out);
        h->last_masks.assign(dn + n, dn + (size_t)(CAND + 1) * n);
        h->last_n = n; h->have_last = true;
        *pose = h->last.pose;
        if (mask_inout) std::memcpy(mask_inout, dn, (size_t)n);
        return LVI_OK;
    });
}

int32_t lvi_relpose_solve(lvi_relpose* h, const double* pairs, int32_t n, lvi_relpose_result* result, uint8_t* status_out)
{
    if (!h || !result || (n > 0 && !pairs)) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (n < 0 || n > h->max_points) return fail(LVI_ERR_INVALID_ARG, "n is outside 0..max_points");
    lvi_relpose_result r;
    identity_result(&r);
    r.average_parallax = lvi_relpose_average_parallax(pairs, n);
    if (n < LVI_RELPOSE_MIN_POINTS) {                              // :195
        r.flags = LVI_RELPOSE_TOO_FEW;
        if (status_out) std::memset(status_out, 0, (size_t)n);
        *result = r;
        return LVI_OK;
    }
    for (int k = 0; k < n; k++) {                                  // cv::Point2f (:200-201)
        h->p1[2 * k] = (float)pairs[6 * k]; h->p1[2 * k + 1] = (float)pairs[6 * k + 1];
        h->p2[2 * k] = (float)pairs[6 * k + 3]; h->p2[2 * k + 1] = (float)pairs[6 * k + 4];
    }
    int32_t st = lvi_fmat_find(h->fmat, h->p1.data(), h->p2.data(), n, h->P.threshold, h->P.confidence, h->status.data(), &r.info);
    if (st != LVI_OK) return st;
    if (r.info.best_iter < 0) r.flags = LVI_RELPOSE_NO_MODEL;      // OpenCV would assert on the empty matrix
    else {
        h->mask = h->status;                                       // recover overwrites its mask: it works on a copy
        st = lvi_relpose_recover(h, r.info.F, h->p1.data(), h->p2.data(), n, h->mask.data(), h->P.distance_thresh, &r.pose);
        if (st != LVI_OK) return st;
        rm::invert_pose(r.pose.R, r.pose.t, r.Rotation, r.Translation);
        r.flags = r.pose.flags;
        r.ok = r.pose.n_inliers > LVI_RELPOSE_MIN_INLIERS;
    }
    if (status_out) std::memcpy(status_out, h->status.data(), (size_t)n);
    *result = r;
    return LVI_OK;
}

int32_t lvi_relpose_last(lvi_relpose* h, double* cand, uint8_t* masks, int32_t cap, int32_t* n_out)
{
    if (!h) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (!h->have_last) return fail(LVI_ERR_STATE, "no lvi_relpose_recover has succeeded yet");
    if (masks && cap < h->last_n) return fail(LVI_ERR_CAPACITY, "cap is smaller than the last n");
    if (n_out) *n_out = h->last_n;
    if (cand) std::memcpy(cand, h->last.cand, sizeof(h->last.cand));
    if (masks)
        for (int c = 0; c < CAND; c++) std::memcpy(masks + (size_t)c * cap, h->last_masks.data() + (size_t)c * h->last_n, (size_t)h->last_n);
    return LVI_OK;
}

}  // extern "C"
