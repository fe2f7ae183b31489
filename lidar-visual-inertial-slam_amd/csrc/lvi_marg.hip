// The marginalisation of vins_estimator's sliding window on the GPU (include/lvi_marg.h; the contract is DESIGN §21):
// preMarginalize + marginalize of marginalization_factor.cpp:110-129, 174-296 with the factors of estimator.cpp:813-976.
// All double.  With m dropped and n kept local columns, pos = m + n and P1 = pos + 1.  The augmented system A over the P1
// columns (sum J'J, b = sum J'r in its last column, the cost in its corner) comes from the front end shared with the window
// solve (lvi_winsys.hip); the prior's rows are written behind the dense rows the host sent.  Then:
//
//   marg_sym         Amm = (Amm + Amm') / 2 (:266), and the same for the Schur complement
//   marg_eigh        one workgroup: parallel cyclic two-sided Jacobi over the disjoint pairs of a round-robin schedule
//   marg_pinv        Amm_inv = V diag(lambda > eps ? 1 / lambda : 0) V' (:271)
//   marg_schur1/2    T = Amm_inv [Amr | bmm], then [Arr | brr] - Arm T (:274-280)
//   marg_refine_*    between the two: one step of iterative refinement of T, its residual summed in two doubles
//   marg_finish      one workgroup: eigenvalues ascending, linearized_jacobians = sqrt(S) V', linearized_residuals =
//                    sqrt(S_inv) V' b (:282-290) into the prior buffer that is not in use, keep_block_data beside them
// Once the flag says non-finite every later kernel returns at once, the host does not swap the prior buffers, and the
// previous prior stays.  No workgroup waits for another: what one launch writes, only later launches read.
#include <cmath>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "lvi_dev.hpp"
#include "lvi_marg_view.hpp"
#include "lvi_winsys.hpp"

using namespace lvi;
using namespace lvi_marg_math;
using namespace lvi_winsys;

namespace {

constexpr int EIG_THREADS = 1024;
constexpr int FIN_THREADS = 256;
struct DevInfo { int flags, sweeps[2], rank, rank_mm, pad; double off[2], cost; };

struct Dev {
    const double* vals; const ProjDev* proj; double* Jf; double* E; double* part; double* A;
    double *Wm, *Vm, *Minv, *T, *Rf, *S, *Wn, *Vn;
    const double *J0, *r0, *x0; const PriorBlk* pb;
    double *J1, *r1, *x1; const int* keepblk;
    DevInfo* info;
    int P, Rd, n0, nkb0, m, n, pos, P1, Cp, C, nkeep, loss_type, max_sweeps;
    double loss_a, eps; ProjConst pc;
};

// what the shared front end reads of d: no costs, flag bit 2, the corner of A is the cost
SysView sys_view(const Dev& d)
{
    return SysView{d.vals, d.proj, d.Jf, d.E, d.part, d.A, d.J0, d.r0, d.x0, d.pb, nullptr, &d.info->flags, 2, &d.info->cost,
                   d.P, d.Rd, d.Rd + d.n0, d.n0, d.nkb0, d.P1, d.Cp, d.C, 0, d.loss_type, d.loss_a, d.pc};
}

// W [dim][dim] = (B + B') / 2 of the dim x dim block of B (leading dimension ld) that starts at (o, o)
__global__ __launch_bounds__(256) void marg_sym(Dev d, const double* B, int ld, int o, double* W, int dim)
{
    if (d.info->flags & 2) return;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= dim * dim) return;
    const int i = e / dim, j = e % dim;
    W[e] = 0.5 * (B[(size_t)(o + i) * ld + o + j] + B[(size_t)(o + j) * ld + o + i]);
}

// Parallel cyclic two-sided Jacobi, one workgroup.  A sweep is dim' - 1 rounds (dim' = dim rounded up to even) of dim' / 2
// disjoint pairs (the round-robin schedule of a tournament: the last index stays, the others rotate); a pair is rotated
// when |a_pq| > delta = 2^-53 ||A||_F / dim.  Stopping rule: a sweep that rotated nothing, so every |a_pq| <= delta and the
// diagonal is within ||off||_F <= 2^-53 ||A||_F of the eigenvalues.  At most max_sweeps sweeps; hitting the bound raises
// flag bit 0.  On return the diagonal of W holds the eigenvalues and the columns of V the eigenvectors.
__global__ __launch_bounds__(EIG_THREADS) void marg_eigh(Dev d, double* W, double* V, int dim, int which)
{
    __shared__ double cc[LVI_MARG_MAX_DROP_DIM / 2], ss[LVI_MARG_MAX_DROP_DIM / 2], red[EIG_THREADS];
    __shared__ int pp[LVI_MARG_MAX_DROP_DIM / 2], qq[LVI_MARG_MAX_DROP_DIM / 2];
    __shared__ double sh_delta, sh_max;
    if (d.info->flags & 2) return;
    const int t = threadIdx.x, M = dim + (dim & 1), half = M / 2, rounds = M - 1;
    double s2 = 0.;
    for (int e = t; e < dim * dim; e += EIG_THREADS) {
        const double w = W[e];
        s2 += w * w;
        V[e] = (e / dim == e % dim) ? 1. : 0.;
    }
    red[t] = s2;
    __syncthreads();
    for (int o = EIG_THREADS / 2; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    if (t == 0) sh_delta = std::sqrt(red[0]) * 0x1p-53 / dim;
    __syncthreads();
    const double delta = sh_delta;
    int sweeps = 0;
    bool done = dim < 2 || !(delta > 0.);
    double last = 0.;
    while (!done && sweeps < d.max_sweeps) {
        double mymax = 0.;
        for (int k = 0; k < rounds; k++) {
            if (t < half) {
                int p = t == 0 ? M - 1 : (k + t) % (M - 1), q = (k + M - 1 - t) % (M - 1);
                if (p > q) { const int x = p; p = q; q = x; }
                double c = 1., s = 0.;
                int ok = -1;
                if (q < dim) {
                    const double apq = W[(size_t)p * dim + q], a = fabs(apq);
                    mymax = fmax(mymax, a);
                    if (a > delta) { jacobi_cs(W[(size_t)p * dim + p], W[(size_t)q * dim + q], apq, &c, &s); ok = p; }
                }
                pp[t] = ok; qq[t] = q; cc[t] = c; ss[t] = s;
            }
            __syncthreads();
            for (int e = t; e < half * dim; e += EIG_THREADS) {              // rows p, q <- J' A
                const int pr = e / dim, j = e % dim, p = pp[pr];
                if (p < 0) continue;
                const int q = qq[pr];
                const double c = cc[pr], s = ss[pr], a = W[(size_t)p * dim + j], b = W[(size_t)q * dim + j];
                W[(size_t)p * dim + j] = c * a - s * b;
                W[(size_t)q * dim + j] = s * a + c * b;
            }
            __syncthreads();
            for (int e = t; e < half * dim; e += EIG_THREADS) {              // columns p, q <- A J, V J
                const int i = e / half, pr = e % half, p = pp[pr];
                if (p < 0) continue;
                const int q = qq[pr];
                const double c = cc[pr], s = ss[pr];
                double a = W[(size_t)i * dim + p], b = W[(size_t)i * dim + q];
                W[(size_t)i * dim + p] = c * a - s * b;
                W[(size_t)i * dim + q] = s * a + c * b;
                a = V[(size_t)i * dim + p]; b = V[(size_t)i * dim + q];
                V[(size_t)i * dim + p] = c * a - s * b;
                V[(size_t)i * dim + q] = s * a + c * b;
            }
            __syncthreads();
            if (t < half && pp[t] >= 0) { W[(size_t)pp[t] * dim + qq[t]] = 0.; W[(size_t)qq[t] * dim + pp[t]] = 0.; }
            __syncthreads();
        }
        red[t] = mymax;
        __syncthreads();
        if (t == 0) {
            double mx = 0.;
            for (int k = 0; k < half; k++) mx = fmax(mx, red[k]);
            sh_max = mx;
        }
        for (int e = t; e < dim * dim; e += EIG_THREADS) {                   // keep the lower triangle the mirror of the upper
            const int i = e / dim, j = e % dim;
            if (i > j) W[e] = W[(size_t)j * dim + i];
        }
        __syncthreads();
        last = sh_max;
        sweeps++;
        done = !(last > delta);
        __syncthreads();
    }
    if (t == 0) {
        d.info->sweeps[which] = sweeps;
        d.info->off[which] = last;
        if (!done) atomicOr(&d.info->flags, 1);
    }
}

__global__ __launch_bounds__(256) void marg_pinv(Dev d)
{
    if (d.info->flags & 2) return;
    const int m = d.m, e = blockIdx.x * 256 + threadIdx.x;
    if (e >= m * m) return;
    const int i = e / m, j = e % m;
    double s = 0.;
    for (int k = 0; k < m; k++) {
        const double l = d.Wm[(size_t)k * m + k];
        if (l > d.eps) s += d.Vm[(size_t)i * m + k] * (1. / l) * d.Vm[(size_t)j * m + k];
    }
    d.Minv[e] = s;
}

__global__ __launch_bounds__(256) void marg_schur1(Dev d)
{
    if (d.info->flags & 2) return;
    const int m = d.m, n1 = d.n + 1, e = blockIdx.x * 256 + threadIdx.x;
    if (e >= m * n1) return;
    const int i = e / n1, j = e % n1;
    double s = 0.;
    for (int k = 0; k < m; k++) s += d.Minv[(size_t)i * m + k] * d.A[(size_t)k * d.P1 + m + j];
    d.T[e] = s;
}

// One step of iterative refinement of T against the rounding of the eigen-solver: R = [Amr | bmm] - Amm T with the sum
// carried in two doubles (error-free products and sums), then T += Amm_inv R.  The pseudo-inverse ignores what R has
// outside the kept eigenspace, so the refined T solves the same thresholded system.
__global__ __launch_bounds__(256) void marg_refine_res(Dev d)
{
    if (d.info->flags & 2) return;
    const int m = d.m, n1 = d.n + 1, e = blockIdx.x * 256 + threadIdx.x;
    if (e >= m * n1) return;
    const int i = e / n1, j = e % n1;
    double s = d.A[(size_t)i * d.P1 + m + j], c = 0.;
    for (int k = 0; k < m; k++) {
        const double a = 0.5 * (d.A[(size_t)i * d.P1 + k] + d.A[(size_t)k * d.P1 + i]), t = d.T[(size_t)k * n1 + j];
        const double p = a * t, pe = fma(a, t, -p);            // a t = p + pe exactly
        const double x = s - p, bb = x - s, se = (s - (x - bb)) + (-p - bb);      // s - p = x + se exactly
        s = x;
        c += se - pe;
    }
    d.Rf[e] = s + c;
}

__global__ __launch_bounds__(256) void marg_refine_add(Dev d)
{
    if (d.info->flags & 2) return;
    const int m = d.m, n1 = d.n + 1, e = blockIdx.x * 256 + threadIdx.x;
    if (e >= m * n1) return;
    const int i = e / n1, j = e % n1;
    double s = 0.;
    for (int k = 0; k < m; k++) s += d.Minv[(size_t)i * m + k] * d.Rf[(size_t)k * n1 + j];
    d.T[e] += s;
}

__global__ __launch_bounds__(256) void marg_schur2(Dev d)
{
    if (d.info->flags & 2) return;
    const int m = d.m, n1 = d.n + 1, e = blockIdx.x * 256 + threadIdx.x;
    if (e >= d.n * n1) return;
    const int i = e / n1, j = e % n1;
    double s = 0.;
    for (int k = 0; k < m; k++) s += d.A[(size_t)(m + i) * d.P1 + k] * d.T[(size_t)k * n1 + j];
    d.S[e] = d.A[(size_t)(m + i) * d.P1 + m + j] - s;
}

__global__ __launch_bounds__(FIN_THREADS) void marg_finish(Dev d)
{
    __shared__ int rank, rank_mm, bad;
    if (d.info->flags & 2) return;
    const int t = threadIdx.x, n = d.n, n1 = n + 1;
    if (t == 0) { rank = 0; rank_mm = 0; bad = 0; }
    __syncthreads();
    for (int k = t; k < d.m; k += FIN_THREADS)
        if (d.Wm[(size_t)k * d.m + k] > d.eps) atomicAdd(&rank_mm, 1);
    for (int k = t; k < n; k += FIN_THREADS) {
        const double l = d.Wn[(size_t)k * n + k];
        int at = 0;
        for (int j = 0; j < n; j++) {
            const double lj = d.Wn[(size_t)j * n + j];
            if (lj < l || (lj == l && j < k)) at++;
        }
        const bool keep = l > d.eps;
        const double sq = keep ? std::sqrt(l) : 0., si = keep ? std::sqrt(1. / l) : 0.;
        double vb = 0.;
        int nf = isfinite(l) ? 0 : 1;
        for (int j = 0; j < n; j++) {
            const double v = d.Vn[(size_t)j * n + k], o = sq * v;
            d.J1[(size_t)at * n + j] = o;
            vb += v * d.S[(size_t)j * n1 + n];
            if (!isfinite(o)) nf = 1;
        }
        const double rr = si * vb;
        d.r1[at] = rr;
        if (!isfinite(rr)) nf = 1;
        if (nf) atomicOr(&bad, 1);
        if (keep) atomicAdd(&rank, 1);
    }
    for (int e = t; e < d.nkeep * VAL; e += FIN_THREADS) d.x1[e] = d.vals[(size_t)VAL * d.keepblk[e / VAL] + e % VAL];
    __syncthreads();
    if (t == 0) {
        d.info->rank = rank; d.info->rank_mm = rank_mm;
        if (bad) atomicOr(&d.info->flags, 2);
    }
}

struct Block { int id, size; double v[VAL]; int seen, drop; };
struct Dense { int rows; std::vector<int> blk, drop; std::vector<double> r, J; };      // J: per block row-major [rows][local size]
struct Prior { bool valid = false; int m = 0, n = 0; std::vector<int> ids, sizes, col; std::vector<double> x0; lvi_marg_info info{}; };

}  // namespace

struct lvi_marg : Handle {
    lvi_marg_caps caps{};
    lvi_marg_params P{};
    Dev d{};
    double *d_vals = nullptr, *d_J[2] = {nullptr, nullptr}, *d_r[2] = {nullptr, nullptr}, *d_x[2] = {nullptr, nullptr};
    ProjDev* d_proj = nullptr; PriorBlk* d_pb = nullptr; int* d_keepblk = nullptr;
    // pinned staging
    double *h_vals = nullptr, *h_E = nullptr; ProjDev* h_proj = nullptr; PriorBlk* h_pb = nullptr; int* h_keepblk = nullptr; DevInfo* h_info = nullptr;
    double* h_out = nullptr;
    // the description
    std::vector<Block> blocks; std::unordered_map<int, int> index; int seq = 0;
    std::vector<lvi_marg_projection> proj;
    std::vector<Dense> dense; int dense_rows = 0;
    bool use_prior = false;
    // the prior in use and the system of the last call
    Prior prior; int cur = 0;
    int sys_pos = 0; bool sys_valid = false;
};

namespace {

int Pmax(const lvi_marg* h) { return h->caps.max_drop_dim + h->caps.max_keep_dim + 1; }
int max_chunks(const lvi_marg* h)
{
    return div_up(h->caps.max_projections, SHARE) + div_up(h->caps.max_dense_rows + h->caps.max_keep_dim, CH_ROWS) + 1;
}

template <class A, class B> void carve(A& a, B& pin, lvi_marg* h)
{
    const size_t Pm = (size_t)Pmax(h), mm = (size_t)h->caps.max_drop_dim, nn = (size_t)h->caps.max_keep_dim, R = (size_t)h->caps.max_dense_rows + nn;
    Dev& d = h->d;
    alloc_pair(a, pin, h->d_vals, h->h_vals, (size_t)VAL * h->caps.max_blocks);
    alloc_pair(a, pin, h->d_proj, h->h_proj, (size_t)h->caps.max_projections);
    d.Jf = a.template alloc<double>((size_t)JF * h->caps.max_projections);
    alloc_pair(a, pin, d.E, h->h_E, R * Pm);
    d.part = a.template alloc<double>((size_t)max_chunks(h) * Pm * Pm);
    alloc_pair(a, pin, d.A, h->h_out, Pm * Pm);
    d.Wm = a.template alloc<double>(mm * mm); d.Vm = a.template alloc<double>(mm * mm); d.Minv = a.template alloc<double>(mm * mm);
    d.T = a.template alloc<double>(mm * (nn + 1)); d.Rf = a.template alloc<double>(mm * (nn + 1)); d.S = a.template alloc<double>(nn * (nn + 1));
    d.Wn = a.template alloc<double>(nn * nn); d.Vn = a.template alloc<double>(nn * nn);
    for (int k = 0; k < 2; k++) {
        h->d_J[k] = a.template alloc<double>(nn * nn); h->d_r[k] = a.template alloc<double>(nn); h->d_x[k] = a.template alloc<double>((size_t)VAL * nn);
    }
    alloc_pair(a, pin, h->d_pb, h->h_pb, nn); alloc_pair(a, pin, h->d_keepblk, h->h_keepblk, nn);
    alloc_pair(a, pin, d.info, h->h_info, 1);
}

bool params_ok(const lvi_marg_params& p)
{
    return p.loss_type >= LVI_MARG_LOSS_NONE && p.loss_type <= LVI_MARG_LOSS_HUBER && p.max_sweeps >= 1 && p.max_sweeps <= LVI_MARG_MAX_SWEEPS &&
           p.loss_a > 0. && std::isfinite(p.loss_a) && p.sqrt_info > 0. && std::isfinite(p.sqrt_info) && std::isfinite(p.tr_over_row) &&
           std::isfinite(p.half_row) && p.eps >= 0. && std::isfinite(p.eps);
}

int find(const lvi_marg* h, int id)
{
    const auto it = h->index.find(id);
    return it == h->index.end() ? -1 : it->second;
}
void appear(lvi_marg* h, int b, bool drop)
{
    Block& k = h->blocks[b];
    if (k.seen < 0) k.seen = h->seq;
    if (drop && k.drop < 0) k.drop = h->seq;
    h->seq++;
}

}  // namespace

// the resident prior for the window solve (lvi_win_set_prior_from_marg): pointers into the buffers in use, nothing is copied
bool lvi::marg_prior_view(lvi_marg* h, lvi::MargPriorView* out)
{
    if (!h || !out || !h->prior.valid) return false;
    const Prior& p = h->prior;
    out->device = h->device; out->n = p.n; out->count = (int)p.ids.size();
    out->J = h->d_J[h->cur]; out->r = h->d_r[h->cur]; out->x0 = h->d_x[h->cur];
    out->ids = p.ids.data(); out->sizes = p.sizes.data(); out->col = p.col.data();
    return true;
}

extern "C" {

int32_t lvi_marg_abi_version(void) { return LVI_MARG_ABI_VERSION; }

void lvi_marg_params_default(lvi_marg_params* p)
{
    if (!p) return;
    p->loss_type = LVI_MARG_LOSS_CAUCHY; p->max_sweeps = 30; p->loss_a = 1.0; p->sqrt_info = 460.0 / 1.5; p->tr_over_row = 0.; p->half_row = 240.; p->eps = 1e-8;
}

int32_t lvi_marg_create(int32_t device, const lvi_marg_caps* caps, lvi_marg** out)
{
    if (!out || !caps) return fail(LVI_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    const lvi_marg_caps& c = *caps;
    if (c.max_blocks < 1 || c.max_blocks > LVI_MARG_MAX_BLOCKS || c.max_projections < 1 || c.max_projections > LVI_MARG_MAX_PROJECTIONS ||
        c.max_dense_factors < 0 || c.max_dense_factors > LVI_MARG_MAX_DENSE_FACTORS || c.max_dense_rows < 0 || c.max_dense_rows > LVI_MARG_MAX_DENSE_ROWS ||
        c.max_drop_dim < 1 || c.max_drop_dim > LVI_MARG_MAX_DROP_DIM || c.max_keep_dim < 1 || c.max_keep_dim > LVI_MARG_MAX_KEEP_DIM)
        return fail(LVI_ERR_INVALID_ARG, "a capacity is outside 1..LVI_MARG_MAX_*");
    return create_handle(device, out, lvi_marg_destroy,
        [&](lvi_marg* h) { h->caps = c; lvi_marg_params_default(&h->P); },
        [&](lvi_marg* h) -> int32_t { h->open(device, [&](auto& dev, auto& pin) { carve(dev, pin, h); }); return LVI_OK; });
}

void lvi_marg_destroy(lvi_marg* h)
{
    if (!h) return;
    h->close();
    delete h;
}

int32_t lvi_marg_begin(lvi_marg* h)
{
    if (!h) return fail(LVI_ERR_INVALID_ARG, "null argument");
    h->blocks.clear(); h->index.clear(); h->seq = 0; h->proj.clear(); h->dense.clear(); h->dense_rows = 0; h->use_prior = false;
    return LVI_OK;
}

int32_t lvi_marg_clear(lvi_marg* h)
{
    if (!h) return fail(LVI_ERR_INVALID_ARG, "null argument");
    lvi_marg_begin(h);
    h->prior = Prior(); h->sys_valid = false;
    return LVI_OK;
}

int32_t lvi_marg_set_params(lvi_marg* h, const lvi_marg_params* p)
{
    if (!h || !p) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (!params_ok(*p)) return fail(LVI_ERR_INVALID_ARG, "loss_type must be LVI_MARG_LOSS_*, max_sweeps 1..LVI_MARG_MAX_SWEEPS, loss_a and sqrt_info > 0, eps >= 0");
    h->P = *p;
    return LVI_OK;
}

int32_t lvi_marg_set_block(lvi_marg* h, int32_t id, int32_t size, const double* values)
{
    if (!h || !values) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (size < 1 || size > LVI_MARG_MAX_BLOCK_SIZE) return fail(LVI_ERR_INVALID_ARG, "block size must be 1..LVI_MARG_MAX_BLOCK_SIZE");
    if (!finite_all(values, (size_t)size)) return fail(LVI_ERR_INVALID_ARG, "a block value is not finite");
    int b = find(h, id);
    if (b >= 0 && h->blocks[b].size != size) return fail(LVI_ERR_INVALID_ARG, "the id was declared with another size");
    if (b < 0) {
        if ((int)h->blocks.size() >= h->caps.max_blocks) return fail(LVI_ERR_CAPACITY, "more parameter blocks than max_blocks");
        Block k{};
        k.id = id; k.size = size; k.seen = -1; k.drop = -1;
        b = (int)h->blocks.size();
        h->blocks.push_back(k);
        h->index[id] = b;
    }
    for (int k = 0; k < VAL; k++) h->blocks[b].v[k] = k < size ? values[k] : 0.;
    return LVI_OK;
}

int32_t lvi_marg_add_projection(lvi_marg* h, int32_t count, const lvi_marg_projection* recs)
{
    if (!h || (count > 0 && !recs)) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (count < 0) return fail(LVI_ERR_INVALID_ARG, "negative count");
    if ((size_t)count + h->proj.size() > (size_t)h->caps.max_projections) return fail(LVI_ERR_CAPACITY, "more projection factors than max_projections");
    const auto look = [&](int id) { const int b = find(h, id); return BlockRef{b, b < 0 ? 0 : h->blocks[b].size, false}; };
    for (int f = 0; f < count; f++) {
        const char* why = nullptr;
        const int32_t st = check_projection(recs[f], look, false, &why);
        if (st != LVI_OK) return fail(st, why);
    }
    for (int f = 0; f < count; f++) {
        const lvi_marg_projection& p = recs[f];
        const int ids[5] = {p.pose_i, p.pose_j, p.ex, p.feature, p.td};
        for (int k = 0; k < 5; k++)
            if (!(k == 4 && p.td == -1)) appear(h, find(h, ids[k]), k == 0 || k == 3);
        h->proj.push_back(p);
    }
    return LVI_OK;
}

int32_t lvi_marg_add_dense(lvi_marg* h, int32_t n_rows, int32_t n_blocks, const int32_t* ids, const double* residual, const double* jacobians, const int32_t* drop_mask)
{
    if (!h || !ids || !residual || !jacobians || !drop_mask) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (n_rows < 1 || n_blocks < 1) return fail(LVI_ERR_INVALID_ARG, "a dense factor needs rows and blocks");
    if ((int)h->dense.size() >= h->caps.max_dense_factors || h->dense_rows + n_rows > h->caps.max_dense_rows)
        return fail(LVI_ERR_CAPACITY, "more dense factors or rows than max_dense_factors / max_dense_rows");
    Dense D;
    D.rows = n_rows;
    size_t at = 0;
    for (int k = 0; k < n_blocks; k++) {
        const int b = find(h, ids[k]);
        if (b < 0) return fail(LVI_ERR_INVALID_ARG, "a dense factor names an id that was not declared");
        for (int j : D.blk) if (j == b) return fail(LVI_ERR_INVALID_ARG, "a dense factor names one block twice");
        const int size = h->blocks[b].size, ls = local_size(size);
        if (!finite_all(jacobians + at, (size_t)n_rows * size)) return fail(LVI_ERR_INVALID_ARG, "a dense Jacobian is not finite");
        for (int r = 0; r < n_rows; r++)
            for (int c = 0; c < ls; c++) D.J.push_back(jacobians[at + (size_t)r * size + c]);
        at += (size_t)n_rows * size;
        D.blk.push_back(b);
        D.drop.push_back(drop_mask[k] != 0);
    }
    if (!finite_all(residual, (size_t)n_rows)) return fail(LVI_ERR_INVALID_ARG, "a dense residual is not finite");
    D.r.assign(residual, residual + n_rows);
    for (size_t k = 0; k < D.blk.size(); k++) appear(h, D.blk[k], D.drop[k] != 0);
    h->dense_rows += n_rows;
    h->dense.push_back(std::move(D));
    return LVI_OK;
}

int32_t lvi_marg_add_last_prior(lvi_marg* h, int32_t n_drop, const int32_t* drop_ids)
{
    if (!h || (n_drop > 0 && !drop_ids)) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (n_drop < 0) return fail(LVI_ERR_INVALID_ARG, "negative count");
    if (!h->prior.valid) return fail(LVI_ERR_STATE, "no previous result");
    if (h->use_prior) return fail(LVI_ERR_STATE, "the previous result was added already");
    const Prior& p = h->prior;
    std::vector<int> b(p.ids.size());
    for (size_t k = 0; k < p.ids.size(); k++) {
        b[k] = find(h, p.ids[k]);
        if (b[k] < 0) return fail(LVI_ERR_INVALID_ARG, "a kept block of the previous result was not declared");
        if (h->blocks[b[k]].size != p.sizes[k]) return fail(LVI_ERR_INVALID_ARG, "a kept block of the previous result was declared with another size");
    }
    std::vector<char> drop(p.ids.size(), 0);
    for (int j = 0; j < n_drop; j++) {
        size_t k = 0;
        while (k < p.ids.size() && p.ids[k] != drop_ids[j]) k++;
        if (k == p.ids.size()) return fail(LVI_ERR_INVALID_ARG, "a drop id is not a kept block of the previous result");
        drop[k] = 1;
    }
    for (size_t k = 0; k < p.ids.size(); k++) appear(h, b[k], drop[k] != 0);
    h->use_prior = true;
    return LVI_OK;
}

int32_t lvi_marg_marginalize(lvi_marg* h, lvi_marg_info* info_out)
{
    if (!h) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (h->proj.empty() && h->dense.empty() && !h->use_prior) return fail(LVI_ERR_STATE, "no factors");
    // the order: dropped blocks by first appearance in a drop set, then kept blocks by first appearance; a block no factor
    // names is not part of the system, as in the reference
    const int nb = (int)h->blocks.size();
    std::vector<int> order;
    for (int pass = 0; pass < 2; pass++) {
        std::vector<std::pair<int, int>> key;
        for (int b = 0; b < nb; b++) {
            const Block& k = h->blocks[b];
            if (pass == 0 && k.drop >= 0) key.push_back({k.drop, b});
            if (pass == 1 && k.drop < 0 && k.seen >= 0) key.push_back({k.seen, b});
        }
        std::sort(key.begin(), key.end());
        for (const auto& kv : key) order.push_back(kv.second);
    }
    std::vector<int> col(nb, 0);
    int m = 0, pos = 0;
    std::vector<int> kept;
    for (int b : order) {
        col[b] = pos;
        pos += local_size(h->blocks[b].size);
        if (h->blocks[b].drop >= 0) m = pos; else kept.push_back(b);
    }
    const int n = pos - m;
    if (m == 0 || n == 0) return fail(LVI_ERR_STATE, "nothing is dropped or nothing is kept");
    if (m > h->caps.max_drop_dim || n > h->caps.max_keep_dim) return fail(LVI_ERR_CAPACITY, "m or n beyond max_drop_dim / max_keep_dim");
    if (h->use_prior)
        for (int id : h->prior.ids)
            if (find(h, id) < 0) return fail(LVI_ERR_STATE, "a kept block of the previous result is no longer declared");
    return guarded(h->device, [&]() -> int32_t {
        hipStream_t s = h->stream;
        const int P1 = pos + 1, P = (int)h->proj.size(), Rd = h->dense_rows, nxt = 1 - h->cur;
        const Prior& pr = h->prior;
        for (int b = 0; b < nb; b++) std::memcpy(h->h_vals + (size_t)VAL * b, h->blocks[b].v, sizeof(double) * VAL);
        const auto fnd = [&](int id) { return find(h, id); };
        for (int f = 0; f < P; f++) stage_projection(h->proj[f], fnd, col.data(), h->h_proj[f]);
        int row = 0;
        for (const Dense& D : h->dense) {
            size_t at = 0;
            for (int r = 0; r < D.rows; r++) {
                double* e = h->h_E + (size_t)(row + r) * P1;
                for (int j = 0; j < P1; j++) e[j] = 0.;
                e[pos] = D.r[r];
            }
            for (size_t k = 0; k < D.blk.size(); k++) {
                const int ls = local_size(h->blocks[D.blk[k]].size);
                for (int r = 0; r < D.rows; r++)
                    for (int c = 0; c < ls; c++) h->h_E[(size_t)(row + r) * P1 + col[D.blk[k]] + c] = D.J[at + (size_t)r * ls + c];
                at += (size_t)D.rows * ls;
            }
            row += D.rows;
        }
        const int n0 = h->use_prior ? pr.n : 0, nkb0 = h->use_prior ? (int)pr.ids.size() : 0;
        stage_prior_blocks(nkb0, pr.ids.data(), pr.sizes.data(), pr.col.data(), fnd, col.data(), h->h_pb);
        for (size_t k = 0; k < kept.size(); k++) h->h_keepblk[k] = kept[k];

        Dev d = h->d;
        d.vals = h->d_vals; d.proj = h->d_proj; d.pb = h->d_pb; d.keepblk = h->d_keepblk;
        d.J0 = h->d_J[h->cur]; d.r0 = h->d_r[h->cur]; d.x0 = h->d_x[h->cur];
        d.J1 = h->d_J[nxt]; d.r1 = h->d_r[nxt]; d.x1 = h->d_x[nxt];
        d.P = P; d.Rd = Rd; d.n0 = n0; d.nkb0 = nkb0; d.m = m; d.n = n; d.pos = pos; d.P1 = P1;
        d.Cp = div_up(P, SHARE); d.C = d.Cp + div_up(Rd + n0, CH_ROWS); d.nkeep = (int)kept.size();
        d.loss_type = h->P.loss_type; d.max_sweeps = h->P.max_sweeps; d.loss_a = h->P.loss_a; d.eps = h->P.eps;
        d.pc = ProjConst{h->P.sqrt_info, h->P.tr_over_row, h->P.half_row};

        LVI_HIP(hipMemcpyAsync(h->d_vals, h->h_vals, sizeof(double) * VAL * nb, hipMemcpyHostToDevice, s));
        if (P > 0) LVI_HIP(hipMemcpyAsync(h->d_proj, h->h_proj, sizeof(ProjDev) * P, hipMemcpyHostToDevice, s));
        if (Rd > 0) LVI_HIP(hipMemcpyAsync(d.E, h->h_E, sizeof(double) * (size_t)Rd * P1, hipMemcpyHostToDevice, s));
        if (nkb0 > 0) LVI_HIP(hipMemcpyAsync(h->d_pb, h->h_pb, sizeof(PriorBlk) * nkb0, hipMemcpyHostToDevice, s));
        LVI_HIP(hipMemcpyAsync(h->d_keepblk, h->h_keepblk, sizeof(int) * kept.size(), hipMemcpyHostToDevice, s));
        LVI_HIP(hipMemsetAsync(d.info, 0, sizeof(DevInfo), s));
        const SysView v = sys_view(d);
        launch_eval_proj(v, s, 1);
        launch_prior_rows(v, s, 1);
        launch_build(v, s);
        hipLaunchKernelGGL(marg_sym, dim3(div_up(m * m, 256)), dim3(256), 0, s, d, (const double*)d.A, P1, 0, d.Wm, m);
        hipLaunchKernelGGL(marg_eigh, dim3(1), dim3(EIG_THREADS), 0, s, d, d.Wm, d.Vm, m, 0);
        hipLaunchKernelGGL(marg_pinv, dim3(div_up(m * m, 256)), dim3(256), 0, s, d);
        hipLaunchKernelGGL(marg_schur1, dim3(div_up(m * (n + 1), 256)), dim3(256), 0, s, d);
        hipLaunchKernelGGL(marg_refine_res, dim3(div_up(m * (n + 1), 256)), dim3(256), 0, s, d);
        hipLaunchKernelGGL(marg_refine_add, dim3(div_up(m * (n + 1), 256)), dim3(256), 0, s, d);
        hipLaunchKernelGGL(marg_schur2, dim3(div_up(n * (n + 1), 256)), dim3(256), 0, s, d);
        hipLaunchKernelGGL(marg_sym, dim3(div_up(n * n, 256)), dim3(256), 0, s, d, (const double*)d.S, n + 1, 0, d.Wn, n);
        hipLaunchKernelGGL(marg_eigh, dim3(1), dim3(EIG_THREADS), 0, s, d, d.Wn, d.Vn, n, 1);
        hipLaunchKernelGGL(marg_finish, dim3(1), dim3(FIN_THREADS), 0, s, d);
        LVI_HIP(hipGetLastError());
        LVI_HIP(hipMemcpyAsync(h->h_info, d.info, sizeof(DevInfo), hipMemcpyDeviceToHost, s));
        LVI_HIP(hipStreamSynchronize(s));                            // the call's one wait
        const DevInfo& di = *h->h_info;
        lvi_marg_info info{};
        info.m = m; info.n = n; info.rank = di.rank; info.rank_mm = di.rank_mm; info.sweeps_mm = di.sweeps[0]; info.sweeps_rr = di.sweeps[1];
        info.flags = di.flags; info.kept_blocks = (int)kept.size(); info.cost = di.cost; info.off_mm = di.off[0]; info.off_rr = di.off[1];
        if (info_out) *info_out = info;
        h->sys_pos = pos; h->sys_valid = true;
        if (di.flags & 2) return LVI_MARG_NOT_FINITE;
        Prior np;
        np.valid = true; np.m = m; np.n = n; np.info = info;
        for (int b : kept) {
            const Block& k = h->blocks[b];
            np.ids.push_back(k.id); np.sizes.push_back(k.size); np.col.push_back(col[b] - m);
            np.x0.insert(np.x0.end(), k.v, k.v + VAL);
        }
        h->prior = std::move(np);
        h->cur = nxt;
        lvi_marg_begin(h);
        return (di.flags & 1) ? LVI_MARG_EIG_NOT_CONVERGED : LVI_OK;
    });
}

int32_t lvi_marg_get_layout(lvi_marg* h, lvi_marg_info* info, int32_t cap, int32_t* count, int32_t* ids, int32_t* sizes, int32_t* idx, double* values)
{
    if (!h) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (!h->prior.valid) return fail(LVI_ERR_STATE, "no result");
    const Prior& p = h->prior;
    const int nk = (int)p.ids.size();
    if ((ids || sizes || idx || values) && cap < nk) return fail(LVI_ERR_CAPACITY, "the arrays are shorter than the kept blocks");
    if (info) *info = p.info;
    if (count) *count = nk;
    for (int k = 0; k < nk; k++) {
        if (ids) ids[k] = p.ids[k];
        if (sizes) sizes[k] = p.sizes[k];
        if (idx) idx[k] = p.m + p.col[k];
        if (values) std::memcpy(values + (size_t)VAL * k, p.x0.data() + (size_t)VAL * k, sizeof(double) * VAL);
    }
    return LVI_OK;
}

int32_t lvi_marg_get_prior(lvi_marg* h, double* jacobians, double* residuals)
{
    if (!h) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (!h->prior.valid) return fail(LVI_ERR_STATE, "no result");
    return guarded(h->device, [&]() -> int32_t {
        const size_t n = (size_t)h->prior.n;
        LVI_HIP(hipMemcpyAsync(h->h_out, h->d_J[h->cur], sizeof(double) * n * n, hipMemcpyDeviceToHost, h->stream));
        LVI_HIP(hipMemcpyAsync(h->h_out + n * n, h->d_r[h->cur], sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
        LVI_HIP(hipStreamSynchronize(h->stream));
        if (jacobians) std::memcpy(jacobians, h->h_out, sizeof(double) * n * n);
        if (residuals) std::memcpy(residuals, h->h_out + n * n, sizeof(double) * n);
        return LVI_OK;
    });
}

int32_t lvi_marg_remap(lvi_marg* h, const int32_t* old_ids, const int32_t* new_ids, int32_t count)
{
    if (!h || (count > 0 && (!old_ids || !new_ids))) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (count < 0) return fail(LVI_ERR_INVALID_ARG, "negative count");
    if (!h->prior.valid) return fail(LVI_ERR_STATE, "no result");
    if (h->use_prior) return fail(LVI_ERR_STATE, "the result is part of the description under its present ids: remap before lvi_marg_add_last_prior or after lvi_marg_marginalize");
    std::vector<int> ids = h->prior.ids;
    for (size_t k = 0; k < ids.size(); k++)
        for (int j = 0; j < count; j++)
            if (h->prior.ids[k] == old_ids[j]) { ids[k] = new_ids[j]; break; }
    for (size_t k = 0; k < ids.size(); k++)
        for (size_t j = 0; j < k; j++)
            if (ids[j] == ids[k]) return fail(LVI_ERR_INVALID_ARG, "two kept blocks under one id");
    h->prior.ids = ids;
    return LVI_OK;
}

int32_t lvi_marg_debug_system(lvi_marg* h, int32_t cap, int32_t* pos_out, double* A, double* b)
{
    if (!h) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (!h->sys_valid) return fail(LVI_ERR_STATE, "no system");
    if ((A || b) && cap < h->sys_pos) return fail(LVI_ERR_CAPACITY, "the arrays are shorter than m + n");
    if (pos_out) *pos_out = h->sys_pos;
    if (!A && !b) return LVI_OK;
    return guarded(h->device, [&]() -> int32_t {
        const size_t pos = (size_t)h->sys_pos, P1 = pos + 1;
        LVI_HIP(hipMemcpyAsync(h->h_out, h->d.A, sizeof(double) * P1 * P1, hipMemcpyDeviceToHost, h->stream));
        LVI_HIP(hipStreamSynchronize(h->stream));
        for (size_t i = 0; i < pos; i++) {
            if (A) std::memcpy(A + i * pos, h->h_out + i * P1, sizeof(double) * pos);
            if (b) b[i] = h->h_out[i * P1 + pos];
        }
        return LVI_OK;
    });
}

}  // extern "C"
