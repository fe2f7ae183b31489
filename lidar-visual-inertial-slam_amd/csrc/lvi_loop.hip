// C-ABI and kernels of the loop-closure registration (include/lvi_loop.h): performLoopClosure's two submaps
// (mapOptimization.cpp:549-628, loopFindNearKeyframes :719-741) and the ICP between them, over the device keyframe
// store, on a stream of its own.
//
// Submaps: the global map's fuse (kf_assemble_kernel, one launch for both clouds: piece.which picks the output) and
// two Submaps in this arena — the same kernels as lvi_gmap_build, hence the same bits.  The stream, the arena, the
// piece table and the fetch are the keyframe job of lvi_kfjob.hpp.
//
// ICP (restated in tests/loop_ref.py):
//   index      a uniform grid over the filtered target: bbox (integer atomics on order-encoded floats), count, one
//              single-workgroup scan, scatter of (xyz, original index).  The order inside a cell is whatever the
//              scatter's atomics gave; a query compares (distance, index), so its answer does not depend on it.
//   iteration  loop_nn_kernel: one thread per source point, shells of cells of growing Chebyshev radius round the
//              query's cell; a row of cells along x is one contiguous range of the sorted points.  Everything in shell r
//              is at least (r - 1) cells away, so the walk stops once the best distance is no larger than that bound
//              (exact nearest neighbour, lowest index on equal f32 distance), or the bound passes max_corr_dist.  The
//              kept pairs' count, sum p, sum q, sum p q^T, sum d2 are accumulated in double: a fixed butterfly per
//              wavefront, waves in order, one partial record per workgroup.  No floating-point atomics.
//              loop_solve_kernel (one workgroup): the partials in workgroup order, Umeyama without scale through a
//              one-sided Jacobi SVD in double, final = step * final in f32, DefaultConvergenceCriteria.
//   one wait   max_iters (nn, solve) pairs are enqueued; a device-side done flag turns the rest into early exits.  Then
//              the fitness pass (unbounded queries on the aligned source) and the finish step.
#include <cfloat>
#include <cmath>

#include "../../include/lvi_loop.h"
#include "lvi_lidar.hpp"

namespace lvi {

constexpr int LOOP_MAX_CELLS = 1 << 21;                    // cells of the nearest-neighbour grid
constexpr int LOOP_MAX_DIM = 2048;                         // cells per axis
constexpr int LOOP_MAX_SEARCH = 1024;                      // largest search_num (segment table: 2 + 2 (2 n + 1) pieces)
constexpr int LOOP_NN_BLOCK = 256;
constexpr int NS = LVI_LOOP_N_SUMS;
enum { NN_ITER = 0, NN_FIT = 1, NN_DEBUG = 2 };

struct LoopJob {                                           // kernel argument of the setup step
    const lvi_pt *srcFused, *srcOut, *tgtFused, *tgtOut;
    const VoxGrid *gS, *gT;
    const int *noutS, *noutT;
    int nS_fused, nT_fused, filtS, filtT;
    int min_s, min_t;
    float cell0;                                           // first cell edge tried
};

struct LoopState {                                         // device; copied whole into pinned host memory by the finish step
    const lvi_pt* src; const lvi_pt* tgt;
    int n_src, n_tgt, ovS, ovT;
    int status, done, iters, converged, conv_state, n_corr;
    float final_T[16];
    float cur[16];                                         // what the next pass applies: the last step (incremental) or final_T
    double prev_mse, mse, fitness;
    unsigned bb[6];                                        // order-encoded target bbox
    float org[3], cs, inv;
    int dim[3], ncells;
    float dbgT[16];
    double dbgSums[NS];
};

struct LoopDev : KfJob {
    int req_s = 0, req_t = 0, nblk_s = 0;                  // the reservations asked for (the submaps' capacities are at least 64)
    Submap src, tgt;
    lvi_pt* aligned = nullptr;                             // [src.cap]
    int *cellStart = nullptr, *cellCount = nullptr;        // [LOOP_MAX_CELLS + 2]
    float4* sorted = nullptr;                              // [tgt.cap] xyz + original index (int bits)
    int* nnIdx = nullptr; float* nnSqd = nullptr;          // [src.cap]
    double* partial = nullptr;                             // [nblk_s][NS]
    LoopState* st = nullptr; LoopState* h_st = nullptr;    // device / pinned
    // last job (host)
    bool started = false;
    int nS_fused = 0, nT_fused = 0, key_cur = -1, key_pre = -1;
    lvi_loop_params P{};
};

// ---------------------------------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------------------------------
namespace {

__device__ __forceinline__ void ident16(float* T)
{
    for (int i = 0; i < 16; i++) T[i] = (i % 5 == 0) ? 1.f : 0.f;
}

__global__ void loop_setup_kernel(LoopJob j, LoopState* st)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int ovS = j.filtS ? j.gS->overflow : 0, ovT = j.filtT ? j.gT->overflow : 0;
    st->ovS = ovS; st->ovT = ovT;
    st->src = (j.filtS && !ovS) ? j.srcOut : j.srcFused;
    st->tgt = (j.filtT && !ovT) ? j.tgtOut : j.tgtFused;
    st->n_src = (j.filtS && !ovS) ? j.noutS[0] : j.nS_fused;
    st->n_tgt = (j.filtT && !ovT) ? j.noutT[0] : j.nT_fused;
    const bool few = st->n_src < j.min_s || st->n_tgt < j.min_t || st->n_src < 1 || st->n_tgt < 1;
    st->status = few ? LVI_LOOP_TOO_FEW_POINTS : LVI_LOOP_OK;
    st->done = few ? 1 : 0;
    st->iters = 0; st->converged = 0; st->conv_state = LVI_LOOP_CONV_NOT_CONVERGED; st->n_corr = 0;
    ident16(st->final_T); ident16(st->cur);
    st->prev_mse = DBL_MAX; st->mse = 0.0; st->fitness = DBL_MAX;
    for (int a = 0; a < 3; a++) { st->bb[a] = 0xffffffffu; st->bb[3 + a] = 0u; }
    st->cs = j.cell0;
}

__global__ __launch_bounds__(256) void loop_bbox_kernel(LoopState* st)
{
    const int n = st->n_tgt;
    const lvi_pt* __restrict__ t = st->tgt;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const lvi_pt p = ld_global_pt(t + i);
        mn[0] = fminf(mn[0], p.x); mn[1] = fminf(mn[1], p.y); mn[2] = fminf(mn[2], p.z);
        mx[0] = fmaxf(mx[0], p.x); mx[1] = fmaxf(mx[1], p.y); mx[2] = fmaxf(mx[2], p.z);
    }
    for (int a = 0; a < 3; a++) { mn[a] = wave_min(mn[a]); mx[a] = wave_max(mx[a]); }
    if (lane_id() == 0) {
        for (int a = 0; a < 3; a++) {
            if (mn[a] <= mx[a]) { atomicMin(&st->bb[a], f2ord(mn[a])); atomicMax(&st->bb[3 + a], f2ord(mx[a])); }
        }
    }
}

// cell edge: the first of cell0, 2 cell0, 4 cell0 … whose grid has at most LOOP_MAX_DIM cells per axis and LOOP_MAX_CELLS in
// all.  One spare cell per axis beyond the largest coordinate: no finite target point is ever clamped into a cell.
__global__ void loop_grid_kernel(LoopState* st)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float lo[3], hi[3];
    bool ok = st->n_tgt > 0;
    for (int a = 0; a < 3; a++) {
        lo[a] = ord2f(st->bb[a]); hi[a] = ord2f(st->bb[3 + a]);
        if (!(lo[a] <= hi[a]) || isinf(lo[a]) || isinf(hi[a])) ok = false;
    }
    if (!ok) { for (int a = 0; a < 3; a++) { lo[a] = 0.f; hi[a] = 0.f; } }
    double cs = st->cs > 0.f ? (double)st->cs : 1.0;
    int dim[3];
    for (;;) {
        double prod = 1.0; bool fits = true;
        for (int a = 0; a < 3; a++) {
            const double c = floor(((double)hi[a] - (double)lo[a]) / cs) + 2.0;
            if (c > (double)LOOP_MAX_DIM) fits = false;
            dim[a] = fits ? (int)c : 1;
            prod *= c;
        }
        if (fits && prod <= (double)LOOP_MAX_CELLS) break;
        cs *= 2.0;
    }
    st->cs = (float)cs; st->inv = 1.f / (float)cs;
    for (int a = 0; a < 3; a++) { st->org[a] = lo[a]; st->dim[a] = dim[a]; }
    st->ncells = dim[0] * dim[1] * dim[2];
}

// the cell coordinate of a value along one axis: monotone in v, the same expression for target points and queries
__device__ __forceinline__ int cell_of(float v, float org, float inv)
{
    const float f = floorf((v - org) * inv);
    return (int)fminf(fmaxf(f, -1.0e6f), 1.0e6f);          // (NaN -> -1e6)
}
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int tgt_cell(const LoopState* st, const lvi_pt& p)
{
    const int cx = clampi(cell_of(p.x, st->org[0], st->inv), 0, st->dim[0] - 1);
    const int cy = clampi(cell_of(p.y, st->org[1], st->inv), 0, st->dim[1] - 1);
    const int cz = clampi(cell_of(p.z, st->org[2], st->inv), 0, st->dim[2] - 1);
    return (cz * st->dim[1] + cy) * st->dim[0] + cx;
}

__global__ __launch_bounds__(256) void loop_count_kernel(const LoopState* st, int* __restrict__ count)
{
    const int n = st->n_tgt;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) atomicAdd(&count[tgt_cell(st, ld_global_pt(st->tgt + i))], 1);
}

// exclusive scan of the cell counts, one workgroup: thread t owns a contiguous run of cells.  count becomes the scatter's cursor.
__global__ __launch_bounds__(1024) void loop_scan_kernel(const LoopState* st, int* __restrict__ count, int* __restrict__ start)
{
    __shared__ int ws[1024 / 64 + 1];
    const int nc = st->ncells;
    const int per = (nc + 1023) / 1024;
    const int a = min((int)threadIdx.x * per, nc), b = min(a + per, nc);
    int s = 0;
    for (int c = a; c < b; c++) s += count[c];
    int total;
    int run = block_excl_scan<1024>(s, ws, &total);
    for (int c = a; c < b; c++) { const int v = count[c]; start[c] = run; count[c] = run; run += v; }
    if (threadIdx.x == 0) start[nc] = total;
}

__global__ __launch_bounds__(256) void loop_scatter_kernel(const LoopState* st, int* __restrict__ cursor, float4* __restrict__ sorted)
{
    const int n = st->n_tgt;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const lvi_pt p = ld_global_pt(st->tgt + i);
        const int pos = atomicAdd(&cursor[tgt_cell(st, p)], 1);
        sorted[pos] = make_float4(p.x, p.y, p.z, __int_as_float(i));
    }
}

__device__ __forceinline__ void nn_scan(const float4* __restrict__ sorted, int a, int b, float px, float py, float pz, int& bi, float& bd)
{
    for (int j = a; j < b; j++) {
        const float4 q = sorted[j];
        const float dx = px - q.x, dy = py - q.y, dz = pz - q.z;
        const float d = (dx * dx + dy * dy) + dz * dz;
        const int idx = __float_as_int(q.w);
        if (d < bd || (d == bd && idx < bi)) { bd = d; bi = idx; }
    }
}

// exact nearest neighbour of (px, py, pz) among the indexed target points; max2 < 0: unbounded
__device__ void nn_query(const LoopState* st, const int* __restrict__ start, const float4* __restrict__ sorted, float px, float py, float pz,
                         double max2, int& bi, float& bd)
{
    const int dx = st->dim[0], dy = st->dim[1], dz = st->dim[2];
    const int cx = cell_of(px, st->org[0], st->inv), cy = cell_of(py, st->org[1], st->inv), cz = cell_of(pz, st->org[2], st->inv);
    bi = 0x7fffffff; bd = INFINITY;
    // first shell that meets the grid, and the shell that covers all of it
    const int r0 = max(0, max(max(max(-cx, cx - (dx - 1)), max(-cy, cy - (dy - 1))), max(-cz, cz - (dz - 1))));
    const int rmax = max(max(max(abs(cx), abs(cx - (dx - 1))), max(abs(cy), abs(cy - (dy - 1)))), max(abs(cz), abs(cz - (dz - 1))));
    const double cs = (double)st->cs, slop = 0.01 * cs;   // cells are cs wide up to the rounding of cell_of: far less than 1 % of a cell
    for (int r = r0; r <= rmax; r++) {
        if (r >= 2) {
            const double lb = (double)(r - 1) * cs - slop, lb2 = lb * lb;   // every point of shells >= r is at least this far
            if ((double)bd <= lb2) break;
            if (max2 >= 0.0 && lb2 > max2) break;
        }
        const int z0 = max(cz - r, 0), z1 = min(cz + r, dz - 1), y0 = max(cy - r, 0), y1 = min(cy + r, dy - 1);
        const int x0 = max(cx - r, 0), x1 = min(cx + r, dx - 1);
        const int xl = cx - r, xh = cx + r;
        for (int z = z0; z <= z1; z++) {
            const bool zf = (z - cz == r) || (cz - z == r);
            for (int y = y0; y <= y1; y++) {
                const int row = (z * dy + y) * dx;
                if (zf || (y - cy == r) || (cy - y == r)) {
                    if (x0 <= x1) nn_scan(sorted, start[row + x0], start[row + x1 + 1], px, py, pz, bi, bd);
                } else {
                    if (xl >= 0 && xl < dx) nn_scan(sorted, start[row + xl], start[row + xl + 1], px, py, pz, bi, bd);
                    if (r > 0 && xh >= 0 && xh < dx) nn_scan(sorted, start[row + xh], start[row + xh + 1], px, py, pz, bi, bd);
                }
            }
        }
    }
    if (bi == 0x7fffffff || (max2 >= 0.0 && !((double)bd <= max2))) { bi = -1; bd = INFINITY; }
}

__device__ __forceinline__ lvi_pt apply16(const float* T, const lvi_pt& p)
{
    lvi_pt o;
    o.x = ((T[0] * p.x + T[1] * p.y) + T[2] * p.z) + T[3];
    o.y = ((T[4] * p.x + T[5] * p.y) + T[6] * p.z) + T[7];
    o.z = ((T[8] * p.x + T[9] * p.y) + T[10] * p.z) + T[11];
    o.intensity = p.intensity;
    return o;
}

// one correspondence pass.  Workgroup b owns source points [256 b, 256 b + 256): its partial record does not depend on the grid.
__global__ __launch_bounds__(LOOP_NN_BLOCK) void loop_nn_kernel(LoopState* st, int mode, int incremental, double max2_iter, const int* __restrict__ start,
                                                                const float4* __restrict__ sorted, lvi_pt* __restrict__ aligned,
                                                                int* __restrict__ nnIdx, float* __restrict__ nnSqd, double* __restrict__ partial)
{
    __shared__ double red[LOOP_NN_BLOCK / 64][NS];
    __shared__ float T[16];
    const int n = st->n_src;
    if (mode == NN_ITER && st->done) return;
    if ((int)blockIdx.x * LOOP_NN_BLOCK >= n) return;
    const bool few = st->status == LVI_LOOP_TOO_FEW_POINTS;
    if (mode == NN_DEBUG && few) return;
    if (threadIdx.x < 16) T[threadIdx.x] = mode == NN_DEBUG ? st->dbgT[threadIdx.x] : st->cur[threadIdx.x];
    __syncthreads();
    const bool from_aligned = mode != NN_DEBUG && incremental && st->iters > 0;
    const int i = blockIdx.x * LOOP_NN_BLOCK + threadIdx.x;
    double s[NS];
    for (int k = 0; k < NS; k++) s[k] = 0.0;
    if (i < n) {
        const lvi_pt p = apply16(T, ld_global_pt((from_aligned ? aligned : st->src) + i));
        if (mode != NN_DEBUG) aligned[i] = p;
        if (!few) {
            int bi; float bd;
            nn_query(st, start, sorted, p.x, p.y, p.z, mode == NN_FIT ? -1.0 : max2_iter, bi, bd);
            nnIdx[i] = bi; nnSqd[i] = bd;
            if (bi >= 0) {
                const lvi_pt q = ld_global_pt(st->tgt + bi);
                const double P[3] = {p.x, p.y, p.z}, Q[3] = {q.x, q.y, q.z};
                s[0] = 1.0;
                for (int a = 0; a < 3; a++) { s[1 + a] = P[a]; s[4 + a] = Q[a]; for (int b = 0; b < 3; b++) s[7 + 3 * a + b] = P[a] * Q[b]; }
                s[16] = (double)bd;
            }
        }
    }
    for (int k = 0; k < NS; k++) s[k] = wave_sum(s[k]);
    if (lane_id() == 0) for (int k = 0; k < NS; k++) red[wave_id()][k] = s[k];
    __syncthreads();
    if (threadIdx.x < NS) {
        double t = red[0][threadIdx.x];
        for (int w = 1; w < LOOP_NN_BLOCK / 64; w++) t += red[w][threadIdx.x];
        partial[(size_t)blockIdx.x * NS + threadIdx.x] = t;
    }
}

// the ordered pass over the workgroup partials: thread k < NS sums column k in workgroup order
__device__ __forceinline__ void loop_total(const LoopState* st, const double* __restrict__ partial, double* S)
{
    if (threadIdx.x < NS) {
        const int nb = (st->n_src + LOOP_NN_BLOCK - 1) / LOOP_NN_BLOCK;
        double t = 0.0;
        for (int b = 0; b < nb; b++) t += partial[(size_t)b * NS + threadIdx.x];
        S[threadIdx.x] = t;
    }
    __syncthreads();
}

__device__ __forceinline__ double det3(const double* M)
{
    return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

// A = U diag(S) V^T, one-sided Jacobi on the columns (row-major 3x3), singular values descending; a column of U whose singular
// value vanishes is completed to an orthonormal basis
__device__ void svd3(const double* A, double* U, double* S, double* V)
{
    double W[9];
    for (int i = 0; i < 9; i++) { W[i] = A[i]; V[i] = (i % 4 == 0) ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 60; sweep++) {
        bool rotated = false;
        for (int p = 0; p < 2; p++) {
            for (int q = p + 1; q < 3; q++) {
                double al = 0.0, be = 0.0, ga = 0.0;
                for (int r = 0; r < 3; r++) { al += W[3 * r + p] * W[3 * r + p]; be += W[3 * r + q] * W[3 * r + q]; ga += W[3 * r + p] * W[3 * r + q]; }
                if (ga == 0.0 || fabs(ga) <= 1e-17 * sqrt(al * be)) continue;
                rotated = true;
                const double zeta = (be - al) / (2.0 * ga);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), sn = c * t;
                for (int r = 0; r < 3; r++) {
                    const double wp = W[3 * r + p], wq = W[3 * r + q];
                    W[3 * r + p] = c * wp - sn * wq; W[3 * r + q] = sn * wp + c * wq;
                    const double vp = V[3 * r + p], vq = V[3 * r + q];
                    V[3 * r + p] = c * vp - sn * vq; V[3 * r + q] = sn * vp + c * vq;
                }
            }
        }
        if (!rotated) break;
    }
    for (int j = 0; j < 3; j++) S[j] = sqrt(W[j] * W[j] + W[3 + j] * W[3 + j] + W[6 + j] * W[6 + j]);
    for (int a = 0; a < 2; a++) {
        for (int b = a + 1; b < 3; b++) {
            if (S[b] > S[a]) {
                const double t = S[a]; S[a] = S[b]; S[b] = t;
                for (int r = 0; r < 3; r++) {
                    const double w = W[3 * r + a]; W[3 * r + a] = W[3 * r + b]; W[3 * r + b] = w;
                    const double v = V[3 * r + a]; V[3 * r + a] = V[3 * r + b]; V[3 * r + b] = v;
                }
            }
        }
    }
    const double tiny = 1e-13 * S[0];
    for (int i = 0; i < 9; i++) U[i] = 0.0;
    if (!(S[0] > 0.0)) { U[0] = U[4] = U[8] = 1.0; return; }
    for (int r = 0; r < 3; r++) U[3 * r] = W[3 * r] / S[0];
    if (S[1] > tiny) {
        for (int r = 0; r < 3; r++) U[3 * r + 1] = W[3 * r + 1] / S[1];
    } else {                                               // any unit vector orthogonal to u0
        const int k = fabs(U[0]) <= fabs(U[3]) ? (fabs(U[0]) <= fabs(U[6]) ? 0 : 2) : (fabs(U[3]) <= fabs(U[6]) ? 1 : 2);
        double e[3] = {0.0, 0.0, 0.0}; e[k] = 1.0;
        const double dp = U[3 * k];
        double v[3], nv = 0.0;
        for (int r = 0; r < 3; r++) { v[r] = e[r] - dp * U[3 * r]; nv += v[r] * v[r]; }
        nv = sqrt(nv);
        for (int r = 0; r < 3; r++) U[3 * r + 1] = v[r] / nv;
    }
    if (S[2] > tiny) {
        for (int r = 0; r < 3; r++) U[3 * r + 2] = W[3 * r + 2] / S[2];
    } else {
        U[2] = U[3] * U[7] - U[6] * U[4];
        U[5] = U[6] * U[1] - U[0] * U[7];
        U[8] = U[0] * U[4] - U[3] * U[1];
    }
}

__global__ __launch_bounds__(64) void loop_solve_kernel(LoopState* st, int incremental, int max_iters, double teps, double feps, const double* __restrict__ partial)
{
    __shared__ double S[NS];
    if (st->done) return;
    loop_total(st, partial, S);
    if (threadIdx.x != 0) return;
    const double cnt = S[0];
    st->n_corr = (int)cnt;
    if (cnt < 3.0) {
        st->status = LVI_LOOP_NO_CORRESPONDENCES; st->conv_state = LVI_LOOP_CONV_NO_CORRESPONDENCES; st->converged = 0; st->done = 1;
        if (incremental) ident16(st->cur);
        return;
    }
    // Umeyama without scale: sigma = 1/n sum (q - mu_q)(p - mu_p)^T = U S V^T, R = U diag(1, 1, sign(det U det V)) V^T
    double mp[3], mq[3], sg[9];
    for (int a = 0; a < 3; a++) { mp[a] = S[1 + a] / cnt; mq[a] = S[4 + a] / cnt; }
    for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) sg[3 * a + b] = S[7 + 3 * b + a] / cnt - mq[a] * mp[b];
    double U[9], sv[3], V[9], R[9];
    svd3(sg, U, sv, V);
    const double sgn = det3(U) * det3(V) < 0.0 ? -1.0 : 1.0;
    for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) R[3 * a + b] = U[3 * a] * V[3 * b] + U[3 * a + 1] * V[3 * b + 1] + sgn * U[3 * a + 2] * V[3 * b + 2];
    float step[16];
    ident16(step);
    for (int a = 0; a < 3; a++) {
        for (int b = 0; b < 3; b++) step[4 * a + b] = (float)R[3 * a + b];
        step[4 * a + 3] = (float)(mq[a] - (R[3 * a] * mp[0] + R[3 * a + 1] * mp[1] + R[3 * a + 2] * mp[2]));
    }
    float fin[16];
    for (int a = 0; a < 4; a++) for (int b = 0; b < 4; b++)
        fin[4 * a + b] = ((step[4 * a] * st->final_T[b] + step[4 * a + 1] * st->final_T[4 + b]) + step[4 * a + 2] * st->final_T[8 + b]) + step[4 * a + 3] * st->final_T[12 + b];
    for (int i = 0; i < 16; i++) { st->final_T[i] = fin[i]; st->cur[i] = incremental ? step[i] : fin[i]; }
    const int it = ++st->iters;
    // DefaultConvergenceCriteria::hasConverged, no similar iterations allowed
    const double cosa = 0.5 * (double)(((step[0] + step[5]) + step[10]) - 1.f);
    const double tsq = (double)((step[3] * step[3] + step[7] * step[7]) + step[11] * step[11]);
    const double mse = S[16] / cnt;
    st->mse = mse;
    int state = LVI_LOOP_CONV_NOT_CONVERGED;
    if (it >= max_iters) state = LVI_LOOP_CONV_ITERATIONS;
    else if (cosa >= 1.0 - teps && tsq <= teps) state = LVI_LOOP_CONV_TRANSFORM;
    else if (mse < 1e-12) state = LVI_LOOP_CONV_ABS_MSE;
    else if (fabs(mse - st->prev_mse) / st->prev_mse < feps) state = LVI_LOOP_CONV_REL_MSE;
    else st->prev_mse = mse;
    if (state != LVI_LOOP_CONV_NOT_CONVERGED) { st->conv_state = state; st->converged = 1; st->done = 1; }
}

__global__ __launch_bounds__(64) void loop_finish_kernel(LoopState* st, const double* __restrict__ partial)
{
    __shared__ double S[NS];
    if (st->status == LVI_LOOP_TOO_FEW_POINTS) return;
    loop_total(st, partial, S);
    if (threadIdx.x == 0) st->fitness = S[0] > 0.0 ? S[16] / S[0] : DBL_MAX;
}

__global__ __launch_bounds__(64) void loop_dbgsum_kernel(LoopState* st, const double* __restrict__ partial)
{
    __shared__ double S[NS];
    loop_total(st, partial, S);
    if (threadIdx.x < NS) st->dbgSums[threadIdx.x] = S[threadIdx.x];
}

// ---------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------
void lp_destroy(LoopDev* g)
{
    if (!g) return;
    g->destroy();
    g->src.release(); g->tgt.release();
    if (g->h_st) (void)hipHostFree(g->h_st);
    delete g;
}

template <class AR>
void lp_layout(AR& ar, LoopDev& g, int cap_s, int cap_t)
{
    g.src.layout(ar, cap_s);
    g.tgt.layout(ar, cap_t);
    g.aligned = ar.template alloc<lvi_pt>(cap_s);
    g.d_seg = ar.template alloc<KfSeg>((size_t)g.seg_cap);
    g.cellStart = ar.template alloc<int>((size_t)LOOP_MAX_CELLS + 2);
    g.cellCount = ar.template alloc<int>((size_t)LOOP_MAX_CELLS + 2);
    g.sorted = ar.template alloc<float4>(cap_t);
    g.nnIdx = ar.template alloc<int>(cap_s);
    g.nnSqd = ar.template alloc<float>(cap_s);
    g.partial = ar.template alloc<double>((size_t)g.nblk_s * NS);
    g.st = ar.template alloc<LoopState>(1);
}

void lp_launch_nn(LoopDev& g, int mode, double max2)
{
    hipLaunchKernelGGL(loop_nn_kernel, dim3(g.nblk_s), dim3(LOOP_NN_BLOCK), 0, g.ctx.stream, g.st, mode, g.P.incremental_cloud, max2, g.cellStart, g.sorted,
                       g.aligned, g.nnIdx, g.nnSqd, g.partial);
    LVI_HIP(hipGetLastError());
}

}  // namespace

void loop_join(LidarDev& d)
{
    if (d.loop) d.loop->wait();
}

void loop_free(LidarDev& d)
{
    LoopDev* g = d.loop;
    d.loop = nullptr;
    lp_destroy(g);
}

}  // namespace lvi

using namespace lvi;

extern "C" {

int32_t lvi_loop_abi_version(void) { return LVI_LOOP_ABI_VERSION; }

void lvi_loop_params_default(lvi_loop_params* p)
{
    if (!p) return;
    p->search_num = 25;
    p->leaf = 0.4f;
    p->max_corr_dist = 30.f;                               // 2 * historyKeyframeSearchRadius (15)
    p->max_iters = 100;
    p->transformation_epsilon = 1e-6;
    p->fitness_epsilon = 1e-6;
    p->min_source = 300;
    p->min_target = 1000;
    p->incremental_cloud = 1;
}

int32_t lvi_loop_reserve(lvi_lidar* h, int32_t max_source_points, int32_t max_target_points)
{
    if (!h) return fail(LVI_ERR_INVALID_ARG, "null handle");
    if (max_source_points < 1 || max_source_points > LVI_LOOP_MAX_POINTS || max_target_points < 1 || max_target_points > LVI_LOOP_MAX_POINTS)
        return fail(LVI_ERR_INVALID_ARG, "reservations must be 1..LVI_LOOP_MAX_POINTS");
    LidarDev& d = lidar_slot0(h);
    if (d.loop && d.loop->req_s >= max_source_points && d.loop->req_t >= max_target_points) return LVI_OK;
    return guarded(d.device, [&]() -> int32_t {
        loop_join(d);
        LoopDev* g = new LoopDev();
        try {
            g->req_s = std::max(max_source_points, d.loop ? d.loop->req_s : 0);
            g->req_t = std::max(max_target_points, d.loop ? d.loop->req_t : 0);
            const int cap_s = std::max(g->req_s, 64), cap_t = std::max(g->req_t, 64);
            g->nblk_s = div_up(cap_s, LOOP_NN_BLOCK);
            g->create(2 + 2 * (2 * LOOP_MAX_SEARCH + 1));
            LVI_HIP(hipHostMalloc((void**)&g->h_st, sizeof(LoopState), hipHostMallocDefault));
            g->init_arena([&](auto& ar) { lp_layout(ar, *g, cap_s, cap_t); });
            g->src.vox.mode = d.P.voxel_mode; g->tgt.vox.mode = d.P.voxel_mode;
            LVI_HIP(hipStreamSynchronize(g->ctx.stream));
        } catch (...) {
            lp_destroy(g);
            throw;
        }
        loop_free(d);                                                  // the old arena (its job has finished)
        d.loop = g;
        return LVI_OK;
    });
}

int32_t lvi_loop_release(lvi_lidar* h)
{
    if (!h) return fail(LVI_ERR_INVALID_ARG, "null handle");
    LidarDev& d = lidar_slot0(h);
    return guarded(d.device, [&]() -> int32_t { loop_free(d); return LVI_OK; });
}

int32_t lvi_loop_arena_bytes(lvi_lidar* h, int64_t* bytes)
{
    if (!h || !bytes) return fail(LVI_ERR_INVALID_ARG, "null argument");
    const LoopDev* g = lidar_slot0(h).loop;
    *bytes = g ? (int64_t)g->arena.size : 0;
    return LVI_OK;
}

int32_t lvi_loop_start(lvi_lidar* h, int32_t key_cur, int32_t key_pre, const lvi_loop_params* params)
{
    if (!h || !params) return fail(LVI_ERR_INVALID_ARG, "null argument");
    const lvi_loop_params P = *params;
    if (P.search_num < 0 || P.search_num > LOOP_MAX_SEARCH) return fail(LVI_ERR_INVALID_ARG, "search_num must be 0..1024");
    if (!(P.leaf >= 0.f) || std::isinf(P.leaf)) return fail(LVI_ERR_INVALID_ARG, "leaf must be 0 (no filter) or a finite positive size");
    if (!(P.max_corr_dist > 0.f) || std::isinf(P.max_corr_dist)) return fail(LVI_ERR_INVALID_ARG, "max_corr_dist must be finite and positive");
    if (P.max_iters < 1 || P.max_iters > LVI_LOOP_MAX_ITERS) return fail(LVI_ERR_INVALID_ARG, "max_iters must be 1..LVI_LOOP_MAX_ITERS");
    if (!(P.transformation_epsilon >= 0.0) || !(P.fitness_epsilon >= 0.0) || P.min_source < 0 || P.min_target < 0)
        return fail(LVI_ERR_INVALID_ARG, "epsilons and point gates must be non-negative");
    LidarDev& d = lidar_slot0(h);
    if (!d.loop) return fail(LVI_ERR_STATE, "no loop-closure reservation (lvi_loop_reserve)");
    LoopDev& g = *d.loop;
    const int nkf = (int)d.kf_pose.size();
    if (key_cur < 0 || key_cur >= nkf || key_pre < 0 || key_pre >= nkf) return fail(LVI_ERR_INVALID_ARG, "key index out of range");
    const int k0 = std::max(key_pre - P.search_num, 0), k1 = std::min(key_pre + P.search_num, nkf - 1);
    const long long totS = (long long)d.kf_n_c[key_cur] + d.kf_n_s[key_cur];
    long long totT = 0;
    for (int k = k0; k <= k1; k++) totT += (long long)d.kf_n_c[k] + d.kf_n_s[k];
    if (totS > g.req_s) return fail(LVI_ERR_CAPACITY, "fused source submap exceeds the loop-closure reservation");
    if (totT > g.req_t) return fail(LVI_ERR_CAPACITY, "fused target submap exceeds the loop-closure reservation");
    return guarded(d.device, [&]() -> int32_t {
        g.wait();                                                      // the previous job still reads h_seg / writes the arena
        const int nS = (int)totS, nT = (int)totT;
        const bool filtS = P.leaf > 0.f && nS > 0, filtT = P.leaf > 0.f && nT > 0;
        if (filtS || filtT) {                                          // (synchronises the job's stream: before the fork below is enqueued)
            g.src.prepare(g.ctx, P.leaf);
            g.tgt.prepare(g.ctx, P.leaf);
        }
        // pieces: the source (output 0 -> src.fused), then the target (output 1 -> tgt.fused); corner_k then surf_k per key
        KfPieces t{g.h_seg};
        kf_pieces_add(d, t, key_cur, 0, 0);
        for (int k = k0; k <= k1; k++) kf_pieces_add(d, t, k, 1, 1);
        g.fork(d.ctx);
        hipStream_t s = g.ctx.stream;
        LVI_HIP(hipMemcpyAsync(g.d_seg, g.h_seg, sizeof(KfSeg) * (size_t)t.n, hipMemcpyHostToDevice, s));
        kf_assemble_launch(g.ctx, g.d_seg, t.n, t.maxn, d.kfPool, g.src.fused, g.tgt.fused, (double)(nS + nT));
        if (filtS) g.src.filter(g.ctx, nS, "loop_src");
        if (filtT) g.tgt.filter(g.ctx, nT, "loop_tgt");
        g.P = P;
        LoopJob j{};
        j.srcFused = g.src.fused; j.srcOut = g.src.out; j.tgtFused = g.tgt.fused; j.tgtOut = g.tgt.out;
        j.gS = g.src.vox.d_grid; j.gT = g.tgt.vox.d_grid; j.noutS = g.src.vox.d_nout; j.noutT = g.tgt.vox.d_nout;
        j.nS_fused = nS; j.nT_fused = nT; j.filtS = filtS; j.filtT = filtT;
        j.min_s = P.min_source; j.min_t = P.min_target;
        j.cell0 = P.leaf > 0.f ? std::max(4.f * P.leaf, 0.5f) : 1.f;
        const int nbT = std::max(1, std::min(div_up(nT, 256), 1024));
        hipLaunchKernelGGL(loop_setup_kernel, dim3(1), dim3(1), 0, s, j, g.st);
        hipLaunchKernelGGL(loop_bbox_kernel, dim3(nbT), dim3(256), 0, s, g.st);
        hipLaunchKernelGGL(loop_grid_kernel, dim3(1), dim3(1), 0, s, g.st);
        LVI_HIP(hipMemsetAsync(g.cellCount, 0, sizeof(int) * ((size_t)LOOP_MAX_CELLS + 2), s));
        hipLaunchKernelGGL(loop_count_kernel, dim3(nbT), dim3(256), 0, s, g.st, g.cellCount);
        hipLaunchKernelGGL(loop_scan_kernel, dim3(1), dim3(1024), 0, s, g.st, g.cellCount, g.cellStart);
        hipLaunchKernelGGL(loop_scatter_kernel, dim3(nbT), dim3(256), 0, s, g.st, g.cellCount, g.sorted);
        LVI_HIP(hipGetLastError());
        const double max2 = (double)P.max_corr_dist * (double)P.max_corr_dist;
        for (int it = 0; it < P.max_iters; it++) {
            lp_launch_nn(g, NN_ITER, max2);
            hipLaunchKernelGGL(loop_solve_kernel, dim3(1), dim3(64), 0, s, g.st, P.incremental_cloud, P.max_iters, P.transformation_epsilon, P.fitness_epsilon, g.partial);
        }
        lp_launch_nn(g, NN_FIT, -1.0);
        hipLaunchKernelGGL(loop_finish_kernel, dim3(1), dim3(64), 0, s, g.st, g.partial);
        LVI_HIP(hipGetLastError());
        LVI_HIP(hipMemcpyAsync(g.h_st, g.st, sizeof(LoopState), hipMemcpyDeviceToHost, s));
        g.mark_done();
        g.started = true;
        g.nS_fused = nS; g.nT_fused = nT; g.key_cur = key_cur; g.key_pre = key_pre;
        return LVI_OK;
    });
}

}  // extern "C"

namespace {

int32_t lp_result(LidarDev& d, lvi_loop_info* info)
{
    if (!d.loop || !d.loop->started) return fail(LVI_ERR_STATE, "no loop-closure job started");
    LoopDev& g = *d.loop;
    LVI_HIP(hipEventSynchronize(g.evDone));                            // this job only: not the handle's other streams
    const LoopState& s = *g.h_st;
    lvi_loop_info r{};
    r.status = s.status;
    r.n_source = s.n_src; r.n_target = s.n_tgt;
    r.n_source_fused = g.nS_fused; r.n_target_fused = g.nT_fused;
    r.overflow_source = s.ovS; r.overflow_target = s.ovT;
    r.iterations = s.iters; r.converged = s.converged; r.convergence_state = s.conv_state; r.n_corr = s.n_corr;
    r.key_cur = g.key_cur; r.key_pre = g.key_pre;
    for (int i = 0; i < 16; i++) r.transformation[i] = s.final_T[i];
    r.fitness = s.fitness; r.mse = s.mse;
    *info = r;
    return LVI_OK;
}

}  // namespace

extern "C" {

int32_t lvi_loop_result(lvi_lidar* h, lvi_loop_info* info)
{
    if (!h || !info) return fail(LVI_ERR_INVALID_ARG, "null argument");
    LidarDev& d = lidar_slot0(h);
    return guarded(d.device, [&]() -> int32_t { return lp_result(d, info); });
}

int32_t lvi_loop_fetch(lvi_lidar* h, int32_t what, int32_t first, int32_t count, lvi_pt* out)
{
    if (!h || (count > 0 && !out) || first < 0 || count < 0) return fail(LVI_ERR_INVALID_ARG, "bad fetch arguments");
    if (what < LVI_LOOP_SOURCE || what > LVI_LOOP_ALIGNED) return fail(LVI_ERR_INVALID_ARG, "what must be LVI_LOOP_SOURCE, _TARGET or _ALIGNED");
    LidarDev& d = lidar_slot0(h);
    return guarded(d.device, [&]() -> int32_t {
        lvi_loop_info r;
        const int32_t st = lp_result(d, &r);
        if (st) return st;
        LoopDev& g = *d.loop;
        const int n = what == LVI_LOOP_TARGET ? r.n_target : r.n_source;
        if ((long long)first + count > n) return fail(LVI_ERR_INVALID_ARG, "fetch range outside the cloud");
        g.fetch((what == LVI_LOOP_ALIGNED ? g.aligned : what == LVI_LOOP_TARGET ? g.h_st->tgt : g.h_st->src) + first, count, out);
        return LVI_OK;
    });
}

int32_t lvi_loop_debug_step(lvi_lidar* h, const float* T, int32_t* nn_idx, float* nn_sqd, double* sums)
{
    if (!h || !T || !nn_idx || !nn_sqd || !sums) return fail(LVI_ERR_INVALID_ARG, "null argument");
    LidarDev& d = lidar_slot0(h);
    return guarded(d.device, [&]() -> int32_t {
        lvi_loop_info r;
        const int32_t st = lp_result(d, &r);
        if (st) return st;
        LoopDev& g = *d.loop;
        if (r.status == LVI_LOOP_TOO_FEW_POINTS) return fail(LVI_ERR_STATE, "the last job had too few points: no index was used");
        hipStream_t s = g.ctx.stream;
        LVI_HIP(hipMemcpyAsync(g.st->dbgT, T, sizeof(float) * 16, hipMemcpyHostToDevice, s));
        lp_launch_nn(g, NN_DEBUG, (double)g.P.max_corr_dist * (double)g.P.max_corr_dist);
        hipLaunchKernelGGL(loop_dbgsum_kernel, dim3(1), dim3(64), 0, s, g.st, g.partial);
        LVI_HIP(hipGetLastError());
        LVI_HIP(hipMemcpyAsync(nn_idx, g.nnIdx, sizeof(int) * (size_t)r.n_source, hipMemcpyDeviceToHost, s));
        LVI_HIP(hipMemcpyAsync(nn_sqd, g.nnSqd, sizeof(float) * (size_t)r.n_source, hipMemcpyDeviceToHost, s));
        LVI_HIP(hipMemcpyAsync(sums, g.st->dbgSums, sizeof(double) * NS, hipMemcpyDeviceToHost, s));
        LVI_HIP(hipStreamSynchronize(s));
        return LVI_OK;
    });
}

}  // extern "C"
