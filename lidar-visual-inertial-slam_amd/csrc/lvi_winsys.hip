// The normal equations of a window's factors (lvi_winsys.hpp), for the marginaliser and the window solve.  All
// double.
//
//   sys_eval_proj    one thread per projection factor: residual, Jacobian and loss correction (lvi_marg_math.hpp), 2 rows of
//                    21; with a cost array also the cost 0.5 rho(s)
//   sys_prior_rows   one workgroup per row of the previous prior: dx from the blocks' values (marginalization_factor.cpp
//                    :344-362), the row r0 + J dx and J's columns scattered to their places in the system, from row prior_row0
//                    of E on; a constant block has no column
//   sys_accumulate   one workgroup per 16x16 tile of the augmented system and per chunk of 256 rows (SHARE projection
//                    factors, or 256 dense rows): the rows' values at the tile's columns are staged in LDS 64 rows at a time
//                    and every thread sums its entry over them in row order; the chunk's partial tile is written out.
//                    Nothing is scattered, so nothing serialises on the columns every factor shares, and there are no
//                    floating-point atomics.
//   sys_reduce       one thread per entry: the partials summed in chunk order; a non-finite entry raises the flag
// With store = 0 the first two leave the rows alone: the window solve's candidate state needs the costs only.
#include "lvi_dev.hpp"
#include "lvi_winsys.hpp"

using namespace lvi;
using namespace lvi_marg_math;

namespace lvi_winsys {
namespace {

__global__ __launch_bounds__(64) void sys_eval_proj(SysView d, int store)
{
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= d.P) return;
    const ProjDev p = d.proj[f];
    double r[2], J[2 * PROJ_COLS], rho[3];
    const double td = p.use_td ? d.vals[(size_t)VAL * p.blk[4]] : 0.;
    projection_eval(d.vals + (size_t)VAL * p.blk[0], d.vals + (size_t)VAL * p.blk[1], d.vals + (size_t)VAL * p.blk[2], d.vals[(size_t)VAL * p.blk[3]], td, p.use_td,
                    p.o, d.pc, r, J);
    if (d.cost || d.loss_type != LOSS_NONE) loss_rho(d.loss_type, d.loss_a, r[0] * r[0] + r[1] * r[1], rho);
    if (d.cost) d.cost[f] = 0.5 * rho[0];
    if (!store) return;
    if (d.loss_type != LOSS_NONE) loss_correct(2, PROJ_COLS, PROJ_COLS, rho, r, J);
    double* o = d.Jf + (size_t)JF * f;
    for (int a = 0; a < 2; a++) {
        for (int k = 0; k < PROJ_COLS; k++) o[(PROJ_COLS + 1) * a + k] = J[PROJ_COLS * a + k];
        o[(PROJ_COLS + 1) * a + PROJ_COLS] = r[a];
    }
}

__global__ __launch_bounds__(PRIOR_THREADS) void sys_prior_rows(SysView d, int store)
{
    __shared__ double dx[PRIOR_THREADS], red[PRIOR_THREADS];
    __shared__ int colmap[PRIOR_THREADS];
    const int row = blockIdx.x, t = threadIdx.x;
    for (int b = t; b < d.nkb0; b += PRIOR_THREADS) {
        const PriorBlk pb = d.pb[b];
        double v[VAL];
        prior_dx(pb.size, d.vals + (size_t)VAL * pb.blk, d.x0 + (size_t)VAL * b, v);
        const int ls = local_size(pb.size);
        for (int k = 0; k < ls; k++) { dx[pb.idx0 + k] = v[k]; colmap[pb.idx0 + k] = pb.newcol < 0 ? -1 : pb.newcol + k; }
    }
    double* out = d.E + (size_t)(d.prior_row0 + row) * d.P1;
    if (store)
        for (int j = t; j < d.P1; j += PRIOR_THREADS) out[j] = 0.;
    __syncthreads();
    const double* Jr = d.J0 + (size_t)row * d.n0;
    if (store)
        for (int k = t; k < d.n0; k += PRIOR_THREADS)
            if (colmap[k] >= 0) out[colmap[k]] = Jr[k];
    // r0 + J dx: n0 <= PRIOR_THREADS, one product per thread, summed by a tree whose shape is fixed
    red[t] = t < d.n0 ? Jr[t] * dx[t] : 0.;
    __syncthreads();
    for (int o = PRIOR_THREADS / 2; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    if (t == 0) {
        const double rr = d.r0[row] + red[0];
        if (store) out[d.P1 - 1] = rr;
        if (d.cost) d.cost[d.cost0 + row] = 0.5 * (rr * rr);
    }
}

// the value of row `row` of chunk c at global column g
__device__ __forceinline__ double row_value(const SysView& d, int c, int row, int g)
{
    if (g >= d.P1) return 0.;
    if (c < d.Cp) {
        const int f = c * SHARE + (row >> 1), a = row & 1;
        if (f >= d.P) return 0.;
        const double* o = d.Jf + (size_t)JF * f + (PROJ_COLS + 1) * a;
        if (g == d.P1 - 1) return o[PROJ_COLS];
        const int* col = d.proj[f].col;
#pragma unroll
        for (int b = 0; b < 5; b++) {
            const int off = col[b], sz = b < 3 ? 6 : 1, base = b < 3 ? 6 * b : 15 + b;
            if (off >= 0 && g >= off && g < off + sz) return o[base + g - off];
        }
        return 0.;
    }
    const int r = (c - d.Cp) * CH_ROWS + row;
    return r < d.rows ? d.E[(size_t)r * d.P1 + g] : 0.;
}

__global__ __launch_bounds__(TILE * TILE) void sys_accumulate(SysView d)
{
    __shared__ double xs[SUB][TILE], ys[SUB][TILE];
    const int tx = threadIdx.x, ty = threadIdx.y, t = ty * TILE + tx, c = blockIdx.z;
    const int gx0 = blockIdx.x * TILE, gy0 = blockIdx.y * TILE;
    double acc = 0.;
    for (int r0 = 0; r0 < CH_ROWS; r0 += SUB) {
        for (int e = t; e < SUB * TILE; e += TILE * TILE) {
            const int rr = e / TILE, k = e % TILE;
            xs[rr][k] = row_value(d, c, r0 + rr, gx0 + k);
            ys[rr][k] = row_value(d, c, r0 + rr, gy0 + k);
        }
        __syncthreads();
        for (int rr = 0; rr < SUB; rr++) acc += ys[rr][ty] * xs[rr][tx];
        __syncthreads();
    }
    const int i = gy0 + ty, j = gx0 + tx;
    if (i < d.P1 && j < d.P1) d.part[((size_t)c * d.P1 + i) * d.P1 + j] = acc;
}

__global__ __launch_bounds__(256) void sys_reduce(SysView d)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x, NN = (size_t)d.P1 * d.P1;
    if (e >= NN) return;
    double s = 0.;
    for (int c = 0; c < d.C; c++) s += d.part[(size_t)c * NN + e];
    d.A[e] = s;
    if (!isfinite(s)) atomicOr(d.flags, d.bit);
    if (d.corner && e == NN - 1) *d.corner = s;
}

}  // namespace

void launch_eval_proj(const SysView& v, hipStream_t s, int store)
{
    if (v.P > 0) hipLaunchKernelGGL(sys_eval_proj, dim3(div_up(v.P, 64)), dim3(64), 0, s, v, store);
}

void launch_prior_rows(const SysView& v, hipStream_t s, int store)
{
    if (v.n0 > 0) hipLaunchKernelGGL(sys_prior_rows, dim3(v.n0), dim3(PRIOR_THREADS), 0, s, v, store);
}

void launch_build(const SysView& v, hipStream_t s)
{
    const int Tn = div_up(v.P1, TILE);
    hipLaunchKernelGGL(sys_accumulate, dim3(Tn, Tn, v.C), dim3(TILE, TILE), 0, s, v);
    hipLaunchKernelGGL(sys_reduce, dim3(div_up(v.P1 * v.P1, 256)), dim3(256), 0, s, v);
}

}  // namespace lvi_winsys
