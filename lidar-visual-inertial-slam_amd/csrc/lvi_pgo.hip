// The keyframe pose graph and its optimisation on the GPU (include/lvi_pgo.h; the contract is DESIGN §18): addOdomFactor,
// addLoopFactor, isam->update and the estimate read-back of mapOptimization.cpp:1414-1428, 1509-1527, 1546-1599, as the
// minimiser of the same cost by undamped Gauss-Newton on SE(3).  All double.
//
// One Gauss-Newton step, N keys, L loops, M = 6 L + 1:
//   pgo_linearise   one thread per edge: whitened residual and the two 6x6 Jacobians (lvi_pgo_math.hpp); the prior's
//                   thread also solves delta_0 = -B_prior^-1 r_prior.  Every between factor is invariant under a common
//                   left transform, so the normal equations projected on the six gauge directions leave exactly this
//                   equation for key 0: its step is the prior's alone.  Solving it apart keeps the prior's information
//                   (1e-8 on the translation) out of a system whose other entries are 1e6.
//   pgo_assemble    one workgroup per key: the block-tridiagonal chain system T of keys 1 .. N - 1 (key 0 substituted, its
//                   block the identity) and M right-hand sides: -g and the columns of V', V = the whitened loop Jacobian
//                   (6 L x 6 N).  The normal matrix is T + V'V.
//   pgo_reduce      block cyclic reduction of T, one launch per level while a level has many keys and one last launch of
//                   a single workgroup for the rest: ceil(log2 N) levels, each eliminating every second remaining key
//   pgo_backsub     the same levels downwards: Y = T^-1 [-g, V']
//   pgo_loops       one workgroup: S = I + V Y[:, 1:] (6 L square, SPD), its Cholesky factor, z = S^-1 V Y[:, 0] (Woodbury)
//   pgo_update      one thread per key: delta = Y[:, 0] - Y[:, 1:] z, X <- X Retract(delta), the largest |component|
//                   by an atomic max on the bits of a non-negative double
// A step is active when it is the first or the step before it was taken and was not below conv_eps; every kernel of a step
// reads that from step[] and returns when the step is not active, so the whole solve is enqueued at once and waited for
// once.  No workgroup waits for another: what one launch writes, only later launches read.
//
// GPS factors (include/lvi_pgo_gps.h).  A GPS factor is not invariant under a common left transform, so with
// G >= 1 of them the shortcut for key 0 no longer holds and the step is the full system's: key 0 is a live key of the chain
// (its block Bp'Bp + A1'A1), nothing is substituted, and every GPS factor adds J'J to its key's diagonal block and J'r to the
// gradient.  The chain stays block tridiagonal, so the same reduce / backsub / loops / update launches run with N live keys.
// The factors are held sorted by key (goff[i] .. goff[i + 1] are key i's), so a key's workgroup sums its own in a fixed order.
// With G == 0 every kernel takes exactly the branches it took before GPS factors existed.
//
// lvi_pgo_gps_marginal_covariance is one pass of the same launches at the current poses with R = 6 unit right-hand sides at
// the key instead of -g (M = 6 L + 6), then pgo_cov: the (key, key) block of T^-1 - T^-1 V' S^-1 V T^-1.  Without GPS factors
// that is the block of the anchored system, and the prior's part Ad (Bp' W Bp)^-1 Ad' is added in closed form.
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "lvi_dev.hpp"
#include "lvi_pgo_math.hpp"
#include "../../include/lvi_pgo.h"
#include "../../include/lvi_pgo_gps.h"

using namespace lvi;
using namespace lvi_pgo_math;

namespace {

constexpr int NB = 64;               // threads of the per-key workgroups
constexpr int TAIL_KEYS = 16;        // reduction levels with at most this many surviving keys run inside one workgroup
constexpr int LOOPS_THREADS = 256;

struct Dev {
    Pose* X; const Pose* Zc; const Pose* Zl; const int2* lidx; const double* lsw;
    double *JAc, *JBc, *rc, *JAl, *JBl, *rl, *e2;
    double *D, *Lo, *Up, *Bm, *S, *w;
    double* delta0; double* step; lvi_pgo_info* info;
    int N, L, M, full, max_iters; double eps;
    // GPS factors, sorted by key: the key, the measurement [3], 1 / sqrt(variance) [3]; goff [N + 1]; the whitened Jacobian [18] and residual [3]
    const int* gkey; const int* goff; const double* gz; const double* gsw;
    double *JG, *rg, *cov;
    int G, R, ckey;                  // R right-hand sides ahead of the columns of V': 1 (-g) for a step, 6 (unit vectors at key ckey) for the covariance
};

__device__ __forceinline__ bool active(const Dev& d, int it) { return it == 0 || d.step[it - 1] >= d.eps; }

__constant__ double PRIOR_SW[6] = {10., 10., 0.31830988618379067154, 1e-4, 1e-4, 1e-4};       // 1 / sqrt(1e-2, 1e-2, pi^2, 1e8 x3)
__constant__ double ODOM_SW[6] = {1e3, 1e3, 1e3, 1e2, 1e2, 1e2};                               // 1 / sqrt(1e-6 x3, 1e-4 x3)
__constant__ double PRIOR_VAR[6] = {1e-2, 1e-2, 9.8696044010893586188, 1e8, 1e8, 1e8};         // mapOptimization.cpp:1418-1420

__global__ __launch_bounds__(NB) void pgo_linearise(Dev d, int it, int eval_only)
{
    if (!eval_only && !active(d, it)) return;
    const int e = blockIdx.x * NB + threadIdx.x;
    if (e >= d.N + d.L + d.G) return;
    if (e >= d.N + d.L) {
        const int g = e - d.N - d.L;
        double r3[3], J[18];
        gps_error(d.X[d.gkey[g]], d.gz + 3 * (size_t)g, r3, J);
        double s2 = 0.;
        for (int i = 0; i < 3; i++) {
            const double sw = d.gsw[3 * (size_t)g + i], rw = sw * r3[i];
            s2 += rw * rw;
            if (!eval_only) {
                d.rg[3 * (size_t)g + i] = rw;
                for (int j = 0; j < 6; j++) d.JG[18 * (size_t)g + 6 * i + j] = sw * J[6 * i + j];
            }
        }
        d.e2[e] = s2;
        return;
    }
    double r[6], A[36], B[36], sw[6];
    double *oA, *oB, *orr;
    if (e == 0) {
        prior_error(d.X[0], d.Zc[0], d.full, r, B);
        for (int k = 0; k < 36; k++) A[k] = 0.;
        if (!eval_only) {
            double Bc[36], x[6];
            for (int k = 0; k < 36; k++) Bc[k] = B[k];
            for (int k = 0; k < 6; k++) x[k] = -r[k];
            solve6(Bc, x);
            for (int k = 0; k < 6; k++) d.delta0[k] = x[k];
        }
        for (int k = 0; k < 6; k++) sw[k] = PRIOR_SW[k];
        oA = d.JAc; oB = d.JBc; orr = d.rc;
    } else if (e < d.N) {
        between_error(d.X[e - 1], d.X[e], d.Zc[e], d.full, r, A, B);
        for (int k = 0; k < 6; k++) sw[k] = ODOM_SW[k];
        oA = d.JAc + 36 * (size_t)e; oB = d.JBc + 36 * (size_t)e; orr = d.rc + 6 * (size_t)e;
    } else {
        const int l = e - d.N;
        const int2 ft = d.lidx[l];
        between_error(d.X[ft.x], d.X[ft.y], d.Zl[l], d.full, r, A, B);
        for (int k = 0; k < 6; k++) sw[k] = d.lsw[l];
        oA = d.JAl + 36 * (size_t)l; oB = d.JBl + 36 * (size_t)l; orr = d.rl + 6 * (size_t)l;
    }
    double s2 = 0.;
    for (int i = 0; i < 6; i++) {
        const double rw = sw[i] * r[i];
        s2 += rw * rw;
        if (!eval_only) {
            orr[i] = rw;
            for (int j = 0; j < 6; j++) { oA[6 * i + j] = sw[i] * A[6 * i + j]; oB[6 * i + j] = sw[i] * B[6 * i + j]; }
        }
    }
    d.e2[e] = s2;
}

// (P' Q)[a][b] of two row-major 6x6
__device__ __forceinline__ double ptq(const double* P, const double* Q, int a, int b)
{
    double s = 0.;
    for (int k = 0; k < 6; k++) s += P[6 * k + a] * Q[6 * k + b];
    return s;
}
// (P' v)[a]
__device__ __forceinline__ double ptv(const double* P, const double* v, int a)
{
    double s = 0.;
    for (int k = 0; k < 6; k++) s += P[6 * k + a] * v[k];
    return s;
}

__global__ __launch_bounds__(NB) void pgo_assemble(Dev d, int it)
{
    if (!active(d, it)) return;
    const int i = blockIdx.x, N = d.N, M = d.M, R = d.R;
    const bool fs = d.G > 0;                                      // the full system: key 0 is live
    const int g0 = fs ? d.goff[i] : 0, g1 = fs ? d.goff[i + 1] : 0;
    double* Di = d.D + 36 * (size_t)i;
    double* Loi = d.Lo + 36 * (size_t)i;
    double* Upi = d.Up + 36 * (size_t)i;
    double* Bi = d.Bm + 6 * (size_t)M * i;
    const int total = 108 + 6 * M;
    for (int t = threadIdx.x; t < total; t += NB) {
        if (t < 108) {
            const int which = t / 36, a = (t % 36) / 6, b = t % 6;
            double v = 0.;
            if (i == 0 && !fs) {
                v = which == 0 && a == b ? 1. : 0.;
            } else if (which == 0) {
                v = ptq(d.JBc + 36 * (size_t)i, d.JBc + 36 * (size_t)i, a, b);
                if (i + 1 < N) v += ptq(d.JAc + 36 * (size_t)(i + 1), d.JAc + 36 * (size_t)(i + 1), a, b);
                for (int g = g0; g < g1; g++)
                    for (int k = 0; k < 3; k++) v += d.JG[18 * (size_t)g + 6 * k + a] * d.JG[18 * (size_t)g + 6 * k + b];
            } else if (which == 1) {
                if (i >= (fs ? 1 : 2)) v = ptq(d.JBc + 36 * (size_t)i, d.JAc + 36 * (size_t)i, a, b);            // row i, column i - 1
            } else {
                if (i + 1 < N) v = ptq(d.JAc + 36 * (size_t)(i + 1), d.JBc + 36 * (size_t)(i + 1), a, b);   // row i, column i + 1
            }
            (which == 0 ? Di : which == 1 ? Loi : Upi)[6 * a + b] = v;
            continue;
        }
        const int q = t - 108, a = q / M, col = q % M;            // row a of the key's block, right-hand side col
        double v = 0.;
        if (i > 0 || fs) {
            if (col < R && R == 6) {
                v = i == d.ckey && col == a ? 1. : 0.;            // the covariance's unit right-hand sides
            } else if (col == 0) {
                // -g_i, with delta_0 substituted into the edges that touch key 0 (not in the full system)
                double rr[6];
                for (int k = 0; k < 6; k++) rr[k] = d.rc[6 * (size_t)i + k];
                if (i == 1 && !fs) for (int k = 0; k < 6; k++) for (int j = 0; j < 6; j++) rr[k] += d.JAc[36 + 6 * k + j] * d.delta0[j];
                v = ptv(d.JBc + 36 * (size_t)i, rr, a);
                if (i + 1 < N) v += ptv(d.JAc + 36 * (size_t)(i + 1), d.rc + 6 * (size_t)(i + 1), a);
                for (int l = 0; l < d.L; l++) {
                    const int2 ft = d.lidx[l];
                    if (ft.x != i && ft.y != i) continue;
                    const double* Jo = fs ? nullptr : ft.x == 0 ? d.JAl + 36 * (size_t)l : ft.y == 0 ? d.JBl + 36 * (size_t)l : nullptr;
                    for (int k = 0; k < 6; k++) {
                        rr[k] = d.rl[6 * (size_t)l + k];
                        if (Jo) for (int j = 0; j < 6; j++) rr[k] += Jo[6 * k + j] * d.delta0[j];
                    }
                    v += ptv((ft.x == i ? d.JAl : d.JBl) + 36 * (size_t)l, rr, a);
                }
                for (int g = g0; g < g1; g++)
                    for (int k = 0; k < 3; k++) v += d.JG[18 * (size_t)g + 6 * k + a] * d.rg[3 * (size_t)g + k];
                v = -v;
            } else {
                const int l = (col - R) / 6, k = (col - R) % 6;       // row k of loop l's Jacobian = column of V'
                const int2 ft = d.lidx[l];
                if (ft.x == i) v = d.JAl[36 * (size_t)l + 6 * k + a];
                else if (ft.y == i) v = d.JBl[36 * (size_t)l + 6 * k + a];
            }
        }
        Bi[(size_t)a * M + col] = v;
    }
}

// levels s = s_first, 2 s_first, ... (n_levels of them): the keys 2 s m survive, their neighbours 2 s m -+ s are eliminated.
// More than one level only with a single workgroup.
__global__ __launch_bounds__(NB) void pgo_reduce(Dev d, int it, int s_first, int n_levels)
{
    if (!active(d, it)) return;
    __shared__ double sLo[36], sUp[36], sLa[36], sLc[36];
    const int N = d.N, M = d.M;
    int s = s_first;
    for (int lev = 0; lev < n_levels; lev++, s *= 2) {
        const int count = (N + 2 * s - 1) / (2 * s);
        for (int m = blockIdx.x; m < count; m += gridDim.x) {
            const int i = 2 * s * m, a = i - s, c = i + s;
            const bool ha = a >= 0, hc = c < N;
            if (threadIdx.x < 36) { sLo[threadIdx.x] = d.Lo[36 * (size_t)i + threadIdx.x]; sUp[threadIdx.x] = d.Up[36 * (size_t)i + threadIdx.x]; }
            if (threadIdx.x == 62 && ha) chol6(d.D + 36 * (size_t)a, sLa);
            if (threadIdx.x == 63 && hc) chol6(d.D + 36 * (size_t)c, sLc);
            __syncthreads();
            for (int q = threadIdx.x; q < 18 + M; q += NB) {
                double ya[6] = {0, 0, 0, 0, 0, 0}, yc[6] = {0, 0, 0, 0, 0, 0};
                const int kind = q < 6 ? 0 : q < 12 ? 1 : q < 18 ? 2 : 3;
                const int col = kind == 3 ? q - 18 : q % 6;
                const bool use_a = ha && kind != 2, use_c = hc && kind != 1;
                if (use_a) {
                    const double* src = kind == 0 ? d.Up + 36 * (size_t)a : kind == 1 ? d.Lo + 36 * (size_t)a : d.Bm + 6 * (size_t)M * a;
                    const int ld = kind == 3 ? M : 6;
                    for (int r = 0; r < 6; r++) ya[r] = src[(size_t)r * ld + col];
                    chol6_solve(sLa, ya);
                }
                if (use_c) {
                    const double* src = kind == 0 ? d.Lo + 36 * (size_t)c : kind == 2 ? d.Up + 36 * (size_t)c : d.Bm + 6 * (size_t)M * c;
                    const int ld = kind == 3 ? M : 6;
                    for (int r = 0; r < 6; r++) yc[r] = src[(size_t)r * ld + col];
                    chol6_solve(sLc, yc);
                }
                for (int r = 0; r < 6; r++) {
                    double ca = 0., cc = 0.;
                    for (int k = 0; k < 6; k++) { ca += sLo[6 * r + k] * ya[k]; cc += sUp[6 * r + k] * yc[k]; }
                    if (kind == 0) d.D[36 * (size_t)i + 6 * r + col] -= ca + cc;
                    else if (kind == 1) d.Lo[36 * (size_t)i + 6 * r + col] = -ca;          // now row i, column i - 2 s
                    else if (kind == 2) d.Up[36 * (size_t)i + 6 * r + col] = -cc;          // now row i, column i + 2 s
                    else d.Bm[6 * (size_t)M * i + (size_t)r * M + col] -= ca + cc;
                }
            }
            __syncthreads();
        }
    }
}

// the root (key 0, when with_root) and then the levels s = s_first, s_first / 2, ... (n_levels of them) downwards: the keys
// s (2 m + 1) take their solution from their two neighbours at distance s.  More than one level, or the root with a level,
// only with a single workgroup.
__global__ __launch_bounds__(NB) void pgo_backsub(Dev d, int it, int with_root, int s_first, int n_levels)
{
    if (!active(d, it)) return;
    __shared__ double sL[36];
    const int N = d.N, M = d.M;
    if (with_root && blockIdx.x == 0) {
        if (threadIdx.x == 0) chol6(d.D, sL);
        __syncthreads();
        for (int col = threadIdx.x; col < M; col += NB) {
            double x[6];
            for (int r = 0; r < 6; r++) x[r] = d.Bm[(size_t)r * M + col];
            chol6_solve(sL, x);
            for (int r = 0; r < 6; r++) d.Bm[(size_t)r * M + col] = x[r];
        }
        __syncthreads();
    }
    int s = s_first;
    for (int lev = 0; lev < n_levels; lev++, s /= 2) {
        const int count = ((N - 1) / s + 1) / 2;
        for (int m = blockIdx.x; m < count; m += gridDim.x) {
            const int i = s * (2 * m + 1), a = i - s, c = i + s;
            if (threadIdx.x == 0) chol6(d.D + 36 * (size_t)i, sL);
            __syncthreads();
            const double *Lo = d.Lo + 36 * (size_t)i, *Up = d.Up + 36 * (size_t)i;
            double* Bi = d.Bm + 6 * (size_t)M * i;
            const double* Ba = d.Bm + 6 * (size_t)M * a;
            const double* Bc = c < N ? d.Bm + 6 * (size_t)M * c : nullptr;
            for (int col = threadIdx.x; col < M; col += NB) {
                double x[6], xa[6], xc[6] = {0, 0, 0, 0, 0, 0};
                for (int r = 0; r < 6; r++) { x[r] = Bi[(size_t)r * M + col]; xa[r] = Ba[(size_t)r * M + col]; if (Bc) xc[r] = Bc[(size_t)r * M + col]; }
                for (int r = 0; r < 6; r++) {
                    double t = 0.;
                    for (int k = 0; k < 6; k++) t += Lo[6 * r + k] * xa[k] + Up[6 * r + k] * xc[k];
                    x[r] -= t;
                }
                chol6_solve(sL, x);
                for (int r = 0; r < 6; r++) Bi[(size_t)r * M + col] = x[r];
            }
            __syncthreads();
        }
    }
}

// one workgroup: S = I + V Y[:, R:], w = V Y[:, :R] (6 L x R, row-major); Cholesky of S in place; w <- S^-1 w
__global__ __launch_bounds__(LOOPS_THREADS) void pgo_loops(Dev d, int it)
{
    if (!active(d, it)) return;
    const int n = 6 * d.L, M = d.M, R = d.R, T = LOOPS_THREADS, tid = threadIdx.x;
    if (n == 0) return;
    double* S = d.S;
    double* w = d.w;
    for (int e = tid; e < n * (n + R); e += T) {
        const int p = e / (n + R), qq = e % (n + R);              // qq >= n: a right-hand side
        const int l = p / 6, k = p % 6, col = qq >= n ? qq - n : R + qq;
        const int2 ft = d.lidx[l];
        const double *Ya = d.Bm + 6 * (size_t)M * ft.x, *Yb = d.Bm + 6 * (size_t)M * ft.y;
        const double *Ja = d.JAl + 36 * (size_t)l + 6 * k, *Jb = d.JBl + 36 * (size_t)l + 6 * k;
        double v = 0.;
        for (int r = 0; r < 6; r++) v += Ja[r] * Ya[(size_t)r * M + col] + Jb[r] * Yb[(size_t)r * M + col];
        if (qq >= n) w[(size_t)p * R + (qq - n)] = v;
        else S[(size_t)p * n + qq] = v + (p == qq ? 1. : 0.);
    }
    __syncthreads();
    for (int j = 0; j < n; j++) {
        if (tid == 0) S[(size_t)j * n + j] = sqrt(S[(size_t)j * n + j]);
        __syncthreads();
        const double dj = S[(size_t)j * n + j];
        for (int p = j + 1 + tid; p < n; p += T) S[(size_t)p * n + j] /= dj;
        __syncthreads();
        const int rem = n - j - 1;
        for (int e = tid; e < rem * rem; e += T) {
            const int p = j + 1 + e / rem, q = j + 1 + e % rem;
            if (q <= p) S[(size_t)p * n + q] -= S[(size_t)p * n + j] * S[(size_t)q * n + j];
        }
        __syncthreads();
    }
    for (int j = 0; j < n; j++) {                                 // L y = w
        if (tid < R) w[(size_t)j * R + tid] /= S[(size_t)j * n + j];
        __syncthreads();
        for (int e = tid; e < (n - j - 1) * R; e += T) {
            const int p = j + 1 + e / R, c = e % R;
            w[(size_t)p * R + c] -= S[(size_t)p * n + j] * w[(size_t)j * R + c];
        }
        __syncthreads();
    }
    for (int j = n - 1; j >= 0; j--) {                            // L' z = y
        if (tid < R) w[(size_t)j * R + tid] /= S[(size_t)j * n + j];
        __syncthreads();
        for (int e = tid; e < j * R; e += T) {
            const int p = e / R, c = e % R;
            w[(size_t)p * R + c] -= S[(size_t)j * n + p] * w[(size_t)j * R + c];
        }
        __syncthreads();
    }
}

// one workgroup, after a pass with R = 6: cov = the (ckey, ckey) block of T^-1 - T^-1 V' S^-1 V T^-1 = Y[:, :6] - Y[:, 6:] w at
// the key's rows.  Without GPS factors T is the anchored system (key 0's block the identity, its right-hand sides zero), the
// block is Sigma_rel, and the gauge part is added in closed form: A Sigma_0 A', A = Ad(X_k^-1 X_0), Sigma_0 = (Bp' W Bp)^-1 =
// Bp^-1 diag(variances) Bp^-T from the unwhitened prior Jacobian, so 1e-8 never meets 1e6 in one matrix.
__global__ __launch_bounds__(NB) void pgo_cov(Dev d)
{
    __shared__ double sA[36], sS0[36];
    const int tid = threadIdx.x, M = d.M, n = 6 * d.L, k = d.ckey;
    const bool fs = d.G > 0;
    if (!fs && tid == 0) {
        double r[6], B[36], Bi[36];
        prior_error(d.X[0], d.Zc[0], d.full, r, B);
        for (int c = 0; c < 6; c++) {                             // column c of Bp^-1
            double Bc[36], x[6];
            for (int q = 0; q < 36; q++) Bc[q] = B[q];
            for (int q = 0; q < 6; q++) x[q] = q == c ? 1. : 0.;
            solve6(Bc, x);
            for (int q = 0; q < 6; q++) Bi[6 * q + c] = x[q];
        }
        for (int a = 0; a < 6; a++)
            for (int b = 0; b < 6; b++) {
                double s = 0.;
                for (int m = 0; m < 6; m++) s += Bi[6 * a + m] * PRIOR_VAR[m] * Bi[6 * b + m];
                sS0[6 * a + b] = s;
            }
        Pose Xi, Rel;
        pose_inv(d.X[k], &Xi);
        pose_mul(Xi, d.X[0], &Rel);
        pose_adjoint(Rel, sA);
    }
    __syncthreads();
    if (tid >= 36) return;
    const int r = tid / 6, c = tid % 6;
    const double* Y = d.Bm + 6 * (size_t)M * k;
    double s = 0.;
    for (int q = 0; q < n; q++) s += Y[(size_t)r * M + 6 + q] * d.w[(size_t)q * 6 + c];
    double v = Y[(size_t)r * M + c] - s;
    if (!fs) {
        double g = 0.;
        for (int a = 0; a < 6; a++) {
            double t = 0.;
            for (int b = 0; b < 6; b++) t += sS0[6 * a + b] * sA[6 * c + b];
            g += sA[6 * r + a] * t;
        }
        v += g;
    }
    d.cov[tid] = v;
}

__global__ __launch_bounds__(NB) void pgo_update(Dev d, int it)
{
    if (!active(d, it)) return;
    const int i = blockIdx.x * NB + threadIdx.x, M = d.M, n = 6 * d.L;
    double m = 0.;
    bool bad = false;
    if (i < d.N) {
        double delta[6];
        if (i == 0 && d.G == 0) {
            for (int r = 0; r < 6; r++) delta[r] = d.delta0[r];
        } else {
            const double* Y = d.Bm + 6 * (size_t)M * i;
            for (int r = 0; r < 6; r++) {
                double s = 0.;
                for (int q = 0; q < n; q++) s += Y[(size_t)r * M + 1 + q] * d.w[q];
                delta[r] = Y[(size_t)r * M] - s;
            }
        }
        for (int r = 0; r < 6; r++) {
            const double a = fabs(delta[r]);
            if (!(a == a) || isinf(a)) bad = true;
            else if (a > m) m = a;
        }
        if (!bad) {
            Pose X = d.X[i];
            pose_retract(&X, delta, d.full);
            d.X[i] = X;
        }
    }
    if (bad) m = std::numeric_limits<double>::quiet_NaN();         // its bits exceed every finite double's: the max keeps it, and the solve ends
    unsigned long long b = (unsigned long long)__double_as_longlong(m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long t = __shfl_xor(b, o, 64); b = t > b ? t : b; }
    if (lane_id() == 0) atomicMax(reinterpret_cast<unsigned long long*>(d.step + it), b);
}

// one workgroup: the sum of the squared whitened errors in a fixed order; which = 0: chi2_before, 1: chi2_after and the
// record of the steps
__global__ __launch_bounds__(LOOPS_THREADS) void pgo_finish(Dev d, int which)
{
    __shared__ double sh[LOOPS_THREADS];
    const int tid = threadIdx.x, E = d.N + d.L + d.G;
    double s = 0.;
    for (int e = tid; e < E; e += LOOPS_THREADS) s += d.e2[e];
    sh[tid] = s;
    __syncthreads();
    for (int o = LOOPS_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) sh[tid] += sh[tid + o];
        __syncthreads();
    }
    if (tid != 0) return;
    if (which == 0) { d.info->chi2_before = sh[0]; return; }
    d.info->chi2_after = sh[0];
    int iters = 0, conv = 0;
    double last = 0.;
    for (int it = 0; it < d.max_iters; it++) {
        if (!active(d, it)) break;
        iters++;
        last = d.step[it];
        conv = last < d.eps ? 1 : 0;
    }
    d.info->iterations = iters; d.info->converged = conv; d.info->max_step = last;
}

}  // namespace

// ---------------------------------------------------------------------------------------------- the handle
struct lvi_pgo : Handle {
    int Ncap = 0, Lcap = 0;
    int N = 0, L = 0, n_up = 0, l_up = 0;          // keys / loops added, and how many of them the device already holds
    lvi_pgo_params P{};
    Dev d{};
    // pinned host staging
    Pose *h_X = nullptr, *h_Zc = nullptr, *h_Zl = nullptr, *h_out = nullptr;
    int2* h_lidx = nullptr; double* h_lsw = nullptr; lvi_pgo_info* h_info = nullptr;
    Pose* d_Zc = nullptr; Pose* d_Zl = nullptr; int2* d_lidx = nullptr; double* d_lsw = nullptr;
    // GPS factors in the order they were added; the device holds them sorted by key (staged and sent by flush when they or N changed)
    std::vector<int> g_key; std::vector<double> g_z, g_sw;
    int g_up_G = 0, g_up_N = 0;
    int *h_gkey = nullptr, *h_goff = nullptr; double *h_gz = nullptr, *h_gsw = nullptr, *h_cov = nullptr;
    int *d_gkey = nullptr, *d_goff = nullptr; double *d_gz = nullptr, *d_gsw = nullptr;
};

namespace {

template <class A, class B> void carve(A& a, B& pin, lvi_pgo* h)
{
    const size_t N = (size_t)h->Ncap, L = (size_t)std::max(h->Lcap, 1), M = 6 * (size_t)h->Lcap + 6, n6 = 6 * L;
    Dev& d = h->d;
    alloc_pair(a, pin, d.X, h->h_X, N); h->h_out = pin.template alloc<Pose>(N);
    alloc_pair(a, pin, h->d_Zc, h->h_Zc, N); alloc_pair(a, pin, h->d_Zl, h->h_Zl, L);
    alloc_pair(a, pin, h->d_lidx, h->h_lidx, L); alloc_pair(a, pin, h->d_lsw, h->h_lsw, L);
    d.JAc = a.template alloc<double>(36 * N); d.JBc = a.template alloc<double>(36 * N); d.rc = a.template alloc<double>(6 * N);
    d.JAl = a.template alloc<double>(36 * L); d.JBl = a.template alloc<double>(36 * L); d.rl = a.template alloc<double>(6 * L);
    d.e2 = a.template alloc<double>(N + L + N);
    d.D = a.template alloc<double>(36 * N); d.Lo = a.template alloc<double>(36 * N); d.Up = a.template alloc<double>(36 * N);
    d.Bm = a.template alloc<double>(6 * N * M);
    d.S = a.template alloc<double>(n6 * n6); d.w = a.template alloc<double>(n6 * 6);
    d.delta0 = a.template alloc<double>(6); d.step = a.template alloc<double>(LVI_PGO_MAX_ITERS);
    alloc_pair(a, pin, d.info, h->h_info, 1);
    alloc_pair(a, pin, h->d_gkey, h->h_gkey, N); alloc_pair(a, pin, h->d_goff, h->h_goff, N + 1);
    alloc_pair(a, pin, h->d_gz, h->h_gz, 3 * N); alloc_pair(a, pin, h->d_gsw, h->h_gsw, 3 * N);
    d.JG = a.template alloc<double>(18 * N); d.rg = a.template alloc<double>(3 * N); alloc_pair(a, pin, d.cov, h->h_cov, 36);
}

// what add_pose / add_loop staged since the last flush goes to the device (stream order: ahead of whatever reads it)
void flush(lvi_pgo* h)
{
    if (h->n_up < h->N) {
        const size_t n = (size_t)(h->N - h->n_up);
        LVI_HIP(hipMemcpyAsync(h->d.X + h->n_up, h->h_X + h->n_up, sizeof(Pose) * n, hipMemcpyHostToDevice, h->stream));
        LVI_HIP(hipMemcpyAsync(h->d_Zc + h->n_up, h->h_Zc + h->n_up, sizeof(Pose) * n, hipMemcpyHostToDevice, h->stream));
        h->n_up = h->N;
    }
    if (h->l_up < h->L) {
        const size_t n = (size_t)(h->L - h->l_up);
        LVI_HIP(hipMemcpyAsync(h->d_Zl + h->l_up, h->h_Zl + h->l_up, sizeof(Pose) * n, hipMemcpyHostToDevice, h->stream));
        LVI_HIP(hipMemcpyAsync(h->d_lidx + h->l_up, h->h_lidx + h->l_up, sizeof(int2) * n, hipMemcpyHostToDevice, h->stream));
        LVI_HIP(hipMemcpyAsync(h->d_lsw + h->l_up, h->h_lsw + h->l_up, sizeof(double) * n, hipMemcpyHostToDevice, h->stream));
        h->l_up = h->L;
    }
    const int G = (int)h->g_key.size();
    if (G > 0 && (h->g_up_G != G || h->g_up_N != h->N)) {
        // a stable counting sort by key: goff[i] .. goff[i + 1] are key i's factors, in the order they were added
        int* off = h->h_goff;
        for (int i = 0; i <= h->N; i++) off[i] = 0;
        for (int g = 0; g < G; g++) off[h->g_key[g] + 1]++;
        for (int i = 0; i < h->N; i++) off[i + 1] += off[i];
        std::vector<int> next(off, off + h->N);
        for (int g = 0; g < G; g++) {
            const int at = next[h->g_key[g]]++;
            h->h_gkey[at] = h->g_key[g];
            for (int k = 0; k < 3; k++) { h->h_gz[3 * (size_t)at + k] = h->g_z[3 * (size_t)g + k]; h->h_gsw[3 * (size_t)at + k] = h->g_sw[3 * (size_t)g + k]; }
        }
        LVI_HIP(hipMemcpyAsync(h->d_gkey, h->h_gkey, sizeof(int) * (size_t)G, hipMemcpyHostToDevice, h->stream));
        LVI_HIP(hipMemcpyAsync(h->d_goff, h->h_goff, sizeof(int) * (size_t)(h->N + 1), hipMemcpyHostToDevice, h->stream));
        LVI_HIP(hipMemcpyAsync(h->d_gz, h->h_gz, sizeof(double) * 3 * (size_t)G, hipMemcpyHostToDevice, h->stream));
        LVI_HIP(hipMemcpyAsync(h->d_gsw, h->h_gsw, sizeof(double) * 3 * (size_t)G, hipMemcpyHostToDevice, h->stream));
        h->g_up_G = G; h->g_up_N = h->N;
    }
}

// the device view of the graph as it stands, with R right-hand sides
Dev view(lvi_pgo* h, int R)
{
    Dev d = h->d;
    d.Zc = h->d_Zc; d.Zl = h->d_Zl; d.lidx = h->d_lidx; d.lsw = h->d_lsw;
    d.gkey = h->d_gkey; d.goff = h->d_goff; d.gz = h->d_gz; d.gsw = h->d_gsw;
    d.N = h->N; d.L = h->L; d.G = (int)h->g_key.size(); d.R = R; d.M = 6 * h->L + R; d.ckey = 0;
    d.full = h->P.full_logmap; d.max_iters = h->P.max_iters; d.eps = h->P.conv_eps;
    return d;
}

// the launches of one linear solve Y = T^-1 B and the loop system, step `it` (linearise is the caller's)
struct Schedule { int n_wide = 0, s_tail = 1, n_tail = 0; };
Schedule schedule(int N)
{
    // single-level launches while more than TAIL_KEYS keys survive a level, then one workgroup
    Schedule c;
    for (int st = 1; st < N; st *= 2) {
        const int count = (N + 2 * st - 1) / (2 * st);
        if (count > TAIL_KEYS && c.n_tail == 0) c.n_wide++;
        else { if (c.n_tail == 0) c.s_tail = st; c.n_tail++; }
    }
    return c;
}
void enqueue_linear_solve(const Dev& d, const Schedule& c, int it, hipStream_t s)
{
    const int N = d.N, n_wide = c.n_wide, s_tail = c.s_tail, n_tail = c.n_tail;
    hipLaunchKernelGGL(pgo_assemble, dim3(N), dim3(NB), 0, s, d, it);
    int st = 1;
    for (int k = 0; k < n_wide; k++, st *= 2)
        hipLaunchKernelGGL(pgo_reduce, dim3((N + 2 * st - 1) / (2 * st)), dim3(NB), 0, s, d, it, st, 1);
    if (n_tail > 0) hipLaunchKernelGGL(pgo_reduce, dim3(1), dim3(NB), 0, s, d, it, s_tail, n_tail);
    // downwards: the root and the tail levels in one workgroup, then the wide levels
    const int s_top = n_tail > 0 ? s_tail << (n_tail - 1) : 0;
    hipLaunchKernelGGL(pgo_backsub, dim3(1), dim3(NB), 0, s, d, it, 1, s_top, n_tail);
    st = n_wide > 0 ? 1 << (n_wide - 1) : 0;
    for (int k = 0; k < n_wide; k++, st /= 2)
        hipLaunchKernelGGL(pgo_backsub, dim3(((N - 1) / st + 1) / 2), dim3(NB), 0, s, d, it, 0, st, 1);
    if (d.L > 0) hipLaunchKernelGGL(pgo_loops, dim3(1), dim3(LOOPS_THREADS), 0, s, d, it);
}

bool params_ok(const lvi_pgo_params& p)
{
    return (p.full_logmap == 0 || p.full_logmap == 1) && p.max_iters >= 1 && p.max_iters <= LVI_PGO_MAX_ITERS && p.conv_eps > 0. && std::isfinite(p.conv_eps);
}

}  // namespace

extern "C" {

int32_t lvi_pgo_abi_version(void) { return LVI_PGO_ABI_VERSION; }

void lvi_pgo_params_default(lvi_pgo_params* p)
{
    if (!p) return;
    p->full_logmap = 1; p->max_iters = 10; p->conv_eps = 1e-10;
}

int32_t lvi_pgo_create(int32_t device, int32_t max_poses, int32_t max_loops, lvi_pgo** out)
{
    if (!out) return fail(LVI_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (max_poses < 1 || max_poses > LVI_PGO_MAX_POSES) return fail(LVI_ERR_INVALID_ARG, "max_poses must be 1..LVI_PGO_MAX_POSES");
    if (max_loops < 0 || max_loops > LVI_PGO_MAX_LOOPS) return fail(LVI_ERR_INVALID_ARG, "max_loops must be 0..LVI_PGO_MAX_LOOPS");
    return create_handle(device, out, lvi_pgo_destroy,
        [&](lvi_pgo* h) { h->Ncap = max_poses; h->Lcap = max_loops; lvi_pgo_params_default(&h->P); },
        [&](lvi_pgo* h) -> int32_t { h->open(device, [&](auto& dev, auto& pin) { carve(dev, pin, h); }); return LVI_OK; });
}

void lvi_pgo_destroy(lvi_pgo* h)
{
    if (!h) return;
    h->close();
    delete h;
}

int32_t lvi_pgo_clear(lvi_pgo* h)
{
    if (!h) return fail(LVI_ERR_INVALID_ARG, "null argument");
    return guarded(h->device, [&]() -> int32_t {
        LVI_HIP(hipStreamSynchronize(h->stream));
        h->N = h->L = h->n_up = h->l_up = 0;
        h->g_key.clear(); h->g_z.clear(); h->g_sw.clear();
        h->g_up_G = h->g_up_N = 0;
        return LVI_OK;
    });
}

int32_t lvi_pgo_set_params(lvi_pgo* h, const lvi_pgo_params* p)
{
    if (!h || !p) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (!params_ok(*p)) return fail(LVI_ERR_INVALID_ARG, "full_logmap must be 0 or 1, max_iters 1..LVI_PGO_MAX_ITERS, conv_eps > 0");
    h->P = *p;
    return LVI_OK;
}

int32_t lvi_pgo_count(lvi_pgo* h, int32_t* n_poses, int32_t* n_loops)
{
    if (!h) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (n_poses) *n_poses = h->N;
    if (n_loops) *n_loops = h->L;
    return LVI_OK;
}

int32_t lvi_pgo_add_pose(lvi_pgo* h, const float pose_from[6], const float pose_to[6], int32_t* index_out)
{
    if (!h || !pose_to || (h->N > 0 && !pose_from)) return fail(LVI_ERR_INVALID_ARG, "null argument");
    for (int k = 0; k < 6; k++)
        if (!std::isfinite(pose_to[k]) || (h->N > 0 && !std::isfinite(pose_from[k]))) return fail(LVI_ERR_INVALID_ARG, "a pose is not finite");
    if (h->N >= h->Ncap) return fail(LVI_ERR_CAPACITY, "more poses than max_poses");
    Pose to;
    pose_from_rpyxyz(pose_to, &to);
    if (h->N == 0) {
        h->h_Zc[0] = to;                                         // PriorFactor(0, poseTo)
    } else {
        Pose from, fi;
        pose_from_rpyxyz(pose_from, &from);
        pose_inv(from, &fi);
        pose_mul(fi, to, &h->h_Zc[h->N]);                        // poseFrom.between(poseTo)
    }
    h->h_X[h->N] = to;
    if (index_out) *index_out = h->N;
    h->N++;
    return LVI_OK;
}

int32_t lvi_pgo_add_loop(lvi_pgo* h, int32_t from, int32_t to, const double between[16], float variance)
{
    if (!h || !between) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (from == to || from < 0 || to < 0 || from >= h->N || to >= h->N) return fail(LVI_ERR_INVALID_ARG, "loop keys must differ and lie inside the keys added");
    if (!(variance > 0.f) || !std::isfinite(variance)) return fail(LVI_ERR_INVALID_ARG, "variance must be positive and finite");
    for (int k = 0; k < 16; k++) if (!std::isfinite(between[k])) return fail(LVI_ERR_INVALID_ARG, "between is not finite");
    if (h->L >= h->Lcap) return fail(LVI_ERR_CAPACITY, "more loops than max_loops");
    pose_from_matrix(between, &h->h_Zl[h->L]);
    h->h_lidx[h->L] = int2{from, to};
    h->h_lsw[h->L] = 1. / std::sqrt((double)variance);
    h->L++;
    return LVI_OK;
}

int32_t lvi_pgo_solve(lvi_pgo* h, lvi_pgo_info* info_out)
{
    if (!h) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (h->N == 0) return fail(LVI_ERR_STATE, "no poses");
    return guarded(h->device, [&]() -> int32_t {
        flush(h);
        const Dev d = view(h, 1);
        const int N = d.N, E = d.N + d.L + d.G;
        hipStream_t s = h->stream;
        LVI_HIP(hipMemsetAsync(d.step, 0, sizeof(double) * LVI_PGO_MAX_ITERS, s));
        const Schedule c = schedule(N);
        for (int it = 0; it < d.max_iters; it++) {
            hipLaunchKernelGGL(pgo_linearise, dim3(div_up(E, NB)), dim3(NB), 0, s, d, it, 0);
            if (it == 0) hipLaunchKernelGGL(pgo_finish, dim3(1), dim3(LOOPS_THREADS), 0, s, d, 0);
            enqueue_linear_solve(d, c, it, s);
            hipLaunchKernelGGL(pgo_update, dim3(div_up(N, NB)), dim3(NB), 0, s, d, it);
            LVI_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(pgo_linearise, dim3(div_up(E, NB)), dim3(NB), 0, s, d, 0, 1);
        hipLaunchKernelGGL(pgo_finish, dim3(1), dim3(LOOPS_THREADS), 0, s, d, 1);
        LVI_HIP(hipGetLastError());
        LVI_HIP(hipMemcpyAsync(h->h_info, d.info, sizeof(lvi_pgo_info), hipMemcpyDeviceToHost, s));
        LVI_HIP(hipStreamSynchronize(s));                            // the solve's one wait
        if (info_out) *info_out = *h->h_info;
        return h->h_info->converged ? LVI_OK : LVI_PGO_NOT_CONVERGED;
    });
}

int32_t lvi_pgo_get_poses(lvi_pgo* h, int32_t first, int32_t count, double* T, float* rpyxyz)
{
    if (!h) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (first < 0 || count < 0 || first > h->N || count > h->N - first) return fail(LVI_ERR_INVALID_ARG, "window outside the poses");
    if (count == 0) return LVI_OK;
    return guarded(h->device, [&]() -> int32_t {
        flush(h);
        LVI_HIP(hipMemcpyAsync(h->h_out, h->d.X + first, sizeof(Pose) * (size_t)count, hipMemcpyDeviceToHost, h->stream));
        LVI_HIP(hipStreamSynchronize(h->stream));
        for (int i = 0; i < count; i++) {
            if (T) pose_to_matrix(h->h_out[i], T + 16 * (size_t)i);
            if (rpyxyz) pose_to_rpyxyz(h->h_out[i], rpyxyz + 6 * (size_t)i);
        }
        return LVI_OK;
    });
}

// ---------------------------------------------------------------------------------------------- include/lvi_pgo_gps.h
int32_t lvi_pgo_gps_abi_version(void) { return LVI_PGO_GPS_ABI_VERSION; }

int32_t lvi_pgo_gps_add(lvi_pgo* h, int32_t key, const float xyz[3], const float variance[3])
{
    if (!h || !xyz || !variance) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (key < 0 || key >= h->N) return fail(LVI_ERR_INVALID_ARG, "the GPS factor's key must lie inside the keys added");
    for (int k = 0; k < 3; k++) {
        if (!std::isfinite(xyz[k])) return fail(LVI_ERR_INVALID_ARG, "a GPS coordinate is not finite");
        if (!(variance[k] > 0.f) || !std::isfinite(variance[k])) return fail(LVI_ERR_INVALID_ARG, "variance must be positive and finite");
    }
    if ((int)h->g_key.size() >= h->Ncap) return fail(LVI_ERR_CAPACITY, "more GPS factors than max_poses");
    h->g_key.push_back(key);
    for (int k = 0; k < 3; k++) { h->g_z.push_back((double)xyz[k]); h->g_sw.push_back(1. / std::sqrt((double)variance[k])); }
    return LVI_OK;
}

int32_t lvi_pgo_gps_count(lvi_pgo* h, int32_t* n_gps)
{
    if (!h) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (n_gps) *n_gps = (int32_t)h->g_key.size();
    return LVI_OK;
}

int32_t lvi_pgo_gps_marginal_covariance(lvi_pgo* h, int32_t key, double cov[36])
{
    if (!h || !cov) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (h->N == 0) return fail(LVI_ERR_STATE, "no poses");
    if (key < 0 || key >= h->N) return fail(LVI_ERR_INVALID_ARG, "key outside the keys added");
    return guarded(h->device, [&]() -> int32_t {
        flush(h);
        Dev d = view(h, 6);
        d.ckey = key;
        hipStream_t s = h->stream;
        // step 0 is always active, and neither step[] nor a pose is written: the pass ends at the loop system
        hipLaunchKernelGGL(pgo_linearise, dim3(div_up(d.N + d.L + d.G, NB)), dim3(NB), 0, s, d, 0, 0);
        enqueue_linear_solve(d, schedule(d.N), 0, s);
        hipLaunchKernelGGL(pgo_cov, dim3(1), dim3(NB), 0, s, d);
        LVI_HIP(hipGetLastError());
        LVI_HIP(hipMemcpyAsync(h->h_cov, d.cov, sizeof(double) * 36, hipMemcpyDeviceToHost, s));
        LVI_HIP(hipStreamSynchronize(s));                            // the call's one wait
        std::memcpy(cov, h->h_cov, sizeof(double) * 36);
        return LVI_OK;
    });
}

}  // extern "C"
