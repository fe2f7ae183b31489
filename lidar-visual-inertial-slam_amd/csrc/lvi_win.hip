// The solve of vins_estimator's sliding window on the GPU (include/lvi_win.h; the contract is DESIGN §22): the problem of
// estimator.cpp:696-789 and a trust-region loop with a traditional dogleg step over a dense Schur system, as
// tests/win_ref.py states it.  All double.  With D columns of the reduced (camera-side) system, P1 = D + 1 and E eliminated
// scalar blocks, the camera side of every factor is a set of rows [J | r] over P1 columns; sc, sf are the Jacobi scales of
// the columns and of the eliminated blocks, dg the trust region's diagonal.  The projection factors, the prior's rows and
// Hcc = sum Jc'Jc, g = sum Jc'r come from the front end shared with the marginaliser (lvi_winsys.hip), with
// the per-factor costs on.  Beside and after it:
//
//   win_imu_info     one workgroup per IMU factor, once per solve: sqrt_info = LLT(covariance^-1).matrixL()'
//   win_eval_imu     one workgroup per IMU factor: residual and Jacobians, multiplied by sqrt_info, 15 rows of P1
//   win_feat         one workgroup per eliminated block: its factors in order, w = sum Jc' jf, h = sum jf^2, gf = sum jf r
//   win_grad         one workgroup: the cost, (first) the Jacobi scales, the diagonal, the gradient, its norms, the Cauchy alpha
//   win_schur        one workgroup per 16x16 tile: S = sc Hcc sc + mu dg^2 - sum_k ws_k ws_k' / (hs_k + mu dg_k^2) and its
//                    right-hand side, the eliminated blocks gathered in index order
//   win_chol         one workgroup: blocked Cholesky of S in place (global memory, the diagonal block in LDS), the two
//                    triangular solves; a pivot that is not positive raises the flag
//   win_step         one workgroup: back-substitution of the eliminated blocks, the dogleg step for the radius, the model
//                    cost change, the candidate state
//   win_cost         one workgroup: the candidate's cost from the per-factor costs
// The evaluation kernels run a second time on the candidate with their Jacobian stores off.  Sums are gathers in a fixed
// order and trees of a fixed shape: no floating-point atomics, two runs give the same bits, H is bitwise symmetric.  No
// workgroup waits for another; every loop has a bound; once a flag is up the later kernels of the sequence return at once.
#include <chrono>
#include <cmath>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "lvi_dev.hpp"
#include "lvi_imu_math.hpp"
#include "lvi_marg_view.hpp"
#include "lvi_winsys.hpp"

using namespace lvi;
using namespace lvi_marg_math;
using namespace lvi_winsys;
using namespace lvi_imu_math;

namespace {

constexpr int ONE = 1024;                // threads of the one-workgroup kernels
constexpr int NB = LVI_WIN_CHOL_BLOCK;
constexpr int MAXD = LVI_WIN_MAX_DIM;
constexpr int F_SYSTEM = 1, F_CHOL = 2, F_STEP = 4, F_COV = 8;

struct ImuDev { int blk[4]; int col[4]; ImuPre p; double cov[225]; };
struct BlkDev { int size, col, elim, pad; };
struct GradInfo { int flags, pad; double cost, grad_max, grad_norm, alpha, x_norm; };
struct StepInfo { int flags, kind; double gn_norm, cauchy_norm, dogleg_norm, model_cost_change, step_norm, cand_cost; };

struct Dev {
    double *x, *xc;
    const ProjDev* proj; const ImuDev* imu; const PriorBlk* pb; const BlkDev* blk;
    const int *feat_ptr, *feat_fac;
    double *Jf, *E, *fc, *part, *A, *W, *h, *Sinfo, *imu_work;
    double *sc, *sf, *dgc, *dgf, *grc, *grf, *S, *gnc, *gnf, *uf;
    const double *J0, *r0, *x0;
    GradInfo* gi; StepInfo* si;
    int P, I, n0, nkb0, nb, D, P1, Ne, Rd, Cp, C, loss_type, jacobi;
    double loss_a, G[3], min_diag, max_diag; ProjConst pc;
};

__device__ __forceinline__ double block_sum(double v, double* red)
{
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int o = ONE / 2; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    const double s = red[0];
    __syncthreads();
    return s;
}
__device__ __forceinline__ double block_max(double v, double* red)
{
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int o = ONE / 2; o > 0; o >>= 1) {
        if (t < o) red[t] = fmax(red[t], red[t + o]);
        __syncthreads();
    }
    const double s = red[0];
    __syncthreads();
    return s;
}

__global__ __launch_bounds__(64) void win_imu_info(Dev d)
{
    if (threadIdx.x != 0) return;
    const int i = blockIdx.x;
    if (!imu_sqrt_info(d.imu[i].cov, d.Sinfo + 225 * (size_t)i, d.imu_work + 675 * (size_t)i)) atomicOr(&d.gi->flags, F_SYSTEM | F_COV);
}

__global__ __launch_bounds__(64) void win_eval_imu(Dev d, int cand)
{
    __shared__ double r[IMU_ROWS], J[IMU_ROWS * IMU_COLS], rs[IMU_ROWS];
    const int i = blockIdx.x, t = threadIdx.x;
    const double* v = cand ? d.xc : d.x;
    const ImuDev& q = d.imu[i];
    if (t == 0)
        imu_eval_raw(v + (size_t)VAL * q.blk[0], v + (size_t)VAL * q.blk[1], v + (size_t)VAL * q.blk[2], v + (size_t)VAL * q.blk[3], q.p, d.G, r, cand ? nullptr : J);
    double* out = d.E + (size_t)IMU_ROWS * i * d.P1;
    if (!cand)
        for (int e = t; e < IMU_ROWS * d.P1; e += 64) out[e] = 0.;
    __syncthreads();
    const double* S = d.Sinfo + 225 * (size_t)i;
    if (t < IMU_ROWS) {
        rs[t] = imu_info_dot(S, t, r, 1, 0);
        if (!cand) out[(size_t)t * d.P1 + d.D] = rs[t];
    }
    if (!cand)
        for (int e = t; e < IMU_ROWS * IMU_COLS; e += 64) {
            const int row = e / IMU_COLS, c = e % IMU_COLS;
            const int b = c < C_SB_I ? 0 : c < C_POSE_J ? 1 : c < C_SB_J ? 2 : 3, start = b == 0 ? 0 : b == 1 ? C_SB_I : b == 2 ? C_POSE_J : C_SB_J;
            if (q.col[b] >= 0) out[(size_t)row * d.P1 + q.col[b] + c - start] = imu_info_dot(S, row, J, IMU_COLS, c);
        }
    __syncthreads();
    if (t == 0) {
        double s = 0.;
        for (int k = 0; k < IMU_ROWS; k++) s += rs[k] * rs[k];
        d.fc[d.P + i] = 0.5 * s;
    }
}

// the reduced column of local column c (0..19 but 18) of projection factor p, or -1
__device__ __forceinline__ int proj_gcol(const ProjDev& p, int c)
{
    const int b = c < 18 ? c / 6 : c == 18 ? 3 : 4, off = c < 18 ? c % 6 : 0;
    return p.col[b] < 0 ? -1 : p.col[b] + off;
}

__global__ __launch_bounds__(64) void win_feat(Dev d)
{
    __shared__ double acc[MAXD + 1];
    __shared__ double hh;
    const int k = blockIdx.x, t = threadIdx.x;
    for (int j = t; j < d.P1; j += 64) acc[j] = 0.;
    if (t == 0) hh = 0.;
    for (int e = d.feat_ptr[k]; e < d.feat_ptr[k + 1]; e++) {
        __syncthreads();
        const int f = d.feat_fac[e];
        const double* o = d.Jf + (size_t)JF * f;
        const double j0 = o[18], j1 = o[(PROJ_COLS + 1) + 18];
        if (t < PROJ_COLS && t != 18) {
            const int g = proj_gcol(d.proj[f], t);
            if (g >= 0) acc[g] += o[t] * j0 + o[(PROJ_COLS + 1) + t] * j1;
        } else if (t == PROJ_COLS) {
            acc[d.D] += o[PROJ_COLS] * j0 + o[(PROJ_COLS + 1) + PROJ_COLS] * j1;
        } else if (t == PROJ_COLS + 1) {
            hh += j0 * j0 + j1 * j1;
        }
    }
    __syncthreads();
    for (int j = t; j < d.P1; j += 64) d.W[(size_t)k * d.P1 + j] = acc[j];
    if (t == 0) d.h[k] = hh;
}

// u' H u over the whole system: uc [D] in LDS, uf [E] in global memory; H = [Hcc W'; W diag(h)]
__device__ __forceinline__ double quad_form(const Dev& d, const double* uc, const double* uf, double* red)
{
    const int t = threadIdx.x, D = d.D;
    double s = 0.;
    for (int e = t; e < D * D; e += ONE) {
        const int i = e / D, j = e % D;
        s += uc[i] * d.A[(size_t)i * d.P1 + j] * uc[j];
    }
    for (int k = t; k < d.Ne; k += ONE) {
        double dot = 0.;
        for (int i = 0; i < D; i++) dot += d.W[(size_t)k * d.P1 + i] * uc[i];
        s += 2. * uf[k] * dot + d.h[k] * uf[k] * uf[k];
    }
    return block_sum(s, red);
}

__device__ __forceinline__ double clampd(double v, double lo, double hi) { return fmin(fmax(v, lo), hi); }

__global__ __launch_bounds__(ONE) void win_grad(Dev d, int first)
{
    __shared__ double red[ONE], uc[MAXD];
    const int t = threadIdx.x, D = d.D, Ne = d.Ne, P1 = d.P1;
    double s = 0.;
    for (int k = t; k < d.P + d.I + d.n0; k += ONE) s += d.fc[k];
    const double cost = block_sum(s, red);
    __shared__ int stop;
    if (t == 0) {
        d.gi->cost = cost;
        if (!isfinite(cost)) atomicOr(&d.gi->flags, F_SYSTEM);
        stop = atomicOr(&d.gi->flags, 0) & F_SYSTEM;
    }
    __syncthreads();
    if (stop) return;
    if (first) {
        for (int i = t; i < D; i += ONE) d.sc[i] = d.jacobi ? 1. / (1. + std::sqrt(d.A[(size_t)i * P1 + i])) : 1.;
        for (int k = t; k < Ne; k += ONE) d.sf[k] = d.jacobi ? 1. / (1. + std::sqrt(d.h[k])) : 1.;
    }
    double gmax = 0., gn2 = 0., xn2 = 0.;
    for (int i = t; i < D; i += ONE) {
        const double sc = d.sc[i], g = d.A[(size_t)i * P1 + D];
        const double dg = std::sqrt(clampd(sc * d.A[(size_t)i * P1 + i] * sc, d.min_diag, d.max_diag)), gr = sc * g / dg;
        d.dgc[i] = dg; d.grc[i] = gr;
        uc[i] = gr / dg * sc;
        gmax = fmax(gmax, fabs(g)); gn2 += gr * gr;
    }
    for (int k = t; k < Ne; k += ONE) {
        const double sf = d.sf[k], g = d.W[(size_t)k * P1 + D];
        const double dg = std::sqrt(clampd(sf * d.h[k] * sf, d.min_diag, d.max_diag)), gr = sf * g / dg;
        d.dgf[k] = dg; d.grf[k] = gr;
        d.uf[k] = gr / dg * sf;
        gmax = fmax(gmax, fabs(g)); gn2 += gr * gr;
    }
    for (int b = t; b < d.nb; b += ONE) {
        const BlkDev k = d.blk[b];
        if (k.col < 0 && k.elim < 0) continue;
        for (int j = 0; j < k.size; j++) { const double v = d.x[(size_t)VAL * b + j]; xn2 += v * v; }
    }
    __syncthreads();
    gmax = block_max(gmax, red);
    gn2 = block_sum(gn2, red);
    xn2 = block_sum(xn2, red);
    const double q = quad_form(d, uc, d.uf, red);
    if (t == 0) {
        d.gi->grad_max = gmax; d.gi->grad_norm = std::sqrt(gn2); d.gi->alpha = gn2 / q; d.gi->x_norm = std::sqrt(xn2);
        if (!isfinite(gn2) || !isfinite(q)) atomicOr(&d.gi->flags, F_SYSTEM);
    }
}

// the scaled coupling of eliminated block k at column j of the augmented reduced system (j == D: its gradient)
__device__ __forceinline__ double ws_value(const Dev& d, int k, int j)
{
    if (k >= d.Ne || j > d.D) return 0.;
    return d.sf[k] * d.W[(size_t)k * d.P1 + j] * (j < d.D ? d.sc[j] : 1.);
}

__global__ __launch_bounds__(TILE * TILE) void win_schur(Dev d, double mu)
{
    __shared__ double xs[SUB][TILE], ys[SUB][TILE], inv[SUB];
    if (d.gi->flags & F_SYSTEM) return;
    const int tx = threadIdx.x, ty = threadIdx.y, t = ty * TILE + tx;
    const int gx0 = blockIdx.x * TILE, gy0 = blockIdx.y * TILE, i = gy0 + ty, j = gx0 + tx, D = d.D;
    double acc = 0.;
    if (i < D && j <= D) {
        acc = d.sc[i] * d.A[(size_t)i * d.P1 + j] * (j < D ? d.sc[j] : 1.);
        if (i == j) acc += mu * (d.dgc[i] * d.dgc[i]);
    }
    for (int k0 = 0; k0 < d.Ne; k0 += SUB) {
        for (int e = t; e < SUB * TILE; e += TILE * TILE) {
            const int rr = e / TILE, k = e % TILE;
            xs[rr][k] = ws_value(d, k0 + rr, gx0 + k);
            ys[rr][k] = ws_value(d, k0 + rr, gy0 + k);
        }
        if (t < SUB) {
            const int k = k0 + t;
            inv[t] = k < d.Ne ? 1. / (d.sf[k] * d.h[k] * d.sf[k] + mu * (d.dgf[k] * d.dgf[k])) : 0.;
        }
        __syncthreads();
        for (int rr = 0; rr < SUB; rr++) acc -= (ys[rr][ty] * xs[rr][tx]) * inv[rr];
        __syncthreads();
    }
    if (i < D && j <= D) d.S[(size_t)i * d.P1 + j] = acc;
}

// Blocked right-looking Cholesky of the D x D matrix S (leading dimension P1, lower triangle) in place, then L z = b and
// L' y = z with b the column D of S; gnc = -y.  One workgroup; the matrix stays in global memory (at D = 256 it is 514 KB,
// three times the LDS of a CU), only the NB x NB diagonal block is held in LDS while it is factored.
__global__ __launch_bounds__(ONE) void win_chol(Dev d)
{
    __shared__ double Ls[NB][NB + 1], yv[MAXD];
    __shared__ int bad;
    if (d.gi->flags & F_SYSTEM) return;
    const int t = threadIdx.x, D = d.D, ld = d.P1;
    double* S = d.S;
    if (t == 0) bad = 0;
    __syncthreads();
    for (int kb = 0; kb < D; kb += NB) {
        const int nb = min(NB, D - kb);
        for (int e = t; e < nb * nb; e += ONE) Ls[e / nb][e % nb] = S[(size_t)(kb + e / nb) * ld + kb + e % nb];
        __syncthreads();
        for (int j = 0; j < nb; j++) {
            if (t == 0) {
                const double p = Ls[j][j];
                if (!(p > 0.)) bad = 1; else Ls[j][j] = std::sqrt(p);
            }
            __syncthreads();
            if (bad) break;
            if (t > j && t < nb) Ls[t][j] /= Ls[j][j];
            __syncthreads();
            if (t < nb * nb) {
                const int i = t / nb, c = t % nb;
                if (c > j && i >= c) Ls[i][c] -= Ls[i][j] * Ls[c][j];
            }
            __syncthreads();
        }
        if (bad) break;
        for (int e = t; e < nb * nb; e += ONE)
            if (e % nb <= e / nb) S[(size_t)(kb + e / nb) * ld + kb + e % nb] = Ls[e / nb][e % nb];
        const int m = D - kb - nb;
        if (t < m) {
            double* row = S + (size_t)(kb + nb + t) * ld + kb;
            for (int c = 0; c < nb; c++) {
                double v = row[c];
                for (int p = 0; p < c; p++) v -= row[p] * Ls[c][p];
                row[c] = v / Ls[c][c];
            }
        }
        __syncthreads();
        for (int e = t; e < m * m; e += ONE) {
            const int i = e / m, j = e % m;
            if (j > i) continue;
            const double *ri = S + (size_t)(kb + nb + i) * ld + kb, *rj = S + (size_t)(kb + nb + j) * ld + kb;
            double s = 0.;
            for (int c = 0; c < nb; c++) s += ri[c] * rj[c];
            S[(size_t)(kb + nb + i) * ld + kb + nb + j] -= s;
        }
        __syncthreads();
    }
    if (bad) {
        if (t == 0) atomicOr(&d.si->flags, F_CHOL);
        return;
    }
    for (int i = t; i < D; i += ONE) yv[i] = S[(size_t)i * ld + D];
    __syncthreads();
    for (int j = 0; j < D; j++) {
        if (t == 0) yv[j] /= S[(size_t)j * ld + j];
        __syncthreads();
        if (t > j && t < D) yv[t] -= S[(size_t)t * ld + j] * yv[j];
        __syncthreads();
    }
    for (int j = D - 1; j >= 0; j--) {
        if (t == 0) yv[j] /= S[(size_t)j * ld + j];
        __syncthreads();
        if (t < j) yv[t] -= S[(size_t)j * ld + t] * yv[j];
        __syncthreads();
    }
    int nf = 0;
    for (int i = t; i < D; i += ONE) { d.gnc[i] = -yv[i]; if (!isfinite(yv[i])) nf = 1; }
    if (nf) atomicOr(&d.si->flags, F_CHOL);
}

__global__ __launch_bounds__(ONE) void win_step(Dev d, double radius, double mu)
{
    __shared__ double red[ONE], uc[MAXD];
    if ((d.gi->flags & F_SYSTEM) || (d.si->flags & F_CHOL)) return;
    const int t = threadIdx.x, D = d.D, Ne = d.Ne, P1 = d.P1;
    const double alpha = d.gi->alpha, grad_norm = d.gi->grad_norm;
    // the eliminated blocks of the Gauss-Newton step, and |dg y|, gradient . (dg y)
    double n2 = 0., dot = 0.;
    for (int k = t; k < Ne; k += ONE) {
        const double sf = d.sf[k];
        double s = 0.;
        for (int i = 0; i < D; i++) s += sf * d.W[(size_t)k * P1 + i] * d.sc[i] * d.gnc[i];
        const double y = (-(sf * d.W[(size_t)k * P1 + D]) - s) / (sf * d.h[k] * sf + mu * (d.dgf[k] * d.dgf[k]));
        d.gnf[k] = y;
        const double dy = d.dgf[k] * y;
        n2 += dy * dy; dot += d.grf[k] * dy;
    }
    for (int i = t; i < D; i += ONE) {
        const double dy = d.dgc[i] * d.gnc[i];
        n2 += dy * dy; dot += d.grc[i] * dy;
    }
    n2 = block_sum(n2, red);
    dot = block_sum(dot, red);
    const double gn_norm = std::sqrt(n2), cauchy_norm = grad_norm * alpha;
    int kind;
    double ca = 0., cb = 0., dogleg_norm = radius;          // step = (ca gradient + cb dg y) / dg
    if (gn_norm <= radius) {
        kind = LVI_WIN_STEP_GAUSS_NEWTON; dogleg_norm = gn_norm;
    } else if (cauchy_norm >= radius) {
        kind = LVI_WIN_STEP_CAUCHY; ca = -(radius / grad_norm);
    } else {
        kind = LVI_WIN_STEP_INTERPOLATED;
        const double b_dot_a = -alpha * dot, a2 = cauchy_norm * cauchy_norm, bma2 = a2 - 2. * b_dot_a + n2;
        const double c = b_dot_a - a2, dd = std::sqrt(c * c + bma2 * (radius * radius - a2));
        const double beta = (c <= 0.) ? (dd - c) / bma2 : (radius * radius - a2) / (dd + c);
        ca = -alpha * (1. - beta); cb = beta;
    }
    double sn2 = 0., gd = 0.;
    for (int i = t; i < D; i += ONE) {
        const double st = kind == LVI_WIN_STEP_GAUSS_NEWTON ? d.gnc[i] : (ca * d.grc[i] + cb * (d.dgc[i] * d.gnc[i])) / d.dgc[i];
        const double de = st * d.sc[i];
        uc[i] = de;
        sn2 += de * de; gd += de * d.A[(size_t)i * P1 + D];
    }
    for (int k = t; k < Ne; k += ONE) {
        const double st = kind == LVI_WIN_STEP_GAUSS_NEWTON ? d.gnf[k] : (ca * d.grf[k] + cb * (d.dgf[k] * d.gnf[k])) / d.dgf[k];
        const double de = st * d.sf[k];
        d.uf[k] = de;
        sn2 += de * de; gd += de * d.W[(size_t)k * P1 + D];
    }
    __syncthreads();
    sn2 = block_sum(sn2, red);
    gd = block_sum(gd, red);
    const double q = quad_form(d, uc, d.uf, red);
    for (int b = t; b < d.nb; b += ONE) {
        const BlkDev k = d.blk[b];
        const double* x = d.x + (size_t)VAL * b;
        double* o = d.xc + (size_t)VAL * b;
        if (k.col >= 0 && k.size == 7) {
            pose_plus(x, uc + k.col, o);
        } else {
            for (int j = 0; j < k.size; j++) o[j] = x[j] + (k.col >= 0 ? uc[k.col + j] : k.elim >= 0 ? d.uf[k.elim] : 0.);
        }
    }
    if (t == 0) {
        StepInfo& s = *d.si;
        s.kind = kind; s.gn_norm = gn_norm; s.cauchy_norm = cauchy_norm; s.dogleg_norm = dogleg_norm;
        s.model_cost_change = -(gd + 0.5 * q); s.step_norm = std::sqrt(sn2);
        if (!isfinite(s.model_cost_change) || !isfinite(sn2)) atomicOr(&s.flags, F_STEP);
    }
}

__global__ __launch_bounds__(ONE) void win_cost(Dev d)
{
    __shared__ double red[ONE];
    if ((d.gi->flags & F_SYSTEM) || (d.si->flags & F_CHOL)) return;
    double s = 0.;
    for (int k = threadIdx.x; k < d.P + d.I + d.n0; k += ONE) s += d.fc[k];
    s = block_sum(s, red);
    if (threadIdx.x == 0) d.si->cand_cost = s;
}

struct Block { int id, size, flags; double v[VAL]; };
struct HostPrior {
    bool valid = false, resident = false;
    int n = 0;
    std::vector<int> ids, sizes, col;
    std::vector<double> J, r, x0;            // the host route
    const double *dJ = nullptr, *dr = nullptr, *dx0 = nullptr;       // the resident route
};

}  // namespace

struct lvi_win : Handle {
    lvi_win_caps caps{};
    lvi_win_params P{};
    Dev d{};
    ProjDev* d_proj = nullptr; ImuDev* d_imu = nullptr; PriorBlk* d_pb = nullptr; BlkDev* d_blk = nullptr; int *d_fptr = nullptr, *d_ffac = nullptr;
    double *d_pJ = nullptr, *d_pr = nullptr, *d_px0 = nullptr;
    // pinned staging
    double* h_x = nullptr; ProjDev* h_proj = nullptr; ImuDev* h_imu = nullptr; PriorBlk* h_pb = nullptr; BlkDev* h_blk = nullptr; int *h_fptr = nullptr, *h_ffac = nullptr;
    GradInfo* h_gi = nullptr; StepInfo* h_si = nullptr;
    // the description
    std::vector<Block> blocks; std::unordered_map<int, int> index;
    std::vector<lvi_marg_projection> proj;
    std::vector<lvi_win_imu> imu;
    HostPrior prior;
    std::vector<lvi_win_iteration> log;
    int D = 0, Ne = 0;
};

namespace {

int P1max(const lvi_win* h) { return h->caps.max_dim + 1; }
int dense_rows_max(const lvi_win* h) { return IMU_ROWS * h->caps.max_imu + h->caps.max_prior_rows; }
int max_chunks(const lvi_win* h) { return div_up(h->caps.max_projections, SHARE) + div_up(dense_rows_max(h), CH_ROWS) + 1; }

template <class A, class B> void carve(A& a, B& pin, lvi_win* h)
{
    const lvi_win_caps& c = h->caps;
    const size_t Pm = (size_t)P1max(h), nb = (size_t)c.max_blocks, np = (size_t)c.max_projections, ne = std::max(1, c.max_eliminated), ni = std::max(1, c.max_imu),
                 n0 = std::max(1, c.max_prior_rows), R = std::max(1, dense_rows_max(h));
    Dev& d = h->d;
    alloc_pair(a, pin, d.x, h->h_x, VAL * nb); d.xc = a.template alloc<double>(VAL * nb);
    alloc_pair(a, pin, h->d_proj, h->h_proj, np); alloc_pair(a, pin, h->d_imu, h->h_imu, ni); alloc_pair(a, pin, h->d_pb, h->h_pb, n0);
    alloc_pair(a, pin, h->d_blk, h->h_blk, nb); alloc_pair(a, pin, h->d_fptr, h->h_fptr, ne + 1); alloc_pair(a, pin, h->d_ffac, h->h_ffac, np);
    d.Jf = a.template alloc<double>(JF * np); d.E = a.template alloc<double>(R * Pm); d.fc = a.template alloc<double>(np + ni + n0);
    d.part = a.template alloc<double>((size_t)max_chunks(h) * Pm * Pm); d.A = a.template alloc<double>(Pm * Pm);
    d.W = a.template alloc<double>(ne * Pm); d.h = a.template alloc<double>(ne);
    d.Sinfo = a.template alloc<double>(225 * ni); d.imu_work = a.template alloc<double>(675 * ni);
    d.sc = a.template alloc<double>(Pm); d.dgc = a.template alloc<double>(Pm); d.grc = a.template alloc<double>(Pm); d.gnc = a.template alloc<double>(Pm);
    d.sf = a.template alloc<double>(ne); d.dgf = a.template alloc<double>(ne); d.grf = a.template alloc<double>(ne); d.gnf = a.template alloc<double>(ne);
    d.uf = a.template alloc<double>(ne);
    d.S = a.template alloc<double>(Pm * Pm);
    h->d_pJ = a.template alloc<double>(n0 * n0); h->d_pr = a.template alloc<double>(n0); h->d_px0 = a.template alloc<double>(VAL * n0);
    alloc_pair(a, pin, d.gi, h->h_gi, 1); alloc_pair(a, pin, d.si, h->h_si, 1);
}

bool params_ok(const lvi_win_params& p)
{
    const double pos[] = {p.loss_a, p.sqrt_info, p.initial_radius, p.max_radius, p.initial_mu, p.min_mu, p.max_mu, p.min_diagonal, p.max_diagonal};
    for (double v : pos) if (!(v > 0.) || !std::isfinite(v)) return false;
    const double nonneg[] = {p.max_time_s, p.min_radius, p.min_relative_decrease, p.function_tolerance, p.gradient_tolerance, p.parameter_tolerance,
                             p.increase_threshold, p.decrease_threshold};
    for (double v : nonneg) if (!(v >= 0.) || !std::isfinite(v)) return false;
    return p.loss_type >= LVI_MARG_LOSS_NONE && p.loss_type <= LVI_MARG_LOSS_HUBER && p.max_iterations >= 0 && p.max_iterations <= LVI_WIN_MAX_ITERATIONS &&
           p.max_invalid_steps >= 1 && p.mu_increase_factor > 1. && std::isfinite(p.mu_increase_factor) && std::isfinite(p.tr_over_row) && std::isfinite(p.half_row) &&
           finite_all(p.G, 3) && p.min_diagonal <= p.max_diagonal;
}

int find(const lvi_win* h, int id)
{
    const auto it = h->index.find(id);
    return it == h->index.end() ? -1 : it->second;
}

// the prior's blocks against the declared ones
int32_t check_prior_blocks(const lvi_win* h, int count, const int* ids, const int* sizes)
{
    for (int k = 0; k < count; k++) {
        const int b = find(h, ids[k]);
        if (b < 0) return fail(LVI_ERR_INVALID_ARG, "a kept block of the prior was not declared");
        if (h->blocks[b].size != sizes[k]) return fail(LVI_ERR_INVALID_ARG, "a kept block of the prior was declared with another size");
        if (h->blocks[b].flags & LVI_WIN_ELIMINATED) return fail(LVI_ERR_INVALID_ARG, "a kept block of the prior is flagged LVI_WIN_ELIMINATED");
        for (int j = 0; j < k; j++) if (ids[j] == ids[k]) return fail(LVI_ERR_INVALID_ARG, "two kept blocks of the prior under one id");
    }
    return LVI_OK;
}

// lay the system out, stage and upload the description; the blocks' host values go to d.x
int32_t upload(lvi_win* h, Dev& d)
{
    const int nb = (int)h->blocks.size(), P = (int)h->proj.size(), I = (int)h->imu.size();
    std::vector<int> col(nb, -1), elim(nb, -1);
    int D = 0, Ne = 0;
    for (int b = 0; b < nb; b++) {
        const Block& k = h->blocks[b];
        if (k.flags & LVI_WIN_CONSTANT) continue;
        if (k.flags & LVI_WIN_ELIMINATED) elim[b] = Ne++;
        else { col[b] = D; D += local_size(k.size); }
    }
    if (D < 1) return fail(LVI_ERR_STATE, "no free block outside the eliminated ones");
    if (D > h->caps.max_dim) return fail(LVI_ERR_CAPACITY, "the reduced system is larger than max_dim");
    const HostPrior& pr = h->prior;
    if (pr.valid) {
        const int32_t st = check_prior_blocks(h, (int)pr.ids.size(), pr.ids.data(), pr.sizes.data());
        if (st != LVI_OK) return st;
    }
    hipStream_t s = h->stream;
    for (int b = 0; b < nb; b++) {
        std::memcpy(h->h_x + (size_t)VAL * b, h->blocks[b].v, sizeof(double) * VAL);
        h->h_blk[b] = BlkDev{h->blocks[b].size, col[b], elim[b], 0};
    }
    std::vector<std::vector<int>> of(Ne);
    const auto fnd = [&](int id) { return find(h, id); };
    for (int f = 0; f < P; f++) {
        stage_projection(h->proj[f], fnd, col.data(), h->h_proj[f]);
        const int e = elim[h->h_proj[f].blk[3]];
        if (e >= 0) of[e].push_back(f);
    }
    int at = 0;
    for (int k = 0; k < Ne; k++) {
        h->h_fptr[k] = at;
        for (int f : of[k]) h->h_ffac[at++] = f;
    }
    h->h_fptr[Ne] = at;
    for (int i = 0; i < I; i++) {
        const lvi_win_imu& r = h->imu[i];
        ImuDev& q = h->h_imu[i];
        const int ids[4] = {r.pose_i, r.speed_bias_i, r.pose_j, r.speed_bias_j};
        for (int k = 0; k < 4; k++) { q.blk[k] = find(h, ids[k]); q.col[k] = col[q.blk[k]]; }
        q.p.sum_dt = r.sum_dt;
        std::memcpy(q.p.delta_p, r.delta_p, sizeof(double) * 3); std::memcpy(q.p.delta_q, r.delta_q, sizeof(double) * 4);
        std::memcpy(q.p.delta_v, r.delta_v, sizeof(double) * 3); std::memcpy(q.p.linearized_ba, r.linearized_ba, sizeof(double) * 3);
        std::memcpy(q.p.linearized_bg, r.linearized_bg, sizeof(double) * 3); std::memcpy(q.p.jacobian, r.jacobian, sizeof(double) * 225);
        std::memcpy(q.cov, r.covariance, sizeof(double) * 225);
    }
    const int n0 = pr.valid ? pr.n : 0, nkb0 = pr.valid ? (int)pr.ids.size() : 0;
    stage_prior_blocks(nkb0, pr.ids.data(), pr.sizes.data(), pr.col.data(), fnd, col.data(), h->h_pb);
    d = h->d;
    d.proj = h->d_proj; d.imu = h->d_imu; d.pb = h->d_pb; d.blk = h->d_blk; d.feat_ptr = h->d_fptr; d.feat_fac = h->d_ffac;
    d.P = P; d.I = I; d.n0 = n0; d.nkb0 = nkb0; d.nb = nb; d.D = D; d.P1 = D + 1; d.Ne = Ne; d.Rd = IMU_ROWS * I + n0;
    d.Cp = div_up(P, SHARE); d.C = d.Cp + div_up(d.Rd, CH_ROWS);
    d.loss_type = h->P.loss_type; d.jacobi = h->P.jacobi_scaling; d.loss_a = h->P.loss_a;
    for (int k = 0; k < 3; k++) d.G[k] = h->P.G[k];
    d.min_diag = h->P.min_diagonal; d.max_diag = h->P.max_diagonal;
    d.pc = ProjConst{h->P.sqrt_info, h->P.tr_over_row, h->P.half_row};
    LVI_HIP(hipMemcpyAsync(d.x, h->h_x, sizeof(double) * VAL * nb, hipMemcpyHostToDevice, s));
    LVI_HIP(hipMemcpyAsync(h->d_blk, h->h_blk, sizeof(BlkDev) * nb, hipMemcpyHostToDevice, s));
    if (P > 0) LVI_HIP(hipMemcpyAsync(h->d_proj, h->h_proj, sizeof(ProjDev) * P, hipMemcpyHostToDevice, s));
    if (P > 0) LVI_HIP(hipMemcpyAsync(h->d_ffac, h->h_ffac, sizeof(int) * P, hipMemcpyHostToDevice, s));
    LVI_HIP(hipMemcpyAsync(h->d_fptr, h->h_fptr, sizeof(int) * (Ne + 1), hipMemcpyHostToDevice, s));
    if (I > 0) LVI_HIP(hipMemcpyAsync(h->d_imu, h->h_imu, sizeof(ImuDev) * I, hipMemcpyHostToDevice, s));
    if (nkb0 > 0) LVI_HIP(hipMemcpyAsync(h->d_pb, h->h_pb, sizeof(PriorBlk) * nkb0, hipMemcpyHostToDevice, s));
    if (pr.valid && pr.resident) {
        d.J0 = pr.dJ; d.r0 = pr.dr; d.x0 = pr.dx0;
    } else if (pr.valid) {
        LVI_HIP(hipMemcpyAsync(h->d_pJ, pr.J.data(), sizeof(double) * (size_t)n0 * n0, hipMemcpyHostToDevice, s));
        LVI_HIP(hipMemcpyAsync(h->d_pr, pr.r.data(), sizeof(double) * n0, hipMemcpyHostToDevice, s));
        LVI_HIP(hipMemcpyAsync(h->d_px0, pr.x0.data(), sizeof(double) * VAL * nkb0, hipMemcpyHostToDevice, s));
        LVI_HIP(hipStreamSynchronize(s));                    // the pageable sources above are read before this returns
        d.J0 = h->d_pJ; d.r0 = h->d_pr; d.x0 = h->d_px0;
    }
    LVI_HIP(hipMemsetAsync(d.gi, 0, sizeof(GradInfo), s));
    if (I > 0) hipLaunchKernelGGL(win_imu_info, dim3(I), dim3(64), 0, s, d);
    LVI_HIP(hipGetLastError());
    h->D = D; h->Ne = Ne;
    return LVI_OK;
}

// what the shared front end reads of d at the blocks' values vals: the costs in fc, flag bit F_SYSTEM, no corner
SysView sys_view(const Dev& d, const double* vals)
{
    return SysView{vals, d.proj, d.Jf, d.E, d.part, d.A, d.J0, d.r0, d.x0, d.pb, d.fc, &d.gi->flags, F_SYSTEM, nullptr,
                   d.P, IMU_ROWS * d.I, d.Rd, d.n0, d.nkb0, d.P1, d.Cp, d.C, d.P + d.I, d.loss_type, d.loss_a, d.pc};
}

// every factor at d.x, or at the candidate d.xc for the costs alone
void launch_eval(const Dev& d, hipStream_t s, int cand)
{
    const SysView v = sys_view(d, cand ? d.xc : d.x);
    launch_eval_proj(v, s, !cand);
    if (d.I > 0) hipLaunchKernelGGL(win_eval_imu, dim3(d.I), dim3(64), 0, s, d, cand);
    launch_prior_rows(v, s, !cand);
}

// factors, system, gradient at d.x -> *h->h_gi
void prepare(lvi_win* h, const Dev& d, int first)
{
    hipStream_t s = h->stream;
    launch_eval(d, s, 0);
    if (d.Ne > 0) hipLaunchKernelGGL(win_feat, dim3(d.Ne), dim3(64), 0, s, d);
    launch_build(sys_view(d, d.x), s);
    hipLaunchKernelGGL(win_grad, dim3(1), dim3(ONE), 0, s, d, first);
    LVI_HIP(hipGetLastError());
    LVI_HIP(hipMemcpyAsync(h->h_gi, d.gi, sizeof(GradInfo), hipMemcpyDeviceToHost, s));
    LVI_HIP(hipStreamSynchronize(s));
}

// one step at d.x for (radius, mu) and its candidate's cost -> *h->h_si; reuse: the Gauss-Newton step of the last attempt
void attempt(lvi_win* h, const Dev& d, double radius, double mu, bool reuse)
{
    hipStream_t s = h->stream;
    LVI_HIP(hipMemsetAsync(d.si, 0, sizeof(StepInfo), s));
    if (!reuse) {
        const int Tn = div_up(d.P1, TILE);
        hipLaunchKernelGGL(win_schur, dim3(Tn, Tn), dim3(TILE, TILE), 0, s, d, mu);
        hipLaunchKernelGGL(win_chol, dim3(1), dim3(ONE), 0, s, d);
    }
    hipLaunchKernelGGL(win_step, dim3(1), dim3(ONE), 0, s, d, radius, mu);
    launch_eval(d, s, 1);
    hipLaunchKernelGGL(win_cost, dim3(1), dim3(ONE), 0, s, d);
    LVI_HIP(hipGetLastError());
    LVI_HIP(hipMemcpyAsync(h->h_si, d.si, sizeof(StepInfo), hipMemcpyDeviceToHost, s));
    LVI_HIP(hipStreamSynchronize(s));                        // the iteration's one wait
}

}  // namespace

extern "C" {

int32_t lvi_win_abi_version(void) { return LVI_WIN_ABI_VERSION; }

void lvi_win_params_default(lvi_win_params* p)
{
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->loss_type = LVI_MARG_LOSS_CAUCHY; p->max_iterations = 8; p->jacobi_scaling = 1; p->max_invalid_steps = 5;
    p->loss_a = 1.0; p->sqrt_info = 460.0 / 1.5; p->tr_over_row = 0.; p->half_row = 240.;
    p->G[0] = 0.; p->G[1] = 0.; p->G[2] = 9.8;
    p->max_time_s = 0.; p->initial_radius = 1e4; p->max_radius = 1e16; p->min_radius = 1e-32; p->min_relative_decrease = 1e-3;
    p->function_tolerance = 1e-6; p->gradient_tolerance = 1e-10; p->parameter_tolerance = 1e-8;
    p->initial_mu = 1e-8; p->min_mu = 1e-8; p->max_mu = 1.0; p->mu_increase_factor = 10.;
    p->increase_threshold = 0.75; p->decrease_threshold = 0.25; p->min_diagonal = 1e-6; p->max_diagonal = 1e32;
}

int32_t lvi_win_create(int32_t device, const lvi_win_caps* caps, lvi_win** out)
{
    if (!out || !caps) return fail(LVI_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    const lvi_win_caps& c = *caps;
    if (c.max_blocks < 1 || c.max_blocks > LVI_WIN_MAX_BLOCKS || c.max_projections < 1 || c.max_projections > LVI_WIN_MAX_PROJECTIONS ||
        c.max_eliminated < 0 || c.max_eliminated > LVI_WIN_MAX_ELIMINATED || c.max_imu < 0 || c.max_imu > LVI_WIN_MAX_IMU ||
        c.max_prior_rows < 0 || c.max_prior_rows > LVI_WIN_MAX_PRIOR_ROWS || c.max_dim < 1 || c.max_dim > LVI_WIN_MAX_DIM)
        return fail(LVI_ERR_INVALID_ARG, "a capacity is outside its range 0 or 1..LVI_WIN_MAX_*");
    return create_handle(device, out, lvi_win_destroy,
        [&](lvi_win* h) { h->caps = c; lvi_win_params_default(&h->P); },
        [&](lvi_win* h) -> int32_t { h->open(device, [&](auto& dev, auto& pin) { carve(dev, pin, h); }); return LVI_OK; });
}

void lvi_win_destroy(lvi_win* h)
{
    if (!h) return;
    h->close();
    delete h;
}

int32_t lvi_win_set_params(lvi_win* h, const lvi_win_params* p)
{
    if (!h || !p) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (!params_ok(*p)) return fail(LVI_ERR_INVALID_ARG, "a parameter is outside its range (max_iterations 0..LVI_WIN_MAX_ITERATIONS, scales and radii > 0, tolerances >= 0)");
    h->P = *p;
    return LVI_OK;
}

int32_t lvi_win_begin(lvi_win* h)
{
    if (!h) return fail(LVI_ERR_INVALID_ARG, "null argument");
    h->blocks.clear(); h->index.clear(); h->proj.clear(); h->imu.clear(); h->prior = HostPrior(); h->log.clear(); h->D = 0; h->Ne = 0;
    return LVI_OK;
}

int32_t lvi_win_set_block(lvi_win* h, int32_t id, int32_t size, const double* values, int32_t flags)
{
    if (!h || !values) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (size < 1 || size > LVI_WIN_MAX_BLOCK_SIZE) return fail(LVI_ERR_INVALID_ARG, "block size must be 1..LVI_WIN_MAX_BLOCK_SIZE");
    if (flags & ~(LVI_WIN_CONSTANT | LVI_WIN_ELIMINATED)) return fail(LVI_ERR_INVALID_ARG, "unknown flag");
    if (flags == (LVI_WIN_CONSTANT | LVI_WIN_ELIMINATED)) return fail(LVI_ERR_INVALID_ARG, "a constant block is not eliminated");
    if ((flags & LVI_WIN_ELIMINATED) && size != 1) return fail(LVI_ERR_INVALID_ARG, "only a block of size 1 can be eliminated");
    if (!finite_all(values, (size_t)size)) return fail(LVI_ERR_INVALID_ARG, "a block value is not finite");
    int b = find(h, id);
    if (b >= 0 && (h->blocks[b].size != size || h->blocks[b].flags != flags)) return fail(LVI_ERR_INVALID_ARG, "the id was declared with another size or other flags");
    if (b < 0) {
        if ((int)h->blocks.size() >= h->caps.max_blocks) return fail(LVI_ERR_CAPACITY, "more parameter blocks than max_blocks");
        if (flags & LVI_WIN_ELIMINATED) {
            int ne = 0;
            for (const Block& k : h->blocks) ne += (k.flags & LVI_WIN_ELIMINATED) ? 1 : 0;
            if (ne >= h->caps.max_eliminated) return fail(LVI_ERR_CAPACITY, "more eliminated blocks than max_eliminated");
        }
        Block k{};
        k.id = id; k.size = size; k.flags = flags;
        b = (int)h->blocks.size();
        h->blocks.push_back(k);
        h->index[id] = b;
    }
    for (int k = 0; k < VAL; k++) h->blocks[b].v[k] = k < size ? values[k] : 0.;
    return LVI_OK;
}

int32_t lvi_win_add_projection(lvi_win* h, int32_t count, const lvi_marg_projection* recs)
{
    if (!h || (count > 0 && !recs)) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (count < 0) return fail(LVI_ERR_INVALID_ARG, "negative count");
    if ((size_t)count + h->proj.size() > (size_t)h->caps.max_projections) return fail(LVI_ERR_CAPACITY, "more projection factors than max_projections");
    const auto look = [&](int id) {
        const int b = find(h, id);
        return b < 0 ? BlockRef{-1, 0, false} : BlockRef{b, h->blocks[b].size, (h->blocks[b].flags & LVI_WIN_ELIMINATED) != 0};
    };
    for (int f = 0; f < count; f++) {
        const char* why = nullptr;
        const int32_t st = check_projection(recs[f], look, true, &why);
        if (st != LVI_OK) return fail(st, why);
    }
    h->proj.insert(h->proj.end(), recs, recs + count);
    return LVI_OK;
}

int32_t lvi_win_add_imu(lvi_win* h, int32_t count, const lvi_win_imu* recs)
{
    if (!h || (count > 0 && !recs)) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (count < 0) return fail(LVI_ERR_INVALID_ARG, "negative count");
    if ((size_t)count + h->imu.size() > (size_t)h->caps.max_imu) return fail(LVI_ERR_CAPACITY, "more IMU factors than max_imu");
    static const int want[4] = {7, 9, 7, 9};
    for (int f = 0; f < count; f++) {
        const lvi_win_imu& r = recs[f];
        const int ids[4] = {r.pose_i, r.speed_bias_i, r.pose_j, r.speed_bias_j};
        int b[4];
        for (int k = 0; k < 4; k++) {
            b[k] = find(h, ids[k]);
            if (b[k] < 0) return fail(LVI_ERR_INVALID_ARG, "an IMU factor names an id that was not declared");
            if (h->blocks[b[k]].size != want[k]) return fail(LVI_ERR_INVALID_ARG, "an IMU factor's blocks must have sizes 7, 9, 7, 9");
            for (int j = 0; j < k; j++) if (b[j] == b[k]) return fail(LVI_ERR_INVALID_ARG, "an IMU factor names one block twice");
        }
        if (!finite_all(&r.sum_dt, 1 + 3 + 4 + 3 + 3 + 3 + 225 + 225)) return fail(LVI_ERR_INVALID_ARG, "an IMU record is not finite");
    }
    h->imu.insert(h->imu.end(), recs, recs + count);
    return LVI_OK;
}

int32_t lvi_win_set_prior_from_marg(lvi_win* h, lvi_marg* m)
{
    if (!h || !m) return fail(LVI_ERR_INVALID_ARG, "null argument");
    MargPriorView v{};
    if (!marg_prior_view(m, &v)) return fail(LVI_ERR_STATE, "the marginaliser has no result");
    if (v.device != h->device) return fail(LVI_ERR_INVALID_ARG, "the marginaliser is on another device");
    if (v.n > h->caps.max_prior_rows) return fail(LVI_ERR_CAPACITY, "the prior has more rows than max_prior_rows");
    const int32_t st = check_prior_blocks(h, v.count, v.ids, v.sizes);
    if (st != LVI_OK) return st;
    HostPrior p;
    p.valid = true; p.resident = true; p.n = v.n;
    p.ids.assign(v.ids, v.ids + v.count); p.sizes.assign(v.sizes, v.sizes + v.count); p.col.assign(v.col, v.col + v.count);
    p.dJ = v.J; p.dr = v.r; p.dx0 = v.x0;
    h->prior = std::move(p);
    return LVI_OK;
}

int32_t lvi_win_set_prior(lvi_win* h, int32_t n, const double* J, const double* r, int32_t count, const int32_t* ids, const int32_t* sizes, const int32_t* idx,
                          const double* values)
{
    if (!h || !J || !r || !ids || !sizes || !idx || !values) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (n < 1 || count < 1) return fail(LVI_ERR_INVALID_ARG, "an empty prior");
    if (n > h->caps.max_prior_rows) return fail(LVI_ERR_CAPACITY, "the prior has more rows than max_prior_rows");
    const int32_t st = check_prior_blocks(h, count, ids, sizes);
    if (st != LVI_OK) return st;
    int lo = idx[0], total = 0;
    for (int k = 0; k < count; k++) { lo = std::min(lo, idx[k]); total += local_size(sizes[k]); }
    if (total != n) return fail(LVI_ERR_INVALID_ARG, "the kept blocks' local sizes do not add up to n");
    std::vector<char> taken((size_t)n, 0);
    for (int k = 0; k < count; k++) {
        if (idx[k] - lo < 0 || idx[k] - lo + local_size(sizes[k]) > n) return fail(LVI_ERR_INVALID_ARG, "a kept block lies outside the prior's columns");
        for (int j = 0; j < local_size(sizes[k]); j++) {
            if (taken[idx[k] - lo + j]) return fail(LVI_ERR_INVALID_ARG, "two kept blocks of the prior share a column");
            taken[idx[k] - lo + j] = 1;
        }
    }
    if (!finite_all(J, (size_t)n * n) || !finite_all(r, (size_t)n) || !finite_all(values, (size_t)VAL * count)) return fail(LVI_ERR_INVALID_ARG, "the prior is not finite");
    HostPrior p;
    p.valid = true; p.n = n;
    p.ids.assign(ids, ids + count); p.sizes.assign(sizes, sizes + count);
    for (int k = 0; k < count; k++) p.col.push_back(idx[k] - lo);
    p.J.assign(J, J + (size_t)n * n); p.r.assign(r, r + n); p.x0.assign(values, values + (size_t)VAL * count);
    h->prior = std::move(p);
    return LVI_OK;
}

int32_t lvi_win_solve(lvi_win* h, lvi_win_info* info_out)
{
    if (!h) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (h->proj.empty() && h->imu.empty() && !h->prior.valid) return fail(LVI_ERR_STATE, "no factors");
    return guarded(h->device, [&]() -> int32_t {
        const auto t0 = std::chrono::steady_clock::now();
        const auto elapsed = [&]() { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); };
        const lvi_win_params& P = h->P;
        Dev d;
        const int32_t st = upload(h, d);
        if (st != LVI_OK) return st;
        hipStream_t s = h->stream;
        lvi_win_info info{};
        info.dim = d.D; info.eliminated = d.Ne;
        h->log.clear();
        prepare(h, d, 1);
        const auto not_finite = [&]() -> int32_t {
            const bool cov = (h->h_gi->flags & F_COV) != 0;
            info.flags = cov ? 3 : 1; info.time_s = elapsed();
            if (info_out) *info_out = info;
            return cov ? LVI_WIN_BAD_COVARIANCE : LVI_WIN_NOT_FINITE;
        };
        if (h->h_gi->flags & F_SYSTEM) { info.initial_cost = info.final_cost = h->h_gi->cost; return not_finite(); }
        double cost = h->h_gi->cost, grad_max = h->h_gi->grad_max, radius = P.initial_radius, mu = P.initial_mu;
        info.initial_cost = cost;
        lvi_win_iteration e0{};
        e0.cost = cost; e0.gradient_max_norm = grad_max; e0.radius = radius; e0.mu = mu;
        h->log.push_back(e0);
        int term = grad_max <= P.gradient_tolerance ? LVI_WIN_TERM_GRADIENT : LVI_WIN_TERM_NONE, iter = 0, invalid = 0, good = 0;
        bool reuse = false;
        while (term == LVI_WIN_TERM_NONE) {
            if (iter >= P.max_iterations) { term = LVI_WIN_TERM_ITERATIONS; break; }
            if (P.max_time_s > 0. && elapsed() >= P.max_time_s) { term = LVI_WIN_TERM_TIME; break; }
            iter++;
            lvi_win_iteration e{};
            e.iteration = iter; e.cost = cost; e.gradient_max_norm = grad_max; e.radius = radius;
            bool ok = false;
            if (reuse) {
                attempt(h, d, radius, mu, true);
                ok = true;
            } else {
                for (int tries = 0; mu < P.max_mu && tries < 64; tries++) {           // the retry ladder: mu, mu f, mu f^2, ... below max_mu
                    attempt(h, d, radius, mu, false);
                    if (h->h_si->flags & F_CHOL) { mu *= P.mu_increase_factor; e.mu_retries++; continue; }
                    ok = true;
                    break;
                }
            }
            e.mu = mu;
            const StepInfo si = *h->h_si;
            const bool valid = ok && !(si.flags & F_STEP) && si.model_cost_change > 0.;
            if (ok) {
                e.step_kind = si.kind; e.gauss_newton_norm = si.gn_norm; e.cauchy_norm = si.cauchy_norm; e.model_cost_change = si.model_cost_change;
                e.step_norm = si.step_norm;
            }
            if (!valid) {
                invalid++;
                h->log.push_back(e);
                if (invalid >= P.max_invalid_steps) { term = LVI_WIN_TERM_INVALID_STEPS; break; }
                radius *= 0.5; reuse = ok;
                if (radius < P.min_radius) term = LVI_WIN_TERM_RADIUS;
                continue;
            }
            invalid = 0;
            const bool fin = std::isfinite(si.cand_cost);
            e.cost_change = cost - si.cand_cost; e.rho = e.cost_change / si.model_cost_change;
            if (si.step_norm <= P.parameter_tolerance * (h->h_gi->x_norm + P.parameter_tolerance)) { term = LVI_WIN_TERM_PARAMETER; h->log.push_back(e); break; }
            if (fin && std::fabs(e.cost_change) <= P.function_tolerance * cost) { term = LVI_WIN_TERM_FUNCTION; h->log.push_back(e); break; }
            if (fin && e.rho > P.min_relative_decrease) {
                LVI_HIP(hipMemcpyAsync(d.x, d.xc, sizeof(double) * VAL * d.nb, hipMemcpyDeviceToDevice, s));
                prepare(h, d, 0);
                if (h->h_gi->flags & F_SYSTEM) return not_finite();
                cost = h->h_gi->cost; grad_max = h->h_gi->grad_max; good++;
                if (e.rho < P.decrease_threshold) radius *= 0.5;
                if (e.rho > P.increase_threshold) radius = std::max(radius, 3.0 * si.dogleg_norm);
                radius = std::min(P.max_radius, radius);
                mu = std::max(P.min_mu, 2.0 * mu / P.mu_increase_factor);
                reuse = false;
                e.accepted = 1; e.cost = cost; e.gradient_max_norm = grad_max;
                h->log.push_back(e);
                if (grad_max <= P.gradient_tolerance) term = LVI_WIN_TERM_GRADIENT;
            } else {
                radius *= 0.5; reuse = true;
                h->log.push_back(e);
                if (radius < P.min_radius) term = LVI_WIN_TERM_RADIUS;
            }
        }
        LVI_HIP(hipMemcpyAsync(h->h_x, d.x, sizeof(double) * VAL * d.nb, hipMemcpyDeviceToHost, s));
        LVI_HIP(hipStreamSynchronize(s));
        for (int b = 0; b < d.nb; b++) std::memcpy(h->blocks[b].v, h->h_x + (size_t)VAL * b, sizeof(double) * VAL);
        info.iterations = iter; info.successful_steps = good; info.termination = term; info.final_cost = cost; info.radius = radius; info.mu = mu;
        info.time_s = elapsed();
        if (info_out) *info_out = info;
        return LVI_OK;
    });
}

int32_t lvi_win_get_block(lvi_win* h, int32_t id, double* values)
{
    if (!h || !values) return fail(LVI_ERR_INVALID_ARG, "null argument");
    const int b = find(h, id);
    if (b < 0) return fail(LVI_ERR_INVALID_ARG, "the id was not declared");
    std::memcpy(values, h->blocks[b].v, sizeof(double) * h->blocks[b].size);
    return LVI_OK;
}

int32_t lvi_win_get_log(lvi_win* h, int32_t cap, int32_t* count, lvi_win_iteration* log)
{
    if (!h) return fail(LVI_ERR_INVALID_ARG, "null argument");
    const int n = (int)h->log.size();
    if (log && cap < n) return fail(LVI_ERR_CAPACITY, "the array is shorter than the log");
    if (count) *count = n;
    if (log && n > 0) std::memcpy(log, h->log.data(), sizeof(lvi_win_iteration) * n);
    return LVI_OK;
}

int32_t lvi_win_debug_system(lvi_win* h, int32_t cap_dim, int32_t cap_elim, int32_t cap_proj, int32_t cap_dense, int32_t* dim, int32_t* eliminated, int32_t* dense_rows,
                             double* H, double* g, double* hdiag, double* gf, double* W, double* proj_rows, double* dense, double* cost)
{
    if (!h) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (h->proj.empty() && h->imu.empty() && !h->prior.valid) return fail(LVI_ERR_STATE, "no factors");
    return guarded(h->device, [&]() -> int32_t {
        Dev d;
        const int32_t st = upload(h, d);
        if (st != LVI_OK) return st;
        if (((H || g || W) && cap_dim < d.D) || ((hdiag || gf || W) && cap_elim < d.Ne) || (proj_rows && cap_proj < d.P) || (dense && cap_dense < d.Rd))
            return fail(LVI_ERR_CAPACITY, "an array is shorter than what it receives");
        if (dim) *dim = d.D;
        if (eliminated) *eliminated = d.Ne;
        if (dense_rows) *dense_rows = d.Rd;
        prepare(h, d, 1);
        if (cost) *cost = h->h_gi->cost;
        const size_t D = (size_t)d.D, P1 = D + 1, Ne = (size_t)d.Ne;
        std::vector<double> a(P1 * P1), w(std::max<size_t>(1, Ne * P1)), hh(std::max<size_t>(1, Ne));
        LVI_HIP(hipMemcpy(a.data(), d.A, sizeof(double) * P1 * P1, hipMemcpyDeviceToHost));
        if (Ne > 0) LVI_HIP(hipMemcpy(w.data(), d.W, sizeof(double) * Ne * P1, hipMemcpyDeviceToHost));
        if (Ne > 0) LVI_HIP(hipMemcpy(hh.data(), d.h, sizeof(double) * Ne, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < D; i++) {
            if (H) std::memcpy(H + i * D, a.data() + i * P1, sizeof(double) * D);
            if (g) g[i] = a[i * P1 + D];
        }
        for (size_t k = 0; k < Ne; k++) {
            if (hdiag) hdiag[k] = hh[k];
            if (gf) gf[k] = w[k * P1 + D];
            if (W) std::memcpy(W + k * D, w.data() + k * P1, sizeof(double) * D);
        }
        if (proj_rows && d.P > 0) LVI_HIP(hipMemcpy(proj_rows, d.Jf, sizeof(double) * JF * d.P, hipMemcpyDeviceToHost));
        if (dense && d.Rd > 0) LVI_HIP(hipMemcpy(dense, d.E, sizeof(double) * (size_t)d.Rd * P1, hipMemcpyDeviceToHost));
        return (h->h_gi->flags & F_COV) ? LVI_WIN_BAD_COVARIANCE : (h->h_gi->flags & F_SYSTEM) ? LVI_WIN_NOT_FINITE : LVI_OK;
    });
}

}  // extern "C"
