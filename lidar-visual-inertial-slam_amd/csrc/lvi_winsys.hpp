// Internal to liblvi_hip.so: the front end the marginaliser (lvi_marg.hip) and the window solve (lvi_win.hip) share, the
// normal equations of a window's factors.  Every factor is a set of rows [J | r] over the P1 columns of an
// augmented system; A = sum [J r]'[J r] holds sum J'J, sum J'r in its last column and sum r'r in its corner.  Not part of
// include/lvi_marg.h or include/lvi_win.h and not exported.  The layout and the host helpers need no HIP.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "lvi_marg_math.hpp"
#include "../../include/lvi_win.h"

namespace lvi_winsys {

static_assert(LVI_MARG_SHARE == LVI_WIN_SHARE, "one accumulation serves both handles");
static_assert(LVI_MARG_MAX_BLOCK_SIZE == LVI_WIN_MAX_BLOCK_SIZE, "one block table stride serves both handles");

constexpr int TILE = 16;                 // the accumulation's tile edge; TILE x TILE threads
constexpr int SHARE = LVI_MARG_SHARE;    // projection factors of one chunk
constexpr int CH_ROWS = 2 * SHARE;       // rows of one chunk
constexpr int SUB = 64;                  // rows staged in LDS at a time
constexpr int VAL = LVI_MARG_MAX_BLOCK_SIZE;
constexpr int JF = 2 * (lvi_marg_math::PROJ_COLS + 1);      // doubles of one evaluated projection factor
constexpr int PRIOR_THREADS = 256;       // of the prior kernel: one product per thread, so also its LDS arrays' length
static_assert(LVI_MARG_MAX_KEEP_DIM <= PRIOR_THREADS && LVI_WIN_MAX_PRIOR_ROWS <= PRIOR_THREADS, "a prior row is one product per thread");

struct ProjDev { int col[5]; int blk[5]; int use_td; int pad; lvi_marg_math::ProjObs o; };    // col: first column of each block, -1 without one
struct PriorBlk { int size, idx0, blk, newcol; };          // newcol: the block's first column in the system, -1 for a constant block

// What the four kernels read and write, passed by value.  A handle fills it from its own Dev, whose layout its other kernels keep.
struct SysView {
    const double* vals;                  // the blocks' values [block][VAL]
    const ProjDev* proj; double *Jf, *E, *part, *A;        // factors, their rows [P][JF], dense rows [rows][P1], partials [C][P1][P1], the system
    const double *J0, *r0, *x0; const PriorBlk* pb;        // the previous prior [n0][n0], [n0], [nkb0][VAL] and its nkb0 blocks
    double* cost;                        // per-factor costs, or null: projections at [f], prior rows at [cost0 + row]
    int* flags; int bit;                 // the word and the bit a non-finite entry of A raises
    double* corner;                      // where the corner of A is stored as well, or null
    int P, prior_row0, rows, n0, nkb0, P1, Cp, C, cost0;   // prior_row0: the first row of E the prior writes; rows: all rows of E
    int loss_type; double loss_a; lvi_marg_math::ProjConst pc;
};

#if defined(__HIPCC__)
// projections (P > 0) and prior rows (n0 > 0) at v.vals; store = 0 leaves Jf and E alone and writes the costs only
__attribute__((visibility("hidden"))) void launch_eval_proj(const SysView& v, hipStream_t s, int store);
__attribute__((visibility("hidden"))) void launch_prior_rows(const SysView& v, hipStream_t s, int store);
// A from Jf and E: the chunks' partial tiles, then their sum in chunk order
__attribute__((visibility("hidden"))) void launch_build(const SysView& v, hipStream_t s);
#endif

inline bool finite_all(const double* v, size_t n) { for (size_t i = 0; i < n; i++) if (!std::isfinite(v[i])) return false; return true; }

struct BlockRef { int index, size; bool eliminated; };     // index < 0: not declared

// LVI_OK, or LVI_ERR_INVALID_ARG and in *why what lvi_*_add_projection says: the record's blocks against look(id) -> BlockRef.
// elim_rule: an eliminated block only in the feature slot.
template <class Look> int32_t check_projection(const lvi_marg_projection& p, Look&& look, bool elim_rule, const char** why)
{
    static const int want[5] = {7, 7, 7, 1, 1};
    const int ids[5] = {p.pose_i, p.pose_j, p.ex, p.feature, p.td};
    const auto refuse = [&](const char* msg) -> int32_t { *why = msg; return LVI_ERR_INVALID_ARG; };
    int b[5];
    for (int k = 0; k < 5; k++) {
        if (k == 4 && p.td == -1) { b[k] = -1; continue; }
        const BlockRef r = look(ids[k]);
        b[k] = r.index;
        if (b[k] < 0) return refuse("a projection factor names an id that was not declared");
        if (r.size != want[k]) return refuse("a projection factor's blocks must have sizes 7, 7, 7, 1, 1");
        if (elim_rule && k != 3 && r.eliminated) return refuse("an eliminated block outside the feature slot");
        for (int j = 0; j < k; j++) if (b[j] == b[k]) return refuse("a projection factor names one block twice");
    }
    if (!finite_all(p.pts_i, 14)) return refuse("a projection record is not finite");
    return LVI_OK;
}

// a checked record -> the kernels' record; find(id) -> block index, col[block] its first column or -1
template <class Find> void stage_projection(const lvi_marg_projection& p, Find&& find, const int* col, ProjDev& q)
{
    const int ids[5] = {p.pose_i, p.pose_j, p.ex, p.feature, p.td};
    q.use_td = p.td != -1; q.pad = 0;
    for (int k = 0; k < 5; k++) {
        const int b = (k == 4 && !q.use_td) ? -1 : find(ids[k]);
        q.blk[k] = b < 0 ? 0 : b; q.col[k] = b < 0 ? -1 : col[b];
    }
    std::memcpy(q.o.pts_i, p.pts_i, sizeof(double) * 14);
}

// the kept blocks of a prior (present ids, global sizes, first columns in the prior) -> the kernels' records
template <class Find> void stage_prior_blocks(int count, const int* ids, const int* sizes, const int* idx0, Find&& find, const int* col, PriorBlk* out)
{
    for (int k = 0; k < count; k++) {
        const int b = find(ids[k]);
        out[k] = PriorBlk{sizes[k], idx0[k], b, col[b]};
    }
}

}  // namespace lvi_winsys
