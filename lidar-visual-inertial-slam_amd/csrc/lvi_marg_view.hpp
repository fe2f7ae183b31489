// Internal to liblvi_hip.so: what the window solve (lvi_win.hip) reads of a marginaliser's resident prior.  Not part of
// include/lvi_marg.h and not exported.
#pragma once

struct lvi_marg;

namespace lvi {

struct MargPriorView {
    int device, n, count;                 // n: rows and columns of linearized_jacobians; count: kept blocks
    const double *J, *r, *x0;             // device: [n][n], [n], keep_block_data [count][LVI_MARG_MAX_BLOCK_SIZE]
    const int *ids, *sizes, *col;         // host, owned by the handle: present ids, global sizes, first column in the prior
};

// false without a result.  lvi_marg_marginalize waits for its stream before it returns, so the buffers are complete.
__attribute__((visibility("hidden"))) bool marg_prior_view(lvi_marg* h, MargPriorView* out);

}  // namespace lvi
