// The pose graph's DBoW2 keyframe database on the GPU (include/lvi_bow.h; the contract is DESIGN §15): db.query and
// db.add of LoopDetector::detectLoop (loop_detector.cpp:69, 73) over the keyframe store of lvi_kf.hip.
//
//   bow_descend   transform(feature, id, weight), TemplatedVocabulary.h:1217-1258: 16 lanes per descriptor, one child per
//                 lane (looping when a node has more than 16), XOR + popcount over 4 x u64, packed (distance << 32 |
//                 child ordinal) minimum over the 16 lanes: the lowest ordinal wins a tie, as `d < best_d` does.  The loop
//                 runs at most the max_depth that lvi_bow_vocab.hpp found while validating the tree.
//   (lvi_sort)    stable radix sort of (word id, descriptor index); stopped words (weight <= 0) carry the key n_words and
//                 end up behind every kept word
//   bow_vector    transform(features, v), TemplatedVocabulary.h:1065-1121 + BowVector.cpp:34-84: one workgroup scans the
//                 run heads of the sorted keys; a head adds its word's weight once per occurrence (TF_IDF, TF) or once
//                 (IDF, BINARY), one thread sums the values in word order, every thread divides
//   bow_score     queryL1, TemplatedDatabase.h:656-697, entry-major instead of through an inverted file: one wavefront per
//                 eligible entry walks the entry's sorted words 64 at a time, each lane looks its word up in the query
//                 vector (held in LDS) by bisection, and the terms of the lanes that hit are added in lane order
//   bow_rank      :699-722: the rank of every scored entry under (raw score ascending, entry id ascending); ranks below
//                 max_results write the result rows
//   bow_append    add(v), :441-475: the staged vector becomes entry `size` of the CSR pool
//
// Order of the sums.  A BowVector is a std::map, so the reference adds the L1 norm in ascending word id, and an entry's
// score receives its terms in ascending word id too (the outer loop of queryL1 runs over the query's words).  bow_vector
// and bow_score add in exactly that order (sequentially; the lanes of bow_score only compute the terms in parallel), and
// a repeated word's value is the same weight added c times, which has one order only.  So values and scores equal
// tests/bow_ref.py bit for bit, and two runs give identical bits; the tests nevertheless only ask for the derived bound
// of DESIGN §15.
//
// Build flags: this file is compiled like the rest of the library, -O3 -ffp-contract=off.  Nothing in it could contract:
// the score is |q - d| - |q| - |d| (no multiply), the vector build is additions and one f64 division per word, which
// hipcc expands to the correctly rounded sequence.  No -ffast-math anywhere in build.py, so the sums are not reassociated.
#include "lvi_bow_vocab.hpp"
#include "lvi_kf_store.hpp"
#include "lvi_sort.hpp"
#include "../../include/lvi_bow.h"

using namespace lvi;

static_assert(lvi_bowvoc::VOCAB_OK == LVI_OK && lvi_bowvoc::VOCAB_INVALID == LVI_ERR_INVALID_ARG && lvi_bowvoc::VOCAB_UNSUPPORTED == LVI_ERR_UNSUPPORTED,
              "lvi_bow_vocab.hpp restates the status codes of lvi_hotpath.h");
static_assert(sizeof(lvi_bow_result) == 16, "lvi_bow_result is {i32, i32, f64}");

namespace {

constexpr int GROUP = 16;                    // lanes per descriptor in bow_descend
constexpr int Q_LDS = 2048;                  // query words bow_score keeps in LDS (24 KiB); a longer vector is read from global memory
constexpr int VEC_BLOCK = 1024;

struct VocabDev {
    const int *child_begin, *child_count, *word;
    const double* weight;
    const ulonglong2* desc;                  // [n_nodes][2]
    int max_depth, n_words;
};

__global__ __launch_bounds__(256) void bow_descend_kernel(VocabDev v, const ulonglong2* __restrict__ desc, int n, int* __restrict__ word_out,
                                                          double* __restrict__ weight_out, unsigned* __restrict__ keys, unsigned* __restrict__ vals,
                                                          int* __restrict__ d_n)
{
    const int gl = threadIdx.x & (GROUP - 1);
    const int i = blockIdx.x * (256 / GROUP) + (threadIdx.x / GROUP);
    if (blockIdx.x == 0 && threadIdx.x == 0) *d_n = n;                           // the length the sort reads
    const bool live = i < n;
    ulonglong2 a0 = make_ulonglong2(0, 0), a1 = a0;
    if (live) { a0 = desc[2 * (size_t)i]; a1 = desc[2 * (size_t)i + 1]; }
    int cur = 0;
    for (int lvl = 0; lvl < v.max_depth; lvl++) {
        const int cc = live ? v.child_count[cur] : 0, cb = live ? v.child_begin[cur] : 0;
        if (!__any(cc > 0)) break;                                               // the whole wavefront stands on leaves
        unsigned long long best = ~0ull;
        for (int c = gl; c < cc; c += GROUP) {
            const ulonglong2 b0 = v.desc[2 * (size_t)(cb + c)], b1 = v.desc[2 * (size_t)(cb + c) + 1];
            const int d = __popcll(a0.x ^ b0.x) + __popcll(a0.y ^ b0.y) + __popcll(a1.x ^ b1.x) + __popcll(a1.y ^ b1.y);
            const unsigned long long key = ((unsigned long long)d << 32) | (unsigned)c;
            best = key < best ? key : best;
        }
#pragma unroll
        for (int o = GROUP / 2; o > 0; o >>= 1) { const unsigned long long t = __shfl_xor(best, o, 64); best = t < best ? t : best; }
        if (cc > 0) cur = cb + (int)(unsigned)best;
    }
    if (live && gl == 0) {
        // a validated tree has no leaf below max_depth, so cur is a leaf here
        const int id = v.word[cur];
        const double w = v.weight[cur];
        if (word_out) word_out[i] = id;
        weight_out[i] = w;
        keys[i] = w > 0 ? (unsigned)id : (unsigned)v.n_words;                    // "if(w > 0)": a stopped word drops out
        vals[i] = (unsigned)i;
    }
}

// one workgroup.  keys/vals: the sorted pairs; weight [n] by descriptor index.  Writes the vector (word ascending) and its length.
__global__ __launch_bounds__(VEC_BLOCK) void bow_vector_kernel(const unsigned* __restrict__ keys, const unsigned* __restrict__ vals, const double* __restrict__ weight,
                                                               int n, unsigned stopped, int accumulate, int* __restrict__ q_word, double* __restrict__ q_val,
                                                               int* __restrict__ q_count)
{
    __shared__ int ws[VEC_BLOCK / 64 + 1];
    __shared__ double s_norm;
    int carry = 0;
    for (int base = 0; base < n; base += VEC_BLOCK) {
        const int i = base + threadIdx.x;
        const unsigned k = i < n ? keys[i] : stopped;
        const bool head = i < n && k != stopped && (i == 0 || keys[i - 1] != k);
        int total;
        const int ex = block_excl_scan<VEC_BLOCK>(head ? 1 : 0, ws, &total);
        if (head) {
            int c = 1;
            while (i + c < n && keys[i + c] == k) c++;
            const double w = weight[vals[i]];                                    // every occurrence of a word carries the same weight
            double val = w;
            if (accumulate)
                for (int j = 1; j < c; j++) val += w;                            // addWeight once per occurrence
            q_word[carry + ex] = (int)k;
            q_val[carry + ex] = val;
        }
        carry += total;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double norm = 0.0;
        for (int j = 0; j < carry; j++) norm += fabs(q_val[j]);                  // BowVector::normalize(L1): in word order
        s_norm = norm;
        *q_count = carry;
    }
    __syncthreads();
    const double norm = s_norm;
    if (norm > 0.0)
        for (int j = threadIdx.x; j < carry; j += VEC_BLOCK) q_val[j] /= norm;
}

// raw[e] = the sum of queryL1 for entry e (negative), or 1 when e is not eligible or shares no word with the query
__global__ __launch_bounds__(256) void bow_score_kernel(const int* __restrict__ q_word, const double* __restrict__ q_val, const int* __restrict__ q_count,
                                                        const int* __restrict__ e_off, const int* __restrict__ pool_word, const double* __restrict__ pool_val,
                                                        int size, int max_id, double* __restrict__ raw, lvi_bow_result* __restrict__ out)
{
    __shared__ int s_w[Q_LDS];
    __shared__ double s_v[Q_LDS];
    const int nq = *q_count;
    const bool in_lds = nq <= Q_LDS;
    if (in_lds)
        for (int j = threadIdx.x; j < nq; j += 256) { s_w[j] = q_word[j]; s_v[j] = q_val[j]; }
    if (blockIdx.x == 0 && threadIdx.x < LVI_BOW_MAX_RESULTS) { out[threadIdx.x].entry_id = -1; out[threadIdx.x].reserved = 0; out[threadIdx.x].score = 0.0; }
    __syncthreads();
    const int e = blockIdx.x * 4 + wave_id(), lane = lane_id();
    if (e >= size) return;                                                       // the whole wavefront; no barrier follows
    const bool eligible = e < max_id || max_id == -1 || e == size - 1;           // TemplatedDatabase.h:679
    double acc = 0.0;
    bool any = false;
    if (eligible && nq > 0) {
        const int b = e_off[e], m = e_off[e + 1] - b;
        for (int base = 0; base < m; base += 64) {
            const int j = base + lane;
            bool hit = false;
            double term = 0.0;
            if (j < m) {
                const int w = pool_word[b + j];
                int lo = 0, hi = nq;                                             // first query word >= w
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    const int qw = in_lds ? s_w[mid] : q_word[mid];
                    if (qw < w) lo = mid + 1; else hi = mid;
                }
                if (lo < nq && (in_lds ? s_w[lo] : q_word[lo]) == w) {
                    const double q = in_lds ? s_v[lo] : q_val[lo], d = pool_val[b + j];
                    term = fabs(q - d) - fabs(q) - fabs(d);
                    hit = true;
                }
            }
            uint64_t mask = __ballot(hit);
            any = any || mask != 0;
            while (mask) {                                                       // wavefront-uniform: the common words in ascending id
                const int l = __ffsll((unsigned long long)mask) - 1;
                acc += __shfl(term, l, 64);
                mask &= mask - 1;
            }
        }
    }
    if (lane == 0) raw[e] = any ? acc : 1.0;
}

// std::sort of the results and the cut (TemplatedDatabase.h:699-722) as a rank: the entries that scored are ordered by
// (raw ascending, entry id ascending), a total order, so the ranks are 0 .. scored-1 without gaps
__global__ __launch_bounds__(256) void bow_rank_kernel(const double* __restrict__ raw, int size, int max_results, lvi_bow_result* __restrict__ out)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= size) return;
    const double r = raw[e];
    if (r > 0.5) return;
    int rank = 0;
    for (int f = 0; f < size; f++) {
        const double rf = raw[f];
        rank += rf <= 0.5 && (rf < r || (rf == r && f < e)) ? 1 : 0;
    }
    if (rank < max_results) { out[rank].entry_id = e; out[rank].reserved = 0; out[rank].score = -r / 2.0; }
}

__global__ __launch_bounds__(256) void bow_append_kernel(const int* __restrict__ q_word, const double* __restrict__ q_val, const int* __restrict__ q_count, int e,
                                                         int* __restrict__ e_off, int* __restrict__ pool_word, double* __restrict__ pool_val)
{
    const int cnt = *q_count, off = e_off[e];
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j == 0) e_off[e + 1] = off + cnt;
    if (j < cnt) { pool_word[off + j] = q_word[j]; pool_val[off + j] = q_val[j]; }
}

int bit_width(unsigned v) { int b = 0; while (v) { b++; v >>= 1; } return b; }

}  // namespace

// ---------------------------------------------------------------------------------------------- the handle
struct lvi_bow : Handle {                   // on the store's device and stream (sv)
    lvi_kf* store = nullptr;
    KfStoreView sv;
    int K = 0, max_entries = 0, size = 0;
    int n_nodes = 0, n_words = 0, max_depth = 0, accumulate = 0, sort_passes = 0;
    int *d_child_begin = nullptr, *d_child_count = nullptr, *d_node_word = nullptr;
    double* d_node_weight = nullptr;
    ulonglong2* d_node_desc = nullptr;
    ulonglong2* d_desc_in = nullptr;         // [K][2] the descriptors of lvi_bow_words
    int* d_word = nullptr;                   // [K] per descriptor
    double* d_weight = nullptr;              // [K]
    SortPlan plan;
    int *d_n = nullptr, *d_nbits = nullptr;
    int *d_q_word = nullptr, *d_q_count = nullptr;      // the staged vector
    double* d_q_val = nullptr;
    int *d_e_off = nullptr, *d_pool_word = nullptr;     // CSR: entry e owns [e_off[e], e_off[e + 1]) of the pool
    double *d_pool_val = nullptr, *d_raw = nullptr;
    lvi_bow_result* d_out = nullptr;
    char* h_out = nullptr;                   // pinned: the result rows | two ints
    bool staged = false;                     // the staged vector is that of (staged_slot, staged_gen)
    int staged_slot = -1;
    uint64_t staged_gen = 0;

    template <class A, class B> void layout(A& a, B& pin)
    {
        h_out = pin.template alloc<char>(sizeof(lvi_bow_result) * LVI_BOW_MAX_RESULTS + 64);
        d_child_begin = a.template alloc<int>(n_nodes);
        d_child_count = a.template alloc<int>(n_nodes);
        d_node_word = a.template alloc<int>(n_nodes);
        d_node_weight = a.template alloc<double>(n_nodes);
        d_node_desc = a.template alloc<ulonglong2>(2 * (size_t)n_nodes);
        d_desc_in = a.template alloc<ulonglong2>(2 * (size_t)K);
        d_word = a.template alloc<int>(K);
        d_weight = a.template alloc<double>(K);
        plan.allocate(a, 1, K, RS_ITEMS_SMALL);
        d_n = a.template alloc<int>(1);
        d_nbits = a.template alloc<int>(1);
        d_q_word = a.template alloc<int>(K);
        d_q_val = a.template alloc<double>(K);
        d_q_count = a.template alloc<int>(1);
        d_e_off = a.template alloc<int>((size_t)max_entries + 1);
        d_pool_word = a.template alloc<int>((size_t)max_entries * K);
        d_pool_val = a.template alloc<double>((size_t)max_entries * K);
        d_raw = a.template alloc<double>(max_entries);
        d_out = a.template alloc<lvi_bow_result>(LVI_BOW_MAX_RESULTS);
    }

    VocabDev vocab() const { return VocabDev{d_child_begin, d_child_count, d_node_word, d_node_weight, d_node_desc, max_depth, n_words}; }
    const unsigned* sorted_keys() const { return (sort_passes & 1) ? plan.keysB : plan.keysA; }
    const unsigned* sorted_vals() const { return (sort_passes & 1) ? plan.valsB : plan.valsA; }
};

namespace {

void launch_descend(lvi_bow* h, const ulonglong2* desc, int n, int* word_out)
{
    hipLaunchKernelGGL(bow_descend_kernel, dim3(std::max(1, div_up(n, 256 / GROUP))), dim3(256), 0, h->sv.stream, h->vocab(), desc, n, word_out, h->d_weight,
                       h->plan.keysA, h->plan.valsA, h->d_n);
    LVI_HIP(hipGetLastError());
}

// m_voc->transform(features, vec) of the slot into the staged vector, unless it already holds that slot's
void stage_vector(lvi_bow* h, int32_t slot, const KfSlotView& s)
{
    if (h->staged && h->staged_slot == slot && h->staged_gen == s.generation) return;
    h->staged = false;
    launch_descend(h, s.kp_desc, s.n_kp, h->d_word);
    Ctx ctx;
    ctx.stream = h->sv.stream;
    radix_sort_pairs(ctx, h->plan, h->d_n, h->d_nbits, h->sort_passes, "bow", (double)s.n_kp);
    hipLaunchKernelGGL(bow_vector_kernel, dim3(1), dim3(VEC_BLOCK), 0, h->sv.stream, h->sorted_keys(), h->sorted_vals(), h->d_weight, s.n_kp, (unsigned)h->n_words,
                       h->accumulate, h->d_q_word, h->d_q_val, h->d_q_count);
    LVI_HIP(hipGetLastError());
    h->staged = true; h->staged_slot = slot; h->staged_gen = s.generation;
}

}  // namespace

extern "C" {

int32_t lvi_bow_abi_version(void) { return LVI_BOW_ABI_VERSION; }

int32_t lvi_bow_create(lvi_kf* store, const void* vocab, int64_t vocab_bytes, int32_t max_entries, lvi_bow** out)
{
    if (!out) return fail(LVI_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    KfStoreView sv;
    if (!kf_store_view(store, &sv)) return fail(LVI_ERR_INVALID_ARG, "null keyframe store");
    if (!vocab) return fail(LVI_ERR_INVALID_ARG, "null vocabulary");
    if (max_entries < 1 || (int64_t)max_entries * sv.max_keypoints > INT32_MAX)
        return fail(LVI_ERR_INVALID_ARG, "max_entries must be positive and max_entries * max_keypoints below 2^31");
    lvi_bowvoc::FlatVocab fv;
    std::string err;
    const int pst = lvi_bowvoc::parse_vocab(vocab, vocab_bytes, fv, err);
    if (pst != lvi_bowvoc::VOCAB_OK) return fail(pst, err);
    const int nbits = bit_width((unsigned)fv.n_words);                           // keys are 0 .. n_words, the last one the stopped words'
    return create_handle(sv.device, out, lvi_bow_destroy, [&](lvi_bow* h) {
        h->store = store; h->sv = sv; h->K = sv.max_keypoints; h->max_entries = max_entries;
        h->n_nodes = fv.n_nodes; h->n_words = fv.n_words; h->max_depth = fv.max_depth; h->accumulate = fv.accumulates() ? 1 : 0;
        h->sort_passes = (nbits + 7) / 8;
    }, [&](lvi_bow* h) -> int32_t {
        h->open(sv.device, [&](auto& dev, auto& pin) { h->layout(dev, pin); }, 0, sv.stream);
        const size_t n = (size_t)fv.n_nodes;
        const int zero = 0;
        LVI_HIP(hipMemcpyAsync(h->d_child_begin, fv.child_begin.data(), 4 * n, hipMemcpyHostToDevice, sv.stream));
        LVI_HIP(hipMemcpyAsync(h->d_child_count, fv.child_count.data(), 4 * n, hipMemcpyHostToDevice, sv.stream));
        LVI_HIP(hipMemcpyAsync(h->d_node_word, fv.word_id.data(), 4 * n, hipMemcpyHostToDevice, sv.stream));
        LVI_HIP(hipMemcpyAsync(h->d_node_weight, fv.weight.data(), 8 * n, hipMemcpyHostToDevice, sv.stream));
        LVI_HIP(hipMemcpyAsync(h->d_node_desc, fv.desc.data(), 32 * n, hipMemcpyHostToDevice, sv.stream));
        LVI_HIP(hipMemcpyAsync(h->d_nbits, &nbits, 4, hipMemcpyHostToDevice, sv.stream));
        LVI_HIP(hipMemcpyAsync(h->d_e_off, &zero, 4, hipMemcpyHostToDevice, sv.stream));
        LVI_HIP(hipMemsetAsync(h->d_q_count, 0, 4, sv.stream));
        LVI_HIP(hipStreamSynchronize(sv.stream));                                // the host arrays die with this call
        return LVI_OK;
    });
}

void lvi_bow_destroy(lvi_bow* h)
{
    if (!h) return;
    h->close();
    delete h;
}

int32_t lvi_bow_size(lvi_bow* h) { return h ? h->size : fail(LVI_ERR_INVALID_ARG, "null handle"); }

int32_t lvi_bow_query(lvi_bow* h, int32_t slot, int32_t max_results, int32_t max_id, lvi_bow_result* out, int32_t* n_out)
{
    if (!h || !out || !n_out) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (max_results < 1 || max_results > LVI_BOW_MAX_RESULTS) return fail(LVI_ERR_INVALID_ARG, "max_results must be 1..LVI_BOW_MAX_RESULTS");
    KfSlotView s;
    if (!kf_slot_view(h->store, slot, &s)) return fail(LVI_ERR_INVALID_ARG, "slot out of range");
    if (!s.valid) return fail(LVI_ERR_INVALID_ARG, "empty or released slot");
    return guarded(h->sv.device, [&]() -> int32_t {
        stage_vector(h, slot, s);
        int n = 0;
        lvi_bow_result* rows = reinterpret_cast<lvi_bow_result*>(h->h_out);
        if (h->size > 0) {
            hipLaunchKernelGGL(bow_score_kernel, dim3(div_up(h->size, 4)), dim3(256), 0, h->sv.stream, h->d_q_word, h->d_q_val, h->d_q_count, h->d_e_off,
                               h->d_pool_word, h->d_pool_val, h->size, max_id, h->d_raw, h->d_out);
            LVI_HIP(hipGetLastError());
            hipLaunchKernelGGL(bow_rank_kernel, dim3(div_up(h->size, 256)), dim3(256), 0, h->sv.stream, h->d_raw, h->size, max_results, h->d_out);
            LVI_HIP(hipGetLastError());
            LVI_HIP(hipMemcpyAsync(rows, h->d_out, sizeof(lvi_bow_result) * max_results, hipMemcpyDeviceToHost, h->sv.stream));
        }
        LVI_HIP(hipStreamSynchronize(h->sv.stream));
        if (h->size > 0)
            while (n < max_results && rows[n].entry_id >= 0) n++;
        std::memcpy(out, rows, sizeof(lvi_bow_result) * (size_t)n);
        *n_out = n;
        return LVI_OK;
    });
}

int32_t lvi_bow_add(lvi_bow* h, int32_t slot, int32_t* entry_id_out)
{
    if (!h) return fail(LVI_ERR_INVALID_ARG, "null handle");
    KfSlotView s;
    if (!kf_slot_view(h->store, slot, &s)) return fail(LVI_ERR_INVALID_ARG, "slot out of range");
    if (!s.valid) return fail(LVI_ERR_INVALID_ARG, "empty or released slot");
    if (h->size >= h->max_entries) return fail(LVI_ERR_CAPACITY, "the database holds max_entries entries");
    return guarded(h->sv.device, [&]() -> int32_t {
        stage_vector(h, slot, s);
        hipLaunchKernelGGL(bow_append_kernel, dim3(div_up(h->K, 256)), dim3(256), 0, h->sv.stream, h->d_q_word, h->d_q_val, h->d_q_count, h->size, h->d_e_off,
                           h->d_pool_word, h->d_pool_val);
        LVI_HIP(hipGetLastError());
        LVI_HIP(hipStreamSynchronize(h->sv.stream));
        if (entry_id_out) *entry_id_out = h->size;
        h->size++;
        return LVI_OK;
    });
}

int32_t lvi_bow_words(lvi_bow* h, const uint64_t* desc, int32_t n, int32_t* word_id, double* weight)
{
    if (!h) return fail(LVI_ERR_INVALID_ARG, "null handle");
    if (n < 0 || n > h->K) return fail(LVI_ERR_INVALID_ARG, "n must be 0..max_keypoints of the store");
    if (n > 0 && !desc) return fail(LVI_ERR_INVALID_ARG, "null descriptors");
    if (n == 0) return LVI_OK;
    return guarded(h->sv.device, [&]() -> int32_t {
        LVI_HIP(hipMemcpyAsync(h->d_desc_in, desc, 32 * (size_t)n, hipMemcpyHostToDevice, h->sv.stream));
        // the descent shares d_word, d_weight and the sort's input with stage_vector; the staged vector itself is not touched
        launch_descend(h, h->d_desc_in, n, h->d_word);
        if (word_id) LVI_HIP(hipMemcpyAsync(word_id, h->d_word, 4 * (size_t)n, hipMemcpyDeviceToHost, h->sv.stream));
        if (weight) LVI_HIP(hipMemcpyAsync(weight, h->d_weight, 8 * (size_t)n, hipMemcpyDeviceToHost, h->sv.stream));
        LVI_HIP(hipStreamSynchronize(h->sv.stream));
        return LVI_OK;
    });
}

int32_t lvi_bow_get_entry(lvi_bow* h, int32_t entry_id, int32_t* n_words, int32_t* word_id, double* value)
{
    if (!h || !n_words) return fail(LVI_ERR_INVALID_ARG, "null argument");
    if (entry_id < -1 || entry_id >= h->size) return fail(LVI_ERR_INVALID_ARG, "entry id out of range");
    if (entry_id == -1 && !h->staged) return fail(LVI_ERR_STATE, "no query or add yet");
    return guarded(h->sv.device, [&]() -> int32_t {
        int* hi = reinterpret_cast<int*>(h->h_out + sizeof(lvi_bow_result) * LVI_BOW_MAX_RESULTS);
        const int *src_w = h->d_q_word;
        const double* src_v = h->d_q_val;
        int n = 0;
        if (entry_id == -1) {
            LVI_HIP(hipMemcpyAsync(hi, h->d_q_count, 4, hipMemcpyDeviceToHost, h->sv.stream));
            LVI_HIP(hipStreamSynchronize(h->sv.stream));
            n = hi[0];
        } else {
            LVI_HIP(hipMemcpyAsync(hi, h->d_e_off + entry_id, 8, hipMemcpyDeviceToHost, h->sv.stream));
            LVI_HIP(hipStreamSynchronize(h->sv.stream));
            n = hi[1] - hi[0];
            src_w = h->d_pool_word + hi[0]; src_v = h->d_pool_val + hi[0];
        }
        *n_words = n;
        if (n > 0 && word_id) LVI_HIP(hipMemcpyAsync(word_id, src_w, 4 * (size_t)n, hipMemcpyDeviceToHost, h->sv.stream));
        if (n > 0 && value) LVI_HIP(hipMemcpyAsync(value, src_v, 8 * (size_t)n, hipMemcpyDeviceToHost, h->sv.stream));
        if (n > 0 && (word_id || value)) LVI_HIP(hipStreamSynchronize(h->sv.stream));
        return LVI_OK;
    });
}

}  // extern "C"
