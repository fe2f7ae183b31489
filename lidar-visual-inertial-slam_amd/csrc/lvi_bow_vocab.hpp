// Host-only model of a DBoW2 BRIEF vocabulary in the VINSLoop binary layout (pose_graph/src/ThirdParty/
// VocabularyBinary.hpp, read by TemplatedVocabulary::loadBin, TemplatedVocabulary.h:1509-1561): parse, validate, flatten.
// No HIP in here: lvi_bow.hip includes it, and a CPU test compiles it alone.
//
//   file    int32 k, L, scoringType, weightingType, nNodes, nWords                          24 bytes
//           nNodes x { int32 nodeId, int32 parentId, double weight, uint64 descriptor[4] }   48 bytes each
//           nWords x { int32 nodeId, int32 wordId }                                           8 bytes each
//
// The root is node 0 and is not in the file.  loadBin appends a node to its parent's children in file order, and the
// descent (TemplatedVocabulary.h:1217-1258) keeps the first child of the smallest distance, so that order decides ties:
// the flattening keeps it.  loadBin itself trusts every id it reads; nothing here does, because the flattened tree is
// what a kernel walks: a malformed file is rejected before anything is allocated, and the device loop is bounded by the
// max_depth found here.
//
// Flat numbering: breadth first from the root (flat 0), the children of one node contiguous and in file order.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace lvi_bowvoc {

// the values of LVI_OK, LVI_ERR_INVALID_ARG and LVI_ERR_UNSUPPORTED (include/lvi_hotpath.h); lvi_bow.hip asserts the equality
constexpr int VOCAB_OK = 0, VOCAB_INVALID = -1, VOCAB_UNSUPPORTED = -6;

constexpr int SCORING_L1_NORM = 0;                                     // BowVector.h:45-53
constexpr int WEIGHT_TF_IDF = 0, WEIGHT_TF = 1, WEIGHT_IDF = 2, WEIGHT_BINARY = 3;   // BowVector.h:36-42
constexpr int64_t HEADER_BYTES = 24, NODE_BYTES = 48, WORD_BYTES = 8;

struct FlatVocab {
    int k = 0, L = 0, scoring = 0, weighting = 0;
    int n_nodes = 0;                       // the root included
    int n_words = 0;
    int max_depth = 0;                     // levels below the root of the deepest leaf: the bound of the descent loop
    std::vector<int32_t> child_begin, child_count;   // [n_nodes] flat index of the first child, number of children (0 = a leaf)
    std::vector<int32_t> word_id;          // [n_nodes] -1 for inner nodes
    std::vector<double> weight;            // [n_nodes]
    std::vector<uint64_t> desc;            // [n_nodes][4]; the root's is zero and never read
    std::vector<int32_t> node_id;          // [n_nodes] the file's nodeId of a flat index

    // TF_IDF and TF accumulate with addWeight, IDF and BINARY with addIfNotExist (TemplatedVocabulary.h:1081-1118)
    bool accumulates() const { return weighting == WEIGHT_TF_IDF || weighting == WEIGHT_TF; }
};

namespace detail {
inline int32_t rd_i32(const unsigned char* p) { int32_t v; std::memcpy(&v, p, 4); return v; }
inline int reject(std::string& err, const char* what) { err = std::string("vocabulary: ") + what; return VOCAB_INVALID; }
}  // namespace detail

// VOCAB_OK and `out` filled, or VOCAB_INVALID / VOCAB_UNSUPPORTED with `out` untouched and the reason in `err`
inline int parse_vocab(const void* buf, int64_t bytes, FlatVocab& out, std::string& err)
{
    using namespace detail;
    if (!buf || bytes < HEADER_BYTES) return reject(err, "shorter than its 24-byte header");
    const unsigned char* p = static_cast<const unsigned char*>(buf);
    const int32_t k = rd_i32(p), L = rd_i32(p + 4), scoring = rd_i32(p + 8), weighting = rd_i32(p + 12), nn = rd_i32(p + 16), nw = rd_i32(p + 20);
    if (nn < 0 || nw < 0) return reject(err, "negative node or word count");
    if (bytes != HEADER_BYTES + NODE_BYTES * (int64_t)nn + WORD_BYTES * (int64_t)nw) return reject(err, "size does not match the node and word counts");
    if (weighting < WEIGHT_TF_IDF || weighting > WEIGHT_BINARY) return reject(err, "unknown weighting type");
    if (scoring != SCORING_L1_NORM) { err = "vocabulary: only L1_NORM scoring is supported"; return VOCAB_UNSUPPORTED; }
    if (nn < 1) return reject(err, "the root has no child");
    if (nn == INT32_MAX) return reject(err, "too many nodes");
    const int N = nn + 1;
    const unsigned char* nodes = p + HEADER_BYTES;
    const unsigned char* words = nodes + NODE_BYTES * (int64_t)nn;

    // file record of each node id, and the children lists in file order as a CSR built in two passes
    std::vector<int32_t> rec_of(N, -1), nchild(N, 0);
    for (int32_t i = 0; i < nn; i++) {
        const unsigned char* r = nodes + NODE_BYTES * (int64_t)i;
        const int32_t id = rd_i32(r), pid = rd_i32(r + 4);
        if (id < 1 || id > nn) return reject(err, "node id out of 1..nNodes");
        if (rec_of[id] >= 0) return reject(err, "duplicated node id");
        if (pid < 0 || pid > nn) return reject(err, "parent id out of 0..nNodes");
        double w;
        std::memcpy(&w, r + 8, 8);
        if (!std::isfinite(w)) return reject(err, "non-finite weight");
        rec_of[id] = i;
        nchild[pid]++;
    }
    std::vector<int32_t> first(N + 1, 0);
    for (int i = 0; i < N; i++) first[i + 1] = first[i] + nchild[i];
    std::vector<int32_t> kids(nn), fill(first.begin(), first.end() - 1);
    for (int32_t i = 0; i < nn; i++) {
        const unsigned char* r = nodes + NODE_BYTES * (int64_t)i;
        kids[fill[rd_i32(r + 4)]++] = rd_i32(r);
    }
    if (nchild[0] < 1) return reject(err, "the root has no child");

    // breadth first from the root: a node that is never reached sits on a cycle (every node has exactly one parent)
    FlatVocab v;
    v.k = k; v.L = L; v.scoring = scoring; v.weighting = weighting; v.n_nodes = N; v.n_words = nw;
    v.child_begin.assign(N, 0); v.child_count.assign(N, 0); v.word_id.assign(N, -1); v.weight.assign(N, 0.0);
    v.desc.assign(4 * (size_t)N, 0); v.node_id.assign(N, 0);
    std::vector<int32_t> flat_of(N, -1), depth(N, 0);
    flat_of[0] = 0;
    int next = 1;
    for (int f = 0; f < next; f++) {                       // v.node_id[0 .. next) is the queue
        const int32_t id = v.node_id[f];
        v.child_begin[f] = next; v.child_count[f] = nchild[id];
        for (int32_t c = first[id]; c < first[id + 1]; c++) {
            const int32_t cid = kids[c];
            if (flat_of[cid] >= 0) return reject(err, "a node is reached twice");     // unreachable with unique ids; kept as a bound on `next`
            flat_of[cid] = next; v.node_id[next] = cid; depth[next] = depth[f] + 1;
            if (depth[next] > v.max_depth) v.max_depth = depth[next];
            const unsigned char* r = nodes + NODE_BYTES * (int64_t)rec_of[cid];
            std::memcpy(&v.weight[next], r + 8, 8);
            std::memcpy(&v.desc[4 * (size_t)next], r + 16, 32);
            next++;
        }
    }
    if (next != N) return reject(err, "a node does not reach the root (cycle)");

    // the words are exactly the leaves, one word per leaf; the word ids a permutation of 0..nWords-1
    int leaves = 0;
    for (int f = 0; f < N; f++) leaves += v.child_count[f] == 0;
    std::vector<char> seen(nw, 0);
    for (int32_t i = 0; i < nw; i++) {
        const unsigned char* r = words + WORD_BYTES * (int64_t)i;
        const int32_t id = rd_i32(r), wid = rd_i32(r + 4);
        if (id < 1 || id > nn) return reject(err, "a word names a node out of 1..nNodes");
        if (wid < 0 || wid >= nw) return reject(err, "word id out of 0..nWords-1");
        const int f = flat_of[id];
        if (v.child_count[f] != 0) return reject(err, "a word names an inner node");
        if (v.word_id[f] >= 0) return reject(err, "two words name one leaf");
        if (seen[wid]) return reject(err, "duplicated word id");
        seen[wid] = 1;
        v.word_id[f] = wid;
    }
    if (leaves != nw) return reject(err, "a leaf has no word");
    out = std::move(v);
    return VOCAB_OK;
}

// BriefVocabulary(voc_path): the whole file through parse_vocab
inline int load_vocab_file(const char* path, FlatVocab& out, std::string& err, std::vector<unsigned char>* raw = nullptr)
{
    FILE* f = path ? std::fopen(path, "rb") : nullptr;
    if (!f) return detail::reject(err, "cannot open the file");
    std::vector<unsigned char> b;
    unsigned char chunk[1 << 16];
    size_t got;
    while ((got = std::fread(chunk, 1, sizeof(chunk), f)) > 0) b.insert(b.end(), chunk, chunk + got);
    std::fclose(f);
    const int st = parse_vocab(b.data(), (int64_t)b.size(), out, err);
    if (st == VOCAB_OK && raw) *raw = std::move(b);
    return st;
}

// TemplatedVocabulary::transform(feature, word_id, weight) on the flattened tree (TemplatedVocabulary.h:1217-1258): the
// host statement of what bow_descend computes, for the stand-alone check of this header
inline void transform_one(const FlatVocab& v, const uint64_t d[4], int32_t& word_id, double& weight)
{
    int cur = 0;
    while (v.child_count[cur] > 0) {
        int best = 0, best_d = 1 << 30;
        for (int c = 0; c < v.child_count[cur]; c++) {
            const uint64_t* n = &v.desc[4 * (size_t)(v.child_begin[cur] + c)];
            const int dist = __builtin_popcountll(d[0] ^ n[0]) + __builtin_popcountll(d[1] ^ n[1]) + __builtin_popcountll(d[2] ^ n[2]) +
                             __builtin_popcountll(d[3] ^ n[3]);
            if (dist < best_d) { best_d = dist; best = c; }                // strict <: a later equal child loses
        }
        cur = v.child_begin[cur] + best;
    }
    word_id = v.word_id[cur];
    weight = v.weight[cur];
}

}  // namespace lvi_bowvoc
