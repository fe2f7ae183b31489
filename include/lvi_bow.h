/* lvi_bow.h — the pose graph's DBoW2 keyframe database on the GPU: query and add of LoopDetector::detectLoop.
 *
 * Restates db.query(keyframe->brief_descriptors, ret, 4, frame_index - 200) and db.add(keyframe->brief_descriptors)
 * (pose_graph/src/loop_detector.cpp:69, 73) over the device-resident keyframe store of include/lvi_kf.h.  The parity
 * target is the reference's own vendored source, restated line by line in tests/bow_ref.py:
 *
 *   vocabulary  the VINSLoop binary layout, ThirdParty/VocabularyBinary.hpp, as TemplatedVocabulary::loadBin reads it
 *               (TemplatedVocabulary.h:1509-1561).  No vocabulary ships with this library: the user supplies the file.
 *   descent     TemplatedVocabulary::transform(feature, id, weight), TemplatedVocabulary.h:1217-1258: from the root, the
 *               first child of the smallest Hamming distance (strict <, so a later equal child loses), down to a leaf
 *   vector      transform(features, v), TemplatedVocabulary.h:1065-1121 with BowVector.cpp:34-84: words of weight > 0
 *               only; TF_IDF and TF add the weight once per occurrence, IDF and BINARY once; divided by the sum of the
 *               values when that sum is > 0 (L1); ordered by word id
 *   query       TemplatedDatabase::queryL1, TemplatedDatabase.h:656-723: entry e takes part iff e < max_id ||
 *               max_id == -1 || e == size - 1; score = -0.5 sum over common words (|q - d| - |q| - |d|); entries without
 *               a common word do not appear; best first, cut to max_results
 *   add         TemplatedDatabase::add, TemplatedDatabase.h:408-475: always consumes the next entry id
 *
 * Two behaviours of the reference are kept on purpose: the newest entry is always eligible, and max_id == -1 (which
 * detectLoop passes at frame 199) lifts the limit altogether.  Equal scores are unspecified there (std::sort on the score
 * alone); here they come back in ascending entry id.
 *
 * The descriptors are the keypoint descriptors of a slot (brief_descriptors), not the window ones.  Only L1_NORM scoring
 * is supported; all four weightings are.  Exported by liblvi_hip.so only; a separate ABI from lvi_hotpath.h and lvi_kf.h,
 * whose versions it does not change.
 */
#ifndef LVI_BOW_H
#define LVI_BOW_H

#include "lvi_kf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LVI_BOW_ABI_VERSION   1
#define LVI_BOW_MAX_RESULTS   32

typedef struct lvi_bow lvi_bow;

typedef struct lvi_bow_result {
    int32_t entry_id;
    int32_t reserved;
    double score;
} lvi_bow_result;

int32_t lvi_bow_abi_version(void);

/* BriefVocabulary(voc_path) + db.setVocabulary(voc, false, 0) (loop_detector.cpp:6-10): `vocab` is the whole file in the
 * VINSLoop layout.  The database lives on the device of `store`, reads its slots and works on its stream; `store` must
 * outlive the handle.  An entry holds at most the store's max_keypoints words.  LVI_ERR_INVALID_ARG for a malformed
 * vocabulary (truncated, ids out of range, a cycle, a leaf without a word, a duplicated word id, a non-finite weight) or
 * max_entries < 1, LVI_ERR_UNSUPPORTED for a scoring other than L1_NORM; nothing is allocated then. */
int32_t lvi_bow_create(lvi_kf *store, const void *vocab, int64_t vocab_bytes, int32_t max_entries, lvi_bow **out);
void lvi_bow_destroy(lvi_bow *h);

/* TemplatedDatabase::size(): m_nentries */
int32_t lvi_bow_size(lvi_bow *h);

/* db.query(kp descriptors of `slot`, ret, max_results, max_id) (TemplatedDatabase.h:607-723).  out holds max_results
 * entries, best first, equal scores in ascending entry id; *n_out = how many were written.  max_results in
 * 1..LVI_BOW_MAX_RESULTS.  LVI_ERR_INVALID_ARG (nothing written) for an empty or released slot or a bad max_results.
 * One launch sequence, one download, one wait. */
int32_t lvi_bow_query(lvi_bow *h, int32_t slot, int32_t max_results, int32_t max_id, lvi_bow_result *out, int32_t *n_out);

/* db.add(kp descriptors of `slot`) (TemplatedDatabase.h:408-475): the entry keeps its BowVector on the device, so the
 * slot may be released or overwritten afterwards.  Always consumes the next entry id, also for an empty vector.  After a
 * query of the same unchanged slot the vector of that query is reused (the reference transforms twice to the same
 * result).  LVI_ERR_CAPACITY with nothing changed once max_entries are held; LVI_ERR_INVALID_ARG for an empty or released
 * slot.  entry_id_out may be NULL. */
int32_t lvi_bow_add(lvi_bow *h, int32_t slot, int32_t *entry_id_out);

/* ---- test views ------------------------------------------------------------------------------------ */
/* transform(feature, id, weight) per descriptor (TemplatedVocabulary.h:1217-1258): desc [n][4] uint64, n at most the
 * store's max_keypoints; word_id [n], weight [n] (either may be NULL).  Stopped words are reported with their weight. */
int32_t lvi_bow_words(lvi_bow *h, const uint64_t *desc, int32_t n, int32_t *word_id, double *weight);
/* the BowVector of an entry, or with entry_id -1 the vector of the last query or add: *n_words, then word_id and value
 * [*n_words] (either may be NULL; max_keypoints entries always suffice).  LVI_ERR_STATE for -1 before any query or add. */
int32_t lvi_bow_get_entry(lvi_bow *h, int32_t entry_id, int32_t *n_words, int32_t *word_id, double *value);

#ifdef __cplusplus
}
#endif
#endif /* LVI_BOW_H */
