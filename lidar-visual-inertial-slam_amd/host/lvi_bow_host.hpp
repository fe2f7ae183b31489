// Host-side mirror of the pose_graph LoopDetector over include/lvi_bow.h and the KeyFrameDescriber of lvi_kf_host.hpp:
//
//   LoopDetector::loadVocabulary       loop_detector.cpp:6-10     BriefVocabulary(voc_path) + db.setVocabulary   -> loadVocabulary
//   LoopDetector::addKeyFrame          loop_detector.cpp:12-40    detectLoop or addKeyFrameIntoVoc, findConnection
//                                                                 on a hit, keyframelist.push_back                -> addKeyFrame
//   LoopDetector::getKeyFrame          loop_detector.cpp:42-54                                                    -> getKeyFrame
//   LoopDetector::detectLoop           loop_detector.cpp:56-139   db.query(.., 4, frame_index - 200), db.add, the
//                                                                 score gates and the min-index scan              -> detectLoop
//   LoopDetector::addKeyFrameIntoVoc   loop_detector.cpp:141-154  db.add                                          -> addKeyFrameIntoVoc
//
// The database works on the descriptors where the describer left them: nothing is downloaded for the query.  What the
// reference does with a confirmed connection (the match message) and the DEBUG_IMAGE code stay with the caller / are not
// restated.  findConnection is the front half of lvi_kf_host.hpp (up to PnPRANSAC) unless usePnP installed a PnPRansac
// (lvi_pnp_host.hpp): then it is the whole of KeyFrame::findConnection and `connected` is the reference's boolean.  Like the reference, detectLoop
// assumes that the database's entry id of a keyframe equals its index: keyframes arrive with index 0, 1, 2, ...
// Only liblvi_hip.so exports this ABI, so only code linked against it may include this header.
#pragma once
#include <cstdio>
#include <list>
#include <string>
#include <vector>

#include "../../include/lvi_bow.h"
#include "lvi_kf_host.hpp"
#include "lvi_pnp_host.hpp"

namespace lvi_host {

struct LoopResult {
    int loop_index = -1;                       // detectLoop's return value
    bool connected = false;                    // findConnectionFront passed its > MIN_LOOP_NUM gate; with usePnP: findConnection's return value
    Connection connection;                     // valid when loop_index != -1; with usePnP it carries PnPRANSAC's status
    std::vector<lvi_bow_result> ret;           // QueryResults of this frame's query (empty without flag_detect_loop)
};

class LoopDetector {
public:
    LoopDetector(KeyFrameDescriber& kd, int max_entries) : kd_(kd), max_entries_(max_entries) {}
    ~LoopDetector() { lvi_bow_destroy(db_); }
    LoopDetector(const LoopDetector&) = delete;
    LoopDetector& operator=(const LoopDetector&) = delete;
    lvi_bow* db() const { return db_; }

    // KeyFrame::findConnection's second half (PnPRANSAC and the second > MIN_LOOP_NUM gate, keyframe.cpp:200-211) :=
    // this PnPRansac, which must outlive its use; nullptr (the default) = the front half alone, as before
    void usePnP(PnPRansac* pnp) { pnp_ = pnp; }

    // loop_detector.cpp:6-10 (pose_graph_node.cpp:300-304 calls it with pkg_path + vocabulary_file).  The file is not
    // shipped with this library.
    void loadVocabulary(const std::string& voc_path)
    {
        FILE* f = std::fopen(voc_path.c_str(), "rb");
        if (!f) throw Error(LVI_ERR_INVALID_ARG, "LoopDetector::loadVocabulary: cannot open " + voc_path);
        std::vector<unsigned char> b;
        unsigned char chunk[1 << 16];
        size_t got;
        while ((got = std::fread(chunk, 1, sizeof(chunk), f)) > 0) b.insert(b.end(), chunk, chunk + got);
        std::fclose(f);
        setVocabulary(b.data(), (int64_t)b.size());
    }

    // db.setVocabulary(voc, false, 0): a fresh, empty database
    void setVocabulary(const void* vocab, int64_t bytes)
    {
        lvi_bow* fresh = nullptr;
        check(lvi_bow_create(kd_.get(), vocab, bytes, max_entries_, &fresh), "lvi_bow_create");
        lvi_bow_destroy(db_);
        db_ = fresh;
    }

    // loop_detector.cpp:12-40.  The keyframe's slot must stay in the store while it may be matched against.
    LoopResult addKeyFrame(const KeyFrame& cur_kf, bool flag_detect_loop)
    {
        LoopResult r;
        if (flag_detect_loop) r.loop_index = detectLoop(cur_kf, cur_kf.index, &r.ret);
        else addKeyFrameIntoVoc(cur_kf);
        if (r.loop_index != -1) {
            const KeyFrame* old_kf = getKeyFrame(r.loop_index);
            // the reference dereferences a NULL here when no keyframe has that index; with entry id == index one always has
            if (old_kf) r.connected = pnp_ ? findConnection(kd_, *pnp_, cur_kf, *old_kf, r.connection) : kd_.findConnectionFront(cur_kf, *old_kf, r.connection);
        }
        keyframelist.push_back(cur_kf);
        return r;
    }

    const KeyFrame* getKeyFrame(int index) const                    // :42-54
    {
        for (const KeyFrame& k : keyframelist)
            if (k.index == index) return &k;
        return nullptr;
    }

    // :56-139 without the DEBUG_IMAGE code
    int detectLoop(const KeyFrame& keyframe, int frame_index, std::vector<lvi_bow_result>* ret_out = nullptr)
    {
        need_db();
        // first query; then add this frame into database!
        lvi_bow_result ret[4];
        int32_t n = 0;
        check(lvi_bow_query(db_, keyframe.slot, 4, frame_index - 200, ret, &n), "lvi_bow_query");
        check(lvi_bow_add(db_, keyframe.slot, nullptr), "lvi_bow_add");
        if (ret_out) ret_out->assign(ret, ret + n);
        // a good match with its neighbour
        bool find_loop = false;
        if (n >= 1 && ret[0].score > 0.05)
            for (int i = 1; i < n; i++)
                if (ret[i].score > 0.015) find_loop = true;
        if (find_loop && frame_index > 50) {
            int min_index = -1;
            for (int i = 0; i < n; i++)
                if (min_index == -1 || (ret[i].entry_id < min_index && ret[i].score > 0.015)) min_index = ret[i].entry_id;
            return min_index;
        }
        return -1;
    }

    void addKeyFrameIntoVoc(const KeyFrame& keyframe)               // :141-154
    {
        need_db();
        check(lvi_bow_add(db_, keyframe.slot, nullptr), "lvi_bow_add");
    }

    std::list<KeyFrame> keyframelist;

private:
    void need_db() const { if (!db_) throw Error(LVI_ERR_STATE, "LoopDetector: loadVocabulary first"); }

    KeyFrameDescriber& kd_;
    int max_entries_;
    lvi_bow* db_ = nullptr;
    PnPRansac* pnp_ = nullptr;
};

}  // namespace lvi_host
