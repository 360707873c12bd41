// What keyframe_db.hip shares with loop_detect.hip: the resident state of a KeyFrameDatabase handle as the kernels see it, the handle itself, the
// checks of a query call and the launch of k_kfdb_query.  Internal to csrc/; the public interface is include/oslam_hip.h ("KeyFrameDatabase").
#pragma once
#include <mutex>
#include <vector>

#include "common.h"

namespace oslam {

// S = n_db * K slots, slot of (d, k) = d * K + k
struct KfdbState {
    int32_t* nwords;      // [S] words of the slot's vector; -1: not present
    uint32_t* serial;     // [S] add serial
    float* reloc;         // [S] reloc_score
    int32_t* covis;       // [S][OSLAM_KFDB_COVIS], -1 = no entry
    int32_t* chunks;      // [S][MC] chunk indices of the slot's words
    uint32_t* pool_ids;   // [n_chunks][OSLAM_KFDB_CHUNK]
    double* pool_vals;    // [n_chunks][OSLAM_KFDB_CHUNK]
    int n_db, K, MW, MC;
};

}  // namespace oslam

struct oslam_kfdb {
    int device = 0, P = 1;
    size_t lds = 0;
    oslam::KfdbState st{};
    oslam::DeviceBuffer nwords, serial, reloc, covis, chunks, pool_ids, pool_vals;
    // the host's side of the state: what the refusals are decided on, and the allocator
    std::vector<int32_t> h_nwords, h_chunks, free_chunks;
    std::vector<uint32_t> next_serial;
    long long n_chunks = 0, n_present = 0;
    hipStream_t stream = nullptr;
    oslam::StagePair io;
    std::mutex mu;
    ~oslam_kfdb() { if (stream) (void)hipStreamDestroy(stream); }
};

namespace oslam {

// the handle, the vocabulary's scoring type and the counts of a query call (sets the error)
int kfdb_check_query_call(const char* fn, const oslam_kfdb* h, const oslam_voc_t* voc, int n_queries, int n_words_total, int n_conn_total);
// the records of a host query call against the arrays they name: what the host entry points refuse as a whole before anything runs (sets the error)
int kfdb_check_queries(const char* fn, const oslam_kfdb* h, bool loop, int n_queries, const oslam_kfdb_query_t* queries, int n_words_total, const uint32_t* ids, int n_conn_total);
// One launch of k_kfdb_query over device arrays.  d_min_score NULL: a loop query's bound is its record's min_score.  Otherwise (loop queries only) each
// workgroup derives it from the connected scores (LoopClosing::DetectLoop, src/LoopClosing.cc:127-139), uses it and writes it to d_min_score[q].
int kfdb_launch_query(oslam_kfdb* h, bool loop, int n_queries, const oslam_kfdb_query_t* d_queries, int n_words_total, const uint32_t* d_ids, const double* d_vals,
                      int n_conn_total, const int32_t* d_conn, int32_t* d_cand, float* d_cand_acc, int32_t* d_n_cand, int32_t* d_diag, float* d_conn_score,
                      float* d_min_score, hipStream_t stream);

}  // namespace oslam
