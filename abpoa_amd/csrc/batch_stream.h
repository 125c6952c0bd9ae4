// BatchStream: one HIP stream + its pinned staging / HBM pools.  A batch of alignments is
//   prepare(shapes)  -> layout computed, pools grown, host slots handed out (pinned memory, zero copy)
//   fill slots       -> caller writes each problem straight into its slot (any thread)
//   run()            -> one H2D copy, one DP-kernel launch, one D2H copy, synchronise; overflowed arenas are retried
//                       (every size, offset and routing answer it uses: batch_plan.h, host arithmetic tested without a GPU)
//   rec()/cigar()    -> results read in place from pinned memory
// Several BatchStreams may be driven concurrently from different host threads (one per read-set group);
// the flat C API (abpoa_hip_align_batch) uses a process-wide default instance under a mutex.
#pragma once
#include <stdint.h>
#include <vector>
#include <hip/hip_runtime.h>
#include "engine.h"
#include "batch_types.h"
#include "batch_plan.h"
#include "../../include/abpoa_hip.h"

namespace abpoa_hip {

// (the BS_* flags of prepare(): batch_plan.h)

struct Blob {                   // device buffer with optional pinned host mirror; grow-only
    uint8_t *dev = nullptr, *host = nullptr; size_t cap = 0; bool mirrored;
    explicit Blob(bool m) : mirrored(m) {}
    int reserve(size_t n);
    void release();
};

struct StreamStats { int64_t n_launches = 0, n_alignments = 0, n_cells = 0, algo_bytes = 0, n_need_scores = 0; double kernel_ms = 0, h2d_ms = 0, d2h_ms = 0, tail_ms = 0, rounds_ms = 0;
        int64_t rounds_launches = 0, rounds_algo_bytes = 0; };

class BatchStream {
  public:
    BatchStream() : in_(true), out_(true), planes_(false) {}
    ~BatchStream() { close(); }
    int open(int device);
    void close();
    int prepare(const abpoa_hip_scoring_t *sc, int n, const BatchShape *shapes, unsigned flags);
    ProblemSlots slots(int i) const { return problem_slots(I_, O_, desc_[i], in_.host, out_.host); }
    int run();
    int n() const { return n_; }
    const AlnOut &rec(int i) const { return recs_[i]; }
    const AlnDesc &desc(int i) const { return desc_[i]; }
    const uint64_t *cigar(int i) const { return (const uint64_t *)(out_.host + O_.cig) + desc_[i].cigar_off; }
    const int32_t *left(int i) const { return (const int32_t *)(out_.host + O_.left) + desc_[i].row0; }
    const int32_t *right(int i) const { return (const int32_t *)(out_.host + O_.right) + desc_[i].row0; }
    int fetch_trace(int i, abpoa_hip_trace_t *T);   // after run(), BS_TRACE only
    StreamStats take_stats() { StreamStats s = stats_; stats_ = StreamStats(); return s; }

  private:
    bool open_ = false; int device_ = -1;
    hipStream_t stream_ = nullptr; hipEvent_t ev_[5] = {};
    Blob in_, out_, planes_;
    abpoa_hip_scoring_t sc_{}; std::vector<int32_t> mat_;
    unsigned flags_ = 0; int n_ = 0, P_ = 1;
    // the stages of a pass of run(): what it uploads (first pass / retry / kept band), and what it keeps of the records that came back
    struct Pass { std::vector<int> todo; std::vector<AlnDesc> descs; DevBatch b; int n_fast = 0; bool first = true, dir = false; };
    int upload_pass(const Pass &ps, std::vector<int32_t> &saved_lr);
    int collect_pass(Pass &ps);
    std::vector<AlnDesc> desc_; std::vector<AlnOut> recs_; std::vector<ArenaCells> cells_;
    std::vector<std::vector<uint8_t>> trace_arena_;     // BS_TRACE: arena of every finished alignment, copied out before a retry pass re-uses the device arenas
    PoolTotals tot_{}; InLayout I_{}; OutLayout O_{};      // pool sizes and the byte offsets of the pools in in_ / out_ (batch_plan.h)
    StreamStats stats_;
};

void set_err(const char *fmt, ...);
const char *thread_last_error();      // the last message set_err formatted on the calling thread ("" if none since clear_thread_error)
void clear_thread_error();
int engine_device();            // device the process is bound to, or -1
int device_cu_count(int device);      // compute units of the device (< 0: the calling thread's current one); 256 when the runtime cannot tell
void add_global_stats(const StreamStats &s);

}  // namespace abpoa_hip
