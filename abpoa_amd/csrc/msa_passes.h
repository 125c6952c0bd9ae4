// The decisions of the batch entry above run_msa_device (msa_hip.cpp runs them): which pass of the node-slot ladder a read-set runs in, how a pass is cut into
// chunks, what the process remembers about a job shape, how sets are dealt to device queues.  No HIP runtime call: tests/pass_ladder.cpp drives all of it on
// the CPU with a scripted runner.
#pragma once
#include <functional>
#include <map>
#include <mutex>
#include <vector>
#include "msa_device.h"

namespace abpoa_hip {

// ---- the pass ladder
// Pass p gives every set PASS_NODE_FACTOR[p] x its longest read in graph-node slots (5 %-error reads need ~2.5x); the sets that outgrow a pass are redone in
// the next one.  (The last pass bounds nothing: a set's graph cannot have more nodes than its reads have bases, and run_msa_device takes the smaller of the two
// -- so node slots are never what sends a set to the host driver; round-4 fuzzing: 22 of 813 sets, all for that reason -- protein sets at 15 % error.)
constexpr int N_PASSES = 4;
constexpr double PASS_NODE_FACTOR[N_PASSES] = {3.0, 4.5, 6.0, 4096.0};

// What the process learned about jobs of one shape (job_shape_key): when most sets of the last such job outgrew the 3x pass and a later pass ran in one piece,
// the next one starts there (noisy long reads: 50 x 10 kb at 15 % error grow to 3.9x; the doomed first pass is ~3 % of such a job).  Results do not depend on
// it.  ABPOA_HIP_NO_PASS_HINT=1: always start at 3x.
class PassHints {
  public:
    bool find(int key, int *pass);
    void set(int key, int pass);
    void erase(int key);
  private:
    std::mutex mu_;
    std::map<int, int> start_;
};
// shape of a job: longest read by power of two, reads per set
int job_shape_key(const abpoa_hip_readset_t *sets, const std::vector<int> &idx);

// One chunk of a pass on the device.  left: the sets that left it, SetFallback.set counting inside the chunk; n_fit_3x / n_done: finished sets that would also
// have fitted the 3x estimate / finished sets.  rc: ABPOA_HIP_ENOMEM -- the chunk does not fit the device; EINVAL -- not a job for the device driver.
struct ChunkOut { int rc = ABPOA_HIP_OK; std::vector<SetFallback> left; int n_fit_3x = 0, n_done = 0; };
using ChunkRunner = std::function<ChunkOut(const std::vector<int> &chunk, int pass, double node_factor)>;
// how many of the open sets the device holds at once (msa_device_resident_sets; 0: no preference)
using ResidentSets = std::function<int(const std::vector<int> &open)>;

// left: the sets for the host driver; why: set -> reason it left its last pass (a set in `left` without one: its pass did not fit or was not the device's);
// device_ok false: the device path gave up on the job, finished results stay
struct LadderOut { int rc = ABPOA_HIP_OK; bool device_ok = true; std::vector<int> left; std::map<int, HostReason> why; };

// The passes over the sets `idx` on one device queue.  The rules:
//   start       ABPOA_HIP_FIRST_PASS in 1..3, then the hint stored for `key` (ABPOA_HIP_NO_PASS_HINT=1: not read)
//   chunks      a pass runs all its open sets at once, capped by `resident` and then by ABPOA_HIP_PASS_SETS
//   ENOMEM      a chunk of more than one set is halved, (nb + 1) / 2, and retried at the same position; the pass counts as halved.  On a single set, and on
//               EINVAL, the ladder gives up (device_ok false, rc OK): `left` lists the leftovers of the chunks already done in this pass, every set from
//               the failing position on, the deferred sets, the hopeless ones
//   other rc    ends the ladder at once with that rc
//   edge slots  a set with a node out of edge slots skips the passes in between (deferred) and rejoins, in index order, in the last pass -- which has an edge
//               slot per read at every node (msa_device_plan.cpp `roomy`); with only such sets open the next pass is the last; marked again there, it is
//               the host driver's (hopeless)
//   learning    0 < pass < last, the previous pass left at least half of its sets, this one fewer than half, in the pieces first tried, device ok:
//               jobs of this shape start here next time
//   forgetting  the first pass run started above 0 and more than half of the sets it finished would have fitted 3x (a cleaner job of the same shape):
//               more graph and arena memory for nothing otherwise, for as long as the process lives
LadderOut run_pass_ladder(const std::vector<int> &idx, int key, PassHints &hints, const ChunkRunner &run, const ResidentSets &resident);

// adds the ladder's leftovers to hist[MSA_HOST_REASONS] (abpoa_hip_get_host_reasons): the reason of the last pass each was in, HOST_WHY_JOB without one
void count_host_reasons(const LadderOut &R, int32_t *hist);

// ---- device queues
// ABPOA_GPU_DEVICES: "all", or a comma list of device ordinals (a repeated ordinal = two queues on that device); unset or nothing
// usable = the device the engine was initialised on.  At most MSA_DEVICE_SLOTS entries.
std::vector<int> parse_device_list(const char *text, int n_devices, int engine_device);

// Batches for the device queues: sets sorted by estimated DP cost (sum of read lengths x reads), heaviest first, dealt round-robin so that every batch holds the
// same mix; the queues pull batches from one shared counter (a fast device simply takes more of them).
// Banded global / extension jobs: the read-sets with ragged read ends (msa_device.h msa_device_set_is_ragged) of a batch become a batch of their own -- the
// uniform sets then keep the all-rounds kernel (narrow bands: one launch for all rounds, ~1.4x the lock-step launches' rate on 1 kb reads), which a job with a
// single ragged set would lose for all of them.  (ABPOA_HIP_NO_RAGGED_SPLIT=1: one batch, as before round 5.)
void split_ragged(std::vector<std::vector<int>> &batches, const abpoa_hip_scoring_t *sc, const abpoa_hip_readset_t *sets);
std::vector<std::vector<int>> deal_batches(const abpoa_hip_scoring_t *sc, const abpoa_hip_readset_t *sets, int n_sets, int n_q);

}  // namespace abpoa_hip
