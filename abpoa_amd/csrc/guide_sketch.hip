// Device half of the guide-tree read order (guide_order.h): the minimizer sketch of every read and the minimizer hits of every read pair.
//
// SKETCH.  The reference walks a read base by base with a ring of the last w k-mer hashes and a running minimum (src/abpoa_seed.c:84-223).  What it
// pushes depends only on a window of that walk, so every position can decide alone what it pushes:
//   * an EVENT is one turn of the reference's loop that reaches the ring: every position except, with both strands, one whose k-mer (over the last k
//     unambiguous bases) equals its own reverse complement -- those turns `continue` before the ring and before l moves;
//   * event e has l_e = events since the last ambiguous base and x_e = hash << 8 | k when l_e >= k, else "none" (all ones).  An ambiguous base is an
//     event with l = 0 and x = none: it clears l, not the ring;
//   * the reference's `min` after event e is the RIGHTMOST smallest x of events e-w+1 .. e (events before the read count as none): a new value takes
//     over on <=, and the rescan after the minimum left the ring keeps the last of equal values;
//   * with M' = that minimum after event e-1, event e pushes
//       - (first full window, l_e == w+k-1, M' not none) every other event of e-w+1 .. e-1 whose x equals M';
//       - (x_e <= M')                     M' itself when l_e >= w+k;
//       - (else, M' was event e-w)        M' itself when l_e >= w+k-1, and then, with M the new minimum of e-w+1 .. e, every other event of that
//                                         window whose x equals M, again when l_e >= w+k-1;
//   * the read ends with one more push of the running minimum, when it is not none.
// Only the pushed x values are kept (the guide tree reads nothing else), sorted ascending per read.  One workgroup walks one read in tiles of GT
// positions; what crosses a tile edge is the reference's own state: the last k-1 unambiguous bases (its k-mer registers), the last w events (its ring,
// and with it min and min_pos), the event count and the last ambiguous event (its l).  No read-length cap.
// The kernel runs twice: once counting the pushes of every read, once -- behind the host's prefix sum of the counts -- writing and sorting them.
//
// PAIRS.  One wavefront per read pair of a set: the lanes share out the distinct values of the shorter list and find each in the longer one by binary
// search; the hits of a value are the smaller of its two multiplicities (abpoa_seed.c:247-278 counts the same per distinct value over all reads).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <mutex>
#include <string.h>
#include <thread>
#include <vector>
#include "batch_stream.h"
#include "batch_types.h"
#include "guide_order.h"

namespace abpoa_hip {
namespace {

constexpr int GT = 256;            // threads of a sketch workgroup = positions of a tile
constexpr int EV_CARRY = 256;      // events kept from the tiles before (>= the largest w, 255)
constexpr int CB_CARRY = 32;       // unambiguous bases kept from the tiles before (>= the largest k - 1, 27)
constexpr int SORT_LDS = 2048;     // sketches of up to this many values are sorted in the LDS, longer ones in place
constexpr uint64_t NONE = ~0ull;

struct SketchArgs {
    const uint8_t *bases; const int64_t *read_off; const int32_t *read_len;
    int k, w, bits, n_codes, both; uint64_t mask;
    int32_t *count;                                  // count pass: pushes of every read
    const int64_t *mm_off; uint64_t *mm; int32_t *bad;      // write pass; *bad counts reads whose pushes differ from the count pass
};

__device__ inline uint64_t kmer_hash(uint64_t key, uint64_t mask) {      // the invertible 64-bit integer mix the reference takes from minimap2
    key = (~key + (key << 21)) & mask;
    key ^= key >> 24;
    key = (key + (key << 3) + (key << 8)) & mask;
    key ^= key >> 14;
    key = (key + (key << 2) + (key << 4)) & mask;
    key ^= key >> 28;
    key = (key + (key << 31)) & mask;
    return key;
}

__device__ inline int wave_scan_sum(int v, int lane) {
    for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(v, d, 64); if (lane >= d) v += t; }
    return v;
}
__device__ inline int wave_scan_max(int v, int lane) {
    for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(v, d, 64); if (lane >= d) v = max(v, t); }
    return v;
}
// exclusive prefix sum over the workgroup and the total; scr: GT / 64 ints that nothing else uses before the next barrier
__device__ inline int block_scan_sum(int v, int *scr, int &total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int inc = wave_scan_sum(v, lane);
    if (lane == 63) scr[wv] = inc;
    __syncthreads();
    int base = 0; total = 0;
    for (int i = 0; i < GT / 64; ++i) { if (i < wv) base += scr[i]; total += scr[i]; }
    return base + inc - v;
}
// inclusive prefix maximum over the workgroup and the maximum of all
__device__ inline int block_scan_max(int v, int *scr, int &all) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int inc = wave_scan_max(v, lane);
    if (lane == 63) scr[wv] = inc;
    __syncthreads();
    all = scr[0];
    for (int i = 1; i < GT / 64; ++i) { if (i <= wv) inc = max(inc, scr[i - 1]); all = max(all, scr[i]); }
    return inc;
}

// ascending sort of a[0..n) by the whole workgroup: the bitonic network for the next power of two in its all-ascending form (first step of a merge
// mirrored), where the missing tail counts as "none" and therefore never moves -- pairs that reach beyond n are skipped
template <class P>
__device__ inline void block_sort(P a, int n) {
    for (long long k2 = 2; k2 < 2ll * n; k2 <<= 1) {
        for (int i = threadIdx.x; i < n; i += GT) {
            const long long p = i ^ (k2 - 1);
            if (p > i && p < n) { const uint64_t u = a[i], v = a[p]; if (u > v) { a[i] = v; a[p] = u; } }
        }
        __syncthreads();
        for (long long j = k2 >> 2; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < n; i += GT) {
                const long long p = i ^ j;
                if (p > i && p < n) { const uint64_t u = a[i], v = a[p]; if (u > v) { a[i] = v; a[p] = u; } }
            }
            __syncthreads();
        }
    }
}

template <bool WRITE>
__global__ __launch_bounds__(GT) void guide_sketch_kernel(SketchArgs a) {
    __shared__ uint64_t ev[EV_CARRY + GT];       // x of the last EV_CARRY events before the tile, then of the tile's events
    __shared__ uint8_t cb[CB_CARRY + GT];        // the last CB_CARRY unambiguous bases before the tile, then the tile's
    __shared__ int scr[3][GT / 64];
    __shared__ int n_out;
    __shared__ uint64_t sorted[WRITE ? SORT_LDS : 1];
    const int tid = threadIdx.x, r = blockIdx.x;
    const int len = a.read_len[r], k = a.k, w = a.w;
    const uint8_t *seq = a.bases + a.read_off[r];
    const int64_t off = WRITE ? a.mm_off[r] : 0;
    const int cap = WRITE ? (int)(a.mm_off[r + 1] - off) : 0;
    int my_pushes = 0;
    auto push = [&](uint64_t x, int times) {
        if (!WRITE) { my_pushes += times; return; }
        const int at = atomicAdd(&n_out, times);
        for (int q = 0; q < times; ++q) if (at + q < cap) a.mm[off + at + q] = x;
    };
    ev[tid] = NONE;
    if (tid < CB_CARRY) cb[tid] = 0;
    if (tid == 0) n_out = 0;
    __syncthreads();
    int n_cb = 0, n_ev = 0, last_amb = -1;       // unambiguous bases / events before the tile; the last ambiguous event (uniform over the workgroup)
    for (int t0 = 0; t0 < len; t0 += GT) {
        const int pos = t0 + tid;
        const bool in = pos < len;
        const int c = in ? seq[pos] : 0;
        const bool amb = in && c >= a.n_codes, base = in && c < a.n_codes;
        int n1, n2, amb_all;
        const int ci = block_scan_sum(base ? 1 : 0, scr[0], n1);
        if (base) cb[CB_CARRY + ci] = (uint8_t)c;
        __syncthreads();
        // the k-mer over the last k unambiguous bases, once there are k of them
        uint64_t key = 0; bool have = false, skip = false;
        if (base && n_cb + ci + 1 >= k) {
            uint64_t fw = 0, rv = 0;
            const uint8_t *b = cb + CB_CARRY + ci - (k - 1);
            for (int t = 0; t < k; ++t) {
                fw = (fw << a.bits | b[t]) & a.mask;
                if (a.both) rv = (rv >> 2) | ((uint64_t)(3 ^ b[t]) << (2 * (k - 1)));
            }
            have = true; key = fw;
            if (a.both) { skip = fw == rv; key = fw < rv ? fw : rv; }
        }
        const bool event = in && !skip;
        const int ei = block_scan_sum(event ? 1 : 0, scr[1], n2);
        const int e = n_ev + ei;
        const int la = max(last_amb, block_scan_max(amb ? e : -1, scr[2], amb_all));
        const int l = amb ? 0 : e - la;
        const uint64_t x = (event && have && l >= k) ? (kmer_hash(key, a.mask) << 8 | (uint64_t)k) : NONE;
        if (event) ev[EV_CARRY + ei] = x;
        __syncthreads();
        if (event) {
            const uint64_t *win = ev + EV_CARRY + ei;      // win[-d]: event e - d
            uint64_t xm = NONE; int dm = w;                  // the minimum after event e - 1: the rightmost smallest of e-w .. e-1
            for (int d = w; d >= 1; --d) { const uint64_t v = win[-d]; if (v <= xm) { xm = v; dm = d; } }
            if (l == w + k - 1 && xm != NONE) {
                int ties = 0;
                for (int d = w - 1; d >= 1; --d) ties += (win[-d] == xm && d != dm);
                if (ties) push(xm, ties);
            }
            if (x <= xm) {
                if (l >= w + k && xm != NONE) push(xm, 1);
            } else if (dm == w) {
                if (l >= w + k - 1 && xm != NONE) push(xm, 1);
                if (l >= w + k - 1) {
                    uint64_t m2 = NONE; int same = 0;
                    for (int d = w - 1; d >= 0; --d) { const uint64_t v = win[-d]; if (v < m2) { m2 = v; same = 1; } else if (v == m2) ++same; }
                    if (m2 != NONE && same > 1) push(m2, same - 1);
                }
            }
        }
        __syncthreads();
        // what the next tile needs of this one: the ring and the k-mer registers
        const uint64_t keep_ev = ev[tid + n2];
        const uint8_t keep_cb = tid < CB_CARRY ? cb[tid + n1] : 0;
        __syncthreads();
        ev[tid] = keep_ev;
        if (tid < CB_CARRY) cb[tid] = keep_cb;
        __syncthreads();
        n_cb += n1; n_ev += n2; last_amb = max(last_amb, amb_all);
    }
    if (tid == 0) {      // the running minimum once more at the end of the read
        uint64_t xm = NONE;
        for (int d = w; d >= 1; --d) { const uint64_t v = ev[EV_CARRY - d]; if (v <= xm) xm = v; }
        if (xm != NONE) push(xm, 1);
    }
    if (!WRITE) {
        int total;
        (void)block_scan_sum(my_pushes, scr[0], total);
        if (tid == 0) a.count[r] = total;
        return;
    }
    __threadfence_block();
    __syncthreads();
    if (n_out != cap) { if (tid == 0) atomicAdd(a.bad, 1); return; }      // (uniform: n_out is read behind the barrier)
    uint64_t *mine = a.mm + off;
    if (cap <= SORT_LDS) {
        for (int i = tid; i < cap; i += GT) sorted[i] = mine[i];
        __syncthreads();
        block_sort(sorted, cap);
        for (int i = tid; i < cap; i += GT) mine[i] = sorted[i];
    } else {
        block_sort(mine, cap);
    }
}

struct PairArgs { const uint64_t *mm; const int64_t *mm_off, *set_read0, *set_hit0; int32_t *hit; };

__device__ inline int first_not_below(const uint64_t *b, int n, uint64_t x) {
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (b[mid] < x) lo = mid + 1; else hi = mid; }
    return lo;
}

// grid: x = read-set, y = a share of the set's pairs; one wavefront per pair (i > j), entry i(i+1)/2 + j of the set's matrix
__global__ __launch_bounds__(256) void guide_pair_kernel(PairArgs a) {
    const int s = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t r0 = a.set_read0[s], n = a.set_read0[s + 1] - r0, n_pairs = n * (n - 1) / 2;
    int32_t *hit = a.hit + a.set_hit0[s];
    if (blockIdx.y == 0)
        for (int64_t r = threadIdx.x; r < n; r += 256) hit[r * (r + 1) / 2 + r] = (int32_t)(a.mm_off[r0 + r + 1] - a.mm_off[r0 + r]);
    for (int64_t p = (int64_t)blockIdx.y * 4 + wv; p < n_pairs; p += (int64_t)gridDim.y * 4) {
        int64_t i = (int64_t)((1.0 + sqrt(1.0 + 8.0 * (double)p)) * 0.5);
        while (i * (i - 1) / 2 > p) --i;
        while ((i + 1) * i / 2 <= p) ++i;
        const int64_t j = p - i * (i - 1) / 2;
        const uint64_t *A = a.mm + a.mm_off[r0 + i], *B = a.mm + a.mm_off[r0 + j];
        int na = (int)(a.mm_off[r0 + i + 1] - a.mm_off[r0 + i]), nb = (int)(a.mm_off[r0 + j + 1] - a.mm_off[r0 + j]);
        if (na > nb) { const uint64_t *t = A; A = B; B = t; const int tn = na; na = nb; nb = tn; }
        int sum = 0;
        for (int q = lane; q < na; q += 64) {
            const uint64_t x = A[q];
            if (q > 0 && A[q - 1] == x) continue;      // a value is counted where it first stands
            int ca = 1; while (q + ca < na && A[q + ca] == x) ++ca;
            const int lb = first_not_below(B, nb, x);
            int cbn = 0; while (lb + cbn < nb && B[lb + cbn] == x) ++cbn;
            sum += min(ca, cbn);
        }
        for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
        if (lane == 0) hit[i * (i + 1) / 2 + j] = sum;
    }
}

#define GUIDE_HIP(call, code) do { const hipError_t e_ = (call); if (e_ != hipSuccess) { set_err("guide order: %s: %s", #call, hipGetErrorString(e_)); return code; } } while (0)

// A pre-pass queue and its pools, kept between calls (abpoa_hip_trim releases them): a stream, the events around the kernels, two device pools
// (inputs / tables / hit matrices, and the sketch values, whose size is known only after the count pass) and one pinned staging buffer.
// One pre-pass at a time per queue: its mutex is held for a whole call.
struct Pool {
    uint8_t *p = nullptr; size_t cap = 0; bool pinned = false;
    int need(size_t n) {
        if (n <= cap) return 0;
        release();
        n += n / 4 + 256;
        const hipError_t e = pinned ? hipHostMalloc((void **)&p, n, hipHostMallocDefault) : hipMalloc((void **)&p, n);
        if (e != hipSuccess) { p = nullptr; (void)hipGetLastError(); return ABPOA_HIP_ENOMEM; }
        cap = n; return 0;
    }
    void release() { if (p) (void)(pinned ? hipHostFree(p) : hipFree(p)); p = nullptr; cap = 0; }
};
struct GuideQueue {
    std::mutex mu; int device = -1; hipStream_t st = nullptr; hipEvent_t ev[5] = {}; Pool dev, dev_mm, host;
    void release() {      // (the caller has made `device` the current one)
        if (st) (void)hipStreamSynchronize(st);
        dev.release(); dev_mm.release(); host.release();
        for (hipEvent_t &e : ev) { if (e) (void)hipEventDestroy(e); e = nullptr; }
        if (st) (void)hipStreamDestroy(st);
        st = nullptr; device = -1;
    }
    int open(int d) {
        if (device == d) return 0;
        if (device >= 0) { GUIDE_HIP(hipSetDevice(device), ABPOA_HIP_ENODEV); release(); }
        GUIDE_HIP(hipSetDevice(d), ABPOA_HIP_ENODEV);
        host.pinned = true;
        hipError_t err = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
        for (hipEvent_t &e : ev) if (err == hipSuccess) err = hipEventCreate(&e);
        if (err != hipSuccess) {      // nothing half-built stays behind: the next call starts afresh
            release();
            set_err("guide order: stream / events on device %d: %s", d, hipGetErrorString(err));
            return ABPOA_HIP_ENODEV;
        }
        device = d;
        return 0;
    }
};
GuideQueue g_queue[GUIDE_QUEUES];      // one per device queue of the batch entry (a context has its own): pre-passes of different callers run side by side
// byte offsets of the pieces of a pool
struct Carve { size_t o = 0; size_t take(size_t bytes) { const size_t at = o; o = (o + bytes + 255) & ~(size_t)255; return at; } };
// fn(t) for t in [0, n_thr) on that many host threads
template <class F> void on_threads(int n_thr, F fn) {
    std::vector<std::thread> th;
    for (int t = 1; t < n_thr; ++t) th.emplace_back(fn, t);
    fn(0);
    for (auto &t : th) t.join();
}

}  // namespace

void release_guide_queues() {
    int cur = -1; (void)hipGetDevice(&cur);
    for (GuideQueue &Q : g_queue) {
        std::lock_guard<std::mutex> lk(Q.mu);
        if (Q.device < 0) continue;
        (void)hipSetDevice(Q.device);
        Q.release();
    }
    if (cur >= 0) (void)hipSetDevice(cur);
}

int guide_tile_length() { return GT; }

int guide_prepass(const GuideParams &gp, int n_sets, const abpoa_hip_readset_t *sets, int device, int slot, bool want_mm, GuideResult &R) {
    const auto t_begin = std::chrono::steady_clock::now();
    R = GuideResult();
    R.set_read0.assign(n_sets + 1, 0); R.set_hit0.assign(n_sets + 1, 0);
    int max_reads = 0;
    for (int s = 0; s < n_sets; ++s) {
        const int64_t n = sets[s].n_reads;
        R.set_read0[s + 1] = R.set_read0[s] + n; R.set_hit0[s + 1] = R.set_hit0[s] + n * (n + 1) / 2;
        max_reads = std::max<int64_t>(max_reads, n);
    }
    const int64_t n_reads = R.set_read0[n_sets], n_hit = R.set_hit0[n_sets];
    R.mm_off.assign(n_reads + 1, 0);
    R.order.resize(n_reads); R.hit.assign(n_hit, 0);
    if (n_reads == 0) return ABPOA_HIP_OK;
    if (n_reads > 0x7fffffff) { set_err("guide order: %lld reads in one call", (long long)n_reads); return ABPOA_HIP_EINVAL; }
    // the reads of all sets, end to end
    std::vector<int64_t> read_off(n_reads + 1, 0);
    std::vector<const uint8_t *> src(n_reads);
    for (int s = 0; s < n_sets; ++s)
        for (int r = 0; r < sets[s].n_reads; ++r) {
            const int64_t g = R.set_read0[s] + r;
            src[g] = sets[s].seqs[r]; read_off[g + 1] = read_off[g] + sets[s].lens[r];
        }
    const int64_t n_bases = read_off[n_reads];
    const int host_thr = std::max(1, std::min(8, effective_host_cores()));
    if (device < 0) device = engine_device();
    if (slot < 0 || slot >= GUIDE_QUEUES) { set_err("guide order: queue %d out of range", slot); return ABPOA_HIP_EINVAL; }
    GuideQueue &Q = g_queue[slot];
    std::lock_guard<std::mutex> lk(Q.mu);
    GUIDE_HIP(hipSetDevice(device), ABPOA_HIP_ENODEV);
    if (const int rc = Q.open(device)) return rc;
    // uploaded in one piece: read offsets, read lengths, the sets' first read / first matrix entry, the bases; behind them, device only: counts, the
    // sketch offsets, the flag, the hit matrices.  The pinned buffer holds the upload, then the counts and the hit matrices on their way back.
    Carve c;
    const size_t o_off = c.take(8 * (n_reads + 1)), o_len = c.take(4 * n_reads), o_sr0 = c.take(8 * (n_sets + 1)), o_sh0 = c.take(8 * (n_sets + 1)),
                 o_bases = c.take(n_bases + 8), up_bytes = c.o, o_cnt = c.take(4 * n_reads), o_mmoff = c.take(8 * (n_reads + 1)), o_bad = c.take(4),
                 o_hit = c.take(4 * n_hit), dev_bytes = c.o;
    if (Q.dev.need(dev_bytes) || Q.host.need(dev_bytes)) { set_err("guide order: memory for %lld reads", (long long)n_reads); return ABPOA_HIP_ENOMEM; }
    uint8_t *h = Q.host.p, *d = Q.dev.p;
    memcpy(h + o_off, read_off.data(), 8 * (n_reads + 1));
    memcpy(h + o_sr0, R.set_read0.data(), 8 * (n_sets + 1)); memcpy(h + o_sh0, R.set_hit0.data(), 8 * (n_sets + 1));
    {
        int32_t *len = (int32_t *)(h + o_len);
        const int n_thr = (int)std::max<int64_t>(1, std::min<int64_t>(host_thr, n_bases >> 20));
        on_threads(n_thr, [&](int t) {
            for (int64_t g = n_reads * t / n_thr, g1 = n_reads * (t + 1) / n_thr; g < g1; ++g) {
                len[g] = (int32_t)(read_off[g + 1] - read_off[g]);
                memcpy(h + o_bases + read_off[g], src[g], (size_t)len[g]);
            }
        });
    }
    GUIDE_HIP(hipMemcpyAsync(d, h, up_bytes, hipMemcpyHostToDevice, Q.st), ABPOA_HIP_ELAUNCH);
    GUIDE_HIP(hipMemsetAsync(d + o_bad, 0, 4, Q.st), ABPOA_HIP_ELAUNCH);
    SketchArgs sa;
    memset(&sa, 0, sizeof(sa));
    sa.bases = d + o_bases; sa.read_off = (const int64_t *)(d + o_off); sa.read_len = (const int32_t *)(d + o_len);
    sa.k = gp.k; sa.w = gp.w; sa.bits = gp.aa ? 5 : 2; sa.n_codes = gp.aa ? 26 : 4; sa.both = gp.both_strands ? 1 : 0;
    sa.mask = (1ull << (sa.bits * gp.k)) - 1;
    sa.count = (int32_t *)(d + o_cnt); sa.bad = (int32_t *)(d + o_bad);
    GUIDE_HIP(hipEventRecord(Q.ev[0], Q.st), ABPOA_HIP_ELAUNCH);
    hipLaunchKernelGGL(guide_sketch_kernel<false>, dim3((unsigned)n_reads), dim3(GT), 0, Q.st, sa);
    GUIDE_HIP(hipGetLastError(), ABPOA_HIP_ELAUNCH);
    GUIDE_HIP(hipEventRecord(Q.ev[1], Q.st), ABPOA_HIP_ELAUNCH);
    GUIDE_HIP(hipMemcpyAsync(h + o_cnt, d + o_cnt, 4 * n_reads, hipMemcpyDeviceToHost, Q.st), ABPOA_HIP_ELAUNCH);
    GUIDE_HIP(hipStreamSynchronize(Q.st), ABPOA_HIP_ELAUNCH);
    const int32_t *cnt = (const int32_t *)(h + o_cnt);
    for (int64_t g = 0; g < n_reads; ++g) R.mm_off[g + 1] = R.mm_off[g] + cnt[g];
    const int64_t n_mm = R.mm_off[n_reads];
    if (Q.dev_mm.need(8 * (size_t)n_mm + 8)) { set_err("guide order: device memory for %lld minimizers", (long long)n_mm); return ABPOA_HIP_ENOMEM; }
    memcpy(h + o_mmoff, R.mm_off.data(), 8 * (n_reads + 1));
    GUIDE_HIP(hipMemcpyAsync(d + o_mmoff, h + o_mmoff, 8 * (n_reads + 1), hipMemcpyHostToDevice, Q.st), ABPOA_HIP_ELAUNCH);
    sa.mm_off = (const int64_t *)(d + o_mmoff); sa.mm = (uint64_t *)Q.dev_mm.p;
    GUIDE_HIP(hipEventRecord(Q.ev[2], Q.st), ABPOA_HIP_ELAUNCH);
    hipLaunchKernelGGL(guide_sketch_kernel<true>, dim3((unsigned)n_reads), dim3(GT), 0, Q.st, sa);
    GUIDE_HIP(hipGetLastError(), ABPOA_HIP_ELAUNCH);
    GUIDE_HIP(hipEventRecord(Q.ev[3], Q.st), ABPOA_HIP_ELAUNCH);
    PairArgs pa{sa.mm, sa.mm_off, (const int64_t *)(d + o_sr0), (const int64_t *)(d + o_sh0), (int32_t *)(d + o_hit)};
    const int64_t max_pairs = (int64_t)max_reads * (max_reads - 1) / 2;
    const unsigned shares = (unsigned)std::max<int64_t>(1, std::min<int64_t>(64, (max_pairs + 3) / 4));
    hipLaunchKernelGGL(guide_pair_kernel, dim3((unsigned)n_sets, shares), dim3(256), 0, Q.st, pa);
    GUIDE_HIP(hipGetLastError(), ABPOA_HIP_ELAUNCH);
    GUIDE_HIP(hipEventRecord(Q.ev[4], Q.st), ABPOA_HIP_ELAUNCH);
    GUIDE_HIP(hipMemcpyAsync(h + o_bad, d + o_bad, dev_bytes - o_bad, hipMemcpyDeviceToHost, Q.st), ABPOA_HIP_ELAUNCH);      // the flag and the hit matrices
    if (want_mm) { R.mm.resize(n_mm); GUIDE_HIP(hipMemcpyAsync(R.mm.data(), Q.dev_mm.p, 8 * (size_t)n_mm, hipMemcpyDeviceToHost, Q.st), ABPOA_HIP_ELAUNCH); }
    GUIDE_HIP(hipStreamSynchronize(Q.st), ABPOA_HIP_ELAUNCH);
    const int32_t bad = *(const int32_t *)(h + o_bad);
    if (bad) { set_err("guide order: the sketch of %d reads changed between its two passes", bad); return ABPOA_HIP_ELAUNCH; }
    float ms = 0;
    GUIDE_HIP(hipEventElapsedTime(&ms, Q.ev[0], Q.ev[1]), ABPOA_HIP_ELAUNCH); R.sketch_ms = ms;
    GUIDE_HIP(hipEventElapsedTime(&ms, Q.ev[2], Q.ev[3]), ABPOA_HIP_ELAUNCH); R.sketch_ms += ms;
    GUIDE_HIP(hipEventElapsedTime(&ms, Q.ev[3], Q.ev[4]), ABPOA_HIP_ELAUNCH); R.pair_ms = ms;
    memcpy(R.hit.data(), h + o_hit, 4 * (size_t)n_hit);
    {
        const int n_thr = (int)std::max<int64_t>(1, std::min<int64_t>(host_thr, n_hit >> 16));
        on_threads(n_thr, [&](int t) {
            for (int s = (int)((int64_t)n_sets * t / n_thr), s1 = (int)((int64_t)n_sets * (t + 1) / n_thr); s < s1; ++s)
                guide_greedy_order(sets[s].n_reads, R.hit.data() + R.set_hit0[s], R.order.data() + R.set_read0[s]);
        });
    }
    R.total_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
    return ABPOA_HIP_OK;
}

}  // namespace abpoa_hip
