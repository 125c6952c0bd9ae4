// GFA output of the device-resident read-set driver (poa_device.h GfaDev): the graph of every set in the order the reference prints it
// (abpoa_generate_gfa, src/abpoa_output.c:168-268), extracted from the graphs in HBM after the last round, in two phases like the MSA output:
//     poa_gfa_walk_kernel   the reference's FIFO Kahn walk -> walk order, segment and link counts per set
//     (host: the sets' segment / link / path pools laid out back to back, GfaDev.off)
//     poa_gfa_fill_kernel   segments, links and one path per read into those pools
// Plain vector loads and stores throughout.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "poa_device.h"
#include "poa_bodies.h"
#include "device_codes.h"

namespace abpoa_hip {

extern __shared__ int gfa_lds[];               // walk kernel, LDS tables: [cap] in-degree counters, [cap] queue
namespace {
// the wave's table accesses in program order (one wavefront per read-set: no barrier needed); global tables: loads and stores acknowledged
template <bool L> __device__ __forceinline__ void gfa_fence() {
    if (L) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ long long ld_fresh64(const int64_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned long long ld_fresh64u(const uint64_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The walk: pops one node at a time; the popped node's out-edges are handled a lane each (64 at a time: only the source can have more), the in-degree counters
// decremented, and the successors that reach zero appended in edge order through a prefix sum over the lanes.  A node has no two edges to the same target, so no
// two lanes touch one counter.  L: counters and queue in LDS (stride cap); else the counters in the set's scratch slice and the queue in the walk pool itself.
// Returns true when the sink was the n-th node popped -- the walk order is then queue[1 .. n - 2].
template <bool L>
__device__ __forceinline__ bool gfa_walk_body(const PoaDev &p, const PoaSet &S, const int n, const int cap, int32_t *walk) {
    const int lane = threadIdx.x;
    const int64_t N0 = S.node0;
    int32_t *cnt_g = p.scratch + S.scratch0;           // (4 * node_cap + ... entries: the order / rank walks' tables live there too)
    int32_t *q_g = walk;                              // global queue: node_cap + 1 entries, position 0 = the source
    for (int u = lane; u < n; u += 64) { const int d = p.nd_nin[N0 + u]; if (L) gfa_lds[u] = d; else cnt_g[u] = d; }
    if (lane == 0) { if (L) gfa_lds[cap] = 0; else q_g[0] = 0; }
    gfa_fence<L>();
    int head = 0, tail = 1;
    while (head < tail) {
        const int cur = uni(L ? gfa_lds[cap + head] : ld_fresh(q_g + head));
        ++head;
        if (cur == 1) return head == n;
        if (cur < 0 || cur >= n) return false;
        const int no = uni((int)p.nd_nout[N0 + cur]);
        for (int e0 = 0; e0 < no; e0 += 64) {
            const int e = e0 + lane;
            int v = -1, push = 0;
            if (e < no) {
                v = out_slot(p, S, N0 + cur, e);
                if (v >= 0 && v < n) {
                    if (L) { const int d = gfa_lds[v] - 1; gfa_lds[v] = d; push = d == 0; }
                    else push = atomicSub(cnt_g + v, 1) == 1;
                }
            }
            if (__ballot(e < no && (v < 0 || v >= n))) return false;      // (not a node of this graph)
            const int incl = wave_scan_add(push), all = __builtin_amdgcn_readlane(incl, 63);
            if (tail + all > n) return false;
            if (push) { if (L) gfa_lds[cap + tail + incl - 1] = v; else q_g[tail + incl - 1] = v; }
            tail += all;
            gfa_fence<L>();
        }
    }
    return false;
}
}  // namespace

__global__ void __launch_bounds__(64) poa_gfa_walk_kernel(const PoaDev p, const GfaDev g) {
    const int s = blockIdx.x, lane = threadIdx.x;
    if (s >= p.n_sets) return;
    const PoaSet S = p.sets[s];
    PoaState *st = p.state + s;
    int32_t *cnt = g.cnt + 3 * (int64_t)s;
    const int n = uni(st->n_nodes);
    if (uni(st->status) != POA_ST_OK || n <= 2 || n > S.node_cap + 1) { if (lane < 3) cnt[lane] = 0; return; }
    const int64_t N0 = S.node0;
    int32_t *walk = g.walk + N0;
    const bool in_lds = n <= g.lds_cap;
    const bool ok = in_lds ? gfa_walk_body<true>(p, S, n, g.lds_cap, walk) : gfa_walk_body<false>(p, S, n, 0, walk);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    if (!ok) {      // (the graph is not what the fuse phase should have left: the host driver redoes the set, as after a failed rank walk)
        if (lane == 0) { st->status = POA_ST_FALLBACK; st->reason = POA_WHY_NONE; }
        if (lane < 3) cnt[lane] = 0;
        return;
    }
    // walk position i (0-based, the source left out) -> walk[i]; the global queue holds the source at 0: shift by one, front to back, 64 at a time
    if (in_lds) for (int i = lane; i < n - 2; i += 64) walk[i] = gfa_lds[g.lds_cap + 1 + i];
    else for (int i0 = 0; i0 < n - 2; i0 += 64) {
        const int i = i0 + lane; int v = 0;
        if (i < n - 2) v = ld_fresh(walk + i + 1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); __builtin_amdgcn_wave_barrier();
        if (i < n - 2) walk[i] = v;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); __builtin_amdgcn_wave_barrier();
    }
    // links: in-edges of the inner nodes, less the source's out-edges (reference :183-185)
    int nl = 0;
    for (int u = 2 + lane; u < n; u += 64) nl += p.nd_nin[N0 + u];
    nl = __builtin_amdgcn_readlane(wave_scan_add(nl), 63) - (int)p.nd_nout[N0];
    if (lane == 0) { cnt[0] = n - 2; cnt[1] = nl < 0 ? 0 : nl; cnt[2] = 0; }
}

// One workgroup per set.  Segments: a thread per walk position; the links' offsets from a block prefix sum over the in-edge counts without the source.
// Paths: every walk position's out-edge bitsets ORed into one bitset per node (GfaDev.orw), then a read at a time -- the reads dealt across the wavefronts --
// two sweeps over the walk order, 64 positions at a time: the ballot of "the read's bit is set" counted, then, once the reads' offsets are known, each set lane
// writes at offset + popcount(mask below it).  A set whose links or path entries do not fit what the host laid out is flagged in cnt[2] and writes nothing there.
__global__ void __launch_bounds__(GT) poa_gfa_fill_kernel(const PoaDev p, const GfaDev g) {
    __shared__ int s_wave[GW]; __shared__ int s_base; __shared__ int s_bad;
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (s >= p.n_sets) return;
    const PoaSet S = p.sets[s];
    int32_t *cnt = g.cnt + 3 * (int64_t)s;
    const int n_seg = cnt[0], n_link = cnt[1];
    if (p.state[s].status != POA_ST_OK || n_seg <= 0 || n_seg > S.node_cap) return;
    const int64_t N0 = S.node0;
    const int64_t seg0 = g.off[4 * (int64_t)s], link0 = g.off[4 * (int64_t)s + 1], path0 = g.off[4 * (int64_t)s + 2], path_cap = g.off[4 * (int64_t)s + 3];
    const int32_t *walk = g.walk + N0;
    int32_t *seg_node = g.seg_node + seg0, *link_off = g.link_off + seg0 + s, *link_from = g.link_from + link0, *path_node = g.path_node + path0;
    uint8_t *seg_base = g.seg_base + seg0;
    int64_t *path_off = g.path_off + S.read0 + s;
    uint64_t *orw = g.orw + N0 * p.rid_words;
    const int W = p.rid_words, n = n_seg + 2;
    if (tid == 0) { s_base = 0; s_bad = 0; }
    __syncthreads();
    for (int i0 = 0; i0 < n_seg; i0 += GT) {
        const int i = i0 + tid; int u = -1, ni = 0, c = 0;
        if (i < n_seg) {
            u = walk[i];
            if (u < 2 || u >= n) u = -1;      // (cannot be: the walk checked its entries)
        }
        if (u >= 0) {
            seg_node[i] = u - 1; seg_base[i] = p.nd_base[N0 + u];
            ni = p.nd_nin[N0 + u];
            for (int t = 0; t < ni; ++t) c += in_slot(p, S, N0 + u, t) != 0;
            const int no = p.nd_nout[N0 + u];
            for (int w_ = 0; w_ < W; ++w_) {
                unsigned long long m_ = 0;
                for (int e = 0; e < no && e < p.out_cap; ++e) m_ |= p.nd_rid[((N0 + u) * p.out_cap + e) * W + w_];
                orw[(int64_t)i * W + w_] = m_;
            }
        } else if (i < n_seg) { for (int w_ = 0; w_ < W; ++w_) orw[(int64_t)i * W + w_] = 0; atomicOr(&s_bad, 1); }
        const int incl = wave_scan_add(c);
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int before = s_base;
        for (int w_ = 0; w_ < wave; ++w_) before += s_wave[w_];
        const int at = before + incl - c;
        if (u >= 0) {
            link_off[i] = at;
            if (at + c <= n_link) { int k = at; for (int t = 0; t < ni; ++t) { const int f = in_slot(p, S, N0 + u, t); if (f != 0) link_from[k++] = f - 1; } }
            else atomicOr(&s_bad, 1);
        }
        __syncthreads();
        if (tid == GT - 1) s_base = before + incl;
        __syncthreads();
    }
    if (tid == 0) { link_off[n_seg] = s_base; if (s_base != n_link) s_bad = 1; }
    __threadfence();
    __syncthreads();
    // ---- paths, sweep 1: entries per read
    const int n_reads = S.n_reads;
    for (int r = wave; r < n_reads; r += GW) {
        int tot = 0;
        for (int i0 = 0; i0 < n_seg; i0 += 64) {
            const int i = i0 + lane;
            const bool on = i < n_seg && (ld_fresh64u(orw + (int64_t)i * W + (r >> 6)) >> (r & 63) & 1);
            tot += __popcll(__ballot(on));
        }
        if (lane == 0) path_off[r + 1] = tot;
    }
    if (tid == 0) path_off[0] = 0;
    __threadfence();
    __syncthreads();
    // offsets: prefix sum over the reads, 64 at a time, on wavefront 0
    if (wave == 0) {
        long long carry = 0;
        for (int r0 = 0; r0 < n_reads; r0 += 64) {
            const int r = r0 + lane;
            const int c = r < n_reads ? (int)ld_fresh64(path_off + r + 1) : 0;
            const int incl = wave_scan_add(c);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); __builtin_amdgcn_wave_barrier();
            if (r < n_reads) path_off[r + 1] = carry + incl;
            carry += __builtin_amdgcn_readlane(incl, 63);
        }
        if (lane == 0 && carry > path_cap) s_bad = 1;
    }
    __threadfence();
    __syncthreads();
    const bool bad = s_bad != 0;
    if (tid == 0) cnt[2] = bad ? 1 : 0;
    if (bad) return;
    // ---- sweep 2: the entries
    for (int r = wave; r < n_reads; r += GW) {
        long long at = ld_fresh64(path_off + r); const long long end = ld_fresh64(path_off + r + 1);
        for (int i0 = 0; i0 < n_seg; i0 += 64) {
            const int i = i0 + lane;
            const bool on = i < n_seg && (ld_fresh64u(orw + (int64_t)i * W + (r >> 6)) >> (r & 63) & 1);
            const unsigned long long mask = __ballot(on);
            const long long mine = at + __popcll(mask & ((1ull << lane) - 1));
            if (on && mine < end && mine < path_cap) path_node[mine] = walk[i] - 1;
            at += __popcll(mask);
        }
    }
}

size_t poa_gfa_walk_lds_bytes(int lds_cap) { return 8 * (size_t)(lds_cap > 0 ? lds_cap : 0) + 16; }
hipError_t launch_poa_gfa_walk(const PoaDev &p, const GfaDev &g, hipStream_t s) {
    if (p.n_sets <= 0) return hipSuccess;
    hipLaunchKernelGGL(poa_gfa_walk_kernel, dim3(p.n_sets), dim3(64), poa_gfa_walk_lds_bytes(g.lds_cap), s, p, g);      // (at most 6000 nodes: 48 KB)
    return hipGetLastError();
}
hipError_t launch_poa_gfa_fill(const PoaDev &p, const GfaDev &g, hipStream_t s) {
    if (p.n_sets <= 0) return hipSuccess;
    hipLaunchKernelGGL(poa_gfa_fill_kernel, dim3(p.n_sets), dim3(GT), 0, s, p, g);
    return hipGetLastError();
}

}  // namespace abpoa_hip
