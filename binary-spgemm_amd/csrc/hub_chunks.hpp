// hub_chunks.hpp -- what the kernels that give a group of lanes to every vertex of a list share (pagerank.hip,
// betweenness.hip, bfs_tree.hip, extract.hip, match.hip, sssp.hip): the chunk records of a long row ("hub"), the opening of
// a kernel with W lanes per listed vertex (GroupRow), and a workgroup's append to the next list (block_list_append).
//
// A row too long for one group of lanes is cut into chunks of CHUNK entries, and a later launch gives every chunk a
// workgroup, so a hub costs what its entries cost.  A chunk is a record {row, chunk number} in an array that the
// classifying launch fills from a cursor: whoever owns the row takes its k records by ONE atomicAdd.  The order of the
// records depends on scheduling and changes nothing: a launch consumes a whole slice of them.  CHUNK is each algorithm's
// own constant (they were tuned apart), and so are the rule for which rows count as hubs and the array's capacity.
#pragma once
#include <hip/hip_runtime.h>
#include "wave.hpp"

namespace bsp {

// the chunks of a row of `len` entries
template <int CHUNK>
__host__ __device__ __forceinline__ int hub_chunks_of(int len)
{
    return (len + CHUNK - 1) / CHUNK;
}

// the chunk records of a row: none for one that a group of lanes walks itself
template <int CHUNK>
__host__ __device__ __forceinline__ int hub_chunks_over(int len)
{
    return len > CHUNK ? hub_chunks_of<CHUNK>(len) : 0;
}

// row v takes its k >= 1 records from *cursor.  The stores are bounded by chunk_cap whatever the cursor holds; the host
// refuses a cursor beyond it.
__device__ __forceinline__ void hub_chunks_emit(int v, int k, int *cursor, int2 *chunk, int chunk_cap)
{
    const int base = atomicAdd(cursor, k);
    for (int j = 0; j < k; j++)
        if ((unsigned)(base + j) < (unsigned)chunk_cap) chunk[base + j] = make_int2(v, j);
}

// the entries [b, e) of record `rec`; rp: the row_ptr of the operand whose rows were cut
template <int CHUNK>
__device__ __forceinline__ void hub_chunk_range(const int *rp, int2 rec, long long &b, long long &e)
{
    b = (long long)rp[rec.x] + (long long)rec.y * CHUNK;
    e = min((long long)rp[rec.x + 1], b + CHUNK);
}

// What a thread of a launch with W lanes per vertex of list[first .. first + fsize) and THREADS per workgroup walks.  In
// two steps, because a kernel's thread 0 resets its counters between them and the stores keep their place in front of the
// loads:
//     GroupRow<W, THREADS> g;                                     t, f and sub
//     g.template row<CHUNK>(fsize, list, first, rp, beside);      pos and e of the group's vertex u, then beside(u)
// A row longer than CHUNK is the chunks' row: its group gets nothing (pos == e), and so does a group without a vertex.
// beside(u) is what the kernel loads or stores for its vertex (a distance, a sigma), under the same test; it must not
// capture the GroupRow by reference.  The users are k_bc_forward and k_sssp_relax, which come out to the instruction as they
// did with the decode spelled out.  k_bc_backward, k_match_point and k_bfs_push keep theirs: each differs in a detail (a
// flag beside the cut, the test in 32 bits, pos before the load of the row's end) and compiles to other code with this.
template <int W, int THREADS>
struct GroupRow {
    long long t, f;                     // the thread of the grid, and its group: the place in the list
    int sub;                            // the lane's place in its group
    long long e = 0, pos = 0;           // the end of the walk and the lane's first entry, in steps of W (64-bit: e may be INT_MAX)

    __device__ __forceinline__ GroupRow() : t((long long)blockIdx.x * THREADS + threadIdx.x), f(t / W), sub((int)(t % W)) {}

    template <int CHUNK, class F>
    __device__ __forceinline__ void row(int fsize, const int *list, int first, const int *rp, F &&beside)
    {
        if (f < fsize) {
            const int u = list[first + f];
            const long long b = rp[u];
            e = rp[u + 1];
            if (e - b > CHUNK) e = b;                        // (the chunks' row)
            pos = b + sub;
            beside(u);
        }
    }
};

// The LDS record of block_list_append.  ALSO: with the third sum (one unused word without it).
template <int THREADS, bool ALSO>
struct ListBlock {
    long long deg[THREADS / 64];
    int cnt[THREADS / 64], also[ALSO ? THREADS / 64 : 1];
    int base;
};

// A workgroup of THREADS appends its vertices with `take` (u each, row lengths from rp) to list[next->x ...]; called by
// every thread.  The workgroup's appends and the row lengths of the appended vertices (into *walked) go out by ONE atomic
// each: with wave_append and a wave_count per wave the counters, which share a cache line, took an atomic per wave each, and
// the launches were bound by them.  ALSO: the threads with `also` are counted into *also_word the same way.
// A hub's chunk records (rows longer than CHUNK) are taken by its own thread, from the cursor next->y.  The caller lists a
// vertex once per launch at most, so a list never passes n entries and the records never pass chunk_cap (the host sized it
// for every hub at once); the stores are bounded all the same.  The walked atomic is guarded by the length sum: an appended
// vertex may have an empty row (sssp.hip).  Where every listed vertex has entries (match.hip) that is the same condition as
// "the workgroup appended something".  No barrier at the end: a caller that calls again in a loop puts one between the calls,
// which frees `sh`.
template <int THREADS, int CHUNK, bool ALSO>
__device__ __forceinline__ void block_list_append(bool take, bool also, int u, const int *__restrict__ rp, int n, int *list,
                                                  int2 *next, u64 *walked, int *also_word, int2 *chunk, int chunk_cap,
                                                  ListBlock<THREADS, ALSO> &sh)
{
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    const u64 m = __ballot(take);
    const int du = take ? rp[u + 1] - rp[u] : 0;
    const long long d = m ? wave_sum((long long)du) : 0;     // (wave-uniform)
    const int p = ALSO ? __popcll(__ballot(also)) : 0;
    if (lane == 0) {
        sh.cnt[wv] = __popcll(m);
        sh.deg[wv] = d;
        if (ALSO) sh.also[wv] = p;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0, as = 0;
        long long dsum = 0;
#pragma unroll
        for (int q = 0; q < THREADS / 64; q++) {
            const int c = sh.cnt[q];
            sh.cnt[q] = total;                               // the wave's offset in the workgroup's slice
            total += c;
            dsum += sh.deg[q];
            if (ALSO) as += sh.also[q];
        }
        sh.base = 0;
        if (total) {
            sh.base = atomicAdd(&next->x, total);
            if (dsum) atomicAdd(walked, (u64)dsum);          // (under `total`, which it implies: the kernels need fewer registers so)
        }
        if (ALSO && as) atomicAdd(also_word, as);
    }
    __syncthreads();
    const int at = sh.base + sh.cnt[wv] + __popcll(m & mask_lt(lane));
    if (take && (unsigned)at < (unsigned)n) list[at] = u;
    const int k = hub_chunks_over<CHUNK>(du);
    if (k) hub_chunks_emit(u, k, &next->y, chunk, chunk_cap);
}

}  // namespace bsp
