// hub_chunks.hpp -- the chunk records of a long row ("hub"): what pagerank.hip and betweenness.hip share.
//
// A row too long for one group of lanes is cut into chunks of CHUNK entries, and a later launch gives every chunk a
// workgroup, so a hub costs what its entries cost.  A chunk is a record {row, chunk number} in an array that the
// classifying launch fills from a cursor: whoever owns the row takes its k records by ONE atomicAdd.  The order of the
// records depends on scheduling and changes nothing: a launch consumes a whole slice of them.  CHUNK is each algorithm's
// own constant (they were tuned apart), and so are the rule for which rows count as hubs and the array's capacity.
#pragma once
#include <hip/hip_runtime.h>

namespace bsp {

// the chunks of a row of `len` entries
template <int CHUNK>
__host__ __device__ __forceinline__ int hub_chunks_of(int len)
{
    return (len + CHUNK - 1) / CHUNK;
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

}  // namespace bsp
