// vg_compact.hpp -- the ordered compaction shared by the packs that keep the reference's raster order (the photometric data
// pack, the bundle adjustment's pack, the multi-hypothesis depth pack, the line detector's maxima).  Each of them counts the
// survivors of every block of LANES items in a first pass (block_place<false>), scans the block counts (scan_block_counts), and
// in a second pass places every survivor at its block's offset plus the survivors of the lower waves and lanes of its block
// (block_place<true>).  Templates, so that every translation unit that launches them may hold its instantiation.
#pragma once

#include <hip/hip_runtime.h>

namespace vgc {

// the set bits of a wave ballot below the calling lane
__device__ __forceinline__ unsigned lanes_below(unsigned long long ball) { return (unsigned)__popcll(ball & ((1ull << (threadIdx.x & 63)) - 1ull)); }

// The block step of both passes.  below: the entries of the wave's lower lanes, total: the entries of the whole wave (a lane may
// hold several); slot: the block's index into counts / offsets.  Pass 1 (WRITE = false) stores the block's count and returns 0;
// pass 2 returns the place of the lane's first entry: the block's scanned offset, the lower waves, the lower lanes.  It holds a
// barrier: every thread of the workgroup calls it, and leaves afterwards.
template <bool WRITE, int LANES>
__device__ __forceinline__ unsigned block_place(unsigned below, unsigned total, int64_t slot, unsigned *counts, const unsigned *offsets)
{
    __shared__ unsigned wave_count[LANES / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_count[wave] = total;
    __syncthreads();
    if (!WRITE) {
        if (threadIdx.x == 0) {
            unsigned n = 0;
#pragma unroll
            for (int k = 0; k < LANES / 64; k++) n += wave_count[k];
            counts[slot] = n;
        }
        return 0;
    }
    unsigned pos = offsets[slot] + below;
    for (int k = 0; k < wave; k++) pos += wave_count[k];
    return pos;
}

// one entry per lane at most
template <bool WRITE, int LANES>
__device__ __forceinline__ unsigned block_place(bool keep, int64_t slot, unsigned *counts, const unsigned *offsets)
{
    const unsigned long long ball = __ballot(keep);
    return block_place<WRITE, LANES>(lanes_below(ball), (unsigned)__popcll(ball), slot, counts, offsets);
}

// exclusive scan of nb block counts by one workgroup: a contiguous run per thread, the LANES run sums in order
template <int LANES>
__device__ __forceinline__ void scan_block_counts(const unsigned *counts, unsigned *offsets, int nb, unsigned *total)
{
    __shared__ unsigned run_sum[LANES];
    const int chunk = (nb + LANES - 1) / LANES;
    const int lo = min((int)threadIdx.x * chunk, nb), hi = min(lo + chunk, nb);
    unsigned s = 0;
    for (int i = lo; i < hi; i++) s += counts[i];
    run_sum[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned run = 0;
        for (int t = 0; t < LANES; t++) {
            const unsigned c = run_sum[t];
            run_sum[t] = run;
            run += c;
        }
        *total = run;
    }
    __syncthreads();
    unsigned run = run_sum[threadIdx.x];
    for (int i = lo; i < hi; i++) {
        offsets[i] = run;
        run += counts[i];
    }
}

// one array of block counts, one workgroup
template <int LANES>
__global__ __launch_bounds__(LANES) void scan_block_counts_kernel(const unsigned *counts, unsigned *offsets, int nb, unsigned *total)
{
    scan_block_counts<LANES>(counts, offsets, nb, total);
}

// counts and offsets [items][nb], total [items]: one workgroup per item, each item scanned on its own
template <int LANES>
__global__ __launch_bounds__(LANES) void scan_block_counts_items_kernel(const unsigned *counts, unsigned *offsets, int nb, unsigned *total)
{
    const size_t first = (size_t)blockIdx.x * nb;
    scan_block_counts<LANES>(counts + first, offsets + first, nb, total + blockIdx.x);
}

}  // namespace vgc
