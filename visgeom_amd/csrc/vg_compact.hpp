// vg_compact.hpp -- the scan of an ordered compaction, shared by the packs that keep the reference's raster order (the
// photometric data pack, the bundle adjustment's pack, the multi-hypothesis depth pack, the line detector's maxima).  Each of
// them counts the survivors of every block of LANES items in a first pass, scans the block counts here, and in a second pass
// places every survivor at its block's offset plus the survivors of the lower waves and lanes of its block.  A template, so that
// every translation unit that launches it may hold its instantiation.
#pragma once

#include <hip/hip_runtime.h>

namespace vgc {

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
