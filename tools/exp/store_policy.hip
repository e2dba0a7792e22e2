// probe: does the emit kernel's launch end pay for dirty lines left in the XCD L2s?  215 MB (the emit output at 10 k images)
// written by one buffer, launched back to back as the headline does, with the emit kernel's pattern (256-thread workgroups,
// 16 KiB contiguous per workgroup, XCD x one contiguous eighth of the buffer).  Store policies:
//   plain     16-B write-back stores
//   sc1       16-B write-through stores (buffer_store_dwordx4 ... sc1: nothing stays dirty in L2 at the launch end)
//   tail-sc1  plain, except the last `tail` bytes of each XCD's eighth, written through
// Prints the time per launch (HIP events over back-to-back launches: kernel + boundary); run under rocprofv3 --kernel-trace
// --stats for the kernels alone.
// build: hipcc --offload-arch=gfx950 -O3 -o store_policy store_policy.hip
#include <hip/hip_runtime.h>
#include <cstdio>

typedef double dbl2 __attribute__((ext_vector_type(2)));
constexpr int kThreads = 256, kPerLane = 4;   // 16 KiB per workgroup

template <int POLICY>   // 0 plain, 1 sc1, 2 tail-sc1
__global__ __launch_bounds__(kThreads) void store_policy_kernel(double *dst, unsigned int n_chunks, unsigned int tail_chunks, double v)
{
    const unsigned int b = blockIdx.x, x = b & 7u, j = b >> 3, q = n_chunks >> 3, r = n_chunks & 7u;
    const unsigned int own = q + (x < r ? 1u : 0u);          // chunks of this XCD's eighth
    const unsigned int chunk = x * q + (x < r ? x : r) + j;  // xcd_contiguous_block
    if (j >= own) return;
    const dbl2 val = {v, v};
    const bool wt = POLICY == 1 || (POLICY == 2 && j + tail_chunks >= own);
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(dst, 0, 0x7fffffff, 0x00020000);
    const unsigned long long base = (unsigned long long)chunk * (kThreads * kPerLane) + threadIdx.x;
#pragma unroll
    for (int k = 0; k < kPerLane; k++) {
        const unsigned long long i = base + (unsigned long long)k * kThreads;
        if (wt) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned int, val), rsrc,
                                                       (int)(i * 16), 0, 16);   // aux 16 = sc1
        else reinterpret_cast<dbl2 *>(dst)[i] = val;
    }
}

template <int POLICY>
void run(double *buf, unsigned int n_chunks, unsigned int tail_chunks, const char *name)
{
    const unsigned int grid = 8 * ((n_chunks + 7) / 8);
    hipEvent_t a, b;
    hipEventCreate(&a);
    hipEventCreate(&b);
    for (int w = 0; w < 20; w++) store_policy_kernel<POLICY><<<grid, kThreads>>>(buf, n_chunks, tail_chunks, 1.0);
    hipEventRecord(a);
    const int reps = 200;
    for (int r = 0; r < reps; r++) store_policy_kernel<POLICY><<<grid, kThreads>>>(buf, n_chunks, tail_chunks, 1.0);
    hipEventRecord(b);
    hipEventSynchronize(b);
    float ms;
    hipEventElapsedTime(&ms, a, b);
    const double us = ms / reps * 1e3, bytes = (double)n_chunks * kThreads * kPerLane * 16;
    printf("%-34s tail %6.2f MiB per XCD  %7.2f us per launch  %.2f TB/s\n", name, tail_chunks * 16384.0 / 1048576, us, bytes / (us * 1e-6) / 1e12);
    hipEventDestroy(a);
    hipEventDestroy(b);
}

int main()
{
    const double mb = 215.04;
    const unsigned int n_chunks = (unsigned int)(mb * 1e6 / 16384);
    double *buf;
    if (hipMalloc(&buf, (size_t)n_chunks * 16384) != hipSuccess) return 1;
    printf("--- %.1f MB, %u chunks of 16 KiB\n", mb, n_chunks);
    for (int round = 0; round < 2; round++) {
        run<0>(buf, n_chunks, 0, "plain");
        run<1>(buf, n_chunks, 0, "sc1 write-through");
        run<2>(buf, n_chunks, 128, "plain, last 2 MiB/XCD sc1");
        run<2>(buf, n_chunks, 256, "plain, last 4 MiB/XCD sc1");
        run<2>(buf, n_chunks, 512, "plain, last 8 MiB/XCD sc1");
    }
    hipFree(buf);
    return 0;
}
