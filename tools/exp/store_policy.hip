// probe: does the emit kernel's launch end pay for dirty lines left in the XCD L2s?  215 MB (the emit output at 10 k images)
// written by one buffer, launched back to back as the headline does, with the emit kernel's pattern (256-thread workgroups,
// 16 KiB contiguous per workgroup, XCD x one contiguous eighth of the buffer).  Store policies:
//   plain     16-B write-back stores
//   sc1       16-B write-through stores (buffer_store_dwordx4 ... sc1: nothing stays dirty in L2 at the launch end)
//   tail-sc1  plain, except the last `tail` bytes of each XCD's eighth, written through
// The emit SHAPE (second part): the same 215 MB as the emit launch lays them out -- three arrays (residual pairs 16 B, intrinsic rows
// 96 B, pose rows 96 B per observation), one-shot workgroups of 4 waves x 64 observations (13 KiB per wave in 13 stores of 1 KiB),
// write-through, XCD x one contiguous eighth -- without any arithmetic or prologue in front of the stores:
//   emit shape            3 750 workgroups of 256 observations (the launch as it is: 3.66 rounds on 1 024 slots)
//   emit shape, tail T    a tail schedule (emit_tail_tile below): the last T workgroups of every XCD 64 observations, the T before
//                         them 128 -- what a write of this shape costs when its end is level
// Prints the time per launch (HIP events over back-to-back launches: kernel + boundary); run under rocprofv3 --kernel-trace
// --stats for the kernels alone.
// build: hipcc --offload-arch=gfx950 -O3 -o store_policy tools/exp/store_policy.hip
#include <hip/hip_runtime.h>
#include <cstdio>

// The tail schedule this probe measures (result: profiles/r14_emit_head_tail.md; the emit kernel does not use it, tools/exp/emit_tail_r14.patch):
// observations in runs of 64, XCD x the x-th contiguous eighth of the runs, its j-th workgroup 4 runs (j < n4), 2 runs (j < n4 + n2), else 1.
#define VG_MAP_HD __host__ __device__ __forceinline__
namespace vg {

constexpr unsigned int kEmitRun = 64;           // observations of a run: one wave

struct EmitTailSchedule {
    unsigned int n4, n2;   // full and two-run workgroups per XCD
};

// workgroups of a launch under the schedule: 8 x (n4 + n2 + the longest eighth's single runs)
VG_MAP_HD unsigned int emit_tail_grid(unsigned int n_obs, unsigned int n4, unsigned int n2)
{
    const unsigned int n_runs = (n_obs + kEmitRun - 1) / kEmitRun, q = n_runs >> 3, r = n_runs & 7u;
    return 8u * (n4 + n2 + (q + (r ? 1u : 0u) - 4u * n4 - 2u * n2));
}

// Workgroup `b` of a launch of n_runs runs: its first run and run count; false = nothing left for it.  Bijective on the runs.
VG_MAP_HD bool emit_tail_tile(unsigned int b, unsigned int n_runs, unsigned int n4, unsigned int n2, unsigned int &run0, unsigned int &n_run)
{
    const unsigned int x = b & 7u, j = b >> 3, q = n_runs >> 3, r = n_runs & 7u;
    const unsigned int own = q + (x < r ? 1u : 0u);   // runs of this XCD's eighth
    unsigned int at;
    if (j < n4) {
        at = 4u * j;
        n_run = 4u;
    } else if (j < n4 + n2) {
        at = 4u * n4 + 2u * (j - n4);
        n_run = 2u;
    } else {
        at = 4u * n4 + 2u * n2 + (j - n4 - n2);
        n_run = 1u;
    }
    if (at >= own) return false;
    run0 = x * q + (x < r ? x : r) + at;
    return true;
}

// The host's schedule for n_obs observations: the last `tail` workgroups of every XCD take one run, the `tail` before them two.
// Launches too small for that keep what fits (single runs first); what is left over of an eighth (< 4 runs, + 1 on the first
// n_runs % 8 dies) goes as single runs as well.
inline EmitTailSchedule emit_tail_schedule(unsigned int n_obs, unsigned int tail)
{
    const unsigned int n_runs = (n_obs + kEmitRun - 1) / kEmitRun, q = n_runs >> 3;
    const unsigned int n1 = tail < q ? tail : q;
    const unsigned int n2 = tail < (q - n1) / 2 ? tail : (q - n1) / 2;
    EmitTailSchedule s;
    s.n2 = n2;
    s.n4 = (q - n1 - 2 * n2) / 4;
    return s;
}

}  // namespace vg

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

// one emit tile's stores without the tile's work: waves [0, n_run) of the workgroup write their 64 observations' rows
__global__ __launch_bounds__(kThreads) void emit_shape_kernel(double *res, double *ji, double *jm, unsigned int n_obs, unsigned int tail_on, unsigned int n4,
                                                              unsigned int n2, double v)
{
    typedef unsigned int u4 __attribute__((ext_vector_type(4)));
    const unsigned int n_runs = (n_obs + vg::kEmitRun - 1) / vg::kEmitRun;
    unsigned int run0, n_run = 4;
    if (tail_on) {
        if (!vg::emit_tail_tile(blockIdx.x, n_runs, n4, n2, run0, n_run)) return;
    } else {
        const unsigned int b = blockIdx.x, n = gridDim.x, x = b & 7u, j = b >> 3, q = n >> 3, r = n & 7u;
        run0 = 4u * (x * q + (x < r ? x : r) + j);   // xcd_contiguous_block
    }
    const unsigned int wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    if (wave >= n_run) return;
    const unsigned int o = (run0 + wave) * vg::kEmitRun;
    if (o + vg::kEmitRun > n_obs) return;   // the probe's n_obs is a multiple of 64
    const dbl2 val = {v, v};
    const u4 bits = __builtin_bit_cast(u4, val);
    dbl2 *r16 = reinterpret_cast<dbl2 *>(res) + o + lane;
    asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(r16), "v"(bits) : "memory");
    dbl2 *a16 = reinterpret_cast<dbl2 *>(ji) + (size_t)o * 6 + lane, *b16 = reinterpret_cast<dbl2 *>(jm) + (size_t)o * 6 + lane;
#pragma unroll
    for (int k = 0; k < 6; k++) asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(a16 + k * 64), "v"(bits) : "memory");
#pragma unroll
    for (int k = 0; k < 6; k++) asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(b16 + k * 64), "v"(bits) : "memory");
}

void run_shape(double *buf, unsigned int n_obs, unsigned int tail)
{
    double *res = buf, *ji = buf + (size_t)n_obs * 2, *jm = ji + (size_t)n_obs * 12;
    const vg::EmitTailSchedule s = vg::emit_tail_schedule(n_obs, tail);
    const unsigned int grid = tail ? vg::emit_tail_grid(n_obs, s.n4, s.n2) : (n_obs + 255) / 256;
    hipEvent_t a, b;
    hipEventCreate(&a);
    hipEventCreate(&b);
    for (int w = 0; w < 20; w++) emit_shape_kernel<<<grid, kThreads>>>(res, ji, jm, n_obs, tail ? 1u : 0u, s.n4, s.n2, 1.0);
    hipEventRecord(a);
    const int reps = 200;
    for (int r = 0; r < reps; r++) emit_shape_kernel<<<grid, kThreads>>>(res, ji, jm, n_obs, tail ? 1u : 0u, s.n4, s.n2, 1.0);
    hipEventRecord(b);
    hipEventSynchronize(b);
    float ms;
    hipEventElapsedTime(&ms, a, b);
    const double us = ms / reps * 1e3, bytes = (double)n_obs * 208;
    printf("emit shape, tail %3u (grid %5u)        %7.2f us per launch  %.2f TB/s\n", tail, grid, us, bytes / (us * 1e-6) / 1e12);
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
    const unsigned int n_obs = 960000;   // 10 000 images x 96 corners: 199.7 MB in the three arrays
    printf("--- emit shape, %u observations x 208 B\n", n_obs);
    for (int round = 0; round < 3; round++)
        for (unsigned int tail : {0u, 32u, 64u, 128u}) run_shape(buf, n_obs, tail);
    hipFree(buf);
    return 0;
}
