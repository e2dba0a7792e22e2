// vg_measure_tu.hip -- translation unit of libvisgeom_amd.so: the roofline helpers (vg_calib_stream_write / _copy, vg_calib_fp64_fma,
// vg_calib_d2h_copies) and their three kernels: what this box delivers, measured next to the kernels that are judged by it.
// Built with hipcc for gfx950 only; compiled on its own so that an edit of one subsystem does not rebuild the others.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "vg_internal.hpp"

using vgi::fail;

namespace vg {

// ------------------------------------------------------------------------------------------
// measurement helpers: pure streaming write / copy with the emit kernel's store pattern -- every wave
// instruction moves 1 KiB of consecutive bytes (16 B per lane) and a workgroup owns one contiguous
// 16 KiB run.  Used to calibrate rocprofv3's FETCH_SIZE / WRITE_SIZE and as the box's measured
// streaming rate.
// ------------------------------------------------------------------------------------------
constexpr int kStreamUnroll = 4;

__global__ __launch_bounds__(256) void vg_stream_write_kernel(double *__restrict__ dst, long long n2, double value)
{
    using d2 = HIP_vector_type<double, 2>;
    d2 v;
    v.x = value;
    v.y = value;
    d2 *d = reinterpret_cast<d2 *>(dst);
    const long long base = (long long)blockIdx.x * (256 * kStreamUnroll) + threadIdx.x;
#pragma unroll
    for (int k = 0; k < kStreamUnroll; k++) {
        const long long i = base + k * 256;
        if (i < n2) d[i] = v;
    }
}

__global__ __launch_bounds__(256) void vg_stream_copy_kernel(double *__restrict__ dst, const double *__restrict__ src,
                                                              long long n2)
{
    using d2 = HIP_vector_type<double, 2>;
    d2 *d = reinterpret_cast<d2 *>(dst);
    const d2 *s = reinterpret_cast<const d2 *>(src);
    const long long base = (long long)blockIdx.x * (256 * kStreamUnroll) + threadIdx.x;
    d2 t[kStreamUnroll];
#pragma unroll
    for (int k = 0; k < kStreamUnroll; k++) {
        const long long i = base + k * 256;
        if (i < n2) t[k] = s[i];
    }
#pragma unroll
    for (int k = 0; k < kStreamUnroll; k++) {
        const long long i = base + k * 256;
        if (i < n2) d[i] = t[k];
    }
}

// What the FP64 vector pipe delivers on this box under the occupancy of the fused Gram kernels (two waves per SIMD: 256-thread
// workgroups, two per CU by their LDS reservation): every lane runs kFmaChains independent chains of dependent v_fma_f64 -- no
// memory, a loop of a few hundred bytes.  The guide's 78.6 TFLOP/s assume 2.4 GHz; under this load the part runs lower
// (profiles/NOTES.md, tools/exp/fp64_ramp.hip), and bench.py prints this next to the Gram kernel's roofline fraction.
constexpr int kFmaChains = 8;
__global__ __launch_bounds__(256) void vg_fp64_fma_kernel(double *__restrict__ out, int iters, double seed)
{
    extern __shared__ double fma_pad[];   // reserves the LDS that limits a CU to two workgroups; never touched
    double x[kFmaChains];
#pragma unroll
    for (int i = 0; i < kFmaChains; i++) x[i] = seed + 1e-3 * i + 1e-9 * threadIdx.x;
    const double a = 1.0000001, b = 1e-9;
#pragma unroll 4
    for (int k = 0; k < iters; k++)
#pragma unroll
        for (int i = 0; i < kFmaChains; i++) x[i] = __builtin_fma(x[i], a, b);
    double t = 0.;
#pragma unroll
    for (int i = 0; i < kFmaChains; i++) t += x[i];
    if (t == 12345.678) {   // never: keeps the chains alive
        fma_pad[threadIdx.x] = t;
        out[blockIdx.x] = fma_pad[threadIdx.x ^ 1];
    }
}

}  // namespace vg

extern "C" {

int vg_calib_stream_write(void *hip_stream, double *dst, int64_t n_doubles, double value)
{
    if (!dst || n_doubles < 0 || (n_doubles & 1)) return fail(VG_ERR_INVALID_ARGUMENT, "need an even number of doubles");
    const long long n2 = n_doubles / 2;
    const unsigned int grid = (unsigned int)((n2 + 256 * vg::kStreamUnroll - 1) / (256 * vg::kStreamUnroll));
    if (!grid) return VG_OK;
    hipLaunchKernelGGL(vg::vg_stream_write_kernel, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(hip_stream),
                       dst, n2, value);
    VG_HIP(hipGetLastError());
    return VG_OK;
}

int vg_calib_fp64_fma(void *hip_stream, double *scratch, int iters, int64_t *flops_out)
{
    if (!scratch || iters < 1 || !flops_out) return fail(VG_ERR_INVALID_ARGUMENT, "scratch / iters / flops_out");
    int dev = 0;
    hipDeviceProp_t prop;
    VG_HIP(hipGetDevice(&dev));
    VG_HIP(hipGetDeviceProperties(&prop, dev));
    const size_t lds = 72 * 1024;   // two workgroups of four waves per CU = two waves per SIMD: the fused Gram kernels' occupancy
    static bool raised = false;
    if (!raised) {
        VG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(vg::vg_fp64_fma_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        raised = true;
    }
    const unsigned int grid = 2u * (unsigned int)prop.multiProcessorCount;
    hipLaunchKernelGGL(vg::vg_fp64_fma_kernel, dim3(grid), dim3(256), lds, reinterpret_cast<hipStream_t>(hip_stream), scratch, iters, 1.0);
    VG_HIP(hipGetLastError());
    *flops_out = (int64_t)grid * 256 * (int64_t)iters * vg::kFmaChains * 2;
    return VG_OK;
}

int vg_calib_d2h_copies(int device, int64_t bytes, int reps, double *seconds_out)
{
    if (bytes <= 0 || reps <= 0 || !seconds_out) return fail(VG_ERR_INVALID_ARGUMENT, "bad arguments");
    VG_HIP(hipSetDevice(device));
    vgi::DeviceMem<void> dev;
    vgi::PinnedMem<void> host;
    VG_HIP(dev.alloc((size_t)bytes));
    if (host.alloc((size_t)bytes, hipHostMallocDefault) != hipSuccess) return fail(VG_ERR_ALLOC, "hipHostMalloc failed");
    int rc = VG_OK;
    if (hipMemset(dev, 1, (size_t)bytes) != hipSuccess) rc = fail(VG_ERR_HIP, "hipMemset failed");
    std::memset(host, 0, (size_t)bytes);
    if (rc == VG_OK && hipMemcpy(host, dev, (size_t)bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(VG_ERR_HIP, "hipMemcpy failed");  // warm
    for (int r = 0; r < reps && rc == VG_OK; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        if (hipMemcpy(host, dev, (size_t)bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(VG_ERR_HIP, "hipMemcpy failed");
        seconds_out[r] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    return rc;
}

int vg_calib_stream_copy(void *hip_stream, double *dst, const double *src, int64_t n_doubles)
{
    if (!dst || !src || n_doubles < 0 || (n_doubles & 1)) return fail(VG_ERR_INVALID_ARGUMENT, "need an even number of doubles");
    const long long n2 = n_doubles / 2;
    const unsigned int grid = (unsigned int)((n2 + 256 * vg::kStreamUnroll - 1) / (256 * vg::kStreamUnroll));
    if (!grid) return VG_OK;
    hipLaunchKernelGGL(vg::vg_stream_copy_kernel, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(hip_stream),
                       dst, src, n2);
    VG_HIP(hipGetLastError());
    return VG_OK;
}

}  // extern "C"
