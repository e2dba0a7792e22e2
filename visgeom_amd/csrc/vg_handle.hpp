// vg_handle.hpp -- what the image-pipeline handles share on the host (vg_stereo, vg_motion_stereo, vg_depth_fusion,
// vg_photometric, vg_sparse_odom, vg_render, vg_trajectory, vg_dense_ba, vg_hough, and through vg_frame_loop.hpp vg_mono_odom
// and vg_mapping): the device and stream of a handle, grow-only buffers, the envelope of a synchronous call, the range check
// of an item count, the staging of per-item counters and the scratch of an ordered pack.  Host only; a new pipeline includes this.
#pragma once

#include <string>

#include "vg_compact.hpp"
#include "vg_internal.hpp"

namespace vgi {

constexpr int64_t kMaxItems = 65535;   // items (images, pairs, poses, hypotheses ...) ride on gridDim.y / gridDim.z

// "the <noun> count must be in [<lowest>, 65535]"
inline int check_items(int64_t n, int64_t lowest, const char *noun)
{
    if (n >= lowest && n <= kMaxItems) return VG_OK;
    return fail(VG_ERR_INVALID_ARGUMENT, std::string("the ") + noun + " count must be in [" + std::to_string(lowest) + ", 65535]");
}

// a failed hipMalloc / hipHostMalloc leaves its error behind as the thread's last error: cleared here, or the next
// hipGetLastError() after a launch would report it as that launch's
inline int alloc_failed(const char *kind, const char *what)
{
    (void)hipGetLastError();
    return fail(VG_ERR_ALLOC, std::string(kind) + " allocation of " + what + " failed");
}

// grow-only device buffer of T, counted in elements.  grow() keeps the block when it is large enough; otherwise the old
// block is freed first and the capacity is zero until the new one exists, so a failure leaves an empty buffer.
template <class T>
struct Grow {
    T *get() const { return m_.get(); }
    operator T *() const { return m_.get(); }
    size_t capacity() const { return cap_; }
    int grow(size_t n, const char *what)
    {
        if (n <= cap_) return VG_OK;
        cap_ = 0;
        if (m_.alloc(n * sizeof(T)) != hipSuccess) return alloc_failed("device", what);
        cap_ = n;
        return VG_OK;
    }

private:
    DeviceMem<T> m_;
    size_t cap_ = 0;
};

// the same in pinned host memory
template <class T>
struct GrowPinned {
    T *get() const { return m_.get(); }
    operator T *() const { return m_.get(); }
    size_t capacity() const { return cap_; }
    int grow(size_t n, const char *what)
    {
        if (n <= cap_) return VG_OK;
        cap_ = 0;
        if (m_.alloc(n * sizeof(T), hipHostMallocDefault) != hipSuccess) return alloc_failed("pinned", what);
        cap_ = n;
        return VG_OK;
    }

private:
    PinnedMem<T> m_;
    size_t cap_ = 0;
};

// first members of every handle.  open() is the tail of a create function; destroy() is the whole destroy function.
struct HandleBase {
    int device = 0;
    hipStream_t stream = nullptr;
    int open(int dev, void *hip_stream, const char *what)   // what: "<what> has no CPU fallback"
    {
        if (const int rc = check_device(dev, what)) return rc;
        device = dev;
        stream = reinterpret_cast<hipStream_t>(hip_stream);
        return VG_OK;
    }
};

template <class H>
void destroy(H *s)   // no work of the handle is left queued when its blocks are freed
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    (void)hipStreamSynchronize(s->stream);
    delete s;
}

// the envelope of a synchronous call on a handle's stream: begin() before the first allocation or enqueue, finish() where
// the call synchronises.  Leaving between the two (a failure path) drains the stream first, so nothing that reads or writes
// the handle's blocks or the caller's arrays is still queued.  A call that synchronises more than once uses one Call per leg.
class Call {
public:
    explicit Call(const HandleBase *h) : h_(h) {}
    Call(const Call &) = delete;
    Call &operator=(const Call &) = delete;
    ~Call()
    {
        if (armed_) (void)hipStreamSynchronize(h_->stream);
    }
    hipStream_t stream() const { return h_->stream; }
    int begin()
    {
        VG_HIP(hipSetDevice(h_->device));
        armed_ = true;
        return VG_OK;
    }
    int finish()
    {
        armed_ = false;
        VG_HIP(hipStreamSynchronize(h_->stream));
        return VG_OK;
    }

private:
    const HandleBase *h_;
    bool armed_ = false;
};

// per-item counters of a call, [n][k]: zeroed on the device in front of the launch, copied to pinned memory behind it and
// widened to the caller's int64 once the call has synchronised.  counts == NULL (the caller wants none) costs nothing.
struct Counters {
    // *dev: the zeroed device counters for the launch, or nullptr
    int begin(const Call &call, int64_t n, int k, const int64_t *counts, unsigned long long **dev)
    {
        *dev = nullptr;
        if (!counts) return VG_OK;
        const size_t len = (size_t)n * k;
        if (const int rc = d_.grow(len, "the counters")) return rc;
        if (const int rc = h_.grow(len, "the counters' staging")) return rc;
        VG_HIP(hipMemsetAsync(d_.get(), 0, len * sizeof(unsigned long long), call.stream()));
        *dev = d_.get();
        return VG_OK;
    }
    // queues the copy back, finishes the call and fills counts
    int end(Call &call, int64_t n, int k, int64_t *counts)
    {
        const size_t len = (size_t)n * k;
        if (counts) VG_HIP(hipMemcpyAsync(h_.get(), d_.get(), len * sizeof(unsigned long long), hipMemcpyDeviceToHost, call.stream()));
        if (const int rc = call.finish()) return rc;
        for (size_t i = 0; counts && i < len; i++) counts[i] = (int64_t)h_.get()[i];
        return VG_OK;
    }

private:
    Grow<unsigned long long> d_;
    GrowPinned<unsigned long long> h_;
};

// the scratch of an ordered pack (vg_compact.hpp): the count of every block, their scanned offsets, and one total per slot
// with its pinned copy.  A slot is one scan: a level of a pyramid, an item of a batch ([item][block] counts), or the only one.
// The count and place launches stay with the pipeline; between them it calls scan() per slot, and fetch() behind the last.
struct PackScratch {
    Grow<unsigned> counts, offsets, totals;
    GrowPinned<unsigned> h_totals;
    int grow(size_t blocks, size_t slots, const char *what)
    {
        if (const int rc = counts.grow(blocks, what)) return rc;
        if (const int rc = offsets.grow(blocks, what)) return rc;
        if (const int rc = totals.grow(slots, what)) return rc;
        return h_totals.grow(slots, what);
    }
    // offsets and totals[slot] of the first nb counts
    template <int LANES>
    void scan(hipStream_t stream, int nb, int slot) const
    {
        hipLaunchKernelGGL(vgc::scan_block_counts_kernel<LANES>, dim3(1), dim3(LANES), 0, stream, (const unsigned *)counts.get(), offsets.get(), nb,
                           totals.get() + slot);
    }
    // queues the copy of the first `slots` totals to h_totals
    int fetch(hipStream_t stream, size_t slots) const
    {
        VG_HIP(hipMemcpyAsync(h_totals.get(), totals.get(), slots * sizeof(unsigned), hipMemcpyDeviceToHost, stream));
        return VG_OK;
    }
};

}  // namespace vgi
