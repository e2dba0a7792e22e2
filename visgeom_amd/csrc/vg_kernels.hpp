// vg_kernels.hpp -- HIP kernels of the residual / Jacobian hot path (gfx950, wave64).
//
//   kernel 1  vg_chain_prep_multi_kernel   one lane per residual block (image) of every dataset: transform chain -> frame
//   kernel 2  vg_emit_kernel         one lane per (image, corner) observation: residual pair +
//                                    the 2 x (K + 6L) Jacobian rows, written in the Ceres block layout
//
// Both are HBM-streaming kernels (about 1 flop per byte); nothing here is GEMM shaped.  Design notes
// and the roofline arithmetic are in DESIGN.md sections 4-5.
#pragma once

#include "vg_camera.hpp"

namespace vg {

constexpr int kMaxChain = 5;
constexpr int kEmitThreads = 256;  // 4 waves
constexpr int kWave = 64;
constexpr double kDoubleBig = 1e15;  // include/std.h:71

// where chain member l of block b lives:  params + base[l] + stride[l] * seq_index[b]
// (stride 0 = global transform, 6 = sequence transform; unified_calibration.h:161-165)
struct ChainDesc {
    int L;
    int status[kMaxChain];
    long long base[kMaxChain];
    long long stride[kMaxChain];
};

// ------------------------------------------------------------------------------------------
// kernel 1: chain prep (vg_chain_prep_multi_kernel below; a table variant for problems of more than kPrepMax datasets).  64-thread
// workgroups so that 10 k images spread over ~157 CUs with one wave each: the small launches are latency bound (a dependent
// chain of sqrt / sincos / divisions), the large ones (>= 512 waves) bandwidth bound on their frame stores.
// ------------------------------------------------------------------------------------------
// all datasets of a problem in ONE launch: the kernel is latency bound, so four datasets cost the same ~7 us as one
struct PrepDataset {
    ChainDesc chain;
    const int *seq_index;
    double *frames;
    long long first;   // global index of the dataset's first block (host bookkeeping)
    long long count;
    int frame_stride_d;
};

// Up to kPrepMax datasets travel BY VALUE in the kernel arguments and every wave belongs to ONE dataset (each dataset's lanes
// are padded to whole waves): the wave finds its dataset with scalar compares and reads the descriptor -- chain length,
// directions, bases, strides, frame pointer -- with scalar loads from the kernel-argument segment.  Round 4's kernel read a
// descriptor TABLE in global memory per lane: `first` of the next dataset -> the descriptor's pointers -> seq_index[b] ->
// base / stride -> the parameters were five dependent memory round trips in front of a two-microsecond walk (8.4-11.9 us per
// launch, SQ "wait any" 0.56); now the parameters are the first vector load.
constexpr int kPrepMax = 8;
struct PrepMultiArgs {
    PrepDataset ds[kPrepMax];
    unsigned int first_wave[kPrepMax + 1];  // first wave (= 64-thread workgroup) of each dataset in this launch
    int n;
    int staged;   // 1: the frames leave through LDS as linear 16-byte stores (launches of >= kPrepStagedMinWaves waves: bandwidth matters)
};
constexpr unsigned int kPrepStagedMinWaves = 512;   // 32 768 images

#ifdef VG_TU_EMIT  // these kernels are launched by one translation unit only; the others see the header without them
// problems of more than kPrepMax datasets: the descriptors in a table in global memory, one lane per block across all datasets
__global__ __launch_bounds__(64) void vg_chain_prep_table_kernel(const double *__restrict__ params,
                                                                  const PrepDataset *__restrict__ dsets, int n_dsets,
                                                                  long long total_blocks)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total_blocks) return;
    int d = 0;
    while (d + 1 < n_dsets && t >= dsets[d + 1].first) d++;
    const PrepDataset *D = dsets + d;
    const long long b = t - D->first;
    const int *seq = D->seq_index;
    const long long si = seq ? (long long)seq[b] : b;
    const long long *base = D->chain.base, *stride = D->chain.stride;
    build_frame(D->chain.L, D->chain.status, [&](int l) { return params + base[l] + stride[l] * si; },
                D->frames + b * D->frame_stride_d);
}

// All members' parameters are requested in one round in front of the walk.  Large launches (m.staged): the wave's 64 frames are
// staged in LDS (dynamic: 64 x the launch's widest frame) and leave as one linear run of 16-byte stores -- written by the lanes
// themselves, every lane its own 264-byte frame, the kernel ran at 1.3 TB/s and cost 20 us per 100 k images, 214 us at 1 M
// (now 13 / 67 us; profiles/r06_emit_drop.md).
__global__ __launch_bounds__(64) void vg_chain_prep_multi_kernel(const double *__restrict__ params, PrepMultiArgs m)
{
    using d2 = HIP_vector_type<double, 2>;
    extern __shared__ __attribute__((aligned(16))) double prep_tile[];
    int d = 0;
    while (d + 1 < m.n && blockIdx.x >= m.first_wave[d + 1]) d++;
    const PrepDataset &D = m.ds[d];
    const long long b0 = (long long)(blockIdx.x - m.first_wave[d]) * 64;
    const long long b = b0 + threadIdx.x;
    const int stride = D.frame_stride_d, L = D.chain.L;
    if (b < D.count) {
        const int *seq = D.seq_index;
        const long long si = seq ? (long long)seq[b] : b;
        double xi[kMaxChain][6];
#pragma unroll
        for (int l = 0; l < kMaxChain; l++)
            if (l < L) {
                const double *src = params + D.chain.base[l] + D.chain.stride[l] * si;
#pragma unroll
                for (int k = 0; k < 6; k++) xi[l][k] = src[k];
            }
        auto walk = [&](double *frame) {   // build_frame(), its member loop unrolled over the preloaded members
            ChainState s;
            chain_state_init(s);
#pragma unroll
            for (int l = 0; l < kMaxChain; l++)
                if (l < L) {
                    const Quat q1 = chain_acc_quat(s);
                    chain_walk_member(s, q1, xi[l], D.chain.status[l] != 0, frame + 12 + 21 * l);
                }
            chain_finish(s, frame);
        };
        // small launches (a stereo pair's 64 waves, a rig's 316) are pure latency: their lanes store their frames themselves, as
        // before round 6 -- the LDS round trip would only add to the dependent chain (7.0 -> 7.6 us for the stereo pair)
        if (!m.staged) {
            walk(D.frames + b * stride);
            return;
        }
        walk(prep_tile + threadIdx.x * stride);
    }
    if (!m.staged) return;
    // one wave per workgroup: LDS executes its DS operations in order, only the compiler needs the fence
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const long long left = D.count - b0;
    const int total = (int)(left < 64 ? left : 64) * stride;   // doubles of this wave's frames, consecutive in memory
    double *dst = D.frames + b0 * stride;
    if ((reinterpret_cast<unsigned long long>(dst) & 15ull) == 0) {
        for (int i = threadIdx.x; i < (total >> 1); i += 64) reinterpret_cast<d2 *>(dst)[i] = reinterpret_cast<const d2 *>(prep_tile)[i];
        if ((total & 1) && threadIdx.x == 0) dst[total - 1] = prep_tile[total - 1];
    } else {
        for (int i = threadIdx.x; i < total; i += 64) dst[i] = prep_tile[i];
    }
}
#endif

// ------------------------------------------------------------------------------------------
// kernel 2: emit.
// ------------------------------------------------------------------------------------------
struct EmitArgs {
    const double *frames;  // [n_blocks][frame_stride]
    const double *board;   // [N][3]
    const double *obs;     // [n_blocks][N][2]
    const double *intr;    // [K]
    double *res;           // [n_blocks][2N]
    double *jac_intr;      // [n_blocks][2N][K] or NULL
    double *jac_member[kMaxChain];  // [n_blocks][2N][6] or NULL
    unsigned long long *failed;     // failed-projection counter word: (epoch << 40) | count  (may be NULL)
    unsigned long long epoch;       // evaluation number (24 bits); a stale epoch in the word means count 0
    // INLINE_CHAIN variant only (single-member DIRECT chain): where the member's 6-vector of image b of this launch
    // lives: chain_params + chain_stride * (seq_index ? seq_index[b] : first_block + b)
    const double *chain_params;
    const int *seq_index;
    long long chain_stride;
    long long first_block;
    unsigned int n_obs;    // n_blocks * N  (< 2^31 per launch; the host chunks larger problems)
    unsigned int N;
    int L;
    int frame_stride_d;
    int nt_stores;         // store policy of the launch (EmitStorePolicy): 1 = past the Infinity Cache, non-temporal; 2 = inside it, write-through
    unsigned int map_window;  // tile map of the launch: 0 = every XCD one contiguous eighth of the tiles; W > 0 = windows of 8 W tiles,
                              // XCD x the x-th run of W tiles in each window (W = 1: the linear map); xcd_window_block, kEmitMapWindow
#ifdef VG_EMIT_STAMPS   // measurement build (tools/exp/emit_stamps_probe.py): kEmitStampsPerWave wall-clock stamps (100 MHz) per wave of the launch, or NULL
    unsigned long long *stamps;
    unsigned long long stamps_waves;   // waves the buffer holds: a launch with more stamps only those
#endif
};

#ifdef VG_EMIT_STAMPS
// stamp k of this wave: 0 entry, 1 after the barrier, 2 at the first store, 3 after the last store; the two store-less intervals
// split: 4 chain-parameter load issued, 5 its data arrived (start of the walk; walking waves only), 6 intrinsics in registers
// (behind the barrier); an ordinary vector store of lane 0
constexpr int kEmitStampsPerWave = 8;
__device__ __forceinline__ void emit_stamp(const EmitArgs &a, int k)
{
    const unsigned long long w = (unsigned long long)blockIdx.x * (kEmitThreads / kWave) + (threadIdx.x >> 6);
    if (a.stamps && w < a.stamps_waves && (threadIdx.x & (kWave - 1)) == 0) a.stamps[w * kEmitStampsPerWave + k] = wall_clock64();
}
#define VG_EMIT_STAMP(a, k) emit_stamp(a, k)
// the stamp behind it is taken once these values have arrived
#define VG_EMIT_STAMP_ARRIVED6(x) asm volatile("" ::"v"((x)[0]), "v"((x)[1]), "v"((x)[2]), "v"((x)[3]), "v"((x)[4]), "v"((x)[5]))
#else
#define VG_EMIT_STAMP(a, k) ((void)0)
#define VG_EMIT_STAMP_ARRIVED6(x) ((void)0)
#endif

// Each lane holds the 2S doubles of its observation's two rows; the wave's 64 observations are one
// contiguous 1024*S-byte run of the output.  Lanes write their rows to the wave's private LDS tile
// (16 B stores at a 16*S-byte lane stride) and the tile is then streamed out linearly, 16 B per lane
// per store -> every global store instruction writes 1 KiB of consecutive bytes.
// The 16-byte store of the output stream, plain or with the non-temporal hint (`global_store_dwordx4 ... nt`), chosen per LAUNCH by
// the host (EmitArgs::nt_stores, which selects the kernel instantiation).  A launch whose output fits the 256 MiB Infinity Cache keeps plain
// stores: the consumer (second-pass Gram, a copy engine, the next evaluation overwriting the same rows) finds the lines there.
// A launch that streams past the cache sets the hint: a line kept behind the write only displaces the next lines of the same
// stream (same box, alternating builds, profiles/r05c_emit_sweep_ab.txt: EUCM 12.5 k images = 250 MB 57 -> 45 us, 25 k 105 -> 83,
// 50 k = 1 GB 201 -> 159 us, 0.67 -> 0.84 of the HBM peak; inside the cache the hint costs: 10 k images 36 -> 41 us).
// A launch inside the cache can instead write through (kStoreWriteThrough, `sc1`): the lines leave the XCD's L2 as they are
// written instead of staying dirty behind the write, and the 215 MB headline write ran 31.0 -> 29.9 us that way
// (tools/exp/store_policy.hip, profiles/r10_emit_store_policy.txt).
enum EmitStorePolicy { kStorePlain = 0, kStoreNonTemporal = 1, kStoreWriteThrough = 2 };

// The policy is a template parameter (of the emit kernels, per launch): a tile's store sequence is straight-line code, not a
// three-way dispatch per 16-byte store.
template <int POLICY>
__device__ __forceinline__ void stream_store16(HIP_vector_type<double, 2> *dst, const HIP_vector_type<double, 2> &v)
{
    if constexpr (POLICY == kStoreNonTemporal) {
        __builtin_nontemporal_store(v.x, &dst->x);
        __builtin_nontemporal_store(v.y, &dst->y);
    } else if constexpr (POLICY == kStoreWriteThrough) {
        // hipcc has no builtin for a flat-address `sc1` store; the trailing nop keeps the data registers intact until the store
        // has read them (the compiler does not pad an asm statement's hazards)
        typedef unsigned int u4 __attribute__((ext_vector_type(4)));
        asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(dst), "v"(__builtin_bit_cast(u4, v)) : "memory");
    } else {
        *dst = v;
    }
}

// Streams the n16 16-byte words of a staged row block out, word idx = k * 64 + lane by store k.  Inside the Infinity Cache
// (plain or write-through stores) the block's LDS reads are issued together ahead of its stores, which then wait on counted
// lgkmcnt instead of one ds_read round trip each.  Reading the tile past n16 only reads stale LDS of the wave's own tile;
// those words are not stored.  A full block (every wave of a launch but its last) stores unpredicated: with a per-lane
// branch around each store the compiler would sink the first read into its branch, behind the others.
// Non-temporal launches stream to DRAM and keep one LDS read per store: with the reads ahead the 2 GB launch (EUCM 100 k
// images) ran 329 us against 290 us this way and 313 us before either (same box, alternating; profiles/r11_emit_waits.md).
template <int NK, int POLICY>
__device__ __forceinline__ void stream_tile_out(const HIP_vector_type<double, 2> *st, HIP_vector_type<double, 2> *dst, int n16, int lane)
{
    using d2 = HIP_vector_type<double, 2>;
    if constexpr (POLICY == kStoreNonTemporal) {
#pragma unroll
        for (int k = 0; k < NK; k++) {
            const int idx = k * kWave + lane;
            if (idx < n16) stream_store16<POLICY>(dst + idx, st[idx]);
        }
        return;
    }
    d2 v[NK];
#pragma unroll
    for (int k = 0; k < NK; k++) v[k] = st[k * kWave + lane];
    if (n16 >= NK * kWave) {
#pragma unroll
        for (int k = 0; k < NK; k++) stream_store16<POLICY>(dst + k * kWave + lane, v[k]);
    } else {
#pragma unroll
        for (int k = 0; k < NK; k++) {
            const int idx = k * kWave + lane;
            if (idx < n16) stream_store16<POLICY>(dst + idx, v[k]);
        }
    }
}

template <int S, int POLICY = kStorePlain>
__device__ __forceinline__ void wave_store_rows(double *__restrict__ stage, const double *vals,
                                                double *__restrict__ out_tile, int n_valid_obs, int lane)
{
    using d2 = HIP_vector_type<double, 2>;
    d2 *st = reinterpret_cast<d2 *>(stage);
#pragma unroll
    for (int i = 0; i < S; i++) {
        d2 v;
        v.x = vals[2 * i];
        v.y = vals[2 * i + 1];
        st[lane * S + i] = v;
    }
    // wave-private tile: LDS executes one wave's DS ops in order, only the compiler needs fencing
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    stream_tile_out<S, POLICY>(st, reinterpret_cast<d2 *>(out_tile), n_valid_obs * S, lane);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Same tile for every model: rows wider than a pose block (Mei, K = 10) are staged in two half-waves of 32
// observations each, so the LDS footprint -- and with it the number of resident waves that keep stores in flight --
// does not depend on K (with a 10 KiB tile per wave only 3 workgroups fit a CU and Mei streamed at 5.2 TB/s).
constexpr int kStageRowDoubles = 6;

template <int MODEL>
constexpr int emit_stage_doubles_per_wave()
{
    return 2 * kWave * kStageRowDoubles;
}

// wave_store_rows for S > kStageRowDoubles: lanes [32h, 32h + 32) stage their rows, the whole wave streams the
// 32 * 16 * S contiguous bytes out, h = 0, 1.
template <int S, int POLICY>
__device__ __forceinline__ void wave_store_rows_halves(double *__restrict__ stage, const double *vals,
                                                       double *__restrict__ out_tile, int n_valid_obs, int lane)
{
    static_assert(S <= 2 * kStageRowDoubles, "half a wave of rows must fit the tile");
    using d2 = HIP_vector_type<double, 2>;
    d2 *st = reinterpret_cast<d2 *>(stage);
    constexpr int kHalf = kWave / 2;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        if ((lane >> 5) == h) {
#pragma unroll
            for (int i = 0; i < S; i++) {
                d2 v;
                v.x = vals[2 * i];
                v.y = vals[2 * i + 1];
                st[(lane & (kHalf - 1)) * S + i] = v;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        int nv = n_valid_obs - h * kHalf;
        nv = nv < 0 ? 0 : (nv > kHalf ? kHalf : nv);
        stream_tile_out<(kHalf * S + kWave - 1) / kWave, POLICY>(st, reinterpret_cast<d2 *>(out_tile) + h * kHalf * S, nv * S, lane);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// Workgroup -> tile mapping for the streaming kernels.  Block b runs on XCD b % 8 (observed dispatch order, used for
// speed only -- any mapping is correct).  Handing XCD x the x-th contiguous eighth of the output instead of every
// eighth tile keeps each die's write stream in its own address range: the same 2.15 GB streaming write runs at
// 6.63 TB/s instead of 6.02 TB/s (tools/exp/store_sweep.hip); below the 256 MiB Infinity Cache it makes no difference.
__device__ __forceinline__ unsigned int xcd_contiguous_block(unsigned int b, unsigned int n)
{
    constexpr unsigned int kXcds = 8;
    const unsigned int x = b % kXcds, j = b / kXcds, q = n / kXcds, r = n % kXcds;
    return x * q + (x < r ? x : r) + j;  // bijective on [0, n): XCD x owns q (+1 for x < r) consecutive tiles
}

// The same with the dies advancing TOGETHER through the output: the tiles are cut into windows of 8 W tiles and XCD x owns the
// x-th run of W consecutive tiles of every window; the last, partial window is split into contiguous eighths like the whole
// range above.  W >= n / 8 is xcd_contiguous_block, W = 1 the linear map.  Bijective on [0, n).
// Why (profiles/r06_emit_drop.md): with one contiguous eighth per die a 2 GB evaluation keeps 8 x 3 write cursors >= 110 MB
// apart, and on most boxes / placements that costs a tenth of the rate (EUCM 100 k images 395 us against 362 us with W = 16
// on the same box and arrays; where the eighths run at full rate, 341 us, the windows give 344 us); inside the Infinity Cache
// the maps do not differ.  The counters say it is the DRAM side: no address-translation misses (TCP_UTCL1_TRANSLATION_MISS
// 1e3 of 4e7 requests), FEWER L2 -> fabric credit stalls and fewer writes in flight than at 1 GB, i.e. requests retire slower.
constexpr unsigned int kEmitMapWindow = 16;   // runs of 16 tiles: 384 KiB of a 6-column Jacobian array per die and window (launches >= 1.2 GB: emit_map_window, vg_emit_launch.hpp)
__device__ __forceinline__ unsigned int xcd_window_block(unsigned int b, unsigned int n, unsigned int W)
{
    const unsigned int x = b & 7u, j = b >> 3, w = j / W, i = j - w * W, base = w * 8u * W, rem = n - base;
    if (rem >= 8u * W) return base + x * W + i;
    const unsigned int q = rem >> 3, r = rem & 7u;
    return base + x * q + (x < r ? x : r) + i;
}

// The Jacobian row blocks of one tile (WANT_JAC), after its residual pair has left: the intrinsic and pose row blocks through the wave's
// LDS tile.  With the frames in LDS nothing waits on vmcnt from the tile's first store on: every global load was consumed before it.
// ONE_MEMBER (an INLINE_CHAIN tile with its state fetched at entry: the chain is one member, dataset_can_inline_chain): no member loop,
// no fetch of L, jac_member[0] only.
template <int MODEL, bool WANT_JAC, int POLICY, bool ONE_MEMBER = false>
__device__ __forceinline__ void emit_tile_rows(const EmitArgs &a, const unsigned int o0, const unsigned int o_end,
                                                 const CornerEval<CameraTraits<MODEL>::K> &e, double X0, double X1, double X2,
                                                 const double *fr, double *stage)
{
    constexpr int K = CameraTraits<MODEL>::K;
    const int lane = threadIdx.x & (kWave - 1);
    if (WANT_JAC) {
        const unsigned int ow = o0 + (threadIdx.x & ~(kWave - 1));  // first observation of this wave
        int n_valid = 0;
        if (ow < o_end) n_valid = (o_end - ow < (unsigned)kWave) ? (int)(o_end - ow) : kWave;

        // intrinsic block, rows 2i / 2i+1 of [2N x K]       calib_cost_functions.cpp:105-114
        if (a.jac_intr) {
            double rows[2 * K];
#pragma unroll
            for (int i = 0; i < K; i++) {
                rows[i] = e.Ju[i];
                rows[K + i] = e.Jv[i];
            }
            if (K > kStageRowDoubles) wave_store_rows_halves<K, POLICY>(stage, rows, a.jac_intr + (size_t)ow * (2 * K), n_valid, lane);
            else wave_store_rows<(K > kStageRowDoubles ? 1 : K), POLICY>(stage, rows, a.jac_intr + (size_t)ow * (2 * K), n_valid, lane);
        }
        // pose blocks, u-row at +12i, v-row at +12i+6       calib_cost_functions.cpp:93-101
        if constexpr (ONE_MEMBER) {
            if (double *Jm = a.jac_member[0]) {
                double rows[12];
                pose_rows(e.P, X0, X1, X2, fr + 12, rows);
                wave_store_rows<6, POLICY>(stage, rows, Jm + (size_t)ow * 12, n_valid, lane);
            }
        } else {
            for (int l = 0; l < a.L; l++) {
                double *Jm = a.jac_member[l];
                if (!Jm) continue;
                double rows[12];
                pose_rows(e.P, X0, X1, X2, fr + 12 + 21 * l, rows);
                wave_store_rows<6, POLICY>(stage, rows, Jm + (size_t)ow * 12, n_valid, lane);
            }
        }
    }
}

// Wave-uniform state of a tile whose state is fetched at entry (ENTRY_STATE below).  Left alone, the compiler fetches every kernel
// argument with an s_load of its own at the point of first use, each behind its own `s_waitcnt lgkmcnt(0)` -- a wait that also drains
// the wave's LDS reads, SMEM and LDS share the counter -- eleven dependent round trips in front of a tile's first store and three more
// between its stores (profiles/r15_emit_scalar_head.md).  One statement consumes every field the instantiation uses as an SGPR input:
// the loads become a few wide ones in the entry block behind ONE wait (the grid size of the tile map, a hidden argument, with them).
// `epoch` is not listed: only the failed-projection CAS block reads it.  (Input-only constraints: an in/out "+s" does not compile,
// "illegal VGPR to SGPR copy".)
template <bool WANT_JAC>
__device__ __forceinline__ void emit_fetch_args(const EmitArgs &a)
{
    if constexpr (WANT_JAC)
        asm volatile("" ::"s"(a.board), "s"(a.obs), "s"(a.intr), "s"(a.res), "s"(a.jac_intr), "s"(a.jac_member[0]), "s"(a.failed),
                     "s"(a.chain_params), "s"(a.seq_index), "s"(a.chain_stride), "s"(a.first_block), "s"(a.n_obs), "s"(a.N),
                     "s"(a.frame_stride_d), "s"(a.map_window), "s"(gridDim.x));
    else
        asm volatile("" ::"s"(a.board), "s"(a.obs), "s"(a.intr), "s"(a.res), "s"(a.failed), "s"(a.chain_params), "s"(a.seq_index),
                     "s"(a.chain_stride), "s"(a.first_block), "s"(a.n_obs), "s"(a.N), "s"(a.frame_stride_d), "s"(a.map_window), "s"(gridDim.x));
}

// The camera's intrinsics, loaded through EmitArgs::intr at entry, held in SGPRs from here on: one statement, one wait.
template <int K>
__device__ __forceinline__ void emit_pin_intrinsics(const double *x)
{
    static_assert(K == 5 || K == 6 || K == 8 || K == 10, "UCM, EUCM / double sphere, Kannala-Brandt, Mei");
    if constexpr (K == 5) asm volatile("" ::"s"(x[0]), "s"(x[1]), "s"(x[2]), "s"(x[3]), "s"(x[4]));
    else if constexpr (K == 6) asm volatile("" ::"s"(x[0]), "s"(x[1]), "s"(x[2]), "s"(x[3]), "s"(x[4]), "s"(x[5]));
    else if constexpr (K == 8) asm volatile("" ::"s"(x[0]), "s"(x[1]), "s"(x[2]), "s"(x[3]), "s"(x[4]), "s"(x[5]), "s"(x[6]), "s"(x[7]));
    else asm volatile("" ::"s"(x[0]), "s"(x[1]), "s"(x[2]), "s"(x[3]), "s"(x[4]), "s"(x[5]), "s"(x[6]), "s"(x[7]), "s"(x[8]), "s"(x[9]));
}

// dynamic LDS: 4 wave tiles, then (FRAMES_LDS) the frames of the images this workgroup touches
// INLINE_CHAIN (with FRAMES_LDS, chain = one DIRECT member): the workgroup derives the <= 4 frames it needs itself
// (thread f walks image b_first + f with build_frame_single_direct) instead of reading them from the chain-prep
// kernel's output -- a full evaluation is then ONE launch.
// One 256-observation tile of one dataset (o0 = first observation of the tile), its stores of policy POLICY (EmitStorePolicy).
// HEAD_FIRST (the single-dataset kernel): the tile is ordered for an early first store -- the chain parameters are its first load and
// the residual pair leaves before the Jacobian arithmetic.  The merged kernel keeps the plain order: with the early order its stereo
// launch ran 18.5-18.7 us against the parent's 18.1 and the rig's 100.3-101.1 against 99.4-99.5 (profiles/r14_emit_head_tail.md).
// ENTRY_STATE (the single-dataset kernel's INLINE_CHAIN tiles): the rule of the tile is that wave-uniform state is fetched at entry
// and nothing scalar lies behind the first vector access.  The kernel has consumed the arguments (emit_fetch_args) and issued the
// loads of the intrinsics (intr_entry) before it calls; the intrinsics' round trip overlaps the chain-parameter load and the walk and
// is waited for once, in front of the barrier.  The chain has one member at compile time.  Only the failed-projection CAS block (rare)
// may still fetch: the epoch (tests/test_emit_scalar_head_isa_cpu.py).
template <int MODEL, bool WANT_JAC, bool FRAMES_LDS, bool INLINE_CHAIN, int POLICY, bool HEAD_FIRST = false, bool ENTRY_STATE = false>
__device__ __forceinline__ void emit_tile(const EmitArgs &a, const unsigned int o0, const double *intr_entry = nullptr)
{
    static_assert(!ENTRY_STATE || INLINE_CHAIN, "the entry fetch is built for the tiles that walk their chain");
    VG_EMIT_STAMP(a, 0);
    static_assert(!INLINE_CHAIN || FRAMES_LDS, "the inline chain writes its frames to LDS");
    constexpr int K = CameraTraits<MODEL>::K;
    using d2 = HIP_vector_type<double, 2>;
    extern __shared__ __attribute__((aligned(16))) double smem[];

    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wave = tid >> 6;
    const unsigned int o_end = o0 + kEmitThreads < a.n_obs ? o0 + kEmitThreads : a.n_obs;   // o0 < n_obs
    const unsigned int b_first = o0 / a.N;

    // INLINE_CHAIN, HEAD_FIRST: the walk is the longest dependent chain in front of the tile's first store; its parameters are the first load of
    // the kernel, ahead of the per-lane address arithmetic (an integer division by the run-time N) of the board / observation loads.
    // A tile of 256 consecutive observations touches at most 256 images: at most one frame per thread (as a loop the walk was
    // scheduled across iterations and cost 16 more VGPRs: 114 instead of 98).
    const unsigned int nf = (o_end - 1) / a.N - b_first + 1;
    double xi_r[6];
    auto load_chain_params = [&]() {
        if ((unsigned)tid < nf) {
            const long long bi = (long long)b_first + tid;
            const long long si = a.seq_index ? (long long)a.seq_index[bi] : a.first_block + bi;
#pragma unroll
            for (int k = 0; k < 6; k++) xi_r[k] = (a.chain_params + a.chain_stride * si)[k];
        }
    };
    if (INLINE_CHAIN && HEAD_FIRST) {
        load_chain_params();
        VG_EMIT_STAMP(a, 4);
    }

    const unsigned int o = o0 + tid;
    const bool active = o < o_end;
    const unsigned int oc = active ? o : o_end - 1;
    const unsigned int b = oc / a.N;
    const unsigned int c = oc - b * a.N;

    // issued before the frames are staged / derived: their latency overlaps the barrier below
    const double g0 = a.board[3 * c], g1 = a.board[3 * c + 1], g2 = a.board[3 * c + 2];
    const d2 ob = reinterpret_cast<const d2 *>(a.obs)[oc];

    const double *fr;
    if (FRAMES_LDS) {
        double *fr_lds = smem + (kEmitThreads / kWave) * emit_stage_doubles_per_wave<MODEL>();
        if (INLINE_CHAIN) {
            if (!HEAD_FIRST) {
                load_chain_params();
                VG_EMIT_STAMP(a, 4);
            }
            if (const unsigned int f = tid; f < nf) {
                VG_EMIT_STAMP_ARRIVED6(xi_r);
                VG_EMIT_STAMP(a, 5);
                {   // The short walk of the Gram kernels (one sincos at the half angle, R12 = I, M12 from uhat^2 = u u^T - I: the
                    // reference's frame to 1e-16; inside and just above its first-order branches it IS the reference-order
                    // routine).  While <= 4 lanes walk, the tile's other 252 wait at the barrier below with no store in
                    // flight: a third of the chain gone is 36.3 -> 34.1 us at 10 k images, 22.0 -> 19.8 at 5 k, 161 -> 152 at 50 k
                    // (same box, alternating; profiles/r06q_emit_fastwalk_ab.txt).  The corner arithmetic stays in reference order.
                    build_frame_single_direct_fast(xi_r, fr_lds + f * a.frame_stride_d);
                }
            }
        } else {
            const int n16 = (int)(nf * (unsigned)a.frame_stride_d) >> 1;
            const d2 *src = reinterpret_cast<const d2 *>(a.frames + (size_t)b_first * a.frame_stride_d);
            d2 *dst = reinterpret_cast<d2 *>(fr_lds);
            for (int i = tid; i < n16; i += kEmitThreads) dst[i] = src[i];
        }
        if constexpr (ENTRY_STATE) emit_pin_intrinsics<K>(intr_entry);
        __syncthreads();
        VG_EMIT_STAMP(a, 1);
        fr = fr_lds + (b - b_first) * a.frame_stride_d;
    } else {
        fr = a.frames + (size_t)b * a.frame_stride_d;
    }

    // pointCam = R(xiAcc.rot) * grid + xiAcc.trans     calib_cost_functions.cpp:49-50
    const double X0 = (fr[0] * g0 + fr[1] * g1 + fr[2] * g2) + fr[9];
    const double X1 = (fr[3] * g0 + fr[4] * g1 + fr[5] * g2) + fr[10];
    const double X2 = (fr[6] * g0 + fr[7] * g1 + fr[8] * g2) + fr[11];

    // HEAD_FIRST: the projection alone first: the residual pair leaves before the Jacobian arithmetic below starts (the same operations in the
    // same order per value as in one eval_corner<.., WANT_JAC, WANT_JAC>: what the two calls share is computed once, here).
    // The intrinsics are read once, into registers: the store below is a memory barrier to the compiler, and a second read behind it
    // would be a global load the wave waits for with its own store in flight.
    double intr[K];
#pragma unroll
    for (int i = 0; i < K; i++) intr[i] = ENTRY_STATE ? intr_entry[i] : a.intr[i];
#ifdef VG_EMIT_STAMPS
#pragma unroll
    for (int i = 0; i < K; i++) asm volatile("" ::"v"(intr[i]));
    VG_EMIT_STAMP(a, 6);
#endif
    CornerEval<K> e;
    if (HEAD_FIRST) eval_corner<MODEL, false, false>(intr, X0, X1, X2, e);
    else eval_corner<MODEL, WANT_JAC, WANT_JAC>(intr, X0, X1, X2, e);

    // residual pair, or the in-band failure value       calib_cost_functions.cpp:57-71
    d2 r;
    r.x = e.ok ? e.u - ob.x : kDoubleBig;
    r.y = e.ok ? e.v - ob.y : kDoubleBig;
    // Pins the residual pair (and with it the observation load) here, ahead of every store.  Left alone, the compiler sinks
    // the two subtractions into the `if (active)` below; the load's vmcnt wait then sits on one path only, and at the join the
    // waitcnt pass still counts the load as pending and waits vmcnt(0) -- for the wave's own stores -- before it reuses the
    // load's registers.  With the load consumed before the first store, no vmcnt wait follows it (tests/test_emit_isa_cpu.py).
    asm volatile("" ::"v"(r.x), "v"(r.y));

    if (a.failed) {
        // Failures are rare: the counter is never zeroed (an 8-byte hipMemsetAsync is a whole 5 us fill
        // kernel).  The word carries the evaluation epoch; the first failing wave of an evaluation
        // replaces a stale word, later ones add to it.
        const unsigned long long m = __ballot(active && !e.ok);
        if (m && lane == 0) {
            const unsigned long long n = (unsigned long long)__popcll(m);
            unsigned long long old = *a.failed, assumed;
            do {
                assumed = old;
                const unsigned long long cnt = (assumed >> 40) == a.epoch ? (assumed & ((1ull << 40) - 1)) + n : n;
                old = atomicCAS(a.failed, assumed, (a.epoch << 40) | cnt);
            } while (old != assumed);
        }
    }

    VG_EMIT_STAMP(a, 2);
    if (active) stream_store16<POLICY>(reinterpret_cast<d2 *>(a.res) + o, r);

    if (WANT_JAC) {
        if (HEAD_FIRST) eval_corner<MODEL, true, true>(intr, X0, X1, X2, e);
        emit_tile_rows<MODEL, WANT_JAC, POLICY, ENTRY_STATE>(a, o0, o_end, e, X0, X1, X2, fr, smem + wave * emit_stage_doubles_per_wave<MODEL>());
    }
    VG_EMIT_STAMP(a, 3);
}

// POLICY: the launch's store policy (EmitArgs::nt_stores), a template argument so that the tile's stores are straight-line code
template <int MODEL, bool WANT_JAC, bool FRAMES_LDS, bool INLINE_CHAIN, int POLICY>
#ifndef VG_EMIT_WAVES
#define VG_EMIT_WAVES 4    // waves per SIMD the register allocation of the emit kernels aims at (experiment switch, profiles/NOTES.md)
#endif
#ifndef VG_EMIT_MULTI_WAVES
#define VG_EMIT_MULTI_WAVES 4
#endif
__global__ __launch_bounds__(kEmitThreads) __attribute__((amdgpu_waves_per_eu(VG_EMIT_WAVES, 8))) void vg_emit_kernel(EmitArgs a)
{
    // INLINE_CHAIN: every argument the tile uses in SGPRs behind one wait, then the intrinsics behind their pointer (emit_tile,
    // ENTRY_STATE).  The prepared-frames instantiations keep the fetch at first use and the run-time member loop.
    constexpr int K = CameraTraits<MODEL>::K;
    double intr[K];
    if constexpr (INLINE_CHAIN) {
        emit_fetch_args<WANT_JAC>(a);
        // Nothing writes the parameters while an evaluation reads them: read through the constant address space, the intrinsics are scalar
        // loads (a plain load behind the statement above becomes a vector load into 2 K VGPRs: the statement counts as a write).
        // volatile: the loads stay in the entry block; left free, the compiler sinks Mei's ten doubles behind the chain-parameter load.
        const volatile __attribute__((address_space(4))) double *ci = (const volatile __attribute__((address_space(4))) double *)a.intr;
#pragma unroll
        for (int i = 0; i < K; i++) intr[i] = ci[i];
    }
    const unsigned int t = a.map_window ? xcd_window_block(blockIdx.x, gridDim.x, a.map_window) : xcd_contiguous_block(blockIdx.x, gridDim.x);
    emit_tile<MODEL, WANT_JAC, FRAMES_LDS, INLINE_CHAIN, POLICY, true, INLINE_CHAIN>(a, t * (unsigned)kEmitThreads, intr);
}

// ------------------------------------------------------------------------------------------
// kernel 2, several datasets in ONE launch (stereo pair, camera rig): a problem's datasets are small launches each
// (2 000 stereo pairs: 42 + 62 MB) whose ramp-up, drain and inter-kernel gap cost a quarter of the pass.  The tiles of
// all datasets form one range; XCD x streams its share of EVERY dataset (the x-th eighth of its tiles, cut into runs of
// kEmitMapWindow tiles: xcd_window_block), dataset after dataset, so a die
// works inside one dataset's output arrays at a time and every die gets the same bytes and the same arithmetic whatever the
// mix of models (a rig's Mei tile writes 1.85 x the bytes of its UCM tile: with one contiguous piece of equal tile count
// per die, the dies holding the wide datasets finished last -- rig, 591 MB: 116 us against 109 us; profiles/NOTES.md "Merged
// emit launch").  The grid is 8 x the sum of the datasets' longest eighths; surplus workgroups leave at once.  Per-dataset
// arguments travel by value in the kernel argument segment (no table upload per evaluation); the camera model and the chain
// route are wave-uniform run-time switches over the same tile routine.
// ------------------------------------------------------------------------------------------
constexpr int kEmitMultiMax = 8;

struct EmitMultiArgs {
    EmitArgs ds[kEmitMultiMax];
    unsigned int first_tile[kEmitMultiMax + 1];
    int model[kEmitMultiMax];
    int inline_chain[kEmitMultiMax];
    int n;
};

template <int MODEL, int POLICY>
__device__ __forceinline__ void emit_tile_route(const EmitArgs &a, unsigned int o0, bool inline_chain)
{
    if (inline_chain) emit_tile<MODEL, true, true, true, POLICY>(a, o0);
    else emit_tile<MODEL, true, true, false, POLICY>(a, o0);
}

// POLICY: the store policy of the launch, shared by all its datasets (emit_store_policy on the launch's summed output)
template <int POLICY>
__global__ __launch_bounds__(kEmitThreads) __attribute__((amdgpu_waves_per_eu(VG_EMIT_MULTI_WAVES, 8))) void vg_emit_multi_kernel(EmitMultiArgs m)
{
    const unsigned int x = blockIdx.x & 7u;   // workgroup b runs on XCD b % 8 (observed dispatch order)
    unsigned int j = blockIdx.x >> 3, t;
    int d = 0;
    for (;; d++) {
        if (d == m.n) return;
        const unsigned int nt = m.first_tile[d + 1] - m.first_tile[d], q = nt >> 3, r = nt & 7u, cnt = q + (x < r ? 1u : 0u);
        if (j < cnt) {
            const unsigned int W = m.ds[d].map_window;   // XCD x's j-th tile of this dataset
            t = m.first_tile[d] + (W ? xcd_window_block(j * 8u + x, nt, W) : x * q + (x < r ? x : r) + j);
            break;
        }
        j -= cnt;
    }
    const unsigned int o0 = (t - m.first_tile[d]) * (unsigned)kEmitThreads;
    const bool inl = m.inline_chain[d] != 0;
    switch (m.model[d]) {
    case kEUCM: emit_tile_route<kEUCM, POLICY>(m.ds[d], o0, inl); break;
    case kUCM: emit_tile_route<kUCM, POLICY>(m.ds[d], o0, inl); break;
    default: emit_tile_route<kMEI, POLICY>(m.ds[d], o0, inl); break;
    }
}

}  // namespace vg
