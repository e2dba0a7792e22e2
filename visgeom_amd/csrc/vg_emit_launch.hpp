// vg_emit_launch.hpp -- host side of the emit kernels (vg_kernels.hpp): everything that decides how an emit launch is made.
// The thresholds with their measurements, the store policy and the tile map, EmitArgs filling, the template dispatch and the
// two launch entries: launch_emit (one dataset, or a chunk of one) and launch_emit_merged (several datasets in one launch).
// Included by vg_emit_tu.hip; vg_dataset_evaluate, vg_problem_evaluate and the host route (vg_host_route.hpp) launch through it.
#pragma once

#include <vector>

#include "vg_internal.hpp"

using vgi::Camera;
using vgi::Dataset;
using vgi::fail;
using vgi::valid_dataset;

namespace {

// Largest evaluation (bytes of residuals + Jacobian rows + observations per launch) for which the emit kernel walks a
// single-member chain itself.  The in-kernel walk saves the chain-prep launch (~7 us + its boundary) and the frames' round trip
// through memory; it costs every workgroup ~2 us in front of its first store.  While the launch is absorbed by the Infinity Cache
// that is hidden -- whole step, same box, alternating (profiles/r06n_inline_vs_prep.txt, in-kernel walk / prep + emit): EUCM
// 35 k images 110 / 121 us, 50 k 156 / 167, 75 k (1.6 GB) 231 / 241; Mei 40 k 151 / 159, 60 k 248 / 257 -- but once the launch streams
// to DRAM the stores are latency bound and a workgroup that waits two microseconds before storing is bytes missing in flight:
// 85 k images (1.8 GB) 301 / 279 us, 100 k 430 / 360.  With the short walk in the tile (profiles/r06s_inline_vs_prep_fastwalk.txt, another
// box): 75 k 212 / 258, 85 k 239 / 304, 100 k 372 / 368, 150 k 556 / 549; Mei 70 k (1.9 GB) 306 / 315, 80 k 350 / 384 -- where the cache-assisted
// range ends depends on the box; 2.0 GB sits between the two.  Rounds 3-5 (before non-temporal stores, then before these A/Bs): 288 MB, 600 MB.
int64_t inline_chain_max_bytes()
{
    const long long h = vgi::debug_hook(vgi::kHookInlineChainMaxBytes);
    return h ? (int64_t)h : (int64_t)2000000000;
}

// Smallest output of a launch (bytes of residuals + Jacobian rows) that is written with non-temporal stores: everything that
// does not fit the 256 MiB Infinity Cache next to the observations it reads (stream_store16 in vg_kernels.hpp).
int64_t emit_nt_min_bytes()
{
    const long long h = vgi::debug_hook(vgi::kHookEmitNtMinBytes);
    return h ? (int64_t)h : (int64_t)230000000;
}

// Store policy of an emit launch (single-dataset or merged) by its output: non-temporal past the Infinity Cache (emit_nt_min_bytes), write-through
// inside it.  Write-through (`sc1`) leaves no dirty Jacobian lines in the XCD L2s for the launch's end to wait on
// (profiles/r10_emit_store_policy.txt); a merged launch (vg_emit_multi_kernel) decides by its summed output: the stereo pair's 104 MB step
// 25.05 -> 23.5 us with write-through, the rig's 591 MB stay non-temporal (profiles/r14_emit_head_tail.md).  hook emit_write_through: -1 = plain stores inside the cache (the policy before), 0 = the default.
int emit_store_policy(int64_t launch_output_bytes)
{
    if (launch_output_bytes >= emit_nt_min_bytes()) return vg::kStoreNonTemporal;
    return vgi::debug_hook(vgi::kHookEmitWriteThrough) < 0 ? vg::kStorePlain : vg::kStoreWriteThrough;
}

// Tile map of an emit launch by its output: one contiguous eighth per XCD while the launch stays inside or near the Infinity Cache
// (<= 1.2 GB: same box, alternating, the eighths are level with the windows for EUCM and 2 % ahead for Mei at 10 k images,
// profiles/r06l_headline_map_ab.txt), windows of 8 x kEmitMapWindow tiles beyond, where the eighths fall into their slow mode on
// most boxes (from ~1.6 GB; profiles/r06_emit_drop.md).  hook emit_map_window: W > 0 that window, -1 the eighths, whatever the size.
unsigned int emit_map_window(int64_t launch_output_bytes)
{
    const long long mw = vgi::debug_hook(vgi::kHookEmitMapWindow);
    if (mw) return mw > 0 ? (unsigned int)mw : 0u;
    return launch_output_bytes >= (int64_t)1200000000 ? vg::kEmitMapWindow : 0u;
}

int64_t emit_output_bytes(const vg::EmitArgs &a, int K)
{
    int64_t per_obs = 16;
    if (a.jac_intr) per_obs += 16 * K;
    for (int l = 0; l < a.L; l++)
        if (a.jac_member[l]) per_obs += 96;
    return per_obs * (int64_t)a.n_obs;
}

bool emit_frames_in_lds(int N, int frame_stride)
{
    const int max_frames = vg::kEmitThreads / N + 2;
    return (size_t)max_frames * frame_stride * sizeof(double) <= 32 * 1024;
}

template <int MODEL>
size_t emit_lds_bytes(bool frames_lds, int N, int frame_stride)
{
    // the tile region is always reserved so the frame region's offset does not depend on WANT_JAC
    size_t bytes = (size_t)(vg::kEmitThreads / vg::kWave) * vg::emit_stage_doubles_per_wave<MODEL>() * sizeof(double);
    if (frames_lds) bytes += (size_t)(vg::kEmitThreads / N + 2) * frame_stride * sizeof(double);
    return bytes;
}

bool dataset_can_inline_chain(const vg_problem *p, const Dataset &d)
{
    return d.L == 1 && d.status[0] == VG_TRANSFORM_DIRECT && emit_frames_in_lds(d.N, d.frame_stride) &&
           d.n_blocks * (int64_t)d.N * (32 + 16 * (p->cams[d.camera].K + 6)) <= inline_chain_max_bytes();
}

// The route of a dataset is a property of THAT dataset (and of the test hook), never of its neighbours or of what ran
// before: a block evaluated on its own, inside a block group or inside a rig problem gets the same bits.
bool single_launch_dataset(const vg_problem *p, const Dataset &d)
{
    return !p->force_prepared_frames && dataset_can_inline_chain(p, d);
}

// every evaluation of a dataset, empty ones included, starts a new epoch: the tag of its failure counter (d_failed)
void next_epoch(Dataset &d)
{
    d.epoch = (d.epoch + 1) & 0xFFFFFFull;
    if (d.epoch == 0) d.epoch = 1;
}

bool wants_jacobian(const Dataset &d, const double *jac_intr, double *const *jac_member)
{
    bool want = jac_intr != nullptr;
    for (int l = 0; l < d.L; l++) want = want || (jac_member && jac_member[l]);
    return want;
}

// 32-bit observation indices inside a launch: very large datasets are evaluated in chunks of whole images
constexpr int64_t kMaxObsPerLaunch = (int64_t)1 << 30;

int64_t max_blocks_per_launch(const Dataset &d, int64_t max_obs = kMaxObsPerLaunch)
{
    return max_obs / d.N > 0 ? max_obs / d.N : 1;
}

// blocks [b0, b0 + nb) of a dataset; the output pointers are those of block b0 (chunk-local).  The store policy and the tile
// map (nt_stores, map_window) belong to the LAUNCH, not to the dataset: whoever launches sets both
void fill_emit_args_at(const vg_problem *p, const Dataset &d, vg::EmitArgs &a, int64_t b0, int64_t nb, double *res_b0, double *ji_b0,
                       double *const *jm_b0)
{
    const Camera &cam = p->cams[d.camera];
    a.frames = d.d_frames + (size_t)b0 * d.frame_stride;
    a.board = d.d_board;
    a.obs = d.d_obs + (size_t)b0 * 2 * d.N;
    a.intr = p->d_params + cam.offset;
    a.res = res_b0;
    a.jac_intr = ji_b0;
    for (int l = 0; l < vg::kMaxChain; l++) a.jac_member[l] = (l < d.L && jm_b0) ? jm_b0[l] : nullptr;
    a.failed = d.d_failed;
    a.epoch = d.epoch;
    a.n_obs = (unsigned int)(nb * d.N);
    a.N = (unsigned int)d.N;
    a.L = d.L;
    a.frame_stride_d = d.frame_stride;
    a.chain_params = d.L ? p->d_params + d.chain.base[0] : nullptr;
    a.chain_stride = d.L ? d.chain.stride[0] : 0;
    a.seq_index = d.seq_identity ? nullptr : d.d_seq + b0;
    a.first_block = b0;
#ifdef VG_EMIT_STAMPS
    a.stamps = reinterpret_cast<unsigned long long *>(vgi::debug_hook(vgi::kHookEmitStamps));
    a.stamps_waves = (unsigned long long)vgi::debug_hook(vgi::kHookEmitStampsWaves);
#endif
}

// the same with whole-dataset arrays: block b0's rows lie b0 blocks into each of them
void fill_emit_args(const vg_problem *p, const Dataset &d, vg::EmitArgs &a, int64_t b0, int64_t nb, double *residuals,
                    double *jac_intr, double *const *jac_member)
{
    const int K = p->cams[d.camera].K;
    double *jm[vg::kMaxChain] = {nullptr};
    for (int l = 0; l < d.L; l++)
        if (jac_member && jac_member[l]) jm[l] = jac_member[l] + (size_t)b0 * 2 * d.N * 6;
    fill_emit_args_at(p, d, a, b0, nb, residuals + (size_t)b0 * 2 * d.N, jac_intr ? jac_intr + (size_t)b0 * 2 * d.N * K : nullptr, jm);
}

// the store policy is a template argument of the emit kernels (one straight-line store sequence per tile): a.nt_stores picks the
// instantiation
template <int MODEL, bool WANT_JAC, bool FRAMES_LDS, bool INLINE_CHAIN>
void launch_emit_policy(hipStream_t stream, const vg::EmitArgs &a, unsigned int grid, size_t lds)
{
    switch (a.nt_stores) {
    case vg::kStoreNonTemporal:
        hipLaunchKernelGGL((vg::vg_emit_kernel<MODEL, WANT_JAC, FRAMES_LDS, INLINE_CHAIN, vg::kStoreNonTemporal>), dim3(grid), dim3(vg::kEmitThreads), lds, stream, a);
        break;
    case vg::kStoreWriteThrough:
        hipLaunchKernelGGL((vg::vg_emit_kernel<MODEL, WANT_JAC, FRAMES_LDS, INLINE_CHAIN, vg::kStoreWriteThrough>), dim3(grid), dim3(vg::kEmitThreads), lds, stream, a);
        break;
    default:
        hipLaunchKernelGGL((vg::vg_emit_kernel<MODEL, WANT_JAC, FRAMES_LDS, INLINE_CHAIN, vg::kStorePlain>), dim3(grid), dim3(vg::kEmitThreads), lds, stream, a);
        break;
    }
}

template <int MODEL>
int launch_emit(hipStream_t stream, const vg::EmitArgs &a, bool want_jac, bool inline_chain)
{
    const bool frames_lds = emit_frames_in_lds((int)a.N, a.frame_stride_d);
    const size_t lds = emit_lds_bytes<MODEL>(frames_lds, (int)a.N, a.frame_stride_d);
    const unsigned int grid = (a.n_obs + vg::kEmitThreads - 1) / vg::kEmitThreads;
    if (inline_chain) {  // the caller checked: one DIRECT member, frames fit the LDS
        if (want_jac) launch_emit_policy<MODEL, true, true, true>(stream, a, grid, lds);
        else launch_emit_policy<MODEL, false, true, true>(stream, a, grid, lds);
    } else if (want_jac) {
        if (frames_lds) launch_emit_policy<MODEL, true, true, false>(stream, a, grid, lds);
        else launch_emit_policy<MODEL, true, false, false>(stream, a, grid, lds);
    } else {
        if (frames_lds) launch_emit_policy<MODEL, false, true, false>(stream, a, grid, lds);
        else launch_emit_policy<MODEL, false, false, false>(stream, a, grid, lds);
    }
    VG_HIP(hipGetLastError());
    return VG_OK;
}

#ifndef VG_TU_EMIT_MODELS   // vg_emit_models_tu.hip takes the launch templates above and nothing below
// one emit launch of one dataset (or of a chunk of it) with the camera model as a value; a.nt_stores and a.map_window are set.
// The reference's three models are instantiated here; Kannala-Brandt and double sphere in a translation unit of their own
// (vg_emit_models_tu.hip): the two compile side by side and this unit's code object holds what it held before.
int launch_emit(hipStream_t stream, int model, const vg::EmitArgs &a, bool want_jac, bool inline_chain)
{
    int rc = VG_OK;
    const bool here = vg::dispatch_model(model, vg::ReferenceModels{}, [&](auto m) { rc = launch_emit<decltype(m)::value>(stream, a, want_jac, inline_chain); });
    return here ? rc : vgi::launch_emit_added_model(stream, model, a, want_jac, inline_chain);   // which refuses a model of neither list
}

// The datasets `ids` of the problem in merged launches (vg_emit_multi_kernel) of up to kEmitMultiMax datasets each, in the order
// given.  The caller checked every one of them: Jacobians wanted, frames fit the LDS, one launch holds its observations; and it
// has the frames prepared that the datasets which do not walk their chain in the kernel read.
int launch_emit_merged(vg_problem *p, const vg_dataset_outputs *outs, const std::vector<int> &ids)
{
    for (size_t g0 = 0; g0 < ids.size(); g0 += vg::kEmitMultiMax) {
        vg::EmitMultiArgs m;
        m.n = (int)(ids.size() - g0 < (size_t)vg::kEmitMultiMax ? ids.size() - g0 : (size_t)vg::kEmitMultiMax);
        unsigned int tiles = 0;
        size_t lds = 0;
        int64_t launch_bytes = 0;
        for (int k = 0; k < m.n; k++) {
            Dataset &d = p->dss[ids[g0 + k]];
            const vg_dataset_outputs &o = outs[ids[g0 + k]];
            next_epoch(d);
            fill_emit_args(p, d, m.ds[k], 0, d.n_blocks, o.residuals, o.jac_intr, o.jac_member);
            m.model[k] = p->cams[d.camera].model;
            m.inline_chain[k] = single_launch_dataset(p, d) ? 1 : 0;
            m.first_tile[k] = tiles;
            tiles += (m.ds[k].n_obs + vg::kEmitThreads - 1) / vg::kEmitThreads;
            const size_t need = emit_lds_bytes<vg::kEUCM>(true, d.N, d.frame_stride);  // same tile size for every model
            lds = need > lds ? need : lds;
            launch_bytes += emit_output_bytes(m.ds[k], p->cams[d.camera].K);
        }
        for (int k = m.n; k <= vg::kEmitMultiMax; k++) m.first_tile[k] = tiles;
        // one store policy and one tile map for the whole launch: its datasets share the Infinity Cache
        const int policy = emit_store_policy(launch_bytes);
        const unsigned int window = emit_map_window(launch_bytes);
        for (int k = 0; k < m.n; k++) {
            m.ds[k].nt_stores = policy;
            m.ds[k].map_window = window;
        }
        // XCD x takes the x-th eighth of EVERY dataset, dataset after dataset -- equal bytes and equal arithmetic per die
        // whatever the mix of models, and the datasets that need no prepared frames come first on every die (same box:
        // stereo 21.1 -> 19.6 us, rig 116 (one contiguous piece of equal tile counts per die) / 108.5 (equal bytes) / 109.4 us)
        unsigned int longest = 0;
        for (int k = 0; k < m.n; k++) longest += (m.first_tile[k + 1] - m.first_tile[k] + 7) / 8;
        switch (policy) {
        case vg::kStoreNonTemporal:
            hipLaunchKernelGGL(vg::vg_emit_multi_kernel<vg::kStoreNonTemporal>, dim3(8 * longest), dim3(vg::kEmitThreads), lds, p->stream, m);
            break;
        case vg::kStoreWriteThrough:
            hipLaunchKernelGGL(vg::vg_emit_multi_kernel<vg::kStoreWriteThrough>, dim3(8 * longest), dim3(vg::kEmitThreads), lds, p->stream, m);
            break;
        default:
            hipLaunchKernelGGL(vg::vg_emit_multi_kernel<vg::kStorePlain>, dim3(8 * longest), dim3(vg::kEmitThreads), lds, p->stream, m);
            break;
        }
        VG_HIP(hipGetLastError());
    }
    return VG_OK;
}
#endif  // VG_TU_EMIT_MODELS

}  // namespace
