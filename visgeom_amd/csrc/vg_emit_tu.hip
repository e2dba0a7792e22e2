// vg_emit_tu.hip -- translation unit of libvisgeom_amd.so: the residual / Jacobian evaluation (vg_problem_prepare,
// vg_dataset_evaluate, vg_problem_evaluate, vg_dataset_evaluate_to_host): the chain-prep launches and every emit launch.
// Built with hipcc for gfx950 only; compiled on its own so that an edit of the emit kernels does not rebuild the others.
#define VG_TU_EMIT  // the non-template kernels this translation unit owns (the headers guard them by owner)
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "vg_emit_launch.hpp"
#include "vg_host_route.hpp"

int vgi::ensure_frames(vg_problem *p)
{
    if (!p->frames_stale) return VG_OK;
    const int rc = vgi::prepare_at(p, p->d_params);
    if (rc == VG_OK) p->frames_stale = false;
    return rc;
}

int vgi::prepare_at(vg_problem *p, const double *d_params)
{
    // whatever point this is, the frames no longer belong to an earlier vg_problem_prepare
    p->frames_stale = d_params != p->d_params;
    if (!p->prep_blocks) return VG_OK;
    if (p->d_prep) {
        const unsigned int grid = (unsigned int)((p->prep_blocks + 63) / 64);
        hipLaunchKernelGGL(vg::vg_chain_prep_table_kernel, dim3(grid), dim3(64), 0, p->stream, d_params, (const vg::PrepDataset *)p->d_prep,
                           (int)p->prep.size(), (long long)p->prep_blocks);
        VG_HIP(hipGetLastError());
        return VG_OK;
    }
    for (size_t g0 = 0; g0 < p->prep.size(); g0 += vg::kPrepMax) {
        vg::PrepMultiArgs m;
        m.n = (int)(p->prep.size() - g0 < (size_t)vg::kPrepMax ? p->prep.size() - g0 : (size_t)vg::kPrepMax);
        unsigned int waves = 0;
        int widest = 0;
        for (int k = 0; k < m.n; k++) {
            m.ds[k] = p->prep[g0 + (size_t)k];
            m.first_wave[k] = waves;
            waves += (unsigned int)((m.ds[k].count + 63) / 64);
            widest = m.ds[k].frame_stride_d > widest ? m.ds[k].frame_stride_d : widest;
        }
        for (int k = m.n; k <= vg::kPrepMax; k++) m.first_wave[k] = waves;
        m.staged = waves >= vg::kPrepStagedMinWaves ? 1 : 0;
        hipLaunchKernelGGL(vg::vg_chain_prep_multi_kernel, dim3(waves), dim3(64), m.staged ? (size_t)64 * widest * sizeof(double) : (size_t)0, p->stream, d_params, m);
        VG_HIP(hipGetLastError());
    }
    return VG_OK;
}

extern "C" {

int vg_problem_force_prepared_frames(vg_problem *p, int on)
{
    if (!p) return fail(VG_ERR_INVALID_ARGUMENT, "problem is NULL");
    p->force_prepared_frames = on != 0;
    p->frames_stale = true;
    return VG_OK;
}

int vg_problem_prepare(vg_problem *p)
{
    if (!p) return fail(VG_ERR_INVALID_ARGUMENT, "problem is NULL");
    if (!p->finalized) return fail(VG_ERR_STATE, "problem not finalized");
    VG_HIP(hipSetDevice(p->device));
    // Lazy: the frames are rebuilt by the first consumer that reads them from HBM (ensure_frames); an evaluation of
    // a single-member DIRECT chain derives them inside the emit kernel and never needs this launch.
    p->frames_stale = true;
    return VG_OK;
}

int vg_dataset_single_launch(const vg_problem *p, int d)
{
    return valid_dataset(p, d) == VG_OK && p->finalized ? (single_launch_dataset(p, p->dss[d]) ? 1 : 0) : -1;
}

int vg_dataset_evaluate(vg_problem *p, int dataset_id, double *residuals, double *jac_intr, double *const *jac_member)
{
    int rc = valid_dataset(p, dataset_id);
    if (rc != VG_OK) return rc;
    if (!p->finalized) return fail(VG_ERR_STATE, "problem not finalized");
    Dataset &d = p->dss[dataset_id];
    next_epoch(d);
    if (!d.n_blocks) return VG_OK;  // nothing to evaluate (outputs may be zero-sized / NULL)
    if (!residuals) return fail(VG_ERR_INVALID_ARGUMENT, "residuals is NULL");
    VG_HIP(hipSetDevice(p->device));
    const Camera &cam = p->cams[d.camera];
    const bool want_jac = wants_jacobian(d, jac_intr, jac_member);
    // one DIRECT member: the emit kernel walks the (trivial) chain itself -- one launch per evaluation (only while the
    // launch's output fits the Infinity Cache, see inline_chain_max_bytes).  The route is a function of the PROBLEM
    // alone (vg_dataset_single_launch), never of what ran before: the same parameters always give the same bits.
    const bool inline_chain = single_launch_dataset(p, d);
    if (!inline_chain && (rc = vgi::ensure_frames(p)) != VG_OK) return rc;

    const long long h = vgi::debug_hook(vgi::kHookMaxObsPerLaunch);  // test hook for the chunked path
    const int64_t max_blocks = h > 0 ? max_blocks_per_launch(d, h) : max_blocks_per_launch(d);
    for (int64_t b0 = 0; b0 < d.n_blocks; b0 += max_blocks) {
        const int64_t nb = d.n_blocks - b0 < max_blocks ? d.n_blocks - b0 : max_blocks;
        vg::EmitArgs a;
        fill_emit_args(p, d, a, b0, nb, residuals, jac_intr, jac_member);
        const int64_t launch_bytes = emit_output_bytes(a, cam.K);
        a.nt_stores = emit_store_policy(launch_bytes);
        a.map_window = emit_map_window(launch_bytes);
        if ((rc = launch_emit(p->stream, cam.model, a, want_jac, inline_chain)) != VG_OK) return rc;
    }
    return VG_OK;
}

int vg_problem_evaluate(vg_problem *p, const vg_dataset_outputs *outs)
{
    if (!p || !outs) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!p->finalized) return fail(VG_ERR_STATE, "problem not finalized");
    VG_HIP(hipSetDevice(p->device));
    const int n_ds = (int)p->dss.size();
    int rc;
    // which datasets can share a launch: every Jacobian-carrying evaluation whose frames fit the LDS and whose
    // observation count fits one launch; the rest (cost-only calls, huge sets) go through vg_dataset_evaluate.  The merged launch
    // (vg_emit_multi_kernel) is built for the reference's three models: a Kannala-Brandt or double-sphere dataset goes alone
    std::vector<int> shared, alone;
    for (int i = 0; i < n_ds; i++) {
        Dataset &d = p->dss[i];
        if (!d.n_blocks) {
            next_epoch(d);
            continue;
        }
        if (!outs[i].residuals) return fail(VG_ERR_INVALID_ARGUMENT, "residuals is NULL");
        if (wants_jacobian(d, outs[i].jac_intr, outs[i].jac_member) && emit_frames_in_lds(d.N, d.frame_stride) &&
            d.n_blocks <= max_blocks_per_launch(d) && vg::model_in(p->cams[d.camera].model, vg::ReferenceModels{}))
            shared.push_back(i);
        else alone.push_back(i);
    }
    if (shared.size() < 2) {  // nothing to merge
        alone.insert(alone.end(), shared.begin(), shared.end());
        shared.clear();
    }
    // widest rows first: every die ends on its lightest tiles
    std::stable_sort(shared.begin(), shared.end(), [&](int a2, int b2) {
        const Dataset &da = p->dss[a2], &db = p->dss[b2];
        return p->cams[da.camera].K + 6 * da.L > p->cams[db.camera].K + 6 * db.L;
    });
    bool need_frames = false;
    for (int i : shared) need_frames = need_frames || !single_launch_dataset(p, p->dss[i]);
    if (need_frames && (rc = vgi::ensure_frames(p)) != VG_OK) return rc;
    if ((rc = launch_emit_merged(p, outs, shared)) != VG_OK) return rc;
    for (int i : alone)
        if ((rc = vg_dataset_evaluate(p, i, outs[i].residuals, outs[i].jac_intr, outs[i].jac_member)) != VG_OK) return rc;
    return VG_OK;
}

int vg_problem_synchronize(vg_problem *p)
{
    if (!p) return fail(VG_ERR_INVALID_ARGUMENT, "problem is NULL");
    VG_HIP(hipSetDevice(p->device));
    VG_HIP(hipStreamSynchronize(p->stream));
    return VG_OK;
}

int vg_dataset_failed_count(vg_problem *p, int dataset_id, int64_t *count)
{
    int rc = valid_dataset(p, dataset_id);
    if (rc != VG_OK) return rc;
    if (!count) return fail(VG_ERR_INVALID_ARGUMENT, "count is NULL");
    if (!p->finalized) return fail(VG_ERR_STATE, "problem not finalized");
    VG_HIP(hipSetDevice(p->device));
    unsigned long long v = 0;
    VG_HIP(hipMemcpyAsync(&v, p->dss[dataset_id].d_failed, sizeof v, hipMemcpyDeviceToHost, p->stream));
    VG_HIP(hipStreamSynchronize(p->stream));
    const Dataset &d = p->dss[dataset_id];
    *count = (v >> 40) == d.epoch ? (int64_t)(v & ((1ull << 40) - 1)) : 0;
    return VG_OK;
}

int vg_dataset_gram_width(const vg_problem *p, int d)
{
    if (valid_dataset(p, d) != VG_OK) return -1;
    return p->cams[p->dss[d].camera].K + 6 * p->dss[d].L + 1;
}

}  // extern "C"
