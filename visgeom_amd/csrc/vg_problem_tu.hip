// vg_problem_tu.hip -- translation unit of libvisgeom_amd.so: what every other unit stands on (the thread's error string,
// check_device, the debug-hook table, the version and model queries) and problem assembly: vg_problem_create / add_* /
// finalize, parameter get / set and the getters that need no launch logic.  Host code only: it owns no kernel.
// Built with hipcc for gfx950 only.  No CPU fallback: every compute entry needs a HIP device.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "vg_internal.hpp"
#include "vg_transf_host.hpp"

namespace {

thread_local std::string g_err;

}  // namespace

int vgi::fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}

using vgi::Camera;
using vgi::Dataset;
using vgi::Transform;
using vgi::fail;
using vgi::valid_dataset;

int vgi::check_device(int device, const char *what)
{
    int n = 0;
    const hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return fail(VG_ERR_NO_DEVICE, std::string("no HIP device available (") + (e == hipSuccess ? "device count 0" : hipGetErrorString(e)) +
                                          "): " + what + " has no CPU fallback");
    }
    if (device < 0 || device >= n) return fail(VG_ERR_INVALID_ARGUMENT, "device index out of range");
    return VG_OK;
}

#ifdef VG_DEBUG_HOOKS
namespace {
long long g_debug_hooks[vgi::kHookCount] = {0};
const char *const kDebugHookNames[vgi::kHookCount] = {"inline_chain_max_bytes", "gram_no_merge", "max_obs_per_launch", "solver_timing",
                                                      "solver_host_loop", "solver_device_loop", "solver_no_fold_frames", "solver_fold_max_groups",
                                                      "emit_nt_min_bytes", "host_chunk_bytes", "gram_persistent", "emit_map_window",
                                                      "emit_write_through", "emit_stamps", "emit_stamps_waves"};
}  // namespace
long long vgi::debug_hook(vgi::DebugHook h) { return g_debug_hooks[h]; }
#endif

extern "C" {

#ifdef VG_DEBUG_HOOKS   // the production library does not export the entry at all (tests/test_capi_cpu.py)
int vg_debug_set(const char *name, long long value)
{
    if (!name) return fail(VG_ERR_INVALID_ARGUMENT, "name is NULL");
    for (int k = 0; k < vgi::kHookCount; k++)
        if (std::strcmp(name, kDebugHookNames[k]) == 0) {
            g_debug_hooks[k] = value;
            return VG_OK;
        }
    return fail(VG_ERR_INVALID_ARGUMENT, std::string("unknown debug hook: ") + name);
}
#endif

int vg_abi_version(void) { return VG_ABI_VERSION; }

const char *vg_last_error(void) { return g_err.c_str(); }

int vg_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int vg_num_intrinsics(int model) { return vg::num_intrinsics(model); }

int vg_intrinsic_bounds(int model, int idx, double *lower, double *upper)
{
    const int K = vg::num_intrinsics(model);
    if (K < 0 || idx < 0 || idx >= K || !lower || !upper) return fail(VG_ERR_INVALID_ARGUMENT, "bad model / index");
    double lo = 1., hi = 1e5;  // "the rest": focal lengths and centre
    if (model == VG_MODEL_EUCM) {          // eucm.h:228-246
        if (idx == 0) { lo = 0.; hi = 1.; }
        else if (idx == 1) { lo = 0.1; hi = 10.; }
    } else if (model == VG_MODEL_UCM) {    // ucm.h:199-215
        if (idx == 0) { lo = 0.; hi = 3.; }
    } else if (model == VG_MODEL_MEI) {    // mei.h:287-313
        if (idx == 0) { lo = 0.; hi = 3.; }
        else if (idx <= 5) { lo = -10.; hi = 10.; }
    } else if (model == VG_MODEL_KB) {     // k1..k4: Mei's distortion range
        if (idx <= 3) { lo = -10.; hi = 10.; }
    } else if (model == VG_MODEL_DS) {     // xi, alpha
        if (idx == 0) { lo = -0.9; hi = 3.; }
        else if (idx == 1) { lo = 0.; hi = 1.; }
    } else {                               // a model of the list (num_intrinsics knows it) without its ranges here
        return fail(VG_ERR_INVALID_ARGUMENT, "unknown camera model");
    }
    *lower = lo;
    *upper = hi;
    return VG_OK;
}

/* ------------------------------------------------------------------------------------------ problem */

int vg_problem_create(vg_problem **out, int device, void *hip_stream)
{
    if (!out) return fail(VG_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    int rc = vgi::check_device(device, "visgeom_amd");
    if (rc != VG_OK) return rc;
    VG_HIP(hipSetDevice(device));
    vg_problem *p = new (std::nothrow) vg_problem();
    if (!p) return fail(VG_ERR_ALLOC, "out of host memory");
    p->device = device;
    p->stream = reinterpret_cast<hipStream_t>(hip_stream);
    *out = p;
    return VG_OK;
}

void vg_problem_destroy(vg_problem *p)
{
    if (!p) return;
    (void)hipSetDevice(p->device);
    delete p;
}

int vg_problem_add_camera(vg_problem *p, int model, const double *intrinsics, int constant, int *camera_id)
{
    if (!p || !intrinsics) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (p->finalized) return fail(VG_ERR_STATE, "problem already finalized");
    const int K = vg::num_intrinsics(model);
    if (K < 0) return fail(VG_ERR_INVALID_ARGUMENT, "unknown camera model");  // :177 throws
    Camera c;
    c.model = model;
    c.K = K;
    c.constant = constant != 0;
    c.init.assign(intrinsics, intrinsics + K);
    p->cams.push_back(c);
    if (camera_id) *camera_id = (int)p->cams.size() - 1;
    return VG_OK;
}

int vg_problem_add_transform(vg_problem *p, int is_global, int constant, int count, const double *values,
                             int *transform_id)
{
    if (!p) return fail(VG_ERR_INVALID_ARGUMENT, "problem is NULL");
    if (p->finalized) return fail(VG_ERR_STATE, "problem already finalized");
    if (is_global) count = 1;
    if (count < 0) return fail(VG_ERR_INVALID_ARGUMENT, "negative transform count");
    Transform t;
    t.global = is_global != 0;
    t.constant = constant != 0;
    t.count = count;
    t.init.assign((size_t)count * 6, 0.);
    if (values) std::memcpy(t.init.data(), values, sizeof(double) * 6 * (size_t)count);
    p->tfs.push_back(t);
    if (transform_id) *transform_id = (int)p->tfs.size() - 1;
    return VG_OK;
}

}  // extern "C"

namespace {
int add_dataset_common(vg_problem *p, int camera_id, int chain_len, const int *transform_ids, const int *status,
                       int n_points, const double *board, int64_t n_images, const int32_t *image_index,
                       const double *corners, const std::shared_ptr<vgi::CornerBlock> &resident, int *dataset_id)
{
    if (!p) return fail(VG_ERR_INVALID_ARGUMENT, "problem is NULL");
    if (p->finalized) return fail(VG_ERR_STATE, "problem already finalized");
    if (camera_id < 0 || camera_id >= (int)p->cams.size()) return fail(VG_ERR_INVALID_ARGUMENT, "camera id out of range");
    if (chain_len < 0 || chain_len > VG_MAX_CHAIN)
        return fail(VG_ERR_INVALID_ARGUMENT, "chain length must be in [0, 5]");  // :566-567 throws above 5
    if (chain_len > 0 && (!transform_ids || !status)) return fail(VG_ERR_INVALID_ARGUMENT, "chain arrays are NULL");
    if (n_points <= 0 || !board) return fail(VG_ERR_INVALID_ARGUMENT, "empty board");
    if (n_images < 0) return fail(VG_ERR_INVALID_ARGUMENT, "negative image count");   // corners NULL: zero observations (see the header)
    Dataset d;
    d.camera = camera_id;
    d.L = chain_len;
    d.N = n_points;
    d.n_blocks = n_images;
    int64_t min_seq = -1;
    for (int l = 0; l < chain_len; l++) {
        const int t = transform_ids[l];
        if (t < 0 || t >= (int)p->tfs.size()) return fail(VG_ERR_INVALID_ARGUMENT, "transform id out of range");
        if (status[l] != VG_TRANSFORM_DIRECT && status[l] != VG_TRANSFORM_INVERSE)
            return fail(VG_ERR_INVALID_ARGUMENT, "status must be DIRECT or INVERSE");
        d.tids[l] = t;
        d.status[l] = status[l];
        if (!p->tfs[t].global && (min_seq < 0 || p->tfs[t].count < min_seq)) min_seq = p->tfs[t].count;
    }
    d.h_seq.resize((size_t)n_images);
    for (int64_t i = 0; i < n_images; i++) {
        const int64_t idx = image_index ? image_index[i] : i;
        if (idx < 0 || (min_seq >= 0 && idx >= min_seq))
            return fail(VG_ERR_INVALID_ARGUMENT, "image index outside the sequence transform");
        d.h_seq[(size_t)i] = (int32_t)idx;
    }
    d.h_board.assign(board, board + 3 * (size_t)n_points);
    if (resident) {
        if (resident->device != p->device || resident->N != n_points || resident->n_images < n_images)
            return fail(VG_ERR_INVALID_ARGUMENT, "the resident corner block does not fit the dataset (device, board size or image count)");
        d.resident = resident;
    } else {
        d.zero_obs = corners == nullptr;
        if (corners) d.h_obs.assign(corners, corners + (size_t)n_images * 2 * n_points);
    }
    p->dss.push_back(std::move(d));
    if (dataset_id) *dataset_id = (int)p->dss.size() - 1;
    return VG_OK;
}
}  // namespace

// a dataset whose observations are zeros (cleared on the device, nothing uploaded): its residuals are the projections
// themselves, which is how writeImageResidual (unified_calibration.cpp:1186-1292) projects the board
int vgi::problem_add_projection_dataset(vg_problem *p, int camera_id, int chain_len, const int *transform_ids, const int *status, int n_points,
                                        const double *board, int64_t n_images, const int32_t *image_index, int *dataset_id)
{
    return add_dataset_common(p, camera_id, chain_len, transform_ids, status, n_points, board, n_images, image_index, nullptr, nullptr, dataset_id);
}

int vgi::problem_add_dataset_resident(vg_problem *p, int camera_id, int chain_len, const int *transform_ids, const int *status, int n_points,
                                      const double *board, int64_t n_images, const int32_t *image_index,
                                      const std::shared_ptr<CornerBlock> &corners, int *dataset_id)
{
    if (!corners) return fail(VG_ERR_INVALID_ARGUMENT, "corner block is NULL");
    return add_dataset_common(p, camera_id, chain_len, transform_ids, status, n_points, board, n_images, image_index, nullptr, corners, dataset_id);
}

extern "C" {

int vg_problem_add_dataset(vg_problem *p, int camera_id, int chain_len, const int *transform_ids, const int *status,
                           int n_points, const double *board, int64_t n_images, const int32_t *image_index,
                           const double *corners, int *dataset_id)
{
    if (n_images > 0 && !corners) return fail(VG_ERR_INVALID_ARGUMENT, "corners is NULL");
    return add_dataset_common(p, camera_id, chain_len, transform_ids, status, n_points, board, n_images, image_index, corners, nullptr, dataset_id);
}

int vg_problem_add_transformation_prior(vg_problem *p, int transform_id, const double *stiffness)
{
    if (!p || !stiffness) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (p->finalized) return fail(VG_ERR_STATE, "problem already finalized");
    if (transform_id < 0 || transform_id >= (int)p->tfs.size()) return fail(VG_ERR_INVALID_ARGUMENT, "transform id out of range");
    const Transform &t = p->tfs[transform_id];
    // a sequence transform gets the block on its element 0: getTransformData(name) defaults to index 0 (:826)
    if (!t.global && t.count < 1) return fail(VG_ERR_INVALID_ARGUMENT, "the sequence transform is empty");
    vgi::Prior pr;
    pr.tf = transform_id;
    for (int k = 0; k < 6; k++) pr.xi[k] = t.init[k];
    const vg::RotTrig g = vg::rot_trig(pr.xi + 3, true, true);
    vg::rotation_matrix(pr.xi + 3, 1., g, pr.R);   // _R(_xiPrior.rotMat())
    double M[9];
    vg::inter_omega_rot(pr.xi + 3, g, M);          // interOmegaRot(_xiPrior.rot())
    for (int k = 0; k < 36; k++) pr.A[k] = 0.;
    for (int k = 0; k < 3; k++) pr.A[6 * k + k] = stiffness[k];
    for (int r = 0; r < 3; r++)                    // bottomRightCorner = diag(stiffness[3..5]) * M
        for (int c = 0; c < 3; c++) pr.A[6 * (3 + r) + 3 + c] = stiffness[3 + r] * M[3 * r + c];
    p->priors.push_back(pr);
    return VG_OK;
}

int vg_problem_add_odometry_prior(vg_problem *p, int transform_id, int64_t index, double err_v, double err_w, double lambda,
                                  const double *xi1, const double *xi2)
{
    if (!p || !xi1 || !xi2) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (p->finalized) return fail(VG_ERR_STATE, "problem already finalized");
    if (transform_id < 0 || transform_id >= (int)p->tfs.size()) return fail(VG_ERR_INVALID_ARGUMENT, "transform id out of range");
    const Transform &t = p->tfs[transform_id];
    if (t.global) return fail(VG_ERR_INVALID_ARGUMENT, "Odometry must be a sequence");  // :749-752
    if (index < 0 || index + 1 >= t.count) return fail(VG_ERR_INVALID_ARGUMENT, "odometry index outside the sequence");
    if (!(lambda > 0.)) return fail(VG_ERR_INVALID_ARGUMENT, "lambda must be positive");
    p->odoms.push_back(vgodo::make_block(transform_id, index, err_v, err_w, lambda, xi1, xi2));
    return VG_OK;
}

int vg_problem_add_parameter_block(vg_problem *p, int size, const double *values, int constant, int *block_id)
{
    if (!p || !values) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (p->finalized) return fail(VG_ERR_STATE, "problem already finalized");
    if (size < 1 || size > 16) return fail(VG_ERR_INVALID_ARGUMENT, "parameter block size must be in [1, 16]");
    vgi::ParamBlock b;
    b.size = size;
    b.constant = constant != 0;
    b.init.assign(values, values + size);
    p->pblocks.push_back(b);
    if (block_id) *block_id = (int)p->pblocks.size() - 1;
    return VG_OK;
}

int64_t vg_problem_parameter_block_offset(const vg_problem *p, int block_id)
{
    if (!p || !p->finalized || block_id < 0 || block_id >= (int)p->pblocks.size()) return -1;
    return p->pblocks[block_id].offset;
}

int vg_problem_add_odometry_cost(vg_problem *p, int transform_id, int64_t index, double err_v, double err_w, double lambda,
                                 int n_steps, const double *delta_q, int param_block_id)
{
    if (!p || !delta_q) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (p->finalized) return fail(VG_ERR_STATE, "problem already finalized");
    if (transform_id < 0 || transform_id >= (int)p->tfs.size()) return fail(VG_ERR_INVALID_ARGUMENT, "transform id out of range");
    const Transform &t = p->tfs[transform_id];
    if (t.global) return fail(VG_ERR_INVALID_ARGUMENT, "Odometry must be a sequence");  // :667-670
    if (index < 0 || index + 1 >= t.count) return fail(VG_ERR_INVALID_ARGUMENT, "odometry index outside the sequence");
    if (!(lambda > 0.)) return fail(VG_ERR_INVALID_ARGUMENT, "lambda must be positive");
    if (n_steps < 1) return fail(VG_ERR_INVALID_ARGUMENT, "an odometry interval needs at least one wheel increment");
    if (param_block_id < 0 || param_block_id >= (int)p->pblocks.size() || p->pblocks[param_block_id].size != 3)
        return fail(VG_ERR_INVALID_ARGUMENT, "the odometry intrinsics must be a parameter block of size 3");
    p->odoms.push_back(vgodo::make_cost_block(transform_id, index, err_v, err_w, lambda, delta_q, n_steps,
                                              p->pblocks[param_block_id].init.data(), param_block_id));
    return VG_OK;
}

int vg_odometry_cost_evaluate(double err_v, double err_w, double lambda, int n_steps, const double *delta_q, const double *intr_prior,
                              const double *xi1, const double *xi2, const double *intr, double *zeta_prior, double *residual,
                              double *J1, double *J2, double *J3)
{
    if (!delta_q || !intr_prior || !xi1 || !xi2 || !intr || !residual) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!(lambda > 0.) || n_steps < 1) return fail(VG_ERR_INVALID_ARGUMENT, "lambda must be positive, n_steps >= 1");
    const vgodo::Block b = vgodo::make_cost_block(0, 0, err_v, err_w, lambda, delta_q, n_steps, intr_prior, 0);
    if (zeta_prior) std::memcpy(zeta_prior, b.zeta, sizeof b.zeta);
    vgodo::evaluate_cost(b, xi1, xi2, intr, residual, J1, J2, J3);
    return VG_OK;
}

int vg_odometry_prior_evaluate(double err_v, double err_w, double lambda, const double *xi1_odom, const double *xi2_odom,
                               const double *xi1, const double *xi2, double *residual, double *J1, double *J2)
{
    if (!xi1_odom || !xi2_odom || !xi1 || !xi2 || !residual) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!(lambda > 0.)) return fail(VG_ERR_INVALID_ARGUMENT, "lambda must be positive");
    const vgodo::Block b = vgodo::make_block(0, 0, err_v, err_w, lambda, xi1_odom, xi2_odom);
    vgodo::evaluate(b, xi1, xi2, residual, J1, J2);
    return VG_OK;
}

int vg_problem_set_pose_constant(vg_problem *p, int transform_id, int64_t index)
{
    if (!p) return fail(VG_ERR_INVALID_ARGUMENT, "problem is NULL");
    if (p->finalized) return fail(VG_ERR_STATE, "problem already finalized");
    if (transform_id < 0 || transform_id >= (int)p->tfs.size()) return fail(VG_ERR_INVALID_ARGUMENT, "transform id out of range");
    const Transform &t = p->tfs[transform_id];
    if (t.global || index < 0 || index >= t.count) return fail(VG_ERR_INVALID_ARGUMENT, "not an element of a sequence transform");
    p->const_poses.emplace_back(transform_id, index);
    return VG_OK;
}

int vg_problem_finalize(vg_problem *p)
{
    if (!p) return fail(VG_ERR_INVALID_ARGUMENT, "problem is NULL");
    if (p->finalized) return fail(VG_ERR_STATE, "problem already finalized");
    VG_HIP(hipSetDevice(p->device));
    int64_t off = 0;
    for (auto &c : p->cams) { c.offset = off; off += c.K; }
    for (auto &t : p->tfs) { t.offset = off; off += 6 * t.count; }
    for (auto &b : p->pblocks) { b.offset = off; off += b.size; }
    p->n_params = off;
    std::vector<double> h((size_t)off, 0.);
    for (auto &c : p->cams) std::memcpy(h.data() + c.offset, c.init.data(), sizeof(double) * c.K);
    for (auto &t : p->tfs)
        if (t.count) std::memcpy(h.data() + t.offset, t.init.data(), sizeof(double) * 6 * (size_t)t.count);
    for (auto &b : p->pblocks) std::memcpy(h.data() + b.offset, b.init.data(), sizeof(double) * (size_t)b.size);
    VG_HIP(p->d_params.alloc(sizeof(double) * (size_t)(off > 0 ? off : 1)));
    if (off) VG_HIP(hipMemcpy(p->d_params, h.data(), sizeof(double) * (size_t)off, hipMemcpyHostToDevice));

    for (auto &d : p->dss) {
        d.frame_stride = vg::frame_stride(d.L);
        d.chain.L = d.L;
        for (int l = 0; l < vg::kMaxChain; l++) {
            d.chain.status[l] = 0;
            d.chain.base[l] = 0;
            d.chain.stride[l] = 0;
        }
        for (int l = 0; l < d.L; l++) {
            const Transform &t = p->tfs[d.tids[l]];
            d.chain.status[l] = d.status[l];
            d.chain.base[l] = t.offset;
            d.chain.stride[l] = t.global ? 0 : 6;
        }
        const size_t nb = (size_t)d.n_blocks;
        VG_HIP(d.d_board.alloc(sizeof(double) * 3 * (size_t)d.N));
        VG_HIP(hipMemcpy(d.d_board, d.h_board.data(), sizeof(double) * 3 * (size_t)d.N, hipMemcpyHostToDevice));
        if (!d.resident) VG_HIP(d.d_obs_own.alloc(sizeof(double) * (nb ? nb : 1) * 2 * d.N));
        d.d_obs = d.resident ? d.resident->d_obs : d.d_obs_own;
        VG_HIP(d.d_seq.alloc(sizeof(int32_t) * (nb ? nb : 1)));
        VG_HIP(d.d_frames.alloc(sizeof(double) * (nb ? nb : 1) * d.frame_stride));
        VG_HIP(d.d_failed.alloc(sizeof(unsigned long long)));
        VG_HIP(hipMemset(d.d_failed, 0, sizeof(unsigned long long)));
        if (nb) {
            if (d.resident) {}   // already in HBM (vgi::upload_corners)
            else if (d.zero_obs) VG_HIP(hipMemset(d.d_obs, 0, sizeof(double) * nb * 2 * d.N));   // a projection dataset: r = proj - 0
            else VG_HIP(hipMemcpy(d.d_obs, d.h_obs.data(), sizeof(double) * nb * 2 * d.N, hipMemcpyHostToDevice));
            VG_HIP(hipMemcpy(d.d_seq, d.h_seq.data(), sizeof(int32_t) * nb, hipMemcpyHostToDevice));
        }
        // host copies are no longer needed; everything stays resident in HBM
        std::vector<double>().swap(d.h_obs);
    }
    // descriptors of the merged chain-prep launch
    std::vector<vg::PrepDataset> prep;
    int64_t first = 0;
    for (auto &d : p->dss) {
        if (!d.n_blocks) continue;
        vg::PrepDataset pd;
        pd.chain = d.chain;
        // image b uses element b of its sequence (the common case): no index array -> one dependent load less
        bool identity = true;
        for (size_t i = 0; i < d.h_seq.size() && identity; i++) identity = d.h_seq[i] == (int32_t)i;
        d.seq_identity = identity;
        pd.seq_index = identity ? nullptr : d.d_seq;
        pd.frames = d.d_frames;
        pd.first = first;
        pd.count = d.n_blocks;
        pd.frame_stride_d = d.frame_stride;
        prep.push_back(pd);
        first += d.n_blocks;
    }
    p->prep = prep;  // up to kPrepMax datasets travel by value in the arguments of vg_chain_prep_multi_kernel
    p->prep_blocks = first;
    if (prep.size() > (size_t)vg::kPrepMax) {  // more: one launch over a descriptor table in global memory
        VG_HIP(p->d_prep.alloc(sizeof(vg::PrepDataset) * prep.size()));
        VG_HIP(hipMemcpy(p->d_prep, prep.data(), sizeof(vg::PrepDataset) * prep.size(), hipMemcpyHostToDevice));
    }
    p->finalized = true;
    return VG_OK;
}

int64_t vg_problem_num_parameters(const vg_problem *p) { return p && p->finalized ? p->n_params : -1; }

int64_t vg_problem_camera_offset(const vg_problem *p, int camera_id)
{
    if (!p || !p->finalized || camera_id < 0 || camera_id >= (int)p->cams.size()) return -1;
    return p->cams[camera_id].offset;
}

int64_t vg_problem_transform_offset(const vg_problem *p, int transform_id, int64_t index)
{
    if (!p || !p->finalized || transform_id < 0 || transform_id >= (int)p->tfs.size()) return -1;
    const Transform &t = p->tfs[transform_id];
    if (index < 0 || index >= t.count) return -1;
    return t.offset + 6 * index;
}

int vg_problem_set_parameters(vg_problem *p, const double *host_params)
{
    if (!p || !host_params) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!p->finalized) return fail(VG_ERR_STATE, "problem not finalized");
    VG_HIP(hipSetDevice(p->device));
    VG_HIP(hipMemcpyAsync(p->d_params, host_params, sizeof(double) * (size_t)p->n_params, hipMemcpyHostToDevice, p->stream));
    VG_HIP(hipStreamSynchronize(p->stream));
    p->frames_stale = true;
    return VG_OK;
}

int vg_problem_get_parameters(vg_problem *p, double *host_params)
{
    if (!p || !host_params) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!p->finalized) return fail(VG_ERR_STATE, "problem not finalized");
    VG_HIP(hipSetDevice(p->device));
    VG_HIP(hipMemcpyAsync(host_params, p->d_params, sizeof(double) * (size_t)p->n_params, hipMemcpyDeviceToHost, p->stream));
    VG_HIP(hipStreamSynchronize(p->stream));
    return VG_OK;
}

double *vg_problem_parameters_device(vg_problem *p) { return p && p->finalized ? p->d_params : nullptr; }

int vg_problem_num_datasets(const vg_problem *p) { return p ? (int)p->dss.size() : -1; }
int64_t vg_dataset_num_blocks(const vg_problem *p, int d) { return valid_dataset(p, d) == VG_OK ? p->dss[d].n_blocks : -1; }
int vg_dataset_num_points(const vg_problem *p, int d) { return valid_dataset(p, d) == VG_OK ? p->dss[d].N : -1; }
int vg_dataset_chain_len(const vg_problem *p, int d) { return valid_dataset(p, d) == VG_OK ? p->dss[d].L : -1; }
int vg_dataset_num_intrinsics(const vg_problem *p, int d)
{
    return valid_dataset(p, d) == VG_OK ? p->cams[p->dss[d].camera].K : -1;
}

}  // extern "C"
