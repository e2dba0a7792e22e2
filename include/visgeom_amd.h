/*
 * visgeom_amd.h -- C ABI of the MI355X-native reprojection residual / Jacobian engine.
 *
 * Drop-in boundary for ONE hot path of BKhomutenko/visgeom: the calibration cost function
 *     GenericProjectionJac::Evaluate        src/calibration/calib_cost_functions.cpp:28-117
 * and the normal-equation build (J^T J, J^T r) that Ceres performs on its output
 * (not in the reference tree; call sites src/calibration/unified_calibration.cpp:53,426,1152).
 *
 * Conventions
 *   - plain C, no torch / Eigen / Ceres types; every function returns a vg_status
 *     (VG_OK == 0) unless documented otherwise; vg_last_error() gives the text.
 *   - all arithmetic is IEEE double (the reference computes in double throughout).
 *   - "device pointer" = memory of the problem's HIP device (hipMalloc'ed or a torch tensor's
 *     data_ptr()); "host pointer" = ordinary memory.  Output buffers are caller-owned.
 *   - a 6-vector transform is [tx,ty,tz, rx,ry,rz] (translation, rotation vector),
 *     include/geometry/transformation.h:46.
 *   - there is NO CPU fallback: without a usable HIP device every compute entry fails with
 *     VG_ERR_NO_DEVICE / VG_ERR_HIP.
 *
 * All file:line citations are relative to the reference tree (/root/reference).
 */
#ifndef VISGEOM_AMD_H
#define VISGEOM_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VG_ABI_VERSION 1

/* camera models: parseCameras, src/calibration/unified_calibration.cpp:134-180 */
enum vg_model {
    VG_MODEL_EUCM = 0, /* [alpha,beta,fu,fv,u0,v0]          include/projection/eucm.h:29-226 */
    VG_MODEL_UCM = 1,  /* [xi,fu,fv,u0,v0]                  include/projection/ucm.h:32-197  */
    VG_MODEL_MEI = 2,  /* [xi,k1,k2,k3,k4,k5,fu,fv,u0,v0]   include/projection/mei.h:29-285  */
    /* 3 is unassigned: every entry refuses it as an unknown model.  The two below are not in the reference (DESIGN.md section
     * 5.26); the calibration, pose refinement and rectification entries take them, the localization costs of section 6, the
     * trajectory planner and the image pipelines do not (VG_ERR_INVALID_ARGUMENT). */
    VG_MODEL_KB = 4,   /* [k1,k2,k3,k4,fu,fv,u0,v0]         Kannala-Brandt (OpenCV "fisheye", Kalibr "equidistant") */
    VG_MODEL_DS = 5    /* [xi,alpha,fu,fv,u0,v0]            double sphere (Usenko et al. 2018) */
};

/* enum TransformationStatus, include/calibration/calib_cost_functions.h:25 */
enum vg_transform_status { VG_TRANSFORM_DIRECT = 0, VG_TRANSFORM_INVERSE = 1 };

enum vg_status {
    VG_OK = 0,
    VG_ERR_INVALID_ARGUMENT = 1,
    VG_ERR_HIP = 2,       /* a HIP runtime call failed (text in vg_last_error) */
    VG_ERR_NO_DEVICE = 3, /* no HIP device: the product path has no CPU fallback */
    VG_ERR_STATE = 4,     /* call order violated (e.g. evaluate before finalize) */
    VG_ERR_ALLOC = 5,
    VG_ERR_NUMERIC = 6    /* solver: a factorisation failed */
};

#define VG_MAX_CHAIN 5       /* src/calibration/unified_calibration.cpp:566-567 (> 5 throws) */
#define VG_MAX_INTRINSICS 10 /* Mei */
#define VG_DOUBLE_BIG 1e15   /* include/std.h:71, in-band failed-projection residual */

int vg_abi_version(void);
const char *vg_last_error(void);       /* thread-local, never NULL */
int vg_device_count(void);             /* number of HIP devices, 0 when none / no driver */
int vg_num_intrinsics(int model);      /* 6 / 5 / 10, -1 for an unknown model */
/* box bounds of intrinsic idx: eucm.h:228-246, ucm.h:199-215, mei.h:287-313 */
int vg_intrinsic_bounds(int model, int idx, double *lower, double *upper);

/* =====================================================================================
 * 1. Per-block entry -- 1:1 with struct GenericProjectionJac
 *    (include/calibration/calib_cost_functions.h:27-62).  A 30-line adapter deriving from
 *    ceres::CostFunction forwards ctor / Evaluate / dtor to these three calls
 *    (INTEGRATION.md section 1).  One block = one image of one camera.
 * ===================================================================================== */
typedef struct vg_block vg_block;

/* ctor (calib_cost_functions.h:29-46): copies obs ("proj", 2N) and grid (3N), records the chain
 * statuses; parameter blocks are [K, 6 x chain_len], residual count 2N.  chain_len in [0,5]. */
int vg_block_create(vg_block **out, int device, int model, int chain_len, const int *status,
                    int n_points, const double *grid /*3N host*/, const double *obs /*2N host*/);
int vg_block_num_residuals(const vg_block *b);                  /* 2N        (:45) */
int vg_block_num_parameter_blocks(const vg_block *b);           /* 1 + L           */
int vg_block_parameter_block_size(const vg_block *b, int idx);  /* K or 6    (:38-42) */

/* Evaluate (calib_cost_functions.cpp:28-117).  Host pointers, exactly Ceres' contract:
 *   parameters[0] -> K intrinsics, parameters[1+l] -> 6-vector of chain member l;
 *   residuals[2N] = [u0,v0,u1,v1,...]; failed projection -> (1e15,1e15) and zero Jacobian rows;
 *   jacobians NULL, or 1+L pointers each NULL or row-major [2N x blocksize].
 * Returns VG_OK where the reference returns true (it always does, :116). */
int vg_block_evaluate(vg_block *b, double const *const *parameters, double *residuals,
                      double **jacobians);
void vg_block_destroy(vg_block *b);

/* ---- block groups: the same per-block entry, amortised.  Blocks created against a group share one resident problem:
 * the FIRST vg_block_evaluate at a new parameter point evaluates every block of the group in one pass (merged
 * launches, one D2H into a pinned mirror), every later call at that point compares its parameter values with the ones
 * the pass used (bitwise) and copies its rows out -- about 2 us per call at 10 000 blocks against ~45 us for a block
 * on its own and ~9 us for the reference's CPU Evaluate.  A block is never served rows computed from other parameter
 * values than the ones it passes: on a mismatch it evaluates alone.
 * The per-block interface shows a block only its own parameter pointers; where the OTHER blocks' parameters are when
 * a pass opens is learned from the first pass (every block evaluates alone once and is bound to its pointers; pointer
 * identity tells which blocks share intrinsics or a global transform) and then follows the mode:
 *   VG_GROUP_IN_PLACE      parameters are read where they were last seen (ceres::Problem::Evaluate, gradient
 *                          checkers, solvers that evaluate in place);
 *   VG_GROUP_STATE_VECTOR  the host evaluates candidate points held in state arrays of a fixed layout (ceres::Solve:
 *                          every variable parameter block of a pass is state + offset): a new pass is the previous
 *                          one displaced by the displacement of the calling block's pointers; blocks whose pointers
 *                          never move (constant parameter blocks) are read in place.  The host guarantees that the
 *                          A displaced address is only read when it lies inside memory the host has PASSED to some
 *                          block of the group before (the group keeps the address ranges it has been shown; the blocks of
 *                          one state array coalesce into one range), so a new state array costs one block-by-block pass
 *                          before it is batched, and pointer arithmetic never leaves memory the host has shown.
 * Pointers passed to vg_block_evaluate must stay readable until the block is called again OR the group is invalidated:
 * call vg_block_group_invalidate when that memory goes away -- in the drop-in, right after ceres::Solve returns (its state
 * arrays are freed) and before the report's Problem::Evaluate / Evaluate calls on user memory.  Not thread safe. */
typedef struct vg_block_group vg_block_group;
enum vg_group_mode { VG_GROUP_IN_PLACE = 0, VG_GROUP_STATE_VECTOR = 1 };
int vg_block_group_create(vg_block_group **out, int device, int mode);
/* vg_block_create with membership; blocks may be added at any time (the group re-learns its layout) */
int vg_block_create_in_group(vg_block **out, vg_block_group *g, int model, int chain_len, const int *status, int n_points,
                             const double *grid /*3N host*/, const double *obs /*2N host*/);
/* Forget where parameters live (bound pointers, shown address ranges, which pointers move): every block evaluates alone
 * once more and is bound again before the next pass.  The resident problem (which blocks form a dataset) is kept. */
int vg_block_group_invalidate(vg_block_group *g);
/* counters since creation: passes over the whole group / calls answered from a pass / calls evaluated alone */
int vg_block_group_stats(const vg_block_group *g, int64_t *n_blocks, int64_t *batched_evaluations, int64_t *served, int64_t *alone);
/* destroy the group after (or before) its blocks; surviving blocks continue on the per-block path */
void vg_block_group_destroy(vg_block_group *g);

/* =====================================================================================
 * 2. Batched problem -- what GenericCameraCalibration assembles
 *    (src/calibration/unified_calibration.cpp:91-180, 514-630), evaluated in ONE pass over
 *    all (image x corner) observations per dataset instead of one Evaluate per image.
 * ===================================================================================== */
typedef struct vg_problem vg_problem;

/* hip_stream: a hipStream_t to launch on (e.g. torch.cuda.current_stream().cuda_stream), or NULL
 * for the device's default stream.  All launches of this problem go to that stream, in order. */
int vg_problem_create(vg_problem **out, int device, void *hip_stream);
void vg_problem_destroy(vg_problem *p);

/* parseCameras (:134-180).  intrinsics: K host doubles.  constant: SetParameterBlockConstant (:614-617). */
int vg_problem_add_camera(vg_problem *p, int model, const double *intrinsics, int constant,
                          int *camera_id);
/* parseTransforms (:91-132).  is_global: one shared 6-vector; otherwise a sequence of `count`
 * 6-vectors indexed by image index (include/calibration/unified_calibration.h:161-165).
 * values: count*6 host doubles or NULL (zeros). */
int vg_problem_add_transform(vg_problem *p, int is_global, int constant, int count,
                             const double *values, int *transform_id);
/* addGridResidualBlocks (:514-630): one residual block per listed image.
 *   transform_ids/status: the chain, camera-side first (initTransformChainInfo :182-231);
 *     at most one member may be a sequence transform... the reference requires exactly one (:223-228),
 *     this ABI also accepts none (all-global chains) and chain_len 0.
 *   board: 3*n_points host doubles (initGrid :279-309 / initGridIR :234-250);
 *   image_index[n_images]: index into the sequence transform(s) for each block; images whose
 *     corner list was empty are simply not listed (:520);
 *   corners: [n_images][2*n_points] host doubles, [u0,v0,u1,v1,...] per image (NULL with n_images > 0 is an error). */
int vg_problem_add_dataset(vg_problem *p, int camera_id, int chain_len, const int *transform_ids,
                           const int *status, int n_points, const double *board, int64_t n_images,
                           const int32_t *image_index, const double *corners, int *dataset_id);
/* TransformationPrior (include/calibration/calib_cost_functions.h:79-103, .cpp:214-228; parseData :808-829): six
 * residuals A * [R e_t; R e_r], e = prior^-1 o xi, pulling a transform towards the value it has NOW (the reference
 * requires the transform to have a prior value and uses it).  stiffness: the 6 diagonal weights.  On a sequence
 * transform the block acts on element 0, as in the reference (getTransformData(name), :826).  Seen by
 * vg_problem_solve, not by the per-dataset evaluation entries. */
int vg_problem_add_transformation_prior(vg_problem *p, int transform_id, const double *stiffness);
/* OdometryPrior (include/calibration/calib_cost_functions.h:64-77, .cpp:119-212; parseData :743-807): six residuals
 * between elements `index` and `index + 1` of a SEQUENCE transform, built from the two odometry poses xi1, xi2 and
 * the relative error model (err_v, err_w, lambda).  These blocks couple consecutive poses: the solver eliminates such
 * a sequence as a block-tridiagonal system on the host (fine for the few-hundred-pose odometry sets the reference
 * targets; not available together with a multi-rank all-reduce). */
int vg_problem_add_odometry_prior(vg_problem *p, int transform_id, int64_t index, double err_v, double err_w,
                                  double lambda, const double *xi1, const double *xi2);
/* Host-only evaluation of one OdometryPrior block, exported so the block can be checked without a solve:
 * constructor arguments (err_v, err_w, lambda, odometry poses xi1_odom / xi2_odom) + the two current poses ->
 * residual[6], J1[36], J2[36] (row-major; either Jacobian may be NULL). */
int vg_odometry_prior_evaluate(double err_v, double err_w, double lambda, const double *xi1_odom, const double *xi2_odom,
                               const double *xi1, const double *xi2, double *residual, double *J1, double *J2);
/* A free-standing global parameter block (1..16 doubles) at the end of the parameter vector -- the
 * [radius_left, radius_right, track_gauge] of data type "odometry_intrinsic" (unified_calibration.cpp:680-683). */
int vg_problem_add_parameter_block(vg_problem *p, int size, const double *values, int constant, int *block_id);
int64_t vg_problem_parameter_block_offset(const vg_problem *p, int block_id);
/* OdometryCost (include/calibration/odometry_cost_function.h:33-57, src/calibration/odometry_cost_function.cpp:147-266;
 * parseData :661-742): six residuals between elements `index` and `index + 1` of a SEQUENCE transform and the three
 * odometry intrinsics of a differential drive, r = A (zeta_odo(intrinsics)^-1 o (xi1^-1 o xi2)) with zeta_odo the
 * chain of the interval's n_steps wheel increments delta_q [n_steps][2] = (left, right).  Parameter blocks (6, 6, 3),
 * as the reference ADDS the block to its problem (:732-735; the class itself declares one block).  The
 * weighting A is fixed from the block's values at the time of the call.  Like OdometryPrior these blocks are
 * evaluated on the host and make the pose system of the sequence block tridiagonal (single rank). */
int vg_problem_add_odometry_cost(vg_problem *p, int transform_id, int64_t index, double err_v, double err_w, double lambda,
                                 int n_steps, const double *delta_q, int param_block_id);
/* Host-only evaluation of one OdometryCost block: constructor arguments + the three parameter blocks ->
 * zeta_prior[6] (NULL ok), residual[6], J1[36], J2[36], J3[18] (6 x 3), row-major, any Jacobian may be NULL. */
int vg_odometry_cost_evaluate(double err_v, double err_w, double lambda, int n_steps, const double *delta_q, const double *intr_prior,
                              const double *xi1, const double *xi2, const double *intr, double *zeta_prior, double *residual,
                              double *J1, double *J2, double *J3);
/* SetParameterBlockConstant on ONE element of a sequence ("anchor": true, :803-806). */
int vg_problem_set_pose_constant(vg_problem *p, int transform_id, int64_t index);
/* freezes the layout, uploads everything, allocates per-block frames. */
int vg_problem_finalize(vg_problem *p);

/* ---- parameter vector: [camera 0 | camera 1 | ... | transform 0 (count x 6) | transform 1 ... | parameter blocks] ---- */
int64_t vg_problem_num_parameters(const vg_problem *p);
int64_t vg_problem_camera_offset(const vg_problem *p, int camera_id);
int64_t vg_problem_transform_offset(const vg_problem *p, int transform_id, int64_t index);
int vg_problem_set_parameters(vg_problem *p, const double *host_params);  /* H2D, stream-ordered + sync */
int vg_problem_get_parameters(vg_problem *p, double *host_params);        /* D2H + sync */
double *vg_problem_parameters_device(vg_problem *p); /* device pointer, valid until destroy */

/* ---- shape queries ---- */
int vg_problem_num_datasets(const vg_problem *p);
int64_t vg_dataset_num_blocks(const vg_problem *p, int dataset_id);
int vg_dataset_num_points(const vg_problem *p, int dataset_id);
int vg_dataset_chain_len(const vg_problem *p, int dataset_id);
/* 1 when an evaluation of this dataset after a parameter change is a single launch (one DIRECT chain member, output
 * of the launch within reach of the Infinity Cache), 0 when it is chain prep + emit, -1 on a bad id */
int vg_dataset_single_launch(const vg_problem *p, int dataset_id);
int vg_dataset_num_intrinsics(const vg_problem *p, int dataset_id);

/* ---- evaluation (asynchronous on the problem's stream; sync with vg_problem_synchronize) ----
 * vg_problem_prepare: declares the device parameters changed.  Every block's transform chain (the two chain walks
 *   of calib_cost_functions.cpp:32-46 and :76-92, the InterJacobian ctor jacobian.h:139-152) is composed into a
 *   per-block frame by kernel 1 the next time a kernel reads frames from memory (Gram kernels, multi-member chains);
 *   for a chain of ONE member used DIRECT (mono calibration) kernel 2 derives the frame itself and an evaluation is a
 *   single launch.  Call after every parameter change (vg_problem_set_parameters implies it).
 * vg_dataset_evaluate: kernel 2 -- one thread per (image, corner): residuals + Jacobian rows in the
 *   Ceres block layout, block after block:
 *     residuals  [n_blocks][2N]            jac_intr [n_blocks][2N][K]   (row-major)
 *     jac_member[l] [n_blocks][2N][6]      any of jac_intr / jac_member / jac_member[l] may be NULL
 *   (device pointers; jac_member itself is a HOST array of chain_len device pointers). */
int vg_problem_prepare(vg_problem *p);
/* Route selection is a function of the problem alone (see vg_dataset_single_launch): a chain of one DIRECT member is
 * walked inside the consuming kernel, from xi itself (the reference's rotvec -> quaternion -> rotvec round trip of
 * compose() is skipped: |dR| < 1e-15); everything else reads the reference-order frames of the chain-prep launch.  Results
 * are bitwise reproducible per route.  on != 0 forces the chain-prep route for every dataset (tests, A/B measurements). */
int vg_problem_force_prepared_frames(vg_problem *p, int on);
int vg_dataset_evaluate(vg_problem *p, int dataset_id, double *residuals, double *jac_intr,
                        double *const *jac_member);
/* Every dataset of the problem in ONE pass: what Ceres' evaluator does when it walks all residual blocks at a new
 * point (src/calibration/unified_calibration.cpp:53 -> calib_cost_functions.cpp:28 per block).  outs[d] holds the
 * device pointers vg_dataset_evaluate would get for dataset d (unused chain slots NULL).  Datasets are merged into
 * shared launches (up to 8 per launch, any mix of camera models and chains): a stereo pair or a rig is one emit launch
 * instead of one per camera.  Same results, bit for bit, as the per-dataset entry. */
typedef struct vg_dataset_outputs {
    double *residuals;
    double *jac_intr;
    double *jac_member[VG_MAX_CHAIN];
} vg_dataset_outputs;
int vg_problem_evaluate(vg_problem *p, const vg_dataset_outputs *outs /* [vg_problem_num_datasets] */);
int vg_problem_synchronize(vg_problem *p);
/* The same evaluation delivered to HOST memory (what a Ceres EvaluationCallback needs):
 * runs kernel 2 into library-owned device buffers, copies the Ceres-layout arrays to the given host pointers
 * (pinned memory recommended; any of the Jacobian pointers may be NULL) and synchronises.  Block b of the dataset
 * is then at  residuals + b*2N,  jac_intr + b*2N*K,  jac_member[l] + b*2N*6. */
int vg_dataset_evaluate_to_host(vg_problem *p, int dataset_id, double *residuals, double *jac_intr,
                                double *const *jac_member);

/* number of failed projections (1e15 residual pairs) seen by the last vg_dataset_evaluate of that
 * dataset; synchronises the stream.  Not in the reference. */
int vg_dataset_failed_count(vg_problem *p, int dataset_id, int64_t *count);

/* =====================================================================================
 * 3. Normal-equation build (what Ceres does with Evaluate's output; not in the reference tree:
 *    SURVEY section 0 fact 2, call sites src/calibration/unified_calibration.cpp:53,426,1152).
 *    Per residual block b:  G_b = S_b^T S_b  with  S_b = [J_0 | J_1 ... J_L | r]  (2N x W, W = K + 6L + 1).
 *    G_b holds J^T J (leading (W-1)x(W-1)), J^T r (last column) and r^T r (last entry) of the block, in
 *    the block's own column order [intrinsics, chain member 0, ..., chain member L-1, residual].
 * ===================================================================================== */
int vg_dataset_gram_width(const vg_problem *p, int dataset_id); /* W */
/* fused: evaluates residuals and Jacobian rows in registers and contracts them there, on the FP64 vector pipe (products per
 * lane, recursive-halving sum over the 32 lanes of an image; chains of two or more members through the factored form
 * J_l = [p | p hat(X)] F_l: the per-corner rows stay K + 7 wide, the W x W block is a per-image congruence); J is never
 * written to HBM.  gram: device [n_blocks][W*W], row-major, full symmetric.  Needs
 * vg_problem_prepare at the current parameters, like vg_dataset_evaluate. */
int vg_dataset_gram_fused(vg_problem *p, int dataset_id, double *gram);
/* the same per-block matrices AND their fixed-order sum over the dataset's blocks (sum[W*W] device, full symmetric)
 * in two launches: narrow row blocks (W <= 13: EUCM / UCM mono) are contracted on the FP64 vector pipe with the
 * chain walked in-kernel, each workgroup leaves the sum of its images, one final launch adds those.  Wider blocks:
 * vg_dataset_gram_fused + vg_dataset_gram_sum.  The sum equals vg_dataset_gram_sum's to rounding (different fixed
 * order) and is run-to-run reproducible. */
int vg_dataset_gram_fused_sum(vg_problem *p, int dataset_id, double *gram, double *sum);
/* vg_dataset_gram_fused for EVERY dataset of the problem (grams[d]: device [n_blocks][W*W], may be NULL for an empty
 * dataset): the datasets (chains of one to five members, boards of more than 32 points) share ONE launch -- a stereo pair
 * or a rig is several launches of a few hundred workgroups otherwise, each ending in a nearly empty round. */
int vg_problem_gram_fused(vg_problem *p, double *const *grams);
/* vg_problem_gram_fused AND the fixed-order sum of every dataset's blocks (sums[d]: device [W*W], required for every
 * dataset; an empty dataset's sum is zero): the merged launch leaves per-workgroup partial sums and ONE more launch adds
 * them for all datasets -- a normal-equation build of a stereo pair or a rig is chain prep + two launches.  Each sum is
 * bit-identical to vg_dataset_gram_fused_sum's. */
int vg_problem_gram_fused_sum(vg_problem *p, double *const *grams, double *const *sums);
/* two-pass: the same Gram matrices from rows already materialised by vg_dataset_evaluate
 * (all of residuals, jac_intr and every jac_member[l] are required). */
int vg_dataset_gram_from_rows(vg_problem *p, int dataset_id, const double *residuals, const double *jac_intr,
                              const double *const *jac_member, double *gram);
/* sum over the dataset's blocks in a fixed order (two-stage tree, no atomics): sum[W*W] device. */
int vg_dataset_gram_sum(vg_problem *p, int dataset_id, const double *gram, double *sum);

/* =====================================================================================
 * 4. Solve -- replaces ceres::Solve(options, &globalProblem, &summary) at
 *    src/calibration/unified_calibration.cpp:53 for problems made of GenericProjectionJac blocks.
 *    Levenberg-Marquardt (Ceres' trust-region policy), per-pose 6x6 blocks eliminated on the GPU
 *    (Schur complement), the small global system factored on the host.  Constant blocks stay fixed
 *    (:604-617); non-constant intrinsics are kept inside the camera's box bounds (:621-627).
 *    The result is written to the problem's parameter vector.
 * ===================================================================================== */
/* ---- multi-GPU: one process per GPU, images sharded over ranks (contiguous image ranges, both cameras of a frame on
 * the same rank), global parameters replicated.  The path has ONE exchange step -- the sum of the small normal-equation
 * blocks -- done by RCCL on DEVICE buffers, in place, on the problem's stream.  Not in the reference (single process,
 * SURVEY section 5); it serves the replacement of ceres::Solve at src/calibration/unified_calibration.cpp:53.
 * RCCL is bound at run time: nothing here is needed, or loaded, on one GPU. */
typedef struct vg_comm vg_comm;
#define VG_COMM_ID_BYTES 128
/* ncclGetUniqueId: rank 0 calls it, the host hands the bytes to every rank (MPI, torch.distributed, a file ...) */
int vg_comm_unique_id(char *id /* VG_COMM_ID_BYTES */);
/* ncclCommInitRank on `device`; collective over all n_ranks ranks */
int vg_comm_create(vg_comm **out, const char *id, int n_ranks, int rank, int device);
/* wrap an ncclComm_t the host application already owns (not destroyed by vg_comm_destroy) */
int vg_comm_adopt(vg_comm **out, void *nccl_comm, int device);
/* A communicator without RCCL behind it: this process stands for `replicas` ranks that all hold the SAME shard, so every
 * sum over ranks is `replicas` times the local value.  It lets a one-GPU box run the multi-rank control flow of the solver
 * (packed collectives, summable convergence tests, identical branches on every rank): the result must be the one-rank
 * solution with the cost multiplied by `replicas`. */
int vg_comm_create_replicated(vg_comm **out, int replicas, int device);
/* n_ranks communicators for n_ranks host THREADS of this process that drive ONE device, each with its own problem, stream
 * and shard (out: array of n_ranks handles, handle r is rank r; every handle is destroyed by its user).  No RCCL behind it:
 * a collective parks every rank's buffer in a device slot, meets at a host barrier and adds the slots in rank order.  It is a
 * test transport: it runs the solver's real multi-rank data flow -- different shards, ranks without images, the in-place
 * collectives -- on a one-GPU box, which vg_comm_create_replicated (identical shards) cannot.  A rank that fails or does
 * not arrive within 120 s breaks the group: every pending and later collective returns VG_ERR_STATE. */
int vg_comm_create_local(vg_comm **out /* [n_ranks] */, int n_ranks, int device);
int vg_comm_size(const vg_comm *c);
int vg_comm_rank(const vg_comm *c);
/* in-place sum of n doubles at device_buf over all ranks (ncclAllReduce, ncclDouble, ncclSum), enqueued on hip_stream */
int vg_comm_allreduce_sum(vg_comm *c, double *device_buf, int64_t n, void *hip_stream);
void vg_comm_destroy(vg_comm *c);

/* Host-staged alternative (tests on CPU-only boxes, non-RCCL transports): sums host_buf[0..n) over all ranks in place
 * (every rank must end with the same values).  NULL = one GPU. */
typedef int (*vg_allreduce_fn)(double *host_buf, int64_t n, void *user);

typedef struct vg_solve_options {
    int max_num_iterations;             /* 1000   unified_calibration.cpp:46 */
    double function_tolerance;          /* 1e-15  :47 */
    double gradient_tolerance;          /* 1e-15  :48 */
    double parameter_tolerance;         /* 1e-15  :49 */
    double initial_trust_region_radius; /* 1e4    Ceres default (the reference does not set it) */
    double max_trust_region_radius;     /* 1e16 */
    double min_trust_region_radius;     /* 1e-32 */
    double min_relative_decrease;       /* 1e-3 */
    double min_lm_diagonal;             /* 1e-6 */
    double max_lm_diagonal;             /* 1e32 */
    int use_bounds;                     /* 1 */
    int verbose;                        /* minimizer_progress_to_stdout, :51 */
    double soft_l1_scale;               /* 0: no loss function (the global problem, :539-564 pass NULL).  a > 0:
                                           ceres::SoftLOneLoss(a) on every grid residual block, rho(s) =
                                           2 a^2 (sqrt(1 + s / a^2) - 1) of the block's squared norm s -- what the two
                                           initial refinements use (a = 25 :1143, a = 1 :379-401) */
    vg_allreduce_fn allreduce;          /* multi-GPU through host buffers (three calls per iteration) */
    void *allreduce_user;
    vg_comm *comm;                      /* multi-GPU through RCCL: one in-place all-reduce of the device buffer
                                           [summed normal-equation blocks | step scalars] per evaluation and one of the
                                           reduced (Schur) system per linear solve, on the problem's stream.  NULL or a
                                           one-rank communicator = one GPU.  Exclusive with `allreduce`. */
} vg_solve_options;

enum vg_termination {
    VG_TERM_CONVERGENCE_FUNCTION = 0,
    VG_TERM_CONVERGENCE_GRADIENT = 1,
    VG_TERM_CONVERGENCE_PARAMETER = 2,
    VG_TERM_NO_CONVERGENCE = 3, /* max_num_iterations reached */
    VG_TERM_RADIUS_TOO_SMALL = 4,
    VG_TERM_FAILURE = 5
};

typedef struct vg_solve_summary {
    double initial_cost, final_cost; /* 1/2 sum r^2, as Ceres reports it */
    int num_iterations, num_successful_steps, termination;
    double gradient_max_norm, final_radius;
    double total_seconds, evaluate_seconds, schur_seconds, host_seconds; /* host-driven loop: time in evaluations / pose
                                    elimination / host algebra; device-resident loop: evaluate_seconds = all iterations,
                                    host_seconds = set-up (tables, buffers), schur_seconds = 0 */
    int num_global_columns;     /* G */
    int64_t num_pose_blocks;
    char message[160];
} vg_solve_summary;

void vg_solve_options_init(vg_solve_options *o); /* the defaults listed above */
/* Limits: at most 127 global columns (sum of the cameras' K + 6 per global transform: e.g. eight Mei cameras and
 * seven global transforms); any number of pose blocks below 2^28.  Beyond that VG_ERR_INVALID_ARGUMENT. */
int vg_problem_solve(vg_problem *p, const vg_solve_options *options, vg_solve_summary *summary);
/* A solve works in one device block and one pinned host block (index tables, Gram sets, Schur rows ...) which the library
 * keeps for the next solve of the process instead of returning them (allocation was a third of a 10 k-image solve).
 * This frees them; safe at any time between solves. */
void vg_release_cached_memory(void);

/* The per-image pose refinement of estimateInitialGrid (src/calibration/unified_calibration.cpp:1137-1155) for n
 * images at once: n INDEPENDENT problems -- one GenericProjectionJac block with chain {DIRECT} each, intrinsics
 * constant, ceres::SoftLOneLoss(options->soft_l1_scale), every image with its own trust region, step acceptance and
 * convergence tests (one half-wave per image runs its whole solve inside ONE kernel launch).  Host pointers:
 *   board [3 N], corners [n_images][2 N], poses [n_images][6] (in: start, out: result); optional per-image outputs
 *   iterations / final_cost (rho(|r|^2) / 2) / termination (enum vg_termination), each [n_images] or NULL.
 * options NULL = what the reference runs: Ceres' defaults (function / gradient / parameter tolerance 1e-6 / 1e-10 /
 * 1e-8) with max_num_iterations = 500 and SoftLOneLoss(25). */
int vg_refine_poses(int device, void *hip_stream, int model, const double *intrinsics, int n_points, const double *board,
                    int64_t n_images, const double *corners, double *poses, const vg_solve_options *options,
                    int32_t *iterations, double *final_cost, int32_t *termination);

/* the same call with a clock on the launch itself: *kernel_seconds = duration of vg_pose_lm_kernel alone (HIP events on the
 * launch stream), without the uploads and the read-back around it (bench.py section pose_init, tools/bench_calib.py) */
int vg_refine_poses_timed(int device, void *hip_stream, int model, const double *intrinsics, int n_points, const double *board,
                          int64_t n_images, const double *corners, double *poses, const vg_solve_options *options,
                          int32_t *iterations, double *final_cost, int32_t *termination, double *kernel_seconds);

/* The same refinement for a dataset that is RESIDENT in a finalized problem (reference flow: estimateInitialGrid
 * unified_calibration.cpp:1137-1155 refines the poses that addGridResidualBlocks :514-630 then hands to the global problem over
 * the same corners): the dataset's observations and board and the camera's CURRENT intrinsics are read where they lie in HBM;
 * only poses [n_blocks][6] (host, in: start, out: result -- camera-frame board poses, independent of the dataset's chain) and
 * the optional per-image outputs cross the bus, in one copy each way.  kernel_seconds (may be NULL): the launch alone. */
int vg_dataset_refine_poses(vg_problem *p, int dataset_id, double *poses, const vg_solve_options *options, int32_t *iterations,
                            double *final_cost, int32_t *termination, double *kernel_seconds);

/* Host-only helper of the solver, exported so the host logic can be tested without a GPU:
 * solves the symmetric positive definite n x n system A x = b (row-major A, untouched) by Cholesky.
 * Returns VG_ERR_NUMERIC when A is not positive definite. */
int vg_host_cholesky_solve(int n, const double *A, const double *b, double *x);

/* =====================================================================================
 * 5. Calibration-JSON front end -- class GenericCameraCalibration
 *    (include/calibration/unified_calibration.h:91-180): same schema (README.md:36-223), same parse order
 *    (parseTransforms :91-132, parseCameras :134-180, parseData :632-831), same pose initialisation
 *    (initTransforms :431-512, estimateInitialGrid :1066-1158, getInitTransform :311-348, initGlobalTransform
 *    :358-429), same report and image_error_<i>.txt formats.  Grid-reprojection datasets only: "ir_data", and
 *    "images" with pre-extracted corners ("corners_file", same layout as ir_data's "data_file").
 * ===================================================================================== */
typedef struct vg_calibration vg_calibration;
int vg_calibration_create(vg_calibration **out, int device);
void vg_calibration_destroy(vg_calibration *c);
/* addResiduals(infoFileName), :350-356.  Parsing runs on the host; initialising a transform ("init" != "none")
 * refines the poses on the GPU unless the dataset carries the "do_not_solve" flag. */
int vg_calibration_add_file(vg_calibration *c, const char *json_path);
/* compute(), :39-89: assemble the problem, solve (options NULL = the reference's Solver::Options, :42-52). */
int vg_calibration_compute(vg_calibration *c, const vg_solve_options *options, vg_solve_summary *summary);
/* the text compute() prints (:56-83) / the parse-time messages; return the size needed including the NUL */
int64_t vg_calibration_report(vg_calibration *c, char *buf, int64_t size);
int64_t vg_calibration_log(vg_calibration *c, char *buf, int64_t size);
int vg_calibration_num_datasets(const vg_calibration *c);
int vg_calibration_get_intrinsics(vg_calibration *c, const char *camera, double *out, int *count);
int vg_calibration_get_transform(vg_calibration *c, const char *name, int64_t index, double *out6, int64_t *count);
/* The corner list of one image of a dataset as parsed (detectedCornersVec[image], unified_calibration.h:86): *count = number
 * of doubles (2 per board point, 0 for an image without corners); out (may be NULL) receives them. */
int vg_calibration_get_corners(const vg_calibration *c, int dataset, int64_t image, double *out, int64_t *count);
int64_t vg_calibration_num_images(const vg_calibration *c, int dataset);
/* writeImageResidual(dataVec[dataset], path), :1186-1292.  sigma_out: one value per image of the dataset (NULL ok). */
int vg_calibration_write_residuals(vg_calibration *c, int dataset, const char *path, double *sigma_out,
                                   int64_t *outliers_out);
/* Where the front end's wall-clock time went, in seconds, accumulated over every vg_calibration_add_file / _compute /
 * _write_residuals call on this handle (the reference's program is `calib a.json`: parse -> estimateInitialGrid per image ->
 * ceres::Solve -> report; tools/bench_calib.py and bench.py's calib_e2e section print this table). */
typedef struct vg_calibration_timings {
    double read_files_s;        /* reading the JSON files into memory */
    double parse_json_s;        /* JSON text -> values (calibration file, corner / wheel files) */
    double geometric_init_s;    /* 4-corner pose construction (:1066-1135) + getInitTransform (:311-348), host */
    double refine_total_s;      /* the per-image refinements as seen by the host: poses up, kernel, results back (corners: corner_upload_s) */
    double refine_kernel_s;     /* ... the vg_pose_lm_kernel launches alone (HIP events) */
    double global_init_s;       /* initGlobalTransform refinements (:358-429): a batched solve per global transform */
    double assemble_s;          /* compute(): problem assembly, uploads, vg_problem_finalize */
    double solve_s;             /* compute(): vg_problem_solve */
    double readback_s;          /* compute(): parameters back into the maps */
    double residual_eval_s;     /* write_residuals: chain composition + projection of every image (GPU) */
    double residual_format_s;   /* write_residuals: statistics, formatting and writing image_error_<i>.txt */
    int64_t refine_images;      /* images refined by vg_refine_poses */
    int64_t refine_iterations;  /* sum of their LM iterations */
    int64_t refine_max_iterations; /* the slowest image's iteration count */
    int64_t json_bytes;         /* bytes of JSON text parsed */
    int64_t residual_lines;     /* lines written by write_residuals */
    double corner_upload_s;     /* gathering the detected corners into pinned staging and their upload into HBM (once per dataset) */
    int64_t corner_uploads;     /* corner blocks uploaded: one per dataset when every consumer shares it */
    int64_t corner_upload_bytes;
} vg_calibration_timings;
int vg_calibration_get_timings(const vg_calibration *c, vg_calibration_timings *out);
/* Host-only pieces of the pose initialisation, exported so that they can be checked block by block without a GPU (the
 * front end calls the same code):
 *   vg_reconstruct_point  ICamera::reconstructPoint (eucm.h:85-106, ucm.h:81-103, mei.h:90-112): uv[2] -> X[3] = (xn, yn, z);
 *                         VG_ERR_NUMERIC where the reference returns false.
 *   vg_initial_grid_pose  the 4-corner construction of estimateInitialGrid (unified_calibration.cpp:1066-1135), before its
 *                         refinement: board4 [4][3] / corners4 [4][2] at idxUL, idxUR, idxBL, idxBR -> xi6.
 *   vg_init_transform     getInitTransform (:311-348): chain_values [chain_len][6] = current value of every chain member
 *                         (camera side first; the entry at init_index is not read), xi_camera = the camera-frame board pose
 *                         -> the value of member init_index. */
int vg_reconstruct_point(int model, const double *intrinsics, const double *uv, double *X);
int vg_initial_grid_pose(int model, const double *intrinsics, const double *board4, const double *corners4, double *xi6);
int vg_init_transform(int chain_len, const int *status, int init_index, const double *chain_values, const double *xi_camera,
                      double *out6);
/* the same for a member that occurs more than once in the chain: the reference's forward loop stops at the FIRST occurrence
 * (:314-318), its backward loop at the LAST (:327-337); the members in between are read by neither */
int vg_init_transform_range(int chain_len, const int *status, int first_index, int last_index, const double *chain_values,
                            const double *xi_camera, double *out6);
/* transformFromData, include/json.h:36-67: 3 [x,y,theta] / 6 [t,rotvec] / 7 [t,qx,qy,qz,qw] / 12 row-major [R|t] */
int vg_transform_from_values(int n, const double *values, double *out6);

/* =====================================================================================
 * 6. Localization reprojection costs on the same device camera models:
 *      MonoReprojectCost    include/localization/local_cost_functions.h:159-180, src/localization/local_cost_functions.cpp:216-278
 *      SparseReprojectCost  .h:183-208, .cpp:281-391  (with Triangulator::computeRegular, src/reconstruction/triangulator.cpp:145-259)
 *      CameraJacobian       include/projection/jacobian.h:51-119
 *    The reference evaluates these one block at a time inside ceres::Solve; its RANSAC (src/localization/sparse_odom.cpp:
 *    511-606) solves 200 independent few-point problems per frame pair.  A SET keeps the constructor arguments of many
 *    blocks resident in HBM; one evaluation of the whole set is two launches (one lane per block for the transform chain,
 *    one lane per feature for triangulation / projection / the 2 x 6 rows).  The camera is constant (the reference clones
 *    it in the constructor).  xi_base_cam: the base -> camera transform shared by all blocks of the set.
 *    These entries evaluate the costs for a solver of the caller's; section 13 (sparse visual odometry) is the library's own
 *    caller: it solves the SparseReprojectCost problems of a frame pair on the device, prior included.
 * ===================================================================================== */
typedef struct vg_reproject_set vg_reproject_set;
/* SparseReprojectCost ctor (.h:185-195) for n_blocks blocks; block b owns points [offsets[b], offsets[b + 1]) of the
 * flat arrays (all HOST pointers): x1 / x2 [total][3] = _xVec1 / _xVec2 (direction vectors in camera frames 1 / 2),
 * p2 [total][2] = _pVec2, size [total] = _sizeVec.  Parameter block [6] (xiOdom), 2 n residuals per block. */
int vg_sparse_reproject_create(vg_reproject_set **out, int device, void *hip_stream, int model, const double *intrinsics,
                               const double *xi_base_cam, int64_t n_blocks, const int64_t *offsets, const double *x1,
                               const double *x2, const double *p2, const double *size);
/* MonoReprojectCost ctor (.h:161-168): five points per block, x1 [n_blocks][5][3], p2 [n_blocks][5][2] (HOST).
 * Parameter blocks [6 (xiOdom), 5 (lengths)], 10 residuals per block. */
int vg_mono_reproject_create(vg_reproject_set **out, int device, void *hip_stream, int model, const double *intrinsics,
                             const double *xi_base_cam, int64_t n_blocks, const double *x1, const double *p2);
int64_t vg_reproject_num_blocks(const vg_reproject_set *s);
int64_t vg_reproject_num_points(const vg_reproject_set *s);
int64_t vg_reproject_block_offset(const vg_reproject_set *s, int64_t block); /* first point of a block; block == n_blocks: total */
/* Evaluate of EVERY block of the set (DEVICE pointers, asynchronous on the set's stream): xi_odom [n_blocks][6];
 * residuals [total][2] (failed projection: the 1e15 pair); jacobian [total][2][6] row-major or NULL: rows 2i / 2i + 1 of
 * block b's [2 n x 6] Jacobian are at point offsets[b] + i.  Reference behaviour kept as written: only the u-row of a point
 * is divided by its size (.cpp:383-389), and the depth part of the Jacobian is exact only for an identity base -> camera
 * rotation (.cpp:355: tBaseCam1 conjugates the odometry rotation once too often). */
int vg_sparse_reproject_evaluate(vg_reproject_set *s, const double *xi_odom, double *residuals, double *jacobian);
/* the same for a MonoReprojectCost set: xi_odom [n_blocks][6], lengths [n_blocks][5]; residuals [n_blocks][10];
 * jac_odom [n_blocks][10][6], jac_lengths [n_blocks][10][5] (row-major, either may be NULL). */
int vg_mono_reproject_evaluate(vg_reproject_set *s, const double *xi_odom, const double *lengths, double *residuals,
                               double *jac_odom, double *jac_lengths);
/* Evaluate of ONE block with ceres::CostFunction::Evaluate's contract (HOST pointers, synchronous): parameters[0] = xiOdom,
 * parameters[1] = the five lengths (mono only); jacobians NULL or an array of 1 (sparse) / 2 (mono) pointers, each NULL or
 * row-major [2 n x block size].  Returns VG_OK where the reference returns true (always). */
int vg_sparse_reproject_block_evaluate(vg_reproject_set *s, int64_t block, double const *const *parameters, double *residuals,
                                       double **jacobians);
int vg_mono_reproject_block_evaluate(vg_reproject_set *s, int64_t block, double const *const *parameters, double *residuals,
                                     double **jacobians);
int vg_reproject_synchronize(vg_reproject_set *s);
void vg_reproject_destroy(vg_reproject_set *s);
/* CameraJacobian (jacobian.h:51-119) for n points: T12 / T23 HOST 6-vectors (T23 NULL: the one-transform constructor),
 * X2 [n][3], grad [n][2] (NULL without dfdxi) DEVICE; outputs DEVICE, either may be NULL: dpdxi [n][2][6] = (dudxi, dvdxi)
 * of CameraJacobian::dpdxi (:75-96), dfdxi [n][6] of ::dfdxi (:99-113).  A point the camera cannot project gives zero rows. */
int vg_camera_jacobian_evaluate(int device, void *hip_stream, int model, const double *intrinsics, const double *T12,
                                const double *T23, int64_t n, const double *X2, const double *grad, double *dpdxi, double *dfdxi);

/* =====================================================================================
 * 7. Fisheye rectification: the reference's `rectify` program (test/calibration/rectify.cpp) on the GPU.  Stateless entries on
 *    DEVICE pointers, asynchronous on hip_stream (no allocation, no synchronisation: a caller may capture them).  Every image
 *    and map side is in [1, 16384]; arrays are dense (pitch = width).
 * ===================================================================================== */
/* initRemap (rectify.cpp:27-58) for EUCM / UCM / Mei: pinhole5 = [width, height, u0, v0, f] (HOST), xi6 = the pinhole -> camera
 * transform [t, rotvec] (HOST).  Pixel (j, i) of the pinhole is the ray ((j - u0) / f, (i - v0) / f, 1) (pinhole.h:40-49), moved
 * by R(xi) X + t(xi) (transformation.h:167-171) and projected in FP64 in the reference's order; map_x / map_y DEVICE float
 * [height][width] receive the projection rounded to float.  A failed projection gives (-1, -1) (the reference leaves the
 * pinhole pixel itself there: DESIGN.md section 9). */
int vg_rectify_map(int device, void *hip_stream, int model, const double *intrinsics, const double *pinhole5, const double *xi6,
                   float *map_x, float *map_y);
enum vg_pixel_type { VG_PIXEL_U8 = 0, VG_PIXEL_F32 = 1 };
/* cv::remap(INTER_LINEAR, BORDER_CONSTANT) of n_images same-size images through ONE map pair, in one launch: src DEVICE
 * [n_images][src_h][src_w][channels], dst DEVICE [n_images][map_h][map_w][channels], pixel_type u8 or f32, channels 1, 3 or 4.
 * A map entry outside (-1, src_w) x (-1, src_h), or NaN, gives `fill`; inside, the float32 bilinear blend of the four taps, a tap
 * outside the image reading `fill`; u8 output is rounded half to even and saturated.  The fractional part is not quantised to
 * 1/32 pixel as OpenCV's is. */
int vg_remap(int device, void *hip_stream, int pixel_type, int channels, int64_t n_images, int src_w, int src_h, const void *src,
             int map_w, int map_h, const float *map_x, const float *map_y, double fill, void *dst);

/* =====================================================================================
 * 8. Checkerboard corner detection: the reference's CornerDetector (include/calibration/corner_detector.h,
 *    src/calibration/corner_detector.cpp) for batches of same-size 8-bit images.  The pixel and per-candidate stages run on the
 *    GPU, the graph stages on at most 16 host threads (one image per task).  Images are DEVICE u8 [n][height][width], dense;
 *    every side is in [16, 16384].  The calls are synchronous on the detector's stream.  Deviations: DESIGN.md section 9.
 * ===================================================================================== */
typedef struct vg_corner_detector vg_corner_detector;
/* A detector for a board of cols x rows inner corners (object.cols / object.rows; cols, rows >= 2, cols x rows <= 400);
 * improve = 1 adds the subpixel refinement (improveCorners).  hip_stream: a hipStream_t or NULL.  Allocates nothing on the
 * device until the first call; then it keeps the scratch of one image size (a call with another size replaces it).
 * Memory bound, whatever n_images is: the device scratch is at most max(1 GiB, the scratch of one image), about 21 bytes per
 * pixel per image of a chunk of up to 64 images; the pinned host staging is 9 bytes per pixel of the same chunk.  Larger
 * calls are worked through chunk by chunk. */
int vg_corner_detector_create(vg_corner_detector **out, int device, void *hip_stream, int cols, int rows, int improve);
void vg_corner_detector_destroy(vg_corner_detector *d);
/* detectPattern (.cpp:223-260) of every image: the sigma retries {1.4, 2, 1} run batched over the images not found yet.
 * HOST outputs: corners [n_images][cols x rows][2] FP64 (u, v) in the reference's order (row by row from the corner with the
 * smallest u + v; zeros for an image not found), found [n_images] (1 / 0), sigma [n_images] (the sigma
 * that found the board, 0 if none) or NULL. */
int vg_corner_detect(vg_corner_detector *d, int64_t n_images, int width, int height, const uint8_t *images, double *corners,
                     uint8_t *found, double *sigma);
/* Stage entry: computeResponse(0.7, sigma) (.cpp:262-330) of n_images images at sigma 1.4, 2 or 1.  DEVICE outputs
 * [n_images][height][width]: src1 / src2 (the two blurred u8 images), gradx / grady / imgrad (float, 0 on the one-pixel
 * border) and resp (float, 0 where not kept); HOST avg [n_images] (_avgVal, NaN when no response is kept). */
int vg_corner_response(vg_corner_detector *d, int64_t n_images, int width, int height, const uint8_t *images, double sigma,
                       uint8_t *src1, uint8_t *src2, float *gradx, float *grady, float *imgrad, float *resp, double *avg);
/* Stage entry: selectCandidates (.cpp:494-610) at sigma 1.4, 2 or 1.  HOST outputs: uv [n_images][max_out][2] the accepted
 * candidates in descending response (ties: smaller v width + u first), count [n_images] how many were accepted (at most
 * 10 cols rows), val_thresh [n_images] VAL_THRESH, n_maxima [n_images] the local maxima not below _avgVal. */
int vg_corner_candidates(vg_corner_detector *d, int64_t n_images, int width, int height, const uint8_t *images, double sigma,
                         int max_out, int32_t *uv, int32_t *count, double *val_thresh, int64_t *n_maxima);
/* getCircle (.cpp:1079-1108) around (0, 0), radius in [1, 64]: the first max_points offsets to du / dv, their number to
 * *n_points.  Host only (the tables the kernels use). */
int vg_corner_circle(int radius, int max_points, int32_t *du, int32_t *dv, int *n_points);
/* measurement: accumulated over the detector's detect calls: [0] GPU stages s, [1] device -> host copy s, [2] its bytes,
 * [3] graph stage wall s, [4] images through it, [5] refinement s (upload, kernel, download), [6] refined corners, [7] calls */
int vg_corner_detector_stats(const vg_corner_detector *d, double *stats8);
/* the number of images one chunk of a detect call holds for this image size */
int vg_corner_detector_chunk(const vg_corner_detector *d, int width, int height, int *chunk);

/* =====================================================================================
 * 9. Dense fisheye stereo: the reference's EnhancedSgm (src/reconstruction/eucm_sgm.cpp), semi-global matching along the
 *    epipolar curves of two unrectified EUCM images, one hypothesis per pixel or up to 8 (vg_stereo_compute_mh).  Images are
 *    DEVICE u8 [n][v_max][u_max], dense; depth maps are [n][y_max][x_max].  The calls are synchronous on the handle's stream.
 *    Deviations: DESIGN.md section 9.
 * ===================================================================================== */
typedef struct vg_stereo vg_stereo;
/* ScaleParameters + StereoParameters + SgmParameters (scale_parameters.h, eucm_stereo.h:34-60, eucm_sgm.h:41-70).  equal_margins
 * != 0 replaces x_max / y_max by (u_max - 2 u0) / scale + 1 and (v_max - 2 v0) / scale + 1.  epipole_margin is the SQUARED
 * pixel distance (the JSON key holds the distance).  verbosity is ignored; hypotheses must be 1, in the struct and in the JSON
 * (vg_stereo_compute_mh takes the hypothesis count per call; hypo_difference is read there). */
typedef struct vg_stereo_params {
    int scale, u0, v0, u_max, v_max, x_max, y_max, equal_margins;
    int num_epipolar_planes, epipole_margin;
    int disp_max, error_max, verbosity, hypotheses, hypo_difference, flaw_cost, desc_length, desc_resp_thresh;
    int n_scales, scales[8];
    int step_cost, jump_cost, image_based_cost, salient_points_only, use_uv_cache;
} vg_stereo_params;
/* the reference's defaults (scale 1, no margins, 1 x 1 image, disparity_max 48, error_max 25, epipole margin 50 px, flaw_cost 7,
 * descriptor_size 5, scales {1, 2, 3, 5}, descriptor_response_thresh 5, 2000 planes, step_cost 5, jump_cost 32, image based cost,
 * salient points only, uv cache) */
void vg_stereo_params_default(vg_stereo_params *p);
/* A handle for one calibrated EUCM pair: eucm1 / eucm2 the 6 intrinsics, xi12 the pose of camera 2 in camera 1 ([t, rotvec],
 * the reference's stereo_transformation), all HOST.  Checks every argument before touching HIP: disp_max even in [4, 256],
 * desc_length odd in [3, 31], 1 to 8 scales each in [1, 16], u_max / v_max in [1, 16384], x_max, y_max in [1, 16384],
 * num_epipolar_planes even in [2, 2^20], |t| > 1e-5, hypotheses 1; a camera neither of whose epipoles projects is refused.
 * Builds the curve tables on the host in FP64 and the per-pixel geometry on the GPU (32 bytes per depth pixel).  hip_stream
 * (a hipStream_t or NULL) is fixed for the handle's life: every later call runs on it, and the caller orders the work that
 * produces the images before the call. */
int vg_stereo_create(vg_stereo **out, int device, void *hip_stream, const double *eucm1, const double *eucm2, const double *xi12,
                     const vg_stereo_params *params);
void vg_stereo_destroy(vg_stereo *s);
/* the depth map size of the handle */
int vg_stereo_size(const vg_stereo *s, int *x_max, int *y_max);
/* EnhancedSgm::computeStereo (eucm_sgm.cpp:140-152) + DepthMap::at / sigma / cost of n_pairs pairs sharing the geometry.
 * DEVICE outputs [n][y_max][x_max], each may be NULL: depth (FP64 range along camera 1's ray, 0 = none), sigma, cost (the
 * matching error at disparity 0, as the reference reports it) and disparity (int32, -1 = none).  Device scratch: at most
 * max(2 GiB, one pair's) of 5 disp_max + 7 bytes per depth pixel per pair; larger batches are worked through in chunks. */
int vg_stereo_compute(vg_stereo *s, int64_t n_pairs, const uint8_t *img1, const uint8_t *img2, double *depth, double *sigma,
                      double *cost, int32_t *disparity);
/* the number of pairs one chunk of vg_stereo_compute holds */
int vg_stereo_chunk(const vg_stereo *s, int64_t *pairs);
/* Multi-hypothesis stereo: computeStereo with hypMax = hyp_max, EnhancedSgm::reconstructDisparityMH (eucm_sgm.cpp:628-738) in
 * place of reconstructDisparity.  The hypothesis count is an argument of the call: vg_stereo_params.hypotheses (and the JSON
 * key) must still be 1 at creation; maxHypDiff is the handle's hypo_difference.  hyp_max must be in [2, 8] and at most disp_max
 * (1 is vg_stereo_compute); n_pairs at least 1.  Per pixel, among the disparities d in [0, disp_max) whose matching error is
 * at most error_max, a local minimum of the aggregated cost (below its next valid disparity, not above its previous one)
 * reports the disparity in front of its next valid one; plane h holds the cheapest minimum dearer than plane h - 1's (or as
 * dear at another disparity) and, from h = 1 on, within hypo_difference of it; the planes after the last one found hold -1.
 * DEVICE outputs [n][hyp_max][y_max][x_max] (the reference's plane layout), each may be NULL: depth, sigma, cost FP64 as
 * vg_stereo_compute gives them per plane (cost of plane h: the matching error at index h, as the reference reports it),
 * disparity int32 (-1 = none) and final_cost int32 (the aggregated cost of the plane's minimum, INT32_MAX where disparity is
 * -1).  Arguments are checked before HIP is touched.  Device scratch: at most max(2 GiB, one pair's) of 5 disp_max + 3 +
 * 4 hyp_max bytes per depth pixel per pair; larger batches are worked through in chunks.  Deviations: DESIGN.md section 9. */
int vg_stereo_compute_mh(vg_stereo *s, int64_t n_pairs, const uint8_t *img1, const uint8_t *img2, int hyp_max, double *depth,
                         double *sigma, double *cost, int32_t *disparity, int32_t *final_cost);
/* Stage entry: the per-pixel geometry, DEVICE int32 [y_max][x_max][8]: status (1 camera 1 reconstructs the pixel, 2 its
 * point at infinity projects into camera 2), round(pinf) u, v, the curve index, chooseEpipole flags of camera 1 and 2
 * (1 inverted, 2 too close), 0, 0. */
int vg_stereo_geometry(vg_stereo *s, int32_t *geometry);
/* Stage entry: computeCurveCost of n pairs, DEVICE outputs: err u8 [n][y][x][disp_max], step u8 [n][y][x] (the descriptor
 * step, 0 where none was set), salient u8, skip u8.  The stage entries are for tests and measurement: unlike vg_stereo_compute
 * they run all n pairs in one launch per kernel, without chunking.  This one needs no scratch. */
int vg_stereo_curve_cost(vg_stereo *s, int64_t n_pairs, const uint8_t *img1, const uint8_t *img2, uint8_t *err, uint8_t *step,
                         uint8_t *salient, uint8_t *skip);
/* Stage entry: the sum of the four directional tableaux (computeDynamicProgramming), DEVICE int32 [n][y][x][disp_max], and
 * the winner, DEVICE int32 [n][y][x] (NULL allowed).  Not chunked; its device scratch is disp_max + 3 bytes per depth pixel
 * per pair (the error volume, step / salient / skip), 4 more and up to 3 of alignment when disparity is NULL. */
int vg_stereo_aggregate(vg_stereo *s, int64_t n_pairs, const uint8_t *img1, const uint8_t *img2, int32_t *total, int32_t *disparity);
/* Host only: CurveRasterizer<int, Polynomial2>(u, v, eu, ev, poly6) after setStep(step_mult), then `steps` steps (negative:
 * unsteps), one at a time, |steps| <= 1000: uv [|steps| + 1][2] receives the start and every position. */
int vg_stereo_curve_walk(const double *poly6, int u, int v, int eu, int ev, int step_mult, int steps, int32_t *uv);

/* =====================================================================================
 * 10. Motion stereo: the reference's MotionStereo (src/reconstruction/eucm_motion_stereo.cpp): a key frame's depth map is
 *     computed or refined from a further image of a moving camera.  Each salient pixel of the key frame is searched along
 *     its epipolar curve in the new image (the whole curve without a prior, the +-3 sigma segment with one), triangulated
 *     and fused into the map.  Images are DEVICE u8 [n][v_max][u_max], depth maps DEVICE FP64 [n][y_max][x_max].  The calls
 *     are synchronous on the handle's stream.  Deviations: DESIGN.md section 9, "Motion stereo".
 * ===================================================================================== */
typedef struct vg_motion_stereo vg_motion_stereo;
/* MotionStereoParameters (eucm_motion_stereo.h:37-53): StereoParameters + gradientThresh.  The SGM-only fields of `stereo`
 * (step_cost, jump_cost, image_based_cost, salient_points_only, use_uv_cache) are ignored; hypotheses must be 1. */
typedef struct vg_motion_stereo_params {
    vg_stereo_params stereo;
    int gradient_thresh;
} vg_motion_stereo_params;
/* vg_stereo_params_default + gradient_thresh 2 */
void vg_motion_stereo_params_default(vg_motion_stereo_params *p);
/* A handle for one pair of EUCM cameras (eucm1: the key frames' camera, eucm2: the camera of the further images; the
 * reference passes the same camera twice), HOST 6 intrinsics each.  The arguments are checked before HIP is touched, as
 * vg_stereo_create checks them, and gradient_thresh must be in [0, 255].  There is no transformation at creation: every
 * compute call brings its own. */
int vg_motion_stereo_create(vg_motion_stereo **out, int device, void *hip_stream, const double *eucm1, const double *eucm2,
                            const vg_motion_stereo_params *params);
void vg_motion_stereo_destroy(vg_motion_stereo *s);
int vg_motion_stereo_size(const vg_motion_stereo *s, int *x_max, int *y_max);
/* setBaseImage of n key frames (n in [1, 65535]): img1 DEVICE u8 [n][v_max][u_max] is copied into the handle and computeMask runs
 * on the GPU; image and mask stay resident until the next set_base.  Allocates only when n exceeds every earlier n. */
int vg_motion_stereo_set_base(vg_motion_stereo *s, int64_t n, const uint8_t *img1);
/* Both overloads of MotionStereo::compute for n independent items, n at most the n of set_base: item k pairs key frame k with
 * img2[k] (DEVICE) under the pose xi12[k] (HOST [n][6], [t, rotvec] of the new camera in the key frame; |t|^2 > 1e-10).
 * depth_in == NULL is the overload without a prior: the outputs start at 0 / 0 / error_max.  Otherwise depth_in, sigma_in and
 * cost_in are the prior map and the outputs start as its copy; an output may be the same array as its input.  depth,
 * sigma, cost: DEVICE outputs, none NULL.  counts (HOST int64 [n][6], may be NULL): the pixels rejected by selectPoint, by
 * computeUncertainty, as too certain (gdispMax / gstep < 2 with a prior; an empty search without one), by sampleImage, the
 * pixels that reached reconstruct, and the pixels it updated.  The curve tables of the n poses are built on the host and go
 * up through pinned staging; a second call with the same n allocates nothing. */
int vg_motion_stereo_compute(vg_motion_stereo *s, int64_t n, const double *xi12, const uint8_t *img2, const double *depth_in,
                             const double *sigma_in, const double *cost_in, double *depth, double *sigma, double *cost,
                             int64_t *counts);
/* Stage entry: the mask of the key frames, DEVICE u8 [n of set_base][v_max][u_max] (0 / 128). */
int vg_motion_stereo_mask(vg_motion_stereo *s, uint8_t *mask);
/* Stage entry: what compute decides per depth pixel, without writing a map.  Arguments as vg_motion_stereo_compute (depth_in
 * NULL: no prior).  record: DEVICE int32 [n][y_max][x_max][16]: [0] status (1 rejected by selectPoint, 2 by computeUncertainty,
 * 3 too certain, 4 rejected by sampleImage, 5 reached reconstruct and was left as it was, 6 updated), [1] gstep, [2] gu2,
 * [3] gv2, [4] [5] the rounded start point, [6] [7] the rounded end point, [8] gdispMax, [9] the inverted-sampling flag,
 * [10] the best sample index, [11] its cost, [12] the curve index of camera 2, [13..15] 0.  A field a pixel never reached is 0. */
int vg_motion_stereo_select(vg_motion_stereo *s, int64_t n, const double *xi12, const uint8_t *img2, const double *depth_in,
                            const double *sigma_in, const double *cost_in, int32_t *record);

/* =====================================================================================
 * 11. Depth map propagation and fusion: what the reference's mapping loop does to a key frame's map besides refining it
 *     (src/localization/mapping.cpp:181-220) -- DepthMap::wrapDepth, merge and filterNoise (src/reconstruction/depth_map.cpp).
 *     Maps are the (depth, sigma, cost) triples of sections 9 and 10: DEVICE FP64 [n][y_max][x_max], depth 0 = none.  Every
 *     call is synchronous on the handle's stream and checks its arguments before HIP is touched.  Constants (stereo_misc.h):
 *     MIN_DEPTH 0.25, OUT_OF_RANGE 0, DEFAULT_SIGMA_DEPTH 30, DEFAULT_COST_DEPTH 5.  Deviations: DESIGN.md section 9,
 *     "Depth map propagation".
 * ===================================================================================== */
typedef struct vg_depth_fusion vg_depth_fusion;
/* A handle for maps of one EUCM camera (eucm: HOST 6 intrinsics; the reference warps within one camera).  Of `params` only
 * the ScaleParameters fields are read (scale, u0, v0, u_max, v_max, x_max, y_max, equal_margins), under the ranges of
 * vg_stereo_create.  The handle owns its scratch (12 bytes per depth pixel and item for the warp, 16 for the filter in
 * place); a second call with the same n allocates nothing. */
int vg_depth_fusion_create(vg_depth_fusion **out, int device, void *hip_stream, const double *eucm, const vg_stereo_params *params);
void vg_depth_fusion_destroy(vg_depth_fusion *h);
int vg_depth_fusion_size(const vg_depth_fusion *h, int *x_max, int *y_max);
/* DepthMap::wrapDepth (depth_map.cpp:723-760) of n maps: item k is carried into the frame xi12[k] (HOST [n][6], [t, rotvec] of the
 * new key frame in the old, the argument of vg_motion_stereo_compute; every entry finite).  A source pixel with depth >=
 * MIN_DEPTH is reconstructed at its range, moved by the inverse transformation, projected and rounded to a target pixel; a
 * target keeps the source with the smallest new range (on an exact tie the smallest source index) and holds that range,
 * sigma_in + 0.005 range and cost_in; a target no source reaches holds 0 / 30 / 5.  The result is bit-identical from run to
 * run.  The outputs must not overlap the inputs or each other.  counts (HOST int64 [n][6], may be NULL): sources, dropped by
 * reconstructPoint, dropped by projectPoint, outside the map, lost the depth test, targets written; [0] is the sum of [1..5]. */
int vg_depth_warp(vg_depth_fusion *h, int64_t n, const double *xi12, const double *depth_in, const double *sigma_in,
                  const double *cost_in, double *depth, double *sigma, double *cost, int64_t *counts);
/* DepthMap::merge (depth_map.cpp:917-958) of map 2 into map 1, in place; cost is not touched.  Per pixel: depth2 < MIN_DEPTH
 * skipped; depth 0: map 2's pair copied; |depth - depth2| < 2 (sigma + sigma2): the two fused by filter (depth_map.cpp:32-36);
 * else the nearer of the two kept.  The four arrays must not overlap.  counts (HOST int64 [n][5], may be NULL): skipped,
 * copied, fused, replaced by map 2, kept. */
int vg_depth_merge(vg_depth_fusion *h, int64_t n, double *depth, double *sigma, const double *depth2, const double *sigma2,
                   int64_t *counts);
/* DepthMap::filterNoise (depth_map.cpp:868-914): every interior pixel with a depth is compared with its eight neighbours of
 * the INPUT map; it is cleared (0 / 0) when fewer than two neighbours hold a depth or fewer than two, and not all, of them
 * match it, and otherwise becomes the mean of itself (weight 5) and the matching neighbours.  Border pixels, and maps with
 * x_max < 3 or y_max < 3, pass through.  depth == depth_in and sigma == sigma_in are allowed (the handle then reads its own
 * copy); any other overlap of an output with an input is refused.  counts (HOST int64 [n][3], may be NULL): interior pixels
 * with a depth, cleared, smoothed. */
int vg_depth_filter_noise(vg_depth_fusion *h, int64_t n, const double *depth_in, const double *sigma_in, double *depth, double *sigma,
                          int64_t *counts);
/* Maps with hypothesis planes (vg_stereo_compute_mh): DEVICE FP64 [n][hyp_max][y_max][x_max], hyp_max in [1, 8].
 * DepthMap::regularize (depth_map.cpp:960-983) of n such maps, in place: per pixel and for h ascending, a plane whose depth is
 * below MIN_DEPTH takes depth, sigma and cost of the first plane above it that holds one, and that plane's depth becomes 0
 * (its sigma and cost stay).  The three arrays must not overlap. */
int vg_depth_regularize(vg_depth_fusion *h, int64_t n, int hyp_max, double *depth, double *sigma, double *cost);
/* DepthMap::reconstruct(pack, ALL_HYPOTHESES | SIGMA_VALUE) (depth_map.cpp:532-635) of ONE map [hyp_max][y_max][x_max]: the
 * pixels whose plane 0 holds a depth >= MIN_DEPTH, in raster order, give one entry per plane with a depth >= MIN_DEPTH, h
 * ascending.  count (HOST, required) receives the number of entries; call once with the four outputs NULL to learn it, then
 * with DEVICE arrays of that many entries (hyp_max x_max y_max always suffice), each may be NULL: indices int32 (y x_max + x),
 * hyp int32, cloud FP64 [count][3] (the pixel's normalised ray times the depth; (0, 0, 0) for a pixel the camera cannot
 * reconstruct) and sigma_out FP64 (needs sigma).  The order is the same on every run. */
int vg_depth_pack_mh(vg_depth_fusion *h, int hyp_max, const double *depth, const double *sigma, int64_t *count, int32_t *indices,
                     int32_t *hyp, double *cloud, double *sigma_out);
/* Section 11, continued: point clouds, the plane prior and the accuracy score (deviations: section 9,
 * "Point clouds and accuracy").  The flags of DepthMap::reconstruct with the reference's values (depth_map.h:39-49). */
#define VG_RECON_QUERY_POINTS 1u
#define VG_RECON_IMAGE_VALUES 2u /* refused: the reference asserts on it */
#define VG_RECON_MINMAX 4u
#define VG_RECON_ALL_HYPOTHESES 8u
#define VG_RECON_DEFAULT_VALUES 16u
#define VG_RECON_SIGMA_VALUE 32u
#define VG_RECON_QUERY_INDICES 64u
#define VG_RECON_INDEX_MAPPING 128u
/* The entries of vg_depth_reconstruct: DEVICE arrays of m entries each (m: the sum of counts), every one may be NULL.  indices
 * (y x_max + x), hyp, points [m][2] (the reference's imagePointVec: the image point the ray goes through), sigma_out (needs
 * SIGMA_VALUE), index_map (the query's position; needs INDEX_MAPPING and a query flag), item (the map an entry came from), valid
 * (1 where the camera reconstructs the ray), cloud [m][3], or [m][2][3] (near, far) under MINMAX. */
typedef struct vg_recon_outputs {
    int32_t *indices, *hyp;
    double *points, *sigma_out;
    int32_t *index_map, *item;
    uint8_t *valid;
    double *cloud;
} vg_recon_outputs;
/* DepthMap::reconstruct(pack, flags) (depth_map.cpp:532-635) of n maps, depth and sigma DEVICE FP64 [n][hyp_max][y_max][x_max],
 * hyp_max in [1, 8]; without ALL_HYPOTHESES only plane 0 is read; sigma may be NULL unless SIGMA_VALUE or MINMAX reads it.
 * Queried are, without a query flag, the pixels whose plane 0 holds a depth >= MIN_DEPTH in raster order, the ray through
 * (uConv(x), vConv(y)); under QUERY_INDICES (stronger than QUERY_POINTS, as in the reference) query_indices, DEVICE int32
 * [n_query] shared by all items: an index in [0, x_max y_max) is used with the ray through its pixel, any other is skipped;
 * under QUERY_POINTS query_points, DEVICE FP64 [n_query][2]: the pixel is x = round((u - u0) / scale), y likewise (half away
 * from zero, compared against the map in double), a point outside the map or not finite is skipped, the depth is the nearest
 * pixel's and the ray goes through the query point itself.  Per queried pixel and for h ascending a plane with depth <
 * MIN_DEPTH (NaN included) is skipped, except under DEFAULT_VALUES at h = 0, where the entry takes depth 5 and sigma 30.  The
 * cloud is the normalised ray times the depth; under MINMAX times max(depth - 3 sigma, MIN_DEPTH) and depth + 3 sigma; (0, 0,
 * 0) with valid 0 where the camera cannot reconstruct.  xi (HOST [n][6], may be NULL, every entry finite): item k's valid
 * cloud points are moved by Transformation::transform of xi[k]; failed entries stay (0, 0, 0).  Order: item after item, query
 * order, h ascending; bit-identical from run to run.  counts (HOST int64 [n], required) receives the entries per item; out ==
 * NULL or all of its members NULL only counts.  A call whose entries could reach 2^31 (n times the queries or pixels times
 * the planes read) is refused. */
int vg_depth_reconstruct(vg_depth_fusion *h, int64_t n, int hyp_max, uint32_t flags, const double *depth, const double *sigma,
                         int64_t n_query, const double *query_points, const int32_t *query_indices, const double *xi, int64_t *counts,
                         const vg_recon_outputs *out);
/* DepthMap::generatePlane (depth_map.cpp:762-803): the depth of the plane z = 0 of the frame xi_cam_plane (HOST [6], the plane's
 * frame in the camera's) inside the polygon (HOST [k][3] in the plane's frame, k in [3, 16]) as one map, DEVICE FP64 [y_max][x_max].
 * A pixel is 0 / 0 where the camera refuses it, where z . ray < 1e-3, or where ray . (p_i x p_i+1) < 0 for an edge; otherwise
 * depth |ray (t . z) / (z . ray)| and sigma 1.  cost (may be NULL) is 5 everywhere. */
int vg_depth_generate_plane(vg_depth_fusion *h, const double *xi_cam_plane, int k, const double *polygon, double *depth, double *sigma,
                            double *cost);
/* analyzeError of the reference's stereo_test (stereo_test.cpp:32-84) for n maps: depth and sigma DEVICE FP64 [n][y_max][x_max]
 * are rounded to float, truth is DEVICE float [n][v_max][u_max] (the renderer's depth buffer) read at (vConv(y), uConv(x)); a
 * grid that leaves the image is refused.  Per pixel: Ngt counts truth != 0; a pixel with truth == 0 or depth == 0, or with a NaN
 * in either, is skipped; otherwise Nmax counts it and dist adds truth; with diff = truth - depth in float it is an inlier unless
 * sigma > sigma_max (the reference's 10) or |diff| > sigma, and then N counts it, err adds diff and err2 diff^2, in double.
 * counts: HOST int64 [n][3] Ngt, Nmax, N; sums: HOST FP64 [n][3] err, err2, dist, the same bits on every run (per-workgroup
 * partials from a fixed tree, added in block order); inliers: DEVICE u8 [n][y_max][x_max], 0 / 255, may be NULL. */
int vg_depth_compare(vg_depth_fusion *h, int64_t n, const double *depth, const double *sigma, const float *truth, double sigma_max,
                     int64_t *counts, double *sums, uint8_t *inliers);
/* Host only, for the key-frame loop: Transformation::inverse (transformation.h:112-119) and inverseCompose (:90-99, a^-1 o b:
 * the pose b re-expressed in the frame a), on [t, rotvec]. */
int vg_transform_inverse(const double *xi, double *out6);
int vg_transform_inverse_compose(const double *a6, const double *b6, double *out6);

/* =====================================================================================
 * 12. Photometric localization: the reference's ScalePhotometric::computePose (src/localization/photometric.cpp:46-157) -- the
 *     pose of a new image against a key frame's depth map, by minimising the photometric error coarse to fine over a binary
 *     image pyramid (BinaryScalSpace, include/localization/scale_space.h) with PhotometricCostFunction
 *     (src/localization/local_cost_functions.cpp:35-210).  Images are DEVICE u8 [height][width], the depth map DEVICE FP64
 *     [y_max][x_max] (sections 9 to 11), poses HOST [t, rotvec] of the new frame's base in the key frame's base.  Every call is
 *     synchronous on the handle's stream and checks its arguments before HIP is touched.  Constants: GRAD_THRESH 250,
 *     DIST_MAX 50, grey limit 240, LOSS_FACTOR 3, margin 50 / scale pixels, at most 150 iterations per scale.  Deviations:
 *     DESIGN.md section 9, "Photometric localization".
 * ===================================================================================== */
typedef struct vg_photometric vg_photometric;
/* A handle for one EUCM camera (eucm: HOST 6 intrinsics), the depth map's geometry (of `params` only the ScaleParameters
 * fields are read, as by vg_depth_fusion_create), xi_base_cam (HOST [6], the camera in the base frame), the image size and
 * num_scales in [1, 8] pyramid levels (the reference uses 5); level i is (width >> i) x (height >> i), and a num_scales that
 * shrinks the coarsest level to zero size is refused. */
int vg_photometric_create(vg_photometric **out, int device, void *hip_stream, const double *eucm, const vg_stereo_params *params,
                          const double *xi_base_cam, int width, int height, int num_scales);
void vg_photometric_destroy(vg_photometric *h);
int vg_photometric_level_size(const vg_photometric *h, int scale_idx, int *width, int *height);
/* setBaseImage + setDepth + initPhotometricData of every scale: the key frame's pyramid with its Sobel / 8 gradients, and per
 * scale the data pack -- the pixels with gu^2 + gv^2 >= 250 whose depth (DepthMap::nearest at the pixel's full-size position)
 * is neither 0 nor above 50, whose grey is at most 240 and which reconstruct, in raster order: packed index v * cols + u, grey
 * value, and the point at its depth moved by xi_base_cam.  The depth map is read during the call only. */
int vg_photometric_set_base(vg_photometric *h, const uint8_t *img, const double *depth);
/* setDepth on a handle whose key frame image is set: the data pack and the mutual-information histogram of every scale again,
 * from the resident pyramid and gradients and the new depth map -- the select / scan / select / histogram launches of set_base
 * without its pyramid and Sobel launches; counts, indices, values, clouds and histograms are bit-identical to
 * set_base(the same image, depth).  VG_ERR_STATE before a key frame exists.  A call that fails leaves no key frame.  Like the
 * vg_mi_ entries it works on a vg_photometric handle under a prefix of its own. */
int vg_photo_set_depth(vg_photometric *h, const double *depth);
/* setTargetImage of n images (DEVICE u8 [n][height][width], n in [1, 65535]): n pyramids, one launch per level; they replace
 * the earlier targets. */
int vg_photometric_set_targets(vg_photometric *h, int64_t n, const uint8_t *imgs);
/* Stage entry: one pyramid level as DEVICE float [rows][cols], each output may be NULL: target = -1 the key frame, else a
 * target index.  A target's gradients are computed for this call (the reference keeps none for the target). */
int vg_photometric_level(vg_photometric *h, int64_t target, int scale_idx, float *img, float *grad_u, float *grad_v);
/* Stage entry: the data pack of a scale.  *count (HOST) receives the number of points; indices (DEVICE int32 [count]), values
 * (DEVICE FP64 [count]) and cloud (DEVICE FP64 [count][3]) may be NULL -- ask for the count first. */
int vg_photometric_pack(vg_photometric *h, int scale_idx, int64_t *count, int32_t *indices, double *values, double *cloud);
/* PhotometricCostFunction::Evaluate of n poses at one scale: xi HOST [n][6], target HOST int32 [n] (which target image a pose
 * is matched against).  With m the pack's count: residuals DEVICE [n][m], jacobians DEVICE [n][m][6]; cost (1/2 sum r^2, HOST
 * [n]), jtj (J^T J, upper triangle row-major, HOST [n][21]) and jtr (J^T r, HOST [n][6]).  Any output may be NULL.  A point
 * that does not project, or that projects into the margin of 50 / scale pixels, has a zero residual and a zero row.  The sums
 * are FP64, added in a fixed order: bit-identical from run to run. */
int vg_photometric_evaluate(vg_photometric *h, int scale_idx, int64_t n, const double *xi, const int32_t *target, double *residuals,
                            double *jacobians, double *cost, double *jtj, double *jtr);
/* computePose of n start poses (HOST [n][6]) against target[k] each: from the coarsest scale to the finest a trust-region
 * Levenberg-Marquardt of at most 150 iterations with Ceres' default tolerances, all poses advancing in the same launches.
 * xi_prior (HOST [n][6], or NULL for none) adds the reference's OdometryPrior(0.03, 0.03, 0.01, 0.01, xi_prior[k]) rows (the
 * reference passes the start pose).  xi_out HOST [n][6]; report (HOST [n][num_scales][4], may be NULL): iterations, initial
 * cost, final cost, vg_termination per scale. */
int vg_photometric_compute_pose(vg_photometric *h, int64_t n, const double *xi_start, const int32_t *target, const double *xi_prior,
                                double *xi_out, double *report);

/* ---- 12, continued: mutual-information localization, the reference's ScalePhotometric::computePoseMI
 * (src/localization/photometric.cpp:159-189, 260-385) on the MutualInformation / MutualInformationOdom cost
 * (src/localization/cost_function_mi.cpp) -- re-localization against a key frame whose image comes from another pass, with
 * another exposure and lighting, where the squared grey difference of computePose is not meant to work.  The cost is the
 * negative mutual information -sum p12 log(p12 / (p1 p2)) of a soft joint histogram of the key frame's grey values and the
 * target's samples, at the settings of computePoseMI below.  Same handle, same packs, pyramids and pose conventions as above;
 * the entries carry the prefix of their options struct, vg_mi_, and take the vg_photometric handle.
 * Deviations: DESIGN.md section 9, "Mutual-information localization". */
#define VG_MI_NUM_BINS 8                 /* numBins; the joint histogram is row-major [second image's bin][key frame's bin] */
#define VG_MI_VALUE_MAX 255.0            /* valMax; the bin width is 255 / 7 */
#define VG_MI_FUNCTION_TOLERANCE 1e-2    /* GradientProblemSolver::Options of computePoseMI */
#define VG_MI_GRADIENT_TOLERANCE 1e-3
#define VG_MI_MAX_ITERATIONS 50          /* Ceres' default */
#define VG_MI_ODOMETRY_DAMPING 0.0002    /* DAMPING of MutualInformationOdom::Evaluate */
typedef struct vg_mi_options {
    double function_tolerance; /* |f - f_previous| <= function_tolerance * |f_previous| ends a scale; 0: 1e-2 */
    double gradient_tolerance; /* max |gradient| <= gradient_tolerance ends a scale; 0: 1e-3 */
    int max_iterations;        /* per scale; 0: 50 */
} vg_mi_options;
/* MutualInformation::Evaluate of n poses at one scale: xi HOST [n][6], target HOST int32 [n].  With m the pack's count: values
 * (valVec2, DEVICE [n][m]) the target's grey at every point, hist (HOST [n][64]) the joint histogram, cost (HOST [n]) and
 * gradient (HOST [n][6]).  Any output may be NULL; without a gradient its two launches are skipped and the other outputs keep
 * their bits.  There is no margin: a point that projects is sampled wherever it lands, through the interpolator's clamping
 * grid; a point that does not project has the value 0, is still counted (in bin 0 of the second axis) and has no gradient.
 * All sums are FP64 in a fixed order: bit-identical from run to run and in every batch.  Refused with
 * VG_ERR_INVALID_ARGUMENT before HIP is touched: no key frame or no targets, a scale or target index out of range, a pose that
 * is not finite (the reference's Evaluate returns false), a scale whose pack is empty (the increment would be 1 / 0). */
int vg_mi_evaluate(vg_photometric *h, int scale_idx, int64_t n, const double *xi, const int32_t *target, double *values,
                   double *hist, double *cost, double *gradient);
/* computePoseMI of n start poses (HOST [n][6]) against target[k] each, from the coarsest scale to the finest; a scale whose
 * pack is empty is skipped (0 iterations in its report), and the call is refused when every pack is.  In place of Ceres'
 * GradientProblemSolver (BFGS) a BFGS of this library's own: inverse Hessian from the identity, first step length
 * min(1, 1 / max|g|), a strong-Wolfe line search (c1 1e-4, c2 0.9, bracketing and zoom with cubic interpolation, at most 20
 * evaluations), no update when s^T y <= 0; a scale ends on the function tolerance, the gradient tolerance, max_iterations
 * (VG_TERM_NO_CONVERGENCE) or a failed line search (VG_TERM_FAILURE).  All poses advance in the same launches, a finished
 * pose is masked; a trial pose that is not finite counts as a failed trial.  options NULL or zero fields: the reference's.
 * xi_odom (HOST [n][6], or NULL) selects MutualInformationOdom(xiOdom = xi_odom[k], xiPrior = xi_start[k], errV 0.1, errW
 * 0.01, lambdaT = lambdaR 0.01): VG_MI_ODOMETRY_DAMPING err (C / 2) err^T is added to the cost and DAMPING err J to the
 * gradient, err = xiPrior^-1 o xi, in host arithmetic.  xi_out HOST [n][6]; report (HOST [n][num_scales][4], may be NULL):
 * iterations, initial cost, final cost, vg_termination per scale. */
int vg_mi_compute_pose(vg_photometric *h, int64_t n, const double *xi_start, const int32_t *target, const double *xi_odom,
                       const vg_mi_options *options, double *xi_out, double *report);
/* Host only: the odometry term of MutualInformationOdom alone, as compute_pose_mi adds it -- *cost = DAMPING err (C / 2) err^T,
 * gradient (HOST [6], may be NULL) = DAMPING err J, for the pose xi (all HOST [6]). */
int vg_mi_odometry(const double *xi_odom, const double *xi_prior, const double *xi, double *cost, double *gradient);

/* =====================================================================================
 * 13. Sparse visual odometry: the reference's SparseOdometry::feedData (src/localization/sparse_odom.cpp:240-437) -- the camera
 *     motion between two consecutive images before any depth map exists, from Harris corners (:161-203), 9 x 9 weighted
 *     patches (:205-238), brute-force L1 matching with cross-check (:266-300), a RANSAC of small SparseReprojectCost +
 *     OdometryPrior solves (:511-606, :440-469) and two refinements (:336-387).  Images are DEVICE u8 [n][height][width],
 *     poses HOST [t, rotvec] of the base frame.  Every call is synchronous on the handle's stream and checks its arguments
 *     before HIP is touched.  All arithmetic is FP64 or integer and every floating-point sum has a fixed order: results are
 *     bit-identical from run to run and do not depend on the batch a problem is part of.  Deviations: DESIGN.md section 9,
 *     "Sparse visual odometry".
 * ===================================================================================== */
typedef struct vg_sparse_odom vg_sparse_odom;
typedef struct vg_sparse_odom_params {
    int max_features;         /* NUM_FEATURES 500; in [1, 1024] */
    double match_threshold;   /* distThresh 2500: a match with a larger L1 distance is dropped */
    int num_ransac_points;    /* numRansacPoints 2; in [2, 16] */
    int ransac_iterations;    /* maxIteration 200; in [1, 65535] */
    double inlier_threshold;  /* thresh 1.0 pixel */
    int max_lm_iterations;    /* max_num_iterations 25 of computeTransfSparse */
    double prior_err_v, prior_err_w, prior_lambda_t, prior_lambda_r; /* OdometryPrior(0.03, 0.5, 0.03, 0.05, xiOdom) */
    double outlier_gate;      /* 3.6: an inlier stays in the last solve when err^2 < outlier_gate * sigma^2 */
    double min_stereo_base;   /* MIN_STEREO_BASE: feed skips a frame whose odometry moves the camera less; 0 */
} vg_sparse_odom_params;
void vg_sparse_odom_params_default(vg_sparse_odom_params *params);
/* A handle for one EUCM camera (eucm: HOST 6 intrinsics), xi_base_cam (HOST [6], the camera in the base frame) and one image
 * size; images smaller than 15 x 15 are refused (the detector's 7-pixel border leaves no interior). */
int vg_sparse_odom_create(vg_sparse_odom **out, int device, void *hip_stream, const double *eucm, const double *xi_base_cam, int width,
                          int height, const vg_sparse_odom_params *params);
void vg_sparse_odom_destroy(vg_sparse_odom *h);
/* Stage entry: the Harris map of n images, DEVICE int64 [n][height][width].  cornerHarris(img, 7, 3, 0.05) in exact integer
 * arithmetic: Sobel 3 x 3 dx, dy (|.| <= 1020), a = sum dx^2, b = sum dx dy, c = sum dy^2 over the 7 x 7 box, R = 20 (a c -
 * b^2) - (a + c)^2 -- the reference's response times the constant 20 (4 * 7 * 255)^4, |R| < 6e16.  Pixels whose Sobel or box
 * window leaves the image use BORDER_REFLECT_101. */
int vg_sparse_odom_response(vg_sparse_odom *h, int64_t n, const uint8_t *img, int64_t *response);
/* Stage entry: harrisCorners + descriptors of n images.  A pixel with 7 <= u < width - 7, 7 <= v < height - 7 is a feature when
 * its response is strictly greater than its 8 neighbours'; the max_features largest are kept, ordered by (R descending, raster
 * index v * width + u descending) -- the order in which the reference's heap of pair<double, int> pops them.  count HOST int32
 * [n]; keypoints DEVICE int32 [n][max_features][2] as (u, v); descriptors DEVICE float [n][max_features][81]: the 9 x 9 patch,
 * each grey value times exp(-(x^2 + y^2) / 2), x = du / 2, y = dv / 2 (the weight in double, the product rounded to float).
 * Entries past count are zero. */
int vg_sparse_odom_detect(vg_sparse_odom *h, int64_t n, const uint8_t *img, int32_t *count, int32_t *keypoints, float *descriptors);
/* Stage entry: BFMatcher(NORM_L1, crossCheck) + the distance threshold for n pairs of descriptor sets (count HOST int32 [n],
 * descriptors DEVICE float [n][max_features][81]; matching reads no key points).  The L1 distance is summed in FP64 over the 81
 * values in patch order; a nearest neighbour is the lowest index on ties; (i, j) is a match when j is the nearest of set 2 to
 * i, i the nearest of set 1 to j and the distance is not above match_threshold.  match_count HOST int32 [n]; matches DEVICE
 * int32 [n][max_features][2], ordered by i; distance DEVICE FP64 [n][max_features]. */
int vg_sparse_odom_match(vg_sparse_odom *h, int64_t n, const int32_t *count1, const float *descriptors1, const int32_t *count2,
                         const float *descriptors2, int32_t *match_count, int32_t *matches, double *distance);
/* Stage entry: computeTransfSparse for n_blocks independent problems in ONE launch.  Block b owns points [offsets[b], offsets[b
 * + 1]) (offsets HOST int64 [n_blocks + 1], offsets[0] = 0; an empty block is the prior alone) of x1 / x2 (DEVICE [m][3], rays in
 * camera frames 1 / 2), p2 (DEVICE [m][2], the pixel in image 2) and size (DEVICE [m]).  Every problem is OdometryPrior(params,
 * xi_odom) + one SparseReprojectCost, started at xi_odom (HOST [6], the odometry increment), solved by a trust-region
 * Levenberg-Marquardt with Ceres' default tolerances and at most max_lm_iterations iterations, one wave per problem.  xi_out
 * HOST [n_blocks][6]; report (HOST [n_blocks][4], may be NULL): iterations, initial cost, final cost, vg_termination. */
int vg_sparse_odom_solve(vg_sparse_odom *h, int64_t n_blocks, const int64_t *offsets, const double *x1, const double *x2,
                         const double *p2, const double *size, const double *xi_odom, double *xi_out, double *report);
/* Stage entry: the scoring of ransacNPoints for n_hyp base-frame motions (xi HOST [n_hyp][6]) on m matches, one launch: camera
 * motion xi_c = xi_base_cam^-1 o xi o xi_base_cam, Triangulator(xi_c).computeRegular, the scaled ray moved by xi_c^-1,
 * projection, pixel distance to p2.  residual DEVICE FP64 [n_hyp][m] (may be NULL; +inf where the point does not project),
 * inliers HOST int32 [n_hyp]: the matches with residual < inlier_threshold. */
int vg_sparse_odom_score(vg_sparse_odom *h, int64_t n_hyp, const double *xi, int64_t m, const double *x1, const double *x2,
                         const double *p2, double *residual, int32_t *inliers);
/* The library's own draw of a RANSAC sample table for m matches (HOST int32 [ransac_iterations][num_ransac_points], distinct
 * within a row): the first num_ransac_points steps of a Fisher-Yates shuffle of an index vector that persists between rows, on
 * xorshift64* (shifts 12, 25, 27, multiplier 0x2545F4914F6CDD1D) seeded 0x9E3779B97F4A7C15 at creation.  Host only. */
int vg_sparse_odom_draw_samples(vg_sparse_odom *h, int64_t m, int32_t *samples);
#define VG_SPARSE_ODOM_REPORT 8          /* best hypothesis (-1: none), its inlier count, inliers kept by the sigma gate, final cost
                                            and vg_termination of the first, then of the second refinement, status */
#define VG_SPARSE_ODOM_OK 0
#define VG_SPARSE_ODOM_TOO_FEW_MATCHES 1 /* fewer matches than num_ransac_points: xi_incr = xi_odom */
#define VG_SPARSE_ODOM_NO_HYPOTHESIS 2   /* no hypothesis with more than num_ransac_points inliers: xi_incr = xi_odom */
/* ransacNPoints and the refinement of feedData for one frame pair: m matches as for solve, xi_odom HOST [6] the odometry
 * increment.  samples: HOST int32 [ransac_iterations][num_ransac_points] with every index in [0, m), or NULL for
 * vg_sparse_odom_draw_samples (the reference's std::shuffle of mt19937(0) is specific to its standard library).  All hypotheses
 * are solved in one launch and scored in one; a hypothesis replaces the best only with strictly more inliers, starting from
 * num_ransac_points.  Then: a solve on the best one's inliers; their reprojection under the camera motion of the ODOMETRY
 * (what the reference passes, sparse_odom.cpp:354-355); sigma^2 = sum err^2 / (n - 2); a last solve, from xi_odom again, on
 * the inliers with err^2 < outlier_gate sigma^2.  xi_incr HOST [6]; mask DEVICE u8 [m] (may be NULL): the best hypothesis'
 * inliers; report HOST [VG_SPARSE_ODOM_REPORT] (may be NULL). */
int vg_sparse_odom_ransac(vg_sparse_odom *h, int64_t m, const double *x1, const double *x2, const double *p2, const double *size,
                          const double *xi_odom, const int32_t *samples, double *xi_incr, uint8_t *mask, double *report);
#define VG_SPARSE_ODOM_FEED_REPORT 12    /* state, key points detected, matches, 0, then the ransac report */
#define VG_SPARSE_ODOM_FIRST 0           /* no previous frame (or one without key points): detected only */
#define VG_SPARSE_ODOM_SKIPPED 1         /* the skip rule: nothing changed */
#define VG_SPARSE_ODOM_ESTIMATED 2
/* feedData: img DEVICE u8 [height][width], xi_odom_new HOST [6] the wheel odometry's pose of the base frame at the image.  With
 * a previous frame whose odometry implies a camera translation below min_stereo_base the call returns at once and changes
 * nothing.  Otherwise: detect; with a previous frame match, lift the matched pixels to rays, ransac with the odometry
 * increment, integrated = integrated o xi_incr; the new frame becomes the previous one.  samples as for ransac, but an index s
 * is used as s % (matches found), since the caller cannot know that count; negative indices are refused.  xi_incr (HOST [6],
 * may be NULL) receives the current increment, report HOST [VG_SPARSE_ODOM_FEED_REPORT] (may be NULL). */
int vg_sparse_odom_feed(vg_sparse_odom *h, const uint8_t *img, const double *xi_odom_new, const int32_t *samples, double *xi_incr,
                        double *report);
/* xiIncr of the last estimated pair and xiLocal, the composition of all increments (HOST [6]; zero at creation) */
int vg_sparse_odom_increment(const vg_sparse_odom *h, double *xi6);
int vg_sparse_odom_integrated(const vg_sparse_odom *h, double *xi6);

/* =====================================================================================
 * 14. Synthetic scene renderer: the reference's RenderDevice (src/render/render.cpp) -- the source of images with exact poses
 *     and exact depth its stereo, mapping and odometry tests are fed and scored from.  The world is textured rectangles in
 *     front of a panoramic background (src/render/plane.cpp, background.cpp); a view is the EUCM image of it at a camera pose,
 *     with the hit buffers behind it: per pixel the object index, the texture coordinates and the range along the ray
 *     (getDepthBuffer, the ground truth).  fillBuffers tests every object per pixel in the order given and keeps the nearest;
 *     fillImage takes the texture-space footprint of a pixel from its neighbours on the same object and filters the texture over
 *     it with Texture::sample (texture.cpp:28-70): one bicubic sample where the footprint is below a texel, else up to 24 x 24
 *     bilinear taps weighted by the separable kernels of LookupFilter (aa_filter_lt.cpp).  All arithmetic is FP64 in the
 *     reference's order and the buffers are its narrow types (int16 index, float u, v, depth): a view is bit-identical from run
 *     to run and does not depend on the batch it is part of.  Every call is synchronous on the handle's stream and checks its
 *     arguments before HIP is touched.  Deviations: DESIGN.md section 9, "Scene renderer".
 * ===================================================================================== */
#define VG_RENDER_BACKGROUND 0
#define VG_RENDER_PLANE 1
#define VG_RENDER_MAX_PLANES 64
#define VG_RENDER_MIN_SIDE 2             /* of the image and of every texture, in pixels */
#define VG_RENDER_MAX_SIDE 16384
#define VG_RENDER_COUNTS 5               /* pixels not reconstructed, covered by nothing, background, plane; single bicubic tap */
typedef struct vg_render vg_render;
typedef struct vg_render_object {
    int kind;               /* VG_RENDER_BACKGROUND or VG_RENDER_PLANE */
    const uint8_t *texture; /* HOST [rows][cols], 8-bit grey; copied at creation */
    int cols, rows;
    double pose[6];         /* plane: [t, rotvec] of the plane in the world; its x and y axes span it, the centre is at t */
    double width, height;   /* plane: its extent in metres along x and y; the texture covers it */
} vg_render_object;
/* A world seen by one EUCM camera (eucm: HOST 6 intrinsics) in images of width x height pixels.  objects[0] must be the
 * background (its texture is the panorama: yaw across, pitch down, 2 pi each; range 150 everywhere), objects[1 ..] planes, at
 * most VG_RENDER_MAX_PLANES.  Image and texture sides are in [VG_RENDER_MIN_SIDE, VG_RENDER_MAX_SIDE]; poses are finite, plane
 * extents positive.  The handle keeps the textures on the device and owns the scratch of its calls. */
int vg_render_create(vg_render **out, int device, void *hip_stream, const double *eucm, int width, int height, int n_objects,
                     const vg_render_object *objects);
void vg_render_destroy(vg_render *h);
int vg_render_size(const vg_render *h, int *width, int *height);
/* setCamera: later views use these intrinsics; the image size stays. */
int vg_render_set_camera(vg_render *h, const double *eucm);
/* render() of n views, n in [0, 65535]: xi_cam HOST [n][6], the camera's pose in the world as [t, rotvec], every entry finite.
 * image DEVICE u8 [n][height][width].  Optional DEVICE outputs, each may be NULL: depth float [n][height][width] (the range of
 * the nearest hit; 1e6 where there is none), index int16 (-1 where there is none; 0 the background, k plane k), u and v float
 * (texture coordinates of the hit, 0 where there is none).  A pixel no object covers, or that does not reconstruct, is written
 * as 0.  counts (HOST int64 [n][VG_RENDER_COUNTS], may be NULL): pixels that do not reconstruct, pixels covered by nothing,
 * background pixels, plane pixels, and covered pixels sampled with the single bicubic tap. */
int vg_render_views(vg_render *h, int64_t n, const double *xi_cam, uint8_t *image, float *depth, int16_t *index, float *u, float *v,
                    int64_t *counts);
/* Host only: the anti-aliasing kernel of `length` taps, length in [1, 24], out HOST [length] -- one row of LookupFilter's table
 * (sigma 0.55, 600 integral samples) as the device reads it. */
int vg_render_filter_kernel(int length, double *out);

/* =====================================================================================
 * 15. Monocular visual odometry: the reference's MonoOdometry (include/localization/mono_odom.h, src/localization/mono_odom.cpp)
 *     -- wheel-odometry poses and camera images in, one after the other; the pose of the base frame and a key frame depth map
 *     that improves with every frame out.  The handle owns one each of the pipelines of sections 10 to 13 and builds one
 *     section 9 object per key frame; images and maps stay on the device between the stages of a frame.  Images are DEVICE u8
 *     [height][width] with width = u_max and height = v_max of the stereo parameters, maps DEVICE FP64 [y_max][x_max], poses
 *     HOST [t, rotvec] of the base frame.  Every call is synchronous on the handle's stream and checks its arguments before
 *     HIP is touched.  Deviations: DESIGN.md section 9, "Monocular odometry".
 * ===================================================================================== */
#define VG_MONO_ODOM_BEGIN 0             /* states: no image yet */
#define VG_MONO_ODOM_SPARSE_INIT 1       /* a first key image, no depth map: waiting for min_init_dist of odometry */
#define VG_MONO_ODOM_READY 2             /* a key frame with a depth map */
#define VG_MONO_ODOM_FIRST 0             /* actions of a feed_image call: the first image was kept */
#define VG_MONO_ODOM_WAITING 1           /* SPARSE_INIT, the odometry has not moved far enough: nothing done */
#define VG_MONO_ODOM_SPARSE_INIT_KEYFRAME 2 /* sparse odometry gave the motion, SGM the first map */
#define VG_MONO_ODOM_REFINED 3           /* pose from the photometric solve, map refined by motion stereo and filtered */
#define VG_MONO_ODOM_KEYFRAME 4          /* pose from the photometric solve, then a new key frame */
#define VG_MONO_ODOM_DISCARDED 5         /* the photometric pose disagreed with the odometry's scale: the odometry is kept */
#define VG_MONO_ODOM_REPORT 16           /* state before, state after, action, K, length, length_prior; of the photometric solve the
                                            iterations over all scales and the finest scale's final cost and vg_termination; six
                                            counters: of vg_motion_stereo_compute on REFINED (zeros when the refinement was skipped),
                                            of vg_depth_merge (five) on KEYFRAME, zeros otherwise; the number of key frames */
typedef struct vg_mono_odom vg_mono_odom;
typedef struct vg_mono_odom_params {
    double min_init_dist;      /* MIN_INIT_DIST 0.25: odometry translation that ends SPARSE_INIT */
    double max_dist;           /* MAX_DIST 0.4: |t(xi_local)| above it asks for a key frame */
    double max_angle;          /* MAX_ANGLE pi / 4: |rot(xi_local)| above it asks for a key frame */
    double min_scale_length;   /* 1e-2: the scale of a shorter photometric step is not touched */
    double max_scale_ratio;    /* 1.2: a step K times shorter than the odometry's, K above it, is discarded */
    int num_scales;            /* 5: pyramid levels of the photometric solve */
    vg_motion_stereo_params motion;   /* "stereo_parameters": SGM reads motion.stereo, motion stereo all of it */
    vg_sparse_odom_params sparse;
} vg_mono_odom_params;
void vg_mono_odom_params_default(vg_mono_odom_params *p);
/* MonoOdometry(ptree): eucm HOST 6 intrinsics, xi_base_cam HOST [6] the camera in the base frame, width x height the image size
 * (equal to u_max x v_max of params->motion.stereo).  The thresholds must be finite, the distances and the angle not negative,
 * max_scale_ratio positive; everything else is checked by the creation of the four pipelines, all of them before the device
 * is asked for.  Allocates the key image and three map triples; later calls allocate only what the pipelines' first calls
 * and the per-key-frame vg_stereo object need. */
int vg_mono_odom_create(vg_mono_odom **out, int device, void *hip_stream, const double *eucm, const double *xi_base_cam, int width,
                        int height, const vg_mono_odom_params *params);
void vg_mono_odom_destroy(vg_mono_odom *h);
int vg_mono_odom_size(const vg_mono_odom *h, int *width, int *height, int *x_max, int *y_max);
/* feedWheelOdometry (:54-61): xi_local = xi_local o xi_odom^-1 o xi_odom_new, xi_odom = xi_odom_new.  The first call only
 * records xi_odom_new. */
int vg_mono_odom_feed_wheel_odometry(vg_mono_odom *h, const double *xi_odom_new);
/* feedImage (:81-173) with pushKeyFrame (:175-216): img DEVICE u8 [height][width]; samples as for vg_sparse_odom_feed (HOST
 * int32 [ransac_iterations][num_ransac_points] or NULL for the library's draw), passed on in BEGIN and SPARSE_INIT; report HOST
 * [VG_MONO_ODOM_REPORT] or NULL.  A call in which a stage fails leaves the poses, the state and the map as they were (a frame
 * writes its maps into scratch and commits last; only the copy of a new key image and motion stereo's set_base, the first
 * steps of that commit, can still fail, and are not undone). */
int vg_mono_odom_feed_image(vg_mono_odom *h, const uint8_t *img, const int32_t *samples, double *report);
/* setDepth (:63-79): depth_image DEVICE float [height][width] (the renderer's depth buffer); map(x, y) = image(v0 + y scale, u0 +
 * x scale), sigma 0.1 everywhere, the cost left as it is (5 in a map that did not exist).  A cell whose pixel lies outside the
 * image holds 0.  In SPARSE_INIT the map is replaced by the first key frame's SGM map all the same. */
int vg_mono_odom_set_depth(vg_mono_odom *h, const float *depth_image);
/* ScalePhotometric::wrapImage (photometric.cpp:387-415): dst(i, j) = src at the rounded projection of key frame pixel (j, i)'s
 * point -- the ray of the pixel at the depth of its nearest map cell -- seen from the pose xi (HOST [6] of the base frame in
 * the key frame's; NULL: the current xi_local); 0 where the cell lies outside the map, its depth is below MIN_DEPTH, the pixel
 * does not reconstruct, the point does not project or lands outside src.  depth DEVICE FP64 [y_max][x_max], NULL: the
 * handle's map.  src, dst DEVICE u8 [height][width], not overlapping.  One thread per pixel, a pure gather: bit-identical
 * from run to run. */
int vg_mono_odom_warp_image(vg_mono_odom *h, const uint8_t *src, const double *xi, const double *depth, uint8_t *dst);
int vg_mono_odom_state(const vg_mono_odom *h, int *state);
int vg_mono_odom_xi_local(const vg_mono_odom *h, double *xi6);
int vg_mono_odom_xi_global(const vg_mono_odom *h, double *xi6);
int vg_mono_odom_xi_composed(const vg_mono_odom *h, double *xi6);   /* xi_global o xi_local */
/* transfVec: the number of key frames so far and the pose of key frame k in key frame k - 1 (zero for k = 0) */
int vg_mono_odom_num_keyframes(const vg_mono_odom *h, int64_t *count);
int vg_mono_odom_keyframe_increment(const vg_mono_odom *h, int64_t k, double *xi6);
/* The current map: copied device to device into the caller's arrays (each may be NULL), or as borrowed DEVICE pointers that
 * stay valid until the next feed_image or set_depth.  VG_ERR_STATE while there is no map. */
int vg_mono_odom_get_map(vg_mono_odom *h, double *depth, double *sigma, double *cost);
int vg_mono_odom_map(const vg_mono_odom *h, const double **depth, const double **sigma, const double **cost);
/* Host only -- the state machine's arithmetic, the code the feed calls run:
 *   integrate        xi_local o xi_odom_old^-1 o xi_odom_new
 *   normalize_scale  zetaPrior = old^-1 o prior, zeta = old^-1 o vo, K = |t(zetaPrior)| / |t(zeta)| (*K, may be NULL; not finite
 *                    for a pure rotation).  |t(zeta)| > min_scale_length and K > max_scale_ratio: out = old o zetaPrior and
 *                    *discarded = 1.  Otherwise *discarded = 0 and out = old o zeta, t(zeta) times K first when |t(zeta)| >
 *                    min_scale_length.
 *   needs_keyframe   *needed = |t| > max_dist or |rot| > max_angle
 *   camera_motion    xi_base_cam^-1 o xi o xi_base_cam
 *   compose          a o b */
int vg_mono_odom_integrate(const double *xi_local, const double *xi_odom_old, const double *xi_odom_new, double *out6);
int vg_mono_odom_normalize_scale(const vg_mono_odom_params *params, const double *xi_local_old, const double *xi_local_prior,
                                 const double *xi_local_vo, double *out6, double *K, int *discarded);
int vg_mono_odom_needs_keyframe(const vg_mono_odom_params *params, const double *xi_local, int *needed);
int vg_mono_odom_camera_motion(const double *xi_base_cam, const double *xi, double *out6);
int vg_mono_odom_compose(const double *a6, const double *b6, double *out6);

/* =====================================================================================
 * 16. Photometric mapping: the reference's PhotometricMapping (include/localization/mapping.h, src/localization/mapping.cpp) --
 *     a persistent map of key frames (image + global pose of the base frame), an inter frame with a depth map that is localized
 *     against the nearest map frame by mutual information (section 12, vg_mi_compute_pose with its odometry term), and the
 *     current frame localized photometrically against the inter frame.  Where the map has no frame near enough the loop runs
 *     as SLAM and the inter frames it leaves behind become the map.  The handle owns one each of the pipelines of sections 10
 *     to 13, builds one section 9 object per inter frame, and keeps the map's images on the device in a pool that grows by
 *     whole chunks (a stored image never moves); the map's poses are host data.  Images are DEVICE u8 [height][width] with
 *     width = u_max and height = v_max of the stereo parameters, maps DEVICE FP64 [y_max][x_max], poses HOST [t, rotvec] of the
 *     base frame.  Every call is synchronous on the handle's stream and checks its arguments before HIP is touched.
 *     ODOM_MODE (false in the reference) is not built.  Deviations: DESIGN.md section 9, "Photometric mapping".
 * ===================================================================================== */
#define VG_MAPPING_BEGIN 0               /* states: no image since creation / reinit */
#define VG_MAPPING_INIT 1                /* an inter image, no depth map: waiting for min_init_dist of odometry */
#define VG_MAPPING_LOCALIZE 2            /* the inter frame is tied to map frame map_index */
#define VG_MAPPING_SLAM 3                /* no map frame near: the inter frames are pushed into the map */
#define VG_MAPPING_WARNING_NONE 0
#define VG_MAPPING_WARNING_SCALE 1       /* the photometric step's length disagreed with the odometry's: the odometry is kept */
#define VG_MAPPING_WARNING_ROTATION 2    /* its rotation component 2 disagreed: the odometry is kept */
#define VG_MAPPING_FIRST 0               /* actions of a feed_image call.  BEGIN: the image was kept */
#define VG_MAPPING_WAITING 1             /* INIT, the odometry has not moved far enough: nothing done */
#define VG_MAPPING_INIT_SLAM 2           /* INIT: sparse odometry, first inter frame, no map frame near -> SLAM */
#define VG_MAPPING_INIT_LOCALIZE 3       /* INIT: the same, a map frame near -> LOCALIZE, MI */
#define VG_MAPPING_LOCALIZE_REFINED 4    /* LOCALIZE, both distances hold: improveStereo */
#define VG_MAPPING_LOCALIZE_INTER_FRAME 5 /* LOCALIZE, only the inter distance fails: new inter frame, MI against the same map frame */
#define VG_MAPPING_LOCALIZE_MAP_FRAME_CHANGED 6 /* LOCALIZE, the map distance fails: new inter frame, another map frame, MI */
#define VG_MAPPING_LOCALIZE_MAP_FRAME_KEPT 7 /* the same, but the selection returns the old index: no MI (as the reference) */
#define VG_MAPPING_LOCALIZE_LEFT_MAP 8   /* the same, no map frame near -> SLAM */
#define VG_MAPPING_SLAM_REFINED 9        /* SLAM, the inter distance holds: improveStereo */
#define VG_MAPPING_SLAM_INTER_FRAME 10   /* SLAM, it fails: the old inter frame into the map, new inter frame, no map frame near */
#define VG_MAPPING_SLAM_ENTERED_MAP 11   /* the same, a map frame near (with K = 4 normally the one just pushed) -> LOCALIZE, MI */
#define VG_MAPPING_REPORT 32             /* [0] state before, state after, action, warning, [4] map index before, after, [6] K, length,
                                            length_prior, |rot2(zeta) - rot2(zetaPrior)| (zeros when no photometric solve ran or
                                            normalize_scale is off); [10] of the photometric solve the iterations over all scales and
                                            the finest scale's final cost and vg_termination; [13] of the MI solve the iterations over all
                                            scales and the finest non-empty scale's initial cost, final cost and vg_termination (zeros when
                                            no MI ran); [17] 1 when SGM ran, [18] 1 when motion stereo refined the map; [19] the six
                                            counters of vg_motion_stereo_compute; [25] the five of vg_depth_merge; [30] frames in the map;
                                            [31] 0 */
typedef struct vg_mapping vg_mapping;
typedef struct vg_mapping_params {
    double new_kf_distance_thresh; /* STORED SQUARED (distThreshSq 0.03): t0^2 / 5 + t1^2 + t2^2 below it (times K) is near */
    double new_kf_angular_thresh;  /* STORED SQUARED (angularThreshSq 0.25): |rot|^2 below it is near; not scaled by K */
    double min_init_dist;          /* 0.1: odometry translation that ends INIT */
    double min_stereo_base;        /* 0.07: below this camera translation neither SGM nor motion stereo runs */
    double dist_thresh;            /* 5: parsed and unused, as in the reference (maxDistance) */
    int normalize_scale;           /* 1 */
    double rotation_tolerance;     /* 0.005: on component 2 of the rotation vector of the step (localizePhoto's literal) */
    double min_scale_length;       /* 1e-2: the scale of a shorter photometric step is not touched */
    double min_scale_ratio;        /* 0.8 */
    double max_scale_ratio;        /* 1.2: K = |t(odometry step)| / |t(photometric step)| outside the two keeps the odometry */
    int num_scales;                /* 5: pyramid levels of both solves */
    vg_motion_stereo_params motion;   /* "stereo_parameters": SGM reads motion.stereo, motion stereo all of it */
    vg_sparse_odom_params sparse;
} vg_mapping_params;
void vg_mapping_params_default(vg_mapping_params *p);
/* PhotometricMapping(ptree): arguments as vg_mono_odom_create.  The thresholds must be finite and not negative, the scale ratios
 * positive with min <= max.  Allocates the inter image and three map triples; the frame store allocates a chunk when the one
 * before it is full. */
int vg_mapping_create(vg_mapping **out, int device, void *hip_stream, const double *eucm, const double *xi_base_cam, int width, int height,
                      const vg_mapping_params *params);
void vg_mapping_destroy(vg_mapping *h);
int vg_mapping_size(const vg_mapping *h, int *width, int *height, int *x_max, int *y_max);
/* feedOdometry (:62-74): xi_local = xi_local o xi_odom^-1 o xi_odom_new; the first call (and the first after reinit) only records. */
int vg_mapping_feed_odometry(vg_mapping *h, const double *xi_odom_new);
/* reInit (:262-273): in SLAM the inter frame is pushed into the map first; the state becomes BEGIN, xi_local = xi_local_old = xi
 * (HOST [6], the global pose of the base frame the next pass starts at), the odometry is forgotten. */
int vg_mapping_reinit(vg_mapping *h, const double *xi);
/* feedImage (:78-179) with pushInterFrame, improveStereo, localizePhoto and localizeMI: img DEVICE u8 [height][width]; samples as
 * for vg_sparse_odom_feed, passed on in BEGIN and INIT; report HOST [VG_MAPPING_REPORT] or NULL.  A frame works on copies of the
 * poses, writes its maps into scratch and commits state, poses, map, inter image and frame store last: a call in which a stage
 * fails leaves them as they were (only the copies of the commit itself and motion stereo's set_base can still fail, and are not
 * undone).  In INIT a camera translation of the sparse increment not above min_stereo_base -- where the reference executes a
 * bare throw -- fails with VG_ERR_STATE and commits nothing: the caller re-initialises with vg_mapping_reinit.  The photometric
 * solve starts at xi_local with xi_local as the prior's pose; the key frame's packs are rebuilt from the map by
 * vg_photo_set_depth.  One vg_photometric handle serves the photometric and the MI solve. */
int vg_mapping_feed_image(vg_mapping *h, const uint8_t *img, const int32_t *samples, double *report);
/* The frame store.  get_frame: pose to xi6 (HOST [6], may be NULL), image to img (DEVICE u8, may be NULL).  add_frame: an
 * unconditional insert (reloading a saved map).  construct_map is constructMap (:45-60): inserts when select_frame(xi, K = 1)
 * finds nothing; *inserted 1 or 0.  select_frame is selectMapFrame on the store (*idx -1: none). */
int vg_mapping_num_frames(const vg_mapping *h, int64_t *count);
int vg_mapping_get_frame(vg_mapping *h, int64_t k, double *xi6, uint8_t *img);
int vg_mapping_add_frame(vg_mapping *h, const double *xi, const uint8_t *img);
int vg_mapping_construct_map(vg_mapping *h, const double *xi, const uint8_t *img, int *inserted);
int vg_mapping_select_frame(const vg_mapping *h, const double *xi, double K, int *idx);
/* The alignment signal both reference programs look at, in one launch: wrapImage of img (DEVICE u8) at the pose xi (HOST [6],
 * NULL: xi_local) through depth (DEVICE FP64 [y_max][x_max], NULL: the handle's map), exactly the values
 * vg_mono_odom_warp_image writes; computeErr against base (DEVICE u8, NULL: the inter image): err (DEVICE u8 [height][width], may
 * be NULL, must not overlap img) is 0 where either pixel is 0, else 127 + base - warped SATURATED to [0, 255] (the reference's
 * conversion wraps); sums HOST int64 [3]: compared pixels, sum |base - warped|, sum (base - warped)^2.  Integer sums: bit-identical
 * from run to run.  VG_ERR_STATE when a default is asked for that does not exist yet. */
int vg_mapping_alignment(vg_mapping *h, const uint8_t *base, const uint8_t *img, const double *xi, const double *depth, uint8_t *err,
                         int64_t *sums);
int vg_mapping_state(const vg_mapping *h, int *state);
int vg_mapping_map_index(const vg_mapping *h, int *idx);      /* -1 until a selection has run */
int vg_mapping_warning(const vg_mapping *h, int *warning);    /* of the last photometric solve */
int vg_mapping_xi_local(const vg_mapping *h, double *xi6);
int vg_mapping_xi_inter(const vg_mapping *h, double *xi6);    /* the inter frame's global pose */
int vg_mapping_xi_composed(const vg_mapping *h, double *xi6); /* xi_inter o xi_local, what both programs log */
/* The inter frame's depth map, as vg_mono_odom_get_map / vg_mono_odom_map; VG_ERR_STATE while there is none. */
int vg_mapping_get_map(vg_mapping *h, double *depth, double *sigma, double *cost);
int vg_mapping_map(const vg_mapping *h, const double **depth, const double **sigma, const double **cost);
/* Host only -- the state machine's arithmetic, the code the feed calls run:
 *   check_distance     *ok = |rot|^2 < new_kf_angular_thresh and t0^2 / 5 + t1^2 + t2^2 < new_kf_distance_thresh K
 *   select_frame_host  over poses HOST [n][6]: delta = xi^-1 o pose; among those that pass check_distance(delta, K) the smallest
 *                      |rot|^2 + |t|^2 (isotropic), the first on a tie; *idx -1 when none.  selectMapFrame's default K is 4.
 *   normalize_scale    zetaPrior = old^-1 o prior, zeta = old^-1 o vo.  |rot2(zeta) - rot2(zetaPrior)| > rotation_tolerance: out =
 *                      old o zetaPrior, ROTATION.  Else with |t(zeta)| > min_scale_length: K = |t(zetaPrior)| / |t(zeta)| outside
 *                      [min_scale_ratio, max_scale_ratio]: out = old o zetaPrior, SCALE; inside: out = old o zeta with t(zeta)
 *                      times K.  A shorter step: out = vo.  The caller sets xi_local_old = out in every one of these branches.
 *                      normalize_scale 0: out = vo, the numbers are zero, xi_local_old is left alone.  K, length, length_prior,
 *                      rot_diff may each be NULL.
 *   relocalized_pose   localizeMI's last line: the inter frame's global pose xi_map o xi_fr_map^-1 from the map frame's pose and
 *                      the map frame's pose in the inter frame (composeInverse). */
int vg_mapping_check_distance(const vg_mapping_params *params, const double *xi, double K, int *ok);
int vg_mapping_select_frame_host(const vg_mapping_params *params, int64_t n, const double *poses, const double *xi, double K, int *idx);
int vg_mapping_normalize_scale(const vg_mapping_params *params, const double *xi_local_old, const double *xi_local_prior,
                               const double *xi_local_vo, double *out6, double *K, double *length, double *length_prior, double *rot_diff,
                               int *warning);
int vg_mapping_relocalized_pose(const double *xi_map, const double *xi_fr_map, double *out6);

/* =====================================================================================
 * 17. Calibration trajectory planning: the reference's TrajectoryVisualQuality (include/calibration/trajectory_generation.h,
 *     src/calibration/trajectory_generation.cpp:86-281) over circular trajectories (CircularTrajectory,
 *     test/calibration/trajectory.cpp:27-82) -- the robot trajectories to drive in front of a calibration board so that the
 *     camera-odometry extrinsics become well observable.  A parameter point is HOST [5 T]: per trajectory x0, y0, theta0, the
 *     chord d and the turn alpha of one step.  The cost of a point is -log det H plus four penalties, H = diag(1 /
 *     prior_variance) + sum over every trajectory and every pose i >= 1 of J^T C^-1 J (C: the visual covariance of the board
 *     seen from the pose plus the transported odometry covariance).  The handle owns the device scratch of a batch; every array
 *     of this section is HOST memory; every call is synchronous on the handle's stream and checks its arguments before HIP is
 *     touched.  A batch of n points costs three launches whatever n is; a point's result does not depend on the batch it is in.
 *     A pose with a corner that does not project, or whose JtCJ or C has no finite inverse, is INVALID: the point's cost is
 *     +inf and invalid[] counts such poses.  EUCM only (VG_MODEL_EUCM; the other models: VG_ERR_INVALID_ARGUMENT).
 *     TrajectoryQuality, the constant-covariance variant nothing calls, is not built.  Deviations: DESIGN.md section 9,
 *     "Trajectory planning".
 * ===================================================================================== */
#define VG_TRAJECTORY_PARAMS 5           /* parameters of one trajectory */
#define VG_TRAJECTORY_MAX 8              /* trajectories of a handle */
#define VG_TRAJECTORY_MIN_STEPS 2        /* poses of one trajectory (number_steps), pose 0 included */
#define VG_TRAJECTORY_MAX_STEPS 256
#define VG_TRAJECTORY_MAX_CORNERS 1024   /* board cols x rows */
#define VG_TRAJECTORY_TERMS 5            /* terms[]: information (-log det H), image limits, curvature, distance, normal */
#define VG_TRAJECTORY_MAX_POINTS 65535   /* points of one batch; a gradient takes 2 x 5 T + 1 of them per point */
typedef struct vg_trajectory vg_trajectory;
typedef struct vg_trajectory_quality {   /* "quality_parameters" of a plan file */
    double xi_base_cam[6];               /* xiBaseCam: the camera in the robot's frame, [t, rotvec] */
    double xi_orig_board[6];             /* xiOrigBoard: the board in the world */
    double turn_radius;                  /* the curvature penalty starts at 1 / turn_radius */
    int board_cols, board_rows;          /* >= 2 each */
    double board_step;
    double min_camera_dist, min_margin, min_cell_size;
    double prior_variance[6];
    double feature_variance;
} vg_trajectory_quality;
typedef struct vg_trajectory_options {   /* of the minimiser; vg_trajectory_default_options: Ceres' defaults */
    double function_tolerance;           /* 1e-6: |df| <= tol |f|; 0 switches the test off */
    double gradient_tolerance;           /* 1e-10: max |g| <= tol */
    double parameter_tolerance;          /* 1e-8: |dx| <= tol (|x| + tol); 0 switches the test off */
    int max_iterations;                  /* 1000 */
} vg_trajectory_options;
void vg_trajectory_default_options(vg_trajectory_options *o);
/* model, intrinsics: the camera; width, height: its image; steps HOST [n_trajectories], each in [2, 256]. */
int vg_trajectory_create(vg_trajectory **out, int device, void *hip_stream, int model, const double *intrinsics, int width, int height,
                         const vg_trajectory_quality *quality, int n_trajectories, const int *steps);
void vg_trajectory_destroy(vg_trajectory *h);
/* *n_params = 5 T, *n_poses = sum of the steps; each may be NULL */
int vg_trajectory_size(const vg_trajectory *h, int *n_trajectories, int *n_params, int *n_poses);
/* EvaluateCost at n points: params [n][5 T], cost [n], terms [n][VG_TRAJECTORY_TERMS] (may be NULL), invalid [n] (may be NULL).
 * cost = terms[0] + the penalties added pose by pose; an invalid point has cost = terms[0] = +inf and its penalty terms summed
 * over the valid poses. */
int vg_trajectory_evaluate(vg_trajectory *h, int64_t n, const double *params, double *cost, double *terms, int32_t *invalid);
/* visualCov at n camera poses [n][6] (the camera in the world): cov [n][36] = JtCJ^-T JtJ JtCJ^-1 and info [n][36] = JtJ,
 * row-major; invalid [n] is 1 where a corner does not project or JtCJ has no finite inverse, and both matrices are +inf there. */
int vg_trajectory_visual_cov(vg_trajectory *h, int64_t n, const double *cam_poses, double *cov, double *info, int32_t *invalid);
/* Evaluate: cost [n] and the central differences grad [n][5 T] with delta_i = max(|p_i| 1e-8, 1e-16), the perturbed values
 * formed as p_i + delta_i and p_i - delta_i; one batch of n (2 x 5 T + 1) points (at most VG_TRAJECTORY_MAX_POINTS).  invalid [n]
 * (may be NULL) is 1 where any of a point's evaluations is invalid; its gradient is NaN then. */
int vg_trajectory_gradient(vg_trajectory *h, int64_t n, const double *params, double *cost, double *grad, int32_t *invalid);
/* Host only: the points of one gradient, points [2 n_params + 1][n_params] -- row 0 the point itself, row 1 + 2 i with
 * p_i + delta_i, row 2 + 2 i with p_i - delta_i -- and delta [n_params]. */
int vg_trajectory_gradient_points(int n_params, const double *params, double *points, double *delta);
/* Host only: CircularTrajectory::compute for every trajectory of params [5 T]: xi [sum steps][6] and cov [sum steps][36],
 * trajectory after trajectory.  cov may be NULL. */
int vg_trajectory_poses(int n_trajectories, const int *steps, const double *params, double *xi, double *cov);
/* One minimisation per start, all in lock-step: params [n_starts][5 T] holds the starts and receives the results; every round
 * is one batch with each unfinished start's trial point and its 2 x 5 T perturbed points.  BFGS with a strong-Wolfe line search
 * (vg_bfgs.hpp) in place of Ceres' GradientProblemSolver; a trial that is invalid, or whose gradient is, is a failed trial and
 * the search shrinks towards the last valid point.  cost [n_starts]: the cost at the returned parameters; iterations and
 * termination (vg_termination) [n_starts] may be NULL.  A start that is itself invalid ends with VG_TERM_FAILURE and keeps its
 * parameters.  options NULL: the defaults. */
int vg_trajectory_optimize(vg_trajectory *h, int64_t n_starts, double *params, const vg_trajectory_options *options, double *cost,
                           int32_t *iterations, int32_t *termination);
/* Host only: the board's corners seen from the camera pose cam_pose [6] -- uv [cols rows][2], row after row of the board, and ok
 * [cols rows], projectPoint's return value (uv of a corner that does not project is what the formula gives). */
int vg_trajectory_project_board(int model, const double *intrinsics, const vg_trajectory_quality *quality, const double *cam_pose, double *uv,
                                int32_t *ok);
/* kernel launches of the handle since its creation (a measurement: the launches of a call do not depend on its n) */
int vg_trajectory_launch_count(const vg_trajectory *h, int64_t *count);

/* =====================================================================================
 * 18. Photometric bundle adjustment: the reference's dense_ba_test (test/reconstruction/dense_ba_test.cpp:38-113, 170-317) --
 *     the poses of F further frames and the depth of every selected key-frame cell refined together on the grey difference.
 *     Per frame f and point i the residual r = (I_f(project(X)) - I_0i) / sigma_grey with X = (xi_f o xi_base_cam)^-1
 *     xi_base_cam (d_i dir_i), sampled by Ceres' bicubic interpolator over the clamping grid on the full-size float image, no
 *     margin and no loss; per point the prior row p_i = lambda (d_i - d0_i) / sigma0_i; the cost is 1/2 sum r^2 + 1/2 sum p^2.
 *     The depth block of the normal equations is diagonal and is eliminated exactly (a Schur complement on the GPU), the
 *     K = 6 F pose system is solved on the host, under the trust-region rule of vg_photometric_compute_pose applied to all
 *     K + m parameters.  Single scale, EUCM, FP64.  Images are DEVICE u8, maps DEVICE FP64 [y_max][x_max], poses HOST
 *     [t, rotvec] of a frame's base in the key frame's base.  Every call is synchronous on the handle's stream and checks
 *     its arguments before HIP is touched; a call out of order gives VG_ERR_STATE.  Deviations: DESIGN.md section 9,
 *     "Photometric bundle adjustment".
 * ===================================================================================== */
#define VG_DENSE_BA_MAX_FRAMES 8
#define VG_DENSE_BA_TAIL 5               /* sum D dx^2, g . dx, |dx|^2, |x|^2, max |g| of the depth block */
#define VG_DENSE_BA_NONE (-1.0)          /* prior_weight / grad_thresh: switched off (a zero field means the default) */
#define VG_DENSE_BA_SIGMA_GREY 5.0
#define VG_DENSE_BA_PRIOR_WEIGHT 1.0
#define VG_DENSE_BA_GRAD_THRESH 250.0    /* GRAD_THRESH of initPhotometricData */
#define VG_DENSE_BA_MAX_ITERATIONS 150
#define VG_DENSE_BA_FUNCTION_TOLERANCE 1e-6
typedef struct vg_dense_ba_options {
    double sigma_grey;         /* the grey residual's sigma; 0: 5.  The reference divides the greys by 255 */
    double prior_weight;       /* lambda of the depth prior; 0: 1; negative: no prior (the reference has none) */
    double grad_thresh;        /* a cell is kept when gu^2 + gv^2 >= grad_thresh; 0: 250; negative: every cell (the reference) */
    int max_iterations;        /* 0: 150 */
    double function_tolerance; /* 0: 1e-6 */
} vg_dense_ba_options;
typedef struct vg_dense_ba vg_dense_ba;
/* A handle for one EUCM camera (eucm: HOST 6 intrinsics), the depth map's geometry (of `params` only the ScaleParameters
 * fields are read, as by vg_photometric_create), xi_base_cam (HOST [6]) and the image size.  options NULL: the defaults; a
 * negative sigma_grey, max_iterations or function_tolerance is refused. */
int vg_dense_ba_create(vg_dense_ba **out, int device, void *hip_stream, const double *eucm, const vg_stereo_params *params,
                       const double *xi_base_cam, int width, int height, const vg_dense_ba_options *options);
void vg_dense_ba_destroy(vg_dense_ba *h);
/* The key frame: its image (DEVICE u8 [height][width]), depth map and sigma map (may be NULL without a prior).  Builds the
 * pack: the cells (x, y) of the depth grid in raster order, pixel (u, v) = (uConv(x), vConv(y)), whose depth is finite and at
 * least MIN_DEPTH 0.25, whose pixel lies in the image and reconstructs, whose Sobel / 8 gradient has gu^2 + gv^2 >=
 * grad_thresh and, with a prior, whose sigma is finite and positive.  The maps are copied: they are read during the call only. */
int vg_dense_ba_set_base(vg_dense_ba *h, const uint8_t *img, const double *depth, const double *sigma);
/* The F further frames, F in [1, 8]: DEVICE u8 [F][height][width]; they replace the earlier ones. */
int vg_dense_ba_set_frames(vg_dense_ba *h, int frames, const uint8_t *imgs);
/* Stage entry: the pack.  *count (HOST) receives the number of points m; indices (DEVICE int32 [m], y x_max + x), greys (DEVICE
 * FP64 [m], 0 .. 255), dirs (DEVICE FP64 [m][3], unit), d0 and sigma0 (DEVICE FP64 [m]) may be NULL -- ask for the count first. */
int vg_dense_ba_pack(vg_dense_ba *h, int64_t *count, int32_t *indices, double *greys, double *dirs, double *d0, double *sigma0);
/* Stage entry: residuals and Jacobians at the poses xi (HOST [F][6]) and the depths (DEVICE [m]; NULL: d0).  residuals DEVICE
 * [F][m], jac_pose DEVICE [F][m][6], jac_depth DEVICE [F][m], a (the depth block's diagonal, sum_f jd^2 + (lambda / sigma0)^2)
 * and g_depth (its gradient) DEVICE [m]; cost HOST [1]; sums HOST [F][28]: per frame J_pose^T J_pose (upper triangle row-major,
 * 21), J_pose^T r (6), 1/2 sum r^2.  Any output may be NULL.  A point that does not project, or whose coordinates exceed
 * +-2^24 px, has a zero residual and zero rows.  All sums are FP64 in a fixed order: bit-identical from run to run.  The rows
 * stay in the handle for vg_dense_ba_reduce and vg_dense_ba_back_substitute. */
int vg_dense_ba_evaluate(vg_dense_ba *h, const double *xi, const double *depths, double *residuals, double *jac_pose, double *jac_depth,
                         double *a, double *g_depth, double *cost, double *sums);
/* Stage entry: the reduced system of the last evaluation under the damping mu > 0, with e_i = a_i + mu clamp(a_i, 1e-6, 1e32)
 * and w_i the stack of J_pose[f][i] jd[f][i] over the frames: S = H_pp + mu D_p - sum_i w_i w_i^T / e_i (HOST [K][K], K = 6 F,
 * symmetric) and rhs = g_p - sum_i w_i g_di / e_i (HOST [K]).  VG_ERR_STATE before an evaluation. */
int vg_dense_ba_reduce(vg_dense_ba *h, double mu, double *S, double *rhs);
/* Stage entry: the depth step of the pose step dp (HOST [K]) under mu, dd_i = -(g_di + w_i . dp) / e_i: the candidate depths
 * d_i + dd_i (DEVICE [m], may be NULL) and the depth block's share of the rule's sums (HOST [VG_DENSE_BA_TAIL]). */
int vg_dense_ba_back_substitute(vg_dense_ba *h, double mu, const double *dp, double *candidate, double *tail);
/* The solve from the start poses (HOST [F][6]) and the key frame's depths: xi_out HOST [F][6]; depth_out / sigma_out DEVICE
 * [y_max][x_max] (may be NULL): the input maps outside the pack, the refined depth and 1 / sqrt(a_i) at the solution inside it;
 * report HOST [4] (may be NULL): iterations, initial cost, final cost, vg_termination.  An empty pack is refused. */
int vg_dense_ba_solve(vg_dense_ba *h, const double *xi_start, double *xi_out, double *depth_out, double *sigma_out, double *report);

/* =====================================================================================
 * 19. Fisheye line detection: the reference's hough_test (test/reconstruction/hough_test.cpp) -- straight 3D lines in one
 *     unrectified EUCM image.  Every pixel with a strong Sobel gradient defines the plane through the projection centre that
 *     contains its edge; the plane's normal, projected through a second, small EUCM "accumulator camera", votes in an int32
 *     accumulator; the accumulator is blurred (float, 5 x 5 Gaussian) and its strict local maxima are the lines; a line's
 *     image is the conic vg_hough_polynomial gives, walked by the curve rasteriser between its end points.  FP64 in the
 *     reference's expression order, integer votes: the same bytes on every run.  Images are DEVICE u8.  Every call is
 *     synchronous on the handle's stream and checks its arguments before HIP is touched.  Deviations: DESIGN.md section 9,
 *     "Line detection".
 * ===================================================================================== */
#define VG_HOUGH_MAX_SIDE 16384
#define VG_HOUGH_MAX_ACC_SIDE 4096
#define VG_HOUGH_MAX_SEARCH 8
#define VG_HOUGH_MIN_BLUR 3
#define VG_HOUGH_MAX_BLUR 15
#define VG_HOUGH_COUNTS 6       /* selected pixels, not reconstructed, first votes cast, antipode votes cast, projections
                                   failed, votes outside the accumulator */
#define VG_HOUGH_LINE 16        /* centroid u, v; blurred value; unit normal [3]; poly6; pt1 [2]; pt2 [2] */
#define VG_HOUGH_MAX_LINES 65536
#define VG_HOUGH_MAX_TRACE 1500  /* LENGTH of the reference's trace */
#define VG_HOUGH_OK 0
#define VG_HOUGH_NO_END_POINTS 1
typedef struct vg_hough_params {
    int margin;               /* MARGIN 5: pixels this close to the border are not visited; at least 1 */
    double grad_thresh;       /* GRAD_THRESH 0.001 on gx^2 + gy^2 of the Sobel / 2048 gradient */
    int search_size;          /* SEARCH_SIZE 2: a maximum beats its (2 s + 1)^2 - 1 neighbours; in [1, 8] */
    double acc_thresh;        /* ACC_THRESH 7 */
    double acc_delta_thresh;  /* ACC_DELTA_THRESH 0.05 */
    double horizon_ratio;     /* 3e-3: C^2 / (A^2 + B^2) below it votes at the antipode as well */
    int blur_size;            /* 5, odd, in [3, 15] */
    double blur_sigma;        /* 0.9 */
} vg_hough_params;
typedef struct vg_hough vg_hough;
void vg_hough_params_default(vg_hough_params *p);
/* A handle for width x height images of the camera eucm6 (HOST 6 intrinsics) voting through the accumulator camera acc_eucm6:
 * the accumulator is int32 [acc_h][acc_w], acc_w = (int)(2 u0_acc), acc_h = (int)(2 v0_acc).  Image sides in
 * [2 margin + 3, 16384]; accumulator sides in [2 search_size + 3, 4096] and at least (blur_size + 1) / 2.  params NULL: the
 * defaults. */
int vg_hough_create(vg_hough **out, int device, void *hip_stream, int width, int height, const double *eucm6, const double *acc_eucm6,
                    const vg_hough_params *params);
void vg_hough_destroy(vg_hough *h);
int vg_hough_size(const vg_hough *h, int *acc_w, int *acc_h);
/* Stage entry: the votes of n images (DEVICE u8 [n][height][width]) into acc (DEVICE int32 [n][acc_h][acc_w], cleared first).
 * counts HOST int64 [n][VG_HOUGH_COUNTS] or NULL.  A pixel that does not reconstruct, a projection that fails and a vote
 * outside the accumulator cast nothing and are counted. */
int vg_hough_vote(vg_hough *h, int64_t n_images, const uint8_t *images, int32_t *acc, int64_t *counts);
/* Votes, blur, maxima and the lines of n images.  lines HOST [n][max_lines][VG_HOUGH_LINE], status HOST int32 [n][max_lines]
 * (VG_HOUGH_OK or VG_HOUGH_NO_END_POINTS: both end points are NaN then), count HOST int32 [n]: the lines found, which may
 * exceed max_lines -- the first max_lines in raster order of the accumulator are returned.  poly6 is vg_hough_polynomial of
 * the reconstructed, unnormalised normal, as in the reference.  acc_blur DEVICE float [n][acc_h][acc_w] or NULL. */
int vg_hough_detect(vg_hough *h, int64_t n_images, const uint8_t *images, int max_lines, double *lines, int32_t *status, int32_t *count,
                    float *acc_blur);
/* Host only: computePolynomial (hough_test.cpp:31-91) of the plane A x + B y + C z = 0 in the camera eucm6. */
int vg_hough_polynomial(const double *eucm6, const double *plane3, double *poly6);
/* Host only: findTerminalPoints (hough_test.cpp:100-283): pt4 = pt1, pt2; *status VG_HOUGH_OK, or VG_HOUGH_NO_END_POINTS and
 * pt4 all NaN when a point outside the image cannot be brought to its border. */
int vg_hough_end_points(int width, int height, const double *eucm6, const double *plane3, const double *poly6, double *pt4, int *status);
/* Host only: the walk of hough_test.cpp:499-536 from round(pt1) towards round(pt2): the pixels visited until the walk is within
 * 2 px (L1) of pt2, at most max_steps (in [0, VG_HOUGH_MAX_TRACE]) of them; uv int32 [max_steps][2], *n the number written.  End points must
 * be within +-2^24. */
int vg_hough_trace(const double *poly6, const double *pt4, int max_steps, int32_t *uv, int *n);

/* =====================================================================================
 * 20. Conversion between camera models: a camera calibrated in one model (Kannala-Brandt, say) brought to another one (EUCM,
 *     which the image pipelines take).  Pixels to unit rays for every model; the remap maps from one camera into another, which
 *     feed vg_remap of section 7 unchanged; and a least-squares fit of a model's intrinsics to a calibrated camera.  The
 *     unprojection of one pixel is visgeom_amd/csrc/vg_unproject.hpp; its order of operations and the fit's rule are DESIGN.md
 *     section 5.27, the deviations from the reference's reconstructPoint DESIGN.md section 9.  All five models, in every
 *     combination; every entry checks its arguments before HIP is touched.
 * ===================================================================================== */
/* n pixels uv DEVICE [n][2] of the camera (model, intrinsics HOST) to unit rays DEVICE [n][3] and ok DEVICE u8 [n].  A pixel
 * outside the model's domain, and a NaN or infinite pixel, gives the ray (0, 0, 0) and ok 0.  Stateless and asynchronous on
 * hip_stream like section 7: no allocation, no synchronisation.  n in [0, 2^31). */
int vg_unproject(int device, void *hip_stream, int model, const double *intrinsics, int64_t n, const double *uv, double *rays,
                 uint8_t *ok);
/* The maps that resample an image of the SOURCE camera into the DESTINATION camera: pixel (j, i) of the destination is
 * unprojected by the destination model, turned by R(rotvec3) (HOST, destination -> source frame; NULL = no rotation; the models
 * are central, so there is no translation) and projected by the source model in FP64; map_x / map_y DEVICE float
 * [height][width] receive the projection rounded to float, (-1, -1) where the unprojection or the projection fails.  The same
 * model on both sides turns a camera or changes its intrinsics.  Sides in [1, 16384].  Stateless and asynchronous. */
int vg_convert_map(int device, void *hip_stream, int dst_model, const double *dst_intrinsics, int src_model, const double *src_intrinsics,
                   const double *rotvec3, int width, int height, float *map_x, float *map_y);
/* Host only: the default start of the fit.  With f0 the source's paraxial focal lengths ((fu, fv) for EUCM and Kannala-Brandt,
 * (fu, fv) / (1 + xi) for UCM, Mei and double sphere) and c its centre: EUCM [0.5, 1, f0, c], UCM [1, 2 f0, c],
 * Mei [1, 0, 0, 0, 0, 0, 2 f0, c], Kannala-Brandt [0, 0, 0, 0, f0, c], double sphere [0, 0.5, f0, c]. */
int vg_convert_start(int src_model, const double *src_intrinsics, int dst_model, double *dst_intrinsics);
typedef struct vg_convert_fit_options {
    int grid_w, grid_h;           /* 64 x 40 samples; at least 1 each, product at most 2^20 */
    double max_angle;             /* pi: samples whose ray is further than this (radians) from the optical axis are dropped */
    int max_iterations;           /* 100 */
    double function_tolerance;    /* 1e-6   Ceres' defaults */
    double gradient_tolerance;    /* 1e-10 */
    double parameter_tolerance;   /* 1e-8 */
    int use_bounds;               /* 1: candidates are kept on the vg_intrinsic_bounds box */
} vg_convert_fit_options;
typedef struct vg_convert_fit_summary {
    int kept, dropped;            /* samples; kept + dropped = grid_w grid_h */
    int iterations, termination;  /* enum vg_termination */
    double initial_cost, final_cost;   /* 1/2 sum of squared pixel residuals over the kept samples */
    double rms, max_residual;     /* pixels, over the kept samples at the returned point */
} vg_convert_fit_summary;
void vg_convert_fit_default_options(vg_convert_fit_options *o);
/* Fits dst_model's intrinsics to the camera (src_model, src_intrinsics HOST) of a width x height image.  Samples: the pixels
 * u = (a + 0.5) width / grid_w - 0.5, v = (b + 0.5) height / grid_h - 0.5, unprojected on the device by the source model; one
 * that fails or lies beyond max_angle is dropped.  Cost: 1/2 sum |project_dst(ray) - (u, v)|^2, minimised by the trust-region rule
 * of the pose solves (Ceres' acceptance and tolerances) from dst_intrinsics (HOST, in / out; a NaN first value means
 * vg_convert_start).  The sums of an evaluation are reduced in a fixed order: two calls return the same bits.  Synchronous.
 * options NULL: the defaults; summary may be NULL.  Fewer than K / 2 kept samples: VG_ERR_INVALID_ARGUMENT; a start that cannot
 * project every kept sample: VG_ERR_NUMERIC, the text names the first one. */
int vg_convert_fit(int device, void *hip_stream, int src_model, const double *src_intrinsics, int width, int height, int dst_model,
                   double *dst_intrinsics, const vg_convert_fit_options *options, vg_convert_fit_summary *summary);

/* ---- measurement / test hooks.  The library reads no environment variable to change what it computes or how; the
 * switches used by tests/ and tools/ are set here (process-wide, not thread safe): "inline_chain_max_bytes", "gram_no_merge",
 * "max_obs_per_launch", "solver_timing", "solver_host_loop", "solver_device_loop", "solver_no_fold_frames",
 * "solver_fold_max_groups", "emit_nt_min_bytes", "host_chunk_bytes", "gram_persistent", "emit_map_window" (what each does:
 * enum DebugHook, visgeom_amd/csrc/vg_internal.hpp); value 0 restores the default.  The PRODUCTION library (python -m visgeom_amd._build --production, built without VG_DEBUG_HOOKS) has none of them:
 * every switch is its default at compile time and this entry is not exported.  (VG_RCCL_LIBRARY, the path of the RCCL library to
 * bind, is deployment configuration, not a hook.) */
int vg_debug_set(const char *name, long long value);

/* ---- measurement helpers (bench / profiling only): a pure streaming write / copy with the same
 * 16 B-per-lane access pattern as the emit kernel, to calibrate rocprofv3's WRITE_SIZE / FETCH_SIZE
 * and to measure the achievable HBM rate on the box. */
int vg_calib_stream_write(void *hip_stream, double *dst, int64_t n_doubles, double value);
int vg_calib_stream_copy(void *hip_stream, double *dst, const double *src, int64_t n_doubles);
/* what the FP64 vector pipe delivers on this box at the occupancy of the fused Gram kernels (two waves per SIMD): one launch of
 * dependent-FMA chains (eight per lane, `iters` FMAs each) on `hip_stream`; *flops_out = the launch's flop count.  `scratch`:
 * any device buffer of at least 2 x (number of CUs) doubles (never written in practice).  The caller times the launch. */
int vg_calib_fp64_fma(void *hip_stream, double *scratch, int iters, int64_t *flops_out);
/* the bus ceiling of the host-memory route on this box: `reps` blocking hipMemcpy device -> hipHostMalloc memory of `bytes`
 * bytes each (buffers allocated and touched first); seconds_out[reps] receives the duration of every copy. */
int vg_calib_d2h_copies(int device, int64_t bytes, int reps, double *seconds_out);

#ifdef __cplusplus
}
#endif
#endif /* VISGEOM_AMD_H */
