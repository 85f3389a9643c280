/*
 * mmk.h — C ABI of libmmk_hip.so: the MI355X (gfx950) implementation of the
 * mm_masking learned-mask -> differentiable-ICP hot path.
 *
 * The reference (utiasASRL/mm_masking) is pure Python and has NO FFI of its own
 * (SURVEY.md §2.1, §8b): each entry point below therefore cites the reference
 * *Python* interface it replaces; the binding a maintainer adds is the ctypes
 * stub shown in INTEGRATION.md (shipped as mm_masking_amd/_lib.py).
 *
 * Conventions
 *  - Every pointer is a DEVICE pointer owned by the caller unless marked host.
 *    Kernels never allocate or free memory; scratch comes in through
 *    (workspace, workspace_bytes) whose size the *_workspace_bytes() helpers give.
 *  - All work is enqueued on `stream` (a hipStream_t passed as void*) and returns
 *    without synchronising (exception: mmk_icp_forward with check_every > 0).
 *  - Return value: 0 on success, negative MMK_ERR_* otherwise; a message for the
 *    calling thread is available from mmk_last_error().  No exceptions cross
 *    the ABI, no global mutable state: safe for one-process-per-GPU use.
 *  - Tensors are dense row-major fp32 unless stated; B = scan pairs in the batch.
 */
#ifndef MMK_H_
#define MMK_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMK_VERSION 502 /* 0.5.2: mmk_voxel_downsample (+ _workspace_bytes) (the voxel filter of clouds: additions only, the number stays), mmk_pose_loss_se3_fwd / _bwd, mmk_val_metric_se3 (the SE(3) pose terms: additions only, the number stays), mmk_icp_soft, mmk_icp_forward_soft, mmk_icp_backward_soft (+ _workspace_bytes), mmk_knn_search (+ _workspace_bytes) (soft correspondences of the dICP; the option travels in a struct of its own, so mmk_icp_params keeps its size: additions only, the number stays), mmk_icp_params.trim_steep appended and mmk_icp_params_bytes (the soft tanh trim gate of the dICP; the struct grows at its end and 0 keeps the hard gate: additions only, the number stays), mmk_mask_polar_scan, mmk_mask_polar_scan_bwd (+ _ws_bytes) (the Cartesian mask applied to the polar scan, fused; additions only), mmk_conv_first_dgrad (+ _ws_bytes), mmk_input_norm_bwd, mmk_unet_backward_input (gradient of the mask network with respect to its input image; additions only), mmk_icp_backward_points (+ _workspace_bytes), mmk_sample_weights_bwd_pc (gradients with respect to the point clouds), mmk_cfar_mask_bwd, mmk_extract_peaks_bwd (+ _workspace_bytes) (gradients of the radar front end with respect to the scan); 0.5.1: mmk_pose_loss_gt_*, mmk_val_metric, mmk_fft_threshold_*, mmk_bce_fft_threshold_*, mmk_channel_meanstd (the gt_eye=False pose terms, the fft-threshold mask loss and standardisation on the kernels); 0.5.0: mmk_unet_backward_buckets / mmk_unet_grad_bucket (per-bucket completion events for an overlapped gradient all-reduce); 0.4.2: arg-max codes of the poolings (mmk_conv_desc.pool_arg, mmk_maxpool2_fwd_arg / _bwd_arg, mmk_unet_desc.keep_full_res); 0.4.1: mmk_pose_loss_*, mmk_bce_mean_*; 0.4.0: mmk_icp_status / _accumulate / _solve_update; 0.3.1: mmk_host_read_rows_batch; 0.3.0: no float atomics left (first / final layer gradients and the mask-gradient scatter take workspaces; mmk_conv3x3_wgrad + _unpack removed) */

#define MMK_OK 0
#define MMK_ERR_ARG (-1)
#define MMK_ERR_HIP (-2)
#define MMK_ERR_WORKSPACE (-3)

#define MMK_ICP_PT2PT 0
#define MMK_ICP_PT2PL 1

#define MMK_NN_BRUTE 0 /* exhaustive scan (north_star's brute-force kernel)                  */
#define MMK_NN_GRID 1  /* exact search through a uniform grid: same indices, fewer evaluations */

#define MMK_LOSS_NONE 0
#define MMK_LOSS_CAUCHY 1
#define MMK_LOSS_HUBER 2
#define MMK_LOSS_GEMAN_MCCLURE 3 /* rho = c c, c = 1 / (1 + r2 / k^2) */
#define MMK_LOSS_WELSCH 4        /* rho = exp(-(r2 / k^2))                              */

int mmk_version(void);
const char *mmk_last_error(void);

/* ------------------------------------------------------------------ dICP (external/dICP, absent upstream)
 * Replaces dICP.ICP.ICP(...).icp(source, target, T_init=, weight=, trim_dist=,
 * loss_fn=, dim=) as called at mm_masking/icp_weight_policy.py:281-287 (ctor
 * :54-55; target_pad_val use mm_masking/icp_weight_dataset.py:59-61,395).
 * Arithmetic: DESIGN.md §3 == oracle/dicp_ref.py.                                     */
typedef struct {
    int32_t B;          /* scan pairs                                            */
    int32_t N;          /* padded source points per pair (zero rows carry weight 0) */
    int32_t M;          /* padded target points per pair (target_pad_val rows)   */
    int32_t tgt_cols;   /* 3 (xyz) or 6 (xyz|normal): icp_weight_dataset.py:397-398 */
    int32_t dim;        /* 2 or 3 (reference passes dim=2)                        */
    int32_t icp_type;   /* MMK_ICP_PT2PT | MMK_ICP_PT2PL (ctor icp_type)          */
    int32_t loss;       /* MMK_LOSS_* from loss_fn["name"]: none | cauchy | huber |
                           geman_mcclure | welsch                                 */
    float loss_k;       /* loss_fn["metric"]: the robust scale k, > 0 under every
                           code but MMK_LOSS_NONE                                 */
    float trim_dist;    /* trim_dist (5.0 at icp_weight_policy.py:279)            */
    float tolerance;    /* ctor tolerance: a pair freezes once ||delta|| < tol    */
    int32_t max_iter;   /* ctor max_iterations (K)                                */
    int32_t save_state; /* 1: keep per-iteration correspondences for backward     */
    int32_t check_every;/* >0: every that many iterations read the active flags
                           back (synchronises `stream`) and stop when all pairs
                           froze; 0: run max_iter iterations, never synchronise   */
    int32_t nn_method;  /* MMK_NN_BRUTE | MMK_NN_GRID: both return identical indices     */
    float trim_steep;   /* 0: hard trim gate keep = d2 < trim_dist^2;
                           > 0: soft gate keep = 0.5 - 0.5 tanh(trim_steep (d - trim_dist)),
                           differentiated in both backward entries (I3', I7'); negative
                           or non-finite: MMK_ERR_ARG ("trim_steep"), workspace size 0  */
} mmk_icp_params;

/* sizeof(mmk_icp_params) of the library, for a binding to check its mirror of the struct against (the struct grows at its
 * end: trim_steep was appended; a caller built against the shorter struct must not be mixed with this library).          */
size_t mmk_icp_params_bytes(void);

size_t mmk_icp_workspace_bytes(const mmk_icp_params *p);

/* State arrays (device): idx_hist int32 (K,B,N) if save_state else (B,N);
 * T_hist fp32 (K+1,B,16): poses before iteration k, T_hist[K] = result;
 * delta_hist fp64 (K,B,6); A_hist fp64 (K,B,36) row-major p x p in the leading
 * block; active_hist int32 (K+1,B): 1 while the pair still iterates.
 * weight may be NULL (all ones).  iters_run (host int*, may be NULL).               */
int mmk_icp_forward(const mmk_icp_params *p, const float *source /*B,N,3*/,
                    const float *target /*B,M,tgt_cols*/, const float *weight /*B,N*/,
                    const float *T_init /*B,16*/, float *T_out /*B,16*/,
                    int32_t *idx_hist, float *T_hist, double *delta_hist, double *A_hist,
                    int32_t *active_hist, void *workspace, size_t workspace_bytes,
                    int *iters_run, void *stream);

/* Reverse sweep over the saved state: grad_weight (B,N) = dL/dweight,
 * grad_T_init (B,16, may be NULL) = dL/dT_init, given grad_T (B,16) = dL/dT_out.
 * Replaces autograd through the unrolled dICP iterations
 * (train_icp_weights.py:51 loss.backward()).                                           */
int mmk_icp_backward(const mmk_icp_params *p, const float *source, const float *target,
                     const float *weight, const int32_t *idx_hist, const float *T_hist,
                     const double *delta_hist, const double *A_hist,
                     const int32_t *active_hist, const float *grad_T /*B,16*/,
                     float *grad_weight /*B,N*/, float *grad_T_init /*B,16 or NULL*/,
                     void *workspace, size_t workspace_bytes, void *stream);

/* The same sweep, also differentiated in the clouds: grad_source (B,N,3) = dL/dsource, grad_target (B,M,tgt_cols) =
 * dL/dtarget, each optional (both NULL: bit-identical to mmk_icp_backward).  As in autograd through the unrolled
 * iterations, the correspondences, the hard trim gate, the freeze decisions and the non-positive-definite fallback are
 * constants; the soft gate (trim_steep > 0) is differentiated in the points (both entries: it moves dL/dT_init through the
 * poses, and dL/dsource, dL/dtarget xyz directly), while trim_dist and trim_steep themselves get no gradient here (mmk_icp_backward_hp gives it).  Entries outside the arithmetic are exactly 0: source z for dim 2; target columns dim..2 and the normals for
 * pt2pt (normal columns >= 3 + dim for pt2pl); targets that were never a correspondent.  The target gradient is a scatter
 * of up to K*N rows per target, summed as 64-bit fixed point (no float atomics, bit-reproducible; resolution max|row
 * entry| * 2^(ceil(log2(K*N)) - 62)); a non-finite entry makes that pair's target gradient NaN.  workspace:
 * mmk_icp_backward_points_workspace_bytes(p, grad_target != NULL) bytes.  Argument errors return MMK_ERR_ARG.         */
size_t mmk_icp_backward_points_workspace_bytes(const mmk_icp_params *p, int32_t with_target);
int mmk_icp_backward_points(const mmk_icp_params *p, const float *source, const float *target,
                            const float *weight, const int32_t *idx_hist, const float *T_hist,
                            const double *delta_hist, const double *A_hist,
                            const int32_t *active_hist, const float *grad_T /*B,16*/,
                            float *grad_weight /*B,N*/, float *grad_T_init /*B,16 or NULL*/,
                            float *grad_source /*B,N,3 or NULL*/, float *grad_target /*B,M,tgt_cols or NULL*/,
                            void *workspace, size_t workspace_bytes, void *stream);

/* Status of the last mmk_icp_forward call that used `workspace`: the MMK_ICP_STATUS_* bits its kernels raised (0 = clean).
 * Asynchronous like everything else: enqueues a 4-byte copy on `stream` into status_out (a device pointer or pinned host
 * memory); the value is valid once the stream has passed it.  MMK_ICP_STATUS_UNARMED_KEY: a source row reached the
 * accumulation stage with a nearest-neighbour key no search kernel wrote (or an index outside the target) -- an internal
 * error, never the result of the caller's data; the row was clamped to stay in bounds and the poses of that call are
 * not to be trusted.                                                                                                     */
#define MMK_ICP_STATUS_UNARMED_KEY 1
/* MMK_ICP_STATUS_BAD_HYPER (mmk_icp_forward_hp): a value of `hyper` the call used was non-finite or out of range -- k > 0
 * under Cauchy / Huber, trim_dist >= 0, the steepness > 0 in soft mode; values the call does not use are not looked at.
 * The caller's data, not an internal error: the arithmetic ran on (floats only, nothing leaves its bounds) and the poses
 * are whatever it gave.                                                                                                   */
#define MMK_ICP_STATUS_BAD_HYPER 2
int mmk_icp_status(const mmk_icp_params *p, const void *workspace, size_t workspace_bytes,
                   int32_t *status_out, void *stream);

/* mmk_icp_forward with the robust scale k, the trim distance and the gate's steepness read ON THE DEVICE (DESIGN.md §3
 * I3''): hyper fp32 (1,3) (per_pair = 0, shared by the batch) or (B,3) (per_pair = 1), columns (k, trim_dist, trim_steep);
 * loss_k and trim_dist of `p` are then ignored, and p->trim_steep only selects the gate (0 hard: column 2 is never read;
 * > 0 soft: the steepness is column 2).  k*k and trim_dist*trim_dist are single fp32 products, so a call whose array holds
 * the values of a scalar call is bit-identical to it.  Nothing is read back: values out of range raise
 * MMK_ICP_STATUS_BAD_HYPER in the status word (mmk_icp_status).  hyper == NULL: mmk_icp_forward exactly.  Workspace:
 * mmk_icp_workspace_bytes(p).  per_pair other than 0 / 1: MMK_ERR_ARG.                                                    */
int mmk_icp_forward_hp(const mmk_icp_params *p, const float *source /*B,N,3*/,
                       const float *target /*B,M,tgt_cols*/, const float *weight /*B,N*/,
                       const float *T_init /*B,16*/, float *T_out /*B,16*/,
                       int32_t *idx_hist, float *T_hist, double *delta_hist, double *A_hist,
                       int32_t *active_hist, const float *hyper /*1|B,3*/, int32_t per_pair,
                       void *workspace, size_t workspace_bytes, int *iters_run, void *stream);

/* The reverse sweep of a mmk_icp_forward_hp call: mmk_icp_backward_points' arguments (grad_source and grad_target each
 * optional, so the entry serves both backward shapes) plus the forward's `hyper` / per_pair and grad_hyper (B,3 -- one
 * row per pair also when hyper is shared: the caller adds the rows -- or NULL) = dL/d(k, trim_dist, trim_steep), DESIGN.md
 * §3 I7'': per point and active iteration in fp32, summed per pair in fp64 by block partials in a fixed order (no float
 * atomics: bit-reproducible).  Exactly 0: trim_dist and trim_steep under the hard gate, k without a robust loss, and
 * whatever a pair's frozen iterations would add.  hyper == NULL (grad_hyper must be NULL too): mmk_icp_backward_points
 * exactly.  workspace: mmk_icp_backward_hp_workspace_bytes(p, grad_target != NULL, hyper != NULL) bytes -- the older
 * entries' sizes are unchanged.  Argument errors return MMK_ERR_ARG.                                                      */
size_t mmk_icp_backward_hp_workspace_bytes(const mmk_icp_params *p, int32_t with_target, int32_t with_hyper);
int mmk_icp_backward_hp(const mmk_icp_params *p, const float *source, const float *target,
                        const float *weight, const int32_t *idx_hist, const float *T_hist,
                        const double *delta_hist, const double *A_hist,
                        const int32_t *active_hist, const float *grad_T /*B,16*/,
                        float *grad_weight /*B,N*/, float *grad_T_init /*B,16 or NULL*/,
                        float *grad_source /*B,N,3 or NULL*/, float *grad_target /*B,M,tgt_cols or NULL*/,
                        const float *hyper /*1|B,3*/, int32_t per_pair, float *grad_hyper /*B,3 or NULL*/,
                        void *workspace, size_t workspace_bytes, void *stream);

/* Soft correspondences (DESIGN.md §3 I2', I3''', I7'''): every source point reads a VIRTUAL target row, the soft-min over
 * its k nearest target rows, a_j = softmax_j(-(d_j - d_0) / temp), row = sum_j a_j row_j (xyz and, for pt2pl, the normal,
 * which is not renormalised), and the backward differentiates the weights a_j in the points.  The option travels in a
 * struct of its own (mmk_icp_params keeps its size, MMK_VERSION its number: additions only).  k in 2..8, M >= k, temp
 * finite and > 0 (a squared length, m^2); anything else: MMK_ERR_ARG, workspace size 0.  The search is always the exact
 * k-NN through the grid: p->nn_method is ignored.  Slot 0 of the k neighbours is the correspondent the hard searches return.
 * mmk_icp_forward_soft: mmk_icp_forward's arguments; idx_hist is int32 (K,B,N,k) if save_state else (B,N,k), neighbours in key
 * order.  Workspace: mmk_icp_soft_workspace_bytes(p, soft); mmk_icp_status reads its status word as usual.
 * mmk_icp_backward_soft: mmk_icp_backward_points' arguments (grad_source and grad_target each optional: the entry serves
 * both backward shapes).  Which k rows are the neighbours is a constant, like the freezes and the delta = 0 fallback;
 * temp gets no gradient here (the _soft_t entries below give it one).  The target gradient is the same fixed-point scatter with K*N*k rows per pair (resolution max|row
 * entry| * 2^(ceil(log2(K*N*k)) - 62)).  Workspace: mmk_icp_backward_soft_workspace_bytes(p, soft, grad_target != NULL);
 * a short one is MMK_ERR_ARG.  Device-resident hyper-parameters (the _hp entries) are not combined with this mode.        */
typedef struct {
    int32_t k;          /* neighbours per point, 2..8                              */
    float temp;         /* tau > 0, m^2: e_j = expf(-(d_j - d_0) / tau)            */
} mmk_icp_soft;
size_t mmk_icp_soft_workspace_bytes(const mmk_icp_params *p, const mmk_icp_soft *soft);
int mmk_icp_forward_soft(const mmk_icp_params *p, const float *source /*B,N,3*/,
                         const float *target /*B,M,tgt_cols*/, const float *weight /*B,N*/,
                         const float *T_init /*B,16*/, float *T_out /*B,16*/,
                         int32_t *idx_hist, float *T_hist, double *delta_hist, double *A_hist,
                         int32_t *active_hist, const mmk_icp_soft *soft,
                         void *workspace, size_t workspace_bytes, int *iters_run, void *stream);
size_t mmk_icp_backward_soft_workspace_bytes(const mmk_icp_params *p, const mmk_icp_soft *soft, int32_t with_target);
int mmk_icp_backward_soft(const mmk_icp_params *p, const float *source, const float *target,
                          const float *weight, const int32_t *idx_hist /*K,B,N,k*/, const float *T_hist,
                          const double *delta_hist, const double *A_hist,
                          const int32_t *active_hist, const float *grad_T /*B,16*/,
                          float *grad_weight /*B,N*/, float *grad_T_init /*B,16 or NULL*/,
                          float *grad_source /*B,N,3 or NULL*/, float *grad_target /*B,M,tgt_cols or NULL*/,
                          const mmk_icp_soft *soft, void *workspace, size_t workspace_bytes, void *stream);

/* The soft entries with the temperature read ON THE DEVICE (DESIGN.md §3 I3'''', I7''''): temp fp32 (1) (per_pair = 0, shared
 * by the batch) or (B) (per_pair = 1).  soft->k is used; soft->temp must still pass the struct's validation (pass 1.0) and is
 * not read.  The expression is that of I3''', e_j = expf(-(d_j - d_0) / tau_b), so a call whose array holds the fp32 value of a
 * mmk_icp_forward_soft call is bit-identical to it.  Nothing is read back: on the first iteration one thread per pair
 * validates tau_b, and a non-finite or <= 0 value raises MMK_ICP_STATUS_BAD_HYPER in the status word (mmk_icp_status); the
 * arithmetic runs on (indices come from the k-NN, never from tau: nothing leaves its bounds).
 * mmk_icp_forward_soft_t: temp == NULL is mmk_icp_forward_soft exactly.  Workspace: mmk_icp_soft_workspace_bytes(p, soft).
 * mmk_icp_backward_soft_t: grad_temp (B -- one row per pair also when temp is shared: the caller adds the rows -- or NULL)
 * = dL/dtau.  Per point and active iteration in fp32: u = sum_j zbar_j (d_j - d_0) in slot order (slot 0 adds exactly 0),
 * tau-bar_i = u / (tau_b * tau_b); summed per pair in fp64 by block partials in a fixed order, as grad_hyper is (no float
 * atomics: bit-reproducible; a pair's frozen iterations add exactly 0).  temp == NULL with grad_temp == NULL is
 * mmk_icp_backward_soft exactly.  Workspace: mmk_icp_backward_soft_t_workspace_bytes(p, soft, grad_target != NULL,
 * grad_temp != NULL) -- the older entries' sizes are unchanged.  per_pair other than 0 / 1, grad_temp without temp and a
 * short workspace: MMK_ERR_ARG.                                                                                           */
int mmk_icp_forward_soft_t(const mmk_icp_params *p, const float *source /*B,N,3*/,
                           const float *target /*B,M,tgt_cols*/, const float *weight /*B,N*/,
                           const float *T_init /*B,16*/, float *T_out /*B,16*/,
                           int32_t *idx_hist, float *T_hist, double *delta_hist, double *A_hist,
                           int32_t *active_hist, const mmk_icp_soft *soft, const float *temp /*1|B*/, int32_t per_pair,
                           void *workspace, size_t workspace_bytes, int *iters_run, void *stream);
size_t mmk_icp_backward_soft_t_workspace_bytes(const mmk_icp_params *p, const mmk_icp_soft *soft, int32_t with_target,
                                               int32_t with_temp);
int mmk_icp_backward_soft_t(const mmk_icp_params *p, const float *source, const float *target,
                            const float *weight, const int32_t *idx_hist /*K,B,N,k*/, const float *T_hist,
                            const double *delta_hist, const double *A_hist,
                            const int32_t *active_hist, const float *grad_T /*B,16*/,
                            float *grad_weight /*B,N*/, float *grad_T_init /*B,16 or NULL*/,
                            float *grad_source /*B,N,3 or NULL*/, float *grad_target /*B,M,tgt_cols or NULL*/,
                            const mmk_icp_soft *soft, const float *temp /*1|B*/, int32_t per_pair,
                            float *grad_temp /*B or NULL*/, void *workspace, size_t workspace_bytes, void *stream);

/* Stage I2' on its own: the k (2..8, M >= k) nearest rows of `target` (B,M,tgt_cols, the first dim columns) to the source
 * points under T (B,16), exact, through the per-call grid.  idx int32 (B,N,k) and d2 fp32 (B,N,k) in key order: ascending
 * d2 (I2's expression), ties to the lowest index.  Workspace: mmk_knn_search_workspace_bytes(B, N, M, k) bytes (0 for
 * arguments the search refuses).                                                                                         */
size_t mmk_knn_search_workspace_bytes(int32_t B, int32_t N, int32_t M, int32_t k);
int mmk_knn_search(const float *source /*B,N,3*/, const float *target /*B,M,tgt_cols*/, const float *T /*B,16*/,
                   int32_t B, int32_t N, int32_t M, int32_t tgt_cols, int32_t dim, int32_t k,
                   int32_t *idx /*B,N,k*/, float *d2 /*B,N,k*/, void *workspace, size_t workspace_bytes, void *stream);

/* The stages of one iteration on their own (SURVEY.md 8b names them; mmk_icp_forward is these in a loop behind the NN search).
 * mmk_icp_accumulate (stages I3 + I4): consumes nearest-neighbour keys ((bits of d2) << 32 | index, (B,N) uint64 -- the
 * layout the search kernels produce), writes the correspondences idx_out (B,N) and per-workgroup partial sums of the normal
 * equations, `partials` fp64 with mmk_icp_partials_count(p) elements ((B, ceil(N/256), 9 | 27): upper triangle of A row-major,
 * then b); ORs MMK_ICP_STATUS_* bits into the device word *status (caller zeroes it).  T (B,16) = the pose the keys were
 * found under.  mmk_icp_solve_update (stages I5 + I6): ordered sum of the partials, Cholesky solve, T_out = Exp(delta) T_in,
 * delta_out (B,6), A_out (B,36), active_out[b] = 0 once ||delta|| < tolerance (active_in[b] = 0: pair frozen, pose copied). */
size_t mmk_icp_partials_count(const mmk_icp_params *p);
int mmk_icp_accumulate(const mmk_icp_params *p, const float *source, const float *target,
                       const float *weight /*B,N or NULL*/, const float *T /*B,16*/,
                       const uint64_t *nn_keys /*B,N*/, int32_t *idx_out /*B,N*/, double *partials,
                       int32_t *status /*device, 1*/, void *stream);
int mmk_icp_solve_update(const mmk_icp_params *p, const double *partials, const float *T_in /*B,16*/,
                         float *T_out /*B,16*/, double *delta_out /*B,6*/, double *A_out /*B,36*/,
                         const int32_t *active_in /*B*/, int32_t *active_out /*B*/, void *stream);

/* Stand-alone brute-force nearest neighbour (stage I2), the roofline kernel.
 * target_planar: (B,dim,Mpad) produced by mmk_pack_target, Mpad = mmk_nn_padded_m(M).
 * T (B,16) is applied to the source first (stage I1).  idx int32 (B,N), d2 fp32 (B,N). */
int32_t mmk_nn_padded_m(int32_t M);
int mmk_pack_target(const float *target /*B,M,tgt_cols*/, int32_t B, int32_t M,
                    int32_t tgt_cols, int32_t dim, float *target_planar, void *stream);
size_t mmk_nn_workspace_bytes(int32_t B, int32_t N, int32_t M, int32_t dim);
int mmk_nn_search(const float *source /*B,N,3*/, const float *target_planar,
                  const float *T /*B,16*/, int32_t B, int32_t N, int32_t M, int32_t dim,
                  int32_t *idx, float *d2, void *workspace, size_t workspace_bytes,
                  void *stream);

/* Target normals: exact k-nearest-neighbour PCA of a cloud against itself.  Produces the normals
 * columns of the map tensor (mm_masking/icp_weight_dataset.py:395-398: xyz | normal), which upstream come out of vtr3
 * pose graphs.  points (B,M,cols), cols >= dim; the search uses the first dim coordinates with the ICP's own distance and
 * key (ascending d2, ties to the lowest index; a row is its own first neighbour).  k in 3..32.  max_radius > 0 drops
 * rows with d2 > max_radius^2; pad_val > 0 makes every row with a |coordinate| >= pad_val a padding row: never a
 * neighbour, all its outputs 0 (nbr_idx -1).  viewpoint (B,3) or NULL = the origin: the normal is flipped to face it.
 * normals (B,M,3) unit length (nz = 0 for dim 2), or 0 with fewer than 3 neighbours kept; curvature (B,M) = lambda_min /
 * sum(lambda); count (B,M) = neighbours kept; nbr_idx (B,M,k) in key order, unused slots -1.  The last three are
 * optional.  Every value depends on the pair's own rows alone: bit-reproducible, no float atomics.  Asynchronous on
 * `stream`, no allocation; workspace: mmk_knn_normals_workspace_bytes(B, M) bytes.                                    */
size_t mmk_knn_normals_workspace_bytes(int32_t B, int32_t M);
int mmk_knn_normals(const float *points /*B,M,cols*/, int32_t B, int32_t M, int32_t cols, int32_t dim /*2|3*/,
                    int32_t k /*3..32*/, float max_radius /*<= 0: none*/, float pad_val /*<= 0: no padding rows*/,
                    const float *viewpoint /*B,3 or NULL = origin*/,
                    float *normals /*B,M,3*/, float *curvature /*B,M or NULL*/, int32_t *count /*B,M or NULL*/,
                    int32_t *nbr_idx /*B,M,k or NULL*/, void *workspace, size_t workspace_bytes, void *stream);

/* Voxel-grid downsampling of a cloud (this build's own, nothing upstream corresponds: upstream the maps
 * arrive voxel-filtered from vtr3).  points (B,M,cols), dim <= cols <= 8.  A row is valid when all its cols values are
 * finite and |x_c| < pad_val for c < dim; every other row is padding (voxel_of -1).  Cell of a valid row: i_c = (int)
 * floorf(x_c * inv), c < dim, inv = (float)(1.0 / (double)voxel) formed once on the host.  One output row per occupied
 * cell, ordered by the lowest member index (first appearance).  out_count[b] = occupied cells (it may exceed max_out: the
 * first max_out are kept); voxel_of[b,i] = rank of row i's cell in that order (also when >= max_out); out_n = members,
 * out_first = lowest member index; rows from min(count, max_out) on are padding: every column pad_val, out_n 0, out_first
 * -1.  MMK_VOXEL_CENTROID: every column the mean of the members, summed as 64-bit fixed point (one power-of-two scale per
 * pair, M max|value| scale < 2^62) and closed by (float)((double)sum / scale / n): independent of the arrival order;
 * normals = 1 (cols >= 6): columns 3..5 are the mean normal divided by its fp64 length, rounded once, exactly 0 when the
 * length is 0.  MMK_VOXEL_FIRST: every column a bit copy of the lowest-index member.  voxel and pad_val finite and > 0,
 * pad_val * inv <= 2^20, dim 2|3, normals 0|1, 1 <= max_out, 1 <= M <= 2^28, 1 <= B <= 65535, points / out / out_count not
 * NULL, workspace of mmk_voxel_downsample_workspace_bytes(B, M, cols, max_out) bytes (0 for refused sizes): anything else
 * is MMK_ERR_ARG before any launch.  Asynchronous on `stream`, no allocation, nothing read back; every value depends on
 * the pair's own rows alone; no float atomics.                                                                          */
#define MMK_VOXEL_CENTROID 0
#define MMK_VOXEL_FIRST 1
size_t mmk_voxel_downsample_workspace_bytes(int32_t B, int32_t M, int32_t cols, int32_t max_out);
int mmk_voxel_downsample(const float *points /*B,M,cols*/, int32_t B, int32_t M, int32_t cols, int32_t dim /*2|3*/,
                         float voxel, float pad_val, int32_t mode, int32_t normals /*0|1*/, int32_t max_out,
                         float *out /*B,max_out,cols*/, int32_t *out_count /*B*/,
                         int32_t *out_n /*B,max_out or NULL*/, int32_t *out_first /*B,max_out or NULL*/,
                         int32_t *voxel_of /*B,M or NULL*/, void *workspace, size_t workspace_bytes, void *stream);

/* Measurement hook (bench.py): while enabled, every nn_search launch made by this
 * process (inside mmk_icp_forward or mmk_nn_search) is bracketed by HIP events on its
 * launch stream.  _end() waits for the recorded events and returns the per-launch
 * durations in milliseconds (ms_out is a HOST array; n_out = launches seen).  Process-wide,
 * not thread-safe: measurement only.  Nothing upstream corresponds to it (the reference
 * times whole epochs, train_icp_weights.py:518-523).                                    */
int mmk_nn_profile_begin(int32_t capacity);
int mmk_nn_profile_end(float *ms_out /*host*/, int32_t max_out, int32_t *n_out /*host*/);

/* ------------------------------------------------------------------ loss terms of train_icp_weights.py:179-253
 * One launch each (plus an ordered final sum) instead of ~45 PyTorch launches per step; deterministic (no float atomics).
 * mmk_pose_loss_fwd: out2[0] = mean_b |T[b,1,0]|  (loss_rot, :199), out2[1] = mean_b ||(T[b,0,3], T[b,1,3])||  (loss_trans, :200)
 *   of xi = T_pred - I (the gt_eye form, :193).  _bwd: grad_T (B,16) = g_rot * d rot / dT + g_trans * d trans / dT, with g_rot /
 *   g_trans DEVICE scalars (NULL = 0): sign(.) / B and (x, y) / norm / B, zero where the norm is zero (as torch.norm's backward).
 * mmk_bce_mean_fwd: out[0] = torch.nn.BCELoss()(x, target) over n elements (logs clamped at -100), ws = mmk_bce_ws_bytes()
 *   bytes of device workspace.  _bwd: grad_x = grad_out[0] * (x - t) / max((1 - x) x, 1e-12) / n, grad_out a device scalar.    */
int mmk_pose_loss_fwd(const float *T_pred /*B,16*/, int32_t B, float *out2, void *stream);
int mmk_pose_loss_bwd(const float *T_pred, int32_t B, const float *g_rot, const float *g_trans,
                      float *grad_T /*B,16*/, void *stream);
size_t mmk_bce_ws_bytes(void);
int mmk_bce_mean_fwd(const float *x, const float *target, int64_t n, void *ws, size_t ws_bytes,
                     float *out, void *stream);
int mmk_bce_mean_bwd(const float *x, const float *target, int64_t n, const float *grad_out,
                     float *grad_x, void *stream);

/* Pose terms against a ground-truth pose (gt_eye=False, :192-200): xi = T_pred T_gt^-1 - I, evaluated as (T_pred - T_gt) T_gt^-1
 * in fp64 with a general 4x4 inverse per pair (Gauss-Jordan, partial pivoting; poses read from data are not exactly orthonormal);
 * a singular T_gt gives inf / NaN.  mmk_pose_loss_gt_fwd: out2 = (mean_b |xi[1,0]|, mean_b ||(xi[0,3], xi[1,3])||).
 * _bwd: grad_T (B,16) = G T_gt^-T, G nonzero only at [1,0] (sign(xi[1,0]) g_rot / B) and [0,3], [1,3] ((x, y) / norm g_trans / B,
 * zero where the norm is zero); g_rot / g_trans DEVICE scalars (NULL = 0).  T_gt gets no gradient.
 * mmk_val_metric: out3 = (mean_b ||(xi[1,0], xi[0,3], xi[1,3])||, mean_b |xi[1,0]|, mean_b ||(xi[0,3], xi[1,3])||), the 3-vector
 *   of eval_validation_loss (:255-273); T_gt NULL = the identity (xi = T_pred - I).
 * FFT-threshold mask term (:204-207): target = fft > 3 * mean_{H,W}(fft) per image, the mean an ordered fp64 reduction rounded
 * to fp32 and the threshold the fp32 product 3.0f * mean.  fft is (B, hw), hw >= 4; ws = mmk_fft_threshold_ws_bytes(B) bytes.
 * mmk_fft_threshold_mask writes the 0/1 target (generate_baseline, :312-316).  mmk_bce_fft_threshold_fwd / _bwd: the BCE of
 *   mmk_bce_mean_* against that target computed on the fly (no target is written), the same bits as mmk_bce_mean_* on the mask
 *   mmk_fft_threshold_mask writes; _fwd also writes the B thresholds to thr_out, which _bwd reads.  16-byte aligned buffers. */
int mmk_pose_loss_gt_fwd(const float *T_pred /*B,16*/, const float *T_gt /*B,16*/, int32_t B, float *out2, void *stream);
int mmk_pose_loss_gt_bwd(const float *T_pred, const float *T_gt, int32_t B, const float *g_rot, const float *g_trans,
                         float *grad_T /*B,16*/, void *stream);
int mmk_val_metric(const float *T_pred /*B,16*/, const float *T_gt /*B,16 or NULL*/, int32_t B, float *out3, void *stream);
/* SE(3) pose terms (pose_loss="se3"; the planar terms above read xi[1,0], xi[0,3], xi[1,3] only).  xi = T_pred T_gt^-1 - I as
 * above: T_pred - I with T_gt NULL, (T_pred - T_gt) T_gt^-1 with the fp64 Gauss-Jordan inverse otherwise, so T_pred = T_gt gives
 * xi = 0 exactly.  Per pair, in fp64 from the fp32 inputs, in both forms:
 *   v = 1/2 (xi[2,1] - xi[1,2], xi[0,2] - xi[2,0], xi[1,0] - xi[0,1]),  s = ||v||,  c = 1 + 1/2 (xi[0,0] + xi[1,1] + xi[2,2]),
 *   theta = atan2(s, c) in [0, pi] (the geodesic rotation angle),  r = ||(xi[0,3], xi[1,3], xi[2,3])||.
 * mmk_pose_loss_se3_fwd: out2 = (mean_b theta_b, mean_b r_b).  mmk_val_metric_se3: out3 = (mean_b sqrt(theta_b^2 + r_b^2),
 *   mean_b theta_b, mean_b r_b).  Means as above: one wave, lane l sums pairs l, l + 64, ... in index order, a fixed shuffle tree
 *   in fp64, rounded once to fp32.
 * mmk_pose_loss_se3_bwd: grad_T (B,16) = G with T_gt NULL, G T_gt^-T otherwise, G = d(g_rot mean theta + g_trans mean r) / dxi;
 *   g_rot / g_trans DEVICE scalars (NULL = 0).  With d = s^2 + c^2: d theta / dv = c v / (s d) (0 at s = 0, the subgradient of
 *   torch.norm's backward) spread with +-1/2 onto the six off-diagonal entries, d theta / dc = -s / d (0 at d = 0) spread with 1/2
 *   onto the diagonal, d r / dxi[i,3] = xi[i,3] / r (0 at r = 0).  Row 3 of G is zero; T_gt gets no gradient.
 * One launch each, deterministic, no float atomics.  B < 1, a NULL T_pred or a NULL output: MMK_ERR_ARG.                        */
int mmk_pose_loss_se3_fwd(const float *T_pred /*B,16*/, const float *T_gt /*B,16 or NULL = identity*/, int32_t B, float *out2, void *stream);
int mmk_pose_loss_se3_bwd(const float *T_pred, const float *T_gt /*or NULL*/, int32_t B, const float *g_rot, const float *g_trans,
                          float *grad_T /*B,16*/, void *stream);
int mmk_val_metric_se3(const float *T_pred, const float *T_gt /*or NULL*/, int32_t B, float *out3, void *stream);
size_t mmk_fft_threshold_ws_bytes(int32_t B);
int mmk_fft_threshold_mask(const float *fft, int32_t B, int64_t hw, void *ws, size_t ws_bytes, float *mask_out,
                           void *stream);
int mmk_bce_fft_threshold_fwd(const float *x, const float *fft, int32_t B, int64_t hw, void *ws, size_t ws_bytes,
                              float *thr_out /*B*/, float *out, void *stream);
int mmk_bce_fft_threshold_bwd(const float *x, const float *fft, int32_t B, int64_t hw, const float *thr /*B*/,
                              const float *grad_out, float *grad_x, void *stream);

/* ------------------------------------------------------------------ radar_utils.py
 * mmk_cfar_mask        <- cfar_mask                      radar_utils.py:29-69
 * mmk_extract_peaks    <- extract_pc (+mean_peaks_parallel_fast, pol_2_cart)
 *                                                        radar_utils.py:71-106,167-195
 * mmk_extract_peaks_t  <- the same, keeping the third (time) column of its pair mean       radar_utils.py:97
 * mmk_deskew_points, mmk_deskew_points_bwd <- the motion compensation that produced the reference's filtered_pc
 *                        (icp_weight_dataset.py:331-332), as a constant-twist operator with its gradients
 * mmk_cfar_mask_bwd, mmk_extract_peaks_bwd <- what autograd does for the two above when
 *                        the scan / the mask requires grad (both default to diff=True upstream)
 * mmk_cfar_mask_p, mmk_cfar_mask_bwd_p <- the same with a_thresh / b_thresh as tensors   radar_utils.py:56
 * mmk_polar_to_cart    <- radar_polar_to_cartesian_diff  radar_utils.py:258-336
 * mmk_cart_to_polar    <- radar_cartesian_to_polar       radar_utils.py:338-372
 * mmk_polar_to_cart_bwd, mmk_cart_to_polar_bwd <- what autograd does for the two above when
 *                        the image requires grad (both are plain F.grid_sample calls upstream)
 * mmk_mask_polar_scan (+ _bwd) <- radar_cartesian_to_polar(mask.double(), ...).float() * fft_data, the masked scan of
 *                        icp_weight_policy.py:266, and what autograd does for it
 * mmk_sample_weights_* <- extract_weights (fwd + autograd bwd) radar_utils.py:108-128
 * mmk_sample_weights_polar_* <- extract_weights for a POLAR mask (absent upstream: SURVEY 8f.3's "polar-aware
 *                        extract_weights"), sampled with radar_polar_to_cartesian_diff's arithmetic   radar_utils.py:276-323
 * mmk_bev_raster       <- extract_bev_from_pts           radar_utils.py:142-165      */

/* GO-CFAR on (B,A,R) polar power.  w2/guard/mincol/maxcol as derived at
 * radar_utils.py:34-39 by the caller.  diff: 0 hard (x>thres), 1 soft (tanh+hardshrink). */
int mmk_cfar_mask(const float *raw, int32_t B, int32_t A, int32_t R, int32_t w2,
                  int32_t guard, int32_t mincol, int32_t maxcol, float a_thresh,
                  float b_thresh, int32_t diff, float steep_fact, float *mask,
                  void *stream);

/* grad_raw (B,A,R) = dL/draw of mmk_cfar_mask(diff=1) <- autograd through radar_utils.py:29-69: tanh (:62) and the direct
 * term, hardshrink's gate (:63, a constant: |0.5 t + 0.5| > 0.99 as the forward decides it), and through the threshold
 * (:57-58) torch.maximum's winner (:56; an exact tie of the two fp32 window sums gives each window half) into every cell
 * of the winning window (:47-54, with the slice's clamp at R).  Outside [mincol, maxcol) the threshold is the constant 1000.
 * The window sums are recomputed with the forward's arithmetic, so gate, winner and ties are the forward's bit for bit.
 * A gather per cell from ordered fp64 prefix sums: no atomics, bit-reproducible; grad_raw is written whole.
 * (diff=0 has no gradient: torch.where of constants, :65.) */
int mmk_cfar_mask_bwd(const float *raw, const float *grad_mask /*B,A,R*/, int32_t B, int32_t A, int32_t R, int32_t w2,
                      int32_t guard, int32_t mincol, int32_t maxcol, float a_thresh, float b_thresh, float steep_fact,
                      float *grad_raw /*B,A,R*/, void *stream);

/* mmk_cfar_mask with the two thresholds of radar_utils.py:56 (thres = a_thresh * stat + b_thresh, plain tensor arithmetic
 * upstream) read from device memory: one float each for the batch (per_scan = 0) or B floats each, one per scan
 * (per_scan = 1).  For equal values the mask is mmk_cfar_mask's bit for bit, for both values of diff; no host
 * synchronisation. */
int mmk_cfar_mask_p(const float *raw, int32_t B, int32_t A, int32_t R, int32_t w2, int32_t guard, int32_t mincol,
                    int32_t maxcol, const float *a_thresh, const float *b_thresh, int32_t per_scan, int32_t diff,
                    float steep_fact, float *mask, void *stream);

/* mmk_cfar_mask_bwd with device thresholds, plus what autograd gives a_thresh and b_thresh when they are tensors that
 * require grad (radar_utils.py:56: dthres/da = stat, dthres/db = 1, and dL/dthres_c = -k_c on the cells hardshrink keeps
 * inside [mincol, maxcol); outside, the threshold is the constant 1000):
 *   grad_a = - sum of k_c stat_c,   grad_b = - sum of k_c      over the batch (per_scan = 0, 1 float each) or over each
 * scan (per_scan = 1, B floats each).  k_c, stat_c and the gate are those of the same launch's grad_raw, so grad_raw is
 * mmk_cfar_mask_bwd's bit for bit.  The sums are fp64 in a fixed order (per thread, per row, then over the rows: no atomics),
 * bit-reproducible, and a scan's pair does not depend on the other scans of the batch.  grad_raw may be NULL (only the
 * thresholds require grad): the kernel then stops after the pass that forms k.  workspace: mmk_cfar_mask_bwd_p_ws_bytes(B, A)
 * bytes (one pair of doubles per row). */
size_t mmk_cfar_mask_bwd_p_ws_bytes(int32_t B, int32_t A);
int mmk_cfar_mask_bwd_p(const float *raw, const float *grad_mask /*B,A,R*/, int32_t B, int32_t A, int32_t R, int32_t w2,
                        int32_t guard, int32_t mincol, int32_t maxcol, const float *a_thresh, const float *b_thresh,
                        int32_t per_scan, float steep_fact, float *grad_raw /*B,A,R; may be NULL*/, float *grad_a,
                        float *grad_b /*1 or B*/, void *workspace, size_t workspace_bytes, void *stream);

size_t mmk_extract_peaks_workspace_bytes(int32_t B, int32_t A, int32_t R, int32_t max_pts);
/* Blob-centre extraction.  out_pc (B,max_pts,3) zero padded in the reference's
 * azimuth-major order; out_count int32 (B) = points the reference would return
 * (may exceed max_pts: then the cloud is truncated); T_ab (B,16) may be NULL.          */
int mmk_extract_peaks(const float *mask, int32_t B, int32_t A, int32_t R, float res,
                      const float *azimuths /*B,A*/, const float *times /*B,A*/,
                      const float *T_ab, int32_t diff, float steep_fact, int32_t max_pts,
                      float *out_pc, int32_t *out_count, void *workspace,
                      size_t workspace_bytes, void *stream);
/* mmk_extract_peaks plus the measurement time of every point: out_time (B,max_pts) holds
 * t_k = (times[b, row of marker 2k+1] + times[b, row of marker 2k]) / 2 (one fp32 add and an exact halving: the pair mean
 * of radar_utils.py:97 applied to the time column) for the rows that hold a point and 0 for the padding rows.  T_ab does not
 * enter the times.  times must not be NULL here.  out_pc and out_count are mmk_extract_peaks's, bit for bit; the workspace
 * is mmk_extract_peaks_workspace_bytes(B, A, R, max_pts). */
int mmk_extract_peaks_t(const float *mask, int32_t B, int32_t A, int32_t R, float res,
                        const float *azimuths /*B,A*/, const float *times /*B,A*/,
                        const float *T_ab, int32_t diff, float steep_fact, int32_t max_pts,
                        float *out_pc, int32_t *out_count, void *workspace,
                        size_t workspace_bytes, float *out_time /*B,max_pts*/, void *stream);
/* grad_mask (B,A,R) = dL/dmask of mmk_extract_peaks given grad_pc (B,max_pts,3) <- autograd through radar_utils.py:74
 * (res * j * mask), mean_peaks_parallel_fast (:167-185; diff=1: through both factors of each product, z = 1 - tanh;
 * diff=0: z is the bool (arr == 0), a constant, and the gradient flows through the arr factors), the pair mean (:95),
 * pol_2_cart (:187-195) and T_ab's rotation (:100).  The set of non-zero markers (nonzero, :88), their order and their
 * pairing are constants and are placed again exactly as the forward places them.  The unpaired last marker of an odd
 * count, points at or beyond max_pts and cells that feed no marker get exactly 0.  azimuths, times and T_ab are not
 * differentiated.  grad_mask is written whole (no memset needed), no atomics, bit-reproducible.
 * workspace: mmk_extract_peaks_bwd_workspace_bytes(B, A, R, max_pts) bytes. */
size_t mmk_extract_peaks_bwd_workspace_bytes(int32_t B, int32_t A, int32_t R, int32_t max_pts);
int mmk_extract_peaks_bwd(const float *mask, int32_t B, int32_t A, int32_t R, float res, const float *azimuths /*B,A*/,
                          const float *T_ab, int32_t diff, float steep_fact, int32_t max_pts,
                          const float *grad_pc /*B,max_pts,3*/, float *grad_mask /*B,A,R*/, void *workspace,
                          size_t workspace_bytes, void *stream);

/* Constant-twist motion compensation of a scan cloud (absent upstream, whose filtered_pc arrives
 * compensated).  twist (B,6) = (v; omega), the sensor's body-frame velocity in m/s and rad/s, translation first, constant
 * over the scan; t (B,N) the measurement time of every point in seconds relative to the scan's reference time.  Point i
 * moves to p' = Exp(t_i twist) p, evaluated per point in fp64 from the fp32 inputs with one rounding per output:
 *   w = t omega, u = t v, th2 = w.w, A = sin th / th, B = (1 - cos th) / th2, C = (th - sin th) / th^3 (Taylor series to
 *   th^6 for th2 < 1e-4), p' = p + A (w x p) + B w x (w x p) + u + B (w x u) + C w x (w x u).
 * A row of pc whose three coordinates are exactly 0 is padding: its output and both of its gradients are 0.  twist = 0 and
 * t_i = 0 return the input bits; a planar twist (vx, vy, 0, 0, 0, wz) keeps z = 0 exactly.
 * mmk_deskew_points_bwd: grad_pc (B,N,3) = R^T grad_out and grad_twist (B,6) = sum_i t_i (u_bar_i; w_bar_i), the
 * hand-derived reverse of the expression above; either may be NULL.  t gets no gradient.  grad_twist is summed in fp64
 * without atomics (thread -> wave -> block partial -> one wave per item in index order) and rounded once: two runs agree
 * in every bit.  The workspace (mmk_deskew_points_bwd_workspace_bytes(B, N) bytes) is read only when grad_twist is asked
 * for; with grad_twist NULL it may be NULL. */
int mmk_deskew_points(const float *pc /*B,N,3*/, const float *t /*B,N*/, const float *twist /*B,6*/,
                      int32_t B, int32_t N, float *out /*B,N,3*/, void *stream);
size_t mmk_deskew_points_bwd_workspace_bytes(int32_t B, int32_t N);
int mmk_deskew_points_bwd(const float *pc /*B,N,3*/, const float *t /*B,N*/, const float *twist /*B,6*/,
                          int32_t B, int32_t N, const float *grad_out /*B,N,3*/,
                          float *grad_pc /*B,N,3 or NULL*/, float *grad_twist /*B,6 or NULL*/,
                          void *workspace, size_t workspace_bytes, void *stream);

/* Polar (B,A,R) -> Cartesian (B,W,W) bilinear resample.  range_grid/angle_grid (W,W)
 * are form_cart_range_angle_grid's outputs (radar_utils.py:399-419), built by the host. */
int mmk_polar_to_cart(const float *polar, const float *azimuths /*B,A*/,
                      const float *range_grid, const float *angle_grid, int32_t B,
                      int32_t A, int32_t R, int32_t W, float radar_resolution,
                      int32_t interpolate_crossover, int32_t fix_wobble, float *cart,
                      void *stream);
/* Two images of one batch resampled with the same azimuths in one pass (FFT and CFAR image of a
 * scan, icp_weight_dataset.py:350-352): coordinates and tap weights are computed once. */
int mmk_polar_to_cart_pair(const float *polar, const float *polar2, const float *azimuths,
                           const float *range_grid, const float *angle_grid, int32_t B, int32_t A,
                           int32_t R, int32_t W, float radar_resolution, int32_t interpolate_crossover,
                           int32_t fix_wobble, float *cart, float *cart2, void *stream);

/* Cartesian (B,H,W) -> polar (B,A,R) bilinear resample in fp64 <- radar_cartesian_to_polar, radar_utils.py:338-372
 * (the reference casts its sampling grid to double at :370: fp64 images only).  sin_az / cos_az (B,A) and
 * range_coords (R) = linspace(0, (R-1) radar_resolution, R) are formed by the host with torch's CPU functions, as the
 * reference does; the output is bit-identical to the reference's. */
int mmk_cart_to_polar(const double *cart, const double *sin_az, const double *cos_az, const double *range_coords,
                      int32_t B, int32_t A, int32_t R, int32_t H, int32_t W, double cart_resolution, double *polar,
                      void *stream);

/* grad_polar (B,A,R) = dL/dpolar of mmk_polar_to_cart given grad_cart (B,W,W) <- autograd through the F.grid_sample at
 * radar_utils.py:334 and the wrap-row concatenation at :318.  The operator is linear in the image: the sampling grid
 * (:286-323: wobble search, the u < 0 -> 0 clamp, the + 1 row of interpolate_crossover, the normalisation) depends on the
 * azimuths and the pixel grid only, which are constants, and is recomputed with the forward's arithmetic bit for bit.
 * Tap (yk, xk) adds g * w_tap to cell (row(yk), xk); with the crossover rows, padded row 0 folds onto row A - 1 and padded
 * row A + 1 onto row 0; taps in the zero padding contribute nowhere.
 * The sums are formed in 64-bit fixed point with integer atomics (per item: scale = the power of two that keeps
 * 4 W^2 * max|g| below 2^62), so they do not depend on the order of arrival: no float atomics, bit-reproducible, a
 * resolution of max|g| * 2^(ceil(log2(4 W^2)) - 62) per tap.  grad_polar is written whole (cells no tap reaches get exactly
 * 0; a non-finite grad_cart makes its item NaN).  ws: mmk_polar_to_cart_bwd_ws_bytes(B, A, R, W) bytes. */
size_t mmk_polar_to_cart_bwd_ws_bytes(int32_t B, int32_t A, int32_t R, int32_t W);
int mmk_polar_to_cart_bwd(const float *grad_cart /*B,W,W*/, const float *azimuths /*B,A*/, const float *range_grid,
                          const float *angle_grid, int32_t B, int32_t A, int32_t R, int32_t W, float radar_resolution,
                          int32_t interpolate_crossover, int32_t fix_wobble, float *grad_polar /*B,A,R*/, void *ws,
                          size_t ws_bytes, void *stream);

/* grad_cart (B,H,W) = dL/dcart of mmk_cart_to_polar given grad_polar (B,A,R), fp64 <- autograd through the F.grid_sample
 * at radar_utils.py:370; the sampling grid (:342-363) is a constant.  sin_az, cos_az and range_coords are the forward's
 * host-formed arrays; radar_resolution is the spacing of range_coords (it bounds how many samples of one ray can reach one
 * pixel: ceil(2 sqrt 2 cart_resolution / radar_resolution) + 1).  The four in-image taps of every polar cell receive
 * g * {(1-wy)(1-wx), (1-wy) wx, wy (1-wx), wy wx}.  Same fixed-point form as mmk_polar_to_cart_bwd, with the count bound
 * A * (ceil(2 sqrt 2 cart_resolution / radar_resolution) + 1): a resolution of max|g| * 2^(cnt_bits - 62) per tap (2^-49 of
 * max|g| at 400 x 3360 -> 640 x 640).  The sums are formed in grad_cart itself, which is written whole (pixels no ray touches
 * get exactly 0).  No float atomics, bit-reproducible.  ws: mmk_cart_to_polar_bwd_ws_bytes(B, A, R, H, W) bytes. */
size_t mmk_cart_to_polar_bwd_ws_bytes(int32_t B, int32_t A, int32_t R, int32_t H, int32_t W);
int mmk_cart_to_polar_bwd(const double *grad_polar /*B,A,R*/, const double *sin_az, const double *cos_az,
                          const double *range_coords, int32_t B, int32_t A, int32_t R, int32_t H, int32_t W,
                          double radar_resolution, double cart_resolution, double *grad_cart /*B,H,W*/, void *ws,
                          size_t ws_bytes, void *stream);

/* out (B,A,R) = fl32(P) * scan, P = mmk_cart_to_polar of mask_cart (B,H,W) fp32 taken as fp64 (exact) -- the Cartesian mask
 * applied to the polar scan in one pass: one read of scan and one write per polar cell, no polar image of the mask.  The
 * blend is mmk_cart_to_polar's fp64 FMA chain rounded to fp32 once, the product one fp32 multiplication: bit-identical to
 * `radar_cartesian_to_polar(mask.double(), ...).float() * scan`.  A cell without a tap in the image gets +0.0 * scan.
 * sin_az / cos_az (B,A) and range_coords (R) as for mmk_cart_to_polar. */
int mmk_mask_polar_scan(const float *scan /*B,A,R*/, const float *mask_cart /*B,H,W*/, const double *sin_az,
                        const double *cos_az, const double *range_coords, int32_t B, int32_t A, int32_t R, int32_t H,
                        int32_t W, double cart_resolution, float *out /*B,A,R*/, void *stream);

/* Backward of mmk_mask_polar_scan given grad_out (B,A,R).  grad_scan (B,A,R) = grad_out * fl32(P), P recomputed from the
 * mask.  grad_mask (B,H,W) = the adjoint of the bilinear gather applied to fl32(grad_out * scan), in the fixed-point form,
 * with the scale rule and the count bound of mmk_cart_to_polar_bwd on that product widened to fp64, closed by
 * (float)((double)word / scale): bit-identical to autograd through the composition above.  Pixels no ray touches get exactly
 * 0; a non-finite product makes its item's grad_mask NaN.  Either of grad_scan / grad_mask may be NULL: that half is not
 * computed (ws is only needed for grad_mask).  No float atomics, bit-reproducible.
 * ws: mmk_mask_polar_scan_bwd_ws_bytes(B, A, R, H, W) bytes (one 64-bit word per pixel). */
size_t mmk_mask_polar_scan_bwd_ws_bytes(int32_t B, int32_t A, int32_t R, int32_t H, int32_t W);
int mmk_mask_polar_scan_bwd(const float *grad_out /*B,A,R*/, const float *scan /*B,A,R*/, const float *mask_cart /*B,H,W*/,
                            const double *sin_az, const double *cos_az, const double *range_coords, int32_t B, int32_t A,
                            int32_t R, int32_t H, int32_t W, double radar_resolution, double cart_resolution,
                            float *grad_scan /*B,A,R or NULL*/, float *grad_mask /*B,H,W or NULL*/, void *ws, size_t ws_bytes,
                            void *stream);

/* weights[b,n] = bilinear(mask[b], point n) with zero padding; fake points
 * (x==0 && y==0) get 0.  cart_resolution / cart_pixel_width as point_to_cart_idx
 * (radar_utils.py:374-397; extract_weights leaves them at 0.2384 / 640): the points are
 * normalised by the Cartesian grid's width, then F.grid_sample maps [-1,1] onto the mask's own
 * (H,W) -- so a polar (400,3360) mask is sampled exactly as the reference samples it. */
int mmk_sample_weights_fwd(const float *mask /*B,H,W*/, const float *pc /*B,N,pc_cols*/,
                           int32_t B, int32_t N, int32_t pc_cols, int32_t H, int32_t W,
                           int32_t cart_pixel_width, float cart_resolution,
                           float *weights /*B,N*/, void *stream);
/* grad_mask (B,H,W) is zero-filled here, then receives the scatter-add -- in a FIXED order: the taps that fall on one
 * pixel are chained (integer exchanges), and the chain's owner adds them in ascending (point, tap) order, which is
 * the order of a sequential loop over the points (what PyTorch's CPU grid_sample backward does): no float atomics,
 * bit-reproducible.  ws: mmk_sample_weights_bwd_ws_bytes(B, N) bytes. */
size_t mmk_sample_weights_bwd_ws_bytes(int32_t B, int32_t N);
int mmk_sample_weights_bwd(const float *grad_weights /*B,N*/, const float *pc, int32_t B,
                           int32_t N, int32_t pc_cols, int32_t H, int32_t W,
                           int32_t cart_pixel_width, float cart_resolution, float *grad_mask,
                           void *ws, size_t ws_bytes, void *stream);
/* grad_pc (B,N,pc_cols) = dL/dpc of the same gather: grid_sample's gradient with respect to its grid (taps as in the
 * forward, out-of-image taps read 0), chained through point_to_cart_idx.  Written whole: columns 0 and 1 carry it; the
 * other columns and fake points (x==0 && y==0) get 0.  One thread per point, no scatter. */
int mmk_sample_weights_bwd_pc(const float *grad_weights /*B,N*/, const float *mask /*B,H,W*/, const float *pc,
                              int32_t B, int32_t N, int32_t pc_cols, int32_t H, int32_t W,
                              int32_t cart_pixel_width, float cart_resolution, float *grad_pc, void *stream);

/* The polar-aware sampler (radar_utils.extract_weights_polar <- the extract_weights call of icp_weight_policy.py:205 when
 * the mask is the polar network's (A,R) image; params["polar_sampling"]).  weights[b,n] = bilinear(mask[b], point n) at the
 * point's own place in the polar image: rng = sqrt(y^2 + x^2), ang = atan2(y, x) brought into [0, 2 pi) -- the geometry of
 * form_cart_range_angle_grid (radar_utils.py:230-256) -- then the sampling position of mmk_polar_to_cart
 * (radar_utils.py:276-323: u = (rng - res / 2) / res clamped at 0, v from the azimuth table with the wobble fix or the
 * uniform step, the crossover rows, grid_sample's align_corners=True round trip), so a point at the centre of a Cartesian
 * pixel reads what mmk_polar_to_cart writes to that pixel.  Taps outside the (padded) image read 0; fake points
 * (x==0 && y==0) get 0.  azimuths (B,A) ascending, A floats of LDS per block. */
int mmk_sample_weights_polar_fwd(const float *mask /*B,A,R*/, const float *pc /*B,N,pc_cols*/, const float *azimuths /*B,A*/,
                                 int32_t B, int32_t N, int32_t pc_cols, int32_t A, int32_t R, float radar_resolution,
                                 int32_t interpolate_crossover, int32_t fix_wobble, float *weights /*B,N*/, void *stream);
/* Its backward in the mask (_SampleWeightsPolar.backward <- autograd through that gather): grad_mask (B,A,R) is zero-filled
 * here, then receives the scatter-add of grad_weights * tap weight with the crossover rows folded onto their data rows
 * (padded row 0 -> row A-1, padded row A+1 -> row 0), by the ordered chain passes of mmk_sample_weights_bwd: ascending
 * (point, tap) order, no float atomics, bit-reproducible; untouched cells are exactly +0.
 * ws: mmk_sample_weights_polar_bwd_ws_bytes(B, N) bytes. */
size_t mmk_sample_weights_polar_bwd_ws_bytes(int32_t B, int32_t N);
int mmk_sample_weights_polar_bwd(const float *grad_weights /*B,N*/, const float *pc, const float *azimuths, int32_t B, int32_t N,
                                 int32_t pc_cols, int32_t A, int32_t R, float radar_resolution, int32_t interpolate_crossover,
                                 int32_t fix_wobble, float *grad_mask /*B,A,R*/, void *ws, size_t ws_bytes, void *stream);
/* Its backward in the points (_SampleWeightsPolar.backward when scan_pc requires grad): grad_pc (B,N,pc_cols) = the bilinear
 * slopes along u and v times du/drng (1 / res, 0 where u is clamped) and dv/dang (the table segment's slope where the wobble
 * fix interpolates, else 0; 1 / step without it), chained through rng and ang.  Written whole: columns 0 and 1 carry it; the
 * other columns and fake points get 0.  One thread per point, no scatter.  The azimuths get no gradient. */
int mmk_sample_weights_polar_bwd_pc(const float *grad_weights /*B,N*/, const float *mask /*B,A,R*/, const float *pc,
                                    const float *azimuths, int32_t B, int32_t N, int32_t pc_cols, int32_t A, int32_t R,
                                    float radar_resolution, int32_t interpolate_crossover, int32_t fix_wobble,
                                    float *grad_pc /*B,N,pc_cols*/, void *stream);

/* ---- loader primitives (icp_weight_dataset.py:323-362: PNG rows -> load_radar -> augmentation roll -> polar -> Cartesian)
 * mmk_host_read_rows: HOST function, no GPU call, thread-safe: rows [0,rows) of a raw row-major byte file (header_bytes
 * skipped, row_bytes per row; the decoded-scan cache / prepared-cloud cache of ICPWeightDataset), columns
 * [col0, col0+ncols) kept, rows rotated as torch.roll(x, roll, dims=0) (the augmentation's azimuth roll, :446-452),
 * written densely to dst (rows*ncols bytes; typically a slice of the batch's pinned buffer).
 * mmk_u8_to_float: out[i] = lut256[in[i]] on the device -- load_radar's bytes / 255 (radar_utils.py:26) and the CFAR
 * cache's (:343) with the table computed by the host's own fp32 division, so that the values are the reference's bit
 * for bit whatever the device's division rounds to. */
int mmk_host_read_rows(const char *path, int64_t header_bytes, int32_t rows, int32_t row_bytes, int32_t col0,
                       int32_t ncols, int32_t roll, void *dst);
/* The same for a list of jobs (typically every tensor of every item of a batch), spread over `threads` host threads
 * that live for the duration of the call: one interpreter thread drives the whole loader (the reference's four worker
 * processes, train_icp_weights.py:454-455, become four C threads).  Fails if any job fails (first message kept). */
typedef struct mmk_read_job {
    const char *path;
    int64_t header_bytes;
    int32_t rows, row_bytes, col0, ncols, roll, reserved;
    void *dst;
} mmk_read_job;
int mmk_host_read_rows_batch(const mmk_read_job *jobs, int32_t n_jobs, int32_t threads);
int mmk_u8_to_float(const void *in /*n bytes*/, const float *lut256, int64_t n, float *out, void *stream);

/* Statistics extract_weights returns next to the weights (radar_utils.py:130-138) and the policy's
 * mean_all_pts (icp_weight_policy.py:209-212), over the real points (not x==0 && y==0):
 * out[0] diff_mean_num_non0 = sum(0.5 tanh(5w)+0.5)/B, out[1] mean_num_non0 = count(w>0.05)/B,
 * out[2] mean_w, out[3] max_w, out[4] min_w, out[5] mean_all_pts = count(x!=0 && y!=0)/B,
 * out[6] number of real points.  partial: B*8 floats of workspace; out: 8 floats. */
int mmk_weight_stats(const float *weights /*B,N*/, const float *pc /*B,N,pc_cols*/, int32_t B, int32_t N,
                     int32_t pc_cols, float *partial, float *out, void *stream);

int mmk_bev_raster(const float *pc /*B,M,pc_cols*/, int32_t B, int32_t M, int32_t pc_cols,
                   int32_t W, float cart_resolution, float *bev /*B,W,W*/, void *stream);

/* ------------------------------------------------------------------ mask U-Net building blocks
 * Replace nn.Conv2d(3x3, pad 1) + ReLU [+ Dropout] and their autograd of the reference's
 * mask predictor (mm_masking/icp_weight_policy.py:84-99 topology, :104-125 conv_block,
 * :161-184 forward) for its default configuration (ReLU, no batch norm).  Activations are
 * NHWC bf16 (B,H,W,C), C in {8,16,32,64,128,256}; accumulation fp32 on the matrix cores.   */
typedef struct {
    const void *x1;        /* bf16 (B,H,W,C1)                                              */
    const void *x2;        /* bf16 (B,H,W,C2) or NULL: the input is concat(x1, x2) — the
                              torch.cat([skip, x]) of icp_weight_policy.py:180 without a copy */
    int32_t C1, C2;
    const void *wpack;     /* from mmk_conv3x3_pack_weights                                */
    const float *bias;     /* [O1+O2] fp32 or NULL                                          */
    void *y1;              /* bf16 (B,H,W,O1): output channels [0,O1)                       */
    const void *relu_src1; /* optional bf16 (B,H,W,O1): y1 = result * (relu_src1 > 0 ? scale1 : 0)
                              (ReLU / dropout backward fused into the data-gradient pass)   */
    int32_t O1, accumulate1; /* accumulate: y1 += result                                    */
    float scale1;
    void *y2;              /* bf16 (B,H,W,O2) or NULL: output channels [O1,O1+O2); O1 a multiple of 8, and of 16
                              where the layer has >= 64 output channels and >= 32 input channels (else refused) */
    const void *relu_src2;
    int32_t O2, accumulate2;
    float scale2;
    int32_t B, H, W;
    int32_t relu;          /* forward: ReLU after the bias                                  */
    float leaky_slope;     /* > 0: the network's LeakyReLU variant (params["leaky"], nn.LeakyReLU(0.1),
                              icp_weight_policy.py:106): forward max(v, slope v) instead of ReLU; relu_src
                              epilogues use (src > 0 ? scale : src < 0 or -0.0 ? slope*scale : 0) -- a kept
                              zero is stored as -0.0, a dropped element as +0.0.  0 = ReLU              */
    float drop_p;          /* forward: inverted dropout with this probability, quantised to thr / 65536 with
                              thr = round(65536 p): thr = 0 (p < 2^-17) is no dropout, thr = 65536
                              (p >= 1 - 2^-17) is refused like p >= 1                             */
    uint32_t seed;
    void *pool_y;          /* optional bf16 (B,H/2,W/2,O1): nn.MaxPool2d(2,2) of y1 written by the same
                              pass (forward role, single output; layers for which
                              mmk_conv3x3_pool_fusable() returns 1), else NULL                  */
    void *pool_arg;        /* optional, with pool_y: (B,H/2,W/2,O1/2) bytes of arg-max codes, one nibble per channel
                              (channel c in bits 4 (c & 1) of byte c / 2) = position 0..3 of the window's first maximum in
                              scan order | (maximum > 0) << 2.  When set, y1 is NOT written (may be NULL): the pooled
                              tensor and the codes are all that the rest of the network and its backward pass
                              (mmk_maxpool2_bwd_arg) read of this layer's output                  */
    const void *x1_pool_arg; /* optional (NULL: x1 is the input itself).  Set: x1 is a POOLED tensor bf16 (B,H/2,W/2,C1) and the
                              convolution's input is its max-pool adjoint -- what mmk_maxpool2_bwd_arg(x1_pool_arg, x1, B, H, W,
                              C1, x1_pool_scale) would have written as a (B,H,W,C1) tensor, bit for bit -- routed by these
                              arg-max codes (layout: pool_arg) inside the kernel's staging.  ReLU network, C2 = 0, data
                              gradients with a ReLU source or accumulate target of 32 -> 32 and of the >= 64-channel layers;
                              other layers are refused                                            */
    float x1_pool_scale;   /* with x1_pool_arg: the factor of the routed values (dropout's 1 / keep) */
} mmk_conv_desc;

/* sizeof(mmk_conv_desc) as the library was built: a caller with its own mirror of the struct compares it with its mirror's size
 * (the struct grows at its end: x1_pool_arg / x1_pool_scale were appended without a change of MMK_VERSION). */
size_t mmk_conv_desc_bytes(void);
/* 1 when mmk_conv3x3 can write the 2x2 max-pool of this layer's output itself (pool_y). */
int32_t mmk_conv3x3_pool_fusable(int32_t cin, int32_t cout, int32_t B, int32_t H, int32_t W);

/* Packed bf16 element count / packing of fp32 master weights W[cout][cin][3][3].
 * transposed = 1 packs the data-gradient operator (cout -> cin, taps flipped).            */
size_t mmk_conv3x3_packed_elems(int32_t cout, int32_t cin, int32_t transposed);
int mmk_conv3x3_pack_weights(const float *W, int32_t cout, int32_t cin, int32_t transposed,
                             void *packed, void *stream);
/* n layers in one launch: W[i] fp32 (cout[i],cin[i],3,3) -> packed[i] (mmk_conv3x3_packed_elems elements
 * each); replaces the per-layer .to(bf16) casts autocast performs on every nn.Conv2d call
 * (icp_weight_policy.py:104-125 run under torch.autocast). */
int mmk_conv3x3_pack_weights_batch(int32_t n, const float *const *W, const int32_t *cout, const int32_t *cin,
                                   int32_t transposed, void *const *packed, void *stream);
int mmk_conv3x3(const mmk_conv_desc *d, void *stream);
/* Weight + bias gradient of the same convolution (autograd of nn.Conv2d, train_icp_weights.py:51), g = gradient
 * w.r.t. the pre-activation, as per-workgroup partial sums (mmk_conv3x3_wgrad_slices() = number of slices for a shape
 * on the current device, 0 = unsupported shape): every workgroup stores its own slice of `partials`
 * (slices, 9*cout*cin + cout) -- the (9,cout,cin) weight sums followed by the cout bias sums -- with plain
 * stores (accumulate != 0: adds to it -- second application of shared weights) and
 * mmk_conv3x3_wgrad_unpack_batch sums the slices: no float atomics, bit-reproducible. */
int32_t mmk_conv3x3_wgrad_slices(int32_t cout, int32_t cin, int32_t c1, int32_t B, int32_t H, int32_t W);
int mmk_conv3x3_wgrad_partial(const void *x1, const void *x2, int32_t C1, int32_t C2, const void *g, int32_t cout,
                              int32_t B, int32_t H, int32_t W, float *partials, int32_t accumulate, void *stream);

/* Backward pass of a C -> C convolution (C = 8 or 16) whose ReLU source IS its input activation (the second convolution of
 * a U-Net block: icp_weight_policy.py:115-121) in one launch: dx = ((x > 0) ? scale : 0) * conv_T(g) as mmk_conv3x3 gives it
 * with relu_src = x, and the partial slices of mmk_conv3x3_wgrad_partial(x, NULL, C, 0, g, C, ...) -- bit-identical to those
 * two calls, reading x and g once instead of twice.  wpack_t = mmk_conv3x3_pack_weights(W, C, C, transposed = 1);
 * partials holds mmk_conv3x3_wgrad_slices(C, C, C, B, H, W) slices of 9*C*C + C floats. */
int mmk_conv_bwd_fused(const void *x, const void *g, const void *wpack_t, float scale, int32_t B, int32_t H, int32_t W,
                       int32_t C, void *dx, float *partials, int32_t accumulate, void *stream);
/* The same (C = 16) and mmk_conv3x3_wgrad_partial (32 -> 32, or channel counts that are multiples of 64) with the output
 * gradient given as a POOLED gradient gy (B,H/2,W/2,cout) + arg-max codes (mmk_conv_desc.pool_arg layout) + factor: g is the
 * max-pool adjoint mmk_maxpool2_bwd_arg(arg, gy, B, H, W, cout, pool_scale) would have written, taken through the codes while
 * staging -- bit-identical to that launch followed by the plain entry point, without the full-resolution tensor. */
int mmk_conv_bwd_fused_pooled(const void *x, const void *gy, const void *arg, float pool_scale, const void *wpack_t, float scale,
                              int32_t B, int32_t H, int32_t W, int32_t C, void *dx, float *partials, int32_t accumulate,
                              void *stream);
int mmk_conv3x3_wgrad_partial_pooled(const void *x1, const void *x2, int32_t C1, int32_t C2, const void *gy, const void *arg,
                                     float pool_scale, int32_t cout, int32_t B, int32_t H, int32_t W, float *partials,
                                     int32_t accumulate, void *stream);

/* The same for the backward of an 8 -> 16 convolution whose data gradient (16 -> 8) takes the layer's input activation x as
 * ReLU source and ADDS its result to what dx holds (first convolution of encoder block 1: the skip gradient is there
 * already): dx += ((x > 0) ? scale : 0) * conv_T(g), as mmk_conv3x3 with relu_src = x, accumulate = 1, and the partial
 * slices of mmk_conv3x3_wgrad_partial(x, NULL, 8, 0, g, 16, ...): mmk_conv3x3_wgrad_slices(16, 8, 8, B, H, W) slices of
 * 9*16*8 + 16 floats.  x: (B,H,W,8), g: (B,H,W,16), wpack_t = mmk_conv3x3_pack_weights(W, 16, 8, transposed = 1). */
int mmk_conv8x16_bwd_fused(const void *x, const void *g, const void *wpack_t, float scale, int32_t B, int32_t H, int32_t W,
                           void *dx, float *partials, int32_t accumulate, void *stream);

/* ... and for the backward of a 16 -> 8 convolution on concat(x1, x2) (8 channels each) whose data gradient (8 -> 16) is
 * split the same way and masked by the two inputs: dx1 = ((x1 > 0) ? scale : 0) * conv_T(g)[0:8], dx2 likewise with x2 and
 * channels 8:16 (second application of the last decoder block's first convolution), as mmk_conv3x3 with two output parts,
 * relu_src = x1 / x2, and the partial slices of mmk_conv3x3_wgrad_partial(x1, x2, 8, 8, g, 8, ...):
 * mmk_conv3x3_wgrad_slices(8, 16, 8, B, H, W) slices of 9*8*16 + 8 floats.  g: (B,H,W,8).
 * x2 = dx2 = NULL: x1 is ONE (B,H,W,16) input and dx1 ONE (B,H,W,16) output without ReLU source (scale unused):
 * dx1 = conv_T(g), as mmk_conv3x3 without epilogue operands + mmk_conv3x3_wgrad_partial(x1, NULL, 16, 0, g, 8, ...). */
int mmk_conv16x8_bwd_fused(const void *x1, const void *x2, const void *g, const void *wpack_t, float scale, int32_t B, int32_t H,
                           int32_t W, void *dx1, void *dx2, float *partials, int32_t accumulate, void *stream);
/* n layers in one launch (no accumulation): dW[i] (cout,cin,3,3) = src[i] (9,cout,cin) when slices is NULL or
 * slices[i] == 0; else the sum over the slices[i] partial slices of src[i], and db[i] (cout, optional) their
 * bias sums */
int mmk_conv3x3_wgrad_unpack_batch(int32_t n, const float *const *src, const int32_t *slices, const int32_t *cout,
                                   const int32_t *cin, float *const *dW, float *const *db, void *stream);

/* First conv of the network (encoder.0.0): fp32 NCHW input (B,cin,H,W), cin = 1..4
 * (fft | cfar | range channels, icp_weight_policy.py:84), W[8][cin][3][3], + bias + ReLU ->
 * bf16 (B,H,W,8).  _wgrad: dW[8][cin][3][3] += , db[8] += (g = grad w.r.t. the pre-activation).
 * pre (may be NULL): 2 floats per input channel (offset, reciprocal scale); the kernels then read
 * (x - offset) * rscale — the policy's per-channel min-max normalisation
 * (icp_weight_policy.py:151-155) applied while loading.  mmk_channel_minmax fills pre with
 * (min, 1 / (max - min)) over (B,H,W) per channel; part: C*2048 floats of workspace; minmax (optional):
 * the raw (min, max) pairs, what a data-parallel job reduces over its ranks to keep the normalisation
 * batch-global (mm_masking_amd/icp_weight_policy.py: params["global_minmax"]). */
int mmk_channel_minmax(const float *x /*B,C,hw*/, int32_t B, int32_t C, int64_t hw, float *part,
                       float *pre /*C*2*/, float *minmax /*C*2 or NULL*/, void *stream);
/* mmk_channel_meanstd fills pre with (mean, 1 / std) over (B,H,W) per channel, std the unbiased (n - 1) standard deviation of
 * torch.std: the policy's standardisation (icp_weight_policy.py:156-159).  Two ordered fp64 passes; part: C*2048 doubles of
 * workspace.  A constant channel gives 1 / std = inf (the reference divides by zero). */
int mmk_channel_meanstd(const float *x /*B,C,hw*/, int32_t B, int32_t C, int64_t hw, double *part,
                        float *pre /*C*2*/, void *stream);
int mmk_conv_first(const float *x, int32_t cin, const float *W, const float *bias, const float *pre,
                   int32_t B, int32_t H, int32_t Wd, float leaky_slope, void *y, void *stream);
/* dW[8][cin][3][3] and db[8] are WRITTEN (not added to): per-block partial sums into ws, then one ordered reduction --
 * no float atomics, bit-reproducible.  ws: mmk_conv_first_wgrad_ws_bytes(cin) bytes. */
size_t mmk_conv_first_wgrad_ws_bytes(int32_t cin);
int mmk_conv_first_wgrad(const float *x, int32_t cin, const void *g, const float *pre, int32_t B,
                         int32_t H, int32_t Wd, float *dW, float *db, float *ws, size_t ws_bytes, void *stream);
/* Gradient with respect to the network's input image (nothing upstream to mirror: the reference leaves its
 * `fft_data...#.requires_grad_(True)` commented out, icp_weight_policy.py:130, and its in-place normalisation :151-159 cannot
 * be differentiated by autograd).  Two steps:
 * mmk_conv_first_dgrad: grad_x (B,cin,H,Wd) fp32 is WRITTEN with rscale_c * g_n,
 *   g_n[b,c,y,x] = sum_co sum_ky,kx g[b, y+1-ky, x+1-kx, co] * W[co][c][ky][kx] over the in-image source pixels
 *   (g = (B,H,Wd,8) bf16, the gradient mmk_conv_first_wgrad consumes; the bf16 rounding of the input is straight-through;
 *   pre == NULL: rscale = 1).  Gather form, no float atomics, bit-reproducible.
 *   ws (may be NULL: no statistics; else x and pre are required): mmk_conv_first_dgrad_ws_bytes(cin) bytes; the same pass then
 *   sums per channel S1 = sum g_n and S2 = sum g_n * x_n, x_n = (x - offset) * rscale, and with minmax (the raw (min, max) pairs
 *   of mmk_channel_minmax) counts the elements equal to each extremum -- fp64 block partials added in a fixed order.
 * mmk_input_norm_bwd: adds the adjoint of the statistics to grad_x in place, from that ws.  MMK_NORM_MINMAX: dL/dmin =
 *   r * (S2 - S1) and dL/dmax = -r * S2 (r = pre[2c+1]), each shared evenly among the elements equal to the extremum (as
 *   torch.min / torch.max of a whole tensor do).  MMK_NORM_STANDARDIZE (mmk_channel_meanstd): grad_x = (g_n - S1 / n - x_n * S2 /
 *   (n - 1)) / sigma, n = B * H * Wd.  MMK_NORM_NONE: nothing to add (no launch).  Argument errors return MMK_ERR_ARG. */
#define MMK_NORM_NONE 0
#define MMK_NORM_MINMAX 1
#define MMK_NORM_STANDARDIZE 2
size_t mmk_conv_first_dgrad_ws_bytes(int32_t cin);
int mmk_conv_first_dgrad(const void *g, int32_t cin, const float *W, const float *x /*or NULL*/, const float *pre /*or NULL*/,
                         const float *minmax /*or NULL*/, int32_t B, int32_t H, int32_t Wd, float *grad_x, void *ws /*or NULL*/,
                         size_t ws_bytes, void *stream);
int mmk_input_norm_bwd(float *grad_x, const float *x, int32_t cin, const float *pre, const float *minmax /*MINMAX only*/,
                       int32_t mode, int32_t B, int32_t H, int32_t Wd, const void *ws, size_t ws_bytes, void *stream);

/* nn.MaxPool2d(2,2) on NHWC bf16 (icp_weight_policy.py:122-123).  _bwd fuses the backward of
 * the preceding Dropout(ReLU(.)): gz = route(gy) * (d > 0 ? scale : 0), d = the pooled tensor's
 * source (B,H,W,C).                                                                          */
int mmk_maxpool2_fwd(const void *x, int32_t B, int32_t H, int32_t W, int32_t C, void *y, void *stream);
int mmk_maxpool2_bwd(const void *d, const void *gy, int32_t B, int32_t H, int32_t W, int32_t C, float scale,
                     float leaky_slope, void *gz, void *stream);
/* The same pair through arg-max codes (layout: mmk_conv_desc.pool_arg): _fwd_arg also writes the codes, _bwd_arg routes
 * gy by them instead of re-deriving the arg-max from the full-resolution tensor d (ReLU network: leaky_slope = 0) --
 * gz is bit-identical to mmk_maxpool2_bwd's, from C/2 + 2C bytes per window instead of 10C.                          */
int mmk_maxpool2_fwd_arg(const void *x, int32_t B, int32_t H, int32_t W, int32_t C, void *y, void *arg, void *stream);
int mmk_maxpool2_bwd_arg(const void *arg, const void *gy, int32_t B, int32_t H, int32_t W, int32_t C, float scale,
                         void *gz, void *stream);

/* nn.UpsamplingBilinear2d(size) = bilinear, align_corners=True (icp_weight_policy.py:175-176).
 * _bwd is the adjoint in gather form; relu_src (optional, source-sized) applies
 * (relu_src > 0 ? scale : 0).                                                                */
int mmk_upsample_fwd(const void *x, int32_t B, int32_t Hs, int32_t Ws, int32_t C, int32_t Ho, int32_t Wo, void *y,
                     void *stream);
int mmk_upsample_bwd(const void *gy, int32_t B, int32_t Hs, int32_t Ws, int32_t C, int32_t Ho, int32_t Wo,
                     const void *relu_src, float scale, float leaky_slope, void *gx, void *stream);

/* final_layer: Conv2d(8,1,1x1) + Sigmoid (icp_weight_policy.py:96-99,184): bf16 (npix,8) -> fp32
 * mask (npix).  _bwd: gx = dL/dx * (x > 0 ? scale : 0) (bf16); dW[8] and db[1] are WRITTEN: per-block partial
 * sums into ws (MMK_FINAL_BWD_WS_FLOATS floats), then one ordered reduction -- no float atomics.  */
#define MMK_FINAL_BWD_WS_FLOATS 16384
int mmk_final_fwd(const void *x, const float *w, const float *bias, int64_t npix, float *mask, void *stream);
int mmk_final_bwd(const void *x, const float *w, const float *mask, const float *gmask, int64_t npix, float scale,
                  float leaky_slope, void *gx, float *dW, float *db, float *ws, void *stream);
/* mask_n = mask / amax(mask over the image) per image (icp_weight_policy.py:192-193), amax (B) out;
 * part: B*64 floats of workspace. */
int mmk_mask_normalize(const float *mask /*B,npix_per*/, int32_t B, int64_t npix_per, float *part,
                       float *mask_n, float *amax, void *stream);
/* mmk_final_bwd for a mask that went through mmk_mask_normalize: gmask_n is the gradient w.r.t.
 * mask_n; the adjoint of the division and of amax (spread evenly over tied maxima, as torch.amax)
 * is applied on the fly.  part: B*128 floats, coef: 2*B floats, ws: MMK_FINAL_BWD_WS_FLOATS floats of workspace. */
int mmk_final_bwd_normalized(const void *x, const float *w, const float *mask, const float *mask_n,
                             const float *amax, const float *gmask_n, int32_t B, int64_t npix_per,
                             float scale, float leaky_slope, float *part, float *coef, void *gx, float *dW,
                             float *db, float *ws, void *stream);

/* nn.BatchNorm2d of the network's batch-norm variant (params["batch_norm"], icp_weight_policy.py:108-113) on NHWC
 * bf16 (npix, C).  _forward_stats: batch statistics -> stat (C,2) = (mean, 1/sqrt(var + eps)) and affine (C,2) =
 * (scale, shift); running_mean / running_var (both or neither) updated as torch does (momentum, unbiased variance);
 * part: 512*C*2 floats of workspace.  _apply: y = a * scale + shift, then the block's inverted dropout (drop_p, seed;
 * 0 = none); a kept zero is stored as -0.0, a dropped value as +0.0.  _backward: gd = dL/d(output), d = the stored
 * post-dropout output when a dropout followed (else NULL; gy = gd * (d != +0 ? drop_scale : 0)), a = the BatchNorm
 * input (= ReLU / LeakyReLU output); writes gz = dL/d(pre-activation of the convolution in front of the ReLU),
 * dgamma / dbeta (accumulate != 0: adds -- decoder blocks run twice with shared modules); stat == NULL selects the
 * evaluation-mode form gz = gy * scale * act'(a).  coef: 3*C floats of workspace. */
int mmk_bn_forward_stats(const void *a, int64_t npix, int32_t C, const float *gamma, const float *beta, float eps,
                         float momentum, float *running_mean, float *running_var, float *part, float *stat,
                         float *affine, void *stream);
int mmk_bn_apply(const void *a, int64_t npix, int32_t C, const float *affine, float drop_p, uint32_t seed, void *y,
                 void *stream);
int mmk_bn_backward(const void *gd, const void *d, float drop_scale, const void *a, int64_t npix, int32_t C,
                    const float *stat, const float *affine, const float *gamma, float leaky_slope, int32_t accumulate,
                    float *part, float *coef, float *dgamma, float *dbeta, void *gz, void *stream);

/* ------------------------------------------------------------------ the mask U-Net as two calls
 * mmk_unet_forward replaces the network part of LearnICPWeightPolicy.forward
 * (mm_masking/icp_weight_policy.py:161-199: encoder, twice-applied decoder blocks, 1x1 + sigmoid, amax
 * normalisation) and mmk_unet_backward its autograd (train_icp_weights.py:51), sequencing the building
 * blocks above from the host side of the ABI: ~290 launches per training step without a Python call each.
 * Results are bit-identical to issuing the same building blocks one by one (tests/test_gpu_unet_driver.py). */
typedef struct {
    int32_t B, H, W, cin;       /* network input: fp32 NCHW (B,cin,H,W), cin = 1..4, H, W >= 32          */
    const float *x;
    const float *pre;           /* (cin,2) offset / reciprocal scale from mmk_channel_minmax, or NULL     */
    const float *const *params; /* HOST array of 46 device pointers in state_dict order: weight, bias of
                                   encoder.{0..5}.{0,2}, decoder.{0..4}.{0,2}, final_layer.0 (fp32 masters) */
    float drop_p;               /* dropout probability of this pass (0 in eval mode)                      */
    uint32_t seed;              /* dropout stream of this pass                                            */
    float leaky_slope;          /* 0 = ReLU, else nn.LeakyReLU(slope) (params["leaky"])                    */
    int32_t norm;               /* 1: mask / amax(mask) per image (params["norm_weights"])                */
    void *workspace;            /* mmk_unet_workspace_bytes(): packed weights + every activation; written by
                                   the forward, read by the backward -- the caller keeps it in between     */
    size_t workspace_bytes;
    float *mask;                /* (B,H,W) fp32: output of the forward, input of the backward             */
    int32_t keep_full_res;      /* 1: the encoder blocks whose second convolution pools in the same pass also write
                                   their pre-pool output (mmk_unet_tensor ids 7, 8; diagnostics).  0: they write the
                                   pooled tensor and its arg-max codes only -- nothing else reads that output     */
} mmk_unet_desc;

size_t mmk_unet_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t cin);
/* scratch of the backward pass (gradient tensors, partial sums); needs a HIP device (occupancy queries) */
size_t mmk_unet_scratch_bytes(int32_t B, int32_t H, int32_t W, int32_t cin);
int mmk_unet_forward(const mmk_unet_desc *d, void *stream);
/* gmask (B,H,W) fp32 = dL/dmask; grads: HOST array of 46 device pointers, same order and shapes as params,
 * overwritten with dL/dparam. */
int mmk_unet_backward(const mmk_unet_desc *d, const float *gmask, float *const *grads, void *scratch,
                      size_t scratch_bytes, void *stream);
/* Data-parallel form of mmk_unet_backward (nothing upstream to mirror: the reference has no multi-GPU path; BASELINE.json
 * configs[3] asks for the gradient all-reduce to overlap the backward pass).  The parameter gradients of a pass become final
 * in MMK_UNET_GRAD_BUCKETS groups; mmk_unet_grad_bucket tells which contiguous run of the 46 parameters (state_dict order)
 * group `bucket` holds -- 0: decoder + final layer (24..45), 1: encoder blocks 3-5 (12..23), 2: encoder blocks 0-2 (0..11),
 * the order in which they complete.  bucket_events: HOST array of MMK_UNET_GRAD_BUCKETS hipEvent_t the caller created;
 * event b is recorded behind the last kernel that writes a gradient of group b, so another stream that waits for it may
 * read (all-reduce) that group while the rest of the pass is still running.  Results are those of mmk_unet_backward. */
#define MMK_UNET_GRAD_BUCKETS 3
int32_t mmk_unet_grad_bucket(int32_t bucket, int32_t *first_param, int32_t *n_params);
int mmk_unet_backward_buckets(const mmk_unet_desc *d, const float *gmask, float *const *grads, void *scratch,
                              size_t scratch_bytes, void *const *bucket_events, void *stream);
/* mmk_unet_backward (bucket_events == NULL) or mmk_unet_backward_buckets, and in the same stream-ordered call the gradient with
 * respect to the input image: the backward schedule runs unchanged, then mmk_conv_first_dgrad + mmk_input_norm_bwd on the
 * gradient of the first pre-activation, which is still in scratch (the statistics' workspace is the one the first layer's
 * weight gradient has just released).  grad_x (B,cin,H,W) fp32 is overwritten.  norm_mode: MMK_NORM_NONE (d->pre, when given,
 * is a pair of constants), MMK_NORM_MINMAX (d->pre from mmk_channel_minmax of d->x, minmax = its raw (min, max) pairs) or
 * MMK_NORM_STANDARDIZE (d->pre from mmk_channel_meanstd of d->x).  The gradient through extrema that were reduced over the
 * ranks of a data-parallel job is out of scope. */
int mmk_unet_backward_input(const mmk_unet_desc *d, const float *gmask, float *const *grads, float *grad_x, int32_t norm_mode,
                            const float *minmax, void *scratch, size_t scratch_bytes, void *const *bucket_events, void *stream);
/* Where an activation lives inside the workspace (tests / diagnostics): id 0..5 first conv output of encoder
 * block i, 6..11 second (post-dropout) output, 12..17 t[i] (block output after pooling), 18 + 5 j + {0..4}:
 * decoder block j's up-sampled input, a1, d1, a2, d2.  NHWC bf16 (B,h,w,c) at byte `offset`. */
int mmk_unet_tensor(int32_t B, int32_t H, int32_t W, int32_t cin, int32_t id, size_t *offset, int32_t *h,
                    int32_t *w, int32_t *c);

#ifdef __cplusplus
}
#endif
#endif /* MMK_H_ */
