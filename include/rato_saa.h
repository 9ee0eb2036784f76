/*
 * rato_saa.h — C ABI of the MI355X-native SAA inner loop (librato_saa.so).
 *
 * Drop-in boundary for the hot path of StanfordASL/RiskAverseTrajOpt: the
 * per-SCP-iteration batched rollout, control-Jacobian linearization, sample
 * mean and Monte-Carlo VaR/CVaR evaluation over M samples x S steps.  The
 * reference has no FFI for this path (it is pure Python on JAX-CPU); each entry
 * point below names the reference method (file:line under /root/reference) it
 * replaces.  INTEGRATION.md shows the ctypes stub a maintainer would add.
 *
 * Conventions (all entry points):
 *   - extern "C", plain pointers and sizes, no torch types.
 *   - every data pointer is a CALLER-OWNED DEVICE pointer (fp32 unless noted),
 *     e.g. torch.Tensor.data_ptr(); nothing is allocated or freed here.
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream); calls
 *     are asynchronous and stream-ordered and never synchronise the device --
 *     with the exceptions that exist to BE the synchronisation point of a host
 *     loop and say so where they are declared: rato_stream_synchronize,
 *     rato_cut_oracle_rollout (one oracle round trip of the cutting-plane loop:
 *     its results are read by the host master) and rato_cut_solve (the whole
 *     loop of one SCP subproblem).  Each waits for the work it issued on
 *     `stream` only, never for the device: by watching the words its last
 *     launch writes into the caller's PINNED host buffers arrive (every kernel
 *     in front of that launch has then completed; the HIP runtime is asked --
 *     hipStreamSynchronize -- only when RATO_CUT_POLL=0 is set or the words stay
 *     away for 2 s, e.g. after a failed launch, whose error comes out there).
 *   - no global state beyond cached device properties (CU count, LDS attribute) and, for the row-parallel
 *     linearize kernels on large batches, one self-cleaning two-word work queue per STREAM in device memory
 *     (up to 64 streams; launches on one stream are ordered and share it, a 65th stream falls back to the static
 *     launch): safe to call concurrently from one host thread per GPU, and — after one ordinary call per kernel
 *     variant — inside a hipGraph stream capture (no non-stream runtime call is made).
 *   - return value: 0 ok; RATO_EINVAL bad argument; RATO_EHIP-<hipError_t>
 *     when a launch fails.
 *   - the sample index m is ALWAYS the fastest-varying index (SoA), so every
 *     wave reads/writes 256 contiguous bytes per instruction.
 *
 * Packed causal layout of the obstacle/separation Jacobian: d g_t / d u_s is
 * identically zero unless s <= t-1 (position lags control by two steps), so
 * only the pairs (t, s), 0 <= s < t < S are stored, row-major in t:
 *     pair(t, s) = t*(t-1)/2 + s,   n_pairs = S*(S-1)/2.
 * The Jacobian buffer G is tile-blocked SoA: samples are grouped in tiles of
 * TILE consecutive samples and each tile is a contiguous [rows][TILE] block, so
 * that one wave's / workgroup's output is one contiguous region that it writes
 * as a stream:
 *     G[tile][row][lane],  tile = m / TILE, lane = m % TILE,
 *     n_tiles = ceil(M / TILE); lanes >= M of the last tile are not written.
 * Tile stride: consecutive tiles are rato_packed_tile_stride(rows * TILE) floats apart -- back to back while a tile
 * is smaller than 1 MiB, otherwise every tile starts on a 2 MiB boundary and G itself must be 2 MiB aligned
 * (buffer size: n_tiles * stride floats).  One rule from the tile shape alone, shared by every producer and consumer
 * of the layout in this library (linearize, rowmax / tail rows, CSC emission).  It is there for the write path: the
 * row-parallel kernels keep one store stream per resident tile, and 512 streams a power-of-two distance apart are
 * spread evenly over the memory channels (1.88 MB tiles, store-only: 5.1-5.2 TB/s back to back, 5.7 at 2 MiB).
 * TILE depends on the kernel variant and is reported by the *_plan() call
 * (64 for the row-parallel drone kernel, RATO_TILE = 256 otherwise).
 */
#ifndef RATO_SAA_H
#define RATO_SAA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RATO_OK 0
#define RATO_EINVAL (-1)
#define RATO_ENONFINITE (-2) /* a checked output holds NaN/Inf: the reference only prints
                                "[solve]: Problem infeasible." (drone_risk.py:458-459) and carries on.
                                Raised by the facades (check_finite=True) from rato_count_nonfinite_acc. */
#define RATO_EINFEASIBLE (-4) /* rato_master_solve: the rows of the master QP admit no point */
#define RATO_ENOCOMM (-3)    /* librccl could not be bound at run time (rato_comm_*) */
#define RATO_ERANK (-6)      /* rato_cut_solve: the final rows are rank deficient / not fewer than the variables */
#define RATO_ESELECT (-7)    /* rato_cut_solve: an oracle round trip came back with NaN statistics (the one-launch tail
                                selection gave up, or the m values hold NaN): repeat with the recovering host loop */
#define RATO_ENNLS (-8)      /* rato_cut_solve: the NNLS of the master did not converge */
#define RATO_EHIP (-1000)    /* RATO_EHIP - hipError_t */
#define RATO_ERCCL (-2000)   /* RATO_ERCCL - ncclResult_t */

#define RATO_TILE 256        /* samples per Jacobian tile (= workgroup size) */
#define RATO_DRONE_NOBS 3   /* drone_params.py:34-43: n_obs = 3 */
#define RATO_HOPPER_NFEAT 30 /* hopper.py:69: num_mu_features = 30 */

/* ABI version, bumped on any signature/layout change (2: factored Jacobian W / A22 outputs, CVaR-cut oracle
 * entry points, record unpack; 3: generators-only linearization, Jacobian-free tail rows, a22_axes; 4: rato_comm_*
 * (RCCL behind the ABI), rato_car_separation_distances, rato_count_nonfinite_acc, Philox sampler entry points;
 * 5: rato_*_linearize_philox, rato_hopper_slip_host_inputs; 6: packed tile stride (rato_packed_tile_stride /
 * rato_packed_buffer_floats), rato_sums_and_risk_stats; 7: fp64 CVaR-cut oracle -- rato_saa_rowmax /
 * rato_drone_rowmax_implicit take (base, sign, double xs), the tail-row entry points write double partials
 * (rato_sum_partials_f64), rato_saa_tail_rows folded into rato_saa_tail_rows_batch (slots == NULL), params.rows_out,
 * rato_drone_rowmax_rollout / rato_drone_tail_rows_rollout, rato_comm_available, rato_device_occupy; 8: fp64 constants in
 * rato_car_params, rato_car_rowmax_rollout / rato_car_tail_rows_rollout, rato_cut_oracle_rollout, rato_nnls_warm, rato_master_*,
 * (9: rato_cut_solver_* / rato_cut_begin / rato_cut_solve -- the cutting-plane loop of a subproblem as one call;
 * params.stats_* -- the statistics of Z in extra workgroups of the row-parallel linearize launch itself)
 * rato_copy_async, rato_stream_synchronize, rato_risk_stats_recover; 12: rato_hopper_slip_hessian,
 * rato_hopper_jacobian_nnz / rato_hopper_emit_jacobian_values -- the hopper's jacrev / Lagrangian Hessian in the reference's
 * layout; rato_scp_run_drone / rato_scp_iter -- the reduced SCP loop as one call; rato_car_ego_final_rows, rato_scp_run_car,
 * rato_scp_batch_run_car -- additions within version 12: the same for the driving problem; rato_drone_rows_plan /
 * rato_car_rows_plan -- a further addition within version 12: the row kernels' launch geometry as a query;
 * rato_hopper_slip_f64 / rato_hopper_slip_f64_nblocks / rato_hopper_slip_hess_blocks_f64 -- likewise: the hopper's slip rows in fp64;
 * rato_hopper_slip_f64_fields -- likewise: the same with friction fields per problem;
 * rato_risk_stats_shaped -- likewise: the selection at the workgroup sizes of the launches that carry their statistics;
 * rato_risk_stats_rows / _rows_init / _rows_workspace_bytes / _rows_plan -- likewise: K rows, each with its own alpha, at any M).
 * The Python binding refuses a library that reports another version. */
#define RATO_ABI_VERSION 12
#define RATO_STATS_IN_LAUNCH 1   /* params.stats_flags */
int rato_abi_version(void);

/* floats between consecutive tiles of a packed tile-blocked Jacobian whose tile holds payload_floats numbers */
size_t rato_packed_tile_stride(size_t payload_floats);
/* floats a packed buffer of n_tiles such tiles needs (n_tiles * stride): what to allocate for G -- the linearize entry
 * points take no buffer sizes, so a G allocated as n_tiles * payload_floats is overrun when the tiles are padded */
size_t rato_packed_buffer_floats(size_t n_tiles, size_t payload_floats);

/* Diagnostic (no reference counterpart): the shader clock the device sustains at this moment -- shader-cycle counter
 * against the constant 100 MHz counter over `us` microseconds (1..100000), one wave.  out3 (device, 3 doubles) =
 * { MHz, elapsed us, 0 }.  bench.py quotes it beside the roofline (boxes of one pool run the same binary several
 * percent apart). */
int rato_device_clock_probe(double* out3, int32_t us, void* stream);

/* Diagnostic (tests): `blocks` workgroups of 1024 threads hold their wave slots for `us` microseconds (<= 5 s); 512 of
 * them occupy every wave slot of an MI355X.  Used to show that the one-launch statistics, which wait inside the
 * launch for their own workgroups, survive a chip that another stream owns. */
int rato_device_occupy(int32_t blocks, int64_t us, void* stream);

/* Plumbing for the facades' small transfers inside the SCP loop: one asynchronous copy between device memory and
 * (pinned) host memory in either direction on `stream` (hipMemcpyDefault), and the matching synchronisation. */
int rato_copy_async(void* dst, const void* src, size_t bytes, void* stream);
int rato_stream_synchronize(void* stream);

/* ------------------------------------------------------------------ drone */

/* Constants of drone_params.py:1-45 / Model.__init__ drone_risk.py:71-93. */
typedef struct rato_drone_params {
  int32_t M;            /* samples in this shard (< 2^31: one GPU holds ~2e7 drone samples at S = 50; every offset
                           derived from it is computed in 64 bits) */
  int32_t ld;           /* row stride (floats) of every [..][M] array, ld >= M; a multiple
                           of samples_per_lane (use a multiple of 4) */
  int32_t S;            /* control intervals; dt = T/S (drone_risk.py:82) */
  float dt;
  float beta;           /* diffusion magnitude, 1e-2 */
  float drag;           /* drag_coefficient, 0.2 */
  float kp, kd;         /* -feedback_gain: 0.05, 0.25 */
  float tol;            /* OSQP_TOL subtracted from the max constraint (1e-3) */
  float x_init[6];
  float x_final[6];
  float obs_xy[RATO_DRONE_NOBS][2];  /* obs_positions[:, :2] */
  int32_t rows_out;     /* what the linearize entry points write into their g_up buffer: 0 = the reference's
                           g_up = -g + (grad g).u_k (drone_risk.py:278); 1 = the constraint value g at u_k itself
                           (the base of the oracle's delta form: rows(u) = g + G (u - u_k), see rato_saa_rowmax) */
  /* The same constants in fp64, for the entry points that compute in double precision (the generators-only
   * linearization and the CVaR-cut oracle): the reference's constants are Python floats, and 0.05f is 1.5e-8 away from
   * 0.05, -1.4f is 2.4e-8 away from -1.4 -- which an obstacle row sees as 5e-7 of d = p - o where the drone grazes the
   * obstacle.  The fp32 kernels keep reading the float fields above; fill both from the same numbers. */
  double dt64, beta64, drag64, kp64, kd64, tol64;
  double x_init64[6];
  double x_final64[6];
  double obs_xy64[RATO_DRONE_NOBS][2];
  /* Statistics with the linearization (round 4).  stats_workspace != NULL (an initialised rato_risk_stats workspace;
     row-parallel kernel only: cols_per_thread = -1; Z requested; M <= 524,288): the call also leaves the rato_risk_stats
     record of the Z it produces in stats_out (double[RATO_N_STATS]; tail level stats_alpha, threshold stats_thr).
     SMALL batches (every workgroup of the launch resident at once: fewer tiles than workgroup slots, e.g. BASELINE C2 /
     C3) compute it in a few extra workgroups of the SAME launch: Z is written right after the rollout, the statistics
     workgroups wait until every tile's Z has been counted in and select while the Jacobian is still being stored -- no
     dependent statistics launch.  Larger batches issue rato_risk_stats behind the kernel from the same call: beside a
     store-saturated producer the selection's dependent global round trips run several times slower than behind it.
     Same selection, same record (fp64 sums equal to summation order).  Ignored by every other entry point. */
  void* stats_workspace;
  double* stats_out;
  double stats_alpha;
  float stats_thr;
  int32_t stats_flags;       /* RATO_STATS_IN_LAUNCH: rato_drone_eval computes them in its own launch (default: behind it) */
} rato_drone_params;

/*
 * Replaces Model.us_to_state_trajectories (drone_risk.py:139-162) fused with
 * obstacle_avoidance_constraints (:169-213) and the Monte-Carlo closure
 * monte_carlo_no_collisions_constraint_verification (:656-662).
 *   us    [S][3]            controls
 *   dW    [S][3][ld]        velocity rows 3..5 of the reference's DWs (M,S,6)
 *   mass  [M]
 *   Qsym  [3 obs][3][M]     (Q00, Q01+Q10, Q11) of obs_Q[:, :2, :2]
 * (every "[M]" below is a row of p->ld floats of which the first M are used)
 * outputs (any may be NULL):
 *   Z     [M]               max_{j,t} g - tol
 *   xs    [S+1][6][M]       state trajectories (SoA of the reference's (M,S+1,6))
 *   g     [3 obs][S][M]     constraint values
 * Without trajectories (xs == NULL) the tiled kernel runs: one wave per tile of 64 samples, the noise of 32 steps in
 * flight before the first step, the vertical axis (which no obstacle row reads) not rolled out; Z and g to the bit as
 * with trajectories.
 * Monte-Carlo step in one call (ABI 11; drone_risk.py:643-725: rollout -> max -> fraction / VaR / AVaR): with
 * p->stats_workspace / stats_out / stats_alpha / stats_thr set (and Z requested) the call also leaves the rato_risk_stats
 * record of Z in stats_out -- by rato_risk_stats behind the kernel; with RATO_STATS_IN_LAUNCH in p->stats_flags, for
 * batches without trajectories up to rato_drone_eval_stats_in_launch(M), in an extra workgroup of the SAME launch
 * (measured slower than the two launches: DESIGN.md; kept for A/B).
 */
int rato_drone_eval_stats_in_launch(int32_t M);
int rato_drone_eval(const rato_drone_params* p, const float* us, const float* dW,
                    const float* mass, const float* Qsym,
                    float* Z, float* xs, float* g, void* stream);

/* Kernel variants of rato_drone_linearize:
 *   cols_per_thread = -1            row-parallel adjoint kernel (default; needs
 *                                   20*64*S + 16 bytes of LDS <= 160 KB, S >= 2)
 *   cols_per_thread in {4,8,16,32}  forward column kernel, samples_per_lane 1
 *   samples_per_lane 2 x cpt {4,8}, samples_per_lane 4 x cpt {2,4}
 * This call resolves 0 / 0 ("let the library choose") to a concrete pair and
 * returns the number of sample blocks the launch will use = rows of
 * part.  Returns <0 on bad arguments. */
int rato_drone_linearize_plan(int32_t M, int32_t S, int32_t ld,
                              int32_t* cols_per_thread, int32_t* samples_per_lane,
                              int32_t* tile /* out: TILE of the G layout */);

/*
 * Replaces vmap(Model.get_all_constraints_coeffs) (drone_risk.py:239-290) and
 * the per-block stage of the sample mean (:294-296).
 * outputs:
 *   G        W == NULL: [n_tiles][n_pairs][2 axes][3 obs][TILE]
 *                                         d g[j,t] / d u[s,axis] for s<t
 *                                         (the z-control column is identically 0)
 *            W != NULL (factored, row-parallel kernel only):
 *                       [n_tiles][n_pairs][2 axes][TILE]   Phi[t,s,axis] = d p_axis(t+1) / d u[s,axis]
 *   W        NULL, or  [3 obs][S][2 axes][ld]              W[j,t,axis] = d g[j,t] / d p_axis(t+1),
 *            so that d g[j,t]/d u[s,axis] = W[j,t,axis] * Phi[t,s,axis]: the three obstacles share
 *            Phi, i.e. the same Jacobian in S(S-1) + 6S instead of 3S(S-1) numbers per sample.
 *   A22      NULL, or  [S][2 axes][ld]  (row-parallel kernel only)  the state-dependent entry of the step
 *            Jacobian A_t = d x_{t+1} / d x_t = [[1, dt], [-kp dt/m, A22[t]]] per horizontal axis: with W and
 *            g_up this is the whole linearization in 11 S numbers per sample, enough to evaluate G.u for
 *            ANY u by an O(S) recursion (rato_drone_rowmax_implicit) instead of an O(S^2) read of Phi.
 *   g_up     [3 obs][S][M]                -g + grad g . u   (:278)
 *   Z        [M] or NULL                  max_{j,t} g - tol at this iterate
 *   part     [nblocks][6*S + 6]           per-block sums (nblocks from rato_drone_linearize_plan):
 *                                         [s*6 + e], e = (P_x,P_y,P_z,V_x,V_y,V_z): d x_S / d u_{s,axis};
 *                                         [6*S + r]: -v_final + v_final_du.u (:271), r = row of x
 * cols_per_thread / samples_per_lane: see rato_drone_linearize_plan (0 = choose).
 * All [..][M] arrays (dW, mass, Qsym, g_up, Z) use the row stride p->ld.
 */
int rato_drone_linearize(const rato_drone_params* p, const float* us, const float* dW,
                         const float* mass, const float* Qsym,
                         float* G, float* W, float* A22, float* g_up, float* Z, float* part,
                         int32_t cols_per_thread, int32_t samples_per_lane, void* stream);

/* Model.obstacle_avoidance_constraints on given trajectories (drone_risk.py:198-213).
 *   xs [S+1][6][M] -> g [3 obs][S][M] */
int rato_drone_obstacle_constraints(const rato_drone_params* p, const float* xs,
                                    const float* Qsym, float* g, void* stream);

/* The reference's Monte-Carlo report evaluates MANY control sequences on one validation batch (drone_risk.py:697-725:
 * 4 alpha x 30 repeats; driving.py:675-740): K sequences in ONE call -- the rollouts of all of them in one launch
 * (grid = tiles x K: a single sequence at M = 1e4 occupies 157 of the chip's 1024 SIMDs), the K exact selections in a
 * second one.    us [K][S][n_u];  Z [K][ldz] (ldz >= M);  stats_out [K][RATO_N_STATS] or NULL (then alpha, thr,
 * workspace are not read).  Row k is, to the bit, what rato_*_eval + rato_risk_stats give for sequence k. */
int rato_drone_eval_batch(const rato_drone_params* p, int32_t K, const float* us, const float* dW, const float* mass,
                          const float* Qsym, float* Z, int64_t ldz, double alpha, float thr, void* workspace,
                          size_t workspace_bytes, double* stats_out, void* stream);
/* (driving: rato_car_eval_batch, below) */

/*
 * The obstacle metric of an evaluation (ABI 12, additive).  The paper's main figure (drone_main_plot.py) validates with
 * the EUCLIDEAN form of the ellipsoid constraint, g = 1 - sqrt((p-o)' Q (p-o)) (:198-208), where drone_risk.py:170-180
 * uses the quadratic form g = 1 - (p-o)' Q (p-o).  Both have the same sign; the Euclidean one measures the clearance
 * in units of the ellipsoid's radius, which is what the figure's histogram shows.
 *   metric 1: a = (p-o)' Q (p-o) by the instructions of metric 0, then g = 1.0f - sqrtf(fmaxf(a, 0.0f)), nothing
 *             contracted.  (An a that is NaN gives g = 1: fmaxf returns its other operand.)  Z = max g - p->tol as in
 *             rato_drone_eval: the main-plot closure keeps the raw maximum and tests it against OSQP_TOL + 1e-6
 *             (:254-269), i.e. its caller passes tol = 0 and the threshold 1e-3 + 1e-6.
 *   metric 0: every output is, to the bit, that of the entry point without a metric.
 * Any other metric is RATO_EINVAL.
 *   arg   [M] int32 or NULL (rato_drone_eval_batch_metric: [K][ldz])   the row j*S + t of g that attains the sample's
 *         maximum (the obstacle an unsafe sample hit and the step at which it did: drone_main_plot.py:791-800) -- the
 *         first such row in the kernels' loop order (t ascending, then j ascending, strict >); -1 when no row compared
 *         greater than -inf (every row NaN).  A call without arg runs the kernel without the index.
 * Everything else -- the tiled kernel without xs, the plain one with, p->stats_* and RATO_STATS_IN_LAUNCH, the batch
 * form's stats_out -- is as in rato_drone_eval / rato_drone_eval_batch.
 */
#define RATO_DRONE_METRIC_QUADRATIC 0   /* drone_risk.py:170-180 */
#define RATO_DRONE_METRIC_EUCLIDEAN 1   /* drone_main_plot.py:198-208 */
int rato_drone_eval_metric(const rato_drone_params* p, int32_t metric, const float* us, const float* dW,
                           const float* mass, const float* Qsym,
                           float* Z, int32_t* arg, float* xs, float* g, void* stream);
int rato_drone_eval_batch_metric(const rato_drone_params* p, int32_t metric, int32_t K, const float* us, const float* dW,
                                 const float* mass, const float* Qsym, float* Z, int64_t ldz, double alpha, float thr,
                                 void* workspace, size_t workspace_bytes, double* stats_out,
                                 int32_t* arg /* [K][ldz] or NULL */, void* stream);
/* Model.obstacle_avoidance_constraints_euclidean on given trajectories (drone_main_plot.py:198-208) for metric 1, with
 * the arithmetic of the eval kernels' row: on the xs an eval call returned, g equals that call's g to the bit.
 * Metric 0 is rato_drone_obstacle_constraints.    xs [S+1][6][M] -> g [3 obs][S][M] */
int rato_drone_obstacle_constraints_metric(const rato_drone_params* p, int32_t metric, const float* xs,
                                           const float* Qsym, float* g, void* stream);
/* the records of K rows of Z [K][ldz] -> out [K][RATO_N_STATS] (one launch while M <= 12,288) */
int rato_risk_stats_batch(const float* Z, int64_t M, int64_t ldz, int32_t K, double alpha, float thr, void* workspace,
                          size_t workspace_bytes, double* out, void* stream);

/* The records of K rows of Z [K][ldz], row k at its OWN alphas[k] (ABI 12, additive): the K selections behind a batched
 * rollout whatever the alphas of its rows are and whatever M is.  alphas is a DEVICE array of K doubles -- nothing is
 * uploaded, every workgroup ranks its row itself by the host rule (floor(alpha * (double)M), M - that - 1, the wrap to
 * the maximum: IEEE-exact on both sides), and the call can be captured.
 *   M <= 12,288: ONE launch of K workgroups; the workspace is not read (it may be NULL).
 *   beyond:      FIVE stream-ordered launches over (workgroups of a row) x (rows) -- the launch-per-pass form, which waits
 *                for nothing and needs no co-residency -- on K workspaces, one per row
 *                (rato_risk_stats_rows_workspace_bytes; rato_risk_stats_rows_init zeroes and tags every one that fits).
 * Guarantees:
 *   - while M <= 12,288 row k is, to the bit and in all RATO_N_STATS entries, rato_risk_stats(Z_k, M, alphas[k]);
 *   - beyond, row k is, to the bit and in all entries, rato_risk_stats_recover(Z_k, M, alphas[k]): the same workgroups per
 *     row, the same fold, the same bits.  Hence it equals rato_risk_stats exactly in VaR, fraction, max, count, rank,
 *     #{Z > t}, #{Z == t} and t, and to summation order in mean, tail sum and CVaR;
 *   - an alphas[k] outside (0, 1], or NaN, gives row k a NaN record and disturbs no other row; that row's histograms are
 *     left zeroed like every other's.  A workspace that was never initialised gives NaN records in every row;
 *   - nothing is read beyond column M of a row; deterministic run to run (integer atomics, fixed-order fp64 folds).
 * RATO_EINVAL before any launch: Z, alphas or out NULL; K < 1 or K > 65535; M <= 0 or M >= 2^32 - 1; ldz < M; beyond
 * 12,288 a workspace that is NULL or smaller than rato_risk_stats_rows_workspace_bytes(M, K). */
size_t rato_risk_stats_rows_workspace_bytes(int64_t M, int32_t K);   /* K workspaces beyond the one-workgroup form; 0 below */
int rato_risk_stats_rows_init(void* workspace, size_t workspace_bytes, void* stream);
int rato_risk_stats_rows(const float* Z, int64_t M, int64_t ldz, int32_t K, const double* alphas /* device [K] */, float thr,
                         void* workspace, size_t workspace_bytes, double* out /* [K][RATO_N_STATS] */, void* stream);
/* host only, nothing is launched: the number of launches of the call (1 or 5) and the workgroups per row of each
 * (1 in the one-workgroup form; beyond, the single-row rule: 4 elements per thread up to 256 workgroups, then 16, floor
 * 256, cap 1024).  Either pointer may be NULL. */
int rato_risk_stats_rows_plan(int64_t M, int32_t K, int32_t* launches, int32_t* blocks_per_row);

/* ---------------------------------------------------------------- driving */

/* Constants of driving_params.py:1-42 / Model.__init__ driving.py:84-120. */
/* 1 when rato_drone_linearize / rato_car_linearize (row-parallel kernel) with params.stats_* would compute the statistics
 * in its own launch for this batch (small batches), 0 when it would issue rato_risk_stats behind the kernel. */
int rato_drone_stats_in_launch(int32_t M, int32_t S);
int rato_car_stats_in_launch(int32_t M, int32_t S);
/* 1 when the row-parallel linearize kernel would write this batch's Jacobian with streaming (non-temporal) stores: the
 * output is far beyond the 256 MB memory-side cache (>= 256 MB) and the batch's noise fits it (<= 128 MB), so that the
 * noise stays cached from one linearization to the next.  factored: the drone's (Phi, W) output. */
int rato_drone_rows_streaming_stores(int64_t M, int32_t S, int32_t factored);
int rato_car_rows_streaming_stores(int64_t M, int32_t S);
/* The launch the row-parallel linearize kernel would get for a batch (csrc/rato_rows_plan.h holds the rule and describes
 * the three forms): a query, nothing is launched.  cus <= 0: the current device's CU count (256 without a device); with
 * cus > 0 no device is touched.  queue_available 0: the form taken when the work-queue pool hands out no queue.
 * switches: the A/B switches as integers, NULL = what this process read from its environment --
 *   drone   [6] RATO_ROWS_SLOTS_PER_CU, RATO_SMALL_SPLIT, RATO_ROWS_DYNAMIC, RATO_ROWS_QSLOTS, RATO_DYN_TAIL_SPLIT,
 *               RATO_DYN_TAIL_TILES      (unset: 0, 0, 1, 0, 0, 0)
 *   driving [5] RATO_CAR_SLOTS_PER_CU, RATO_CAR_SMALL_SPLIT, RATO_ROWS_DYNAMIC, RATO_CAR_TAIL_SPLIT, RATO_CAR_TAIL_TILES
 *               (unset: 0, -1, 1, 1, -1)
 * RATO_EINVAL where the row-parallel kernel does not apply (M < 1, S < 2, more than 160 KiB of LDS per workgroup). */
#define RATO_ROWS_FORM_SPLIT 0    /* every tile dealt to `split` workgroups */
#define RATO_ROWS_FORM_STATIC 1   /* one tile per workgroup */
#define RATO_ROWS_FORM_QUEUE 2    /* `workgroups` of them take n_whole whole tiles, then the other tiles' `split` parts */
typedef struct rato_rows_plan {
  int32_t n_tiles;       /* ceil(M / 64) */
  int32_t per_cu;        /* resident workgroups per CU */
  int32_t slots;         /* cus * per_cu */
  int32_t qslots;        /* workgroups of the queue form (drone: 0 in the other forms) */
  int32_t wants_queue;   /* the shape takes a queue when one is available */
  int32_t form;          /* RATO_ROWS_FORM_* */
  int32_t split;
  int32_t n_whole;       /* static form: n_tiles (drone), 0 (driving) */
  int32_t workgroups;    /* producer workgroups of the launch (statistics workgroups not counted) */
  int32_t n_units;       /* n_whole + (n_tiles - n_whole) * split */
} rato_rows_plan;
int rato_drone_rows_plan(int32_t M, int32_t S, int32_t factored, int32_t cus, int32_t queue_available,
                         const int32_t* switches, rato_rows_plan* out);
int rato_car_rows_plan(int32_t M, int32_t S, int32_t cus, int32_t queue_available, const int32_t* switches,
                       rato_rows_plan* out);

typedef struct rato_car_params {
  int32_t M;
  int32_t S;
  float dt;
  float beta;            /* 3e-2 */
  float speed_ped_des;   /* 1.3 */
  float d_min;           /* min_separation_distance */
  float tol;             /* OSQP_TOL (3e-4) */
  float ego_init[4];     /* state_init[0:4] (sample independent) */
  float ego_goal[4];     /* driving.py:217-220 */
  int32_t rows_out;      /* g_up buffer of rato_car_linearize*: 0 = g_up = -g + (grad g).u_k (driving.py:295),
                            1 = g itself (see rato_drone_params.rows_out) */
  /* the same constants in double precision, for the entry points that compute in fp64 (rato_car_*_rollout) */
  double dt64, beta64, speed_ped_des64, d_min64;
  double ego_init64[4];
  void* stats_workspace;  /* statistics in the same launch: as rato_drone_params.stats_* */
  double* stats_out;
  double stats_alpha;
  float stats_thr;
  int32_t stats_flags;       /* as rato_drone_params.stats_flags */
} rato_car_params;

/* Scratch floats needed by the driving entry points for the shared ego
 * trajectory and ego sensitivities (sample-independent, recomputed per call). */
size_t rato_car_ego_scratch_floats(int32_t S);

/*
 * Replaces Model.us_to_state_trajectories (driving.py:186-214) fused with
 * separation_distances_at_all_times (:223-236) and
 * monte_carlo_separation_constraints_verification (:630-638).
 *   us      [S][2]
 *   dW      [S][2][M]       rows 6..7 of the reference's DWs (M,S,8)
 *   x0_ped  [4][M]          states_init[:, 4:8]
 *   w_speed [M], w_rep [M]  omegas_speed, omegas_repulsive
 *   ego_scratch             rato_car_ego_scratch_floats(S) floats
 * outputs (any may be NULL):
 *   Z   [M]                 max_t(-distance_t) - tol
 *   xs  [S+1][8][M]
 *   g   [S][M]              -distance_t
 * Without trajectories (xs == NULL) the rollout is ONE launch: every workgroup folds the sample-independent ego trajectory
 * into its own LDS (the arithmetic of the ego prologue, to the bit) and rolls its tiles out (one wave per 64 samples, the
 * noise of 32 steps in flight).  Monte-Carlo step in one call (ABI 11; driving.py:618-740): p->stats_* / stats_flags as
 * for rato_drone_eval.
 */
int rato_car_eval_stats_in_launch(int32_t M);
int rato_car_eval(const rato_car_params* p, const float* us, const float* dW,
                  const float* x0_ped, const float* w_speed, const float* w_rep,
                  float* ego_scratch, float* Z, float* xs, float* g, void* stream);
/* K control sequences in one call: see rato_drone_eval_batch.  us [K][S][2]. */
int rato_car_eval_batch(const rato_car_params* p, int32_t K, const float* us, const float* dW, const float* x0_ped,
                        const float* w_speed, const float* w_rep, float* Z, int64_t ldz, double alpha, float thr,
                        void* workspace, size_t workspace_bytes, double* stats_out, void* stream);

/* Model.separation_distances_at_all_times on GIVEN trajectories (driving.py:223-236):
 *   xs [S+1][8][M] -> dist [S][M] = ||p_ego(t+1) - p_ped(t+1)|| - d_min   (the constraint value is -dist). */
int rato_car_separation_distances(const rato_car_params* p, const float* xs, float* dist, void* stream);

/* Kernel variants of rato_car_linearize: cols_per_thread = -1 row-parallel adjoint kernel (default;
 * needs ~20*64*S bytes of LDS <= 160 KB), 4/8/16 forward column kernel.  Resolves 0 to a concrete
 * value, reports the TILE of the G layout and returns the number of sample blocks (<0: bad arguments). */
int rato_car_linearize_plan(int32_t M, int32_t S, int32_t* cols_per_thread, int32_t* tile);

/*
 * Replaces vmap(Model.get_all_constraints_coeffs) (driving.py:260-307).
 * outputs:
 *   G        [n_tiles][n_pairs][2 controls][TILE]   d g_t / d u[s,i] for s<t
 *   g_up     [S][M]
 *   Z        [M] or NULL
 *   final_du [4][2S]   d x_S[0:4] / d u  (sample independent, so already the mean; :311)
 *   final_rhs[4]       -v_final + v_final_du.u (:288)
 */
int rato_car_linearize(const rato_car_params* p, const float* us, const float* dW,
                       const float* x0_ped, const float* w_speed, const float* w_rep,
                       float* ego_scratch, float* G, float* g_up, float* Z,
                       float* final_du, float* final_rhs,
                       int32_t cols_per_thread, void* stream);

/* ----------------------------------------------------------------- hopper */

/*
 * Replaces the sample-dependent part of Model.slip_risk_constraints
 * (hopper.py:300-367), friction_at_px (:75-81), its Jacobian/Hessian slices
 * (jacrev/hessian at :569,:577-580) and no_slip_constraints_verification
 * (:901-925).  C = number of contact steps ([0,time_jump) U [time_land,S)).
 *   px [C], fx [C], fz [C]        contact inputs gathered as at :305-311
 *   a, theta, tau [30][M]         friction-field features (SoA of (M,30))
 *   lam [C][M] or NULL            multipliers of the slip rows (for the Hessian sums)
 * outputs (any may be NULL):
 *   Z      [M]                    max_c (fx - mu fz)
 *   h      [C][M]                 fx - mu_i(px_c) fz
 *   dh_dfz [C][M]                 -mu_i(px_c)
 *   dh_dpx [C][M]                 -mu_i'(px_c) fz
 *   part_hess [nblocks][C][2]     per-block sums of lam*d2h/(dpx dfz), lam*d2h/dpx^2  (needs 8 C bytes of LDS per
 *                                 sample-wave: C <= 2032 contacts for M < 98,304 samples, 4064 above; RATO_EINVAL beyond)
 */
int rato_hopper_nblocks(int32_t M);
int rato_hopper_slip(int32_t M, int32_t C, const float* px, const float* fx, const float* fz,
                     const float* a, const float* theta, const float* tau, const float* lam,
                     float* Z, float* h, float* dh_dfz, float* dh_dpx, float* part_hess,
                     void* stream);

/* Same computation with px / fx / fz given as HOST arrays -- what the reference's IPOPT callbacks hold at every
 * iterate (hopper.py:305-311).  They are read during the call and travel in the kernel's argument block: no staging
 * buffer and no upload in front of the kernel (the upload was a third of the step at M = 5e4).  C must not exceed
 * RATO_HOPPER_MAX_HOST_CONTACTS (RATO_EINVAL beyond; use rato_hopper_slip with device arrays).  Under stream capture
 * the values are frozen into the captured launch: capture rato_hopper_slip if replays must see new inputs. */
#define RATO_HOPPER_MAX_HOST_CONTACTS 128
int rato_hopper_slip_host_inputs(int32_t M, int32_t C, const float* px_host, const float* fx_host,
                                 const float* fz_host, const float* a, const float* theta, const float* tau,
                                 const float* lam, float* Z, float* h, float* dh_dfz, float* dh_dpx,
                                 float* part_hess, void* stream);

/* rato_hopper_slip / rato_hopper_slip_host_inputs (host_inputs != 0) with THREE per-block sums per contact,
 *   part_hess3 [nblocks][C][3] = lam*d2h/(dpx dfz), lam*d2h/dpx^2, lam*dh/dpx
 * -- everything ``hessian(lambda . g)`` of the reference (hopper.py:575-580) needs from the samples: with the chain factors
 * J_c, H_c of the end-effector map p = x0 + x3 sin x2 (:166-171) the block of contact c on (x0, x2, x3) is
 * D2_c J_c J_c' + D0_c H_c and its mixed entries with fz are D1_c J_c (Model.slip_hessian). */
int rato_hopper_slip_hessian(int32_t M, int32_t C, const float* px, const float* fx, const float* fz,
                             int32_t host_inputs, const float* a, const float* theta, const float* tau,
                             const float* lam, float* Z, float* h, float* dh_dfz, float* dh_dpx, float* part_hess3,
                             void* stream);

/* The script's Monte-Carlo report (hopper.py:960-1007) evaluates K solutions -- the alphas and the baseline, or an alpha x
 * repeat grid -- on ONE set of validation fields: K solutions in one launch, the hopper counterpart of rato_drone_eval_batch.
 * ABI: additive (RATO_ABI_VERSION stays 12).
 *   px, fx, fz [K][ldc] (device, ldc >= C)   the contact inputs of solution k in row k, gathered as for rato_hopper_slip
 *   a, theta, tau [30][M]                    as rato_hopper_slip
 *   Z   [K][ldz] (ldz >= M)                  Z[k][m] = max_c (fx[k][c] - mu_m(px[k][c]) fz[k][c]): row k is, to the bit, the Z
 *                                            that rato_hopper_slip writes for solution k (one device function holds the value
 *                                            arithmetic of both kernels)
 *   arg [K][ldz] int32 or NULL               the smallest c (position in the gathered contact list) whose value equals
 *                                            Z[k][m]: the contact step that slips; -1 when Z[k][m] is -inf (every value NaN).
 *                                            A call without arg runs the kernel without the index.
 *   alphas_host [K] HOST doubles, stats_out [K][RATO_N_STATS] device, or both NULL: row k of stats_out is, to the bit, the
 *                                            rato_risk_stats record of row k of Z at alphas_host[k] (threshold thr; workspace
 *                                            as rato_risk_stats) -- one rato_risk_stats_batch call per run of consecutive
 *                                            equal alphas, i.e. one launch per run while M <= 12,288.
 * Lanes past M and the columns M .. ldz-1 of Z and arg are not written; nothing has to be initialised; no atomics, no
 * workgroup waits for another; the inputs are read through their device pointers at run time (a captured call sees what
 * they hold at replay).  Launch shape: a lane is a sample whose 90 feature registers serve k_chunk solutions x C contacts;
 * grid x = groups of (4 >> nw_log2) sample-waves, y = chunks of k_chunk consecutive solutions (the last may be short); the
 * contacts of a solution are split over 1 << nw_log2 waves of the workgroup and folded through k_chunk KiB of LDS (2 k_chunk
 * with arg) by max, ties to the smaller c.  Z and arg are the same bits under every shape.
 * rato_hopper_eval_batch_plan: the shape the rule picks (host only, no HIP call): about three waves per SIMD where the work
 * allows it, the contact split (never over more waves than contacts) before a k_chunk of 1.
 * rato_hopper_eval_batch_shaped: the same call with the shape forced (nw_log2 in {0, 1, 2}, 1 <= k_chunk <= K; -1 = the
 * rule's value for that argument).
 * RATO_EINVAL without a launch: M, C or K < 1; ldc < C; ldz < M; a NULL px, fx, fz, a, theta, tau or Z; stats_out without
 * alphas_host; an alpha outside (0, 1] (with stats_out); an illegal shape; more than 65535 chunks; a fold that needs more than
 * 160 KiB of LDS. */
int rato_hopper_eval_batch(int32_t M, int32_t C, int32_t K, const float* px, const float* fx, const float* fz, int64_t ldc,
                           const float* a, const float* theta, const float* tau, float* Z, int64_t ldz, int32_t* arg,
                           const double* alphas_host, float thr, void* workspace, size_t workspace_bytes, double* stats_out,
                           void* stream);
int rato_hopper_eval_batch_shaped(int32_t M, int32_t C, int32_t K, const float* px, const float* fx, const float* fz,
                                  int64_t ldc, const float* a, const float* theta, const float* tau, float* Z, int64_t ldz,
                                  int32_t* arg, const double* alphas_host, float thr, void* workspace, size_t workspace_bytes,
                                  double* stats_out, void* stream, int32_t nw_log2, int32_t k_chunk);
int rato_hopper_eval_batch_plan(int32_t M, int32_t C, int32_t K, int32_t* nw_log2, int32_t* k_chunk, int32_t* grid_x,
                                int32_t* grid_y);

/* ``jacrev(slip_risk_constraints)`` (hopper.py:569 on the rows of :300-367) in the reference's own layout: the CSC VALUE
 * array, written on the device from dh_dfz / dh_dpx [C][M] of the calls above.  Rows ('saa', saa != 0; :351-366):
 * 0 = (M alpha) t + sum y; 1 + i = -y_i; 1 + M + i C + c = h_ic - t - y_i - slack; one trailing zero row; ('baseline',
 * :339-348: i C + c = h_ic - slack).  Columns in Z order (:105-132).  Values, columns ascending and rows ascending
 * inside a column:  [c][x0, x2, x3][i] dh_dpx * chain[c][k];  [c][fx, fz][i] 1, dh_dfz;  saa: [i][1, -1, C x -1];
 * slack: M C x -1;  saa: t_risk: M alpha, M C x -1.  rato_hopper_jacobian_nnz values in all (8 C M + 2 M + 1 / 6 C M).
 *   chain_host [C][3] host floats (C <= RATO_HOPPER_MAX_HOST_CONTACTS: kernel arguments) and / or chain_dev (device);
 *   write_constants = 0 skips the constant part (a buffer written once keeps it).
 * Exact zeros (sin x2 = 0) are written as zeros; the reference's csc_matrix(dense) drops them (Model.slip_jacobian does). */
int64_t rato_hopper_jacobian_nnz(int32_t M, int32_t C, int32_t saa);
int rato_hopper_emit_jacobian_values(int32_t M, int32_t C, int32_t saa, double alpha, const float* dh_dfz,
                                     const float* dh_dpx, const float* chain_host, const float* chain_dev,
                                     int32_t write_constants, float* out, void* stream);

/* --------------------------------------------------------------- assembly */

/*
 * Device side of the sparse QP assembly (replaces the dense packing loop of
 * drone_risk.py:339-364 / driving.py:344-363 and the dense->csr scan of :419).
 * Emits the linearized-constraint block of the CSC value array in the
 * reference's order: for s = 0..S-2, for g = 0..n_g-1 (u-column s*n_u + g), for
 * sample i, for row-group r (obstacle), for t = s+1..S-1:
 *     out[...] = scale * d row(r,t) / d u[s,g]
 * i.e. column (s,g) occupies M*R*(S-1-s) consecutive values.  G is the packed
 * tile-blocked Jacobian of the linearize calls (tile = its TILE, n_g = 2,
 * R = 3 drone / 1 driving).  scale = the reference's MULTIPLIER (0.01 drone, 1
 * driving), times 1e-7 while scp_iter < 2 (drone_risk.py:413-415).
 * The transposition is staged through 64 (R (S-1) + 1) floats of LDS: RATO_EINVAL when that exceeds 160 KiB = 163,840 B
 * (S > 214 for the drone, S > 640 for driving; S = 214 / 640 take exactly 163,840 B and are accepted) -- the facades then
 * assemble on the host from the untiled Jacobian
 * (Model.get_constraints_coeffs_host), same pattern and values.
 */
int rato_emit_csc_values(const float* G, const float* W /* NULL, or the factor of a factored G */,
                         int64_t ld /* row stride of W */, int32_t tile, int32_t n_g, int32_t R, int32_t S,
                         int64_t M, float scale, float* out, void* stream);

/* ------------------------------------------- linearized CVaR constraint oracle */

/*
 * Eliminating the auxiliary y_i of the reference's QP (drone_risk.py:327-368:
 * y_i >= -slack, y_i >= (G_i u - g_up_i)_r - t for every row r) leaves the single
 * convex constraint  alpha*M*CVaR_alpha(m(u)) - (M*(1-alpha) - 1)*slack <= 0  with
 *     m_i(u) = max_r [ (G_i u)_r - g_up_{i,r} ].
 * These calls are the device oracle a cutting-plane solve needs per cut (selection of the tail: rato_risk_stats on
 * m; the cut itself: tail-weighted sums of the arg-max rows and of their offsets).  The rows are evaluated as
 *     (G_i x)_r + sign * base_{i,r}
 * which covers the reference's expression (x = u, base = g_up, sign = -1) and its delta form (x = u - u_k,
 * base = g, sign = +1: g_up = -g + G u_k, params.rows_out = 1 makes the linearize kernels write g).  Inputs are the
 * fp32 arrays of the linearize calls; ALL arithmetic is fp64 (x and the partial sums are double): value and gradient
 * of a cut agree to 1e-13, which is what the 1e-5 parity of SCP iterates with the full QP rests on.
 *
 * rato_saa_rowmax: one streaming read of the packed Jacobian G (layout of the
 * linearize calls; tile = its TILE; R = 3 drone / 1 driving; rows of sample i
 * indexed r*S + t):  m_out[i], arg_out[i] = max (rounded to fp32) / arg-max (smallest row index on ties).
 *   base [R][S][ld], xs [S][n_u] doubles (only controls 0 and 1 enter the rows).
 */
int rato_saa_rowmax(const float* G, const float* W /* NULL, or the factor of a factored G (R = 3) */,
                    int32_t tile, int32_t R, int32_t S, int64_t M, int64_t ld,
                    const float* base, double sign /* +1 or -1 */, const double* xs, int32_t n_u,
                    float* m_out, int32_t* arg_out, void* stream);

/*
 * The same m_out / arg_out for the drone WITHOUT reading the Jacobian: (G_i x)_{j,t} =
 * sum_a W[j,t,a] dp_a(t+1), where dp is the response of the linearized dynamics
 * d x_{k+1} = A_k d x_k + B x_k (d x_0 = 0, B = [0, dt/m]^T, A_k from A22: see rato_drone_linearize).
 * One pass over A22, W, base (11 S floats per sample instead of S(S-1) + 9 S).  xs [S][3] doubles (n_u = 3);
 * p supplies M, ld, S, dt, kp.
 */
int rato_drone_rowmax_implicit(const rato_drone_params* p, const float* mass, const float* A22,
                               int32_t a22_axes /* 2: [S][2][ld] of rato_drone_linearize (a22); 3: [S][3][ld] of
                                                   rato_drone_linearize_generators (1 - a22) */,
                               const float* W, const float* base, double sign, const double* xs,
                               float* m_out, int32_t* arg_out, void* stream);

/*
 * Generators-only linearization (drone): A22 [S][3 axes][ld] -- holding the COMPLEMENT 1 - a22 = dt (k_d + 2 c_d |v|) / m
 * (~1e-3: as an fp32 number it is exact to 1e-10 of a22; the consumers below rebuild a22 in fp64; the [S][2][ld] table
 * of rato_drone_linearize holds a22 itself, and a22_axes tells the two apart) --, W [3 obs][S][2][ld], g_up [3 obs][S][ld] (or g:
 * p->rows_out), Z [M] or NULL, part [ceil(M/256)][6S+6] (per-block sums, layout of rato_drone_linearize) -- the whole
 * linearization in 12 S numbers per sample and NO Jacobian entries: Phi[t,s,a] = e_0' A_t ... A_{s+1} B is
 * regenerated from A22 by the consumers (rato_drone_rowmax_implicit for G.x, rato_drone_tail_rows_implicit for rows
 * of G).  60 B per sample-step of HBM traffic instead of 245 B; what a reduced SCP iteration needs
 * (Model.solve_reduced).  W and g_up may both be NULL (a caller whose cut oracle re-runs the rollout --
 * rato_drone_*_rollout -- needs only the sample sums; A22 stays: it is the lane's scratch for the final-state adjoint).
 */
int rato_drone_linearize_generators(const rato_drone_params* p, const float* us, const float* dW,
                                    const float* mass, const float* Qsym,
                                    float* A22, float* W, float* g_up, float* Z, float* part, void* stream);

/*
 * Cuts under a linearization (the new cut of an oracle call, and cut recycling across SCP iterations).  A cut is a
 * tail weighting w (from the m values and the rato_risk_stats record that was computed on them: 1 above the
 * threshold out[10], lambda = clamp((alphaM - #{m > t}) / #{m == t}, 0, 1) on ties) plus the arg-max row of every
 * sample; it is a valid cut under ANY linearization,
 *     CVaR(m(x)) >= (1/(alpha M)) sum_i w_i [(G_i x)_{r_i} + sign base_{i,r_i}],
 * tight at the x it was computed for under the linearization it was computed with.
 * lambda is formed in fp64 from the record and then carried as a FLOAT, in every tail-rows form and in rato_kkt_sums
 * (the products and sums are fp64): a sum differs from the fp64 rule by at most |float(lambda) - lambda| sum_ties |entry|
 * <= 2^-24 lambda sum_ties |entry| -- nothing where lambda is 0, 1 or dyadic (tests/test_gpu_cut_tails.py holds the
 * kernels to that term).
 * K cuts kept in rings  m_base [slot][M], arg_base [slot][M], stats_base [slot][stats_stride >= 11 doubles]  are
 * evaluated in one launch (slots: device array of K ring slots; NULL: K = 1, the pointers are the slot):
 *   part[blk][k][0 .. 2(S-1))  block sums of w_i G_i[r_i, (s,g)]      (doubles)
 *   part[blk][k][2(S-1)]       block sum  of w_i base_{i,r_i}
 * Reduce with rato_sum_partials_f64(part, nblk, K * (2(S-1) + 1), ...).
 */
int rato_saa_tail_rows_batch(const float* G, const float* W /* NULL or factor */, int64_t ld, int32_t tile,
                             int32_t R, int32_t S, int64_t M, const float* base,
                             const float* m_base, const int32_t* arg_base, const double* stats_base,
                             int64_t stats_stride, const int32_t* slots, int32_t K, double alphaM, double* part,
                             void* stream);

/*
 * The same for the drone without reading the Jacobian: the arg-max row of every tail sample is regenerated from A22
 * (adjoint sweep from its t*, fp64).  Same part layout.
 */
int rato_drone_tail_rows_implicit(const rato_drone_params* p, const float* mass, const float* A22, int32_t a22_axes,
                                  const float* W, const float* base,
                                  const float* m_base, const int32_t* arg_base, const double* stats_base,
                                  int64_t stats_stride, const int32_t* slots, int32_t K, double alphaM,
                                  double* part, void* stream);

/*
 * Table-free ("rollout") form of the drone oracle, delta form only:  rows(u) = g(u_k) + grad g(u_k) . (u - u_k).
 * Instead of reading what a linearize call stored of the rollout at u_k in fp32 (A22, W, g: 44 S bytes per sample, each
 * number rounded to 6e-8 of its own magnitude), these two calls RE-RUN that rollout in fp64 from the samples themselves
 * (dW rows of the two horizontal axes, mass, Qsym: 8 S + 40 bytes per sample) while they propagate the response to
 * xs = u - u_k (rowmax) / the adjoint of the arg-max rows (tail rows): 5 x less HBM traffic, and nothing of the fp32
 * device path is left in the rows but the rounding of its inputs.  uk, xs: doubles [S][3].  Outputs as
 * rato_drone_rowmax_implicit / rato_drone_tail_rows_implicit (the offset sum is sum_i w_i g_{i,r_i}: sign = +1).
 */
int rato_drone_rowmax_rollout(const rato_drone_params* p, const double* uk, const float* dW, const float* mass,
                              const float* Qsym, const double* xs, float* m_out, int32_t* arg_out, void* stream);
int rato_drone_tail_rows_rollout(const rato_drone_params* p, const double* uk, const float* dW, const float* mass,
                                 const float* Qsym, const float* m_base, const int32_t* arg_base,
                                 const double* stats_base, int64_t stats_stride, const int32_t* slots, int32_t K,
                                 double alphaM, double* part, void* stream);

/*
 * The same for the driving problem (R = 1 row per step: g_t = -(|p_ego(t+1) - p_ped(t+1)| - d_min), driving.py:223-230,
 * :260-313).  The ego trajectory at u_k, its tangent along xs and the tables of the adjoint are sample independent: every
 * workgroup folds them in fp64 from uk / xs (doubles [S][2]); the pedestrian is re-rolled per sample from dW [S][2][M],
 * x0_ped [4][M], w_speed [M], w_rep [M] (8 S + 24 bytes per sample against the 6240 of the packed Jacobian at S = 40).
 * m_out / arg_out, part layout and reduction as above (2(S-1) gradient sums: u_s enters g_t for s <= t - 1).
 */
int rato_car_rowmax_rollout(const rato_car_params* p, const double* uk, const float* dW, const float* x0_ped,
                            const float* w_speed, const float* w_rep, const double* xs, float* m_out,
                            int32_t* arg_out, void* stream);
int rato_car_tail_rows_rollout(const rato_car_params* p, const double* uk, const float* dW, const float* x0_ped,
                               const float* w_speed, const float* w_rep, const float* m_base, const int32_t* arg_base,
                               const double* stats_base, int64_t stats_stride, const int32_t* slots, int32_t K,
                               double alphaM, double* part, void* stream);

/*
 * One oracle round trip of a cutting-plane solve in ONE call (table-free forms; system 0 = drone: s0..s2 = dW, mass,
 * Qsym, s3 unused; 1 = driving: s0..s3 = dW, x0_ped, w_speed, w_rep):
 *   x_host [S][n_u] doubles (pinned for an asynchronous copy) -> x_dev;  m_out / arg_out = rato_*_rowmax_rollout;
 *   res_dev[0..11) = rato_risk_stats(m_out, alpha, thr);  S > 1: part_dev = rato_*_tail_rows_rollout (K = 1, record =
 *   res_dev, stride 11 + nc), res_dev[11..11+nc) = its column sums, nc = 2(S-1) + 1;  res_dev -> res_host (PINNED,
 *   device-visible host memory: the last launch writes it directly, no copy node follows);  the call RETURNS WHEN THE
 *   RECORD HAS ARRIVED in res_host (see the conventions at the top: res_host is pre-set and watched; RATO_CUT_POLL=0:
 *   hipStreamSynchronize).  Replaces two copies, four calls and a synchronize of the host loop
 *   (drone_risk.py:425-469 hands the whole QP to OSQP; here every cut of the reduced subproblem is one such trip).
 */
int rato_cut_oracle_rollout(int32_t system, const void* params, const double* uk, const float* s0, const float* s1,
                            const float* s2, const float* s3, const double* x_host, double* x_dev, float* m_out,
                            int32_t* arg_out, double alpha, float thr, double alphaM, void* workspace,
                            size_t workspace_bytes, double* res_dev, double* part_dev, double* res_host, void* stream);

/*
 * Sums of the matrix-free KKT certificate of a reduced solution against the reference's full QP (drone_risk.py:327-368,
 * driving.py:330-373; riskaversetrajopt_amd/certificate.py): m_star [M] = the m values at the solution (a rowmax call),
 * cut k < K = ring slot slots[k] of (m_base, stats_base) with multiplier lam[k] (device doubles), v = t_risk - slack.
 * part [ceil(M/256)][2K + 2] doubles per block:  [k] sum_i w_ki (m_i* - v)^+;  [K + k] sum_i w_ki;  [2K] sum_i (m_i* - v)^+;
 * [2K + 1] max_i sum_k lam_k w_ki  (w_k: the tail weighting of cut k, as in rato_saa_tail_rows_batch).
 */
int rato_kkt_sums(const float* m_star, int64_t M, const float* m_base, const double* stats_base, int64_t stats_stride,
                  const int32_t* slots, const double* lam, int32_t K, double alphaM, double v, double* part, void* stream);

/* ------------------------------------------------- the cutting-plane loop of one SCP subproblem (host, csrc/cutloop.hip)
 *
 * The reference hands every SCP subproblem to OSQP (drone_risk.py:425-469, driving.py:423-456).  Here the subproblem is
 * that QP reduced exactly to (u, slack) and solved by Kelley cuts on the linearized CVaR constraint: master QP on the
 * host (rato_master_*), cut oracle on the device (rato_cut_oracle_rollout, the table-free forms).  rato_cut_solve is
 * that whole loop -- master, lazily entering control bounds, "the last evaluated cut joins the master", the keep rule
 * for cuts recycled into the next subproblem, the multipliers -- as ONE call (statement for statement the loop of
 * riskaversetrajopt_amd/cvar_cuts.py::CvarCutSolver._solve, which remains for sharded batches and the table forms; both
 * produce bitwise the same iterates).
 *
 * rato_cut_config: sizes, constants and the CALLER-OWNED buffers of a solver (nothing is allocated on the device here):
 *   system 0 drone (n_u 3, params = rato_drone_params*, s0..s2 = dW, mass, Qsym), 1 driving (n_u 2, rato_car_params*,
 *   s0..s3 = dW, x0_ped, w_speed, w_rep); params is copied.  nU = n_u S, n = nU + 1 (u, slack), nc = 2(S-1) + 1,
 *   nres = RATO_N_STATS + nc, nblk = ceil(M / 256).
 *   device: uk_dev, x_dev [nU] doubles; ring_m [cap][M] floats, ring_arg [cap][M] int32, ring_res [cap][nres] doubles
 *   (slot cap-1 is scratch); workspace of rato_risk_stats (initialised); part [nblk][nc], part_b [nblk][keep_max nc]
 *   doubles; slots_dev [keep_max] int32.
 *   pinned host (device-visible: the reductions write into them directly): uk_host, x_host [nU], res_host [nres],
 *   sums_b_host [keep_max nc] doubles, slots_host [keep_max] int32.
 *   p_diag, q [n]: the objective 1/2 z' diag(p_diag) z + q' z (copied).
 *   mode_saa 1: CVaR_alpha(m(u)) - c_s slack <= rhs0 with the row -slack <= 0; 0 ('baseline'): max_i m_i(u) <= rhs0.
 */
typedef struct {
  int32_t system, S, cap, keep_max, keep_recent, keep_idle, mode_saa, recycle;
  int64_t M;
  double alpha, alphaM, c_s, rhs0, u_min, u_max;
  float thr;
  const void* params;
  const float *s0, *s1, *s2, *s3;
  double *uk_dev, *uk_host, *x_host, *x_dev;
  float* ring_m;
  int32_t* ring_arg;
  double* ring_res;
  void* workspace;
  size_t workspace_bytes;
  double *part, *part_b, *sums_b_host;
  int32_t *slots_dev, *slots_host;
  double* res_host;
  const double *p_diag, *q;
} rato_cut_config;

/* What a solve returns.  Caller-provided arrays: us [nU]; cut_slot / cut_lambda [cut_capacity] (ring slot and
 * multiplier of every cut row of the last master: the data of a KKT certificate against the full QP); bound_var /
 * bound_sign / bound_lambda [bound_capacity] (the control bounds that entered: variable, +1 upper / -1 lower,
 * multiplier).  status 0 solved, 1 maximum cuts reached, 2 solved: the last cut no longer moved the master's solution
 * (violation <= 1e-7, step <= 1e-10: what is left is the accuracy of the master's own NNLS). */
typedef struct {
  double* us;
  double slack, t_risk, phi, oracle_s, master_s, lam_slack;
  int32_t cuts, recycled, status, uncertified_cuts;
  int32_t* cut_slot;
  double* cut_lambda;
  int32_t cut_capacity, n_cut_rows;
  int32_t* bound_var;
  double* bound_sign;
  double* bound_lambda;
  int32_t bound_capacity, n_bounds;
} rato_cut_result;

typedef struct rato_cut_solver rato_cut_solver;
int rato_cut_solver_create(rato_cut_solver** out, const rato_cut_config* cfg);
void rato_cut_solver_destroy(rato_cut_solver* s);
size_t rato_cut_config_bytes(void); /* sizeof the two structs as this library was built: a binding checks its layout */
size_t rato_cut_result_bytes(void);

/* Stream-ordered prologue of a subproblem, NO synchronisation: u_lin [nU] (host) -> uk_dev; for the n_keep ring slots
 * kept from the previous subproblem, their tail-row sums under the new linearization point, reduced into sums_b_host. */
int rato_cut_begin(rato_cut_solver* s, const double* u_lin, const int32_t* keep, int32_t n_keep, void* stream);

/* The "define" half of a reduced SCP iteration of the drone (system 0) as one call: us [S][3] doubles (host) -> us_dev
 * (through the pinned us_host), rato_drone_linearize_generators at them without tables (A22 [S][3][ld]: kernel scratch;
 * Z [z_floats >= M] or NULL; part [ceil(M/256)][6S+6]), the sample sums reduced straight into sums_host (pinned, 6S+6 doubles),
 * the non-finite count of Z and part (bad_dev / bad_host pinned, or both NULL), rato_cut_begin(us, keep, n_keep).  WAITS
 * for the sample sums only (watched in sums_host; with the non-finite count: an event behind the count's copy): the kept
 * cuts' sums may still be in flight when it returns -- follow with rato_cut_solve(kept_in_flight = 1), which builds the
 * master first and then waits for them (or synchronise the stream yourself before reading sums_b_host).
 * RATO_ENONFINITE when the count is not zero. */
int rato_cut_define_drone(rato_cut_solver* s, const double* us, float* us_host, float* us_dev, float* A22, float* Z,
                          int64_t z_floats, float* part, double* sums_host, uint32_t* bad_dev, uint32_t* bad_host,
                          const int32_t* keep, int32_t n_keep, void* stream);

/* The loop.  final_du (n_c x nU, row-major), final_rhs (n_c): the equality rows;  u_lin: the linearization point (the
 * one given to rato_cut_begin);  with_cvar 0: the reference's relaxed first iterations (no CVaR rows: one master solve);
 * tol: a cut is added while CVaR - c_s slack - rhs0 > tol, at most max_cuts; a last cut with violation in
 * (final_cut_above, tol] still joins the master, which is solved once more.  keep / keep_idle_count [keep_max] and
 * *n_keep_io: in -- the slots kept from the previous subproblem (+ for how many solves each has carried no multiplier);
 * out -- the same for the next one.  kept_in_flight 1: rato_cut_begin was called for these slots on this stream.
 * SYNCHRONISES the stream (every oracle round trip is read by the host master).  Returns RATO_OK, RATO_ERANK,
 * RATO_EINFEASIBLE, RATO_ENNLS, RATO_ESELECT, RATO_ENONFINITE (check_finite: an oracle call saw non-finite m values). */
int rato_cut_solve(rato_cut_solver* s, const double* final_du, const double* final_rhs, int32_t n_c, const double* u_lin,
                   int32_t with_cvar, double tol, int32_t max_cuts, double final_cut_above, int32_t check_finite,
                   int32_t* keep, int32_t* keep_idle_count, int32_t* n_keep_io, int32_t kept_in_flight,
                   rato_cut_result* out, void* stream);

/* The reduced SCP of the drone as ONE call (drone_risk.py:519-532 with the timing protocol of drone_times.py:509-550):
 * `iters` iterations of [rato_cut_define_drone at the current controls -> equality rows from the sample sums ->
 * rato_cut_solve], starting from us0 [S][3]; iteration k < first_cvar runs without the CVaR rows (:413-417).  Every
 * iteration is timed from its first instruction to the moment its solution is on the host; the stream is synchronised
 * once, inside the last iteration's clock.  us_hist [iters][S][3] and rec [iters] (host) receive every iteration's
 * solution and record; the define's buffers are those of rato_cut_define_drone (no Z, no non-finite scan: check_finite
 * tests the sample sums and the oracle's m values); keep / keep_idle_count / n_keep_io as for rato_cut_solve.  Returns the
 * first non-OK status (RATO_ERANK / RATO_ESELECT: repeat with the per-iteration calls), *done = iterations completed. */
typedef struct rato_scp_iter {
  double define_s, solve_s, oracle_s, master_s; /* solve = oracle round trips + master; define = the rest of the iteration */
  double t_risk, slack, phi;
  int32_t cuts, status, recycled, reserved;
} rato_scp_iter;
size_t rato_scp_iter_bytes(void);
int rato_scp_run_drone(rato_cut_solver* s, const double* us0, int32_t iters, int32_t first_cvar, double tol,
                       int32_t max_cuts, double final_cut_above, int32_t check_finite, float* us_host, float* us_dev,
                       float* A22, float* part, double* sums_host, int32_t* keep, int32_t* keep_idle_count,
                       int32_t* n_keep_io, double* us_hist, rato_scp_iter* rec, int32_t* done, void* stream);

/* The final-state rows of the ego (driving.py:283-288) on the host, in fp64: the ego carries no noise, so they are sample
 * independent and the driving problem's "define" needs no device linearization.  us [S][2] (host), goal [4] (the ego's goal
 * position, speed and heading) -> final_du [4][2S], final_rhs [4] = -(x_S - goal) + final_du . u.  p->ego_init64 and
 * p->dt64 are the inputs.  Sequential sums in ascending k and libm's sincos, compiled without contraction: a pure function
 * of its inputs, shared by rato_scp_run_car, rato_scp_batch_run_car and their per-iteration checker. */
int rato_car_ego_final_rows(const rato_car_params* p, const double* us /* [S][2] */, const double* goal /* [4] */,
                            double* final_du /* [4][2S] */, double* final_rhs /* [4] */);

/* The reduced SCP of the driving problem as ONE call (driving.py:486-513), modelled on rato_scp_run_drone: `iters` iterations
 * of [rato_car_ego_final_rows at the current controls -> rato_cut_begin -> rato_cut_solve with the 4 equality rows],
 * starting from us0 [S][2]; iteration k < first_cvar runs without the CVaR rows (1: driving.py:411-415).  Clocks, records
 * (us_hist [iters][S][2], rec [iters]), kept cuts and the statuses handed back (RATO_ERANK / RATO_ESELECT; check_finite:
 * RATO_ENONFINITE for non-finite rows or m values) as for rato_scp_run_drone.  RATO_EINVAL unless the solver's system is 1. */
int rato_scp_run_car(rato_cut_solver* s, const double* us0, const double* goal, int32_t iters, int32_t first_cvar, double tol,
                     int32_t max_cuts, double final_cut_above, int32_t check_finite, int32_t* keep, int32_t* keep_idle_count,
                     int32_t* n_keep_io, double* us_hist, rato_scp_iter* rec, int32_t* done, void* stream);

/* The reduced SCP of K problems of ONE system in lockstep (the reference's alpha x repeat grids, drone_risk.py:495-539,
 * driving.py:467-529), each problem a rato_cut_solver of its own (samples, alpha, rings, kept cuts) over ONE shared S, M
 * and parameter struct (all of system 0 with equal rato_drone_params, or all of system 1 with equal rato_car_params;
 * mode_saa 1, S >= 2, equal keep_max and cap, distinct solvers; RATO_EINVAL otherwise).  A drone batch is run by
 * rato_scp_batch_run_drone, a driving batch by rato_scp_batch_run_car (RATO_EINVAL for the other system's batch).  Per SCP iteration: one batched
 * define for every problem still running, then rounds of one batched oracle round trip for every problem still cutting
 * (a constant number of launches per round whatever K is), the masters of a round on up to n_threads host threads.  Every
 * problem's iterates, cut counts, t_risk and kept cuts are bitwise those of rato_scp_run_drone on its solver alone.
 * Nothing is allocated on the device here: rato_scp_batch_bytes gives the sizes of the caller-owned device buffer (aligned
 * to 256 bytes) and PINNED host buffer (device-visible, aligned to 16) that rato_scp_batch_create binds to the batch; the
 * solvers must outlive it.  One stream, one run at a time per batch. */
typedef struct rato_scp_batch rato_scp_batch;
typedef struct rato_scp_batch_iter {
  double define_s;   /* the batched define, up to every problem's sample sums on the host */
  double oracle_s;   /* the batched oracle round trips (staging, launches, read-back) */
  double master_s;   /* the host masters of every round (wall time of the parallel phases) */
  double total_s;    /* the whole iteration */
  int32_t rounds, active, reserved0, reserved1; /* oracle round trips; problems that entered the iteration */
} rato_scp_batch_iter;
size_t rato_scp_batch_iter_bytes(void);
int rato_scp_batch_bytes(rato_cut_solver* const* solvers, int32_t K, size_t* device_bytes, size_t* host_bytes);
int rato_scp_batch_create(rato_scp_batch** out, rato_cut_solver* const* solvers, int32_t K, int32_t n_threads,
                          void* device_buf, size_t device_bytes, void* host_buf, size_t host_bytes);
void rato_scp_batch_destroy(rato_scp_batch* b);
/* `iters` lockstep iterations from us0 [K][S][3] (iteration k < first_cvar without the CVaR rows).  keep /
 * keep_idle_count [K][keep_max] and n_keep [K]: each problem's kept cuts, in and out as for rato_scp_run_drone.  Outputs:
 * us_hist [K][iters][S][3]; rec [K][iters] -- cuts, t_risk, slack, phi, status, recycled per problem, and master_s = that
 * problem's own master time; its define_s / solve_s / oracle_s are NaN (lockstep has no per-problem clock): the clocks
 * are brec [iters], batch-level; status [K]: RATO_OK or the problem's first failure (RATO_ERANK / RATO_ESELECT: repeat it
 * with the per-iteration calls; RATO_ENONFINITE, RATO_EINFEASIBLE, RATO_ENNLS, RATO_EINVAL: failed) -- a failed problem
 * leaves the batch, the others go on; done [K]: iterations each completed; *rounds: batched oracle round trips.
 * Returns RATO_OK unless the device fails (RATO_EHIP - e) or an argument is invalid. */
int rato_scp_batch_run_drone(rato_scp_batch* b, const double* us0, int32_t iters, int32_t first_cvar, double tol,
                             int32_t max_cuts, double final_cut_above, int32_t check_finite, int32_t* keep,
                             int32_t* keep_idle_count, int32_t* n_keep, double* us_hist, rato_scp_iter* rec,
                             rato_scp_batch_iter* brec, int32_t* status, int32_t* done, int32_t* rounds, void* stream);
/* The same for a driving batch: us0 [K][S][2], goal [4] as for rato_scp_run_car, first_cvar 1.  Per SCP iteration the final
 * rows of every problem on the host threads, one copy (u_k, kept slots, kept-cut rows), one kept-cuts launch when any
 * problem keeps cuts, then the rounds.  Every problem's iterates are bitwise those of rato_scp_run_car on its solver alone. */
int rato_scp_batch_run_car(rato_scp_batch* b, const double* us0, const double* goal, int32_t iters, int32_t first_cvar,
                           double tol, int32_t max_cuts, double final_cut_above, int32_t check_finite, int32_t* keep,
                           int32_t* keep_idle_count, int32_t* n_keep, double* us_hist, rato_scp_iter* rec,
                           rato_scp_batch_iter* brec, int32_t* status, int32_t* done, int32_t* rounds, void* stream);

/* ------------------------------------------------------------ device sampler */

/*
 * Device-side sampler: Philox4x32-10 (Salmon et al., SC'11), counter = (sample m, step / row t, stream
 * id), key = seed; 24-bit uniforms, Box-Muller normals (csrc/philox.h).  The value at (seed, stream, t, m) is a pure
 * function of those numbers: the same batch can be MATERIALISED (rato_*_sample) or REGENERATED inside the rollout
 * kernels (rato_*_eval_philox), bit for bit.  These replace, for synthetic / Monte-Carlo batches that never leave
 * HBM, the host loops of drone_utils.py:61-93, driving.py:84-120, hopper.py:70-74 (same distributions; the host
 * samplers of the Python facades replay the reference's MT19937 stream when identical draws are wanted).
 *
 * Generic fills, layout out[T][C][ld] (C <= 4 values per Philox call), used by the tests and as utilities:
 *   rato_philox_u32      the raw 4 words            out[t][0..3][m]
 *   rato_philox_normal   scale[k] * N(0,1) + mean[k]           (scale / mean: HOST float[C], NULL = 1 / 0)
 *   rato_philox_uniform  low[k] + width[k] * U(0,1)
 */
int rato_philox_u32(uint32_t* out, int32_t T, int64_t M, int64_t ld, uint64_t seed, uint32_t stream_id, void* stream);
int rato_philox_normal(float* out, int32_t T, int32_t C, int64_t M, int64_t ld, uint64_t seed, uint32_t stream_id,
                       const float* scale, const float* mean, void* stream);
int rato_philox_uniform(float* out, int32_t T, int32_t C, int64_t M, int64_t ld, uint64_t seed, uint32_t stream_id,
                        const float* width, const float* low, void* stream);

/* drone_utils.py:61-93: dW [S][3][ld] = sqrt(sampler_dt) N(0,1) (velocity rows), mass [ld] ~ U(nom -+ delta),
 * Qsym [3][3][ld] from semi-axes obs_radii[j] + U(-+ obs_radii_delta) per dimension (HOST float[3]).  dW may be NULL
 * (noise regenerated in rato_drone_eval_philox); mass and Qsym may both be NULL. */
int rato_drone_sample(int64_t M, int64_t ld, int32_t S, float sampler_dt, uint64_t seed, float mass_nom,
                      float mass_delta, const float* obs_radii, float obs_radii_delta, float* dW, float* mass,
                      float* Qsym, void* stream);
/* rato_drone_eval with the noise of rato_drone_sample(seed, sampler_dt) regenerated in the kernel (no dW array). */
int rato_drone_eval_philox(const rato_drone_params* p, const float* us, uint64_t seed, float sampler_dt,
                           const float* mass, const float* Qsym, float* Z, float* xs, float* g, void* stream);
/* rato_drone_linearize (row-parallel kernel, cols_per_thread = -1: S <= 126) with the noise of
 * rato_drone_sample(seed, sampler_dt) regenerated while a tile is staged: bit for bit the outputs of rato_drone_linearize
 * on the materialised dW, without the array and without its reads in the middle of the store stream (the reads are
 * 2 % of the bytes of the products output but cost 3-8 % of the kernel's time: DESIGN.md 4.1). */
int rato_drone_linearize_philox(const rato_drone_params* p, const float* us, uint64_t seed, float sampler_dt,
                                const float* mass, const float* Qsym, float* G, float* W, float* A22, float* g_up,
                                float* Z, float* part, void* stream);

/* The row-parallel kernels read a tile's noise while the tiles of other workgroups are being stored, and reads beside a
 * saturated store stream cost more than their bytes (the noise regenerated in the kernel: -7 % at the metric
 * configuration).  A batch that is linearized again and again is re-tiled ONCE, so that a tile's 3S rows are one
 * contiguous block instead of 3S rows of 256 B that lie ld floats apart:
 *   rato_drone_tiled_noise_floats(M, S)              floats of the tiled copy: ceil(M / 64) * 3S * 64
 *   rato_drone_tile_noise(dW, M, ld, S, dW_tiled)    dW [S][3][ld] -> dW_tiled [ceil(M/64)] blocks of 3S * 64 floats, each the
 *                                                    image the kernel keeps in LDS: [S][64] (xi_x, xi_y) pairs, then [S][64]
 *                                                    xi_z (lanes beyond M: 0)
 *   rato_drone_linearize_tiled(...)                  rato_drone_linearize(cols_per_thread = -1) reading dW_tiled: the
 *                                                    same outputs, bit for bit (see also rato_car_linearize_tiled) */
size_t rato_drone_tiled_noise_floats(int64_t M, int32_t S);
int rato_drone_tile_noise(const float* dW, int64_t M, int64_t ld, int32_t S, float* dW_tiled, void* stream);
int rato_drone_linearize_tiled(const rato_drone_params* p, const float* us, const float* dW_tiled, const float* mass,
                               const float* Qsym, float* G, float* W, float* A22, float* g_up, float* Z, float* part,
                               void* stream);

/* driving.py:84-120: dW [S][2][M], x0_ped [4][M] = x0_mean + x0_std * N(0,1) (HOST float[4] each), w_speed, w_rep [M]
 * ~ U(nom -+ del).  dW may be NULL; the three parameter arrays may all be NULL. */
int rato_car_sample(int64_t M, int32_t S, float sampler_dt, uint64_t seed, float w_speed_nom, float w_speed_del,
                    float w_rep_nom, float w_rep_del, const float* x0_mean, const float* x0_std, float* dW,
                    float* x0_ped, float* w_speed, float* w_rep, void* stream);
int rato_car_eval_philox(const rato_car_params* p, const float* us, uint64_t seed, float sampler_dt,
                         const float* x0_ped, const float* w_speed, const float* w_rep, float* ego_scratch, float* Z,
                         float* xs, float* g, void* stream);
/* rato_car_linearize (row-parallel kernel, cols_per_thread = -1) with the noise of rato_car_sample(seed, sampler_dt)
 * regenerated while a tile is staged: bit for bit the outputs of rato_car_linearize on the materialised dW. */
int rato_car_linearize_philox(const rato_car_params* p, const float* us, uint64_t seed, float sampler_dt,
                              const float* x0_ped, const float* w_speed, const float* w_rep, float* ego_scratch,
                              float* G, float* g_up, float* Z, float* final_du, float* final_rhs, void* stream);

/* The row-parallel driving kernel reads a tile's noise -- 2S rows of 64 samples -- while the tiles of other workgroups are
 * being stored; as 2S rows of 256 B that lie M floats apart these reads cost the launch 6-11 % (5 % more bytes; reads and
 * writes share the HBM bus), as ONE contiguous block per tile a third less.  A batch that is linearized
 * again and again (every SCP iteration) is therefore re-tiled ONCE:
 *   rato_car_tiled_noise_floats(M, S)           floats of the tiled copy: ceil(M / 64) * 2S * 64
 *   rato_car_tile_noise(dW, M, S, dW_tiled)     dW [S][2][M] -> dW_tiled [ceil(M/64)] blocks of 2S * 64 floats, each the image
 *                                               the kernel keeps in LDS: [S][64] (xi_0, xi_1) pairs (lanes beyond M: 0)
 *   rato_car_linearize_tiled(...)               rato_car_linearize(cols_per_thread = -1) reading dW_tiled: the same
 *                                               outputs, bit for bit */
size_t rato_car_tiled_noise_floats(int64_t M, int32_t S);
int rato_car_tile_noise(const float* dW, int64_t M, int32_t S, float* dW_tiled, void* stream);
int rato_car_linearize_tiled(const rato_car_params* p, const float* us, const float* dW_tiled, const float* x0_ped,
                             const float* w_speed, const float* w_rep, float* ego_scratch, float* G, float* g_up, float* Z,
                             float* final_du, float* final_rhs, void* stream);

/* hopper.py:70-74: a = 0.025 sqrt(2/30) U(0,1), theta = pi U(0,1), tau = 2 pi U(0,1), each [30][M]. */
int rato_hopper_sample(int64_t M, uint64_t seed, float* a, float* theta, float* tau, void* stream);

/* ---------------------------------------------------------------- multi-GPU */

/*
 * The path shards over samples; the only exchange of an evaluation is ONE all-gather (RCCL) of each rank's record
 *   [ fp64 partial sums (n_sums) | fp32 Z row (>= M_local floats) ]      (rec_bytes each, a multiple of 8).
 * rato_unpack_records turns the gathered buffer (world records) into  Z_all [world * M_local]  (rank order) and
 * total [n_sums] = the partial sums added in rank order (bitwise identical on every rank), in one launch.
 */
int rato_unpack_records(const void* all, int32_t world, int32_t n_sums, int64_t M_local, int64_t rec_bytes,
                        double* total, float* Z_all, void* stream);

/*
 * The collective itself (saa_comm_init / exchange / destroy).  The reference is one process
 * (drone_risk.py:18); with the sample axis sharded over one process per GPU, the mean of drone_risk.py:294-296 and the
 * statistics of :663-695 / drone_main_plot.py:640-652 need every rank's record.  RCCL (librccl, bound at run time)
 * over xGMI; one communicator per (process, GPU); the caller selects the device (hipSetDevice) before rato_comm_init.
 *   rato_comm_unique_id   rank 0 only: 128 opaque bytes (ncclUniqueId) that the host ships to the other ranks by
 *                         any means it has (the Python facade: one torch.distributed broadcast)
 *   rato_comm_init        collective over all `world` ranks; *comm is the opaque handle
 *   rato_comm_allgather   stream-ordered all-gather of `bytes` bytes per rank into recv_all [world * bytes]
 *   rato_comm_exchange    the whole exchange of an evaluation: all-gather of the record + rato_unpack_records
 *   rato_comm_destroy     collective teardown
 * Errors: RATO_ENOCOMM (no librccl), RATO_ERCCL - ncclResult_t.
 */
#define RATO_COMM_ID_BYTES 128
typedef struct rato_comm rato_comm;
/* RATO_OK if librccl can be bound in this process, RATO_ENOCOMM otherwise: local and cheap, no communication.  Ranks
 * agree on it BEFORE any of them enters the collective rato_comm_init (a rank that cannot bind the library would
 * return at once and leave the others blocked inside ncclCommInitRank). */
int rato_comm_available(void);
int rato_comm_unique_id(void* id_out /* host, RATO_COMM_ID_BYTES */);
int rato_comm_init(rato_comm** comm, const void* id_bytes /* host */, int32_t rank, int32_t world);
int rato_comm_world(const rato_comm* comm);
int rato_comm_rank(const rato_comm* comm);
int rato_comm_allgather(rato_comm* comm, const void* send, void* recv_all, int64_t bytes, void* stream);
int rato_comm_exchange(rato_comm* comm, const void* record, void* all, int64_t rec_bytes, int32_t n_sums,
                       int64_t M_local, double* total, float* Z_all, void* stream);
int rato_comm_destroy(rato_comm* comm);

/* ----------------------------------------------------- host: the master QP */

/*
 * HOST function (no device work): Lawson-Hanson non-negative least squares  min |A y - b|, y >= 0  started from a
 * guess of the passive set, with an incrementally updated QR of the passive columns (csrc/nnls.hip).  It is the inner
 * solver of the cutting-plane master QP (riskaversetrajopt_amd/dense_qp.py) -- the counterpart of the C solver the
 * reference hands its subproblem to (osqp, drone_risk.py:433-457).  A: m x n COLUMN-major; passive: n bytes in/out;
 * y: n doubles out; maxiter <= 0: 3 n + 10.  Returns 1 converged (KKT test of the original algorithm), 0 not, < 0 bad
 * arguments.
 */
int rato_nnls_warm(const double* A, int32_t m, int32_t n, const double* b, uint8_t* passive, double* y,
                   int32_t maxiter);

/*
 * The master QP of the cutting-plane loop as an object that lives across the cuts of one SCP subproblem (host code,
 * csrc/master.hip):   min 1/2 z'Pz + q'z   s.t.  A_eq z = b_eq,  rows_j . z <= rhs_j  (rows appended one at a time),
 * P = diag(p_diag) > 0, A_eq (m_eq x n, row-major) of full row rank (RATO_EINVAL otherwise: the Python facade then takes
 * its general NumPy path).  Equalities are eliminated and the Hessian whitened once, in O(n m_eq^2); a row costs
 * O(n m_eq); a solve is one warm-started rato_nnls_warm on the rows so far.
 *   rato_master_solve -> 1: z (n doubles) and lam (one multiplier >= 0 per row);  0: NNLS did not converge;
 *                        RATO_EINFEASIBLE.
 * A row that vanishes in the null space of the equalities (a combination of rows of A_eq, or all zero) is constant on the
 * feasible set and is decided when it is added: it holds (multiplier 0) or every later solve returns RATO_EINFEASIBLE.
 */
typedef struct rato_master rato_master;
int rato_master_create(rato_master** out, int32_t n, const double* p_diag, const double* q, int32_t m_eq,
                       const double* A_eq, const double* b_eq);
int rato_master_add_rows(rato_master* m, int32_t k, const double* A /* k x n, row-major */, const double* b);
int rato_master_solve(rato_master* m, double* z, double* lam);
int32_t rato_master_rows(const rato_master* m);
void rato_master_destroy(rato_master* m);

/* ------------------------------------------------------------- statistics */

/* Deterministic second stage of the sample mean (drone_risk.py:294-296,
 * driving.py:311-313): out[c] = scale * sum_b part[b][c], accumulated in fp64
 * in a fixed order.  out is double[ncols]. */
int rato_sum_partials(const float* part, int32_t nblocks, int32_t ncols, double scale,
                      double* out, void* stream);
/* the same for double partials (the fp64 block sums of the CVaR-cut oracle) */
int rato_sum_partials_f64(const double* part, int32_t nblocks, int32_t ncols, double scale,
                          double* out, void* stream);

/* Failure detection (the reference has none: an infeasible QP only prints, drone_risk.py:458-459):
 * counts the NaN/Inf entries of a device array into *count (device uint32). */
int rato_count_nonfinite(const float* x, int64_t n, uint32_t* count, void* stream);

/* Same scan ACCUMULATING into *count (no reset): chain several arrays (g_up, Z, partial sums ...) into one counter,
 * zeroed by the caller (or by one rato_count_nonfinite), then read it once.  The facades' ``check_finite=True``
 * turns a non-zero count into RATO_ENONFINITE / RatoNonFiniteError. */
int rato_count_nonfinite_acc(const float* x, int64_t n, uint32_t* count, void* stream);

/* Workspace of rato_risk_stats for M samples: caller-owned device memory of this many bytes, set up ONCE with
 * rato_risk_stats_init (zero fill + a tag) before its first use; one workspace per stream that computes statistics
 * concurrently.  Every call leaves it ready for the next one (the histograms are re-zeroed by the last launch).  A
 * workspace that was never initialised makes the multi-launch path write NaN into all of `out` instead of numbers
 * computed from garbage. */
size_t rato_risk_stats_workspace_bytes(int64_t M);
int rato_risk_stats_init(void* workspace, size_t workspace_bytes, void* stream);

/*
 * Replaces the Monte-Carlo statistics: fraction satisfied (drone_risk.py:661,719),
 * empirical VaR (drone_main_plot.py:640-652: sort(Z)[M - floor(alpha M) - 1])
 * and AVaR/CVaR (drone_risk.py:663-695; the OSQP LP there is replaced by exact
 * selection of the Rockafellar-Uryasev minimiser followed by the closed form :694).
 *   Z [M]; thr = 1e-6 (the B_satisfied threshold)
 *   out: double[RATO_N_STATS] = { VaR, CVaR, fraction(Z<=thr), mean(Z), max(Z),
 *                       count(Z<=thr), sum(max(Z-t,0)), k (selected ascending rank),
 *                       #{Z > t}, #{Z == t}, t }
 *        t = the Rockafellar-Uryasev minimiser = sort(Z)[k]; VaR = t except when floor(alpha M) == M, where the
 *        reference's index -1 wraps to max(Z) (NumPy negative index, drone_main_plot.py:651) while CVaR, the counts
 *        and every consumer of the threshold (rato_saa_tail_rows*) keep using t = out[10].
 * Launches: 1 for M <= 12,288 (one workgroup, Z read once, keys resident in LDS: csrc/stats.hip rs_small); 1 for
 * M <= 1,048,576 (<= 64 workgroups, keys in registers, global histograms that the workgroups wait on: rs_coop -- these
 * workgroups must be resident together, which an otherwise idle or normally loaded GPU guarantees; a wait that does
 * not complete within ~0.5 s, e.g. on a workspace some aborted call left unclean, ends in NaN statistics and an
 * un-tagged workspace, never in a hang); 5 beyond (3 histogram passes, tail, final).  Exact selection, deterministic
 * sums; the three forms agree exactly on every output except the fp64 sums (equal to summation order).
 */
#define RATO_N_STATS 11
int rato_risk_stats(const float* Z, int64_t M, double alpha, float thr,
                    void* workspace, size_t workspace_bytes, double* out, void* stream);

/* The same record by the selection bodies at nt threads per workgroup (256, 512 or 1024; anything else: RATO_EINVAL), with
 * no producer to wait for: what the statistics workgroups of a launch that carries its own statistics run (params.stats_*:
 * 512 threads at the end of the row-parallel linearize launches, 256 at the end of the tiled eval launches; 1024 is
 * rato_risk_stats' own size), reachable on any Z.  Placed by those launches' rule: one workgroup for M <= 12,288, otherwise
 * ceil(M / (4 nt)) <= 64 cooperating workgroups, RATO_EINVAL beyond 64 * 16 * nt samples (nothing is launched, out is
 * not written).  Arguments and their errors as rato_risk_stats; the exactly defined entries of the record are those of
 * rato_risk_stats to the bit, the fp64 sums equal to summation order.  For tests of the selection at the sizes production
 * runs it at.  ABI: additive (RATO_ABI_VERSION stays 12). */
int rato_risk_stats_shaped(const float* Z, int64_t M, double alpha, float thr, void* workspace, size_t workspace_bytes,
                           double* out, void* stream, int32_t nt);

/* Recovery path: the same statistics by the launch-per-pass form (which waits for nothing) on a workspace re-initialised
 * on the stream.  For a caller whose rato_risk_stats record came back NaN although Z is finite -- the one-launch forms
 * give up, loudly, when the workgroups of their launch could not run together for seconds or the workspace was left
 * unclean by an aborted call.  The Python facades do this by themselves (stats.risk_stats, CvarCutSolver.evaluate). */
int rato_risk_stats_recover(const float* Z, int64_t M, double alpha, float thr,
                            void* workspace, size_t workspace_bytes, double* out, void* stream);

/*
 * Histogram of Z on the device (the main figure's histogram of the per-sample maxima, drone_main_plot.py:716-759, for
 * validation batches too large to bin on the host).  counts: uint32[bins + 3]
 *   [0] #{z < lo}    [1 + b] bin b    [bins + 1] #{z >= hi}    [bins + 2] #{z is NaN}
 *   b = min((int)((z - lo) * inv_w), bins - 1),  inv_w = (float)bins / (hi - lo)   -- all in fp32, nothing contracted, so
 *   that the same three float32 operations in NumPy give the same bin for every z.
 * 1 <= bins <= 4096, lo < hi, both finite (and hi - lo, inv_w finite), M >= 1; otherwise RATO_EINVAL.  The call zeroes
 * counts itself on the stream.  Integer atomics only (a histogram private to each workgroup in LDS, flushed once): the
 * result is deterministic and does not depend on the grid.
 */
int rato_histogram(const float* Z, int64_t M, float lo, float hi, int32_t bins, uint32_t* counts, void* stream);

/* rato_sum_partials(part, nblocks, ncols, scale, sums_out) and rato_risk_stats(Z, ...) in ONE launch when
 * M <= 1,048,576 (the partial-sum workgroups ride along with the selection workgroups; two stream-ordered calls
 * otherwise): the whole reduction stage of a single-GPU SAA step. */
int rato_sums_and_risk_stats(const float* part, int32_t nblocks, int32_t ncols, double scale, double* sums_out,
                             const float* Z, int64_t M, double alpha, float thr, void* workspace,
                             size_t workspace_bytes, double* out, void* stream);

/* ---- Driving Gaussian baseline (car/driving_gaussian.py) ------------------------------------------------------------
 * The define step of the baseline's SCP (get_all_constraints_coeffs, :303-354) has no sample axis but a tangent axis: it
 * is jacfwd of an S-step recursion of the mean (Euler, x+ = x + dt b(x, u; omega_nom), :172-186) and of the 8x8 covariance
 * (Sigma+ = A Sigma A^T + dt sigma sigma^T + Sigma_omega with A = I + dt db/dx, :188-228) with respect to the 2S controls
 * and the S risk allocations.  rato_car_gaussian_linearize evaluates values and closed-form derivatives for K problems in
 * ONE launch, fp64 throughout: one workgroup per problem, one lane per control direction (csrc/car_gaussian.hip).
 *
 *   g_t = -( |d| - ppf(1 - alpha_t) sqrt(n^T Sigma[4:6,4:6] n) - min_separation_distance ),  d = p_ego - p_ped, n = d/|d|,
 *   at steps 1..S (:238-264); ppf is Wichura's AS 241 (PPND16) evaluated at 1 - alpha as the reference does;
 *   d g_t / d alpha_t = -sqrt(n^T Sigma n) / pdf(ppf(1 - alpha_t)), and d g_t / d alpha_s = 0 for s != t.
 *
 * Reproduced as written in the reference (outer_product = 0):
 *   - force_on_pedestrian reads x[7] (the pedestrian's y velocity) as "speed_ego_along_y" (:120) and adds the SCALAR
 *     omega_speed (speed_ped_des - x[7]) to both force components (:127);
 *   - b_ds and b_dr are 1-D, so `b_ds @ b_ds.T` (:209-211) is an inner product and Sigma_due_to_omega is one scalar that
 *     `Sig_next +=` adds to all 64 entries (the quirk oracle/gaussian.py documents for the drone): the ego block of Sigma
 *     is not zero and the full symmetric 8x8 is carried.
 * outer_product = 1 adds the rank-one terms var_s b_ds b_ds^T + var_r b_dr b_dr^T instead.
 *
 * Every constant comes from the caller (the facade fills it from driving_params): nothing is baked into the kernel. */
typedef struct rato_car_gauss_params {
  int32_t S;                      /* 1..64 */
  int32_t outer_product;          /* 0: the reference's scalar Sigma_omega; 1: the rank-one terms */
  double dt;
  double omega_speed_nom, omega_repulsive_nom;     /* :79-80 */
  double omega_speed_var, omega_repulsive_var;     /* (2 del)^2 / 12, :81-84 */
  double beta;                    /* diffusion magnitude, 3e-2 (:77) */
  double speed_ped_des, min_separation_distance;
  double mean_init[8];            /* state_init */
  double ped_var_init[4];         /* diagonal of variance_ped_initial_state: Sigma_0[4+i][4+i] */
  double ego_goal[4];             /* (position_ego_goal, velocity_ego_goal) */
} rato_car_gauss_params;
size_t rato_car_gauss_params_bytes(void); /* sizeof the struct as this library was built: a binding checks its layout */

/* Device pointers (fp64), stream ordered, no allocation.  mus / Sigmas may be NULL (not written); every other pointer is
 * required.  g_obs_du column t*2+i is d/d u[t][i] (reshape(.., 'C') at :330); its strict upper triangle (column step >= row
 * step: step t+1 of the recursion does not see u[t'] for t' > t) is written as exactly 0.0.  g_obs_dalpha holds the diagonal
 * of the S x S block (the off-diagonal is identically zero).  v_final = x_S[0:4] - ego_goal (:230-235).
 * RATO_EINVAL without a launch unless 1 <= S <= 64, K >= 1 and the required pointers are non-NULL. */
int rato_car_gaussian_linearize(const rato_car_gauss_params* p, int32_t K,
                                const double* us /* [K][S][2] */, const double* alphas_risk /* [K][S] */,
                                double* mus /* [K][S+1][8] or NULL */, double* Sigmas /* [K][S+1][8][8] or NULL */,
                                double* g_obs /* [K][S] = -separation_distances_at_all_times */,
                                double* g_obs_du /* [K][S][2S] */, double* g_obs_dalpha /* [K][S] */,
                                double* v_final /* [K][4] */, double* v_final_du /* [K][4][2S] */, void* stream);

/*
 * Drone Gaussian baseline (drone/drone_gaussian.py) -- an addition within version 12.
 *
 * The script hands IPOPT three callbacks in z = (u (3S), state allocations (S n_obs), obstacle allocations (n_obs)), n_obs = 3:
 * g, jacfwd(g) and jacfwd(jacfwd(lam . g)) (:414-486), all through the S-step recursion of the mean (Euler at the nominal
 * mass, :161-174) and of the 6x6 covariance (Sigma+ = A Sigma A^T + dt sigma sigma^T + var_m (b_dm @ b_dm.T), :176-227).  The
 * two calls below evaluate them for K problems, fp64 throughout (csrc/drone_gaussian.hip).
 *
 * Layout of z, the reference's (:86-102, :356-366): us_mat[t][i] = z[3t + i]; the state allocation of obstacle i at step t
 * (state t+1) is z[3S + t n_obs + i]; the obstacle allocation of obstacle i is z[3S + S n_obs + i].  nvar = 3S + S n_obs + n_obs.
 *
 * The n_nl = 6 + n_obs S + 4 (S+1) non-linear rows, in the reference's order (:351-382):
 *   final  [6]           x_S - x_final
 *   obs    [6 + i S + t] -( |d| - ppf(1 - a_{t,i}) sqrt(n^T Sigma_{t+1}[:2,:2] n) - r_i ),  d = p_{t+1}[:2] - obs_positions[i],
 *                        n = d/|d|,  r_i = (obs_radii[i] + delta) - (a_obs,i / 3) 2 delta;  ppf is Wichura's AS 241 (PPND16)
 *   high   [.. + t 2 + j]  xs[t][j] - bound_high[j],  t = 0..S, j = 0, 1
 *   low    [.. + t 2 + j]  -xs[t][j] + bound_low[j]
 * The script's remaining nvar + 1 rows (z itself and the sum of the allocations, :323-349) are linear with constant
 * coefficients and no second derivative: they stay with the caller, and lam holds n_nl multipliers.
 *
 * Reference quirk, reproduced (there is no other mode): b_dm (:208) is 1-D, so `b_dm @ b_dm.T` is an inner product and the
 * mass term is ONE scalar added to all 36 entries of the covariance.  |v| in the drag differentiates as sign(v) with
 * sign(0) = 0, the convention of the reference's AD.
 *
 * Every constant comes from the caller (the facade fills it from drone_params): nothing is baked into the kernels. */
typedef struct rato_drone_gauss_params {
  int32_t S;                      /* 1..64 (one lane per control direction: 3S <= 192 lanes of one workgroup) */
  int32_t reserved;
  double dt;
  double mass_nom, mass_var;      /* mass_var = (2 mass_delta)^2 / 12 */
  double beta, drag;
  double feedback_kp, feedback_kd; /* feedback_gain = (kp I, kd I): control_applied = u + kp p + kd v */
  double x_init[6], x_final[6];
  double obs_positions[3][2];
  double obs_radii[3];
  double obs_radii_delta;
  double bound_high[2], bound_low[2]; /* (0.5, 0.5) and (-2, -0.5) in the script */
} rato_drone_gauss_params;
size_t rato_drone_gauss_params_bytes(void); /* sizeof the struct as this library was built: a binding checks its layout */

/* g and its Jacobian.  Device pointers (fp64), stream ordered, no allocation.  mus / Sigmas may be NULL (not written, and
 * the other outputs are bitwise the same either way); every other pointer is required.  jac_nl is dense row-major; its
 * structural zeros are written as exactly 0.0: control columns of step t' > t on obstacle row t, control columns of step
 * t' >= t and of another axis on a mean row of state t, and every allocation column but the row's own a_{t,i}
 * (-sqrt(w) / pdf(q)) and a_obs,i (-2 delta / 3).
 * RATO_EINVAL without a launch unless 1 <= S <= 64, K >= 1 and the required pointers are non-NULL. */
int rato_drone_gaussian_linearize(const rato_drone_gauss_params* p, int32_t K, const double* Z /* [K][nvar] */,
                                  double* mus /* [K][S+1][6] or NULL */, double* Sigmas /* [K][S+1][6][6] or NULL */,
                                  double* g_nl /* [K][n_nl] */, double* jac_nl /* [K][n_nl][nvar] */, void* stream);

/* The Hessian of lam . g in np.tril_indices(nvar) order, what eval_h hands to IPOPT (:480-486): the dense (u,u) block (one
 * lane per pair of control directions), (u, a_{t,i}) = -lam_{(i,t)} (d sqrt(w) / du) / pdf(q), the diagonal of (a,a) =
 * lam q sqrt(w) / pdf(q)^2, and exactly 0.0 everywhere else (everything involving a_obs included).
 * The kernels keep their state in registers, so rato_drone_gaussian_hessian_workspace_bytes is 0 at every (S, K) today and
 * workspace may then be NULL; a caller still passes what the query returns.  RATO_EINVAL without a launch unless
 * 1 <= S <= 64, K >= 1, Z, lam and hess_tril are non-NULL and workspace_bytes covers the query. */
size_t rato_drone_gaussian_hessian_workspace_bytes(int32_t S, int32_t K);
int rato_drone_gaussian_hessian(const rato_drone_gauss_params* p, int32_t K, const double* Z /* [K][nvar] */,
                                const double* lam /* [K][n_nl] */, double* hess_tril /* [K][nvar (nvar+1) / 2] */,
                                void* workspace, size_t workspace_bytes, void* stream);

/*
 * Hopper NLP (hopper/hopper.py:491-514, :569-580) -- an addition within version 12.
 *
 * The script hands IPOPT g, jacrev(g) and hessian(lam . g) in z = (x_0 .. x_S (8 each), u_0 .. u_{S-1} (4 each), ys (M), slack,
 * t_risk): x_t = z[8t .. 8t+8), u_t = z[8(S+1) + 4t ..) (:105-132); nvar = 8(S+1) + 4S + M + 2.  The rows that carry the
 * sample axis are rato_hopper_slip* above.  The calls below evaluate every other non-linear row for K problems, fp64
 * throughout (csrc/hopper_nlp.hip), as per-step LOCAL quantities: they are phase-agnostic, and the caller owns the contact /
 * flight masks (time_jump, time_land), the constant unit coefficients and the placement in the script's row order.
 *
 * Every constant comes from the caller (the facade fills it from the script's values): nothing is baked into the kernels.
 * state_initial / state_final and the phase times travel with the struct for the caller's rows (x_0 - state_initial,
 * x_S[4:6] - state_final[4:6], the masks); the kernels validate the phase times and read neither state. */
typedef struct rato_hopper_nlp_params {
  int32_t S;                      /* >= 1 */
  int32_t time_jump, time_land;   /* 0 <= time_jump <= time_land <= S */
  int32_t reserved;
  double dt;
  double mass_body, mass_leg;
  double inertia_body, inertia_leg;
  double gravity;
  double state_initial[8], state_final[8];
} rato_hopper_nlp_params;
size_t rato_hopper_nlp_params_bytes(void); /* sizeof the struct as this library was built: a binding checks its layout */

/* The RK4 defect (:240-248) of every step and the two state rows of every state, with their first derivatives.  Device pointers
 * (fp64), stream ordered, no allocation.  Z is [K][ldz] with ldz >= 8(S+1) + 4S (the tail of a problem's z is not read).
 *   defect   [K][S][8]       x_{t+1} - (x_t + dt/6 (k1 + 2 k2 + 2 k3 + k4))
 *   d_defect [K][S][8][12]   its derivative with respect to (x_t, u_t); the x_{t+1} coefficient is the identity and stays
 *                            with the caller
 *   rows     [K][S+1][2]     [0] the no-slip value J_T q_dot = x4 + x3 cos(x2) x6 + sin(x2) x7 (:288-293),
 *                            [1] the end-effector height x1 - x3 cos(x2) (:166-171), at every state
 *   d_rows   [K][S+1][2][4]  their derivatives with respect to (x2, x3, x6, x7); the unit coefficients on x4 and x1 stay with
 *                            the caller
 * Any output may be NULL (not written; the others are bitwise the same either way).  One lane per (problem, state, direction);
 * nothing depends on S fitting a workgroup.  RATO_EINVAL without a launch unless S >= 1, K >= 1, ldz >= 8(S+1) + 4S,
 * 0 <= time_jump <= time_land <= S, Z is non-NULL and K (S+1) 12 lanes fit the grid's index range. */
int rato_hopper_nlp_linearize(const rato_hopper_nlp_params* p, int32_t K, const double* Z /* [K][ldz] */, int64_t ldz,
                              double* defect, double* d_defect, double* rows, double* d_rows, void* stream);

/* The Hessian of lam . g over the rows above, which is block diagonal over the steps: block t on (x_t (8), u_t (4)), t = 0..S,
 * as the lower triangle in np.tril_indices(12) order (78 entries); the u part of block S is exactly 0.0.
 *   lam_dyn     [K][S][8]     multipliers of the defect rows
 *   lam_rows    [K][S+1][2]   per-state weights of the two state rows (the caller folds the no-slip, contact and leg-over-ground
 *                             (sign -1) multipliers into them by phase)
 *   add         [K][S+1][78]  or NULL: blocks added to the output (the slip part and obj_factor hess_f)
 *   hess_blocks [K][S+1][78]
 * Second-order tangents are carried through the four RK4 stages, one lane per (problem, block, pair of directions); pairs that
 * hold x0, x1, x4 or x5 carry no second derivative and only forward `add`.  RATO_EINVAL without a launch as above, and when
 * lam_dyn, lam_rows or hess_blocks is NULL. */
int rato_hopper_nlp_hessian(const rato_hopper_nlp_params* p, int32_t K, const double* Z /* [K][ldz] */, int64_t ldz,
                            const double* lam_dyn, const double* lam_rows, const double* add, double* hess_blocks,
                            void* stream);

/* Emission: dst[k][map[i]] = scale[i] src[k][i] for i < n, k < K (scale NULL: 1).  map is a device array of int64; an entry
 * outside [0, n_dst) is not emitted.  The caller zeroes (or pre-fills) dst once: what the map does not point at is left alone.
 * Places the local blocks into the CSC value array of the Jacobian and into the tril-packed dense Hessian.
 * RATO_EINVAL without a launch unless 1 <= K <= 65535, n >= 1, ld_src >= n, n_dst >= 1, ld_dst >= n_dst and src, map, dst are
 * non-NULL. */
int rato_scatter_f64(int32_t K, int64_t n, const double* src /* [K][ld_src] */, int64_t ld_src, const int64_t* map /* [n] */,
                     const double* scale /* [n] or NULL */, double* dst /* [K][ld_dst] */, int64_t ld_dst, int64_t n_dst,
                     void* stream);

/*
 * Hopper slip rows in fp64 (hopper/hopper.py:68-81, :300-367, :569-580) -- a further addition within version 12.
 *
 * The risk group of the NLP above at the precision of its other rows: h_ic = fx_c - mu_i(p_c) fz_c for problem k, sample i and
 * contact c on step t_c of [0, time_jump) U [time_land, S) (C = time_jump + S - time_land contacts), computed from Z on the
 * device: x_t = Z[k][8t ..), (fx, fz) = Z[k][8(S+1) + 4t + 2 ..), p = x0 + x3 sin x2, chain J = (1, x3 cos x2, sin x2),
 * mu_i(p) = mu_nom + sum_k a_ik cos(theta_ik p + tau_ik) with fp64 sin / cos (csrc/hopper_slip64.hip; the per-lane arithmetic
 * is csrc/rato_hopper_slip64.h).  rato_hopper_slip* above (fp32) stays the Monte-Carlo / large-M throughput path.
 *
 * Device pointers (fp64), stream ordered, no allocation.  p supplies S and the phase times (nothing else of it is read);
 * mu_nom comes from the caller.  a, theta, tau are [30][M].  Outputs, any of which may be NULL (not written; the others are
 * bitwise the same either way):
 *   h      [K][C][M]      fx - mu fz
 *   dh_dfz [K][C][M]      -mu
 *   dh_dx  [K][C][3][M]   dh/d(x0, x2, x3) = -mu' fz J, the chain applied: the x3 entry is 0.0 where sin x2 is
 *   Zmax   [K][M]         max over the contacts of h
 * lam (or NULL) is the caller's multiplier array [K][ldlam] read in place at lam[k][lam_r0 + i C + c] (the risk rows' own
 * order; ldlam >= lam_r0 + M C).  With lam:
 *   part   workspace, double[rato_hopper_slip_f64_nblocks(M)][K][C][3]: per-workgroup sums over the samples of a tile
 *   D      [K][C][3]      (D1, D2, D0) = sum_i lam (d2h/(dp dfz), d2h/dp2, dh/dp) = sum_i lam (-mu', -mu'' fz, -mu' fz)
 * The sums are fp64 in a fixed order (a tree inside the workgroup, then rato_sum_partials_f64 over the tiles), without atomics:
 * two calls on the same inputs are bitwise equal, and row k of a K-problem call is bitwise what the K = 1 call gives.
 * One launch for K problems, two with lam.  A workgroup is a tile of TI samples x 256 / TI contacts, TI the smallest power of
 * two >= M, at most 256 (rato_hopper_slip_f64_nblocks(M) = ceil(M / TI) tiles).
 * RATO_EINVAL without a launch unless S >= 1, 1 <= K <= 65535, M >= 1, ldz >= 8(S+1) + 4S, 0 <= time_jump <= time_land <= S,
 * Z and the fields are non-NULL and, with lam, part and D are non-NULL, lam_r0 >= 0 and ldlam >= lam_r0 + M C.  C = 0 is valid
 * and launches nothing.
 *
 * rato_hopper_slip_f64_fields -- a further addition within version 12: the same call with friction fields per problem.  ldf is
 * the number of doubles between the field arrays of problem k and problem k + 1: problem k reads a + k ldf, theta + k ldf and
 * tau + k ldf, each [30][M] (ldf > 30 M: the padding is never read).  ldf = 0 shares one set of fields among the K problems,
 * which is rato_hopper_slip_f64 (that entry is this one with ldf = 0).  Any other ldf (negative, or 0 < ldf < 30 M) is
 * RATO_EINVAL without a launch.  Launch shape, workspace and the order of every sum do not depend on ldf: row k of a K-problem
 * call with fields per problem is bitwise the K = 1 call on problem k's fields.
 */
int rato_hopper_slip_f64_nblocks(int32_t M);
int rato_hopper_slip_f64(const rato_hopper_nlp_params* p, double mu_nom, int32_t K, int32_t M,
                         const double* Z /* [K][ldz] */, int64_t ldz, const double* a, const double* theta, const double* tau,
                         const double* lam /* [K][ldlam] or NULL */, int64_t ldlam, int64_t lam_r0, double* h, double* dh_dfz,
                         double* dh_dx, double* Zmax, double* part, double* D, void* stream);
int rato_hopper_slip_f64_fields(const rato_hopper_nlp_params* p, double mu_nom, int32_t K, int32_t M,
                                const double* Z /* [K][ldz] */, int64_t ldz, const double* a, const double* theta,
                                const double* tau, int64_t ldf, const double* lam /* [K][ldlam] or NULL */, int64_t ldlam,
                                int64_t lam_r0, double* h, double* dh_dfz, double* dh_dx, double* Zmax, double* part, double* D,
                                void* stream);

/* The slip rows' share of hess(lam . g), added IN PLACE into add [K][S+1][78] (the `add` of rato_hopper_nlp_hessian, zeroed or
 * pre-filled by the caller) at the np.tril_indices(12) positions of step t_c: local indices 0, 2, 3 (x0, x2, x3) and 11 (fz),
 * nine entries per contact -- the block D2 J J' + D0 H with H the curvature of p (H11 = -x3 sin x2, H12 = H21 = cos x2) and
 * the mixed entries D1 J.  D [K][C][3] is rato_hopper_slip_f64's.  One lane per (problem, contact, entry); contacts sit on
 * distinct steps, so every entry has one writer.  RATO_EINVAL as above, and when Z, D or add is NULL; C = 0 launches nothing. */
int rato_hopper_slip_hess_blocks_f64(const rato_hopper_nlp_params* p, int32_t K, const double* Z /* [K][ldz] */, int64_t ldz,
                                     const double* D, double* add, void* stream);

/*
 * The Newton step of the hopper's interior-point solver (riskaversetrajopt_amd/hopper_ipm.py; csrc/hopper_ipm.hip) -- a further
 * addition within version 12.  fp64 throughout, K problems per launch, device pointers, stream ordered, no allocation.  No
 * floating-point atomics: every output entry has one owner that sums in a fixed order, so two calls are bitwise equal and
 * problem k of a batch is bitwise its K = 1 call.
 *
 * The Jacobian J (ncon x n) is given by its values on a FIXED pattern, as one or two arrays per problem: value index i is
 * vals0[k][i] for i < n0 and vals1[k][i - n0] otherwise (n1 = 0: vals1 is not read).  For the hopper these are nlp_device's
 * jac_values and slip_jac_values where they lie; the index lists below are built once on the host in that numbering.
 *
 * rato_normal_matrix_f64:  Kc[k] = J' diag(d[k]) J + W[k] + diag(diag[k]), the lower triangle (b <= a) of a row-major n x n
 * array with leading dimension lda >= n, Kc[k][a][b] at Kc[(k n + a) lda + b]; the strict upper triangle and the padding are
 * not touched.  One lane per (a, b):
 *   ent_of   [n][n] int32   the structural entry of (a, b), or -1: the lane writes 0.0
 *   ptr      [n_ent + 1]    the entry's segment of the product map
 *   tri_a, tri_b, tri_r     per triple the value indices of J_ra and J_rb and the row r, sorted by r inside a segment; the
 *                           lane sums (J_ra d_r) J_rb in that order
 *   hess_src [n_ent] int32  where the entry lies in hess[k] (-1: nowhere); hess [K][n_hess] (the step blocks, or NULL) is
 *                           added after the sum, diag [K][n] (or NULL) after that on a == b
 * rato_csc_matvec_f64 / rato_csc_tmatvec_f64:  out[k] = J v[k] (one lane per row, through the row list row_ptr / row_idx /
 * row_col) and out[k] = J' w[k] (one lane per column: col_ptr is the CSC indptr in the same numbering, col_idx the value
 * index, col_row the row).
 * RATO_EINVAL without a launch on a NULL or undersized argument, K outside [1, 65535] or n > 32768.  The lists are trusted:
 * their indices must lie inside the arrays they address.
 */
int rato_normal_matrix_f64(int32_t K, int32_t n, int64_t lda, const double* vals0, int64_t ld0, int64_t n0, const double* vals1,
                           int64_t ld1, int64_t n1, const double* d /* [K][ncon] */, int64_t ncon, const double* hess,
                           int64_t n_hess, const double* diag, const int32_t* ent_of, const int64_t* ptr, const int32_t* tri_a,
                           const int32_t* tri_b, const int32_t* tri_r, const int32_t* hess_src, double* Kc, void* stream);
int rato_csc_matvec_f64(int32_t K, int64_t ncon, int64_t n, const double* vals0, int64_t ld0, int64_t n0, const double* vals1,
                        int64_t ld1, int64_t n1, const int64_t* row_ptr, const int32_t* row_idx, const int32_t* row_col,
                        const double* v /* [K][ldv] */, int64_t ldv, double* out /* [K][ldo] */, int64_t ldo, void* stream);
int rato_csc_tmatvec_f64(int32_t K, int64_t ncon, int64_t n, const double* vals0, int64_t ld0, int64_t n0, const double* vals1,
                         int64_t ld1, int64_t n1, const int64_t* col_ptr, const int32_t* col_idx, const int32_t* col_row,
                         const double* w /* [K][ldw] */, int64_t ldw, double* out /* [K][ldo] */, int64_t ldo, void* stream);

/* ---- What the interior-point driver on the device needs of the hopper between those launches (csrc/hopper_g.hip)
 * -- a further addition within version 12.  fp64, K problems per launch, device pointers, stream ordered, no allocation, no
 * workspace, no atomics: two calls are bitwise equal and problem k of a batch is bitwise its K = 1 call.
 *
 * rato_hopper_g_f64: g [K][ldg >= ncon] in the script's row order (:491-514; hopper.Model.nlp_layout()["off"]): the defect, x_0 -
 *   state_initial, (x_S - state_final)[4:6], the no-slip and contact rows on the contact states, minus the end-effector height on
 *   the flight steps, the risk group, the controls, the slack and the three leg rows -- from Z [K][ldz >= nvar = 8(S+1) + 4S + M +
 *   2], defect [K][S][8] and rows [K][S+1][2] (rato_hopper_nlp_linearize's) and the slip values h of rato_hopper_slip_f64, problem
 *   k at h + k M C, sample i and contact c at i h_stride_sample + c h_stride_contact: (C, 1) reads the rows' order i C + c, (1, M)
 *   reads [C][M] as the slip kernel leaves it.  saa != 0: the risk group is (malpha[k] t + sum ys, -ys_i, ((h_ic - t) - ys_i) -
 *   slack, 0), malpha [K] = M alpha per problem; saa == 0: h_ic - slack.  C = 0 (no contact step) is valid: h is not read.
 *   p supplies S, the phase times and the two states.  One lane per row; every row but the sum row is bitwise the host's
 *   (hopper_ipm.assemble_g) from the same pieces.  The sum row has one owner, a workgroup that adds ys lane-strided ascending,
 *   the wave's fixed tree, then the four waves in order: the order depends on M alone.  Padding is never written.
 * rato_hopper_block_symv_f64: out[k] = W x[k] (x [K][ldx >= n], out [K][ldo >= n]) with W given as the step blocks [K][S+1][78] of
 *   rato_hopper_nlp_hessian: one lane per (problem, block, local row) sums its 12 products with the column ascending (8 in
 *   block S, whose u part does not exist); the n - 8(S+1) - 4S entries behind the blocks' variables (ys, slack, t_risk) are
 *   written +0.
 * RATO_EINVAL without a launch on a NULL or undersized argument, K outside [1, 65535], S < 1, M < 1, phase times outside
 * 0 <= time_jump <= time_land <= S, h strides below 1 or reaching past M C values, n < 8(S+1) + 4S. */
int rato_hopper_g_f64(const rato_hopper_nlp_params* p, int32_t K, int64_t M, int32_t saa, const double* Z /* [K][ldz] */,
                      int64_t ldz, const double* defect, const double* rows, const double* h, int64_t h_stride_sample,
                      int64_t h_stride_contact, const double* malpha /* [K], saa only */, double* g, int64_t ldg, void* stream);
int rato_hopper_block_symv_f64(int32_t K, int32_t S, int64_t n, const double* blocks, const double* x, int64_t ldx, double* out,
                               int64_t ldo, void* stream);

/* ---- Batched Cholesky, fp64 (csrc/chol.hip, on the workgroup functions of csrc/rato_chol.h; riskaversetrajopt_amd/ipm.py).
 * In-place blocked Cholesky A = L L' of K row-major matrices A[k] (n x n, leading dimension lda >= n), lower triangle: only
 * entries with b <= a < n are read or written, so the strict upper triangle and the padding may hold anything (NaN included).
 * One workgroup per problem, panels of rato_chol_panel_width() columns.  info[k] = 0, or j + 1 for the first pivot j that is
 * not a positive finite number: that problem stops there (its matrix is left partly factored), the others are not affected and
 * the call still returns RATO_OK -- an indefinite matrix is an answer (the solver's inertia test), not an error.
 * rato_chol_solve_batch_f64 solves L L' x = b in place for nrhs right-hand sides per problem, B[k][r] at B[(k nrhs + r) ldb],
 * ldb >= n, n <= 8000.  RATO_EINVAL without a launch on NULL pointers, n < 1, lda < n, ldb < n or K outside [1, 65535]. */
int rato_chol_panel_width(void);
int rato_chol_factor_batch_f64(double* A, int32_t n, int64_t lda, int32_t K, int32_t* info, void* stream);
int rato_chol_solve_batch_f64(const double* L, int32_t n, int64_t lda, int32_t K, double* B, int32_t nrhs, int64_t ldb,
                              void* stream);

/* ---- The same Cholesky spread over the device (csrc/chol_grid.hip; ipm.chol_factor / chol_solve with method='grid').
 * ABI: additive (RATO_ABI_VERSION stays 12).  Same layout, panels, arguments and info as the two entries above, and the same
 * arithmetic per entry in the same order: L, info of the problems that succeed, and X are BITWISE those of
 * rato_chol_factor_batch_f64 / rato_chol_solve_batch_f64 (what a failed problem's matrix holds is unspecified, as there).
 * The factorization is a stream-ordered sequence of launches, ONE per panel.  Launch q holds, per problem, a workgroup per
 * 64-row block below panel q, which applies panel q - 1's update to its own rows of panel q and to the old diagonal block,
 * factors the 32 x 32 diagonal block for itself and solves its rows in place, and a workgroup per 64 x 64 tile right of panel
 * q, which applies panel q - 1's update there.  Workgroups of a launch never wait for each other and none reads an entry
 * another one of the same launch writes: the factored diagonal block goes to work and is copied into A by the next launch.
 * The first launch sets info[k]; every later launch returns at once for a problem whose info[k] is set.  work: K *
 * rato_chol_grid_work_doubles(n) doubles of the caller's, contents irrelevant before and after; it may be NULL when the
 * query returns 0 (n <= rato_chol_panel_width()).  The library
 * allocates nothing.  The solve runs one workgroup per (problem, right-hand side) with no global load inside a dependent
 * chain.  No atomics: two calls are bitwise equal and problem k of a batch is bitwise its K = 1 call.  RATO_EINVAL without
 * a launch and with every output untouched on NULL pointers (work included where the query is positive), n < 1 (solve:
 * n > 8000), lda < n, ldb < n, nrhs or K outside [1, 65535]. */
int64_t rato_chol_grid_work_doubles(int32_t n);
int rato_chol_factor_grid_batch_f64(double* A, int32_t n, int64_t lda, int32_t K, int32_t* info, double* work, void* stream);
int rato_chol_solve_grid_batch_f64(const double* L, int32_t n, int64_t lda, int32_t K, double* B, int32_t nrhs, int64_t ldb,
                                   void* stream);

/* ---- Batched dense convex QP solve, fp64 (csrc/qp_ipm.hip): the QPs of the driving Gaussian baseline's SCP
 * (car/driving_gaussian.py:428-456, n = 3S + 1 and m = 4S + 5 before the host presolve), which the reference hands to OSQP.
 * ABI: additive (RATO_ABI_VERSION stays 12).
 *
 * Problem k:  min 1/2 z'P z + q'z  s.t.  l <= A z <= u.  P [k] n x n row-major, symmetric positive semi-definite (its lower
 * triangle and its columns are read), at P + k strideP; q [k] at q + k strideq; a stride of 0 shares P or q across the batch.
 * A [k] m x n row-major with leading dimension lda >= n at A + k strideA (the padding is never read); l, u [k] at
 * l + k stridelu, u + k stridelu: +-inf = that side is absent, l == u = an equality.  m = 0 is allowed (A, l, u may be NULL).
 *
 * ONE launch solves all K problems to completion, one workgroup per problem, by a Mehrotra predictor-corrector interior-point
 * method (cold start from z = 0; the method and its constants: riskaversetrajopt_amd/qp_ipm.py, whose solve_numpy is the same
 * algorithm on the host).  tol <= 0 means 1e-8, max_iter <= 0 means 100; the loop is capped at 200 iterations and 12 retries
 * per factorization whatever the arguments say.  Outputs, all fully written whatever the status: z [k] (n) at z + k stridez,
 * y [k] (m, OSQP's sign: y > 0 on an active upper side, y < 0 on an active lower side) at y + k stridey, and
 * info [k][8] = {status, iterations, factorizations, primal residual, dual residual, mu, last delta_w, largest
 * complementarity product max_i(lam_l |A z - l|, lam_u |u - A z|)_i} with status
 * 0 solved, 1 max_iter, 2 numerical (the factorization failed through the whole retry ladder, or a residual or step went
 * non-finite: z, y are the last finite iterate), 3 invalid (NaN or inf in P, q, A, NaN in l or u, l > u, l = +inf or
 * u = -inf on a row: z, y are NaN).  No floating-point atomics and fixed summation orders: problem k of a batch is bitwise its
 * K = 1 run.
 *
 * workspace: rato_qp_ipm_workspace_bytes(K, n, m) bytes of device memory, 8-byte aligned (the condensed matrices; nothing is
 * read from it before it is written).  Stream-ordered, no allocation.  RATO_EINVAL without a launch on NULL pointers, n < 1 or
 * n > 256, m < 0 or m > 384, lda < n, a stride too small for its array, a workspace too small, or K outside [1, 65535]. */
size_t rato_qp_ipm_workspace_bytes(int32_t K, int32_t n, int32_t m);
int rato_qp_ipm_batch_f64(int32_t K, int32_t n, int32_t m, const double* P, int64_t strideP, const double* q, int64_t strideq,
                          const double* A, int64_t lda, int64_t strideA, const double* l, const double* u, int64_t stridelu,
                          double tol, int32_t max_iter, double* z, int64_t stridez, double* y, int64_t stridey,
                          double* info /* [K][8] */, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Dense Newton-step arithmetic, fp64 (csrc/drone_gaussian_ipm.hip): what the interior-point solve of the drone Gaussian
 * baseline (riskaversetrajopt_amd/drone_gaussian_ipm.py) does on the values rato_drone_gaussian_linearize /
 * rato_drone_gaussian_hessian leave on the device.  ABI: additive (RATO_ABI_VERSION stays 12).  K problems per launch, device
 * pointers, stream ordered, no allocation, no workspace.  No floating-point atomics: every output entry has one owner that
 * sums in a fixed order, so two calls are bitwise equal and problem k of a batch is bitwise its K = 1 call.
 *
 * The kernels are generic.  The constraint matrix J (m x n, m = m0 + m1) is given as two dense row-major row blocks:
 *   J0 [K][m0][ld0], ld0 >= n, m0 >= 1                    one block per problem
 *   J1 [m1][ld1] at J1 + k stride1, ld1 >= n, m1 >= 0     stride1 = 0: shared by the batch (m1 = 0: J1 is not read)
 * Padding columns (>= n) are never read.  Vectors over the rows (d, w, the matvec's out) have length m0 + m1, J0's rows first.
 *
 * rato_dense_normal_matrix_f64:  Kc[k] = unpack(hess_tril[k]) + diag(diag[k]) + J' diag(d[k]) J, the lower triangle of a
 *   row-major n x n array with leading dimension lda >= n (what rato_chol_factor_batch_f64 reads): only entries b <= a < n are
 *   written, the strict upper triangle and the padding are never touched.  hess_tril [K][n (n + 1) / 2] in np.tril_indices
 *   order (entry (a, b) at a (a + 1) / 2 + b) or NULL; diag [K][n] or NULL.  Every entry is one accumulator that takes
 *   (J_ra d_r) J_rb for r ascending, then hess_tril, then diag: the order depends on neither K, nor the tile of
 *   rato_dense_tile_width() columns the entry falls in, nor n's relation to that width.
 * rato_dense_matvec_f64:   out[k] = J x[k]  (x [K][ldx >= n], out [K][ldo >= m]); a row is one wave's fixed-order reduction.
 * rato_dense_tmatvec_f64:  out[k] = J' w[k] (w [K][ldw >= m], out [K][ldo >= n]); one lane per column, rows ascending.
 * rato_tril_symv_f64:      out[k] = H[k] x[k] for the symmetric H given tril-packed as above.
 * RATO_EINVAL without a launch on NULL pointers, n < 1 or n > 32768, lda < n, a leading dimension below the length it serves,
 * m0 < 1, m1 < 0, 0 < stride1 < (m1 - 1) ld1 + n, or K outside [1, 65535]. */
int rato_dense_tile_width(void);
int rato_dense_normal_matrix_f64(int32_t K, int32_t n, int64_t lda, const double* J0, int32_t m0, int64_t ld0, const double* J1,
                                 int32_t m1, int64_t ld1, int64_t stride1, const double* d /* [K][ldd] */, int64_t ldd,
                                 const double* hess_tril, const double* diag, double* Kc, void* stream);
int rato_dense_matvec_f64(int32_t K, int32_t n, const double* J0, int32_t m0, int64_t ld0, const double* J1, int32_t m1,
                          int64_t ld1, int64_t stride1, const double* x, int64_t ldx, double* out, int64_t ldo, void* stream);
int rato_dense_tmatvec_f64(int32_t K, int32_t n, const double* J0, int32_t m0, int64_t ld0, const double* J1, int32_t m1,
                           int64_t ld1, int64_t stride1, const double* w, int64_t ldw, double* out, int64_t ldo, void* stream);
int rato_tril_symv_f64(int32_t K, int32_t n, const double* hess_tril, const double* x, int64_t ldx, double* out, int64_t ldo,
                       void* stream);

/* ---- Arrowhead Newton step of the hopper's interior-point solve at large M, fp64 (csrc/hopper_arrow.hip; hopper_arrow.py,
 * newton='arrow').  ABI: additive (RATO_ABI_VERSION stays 12).  K problems per launch, device pointers, stream ordered, no
 * allocation.  No floating-point atomics: every output has one owner that sums in a fixed order, so two calls are bitwise equal
 * and problem k of a batch is bitwise its K = 1 call.
 *
 * The M variables ys enter the condensed matrix only through E = diag(e) + d_0 1 1' and one row each of B = B_s + beta 1 e_t',
 * so they are eliminated exactly; these entry points do the work over the sample axis.  Inputs shared by all of them:
 *   dh_dx [K][C][3][M], dh_dfz [K][C][M]   the partials rato_hopper_slip_f64 leaves; with them
 *                                          g_ic = (dh/dx0, dh/dx2, dh/dx3, 1 on fx, dh/dfz) and grad h_ic = (g_ic, -1 on slack,
 *                                          -1 on t_risk [saa only])
 *   d [K][ldd], r0, saa                    row weights read in place: the slip row of sample i, contact c at r0 + i C + c; with
 *                                          saa != 0 the row -y_i at r0 - M + i and the sum row at r0 - M - 1
 *   touched columns                        q = 5C + 2: contact c owns 5c .. 5c + 4 (x0, x2, x3, fx, fz), then slack, then t_risk
 * Samples are cut into chunks of rato_hopper_arrow_chunk(); a chunk sums its samples ascending into part
 * [rato_hopper_arrow_nchunks(M)][K][n_part], a second launch sums the chunks ascending into red [K][n_part].
 *
 * rato_hopper_arrow_reduce_f64: with b_i = -sum_c d_ic grad h_ic (never stored in memory), e_i = ydiag_i (+ d_(1+i) + sum_c d_ic
 *   with saa) is written to e [K][M], and with u = 1 / e, n_part = rato_hopper_arrow_npart(C) values per problem in this order:
 *   G = sum u_i b_i b_i' (lower triangle, entry (p, r <= p) at p (p + 1) / 2 + r), w = sum u_i b_i (q), a = sum b_i (q),
 *   s = sum u_i (1), P_c = sum_i d_ic g_ic g_ic' (per contact the 15 entries of its lower triangle).
 * rato_hopper_arrow_assemble_f64: adds into the row-major lower triangle Sh [K][nc][lda] (what rato_normal_matrix_f64 left for
 *   the deterministic rows on the core columns) at (qcol[p], qcol[r]) the slip rows' share (P_c, a) and, with saa,
 *   - [G + beta (w e_t' + e_t w') + beta^2 s e_t e_t'] + k v v' + d_0 malpha^2 e_t e_t', beta = d_0 malpha[k],
 *   k = d_0 / (1 + d_0 s), v = w + beta s e_t.  Nothing else of Sh is read or written.
 * rato_hopper_arrow_cols_f64: red [K][5C + 1] = per (c, j) sum_i omega_ic g_ic[j]; mode 0: omega_ic = w[r0 + i C + c], and yout
 *   [K][M] (may be NULL) takes w_0 - w_(1+i) - sum_c omega_ic (0 without saa): J_risk' w.  mode 1: omega_ic = -t_i w[r0 + i C + c]
 *   (pass d as w), slot 5C takes sum_i t_i: B_s' t.
 * rato_hopper_arrow_rows_f64: mode 0: out[k][r0 + i C + c] = g_ic . xq_c - xq_slack - xq_t - xy_i, and with saa out[k][r0 - M + i]
 *   = -xy_i and red[k] = sum_i xy_i (xq [K][q], xy [K][M]): J_risk v but for the sum row's M alpha v_t.  mode 1: out[k][i] =
 *   sum_c -d_ic (g_ic . xq_c - xq_slack - xq_t) + addc[k]: B x_c; with xy != NULL, xy_i minus that: r_y - B x_c.
 * rato_hopper_arrow_edot_f64: red[k] = sum_i (1 / e_i) v_i.  rato_hopper_arrow_eapply_f64: out_i = (1 / e_i) (v_i - kappa[k]).
 * RATO_EINVAL without a launch on a NULL or undersized argument, K outside [1, 65535], M < 1, C outside [1, 50], a mode other
 * than 0 or 1, or r0 too small for the rows in front of it. */
int rato_hopper_arrow_nchunks(int64_t M);
int rato_hopper_arrow_chunk(void);
int64_t rato_hopper_arrow_npart(int32_t C);
int rato_hopper_arrow_reduce_f64(int32_t K, int64_t M, int32_t C, int32_t saa, const double* dh_dx, const double* dh_dfz,
                                 const double* d, int64_t ldd, int64_t r0, const double* ydiag /* [K][M] */, double* e,
                                 double* part, double* red, void* stream);
int rato_hopper_arrow_assemble_f64(int32_t K, int64_t M, int32_t C, int32_t saa, int32_t nc, int64_t lda, const int32_t* qcol,
                                   const double* red, const double* d, int64_t ldd, int64_t r0, const double* malpha /* [K] */,
                                   double* Sh, void* stream);
int rato_hopper_arrow_cols_f64(int32_t K, int64_t M, int32_t C, int32_t saa, int32_t mode, const double* dh_dx,
                               const double* dh_dfz, const double* w, int64_t ldw, int64_t r0, const double* t, double* yout,
                               double* part, double* red, void* stream);
int rato_hopper_arrow_rows_f64(int32_t K, int64_t M, int32_t C, int32_t saa, int32_t mode, const double* dh_dx,
                               const double* dh_dfz, const double* xq, const double* xy, const double* d, int64_t ldd, int64_t r0,
                               const double* addc, double* out, int64_t ldo, double* part, double* red, void* stream);
int rato_hopper_arrow_edot_f64(int32_t K, int64_t M, const double* e, const double* v, double* part, double* red, void* stream);
int rato_hopper_arrow_eapply_f64(int32_t K, int64_t M, const double* e, const double* v, const double* kappa, double* out,
                                 void* stream);

/* The fix-ups between the launches above, for the step under the interior-point driver on the device (hopper_arrow.py,
 * ArrowDeviceBackend's *_t methods): what the list methods do on the host, operation by operation in the host's order (every
 * product that feeds a sum is rounded on its own), so each output is bitwise the host's line.  ABI: additive.  One lane per
 * output, no sums over K, no scratch; vectors in z / row / core numbering come with their leading dimension and their padding
 * is neither read nor written; red is what the named launch left, [K][ldr].
 * rato_hopper_arrow_scale_f64: out[k][ocol] = a[k] x[k][col] (+ add[k] unless add is NULL).  With a = malpha, col = n - 1, add =
 *   the red of rows mode 0, ocol = the sum row: the sum row of J x; with a = beta, col = nc - 1: addc of rows mode 1.
 * rato_hopper_arrow_tfix_f64: after cols mode 0, with tot = -(red[3] + red[8] + ... ) summed contacts ascending from 0:
 *   out[k][qz[j]] += red[k][j] (j < 5C; qz [5C] the z index of the touched columns, an entry outside [0, n - 2 - M) is skipped),
 *   out[k][n - 2] += tot, and with saa out[k][n - 1] += malpha[k] w[k][rr] + tot and out[k][n - 2 - M + i] = yout[k][i]
 *   (yout [K][M] as cols leaves it): J' w in z numbering, n the number of variables, rr the sum row.
 * rato_hopper_arrow_kkbeta_f64: after reduce, kk[k] = d0 / (1 + d0 s), beta[k] = d0 malpha[k] with d0 = d[k][rr] and s =
 *   red[k][q (q + 1) / 2 + 2 q] (ldr >= rato_hopper_arrow_npart(C)).
 * rato_hopper_arrow_einv_f64: out[k][i] = (1 / e[k][i]) (v[k][i] - kk[k] red[k]), red [K] the result of edot; kk NULL: the
 *   baseline's (1 / e) v.  e [K][M] as reduce leaves it.
 * rato_hopper_arrow_rhsfix_f64: after cols mode 1, on rc [K][ldrc >= nc] in core numbering: rc[qcol[j]] -= red[j] (j < 5C; an
 *   entry outside [0, nc - 2) is skipped), rc[nc - 2] -= tot, rc[nc - 1] -= tot + beta[k] red[5C].
 * RATO_EINVAL without a launch on a NULL or undersized argument, a column outside its array, K outside [1, 65535], M < 1 or C
 * outside [1, 50]. */
int rato_hopper_arrow_scale_f64(int32_t K, const double* a /* [K] */, const double* x /* [K][ldx] */, int64_t ldx, int64_t col,
                                const double* add /* [K] or NULL */, double* out /* [K][ldo] */, int64_t ldo, int64_t ocol,
                                void* stream);
int rato_hopper_arrow_tfix_f64(int32_t K, int64_t M, int32_t C, int32_t saa, int64_t n, const int32_t* qz, const double* red,
                               int64_t ldr, const double* malpha, const double* w, int64_t ldw, int64_t rr, const double* yout,
                               double* out, int64_t ldo, void* stream);
int rato_hopper_arrow_kkbeta_f64(int32_t K, int32_t C, const double* d, int64_t ldd, int64_t rr, const double* red, int64_t ldr,
                                 const double* malpha, double* kk, double* beta, void* stream);
int rato_hopper_arrow_einv_f64(int32_t K, int64_t M, const double* e, const double* v, int64_t ldv, const double* kk,
                               const double* red, double* out, int64_t ldo, void* stream);
int rato_hopper_arrow_rhsfix_f64(int32_t K, int32_t C, int32_t nc, const int32_t* qcol, const double* red, int64_t ldr,
                                 const double* beta, double* rc, int64_t ldrc, void* stream);

/* ---- The interior-point driver's O(n + m) algebra on a state that stays on the device, fp64 (csrc/ipm_driver.hip): what
 * riskaversetrajopt_amd/ipm.py (Problem, newton_steps, solve_group) does on the host between the launches of a Newton step,
 * restated phase by phase.  ABI: additive (RATO_ABI_VERSION stays 12).  Model independent.  K problems per
 * launch, one workgroup of 256 lanes per problem, device pointers, stream ordered, no allocation, no workspace, no
 * floating-point atomics.  Every loop is lane-strided over ascending indices; a max is exact; a sum takes the per-lane
 * partials in ascending order, the wave's fixed tree and then the four waves in order: two calls are bitwise equal and problem
 * k of a batch is bitwise its K = 1 call.
 *
 * The state.  v = (z, s), nv = n + nI; rows of [K][ldv] arrays hold vectors of length nv or n, rows of [K][ldm] arrays
 * vectors over the m constraint rows; padding is never read or written.  vL / vU: -inf / +inf where a bound is absent.
 * row_slack [m] (shared): the slack number in [0, nI) of an inequality row, -1 for an equality row (whose value is gL).
 * The objective is f = sf (1/2 sum curv_j z_j^2 + sum lin_j z_j); lin is mandatory like every pointer of the struct (a model
 * without a linear part passes zeros) and enters gradf = sf (curv z + lin) -- hence rz, dual, E0 and Dbar -- and the objective
 * values of _step_setup and _accept; diag, phase R and quad know curv alone.  The struct grew by lin within version 12:
 * RATO_ABI_VERSION stays 12 and rato_ipm_state_bytes() against the binding's sizeof is the guard.  rec [K][RATO_IPM_REC] is the record of scalars the host reads back; status is
 * RATO_IPM_RUNNING or the index into ('converged', 'max_iter', 'line_search').  A problem whose status is not
 * RATO_IPM_RUNNING is left untouched by every call, and so is one that is not searching by _trial and _accept. */
#define RATO_IPM_REC 32
#define RATO_IPM_RUNNING (-1)
enum {
  RATO_IPM_MU = 0, RATO_IPM_NU, RATO_IPM_DW, RATO_IPM_DC, RATO_IPM_TOL, RATO_IPM_E0, RATO_IPM_PRIM, RATO_IPM_DUAL,
  RATO_IPM_A_MAX, RATO_IPM_A_DUAL, RATO_IPM_C1, RATO_IPM_DBAR, RATO_IPM_QUAD, RATO_IPM_PHI, RATO_IPM_DPHI, RATO_IPM_ALPHA,
  RATO_IPM_TRIALS, RATO_IPM_ITERATIONS, RATO_IPM_STATUS, RATO_IPM_SF, RATO_IPM_MU_PASSES, RATO_IPM_SEARCHING,
  RATO_IPM_PHI_T, RATO_IPM_BARRIER, RATO_IPM_OBJECTIVE, RATO_IPM_ACCEPTED
};
typedef struct rato_ipm_state {
  int32_t K, n, nI, m;
  int64_t ldv, ldm;
  const int32_t* row_slack;          /* [m] */
  double *v, *zl, *zu;               /* [K][ldv] the iterate and the bound multipliers */
  const double *vL, *vU, *curv, *lin; /* [K][ldv] bounds (nv), the objective's curvature and linear term (n) */
  double* y;                         /* [K][ldm] */
  const double* gL;                  /* [K][ldm] read on equality rows */
  double* rec;                       /* [K][RATO_IPM_REC] */
  double *Sigma, *gbar, *dv, *dzl, *dzu, *vt;      /* [K][ldv] work, length nv */
  double *gradf, *rz, *dz, *ez;                    /* [K][ldv] work, length n */
  double* diag;                                    /* [K][n]: what rato_dense_normal_matrix_f64 takes */
  double *c, *d, *w, *rs, *dyE, *r2, *q, *dy;      /* [K][ldm] work; rs on inequality rows, dyE and r2 on equality rows */
} rato_ipm_state;
size_t rato_ipm_state_bytes(void);
/* rato_ipm_g_rows_f64: g[k] = (g0[k] (m0 entries), J1 z[k] (m1 rows of the shared block J1 [m1][ld1 >= n])), g [K][ldg >= m0 + m1].
 * rato_ipm_residuals_f64 (Problem.residuals, error, the status and mu logic of solve_group, prepare_step): from g [K][ldg >= m]
 *   and JTy [K][ldj >= n] -> c, gradf, prim, dual, E0; status 'line_search' (E0 not finite) | 'converged' (E0 <= tol) |
 *   'max_iter' (last != 0); otherwise the mu loop (mu <- max(tol / 10, min(0.2 mu, mu sqrt(mu))), nu <- 0 while E_mu <= 10 mu and
 *   mu > tol / 10; mu_passes counts), then Sigma, gbar, rz, rs, dc = 1e-8 sqrt(sqrt(mu)), d, w, dw = 0, diag = Sigma_z + dw + sf curv.
 * rato_ipm_newton_f64 (newton_steps), by phase, a / b [K][ld >= the length read]:
 *   RHS     a = J'w                  dz <- -(rz + a)                 (the right-hand side; the solve turns it into dz in place)
 *   LADDER  info [K] int32, attempt  where info != 0: dw <- 1e-4 or 8 dw and diag again; status 'line_search' once attempt >= 60
 *   Q       a = J dz, first          dyE <- (a + c)_E / dc if first; r2, q
 *   R       a = W dz, b = J'q        ez <- -(rz + (a + sf curv dz) + (Sigma_z + dw) dz + b)      (solved in place into ez)
 *   UPDATE  a = J ez                 dz += ez, dyE += (a_E - r2) / dc
 *   FINISH  a = J dz                 ds, dv, dy
 * rato_ipm_step_setup_f64 (solve_group's step setup): Hdv = W dv_z [K][ldh >= n] -> dzl, dzu, a_max, a_dual, c1, Dbar, quad, the
 *   nu rule, Dphi, phi = objective + barrier + nu c1, alpha = a_max, trials = 0, searching = 1.
 * rato_ipm_trial_f64: vt <- v + alpha dv for the searching problems.
 * rato_ipm_accept_f64: gt = g(vt_z) [K][ldg >= m] -> phi_t and the Armijo test; accepted: v, y, zl, zu (the kappa_Sigma clip),
 *   iterations + 1, searching = 0; else alpha / 2, or status 'line_search' at 40 trials.
 * RATO_EINVAL without a launch on a NULL pointer, K outside [1, 65535], n < 1, nI < 0, m < 1, nI > m, ldv < n + nI, ldm < m, a
 * leading dimension below the length it serves, or an unknown phase. */
#define RATO_IPM_PHASE_RHS 0
#define RATO_IPM_PHASE_LADDER 1
#define RATO_IPM_PHASE_Q 2
#define RATO_IPM_PHASE_R 3
#define RATO_IPM_PHASE_UPDATE 4
#define RATO_IPM_PHASE_FINISH 5
int rato_ipm_g_rows_f64(int32_t K, int32_t n, const double* g0, int32_t m0, int64_t ldg0, const double* J1, int32_t m1, int64_t ld1,
                        const double* z, int64_t ldz, double* g, int64_t ldg, void* stream);
int rato_ipm_residuals_f64(const rato_ipm_state* st, const double* g, int64_t ldg, const double* JTy, int64_t ldj, int32_t last,
                           void* stream);
int rato_ipm_newton_f64(const rato_ipm_state* st, int32_t phase, const double* a, int64_t lda, const double* b, int64_t ldb,
                        const int32_t* info, int32_t flag, void* stream);
int rato_ipm_step_setup_f64(const rato_ipm_state* st, const double* Hdv, int64_t ldh, void* stream);
int rato_ipm_trial_f64(const rato_ipm_state* st, void* stream);
int rato_ipm_accept_f64(const rato_ipm_state* st, const double* gt, int64_t ldg, void* stream);

/* ---- The same phases spread over the rows (csrc/ipm_driver_grid.hip; ipm.DeviceState(vec='grid'), driver='device_grid';
 * DESIGN §7.al).  ABI: additive (RATO_ABI_VERSION stays 12).  Same state, arguments and meaning as the five entries above,
 * and the same arithmetic per entry and per sum in the same order (both forms compile csrc/rato_ipm_rows.h): every array of
 * the state, the padding and every field of rec are BITWISE what the entry above leaves, after every call, for running and
 * for ended problems, for a batch and for K = 1.  Elementwise work runs on a grid of (rato_ipm_grid_rows() rows) x (problem);
 * a scalar that needs every row is made by a stream-ordered sequence of launches (per-block extremes combined by a finishing
 * launch of one workgroup per problem; each sum by ONE workgroup that walks the full length as the workgroup form does; rec
 * written by the finishing launches alone).  Workgroups of a launch never wait for each other and none reads what another
 * one of the same launch writes; no atomics, no private memory, and the library allocates and keeps nothing.  Launches per
 * call: residuals 3, newton 1 (LADDER: 2, or 1 at flag >= 60), step_setup 3, trial 1, accept 4.
 * work: rato_ipm_grid_work_doubles(n, nI, m, K) doubles of the caller's, at least; contents irrelevant before the first call,
 * and owned by the state's calls from then on (accept applies a step exactly once through a token it keeps there).  work_len:
 * the doubles work holds.  RATO_EINVAL without a launch and with everything untouched on whatever the entries above
 * refuse, on a NULL work and on work_len below the query.  rato_ipm_grid_work_doubles: positive and non-decreasing in each
 * argument (0 for n < 1, nI < 0, m < 1 or K < 1). */
int32_t rato_ipm_grid_rows(void);
int64_t rato_ipm_grid_work_doubles(int32_t n, int32_t nI, int32_t m, int32_t K);
int rato_ipm_residuals_grid_f64(const rato_ipm_state* st, const double* g, int64_t ldg, const double* JTy, int64_t ldj, int32_t last,
                                double* work, int64_t work_len, void* stream);
int rato_ipm_newton_grid_f64(const rato_ipm_state* st, int32_t phase, const double* a, int64_t lda, const double* b, int64_t ldb,
                             const int32_t* info, int32_t flag, double* work, int64_t work_len, void* stream);
int rato_ipm_step_setup_grid_f64(const rato_ipm_state* st, const double* Hdv, int64_t ldh, double* work, int64_t work_len,
                                 void* stream);
int rato_ipm_trial_grid_f64(const rato_ipm_state* st, double* work, int64_t work_len, void* stream);
int rato_ipm_accept_grid_f64(const rato_ipm_state* st, const double* gt, int64_t ldg, double* work, int64_t work_len, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RATO_SAA_H */
