// Risk statistics of K rows of Z [K][ldz], every row with its OWN alpha (rato_risk_stats_rows, gfx950): the K exact
// selections behind a batched rollout (rato_*_eval_batch: K solutions on one validation batch) whatever the alphas of the
// rows are and whatever M is -- 1 launch of K workgroups while a row fits the one-workgroup form (M <= RS_SMALL_MAX),
// 5 stream-ordered launches over (workgroups of a row) x (rows) beyond.
//
// Nothing here is new arithmetic: the kernels are the bodies of rato_select.h (rs_small_body; rs_pass1_body ..
// rs_final_body, the text stats.hip's single-row kernels compile from) on row blockIdx.y with that row's own Workspace.
// The alphas are read from a DEVICE array and every workgroup ranks its row itself (stats_rank: the host rule, IEEE-exact
// on both sides), so nothing is uploaded and the call can be captured.  The launch-per-pass form waits for nothing inside
// a launch and has no co-residency requirement: the grid over rows needs no new synchronisation.  Integer atomics only;
// the fp64 partials of a row are folded by one wave in a fixed order (rs_final_body) -- deterministic run to run.
//
// Workgroups per row: rs_pass_blocks(M), the single-row rule.  Its 256-workgroup knee was measured for ONE row (global
// atomic contention on the few occupied bins of the row's histograms).  With K rows the histograms are per row, so the
// number of workgroups adding to one address is unchanged; what grows is the total number of atomics in flight.
#include "rato_common.h"
#include "rato_select.h"

namespace {
using namespace rato_sel;

__device__ __forceinline__ bool alpha_valid(double alpha) { return alpha > 0.0 && alpha <= 1.0; }   // (NaN: false)

// K workgroups: workgroup r is rs_small on row r at alphas[r] (stats.hip: rs_small_batch with the row's own alpha)
__global__ __launch_bounds__(RS1_T) void rs_rows_small(const float* __restrict__ Z, long M, long ldz,
                                                       const double* __restrict__ alphas, float thr, double* __restrict__ out) {
  __shared__ unsigned h[B1];
  __shared__ double red[5 * (RS1_T / RATO_WAVE)];
  __shared__ float redmax[RS1_T / RATO_WAVE];
  const double alpha = alphas[blockIdx.x];
  double* o = out + (size_t)blockIdx.x * RATO_N_STATS;
  if (!alpha_valid(alpha)) {   // uniform over the workgroup
    if (threadIdx.x < RATO_N_STATS) o[threadIdx.x] = __longlong_as_double(0x7ff8000000000000LL);
    return;
  }
  unsigned k;
  int var_is_max;
  stats_rank(M, alpha, k, var_is_max);
  rs_small_body<RS1_T>(Z + (size_t)blockIdx.x * ldz, M, alpha, k, var_is_max, thr, o, nullptr, h, red, redmax);
}

// ---- the pass form: workgroup (b, r) is workgroup b of row r's single-row launch.  A row with an invalid alpha skips
// its passes (nothing is added to its histograms); rs_rows_final leaves them zeroed and writes its NaN record.
__global__ __launch_bounds__(RATO_BLOCK) void rs_rows_pass1(const float* __restrict__ Z, long M, long ldz,
                                                            const double* __restrict__ alphas, float thr, Workspace* __restrict__ ws) {
  if (!alpha_valid(alphas[blockIdx.y])) return;
  rs_pass1_body(Z + (size_t)blockIdx.y * ldz, M, thr, ws + blockIdx.y, (int)blockIdx.x, (int)gridDim.x);
}

__global__ __launch_bounds__(RATO_BLOCK) void rs_rows_pass2(const float* __restrict__ Z, long M, long ldz,
                                                            const double* __restrict__ alphas, Workspace* __restrict__ ws) {
  const double alpha = alphas[blockIdx.y];
  if (!alpha_valid(alpha)) return;
  unsigned k;
  int var_is_max;
  stats_rank(M, alpha, k, var_is_max);
  rs_pass2_body(Z + (size_t)blockIdx.y * ldz, M, k, ws + blockIdx.y, (int)blockIdx.x, (int)gridDim.x);
}

__global__ __launch_bounds__(RATO_BLOCK) void rs_rows_pass3(const float* __restrict__ Z, long M, long ldz,
                                                            const double* __restrict__ alphas, Workspace* __restrict__ ws) {
  const double alpha = alphas[blockIdx.y];
  if (!alpha_valid(alpha)) return;
  unsigned k;
  int var_is_max;
  stats_rank(M, alpha, k, var_is_max);
  rs_pass3_body(Z + (size_t)blockIdx.y * ldz, M, k, ws + blockIdx.y, (int)blockIdx.x, (int)gridDim.x);
}

__global__ __launch_bounds__(RATO_BLOCK) void rs_rows_tail(const float* __restrict__ Z, long M, long ldz,
                                                           const double* __restrict__ alphas, Workspace* __restrict__ ws) {
  const double alpha = alphas[blockIdx.y];
  if (!alpha_valid(alpha)) return;
  unsigned k;
  int var_is_max;
  stats_rank(M, alpha, k, var_is_max);
  rs_tail_body(Z + (size_t)blockIdx.y * ldz, M, k, ws + blockIdx.y, (int)blockIdx.x, (int)gridDim.x);
}

// K workgroups: workgroup r folds row r's partials (same wave, same order as rs_final) and zeroes its histograms
__global__ __launch_bounds__(RATO_BLOCK) void rs_rows_final(long M, const double* __restrict__ alphas, int nblocks,
                                                            Workspace* __restrict__ ws, double* __restrict__ out) {
  const double alpha = alphas[blockIdx.x];
  const bool valid = alpha_valid(alpha);
  unsigned k = 0;
  int var_is_max = 0;
  if (valid) stats_rank(M, alpha, k, var_is_max);
  rs_final_body(M, alpha, k, var_is_max, nblocks, ws + blockIdx.x, out + (size_t)blockIdx.x * RATO_N_STATS, valid);
}

// workgroup i: zero and tag Workspace i
__global__ __launch_bounds__(RATO_BLOCK) void rs_rows_init_kernel(Workspace* __restrict__ ws) { rs_init_body(ws + blockIdx.x); }

bool rows_shape_ok(int64_t M, int32_t K) { return K >= 1 && K <= 65535 && M > 0 && M < (int64_t)0xffffffffLL; }
}  // namespace

extern "C" size_t rato_risk_stats_rows_workspace_bytes(int64_t M, int32_t K) {
  if (!rows_shape_ok(M, K) || M <= RS_SMALL_MAX) return 0;
  return (size_t)K * sizeof(Workspace);
}

extern "C" int rato_risk_stats_rows_plan(int64_t M, int32_t K, int32_t* launches, int32_t* blocks_per_row) {
  if (!rows_shape_ok(M, K)) return RATO_EINVAL;
  const bool small = M <= RS_SMALL_MAX;
  if (launches) *launches = small ? 1 : 5;
  if (blocks_per_row) *blocks_per_row = small ? 1 : (int32_t)rs_pass_blocks(M);
  return RATO_OK;
}

extern "C" int rato_risk_stats_rows_init(void* workspace, size_t workspace_bytes, void* stream) {
  RATO_CLEAR_ERROR();
  const size_t n = workspace_bytes / sizeof(Workspace);
  if (!workspace || n < 1 || n > 0x7fffffffu) return RATO_EINVAL;
  hipLaunchKernelGGL(rs_rows_init_kernel, dim3((unsigned)n), dim3(RATO_BLOCK), 0, rato::as_stream(stream),
                     static_cast<Workspace*>(workspace));
  RATO_LAUNCH_CHECK();
  return RATO_OK;
}

extern "C" int rato_risk_stats_rows(const float* Z, int64_t M, int64_t ldz, int32_t K, const double* alphas, float thr,
                                    void* workspace, size_t workspace_bytes, double* out, void* stream) {
  RATO_CLEAR_ERROR();
  if (!Z || !alphas || !out || !rows_shape_ok(M, K) || ldz < M) return RATO_EINVAL;
  hipStream_t st = rato::as_stream(stream);
  if (M <= RS_SMALL_MAX) {   // ONE launch; no workspace is read
    hipLaunchKernelGGL(rs_rows_small, dim3((unsigned)K), dim3(RS1_T), 0, st, Z, (long)M, (long)ldz, alphas, thr, out);
    RATO_LAUNCH_CHECK();
    return RATO_OK;
  }
  if (!workspace || workspace_bytes < (size_t)K * sizeof(Workspace)) return RATO_EINVAL;
  Workspace* ws = static_cast<Workspace*>(workspace);
  const long nb = rs_pass_blocks(M);
  const dim3 grid((unsigned)nb, (unsigned)K), block(RATO_BLOCK);
  hipLaunchKernelGGL(rs_rows_pass1, grid, block, 0, st, Z, (long)M, (long)ldz, alphas, thr, ws);
  hipLaunchKernelGGL(rs_rows_pass2, grid, block, 0, st, Z, (long)M, (long)ldz, alphas, ws);
  hipLaunchKernelGGL(rs_rows_pass3, grid, block, 0, st, Z, (long)M, (long)ldz, alphas, ws);
  hipLaunchKernelGGL(rs_rows_tail, grid, block, 0, st, Z, (long)M, (long)ldz, alphas, ws);
  hipLaunchKernelGGL(rs_rows_final, dim3((unsigned)K), block, 0, st, (long)M, alphas, (int)nb, ws, out);
  RATO_LAUNCH_CHECK();
  return RATO_OK;
}
