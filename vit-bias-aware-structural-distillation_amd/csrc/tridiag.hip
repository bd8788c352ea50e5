// Eigenvalue COUNTS of a symmetric fp64 matrix of order up to 2048, for the Marchenko-Pastur rank of wide token
// matrices (reference src/losses/layer_selector.py:8-20 at min(M, D) > 1024, where the Jacobi eigen-solver and the
// one-workgroup sort of basd_mp_rank stop).  The rank needs one order statistic (the lower median eigenvalue) and one
// count (eigenvalues above the noise edge): both are Sturm counts of a tridiagonal matrix with the same spectrum.
//
//   basd_sym_tridiag_f64   unblocked Householder reduction, one reflector per column, two launches per column on the
//                          caller's stream (no host sync, no grid-wide wait, no floating-point atomics: every sum has
//                          a fixed order, so two runs agree bit for bit)
//   basd_tridiag_mp_rank   one workgroup: diag / off^2 in LDS, one Sturm count per thread, 256-section inside the
//                          Gershgorin bracket, then the count above the edge
#include <float.h>

#include "basd_common.h"

namespace basd {
namespace {

constexpr int TD_MAX_N = 2048;
constexpr int TD_THREADS = 256;                   // 4 waves
constexpr int TD_WAVE_ROWS = 2;                   // rows of the trailing block per wave
constexpr int TD_ROWS = 4 * TD_WAVE_ROWS;         // ... per workgroup: 256 workgroups at n = 2048
constexpr int TD_HDR = 8;                         // workspace: [0] tau, [1] beta, [8, 8 + n) v, [8 + n, 8 + 2n) p

// Sum over the workgroup in a fixed order; every thread gets the same bits (the xor butterfly adds the same pairs in
// every lane and a + b == b + a).  Barriers on both sides: s_red may be reused right away, and LDS written before the
// call is visible after it.
__device__ __forceinline__ double block_sum(double v, double* s_red) {
  v = wave_sum_d(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
}

// Step k, launch 1.  Every workgroup rebuilds the reflector H = I - tau v v^T that maps x = A[k+1:, k] onto beta e_1 from
// ROW k of the trailing block (contiguous; A is kept symmetric bit for bit by launch 2), then forms its rows of
// p = tau A22 v.  Workgroup 0 also stores v, tau and beta for launch 2.
__global__ __launch_bounds__(TD_THREADS) void tridiag_pv_kernel(const double* __restrict__ a, int n, int k,
                                                                double* __restrict__ ws) {
  __shared__ double s_v[TD_MAX_N];
  __shared__ double s_red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = n - k - 1;                                  // order of the trailing block A22 = A[k+1:, k+1:]
  const double* x = a + (size_t)k * n + k + 1;
  double ss = 0.0;
  for (int j = tid; j < m; j += TD_THREADS) {
    const double xj = x[j];
    s_v[j] = xj;
    if (j > 0) ss = fma(xj, xj, ss);
  }
  const double xnorm2 = block_sum(ss, s_red);
  const double alpha = s_v[0];
  if (xnorm2 == 0.0) {                                      // nothing below the sub-diagonal: H = I (LAPACK dlarfg)
    if (blockIdx.x == 0 && tid == 0) { ws[0] = 0.0; ws[1] = alpha; }
    return;
  }
  const double beta = -copysign(sqrt(fma(alpha, alpha, xnorm2)), alpha);
  const double tau = (beta - alpha) / beta;
  const double scale = 1.0 / (alpha - beta);
  __syncthreads();                                          // alpha has been read
  for (int j = tid; j < m; j += TD_THREADS) {
    const double vj = (j == 0) ? 1.0 : s_v[j] * scale;
    s_v[j] = vj;
    if (blockIdx.x == 0) ws[TD_HDR + j] = vj;
  }
  if (blockIdx.x == 0 && tid == 0) { ws[0] = tau; ws[1] = beta; }
  __syncthreads();
  const int i0 = blockIdx.x * TD_ROWS + wave * TD_WAVE_ROWS;
  double acc[TD_WAVE_ROWS];
  const double* row[TD_WAVE_ROWS];
#pragma unroll
  for (int r = 0; r < TD_WAVE_ROWS; ++r) {
    acc[r] = 0.0;
    const int i = (i0 + r < m) ? i0 + r : m - 1;            // a row past the end repeats the last one (not stored)
    row[r] = a + (size_t)(k + 1 + i) * n + k + 1;
  }
  for (int j = lane; j < m; j += 64) {
    const double vj = s_v[j];
#pragma unroll
    for (int r = 0; r < TD_WAVE_ROWS; ++r) acc[r] = fma(row[r][j], vj, acc[r]);
  }
#pragma unroll
  for (int r = 0; r < TD_WAVE_ROWS; ++r) {
    const double dot = wave_sum_d(acc[r]);
    if (lane == 0 && i0 + r < m) ws[TD_HDR + n + i0 + r] = tau * dot;
  }
}

// Step k, launch 2.  Every workgroup forms s = p . v and w = p - (tau / 2) s v, then applies A22 -= v w^T + w v^T to its
// rows.  The two products are rounded separately and added, so element (i, j) and element (j, i) get the same bits:
// v_i w_j + w_i v_j is the same sum read from either side.  Workgroup 0 writes diag[k] and off[k].
__global__ __launch_bounds__(TD_THREADS) void tridiag_update_kernel(double* __restrict__ a, int n, int k,
                                                                    const double* __restrict__ ws,
                                                                    double* __restrict__ diag, double* __restrict__ off) {
  __shared__ double s_v[TD_MAX_N];
  __shared__ double s_w[TD_MAX_N];
  __shared__ double s_red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = n - k - 1;
  const double tau = ws[0];
  if (blockIdx.x == 0 && tid == 0) {
    diag[k] = a[(size_t)k * n + k];
    off[k] = ws[1];
  }
  if (tau == 0.0) return;                                   // H = I: no update (a NaN tau goes on and propagates)
  double ss = 0.0;
  for (int j = tid; j < m; j += TD_THREADS) {
    const double vj = ws[TD_HDR + j], pj = ws[TD_HDR + n + j];
    s_v[j] = vj;
    s_w[j] = pj;
    ss = fma(pj, vj, ss);
  }
  const double c = 0.5 * tau * block_sum(ss, s_red);
  for (int j = tid; j < m; j += TD_THREADS) s_w[j] = fma(-c, s_v[j], s_w[j]);
  __syncthreads();
  const int i0 = blockIdx.x * TD_ROWS + wave * TD_WAVE_ROWS;
#pragma unroll
  for (int r = 0; r < TD_WAVE_ROWS; ++r) {
    const int i = i0 + r;
    if (i >= m) break;                                      // wave-uniform
    const double vi = s_v[i], wi = s_w[i];
    double* row = a + (size_t)(k + 1 + i) * n + k + 1;
    for (int j = lane; j < m; j += 64)
      row[j] = __dsub_rn(row[j], __dadd_rn(__dmul_rn(vi, s_w[j]), __dmul_rn(wi, s_v[j])));
  }
}

// The last 2 x 2 block is tridiagonal as it stands.
__global__ void tridiag_tail_kernel(const double* __restrict__ a, int n, double* __restrict__ diag,
                                    double* __restrict__ off) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    diag[n - 2] = a[(size_t)(n - 2) * n + n - 2];
    off[n - 2] = a[(size_t)(n - 1) * n + n - 2];
    diag[n - 1] = a[(size_t)(n - 1) * n + n - 1];
  }
}

// Number of eigenvalues of the tridiagonal matrix below x: negative terms of the LDL^T pivot sequence
// q_i = (d_i - x) - e_{i-1}^2 / q_{i-1}, with the pivmin guard of LAPACK dlaebz (a pivot of at most pivmin counts as
// negative and is pushed to -pivmin, so no division by zero and a count that is monotone in x).
__device__ __forceinline__ int sturm_count(const double* s_d, const double* s_e2, int n, double x, double pivmin) {
  double q = s_d[0] - x;
  int c = 0;
  if (q <= pivmin) { ++c; q = fmin(q, -pivmin); }
  for (int i = 1; i < n; ++i) {
    q = (s_d[i] - x) - s_e2[i] / q;
    if (q <= pivmin) { ++c; q = fmin(q, -pivmin); }
  }
  return c;
}

// point j of 257 equal sections of [lo, lo + width]: one expression, so a thread's shift and the new bracket end agree
__device__ __forceinline__ double section_point(double lo, double width, int j) {
  return fma(width, (double)j / 257.0, lo);
}

__global__ __launch_bounds__(TD_THREADS) void tridiag_mp_rank_kernel(const double* __restrict__ diag,
                                                                     const double* __restrict__ off, int n, int64_t rows,
                                                                     int d, int cap, int32_t* __restrict__ rank,
                                                                     int32_t* __restrict__ status) {
  __shared__ double s_d[TD_MAX_N];
  __shared__ double s_e2[TD_MAX_N];          // s_e2[i] = off[i - 1]^2 couples rows i - 1 and i; s_e2[0] = 0
  __shared__ double s_gl[4], s_gu[4], s_em[4];
  __shared__ int s_cnt[TD_THREADS];
  __shared__ int s_bad;
  const int tid = threadIdx.x;
  if (tid == 0) s_bad = 0;
  __syncthreads();
  double gl = DBL_MAX, gu = -DBL_MAX, emax = 0.0;
  bool bad = false;
  for (int i = tid; i < n; i += TD_THREADS) {
    const double di = diag[i];
    const double el = (i > 0) ? off[i - 1] : 0.0;
    const double er = (i < n - 1) ? off[i] : 0.0;
    s_d[i] = di;
    s_e2[i] = el * el;
    bad |= !(fabs(di) <= DBL_MAX) || !(fabs(er) <= DBL_MAX);
    const double r = fabs(el) + fabs(er);                   // Gershgorin disc of row i
    gl = fmin(gl, di - r);
    gu = fmax(gu, di + r);
    emax = fmax(emax, el * el);
  }
  if (bad) s_bad = 1;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    gl = fmin(gl, __shfl_xor(gl, o, 64));
    gu = fmax(gu, __shfl_xor(gu, o, 64));
    emax = fmax(emax, __shfl_xor(emax, o, 64));
  }
  if ((tid & 63) == 0) { s_gl[tid >> 6] = gl; s_gu[tid >> 6] = gu; s_em[tid >> 6] = emax; }
  __syncthreads();
  if (s_bad) {                                              // a NaN / Inf spectrum counts 0, like basd_mp_rank
    if (tid == 0) {
      rank[0] = 0;
      if (status) atomicOr(status, BASD_STATUS_NONFINITE);
    }
    return;
  }
  gl = fmin(fmin(s_gl[0], s_gl[1]), fmin(s_gl[2], s_gl[3]));
  gu = fmax(fmax(s_gu[0], s_gu[1]), fmax(s_gu[2], s_gu[3]));
  emax = fmax(fmax(s_em[0], s_em[1]), fmax(s_em[2], s_em[3]));
  const double pivmin = DBL_MIN * fmax(1.0, emax);
  const double radius = gu - gl;
  const double margin = 2.0 * fmax(fabs(gl), fabs(gu)) * DBL_EPSILON * (double)n + 4.0 * pivmin;
  double lo = gl - margin, hi = gu + margin;                // count(lo) = 0, count(hi) = n
  const int want = (n - 1) / 2 + 1;                         // lambda_t, t = (n - 1) / 2 ascending: first x with count >= t + 1
  const double tolw = ldexp(radius, -48);
  for (int round = 0; round < 8; ++round) {                 // 257^7 > 2^53: the bound is never what stops a finite input
    const double width = hi - lo;
    if (width <= tolw) break;
    s_cnt[tid] = sturm_count(s_d, s_e2, n, section_point(lo, width, tid + 1), pivmin);
    __syncthreads();
    int first = TD_THREADS;                                 // first of the 256 shifts with at least `want` below it
    for (int j = 0; j < TD_THREADS; ++j)
      if (s_cnt[j] >= want) { first = j; break; }
    const double nlo = (first > 0) ? section_point(lo, width, first) : lo;
    const double nhi = (first < TD_THREADS) ? section_point(lo, width, first + 1) : hi;
    lo = nlo;
    hi = nhi;
    __syncthreads();
  }
  if (tid == 0) {
    const double med = 0.5 * (lo + hi);
    const double sigma2 = med / (double)rows;               // eigenvalues of the Gram / rows (layer_selector.py:13-15)
    const double sq = 1.0 + sqrt((double)d / (double)rows);
    const double edge = sigma2 * sq * sq;
    const int above = n - sturm_count(s_d, s_e2, n, edge * (double)rows, pivmin);
    rank[0] = above < cap ? above : cap;
    // rank 0 makes the reference divide by sum(sw) = 0 (layer_selector.py:105)
    if (status && above == 0) atomicOr(status, BASD_STATUS_RANK0);
  }
}

}  // namespace
}  // namespace basd

extern "C" int64_t basd_sym_tridiag_f64_workspace_bytes(int n) {
  return (int64_t)sizeof(double) * (basd::TD_HDR + 2 * (int64_t)(n > 0 ? n : 0));
}

extern "C" int basd_sym_tridiag_f64(double* a, int n, double* diag, double* off, void* work, void* stream) {
  using namespace basd;
  if (n < 2 || n > TD_MAX_N) return fail(BASD_ERR_SHAPE, "sym_tridiag_f64: n=%d outside 2 .. %d", n, TD_MAX_N);
  hipStream_t st = (hipStream_t)stream;
  double* ws = (double*)work;
  for (int k = 0; k + 2 < n; ++k) {
    const int blocks = (n - k - 1 + TD_ROWS - 1) / TD_ROWS;
    hipLaunchKernelGGL(tridiag_pv_kernel, dim3(blocks), dim3(TD_THREADS), 0, st, a, n, k, ws);
    hipLaunchKernelGGL(tridiag_update_kernel, dim3(blocks), dim3(TD_THREADS), 0, st, a, n, k, ws, diag, off);
  }
  hipLaunchKernelGGL(tridiag_tail_kernel, dim3(1), dim3(64), 0, st, a, n, diag, off);
  return check_launch("sym_tridiag_f64");
}

extern "C" int basd_tridiag_mp_rank(const double* diag, const double* off, int n, int64_t rows, int d, int cap,
                                    int32_t* rank, int32_t* status, void* stream) {
  using namespace basd;
  if (n < 2 || n > TD_MAX_N) return fail(BASD_ERR_SHAPE, "tridiag_mp_rank: n=%d outside 2 .. %d", n, TD_MAX_N);
  if (rows < 1 || d < 1 || (int64_t)n > rows || n > d)
    return fail(BASD_ERR_SHAPE, "tridiag_mp_rank: n=%d is not the smaller side of a [%lld, %d] matrix", n, (long long)rows, d);
  hipLaunchKernelGGL(tridiag_mp_rank_kernel, dim3(1), dim3(TD_THREADS), 0, (hipStream_t)stream, diag, off, n, rows, d, cap,
                     rank, status);
  return check_launch("tridiag_mp_rank");
}
