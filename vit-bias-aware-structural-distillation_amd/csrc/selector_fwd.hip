// Forward of the Grassmannian layer selector as two C entries (reference src/losses/layer_selector.py:69-74, 84-108,
// 133-138): the frames of one side (teacher or student) from its Gram statistics, and the mixing weights from both
// frames.  Rounds 1 - 4 ran this as a torch composition around the kernels (zero-fills, centring, cat, rank masks, an
// einsum and two library fp32 matmuls on the step's own chain).
//
//   basd_selector_frames   centring -> basd_pchol_f64 -> basd_jacobi_svd [-> sigma^2 -> basd_mp_rank] -> w0 / sigma,
//                          rank masks, lam = sigma^2 in fp64
//   basd_selector_weights  A = V_s V_t^T (epilogue: A_bar into the Jacobi layout + the active-block array),
//                          X = A A_bar^T, rank-masked basd_jacobi_svd, basd_angle_weights,
//                          Phi = vec^T diag(coef) vec (coef on the operand load), T = X Phi (epilogue: rows b >= k_j)
//
// The four products are batched fp32 GEMMs on the fp32-input MFMA (v_mfma_f32_16x16x4_f32: a k-ordered fp32 fma chain,
// the numerics class of an fp32 torch.matmul), one launch each over the whole E L batch.
#include "basd_common.h"

namespace basd {

// ---------------------------------------------------------------------------------------------
// batched fp32 product  C[p](r, c) = sum_k opA[p](r, k) opB[p](c, k)
// Operand element (r, k) of batch p = i L + j lives at ptr[i * si + j * sj + r * sr + k * sk] (any strides: row-major,
// transposed and Jacobi-layout operands all go through the same loader), optionally multiplied on load by
// kscale[i * ksi + j * ksj + k].
struct SelOperand {
  const float* ptr;
  int64_t si, sj, sr, sk;
  const float* kscale;
  int64_t ksi, ksj;
};

// Output element (r, c) of batch p at ptr[i * si + j * sj + r * sr + c * sc].  mask: 0 none, 1 keep rows r < ranks[j],
// 2 keep rows r >= ranks[j] (the others are written as the value times 0, as the torch composition multiplied by its
// keep mask).  pad_rows > M: rows [M, pad_rows) of the columns are written as zeros (the Jacobi layout's padding).
struct SelOutput {
  float* ptr;
  int64_t si, sj, sr, sc;
  int mask;
  int pad_rows;
};

constexpr int SEL_TILE = 64;      // output tile per workgroup (4 waves, 32 x 32 each)
constexpr int SEL_KT = 16;        // k per LDS stage
constexpr int SEL_LDS_LD = SEL_TILE + 4;

__device__ __forceinline__ void sel_load_tile(const SelOperand& op, int i, int j, int r0, int k0, int rows, int K,
                                              float (*dst)[SEL_LDS_LD]) {
  const float* base = op.ptr + (int64_t)i * op.si + (int64_t)j * op.sj;
  const float* ks = op.kscale ? op.kscale + (int64_t)i * op.ksi + (int64_t)j * op.ksj : nullptr;
  const int t = threadIdx.x;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    int r, k;
    if (op.sk == 1) {                 // k contiguous: lanes along k
      k = t & 15;
      r = (t >> 4) + 16 * q;
    } else {                          // rows contiguous: lanes along r
      r = t & 63;
      k = (t >> 6) + 4 * q;
    }
    const int gr = r0 + r, gk = k0 + k;
    float v = 0.f;
    if (gr < rows && gk < K) {
      v = base[(int64_t)gr * op.sr + (int64_t)gk * op.sk];
      if (ks) v *= ks[gk];
    }
    dst[k][r] = v;
  }
}

__global__ __launch_bounds__(256) void sel_bgemm_kernel(SelOperand A, SelOperand B, int L, int M, int N, int K,
                                                        SelOutput o1, SelOutput o2, const int32_t* __restrict__ ranks,
                                                        int32_t* __restrict__ active) {
  __shared__ float As[SEL_KT][SEL_LDS_LD];
  __shared__ float Bs[SEL_KT][SEL_LDS_LD];
  using f4 = __attribute__((ext_vector_type(4))) float;
  const int p = blockIdx.z, i = p / L, j = p - (p / L) * L;
  const int r0 = blockIdx.y * SEL_TILE, c0 = blockIdx.x * SEL_TILE;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
  f4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = f4{0.f, 0.f, 0.f, 0.f};

  for (int k0 = 0; k0 < K; k0 += SEL_KT) {
    sel_load_tile(A, i, j, r0, k0, M, K, As);
    sel_load_tile(B, i, j, c0, k0, N, K, Bs);
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < SEL_KT; kk += 4) {
      // 16x16x4: lane l holds A[row l & 15][k l >> 4] and B[k l >> 4][col l & 15]
      const int kr = kk + (lane >> 4);
      float a0 = As[kr][wr + (lane & 15)], a1 = As[kr][wr + 16 + (lane & 15)];
      float b0 = Bs[kr][wc + (lane & 15)], b1 = Bs[kr][wc + 16 + (lane & 15)];
      acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }

  const int kj = ranks ? ranks[j] : 0;
  // C/D layout: col = lane & 15, row = 4 (lane >> 4) + reg
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int r = r0 + wr + 16 * a + 4 * (lane >> 4) + reg, c = c0 + wc + 16 * b + (lane & 15);
        if (r >= M || c >= N) continue;
        const float v = acc[a][b][reg];
#pragma unroll
        for (int w = 0; w < 2; ++w) {
          const SelOutput& o = w == 0 ? o1 : o2;
          if (o.ptr == nullptr) continue;
          const float keep = o.mask == 1 ? (r < kj ? 1.f : 0.f) : o.mask == 2 ? (r >= kj ? 1.f : 0.f) : 1.f;
          o.ptr[(int64_t)i * o.si + (int64_t)j * o.sj + (int64_t)r * o.sr + (int64_t)c * o.sc] = o.mask ? v * keep : v;
        }
      }
  // padding rows of the Jacobi layout, and the active-block array, from the workgroups that own them
  if (blockIdx.y == gridDim.y - 1) {
#pragma unroll
    for (int w = 0; w < 2; ++w) {
      const SelOutput& o = w == 0 ? o1 : o2;
      if (o.ptr == nullptr || o.pad_rows <= M) continue;
      const int np = o.pad_rows - M;
      for (int e = threadIdx.x; e < np * SEL_TILE; e += 256) {
        const int r = M + e / SEL_TILE, c = c0 + e % SEL_TILE;
        if (c < N) o.ptr[(int64_t)i * o.si + (int64_t)j * o.sj + (int64_t)r * o.sr + (int64_t)c * o.sc] = 0.f;
      }
    }
  }
  if (active != nullptr && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) active[p] = kj;
}

int sel_bgemm(const SelOperand& a, const SelOperand& b, int E, int L, int M, int N, int K, const SelOutput& o1,
              const SelOutput& o2, const int32_t* ranks, int32_t* active, hipStream_t st, const char* what) {
  dim3 grid((N + SEL_TILE - 1) / SEL_TILE, (M + SEL_TILE - 1) / SEL_TILE, E * L);
  hipLaunchKernelGGL(sel_bgemm_kernel, grid, dim3(256), 0, st, a, b, L, M, N, K, o1, o2, ranks, active);
  return check_launch(what);
}

// ---------------------------------------------------------------------------------------------
// frames glue
// centred Gram  cen = unc - csum csum^T / m  (lower triangles only: all the pivoted Cholesky reads).  with_unc: the
// uncentred matrices are copied in front (batch [unc; cen] of 2 n problems, one factorisation / Jacobi launch).
__global__ __launch_bounds__(256) void sel_centre_kernel(const double* __restrict__ unc, const double* __restrict__ csum,
                                                         int n, int D, double m, int with_unc, double* __restrict__ out,
                                                         int32_t* __restrict__ status) {
  const int r = blockIdx.x, b = blockIdx.y;
  const double* u = unc + ((int64_t)b * D + r) * D;
  const double* cs = csum + (int64_t)b * D;
  double* cen = out + (((int64_t)(with_unc ? n + b : b)) * D + r) * D;
  double* cp = out + ((int64_t)b * D + r) * D;
  const double cr = cs[r];
  bool bad = false;
  for (int c = threadIdx.x; c <= r; c += 256) {
    const double v = u[c];
    cen[c] = v - cr * cs[c] / m;
    if (with_unc) cp[c] = v;
    bad |= !isfinite(v) || !isfinite(cs[c]);
  }
  // a non-finite Gram entry (NaN / Inf tokens) ends the pivoted Cholesky at rank 0, so neither the Jacobi nor the rank
  // count would see it: flag it here
  if (status != nullptr && __any(bad) && (threadIdx.x & 63) == 0) atomicOr((int*)status, BASD_STATUS_NONFINITE);
}

__global__ __launch_bounds__(256) void sel_square_kernel(const float* __restrict__ sigma, int64_t count,
                                                         float* __restrict__ evals) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < count) evals[e] = sigma[e] * sigma[e];
}

// row m of matrix b: v = w0 column m / sigma_m (zero where sigma_m = 0), lam = sigma^2 in fp64; with ranks, v rows and
// sigma entries m >= k_b are multiplied by 0 (the torch composition's keep mask)
__global__ __launch_bounds__(256) void sel_finish_kernel(const float* __restrict__ w0, const float* __restrict__ sig,
                                                         int D, int ld, const int32_t* __restrict__ ranks,
                                                         float* __restrict__ sigma_out, double* __restrict__ lam,
                                                         float* __restrict__ v) {
  const int m = blockIdx.x, b = blockIdx.y;
  const float s = sig[(int64_t)b * D + m];
  const float keep = ranks ? (m < ranks[b] ? 1.f : 0.f) : 1.f;
  const float* col = w0 + ((int64_t)b * D + m) * ld;
  float* row = v + ((int64_t)b * D + m) * D;
  const float safe = fmaxf(s, 1e-30f);
  for (int c = threadIdx.x; c < D; c += 256) {
    const float x = s > 0.f ? col[c] / safe : 0.f;
    row[c] = ranks ? x * keep : x;
  }
  if (threadIdx.x == 0) {
    sigma_out[(int64_t)b * D + m] = ranks ? s * keep : s;
    if (lam) lam[(int64_t)b * D + m] = (double)s * (double)s;
  }
}

inline int jacobi_ld_of(int n) {
  int ld = (n + 3) / 4 * 4;
  if (ld % 32 == 0) ld += 4;
  return ld;
}

inline int64_t al256(int64_t b) { return (b + 255) & ~(int64_t)255; }

// workspace carving: each piece 256-byte aligned
struct Carver {
  uintptr_t p;
  template <class T> T* take(int64_t count) {
    T* r = reinterpret_cast<T*>(p);
    p += (uintptr_t)al256(count * (int64_t)sizeof(T));
    return r;
  }
};

}  // namespace basd

// ---------------------------------------------------------------------------------------------
extern "C" int64_t basd_selector_frames_workspace_bytes(int n, int D) {
  using namespace basd;
  if (n < 1 || D < 1) return 256;
  const int64_t nb = 2 * (int64_t)n, ld = jacobi_ld_of(D);
  return 256 + al256(nb * D * D * 8) * 2 + al256(nb * D * ld * 4) + al256(nb * D * 4) * 2 + al256(nb * 4) * 2 +
         al256((int64_t)n * D * 4);
}

extern "C" int basd_selector_frames(const double* unc, const double* csum, int n, int64_t m_rows, int D, int with_ranks,
                                    int32_t* ranks, float* sigma, double* lam, float* v, int32_t* status,
                                    void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace basd;
  if (n <= 0) return BASD_OK;
  if (D < 1 || D > 192 || m_rows < 1)
    return fail(BASD_ERR_SHAPE, "selector_frames: D=%d (1 .. 192) m_rows=%lld", D, (long long)m_rows);
  if (workspace == nullptr || workspace_bytes < basd_selector_frames_workspace_bytes(n, D))
    return fail(BASD_ERR_WORKSPACE, "selector_frames: workspace of %lld bytes, need %lld", (long long)workspace_bytes,
                (long long)basd_selector_frames_workspace_bytes(n, D));
  if (!unc || !csum || !sigma || !v || (with_ranks && !ranks))
    return fail(BASD_ERR_SHAPE, "selector_frames: a required pointer is NULL");
  const int nb = with_ranks ? 2 * n : n, ld = jacobi_ld_of(D);
  Carver cv{(((uintptr_t)workspace) + 255) & ~(uintptr_t)255};
  double* a2 = cv.take<double>((int64_t)2 * n * D * D);
  double* lwork = cv.take<double>((int64_t)2 * n * D * D);
  float* w0 = cv.take<float>((int64_t)2 * n * D * ld);
  int32_t* piv = cv.take<int32_t>((int64_t)2 * n * D);
  float* sig = cv.take<float>((int64_t)2 * n * D);
  int32_t* prank = cv.take<int32_t>(2 * n);
  int32_t* sweeps = cv.take<int32_t>(2 * n);
  float* evals = cv.take<float>((int64_t)n * D);
  hipStream_t st = (hipStream_t)stream;

  hipLaunchKernelGGL(sel_centre_kernel, dim3(D, n), dim3(256), 0, st, unc, csum, n, D, (double)m_rows, with_ranks, a2,
                     status);
  int rc = check_launch("selector_frames (centring)");
  if (rc) return rc;
  rc = basd_pchol_f64(a2, nb, D, 1e-13, nullptr, w0, ld, lwork, piv, prank, stream);
  if (rc) return rc;
  // the Jacobi's defaults of the Python binding: tol = sqrt(m) 2^-24, 60 sweeps, sorted
  rc = basd_jacobi_svd(w0, nb, D, D, ld, D, sqrtf((float)D) * 5.96e-8f, 60, 1, sig, sweeps, nullptr, 0, status, stream);
  if (rc) return rc;
  const int64_t off = with_ranks ? (int64_t)n * D : 0;        // the centred half
  if (with_ranks) {
    // MP rank from the uncentred spectra (eigenvalues = sigma^2 in fp32), capped at D - 1
    hipLaunchKernelGGL(sel_square_kernel, dim3((unsigned)(((int64_t)n * D + 255) / 256)), dim3(256), 0, st, sig,
                       (int64_t)n * D, evals);
    rc = check_launch("selector_frames (spectra)");
    if (rc) return rc;
    rc = basd_mp_rank(evals, n, D, m_rows, D, D - 1, ranks, status, stream);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(sel_finish_kernel, dim3(D, n), dim3(256), 0, st, w0 + off * ld, sig + off, D, ld,
                     with_ranks ? (const int32_t*)ranks : nullptr, sigma, lam, v);
  return check_launch("selector_frames (normalise / mask)");
}

extern "C" int64_t basd_selector_weights_workspace_bytes(int E, int L, int D) {
  using namespace basd;
  if (E < 1 || L < 1 || D < 1) return 256;
  const int64_t P = (int64_t)E * L, ld = jacobi_ld_of(D);
  return 256 + al256(P * D * D * 4) * 2 + al256(P * D * ld * 4) + al256(P * D * 4) * 2 + al256(P * 4) * 2;
}

extern "C" int basd_selector_weights(const float* v_s, const int32_t* ranks, const float* vm_t, const float* sw,
                                     const float* log_temp, int E, int L, int D, float* weights, float* pre, float* d2,
                                     float* t_seed, int32_t* status, void* workspace, int64_t workspace_bytes,
                                     void* stream) {
  using namespace basd;
  if (E <= 0 || L <= 0) return BASD_OK;
  if (L > 64 || D < 1 || D > 192)
    return fail(BASD_ERR_SHAPE, "selector_weights: L=%d (<= 64) D=%d (1 .. 192)", L, D);
  if (workspace == nullptr || workspace_bytes < basd_selector_weights_workspace_bytes(E, L, D))
    return fail(BASD_ERR_WORKSPACE, "selector_weights: workspace of %lld bytes, need %lld", (long long)workspace_bytes,
                (long long)basd_selector_weights_workspace_bytes(E, L, D));
  if (!v_s || !ranks || !vm_t || !sw || !log_temp || !weights || !pre || !d2 || !t_seed)
    return fail(BASD_ERR_SHAPE, "selector_weights: a required pointer is NULL");
  const int ld = jacobi_ld_of(D);
  const int64_t P = (int64_t)E * L, dd = (int64_t)D * D, dl = (int64_t)D * ld;
  Carver cv{(((uintptr_t)workspace) + 255) & ~(uintptr_t)255};
  float* a_full = cv.take<float>(P * dd);        // A = V_s V_t^T; later Phi
  float* x = cv.take<float>(P * dd);             // A A_bar^T
  float* w = cv.take<float>(P * dl);             // A_bar in the Jacobi layout: w[p, c, b] = A_bar[b, c]
  float* sig = cv.take<float>(P * D);
  float* coef = cv.take<float>(P * D);
  int32_t* active = cv.take<int32_t>(P);
  int32_t* sweeps = cv.take<int32_t>(P);
  hipStream_t st = (hipStream_t)stream;
  const SelOutput none{nullptr, 0, 0, 0, 0, 0, 0};

  // A_full[i, j](b, c) = sum_d v_s[i](b, d) vm_t[j](c, d); epilogue: the row-masked copy into the Jacobi layout
  int rc = sel_bgemm(SelOperand{v_s, dd, 0, D, 1, nullptr, 0, 0}, SelOperand{vm_t, 0, dd, D, 1, nullptr, 0, 0}, E, L, D,
                     D, D, SelOutput{a_full, L * dd, dd, D, 1, 0, 0}, SelOutput{w, L * dl, dl, 1, ld, 1, ld}, ranks,
                     active, st, "selector_weights (A = V_s V_t^T)");
  if (rc) return rc;
  // X(b, e) = sum_c A(b, c) A_bar(e, c), A_bar(e, c) = w[c, e]  (before the Jacobi rotates w in place)
  rc = sel_bgemm(SelOperand{a_full, L * dd, dd, D, 1, nullptr, 0, 0}, SelOperand{w, L * dl, dl, 1, ld, nullptr, 0, 0},
                 E, L, D, D, D, SelOutput{x, L * dd, dd, D, 1, 0, 0}, none, nullptr, nullptr, st,
                 "selector_weights (A A_bar^T)");
  if (rc) return rc;
  // cosines of the principal angles: only the leading k_j x k_j block of pair (i, j) is non-zero
  rc = basd_jacobi_svd(w, (int)P, D, D, ld, D, sqrtf((float)D) * 5.96e-8f, 60, 1, sig, sweeps, active, 1, status,
                       stream);
  if (rc) return rc;
  // columns of w are now sigma_m u_m (un-normalised)
  rc = basd_angle_weights(sig, sw, log_temp, E, L, D, 1, d2, pre, weights, coef, stream);
  if (rc) return rc;
  // Phi(b, c) = sum_m coef_m vec(m, b) vec(m, c), vec(m, b) = w[m, b]  (into A_full's buffer)
  float* phi = a_full;
  rc = sel_bgemm(SelOperand{w, L * dl, dl, 1, ld, coef, L * D, D}, SelOperand{w, L * dl, dl, 1, ld, nullptr, 0, 0}, E,
                 L, D, D, D, SelOutput{phi, L * dd, dd, D, 1, 0, 0}, none, nullptr, nullptr, st,
                 "selector_weights (Phi)");
  if (rc) return rc;
  // T(b, a) = sum_e X(b, e) Phi(e, a), rows b >= k_j only
  return sel_bgemm(SelOperand{x, L * dd, dd, D, 1, nullptr, 0, 0}, SelOperand{phi, L * dd, dd, 1, D, nullptr, 0, 0}, E,
                   L, D, D, D, SelOutput{t_seed, L * dd, dd, D, 1, 2, 0}, none, ranks, nullptr, st,
                   "selector_weights (T = X Phi)");
}
