// Batched one-sided (Hestenes) Jacobi SVD, one matrix per workgroup, the columns
// resident in registers (column-major, fp32).  Replaces the torch.linalg.svd /
// svdvals / eigvalsh / matrix_norm('nuc') calls of the reference loss path
// (src/losses/layer_selector.py:16,36,92,99; src/losses/relational.py:48).
//
// Layout: column c at W + c*ld, rows 0..m-1 significant, rows m..ld-1 zero.
// Two kernels, chosen by shape alone in basd_jacobi_svd at the end of this file (DESIGN.md has the route table): the
// block kernel with scaled rotations in its hex-block or quad-block ordering for up to 196 columns, odd-even ordering
// of single columns for everything else that is accepted.
#include <type_traits>
#include "basd_common.h"

namespace basd {

// floor of the squared-norm product in the rotation test (gamma / tol)^2 > max(alpha beta, TINY): below it the product
// is denormal or flushed (both columns under 1e-19: under-scaled input) and the "cosine" would be the quotient of two
// underflowed numbers
#define BASD_JACOBI_TINY 1.0e-37f
// Debris: a column whose squared norm has fallen below DEBRIS x the largest of its matrix (norm ratio 1e-10) is the
// rounding residue of a cancelled direction (rank-deficient input: the pivoted Cholesky factors these kernels are fed
// keep every real column above 3e-7 of the largest).  Its direction is noise, so its cosines with the real columns are
// O(1) again after every rotation that shrinks it: left in the game it asks for LARGE rotations sweep after sweep until
// it underflows (measured: 192 columns of rank 96 used all 40 sweeps).  Such columns are set to zero at the start of a
// sweep (the exact norms and the largest of them are at hand there): sigma = 0, never rotated again.
#define BASD_JACOBI_DEBRIS 1.0e-20f

// Health word (optional, one int32 per launch set, OR-ed with atomics): BASD_STATUS_NONCONVERGED when a matrix used
// all max_sweeps sweeps and was still rotating, BASD_STATUS_NONFINITE when a singular value is NaN / Inf (a NaN input
// makes every rotation test false, so such a matrix "converges" at once and would otherwise pass silently).
// Bits 8 .. 27 of the word are diagnostics of a non-converged solve (informational; OR-ed like the rest, so exact
// for the usual single offender): bits 8-11 the kernel variant (2 / 3 odd-even with a double / single mailbox, 6 quad-block,
// 7 hex-block; 1, 4, 5 belonged to retired kernels), bits 12-27 the matrix index (saturating at 65535).
__device__ __forceinline__ void report_status(int32_t* status, bool converged, const float* s_sig, int n, int tid,
                                              int nthreads, int kind, int mat) {
  if (!status) return;
  int st = 0;
  for (int c = tid; c < n; c += nthreads) {
    const float v = s_sig[c];
    if (!(v == v) || v > 3.0e38f) st |= BASD_STATUS_NONFINITE;
  }
  if (tid == 0 && !converged) st |= BASD_STATUS_NONCONVERGED | ((kind & 15) << 8) | ((mat > 65535 ? 65535 : mat) << 12);
  if (st) atomicOr(status, st);
}

// ---------------------------------------------------------------------------------------------
// Odd-even transposition ordering of single columns.
// The n columns form a line; steps alternate between pairing positions (2k, 2k+1) and
// (2k+1, 2k+2), every rotation is followed by a (logical) swap, and n consecutive steps visit
// every column pair exactly once.  An 8-lane slot keeps its two columns X, Y in VGPRs for the
// whole solve; the rotation itself touches no LDS.  Between steps each slot hands ONE column to a
// neighbour through an LDS mailbox (even->odd: Y goes to slot k-1, odd->even: X goes to slot k+1).
//
// The kernel is bound by the per-step dependent chain (LDS hand-over -> dot -> 8-lane reduction
// -> rotation parameters -> update -> hand-over), not by bandwidth.  NMAT matrices share a workgroup and its
// barriers; every instantiation has NMAT = 1 since the two-matrix form was retired (the quad-block kernel took its
// shapes).  The parameter and its loops stay: without them the compiler schedules all six instantiations differently.
typedef float v4f __attribute__((ext_vector_type(4)));
// Quadratic-convergence stop: a sweep in which every rotation was SMALL -- |cos| of the pair below QUAD and
// rotation tangent below QUAD_TAN -- is the last one: small-angle rotations at small cosines disturb the other
// pairs of their columns by (sine x cosine) <= 5e-6 each, the residual cosines stay at the tolerance and the next
// sweep would only verify that.  The tangent bound matters: inside a cluster of nearly equal singular values a
// tiny cosine still calls for a 45-degree rotation, and stopping on the cosine alone leaves 1e-4 residuals there
// (measured; scripts/time_jacobi.py has that stress case).  Saves 1-2 of ~9 sweeps at n = 192 on graded spectra
// with identical final orthogonality and singular values.
#define BASD_JACOBI_QUAD 5.0e-4f
#define BASD_JACOBI_QUAD_TAN 1.0e-2f

// x' = x - s (y + tau x),  y' = y + s (x - tau y)  on four rows of a column pair, IN PLACE.  Written as C++ inside the
// `if (rotate)` of the kernels below, the compiler computes the new columns into fresh registers and moves all of them
// back at the merge point (52 v_mov per rotation of 2 x 24 values: a quarter of a rotation's VALU issue cycles, and
// these kernels are VALU-issue-bound); with the outputs tied to the inputs there is nothing to move.  One register
// pair {tau, s} feeds every FMA: op_sel broadcasts one half, neg_lo / neg_hi negate it.
typedef float v2f_rot __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void rotate_in_place(v4f& xa, v4f& ya, float tau, float s) {
  const v2f_rot ts = {tau, s};
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    v2f_rot x = h ? (v2f_rot){xa.z, xa.w} : (v2f_rot){xa.x, xa.y};
    v2f_rot y = h ? (v2f_rot){ya.z, ya.w} : (v2f_rot){ya.x, ya.y};
    v2f_rot t1, t2;
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,1,1]" : "=v"(t1) : "v"(ts), "v"(x), "v"(y));                  // y + tau x
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,1,1] neg_lo:[1,0,0] neg_hi:[1,0,0]"
        : "=v"(t2) : "v"(ts), "v"(y), "v"(x));                                                                   // x - tau y
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,1,1] neg_lo:[1,0,0] neg_hi:[1,0,0]"
        : "+v"(x) : "v"(ts), "v"(t1));                                                                           // x - s t1
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,1,1]" : "+v"(y) : "v"(ts), "v"(t2));          // y + s t2
    if (h) { xa.z = x.x; xa.w = x.y; ya.z = y.x; ya.w = y.y; }
    else { xa.x = x.x; xa.y = x.y; ya.x = y.x; ya.y = y.y; }
  }
}

// NBUF = 2 double-buffers the mailbox (one barrier per step); NBUF = 1 halves its LDS footprint for a second
// barrier per step: what lets columns of up to 384 rows (MAXCH = 12: the block pairs of the D_s = 384 eigensolver,
// 96 slots x 1.5 KiB = 147 KiB) stay register-resident.
// LDS behind the mailbox: s_sig [260], s_rank [260], s_id and s_nrm [2][2][132] each, s_flag [8]
constexpr size_t JACOBI_OE_SCRATCH = (260 + 260 + 2 * 2 * 132 * 2 + 8) * 4;
template <int MAXCH, int NMAT, int NBUF>
__global__ __launch_bounds__((NMAT == 2 || MAXCH > 7) ? 768 : 1024)
__attribute__((amdgpu_waves_per_eu((NMAT == 2 || MAXCH > 7) ? 3 : 4, (NMAT == 2 || MAXCH > 7) ? 3 : 4))) void jacobi_oe_kernel(
    float* __restrict__ wg, int batch, int m, int n, int ld, int norm_rows, float tol, int max_sweeps, int sort,
    float* __restrict__ sigma, int32_t* __restrict__ sweeps_out, const int32_t* __restrict__ active,
    int active_rows, int32_t* __restrict__ status) {
  extern __shared__ __align__(16) float lds[];
  static_assert(NMAT == 1 || NBUF == 1, "two matrices per workgroup use one mailbox each");
  constexpr int LDM = 32 * MAXCH;                  // mailbox column stride (all MAXCH chunks, no row guards)
  const int tid = threadIdx.x;
  const int k = tid >> 3, sub = tid & 7, roff = sub * 4;
  const int S_all = (n + 1) >> 1;                 // slots that own real columns
  float* mbox = lds;                               // [NMAT][NBUF][S_all][LDM]
  float* s_sig = mbox + (size_t)NMAT * NBUF * S_all * LDM;   // [n + 1]
  int* s_rank = reinterpret_cast<int*>(s_sig + 260);          // [n + 1]
  int* s_id = s_rank + 260;                        // [NMAT][NBUF][132] column ids travelling with the mailbox
  float* s_nrm = reinterpret_cast<float*>(s_id + 2 * 2 * 132);   // [NMAT][NBUF][132] squared norms travelling along
  int* s_flag = reinterpret_cast<int*>(s_nrm + 2 * 2 * 132);     // [2] any rotation, [2] any LARGE rotation

  if (NMAT == 1 && active != nullptr && active[blockIdx.x] < 0) {
    // skipped matrix (a block pair of a tournament whose matrix has already converged): nothing is read or written
    if (sweeps_out && threadIdx.x == 0) sweeps_out[blockIdx.x] = 0;
    return;
  }
  float* src[NMAT];
  int n_act[NMAT], mrows[NMAT], n_e[NMAT], S[NMAT], idX[NMAT], idY[NMAT];
  bool live[NMAT];
  v4f X[NMAT][MAXCH], Y[NMAT][MAXCH];
  float nX[NMAT], nY[NMAT];                        // squared column norms, updated by a' = a - t g, b' = b + t g
  int n_loop = 2;
#pragma unroll
  for (int mi = 0; mi < NMAT; ++mi) {
    const int mat = blockIdx.x * NMAT + mi;
    const bool exists = mat < batch;
    src[mi] = wg + (size_t)(exists ? mat : 0) * n * ld;
    int na = n;
    if (active && exists) { na = active[mat]; na = na < 2 ? 2 : (na > n ? n : na); }
    n_act[mi] = na;
    int mr = (m + 3) & ~3;
    if (active && active_rows) { const int ma = (na + 3) & ~3; mr = ma < mr ? ma : mr; }
    mrows[mi] = mr;
    n_e[mi] = na + (na & 1);                       // line length (a zero phantom column pads odd n)
    S[mi] = n_e[mi] >> 1;
    live[mi] = exists && (k < S[mi]);
    if (exists && n_e[mi] > n_loop) n_loop = n_e[mi];
    idX[mi] = 2 * k; idY[mi] = 2 * k + 1;
#pragma unroll
    for (int ch = 0; ch < MAXCH; ++ch) {
      const int r = roff + 32 * ch;
      const bool in = live[mi] && r < mr;
      X[mi][ch] = (in && idX[mi] < na) ? *reinterpret_cast<const v4f*>(src[mi] + (size_t)idX[mi] * ld + r) : (v4f){0.f, 0.f, 0.f, 0.f};
      Y[mi][ch] = (in && idY[mi] < na) ? *reinterpret_cast<const v4f*>(src[mi] + (size_t)idY[mi] * ld + r) : (v4f){0.f, 0.f, 0.f, 0.f};
    }
  }
  if (tid < 8) s_flag[tid] = 0;                    // [4 + 2 mi + parity]: largest squared column norm of the sweep
  __syncthreads();

  // rotation test |gamma| > tol sqrt(alpha beta) as (gamma / tol)^2 > alpha beta: with the tolerance on the right-hand
  // side (tol^2 alpha beta ~ 7e-13 alpha beta) the product underflows for the graded factors of rank-deficient Gram
  // matrices (a column of norm 1e-17 next to one of norm 1: the debris of cancelled directions) and the test
  // degenerates to gamma^2 > 0 -- such pairs then rotate, and count as LARGE rotations, on noise, sweep after sweep
  // (seen at BASELINE c5: a principal-angle problem of the 768-wide selector used all 40 sweeps once in ~30 steps)
  const float inv_tol = 1.0f / tol;
  int used_sweeps = 0;
  bool converged = false;
  int step = 0;                                    // global step counter: even = (2k, 2k+1) view
#pragma unroll 1
  for (int sweep = 0; sweep < max_sweeps; ++sweep) {
    bool rotated = false, bigrot = false;
    // exact squared norms once per sweep; inside the sweep they follow the rotation identities
    // (drift ~ n eps only perturbs the rotation angle and the skip test, never the columns)
#pragma unroll
    for (int mi = 0; mi < NMAT; ++mi) {
      float ax = 0.f, ay = 0.f;
#pragma unroll
      for (int ch = 0; ch < MAXCH; ++ch) {
        const v4f x = X[mi][ch], y = Y[mi][ch];
        ax = fmaf(x.x, x.x, fmaf(x.y, x.y, fmaf(x.z, x.z, fmaf(x.w, x.w, ax))));
        ay = fmaf(y.x, y.x, fmaf(y.y, y.y, fmaf(y.z, y.z, fmaf(y.w, y.w, ay))));
      }
      nX[mi] = group8_sum(ax);
      nY[mi] = group8_sum(ay);
      if (live[mi] && sub == 0) atomicMax(&s_flag[4 + 2 * mi + (sweep & 1)], __float_as_int(fmaxf(nX[mi], nY[mi])));
    }
    __syncthreads();
#pragma unroll
    for (int mi = 0; mi < NMAT; ++mi) {            // debris columns become exact zero columns (gamma = 0: never rotated)
      const float debris = __int_as_float(s_flag[4 + 2 * mi + (sweep & 1)]) * BASD_JACOBI_DEBRIS;
      const bool zx = nX[mi] < debris, zy = nY[mi] < debris;
#pragma unroll
      for (int ch = 0; ch < MAXCH; ++ch) {
        if (zx) X[mi][ch] = (v4f){0.f, 0.f, 0.f, 0.f};
        if (zy) Y[mi][ch] = (v4f){0.f, 0.f, 0.f, 0.f};
      }
      if (zx) nX[mi] = 0.f;
      if (zy) nY[mi] = 0.f;
    }
#pragma unroll 1
    for (int t = 0; t < n_loop; ++t, ++step) {
      const bool even_view = (step & 1) == 0;
      const int buf = (NBUF == 2) ? (step & 1) : 0;
#pragma unroll
      for (int mi = 0; mi < NMAT; ++mi) {
        // in the odd view the last slot owns a single column (X) and slot 0's old first column idles
        const bool pair_ok = live[mi] && (even_view || k < S[mi] - 1);
        if (pair_ok) {
          const float alpha = nX[mi], beta = nY[mi];
          float gamma = 0.f;
#pragma unroll
          for (int ch = 0; ch < MAXCH; ++ch) {
            const v4f x = X[mi][ch], y = Y[mi][ch];
            gamma = fmaf(x.x, y.x, fmaf(x.y, y.y, fmaf(x.z, y.z, fmaf(x.w, y.w, gamma))));
          }
          gamma = group8_sum(gamma);
          const float gsc = gamma * inv_tol;
          if (gsc * gsc > fmaxf(alpha * beta, BASD_JACOBI_TINY)) {
            rotated = true;
            const float gq = gamma * (1.0f / BASD_JACOBI_QUAD);
            const bool big_cos = gq * gq > alpha * beta;
            const float zeta = (beta - alpha) * __builtin_amdgcn_rcpf(2.f * gamma);
            const float tt = copysignf(1.f, zeta) * __builtin_amdgcn_rcpf(fabsf(zeta) + __builtin_amdgcn_sqrtf(fmaf(zeta, zeta, 1.f)));
            bigrot = bigrot || big_cos || fabsf(tt) > BASD_JACOBI_QUAD_TAN;
            const float w1 = fmaf(tt, tt, 1.f);
            float c = __builtin_amdgcn_rsqf(w1);
            c = c * fmaf(-0.5f * w1, c * c, 1.5f);
            const float s = c * tt;
            const float tau = s * __builtin_amdgcn_rcpf(1.0f + c);
            nX[mi] = fmaf(-tt, gamma, alpha);
            nY[mi] = fmaf(tt, gamma, beta);
#pragma unroll
            for (int ch = 0; ch < MAXCH; ++ch) rotate_in_place(X[mi][ch], Y[mi][ch], tau, s);
          }
        }
      }
      // ---- hand one column over.  After the (logical) swap the pair is stored as (lo = Y, hi = X).
      // even -> odd view: position 2k (held in Y) goes to slot k-1; slot 0's copy stays parked in
      //   box[0] until the next odd -> even hand-over; the new Y is slot k+1's old position 2k+2.
      // odd -> even view: position 2k+2 (held in X after the swap; the lone last slot did not swap)
      //   goes to slot k+1; the new X is slot k-1's old position 2k (slot 0: the parked column).
#pragma unroll
      for (int mi = 0; mi < NMAT; ++mi) {
        float* box = mbox + ((size_t)mi * NBUF + buf) * S_all * LDM;
        int* idbox = s_id + (mi * 2 + buf) * 132;
        float* nbox = s_nrm + (mi * 2 + buf) * 132;
        if (even_view) {
          if (live[mi]) {
#pragma unroll
            for (int ch = 0; ch < MAXCH; ++ch) *reinterpret_cast<v4f*>(box + (size_t)k * LDM + roff + 32 * ch) = Y[mi][ch];
            if (sub == 0) { idbox[k] = idY[mi]; nbox[k] = nY[mi]; }
          }
        } else if (live[mi] && k < S[mi] - 1) {
#pragma unroll
          for (int ch = 0; ch < MAXCH; ++ch) *reinterpret_cast<v4f*>(box + (size_t)(k + 1) * LDM + roff + 32 * ch) = X[mi][ch];
          if (sub == 0) { idbox[k + 1] = idX[mi]; nbox[k + 1] = nX[mi]; }
        }
      }
      __syncthreads();
#pragma unroll
      for (int mi = 0; mi < NMAT; ++mi) {
        const float* box = mbox + ((size_t)mi * NBUF + buf) * S_all * LDM;
        const int* idbox = s_id + (mi * 2 + buf) * 132;
        const float* nbox = s_nrm + (mi * 2 + buf) * 132;
        if (even_view) {
          if (live[mi] && k < S[mi] - 1) {
#pragma unroll
            for (int ch = 0; ch < MAXCH; ++ch) Y[mi][ch] = *reinterpret_cast<const v4f*>(box + (size_t)(k + 1) * LDM + roff + 32 * ch);
            idY[mi] = idbox[k + 1];
            nY[mi] = nbox[k + 1];
          }
        } else if (live[mi]) {
          const int pbuf = (NBUF == 2) ? (buf ^ 1) : 0;             // where slot 0 parked its column
          const float* rbox = (k == 0) ? mbox + ((size_t)mi * NBUF + pbuf) * S_all * LDM : box + (size_t)k * LDM;
          const int* ridbox = (k == 0) ? s_id + (mi * 2 + pbuf) * 132 : idbox + k;
          const float* rnbox = (k == 0) ? s_nrm + (mi * 2 + pbuf) * 132 : nbox + k;
          const bool lone = (k == S[mi] - 1);    // its single column stayed at position 2k+1 -> becomes Y
#pragma unroll
          for (int ch = 0; ch < MAXCH; ++ch) {
            if (lone) Y[mi][ch] = X[mi][ch];
            X[mi][ch] = *reinterpret_cast<const v4f*>(rbox + roff + 32 * ch);
          }
          if (lone) { idY[mi] = idX[mi]; nY[mi] = nX[mi]; }
          idX[mi] = ridbox[0];
          nX[mi] = rnbox[0];
        }
      }
      if (NBUF == 1) __syncthreads();            // single mailbox: reads done before the next writes
    }
    used_sweeps = sweep + 1;
    if (rotated) s_flag[sweep & 1] = 1;
    if (bigrot) s_flag[2 + (sweep & 1)] = 1;
    __syncthreads();
    const int any = s_flag[sweep & 1], anybig = s_flag[2 + (sweep & 1)];
    if (tid == 0) {
      s_flag[(sweep + 1) & 1] = 0; s_flag[2 + ((sweep + 1) & 1)] = 0;
      s_flag[4 + ((sweep + 1) & 1)] = 0; s_flag[6 + ((sweep + 1) & 1)] = 0;
    }
    __syncthreads();
    if (!any || !anybig) { converged = true; break; }
  }
  // n_loop is even, so the solve ends in the even view: slot k holds positions 2k (X) and 2k+1 (Y)

#pragma unroll
  for (int mi = 0; mi < NMAT; ++mi) {
    const int mat = blockIdx.x * NMAT + mi;
    if (mat >= batch) break;                     // uniform across the workgroup
    // ---- norms over the first norm_rows rows; the phantom column (id == n_act, only when n_act is
    //      odd) gets -1 so that it ranks last and is dropped
    __syncthreads();
    for (int c = tid; c <= n; c += blockDim.x) s_sig[c] = 0.f;
    __syncthreads();
    if (live[mi]) {
      float ax = 0.f, ay = 0.f;
#pragma unroll
      for (int ch = 0; ch < MAXCH; ++ch) {
        const int r = roff + 32 * ch;
        const float mx = (r + 0 < norm_rows) ? 1.f : 0.f, my = (r + 1 < norm_rows) ? 1.f : 0.f;
        const float mz = (r + 2 < norm_rows) ? 1.f : 0.f, mw = (r + 3 < norm_rows) ? 1.f : 0.f;
        const v4f x = X[mi][ch], y = Y[mi][ch];
        ax = fmaf(mx * x.x, x.x, fmaf(my * x.y, x.y, fmaf(mz * x.z, x.z, fmaf(mw * x.w, x.w, ax))));
        ay = fmaf(mx * y.x, y.x, fmaf(my * y.y, y.y, fmaf(mz * y.z, y.z, fmaf(mw * y.w, y.w, ay))));
      }
      ax = group8_sum(ax);
      ay = group8_sum(ay);
      if (sub == 0) {
        s_sig[2 * k] = (idX[mi] >= n_act[mi]) ? -1.f : sqrtf(ax);
        s_sig[2 * k + 1] = (idY[mi] >= n_act[mi]) ? -1.f : sqrtf(ay);
      }
    }
    __syncthreads();
    // positions 0 .. n_e-1 hold the active columns (one may be the phantom), n_e .. n-1 are the
    // untouched zero columns of an `active` call; rank all of them (descending, ties by position)
    const int n_tot = (n_e[mi] > n) ? n_e[mi] : n;
    if (tid < n_tot) {
      int rank = tid;
      if (sort) {
        const float mine = s_sig[tid];
        rank = 0;
        for (int c = 0; c < n_tot; ++c) {
          const float o = s_sig[c];
          rank += (o > mine) || (o == mine && c < tid);
        }
      }
      s_rank[tid] = rank;
    }
    __syncthreads();
    {
      // every slot (live or not) writes the two positions it stands for
      const int p0 = 2 * k, p1 = 2 * k + 1;
      int d0 = (p0 < n_tot) ? s_rank[p0] : n, d1 = (p1 < n_tot) ? s_rank[p1] : n;
      if (!sort) { d0 = live[mi] ? idX[mi] : p0; d1 = live[mi] ? idY[mi] : p1; }
      const float sg0 = (p0 < n_tot) ? s_sig[p0] : -1.f, sg1 = (p1 < n_tot) ? s_sig[p1] : -1.f;
      if (k < ((n_tot + 1) >> 1)) {
#pragma unroll
        for (int ch = 0; ch < MAXCH; ++ch) {
          const int r = roff + 32 * ch;
          if (r < ld) {
            const v4f z4 = (v4f){0.f, 0.f, 0.f, 0.f};
            const bool inr = r < mrows[mi];
            if (d0 >= 0 && d0 < n && p0 < n_tot) *reinterpret_cast<v4f*>(src[mi] + (size_t)d0 * ld + r) = (live[mi] && inr) ? X[mi][ch] : z4;
            if (d1 >= 0 && d1 < n && p1 < n_tot) *reinterpret_cast<v4f*>(src[mi] + (size_t)d1 * ld + r) = (live[mi] && inr) ? Y[mi][ch] : z4;
          }
        }
        if (sub == 0) {
          if (d0 >= 0 && d0 < n && p0 < n_tot) sigma[(size_t)mat * n + d0] = sg0 < 0.f ? 0.f : sg0;
          if (d1 >= 0 && d1 < n && p1 < n_tot) sigma[(size_t)mat * n + d1] = sg1 < 0.f ? 0.f : sg1;
        }
      }
    }
    if (sweeps_out && tid == 0) sweeps_out[mat] = converged ? used_sweeps : -used_sweeps;
    __syncthreads();
    report_status(status, converged, s_sig, n_tot, tid, blockDim.x, NMAT == 2 ? 4 : (NBUF == 2 ? 2 : 3), mat);
  }
}

// ---------------------------------------------------------------------------------------------
// Block orderings with scaled rotations: jacobi_block_kernel, further down, with BlockOrder<4> or BlockOrder<6>.
// Quad-block ordering (the default for 8 .. 196 columns where the hex-block ordering below does not apply).  What its retired predecessor (block odd-even: 8-lane slots owning two blocks of TWO columns, DESIGN.md
// section 5) still paid per rotation and wave: the rotation parameters (five
// transcendentals, ~25 VALU instructions) are computed by all 8 lanes of a slot, i.e. 8 distinct
// parameter sets per wave instruction stream; the plane rotation is four FMAs per row pair; and the
// mailbox costs two barriers per hand-over.  Here
//   * a slot is 16 lanes (12 rows per lane at 192 rows) and owns two blocks of FOUR columns (the same 96
//     column VGPRs); a meeting of two blocks is 16 cross rotations in four rounds of four INDEPENDENT
//     rotations, one hand-over per 16 rotations (two-column blocks: per 4);
//   * the four dot products of a round are reduced with a reduce-scatter (11 DPP / select instructions for
//     all four), after which lane q of every quad holds rotation q's sum and computes rotation q's
//     parameters: ONE parameter instruction stream serves four rotations per slot, 16 per wave;
//   * the per-column bookkeeping (squared norm, scale, id) is DISTRIBUTED: lane q of a quad owns column q of
//     either block; a round fetches / returns the partner column's entry with one quad_perm each;
//   * rotations are applied as two shears on scaled columns (x = dx x~, y = dy y~):
//         x~' = x~ - a y~,  y~' = y~ + b x~',   a = t dy / dx,  b = s c dx / dy,  dx' = c dx,  dy' = dy / c
//     -- exactly the rotation x' = c x - s y, y' = s x + c y, two FMAs per row pair instead of four, in place.
//     The scales follow dx' = dx - dx h, dy' = dy + dy h / c with h = 1 - c = s^2 / (1 + c) computed without
//     cancellation: a c that rounds to 1 (t^2 < eps) must not inflate the norms (the bias the Rutishauser form
//     removed from the unscaled kernels); the scales are folded back into the columns once per sweep, where the
//     exact norms are recomputed anyway, so a scale is the product of at most ~190 factors in [0.70, 1.42].
//   * ONE barrier per hand-over: box j is written by slot j (even steps) or slot j - 1 (odd steps) and read by
//     the other one after the barrier; the next write to it comes from the slot that just read it (same lanes,
//     same addresses, LDS operations of a wave execute in order), so no second barrier is needed.
template <int CTRL> __device__ __forceinline__ float dppf(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
template <int CTRL> __device__ __forceinline__ int dppi(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true);
}
__host__ __device__ constexpr int qperm(int a, int b, int c, int d) { return a | (b << 2) | (c << 4) | (d << 6); }

// lane (l & 3) = q of every quad receives the sum over the LANES (16: one DPP row, 32: two) lanes of its slot of p_q
template <int LANES>
__device__ __forceinline__ float reduce_scatter4(float p0, float p1, float p2, float p3, bool bit0, bool bit1) {
  const float keepA = bit0 ? p1 : p0, giveA = bit0 ? p0 : p1;
  const float keepB = bit0 ? p3 : p2, giveB = bit0 ? p2 : p3;
  const float uA = keepA + dppf<qperm(1, 0, 3, 2)>(giveA);
  const float uB = keepB + dppf<qperm(1, 0, 3, 2)>(giveB);
  const float keep = bit1 ? uB : uA, give = bit1 ? uA : uB;
  float v = keep + dppf<qperm(2, 3, 0, 1)>(give);
  // across the four quads: row_ror:8 FIRST, then row_ror:4.  In this order every step adds the same two operands in
  // all lanes that end up with the same sum (l and l + 8, then l and l + 4), so the four quads hold BITWISE identical
  // copies.  (ror:4 then ror:8 pairs the partial sums differently in quads {0, 2} and {1, 3}: replicas that differ in
  // the last bit -- and inside a cluster of equal singular values the sign of beta - alpha, i.e. the direction of a
  // 45-degree rotation, then differs between the rows of one column.)
  v += dppf<0x128>(v);                              // row_ror:8
  v += dppf<0x124>(v);                              // row_ror:4
  if constexpr (LANES == 32) {
    // the slot's two DPP rows: v_permlane16_swap with the same register as both operands leaves (row 0's value, row
    // 1's value) in every lane of the row pair -- the same two operands in the same order in both rows
    typedef unsigned int pl_u32x2 __attribute__((ext_vector_type(2)));
    const pl_u32x2 sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
  }
  return v;
}

// the two shears of a scaled rotation on four rows, in place: ab = {a, b}
__device__ __forceinline__ void shear_in_place(v4f& xa, v4f& ya, v2f_rot ab) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    v2f_rot x = h ? (v2f_rot){xa.z, xa.w} : (v2f_rot){xa.x, xa.y};
    v2f_rot y = h ? (v2f_rot){ya.z, ya.w} : (v2f_rot){ya.x, ya.y};
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[0,1,1] neg_lo:[1,0,0] neg_hi:[1,0,0]" : "+v"(x) : "v"(ab), "v"(y));   // x - a y
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,1,1]" : "+v"(y) : "v"(ab), "v"(x));                // y + b x'
    if (h) { xa.z = x.x; xa.w = x.y; ya.z = y.x; ya.w = y.y; }
    else { xa.x = x.x; xa.y = x.y; ya.x = y.x; ya.y = y.y; }
  }
}

// partial dot products (over this lane's rows) of the four column pairs of a round, on the packed FMA, the four
// accumulation chains interleaved.  Written as asm: left to itself the SLP vectoriser packs the four dot products
// ACROSS columns and pays four v_mov per v_pk_fma.
#define BASD_LO2(v) __builtin_shufflevector(v, v, 0, 1)
#define BASD_HI2(v) __builtin_shufflevector(v, v, 2, 3)
template <int MAXCH>
__device__ __forceinline__ void dot4_cols(const v4f (&A0)[MAXCH], const v4f (&B0)[MAXCH], const v4f (&A1)[MAXCH],
                                          const v4f (&B1)[MAXCH], const v4f (&A2)[MAXCH], const v4f (&B2)[MAXCH],
                                          const v4f (&A3)[MAXCH], const v4f (&B3)[MAXCH], float (&p)[4]) {
  v2f_rot a0, a1, a2, a3;
  asm("v_pk_mul_f32 %0, %1, %2" : "=v"(a0) : "v"(BASD_LO2(A0[0])), "v"(BASD_LO2(B0[0])));
  asm("v_pk_mul_f32 %0, %1, %2" : "=v"(a1) : "v"(BASD_LO2(A1[0])), "v"(BASD_LO2(B1[0])));
  asm("v_pk_mul_f32 %0, %1, %2" : "=v"(a2) : "v"(BASD_LO2(A2[0])), "v"(BASD_LO2(B2[0])));
  asm("v_pk_mul_f32 %0, %1, %2" : "=v"(a3) : "v"(BASD_LO2(A3[0])), "v"(BASD_LO2(B3[0])));
  asm("v_pk_fma_f32 %0, %1, %2, %0" : "+v"(a0) : "v"(BASD_HI2(A0[0])), "v"(BASD_HI2(B0[0])));
  asm("v_pk_fma_f32 %0, %1, %2, %0" : "+v"(a1) : "v"(BASD_HI2(A1[0])), "v"(BASD_HI2(B1[0])));
  asm("v_pk_fma_f32 %0, %1, %2, %0" : "+v"(a2) : "v"(BASD_HI2(A2[0])), "v"(BASD_HI2(B2[0])));
  asm("v_pk_fma_f32 %0, %1, %2, %0" : "+v"(a3) : "v"(BASD_HI2(A3[0])), "v"(BASD_HI2(B3[0])));
#pragma unroll
  for (int ch = 1; ch < MAXCH; ++ch) {
    asm("v_pk_fma_f32 %0, %1, %2, %0" : "+v"(a0) : "v"(BASD_LO2(A0[ch])), "v"(BASD_LO2(B0[ch])));
    asm("v_pk_fma_f32 %0, %1, %2, %0" : "+v"(a1) : "v"(BASD_LO2(A1[ch])), "v"(BASD_LO2(B1[ch])));
    asm("v_pk_fma_f32 %0, %1, %2, %0" : "+v"(a2) : "v"(BASD_LO2(A2[ch])), "v"(BASD_LO2(B2[ch])));
    asm("v_pk_fma_f32 %0, %1, %2, %0" : "+v"(a3) : "v"(BASD_LO2(A3[ch])), "v"(BASD_LO2(B3[ch])));
    asm("v_pk_fma_f32 %0, %1, %2, %0" : "+v"(a0) : "v"(BASD_HI2(A0[ch])), "v"(BASD_HI2(B0[ch])));
    asm("v_pk_fma_f32 %0, %1, %2, %0" : "+v"(a1) : "v"(BASD_HI2(A1[ch])), "v"(BASD_HI2(B1[ch])));
    asm("v_pk_fma_f32 %0, %1, %2, %0" : "+v"(a2) : "v"(BASD_HI2(A2[ch])), "v"(BASD_HI2(B2[ch])));
    asm("v_pk_fma_f32 %0, %1, %2, %0" : "+v"(a3) : "v"(BASD_HI2(A3[ch])), "v"(BASD_HI2(B3[ch])));
  }
  p[0] = a0.x + a0.y; p[1] = a1.x + a1.y; p[2] = a2.x + a2.y; p[3] = a3.x + a3.y;
}

// One round = four independent rotations (X_i, Y_i), i = 0..3, column indices 0..7 (0-3 block P, 4-7 block Q)
// covering all eight columns of the slot.  Lane q of a quad computes rotation q.
template <int X0, int Y0, int X1, int Y1, int X2, int Y2, int X3, int Y3>
struct RoundMap {
  __host__ __device__ static constexpr int X(int i) { return i == 0 ? X0 : (i == 1 ? X1 : (i == 2 ? X2 : X3)); }
  __host__ __device__ static constexpr int Y(int i) { return i == 0 ? Y0 : (i == 1 ? Y1 : (i == 2 ? Y2 : Y3)); }
  // gather: lane q takes the entry of column X[q] / Y[q] from its owner lane (column & 3) of register P (column < 4) or Q
  static constexpr int gx = qperm(X0 & 3, X1 & 3, X2 & 3, X3 & 3), gy = qperm(Y0 & 3, Y1 & 3, Y2 & 3, Y3 & 3);
  static constexpr int xq_mask = (X0 >> 2) | ((X1 >> 2) << 1) | ((X2 >> 2) << 2) | ((X3 >> 2) << 3);   // bit q: X[q] in block Q
  static constexpr int yq_mask = (Y0 >> 2) | ((Y1 >> 2) << 1) | ((Y2 >> 2) << 2) | ((Y3 >> 2) << 3);
  // scatter: owner lane j of P[j] (Q[j]) takes the new entry from the rotation that held the column
  static constexpr int src_of(int col) {
    for (int i = 0; i < 4; ++i) if (X(i) == col || Y(i) == col) return i;
    return 0;
  }
  static constexpr bool from_y(int col) {
    for (int i = 0; i < 4; ++i) if (Y(i) == col) return true;
    return false;
  }
  static constexpr int sp = qperm(src_of(0), src_of(1), src_of(2), src_of(3));
  static constexpr int sq = qperm(src_of(4), src_of(5), src_of(6), src_of(7));
  static constexpr int py_mask = (from_y(0) ? 1 : 0) | (from_y(1) ? 2 : 0) | (from_y(2) ? 4 : 0) | (from_y(3) ? 8 : 0);
  static constexpr int qy_mask = (from_y(4) ? 1 : 0) | (from_y(5) ? 2 : 0) | (from_y(6) ? 4 : 0) | (from_y(7) ? 8 : 0);
};
template <int CTRL> __device__ __forceinline__ float qgather(float v) {
  if constexpr (CTRL == qperm(0, 1, 2, 3)) return v;
  else return dppf<CTRL>(v);
}
template <int GCTRL, int QMASK> __device__ __forceinline__ float meta_gather(float mp, float mq, int q) {
  if constexpr (QMASK == 0) return qgather<GCTRL>(mp);
  else if constexpr (QMASK == 15) return qgather<GCTRL>(mq);
  else {
    const float a = qgather<GCTRL>(mp), b = qgather<GCTRL>(mq);
    return ((QMASK >> q) & 1) ? b : a;
  }
}
template <int SCTRL, int YMASK> __device__ __forceinline__ float meta_scatter(float xn, float yn, int q) {
  if constexpr (YMASK == 0) return qgather<SCTRL>(xn);
  else if constexpr (YMASK == 15) return qgather<SCTRL>(yn);
  else {
    const float a = qgather<SCTRL>(xn), b = qgather<SCTRL>(yn);
    return ((YMASK >> q) & 1) ? b : a;
  }
}

// ceil(x / D) for x >= 0: a shift where D is a power of two (the signed division costs three instructions more)
template <int D> __host__ __device__ constexpr int ceil_div(int x) {
  return (D & (D - 1)) == 0 ? (x + D - 1) >> __builtin_ctz(D) : (x + D - 1) / D;
}
// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): a loop whose index is a template argument
template <int N, int I = 0, class F> __device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) { f(std::integral_constant<int, I>{}); static_for<N, I + 1>(f); }
}

// What jacobi_block_kernel (below) needs to know about an ordering with blocks of BC columns: how a round's BC partial
// dot products are formed and reduced, how (norm, scale) entries and rotation parameters travel between lanes, which
// lanes hold them, and the round schedule.  Everything here is resolved at compile time.
template <int BC> struct BlockOrder;

// Quad-block: lane q of every quad computes rotation q and owns column q of either block; entries move with quad
// permutes (DPP), so every quad of the slot carries a full replica of the bookkeeping.
template <> struct BlockOrder<4> {
  struct Lane {
    int q;                                         // lane within its quad
    bool bit0, bit1;
    static constexpr bool rlane = true;            // every lane computes a rotation
  };
  __device__ __forceinline__ static Lane lane(int /*tid*/, int sub) { return {sub & 3, (sub & 1) != 0, (sub & 2) != 0}; }
  // the lanes that speak for the slot's column entries (largest norm of the sweep): one replica is enough
  __device__ __forceinline__ static bool owner(const Lane&, int sub) { return sub < 4; }
  __device__ __forceinline__ static int meta_col(const Lane& L) { return L.q; }   // mailbox entry this lane reads
  // LANES = 16: rows 4 sub + 64 ch; 32: rows 4 sub + 128 ch (columns of up to 384 rows at the same 96 column VGPRs,
  // 768 threads -- the block pairs of the D_s = 384 eigensolver).  MAXCH = 4 at 16 lanes (193 .. 256 rows: the
  // 196 x 196 token-side Procrustes cores of the wide students) holds 128 column VGPRs: two waves per SIMD.
  static constexpr int max_threads(int maxch, int lanes) { return lanes == 32 ? 768 : (maxch > 3 ? 448 : 384); }
  static constexpr int status_kind = 6;           // the kernel variant in the health word (report_status)
  // quad permutes have no latency to hide: a round fetches the entries of its columns where it uses them (after the
  // dot products) and hands the new ones back before it broadcasts the rotation parameters
  static constexpr bool entries_first = false;

  template <class M, int MAXCH> __device__ __forceinline__ static void dots(const v4f (&C)[8][MAXCH], float (&p)[4]) {
    dot4_cols<MAXCH>(C[M::X(0)], C[M::Y(0)], C[M::X(1)], C[M::Y(1)], C[M::X(2)], C[M::Y(2)], C[M::X(3)], C[M::Y(3)], p);
  }
  template <int LANES> __device__ __forceinline__ static float reduce_scatter(const float (&p)[4], const Lane& L) {
    return reduce_scatter4<LANES>(p[0], p[1], p[2], p[3], L.bit0, L.bit1);
  }
  // entry (held as mp for block P, mq for block Q) of the column this lane's rotation takes as X / as Y
  template <class M> __device__ __forceinline__ static float gather_x(float mp, float mq, const Lane& L) {
    return meta_gather<M::gx, M::xq_mask>(mp, mq, L.q);
  }
  template <class M> __device__ __forceinline__ static float gather_y(float mp, float mq, const Lane& L) {
    return meta_gather<M::gy, M::yq_mask>(mp, mq, L.q);
  }
  // new entry of the column of block P / Q this lane owns, from the rotation that held it (as its X: xn, as its Y: yn)
  template <class M> __device__ __forceinline__ static float scatter_p(float xn, float yn, const Lane& L) {
    return meta_scatter<M::sp, M::py_mask>(xn, yn, L.q);
  }
  template <class M> __device__ __forceinline__ static float scatter_q(float xn, float yn, const Lane& L) {
    return meta_scatter<M::sq, M::qy_mask>(xn, yn, L.q);
  }
  // v of the lane that computes rotation I / owns column I
  template <int I> __device__ __forceinline__ static float bcast(float v) { return dppf<qperm(I, I, I, I)>(v); }
  // the six pairs inside each block, once per sweep: three rounds of two pairs per block
  template <class F> __device__ __forceinline__ static void inner_rounds(F&& round, bool ok) {
    round(RoundMap<0, 1, 2, 3, 4, 5, 6, 7>{}, ok);
    round(RoundMap<0, 2, 1, 3, 4, 6, 5, 7>{}, ok);
    round(RoundMap<0, 3, 1, 2, 4, 7, 5, 6>{}, ok);
  }
  // a meeting of blocks P and Q: 16 cross rotations in four rounds
  template <class F> __device__ __forceinline__ static void cross_rounds(F&& round, bool ok) {
    round(RoundMap<0, 4, 1, 5, 2, 6, 3, 7>{}, ok);
    round(RoundMap<0, 5, 1, 6, 2, 7, 3, 4>{}, ok);
    round(RoundMap<0, 6, 1, 7, 2, 4, 3, 5>{}, ok);
    round(RoundMap<0, 7, 1, 4, 2, 5, 3, 6>{}, ok);
  }
};

// ---------------------------------------------------------------------------------------------
// Hex-block ordering: blocks of SIX columns, 16 slots of 16 lanes for 192 columns -- FOUR
// waves, one per SIMD.  What the quad-block kernel leaves on the table: its 24 slots are six waves on four SIMDs
// (two SIMDs carry two waves, two carry one: the workgroup runs at the pace of the loaded pair), and one
// parameter stream serves four rotations.  Here a meeting of two blocks is 36 cross rotations in six rounds of SIX
// independent rotations (one hand-over per 36), lane q (q = lane & 7 < 6) of each half of a slot computes rotation
// q, and a sweep is 32 steps instead of 48.  The price is 144 column VGPRs (two waves per SIMD at most) and that
// the per-column bookkeeping no longer moves with quad permutes: partner entries travel by ds_bpermute, rotation
// parameters are broadcast with ds_swizzle (lane i of every group of 8) -- 16 LDS-crossbar operations per round,
// no LDS memory.  Everything else (scaled rotations as two shears, scales folded once per sweep, one barrier per
// hand-over, analytic column ids) is shared with the quad-block ordering: jacobi_block_kernel below.
__device__ __forceinline__ float bperm(int idx4, float v) {
  return __int_as_float(__builtin_amdgcn_ds_bpermute(idx4, __float_as_int(v)));
}
template <int I> __device__ __forceinline__ float bcast8(float v) {          // lane I of this lane's group of 8
  return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), (I << 5) | 0x18));
}

// lane (l & 7) = q < 6 of the slot's 16 lanes receives the sum over the 16 lanes of p_q (lanes 6, 7: unspecified)
template <int LANES>
__device__ __forceinline__ float reduce_scatter6(const float (&p)[6], bool bit0, bool bit1, bool bit2) {
  const float k0 = bit0 ? p[1] : p[0], g0 = bit0 ? p[0] : p[1];
  const float k1 = bit0 ? p[3] : p[2], g1 = bit0 ? p[2] : p[3];
  const float k2 = bit0 ? p[5] : p[4], g2 = bit0 ? p[4] : p[5];
  const float u0 = k0 + dppf<qperm(1, 0, 3, 2)>(g0);           // index 0 + bit0
  const float u1 = k1 + dppf<qperm(1, 0, 3, 2)>(g1);           // index 2 + bit0
  const float u2 = k2 + dppf<qperm(1, 0, 3, 2)>(g2);           // index 4 + bit0
  const float ka = bit1 ? u1 : u0, ga = bit1 ? u0 : u1;
  const float kb = bit1 ? 0.f : u2, gb = bit1 ? u2 : 0.f;
  float v0 = ka + dppf<qperm(2, 3, 0, 1)>(ga);                 // index (l & 3), sum over the quad
  float v1 = kb + dppf<qperm(2, 3, 0, 1)>(gb);                 // index 4 + (l & 3) (only 4, 5 exist)
  // all four quads receive the sum over the quads of both (row_ror:8 first: bitwise identical replicas, see
  // reduce_scatter4), then each lane keeps the one its (l & 7) names
  v0 += dppf<0x128>(v0);
  v1 += dppf<0x128>(v1);
  v0 += dppf<0x124>(v0);
  v1 += dppf<0x124>(v1);
  float v = bit2 ? v1 : v0;
  if constexpr (LANES == 32) {                                  // the slot's two DPP rows (see reduce_scatter4)
    typedef unsigned int pl_u32x2 __attribute__((ext_vector_type(2)));
    const pl_u32x2 sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
  }
  return v;
}

template <int MAXCH>
__device__ __forceinline__ void dot6_cols(const v4f (&A0)[MAXCH], const v4f (&B0)[MAXCH], const v4f (&A1)[MAXCH],
                                          const v4f (&B1)[MAXCH], const v4f (&A2)[MAXCH], const v4f (&B2)[MAXCH],
                                          const v4f (&A3)[MAXCH], const v4f (&B3)[MAXCH], const v4f (&A4)[MAXCH],
                                          const v4f (&B4)[MAXCH], const v4f (&A5)[MAXCH], const v4f (&B5)[MAXCH],
                                          float (&p)[6]) {
  v2f_rot a0, a1, a2, a3, a4, a5;
#define BASD_D6_MUL(acc, A, B) asm("v_pk_mul_f32 %0, %1, %2" : "=v"(acc) : "v"(BASD_LO2(A[0])), "v"(BASD_LO2(B[0])))
#define BASD_D6_FMA(acc, a, b) asm("v_pk_fma_f32 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b))
  BASD_D6_MUL(a0, A0, B0); BASD_D6_MUL(a1, A1, B1); BASD_D6_MUL(a2, A2, B2);
  BASD_D6_MUL(a3, A3, B3); BASD_D6_MUL(a4, A4, B4); BASD_D6_MUL(a5, A5, B5);
  BASD_D6_FMA(a0, BASD_HI2(A0[0]), BASD_HI2(B0[0])); BASD_D6_FMA(a1, BASD_HI2(A1[0]), BASD_HI2(B1[0]));
  BASD_D6_FMA(a2, BASD_HI2(A2[0]), BASD_HI2(B2[0])); BASD_D6_FMA(a3, BASD_HI2(A3[0]), BASD_HI2(B3[0]));
  BASD_D6_FMA(a4, BASD_HI2(A4[0]), BASD_HI2(B4[0])); BASD_D6_FMA(a5, BASD_HI2(A5[0]), BASD_HI2(B5[0]));
#pragma unroll
  for (int ch = 1; ch < MAXCH; ++ch) {
    BASD_D6_FMA(a0, BASD_LO2(A0[ch]), BASD_LO2(B0[ch])); BASD_D6_FMA(a1, BASD_LO2(A1[ch]), BASD_LO2(B1[ch]));
    BASD_D6_FMA(a2, BASD_LO2(A2[ch]), BASD_LO2(B2[ch])); BASD_D6_FMA(a3, BASD_LO2(A3[ch]), BASD_LO2(B3[ch]));
    BASD_D6_FMA(a4, BASD_LO2(A4[ch]), BASD_LO2(B4[ch])); BASD_D6_FMA(a5, BASD_LO2(A5[ch]), BASD_LO2(B5[ch]));
    BASD_D6_FMA(a0, BASD_HI2(A0[ch]), BASD_HI2(B0[ch])); BASD_D6_FMA(a1, BASD_HI2(A1[ch]), BASD_HI2(B1[ch]));
    BASD_D6_FMA(a2, BASD_HI2(A2[ch]), BASD_HI2(B2[ch])); BASD_D6_FMA(a3, BASD_HI2(A3[ch]), BASD_HI2(B3[ch]));
    BASD_D6_FMA(a4, BASD_HI2(A4[ch]), BASD_HI2(B4[ch])); BASD_D6_FMA(a5, BASD_HI2(A5[ch]), BASD_HI2(B5[ch]));
  }
#undef BASD_D6_MUL
#undef BASD_D6_FMA
  p[0] = a0.x + a0.y; p[1] = a1.x + a1.y; p[2] = a2.x + a2.y;
  p[3] = a3.x + a3.y; p[4] = a4.x + a4.y; p[5] = a5.x + a5.y;
}

// One round = six independent rotations (X_i, Y_i), column indices 0..11 (0-5 block P, 6-11 block Q) covering all
// twelve columns of the slot; lane i (of each group of 8) computes rotation i.  The tables are 3 bits per lane:
// which lane of the group owns the entry a lane needs (gather) or produced the entry a lane owns (scatter).
template <int X0, int Y0, int X1, int Y1, int X2, int Y2, int X3, int Y3, int X4, int Y4, int X5, int Y5>
struct Round6 {
  __host__ __device__ static constexpr int X(int i) {
    return i == 0 ? X0 : (i == 1 ? X1 : (i == 2 ? X2 : (i == 3 ? X3 : (i == 4 ? X4 : X5))));
  }
  __host__ __device__ static constexpr int Y(int i) {
    return i == 0 ? Y0 : (i == 1 ? Y1 : (i == 2 ? Y2 : (i == 3 ? Y3 : (i == 4 ? Y4 : Y5))));
  }
  static constexpr int src_of(int col) {
    for (int i = 0; i < 6; ++i) if (X(i) == col || Y(i) == col) return i;
    return 0;
  }
  static constexpr bool from_y(int col) {
    for (int i = 0; i < 6; ++i) if (Y(i) == col) return true;
    return false;
  }
  static constexpr unsigned IDENT = 0 | (1u << 3) | (2u << 6) | (3u << 9) | (4u << 12) | (5u << 15) | (6u << 18) | (7u << 21);
  static constexpr unsigned tail = (6u << 18) | (7u << 21);    // lanes 6, 7 of a group point at themselves
  static constexpr unsigned gx_tbl() { unsigned t = tail; for (int i = 0; i < 6; ++i) t |= (unsigned)(X(i) % 6) << (3 * i); return t; }
  static constexpr unsigned gy_tbl() { unsigned t = tail; for (int i = 0; i < 6; ++i) t |= (unsigned)(Y(i) % 6) << (3 * i); return t; }
  static constexpr unsigned xq_msk() { unsigned t = 0; for (int i = 0; i < 6; ++i) t |= (unsigned)(X(i) / 6) << i; return t; }
  static constexpr unsigned yq_msk() { unsigned t = 0; for (int i = 0; i < 6; ++i) t |= (unsigned)(Y(i) / 6) << i; return t; }
  static constexpr unsigned sp_tbl() { unsigned t = tail; for (int j = 0; j < 6; ++j) t |= (unsigned)src_of(j) << (3 * j); return t; }
  static constexpr unsigned sq_tbl() { unsigned t = tail; for (int j = 0; j < 6; ++j) t |= (unsigned)src_of(6 + j) << (3 * j); return t; }
  static constexpr unsigned py_msk() { unsigned t = 0; for (int j = 0; j < 6; ++j) t |= (from_y(j) ? 1u : 0u) << j; return t; }
  static constexpr unsigned qy_msk() { unsigned t = 0; for (int j = 0; j < 6; ++j) t |= (from_y(6 + j) ? 1u : 0u) << j; return t; }
  static constexpr unsigned gx = gx_tbl(), gy = gy_tbl(), xq = xq_msk(), yq = yq_msk();
  static constexpr unsigned sp = sp_tbl(), sq = sq_tbl(), py = py_msk(), qy = qy_msk();
};
// entry of the lane the table names: register mp where the mask bit of this lane is 0, mq where it is 1
template <unsigned TBL, unsigned MASK, unsigned IDENT>
__device__ __forceinline__ float meta_move6(float mp, float mq, int q8, int idx4) {
  if constexpr (TBL == IDENT) {
    if constexpr (MASK == 0) return mp;
    else if constexpr (MASK == 0x3F) return mq;
    else return ((MASK >> q8) & 1) ? mq : mp;
  } else {
    if constexpr (MASK == 0) return bperm(idx4, mp);
    else if constexpr (MASK == 0x3F) return bperm(idx4, mq);
    else {
      const float a = bperm(idx4, mp), b = bperm(idx4, mq);
      return ((MASK >> q8) & 1) ? b : a;
    }
  }
}

// Hex-block: lane i < 6 of every group of 8 computes rotation i and owns column i of either block (lanes 6, 7 idle
// along: their entries are kept at zero and they never rotate); entries move over the LDS crossbar.
template <> struct BlockOrder<6> {
  struct Lane {
    int q8;                                        // lane within its group of 8
    bool bit0, bit1, bit2;
    bool rlane;                                    // this lane computes a rotation / owns a column entry
    int grp4;                                      // byte index of lane 0 of this lane's group of 8 (ds_bpermute)
  };
  __device__ __forceinline__ static Lane lane(int tid, int sub) {
    return {sub & 7, (sub & 1) != 0, (sub & 2) != 0, (sub & 4) != 0, (sub & 7) < 6, ((tid & 63) & ~7) << 2};
  }
  __device__ __forceinline__ static bool owner(const Lane& L, int /*sub*/) { return L.rlane; }
  __device__ __forceinline__ static int meta_col(const Lane& L) { return L.rlane ? L.q8 : 5; }
  // 16 slots: four waves at 16 lanes, eight at 32 (columns of up to 384 rows at the same 144 column VGPRs: the block
  // pairs of the D_s = 384 eigensolver)
  static constexpr int max_threads(int /*maxch*/, int lanes) { return 16 * lanes; }
  static constexpr int status_kind = 7;
  // the crossbar has latency: a round asks for the entries of its columns before the dot products, which hide it, and
  // hands the new ones back after the parameter broadcasts
  static constexpr bool entries_first = true;

  template <class M, int MAXCH> __device__ __forceinline__ static void dots(const v4f (&C)[12][MAXCH], float (&p)[6]) {
    dot6_cols<MAXCH>(C[M::X(0)], C[M::Y(0)], C[M::X(1)], C[M::Y(1)], C[M::X(2)], C[M::Y(2)], C[M::X(3)], C[M::Y(3)],
                     C[M::X(4)], C[M::Y(4)], C[M::X(5)], C[M::Y(5)], p);
  }
  template <int LANES> __device__ __forceinline__ static float reduce_scatter(const float (&p)[6], const Lane& L) {
    return reduce_scatter6<LANES>(p, L.bit0, L.bit1, L.bit2);
  }
  template <unsigned TBL, unsigned MASK, unsigned IDENT>
  __device__ __forceinline__ static float move(float mp, float mq, const Lane& L) {
    return meta_move6<TBL, MASK, IDENT>(mp, mq, L.q8, L.grp4 | (((TBL >> (3 * L.q8)) & 7) << 2));
  }
  template <class M> __device__ __forceinline__ static float gather_x(float mp, float mq, const Lane& L) {
    return move<M::gx, M::xq, M::IDENT>(mp, mq, L);
  }
  template <class M> __device__ __forceinline__ static float gather_y(float mp, float mq, const Lane& L) {
    return move<M::gy, M::yq, M::IDENT>(mp, mq, L);
  }
  template <class M> __device__ __forceinline__ static float scatter_p(float xn, float yn, const Lane& L) {
    return move<M::sp, M::py, M::IDENT>(xn, yn, L);
  }
  template <class M> __device__ __forceinline__ static float scatter_q(float xn, float yn, const Lane& L) {
    return move<M::sq, M::qy, M::IDENT>(xn, yn, L);
  }
  // (measured for the (a, b) pairs of a round: through 96 bytes of LDS per slot -- one 8-byte write by the parameter
  // lanes, three 16-byte broadcast reads by all lanes -- instead of twelve swizzles: 3.335 vs 3.32 ms per 1024 x 192^2,
  // 0.97 vs 0.98 for a single matrix: the crossbar operations are not what a round waits for; not kept)
  template <int I> __device__ __forceinline__ static float bcast(float v) { return bcast8<I>(v); }
  // the fifteen pairs inside each block, once per sweep: five rounds of three pairs per block
  template <class F> __device__ __forceinline__ static void inner_rounds(F&& round, bool ok) {
    round(Round6<0, 5, 1, 4, 2, 3, 6, 11, 7, 10, 8, 9>{}, ok);
    round(Round6<0, 4, 5, 3, 1, 2, 6, 10, 11, 9, 7, 8>{}, ok);
    round(Round6<0, 3, 4, 2, 5, 1, 6, 9, 10, 8, 11, 7>{}, ok);
    round(Round6<0, 2, 3, 1, 4, 5, 6, 8, 9, 7, 10, 11>{}, ok);
    round(Round6<0, 1, 2, 5, 3, 4, 6, 7, 8, 11, 9, 10>{}, ok);
  }
  // a meeting of blocks P and Q: 36 cross rotations in six rounds
  template <class F> __device__ __forceinline__ static void cross_rounds(F&& round, bool ok) {
    round(Round6<0, 6, 1, 7, 2, 8, 3, 9, 4, 10, 5, 11>{}, ok);
    round(Round6<0, 7, 1, 8, 2, 9, 3, 10, 4, 11, 5, 6>{}, ok);
    round(Round6<0, 8, 1, 9, 2, 10, 3, 11, 4, 6, 5, 7>{}, ok);
    round(Round6<0, 9, 1, 10, 2, 11, 3, 6, 4, 7, 5, 8>{}, ok);
    round(Round6<0, 10, 1, 11, 2, 6, 3, 7, 4, 8, 5, 9>{}, ok);
    round(Round6<0, 11, 1, 6, 2, 7, 3, 8, 4, 9, 5, 10>{}, ok);
  }
};

// The block kernel: one workgroup per matrix, a slot of LANES lanes owns two blocks (P, Q) of BC columns, 4 * LANES
// rows per chunk, MAXCH chunks.  BlockOrder<BC> supplies what depends on the block width; the sweep, the debris pass,
// the hand-over, convergence, ranking and write-back below are the same for both orderings.
// OCC = waves per SIMD the register allocation aims at.  Hex-block at three chunks: 1 (a batch that leaves every CU at
// most one matrix at a time: no spills, the latency of the parameter stream is all that counts) or 2 (two matrices
// per CU hide each other's parameter stream).
template <int BC, int MAXCH, int OCC, int LANES>
__global__ __launch_bounds__(BlockOrder<BC>::max_threads(MAXCH, LANES))
__attribute__((amdgpu_waves_per_eu(OCC, OCC))) void jacobi_block_kernel(
    float* __restrict__ wg, int batch, int m, int n, int ld, int norm_rows, float tol, int max_sweeps, int sort,
    float* __restrict__ sigma, int32_t* __restrict__ sweeps_out, int32_t* __restrict__ status,
    const int32_t* __restrict__ active, int active_mode) {
  // active_mode 0: no `active`; 1: active[mat] = number of leading non-zero columns (the tournament runs over those,
  // the other columns are zero and stay zero); 2: the same and only the leading active[mat] ROWS are non-zero;
  // 3: `active` is a mask (< 0: skip the matrix, otherwise solve it completely)
  using P = BlockOrder<BC>;
  extern __shared__ __align__(16) float lds[];
  const int mat = blockIdx.x;
  int n_act = n;
  if (active_mode != 0) {
    const int av = active[mat];
    if (av < 0) {                                  // masked problem (any mode): nothing is read or written
      if (sweeps_out && threadIdx.x == 0) sweeps_out[mat] = 0;
      return;
    }
    if (active_mode != 3) n_act = av < 2 ? 2 : (av > n ? n : av);
  }
  constexpr int NC = 2 * BC;                       // columns of a slot: 0 .. BC-1 block P, BC .. NC-1 block Q
  constexpr int CHR = 4 * LANES;                   // rows of one chunk (4 per lane)
  constexpr int LDC = CHR * MAXCH;                 // one column in the mailbox
  constexpr int LDB = BC * LDC;                    // one block
  const int tid = threadIdx.x;
  const int k = tid / LANES, sub = tid % LANES, roff = sub * 4;
  const typename P::Lane L = P::lane(tid, sub);
  const int nb_all = ceil_div<BC>(n);
  const int S_all = (nb_all + 1) >> 1;             // slots the launch provides (threads / LANES, rounded up to waves)
  const int nb = ceil_div<BC>(n_act);              // blocks that hold active columns
  const int nbe = nb + (nb & 1);                   // line length in blocks (a zero phantom block pads odd nb)
  const int S = nbe >> 1;                          // slots that take part
  float* mbox = lds;                               // [S_all + 1][LDB]
  float* s_sig = mbox + (size_t)(S_all + 1) * LDB; // [NC S_all] by position
  int* s_rank = reinterpret_cast<int*>(s_sig + 200);      // [NC S_all]
  float* s_nrm = reinterpret_cast<float*>(s_rank + 200);  // [S_all + 1][BC] squared norms travelling with the mailbox
  float* s_scl = s_nrm + 104;                      // [S_all + 1][BC] scales
  int* s_flag = reinterpret_cast<int*>(s_scl + 104);      // [2] any rotation, [2] any LARGE rotation, [2] max norm

  float* src = wg + (size_t)mat * n * ld;
  int mr = (m + 3) & ~3;
  if (active_mode == 2) { const int ma = (n_act + 3) & ~3; mr = ma < mr ? ma : mr; }
  const bool live = k < S;
  const bool last = k == S - 1;
  float* const mybox = mbox + (size_t)k * LDB + roff;          // box k, this lane's rows
  float* const mymeta = s_nrm + BC * k + P::meta_col(L);       // box k, this lane's column: norm, +104 scale
  v4f C[NC][MAXCH];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int idc = NC * k + c;
#pragma unroll
    for (int ch = 0; ch < MAXCH; ++ch) {
      const int r = roff + CHR * ch;
      C[c][ch] = (live && idc < n_act && r < mr) ? *reinterpret_cast<const v4f*>(src + (size_t)idc * ld + r)
                                                 : (v4f){0.f, 0.f, 0.f, 0.f};
    }
  }
  // distributed bookkeeping: an owner lane holds the entry of one column of block P (nP, dP) and of one of block Q.
  // Column ids are NOT carried: blocks move as wholes on a data-independent schedule -- a sweep of the odd-even
  // transposition line reverses the block order, so after s sweeps position p holds block (s odd ? nbe - 1 - p : p).
  float nP = 0.f, nQ = 0.f, dP = 1.f, dQ = 1.f;
  if (tid < 8) s_flag[tid] = 0;
  __syncthreads();

  const float inv_tol = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(1.0f / tol)));
  bool rotated = false, bigrot = false;

  // one round: BC independent rotations (M::X(i), M::Y(i)) covering all NC columns of the slot
  auto round = [&](auto map, bool ok) {
    using M = decltype(map);
    // WHERE the entries of the round's columns are fetched and handed back is the ordering's (P::entries_first): the
    // instruction schedule and the register allocation of these kernels follow the statement order
    float al, be, dx, dy;
    auto fetch = [&] {
      al = P::template gather_x<M>(nP, nQ, L); be = P::template gather_y<M>(nP, nQ, L);
      dx = P::template gather_x<M>(dP, dQ, L); dy = P::template gather_y<M>(dP, dQ, L);
    };
    if constexpr (P::entries_first) fetch();
    float p[BC];
    P::template dots<M, MAXCH>(C, p);
    const float gt = P::template reduce_scatter<LANES>(p, L);
    if constexpr (!P::entries_first) fetch();
    const float g = gt * dx * dy;                 // dot product of the true columns
    const float gsc = g * inv_tol;
    const float ab_ = al * be;
    const bool rot = ok & L.rlane & (gsc * gsc > fmaxf(ab_, BASD_JACOBI_TINY));
    // no branch around the rotation: a round in which all rotations of the wave are below the threshold only
    // occurs on padded / rank-deficient columns (the solve stops after the first sweep of small rotations), and a
    // merge point after the in-place shears costs 48 register moves per round (the allocator does not coalesce the
    // halves of the column registers across it); converged pairs run the shears with a = b = 0, an exact no-op
    rotated |= rot;
    const float gq = g * (1.0f / BASD_JACOBI_QUAD);
    const bool big_cos = gq * gq > ab_;
    const float z = (be - al) * __builtin_amdgcn_rcpf(2.f * g);
    float t = copysignf(1.f, z) * __builtin_amdgcn_rcpf(fabsf(z) + __builtin_amdgcn_sqrtf(fmaf(z, z, 1.f)));
    t = rot ? t : 0.f;
    bigrot |= rot & (big_cos | (fabsf(t) > BASD_JACOBI_QUAD_TAN));
    const float w = fmaf(t, t, 1.f);
    float c = __builtin_amdgcn_rsqf(w);
    c = c * fmaf(-0.5f * w, c * c, 1.5f);
    const float sn = c * t;
    const float u = sn * __builtin_amdgcn_rcpf(1.0f + c);
    const float h = sn * u, hp = t * u;            // 1 - c and 1 / c - 1, no cancellation
    const float aln = fmaf(-t, g, al), ben = fmaf(t, g, be);
    const float a = t * (dy * __builtin_amdgcn_rcpf(dx));
    const float b = (sn * c) * (dx * __builtin_amdgcn_rcpf(dy));
    const float dxn = fmaf(-dx, h, dx), dyn = fmaf(dy, hp, dy);
    auto hand_back = [&] {
      nP = P::template scatter_p<M>(aln, ben, L);
      nQ = P::template scatter_q<M>(aln, ben, L);
      dP = P::template scatter_p<M>(dxn, dyn, L);
      dQ = P::template scatter_q<M>(dxn, dyn, L);
    };
    if constexpr (!P::entries_first) hand_back();
    v2f_rot ab[BC];
    static_for<BC>([&](auto i) { ab[i] = (v2f_rot){P::template bcast<i>(a), P::template bcast<i>(b)}; });
    if constexpr (P::entries_first) hand_back();
#pragma unroll
    for (int i = 0; i < BC; ++i) {
#pragma unroll
      for (int ch = 0; ch < MAXCH; ++ch) shear_in_place(C[M::X(i)][ch], C[M::Y(i)][ch], ab[i]);
    }
    __builtin_amdgcn_sched_barrier(0);
  };

  // fold the scales into the columns (x <- d x~, d <- 1); `kill` zeroes a column instead
  auto fold = [&](bool killP, bool killQ) {
    const float fP = killP ? 0.f : dP, fQ = killQ ? 0.f : dQ;
    float f[2][BC];
    static_for<BC>([&](auto i) { f[0][i] = P::template bcast<i>(fP); });
    static_for<BC>([&](auto i) { f[1][i] = P::template bcast<i>(fQ); });
#pragma unroll
    for (int c = 0; c < NC; ++c) {
#pragma unroll
      for (int ch = 0; ch < MAXCH; ++ch) C[c][ch] *= f[c / BC][c % BC];
    }
    dP = 1.f; dQ = 1.f;
  };
  auto exact_norms = [&](int rows) {
    float p[2][BC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      float a = 0.f;
#pragma unroll
      for (int ch = 0; ch < MAXCH; ++ch) {
        const int r = roff + CHR * ch;
        const v4f x = C[c][ch];
        const float mx = (r + 0 < rows) ? 1.f : 0.f, my = (r + 1 < rows) ? 1.f : 0.f;
        const float mz = (r + 2 < rows) ? 1.f : 0.f, mw = (r + 3 < rows) ? 1.f : 0.f;
        a = fmaf(mx * x.x, x.x, fmaf(my * x.y, x.y, fmaf(mz * x.z, x.z, fmaf(mw * x.w, x.w, a))));
      }
      p[c / BC][c % BC] = a;
    }
    nP = P::template reduce_scatter<LANES>(p[0], L);
    nQ = P::template reduce_scatter<LANES>(p[1], L);
    if (!L.rlane) { nP = 0.f; nQ = 0.f; }
  };

  int used_sweeps = 0;
  bool converged = false;
  int step = 0;                                    // even = blocks (2k, 2k+1); nbe is even, sweeps start and end there
#pragma unroll 1
  for (int sweep = 0; sweep < max_sweeps; ++sweep) {
    rotated = false;
    bigrot = false;
    fold(false, false);
    exact_norms(1 << 30);
    if (live && P::owner(L, sub)) atomicMax(&s_flag[4 + (sweep & 1)], __float_as_int(fmaxf(nP, nQ)));
    lds_barrier();
    {
      const float debris = __int_as_float(s_flag[4 + (sweep & 1)]) * BASD_JACOBI_DEBRIS;
      const bool zP = L.rlane & (nP < debris), zQ = L.rlane & (nQ < debris);   // debris columns become exact zero columns
      if (__builtin_amdgcn_ballot_w64(zP || zQ) != 0) {
        fold(zP, zQ);
        if (zP) nP = 0.f;
        if (zQ) nQ = 0.f;
      }
    }
    P::inner_rounds(round, live);
#pragma unroll 1
    for (int t = 0; t < nbe; ++t, ++step) {
      const bool even_view = (step & 1) == 0;
      const bool pair_ok = live & (even_view | !last);
      P::cross_rounds(round, pair_ok);
      // ---- hand one block over (positions swap after a meeting: the pair is then stored as lo = Q, hi = P).
      // ONE base address per lane for the boxes and one for their bookkeeping entries; everything else is an
      // immediate offset (box k at 0, box k + 1 at LDB; norms / scales 104 entries apart)
      if (even_view) {
        // Q (block position 2k) goes to slot k-1 through box k (slot 0's stays parked there); the last slot has no
        // right neighbour: it parks its P in box S and takes it back as Q (its lone block of the odd view)
        if (live) {
#pragma unroll
          for (int c = 0; c < BC; ++c) {
#pragma unroll
            for (int ch = 0; ch < MAXCH; ++ch) *reinterpret_cast<v4f*>(mybox + c * LDC + CHR * ch) = C[BC + c][ch];
          }
          if (sub < BC) { mymeta[0] = nQ; mymeta[104] = dQ; }
          if (last) {
#pragma unroll
            for (int c = 0; c < BC; ++c) {
#pragma unroll
              for (int ch = 0; ch < MAXCH; ++ch) *reinterpret_cast<v4f*>(mybox + LDB + c * LDC + CHR * ch) = C[c][ch];
            }
            if (sub < BC) { mymeta[BC] = nP; mymeta[104 + BC] = dP; }
          }
        }
        lds_barrier();
        if (live) {
#pragma unroll
          for (int c = 0; c < BC; ++c) {
#pragma unroll
            for (int ch = 0; ch < MAXCH; ++ch) C[BC + c][ch] = *reinterpret_cast<const v4f*>(mybox + LDB + c * LDC + CHR * ch);
          }
          nQ = mymeta[BC]; dQ = mymeta[104 + BC];
        }
      } else {
        // P (position 2k+2 after the swap) goes to slot k+1 through box k+1; slot 0 takes the parked block back
        if (live && !last) {
#pragma unroll
          for (int c = 0; c < BC; ++c) {
#pragma unroll
            for (int ch = 0; ch < MAXCH; ++ch) *reinterpret_cast<v4f*>(mybox + LDB + c * LDC + CHR * ch) = C[c][ch];
          }
          if (sub < BC) { mymeta[BC] = nP; mymeta[104 + BC] = dP; }
        }
        lds_barrier();
        if (live) {
#pragma unroll
          for (int c = 0; c < BC; ++c) {
#pragma unroll
            for (int ch = 0; ch < MAXCH; ++ch) C[c][ch] = *reinterpret_cast<const v4f*>(mybox + c * LDC + CHR * ch);
          }
          nP = mymeta[0]; dP = mymeta[104];
        }
      }
      // no second barrier: the next write to a box comes from the slot that has just read it (see the quad-block header)
    }
    used_sweeps = sweep + 1;
    if (rotated) s_flag[sweep & 1] = 1;
    if (bigrot) s_flag[2 + (sweep & 1)] = 1;
    lds_barrier();
    const int any = s_flag[sweep & 1], anybig = s_flag[2 + (sweep & 1)];
    if (tid == 0) { s_flag[(sweep + 1) & 1] = 0; s_flag[2 + ((sweep + 1) & 1)] = 0; s_flag[4 + ((sweep + 1) & 1)] = 0; }
    lds_barrier();
    if (!any || !anybig) { converged = true; break; }
  }

  // ---- singular values = norms of the true columns over the first norm_rows rows
  fold(false, false);
  exact_norms(norm_rows);
  lds_barrier();                                   // every wave is out of the sweep loop (mailbox reads done)
  // The thread-derived indices are re-derived here from an opaque copy of the thread id: kept live across the sweep
  // loop they cost registers the rotation rounds need (the allocator spills them into the inner loop otherwise).
  int tid2 = threadIdx.x;
  asm volatile("" : "+v"(tid2));
  const int k2 = tid2 / LANES, sub2 = tid2 % LANES, roff2 = sub2 * 4;
  const bool live2 = k2 < S;
  // column ids by position: live slots hold block (sweeps odd ? nbe - 1 - p : p) at block position p; slots beyond
  // the tournament never moved.  Ranking levels: active columns >= 0, inactive real columns -1, phantoms (id >= n) -2.
  const bool odd = (used_sweeps & 1) != 0;
  const int bP = live2 ? (odd ? nbe - 1 - 2 * k2 : 2 * k2) : 2 * k2;
  const int bQ = live2 ? (odd ? nbe - 2 - 2 * k2 : 2 * k2 + 1) : 2 * k2 + 1;
  if (k2 < S_all && sub2 < BC) {
    const int idP = BC * bP + sub2, idQ = BC * bQ + sub2;
    s_sig[NC * k2 + sub2] = idP >= n ? -2.f : ((live2 && idP < n_act) ? sqrtf(nP) : -1.f);
    s_sig[NC * k2 + BC + sub2] = idQ >= n ? -2.f : ((live2 && idQ < n_act) ? sqrtf(nQ) : -1.f);
  }
  lds_barrier();
  const int n_tot = NC * S_all;                    // >= n
  for (int p = tid2; p < n_tot; p += blockDim.x) {
    int rank = p;
    if (sort) {
      const float mine = s_sig[p];
      rank = 0;
      for (int c = 0; c < n_tot; ++c) {
        const float o = s_sig[c];
        rank += (o > mine) || (o == mine && c < p);
      }
    }
    s_rank[p] = rank;
  }
  lds_barrier();
  if (k2 < S_all) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int idc = BC * (c < BC ? bP : bQ) + (c % BC);
      const int d = sort ? s_rank[NC * k2 + c] : idc;
      const float sg = s_sig[NC * k2 + c];
      if (idc < n && d < n) {
#pragma unroll
        for (int ch = 0; ch < MAXCH; ++ch) {
          const int r = roff2 + CHR * ch;
          if (r < ld) *reinterpret_cast<v4f*>(src + (size_t)d * ld + r) = (live2 && r < mr) ? C[c][ch] : (v4f){0.f, 0.f, 0.f, 0.f};
        }
        if (sub2 == 0) sigma[(size_t)mat * n + d] = sg < 0.f ? 0.f : sg;
      }
    }
  }
  if (sweeps_out && tid2 == 0) sweeps_out[mat] = converged ? used_sweeps : -used_sweeps;
  report_status(status, converged, s_sig, n_tot, tid2, blockDim.x, P::status_kind, mat);
}

}  // namespace basd

// Shape classes in priority order; each is tested on (rows4, n_cols) alone, so batch size and `active` never change
// the class (only the hex-block kernel's occupancy variant looks at the batch size).  Anything outside them is
// BASD_ERR_SHAPE (DESIGN.md section 5 has the table).
//   hex-block   129 .. 192 columns, rows4 <= 192 (16-lane slots) or 257 .. 384 (32-lane slots)
//   quad-block  8 .. 192 columns up to 384 rows (32-lane slots above 256), 8 .. 196 columns at 193 .. 256 rows
//   odd-even    rows4 <= 224: what is left, i.e. fewer than 8 or more than 192 (196) columns
//   tall        fewer than 8 columns, 225 .. 384 rows
extern "C" int basd_jacobi_svd(float* w, int batch, int m_rows, int n_cols, int ld, int norm_rows,
                               float tol, int max_sweeps, int sort, float* sigma,
                               int32_t* sweeps, const int32_t* active, int active_rows, int32_t* status,
                               void* stream) {
  using namespace basd;
  if (batch <= 0) return BASD_OK;
  if (n_cols < 1 || n_cols > BASD_JACOBI_MAX_COLS || ld % 4 != 0 || m_rows > ld || m_rows < 1 ||
      norm_rows < 1 || norm_rows > m_rows)
    return fail(BASD_ERR_SHAPE, "jacobi_svd: bad shape m=%d n=%d ld=%d norm_rows=%d", m_rows, n_cols, ld, norm_rows);
  hipStream_t st = (hipStream_t)stream;
  const int rows4 = (m_rows + 3) & ~3;
  // active_rows == 2: `active` is a MASK -- entries are either < 0 (skip the matrix) or n_cols (solve it completely)
  const bool mask_only = active != nullptr && active_rows == 2;
  if (mask_only) active_rows = 0;
  const int mode = active == nullptr ? 0 : (mask_only ? 3 : (active_rows ? 2 : 1));      // the block kernels' view of it

  // block kernels: a slot of `lanes` lanes owns two blocks of BC columns, 4 * lanes rows per chunk; the mailbox holds
  // one block per slot and one spare
  const int lanes = rows4 > 256 ? 32 : 16;
  const int chn = (rows4 + 4 * lanes - 1) / (4 * lanes);
  auto launch_block = [&](auto kernel, int bc, const char* what) {
    const int slots = ((n_cols + bc - 1) / bc + 1) / 2;
    const int threads = ((slots * lanes + 63) / 64) * 64;
    const size_t lds = ((size_t)(slots + 1) * bc * 4 * lanes * chn + 200 * 2 + 104 * 2 + 8) * 4;
    if (lds > BASD_JACOBI_LDS_BYTES)
      return fail(BASD_ERR_SHAPE, "jacobi_svd: %d x %d needs %zu B of LDS", m_rows, n_cols, lds);
    allow_full_lds((const void*)kernel);
    hipLaunchKernelGGL(kernel, dim3(batch), dim3(threads), lds, st, w, batch, m_rows, n_cols, ld, norm_rows, tol,
                       max_sweeps, sort, sigma, sweeps, status, active, mode);
    return check_launch(what);
  };
  // odd-even kernels: an 8-lane slot per column pair, NBUF mailboxes of one column (32 * MAXCH rows) per slot
  auto launch_oe = [&](auto kernel, int maxch, int nbuf, const char* what) {
    const int npairs = (n_cols + 1) / 2;
    const int threads = ((npairs * 8 + 63) / 64) * 64;
    const size_t lds = (size_t)nbuf * npairs * 32 * maxch * 4 + JACOBI_OE_SCRATCH;
    allow_full_lds((const void*)kernel);
    hipLaunchKernelGGL(kernel, dim3(batch), dim3(threads), lds, st, w, batch, m_rows, n_cols, ld, norm_rows, tol,
                       max_sweeps, sort, sigma, sweeps, active, active_rows, status);
    return check_launch(what);
  };

  // (hex-block from 129 columns: below that the quad-block kernel is four waves or fewer itself and its shorter rounds
  // win -- 48 x 64^2: 0.136 vs 0.210 ms)
  if (n_cols > 128 && n_cols <= 192 && (rows4 <= 192 || (rows4 > 256 && rows4 <= 384))) {
    const char* what = "jacobi_svd (hex-block, scaled rotations)";
    if (lanes == 32) return launch_block(jacobi_block_kernel<6, 3, 2, 32>, 6, what);
    if (chn == 1) return launch_block(jacobi_block_kernel<6, 1, 2, 16>, 6, what);
    if (chn == 2) return launch_block(jacobi_block_kernel<6, 2, 2, 16>, 6, what);
    // 144 column VGPRs: a second workgroup per SIMD only pays once every CU has more than one matrix
    if (batch > 256) return launch_block(jacobi_block_kernel<6, 3, 2, 16>, 6, what);
    return launch_block(jacobi_block_kernel<6, 3, 1, 16>, 6, what);
  }
  if (n_cols >= 8 && rows4 <= 384 && n_cols <= ((rows4 > 192 && rows4 <= 256) ? 196 : 192)) {
    const char* what = "jacobi_svd (quad-block, scaled rotations)";
    if (lanes == 32) return launch_block(jacobi_block_kernel<4, 3, 3, 32>, 4, what);
    if (chn == 1) return launch_block(jacobi_block_kernel<4, 1, 3, 16>, 4, what);
    if (chn == 2) return launch_block(jacobi_block_kernel<4, 2, 3, 16>, 4, what);
    if (chn == 3) return launch_block(jacobi_block_kernel<4, 3, 3, 16>, 4, what);
    return launch_block(jacobi_block_kernel<4, 4, 2, 16>, 4, what);
  }
  if (rows4 <= 224) {
    // 2, 4, 6 or 7 chunks of 32 rows in registers; double-buffered mailbox if it fits, else a single one (more than
    // 204 columns of 129 .. 192 rows, more than 196 of 193 .. 224: the 196-token Procrustes cores of the wide students)
    const int chunks = (rows4 + 31) / 32;
    const int maxch = chunks <= 2 ? 2 : (chunks <= 4 ? 4 : (chunks <= 6 ? 6 : 7));
    const size_t lds2 = (size_t)2 * ((n_cols + 1) / 2) * 32 * maxch * 4 + JACOBI_OE_SCRATCH;
    if (lds2 > BASD_JACOBI_LDS_BYTES)
      return launch_oe(jacobi_oe_kernel<7, 1, 1>, 7, 1, "jacobi_svd (odd-even, single mailbox)");
    const char* what = "jacobi_svd (odd-even)";
    if (maxch == 2) return launch_oe(jacobi_oe_kernel<2, 1, 2>, 2, 2, what);
    if (maxch == 4) return launch_oe(jacobi_oe_kernel<4, 1, 2>, 4, 2, what);
    if (maxch == 6) return launch_oe(jacobi_oe_kernel<6, 1, 2>, 6, 2, what);
    return launch_oe(jacobi_oe_kernel<7, 1, 2>, 7, 2, what);
  }
  if (n_cols < 8 && rows4 <= 384)   // single mailbox, 3 waves per SIMD
    return launch_oe(jacobi_oe_kernel<12, 1, 1>, 12, 1, "jacobi_svd (odd-even, tall columns)");
  return fail(BASD_ERR_SHAPE, "jacobi_svd: %d rows x %d columns is outside every kernel's domain (DESIGN.md section 5)",
              m_rows, n_cols);
}
