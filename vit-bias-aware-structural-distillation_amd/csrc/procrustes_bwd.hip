// Backward of the attention-weighted Procrustes term as ONE C entry (reference: autograd of
// src/losses/relational.py:47-48, i.e. svd_backward of the nuclear norm = the polar factor U V^T, then the centring /
// weighting of :29-46).  With the factors the forward saved (basd_procrustes_fwd: fac_s, a_t) the gradient w.r.t. the
// weighted tokens is a residual
//     R_t = t_w - (s_w G)   = t_w - a_t t_w        [n, d_t]        (G = U V^T, never formed)
//     R_s = s_w - (t_w G^T) = s_w - a_s s_w (token side)  or  s_w - fac_s (feature side)       [n, d_s]
// scaled per row, g = 2 gl sqrt(a) R, plus the row dots 2 gl <R, W> that make up d loss / d a.
//
// The one big product, a_t t_w (batch x [n, n] x [n, d_t]: 60 GFLOP at BASELINE c2), ran as a library fp32 bmm
// (0.62 ms) followed by basd_procrustes_bwd_rows (another 1.9 GB pass).  Here it runs on the bf16 matrix cores as a
// THREE-PRODUCT SPLIT of both fp32 operands (x = hi + mid + ..., hi = bf16(x), mid = bf16(x - hi);
// A W ~ A_hi W_hi + A_hi W_mid + A_mid W_hi: relative error 2^-16 of |A| |W| -- the gradient tolerance is 5e-4), with
// the residual, the scaling and the row dots in the epilogue of the same kernel: t_w is read once as the B operand and
// once (L2-hot) as the residual's W, g_t is written once, nothing else touches HBM.
//
// One workgroup (6 waves; two workgroups per CU, three waves per SIMD: one's barriers and epilogue overlap the other's
// matrix work) per matrix of the batch.  The A factor ([n, n] fp32) is staged per 32-wide K step into LDS as two bf16 planes (split on the way
// in; 80-byte rows: conflict-free 16-byte fragment reads), double buffered, its global loads issued one step ahead; a
// wave owns one 16-column strip of the current 96-column group and keeps its B fragment (loaded straight from global
// memory, 64 contiguous bytes per 16 lanes, split in registers) for one K step at a time, prefetched one step ahead;
// accumulators: MT tiles of 16 x 16 fp32 (52 VGPRs at 196 rows).  v_mfma_f32_16x16x32_bf16, fp32 accumulation.
//
// Measured (round 4, 1024 x [196, 196] x [196, 768], one MI355X): 1.10 ms for the whole backward against 1.00 ms with the
// library fp32 bmm (0.62) + two row passes; inside the captured step the two are equal within the noise (35.93 vs 35.79
// ms).  PMC of this kernel: 1.70 GB fetched / 0.71 GB written (1.23 + 0.62 algorithmic), 74 % of the wave cycles
// WAITING, 14 % issuing, matrix cores busy 23 %: it is bound by one exposed memory round trip per K step (the B strip
// is a cold HBM read and the 39 MFMAs of a step last 0.3 us), not by arithmetic or bandwidth.  Tried on the way and
// dropped: 8 waves x 2 strips (104 accumulator registers: 85 - 300 spilled VGPRs whatever the fencing), the residual in
// the accumulator layout (4-byte loads / stores + 16-lane reductions: 0.8 of 1.2 ms), fragment reads in two batches
// (no change), the whole B strip of a group loaded in one burst into 56 registers (the right idea for the measured
// bottleneck, but 259 spilled registers at the 168-register budget of three waves per SIMD: 1.78 ms).
// From five m tiles on (n > 64) these kernels are replaced by procrustes_bwd_side_resident_kernel below (0.94 -> 0.52 ms
// at the shape above); they remain for n <= 64 and for up to 128 rows with fewer than 112 columns.
// The file: the pieces all kernels share (pb_*, PbStage*), then the direct kernel (W from global memory: n <= 48), the
// tiled kernel (W through LDS: one row tile up to 128 rows, row tiles of 128 from 257 rows on and for n % 4 != 0), the
// resident kernel (5 to 16 m tiles) and the dispatch.
#include "basd_frag.h"

namespace basd {

constexpr int PB_ROWB = 80;                 // bytes per staged A row (32 bf16 = 64 + 16 pad)
constexpr int PB_WAVES = 6;                 // waves per workgroup: two workgroups per CU at three waves per SIMD (168 VGPRs)
constexpr int PB_THREADS = 64 * PB_WAVES;

// (hi, mid) bf16 split of two floats, packed: hi = bf16(x) (round to nearest even), mid = bf16(x - hi)
__device__ __forceinline__ void pb_split2(float x0, float x1, unsigned int& hi, unsigned int& mid) {
  const bf16x2 h = __builtin_convertvector((f32x2){x0, x1}, bf16x2);
  const f32x2 hf = __builtin_convertvector(h, f32x2);
  const bf16x2 m = __builtin_convertvector((f32x2){x0 - hf.x, x1 - hf.y}, bf16x2);
  hi = __builtin_bit_cast(unsigned int, h);
  mid = __builtin_bit_cast(unsigned int, m);
}

constexpr int PB_BPITCH = 208;              // bytes between the k rows of the staged W tile (96 bf16 = 192 + 16 pad)

// ---- the pieces every kernel of this file is made of, each written once -------------------------------------------
// `out` and `rowdot` have the same bits whichever kernel the dispatch picks (no atomics, a fixed slot order), so a
// training run does not change when a dispatch boundary moves.  That holds because the arithmetic of a tile -- the
// masked (hi, mid) split of both operands, K ascending in steps of 32 with the MFMAs in the order hi hi, hi mid, mid hi,
// the epilogue's residual, scale, fmaf chain and quad reduction, the six row-dot slots added in order -- is THIS code
// in every kernel.  An edit here reaches all of them; an edit that forks one of them breaks the rule.

// Row scales 2 gl sqrt(a) of the rows r0 .. r0 + trows - 1 (0 for padded rows) and the zeroed [PB_WAVES][rows] row dots
__device__ __forceinline__ void pb_rows_init(float* s_c, float* s_dot, int rows, int tid, int threads,
                                             const float* __restrict__ a_b, float c2, int r0, int trows, int n) {
  for (int i = tid; i < rows; i += threads) {
#pragma unroll
    for (int j = 0; j < PB_WAVES; ++j) s_dot[j * rows + i] = 0.f;
    s_c[i] = (i < trows && r0 + i < n) ? c2 * __builtin_amdgcn_sqrtf(a_b[r0 + i]) : 0.f;
  }
}

// rowdot = the PB_WAVES slices added in slice order (the caller's barrier has made them complete)
__device__ __forceinline__ void pb_rows_sum(const float* s_dot, int rows, int tid, int threads,
                                            float* __restrict__ rowdot_b, int r0, int trows, int n) {
  for (int i = tid; i < trows; i += threads) {
    if (r0 + i < n) {
      float t = 0.f;
#pragma unroll
      for (int j = 0; j < PB_WAVES; ++j) t += s_dot[j * rows + i];
      rowdot_b[r0 + i] = t;
    }
  }
}

// Staging of one K step of the factor's rows r0 .. r0 + 16 MT - 1 into the (hi, mid) planes at `dst` ([2 planes]
// [MT * 16 rows][PB_ROWB]): item = (row, k octet).  load() issues the global loads only -- the callers put it BEFORE
// the MFMAs of the current step and store() (the split and the LDS writes) after them, so the L2 round trip hides under
// the matrix work.  Offsets are computed once per item; a K step only adds a uniform base.  Every address is clamped
// into the matrix (rows >= n to row n - 1, the end of the last row to the last 16 / 4 bytes) and what was clamped is
// zeroed in store().
// VEC4: n % 4 == 0 and a 16-byte aligned factor, every load is 16 bytes wide; otherwise 4-byte loads (the rows of the
// factor are not aligned), same values.
// SELECT: how the clamped values are zeroed.  true: a select per element.  false: a multiply by 0 / 1 per 16 bytes,
// applied in the last K step / for the padded rows -- the form the direct kernel was measured and profiled with.  The
// two give the same planes for a finite factor (x * 1 = x; 0 and -0 split into planes whose products add nothing to an
// accumulator) and differ for a non-finite one (inf * 0), so they are kept apart and not unified.
template <int MT, bool VEC4, bool SELECT>
struct PbStageA {
  static constexpr int ITEMS = (MT * 16 * 4 + PB_THREADS - 1) / PB_THREADS;     // items per thread and K step
  float v[ITEMS][8];
  unsigned off[ITEMS];
  unsigned a_last;

  __device__ __forceinline__ void init(int tid, int r0, int n) {
    a_last = (unsigned)n * (unsigned)n - (VEC4 ? 4u : 1u);
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
      const int item = tid + PB_THREADS * it;
      const int row = r0 + (item >> 2), oct = item & 3;
      off[it] = (unsigned)(row < n ? row : n - 1) * (unsigned)n + (unsigned)(oct * 8);
    }
  }
  __device__ __forceinline__ void load(const float* __restrict__ A, int ks) {
    const unsigned kbase = (unsigned)ks * 32u;
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
      const unsigned o0 = off[it] + kbase;
      if constexpr (VEC4) {
        const unsigned o1 = o0 + 4u;
        const float4 v0 = *reinterpret_cast<const float4*>(A + (o0 < a_last ? o0 : a_last));
        const float4 v1 = *reinterpret_cast<const float4*>(A + (o1 < a_last ? o1 : a_last));
        v[it][0] = v0.x; v[it][1] = v0.y; v[it][2] = v0.z; v[it][3] = v0.w;
        v[it][4] = v1.x; v[it][5] = v1.y; v[it][6] = v1.z; v[it][7] = v1.w;
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const unsigned oj = o0 + (unsigned)j;
          v[it][j] = A[oj < a_last ? oj : a_last];
        }
      }
    }
  }
  __device__ __forceinline__ void store(unsigned char* dst, int tid, int r0, int n, int ks) const {
    constexpr int PLANE = MT * 16 * PB_ROWB;
    const bool tail = (ks + 1) * 32 > n;                   // uniform
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
      const int item = tid + PB_THREADS * it;
      const int row = item >> 2, oct = item & 3;
      if (item < MT * 16 * 4) {
        const int k0 = ks * 32 + oct * 8;
        const bool rok = r0 + row < n;
        float x[8];
        if constexpr (SELECT) {
#pragma unroll
          for (int j = 0; j < 8; ++j) x[j] = (rok && k0 + j < n) ? v[it][j] : 0.f;
        } else {
          const float m0 = (rok && (!tail || k0 + 4 <= n)) ? 1.f : 0.f;
          const float m1 = (rok && (!tail || k0 + 8 <= n)) ? 1.f : 0.f;
#pragma unroll
          for (int j = 0; j < 8; ++j) x[j] = v[it][j] * (j < 4 ? m0 : m1);
        }
        uint4 hi, mid;
        pb_split2(x[0], x[1], hi.x, mid.x); pb_split2(x[2], x[3], hi.y, mid.y);
        pb_split2(x[4], x[5], hi.z, mid.z); pb_split2(x[6], x[7], hi.w, mid.w);
        const unsigned lo = (unsigned)row * PB_ROWB + (unsigned)oct * 16;
        *reinterpret_cast<uint4*>(dst + lo) = hi;
        *reinterpret_cast<uint4*>(dst + PLANE + lo) = mid;
      }
    }
  }
};

// The W tile of a K step ([32 k rows][96 columns from c0 on] fp32, 12 KiB) goes global -> registers (16-byte loads, 384
// contiguous bytes per row: two per thread) -> bf16 (hi, mid) planes in LDS, row-major with the k rows PB_BPITCH bytes
// apart; a wave's B fragment comes out of the transposing read (pb_read_b_tr).  (The direct kernel fetches the fragment
// with eight 4-byte loads per lane, 64-byte segments: 2.2 TB/s of such requests was all the 1.08 ms it took.)
// The resident kernel stages its own, 128 columns wide and PBR_PF steps ahead (wload / wstore there).
struct PbStageW {
  float4 v[2];

  __device__ __forceinline__ void load(const float* __restrict__ W, int tid, int ks, int c0, int n, int d) {
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int item = tid + PB_THREADS * it;              // 768 items = 32 rows x 24 quads
      const int row = item / 24, q = item - row * 24;
      const int kr = ks * 32 + row, cc = c0 + 4 * q;
      const bool ok = kr < n && cc < d;
      v[it] = *reinterpret_cast<const float4*>(W + (size_t)(ok ? kr : 0) * d + (ok ? cc : 0));
      if (!ok) v[it] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  __device__ __forceinline__ void store(unsigned char* bbuf, int tid) const {
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int item = tid + PB_THREADS * it;
      const int row = item / 24, q = item - row * 24;
      uint2 hi, mid;
      pb_split2(v[it].x, v[it].y, hi.x, mid.x); pb_split2(v[it].z, v[it].w, hi.y, mid.y);
      const unsigned lo = (unsigned)row * PB_BPITCH + (unsigned)q * 8;
      *reinterpret_cast<uint2*>(bbuf + lo) = hi;
      *reinterpret_cast<uint2*>(bbuf + 32 * PB_BPITCH + lo) = mid;
    }
  }
};

// B fragment of a wave out of a staged W tile: tr_cons of basd_frag.h on the hi and the mid plane, on a byte pitch.
// Lane holds column 16 wave + li, k rows 8 g4 + 0..7; li = lane & 15 and g4 = lane >> 4 are the caller's (a helper that
// derives them from the thread id again reorders the code around it).
__device__ __forceinline__ void pb_read_b_tr(const unsigned char* tile, int pitch, int plane, int li, int g4, int wave,
                                             bf16x8& bh, bf16x8& bm) {
  const int qq = li >> 2, pp = li & 3;
  const unsigned char* b0 = tile + (size_t)(g4 * 8 + qq) * pitch + (size_t)(wave * 16 + 4 * pp) * 2;
  const v4s h0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)b0);
  const v4s h1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)(b0 + 4 * pitch));
  const v4s m0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)(b0 + plane));
  const v4s m1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)(b0 + plane + 4 * pitch));
  bh = (bf16x8){h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
  bm = (bf16x8){m0[0], m0[1], m0[2], m0[3], m1[0], m1[1], m1[2], m1[3]};
}

// One K step of a strip: A fragments (ap = this lane's 16 bytes of m tile 0 in the hi plane; the mid plane `plane`
// bytes, m tile i `i * tile` bytes further) in two batches of (MT + 1) / 2 tiles.  All 16-byte fragment reads of a batch
// are issued together (one exposed LDS latency per batch; a fence per tile pair exposed it MT / 2 times per K step:
// 4.8 k cycles per step measured with in-kernel stamps against 0.6 k of matrix work), the fence between the batches
// keeps the scheduler from hoisting the second batch on top of the first (registers).
template <int MT>
__device__ __forceinline__ void pb_mfma_step(const unsigned char* ap, int plane, int tile, const bf16x8& bh,
                                             const bf16x8& bm, f32x4 (&acc)[MT]) {
  constexpr int HB = (MT + 1) / 2;
#pragma unroll
  for (int hb = 0; hb < 2; ++hb) {
    bf16x8 fh[HB], fm[HB];
#pragma unroll
    for (int j = 0; j < HB; ++j) {
      const int i = hb * HB + j < MT ? hb * HB + j : MT - 1;
      fh[j] = *reinterpret_cast<const bf16x8*>(ap + (size_t)i * tile);
      fm[j] = *reinterpret_cast<const bf16x8*>(ap + plane + (size_t)i * tile);
    }
#pragma unroll
    for (int j = 0; j < HB; ++j) {
      const int i = hb * HB + j;
      if (i < MT) {
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fh[j], bh, acc[i], 0, 0, 0);
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fh[j], bm, acc[i], 0, 0, 0);
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fm[j], bh, acc[i], 0, 0, 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// ---- epilogue.  acc[i][r] = P at row r0 + 16 i + 4 (lane >> 4) + r, column 16 s0 + (lane & 15): one value per lane
// and row -- consumed in that layout the residual costs a 4-byte load, a 4-byte store and a 16-lane reduction per
// element group (measured: 0.8 of 1.2 ms).  Instead the wave parks one 16 x 16 tile at a time in its own 1 KiB of
// LDS and reads it back row-wise: 16 bytes per lane, 64 contiguous bytes per row segment for the W load and the
// store, a 4-lane reduction per row.
// One parked tile: residual of the row chunk against wv (the fp32 W of the same 4 columns), scaled by cr and stored at
// O + off when ok; returns the chunk's <R, W>, summed over the four lanes of the row (0 when not ok).
template <typename TO>
__device__ __forceinline__ float pb_epilogue_tile(const f32x4& acc, float* park, int lane, const float4& wv, float cr,
                                                  bool ok, TO* __restrict__ O, unsigned off) {
  const int col = lane & 15, g4 = lane >> 4, prow = lane >> 2, pch = lane & 3;
#pragma unroll
  for (int r = 0; r < 4; ++r) park[(g4 * 4 + r) * 16 + col] = acc[r];
  // wave-private tile: the wave's own LDS writes precede its reads (in order), no barrier
  const float4 pv = *reinterpret_cast<const float4*>(park + prow * 16 + pch * 4);
  const float4 rv = make_float4(wv.x - pv.x, wv.y - pv.y, wv.z - pv.z, wv.w - pv.w);
  float dot = ok ? fmaf(rv.x, wv.x, fmaf(rv.y, wv.y, fmaf(rv.z, wv.z, rv.w * wv.w))) : 0.f;
  if (ok) {
    if constexpr (sizeof(TO) == 4) {
      *reinterpret_cast<float4*>(O + off) = make_float4(cr * rv.x, cr * rv.y, cr * rv.z, cr * rv.w);
    } else {
      uint2 o;
      o.x = pack_bf16_bits(cr * rv.x, cr * rv.y);
      o.y = pack_bf16_bits(cr * rv.z, cr * rv.w);
      *reinterpret_cast<uint2*>(O + off) = o;
    }
  }
  dot += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(dot), 0xB1, 0xF, 0xF, true));     // quad_perm 1,0,3,2
  dot += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(dot), 0x4E, 0xF, 0xF, true));     // quad_perm 2,3,0,1
  return dot;
}

// The MT tiles of strip s0 (`has`: the strip exists), rows r0 .. r0 + trows - 1 of the matrix (trows <= 16 MT; rows of
// other row tiles and rows >= n are never stored), in two batches: the W loads of a batch are in flight together.
// What differs between the kernels stays with the caller: sink(i, lrow, dot) takes the row dot of tile i, local row
// lrow (every lane of the row's quad holds it).
template <int MT, typename TO, typename Sink>
__device__ __forceinline__ void pb_epilogue_strip(const f32x4 (&acc)[MT], float* park, int lane, bool has, int s0,
                                                  int r0, int trows, int n, int d, const float* __restrict__ W,
                                                  TO* __restrict__ O, const float* s_c, Sink&& sink) {
  const int prow = lane >> 2, pch = lane & 3;              // row-wise walk: 16 rows x 4 chunks of 4 columns
  const int pcol = s0 * 16 + pch * 4;
  constexpr int H0 = (MT + 1) / 2;
#pragma unroll
  for (int hb = 0; hb < 2; ++hb) {
    float4 wq[H0];
#pragma unroll
    for (int j = 0; j < H0; ++j) {
      const int lrow = (hb * H0 + j) * 16 + prow, row = r0 + lrow;
      const bool ok = has && lrow < trows && row < n;
      wq[j] = *reinterpret_cast<const float4*>(W + (unsigned)(ok ? row : 0) * (unsigned)d + (unsigned)(ok ? pcol : 0));
    }
#pragma unroll
    for (int j = 0; j < H0; ++j) {
      const int i = hb * H0 + j;
      if (i < MT) {
        const int lrow = i * 16 + prow, row = r0 + lrow;
        const bool ok = has && lrow < trows && row < n;
        const unsigned off = (unsigned)(ok ? row : 0) * (unsigned)d + (unsigned)(ok ? pcol : 0);      // 32-bit: n d < 2^31
        sink(i, lrow, pb_epilogue_tile<TO>(acc[i], park, lane, wq[j], s_c[lrow], ok, O, off));
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// ---- the direct form: up to three m tiles (n <= 48) ---------------------------------------------------------------------
// W straight from global memory as the B fragment, the factor double buffered; LDS: 4 planes of a K step + the row dots
// and scales, the parked epilogue tiles (6 KiB) alias the operand buffers, which are idle then (MT >= 2: they fit).
template <int MT>
constexpr size_t pb_direct_lds() { return (size_t)4 * MT * 16 * PB_ROWB + (size_t)MT * 16 * 4 * (PB_WAVES + 1); }

template <int MT, typename TO>      // MT = m tiles (16 rows each) >= ceil(n / 16)
__global__ __launch_bounds__(PB_THREADS) __attribute__((amdgpu_waves_per_eu(3, 3))) void procrustes_bwd_side_kernel(
    const float* __restrict__ fac, const float* __restrict__ w, const float* __restrict__ a,
    const float* __restrict__ gl, int n, int d, TO* __restrict__ out, float* __restrict__ rowdot) {
  extern __shared__ __align__(16) unsigned char smem[];
  constexpr int PLANE = MT * 16 * PB_ROWB;                 // one bf16 plane of one K step
  unsigned char* abuf = smem;                              // [2 buffers][2 planes][MT * 16 rows][PB_ROWB]
  float* s_dotw = reinterpret_cast<float*>(smem + 4 * PLANE);  // [waves][MT * 16] row dots, one slice per wave
  float* s_c = s_dotw + PB_WAVES * MT * 16;                    // [MT * 16] row scales 2 gl sqrt(a)
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* A = fac + (size_t)b * n * n;
  const float* W = w + (size_t)b * n * d;
  TO* O = out + (size_t)b * n * d;
  const int ksteps = (n + 31) >> 5;
  const int strips = d >> 4;
  const float c2 = 2.f * gl[b];
  pb_rows_init(s_c, s_dotw, MT * 16, tid, PB_THREADS, a + (size_t)b * n, c2, 0, MT * 16, n);
  PbStageA<MT, true, false> sa;                            // n % 4 == 0, 16-byte aligned factor (checked by the C entry)
  sa.init(tid, 0, n);

  for (int g0 = 0; g0 < strips; g0 += PB_WAVES) {          // column groups of PB_WAVES strips (96 columns), one per wave
    const int s0 = g0 + wave;
    const bool has = s0 < strips;
    const int col = (lane & 15);
    const unsigned cs = has ? (unsigned)(s0 * 16 + col) : (unsigned)col;                // 32-bit offsets: n d < 2^31
    // B fragment of one K step: lane holds column 16 s0 + (lane & 15), rows k0 + 8 (lane >> 4) + 0..7 (clamped, select)
    float bn[8];
    const unsigned b_off = (unsigned)((lane >> 4) * 8) * (unsigned)d + cs;    // row 8 (lane >> 4) of a K step, this column
    const unsigned b_last = (unsigned)(n - 1) * (unsigned)d + cs;             // same column, last row
    auto fetch_b = [&](int ks) {
      const unsigned o = b_off + (unsigned)ks * 32u * (unsigned)d;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const unsigned oj = o + (unsigned)j * (unsigned)d;
        bn[j] = W[oj < b_last ? oj : b_last];
      }
    };
    __syncthreads();                                       // previous group's fragment reads are done
    sa.load(A, 0);
    fetch_b(0);
    sa.store(abuf, tid, 0, n, 0);
    __syncthreads();
    f32x4 acc[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int ks = 0; ks < ksteps; ++ks) {
      const int buf = ks & 1;
      const int kb = ks * 32 + (lane >> 4) * 8;
      bf16x8 bh, bm;
      {
        float x[8];
        if ((ks + 1) * 32 > n) {                           // uniform: the last K step, rows beyond n
#pragma unroll
          for (int j = 0; j < 8; ++j) x[j] = (has && kb + j < n) ? bn[j] : 0.f;
        } else {
          const float keep = has ? 1.f : 0.f;
#pragma unroll
          for (int j = 0; j < 8; ++j) x[j] = bn[j] * keep;
        }
        uint4 hi, mid;
        pb_split2(x[0], x[1], hi.x, mid.x); pb_split2(x[2], x[3], hi.y, mid.y);
        pb_split2(x[4], x[5], hi.z, mid.z); pb_split2(x[6], x[7], hi.w, mid.w);
        bh = __builtin_bit_cast(bf16x8, hi);
        bm = __builtin_bit_cast(bf16x8, mid);
      }
      const bool more = ks + 1 < ksteps;
      if (more) {                                          // next step's operands: loads only, consumed after the MFMAs
        fetch_b(ks + 1);
        sa.load(A, ks + 1);
      }
      pb_mfma_step<MT>(abuf + (size_t)buf * 2 * PLANE + (size_t)(lane & 15) * PB_ROWB + (lane >> 4) * 16, PLANE,
                       16 * PB_ROWB, bh, bm, acc);
      if (more) sa.store(abuf + (size_t)(buf ^ 1) * 2 * PLANE, tid, 0, n, ks + 1);
      __syncthreads();                                     // buffer `buf` may be overwritten, `buf ^ 1` is complete
    }
    pb_epilogue_strip<MT, TO>(acc, reinterpret_cast<float*>(abuf) + wave * 256, lane, has, s0, 0, MT * 16, n, d, W, O, s_c,
                              [&](int, int lrow, float dot) {
                                if ((lane & 3) == 0) s_dotw[wave * (MT * 16) + lrow] += c2 * dot;
                              });
  }
  __syncthreads();
  pb_rows_sum(s_dotw, MT * 16, tid, PB_THREADS, rowdot + (size_t)b * n, 0, MT * 16, n);
}

// ---- the tiled form: W staged through LDS; a workgroup owns a row tile of MT m tiles of one matrix --------------------
// The direct kernel with the B operand (W) staged through LDS -- see PbStageW.  One operand buffer each, two barriers per
// K step.  Measured (1024 x [196, 196] x [196, 768], a whole matrix per workgroup): 1.04 vs 1.15 ms, the c4 shape 0.91
// vs 1.01 -- the 4-byte fragment loads were a tenth of the time, not the bulk of it.  What is left is traffic: per
// matrix W is read twice (operand + residual; 300 MB of W are in flight across the chip, the second read is not an L2
// hit), the [n, n] factor once per 96-column group (8 x 154 KB), the gradient written once -- ~3 GB per launch at 3 - 4
// TB/s.  Fewer, wider groups (12 waves, one workgroup per CU) would halve the factor's re-reads; keeping it resident
// needs 154 KiB of bf16 planes: the resident kernel below, which took over from five m tiles on.
// The kernel serves two dispatch ranges:
// * WHOLE: one row tile is the whole matrix (tiles = 1, grid = batch), MT = 4 | 8: n = 49 .. 64, and up to 128 rows with
//   fewer than 112 columns (launch_side) -- "the staged kernel" of the measurements in this file.  r0 = 0 is known to
//   the compiler and the factor is masked in the direct kernel's form (PbStageA, SELECT = false): with r0 and the
//   selects of the row-tiled form these shapes measured 1.4 - 3.9 % slower than before (1024 x 64 x 768: 0.1369 ->
//   0.1388 ms, 1024 x 128 x 96: 0.0408 -> 0.0424), same bits;
// * 257 <= n <= 1024, and every n % 4 != 0: row tiles of PBL_RT = 128 rows (MT = 8: 8 accumulator tiles per strip; a
//   whole matrix would be 144 accumulator registers per lane at 576 rows), grid = batch x ceil(n / 128), the row tiles
//   of a matrix adjacent in the grid so that they run together and share W in the caches (at batch-major order 256
//   matrices x 1.8 MB of W would be re-read from HBM once per row tile).  The K loop runs over all n rows of W.
// A row tile sees all d columns, so its row dots are complete inside the workgroup: each wave adds its column groups
// in order into its own slice, the slices are added in wave order -- no atomics, bitwise reproducible.  Rows >= n of
// the last tile and the K tail (n % 32) are zeroed on the way into LDS and never stored.
// VEC4 = false (n % 4 != 0: the rows of the factor, and every matrix of the batch but the first, are not 16-byte
// aligned -- 729 tokens of a /14 grid at 384 px) loads the factor with 4-byte loads; W, the gradient and the LDS
// traffic are the same (d % 16 == 0 keeps their rows aligned).
// LDS: 2 A planes + 2 W planes + 7 x 64 MT bytes of row dots / scales (MT = 8: 37376 bytes = 2 x 10240 + 2 x 6656 + 7 x
// 512; two workgroups per CU); the parked epilogue tiles (6 KiB) alias the A planes, which are idle then.
// Compiler's resource report (hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; fp32 and bf16 output
// alike; LDS is dynamic):
//   direct <2>               VGPRs 110  AGPRs 0  scratch 0 bytes/lane  occupancy 3 waves/SIMD
//   direct <4>               VGPRs 122  AGPRs 0  scratch 0 bytes/lane  occupancy 3 waves/SIMD
//   tiled  <4, WHOLE>            VGPRs 108  AGPRs 0  scratch 0 bytes/lane  occupancy 3 waves/SIMD
//   tiled  <8, WHOLE>            VGPRs 158  AGPRs 0  scratch 0 bytes/lane  occupancy 3 waves/SIMD
//   tiled  <8, row tiles, VEC4>  VGPRs 160  AGPRs 0  scratch 0 bytes/lane  occupancy 3 waves/SIMD
//   tiled  <8, row tiles, 4-byte loads>  VGPRs 162  AGPRs 0  scratch 0 bytes/lane  occupancy 3 waves/SIMD
// (While the whole-matrix and the row-tiled form were two kernels: 106 / 158 for the former at MT = 4 / 8, 156 / 164 for
// the latter.  Same bits and, against that build in one process, times inside its own bracket-to-bracket band:
// profiles/procrustes_bwd_one_copy_bits.txt, profiles/procrustes_bwd_one_copy_ab.txt.)
constexpr int PBL_MT = 8;                   // m tiles (16 rows each) of a row tile of the long form
constexpr int PBL_RT = 16 * PBL_MT;         // rows of a row tile

template <int MT>
constexpr size_t pb_tiled_lds() {
  return (size_t)2 * MT * 16 * PB_ROWB + (size_t)2 * 32 * PB_BPITCH + (size_t)MT * 16 * 4 * (PB_WAVES + 1);
}

template <int MT, typename TO, bool VEC4, bool WHOLE>
__global__ __launch_bounds__(PB_THREADS) __attribute__((amdgpu_waves_per_eu(3, 3))) void procrustes_bwd_side_tiled_kernel(
    const float* __restrict__ fac, const float* __restrict__ w, const float* __restrict__ a,
    const float* __restrict__ gl, int n, int d, int tiles, TO* __restrict__ out, float* __restrict__ rowdot) {
  extern __shared__ __align__(16) unsigned char smem[];
  constexpr int PLANE = MT * 16 * PB_ROWB;                 // one bf16 plane of one K step
  unsigned char* abuf = smem;                              // [2 planes][MT * 16 rows][PB_ROWB]   (ONE buffer)
  unsigned char* bbuf = smem + 2 * PLANE;                  // [2 planes][32 k rows][PB_BPITCH]: the W tile of a K step
  float* s_dotw = reinterpret_cast<float*>(smem + 2 * PLANE + 2 * 32 * PB_BPITCH);  // [waves][MT * 16] row dots
  float* s_c = s_dotw + PB_WAVES * MT * 16;                // [MT * 16] row scales 2 gl sqrt(a)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = WHOLE ? (int)blockIdx.x : (int)blockIdx.x / tiles;
  const int r0 = WHOLE ? 0 : ((int)blockIdx.x - b * tiles) * (MT * 16);   // first row of this tile; r0 < n
  const float* A = fac + (size_t)b * n * n;
  const float* W = w + (size_t)b * n * d;
  TO* O = out + (size_t)b * n * d;
  const int ksteps = (n + 31) >> 5;
  const int strips = d >> 4;
  const float c2 = 2.f * gl[b];
  pb_rows_init(s_c, s_dotw, MT * 16, tid, PB_THREADS, a + (size_t)b * n, c2, r0, MT * 16, n);
  PbStageA<MT, VEC4, !WHOLE> sa;
  PbStageW sb;
  sa.init(tid, r0, n);

  for (int g0 = 0; g0 < strips; g0 += PB_WAVES) {          // column groups of PB_WAVES strips (96 columns), one per wave
    const int s0 = g0 + wave;
    const int c0 = g0 * 16;                                // first column of the group
    __syncthreads();                                       // previous group's fragment / parked-tile reads are done
    sa.load(A, 0);
    sb.load(W, tid, 0, c0, n, d);
    sa.store(abuf, tid, r0, n, 0);
    sb.store(bbuf, tid);
    __syncthreads();
    f32x4 acc[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int ks = 0; ks < ksteps; ++ks) {
      const bool more = ks + 1 < ksteps;
      if (more) {                                          // next step's operands: loads only, stored after the MFMAs
        sb.load(W, tid, ks + 1, c0, n, d);
        sa.load(A, ks + 1);
      }
      bf16x8 bh, bm;
      pb_read_b_tr(bbuf, PB_BPITCH, 32 * PB_BPITCH, lane & 15, lane >> 4, wave, bh, bm);
      pb_mfma_step<MT>(abuf + (size_t)(lane & 15) * PB_ROWB + (lane >> 4) * 16, PLANE, 16 * PB_ROWB, bh, bm, acc);
      __syncthreads();                                     // every wave has read the operands of step ks
      if (more) { sa.store(abuf, tid, r0, n, ks + 1); sb.store(bbuf, tid); }
      __syncthreads();                                     // step ks + 1 is complete
    }
    pb_epilogue_strip<MT, TO>(acc, reinterpret_cast<float*>(abuf) + wave * 256, lane, s0 < strips, s0, r0, MT * 16, n, d,
                              W, O, s_c, [&](int, int lrow, float dot) {
                                if ((lane & 3) == 0) s_dotw[wave * (MT * 16) + lrow] += c2 * dot;
                              });
  }
  __syncthreads();
  pb_rows_sum(s_dotw, MT * 16, tid, PB_THREADS, rowdot + (size_t)b * n, r0, MT * 16, n);
}

// g_a = (dot_s + dot_t) / (2 a)
__global__ __launch_bounds__(256) void procrustes_ga_kernel(const float* __restrict__ dot_s, const float* __restrict__ dot_t,
                                                           const float* __restrict__ a, int64_t total,
                                                           float* __restrict__ g_a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < total) g_a[i] = (dot_s[i] + dot_t[i]) / (2.0f * a[i]);
}

// ---- the resident form: 5 <= ceil(n / 16) <= 16 m tiles ------------------------------------------------------------
// The tiled kernel above (one row tile: "the staged kernel") re-reads, re-splits and re-stores the [n, n] factor once per 96-column group (8 times at
// d = 768) and puts two __syncthreads() -- each of which also drains the wave's outstanding global loads -- into every
// K step, so every step exposes one memory round trip.  Here the factor is loaded, masked and split ONCE per workgroup
// and its (hi, mid) planes stay in LDS for all column groups; what moves in the loop is W alone.
// * A workgroup owns a ROW TILE of one matrix, MT <= 8 m tiles (the accumulator budget of the tiled kernel),
//   and runs over all d columns: its row dots are complete inside the workgroup (no atomics).  Tiles per matrix: the
//   fewest that fit the 160 KiB of LDS -- one up to 128 rows, two up to 224 (196 rows: 7 + 6 m tiles), three above.
//   A short tile runs the MFMAs of MT m tiles on rows zeroed in LDS (1 / 14 of the matrix work at 196 rows).
// * Resident planes: row-major, [2 planes][16 MT rows][pbr_apitch(ksteps)] bytes: 64 bytes per K step and 16 or 48
//   bytes of padding -- the pitch for which the 16-lane groups of the 16-byte fragment reads meet fewest banks twice.
// * Grid: the tiles of matrix b sit 8 blocks apart (block = 8 T (b / 8) + 8 t + b % 8).  Workgroups go to the 8 XCDs
//   round-robin, so the tiles of a matrix, which read the same W, run at the same time on the same L2.  This is the
//   mapping that was measured; adjacent tiles (block = T b + t) land on different L2s and were not timed.
// * 8 waves (two per SIMD, 256 registers each), one 16-column strip each: 128-column groups.  The (group, K step)
//   pairs form ONE flat sequence of steps.  The W tile of a step ([32 k rows][128 columns] fp32: two 16-byte loads
//   per thread) is loaded PBR_PF = 4 steps ahead into registers -- across group boundaries, so the epilogue of a group
//   runs with the next group's tiles in flight --, split and stored into the other of two LDS buffers one step ahead.
//   One barrier per step, and it orders LDS traffic only (lds_barrier): global loads stay in flight across it.
// * Same arithmetic as the kernels above: pb_mfma_step and pb_epilogue_strip are the code they run, so `out` has the
//   same bits.  Row dots: strip s is added to slot s % 6 in LDS, strips ascending, and the six slots are added in order
//   (pb_rows_sum) -- the order of the kernels above, whose wave s % 6 owns strip s; so `rowdot` has the same bits too,
//   and the step computes what it computed.  No atomics (see `pend` in the kernel).
// * Bounds: rows >= n and the rows of the other tiles are clamped to row n - 1 on the load and zeroed by a select, the
//   K tail likewise (every load is clamped to the last 16 bytes of the matrix's own factor); W rows >= n and columns
//   >= d of a ragged last group read element 0 of the matrix and are zeroed; nothing is stored outside [n, d].
// Rejected: (b) hi plane resident, mid plane streamed -- it keeps a whole matrix per workgroup (13 accumulator tiles,
// 168-register budget gone) but puts half of the factor's traffic and its split back into every column group; not built
// once (a) fitted with no scratch.  Two strips per wave (4 waves): halves the fragment reads per MFMA, one wave per
// SIMD; not built: LDS reads (0.07 ms per launch by the rates of the LDS table) are not what bounds this kernel.
constexpr int PBR_WAVES = 8;
constexpr int PBR_THREADS = 64 * PBR_WAVES;
constexpr int PBR_COLS = 16 * PBR_WAVES;     // columns of a group
constexpr int PBR_BPITCH = 304;              // bytes between the k rows of a staged W plane (128 bf16 = 256 + 48 pad)
constexpr int PBR_PF = 4;                    // W tiles in flight (steps between a tile's global load and its LDS store)

__host__ __device__ inline int pbr_apitch(int ksteps) { return ksteps * 64 + ((ksteps & 3) == 3 ? 48 : 16); }
// LDS of a workgroup with m m tiles: resident factor planes + two W buffers + parked tiles + row scales and row-dot slots
inline size_t pbr_lds(int m, int ksteps) {
  return (size_t)2 * m * 16 * pbr_apitch(ksteps) + (size_t)4 * 32 * PBR_BPITCH + (size_t)PBR_WAVES * 1024 +
         (size_t)m * 64 * (1 + PB_WAVES);
}

template <int MT, typename TO>      // MT = m tiles of the longest row tile
__global__ __launch_bounds__(PBR_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void procrustes_bwd_side_resident_kernel(
    const float* __restrict__ fac, const float* __restrict__ w, const float* __restrict__ a,
    const float* __restrict__ gl, int batch, int n, int d, int tiles, TO* __restrict__ out, float* __restrict__ rowdot) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int per = 8 * tiles;
  const int grp = (int)blockIdx.x / per, rem = (int)blockIdx.x - grp * per;
  const int b = grp * 8 + (rem & 7), t = rem >> 3;
  if (b >= batch) return;                                  // the grid is padded to whole groups of 8 matrices
  const int mt = (n + 15) >> 4;
  const int base = mt / tiles, extra = mt - base * tiles;  // the first `extra` tiles hold base + 1 m tiles (= MT)
  const int trows = 16 * (base + (t < extra ? 1 : 0));     // rows of this tile (the last one of the matrix: padded)
  const int r0 = 16 * (t * base + (t < extra ? t : extra));
  const int ksteps = (n + 31) >> 5;
  const int AP = pbr_apitch(ksteps);
  const int APLANE = MT * 16 * AP;
  constexpr int BPLANE = 32 * PBR_BPITCH;
  unsigned char* abuf = smem;                              // [2 planes][MT * 16 rows][AP]: the resident factor slice
  unsigned char* bbuf = smem + 2 * APLANE;                 // [2 buffers][2 planes][32 k rows][PBR_BPITCH]: W tiles
  float* s_park = reinterpret_cast<float*>(bbuf + 4 * BPLANE);   // [waves][16 rows][16 columns] epilogue tiles
  float* s_c = s_park + PBR_WAVES * 256;                   // [MT * 16] row scales 2 gl sqrt(a)
  float* s_slot = s_c + MT * 16;                           // [PB_WAVES slots][MT * 16] row dots, see the epilogue
  const float* A = fac + (size_t)b * n * n;
  const float* W = w + (size_t)b * n * d;
  TO* O = out + (size_t)b * n * d;
  const int strips = d >> 4;
  const int total = ((d + PBR_COLS - 1) / PBR_COLS) * ksteps;    // steps = (column group, K step), group-major
  const float c2 = 2.f * gl[b];

  // the W tile of a step: global -> registers (16-byte loads, 512 contiguous bytes per k row) -> (hi, mid) planes
  // The loads are unconditional and only clamp their address (W rows >= n and the columns >= d of a ragged last group
  // read element 0 of the matrix); what was clamped is zeroed by a select when the tile is stored.  A select or a
  // branch right behind the load would make the wave wait for it there.
  float4 wr[PBR_PF][2];
  auto wload = [&](float4 (&r)[2], int g, int ks) {
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int item = tid + PBR_THREADS * it;             // 1024 items = 32 rows x 32 quads
      const int kr = ks * 32 + (item >> 5), cc = g * PBR_COLS + 4 * (item & 31);
      const bool ok = kr < n && cc < d;
      r[it] = *reinterpret_cast<const float4*>(W + (size_t)(ok ? kr : 0) * d + (ok ? cc : 0));
    }
  };
  auto wstore = [&](const float4 (&r)[2], int buf, int g, int ks) {
    unsigned char* dst = bbuf + (size_t)buf * 2 * BPLANE;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int item = tid + PBR_THREADS * it;
      const int kr = ks * 32 + (item >> 5), cc = g * PBR_COLS + 4 * (item & 31);
      const bool ok = kr < n && cc < d;
      const float4 v = ok ? r[it] : make_float4(0.f, 0.f, 0.f, 0.f);
      uint2 hi, mid;
      pb_split2(v.x, v.y, hi.x, mid.x); pb_split2(v.z, v.w, hi.y, mid.y);
      const unsigned lo = (unsigned)(item >> 5) * PBR_BPITCH + (unsigned)(item & 31) * 8;
      *reinterpret_cast<uint2*>(dst + lo) = hi;
      *reinterpret_cast<uint2*>(dst + BPLANE + lo) = mid;
    }
  };
  // The step sequence is padded to a multiple of PF with steps that repeat the last tile: no branch around a load or
  // a barrier in the loop.  A padding step's products land in accumulators whose epilogue, if it comes at all (fewer
  // K steps than PF), belongs to a column group past d and stores nothing.
  const int padded = (total + PBR_PF - 1) / PBR_PF * PBR_PF;
  int lt = 0, lg = 0, lks = 0;                             // the next step to load, as index and as (group, K step)
  auto wnext = [&](float4 (&r)[2]) {
    wload(r, lg, lks);
    if (++lt < total && ++lks == ksteps) { lks = 0; ++lg; }
  };
#pragma unroll
  for (int u = 0; u < PBR_PF; ++u) wnext(wr[u]);           // steps 0 .. PF - 1 are in flight under the factor's staging

  pb_rows_init(s_c, s_slot, MT * 16, tid, PBR_THREADS, a + (size_t)b * n, c2, r0, trows, n);

  // ---- the factor slice, once: item = (row of the tile, k octet of 32 slots), two 16-byte loads each, four items in
  // flight per thread.  n % 4 == 0: a 16-byte load is inside the row or beyond it as a whole.
  {
    const int octs = ksteps * 4;
    const unsigned a_last = (unsigned)n * (unsigned)n - 4u;
    for (int it0 = 0; it0 < MT * 16 * 32; it0 += 4 * PBR_THREADS) {
      float4 v[4][2];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int item = it0 + j * PBR_THREADS + tid;
        const int rg = r0 + (item >> 5);
        const unsigned o0 = (unsigned)(rg < n ? rg : n - 1) * (unsigned)n + (unsigned)((item & 31) * 8), o1 = o0 + 4u;
        v[j][0] = *reinterpret_cast<const float4*>(A + (o0 < a_last ? o0 : a_last));
        v[j][1] = *reinterpret_cast<const float4*>(A + (o1 < a_last ? o1 : a_last));
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int item = it0 + j * PBR_THREADS + tid;
        const int row = item >> 5, oct = item & 31;
        if (row < MT * 16 && oct < octs) {
          const bool rok = row < trows && r0 + row < n;
          const bool k0 = rok && oct * 8 + 4 <= n, k1 = rok && oct * 8 + 8 <= n;
          const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
          const float4 v0 = k0 ? v[j][0] : z, v1 = k1 ? v[j][1] : z;
          uint4 hi, mid;
          pb_split2(v0.x, v0.y, hi.x, mid.x); pb_split2(v0.z, v0.w, hi.y, mid.y);
          pb_split2(v1.x, v1.y, hi.z, mid.z); pb_split2(v1.z, v1.w, hi.w, mid.w);
          const unsigned lo = (unsigned)row * (unsigned)AP + (unsigned)oct * 16;
          *reinterpret_cast<uint4*>(abuf + lo) = hi;
          *reinterpret_cast<uint4*>(abuf + APLANE + lo) = mid;
        }
      }
    }
  }
  wstore(wr[0], 0, 0, 0);                                  // step 0; visible after the barrier of step 0
  wnext(wr[0]);                                            // step PF

  f32x4 acc[MT];
  const int col = lane & 15, g4 = lane >> 4;
  const int prow = lane >> 2, pch = lane & 3;              // the epilogue's row-wise walk (row of a tile, 4-column chunk)
  // Row dots in the order of the staged kernel, whose wave s % 6 adds strip s to its own slice, strips ascending, and
  // whose slices are added in wave order: strip s goes to slot s % 6 here as well.  The strips of waves 0 .. 5 of a
  // group fall into six different slots; those of waves 6 and 7 share a slot with waves 0 and 1 and come after them,
  // so these two waves keep their dots (pend) and add them behind the next barrier.  At least two barriers separate
  // the epilogues of two groups (ksteps >= 3 from 65 rows on), so every slot is added to in strip order.
  float pend[MT];
  int pend_slot = -1;                                      // wave-uniform: >= 0 while dots are waiting
#pragma unroll
  for (int i = 0; i < MT; ++i) { acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f}; pend[i] = 0.f; }
  auto flush = [&]() {
    if (pend_slot >= 0) {
      if (pch == 0) {
#pragma unroll
        for (int i = 0; i < MT; ++i) s_slot[pend_slot * MT * 16 + i * 16 + prow] += c2 * pend[i];
      }
      pend_slot = -1;
    }
  };
  float* park = s_park + wave * 256;
  int ks = 0, g = 0;
  for (int t0 = 0; t0 < padded; t0 += PBR_PF) {
#pragma unroll
    for (int u = 0; u < PBR_PF; ++u) {                     // unrolled: step t lives in the register set t % PF
      {
        const int buf = (t0 + u) & 1;
        lds_barrier();                                     // this step's tile is complete, buffer buf ^ 1 has been read
        flush();
        {
          const bool wrap = ks + 1 == ksteps;
          wstore(wr[(u + 1) % PBR_PF], buf ^ 1, wrap ? g + 1 : g, wrap ? 0 : ks + 1);   // the next step, loaded PF steps ago
          wnext(wr[(u + 1) % PBR_PF]);                     // the step PF after it
        }
        bf16x8 bh, bm;
        pb_read_b_tr(bbuf + (size_t)buf * 2 * BPLANE, PBR_BPITCH, BPLANE, col, g4, wave, bh, bm);
        // A fragments of K step ks out of the resident planes
        pb_mfma_step<MT>(abuf + (size_t)col * AP + (size_t)ks * 64 + g4 * 16, APLANE, 16 * AP, bh, bm, acc);
        if (++ks == ksteps) {
          // ---- epilogue of group g (pb_epilogue_strip); the accumulators are zeroed for the next group on the way
          const int s0 = g * PBR_WAVES + wave;
          const bool has = s0 < strips;
          const int slot = s0 % PB_WAVES;
          const bool later = has && wave >= PB_WAVES;      // wave-uniform
          if (later) pend_slot = slot;
          pb_epilogue_strip<MT, TO>(acc, park, lane, has, s0, r0, trows, n, d, W, O, s_c, [&](int i, int lrow, float dot) {
            if (later) pend[i] = dot;
            else if (has && pch == 0) s_slot[slot * MT * 16 + lrow] += c2 * dot;
            acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
          });
          ks = 0;
          ++g;
        }
      }
    }
  }
  // row dots: the slots are added in slot order, as the staged kernel adds its waves' slices
  lds_barrier();
  flush();
  lds_barrier();
  pb_rows_sum(s_slot, MT * 16, tid, PBR_THREADS, rowdot + (size_t)b * n, r0, trows, n);
}

// Compiler's resource report (hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; fp32 and bf16 output
// alike; LDS is dynamic, pbr_lds(): 2 x 16 MT x pitch factor planes + 38912 W tiles + 8192 parked tiles + 64 MT row
// scales + 384 MT row-dot slots):
//   MT = 5   VGPRs 122  AGPRs 0  scratch 0 bytes/lane  occupancy 2 waves/SIMD
//   MT = 6   VGPRs 134  AGPRs 0  scratch 0 bytes/lane  occupancy 2 waves/SIMD
//   MT = 7   VGPRs 140  AGPRs 0  scratch 0 bytes/lane  occupancy 2 waves/SIMD   (196 rows: 161344 bytes of LDS)
//   MT = 8   VGPRs 150  AGPRs 0  scratch 0 bytes/lane  occupancy 2 waves/SIMD
// Measured on one MI355X against the staged kernel of the parent commit, both libraries loaded into one process, the
// same inputs, alternated medians of 4 brackets of 10 launches (ms; the parent's own brackets differ by 0.005 - 0.026,
// 0.061 at 128 rows):
//   batch x n x d       staged   resident
//   1024 x 196 x  768   0.936    0.516      (c2, teacher side; 1.85 GB algorithmic: 3.6 TB/s)
//    512 x 196 x 1024   0.650    0.326      (c4)
//   1024 x 196 x 1280   1.613    0.832      (c5)
//   1024 x 196 x  192   0.257    0.216
//   1024 x  80 x  768   0.255    0.151      (5 m tiles: the dispatch boundary)
//   1024 x 128 x  768   0.354    0.226      (one row tile of 8)
//   1024 x 256 x  768   1.316    0.757      (three row tiles)
//      2 x 100 x  112   0.0153   0.0100
//    300 x  80 x   16   0.0141   0.0161     (slower: stays on the staged kernel, see launch_side)
// (With the row dots kept per wave in registers and added in 8-wave order the c2 shape took 0.493 ms in another session;
// that order changes `rowdot` by 6.6e-8 rel-L2 and with it every later step of a training run.)  `out` and `rowdot` have
// the bits of the staged kernel at these and six smaller shapes, fp32 and bf16.  Up to four m tiles (c1: 64 tokens)
// were not timed and stay on the kernels above.

// one launch; a kernel that asks for more than the default 64 KiB of dynamic LDS has its limit raised once
template <typename... P, typename... Args>
static void launch_pb(void (*kernel)(P...), dim3 grid, int threads, size_t lds, hipStream_t st, Args... args) {
  if (lds > 64 * 1024) allow_full_lds((const void*)kernel);
  hipLaunchKernelGGL(kernel, grid, dim3(threads), lds, st, args...);
}

template <typename TO>
static int launch_side_resident(const float* fac, const float* w, const float* a, const float* gl, int batch, int n,
                                int d, TO* out, float* rowdot, hipStream_t st) {
  const int mt = (n + 15) / 16, ksteps = (n + 31) / 32;
  int tiles = (mt + 7) / 8, m = 0;
  size_t lds = 0;
  for (;; ++tiles) {                                       // the fewest row tiles whose resident planes fit
    m = (mt + tiles - 1) / tiles;
    lds = pbr_lds(m, ksteps);
    if (lds <= 160 * 1024) break;
  }
  const dim3 grid((unsigned)((batch + 7) / 8) * 8u * (unsigned)tiles);
  auto go = [&](auto kernel) { launch_pb(kernel, grid, PBR_THREADS, lds, st, fac, w, a, gl, batch, n, d, tiles, out, rowdot); };
  switch (m) {
    case 5: go(procrustes_bwd_side_resident_kernel<5, TO>); break;
    case 6: go(procrustes_bwd_side_resident_kernel<6, TO>); break;
    case 7: go(procrustes_bwd_side_resident_kernel<7, TO>); break;
    case 8: go(procrustes_bwd_side_resident_kernel<8, TO>); break;
    default: return fail(BASD_ERR_SHAPE, "procrustes_bwd_side: no resident kernel for %d m tiles in %d row tiles", mt, tiles);
  }
  return check_launch("procrustes_bwd (resident residual product)");
}

// n <= 256, n % 4 == 0, a 16-byte aligned factor: one workgroup per matrix, or per row tile of the resident kernel
template <typename TO>
static int launch_side(const float* fac, const float* w, const float* a, const float* gl, int batch, int n, int d,
                       TO* out, float* rowdot, hipStream_t st) {
  const int mt = (n + 15) / 16;
  // resident factor where it was measured faster: from five m tiles on, a single row tile (mt <= 8) only with at least
  // 112 columns (300 x 80 x 16: 16.1 against 14.1 us -- one strip for eight waves, and the whole factor is staged first)
  if (mt >= 9 || (mt >= 5 && d >= 112)) return launch_side_resident<TO>(fac, w, a, gl, batch, n, d, out, rowdot, st);
  // fewer than four rows of tiles: W straight from global memory; from four on W goes through LDS
  const dim3 grid((unsigned)batch);
  if (mt <= 2)
    launch_pb(procrustes_bwd_side_kernel<2, TO>, grid, PB_THREADS, pb_direct_lds<2>(), st, fac, w, a, gl, n, d, out, rowdot);
  else if (mt == 3)
    launch_pb(procrustes_bwd_side_kernel<4, TO>, grid, PB_THREADS, pb_direct_lds<4>(), st, fac, w, a, gl, n, d, out, rowdot);
  else if (mt == 4)
    launch_pb(procrustes_bwd_side_tiled_kernel<4, TO, true, true>, grid, PB_THREADS, pb_tiled_lds<4>(), st, fac, w, a, gl, n, d, 1,
              out, rowdot);
  else                                                     // mt = 5 .. 8 with d < 112
    launch_pb(procrustes_bwd_side_tiled_kernel<8, TO, true, true>, grid, PB_THREADS, pb_tiled_lds<8>(), st, fac, w, a, gl, n, d, 1,
              out, rowdot);
  return check_launch("procrustes_bwd (fused residual product)");
}

// 257 <= n <= 1024, and every n % 4 != 0: row tiles of PBL_RT rows
template <typename TO>
static int launch_side_long(const float* fac, const float* w, const float* a, const float* gl, int batch, int n, int d,
                            TO* out, float* rowdot, hipStream_t st) {
  const int tiles = (n + PBL_RT - 1) / PBL_RT;
  const dim3 grid((unsigned)batch * (unsigned)tiles);
  if (n % 4 == 0 && (((uintptr_t)fac) & 15) == 0)
    launch_pb(procrustes_bwd_side_tiled_kernel<PBL_MT, TO, true, false>, grid, PB_THREADS, pb_tiled_lds<PBL_MT>(), st, fac, w, a, gl,
              n, d, tiles, out, rowdot);
  else
    launch_pb(procrustes_bwd_side_tiled_kernel<PBL_MT, TO, false, false>, grid, PB_THREADS, pb_tiled_lds<PBL_MT>(), st, fac, w, a, gl,
              n, d, tiles, out, rowdot);
  return check_launch("procrustes_bwd (row-tiled residual product)");
}

}  // namespace basd

extern "C" int basd_procrustes_bwd_side(const float* fac, const float* w, const float* a, const float* gl, int batch,
                                        int n, int d, void* out, int out_dtype, float* rowdot, void* stream) {
  using namespace basd;
  if (batch <= 0) return BASD_OK;
  const bool whole = n <= 256 && n % 4 == 0;   // one workgroup per matrix (launch_side); everything else is row-tiled
  if (n < 4 || n > 1024 || d < 16 || d % 16 || (((uintptr_t)fac) & (whole ? 15 : 3)) || (((uintptr_t)w) & 15) ||
      (((uintptr_t)out) & 15))
    return fail(BASD_ERR_SHAPE, "procrustes_bwd_side: need 4 <= n <= 1024, d %% 16 == 0, 16-byte aligned buffers "
                                "(n=%d d=%d)", n, d);
  hipStream_t st = (hipStream_t)stream;
  if (out_dtype == BASD_DTYPE_F32)
    return whole ? launch_side<float>(fac, w, a, gl, batch, n, d, (float*)out, rowdot, st)
                 : launch_side_long<float>(fac, w, a, gl, batch, n, d, (float*)out, rowdot, st);
  if (out_dtype == BASD_DTYPE_BF16)
    return whole ? launch_side<unsigned short>(fac, w, a, gl, batch, n, d, (unsigned short*)out, rowdot, st)
                 : launch_side_long<unsigned short>(fac, w, a, gl, batch, n, d, (unsigned short*)out, rowdot, st);
  return fail(BASD_ERR_DTYPE, "procrustes_bwd_side: out dtype %d", out_dtype);
}

extern "C" int64_t basd_procrustes_bwd_workspace_bytes(int batch, int n) { return (int64_t)2 * batch * n * 4; }

extern "C" int basd_procrustes_bwd(const float* s_w, const float* t_w, const float* a, const float* gl,
                                   const float* fac_s, const float* a_t, int batch, int n, int d_s, int d_t,
                                   void* g_s, int g_s_dtype, float* g_t, float* g_a, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
  using namespace basd;
  if (batch <= 0) return BASD_OK;
  if (workspace == nullptr || workspace_bytes < basd_procrustes_bwd_workspace_bytes(batch, n))
    return fail(BASD_ERR_SHAPE, "procrustes_bwd: workspace of %lld bytes, need %lld", (long long)workspace_bytes,
                (long long)basd_procrustes_bwd_workspace_bytes(batch, n));
  float* dot_s = (float*)workspace;
  float* dot_t = dot_s + (size_t)batch * n;
  int rc = basd_procrustes_bwd_side(a_t, t_w, a, gl, batch, n, d_t, g_t, BASD_DTYPE_F32, dot_t, stream);
  if (rc) return rc;
  if (n <= d_s) {                          // token side: fac_s = a_s [n, n], t_w G^T = a_s s_w
    rc = basd_procrustes_bwd_side(fac_s, s_w, a, gl, batch, n, d_s, g_s, g_s_dtype, dot_s, stream);
  } else {                                 // feature side: fac_s = t_w G^T [n, d_s] was formed in the forward
    rc = basd_procrustes_bwd_rows(fac_s, s_w, a, gl, (int64_t)batch * n, n, d_s, g_s, g_s_dtype, dot_s, stream);
  }
  if (rc) return rc;
  const int64_t total = (int64_t)batch * n;
  hipLaunchKernelGGL(procrustes_ga_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     dot_s, dot_t, a, total, g_a);
  return check_launch("procrustes_bwd (g_a)");
}
