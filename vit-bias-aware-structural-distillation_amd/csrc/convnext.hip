// Kernels of the frozen ConvNeXt-V2 teacher trunk (models/convnext.py): everything between the bf16 GEMMs.
//
// Activations are channels-last rows: a feature map [B, H, W, C] is a [B H W, ld] bf16 matrix (ld >= C; the columns
// C .. ld are zero -- stage 0 of ConvNeXt-T lives in rows of 128 for its 96 channels, the narrowest row the GEMM tiles).
//
//   basd_dwconv7_ln_bf16  depthwise 7 x 7 (zero padding 3, bias) + LayerNorm over the channels of every output pixel in
//                         one launch: the convolution output stays in registers.
//   basd_grn_bf16         global response normalisation in place on fc1's output: a statistics pass (sum of squares per
//                         image and channel over H W, fp32, summed in a fixed order) and an apply pass.
//   basd_patchify_bf16    non-overlapping p x p patches as GEMM rows (the stride-p convolutions of the stem and of the
//                         downsample layers): pure data movement.
//
// None of them is matrix-core work.  A lane owns 8 contiguous channels (one 16-byte load) everywhere.
#include "basd_frag.h"

namespace basd {

// ---------------------------------------------------------------------------------------------------------------------
// Depthwise 7 x 7 + LayerNorm.
//
// Work item = a strip of DW_S horizontally adjacent output pixels of one image row.  LP = C / 8 lanes share an item (lane
// lc owns channels 8 lc .. 8 lc + 7 of all DW_S pixels) and a workgroup of 384 threads holds PP = 384 / LP items, which
// is the whole workgroup for every width 96 * 2^k (LP = 12 .. 96) and for 128 * 2^k.  Per input row a lane loads the
// DW_S + 6 input vectors and the 7 weight vectors of the row once and feeds 7 DW_S x 8 FMAs from them (a lane that owned
// one pixel would issue 98 loads per pixel instead of 119 per four).  The halo between neighbouring items is shared
// through L1 / L2 (consecutive items are neighbours in the row, then in the column).
// The channel statistics are two-pass (mean, then centred squares) on the register copy.  LP is not a power of two and
// an item's lanes straddle waves, so the per-lane partials go through LDS: the partials of a pixel form a row of LP
// floats, 8 lanes sum a row (strided, then DPP), always in the same order.
constexpr int DW_S = 4;
constexpr int DW_THREADS = 384;

__device__ __forceinline__ void dw_row_sums(const float* red, float* stat, int R, int LP) {
  const int t = threadIdx.x, j = t & 7;
  for (int r = t >> 3; r < R; r += DW_THREADS / 8) {
    float v = 0.f;
    for (int k = j; k < LP; k += 8) v += red[r * LP + k];
    v = group8_sum(v);
    if (j == 0) stat[r] = v;
  }
}

__global__ __launch_bounds__(DW_THREADS) void dwconv7_ln_kernel(
    const unsigned short* __restrict__ x, const unsigned short* __restrict__ w49, const float* __restrict__ bias,
    const float* __restrict__ gamma, const float* __restrict__ beta, int H, int W, int C, int ld_in, int ld_out,
    float eps, unsigned short* __restrict__ y, int LP, int PP, int nstrips, int64_t items) {
  __shared__ float red[DW_THREADS * DW_S];
  __shared__ float stat[DW_THREADS * DW_S];
  const int t = threadIdx.x;
  const int pslot = t / LP, lc = t - pslot * LP;
  const bool active = pslot < PP;
  const int64_t item = (int64_t)blockIdx.x * PP + pslot;
  const bool live = active && item < items;
  int w0 = 0, hh = 0;
  int64_t img = 0;
  if (live) {
    w0 = (int)(item % nstrips) * DW_S;
    const int64_t q = item / nstrips;
    hh = (int)(q % H);
    img = q / H;
  }

  float acc[DW_S][8];
#pragma unroll
  for (int s = 0; s < DW_S; ++s)
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[s][i] = 0.f;

  if (live) {
    const float4 b0 = *reinterpret_cast<const float4*>(bias + lc * 8);
    const float4 b1 = *reinterpret_cast<const float4*>(bias + lc * 8 + 4);
    const float bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
    for (int s = 0; s < DW_S; ++s)
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[s][i] = bv[i];
    const int dy_lo = hh < 3 ? 3 - hh : 0;
    const int dy_hi = hh + 3 >= H ? H + 2 - hh : 6;                    // inclusive: rows hh + dy - 3 inside [0, H)
    for (int dy = dy_lo; dy <= dy_hi; ++dy) {
      const int iy = hh + dy - 3;
      const unsigned short* xrow = x + ((img * H + iy) * (int64_t)W) * ld_in + lc * 8;
      uint4 raw[DW_S + 6];
#pragma unroll
      for (int j = 0; j < DW_S + 6; ++j) {
        const int ix = w0 + j - 3;
        raw[j] = make_uint4(0, 0, 0, 0);
        if (ix >= 0 && ix < W) raw[j] = *reinterpret_cast<const uint4*>(xrow + (int64_t)ix * ld_in);
      }
      float wf[7][8];
#pragma unroll
      for (int dx = 0; dx < 7; ++dx)
        unpack8(*reinterpret_cast<const uint4*>(w49 + (size_t)(dy * 7 + dx) * C + lc * 8), wf[dx]);
#pragma unroll
      for (int j = 0; j < DW_S + 6; ++j) {
        float xf[8];
        unpack8(raw[j], xf);
#pragma unroll
        for (int s = 0; s < DW_S; ++s) {
          const int dx = j - s;                                        // compile-time after unrolling
          if (dx >= 0 && dx < 7) {
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[s][i] = fmaf(xf[i], wf[dx][i], acc[s][i]);
          }
        }
      }
    }
  }

  // ---- LayerNorm over C of every pixel: mean
  const int R = PP * DW_S;
  const float inv_c = 1.f / (float)C;
  if (active) {
#pragma unroll
    for (int s = 0; s < DW_S; ++s) {
      float p = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) p += acc[s][i];
      red[(pslot * DW_S + s) * LP + lc] = p;
    }
  }
  __syncthreads();
  dw_row_sums(red, stat, R, LP);
  __syncthreads();
  float mean[DW_S];
  if (active) {
#pragma unroll
    for (int s = 0; s < DW_S; ++s) {
      mean[s] = stat[pslot * DW_S + s] * inv_c;
      float p = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        acc[s][i] -= mean[s];
        p += acc[s][i] * acc[s][i];
      }
      red[(pslot * DW_S + s) * LP + lc] = p;
    }
  }
  __syncthreads();
  dw_row_sums(red, stat, R, LP);
  __syncthreads();
  if (!live) return;

  const float4 g0 = *reinterpret_cast<const float4*>(gamma + lc * 8);
  const float4 g1 = *reinterpret_cast<const float4*>(gamma + lc * 8 + 4);
  const float4 e0 = *reinterpret_cast<const float4*>(beta + lc * 8);
  const float4 e1 = *reinterpret_cast<const float4*>(beta + lc * 8 + 4);
  const float gv[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
  const float ev[8] = {e0.x, e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w};
  const int npad = (ld_out - C) >> 3;                                  // zero vectors behind the C channels (<= LP)
  unsigned short* yrow = y + ((img * H + hh) * (int64_t)W) * ld_out;
#pragma unroll
  for (int s = 0; s < DW_S; ++s) {
    if (w0 + s >= W) break;
    const float rstd = rsqrtf(stat[pslot * DW_S + s] * inv_c + eps);
    float o[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = acc[s][i] * rstd * gv[i] + ev[i];
    unsigned short* yp = yrow + (int64_t)(w0 + s) * ld_out;
    *reinterpret_cast<uint4*>(yp + lc * 8) = pack8(o);
    if (lc < npad) *reinterpret_cast<uint4*>(yp + C + lc * 8) = make_uint4(0, 0, 0, 0);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// GRN.  Workspace: fp32 [B, NS, C] partial sums of squares, NS = ceil(HW / 256) row splits of 256 rows; a workgroup of
// the statistics pass owns (image, split, CL 8-channel chunks) and sums its rows in RS = 256 / CL interleaved slices,
// combined in slice order through LDS: no atomics, the result does not depend on the schedule.
constexpr int GRN_ROWS = 256;
constexpr int GRN_MAX_C = 4096;

static int grn_splits(int HW) { return (HW + GRN_ROWS - 1) / GRN_ROWS; }

__global__ __launch_bounds__(256) void grn_stats_kernel(const unsigned short* __restrict__ x, int HW, int C, int CL,
                                                        float* __restrict__ ws) {
  __shared__ float part[256 * 8];
  const int t = threadIdx.x, split = blockIdx.y, b = blockIdx.z, NS = gridDim.y;
  const int RS = 256 / CL;
  const int rs = t / CL, cl = t - rs * CL;
  const int r0 = split * GRN_ROWS;
  const int r1 = r0 + GRN_ROWS < HW ? r0 + GRN_ROWS : HW;
  float s[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) s[i] = 0.f;
  if (rs < RS) {
    const unsigned short* p = x + ((int64_t)b * HW) * C + ((int64_t)blockIdx.x * CL + cl) * 8;
    int r = r0 + rs;
    for (; r + 3 * RS < r1; r += 4 * RS) {                              // four rows in flight
      uint4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const uint4*>(p + (int64_t)(r + u * RS) * C);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float f[8];
        unpack8(v[u], f);
#pragma unroll
        for (int i = 0; i < 8; ++i) s[i] = fmaf(f[i], f[i], s[i]);
      }
    }
    for (; r < r1; r += RS) {
      float f[8];
      unpack8(*reinterpret_cast<const uint4*>(p + (int64_t)r * C), f);
#pragma unroll
      for (int i = 0; i < 8; ++i) s[i] = fmaf(f[i], f[i], s[i]);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) part[(rs * CL + cl) * 8 + i] = s[i];
  }
  __syncthreads();
  float* out = ws + ((int64_t)b * NS + split) * C + (int64_t)blockIdx.x * CL * 8;
  for (int e = t; e < CL * 8; e += 256) {
    float v = 0.f;
    for (int k = 0; k < RS; ++k) v += part[k * CL * 8 + e];
    out[e] = v;
  }
}

__global__ __launch_bounds__(256) void grn_apply_kernel(unsigned short* __restrict__ x, const float* __restrict__ weight,
                                                        const float* __restrict__ bias, int HW, int C, float eps,
                                                        const float* __restrict__ ws) {
  __shared__ float a[GRN_MAX_C];
  __shared__ float bsh[GRN_MAX_C];
  __shared__ float wsum[4];
  const int t = threadIdx.x, split = blockIdx.x, b = blockIdx.y, NS = gridDim.x;
  // prologue: g = ||x||_2 over (H, W) per channel of this image, n = g / (mean_c g + eps)
  float local = 0.f;
  for (int c = t; c < C; c += 256) {
    float s = 0.f;
    for (int k = 0; k < NS; ++k) s += ws[((int64_t)b * NS + k) * C + c];
    const float g = sqrtf(s);
    a[c] = g;
    local += g;
  }
  local = wave_sum(local);
  if ((t & 63) == 0) wsum[t >> 6] = local;
  __syncthreads();
  const float inv = 1.f / ((wsum[0] + wsum[1] + wsum[2] + wsum[3]) / (float)C + eps);
  for (int c = t; c < C; c += 256) {
    a[c] = weight[c] * (a[c] * inv);
    bsh[c] = bias[c];
  }
  __syncthreads();
  // y = x + (bias + weight n x)
  const int r0 = split * GRN_ROWS;
  const int r1 = r0 + GRN_ROWS < HW ? r0 + GRN_ROWS : HW;
  const int c8 = C >> 3;
  const int nvec = (r1 - r0) * c8;
  unsigned short* base = x + ((int64_t)b * HW + r0) * C;
  for (int v = t; v < nvec; v += 256) {
    const int c = (v % c8) * 8;
    uint4* p = reinterpret_cast<uint4*>(base + (int64_t)v * 8);
    float f[8];
    unpack8(*p, f);
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = f[i] + fmaf(a[c + i], f[i], bsh[c + i]);
    *p = pack8(f);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Patch gather.  Output row (b, oh, ow), column k = (i p + j) C + c  <-  x[b, c, oh p + i, ow p + j] through element
// strides, columns K .. K_pad zero.  One 16-byte output vector per thread; VEC: the 8 columns are 8 contiguous channels
// of one input pixel (channels-last source, C % 8 == 0, 16-byte aligned), one load.
template <bool VEC>
__global__ __launch_bounds__(256) void patchify_kernel(const unsigned short* __restrict__ x, int C, int OH, int OW,
                                                       int64_t sb, int64_t sc, int64_t sh, int64_t sw, int p, int K,
                                                       int K_pad, unsigned short* __restrict__ out, int64_t nvec) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= nvec) return;
  const int kv = K_pad >> 3;
  const int64_t row = v / kv;
  const int k0 = (int)(v - row * kv) * 8;
  const int ow = (int)(row % OW);
  const int64_t q = row / OW;
  const int oh = (int)(q % OH);
  const int64_t b = q / OH;
  const unsigned short* src = x + b * sb + (int64_t)oh * p * sh + (int64_t)ow * p * sw;
  uint4 o = make_uint4(0, 0, 0, 0);
  if (VEC) {
    if (k0 < K) {
      const int pix = k0 / C, c = k0 - pix * C;
      const int i = pix / p, j = pix - i * p;
      o = *reinterpret_cast<const uint4*>(src + i * sh + j * sw + c);
    }
  } else {
    unsigned short e[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int k = k0 + u;
      e[u] = 0;
      if (k < K) {
        const int pix = k / C, c = k - pix * C;
        const int i = pix / p, j = pix - i * p;
        e[u] = src[i * sh + j * sw + c * sc];
      }
    }
    o = make_uint4(e[0] | ((unsigned)e[1] << 16), e[2] | ((unsigned)e[3] << 16), e[4] | ((unsigned)e[5] << 16),
                   e[6] | ((unsigned)e[7] << 16));
  }
  *reinterpret_cast<uint4*>(out + v * 8) = o;
}

}  // namespace basd

extern "C" int basd_dwconv7_ln_bf16(const void* x, const void* w49, const float* bias, const float* gamma,
                                    const float* beta, int B, int H, int W, int C, int ld_in, int ld_out, float eps,
                                    void* y, void* stream) {
  using namespace basd;
  if (B <= 0) return BASD_OK;
  if (H < 1 || W < 1) return fail(BASD_ERR_SHAPE, "dwconv7_ln_bf16: H, W >= 1 required (got %d x %d)", H, W);
  if (C % 8 || C < 8 || C > 2048) return fail(BASD_ERR_SHAPE, "dwconv7_ln_bf16: C %% 8 == 0, 8 <= C <= 2048 (got %d)", C);
  if (ld_in < C || ld_in % 8 || ld_out < C || ld_out % 8 || ld_out - C > C)
    return fail(BASD_ERR_SHAPE, "dwconv7_ln_bf16: row strides must be multiples of 8 with C <= ld, ld_out <= 2 C "
                "(got C=%d ld_in=%d ld_out=%d)", C, ld_in, ld_out);
  if (((uintptr_t)x | (uintptr_t)w49 | (uintptr_t)y | (uintptr_t)bias | (uintptr_t)gamma | (uintptr_t)beta) & 15)
    return fail(BASD_ERR_SHAPE, "dwconv7_ln_bf16: 16-byte aligned buffers required");
  const int LP = C / 8, PP = DW_THREADS / LP;
  const int nstrips = (W + DW_S - 1) / DW_S;
  const int64_t items = (int64_t)B * H * nstrips;
  const int64_t grid = (items + PP - 1) / PP;
  if (grid > 0x7fffffffLL) return fail(BASD_ERR_SHAPE, "dwconv7_ln_bf16: %lld workgroups", (long long)grid);
  hipLaunchKernelGGL(dwconv7_ln_kernel, dim3((unsigned)grid), dim3(DW_THREADS), 0, (hipStream_t)stream,
                     (const unsigned short*)x, (const unsigned short*)w49, bias, gamma, beta, H, W, C, ld_in, ld_out,
                     eps, (unsigned short*)y, LP, PP, nstrips, items);
  return check_launch("dwconv7_ln_bf16");
}

extern "C" int64_t basd_grn_workspace_bytes(int B, int HW, int C) {
  if (B <= 0 || HW <= 0 || C <= 0) return 0;
  return (int64_t)B * basd::grn_splits(HW) * C * (int64_t)sizeof(float);
}

extern "C" int basd_grn_bf16(void* x, const float* weight, const float* bias, int B, int HW, int C, float eps,
                             void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace basd;
  if (B <= 0 || HW <= 0) return BASD_OK;
  if (C % 8 || C < 8 || C > GRN_MAX_C)
    return fail(BASD_ERR_SHAPE, "grn_bf16: C %% 8 == 0, 8 <= C <= %d (got %d)", GRN_MAX_C, C);
  const int NS = grn_splits(HW);
  if (B > 65535 || NS > 65535) return fail(BASD_ERR_SHAPE, "grn_bf16: B and H W / 256 <= 65535 (got %d, %d)", B, NS);
  if (workspace == nullptr || workspace_bytes < basd_grn_workspace_bytes(B, HW, C))
    return fail(BASD_ERR_WORKSPACE, "grn_bf16: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                (long long)basd_grn_workspace_bytes(B, HW, C));
  if (((uintptr_t)x | (uintptr_t)workspace) & 15) return fail(BASD_ERR_SHAPE, "grn_bf16: 16-byte aligned buffers required");
  const int c8 = C / 8;
  int CL = 1;
  for (int d = 64; d >= 1; --d)
    if (c8 % d == 0) { CL = d; break; }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(grn_stats_kernel, dim3(c8 / CL, NS, B), dim3(256), 0, st, (const unsigned short*)x, HW, C, CL,
                     (float*)workspace);
  hipLaunchKernelGGL(grn_apply_kernel, dim3(NS, B), dim3(256), 0, st, (unsigned short*)x, weight, bias, HW, C, eps,
                     (const float*)workspace);
  return check_launch("grn_bf16");
}

extern "C" int basd_patchify_bf16(const void* x, int B, int C, int H, int W, int64_t sb, int64_t sc, int64_t sh,
                                  int64_t sw, int p, int K_pad, void* out, void* stream) {
  using namespace basd;
  if (B <= 0) return BASD_OK;
  if (p < 1 || C < 1 || H < p || W < p || H % p || W % p)
    return fail(BASD_ERR_SHAPE, "patchify_bf16: H and W must be multiples of p (got %d x %d, p=%d)", H, W, p);
  const int64_t K = (int64_t)C * p * p;
  if (K_pad % 8 || K > K_pad || K_pad > (1 << 20))
    return fail(BASD_ERR_SHAPE, "patchify_bf16: K_pad %% 8 == 0 and C p p <= K_pad (got K=%lld K_pad=%d)", (long long)K, K_pad);
  if ((uintptr_t)out & 15) return fail(BASD_ERR_SHAPE, "patchify_bf16: 16-byte aligned output required");
  const int OH = H / p, OW = W / p;
  const int64_t nvec = (int64_t)B * OH * OW * (K_pad / 8);
  const int64_t grid = (nvec + 255) / 256;
  if (grid > 0x7fffffffLL) return fail(BASD_ERR_SHAPE, "patchify_bf16: %lld workgroups", (long long)grid);
  const bool vec = sc == 1 && C % 8 == 0 && sb % 8 == 0 && sh % 8 == 0 && sw % 8 == 0 && ((uintptr_t)x & 15) == 0;
  hipStream_t st = (hipStream_t)stream;
  if (vec)
    hipLaunchKernelGGL(patchify_kernel<true>, dim3((unsigned)grid), dim3(256), 0, st, (const unsigned short*)x, C, OH, OW,
                       sb, sc, sh, sw, p, (int)K, K_pad, (unsigned short*)out, nvec);
  else
    hipLaunchKernelGGL(patchify_kernel<false>, dim3((unsigned)grid), dim3(256), 0, st, (const unsigned short*)x, C, OH, OW,
                       sb, sc, sh, sw, p, (int)K, K_pad, (unsigned short*)out, nvec);
  return check_launch("patchify_bf16");
}
