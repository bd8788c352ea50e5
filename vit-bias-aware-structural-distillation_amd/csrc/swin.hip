// Kernels of the frozen Swin teacher trunk (models/swin.py): what lies between the bf16 GEMMs and the LayerNorms.
//
// Activations are the channels-last rows of csrc/convnext.hip: a token grid [B, H, W, C] is a [B H W, ld] bf16 matrix
// (ld >= C, columns C .. ld zero; the 96-wide stage of Swin-T lives in rows of 128).
//
//   basd_window_attention_fwd_bf16   (shifted-)window attention straight from the packed qkv rows, windows up to 8 x 8.
//                                    Layout, slot rule and everything behind the logits: window_attn.h.
//   basd_patch_merge_ln_bf16         2 x 2 neighbour concatenation + LayerNorm over the 4 C channels, one pass.
#include "window_attn.h"

namespace basd {

// ---------------------------------------------------------------------------------------------------------------------
// Window attention.  One wave per (window, head), four per workgroup (consecutive heads of one window, so the waves of a
// workgroup read neighbouring 64-byte pieces of the same rows).  N = ws^2 <= 64 slots fill up to four 16-slot tiles.
//   S^T = K Q^T   A = K rows, B = Q rows, both straight from global memory (slot 16 t + (lane & 15), d = 8 (lane >> 4) ..);
//   logits        the bias is bias[h][query][key] of the image, a padding key is one whose number is >= N;
//   V of the head is the only operand staged in LDS.
// Every global load of the wave is issued before its first LDS store.  Padding slots (>= N) load nothing (zero q, k, v),
// are excluded from every softmax as keys and are never stored as queries.
constexpr int WA_WAVES = 4;
constexpr int WA_SLOTS = 64;                          // slots of a window tile = row / column count of a bias image

__global__ __launch_bounds__(64 * WA_WAVES) void window_attention_kernel(
    const unsigned short* __restrict__ qkv, const float* __restrict__ bias, int H, int W, int heads, int C, int ws,
    int shift, int ld_qkv, int ld_out, float scale, unsigned short* __restrict__ out, int64_t problems) {
  __shared__ __align__(16) unsigned short Vs[WA_WAVES][WA_SLOTS * WIN_LD];
  __shared__ __align__(16) unsigned short Os[WA_WAVES][16 * WIN_LD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int N = ws * ws, nt = (N + 15) >> 4;          // live slots, live 16-slot tiles
  const int nwx = W / ws, nwy = H / ws;
  const int64_t prob = (int64_t)blockIdx.x * WA_WAVES + wave;
  const bool live = prob < problems;                  // no early exit: the workgroup barriers below are reached by all
  int h = 0, wx = 0, wy = 0;
  int64_t b = 0;
  if (live) {
    h = (int)(prob % heads);
    int64_t q = prob / heads;
    wx = (int)(q % nwx);
    q /= nwx;
    wy = (int)(q % nwy);
    b = q / nwy;
  }
  // slot = lane: its token row in [B H W) and the mask label of its rolled coordinate
  int64_t myrow = 0;
  int mylab = 0;
  if (lane < N) myrow = window_slot(lane, ws, wy, wx, b, H, W, shift, mylab);
  const int rlo = (int)(myrow & 0xffffffff), rhi = (int)(myrow >> 32);

  // ---- all loads of the wave: q, k, v fragments of slot 16 t + li, d = 8 g .. 8 g + 7
  uint4 qf[4], kf[4], vf[4];
  int qlab[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int slot = 16 * t + li;
    const int64_t row = ((int64_t)__shfl(rhi, slot, 64) << 32) | (unsigned int)__shfl(rlo, slot, 64);
    qlab[t] = __shfl(mylab, slot, 64);
    qf[t] = kf[t] = vf[t] = make_uint4(0, 0, 0, 0);
    if (live && slot < N) {
      const unsigned short* p = qkv + row * ld_qkv + h * 32 + 8 * g;
      qf[t] = *reinterpret_cast<const uint4*>(p);
      kf[t] = *reinterpret_cast<const uint4*>(p + C);
      vf[t] = *reinterpret_cast<const uint4*>(p + 2 * C);
    }
  }
  unsigned short* Vw = Vs[wave];
  unsigned short* Ow = Os[wave];
#pragma unroll
  for (int t = 0; t < 4; ++t) *reinterpret_cast<uint4*>(Vw + (16 * t + li) * WIN_LD + 8 * g) = vf[t];
  __syncthreads();

  // labels of this lane's keys 16 kt + 4 g + r
  int klab[4][4];
#pragma unroll
  for (int kt = 0; kt < 4; ++kt)
#pragma unroll
    for (int r = 0; r < 4; ++r) klab[kt][r] = __shfl(mylab, 16 * kt + 4 * g + r, 64);

  const float* bh = bias + (size_t)h * WA_SLOTS * WA_SLOTS;
  const int npad = (ld_out - C) >> 3;                 // 16-byte zero vectors behind the C channels of an output row
  for (int qt = 0; qt < nt; ++qt) {
    const int query = 16 * qt + li;
    // qf / qlab of the running tile: static register indices only
    const uint4 qq = qt == 0 ? qf[0] : qt == 1 ? qf[1] : qt == 2 ? qf[2] : qf[3];
    const int ql = qt == 0 ? qlab[0] : qt == 1 ? qlab[1] : qt == 2 ? qlab[2] : qlab[3];
    float s[4][4];
    float mx = -3.0e38f;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
      if (kt < nt) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(&kf[kt]),
                                                      *reinterpret_cast<const bf16x8*>(&qq), acc, 0, 0, 0);
        bv = *reinterpret_cast<const float4*>(bh + query * WA_SLOTS + 16 * kt + 4 * g);
      }
      const float bb[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float l = fmaf(acc[r], scale, bb[r]);
        if (klab[kt][r] != ql) l += -100.0f;
        if (16 * kt + 4 * g + r >= N) l = -3.0e38f;
        s[kt][r] = l;
        mx = fmaxf(mx, l);
      }
    }
    const float inv = window_softmax<4, false>(s, mx, nt);
    f32x4 o[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    window_pv<4>(s, inv, Vw, nt, lane, o);
    window_tile_to_lds(o, Ow, lane);
    __syncthreads();
    {
      const int slot = 16 * qt + (lane >> 2);
      const int64_t row = ((int64_t)__shfl(rhi, slot, 64) << 32) | (unsigned int)__shfl(rlo, slot, 64);
      if (live && slot < N) window_store_row(out, row, ld_out, Ow, h, heads, C, npad, lane);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Patch merging + LayerNorm.  One wave per output pixel, four per workgroup.  The 4 C output channels are 4 C / 8 vectors
// of 8; vector j belongs to neighbour j / (C / 8) in the order (2r, 2c), (2r+1, 2c), (2r, 2c+1), (2r+1, 2c+1) and lane l
// owns the vectors l, l + 64, ... (at most 8: 4 C <= 4096).  Two-pass fp32 statistics on the register copy, summed over
// the lane's registers in index order and over the wave by the xor butterfly: the same input gives the same bits.
constexpr int PM_WAVES = 4;
constexpr int PM_VEC = 8;

__global__ __launch_bounds__(64 * PM_WAVES) void patch_merge_ln_kernel(
    const unsigned short* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta, int H, int W,
    int C, int ld_in, float eps, unsigned short* __restrict__ y, int64_t pixels) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t pix = (int64_t)blockIdx.x * PM_WAVES + wave;
  if (pix >= pixels) return;                          // wave-uniform; the kernel has no workgroup barrier
  const int Ho = H >> 1, Wo = W >> 1;
  const int ow = (int)(pix % Wo);
  const int64_t q = pix / Wo;
  const int oh = (int)(q % Ho);
  const int64_t b = q / Ho;
  const int cv = C >> 3, nvec = 4 * cv;
  const unsigned short* src = x + ((b * H + 2 * oh) * (int64_t)W + 2 * ow) * ld_in;
  uint4 raw[PM_VEC];
#pragma unroll
  for (int i = 0; i < PM_VEC; ++i) {
    const int j = lane + 64 * i;
    raw[i] = make_uint4(0, 0, 0, 0);
    if (j < nvec) {
      const int nb = j / cv, c8 = j - nb * cv;
      raw[i] = *reinterpret_cast<const uint4*>(src + ((int64_t)(nb & 1) * W + (nb >> 1)) * ld_in + c8 * 8);
    }
  }
  float v[PM_VEC][8];
  float part = 0.f;
#pragma unroll
  for (int i = 0; i < PM_VEC; ++i) {
    unpack8(raw[i], v[i]);                            // vectors behind nvec are zero: they add nothing to the sum
#pragma unroll
    for (int e = 0; e < 8; ++e) part += v[i][e];
  }
  const float inv_n = 1.f / (float)(4 * C);
  const float mean = wave_sum(part) * inv_n;
  part = 0.f;
#pragma unroll
  for (int i = 0; i < PM_VEC; ++i) {
    if (lane + 64 * i < nvec) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        v[i][e] -= mean;
        part += v[i][e] * v[i][e];
      }
    }
  }
  const float rstd = rsqrtf(wave_sum(part) * inv_n + eps);
  unsigned short* dst = y + pix * (int64_t)(4 * C);
#pragma unroll
  for (int i = 0; i < PM_VEC; ++i) {
    const int j = lane + 64 * i;
    if (j < nvec) {
      const float4 g0 = *reinterpret_cast<const float4*>(gamma + j * 8);
      const float4 g1 = *reinterpret_cast<const float4*>(gamma + j * 8 + 4);
      const float4 e0 = *reinterpret_cast<const float4*>(beta + j * 8);
      const float4 e1 = *reinterpret_cast<const float4*>(beta + j * 8 + 4);
      const float gv[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
      const float ev[8] = {e0.x, e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w};
      float o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = v[i][e] * rstd * gv[e] + ev[e];
      *reinterpret_cast<uint4*>(dst + j * 8) = pack8(o);
    }
  }
}

}  // namespace basd

extern "C" int basd_window_attention_fwd_bf16(const void* qkv, const float* bias, int B, int H, int W, int heads, int C,
                                              int ws, int shift, int ld_qkv, int ld_out, float scale, void* out,
                                              void* stream) {
  using namespace basd;
  if (B <= 0) return BASD_OK;
  int64_t problems, grid;
  if (int rc = window_attention_check("window_attention_fwd", 1, 8, qkv, bias, out, B, H, W, heads, C, ws, shift, ld_qkv,
                                      ld_out, WA_WAVES, problems, grid))
    return rc;
  hipLaunchKernelGGL(window_attention_kernel, dim3((unsigned)grid), dim3(64 * WA_WAVES), 0, (hipStream_t)stream,
                     (const unsigned short*)qkv, bias, H, W, heads, C, ws, shift, ld_qkv, ld_out, scale,
                     (unsigned short*)out, problems);
  return check_launch("window_attention_fwd");
}

extern "C" int basd_patch_merge_ln_bf16(const void* x, const float* gamma, const float* beta, int B, int H, int W, int C,
                                        int ld_in, float eps, void* y, void* stream) {
  using namespace basd;
  if (B <= 0) return BASD_OK;
  if (H < 2 || W < 2 || H % 2 || W % 2)
    return fail(BASD_ERR_SHAPE, "patch_merge_ln: H and W must be even (got %d x %d)", H, W);
  if (C % 8 || 4 * C < 8 || 4 * C > 64 * PM_VEC * 8)
    return fail(BASD_ERR_SHAPE, "patch_merge_ln: C %% 8 == 0, 8 <= 4 C <= %d (got C=%d)", 64 * PM_VEC * 8, C);
  if (ld_in % 8 || ld_in < C)
    return fail(BASD_ERR_SHAPE, "patch_merge_ln: ld_in must be a multiple of 8 with C <= ld_in (got C=%d ld_in=%d)", C, ld_in);
  if (((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)y) & 15)
    return fail(BASD_ERR_SHAPE, "patch_merge_ln: 16-byte aligned buffers required");
  if (x == y) return fail(BASD_ERR_SHAPE, "patch_merge_ln: y must not alias x");
  const int64_t pixels = (int64_t)B * (H / 2) * (W / 2);
  const int64_t grid = (pixels + PM_WAVES - 1) / PM_WAVES;
  if (grid > 0x7fffffffLL) return fail(BASD_ERR_SHAPE, "patch_merge_ln: %lld workgroups", (long long)grid);
  hipLaunchKernelGGL(patch_merge_ln_kernel, dim3((unsigned)grid), dim3(64 * PM_WAVES), 0, (hipStream_t)stream,
                     (const unsigned short*)x, gamma, beta, H, W, C, ld_in, eps, (unsigned short*)y, pixels);
  return check_launch("patch_merge_ln");
}
