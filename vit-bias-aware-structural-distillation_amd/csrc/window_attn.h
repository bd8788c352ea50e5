// What the two window attention kernels of the Swin trunk share (swin.hip: windows up to 8 x 8, one wave per (window,
// head), operands in registers, bias as a [heads, 64, 64] image; swin_wide.hip: windows 9 x 9 to 16 x 16, one workgroup
// per (window, head), K / V in LDS, bias as timm's table): the layout, the slot rule, everything behind the logits, and
// the refusals of the two C entries.  A change of the roll, the mask or a rounding point is made here, once.
//
// Layout.  Activations are channels-last rows: a token grid [B, H, W, C] is a [B H W, ld] bf16 matrix (ld >= C, columns
// C .. ld zero).  qkv rows hold q | k | v in their first 3 C columns, each [heads, 32]; head dim 32 is exactly one
// k-step of v_mfma_f32_16x16x32_bf16.  The N = ws^2 slots of a window fill TILES 16-slot tiles (4 or 16).
//
// Slot rule (window_slot).  The cyclic roll, the window partition and their inverses are index arithmetic: slot
// (iy, ix) of window (wy, wx) IS token ((wy ws + iy + shift) mod H, (wx ws + ix + shift) mod W), for the loads and for
// the store; the shift mask is the label 3 ly + lx of the slot's rolled coordinate (wy ws + iy, wx ws + ix) under the
// slices [0, -ws), [-ws, -shift), [-shift, end) of each axis, all zero without a shift.
//
// Behind the logits.  Both kernels hold S^T = K Q^T in 16x16x32 accumulators: lane (li = lane & 15, g = lane >> 4) owns
// query 16 qt + li and, of key tile kt, the keys 16 kt + 4 g + {0..3}.  Each kernel forms its own logits
//   scale * s + bias + (label[query] != label[key] ? -100 : 0) in fp32, dead keys (>= N) -3e38
// -- the bias source and the dead-key test are where the two really differ -- and hands s[TILES][4] with the lane's
// running max to window_softmax, window_pv, window_tile_to_lds and window_store_row below.
#pragma once
#include "basd_frag.h"

namespace basd {

constexpr int WIN_LD = 40;                            // LDS row stride in bf16: 32 + 8 (16-byte aligned, bank rotation)

// slot iy ws + ix (< ws^2) of window (wy, wx) of image b -> its token row in [B H W), label = its mask label
__device__ __forceinline__ int64_t window_slot(int slot, int ws, int wy, int wx, int64_t b, int H, int W, int shift,
                                               int& label) {
  const int iy = slot / ws, ix = slot - iy * ws;
  const int ry = wy * ws + iy, rx = wx * ws + ix;                      // coordinate in the rolled grid
  int y = ry + shift, x = rx + shift;
  if (y >= H) y -= H;
  if (x >= W) x -= W;
  const int64_t row = (b * H + y) * (int64_t)W + x;
  label = 0;
  if (shift > 0) {                                                     // slices [0, -ws), [-ws, -shift), [-shift, end)
    const int ly = ry < H - ws ? 0 : (ry < H - shift ? 1 : 2);
    const int lx = rx < W - ws ? 0 : (rx < W - shift ? 1 : 2);
    label = 3 * ly + lx;
  }
  return row;
}

// s: the lane's logits, mx: their max -> s: exp2((s - max) log2 e) of the query column, returns 1 / sum.  GUARD: only
// the nt live tiles are touched and the others are set to zero (the empty half of the last 32-key step of window_pv);
// without it every tile is live or holds -3e38: exp2(-huge) = 0.
template <int TILES, bool GUARD>
__device__ __forceinline__ float window_softmax(float (&s)[TILES][4], float mx, int nt) {
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  float sum = 0.f;
#pragma unroll
  for (int kt = 0; kt < TILES; ++kt) {
    if (!GUARD || kt < nt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = __builtin_amdgcn_exp2f((s[kt][r] - mx) * 1.4426950408889634f);
        s[kt][r] = p;
        sum += p;
      }
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) s[kt][r] = 0.f;
    }
  }
  sum += __shfl_xor(sum, 16, 64);
  sum += __shfl_xor(sum, 32, 64);
  return 1.f / sum;
}

// o[dt][r] (zero on entry) += O[query 4 g + r of the tile][d = 16 dt + li] over TILES / 2 32-key steps: the probabilities
// of a step, times inv and rounded to bf16, are the A fragment (attention.hip), B = V through the transposing LDS read
// on the same eight keys.  V: rows of WIN_LD, zero behind N (a half-empty step has P = 0 against V = 0).
template <int TILES>
__device__ __forceinline__ void window_pv(const float (&s)[TILES][4], float inv, const unsigned short* V, int nt, int lane,
                                          f32x4 (&o)[2]) {
  const int g = lane >> 4;
#pragma unroll
  for (int ks = 0; ks < TILES / 2; ++ks) {
    if (2 * ks < nt) {
      uint4 pw;
      pw.x = pack_bf16(s[2 * ks][0] * inv, s[2 * ks][1] * inv);
      pw.y = pack_bf16(s[2 * ks][2] * inv, s[2 * ks][3] * inv);
      pw.z = pack_bf16(s[2 * ks + 1][0] * inv, s[2 * ks + 1][1] * inv);
      pw.w = pack_bf16(s[2 * ks + 1][2] * inv, s[2 * ks + 1][3] * inv);
      const bf16x8 pa = *reinterpret_cast<const bf16x8*>(&pw);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, tr_split(V, WIN_LD, 32 * ks + 4 * g, 16 * dt, lane), o[dt], 0,
                                                        0, 0);
    }
  }
}

// the accumulators of window_pv -> the wave's 16 x WIN_LD tile Ow, rounded to bf16 (a workgroup barrier follows)
__device__ __forceinline__ void window_tile_to_lds(const f32x4 (&o)[2], unsigned short* Ow, int lane) {
  const int li = lane & 15, g = lane >> 4;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 4; r += 2) {
      const unsigned int w2 = pack_bf16(o[dt][r], o[dt][r + 1]);
      Ow[(4 * g + r) * WIN_LD + 16 * dt + li] = (unsigned short)(w2 & 0xffffu);
      Ow[(4 * g + r + 1) * WIN_LD + 16 * dt + li] = (unsigned short)(w2 >> 16);
    }
}

// lane stores the 16 bytes c8 = lane & 3 of tile row lane >> 2 to token row `row` (the caller's: from a shuffle or from
// LDS) and its share of the npad = (ld_out - C) / 8 zero vectors behind the C channels
__device__ __forceinline__ void window_store_row(unsigned short* __restrict__ out, int64_t row, int ld_out,
                                                 const unsigned short* Ow, int h, int heads, int C, int npad, int lane) {
  const int r = lane >> 2, c8 = lane & 3;
  unsigned short* orow = out + row * ld_out;
  *reinterpret_cast<uint4*>(orow + h * 32 + c8 * 8) = *reinterpret_cast<const uint4*>(Ow + r * WIN_LD + c8 * 8);
  for (int j = h * 4 + c8; j < npad; j += heads * 4)                   // the pad columns, shared out over the heads
    *reinterpret_cast<uint4*>(orow + C + j * 8) = make_uint4(0, 0, 0, 0);
}

// The refusals of both C entries (name: the entry without basd_ / _bf16, lo .. hi: its windows) -> BASD_OK and the
// grid for `per_group` (window, head) problems per workgroup.
inline int window_attention_check(const char* name, int lo, int hi, const void* qkv, const void* bias, const void* out,
                                  int B, int H, int W, int heads, int C, int ws, int shift, int ld_qkv, int ld_out,
                                  int per_group, int64_t& problems, int64_t& grid) {
  if (ws < lo || ws > hi || shift < 0 || shift >= ws)
    return fail(BASD_ERR_SHAPE, "%s: %d <= ws <= %d and 0 <= shift < ws (got ws=%d shift=%d)", name, lo, hi, ws, shift);
  if (H < ws || W < ws || H % ws || W % ws)
    return fail(BASD_ERR_SHAPE, "%s: H and W must be multiples of ws (got %d x %d, ws=%d)", name, H, W, ws);
  if (heads < 1 || C != 32 * heads)
    return fail(BASD_ERR_SHAPE, "%s: head dim 32 only, C = 32 heads (got C=%d heads=%d)", name, C, heads);
  if (ld_qkv % 8 || ld_out % 8 || ld_qkv < 3 * C || ld_out < C)
    return fail(BASD_ERR_SHAPE, "%s: row strides must be multiples of 8 with 3 C <= ld_qkv, C <= ld_out "
                "(got C=%d ld_qkv=%d ld_out=%d)", name, C, ld_qkv, ld_out);
  if (((uintptr_t)qkv | (uintptr_t)bias | (uintptr_t)out) & 15)
    return fail(BASD_ERR_SHAPE, "%s: 16-byte aligned buffers required", name);
  if (out == qkv) return fail(BASD_ERR_SHAPE, "%s: out must not alias qkv", name);
  problems = (int64_t)B * (H / ws) * (W / ws) * heads;
  grid = (problems + per_group - 1) / per_group;
  if (grid > 0x7fffffffLL) return fail(BASD_ERR_SHAPE, "%s: %lld workgroups", name, (long long)grid);
  return BASD_OK;
}

}  // namespace basd
