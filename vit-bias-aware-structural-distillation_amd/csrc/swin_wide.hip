// Window attention of the frozen Swin teacher trunk for windows of 9 x 9 to 16 x 16 slots (window 12 of the 384 px
// checkpoints; 16 for a later Swin-V2): what basd_window_attention_fwd_bf16 (csrc/swin.hip, one 64-slot tile per wave)
// refuses.  Layout, slot rule and everything behind the logits are that kernel's: window_attn.h.
//
//   basd_window_attention_fwd_wide_bf16   one workgroup of four waves per (window, head).  N = ws^2 <= 256 slots fill up
//                                         to sixteen 16-slot tiles.  The relative-position bias is read from timm's
//                                         TABLE [(2 ws - 1)^2, heads]: the head's column (at most 961 floats) is staged
//                                         in LDS and indexed per logit from the slot coordinates; no [N, N] image exists.
#include "window_attn.h"

namespace basd {

// Phase 0  every thread owns slot = threadIdx.x: its token row and its key word (mask label << 16 | iy (2 ws - 1) + ix)
//          go to LDS; the head's bias column is gathered into LDS.
// Phase 1  K and V of the head are staged once: 256 rows x 32 channels at the 40-element stride of swin.hip.  Rows behind
//          N are written as ZERO: the last 32-key step of P V is half empty when the tile count is odd (N = 144: nine
//          tiles, N = 100: seven) and an uninitialised V row times a zero probability may be NaN.  The Q fragment of
//          a query tile (the wave takes tiles wave, wave + 4, ...) comes straight from global memory, one tile ahead.
// Loop     a query tile's logits against all nt key tiles stay in registers (64 accumulators at most): one-pass softmax.
//   S^T = K Q^T   A = K rows from LDS (key 16 kt + (lane & 15), d = 8 (lane >> 4) ..), B = the Q fragment;
//   logits        the bias is table[qbase - koff[key]], a dead key is one whose key word is negative;
//                 qbase - koff = (iy_q - iy_k + ws - 1)(2 ws - 1) + (ix_q - ix_k + ws - 1)
// The loop runs (nt + 3) / 4 times in EVERY wave (a wave without a tile left only meets the barriers), so each barrier
// is reached by all four waves.  Dead slots (>= N) load nothing, are -3e38 as keys and are never stored as queries.
constexpr int WW_WAVES = 4;
constexpr int WW_SLOTS = 256;                         // ws <= 16
constexpr int WW_TILES = WW_SLOTS / 16;
constexpr int WW_TABLE = 31 * 31;                     // (2 ws - 1)^2 at ws = 16

__global__ __launch_bounds__(64 * WW_WAVES) void window_attention_wide_kernel(
    const unsigned short* __restrict__ qkv, const float* __restrict__ table, int H, int W, int heads, int C, int ws,
    int shift, int ld_qkv, int ld_out, float scale, unsigned short* __restrict__ out) {
  __shared__ __align__(16) unsigned short Ks[WW_SLOTS * WIN_LD];
  __shared__ __align__(16) unsigned short Vs[WW_SLOTS * WIN_LD];
  __shared__ __align__(16) unsigned short Os[WW_WAVES][16 * WIN_LD];
  __shared__ __align__(16) float tabS[WW_TABLE + 3];
  __shared__ __align__(16) int keyS[WW_SLOTS];
  __shared__ __align__(16) long long rowS[WW_SLOTS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int N = ws * ws, nt = (N + 15) >> 4;          // live slots, live 16-slot tiles
  const int tw = 2 * ws - 1;
  const int nwx = W / ws, nwy = H / ws;
  int h, wx, wy;
  int64_t b;
  {
    int64_t q = blockIdx.x;                           // the grid is exactly B nwy nwx heads: every workgroup is live
    h = (int)(q % heads);
    q /= heads;
    wx = (int)(q % nwx);
    q /= nwx;
    wy = (int)(q % nwy);
    b = q / nwy;
  }
  // ---- phase 0: slot = tid
  {
    const int iy = tid / ws, ix = tid - iy * ws;
    int64_t row = 0;
    int key = (int)0x80000000u;                                          // the sign bit marks a dead slot
    if (tid < N) {
      int lab;
      row = window_slot(tid, ws, wy, wx, b, H, W, shift, lab);
      key = (lab << 16) | (iy * tw + ix);
    }
    rowS[tid] = row;
    keyS[tid] = key;
    for (int i = tid; i < tw * tw; i += 64 * WW_WAVES) tabS[i] = table[(size_t)i * heads + h];
  }
  __syncthreads();

  // ---- phase 1: every global load of the thread is issued before its first LDS store
  const unsigned short* qhead = qkv + h * 32 + 8 * g;
  uint4 qnext = make_uint4(0, 0, 0, 0);               // Q fragment of the wave's first tile; the loop fetches one ahead
  int knext = keyS[16 * wave + li];
  if (16 * wave + li < N) qnext = *reinterpret_cast<const uint4*>(qhead + rowS[16 * wave + li] * ld_qkv);
  {
    uint4 kf[4], vf[4];
    const int c8 = tid & 3;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int slot = (tid >> 2) + 64 * i;
      kf[i] = vf[i] = make_uint4(0, 0, 0, 0);
      if (slot < N) {
        const unsigned short* p = qkv + rowS[slot] * ld_qkv + C + h * 32 + 8 * c8;
        kf[i] = *reinterpret_cast<const uint4*>(p);
        vf[i] = *reinterpret_cast<const uint4*>(p + C);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int slot = (tid >> 2) + 64 * i;
      *reinterpret_cast<uint4*>(Ks + slot * WIN_LD + 8 * c8) = kf[i];
      *reinterpret_cast<uint4*>(Vs + slot * WIN_LD + 8 * c8) = vf[i];
    }
  }
  __syncthreads();

  unsigned short* Ow = Os[wave];
  const int cbase = (ws - 1) * tw + ws - 1;
  const int npad = (ld_out - C) >> 3;                 // 16-byte zero vectors behind the C channels of an output row
  const int iters = (nt + WW_WAVES - 1) / WW_WAVES;   // the same in every wave
  for (int it = 0; it < iters; ++it) {
    const int qt = wave + WW_WAVES * it;
    const bool active = qt < nt;                      // wave-uniform
    const uint4 qq = qnext;
    const int qk = knext;
    {
      const int slot = 16 * (qt + WW_WAVES) + li;     // the wave's next tile: behind N when there is none
      qnext = make_uint4(0, 0, 0, 0);
      if (slot < N) {
        knext = keyS[slot];
        qnext = *reinterpret_cast<const uint4*>(qhead + rowS[slot] * ld_qkv);
      }
    }
    if (active) {
      const int ql = qk >> 16, qb = cbase + (qk & 0xffff);
      float s[WW_TILES][4];
      float mx = -3.0e38f;
#pragma unroll
      for (int kt = 0; kt < WW_TILES; ++kt) {
        if (kt < nt) {
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              *reinterpret_cast<const bf16x8*>(Ks + (16 * kt + li) * WIN_LD + 8 * g), *reinterpret_cast<const bf16x8*>(&qq),
              acc, 0, 0, 0);
          const int4 kk4 = *reinterpret_cast<const int4*>(keyS + 16 * kt + 4 * g);
          const int kk[4] = {kk4.x, kk4.y, kk4.z, kk4.w};
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float l = fmaf(acc[r], scale, tabS[qb - (kk[r] & 0xffff)]);
            if ((kk[r] >> 16) != ql) l += -100.0f;
            if (kk[r] < 0) l = -3.0e38f;                                 // dead key, from the word and not from a compare
                                                                         // against N: that one is loop invariant, and
                                                                         // 64 hoisted lane masks do not fit the SGPRs
            s[kt][r] = l;
            mx = fmaxf(mx, l);
          }
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) s[kt][r] = -3.0e38f;
        }
      }
      const float inv = window_softmax<WW_TILES, true>(s, mx, nt);
      f32x4 o[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
      window_pv<WW_TILES>(s, inv, Vs, nt, lane, o);
      window_tile_to_lds(o, Ow, lane);
    }
    __syncthreads();
    if (active) {
      const int slot = 16 * qt + (lane >> 2);
      if (slot < N) window_store_row(out, rowS[slot], ld_out, Ow, h, heads, C, npad, lane);
    }
    __syncthreads();
  }
}

}  // namespace basd

extern "C" int basd_window_attention_fwd_wide_bf16(const void* qkv, const float* table, int B, int H, int W, int heads,
                                                   int C, int ws, int shift, int ld_qkv, int ld_out, float scale,
                                                   void* out, void* stream) {
  using namespace basd;
  if (B <= 0) return BASD_OK;
  int64_t problems, grid;                               // one problem per workgroup: every workgroup is live
  if (int rc = window_attention_check("window_attention_fwd_wide", 9, 16, qkv, table, out, B, H, W, heads, C, ws, shift,
                                      ld_qkv, ld_out, 1, problems, grid))
    return rc;
  hipLaunchKernelGGL(window_attention_wide_kernel, dim3((unsigned)grid), dim3(64 * WW_WAVES), 0, (hipStream_t)stream,
                     (const unsigned short*)qkv, table, H, W, heads, C, ws, shift, ld_qkv, ld_out, scale,
                     (unsigned short*)out);
  return check_launch("window_attention_fwd_wide");
}
