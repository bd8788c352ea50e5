// Window attention of the frozen Swin teacher trunk for windows of 9 x 9 to 16 x 16 slots (window 12 of the 384 px
// checkpoints; 16 for a later Swin-V2): what basd_window_attention_fwd_bf16 (csrc/swin.hip, one 64-slot tile per wave)
// refuses.  Same rows, same index arithmetic for the roll and the partition, same label mask, same rounding points.
//
//   basd_window_attention_fwd_wide_bf16   one workgroup of four waves per (window, head).  N = ws^2 <= 256 slots fill up
//                                         to sixteen 16-slot tiles.  The relative-position bias is read from timm's
//                                         TABLE [(2 ws - 1)^2, heads]: the head's column (at most 961 floats) is staged
//                                         in LDS and indexed per logit from the slot coordinates; no [N, N] image exists.
#include "basd_frag.h"

namespace basd {

// Phase 0  every thread owns slot = threadIdx.x: its token row and its key word (mask label << 16 | iy (2 ws - 1) + ix)
//          go to LDS; the head's bias column is gathered into LDS.
// Phase 1  K and V of the head are staged once: 256 rows x 32 channels at the 40-element stride of swin.hip.  Rows behind
//          N are written as ZERO: the last 32-key step of P V is half empty when the tile count is odd (N = 144: nine
//          tiles, N = 100: seven) and an uninitialised V row times a zero probability may be NaN.  The Q fragment of
//          a query tile (the wave takes tiles wave, wave + 4, ...) comes straight from global memory, one tile ahead.
// Loop     a query tile's logits against all nt key tiles stay in registers (64 accumulators at most): one-pass softmax.
//   S^T = K Q^T   A = K rows from LDS (key 16 kt + (lane & 15), d = 8 (lane >> 4) ..), B = the Q fragment:
//                 accumulator of key tile kt: keys 16 kt + 4 (lane >> 4) + {0..3}, query 16 qt + (lane & 15);
//   logits        fmaf(s, scale, table[qbase - koff[key]]) + (label[query] != label[key] ? -100 : 0), keys >= N -3e38;
//                 qbase - koff = (iy_q - iy_k + ws - 1)(2 ws - 1) + (ix_q - ix_k + ws - 1)
//   softmax       fp32 over the registers and the four lane groups of a query column (xor 16, 32);
//   O = P V       the accumulators of a 32-key step are the A fragment, B = V through the transposing LDS read;
//   the 16 x 32 output tile goes through the wave's LDS tile so that every lane stores 16 contiguous bytes.
// The loop runs (nt + 3) / 4 times in EVERY wave (a wave without a tile left only meets the barriers), so each barrier
// is reached by all four waves.  Dead slots (>= N) load nothing, are -3e38 as keys and are never stored as queries.
constexpr int WW_WAVES = 4;
constexpr int WW_LD = 40;                             // LDS row stride in bf16: 32 + 8 (16-byte aligned, bank rotation)
constexpr int WW_SLOTS = 256;                         // ws <= 16
constexpr int WW_TILES = WW_SLOTS / 16;
constexpr int WW_TABLE = 31 * 31;                     // (2 ws - 1)^2 at ws = 16

__global__ __launch_bounds__(64 * WW_WAVES) void window_attention_wide_kernel(
    const unsigned short* __restrict__ qkv, const float* __restrict__ table, int H, int W, int heads, int C, int ws,
    int shift, int ld_qkv, int ld_out, float scale, unsigned short* __restrict__ out) {
  __shared__ __align__(16) unsigned short Ks[WW_SLOTS * WW_LD];
  __shared__ __align__(16) unsigned short Vs[WW_SLOTS * WW_LD];
  __shared__ __align__(16) unsigned short Os[WW_WAVES][16 * WW_LD];
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
      const int ry = wy * ws + iy, rx = wx * ws + ix;                    // coordinate in the rolled grid
      int y = ry + shift, x = rx + shift;
      if (y >= H) y -= H;
      if (x >= W) x -= W;
      row = (b * H + y) * (int64_t)W + x;
      int lab = 0;
      if (shift > 0) {                                                   // slices [0, -ws), [-ws, -shift), [-shift, end)
        const int ly = ry < H - ws ? 0 : (ry < H - shift ? 1 : 2);
        const int lx = rx < W - ws ? 0 : (rx < W - shift ? 1 : 2);
        lab = 3 * ly + lx;
      }
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
      *reinterpret_cast<uint4*>(Ks + slot * WW_LD + 8 * c8) = kf[i];
      *reinterpret_cast<uint4*>(Vs + slot * WW_LD + 8 * c8) = vf[i];
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
              *reinterpret_cast<const bf16x8*>(Ks + (16 * kt + li) * WW_LD + 8 * g), *reinterpret_cast<const bf16x8*>(&qq),
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
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      float sum = 0.f;
#pragma unroll
      for (int kt = 0; kt < WW_TILES; ++kt) {
        if (kt < nt) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float p = __builtin_amdgcn_exp2f((s[kt][r] - mx) * 1.4426950408889634f);   // dead keys: exp2(-huge) = 0
            s[kt][r] = p;
            sum += p;
          }
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) s[kt][r] = 0.f;                    // the empty half of the last 32-key step
        }
      }
      sum += __shfl_xor(sum, 16, 64);
      sum += __shfl_xor(sum, 32, 64);
      const float inv = 1.f / sum;
      // ---- O = P V over up to eight 32-key steps
      f32x4 o[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int ks = 0; ks < WW_TILES / 2; ++ks) {
        if (2 * ks < nt) {
          uint4 pw;
          pw.x = pack_bf16(s[2 * ks][0] * inv, s[2 * ks][1] * inv);
          pw.y = pack_bf16(s[2 * ks][2] * inv, s[2 * ks][3] * inv);
          pw.z = pack_bf16(s[2 * ks + 1][0] * inv, s[2 * ks + 1][1] * inv);
          pw.w = pack_bf16(s[2 * ks + 1][2] * inv, s[2 * ks + 1][3] * inv);
          const bf16x8 pa = *reinterpret_cast<const bf16x8*>(&pw);
#pragma unroll
          for (int dt = 0; dt < 2; ++dt)
            o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, tr_split(Vs, WW_LD, 32 * ks + 4 * g, 16 * dt, lane), o[dt],
                                                            0, 0, 0);
        }
      }
      // ---- o[dt][r] = O[query 16 qt + 4 g + r][d = 16 dt + li]: through LDS, then one 16-byte store per lane
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 4; r += 2) {
          const unsigned int w2 = pack_bf16(o[dt][r], o[dt][r + 1]);
          Ow[(4 * g + r) * WW_LD + 16 * dt + li] = (unsigned short)(w2 & 0xffffu);
          Ow[(4 * g + r + 1) * WW_LD + 16 * dt + li] = (unsigned short)(w2 >> 16);
        }
    }
    __syncthreads();
    if (active) {
      const int r = lane >> 2, c8 = lane & 3, slot = 16 * qt + r;
      if (slot < N) {
        unsigned short* orow = out + rowS[slot] * ld_out;
        *reinterpret_cast<uint4*>(orow + h * 32 + c8 * 8) = *reinterpret_cast<const uint4*>(Ow + r * WW_LD + c8 * 8);
        for (int j = h * 4 + c8; j < npad; j += heads * 4)               // the pad columns, shared out over the heads
          *reinterpret_cast<uint4*>(orow + C + j * 8) = make_uint4(0, 0, 0, 0);
      }
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
  if (ws < 9 || ws > 16 || shift < 0 || shift >= ws)
    return fail(BASD_ERR_SHAPE, "window_attention_fwd_wide: 9 <= ws <= 16 and 0 <= shift < ws (got ws=%d shift=%d)", ws,
                shift);
  if (H < ws || W < ws || H % ws || W % ws)
    return fail(BASD_ERR_SHAPE, "window_attention_fwd_wide: H and W must be multiples of ws (got %d x %d, ws=%d)", H, W, ws);
  if (heads < 1 || C != 32 * heads)
    return fail(BASD_ERR_SHAPE, "window_attention_fwd_wide: head dim 32 only, C = 32 heads (got C=%d heads=%d)", C, heads);
  if (ld_qkv % 8 || ld_out % 8 || ld_qkv < 3 * C || ld_out < C)
    return fail(BASD_ERR_SHAPE, "window_attention_fwd_wide: row strides must be multiples of 8 with 3 C <= ld_qkv, "
                "C <= ld_out (got C=%d ld_qkv=%d ld_out=%d)", C, ld_qkv, ld_out);
  if (((uintptr_t)qkv | (uintptr_t)table | (uintptr_t)out) & 15)
    return fail(BASD_ERR_SHAPE, "window_attention_fwd_wide: 16-byte aligned buffers required");
  if (out == qkv) return fail(BASD_ERR_SHAPE, "window_attention_fwd_wide: out must not alias qkv");
  const int64_t grid = (int64_t)B * (H / ws) * (W / ws) * heads;
  if (grid > 0x7fffffffLL) return fail(BASD_ERR_SHAPE, "window_attention_fwd_wide: %lld workgroups", (long long)grid);
  hipLaunchKernelGGL(window_attention_wide_kernel, dim3((unsigned)grid), dim3(64 * WW_WAVES), 0, (hipStream_t)stream,
                     (const unsigned short*)qkv, table, H, W, heads, C, ws, shift, ld_qkv, ld_out, scale,
                     (unsigned short*)out);
  return check_launch("window_attention_fwd_wide");
}
