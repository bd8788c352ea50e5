// Token assembly of a ViT in front of block 0, one launch:
//     out[b, t, :] = LN( bf16( src(b, t) + pos[t] ) ),   src = cls for t = 0 (when the model has a CLS token), else the
//                                                         patch-embedding row
// i.e. timm's _pos_embed (cat of the expanded CLS token and the patch rows, + pos_embed) followed by CLIP's norm_pre.
// As torch ops on bf16 that is cat + add + layer_norm: three kernels and two more copies of [B, T, D].  Here every row
// is read once and written once; with gamma == NULL the LayerNorm is left out and the result is the plain assembly.
//
// Arithmetic: the sum is taken in fp32 and rounded to bf16 (what torch's bf16 add gives), the LayerNorm is the one of
// layernorm.hip on that rounded row -- same row ownership (G lanes of a wave, NCH chunks of 8 columns per lane), same
// reduction (group_allsum), two-pass fp32 statistics, one rounding at the store -- so the output equals
// basd_layernorm_fwd_bf16 of the torch-assembled tensor bit for bit.
// Register tokens (DINOv2 "_reg" models, basd_vit_embed_reg_bf16): R learned rows stand between the CLS row and the
// patch rows and take NO position embedding -- out[b, 1 + r] = reg[r], out[b, 1 + R + n] = patches[b, n] + pos[1 + n],
// pos keeps its 1 + N rows.  The same kernel body: a register row adds -0.0 instead of a position row (x + -0.0 == x
// for every x, a negative zero included, so the row passes through the fp32 add and the rounding bit for bit), and
// with R = 0 no row takes that branch: basd_vit_embed_bf16 is this kernel with R = 0.
// Access: 16 bytes per lane when every pointer is 16-byte aligned (D % 8 == 0 makes every row pitch a multiple of 16
// bytes, so the bases decide), else the same chunks element by element (views that start at an odd offset).
#include "basd_frag.h"

namespace basd {

template <bool WIDE>
__device__ __forceinline__ uint4 embed_load8(const unsigned short* p) {
  if (WIDE) return *reinterpret_cast<const uint4*>(p);
  return make_uint4(p[0] | ((unsigned int)p[1] << 16), p[2] | ((unsigned int)p[3] << 16),
                    p[4] | ((unsigned int)p[5] << 16), p[6] | ((unsigned int)p[7] << 16));
}

template <bool WIDE>
__device__ __forceinline__ void embed_store8(unsigned short* p, const uint4& v) {
  if (WIDE) { *reinterpret_cast<uint4*>(p) = v; return; }
  const unsigned int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    p[2 * i] = (unsigned short)(w[i] & 0xffffu);
    p[2 * i + 1] = (unsigned short)(w[i] >> 16);
  }
}

// U rows per group in flight, as in ln_fwd_kernel
template <int G, int NCH, bool LN, bool WIDE, int U>
__global__ __launch_bounds__(256) void vit_embed_kernel(const unsigned short* __restrict__ patches,
                                                        const unsigned short* __restrict__ cls,
                                                        const unsigned short* __restrict__ reg, int R,
                                                        const unsigned short* __restrict__ pos,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        float eps, int64_t rows, int N, int T, int D,
                                                        unsigned short* __restrict__ out) {
  constexpr int RPW = 64 / G;                       // rows per wave
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lg = lane & (G - 1), sub = lane / G;
  const int nchunk = D >> 3;
  const int has_cls = cls != nullptr;
  float g[NCH][8], b[NCH][8];
  if (LN) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int ch = lg + c * G;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        g[c][i] = ch < nchunk ? gamma[ch * 8 + i] : 0.f;
        b[c][i] = ch < nchunk ? beta[ch * 8 + i] : 0.f;
      }
    }
  }
  const float inv_d = 1.f / (float)D;
  const int64_t wstride = (int64_t)gridDim.x * 4 * RPW;
  for (int64_t r0 = ((int64_t)blockIdx.x * 4 + wave) * RPW + sub; r0 < rows; r0 += wstride * U) {
    uint4 xv[U][NCH], pv[U][NCH];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t r = r0 + u * wstride;
      const int64_t smp = r / T;
      const int t = (int)(r - smp * T);
      // rows beyond the end load nothing; a CLS row reads the [D] token, a register row (has_cls <= t < has_cls + R)
      // its [D] row of reg and no position row, every other row its patch row and the position row t - R
      const bool is_reg = t >= has_cls && t < has_cls + R;
      const unsigned short* src = (has_cls && t == 0) ? cls
                                  : is_reg ? reg + (int64_t)(t - has_cls) * D
                                           : patches + (smp * N + (t - has_cls - R)) * D;
      const int tp = t < has_cls + R ? t : t - R;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int ch = lg + c * G;
        xv[u][c] = make_uint4(0, 0, 0, 0);
        pv[u][c] = make_uint4(0, 0, 0, 0);
        if (ch < nchunk && r < rows) {
          xv[u][c] = embed_load8<WIDE>(src + ch * 8);
          pv[u][c] = is_reg ? make_uint4(0x80008000u, 0x80008000u, 0x80008000u, 0x80008000u)
                            : embed_load8<WIDE>(pos + (int64_t)tp * D + ch * 8);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t r = r0 + u * wstride;
      const bool live = r < rows;
      float f[NCH][8];
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        float fp[8];
        unpack8(xv[u][c], f[c]);
        unpack8(pv[u][c], fp);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          f[c][i] = round_bf16(f[c][i] + fp[i]);
          s += f[c][i];
        }
      }
      if (!LN) {
        if (live) {
#pragma unroll
          for (int c = 0; c < NCH; ++c) {
            const int ch = lg + c * G;
            if (ch < nchunk) embed_store8<WIDE>(out + r * D + ch * 8, pack8(f[c]));
          }
        }
        continue;
      }
      const float mu = group_allsum<G>(s) * inv_d;
      float q = 0.f;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int ch = lg + c * G;
        if (ch < nchunk) {
#pragma unroll
          for (int i = 0; i < 8; ++i) { const float d = f[c][i] - mu; q = fmaf(d, d, q); }   // two-pass variance
        }
      }
      const float rs = rsqrtf(group_allsum<G>(q) * inv_d + eps);
      if (live) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const int ch = lg + c * G;
          if (ch < nchunk) {
            float o[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) o[i] = fmaf((f[c][i] - mu) * rs, g[c][i], b[c][i]);
            embed_store8<WIDE>(out + r * D + ch * 8, pack8(o));
          }
        }
      }
    }
  }
}

template <bool LN, bool WIDE>
static int launch_vit_embed(const unsigned short* patches, const unsigned short* cls, const unsigned short* reg, int R,
                            const unsigned short* pos,
                            const float* gamma, const float* beta, float eps, int64_t rows, int N, int T, int D,
                            unsigned short* out, hipStream_t st, const char* what) {
  const int nchunk = D / 8;
  auto grid = [&](int rows_per_wg) {
    const int64_t g = (rows + rows_per_wg - 1) / rows_per_wg;
    return (int)(g > 2048 ? 2048 : g);
  };
  // the (G, NCH, U) table of launch_ln_fwd: the row ownership decides the summation order
#define BASD_VIT_EMBED(G, NCH, U)                                                                                  \
  hipLaunchKernelGGL((vit_embed_kernel<G, NCH, LN, WIDE, U>), dim3(grid(4 * (64 / G) * U)), dim3(256), 0, st, patches, \
                     cls, reg, R, pos, gamma, beta, eps, rows, N, T, D, out)
  if (nchunk <= 32) BASD_VIT_EMBED(32, 1, 4);
  else if (nchunk <= 64) BASD_VIT_EMBED(64, 1, 4);
  else if (nchunk <= 128) BASD_VIT_EMBED(64, 2, 2);
  else if (nchunk <= 192) BASD_VIT_EMBED(64, 3, 1);
  else BASD_VIT_EMBED(64, 4, 1);
#undef BASD_VIT_EMBED
  return check_launch(what);
}

}  // namespace basd

// both entries; `what` names the caller in the messages
static int vit_embed_entry(const char* what, const void* patches, const void* cls, const void* reg, int R,
                           const void* pos, const float* gamma, const float* beta, float eps, int B, int N, int D,
                           void* out, void* stream) {
  using namespace basd;
  if (D % 8 || D < 8 || D > 2048) return fail(BASD_ERR_SHAPE, "%s: D %% 8 != 0 or D outside 8 .. 2048 (%d)", what, D);
  if (R < 0 || (R > 0 && (cls == nullptr || reg == nullptr)))
    return fail(BASD_ERR_SHAPE, "%s: R = %d register rows need R >= 0, a CLS token and reg", what, R);
  const int64_t T = (int64_t)N + R + (cls != nullptr ? 1 : 0);
  if (B < 0 || N < 0 || T < 1) return fail(BASD_ERR_SHAPE, "%s: B = %d, N = %d and no CLS token: no rows", what, B, N);
  if (T > 0x7fffffff) return fail(BASD_ERR_SHAPE, "%s: N + R = %lld rows per image", what, (long long)T);
  if ((gamma == nullptr) != (beta == nullptr)) return fail(BASD_ERR_SHAPE, "%s: gamma and beta go together", what);
  if (pos == nullptr || out == nullptr || (patches == nullptr && N > 0))
    return fail(BASD_ERR_SHAPE, "%s: null patches / pos / out", what);
  if (B == 0) return BASD_OK;
  const int64_t rows = (int64_t)B * T;
  const uintptr_t p0 = (uintptr_t)patches, p1 = p0 + (uintptr_t)B * N * D * 2;
  const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (uintptr_t)rows * D * 2;
  if (N > 0 && p0 < o1 && o0 < p1) return fail(BASD_ERR_SHAPE, "%s: out overlaps patches", what);
  const bool wide = (((uintptr_t)patches | (uintptr_t)cls | (uintptr_t)reg | (uintptr_t)pos | (uintptr_t)out) & 15) == 0;
  const unsigned short* pp = (const unsigned short*)patches;
  const unsigned short* cp = (const unsigned short*)cls;
  const unsigned short* rp = (const unsigned short*)reg;
  const unsigned short* sp = (const unsigned short*)pos;
  unsigned short* op = (unsigned short*)out;
  hipStream_t st = (hipStream_t)stream;
  const int t = (int)T;
  if (gamma != nullptr)
    return wide ? launch_vit_embed<true, true>(pp, cp, rp, R, sp, gamma, beta, eps, rows, N, t, D, op, st, what)
                : launch_vit_embed<true, false>(pp, cp, rp, R, sp, gamma, beta, eps, rows, N, t, D, op, st, what);
  return wide ? launch_vit_embed<false, true>(pp, cp, rp, R, sp, gamma, beta, eps, rows, N, t, D, op, st, what)
              : launch_vit_embed<false, false>(pp, cp, rp, R, sp, gamma, beta, eps, rows, N, t, D, op, st, what);
}

extern "C" int basd_vit_embed_bf16(const void* patches, const void* cls, const void* pos, const float* gamma,
                                   const float* beta, float eps, int B, int N, int D, void* out, void* stream) {
  return vit_embed_entry("vit_embed_bf16", patches, cls, nullptr, 0, pos, gamma, beta, eps, B, N, D, out, stream);
}

extern "C" int basd_vit_embed_reg_bf16(const void* patches, const void* cls, const void* reg, int R, const void* pos,
                                       const float* gamma, const float* beta, float eps, int B, int N, int D, void* out,
                                       void* stream) {
  // R = 0: reg is not read (and does not take part in the alignment test)
  return vit_embed_entry("vit_embed_reg_bf16", patches, cls, R > 0 ? reg : nullptr, R, pos, gamma, beta, eps, B, N, D,
                         out, stream);
}
