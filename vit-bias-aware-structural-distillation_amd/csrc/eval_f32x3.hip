// fp32 evaluation forward of the ViT on split-bf16 ("bf16x3") products: what torch.set_float32_matmul_precision("high")
// asks of an fp32 matmul (reference src/training/trainer.py:183-188, src/train.py:153-160, src/eval.py:16) on a GPU
// without xf32 MFMA forms (gfx950 dropped CDNA3's; its fp32 MFMA runs at 1/16 of the bf16 rate).
//
// Every fp32 operand v is carried as the SPLIT IMAGE (hi | lo): hi = bf16_rne(v), lo = bf16_rne(v - hi), the two halves
// side by side in one bf16 row of 2 Kp elements (zero columns up to a padded Kp).  A product x w is
//     x_hi w_hi + x_hi w_lo + x_lo w_hi          (three v_mfma_f32_16x16x32_bf16, fp32 accumulation)
// i.e. ~16 significand bits per product at 3/16 of the cost of the fp32 MFMA.  Producers of GEMM inputs (the patch
// unfold, the LayerNorm, the attention, the fc1 epilogue) write the image directly: there is no split pass over
// activations.
//
//   split_table_kernel    fp32 weight matrices -> images, all layers of a model in one launch
//   split_patches_kernel  [B, C, H, W] fp32 image batch -> unfolded patch rows (the stride-p convolution as a GEMM)
//   gemm_f32x3_kernel     y = epi(x w^T + bias): fp32 out, exact-erf GELU, or the image of either for the next GEMM
//   attn_f32x3_kernel     softmax(q k^T scale) v per (batch, head, 128 queries) from the packed fp32 qkv projection;
//                         fp32 logits (no bf16 rounding), fp32 softmax, P split against V split; T <= 272
//   attn_f32x3_long_kernel  the same arithmetic tiled over key blocks of 128 with an online softmax: 1 <= T <= 1024
//   ln_f32_kernel         s = residual + gamma_ls x (optional), y = LayerNorm(s): fp32 s, fp32 y and / or the image
#include "basd_frag.h"

namespace basd {

// (hi, lo) of one fp32 value
__device__ __forceinline__ void ev_split(float v, unsigned short& hi, unsigned short& lo) {
  hi = f32_to_bf16_bits(v);
  lo = f32_to_bf16_bits(v - bf16_bits_to_f32(hi));
}

// hi / lo halves of four values as two 8-byte words
__device__ __forceinline__ void ev_split4(const float (&v)[4], uint2& hi, uint2& lo) {
  unsigned short h[4], l[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) ev_split(v[i], h[i], l[i]);
  hi = make_uint2(h[0] | ((unsigned int)h[1] << 16), h[2] | ((unsigned int)h[3] << 16));
  lo = make_uint2(l[0] | ((unsigned int)l[1] << 16), l[2] | ((unsigned int)l[3] << 16));
}

__device__ __forceinline__ float ev_gelu(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752f)); }

// ------------------------------------------------------------------------------------------------------------------
// Weight images.  Entry e: fp32 [rows, k] at src -> bf16 [rows, 2 kp] at dst; 1024 elements of one entry per workgroup.
constexpr int ST_MAX = 64;
struct SplitTable {
  int64_t src[ST_MAX], dst[ST_MAX];
  int rows[ST_MAX], k[ST_MAX], kp[ST_MAX], blk0[ST_MAX + 1];
  int n;
};

__global__ __launch_bounds__(256) void split_table_kernel(SplitTable t) {
  const int b = blockIdx.x;
  int e = 0;
  while (e + 1 < t.n && b >= t.blk0[e + 1]) ++e;
  const int k = t.k[e], kp = t.kp[e];
  const int64_t total = (int64_t)t.rows[e] * kp;
  const float* src = reinterpret_cast<const float*>(t.src[e]);
  unsigned short* dst = reinterpret_cast<unsigned short*>(t.dst[e]);
  const int64_t base = (int64_t)(b - t.blk0[e]) * 1024;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t idx = base + threadIdx.x + 256 * i;
    if (idx >= total) break;
    const int64_t r = idx / kp;
    const int c = (int)(idx - r * kp);
    unsigned short hi = 0, lo = 0;
    if (c < k) ev_split(src[r * k + c], hi, lo);
    dst[r * 2 * kp + c] = hi;
    dst[r * 2 * kp + kp + c] = lo;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Patch rows: out[(b Np + py Wp + px)][c p p + i p + j] = x[b][c][py p + i][px p + j], zero for k >= C p p.
__global__ __launch_bounds__(256) void split_patches_kernel(const float* __restrict__ x, int C, int H, int W, int p,
                                                            int kp, int64_t total, unsigned short* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int64_t row = idx / kp;
  const int k = (int)(idx - row * kp);
  const int hp = H / p, wp = W / p, np = hp * wp;
  const int64_t b = row / np;
  const int pr = (int)(row - b * np), py = pr / wp, px = pr - py * wp;
  unsigned short hi = 0, lo = 0;
  if (k < C * p * p) {
    const int c = k / (p * p), ij = k - c * p * p, i = ij / p, j = ij - i * p;
    ev_split(x[((b * C + c) * H + py * p + i) * W + px * p + j], hi, lo);
  }
  out[row * 2 * kp + k] = hi;
  out[row * 2 * kp + kp + k] = lo;
}

// ------------------------------------------------------------------------------------------------------------------
// GEMM.  Workgroup = 4 waves, output tile 128 (n) x 128 (m), K step 32.  The four operand tiles of a step (W hi, W lo,
// X hi, X lo: [128 rows][32 k] each) go global -> registers (one step ahead) -> LDS (rows padded to 40 elements: the
// 16-byte fragment reads of 16 rows fall on distinct banks), two LDS stages: one barrier per K step.  Wave (wn, wm) owns 64 n x 64 m = 4 x 4 accumulator tiles;
// the MFMA takes the WEIGHT fragment as A and the activation as B, so a lane holds 4 consecutive n of one row m: one
// 16-byte fp32 store (or two 8-byte image stores) per tile.  Rows m >= M and n >= N load as zero and are not stored.
constexpr int EG_LD = 40;
constexpr int EG_TILE = 128 * EG_LD;                  // one operand tile in LDS (bf16 elements)
constexpr int EG_LDS = 2 * 4 * EG_TILE * 2;           // bytes: two stages (80 KiB: two workgroups per CU)

__device__ __forceinline__ uint4 eg_keep(uint4 v, bool ok) {
  return make_uint4(ok ? v.x : 0u, ok ? v.y : 0u, ok ? v.z : 0u, ok ? v.w : 0u);
}

template <bool GELU, bool SPLIT>
__global__ __launch_bounds__(256) void gemm_f32x3_kernel(const unsigned short* __restrict__ X,
                                                         const unsigned short* __restrict__ W,
                                                         const float* __restrict__ bias, void* __restrict__ Y, int M,
                                                         int N, int kp) {
  extern __shared__ __align__(16) unsigned short eg_sm[];         // 2 stages x {W hi, W lo, X hi, X lo}
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int wn = wave & 1, wm = wave >> 1;
  const int n0 = blockIdx.x * 128, m0 = blockIdx.y * 128;
  const size_t pitch = 2 * (size_t)kp;

  uint4 pre[8];
#define EG_LOAD(k0)                                                                              \
  _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                                \
    const int c = tid + 256 * i, r = c >> 2, q = c & 3;                                          \
    const bool okw = n0 + r < N, okx = m0 + r < M;                                               \
    /* rows past the end load row 0 (always valid) and are zeroed by value, not by address */   \
    const unsigned short* wp = W + (size_t)(okw ? n0 + r : 0) * pitch + (k0) + 8 * q;            \
    const unsigned short* xp = X + (size_t)(okx ? m0 + r : 0) * pitch + (k0) + 8 * q;            \
    pre[4 * i + 0] = eg_keep(*reinterpret_cast<const uint4*>(wp), okw);                          \
    pre[4 * i + 1] = eg_keep(*reinterpret_cast<const uint4*>(wp + kp), okw);                     \
    pre[4 * i + 2] = eg_keep(*reinterpret_cast<const uint4*>(xp), okx);                          \
    pre[4 * i + 3] = eg_keep(*reinterpret_cast<const uint4*>(xp + kp), okx);                     \
  }

  f32x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int nk = kp / 32;
  EG_LOAD(0)
  for (int t = 0; t < nk; ++t) {
    // stage t & 1: the barrier of step t - 1 already ordered every read of this stage (step t - 2) before these stores
    unsigned short* sm = eg_sm + (t & 1) * 4 * EG_TILE;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = tid + 256 * i, r = c >> 2, q = c & 3;
#pragma unroll
      for (int s = 0; s < 4; ++s) *reinterpret_cast<uint4*>(sm + s * EG_TILE + r * EG_LD + 8 * q) = pre[4 * i + s];
    }
    __syncthreads();
    if (t + 1 < nk) {
      EG_LOAD(32 * (t + 1))
    }
    bf16x8 wh[4], wl[4], xh[4], xl[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int rw = (wn * 64 + a * 16 + li) * EG_LD + 8 * g, rx = (wm * 64 + a * 16 + li) * EG_LD + 8 * g;
      wh[a] = *reinterpret_cast<const bf16x8*>(sm + rw);
      wl[a] = *reinterpret_cast<const bf16x8*>(sm + EG_TILE + rw);
      xh[a] = *reinterpret_cast<const bf16x8*>(sm + 2 * EG_TILE + rx);
      xl[a] = *reinterpret_cast<const bf16x8*>(sm + 3 * EG_TILE + rx);
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl[a], xh[b], acc[a][b], 0, 0, 0);
        acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[a], xl[b], acc[a][b], 0, 0, 0);
        acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[a], xh[b], acc[a][b], 0, 0, 0);
      }
  }
#undef EG_LOAD

  // acc[a][b][r] = Y[m = m0 + wm 64 + 16 b + li][n = n0 + wn 64 + 16 a + 4 g + r]
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int n = n0 + wn * 64 + 16 * a + 4 * g;
    const bool okn = n < N;
    float4 b4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (bias != nullptr && okn) b4 = *reinterpret_cast<const float4*>(bias + n);
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int m = m0 + wm * 64 + 16 * b + li;
      float v0 = acc[a][b][0] + b4.x, v1 = acc[a][b][1] + b4.y, v2 = acc[a][b][2] + b4.z, v3 = acc[a][b][3] + b4.w;
      if (GELU) {
        v0 = ev_gelu(v0); v1 = ev_gelu(v1); v2 = ev_gelu(v2); v3 = ev_gelu(v3);
      }
      if (okn && m < M) {
        if constexpr (SPLIT) {
          unsigned short h0, h1, h2, h3, l0, l1, l2, l3;
          ev_split(v0, h0, l0); ev_split(v1, h1, l1); ev_split(v2, h2, l2); ev_split(v3, h3, l3);
          unsigned short* y = reinterpret_cast<unsigned short*>(Y) + (size_t)m * 2 * N + n;
          *reinterpret_cast<uint2*>(y) = make_uint2(h0 | ((unsigned int)h1 << 16), h2 | ((unsigned int)h3 << 16));
          *reinterpret_cast<uint2*>(y + N) = make_uint2(l0 | ((unsigned int)l1 << 16), l2 | ((unsigned int)l3 << 16));
        } else {
          *reinterpret_cast<float4*>(reinterpret_cast<float*>(Y) + (size_t)m * N + n) = make_float4(v0, v1, v2, v3);
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Attention.  Workgroup = 8 waves = 8 query tiles of 16 of one (batch, head); grid (B H, ceil(T / 128)).  The K and V
// images of the head do not both fit in LDS at hd 80 (226 KB at T = 272), so the kernel runs in two phases over ONE
// buffer: K (hi, lo) staged -> S^T = K Q^T for the wave's tile (NKT x 4 fp32 registers per lane) -> barrier -> V (hi, lo)
// staged over K -> O = P V.  Fragment layouts as csrc/attention.hip: the S^T accumulator of key tile kt holds, for
// query column lane & 15, the keys 16 kt + 4 (lane >> 4) + {0..3}; two of them are the A fragment of a 32-key step of
// P V, B = V through ds_read_tr16_b64 on the same eight keys.  Logits scaled in fp32, softmax in fp32, P unnormalised
// (in (0, 1]) split into (hi, lo); the 1 / sum is applied to the fp32 output.
template <int NKT, int HD>
__global__ __launch_bounds__(512) void attn_f32x3_kernel(const float* __restrict__ qkv, int T, int H, float scale,
                                                         unsigned short* __restrict__ out) {
  constexpr int NKS = (NKT + 1) / 2;
  constexpr int KROWS = 32 * NKS;
  constexpr int NDS = (HD + 31) / 32;
  constexpr int NDT = HD / 16;
  constexpr int LD = NDS * 32 + 8;
  constexpr int NC4 = NDS * 8;                       // 4-float chunks of a padded row
  extern __shared__ __align__(16) unsigned short sm[];
  unsigned short* Sh = sm;                            // [KROWS][LD] hi
  unsigned short* Sl = sm + KROWS * LD;               // [KROWS][LD] lo
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int b = blockIdx.x / H, h = blockIdx.x - b * H;
  const int C = H * HD;
  const size_t row = (size_t)3 * C;
  const float* base = qkv + (size_t)b * T * row + (size_t)h * HD;
  const int qt = blockIdx.y * 8 + wave;
  const int nqt = (T + 15) >> 4;
  const bool active = qt < nqt;
  const int q0 = qt * 16;

  auto stage = [&](int which) {                      // 1 = K, 2 = V
    for (int idx = tid; idx < KROWS * NC4; idx += 512) {
      const int r = idx / NC4, c4 = idx - r * NC4;
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (r < T && 4 * c4 < HD) {
        const float4 f = *reinterpret_cast<const float4*>(base + (size_t)r * row + (size_t)which * C + 4 * c4);
        v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
      }
      uint2 hi, lo;
      ev_split4(v, hi, lo);
      *reinterpret_cast<uint2*>(Sh + r * LD + 4 * c4) = hi;
      *reinterpret_cast<uint2*>(Sl + r * LD + 4 * c4) = lo;
    }
  };

  stage(1);
  // Q fragments: query q0 + li, d = 32 ks + 8 g .. + 7
  bf16x8 qh[NDS], ql[NDS];
#pragma unroll
  for (int ks = 0; ks < NDS; ++ks) {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = 0.f;
    if (active && q0 + li < T && 32 * ks + 8 * g < HD) {
      const float* p = base + (size_t)(q0 + li) * row + 32 * ks + 8 * g;
      const float4 f0 = *reinterpret_cast<const float4*>(p), f1 = *reinterpret_cast<const float4*>(p + 4);
      v[0] = f0.x; v[1] = f0.y; v[2] = f0.z; v[3] = f0.w; v[4] = f1.x; v[5] = f1.y; v[6] = f1.z; v[7] = f1.w;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      unsigned short hi, lo;
      ev_split(v[e], hi, lo);
      qh[ks][e] = (short)hi;
      ql[ks][e] = (short)lo;
    }
  }
  __syncthreads();

  f32x4 s[NKT];
  if (active) {
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < NDS; ++ks) {
        const int off = (16 * kt + li) * LD + 32 * ks + 8 * g;
        const bf16x8 kh = *reinterpret_cast<const bf16x8*>(Sh + off);
        const bf16x8 kl = *reinterpret_cast<const bf16x8*>(Sl + off);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kl, qh[ks], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kh, ql[ks], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kh, qh[ks], acc, 0, 0, 0);
      }
      s[kt] = acc;
    }
  }
  __syncthreads();                                   // every wave is done with K
  stage(2);
  float inv = 0.f;
  if (active) {
    float mx = -3.0e38f;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[kt][r] *= scale;
        if (16 * kt + 4 * g + r >= T) s[kt][r] = -3.0e38f;
        mx = fmaxf(mx, s[kt][r]);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = __expf(s[kt][r] - mx);
        s[kt][r] = p;
        sum += p;
      }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    inv = 1.f / sum;
  }
  __syncthreads();                                   // V staged
  if (!active) return;

  f32x4 o[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) o[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    float pv[8];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      pv[r] = s[2 * ks][r];
      pv[4 + r] = (2 * ks + 1 < NKT) ? s[(2 * ks + 1 < NKT) ? 2 * ks + 1 : 0][r] : 0.f;
    }
    bf16x8 ph, pl;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      unsigned short hi, lo;
      ev_split(pv[e], hi, lo);
      ph[e] = (short)hi;
      pl[e] = (short)lo;
    }
    // tr_split of basd_frag.h on both planes, written out on the kernel's own li (the helper changes the generated code)
    const int qq = li >> 2, pp = li & 3;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
      const int off = (32 * ks + 4 * g + qq) * LD + 16 * dt + 4 * pp;
      const v4s h0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)(Sh + off));
      const v4s h1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)(Sh + off + 16 * LD));
      const v4s l0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)(Sl + off));
      const v4s l1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)(Sl + off + 16 * LD));
      const bf16x8 vh = {h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
      const bf16x8 vl = {l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3]};
      o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pl, vh, o[dt], 0, 0, 0);
      o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ph, vl, o[dt], 0, 0, 0);
      o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ph, vh, o[dt], 0, 0, 0);
    }
  }
  // o[dt][r] = O[query q0 + 4 g + r][d = 16 dt + li] * sum; 1 / sum belongs to query q0 + li: fetch it from lane
  // 4 g + r (any lane group holds the same value)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float ir = __shfl(inv, 4 * g + r, 64);
    const int q = q0 + 4 * g + r;
    if (q >= T) continue;
    unsigned short* dst = out + (size_t)(b * T + q) * 2 * C + h * HD;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
      unsigned short hi, lo;
      ev_split(o[dt][r] * ir, hi, lo);
      dst[16 * dt + li] = hi;
      dst[C + 16 * dt + li] = lo;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Tiled attention for 1 <= T <= 1024: the arithmetic of attn_f32x3_kernel without its T x T state.  Workgroup = 8 waves
// = 8 query tiles of 16 of one (batch, head); grid (B H, ceil(T / 128)).  Keys stream through LDS in blocks of 128: the
// four images of a block (K hi, K lo, V hi, V lo: [128][LD] bf16 each, 72 KiB at hd 64 and 104 KiB at hd 80) fit
// together, so a block is staged once; the fp32 rows of the next block are loaded into registers while the current one
// multiplies and are split on their way into LDS.  Per block: S^T = K Q^T (8 key tiles, fragment layout as above),
// scaled in fp32, online softmax (running maximum and sum per query, kept on lane & 15; the output accumulators are
// rescaled by exp(m_old - m_new), fetched from the query's lane), P unnormalised in (0, 1] against the running maximum
// split into (hi, lo), O += P V through ds_read_tr16_b64.  The blocks are walked in key order by every wave: the sum has
// one order and the result is bitwise reproducible.  1 / sum is applied once to the fp32 output.
template <int HD>
__global__ __launch_bounds__(512) void attn_f32x3_long_kernel(const float* __restrict__ qkv, int T, int H, float scale,
                                                              unsigned short* __restrict__ out) {
  constexpr int KB = 128;                            // keys per block
  constexpr int NKT = KB / 16, NKS = KB / 32;
  constexpr int NDS = (HD + 31) / 32;
  constexpr int NDT = HD / 16;
  constexpr int LD = NDS * 32 + 8;
  constexpr int NC4 = HD / 4;                        // 4-float chunks of a row that hold data
  constexpr int NLD = KB * NC4 / 512;                // chunks per thread, block and operand (4 | 5)
  static_assert(KB * NC4 % 512 == 0, "a key block is a whole number of chunks per thread");
  extern __shared__ __align__(16) unsigned short sm[];
  unsigned short* Kh = sm;                            // [KB][LD] each
  unsigned short* Kl = sm + KB * LD;
  unsigned short* Vh = sm + 2 * KB * LD;
  unsigned short* Vl = sm + 3 * KB * LD;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int b = blockIdx.x / H, h = blockIdx.x - b * H;
  const int C = H * HD;
  const size_t row = (size_t)3 * C;
  const float* base = qkv + (size_t)b * T * row + (size_t)h * HD;
  const int q0 = (blockIdx.y * 8 + wave) * 16;
  const bool active = q0 < T;                        // wave-uniform; idle waves still stage and meet the barriers

  float4 kreg[NLD], vreg[NLD];
  auto load_kv = [&](int k0) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int idx = tid + 512 * i;
      const int r = idx / NC4, c4 = idx - r * NC4;
      kreg[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      vreg[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (k0 + r < T) {                              // keys past the end are zero rows (and masked below)
        const float* p = base + (size_t)(k0 + r) * row + 4 * c4;
        kreg[i] = *reinterpret_cast<const float4*>(p + C);
        vreg[i] = *reinterpret_cast<const float4*>(p + 2 * C);
      }
    }
  };
  load_kv(0);
  // the K columns hd .. 32 NDS - 1 meet the zero columns of Q in the contraction: written once, never staged over
  if constexpr (NDS * 32 > HD) {
    if (tid < 2 * KB) {
      unsigned short* p = (tid & 1 ? Kl : Kh) + (tid >> 1) * LD + HD;
#pragma unroll
      for (int c = 0; c < NDS * 32 - HD; c += 8) *reinterpret_cast<uint4*>(p + c) = make_uint4(0u, 0u, 0u, 0u);
    }
  }
  // Q fragments: query q0 + li, d = 32 ks + 8 g .. + 7
  bf16x8 qh[NDS], ql[NDS];
#pragma unroll
  for (int ks = 0; ks < NDS; ++ks) {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = 0.f;
    if (q0 + li < T && 32 * ks + 8 * g < HD) {
      const float* p = base + (size_t)(q0 + li) * row + 32 * ks + 8 * g;
      const float4 f0 = *reinterpret_cast<const float4*>(p), f1 = *reinterpret_cast<const float4*>(p + 4);
      v[0] = f0.x; v[1] = f0.y; v[2] = f0.z; v[3] = f0.w; v[4] = f1.x; v[5] = f1.y; v[6] = f1.z; v[7] = f1.w;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      unsigned short hi, lo;
      ev_split(v[e], hi, lo);
      qh[ks][e] = (short)hi;
      ql[ks][e] = (short)lo;
    }
  }

  float m_run = -3.0e38f, l_run = 0.f;               // of query q0 + li (the same value in the four lane groups)
  f32x4 o[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) o[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int nblocks = (T + KB - 1) / KB;
  for (int j = 0; j < nblocks; ++j) {
    const int k0 = j * KB;
    if (j > 0) lds_barrier();                        // every wave is done with the previous block
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int idx = tid + 512 * i;
      const int r = idx / NC4, c4 = idx - r * NC4;
      const float kv[4] = {kreg[i].x, kreg[i].y, kreg[i].z, kreg[i].w};
      const float vv[4] = {vreg[i].x, vreg[i].y, vreg[i].z, vreg[i].w};
      uint2 hi, lo;
      ev_split4(kv, hi, lo);
      *reinterpret_cast<uint2*>(Kh + r * LD + 4 * c4) = hi;
      *reinterpret_cast<uint2*>(Kl + r * LD + 4 * c4) = lo;
      ev_split4(vv, hi, lo);
      *reinterpret_cast<uint2*>(Vh + r * LD + 4 * c4) = hi;
      *reinterpret_cast<uint2*>(Vl + r * LD + 4 * c4) = lo;
    }
    lds_barrier();
    if (j + 1 < nblocks) load_kv(k0 + KB);           // in flight during this block's products
    if (!active) continue;

    // ---- S^T of the 8 key tiles
    f32x4 s[NKT];
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < NDS; ++ks) {
        const int off = (16 * kt + li) * LD + 32 * ks + 8 * g;
        const bf16x8 kh = *reinterpret_cast<const bf16x8*>(Kh + off);
        const bf16x8 kl = *reinterpret_cast<const bf16x8*>(Kl + off);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kl, qh[ks], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kh, ql[ks], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kh, qh[ks], acc, 0, 0, 0);
      }
      s[kt] = acc;
    }
    // ---- online softmax of this block
    float mx = -3.0e38f;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[kt][r] *= scale;
        if (k0 + 16 * kt + 4 * g + r >= T) s[kt][r] = -3.0e38f;
        mx = fmaxf(mx, s[kt][r]);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx);            // every block holds a valid key: m_new is finite
    const float alpha = __expf(m_run - m_new);       // first block: exp(-3e38) = 0 against l_run = 0, o = 0
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = __expf(s[kt][r] - m_new);
        s[kt][r] = p;
        sum += p;
      }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    l_run = fmaf(l_run, alpha, sum);
    m_run = m_new;
    // O rows are the queries q0 + 4 g + r: their factors live on lanes 4 g + r
    if (j > 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float ar = __shfl(alpha, 4 * g + r, 64);
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) o[dt][r] *= ar;
      }
    }
    // ---- O += P V
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      bf16x8 ph, pl;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        unsigned short hi, lo;
        ev_split(s[2 * ks + (e >> 2)][e & 3], hi, lo);
        ph[e] = (short)hi;
        pl[e] = (short)lo;
      }
      // tr_split of basd_frag.h on both planes, written out on the kernel's own li (the helper changes the generated code)
      const int qq = li >> 2, pp = li & 3;
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        const int off = (32 * ks + 4 * g + qq) * LD + 16 * dt + 4 * pp;
        const v4s h0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)(Vh + off));
        const v4s h1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)(Vh + off + 16 * LD));
        const v4s l0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)(Vl + off));
        const v4s l1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)(Vl + off + 16 * LD));
        const bf16x8 vh = {h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
        const bf16x8 vl = {l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3]};
        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pl, vh, o[dt], 0, 0, 0);
        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ph, vl, o[dt], 0, 0, 0);
        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ph, vh, o[dt], 0, 0, 0);
      }
    }
  }
  if (!active) return;
  // o[dt][r] = O[query q0 + 4 g + r][d = 16 dt + li] * sum; 1 / sum belongs to query q0 + li: fetch it from lane 4 g + r
  const float inv = 1.f / l_run;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float ir = __shfl(inv, 4 * g + r, 64);
    const int q = q0 + 4 * g + r;
    if (q >= T) continue;
    unsigned short* dst = out + (size_t)(b * T + q) * 2 * C + h * HD;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
      unsigned short hi, lo;
      ev_split(o[dt][r] * ir, hi, lo);
      dst[16 * dt + li] = hi;
      dst[C + 16 * dt + li] = lo;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// LayerNorm, one wave per row, D % 4 == 0, D <= 2048 (<= 8 float4 per lane); statistics two-pass in fp32 from registers.
__global__ __launch_bounds__(256) void ln_f32_kernel(const float* x, const float* res,
                                                     const float* __restrict__ xscale, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, int64_t rows, int D, float eps,
                                                     float* s_out, float* __restrict__ y,
                                                     unsigned short* __restrict__ y_img) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int nch = D >> 2;
  float4 v[8];
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = lane + 64 * i;
    v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < nch) {
      float4 a = *reinterpret_cast<const float4*>(x + r * D + 4 * c);
      if (xscale != nullptr) {
        const float4 g4 = *reinterpret_cast<const float4*>(xscale + 4 * c);
        a.x *= g4.x; a.y *= g4.y; a.z *= g4.z; a.w *= g4.w;
      }
      if (res != nullptr) {
        const float4 q = *reinterpret_cast<const float4*>(res + r * D + 4 * c);
        a.x += q.x; a.y += q.y; a.z += q.z; a.w += q.w;
      }
      v[i] = a;
      sum += (a.x + a.y) + (a.z + a.w);
    }
  }
  const float mean = wave_sum(sum) / (float)D;
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (lane + 64 * i < nch) {
      const float a = v[i].x - mean, b = v[i].y - mean, c = v[i].z - mean, d = v[i].w - mean;
      sq += (a * a + b * b) + (c * c + d * d);
    }
  }
  const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)D + eps);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = lane + 64 * i;
    if (c >= nch) continue;
    if (s_out != nullptr) *reinterpret_cast<float4*>(s_out + r * D + 4 * c) = v[i];
    const float4 g4 = *reinterpret_cast<const float4*>(gamma + 4 * c);
    const float4 b4 = *reinterpret_cast<const float4*>(beta + 4 * c);
    float o[4] = {(v[i].x - mean) * rstd * g4.x + b4.x, (v[i].y - mean) * rstd * g4.y + b4.y,
                  (v[i].z - mean) * rstd * g4.z + b4.z, (v[i].w - mean) * rstd * g4.w + b4.w};
    if (y != nullptr) *reinterpret_cast<float4*>(y + r * D + 4 * c) = make_float4(o[0], o[1], o[2], o[3]);
    if (y_img != nullptr) {
      uint2 hi, lo;
      ev_split4(o, hi, lo);
      *reinterpret_cast<uint2*>(y_img + r * 2 * D + 4 * c) = hi;
      *reinterpret_cast<uint2*>(y_img + r * 2 * D + D + 4 * c) = lo;
    }
  }
}

template <int NKT, int HD>
static void launch_attn(const float* qkv, int B, int T, int H, float scale, unsigned short* out, hipStream_t st) {
  constexpr int LD = ((HD + 31) / 32) * 32 + 8;
  const size_t lds = (size_t)2 * 32 * ((NKT + 1) / 2) * LD * sizeof(unsigned short);
  allow_full_lds((const void*)attn_f32x3_kernel<NKT, HD>);
  hipLaunchKernelGGL((attn_f32x3_kernel<NKT, HD>), dim3(B * H, (((T + 15) >> 4) + 7) / 8), dim3(512), lds, st, qkv, T,
                     H, scale, out);
}

template <int HD>
static void launch_attn_long(const float* qkv, int B, int T, int H, float scale, unsigned short* out, hipStream_t st) {
  constexpr int LD = ((HD + 31) / 32) * 32 + 8;
  const size_t lds = (size_t)4 * 128 * LD * sizeof(unsigned short);
  allow_full_lds((const void*)attn_f32x3_long_kernel<HD>);
  hipLaunchKernelGGL(attn_f32x3_long_kernel<HD>, dim3(B * H, (T + 127) / 128), dim3(512), lds, st, qkv, T, H, scale,
                     out);
}

}  // namespace basd

static bool ev_aligned(const void* p, int bytes) { return ((uintptr_t)p % (uintptr_t)bytes) == 0; }

extern "C" int basd_split_bf16x2_table(const int64_t* table, int n_entries, void* stream) {
  using namespace basd;
  if (n_entries < 0) return fail(BASD_ERR_SHAPE, "split_bf16x2_table: n_entries = %d", n_entries);
  for (int base = 0; base < n_entries; base += ST_MAX) {
    SplitTable t;
    t.n = n_entries - base < ST_MAX ? n_entries - base : ST_MAX;
    int blocks = 0;
    for (int i = 0; i < t.n; ++i) {
      const int64_t* e = table + 5 * (int64_t)(base + i);
      if (e[0] == 0 || e[1] == 0 || e[2] <= 0 || e[3] <= 0 || e[4] < e[3] || e[2] * e[4] > 0x7fffffffLL * 256)
        return fail(BASD_ERR_SHAPE, "split_bf16x2_table: entry %d: rows %lld k %lld k_pad %lld", base + i,
                    (long long)e[2], (long long)e[3], (long long)e[4]);
      t.src[i] = e[0]; t.dst[i] = e[1]; t.rows[i] = (int)e[2]; t.k[i] = (int)e[3]; t.kp[i] = (int)e[4];
      t.blk0[i] = blocks;
      blocks += (int)((e[2] * e[4] + 1023) / 1024);
    }
    t.blk0[t.n] = blocks;
    if (blocks > 0) hipLaunchKernelGGL(split_table_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, t);
  }
  return check_launch("split_bf16x2_table");
}

extern "C" int basd_split_patches_bf16x2(const float* x, int B, int C, int H, int W, int p, int k_pad, void* out,
                                         void* stream) {
  using namespace basd;
  if (B <= 0) return BASD_OK;
  if (C <= 0 || p <= 0 || H % p || W % p || H < p || W < p || k_pad < C * p * p || k_pad % 32)
    return fail(BASD_ERR_SHAPE, "split_patches_bf16x2: C=%d H=%d W=%d p=%d k_pad=%d", C, H, W, p, k_pad);
  const int64_t total = (int64_t)B * (H / p) * (W / p) * k_pad;
  if ((total + 255) / 256 > 0x7fffffffLL) return fail(BASD_ERR_SHAPE, "split_patches_bf16x2: too large");
  hipLaunchKernelGGL(split_patches_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x,
                     C, H, W, p, k_pad, total, (unsigned short*)out);
  return check_launch("split_patches_bf16x2");
}

extern "C" int basd_gemm_f32x3(const void* x_img, const void* w_img, const float* bias, void* y, int64_t M, int N,
                               int k_pad, int epilogue, void* stream) {
  using namespace basd;
  if (M <= 0) return BASD_OK;
  if (epilogue < 0 || epilogue > 3) return fail(BASD_ERR_SHAPE, "gemm_f32x3: epilogue %d not in 0..3", epilogue);
  if (N < 16 || N % 16 || k_pad < 32 || k_pad % 32)
    return fail(BASD_ERR_SHAPE, "gemm_f32x3: need N %% 16 == 0 and k_pad %% 32 == 0 (got N=%d k_pad=%d)", N, k_pad);
  if ((M + 127) / 128 > 65535) return fail(BASD_ERR_SHAPE, "gemm_f32x3: M = %lld too large", (long long)M);
  if (!ev_aligned(x_img, 16) || !ev_aligned(w_img, 16) || !ev_aligned(y, 16) || (bias && !ev_aligned(bias, 16)))
    return fail(BASD_ERR_SHAPE, "gemm_f32x3: operands must be 16-byte aligned");
  const dim3 grid(N / 128 + (N % 128 ? 1 : 0), (unsigned)((M + 127) / 128));
  hipStream_t st = (hipStream_t)stream;
  const unsigned short* X = (const unsigned short*)x_img;
  const unsigned short* Wt = (const unsigned short*)w_img;
  const int m = (int)M;
#define BASD_EG(G, S)                                                                                    \
  do {                                                                                                   \
    allow_full_lds((const void*)gemm_f32x3_kernel<G, S>);                                                \
    hipLaunchKernelGGL((gemm_f32x3_kernel<G, S>), grid, dim3(256), EG_LDS, st, X, Wt, bias, y, m, N, k_pad); \
  } while (0)
  switch (epilogue) {
    case 0: BASD_EG(false, false); break;
    case 1: BASD_EG(true, false); break;
    case 2: BASD_EG(false, true); break;
    default: BASD_EG(true, true); break;
  }
#undef BASD_EG
  return check_launch("gemm_f32x3");
}

extern "C" int basd_attention_fwd_f32x3(const float* qkv, int B, int T, int H, int hd, float scale, void* out_img,
                                        void* stream) {
  using namespace basd;
  if (B <= 0) return BASD_OK;
  if (T < 1 || T > 272 || (hd != 64 && hd != 80) || H < 1)
    return fail(BASD_ERR_SHAPE, "attention_fwd_f32x3: need hd in {64, 80}, 1 <= T <= 272 (got T=%d hd=%d H=%d)", T, hd, H);
  if (!ev_aligned(qkv, 16)) return fail(BASD_ERR_SHAPE, "attention_fwd_f32x3: qkv must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  unsigned short* o = (unsigned short*)out_img;
  const int nkt = (T + 15) / 16;
#define BASD_ATTN32(NKT_)                                                    \
  if (nkt <= NKT_) {                                                         \
    if (hd == 64) launch_attn<NKT_, 64>(qkv, B, T, H, scale, o, st);         \
    else launch_attn<NKT_, 80>(qkv, B, T, H, scale, o, st);                  \
    return check_launch("attention_fwd_f32x3");                              \
  }
  BASD_ATTN32(4)
  BASD_ATTN32(9)
  BASD_ATTN32(13)
  BASD_ATTN32(17)
#undef BASD_ATTN32
  return fail(BASD_ERR_SHAPE, "attention_fwd_f32x3: T = %d", T);
}

extern "C" int basd_attention_fwd_f32x3_long(const float* qkv, int B, int T, int H, int hd, float scale, void* out_img,
                                             void* stream) {
  using namespace basd;
  if (B <= 0) return BASD_OK;
  if (T < 1 || T > 1024 || (hd != 64 && hd != 80) || H < 1)
    return fail(BASD_ERR_SHAPE, "attention_fwd_f32x3_long: need hd in {64, 80}, 1 <= T <= 1024, H >= 1 (got T=%d hd=%d H=%d)",
                T, hd, H);
  if (!ev_aligned(qkv, 16)) return fail(BASD_ERR_SHAPE, "attention_fwd_f32x3_long: qkv must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (hd == 64) launch_attn_long<64>(qkv, B, T, H, scale, (unsigned short*)out_img, st);
  else launch_attn_long<80>(qkv, B, T, H, scale, (unsigned short*)out_img, st);
  return check_launch("attention_fwd_f32x3_long");
}

extern "C" int basd_add_layernorm_fwd_f32(const float* x, const float* residual, const float* xscale, const float* gamma,
                                          const float* beta, int64_t rows, int D, float eps, float* s_out, float* y,
                                          void* y_img, void* stream) {
  using namespace basd;
  if (rows <= 0) return BASD_OK;
  if (D < 4 || D % 4 || D > 2048) return fail(BASD_ERR_SHAPE, "add_layernorm_fwd_f32: D = %d (need D %% 4 == 0, <= 2048)", D);
  if (y == nullptr && y_img == nullptr) return fail(BASD_ERR_SHAPE, "add_layernorm_fwd_f32: no output");
  if ((rows + 3) / 4 > 0x7fffffffLL) return fail(BASD_ERR_SHAPE, "add_layernorm_fwd_f32: rows = %lld", (long long)rows);
  hipLaunchKernelGGL(ln_f32_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, residual,
                     xscale, gamma, beta, rows, D, eps, s_out, y, (unsigned short*)y_img);
  return check_launch("add_layernorm_fwd_f32");
}
