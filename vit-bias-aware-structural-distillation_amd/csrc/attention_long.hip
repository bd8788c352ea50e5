// Tiled (flash-style) attention for token counts past the single-workgroup kernels of attention.hip /
// attention_bwd.hip / attn_tap.hip: 1 <= T <= 1024, hd 64 or 80.  The entries below only take over the shapes those
// kernels refuse (ViT /14 grids at 224 px: T = 257; 384 px: T = 577; hd-80 students of a ViT-H/14 teacher); the
// dispatch lives in _native.py.
//
// Forward: one workgroup (4 waves) per (image, head, 64-query block); wave w owns the 16 queries 64 qb + 16 w.
//   K / V tiles of 64 keys stream through LDS (row-major, rows of hd padded to a multiple of 32 plus 8 elements: the
//   bank rotation of attention.hip); the next tile is loaded into registers while the current one is used.
//   S^T = K Q^T  v_mfma_f32_16x16x32_bf16 with A = K rows from LDS, B = Q rows (registers for the whole loop): the
//                accumulator of key tile kt holds, for the query of column lane & 15, the keys 16 kt + 4 (lane >> 4) +
//                {0..3}, so the row max / row sum of the online softmax is a register reduction plus two xor shuffles;
//   O  += P V    A = P (the two S^T accumulators of a 32-key step, rounded to bf16 unnormalised), B = V through the
//                transposing LDS read ds_read_b64_tr_b16; O rows are queries 4 (lane >> 4) + r, so the per-query rescale
//                factor exp(m_old - m_new) is fetched from the query's lane (one ds_bpermute per row).
//   The S x S matrix is never stored; the LSE (natural log of sum_k exp(scale q.k)) is written per query.
// Taps (exact contracts of attention.hip):
//   CLS row      attn_long_cls_kernel: query 0 of every head over all keys with bf16-rounded logits (the teacher's
//                autocast matmul), a separate pass because that softmax is not the one of the main loop;
//   query mean   attn_long_qmean_kernel: one wave per 16-key tile walks every query tile, recomputes P from the LSE of
//                the main pass and sums it down the column in a fixed order -- no partials, no atomics, bitwise
//                reproducible.
// Position schemes (frozen teachers past the 272 tokens of attention.hip; the schemes, their argument and the legal
// combinations: attn_pos.h).  The forward and the CLS tap take the AttnPosArg behind their plain argument list, which
// the plain instantiations do not read.  No LSE, no query mean.
//   AttnPos::Rope    basd_attention_fwd_long_rope_bf16: a K chunk is rotated between its global load and its LDS store --
//                    its table rows travel with it through the prefetch registers -- and the Q fragments once in front
//                    of the key loop.  The CLS tap rotates q_0 and every k row the same way before its dot: it is the
//                    tap above on the rotated, bf16-rounded operands.
//   AttnPos::RelBias basd_attention_fwd_long_relbias_bf16: the head's column of the table is staged DIVIDED BY scale
//                    (R <= 4095 floats for T <= 1024) and added to the raw accumulator in front of the tile's maximum,
//                    so the online softmax below it is the plain kernel's to the instruction (an all-zero table gives
//                    the plain kernel's bits) and a masked tail key stays masked.  The CLS row's bias is two constants
//                    per head: the tap adds them to its scaled, bf16-rounded logits.
//
// Backward (FA2): attn_long_delta_kernel computes delta = rowsum(dO * O); attn_long_bwd_kernel runs one workgroup per
// (image, head, 128-key block), wave w owning 32 keys whose K / V fragments and dK^T / dV^T accumulators stay in
// registers (key on the lane, the layout of attention_bwd.hip) while the workgroup walks all queries 32 at a time.
// dQ: the four waves' 32 x hd contributions meet in LDS and are added in wave order; the block's sum goes to a
// per-key-block fp32 partial in the workspace (vector stores), and attn_long_dq_kernel adds the partials in key-block
// order and writes the bf16 dQ slice of dqkv.  No atomics: the gradient is bitwise reproducible.
#include "attn_pos.h"

namespace basd {

constexpr int AL_MAXT = 1024;
constexpr float AL_LOG2E = 1.4426950408889634f;
constexpr int AL_MAXR = 4096;                        // R <= 4 gh gw + 3 <= 4095 for T <= AL_MAXT

// ------------------------------------------------------------------------------------------------------ forward ----
template <int HD, AttnPos POS = AttnPos::None>
__global__ __launch_bounds__(256) void attn_long_fwd_kernel(
    const unsigned short* __restrict__ qkv, int T, int H, float scale, unsigned short* __restrict__ out,
    float* __restrict__ lse, AttnPosArg pos) {
  static_assert(attn_pos_ok<POS, HD>, "a position scheme: head dim 64");
  constexpr bool RELBIAS = POS == AttnPos::RelBias, ROPE = POS == AttnPos::Rope;
  constexpr int KB = 64;                             // keys per LDS tile
  constexpr int NDS = (HD + 31) / 32;                // 32-deep steps of the Q K^T contraction
  constexpr int NDT = HD / 16;                       // 16-column tiles of the output
  constexpr int NCH = HD / 8;                        // 16-byte chunks of a row that hold data
  constexpr int NCHP = NDS * 4;                      // ... of a padded row
  constexpr int LD = NDS * 32 + 8;                   // LDS row stride in bf16
  constexpr int NLD = (KB * NCHP + 255) / 256;       // 16-byte chunks per thread and tile
  __shared__ __align__(16) unsigned short Ks[KB * LD];
  __shared__ __align__(16) unsigned short Vs[KB * LD];
  __shared__ __align__(16) unsigned short Os[4 * 16 * LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const int q0 = blockIdx.y * 64 + 16 * wave;
  const size_t row = (size_t)3 * H * HD;
  const unsigned short* base = qkv + (size_t)b * T * row + (size_t)h * HD;

  float* tab = nullptr;                              // RELBIAS: the head's column of the table / scale, [R]
  int* koff = nullptr;                               // RELBIAS: y_k (2 gw - 1) + x_k of patch key k, [AL_MAXT]
  if constexpr (RELBIAS) {
    __shared__ float tab_s[AL_MAXR];
    __shared__ __align__(16) int koff_s[AL_MAXT];
    tab = tab_s;
    koff = koff_s;
  }

  uint4 kreg[NLD], vreg[NLD];
  float4 kcs[ROPE ? NLD : 1][2];                     // ROPE: (cos, sin) of the four pairs of every K chunk
  auto load_kv = [&](int k0) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int idx = tid + 256 * i;
      const int r = idx / NCHP, c8 = idx - r * NCHP;
      kreg[i] = make_uint4(0, 0, 0, 0);
      vreg[i] = make_uint4(0, 0, 0, 0);
      if constexpr (ROPE) rope_none(kcs[i]);
      if (idx < KB * NCHP && k0 + r < T && c8 < NCH) {
        const unsigned short* p = base + (size_t)(k0 + r) * row + c8 * 8;
        kreg[i] = *reinterpret_cast<const uint4*>(p + (size_t)H * HD);
        vreg[i] = *reinterpret_cast<const uint4*>(p + (size_t)2 * H * HD);
        if constexpr (ROPE) rope_rows(pos.table, k0 + r, HD, c8 * 8, kcs[i]);    // the row of the GLOBAL key index
      }
    }
  };
  load_kv(0);
  // Q fragments of this wave's tile: query q0 + li, d = 32 ks + 8 g .. + 7 (zero beyond T and beyond hd; written out
  // in both files, see attention.hip)
  bf16x8 qf[NDS];
#pragma unroll
  for (int ks = 0; ks < NDS; ++ks) {
    uint4 v = make_uint4(0, 0, 0, 0);
    if (q0 + li < T && 32 * ks + 8 * g < HD)
      v = *reinterpret_cast<const uint4*>(base + (size_t)(q0 + li) * row + 32 * ks + 8 * g);
    if constexpr (ROPE) {                            // rotated once: the fragments stay in registers for the whole loop
      if (q0 + li < T) {
        float4 cs[2];
        rope_rows(pos.table, q0 + li, HD, 32 * ks + 8 * g, cs);
        v = rope_chunk(v, cs[0], cs[1]);
      }
    }
    qf[ks] = *reinterpret_cast<const bf16x8*>(&v);
  }
  // RELBIAS: the column divided by scale and the key offsets (rule: relbias_koff); the first barrier of the key loop
  // publishes tab and koff
  RelBiasQuery rq = {0, 0, false};
  if constexpr (RELBIAS) {
    const int R = relbias_rows(pos);
    for (int i0 = 0; i0 < R; i0 += 1024) {
      float tv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int idx = i0 + tid + 256 * i;
        tv[i] = (idx < R) ? pos.table[(size_t)idx * H + h] / scale : 0.f;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int idx = i0 + tid + 256 * i;
        if (idx < R) tab[idx] = tv[i];
      }
    }
    for (int key = tid; key < AL_MAXT; key += 256) koff[key] = relbias_koff(pos, key, T);
    rq = relbias_query(pos, q0 + li, T);
  }
  const float sl2 = scale * AL_LOG2E;
  float m_run = -3.0e38f, l_run = 0.f;               // per query column li (same value in the four lane groups)
  f32x4 o[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) o[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int ntiles = (T + KB - 1) / KB;
  for (int j = 0; j < ntiles; ++j) {
    const int k0 = j * KB;
    if (j > 0) lds_barrier();                        // every wave is done with the previous tile
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int idx = tid + 256 * i;
      const int r = idx / NCHP, c8 = idx - r * NCHP;
      if constexpr (ROPE) kreg[i] = rope_chunk(kreg[i], kcs[i][0], kcs[i][1]);    // padding rows: zeros stay zeros
      if (idx < KB * NCHP) {
        *reinterpret_cast<uint4*>(Ks + r * LD + c8 * 8) = kreg[i];
        *reinterpret_cast<uint4*>(Vs + r * LD + c8 * 8) = vreg[i];
      }
    }
    lds_barrier();
    if (j + 1 < ntiles) load_kv(k0 + KB);            // in flight during this tile's products
    // ---- S^T of the 4 key tiles
    f32x4 s[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < NDS; ++ks) {
        const bf16x8 kk = *reinterpret_cast<const bf16x8*>(Ks + (16 * kt + li) * LD + 32 * ks + 8 * g);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kk, qf[ks], acc, 0, 0, 0);
      }
      s[kt] = acc;
    }
    if constexpr (RELBIAS) {                         // s += table[idx(query, key)] / scale: keys k0 + 16 kt + 4 g + r
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        float bias[4];
        relbias_gather(rq, tab, koff + k0 + 16 * kt, g, kt == 0 && k0 == 0, bias);
#pragma unroll
        for (int r = 0; r < 4; ++r) s[kt][r] += bias[r];
      }
    }
    // ---- online softmax of this tile
    float mx = -3.0e38f;
    const bool tail = k0 + KB > T;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (tail && k0 + 16 * kt + 4 * g + r >= T) s[kt][r] = -3.0e38f;
        mx = fmaxf(mx, s[kt][r]);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx);            // every tile holds a valid key: m_new is finite
    const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * sl2);
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = __builtin_amdgcn_exp2f((s[kt][r] - m_new) * sl2);
        s[kt][r] = p;
        sum += p;
      }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    l_run = fmaf(l_run, alpha, sum);
    m_run = m_new;
    // O rows are the queries 4 g + r: their factors live on lanes 4 g + r
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float ar = __shfl(alpha, 4 * g + r, 64);
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) o[dt][r] *= ar;
    }
    // ---- O += P V
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      uint4 pw;
      pw.x = pack_bf16(s[2 * ks][0], s[2 * ks][1]);
      pw.y = pack_bf16(s[2 * ks][2], s[2 * ks][3]);
      pw.z = pack_bf16(s[2 * ks + 1][0], s[2 * ks + 1][1]);
      pw.w = pack_bf16(s[2 * ks + 1][2], s[2 * ks + 1][3]);
      const bf16x8 pa = *reinterpret_cast<const bf16x8*>(&pw);
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        const bf16x8 vb = tr_split(Vs, LD, 32 * ks + 4 * g, 16 * dt, lane);
        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, vb, o[dt], 0, 0, 0);
      }
    }
  }
  // ---- normalise, LSE, store (rows through the wave's LDS tile: 16-byte row stores; written out in both files, see
  //      attention.hip)
  if (POS == AttnPos::None && lse != nullptr && g == 0 && q0 + li < T)
    lse[(size_t)bh * T + q0 + li] = fmaf(m_run, scale, __logf(l_run));
  const float inv = 1.f / l_run;
  unsigned short* Ow = Os + wave * 16 * LD;
#pragma unroll
  for (int r = 0; r < 4; r += 2) {
    const float i0 = __shfl(inv, 4 * g + r, 64), i1 = __shfl(inv, 4 * g + r + 1, 64);
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
      const unsigned int w = pack_bf16(o[dt][r] * i0, o[dt][r + 1] * i1);
      Ow[(4 * g + r) * LD + 16 * dt + li] = (unsigned short)(w & 0xffffu);
      Ow[(4 * g + r + 1) * LD + 16 * dt + li] = (unsigned short)(w >> 16);
    }
  }
  __builtin_amdgcn_s_waitcnt(0xc07f);                // lgkmcnt(0): the tile is private to this wave
#pragma unroll
  for (int c = 0; c < (16 * NCH + 63) / 64; ++c) {
    const int idx = lane + 64 * c, r = idx / NCH, c8 = idx - r * NCH;
    if (idx < 16 * NCH && q0 + r < T) {
      const uint4 v = *reinterpret_cast<const uint4*>(Ow + r * LD + c8 * 8);
      *reinterpret_cast<uint4*>(out + ((size_t)(b * T + q0 + r) * H + h) * HD + c8 * 8) = v;
    }
  }
}

// CLS-row tap, per head: importance[b, h, t-1] = softmax_t(bf16(q_0 . k_t) * scale) / H, the arithmetic of
// attn_tap.hip (fp32 dot in d order, round to bf16, scale, expf).  One workgroup per (image, head).  ROPE: q_0 and
// every k row are rotated by their table rows and rounded to bf16 in front of that dot.  RELBIAS: the CLS row's bias,
// table[R - 1][h] for key 0 and table[R - 3][h] for every patch key, is added to the scaled logit.
template <int HD, AttnPos POS = AttnPos::None>
__global__ __launch_bounds__(256) void attn_long_cls_kernel(
    const unsigned short* __restrict__ qkv, int T, int H, float scale, float* __restrict__ importance, AttnPosArg pos) {
  static_assert(attn_pos_ok<POS, HD>, "a position scheme: head dim 64");
  constexpr bool RELBIAS = POS == AttnPos::RelBias, ROPE = POS == AttnPos::Rope;
  __shared__ float logit[AL_MAXT];
  __shared__ float red[8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const size_t row = (size_t)3 * H * HD;
  const unsigned short* base = qkv + (size_t)b * T * row;
  float bias_cls = 0.f, bias_patch = 0.f;            // RELBIAS: the CLS query against the CLS key / against a patch key
  if constexpr (RELBIAS) {
    const int R = relbias_rows(pos);
    bias_cls = pos.table[(size_t)(R - 1) * H + h];
    bias_patch = pos.table[(size_t)(R - 3) * H + h];
  }
  float q[HD];
  if constexpr (ROPE) {
#pragma unroll
    for (int v = 0; v < HD / 8; ++v) {               // token 0's table row
      float4 cs[2];
      rope_rows(pos.table, 0, HD, 8 * v, cs);
      const uint4 w = rope_chunk(*reinterpret_cast<const uint4*>(base + (size_t)h * HD + 8 * v), cs[0], cs[1]);
      const unsigned int ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        q[8 * v + 2 * e] = __uint_as_float(ww[e] << 16);
        q[8 * v + 2 * e + 1] = __uint_as_float(ww[e] & 0xffff0000u);
      }
    }
  } else {
#pragma unroll
    for (int d = 0; d < HD; ++d) q[d] = bf16_bits_to_f32(base[(size_t)h * HD + d]);
  }
  float mx = -3.0e38f;
  for (int t = tid; t < T; t += 256) {
    const uint4* kp = reinterpret_cast<const uint4*>(base + (size_t)t * row + (size_t)(H + h) * HD);
    float dot = 0.f;
#pragma unroll
    for (int v = 0; v < HD / 8; ++v) {
      uint4 w = kp[v];
      if constexpr (ROPE) {
        float4 cs[2];
        rope_rows(pos.table, t, HD, 8 * v, cs);
        w = rope_chunk(w, cs[0], cs[1]);
      }
      const unsigned int ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        dot = fmaf(q[8 * v + 2 * e], __uint_as_float(ww[e] << 16), dot);
        dot = fmaf(q[8 * v + 2 * e + 1], __uint_as_float(ww[e] & 0xffff0000u), dot);
      }
    }
    unsigned int bits = __float_as_uint(dot);
    bits += 0x7fffu + ((bits >> 16) & 1u);
    float l = __uint_as_float(bits & 0xffff0000u) * scale;
    if constexpr (RELBIAS) l += (t == 0) ? bias_cls : bias_patch;
    logit[t] = l;
    mx = fmaxf(mx, l);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float sum = 0.f;
  for (int t = tid; t < T; t += 256) {
    const float p = expf(logit[t] - mx);
    logit[t] = p;
    sum += p;
  }
  sum = wave_sum(sum);
  if (lane == 0) red[4 + wave] = sum;
  __syncthreads();
  sum = (red[4] + red[5]) + (red[6] + red[7]);
  const float inv = 1.f / (sum * (float)H);
  for (int t = 1 + tid; t < T; t += 256) importance[(size_t)bh * (T - 1) + t - 1] = logit[t] * inv;
}

// Query-mean tap, per head: importance[b, h, key] = sum_q P[q][key] / (H T), P = exp(scale q.k - LSE_q) with the LSE of
// the main pass.  Wave = 16 keys (a workgroup 64); K fragments in registers, Q tiles read from global (L2) in query
// order; the column sum is per lane, then over the 16 query lanes: a fixed order.
template <int HD>
__global__ __launch_bounds__(256) void attn_long_qmean_kernel(const unsigned short* __restrict__ qkv, int T, int H,
                                                              float scale, const float* __restrict__ lse,
                                                              float* __restrict__ importance) {
  constexpr int NDS = (HD + 31) / 32;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const int k0 = blockIdx.y * 64 + 16 * wave;
  if (k0 >= T) return;                               // wave-uniform; no barriers below
  const size_t row = (size_t)3 * H * HD;
  const unsigned short* base = qkv + (size_t)b * T * row + (size_t)h * HD;
  const float* lrow = lse + (size_t)bh * T;
  bf16x8 kf[NDS];
#pragma unroll
  for (int ks = 0; ks < NDS; ++ks) {
    uint4 v = make_uint4(0, 0, 0, 0);
    if (k0 + li < T && 32 * ks + 8 * g < HD)
      v = *reinterpret_cast<const uint4*>(base + (size_t)(k0 + li) * row + (size_t)H * HD + 32 * ks + 8 * g);
    kf[ks] = *reinterpret_cast<const bf16x8*>(&v);
  }
  const float sl2 = scale * AL_LOG2E;
  float csum[4] = {0.f, 0.f, 0.f, 0.f};
  for (int qs = 0; qs < T; qs += 16) {
    const int q = qs + li;
    bf16x8 qf[NDS];
#pragma unroll
    for (int ks = 0; ks < NDS; ++ks) {
      uint4 v = make_uint4(0, 0, 0, 0);
      if (q < T && 32 * ks + 8 * g < HD) v = *reinterpret_cast<const uint4*>(base + (size_t)q * row + 32 * ks + 8 * g);
      qf[ks] = *reinterpret_cast<const bf16x8*>(&v);
    }
    const float nl = (q < T) ? lrow[q] * AL_LOG2E : 0.f;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < NDS; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[ks], qf[ks], acc, 0, 0, 0);
    // acc[r]: key k0 + 4 g + r, query q
    if (q < T) {
#pragma unroll
      for (int r = 0; r < 4; ++r) csum[r] += __builtin_amdgcn_exp2f(fmaf(acc[r], sl2, -nl));
    }
  }
  const float norm = 1.f / ((float)H * (float)T);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float v = csum[r];
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
    const int key = k0 + 4 * g + r;
    if (li == 0 && key < T) importance[(size_t)bh * T + key] = v * norm;
  }
}

// ----------------------------------------------------------------------------------------------------- backward ----
// delta[b, h, t] = sum_d dO[b, t, h, d] O[b, t, h, d] (bf16 inputs, fp32 sum); one thread per (b, t, h)
template <int HD>
__global__ __launch_bounds__(256) void attn_long_delta_kernel(const unsigned short* __restrict__ out,
                                                              const unsigned short* __restrict__ dout, int B, int T,
                                                              int H, float* __restrict__ delta) {
  const int64_t n = (int64_t)B * T * H;
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int h = (int)(i % H);
    const int64_t bt = i / H;
    const int t = (int)(bt % T), b = (int)(bt / T);
    const uint4* op = reinterpret_cast<const uint4*>(out + i * HD);
    const uint4* dp = reinterpret_cast<const uint4*>(dout + i * HD);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < HD / 8; ++c) {
      const uint4 ov = op[c], dv = dp[c];
      const unsigned int ow[4] = {ov.x, ov.y, ov.z, ov.w}, dw[4] = {dv.x, dv.y, dv.z, dv.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        s = fmaf(__uint_as_float(dw[e] << 16), __uint_as_float(ow[e] << 16), s);
        s = fmaf(__uint_as_float(dw[e] & 0xffff0000u), __uint_as_float(ow[e] & 0xffff0000u), s);
      }
    }
    delta[((size_t)b * H + h) * T + t] = s;
  }
}

template <int HD>
struct AlBwdCfg {
  static constexpr int NDS = (HD + 31) / 32;         // 32-deep steps of the S / dP contraction
  static constexpr int NDT = HD / 16;                // 16-column tiles of d
  static constexpr int NCH = HD / 8;
  static constexpr int NCHP = NDS * 4;
  static constexpr int LD = NDS * 32 + 8;            // bf16 row stride of the Q / dO / K images
  static constexpr int SLD = 40;                     // bf16 row stride of the wave's dS tile
  static constexpr int QLD = HD + 4;                 // fp32 row stride of the dQ images
  static constexpr int NST = (32 * NCHP + 255) / 256;   // 16-byte chunks per thread of a 32-row slice
  static constexpr size_t LDS = (size_t)2 * 32 * LD * 2 + (size_t)2 * 32 * 4 + (size_t)4 * 32 * LD * 2 +
                                (size_t)4 * 32 * QLD * 4;
};

template <int HD>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void attn_long_bwd_kernel(
    const unsigned short* __restrict__ qkv, const unsigned short* __restrict__ dout, const float* __restrict__ lse,
    const float* __restrict__ delta, unsigned short* __restrict__ dqkv, float* __restrict__ dq_part, int T, int H,
    float scale) {
  using C = AlBwdCfg<HD>;
  constexpr int NDS = C::NDS, NDT = C::NDT, NCH = C::NCH, NCHP = C::NCHP, LD = C::LD, SLD = C::SLD, QLD = C::QLD;
  constexpr int NST = C::NST;
  extern __shared__ __align__(16) unsigned char al_smem[];
  unsigned short* Qs = reinterpret_cast<unsigned short*>(al_smem);     // [32][LD]
  unsigned short* dOs = Qs + 32 * LD;                                  // [32][LD]
  float* nlse = reinterpret_cast<float*>(dOs + 32 * LD);               // [32]  -LSE / scale
  float* ndel = nlse + 32;                                             // [32]  -delta
  unsigned short* wtile = reinterpret_cast<unsigned short*>(ndel + 32);   // [4 waves][32][LD]
  float* dqs = reinterpret_cast<float*>(wtile + 4 * 32 * LD);          // [4 waves][32][QLD]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const int kblk = blockIdx.y, nkb = gridDim.y;
  const int kbase = 128 * kblk + 32 * wave;
  const bool active = kbase < T;
  const size_t row = (size_t)3 * H * HD;
  const size_t orow = (size_t)H * HD;
  const unsigned short* qbase = qkv + (size_t)b * T * row + (size_t)h * HD;
  const unsigned short* dobase = dout + (size_t)b * T * orow + (size_t)h * HD;
  unsigned short* mytile = wtile + wave * 32 * LD;
  float* mydq = dqs + wave * 32 * QLD;

  // ---- this wave's 32 keys: B operands of S / dP (key kbase + 16 t + li, d = 32 ks + 8 g ..) and of dQ = dS K
  bf16x8 kb[2][NDS], vb[2][NDS], kt[NDT];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int ks = 0; ks < NDS; ++ks) {
      const int key = kbase + 16 * t + li;
      uint4 kv = make_uint4(0, 0, 0, 0), vv = make_uint4(0, 0, 0, 0);
      if (key < T && 32 * ks + 8 * g < HD) {
        const unsigned short* p = qbase + (size_t)key * row + 32 * ks + 8 * g;
        kv = *reinterpret_cast<const uint4*>(p + (size_t)H * HD);
        vv = *reinterpret_cast<const uint4*>(p + (size_t)2 * H * HD);
      }
      kb[t][ks] = *reinterpret_cast<const bf16x8*>(&kv);
      vb[t][ks] = *reinterpret_cast<const bf16x8*>(&vv);
    }
  for (int idx = lane; idx < 32 * NCH; idx += 64) {
    const int r = idx / NCH, c8 = idx - r * NCH;
    const int key = kbase + r;
    uint4 kv = make_uint4(0, 0, 0, 0);
    if (key < T) kv = *reinterpret_cast<const uint4*>(qbase + (size_t)key * row + (size_t)H * HD + c8 * 8);
    *reinterpret_cast<uint4*>(mytile + r * LD + c8 * 8) = kv;
  }
  __builtin_amdgcn_s_waitcnt(0xc07f);                // lgkmcnt(0): a wave's LDS operations complete in order
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) kt[dt] = tr_cons(mytile, LD, 8 * g, 16 * dt, lane);
  __builtin_amdgcn_s_waitcnt(0xc07f);
  f32x4 dkt[2][NDT], dvt[2][NDT];                 // dK^T / dV^T [key tile][d tile]: rows d = 16 dt + 4 g + r
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
      dkt[t][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
      dvt[t][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }

  // ---- 32-query slices: Q / dO chunks and the row constants prefetched one slice ahead
  uint4 qreg[NST], dreg[NST];
  float rl = 0.f, rd = 0.f;
  auto load_slice = [&](int q0) {
#pragma unroll
    for (int i = 0; i < NST; ++i) {
      const int idx = tid + 256 * i;
      const int r = idx / NCHP, c8 = idx - r * NCHP;
      qreg[i] = make_uint4(0, 0, 0, 0);
      dreg[i] = make_uint4(0, 0, 0, 0);
      if (idx < 32 * NCHP && q0 + r < T && c8 < NCH) {
        qreg[i] = *reinterpret_cast<const uint4*>(qbase + (size_t)(q0 + r) * row + c8 * 8);
        dreg[i] = *reinterpret_cast<const uint4*>(dobase + (size_t)(q0 + r) * orow + c8 * 8);
      }
    }
    if (tid < 32) {
      rl = (q0 + tid < T) ? -lse[(size_t)bh * T + q0 + tid] / scale : 0.f;
      rd = (q0 + tid < T) ? -delta[(size_t)bh * T + q0 + tid] : 0.f;
    }
  };
  const float c2 = scale * AL_LOG2E;                 // P = exp2(c2 * S'),  S' = q.k - LSE / scale
  const int nslices = (T + 31) / 32;
  float* part = dq_part + ((size_t)bh * nkb + kblk) * T * HD;
  load_slice(0);
  for (int sl = 0; sl < nslices; ++sl) {
    const int q0 = 32 * sl;
#pragma unroll
    for (int i = 0; i < NST; ++i) {
      const int idx = tid + 256 * i;
      const int r = idx / NCHP, c8 = idx - r * NCHP;
      if (idx < 32 * NCHP) {
        *reinterpret_cast<uint4*>(Qs + r * LD + c8 * 8) = qreg[i];
        *reinterpret_cast<uint4*>(dOs + r * LD + c8 * 8) = dreg[i];
      }
    }
    if (tid < 32) {
      nlse[tid] = rl;
      ndel[tid] = rd;
    }
    lds_barrier();
    if (sl + 1 < nslices) load_slice(q0 + 32);
    f32x4 dq[2][NDT];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) dq[t][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (active) {
      // A operands (row reads): query 16 t + li, d = 32 ks + 8 g ..
      bf16x8 qa[2][NDS], da[2][NDS];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int ks = 0; ks < NDS; ++ks) {
          qa[t][ks] = *reinterpret_cast<const bf16x8*>(Qs + (16 * t + li) * LD + 32 * ks + 8 * g);
          da[t][ks] = *reinterpret_cast<const bf16x8*>(dOs + (16 * t + li) * LD + 32 * ks + 8 * g);
        }
      f32x4 c_lse[2], c_del[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        c_lse[t] = *reinterpret_cast<const f32x4*>(nlse + 16 * t + 4 * g);
        c_del[t] = *reinterpret_cast<const f32x4*>(ndel + 16 * t + 4 * g);
      }
      // S' and dP' of the 32 x 32 block [query tile tq][key tile tk]: rows = queries 4 g + r, column = key li
      f32x4 s[2][2], dp[2][2];
#pragma unroll
      for (int tq = 0; tq < 2; ++tq)
#pragma unroll
        for (int tk = 0; tk < 2; ++tk) {
          f32x4 a = c_lse[tq], d = c_del[tq];
#pragma unroll
          for (int ks = 0; ks < NDS; ++ks) {
            a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[tq][ks], kb[tk][ks], a, 0, 0, 0);
            d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(da[tq][ks], vb[tk][ks], d, 0, 0, 0);
          }
          s[tq][tk] = a;
          dp[tq][tk] = d;
        }
      // transposed operands (column reads): d = 16 dt + li, queries {4 g + r} and {16 + 4 g + r}
      bf16x8 qT[NDT], dT[NDT];
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        qT[dt] = tr_split(Qs, LD, 4 * g, 16 * dt, lane);
        dT[dt] = tr_split(dOs, LD, 4 * g, 16 * dt, lane);
      }
      bf16x8 pB[2], sB[2];
#pragma unroll
      for (int tk = 0; tk < 2; ++tk) {
        unsigned int pw[4], sw[4];
#pragma unroll
        for (int tq = 0; tq < 2; ++tq) {
          float p[4], ds[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            p[r] = __builtin_amdgcn_exp2f(c2 * s[tq][tk][r]);
            ds[r] = scale * p[r] * dp[tq][tk][r];
          }
          pw[2 * tq] = pack_bf16(p[0], p[1]);
          pw[2 * tq + 1] = pack_bf16(p[2], p[3]);
          sw[2 * tq] = pack_bf16(ds[0], ds[1]);
          sw[2 * tq + 1] = pack_bf16(ds[2], ds[3]);
          // dS tile for dQ: row = query 16 tq + 4 g + r, column = key 16 tk + li
#pragma unroll
          for (int r = 0; r < 4; r += 2) {
            const unsigned int w = sw[2 * tq + (r >> 1)];
            mytile[(16 * tq + 4 * g + r) * SLD + 16 * tk + li] = (unsigned short)(w & 0xffffu);
            mytile[(16 * tq + 4 * g + r + 1) * SLD + 16 * tk + li] = (unsigned short)(w >> 16);
          }
        }
        pB[tk] = *reinterpret_cast<const bf16x8*>(pw);
        sB[tk] = *reinterpret_cast<const bf16x8*>(sw);
      }
      // dV^T += dO^T P,  dK^T += Q^T dS
#pragma unroll
      for (int tk = 0; tk < 2; ++tk)
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
          dvt[tk][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dT[dt], pB[tk], dvt[tk][dt], 0, 0, 0);
          dkt[tk][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qT[dt], sB[tk], dkt[tk][dt], 0, 0, 0);
        }
      // dQ += dS K: A = dS rows from the wave's tile (query 16 tq + li, keys 8 g .. + 7)
      __builtin_amdgcn_s_waitcnt(0xc07f);
#pragma unroll
      for (int tq = 0; tq < 2; ++tq) {
        const bf16x8 sa = *reinterpret_cast<const bf16x8*>(mytile + (16 * tq + li) * SLD + 8 * g);
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
          dq[tq][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sa, kt[dt], dq[tq][dt], 0, 0, 0);
      }
    }
    // ---- this wave's dQ contribution: rows 16 tq + 4 g + r, column 16 dt + li
#pragma unroll
    for (int tq = 0; tq < 2; ++tq)
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) mydq[(16 * tq + 4 * g + r) * QLD + 16 * dt + li] = dq[tq][dt][r];
    lds_barrier();
    // ---- the block's partial: waves added in order, float4 stores of the rows < T
    for (int idx = tid; idx < 32 * (HD / 4); idx += 256) {
      const int r = idx / (HD / 4), c4 = idx - r * (HD / 4);
      if (q0 + r < T) {
        const float* src = dqs + r * QLD + 4 * c4;
        float4 v = *reinterpret_cast<const float4*>(src);
#pragma unroll
        for (int w = 1; w < 4; ++w) {
          const float4 u = *reinterpret_cast<const float4*>(src + w * 32 * QLD);
          v.x += u.x;
          v.y += u.y;
          v.z += u.z;
          v.w += u.w;
        }
        *reinterpret_cast<float4*>(part + (size_t)(q0 + r) * HD + 4 * c4) = v;
      }
    }
    // no barrier here: every wave has finished reading Qs / dOs (barrier above), and dqs is written again only after
    // the next slice's first barrier, which no thread reaches before its reads of dqs above
  }

  // ---- dK / dV of this wave's keys: accumulator rows d = 16 dt + 4 g + r, column = key
  if (active) {
    unsigned short* dbase = dqkv + (size_t)b * T * row + (size_t)h * HD;
#pragma unroll
    for (int tk = 0; tk < 2; ++tk) {
      const int key = kbase + 16 * tk + li;
      if (key < T) {
        unsigned short* pk = dbase + (size_t)key * row + (size_t)H * HD + 4 * g;
        unsigned short* pv = dbase + (size_t)key * row + (size_t)2 * H * HD + 4 * g;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
          uint2 wk, wv;
          wk.x = pack_bf16(dkt[tk][dt][0], dkt[tk][dt][1]);
          wk.y = pack_bf16(dkt[tk][dt][2], dkt[tk][dt][3]);
          wv.x = pack_bf16(dvt[tk][dt][0], dvt[tk][dt][1]);
          wv.y = pack_bf16(dvt[tk][dt][2], dvt[tk][dt][3]);
          *reinterpret_cast<uint2*>(pk + 16 * dt) = wk;
          *reinterpret_cast<uint2*>(pv + 16 * dt) = wv;
        }
      }
    }
  }
}

// dQ = sum over the key blocks of the partials, in key-block order -> bf16 Q slice of dqkv.  One thread per
// (b, t, h, 8 columns).
template <int HD>
__global__ __launch_bounds__(256) void attn_long_dq_kernel(const float* __restrict__ dq_part, int B, int T, int H,
                                                           int nkb, unsigned short* __restrict__ dqkv) {
  constexpr int NC = HD / 8;
  const int64_t n = (int64_t)B * T * H * NC;
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int c8 = (int)(i % NC);
    int64_t rest = i / NC;
    const int h = (int)(rest % H);
    rest /= H;
    const int t = (int)(rest % T), b = (int)(rest / T);
    const float* src = dq_part + (((size_t)b * H + h) * nkb * T + t) * HD + 8 * c8;
    float4 a = *reinterpret_cast<const float4*>(src), c = *reinterpret_cast<const float4*>(src + 4);
    for (int k = 1; k < nkb; ++k) {
      const float4 u = *reinterpret_cast<const float4*>(src + (size_t)k * T * HD);
      const float4 v = *reinterpret_cast<const float4*>(src + (size_t)k * T * HD + 4);
      a.x += u.x; a.y += u.y; a.z += u.z; a.w += u.w;
      c.x += v.x; c.y += v.y; c.z += v.z; c.w += v.w;
    }
    uint4 w;
    w.x = pack_bf16(a.x, a.y);
    w.y = pack_bf16(a.z, a.w);
    w.z = pack_bf16(c.x, c.y);
    w.w = pack_bf16(c.z, c.w);
    *reinterpret_cast<uint4*>(dqkv + (((size_t)b * T + t) * 3 * H + h) * HD + 8 * c8) = w;
  }
}

static inline int al_grid(int64_t n) {
  const int64_t blocks = (n + 255) / 256;
  return (int)(blocks < 8192 ? (blocks < 1 ? 1 : blocks) : 8192);
}

static inline int64_t al_a256(int64_t x) { return (x + 255) & ~(int64_t)255; }

// the main pass (out given), the CLS tap (cls given) and, without a position scheme, the query-mean tap (qmean given)
template <int HD, AttnPos POS = AttnPos::None>
static void launch_fwd_long(const void* qkv, int B, int T, int H, float scale, void* out, float* cls, float* qmean,
                            float* lse, void* stream, AttnPosArg pos = AttnPosArg{nullptr, 0, 0}) {
  hipStream_t st = (hipStream_t)stream;
  const unsigned short* p = (const unsigned short*)qkv;
  if (out != nullptr)
    hipLaunchKernelGGL((attn_long_fwd_kernel<HD, POS>), dim3(B * H, (T + 63) / 64), dim3(256), 0, st, p, T, H, scale,
                       (unsigned short*)out, lse, pos);
  if (cls != nullptr)
    hipLaunchKernelGGL((attn_long_cls_kernel<HD, POS>), dim3(B * H), dim3(256), 0, st, p, T, H, scale, cls, pos);
  if constexpr (POS == AttnPos::None)
    if (qmean != nullptr)
      hipLaunchKernelGGL(attn_long_qmean_kernel<HD>, dim3(B * H, (T + 63) / 64), dim3(256), 0, st, p, T, H, scale,
                         (const float*)lse, qmean);
}

template <int HD>
static void launch_bwd_long(const void* qkv, const void* out, const void* dout, const float* lse, int B, int T, int H,
                            float scale, void* dqkv, float* delta, float* part, hipStream_t st) {
  const int nkb = (T + 127) / 128;
  hipLaunchKernelGGL(attn_long_delta_kernel<HD>, dim3(al_grid((int64_t)B * T * H)), dim3(256), 0, st,
                     (const unsigned short*)out, (const unsigned short*)dout, B, T, H, delta);
  allow_full_lds((const void*)attn_long_bwd_kernel<HD>);
  hipLaunchKernelGGL(attn_long_bwd_kernel<HD>, dim3(B * H, nkb), dim3(256), AlBwdCfg<HD>::LDS, st,
                     (const unsigned short*)qkv, (const unsigned short*)dout, lse, (const float*)delta,
                     (unsigned short*)dqkv, part, T, H, scale);
  hipLaunchKernelGGL(attn_long_dq_kernel<HD>, dim3(al_grid((int64_t)B * T * H * (HD / 8))), dim3(256), 0, st,
                     (const float*)part, B, T, H, nkb, (unsigned short*)dqkv);
}

}  // namespace basd

extern "C" int basd_attention_fwd_long_bf16(const void* qkv, int B, int T, int H, int hd, float scale, void* out,
                                            float* cls_importance, float* qmean_importance, float* lse, void* stream) {
  using namespace basd;
  if (B <= 0) return BASD_OK;
  if ((hd != 64 && hd != 80) || T < 1 || T > AL_MAXT || H < 1)
    return fail(BASD_ERR_SHAPE, "attention_fwd_long: T=%d H=%d hd=%d unsupported (hd 64 | 80, 1 <= T <= %d)", T, H,
                hd, AL_MAXT);
  if (cls_importance != nullptr && T < 2) return fail(BASD_ERR_SHAPE, "attention_fwd_long: the CLS tap needs T >= 2");
  if (qmean_importance != nullptr && (out == nullptr || lse == nullptr))
    return fail(BASD_ERR_SHAPE, "attention_fwd_long: the query-mean tap needs out and lse");
  if (hd == 64) launch_fwd_long<64>(qkv, B, T, H, scale, out, cls_importance, qmean_importance, lse, stream);
  else launch_fwd_long<80>(qkv, B, T, H, scale, out, cls_importance, qmean_importance, lse, stream);
  return check_launch("attention_fwd_long");
}

extern "C" int basd_attention_fwd_long_rope_bf16(const void* qkv, const float* rope, int B, int T, int H, int hd,
                                                 float scale, void* out, float* cls_importance, void* stream) {
  using namespace basd;
  if (hd != 64 || T < 2 || T > AL_MAXT || H < 1 || B < 1 || rope == nullptr)
    return fail(BASD_ERR_SHAPE, "attention_fwd_long_rope: B=%d T=%d H=%d hd=%d rope=%s unsupported (hd 64, 2 <= T <= %d, "
                                "B, H >= 1, a table)", B, T, H, hd, rope == nullptr ? "NULL" : "given", AL_MAXT);
  launch_fwd_long<64, AttnPos::Rope>(qkv, B, T, H, scale, out, cls_importance, nullptr, nullptr, stream,
                                     AttnPosArg{rope, 0, 0});
  return check_launch("attention_fwd_long_rope");
}

extern "C" int basd_attention_fwd_long_relbias_bf16(const void* qkv, const float* table, int B, int gh, int gw, int H,
                                                    int hd, float scale, void* out, float* cls_importance,
                                                    void* stream) {
  using namespace basd;
  const int64_t T64 = (gh >= 1 && gw >= 1) ? (int64_t)gh * gw + 1 : 0;
  if (hd != 64 || T64 < 2 || T64 > AL_MAXT || H < 1 || B < 1 || qkv == nullptr || table == nullptr || out == nullptr ||
      !(scale > 0.f) || !(scale <= 3.0e38f))
    return fail(BASD_ERR_SHAPE, "attention_fwd_long_relbias: B=%d grid %d x %d H=%d hd=%d scale=%g qkv / table / out=%s unsupported "
                                "(hd 64, 2 <= gh * gw + 1 <= %d, B, H >= 1, the three pointers, a finite scale > 0)",
                B, gh, gw, H, hd, (double)scale,
                (qkv == nullptr || table == nullptr || out == nullptr) ? "a NULL" : "given", AL_MAXT);
  launch_fwd_long<64, AttnPos::RelBias>(qkv, B, (int)T64, H, scale, out, cls_importance, nullptr, nullptr, stream,
                                        AttnPosArg{table, gh, gw});
  return check_launch("attention_fwd_long_relbias");
}

extern "C" int64_t basd_attention_bwd_long_workspace_bytes(int B, int T, int H, int hd) {
  using namespace basd;
  if (B < 1 || T < 1 || H < 1 || hd < 1) return 256;
  const int64_t bh = (int64_t)B * H, nkb = (T + 127) / 128;
  return 256 + al_a256(bh * T * 4) + al_a256(bh * nkb * T * hd * 4);
}

extern "C" int basd_attention_bwd_long_bf16(const void* qkv, const void* out, const void* dout, const float* lse, int B,
                                            int T, int H, int hd, float scale, void* dqkv, void* workspace,
                                            int64_t workspace_bytes, void* stream) {
  using namespace basd;
  if (B <= 0) return BASD_OK;
  if ((hd != 64 && hd != 80) || T < 1 || T > AL_MAXT || H < 1)
    return fail(BASD_ERR_SHAPE, "attention_bwd_long: T=%d H=%d hd=%d unsupported (hd 64 | 80, 1 <= T <= %d)", T, H,
                hd, AL_MAXT);
  const int64_t need = basd_attention_bwd_long_workspace_bytes(B, T, H, hd);
  if (workspace == nullptr || workspace_bytes < need)
    return fail(BASD_ERR_WORKSPACE, "attention_bwd_long: workspace of %lld bytes, need %lld",
                (long long)workspace_bytes, (long long)need);
  const uintptr_t w0 = (((uintptr_t)workspace) + 255) & ~(uintptr_t)255;
  float* delta = reinterpret_cast<float*>(w0);
  float* part = reinterpret_cast<float*>(w0 + al_a256((int64_t)B * H * T * 4));
  hipStream_t st = (hipStream_t)stream;
  if (hd == 64) launch_bwd_long<64>(qkv, out, dout, lse, B, T, H, scale, dqkv, delta, part, st);
  else launch_bwd_long<80>(qkv, out, dout, lse, B, T, H, scale, dqkv, delta, part, st);
  return check_launch("attention_bwd_long");
}
