// Fused attention backward for the student's MHSA blocks (reference src/training/trainer.py:157: autograd through
// timm Attention.forward).  Inputs: the packed projection qkv [B, T, 3, H, 64] bf16, the forward output
// O [B, T, H * 64] bf16, its gradient dO (same layout) and the forward's log-sum-exp LSE [B, H, T] fp32 (natural
// log of sum_k exp(scale * q.k), written by basd_attention_fwd_bf16).  Output: dqkv [B, T, 3, H, 64] bf16, the
// gradient of the packed projection (what the qkv Linear's backward consumes, no stack / transpose copies).
// Replaces the library's Triton-built flash-attention backward (three kernels, 0.86 TB/s effective).
//
// P is recomputed from Q, K and LSE (nothing of size T x T is ever stored).  One workgroup per (image, head); T <= 224
// tokens are NP pairs of 16-row tiles.  With S = Q K^T and dP = dO V^T computed KEY-ON-THE-LANE (A = query rows,
// B = key rows: accumulator rows = 4 queries per lane, column = key), the bf16-packed accumulators of a 32-query step
// ARE the B operands of
//     dV^T[d][key] += dO^T[d][q] P[q][key]      dK^T[d][key] += Q^T[d][q] dS[q][key]
// (A = dO^T / Q^T through the transposing LDS read ds_read_b64_tr_b16: no transpose of P, dS, Q or dO); only dS
// crosses LDS once: written TRANSPOSED (row = key: 8-byte stores) into a wave-private 32 x 32 tile and read back through
// the transposing read as the B operand of dQ^T[d][q] += K^T[d][key] dS^T[key][q], whose accumulator holds four
// consecutive d of one query: the fp32 dQ image in LDS is read (as the initial accumulator) and written 16 bytes a lane.
// The row constants -LSE / scale and -delta (delta = rowsum(dO * O)) are the INITIAL accumulators of S and dP, so
// P = exp2(c * S') and dS = scale * P * dP' need no subtraction and no running maximum.
//
// Work split: ONE key pair per wave.  Wave w owns key pair w: its K / V / K^T fragments and dK^T / dV^T accumulators
// (112 registers) stay in registers for the whole kernel.  T > 96: NP = 7, 8 waves (two per SIMD; wave 7 only keeps the
// barriers company), T <= 96: NP = 3, 4 waves, two workgroups per CU.  npl = ceil(T / 32) pairs hold tokens: waves
// w >= npl do nothing, the others walk the npl query pairs staggered (pair (step + w) mod npl at step `step`), so the
// waves always update DIFFERENT rows of the dQ image: plain read-modify-write, one barrier per step, no atomics, and the
// order in which a dQ row is summed is a function of (step, wave) alone: results are bitwise reproducible.  Step 0 covers
// every pair once and stores, so the image is never zeroed.
//
// Prologue: every global load (Q, dO, O, LSE of the head, K and V of the wave's pair) is issued before the first LDS
// store: one HBM round trip before the first MFMA (it was about nine).  K^T comes from the K fragments through a
// wave-private tile that aliases the not yet used dQ image.  Tail: dK and dV go through the wave's own 32 rows of the
// (dead) Q and dO images so that 8 lanes store one whole 128-byte row segment.
//
// Compiler resource report (gfx950): NP = 7: 252 VGPRs, no scratch, 2 waves per SIMD, 143 360 B of LDS (one workgroup per
// CU); NP = 3: 248 VGPRs, no scratch, 61 440 B of LDS.  Measured (MI355X, kernel trace, B 256, T 197, H 3): 63.5 us per
// launch, 2.45 TB/s over the algorithmic 155.5 MB (the two-key-pairs-per-wave, one-wave-per-SIMD version: 85 us); B 64,
// T 65, H 3: 8.5 us (11.1).  Tried and kept out: 8 waves for NP = 3 (8.1 .. 9.0 us: no better than 4).
#include "basd_frag.h"

namespace basd {

constexpr int AB_HD = 64;
constexpr int AB_LD = AB_HD + 8;          // bf16 row stride of the Q / dO / K images (144 B)
constexpr int AB_SLD = 36;                // bf16 row stride of the wave-private dS^T tile (72 B: 8-byte stores of 16 lanes hit 32 banks)
constexpr int AB_QLD = 68;                // fp32 row stride of the dQ image (272 B)

template <int NP, int NW>   // pairs of 16-row tiles: T <= 32 * NP; waves per workgroup (NW > NP never work: barriers only)
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(2, 2))) void attention_bwd_kernel(
    const unsigned short* __restrict__ qkv, const unsigned short* __restrict__ out,
    const unsigned short* __restrict__ dout, const float* __restrict__ lse, unsigned short* __restrict__ dqkv, int T,
    int H, float scale) {
  constexpr int TP = 32 * NP;                        // padded token count
  constexpr int NT = 64 * NW;
  constexpr int NLD = (TP * 8 + NT - 1) / NT;        // 16-byte chunks of Q (dO, O) per thread
  static_assert(NW >= NP, "one key pair per wave");
  static_assert(NP * 32 * AB_LD * 2 <= TP * AB_QLD * 4, "the K staging tiles alias the dQ image");
  extern __shared__ __align__(16) unsigned char ab_smem[];
  unsigned short* Qs = reinterpret_cast<unsigned short*>(ab_smem);                 // [TP][AB_LD]
  unsigned short* dOs = Qs + TP * AB_LD;                                            // [TP][AB_LD]
  float* dQs = reinterpret_cast<float*>(dOs + TP * AB_LD);                          // [TP][AB_QLD]
  float* nlse = dQs + TP * AB_QLD;                                                  // [TP]  -LSE / scale
  float* ndel = nlse + TP;                                                          // [TP]  -delta
  unsigned short* wtile = reinterpret_cast<unsigned short*>(ndel + TP);             // [NP waves][32][AB_SLD]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int b = blockIdx.x / H, h = blockIdx.x - b * H;
  const size_t row = (size_t)3 * H * AB_HD;          // elements per token of qkv
  const size_t orow = (size_t)H * AB_HD;             // elements per token of O / dO
  const unsigned short* qbase = qkv + (size_t)b * T * row + (size_t)h * AB_HD;
  const unsigned short* obase = out + (size_t)b * T * orow + (size_t)h * AB_HD;
  const unsigned short* dobase = dout + (size_t)b * T * orow + (size_t)h * AB_HD;
  const int npl = (T + 31) >> 5;                     // query / key pairs that hold tokens
  const bool live = wave < npl;                      // this wave owns key pair `wave`

  // ---- every global load of the prologue is issued before the first LDS store (one HBM round trip, as in
  //      attention.hip): Q, dO, O and LSE of the head, and the K / V fragments of the wave's key pair
  uint4 qreg[NLD], dreg[NLD], oreg[NLD];
  float lreg[NLD];
#pragma unroll
  for (int i = 0; i < NLD; ++i) {
    const int idx = tid + NT * i, r = idx >> 3, c8 = idx & 7;
    qreg[i] = make_uint4(0, 0, 0, 0);
    dreg[i] = make_uint4(0, 0, 0, 0);
    oreg[i] = make_uint4(0, 0, 0, 0);
    lreg[i] = 0.f;
    if (r < T) {
      qreg[i] = *reinterpret_cast<const uint4*>(qbase + (size_t)r * row + c8 * 8);
      dreg[i] = *reinterpret_cast<const uint4*>(dobase + (size_t)r * orow + c8 * 8);
      oreg[i] = *reinterpret_cast<const uint4*>(obase + (size_t)r * orow + c8 * 8);
      if (c8 == 0) lreg[i] = lse[((size_t)b * H + h) * T + r];
    }
  }
  // B operands of S / dP: lane holds key 32 wave + 16 t + li, d = 32 ks + 8 g .. + 7 (16-byte global loads)
  bf16x8 kb[2][2], vb[2][2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int key = 32 * wave + 16 * t + li;
      uint4 kv = make_uint4(0, 0, 0, 0), vv = make_uint4(0, 0, 0, 0);
      if (key < T) {
        const unsigned short* p = qbase + (size_t)key * row + 32 * ks + 8 * g;
        kv = *reinterpret_cast<const uint4*>(p + (size_t)H * AB_HD);
        vv = *reinterpret_cast<const uint4*>(p + (size_t)2 * H * AB_HD);
      }
      kb[t][ks] = *reinterpret_cast<const bf16x8*>(&kv);
      vb[t][ks] = *reinterpret_cast<const bf16x8*>(&vv);
    }

  // ---- Q and dO images (rows >= T zero), delta = rowsum(dO * O), -LSE / scale
#pragma unroll
  for (int i = 0; i < NLD; ++i) {
    const int idx = tid + NT * i, r = idx >> 3, c8 = idx & 7;
    const unsigned int* dw = reinterpret_cast<const unsigned int*>(&dreg[i]);
    const unsigned int* ow = reinterpret_cast<const unsigned int*>(&oreg[i]);
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      s = fmaf(__uint_as_float(dw[e] << 16), __uint_as_float(ow[e] << 16), s);
      s = fmaf(__uint_as_float(dw[e] & 0xffff0000u), __uint_as_float(ow[e] & 0xffff0000u), s);
    }
    // the 8 chunks of a row sit in 8 consecutive lanes
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    if (idx < TP * 8) {
      *reinterpret_cast<uint4*>(Qs + r * AB_LD + c8 * 8) = qreg[i];
      *reinterpret_cast<uint4*>(dOs + r * AB_LD + c8 * 8) = dreg[i];
      if (c8 == 0) {
        ndel[r] = -s;
        nlse[r] = -lreg[i] / scale;
      }
    }
  }
  // A operand of dQ^T += K^T dS^T: lane holds d = 16 dt + li, keys 8 g .. + 7 of the pair.  The K fragments above ARE
  // the pair's row-major tile (row 16 t + li, columns 32 ks + 8 g .. + 7): it goes through a wave-private tile inside
  // the (not yet used) dQ image and comes back through the transposing read
  bf16x8 kt[4] = {};
  if (wave < NP) {
    unsigned short* kst = reinterpret_cast<unsigned short*>(dQs) + wave * 32 * AB_LD;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
        *reinterpret_cast<bf16x8*>(kst + (16 * t + li) * AB_LD + 32 * ks + 8 * g) = kb[t][ks];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) kt[dt] = tr_cons(kst, AB_LD, 8 * g, 16 * dt, lane);
  }
  f32x4 dkt[2][4], dvt[2][4];                     // dK^T / dV^T [key tile][d tile]: rows d = 4 g + r, column key li
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      dkt[t][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
      dvt[t][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
  __syncthreads();                                   // the images are complete; every kt read has returned

  const float c2 = scale * 1.4426950408889634f;      // P = exp2(c2 * S'),  S' = q.k - LSE / scale
  unsigned short* mytile = wtile + (live ? wave : 0) * 32 * AB_SLD;
#pragma unroll 1
  for (int step = 0; step < npl; ++step) {
    int qp = step + wave;                            // live waves are on npl different query pairs at every step
    if (qp >= npl) qp -= npl;
    if (live) {
      const int q0 = 32 * qp;
      // A operands (row reads): query q0 + 16 t + li, d = 32 ks + 8 g .. + 7
      bf16x8 qa[2][2], da[2][2];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          qa[t][ks] = *reinterpret_cast<const bf16x8*>(Qs + (q0 + 16 * t + li) * AB_LD + 32 * ks + 8 * g);
          da[t][ks] = *reinterpret_cast<const bf16x8*>(dOs + (q0 + 16 * t + li) * AB_LD + 32 * ks + 8 * g);
        }
      // row constants of the two query tiles: rows 4 g + r
      f32x4 c_lse[2], c_del[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        c_lse[t] = *reinterpret_cast<const f32x4*>(nlse + q0 + 16 * t + 4 * g);
        c_del[t] = *reinterpret_cast<const f32x4*>(ndel + q0 + 16 * t + 4 * g);
      }
      // transposed operands (column reads): d = 16 dt + li, queries {q0 + 4 g + r} and {q0 + 16 + 4 g + r}
      bf16x8 qT[4], dT[4];
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        qT[dt] = tr_split(Qs, AB_LD, q0 + 4 * g, 16 * dt, lane);
        dT[dt] = tr_split(dOs, AB_LD, q0 + 4 * g, 16 * dt, lane);
      }
      // the pair's rows of the dQ image, as the initial accumulators of dQ^T below: row = query 16 tq + li, FOUR
      // CONSECUTIVE d (16 dt + 4 g + r) per lane, 16-byte accesses.  No other wave is on this query pair during the
      // step.  Step 0 starts from zero and so overwrites (it covers every pair that holds tokens: the image is never
      // zeroed).
      f32x4 dq[2][4];
      float* dqrow = dQs + (q0 + li) * AB_QLD + 4 * g;
#pragma unroll
      for (int tq = 0; tq < 2; ++tq)
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) dq[tq][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (step != 0) {
#pragma unroll
        for (int tq = 0; tq < 2; ++tq)
#pragma unroll
          for (int dt = 0; dt < 4; ++dt)
            dq[tq][dt] = *reinterpret_cast<const f32x4*>(dqrow + 16 * tq * AB_QLD + 16 * dt);
      }
      // S' and dP' of the 32 x 32 block: [query tile tq][key tile tk]
      f32x4 s[2][2], dp[2][2];
#pragma unroll
      for (int tq = 0; tq < 2; ++tq)
#pragma unroll
        for (int tk = 0; tk < 2; ++tk) {
          f32x4 a = c_lse[tq], d = c_del[tq];
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[tq][ks], kb[tk][ks], a, 0, 0, 0);
            d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(da[tq][ks], vb[tk][ks], d, 0, 0, 0);
          }
          s[tq][tk] = a;
          dp[tq][tk] = d;
        }
      // P and dS; packed as B operands: element j of lane group g <-> query 16 (j >> 2) + 4 g + (j & 3)
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
          // dS^T tile for dQ: row = key 16 tk + li, columns = queries 16 tq + 4 g .. + 3 (one 8-byte store)
          *reinterpret_cast<uint2*>(mytile + (16 * tk + li) * AB_SLD + 16 * tq + 4 * g) =
              make_uint2(sw[2 * tq], sw[2 * tq + 1]);
        }
        pB[tk] = *reinterpret_cast<const bf16x8*>(pw);
        sB[tk] = *reinterpret_cast<const bf16x8*>(sw);
      }
      // dV^T += dO^T P,  dK^T += Q^T dS
#pragma unroll
      for (int tk = 0; tk < 2; ++tk)
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          dvt[tk][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dT[dt], pB[tk], dvt[tk][dt], 0, 0, 0);
          dkt[tk][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qT[dt], sB[tk], dkt[tk][dt], 0, 0, 0);
        }
      // dQ^T += K^T dS^T: B = dS^T through the transposing read (query 16 tq + li, keys 8 g .. + 7; a wave's LDS
      // operations complete in order)
#pragma unroll
      for (int tq = 0; tq < 2; ++tq) {
        const bf16x8 sa = tr_cons(mytile, AB_SLD, 8 * g, 16 * tq, lane);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          dq[tq][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kt[dt], sa, dq[tq][dt], 0, 0, 0);
          *reinterpret_cast<f32x4*>(dqrow + 16 * tq * AB_QLD + 16 * dt) = dq[tq][dt];
        }
      }
    }
    __syncthreads();
  }

  // ---- write dK / dV: the wave's 32 keys x 64 d tiles go through LDS (its own 32 rows of the Q and dO images, dead
  //      after the last barrier) so that 8 lanes store one whole 128-byte row segment
  unsigned short* dbase = dqkv + (size_t)b * T * row + (size_t)h * AB_HD;
  if (live) {
    unsigned short* kst = Qs + wave * 32 * AB_LD;
    unsigned short* vst = dOs + wave * 32 * AB_LD;
    // accumulator rows d = 16 dt + 4 g + r (4 consecutive), column = key 16 tk + li
#pragma unroll
    for (int tk = 0; tk < 2; ++tk)
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        *reinterpret_cast<uint2*>(kst + (16 * tk + li) * AB_LD + 16 * dt + 4 * g) =
            make_uint2(pack_bf16(dkt[tk][dt][0], dkt[tk][dt][1]), pack_bf16(dkt[tk][dt][2], dkt[tk][dt][3]));
        *reinterpret_cast<uint2*>(vst + (16 * tk + li) * AB_LD + 16 * dt + 4 * g) =
            make_uint2(pack_bf16(dvt[tk][dt][0], dvt[tk][dt][1]), pack_bf16(dvt[tk][dt][2], dvt[tk][dt][3]));
      }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int idx = lane + 64 * c, r = idx >> 3, c8 = idx & 7;
      const int key = 32 * wave + r;
      const uint4 wk = *reinterpret_cast<const uint4*>(kst + r * AB_LD + c8 * 8);
      const uint4 wv = *reinterpret_cast<const uint4*>(vst + r * AB_LD + c8 * 8);
      if (key < T) {
        *reinterpret_cast<uint4*>(dbase + (size_t)key * row + (size_t)H * AB_HD + c8 * 8) = wk;
        *reinterpret_cast<uint4*>(dbase + (size_t)key * row + (size_t)2 * H * AB_HD + c8 * 8) = wv;
      }
    }
  }
  // ---- write dQ from the fp32 image: 16 bytes (8 bf16) per lane
  for (int idx = tid; idx < T * 8; idx += NT) {
    const int r = idx >> 3, c8 = idx & 7;
    const float4 a = *reinterpret_cast<const float4*>(dQs + r * AB_QLD + c8 * 8);
    const float4 c = *reinterpret_cast<const float4*>(dQs + r * AB_QLD + c8 * 8 + 4);
    uint4 w;
    w.x = pack_bf16(a.x, a.y);
    w.y = pack_bf16(a.z, a.w);
    w.z = pack_bf16(c.x, c.y);
    w.w = pack_bf16(c.z, c.w);
    *reinterpret_cast<uint4*>(dbase + (size_t)r * row + c8 * 8) = w;
  }
}

template <int NP, int NW>
static void launch_attention_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int B,
                                 int T, int H, float scale, hipStream_t st) {
  constexpr int TP = 32 * NP;
  const size_t lds = (size_t)2 * TP * AB_LD * 2 + (size_t)TP * AB_QLD * 4 + (size_t)2 * TP * 4 + (size_t)NP * 32 * AB_SLD * 2;
  allow_full_lds((const void*)attention_bwd_kernel<NP, NW>);
  hipLaunchKernelGGL((attention_bwd_kernel<NP, NW>), dim3(B * H), dim3(64 * NW), lds, st, (const unsigned short*)qkv,
                     (const unsigned short*)out, (const unsigned short*)dout, lse, (unsigned short*)dqkv, T, H, scale);
}

}  // namespace basd

extern "C" int basd_attention_bwd_bf16(const void* qkv, const void* out, const void* dout, const float* lse, int B,
                                       int T, int H, int hd, float scale, void* dqkv, void* stream) {
  using namespace basd;
  if (B <= 0) return BASD_OK;
  if (hd != AB_HD || T < 1 || T > 224 || H < 1)
    return fail(BASD_ERR_SHAPE, "attention_bwd: T=%d H=%d hd=%d unsupported (hd 64, T <= 224)", T, H, hd);
  hipStream_t st = (hipStream_t)stream;
  if (T <= 96) launch_attention_bwd<3, 4>(qkv, out, dout, lse, dqkv, B, T, H, scale, st);
  else launch_attention_bwd<7, 8>(qkv, out, dout, lse, dqkv, B, T, H, scale, st);
  return check_launch("attention_bwd");
}
