// Kernels of the frozen ResNet teacher trunk (models/cnn.py): everything that is not a 1 x 1 convolution (those are
// basd_gemm_bf16 on the channels-last rows, BatchNorm folded into weight and bias).
//
// Activations use the layout of csrc/convnext.hip: a feature map [B, H, W, C] is a [B H W, ld] bf16 matrix, ld >= C,
// columns C .. ld written as zero and never read (the 64-channel maps live in rows of 128, the narrowest N of the GEMM).
//
//   basd_conv3x3_bf16          3 x 3, padding 1, stride 1 / 2, C -> C: implicit GEMM on the bf16 matrix cores.  The K
//                              axis is (tap, channel): channels-last makes every tap's slice of a pixel a contiguous
//                              run of channels, so an operand row is gathered with 16-byte loads and the im2col
//                              matrix exists only as one 128 x 64 LDS tile at a time.
//   basd_conv7x7s2_relu_bf16   the stem (3 -> 64, K = 147): the patch matrix of 128 output pixels is gathered
//                              element-wise into LDS (the input is read through strides: NCHW or channels-last),
//                              then 5 k-blocks of MFMA.  3 % of the trunk's FLOPs.
//   basd_maxpool3x3s2_bf16, basd_add_relu_bf16
//                              16 bytes (8 channels) per lane, exact.
//
// LDS operand image (both matrix kernels): [16 rows][32 k] bf16 sub-tiles of 1 KiB with the XOR swizzle of
// gemm_bf16.hip (byte ^= ((byte >> 9) & 1) << 5), which keeps the 16 lanes a ds_read_b128 services together on 16
// different 16-byte slots.  Both operands are k-contiguous per row, so a fragment is one ds_read_b128 and no
// transposing read is needed.  The weight tile is the MFMA's A operand and the pixel tile its B operand: a lane then
// owns 4 consecutive output channels of one pixel (as in the GEMM).
#include "basd_frag.h"

namespace basd {

__device__ __forceinline__ int rn_swz(int byte) { return byte ^ (((byte >> 9) & 1) << 5); }

// byte offset of (row, 16-byte k chunk c) in an image of sub-tiles, `kblocks` sub-tiles per 16-row block
__device__ __forceinline__ int rn_img(int row, int c, int kblocks) {
  return ((row >> 4) * kblocks + (c >> 2)) * 1024 + rn_swz((row & 15) * 64 + (c & 3) * 16);
}

// max(0, .) on two packed bf16: a set sign bit clears its half
__device__ __forceinline__ u32x4 relu_pk8(u32x4 w) {
  return w & ~(((w >> 15) & 0x00010001u) * 0xffffu);
}

// ---------------------------------------------------------------------------------------------------------------------
// 3 x 3 convolution.  Workgroup = 256 threads = 4 waves (2 along m x 2 along n), output tile 128 pixels x BN channels
// (BN = 128 when C % 128 == 0, else 64), K step = 64 channels of one tap: 9 C / 64 steps.  Two LDS stages; the operands of
// step t + 1 are loaded into registers (ReLU applied there) before the MFMAs of step t and stored behind them: one
// barrier per step.  A thread stages the same 4 pixels (rows r0 + 32 i, 16-byte chunk tid & 7) in every step, so the
// pixel decode is done once; a tap outside the image (or a row behind M) stages zeros.
// Tile order as the GEMM: the n tiles of one pixel block are neighbours on ONE XCD (they re-read the same pixels from
// its L2).
constexpr int CV_BM = 128;
constexpr int CV_A_BYTES = CV_BM * 64 * 2;

template <int BN>
__global__ __launch_bounds__(256) void conv3x3_kernel(const unsigned short* __restrict__ x,
                                                      const unsigned short* __restrict__ w9,
                                                      const unsigned short* __restrict__ bias,
                                                      unsigned short* __restrict__ y, int H, int W, int Ho, int Wo,
                                                      int C, int stride, int ld_in, int ld_out, int relu_in,
                                                      int relu_out, int64_t M, int mblocks, int tiles_n) {
  constexpr int W_BYTES = BN * 64 * 2;
  constexpr int STAGE = CV_A_BYTES + W_BYTES;
  constexpr int NT = BN / 32;                      // 16-wide n tiles of a wave (it owns 64 pixels x BN / 2 channels)
  constexpr int WPT = BN / 32;                     // 16-byte weight pieces per thread and step
  constexpr int ROWB = BN * 2 + 16;                // row stride of the epilogue image
  static_assert(2 * STAGE >= CV_BM * ROWB, "the epilogue image fits the operand stages");
  __shared__ __align__(16) unsigned char lds[2 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
  const int nb = idx % tiles_n, mb = (idx / tiles_n) * 8 + xcd;
  if (mb >= mblocks) return;
  const int64_t m0 = (int64_t)mb * CV_BM;
  const int n0 = nb * BN;

  // ---- staging coordinates
  const int ac = tid & 7, r0 = tid >> 3;
  const unsigned short* xb[4];
  int ih0[4], iw0[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = (int)m0 + r0 + 32 * i;            // M < 2^31 (checked by the entry)
    xb[i] = x;
    ih0[i] = -4;                                    // a row behind M: every tap is out of bounds
    iw0[i] = -4;
    if (m < M) {
      const int ow = m % Wo, q = m / Wo;
      const int oh = q % Ho, b = q / Ho;
      ih0[i] = oh * stride - 1;
      iw0[i] = ow * stride - 1;
      xb[i] = x + (int64_t)b * H * W * ld_in + ac * 8;
    }
  }
  const int a_dst = rn_img(r0, ac, 2);             // + i * 4096: row r0 + 32 i is two 16-row blocks further
  const int w_dst = CV_A_BYTES + a_dst;
  const int K9 = 9 * C;
  const unsigned short* wsrc = w9 + (size_t)(n0 + r0) * K9 + ac * 8;

  u32x4 areg[4], wreg[WPT];
  auto load = [&](int t, int dy, int dx, int c0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ih = ih0[i] + dy, iw = iw0[i] + dx;
      areg[i] = (u32x4){0u, 0u, 0u, 0u};
      if ((unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W)
        areg[i] = *reinterpret_cast<const u32x4*>(xb[i] + ((int64_t)ih * W + iw) * ld_in + c0);
    }
#pragma unroll
    for (int i = 0; i < WPT; ++i)
      wreg[i] = *reinterpret_cast<const u32x4*>(wsrc + (size_t)i * 32 * K9 + (size_t)t * 64);   // tap C + c0 = 64 t
  };
  auto store = [&](int stage) {
    unsigned char* base = lds + stage * STAGE;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      *reinterpret_cast<u32x4*>(base + a_dst + i * 4096) = relu_in ? relu_pk8(areg[i]) : areg[i];
#pragma unroll
    for (int i = 0; i < WPT; ++i) *reinterpret_cast<u32x4*>(base + w_dst + i * 4096) = wreg[i];
  };

  f32x4 acc[NT][4];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int frag_off = rn_swz((lane & 15) * 64 + (lane >> 4) * 16);
  const int a_sub0 = (wm * 4) * 2;
  const int b_sub0 = (wn * NT) * 2;

  const int nsteps = 9 * (C >> 6);
  int dy = 0, dx = 0, c0 = 0;                      // coordinates of the step being loaded
  auto advance = [&]() {
    c0 += 64;
    if (c0 == C) {
      c0 = 0;
      if (++dx == 3) { dx = 0; ++dy; }
    }
  };
  load(0, dy, dx, c0);
  advance();
  store(0);
  __syncthreads();
  for (int t = 0; t < nsteps; ++t) {
    const bool more = t + 1 < nsteps;
    if (more) {
      load(t + 1, dy, dx, c0);
      advance();
    }
    const unsigned char* base = lds + (t & 1) * STAGE + frag_off;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      bf16x8 wf[NT], xf[4];
#pragma unroll
      for (int i = 0; i < NT; ++i)
        wf[i] = *reinterpret_cast<const bf16x8*>(base + CV_A_BYTES + (b_sub0 + i * 2 + kb) * 1024);
#pragma unroll
      for (int j = 0; j < 4; ++j) xf[j] = *reinterpret_cast<const bf16x8*>(base + (a_sub0 + j * 2 + kb) * 1024);
#pragma unroll
      for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[i], xf[j], acc[i][j], 0, 0, 0);
    }
    if (more) store((t + 1) & 1);
    __syncthreads();
  }

  // ---- epilogue: + bias, ReLU, bf16; through an LDS image [128][BN] so that the rows leave as 16 bytes per lane
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int nl = wn * (BN / 2) + i * 16 + 4 * (lane >> 4);
    const u16x4 b4 = *reinterpret_cast<const u16x4*>(bias + n0 + nl);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int ml = wm * 64 + j * 16 + (lane & 15);
      u16x4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = acc[i][j][r] + bf16_bits_to_f32(b4[r]);
        if (relu_out) v = fmaxf(v, 0.f);
        o[r] = f32_to_bf16_bits(v);
      }
      *reinterpret_cast<u16x4*>(lds + ml * ROWB + nl * 2) = o;
    }
  }
  __syncthreads();
  constexpr int CH = BN / 8;
#pragma unroll
  for (int it = 0; it < CV_BM * CH / 256; ++it) {
    const int item = it * 256 + tid;
    const int row = item / CH, ch = item - row * CH;
    if (m0 + row < M)
      *reinterpret_cast<uint4*>(y + (m0 + row) * ld_out + n0 + ch * 8) =
          *reinterpret_cast<const uint4*>(lds + row * ROWB + ch * 16);
  }
  if (nb == 0 && ld_out > C) {                     // the zero columns behind C (at most C of them)
    const int npad = (ld_out - C) >> 3;
    for (int item = tid; item < CV_BM * npad; item += 256) {
      const int row = item / npad, ch = item - row * npad;
      if (m0 + row < M) *reinterpret_cast<uint4*>(y + (m0 + row) * ld_out + C + ch * 8) = make_uint4(0, 0, 0, 0);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Stem: 7 x 7, stride 2, padding 3, 3 -> 64 channels, + bias, ReLU.  Workgroup = 256 threads, 128 output pixels x all 64
// channels, K = 147 padded to 160 = 5 k-blocks.  Thread t gathers pixel t & 127 of the tile: 10 chunks of 8 k each,
// and for a fixed chunk the 64 lanes of a wave read 64 neighbouring pixels (stride 2 elements in an NCHW row).
constexpr int ST_K = 147, ST_KP = 160, ST_KB = ST_KP / 32;

__global__ __launch_bounds__(256) void conv7x7s2_kernel(const unsigned short* __restrict__ x,
                                                        const unsigned short* __restrict__ w,
                                                        const unsigned short* __restrict__ bias,
                                                        unsigned short* __restrict__ y, int H, int W, int H1, int W1,
                                                        int64_t sb, int64_t sc, int64_t sh, int64_t sw, int K_pad,
                                                        int ld_out, int64_t M) {
  __shared__ __align__(16) unsigned char lds_a[128 * ST_KP * 2];
  __shared__ __align__(16) unsigned char lds_w[64 * ST_KP * 2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t m0 = (int64_t)blockIdx.x * 128;

  for (int j = tid; j < 64 * (ST_KP / 8); j += 256) {
    const int row = j / (ST_KP / 8), c = j - row * (ST_KP / 8);
    *reinterpret_cast<uint4*>(lds_w + rn_img(row, c, ST_KB)) =
        *reinterpret_cast<const uint4*>(w + (size_t)row * K_pad + c * 8);
  }

  const int row = tid & 127;
  const int64_t m = m0 + row;
  const bool live = m < M;
  int ih0 = 0, iw0 = 0;
  const unsigned short* xb = x;
  if (live) {
    const int ow = (int)(m % W1);
    const int64_t q = m / W1;
    const int oh = (int)(q % H1);
    ih0 = oh * 2 - 3;
    iw0 = ow * 2 - 3;
    xb = x + (q / H1) * sb;
  }
#pragma unroll 2
  for (int it = 0; it < ST_KP / 16; ++it) {
    const int cq = (tid >> 7) + 2 * it;
    unsigned short e[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int k = cq * 8 + u;
      const int pix = k / 3, c = k - 3 * pix;
      const int dy = pix / 7, dx = pix - 7 * dy;
      const int ih = ih0 + dy, iw = iw0 + dx;
      e[u] = 0;
      if (live && k < ST_K && (unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W)
        e[u] = xb[c * sc + ih * sh + iw * sw];
    }
    *reinterpret_cast<uint4*>(lds_a + rn_img(row, cq, ST_KB)) =
        make_uint4(e[0] | ((unsigned)e[1] << 16), e[2] | ((unsigned)e[3] << 16), e[4] | ((unsigned)e[5] << 16),
                   e[6] | ((unsigned)e[7] << 16));
  }
  __syncthreads();

  // wave: 32 pixels x 64 channels
  f32x4 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int frag_off = rn_swz((lane & 15) * 64 + (lane >> 4) * 16);
#pragma unroll
  for (int kb = 0; kb < ST_KB; ++kb) {
    bf16x8 wf[4], xf[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) wf[i] = *reinterpret_cast<const bf16x8*>(lds_w + (i * ST_KB + kb) * 1024 + frag_off);
#pragma unroll
    for (int j = 0; j < 2; ++j)
      xf[j] = *reinterpret_cast<const bf16x8*>(lds_a + ((wave * 2 + j) * ST_KB + kb) * 1024 + frag_off);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[i], xf[j], acc[i][j], 0, 0, 0);
  }
  __syncthreads();                                  // the patch image is dead: it becomes the [128][64] output image
  constexpr int ROWB = 64 * 2 + 16;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int nl = i * 16 + 4 * (lane >> 4);
    const u16x4 b4 = *reinterpret_cast<const u16x4*>(bias + nl);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int ml = wave * 32 + j * 16 + (lane & 15);
      u16x4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = f32_to_bf16_bits(fmaxf(acc[i][j][r] + bf16_bits_to_f32(b4[r]), 0.f));
      *reinterpret_cast<u16x4*>(lds_a + ml * ROWB + nl * 2) = o;
    }
  }
  __syncthreads();
  const int lv = ld_out >> 3;                        // 8 .. 16 vectors per row, the ones behind 64 channels zero
  for (int item = tid; item < 128 * lv; item += 256) {
    const int r = item / lv, ch = item - r * lv;
    if (m0 + r < M) {
      uint4 v = make_uint4(0, 0, 0, 0);
      if (ch < 8) v = *reinterpret_cast<const uint4*>(lds_a + r * ROWB + ch * 16);
      *reinterpret_cast<uint4*>(y + (m0 + r) * ld_out + ch * 8) = v;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// 3 x 3 max pool, stride 2, padding 1: one 16-byte output vector per thread.  The centre tap (2 oh, 2 ow) is always
// inside the image, so the padding never wins.
__global__ __launch_bounds__(256) void maxpool3x3s2_kernel(const unsigned short* __restrict__ x, int H, int W, int Ho,
                                                           int Wo, int C, int ld_in, int ld_out,
                                                           unsigned short* __restrict__ y, int64_t nvec) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= nvec) return;
  const int lv = ld_out >> 3;
  const int64_t pixel = v / lv;
  const int c = (int)(v - pixel * lv) * 8;
  uint4 o = make_uint4(0, 0, 0, 0);
  if (c < C) {
    const int ow = (int)(pixel % Wo);
    const int64_t q = pixel / Wo;
    const int oh = (int)(q % Ho);
    const unsigned short* img = x + (q / Ho) * H * (int64_t)W * ld_in + c;
    float best[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) best[i] = -INFINITY;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
      const int ih = 2 * oh - 1 + dy;
      if ((unsigned)ih >= (unsigned)H) continue;
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const int iw = 2 * ow - 1 + dx;
        if ((unsigned)iw >= (unsigned)W) continue;
        float f[8];
        unpack8(*reinterpret_cast<const uint4*>(img + ((int64_t)ih * W + iw) * ld_in), f);
#pragma unroll
        for (int i = 0; i < 8; ++i) best[i] = fmaxf(best[i], f[i]);
      }
    }
    o = pack8(best);
  }
  *reinterpret_cast<uint4*>(y + v * 8) = o;
}

// y <- bf16(max(0, y + r)) on rows x C, 16 bytes per lane
__global__ __launch_bounds__(256) void add_relu_kernel(unsigned short* __restrict__ y,
                                                       const unsigned short* __restrict__ r, int C, int ld_y, int ld_r,
                                                       int64_t nvec) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= nvec) return;
  const int cv = C >> 3;
  const int64_t row = v / cv;
  const int c = (int)(v - row * cv) * 8;
  uint4* py = reinterpret_cast<uint4*>(y + row * ld_y + c);
  float a[8], b[8];
  unpack8(*py, a);
  unpack8(*reinterpret_cast<const uint4*>(r + row * ld_r + c), b);
#pragma unroll
  for (int i = 0; i < 8; ++i) a[i] = fmaxf(a[i] + b[i], 0.f);
  *py = pack8(a);
}

}  // namespace basd

extern "C" int basd_conv3x3_bf16(const void* x, const void* w9, const void* bias, int B, int H, int W, int C, int stride,
                                 int ld_in, int ld_out, int relu_in, int relu_out, void* y, void* stream) {
  using namespace basd;
  if (B <= 0) return BASD_OK;
  if (H < 1 || W < 1) return fail(BASD_ERR_SHAPE, "conv3x3_bf16: H, W >= 1 required (got %d x %d)", H, W);
  if (stride != 1 && stride != 2) return fail(BASD_ERR_SHAPE, "conv3x3_bf16: stride 1 or 2 (got %d)", stride);
  if (C % 64 || C < 64 || C > 512) return fail(BASD_ERR_SHAPE, "conv3x3_bf16: C %% 64 == 0, 64 <= C <= 512 (got %d)", C);
  if (ld_in < C || ld_in % 8 || ld_out < C || ld_out % 8 || ld_out > 2 * C)
    return fail(BASD_ERR_SHAPE, "conv3x3_bf16: row strides must be multiples of 8 with C <= ld_in, C <= ld_out <= 2 C "
                "(got C=%d ld_in=%d ld_out=%d)", C, ld_in, ld_out);
  if (((uintptr_t)x | (uintptr_t)w9 | (uintptr_t)bias | (uintptr_t)y) & 15)
    return fail(BASD_ERR_SHAPE, "conv3x3_bf16: 16-byte aligned buffers required");
  if (x == y) return fail(BASD_ERR_SHAPE, "conv3x3_bf16: y must not alias x");
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  const int64_t M = (int64_t)B * Ho * Wo;
  const int64_t mblocks = (M + CV_BM - 1) / CV_BM;
  const bool wide = C % 128 == 0;                   // 64, 192, 320, 448: tiles of 64 channels
  const int tiles_n = wide ? C / 128 : C / 64;
  const int64_t grid = (mblocks + 7) / 8 * 8 * tiles_n;
  if (M > 0x7fffff00LL || grid > 0x7fffffffLL)
    return fail(BASD_ERR_SHAPE, "conv3x3_bf16: %lld output pixels, %lld workgroups", (long long)M, (long long)grid);
  hipStream_t st = (hipStream_t)stream;
  if (!wide)
    hipLaunchKernelGGL(conv3x3_kernel<64>, dim3((unsigned)grid), dim3(256), 0, st, (const unsigned short*)x,
                       (const unsigned short*)w9, (const unsigned short*)bias, (unsigned short*)y, H, W, Ho, Wo, C,
                       stride, ld_in, ld_out, relu_in, relu_out, M, (int)mblocks, tiles_n);
  else
    hipLaunchKernelGGL(conv3x3_kernel<128>, dim3((unsigned)grid), dim3(256), 0, st, (const unsigned short*)x,
                       (const unsigned short*)w9, (const unsigned short*)bias, (unsigned short*)y, H, W, Ho, Wo, C,
                       stride, ld_in, ld_out, relu_in, relu_out, M, (int)mblocks, tiles_n);
  return check_launch("conv3x3_bf16");
}

extern "C" int basd_conv7x7s2_relu_bf16(const void* x, const void* w, const void* bias, int B, int H, int W, int64_t sb,
                                        int64_t sc, int64_t sh, int64_t sw, int K_pad, int ld_out, void* y,
                                        void* stream) {
  using namespace basd;
  if (B <= 0) return BASD_OK;
  if (H < 1 || W < 1) return fail(BASD_ERR_SHAPE, "conv7x7s2_relu_bf16: H, W >= 1 required (got %d x %d)", H, W);
  if (K_pad < ST_KP || K_pad % 8)
    return fail(BASD_ERR_SHAPE, "conv7x7s2_relu_bf16: K_pad %% 8 == 0 and K_pad >= %d (got %d)", ST_KP, K_pad);
  if (ld_out < 64 || ld_out > 128 || ld_out % 8)
    return fail(BASD_ERR_SHAPE, "conv7x7s2_relu_bf16: ld_out %% 8 == 0, 64 <= ld_out <= 128 (got %d)", ld_out);
  if (((uintptr_t)w | (uintptr_t)bias | (uintptr_t)y) & 15)
    return fail(BASD_ERR_SHAPE, "conv7x7s2_relu_bf16: 16-byte aligned weight, bias and output required");
  const int H1 = (H - 1) / 2 + 1, W1 = (W - 1) / 2 + 1;
  const int64_t M = (int64_t)B * H1 * W1;
  const int64_t grid = (M + 127) / 128;
  if (grid > 0x7fffffffLL) return fail(BASD_ERR_SHAPE, "conv7x7s2_relu_bf16: %lld workgroups", (long long)grid);
  hipLaunchKernelGGL(conv7x7s2_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream,
                     (const unsigned short*)x, (const unsigned short*)w, (const unsigned short*)bias,
                     (unsigned short*)y, H, W, H1, W1, sb, sc, sh, sw, K_pad, ld_out, M);
  return check_launch("conv7x7s2_relu_bf16");
}

extern "C" int basd_maxpool3x3s2_bf16(const void* x, int B, int H, int W, int C, int ld_in, int ld_out, void* y,
                                      void* stream) {
  using namespace basd;
  if (B <= 0) return BASD_OK;
  if (H < 1 || W < 1) return fail(BASD_ERR_SHAPE, "maxpool3x3s2_bf16: H, W >= 1 required (got %d x %d)", H, W);
  if (C % 8 || C < 8 || ld_in < C || ld_in % 8 || ld_out < C || ld_out % 8)
    return fail(BASD_ERR_SHAPE, "maxpool3x3s2_bf16: C and the row strides must be multiples of 8 with C <= ld "
                "(got C=%d ld_in=%d ld_out=%d)", C, ld_in, ld_out);
  if (((uintptr_t)x | (uintptr_t)y) & 15) return fail(BASD_ERR_SHAPE, "maxpool3x3s2_bf16: 16-byte aligned buffers required");
  if (x == y) return fail(BASD_ERR_SHAPE, "maxpool3x3s2_bf16: y must not alias x");
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  const int64_t nvec = (int64_t)B * Ho * Wo * (ld_out / 8);
  const int64_t grid = (nvec + 255) / 256;
  if (grid > 0x7fffffffLL) return fail(BASD_ERR_SHAPE, "maxpool3x3s2_bf16: %lld workgroups", (long long)grid);
  hipLaunchKernelGGL(maxpool3x3s2_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream,
                     (const unsigned short*)x, H, W, Ho, Wo, C, ld_in, ld_out, (unsigned short*)y, nvec);
  return check_launch("maxpool3x3s2_bf16");
}

extern "C" int basd_add_relu_bf16(void* y, const void* r, int64_t rows, int C, int ld_y, int ld_r, void* stream) {
  using namespace basd;
  if (rows <= 0) return BASD_OK;
  if (C % 8 || C < 8 || ld_y < C || ld_y % 8 || ld_r < C || ld_r % 8)
    return fail(BASD_ERR_SHAPE, "add_relu_bf16: C and the row strides must be multiples of 8 with C <= ld "
                "(got C=%d ld_y=%d ld_r=%d)", C, ld_y, ld_r);
  if (((uintptr_t)y | (uintptr_t)r) & 15) return fail(BASD_ERR_SHAPE, "add_relu_bf16: 16-byte aligned buffers required");
  const int64_t nvec = rows * (C / 8);
  const int64_t grid = (nvec + 255) / 256;
  if (grid > 0x7fffffffLL) return fail(BASD_ERR_SHAPE, "add_relu_bf16: %lld workgroups", (long long)grid);
  hipLaunchKernelGGL(add_relu_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, (unsigned short*)y,
                     (const unsigned short*)r, C, ld_y, ld_r, nvec);
  return check_launch("add_relu_bf16");
}
