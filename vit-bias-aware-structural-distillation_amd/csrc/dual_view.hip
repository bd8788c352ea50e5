// Both training views from one uint8 batch (data/device_views.py; reference src/data/datasets.py:80-94, 137-149 runs
// torchvision v2 in the loader workers):
//   basd_resample_u8      window -> antialiased bilinear resize -> offset crop -> horizontal flip, uint8 out
//   basd_resample_u8_packed  the same per sample, for samples of different sizes packed into one byte buffer
//   basd_ta_normalize_u8  one TrivialAugmentWide operation (data/transforms.py, apply_ta_op) + ToDtype + Normalize, fp32 out
// The arithmetic follows the CPU functions operation by operation: where they round a product before adding (the affine
// coordinates, the blends) so do these kernels, hence no contraction in this file; the two resize passes accumulate with
// explicit fused multiply-adds.
#include "basd_common.h"

#pragma clang fp contract(off)

namespace basd {
namespace {

constexpr int REC = 9;             // top, left, h, w, nh, nw, off_y, off_x, flip
constexpr int TA_THREADS = 1024;
constexpr int XW = 8;              // horizontal weights kept in registers (scale <= 3); wider filters recompute them

// One axis of F.interpolate(mode="bilinear", antialias=True, align_corners=False): the triangle filter of output index i.
struct Taps {
  float center, invscale;
  int lo, cnt;
};

__device__ __forceinline__ Taps aa_taps(int i, int n_in, int n_out) {
  Taps t;
  const float scale = (float)n_in / (float)n_out;
  const float support = scale >= 1.0f ? scale : 1.0f;
  t.invscale = scale >= 1.0f ? 1.0f / scale : 1.0f;
  t.center = scale * ((float)i + 0.5f);
  const float d = t.center - support, u = t.center + support;
  t.lo = max((int)((double)d + 0.5), 0);
  t.cnt = min((int)((double)u + 0.5), n_in) - t.lo;
  return t;
}

__device__ __forceinline__ float aa_weight(const Taps& t, int j) {       // tap j of the window, unnormalised
  const float a = (float)(j + t.lo) - t.center;
  const float x = fabsf((float)(((double)a + 0.5) * (double)t.invscale));
  return x < 1.0f ? 1.0f - x : 0.0f;
}

__device__ __forceinline__ float aa_total(const Taps& t) {
  float s = 0.0f;
  for (int j = 0; j < t.cnt; ++j) s += aa_weight(t, j);
  return s;
}

// One output byte.  Every index is clamped into the canvas, whatever the record holds.
__device__ __forceinline__ unsigned resample_px(const unsigned char* __restrict__ src, const int* __restrict__ rec, int H,
                                                int W, int S, int64_t e) {
  const int P = S * S;
  const int64_t b = e / (3 * (int64_t)P);
  int r = (int)(e - b * 3 * (int64_t)P);
  const int c = r / P;
  r -= c * P;
  const int y = r / S, x = r - y * S;
  const int* R = rec + b * REC;
  const int top = min(max(R[0], 0), H - 1), left = min(max(R[1], 0), W - 1);
  const int h = min(max(R[2], 1), H - top), w = min(max(R[3], 1), W - left);
  const int nh = max(R[4], 1), nw = max(R[5], 1);
  const int vy = min(max(R[6] + y, 0), nh - 1);
  const int vx = min(max(R[7] + (R[8] ? S - 1 - x : x), 0), nw - 1);
  const Taps ty = aa_taps(vy, h, nh), tx = aa_taps(vx, w, nw);
  if (ty.cnt < 1 || tx.cnt < 1) return 0u;
  const float tot_y = aa_total(ty), tot_x = aa_total(tx);
  float wx[XW];
#pragma unroll
  for (int j = 0; j < XW; ++j) wx[j] = j < tx.cnt ? aa_weight(tx, j) / tot_x : 0.0f;
  const unsigned char* plane = src + ((b * 3 + c) * (int64_t)H + top + ty.lo) * W + left + tx.lo;
  float acc = 0.0f;
  for (int i = 0; i < ty.cnt; ++i) {
    const unsigned char* row = plane + (int64_t)i * W;
    float hs = (float)row[0] * wx[0];                       // horizontal pass first; its result is an fp32 value
#pragma unroll
    for (int j = 1; j < XW; ++j)
      if (j < tx.cnt) hs = fmaf((float)row[j], wx[j], hs);
    for (int j = XW; j < tx.cnt; ++j) hs = fmaf((float)row[j], aa_weight(tx, j) / tot_x, hs);
    const float wy = aa_weight(ty, i) / tot_y;
    acc = i == 0 ? hs * wy : fmaf(hs, wy, acc);
  }
  return (unsigned)fminf(fmaxf(rintf(acc), 0.0f), 255.0f);
}

// one packed 32-bit word of the output per thread (the output is a dense byte array: a word may straddle rows)
__global__ void __launch_bounds__(256) resample_u8_kernel(const unsigned char* __restrict__ src,
                                                          const int* __restrict__ rec, int H, int W, int S,
                                                          unsigned char* __restrict__ out, int64_t total) {
  const int64_t base = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (base >= total) return;
  if (base + 4 <= total) {
    unsigned word = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) word |= resample_px(src, rec, H, W, S, base + q) << (8 * q);
    *reinterpret_cast<unsigned*>(out + base) = word;
  } else {
    for (int64_t e = base; e < total; ++e) out[e] = (unsigned char)resample_px(src, rec, H, W, S, e);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Samples of different sizes packed into one byte buffer.  One workgroup per (sample, band of PK_ROWS output rows), all
// three channels.  The taps of the S output columns and of the band's rows are worked out once per workgroup into LDS
// (window start, tap count, weight sum, the first XW weights already divided by the sum: the same bits resample_px
// recomputes per byte); the pixels then only read the tables.  A lane owns one output BYTE, so that the lanes of a
// wave walk a row: the column table is read without bank conflicts and the source bytes of neighbouring lanes are
// neighbours.  Four lanes put their bytes together for one 32-bit store.
constexpr int PK_THREADS = 256;
constexpr int PK_ROWS = 16;

__host__ __device__ constexpr int pk_lds_bytes(int S) { return (S + PK_ROWS) * (2 * 16 + 3 * 4); }

struct AxisTable {          // n entries, in this order in LDS (the float4 arrays first: 16-byte aligned)
  float4* w03;              // normalised weights 0 .. 3 (0 beyond cnt)
  float4* w47;              // 4 .. 7
  float* tot;
  int* lo;
  int* cnt;
};

__device__ __forceinline__ void axis_entry(const AxisTable& T, int k, int v, int n_in, int n_out) {
  const Taps t = aa_taps(v, n_in, n_out);
  const float tot = aa_total(t);
  float w[XW];
#pragma unroll
  for (int j = 0; j < XW; ++j) w[j] = j < t.cnt ? aa_weight(t, j) / tot : 0.0f;
  T.w03[k] = make_float4(w[0], w[1], w[2], w[3]);
  T.w47[k] = make_float4(w[4], w[5], w[6], w[7]);
  T.tot[k] = tot;
  T.lo[k] = t.lo;
  T.cnt[k] = t.cnt;
}

__global__ void __launch_bounds__(PK_THREADS) resample_u8_packed_kernel(const unsigned char* __restrict__ pixels,
                                                                        int64_t pixels_bytes,
                                                                        const int64_t* __restrict__ geom,
                                                                        const int* __restrict__ rec, int S, int bands,
                                                                        unsigned char* __restrict__ out) {
  extern __shared__ float4 pk_lds[];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / bands, band = blockIdx.x - b * bands;
  const int y0 = band * PK_ROWS, rows = min(PK_ROWS, S - y0);

  AxisTable col, row;
  col.w03 = pk_lds;
  col.w47 = col.w03 + S;
  row.w03 = col.w47 + S;
  row.w47 = row.w03 + PK_ROWS;
  col.tot = reinterpret_cast<float*>(row.w47 + PK_ROWS);
  row.tot = col.tot + S;
  col.lo = reinterpret_cast<int*>(row.tot + PK_ROWS);
  row.lo = col.lo + S;
  col.cnt = row.lo + PK_ROWS;
  row.cnt = col.cnt + S;

  // a sample that does not lie inside the buffer is never read: its output is zero
  const int64_t off = geom[b * 3], H64 = geom[b * 3 + 1], W64 = geom[b * 3 + 2];
  bool valid = off >= 0 && H64 >= 1 && H64 <= 16384 && W64 >= 1 && W64 <= 16384;
  if (valid) {
    const int64_t need = 3 * H64 * W64;                         // at most 3 * 2^28
    valid = need <= pixels_bytes && off <= pixels_bytes - need;
  }
  const int H = valid ? (int)H64 : 1, W = valid ? (int)W64 : 1;

  const int* R = rec + (int64_t)b * REC;                        // clamped as in resample_px
  const int top = min(max(R[0], 0), H - 1), left = min(max(R[1], 0), W - 1);
  const int h = min(max(R[2], 1), H - top), w = min(max(R[3], 1), W - left);
  const int nh = max(R[4], 1), nw = max(R[5], 1);
  const int off_y = R[6], off_x = R[7];
  const bool flip = R[8] != 0;

  if (valid) {
    for (int k = tid; k < S + rows; k += PK_THREADS) {
      if (k < S) axis_entry(col, k, min(max(off_x + k, 0), nw - 1), w, nw);
      else axis_entry(row, k - S, min(max(off_y + y0 + (k - S), 0), nh - 1), h, nh);
    }
  }
  __syncthreads();

  const unsigned char* src = pixels + (valid ? off : 0);
  const int len = rows * S;                                     // bytes of one channel of the band: contiguous in out
  for (int c = 0; c < 3; ++c) {
    const int64_t g0 = (((int64_t)b * 3 + c) * S + y0) * S;     // first byte; not 4-byte aligned when S is odd
    const int lead = (int)(g0 & 3);                             // lanes walk from the aligned address below g0
    const unsigned char* plane0 = src + ((int64_t)c * H + top) * W + left;
    for (int p0 = 0; p0 < lead + len; p0 += PK_THREADS) {
      const int p = p0 + tid - lead;                            // byte of the band, (p + lead) % 4 == tid % 4
      const bool mine = p >= 0 && p < len;
      unsigned v = 0;
      if (mine && valid) {
        const int y = p / S, x = p - y * S;
        const int k = flip ? S - 1 - x : x;
        const int cx = col.cnt[k], cy = row.cnt[y];
        if (cx >= 1 && cy >= 1) {
          const float4 a = col.w03[k], bq = col.w47[k];
          const float wx[XW] = {a.x, a.y, a.z, a.w, bq.x, bq.y, bq.z, bq.w};
          const float4 ya = row.w03[y], yb = row.w47[y];
          const float wy8[XW] = {ya.x, ya.y, ya.z, ya.w, yb.x, yb.y, yb.z, yb.w};
          Taps tx = {}, ty = {};                                    // only filters of more than XW taps need them
          float tot_x = 0.0f, tot_y = 0.0f;
          if (cx > XW) {
            tx = aa_taps(min(max(off_x + k, 0), nw - 1), w, nw);
            tot_x = col.tot[k];
          }
          if (cy > XW) {
            ty = aa_taps(min(max(off_y + y0 + y, 0), nh - 1), h, nh);
            tot_y = row.tot[y];
          }
          const unsigned char* plane = plane0 + (int64_t)row.lo[y] * W + col.lo[k];
          float acc = 0.0f;
          for (int i = 0; i < cy; ++i) {
            const unsigned char* line = plane + (int64_t)i * W;
            float hs = (float)line[0] * wx[0];
#pragma unroll
            for (int j = 1; j < XW; ++j)
              if (j < cx) hs = fmaf((float)line[j], wx[j], hs);
            for (int j = XW; j < cx; ++j) hs = fmaf((float)line[j], aa_weight(tx, j) / tot_x, hs);
            float wy = 0.0f;
#pragma unroll
            for (int j = 0; j < XW; ++j)
              if (i == j) wy = wy8[j];
            if (i >= XW) wy = aa_weight(ty, i) / tot_y;
            acc = i == 0 ? hs * wy : fmaf(hs, wy, acc);
          }
          v = (unsigned)fminf(fmaxf(rintf(acc), 0.0f), 255.0f);
        }
      }
      // lanes 4 m .. 4 m + 3 hold the bytes of one aligned word of out
      unsigned word = v;
      word |= (unsigned)__shfl_down((int)v, 1, 64) << 8;
      word |= (unsigned)__shfl_down((int)v, 2, 64) << 16;
      word |= (unsigned)__shfl_down((int)v, 3, 64) << 24;
      const int q = tid & 3;
      const bool whole = p - q >= 0 && p - q + 4 <= len;        // the same answer in the four lanes
      if (whole) {
        if (q == 0) *reinterpret_cast<unsigned*>(out + g0 + p) = word;
      } else if (mine) {
        out[g0 + p] = (unsigned char)v;                         // the band's byte head and tail
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
enum TaOp { ID = 0, SHEAR_X, SHEAR_Y, TRANS_X, TRANS_Y, ROTATE, BRIGHT, COLOR, CONTRAST, SHARP, POSTER, SOLAR, AUTOC, EQUAL };

struct Norm {
  float mean[3], std[3];
};

struct TaParams {
  int op;
  float a, b, c, d, e, f;     // inverse affine map about the centre
  float f1, f2;               // blend factors: factor, 1 - factor
  float gray_mean, thr;
  int mask;
};

__device__ __forceinline__ unsigned blend_u8(float f1, float x, float f2, float other) {
  const float m1 = f1 * x, m2 = f2 * other;                  // both products rounded, then added (transforms._blend)
  const float t = m1 + m2;
  return (unsigned)rintf(fminf(fmaxf(t, 0.0f), 255.0f));
}

__device__ __forceinline__ float gray_of(const unsigned char* img, int P, int r) {
  const float g0 = 0.299f * (float)img[r], g1 = 0.587f * (float)img[P + r], g2 = 0.114f * (float)img[2 * P + r];
  return (g0 + g1) + g2;
}

struct TaShared {
  float lut[3][256];           // the normalisation of every byte value
  int hist[3][256];
  unsigned char eq[3][256];
  int mn[3], mx[3];
  float lo[3], scale[3];
  double red[TA_THREADS / 64];
};

// pixel (c, y, x) of the operation's uint8 result; r = y S + x
__device__ __forceinline__ unsigned ta_px(const TaParams& p, const TaShared& sh, const unsigned char* __restrict__ img,
                                          int S, int c, int y, int x, int r) {
  const int P = S * S;
  const unsigned v = img[c * P + r];
  switch (p.op) {
    case SHEAR_X: case SHEAR_Y: case TRANS_X: case TRANS_Y: case ROTATE: {
      const float ctr = (float)(S - 1) * 0.5f;
      const float xs = (float)x - ctr, ys = (float)y - ctr;
      const float ax = p.a * xs, bx = p.b * ys, dy = p.d * xs, ey = p.e * ys;
      const float xi = rintf(((ax + bx) + p.c) + ctr);         // the operation order of transforms._affine_nearest
      const float yi = rintf(((dy + ey) + p.f) + ctr);
      if (!(xi >= 0.0f && xi < (float)S && yi >= 0.0f && yi < (float)S)) return 0u;
      return img[c * P + (int)yi * S + (int)xi];
    }
    case BRIGHT: return blend_u8(p.f1, (float)v, p.f2, 0.0f);
    case COLOR: return blend_u8(p.f1, (float)v, p.f2, gray_of(img, P, r));
    case CONTRAST: return blend_u8(p.f1, (float)v, p.f2, p.gray_mean);
    case SHARP: {
      float soft = (float)v;
      if (x >= 1 && x < S - 1 && y >= 1 && y < S - 1) {
        const unsigned char* q = img + c * P + r - S - 1;
        const int n = q[0] + q[1] + q[2] + q[S] + 5 * q[S + 1] + q[S + 2] + q[2 * S] + q[2 * S + 1] + q[2 * S + 2];
        soft = rintf((float)n / 13.0f);     // n / 13 is never within 1 / 26 of a tie: the integer the fp32 convolution rounds to
      }
      return blend_u8(p.f1, (float)v, p.f2, soft);
    }
    case POSTER: return v & (unsigned)p.mask;
    case SOLAR: return (float)v >= p.thr ? 255u - v : v;
    case AUTOC: {
      const float d = (float)v - sh.lo[c];
      return (unsigned)fminf(fmaxf(d * sh.scale[c], 0.0f), 255.0f);       // truncates, as the CPU's .to(uint8)
    }
    case EQUAL: return sh.eq[c][v];
    default: return v;
  }
}

// One workgroup per image: the reductions the operation needs (LDS), then a block-strided apply with 16-byte stores.
__global__ void __launch_bounds__(TA_THREADS) ta_normalize_u8_kernel(const unsigned char* __restrict__ in,
                                                                     const int* __restrict__ ops,
                                                                     const double* __restrict__ mags, Norm nm, int S,
                                                                     float* __restrict__ out) {
  __shared__ TaShared sh;
  const int tid = threadIdx.x, P = S * S, n = 3 * P;
  const int64_t g0 = (int64_t)blockIdx.x * n;
  const unsigned char* img = in + g0;
  TaParams p;
  p.op = ops ? ops[blockIdx.x] : ID;
  if (p.op < 0 || p.op > EQUAL) p.op = ID;
  const double mag = ops ? mags[blockIdx.x] : 0.0;
  p.a = 1.0f; p.b = 0.0f; p.c = 0.0f; p.d = 0.0f; p.e = 1.0f; p.f = 0.0f;
  p.f1 = (float)(1.0 + mag);
  p.f2 = (float)(1.0 - (1.0 + mag));
  p.gray_mean = 0.0f;
  p.thr = (float)mag;
  p.mask = 255;
  if (p.op == SHEAR_X) p.b = (float)mag;
  if (p.op == SHEAR_Y) p.d = (float)mag;
  if (p.op == TRANS_X) p.c = (float)(-trunc(mag));
  if (p.op == TRANS_Y) p.f = (float)(-trunc(mag));
  if (p.op == ROTATE) {
    const double t = mag * (3.14159265358979323846 / 180.0);
    p.a = p.e = (float)cos(t);
    p.b = (float)(-sin(t));
    p.d = (float)sin(t);
  }
  if (p.op == POSTER) {
    const int bits = min(max((int)mag, 0), 8);
    p.mask = 255 - ((1 << (8 - bits)) - 1);
  }

  for (int i = tid; i < 768; i += TA_THREADS) {
    const int c = i >> 8;
    sh.lut[c][i & 255] = ((float)(i & 255) / 255.0f - nm.mean[c]) / nm.std[c];
    sh.hist[c][i & 255] = 0;
  }
  if (tid < 3) {
    sh.mn[tid] = 255;
    sh.mx[tid] = 0;
  }
  __syncthreads();

  if (p.op == CONTRAST) {                       // mean of the unrounded fp32 gray image, summed in fp64
    double s = 0.0;
    for (int r = tid; r < P; r += TA_THREADS) s += (double)gray_of(img, P, r);
    s = wave_sum_d(s);
    if ((tid & 63) == 0) sh.red[tid >> 6] = s;
    __syncthreads();
    double t = 0.0;
    for (int i = 0; i < TA_THREADS / 64; ++i) t += sh.red[i];
    p.gray_mean = (float)(t / (double)P);
  } else if (p.op == AUTOC) {
    for (int c = 0; c < 3; ++c) {
      int lo_ = 255, hi_ = 0;
      for (int r = tid; r < P; r += TA_THREADS) {
        const int v = img[c * P + r];
        lo_ = min(lo_, v);
        hi_ = max(hi_, v);
      }
      atomicMin(&sh.mn[c], lo_);
      atomicMax(&sh.mx[c], hi_);
    }
    __syncthreads();
    if (tid < 3) {                              // transforms.autocontrast: a constant channel stays as it is
      const bool same = sh.mx[tid] == sh.mn[tid];
      sh.lo[tid] = same ? 0.0f : (float)sh.mn[tid];
      sh.scale[tid] = same ? 1.0f : 255.0f / ((float)sh.mx[tid] - (float)sh.mn[tid]);
    }
    __syncthreads();
  } else if (p.op == EQUAL) {
    for (int c = 0; c < 3; ++c)
      for (int r = tid; r < P; r += TA_THREADS) atomicAdd(&sh.hist[c][img[c * P + r]], 1);
    __syncthreads();
    if (tid < 3) {                              // transforms.equalize in integers
      const int* h = sh.hist[tid];
      int last = 255;
      while (last > 0 && h[last] == 0) --last;
      const int step = (P - h[last]) / 255;     // the sum of the non-empty bins but the last one, floor-divided
      int cum = 0;
      for (int v = 0; v < 256; ++v) {
        sh.eq[tid][v] = step == 0 ? (unsigned char)v : (unsigned char)min((cum + step / 2) / step, 255);
        cum += h[v];
      }
    }
    __syncthreads();
  }

  // out + g0 is 16-byte aligned only every fourth image when n % 4 != 0: scalar head, float4 body, scalar tail
  const int head = min((int)((4 - (g0 & 3)) & 3), n);
  const int quads = (n - head) / 4;
  float* o = out + g0;
  for (int k = tid; k < quads; k += TA_THREADS) {
    const int e = head + 4 * k;
    int c = e / P, r = e - c * P;
    int y = r / S, x = r - y * S;
    float v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      v[q] = sh.lut[c][ta_px(p, sh, img, S, c, y, x, r)];
      ++r;
      if (++x == S) {
        x = 0;
        if (++y == S) { y = 0; r = 0; ++c; }
      }
    }
    *reinterpret_cast<float4*>(o + e) = make_float4(v[0], v[1], v[2], v[3]);
  }
  const int tail0 = head + 4 * quads;
  const int e = tid < head ? tid : tail0 + (tid - head);      // the at most six elements outside the float4 body
  if (tid < head + (n - tail0)) {
    const int c = e / P, r = e - c * P;
    o[e] = sh.lut[c][ta_px(p, sh, img, S, c, r / S, r % S, r)];
  }
}

}  // namespace
}  // namespace basd

static bool dual_view_size_ok(int S) { return S >= 3 && S <= 1024; }

extern "C" int basd_resample_u8(const void* src, const int* rec, int B, int H, int W, int S, void* out, void* stream) {
  using namespace basd;
  if (B <= 0) return BASD_OK;
  if (!dual_view_size_ok(S) || H < 1 || W < 1 || H > 16384 || W > 16384)
    return fail(BASD_ERR_SHAPE, "resample_u8: S = %d (3 .. 1024), source %d x %d (1 .. 16384)", S, H, W);
  if (((uintptr_t)out & 3) != 0 || ((uintptr_t)rec & 3) != 0)
    return fail(BASD_ERR_SHAPE, "resample_u8: out and rec must be 4-byte aligned");
  const int64_t total = (int64_t)B * 3 * S * S;
  const int64_t grid = ((total + 3) / 4 + 255) / 256;
  if (grid > 0x7fffffffLL) return fail(BASD_ERR_SHAPE, "resample_u8: %lld workgroups", (long long)grid);
  hipLaunchKernelGGL(resample_u8_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream,
                     (const unsigned char*)src, rec, H, W, S, (unsigned char*)out, total);
  return check_launch("resample_u8");
}

extern "C" int basd_resample_u8_packed(const void* pixels, int64_t pixels_bytes, const int64_t* geom, const int* rec,
                                       int B, int S, void* out, void* stream) {
  using namespace basd;
  if (B == 0) return BASD_OK;
  if (B < 0 || !dual_view_size_ok(S)) return fail(BASD_ERR_SHAPE, "resample_u8_packed: B = %d, S = %d (3 .. 1024)", B, S);
  if (pixels == nullptr || geom == nullptr || rec == nullptr || out == nullptr || pixels_bytes < 0)
    return fail(BASD_ERR_SHAPE, "resample_u8_packed: null pointer or negative pixels_bytes");
  if (((uintptr_t)out & 3) != 0 || ((uintptr_t)rec & 3) != 0 || ((uintptr_t)geom & 7) != 0)
    return fail(BASD_ERR_SHAPE, "resample_u8_packed: out and rec must be 4-byte aligned, geom 8-byte aligned");
  const int bands = (S + PK_ROWS - 1) / PK_ROWS;
  const int64_t grid = (int64_t)B * bands;
  if (grid > 0x7fffffffLL) return fail(BASD_ERR_SHAPE, "resample_u8_packed: %lld workgroups", (long long)grid);
  hipLaunchKernelGGL(resample_u8_packed_kernel, dim3((unsigned)grid), dim3(PK_THREADS), (size_t)pk_lds_bytes(S),
                     (hipStream_t)stream, (const unsigned char*)pixels, pixels_bytes, geom, rec, S, bands,
                     (unsigned char*)out);
  return check_launch("resample_u8_packed");
}

extern "C" int basd_ta_normalize_u8(const void* img, const int* ops, const double* mags, int B, int S, float mean0,
                                    float mean1, float mean2, float std0, float std1, float std2, float* out,
                                    void* stream) {
  using namespace basd;
  if (B <= 0) return BASD_OK;
  if (!dual_view_size_ok(S)) return fail(BASD_ERR_SHAPE, "ta_normalize_u8: S = %d (3 .. 1024)", S);
  if (((uintptr_t)out & 15) != 0) return fail(BASD_ERR_SHAPE, "ta_normalize_u8: out must be 16-byte aligned");
  if (ops != nullptr && mags == nullptr) return fail(BASD_ERR_SHAPE, "ta_normalize_u8: ops without magnitudes");
  Norm nm = {{mean0, mean1, mean2}, {std0, std1, std2}};
  hipLaunchKernelGGL(ta_normalize_u8_kernel, dim3((unsigned)B), dim3(TA_THREADS), 0, (hipStream_t)stream,
                     (const unsigned char*)img, ops, mags, nm, S, out);
  return check_launch("ta_normalize_u8");
}
