// 1-D linear resampling along the token axis (F.interpolate(mode="linear", align_corners=False)), its adjoint, and the
// backward of the importance normalisation of the Procrustes term, as three C entries.
//
// basd_resample_tokens          out[b, i, :] = (1 - fr_i) x[b, lo_i, :] + fr_i x[b, hi_i, :]
// basd_resample_tokens_adjoint  out[b, j, :] = sum_{i: lo_i = j} (1 - fr_i) g[b, i, :] + sum_{i: hi_i = j} fr_i g[b, i, :]
// basd_procrustes_importance_bwd  d loss / d imp from d loss / d a, a = R imp / sum(R imp)
//
// The taps (lo, hi, fr) of output index i are those of procrustes_prep_kernel (stream_kernels.hip), here with the
// multiply and the subtract as separate roundings (no FMA), so that a float32 restatement has the same bits.
//
// The two token kernels stream: a workgroup owns RS_ROWS consecutive OUTPUT rows of one sample, which are contiguous in
// memory, and its threads walk them as one flat run of vectors (16 bytes where the pointers and d allow, see
// resample_vec).  The adjoint is in gather form: lo is monotone in i, so the contributors of row j are the contiguous
// run of i with lo_i in {j - 1, j}; the workgroup keeps lo / fr of all n_out <= 1024 source rows in LDS, finds the start
// of each of its rows by bisection once, and every thread sums its run in ascending i.  No atomics: bitwise
// reproducible, and a row without contributors is written as zeros.
#include "basd_frag.h"

namespace basd {

constexpr int RS_MAX_N = 1024;
constexpr int RS_ROWS = 16;           // output rows per workgroup
constexpr int RS_THREADS = 256;

struct Tap {
  int lo, hi;
  float fr;
};

// taps of output index i of an n_in -> n_out resample.  hipcc contracts a * b - c into one FMA by default, through
// __fmul_rn / __fsub_rn as well (HIP inlines them as plain operators): the pragma keeps the two roundings apart.
__device__ __forceinline__ Tap resample_tap(int i, int n_in, int n_out) {
#pragma clang fp contract(off)
  Tap t;
  if (n_in == n_out) {
    t.lo = i; t.hi = i; t.fr = 0.f;
    return t;
  }
  const float ratio = (float)n_in / (float)n_out;
  const float scaled = ((float)i + 0.5f) * ratio;
  float pos = scaled - 0.5f;
  pos = pos < 0.f ? 0.f : pos;
  int lo = (int)pos;
  if (lo > n_in - 1) lo = n_in - 1;
  t.lo = lo;
  t.hi = lo + 1 < n_in ? lo + 1 : n_in - 1;
  t.fr = pos - (float)lo;
  return t;
}

// V elements of T <-> fp32.  T = float: V in {4, 1}; T = unsigned short (bf16 bits): V in {8, 4, 2, 1}
template <typename T, int V>
__device__ __forceinline__ void load_vec(const T* p, float (&f)[V]) {
  if constexpr (sizeof(T) == 4) {
    if constexpr (V == 4) {
      const float4 v = *reinterpret_cast<const float4*>(p);
      f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
    } else {
      f[0] = p[0];
    }
  } else {
    if constexpr (V == 8) {
      unpack8(*reinterpret_cast<const uint4*>(p), f);
    } else if constexpr (V == 4) {
      const uint2 v = *reinterpret_cast<const uint2*>(p);
      f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xffff0000u);
      f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xffff0000u);
    } else if constexpr (V == 2) {
      const unsigned int v = *reinterpret_cast<const unsigned int*>(p);
      f[0] = __uint_as_float(v << 16); f[1] = __uint_as_float(v & 0xffff0000u);
    } else {
      f[0] = bf16_bits_to_f32(p[0]);
    }
  }
}

template <typename T, int V>
__device__ __forceinline__ void store_vec(T* p, const float (&f)[V]) {
  if constexpr (sizeof(T) == 4) {
    if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2], f[3]);
    else p[0] = f[0];
  } else {
    if constexpr (V == 8) {
      *reinterpret_cast<uint4*>(p) = make_uint4(pack_bf16(f[0], f[1]), pack_bf16(f[2], f[3]), pack_bf16(f[4], f[5]),
                                                pack_bf16(f[6], f[7]));
    } else if constexpr (V == 4) {
      *reinterpret_cast<uint2*>(p) = make_uint2(pack_bf16(f[0], f[1]), pack_bf16(f[2], f[3]));
    } else if constexpr (V == 2) {
      *reinterpret_cast<unsigned int*>(p) = pack_bf16(f[0], f[1]);
    } else {
      p[0] = f32_to_bf16_bits(f[0]);
    }
  }
}

template <typename T, int V>
__global__ __launch_bounds__(RS_THREADS) void resample_tokens_kernel(const T* __restrict__ x, int n_in, int n_out, int d,
                                                                     int tiles, T* __restrict__ out) {
  const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
  const int row0 = tile * RS_ROWS;
  const int rows = n_out - row0 < RS_ROWS ? n_out - row0 : RS_ROWS;
  const int dv = d / V;
  const T* xb = x + (size_t)b * n_in * d;
  T* ob = out + ((size_t)b * n_out + row0) * d;
  for (int idx = threadIdx.x; idx < rows * dv; idx += RS_THREADS) {
    const int r = idx / dv, c = (idx - r * dv) * V;
    const Tap t = resample_tap(row0 + r, n_in, n_out);
    float lo[V], o[V];
    load_vec<T, V>(xb + (size_t)t.lo * d + c, lo);
    if (t.fr != 0.f) {
      float hi[V];
      load_vec<T, V>(xb + (size_t)t.hi * d + c, hi);
      const float wl = 1.f - t.fr;
#pragma unroll
      for (int k = 0; k < V; ++k) o[k] = fmaf(t.fr, hi[k], wl * lo[k]);
    } else {
#pragma unroll
      for (int k = 0; k < V; ++k) o[k] = lo[k];
    }
    store_vec<T, V>(ob + (size_t)r * d + c, o);
  }
}

// lo / fr of the n_out source rows into LDS (all threads of the workgroup; a barrier follows in the caller)
__device__ __forceinline__ void fill_taps(int* s_lo, float* s_fr, int n_in, int n_out) {
  for (int i = threadIdx.x; i < n_out; i += blockDim.x) {
    const Tap t = resample_tap(i, n_in, n_out);
    s_lo[i] = t.lo;
    s_fr[i] = t.fr;
  }
}

// first i in [0, n_out] with lo_i >= j - 1: where the contributors of adjoint row j begin
__device__ __forceinline__ int first_contributor(const int* s_lo, int n_out, int j) {
  int a = 0, e = n_out;
  while (a < e) {
    const int m = (a + e) >> 1;
    if (s_lo[m] < j - 1) a = m + 1;
    else e = m;
  }
  return a;
}

template <typename T, int V>
__global__ __launch_bounds__(RS_THREADS) void resample_adjoint_kernel(const T* __restrict__ g, int n_in, int n_out, int d,
                                                                      int tiles, T* __restrict__ out) {
  __shared__ int s_lo[RS_MAX_N];
  __shared__ float s_fr[RS_MAX_N];
  __shared__ int s_start[RS_ROWS];
  const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
  const int row0 = tile * RS_ROWS;
  const int rows = n_in - row0 < RS_ROWS ? n_in - row0 : RS_ROWS;
  fill_taps(s_lo, s_fr, n_in, n_out);
  __syncthreads();
  if ((int)threadIdx.x < rows) s_start[threadIdx.x] = first_contributor(s_lo, n_out, row0 + threadIdx.x);
  __syncthreads();
  const int dv = d / V;
  const int last = n_in - 1;
  const T* gb = g + (size_t)b * n_out * d;
  T* ob = out + ((size_t)b * n_in + row0) * d;
  for (int idx = threadIdx.x; idx < rows * dv; idx += RS_THREADS) {
    const int r = idx / dv, c = (idx - r * dv) * V;
    const int j = row0 + r;
    float acc[V];
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = 0.f;
    for (int i = s_start[r]; i < n_out; ++i) {
      const int lo = s_lo[i];
      if (lo > j) break;
      const float fr = s_fr[i];
      const int hi = lo + 1 < n_in ? lo + 1 : last;
      const bool by_lo = lo == j, by_hi = hi == j && fr != 0.f;
      if (!(by_lo || by_hi)) continue;
      float v[V];
      load_vec<T, V>(gb + (size_t)i * d + c, v);
      if (by_lo) {
        const float wl = 1.f - fr;
#pragma unroll
        for (int k = 0; k < V; ++k) acc[k] = fmaf(wl, v[k], acc[k]);
      }
      if (by_hi) {
#pragma unroll
        for (int k = 0; k < V; ++k) acc[k] = fmaf(fr, v[k], acc[k]);
      }
    }
    store_vec<T, V>(ob + (size_t)r * d + c, acc);
  }
}

// one workgroup per sample; everything in fp64 from the fp32 inputs and taps, one rounding at the store
__global__ __launch_bounds__(RS_THREADS) void importance_bwd_kernel(const float* __restrict__ g_a,
                                                                    const float* __restrict__ a,
                                                                    const float* __restrict__ imp, int n_s, int n_t,
                                                                    float* __restrict__ g_imp) {
  __shared__ int s_lo[RS_MAX_N];
  __shared__ float s_fr[RS_MAX_N];
  __shared__ double s_gv[RS_MAX_N];
  __shared__ double s_red[2][RS_THREADS / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* ga = g_a + (size_t)b * n_s;
  const float* ab = a + (size_t)b * n_s;
  const float* ib = imp + (size_t)b * n_t;
  fill_taps(s_lo, s_fr, n_t, n_s);
  __syncthreads();
  const int last = n_t - 1;
  // tot = sum_i (R imp)_i and dot = sum_k a_k g_a_k: per-thread strided partials, the xor tree of a wave, then the
  // waves in order
  double tot = 0.0, dot = 0.0;
  for (int i = tid; i < n_s; i += RS_THREADS) {
    const int lo = s_lo[i];
    const float fr = s_fr[i];
    double v = (double)ib[lo];
    if (fr != 0.f) {
      const int hi = lo + 1 < n_t ? lo + 1 : last;
      v = (1.0 - (double)fr) * v + (double)fr * (double)ib[hi];
    }
    tot += v;
    dot += (double)ab[i] * (double)ga[i];
  }
  tot = wave_sum_d(tot);
  dot = wave_sum_d(dot);
  if ((tid & 63) == 0) { s_red[0][tid >> 6] = tot; s_red[1][tid >> 6] = dot; }
  __syncthreads();
  tot = 0.0; dot = 0.0;
  for (int w = 0; w < RS_THREADS / 64; ++w) { tot += s_red[0][w]; dot += s_red[1][w]; }
  for (int i = tid; i < n_s; i += RS_THREADS) s_gv[i] = ((double)ga[i] - dot) / tot;
  __syncthreads();
  // g_imp = R^T g_v, gather form as in resample_adjoint_kernel
  for (int j = tid; j < n_t; j += RS_THREADS) {
    double acc = 0.0;
    for (int i = first_contributor(s_lo, n_s, j); i < n_s; ++i) {
      const int lo = s_lo[i];
      if (lo > j) break;
      const float fr = s_fr[i];
      const int hi = lo + 1 < n_t ? lo + 1 : last;
      if (lo == j) acc += (1.0 - (double)fr) * s_gv[i];
      if (hi == j && fr != 0.f) acc += (double)fr * s_gv[i];
    }
    g_imp[(size_t)b * n_t + j] = (float)acc;
  }
}

// widest vector (in elements) both pointers and the row length allow
static int resample_vec(const void* x, const void* out, int d, int elem_bytes) {
  const uintptr_t both = (uintptr_t)x | (uintptr_t)out;
  for (int v = 16 / elem_bytes; v > 1; v >>= 1)
    if (d % v == 0 && both % (uintptr_t)(v * elem_bytes) == 0) return v;
  return 1;
}

template <bool ADJOINT, typename T, int V>
static void launch_resample(const void* x, int n_in, int n_out, int d, int tiles, unsigned grid, void* out,
                            hipStream_t st) {
  if constexpr (ADJOINT)
    hipLaunchKernelGGL((resample_adjoint_kernel<T, V>), dim3(grid), dim3(RS_THREADS), 0, st, (const T*)x, n_in, n_out, d,
                       tiles, (T*)out);
  else
    hipLaunchKernelGGL((resample_tokens_kernel<T, V>), dim3(grid), dim3(RS_THREADS), 0, st, (const T*)x, n_in, n_out, d,
                       tiles, (T*)out);
}

template <bool ADJOINT>
static int resample_entry(const char* what, const void* x, int dtype, int batch, int n_in, int n_out, int d, void* out,
                          void* stream) {
  if (dtype != BASD_DTYPE_F32 && dtype != BASD_DTYPE_BF16) return fail(BASD_ERR_DTYPE, "%s: dtype %d", what, dtype);
  if (batch < 1 || n_in < 1 || n_in > RS_MAX_N || n_out < 1 || n_out > RS_MAX_N || d < 4 || d % 4)
    return fail(BASD_ERR_SHAPE, "%s: batch=%d n_in=%d n_out=%d (1 .. %d) d=%d (a multiple of 4)", what, batch, n_in,
                n_out, RS_MAX_N, d);
  if (x == nullptr || out == nullptr) return fail(BASD_ERR_SHAPE, "%s: null pointer", what);
  const int eb = dtype == BASD_DTYPE_F32 ? 4 : 2;
  if (((uintptr_t)x | (uintptr_t)out) % (uintptr_t)eb)
    return fail(BASD_ERR_SHAPE, "%s: pointers must be aligned to the element size", what);
  const int n_rows = ADJOINT ? n_in : n_out;                 // rows of the output
  const int tiles = (n_rows + RS_ROWS - 1) / RS_ROWS;
  const int64_t grid = (int64_t)batch * tiles;
  if (grid > 0x7fffffffLL) return fail(BASD_ERR_SHAPE, "%s: %lld workgroups", what, (long long)grid);
  hipStream_t st = (hipStream_t)stream;
  const int v = resample_vec(x, out, d, eb);
  const unsigned gr = (unsigned)grid;
  if (eb == 4) {
    if (v == 4) launch_resample<ADJOINT, float, 4>(x, n_in, n_out, d, tiles, gr, out, st);
    else launch_resample<ADJOINT, float, 1>(x, n_in, n_out, d, tiles, gr, out, st);
  } else {
    if (v == 8) launch_resample<ADJOINT, unsigned short, 8>(x, n_in, n_out, d, tiles, gr, out, st);
    else if (v == 4) launch_resample<ADJOINT, unsigned short, 4>(x, n_in, n_out, d, tiles, gr, out, st);
    else if (v == 2) launch_resample<ADJOINT, unsigned short, 2>(x, n_in, n_out, d, tiles, gr, out, st);
    else launch_resample<ADJOINT, unsigned short, 1>(x, n_in, n_out, d, tiles, gr, out, st);
  }
  return check_launch(what);
}

}  // namespace basd

extern "C" int basd_resample_tokens(const void* x, int dtype, int batch, int n_in, int n_out, int d, void* out,
                                    void* stream) {
  return basd::resample_entry<false>("resample_tokens", x, dtype, batch, n_in, n_out, d, out, stream);
}

extern "C" int basd_resample_tokens_adjoint(const void* g, int dtype, int batch, int n_in, int n_out, int d, void* out,
                                            void* stream) {
  return basd::resample_entry<true>("resample_tokens_adjoint", g, dtype, batch, n_in, n_out, d, out, stream);
}

extern "C" int basd_procrustes_importance_bwd(const float* g_a, const float* a, const float* imp, int batch, int n_s,
                                              int n_t, float* g_imp, void* stream) {
  using namespace basd;
  if (batch < 1 || n_s < 1 || n_s > RS_MAX_N || n_t < 1 || n_t > RS_MAX_N)
    return fail(BASD_ERR_SHAPE, "procrustes_importance_bwd: batch=%d n_s=%d n_t=%d (1 .. %d)", batch, n_s, n_t, RS_MAX_N);
  if (g_a == nullptr || a == nullptr || imp == nullptr || g_imp == nullptr)
    return fail(BASD_ERR_SHAPE, "procrustes_importance_bwd: null pointer");
  if (((uintptr_t)g_a | (uintptr_t)a | (uintptr_t)imp | (uintptr_t)g_imp) & 3)
    return fail(BASD_ERR_SHAPE, "procrustes_importance_bwd: pointers must be 4-byte aligned");
  hipLaunchKernelGGL(importance_bwd_kernel, dim3((unsigned)batch), dim3(RS_THREADS), 0, (hipStream_t)stream, g_a, a, imp,
                     n_s, n_t, g_imp);
  return check_launch("procrustes_importance_bwd");
}
