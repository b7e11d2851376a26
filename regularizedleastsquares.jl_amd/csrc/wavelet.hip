// WaveletOp: orthogonal, periodic wavelet transform of 1-D signals and 2-D images (LinearOperatorCollection.WaveletOp is third-party
// to the reference, like GradientOp: restated from its definition) and the prox of lambda ||W x||_1.
//
// Real filter h of even length L (Haar: 2, db2: 4), g[k] = (-1)^k h[L-1-k].  One analysis level on a line s of even length m:
//     a[i] = sum_k h[k] s[(2i + k) mod m],   d[i] = sum_k g[k] s[(2i + k) mod m],   i = 0 .. m/2 - 1,   output [a | d];
// synthesis is its transpose, gathered: s[2i + p] = sum_q h[2q + p] a[(i - q) mod m/2] + g[2q + p] d[(i - q) mod m/2].
// Level j acts on the leading (n1 >> j) x (n2 >> j) block: along dimension 1 for every column, then along dimension 2 for every row.
//
// Two paths, the same arithmetic (wv_ana / wv_syn: explicit fma chains in one order, so their results are the same bits):
//   * general: one launch per level and dimension, block -> scratch -> block (the handle owns the scratch image); any size;
//   * single workgroup: the image and a second copy of it in ONE workgroup's LDS, every level there, optionally the soft threshold
//     of prox.hip's L1 between analysis and synthesis -- forward + threshold + inverse in one launch (the FISTA plan's prox launch).
// wv_fused_fits / wv_use_fused (host) are THE statement of which path runs.
#include "rls_common.hpp"

namespace {

constexpr int WV_THREADS = 256;          // general path
constexpr int WV_FUSED_THREADS = 1024;   // single-workgroup path (256 for images of up to WV_FUSED_SMALL_N elements)
constexpr int64_t WV_FUSED_SMALL_N = 2048;
constexpr size_t WV_LDS_BUDGET = 160 * 1024 - 512;
enum { WV_FWD = 1, WV_THR = 2, WV_INV = 4 };

template <typename E>
struct wv;  // the scalar type of E and the real filter's arithmetic on it (real and imaginary part alike)
template <>
struct wv<float> {
  using T = float;
  __device__ static inline float mul(float h, float s) { return h * s; }
  __device__ static inline float fma(float h, float s, float a) { return fmaf(h, s, a); }
  __device__ static inline float soft(float v, float thr) { return fista_prox_elem<float>(v, RLS_REG_L1, thr); }
};
template <>
struct wv<float2> {
  using T = float;
  __device__ static inline float2 mul(float h, float2 s) { return make_float2(h * s.x, h * s.y); }
  __device__ static inline float2 fma(float h, float2 s, float2 a) { return make_float2(fmaf(h, s.x, a.x), fmaf(h, s.y, a.y)); }
  __device__ static inline float2 soft(float2 v, float thr) { return fista_prox_elem<float2>(v, RLS_REG_L1, thr); }
};
template <>
struct wv<double> {
  using T = double;
  __device__ static inline double mul(double h, double s) { return h * s; }
  __device__ static inline double fma(double h, double s, double a) { return ::fma(h, s, a); }
  __device__ static inline double soft(double v, double thr) { return dp_prox_elem<double>(v, RLS_REG_L1, thr); }
};
template <>
struct wv<double2> {
  using T = double;
  __device__ static inline double2 mul(double h, double2 s) { return make_double2(h * s.x, h * s.y); }
  __device__ static inline double2 fma(double h, double2 s, double2 a) { return make_double2(::fma(h, s.x, a.x), ::fma(h, s.y, a.y)); }
  __device__ static inline double2 soft(double2 v, double thr) { return dp_prox_elem<double2>(v, RLS_REG_L1, thr); }
};

template <typename T>
struct wv_taps {
  T h[4], g[4];  // (Haar: the upper two unused)
};

// a[i], d[i] from s[2i .. 2i+L-1] (indices already wrapped)
template <typename E, int L>
__device__ static inline void wv_ana(const wv_taps<typename wv<E>::T>& f, E s0, E s1, E s2, E s3, E& a, E& d) {
  a = wv<E>::mul(f.h[0], s0);
  a = wv<E>::fma(f.h[1], s1, a);
  d = wv<E>::mul(f.g[0], s0);
  d = wv<E>::fma(f.g[1], s1, d);
  if constexpr (L == 4) {
    a = wv<E>::fma(f.h[2], s2, a);
    a = wv<E>::fma(f.h[3], s3, a);
    d = wv<E>::fma(f.g[2], s2, d);
    d = wv<E>::fma(f.g[3], s3, d);
  }
}
// s[2i], s[2i+1] from a[i], a[i-1], d[i], d[i-1] (indices already wrapped; Haar reads only a[i], d[i])
template <typename E, int L>
__device__ static inline void wv_syn(const wv_taps<typename wv<E>::T>& f, E ai, E ap, E di, E dp, E& se, E& so) {
  se = wv<E>::mul(f.h[0], ai);
  so = wv<E>::mul(f.h[1], ai);
  if constexpr (L == 4) {
    se = wv<E>::fma(f.h[2], ap, se);
    so = wv<E>::fma(f.h[3], ap, so);
  }
  se = wv<E>::fma(f.g[0], di, se);
  so = wv<E>::fma(f.g[1], di, so);
  if constexpr (L == 4) {
    se = wv<E>::fma(f.g[2], dp, se);
    so = wv<E>::fma(f.g[3], dp, so);
  }
}

// ---- general path: one level along one dimension of the leading m1 x m2 block (columns ld apart in src and dst, src != dst).
// DIM2 = false: along dimension 1, a thread per coefficient pair, consecutive threads on consecutive pairs of one column;
// DIM2 = true: along dimension 2, consecutive threads on consecutive ROWS (dimension 1) of one pair of columns, so every load and
// store of a wave is one contiguous run along dimension 1.
template <typename E, int L, bool DIM2, bool SYN>
__global__ __launch_bounds__(WV_THREADS) void wavelet_level_kernel(const E* __restrict__ src, E* __restrict__ dst, int64_t ld, int64_t m1,
                                                                   int64_t m2, wv_taps<typename wv<E>::T> f) {
  const int64_t m = DIM2 ? m2 : m1, half = m / 2;
  const int64_t total = DIM2 ? m1 * half : half * m2;
  const int64_t es = DIM2 ? ld : 1;  // distance of two neighbours along the transformed dimension
  for (int64_t idx = (int64_t)blockIdx.x * WV_THREADS + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * WV_THREADS) {
    int64_t i, off;
    if constexpr (DIM2) {
      i = idx / m1;
      off = idx - i * m1;
    } else {
      const int64_t c = idx / half;
      i = idx - c * half;
      off = c * ld;
    }
    const E* s = src + off;
    E* o = dst + off;
    if constexpr (!SYN) {
      int64_t k2 = 2 * i + 2, k3 = 2 * i + 3;  // (2i + k) mod m: at most one wrap for m >= 2
      if (k2 >= m) k2 -= m;
      if (k3 >= m) k3 -= m;
      const E s0 = s[2 * i * es], s1 = s[(2 * i + 1) * es];
      E s2 = s0, s3 = s0;
      if constexpr (L == 4) s2 = s[k2 * es], s3 = s[k3 * es];
      E a, d;
      wv_ana<E, L>(f, s0, s1, s2, s3, a, d);
      o[i * es] = a;
      o[(half + i) * es] = d;
    } else {
      const int64_t ip = i == 0 ? half - 1 : i - 1;
      const E ai = s[i * es], di = s[(half + i) * es];
      E ap = ai, dp = di;
      if constexpr (L == 4) ap = s[ip * es], dp = s[(half + ip) * es];
      E se, so;
      wv_syn<E, L>(f, ai, ap, di, dp, se, so);
      o[2 * i * es] = se;
      o[(2 * i + 1) * es] = so;
    }
  }
}

// ---- single-workgroup path.  The stride-2 reads of the analysis along dimension 1 (and the stride-2 writes of its synthesis) go
// through LDS as PAIRS -- (s[2i], s[2i+1]) is one 8 / 16-byte access per lane, consecutive lanes on consecutive pairs: no two lanes
// of a group on one bank, where a stride-2 ds_read_b32 would put lanes l and l + 16 on the same one.  Along dimension 2 consecutive
// lanes hold consecutive rows, i.e. consecutive addresses.  (Blocks narrower than a lane group -- the deepest levels, < 1/16 of the
// work -- wrap to the next column pair and may share banks.)
template <typename E>
struct alignas(2 * sizeof(E)) wv_pair {
  E lo, hi;
};

template <typename E, int L, bool SYN>
__device__ static inline void wv_lds_dim1(const E* __restrict__ src, E* __restrict__ dst, int ld, int m1, int m2,
                                          const wv_taps<typename wv<E>::T>& f) {
  const int half = m1 / 2, total = half * m2;
  for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
    const int c = idx / half, i = idx - c * half;
    const E* s = src + c * ld;
    E* o = dst + c * ld;
    if constexpr (!SYN) {
      int k2 = 2 * i + 2;
      if (k2 >= m1) k2 -= m1;
      const wv_pair<E> p0 = *reinterpret_cast<const wv_pair<E>*>(s + 2 * i);
      wv_pair<E> p1 = p0;
      if constexpr (L == 4) p1 = *reinterpret_cast<const wv_pair<E>*>(s + k2);
      E a, d;
      wv_ana<E, L>(f, p0.lo, p0.hi, p1.lo, p1.hi, a, d);
      o[i] = a;
      o[half + i] = d;
    } else {
      const int ip = i == 0 ? half - 1 : i - 1;
      const E ai = s[i], di = s[half + i];
      E ap = ai, dp = di;
      if constexpr (L == 4) ap = s[ip], dp = s[half + ip];
      wv_pair<E> r;
      wv_syn<E, L>(f, ai, ap, di, dp, r.lo, r.hi);
      *reinterpret_cast<wv_pair<E>*>(o + 2 * i) = r;
    }
  }
}

template <typename E, int L, bool SYN>
__device__ static inline void wv_lds_dim2(const E* __restrict__ src, E* __restrict__ dst, int ld, int m1, int m2,
                                          const wv_taps<typename wv<E>::T>& f) {
  const int half = m2 / 2, total = m1 * half;
  for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
    const int i = idx / m1, r = idx - i * m1;
    const E* s = src + r;
    E* o = dst + r;
    if constexpr (!SYN) {
      int k2 = 2 * i + 2, k3 = 2 * i + 3;
      if (k2 >= m2) k2 -= m2;
      if (k3 >= m2) k3 -= m2;
      const E s0 = s[2 * i * ld], s1 = s[(2 * i + 1) * ld];
      E s2 = s0, s3 = s0;
      if constexpr (L == 4) s2 = s[k2 * ld], s3 = s[k3 * ld];
      E a, d;
      wv_ana<E, L>(f, s0, s1, s2, s3, a, d);
      o[i * ld] = a;
      o[(half + i) * ld] = d;
    } else {
      const int ip = i == 0 ? half - 1 : i - 1;
      const E ai = s[i * ld], di = s[(half + i) * ld];
      E ap = ai, dp = di;
      if constexpr (L == 4) ap = s[ip * ld], dp = s[(half + ip) * ld];
      E se, so;
      wv_syn<E, L>(f, ai, ap, di, dp, se, so);
      o[2 * i * ld] = se;
      o[(2 * i + 1) * ld] = so;
    }
  }
}

// y = W x (WV_FWD), W^T x (WV_INV) or W^T soft(W x, thr) (all three); x may be y.  n2 == 1: a signal.  *skip != 0: nothing (the FISTA
// plan's `done`).  Dynamic LDS: 2 n1 n2 elements.
template <typename E, int L>
__global__ __launch_bounds__(WV_FUSED_THREADS) void wavelet_fused_kernel(const E* x, E* y, int n1, int n2, int J, wv_taps<typename wv<E>::T> f,
                                                                         int mode, typename wv<E>::T thr, const int* skip) {
  extern __shared__ __align__(32) unsigned char wv_smem[];
  if (skip && *skip) return;
  const int N = n1 * n2;
  E* b0 = reinterpret_cast<E*>(wv_smem);
  E* b1 = b0 + N;
  for (int i = threadIdx.x; i < N; i += blockDim.x) b0[i] = x[i];
  __syncthreads();
  if (mode & WV_FWD) {
    for (int j = 0; j < J; ++j) {
      const int m1 = n1 >> j, m2 = n2 > 1 ? n2 >> j : 1;
      wv_lds_dim1<E, L, false>(b0, b1, n1, m1, m2, f);
      __syncthreads();
      if (n2 > 1) {
        wv_lds_dim2<E, L, false>(b1, b0, n1, m1, m2, f);
      } else {
        for (int i = threadIdx.x; i < m1; i += blockDim.x) b0[i] = b1[i];
      }
      __syncthreads();
    }
  }
  if (mode & WV_THR) {
    for (int i = threadIdx.x; i < N; i += blockDim.x) b0[i] = wv<E>::soft(b0[i], thr);
    __syncthreads();
  }
  if (mode & WV_INV) {
    for (int j = J - 1; j >= 0; --j) {
      const int m1 = n1 >> j, m2 = n2 > 1 ? n2 >> j : 1;
      if (n2 > 1) {
        wv_lds_dim2<E, L, true>(b0, b1, n1, m1, m2, f);
        __syncthreads();
        wv_lds_dim1<E, L, true>(b1, b0, n1, m1, m2, f);
      } else {
        wv_lds_dim1<E, L, true>(b0, b1, n1, m1, 1, f);
        __syncthreads();
        for (int i = threadIdx.x; i < m1; i += blockDim.x) b0[i] = b1[i];
      }
      __syncthreads();
    }
  }
  for (int i = threadIdx.x; i < N; i += blockDim.x) y[i] = b0[i];
}

static inline size_t wv_elem_size(int32_t dtype) { return dtype == RLS_F32 ? 4 : dtype == RLS_C64 ? 16 : 8; }

// calls fn(rls_type<E>{}, integral_constant<int, L>{}) for the handle's element type and filter length
template <typename F>
static inline int32_t wv_dispatch(int32_t dtype, int flen, F&& fn) {
  return rls_with<2, 4>(flen, [&](auto l) {
    if (dtype == RLS_F64 || dtype == RLS_C64) return rls_with_elem64(dtype, [&](auto t) { return fn(t, l); });
    return rls_with_elem(dtype, [&](auto t) { return fn(t, l); });
  });
}

}  // namespace

struct rls_wavelet {
  rls_ctx* ctx = nullptr;
  uint64_t ctx_id = 0;
  int32_t dtype = RLS_F32;
  int64_t n1 = 1, n2 = 1;  // the transformed extents (unit dimensions dropped); n2 == 1: a signal
  int32_t J = 0, flen = 4;
  double h[4] = {0, 0, 0, 0}, g[4] = {0, 0, 0, 0};
  void* tmp = nullptr;  // the general path's scratch image
  uint64_t serial = 0;  // unique per handle of this process: what a plan that caches launches of this handle compares (plan_fista.hip)
};

namespace {

template <typename T>
static wv_taps<T> wv_make_taps(const rls_wavelet* w) {
  wv_taps<T> f;
  for (int k = 0; k < 4; ++k) f.h[k] = (T)w->h[k], f.g[k] = (T)w->g[k];
  return f;
}

// the image and its second copy fit one workgroup's LDS
static bool wv_fused_fits(const rls_wavelet* w) {
  return w->J >= 1 && (size_t)2 * (size_t)(w->n1 * w->n2) * wv_elem_size(w->dtype) <= WV_LDS_BUDGET;
}
// THE choice between the two paths: the single-workgroup kernel whenever the image fits (profiles/wavelet.txt: it is ahead of the
// general path's 2 J launches at every size that fits), unless rls_tune_set("wavelet_fused", 0) forces the general path
static bool wv_use_fused(const rls_wavelet* w) { return w->ctx->tune.wavelet_fused != 0 && wv_fused_fits(w); }

static int32_t wv_fused_launch(rls_wavelet* w, const void* x, void* y, int mode, double thr, const int* skip) {
  rls_ctx* ctx = w->ctx;
  const int64_t N = w->n1 * w->n2;
  const size_t lds = (size_t)2 * N * wv_elem_size(w->dtype);
  const unsigned nt = N <= WV_FUSED_SMALL_N ? 256 : WV_FUSED_THREADS;
  return wv_dispatch(w->dtype, w->flen, [&](auto t, auto l) {
    using E = typename decltype(t)::type;
    using T = typename wv<E>::T;
    constexpr int L = decltype(l)::value;
    // (every launch of an instantiation is allowed the whole budget: rls_allow_lds sets the attribute once per device)
    const hipError_t e = rls_allow_lds<wavelet_fused_kernel<E, L>>(ctx->device, WV_LDS_BUDGET);
    if (e != hipSuccess) return rls_fail(ctx, (int32_t)e, "hipFuncSetAttribute (dynamic LDS) failed");
    hipLaunchKernelGGL((wavelet_fused_kernel<E, L>), dim3(1), dim3(nt), lds, ctx->stream, (const E*)x, (E*)y, (int)w->n1, (int)w->n2,
                       (int)w->J, wv_make_taps<T>(w), mode, (T)thr, skip);
    return launch_status(ctx);
  });
}

static inline unsigned wv_grid(int64_t total) {
  int64_t g = (total + WV_THREADS - 1) / WV_THREADS;
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  return (unsigned)g;
}

template <typename E, int L, bool DIM2, bool SYN>
static int32_t wv_level(rls_wavelet* w, const void* src, void* dst, int64_t m1, int64_t m2) {
  const int64_t total = DIM2 ? m1 * (m2 / 2) : (m1 / 2) * m2;
  return rls_launch<wavelet_level_kernel<E, L, DIM2, SYN>>(w->ctx, dim3(wv_grid(total)), dim3(WV_THREADS), 0, (const E*)src, (E*)dst, w->n1, m1,
                                                           m2, wv_make_taps<typename wv<E>::T>(w));
}

static int32_t wv_general(rls_wavelet* w, bool adjoint, const void* x, void* y) {
  rls_ctx* ctx = w->ctx;
  const size_t es = wv_elem_size(w->dtype);
  const int64_t N = w->n1 * w->n2;
  const bool img = w->n2 > 1;
  if ((adjoint || w->J == 0) && x != y) RLS_HIP(ctx, hipMemcpyAsync(y, x, (size_t)N * es, hipMemcpyDeviceToDevice, ctx->stream));
  if (w->J == 0) return 0;
  return wv_dispatch(w->dtype, w->flen, [&](auto t, auto l) -> int32_t {
    using E = typename decltype(t)::type;
    constexpr int L = decltype(l)::value;
    if (!adjoint) {
      const void* src = x;  // level 0 covers the whole image: it may read x where x != y
      for (int j = 0; j < w->J; ++j, src = y) {
        const int64_t m1 = w->n1 >> j, m2 = img ? w->n2 >> j : 1;
        RLS_TRY((wv_level<E, L, false, false>(w, src, w->tmp, m1, m2)));
        if (img) RLS_TRY((wv_level<E, L, true, false>(w, w->tmp, y, m1, m2)));
        else RLS_HIP(ctx, hipMemcpyAsync(y, w->tmp, (size_t)m1 * es, hipMemcpyDeviceToDevice, ctx->stream));
      }
    } else {
      for (int j = w->J - 1; j >= 0; --j) {
        const int64_t m1 = w->n1 >> j, m2 = img ? w->n2 >> j : 1;
        if (img) {
          RLS_TRY((wv_level<E, L, true, true>(w, y, w->tmp, m1, m2)));
          RLS_TRY((wv_level<E, L, false, true>(w, w->tmp, y, m1, m2)));
        } else {
          RLS_TRY((wv_level<E, L, false, true>(w, y, w->tmp, m1, 1)));
          RLS_HIP(ctx, hipMemcpyAsync(y, w->tmp, (size_t)m1 * es, hipMemcpyDeviceToDevice, ctx->stream));
        }
      }
    }
    return 0;
  });
}

static bool wv_live(const rls_wavelet* w) { return w && rls_ctx_alive(w->ctx, w->ctx_id); }

}  // namespace

// ---- what the FISTA plan (plan_fista.hip) needs of a handle
bool rls_wavelet_single_ok(const rls_wavelet* w, const rls_ctx* ctx, int32_t dtype, int64_t n) {
  return wv_live(w) && w->ctx == ctx && w->dtype == dtype && w->n1 * w->n2 == n && wv_use_fused(w);
}
uint64_t rls_wavelet_serial(const rls_wavelet* w) { return w->serial; }
int32_t rls_wavelet_prox_launch(rls_wavelet* w, const void* in, void* out, float thr, const int* skip) {
  return wv_fused_launch(w, in, out, WV_FWD | WV_THR | WV_INV, (double)thr, skip);
}

extern "C" {

int32_t rls_wavelet_create(rls_ctx* ctx, int32_t dtype, int32_t ndims, const int64_t* shape, int32_t filter_kind, int32_t levels,
                           rls_wavelet** out) {
  RLS_CHECK_CTX(ctx);
  if (!out) return rls_fail(ctx, RLS_E_INVALID, "wavelet_create: null out");
  *out = nullptr;
  if (dtype < RLS_F32 || dtype > RLS_C64 || ndims < 1 || !shape || (filter_kind != RLS_WT_HAAR && filter_kind != RLS_WT_DB2))
    return rls_fail(ctx, RLS_E_INVALID, "wavelet_create: bad argument");
  int64_t ext[2] = {1, 1};
  int nd = 0;
  for (int k = 0; k < ndims; ++k) {
    if (shape[k] < 1) return rls_fail(ctx, RLS_E_INVALID, "wavelet_create: extents must be positive");
    if (shape[k] == 1) continue;  // unit dimensions are dropped
    if (nd == 2) return rls_fail(ctx, RLS_E_INVALID, "wavelet_create: 1-D and 2-D shapes only");
    ext[nd++] = shape[k];
  }
  if (ext[0] > ((int64_t)1 << 31) || ext[1] > ((int64_t)1 << 31) || ext[0] * ext[1] > ((int64_t)1 << 40))
    return rls_fail(ctx, RLS_E_INVALID, "wavelet_create: image too large");
  int maxJ = 0;
  if (nd > 0)
    while (maxJ < 40 && ext[0] % ((int64_t)2 << maxJ) == 0 && (nd < 2 || ext[1] % ((int64_t)2 << maxJ) == 0)) ++maxJ;
  if (levels > maxJ) return rls_fail(ctx, RLS_E_INVALID, "wavelet_create: an extent is not divisible by 2^levels");
  rls_wavelet* w = new rls_wavelet();
  static std::atomic<uint64_t> serials{0};
  w->serial = ++serials;
  w->ctx = ctx;
  w->ctx_id = ctx->id;
  w->dtype = dtype;
  w->n1 = ext[0];
  w->n2 = ext[1];
  w->J = levels < 0 ? maxJ : levels;
  const double r2 = 1.4142135623730951, r3 = 1.7320508075688772;
  if (filter_kind == RLS_WT_HAAR) {
    w->flen = 2;
    w->h[0] = w->h[1] = 1.0 / r2;
  } else {
    w->flen = 4;
    const double den = 4.0 * r2;
    w->h[0] = (1.0 + r3) / den, w->h[1] = (3.0 + r3) / den, w->h[2] = (3.0 - r3) / den, w->h[3] = (1.0 - r3) / den;
  }
  for (int k = 0; k < w->flen; ++k) w->g[k] = ((k & 1) ? -1.0 : 1.0) * w->h[w->flen - 1 - k];
  if (w->J > 0) {
    const hipError_t e0 = rls_enter(ctx);
    const hipError_t e = e0 != hipSuccess ? e0 : rls_dev_alloc(ctx, &w->tmp, (size_t)(w->n1 * w->n2) * wv_elem_size(dtype));
    if (e != hipSuccess) {
      delete w;
      return rls_fail(ctx, RLS_E_WORKSPACE, "wavelet_create: allocation failed");
    }
  }
  *out = w;
  return 0;
}

int32_t rls_wavelet_destroy(rls_wavelet* w) {
  if (!w) return RLS_E_INVALID;
  if (w->tmp) rls_dev_free(wv_live(w) ? w->ctx : nullptr, w->tmp);
  delete w;
  return 0;
}

int32_t rls_wavelet_levels(rls_wavelet* w, int32_t* out) {
  if (!w || !out) return RLS_E_INVALID;
  *out = w->J;
  return 0;
}

int32_t rls_wavelet_apply(rls_wavelet* w, int32_t adjoint, const void* x, void* y) {
  if (!wv_live(w)) return RLS_E_INVALID;
  rls_ctx* ctx = w->ctx;
  if (!x || !y || (adjoint != 0 && adjoint != 1)) return rls_fail(ctx, RLS_E_INVALID, "wavelet_apply: bad argument");
  RLS_HIP(ctx, rls_enter(ctx));
  if (wv_use_fused(w)) return wv_fused_launch(w, x, y, adjoint ? WV_INV : WV_FWD, 0.0, nullptr);
  return wv_general(w, adjoint != 0, x, y);
}

int32_t rls_prox_wavelet_l1(rls_wavelet* w, void* x, double lambda) {
  if (!wv_live(w)) return RLS_E_INVALID;
  rls_ctx* ctx = w->ctx;
  if (!x) return rls_fail(ctx, RLS_E_INVALID, "prox_wavelet_l1: null x");
  RLS_HIP(ctx, rls_enter(ctx));
  if (wv_use_fused(w)) return wv_fused_launch(w, x, x, WV_FWD | WV_THR | WV_INV, lambda, nullptr);
  const int64_t N = w->n1 * w->n2;
  RLS_TRY(wv_general(w, false, x, x));
  if (w->dtype == RLS_F64 || w->dtype == RLS_C64) RLS_TRY(rls_prox_l1_d(ctx, w->dtype, N, x, lambda));
  else RLS_TRY(rls_prox_l1(ctx, w->dtype, N, x, (float)lambda));
  return wv_general(w, true, x, x);
}

}  // extern "C"
