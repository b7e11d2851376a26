// Matrix-free RadonOp: the operator of the reference's computed-tomography example
// (docs/src/literate/examples/computed_tomography.jl).  RadonKA.jl is third-party to the reference, like the operators of fft.hip:
// the operator is DEFINED here as the exact parallel-beam line integral of a piecewise-constant image, in closed form.
//
// Layout.  Image n1 x n2, column-major: pixel (i, j) is element i + n1 j, its centre at xr = i - (n1 - 1) / 2, yr = j - (n2 - 1) / 2.
// D detector bins per angle, t_k = k - (D - 1) / 2; sinogram D x nA, detector fastest: row k + D q.  M = D nA, N = n1 n2.
// Entry.   A[k + D q, i + n1 j] = w(|t_k - (xr c_q + yr s_q)|), the chord of the line through the unit pixel:
//            mn > 0:  w(d) = clamp((hi - d) / mn, 0, 1) / mx;     mn = 0:  w(d) = 1 / mx (d < hi), 0.5 / mx (d == hi), 0 otherwise
//          with mx = max(|c|, |s|), mn = min(|c|, |s|), hi = (|c| + |s|) / 2.  The table (radon_entry, one per angle) is computed in
//          double on the host -- angles within 2^-40 of an axis are snapped onto it -- and stored in the element's real type; the two
//          divisions are multiplications by the table's reciprocals.
//
// radon_weight is THE evaluation of an entry: the forward, adjoint and densify kernels all call it with (k, i, j, entry), so all three
// see the same bits for every entry (explicit fma, no expression the compiler could contract differently from one caller to the next).
//
// Forward:  a lane per ray, a wave on 64 consecutive detectors of ONE angle (the entry and the marching axis are wave-uniform).  The
//           ray marches along the major axis (i when |s| >= |c|, else j), solves for the minor coordinate and evaluates the three
//           pixels around its rounded value: a pixel with a non-zero weight lies within hi / mx <= 1 of the solution.
// Adjoint:  L lanes per pixel (1, 4, 16, 64), i fastest across a wave; lane s walks angles s, s + L, ... in order and evaluates the three
//           bins around round(xr c + yr s + (D - 1) / 2) (hi < 1); the L partials meet in the fixed butterfly sparse.hip uses.
// No atomics: every output element is summed by one lane or one group in a fixed order, the same bits run to run.  Sums are carried
// in the element's real type (Float32 for Float32 / ComplexF32), like the sparse products.
#include <cmath>
#include <vector>

#include "rls_common.hpp"

namespace {

constexpr int RD_THREADS = 256;
constexpr int RD_WAVES = RD_THREADS / RLS_WAVE;
constexpr int RD_MAX_BLOCKS = 2048 * 8;  // more work than one pass covers: grid stride

template <typename E>
struct rde;  // the scalar type of E
template <>
struct rde<float> {
  using R = float;
  static constexpr bool cplx = false;
};
template <>
struct rde<float2> {
  using R = float;
  static constexpr bool cplx = true;
};
template <>
struct rde<double> {
  using R = double;
  static constexpr bool cplx = false;
};
template <>
struct rde<double2> {
  using R = double;
  static constexpr bool cplx = true;
};

// one angle: c, s (snapped), hi = (|c| + |s|) / 2, rmn = 1 / mn (0 when mn = 0), rmx = 1 / mx
template <typename R>
struct alignas(8 * sizeof(R)) radon_entry {
  R c, s, hi, rmn, rmx, pad0, pad1, pad2;
};
// the centres: ct = (D - 1) / 2, cx = (n1 - 1) / 2, cy = (n2 - 1) / 2 (half-integers: exact in every real type)
template <typename R>
struct radon_geom {
  int n1, n2, D, nA;
  R ct, cx, cy;
};

__device__ static inline float rd_fma(float a, float b, float c) { return fmaf(a, b, c); }
__device__ static inline double rd_fma(double a, double b, double c) { return ::fma(a, b, c); }
__device__ static inline float rd_abs(float a) { return fabsf(a); }
__device__ static inline double rd_abs(double a) { return fabs(a); }
__device__ static inline float rd_rint(float a) { return rintf(a); }
__device__ static inline double rd_rint(double a) { return rint(a); }
__device__ static inline float rd_dpp(float v, int ctrl) { return dpp_f(v, ctrl); }
__device__ static inline double rd_dpp(double v, int ctrl) { return dpp_d(v, ctrl); }

template <typename E>
__device__ static inline typename rde<E>::R rd_re(E v) {
  if constexpr (rde<E>::cplx) return v.x;
  else return v;
}
template <typename E>
__device__ static inline typename rde<E>::R rd_im(E v) {
  if constexpr (rde<E>::cplx) return v.y;
  else return 0;
}
template <typename E>
__device__ static inline E rd_make(typename rde<E>::R re, typename rde<E>::R im) {
  if constexpr (rde<E>::cplx) {
    E e;
    e.x = re;
    e.y = im;
    return e;
  } else {
    return re;
  }
}

// THE matrix entry A[k + D q, i + n1 j], e the entry of angle q
template <typename R>
__device__ static inline R radon_weight(int k, int i, int j, const radon_entry<R>& e, const radon_geom<R>& g) {
  const R t = (R)k - g.ct, xr = (R)i - g.cx, yr = (R)j - g.cy;
  const R p = rd_fma(xr, e.c, yr * e.s);
  const R d = rd_abs(t - p);
  if (e.rmn == (R)0) return (d < e.hi ? (R)1 : (d == e.hi ? (R)0.5 : (R)0)) * e.rmx;
  R u = (e.hi - d) * e.rmn;
  u = u < (R)0 ? (R)0 : (u > (R)1 ? (R)1 : u);
  return u * e.rmx;
}

// out = alpha (sr + i si) + beta out  (beta_zero: out is not read)
template <typename E>
__device__ static inline void rd_store(E* out, typename rde<E>::R sr, typename rde<E>::R si, typename rde<E>::R ar, typename rde<E>::R ai,
                                       typename rde<E>::R br, typename rde<E>::R bi, int beta_zero) {
  using R = typename rde<E>::R;
  R re = ar * sr, im = 0;
  if constexpr (rde<E>::cplx) {
    re = rd_fma(-ai, si, re);
    im = rd_fma(ai, sr, ar * si);
  }
  if (!beta_zero) {
    const E yv = *out;
    re = rd_fma(br, rd_re(yv), re);
    if constexpr (rde<E>::cplx) {
      re = rd_fma(-bi, rd_im(yv), re);
      im = rd_fma(br, rd_im(yv), im);
      im = rd_fma(bi, rd_re(yv), im);
    }
  }
  *out = rd_make<E>(re, im);
}

// y = alpha A x + beta y.  A wave item is (angle q, chunk of 64 detectors); items = nA * ceil(D / 64).
template <typename E>
__global__ __launch_bounds__(RD_THREADS) void radon_forward_kernel(const radon_entry<typename rde<E>::R>* __restrict__ tab,
                                                                   radon_geom<typename rde<E>::R> g, const E* __restrict__ x, E* __restrict__ y,
                                                                   typename rde<E>::R ar, typename rde<E>::R ai, typename rde<E>::R br,
                                                                   typename rde<E>::R bi, int beta_zero) {
  using R = typename rde<E>::R;
  const int lane = threadIdx.x & (RLS_WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t chunks = (g.D + RLS_WAVE - 1) / RLS_WAVE, items = chunks * g.nA;
  for (int64_t item = (int64_t)blockIdx.x * RD_WAVES + wave; item < items; item += (int64_t)gridDim.x * RD_WAVES) {
    const int q = (int)(item / chunks);
    const int k = (int)(item - (int64_t)q * chunks) * RLS_WAVE + lane;
    if (k >= g.D) continue;
    const radon_entry<R> e = tab[q];
    const bool major_i = rd_abs(e.s) >= rd_abs(e.c);  // wave-uniform
    // minor* = a + b (major index): the solution of t = xr c + yr s for the minor centred coordinate, moved to an index
    const R t = (R)k - g.ct;
    const R rmaj = (R)1 / (major_i ? e.s : e.c);
    const R b = -(major_i ? e.c : e.s) * rmaj;
    const R a = rd_fma(-(major_i ? g.cx : g.cy), b, rd_fma(t, rmaj, major_i ? g.cy : g.cx));
    const int nmaj = major_i ? g.n1 : g.n2, nmin = major_i ? g.n2 : g.n1;
    R sr = 0, si = 0;
    for (int u = 0; u < nmaj; ++u) {
      const int v0 = (int)rd_rint(rd_fma((R)u, b, a));
      if (v0 < -1 || v0 > nmin) continue;
#pragma unroll
      for (int dv = -1; dv <= 1; ++dv) {
        const int v = v0 + dv;
        if (v < 0 || v >= nmin) continue;
        const int i = major_i ? u : v, j = major_i ? v : u;
        const R w = radon_weight<R>(k, i, j, e, g);
        const E xv = x[(int64_t)i + (int64_t)g.n1 * j];
        sr = rd_fma(w, rd_re(xv), sr);
        if constexpr (rde<E>::cplx) si = rd_fma(w, rd_im(xv), si);
      }
    }
    rd_store<E>(y + ((int64_t)k + (int64_t)g.D * q), sr, si, ar, ai, br, bi, beta_zero);
  }
}

// sum over the L consecutive lanes of a group (aligned to L), complete in every lane of the group; every lane of the wave is active
template <int L, typename T>
__device__ static inline T rd_group_sum(T v) {
  static_assert(L == 1 || L == 4 || L == 16 || L == 64, "lanes per pixel");
  if constexpr (L >= 4) {
    v += rd_dpp(v, 0xB1);
    v += rd_dpp(v, 0x4E);
  }
  if constexpr (L >= 16) {
    v += rd_dpp(v, 0x141);
    v += rd_dpp(v, 0x140);
  }
  if constexpr (L == 64) {
    v = pair_sum16(v);
    v = pair_sum32(v);
  }
  return v;
}

// x = alpha A^T y + beta x.  L lanes per pixel; the trip over pixel blocks is uniform for the workgroup (the butterfly needs every lane).
template <typename E, int L>
__global__ __launch_bounds__(RD_THREADS) void radon_adjoint_kernel(const radon_entry<typename rde<E>::R>* __restrict__ tab,
                                                                   radon_geom<typename rde<E>::R> g, const E* __restrict__ y, E* __restrict__ x,
                                                                   typename rde<E>::R ar, typename rde<E>::R ai, typename rde<E>::R br,
                                                                   typename rde<E>::R bi, int beta_zero) {
  using R = typename rde<E>::R;
  constexpr int PPB = RD_THREADS / L;
  const int sub = threadIdx.x % L, ploc = threadIdx.x / L;
  const int64_t N = (int64_t)g.n1 * g.n2;
  for (int64_t p0 = (int64_t)blockIdx.x * PPB; p0 < N; p0 += (int64_t)gridDim.x * PPB) {
    const int64_t pix = p0 + ploc;
    const bool live = pix < N;
    R sr = 0, si = 0;
    if (live) {
      const int j = (int)(pix / g.n1), i = (int)(pix - (int64_t)j * g.n1);
      const R xr = (R)i - g.cx, yr = (R)j - g.cy;
      for (int q = sub; q < g.nA; q += L) {
        const radon_entry<R> e = tab[q];
        const int k0 = (int)rd_rint(rd_fma(xr, e.c, yr * e.s) + g.ct);
        if (k0 < -1 || k0 > g.D) continue;
        const E* yq = y + (int64_t)g.D * q;
#pragma unroll
        for (int dk = -1; dk <= 1; ++dk) {
          const int k = k0 + dk;
          if (k < 0 || k >= g.D) continue;
          const R w = radon_weight<R>(k, i, j, e, g);
          const E yv = yq[k];
          sr = rd_fma(w, rd_re(yv), sr);
          if constexpr (rde<E>::cplx) si = rd_fma(w, rd_im(yv), si);
        }
      }
    }
    sr = rd_group_sum<L>(sr);
    if constexpr (rde<E>::cplx) si = rd_group_sum<L>(si);
    if (live && sub == 0) rd_store<E>(x + pix, sr, si, ar, ai, br, bi, beta_zero);
  }
}

// A (M x N, column-major, leading dimension lda) = the matrix, a lane per entry
template <typename E>
__global__ __launch_bounds__(RD_THREADS) void radon_dense_kernel(const radon_entry<typename rde<E>::R>* __restrict__ tab,
                                                                 radon_geom<typename rde<E>::R> g, E* __restrict__ A, int64_t lda) {
  using R = typename rde<E>::R;
  const int64_t M = (int64_t)g.D * g.nA, total = M * g.n1 * g.n2;
  for (int64_t idx = (int64_t)blockIdx.x * RD_THREADS + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * RD_THREADS) {
    const int64_t col = idx / M, row = idx - col * M;
    const int q = (int)(row / g.D), k = (int)(row - (int64_t)q * g.D);
    const int j = (int)(col / g.n1), i = (int)(col - (int64_t)j * g.n1);
    A[row + col * lda] = rd_make<E>(radon_weight<R>(k, i, j, tab[q], g), (R)0);
  }
}

template <typename F>
static inline int32_t rd_dispatch(int32_t dtype, F&& fn) {
  if (dtype == RLS_F64 || dtype == RLS_C64) return rls_with_elem64(dtype, fn);
  return rls_with_elem(dtype, fn);
}
static inline size_t rd_elem_size(int32_t dtype) { return dtype == RLS_F32 ? 4 : dtype == RLS_C64 ? 16 : 8; }
static inline unsigned rd_grid(int64_t items, int per_block) {
  int64_t g = (items + per_block - 1) / per_block;
  if (g > RD_MAX_BLOCKS) g = RD_MAX_BLOCKS;
  if (g < 1) g = 1;
  return (unsigned)g;
}

// Lanes per pixel of the adjoint from the pixel count: few pixels need the lanes of a group to fill the chip, many pixels fill it
// alone and a group's butterfly and idle lanes (L above the angle count) only cost.  profiles/radon.txt (tools/bench_radon.py, Float32,
// every instantiation forced in turn, us per adjoint at L = 1 / 4 / 16 / 64): 64 x 64, 64 angles 36.2 / 11.4 / 4.7 / 4.0;
// 128 x 128, 128 angles 70.1 / 21.1 / 12.1 / 12.1; 256 x 256, 256 angles 139.2 / 46.5 / 79.2 / 97.0.  Nothing is measured between
// those three sizes or beyond the last: the thresholds sit at the measured pixel counts.
static int rd_pick_lanes(int64_t N) {
  if (N <= 4096) return 64;
  if (N <= 16384) return 16;
  if (N <= 65536) return 4;
  return 1;
}

}  // namespace

struct rls_radon {
  rls_ctx* ctx = nullptr;
  uint64_t ctx_id = 0;
  int32_t dtype = RLS_F32;
  int64_t n1 = 0, n2 = 0, nA = 0, D = 0, M = 0, N = 0;
  void* tab = nullptr;   // nA entries of the element's real type, device
  void* work = nullptr;  // M elements: the sinogram between the two halves of rls_radon_mul_normal
};

namespace {

static bool rd_live(const rls_radon* r) { return r && rls_ctx_alive(r->ctx, r->ctx_id); }
static int rd_lanes(const rls_radon* r) {
  const int forced = r->ctx->tune.radon_lanes;
  return forced ? forced : rd_pick_lanes(r->N);
}
template <typename R>
static radon_geom<R> rd_geom(const rls_radon* r) {
  radon_geom<R> g;
  g.n1 = (int)r->n1, g.n2 = (int)r->n2, g.D = (int)r->D, g.nA = (int)r->nA;
  g.ct = (R)((double)(r->D - 1) / 2), g.cx = (R)((double)(r->n1 - 1) / 2), g.cy = (R)((double)(r->n2 - 1) / 2);
  return g;
}

static int32_t rd_mul(rls_radon* r, bool fwd, double ar, double ai, const void* x, double br, double bi, void* y) {
  rls_ctx* ctx = r->ctx;
  const int beta_zero = br == 0.0 && bi == 0.0;
  return rd_dispatch(r->dtype, [&](auto t) -> int32_t {
    using E = typename decltype(t)::type;
    using R = typename rde<E>::R;
    const radon_geom<R> g = rd_geom<R>(r);
    const auto* tab = (const radon_entry<R>*)r->tab;
    if (fwd) {
      const int64_t items = ((r->D + RLS_WAVE - 1) / RLS_WAVE) * r->nA;
      return rls_launch<radon_forward_kernel<E>>(ctx, dim3(rd_grid(items, RD_WAVES)), dim3(RD_THREADS), 0, tab, g, (const E*)x, (E*)y, (R)ar,
                                                 (R)ai, (R)br, (R)bi, beta_zero);
    }
    return rls_with<1, 4, 16, 64>(rd_lanes(r), [&](auto l) -> int32_t {
      constexpr int L = decltype(l)::value;
      return rls_launch<radon_adjoint_kernel<E, L>>(ctx, dim3(rd_grid(r->N, RD_THREADS / L)), dim3(RD_THREADS), 0, tab, g, (const E*)x, (E*)y,
                                                    (R)ar, (R)ai, (R)br, (R)bi, beta_zero);
    });
  });
}

}  // namespace

extern "C" {

int32_t rls_radon_create(rls_ctx* ctx, int32_t dtype, int64_t n1, int64_t n2, int64_t n_angles, const double* angles_host, int64_t detectors,
                         rls_radon** out) {
  RLS_CHECK_CTX(ctx);
  if (!out) return rls_fail(ctx, RLS_E_INVALID, "radon_create: null out");
  *out = nullptr;
  const int64_t lim = (int64_t)1 << 31;
  if (dtype < RLS_F32 || dtype > RLS_C64 || n1 < 1 || n2 < 1 || n1 >= lim || n2 >= lim || n_angles < 1 || n_angles >= lim || !angles_host ||
      detectors < 0 || detectors >= lim)
    return rls_fail(ctx, RLS_E_INVALID, "radon_create: bad argument (extents, angle count >= 1; detectors >= 0; one of the four element types)");
  for (int64_t q = 0; q < n_angles; ++q)
    if (!std::isfinite(angles_host[q])) return rls_fail(ctx, RLS_E_INVALID, "radon_create: an angle is not finite");
  const int64_t N = n1 * n2;
  const int64_t D = detectors > 0 ? detectors : 2 * (int64_t)std::ceil(std::hypot((double)n1, (double)n2) / 2.0) + 1;
  if (N >= lim || D >= lim || D * n_angles >= lim) return rls_fail(ctx, RLS_E_INVALID, "radon_create: M = D n_angles and N = n1 n2 must be below 2^31");
  // the table, in double on the host, rounded once to the element's real type
  const bool dbl = dtype == RLS_F64 || dtype == RLS_C64;
  std::vector<double> td((size_t)n_angles * 8, 0.0);
  for (int64_t q = 0; q < n_angles; ++q) {
    double c = std::cos(angles_host[q]), s = std::sin(angles_host[q]);
    if (std::fmin(std::fabs(c), std::fabs(s)) <= 0x1p-40) {  // snapped onto the axis
      if (std::fabs(c) > std::fabs(s)) c = c > 0 ? 1.0 : -1.0, s = 0.0;
      else s = s > 0 ? 1.0 : -1.0, c = 0.0;
    }
    const double mx = std::fmax(std::fabs(c), std::fabs(s)), mn = std::fmin(std::fabs(c), std::fabs(s));
    double* e = &td[(size_t)q * 8];
    e[0] = c, e[1] = s, e[2] = (std::fabs(c) + std::fabs(s)) / 2, e[3] = mn > 0 ? 1.0 / mn : 0.0, e[4] = 1.0 / mx;
  }
  std::vector<float> tf(dbl ? 0 : td.size());
  for (size_t k = 0; k < tf.size(); ++k) tf[k] = (float)td[k];  // (mn > 2^-40: neither mn nor 1 / mn leaves Float32's range)
  RLS_HIP(ctx, rls_enter(ctx));
  rls_radon* r = new rls_radon();
  r->ctx = ctx;
  r->ctx_id = ctx->id;
  r->dtype = dtype;
  r->n1 = n1, r->n2 = n2, r->nA = n_angles, r->D = D, r->M = D * n_angles, r->N = N;
  const size_t tb = (size_t)n_angles * 8 * (dbl ? 8 : 4);
  hipError_t e = rls_dev_alloc(ctx, &r->tab, tb);
  if (e == hipSuccess) e = rls_dev_alloc(ctx, &r->work, (size_t)r->M * rd_elem_size(dtype));
  if (e != hipSuccess) {
    rls_radon_destroy(r);
    return rls_fail(ctx, RLS_E_WORKSPACE, "radon_create: allocation failed");
  }
  e = hipMemcpyAsync(r->tab, dbl ? (const void*)td.data() : (const void*)tf.data(), tb, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = rls_stream_wait(ctx->stream);  // (the host table goes out of scope)
  if (e != hipSuccess) {
    rls_radon_destroy(r);
    return rls_fail(ctx, (int32_t)e, "radon_create: upload failed");
  }
  *out = r;
  return 0;
}

int32_t rls_radon_destroy(rls_radon* r) {
  if (!r) return RLS_E_INVALID;
  rls_ctx* ctx = rd_live(r) ? r->ctx : nullptr;
  if (r->tab) rls_dev_free(ctx, r->tab);
  if (r->work) rls_dev_free(ctx, r->work);
  delete r;
  return 0;
}

int32_t rls_radon_info(rls_radon* r, int64_t* M, int64_t* N, int64_t* D) {
  if (!r) return RLS_E_INVALID;
  if (M) *M = r->M;
  if (N) *N = r->N;
  if (D) *D = r->D;
  return 0;
}

int32_t rls_radon_mul(rls_radon* r, int32_t op, double alpha_re, double alpha_im, const void* x, double beta_re, double beta_im, void* y) {
  if (!rd_live(r)) return RLS_E_INVALID;
  rls_ctx* ctx = r->ctx;
  if (!x || !y || x == y || op < RLS_OP_N || op > RLS_OP_C) return rls_fail(ctx, RLS_E_INVALID, "radon_mul: bad argument");
  RLS_HIP(ctx, rls_enter(ctx));
  return rd_mul(r, op == RLS_OP_N, alpha_re, alpha_im, x, beta_re, beta_im, y);
}

int32_t rls_radon_mul_normal(rls_radon* r, const void* p, void* v) {
  if (!rd_live(r)) return RLS_E_INVALID;
  rls_ctx* ctx = r->ctx;
  if (!p || !v) return rls_fail(ctx, RLS_E_INVALID, "radon_mul_normal: null pointer");
  RLS_HIP(ctx, rls_enter(ctx));
  RLS_TRY(rd_mul(r, true, 1.0, 0.0, p, 0.0, 0.0, r->work));
  return rd_mul(r, false, 1.0, 0.0, r->work, 0.0, 0.0, v);
}

int32_t rls_radon_to_dense(rls_radon* r, void* A, int64_t lda) {
  if (!rd_live(r)) return RLS_E_INVALID;
  rls_ctx* ctx = r->ctx;
  if (!A || lda < r->M) return rls_fail(ctx, RLS_E_INVALID, "radon_to_dense: null pointer or lda < M");
  RLS_HIP(ctx, rls_enter(ctx));
  return rd_dispatch(r->dtype, [&](auto t) -> int32_t {
    using E = typename decltype(t)::type;
    using R = typename rde<E>::R;
    return rls_launch<radon_dense_kernel<E>>(ctx, dim3(rd_grid(r->M * r->N, RD_THREADS)), dim3(RD_THREADS), 0, (const radon_entry<R>*)r->tab,
                                             rd_geom<R>(r), (E*)A, lda);
  });
}

int32_t rls_radon_lanes(rls_radon* r, int32_t* out) {
  if (!rd_live(r) || !out) return RLS_E_INVALID;
  *out = rd_lanes(r);
  return 0;
}

}  // extern "C"
