// Matrix-free NFFTOp: non-uniform Fourier sampling, the operator of radial and spiral MRI and of
// magnetic-particle imaging.  NFFT.jl is third-party to the reference, like the operators of fft.hip and radon.hip: the operator is
// DEFINED here in closed form,
//     y_j = sum_k x_k exp(-2 pi i k . nu_j),   k_d in {-floor(N_d / 2), ..., ceil(N_d / 2) - 1},   nu_j in [-0.5, 0.5)^d,
// no scale factor, the image column-major, and computed by the standard three steps on a grid of n_d = the smallest power of two
// >= 2 N_d points (sigma_d = n_d / N_d in [2, 4)) with the Kaiser-Bessel window of NFFT3,
//     phi(t) = sinh(b sqrt(m^2 - t^2)) / (pi sqrt(m^2 - t^2)),   b = pi (2 - 1 / sigma),   phi(+-m) = b / pi,
//     phihat(k) = I0(m sqrt(b^2 - (2 pi k / n)^2))   (the transform of phi in grid units t: the 1 / n of the periodic window's
//                                                     Fourier coefficient and the n of the unscaled transform cancel),
// at the 2 m taps u0 - m + 1 ... u0 + m, u0 = floor(n nu), periodic in u (for n < 2 m the footprint wraps onto itself: a grid point
// is then visited by several taps of one node, which is what the periodic window asks for).
//
// Forward:  embed   a lane per grid point: (x_k / phihat_1(k_1)) / phihat_2(k_2) at the centred position, zero elsewhere (one launch
//                   writes the whole grid; the divisions are products with the tables' reciprocals);
//           FFT     the handle's own rls_fft (RLS_FFT_SHIFT only), in place, through rls_fft_apply;
//           gather  a lane per node: the (2 m)^d products (w_1 w_2) G summed by one fma chain, dimension 2 outer, taps ascending.
// Adjoint:  spread  OUTPUT-driven, a lane per grid point: the host has binned the nodes by grid cell (u0) at create time -- cell ->
//                   node list, nodes in input order; the lane walks the (2 m)^d cells its value can depend on, dimension 2 outer,
//                   cell offsets ascending (u0 = l - m ... l + m - 1, periodic), nodes in list order, one fma chain.  No atomics
//                   of any kind: the same bits run to run;
//           FFT^H   in place; crop + the same two products with the (real) tables.
// The weights w_d (J d 2m reals) and the two phihat tables are computed in double on the host and rounded once to the element's real
// type; every device sum is an explicit fma chain and every product an explicit *_rn, as in fft.hip, so contraction cannot regroup.
// No kernel has a grid-stride loop: the launches cover their items exactly (grid points <= 2^26, nodes < 2^31).
#include <cmath>
#include <vector>

#include "rls_common.hpp"

namespace {

constexpr int NF_THREADS = 256;
constexpr int NF_M_MAX = 8;
constexpr size_t NF_LINE_LDS = 64 * 1024;  // fft.hip's FFT_LINE_LDS: the longest line is 8192 ComplexF32 / 4096 ComplexF64 points

template <typename E>
struct nfe;
template <>
struct nfe<float2> {
  using R = float;
  __device__ static inline float mul(float a, float b) { return __fmul_rn(a, b); }
  __device__ static inline float fma(float a, float b, float c) { return fmaf(a, b, c); }
  __device__ static inline float2 make(float re, float im) { return make_float2(re, im); }
};
template <>
struct nfe<double2> {
  using R = double;
  __device__ static inline double mul(double a, double b) { return __dmul_rn(a, b); }
  __device__ static inline double fma(double a, double b, double c) { return ::fma(a, b, c); }
  __device__ static inline double2 make(double re, double im) { return make_double2(re, im); }
};

// the geometry every kernel sees.  A signal is an image with n2 = N2 = 1 (lg2 = 0, one tap of weight 1 along dimension 2, which the
// TWO = false instantiations leave out)
struct nfft_geom {
  int N1, N2;      // image extents
  int lg1, lg2;    // grid extents 2^lg1 x 2^lg2
  int lo1, lo2;    // where the centred image starts in the centred grid: n / 2 - floor(N / 2)
  int m;           // 2 m taps per dimension
  int64_t J;
};

// grid = zero, but the centred image times the two deapodisation tables
template <typename E, bool TWO>
__global__ __launch_bounds__(NF_THREADS) void nfft_embed_kernel(nfft_geom g, const typename nfe<E>::R* __restrict__ d1,
                                                                const typename nfe<E>::R* __restrict__ d2, const E* __restrict__ x,
                                                                E* __restrict__ grid) {
  using R = typename nfe<E>::R;
  const int idx = blockIdx.x * NF_THREADS + threadIdx.x;
  if (idx >= (1 << (g.lg1 + g.lg2))) return;
  const int k1 = (idx & ((1 << g.lg1) - 1)) - g.lo1, k2 = (idx >> g.lg1) - g.lo2;
  E v = nfe<E>::make((R)0, (R)0);
  if (k1 >= 0 && k1 < g.N1 && k2 >= 0 && k2 < g.N2) {
    const E xv = x[k1 + g.N1 * k2];
    const R a = d1[k1];
    v = nfe<E>::make(nfe<E>::mul(xv.x, a), nfe<E>::mul(xv.y, a));
    if constexpr (TWO) {
      const R b = d2[k2];
      v = nfe<E>::make(nfe<E>::mul(v.x, b), nfe<E>::mul(v.y, b));
    }
  }
  grid[idx] = v;
}

// x_k = (grid at the centred position of k) times the two tables
template <typename E, bool TWO>
__global__ __launch_bounds__(NF_THREADS) void nfft_crop_kernel(nfft_geom g, const typename nfe<E>::R* __restrict__ d1,
                                                               const typename nfe<E>::R* __restrict__ d2, const E* __restrict__ grid,
                                                               E* __restrict__ x) {
  using R = typename nfe<E>::R;
  const int idx = blockIdx.x * NF_THREADS + threadIdx.x;
  if (idx >= g.N1 * g.N2) return;
  const int k2 = idx / g.N1, k1 = idx - k2 * g.N1;
  const E gv = grid[(k1 + g.lo1) + ((k2 + g.lo2) << g.lg1)];
  const R a = d1[k1];
  E v = nfe<E>::make(nfe<E>::mul(gv.x, a), nfe<E>::mul(gv.y, a));
  if constexpr (TWO) {
    const R b = d2[k2];
    v = nfe<E>::make(nfe<E>::mul(v.x, b), nfe<E>::mul(v.y, b));
  }
  x[idx] = v;
}

// y_j = sum over the taps of (w_1 w_2) G.  w[(dim 2m + t) J + j]; q0[dim J + j] = the grid index of the node's first tap
template <typename E, bool TWO>
__global__ __launch_bounds__(NF_THREADS) void nfft_gather_kernel(nfft_geom g, const typename nfe<E>::R* __restrict__ w,
                                                                 const int32_t* __restrict__ q0, const E* __restrict__ grid, E* __restrict__ y) {
  using R = typename nfe<E>::R;
  const int64_t j = (int64_t)blockIdx.x * NF_THREADS + threadIdx.x;
  if (j >= g.J) return;
  const int T = 2 * g.m, mask1 = (1 << g.lg1) - 1, mask2 = (1 << g.lg2) - 1;
  const int a1 = q0[j], a2 = TWO ? q0[g.J + j] : 0;
  R re = 0, im = 0;
  for (int t2 = 0; t2 < (TWO ? T : 1); ++t2) {
    const int p2 = (a2 + t2) & mask2;
    const R w2 = TWO ? w[(int64_t)(T + t2) * g.J + j] : (R)1;
    for (int t1 = 0; t1 < T; ++t1) {
      const int p1 = (a1 + t1) & mask1;
      R ww = w[(int64_t)t1 * g.J + j];
      if constexpr (TWO) ww = nfe<E>::mul(ww, w2);
      const E gv = grid[p1 + (p2 << g.lg1)];
      re = nfe<E>::fma(ww, gv.x, re);
      im = nfe<E>::fma(ww, gv.y, im);
    }
  }
  y[j] = nfe<E>::make(re, im);
}

// G_p = sum over the nodes whose footprint holds p of (w_1 w_2) y_j.  cell c = c1 + n1 c2 holds the nodes with u0 + n / 2 = (c1, c2),
// nodes[cs[c] ... cs[c + 1]) in input order; the node of cell c1 reaches p1 with its tap t1 = (p1 + m - 1 - c1) mod n1
template <typename E, bool TWO>
__global__ __launch_bounds__(NF_THREADS) void nfft_spread_kernel(nfft_geom g, const typename nfe<E>::R* __restrict__ w,
                                                                 const int32_t* __restrict__ cs, const int32_t* __restrict__ nodes,
                                                                 const E* __restrict__ y, E* __restrict__ grid) {
  using R = typename nfe<E>::R;
  const int idx = blockIdx.x * NF_THREADS + threadIdx.x;
  if (idx >= (1 << (g.lg1 + g.lg2))) return;
  const int T = 2 * g.m, mask1 = (1 << g.lg1) - 1, mask2 = (1 << g.lg2) - 1;
  const int p1 = idx & mask1, p2 = idx >> g.lg1;
  R re = 0, im = 0;
  for (int t2 = (TWO ? T : 1) - 1; t2 >= 0; --t2) {
    const int c2 = TWO ? ((p2 + g.m - 1 - t2) & mask2) : 0;
    for (int t1 = T - 1; t1 >= 0; --t1) {
      const int c = ((p1 + g.m - 1 - t1) & mask1) + (c2 << g.lg1);
      const int s = cs[c], e = cs[c + 1];
      for (int i = s; i < e; ++i) {
        const int64_t j = nodes[i];
        R ww = w[(int64_t)t1 * g.J + j];
        if constexpr (TWO) ww = nfe<E>::mul(ww, w[(int64_t)(T + t2) * g.J + j]);
        const E yv = y[j];
        re = nfe<E>::fma(ww, yv.x, re);
        im = nfe<E>::fma(ww, yv.y, im);
      }
    }
  }
  grid[idx] = nfe<E>::make(re, im);
}

template <typename F>
static inline int32_t nf_dispatch(int32_t dtype, F&& fn) {
  if (dtype == RLS_C64) return fn(rls_type<double2>{});
  return fn(rls_type<float2>{});
}
static inline unsigned nf_blocks(int64_t items) { return (unsigned)((items + NF_THREADS - 1) / NF_THREADS); }

// I0 by its power series (all terms positive; z <= 8 b < 45): the loop tests/nfft_ref.py restates
static double nf_i0(double z) {
  const double q = z * z / 4.0;
  double term = 1.0, s = 1.0;
  for (int k = 1; k <= 128; ++k) {
    term = term * q / (double)(k * k);
    s = s + term;
  }
  return s;
}
// (m - t)(m + t) and (b - w)(b + w): no a * b + c the host compiler could contract
static double nf_window(double t, double m, double b) {
  const double s = (m - t) * (m + t);
  if (!(s > 0.0)) return b / M_PI;
  const double r = std::sqrt(s);
  return std::sinh(b * r) / (M_PI * r);
}

}  // namespace

struct rls_nfft {
  rls_ctx* ctx = nullptr;
  uint64_t ctx_id = 0;
  int32_t dtype = RLS_C32;
  int d = 1;
  nfft_geom g{};
  int64_t Nimg = 0, points = 0;
  rls_fft* fft = nullptr;
  void* dtab = nullptr;         // N1 + N2 reals: 1 / phihat_1, 1 / phihat_2
  void* w = nullptr;            // d 2m J reals
  int32_t* q0 = nullptr;        // d J
  int32_t* cs = nullptr;        // points + 1
  int32_t* nodes = nullptr;     // J
  void* grid = nullptr;         // points elements
  void* work = nullptr;         // J elements: the samples between the two halves of rls_nfft_mul_normal
};

namespace {

static bool nf_live(const rls_nfft* h) { return h && rls_ctx_alive(h->ctx, h->ctx_id); }

static int32_t nf_forward(rls_nfft* h, const void* x, void* y) {
  rls_ctx* ctx = h->ctx;
  RLS_TRY(nf_dispatch(h->dtype, [&](auto t) -> int32_t {
    using E = typename decltype(t)::type;
    using R = typename nfe<E>::R;
    return with_bool(h->d == 2, [&](auto two) -> int32_t {
      return rls_launch<nfft_embed_kernel<E, decltype(two)::value>>(ctx, dim3(nf_blocks(h->points)), dim3(NF_THREADS), 0, h->g, (const R*)h->dtab,
                                                                    (const R*)h->dtab + h->g.N1, (const E*)x, (E*)h->grid);
    });
  }));
  RLS_TRY(rls_fft_apply(h->fft, 0, h->grid, h->grid));
  return nf_dispatch(h->dtype, [&](auto t) -> int32_t {
    using E = typename decltype(t)::type;
    using R = typename nfe<E>::R;
    return with_bool(h->d == 2, [&](auto two) -> int32_t {
      return rls_launch<nfft_gather_kernel<E, decltype(two)::value>>(ctx, dim3(nf_blocks(h->g.J)), dim3(NF_THREADS), 0, h->g, (const R*)h->w,
                                                                     (const int32_t*)h->q0, (const E*)h->grid, (E*)y);
    });
  });
}

static int32_t nf_adjoint(rls_nfft* h, const void* y, void* x) {
  rls_ctx* ctx = h->ctx;
  RLS_TRY(nf_dispatch(h->dtype, [&](auto t) -> int32_t {
    using E = typename decltype(t)::type;
    using R = typename nfe<E>::R;
    return with_bool(h->d == 2, [&](auto two) -> int32_t {
      return rls_launch<nfft_spread_kernel<E, decltype(two)::value>>(ctx, dim3(nf_blocks(h->points)), dim3(NF_THREADS), 0, h->g, (const R*)h->w,
                                                                     (const int32_t*)h->cs, (const int32_t*)h->nodes, (const E*)y, (E*)h->grid);
    });
  }));
  RLS_TRY(rls_fft_apply(h->fft, 1, h->grid, h->grid));
  return nf_dispatch(h->dtype, [&](auto t) -> int32_t {
    using E = typename decltype(t)::type;
    using R = typename nfe<E>::R;
    return with_bool(h->d == 2, [&](auto two) -> int32_t {
      return rls_launch<nfft_crop_kernel<E, decltype(two)::value>>(ctx, dim3(nf_blocks(h->Nimg)), dim3(NF_THREADS), 0, h->g, (const R*)h->dtab,
                                                                   (const R*)h->dtab + h->g.N1, (const E*)h->grid, (E*)x);
    });
  });
}

}  // namespace

extern "C" {

int32_t rls_nfft_create(rls_ctx* ctx, int32_t dtype, int32_t ndims, const int64_t* shape, int64_t J, const double* nodes_host, int32_t m,
                        rls_nfft** out) {
  RLS_CHECK_CTX(ctx);
  if (!out) return rls_fail(ctx, RLS_E_INVALID, "nfft_create: null out");
  *out = nullptr;
  if ((dtype != RLS_C32 && dtype != RLS_C64) || ndims < 1 || !shape || !nodes_host)
    return rls_fail(ctx, RLS_E_INVALID, "nfft_create: bad argument (complex element types only)");
  if (J < 1 || J >= ((int64_t)1 << 31)) return rls_fail(ctx, RLS_E_INVALID, "nfft_create: 1 <= J < 2^31 nodes");
  if (m < 1 || m > NF_M_MAX) return rls_fail(ctx, RLS_E_UNSUPPORTED, "nfft_create: m is an integer in 1 ... 8");
  const int64_t max_line = (int64_t)(NF_LINE_LDS / (dtype == RLS_C64 ? 16 : 8));
  int64_t N[2] = {1, 1}, n[2] = {1, 1};
  int lg[2] = {0, 0}, d = 0;
  for (int k = 0; k < ndims; ++k) {
    if (shape[k] < 1) return rls_fail(ctx, RLS_E_INVALID, "nfft_create: extents must be positive");
    if (shape[k] == 1) continue;  // unit dimensions are dropped
    if (d == 2) return rls_fail(ctx, RLS_E_UNSUPPORTED, "nfft_create: 1-D and 2-D shapes only");
    if (2 * shape[k] > max_line)
      return rls_fail(ctx, RLS_E_UNSUPPORTED, "nfft_create: the grid line 2 N_d is longer than 8192 (ComplexF32) / 4096 (ComplexF64) points");
    N[d++] = shape[k];
  }
  if (d == 0) d = 1;  // every extent is one: a signal of one point
  for (int k = 0; k < d; ++k) {
    n[k] = 2;
    lg[k] = 1;
    while (n[k] < 2 * N[k]) n[k] *= 2, ++lg[k];
  }
  const int64_t points = n[0] * n[1];
  for (int64_t i = 0; i < (int64_t)d * J; ++i)
    if (!(nodes_host[i] >= -0.5 && nodes_host[i] < 0.5))  // (a NaN fails both)
      return rls_fail(ctx, RLS_E_INVALID, "nfft_create: a node lies outside [-0.5, 0.5) or is not a number");
  // ---- the tables, in double on the host -------------------------------------------------------------------------------------------
  const int T = 2 * m;
  std::vector<double> dt((size_t)(N[0] + N[1]), 1.0), wt((size_t)d * T * J);
  std::vector<int32_t> q0((size_t)d * J), cell((size_t)J, 0), cs((size_t)points + 1, 0), order((size_t)J);
  for (int k = 0; k < d; ++k) {
    const double b = M_PI * (2.0 - (double)N[k] / (double)n[k]);
    for (int64_t i = 0; i < N[k]; ++i) {
      const double om = 2.0 * M_PI * (double)(i - N[k] / 2) / (double)n[k];
      dt[(size_t)(k ? N[0] : 0) + i] = 1.0 / nf_i0((double)m * std::sqrt((b - om) * (b + om)));
    }
    for (int64_t j = 0; j < J; ++j) {
      const double v = (double)n[k] * nodes_host[(int64_t)k * J + j];  // exact: n is a power of two
      const double u0 = std::floor(v);                                 // in [-n / 2, n / 2)
      const double first = u0 - (double)m + 1.0;
      for (int t = 0; t < T; ++t) wt[((size_t)k * T + t) * J + j] = nf_window(v - (first + (double)t), (double)m, b);
      const int64_t c = (int64_t)u0 + n[k] / 2;
      q0[(size_t)k * J + j] = (int32_t)((((c - m + 1) % n[k]) + n[k]) % n[k]);
      cell[(size_t)j] += (int32_t)(k ? c * n[0] : c);
    }
  }
  // cell -> node list by a stable counting sort: nodes in input order within a cell
  for (int64_t j = 0; j < J; ++j) ++cs[(size_t)cell[(size_t)j] + 1];
  for (int64_t c = 0; c < points; ++c) cs[(size_t)c + 1] += cs[(size_t)c];
  {
    std::vector<int32_t> at(cs.begin(), cs.end() - 1);
    for (int64_t j = 0; j < J; ++j) order[(size_t)at[(size_t)cell[(size_t)j]]++] = (int32_t)j;
  }
  const bool dbl = dtype == RLS_C64;
  const size_t rs = dbl ? 8 : 4, es = 2 * rs;
  std::vector<float> dtf(dbl ? 0 : dt.size()), wtf(dbl ? 0 : wt.size());
  for (size_t i = 0; i < dtf.size(); ++i) dtf[i] = (float)dt[i];
  for (size_t i = 0; i < wtf.size(); ++i) wtf[i] = (float)wt[i];
  // ---- the handle ------------------------------------------------------------------------------------------------------------------
  RLS_HIP(ctx, rls_enter(ctx));
  rls_nfft* h = new rls_nfft();
  h->ctx = ctx;
  h->ctx_id = ctx->id;
  h->dtype = dtype;
  h->d = d;
  h->g.N1 = (int)N[0], h->g.N2 = (int)N[1], h->g.lg1 = lg[0], h->g.lg2 = lg[1];
  h->g.lo1 = (int)(n[0] / 2 - N[0] / 2), h->g.lo2 = d == 2 ? (int)(n[1] / 2 - N[1] / 2) : 0;
  h->g.m = m, h->g.J = J;
  h->Nimg = N[0] * N[1], h->points = points;
  const int64_t gshape[2] = {n[0], n[1]};
  int32_t st = rls_fft_create(ctx, dtype, d, gshape, RLS_FFT_SHIFT, &h->fft);
  if (st != 0) {
    rls_nfft_destroy(h);
    return st;
  }
  hipError_t e = rls_dev_alloc(ctx, &h->dtab, dt.size() * rs);
  if (e == hipSuccess) e = rls_dev_alloc(ctx, &h->w, wt.size() * rs);
  if (e == hipSuccess) e = rls_dev_alloc(ctx, (void**)&h->q0, q0.size() * 4);
  if (e == hipSuccess) e = rls_dev_alloc(ctx, (void**)&h->cs, cs.size() * 4);
  if (e == hipSuccess) e = rls_dev_alloc(ctx, (void**)&h->nodes, order.size() * 4);
  if (e == hipSuccess) e = rls_dev_alloc(ctx, &h->grid, (size_t)points * es);
  if (e == hipSuccess) e = rls_dev_alloc(ctx, &h->work, (size_t)J * es);
  if (e != hipSuccess) {
    rls_nfft_destroy(h);
    return rls_fail(ctx, RLS_E_WORKSPACE, "nfft_create: allocation failed (the grid and the tables must fit)");
  }
  e = hipMemcpyAsync(h->dtab, dbl ? (const void*)dt.data() : (const void*)dtf.data(), dt.size() * rs, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(h->w, dbl ? (const void*)wt.data() : (const void*)wtf.data(), wt.size() * rs, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(h->q0, q0.data(), q0.size() * 4, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(h->cs, cs.data(), cs.size() * 4, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(h->nodes, order.data(), order.size() * 4, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = rls_stream_wait(ctx->stream);  // (the host tables go out of scope)
  if (e != hipSuccess) {
    rls_nfft_destroy(h);
    return rls_fail(ctx, (int32_t)e, "nfft_create: upload failed");
  }
  *out = h;
  return 0;
}

int32_t rls_nfft_destroy(rls_nfft* h) {
  if (!h) return RLS_E_INVALID;
  rls_ctx* ctx = nf_live(h) ? h->ctx : nullptr;
  if (h->fft) rls_fft_destroy(h->fft);
  for (void* p : {h->dtab, h->w, (void*)h->q0, (void*)h->cs, (void*)h->nodes, h->grid, h->work})
    if (p) rls_dev_free(ctx, p);
  delete h;
  return 0;
}

int32_t rls_nfft_info(rls_nfft* h, int64_t* M, int64_t* N, int64_t* grid_points) {
  if (!h) return RLS_E_INVALID;
  if (M) *M = h->g.J;
  if (N) *N = h->Nimg;
  if (grid_points) *grid_points = h->points;
  return 0;
}

int32_t rls_nfft_mul(rls_nfft* h, int32_t op, const void* x, void* y) {
  if (!nf_live(h)) return RLS_E_INVALID;
  rls_ctx* ctx = h->ctx;
  if (!x || !y || x == y) return rls_fail(ctx, RLS_E_INVALID, "nfft_mul: bad argument");
  if (op == RLS_OP_T) return rls_fail(ctx, RLS_E_UNSUPPORTED, "nfft_mul: the product and its adjoint only (RLS_OP_N, RLS_OP_C)");
  if (op != RLS_OP_N && op != RLS_OP_C) return rls_fail(ctx, RLS_E_INVALID, "nfft_mul: bad op");
  RLS_HIP(ctx, rls_enter(ctx));
  return op == RLS_OP_N ? nf_forward(h, x, y) : nf_adjoint(h, x, y);
}

int32_t rls_nfft_mul_normal(rls_nfft* h, const void* p, void* v) {
  if (!nf_live(h)) return RLS_E_INVALID;
  rls_ctx* ctx = h->ctx;
  if (!p || !v) return rls_fail(ctx, RLS_E_INVALID, "nfft_mul_normal: null pointer");
  RLS_HIP(ctx, rls_enter(ctx));
  RLS_TRY(nf_forward(h, p, h->work));
  return nf_adjoint(h, h->work, v);
}

}  // extern "C"
