// Float64 / ComplexF64 device plans for CGNR and FISTA (rls_cgnr_*_d, rls_fista_*_d): the streaming pipeline of the Float32 side
// for double-precision element types.  Every scalar of the solve (alpha, beta, zeta, theta, the residual norms, `iteration`, `done`)
// lives in a device record; a step call enqueues plain stream launches and nothing comes back to the host before a status read.
//
// Per iteration, matrix-free:  t = A p (+ ||t||^2 as per-workgroup partials)  ->  v = A^H t  ->  one update kernel
// (FISTA: one elementwise kernel for the extrapolated point ahead of them: four launches).  Gram mode: v = AHA p -> update.
//   * dp_gemv_n_kernel: A column-major, 16-byte loads, G lanes along the rows and 64 / G column slots per wave, 8 waves per
//     workgroup striding the columns, 8 independent loads in flight per lane; the column slots are folded with a fixed butterfly,
//     the waves through LDS in wave order.  G shrinks (64 -> 32 -> 16) until the grid covers the chip.
//   * dp_gemv_t_kernel: columns are contiguous; one wave owns CB columns at a time and shares every load of t between them;
//     Float64 sums per lane in row order, then the fixed wave butterfly.  The column blocks are walked from the LAST one down:
//     the product starts on what t = A p has just left in the Infinity Cache (the Float32 two-GEMV path does the same).
//   * the update kernels are one workgroup of 1024 threads: the vectors are N long (KiB, against MiB of A), and the three
//     reductions of an iteration then need no second launch.  Every thread owns the same indices in every pass.
// All reductions are fixed-order: results are bit-identical run to run.  No kernel here uses scratch.
#include "rls_common.hpp"
#include "plan_buffers.hpp"

namespace {

template <typename D>
struct dl;
template <>
struct dl<double> {
  static constexpr bool cplx = false;
  __device__ static inline double zero() { return 0.0; }
  __device__ static inline double make(double re, double) { return re; }
  __device__ static inline double re(double a) { return a; }
  __device__ static inline double im(double) { return 0.0; }
  __device__ static inline double fma(double a, double b, double c) { return ::fma(a, b, c); }  // a b + c
  __device__ static inline double add(double a, double b) { return a + b; }
  __device__ static inline double sub(double a, double b) { return a - b; }
  __device__ static inline double scale(double s, double a) { return s * a; }
  __device__ static inline double abs2(double a) { return a * a; }
  __device__ static inline double absv(double a) { return fabs(a); }
  __device__ static inline double shfl_xor(double a, int off) { return __shfl_xor(a, off, 64); }
};
template <>
struct dl<double2> {
  static constexpr bool cplx = true;
  __device__ static inline double2 zero() { return make_double2(0.0, 0.0); }
  __device__ static inline double2 make(double re, double im) { return make_double2(re, im); }
  __device__ static inline double re(double2 a) { return a.x; }
  __device__ static inline double im(double2 a) { return a.y; }
  __device__ static inline double2 fma(double2 a, double2 b, double2 c) {
    double re = ::fma(a.x, b.x, c.x), im = ::fma(a.x, b.y, c.y);
    re = ::fma(-a.y, b.y, re);
    im = ::fma(a.y, b.x, im);
    return make_double2(re, im);
  }
  __device__ static inline double2 add(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
  __device__ static inline double2 sub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
  __device__ static inline double2 scale(double s, double2 a) { return make_double2(s * a.x, s * a.y); }
  __device__ static inline double abs2(double2 a) { return ::fma(a.x, a.x, a.y * a.y); }
  __device__ static inline double absv(double2 a) { return hypot(a.x, a.y); }
  __device__ static inline double2 shfl_xor(double2 a, int off) { return make_double2(__shfl_xor(a.x, off, 64), __shfl_xor(a.y, off, 64)); }
};

// V consecutive elements of one column in one load (16 bytes: one double2, or two doubles)
template <typename D, int V>
struct dpack {
  D e[V];
};
template <typename D, int V>
__device__ static inline dpack<D, V> dp_load(const D* p) {
  dpack<D, V> r;
  if constexpr (V == 2) {
    static_assert(!dl<D>::cplx, "two elements per load: Float64 only");
    const double2 q = *reinterpret_cast<const double2*>(p);
    r.e[0] = q.x;
    r.e[1] = q.y;
  } else {
    r.e[0] = *p;
  }
  return r;
}

// device-resident scalars of a solve
struct dcg_rec {
  double rr, z0, zeta, alpha_re, alpha_im, beta_re, beta_im, residual, lambda, rel_tol;
  int iteration, max_iter, done, pad;
};
struct dfi_rec {
  double norm_x0, res_norm, rel_res_norm, rho, theta, theta_old, rel_tol, thr;  // thr = rho lambda
  long long l21_slices;
  int iteration, max_iter, done, restart, reg_kind, proj_kind;
};

constexpr int GN_WAVES = 8, GN_U = 8;  // dp_gemv_n_kernel: waves per workgroup, loads in flight per lane
constexpr int GT_WAVES = 4;            // dp_gemv_t_kernel: waves per workgroup
constexpr int UPD_T = 1024;            // the single-workgroup update / init kernels

// y = A x and part[workgroup] = sum |y[rows of this workgroup]|^2.  `done` (nullable): the launch is a no-op when *done != 0.
template <typename D, int V, int G>
__global__ __launch_bounds__(GN_WAVES * 64) void dp_gemv_n_kernel(const D* __restrict__ A, int64_t lda, const D* __restrict__ x, D* __restrict__ y,
                                                                  int64_t M, int64_t N, double* __restrict__ part, const int* __restrict__ done) {
  if (done && *done) return;
  constexpr int CS = 64 / G, R = G * V;  // column slots per wave, rows per workgroup
  __shared__ D sm[GN_WAVES][R];
  __shared__ double red[16];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int g = lane % G, c = lane / G;
  const int64_t row = (int64_t)blockIdx.x * R + (int64_t)g * V;
  const D* a = A + row;
  const bool live = row < M;  // lanes past the last row load nothing (they still take part in the butterfly and the barrier below)
  D acc[V];
#pragma unroll
  for (int k = 0; k < V; ++k) acc[k] = dl<D>::zero();
  constexpr int64_t step = (int64_t)GN_WAVES * CS;
  int64_t j = live ? (int64_t)w * CS + c : N;
  for (; j + step * (GN_U - 1) < N; j += step * GN_U) {
    dpack<D, V> av[GN_U];
    D xv[GN_U];
#pragma unroll
    for (int u = 0; u < GN_U; ++u) {
      av[u] = dp_load<D, V>(a + (j + u * step) * lda);
      xv[u] = x[j + u * step];
    }
#pragma unroll
    for (int u = 0; u < GN_U; ++u)
#pragma unroll
      for (int k = 0; k < V; ++k) acc[k] = dl<D>::fma(av[u].e[k], xv[u], acc[k]);
  }
  for (; j < N; j += step) {
    const dpack<D, V> av = dp_load<D, V>(a + j * lda);
    const D xv = x[j];
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = dl<D>::fma(av.e[k], xv, acc[k]);
  }
#pragma unroll
  for (int off = G; off < 64; off <<= 1)
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = dl<D>::add(acc[k], dl<D>::shfl_xor(acc[k], off));
  if (c == 0) {
#pragma unroll
    for (int k = 0; k < V; ++k) sm[w][g * V + k] = acc[k];
  }
  __syncthreads();
  double q = 0.0;
  if ((int)threadIdx.x < R) {
    D s = sm[0][threadIdx.x];
#pragma unroll
    for (int ww = 1; ww < GN_WAVES; ++ww) s = dl<D>::add(s, sm[ww][threadIdx.x]);
    const int64_t r = (int64_t)blockIdx.x * R + threadIdx.x;
    if (r < M) {
      y[r] = s;
      q = dl<D>::abs2(s);
    }
  }
  q = block_sum_n<GN_WAVES>(q, red);
  if (threadIdx.x == 0) part[blockIdx.x] = q;
}

// v = A^H t: a wave owns CB columns, workgroup b of the grid takes column block (gridDim.x - 1 - b)
template <typename D, int V, int CB>
__global__ __launch_bounds__(GT_WAVES * 64) void dp_gemv_t_kernel(const D* __restrict__ A, int64_t lda, const D* __restrict__ t, D* __restrict__ v,
                                                                  int64_t M, int64_t N, const int* __restrict__ done) {
  if (done && *done) return;
  constexpr int U = 8 / CB;
  constexpr int64_t chunk = 64 * V;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t blk = (int64_t)gridDim.x - 1 - blockIdx.x;
  const int64_t col0 = (blk * GT_WAVES + w) * CB;
  if (col0 >= N) return;  // (no workgroup barrier in this kernel)
  const D* a[CB];
#pragma unroll
  for (int cc = 0; cc < CB; ++cc) a[cc] = A + (col0 + cc < N ? col0 + cc : col0) * lda;  // columns past N: a duplicate, never stored
  double re[CB], im[CB];
#pragma unroll
  for (int cc = 0; cc < CB; ++cc) re[cc] = im[cc] = 0.0;
  const int64_t l0 = (int64_t)lane * V;
  int64_t ib = 0;
  for (; ib + U * chunk <= M; ib += U * chunk) {
    dpack<D, V> tv[U], av[U][CB];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = ib + u * chunk + l0;
      tv[u] = dp_load<D, V>(t + i);
#pragma unroll
      for (int cc = 0; cc < CB; ++cc) av[u][cc] = dp_load<D, V>(a[cc] + i);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int cc = 0; cc < CB; ++cc)
#pragma unroll
        for (int k = 0; k < V; ++k) {  // conj(a) t
          const D p = av[u][cc].e[k], q = tv[u].e[k];
          re[cc] = ::fma(dl<D>::re(p), dl<D>::re(q), re[cc]);
          if constexpr (dl<D>::cplx) {
            re[cc] = ::fma(dl<D>::im(p), dl<D>::im(q), re[cc]);
            im[cc] = ::fma(dl<D>::re(p), dl<D>::im(q), im[cc]);
            im[cc] = ::fma(-dl<D>::im(p), dl<D>::re(q), im[cc]);
          }
        }
  }
  for (; ib < M; ib += chunk) {
    const int64_t i = ib + l0;
    if (i < M) {  // (V == 2 is chosen for even M only: i + 1 < M as well)
      const dpack<D, V> tv = dp_load<D, V>(t + i);
#pragma unroll
      for (int cc = 0; cc < CB; ++cc) {
        const dpack<D, V> av = dp_load<D, V>(a[cc] + i);
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const D p = av.e[k], q = tv.e[k];
          re[cc] = ::fma(dl<D>::re(p), dl<D>::re(q), re[cc]);
          if constexpr (dl<D>::cplx) {
            re[cc] = ::fma(dl<D>::im(p), dl<D>::im(q), re[cc]);
            im[cc] = ::fma(dl<D>::re(p), dl<D>::im(q), im[cc]);
            im[cc] = ::fma(-dl<D>::im(p), dl<D>::re(q), im[cc]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int cc = 0; cc < CB; ++cc) {
    re[cc] = wave_sum(re[cc]);
    if constexpr (dl<D>::cplx) im[cc] = wave_sum(im[cc]);
    if (lane == 0 && col0 + cc < N) v[col0 + cc] = dl<D>::make(re[cc], im[cc]);
  }
}

// ---- CGNR -----------------------------------------------------------------------------------------------------------------------
// init! behind r = A^H b (src/CGNR.jl:107-130): x = 0, p = r, v = 0, z0 = ||r||, the record
template <typename D>
__global__ __launch_bounds__(UPD_T) void dp_cgnr_init_kernel(D* __restrict__ x, const D* __restrict__ r, D* __restrict__ p, D* __restrict__ v, int64_t N,
                                                             double lambda, double rel_tol, int max_iter, dcg_rec* __restrict__ rec) {
  __shared__ double sm[16];
  double rr = 0.0;
  for (int64_t i = threadIdx.x; i < N; i += UPD_T) {
    const D ri = r[i];
    rr += dl<D>::abs2(ri);
    x[i] = dl<D>::zero();
    p[i] = ri;
    v[i] = dl<D>::zero();
  }
  rr = block_sum_n<UPD_T / 64>(rr, sm);
  if (threadIdx.x == 0) {
    const double z0 = sqrt(rr);
    rec->rr = rr;
    rec->z0 = z0;
    rec->zeta = 0.0;
    rec->alpha_re = rec->alpha_im = rec->beta_re = rec->beta_im = 0.0;
    rec->residual = z0;
    rec->lambda = lambda;
    rec->rel_tol = rel_tol;
    rec->iteration = 0;
    rec->max_iter = max_iter;
    rec->done = (z0 / z0 <= rel_tol) || 0 >= max_iter;  // converged(): 0 / 0 = NaN compares false (src/CGNR.jl:181-185)
    rec->pad = 0;
  }
}

// src/CGNR.jl:153-176 behind v = AHA p.  GRAM: alpha's denominator is <p, v>; otherwise ||A p||^2 from the partials of t = A p.
template <typename D, bool GRAM>
__global__ __launch_bounds__(UPD_T) void dp_cgnr_update_kernel(D* __restrict__ x, D* __restrict__ r, D* __restrict__ p, const D* __restrict__ v, int64_t N,
                                                               const double* __restrict__ part, int npart, dcg_rec* __restrict__ rec) {
  __shared__ double sm[48];
  if (rec->done) return;
  const double lam = rec->lambda, zeta = rec->rr, z0 = rec->z0, rel_tol = rec->rel_tol;
  const int iteration = rec->iteration, max_iter = rec->max_iter;
  double dr = 0.0, di = 0.0, pp = 0.0;
  if constexpr (GRAM) {
    for (int64_t i = threadIdx.x; i < N; i += UPD_T) {  // conj(p) v
      const D pi = p[i], vi = v[i];
      dr = ::fma(dl<D>::re(pi), dl<D>::re(vi), dr);
      if constexpr (dl<D>::cplx) {
        dr = ::fma(dl<D>::im(pi), dl<D>::im(vi), dr);
        di = ::fma(dl<D>::re(pi), dl<D>::im(vi), di);
        di = ::fma(-dl<D>::im(pi), dl<D>::re(vi), di);
      }
    }
  } else {
    for (int i = threadIdx.x; i < npart; i += UPD_T) dr += part[i];
  }
  if (lam > 0.0)
    for (int64_t i = threadIdx.x; i < N; i += UPD_T) pp += dl<D>::abs2(p[i]);
  block_sum3_n<UPD_T / 64>(dr, di, pp, sm);
  if (lam > 0.0) dr += lam * pp;  // :158-160
  double are, aim;
  if (dl<D>::cplx && GRAM) {
    const dcomplex al = dc_div(dcomplex{zeta, 0.0}, dcomplex{dr, di});
    are = al.re;
    aim = al.im;
  } else {
    are = zeta / dr;
    aim = 0.0;
  }
  const D alpha = dl<D>::make(are, aim), nalpha = dl<D>::make(-are, -aim), nlalpha = dl<D>::make(-lam * are, -lam * aim);
  double rr = 0.0;
  for (int64_t i = threadIdx.x; i < N; i += UPD_T) {
    const D pi = p[i];
    x[i] = dl<D>::fma(alpha, pi, x[i]);            // :163
    D ri = dl<D>::fma(nalpha, v[i], r[i]);         // :165
    if (lam > 0.0) ri = dl<D>::fma(nlalpha, pi, ri);  // :168
    r[i] = ri;
    rr += dl<D>::abs2(ri);
  }
  rr = block_sum_n<UPD_T / 64>(rr, sm);
  const double beta = rr / zeta;  // :171
  for (int64_t i = threadIdx.x; i < N; i += UPD_T) p[i] = dl<D>::add(dl<D>::scale(beta, p[i]), r[i]);  // :173-174
  if (threadIdx.x == 0) {
    const double res = sqrt(rr);
    rec->zeta = zeta;
    rec->rr = rr;
    rec->alpha_re = are;
    rec->alpha_im = aim;
    rec->beta_re = beta;
    rec->beta_im = 0.0;
    rec->residual = res;
    rec->iteration = iteration + 1;
    rec->done = (res / z0 <= rel_tol) || iteration + 1 >= max_iter;
  }
}

// ---- FISTA ----------------------------------------------------------------------------------------------------------------------
// init! behind x0 = A^H b (src/FISTA.jl:110-129): x = xold = 0, res = Inf, ||x0||, the record.  reg_kind etc. come from set_reg_d.
template <typename D>
__global__ __launch_bounds__(UPD_T) void dp_fista_init_kernel(D* __restrict__ b0, D* __restrict__ b1, const D* __restrict__ x0, D* __restrict__ res, int64_t N,
                                                              dfi_rec init, dfi_rec* __restrict__ rec) {
  __shared__ double sm[16];
  double nn = 0.0;
  for (int64_t i = threadIdx.x; i < N; i += UPD_T) {
    nn += dl<D>::abs2(x0[i]);
    b0[i] = dl<D>::zero();
    b1[i] = dl<D>::zero();
    res[i] = dl<D>::make(HUGE_VAL, 0.0);
  }
  nn = block_sum_n<UPD_T / 64>(nn, sm);
  if (threadIdx.x == 0) {
    init.norm_x0 = sqrt(nn);
    init.res_norm = init.rel_res_norm = HUGE_VAL;
    init.theta_old = init.theta;
    init.iteration = 0;
    init.done = (init.rel_res_norm < init.rel_tol) || 0 >= init.max_iter;
    *rec = init;
  }
}

// the extrapolated point, written over x_{k-2} (the reference's pointer swap, src/FISTA.jl:144-148): y = c1 y + c2 xprev
template <typename D>
__global__ void dp_fista_extrapolate_kernel(D* __restrict__ y, const D* __restrict__ xprev, int64_t N, const dfi_rec* __restrict__ rec) {
  if (rec->done) return;
  const double th = rec->theta, tho = rec->theta_old;
  const double c1 = (1.0 - tho) / th, c2 = (tho - 1.0) / th + 1.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x)
    y[i] = dl<D>::add(dl<D>::scale(c1, y[i]), dl<D>::scale(c2, xprev[i]));
}

// src/FISTA.jl:153-185 behind res = AHA y: res -= x0, x = y - rho res, ||res||, prox, projection, gradient restart, theta, done.
// x holds y on entry and the new iterate on exit.
template <typename D>
__global__ __launch_bounds__(UPD_T) void dp_fista_update_kernel(D* __restrict__ x, const D* __restrict__ xold, const D* __restrict__ x0, D* __restrict__ res,
                                                                int64_t N, dfi_rec* __restrict__ rec) {
  __shared__ double sm[48];
  if (rec->done) return;
  const double rho = rec->rho, thr = rec->thr, norm_x0 = rec->norm_x0, rel_tol = rec->rel_tol;
  double theta = rec->theta;
  const int kind = rec->reg_kind, proj = rec->proj_kind, restart = rec->restart, iteration = rec->iteration, max_iter = rec->max_iter;
  const long long slices = rec->l21_slices;
  const bool late = kind == RLS_REG_L21;  // the group norms need every element of the gradient step first
  double nn = 0.0, dd = 0.0, zz = 0.0;
  for (int64_t i = threadIdx.x; i < N; i += UPD_T) {
    const D ri = dl<D>::sub(res[i], x0[i]);                              // :153
    res[i] = ri;
    nn += dl<D>::abs2(ri);
    D g = dl<D>::sub(x[i], dl<D>::scale(rho, ri));                       // :154
    if (!late) {
      g = dp_proj_elem(dp_prox_elem(g, kind, thr), proj);                // :164-168
      if (restart) {
        const D d = dl<D>::sub(g, xold[i]);                              // real(dot(res, x - xold))   :172
        dd = ::fma(dl<D>::re(ri), dl<D>::re(d), dd);
        if constexpr (dl<D>::cplx) dd = ::fma(dl<D>::im(ri), dl<D>::im(d), dd);
      }
    }
    x[i] = g;
  }
  if (late) {
    __syncthreads();
    const int64_t slen = N / slices;
    for (int64_t i = threadIdx.x; i < slen; i += UPD_T) {  // ProxL21.jl:30-35, a thread per group (as d_l21_kernel)
      double s2 = 0.0;
      for (int64_t k = i; k < N; k += slen) s2 += dl<D>::abs2(x[k]);
      const double gn = sqrt(s2), q = (gn - thr) / gn;
      const double fac = (q != q) ? q : fmax(q, 0.0);
      for (int64_t k = i; k < N; k += slen) x[k] = dl<D>::scale(fac, x[k]);
    }
    __syncthreads();
    for (int64_t i = threadIdx.x; i < N; i += UPD_T) {
      const D g = dp_proj_elem(x[i], proj);
      x[i] = g;
      if (restart) {
        const D ri = res[i], d = dl<D>::sub(g, xold[i]);
        dd = ::fma(dl<D>::re(ri), dl<D>::re(d), dd);
        if constexpr (dl<D>::cplx) dd = ::fma(dl<D>::im(ri), dl<D>::im(d), dd);
      }
    }
  }
  block_sum3_n<UPD_T / 64>(nn, dd, zz, sm);
  if (threadIdx.x == 0) {
    const double rn = sqrt(nn), rel = rn / norm_x0;                       // :156
    if (restart && dd > 0.0) theta = 1.0;                                 // :172-175
    rec->res_norm = rn;
    rec->rel_res_norm = rel;
    rec->theta_old = theta;                                               // :178-180
    rec->theta = (1.0 + sqrt(1.0 + 4.0 * theta * theta)) / 2.0;
    rec->iteration = iteration + 1;
    rec->done = (rel < rel_tol) || iteration + 1 >= max_iter;             // :183-185
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
static inline bool dp_dtype_ok(int32_t dtype) { return dtype == RLS_F64 || dtype == RLS_C64; }
static inline size_t dp_elem(int32_t dtype) { return dtype == RLS_C64 ? 16 : 8; }
static inline bool dp_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// The owner of a plan's blocks (plan_buffers.hpp) on `ctx`'s pool; a block freed after that context is gone goes back through the
// synchronous hipFree (rls_dev_free with a null context).
static plan_buffers dp_memory(rls_ctx* ctx) {
  const uint64_t id = ctx->id;
  return plan_buffers([ctx](void** p, size_t bytes) { return (int)rls_dev_alloc(ctx, p, bytes); },
                      [ctx, id](void* p) { (void)rls_dev_free(rls_ctx_alive(ctx, id) ? ctx : nullptr, p); },
                      [](void** p, size_t bytes) { return (int)rls_pinned_alloc(p, bytes); }, [](void* p) { rls_pinned_free(p); },
                      [ctx](void* p, size_t bytes) { return (int)hipMemsetAsync(p, 0, bytes, ctx->stream); });
}

// what both plans share: the operands, the products' scratch and the launch geometry
struct dp_base {
  plan_buffers mem;  // t, part, and the plan's record with its pinned mirror
  rls_ctx* ctx = nullptr;
  uint64_t ctx_id = 0;
  int32_t dtype = 0;
  int64_t M = 0, N = 0, lda = 0, ldg = 0;
  const void *A = nullptr, *G = nullptr;
  void* t = nullptr;       // A p (M elements), matrix-free iterations only
  double* part = nullptr;  // per-workgroup ||t||^2 partials of dp_gemv_n_kernel
  int npart = 0;           // ... of the iteration's product
  bool initialised = false;
};

static int dp_gn_lanes(int64_t M, int V) {  // lanes along the rows: the widest group that still gives the chip a workgroup per CU
  for (int G = 64; G > 16; G >>= 1)
    if ((M + (int64_t)G * V - 1) / ((int64_t)G * V) >= 256) return G;
  return 16;
}
static int64_t dp_gn_grid(int64_t M, int V) {
  const int64_t R = (int64_t)dp_gn_lanes(M, V) * V;
  return (M + R - 1) / R;
}
static int dp_vec(int32_t dtype, const void* A, int64_t lda, int64_t M, const void* vecs_16 = nullptr) {
  return (dtype == RLS_F64 && (M & 1) == 0 && (lda & 1) == 0 && dp_aligned16(A) && dp_aligned16(vecs_16)) ? 2 : 1;
}

template <typename D, int V>
static int32_t dp_gemv_n_v(rls_ctx* ctx, const void* A, int64_t lda, const void* x, void* y, int64_t M, int64_t N, double* part, const int* done) {
  const dim3 grid((unsigned)dp_gn_grid(M, V)), block(GN_WAVES * 64);
  const int G = dp_gn_lanes(M, V);
  if (G == 64) return rls_launch<dp_gemv_n_kernel<D, V, 64>>(ctx, grid, block, 0, (const D*)A, lda, (const D*)x, (D*)y, M, N, part, done);
  if (G == 32) return rls_launch<dp_gemv_n_kernel<D, V, 32>>(ctx, grid, block, 0, (const D*)A, lda, (const D*)x, (D*)y, M, N, part, done);
  return rls_launch<dp_gemv_n_kernel<D, V, 16>>(ctx, grid, block, 0, (const D*)A, lda, (const D*)x, (D*)y, M, N, part, done);
}
// y = A x (A: M x N), part: dp_gn_grid(M, V) doubles
static int32_t dp_gemv_n(rls_ctx* ctx, int32_t dtype, const void* A, int64_t lda, const void* x, void* y, int64_t M, int64_t N, double* part,
                         const int* done) {
  if (dtype == RLS_C64) return dp_gemv_n_v<double2, 1>(ctx, A, lda, x, y, M, N, part, done);
  if (dp_vec(dtype, A, lda, M) == 2) return dp_gemv_n_v<double, 2>(ctx, A, lda, x, y, M, N, part, done);
  return dp_gemv_n_v<double, 1>(ctx, A, lda, x, y, M, N, part, done);
}
static int64_t dp_gn_parts(int32_t dtype, const void* A, int64_t lda, int64_t M) { return dp_gn_grid(M, dp_vec(dtype, A, lda, M)); }

template <typename D, int V>
static int32_t dp_gemv_t_v(rls_ctx* ctx, const void* A, int64_t lda, const void* t, void* v, int64_t M, int64_t N, const int* done) {
  const int CB = N / (GT_WAVES * 4) >= 512 ? 4 : N / (GT_WAVES * 2) >= 256 ? 2 : 1;
  const int64_t per = (int64_t)GT_WAVES * CB;
  const dim3 grid((unsigned)((N + per - 1) / per)), block(GT_WAVES * 64);
  if (CB == 4) return rls_launch<dp_gemv_t_kernel<D, V, 4>>(ctx, grid, block, 0, (const D*)A, lda, (const D*)t, (D*)v, M, N, done);
  if (CB == 2) return rls_launch<dp_gemv_t_kernel<D, V, 2>>(ctx, grid, block, 0, (const D*)A, lda, (const D*)t, (D*)v, M, N, done);
  return rls_launch<dp_gemv_t_kernel<D, V, 1>>(ctx, grid, block, 0, (const D*)A, lda, (const D*)t, (D*)v, M, N, done);
}
// v = A^H t
static int32_t dp_gemv_t(rls_ctx* ctx, int32_t dtype, const void* A, int64_t lda, const void* t, void* v, int64_t M, int64_t N, const int* done) {
  if (dtype == RLS_C64) return dp_gemv_t_v<double2, 1>(ctx, A, lda, t, v, M, N, done);
  if (dp_vec(dtype, A, lda, M, t) == 2) return dp_gemv_t_v<double, 2>(ctx, A, lda, t, v, M, N, done);
  return dp_gemv_t_v<double, 1>(ctx, A, lda, t, v, M, N, done);
}

// v = AHA p of one iteration: one product over the Gram matrix, or t = A p and v = A^H t (the only passes over A)
static int32_t dp_normal(dp_base& B, const void* p, void* v, const int* done) {
  if (B.G) return dp_gemv_n(B.ctx, B.dtype, B.G, B.ldg, p, v, B.N, B.N, B.part, done);
  RLS_TRY(dp_gemv_n(B.ctx, B.dtype, B.A, B.lda, p, B.t, B.M, B.N, B.part, done));
  return dp_gemv_t(B.ctx, B.dtype, B.A, B.lda, B.t, v, B.M, B.N, done);
}
// out = A^H b, or b itself for a Gram-only plan (initCGNR src/CGNR.jl:132-134, src/FISTA.jl:114-116)
static int32_t dp_adjoint_b(dp_base& B, const void* b, void* out) {
  if (B.A) return dp_gemv_t(B.ctx, B.dtype, B.A, B.lda, b, out, B.M, B.N, nullptr);
  RLS_HIP(B.ctx, hipMemcpyAsync(out, b, (size_t)B.N * dp_elem(B.dtype), hipMemcpyDeviceToDevice, B.ctx->stream));
  return 0;
}

static int32_t dp_base_create(dp_base& B, rls_ctx* ctx, int32_t dtype, int64_t M, int64_t N, const void* A, int64_t lda, const void* AHA, int64_t ldg,
                              const char* who) {
  if (!dp_dtype_ok(dtype)) return rls_fail(ctx, RLS_E_INVALID, "Float64 / ComplexF64 plan: dtype must be RLS_F64 or RLS_C64");
  if (N <= 0 || (!A && !AHA) || (A && (M <= 0 || lda < M)) || (AHA && ldg < N)) return rls_fail(ctx, RLS_E_INVALID, who);
  B.ctx = ctx;
  B.ctx_id = ctx->id;
  B.dtype = dtype;
  B.M = A ? M : 0;
  B.N = N;
  B.A = A;
  B.lda = lda;
  B.G = AHA;
  B.ldg = ldg;
  RLS_HIP(ctx, rls_enter(ctx));
  int64_t parts = 1;
  if (AHA) {
    parts = dp_gn_parts(dtype, AHA, ldg, N);
  } else {
    parts = dp_gn_parts(dtype, A, lda, M);
    B.mem.dev(&B.t, (size_t)M * dp_elem(dtype), false);
  }
  B.npart = (int)parts;
  B.mem.dev(&B.part, (size_t)parts * sizeof(double), false);
  return 0;
}
// the record and its pinned mirror, behind dp_base_create; the status of everything the plan has asked for
template <typename R>
static int32_t dp_rec_create(dp_base& B, R** rec_d, R** rec_h, const char* who) {
  B.mem.dev(rec_d, sizeof(R), false);
  B.mem.pinned(rec_h, sizeof(R), false);
  const int e = B.mem.error();
  return e ? rls_fail(B.ctx, e, who) : 0;
}
static void dp_base_destroy(dp_base& B) {
  if (rls_ctx_alive(B.ctx, B.ctx_id)) (void)rls_enter(B.ctx);
  B.mem.release();
}
// one synchronising read of the device record
template <typename R>
static int32_t dp_fetch(rls_ctx* ctx, const R* rec_d, R* rec_h) {
  RLS_HIP(ctx, hipMemcpyAsync(rec_h, rec_d, sizeof(R), hipMemcpyDeviceToHost, ctx->stream));
  RLS_HIP(ctx, rls_stream_wait(ctx->stream));
  return 0;
}

}  // namespace

struct rls_cgnr_d {
  dp_base B;
  void *x = nullptr, *r = nullptr, *p = nullptr, *v = nullptr;
  dcg_rec *rec = nullptr, *rec_h = nullptr;
};
struct rls_fista_d {
  dp_base B;
  void* buf[2] = {nullptr, nullptr};
  void *x0 = nullptr, *res = nullptr;
  dfi_rec *rec = nullptr, *rec_h = nullptr;
  int32_t reg_kind = RLS_REG_NONE, proj_kind = RLS_PROJ_NONE;
  int64_t l21_slices = 1;
  double lambda = 0.0;
  bool status_current = false;  // rec_h holds the record as of the last launch enqueued (rls_fista_solution_d then needs no read)
  int64_t enqueued = 0;  // iterations enqueued since init: the parity that says which buffer is x.  Launches behind `done` are
                         // no-ops, so every launch that does work sees this count equal to the record's `iteration`.
};

namespace {

template <typename D>
static int32_t dp_cgnr_step(rls_cgnr_d* s, int32_t n) {
  dp_base& B = s->B;
  for (int32_t k = 0; k < n; ++k) {
    RLS_TRY(dp_normal(B, s->p, s->v, &s->rec->done));
    if (B.G)
      RLS_TRY((rls_launch<dp_cgnr_update_kernel<D, true>>(B.ctx, dim3(1), dim3(UPD_T), 0, (D*)s->x, (D*)s->r, (D*)s->p, (const D*)s->v, B.N,
                                                          (const double*)B.part, B.npart, s->rec)));
    else
      RLS_TRY((rls_launch<dp_cgnr_update_kernel<D, false>>(B.ctx, dim3(1), dim3(UPD_T), 0, (D*)s->x, (D*)s->r, (D*)s->p, (const D*)s->v, B.N,
                                                           (const double*)B.part, B.npart, s->rec)));
  }
  return 0;
}

template <typename D>
static int32_t dp_fista_step(rls_fista_d* s, int32_t n) {
  dp_base& B = s->B;
  unsigned eg = (unsigned)((B.N + 255) / 256);
  if (eg > 2048) eg = 2048;
  for (int32_t k = 0; k < n; ++k) {
    D* y = (D*)s->buf[(s->enqueued + 1) & 1];            // x_{k-2}, overwritten by the extrapolated point and then by x_k
    const D* xprev = (const D*)s->buf[s->enqueued & 1];  // x_{k-1}
    RLS_TRY((rls_launch<dp_fista_extrapolate_kernel<D>>(B.ctx, dim3(eg), dim3(256), 0, y, xprev, B.N, (const dfi_rec*)s->rec)));
    RLS_TRY(dp_normal(B, y, s->res, &s->rec->done));
    RLS_TRY((rls_launch<dp_fista_update_kernel<D>>(B.ctx, dim3(1), dim3(UPD_T), 0, y, xprev, (const D*)s->x0, (D*)s->res, B.N, s->rec)));
    ++s->enqueued;
  }
  return 0;
}

static void dp_cgnr_publish(const dcg_rec& r, rls_cgnr_status_d* o) {
  o->iteration = r.iteration;
  o->done = r.done;
  o->alpha_re = r.alpha_re;
  o->alpha_im = r.alpha_im;
  o->beta_re = r.beta_re;
  o->beta_im = r.beta_im;
  o->zeta = r.zeta;
  o->residual = r.residual;
  o->z0 = r.z0;
}
static void dp_fista_publish(const dfi_rec& r, rls_fista_status_d* o) {
  o->iteration = r.iteration;
  o->done = r.done;
  o->theta = r.theta;
  o->theta_old = r.theta_old;
  o->rel_res_norm = r.rel_res_norm;
  o->residual = r.res_norm;
  o->norm_x0 = r.norm_x0;
}

}  // namespace

extern "C" {

int32_t rls_cgnr_create_d(rls_ctx* ctx, int32_t dtype, int64_t M, int64_t N, const void* A, int64_t lda, const void* AHA, int64_t ldg, void* x,
                          void* r, void* p, void* v, rls_cgnr_d** out) {
  RLS_CHECK_CTX(ctx);
  if (!out || !x || !r || !p || !v) return rls_fail(ctx, RLS_E_INVALID, "cgnr_create_d: null pointer");
  *out = nullptr;
  rls_cgnr_d* s = new rls_cgnr_d{{dp_memory(ctx)}};
  int32_t st = dp_base_create(s->B, ctx, dtype, M, N, A, lda, AHA, ldg, "cgnr_create_d: bad argument");
  if (st == 0) st = dp_rec_create(s->B, &s->rec, &s->rec_h, "cgnr_create_d: allocation failed");
  if (st != 0) {
    rls_cgnr_destroy_d(s);
    return st;
  }
  s->x = x;
  s->r = r;
  s->p = p;
  s->v = v;
  *out = s;
  return 0;
}
int32_t rls_cgnr_destroy_d(rls_cgnr_d* s) {
  if (!s) return RLS_E_INVALID;
  dp_base_destroy(s->B);
  delete s;
  return 0;
}
int32_t rls_cgnr_init_d(rls_cgnr_d* s, const void* b, double lambda, double rel_tol, int32_t iterations) {
  if (!s) return RLS_E_INVALID;
  dp_base& B = s->B;
  if (!b) return rls_fail(B.ctx, RLS_E_INVALID, "cgnr_init_d: null pointer");
  RLS_HIP(B.ctx, rls_enter(B.ctx));
  RLS_TRY(dp_adjoint_b(B, b, s->r));
  const int max_iter = (int)(iterations < B.N ? iterations : B.N);  // done(): iteration >= min(iterations, N)
  RLS_TRY(rls_with_elem64(B.dtype, [&](auto t) {
    using D = typename decltype(t)::type;
    return rls_launch<dp_cgnr_init_kernel<D>>(B.ctx, dim3(1), dim3(UPD_T), 0, (D*)s->x, (const D*)s->r, (D*)s->p, (D*)s->v, B.N, lambda,
                                              rel_tol, max_iter, s->rec);
  }));
  B.initialised = true;
  return 0;
}
int32_t rls_cgnr_step_d(rls_cgnr_d* s, int32_t n_steps) {
  if (!s) return RLS_E_INVALID;
  dp_base& B = s->B;
  if (!B.initialised) return rls_fail(B.ctx, RLS_E_STATE, "cgnr_step_d before cgnr_init_d");
  if (n_steps < 0) return rls_fail(B.ctx, RLS_E_INVALID, "cgnr_step_d: negative step count");
  RLS_HIP(B.ctx, rls_enter(B.ctx));
  return rls_with_elem64(B.dtype, [&](auto t) { return dp_cgnr_step<typename decltype(t)::type>(s, n_steps); });
}
int32_t rls_cgnr_get_status_d(rls_cgnr_d* s, rls_cgnr_status_d* out_h) {
  if (!s) return RLS_E_INVALID;
  dp_base& B = s->B;
  if (!out_h) return rls_fail(B.ctx, RLS_E_INVALID, "cgnr_get_status_d: null pointer");
  if (!B.initialised) return rls_fail(B.ctx, RLS_E_STATE, "cgnr_get_status_d before cgnr_init_d");
  RLS_HIP(B.ctx, rls_enter(B.ctx));
  RLS_TRY(dp_fetch(B.ctx, s->rec, s->rec_h));
  dp_cgnr_publish(*s->rec_h, out_h);
  return 0;
}
int32_t rls_cgnr_step_status_d(rls_cgnr_d* s, int32_t n_steps, rls_cgnr_status_d* out_h) {
  if (!s) return RLS_E_INVALID;
  if (!out_h) return rls_fail(s->B.ctx, RLS_E_INVALID, "cgnr_step_status_d: null pointer");
  RLS_TRY(rls_cgnr_step_d(s, n_steps));
  return rls_cgnr_get_status_d(s, out_h);
}
int32_t rls_cgnr_path_d(rls_cgnr_d* s, int32_t* out) {
  if (!s) return RLS_E_INVALID;
  if (!out) return rls_fail(s->B.ctx, RLS_E_INVALID, "cgnr_path_d: null pointer");
  *out = s->B.G ? 2 : 0;
  return 0;
}

int32_t rls_fista_create_d(rls_ctx* ctx, int32_t dtype, int64_t M, int64_t N, const void* A, int64_t lda, const void* AHA, int64_t ldg, void* x,
                           void* x0, void* xold, void* res, rls_fista_d** out) {
  RLS_CHECK_CTX(ctx);
  if (!out || !x || !x0 || !xold || !res) return rls_fail(ctx, RLS_E_INVALID, "fista_create_d: null pointer");
  *out = nullptr;
  rls_fista_d* s = new rls_fista_d{{dp_memory(ctx)}};
  int32_t st = dp_base_create(s->B, ctx, dtype, M, N, A, lda, AHA, ldg, "fista_create_d: bad argument");
  if (st == 0) st = dp_rec_create(s->B, &s->rec, &s->rec_h, "fista_create_d: allocation failed");
  if (st != 0) {
    rls_fista_destroy_d(s);
    return st;
  }
  s->buf[0] = x;
  s->buf[1] = xold;
  s->x0 = x0;
  s->res = res;
  *out = s;
  return 0;
}
int32_t rls_fista_destroy_d(rls_fista_d* s) {
  if (!s) return RLS_E_INVALID;
  dp_base_destroy(s->B);
  delete s;
  return 0;
}
int32_t rls_fista_set_reg_d(rls_fista_d* s, int32_t reg_kind, double lambda, int64_t l21_slices, int32_t proj_kind) {
  if (!s) return RLS_E_INVALID;
  rls_ctx* ctx = s->B.ctx;
  if (reg_kind != RLS_REG_NONE && reg_kind != RLS_REG_L1 && reg_kind != RLS_REG_L2 && reg_kind != RLS_REG_L21)
    return rls_fail(ctx, RLS_E_UNSUPPORTED, "fista_set_reg_d: the plan applies none / L1 / L2 / L21 (TV and nested terms: the primitives)");
  if (proj_kind != RLS_PROJ_NONE && proj_kind != RLS_PROJ_REAL && proj_kind != RLS_PROJ_POSITIVE)
    return rls_fail(ctx, RLS_E_INVALID, "fista_set_reg_d: unknown projection");
  if (reg_kind == RLS_REG_L21 && (l21_slices <= 0 || s->B.N / l21_slices == 0)) return rls_fail(ctx, RLS_E_INVALID, "fista_set_reg_d: bad l21_slices");
  s->reg_kind = reg_kind;
  s->lambda = lambda;
  s->l21_slices = reg_kind == RLS_REG_L21 ? l21_slices : 1;
  s->proj_kind = proj_kind;
  return 0;
}
int32_t rls_fista_init_d(rls_fista_d* s, const void* b, double rho, double theta, double rel_tol, int32_t iterations, int32_t restart_gradient) {
  if (!s) return RLS_E_INVALID;
  dp_base& B = s->B;
  if (!b) return rls_fail(B.ctx, RLS_E_INVALID, "fista_init_d: null pointer");
  RLS_HIP(B.ctx, rls_enter(B.ctx));
  RLS_TRY(dp_adjoint_b(B, b, s->x0));
  dfi_rec init = {};
  init.rho = rho;
  init.theta = theta;
  init.rel_tol = rel_tol;
  init.thr = rho * s->lambda;  // prox!(reg, x, rho * lambda)   src/FISTA.jl:164
  init.l21_slices = s->l21_slices;
  init.max_iter = iterations;
  init.restart = restart_gradient ? 1 : 0;
  init.reg_kind = s->reg_kind;
  init.proj_kind = s->proj_kind;
  RLS_TRY(rls_with_elem64(B.dtype, [&](auto t) {
    using D = typename decltype(t)::type;
    return rls_launch<dp_fista_init_kernel<D>>(B.ctx, dim3(1), dim3(UPD_T), 0, (D*)s->buf[0], (D*)s->buf[1], (const D*)s->x0,
                                               (D*)s->res, B.N, init, s->rec);
  }));
  s->enqueued = 0;
  s->status_current = false;
  B.initialised = true;
  return 0;
}
int32_t rls_fista_set_start_d(rls_fista_d* s, const void* x_init, int64_t n) {
  if (!s) return RLS_E_INVALID;
  dp_base& B = s->B;
  if (!B.initialised || s->enqueued != 0) return rls_fail(B.ctx, RLS_E_STATE, "fista_set_start_d: call right after fista_init_d");
  if (!x_init) return rls_fail(B.ctx, RLS_E_INVALID, "fista_set_start_d: null pointer");
  if (n != B.N) return rls_fail(B.ctx, RLS_E_INVALID, "fista_set_start_d: x_init must have the solution's length N");
  RLS_HIP(B.ctx, rls_enter(B.ctx));
  // state.x .= x0 (src/FISTA.jl:120): iteration 0's x is buf[0]; the first extrapolated point is formed from it by the first step
  RLS_HIP(B.ctx, hipMemcpyAsync(s->buf[0], x_init, (size_t)B.N * dp_elem(B.dtype), hipMemcpyDeviceToDevice, B.ctx->stream));
  return 0;
}
int32_t rls_fista_step_d(rls_fista_d* s, int32_t n_steps) {
  if (!s) return RLS_E_INVALID;
  dp_base& B = s->B;
  if (!B.initialised) return rls_fail(B.ctx, RLS_E_STATE, "fista_step_d before fista_init_d");
  if (n_steps < 0) return rls_fail(B.ctx, RLS_E_INVALID, "fista_step_d: negative step count");
  RLS_HIP(B.ctx, rls_enter(B.ctx));
  if (n_steps > 0) s->status_current = false;
  return rls_with_elem64(B.dtype, [&](auto t) { return dp_fista_step<typename decltype(t)::type>(s, n_steps); });
}
int32_t rls_fista_get_status_d(rls_fista_d* s, rls_fista_status_d* out_h) {
  if (!s) return RLS_E_INVALID;
  dp_base& B = s->B;
  if (!out_h) return rls_fail(B.ctx, RLS_E_INVALID, "fista_get_status_d: null pointer");
  if (!B.initialised) return rls_fail(B.ctx, RLS_E_STATE, "fista_get_status_d before fista_init_d");
  RLS_HIP(B.ctx, rls_enter(B.ctx));
  RLS_TRY(dp_fetch(B.ctx, s->rec, s->rec_h));
  s->status_current = true;
  dp_fista_publish(*s->rec_h, out_h);
  return 0;
}
int32_t rls_fista_step_status_d(rls_fista_d* s, int32_t n_steps, rls_fista_status_d* out_h) {
  if (!s) return RLS_E_INVALID;
  if (!out_h) return rls_fail(s->B.ctx, RLS_E_INVALID, "fista_step_status_d: null pointer");
  RLS_TRY(rls_fista_step_d(s, n_steps));
  return rls_fista_get_status_d(s, out_h);
}
int32_t rls_fista_solution_d(rls_fista_d* s, void** x_out) {
  if (!s) return RLS_E_INVALID;
  if (!x_out) return rls_fail(s->B.ctx, RLS_E_INVALID, "fista_solution_d: null pointer");
  if (!s->B.initialised) return rls_fail(s->B.ctx, RLS_E_STATE, "fista_solution_d before fista_init_d");
  if (!s->status_current) {  // (right behind a status call the record is on the host already: no second synchronisation)
    rls_fista_status_d st;
    RLS_TRY(rls_fista_get_status_d(s, &st));
  }
  *x_out = s->buf[s->rec_h->iteration & 1];  // the pointer swap of src/FISTA.jl:144-146
  return 0;
}
int32_t rls_fista_path_d(rls_fista_d* s, int32_t* out) {
  if (!s) return RLS_E_INVALID;
  if (!out) return rls_fail(s->B.ctx, RLS_E_INVALID, "fista_path_d: null pointer");
  *out = s->B.G ? 2 : 0;
  return 0;
}

}  // extern "C"
