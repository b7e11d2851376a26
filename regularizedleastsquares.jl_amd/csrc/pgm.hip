// Fused elementwise halves of the OptISTA and POGM iterations: everything of iterate that follows
// res = AHA x (src/OptISTA.jl:176-204, src/POGM.jl:176-233) in ONE launch instead of 8-12 BLAS-1 style launches.
// The momentum coefficients depend on the iteration index only and are computed by the host in Float32 exactly as
// the reference does; the kernels return the data-dependent scalars (||res||, and for POGM's gradient restart the
// real parts of <w,x>, <w,z>, <w,res>) through the context's result block.
#include "rls_common.hpp"

constexpr int PGM_THREADS = 1024;

// Deferred mode (rls_*_update_async): the iteration count, ||res|| and the reference's stopping test
// `rel_res_norm < relTol` (src/OptISTA.jl:206-209, src/POGM.jl:234-237) live in a 4-word device record, every
// launch of the sequence is a no-op once `done` is set, and the host reads the record once per solve.
// (struct pgm_state: rls_common.hpp)
__device__ static inline void pgm_state_step(pgm_state* st, float res_norm, float norm_x0, float rel_tol) {
  if (!st) return;
  st->iteration += 1;
  st->res_norm = res_norm;
  st->done = ((double)res_norm / (double)norm_x0) < (double)rel_tol;  // the host forms this quotient in double
}

template <typename E>
__device__ static inline double redot(E a, E b) {  // real(conj(a) * b)
  return (double)elem<E>::re(a) * (double)elem<E>::re(b) + (double)elem<E>::im(a) * (double)elem<E>::im(b);
}

// zold = z; z = y; res -= x0; y -= step * res; prox(y, thr); z = z / (-gamma) + x + y / gamma;
// x = -beta x + (1 + alpha + beta) z - alpha zold
// One element of it (shared with the batched kernel below): `raw` = (AHA x)[i], zo / ztmp / xi = z[i], y[i], x[i] on entry.
struct optista_coefs {
  float step, thr, c_z, c_y, c_x, c_zn, c_zo;
  int reg_kind;
};
template <typename E>
__device__ static inline void optista_elem(const optista_coefs& c, E raw, E x0i, E zo, E ztmp, E xi, E& r, E& yn, E& zn, E& xn) {
  r = elem<E>::sub(raw, x0i);
  yn = elem<E>::add(ztmp, elem<E>::scale(-c.step, r));
  yn = fista_prox_elem<E>(yn, c.reg_kind, c.thr);
  zn = elem<E>::add(elem<E>::scale(c.c_z, ztmp), xi);
  zn = elem<E>::add(zn, elem<E>::scale(c.c_y, yn));
  xn = elem<E>::add(elem<E>::scale(c.c_x, xi), elem<E>::scale(c.c_zn, zn));
  xn = elem<E>::add(xn, elem<E>::scale(c.c_zo, zo));
}

template <typename E>
__global__ __launch_bounds__(PGM_THREADS) void optista_update_kernel(E* __restrict__ res, const E* __restrict__ x0,
                                                                     E* __restrict__ x, E* __restrict__ y,
                                                                     E* __restrict__ z, E* __restrict__ zold, int64_t n,
                                                                     float step, int reg_kind, float thr, float c_z,
                                                                     float c_y, float c_x, float c_zn, float c_zo,
                                                                     float* __restrict__ out, pgm_state* state,
                                                                     float norm_x0, float rel_tol) {
  __shared__ double sm[16];
  if (state && state->done) return;
  const optista_coefs c{step, thr, c_z, c_y, c_x, c_zn, c_zo, reg_kind};
  double rn = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += PGM_THREADS) {
    const E zo = z[i], ztmp = y[i], xi = x[i];
    E r, yn, zn, xn;
    optista_elem<E>(c, res[i], x0[i], zo, ztmp, xi, r, yn, zn, xn);
    res[i] = r;
    rn += redot<E>(r, r);
    zold[i] = zo;
    y[i] = yn;
    z[i] = zn;
    x[i] = xn;
  }
  rn = block_sum(rn, sm);
  if (threadIdx.x == 0) {
    out[0] = (float)sqrt(rn);
    pgm_state_step(state, out[0], norm_x0, rel_tol);
  }
}

// xbuf holds x_k, ybuf holds y_{k-1} on entry; on exit xbuf holds the gradient point (the new y after the
// reference's swap, src/POGM.jl:203) and ybuf the new x, so the caller swaps its two references.
// Returns (valid in every thread) ||res||^2 and, with RESTART, real <w,x>, <w,z>, <w,res>.
// One element of it (shared with the batched kernel below): `raw` = (AHA x)[i]; xo, yp, zi, wi = xbuf[i], ybuf[i], z[i], w[i]
// on entry (wi is read with RESTART only).  x1 goes to xbuf, xn to ybuf, zn to z, wn to w, xo to xold.
struct pogm_coefs {
  float rho, c_y, c_x1, c_xo, c_z, thr, rg;
  int reg_kind, proj_kind;
};
template <typename E, bool RESTART>
__device__ static inline void pogm_elem(const pogm_coefs& c, E raw, E x0i, E xo, E yp, E zi, E wi, E& r, E& x1, E& xn, E& zn,
                                        E& wn, double& dwx, double& dwz, double& dwr) {
  r = elem<E>::sub(raw, x0i);                             // res .-= x0                         :178
  x1 = elem<E>::add(xo, elem<E>::scale(-c.rho, r));       // x .-= rho .* res                   :179
  xn = elem<E>::add(elem<E>::scale(c.c_y, yp), elem<E>::scale(c.c_x1, x1));  // after the swap  :204-205
  xn = elem<E>::add(xn, elem<E>::scale(c.c_xo, xo));
  xn = elem<E>::add(xn, elem<E>::scale(c.c_z, zi));
  zn = xn;                                                // z .= x                              :210
  xn = fista_proj_elem<E>(fista_prox_elem<E>(xn, c.reg_kind, c.thr), c.proj_kind);
  if constexpr (RESTART) {                                // gradient restart                    :218-232
    wi = elem<E>::add(wi, x1);
    wi = elem<E>::add(wi, elem<E>::scale(c.rg, xn));
    wi = elem<E>::add(wi, elem<E>::scale(-c.rg, zn));
    dwx += redot<E>(wi, xn);
    dwz += redot<E>(wi, zn);
    dwr += redot<E>(wi, r);
    wn = elem<E>::add(elem<E>::scale(c.rg, zn), elem<E>::scale(-c.rg, xn));
    wn = elem<E>::sub(wn, x1);
  }
}

template <typename E, bool RESTART>
__device__ static inline void pogm_update_body(E* __restrict__ res, const E* __restrict__ x0, E* __restrict__ xbuf,
                                               E* __restrict__ ybuf, E* __restrict__ xold, E* __restrict__ z,
                                               E* __restrict__ w, int64_t n, float rho, float c_y, float c_x1,
                                               float c_xo, float c_z, int reg_kind, float thr, int proj_kind, float rg,
                                               double* sm /* 48 */, double& rn, double& dwx, double& dwz, double& dwr) {
  rn = dwx = dwz = dwr = 0.0;
  const pogm_coefs c{rho, c_y, c_x1, c_xo, c_z, thr, rg, reg_kind, proj_kind};
  for (int64_t i = threadIdx.x; i < n; i += PGM_THREADS) {
    const E xo = xbuf[i], yp = ybuf[i];
    E wi = elem<E>::zero();
    if constexpr (RESTART) wi = w[i];
    E r, x1, xn, zn, wn;
    pogm_elem<E, RESTART>(c, res[i], x0[i], xo, yp, z[i], wi, r, x1, xn, zn, wn, dwx, dwz, dwr);
    res[i] = r;
    rn += redot<E>(r, r);
    xold[i] = xo;
    z[i] = zn;
    xbuf[i] = x1;
    ybuf[i] = xn;
    if constexpr (RESTART) w[i] = wn;
  }
  rn = block_sum(rn, sm);
  if constexpr (RESTART) block_sum3(dwx, dwz, dwr, sm);
}

template <typename E, bool RESTART>
__global__ __launch_bounds__(PGM_THREADS) void pogm_update_kernel(E* __restrict__ res, const E* __restrict__ x0,
                                                                  E* __restrict__ xbuf, E* __restrict__ ybuf,
                                                                  E* __restrict__ xold, E* __restrict__ z,
                                                                  E* __restrict__ w, int64_t n, float rho, float c_y,
                                                                  float c_x1, float c_xo, float c_z, int reg_kind,
                                                                  float thr, int proj_kind, float rg,
                                                                  float* __restrict__ out, pgm_state* state,
                                                                  float norm_x0, float rel_tol) {
  __shared__ double sm[48];
  if (state && state->done) return;
  double rn, dwx, dwz, dwr;
  pogm_update_body<E, RESTART>(res, x0, xbuf, ybuf, xold, z, w, n, rho, c_y, c_x1, c_xo, c_z, reg_kind, thr, proj_kind, rg,
                               sm, rn, dwx, dwz, dwr);
  if (threadIdx.x == 0) {
    out[0] = (float)sqrt(rn);
    out[1] = (float)dwx;
    out[2] = (float)dwz;
    out[3] = (float)dwr;
    pgm_state_step(state, out[0], norm_x0, rel_tol);
  }
}

// the coefficients of one POGM iteration with restart = :gradient, formed from the record's theta, sigma, gamma
// (src/POGM.jl:183-201; `last`: the final iteration's theta rule, :185).  One rounding per operation, as NumPy's Float32
// scalars on the host (f32_mul / f32_add: never fused).
struct pogm_auto_coefs {
  float th, alpha, c_x1, gamma, c_z, c_xo, thr, rg;
};
__device__ static inline pogm_auto_coefs pogm_auto_form(float tho, float sigma, float gamma_old, bool last, float rho, float lam) {
  pogm_auto_coefs a;
  const float t2 = f32_mul(f32_mul(last ? 8.f : 4.f, tho), tho);      // :183-187
  a.th = f32_add(1.f, sqrtf(f32_add(1.f, t2))) / 2.f;  // sqrtf: correctly rounded (v_sqrt_f32 alone is not)
  a.alpha = f32_sub(tho, 1.f) / a.th;                                  // :189
  const float beta = f32_mul(sigma, tho) / a.th;                       // :190
  a.c_x1 = f32_add(f32_add(1.f, a.alpha), beta);
  a.gamma = f32_mul(rho, a.c_x1);                                      // :195  rho (1 + alpha + beta)
  a.c_z = f32_mul(rho, a.alpha) / gamma_old;
  a.c_xo = -f32_add(beta, a.c_z);
  a.thr = f32_mul(a.gamma, lam);
  a.rg = rho / a.gamma;
  return a;
}
// the restart criterion (:224) from the three real dot products
__device__ static inline bool pogm_auto_restart(float gamma, double dwx, double dwz, double dwr) {
  const float crit = f32_sub(f32_sub((float)dwx, (float)dwz) / gamma, (float)dwr);
  return crit < 0.f;
}

// POGM with gradient restart, deferred: theta, sigma and gamma live in the device record and the coefficients of an
// iteration (src/POGM.jl:183-201) are formed HERE from them, in Float32 with the host's operation order (explicit
// round-to-nearest intrinsics: no contraction), so that the data-dependent restart decision (:218-232) never has to
// travel to the host.
// (struct pogm_auto_state: rls_common.hpp)
template <typename E>
__global__ __launch_bounds__(PGM_THREADS) void pogm_auto_kernel(E* __restrict__ res, const E* __restrict__ x0,
                                                                E* __restrict__ xbuf, E* __restrict__ ybuf,
                                                                E* __restrict__ xold, E* __restrict__ z,
                                                                E* __restrict__ w, int64_t n, float rho, float lam,
                                                                float sigma_fac, int max_iter, int reg_kind,
                                                                int proj_kind, pogm_auto_state* st, float norm_x0,
                                                                float rel_tol) {
  __shared__ double sm[48];
  if (st->done) return;
  const float tho = st->theta, sigma = st->sigma;
  const pogm_auto_coefs a = pogm_auto_form(tho, sigma, st->gamma, st->iteration == max_iter - 1, rho, lam);
  double rn, dwx, dwz, dwr;
  pogm_update_body<E, true>(res, x0, xbuf, ybuf, xold, z, w, n, rho, -a.alpha, a.c_x1, a.c_xo, a.c_z, reg_kind, a.thr, proj_kind,
                            a.rg, sm, rn, dwx, dwz, dwr);
  if (threadIdx.x == 0) {
    const bool restart = pogm_auto_restart(a.gamma, dwx, dwz, dwr);
    st->theta_old = tho;
    st->theta = restart ? 1.f : a.th;
    st->sigma = restart ? 1.f : f32_mul(sigma, sigma_fac);
    st->gamma = a.gamma;
    const float rnorm = (float)sqrt(rn);
    st->res_norm = rnorm;
    st->iteration += 1;
    st->done = ((double)rnorm / (double)norm_x0) < (double)rel_tol;
  }
}

// ---------------------------------------------------------------------------------------------
// Batched OptISTA / POGM: K right-hand sides share one pass over A per product (skinny.hip); these kernels are the
// per-column halves, workgroup b = column b (the plan: plan_pgm.hip, rls_pgm_create_batched).  AHA x arrives as `S`
// partial rows per column and is summed here in fixed order; the next gradient point also goes into the operand
// panel.  Every column carries its own iteration count: the coefficient row and (POGM) the roles of the two x / y
// buffers follow it, so columns that retire at different iterations need nothing from the host.
// ---------------------------------------------------------------------------------------------
constexpr int PGMB_THREADS = 1024;

// x0 = A^H b from the partial rows, ||x0||, the state vectors as OptISTA.init_ / POGM.init_ leave them (x = 0 and every
// other vector 0, res = Inf), the first gradient point (x = 0) in the panel, the column's record
template <typename E>
__global__ __launch_bounds__(PGMB_THREADS) void pgmb_init_kernel(rls_pgmb D) {
  __shared__ double sm[16];
  const int b = blockIdx.x;
  const int64_t n = D.N, off = (int64_t)b * D.ldv;
  E* x0 = (E*)D.x0 + off;
  E* res = (E*)D.res + off;
  E* v[5] = {(E*)D.v0 + off, (E*)D.v1 + off, (E*)D.v2 + off, (E*)D.o0 + off, D.v3 ? (E*)D.v3 + off : nullptr};
  const operand_view<E> O(D.ops);
  const panel_col<E> pc = O.column(n, b);
  const float inf = __builtin_huge_valf();
  double nn = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += PGMB_THREADS) {
    const E a = O.sum(b, n, i);
    x0[i] = a;
    nn += redot<E>(a, a);
#pragma unroll
    for (int k = 0; k < 5; ++k)
      if (v[k]) v[k][i] = elem<E>::zero();
    res[i] = elem<E>::make(inf, 0.f);
    pc.put(i, elem<E>::zero());
  }
  nn = block_sum_n<PGMB_THREADS / 64>(nn, sm);
  if (threadIdx.x == 0) {
    pgmb_scalars* sc = D.sc + b;
    sc->norm_x0 = sqrt(nn);
    sc->res_norm = inf;
    sc->rel_res_norm = inf;
    sc->theta = D.theta;
    sc->theta_old = D.theta;
    sc->sigma = 1.f;
    sc->gamma = D.gamma0;
    sc->iteration = 0;
    sc->done = (0 >= D.max_iter);
  }
}

// One iteration of column b after the two products: optista_elem / pogm_elem over the column, in tiles of EPT elements per
// thread whose loads are all requested before the first use (EPT * PGMB_THREADS >= N: the whole column in registers, one
// tile; EPT = 1 is the plain strided loop).  The per-thread summation order is the element order in both forms.
template <typename E, int KIND, int EPT>
__global__ __launch_bounds__(PGMB_THREADS) void pgmb_update_kernel(rls_pgmb D) {
  constexpr bool POGM = KIND != RLS_PGMB_OPTISTA, RESTART = KIND == RLS_PGMB_POGM_RESTART;
  __shared__ double sm[48];
  const int b = blockIdx.x;
  pgmb_scalars* sc = D.sc + b;
  if (sc->done) return;  // a retired column keeps its vectors, its panel entry and its record
  const int it = sc->iteration;
  const int64_t n = D.N, off = (int64_t)b * D.ldv;
  // OptISTA: a0 = x, a1 = y.  POGM: a0 = the buffer that holds x_k (v0 after an even number of iterations), a1 = y_{k-1};
  // on exit a1 holds the new x (src/POGM.jl:203)
  E* a0 = (E*)((POGM && (it & 1)) ? D.v1 : D.v0) + off;
  E* a1 = (E*)((POGM && (it & 1)) ? D.v0 : D.v1) + off;
  E* z = (E*)D.v2 + off;
  E* o0 = (E*)D.o0 + off;
  E* res = (E*)D.res + off;
  E* w = RESTART ? (E*)D.v3 + off : nullptr;
  const E* x0 = (const E*)D.x0 + off;
  const operand_view<E> O(D.ops);
  const panel_col<E> pc = O.column(n, b);
  optista_coefs oc = {};
  pogm_coefs gc = {};
  pogm_auto_coefs au = {};
  float tho = 0.f, sigma = 0.f;
  if constexpr (KIND == RLS_PGMB_OPTISTA) {  // the row of THIS column's iteration (rls_pgm_coefs)
    const float* r = D.table + 8 * (int64_t)it;
    oc = optista_coefs{r[0], r[1], r[2], r[3], r[4], r[5], r[6], D.reg_kind};
  } else if constexpr (KIND == RLS_PGMB_POGM) {
    const float* r = D.table + 8 * (int64_t)it;
    gc = pogm_coefs{r[0], r[2], r[3], r[4], r[5], r[1], 0.f, D.reg_kind, D.proj_kind};
  } else {  // the record's theta, sigma, gamma (pogm_auto_kernel)
    tho = sc->theta;
    sigma = sc->sigma;
    au = pogm_auto_form(tho, sigma, sc->gamma, it == D.max_iter - 1, D.rho, D.lambda);
    gc = pogm_coefs{D.rho, -au.alpha, au.c_x1, au.c_xo, au.c_z, au.thr, au.rg, D.reg_kind, D.proj_kind};
  }
  double rn = 0.0, dwx = 0.0, dwz = 0.0, dwr = 0.0;
  for (int64_t base = 0; base < n; base += (int64_t)EPT * PGMB_THREADS) {
    E raw[EPT], x0v[EPT], p0[EPT], p1[EPT], zv[EPT], wv[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      const int64_t i = base + threadIdx.x + (int64_t)e * PGMB_THREADS;
      const int64_t ic = i < n ? i : n - 1;
      raw[e] = O.sum(b, n, ic);
      x0v[e] = x0[ic];
      p0[e] = a0[ic];
      p1[e] = a1[ic];
      zv[e] = z[ic];
      wv[e] = elem<E>::zero();
      if constexpr (RESTART) wv[e] = w[ic];
    }
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      const int64_t i = base + threadIdx.x + (int64_t)e * PGMB_THREADS;
      if (i >= n) continue;
      E r, xn;
      if constexpr (!POGM) {
        E yn, zn;
        optista_elem<E>(oc, raw[e], x0v[e], zv[e], p1[e], p0[e], r, yn, zn, xn);
        o0[i] = zv[e];
        a1[i] = yn;
        z[i] = zn;
        a0[i] = xn;
      } else {
        E x1, zn, wn;
        pogm_elem<E, RESTART>(gc, raw[e], x0v[e], p0[e], p1[e], zv[e], wv[e], r, x1, xn, zn, wn, dwx, dwz, dwr);
        o0[i] = p0[e];
        z[i] = zn;
        a0[i] = x1;
        a1[i] = xn;
        if constexpr (RESTART) w[i] = wn;
      }
      res[i] = r;
      rn += redot<E>(r, r);
      pc.put(i, xn);  // the next gradient point: the new x
    }
  }
  rn = block_sum_n<PGMB_THREADS / 64>(rn, sm);
  if constexpr (RESTART) block_sum3_n<PGMB_THREADS / 64>(dwx, dwz, dwr, sm);
  if (threadIdx.x == 0) {
    if constexpr (RESTART) {
      const bool restart = pogm_auto_restart(au.gamma, dwx, dwz, dwr);
      sc->theta_old = tho;
      sc->theta = restart ? 1.f : au.th;
      sc->sigma = restart ? 1.f : f32_mul(sigma, D.sigma_fac);
      sc->gamma = au.gamma;
    }
    const float rnorm = (float)sqrt(rn);
    const double rel = (double)rnorm / sc->norm_x0;  // the quotient in double (pgm_state_step)
    sc->res_norm = rnorm;
    sc->rel_res_norm = (float)rel;
    sc->iteration = it + 1;
    sc->done = (rel < (double)D.rel_tol) || (it + 1 >= D.max_iter);
  }
}

template <typename E, int KIND>
static void pgmb_launch_update_typed(rls_ctx* ctx, const rls_pgmb& D) {
  const dim3 grid((unsigned)D.nrhs), block(PGMB_THREADS);
  const int64_t n = D.N;
  if (ctx->tune.pgm_batched_reg && n > PGMB_THREADS && n <= 2 * PGMB_THREADS)
    hipLaunchKernelGGL((pgmb_update_kernel<E, KIND, 2>), grid, block, 0, ctx->stream, D);
  else if (ctx->tune.pgm_batched_reg && n > 2 * PGMB_THREADS && n <= 4 * PGMB_THREADS)
    hipLaunchKernelGGL((pgmb_update_kernel<E, KIND, 4>), grid, block, 0, ctx->stream, D);
  else
    hipLaunchKernelGGL((pgmb_update_kernel<E, KIND, 1>), grid, block, 0, ctx->stream, D);
}

static bool pgmb_desc_ok(const rls_pgmb& D) {
  return D.kind >= RLS_PGMB_OPTISTA && D.kind <= RLS_PGMB_POGM_RESTART && D.N > 0 && D.ldv >= D.N && D.nrhs >= 1 && D.v0 && D.v1 &&
         D.v2 && D.o0 && D.res && D.x0 && D.ops.Vpart && D.ops.panel && D.sc && D.ops.S >= 1 && D.ops.nrhs_pad >= D.nrhs &&
         (D.kind != RLS_PGMB_POGM_RESTART || D.v3) && (D.kind == RLS_PGMB_POGM_RESTART || D.table) &&
         D.reg_kind >= RLS_REG_NONE && D.reg_kind <= RLS_REG_L2 && D.proj_kind >= RLS_PROJ_NONE && D.proj_kind <= RLS_PROJ_POSITIVE;
}

int32_t rls_pgmb_launch_init(rls_ctx* ctx, int32_t dtype, const rls_pgmb& D) {
  if (!rls_dtype_ok(dtype) || !pgmb_desc_ok(D)) return rls_fail(ctx, RLS_E_INVALID, "batched OptISTA / POGM init: bad argument");
  return rls_with_elem(dtype, [&](auto t) {
    return rls_launch<pgmb_init_kernel<typename decltype(t)::type>>(ctx, dim3((unsigned)D.nrhs), dim3(PGMB_THREADS), 0, D);
  });
}

int32_t rls_pgmb_launch_update(rls_ctx* ctx, int32_t dtype, const rls_pgmb& D) {
  if (!rls_dtype_ok(dtype) || !pgmb_desc_ok(D)) return rls_fail(ctx, RLS_E_INVALID, "batched OptISTA / POGM update: bad argument");
  rls_with_elem(dtype, [&](auto t) {
    rls_with<RLS_PGMB_OPTISTA, RLS_PGMB_POGM, RLS_PGMB_POGM_RESTART>(
        D.kind, [&](auto KIND) { pgmb_launch_update_typed<typename decltype(t)::type, KIND>(ctx, D); });
  });
  return launch_status(ctx);
}

static int32_t pgm_fetch(rls_ctx* ctx, float* out_h, int nfloats) {
  RLS_HIP(ctx, hipMemcpyAsync(ctx->res_h, ctx->res_d, sizeof(float) * (size_t)nfloats, hipMemcpyDeviceToHost, ctx->stream));
  RLS_HIP(ctx, rls_stream_wait(ctx->stream));
  for (int i = 0; i < nfloats; ++i) out_h[i] = ctx->res_h[i];
  return 0;
}

extern "C" {

static int32_t optista_launch(rls_ctx* ctx, int32_t dtype, int64_t n, void* res, const void* x0, void* x, void* y, void* z,
                              void* zold, float step, int32_t reg_kind, float thr, float c_z, float c_y, float c_x,
                              float c_zn, float c_zo, pgm_state* state, float norm_x0, float rel_tol) {
  RLS_CHECK_CTX(ctx);
  if (!rls_dtype_ok(dtype) || n <= 0 || !res || !x0 || !x || !y || !z || !zold || reg_kind < RLS_REG_NONE ||
      reg_kind > RLS_REG_L2)
    return rls_fail(ctx, RLS_E_INVALID, "optista_update: bad argument");
  RLS_HIP(ctx, rls_enter(ctx));
  return rls_with_elem(dtype, [&](auto t) {
    using E = typename decltype(t)::type;
    return rls_launch<optista_update_kernel<E>>(ctx, dim3(1), dim3(PGM_THREADS), 0, (E*)res, (const E*)x0, (E*)x, (E*)y, (E*)z,
                                                (E*)zold, n, step, reg_kind, thr, c_z, c_y, c_x, c_zn, c_zo, ctx->res_d, state,
                                                norm_x0, rel_tol);
  });
}

int32_t rls_optista_update(rls_ctx* ctx, int32_t dtype, int64_t n, void* res, const void* x0, void* x, void* y, void* z,
                           void* zold, float step, int32_t reg_kind, float thr, float c_z, float c_y, float c_x,
                           float c_zn, float c_zo, float* res_norm_h) {
  RLS_CHECK_CTX(ctx);
  if (!res_norm_h) return rls_fail(ctx, RLS_E_INVALID, "optista_update: null result pointer");
  RLS_TRY(optista_launch(ctx, dtype, n, res, x0, x, y, z, zold, step, reg_kind, thr, c_z, c_y, c_x, c_zn, c_zo, nullptr,
                         1.f, 0.f));
  return pgm_fetch(ctx, res_norm_h, 1);
}

int32_t rls_optista_update_async(rls_ctx* ctx, int32_t dtype, int64_t n, void* res, const void* x0, void* x, void* y,
                                 void* z, void* zold, float step, int32_t reg_kind, float thr, float c_z, float c_y,
                                 float c_x, float c_zn, float c_zo, float norm_x0, float rel_tol, void* state_d) {
  RLS_CHECK_CTX(ctx);
  if (!state_d) return rls_fail(ctx, RLS_E_INVALID, "optista_update_async: null state");
  return optista_launch(ctx, dtype, n, res, x0, x, y, z, zold, step, reg_kind, thr, c_z, c_y, c_x, c_zn, c_zo,
                        (pgm_state*)state_d, norm_x0, rel_tol);
}

static int32_t pogm_launch(rls_ctx* ctx, int32_t dtype, int64_t n, void* res, const void* x0, void* xbuf, void* ybuf,
                           void* xold, void* z, void* w, float rho, float c_y, float c_x1, float c_xo, float c_z,
                           int32_t reg_kind, float thr, int32_t proj_kind, int32_t restart, float rho_over_gamma,
                           pgm_state* state, float norm_x0, float rel_tol) {
  RLS_CHECK_CTX(ctx);
  if (!rls_dtype_ok(dtype) || n <= 0 || !res || !x0 || !xbuf || !ybuf || !xold || !z || (restart && !w) ||
      reg_kind < RLS_REG_NONE || reg_kind > RLS_REG_L2 || proj_kind < RLS_PROJ_NONE || proj_kind > RLS_PROJ_POSITIVE)
    return rls_fail(ctx, RLS_E_INVALID, "pogm_update: bad argument");
  RLS_HIP(ctx, rls_enter(ctx));
  return rls_with_elem(dtype, [&](auto t) {
    using E = typename decltype(t)::type;
    return with_bool(restart != 0, [&](auto RESTART) {
      return rls_launch<pogm_update_kernel<E, RESTART>>(ctx, dim3(1), dim3(PGM_THREADS), 0, (E*)res, (const E*)x0, (E*)xbuf,
                                                        (E*)ybuf, (E*)xold, (E*)z, (E*)w, n, rho, c_y, c_x1, c_xo, c_z, reg_kind,
                                                        thr, proj_kind, rho_over_gamma, ctx->res_d, state, norm_x0, rel_tol);
    });
  });
}

int32_t rls_pogm_update(rls_ctx* ctx, int32_t dtype, int64_t n, void* res, const void* x0, void* xbuf, void* ybuf,
                        void* xold, void* z, void* w, float rho, float c_y, float c_x1, float c_xo, float c_z,
                        int32_t reg_kind, float thr, int32_t proj_kind, int32_t restart, float rho_over_gamma,
                        float* out_h) {
  RLS_CHECK_CTX(ctx);
  if (!out_h) return rls_fail(ctx, RLS_E_INVALID, "pogm_update: null result pointer");
  RLS_TRY(pogm_launch(ctx, dtype, n, res, x0, xbuf, ybuf, xold, z, w, rho, c_y, c_x1, c_xo, c_z, reg_kind, thr, proj_kind,
                      restart, rho_over_gamma, nullptr, 1.f, 0.f));
  return pgm_fetch(ctx, out_h, 4);
}

// restart = :none only (the gradient restart feeds data-dependent theta / sigma back into the next coefficients)
int32_t rls_pogm_update_async(rls_ctx* ctx, int32_t dtype, int64_t n, void* res, const void* x0, void* xbuf, void* ybuf,
                              void* xold, void* z, float rho, float c_y, float c_x1, float c_xo, float c_z,
                              int32_t reg_kind, float thr, int32_t proj_kind, float norm_x0, float rel_tol,
                              void* state_d) {
  RLS_CHECK_CTX(ctx);
  if (!state_d) return rls_fail(ctx, RLS_E_INVALID, "pogm_update_async: null state");
  return pogm_launch(ctx, dtype, n, res, x0, xbuf, ybuf, xold, z, nullptr, rho, c_y, c_x1, c_xo, c_z, reg_kind, thr,
                     proj_kind, 0, 0.f, (pgm_state*)state_d, norm_x0, rel_tol);
}

// POGM, restart = :gradient, deferred.  state_d: 8 device words {int32 iteration, int32 done, float ||res||, pad,
// float theta, theta_old, sigma, gamma}; the caller writes theta, sigma, gamma (and zeroes the rest) before the
// first iteration and reads all of it back after the last.
int32_t rls_pogm_update_auto(rls_ctx* ctx, int32_t dtype, int64_t n, void* res, const void* x0, void* xbuf, void* ybuf,
                             void* xold, void* z, void* w, float rho, float lambda, float sigma_fac, int32_t iterations,
                             int32_t reg_kind, int32_t proj_kind, float norm_x0, float rel_tol, void* state_d) {
  RLS_CHECK_CTX(ctx);
  if (!rls_dtype_ok(dtype) || n <= 0 || !res || !x0 || !xbuf || !ybuf || !xold || !z || !w || !state_d ||
      reg_kind < RLS_REG_NONE || reg_kind > RLS_REG_L2 || proj_kind < RLS_PROJ_NONE || proj_kind > RLS_PROJ_POSITIVE)
    return rls_fail(ctx, RLS_E_INVALID, "pogm_update_auto: bad argument");
  RLS_HIP(ctx, rls_enter(ctx));
  return rls_with_elem(dtype, [&](auto t) {
    using E = typename decltype(t)::type;
    return rls_launch<pogm_auto_kernel<E>>(ctx, dim3(1), dim3(PGM_THREADS), 0, (E*)res, (const E*)x0, (E*)xbuf, (E*)ybuf, (E*)xold,
                                           (E*)z, (E*)w, n, rho, lambda, sigma_fac, iterations, reg_kind, proj_kind,
                                           (pogm_auto_state*)state_d, norm_x0, rel_tol);
  });
}

}  // extern "C"
