// FISTA (src/FISTA.jl:110-189) as a device plan: single and batched right-hand sides, the TV and wavelet regularisers as
// launches of their own inside the update, server mode of the resident kernels, and the row-sharded entry points.
#include "plans.hpp"

// ---------------------------------------------------------------------------------------------
// FISTA
// ---------------------------------------------------------------------------------------------
struct rls_fista {
  plan_buffers mem;  // owns every block below, srv.ctl and resident.{sync, flags_h} included
  rls_operator* op = nullptr;
  rls_ctx* actx = nullptr;
  uint64_t actx_id = 0;
  int device = 0;
  void* buf[2] = {nullptr, nullptr};  // x / xold, swapped by iteration parity: state.x == buf[iteration & 1]
  void *x0 = nullptr, *res = nullptr;
  void* y = nullptr;       // extrapolated point (plan-owned), the GEMV input
  void *y1 = nullptr, *res_raw = nullptr;  // fused pipeline: second extrapolated-point buffer, AHA y before "- x0"
  fista_scalars* scn = nullptr;  // staged scalars (slab pipeline) / second parity (Gram pipeline)
  bool use_pipe = false;
  void* res_raw1 = nullptr;      // Gram pipeline: second parity of AHA y
  bool use_gram = false;
  fista_scalars* sc = nullptr;
  fista_scalars* sc_h = nullptr;
  step_graph graph;
  int32_t reg_kind = RLS_REG_L1, proj_kind = RLS_PROJ_NONE;
  float lambda = 0.f;
  int64_t l21_slices = 1;
  bool initialised = false;
  // batched plan (rls_fista_create_batched): nrhs columns ldv elements apart, the K extrapolated points as an
  // MFMA operand panel, T = A Y and the partial rows of A^H T (skinny.hip)
  int nrhs = 1;
  int64_t ldv = 0;
  shared_operands ops;             // (the panel: the extrapolated points)
  fista_scalars* scb_h = nullptr;  // pinned [nrhs]
  int enq = 0;           // iterations enqueued since init (== the device's count unless the plan stopped early); its parity at
                         // capture is the key of the cached graph (step_graph::mode): the buffer hints belong to it
  float theta0 = 1.f;    // theta given to the last init (rls_fista_set_start needs it)
  resident_slot resident;     // resident mode (normal.hip, fista_resident_kernel)
  bool small = false;         // dense A that fits ONE CU's registers: whole step calls on fista_small_kernel (small.hip)
  srv_state srv;              // server mode of the resident kernel (rls_fista_step_status)
  rls_mailbox_slot mb_arm;    // as the cgnr plan's
  bool mb_sent = false;
  long long requested = 0;    // iterations asked for since init
  // batched plan on an explicit Gram matrix, <= 8 ComplexF32 columns, AHA in the register files (gramk.hip): exchange scratch
  bool fgramk = false;
  int restart_b = 0;          // gradient restart asked for at init (the resident batched kernel does not carry it)
  float* fk_yx = nullptr;
  void* fk_xx = nullptr;
  double* fk_dots = nullptr;
  // TV regulariser (rls_fista_set_reg_tv): the FGP launch sits BETWEEN the two halves of the update (src/FISTA.jl:164), reading the
  // gradient step from tv_in and leaving prox_TV of it in tv_out (plan scratch: no pointer depends on the iteration's parity)
  int tv_ndims = 0, tv_ntv = 0, tv_iters = 10;
  int64_t tv_shape[4] = {1, 1, 1, 1};
  int32_t tv_dims[4] = {0, 0, 0, 0};
  void *tv_in = nullptr, *tv_out = nullptr;
  rls_wavelet* wav = nullptr;  // RLS_REG_WAVELET (rls_fista_set_reg_wavelet): the caller's handle; its launch takes the FGP launch's place
  uint64_t wav_serial = 0;     // ... and that handle's serial number: a cached graph has ITS filter, extents and depth as launch
                               // arguments, and a handle created after another was destroyed may come back at the same address
  float rho_h = 0.f;  // rho of the last init (the prox threshold rho * lambda is a launch argument of the FGP / wavelet kernel)
};

// x0 = A^H b is already in place.  x = x_init (zero), xold = 0, res = Inf, y = x   (src/FISTA.jl:110-129)
template <typename E>
__global__ __launch_bounds__(UPD_THREADS) void fista_init_kernel(E* __restrict__ b0, E* __restrict__ b1,
                                                                 E* __restrict__ x0, E* __restrict__ res,
                                                                 E* __restrict__ y, int64_t n, fista_scalars* sc,
                                                                 float rho, float theta, float rel_tol, int max_iter,
                                                                 int restart, int reg_kind, int proj_kind,
                                                                 float lambda, long long slices, col_batch<E> Bt,
                                                                 unsigned* clear_words = nullptr, int n_clear = 0) {
  __shared__ double sm[16];
  for (int i = threadIdx.x; i < n_clear; i += UPD_THREADS) clear_words[i] = 0u;  // (cgnr_init_kernel)
  const int b = blockIdx.x;
  b0 += b * Bt.ldv;
  b1 += b * Bt.ldv;
  x0 += b * Bt.ldv;
  res += b * Bt.ldv;
  y += b * Bt.ldv;
  sc += b;
  const panel_col<E> yp = Bt.ops.column(n, b);
  double nn = 0.0;
  const float inf = __builtin_huge_valf();
  for (int64_t i = threadIdx.x; i < n; i += UPD_THREADS) {
    E v;
    if (Bt.ops.Vpart) {  // x0 = A^H b from the partial rows of the skinny product
      v = Bt.ops.sum(b, n, i);
      x0[i] = v;
    } else {
      v = x0[i];
    }
    nn += (double)elem<E>::re(v) * (double)elem<E>::re(v) + (double)elem<E>::im(v) * (double)elem<E>::im(v);
    b0[i] = elem<E>::zero();
    b1[i] = elem<E>::zero();
    y[i] = elem<E>::zero();
    if (Bt.ops.panel) yp.put(i, elem<E>::zero());
    res[i] = elem<E>::make(inf, 0.f);
  }
  nn = block_sum_n<UPD_THREADS / 64>(nn, sm);
  if (threadIdx.x == 0) {
    sc->norm_x0 = sqrt(nn);
    sc->res_norm = (double)inf;
    sc->rel_res_norm = (double)inf;
    sc->rho = rho;
    sc->theta = theta;
    sc->theta_old = theta;
    sc->rel_tol = rel_tol;
    sc->lambda = lambda;
    sc->iteration = 0;
    sc->max_iter = max_iter;
    sc->done = (0 >= max_iter);
    sc->restart = restart;
    sc->reg_kind = reg_kind;
    sc->proj_kind = proj_kind;
    sc->l21_slices = slices;
    sc->pending = 0;
    sc->ycur = 0;
    sc->fresh = 0;
  }
}

// everything of src/FISTA.jl:153-180 after res = AHA y, plus the NEXT iteration's momentum step
// (:144-148) so that one iteration is GEMV, GEMV, this kernel.
// `phase` splits it around a prox that is a launch of its own (TV: the FGP kernel): 0 = everything; 1 = res, the gradient step
// into tv_in (not into x) and the residual norm; 2 = x = proj(tv_out), then the restart test, theta, `done` and the next y.
template <typename E>
__global__ __launch_bounds__(UPD_THREADS) void fista_update_kernel(E* __restrict__ b0, E* __restrict__ b1,
                                                                   const E* __restrict__ x0, E* __restrict__ res,
                                                                   E* __restrict__ y, int64_t n, fista_scalars* sc,
                                                                   col_batch<E> Bt, int phase = 0, E* __restrict__ tv_in = nullptr,
                                                                   const E* __restrict__ tv_out = nullptr) {
  const int b = blockIdx.x;
  b0 += b * Bt.ldv;
  b1 += b * Bt.ldv;
  x0 += b * Bt.ldv;
  res += b * Bt.ldv;
  y += b * Bt.ldv;
  sc += b;
  const panel_col<E> yp = Bt.ops.column(n, b);
  if (sc->done) return;  // a retired column keeps its panel entry (src/MultiThreading.jl:60-78)
  __shared__ double sm[16];
  const int it = sc->iteration;
  E* xnew = (it & 1) ? b0 : b1;  // after the reference's pointer swap: state.x      :144-146
  E* xold = (it & 1) ? b1 : b0;  // holds x_k
  const float rho = sc->rho;
  const int reg_kind = sc->reg_kind, proj_kind = sc->proj_kind;
  const float thr = rho * sc->lambda;  // prox!(reg, x, rho * lambda(reg))             :164
  double rn = 0.0;
  if (phase == 2) {  // the prox ran as a launch of its own: x = proj(prox), the residual norm is phase 1's
    for (int64_t i = threadIdx.x; i < n; i += UPD_THREADS) xnew[i] = fista_proj_elem<E>(tv_out[i], proj_kind);
    __syncthreads();
  } else {
  for (int64_t i = threadIdx.x; i < n; i += UPD_THREADS) {
    const E ri = elem<E>::sub(Bt.ops.Vpart ? Bt.ops.sum(b, n, i) : res[i], x0[i]);  // res .-= x0      :153
    res[i] = ri;
    rn += (double)elem<E>::re(ri) * (double)elem<E>::re(ri) + (double)elem<E>::im(ri) * (double)elem<E>::im(ri);
    E xi = elem<E>::sub(y[i], elem<E>::scale(rho, ri));             // x .-= rho .* res :154
    if (phase == 1) {
      tv_in[i] = xi;
      continue;
    }
    if (reg_kind != RLS_REG_L21) xi = fista_proj_elem<E>(fista_prox_elem<E>(xi, reg_kind, thr), proj_kind);
    xnew[i] = xi;
  }
  }
  if (reg_kind == RLS_REG_L21) {  // group soft-threshold needs the whole new x         ProxL21.jl:30-35
    __syncthreads();
    const int64_t slen = n / sc->l21_slices;
    for (int64_t g = threadIdx.x; g < slen; g += UPD_THREADS) {
      float s2 = 0.f;
      for (int64_t k = g; k < n; k += slen) s2 += elem<E>::abs2(xnew[k]);
      const float gn = sqrtf(s2);
      const float q = (gn - thr) / gn;
      const float fac = (q != q) ? q : fmaxf(q, 0.f);
      for (int64_t k = g; k < n; k += slen) xnew[k] = fista_proj_elem<E>(elem<E>::scale(fac, xnew[k]), proj_kind);
    }
    __syncthreads();
  }
  rn = block_sum(rn, sm);
  if (phase == 1) {
    if (threadIdx.x == 0) sc->res_norm = sqrt(rn);
    return;
  }
  float theta = sc->theta;
  if (sc->restart) {  // real(res . (x - xold)) > 0  => theta = 1                       :171-176
    double d = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += UPD_THREADS) {
      const E df = elem<E>::sub(xnew[i], xold[i]);
      const E ri = res[i];
      d += (double)elem<E>::re(ri) * (double)elem<E>::re(df) + (double)elem<E>::im(ri) * (double)elem<E>::im(df);
    }
    d = block_sum(d, sm);
    if (d > 0.0) theta = 1.f;
  }
  const float theta_old = theta;                                     // :179
  theta = (1.f + sqrtf(1.f + 4.f * theta_old * theta_old)) / 2.f;    // :180
  const double res_norm = phase == 2 ? sc->res_norm : sqrt(rn);
  const float rel = (float)(res_norm / sc->norm_x0);                 // :156
  const int done = (rel < sc->rel_tol) || (it + 1 >= sc->max_iter);  // :187-189
  if (!done) {
    // next iteration's Nesterov step, formed out of place in y                         :147-148
    const float c1 = (1.f - theta_old) / theta;
    const float c2 = (theta_old - 1.f) / theta + 1.f;
    for (int64_t i = threadIdx.x; i < n; i += UPD_THREADS) {
      const E yi = elem<E>::add(elem<E>::scale(c1, xold[i]), elem<E>::scale(c2, xnew[i]));
      y[i] = yi;
      if (Bt.ops.panel) yp.put(i, yi);
    }
  }
  if (threadIdx.x == 0) {
    sc->res_norm = res_norm;
    sc->rel_res_norm = (double)rel;
    sc->theta = theta;
    sc->theta_old = theta_old;
    sc->iteration = it + 1;
    sc->done = done;
  }
}

// fista_update_kernel with the vectors in registers (n <= EPT * UPD_THREADS; every regulariser but L21, whose
// group norms need the whole new x): all loads requested up front, the same per-thread summation order.
template <typename E, int EPT>
__global__ __launch_bounds__(UPD_THREADS) void fista_update_reg_kernel(E* __restrict__ b0, E* __restrict__ b1,
                                                                       const E* __restrict__ x0, E* __restrict__ res,
                                                                       E* __restrict__ y, int64_t n, fista_scalars* sc,
                                                                       col_batch<E> Bt) {
  const int b = blockIdx.x;
  b0 += b * Bt.ldv;
  b1 += b * Bt.ldv;
  x0 += b * Bt.ldv;
  res += b * Bt.ldv;
  y += b * Bt.ldv;
  sc += b;
  const panel_col<E> yp = Bt.ops.column(n, b);
  __shared__ double sm[16];
  const int done0 = sc->done, it = sc->iteration, reg_kind = sc->reg_kind, proj_kind = sc->proj_kind;
  const int restart = sc->restart, max_iter = sc->max_iter;
  const float rho = sc->rho, lam = sc->lambda, rel_tol = sc->rel_tol, theta0 = sc->theta;
  const double norm_x0 = sc->norm_x0;
  E* xnew = (it & 1) ? b0 : b1;  // after the reference's pointer swap: state.x      :144-146
  E* xold = (it & 1) ? b1 : b0;  // holds x_k
  E raw[EPT], x0v[EPT], yv[EPT], xo[EPT];
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const int64_t i = threadIdx.x + (int64_t)e * UPD_THREADS;
    const int64_t ic = i < n ? i : n - 1;
    raw[e] = Bt.ops.Vpart ? Bt.ops.sum(b, n, ic) : res[ic];
    x0v[e] = x0[ic];
    yv[e] = y[ic];
    xo[e] = xold[ic];
  }
  if (done0) return;  // a retired column keeps its panel entry (src/MultiThreading.jl:60-78)
  const float thr = rho * lam;  // prox!(reg, x, rho * lambda(reg))             :164
  E ri[EPT], xn[EPT];
  double rn = 0.0;
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const int64_t i = threadIdx.x + (int64_t)e * UPD_THREADS;
    ri[e] = elem<E>::sub(raw[e], x0v[e]);                                      // res .-= x0      :153
    E xi = elem<E>::sub(yv[e], elem<E>::scale(rho, ri[e]));                    // x .-= rho .* res :154
    xn[e] = fista_proj_elem<E>(fista_prox_elem<E>(xi, reg_kind, thr), proj_kind);
    if (i < n) rn += (double)elem<E>::re(ri[e]) * (double)elem<E>::re(ri[e]) + (double)elem<E>::im(ri[e]) * (double)elem<E>::im(ri[e]);
  }
  rn = block_sum(rn, sm);
  float theta = theta0;
  if (restart) {  // real(res . (x - xold)) > 0  => theta = 1                       :171-176
    double d = 0.0;
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      const int64_t i = threadIdx.x + (int64_t)e * UPD_THREADS;
      const E df = elem<E>::sub(xn[e], xo[e]);
      if (i < n) d += (double)elem<E>::re(ri[e]) * (double)elem<E>::re(df) + (double)elem<E>::im(ri[e]) * (double)elem<E>::im(df);
    }
    d = block_sum(d, sm);
    if (d > 0.0) theta = 1.f;
  }
  const float theta_old = theta;                                     // :179
  theta = (1.f + sqrtf(1.f + 4.f * theta_old * theta_old)) / 2.f;    // :180
  const double res_norm = sqrt(rn);
  const float rel = (float)(res_norm / norm_x0);                     // :156
  const int done = (rel < rel_tol) || (it + 1 >= max_iter);          // :187-189
  const float c1 = (1.f - theta_old) / theta;
  const float c2 = (theta_old - 1.f) / theta + 1.f;
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const int64_t i = threadIdx.x + (int64_t)e * UPD_THREADS;
    if (i < n) {
      xnew[i] = xn[e];
      res[i] = ri[e];
      if (!done) {  // next iteration's Nesterov step, formed out of place in y                         :147-148
        const E yi = elem<E>::add(elem<E>::scale(c1, xo[e]), elem<E>::scale(c2, xn[e]));
        y[i] = yi;
        if (Bt.ops.panel) yp.put(i, yi);
      }
    }
  }
  if (threadIdx.x == 0) {
    sc->res_norm = res_norm;
    sc->rel_res_norm = (double)rel;
    sc->theta = theta;
    sc->theta_old = theta_old;
    sc->iteration = it + 1;
    sc->done = done;
  }
}

// launch of the update half of an unfused / batched FISTA iteration: the register form when it applies
template <typename E>
static int32_t fista_launch_update(rls_fista* s, unsigned nblocks, const col_batch<E>& Bt) {
  rls_operator* op = s->op;
  const int64_t n = op->N;
  int32_t tv_status = 0;
#define RLS_FUPD_REG(EE)                                                                                            \
  hipLaunchKernelGGL((fista_update_reg_kernel<E, EE>), dim3(nblocks), dim3(UPD_THREADS), 0, op->ctx->stream,        \
                     (E*)s->buf[0], (E*)s->buf[1], (const E*)s->x0, (E*)s->res, (E*)s->y, n, s->sc, Bt)
  if (s->reg_kind == RLS_REG_TV || s->reg_kind == RLS_REG_WAVELET) {  // gradient step | prox launch (its own workgroup, skipped once `done`) | projection, theta, y
    hipLaunchKernelGGL(fista_update_kernel<E>, dim3(1), dim3(UPD_THREADS), 0, op->ctx->stream, (E*)s->buf[0], (E*)s->buf[1],
                       (const E*)s->x0, (E*)s->res, (E*)s->y, n, s->sc, Bt, 1, (E*)s->tv_in, (const E*)s->tv_out);
    // (the threshold rho * lambda, the geometry and iterationsTV are kernel ARGUMENTS: a cached graph of this sequence is dropped
    //  whenever one of them changes -- fista_drop_graph in rls_fista_set_reg / _set_reg_tv / fista_init_finish)
    if (s->reg_kind == RLS_REG_WAVELET)  // W^T soft(W tv_in, rho lambda): analysis, threshold and synthesis in one workgroup's LDS
      tv_status = rls_wavelet_prox_launch(s->wav, s->tv_in, s->tv_out, s->rho_h * s->lambda, &s->sc->done);
    else
      tv_status = rls_tv_single_launch(op->ctx, op->dtype, s->tv_ndims, s->tv_shape, s->tv_ntv, s->tv_dims, s->tv_in, nullptr, s->tv_out,
                                       s->rho_h * s->lambda, s->tv_iters, &s->sc->done, 1, 0, 0);
    hipLaunchKernelGGL(fista_update_kernel<E>, dim3(1), dim3(UPD_THREADS), 0, op->ctx->stream, (E*)s->buf[0], (E*)s->buf[1],
                       (const E*)s->x0, (E*)s->res, (E*)s->y, n, s->sc, Bt, 2, (E*)s->tv_in, (const E*)s->tv_out);
  } else if (s->reg_kind != RLS_REG_L21 && n <= 4 * UPD_THREADS) {
    if (n <= UPD_THREADS) RLS_FUPD_REG(1);
    else if (n <= 2 * UPD_THREADS) RLS_FUPD_REG(2);
    else RLS_FUPD_REG(4);
  } else {
    hipLaunchKernelGGL(fista_update_kernel<E>, dim3(nblocks), dim3(UPD_THREADS), 0, op->ctx->stream, (E*)s->buf[0],
                       (E*)s->buf[1], (const E*)s->x0, (E*)s->res, (E*)s->y, n, s->sc, Bt);
  }
#undef RLS_FUPD_REG
  return tv_status;  // (a refused FGP launch would leave phase 2 reading a stale tv_out: the step reports it)
}

static bool fista_pipe_ok(const rls_fista* s) {
  const rls_ctx* ctx = s->op->ctx;
  return s->y1 && s->op->slab && !s->op->G && ctx->tune.fused_normal && ctx->tune.cgnr_pipeline &&
         (s->reg_kind == RLS_REG_NONE || s->reg_kind == RLS_REG_L1 || s->reg_kind == RLS_REG_L2);
}

static bool fista_gram_ok(const rls_fista* s) {
  const rls_ctx* ctx = s->op->ctx;
  return s->res_raw1 && s->op->G && ctx->tune.gram_pipeline &&
         (s->reg_kind == RLS_REG_NONE || s->reg_kind == RLS_REG_L1 || s->reg_kind == RLS_REG_L2);
}

static rls_fista_gram fista_gram_desc(const rls_fista* s) {
  rls_fista_gram P;
  P.G = s->op->G;
  P.ldg = s->op->ldg;
  P.N = s->op->N;
  P.b0 = s->buf[0];
  P.b1 = s->buf[1];
  P.x0 = s->x0;
  P.res = s->res;
  P.y0 = s->y;
  P.y1 = s->y1;
  P.rr[0] = s->res_raw;
  P.rr[1] = s->res_raw1;
  P.sc[0] = s->sc;
  P.sc[1] = s->scn;
  return P;
}

static rls_fista_pipe fista_pipe_desc(const rls_fista* s) {
  rls_fista_pipe P;
  P.A = s->op->A;
  P.lda = s->op->lda;
  P.M = s->op->M;
  P.N = s->op->N;
  P.b0 = s->buf[0];
  P.b1 = s->buf[1];
  P.x0 = s->x0;
  P.res = s->res;
  P.y0 = s->y;
  P.y1 = s->y1;
  P.res_raw = s->res_raw;
  P.slab = s->op->slab;
  P.sc = s->sc;
  P.scn = s->scn;
  return P;
}

static int32_t fista_enqueue_iteration(rls_fista* s) {
  rls_operator* op = s->op;
  RLS_TRY(op_normal(op, s->y, s->res, &s->sc->done));
  RLS_TRY(rls_with_elem(op->dtype, [&](auto t) {
    using E = typename decltype(t)::type;
    return fista_launch_update<E>(s, 1, col_batch<E>());
  }));
  return launch_status(op->ctx);
}

// ---- batched FISTA (shared A, matrix-core products) ----------------------------------------------
static rls_skinny fista_skinny_desc(const rls_fista* s) { return s->ops.desc(s->op, s->nrhs, s->ldv); }

template <typename E>
static col_batch<E> fista_batch_desc(const rls_fista* s) {
  return col_batch<E>{s->ldv, s->ops.view<E>(s->nrhs)};
}

static int32_t fista_enqueue_batched(rls_fista* s) {
  rls_operator* op = s->op;
  rls_ctx* ctx = op->ctx;
  RLS_TRY(rls_skinny_launch(ctx, op->dtype, fista_skinny_desc(s), 1 | 2));
  RLS_TRY(rls_with_elem(op->dtype, [&](auto t) {
    using E = typename decltype(t)::type;
    return fista_launch_update<E>(s, (unsigned)s->nrhs, fista_batch_desc<E>(s));
  }));
  return launch_status(ctx);
}

static rls_operator* fista_op(rls_fista* s) { return s->op; }
static bool fista_single(rls_fista* s) { return s->nrhs == 1; }

static int32_t fista_init_finish(rls_fista* s, float rho, float theta, float rel_tol, int32_t iterations,
                                 int32_t restart_gradient, bool local) {
  rls_operator* op = s->op;
  rls_ctx* ctx = op->ctx;
  RLS_HIP(ctx, rls_enter(ctx));
  rls_with_elem(op->dtype, [&](auto t) {
    using E = typename decltype(t)::type;
    hipLaunchKernelGGL(fista_init_kernel<E>, dim3(1), dim3(UPD_THREADS), 0, ctx->stream, (E*)s->buf[0], (E*)s->buf[1], (E*)s->x0,
                       (E*)s->res, (E*)s->y, op->N, s->sc, rho, theta, rel_tol, iterations, restart_gradient, s->reg_kind,
                       s->proj_kind, s->lambda, (long long)s->l21_slices, col_batch<E>(),
                       (unsigned*)s->resident.sync,
                       s->resident.sync ? (int)(rls_resident_sync_clear_bytes() / sizeof(unsigned)) : 0);
  });
  s->resident.clean = s->resident.sync != nullptr;
  s->enq = 0;
  s->requested = 0;
  s->theta0 = theta;
  if (s->reg_kind == RLS_REG_TV) {
    if (rho != s->rho_h) s->graph.drop();  // rho * lambda is an argument of the captured FGP launch
    // the single-workgroup FGP kernel was checked when the regulariser was set; its limits are context tunables that may have moved
    if (!rls_tv_single_ok(op->ctx, op->dtype, s->tv_ndims, s->tv_shape, s->tv_ntv, s->tv_dims))
      return rls_fail(ctx, RLS_E_UNSUPPORTED, "fista_init: the TV image no longer fits the single-workgroup FGP kernel");
  }
  if (s->reg_kind == RLS_REG_WAVELET) {  // the same two rules for the wavelet launch
    if (rho != s->rho_h) s->graph.drop();
    if (!rls_wavelet_single_ok(s->wav, op->ctx, op->dtype, op->N) || rls_wavelet_serial(s->wav) != s->wav_serial)
      return rls_fail(ctx, RLS_E_UNSUPPORTED, "fista_init: the image no longer takes the single-workgroup wavelet kernel");
  }
  s->rho_h = rho;
  s->srv.off = false;  // (a new solve: the caller's pattern between iterates is judged afresh)
  s->srv.short_lives = 0;
  s->initialised = true;
  // row-sharded plans exchange `res` between the operator apply and the update: two-half iterations only
  const bool gram = !local && fista_gram_ok(s);
  const bool pipe = !local && !gram && fista_pipe_ok(s);
  if ((pipe != s->use_pipe || gram != s->use_gram) && s->graph.exec) s->graph.drop();  // captured for another kernel sequence
  s->use_pipe = pipe;
  s->use_gram = gram;
  return launch_status(ctx);
}

static void fista_status_out(const rls_fista* s, const fista_scalars& h, rls_fista_status* out) {
  out->iteration = h.iteration;
  out->done = h.done;
  out->theta = h.theta;
  out->theta_old = h.theta_old;
  out->rel_res_norm = (float)h.rel_res_norm;
  out->residual = (float)h.res_norm;
  out->norm_x0 = (float)h.norm_x0;
  out->fallbacks = s->resident.fallbacks;
}

static bool fista_use_resident(const rls_fista* s) {
  return s->nrhs == 1 && s->use_pipe && s->resident.usable(s->op->ctx) && aligned16(s->buf[0], s->buf[1], s->x0, s->res);
}

static bool fista_use_gram_resident(const rls_fista* s) {
  return s->nrhs == 1 && s->use_gram && s->resident.usable(s->op->ctx);
}

// batched Gram mode as ONE resident launch per step call (cgnr_use_gramk): no gradient restart -- its theta is the one global
// scalar the distributed update would have to wait for -- and the elementwise regularisers
static bool fista_use_gramk(const rls_fista* s, int n_steps) {
  return s->fgramk && s->resident.usable(s->op->ctx) && !s->restart_b &&
         (s->reg_kind == RLS_REG_NONE || s->reg_kind == RLS_REG_L1 || s->reg_kind == RLS_REG_L2) &&
         (n_steps != 1 || s->op->ctx->tune.resident == 2);
}

static rls_fgramk fista_gramk_desc(const rls_fista* s) {
  rls_fgramk D;
  D.G = s->op->G;
  D.ldg = s->op->ldg;
  D.N = s->op->N;
  D.nrhs = s->nrhs;
  D.b0 = s->buf[0];
  D.b1 = s->buf[1];
  D.x0 = s->x0;
  D.res = s->res;
  D.y = s->y;
  D.ldv = s->ldv;
  D.sc = s->sc;
  D.Yx = s->fk_yx;
  D.Xx = s->fk_xx;
  D.dots = s->fk_dots;
  D.Ypack = s->ops.panel;
  return D;
}

// small systems: the whole step call as a single-workgroup launch, A in ONE CU's registers (as cgnr_use_small), for the
// regularisers the fused updates cover elementwise.  The kernel keeps the plan's state in the pipeline's layout (y0 / y1 by
// `ycur`); a plan without the pipeline's second buffer (shapes the slab kernels do not take) hands it y0 twice, which is the
// two-GEMV path's layout.
static bool fista_use_small(const rls_fista* s) {
  return s->small && s->nrhs == 1 && !s->use_gram && s->op->ctx->tune.small && s->op->ctx->tune.resident &&
         (s->reg_kind == RLS_REG_NONE || s->reg_kind == RLS_REG_L1 || s->reg_kind == RLS_REG_L2);
}

static int32_t fista_step_impl(rls_fista* s, int32_t n_steps) {
  rls_ctx* ctx = s->op->ctx;
  if (fista_use_small(s)) {
    if (n_steps == 0) return 0;
    rls_fista_pipe P = fista_pipe_desc(s);
    if (!P.y1) P.y1 = P.y0;
    P.mb = s->mb_arm;
    s->mb_sent = s->mb_arm.dst != nullptr;
    s->enq += n_steps;
    return rls_fista_small_launch(ctx, s->op->dtype, P, n_steps);
  }
  if (fista_use_gramk(s, n_steps)) {  // AHA explicit, <= 8 columns: the whole call as ONE launch (fista_gramk_resident_kernel)
    if (n_steps == 0) return 0;
    const rls_fgramk D = fista_gramk_desc(s);
    return s->resident.launch(ctx, [&](void* sync, unsigned spin) { return rls_fgramk_resident_launch(ctx, D, sync, n_steps, spin); });
  }
  if (s->nrhs > 1) {  // K columns share A: T = A Y, V = A^H T on the matrix cores, then one workgroup per column
    return run_steps(ctx, &s->graph, n_steps, [s]() { return fista_enqueue_batched(s); });
  }
  if (s->use_gram) {
    // explicit AHA: one launch per iteration (two-parity state, see cgnr_gram_kernel); the finish kernel
    // applies the last update and leaves the scalars in both parities, so every call starts at parity 0
    rls_fista_gram P = fista_gram_desc(s);
    const int32_t dtype = s->op->dtype;
    if (fista_use_gram_resident(s)) {  // the whole call as ONE launch, AHA in registers (fista_gram_resident_kernel)
      if (n_steps == 0) return 0;
      s->enq += n_steps;
      return s->resident.launch(ctx, [&](void* sync, unsigned spin) {
        return rls_fista_gram_resident_launch(ctx, dtype, P, sync, n_steps, spin);
      });
    }
    const int it0 = s->enq;  // buffer hints as in the slab pipeline below
    s->graph.keep_for(it0 & 1);
    int parity = 0, k = 0;
    auto one = [ctx, dtype, &P, &parity, &k, it0]() {
      const int hk = pipe_cur_hint(ctx, k);
      P.par_hint = hk < 0 ? -1 : ((it0 + (k > 0 ? k - 1 : 0)) & 1);
      if (hk >= 0 && ctx->tune.pipe_hint_mode == 2) P.par_hint ^= 1;
      ++k;
      const int32_t st = rls_fista_gram_iteration(ctx, dtype, P, parity);
      parity ^= 1;
      return st;
    };
    if (ctx->tune.graph_chunk % 2) {
      for (int i = 0; i < n_steps; ++i) RLS_TRY(one());
    } else {
      RLS_TRY(run_steps(ctx, &s->graph, n_steps, one, [&parity, &k](int c) { parity ^= c & 1; k -= c; }));
    }
    s->enq += n_steps;
    return rls_fista_gram_finish(ctx, dtype, P, n_steps & 1);
  }
  if (fista_use_resident(s) && n_steps != 1) {  // (a single iteration: the pipeline, as in rls_cgnr_step)
    // the whole call as ONE launch, A held in registers (normal.hip, fista_resident_kernel)
    if (n_steps == 0) return 0;
    const rls_fista_pipe P = fista_pipe_desc(s);
    s->enq += n_steps;
    return s->resident.launch(ctx, [&](void* sync, unsigned spin) {
      return rls_fista_resident_launch(ctx, s->op->dtype, P, sync, n_steps, spin);
    });
  }
  if (s->use_pipe) {
    // iteration k = K_A (applies the gradient/prox/momentum update k-1 in its prologue, then one pass
    // over A for AHA y) + K_R (sums the partial rows); the last update of this call is applied by K_F
    rls_fista_pipe P = fista_pipe_desc(s);
    const int32_t dtype = s->op->dtype;
    // buffer hints: launch k >= 1 of this call finds iteration count enq + k - 1 (launch 0 applies nothing); the
    // hints a cached graph carries belong to the parity of `enq` it was captured with
    const int it0 = s->enq;
    s->graph.keep_for(it0 & 1);
    int k = 0;
    RLS_TRY(run_steps(ctx, &s->graph, n_steps, [ctx, dtype, &P, &k, it0]() {
      const int h = pipe_cur_hint(ctx, k);  // -1 where the position may be replayed out of sequence
      P.par_hint = h < 0 ? -1 : ((it0 + (k > 0 ? k - 1 : 0)) & 1);
      if (h >= 0 && ctx->tune.pipe_hint_mode == 2) P.par_hint ^= 1;  // tests: exercise the check-and-reload path
      ++k;
      return rls_fista_pipe_iteration(ctx, dtype, P);
    }, [&k](int c) { k -= c; }));
    s->enq += n_steps;
    P.mb = s->mb_arm;
    s->mb_sent = s->mb_arm.dst != nullptr;
    return rls_fista_pipe_finish(ctx, dtype, P);
  }
  return run_steps(ctx, &s->graph, n_steps, [s]() { return fista_enqueue_iteration(s); });
}

// status read-back of a single-column plan; re-runs on the per-iteration pipeline whatever a lost resident launch left
// undone (cgnr_fetch_status)
static int32_t fista_fetch_status(rls_fista* s) {
  return status_read(s->op->ctx, s, s->sc_h, 1, [s](int32_t n) { return fista_step_impl(s, n); },
                     [s](long long at) { s->enq = (int)at; });  // the buffer-parity hints of the pipeline follow the device's count
}

extern "C" {

int32_t rls_fista_create(rls_operator* op, void* x, void* x0, void* xold, void* res, rls_fista** out) {
  if (!op) return RLS_E_INVALID;
  rls_ctx* ctx = op->ctx;
  if (!x || !x0 || !xold || !res || !out) return rls_fail(ctx, RLS_E_INVALID, "fista_create: null pointer");
  RLS_HIP(ctx, rls_enter(ctx));
  *out = nullptr;
  rls_alloc_scope alloc_scope(ctx);
  rls_fista* s = new rls_fista{plan_memory(ctx)};
  plan_buffers& mem = s->mem;
  s->op = op;
  s->actx = ctx;
  s->actx_id = ctx->id;
  s->device = op->ctx->device;
  s->buf[0] = x;
  s->buf[1] = xold;
  s->x0 = x0;
  s->res = res;
  s->small = op->A && !op->G && rls_small_ok(op->dtype, op->M, op->N, op->A, op->lda);
  if (s->small) server_ctl_optional(mem, &s->srv);  // (server mode of the single-workgroup kernel)
  const size_t vb = (size_t)op->N * rls_elem_size(op->dtype);
  mem.dev(&s->y, vb, false);
  const bool gram = op->G && rls_gram_pipe_ok(op->dtype, op->N, op->G, op->ldg);
  if (gram) mem.dev(&s->res_raw1, vb, true);
  if (op->slab || gram) {
    mem.dev(&s->y1, vb, true);
    mem.dev(&s->res_raw, 2 * vb, true);  // (second half: state.res of the iteration a listening kernel runs ahead, fista_resident_kernel's SPEC)
    mem.dev(&s->scn, sizeof(fista_scalars), true);
  }
  if (!mem.error() && ((op->slab && op->A && !op->G && rls_cgnr_resident_ok(ctx, op->dtype, op->M, op->N, op->A, op->lda)) ||
                       (gram && rls_gram_resident_ok(ctx, op->dtype, op->N, op->G, op->ldg)))) {
    const plan_buffers::mark_t m = mem.mark();
    s->resident.alloc(mem, ctx, op);
    if (mem.error()) {
      mem.rollback(m);  // resident mode is an optimisation: without its scratch the pipeline runs
      (void)hipGetLastError();
    } else if ((!gram || rls_gram_resident_server_ok(op->dtype, op->N)) && (s->srv.ctl || server_ctl_optional(mem, &s->srv))) {
      s->srv.resident_used = &s->resident.used;  // (both resident kernels can stay and listen)
    }
  }
  alloc_scalars(mem, &s->sc, &s->sc_h);
  if (const int e = mem.error()) {
    rls_fista_destroy(s);
    return rls_fail(ctx, e, "fista_create: hipMalloc failed");
  }
  *out = s;
  return 0;
}

int32_t rls_fista_destroy(rls_fista* s) {
  if (!s) return RLS_E_INVALID;
  if (rls_ctx_alive(s->actx, s->actx_id) && s->actx->server == &s->srv) rls_server_stop(s->actx);  // (a kernel of this plan left listening)
  hipSetDevice(s->device);
  rls_alloc_scope alloc_scope(alloc_ctx_of(s->actx, s->actx_id));
  s->graph.drop();
  s->mem.release();
  delete s;
  return 0;
}

// A cached graph of this plan's iteration holds the kernel SEQUENCE of its regulariser and, for TV, the threshold rho * lambda, the
// image geometry and iterationsTV as kernel arguments (every other regulariser reads rho and lambda from the scalars on the device):
// whatever changes one of them drops the graph (step_graph::drop), the next step call captures afresh.

int32_t rls_fista_set_reg(rls_fista* s, int32_t reg_kind, float lambda, int64_t l21_slices, int32_t proj_kind) {
  if (!s) return RLS_E_INVALID;
  rls_ctx* ctx = s->op->ctx;
  if (reg_kind == RLS_REG_TV)
    return rls_fail(ctx, RLS_E_UNSUPPORTED, "fused FISTA: TV prox is not fused; drive FISTA from the primitives");
  if (reg_kind < RLS_REG_NONE || reg_kind > RLS_REG_L21 || proj_kind < RLS_PROJ_NONE || proj_kind > RLS_PROJ_POSITIVE)
    return rls_fail(ctx, RLS_E_INVALID, "fista_set_reg: unknown kind");
  if (reg_kind == RLS_REG_L21 && (l21_slices <= 0 || s->op->N / l21_slices == 0))
    return rls_fail(ctx, RLS_E_INVALID, "fista_set_reg: slices must be in 1..N");
  if (s->reg_kind == RLS_REG_TV || reg_kind != s->reg_kind) s->graph.drop();  // another kernel sequence (or TV's baked arguments)
  s->wav = nullptr;
  s->reg_kind = reg_kind;
  s->proj_kind = proj_kind;
  s->lambda = lambda;
  s->l21_slices = l21_slices > 0 ? l21_slices : 1;
  return 0;
}

// FISTA with prox!(::TVRegularization) (src/FISTA.jl:164 -> src/proximalMaps/ProxTV.jl:64-125): the FGP loop is one
// single-workgroup launch between the two halves of the update, for images that fit one workgroup (rls_tv_single_ok: 1-D / 2-D
// images of up to 8192 Float32 / 4096 ComplexF32 pixels, other geometries up to 2048); single right-hand side.  The plan then
// runs on the two-product path (operator apply, update half, FGP, update half); row-sharded plans (rls_fista_step_local_b,
// rls_fista_step_rowsharded) take the same three launches behind their all-reduce.
int32_t rls_fista_set_reg_tv(rls_fista* s, float lambda, int32_t ndims, const int64_t* shape, int32_t ntv, const int32_t* dims,
                             int32_t iterations_tv, int32_t proj_kind) {
  if (!s) return RLS_E_INVALID;
  rls_ctx* ctx = s->op->ctx;
  if (proj_kind < RLS_PROJ_NONE || proj_kind > RLS_PROJ_POSITIVE || iterations_tv < 0 || ndims < 1 || ndims > 4 || ntv < 0 || ntv > 4 ||
      !shape || (ntv > 0 && !dims))
    return rls_fail(ctx, RLS_E_INVALID, "fista_set_reg_tv: bad argument");
  int64_t n = 1;
  for (int k = 0; k < ndims; ++k) n *= shape[k];
  if (n != s->op->N) return rls_fail(ctx, RLS_E_INVALID, "fista_set_reg_tv: prod(shape) != N");
  if (s->nrhs != 1) return rls_fail(ctx, RLS_E_UNSUPPORTED, "fista_set_reg_tv: single right-hand side plans only");
  if (!rls_tv_single_ok(s->op->ctx, s->op->dtype, ndims, shape, ntv, dims))
    return rls_fail(ctx, RLS_E_UNSUPPORTED, "fista_set_reg_tv: the image does not fit the single-workgroup FGP kernel; drive FISTA from the primitives");
  RLS_HIP(ctx, rls_enter(ctx));
  if (!s->tv_in) {  // both or neither
    rls_alloc_scope alloc_scope(ctx);
    const size_t bytes = (size_t)s->op->N * rls_elem_size(s->op->dtype);
    const plan_buffers::mark_t m = s->mem.mark();
    s->mem.dev(&s->tv_in, bytes, false);
    s->mem.dev(&s->tv_out, bytes, false);
    if (const int e = s->mem.error()) {
      s->mem.rollback(m);
      return rls_fail(ctx, e, "fista_set_reg_tv: allocation failed");
    }
  }
  // lambda, the geometry and iterationsTV are arguments of the captured FGP launch: a cached graph survives only an identical call
  bool same = s->reg_kind == RLS_REG_TV && s->lambda == lambda && s->tv_iters == iterations_tv && s->tv_ndims == ndims &&
              s->tv_ntv == ntv && s->proj_kind == proj_kind;
  for (int k = 0; k < 4 && same; ++k)
    same = s->tv_shape[k] == (k < ndims ? shape[k] : 1) && s->tv_dims[k] == (k < ntv ? dims[k] : 0);
  if (!same) s->graph.drop();
  s->tv_ndims = ndims;
  s->tv_ntv = ntv;
  for (int k = 0; k < 4; ++k) {
    s->tv_shape[k] = k < ndims ? shape[k] : 1;
    s->tv_dims[k] = k < ntv ? dims[k] : 0;
  }
  s->tv_iters = iterations_tv;
  s->reg_kind = RLS_REG_TV;
  s->proj_kind = proj_kind;
  s->lambda = lambda;
  s->l21_slices = 1;
  s->wav = nullptr;
  return 0;
}

// FISTA with prox!(TransformedRegularization(L1Regularization, WaveletOp)): x <- W^T soft(W x, rho lambda) is the single-workgroup
// launch of wavelet.hip between the two halves of the update, in the place and under the rules of the FGP launch above (single
// right-hand side; the threshold is a launch argument, so a cached graph survives only an identical call).
int32_t rls_fista_set_reg_wavelet(rls_fista* s, rls_wavelet* w, float lambda, int32_t proj_kind) {
  if (!s) return RLS_E_INVALID;
  rls_ctx* ctx = s->op->ctx;
  if (!w || proj_kind < RLS_PROJ_NONE || proj_kind > RLS_PROJ_POSITIVE) return rls_fail(ctx, RLS_E_INVALID, "fista_set_reg_wavelet: bad argument");
  if (s->nrhs != 1) return rls_fail(ctx, RLS_E_UNSUPPORTED, "fista_set_reg_wavelet: single right-hand side plans only");
  if (!rls_wavelet_single_ok(w, ctx, s->op->dtype, s->op->N))
    return rls_fail(ctx, RLS_E_UNSUPPORTED, "fista_set_reg_wavelet: the image does not take the single-workgroup wavelet kernel (or the handle is of another "
                                            "context, element type or length); drive FISTA from the primitives");
  RLS_HIP(ctx, rls_enter(ctx));
  if (!s->tv_in) {  // both or neither (the blocks the TV launch uses)
    rls_alloc_scope alloc_scope(ctx);
    const size_t bytes = (size_t)s->op->N * rls_elem_size(s->op->dtype);
    const plan_buffers::mark_t m = s->mem.mark();
    s->mem.dev(&s->tv_in, bytes, false);
    s->mem.dev(&s->tv_out, bytes, false);
    if (const int e = s->mem.error()) {
      s->mem.rollback(m);
      return rls_fail(ctx, e, "fista_set_reg_wavelet: allocation failed");
    }
  }
  // the handle's filter, extents and depth, lambda and rho are arguments of the captured launch: a cached graph survives only a call
  // with the very same handle (by serial number: addresses are reused), lambda and projection
  const uint64_t serial = rls_wavelet_serial(w);
  if (!(s->reg_kind == RLS_REG_WAVELET && s->wav == w && s->wav_serial == serial && s->lambda == lambda && s->proj_kind == proj_kind))
    s->graph.drop();
  s->wav = w;
  s->wav_serial = serial;
  s->reg_kind = RLS_REG_WAVELET;
  s->proj_kind = proj_kind;
  s->lambda = lambda;
  s->l21_slices = 1;
  return 0;
}

// x0 = A^H b (src/FISTA.jl:114); on a row shard this is the partial sum the caller all-reduces
int32_t rls_fista_init_local_a(rls_fista* s, const void* b) {
  if (!s) return RLS_E_INVALID;
  rls_operator* op = s->op;
  rls_ctx* ctx = op->ctx;
  if (!b) return rls_fail(ctx, RLS_E_INVALID, "fista_init: null b");
  RLS_HIP(ctx, rls_enter(ctx));
  if (op->A)
    RLS_TRY(rls_launch_gemv(ctx, op->dtype, RLS_OP_C, op->M, op->N, 1.f, 0.f, op->A, op->lda, b, 0.f, 0.f, s->x0, nullptr));
  else
    RLS_HIP(ctx, hipMemcpyAsync(s->x0, b, (size_t)op->N * rls_elem_size(op->dtype), hipMemcpyDeviceToDevice, ctx->stream));
  return 0;
}

int32_t rls_fista_init(rls_fista* s, const void* b, float rho, float theta, float rel_tol, int32_t iterations,
                       int32_t restart_gradient) {
  RLS_TRY(rls_fista_init_local_a(s, b));
  return fista_init_finish(s, rho, theta, rel_tol, iterations, restart_gradient, false);
}

int32_t rls_fista_init_local_b(rls_fista* s, float rho, float theta, float rel_tol, int32_t iterations,
                               int32_t restart_gradient) {
  if (!s) return RLS_E_INVALID;
  return fista_init_finish(s, rho, theta, rel_tol, iterations, restart_gradient, true);
}

// one row-sharded iteration: res_partial = A_g^H A_g y ; [caller: all-reduce(res)] ; gradient step, prox, momentum
int32_t rls_fista_step_local_a(rls_fista* s) {
  if (!s) return RLS_E_INVALID;
  rls_ctx* ctx = s->op->ctx;
  if (!s->initialised || s->use_pipe || s->use_gram) return rls_fail(ctx, RLS_E_STATE, "fista_step_local before fista_init_local_b");
  RLS_HIP(ctx, rls_enter(ctx));
  return op_normal(s->op, s->y, s->res, &s->sc->done);
}
int32_t rls_fista_step_local_b(rls_fista* s) {
  if (!s) return RLS_E_INVALID;
  rls_operator* op = s->op;
  rls_ctx* ctx = op->ctx;
  if (!s->initialised || s->use_pipe || s->use_gram) return rls_fail(ctx, RLS_E_STATE, "fista_step_local before fista_init_local_b");
  RLS_HIP(ctx, rls_enter(ctx));
  RLS_TRY(rls_with_elem(op->dtype, [&](auto t) {
    using E = typename decltype(t)::type;
    return fista_launch_update<E>(s, 1, col_batch<E>());
  }));
  return launch_status(ctx);
}

// K right-hand sides sharing A (solve!(solver, B) of src/MultiThreading.jl:30-79 for FISTA): per-column scalars,
// per-column retirement, the two products as skinny GEMMs on the matrix cores.
int32_t rls_fista_create_batched(rls_operator* op, int32_t nrhs, void* x, void* x0, void* xold, void* res, int64_t ldv,
                                 rls_fista** out) {
  if (!op) return RLS_E_INVALID;
  rls_ctx* ctx = op->ctx;
  if (!x || !x0 || !xold || !res || !out || nrhs < 1 || ldv < op->N)
    return rls_fail(ctx, RLS_E_INVALID, "fista_create_batched: bad argument");
  if (!ctx->tune.batched_mfma || !shared_operands::supported(op))
    return rls_fail(ctx, RLS_E_UNSUPPORTED, "batched FISTA needs A (and AHA, when explicit) with 16-aligned M, N (matrix-core path)");
  RLS_HIP(ctx, rls_enter(ctx));
  *out = nullptr;
  rls_alloc_scope alloc_scope(ctx);
  rls_fista* s = new rls_fista{plan_memory(ctx)};
  plan_buffers& mem = s->mem;
  s->op = op;
  s->actx = ctx;
  s->actx_id = ctx->id;
  s->device = ctx->device;
  s->buf[0] = x;
  s->buf[1] = xold;
  s->x0 = x0;
  s->res = res;
  s->nrhs = nrhs;
  s->ldv = ldv;
  mem.dev(&s->y, (size_t)ldv * nrhs * rls_elem_size(op->dtype), false);
  s->ops.alloc(mem, op, nrhs);
  mem.dev(&s->sc, sizeof(fista_scalars) * nrhs, true);
  mem.pinned(&s->scb_h, sizeof(fista_scalars) * nrhs, false);
  mem.pinned(&s->sc_h, sizeof(fista_scalars), false);
  const bool vec16 = ldv % 2 == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(xold) | reinterpret_cast<uintptr_t>(res)) & 15) == 0;
  if (!mem.error() && op->G && s->ops.half && vec16 && rls_fgramk_resident_ok(ctx, op->dtype, op->N, nrhs, op->G, op->ldg)) {
    size_t yxb, xxb, db;
    rls_fgramk_sizes(op->N, &yxb, &xxb, &db);
    s->resident.alloc(mem, ctx, op);
    mem.dev(&s->fk_yx, yxb, true);  // rows >= N are read, never written
    mem.dev(&s->fk_xx, xxb, false);
    mem.dev(&s->fk_dots, db, true);  // slots of absent workgroups add 0.0
    s->fgramk = !mem.error();
  }
  if (const int e = mem.error()) {
    rls_fista_destroy(s);
    return rls_fail(ctx, e, "fista_create_batched: allocation failed");
  }
  *out = s;
  return 0;
}

int32_t rls_fista_init_batched(rls_fista* s, const void* B, int64_t ldb, float rho, float theta, float rel_tol,
                               int32_t iterations, int32_t restart_gradient) {
  if (!s) return RLS_E_INVALID;
  rls_operator* op = s->op;
  rls_ctx* ctx = op->ctx;
  if (s->nrhs < 2 && !s->ops.allocated()) return rls_fail(ctx, RLS_E_STATE, "fista_init_batched on a single-column plan");
  if (!B || ldb < op->M) return rls_fail(ctx, RLS_E_INVALID, "fista_init_batched: bad argument");
  RLS_HIP(ctx, rls_enter(ctx));
  RLS_TRY(rls_skinny_atb(ctx, op->dtype, fista_skinny_desc(s), B, ldb));  // partial rows of A^H B   (src/FISTA.jl:114)
  // (the resident launch's arrival counters are zeroed by the init kernel: every workgroup writes the same zeros)
  const int n_clear = s->resident.sync ? (int)(rls_resident_sync_clear_bytes() / sizeof(unsigned)) : 0;
  rls_with_elem(op->dtype, [&](auto t) {
    using E = typename decltype(t)::type;
    hipLaunchKernelGGL(fista_init_kernel<E>, dim3((unsigned)s->nrhs), dim3(UPD_THREADS), 0, ctx->stream, (E*)s->buf[0],
                       (E*)s->buf[1], (E*)s->x0, (E*)s->res, (E*)s->y, op->N, s->sc, rho, theta, rel_tol, iterations,
                       restart_gradient, s->reg_kind, s->proj_kind, s->lambda, (long long)s->l21_slices, fista_batch_desc<E>(s),
                       (unsigned*)s->resident.sync, n_clear);
  });
  s->initialised = true;
  s->use_pipe = s->use_gram = false;
  s->restart_b = restart_gradient;
  s->resident.clean = s->resident.sync != nullptr;
  s->requested = 0;
  s->enq = 0;
  s->resident.used = false;
  return launch_status(ctx);
}

int32_t rls_fista_get_status_batched(rls_fista* s, rls_fista_status* out) {
  if (!s || !out) return RLS_E_INVALID;
  rls_ctx* ctx = s->op->ctx;
  if (!s->initialised || !s->scb_h) return rls_fail(ctx, RLS_E_STATE, "fista_get_status_batched: not a batched, initialised plan");
  RLS_HIP(ctx, rls_enter(ctx));
  RLS_TRY(status_read(ctx, s, s->scb_h, s->nrhs, [s](int32_t n) { return fista_step_impl(s, n); }, [](long long) {}));
  for (int b = 0; b < s->nrhs; ++b) fista_status_out(s, s->scb_h[b], out + b);
  return 0;
}

int32_t rls_fista_set_start(rls_fista* s, const void* x_init, int64_t n) {
  if (!s) return RLS_E_INVALID;
  rls_ctx* ctx = s->op->ctx;
  if (!s->initialised) return rls_fail(ctx, RLS_E_STATE, "fista_set_start before fista_init");
  if (!x_init) return rls_fail(ctx, RLS_E_INVALID, "fista_set_start: null pointer");
  if (n != s->op->N) return rls_fail(ctx, RLS_E_INVALID, "fista_set_start: x_init must have the solution's length N");
  if (s->nrhs != 1) return rls_fail(ctx, RLS_E_UNSUPPORTED, "fista_set_start on a batched plan");
  RLS_HIP(ctx, rls_enter(ctx));
  const size_t bytes = (size_t)s->op->N * rls_elem_size(s->op->dtype);
  // iteration 0: state.x == buf[0], xold == 0; the first extrapolated point (src/FISTA.jl:147-148 with
  // thetaold == theta) is ((theta - 1) / theta + 1) x0 -- x0 itself only for the default theta = 1
  RLS_HIP(ctx, hipMemcpyAsync(s->buf[0], x_init, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  const float c2 = (s->theta0 - 1.f) / s->theta0 + 1.f;
  return rls_lincomb(ctx, s->op->dtype, n, c2, 0.f, x_init, 0.f, 0.f, x_init, s->y);
}

int32_t rls_fista_step(rls_fista* s, int32_t n_steps) {
  if (!s) return RLS_E_INVALID;
  rls_ctx* ctx = s->op->ctx;
  if (!s->initialised) return rls_fail(ctx, RLS_E_STATE, "fista_step before fista_init");
  if (n_steps < 0) return rls_fail(ctx, RLS_E_INVALID, "fista_step: n_steps < 0");
  RLS_HIP(ctx, rls_enter(ctx));
  s->requested += n_steps;
  return fista_step_impl(s, n_steps);
}

int32_t rls_fista_path(rls_fista* s, int32_t* out) {
  if (!s || !out) return RLS_E_INVALID;
  *out = fista_use_small(s) ? 8 : s->nrhs > 1 ? (fista_use_gramk(s, 0) ? 7 : 3) : fista_use_gram_resident(s) ? 5 : s->use_gram ? 2 : fista_use_resident(s) ? 4 : s->use_pipe ? 1 : 0;
  return 0;
}

int32_t rls_fista_get_status(rls_fista* s, rls_fista_status* out) {
  if (!s || !out) return RLS_E_INVALID;
  rls_ctx* ctx = s->op->ctx;
  if (!s->initialised) return rls_fail(ctx, RLS_E_STATE, "fista_get_status before fista_init");
  if (ctx->server == &s->srv && s->srv.alive && s->srv.fresh) {  // a kernel left listening: the mirror holds its last command's status
    fista_status_out(s, *s->sc_h, out);
    return 0;
  }
  RLS_HIP(ctx, rls_enter(ctx));
  RLS_TRY(fista_fetch_status(s));
  fista_status_out(s, *s->sc_h, out);
  return 0;
}

int32_t rls_fista_step_status(rls_fista* s, int32_t n_steps, rls_fista_status* out) {  // as rls_cgnr_step_status
  if (!s || !out) return RLS_E_INVALID;
  rls_ctx* ctx = s->op->ctx;
  auto serve_launch = [&](const rls_srv_args& a) {
    rls_fista_pipe P = fista_pipe_desc(s);
    if (fista_use_small(s)) {  // the single-workgroup kernel: one CU stays, nothing to chain
      if (!P.y1) P.y1 = P.y0;
      P.mb = a.mb;
      return rls_fista_small_launch(ctx, s->op->dtype, P, n_steps, a);
    }
    rls_srv_args ar = a;  // (the resident kernels take the idle time as it is: the run-ahead choice is their instantiation)
    ar.idle_us &= ~RLS_SRV_AHEAD;
    if (fista_use_gram_resident(s)) {  // AHA explicit, in the register files (fista_gram_resident_kernel)
      const rls_fista_gram Pg = fista_gram_desc(s);
      return s->resident.chain(ctx, [&](void* sync, unsigned spin) {
        return rls_fista_gram_resident_launch(ctx, s->op->dtype, Pg, sync, n_steps, spin, ar);
      });
    }
    return s->resident.chain(ctx, [&](void* sync, unsigned spin) {
      return rls_fista_resident_launch(ctx, s->op->dtype, P, sync, n_steps, spin, ar);
    });
  };
  const bool serve = server_usable(ctx, &s->srv) && (fista_use_small(s) || fista_use_gram_resident(s) || fista_use_resident(s));
  return step_status(s, n_steps, out, serve, serve_launch, [s](int32_t n) { s->requested += n; s->enq += n; }, rls_fista_step,
                     rls_fista_get_status, fista_status_out);
}

int32_t rls_fista_solution(rls_fista* s, void** x_out) {
  if (!s || !x_out) return RLS_E_INVALID;
  rls_ctx* ctx = s->op->ctx;
  if (!s->initialised) return rls_fail(ctx, RLS_E_STATE, "fista_solution before fista_init");
  RLS_HIP(ctx, rls_enter(ctx));
  RLS_TRY(fista_fetch_status(s));
  *x_out = s->buf[s->sc_h->iteration & 1];
  return 0;
}

// FISTA on a row-partitioned A (src/FISTA.jl:110-185): x0 = sum_g A_g^H b_g at init, res_g = A_g^H A_g y per iteration;
// gradient step, prox, momentum and `done` replicated.  plans[r]: rls_fista_create on rank r's shard operator (+ set_reg).
int32_t rls_fista_init_rowsharded(rls_comm* comm, rls_fista* const* plans, const void* const* b_parts, float rho, float theta,
                                  float rel_tol, int32_t iterations, int32_t restart_gradient) {
  RLS_TRY(rowsharded_check<rls_fista>(comm, plans, fista_op, fista_single));
  if (!b_parts) return RLS_E_INVALID;
  const int64_t N = plans[0]->op->N;
  const int32_t dtype = plans[0]->op->dtype;
  int round0 = 0;
  RLS_TRY(rls_comm_next_rounds(comm, 1, N, dtype, &round0));
  const std::vector<rls_comm_phase> phases = {
      {[&](int r, int) {
         RLS_TRY(rls_fista_init_local_a(plans[r], b_parts[r]));
         return rls_comm_publish(comm, r, plans[r]->x0, N, dtype, round0);
       }, true},
      {[&](int r, int) {
         RLS_TRY(rls_comm_collect(comm, r, plans[r]->x0, N, dtype, round0));
         return rls_fista_init_local_b(plans[r], rho, theta, rel_tol, iterations, restart_gradient);
       }, false}};
  return rls_comm_run(comm, phases, 1);
}

int32_t rls_fista_step_rowsharded(rls_comm* comm, rls_fista* const* plans, int32_t n_steps) {
  RLS_TRY(rowsharded_check<rls_fista>(comm, plans, fista_op, fista_single));
  if (n_steps < 0) return RLS_E_INVALID;
  const int64_t N = plans[0]->op->N;
  const int32_t dtype = plans[0]->op->dtype;
  int round0 = 0;
  RLS_TRY(rls_comm_next_rounds(comm, n_steps, N, dtype, &round0));
  const std::vector<rls_comm_phase> phases = {
      {[&](int r, int k) {
         RLS_TRY(rls_fista_step_local_a(plans[r]));
         return rls_comm_publish(comm, r, plans[r]->res, N, dtype, round0 + k);
       }, true},
      {[&](int r, int k) {
         RLS_TRY(rls_comm_collect(comm, r, plans[r]->res, N, dtype, round0 + k));
         return rls_fista_step_local_b(plans[r]);
       }, false}};
  return rls_comm_run(comm, phases, n_steps);
}

}  // extern "C"
