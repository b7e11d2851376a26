// CGNR (src/CGNR.jl:107-185) and IterativeSolvers.cg! as ADMM calls it (src/ADMM.jl:244), with the ADMM / SplitBregman plan
// that owns a cg plan: the device plans, their kernels and entry points.  What they share with the other plans is plans.hpp.
#include "plans.hpp"

// ---------------------------------------------------------------------------------------------
// CGNR
// ---------------------------------------------------------------------------------------------
struct rls_cgnr {
  plan_buffers mem;  // owns every block below, srv.ctl and resident.{sync, flags_h} included
  rls_operator* op = nullptr;
  rls_ctx* actx = nullptr;  // the context whose pool the plan's scratch came from (checked alive before it is used in destroy)
  uint64_t actx_id = 0;
  int device = 0;
  void *x = nullptr, *r = nullptr, *p = nullptr, *v = nullptr;
  cgnr_scalars* sc = nullptr;    // device
  cgnr_scalars* sc_h = nullptr;  // pinned host
  step_graph graph;
  bool initialised = false;
  // fused pipeline (normal.hip): alternate (r, p) pair, partial dots, staged scalars
  void *r1 = nullptr, *p1 = nullptr;
  double* dots = nullptr;
  double* ttw = nullptr;
  cgnr_scalars* scn = nullptr;
  // batched plans: nrhs right-hand sides, columns ldv elements apart, own partial-row slab
  int nrhs = 1;
  int64_t ldv = 0;
  void* slab_b = nullptr;
  // Gram-mode pipeline (normal.hip): one launch per iteration, second parity of v and the partial dots
  bool gram_pipe = false;
  void* v1 = nullptr;
  double* gdots = nullptr;
  // batched plans on the matrix cores (skinny.hip): packed operands + row-split partials
  bool skinny = false;
  shared_operands ops;
  // resident mode (normal.hip, cgnr_resident_kernel): sync block + lost-launch bookkeeping, per-workgroup partial dots
  resident_slot resident;
  double* rdots = nullptr;
  rls_mailbox_slot mb_arm;  // step_status: the call's last kernel publishes the scalars (pipeline and small-system paths)
  srv_state srv;  // server mode of the resident kernel (rls_cgnr_step_status)
  bool mb_sent = false;     // ... and this call's path did take the slot
  bool gram_resident = false;  // Gram mode: AHA fits the register files (rls_gram_resident_ok)
  long long requested = 0;  // iterations asked for since init (what a lost launch did not run: requested - the device's count)
  bool small = false;  // the system fits one CU's registers: a step call is ONE single-workgroup launch (small.hip)
  // batched plan on an explicit Gram matrix, <= 8 ComplexF32 columns, AHA in the register files (gramk.hip): exchange scratch
  bool gramk = false;
  float* gk_vx = nullptr;
  void* gk_xx = nullptr;
  double* gk_dots = nullptr;
  // rls_cgnr_solve_queue_host: this problem's right-hand side on the device and the pinned staging of b and x (created on first use)
  void* q_b = nullptr;
  void* q_bh = nullptr;
  void* q_xh = nullptr;
  // queue mode (cgnr_use_queue): the control block has room for the command ring; ctx->syncs at the plan's last resident step call
  bool q_ok = false;
  uint64_t q_mark = ~0ull;
};

static bool cgnr_use_gram_pipeline(const rls_cgnr* s) {
  return s->gram_pipe && s->op->G && s->op->ctx->tune.gram_pipeline;
}

static rls_gram_pipe cgnr_gram_desc(const rls_cgnr* s) {
  return gram_pipe_desc(s->op, s->x, s->r, s->r1, s->p, s->p1, s->v, s->v1, s->gdots, s->sc, s->scn);
}

static rls_skinny cgnr_skinny_desc(const rls_cgnr* s) {
  rls_skinny K = s->ops.desc(s->op, s->nrhs, s->ldv);
  K.X = s->x;
  K.R = s->r;
  K.P = s->p;
  K.V = s->v;
  K.sc = s->sc;
  return K;
}

// small systems: single right-hand side, matrix-free, A in ONE CU's registers for the whole step call (no grid exchange, no
// co-residency requirement: always available)
static bool cgnr_use_small(const rls_cgnr* s) {
  return s->small && s->nrhs == 1 && !s->op->G && s->op->ctx->tune.small && s->op->ctx->tune.resident;
}

// batched Gram mode as ONE resident launch per step call (a call of one iteration -- the callback cadence -- is cheaper on
// the streaming kernels: a resident launch loads its rows of AHA and gathers x once per call)
static bool cgnr_use_gramk(const rls_cgnr* s, int n_steps) {
  return s->gramk && s->resident.usable(s->op->ctx) &&
         (n_steps != 1 || s->op->ctx->tune.resident == 2);  // resident = 2 (tools, tests): single-iteration calls too
}

static rls_gramk cgnr_gramk_desc(const rls_cgnr* s) {
  rls_gramk D;
  D.G = s->op->G;
  D.ldg = s->op->ldg;
  D.N = s->op->N;
  D.nrhs = s->nrhs;
  D.X = s->x;
  D.R = s->r;
  D.P = s->p;
  D.V = s->v;
  D.ldv = s->ldv;
  D.sc = s->sc;
  D.Vx = s->gk_vx;
  D.Xx = s->gk_xx;
  D.dots = s->gk_dots;
  D.Ppack = s->ops.half ? s->ops.panel : nullptr;  // (<= 8 complex columns: the half layout, unless switched off by the tools)
  return D;
}

static bool cgnr_use_gram_resident(const rls_cgnr* s) {
  return s->gram_resident && s->resident.usable(s->op->ctx) && s->nrhs == 1 && cgnr_use_gram_pipeline(s);
}

static bool cgnr_use_pipeline(const rls_cgnr* s) {
  const rls_ctx* ctx = s->op->ctx;
  return s->r1 && s->op->slab && !s->op->G && ctx->tune.fused_normal && ctx->tune.cgnr_pipeline;
}

// the whole step call as one launch: single right-hand side, matrix-free, A small enough to stay in the register
// files (one workgroup per CU), 16-byte aligned state vectors
static bool cgnr_use_resident(const rls_cgnr* s) {
  return s->resident.usable(s->op->ctx) && s->nrhs == 1 && cgnr_use_pipeline(s) && aligned16(s->x, s->r, s->p, s->v);
}

static rls_cgnr_pipe cgnr_pipe_desc(const rls_cgnr* s) {
  rls_cgnr_pipe P = pipe_desc(s->op, s->x, s->r, s->r1, s->p, s->p1, s->v, s->dots, s->sc, s->scn);
  if (s->slab_b) P.slab = s->slab_b;
  P.ttw = s->ttw;
  P.nrhs = s->nrhs;
  P.vstride = s->ldv;
  return P;
}
// small systems (small.hip): the plan as the single-workgroup kernel sees it
static rls_small cgnr_small_desc(const rls_cgnr* s) {
  rls_small D;
  D.A = s->op->A;
  D.lda = s->op->lda;
  D.M = s->op->M;
  D.N = s->op->N;
  D.x = s->x;
  D.r = s->r;
  D.p = s->p;
  D.v = s->v;
  D.sc = s->sc;
  return D;
}

// after r = A^H b:  x = 0, v = 0, p = r, z0 = ||r||, scalars reset          (src/CGNR.jl:108-126)
template <typename E>
__global__ __launch_bounds__(UPD_THREADS) void cgnr_init_kernel(E* __restrict__ x, const E* __restrict__ r,
                                                                E* __restrict__ p, E* __restrict__ v, int64_t n,
                                                                cgnr_scalars* sc, float lambda, float rel_tol,
                                                                int max_iter, unsigned* clear_words = nullptr,
                                                                int n_clear = 0) {
  __shared__ double sm[16];
  // the arrival counters of the plan's resident kernel (resident_chain: saves the memset launch ahead of it)
  for (int i = threadIdx.x; i < n_clear; i += UPD_THREADS) clear_words[i] = 0u;
  double rr = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += UPD_THREADS) {
    const E ri = r[i];
    x[i] = elem<E>::zero();
    v[i] = elem<E>::zero();
    p[i] = ri;
    rr += (double)elem<E>::re(ri) * (double)elem<E>::re(ri) + (double)elem<E>::im(ri) * (double)elem<E>::im(ri);
  }
  rr = block_sum_n<UPD_THREADS / 64>(rr, sm);  // (constant wave count: no dispatch-packet read)
  if (threadIdx.x == 0) {
    sc->rr = rr;
    sc->z0 = sqrt(rr);
    sc->zeta = 0.0;
    sc->alpha_re = sc->alpha_im = sc->beta_re = sc->beta_im = 0.0;
    sc->lambda = lambda;
    sc->rel_tol = rel_tol;
    sc->iteration = 0;
    sc->max_iter = max_iter;
    sc->pending = 0;
    sc->cur = 0;
    sc->fresh = 0;
    // done() evaluated before the first iteration: ||r||/z0 <= relTol || 0 >= min(iterations, N)
    const float ratio = (float)(sqrt(rr) / sqrt(rr));  // NaN when r == 0, as in the reference
    sc->done = (ratio <= rel_tol) || (0 >= max_iter);
  }
}

// the BLAS-1 part of one CGNR iteration, src/CGNR.jl:153-176, after v = AHA p
template <typename E>
__global__ __launch_bounds__(UPD_THREADS) void cgnr_update_kernel(E* __restrict__ x, E* __restrict__ r,
                                                                  E* __restrict__ p, const E* __restrict__ v,
                                                                  int64_t n, cgnr_scalars* sc) {
  if (sc->done) return;
  __shared__ double sm[16];
  const float lambda = sc->lambda;
  const double zeta = sc->rr;  // zeta = ||r||^2                                        :153
  // normvl = <p, v> (conjugating, complex-typed) and ||p||^2                           :154,158
  double nre = 0.0, nim = 0.0, pp = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += UPD_THREADS) {
    const E pi = p[i], vi = v[i];
    nre += (double)elem<E>::re(pi) * (double)elem<E>::re(vi) + (double)elem<E>::im(pi) * (double)elem<E>::im(vi);
    if constexpr (elem<E>::cplx)
      nim += (double)elem<E>::re(pi) * (double)elem<E>::im(vi) - (double)elem<E>::im(pi) * (double)elem<E>::re(vi);
    if (lambda > 0.f)
      pp += (double)elem<E>::re(pi) * (double)elem<E>::re(pi) + (double)elem<E>::im(pi) * (double)elem<E>::im(pi);
  }
  nre = block_sum(nre, sm);
  if constexpr (elem<E>::cplx) nim = block_sum(nim, sm);
  if (lambda > 0.f) pp = block_sum(pp, sm);
  // alpha = zeta / (normvl + lambda ||p||^2)                                            :156-161
  dcomplex den = {nre + (lambda > 0.f ? (double)lambda * pp : 0.0), nim};
  dcomplex alpha = dc_div({zeta, 0.0}, den);
  const E a = elem<E>::make((float)alpha.re, (float)alpha.im);
  const E na = elem<E>::make(-(float)alpha.re, -(float)alpha.im);
  // x += alpha p ; r -= alpha v ; r -= lambda alpha p                                   :163-169
  double rr = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += UPD_THREADS) {
    const E pi = p[i];
    x[i] = elem<E>::fma(pi, a, x[i]);
    E ri = elem<E>::fma(v[i], na, r[i]);
    if (lambda > 0.f) ri = elem<E>::fma(elem<E>::scale(-lambda, pi), a, ri);
    r[i] = ri;
    rr += (double)elem<E>::re(ri) * (double)elem<E>::re(ri) + (double)elem<E>::im(ri) * (double)elem<E>::im(ri);
  }
  rr = block_sum(rr, sm);
  // beta = <r, r> / zeta ; p = beta p + r                                               :171-174
  const double beta = rr / zeta;
  const float bf = (float)beta;
  for (int64_t i = threadIdx.x; i < n; i += UPD_THREADS) p[i] = elem<E>::add(elem<E>::scale(bf, p[i]), r[i]);
  if (threadIdx.x == 0) {
    sc->zeta = zeta;
    sc->rr = rr;
    sc->alpha_re = alpha.re;
    sc->alpha_im = alpha.im;
    sc->beta_re = beta;
    sc->beta_im = 0.0;
    const int it = sc->iteration + 1;
    sc->iteration = it;
    const float ratio = (float)(sqrt(rr) / sc->z0);
    sc->done = (ratio <= sc->rel_tol) || (it >= sc->max_iter);  // :181-185
  }
}

// The same update with the four vectors held in registers (n <= EPT * UPD_THREADS): every load is requested before
// anything is waited for -- one memory round trip instead of the seven dependent ones of the loop form above
// (scalars, three passes over the vectors) -- and the same per-thread summation order, so the same bits.
template <typename E, int EPT>
__global__ __launch_bounds__(UPD_THREADS) void cgnr_update_reg_kernel(E* __restrict__ x, E* __restrict__ r,
                                                                      E* __restrict__ p, const E* __restrict__ v,
                                                                      int64_t n, cgnr_scalars* sc) {
  __shared__ double sm[48];
  const cgnr_scalars S = *sc;
  E pv[EPT], vv[EPT], xv[EPT], rv[EPT];
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const int64_t i = threadIdx.x + (int64_t)e * UPD_THREADS;
    const int64_t ic = i < n ? i : n - 1;
    pv[e] = p[ic];
    vv[e] = v[ic];
    xv[e] = x[ic];
    rv[e] = r[ic];
  }
  if (S.done) return;
  const float lambda = S.lambda;
  const double zeta = S.rr;
  double nre = 0.0, nim = 0.0, pp = 0.0;
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const int64_t i = threadIdx.x + (int64_t)e * UPD_THREADS;
    if (i >= n) pv[e] = vv[e] = rv[e] = elem<E>::zero();
    nre += (double)elem<E>::re(pv[e]) * (double)elem<E>::re(vv[e]) + (double)elem<E>::im(pv[e]) * (double)elem<E>::im(vv[e]);
    if constexpr (elem<E>::cplx)
      nim += (double)elem<E>::re(pv[e]) * (double)elem<E>::im(vv[e]) - (double)elem<E>::im(pv[e]) * (double)elem<E>::re(vv[e]);
    pp += (double)elem<E>::re(pv[e]) * (double)elem<E>::re(pv[e]) + (double)elem<E>::im(pv[e]) * (double)elem<E>::im(pv[e]);
  }
  block_sum3(nre, nim, pp, sm);
  const dcomplex den = {nre + (lambda > 0.f ? (double)lambda * pp : 0.0), nim};
  const dcomplex alpha = dc_div({zeta, 0.0}, den);
  const E a = elem<E>::make((float)alpha.re, (float)alpha.im);
  const E na = elem<E>::make(-(float)alpha.re, -(float)alpha.im);
  double rr = 0.0;
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    xv[e] = elem<E>::fma(pv[e], a, xv[e]);
    E ri = elem<E>::fma(vv[e], na, rv[e]);
    if (lambda > 0.f) ri = elem<E>::fma(elem<E>::scale(-lambda, pv[e]), a, ri);
    rv[e] = ri;
    rr += (double)elem<E>::re(ri) * (double)elem<E>::re(ri) + (double)elem<E>::im(ri) * (double)elem<E>::im(ri);
  }
  rr = block_sum(rr, sm);
  const double beta = rr / zeta;
  const float bf = (float)beta;
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const int64_t i = threadIdx.x + (int64_t)e * UPD_THREADS;
    if (i < n) {
      x[i] = xv[e];
      r[i] = rv[e];
      p[i] = elem<E>::add(elem<E>::scale(bf, pv[e]), rv[e]);
    }
  }
  if (threadIdx.x == 0) {
    sc->zeta = zeta;
    sc->rr = rr;
    sc->alpha_re = alpha.re;
    sc->alpha_im = alpha.im;
    sc->beta_re = beta;
    sc->beta_im = 0.0;
    const int it = S.iteration + 1;
    sc->iteration = it;
    const float ratio = (float)(sqrt(rr) / S.z0);
    sc->done = (ratio <= S.rel_tol) || (it >= S.max_iter);  // :181-185
  }
}

template <typename E>
static void cgnr_launch_init(rls_cgnr* s, float lambda, float rel_tol, int max_iter) {
  rls_operator* op = s->op;
  const bool clr = s->resident.sync && s->nrhs == 1;
  hipLaunchKernelGGL(cgnr_init_kernel<E>, dim3(1), dim3(UPD_THREADS), 0, op->ctx->stream, (E*)s->x, (const E*)s->r,
                     (E*)s->p, (E*)s->v, op->N, s->sc, lambda, rel_tol, max_iter, clr ? (unsigned*)s->resident.sync : nullptr,
                     clr ? (int)(rls_resident_sync_clear_bytes() / sizeof(unsigned)) : 0);
  s->resident.clean = clr;
}
template <typename E>
static void cgnr_launch_update(rls_cgnr* s) {
  rls_operator* op = s->op;
  const int64_t n = op->N;
#define RLS_UPD_REG(EE)                                                                                             \
  hipLaunchKernelGGL((cgnr_update_reg_kernel<E, EE>), dim3(1), dim3(UPD_THREADS), 0, op->ctx->stream, (E*)s->x, (E*)s->r, \
                     (E*)s->p, (const E*)s->v, n, s->sc)
  if (n <= UPD_THREADS) RLS_UPD_REG(1);
  else if (n <= 2 * UPD_THREADS) RLS_UPD_REG(2);
  else if (n <= 4 * UPD_THREADS) RLS_UPD_REG(4);
  else if (n <= 8 * UPD_THREADS) RLS_UPD_REG(8);
  else
    hipLaunchKernelGGL(cgnr_update_kernel<E>, dim3(1), dim3(UPD_THREADS), 0, op->ctx->stream, (E*)s->x, (E*)s->r,
                       (E*)s->p, (const E*)s->v, n, s->sc);
#undef RLS_UPD_REG
}

static int32_t cgnr_enqueue_update(rls_cgnr* s) {
  rls_with_elem(s->op->dtype, [&](auto t) { cgnr_launch_update<typename decltype(t)::type>(s); });
  return launch_status(s->op->ctx);
}

static int32_t cgnr_enqueue_iteration(rls_cgnr* s) {
  RLS_TRY(op_normal(s->op, s->p, s->v, &s->sc->done));
  return cgnr_enqueue_update(s);
}

static int32_t cgnr_effective_iterations(rls_cgnr* s, int32_t iterations) {
  // iteration >= min(solver.iterations, size(AHA, 2))    src/CGNR.jl:185
  int64_t m = iterations < s->op->N ? iterations : s->op->N;
  return (int32_t)(m < 0 ? 0 : m);
}

// ---------------------------------------------------------------------------------------------
// cg!  (IterativeSolvers v0.9 semantics, restated; see oracle/rls_oracle.py::cg_inplace)
// ---------------------------------------------------------------------------------------------
struct cg_scalars {
  double residual, prev, tol;
  float rho, reltol;
  int iteration, maxiter, done, pad;
};

struct rls_cg {
  plan_buffers mem;  // owns every block below, resident.{sync, flags_h} included
  rls_operator* op = nullptr;
  rls_ctx* actx = nullptr;
  uint64_t actx_id = 0;
  int device = 0;
  void *u = nullptr, *r = nullptr, *c = nullptr;
  cg_scalars* sc = nullptr;
  cg_scalars* sc_h = nullptr;
  // fused pipeline (normal.hip): cg! on (AHA + rho I) is the CGNR recurrence with lambda = rho and the
  // start residual b - (AHA + rho I) x0, so it reuses the two-launch CGNR pipeline (p = u, v = c)
  void *r1 = nullptr, *p1 = nullptr;
  double* dots = nullptr;
  cgnr_scalars *psc = nullptr, *pscn = nullptr, *psc_h = nullptr;
  step_graph graph;
  bool used_pipeline = false;
  // Gram-mode pipeline: second parity of c (= v) and of the partial dots
  void* v1 = nullptr;
  double* gdots = nullptr;
  // batched plan (rls_cg_create_batched): nrhs columns ldv elements apart, operand panel + partial rows of the
  // skinny matrix-core products (skinny.hip); sc / sc_h hold nrhs structs
  int nrhs = 1;
  int64_t ldv = 0;
  shared_operands ops;
  // resident mode: cg! on (AHA + rho I) IS the CGNR recurrence, so after the start kernel the whole inner solve runs as
  // ONE launch of cgnr_resident_kernel with A in registers (normal.hip)
  resident_slot resident;
  double* rdots = nullptr;
  bool gram_resident = false;  // Gram mode with AHA small enough for the register files (rls_gram_resident_ok)
  // the last rls_cg_solve, kept so that rls_cg_get_status can repeat it on the pipeline if its resident launch was lost
  // (a lost launch is a no-op: x still holds the warm start)
  struct {
    void* x = nullptr;
    const void* b = nullptr;
    float rho = 0.f, reltol = 0.f;
    int32_t maxiter = 0;
    bool valid = false;
  } last;
};

static bool cg_use_gram_pipeline(const rls_cg* s) {
  return s->gdots && s->op->G && s->op->ctx->tune.gram_pipeline;
}

static rls_gram_pipe cg_gram_desc(const rls_cg* s, void* x) {
  return gram_pipe_desc(s->op, x, s->r, s->r1, s->u, s->p1, s->c, s->v1, s->gdots, s->psc, s->pscn);
}

static bool cg_use_pipeline(const rls_cg* s) {
  const rls_ctx* ctx = s->op->ctx;
  return s->r1 && s->op->slab && !s->op->G && ctx->tune.fused_normal && ctx->tune.cgnr_pipeline;
}

static rls_cgnr_pipe cg_pipe_desc(const rls_cg* s, void* x) {
  return pipe_desc(s->op, x, s->r, s->r1, s->u, s->p1, s->c, s->dots, s->psc, s->pscn);
}

// warm start of the pipeline: c = AHA x is in place; r = b - c - rho x, u = r, scalars reset.
// done at entry mirrors cg!: residual <= tol = reltol * residual (only for reltol >= 1) or maxiter == 0;
// r == 0 exactly is also final (the next alpha would be 0/0).
// ADMM plan (rls_admm_step): the start kernel also forms the right-hand side, b = beta_y + rho (z - u), keeps
// xold = x (src/ADMM.jl:236-243, identity regTrafo), and turns the whole x-update into no-ops once the plan's
// `done` flag is set.  All pointers null for a plain cg! call.
template <typename E>
struct admm_fuse {
  const E *beta_y, *z, *u;
  E *beta, *xold;
  float rho;
  const int* skip;
};
// Batched plans (rls_cg_create_batched): col_batch above.
// X (N x K) -> operand panel, ahead of the warm-start apply AHA x of every outer iteration
template <typename E>
__global__ __launch_bounds__(256) void pack_panel_kernel(const E* __restrict__ X, int64_t ldv, operand_view<E> O, int64_t n) {
  const int b = blockIdx.y;
  const panel_col<E> up = O.column(n, b);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    up.put(i, X[(int64_t)b * ldv + i]);
}
template <typename E>
__device__ static inline E admm_rhs(const admm_fuse<E>& F, const E* b, const E* x, int64_t i) {
  if (!F.beta_y) return b[i];
  E bi = F.beta_y[i];
  bi = elem<E>::add(bi, elem<E>::scale(F.rho, F.z[i]));
  bi = elem<E>::add(bi, elem<E>::scale(-F.rho, F.u[i]));
  F.beta[i] = bi;
  F.xold[i] = x[i];
  return bi;
}

template <typename E>
__global__ __launch_bounds__(UPD_THREADS) void cg_pipe_start_kernel(const E* __restrict__ x, const E* b,
                                                                    E* __restrict__ u, E* __restrict__ r,
                                                                    const E* __restrict__ c, int64_t n,
                                                                    cgnr_scalars* sc, float rho, float reltol,
                                                                    int maxiter, admm_fuse<E> F) {
  __shared__ double sm[16];
  if (F.skip && *F.skip) {
    if (threadIdx.x == 0) {
      sc->iteration = 0;
      sc->max_iter = maxiter;
      sc->pending = 0;
      sc->cur = 0;
      sc->fresh = 0;
      sc->done = 1;
    }
    return;
  }
  double rr = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += UPD_THREADS) {
    const E ci = elem<E>::add(c[i], elem<E>::scale(rho, x[i]));
    const E ri = elem<E>::sub(admm_rhs<E>(F, b, x, i), ci);
    r[i] = ri;
    u[i] = ri;
    rr += (double)elem<E>::re(ri) * (double)elem<E>::re(ri) + (double)elem<E>::im(ri) * (double)elem<E>::im(ri);
  }
  rr = block_sum(rr, sm);
  if (threadIdx.x == 0) {
    sc->rr = rr;
    sc->z0 = sqrt(rr);
    sc->zeta = 0.0;
    sc->alpha_re = sc->alpha_im = sc->beta_re = sc->beta_im = 0.0;
    sc->lambda = rho;
    sc->rel_tol = reltol;
    sc->iteration = 0;
    sc->max_iter = maxiter;
    sc->pending = 0;
    sc->cur = 0;
    sc->fresh = 0;
    sc->done = (maxiter <= 0) || (rr == 0.0) || (1.0f <= reltol);
  }
}

// ADMM bookkeeping for an identity regTrafo, src/ADMM.jl:259-299 in ONE single-workgroup launch:
//   u_new = u + x - z ;  Delta = ||x-xold|| + ||z-zold|| + ||u_new-u|| ;  s = rho ||z-zold|| ;
//   eps_pri = max(||x||, ||z||) ; r = ||x-z|| ; eps_dua = rho ||u_new||
// (with Phi = I the reference's hijacked scratch sequence reduces to exactly these seven norms).
// out[0..5] = Delta, s/rho, eps_pri, r, eps_dua/rho, ||x-xold||   (floats; rho applied on the host)
template <typename E>
__global__ __launch_bounds__(UPD_THREADS) void admm_post_kernel(const E* __restrict__ x, const E* __restrict__ xold,
                                                                const E* __restrict__ z, const E* __restrict__ zold,
                                                                E* __restrict__ u, int64_t n, float* __restrict__ out) {
  __shared__ double sm[48];
  double dx = 0, dz = 0, du = 0, nx = 0, nz = 0, nxz = 0, nu = 0;
  auto sq = [](E a) { return (double)elem<E>::re(a) * (double)elem<E>::re(a) + (double)elem<E>::im(a) * (double)elem<E>::im(a); };
  for (int64_t i = threadIdx.x; i < n; i += UPD_THREADS) {
    const E xi = x[i], zi = z[i], ui = u[i];
    const E xz = elem<E>::sub(xi, zi);
    const E un = elem<E>::sub(elem<E>::add(ui, xi), zi);  // u += x ; u -= z   (:266-267)
    u[i] = un;
    dx += sq(elem<E>::sub(xi, xold[i]));
    dz += sq(elem<E>::sub(zi, zold[i]));
    du += sq(elem<E>::sub(un, ui));
    nx += sq(xi);
    nz += sq(zi);
    nxz += sq(xz);
    nu += sq(un);
  }
  block_sum3(dx, dz, du, sm);
  block_sum3(nx, nz, nxz, sm);
  nu = block_sum(nu, sm);
  if (threadIdx.x == 0) {
    out[0] = (float)sqrt(dx) + (float)sqrt(dz) + (float)sqrt(du);
    out[1] = (float)sqrt(dz);
    out[2] = fmaxf((float)sqrt(nx), (float)sqrt(nz));
    out[3] = (float)sqrt(nxz);
    out[4] = (float)sqrt(nu);
    out[5] = (float)sqrt(dx);
  }
}

// beta = beta_y + rho (z - u) ; xold = x      (src/ADMM.jl:236-243, identity regTrafo)
template <typename E>
__global__ void admm_pre_kernel(E* __restrict__ beta, const E* __restrict__ beta_y, const E* __restrict__ z,
                                const E* __restrict__ u, const E* __restrict__ x, E* __restrict__ xold, int64_t n,
                                float rho, int accumulate) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    E bi = accumulate ? beta[i] : beta_y[i];
    bi = elem<E>::add(bi, elem<E>::scale(rho, z[i]));
    bi = elem<E>::add(bi, elem<E>::scale(-rho, u[i]));
    beta[i] = bi;
    if (!accumulate) xold[i] = x[i];
  }
}

// the scalars of a cg! that starts with ||r||^2 = rr (thread 0 of the column's workgroup)
__device__ static inline void cg_start_scalars(cg_scalars* sc, double rr, float rho, float reltol, int maxiter) {
  const double residual = sqrt(rr);
  const double tol = fmax((double)((float)reltol * (float)residual), 0.0);
  sc->residual = residual;
  sc->prev = 1.0;
  sc->tol = tol;
  sc->rho = rho;
  sc->reltol = reltol;
  sc->iteration = 0;
  sc->maxiter = maxiter;
  sc->done = (0 >= maxiter) || ((float)residual <= (float)tol);
}

// c = AHA x is in place.  c += rho x ; r = b - c ; residual = ||r|| ; tol ; u = r (= r + beta*0)
template <typename E>
__global__ __launch_bounds__(UPD_THREADS) void cg_start_kernel(const E* __restrict__ x, const E* b,
                                                               E* __restrict__ u, E* __restrict__ r,
                                                               const E* __restrict__ c, int64_t n, cg_scalars* sc,
                                                               float rho, float reltol, int maxiter, admm_fuse<E> F,
                                                               col_batch<E> B) {
  __shared__ double sm[16];
  const int bq = blockIdx.x;
  {
    const int64_t o = (int64_t)bq * B.ldv;
    x += o; u += o; r += o; c += o;
    if (b) b += o;
    if (F.beta_y) { F.beta_y += o; F.z += o; F.u += o; F.beta += o; F.xold += o; }
    if (F.skip) F.skip += (int64_t)bq * B.skip_stride;
    sc += bq;
  }
  const panel_col<E> up = B.ops.column(n, bq);
  if (F.skip && *F.skip) {
    if (threadIdx.x == 0) {
      sc->iteration = 0;
      sc->maxiter = maxiter;
      sc->done = 1;
    }
    return;
  }
  double rr = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += UPD_THREADS) {
    const E cv = B.ops.Vpart ? B.ops.sum(bq, n, i) : c[i];
    const E ci = elem<E>::add(cv, elem<E>::scale(rho, x[i]));
    const E ri = elem<E>::sub(admm_rhs<E>(F, b, x, i), ci);
    r[i] = ri;
    u[i] = ri;  // first iteration: beta = residual^2 / 1^2 multiplies u == 0
    if (B.ops.panel) up.put(i, ri);
    rr += (double)elem<E>::re(ri) * (double)elem<E>::re(ri) + (double)elem<E>::im(ri) * (double)elem<E>::im(ri);
  }
  rr = block_sum(rr, sm);
  if (threadIdx.x == 0) cg_start_scalars(sc, rr, rho, reltol, maxiter);
}

// SplitBregman on a batched plan (rls_admm_set_bregman): the start kernel of the first inner iteration of a block.  The
// partial rows hold AHA x, the product of this iteration's warm start, and x has not changed since the block before
// ended -- so the Bregman update of that block (src/SplitBregman.jl:257-267) needs no product of its own:
//   beta_y = (beta_y + y) - AHA x  (two roundings: `.+=`, then the 5-argument mul!) ;  z = x ;  u = 0
// and then what cg_start_kernel does: beta = beta_y + rho (z - u), xold = x, r = beta - AHA x - rho x.  One workgroup
// per column.  A column whose `done` is set has no next inner iteration: its x, beta_y, z and u stay as they are.
template <typename E>
__global__ __launch_bounds__(UPD_THREADS) void cg_start_bregman_kernel(const E* __restrict__ x, const E* __restrict__ y,
                                                                       int64_t ldy, E* __restrict__ beta_y,
                                                                       E* __restrict__ z, E* __restrict__ zu,
                                                                       E* __restrict__ beta, E* __restrict__ xold,
                                                                       E* __restrict__ u, E* __restrict__ r, int64_t n,
                                                                       cg_scalars* sc, float rho, float reltol,
                                                                       int maxiter, const int* skip, col_batch<E> B) {
  __shared__ double sm[16];
  const int bq = blockIdx.x;
  {
    const int64_t o = (int64_t)bq * B.ldv;
    x += o; beta_y += o; z += o; zu += o; beta += o; xold += o; u += o; r += o;
    y += (int64_t)bq * ldy;
    skip += (int64_t)bq * B.skip_stride;
    sc += bq;
  }
  if (*skip) {
    if (threadIdx.x == 0) {
      sc->iteration = 0;
      sc->maxiter = maxiter;
      sc->done = 1;
    }
    return;
  }
  const panel_col<E> up = B.ops.column(n, bq);
  double rr = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += UPD_THREADS) {
    const E cv = B.ops.sum(bq, n, i);
    const E xi = x[i];
    const E by = elem<E>::sub(elem<E>::add(beta_y[i], y[i]), cv);
    beta_y[i] = by;
    z[i] = xi;
    zu[i] = elem<E>::zero();
    const E bi = elem<E>::add(by, elem<E>::scale(rho, xi));  // beta_y + rho z - rho u with z = x, u = 0
    beta[i] = bi;
    xold[i] = xi;
    const E ri = elem<E>::sub(bi, elem<E>::add(cv, elem<E>::scale(rho, xi)));
    r[i] = ri;
    u[i] = ri;
    up.put(i, ri);
    rr += (double)elem<E>::re(ri) * (double)elem<E>::re(ri) + (double)elem<E>::im(ri) * (double)elem<E>::im(ri);
  }
  rr = block_sum(rr, sm);
  if (threadIdx.x == 0) cg_start_scalars(sc, rr, rho, reltol, maxiter);
}

// after c = AHA u:  c += rho u ; alpha = residual^2 / <u, c> ; x += alpha u ; r -= alpha c ;
// residual = ||r|| ; then the next direction u = r + beta u
template <typename E>
__global__ __launch_bounds__(UPD_THREADS) void cg_update_kernel(E* __restrict__ x, E* __restrict__ u,
                                                                E* __restrict__ r, E* __restrict__ c, int64_t n,
                                                                cg_scalars* sc, col_batch<E> B) {
  const int bq = blockIdx.x;
  {
    const int64_t o = (int64_t)bq * B.ldv;
    x += o; u += o; r += o; c += o;
    sc += bq;
  }
  if (sc->done) return;
  const panel_col<E> up = B.ops.column(n, bq);
  __shared__ double sm[16];
  const float rho = sc->rho;
  double dre = 0.0, dim_ = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += UPD_THREADS) {
    const E ui = u[i];
    const E cv = B.ops.Vpart ? B.ops.sum(bq, n, i) : c[i];
    const E ci = elem<E>::add(cv, elem<E>::scale(rho, ui));
    c[i] = ci;
    dre += (double)elem<E>::re(ui) * (double)elem<E>::re(ci) + (double)elem<E>::im(ui) * (double)elem<E>::im(ci);
    if constexpr (elem<E>::cplx)
      dim_ += (double)elem<E>::re(ui) * (double)elem<E>::im(ci) - (double)elem<E>::im(ui) * (double)elem<E>::re(ci);
  }
  dre = block_sum(dre, sm);
  if constexpr (elem<E>::cplx) dim_ = block_sum(dim_, sm);
  const double res = sc->residual;
  dcomplex alpha = dc_div({res * res, 0.0}, {dre, dim_});
  const E a = elem<E>::make((float)alpha.re, (float)alpha.im);
  const E na = elem<E>::make(-(float)alpha.re, -(float)alpha.im);
  double rr = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += UPD_THREADS) {
    x[i] = elem<E>::fma(a, u[i], x[i]);
    const E ri = elem<E>::fma(na, c[i], r[i]);
    r[i] = ri;
    rr += (double)elem<E>::re(ri) * (double)elem<E>::re(ri) + (double)elem<E>::im(ri) * (double)elem<E>::im(ri);
  }
  rr = block_sum(rr, sm);
  const double residual = sqrt(rr);
  const int it = sc->iteration + 1;
  const int done = (it >= sc->maxiter) || ((float)residual <= (float)sc->tol);
  if (!done) {
    const float beta = (float)(rr / (res * res));
    for (int64_t i = threadIdx.x; i < n; i += UPD_THREADS) {
      const E un = elem<E>::add(r[i], elem<E>::scale(beta, u[i]));
      u[i] = un;
      if (B.ops.panel) up.put(i, un);
    }
  }
  if (threadIdx.x == 0) {
    sc->prev = res;
    sc->residual = residual;
    sc->iteration = it;
    sc->done = done;
  }
}

// ---------------------------------------------------------------------------------------------
// ADMM plan: whole outer iterations without host involvement (one regulariser, identity regTrafo)
// ---------------------------------------------------------------------------------------------
struct admm_scalars {
  int iteration, done, max_iter, pad;
  float rho, sigma_abs, rel_tol, pad2;
};
constexpr int ADMM_REC = 8;  // floats per log record: Delta, sk, eps_pri, rk, eps_dua, cg iterations, 0, 0

struct rls_admm {
  plan_buffers mem;
  rls_cg* cg = nullptr;
  rls_ctx* actx = nullptr;
  uint64_t actx_id = 0;
  int device = 0;
  rls_admm_params P = {};
  bool ready = false;
  admm_scalars *sc = nullptr, *sc_h = nullptr;
  float *log = nullptr, *log_h = nullptr;  // the group behind log_mark: replaced as a whole when an init asks for more records
  plan_buffers::mark_t log_mark = {};
  int log_cap = 0;
  int enq = 0;  // outer iterations enqueued since init (== device iteration unless the plan stopped early)
  int nrhs = 1;  // batched plans: sc / sc_h / log hold one entry per column
  int requested = 0;  // outer iterations asked for since init (capped at P.iterations)
  int fallbacks = 0;  // resident cg! launches lost and recovered (rls_admm_get_status)
  // Bregman mode of a batched plan (rls_admm_set_bregman): block length, and y = A^H b per column (N x nrhs, ldy)
  int breg_inner = 0;
  const void* breg_y = nullptr;
  int64_t breg_ldy = 0;
};

// src/ADMM.jl:246-309 in ONE single-workgroup launch: projections on x, z = prox(x + u) (L1 / L2 inline; a TV prox
// has been written to `znew` by the FGP launch before this one), u += x - z, the seven norms (see admm_post_kernel),
// then `converged` / `done` (:324-330) decided HERE in Float32 exactly as the host would, and one log record.
template <typename E>
__global__ __launch_bounds__(UPD_THREADS) void admm_zu_kernel(E* __restrict__ x, const E* __restrict__ xold,
                                                              E* __restrict__ znew, const E* __restrict__ zold,
                                                              E* __restrict__ u, int64_t n, int reg_kind, float lam,
                                                              int proj_kind, int z_ready, admm_scalars* sc,
                                                              const int* cg_iterations, float* __restrict__ log,
                                                              col_batch<E> B, const cg_scalars* cgs) {
  __shared__ double sm[48];
  {
    const int bq = blockIdx.x;  // batched plans: one workgroup per column
    const int64_t o = (int64_t)bq * B.ldv;
    x += o; xold += o; znew += o; zold += o; u += o;
    sc += bq;
    log += (int64_t)bq * B.log_stride;
    if (cgs) cg_iterations = &cgs[bq].iteration;
  }
  if (sc->done) return;
  double dx = 0, dz = 0, du = 0, nx = 0, nz = 0, nxz = 0, nu = 0;
  auto sq = [](E a) { return (double)elem<E>::re(a) * (double)elem<E>::re(a) + (double)elem<E>::im(a) * (double)elem<E>::im(a); };
  // four elements per thread and trip, every load of a trip requested before the first is used (the obvious loop was one
  // dependent memory round trip per element: 8.5 us for N = 4096, most of it waiting)
  constexpr int U = 4;
  for (int64_t i0 = threadIdx.x; i0 < n; i0 += (int64_t)U * UPD_THREADS) {
    E xa[U], ua[U], za[U], xo[U], zo[U];
#pragma unroll
    for (int q = 0; q < U; ++q) {
      const int64_t i = i0 + (int64_t)q * UPD_THREADS;
      const int64_t ic = i < n ? i : i0;  // clamped address, masked below
      xa[q] = x[ic];
      ua[q] = u[ic];
      za[q] = z_ready ? znew[ic] : elem<E>::zero();
      xo[q] = xold[ic];
      zo[q] = zold[ic];
    }
#pragma unroll
    for (int q = 0; q < U; ++q) {
      const int64_t i = i0 + (int64_t)q * UPD_THREADS;
      if (i >= n) continue;
      E xi = xa[q];
      if (proj_kind != RLS_PROJ_NONE) {
        xi = fista_proj_elem<E>(xi, proj_kind);
        x[i] = xi;
      }
      const E ui = ua[q];
      E zi;
      if (z_ready) {
        zi = za[q];
      } else {
        zi = fista_prox_elem<E>(elem<E>::add(xi, ui), reg_kind, lam);
        znew[i] = zi;
      }
      const E xz = elem<E>::sub(xi, zi);
      const E un = elem<E>::sub(elem<E>::add(ui, xi), zi);  // u += x ; u -= z   (:266-267)
      u[i] = un;
      dx += sq(elem<E>::sub(xi, xo[q]));
      dz += sq(elem<E>::sub(zi, zo[q]));
      du += sq(elem<E>::sub(un, ui));
      nx += sq(xi);
      nz += sq(zi);
      nxz += sq(xz);
      nu += sq(un);
    }
  }
  block_sum3(dx, dz, du, sm);
  block_sum3(nx, nz, nxz, sm);
  nu = block_sum(nu, sm);
  if (threadIdx.x == 0) {
    // one rounding per operation, as the host's Float32 arithmetic (f32_mul / f32_add: never fused into an FMA)
    const float rho = sc->rho;
    const float delta = f32_add(f32_add((float)sqrt(dx), (float)sqrt(dz)), (float)sqrt(du));
    const float sk = f32_mul(rho, (float)sqrt(dz));
    const float eps_pri = fmaxf((float)sqrt(nx), (float)sqrt(nz));
    const float rk = (float)sqrt(nxz);
    const float eps_dua = f32_mul(rho, (float)sqrt(nu));
    const float lim_pri = f32_add(sc->sigma_abs, f32_mul(sc->rel_tol, eps_pri));
    const float lim_dua = f32_add(sc->sigma_abs, f32_mul(sc->rel_tol, eps_dua));
    const bool conv = rk < lim_pri && sk < lim_dua;
    const int it = sc->iteration;
    float* rec = log + (int64_t)it * ADMM_REC;
    rec[0] = delta;
    rec[1] = sk;
    rec[2] = eps_pri;
    rec[3] = rk;
    rec[4] = eps_dua;
    rec[5] = (float)*cg_iterations;
    rec[6] = rec[7] = 0.f;
    sc->iteration = it + 1;
    sc->done = conv || (it + 1 >= sc->max_iter);
  }
}

template <typename E>
__global__ void admm_reset_kernel(admm_scalars* sc, int max_iter, float rho, float sigma_abs, float rel_tol) {
  sc += blockIdx.x;
  sc->iteration = 0;
  sc->max_iter = max_iter;
  sc->done = max_iter <= 0;
  sc->rho = rho;
  sc->sigma_abs = sigma_abs;
  sc->rel_tol = rel_tol;
}

// type-erased admm_fuse (null beta_y = plain cg!)
struct admm_fuse_v {
  const void *beta_y = nullptr, *z = nullptr, *u = nullptr;
  void *beta = nullptr, *xold = nullptr;
  float rho = 0.f;
  const int* skip = nullptr;
  int* poison = nullptr;  // rls_cg_start::poison
};
template <typename E>
static admm_fuse<E> typed_fuse(const admm_fuse_v& V) {
  admm_fuse<E> F;
  F.beta_y = (const E*)V.beta_y;
  F.z = (const E*)V.z;
  F.u = (const E*)V.u;
  F.beta = (E*)V.beta;
  F.xold = (E*)V.xold;
  F.rho = V.rho;
  F.skip = V.skip;
  return F;
}

static int32_t cg_solve_impl(rls_cg* s, void* x, const void* b, float rho, int32_t maxiter, float reltol,
                             const admm_fuse_v& FV) {
  rls_operator* op = s->op;
  rls_ctx* ctx = op->ctx;
  const int64_t n = op->N;
  // the start kernel of both per-iteration pipelines (Gram mode and matrix-free)
  auto pipe_start = [&] {
    return rls_with_elem(op->dtype, [&](auto t) {
      using E = typename decltype(t)::type;
      return rls_launch<cg_pipe_start_kernel<E>>(ctx, dim3(1), dim3(UPD_THREADS), 0, (const E*)x, (const E*)b, (E*)s->u, (E*)s->r,
                                                 (const E*)s->c, n, s->psc, rho, reltol, maxiter, typed_fuse<E>(FV));
    });
  };
  // the cg! entry folded into a resident launch: warm-start apply, r = b - (AHA + rho I) x (ADMM's beta formed on the way)
  rls_cg_start St;
  St.enabled = 1;
  St.b = b;
  St.beta_y = FV.beta_y;
  St.z = FV.z;
  St.u = FV.u;
  St.beta = FV.beta;
  St.xold = FV.xold;
  St.rho_admm = FV.rho;
  St.rho = rho;
  St.reltol = reltol;
  St.maxiter = maxiter;
  St.skip = FV.skip;
  St.poison = FV.poison;
  if (cg_use_gram_pipeline(s) && s->gram_resident && s->resident.usable(ctx) && maxiter > 0) {
    // Gram mode, AHA in the register files: the whole cg! -- start and every iteration -- is ONE launch of
    // cgnr_gram_resident_kernel (normal.hip)
    s->used_pipeline = true;
    const rls_gram_pipe P = cg_gram_desc(s, x);
    return s->resident.launch(ctx, [&](void* sync, unsigned spin) {
      return rls_gram_resident_launch(ctx, op->dtype, P, sync, maxiter, spin, St);
    });
  }
  const bool resident_mf = cg_use_pipeline(s) && !cg_use_gram_pipeline(s) && s->resident.usable(ctx) && maxiter > 0 &&
                           aligned16(x, s->r, s->u, s->c, b, FV.beta_y, FV.z, FV.u, FV.beta, FV.xold);
  // warm start: one operator apply for r = b - (AHA + rho I) x   (inside the resident launch where that runs)
  if (!resident_mf) RLS_TRY(op_normal(op, x, s->c, FV.skip));
  if (cg_use_gram_pipeline(s)) {
    s->used_pipeline = true;
    RLS_TRY(pipe_start());
    const rls_gram_pipe P = cg_gram_desc(s, x);
    const int32_t dtype = op->dtype;
    s->graph.keep_for(3, x);
    int parity = 0;
    auto one = [ctx, dtype, &P, &parity]() {
      const int32_t st = rls_gram_pipe_iteration(ctx, dtype, P, parity);
      parity ^= 1;
      return st;
    };
    if (ctx->tune.graph_chunk % 2) {
      for (int i = 0; i < maxiter; ++i) RLS_TRY(one());
    } else {
      RLS_TRY(run_steps(ctx, &s->graph, maxiter, one, [&parity](int c) { parity ^= c & 1; }));
    }
    return rls_gram_pipe_finish(ctx, dtype, P, maxiter & 1);
  }
  s->used_pipeline = cg_use_pipeline(s);
  if (s->used_pipeline) {
    if (resident_mf) {
      // matrix-free, A in the register files: start and every iteration in ONE launch of cgnr_resident_kernel (normal.hip)
      const rls_cgnr_pipe P = cg_pipe_desc(s, x);
      return s->resident.launch(ctx, [&](void* sync, unsigned spin) {
        return rls_cgnr_resident_launch(ctx, op->dtype, P, s->rdots, sync, maxiter, spin, St);
      });
    }
    RLS_TRY(pipe_start());
    rls_cgnr_pipe P = cg_pipe_desc(s, x);
    const int32_t dtype = op->dtype;
    s->graph.keep_for(1, x);
    int k = 0;
    RLS_TRY(run_steps(ctx, &s->graph, maxiter, [ctx, dtype, &P, &k]() {
      P.cur_hint = pipe_cur_hint(ctx, k++);
      return rls_cgnr_pipe_iteration(ctx, dtype, P);
    }, [&k](int c) { k -= c; }));
    return rls_cgnr_pipe_finish(ctx, dtype, P);
  }
  return rls_with_elem(op->dtype, [&](auto t) -> int32_t {
    using E = typename decltype(t)::type;
    RLS_TRY(rls_launch<cg_start_kernel<E>>(ctx, dim3(1), dim3(UPD_THREADS), 0, (const E*)x, (const E*)b, (E*)s->u, (E*)s->r,
                                           (const E*)s->c, n, s->sc, rho, reltol, maxiter, typed_fuse<E>(FV), col_batch<E>()));
    for (int it = 0; it < maxiter; ++it) {
      RLS_TRY(op_normal(op, s->u, s->c, &s->sc->done));
      RLS_TRY(rls_launch<cg_update_kernel<E>>(ctx, dim3(1), dim3(UPD_THREADS), 0, (E*)x, (E*)s->u, (E*)s->r, (E*)s->c, n, s->sc,
                                              col_batch<E>()));
    }
    return 0;
  });
}

// ---- batched ADMM (shared A): every column's outer iteration advances together --------------------------------
// Per outer iteration: X -> operand panel, T = A X and V = A^H T on the matrix cores (the warm-start apply of every
// column's cg!), the per-column start kernel (beta = beta_y + rho (z - u), r, u; next operand = u), iterations_cg x
// {T = A U, V = A^H T, per-column CG update}, the FGP launch with one workgroup per column for a TV term, and the
// per-column z / u / residual-norm / `done` kernel.  Columns retire independently (per-column device flags), exactly
// as K independent solves do (src/MultiThreading.jl:60-78).
template <typename E>
static int32_t admm_step_batched_typed(rls_admm* a, int32_t n_outer) {
  rls_cg* cg = a->cg;
  rls_ctx* ctx = cg->op->ctx;
  const rls_admm_params& P = a->P;
  const int32_t dtype = cg->op->dtype;
  const int64_t n = cg->op->N;
  const unsigned K = (unsigned)a->nrhs;
  const rls_skinny SK = cg->ops.desc(cg->op, cg->nrhs, cg->ldv);
  const col_batch<E> B{cg->ldv, cg->ops.view<E>(a->nrhs), (int)(sizeof(admm_scalars) / sizeof(int)), (int64_t)ADMM_REC * a->log_cap};
  const col_batch<E> Bz{B.ldv, operand_view<E>(), B.skip_stride, B.log_stride};  // the z / u kernel: no partial rows, no panel
  for (int k = 0; k < n_outer && a->enq < P.iterations; ++k, ++a->enq) {
    E* zcur = (E*)((a->enq & 1) ? P.z1 : P.z0);
    E* znew = (E*)((a->enq & 1) ? P.z0 : P.z1);
    hipLaunchKernelGGL(pack_panel_kernel<E>, dim3((unsigned)((n + 255) / 256 < 64 ? (n + 255) / 256 : 64), K), dim3(256), 0,
                       ctx->stream, (const E*)P.x, cg->ldv, B.ops, n);
    RLS_TRY(rls_skinny_launch(ctx, dtype, SK, 1 | 2));  // AHA x of every column  (:244, warm start)
    admm_fuse<E> F;
    F.beta_y = (const E*)P.beta_y;
    F.z = zcur;
    F.u = (const E*)P.u;
    F.beta = (E*)P.beta;
    F.xold = (E*)P.xold;
    F.rho = P.rho;
    F.skip = &a->sc->done;
    if (a->breg_inner > 0 && a->enq > 0 && a->enq % a->breg_inner == 0)
      // SplitBregman: a block of inner iterations ended here; its Bregman update rides on this start (the product is shared)
      hipLaunchKernelGGL(cg_start_bregman_kernel<E>, dim3(K), dim3(UPD_THREADS), 0, ctx->stream, (const E*)P.x,
                         (const E*)a->breg_y, a->breg_ldy, (E*)P.beta_y, zcur, (E*)P.u, (E*)P.beta, (E*)P.xold, (E*)cg->u,
                         (E*)cg->r, n, cg->sc, P.rho, P.tol_inner, P.iterations_cg, F.skip, B);
    else
      hipLaunchKernelGGL(cg_start_kernel<E>, dim3(K), dim3(UPD_THREADS), 0, ctx->stream, (const E*)P.x, (const E*)P.beta,
                         (E*)cg->u, (E*)cg->r, (const E*)cg->c, n, cg->sc, P.rho, P.tol_inner, P.iterations_cg, F, B);
    for (int it = 0; it < P.iterations_cg; ++it) {
      RLS_TRY(rls_skinny_launch(ctx, dtype, SK, 1 | 2));
      hipLaunchKernelGGL(cg_update_kernel<E>, dim3(K), dim3(UPD_THREADS), 0, ctx->stream, (E*)P.x, (E*)cg->u, (E*)cg->r,
                         (E*)cg->c, n, cg->sc, B);
    }
    const int z_ready = P.reg_kind == RLS_REG_TV;
    if (z_ready)
      RLS_TRY(rls_tv_single_launch(ctx, dtype, P.tv_ndims, P.tv_shape, P.tv_ntv, P.tv_dims, P.x, P.u, znew, P.prox_lambda,
                                   P.tv_iterations, &a->sc->done, (int)K, cg->ldv, B.skip_stride));
    hipLaunchKernelGGL(admm_zu_kernel<E>, dim3(K), dim3(UPD_THREADS), 0, ctx->stream, (E*)P.x, (const E*)P.xold, znew,
                       (const E*)zcur, (E*)P.u, n, P.reg_kind, P.prox_lambda, P.proj_kind, z_ready, a->sc,
                       (const int*)nullptr, a->log, Bz, (const cg_scalars*)cg->sc);
    RLS_TRY(launch_status(ctx));
  }
  return 0;
}

static int32_t admm_step_batched(rls_admm* a, int32_t n_outer) {
  return rls_with_elem(a->cg->op->dtype, [&](auto t) { return admm_step_batched_typed<typename decltype(t)::type>(a, n_outer); });
}

static rls_operator* cgnr_op(rls_cgnr* s) { return s->op; }
static bool cgnr_single(rls_cgnr* s) { return s->nrhs == 1; }
static rls_operator* admm_op(rls_admm* a) { return a->cg->op; }
static bool admm_single(rls_admm* a) { return a->nrhs == 1 && !a->cg->ops.allocated(); }

template <typename E>
static void admm_local_start(rls_admm* a, const admm_fuse_v& F) {
  rls_cg* cg = a->cg;
  rls_ctx* ctx = cg->op->ctx;
  const rls_admm_params& P = a->P;
  hipLaunchKernelGGL(cg_start_kernel<E>, dim3(1), dim3(UPD_THREADS), 0, ctx->stream, (const E*)P.x, (const E*)P.beta, (E*)cg->u,
                     (E*)cg->r, (const E*)cg->c, cg->op->N, cg->sc, P.rho, P.tol_inner, P.iterations_cg, typed_fuse<E>(F),
                     col_batch<E>());
}
template <typename E>
static void admm_local_finish(rls_admm* a, void* zcur, void* znew) {
  rls_cg* cg = a->cg;
  rls_ctx* ctx = cg->op->ctx;
  const rls_admm_params& P = a->P;
  hipLaunchKernelGGL(admm_zu_kernel<E>, dim3(1), dim3(UPD_THREADS), 0, ctx->stream, (E*)P.x, (const E*)P.xold, (E*)znew,
                     (const E*)zcur, (E*)P.u, cg->op->N, P.reg_kind, P.prox_lambda, P.proj_kind,
                     P.reg_kind == RLS_REG_TV ? 1 : 0, a->sc, &cg->sc->iteration, a->log, col_batch<E>(), nullptr);
}

extern "C" {

// ---- CGNR -----------------------------------------------------------------------------------
static int32_t cgnr_create_impl(rls_operator* op, int32_t nrhs, void* x, void* r, void* p, void* v, int64_t ldv,
                                rls_cgnr** out) {
  if (!op) return RLS_E_INVALID;
  rls_ctx* ctx = op->ctx;
  if (!x || !r || !p || !v || !out || nrhs < 1 || ldv < op->N)
    return rls_fail(ctx, RLS_E_INVALID, "cgnr_create: bad argument");
  RLS_HIP(ctx, rls_enter(ctx));
  // the columns share solver.AHA (src/MultiThreading.jl:30-48): an explicit Gram matrix when the operator has one -- the
  // reference constructors' default for a dense matrix, src/CGNR.jl:49 --, otherwise the two products over A
  const bool skinny = nrhs > 1 && ctx->tune.batched_mfma && shared_operands::supported(op);
  if (nrhs > 1 && !skinny)
    return rls_fail(ctx, RLS_E_UNSUPPORTED, "batched CGNR runs on the matrix cores: A (and AHA, when explicit) with M, N multiples "
                                            "of 16 and 16-byte aligned columns (other shapes: one plan per column)");
  *out = nullptr;
  rls_alloc_scope alloc_scope(ctx);
  rls_cgnr* s = new rls_cgnr{plan_memory(ctx)};
  plan_buffers& mem = s->mem;  // after the first failure every request below is a no-op
  s->actx = ctx;
  s->actx_id = ctx->id;
  s->skinny = skinny;
  s->op = op;
  s->device = ctx->device;
  s->x = x;
  s->r = r;
  s->p = p;
  s->v = v;
  s->nrhs = nrhs;
  s->ldv = ldv;
  const size_t sb = sizeof(cgnr_scalars) * (size_t)nrhs;
  mem.dev(&s->sc, sb, true);
  mem.pinned(&s->sc_h, sb, true);
  if (op->slab) {  // scratch of the fused pipeline
    const size_t vb = (size_t)ldv * nrhs * rls_elem_size(op->dtype);
    const size_t nd = (size_t)((op->N + 15) / 16) * 4 * sizeof(double) * nrhs;
    mem.dev(&s->r1, vb, true);
    mem.dev(&s->p1, vb, true);
    mem.dev(&s->dots, nd, true);
    if (op->A && !op->G)  // matrix-free: K_A's ||t_w||^2 per row block (alpha = zeta / ||A p||^2)
      mem.dev(&s->ttw, (size_t)rls_cgnr_resident_nwg(op->ctx, op->dtype, op->M, op->N) * sizeof(double) * nrhs, true);
    mem.dev(&s->scn, sb, true);
    if (nrhs > 1 && !skinny)
      mem.dev(&s->slab_b, rls_normal_fused_workspace(op->ctx, op->dtype, op->M, op->N, op->A, op->lda) * (size_t)nrhs, false);
  }
  s->small = nrhs == 1 && op->A && !op->G && rls_small_ok(op->dtype, op->M, op->N, op->A, op->lda);
  // (the single-workgroup kernel can stay and listen as well: rls_cgnr_step_status; no co-residency requirement, nothing to give
  // up: no flags to read)
  if (s->small) server_ctl_optional(mem, &s->srv);
  if (!mem.error() && nrhs == 1 && op->slab && op->A && !op->G && rls_cgnr_resident_ok(ctx, op->dtype, op->M, op->N, op->A, op->lda)) {
    s->resident.alloc(mem, ctx, op);
    mem.dev(&s->rdots, (size_t)rls_cgnr_resident_nwg(op->ctx, op->dtype, op->M, op->N) * 4 * sizeof(double), true);
    if (!s->srv.ctl) {
      mem.pinned(&s->srv.ctl, RLS_Q_CTL_WORDS * sizeof(unsigned), true);  // (the control block and the command ring of queue mode)
      s->q_ok = !mem.error() && rls_cgnr_resident_queue_ok(ctx, op->dtype, op->M, op->N);
    }
    s->srv.resident_used = &s->resident.used;
    s->srv.q_plan = s;
  }
  if (!mem.error() && nrhs == 1 && op->G && rls_gram_pipe_ok(op->dtype, op->N, op->G, op->ldg)) {
    const size_t vb = (size_t)op->N * rls_elem_size(op->dtype);
    const size_t nd = (size_t)2 * rls_gram_pipe_nwg(op->dtype, op->N) * 4 * sizeof(double);
    if (!s->r1) mem.dev(&s->r1, vb, true);  // (an operator with A and AHA: the fused pipeline's blocks above, same sizes, zeroed)
    if (!s->p1) mem.dev(&s->p1, vb, true);
    mem.dev(&s->v1, vb, true);
    mem.dev(&s->gdots, nd, true);
    if (!s->scn) mem.dev(&s->scn, sb, true);
    s->gram_pipe = !mem.error();
    if (s->gram_pipe && !s->resident.sync && rls_gram_resident_ok(ctx, op->dtype, op->N, op->G, op->ldg)) {
      s->resident.alloc(mem, ctx, op);
      s->gram_resident = !mem.error();
      if (s->gram_resident && !s->srv.ctl && rls_gram_resident_server_ok(op->dtype, op->N) && server_ctl_optional(mem, &s->srv))
        s->srv.resident_used = &s->resident.used;
    }
  }
  if (!mem.error() && skinny) {
    s->ops.alloc(mem, op, nrhs);
    if (!mem.error() && op->G && s->ops.half && rls_gramk_resident_ok(ctx, op->dtype, op->N, nrhs, op->G, op->ldg)) {
      size_t xb, xxb, db;
      rls_gramk_sizes(op->N, &xb, &xxb, &db);
      s->resident.alloc(mem, ctx, op);
      mem.dev(&s->gk_vx, xb, true);  // rows >= N are read, never written
      mem.dev(&s->gk_xx, xxb, false);
      mem.dev(&s->gk_dots, db, true);  // slots of absent workgroups add 0.0
      s->gramk = !mem.error();
    }
  }
  if (const int e = mem.error()) {
    rls_cgnr_destroy(s);
    return rls_fail(ctx, e, "cgnr_create: allocation failed");
  }
  *out = s;
  return 0;
}

int32_t rls_cgnr_create(rls_operator* op, void* x, void* r, void* p, void* v, rls_cgnr** out) {
  if (!op) return RLS_E_INVALID;
  return cgnr_create_impl(op, 1, x, r, p, v, op->N, out);
}

int32_t rls_cgnr_create_batched(rls_operator* op, int32_t nrhs, void* X, void* R, void* P, void* V, int64_t ldv,
                                rls_cgnr** out) {
  return cgnr_create_impl(op, nrhs, X, R, P, V, ldv, out);
}

int32_t rls_cgnr_destroy(rls_cgnr* s) {
  if (!s) return RLS_E_INVALID;
  if (rls_ctx_alive(s->actx, s->actx_id) && s->actx->server == &s->srv) rls_server_stop(s->actx);  // (a kernel of this plan left listening)
  hipSetDevice(s->device);
  rls_alloc_scope alloc_scope(alloc_ctx_of(s->actx, s->actx_id));
  s->graph.drop();
  s->mem.release();
  delete s;
  return 0;
}

int32_t rls_cgnr_init_local_a(rls_cgnr* s, const void* b, float lambda, float rel_tol, int32_t iterations) {
  if (!s) return RLS_E_INVALID;
  rls_operator* op = s->op;
  rls_ctx* ctx = op->ctx;
  if (!b) return rls_fail(ctx, RLS_E_INVALID, "cgnr_init: null b");
  if (s->nrhs != 1) return rls_fail(ctx, RLS_E_STATE, "cgnr_init on a batched plan: use rls_cgnr_init_batched");
  RLS_HIP(ctx, rls_enter(ctx));
  // r = A^H b   (initCGNR, src/CGNR.jl:132) ; without A, b already is A^H b (:134)
  if (op->A)
    RLS_TRY(rls_launch_gemv(ctx, op->dtype, RLS_OP_C, op->M, op->N, 1.f, 0.f, op->A, op->lda, b, 0.f, 0.f, s->r, nullptr));
  else
    RLS_HIP(ctx, hipMemcpyAsync(s->r, b, (size_t)op->N * rls_elem_size(op->dtype), hipMemcpyDeviceToDevice, ctx->stream));
  s->sc_h->lambda = lambda;
  s->sc_h->rel_tol = rel_tol;
  s->sc_h->max_iter = cgnr_effective_iterations(s, iterations);
  return 0;
}

int32_t rls_cgnr_init_local_b(rls_cgnr* s) {
  if (!s) return RLS_E_INVALID;
  rls_ctx* ctx = s->op->ctx;
  RLS_HIP(ctx, rls_enter(ctx));
  rls_with_elem(s->op->dtype, [&](auto t) {
    cgnr_launch_init<typename decltype(t)::type>(s, s->sc_h->lambda, s->sc_h->rel_tol, s->sc_h->max_iter);
  });
  s->initialised = true;
  s->requested = 0;
  s->srv.off = false;  // (a new solve: the caller's pattern between iterates is judged afresh)
  s->srv.short_lives = 0;
  return launch_status(ctx);
}

static int32_t cgnr_group(rls_cgnr* const* plans, const void* const* b, int32_t count, float lambda, float rel_tol, int32_t iterations,
                          int32_t n_steps);
extern "C++" {
static bool cgnr_listening_q(const rls_cgnr* s);
static int32_t cgnr_queue_init(rls_cgnr* s, const void* b, float lambda, float rel_tol, int32_t iterations);
static int32_t cgnr_queue_step(rls_cgnr* s, int32_t n_steps);
static bool cgnr_use_queue(const rls_cgnr* s);
static int32_t cgnr_queue_launch(rls_cgnr* s, unsigned seq0, int32_t n_steps);
}
int32_t rls_cgnr_init(rls_cgnr* s, const void* b, float lambda, float rel_tol, int32_t iterations) {
  // queue mode: the plan's kernel is listening -- init! travels with the next rls_cgnr_step, nothing is launched
  if (s && b && s->nrhs == 1 && cgnr_listening_q(s) && (reinterpret_cast<uintptr_t>(b) & 15) == 0)
    return cgnr_queue_init(s, b, lambda, rel_tol, iterations);
  // small systems: init! is the single-workgroup kernel's own (r = A^H b from the registers: ONE launch instead of a GEMV and an
  // init kernel, and the same bits whether a solve is init + steps or one fused launch, rls_cgnr_init_step_group)
  if (s && b && s->nrhs == 1 && s->op->A && cgnr_use_small(s)) return cgnr_group(&s, &b, 1, lambda, rel_tol, iterations, 0);
  RLS_TRY(rls_cgnr_init_local_a(s, b, lambda, rel_tol, iterations));
  return rls_cgnr_init_local_b(s);
}

int32_t rls_cgnr_init_batched(rls_cgnr* s, const void* B, int64_t ldb, float lambda, float rel_tol, int32_t iterations) {
  if (!s) return RLS_E_INVALID;
  rls_operator* op = s->op;
  rls_ctx* ctx = op->ctx;
  if (!B || !op->A || ldb < op->M) return rls_fail(ctx, RLS_E_INVALID, "cgnr_init_batched: bad argument");
  RLS_HIP(ctx, rls_enter(ctx));
  const size_t es = rls_elem_size(op->dtype);
  const int max_iter = cgnr_effective_iterations(s, iterations);
  if (s->skinny) {
    // R = A^H B on the matrix cores (B packed as the T operand), then the per-column init
    RLS_TRY(rls_skinny_init(ctx, op->dtype, cgnr_skinny_desc(s), B, ldb, lambda, rel_tol, max_iter));
    s->sc_h->lambda = lambda;
    s->sc_h->rel_tol = rel_tol;
    s->sc_h->max_iter = max_iter;
    s->initialised = true;
    s->requested = 0;
    return 0;
  }
  if (!cgnr_use_pipeline(s)) return rls_fail(ctx, RLS_E_UNSUPPORTED, "cgnr_init_batched: fused pipeline not active");
  for (int b = 0; b < s->nrhs; ++b) {
    char* rb = (char*)s->r + (size_t)b * s->ldv * es;
    RLS_TRY(rls_launch_gemv(ctx, op->dtype, RLS_OP_C, op->M, op->N, 1.f, 0.f, op->A, op->lda,
                            (const char*)B + (size_t)b * ldb * es, 0.f, 0.f, rb, nullptr));
    char* xb = (char*)s->x + (size_t)b * s->ldv * es;
    char* pb = (char*)s->p + (size_t)b * s->ldv * es;
    char* vb = (char*)s->v + (size_t)b * s->ldv * es;
    rls_with_elem(op->dtype, [&](auto t) {
      using E = typename decltype(t)::type;
      hipLaunchKernelGGL(cgnr_init_kernel<E>, dim3(1), dim3(UPD_THREADS), 0, ctx->stream, (E*)xb, (const E*)rb, (E*)pb, (E*)vb,
                         op->N, s->sc + b, lambda, rel_tol, max_iter);
    });
  }
  s->sc_h->lambda = lambda;
  s->sc_h->rel_tol = rel_tol;
  s->sc_h->max_iter = max_iter;
  s->initialised = true;
  return launch_status(ctx);
}

static int32_t cgnr_step_impl(rls_cgnr* s, int32_t n_steps);
static void cgnr_status_out(const rls_cgnr* s, const cgnr_scalars& h, rls_cgnr_status* out);
// a CGNR plan's status read: the first `nrhs` structs of sc_h (rls_cgnr_get_status: 1)
static int32_t cgnr_fetch_status(rls_cgnr* s, int nrhs) {
  return status_read(s->op->ctx, s, s->sc_h, nrhs, [s](int32_t n) { return cgnr_step_impl(s, n); }, [](long long) {});
}
int32_t rls_cgnr_get_status_batched(rls_cgnr* s, rls_cgnr_status* out) {
  if (!s || !out) return RLS_E_INVALID;
  rls_ctx* ctx = s->op->ctx;
  if (!s->initialised) return rls_fail(ctx, RLS_E_STATE, "cgnr_get_status before cgnr_init");
  RLS_HIP(ctx, rls_enter(ctx));
  RLS_TRY(cgnr_fetch_status(s, s->nrhs));
  for (int b = 0; b < s->nrhs; ++b) cgnr_status_out(s, s->sc_h[b], out + b);
  return 0;
}

static int32_t cgnr_step_impl(rls_cgnr* s, int32_t n_steps) {
  rls_ctx* ctx = s->op->ctx;
  if (cgnr_use_small(s)) {
    if (n_steps == 0) return 0;
    rls_small D = cgnr_small_desc(s);
    D.mb = s->mb_arm;
    s->mb_sent = s->mb_arm.dst != nullptr;
    return rls_small_launch(ctx, s->op->dtype, D, n_steps);
  }
  if (s->skinny && cgnr_use_gramk(s, n_steps)) {
    if (n_steps == 0) return 0;
    const rls_gramk D = cgnr_gramk_desc(s);
    return s->resident.launch(ctx, [&](void* sync, unsigned spin) { return rls_gramk_resident_launch(ctx, D, sync, n_steps, spin); });
  }
  if (s->skinny) {
    const rls_skinny K = cgnr_skinny_desc(s);
    const int32_t dtype = s->op->dtype;
    s->graph.keep_for(2);
    return run_steps(ctx, &s->graph, n_steps, [ctx, dtype, &K]() { return rls_skinny_launch(ctx, dtype, K, 7); });
  }
  if (cgnr_use_gram_pipeline(s)) {
    // one launch per iteration; every call starts at parity 0 (the finish kernel brings the state back to
    // the caller's vectors), and a graph chunk holds an even number of launches, so the captured parities
    // are always the right ones
    const rls_gram_pipe P = cgnr_gram_desc(s);
    const int32_t dtype = s->op->dtype;
    if (cgnr_use_gram_resident(s)) {  // the whole call as ONE launch, AHA in registers, one grid exchange per iteration
      if (n_steps == 0) return 0;
      return s->resident.launch(ctx, [&](void* sync, unsigned spin) {
        return rls_gram_resident_launch(ctx, dtype, P, sync, n_steps, spin);
      });
    }
    s->graph.keep_for(3);
    int parity = 0;
    auto one = [ctx, dtype, &P, &parity]() {
      const int32_t st = rls_gram_pipe_iteration(ctx, dtype, P, parity);
      parity ^= 1;
      return st;
    };
    if (ctx->tune.graph_chunk % 2) {  // an odd chunk would replay the captured parities out of phase
      for (int i = 0; i < n_steps; ++i) RLS_TRY(one());
    } else {
      RLS_TRY(run_steps(ctx, &s->graph, n_steps, one, [&parity](int c) { parity ^= c & 1; }));
    }
    return rls_gram_pipe_finish(ctx, dtype, P, n_steps & 1);
  }
  // A resident launch pays for loading its slab of A (~10 us at the headline shape) before its first iteration: a call of
  // ONE iteration -- the reference's solve! loop with callbacks, one iterate per call -- is cheaper on the two-launch
  // pipeline (bench.py other_paths, iterate_per_call_cadence: 40 us against 52 us per call, host synchronisation included)
  if (cgnr_use_resident(s) && n_steps != 1) {
    // ONE launch for the whole call: A stays in the register files, iterations are separated by an in-kernel
    // grid-wide all-reduce (normal.hip).  The arrival counters and flags are zeroed ahead of every launch.
    if (n_steps == 0) return 0;
    const rls_cgnr_pipe P = cgnr_pipe_desc(s);
    return s->resident.launch(ctx, [&](void* sync, unsigned spin) {
      return rls_cgnr_resident_launch(ctx, s->op->dtype, P, s->rdots, sync, n_steps, spin);
    });
  }
  if (cgnr_use_pipeline(s)) {
    // iteration k = K_A (applies update k-1 in its prologue, then one pass over A) + K_R; the last
    // update of this call is applied by K_F, which also returns r, p to the caller's vectors
    rls_cgnr_pipe P = cgnr_pipe_desc(s);
    const int32_t dtype = s->op->dtype;
    s->graph.keep_for(1);
    int k = 0;
    RLS_TRY(run_steps(ctx, &s->graph, n_steps, [ctx, dtype, &P, &k]() {
      P.cur_hint = pipe_cur_hint(ctx, k++);
      return rls_cgnr_pipe_iteration(ctx, dtype, P);
    }, [&k](int c) { k -= c; }));
    if (s->nrhs == 1) {
      P.mb = s->mb_arm;
      s->mb_sent = s->mb_arm.dst != nullptr;
    }
    return rls_cgnr_pipe_finish(ctx, dtype, P);
  }
  if (s->nrhs != 1) return rls_fail(ctx, RLS_E_UNSUPPORTED, "batched CGNR: fused pipeline switched off");
  s->graph.keep_for(0);
  return run_steps(ctx, &s->graph, n_steps, [s]() { return cgnr_enqueue_iteration(s); });
}

// `queue`: the call may post to (or start) a kernel that stays across solves (queue mode, cgnr_use_queue)
static int32_t cgnr_step_call(rls_cgnr* s, int32_t n_steps, bool queue) {
  if (!s) return RLS_E_INVALID;
  rls_ctx* ctx = s->op->ctx;
  if (!s->initialised) return rls_fail(ctx, RLS_E_STATE, "cgnr_step before cgnr_init");
  if (n_steps < 0) return rls_fail(ctx, RLS_E_INVALID, "cgnr_step: n_steps < 0");
  if (queue && cgnr_listening_q(s) && (unsigned)n_steps <= RLS_Q_STEPS) {
    const int32_t r = cgnr_queue_step(s, n_steps);
    if (r <= 0) return r;  // (1: the plan left queue mode and this call has run its init!, if any: the steps go the ordinary way)
  }
  RLS_HIP(ctx, rls_enter(ctx));
  s->requested += n_steps;
  // queue mode starts on the second resident step call of back-to-back solves: no status read (resident_used) and no host wait for
  // the stream (ctx->syncs) since the plan's previous one.  The first call of a run is the plain single launch.
  if (queue && n_steps > 1 && (unsigned)n_steps <= RLS_Q_STEPS && cgnr_use_resident(s)) {
    if (s->resident.used && s->q_mark == ctx->syncs && cgnr_use_queue(s)) return cgnr_queue_launch(s, s->srv.seq + 1u, n_steps);
    s->q_mark = ctx->syncs;
  }
  return cgnr_step_impl(s, n_steps);
}
int32_t rls_cgnr_step(rls_cgnr* s, int32_t n_steps) { return cgnr_step_call(s, n_steps, true); }

// ---- K independent small systems in ONE launch (small.hip, rls_small_group) -----------------------------------------------------
// The distinct-A flavour of a multi-solve (docs/src/literate/howto/multi_threading.jl:8-17: one solver and one A per problem) for
// problems that each fit one CU's registers: every plan is an ordinary single-column plan on rls_cgnr_path 8; the group call
// advances them together, one workgroup per plan, optionally with their init! in the same launch.
static int32_t cgnr_group(rls_cgnr* const* plans, const void* const* b, int32_t count, float lambda, float rel_tol, int32_t iterations,
                          int32_t n_steps) {
  if (!plans || count < 1 || !plans[0]) return RLS_E_INVALID;
  rls_ctx* ctx = plans[0]->op->ctx;
  if (n_steps < 0) return rls_fail(ctx, RLS_E_INVALID, "cgnr group: n_steps < 0");
  const int32_t dtype = plans[0]->op->dtype;
  RLS_HIP(ctx, rls_enter(ctx));
  for (int32_t k = 0; k < count; ++k) {
    rls_cgnr* s = plans[k];
    if (!s || s->op->ctx != ctx || s->op->dtype != dtype) return rls_fail(ctx, RLS_E_INVALID, "cgnr group: plans of one context and one element type");
    if (!cgnr_use_small(s)) return rls_fail(ctx, RLS_E_UNSUPPORTED, "cgnr group: a plan is not on the small-system path (rls_cgnr_path 8)");
    if (!b && !s->initialised) return rls_fail(ctx, RLS_E_STATE, "cgnr group: step before init");
    if (b && !b[k]) return rls_fail(ctx, RLS_E_INVALID, "cgnr group: null right-hand side");
  }
  for (int32_t k0 = 0; k0 < count; k0 += RLS_SMALL_GROUP_MAX) {
    rls_small_group G;
    G.count = count - k0 < RLS_SMALL_GROUP_MAX ? count - k0 : RLS_SMALL_GROUP_MAX;
    for (int j = 0; j < G.count; ++j) {
      rls_cgnr* s = plans[k0 + j];
      rls_small& D = G.d[j] = cgnr_small_desc(s);
      if (b) {
        D.b = b[k0 + j];
        D.lambda = lambda;
        D.rel_tol = rel_tol;
        D.max_iter = cgnr_effective_iterations(s, iterations);
        s->sc_h->lambda = lambda;
        s->sc_h->rel_tol = rel_tol;
        s->sc_h->max_iter = D.max_iter;
        s->initialised = true;
        s->requested = 0;
      }
      s->requested += n_steps;
    }
    if (b || n_steps > 0) RLS_TRY(rls_small_group_launch(ctx, dtype, G, n_steps));
  }
  return 0;
}

// the statuses of a group in ONE read-back (one publishing kernel + one host spin per 24 plans instead of one per plan)
int32_t rls_cgnr_get_status_group(rls_cgnr* const* plans, int32_t count, rls_cgnr_status* out) {
  if (!plans || !out || count < 1 || !plans[0]) return RLS_E_INVALID;
  rls_ctx* ctx = plans[0]->op->ctx;
  RLS_HIP(ctx, rls_enter(ctx));
  for (int32_t k = 0; k < count; ++k) {
    rls_cgnr* s = plans[k];
    if (!s || s->op->ctx != ctx || s->nrhs != 1) return rls_fail(ctx, RLS_E_INVALID, "cgnr status group: single-column plans of one context");
    if (!s->initialised) return rls_fail(ctx, RLS_E_STATE, "cgnr_get_status before cgnr_init");
    if (s->resident.used) return rls_fail(ctx, RLS_E_UNSUPPORTED, "cgnr status group: a plan has resident launches to account for (use rls_cgnr_get_status)");
  }
  for (int32_t k0 = 0; k0 < count; k0 += RLS_FETCH_MAX) {
    const int32_t k1 = k0 + RLS_FETCH_MAX < count ? k0 + RLS_FETCH_MAX : count;
    for (int32_t k = k0; k < k1; ++k) RLS_TRY(rls_fetch_add(ctx, plans[k]->sc, plans[k]->sc_h, sizeof(cgnr_scalars)));
    RLS_TRY(rls_fetch_wait(ctx));
  }
  for (int32_t k = 0; k < count; ++k) cgnr_status_out(plans[k], *plans[k]->sc_h, out + k);
  return 0;
}

// ---- the distinct-A multi-solve as a queue (docs/src/literate/howto/multi_threading.jl:8-17: a solver AND an operator per task) ----
// `count` independent problems, each an ordinary single right-hand-side plan on its own operator (any shape, any kernel path; one
// context, hence one stream): problem k's init! (r = A_k^H b_k, x = 0, p = r: src/CGNR.jl:107-130) and all of its iterations
// (:143-178) are enqueued behind problem k - 1's, nothing is waited for in between, and ONE read-back at the end brings every
// problem's status.  A resident launch that was lost (its grid not on the chip in time) is re-run on the per-iteration pipeline
// exactly as rls_cgnr_get_status does it, for that problem alone.  The register-resident kernels need the whole chip each, so the
// problems run one after the other on the device -- what the queue removes is the host between them: per problem, plan creation,
// upload, a synchronising status call and a download (measured: 210 us of host per 320 us of kernels, round 5).
static int32_t cgnr_queue_validate(rls_cgnr* const* plans, int32_t count, rls_ctx** ctx_out) {
  if (!plans || count < 1 || !plans[0]) return RLS_E_INVALID;
  rls_ctx* ctx = plans[0]->op->ctx;
  for (int32_t k = 0; k < count; ++k) {
    const rls_cgnr* s = plans[k];
    if (!s || s->op->ctx != ctx || s->nrhs != 1)
      return rls_fail(ctx, RLS_E_INVALID, "cgnr solve queue: single right-hand-side plans of one context");
    for (int32_t j = 0; j < k; ++j)
      if (plans[j] == s) return rls_fail(ctx, RLS_E_INVALID, "cgnr solve queue: a plan appears twice (one plan per problem)");
  }
  *ctx_out = ctx;
  return 0;
}

// every plan's scalars (and, after resident launches, its sync block's flags) in as few publishing launches as the mailbox holds
static int32_t cgnr_queue_statuses(rls_ctx* ctx, rls_cgnr* const* plans, int32_t count, rls_cgnr_status* out) {
  constexpr int32_t PER = RLS_FETCH_MAX / 2;  // two read-backs per plan at most
  for (int32_t k0 = 0; k0 < count; k0 += PER) {
    const int32_t k1 = k0 + PER < count ? k0 + PER : count;
    for (int32_t k = k0; k < k1; ++k) RLS_TRY(status_fetch_add(ctx, plans[k], plans[k]->sc_h, 1));
    RLS_TRY(rls_fetch_wait(ctx));
  }
  for (int32_t k = 0; k < count; ++k) {
    rls_cgnr* s = plans[k];
    RLS_TRY(status_recover(ctx, s, s->sc_h, 1, [s](int32_t n) { return cgnr_step_impl(s, n); }, [](long long) {}));
    if (out) cgnr_status_out(s, *s->sc_h, out + k);
  }
  return 0;
}

int32_t rls_cgnr_solve_queue(rls_cgnr* const* plans, const void* const* b, int32_t count, float lambda, float rel_tol,
                             int32_t iterations, rls_cgnr_status* out) {
  rls_ctx* ctx = nullptr;
  RLS_TRY(cgnr_queue_validate(plans, count, &ctx));
  if (!b || iterations < 0) return rls_fail(ctx, RLS_E_INVALID, "cgnr solve queue: bad argument");
  for (int32_t k = 0; k < count; ++k) {
    RLS_TRY(rls_cgnr_init(plans[k], b[k], lambda, rel_tol, iterations));
    RLS_TRY(rls_cgnr_step(plans[k], iterations));
  }
  return cgnr_queue_statuses(ctx, plans, count, out);
}

// the same with b and x in HOST memory (the shape of the reference's task: host arrays in, host array out): b_k is staged through
// pinned memory and uploaded on the stream ahead of problem k's init, x_k is downloaded into pinned memory behind its last
// iteration -- every copy asynchronous, one synchronisation for the whole queue -- and handed to x_h[k] at the end.
int32_t rls_cgnr_solve_queue_host(rls_cgnr* const* plans, const void* const* b_h, void* const* x_h, int32_t count, float lambda,
                                  float rel_tol, int32_t iterations, rls_cgnr_status* out) {
  rls_ctx* ctx = nullptr;
  RLS_TRY(cgnr_queue_validate(plans, count, &ctx));
  if (!b_h || !x_h || iterations < 0) return rls_fail(ctx, RLS_E_INVALID, "cgnr solve queue: bad argument");
  RLS_HIP(ctx, rls_enter(ctx));
  for (int32_t k = 0; k < count; ++k) {
    rls_cgnr* s = plans[k];
    const rls_operator* op = s->op;
    const size_t es = rls_elem_size(op->dtype);
    const size_t bb = (size_t)(op->A ? op->M : op->N) * es, xb = (size_t)op->N * es;
    if (!b_h[k] || !x_h[k]) return rls_fail(ctx, RLS_E_INVALID, "cgnr solve queue: null buffer");
    if (!s->q_b) {  // all three or none: a later call finds either the whole staging or nothing
      rls_alloc_scope alloc_scope(ctx);
      const plan_buffers::mark_t m = s->mem.mark();
      s->mem.dev(&s->q_b, bb, false);
      s->mem.pinned(&s->q_bh, bb, false);
      s->mem.pinned(&s->q_xh, xb, false);
      if (const int e = s->mem.error()) {
        s->mem.rollback(m);
        return rls_fail(ctx, e, "cgnr solve queue: allocation failed");
      }
    }
    memcpy(s->q_bh, b_h[k], bb);
    RLS_HIP(ctx, hipMemcpyAsync(s->q_b, s->q_bh, bb, hipMemcpyHostToDevice, ctx->stream));
    RLS_TRY(rls_cgnr_init(s, s->q_b, lambda, rel_tol, iterations));
    RLS_TRY(rls_cgnr_step(s, iterations));
    RLS_HIP(ctx, hipMemcpyAsync(s->q_xh, s->x, xb, hipMemcpyDeviceToHost, ctx->stream));
  }
  RLS_TRY(cgnr_queue_statuses(ctx, plans, count, out));
  // a problem whose resident launch was lost has been re-run behind the queued download of its x: fetch that one again
  bool any = false;
  for (int32_t k = 0; k < count; ++k) {
    rls_cgnr* s = plans[k];
    if (s->resident.off && s->resident.fallbacks > 0) {
      RLS_HIP(ctx, hipMemcpyAsync(s->q_xh, s->x, (size_t)s->op->N * rls_elem_size(s->op->dtype), hipMemcpyDeviceToHost, ctx->stream));
      any = true;
    }
  }
  if (any) RLS_HIP(ctx, rls_stream_wait(ctx->stream));
  for (int32_t k = 0; k < count; ++k) memcpy(x_h[k], plans[k]->q_xh, (size_t)plans[k]->op->N * rls_elem_size(plans[k]->op->dtype));
  return 0;
}

int32_t rls_cgnr_step_group(rls_cgnr* const* plans, int32_t count, int32_t n_steps) {
  return cgnr_group(plans, nullptr, count, 0.f, 0.f, 0, n_steps);
}

int32_t rls_cgnr_init_step_group(rls_cgnr* const* plans, const void* const* b, int32_t count, float lambda, float rel_tol,
                                 int32_t iterations, int32_t n_steps) {
  if (!b) return RLS_E_INVALID;
  return cgnr_group(plans, b, count, lambda, rel_tol, iterations, n_steps);
}

// measurement only: the two kernels of the fused pipeline timed separately.  Each is idempotent
// when repeated (K_A reads the committed scalars and writes the staged ones, K_R the reverse), so
// after one ordinary iteration the normal-operator kernel is launched n_steps times back to back
// between two hipEvents, then the reduce kernel likewise; the averages are what rocprofv3 reports
// for back-to-back dispatches.  The solver state afterwards is that of ONE more iteration.
int32_t rls_cgnr_step_profiled(rls_cgnr* s, int32_t n_steps, float* us_normal, float* us_reduce) {
  if (!s || !us_normal || !us_reduce || n_steps <= 0) return RLS_E_INVALID;
  rls_ctx* ctx = s->op->ctx;
  if (!s->initialised) return rls_fail(ctx, RLS_E_STATE, "cgnr_step_profiled before cgnr_init");
  if (!cgnr_use_pipeline(s)) return rls_fail(ctx, RLS_E_UNSUPPORTED, "cgnr_step_profiled: fused pipeline not active");
  RLS_HIP(ctx, rls_enter(ctx));
  rls_cgnr_pipe P = cgnr_pipe_desc(s);
  const int32_t dtype = s->op->dtype;
  RLS_TRY(rls_cgnr_pipe_iteration(ctx, dtype, P));  // leaves an update pending: K_A then does full work
  P.cur_hint = 0;  // ... on pair 0, every time (the reduce kernel that would commit the flip is not run in between)
  hipEvent_t ev[3];
  for (auto& e : ev) RLS_HIP(ctx, hipEventCreate(&e));
  int32_t st = 0;
  RLS_HIP(ctx, hipEventRecord(ev[0], ctx->stream));
  for (int i = 0; i < n_steps && st == 0; ++i) st = rls_cgnr_pipe_launch(ctx, dtype, P, 1);
  RLS_HIP(ctx, hipEventRecord(ev[1], ctx->stream));
  for (int i = 0; i < n_steps && st == 0; ++i) st = rls_cgnr_pipe_launch(ctx, dtype, P, 2);
  RLS_HIP(ctx, hipEventRecord(ev[2], ctx->stream));
  RLS_HIP(ctx, rls_event_wait(ev[2]));
  float a = 0.f, r = 0.f;
  RLS_HIP(ctx, hipEventElapsedTime(&a, ev[0], ev[1]));
  RLS_HIP(ctx, hipEventElapsedTime(&r, ev[1], ev[2]));
  for (auto& e : ev) hipEventDestroy(e);
  if (st != 0) return st;
  RLS_TRY(rls_cgnr_pipe_finish(ctx, dtype, P));
  *us_normal = 1e3f * a / n_steps;
  *us_reduce = 1e3f * r / n_steps;
  return 0;
}

// ---- row-partitioned solvers through a communicator (comm.hip): the collective lives inside the library ----------------
// Every loop below is a list of PHASES run by rls_comm_run: each rank's worker thread walks the whole list for its rank
// (src/MultiThreading.jl:60-78's Threads.@threads, inside the library), meeting the others at a host barrier wherever
// one rank's stream must not wait on an event another rank has not recorded yet -- i.e. between "publish" and "collect"
// of an all-reduce round.  The host side of an iteration therefore costs one rank's launches, not n ranks'.
int32_t rls_cgnr_init_rowsharded(rls_comm* comm, rls_cgnr* const* plans, const void* const* b_parts, float lambda,
                                 float rel_tol, int32_t iterations) {
  RLS_TRY(rowsharded_check<rls_cgnr>(comm, plans, cgnr_op, cgnr_single));
  if (!b_parts) return RLS_E_INVALID;
  const int64_t N = plans[0]->op->N;
  const int32_t dtype = plans[0]->op->dtype;
  int round0 = 0;
  RLS_TRY(rls_comm_next_rounds(comm, 1, N, dtype, &round0));
  const std::vector<rls_comm_phase> phases = {
      {[&](int r, int) {  // r_g = A_g^H b_g
         RLS_TRY(rls_cgnr_init_local_a(plans[r], b_parts[r], lambda, rel_tol, iterations));
         return rls_comm_publish(comm, r, plans[r]->r, N, dtype, round0);
       }, true},
      {[&](int r, int) {  // r = sum_g r_g, then the replicated rest of initCGNR
         RLS_TRY(rls_comm_collect(comm, r, plans[r]->r, N, dtype, round0));
         return rls_cgnr_init_local_b(plans[r]);
       }, false}};
  return rls_comm_run(comm, phases, 1);
}

int32_t rls_cgnr_step_rowsharded(rls_comm* comm, rls_cgnr* const* plans, int32_t n_steps) {
  RLS_TRY(rowsharded_check<rls_cgnr>(comm, plans, cgnr_op, cgnr_single));
  if (n_steps < 0) return RLS_E_INVALID;
  const int64_t N = plans[0]->op->N;
  const int32_t dtype = plans[0]->op->dtype;
  int round0 = 0;
  RLS_TRY(rls_comm_next_rounds(comm, n_steps, N, dtype, &round0));
  const std::vector<rls_comm_phase> phases = {
      {[&](int r, int k) {  // t_g = A_g p, v_g = A_g^H t_g
         RLS_TRY(rls_cgnr_step_local_a(plans[r]));
         return rls_comm_publish(comm, r, plans[r]->v, N, dtype, round0 + k);
       }, true},
      {[&](int r, int k) {  // v = sum_g v_g, the replicated update.  No barrier behind it: a rank can run at most one round
         RLS_TRY(rls_comm_collect(comm, r, plans[r]->v, N, dtype, round0 + k));  // ahead, and the rounds alternate buffers
         return rls_cgnr_step_local_b(plans[r]);
       }, false}};
  return rls_comm_run(comm, phases, n_steps);
}

int32_t rls_cgnr_path(rls_cgnr* s, int32_t* out) {
  if (!s || !out) return RLS_E_INVALID;
  *out = cgnr_use_small(s) ? 8 : s->skinny ? (cgnr_use_gramk(s, 0) ? 7 : s->op->G ? 6 : 3) : cgnr_use_gram_resident(s) ? 5 : cgnr_use_gram_pipeline(s) ? 2 : cgnr_use_resident(s) ? 4 : cgnr_use_pipeline(s) ? 1 : 0;
  return 0;
}

int32_t rls_cgnr_step_local_a(rls_cgnr* s) {
  if (!s) return RLS_E_INVALID;
  if (!s->initialised) return rls_fail(s->op->ctx, RLS_E_STATE, "cgnr_step before cgnr_init");
  RLS_HIP(s->op->ctx, hipSetDevice(s->op->ctx->device));
  return op_normal(s->op, s->p, s->v, &s->sc->done);
}
int32_t rls_cgnr_step_local_b(rls_cgnr* s) {
  if (!s) return RLS_E_INVALID;
  if (!s->initialised) return rls_fail(s->op->ctx, RLS_E_STATE, "cgnr_step before cgnr_init");
  RLS_HIP(s->op->ctx, hipSetDevice(s->op->ctx->device));
  return cgnr_enqueue_update(s);
}

int32_t rls_cgnr_get_status(rls_cgnr* s, rls_cgnr_status* out) {
  if (!s || !out) return RLS_E_INVALID;
  rls_ctx* ctx = s->op->ctx;
  if (!s->initialised) return rls_fail(ctx, RLS_E_STATE, "cgnr_get_status before cgnr_init");
  if (ctx->server == &s->srv && s->srv.alive && s->srv.fresh) {  // a kernel left listening: the mirror holds its last command's status
    cgnr_status_out(s, *s->sc_h, out);
    return 0;
  }
  RLS_HIP(ctx, rls_enter(ctx));
  RLS_TRY(cgnr_fetch_status(s, 1));
  cgnr_status_out(s, *s->sc_h, out);
  return 0;
}

static void cgnr_status_out(const rls_cgnr* s, const cgnr_scalars& h, rls_cgnr_status* out) {
  out->iteration = h.iteration;
  out->done = h.done;
  out->alpha_re = (float)h.alpha_re;
  out->alpha_im = (float)h.alpha_im;
  out->beta_re = (float)h.beta_re;
  out->beta_im = (float)h.beta_im;
  out->zeta = (float)h.zeta;
  out->residual = (float)sqrt(h.rr);
  out->z0 = (float)h.z0;
  out->fallbacks = s->resident.fallbacks;
}

extern "C++" {
static bool cgnr_use_server(const rls_cgnr* s) {
  return server_usable(s->op->ctx, &s->srv) &&
         (cgnr_use_small(s) || cgnr_use_resident(s) || (cgnr_use_gram_resident(s) && s->nrhs == 1));
}

// ---- queue mode: back-to-back solves served by ONE resident launch that keeps A in its registers ---------------------------------
// The first resident step call of a run is the plain launch; the second (no status read, no host wait in between: rls_cgnr_step)
// launches the QUEUE instantiation, which stays when its command is done.  From then on rls_cgnr_init + rls_cgnr_step post ONE
// command {INIT b, lambda, relTol, maxiter; STEP n} into the ring behind the control block and return; rls_cgnr_step alone posts
// {STEP n}.  Every other entry point goes through rls_enter, which posts EXIT behind the queued commands and waits until the kernel
// has left: stream order for everything the caller can observe.  b must be final on the device when rls_cgnr_init is called.
static bool cgnr_use_queue(const rls_cgnr* s) {
  const rls_ctx* ctx = s->op->ctx;
  return s->q_ok && ctx->tune.resident_queue && ctx->tune.resident_server && !s->srv.off &&
         (ctx->server == nullptr || ctx->server == &s->srv) && cgnr_use_resident(s);
}
static bool cgnr_listening_q(const rls_cgnr* s) {
  const srv_state& v = s->srv;
  return s->op->ctx->server == &v && v.alive && v.queue && s->op->ctx->tune.resident_queue;
}
// a new life of the queue instantiation: its first command (seq0, n_steps) travels as launch arguments; a life that takes over
// the commands left in the ring starts at the last one done with n_steps = 0
static int32_t cgnr_queue_launch(rls_cgnr* s, unsigned seq0, int32_t n_steps) {
  rls_ctx* ctx = s->op->ctx;
  srv_state* v = &s->srv;
  volatile unsigned* ctl = v->ctl;
  ctl[16] = ctl[17] = 0;
  if (n_steps > 0) {  // (a fresh command)
    ctl[RLS_Q_DONE] = seq0 - 1u;
    v->seq = v->q_last = seq0;
  }
  rls_cg_start St;
  St.srv_ctl = v->ctl;
  St.srv_seq0 = seq0;
  St.srv_idle_us = (unsigned)(ctx->tune.resident_server_idle_us > 0 ? ctx->tune.resident_server_idle_us : 1) | RLS_SRV_QUEUE;
  const rls_cgnr_pipe P = cgnr_pipe_desc(s);
  RLS_TRY(s->resident.launch(ctx, [&](void* sync, unsigned spin) {
    return rls_cgnr_resident_launch(ctx, s->op->dtype, P, s->rdots, sync, n_steps, spin, St);
  }));
  v->alive = true;
  v->queue = true;
  v->served = (int)(v->q_last - seq0) + (n_steps > 0 ? 1 : 0);
  ctx->server = v;
  return 0;
}
// one command on the ordinary path (init! by GEMV + init kernel, the steps by whatever cgnr_step_impl picks)
static int32_t cgnr_queue_ordinary(rls_cgnr* s, unsigned cmd, const unsigned* pay) {
  if (cmd & RLS_Q_INIT) {
    const void* b = reinterpret_cast<const void*>((uintptr_t)pay[1] | ((uintptr_t)pay[2] << 32));
    const long long req = s->requested;
    const bool off = s->srv.off;
    RLS_TRY(rls_cgnr_init_local_a(s, b, __builtin_bit_cast(float, pay[3]), __builtin_bit_cast(float, pay[4]), (int32_t)pay[0]));
    RLS_TRY(rls_cgnr_init_local_b(s));
    s->requested = req;
    s->srv.off = off;
  }
  const int32_t n = (int32_t)(cmd & RLS_Q_STEPS);
  return n > 0 ? cgnr_step_impl(s, n) : 0;
}
// The life has left (ctl[17]): the commands posted after the last one it finished are served by a new life -- or, behind a wait
// that ran out (a lost launch) or when lives keep ending early, one by one on the ordinary path.  Leaves v->alive as the new state.
static int32_t cgnr_queue_resume(rls_cgnr* s) {
  rls_ctx* ctx = s->op->ctx;
  srv_state* v = &s->srv;
  volatile unsigned* ctl = v->ctl;
  const bool gave_up = ctl[17] == 2;
  const unsigned done = ctl[RLS_Q_DONE];
  server_life_over(ctx, v);
  v->queue = false;
  if (done == v->q_last) return 0;
  if (!gave_up && cgnr_use_queue(s)) return cgnr_queue_launch(s, done, 0);
  if (gave_up) s->resident.off = true;  // (the status call behind it reads the lost launch from the sync block: resident_slot::lost)
  for (unsigned q = done + 1u; q != v->q_last + 1u; ++q) {
    const volatile unsigned* sl = v->ctl + RLS_Q_RING_OFF + (q % RLS_Q_RING) * RLS_Q_SLOT_WORDS;
    const unsigned pay[5] = {sl[2], sl[4], sl[6], sl[8], sl[10]};
    RLS_TRY(cgnr_queue_ordinary(s, sl[0], pay));
  }
  return 0;
}
// Posts one command to the ring of the listening life.  0: posted (or, the life being gone, already served another way);
// 1: the plan has left queue mode before the command could be posted (the caller runs it on the ordinary path); < 0: error.
static int32_t cgnr_queue_post(rls_cgnr* s, unsigned cmd, const unsigned (&pay)[5]) {
  rls_ctx* ctx = s->op->ctx;
  srv_state* v = &s->srv;
  volatile unsigned* ctl = v->ctl;
  const unsigned seq = v->seq + 1u;
  auto t0 = std::chrono::steady_clock::now();
  // a free slot: the command RLS_Q_RING before this one is done (bounded: behind 2 s the host waits for the stream, which ends the
  // life at its idle time at the latest)
  for (unsigned n = 0; seq - ctl[RLS_Q_DONE] > RLS_Q_RING; ++n) {
    if (ctl[17]) {
      RLS_TRY(cgnr_queue_resume(s));
      if (!v->alive) return 1;
      t0 = std::chrono::steady_clock::now();
      continue;
    }
    rls_cpu_relax();
    if ((n & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) {
      (void)hipSetDevice(ctx->device);
      (void)hipStreamSynchronize(ctx->stream);
      if (!ctl[17]) ctl[17] = 2;  // (nothing left running on the stream: the life is over whatever it said)
    }
  }
  // six 8-byte halves {payload, sequence number}, each ONE store: the kernel takes the slot once all six carry `seq`
  volatile unsigned long long* sl = reinterpret_cast<volatile unsigned long long*>(v->ctl + RLS_Q_RING_OFF + (seq % RLS_Q_RING) * RLS_Q_SLOT_WORDS);
  const unsigned w[6] = {cmd, pay[0], pay[1], pay[2], pay[3], pay[4]};
  for (int i = 0; i < 6; ++i) sl[i] = ((unsigned long long)seq << 32) | w[i];
  v->seq = seq;
  if (cmd != RLS_SRV_EXIT) v->q_last = seq;
  v->served += 1;
  std::atomic_thread_fence(std::memory_order_seq_cst);
  // a life that is leaving (idle, life cap) either takes this command (and says so by clearing "leaving") or leaves
  t0 = std::chrono::steady_clock::now();
  for (unsigned n = 0; ctl[16] || ctl[17]; ++n) {
    if (ctl[17]) return cgnr_queue_resume(s);
    rls_cpu_relax();
    if ((n & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(500)) {
      (void)hipSetDevice(ctx->device);
      (void)hipStreamSynchronize(ctx->stream);
      if (!ctl[17]) ctl[17] = 2;
    }
  }
  return 0;
}
static int32_t cgnr_queue_init(rls_cgnr* s, const void* b, float lambda, float rel_tol, int32_t iterations) {
  srv_state* v = &s->srv;
  if (v->q_pending) {  // an init! nobody stepped: it still sets the plan's state
    v->q_pending = false;
    const int32_t r = cgnr_queue_post(s, RLS_Q_INIT, v->q_pay);
    if (r < 0) return r;
    if (r == 1) RLS_TRY(cgnr_queue_ordinary(s, RLS_Q_INIT, v->q_pay));
    if (!cgnr_listening_q(s)) return rls_cgnr_init(s, b, lambda, rel_tol, iterations);
  }
  const int max_iter = cgnr_effective_iterations(s, iterations);
  const uintptr_t bp = reinterpret_cast<uintptr_t>(b);
  v->q_pay[0] = (unsigned)max_iter;
  v->q_pay[1] = (unsigned)bp;
  v->q_pay[2] = (unsigned)(bp >> 32);
  v->q_pay[3] = __builtin_bit_cast(unsigned, lambda);
  v->q_pay[4] = __builtin_bit_cast(unsigned, rel_tol);
  v->q_pending = true;
  s->sc_h->lambda = lambda;
  s->sc_h->rel_tol = rel_tol;
  s->sc_h->max_iter = max_iter;
  s->initialised = true;
  s->requested = 0;
  return 0;
}
// 0: posted; 1: the plan left queue mode (its pending init!, if any, has run): the caller runs the steps the ordinary way
static int32_t cgnr_queue_step(rls_cgnr* s, int32_t n_steps) {
  srv_state* v = &s->srv;
  static const unsigned none[5] = {0u, 0u, 0u, 0u, 0u};
  const bool init = v->q_pending;
  if (!init && n_steps == 0) return 0;
  unsigned pay[5];
  for (int i = 0; i < 5; ++i) pay[i] = init ? v->q_pay[i] : none[i];
  const unsigned cmd = (unsigned)n_steps | (init ? RLS_Q_INIT : 0u);
  v->q_pending = false;
  const long long req = s->requested;
  s->requested += n_steps;
  const int32_t r = cgnr_queue_post(s, cmd, pay);
  if (r != 1) return r;
  s->requested = req;
  if (init) RLS_TRY(cgnr_queue_ordinary(s, RLS_Q_INIT, pay));
  return 1;
}
// rls_enter on a queue life: the pending init!, then EXIT behind everything posted; a life that leaves before it reaches the EXIT
// hands the rest to the next (cgnr_queue_resume) until all is done
void cgnr_queue_stop(rls_ctx* ctx, srv_state* v) {
  rls_cgnr* s = static_cast<rls_cgnr*>(v->q_plan);
  static const unsigned none[5] = {0u, 0u, 0u, 0u, 0u};
  if (v->q_pending) {
    v->q_pending = false;
    const unsigned pay[5] = {v->q_pay[0], v->q_pay[1], v->q_pay[2], v->q_pay[3], v->q_pay[4]};
    const int32_t r = cgnr_queue_post(s, RLS_Q_INIT, pay);
    if (r == 1) (void)cgnr_queue_ordinary(s, RLS_Q_INIT, pay);
    if (r != 0) return;
  }
  if (!v->alive) return;
  if (cgnr_queue_post(s, RLS_SRV_EXIT, none) != 0) return;
  volatile unsigned* ctl = v->ctl;
  for (int lives = 0; v->alive && v->queue && lives < 1024; ++lives) {
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned n = 0; !ctl[17]; ++n) {
      rls_cpu_relax();
      if ((n & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(500)) {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);  // (its idle timeout or its wait bounds end it at the latest)
        if (!ctl[17]) ctl[17] = 2;
      }
    }
    if (cgnr_queue_resume(s) != 0) break;
  }
  if (ctx->server == v) ctx->server = nullptr;
}
}  // extern "C++"

int32_t rls_cgnr_step_status(rls_cgnr* s, int32_t n_steps, rls_cgnr_status* out) {
  if (!s || !out) return RLS_E_INVALID;
  rls_ctx* ctx = s->op->ctx;
  if (cgnr_listening_q(s)) rls_server_stop(ctx);  // (queue mode: the calls of a solve! loop with callbacks take their own path)
  auto serve_launch = [&](const rls_srv_args& a) {
    rls_cg_start St;
    St.srv_ctl = a.ctl;
    St.srv_seq0 = a.seq0;
    St.srv_idle_us = a.idle_us & ~RLS_SRV_AHEAD;
    St.srv_mb = a.mb;
    if (cgnr_use_small(s)) {  // the single-workgroup kernel: one CU stays, nothing to chain
      rls_small D = cgnr_small_desc(s);
      D.mb = a.mb;
      D.srv = a;
      return rls_small_launch(ctx, s->op->dtype, D, n_steps);
    }
    if (cgnr_use_gram_resident(s)) {  // AHA explicit, held in the register files
      const rls_gram_pipe G = cgnr_gram_desc(s);
      return s->resident.chain(ctx, [&](void* sync, unsigned spin) {
        return rls_gram_resident_launch(ctx, s->op->dtype, G, sync, n_steps, spin, St);
      });
    }
    const rls_cgnr_pipe P = cgnr_pipe_desc(s);
    return s->resident.chain(ctx, [&](void* sync, unsigned spin) {
      return rls_cgnr_resident_launch(ctx, s->op->dtype, P, s->rdots, sync, n_steps, spin, St);
    });
  };
  return step_status(s, n_steps, out, cgnr_use_server(s), serve_launch, [s](int32_t n) { s->requested += n; },
                     [](rls_cgnr* p, int32_t n) { return cgnr_step_call(p, n, false); }, rls_cgnr_get_status, cgnr_status_out);
}

// ---- cg! ------------------------------------------------------------------------------------
int32_t rls_cg_create(rls_operator* op, void* u, void* r, void* c, rls_cg** out) {
  if (!op) return RLS_E_INVALID;
  rls_ctx* ctx = op->ctx;
  if (!u || !r || !c || !out) return rls_fail(ctx, RLS_E_INVALID, "cg_create: null pointer");
  RLS_HIP(ctx, rls_enter(ctx));
  *out = nullptr;
  rls_alloc_scope alloc_scope(ctx);
  rls_cg* s = new rls_cg{plan_memory(ctx)};
  plan_buffers& mem = s->mem;
  s->op = op;
  s->actx = ctx;
  s->actx_id = ctx->id;
  s->device = op->ctx->device;
  s->u = u;
  s->r = r;
  s->c = c;
  alloc_scalars(mem, &s->sc, &s->sc_h);
  if (op->G && rls_gram_pipe_ok(op->dtype, op->N, op->G, op->ldg)) {
    const size_t vb = (size_t)op->N * rls_elem_size(op->dtype);
    const size_t nd = (size_t)2 * rls_gram_pipe_nwg(op->dtype, op->N) * 4 * sizeof(double);
    mem.dev(&s->r1, vb, false);
    mem.dev(&s->p1, vb, false);
    mem.dev(&s->v1, vb, true);
    mem.dev(&s->gdots, nd, true);
    mem.dev(&s->pscn, sizeof(cgnr_scalars), true);
    alloc_scalars(mem, &s->psc, &s->psc_h);
    if (!mem.error() && rls_gram_resident_ok(ctx, op->dtype, op->N, op->G, op->ldg)) {
      const plan_buffers::mark_t m = mem.mark();
      s->resident.alloc(mem, ctx, op);
      s->gram_resident = !mem.error();
      if (!s->gram_resident) {
        mem.rollback(m);  // an optimisation only: the one-launch-per-iteration pipeline runs without it
        (void)hipGetLastError();
      }
    }
  } else if (op->slab) {
    if (!mem.error() && op->A && rls_cgnr_resident_ok(ctx, op->dtype, op->M, op->N, op->A, op->lda)) {
      const plan_buffers::mark_t m = mem.mark();
      s->resident.alloc(mem, ctx, op);
      mem.dev(&s->rdots, (size_t)rls_cgnr_resident_nwg(op->ctx, op->dtype, op->M, op->N) * 4 * sizeof(double), false);
      if (mem.error()) {
        mem.rollback(m);  // an optimisation only: the two-launch pipeline runs without it
        (void)hipGetLastError();
      }
    }
    mem.dev(&s->r1, (size_t)op->N * rls_elem_size(op->dtype), false);
    mem.dev(&s->p1, (size_t)op->N * rls_elem_size(op->dtype), false);
    mem.dev(&s->dots, (size_t)((op->N + 15) / 16) * 4 * sizeof(double), true);
    mem.dev(&s->pscn, sizeof(cgnr_scalars), true);
    alloc_scalars(mem, &s->psc, &s->psc_h);
  }
  if (const int e = mem.error()) {
    rls_cg_destroy(s);
    return rls_fail(ctx, e, "cg_create: hipMalloc failed");
  }
  *out = s;
  return 0;
}

// K right-hand sides sharing A (solve!(solver::ADMM, B) with the shared-A scheduler; src/MultiThreading.jl:30-79 applies
// to every solver): U, R, C are N x nrhs scratch matrices (the CGStateVariables of every column, src/ADMM.jl:129)
int32_t rls_cg_create_batched(rls_operator* op, int32_t nrhs, void* U, void* R, void* Cm, int64_t ldv, rls_cg** out) {
  if (!op) return RLS_E_INVALID;
  rls_ctx* ctx = op->ctx;
  if (!U || !R || !Cm || !out || nrhs < 1 || ldv < op->N) return rls_fail(ctx, RLS_E_INVALID, "cg_create_batched: bad argument");
  if (!shared_operands::supported(op))
    return rls_fail(ctx, RLS_E_UNSUPPORTED, "cg_create_batched: needs A (and AHA, when explicit) with M, N multiples of 16");
  RLS_HIP(ctx, rls_enter(ctx));
  *out = nullptr;
  rls_alloc_scope alloc_scope(ctx);
  rls_cg* s = new rls_cg{plan_memory(ctx)};
  plan_buffers& mem = s->mem;
  s->op = op;
  s->actx = ctx;
  s->actx_id = ctx->id;
  s->device = ctx->device;
  s->u = U;
  s->r = R;
  s->c = Cm;
  s->nrhs = nrhs;
  s->ldv = ldv;
  s->ops.alloc(mem, op, nrhs);
  alloc_scalars(mem, &s->sc, &s->sc_h, nrhs);
  if (const int e = mem.error()) {
    rls_cg_destroy(s);
    return rls_fail(ctx, e, "cg_create_batched: allocation failed");
  }
  *out = s;
  return 0;
}

int32_t rls_cg_destroy(rls_cg* s) {
  if (!s) return RLS_E_INVALID;
  hipSetDevice(s->device);
  rls_alloc_scope alloc_scope(alloc_ctx_of(s->actx, s->actx_id));
  s->graph.drop();
  s->mem.release();
  delete s;
  return 0;
}

int32_t rls_cg_solve(rls_cg* s, void* x, const void* b, float rho, int32_t maxiter, float reltol) {
  if (!s) return RLS_E_INVALID;
  rls_ctx* ctx = s->op->ctx;
  if (!x || !b || maxiter < 0) return rls_fail(ctx, RLS_E_INVALID, "cg_solve: bad argument");
  if (s->nrhs != 1) return rls_fail(ctx, RLS_E_STATE, "cg_solve on a batched plan: batched cg! runs inside rls_admm_step");
  RLS_HIP(ctx, rls_enter(ctx));
  s->last.x = x;
  s->last.b = b;
  s->last.rho = rho;
  s->last.reltol = reltol;
  s->last.maxiter = maxiter;
  s->last.valid = true;
  return cg_solve_impl(s, x, b, rho, maxiter, reltol, admm_fuse_v());
}

// row-sharded cg! (ADMM on a row-partitioned A): the operator apply and the update are separate calls with the
// caller's all-reduce of c between them; the unfused scalars / kernels, `done` on the device as usual
//   rls_cg_local_apply(s, x)      c_partial = A_g^H A_g x        (warm start; null = the direction u, skipped once done)
//   rls_cg_local_start(...)       r = b - (c + rho x), u = r, residual, tol
//   rls_cg_local_update(s, x)     alpha, x, r, residual, next direction
int32_t rls_cg_local_apply(rls_cg* s, const void* x) {
  if (!s) return RLS_E_INVALID;
  rls_ctx* ctx = s->op->ctx;
  RLS_HIP(ctx, rls_enter(ctx));
  return x ? op_normal(s->op, x, s->c, nullptr) : op_normal(s->op, s->u, s->c, &s->sc->done);
}

int32_t rls_cg_local_start(rls_cg* s, const void* x, const void* b, float rho, int32_t maxiter, float reltol) {
  if (!s) return RLS_E_INVALID;
  rls_operator* op = s->op;
  rls_ctx* ctx = op->ctx;
  if (!x || !b || maxiter < 0) return rls_fail(ctx, RLS_E_INVALID, "cg_local_start: bad argument");
  RLS_HIP(ctx, rls_enter(ctx));
  s->used_pipeline = false;
  return rls_with_elem(op->dtype, [&](auto t) {
    using E = typename decltype(t)::type;
    return rls_launch<cg_start_kernel<E>>(ctx, dim3(1), dim3(UPD_THREADS), 0, (const E*)x, (const E*)b, (E*)s->u, (E*)s->r,
                                          (const E*)s->c, op->N, s->sc, rho, reltol, maxiter, typed_fuse<E>(admm_fuse_v()),
                                          col_batch<E>());
  });
}

int32_t rls_cg_local_update(rls_cg* s, void* x) {
  if (!s) return RLS_E_INVALID;
  rls_operator* op = s->op;
  rls_ctx* ctx = op->ctx;
  if (!x) return rls_fail(ctx, RLS_E_INVALID, "cg_local_update: null x");
  RLS_HIP(ctx, rls_enter(ctx));
  return rls_with_elem(op->dtype, [&](auto t) {
    using E = typename decltype(t)::type;
    return rls_launch<cg_update_kernel<E>>(ctx, dim3(1), dim3(UPD_THREADS), 0, (E*)x, (E*)s->u, (E*)s->r, (E*)s->c, op->N, s->sc,
                                           col_batch<E>());
  });
}

int32_t rls_cg_path(rls_cg* s, int32_t* out) {
  if (!s || !out) return RLS_E_INVALID;
  const rls_ctx* ctx = s->op->ctx;
  const bool res = s->resident.usable(ctx);
  if (s->nrhs > 1 || s->ops.allocated()) *out = 3;
  else if (cg_use_gram_pipeline(s)) *out = (res && s->gram_resident) ? 5 : 2;
  else if (cg_use_pipeline(s)) *out = res ? 4 : 1;
  else *out = 0;
  return 0;
}

int32_t rls_cg_get_status(rls_cg* s, rls_cg_status* out) {
  if (!s || !out) return RLS_E_INVALID;
  rls_ctx* ctx = s->op->ctx;
  RLS_HIP(ctx, rls_enter(ctx));
  if (s->resident.used) {
    // a lost resident launch left x at its warm start: repeat the solve on the per-iteration pipeline
    RLS_TRY(s->resident.fetch_flags(ctx));
    RLS_TRY(rls_fetch_wait(ctx));
    if (s->resident.lost(ctx) && s->last.valid)
      RLS_TRY(cg_solve_impl(s, s->last.x, s->last.b, s->last.rho, s->last.maxiter, s->last.reltol, admm_fuse_v()));
  }
  out->fallbacks = s->resident.fallbacks;
  if (s->used_pipeline) {
    RLS_TRY(fetch_scalars(ctx, s->psc, s->psc_h));
    out->iterations = s->psc_h->iteration;
    out->residual = (float)sqrt(s->psc_h->rr);
    out->tol = s->psc_h->rel_tol * (float)s->psc_h->z0;
    return 0;
  }
  RLS_TRY(fetch_scalars(ctx, s->sc, s->sc_h));
  out->iterations = s->sc_h->iteration;
  out->residual = (float)s->sc_h->residual;
  out->tol = (float)s->sc_h->tol;
  return 0;
}

// ---- ADMM fused elementwise steps (identity regTrafo) ----------------------------------------
int32_t rls_admm_pre(rls_ctx* ctx, int32_t dtype, int64_t n, void* beta, const void* beta_y, const void* z,
                     const void* u, const void* x, void* xold, float rho, int32_t accumulate) {
  RLS_CHECK_CTX(ctx);
  if (!rls_dtype_ok(dtype) || n < 0 || (n > 0 && (!beta || !beta_y || !z || !u || !x || !xold)))
    return rls_fail(ctx, RLS_E_INVALID, "admm_pre: bad argument");
  if (n == 0) return 0;
  RLS_HIP(ctx, rls_enter(ctx));
  unsigned grid = (unsigned)((n + 255) / 256);
  if (grid > 2048) grid = 2048;
  return rls_with_elem(dtype, [&](auto t) {
    using E = typename decltype(t)::type;
    return rls_launch<admm_pre_kernel<E>>(ctx, dim3(grid), dim3(256), 0, (E*)beta, (const E*)beta_y, (const E*)z, (const E*)u,
                                          (const E*)x, (E*)xold, n, rho, accumulate);
  });
}

int32_t rls_admm_post(rls_ctx* ctx, int32_t dtype, int64_t n, const void* x, const void* xold, const void* z,
                      const void* zold, void* u, float* out_h) {
  RLS_CHECK_CTX(ctx);
  if (!rls_dtype_ok(dtype) || n <= 0 || !x || !xold || !z || !zold || !u || !out_h)
    return rls_fail(ctx, RLS_E_INVALID, "admm_post: bad argument");
  RLS_HIP(ctx, rls_enter(ctx));
  RLS_TRY(rls_with_elem(dtype, [&](auto t) {
    using E = typename decltype(t)::type;
    return rls_launch<admm_post_kernel<E>>(ctx, dim3(1), dim3(UPD_THREADS), 0, (const E*)x, (const E*)xold, (const E*)z,
                                           (const E*)zold, (E*)u, n, ctx->res_d);
  }));
  RLS_HIP(ctx, hipMemcpyAsync(ctx->res_h, ctx->res_d, sizeof(float) * 6, hipMemcpyDeviceToHost, ctx->stream));
  RLS_HIP(ctx, rls_stream_wait(ctx->stream));
  for (int i = 0; i < 6; ++i) out_h[i] = ctx->res_h[i];
  return 0;
}

// ---- ADMM plan ------------------------------------------------------------------------------
int32_t rls_admm_create(rls_cg* cg, rls_admm** out) {
  if (!cg) return RLS_E_INVALID;
  rls_ctx* ctx = cg->op->ctx;
  if (!out) return rls_fail(ctx, RLS_E_INVALID, "admm_create: null out");
  RLS_HIP(ctx, rls_enter(ctx));
  rls_alloc_scope alloc_scope(ctx);
  *out = nullptr;
  rls_admm* a = new rls_admm{plan_memory(ctx)};
  a->cg = cg;
  a->actx = ctx;
  a->actx_id = ctx->id;
  a->device = ctx->device;
  a->nrhs = cg->nrhs;
  alloc_scalars(a->mem, &a->sc, &a->sc_h, cg->nrhs);
  if (const int e = a->mem.error()) {
    rls_admm_destroy(a);
    return rls_fail(ctx, e, "admm_create: allocation failed");
  }
  a->log_mark = a->mem.mark();
  *out = a;
  return 0;
}

int32_t rls_admm_destroy(rls_admm* a) {
  if (!a) return RLS_E_INVALID;
  hipSetDevice(a->device);
  rls_alloc_scope alloc_scope(alloc_ctx_of(a->actx, a->actx_id));
  a->mem.release();
  delete a;
  return 0;
}

int32_t rls_admm_init(rls_admm* a, const rls_admm_params* p) {
  if (!a) return RLS_E_INVALID;
  rls_ctx* ctx = a->cg->op->ctx;
  a->ready = false;
  if (!p || !p->x || !p->xold || !p->beta || !p->beta_y || !p->z0 || !p->z1 || !p->u || p->iterations < 0 ||
      p->iterations_cg < 0)
    return rls_fail(ctx, RLS_E_INVALID, "admm_init: bad argument");
  const int32_t dtype = a->cg->op->dtype;
  switch (p->reg_kind) {
    case RLS_REG_NONE:
    case RLS_REG_L1:
    case RLS_REG_L2:
      break;
    case RLS_REG_TV:
      if (p->proj_kind != RLS_PROJ_NONE || p->tv_iterations < 0 ||
          !rls_tv_single_ok(ctx, dtype, p->tv_ndims, p->tv_shape, p->tv_ntv, p->tv_dims))
        return rls_fail(ctx, RLS_E_UNSUPPORTED, "admm_init: TV prox does not fit the single-workgroup FGP kernel");
      {
        int64_t n = 1;
        for (int k = 0; k < p->tv_ndims; ++k) n *= p->tv_shape[k];
        if (n != a->cg->op->N) return rls_fail(ctx, RLS_E_INVALID, "admm_init: prod(shape) != N");
      }
      break;
    default:
      return rls_fail(ctx, RLS_E_UNSUPPORTED, "admm_init: regulariser not fused (use the per-call path)");
  }
  if (p->proj_kind != RLS_PROJ_NONE && p->proj_kind != RLS_PROJ_REAL && p->proj_kind != RLS_PROJ_POSITIVE)
    return rls_fail(ctx, RLS_E_INVALID, "admm_init: bad proj_kind");
  RLS_HIP(ctx, rls_enter(ctx));
  rls_alloc_scope alloc_scope(ctx);
  const int cap = p->iterations > 0 ? p->iterations : 1;
  if (cap > a->log_cap) {
    a->mem.rollback(a->log_mark);  // (the smaller log)
    a->log_cap = 0;
    a->mem.dev(&a->log, sizeof(float) * ADMM_REC * cap * a->nrhs, false);
    a->mem.pinned(&a->log_h, sizeof(float) * ADMM_REC * cap * a->nrhs, false);
    if (const int e = a->mem.error()) {
      a->mem.rollback(a->log_mark);
      return rls_fail(ctx, e, "admm_init: allocation failed");
    }
    a->log_cap = cap;
  }
  a->P = *p;
  a->enq = 0;
  a->requested = 0;
  a->breg_inner = 0;
  hipLaunchKernelGGL(admm_reset_kernel<float>, dim3((unsigned)a->nrhs), dim3(1), 0, ctx->stream, a->sc, p->iterations,
                     p->rho, p->sigma_abs, p->rel_tol);
  RLS_TRY(launch_status(ctx));
  a->ready = true;
  return 0;
}

int32_t rls_admm_set_bregman(rls_admm* a, int32_t iterations_inner, void* Y, int64_t ldy) {
  if (!a) return RLS_E_INVALID;
  rls_ctx* ctx = a->cg->op->ctx;
  if (!a->ready || a->enq != 0) return rls_fail(ctx, RLS_E_STATE, "admm_set_bregman: call it right after admm_init");
  if (!a->cg->ops.allocated()) return rls_fail(ctx, RLS_E_UNSUPPORTED, "admm_set_bregman: batched plans only (rls_cg_create_batched)");
  if (a->P.reg_kind == RLS_REG_TV) return rls_fail(ctx, RLS_E_UNSUPPORTED, "admm_set_bregman: no TV term in Bregman mode");
  if (iterations_inner < 1 || !Y || ldy < a->cg->op->N) return rls_fail(ctx, RLS_E_INVALID, "admm_set_bregman: bad argument");
  a->breg_inner = iterations_inner;
  a->breg_y = Y;
  a->breg_ldy = ldy;
  return 0;
}

int32_t rls_admm_step(rls_admm* a, int32_t n_outer) {
  if (!a) return RLS_E_INVALID;
  rls_cg* cg = a->cg;
  rls_ctx* ctx = cg->op->ctx;
  if (!a->ready) return rls_fail(ctx, RLS_E_STATE, "admm_step before admm_init");
  if (n_outer < 0) return rls_fail(ctx, RLS_E_INVALID, "admm_step: n_outer < 0");
  RLS_HIP(ctx, rls_enter(ctx));
  const rls_admm_params& P = a->P;
  const int32_t dtype = cg->op->dtype;
  const int64_t n = cg->op->N;
  if (a->nrhs > 1 || cg->ops.allocated()) return admm_step_batched(a, n_outer);
  a->requested = (int)std::min<long long>((long long)a->requested + n_outer, (long long)P.iterations);
  for (int k = 0; k < n_outer && a->enq < P.iterations; ++k, ++a->enq) {
    void* zcur = (a->enq & 1) ? P.z1 : P.z0;
    void* znew = (a->enq & 1) ? P.z0 : P.z1;
    admm_fuse_v F;
    F.beta_y = P.beta_y;
    F.z = zcur;
    F.u = P.u;
    F.beta = P.beta;
    F.xold = P.xold;
    F.rho = P.rho;
    F.skip = &a->sc->done;
    F.poison = &a->sc->done;  // a resident cg! that gives up sets done = 2: the z / u kernels behind it skip
    RLS_TRY(cg_solve_impl(cg, P.x, P.beta, P.rho, P.iterations_cg, P.tol_inner, F));  // :236-244
    const int* cg_it = cg->used_pipeline ? &cg->psc->iteration : &cg->sc->iteration;
    const int z_ready = P.reg_kind == RLS_REG_TV;
    if (z_ready)
      RLS_TRY(rls_tv_single_launch(ctx, dtype, P.tv_ndims, P.tv_shape, P.tv_ntv, P.tv_dims, P.x, P.u, znew,
                                   P.prox_lambda, P.tv_iterations, &a->sc->done));
    RLS_TRY(rls_with_elem(dtype, [&](auto t) {
      using E = typename decltype(t)::type;
      return rls_launch<admm_zu_kernel<E>>(ctx, dim3(1), dim3(UPD_THREADS), 0, (E*)P.x, (const E*)P.xold, (E*)znew, (const E*)zcur,
                                           (E*)P.u, n, P.reg_kind, P.prox_lambda, P.proj_kind, z_ready, a->sc, cg_it, a->log,
                                           col_batch<E>(), (const cg_scalars*)nullptr);
    }));
  }
  return 0;
}

// ---- ADMM on a row-partitioned A (src/ADMM.jl:191-330; one regulariser, identity regTrafo, vary_rho = :none) --------------
// plans[r]: rls_cg_create + rls_admm_create + rls_admm_init on rank r's shard operator, every rank with the same
// parameters (sigma_abs from the length of the WHOLE b, :214).  The x-update's cg! is the distributed part: its operator
// applies are per-shard products followed by ONE all-reduce of c each; it always runs its `iterations_cg` half-step
// pairs -- its own convergence and the plan's `done` are device flags replicated on every rank (identical inputs,
// identical order), so the collective count never depends on the data.  Everything else of the outer iteration is the
// single-GPU plan's kernels, replicated: beta = beta_y + rho (z - u) inside the start kernel, the FGP launch for a TV
// term, admm_zu_kernel (projections, z, u, the norms, `converged`).
int32_t rls_admm_init_rowsharded(rls_comm* comm, rls_admm* const* plans, const void* const* b_parts) {
  RLS_TRY(rowsharded_check<rls_admm>(comm, plans, admm_op, admm_single));
  if (!b_parts) return RLS_E_INVALID;
  const int n = rls_comm_size(comm);
  for (int r = 0; r < n; ++r)
    if (!plans[r]->ready || !b_parts[r]) return rls_fail(plans[r]->cg->op->ctx, RLS_E_STATE, "admm_init_rowsharded before admm_init");
  const int64_t N = plans[0]->cg->op->N;
  const int32_t dtype = plans[0]->cg->op->dtype;
  int round0 = 0;
  RLS_TRY(rls_comm_next_rounds(comm, 1, N, dtype, &round0));
  const std::vector<rls_comm_phase> phases = {
      {[&](int r, int) {  // beta_y = A^H b   (:198), per shard
         rls_operator* op = plans[r]->cg->op;
         RLS_HIP(op->ctx, hipSetDevice(op->ctx->device));
         RLS_TRY(rls_launch_gemv(op->ctx, dtype, RLS_OP_C, op->M, op->N, 1.f, 0.f, op->A, op->lda, b_parts[r], 0.f, 0.f,
                                 plans[r]->P.beta_y, nullptr));
         return rls_comm_publish(comm, r, plans[r]->P.beta_y, N, dtype, round0);
       }, true},
      {[&](int r, int) { return rls_comm_collect(comm, r, plans[r]->P.beta_y, N, dtype, round0); }, false}};
  return rls_comm_run(comm, phases, 1);
}

int32_t rls_admm_step_rowsharded(rls_comm* comm, rls_admm* const* plans, int32_t n_outer) {
  RLS_TRY(rowsharded_check<rls_admm>(comm, plans, admm_op, admm_single));
  if (n_outer < 0) return RLS_E_INVALID;
  const int n = rls_comm_size(comm);
  for (int r = 0; r < n; ++r) {
    if (!plans[r]->ready) return rls_fail(plans[r]->cg->op->ctx, RLS_E_STATE, "admm_step_rowsharded before admm_init");
    if (plans[r]->enq != plans[0]->enq || plans[r]->P.iterations != plans[0]->P.iterations ||
        plans[r]->P.iterations_cg != plans[0]->P.iterations_cg)
      return rls_fail(plans[r]->cg->op->ctx, RLS_E_INVALID, "admm_step_rowsharded: the ranks' plans are out of step");
  }
  const int64_t N = plans[0]->cg->op->N;
  const int32_t dtype = plans[0]->cg->op->dtype;
  const int icg = plans[0]->P.iterations_cg;
  const int todo = std::min<int>(n_outer, plans[0]->P.iterations - plans[0]->enq);
  if (todo <= 0) return 0;
  const int per_outer = icg + 1;  // all-reduce rounds of one outer iteration: the warm-start apply + one per inner step
  int round0 = 0;
  RLS_TRY(rls_comm_next_rounds(comm, todo * per_outer, N, dtype, &round0));
  auto zbufs = [&](rls_admm* a, void** zcur, void** znew) {
    *zcur = (a->enq & 1) ? a->P.z1 : a->P.z0;
    *znew = (a->enq & 1) ? a->P.z0 : a->P.z1;
  };
  std::vector<rls_comm_phase> phases;
  phases.push_back({[&](int r, int k) {  // c_g = A_g^H A_g x   (warm start of cg!, src/ADMM.jl:244)
                      rls_admm* a = plans[r];
                      rls_cg* cg = a->cg;
                      RLS_HIP(cg->op->ctx, hipSetDevice(cg->op->ctx->device));
                      cg->used_pipeline = false;
                      RLS_TRY(op_normal(cg->op, a->P.x, cg->c, &a->sc->done));
                      return rls_comm_publish(comm, r, cg->c, N, dtype, round0 + k * per_outer);
                    }, true});
  for (int j = 0; j <= icg; ++j) {
    phases.push_back({[&, j](int r, int k) {
                        rls_admm* a = plans[r];
                        rls_cg* cg = a->cg;
                        rls_ctx* ctx = cg->op->ctx;
                        RLS_HIP(ctx, rls_enter(ctx));
                        RLS_TRY(rls_comm_collect(comm, r, cg->c, N, dtype, round0 + k * per_outer + j));
                        void *zcur, *znew;
                        zbufs(a, &zcur, &znew);
                        if (j == 0) {  // beta = beta_y + rho (z - u), xold = x, r = beta - (c + rho x), u = r   (:236-243)
                          admm_fuse_v F;
                          F.beta_y = a->P.beta_y;
                          F.z = zcur;
                          F.u = a->P.u;
                          F.beta = a->P.beta;
                          F.xold = a->P.xold;
                          F.rho = a->P.rho;
                          F.skip = &a->sc->done;
                          rls_with_elem(dtype, [&](auto t) { admm_local_start<typename decltype(t)::type>(a, F); });
                        } else {
                          RLS_TRY(rls_cg_local_update(cg, a->P.x));
                        }
                        RLS_TRY(launch_status(ctx));
                        if (j < icg) {  // next inner step's operator apply on the direction u
                          RLS_TRY(op_normal(cg->op, cg->u, cg->c, &cg->sc->done));
                          return rls_comm_publish(comm, r, cg->c, N, dtype, round0 + k * per_outer + j + 1);
                        }
                        // the rest of the outer iteration, replicated (:246-309)
                        if (a->P.reg_kind == RLS_REG_TV)
                          RLS_TRY(rls_tv_single_launch(ctx, dtype, a->P.tv_ndims, a->P.tv_shape, a->P.tv_ntv, a->P.tv_dims, a->P.x,
                                                       a->P.u, znew, a->P.prox_lambda, a->P.tv_iterations, &a->sc->done));
                        rls_with_elem(dtype, [&](auto t) { admm_local_finish<typename decltype(t)::type>(a, zcur, znew); });
                        ++a->enq;
                        a->requested = a->enq;
                        return launch_status(ctx);
                      }, j < icg});
  }
  return rls_comm_run(comm, phases, todo);
}

// batched plans: out_h[nrhs]; log_h (nullable): nrhs blocks of log_records records, column after column
int32_t rls_admm_get_status_batched(rls_admm* a, rls_admm_status* out, float* log_h, int32_t log_records) {
  if (!a || !out) return RLS_E_INVALID;
  rls_ctx* ctx = a->cg->op->ctx;
  if (!a->ready) return rls_fail(ctx, RLS_E_STATE, "admm_get_status before admm_init");
  if (log_records < 0 || (log_records > 0 && !log_h)) return rls_fail(ctx, RLS_E_INVALID, "admm_get_status: bad log");
  RLS_HIP(ctx, rls_enter(ctx));
  const size_t stride = (size_t)ADMM_REC * a->log_cap;
  RLS_HIP(ctx, hipMemcpyAsync(a->log_h, a->log, sizeof(float) * stride * a->nrhs, hipMemcpyDeviceToHost, ctx->stream));
  RLS_HIP(ctx, hipMemcpyAsync(a->sc_h, a->sc, sizeof(admm_scalars) * a->nrhs, hipMemcpyDeviceToHost, ctx->stream));
  RLS_HIP(ctx, rls_stream_wait(ctx->stream));
  for (int b = 0; b < a->nrhs; ++b) {
    const int it = a->sc_h[b].iteration;
    out[b].iteration = it;
    out[b].done = a->sc_h[b].done;
    out[b].fallbacks = 0;
    out[b].delta = out[b].sk = out[b].eps_pri = out[b].rk = out[b].eps_dua = 0.f;
    out[b].cg_iterations = 0;
    if (it > 0 && it <= a->log_cap) {
      const float* rec = a->log_h + stride * b + (size_t)(it - 1) * ADMM_REC;
      out[b].delta = rec[0];
      out[b].sk = rec[1];
      out[b].eps_pri = rec[2];
      out[b].rk = rec[3];
      out[b].eps_dua = rec[4];
      out[b].cg_iterations = (int32_t)rec[5];
    }
    const int ncopy = it < log_records ? it : log_records;
    for (int i = 0; i < ncopy * ADMM_REC; ++i) log_h[(size_t)b * log_records * ADMM_REC + i] = a->log_h[stride * b + i];
  }
  return 0;
}

int32_t rls_admm_get_status(rls_admm* a, rls_admm_status* out, float* log_h, int32_t log_records) {
  if (!a || !out) return RLS_E_INVALID;
  rls_ctx* ctx = a->cg->op->ctx;
  if (!a->ready) return rls_fail(ctx, RLS_E_STATE, "admm_get_status before admm_init");
  if (a->nrhs != 1) return rls_fail(ctx, RLS_E_STATE, "admm_get_status on a batched plan: use rls_admm_get_status_batched");
  if (log_records < 0 || (log_records > 0 && !log_h)) return rls_fail(ctx, RLS_E_INVALID, "admm_get_status: bad log");
  RLS_HIP(ctx, rls_enter(ctx));
  rls_cg* cg = a->cg;
  int nrec = a->enq < a->log_cap ? a->enq : a->log_cap;
  if (nrec > 0) RLS_TRY(rls_fetch_add(ctx, a->log, a->log_h, sizeof(float) * ADMM_REC * nrec));
  if (cg->resident.used) RLS_TRY(cg->resident.fetch_flags(ctx));
  RLS_TRY(fetch_scalars(ctx, a->sc, a->sc_h));  // synchronises the stream
  if (cg->resident.used && cg->resident.lost(ctx)) {
    // A resident cg! gave up: it was a no-op and poisoned `done` (= 2), so everything queued behind it skipped.  The
    // outer iteration it belonged to has changed nothing that its repetition does not rewrite (beta, xold), so clear the
    // poison and run the missing outer iterations again; the inner solves now take the per-iteration pipeline.
    a->fallbacks = cg->resident.fallbacks;
    if (a->sc_h->done == 2) {
      const int it_done = a->sc_h->iteration;
      RLS_HIP(ctx, hipMemsetAsync(&a->sc->done, 0, sizeof(int), ctx->stream));
      a->enq = it_done;
      const int missing = a->requested - it_done;
      a->requested = it_done;
      if (missing > 0) RLS_TRY(rls_admm_step(a, missing));
      nrec = a->enq < a->log_cap ? a->enq : a->log_cap;
      if (nrec > 0) RLS_TRY(rls_fetch_add(ctx, a->log, a->log_h, sizeof(float) * ADMM_REC * nrec));
      RLS_TRY(fetch_scalars(ctx, a->sc, a->sc_h));
    }
  }
  const int it = a->sc_h->iteration;
  a->enq = it;  // a plan that stopped early continues (after a re-init only) from the device's count
  out->iteration = it;
  out->done = a->sc_h->done;
  out->fallbacks = a->fallbacks;
  out->delta = out->sk = out->eps_pri = out->rk = out->eps_dua = 0.f;
  out->cg_iterations = 0;
  if (it > 0 && it <= nrec) {
    const float* rec = a->log_h + (size_t)(it - 1) * ADMM_REC;
    out->delta = rec[0];
    out->sk = rec[1];
    out->eps_pri = rec[2];
    out->rk = rec[3];
    out->eps_dua = rec[4];
    out->cg_iterations = (int32_t)rec[5];
  }
  const int ncopy = it < log_records ? it : log_records;
  for (int i = 0; i < ncopy * ADMM_REC; ++i) log_h[i] = a->log_h[i];
  return 0;
}

int32_t rls_admm_step_status(rls_admm* a, int32_t n_outer, rls_admm_status* out, float* log_h, int32_t log_records) {
  RLS_TRY(rls_admm_step(a, n_outer));
  return rls_admm_get_status(a, out, log_h, log_records);
}

}  // extern "C"
