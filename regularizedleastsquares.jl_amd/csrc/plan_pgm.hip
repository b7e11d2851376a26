// OptISTA / POGM: the resident plan and the batched plan (kernels: normal.hip, pgm.hip).
#include "plans.hpp"

// ---------------------------------------------------------------------------------------------
// OptISTA / POGM (restart = :none) as resident launches (kernel: normal.hip, pgm_resident_kernel)
// ---------------------------------------------------------------------------------------------
// The solver state (x, y, z, zold / xold, res, x0 and the 4-word record) belongs to the caller, as with the per-iteration
// entry points rls_optista_update_async / rls_pogm_update_async; the plan owns what a resident launch needs on top: the
// arrival counters and the N-vector of the flat exchange.
struct rls_pgm {
  plan_buffers mem;
  rls_operator* op = nullptr;
  rls_ctx* actx = nullptr;
  uint64_t actx_id = 0;
  int device = 0;
  resident_slot resident;  // (`used` stays false: the caller asks rls_pgm_lost behind its launches)
  void* raw = nullptr;
};

// the launch's view of the caller's state: `kind` 0 = OptISTA (v0..v2 = x, y, z; o0 = zold), 1 / 2 = POGM (x, y, z; o0 = xold;
// kind 2 also w in D.v3)
static rls_pgm_desc pgm_desc(const rls_pgm* s, int kind, void* v0, void* v1, void* v2, void* o0, void* res, const void* x0,
                             int32_t reg_kind, int32_t proj_kind, float norm_x0, float rel_tol, void* state_d, int32_t first_iteration) {
  rls_pgm_desc D;
  D.A = s->op->A;
  D.lda = s->op->lda;
  D.M = s->op->M;
  D.N = s->op->N;
  D.kind = kind;
  D.v0 = v0;
  D.v1 = v1;
  D.v2 = v2;
  D.o0 = o0;
  D.res = res;
  D.x0 = x0;
  D.slab = s->op->slab;
  D.raw = s->raw;
  D.st = (pgm_state*)state_d;
  D.norm_x0 = norm_x0;
  D.rel_tol = rel_tol;
  D.reg_kind = reg_kind;
  D.proj_kind = proj_kind;
  D.first_it = first_iteration;
  return D;
}
// (not through resident_slot::launch: the caller accounts for its launches itself, rls_pgm_lost)
static int32_t pgm_launch(rls_pgm* s, const rls_pgm_desc& D, const rls_pgm_coefs& C, int32_t n_steps) {
  rls_ctx* ctx = s->op->ctx;
  return s->resident.chain(ctx, [&](void* sync, unsigned spin) {
    return rls_pgm_resident_launch(ctx, s->op->dtype, D, C, sync, n_steps, spin);
  });
}

// ---------------------------------------------------------------------------------------------
// Batched OptISTA / POGM: K right-hand sides sharing A (solve!(solver, B) of src/MultiThreading.jl:30-79), shaped like
// the batched FISTA plan: the K gradient points as an MFMA operand panel, T = A X and the partial rows of A^H T (or one
// product over an explicit AHA) on the matrix cores, then one workgroup per column (pgm.hip, pgmb_update_kernel).
// ---------------------------------------------------------------------------------------------
struct rls_pgm_batched {
  plan_buffers mem;
  rls_operator* op = nullptr;
  rls_ctx* actx = nullptr;
  uint64_t actx_id = 0;
  int device = 0;
  int kind = 0;  // 0 = OptISTA, 1 = POGM
  rls_pgmb D;
  shared_operands ops;  // (the panel: the gradient points)
  pgmb_scalars *sc = nullptr, *sc_h = nullptr;  // [nrhs], pinned mirror
  step_graph graph;
  bool initialised = false;
};

static rls_skinny pgmb_skinny_desc(const rls_pgm_batched* s) { return s->ops.desc(s->op, s->D.nrhs, s->D.ldv); }

extern "C" {

int32_t rls_pgm_create(rls_operator* op, rls_pgm** out) {
  if (!op || !out) return RLS_E_INVALID;
  rls_ctx* ctx = op->ctx;
  *out = nullptr;
  RLS_HIP(ctx, rls_enter(ctx));
  if (!(op->slab && op->A && !op->G && rls_pgm_resident_ok(ctx, op->dtype, op->M, op->N, op->A, op->lda)))
    return RLS_E_UNSUPPORTED;  // (not an error state: the caller keeps its launch-per-iteration sequence)
  rls_alloc_scope alloc_scope(ctx);
  rls_pgm* s = new rls_pgm{plan_memory(ctx)};
  s->op = op;
  s->actx = ctx;
  s->actx_id = ctx->id;
  s->device = ctx->device;
  s->resident.alloc(s->mem, ctx, op);
  s->mem.dev(&s->raw, (size_t)op->N * rls_elem_size(op->dtype), false);
  if (const int e = s->mem.error()) {
    rls_pgm_destroy(s);
    (void)hipGetLastError();
    return rls_fail(ctx, e, "pgm_create: hipMalloc failed");
  }
  *out = s;
  return 0;
}

int32_t rls_pgm_destroy(rls_pgm* s) {
  if (!s) return RLS_E_INVALID;
  hipSetDevice(s->device);
  rls_alloc_scope alloc_scope(alloc_ctx_of(s->actx, s->actx_id));
  s->mem.release();
  delete s;
  return 0;
}

int32_t rls_pgm_step_resident(rls_pgm* s, int32_t kind, int32_t n_steps, int32_t first_iteration, const float* coefs, void* v0,
                              void* v1, void* v2, void* o0, void* res, const void* x0, int32_t reg_kind, int32_t proj_kind,
                              float norm_x0, float rel_tol, void* state_d) {
  if (!s) return RLS_E_INVALID;
  rls_ctx* ctx = s->op->ctx;
  if ((kind != 0 && kind != 1) || n_steps < 0 || n_steps > RLS_PGM_MAX_IT || first_iteration < 0 || !coefs || !v0 || !v1 || !v2 ||
      !o0 || !res || !x0 || !state_d || reg_kind < RLS_REG_NONE || reg_kind > RLS_REG_L2 || proj_kind < RLS_PROJ_NONE ||
      proj_kind > RLS_PROJ_POSITIVE || (kind == 0 && proj_kind != RLS_PROJ_NONE))
    return rls_fail(ctx, RLS_E_INVALID, "pgm_step_resident: bad argument");
  if (!aligned16(v0, v1, v2, o0, res, x0))
    return rls_fail(ctx, RLS_E_INVALID, "pgm_step_resident: vectors must be 16-byte aligned");
  if (s->resident.off || !ctx->tune.resident) return RLS_E_UNSUPPORTED;  // lost a launch earlier: per-iteration launches
  if (n_steps == 0) return 0;
  RLS_HIP(ctx, rls_enter(ctx));
  rls_pgm_coefs C;
  memcpy(C.c, coefs, sizeof(float) * 8 * (size_t)n_steps);
  return pgm_launch(s, pgm_desc(s, kind, v0, v1, v2, o0, res, x0, reg_kind, proj_kind, norm_x0, rel_tol, state_d, first_iteration), C,
                    n_steps);
}

// POGM with restart = :gradient as resident launches: theta, sigma, gamma live in the record (pogm_auto_state) and the kernel
// forms every iteration's coefficients from them (src/POGM.jl:183-232), so a block needs no table -- only rho, lambda, sigma_fac
// and the iteration count of the solve (the last iteration's theta rule, :185).
int32_t rls_pogm_step_resident_restart(rls_pgm* s, int32_t n_steps, int32_t first_iteration, float rho, float lambda, float sigma_fac,
                                       int32_t iterations, void* xbuf, void* ybuf, void* z, void* w, void* xold, void* res,
                                       const void* x0, int32_t reg_kind, int32_t proj_kind, float norm_x0, float rel_tol,
                                       void* state_d) {
  if (!s) return RLS_E_INVALID;
  rls_ctx* ctx = s->op->ctx;
  if (n_steps < 0 || first_iteration < 0 || iterations < 1 || iterations >= (1 << 24) || !xbuf || !ybuf || !z || !w || !xold || !res ||
      !x0 || !state_d || reg_kind < RLS_REG_NONE || reg_kind > RLS_REG_L2 || proj_kind < RLS_PROJ_NONE || proj_kind > RLS_PROJ_POSITIVE)
    return rls_fail(ctx, RLS_E_INVALID, "pogm_step_resident_restart: bad argument");
  if (!aligned16(xbuf, ybuf, z, w, xold, res, x0))
    return rls_fail(ctx, RLS_E_INVALID, "pogm_step_resident_restart: vectors must be 16-byte aligned");
  if (s->resident.off || !ctx->tune.resident) return RLS_E_UNSUPPORTED;
  if (n_steps == 0) return 0;
  RLS_HIP(ctx, rls_enter(ctx));
  rls_pgm_coefs C;
  C.c[0][0] = rho;
  C.c[0][1] = lambda;
  C.c[0][2] = sigma_fac;
  C.c[0][3] = (float)iterations;  // (exact: < 2^24)
  rls_pgm_desc D = pgm_desc(s, 2, xbuf, ybuf, z, xold, res, x0, reg_kind, proj_kind, norm_x0, rel_tol, state_d, first_iteration);
  D.v3 = w;
  return pgm_launch(s, D, C, n_steps);
}

// after the launches of a sequence: how many of them gave up (bounded wait; they changed nothing).  Synchronises.
int32_t rls_pgm_lost(rls_pgm* s, int32_t* lost, int32_t* fallbacks_total) {
  if (!s || !lost) return RLS_E_INVALID;
  rls_ctx* ctx = s->op->ctx;
  RLS_HIP(ctx, rls_enter(ctx));
  RLS_TRY(s->resident.fetch_flags(ctx));
  RLS_TRY(rls_fetch_wait(ctx));
  *lost = (int32_t)s->resident.lost(ctx);
  if (fallbacks_total) *fallbacks_total = s->resident.fallbacks;
  return 0;
}

int32_t rls_pgm_create_batched(rls_operator* op, int32_t kind, int32_t nrhs, void* v0, void* v1, void* z, void* w, void* old,
                               void* res, void* x0, int64_t ldv, rls_pgm_batched** out) {
  if (!op) return RLS_E_INVALID;
  rls_ctx* ctx = op->ctx;
  if ((kind != 0 && kind != 1) || !v0 || !v1 || !z || !old || !res || !x0 || !out || nrhs < 1 || ldv < op->N)
    return rls_fail(ctx, RLS_E_INVALID, "pgm_create_batched: bad argument");
  *out = nullptr;
  if (!ctx->tune.batched_mfma || !shared_operands::supported(op))
    return rls_fail(ctx, RLS_E_UNSUPPORTED, "batched OptISTA / POGM needs A (and AHA, when explicit) with 16-aligned M, N (matrix-core path)");
  RLS_HIP(ctx, rls_enter(ctx));
  rls_alloc_scope alloc_scope(ctx);
  rls_pgm_batched* s = new rls_pgm_batched{plan_memory(ctx)};
  s->op = op;
  s->actx = ctx;
  s->actx_id = ctx->id;
  s->device = ctx->device;
  s->kind = kind;
  s->ops.alloc(s->mem, op, nrhs);
  s->mem.dev(&s->sc, sizeof(pgmb_scalars) * nrhs, true);
  s->mem.pinned(&s->sc_h, sizeof(pgmb_scalars) * nrhs, false);
  if (const int e = s->mem.error()) {
    rls_pgm_destroy_batched(s);
    (void)hipGetLastError();
    return rls_fail(ctx, e, "pgm_create_batched: allocation failed");
  }
  rls_pgmb& D = s->D;
  D = rls_pgmb();
  D.kind = kind == 0 ? RLS_PGMB_OPTISTA : RLS_PGMB_POGM;
  D.N = op->N;
  D.ldv = ldv;
  D.nrhs = nrhs;
  D.v0 = v0;
  D.v1 = v1;
  D.v2 = z;
  D.v3 = w;
  D.o0 = old;
  D.res = res;
  D.x0 = x0;
  D.ops = s->ops.erased(nrhs);
  D.sc = s->sc;
  D.table = nullptr;
  D.reg_kind = RLS_REG_L1;
  D.proj_kind = RLS_PROJ_NONE;
  D.lambda = 0.f;
  *out = s;
  return 0;
}

int32_t rls_pgm_destroy_batched(rls_pgm_batched* s) {
  if (!s) return RLS_E_INVALID;
  hipSetDevice(s->device);
  rls_alloc_scope alloc_scope(alloc_ctx_of(s->actx, s->actx_id));
  s->graph.drop();
  s->mem.release();
  delete s;
  return 0;
}

int32_t rls_pgm_set_reg_batched(rls_pgm_batched* s, int32_t reg_kind, float lambda, int32_t proj_kind) {
  if (!s) return RLS_E_INVALID;
  rls_ctx* ctx = s->op->ctx;
  if (reg_kind < RLS_REG_NONE || reg_kind > RLS_REG_L2 || proj_kind < RLS_PROJ_NONE || proj_kind > RLS_PROJ_POSITIVE ||
      (s->kind == 0 && proj_kind != RLS_PROJ_NONE))
    return rls_fail(ctx, RLS_E_INVALID, "pgm_set_reg_batched: regulariser / projection not covered by the batched update");
  if (reg_kind != s->D.reg_kind || lambda != s->D.lambda || proj_kind != s->D.proj_kind) s->graph.drop();  // (kernel arguments)
  s->D.reg_kind = reg_kind;
  s->D.lambda = lambda;
  s->D.proj_kind = proj_kind;
  return 0;
}

int32_t rls_pgm_init_batched(rls_pgm_batched* s, const void* B, int64_t ldb, float rho, float theta, float sigma_fac, float gamma0,
                             float rel_tol, int32_t iterations, int32_t restart_gradient, const void* table_d, int32_t table_rows) {
  if (!s) return RLS_E_INVALID;
  rls_operator* op = s->op;
  rls_ctx* ctx = op->ctx;
  const bool restart = restart_gradient != 0;
  if (!B || ldb < op->M || iterations < 0 || (restart && (s->kind != 1 || !s->D.v3)) ||
      (!restart && iterations > 0 && (!table_d || table_rows < iterations)))
    return rls_fail(ctx, RLS_E_INVALID, "pgm_init_batched: bad argument");
  RLS_HIP(ctx, rls_enter(ctx));
  rls_pgmb D = s->D;
  D.kind = s->kind == 0 ? RLS_PGMB_OPTISTA : restart ? RLS_PGMB_POGM_RESTART : RLS_PGMB_POGM;
  D.table = restart ? nullptr : (const float*)table_d;
  D.max_iter = iterations;
  D.rho = rho;
  D.rel_tol = rel_tol;
  D.sigma_fac = sigma_fac;
  D.theta = theta;
  D.gamma0 = gamma0;
  if (!restart && !D.table) D.table = (const float*)s->sc;  // iterations == 0: never read
  // every one of these is an argument of the captured kernels
  if (D.kind != s->D.kind || D.table != s->D.table || D.max_iter != s->D.max_iter || D.rho != s->D.rho || D.rel_tol != s->D.rel_tol ||
      D.sigma_fac != s->D.sigma_fac)
    s->graph.drop();
  s->D = D;
  RLS_TRY(rls_skinny_atb(ctx, op->dtype, pgmb_skinny_desc(s), B, ldb));  // partial rows of A^H B
  RLS_TRY(rls_pgmb_launch_init(ctx, op->dtype, s->D));
  s->initialised = true;
  return 0;
}

int32_t rls_pgm_step_batched(rls_pgm_batched* s, int32_t n_steps) {
  if (!s) return RLS_E_INVALID;
  rls_ctx* ctx = s->op->ctx;
  if (!s->initialised) return rls_fail(ctx, RLS_E_STATE, "pgm_step_batched before pgm_init_batched");
  if (n_steps < 0) return rls_fail(ctx, RLS_E_INVALID, "pgm_step_batched: n_steps < 0");
  RLS_HIP(ctx, rls_enter(ctx));
  const int32_t dtype = s->op->dtype;
  return run_steps(ctx, &s->graph, n_steps, [s, ctx, dtype]() {
    RLS_TRY(rls_skinny_launch(ctx, dtype, pgmb_skinny_desc(s), 1 | 2));
    return rls_pgmb_launch_update(ctx, dtype, s->D);
  });
}

int32_t rls_pgm_get_status_batched(rls_pgm_batched* s, rls_pgm_status* out) {
  if (!s || !out) return RLS_E_INVALID;
  rls_ctx* ctx = s->op->ctx;
  if (!s->initialised) return rls_fail(ctx, RLS_E_STATE, "pgm_get_status_batched before pgm_init_batched");
  RLS_HIP(ctx, rls_enter(ctx));
  static_assert(sizeof(pgmb_scalars) % 4 == 0, "status structs are copied dword by dword");
  RLS_TRY(rls_fetch_add(ctx, s->sc, s->sc_h, sizeof(pgmb_scalars) * (size_t)s->D.nrhs));
  RLS_TRY(rls_fetch_wait(ctx));
  for (int b = 0; b < s->D.nrhs; ++b) {
    const pgmb_scalars& h = s->sc_h[b];
    out[b].iteration = h.iteration;
    out[b].done = h.done;
    out[b].res_norm = h.res_norm;
    out[b].rel_res_norm = h.rel_res_norm;
    out[b].norm_x0 = (float)h.norm_x0;
    out[b].theta = h.theta;
    out[b].theta_old = h.theta_old;
    out[b].sigma = h.sigma;
    out[b].gamma = h.gamma;
  }
  return 0;
}

}  // extern "C"
