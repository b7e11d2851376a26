// DirectSolver and PseudoInverse: the plans only (kernels: direct.hip, pinv.hip).
#include "plans.hpp"

// ---------------------------------------------------------------------------------------------
// DirectSolver (src/Direct.jl:17-67): x = (A^H A + lambda I) \ A^H b; kernels in direct.hip
// ---------------------------------------------------------------------------------------------
// The plan owns the Cholesky factor of G + lambda I and reuses it for every solve until lambda (or the operator's Gram matrix)
// changes; the reference factors anew on every iterate.  G is the operator's explicit Gram matrix where it carries one,
// otherwise the plan forms it once (rls_gram) and keeps it.
struct rls_direct {
  plan_buffers mem;
  rls_operator* op = nullptr;
  rls_ctx* actx = nullptr;
  uint64_t actx_id = 0;
  int device = 0;
  void* L = nullptr;        // rls_direct_factor_elems(N) elements: the padded square, then the factored diagonal tiles
  int* info = nullptr;      // device word: 0, or the 1-based column of the first bad pivot
  int* info_h = nullptr;    // its pinned mirror (rls_direct_get_status)
  void* Gown = nullptr;     // A^H A formed by the plan (operators without an explicit Gram matrix)
  void* Y = nullptr;        // workspace of the solves: rls_direct_padded(N) x ycols elements; the plan's youngest block
  int64_t ycols = 0;
  plan_buffers::mark_t ymark{0, 0};
  float lambda = 0.f;       // of the factor the plan holds
  const void* Gfact = nullptr;
  bool factored = false;    // a factorisation of (lambda, Gfact) has been enqueued ...
  bool known_good = false;  // ... and a status read behind it found info == 0: only then is it reused (rls_direct_factor)
  int32_t factorizations = 0;
};

// ---------------------------------------------------------------------------------------------
// PseudoInverse (src/Direct.jl:70-162): x = V diag(1 / (sigma^2 + lambda)) W^H b on A = W V^H; kernels in pinv.hip
// ---------------------------------------------------------------------------------------------
// The plan owns W, V and the singular values of one operator's A; lambda belongs to a solve.  The reference calls LAPACK's
// svd in the constructor; here the sweeps run on the first rls_pinv_factor.
struct rls_pinv {
  plan_buffers mem;
  rls_operator* op = nullptr;
  rls_ctx* actx = nullptr;
  uint64_t actx_id = 0;
  int device = 0;
  void* W = nullptr;        // rls_pinv_padded(M) x N
  void* V = nullptr;        // rls_pinv_padded(N) x N
  void* t = nullptr;        // N elements: W^H b, scaled, of the column being solved
  float* stats = nullptr;   // sigma_j^2 [N], then |A|_F^2
  float* stats_h = nullptr; // pinned mirror (rls_pinv_singular_values)
  int* rotated = nullptr;   // the sweep word: a workgroup that rotated stores 1
  int* rotated_h = nullptr; // its pinned mirror
  const void* Afact = nullptr;
  bool factored = false;
  float lambda = 0.f;
  int32_t factorizations = 0, sweeps = 0, info = 0;
  // phase 1 (blocked sweeps): the scratch is asked for by the first factorisation that runs it -- always the arena's youngest block
  void* scratch = nullptr;
  size_t scratch_bytes = 0;
  plan_buffers::mark_t scratch_mark{0, 0};
  int32_t block = 0, block_sweeps = 0, block_rounds = 0;
};

// the block width phase 1 of this factorisation runs with (0: none): rls_tuning::pinv_block, read here
static int pinv_block_width(const rls_ctx* ctx, int64_t N) {
  const int v = ctx->tune.pinv_block;
  int b = 0;
  if (v == 16 || v == 32) b = v;
  else if (v == -1 && RLS_PINV_BLOCK_AUTO_N > 0 && N >= 256 && N >= RLS_PINV_BLOCK_AUTO_N) b = RLS_PINV_BLOCK;
  return b > 0 && N > b ? b : 0;  // one block: nothing to pair
}

static int32_t pinv_block_scratch(rls_pinv* s, rls_ctx* ctx, size_t bytes) {
  if (bytes <= s->scratch_bytes) return 0;
  rls_alloc_scope alloc_scope(ctx);
  if (s->scratch) s->mem.rollback(s->scratch_mark);
  s->scratch_bytes = 0;
  s->scratch_mark = s->mem.mark();
  s->mem.dev(&s->scratch, bytes, false);
  if (const int e = s->mem.error()) {
    s->mem.rollback(s->scratch_mark);
    (void)hipGetLastError();
    return rls_fail(ctx, e, "pinv_factor: hipMalloc failed (scratch of the blocked sweeps)");
  }
  s->scratch_bytes = bytes;
  return 0;
}

extern "C" {

int32_t rls_direct_create(rls_operator* op, rls_direct** out) {
  if (!op || !out) return RLS_E_INVALID;
  rls_ctx* ctx = op->ctx;
  *out = nullptr;
  if (!rls_dtype_ok(op->dtype))
    return rls_fail(ctx, RLS_E_UNSUPPORTED, "direct_create: the Cholesky kernels are Float32 / ComplexF32 (no Float64 / ComplexF64 path)");
  if (!op->A && !op->G) return rls_fail(ctx, RLS_E_STATE, "direct_create: operator has neither A nor a Gram matrix");
  RLS_HIP(ctx, rls_enter(ctx));
  const size_t es = rls_elem_size(op->dtype);
  rls_direct* s;
  {
    rls_alloc_scope alloc_scope(ctx);
    s = new rls_direct{plan_memory(ctx)};
    s->op = op;
    s->actx = ctx;
    s->actx_id = ctx->id;
    s->device = ctx->device;
    s->mem.dev(&s->L, rls_direct_factor_elems(op->N) * es, false);
    s->mem.dev(&s->info, sizeof(int), true);
    s->mem.pinned(&s->info_h, sizeof(int), true);
    if (!op->G) s->mem.dev(&s->Gown, (size_t)op->N * (size_t)op->N * es, false);
    s->ymark = s->mem.mark();
  }
  if (const int e = s->mem.error()) {
    rls_direct_destroy(s);
    (void)hipGetLastError();
    return rls_fail(ctx, e, "direct_create: hipMalloc failed");
  }
  if (s->Gown) {
    const int32_t st = rls_gram(ctx, op->dtype, op->M, op->N, op->A, op->lda, s->Gown, op->N);
    if (st != 0) {
      rls_direct_destroy(s);
      return st;
    }
  }
  *out = s;
  return 0;
}

int32_t rls_direct_destroy(rls_direct* s) {
  if (!s) return RLS_E_INVALID;
  hipSetDevice(s->device);
  rls_alloc_scope alloc_scope(alloc_ctx_of(s->actx, s->actx_id));
  s->mem.release();
  delete s;
  return 0;
}

int32_t rls_direct_factor(rls_direct* s, float lambda) {
  if (!s) return RLS_E_INVALID;
  rls_operator* op = s->op;
  rls_ctx* ctx = op->ctx;
  const void* G = op->G ? op->G : s->Gown;
  const int64_t ldg = op->G ? op->ldg : op->N;
  if (!G) return rls_fail(ctx, RLS_E_STATE, "direct_factor: the operator's Gram matrix was taken away and the plan formed none");
  // Reuse needs a factor that is KNOWN to be good: a failed one leaves only the device word behind, which the host sees in
  // rls_direct_get_status alone.  A caller that never reads the status factors on every call (and its solves stay no-ops
  // after a failure, as documented); one that reads it after a solve -- the Python and Julia bindings do -- factors once.
  if (s->factored && s->known_good && lambda == s->lambda && G == s->Gfact) return 0;
  RLS_HIP(ctx, rls_enter(ctx));
  RLS_TRY(rls_direct_launch_factor(ctx, op->dtype, op->N, G, ldg, lambda, s->L, s->info));
  s->lambda = lambda;
  s->Gfact = G;
  s->factored = true;
  s->known_good = false;
  s->factorizations += 1;
  return 0;
}

int32_t rls_direct_solve(rls_direct* s, int64_t K, const void* B, int64_t ldb, void* X, int64_t ldx, int32_t proj_kind) {
  if (!s || !B || !X) return RLS_E_INVALID;
  rls_operator* op = s->op;
  rls_ctx* ctx = op->ctx;
  const int64_t rows = op->A ? op->M : op->N;  // a Gram-only operator takes B = A^H b (as CGNR does, src/CGNR.jl:134)
  if (K < 1 || K > RLS_DIRECT_MAX_RHS || ldb < rows || ldx < op->N || proj_kind < RLS_PROJ_NONE || proj_kind > RLS_PROJ_POSITIVE)
    return rls_fail(ctx, RLS_E_INVALID, "direct_solve: bad argument");
  if (!s->factored) return rls_fail(ctx, RLS_E_STATE, "direct_solve: rls_direct_factor has not run");
  const size_t es = rls_elem_size(op->dtype);
  if (!op->A && !(B == X && ldb == ldx)) {  // the copy X = B runs all columns at once: the two must be the same block or apart
    const char *b0 = (const char*)B, *x0 = (const char*)X;
    const char* b1 = b0 + ((size_t)(K - 1) * (size_t)ldb + (size_t)op->N) * es;
    const char* x1 = x0 + ((size_t)(K - 1) * (size_t)ldx + (size_t)op->N) * es;
    if (b0 < x1 && x0 < b1) return rls_fail(ctx, RLS_E_INVALID, "direct_solve: B and X overlap (pass B == X with ldb == ldx, or disjoint blocks)");
  }
  RLS_HIP(ctx, rls_enter(ctx));
  if (K > s->ycols) {  // the workspace grows with the widest solve seen (stream-ordered: earlier solves still own the old block)
    rls_alloc_scope alloc_scope(ctx);
    s->mem.rollback(s->ymark);
    s->ycols = 0;
    s->mem.dev(&s->Y, (size_t)rls_direct_padded(op->N) * (size_t)K * es, false);
    if (const int e = s->mem.error()) {
      s->mem.rollback(s->ymark);
      (void)hipGetLastError();
      return rls_fail(ctx, e, "direct_solve: hipMalloc failed");
    }
    s->ycols = K;
  }
  // X = A^H B, column by column (each a no-op once the pivot word is set); a Gram-only operator's B is A^H B already: one guarded copy
  for (int64_t k = 0; op->A && k < K; ++k) {
    const char* b = (const char*)B + (size_t)k * (size_t)ldb * es;
    char* x = (char*)X + (size_t)k * (size_t)ldx * es;
    RLS_TRY(rls_launch_gemv(ctx, op->dtype, RLS_OP_C, op->M, op->N, 1.f, 0.f, op->A, op->lda, b, 0.f, 0.f, x, s->info));
  }
  if (!op->A && !(B == X && ldb == ldx)) RLS_TRY(rls_direct_launch_copy(ctx, op->dtype, op->N, (int)K, B, ldb, X, ldx, s->info));
  return rls_direct_launch_solve(ctx, op->dtype, op->N, s->L, (int)K, X, ldx, s->Y, proj_kind, s->info);
}

int32_t rls_direct_get_status(rls_direct* s, rls_direct_status* out) {
  if (!s || !out) return RLS_E_INVALID;
  rls_ctx* ctx = s->op->ctx;
  RLS_HIP(ctx, rls_enter(ctx));
  RLS_HIP(ctx, hipMemcpyAsync(s->info_h, s->info, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  RLS_HIP(ctx, rls_stream_wait(ctx->stream));
  ctx->syncs += 1;
  out->lambda = s->lambda;
  out->factorizations = s->factorizations;
  out->info = *s->info_h;
  s->known_good = s->factored && out->info == 0;  // (the stream has been waited for: the word belongs to the last factorisation)
  return 0;
}

int32_t rls_direct_get_factor(rls_direct* s, void** W, int64_t* ld, void** Ldiag) {
  if (!s || !W || !ld || !Ldiag) return RLS_E_INVALID;
  const int64_t np = rls_direct_padded(s->op->N);
  *W = s->L;
  *ld = np;
  *Ldiag = (char*)s->L + (size_t)np * (size_t)np * rls_elem_size(s->op->dtype);
  return 0;
}

int32_t rls_pinv_create(rls_operator* op, rls_pinv** out) {
  if (!op || !out) return RLS_E_INVALID;
  rls_ctx* ctx = op->ctx;
  *out = nullptr;
  if (!rls_dtype_ok(op->dtype))
    return rls_fail(ctx, RLS_E_UNSUPPORTED, "pinv_create: the Jacobi kernels are Float32 / ComplexF32 (no Float64 / ComplexF64 path)");
  if (!op->A) return rls_fail(ctx, RLS_E_INVALID, "pinv_create: the operator has no explicit A (a Gram matrix alone has no SVD of A)");
  if (op->N > 0x7ffffffe) return rls_fail(ctx, RLS_E_INVALID, "pinv_create: too many columns");
  RLS_HIP(ctx, rls_enter(ctx));
  const size_t es = rls_elem_size(op->dtype);
  const size_t N = (size_t)op->N;
  rls_pinv* s;
  {
    rls_alloc_scope alloc_scope(ctx);
    s = new rls_pinv{plan_memory(ctx)};
    s->op = op;
    s->actx = ctx;
    s->actx_id = ctx->id;
    s->device = ctx->device;
    s->mem.dev(&s->W, (size_t)rls_pinv_padded(op->dtype, op->M) * N * es, false);
    s->mem.dev(&s->V, (size_t)rls_pinv_padded(op->dtype, op->N) * N * es, false);
    s->mem.dev(&s->t, N * es, false);
    s->mem.dev(&s->stats, (N + 1) * sizeof(float), true);
    s->mem.pinned(&s->stats_h, (N + 1) * sizeof(float), true);
    s->mem.dev(&s->rotated, sizeof(int), true);
    s->mem.pinned(&s->rotated_h, sizeof(int), true);
  }
  if (const int e = s->mem.error()) {
    rls_pinv_destroy(s);
    (void)hipGetLastError();
    return rls_fail(ctx, e, "pinv_create: hipMalloc failed");
  }
  *out = s;
  return 0;
}

int32_t rls_pinv_destroy(rls_pinv* s) {
  if (!s) return RLS_E_INVALID;
  hipSetDevice(s->device);
  rls_alloc_scope alloc_scope(alloc_ctx_of(s->actx, s->actx_id));
  s->mem.release();
  delete s;
  return 0;
}

int32_t rls_pinv_factor(rls_pinv* s) {
  if (!s) return RLS_E_INVALID;
  rls_operator* op = s->op;
  rls_ctx* ctx = op->ctx;
  if (!op->A) return rls_fail(ctx, RLS_E_STATE, "pinv_factor: the operator's A was taken away");
  if (s->factored && s->info == 0 && s->Afact == op->A) return 0;
  RLS_HIP(ctx, rls_enter(ctx));
  s->factored = false;
  RLS_TRY(rls_pinv_launch_load(ctx, op->dtype, op->M, op->N, op->A, op->lda, s->W, s->V, s->stats));
  s->factorizations += 1;
  s->sweeps = 0;
  s->info = 1;  // until a sweep finds nothing to rotate
  // phase 1: blocked sweeps until one rotates nothing, or the cap (no error: phase 2 decides convergence)
  s->block = pinv_block_width(ctx, op->N);
  s->block_sweeps = s->block_rounds = 0;
  if (s->block) {
    RLS_TRY(pinv_block_scratch(s, ctx, rls_pinv_block_scratch_bytes(op->dtype, op->M, op->N, s->block)));
    const int cap = ctx->tune.pinv_block_cap > 0 ? ctx->tune.pinv_block_cap : RLS_PINV_BLOCK_CAP;
    float tol = RLS_PINV_BLOCK_TOL;
    if (ctx->tune.pinv_block_tol > 0) tol = powf(10.f, -(float)ctx->tune.pinv_block_tol);
    while (s->block_sweeps < cap) {
      int rounds = 0;
      RLS_HIP(ctx, hipMemsetAsync(s->rotated, 0, sizeof(int), ctx->stream));
      RLS_TRY(rls_pinv_launch_block_sweep(ctx, op->dtype, op->M, op->N, s->block, tol, s->W, s->V, s->stats, s->scratch, s->rotated, &rounds));
      RLS_HIP(ctx, hipMemcpyAsync(s->rotated_h, s->rotated, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
      RLS_HIP(ctx, rls_stream_wait(ctx->stream));
      ctx->syncs += 1;
      s->block_sweeps += 1;
      s->block_rounds += rounds;
      if (*s->rotated_h == 0) break;
    }
  }
  while (s->sweeps < RLS_PINV_MAX_SWEEPS) {
    RLS_HIP(ctx, hipMemsetAsync(s->rotated, 0, sizeof(int), ctx->stream));
    RLS_TRY(rls_pinv_launch_sweep(ctx, op->dtype, op->M, op->N, s->W, s->V, s->stats, s->rotated));
    RLS_HIP(ctx, hipMemcpyAsync(s->rotated_h, s->rotated, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    RLS_HIP(ctx, rls_stream_wait(ctx->stream));
    ctx->syncs += 1;
    s->sweeps += 1;
    if (*s->rotated_h == 0) {
      s->info = 0;
      break;
    }
  }
  RLS_TRY(rls_pinv_launch_finish(ctx, op->dtype, op->M, op->N, s->W, s->stats));
  s->Afact = op->A;
  s->factored = true;
  return 0;
}

int32_t rls_pinv_solve(rls_pinv* s, float lambda, int64_t K, const void* B, int64_t ldb, void* X, int64_t ldx, int32_t proj_kind) {
  if (!s || !B || !X) return RLS_E_INVALID;
  rls_operator* op = s->op;
  rls_ctx* ctx = op->ctx;
  if (K < 1 || ldb < op->M || ldx < op->N || proj_kind < RLS_PROJ_NONE || proj_kind > RLS_PROJ_POSITIVE || !(lambda >= 0.f))
    return rls_fail(ctx, RLS_E_INVALID, "pinv_solve: bad argument");
  if (!s->factored) return rls_fail(ctx, RLS_E_STATE, "pinv_solve: rls_pinv_factor has not run");
  s->lambda = lambda;
  if (s->info != 0) return 0;  // the sweep cap was hit: W's columns are not orthogonal, nothing is written (rls_pinv_get_status)
  RLS_HIP(ctx, rls_enter(ctx));
  const size_t es = rls_elem_size(op->dtype);
  for (int64_t k = 0; k < K; ++k) {
    const char* b = (const char*)B + (size_t)k * (size_t)ldb * es;
    char* x = (char*)X + (size_t)k * (size_t)ldx * es;
    RLS_TRY(rls_pinv_launch_solve(ctx, op->dtype, op->M, op->N, s->W, s->V, s->stats, lambda, b, s->t, x, proj_kind));
  }
  return 0;
}

int32_t rls_pinv_singular_values(rls_pinv* s, float* host_out) {
  if (!s || !host_out) return RLS_E_INVALID;
  rls_ctx* ctx = s->op->ctx;
  if (!s->factored) return rls_fail(ctx, RLS_E_STATE, "pinv_singular_values: rls_pinv_factor has not run");
  RLS_HIP(ctx, rls_enter(ctx));
  const size_t N = (size_t)s->op->N;
  RLS_HIP(ctx, hipMemcpyAsync(s->stats_h, s->stats, (N + 1) * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  RLS_HIP(ctx, rls_stream_wait(ctx->stream));
  ctx->syncs += 1;
  for (size_t j = 0; j < N; ++j) host_out[j] = sqrtf(s->stats_h[j]);
  std::sort(host_out, host_out + N, [](float a, float b) { return a > b; });
  return 0;
}

int32_t rls_pinv_get_status(rls_pinv* s, rls_pinv_status* out) {
  if (!s || !out) return RLS_E_INVALID;
  out->lambda = s->lambda;
  out->factorizations = s->factorizations;
  out->sweeps = s->sweeps;
  out->info = s->info;
  return 0;
}

int32_t rls_pinv_get_block_status(rls_pinv* s, rls_pinv_block_status* out) {
  if (!s || !out) return RLS_E_INVALID;
  out->block = s->block;
  out->block_sweeps = s->block_sweeps;
  out->block_rounds = s->block_rounds;
  out->reserved = 0;
  return 0;
}

int32_t rls_pinv_get_factor(rls_pinv* s, void** W, int64_t* ldw, void** V, int64_t* ldv) {
  if (!s || !W || !ldw || !V || !ldv) return RLS_E_INVALID;
  *W = s->W;
  *ldw = rls_pinv_padded(s->op->dtype, s->op->M);
  *V = s->V;
  *ldv = rls_pinv_padded(s->op->dtype, s->op->N);
  return 0;
}

}  // extern "C"
