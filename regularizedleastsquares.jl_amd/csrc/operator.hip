// Operator handle (rls_operator_*), the setup product G = A^H A (rls_gram), and what exists once per process for every
// plan: the chain of resident launches across streams, and the server-mode helpers CGNR and FISTA share.
#include "plans.hpp"

// A resident kernel needs every one of its workgroups on a CU at the same time.  Other kernels only delay that, but
// two resident kernels running side by side (two contexts = two streams of this process) could each hold CUs the
// other is waiting for.  So resident launches on one device form ONE chain across all streams of the process.  A launch
// on the stream that issued the previous one is ordered by the stream itself (no event traffic at all: the common
// single-context case); only when the stream CHANGES is an event recorded on the previous stream -- now, i.e. behind
// everything it has queued since: conservative -- and waited for by the new one.  (Another PROCESS on the same device
// is not covered: its symptom is the bounded-wait timeout reported by rls_cgnr_get_status.)
hipEvent_t g_resident_ev[64];
resident_chain_state g_resident_chain;  // guarded by rls_capture_mutex(); cleared by rls_resident_forget (context teardown)
void rls_resident_forget(int device, hipStream_t stream) {
  resident_chain_forget(rls_capture_mutex(), g_resident_chain, device, (void*)stream);
}

// ---------------------------------------------------------------------------------------------
// Gram matrix  G = A^H A  (setup GEMM, src/CGNR.jl:49).  LDS-tiled, f32 FMA; not on the
// per-iteration path.  64 x 64 output tile per workgroup, K streamed in 16-row panels.
// ---------------------------------------------------------------------------------------------
template <typename E>
__global__ __launch_bounds__(256) void gram_kernel(const E* __restrict__ A, int64_t lda, int64_t M, int64_t N,
                                                   E* __restrict__ G, int64_t ldg) {
  constexpr int T = 64, KP = 16;
  __shared__ E sa[KP][T + 1];
  __shared__ E sb[KP][T + 1];
  const int64_t i0 = (int64_t)blockIdx.x * T, j0 = (int64_t)blockIdx.y * T;
  const int tx = threadIdx.x % 16, ty = threadIdx.x / 16;  // 16 x 16 threads, 4 x 4 outputs each
  E acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = elem<E>::zero();
  for (int64_t k0 = 0; k0 < M; k0 += KP) {
    for (int idx = threadIdx.x; idx < KP * T; idx += 256) {
      const int kk = idx % KP, cc = idx / KP;
      const int64_t k = k0 + kk;
      sa[kk][cc] = (k < M && i0 + cc < N) ? A[(i0 + cc) * lda + k] : elem<E>::zero();
      sb[kk][cc] = (k < M && j0 + cc < N) ? A[(j0 + cc) * lda + k] : elem<E>::zero();
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < KP; ++kk) {
      E av[4], bv[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) av[a] = sa[kk][ty * 4 + a];
#pragma unroll
      for (int b = 0; b < 4; ++b) bv[b] = sb[kk][tx * 4 + b];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = elem<E>::fmac(av[a], bv[b], acc[a][b]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int64_t i = i0 + ty * 4 + a, j = j0 + tx * 4 + b;
      if (i < N && j < N) G[j * ldg + i] = acc[a][b];
    }
}

// G = A^H A is Hermitian with a real diagonal (Julia's A'*A goes through herk).  The generic kernels compute
// both triangles independently, so the two images of an entry can differ in the last bit: copy the upper triangle
// over the lower one as its conjugate and clear the imaginary part of the diagonal (the 64 x 64 tile kernel is
// Hermitian by construction and does not need this).
template <typename E>
__global__ void hermitianize_kernel(E* __restrict__ G, int64_t ld, int64_t N) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // column
  const int64_t i = (int64_t)blockIdx.y * blockDim.y + threadIdx.y;  // row
  if (i >= N || j >= N || i < j) return;
  if (i == j) {
    G[i + j * ld] = elem<E>::make(elem<E>::re(G[i + j * ld]), 0.f);
  } else {  // i > j: lower triangle <- conj(upper)
    const E u = G[j + i * ld];
    G[i + j * ld] = elem<E>::make(elem<E>::re(u), -elem<E>::im(u));
  }
}

static int32_t gram_hermitianize(rls_ctx* ctx, int32_t dtype, int64_t N, void* G, int64_t ld) {
  const dim3 block(32, 8), grid((unsigned)((N + 31) / 32), (unsigned)((N + 7) / 8));
  return rls_with_elem(dtype, [&](auto t) {
    using E = typename decltype(t)::type;
    return rls_launch<hermitianize_kernel<E>>(ctx, grid, block, 0, (E*)G, ld, N);
  });
}

// ---- resident kernels in server mode (plans.hpp): the helpers that need no plan type ----
bool server_usable(const rls_ctx* ctx, const srv_state* v) {
  return ctx->tune.resident_server && ctx->tune.status_mailbox && v->ctl && !v->off && (ctx->server == nullptr || ctx->server == v);
}

// the life of a listening kernel is over (it was told to leave, left idle, or gave up): bookkeeping, and the verdict on lives
// too short to pay for their launch
void server_life_over(rls_ctx* ctx, srv_state* v) {
  const bool gave_up = v->ctl[17] == 2;
  if (v->alive) {
    if (v->served < 3) {
      if (++v->short_lives >= 2) v->off = true;
    } else {
      v->short_lives = 0;
    }
  }
  v->alive = false;
  v->fresh = false;
  if (gave_up && v->resident_used) *v->resident_used = true;  // a wait ran out in that life: the next status call reads the sync block's flags
  if (ctx->server == v) ctx->server = nullptr;
}

void rls_server_stop(rls_ctx* ctx) {
  srv_state* v = static_cast<srv_state*>(ctx->server);
  if (!v) return;
  if (v->queue) return cgnr_queue_stop(ctx, v);
  if (v->alive) {
    volatile unsigned* ctl = v->ctl;
    if (!ctl[17]) {
      ctl[1] = RLS_SRV_EXIT;
      std::atomic_thread_fence(std::memory_order_release);
      ctl[0] = ++v->seq;
      const auto t0 = std::chrono::steady_clock::now();
      for (unsigned n = 0; !ctl[17]; ++n) {
        rls_cpu_relax();
        if ((n & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(500)) {
          (void)hipSetDevice(ctx->device);
          (void)hipStreamSynchronize(ctx->stream);  // (its idle timeout or its wait bounds end it at the latest)
          break;
        }
      }
    }
  }
  server_life_over(ctx, v);
}

// 0: the command was served (status in the mirror); 1: the kernel had left before it saw the command; 2: it gave up inside it
int server_wait(rls_ctx* ctx, srv_state* v, unsigned mbseq) {
  volatile unsigned* mb = ctx->mb_h;
  volatile unsigned* ctl = v->ctl;
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned n = 0;; ++n) {
    if (*mb == mbseq) break;
    const unsigned ex = ctl[17];
    if (ex) {  // (the status of a served command is published before the kernel can leave: look once more)
      std::atomic_thread_fence(std::memory_order_acquire);
      if (*mb == mbseq) break;
      return (int)ex;
    }
    rls_cpu_relax();
    if ((n & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) {
      (void)hipStreamSynchronize(ctx->stream);
      if (*mb == mbseq) break;
      return ctl[17] == 1 ? 1 : 2;
    }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  return 0;
}

extern "C" {

int32_t rls_operator_create(rls_ctx* ctx, int32_t dtype, int64_t M, int64_t N, const void* A, int64_t lda,
                            rls_operator** out) {
  RLS_CHECK_CTX(ctx);
  if (!out || !rls_dtype_ok(dtype) || M < 0 || N <= 0) return rls_fail(ctx, RLS_E_INVALID, "operator_create: bad argument");
  if (A && (M <= 0 || lda < M)) return rls_fail(ctx, RLS_E_INVALID, "operator_create: bad shape/lda");
  RLS_HIP(ctx, rls_enter(ctx));
  rls_alloc_scope alloc_scope(ctx);
  *out = nullptr;
  rls_operator* op = new rls_operator{plan_memory(ctx)};
  op->ctx = ctx;
  op->ctx_id = ctx->id;
  op->dtype = dtype;
  op->M = M;
  op->N = N;
  op->A = A;
  op->lda = lda;
  if (A) {
    op->mem.dev(&op->t, (size_t)M * rls_elem_size(dtype), false);
    const size_t ws = rls_normal_fused_workspace(ctx, dtype, M, N, A, lda);
    if (ws > 0) op->mem.dev(&op->slab, ws, false);
    if (const int e = op->mem.error()) {
      rls_operator_destroy(op);
      return rls_fail(ctx, e, "operator_create: hipMalloc failed");
    }
  }
  *out = op;
  return 0;
}

int32_t rls_operator_set_gram(rls_operator* op, const void* AHA, int64_t ld) {
  if (!op) return RLS_E_INVALID;
  if (AHA && ld < op->N) return rls_fail(op->ctx, RLS_E_INVALID, "operator_set_gram: ld < N");
  op->G = AHA;
  op->ldg = ld;
  return 0;
}

int32_t rls_operator_destroy(rls_operator* op) {
  if (!op) return RLS_E_INVALID;
  rls_alloc_scope alloc_scope(alloc_ctx_of(op->ctx, op->ctx_id));
  op->mem.release();  // hipFree resolves the owning device from the pointer
  delete op;
  return 0;
}

int32_t rls_operator_mul(rls_operator* op, const void* x, void* y) {
  if (!op) return RLS_E_INVALID;
  if (!op->A) return rls_fail(op->ctx, RLS_E_STATE, "operator_mul: operator has no forward matrix");
  return rls_launch_gemv(op->ctx, op->dtype, RLS_OP_N, op->M, op->N, 1.f, 0.f, op->A, op->lda, x, 0.f, 0.f, y, nullptr);
}
int32_t rls_operator_mul_adj(rls_operator* op, const void* y, void* x) {
  if (!op) return RLS_E_INVALID;
  if (!op->A) return rls_fail(op->ctx, RLS_E_STATE, "operator_mul_adj: operator has no forward matrix");
  return rls_launch_gemv(op->ctx, op->dtype, RLS_OP_C, op->M, op->N, 1.f, 0.f, op->A, op->lda, y, 0.f, 0.f, x, nullptr);
}
// the same with a device flag that turns the launches into no-ops (deferred OptISTA / POGM sequences)
int32_t rls_operator_mul_normal_skip(rls_operator* op, const void* p, void* v, const void* skip_d) {
  if (!op) return RLS_E_INVALID;
  rls_ctx* ctx = op->ctx;
  if (!p || !v) return rls_fail(ctx, RLS_E_INVALID, "operator_mul_normal_skip: null pointer");
  RLS_HIP(ctx, rls_enter(ctx));
  return op_normal(op, p, v, (const int*)skip_d);
}

int32_t rls_operator_mul_normal(rls_operator* op, const void* p, void* v) {
  if (!op || !p || !v) return RLS_E_INVALID;
  return op_normal(op, p, v, nullptr);
}

int32_t rls_gram(rls_ctx* ctx, int32_t dtype, int64_t M, int64_t N, const void* A, int64_t lda, void* G, int64_t ld) {
  RLS_CHECK_CTX(ctx);
  if (!rls_dtype_ok(dtype) || M <= 0 || N <= 0 || !A || !G || lda < M || ld < N)
    return rls_fail(ctx, RLS_E_INVALID, "gram: bad argument");
  RLS_HIP(ctx, rls_enter(ctx));
  if (ctx->tune.batched_mfma && rls_gram_tiles_ok(M, N) && rls_skinny_ok(dtype, M, N, A, lda))
    return rls_gram_tiles(ctx, dtype, M, N, A, lda, G, ld);  // Hermitian 64 x 64 tiles, no scratch
  if (ctx->tune.batched_mfma && N <= 65535 * 16 && rls_skinny_ok(dtype, M, N, A, lda)) {
    // matrix cores: A^H T with T = A in 16-column panels (skinny.hip); M x N scratch for the panels
    void* panels = nullptr;
    rls_alloc_scope alloc_scope(ctx);
    plan_buffers scratch = plan_memory(ctx);
    scratch.dev(&panels, (size_t)M * (size_t)N * rls_elem_size(dtype), false);
    RLS_HIP(ctx, (hipError_t)scratch.error());
    int32_t st = rls_skinny_gram(ctx, dtype, M, N, A, lda, G, ld, panels);
    if (st == 0) st = gram_hermitianize(ctx, dtype, N, G, ld);
    hipError_t e = rls_stream_wait(ctx->stream);  // setup path: the scratch is freed before returning
    scratch.release();
    if (st == 0 && e != hipSuccess) st = rls_fail(ctx, (int32_t)e, hipGetErrorString(e));
    return st;
  }
  dim3 grid((unsigned)((N + 63) / 64), (unsigned)((N + 63) / 64));
  RLS_TRY(rls_with_elem(dtype, [&](auto t) {
    using E = typename decltype(t)::type;
    return rls_launch<gram_kernel<E>>(ctx, grid, dim3(256), 0, (const E*)A, lda, M, N, (E*)G, ld);
  }));
  return gram_hermitianize(ctx, dtype, N, G, ld);
}

}  // extern "C"
