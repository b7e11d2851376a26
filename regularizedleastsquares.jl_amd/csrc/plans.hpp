// What the solver plans share.  Internal: included by operator.hip, solvers.hip and the plan_*.hip files only, and the only
// place two plans meet.  The operator handle, the plans' arena and their shared matrix-core operands, hipGraph chunking, the
// resident-launch slot, the host state of server mode, the status read-back with its lost-launch recovery, and the descriptor
// builders that CGNR and cg! have in common.  Everything defined here is a template, a struct or a static inline function, so a
// step call inlines in its plan's file what it needs; what has state or bulk is declared here and defined once (operator.hip;
// the one function that is CGNR's, cgnr_queue_stop, with CGNR).
//
// One iteration = the normal-operator apply (two GEMVs, matrix-free; one in Gram mode) plus ONE
// single-workgroup "update" kernel that holds every scalar (alpha, beta, zeta, theta, residuals,
// iteration count, done flag) in device memory, so the host never synchronises inside the loop
// (the reference's generic GPU path pays 4-5 blocking scalar read-backs per iteration).
// Once `done` is set every later kernel of the plan exits at entry, which reproduces the
// reference's "stop at the first iteration where done() holds" exactly while letting the host
// enqueue iterations in hipGraph-captured chunks.
#pragma once
#include "rls_common.hpp"
#include "plan_buffers.hpp"

#include <algorithm>
#include <mutex>
#include <vector>

// ---- allocation: the plans' scratch comes from the stream-ordered pool of the context named by the innermost
// rls_alloc_scope of the calling thread; the pinned status mirrors from the process-wide free list (rls_common.hpp) ----
// Every plan's blocks have one owner (plan_buffers.hpp): the plan's FIRST member `mem`, so that `new T{plan_memory(ctx)}`
// initialises every member after it from its default initialiser.  Requests and release() run inside the plan's rls_alloc_scope.
static inline plan_buffers plan_memory(rls_ctx* ctx) {
  return plan_buffers([](void** p, size_t bytes) { return (int)rls_scoped_malloc(p, bytes); }, [](void* p) { (void)rls_scoped_free(p); },
                      [](void** p, size_t bytes) { return (int)rls_pinned_alloc(p, bytes); }, [](void* p) { rls_pinned_free(p); },
                      [ctx](void* p, size_t bytes) { return (int)hipMemsetAsync(p, 0, bytes, ctx->stream); });
}
// the context a plan allocated from, if it still exists (plans may outlive their context in a garbage-collected host)
// (pointer AND generation id: a destroyed context's address can be handed out again to a new one, possibly on another device)
static inline rls_ctx* alloc_ctx_of(rls_ctx* ctx, uint64_t id) { return rls_ctx_alive(ctx, id) ? ctx : nullptr; }

// ---------------------------------------------------------------------------------------------
// operator
// ---------------------------------------------------------------------------------------------
struct rls_operator {
  plan_buffers mem;
  rls_ctx* ctx = nullptr;
  uint64_t ctx_id = 0;  // ctx->id at creation (alloc_ctx_of)
  int32_t dtype = 0;
  int64_t M = 0, N = 0;
  const void* A = nullptr;  // may be null (Gram-only operator)
  int64_t lda = 0;
  const void* G = nullptr;  // Gram matrix (N x N) or null
  int64_t ldg = 0;
  void* t = nullptr;        // length-M scratch for the matrix-free normal operator
  void* slab = nullptr;     // per-workgroup partial-v slab of the fused one-pass normal operator (or null)
};

// The matrix-core operands of a shared-A batched plan (skinny.hip): K right-hand sides over one pass of A.  The plan's
// per-column kernels write their next points into `panel`, the T kernel reads it and leaves T = A P in Tpack, the V kernel
// leaves A^H T as `splits` partial rows per column in Vpart (with an explicit AHA: one product, panel -> Vpart).
struct shared_operands {
  float *panel = nullptr, *Tpack = nullptr;
  void* Vpart = nullptr;
  int splits = 1;
  int half = 0;  // operand-panel layout, fixed at creation (rls_skinny_half)

  // the shapes the matrix-core kernels take: A, and AHA when it is explicit
  static bool supported(const rls_operator* op) {
    return op->A && rls_skinny_ok(op->dtype, op->M, op->N, op->A, op->lda) &&
           (!op->G || rls_skinny_ok(op->dtype, op->N, op->N, op->G, op->ldg));
  }
  void alloc(plan_buffers& mem, const rls_operator* op, int nrhs) {
    size_t pb, tb, vb;
    rls_skinny_sizes(op->ctx, op->dtype, op->M, op->N, nrhs, &pb, &tb, &vb, &splits);
    half = rls_skinny_half(op->ctx, op->dtype, nrhs);
    mem.dev(&panel, pb, true);  // the padding columns of the last group stay zero
    mem.dev(&Tpack, tb, false);
    mem.dev(&Vpart, vb, false);
  }
  bool allocated() const { return Vpart != nullptr; }  // "this plan is a batched one", whatever its nrhs

  // the products' descriptor; X / R / P / V / sc are the batched CGNR update's (skinny_u_kernel), null for every other plan
  rls_skinny desc(const rls_operator* op, int nrhs, int64_t ldv) const {
    rls_skinny K;
    K.A = op->A;
    K.lda = op->lda;
    K.M = op->M;
    K.N = op->N;
    K.G = op->G;  // explicit AHA (src/CGNR.jl:49): every operator apply of the batched loop is ONE product over it
    K.ldg = op->ldg;
    K.nrhs = nrhs;
    K.half = half;
    K.ngroups = rls_skinny_groups(nrhs, half);
    K.splits = splits;
    K.X = K.R = K.P = K.V = nullptr;
    K.ldv = ldv;
    K.Ppack = panel;
    K.Tpack = Tpack;
    K.Vpart = Vpart;
    K.ldvp = op->N;
    K.sc = nullptr;
    return K;
  }
  // what the per-column kernels get (rls_common.hpp)
  rls_operands erased(int nrhs) const { return rls_operands{Vpart, splits, rls_skinny_pad(nrhs, half), panel, half}; }
  template <typename E>
  operand_view<E> view(int nrhs) const { return operand_view<E>(erased(nrhs)); }
};

static inline int32_t op_normal(rls_operator* op, const void* p, void* v, const int* skip) {
  rls_ctx* ctx = op->ctx;
  if (op->G) return rls_launch_gemv(ctx, op->dtype, RLS_OP_N, op->N, op->N, 1.f, 0.f, op->G, op->ldg, p, 0.f, 0.f, v, skip);
  if (!op->A) return rls_fail(ctx, RLS_E_STATE, "operator has neither A nor a Gram matrix");
  if (op->slab && ctx->tune.fused_normal)
    return rls_launch_normal_fused(ctx, op->dtype, op->M, op->N, op->A, op->lda, p, v, op->slab, skip);
  RLS_TRY(rls_launch_gemv(ctx, op->dtype, RLS_OP_N, op->M, op->N, 1.f, 0.f, op->A, op->lda, p, 0.f, 0.f, op->t, skip));
  return rls_launch_gemv(ctx, op->dtype, RLS_OP_C, op->M, op->N, 1.f, 0.f, op->A, op->lda, op->t, 0.f, 0.f, v, skip);
}

// ---------------------------------------------------------------------------------------------
// hipGraph chunking shared by the three plans
// ---------------------------------------------------------------------------------------------
struct step_graph {
  hipGraphExec_t exec = nullptr;
  int steps = 0;
  void* x_bound = nullptr;  // cg plans: the solution vector whose address the captured kernels carry
  int mode = 0;  // which kernel sequence was captured
  bool failed = false;
  uint64_t epoch = 0;  // rls_ctx::tune_epoch at capture: launch shapes and kernel choices follow the context's switches
  // forget the cached graph (another kernel sequence, other baked arguments, the plan goes away): the next step call captures afresh
  void drop() {
    if (exec) hipGraphExecDestroy(exec);
    *this = step_graph();
  }
  // the call about to run captures / replays kernel sequence `m` on solution vector `x` (the captured kernels carry its address):
  // a graph cached for another key is dropped
  void keep_for(int m, void* x = nullptr) {
    if (exec && (mode != m || x_bound != x)) drop();
    mode = m;
    x_bound = x;
  }
};

// `rewind(c)`: a capture that fails has already called enqueue_one c times WITHOUT any of those launches running; a
// caller whose callback keeps a position (parity, launch index) gets the chance to step it back before the eager retry.
template <typename F, typename R>
static int32_t run_steps(rls_ctx* ctx, step_graph* big, int n_steps, F&& enqueue_one, R&& rewind) {
  const int chunk = ctx->tune.graph_chunk;
  while (n_steps > 0) {
    if (ctx->tune.use_graph && chunk > 1 && n_steps >= chunk && !big->failed) {
      if (!big->exec || big->steps != chunk || big->epoch != ctx->tune_epoch) {
        if (big->exec) {
          hipGraphExecDestroy(big->exec);
          big->exec = nullptr;
        }
        hipGraph_t graph = nullptr;
        std::unique_lock<std::mutex> capture_lock(rls_capture_mutex());
        hipError_t e = hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeRelaxed);
        int32_t st = 0;
        int calls = 0;
        if (e == hipSuccess) {
          for (int i = 0; i < chunk && st == 0; ++i, ++calls) st = enqueue_one();
          e = hipStreamEndCapture(ctx->stream, &graph);
        }
        capture_lock.unlock();
        if (e != hipSuccess || st != 0 || !graph ||
            hipGraphInstantiate(&big->exec, graph, nullptr, nullptr, 0) != hipSuccess) {
          big->failed = true;  // fall back to eager launches (still the HIP kernels)
          big->exec = nullptr;
          (void)hipGetLastError();
          rewind(calls);
        } else {
          big->steps = chunk;
          big->epoch = ctx->tune_epoch;
        }
        if (graph) hipGraphDestroy(graph);
        if (big->failed) continue;
      }
      RLS_HIP(ctx, hipGraphLaunch(big->exec, ctx->stream));
      n_steps -= chunk;
    } else {
      RLS_TRY(enqueue_one());
      n_steps -= 1;
    }
  }
  return 0;
}

template <typename F>
static int32_t run_steps(rls_ctx* ctx, step_graph* big, int n_steps, F&& enqueue_one) {
  return run_steps(ctx, big, n_steps, enqueue_one, [](int) {});
}

// Which (r, p) pair launch k of a step call finds current (rls_cgnr_pipe::cur_hint): the call starts at pair 0
// with nothing pending, launch 0 flips nothing, every later launch flips.  Launches at a chunk boundary may be
// the first node of a REPLAYED graph, whose captured hint belongs to another position in the sequence, so they
// get "unknown"; so does everything when the chunk length is odd (replays would be out of phase).
static inline int pipe_cur_hint(const rls_ctx* ctx, int k) {
  const int chunk = ctx->tune.graph_chunk;
  if (ctx->tune.pipe_hint_mode == 1) return -1;
  if (ctx->tune.pipe_hint_mode == 2) return k == 0 ? 1 : (k & 1);  // the opposite of the bookkeeping below
  if (k == 0) return (ctx->tune.use_graph && chunk > 1) ? -1 : 0;
  if (ctx->tune.use_graph && chunk > 1 && (chunk % 2 != 0 || k % chunk == 0)) return -1;
  return (k - 1) & 1;
}

// ---------------------------------------------------------------------------------------------
// resident launches: the chain across streams, and what a plan keeps to run them and to notice lost ones
// ---------------------------------------------------------------------------------------------
static inline bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }
template <typename... P>
static inline bool aligned16(const void* q, P... more) { return aligned16(q) && aligned16(more...); }

// the chain of resident launches across the streams of this process: ONE per process, defined in operator.hip (hidden: not
// part of the library's dynamic symbol table, reached without the GOT as when they were file-local)
extern __attribute__((visibility("hidden"))) hipEvent_t g_resident_ev[64];
extern __attribute__((visibility("hidden"))) resident_chain_state g_resident_chain;

// What a plan needs to run resident launches and to notice lost ones.  A launch whose workgroups were not all on the chip in
// time is a no-op (x, r, p and the scalars are written back by workgroup 0 only after its last barrier) that counts itself in
// the sync block's sticky third flag word; the plan's next status read fetches the flags, and the plan re-runs what is missing
// on the per-iteration pipeline (status_recover below; cg!, the PGM plans and ADMM have their own re-run rule).  `off` and
// `fallbacks` (resident_loss_state, host_pool.hpp): the plan stays off the resident kernels from its first loss on.
struct resident_slot : resident_loss_state {
  void* sync = nullptr;         // device: arrival counters, {fail, completed, failed} (resident_sync.hpp), the exchange's group partials
  unsigned* flags_h = nullptr;  // pinned mirror of the three flag words, read with the status
  bool used = false;            // a resident launch went out since the last status read: that read fetches the flags
  bool clean = false;           // the plan's init kernel has just zeroed the arrival counters itself (chain)

  // the sync block (its head zeroed once: the sticky word starts at 0) and the pinned mirror, from the owning plan's arena.  A plan
  // for which resident mode is only an optimisation asks between mark() and rollback(): without the block its pipeline runs
  void alloc(plan_buffers& mem, rls_ctx* ctx, const rls_operator* op) {
    mem.dev(&sync, rls_resident_sync_alloc_bytes(op->dtype, op->N), false);
    if (sync) mem.fail((int)hipMemsetAsync(sync, 0, rls_cgnr_resident_sync_bytes(), ctx->stream));
    mem.pinned(&flags_h, 4 * sizeof(unsigned), true);
  }
  bool usable(const rls_ctx* ctx) const { return sync && !off && ctx->tune.resident; }

  // `launch(sync, spin_limit)` as the next link of the device's chain, behind the memset of the arrival counters and of the
  // {fail, completed} words of THIS launch (the count of lost launches behind them is sticky).  `clean`: the init kernel has
  // zeroed them and nothing has used them since -- the memset (a launch of its own: ~4 us on the stream between init! and the
  // resident kernel of every solve) is skipped, once.
  template <typename F>
  int32_t chain(rls_ctx* ctx, F&& launch) {
    const int d = ctx->device < 64 ? ctx->device : 63;
    return resident_chain_step(
        rls_capture_mutex(), g_resident_chain, ctx->device, (void*)ctx->stream,
        [&](void* prev) -> int32_t {  // the chain changes streams: order this launch behind everything the previous stream has queued
          if (!g_resident_ev[d]) RLS_HIP(ctx, hipEventCreateWithFlags(&g_resident_ev[d], hipEventDisableTiming));
          RLS_HIP(ctx, hipEventRecord(g_resident_ev[d], (hipStream_t)prev));
          RLS_HIP(ctx, hipStreamWaitEvent(ctx->stream, g_resident_ev[d], 0));
          return 0;
        },
        [&]() -> int32_t {
          if (clean && ctx->tune.resident_preclear) clean = false;
          else RLS_HIP(ctx, hipMemsetAsync(sync, 0, rls_resident_sync_clear_bytes(), ctx->stream));
          if (!ctx->tune.resident_l2_rows)  // measurement switch: pretend a workgroup is misplaced -- partial rows are written through
            RLS_HIP(ctx, hipMemsetAsync((char*)sync + rls_resident_sync_placement_offset(), 1, 1, ctx->stream));
          return launch(sync, (unsigned)ctx->tune.resident_spin);
        });
  }
  // a launch the plan's next status read has to account for (the launches of a kernel that stays and listens are accounted for
  // when its life ends: srv_state::resident_used; the PGM plans count theirs in rls_pgm_lost)
  template <typename F>
  int32_t launch(rls_ctx* ctx, F&& f) {
    used = true;
    return chain(ctx, f);
  }

  // enqueue the read-back of {fail, completed, failed}; the caller synchronises (normally with its scalar read-back)
  int32_t fetch_flags(rls_ctx* ctx) {
    return rls_fetch_add(ctx, (const char*)sync + rls_resident_sync_flags_offset(), flags_h, 3 * sizeof(unsigned));
  }
  // Launches lost since the last call (0 = none), behind a fetch_flags() the host has waited for.  The plan is off the resident
  // kernels from here on, and a context that has met losses twice stops using them at all (resident_note_lost, host_pool.hpp).
  unsigned lost(rls_ctx* ctx) {
    const unsigned n = flags_h[2];
    if (!n) return 0;
    (void)hipMemsetAsync((char*)sync + rls_resident_sync_flags_offset() + 2 * sizeof(unsigned), 0, sizeof(unsigned), ctx->stream);
    flags_h[2] = 0;
    if (resident_note_lost(*this, ctx->resident_failures, n)) ctx->tune.resident = 0;
    return n;
  }
};

// server mode of a plan's resident kernel (rls_cg_start::srv_ctl / rls_srv_args): the control block in pinned host memory and what
// the host knows about the kernel it left listening.  rls_ctx::server points at the one that is alive on the context's stream.
struct srv_state {
  unsigned* ctl = nullptr;
  bool alive = false;   // a kernel was left listening (it may have left on its own since: ctl[17])
  bool fresh = false;   // ... and the plan's status mirror holds the status of its last command
  bool off = false;     // lives that served fewer than three commands, twice in a row (the caller touches the device between
  int served = 0, short_lives = 0;  // iterates: a listening kernel only stands in its way): per-iteration pipeline until init!
  unsigned seq = 0;
  bool* resident_used = nullptr;  // the plan's flag: "a status call must read the sync block's flags" (set when a life ends)
  // queue mode (rls_cgnr plans, cgnr_queue_post): the life alive serves the command ring behind ctl
  bool queue = false;
  bool q_pending = false;  // an init! of rls_cgnr_init waits for the rls_cgnr_step that posts it
  unsigned q_pay[5] = {};  // ... its payload {maxiter, b low, b high, lambda, relTol}
  unsigned q_last = 0;     // the sequence number of the last command other than EXIT posted to the ring
  void* q_plan = nullptr;  // the rls_cgnr the ring belongs to
};

// The 32-word control block, if it can be had: server mode is an optimisation, a plan without the block answers every step call
// with a launch of its own.
static inline bool server_ctl_optional(plan_buffers& mem, srv_state* v) {
  if (mem.error()) return false;
  const plan_buffers::mark_t m = mem.mark();
  mem.pinned(&v->ctl, 32 * sizeof(unsigned), true);
  if (mem.error()) mem.rollback(m);
  return v->ctl != nullptr;
}

// ---- resident kernels in server mode (rls_cg_start::srv_ctl, rls_srv_args) ---------------------------------------------------------
// rls_cgnr_step_status / rls_fista_step_status on a plan whose A lives in the register files do not let the kernel end: the next
// call posts {n_steps, mailbox sequence, command sequence} into the pinned control block the kernel listens on and spins on the
// mailbox -- no launch, no load of A per call.  Everything else that wants the stream sends EXIT first (rls_enter -> rls_server_stop).
__attribute__((visibility("hidden"))) bool server_usable(const rls_ctx* ctx, const srv_state* v);
__attribute__((visibility("hidden"))) void server_life_over(rls_ctx* ctx, srv_state* v);
__attribute__((visibility("hidden"))) int server_wait(rls_ctx* ctx, srv_state* v, unsigned mbseq);
__attribute__((visibility("hidden"))) void cgnr_queue_stop(rls_ctx* ctx, srv_state* v);  // rls_server_stop on a queue life (defined with CGNR)

// One command: posted to the listening kernel, or carried by a launch (`launch(args)`, through the resident chain).
// Returns 0 = served (mirror current), 1 = nothing ran and the plan should take its ordinary path, 2 = a launch gave up inside
// the command (the caller's lost-launch recovery re-runs it), < 0 = error.
template <typename L>
static int32_t server_command(rls_ctx* ctx, srv_state* v, void* mirror, int32_t n_steps, bool usable_again, L&& launch) {
  volatile unsigned* ctl = v->ctl;
  for (int attempt = 0; attempt < 2; ++attempt) {
    const unsigned mbseq = ++ctx->mb_seq;
    if (v->alive) {  // post the command: payload, then the sequence word
      ctl[1] = (unsigned)n_steps;
      ctl[2] = mbseq;
      std::atomic_thread_fence(std::memory_order_release);
      ctl[0] = ++v->seq;
      std::atomic_thread_fence(std::memory_order_seq_cst);
    } else {
      ctl[16] = ctl[17] = 0;
      ctl[0] = v->seq;
      rls_srv_args a;
      a.ctl = v->ctl;
      a.seq0 = v->seq;
      a.idle_us = (unsigned)(ctx->tune.resident_server_idle_us > 0 ? ctx->tune.resident_server_idle_us : 1);
      if (ctx->tune.resident_ahead) a.idle_us |= RLS_SRV_AHEAD;  // (read by the single-workgroup kernels; the resident launches below mask it)
      a.mb.dst = mirror;
      a.mb.seq_h = ctx->mb_h;
      a.mb.seq = mbseq;
      const int32_t st = launch(a);
      if (st != 0) return st < 0 ? st : -1;
      v->alive = true;
      v->served = 0;
      ctx->server = v;
    }
    const int r = server_wait(ctx, v, mbseq);
    if (r == 0) {
      v->served += 1;
      v->fresh = true;
      return 0;
    }
    server_life_over(ctx, v);
    if (r == 2) {
      if (v->resident_used) *v->resident_used = true;  // (the status call that follows reads the sync block's flags)
      return 2;
    }
    // r == 1: it had left (idle) before it saw the command -- nothing ran.  Once more with a launch, or -- this plan's lives
    // keep ending early -- on the ordinary path
    if (attempt == 1 || !usable_again || v->off) {
      v->off = true;
      return 1;
    }
  }
  return 1;
}

// the Gram-mode pipeline's view of a CGNR recurrence (a CGNR plan's own, or cg! on AHA + rho I: p = u, v = c): index 0 = the
// caller's vectors, 1 = the second parity in plan scratch
static inline rls_gram_pipe gram_pipe_desc(const rls_operator* op, void* x, void* r, void* r1, void* p, void* p1, void* v, void* v1,
                                    double* gdots, cgnr_scalars* sc, cgnr_scalars* scn) {
  rls_gram_pipe P;
  P.G = op->G;
  P.ldg = op->ldg;
  P.N = op->N;
  P.x = x;
  P.r[0] = r;
  P.r[1] = r1;
  P.p[0] = p;
  P.p[1] = p1;
  P.v[0] = v;
  P.v[1] = v1;
  P.dots = gdots;
  P.sc[0] = sc;
  P.sc[1] = scn;
  return P;
}

// the matrix-free pipeline's view of a CGNR recurrence (as gram_pipe_desc); the batch fields keep their single-column defaults
static inline rls_cgnr_pipe pipe_desc(const rls_operator* op, void* x, void* r, void* r1, void* p, void* p1, void* v, double* dots,
                               cgnr_scalars* sc, cgnr_scalars* scn) {
  rls_cgnr_pipe P;
  P.A = op->A;
  P.lda = op->lda;
  P.M = op->M;
  P.N = op->N;
  P.x = x;
  P.r0 = r;
  P.p0 = p;
  P.r1 = r1;
  P.p1 = p1;
  P.v = v;
  P.slab = op->slab;
  P.dots = dots;
  P.ndots = (int)((op->N + 15) / 16);
  P.sc = sc;
  P.scn = scn;
  return P;
}

constexpr int UPD_THREADS = 1024;

// Batched plans (shared A: rls_fista_create_batched, rls_cg_create_batched): the per-column kernels of FISTA, cg! and ADMM run
// one workgroup per column (blockIdx.x = column, state matrices N x K with leading dimension ldv, one scalar struct per
// column); the operator apply in front of them is the pair of skinny matrix-core products.  ops.Vpart non-null: AHA y arrives
// as partial rows and is summed here; ops.panel non-null: the kernel's next point also goes into the operand panel.
// The default = the single-column plans.
template <typename E>
struct col_batch {
  int64_t ldv = 0;
  operand_view<E> ops;
  int skip_stride = 0;      // ints between the columns' skip flags (ADMM)
  int64_t log_stride = 0;   // floats between the columns' ADMM logs
};

// a plan's scalars on the device and their pinned mirror, both zeroed
template <typename S>
static void alloc_scalars(plan_buffers& mem, S** d, S** h, int n = 1) {
  mem.dev(d, sizeof(S) * n, true);
  mem.pinned(h, sizeof(S) * n, true);
}
template <typename S>
static int32_t fetch_scalars(rls_ctx* ctx, S* d, S* h) {
  static_assert(sizeof(S) % 4 == 0, "status structs are copied dword by dword");
  RLS_TRY(rls_fetch_add(ctx, d, h, sizeof(S)));
  return rls_fetch_wait(ctx);  // one publishing launch for everything queued (resident flags, logs), then the host sees it
}

// ---- status read-back of a CGNR / FISTA plan, with the recovery of lost resident launches -----------------------------------------
// `h`: the pinned mirror of the plan's `nrhs` scalar structs.  First half: enqueue the read-back of the scalars and, behind
// resident launches, of the sync block's flags; the caller waits (rls_fetch_wait: one publishing launch for everything queued).
template <typename Plan, typename S>
static int32_t status_fetch_add(rls_ctx* ctx, Plan* s, S* h, int nrhs) {
  static_assert(sizeof(S) % 4 == 0, "status structs are copied dword by dword");
  if (s->resident.used) RLS_TRY(s->resident.fetch_flags(ctx));
  return rls_fetch_add(ctx, s->sc, h, sizeof(S) * (size_t)nrhs);
}
// Second half, the mirrors being current.  A lost resident launch changed nothing: the live columns are all at the same count
// (they advance in lockstep since init; retired ones stay behind), so what is missing is `requested` - that count, and
// `rerun(n)` runs it on the plan's per-iteration path -- the plan is off the resident kernels by then -- before the scalars are
// read again.  `on_lost(count)`: what else of the plan follows the device's count.  Every resident launch up to here is then
// accounted for (the lost count is sticky until it is read).
template <typename Plan, typename S, typename R, typename L>
static int32_t status_recover(rls_ctx* ctx, Plan* s, S* h, int nrhs, R&& rerun, L&& on_lost) {
  if (s->resident.used && s->resident.lost(ctx)) {
    long long at = 0;
    bool live = false;
    for (int b = 0; b < nrhs; ++b) {
      if (h[b].iteration > at) at = h[b].iteration;
      live = live || !h[b].done;
    }
    on_lost(at);
    const long long missing = s->requested - at;
    if (live && missing > 0) {
      RLS_TRY(rerun((int32_t)(missing > 0x7fffffff ? 0x7fffffff : missing)));
      RLS_TRY(rls_fetch_add(ctx, s->sc, h, sizeof(S) * (size_t)nrhs));
      RLS_TRY(rls_fetch_wait(ctx));
    }
  }
  s->resident.used = false;
  return 0;
}
template <typename Plan, typename S, typename R, typename L>
static int32_t status_read(rls_ctx* ctx, Plan* s, S* h, int nrhs, R&& rerun, L&& on_lost) {
  RLS_TRY(status_fetch_add(ctx, s, h, nrhs));
  RLS_TRY(rls_fetch_wait(ctx));
  return status_recover(ctx, s, h, nrhs, rerun, on_lost);
}

// One iterate per call is the reference's solve! loop with callbacks (src/RegularizedLeastSquares.jl:161-176): step and read-back
// as ONE entry point (rls_cgnr_step_status, rls_fista_step_status).
//   `serve`: the plan's resident kernel in server mode -- the command is posted to the kernel left listening, or carried by
// `serve_launch(args)` (whole-solve calls gain nothing from a kernel that stays: per-iterate calls of up to 8 steps only).
// `account(+-n)` books the command's iterations into the plan's counts and takes them back when nothing ran.
//   Otherwise `step`, and on the per-iteration pipeline and the small-system kernel the call's last kernel stores the scalars into
// the plan's pinned mirror itself (the armed mailbox slot) -- no publishing launch behind it; where the path did not take the
// slot, `get_status`.
template <typename Plan, typename Status, typename SL, typename A, typename St, typename G, typename F>
static int32_t step_status(Plan* s, int32_t n_steps, Status* out, bool serve, SL&& serve_launch, A&& account, St&& step, G&& get_status,
                           F&& status_out) {
  rls_ctx* ctx = s->op->ctx;
  if (serve && s->initialised && n_steps > 0 && n_steps <= 8 && !s->resident.used) {
    RLS_HIP(ctx, hipSetDevice(s->device));
    account(n_steps);
    const int32_t r = server_command(ctx, &s->srv, s->sc_h, n_steps, true, serve_launch);
    if (r < 0) return r;
    if (r == 0) {
      status_out(s, *s->sc_h, out);
      return 0;
    }
    if (r == 2) return get_status(s, out);  // a launch gave up inside the command: the lost-launch recovery re-runs it
    account(-n_steps);  // r == 1, nothing ran (and the plan's server mode is off): the ordinary path
  }
  if (s->initialised && s->nrhs == 1 && n_steps > 0 && !s->resident.used) {
    RLS_HIP(ctx, rls_enter(ctx));
    s->mb_arm = rls_mailbox_arm(ctx, s->sc_h);
  }
  s->mb_sent = false;
  const int32_t st = step(s, n_steps);
  const rls_mailbox_slot mb = s->mb_arm;
  s->mb_arm = rls_mailbox_slot();
  if (st != 0) return st;
  if (!s->mb_sent) return get_status(s, out);
  RLS_TRY(rls_mailbox_wait(ctx, mb.seq));
  status_out(s, *s->sc_h, out);
  return 0;
}

// ---- helpers of the row-sharded entry points (templates: C++ linkage) --------------------------------------------------
template <typename PlanT>
static int32_t rowsharded_check(rls_comm* comm, PlanT* const* plans, rls_operator* (*op_of)(PlanT*), bool (*single)(PlanT*)) {
  if (!comm || !plans) return RLS_E_INVALID;
  const int n = rls_comm_size(comm);
  for (int r = 0; r < n; ++r) {
    rls_ctx* cr = nullptr;
    RLS_TRY(rls_comm_ctx(comm, r, &cr));
    if (!plans[r]) return rls_fail(cr, RLS_E_INVALID, "rowsharded: null plan");
    rls_operator* op = op_of(plans[r]);
    if (op->ctx != cr) return rls_fail(cr, RLS_E_INVALID, "rowsharded: plan r must live on the communicator's context r");
    if (!single(plans[r]) || op->N != op_of(plans[0])->N || op->dtype != op_of(plans[0])->dtype)
      return rls_fail(cr, RLS_E_INVALID, "rowsharded: the shards must share N and the element type (single right-hand side)");
    if (!op->A) return rls_fail(cr, RLS_E_INVALID, "rowsharded: a row shard needs its matrix (no Gram-only operators)");
  }
  return 0;
}
