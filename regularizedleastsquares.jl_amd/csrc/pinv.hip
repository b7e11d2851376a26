// PseudoInverse (src/Direct.jl:70-162): x = V diag(sigma / (sigma^2 + lambda)) U^H b from a one-sided (Hestenes) Jacobi SVD of A
// on the device.  svt.hip runs the same method on small matrices inside one CU's LDS; here ONE large matrix lives in HBM and the
// whole chip works on it.
//
// W := a copy of A (M x N) and V := I (N x N), both plan-owned.  Column pairs of W, and the same pairs of V, are rotated in
// the round-robin tournament order of svt.hip (a dummy player for odd N) until every pair is orthogonal to rounding.  The
// invariant is A = W V^H with the columns of W orthogonal and of norm sigma_j; U = W Sigma^-1 is never formed, and the solve
// x = V diag(1 / (sigma^2 + lambda)) W^H b needs no division by sigma_j.
//
// The plan pads the leading dimensions of W and V to a multiple of 16 bytes and keeps the padding rows ZERO (a rotation maps
// zeros to zeros), so every kernel reads and writes W and V in 16-byte chunks with no tail; the caller's A (any lda, any
// alignment) is read element by element, once, by the load kernel, and B by the product kernel (below).
//
//   pinv_load_kernel    W = A (padding rows zero), V = I.
//   pinv_round_kernel   ONE launch per tournament round; the launch boundary is the only synchronisation.  The pairs of a round
//                       are disjoint and one workgroup owns one pair: it streams the two W columns once, accumulating
//                       a = |w_p|^2, b = |w_q|^2, g = w_p^H w_q (and keeps the chunks in LDS where 2 M elements fit 64 KiB;
//                       otherwise it reads them again), reduces in a fixed order, forms (c, s, e^{i phi}) with the
//                       renormalisation of svt.hip, rotates and stores the W pair, then the V pair.  A workgroup that rotated
//                       stores 1 into the plan's sweep word: a plain store, every writer writes the same value.  The host
//                       clears the word before a sweep and reads it once behind the sweep's launches; no loop on the device
//                       depends on data.
//   pinv_norms_kernel   sigma_j^2 = |w_j|^2, one workgroup per column; pinv_fro_kernel adds them up, |A|_F^2, in one workgroup.
//                       Both run once ahead of the sweeps (the null level below needs |A|_F) and once behind the last one.
//   pinv_wtb_kernel     t_j = w_j^H b / (sigma_j^2 + lambda), one wave per column; t_j = 0 where sigma_j <= 1e-6 |A|_F.
//   pinv_vt_kernel      x = V t, then the projection (RLS_PROJ_*) on the store.
//
// Vectors at the null level (|w| <= 1e-6 |A|_F) are left alone by the rotations, as in svt.hip, so below that level the
// columns of W are NOT orthogonal and their "singular values" are rounding noise: the solve drops them.  That is the one
// deviation from src/Direct.jl:158, which has no truncation (LAPACK hands it noise-level sigma).
//
// Every sum runs in a fixed order: two factorisations of the same A give the same bits, and a column of a K-column solve has
// the bits of a vector solve.  No atomics, no grid-wide synchronisation, no resident kernel.
#include "rls_common.hpp"

constexpr int PTHREADS = 256;             // four waves per workgroup in every kernel but pinv_vt_kernel
constexpr int PINV_LDS_BYTES = 64 * 1024;  // the W pair stays in LDS up to this size (2 columns): 8192 rows Float32, 4096 ComplexF32
constexpr int PINV_RED_BYTES = 4 * (PTHREADS / 64) * sizeof(float);  // the four sums of a pair, per wave
constexpr int VT_WAVES = 16;              // pinv_vt_kernel: the waves of a workgroup share the columns of V
constexpr float PINV_TOL = 2e-7f;         // a pair is orthogonal when |g| <= tol |w_p| |w_q|  (svt.hip)
constexpr float PINV_NULL = 1e-6f;        // null level, relative to |A|_F  (svt.hip)

// grid: N workgroups, one per column c
template <typename E>
__global__ __launch_bounds__(PTHREADS) void pinv_load_kernel(const E* __restrict__ A, int64_t lda, int64_t M, int64_t N, E* __restrict__ W,
                                                             int64_t ldw, E* __restrict__ V, int64_t ldv) {
  const int64_t c = blockIdx.x;
  for (int64_t r = threadIdx.x; r < ldw; r += PTHREADS) W[r + c * ldw] = r < M ? A[r + c * lda] : elem<E>::zero();
  for (int64_t r = threadIdx.x; r < ldv; r += PTHREADS) V[r + c * ldv] = r == c ? elem<E>::make(1.f, 0.f) : elem<E>::zero();
}

// the four sums of a pair over the workgroup's four waves, in a fixed order, in every thread
__device__ static inline void pinv_block_sum4(float& a, float& b, float& gr, float& gi, float* red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  a = wave_sum(a);
  b = wave_sum(b);
  gr = wave_sum(gr);
  gi = wave_sum(gi);
  if (lane == 0) {
    red[4 * w + 0] = a;
    red[4 * w + 1] = b;
    red[4 * w + 2] = gr;
    red[4 * w + 3] = gi;
  }
  __syncthreads();
  a = b = gr = gi = 0.f;
#pragma unroll
  for (int i = 0; i < PTHREADS / 64; ++i) {
    a += red[4 * i + 0];
    b += red[4 * i + 1];
    gr += red[4 * i + 2];
    gi += red[4 * i + 3];
  }
}

// (p', q') = (c p - s e^{-i phi} q, s p + c e^{-i phi} q) on one 16-byte chunk of each column
template <typename E>
__device__ static inline void pinv_rotate(chunk<E, elem<E>::vec>& p, chunk<E, elem<E>::vec>& q, float c, float s, E ph) {
#pragma unroll
  for (int e = 0; e < elem<E>::vec; ++e) {
    const E wp = p.e[e];
    const E qt = elem<E>::mulc(ph, q.e[e]);
    p.e[e] = elem<E>::sub(elem<E>::scale(c, wp), elem<E>::scale(s, qt));
    q.e[e] = elem<E>::add(elem<E>::scale(s, wp), elem<E>::scale(c, qt));
  }
}
template <typename E>
__device__ static inline void pinv_store(E* p, const chunk<E, elem<E>::vec>& c) {
  *reinterpret_cast<f4*>(p) = __builtin_bit_cast(f4, c);
}

// Round `round` of the tournament on m = N + (N & 1) players: grid m / 2 workgroups, workgroup i owns the pair (p, q).
// nw = ldw / vec, nv = ldv / vec chunks per column.  KEEP: the W pair's chunks stay in LDS (2 nw chunks, at most PINV_LDS_BYTES) between
// the sums and the rotation; each thread reads back only what it stored itself, so the stash needs no barrier of its own.
// stats = {sigma_j^2 [N], |A|_F^2}: only |A|_F^2 (the null level) is read.
template <typename E, bool KEEP>
__global__ __launch_bounds__(PTHREADS) void pinv_round_kernel(E* __restrict__ W, int64_t ldw, E* __restrict__ V, int64_t ldv, int N, int round,
                                                              const float* __restrict__ stats, int* __restrict__ rotated) {
  extern __shared__ __align__(16) unsigned char pinv_lds[];
  float* red = reinterpret_cast<float*>(pinv_lds);  // PINV_RED_BYTES, then the stash
  constexpr int VEC = elem<E>::vec;
  using CH = chunk<E, VEC>;
  const int m = N + (N & 1), i = blockIdx.x, tid = threadIdx.x;
  int p = i == 0 ? m - 1 : (round + i) % (m - 1);
  int q = i == 0 ? round : (round - i + (m - 1)) % (m - 1);
  if (p > q) {
    const int tmp = p;
    p = q;
    q = tmp;
  }
  if (q >= N) return;  // the dummy player (uniform: the whole workgroup leaves)
  const int64_t nw = ldw / VEC, nv = ldv / VEC;
  E* wp = W + (int64_t)p * ldw;
  E* wq = W + (int64_t)q * ldw;
  CH* stash = reinterpret_cast<CH*>(pinv_lds + PINV_RED_BYTES);
  constexpr int HALF = PINV_LDS_BYTES / 2 / (int)sizeof(CH);  // column p's chunks, then column q's
  float a = 0.f, bb = 0.f, gr = 0.f, gi = 0.f;
  for (int64_t v = tid; v < nw; v += PTHREADS) {
    const CH cp = load_chunk<E, VEC>(wp + v * VEC), cq = load_chunk<E, VEC>(wq + v * VEC);
    if constexpr (KEEP) {
      stash[v] = cp;
      stash[HALF + v] = cq;
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      a += elem<E>::abs2(cp.e[e]);
      bb += elem<E>::abs2(cq.e[e]);
      const E g = elem<E>::mulc(cp.e[e], cq.e[e]);  // conj(wp) * wq
      gr += elem<E>::re(g);
      gi += elem<E>::im(g);
    }
  }
  pinv_block_sum4(a, bb, gr, gi, red);
  // |g| and the phase without squaring g; vectors at the null level are left alone (svt.hip has the reasons)
  const float gabs = elem<E>::cplx ? hypotf(gr, gi) : fabsf(gr);
  const float na = sqrtf(a), nb = sqrtf(bb);
  const float null_tol = PINV_NULL * sqrtf(stats[N]);
  if (!(gabs > PINV_TOL * na * nb && na > null_tol && nb > null_tol)) return;  // uniform: every thread holds the same sums
  float er = gr / gabs, ei = gi / gabs;  // e^{i phi}
  const float zeta = (bb - a) / (2.f * gabs);
  const float tt = (zeta >= 0.f ? 1.f : -1.f) / (fabsf(zeta) + sqrtf(1.f + zeta * zeta));
  const float c0 = 1.f / sqrtf(1.f + tt * tt), s0 = c0 * tt;
  // c0^2 + s0^2 misses 1 by an ulp or so, mostly to the same side, and the same (c, s) goes into W and V: one Newton step on
  // the norm, the residual taken by fma (exact where it cancels); the same for the phase's modulus (svt.hip measured the drift)
  const float hn = -0.5f * fmaf(s0, s0, fmaf(c0, c0, -1.f));
  const float c = fmaf(hn, c0, c0), s = fmaf(hn, s0, s0);
  if constexpr (elem<E>::cplx) {
    const float hp = -0.5f * fmaf(ei, ei, fmaf(er, er, -1.f));
    er = fmaf(hp, er, er);
    ei = fmaf(hp, ei, ei);
  }
  const E ph = elem<E>::make(er, ei);
  if (tid == 0) *rotated = 1;
  for (int64_t v = tid; v < nw; v += PTHREADS) {
    CH cp, cq;
    if constexpr (KEEP) {
      cp = stash[v];
      cq = stash[HALF + v];
    } else {
      cp = load_chunk<E, VEC>(wp + v * VEC);
      cq = load_chunk<E, VEC>(wq + v * VEC);
    }
    pinv_rotate<E>(cp, cq, c, s, ph);
    pinv_store<E>(wp + v * VEC, cp);
    pinv_store<E>(wq + v * VEC, cq);
  }
  E* vp = V + (int64_t)p * ldv;
  E* vq = V + (int64_t)q * ldv;
  for (int64_t v = tid; v < nv; v += PTHREADS) {
    CH cp = load_chunk<E, VEC>(vp + v * VEC), cq = load_chunk<E, VEC>(vq + v * VEC);
    pinv_rotate<E>(cp, cq, c, s, ph);
    pinv_store<E>(vp + v * VEC, cp);
    pinv_store<E>(vq + v * VEC, cq);
  }
}

// stats[j] = |w_j|^2: grid N workgroups
template <typename E>
__global__ __launch_bounds__(PTHREADS) void pinv_norms_kernel(const E* __restrict__ W, int64_t ldw, float* __restrict__ stats) {
  __shared__ float red[4 * (PTHREADS / 64)];
  constexpr int VEC = elem<E>::vec;
  const E* w = W + (int64_t)blockIdx.x * ldw;
  float a = 0.f, z0 = 0.f, z1 = 0.f, z2 = 0.f;
  for (int64_t v = threadIdx.x; v < ldw / VEC; v += PTHREADS) {
    const chunk<E, VEC> c = load_chunk<E, VEC>(w + v * VEC);
#pragma unroll
    for (int e = 0; e < VEC; ++e) a += elem<E>::abs2(c.e[e]);
  }
  pinv_block_sum4(a, z0, z1, z2, red);
  if (threadIdx.x == 0) stats[blockIdx.x] = a;
}
// stats[N] = sum_j stats[j]: one workgroup
__global__ __launch_bounds__(PTHREADS) void pinv_fro_kernel(float* __restrict__ stats, int N) {
  __shared__ float red[4 * (PTHREADS / 64)];
  float a = 0.f, z0 = 0.f, z1 = 0.f, z2 = 0.f;
  for (int j = threadIdx.x; j < N; j += PTHREADS) a += stats[j];
  pinv_block_sum4(a, z0, z1, z2, red);
  if (threadIdx.x == 0) stats[N] = a;
}

// t_j = w_j^H b / (sigma_j^2 + lambda), or 0 for a dropped column: one wave per column, grid ceil(N / 4) workgroups.
// Lane l owns the chunks l, l + 64, ... of the column whichever way b is read -- ALIGNED: b in 16-byte loads (its last, partial
// chunk element by element), otherwise element by element -- so both paths add the same terms in the same order: the same bits.
template <typename E, bool ALIGNED>
__global__ __launch_bounds__(PTHREADS) void pinv_wtb_kernel(const E* __restrict__ W, int64_t ldw, int64_t M, int N, const float* __restrict__ stats,
                                                            float lambda, const E* __restrict__ b, E* __restrict__ t) {
  constexpr int VEC = elem<E>::vec;
  const int lane = threadIdx.x & 63, j = blockIdx.x * (PTHREADS / 64) + (threadIdx.x >> 6);
  if (j >= N) return;  // uniform per wave; no barrier below
  const E* w = W + (int64_t)j * ldw;
  E acc = elem<E>::zero();
  for (int64_t v = lane; v < ldw / VEC; v += 64) {
    const chunk<E, VEC> cw = load_chunk<E, VEC>(w + v * VEC);
    chunk<E, VEC> cb;
    if (ALIGNED && (v + 1) * VEC <= M) {
      cb = load_chunk<E, VEC>(b + v * VEC);
    } else {
#pragma unroll
      for (int e = 0; e < VEC; ++e) cb.e[e] = v * VEC + e < M ? b[v * VEC + e] : elem<E>::zero();
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc = elem<E>::fmac(cw.e[e], cb.e[e], acc);
  }
  const float re = wave_sum(elem<E>::re(acc));
  float im = 0.f;
  if constexpr (elem<E>::cplx) im = wave_sum(elem<E>::im(acc));
  if (lane == 0) {
    const float s2 = stats[j], drop2 = PINV_NULL * PINV_NULL * stats[N];
    const float f = s2 > drop2 ? 1.f / (s2 + lambda) : 0.f;  // sigma_j <= 1e-6 |A|_F: dropped (a zero column, too: no 0 / 0)
    t[j] = elem<E>::make(f * re, f * im);
  }
}

// x = proj(V t): workgroup g owns rows [64 g, 64 g + 64), lane = row; wave w adds the columns w, w + 16, ... and the 16
// partial sums are added in wave order.  grid ceil(N / 64) workgroups of 1024 threads.
template <typename E>
__global__ __launch_bounds__(64 * VT_WAVES) void pinv_vt_kernel(const E* __restrict__ V, int64_t ldv, int N, const E* __restrict__ t,
                                                                E* __restrict__ x, int proj) {
  __shared__ E part[VT_WAVES][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t r = (int64_t)blockIdx.x * 64 + lane;
  E acc = elem<E>::zero();
  if (r < N)
    for (int j = w; j < N; j += VT_WAVES) acc = elem<E>::fma(V[r + (int64_t)j * ldv], t[j], acc);
  part[w][lane] = acc;
  __syncthreads();
  if (w != 0 || r >= N) return;
  E sum = part[0][lane];
#pragma unroll
  for (int i = 1; i < VT_WAVES; ++i) sum = elem<E>::add(sum, part[i][lane]);
  x[r] = fista_proj_elem<E>(sum, proj);
}

// rows of the plan's W (V: pass N): the next multiple of a 16-byte chunk
int64_t rls_pinv_padded(int32_t dtype, int64_t n) {
  const int64_t vec = dtype == RLS_C32 ? 2 : 4;
  return (n + vec - 1) / vec * vec;
}
// the largest M whose column pair stays in LDS during a round (tests: one past it takes the re-reading kernel)
int64_t rls_pinv_lds_rows(int32_t dtype) { return PINV_LDS_BYTES / (2 * (int64_t)rls_elem_size(dtype)); }

static int32_t pinv_launch_stats(rls_ctx* ctx, int32_t dtype, int64_t M, int64_t N, const void* W, float* stats) {
  const int64_t ldw = rls_pinv_padded(dtype, M);
  RLS_TRY(rls_with_elem(dtype, [&](auto t) -> int32_t {
    using E = typename decltype(t)::type;
    return rls_launch<pinv_norms_kernel<E>>(ctx, dim3((unsigned)N), dim3(PTHREADS), 0, (const E*)W, ldw, stats);
  }));
  return rls_launch<pinv_fro_kernel>(ctx, dim3(1), dim3(PTHREADS), 0, stats, (int)N);
}

int32_t rls_pinv_launch_load(rls_ctx* ctx, int32_t dtype, int64_t M, int64_t N, const void* A, int64_t lda, void* W, void* V, float* stats) {
  const int64_t ldw = rls_pinv_padded(dtype, M), ldv = rls_pinv_padded(dtype, N);
  RLS_TRY(rls_with_elem(dtype, [&](auto t) -> int32_t {
    using E = typename decltype(t)::type;
    return rls_launch<pinv_load_kernel<E>>(ctx, dim3((unsigned)N), dim3(PTHREADS), 0, (const E*)A, lda, M, N, (E*)W, ldw, (E*)V, ldv);
  }));
  return pinv_launch_stats(ctx, dtype, M, N, W, stats);
}

// one sweep: every round of the tournament, one launch each (N - 1 for even N, N for odd N)
int32_t rls_pinv_launch_sweep(rls_ctx* ctx, int32_t dtype, int64_t M, int64_t N, void* W, void* V, const float* stats, int* rotated) {
  const int64_t ldw = rls_pinv_padded(dtype, M), ldv = rls_pinv_padded(dtype, N);
  const int m = (int)(N + (N & 1));
  const bool keep = M <= rls_pinv_lds_rows(dtype);
  // (the same size for every launch of an instantiation, whatever M: rls_allow_lds sets the kernel's limit once)
  const size_t lds = PINV_RED_BYTES + (keep ? PINV_LDS_BYTES : 0);
  return rls_with_elem(dtype, [&](auto t) -> int32_t {
    using E = typename decltype(t)::type;
    return with_bool(keep, [&](auto KEEP) -> int32_t {
      for (int round = 0; round < m - 1; ++round)
        RLS_TRY((rls_launch<pinv_round_kernel<E, KEEP>>(ctx, dim3(m / 2), dim3(PTHREADS), lds, (E*)W, ldw, (E*)V, ldv, (int)N, round, stats, rotated)));
      return 0;
    });
  });
}

int32_t rls_pinv_launch_finish(rls_ctx* ctx, int32_t dtype, int64_t M, int64_t N, const void* W, float* stats) {
  return pinv_launch_stats(ctx, dtype, M, N, W, stats);
}

// one column: t = diag(1 / (sigma^2 + lambda)) W^H b (dropped columns: 0), x = proj(V t)
int32_t rls_pinv_launch_solve(rls_ctx* ctx, int32_t dtype, int64_t M, int64_t N, const void* W, const void* V, const float* stats, float lambda,
                              const void* b, void* t, void* x, int proj) {
  const int64_t ldw = rls_pinv_padded(dtype, M), ldv = rls_pinv_padded(dtype, N);
  const bool aligned = ((uintptr_t)b & 15) == 0;
  constexpr int per = PTHREADS / 64;
  return rls_with_elem(dtype, [&](auto ty) -> int32_t {
    using E = typename decltype(ty)::type;
    RLS_TRY(with_bool(aligned, [&](auto AL) -> int32_t {
      return rls_launch<pinv_wtb_kernel<E, AL>>(ctx, dim3((unsigned)((N + per - 1) / per)), dim3(PTHREADS), 0, (const E*)W, ldw, M, (int)N, stats,
                                                lambda, (const E*)b, (E*)t);
    }));
    return rls_launch<pinv_vt_kernel<E>>(ctx, dim3((unsigned)((N + 63) / 64)), dim3(64 * VT_WAVES), 0, (const E*)V, ldv, (int)N, (const E*)t,
                                         (E*)x, proj);
  });
}
