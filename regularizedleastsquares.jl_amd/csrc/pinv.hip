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

// ---------------------------------------------------------------------------------------------
// Phase 1: blocked sweeps on the matrix cores.  The columns are cut into blocks of B (16 or 32); the blocks play
// the tournament the columns play above (a dummy block for an odd count), and a round is three launches over its block pairs:
//   pinv_block_gram_kernel   G = X^H X of the pair's 2B columns X = [W_P W_Q] on v_mfma_f32_16x16x4_f32, the rows split over
//                            `nslots` slots per pair; every slot writes its partial G to plan scratch.
//   pinv_block_diag_kernel   one workgroup per pair: adds the partials in slot order, diagonalises G in LDS by a cyclic TWO-SIDED
//                            Jacobi (G <- J^H G J; a singular G -- pad, null or repeated columns -- needs no care: such columns
//                            are not rotated, or rotate like any other pair) with the rotation of pinv_round_kernel, and
//                            accumulates the unitary Q.  A pair that rotated stores 1 into the sweep word and into its own flag.
//   pinv_block_apply_kernel  X <- X Q on the W pair and on the V pair, 16-row tiles on the matrix cores; a wave holds its rows of
//                            all 2B columns in registers before it stores any.  Pairs whose flag is 0 are left alone.
// Columns past N of a ragged last block are read as zeros and never stored; their rows and columns of G are exactly zero, so
// they sit at the null level and Q is the identity on them.  Every sum runs in a fixed order; no atomics.
// ---------------------------------------------------------------------------------------------
typedef float pinv_f32x4 __attribute__((ext_vector_type(4)));
__device__ static inline pinv_f32x4 pinv_mfma(float a, float b, pinv_f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

constexpr int PINV_BLOCK_INNER = 10;      // cap of the cyclic sweeps over G in pinv_block_diag_kernel
constexpr int PINV_APPLY_SUB = 4;         // 16-row tiles a wave of pinv_block_apply_kernel walks: 256 rows per workgroup
constexpr int PINV_GRAM_WGS = 512;        // workgroups a Gram launch aims for (two per CU)
constexpr int PINV_GRAM_SPLIT_MAX = 32;   // row splits (workgroups) per block pair, at most

// the block pair i of round `round` on nb blocks; false for the pair that holds the dummy block
__device__ static inline bool pinv_block_pair(int nb, int round, int i, int& P, int& Q) {
  const int m = nb + (nb & 1);
  const int p = i == 0 ? m - 1 : (round + i) % (m - 1);
  const int q = i == 0 ? round : (round - i + (m - 1)) % (m - 1);
  P = p < q ? p : q;
  Q = p < q ? q : p;
  return Q < nb;
}
// column of W / V behind local column j of the pair
template <int B>
__device__ static inline int pinv_block_col(int P, int Q, int j) {
  return j < B ? P * B + j : Q * B + (j - B);
}

// grid (S, pairs); the workgroup's 4 waves are 4 / T row sub-splits x T tile rows (T = 2B / 16): wave w adds, over the 16-row
// steps of its slot, the tiles (ti, 0..T-1) of G.  Lane l holds rows 4 (l >> 4) .. + 3 of column l & 15 of a column block -- one
// register layout for both MFMA operands (gram_mfma_kernel, skinny.hip).  part: [pair][slot][2B x 2B, column-major].
template <typename E, int B>
__global__ __launch_bounds__(PTHREADS) void pinv_block_gram_kernel(const E* __restrict__ W, int64_t ldw, int N, int nb, int round, int nslots,
                                                                   E* __restrict__ part) {
  constexpr bool CX = elem<E>::cplx;
  constexpr int n = 2 * B, T = n / 16, NSUB = 4 / T;
  int P, Q;
  if (!pinv_block_pair(nb, round, blockIdx.y, P, Q)) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int ti = w % T, slot = (int)blockIdx.x * NSUB + w / T;
  const int64_t steps = (ldw + 15) / 16, per = (steps + nslots - 1) / nslots;
  const int64_t s0 = slot * per, s1 = s0 + per < steps ? s0 + per : steps;
  const E* col[T];
  bool okc[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int c = pinv_block_col<B>(P, Q, 16 * t + (lane & 15));
    okc[t] = c < N;
    col[t] = W + (int64_t)(okc[t] ? c : 0) * ldw + 4 * (lane >> 4);
  }
  pinv_f32x4 acc[T][4];
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[t][k] = pinv_f32x4{0.f, 0.f, 0.f, 0.f};
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t st = s0; st < s1; ++st) {
    const int64_t r = 16 * st + 4 * (lane >> 4);  // ldw is a multiple of the 16-byte chunk: a chunk is inside the column or past it
    float4 x0[T], x1[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const float4* ap = reinterpret_cast<const float4*>(col[t] + 16 * st);
      x0[t] = okc[t] && r < ldw ? ap[0] : z4;
      x1[t] = z4;
      if constexpr (CX) x1[t] = okc[t] && r + 2 < ldw ? ap[1] : z4;
    }
    float4 a0 = x0[0], a1 = x1[0];
#pragma unroll
    for (int t = 1; t < T; ++t) {
      if (t == ti) {
        a0 = x0[t];
        a1 = x1[t];
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
      for (int t = 0; t < T; ++t) {
        if constexpr (CX) {
          const float4 ia = k < 2 ? a0 : a1, jb = k < 2 ? x0[t] : x1[t];
          const float ar = (k & 1) ? ia.z : ia.x, ai = (k & 1) ? ia.w : ia.y;
          const float br = (k & 1) ? jb.z : jb.x, bi = (k & 1) ? jb.w : jb.y;
          acc[t][0] = pinv_mfma(ar, br, acc[t][0]);
          acc[t][1] = pinv_mfma(ai, bi, acc[t][1]);
          acc[t][2] = pinv_mfma(ar, bi, acc[t][2]);
          acc[t][3] = pinv_mfma(ai, br, acc[t][3]);
        } else {
          const float ia[4] = {a0.x, a0.y, a0.z, a0.w};
          const float jb[4] = {x0[t].x, x0[t].y, x0[t].z, x0[t].w};
          acc[t][k & 1] = pinv_mfma(ia[k], jb[k], acc[t][k & 1]);
        }
      }
    }
  }
  // accumulator register u of lane (q = l >> 4, j = l & 15) is entry (16 ti + 4 q + u, 16 t + j) of G = conj(X)^T X
  E* out = part + ((int64_t)blockIdx.y * nslots + slot) * (n * n);
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const pinv_f32x4 gre = acc[t][0] + acc[t][1], gim = acc[t][2] - acc[t][3];
#pragma unroll
    for (int u = 0; u < 4; ++u) out[(16 * ti + 4 * (lane >> 4) + u) + (16 * t + (lane & 15)) * n] = elem<E>::make(gre[u], gim[u]);
  }
}

// (c, s, e^{i phi}) of the pair with a = g_pp, b = g_qq, g = g_pq, exactly as pinv_round_kernel forms them; false: no rotation
template <typename E>
__device__ static inline bool pinv_rotation(float a, float bb, float gr, float gi, float tol, float null_tol, float& c, float& s, float& er,
                                            float& ei) {
  const float gabs = elem<E>::cplx ? hypotf(gr, gi) : fabsf(gr);
  const float na = sqrtf(a), nb = sqrtf(bb);
  if (!(gabs > tol * na * nb && na > null_tol && nb > null_tol)) return false;
  er = gr / gabs;
  ei = gi / gabs;
  const float zeta = (bb - a) / (2.f * gabs);
  const float tt = (zeta >= 0.f ? 1.f : -1.f) / (fabsf(zeta) + sqrtf(1.f + zeta * zeta));
  const float c0 = 1.f / sqrtf(1.f + tt * tt), s0 = c0 * tt;
  const float hn = -0.5f * fmaf(s0, s0, fmaf(c0, c0, -1.f));
  c = fmaf(hn, c0, c0);
  s = fmaf(hn, s0, s0);
  if constexpr (elem<E>::cplx) {
    const float hp = -0.5f * fmaf(ei, ei, fmaf(er, er, -1.f));
    er = fmaf(hp, er, er);
    ei = fmaf(hp, ei, ei);
  }
  return true;
}

// grid: pairs workgroups.  LDS: G and Q (2B x 2B each, column-major), the round's rotations, the sweep's flag.  A round of the
// inner tournament (2B players, B disjoint pairs) is three steps between barriers: the B rotations from (g_pp, g_qq, g_pq); the
// column step G <- G J, Q <- Q J; the row step G <- J^H G.  stats[N] = |A|_F^2 (the null level).
template <typename E, int B>
__global__ __launch_bounds__(PTHREADS) void pinv_block_diag_kernel(const E* __restrict__ part, int N, int nb, int round, int nslots, float tol,
                                                                   const float* __restrict__ stats, E* __restrict__ Qbuf, int* __restrict__ flags,
                                                                   int* __restrict__ rotated) {
  extern __shared__ __align__(16) unsigned char pinv_lds[];
  constexpr int n = 2 * B;
  E* G = reinterpret_cast<E*>(pinv_lds);
  E* Qm = G + n * n;
  float4* rot = reinterpret_cast<float4*>(Qm + n * n);  // (c, s, re e^{i phi}, im e^{i phi}); c = 2: the pair does not rotate
  int* any = reinterpret_cast<int*>(rot + B);           // [0]: this inner sweep rotated, [1]: some sweep did
  int P, Q;
  if (!pinv_block_pair(nb, round, blockIdx.x, P, Q)) return;
  const int tid = threadIdx.x;
  const E* src = part + (int64_t)blockIdx.x * nslots * (n * n);
  for (int idx = tid; idx < n * n; idx += PTHREADS) {
    E g = src[idx];
    for (int sl = 1; sl < nslots; ++sl) g = elem<E>::add(g, src[(int64_t)sl * (n * n) + idx]);
    G[idx] = g;
    Qm[idx] = (idx % n == idx / n) ? elem<E>::make(1.f, 0.f) : elem<E>::zero();
  }
  if (tid == 0) any[1] = 0;
  const float null_tol = PINV_NULL * sqrtf(stats[N]);
  for (int sweep = 0; sweep < PINV_BLOCK_INNER; ++sweep) {
    __syncthreads();
    if (tid == 0) any[0] = 0;
    __syncthreads();
    for (int r = 0; r < n - 1; ++r) {
      if (tid < B) {
        const int i = tid;
        const int a0 = i == 0 ? n - 1 : (r + i) % (n - 1), b0 = i == 0 ? r : (r - i + (n - 1)) % (n - 1);
        const int p = a0 < b0 ? a0 : b0, q = a0 < b0 ? b0 : a0;
        const E g = G[p + q * n];
        float c, s, er, ei;
        if (pinv_rotation<E>(elem<E>::re(G[p + p * n]), elem<E>::re(G[q + q * n]), elem<E>::re(g), elem<E>::im(g), tol, null_tol, c, s, er, ei)) {
          rot[i] = make_float4(c, s, er, ei);
          any[0] = 1;  // (every writer writes the same value)
          any[1] = 1;
        } else {
          rot[i] = make_float4(2.f, 0.f, 1.f, 0.f);
        }
      }
      __syncthreads();
      for (int it = tid; it < B * n; it += PTHREADS) {  // columns: (x_p, x_q) <- (c x_p - s conj(ph) x_q, s x_p + c conj(ph) x_q)
        const int i = it / n, row = it % n;
        const float4 R = rot[i];
        if (R.x > 1.5f) continue;
        const int a0 = i == 0 ? n - 1 : (r + i) % (n - 1), b0 = i == 0 ? r : (r - i + (n - 1)) % (n - 1);
        const int p = a0 < b0 ? a0 : b0, q = a0 < b0 ? b0 : a0;
        const E ph = elem<E>::make(R.z, R.w);
#pragma unroll
        for (int which = 0; which < 2; ++which) {
          E* X = which ? Qm : G;
          const E xp = X[row + p * n], qt = elem<E>::mulc(ph, X[row + q * n]);
          X[row + p * n] = elem<E>::sub(elem<E>::scale(R.x, xp), elem<E>::scale(R.y, qt));
          X[row + q * n] = elem<E>::add(elem<E>::scale(R.y, xp), elem<E>::scale(R.x, qt));
        }
      }
      __syncthreads();
      for (int it = tid; it < B * n; it += PTHREADS) {  // rows of G: (g_p, g_q) <- (c g_p - s ph g_q, s g_p + c ph g_q)
        const int i = it / n, colj = it % n;
        const float4 R = rot[i];
        if (R.x > 1.5f) continue;
        const int a0 = i == 0 ? n - 1 : (r + i) % (n - 1), b0 = i == 0 ? r : (r - i + (n - 1)) % (n - 1);
        const int p = a0 < b0 ? a0 : b0, q = a0 < b0 ? b0 : a0;
        const E ph = elem<E>::make(R.z, R.w);
        const E gp = G[p + colj * n], qt = elem<E>::mul(ph, G[q + colj * n]);
        G[p + colj * n] = elem<E>::sub(elem<E>::scale(R.x, gp), elem<E>::scale(R.y, qt));
        G[q + colj * n] = elem<E>::add(elem<E>::scale(R.y, gp), elem<E>::scale(R.x, qt));
      }
      __syncthreads();
    }
    if (any[0] == 0) break;  // uniform: read behind the round's last barrier, written next behind the barrier at the loop's top
  }
  const int did = any[1];
  if (did) {
    E* dst = Qbuf + (int64_t)blockIdx.x * (n * n);
    for (int idx = tid; idx < n * n; idx += PTHREADS) dst[idx] = Qm[idx];
  }
  if (tid == 0) {
    flags[blockIdx.x] = did;
    if (did) *rotated = 1;
  }
}

// grid (tiles of W + tiles of V, pairs): a workgroup owns 64 PINV_APPLY_SUB rows of the pair's 2B columns of W or of V, a wave 16
// of them at a time.  Lane l holds X[16-row tile][row l & 15][column 4 kb + (l >> 4)] (the MFMA A operand); Q sits in LDS as two
// planes, k-major and padded (the B operand: Q[4 kb + (l >> 4)][16 t + (l & 15)]).
template <typename E, int B>
__global__ __launch_bounds__(PTHREADS) void pinv_block_apply_kernel(E* W, int64_t ldw, E* V, int64_t ldv, int N, int nb, int round, int tiles_w,
                                                                    const E* __restrict__ Qbuf, const int* __restrict__ flags) {
  constexpr bool CX = elem<E>::cplx;
  constexpr int n = 2 * B, T = n / 16, KB = n / 4, LDQ = n + 16;
  __shared__ float qre[n * LDQ];
  __shared__ float qim[CX ? n * LDQ : 1];
  int P, Q;
  if (!pinv_block_pair(nb, round, blockIdx.y, P, Q)) return;
  if (flags[blockIdx.y] == 0) return;  // the pair rotated nothing: Q = I, and W, V keep their bits
  const bool isw = (int)blockIdx.x < tiles_w;
  E* X = isw ? W : V;
  const int64_t ld = isw ? ldw : ldv;
  const int64_t row0 = (int64_t)(isw ? blockIdx.x : blockIdx.x - tiles_w) * (64 * PINV_APPLY_SUB);
  const E* qsrc = Qbuf + (int64_t)blockIdx.y * (n * n);
  for (int idx = threadIdx.x; idx < n * n; idx += PTHREADS) {  // Q[k + j n] -> plane[k LDQ + j]
    const E q = qsrc[idx];
    const int k = idx % n, j = idx / n;
    qre[k * LDQ + j] = elem<E>::re(q);
    if constexpr (CX) qim[k * LDQ + j] = elem<E>::im(q);
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int sub = 0; sub < PINV_APPLY_SUB; ++sub) {
    const int64_t r0 = row0 + 16 * (w * PINV_APPLY_SUB + sub);
    if (r0 >= ld) break;  // uniform per wave; no barrier below
    E xs[KB];
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      const int c = pinv_block_col<B>(P, Q, 4 * kb + (lane >> 4));
      const int64_t r = r0 + (lane & 15);
      xs[kb] = (c < N && r < ld) ? X[r + (int64_t)c * ld] : elem<E>::zero();
    }
    pinv_f32x4 acc[T][4];
#pragma unroll
    for (int t = 0; t < T; ++t) {
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[t][k] = pinv_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) {
        const int qi = (4 * kb + (lane >> 4)) * LDQ + 16 * t + (lane & 15);
        if constexpr (CX) {
          const float xr = xs[kb].x, xi = xs[kb].y, qr = qre[qi], qm = qim[qi];
          acc[t][0] = pinv_mfma(xr, qr, acc[t][0]);
          acc[t][1] = pinv_mfma(xi, qm, acc[t][1]);
          acc[t][2] = pinv_mfma(xr, qm, acc[t][2]);
          acc[t][3] = pinv_mfma(xi, qr, acc[t][3]);
        } else {
          acc[t][kb & 1] = pinv_mfma(xs[kb], qre[qi], acc[t][kb & 1]);
        }
      }
    }
    // every load of the tile is behind us (xs); accumulator register u of lane (q = l >> 4, j = l & 15) is (row 4 q + u, column 16 t + j)
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const int c = pinv_block_col<B>(P, Q, 16 * t + (lane & 15));
      const int64_t r = r0 + 4 * (lane >> 4);
      if (c >= N) continue;
      E* dst = X + r + (int64_t)c * ld;
      if constexpr (CX) {
        const pinv_f32x4 yr = acc[t][0] - acc[t][1], yi = acc[t][2] + acc[t][3];
        if (r < ld) *reinterpret_cast<f4*>(dst) = f4{yr[0], yi[0], yr[1], yi[1]};
        if (r + 2 < ld) *reinterpret_cast<f4*>(dst + 2) = f4{yr[2], yi[2], yr[3], yi[3]};
      } else {
        const pinv_f32x4 y = acc[t][0] + acc[t][1];
        if (r < ld) *reinterpret_cast<f4*>(dst) = f4{y[0], y[1], y[2], y[3]};
      }
    }
  }
}

// slots per block pair of the Gram launch: enough workgroups to fill the chip, at least two 16-row steps per slot where M allows
static int pinv_block_slots(int32_t dtype, int64_t M, int64_t N, int block) {
  const int64_t nb = (N + block - 1) / block, pairs = (nb + (nb & 1)) / 2;
  const int nsub = 4 / (2 * block / 16);
  const int64_t steps = (rls_pinv_padded(dtype, M) + 15) / 16;
  int64_t S = (PINV_GRAM_WGS + pairs - 1) / pairs;
  if (S > PINV_GRAM_SPLIT_MAX) S = PINV_GRAM_SPLIT_MAX;
  if (S > steps / (2 * nsub)) S = steps / (2 * nsub);
  if (S < 1) S = 1;
  return (int)S * nsub;
}

// plan scratch of the blocked phase: the Gram partials [pairs][slots][2B x 2B], Q [pairs][2B x 2B], the pairs' flags
size_t rls_pinv_block_scratch_bytes(int32_t dtype, int64_t M, int64_t N, int block) {
  const size_t nb = (size_t)((N + block - 1) / block), pairs = (nb + (nb & 1)) / 2, nn = (size_t)4 * block * block;
  return pairs * ((size_t)pinv_block_slots(dtype, M, N, block) + 1) * nn * rls_elem_size(dtype) + pairs * sizeof(int);
}

// one blocked sweep: every round of the block tournament, three launches each; returns the rounds launched in *rounds
int32_t rls_pinv_launch_block_sweep(rls_ctx* ctx, int32_t dtype, int64_t M, int64_t N, int block, float tol, void* W, void* V, const float* stats,
                                    void* scratch, int* rotated, int* rounds) {
  const int64_t ldw = rls_pinv_padded(dtype, M), ldv = rls_pinv_padded(dtype, N);
  const int nb = (int)((N + block - 1) / block), mb = nb + (nb & 1), pairs = mb / 2;
  const int nslots = pinv_block_slots(dtype, M, N, block);
  const int per_wg = 64 * PINV_APPLY_SUB;
  const int tiles_w = (int)((ldw + per_wg - 1) / per_wg), tiles_v = (int)((ldv + per_wg - 1) / per_wg);
  return rls_with_elem(dtype, [&](auto t) -> int32_t {
    using E = typename decltype(t)::type;
    return rls_with<16, 32>(block, [&](auto BW) -> int32_t {
      constexpr int B = decltype(BW)::value, n = 2 * B, nsub = 4 / (n / 16);
      E* part = (E*)scratch;
      E* Qbuf = part + (size_t)pairs * nslots * n * n;
      int* flags = (int*)(Qbuf + (size_t)pairs * n * n);
      const size_t lds = 2 * n * n * sizeof(E) + B * sizeof(float4) + 16;
      for (int round = 0; round < mb - 1; ++round) {
        RLS_TRY((rls_launch<pinv_block_gram_kernel<E, B>>(ctx, dim3(nslots / nsub, pairs), dim3(PTHREADS), 0, (const E*)W, ldw, (int)N, nb, round,
                                                          nslots, part)));
        RLS_TRY((rls_launch<pinv_block_diag_kernel<E, B>>(ctx, dim3(pairs), dim3(PTHREADS), lds, (const E*)part, (int)N, nb, round, nslots, tol,
                                                          stats, Qbuf, flags, rotated)));
        RLS_TRY((rls_launch<pinv_block_apply_kernel<E, B>>(ctx, dim3(tiles_w + tiles_v, pairs), dim3(PTHREADS), 0, (E*)W, ldw, (E*)V, ldv, (int)N, nb,
                                                           round, tiles_w, (const E*)Qbuf, (const int*)flags)));
      }
      *rounds = mb - 1;
      return 0;
    });
  });
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
