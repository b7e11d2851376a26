// DirectSolver (src/Direct.jl:17-67): x = (A^H A + lambda I) \ A^H b by a blocked Cholesky factorisation on the device.
//
// The factor lives in a PADDED square matrix W of NB x NB blocks of 64 x 64 (NB = ceil(N / 64), leading dimension 64 NB);
// the padding carries the identity, so [G + lambda I, 0; 0, I] = [L, 0; 0, I] [L, 0; 0, I]^H and no kernel has a partial
// tile.  The factored DIAGONAL blocks L_jj go to a buffer of their own behind W (NB tiles of 64 x 64): every workgroup of a
// panel launch reads the unfactored diagonal block from W, so nothing in that launch may write it.  The rule for every
// kernel here: no workgroup reads a word that another workgroup of the same launch writes.
// Right-looking on the lower triangle, one block column j after the other:
//   chol_panel_kernel   every workgroup owns one 64-row strip below the diagonal block.  It factors the diagonal block in LDS
//                       for itself (the same operations in the same order in every workgroup: the same bits) and carries
//                       its strip through the same 64 elimination steps, which is L21 = A21 L11^-H.  Workgroup 0 stores L11
//                       into the diagonal buffer; W's diagonal block stays as the launch found it.
//   chol_trail_kernel   A22 -= L21 L21^H on the lower-triangle tiles, v_mfma_f32_16x16x4_f32 (exact f32 FMA chains); the
//                       contraction length is 64, so one workgroup finishes a tile.  ComplexF32: the operands are split
//                       into their (re | im) parts, four real products per complex one (as skinny.hip does).
// 2 NB launches per factorisation (1 load + NB panels + NB - 1 trailing updates).
//
// A pivot that is not strictly positive and finite stops the factorisation: workgroup 0 of that panel stores the 1-based
// column in the plan's device word `info`, and every later kernel (of the factorisation and of the solves) reads the word
// at entry and returns.  Nothing waits, nothing is read back; rls_direct_get_status reports the column.
//
// The triangular solves of K right-hand sides (16 columns per workgroup, blockIdx.y) run one launch per block:
//   chol_trsm_kernel    every workgroup solves the 64 x 64 diagonal block for its 16 columns in LDS (redundantly, as the
//                       panel kernel does); workgroup 0 writes the solved block, workgroup r > 0 subtracts the block's
//                       contribution from ITS row block below (forward, L Y = X) or above (backward, L^H X = Y).
// The forward pass reads X and writes the solved blocks to the plan's workspace, the backward pass goes the other way, so no
// workgroup reads a block another one of the same launch writes.  The projection (RLS_PROJ_*) rides on the backward pass's
// store.  2 NB launches per solve, behind the K products A^H b (a Gram-only
// operator: behind chol_copy_kernel, X = B).
//
// Every sum runs in a fixed order: two runs give the same bits.  No atomics, no grid-wide synchronisation.
#include "rls_common.hpp"

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int DB = 64;         // block size
constexpr int DTHREADS = 256;  // four waves: thread t works on row t & 63 of a tile and on every fourth column from t >> 6
constexpr int DCOLS = 16;      // right-hand sides per workgroup of the triangular solves
constexpr int DLDT = DB + 1;   // leading dimension of the solves' LDS tile (read along either index without bank conflicts)

template <typename E>
__device__ static inline E conj_e(E v) {
  return elem<E>::make(elem<E>::re(v), -elem<E>::im(v));
}
// c - a b
template <typename E>
__device__ static inline E msub_e(E a, E b, E c) {
  return elem<E>::sub(c, elem<E>::mul(a, b));
}

// W = [G + lambda I, 0; 0, I], lower-triangle tiles only (nothing reads the others); resets the pivot word
template <typename E>
__global__ __launch_bounds__(DTHREADS) void chol_load_kernel(const E* __restrict__ G, int64_t ldg, int64_t N, float lambda,
                                                             E* __restrict__ W, int64_t ld, int* info) {
  const int p = blockIdx.x, q = blockIdx.y;
  if (p == 0 && q == 0 && threadIdx.x == 0) *info = 0;
  if (q > p) return;
  const int i = threadIdx.x & 63, cg = threadIdx.x >> 6;
  const int64_t R = (int64_t)p * DB + i;
  for (int c = cg; c < DB; c += 4) {
    const int64_t Cc = (int64_t)q * DB + c;
    E v = elem<E>::zero();
    if (R < N && Cc < N) {
      if (R > Cc) v = G[R + Cc * ldg];
      else if (R == Cc) v = elem<E>::make(elem<E>::re(G[R + Cc * ldg]) + lambda, 0.f);
    } else if (R == Cc) {
      v = elem<E>::make(1.f, 0.f);
    }
    W[R + Cc * ld] = v;
  }
}

// block column j: grid = max(1, NB - 1 - j) workgroups; dynamic LDS: two 64 x 64 tiles.  Ld: the diagonal buffer's tile j
template <typename E>
__global__ __launch_bounds__(DTHREADS) void chol_panel_kernel(E* __restrict__ W, int64_t ld, int nb, int j, E* __restrict__ Ld, int* info) {
  extern __shared__ __align__(16) unsigned char direct_lds[];
  E* D = reinterpret_cast<E*>(direct_lds);  // the diagonal block, column-major
  E* S = D + DB * DB;                       // this workgroup's strip
  if (*info != 0) return;
  const int t = threadIdx.x, i = t & 63, cg = t >> 6;
  const bool strip = j + 1 < nb;
  const int64_t d0 = (int64_t)j * DB, s0 = d0 + (int64_t)DB * (1 + blockIdx.x);
  for (int c = cg; c < DB; c += 4) {
    D[i + DB * c] = W[(d0 + i) + (d0 + c) * ld];
    if (strip) S[i + DB * c] = W[(s0 + i) + (d0 + c) * ld];
  }
  __syncthreads();
  int bad = 0;
  // the diagonal keeps the PIVOTS (not their roots) inside the loop, so that a step's pivot is read and never rewritten
  for (int k = 0; k < DB; ++k) {
    const float d = elem<E>::re(D[k + DB * k]);  // the same LDS word in every thread: the branch is uniform
    if (!(d > 0.f && d <= 3.4028235e38f)) {
      bad = k + 1;
      break;
    }
    const float rs = 1.0f / sqrtf(d);
    if (cg == 0 && i > k) D[i + DB * k] = elem<E>::scale(rs, D[i + DB * k]);
    if (cg == 1 && strip) S[i + DB * k] = elem<E>::scale(rs, S[i + DB * k]);
    __syncthreads();
    for (int c = k + 1 + cg; c < DB; c += 4) {
      const E lc = conj_e(D[c + DB * k]);
      if (i >= c) D[i + DB * c] = msub_e(D[i + DB * k], lc, D[i + DB * c]);
      if (strip) S[i + DB * c] = msub_e(S[i + DB * k], lc, S[i + DB * c]);
    }
    __syncthreads();
  }
  if (bad) {
    if (blockIdx.x == 0 && t == 0) *info = (int)(d0 + bad);
    return;
  }
  for (int c = cg; c < DB; c += 4) {
    if (blockIdx.x == 0) {
      E v = elem<E>::zero();
      if (i > c) v = D[i + DB * c];
      else if (i == c) v = elem<E>::make(sqrtf(elem<E>::re(D[i + DB * c])), 0.f);
      Ld[i + DB * c] = v;
    }
    if (strip) W[(s0 + i) + (d0 + c) * ld] = S[i + DB * c];
  }
}

__device__ static inline f32x4 direct_mfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// tile (p, q), q <= p, of the trailing matrix behind block column j: C -= P Q^H with P = L[j+1+p, j], Q = L[j+1+q, j].
// Wave w owns rows [16 w, 16 w + 16) of the tile: four 16 x 16 accumulators (eight for complex), 16 MFMA steps of k = 4.
// Operand lane maps: A[l & 15][k = l >> 4], B[k = l >> 4][l & 15]; result column l & 15, rows 4 (l >> 4) + reg.
template <typename E>
__global__ __launch_bounds__(DTHREADS) void chol_trail_kernel(E* __restrict__ W, int64_t ld, int j, const int* info) {
  const int p = blockIdx.x, q = blockIdx.y;
  if (q > p) return;
  if (*info != 0) return;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
  const int64_t k0 = (int64_t)j * DB, r0 = k0 + (int64_t)DB * (1 + p), c0 = k0 + (int64_t)DB * (1 + q);
  const E* P = W + (r0 + 16 * w + li) + (k0 + lk) * ld;
  E a[16];
#pragma unroll
  for (int kk = 0; kk < 16; ++kk) a[kk] = P[(int64_t)(4 * kk) * ld];
#pragma unroll
  for (int sj = 0; sj < 4; ++sj) {
    const E* Q = W + (c0 + 16 * sj + li) + (k0 + lk) * ld;
    E* C = W + (r0 + 16 * w + 4 * lk) + (c0 + 16 * sj + li) * ld;
    E b[16];
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) b[kk] = Q[(int64_t)(4 * kk) * ld];
    if constexpr (elem<E>::cplx) {
      f32x4 cr, ci;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const E v = C[g];
        cr[g] = v.x;
        ci[g] = v.y;
      }
      // P conj(Q) = (pr qr + pi qi) + i (pi qr - pr qi)
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) {
        cr = direct_mfma(-a[kk].x, b[kk].x, cr);
        ci = direct_mfma(-a[kk].y, b[kk].x, ci);
        cr = direct_mfma(-a[kk].y, b[kk].y, cr);
        ci = direct_mfma(a[kk].x, b[kk].y, ci);
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) C[g] = make_float2(cr[g], ci[g]);
    } else {
      f32x4 acc;
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[g] = C[g];
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) acc = direct_mfma(-a[kk], b[kk], acc);
#pragma unroll
      for (int g = 0; g < 4; ++g) C[g] = acc[g];
    }
  }
}

// One block step of a triangular solve for the 16 columns from 16 blockIdx.y.
//   BACK = false (L Y = X):   block j; grid.x = NB - j;  workgroup r > 0 owns row block j + r
//   BACK = true  (L^H X = Y): block j; grid.x = j + 1;   workgroup r > 0 owns row block j - r
// `src` holds the right-hand side (rows < nsrc exist, the others read as zero) and is updated in place by the workgroups
// r > 0; workgroup 0 stores the solved block into `dst` (rows < ndst), through the projection `proj`.
template <typename E, bool BACK>
__global__ __launch_bounds__(DTHREADS) void chol_trsm_kernel(const E* __restrict__ L, int64_t ld, int j, int K, E* src, int64_t ldsrc,
                                                             int64_t nsrc, E* dst, int64_t lddst, int64_t ndst, int proj, const int* info) {
  __shared__ E T[DB * DLDT];
  __shared__ E Y[DB * DCOLS];
  if (*info != 0) return;
  const int t = threadIdx.x, i = t & 63, cg = t >> 6;
  const int col0 = blockIdx.y * DCOLS;
  const int kc = min(DCOLS, K - col0);
  const int64_t d0 = (int64_t)j * DB;
  const E* Ljj = L + ld * ld + (int64_t)j * DB * DB;  // the factored diagonal block: the buffer behind W, tile j
  for (int c = cg; c < DB; c += 4) T[i + DLDT * c] = Ljj[i + DB * c];
  for (int c = cg; c < DCOLS; c += 4)
    Y[i + DB * c] = (c < kc && d0 + i < nsrc) ? src[(d0 + i) + (int64_t)(col0 + c) * ldsrc] : elem<E>::zero();
  __syncthreads();
  // substitution.  Column c of Y belongs to ONE wave (its 64 rows are that wave's lanes, c = cg mod 4), and T is read-only here:
  // lane k rewrites Y[k] in the step in which its wave's other lanes read it, which is right because every lane has loaded yk
  // before the branch and a wave issues its LDS operations in program order.  So the algorithm needs no workgroup barrier in
  // this loop; the one per step is a conservative guard that does not rest on that lockstep, kept until it is measured away.
  for (int s = 0; s < DB; ++s) {
    const int k = BACK ? DB - 1 - s : s;
    const float rd = 1.0f / elem<E>::re(T[k + DLDT * k]);
    const bool mine = BACK ? i < k : i > k;
    E l = elem<E>::zero();
    if (mine) l = BACK ? conj_e(T[k + DLDT * i]) : T[i + DLDT * k];
    for (int c = cg; c < DCOLS; c += 4) {
      const E yk = elem<E>::scale(rd, Y[k + DB * c]);
      if (mine) Y[i + DB * c] = msub_e(l, yk, Y[i + DB * c]);
      else if (i == k) Y[k + DB * c] = yk;
    }
    __syncthreads();
  }
  const int r = blockIdx.x;
  if (r == 0) {
    for (int c = cg; c < kc; c += 4)
      if (d0 + i < ndst) dst[(d0 + i) + (int64_t)(col0 + c) * lddst] = BACK ? fista_proj_elem<E>(Y[i + DB * c], proj) : Y[i + DB * c];
    return;
  }
  // the coupling tile into T (the diagonal block is no longer needed), stored so that thread i reads along its own index:
  //   forward  T[i + DLDT k] = L[b0 + i, d0 + k];   backward  T[i + DLDT k] = conj(L[d0 + k, b0 + i])
  const int64_t b0 = BACK ? d0 - (int64_t)DB * r : d0 + (int64_t)DB * r;
  for (int c = cg; c < DB; c += 4) {
    if (BACK) T[c + DLDT * i] = conj_e(L[(d0 + i) + (b0 + c) * ld]);
    else T[i + DLDT * c] = L[(b0 + i) + (d0 + c) * ld];
  }
  __syncthreads();
  if (b0 + i >= nsrc) return;
  for (int c = cg; c < kc; c += 4) {
    E* x = src + (b0 + i) + (int64_t)(col0 + c) * ldsrc;
    E acc = *x;
    for (int k = 0; k < DB; ++k) acc = msub_e(T[i + DLDT * k], Y[k + DB * c], acc);
    *x = acc;
  }
}

// X = B, one workgroup per column: the right-hand sides of a Gram-only operator (B is A^H b already).  A kernel and not a copy of
// the runtime's, so that it reads the pivot word like every other one: after a failed factorisation X is not written.
template <typename E>
__global__ __launch_bounds__(DTHREADS) void chol_copy_kernel(const E* B, int64_t ldb, E* X, int64_t ldx, int64_t N, const int* info) {
  if (*info != 0) return;
  const E* b = B + (int64_t)blockIdx.x * ldb;
  E* x = X + (int64_t)blockIdx.x * ldx;
  for (int64_t i = threadIdx.x; i < N; i += DTHREADS) x[i] = b[i];
}

int64_t rls_direct_padded(int64_t N) { return (N + DB - 1) / DB * DB; }
// elements of the factor's allocation: the padded square and, behind it, the NB factored diagonal tiles
size_t rls_direct_factor_elems(int64_t N) {
  const size_t np = (size_t)rls_direct_padded(N);
  return np * np + np * DB;
}

int32_t rls_direct_launch_factor(rls_ctx* ctx, int32_t dtype, int64_t N, const void* G, int64_t ldg, float lambda, void* W, int* info) {
  const int64_t ld = rls_direct_padded(N);
  const int nb = (int)(ld / DB);
  return rls_with_elem(dtype, [&](auto t) -> int32_t {
    using E = typename decltype(t)::type;
    const size_t lds = 2 * (size_t)DB * DB * sizeof(E);
    RLS_TRY(rls_launch<chol_load_kernel<E>>(ctx, dim3(nb, nb), dim3(DTHREADS), 0, (const E*)G, ldg, N, lambda, (E*)W, ld, info));
    for (int j = 0; j < nb; ++j) {
      const int m = nb - 1 - j;
      RLS_TRY(rls_launch<chol_panel_kernel<E>>(ctx, dim3(m > 0 ? m : 1), dim3(DTHREADS), lds, (E*)W, ld, nb, j, (E*)W + ld * ld + (int64_t)j * DB * DB, info));
      if (m > 0) RLS_TRY(rls_launch<chol_trail_kernel<E>>(ctx, dim3(m, m), dim3(DTHREADS), 0, (E*)W, ld, j, (const int*)info));
    }
    return 0;
  });
}

int32_t rls_direct_launch_copy(rls_ctx* ctx, int32_t dtype, int64_t N, int K, const void* B, int64_t ldb, void* X, int64_t ldx, const int* info) {
  return rls_with_elem(dtype, [&](auto t) -> int32_t {
    using E = typename decltype(t)::type;
    return rls_launch<chol_copy_kernel<E>>(ctx, dim3((unsigned)K), dim3(DTHREADS), 0, (const E*)B, ldb, (E*)X, ldx, N, info);
  });
}

// X (N x K, columns ldx apart) holds the right-hand sides A^H B and receives the solutions; Y: workspace of 64 NB x K elements;
// K <= RLS_DIRECT_MAX_RHS (the column chunks are gridDim.y)
int32_t rls_direct_launch_solve(rls_ctx* ctx, int32_t dtype, int64_t N, const void* W, int K, void* X, int64_t ldx, void* Y, int proj,
                                const int* info) {
  const int64_t ld = rls_direct_padded(N);
  const int nb = (int)(ld / DB);
  const unsigned chunks = (unsigned)((K + DCOLS - 1) / DCOLS);
  return rls_with_elem(dtype, [&](auto t) -> int32_t {
    using E = typename decltype(t)::type;
    for (int j = 0; j < nb; ++j)
      RLS_TRY((rls_launch<chol_trsm_kernel<E, false>>(ctx, dim3(nb - j, chunks), dim3(DTHREADS), 0, (const E*)W, ld, j, K, (E*)X, ldx, N,
                                                      (E*)Y, ld, ld, (int)RLS_PROJ_NONE, info)));
    for (int j = nb - 1; j >= 0; --j)
      RLS_TRY((rls_launch<chol_trsm_kernel<E, true>>(ctx, dim3(j + 1, chunks), dim3(DTHREADS), 0, (const E*)W, ld, j, K, (E*)Y, ld, ld,
                                                     (E*)X, ldx, N, proj, info)));
    return 0;
  });
}
