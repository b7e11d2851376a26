// Sparse system matrices: the rls_sparse operator handle, its two products, rownorm², the scatter to a dense matrix and the
// Kaczmarz row sweep on sparse rows.  The reference treats a SparseMatrixCSC as a first-class operator:
// its own row dot (src/Utils.jl:89-100), row update (src/Kaczmarz.jl:526-539) and rownorm² (src/Utils.jl:26-33).
//
// Layouts.  The handle keeps the matrix TWICE on the device: CSC as the caller gave it (colptr / rowval / nzval, the layout of
// Julia's SparseMatrixCSC, 0-based) and a CSR copy built on the host by a stable counting transpose (columns ascend inside every
// row).  Both products are then GATHERS: y = A x walks the CSR rows, x = A^T y / A^H y walks the CSC columns, and every output
// element is summed by ONE group of lanes in a fixed order -- no atomics, the same bits run to run.  The second copy and the host
// transpose are setup cost, paid once per matrix in rls_sparse_create.
//
// Products.  L lanes own one output row (L = 1, 4, 16 or 64); lane s reads non-zeros k0 + s, k0 + s + L, ... of its row,
// so the L lanes of a row read consecutive values and indices (one coalesced run per pass) while the gathers of x go through L2.
// The partial sums meet in a DPP / permlane butterfly inside the group.  sp_pick_lanes chooses L per direction from the mean
// non-zeros per output row; rls_tune_set("sparse_lanes", L) forces it.
//
// Sweep.  One workgroup per right-hand side runs the row steps in order (rls_sparse_kaczmarz_sweep, the contract of
// rls_kaczmarz_sweep): x in the workgroup's LDS where N elements fit, else in global memory.  Only the immutable matrix data (row
// id, row pointers, the first pass of indices / values, u) is fetched ahead; x and vl are read inside the step that uses them.
#include "rls_common.hpp"
#include "plan_buffers.hpp"

#include <vector>

namespace {

constexpr int SP_THREADS = 256;                     // the product / rownorm² / scatter kernels
constexpr int SP_MAX_BLOCKS = 2048;                 // 8 workgroups of 256 per CU; more rows than one pass covers: grid stride
constexpr size_t SPK_LDS_BUDGET = 160 * 1024 - 512;  // the sweep's x in LDS (the budget of the other single-workgroup kernels)

template <typename E>
struct spe;  // the scalar type of E
template <>
struct spe<float> {
  using R = float;
  static constexpr bool cplx = false;
};
template <>
struct spe<float2> {
  using R = float;
  static constexpr bool cplx = true;
};
template <>
struct spe<double> {
  using R = double;
  static constexpr bool cplx = false;
};
template <>
struct spe<double2> {
  using R = double;
  static constexpr bool cplx = true;
};

template <typename E>
__device__ static inline typename spe<E>::R sp_re(E v) {
  if constexpr (spe<E>::cplx) return v.x;
  else return v;
}
template <typename E>
__device__ static inline typename spe<E>::R sp_im(E v) {
  if constexpr (spe<E>::cplx) return v.y;
  else return 0;
}
template <typename E>
__device__ static inline E sp_make(typename spe<E>::R re, typename spe<E>::R im) {
  if constexpr (spe<E>::cplx) {
    E e;
    e.x = re;
    e.y = im;
    return e;
  } else {
    return re;
  }
}
__device__ static inline float sp_fma(float a, float b, float c) { return fmaf(a, b, c); }
__device__ static inline double sp_fma(double a, double b, double c) { return ::fma(a, b, c); }
__device__ static inline float sp_dpp(float v, int ctrl) { return dpp_f(v, ctrl); }
__device__ static inline double sp_dpp(double v, int ctrl) { return dpp_d(v, ctrl); }

// sum over the L consecutive lanes of a group (aligned to L), complete in every lane of the group: the first steps of wave_sum.
// Every lane of the wave must be active.
template <int L, typename T>
__device__ static inline T sp_group_sum(T v) {
  static_assert(L == 1 || L == 4 || L == 16 || L == 64, "lanes per row");
  if constexpr (L >= 4) {
    v += sp_dpp(v, 0xB1);
    v += sp_dpp(v, 0x4E);
  }
  if constexpr (L >= 16) {
    v += sp_dpp(v, 0x141);
    v += sp_dpp(v, 0x140);
  }
  if constexpr (L == 64) {
    v = pair_sum16(v);
    v = pair_sum32(v);
  }
  return v;
}

// (sr, si) += op(a) * x, op = conj with CONJ
template <typename E, bool CONJ>
__device__ static inline void sp_acc(E a, E x, typename spe<E>::R& sr, typename spe<E>::R& si) {
  sr = sp_fma(sp_re(a), sp_re(x), sr);
  if constexpr (spe<E>::cplx) {
    if constexpr (CONJ) {
      sr = sp_fma(sp_im(a), sp_im(x), sr);
      si = sp_fma(sp_re(a), sp_im(x), si);
      si = sp_fma(-sp_im(a), sp_re(x), si);
    } else {
      sr = sp_fma(-sp_im(a), sp_im(x), sr);
      si = sp_fma(sp_re(a), sp_im(x), si);
      si = sp_fma(sp_im(a), sp_re(x), si);
    }
  }
}

// y[i] = alpha * sum_k op(val[k]) x[idx[k]] + beta * y[i] over the compressed rows ptr[i] .. ptr[i + 1] (CSR rows for A x, CSC
// columns for A^T y / A^H y).  L lanes per output row; the trip over row blocks is uniform for the whole workgroup, so every lane
// is active in the butterfly.  beta_zero: y is not read.
template <typename E, int L, bool CONJ>
__global__ __launch_bounds__(SP_THREADS) void sparse_mul_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx,
                                                                const E* __restrict__ val, const E* __restrict__ x, E* __restrict__ y,
                                                                int64_t nout, typename spe<E>::R ar, typename spe<E>::R ai,
                                                                typename spe<E>::R br, typename spe<E>::R bi, int beta_zero) {
  using R = typename spe<E>::R;
  constexpr int RPB = SP_THREADS / L;
  const int sub = threadIdx.x % L, rloc = threadIdx.x / L;
  for (int64_t row0 = (int64_t)blockIdx.x * RPB; row0 < nout; row0 += (int64_t)gridDim.x * RPB) {
    const int64_t row = row0 + rloc;
    const bool live = row < nout;
    R sr = 0, si = 0;
    if (live) {
      const int64_t k1 = ptr[row + 1];
      for (int64_t k = ptr[row] + sub; k < k1; k += L) sp_acc<E, CONJ>(val[k], x[idx[k]], sr, si);
    }
    sr = sp_group_sum<L>(sr);
    if constexpr (spe<E>::cplx) si = sp_group_sum<L>(si);
    if (live && sub == 0) {
      R re = ar * sr, im = 0;
      if constexpr (spe<E>::cplx) {
        re = sp_fma(-ai, si, re);
        im = sp_fma(ai, sr, ar * si);
      }
      if (!beta_zero) {
        const E yv = y[row];
        re = sp_fma(br, sp_re(yv), re);
        if constexpr (spe<E>::cplx) {
          re = sp_fma(-bi, sp_im(yv), re);
          im = sp_fma(br, sp_im(yv), im);
          im = sp_fma(bi, sp_re(yv), im);
        }
      }
      y[row] = sp_make<E>(re, im);
    }
  }
}

// out[i] = sum_k |val[k]|^2 over CSR row i (src/Utils.jl:26-33), 16 lanes per row
template <typename E>
__global__ __launch_bounds__(SP_THREADS) void sparse_rownorm2_kernel(const int64_t* __restrict__ ptr, const E* __restrict__ val,
                                                                     typename spe<E>::R* __restrict__ out, int64_t M) {
  using R = typename spe<E>::R;
  constexpr int L = 16, RPB = SP_THREADS / L;
  const int sub = threadIdx.x % L, rloc = threadIdx.x / L;
  for (int64_t row0 = (int64_t)blockIdx.x * RPB; row0 < M; row0 += (int64_t)gridDim.x * RPB) {
    const int64_t row = row0 + rloc;
    const bool live = row < M;
    R s = 0;
    if (live) {
      const int64_t k1 = ptr[row + 1];
      for (int64_t k = ptr[row] + sub; k < k1; k += L) {
        const E a = val[k];
        s = sp_fma(sp_re(a), sp_re(a), s);
        if constexpr (spe<E>::cplx) s = sp_fma(sp_im(a), sp_im(a), s);
      }
    }
    s = sp_group_sum<L>(s);
    if (live && sub == 0) out[row] = s;
  }
}

// A[rowval[k], j] = val[k] for the non-zeros of CSC column j, 16 lanes per column (A zeroed by the launcher)
template <typename E>
__global__ __launch_bounds__(SP_THREADS) void sparse_scatter_kernel(const int64_t* __restrict__ colptr, const int32_t* __restrict__ rowval,
                                                                    const E* __restrict__ val, E* __restrict__ A, int64_t lda, int64_t N) {
  constexpr int L = 16, CPB = SP_THREADS / L;
  const int sub = threadIdx.x % L, cloc = threadIdx.x / L;
  for (int64_t col = (int64_t)blockIdx.x * CPB + cloc; col < N; col += (int64_t)gridDim.x * CPB) {
    const int64_t k1 = colptr[col + 1];
    for (int64_t k = colptr[col] + sub; k < k1; k += L) A[(int64_t)rowval[k] + col * lda] = val[k];
  }
}

// The sparse row sweep.  Row step (src/Kaczmarz.jl:283-308 on a sparse row):
//   tau = sum_k a_k x[col_k]  (src/Utils.jl:89-100, non-conjugating);  alpha = denom[i] (u[row] - tau - eps_w vl[row])  (:305);
//   x[col_k] += alpha conj(a_k)  (:532-539);  vl[row] += alpha eps_w  (:307).
// Thread t owns non-zeros k0 + t, k0 + t + NT, ... of the row in BOTH passes, and the columns of a row are distinct: no two threads
// touch one x element inside a step.  The barrier at the end of a step orders its writes of x and vl ahead of the next step's
// reads, so consecutive rows may share columns, and the same row may run back to back (nused = 1).  tau and alpha are carried in
// double for every element type.
// Fetched ahead, three stages deep, is immutable data only: the row id and denominator of step j + 3, the row pointers of step
// j + 2, the first pass of indices / values and u[row] of step j + 1.  Their addresses are clamped, never predicated; positions
// wrap inside [0, nused), so what is fetched behind the last step is in bounds and unused.
template <typename E, int NT, bool LDSX>
__global__ __launch_bounds__(NT) void sparse_kaczmarz_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ colval,
                                                             const E* __restrict__ val, E* X, int64_t ldx, const E* __restrict__ U, int64_t ldu,
                                                             E* VL, int64_t ldvl, const int32_t* __restrict__ rows,
                                                             const typename spe<E>::R* __restrict__ den, int nused, int n_sweeps,
                                                             double eps_w, int64_t N) {
  using R = typename spe<E>::R;
  constexpr int NW = NT / 64;
  extern __shared__ __align__(16) unsigned char spk_smem[];
  __shared__ double red[NW][2];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  E* xg = X + (int64_t)blockIdx.x * ldx;
  const E* u = U + (int64_t)blockIdx.x * ldu;
  E* vl = VL + (int64_t)blockIdx.x * ldvl;
  E* xs = xg;
  if constexpr (LDSX) {
    xs = reinterpret_cast<E*>(spk_smem);
    for (int64_t i = tid; i < N; i += NT) xs[i] = xg[i];
    __syncthreads();
  }

  const int64_t total = (int64_t)nused * n_sweeps;
  auto next_pos = [nused](int p) { return p + 1 == nused ? 0 : p + 1; };
  // prologue: the three stages, filled one after the other
  int p3 = 0;
  int r0 = rows[p3];
  R d0 = den[p3];
  p3 = next_pos(p3);
  int r1 = rows[p3];
  R d1 = den[p3];
  p3 = next_pos(p3);
  int r2 = rows[p3];
  R d2 = den[p3];
  p3 = next_pos(p3);
  int64_t k00 = rowptr[r0], k10 = rowptr[r0 + 1];
  int64_t k01 = rowptr[r1], k11 = rowptr[r1 + 1];
  bool have0 = k00 + tid < k10;
  int64_t ka = have0 ? k00 + tid : 0;
  int c0 = colval[ka];
  E a0 = val[ka];
  E u0 = u[r0];

  for (int64_t j = 0; j < total; ++j) {
    // ---- the loads of the next three steps (matrix data, u, the order table: nothing a row step writes)
    const int r3 = rows[p3];
    const R d3 = den[p3];
    p3 = next_pos(p3);
    const int64_t k02 = rowptr[r2], k12 = rowptr[r2 + 1];
    const bool have1 = k01 + tid < k11;
    ka = have1 ? k01 + tid : 0;
    const int c1 = colval[ka];
    const E a1 = val[ka];
    const E u1 = u[r1];
    // vl[row] of THIS step: issued here, behind the barrier that ended the previous step (which wrote vl), so that its flight
    // overlaps the dot product instead of following it
    const E vv = vl[r0];

    // ---- tau
    double tr = 0.0, ti = 0.0;
    if (have0) {
      const E xe = xs[c0];
      tr = (double)sp_re(a0) * (double)sp_re(xe);
      if constexpr (spe<E>::cplx) {
        tr = ::fma(-(double)sp_im(a0), (double)sp_im(xe), tr);
        ti = (double)sp_re(a0) * (double)sp_im(xe);
        ti = ::fma((double)sp_im(a0), (double)sp_re(xe), ti);
      }
    }
    for (int64_t k = k00 + tid + NT; k < k10; k += NT) {
      const E av = val[k], xe = xs[colval[k]];
      tr = ::fma((double)sp_re(av), (double)sp_re(xe), tr);
      if constexpr (spe<E>::cplx) {
        tr = ::fma(-(double)sp_im(av), (double)sp_im(xe), tr);
        ti = ::fma((double)sp_re(av), (double)sp_im(xe), ti);
        ti = ::fma((double)sp_im(av), (double)sp_re(xe), ti);
      }
    }
    tr = wave_sum(tr);
    if constexpr (spe<E>::cplx) ti = wave_sum(ti);
    if constexpr (NW > 1) {
      if (lane == 0) {
        red[w][0] = tr;
        red[w][1] = ti;
      }
      __syncthreads();  // (red is rewritten only behind the barrier that ends this step)
      tr = 0.0, ti = 0.0;
#pragma unroll
      for (int ww = 0; ww < NW; ++ww) {
        tr += red[ww][0];
        ti += red[ww][1];
      }
    }
    // ---- alpha = denom (u[row] - tau - eps_w vl[row])
    const double are = (double)d0 * (((double)sp_re(u0) - tr) - eps_w * (double)sp_re(vv));
    const double aim = spe<E>::cplx ? (double)d0 * (((double)sp_im(u0) - ti) - eps_w * (double)sp_im(vv)) : 0.0;
    const R alr = (R)are, ali = (R)aim;
    // ---- x[col_k] += alpha conj(a_k)
    if (have0) {
      const E xe = xs[c0];
      R xr = sp_fma(alr, sp_re(a0), sp_re(xe)), xi = sp_im(xe);
      if constexpr (spe<E>::cplx) {
        xr = sp_fma(ali, sp_im(a0), xr);
        xi = sp_fma(ali, sp_re(a0), xi);
        xi = sp_fma(-alr, sp_im(a0), xi);
      }
      xs[c0] = sp_make<E>(xr, xi);
    }
    for (int64_t k = k00 + tid + NT; k < k10; k += NT) {
      const E av = val[k];
      const int c = colval[k];
      const E xe = xs[c];
      R xr = sp_fma(alr, sp_re(av), sp_re(xe)), xi = sp_im(xe);
      if constexpr (spe<E>::cplx) {
        xr = sp_fma(ali, sp_im(av), xr);
        xi = sp_fma(ali, sp_re(av), xi);
        xi = sp_fma(-alr, sp_im(av), xi);
      }
      xs[c] = sp_make<E>(xr, xi);
    }
    // ---- vl[row] += alpha eps_w
    if (tid == 0) vl[r0] = sp_make<E>((R)((double)sp_re(vv) + are * eps_w), (R)((double)sp_im(vv) + aim * eps_w));
    __syncthreads();  // x and vl of this step are written before the next step reads them
    r0 = r1, d0 = d1, k00 = k01, k10 = k11, have0 = have1, c0 = c1, a0 = a1, u0 = u1;
    r1 = r2, d1 = d2, k01 = k02, k11 = k12;
    r2 = r3, d2 = d3;
  }
  if constexpr (LDSX) {
    for (int64_t i = tid; i < N; i += NT) xg[i] = xs[i];
  }
}

static inline size_t sp_elem_size(int32_t dtype) { return dtype == RLS_F32 ? 4 : dtype == RLS_C64 ? 16 : 8; }
static inline size_t sp_real_size(int32_t dtype) { return dtype == RLS_F64 || dtype == RLS_C64 ? 8 : 4; }

// calls fn(rls_type<E>{}) for the handle's element type
template <typename F>
static inline int32_t sp_dispatch(int32_t dtype, F&& fn) {
  if (dtype == RLS_F64 || dtype == RLS_C64) return rls_with_elem64(dtype, fn);
  return rls_with_elem(dtype, fn);
}

static plan_buffers sp_memory(rls_ctx* ctx) {
  return plan_buffers([](void** p, size_t bytes) { return (int)rls_scoped_malloc(p, bytes); }, [](void* p) { (void)rls_scoped_free(p); },
                      [](void** p, size_t bytes) { return (int)rls_pinned_alloc(p, bytes); }, [](void* p) { rls_pinned_free(p); },
                      [ctx](void* p, size_t bytes) { return (int)hipMemsetAsync(p, 0, bytes, ctx->stream); });
}

// Lanes per output row from the mean non-zeros per output row.  The thresholds come from profiles/sparse.txt (tools/bench_sparse.py,
// every instantiation forced in turn):
//   1 | 4    the tall table (524288 x 1024, exactly k per row, bandwidth-bound): L = 1 leads at 1 and 2 per row (3.9 against 6.6 us,
//            4.2 against 6.2 us), L = 4 at 4 per row (6.0 us as the automatic choice against 7.1 us);
//   4 | 16   the tall table: L = 4 leads at 8 per row (11.3 against 17.0 us) and still by 7 % at 16 (18.3 against 19.6 us, outside
//            the spread); the square shapes: L = 16 leads at 41 per row (4.4 against 4.9 us) and 82 (4.3 against 6.9 us);
//   16 | 64  the square shapes: within the spread of each other up to 102 per row, L = 64 leads at 205 (4.4 against 5.0 us) and
//            by 3 x at 410.  Between 102 and 205 nothing is measured: 128 is a choice inside that gap.
static int sp_pick_lanes(int64_t nnz, int64_t nout) {
  const double mean = nout > 0 ? (double)nnz / (double)nout : 0.0;
  if (mean <= 2.0) return 1;
  if (mean <= 16.0) return 4;
  if (mean <= 128.0) return 16;
  return 64;
}

static inline unsigned sp_grid(int64_t items, int per_block) {
  int64_t g = (items + per_block - 1) / per_block;
  if (g > SP_MAX_BLOCKS) g = SP_MAX_BLOCKS;
  if (g < 1) g = 1;
  return (unsigned)g;
}

}  // namespace

struct rls_sparse {
  plan_buffers mem;  // owns every device block below
  rls_ctx* ctx = nullptr;
  uint64_t ctx_id = 0;
  int32_t dtype = RLS_F32;
  int64_t M = 0, N = 0, nnz = 0;
  int64_t *rowptr = nullptr, *colptr = nullptr;  // CSR: int64[M + 1]; CSC: int64[N + 1]
  int32_t *colval = nullptr, *rowval = nullptr;  // CSR column of every non-zero; CSC row of every non-zero
  void *rnz = nullptr, *cnz = nullptr;           // the values in CSR order and in CSC order
  int lanes_n = 1, lanes_t = 1;                  // sp_pick_lanes for A x and for A^T y / A^H y
};

namespace {

static bool sp_live(const rls_sparse* sp) { return sp && rls_ctx_alive(sp->ctx, sp->ctx_id); }
static int sp_lanes(const rls_sparse* sp, int32_t op) {
  const int forced = sp->ctx->tune.sparse_lanes;
  return forced ? forced : (op == RLS_OP_N ? sp->lanes_n : sp->lanes_t);
}

template <typename T>
static int32_t sp_transpose_host(int64_t M, int64_t N, const int64_t* colptr, const int32_t* rowval, const T* nz, int64_t* rowptr,
                                 int32_t* colval, T* out) {
  const int64_t nnz = colptr[N];
  for (int64_t i = 0; i <= M; ++i) rowptr[i] = 0;
  for (int64_t k = 0; k < nnz; ++k) ++rowptr[rowval[k] + 1];
  for (int64_t i = 0; i < M; ++i) rowptr[i + 1] += rowptr[i];
  std::vector<int64_t> at(rowptr, rowptr + M);
  for (int64_t j = 0; j < N; ++j)  // columns in ascending order: they ascend inside every row (stable)
    for (int64_t k = colptr[j]; k < colptr[j + 1]; ++k) {
      const int64_t q = at[rowval[k]]++;
      colval[q] = (int32_t)j;
      out[q] = nz[k];
    }
  return 0;
}

}  // namespace

extern "C" {

int32_t rls_sparse_csr_from_csc_host(int32_t dtype, int64_t M, int64_t N, const int64_t* colptr, const int32_t* rowval, const void* nzval,
                                     int64_t* rowptr_out, int32_t* colval_out, void* nzval_out) {
  if (dtype < RLS_F32 || dtype > RLS_C64 || M < 1 || N < 1 || M >= ((int64_t)1 << 31) || N >= ((int64_t)1 << 31) || !colptr)
    return RLS_E_INVALID;
  const bool validate_only = !rowptr_out && !colval_out && !nzval_out;  // all three outputs null: the checks alone, nothing written
  if (!rowptr_out && !validate_only) return RLS_E_INVALID;
  if (colptr[0] != 0) return RLS_E_INVALID;
  for (int64_t j = 0; j < N; ++j)
    if (colptr[j + 1] < colptr[j]) return RLS_E_INVALID;
  const int64_t nnz = colptr[N];
  if (nnz > 0 && (!rowval || !nzval || (!validate_only && (!colval_out || !nzval_out)))) return RLS_E_INVALID;
  for (int64_t j = 0; j < N; ++j)
    for (int64_t k = colptr[j]; k < colptr[j + 1]; ++k) {
      if (rowval[k] < 0 || rowval[k] >= M) return RLS_E_INVALID;
      if (k > colptr[j] && rowval[k] <= rowval[k - 1]) return RLS_E_INVALID;  // unsorted or duplicated inside a column
    }
  if (validate_only) return 0;
  struct c16 {
    double re, im;
  };
  switch (sp_elem_size(dtype)) {
    case 4: return sp_transpose_host(M, N, colptr, rowval, (const uint32_t*)nzval, rowptr_out, colval_out, (uint32_t*)nzval_out);
    case 8: return sp_transpose_host(M, N, colptr, rowval, (const uint64_t*)nzval, rowptr_out, colval_out, (uint64_t*)nzval_out);
    default: return sp_transpose_host(M, N, colptr, rowval, (const c16*)nzval, rowptr_out, colval_out, (c16*)nzval_out);
  }
}

int32_t rls_sparse_destroy(rls_sparse* sp) {
  if (!sp) return RLS_E_INVALID;
  rls_ctx* ctx = sp_live(sp) ? sp->ctx : nullptr;
  rls_alloc_scope alloc_scope(ctx);
  sp->mem.release();
  delete sp;
  return 0;
}

int32_t rls_sparse_create(rls_ctx* ctx, int32_t dtype, int64_t M, int64_t N, const int64_t* colptr_h, const int32_t* rowval_h,
                          const void* nzval_h, rls_sparse** out) {
  RLS_CHECK_CTX(ctx);
  if (!out) return rls_fail(ctx, RLS_E_INVALID, "sparse_create: null out");
  *out = nullptr;
  if (dtype < RLS_F32 || dtype > RLS_C64 || M < 1 || N < 1 || M >= ((int64_t)1 << 31) || N >= ((int64_t)1 << 31) || !colptr_h)
    return rls_fail(ctx, RLS_E_INVALID, "sparse_create: bad argument");
  const size_t es = sp_elem_size(dtype);
  // (colptr is checked here as well: nnz = colptr[N] sizes the host copy before the validating transpose runs)
  if (colptr_h[0] != 0) return rls_fail(ctx, RLS_E_INVALID, "sparse_create: colptr[0] != 0");
  for (int64_t j = 0; j < N; ++j)
    if (colptr_h[j + 1] < colptr_h[j]) return rls_fail(ctx, RLS_E_INVALID, "sparse_create: colptr decreases");
  const int64_t nnz = colptr_h[N];
  std::vector<int64_t> rowptr((size_t)M + 1);
  std::vector<int32_t> colval((size_t)nnz + 1);
  std::vector<unsigned char> rnz((size_t)nnz * es + 16);
  if (rls_sparse_csr_from_csc_host(dtype, M, N, colptr_h, rowval_h, nzval_h, rowptr.data(), colval.data(), rnz.data()) != 0)
    return rls_fail(ctx, RLS_E_INVALID, "sparse_create: not a valid CSC matrix (row indices in [0, M), strictly increasing inside a column)");
  RLS_HIP(ctx, rls_enter(ctx));
  rls_alloc_scope alloc_scope(ctx);
  rls_sparse* sp = new rls_sparse{sp_memory(ctx)};
  sp->ctx = ctx;
  sp->ctx_id = ctx->id;
  sp->dtype = dtype;
  sp->M = M;
  sp->N = N;
  sp->nnz = nnz;
  sp->lanes_n = sp_pick_lanes(nnz, M);
  sp->lanes_t = sp_pick_lanes(nnz, N);
  // (at least 16 bytes behind every index / value block: the sweep's clamped prefetch reads element 0 of a matrix without non-zeros)
  const size_t ib = (size_t)nnz * 4 + 16, vb = (size_t)nnz * es + 16;
  sp->mem.dev(&sp->rowptr, ((size_t)M + 1) * 8, false);
  sp->mem.dev(&sp->colptr, ((size_t)N + 1) * 8, false);
  sp->mem.dev(&sp->colval, ib, true);
  sp->mem.dev(&sp->rowval, ib, true);
  sp->mem.dev(&sp->rnz, vb, true);
  sp->mem.dev(&sp->cnz, vb, true);
  if (const int e = sp->mem.error()) {
    rls_sparse_destroy(sp);
    return rls_fail(ctx, e, "sparse_create: allocation failed");
  }
  hipError_t e = hipMemcpyAsync(sp->rowptr, rowptr.data(), ((size_t)M + 1) * 8, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(sp->colptr, colptr_h, ((size_t)N + 1) * 8, hipMemcpyHostToDevice, ctx->stream);
  if (nnz > 0) {
    if (e == hipSuccess) e = hipMemcpyAsync(sp->colval, colval.data(), (size_t)nnz * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(sp->rowval, rowval_h, (size_t)nnz * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(sp->rnz, rnz.data(), (size_t)nnz * es, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(sp->cnz, nzval_h, (size_t)nnz * es, hipMemcpyHostToDevice, ctx->stream);
  }
  if (e == hipSuccess) e = rls_stream_wait(ctx->stream);  // the host arrays (the caller's and the CSR copy here) are free on return
  if (e != hipSuccess) {
    rls_sparse_destroy(sp);
    return rls_fail(ctx, (int32_t)e, "sparse_create: upload failed");
  }
  *out = sp;
  return 0;
}

int32_t rls_sparse_info(rls_sparse* sp, int64_t* M, int64_t* N, int64_t* nnz) {
  if (!sp) return RLS_E_INVALID;
  if (M) *M = sp->M;
  if (N) *N = sp->N;
  if (nnz) *nnz = sp->nnz;
  return 0;
}

int32_t rls_sparse_to_host(rls_sparse* sp, int64_t* colptr_h, int32_t* rowval_h, void* nzval_h) {
  if (!sp_live(sp)) return RLS_E_INVALID;
  rls_ctx* ctx = sp->ctx;
  if (!colptr_h || (sp->nnz > 0 && (!rowval_h || !nzval_h))) return rls_fail(ctx, RLS_E_INVALID, "sparse_to_host: null pointer");
  RLS_HIP(ctx, rls_enter(ctx));
  RLS_HIP(ctx, hipMemcpyAsync(colptr_h, sp->colptr, ((size_t)sp->N + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (sp->nnz > 0) {
    RLS_HIP(ctx, hipMemcpyAsync(rowval_h, sp->rowval, (size_t)sp->nnz * 4, hipMemcpyDeviceToHost, ctx->stream));
    RLS_HIP(ctx, hipMemcpyAsync(nzval_h, sp->cnz, (size_t)sp->nnz * sp_elem_size(sp->dtype), hipMemcpyDeviceToHost, ctx->stream));
  }
  RLS_HIP(ctx, rls_stream_wait(ctx->stream));
  return 0;
}

int32_t rls_sparse_variant(rls_sparse* sp, int32_t op, int32_t* out) {
  if (!sp_live(sp) || !out || op < RLS_OP_N || op > RLS_OP_C) return RLS_E_INVALID;
  *out = sp_lanes(sp, op);
  return 0;
}

int32_t rls_sparse_mul(rls_sparse* sp, int32_t op, double alpha_re, double alpha_im, const void* x, double beta_re, double beta_im, void* y) {
  if (!sp_live(sp)) return RLS_E_INVALID;
  rls_ctx* ctx = sp->ctx;
  if (!x || !y || op < RLS_OP_N || op > RLS_OP_C) return rls_fail(ctx, RLS_E_INVALID, "sparse_mul: bad argument");
  RLS_HIP(ctx, rls_enter(ctx));
  const bool fwd = op == RLS_OP_N;
  const int64_t nout = fwd ? sp->M : sp->N;
  const int64_t* ptr = fwd ? sp->rowptr : sp->colptr;
  const int32_t* idx = fwd ? sp->colval : sp->rowval;
  const void* val = fwd ? sp->rnz : sp->cnz;
  const int beta_zero = beta_re == 0.0 && beta_im == 0.0;
  const bool real = sp->dtype == RLS_F32 || sp->dtype == RLS_F64;
  return sp_dispatch(sp->dtype, [&](auto t) {
    using E = typename decltype(t)::type;
    using R = typename spe<E>::R;
    return rls_with<1, 4, 16, 64>(sp_lanes(sp, op), [&](auto l) {
      constexpr int L = decltype(l)::value;
      return with_bool(op == RLS_OP_C && !real, [&](auto c) {
        constexpr bool CONJ = decltype(c)::value;
        if constexpr (CONJ && !spe<E>::cplx) {
          return (int32_t)RLS_E_INVALID;  // (not reached: real types never conjugate)
        } else {
          return rls_launch<sparse_mul_kernel<E, L, CONJ>>(ctx, dim3(sp_grid(nout, SP_THREADS / L)), dim3(SP_THREADS), 0, ptr, idx, (const E*)val,
                                                           (const E*)x, (E*)y, nout, (R)alpha_re, (R)alpha_im, (R)beta_re, (R)beta_im, beta_zero);
        }
      });
    });
  });
}

int32_t rls_sparse_rownorm2(rls_sparse* sp, void* out_d) {
  if (!sp_live(sp)) return RLS_E_INVALID;
  rls_ctx* ctx = sp->ctx;
  if (!out_d) return rls_fail(ctx, RLS_E_INVALID, "sparse_rownorm2: null out");
  RLS_HIP(ctx, rls_enter(ctx));
  return sp_dispatch(sp->dtype, [&](auto t) {
    using E = typename decltype(t)::type;
    return rls_launch<sparse_rownorm2_kernel<E>>(ctx, dim3(sp_grid(sp->M, SP_THREADS / 16)), dim3(SP_THREADS), 0, sp->rowptr, (const E*)sp->rnz,
                                                 (typename spe<E>::R*)out_d, sp->M);
  });
}

int32_t rls_sparse_to_dense(rls_sparse* sp, void* A, int64_t lda) {
  if (!sp_live(sp)) return RLS_E_INVALID;
  rls_ctx* ctx = sp->ctx;
  if (!A || lda < sp->M) return rls_fail(ctx, RLS_E_INVALID, "sparse_to_dense: null A or lda < M");
  RLS_HIP(ctx, rls_enter(ctx));
  const size_t es = sp_elem_size(sp->dtype);
  RLS_HIP(ctx, hipMemset2DAsync(A, (size_t)lda * es, 0, (size_t)sp->M * es, (size_t)sp->N, ctx->stream));
  return sp_dispatch(sp->dtype, [&](auto t) {
    using E = typename decltype(t)::type;
    return rls_launch<sparse_scatter_kernel<E>>(ctx, dim3(sp_grid(sp->N, SP_THREADS / 16)), dim3(SP_THREADS), 0, sp->colptr, sp->rowval,
                                                (const E*)sp->cnz, (E*)A, lda, sp->N);
  });
}

int32_t rls_sparse_kaczmarz_sweep(rls_sparse* sp, int32_t nrhs, void* X, int64_t ldx, const void* U, int64_t ldu, void* VL, int64_t ldvl,
                                  const int32_t* rows_d, const void* denom_d, int32_t nused, double eps_w, int32_t n_sweeps) {
  if (!sp_live(sp)) return RLS_E_INVALID;
  rls_ctx* ctx = sp->ctx;
  if (!X || !U || !VL || !rows_d || !denom_d || nrhs < 1 || nused < 1 || nused > sp->M || n_sweeps < 0 || ldx < sp->N || ldu < sp->M ||
      ldvl < sp->M)
    return rls_fail(ctx, RLS_E_INVALID, "sparse_kaczmarz_sweep: bad argument");
  if (n_sweeps == 0) return 0;
  RLS_HIP(ctx, rls_enter(ctx));
  const size_t xbytes = (size_t)sp->N * sp_elem_size(sp->dtype);
  const bool ldsx = ctx->tune.sparse_kaczmarz_lds != 0 && xbytes <= SPK_LDS_BUDGET;
  // one wave while the mean row is one pass of it (no cross-wave reduction, no second barrier); longer rows: four waves, so that
  // rows of up to 256 non-zeros stay one pass -- only the first pass of a row is fetched ahead, a second one loads inside the step
  const bool wide = sp->nnz > 64 * sp->M;
  return sp_dispatch(sp->dtype, [&](auto t) {
    using E = typename decltype(t)::type;
    using R = typename spe<E>::R;
    return rls_with<64, 256>(wide ? 256 : 64, [&](auto n) {
      constexpr int NT = decltype(n)::value;
      return with_bool(ldsx, [&](auto b) -> int32_t {
        constexpr bool LDSX = decltype(b)::value;
        if constexpr (LDSX) {
          // (every launch of an instantiation is allowed the whole budget: rls_allow_lds sets the attribute once per device)
          const hipError_t e = rls_allow_lds<sparse_kaczmarz_kernel<E, NT, LDSX>>(ctx->device, SPK_LDS_BUDGET);
          if (e != hipSuccess) return rls_fail(ctx, (int32_t)e, "hipFuncSetAttribute (dynamic LDS) failed");
        }
        hipLaunchKernelGGL((sparse_kaczmarz_kernel<E, NT, LDSX>), dim3((unsigned)nrhs), dim3(NT), LDSX ? xbytes : 0, ctx->stream, sp->rowptr,
                           sp->colval, (const E*)sp->rnz, (E*)X, ldx, (const E*)U, ldu, (E*)VL, ldvl, rows_d, (const R*)denom_d, (int)nused,
                           (int)n_sweeps, eps_w, sp->N);
        return launch_status(ctx);
      });
    });
  });
}

}  // extern "C"
