// Matrix-free operators: SamplingOp, FFTOp and their product S o F, the operator of the reference's
// compressed-sensing example (docs/src/literate/examples/compressed_sensing.jl).  LinearOperatorCollection is third-party to the
// reference, like GradientOp and WaveletOp: the operators are restated from their documented definitions.
//
// Sampling (all four element types): y[k] = x[idx[k]], its adjoint (zero, then a scatter: the indices are unique, so no atomics) and
// the normal operator v = mask .* p with a 0 / 1 mask of the element's REAL type (exact products, signs of zero included).
//
// FFT (ComplexF32 / ComplexF64, power-of-two extents, 1-D and 2-D column-major): radix-2 IN PLACE in LDS.
//   forward:  natural order in, decimation in frequency (half-span n/2 ... 1), result at the bit-reversed positions;
//   adjoint:  input placed at the bit-reversed positions, decimation in time with conjugated twiddles (half-span 1 ... n/2), natural out.
// Stage by stage the adjoint is the conjugate transpose of the forward, and F^H diag(mask) F needs no permutation at all: the mask is
// applied at the bit-reversed positions between the two.  Twiddles come from a table computed in double on the host (rls_fft_create).
// fftshift / ifftshift of an even extent are the sign pattern (-1)^k on input and output (and one global sign for n = 2), folded into
// the load and the store; the unitary scale 1 / sqrt(n1 n2) multiplies in the last store.
//
// Two paths, one arithmetic (fft_lines: explicit fma chains, so the results are the same bits):
//   * general: one launch per dimension, a workgroup transforms a bundle of lines in LDS (in place in global memory is fine: a
//     workgroup has read its whole bundle before it stores);
//   * single workgroup: the image in ONE workgroup's LDS, both dimensions -- and for the normal operator the mask and the way back --
//     in one launch.
// fft_use_fused (host) is THE statement of which path runs.
//
// LDS layout.  Lines along dimension 0 are contiguous ([line][k]); a butterfly of half-span h >= 64 is two runs of consecutive
// 8-byte elements per half wave: conflict-free.  Below that a radix-2 stage would put the two 16-lane runs of a half wave on the
// same banks (elements i .. i+15 and i+32 .. i+47 are 64 dwords apart), so the last six stages do not go through LDS: a lane holds
// one element and exchanges with lane ^ h (fft_tail_wave).  Lines along dimension 1 are stored [k][line]: consecutive lanes take
// consecutive lines of one butterfly, consecutive addresses at every half-span.  The bit-reversed placement on load (adjoint) or
// store (forward) is the one LDS pass that does conflict (up to 8-way on the writes): one pass of log2(n) + 2.
#include <cmath>
#include <vector>

#include "rls_common.hpp"

namespace {

constexpr int MF_THREADS = 256;      // sampling kernels: grid-stride
constexpr int MF_MAX_GRID = 2048;    // ... over at most this many workgroups (a second pass from 2048 * 256 = 524288 elements on)
// general path: the dynamic LDS of one workgroup.  64 KiB is what a kernel gets without raising its limit, and two workgroups of the
// longest line still share a CU (160 KiB); it fixes the longest line: 8192 ComplexF32, 4096 ComplexF64 points.
constexpr size_t FFT_LINE_LDS = 64 * 1024;
// single-workgroup path: the whole image in one workgroup's LDS (160 KiB a CU, 512 bytes left to the runtime, as wavelet.hip has it):
// up to 16384 ComplexF32 (128 x 128) or 8192 ComplexF64 points
constexpr size_t FFT_FUSED_LDS = 160 * 1024 - 512;
constexpr int64_t FFT_FUSED_AUTO_N = 1024;  // ... and what the automatic choice sends there (fft_use_fused)
constexpr int FFT_THREADS = 1024;
constexpr int FFT_LG_BUNDLE = 10;    // general path: a workgroup takes 2^10 points where the lines are shorter than that
enum { FFT_FWD = 1, FFT_MASK = 2, FFT_INV = 4 };

static inline size_t mf_elem_size(int32_t dtype) { return dtype == RLS_F32 ? 4 : dtype == RLS_C64 ? 16 : 8; }
static inline unsigned mf_grid(int64_t total) {
  int64_t g = (total + MF_THREADS - 1) / MF_THREADS;
  return (unsigned)(g > MF_MAX_GRID ? MF_MAX_GRID : (g < 1 ? 1 : g));
}

// ---- element arithmetic: explicit products and fma chains in one order (-ffp-contract may not regroup them) ----------------------
template <typename E>
struct mfe;
template <>
struct mfe<float> {
  using R = float;
  __device__ static inline float zero() { return 0.0f; }
  __device__ static inline float rmul(float a, float s) { return __fmul_rn(a, s); }
  __device__ static inline float add(float a, float b) { return a + b; }
  __device__ static inline float mul(float a, float wr, float) { return __fmul_rn(a, wr); }
};
template <>
struct mfe<double> {
  using R = double;
  __device__ static inline double zero() { return 0.0; }
  __device__ static inline double rmul(double a, double s) { return __dmul_rn(a, s); }
  __device__ static inline double add(double a, double b) { return a + b; }
  __device__ static inline double mul(double a, double wr, double) { return __dmul_rn(a, wr); }
};
template <>
struct mfe<float2> {
  using R = float;
  __device__ static inline float2 zero() { return make_float2(0.0f, 0.0f); }
  __device__ static inline float2 rmul(float2 a, float s) { return make_float2(__fmul_rn(a.x, s), __fmul_rn(a.y, s)); }
  __device__ static inline float2 add(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
  __device__ static inline float2 sub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
  __device__ static inline float2 neg(float2 a) { return make_float2(-a.x, -a.y); }
  // a * (wr + i wi)
  __device__ static inline float2 mul(float2 a, float wr, float wi) {
    return make_float2(fmaf(a.x, wr, -__fmul_rn(a.y, wi)), fmaf(a.x, wi, __fmul_rn(a.y, wr)));
  }
  // a * conj(w)
  __device__ static inline float2 mulc(float2 a, float2 w) {
    return make_float2(fmaf(a.x, w.x, __fmul_rn(a.y, w.y)), fmaf(a.y, w.x, -__fmul_rn(a.x, w.y)));
  }
  __device__ static inline float2 xchg(float2 a, int h) { return make_float2(__shfl_xor(a.x, h), __shfl_xor(a.y, h)); }
};
template <>
struct mfe<double2> {
  using R = double;
  __device__ static inline double2 zero() { return make_double2(0.0, 0.0); }
  __device__ static inline double2 rmul(double2 a, double s) { return make_double2(__dmul_rn(a.x, s), __dmul_rn(a.y, s)); }
  __device__ static inline double2 add(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
  __device__ static inline double2 sub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
  __device__ static inline double2 neg(double2 a) { return make_double2(-a.x, -a.y); }
  __device__ static inline double2 mul(double2 a, double wr, double wi) {
    return make_double2(fma(a.x, wr, -__dmul_rn(a.y, wi)), fma(a.x, wi, __dmul_rn(a.y, wr)));
  }
  __device__ static inline double2 mulc(double2 a, double2 w) {
    return make_double2(fma(a.x, w.x, __dmul_rn(a.y, w.y)), fma(a.y, w.x, -__dmul_rn(a.x, w.y)));
  }
  __device__ static inline double2 xchg(double2 a, int h) { return make_double2(__shfl_xor(a.x, h), __shfl_xor(a.y, h)); }
};

// ---- sampling --------------------------------------------------------------------------------------------------------------------
// y[k] = alpha x[idx[k]] + beta y[k]  (PLAIN: alpha = 1, beta = 0, a copy; beta_zero: y is not read)
template <typename E, bool PLAIN>
__global__ __launch_bounds__(MF_THREADS) void sampling_gather_kernel(const int32_t* __restrict__ idx, const E* __restrict__ x, E* __restrict__ y,
                                                                     int64_t m, typename mfe<E>::R ar, typename mfe<E>::R ai,
                                                                     typename mfe<E>::R br, typename mfe<E>::R bi, int beta_zero) {
  for (int64_t k = (int64_t)blockIdx.x * MF_THREADS + threadIdx.x; k < m; k += (int64_t)gridDim.x * MF_THREADS) {
    const E v = x[idx[k]];
    if constexpr (PLAIN) {
      y[k] = v;
    } else {
      E r = mfe<E>::mul(v, ar, ai);
      if (!beta_zero) r = mfe<E>::add(r, mfe<E>::mul(y[k], br, bi));
      y[k] = r;
    }
  }
}
// x = beta x over all N elements (beta_zero: x = 0, x is not read): the first half of the adjoint
template <typename E>
__global__ __launch_bounds__(MF_THREADS) void sampling_scale_kernel(E* __restrict__ x, int64_t n, typename mfe<E>::R br, typename mfe<E>::R bi,
                                                                    int beta_zero) {
  for (int64_t i = (int64_t)blockIdx.x * MF_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * MF_THREADS)
    x[i] = beta_zero ? mfe<E>::zero() : mfe<E>::mul(x[i], br, bi);
}
// x[idx[k]] (+)= alpha y[k]: unique indices, every element written by one thread (PLAIN: x[idx[k]] = y[k]; ACC: on top of beta x)
template <typename E, bool PLAIN, bool ACC>
__global__ __launch_bounds__(MF_THREADS) void sampling_scatter_kernel(const int32_t* __restrict__ idx, const E* __restrict__ y, E* __restrict__ x,
                                                                      int64_t m, typename mfe<E>::R ar, typename mfe<E>::R ai) {
  for (int64_t k = (int64_t)blockIdx.x * MF_THREADS + threadIdx.x; k < m; k += (int64_t)gridDim.x * MF_THREADS) {
    const int32_t i = idx[k];
    if constexpr (PLAIN) {
      x[i] = y[k];
    } else {
      const E r = mfe<E>::mul(y[k], ar, ai);
      x[i] = ACC ? mfe<E>::add(x[i], r) : r;
    }
  }
}
template <typename R>
__global__ __launch_bounds__(MF_THREADS) void sampling_mask_build_kernel(const int32_t* __restrict__ idx, R* __restrict__ mask, int64_t m) {
  for (int64_t k = (int64_t)blockIdx.x * MF_THREADS + threadIdx.x; k < m; k += (int64_t)gridDim.x * MF_THREADS) mask[idx[k]] = (R)1;
}
// v = mask .* p (p may be v)
template <typename E>
__global__ __launch_bounds__(MF_THREADS) void sampling_mask_kernel(const typename mfe<E>::R* __restrict__ mask, const E* p, E* v, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * MF_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * MF_THREADS)
    v[i] = mfe<E>::rmul(p[i], mask[i]);
}

// ---- FFT: the line routine both paths call -------------------------------------------------------------------------------------------
__device__ static inline int fft_rev(int k, int lgn) { return lgn ? (int)(__brev((unsigned)k) >> (32 - lgn)) : 0; }

// One radix-2 stage of half-span h = 2^lgh on 2^lgnl lines of n = 2^lgn points in LDS, a thread per butterfly.
// CONTIG: point k of line l at s[l n + k], consecutive lanes on consecutive butterflies of a line (used for h >= 64 only);
// else:   point k of line l at s[k nl + l], consecutive lanes on consecutive lines of one butterfly.
// tw[j << lgtw] = exp(-2 pi i j / n), j < n / 2.
template <typename E, bool INV, bool CONTIG>
__device__ static inline void fft_stage_lds(E* s, int lgn, int lgnl, int lgh, const E* __restrict__ tw, int lgtw) {
  const int h = 1 << lgh, total = 1 << (lgn - 1 + lgnl);
  for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
    int l, b;
    if constexpr (CONTIG) {
      l = idx >> (lgn - 1);
      b = idx & ((1 << (lgn - 1)) - 1);
    } else {
      b = idx >> lgnl;
      l = idx & ((1 << lgnl) - 1);
    }
    const int p = b & (h - 1);
    const int i = ((b - p) << 1) + p;  // the butterfly's lower point
    E* pa = CONTIG ? s + (l << lgn) + i : s + (i << lgnl) + l;
    E* pb = CONTIG ? pa + h : pa + (h << lgnl);
    const E w = tw[(p << (lgn - 1 - lgh)) << lgtw];
    const E a = *pa, u = *pb;
    if constexpr (!INV) {
      *pa = mfe<E>::add(a, u);
      *pb = mfe<E>::mul(mfe<E>::sub(a, u), w.x, w.y);
    } else {
      const E t = mfe<E>::mulc(u, w);
      *pa = mfe<E>::add(a, t);
      *pb = mfe<E>::sub(a, t);
    }
  }
}

// The stages of half-span < 64 of contiguous lines: `total` consecutive points (whole lines), a lane per point, the partner's point
// from lane ^ h.  The workgroup is a whole number of waves and every 64-point block is aligned, so lane = point mod 64.
template <typename E, bool INV>
__device__ static inline void fft_tail_wave(E* s, int lgn, int total, const E* __restrict__ tw, int lgtw) {
  const int lgw = lgn < 6 ? lgn : 6;
  for (int e = threadIdx.x; e < total; e += blockDim.x) {
    E v = s[e];
    const int k = e & ((1 << lgn) - 1);
    for (int q = 0; q < lgw; ++q) {
      const int lgh = INV ? q : lgw - 1 - q, h = 1 << lgh;
      const E o = mfe<E>::xchg(v, h);
      const bool up = (k & h) != 0;
      const E w = tw[((k & (h - 1)) << (lgn - 1 - lgh)) << lgtw];
      const E a = up ? o : v, u = up ? v : o;
      if constexpr (!INV) {
        const E lo = mfe<E>::add(a, u), hi = mfe<E>::mul(mfe<E>::sub(a, u), w.x, w.y);
        v = up ? hi : lo;
      } else {
        const E t = mfe<E>::mulc(u, w);
        const E lo = mfe<E>::add(a, t), hi = mfe<E>::sub(a, t);
        v = up ? hi : lo;
      }
    }
    s[e] = v;
  }
}

// All stages of 2^lgnl lines of 2^lgn points, in place; the caller has synchronised the workgroup, and so has this on return.
template <typename E, bool INV, bool CONTIG>
__device__ static inline void fft_lines(E* s, int lgn, int lgnl, const E* __restrict__ tw, int lgtw) {
  if (lgn == 0) return;
  const int lgw = CONTIG ? (lgn < 6 ? lgn : 6) : 0;  // stages of half-span < 2^lgw run in the waves
  if constexpr (!INV) {
    for (int lgh = lgn - 1; lgh >= lgw; --lgh) {
      fft_stage_lds<E, false, CONTIG>(s, lgn, lgnl, lgh, tw, lgtw);
      __syncthreads();
    }
    if constexpr (CONTIG) {
      fft_tail_wave<E, false>(s, lgn, 1 << (lgn + lgnl), tw, lgtw);
      __syncthreads();
    }
  } else {
    if constexpr (CONTIG) {
      fft_tail_wave<E, true>(s, lgn, 1 << (lgn + lgnl), tw, lgtw);
      __syncthreads();
    }
    for (int lgh = lgw; lgh < lgn; ++lgh) {
      fft_stage_lds<E, true, CONTIG>(s, lgn, lgnl, lgh, tw, lgtw);
      __syncthreads();
    }
  }
}

// the shifts of one dimension as signs: (-1)^k on the way in and out, and (-1)^(n/2) -- a minus for n = 2 only -- on the forward's
// way out and the adjoint's way in (so that the two cancel between a forward and an adjoint)
__device__ static inline bool fft_neg(int k, int lgn, bool global_side) { return ((k & 1) != 0) != (global_side && lgn == 1); }

// ---- general path: one dimension of the image per launch.  DIM1 = false: bundles of 2^lgb contiguous lines along dimension 0;
// DIM1 = true: bundles of 2^lgb neighbouring lines along dimension 1 (a strided load, 2^lgb consecutive elements per stride).
// The shift signs of BOTH dimensions go into the load of the transform's `first` pass and into the store of its `last`, where the
// single-workgroup kernel has them: a sign moved across a pass changes the sign of the exact zeros that cancellation leaves
// (x - x = +0 whatever the sign in front), and the two paths are to give the same bits.
// scale multiplies in the store when `last`; mask_at 1: the load is multiplied by the mask, 2: the store (behind the scale).
template <typename E, bool INV, bool DIM1>
__global__ __launch_bounds__(FFT_THREADS) void fft_pass_kernel(const E* src, E* dst, int lg1, int lg2, int lgb, const E* __restrict__ tw, int lgtw,
                                                               int shift, int first, int last, typename mfe<E>::R scale,
                                                               const typename mfe<E>::R* __restrict__ mask, int mask_at) {
  extern __shared__ __align__(16) unsigned char fft_smem[];
  E* s = reinterpret_cast<E*>(fft_smem);
  const int lgn = DIM1 ? lg2 : lg1, lgo = DIM1 ? lg1 : lg2, n = 1 << lgn, B = 1 << lgb;
  const int nb = 1 << ((DIM1 ? lg1 : lg2) - lgb), cnt = 1 << (lgn + lgb);
  for (int bundle = blockIdx.x; bundle < nb; bundle += gridDim.x) {
    for (int idx = threadIdx.x; idx < cnt; idx += blockDim.x) {
      int k, l, pos;
      int64_t g;
      if constexpr (DIM1) {
        l = idx & (B - 1), k = idx >> lgb;
        g = (int64_t)(bundle * B + l) + ((int64_t)k << lg1);
        pos = ((INV ? fft_rev(k, lgn) : k) << lgb) + l;
      } else {
        k = idx & (n - 1), l = idx >> lgn;
        g = ((int64_t)(bundle * B + l) << lg1) + k;
        pos = (l << lgn) + (INV ? fft_rev(k, lgn) : k);
      }
      E v = src[g];
      if (mask_at == 1) v = mfe<E>::rmul(v, mask[g]);
      if (shift && first && (fft_neg(k, lgn, INV) != fft_neg(bundle * B + l, lgo, INV))) v = mfe<E>::neg(v);
      s[pos] = v;
    }
    __syncthreads();
    fft_lines<E, INV, !DIM1>(s, lgn, lgb, tw, lgtw);
    for (int idx = threadIdx.x; idx < cnt; idx += blockDim.x) {
      int k, l, pos;
      int64_t g;
      if constexpr (DIM1) {
        l = idx & (B - 1), k = idx >> lgb;
        g = (int64_t)(bundle * B + l) + ((int64_t)k << lg1);
        pos = ((INV ? k : fft_rev(k, lgn)) << lgb) + l;
      } else {
        k = idx & (n - 1), l = idx >> lgn;
        g = ((int64_t)(bundle * B + l) << lg1) + k;
        pos = (l << lgn) + (INV ? k : fft_rev(k, lgn));
      }
      E v = s[pos];
      if (shift && last && (fft_neg(k, lgn, !INV) != fft_neg(bundle * B + l, lgo, !INV))) v = mfe<E>::neg(v);
      if (last) v = mfe<E>::rmul(v, scale);
      if (mask_at == 2) v = mfe<E>::rmul(v, mask[g]);
      dst[g] = v;
    }
    __syncthreads();
  }
}

// ---- single-workgroup path: y = F x (FFT_FWD), F^H x (FFT_INV) or F^H diag(mask) F x (all three); x may be y.  Dynamic LDS: the image.
template <typename E>
__global__ __launch_bounds__(FFT_THREADS) void fft_fused_kernel(const E* x, E* y, int lg1, int lg2, int mode, const E* __restrict__ tw, int lgtw1,
                                                                int lgtw2, int shift, typename mfe<E>::R scale,
                                                                const typename mfe<E>::R* __restrict__ mask) {
  extern __shared__ __align__(16) unsigned char fft_smem[];
  E* s = reinterpret_cast<E*>(fft_smem);
  const int n1 = 1 << lg1, N = 1 << (lg1 + lg2);
  const bool fwd = (mode & FFT_FWD) != 0, inv = (mode & FFT_INV) != 0;
  for (int idx = threadIdx.x; idx < N; idx += blockDim.x) {
    const int k1 = idx & (n1 - 1), k2 = idx >> lg1;
    E v = x[idx];
    if (shift && (fft_neg(k1, lg1, !fwd) != fft_neg(k2, lg2, !fwd))) v = mfe<E>::neg(v);
    s[fwd ? idx : fft_rev(k1, lg1) + (fft_rev(k2, lg2) << lg1)] = v;
  }
  __syncthreads();
  if (fwd) {
    fft_lines<E, false, true>(s, lg1, lg2, tw, lgtw1);
    fft_lines<E, false, false>(s, lg2, lg1, tw, lgtw2);
  }
  if (mode & FFT_MASK) {
    // (the forward's signs on the way out and the adjoint's on the way in cancel: neither is applied)
    for (int pos = threadIdx.x; pos < N; pos += blockDim.x) {
      const int g = fft_rev(pos & (n1 - 1), lg1) + (fft_rev(pos >> lg1, lg2) << lg1);
      s[pos] = mfe<E>::rmul(mfe<E>::rmul(s[pos], scale), mask[g]);
    }
    __syncthreads();
  }
  if (inv) {
    fft_lines<E, true, false>(s, lg2, lg1, tw, lgtw2);
    fft_lines<E, true, true>(s, lg1, lg2, tw, lgtw1);
  }
  for (int idx = threadIdx.x; idx < N; idx += blockDim.x) {
    const int k1 = idx & (n1 - 1), k2 = idx >> lg1;
    E v = s[inv ? idx : fft_rev(k1, lg1) + (fft_rev(k2, lg2) << lg1)];
    if (shift && (fft_neg(k1, lg1, !inv) != fft_neg(k2, lg2, !inv))) v = mfe<E>::neg(v);
    y[idx] = mfe<E>::rmul(v, scale);
  }
}

template <typename F>
static inline int32_t mf_dispatch(int32_t dtype, F&& fn) {
  if (dtype == RLS_F64 || dtype == RLS_C64) return rls_with_elem64(dtype, fn);
  return rls_with_elem(dtype, fn);
}
template <typename F>
static inline int32_t fft_dispatch(int32_t dtype, F&& fn) {
  if (dtype == RLS_C64) return fn(rls_type<double2>{});
  return fn(rls_type<float2>{});
}

}  // namespace

struct rls_sampling {
  rls_ctx* ctx = nullptr;
  uint64_t ctx_id = 0;
  int32_t dtype = RLS_F32;
  int64_t N = 0, m = 0;
  int32_t* idx = nullptr;  // m indices, device
  void* mask = nullptr;    // N values 0 / 1 of the element's real type, device
};

struct rls_fft {
  rls_ctx* ctx = nullptr;
  uint64_t ctx_id = 0;
  int32_t dtype = RLS_C32;
  int lg1 = 0, lg2 = 0;  // the transformed extents 2^lg1 x 2^lg2 (unit dimensions dropped; lg2 = 0: a signal)
  int shift = 1, unitary = 1;
  int lgmax = 0;         // the table serves 2^lgmax points: tw[j] = exp(-2 pi i j / 2^lgmax), j < max(2^lgmax / 2, 1)
  void* tw = nullptr;
  void* tmp = nullptr;   // the image between F and S in rls_fft_sampled_mul
};

namespace {

static bool samp_live(const rls_sampling* s) { return s && rls_ctx_alive(s->ctx, s->ctx_id); }
static bool fft_live(const rls_fft* f) { return f && rls_ctx_alive(f->ctx, f->ctx_id); }

static double fft_scale(const rls_fft* f) { return f->unitary ? 1.0 / std::sqrt((double)((int64_t)1 << (f->lg1 + f->lg2))) : 1.0; }
static bool fft_fused_fits(const rls_fft* f) { return ((size_t)1 << (f->lg1 + f->lg2)) * mf_elem_size(f->dtype) <= FFT_FUSED_LDS; }
// THE choice between the two paths.  "fft_fused" = 1 (default): the single-workgroup kernel for images of up to FFT_FUSED_AUTO_N points
// -- beyond that one CU loses to the general path's one or two chip-wide launches (profiles/matfree.txt); 2: whenever the image
// fits the LDS; 0: never.
static bool fft_use_fused(const rls_fft* f) {
  const int t = f->ctx->tune.fft_fused;
  if (t == 0 || !fft_fused_fits(f)) return false;
  return t >= 2 || ((int64_t)1 << (f->lg1 + f->lg2)) <= FFT_FUSED_AUTO_N;
}

static int32_t fft_fused_launch(rls_fft* f, const void* x, void* y, int mode, const void* mask) {
  rls_ctx* ctx = f->ctx;
  const size_t N = (size_t)1 << (f->lg1 + f->lg2);
  const unsigned nt = N <= 2048 ? 256 : FFT_THREADS;
  return fft_dispatch(f->dtype, [&](auto t) -> int32_t {
    using E = typename decltype(t)::type;
    using R = typename mfe<E>::R;
    const hipError_t e = rls_allow_lds<fft_fused_kernel<E>>(ctx->device, FFT_FUSED_LDS);
    if (e != hipSuccess) return rls_fail(ctx, (int32_t)e, "hipFuncSetAttribute (dynamic LDS) failed");
    hipLaunchKernelGGL((fft_fused_kernel<E>), dim3(1), dim3(nt), N * sizeof(E), ctx->stream, (const E*)x, (E*)y, f->lg1, f->lg2, mode,
                       (const E*)f->tw, f->lgmax - f->lg1, f->lgmax - f->lg2, f->shift, (R)fft_scale(f), (const R*)mask);
    return launch_status(ctx);
  });
}

// one dimension on the general path
static int32_t fft_pass(rls_fft* f, bool inv, bool dim1, const void* src, void* dst, bool first, bool last, const void* mask, int mask_at) {
  rls_ctx* ctx = f->ctx;
  const int lgn = dim1 ? f->lg2 : f->lg1, lgo = dim1 ? f->lg1 : f->lg2;
  return fft_dispatch(f->dtype, [&](auto t) -> int32_t {
    using E = typename decltype(t)::type;
    using R = typename mfe<E>::R;
    // lines per workgroup: 2^FFT_LG_BUNDLE points where the lines are short, at least 8 neighbouring lines along dimension 1 (64 contiguous
    // bytes per stride), never more than the LDS holds or the image has
    int lgb = FFT_LG_BUNDLE - lgn < 0 ? 0 : FFT_LG_BUNDLE - lgn;
    if (dim1 && lgb < 3) lgb = 3;
    if (lgb > lgo) lgb = lgo;
    while (lgb > 0 && ((size_t)sizeof(E) << (lgn + lgb)) > FFT_LINE_LDS) --lgb;
    const size_t cnt = (size_t)1 << (lgn + lgb);
    unsigned nt = (unsigned)(cnt / 2 < 64 ? 64 : (cnt / 2 > FFT_THREADS ? FFT_THREADS : cnt / 2));
    const int nb = 1 << (lgo - lgb);
    const unsigned grid = (unsigned)(nb > 4096 ? 4096 : nb);
    return with_bool(inv, [&](auto iv) {
      return with_bool(dim1, [&](auto d1) -> int32_t {
        constexpr bool INV = decltype(iv)::value, DIM1 = decltype(d1)::value;
        const hipError_t e = rls_allow_lds<fft_pass_kernel<E, INV, DIM1>>(ctx->device, FFT_LINE_LDS);
        if (e != hipSuccess) return rls_fail(ctx, (int32_t)e, "hipFuncSetAttribute (dynamic LDS) failed");
        hipLaunchKernelGGL((fft_pass_kernel<E, INV, DIM1>), dim3(grid), dim3(nt), cnt * sizeof(E), ctx->stream, (const E*)src, (E*)dst, f->lg1,
                           f->lg2, lgb, (const E*)f->tw, f->lgmax - lgn, f->shift, first ? 1 : 0, last ? 1 : 0, (R)fft_scale(f), (const R*)mask, mask_at);
        return launch_status(ctx);
      });
    });
  });
}

// y = F x or F^H x on the general path (a signal: one launch, an image: two); mask (may be null) multiplies the forward's last store
// or the adjoint's first load
static int32_t fft_general(rls_fft* f, bool adjoint, const void* x, void* y, const void* mask) {
  const bool img = f->lg2 > 0;
  if (!adjoint) {
    RLS_TRY(fft_pass(f, false, false, x, y, true, !img, img ? nullptr : mask, !img && mask ? 2 : 0));
    if (img) RLS_TRY(fft_pass(f, false, true, y, y, false, true, mask, mask ? 2 : 0));
  } else {
    if (img) RLS_TRY(fft_pass(f, true, true, x, y, true, false, mask, mask ? 1 : 0));
    RLS_TRY(fft_pass(f, true, false, img ? y : x, y, !img, true, img ? nullptr : mask, !img && mask ? 1 : 0));
  }
  return 0;
}

static int32_t fft_run(rls_fft* f, bool adjoint, const void* x, void* y) {
  if (fft_use_fused(f)) return fft_fused_launch(f, x, y, adjoint ? FFT_INV : FFT_FWD, nullptr);
  return fft_general(f, adjoint, x, y, nullptr);
}

static int32_t samp_mul(rls_sampling* s, int32_t op, double ar, double ai, const void* x, double br, double bi, void* y) {
  rls_ctx* ctx = s->ctx;
  const int beta_zero = br == 0.0 && bi == 0.0;
  const bool plain = ar == 1.0 && ai == 0.0 && beta_zero;
  return mf_dispatch(s->dtype, [&](auto t) -> int32_t {
    using E = typename decltype(t)::type;
    using R = typename mfe<E>::R;
    return with_bool(plain, [&](auto pl) -> int32_t {
      constexpr bool PLAIN = decltype(pl)::value;
      if (op == RLS_OP_N)
        return rls_launch<sampling_gather_kernel<E, PLAIN>>(ctx, dim3(mf_grid(s->m)), dim3(MF_THREADS), 0, (const int32_t*)s->idx, (const E*)x,
                                                            (E*)y, s->m, (R)ar, (R)ai, (R)br, (R)bi, beta_zero);
      // the transpose and the adjoint of a real 0 / 1 matrix are one: y (length N) = beta y, then the m sampled elements on top
      RLS_TRY((rls_launch<sampling_scale_kernel<E>>(ctx, dim3(mf_grid(s->N)), dim3(MF_THREADS), 0, (E*)y, s->N, (R)br, (R)bi, beta_zero)));
      if (beta_zero)
        return rls_launch<sampling_scatter_kernel<E, PLAIN, false>>(ctx, dim3(mf_grid(s->m)), dim3(MF_THREADS), 0, (const int32_t*)s->idx,
                                                                    (const E*)x, (E*)y, s->m, (R)ar, (R)ai);
      return rls_launch<sampling_scatter_kernel<E, false, true>>(ctx, dim3(mf_grid(s->m)), dim3(MF_THREADS), 0, (const int32_t*)s->idx,
                                                                 (const E*)x, (E*)y, s->m, (R)ar, (R)ai);
    });
  });
}

static bool fft_pairs(const rls_fft* f, const rls_sampling* s) {
  return fft_live(f) && samp_live(s) && f->ctx == s->ctx && f->dtype == s->dtype && s->N == ((int64_t)1 << (f->lg1 + f->lg2));
}

}  // namespace

extern "C" {

int32_t rls_sampling_create(rls_ctx* ctx, int32_t dtype, int64_t N, int64_t m, const int32_t* idx_host, rls_sampling** out) {
  RLS_CHECK_CTX(ctx);
  if (!out) return rls_fail(ctx, RLS_E_INVALID, "sampling_create: null out");
  *out = nullptr;
  if (dtype < RLS_F32 || dtype > RLS_C64 || N < 1 || N >= ((int64_t)1 << 31) || m < 1 || m > N || !idx_host)
    return rls_fail(ctx, RLS_E_INVALID, "sampling_create: bad argument (1 <= m <= N < 2^31)");
  {  // on the host, before anything is uploaded: every index inside [0, N), none twice
    std::vector<bool> seen((size_t)N, false);
    for (int64_t k = 0; k < m; ++k) {
      const int64_t i = idx_host[k];
      if (i < 0 || i >= N) return rls_fail(ctx, RLS_E_INVALID, "sampling_create: an index lies outside [0, N)");
      if (seen[(size_t)i]) return rls_fail(ctx, RLS_E_INVALID, "sampling_create: an index is repeated");
      seen[(size_t)i] = true;
    }
  }
  RLS_HIP(ctx, rls_enter(ctx));
  rls_sampling* s = new rls_sampling();
  s->ctx = ctx;
  s->ctx_id = ctx->id;
  s->dtype = dtype;
  s->N = N;
  s->m = m;
  const bool dbl = dtype == RLS_F64 || dtype == RLS_C64;
  const size_t mb = (size_t)N * (dbl ? 8 : 4);
  hipError_t e = rls_dev_alloc(ctx, (void**)&s->idx, (size_t)m * 4);
  if (e == hipSuccess) e = rls_dev_alloc(ctx, &s->mask, mb);
  if (e != hipSuccess) {
    rls_sampling_destroy(s);
    return rls_fail(ctx, RLS_E_WORKSPACE, "sampling_create: allocation failed");
  }
  e = hipMemcpyAsync(s->idx, idx_host, (size_t)m * 4, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(s->mask, 0, mb, ctx->stream);
  int32_t st = 0;
  if (e == hipSuccess) {  // the mask is built on the device, once
    if (dbl) st = rls_launch<sampling_mask_build_kernel<double>>(ctx, dim3(mf_grid(m)), dim3(MF_THREADS), 0, (const int32_t*)s->idx, (double*)s->mask, m);
    else st = rls_launch<sampling_mask_build_kernel<float>>(ctx, dim3(mf_grid(m)), dim3(MF_THREADS), 0, (const int32_t*)s->idx, (float*)s->mask, m);
  }
  if (e == hipSuccess && st == 0) e = rls_stream_wait(ctx->stream);  // the caller's index array is free on return
  if (e != hipSuccess || st != 0) {
    rls_sampling_destroy(s);
    return st != 0 ? st : rls_fail(ctx, (int32_t)e, "sampling_create: upload failed");
  }
  *out = s;
  return 0;
}

int32_t rls_sampling_destroy(rls_sampling* s) {
  if (!s) return RLS_E_INVALID;
  rls_ctx* ctx = samp_live(s) ? s->ctx : nullptr;
  if (s->idx) rls_dev_free(ctx, s->idx);
  if (s->mask) rls_dev_free(ctx, s->mask);
  delete s;
  return 0;
}

int32_t rls_sampling_mul(rls_sampling* s, int32_t op, double alpha_re, double alpha_im, const void* x, double beta_re, double beta_im, void* y) {
  if (!samp_live(s)) return RLS_E_INVALID;
  rls_ctx* ctx = s->ctx;
  if (!x || !y || x == y || op < RLS_OP_N || op > RLS_OP_C) return rls_fail(ctx, RLS_E_INVALID, "sampling_mul: bad argument");
  RLS_HIP(ctx, rls_enter(ctx));
  return samp_mul(s, op, alpha_re, alpha_im, x, beta_re, beta_im, y);
}

int32_t rls_sampling_mul_normal(rls_sampling* s, const void* p, void* v) {
  if (!samp_live(s)) return RLS_E_INVALID;
  rls_ctx* ctx = s->ctx;
  if (!p || !v) return rls_fail(ctx, RLS_E_INVALID, "sampling_mul_normal: null pointer");
  RLS_HIP(ctx, rls_enter(ctx));
  return mf_dispatch(s->dtype, [&](auto t) -> int32_t {
    using E = typename decltype(t)::type;
    return rls_launch<sampling_mask_kernel<E>>(ctx, dim3(mf_grid(s->N)), dim3(MF_THREADS), 0, (const typename mfe<E>::R*)s->mask, (const E*)p,
                                               (E*)v, s->N);
  });
}

int32_t rls_fft_create(rls_ctx* ctx, int32_t dtype, int32_t ndims, const int64_t* shape, int32_t flags, rls_fft** out) {
  RLS_CHECK_CTX(ctx);
  if (!out) return rls_fail(ctx, RLS_E_INVALID, "fft_create: null out");
  *out = nullptr;
  if ((dtype != RLS_C32 && dtype != RLS_C64) || ndims < 1 || !shape || (flags & ~(RLS_FFT_SHIFT | RLS_FFT_UNITARY)))
    return rls_fail(ctx, RLS_E_INVALID, "fft_create: bad argument (complex element types only)");
  const int64_t max_line = (int64_t)(FFT_LINE_LDS / mf_elem_size(dtype));
  int lg[2] = {0, 0}, nd = 0;
  for (int k = 0; k < ndims; ++k) {
    if (shape[k] < 1) return rls_fail(ctx, RLS_E_INVALID, "fft_create: extents must be positive");
    if (shape[k] == 1) continue;  // unit dimensions are dropped
    if (nd == 2) return rls_fail(ctx, RLS_E_UNSUPPORTED, "fft_create: 1-D and 2-D shapes only");
    if (shape[k] & (shape[k] - 1)) return rls_fail(ctx, RLS_E_UNSUPPORTED, "fft_create: extents must be powers of two");
    if (shape[k] > max_line) return rls_fail(ctx, RLS_E_UNSUPPORTED, "fft_create: a line is longer than 8192 (ComplexF32) / 4096 (ComplexF64) points");
    int l = 0;
    while (((int64_t)1 << l) < shape[k]) ++l;
    lg[nd++] = l;
  }
  RLS_HIP(ctx, rls_enter(ctx));
  rls_fft* f = new rls_fft();
  f->ctx = ctx;
  f->ctx_id = ctx->id;
  f->dtype = dtype;
  f->lg1 = lg[0];
  f->lg2 = lg[1];
  f->shift = (flags & RLS_FFT_SHIFT) ? 1 : 0;
  f->unitary = (flags & RLS_FFT_UNITARY) ? 1 : 0;
  f->lgmax = lg[0] > lg[1] ? lg[0] : lg[1];
  // the twiddle table, in double on the host, rounded once to the element's real type
  const size_t nt = f->lgmax > 0 ? (size_t)1 << (f->lgmax - 1) : 1, es = mf_elem_size(dtype);
  const double nmax = (double)((int64_t)1 << f->lgmax);
  std::vector<double> td(2 * nt);
  std::vector<float> tf(dtype == RLS_C32 ? 2 * nt : 0);
  for (size_t j = 0; j < nt; ++j) {
    const double a = -2.0 * M_PI * (double)j / nmax;
    td[2 * j] = std::cos(a);
    td[2 * j + 1] = std::sin(a);
  }
  td[0] = 1.0, td[1] = 0.0;
  if (nt >= 2) td[nt] = 0.0, td[nt + 1] = -1.0;  // j = n / 4: exactly -i
  for (size_t j = 0; j < tf.size(); ++j) tf[j] = (float)td[j];
  hipError_t e = rls_dev_alloc(ctx, &f->tw, nt * es);
  if (e == hipSuccess) e = rls_dev_alloc(ctx, &f->tmp, es << (f->lg1 + f->lg2));
  if (e != hipSuccess) {
    rls_fft_destroy(f);
    return rls_fail(ctx, RLS_E_WORKSPACE, "fft_create: allocation failed");
  }
  e = hipMemcpyAsync(f->tw, dtype == RLS_C32 ? (const void*)tf.data() : (const void*)td.data(), nt * es, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = rls_stream_wait(ctx->stream);  // (the host table goes out of scope)
  if (e != hipSuccess) {
    rls_fft_destroy(f);
    return rls_fail(ctx, (int32_t)e, "fft_create: upload failed");
  }
  *out = f;
  return 0;
}

int32_t rls_fft_destroy(rls_fft* f) {
  if (!f) return RLS_E_INVALID;
  rls_ctx* ctx = fft_live(f) ? f->ctx : nullptr;
  if (f->tw) rls_dev_free(ctx, f->tw);
  if (f->tmp) rls_dev_free(ctx, f->tmp);
  delete f;
  return 0;
}

int32_t rls_fft_variant(rls_fft* f, int32_t* out) {
  if (!fft_live(f) || !out) return RLS_E_INVALID;
  *out = fft_use_fused(f) ? 1 : 0;
  return 0;
}

int32_t rls_fft_apply(rls_fft* f, int32_t adjoint, const void* x, void* y) {
  if (!fft_live(f)) return RLS_E_INVALID;
  rls_ctx* ctx = f->ctx;
  if (!x || !y || (adjoint != 0 && adjoint != 1)) return rls_fail(ctx, RLS_E_INVALID, "fft_apply: bad argument");
  RLS_HIP(ctx, rls_enter(ctx));
  return fft_run(f, adjoint != 0, x, y);
}

int32_t rls_fft_sampled_mul(rls_fft* f, rls_sampling* s, int32_t op, const void* x, void* y) {
  if (!fft_live(f) || !samp_live(s)) return RLS_E_INVALID;
  rls_ctx* ctx = f->ctx;
  if (!fft_pairs(f, s)) return rls_fail(ctx, RLS_E_INVALID, "fft_sampled_mul: the two operators differ in context, element type or size");
  if (!x || !y || x == y) return rls_fail(ctx, RLS_E_INVALID, "fft_sampled_mul: bad argument");
  if (op == RLS_OP_T) return rls_fail(ctx, RLS_E_UNSUPPORTED, "fft_sampled_mul: the product and its adjoint only (RLS_OP_N, RLS_OP_C)");
  if (op != RLS_OP_N && op != RLS_OP_C) return rls_fail(ctx, RLS_E_INVALID, "fft_sampled_mul: bad op");
  RLS_HIP(ctx, rls_enter(ctx));
  if (op == RLS_OP_N) {  // y = S (F x)
    RLS_TRY(fft_run(f, false, x, f->tmp));
    return samp_mul(s, RLS_OP_N, 1.0, 0.0, f->tmp, 0.0, 0.0, y);
  }
  RLS_TRY(samp_mul(s, RLS_OP_C, 1.0, 0.0, x, 0.0, 0.0, f->tmp));  // y = F^H (S^H x)
  return fft_run(f, true, f->tmp, y);
}

int32_t rls_fft_sampled_mul_normal(rls_fft* f, rls_sampling* s, const void* p, void* v) {
  if (!fft_live(f) || !samp_live(s)) return RLS_E_INVALID;
  rls_ctx* ctx = f->ctx;
  if (!fft_pairs(f, s)) return rls_fail(ctx, RLS_E_INVALID, "fft_sampled_mul_normal: the two operators differ in context, element type or size");
  if (!p || !v) return rls_fail(ctx, RLS_E_INVALID, "fft_sampled_mul_normal: null pointer");
  RLS_HIP(ctx, rls_enter(ctx));
  if (fft_use_fused(f)) return fft_fused_launch(f, p, v, FFT_FWD | FFT_MASK | FFT_INV, s->mask);
  RLS_TRY(fft_general(f, false, p, v, s->mask));  // the mask rides in the store of the last forward pass
  return fft_general(f, true, v, v, nullptr);
}

}  // extern "C"
