// Wavefront-level dense linear algebra for one parameter draw (gfx950 / CDNA4).
//
// Execution model used by every kernel in this directory: ONE 64-lane wavefront owns ONE
// draw.  The workgroup is exactly one wave, so `__syncthreads()` is a wave-local LDS fence
// (no cross-wave barrier traffic).  Matrices of the draw live in LDS, row-major, zero-padded
// to NP = 8*BS rows/cols with an ODD leading dimension (LD = NP|1) so that both access
// patterns of the register-blocked product below are bank-conflict free for ds_read_b64:
//   - lanes form an 8x8 grid (lr = lane>>3, lc = lane&7); lane (lr,lc) owns the BSxBS block
//     of rows lr*BS.. and columns lc*BS.. of every n x n result and keeps it in VGPRs;
//   - a product C += A*B walks k and needs A[lr*BS+i][k] (8 distinct addresses per
//     instruction, broadcast over lc) and B[k][lc*BS+j] (8 distinct, broadcast over lr):
//     2*BS LDS reads feed BS*BS fp64 FMAs.
// FP64 FMA on the VALU runs at the same rate as v_mfma_f64_16x16x4 on gfx950, and an
// 8x8 lane grid tiles n = 40 with no padding waste (MFMA 16x16 tiles would pad 40 -> 48).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "dsge_filter_conv.hpp"

namespace dsge {

template <int BS>
struct Tile {
  static constexpr int NP = 8 * BS;
  static constexpr int LD = NP | 1;
};

// internal per-draw status value: "a structure-exploiting kernel could not take this draw; the general
// kernel must".  Never returned to the caller.
constexpr int32_t DSGE_ST_INTERNAL_RERUN = 1 << 30;

__device__ __forceinline__ void wave_sync() { __syncthreads(); }

// Second passes of the kernel cascades visit only the draws an earlier kernel flagged DSGE_ST_INTERNAL_RERUN -- normally
// none.  True if none of the draws this workgroup would visit (indices blockIdx.x + i gridDim.x, through `order` if
// given) carries the flag: ONE parallel load per 64 draws instead of a dependent load per draw, so that an empty pass
// costs its launch and little else.
__device__ __forceinline__ bool rerun_pass_is_empty(const int32_t* __restrict__ status, int batch,
                                                    const int32_t* __restrict__ order = nullptr) {
  const int lane = threadIdx.x & 63;
  bool any = false;
  for (int b0 = blockIdx.x; b0 < batch; b0 += 64 * gridDim.x) {
    const int bi = b0 + lane * gridDim.x;
    if (bi < batch) any = any || ((status[order ? order[bi] : bi] & DSGE_ST_INTERNAL_RERUN) != 0);
  }
  return __ballot(any) == 0ull;
}

// NaN-propagating max (np.max semantics, used by the induced 1-norm)
__device__ __forceinline__ double nanmax(double a, double b) { return (a > b || a != a) ? a : b; }

__device__ __forceinline__ double shfl_xor_f64(double v, int mask) { return __shfl_xor(v, mask, 64); }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += shfl_xor_f64(v, m);
  return v;
}
__device__ __forceinline__ double wave_nanmax(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = nanmax(v, shfl_xor_f64(v, m));
  return v;
}

template <int BS>
__device__ __forceinline__ void blk_zero(double (&x)[BS][BS]) {
#pragma unroll
  for (int i = 0; i < BS; ++i)
#pragma unroll
    for (int j = 0; j < BS; ++j) x[i][j] = 0.0;
}

// register block <- global row-major [n][ldg] matrix (zero outside n x ncols)
template <int BS>
__device__ __forceinline__ void blk_load_global(double (&x)[BS][BS], const double* __restrict__ g, int n,
                                                int ncols, int ldg, int lr, int lc) {
  // Unconditional loads from clamped (always valid) addresses, a scheduling barrier, then the selects: a conditional
  // load compiles to its own exec-masked block, and the scheduler, when short of registers, pairs each load with its
  // use -- BS * BS serial round trips to HBM instead of BS * BS loads in flight (32 of them opened the compact
  // cycle-reduction kernel).
#pragma unroll
  for (int i = 0; i < BS; ++i)
#pragma unroll
    for (int j = 0; j < BS; ++j) {
      const int r = lr * BS + i, c = lc * BS + j;
      const int rc = r < n ? r : n - 1, cc = c < ncols ? c : ncols - 1;
      x[i][j] = g[(size_t)rc * ldg + cc];
    }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int i = 0; i < BS; ++i)
#pragma unroll
    for (int j = 0; j < BS; ++j) {
      const int r = lr * BS + i, c = lc * BS + j;
      x[i][j] = (r < n && c < ncols) ? x[i][j] : 0.0;
    }
}

template <int BS>
__device__ __forceinline__ void blk_store_global(const double (&x)[BS][BS], double* __restrict__ g, int n,
                                                 int ncols, int ldg, int lr, int lc, double scale = 1.0) {
#pragma unroll
  for (int i = 0; i < BS; ++i)
#pragma unroll
    for (int j = 0; j < BS; ++j) {
      const int r = lr * BS + i, c = lc * BS + j;
      if (r < n && c < ncols) g[(size_t)r * ldg + c] = scale * x[i][j];
    }
}

template <int BS>
__device__ __forceinline__ void blk_store_lds(const double (&x)[BS][BS], double* s, int ld, int lr, int lc,
                                              double scale = 1.0) {
#pragma unroll
  for (int i = 0; i < BS; ++i)
#pragma unroll
    for (int j = 0; j < BS; ++j) s[(lr * BS + i) * ld + lc * BS + j] = scale * x[i][j];
}

template <int BS>
__device__ __forceinline__ void blk_load_lds(double (&x)[BS][BS], const double* s, int ld, int lr, int lc) {
#pragma unroll
  for (int i = 0; i < BS; ++i)
#pragma unroll
    for (int j = 0; j < BS; ++j) x[i][j] = s[(lr * BS + i) * ld + lc * BS + j];
}

// transposed block read: x[i][j] = s[col-block row][row-block col]  (for sym(X) = (X+X^T)/2)
template <int BS>
__device__ __forceinline__ void blk_load_lds_t(double (&x)[BS][BS], const double* s, int ld, int lr, int lc) {
#pragma unroll
  for (int i = 0; i < BS; ++i)
#pragma unroll
    for (int j = 0; j < BS; ++j) x[i][j] = s[(lc * BS + j) * ld + lr * BS + i];
}

// LDS matrix (NP x LD) <- global [n][ncols] (coalesced), zero padding
__device__ __forceinline__ void lds_load_matrix(double* s, int ld, int np_rows, int np_cols,
                                                const double* __restrict__ g, int n, int ncols, int lane) {
  // eight loads in flight per trip (clamped, unconditional addresses; the selects wait behind a scheduling barrier):
  // the plain loop -- conditional load, store to LDS -- is one round trip to memory per 64 elements
  const int total = np_rows * np_cols;
  for (int base = 0; base < total; base += 8 * 64) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = base + u * 64 + lane;
      const int ic = idx < total ? idx : total - 1;
      const int r = ic / np_cols, c = ic - r * np_cols;
      const int rc = r < n ? r : n - 1, cc = c < ncols ? c : ncols - 1;
      v[u] = g[(size_t)rc * ncols + cc];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = base + u * 64 + lane;
      const int r = idx / np_cols, c = idx - r * np_cols;
      if (idx < total) s[r * ld + c] = (r < n && c < ncols) ? v[u] : 0.0;
    }
  }
}

// Lane-strided loop `for (idx = lane; idx < total; idx += 64) store(idx, load(idx))` with U loads in flight per trip: the
// loads of a trip are issued (from clamped, always valid indices) before the first store waits for one.  The plain loop is
// one round trip to memory per 64 elements.  load: int -> V (any trivially copyable value), store: (int, V) -> void.
template <int U = 8, int NT = 64, class LoadF, class StoreF>
__device__ __forceinline__ void lane_loop_batched(int total, int lane, LoadF load, StoreF store) {
  for (int base = 0; base < total; base += U * NT) {
    decltype(load(0)) v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int idx = base + u * NT + lane;
      v[u] = load(idx < total ? idx : total - 1);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int idx = base + u * NT + lane;
      if (idx < total) store(idx, v[u]);
    }
  }
}

// acc += A(rows lr*BS.., :) * B(:, cols lc*BS..)           (TB = false)
// acc += A(rows lr*BS.., :) * B(rows lc*BS.., :)^T          (TB = true)
template <int BS, bool TB>
__device__ __forceinline__ void mm_acc(double (&acc)[BS][BS], const double* A, int lda, const double* B,
                                       int ldb, int K, int lr, int lc) {
  // Software-pipelined by hand: two operand register sets ping-pong; the LDS loads of step k+1 are
  // issued before the FMAs of step k, and scheduling barriers keep hipcc from sinking them.
  const double* a0p = A + lr * BS * lda;
  const double* b0p = TB ? (B + lc * BS * ldb) : (B + lc * BS);
  double a0[BS], b0[BS], a1[BS], b1[BS];
#define MM_LOAD(a, b, k)                                                              \
  do {                                                                                \
    _Pragma("unroll") for (int i = 0; i < BS; ++i) a[i] = a0p[i * lda + (k)];         \
    _Pragma("unroll") for (int j = 0; j < BS; ++j) b[j] = TB ? b0p[j * ldb + (k)] : b0p[(k)*ldb + j]; \
  } while (0)
#define MM_FMA(a, b)                                                                  \
  do {                                                                                \
    _Pragma("unroll") for (int i = 0; i < BS; ++i)                                    \
      _Pragma("unroll") for (int j = 0; j < BS; ++j) acc[i][j] = fma(a[i], b[j], acc[i][j]); \
  } while (0)
  if (K <= 0) return;
  MM_LOAD(a0, b0, 0);
  int k = 0;
  for (; k + 2 <= K; k += 2) {
    MM_LOAD(a1, b1, k + 1);
    __builtin_amdgcn_sched_barrier(0);
    MM_FMA(a0, b0);
    __builtin_amdgcn_sched_barrier(0);
    const int kn = (k + 2 < K) ? k + 2 : K - 1;
    MM_LOAD(a0, b0, kn);
    __builtin_amdgcn_sched_barrier(0);
    MM_FMA(a1, b1);
    __builtin_amdgcn_sched_barrier(0);
  }
  if (k < K) MM_FMA(a0, b0);
#undef MM_LOAD
#undef MM_FMA
}

// out = R - A(rows lr*BS.., :K) * B(:K, cols lc*BS..) with the inner products in twice the working precision (Dot2 of Ogita,
// Rump & Oishi 2005: every product split exactly by an FMA, every addition by TwoSum, the error terms summed on the side): the
// residual of the refinement step of the cycle-reduction solves.  A residual formed in plain float64 limits one step of
// iterative refinement to the accuracy of a backward-stable solver -- |dX| ~ cond(A1) eps |X|, what LAPACK's LU gives the
// reference --; with this one the corrected X is good to working precision as long as cond(A1) eps << 1, i.e. BETTER than
// the reference's on exactly the draws where two float64 algorithms cannot agree to 1e-9 anyway (tools/cr_accuracy_study.py:
// a 54-variable system with cond(A1) = 2..5e6 and |C| = 3e5, reference 0.8..4.5e-8 from the 40-digit T).  Ten operations per
// term instead of one FMA; only the refined iterations of the flagged draws run it (+0.04 ms on the 0.71 ms solver launch of
// the bench: a refined iteration of the 32-wide tile is two eliminations + 19 k cycles of this).  Tried: a plain first step and
// this one only when the first correction exceeds 1e-11 |X| (the level at which the error reaches 1e-9 in T) -- the refined
// draws of the bench are above that level too and then pay a third elimination: slower.  Contraction is switched off: the
// error-free transformations need p = fl(a b) and t = fl(s + p) as written.
template <int BS>
__device__ __forceinline__ void mm_residual_dot2(double (&out)[BS][BS], const double (&R)[BS][BS], const double* A, int lda,
                                                 const double* B, int ldb, int K, int lr, int lc) {
#pragma clang fp contract(off)
  const double* ap = A + lr * BS * lda;
  const double* bp = B + lc * BS;
  double s[BS][BS], c[BS][BS];
  blk_zero<BS>(s);
  blk_zero<BS>(c);
  for (int k = 0; k < K; ++k) {
    double a[BS], b[BS];
#pragma unroll
    for (int i = 0; i < BS; ++i) a[i] = ap[i * lda + k];
#pragma unroll
    for (int j = 0; j < BS; ++j) b[j] = bp[k * ldb + j];
#pragma unroll
    for (int i = 0; i < BS; ++i)
#pragma unroll
      for (int j = 0; j < BS; ++j) {
        const double p = a[i] * b[j];
        const double e = __builtin_fma(a[i], b[j], -p);  // a b = p + e exactly
        const double t = s[i][j] + p;
        const double z = t - s[i][j];
        const double err = (s[i][j] - (t - z)) + (p - z);  // s + p = t + err exactly
        s[i][j] = t;
        c[i][j] += e + err;
      }
  }
#pragma unroll
  for (int i = 0; i < BS; ++i)
#pragma unroll
    for (int j = 0; j < BS; ++j) out[i][j] = (R[i][j] - s[i][j]) - c[i][j];
}

// acc += A(:, rows lr*BS..)^T * B(:, cols lc*BS..)   i.e. (A' B) with A, B row-major in LDS: both operands are read
// along rows (conflict-free with the odd leading dimension), no transposed copy of A needed.
template <int BS>
__device__ __forceinline__ void mm_acc_ta(double (&acc)[BS][BS], const double* A, int lda, const double* B, int ldb, int K,
                                          int lr, int lc) {
  const double* a0p = A + lr * BS;
  const double* b0p = B + lc * BS;
  for (int k = 0; k < K; ++k) {
    double a[BS], b[BS];
#pragma unroll
    for (int i = 0; i < BS; ++i) a[i] = a0p[k * lda + i];
#pragma unroll
    for (int j = 0; j < BS; ++j) b[j] = b0p[k * ldb + j];
#pragma unroll
    for (int i = 0; i < BS; ++i)
#pragma unroll
      for (int j = 0; j < BS; ++j) acc[i][j] = fma(a[i], b[j], acc[i][j]);
  }
}

// induced 1-norm (max absolute column sum, NaN-propagating) of a register-block matrix
template <int BS>
__device__ __forceinline__ double blk_norm1(const double (&x)[BS][BS]) {
  double m = 0.0;
#pragma unroll
  for (int j = 0; j < BS; ++j) {
    double cs = 0.0;
#pragma unroll
    for (int i = 0; i < BS; ++i) cs += fabs(x[i][j]);
    cs += shfl_xor_f64(cs, 8);
    cs += shfl_xor_f64(cs, 16);
    cs += shfl_xor_f64(cs, 32);
    m = (j == 0) ? cs : nanmax(m, cs);
  }
  m = nanmax(m, shfl_xor_f64(m, 1));
  m = nanmax(m, shfl_xor_f64(m, 2));
  m = nanmax(m, shfl_xor_f64(m, 4));
  return m;
}

template <int BS>
__device__ __forceinline__ double blk_maxabs(const double (&x)[BS][BS]) {
  double m = 0.0;
#pragma unroll
  for (int i = 0; i < BS; ++i)
#pragma unroll
    for (int j = 0; j < BS; ++j) m = nanmax(m, fabs(x[i][j]));
  return wave_nanmax(m);
}

// In-place Gauss-Jordan elimination with partial (row) pivoting on an LDS-resident augmented
// system [M | RHS]: rows 0..n-1, row stride ldw, M in columns [0,n), right-hand sides up to
// column `ncols` (zero padding columns in between are harmless).  On exit columns >= n of
// row j hold row j of M^-1 RHS.  Lanes own columns, so within one elimination step no lane
// reads what another lane writes; one wave_sync per step orders consecutive steps.
// A zero pivot yields inf/NaN in the result (no trap, no hang) -- callers test for it.
__device__ __forceinline__ void gauss_jordan_lds(double* W, int ldw, int n, int ncols, int lane) {
  for (int j = 0; j < n; ++j) {
    wave_sync();
    // pivot search, redundantly in every lane (broadcast reads): first max |W[i][j]|, i >= j
    int r = j;
    double best = fabs(W[j * ldw + j]);
    for (int i = j + 1; i < n; ++i) {
      const double v = fabs(W[i * ldw + j]);
      if (v > best) {
        best = v;
        r = i;
      }
    }
    const double wjj = W[j * ldw + j];
    const double inv = 1.0 / W[r * ldw + j];
    for (int c = j + 1 + lane; c < ncols; c += 64) {
      const double xr = W[r * ldw + c];
      const double xj = W[j * ldw + c];
      const double pr = xr * inv;
      W[j * ldw + c] = pr;
      if (r != j) W[r * ldw + c] = xj;
      for (int i = 0; i < n; ++i) {
        if (i == j) continue;
        const double f = (i == r) ? wjj : W[i * ldw + j];
        W[i * ldw + c] = fma(-f, pr, W[i * ldw + c]);
      }
    }
  }
  wave_sync();
}

}  // namespace dsge

// ===========================================================================================
// Blocked Gauss-Jordan with partial pivoting inside each BS-column panel.
//
// Same elimination as gauss_jordan_lds (identical pivot sequence: the panel is eliminated column
// by column on a copy, exactly as the unblocked sweep would update those columns), but the
// O(n^2 ncols) work is done as rank-BS updates on BSxBS register blocks, and the O(n BS^2) panel
// work runs in registers with one matrix row per lane, pivot search by a DPP wave reduction and
// pivot-row broadcast by v_readlane.  Rows are never swapped: row r that served as pivot for
// column j ends up holding solution row j; `prow[j] = r` records it and gj_unpermute() restores
// the natural order of the right-hand-side columns.
//
// Block step for panel columns J (width bw), pivot rows Rk = (r_0..r_{bw-1}), M = W[Rk, J]:
//   Lhat[i,:] = W[i,J] M^-1 (i not in Rk),  Lhat[r_a,:] = e_a - M^-1[a,:]
//   Y = M^-1 W[Rk,:]                         W[i,:] -= Lhat[i,:] W[Rk,:]  (all rows)
// Lhat and M^-1 come out of the augmented panel elimination [W[:,J] | 0 or e_a].
// ===========================================================================================
namespace dsge {

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned long long dpp_move_u64(unsigned long long v) {
  int lo = (int)(v & 0xffffffffull), hi = (int)(v >> 32);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, ROW_MASK, 0xf, false);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, ROW_MASK, 0xf, false);
  return ((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo;
}

// max over the 64 lanes of an unsigned 64-bit key (identity 0); result is wave-uniform
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
  unsigned long long t;
  t = dpp_move_u64<0x111, 0xf>(v);  // row_shr:1
  v = t > v ? t : v;
  t = dpp_move_u64<0x112, 0xf>(v);  // row_shr:2
  v = t > v ? t : v;
  t = dpp_move_u64<0x114, 0xf>(v);  // row_shr:4
  v = t > v ? t : v;
  t = dpp_move_u64<0x118, 0xf>(v);  // row_shr:8
  v = t > v ? t : v;
  t = dpp_move_u64<0x142, 0xa>(v);  // row_bcast:15 -> rows 1,3
  v = t > v ? t : v;
  t = dpp_move_u64<0x143, 0xc>(v);  // row_bcast:31 -> rows 2,3
  v = t > v ? t : v;
  int lo = (int)(v & 0xffffffffull), hi = (int)(v >> 32);
  lo = __builtin_amdgcn_readlane(lo, 63);
  hi = __builtin_amdgcn_readlane(hi, 63);
  return ((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo;
}

// max over the 64 lanes of an unsigned 32-bit key (identity 0); wave-uniform result.  One v_max_u32 with a
// DPP operand per step.
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
#define DSGE_DPP_MAX(CTRL, ROWS)                                                                   \
  do {                                                                                             \
    const unsigned t = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROWS, 0xf, false);   \
    v = t > v ? t : v;                                                                             \
  } while (0)
  DSGE_DPP_MAX(0x111, 0xf);  // row_shr:1
  DSGE_DPP_MAX(0x112, 0xf);  // row_shr:2
  DSGE_DPP_MAX(0x114, 0xf);  // row_shr:4
  DSGE_DPP_MAX(0x118, 0xf);  // row_shr:8
  DSGE_DPP_MAX(0x142, 0xa);  // row_bcast:15 -> rows 1,3
  DSGE_DPP_MAX(0x143, 0xc);  // row_bcast:31 -> rows 2,3
#undef DSGE_DPP_MAX
  return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_move_f64(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, ROW_MASK, 0xf, false);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, ROW_MASK, 0xf, false);
  return __hiloint2double(hi, lo);
}

// A double moved between lanes by a DPP control under which EVERY lane has a source lane (quad_perm, row_mirror, row_half_mirror,
// row_ror, all rows and banks enabled): no old value exists to keep, so none is handed over -- dpp_move_f64 zeroes the destination
// first (two v_mov_b32 per double) for the controls that leave lanes without a source.  Same two v_mov_b32_dpp, same values.
template <int CTRL>
__device__ __forceinline__ double dpp_perm_f64(double v) {
  static_assert((CTRL >= 0 && CTRL <= 0xFF) || CTRL == 0x140 || CTRL == 0x141 || (CTRL >= 0x121 && CTRL <= 0x12F),
                "a control that gives every lane a source");
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_mov_dpp(lo, CTRL, 0xf, 0xf, true);
  hi = __builtin_amdgcn_mov_dpp(hi, CTRL, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}

// max over the 64 lanes of doubles that are >= +0 and not NaN, where only the lanes with (lane & 3) == (lane >> 4) may hold anything but
// +0: the diagonal positions of the 4 x 4 tile layout (dsge_mfma4.hpp: lane l holds row l >> 4 and column l & 3 of its block).  Two
// row rotations (by 4 and by 8 lanes) leave the maximum of 16-lane row k in every lane of that row with (lane & 3) == k, lane 17 k among
// them; the four row maxima are read from there and folded in.  A maximum of such values is exact in any order: the same double as
// wave_max_u32 on the high word followed by wave_max_u32 on the low words of the lanes that reach it, in four lane moves, eight
// read-lanes and six v_max_f64 instead of twelve DPP maxima with a wait state in front of each.  Wave-uniform result; every lane
// active.  The maxima are assembly: fmax() puts a canonicalising v_max_f64 in front of every operand it cannot prove quiet, and these
// operands come out of integer moves.  Wait states: the lane moves and read-lanes are builtins, the compiler keeps theirs (it takes an
// assembly statement's outputs as VALU writes); the last statement opens with the two a VALU read of a scalar register needs behind
// the read-lane that wrote it (gfx940 and later), which it does not add in front of assembly text.
__device__ __forceinline__ double tile_diag_wave_max(double v) {
  double t = dpp_perm_f64<0x124>(v);  // row_ror:4
  asm("v_max_f64 %0, %1, %2" : "=v"(v) : "v"(v), "v"(t));
  t = dpp_perm_f64<0x128>(v);  // row_ror:8
  asm("v_max_f64 %0, %1, %2" : "=v"(v) : "v"(v), "v"(t));
  const int lo = __double2loint(v), hi = __double2hiint(v);
  double r[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) r[k] = __hiloint2double(__builtin_amdgcn_readlane(hi, 17 * k), __builtin_amdgcn_readlane(lo, 17 * k));
  double mx;
  asm("s_nop 1\n\tv_max_f64 %0, %1, %2\n\tv_max_f64 %0, %0, %3\n\tv_max_f64 %0, %0, %4\n\tv_max_f64 %0, %0, %5"
      : "=&v"(mx)
      : "v"(v), "s"(r[0]), "s"(r[1]), "s"(r[2]), "s"(r[3]));
  return mx;
}

// ---- row broadcasts of a double inside the consuming instruction (gfx90a and later: the FP64 ALU's only DPP control) -----------
// row_newbcast:J hands every lane the value lane J of its own 16-lane row holds (tools/dpp_probe/dpp_probe.hip checks that, the
// in-place form d == row_src included, and gives the issue costs).  hipcc does not select these forms (update_dpp on the halves is
// two v_mov_b32_dpp, v_fma_f64 stays VOP3), hence the assembly.  Conditions the CALLER keeps, the compiler's hazard handling does not
// look into assembly text:
//   * every lane is active (a masked-off source lane delivers nothing);
//   * a DPP operand written by a VALU instruction needs two wait states before it is read: NOP = true puts an s_nop 1 in front,
//     NOP = false is for operands whose last write lies at least two instructions back BY CONSTRUCTION (say how at the call).
// the value of lane J of the own row (v_mov_b64_dpp)
template <int J, bool NOP>
__device__ __forceinline__ double row_bcast_f64(double row_src) {
  static_assert(J >= 0 && J < 16, "lane of the row");
  double d;
  if constexpr (NOP)
    asm("s_nop 1\n\tv_mov_b64_dpp %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "=v"(d) : "v"(row_src), "n"(J));
  else
    asm("v_mov_b64_dpp %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "=v"(d) : "v"(row_src), "n"(J));
  return d;
}

// d = fma(row_src[lane J of the own row], s, d) in one v_fmac_f64_dpp: the same fused multiply-add on the same three values as
// fma(readlane(row_src, 16 (lane / 16) + J), s, d)
template <int J, bool NOP>
__device__ __forceinline__ void fmac_row_bcast(double& d, double row_src, double s) {
  static_assert(J >= 0 && J < 16, "lane of the row");
  if constexpr (NOP)
    asm("s_nop 1\n\tv_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(d) : "v"(row_src), "v"(s), "n"(J));
  else
    asm("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(d) : "v"(row_src), "v"(s), "n"(J));
}

// One pivot's update of the other seven columns of a row-per-lane 8 x 8 elimination whose rows are replicated over the 8-lane groups
// (lane J of every row holds pivot row J): fr[q] = fma(-ci, fr[q] of lane J, fr[q]) for q != J, in ONE assembly statement and in
// the order q = J + 1, J + 2, ... (mod 8).  The order is what keeps the DPP wait states without a nop (kalman_mf_kernel, phase c):
// the column the NEXT pivot broadcasts first (J + 1) is written first, six instructions ahead of the statement's end, and the
// column a select wrote last (J - 1: the previous pivot's own) is read last, six instructions behind its start.
template <int J, bool NOP>
__device__ __forceinline__ void pivot_row_bcast_update(double (&fr)[8], double ci) {
  static_assert(J >= 0 && J < 8, "pivot");
#define DSGE_PV(K) "v_fmac_f64_dpp %" #K ", %" #K ", -%7 row_newbcast:%8 row_mask:0xf bank_mask:0xf\n\t"
  if constexpr (NOP)
    asm("s_nop 1\n\t" DSGE_PV(0) DSGE_PV(1) DSGE_PV(2) DSGE_PV(3) DSGE_PV(4) DSGE_PV(5) DSGE_PV(6)
        : "+v"(fr[(J + 1) & 7]), "+v"(fr[(J + 2) & 7]), "+v"(fr[(J + 3) & 7]), "+v"(fr[(J + 4) & 7]), "+v"(fr[(J + 5) & 7]),
          "+v"(fr[(J + 6) & 7]), "+v"(fr[(J + 7) & 7])
        : "v"(ci), "n"(J));
  else
    asm(DSGE_PV(0) DSGE_PV(1) DSGE_PV(2) DSGE_PV(3) DSGE_PV(4) DSGE_PV(5) DSGE_PV(6)
        : "+v"(fr[(J + 1) & 7]), "+v"(fr[(J + 2) & 7]), "+v"(fr[(J + 3) & 7]), "+v"(fr[(J + 4) & 7]), "+v"(fr[(J + 5) & 7]),
          "+v"(fr[(J + 6) & 7]), "+v"(fr[(J + 7) & 7])
        : "v"(ci), "n"(J));
#undef DSGE_PV
}

// The four running sums of a steady filter step over the eight entries of a vector v that sits in lanes 0..7 of every row:
//   w0 = fma(f[o], v[o], w0), a0 = fma(k[o], v[o], a0) for o = 0, 2, 4, 6;  w1, a1 likewise for o = 1, 3, 5, 7,
// each sum in that order.  v_own is the lane's own entry, written just before: the statement starts with the wait states.
__device__ __forceinline__ void steady_sums_row_bcast(double& w0, double& w1, double& a0, double& a1, double v_own,
                                                      const double (&f)[8], const double (&k)[8]) {
#define DSGE_SS(O, O1, F0, F1, K0, K1)                                                       \
  "v_fmac_f64_dpp %0, %4, %" #F0 " row_newbcast:" #O " row_mask:0xf bank_mask:0xf\n\t"    \
  "v_fmac_f64_dpp %1, %4, %" #F1 " row_newbcast:" #O1 " row_mask:0xf bank_mask:0xf\n\t"  \
  "v_fmac_f64_dpp %2, %4, %" #K0 " row_newbcast:" #O " row_mask:0xf bank_mask:0xf\n\t"    \
  "v_fmac_f64_dpp %3, %4, %" #K1 " row_newbcast:" #O1 " row_mask:0xf bank_mask:0xf\n\t"
  asm("s_nop 1\n\t" DSGE_SS(0, 1, 5, 6, 13, 14) DSGE_SS(2, 3, 7, 8, 15, 16) DSGE_SS(4, 5, 9, 10, 17, 18) DSGE_SS(6, 7, 11, 12, 19, 20)
      : "+v"(w0), "+v"(w1), "+v"(a0), "+v"(a1)
      : "v"(v_own), "v"(f[0]), "v"(f[1]), "v"(f[2]), "v"(f[3]), "v"(f[4]), "v"(f[5]), "v"(f[6]), "v"(f[7]), "v"(k[0]), "v"(k[1]),
        "v"(k[2]), "v"(k[3]), "v"(k[4]), "v"(k[5]), "v"(k[6]), "v"(k[7]));
#undef DSGE_SS
}

// ---- a vector of up to 32 doubles, one per lane of rows 0 and 1, made readable by row broadcasts in BOTH of these rows ----------
// v_permlane16_swap_b32 vdst, src (gfx950) exchanges the odd 16-lane rows of vdst with the even rows of src.  Started from two
// copies of v, one swap per half of the double leaves
//   x: rows 0 and 1 both hold v[0..15]  (rows 2 and 3: v[32..47]),     y: rows 0 and 1 both hold v[16..31]  (rows 2, 3: v[48..63]),
// so that entry kk of v is lane kk & 15 of the own row of x (kk < 16) or y (kk >= 16) for every lane below 32
// (tools/dpp_probe/dpp_probe.hip checks the pattern in all 64 lanes).  The builtin, not assembly: the compiler keeps the swap's own
// wait states (a VALU write of either operand, two wait states, the swap) and makes the copies.  WITH_Y = false: y is not produced
// (the second register of the swap is a scratch copy).
template <bool WITH_Y>
__device__ __forceinline__ void rows01_pair_f64(double v, double& x, double& y) {
  const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
  const auto l2 = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
  const auto h2 = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
  x = __hiloint2double((int)h2[0], (int)l2[0]);
  if constexpr (WITH_Y) y = __hiloint2double((int)h2[1], (int)l2[1]);
}

// The two running sums of a matrix-vector product, one row of the matrix per lane (t[kk]: this lane's entry of column kk), the
// vector as rows01_pair_f64 left it:
//   s0 = +0.0, s0 = fma(t[kk], v[kk], s0) for kk = 0, 2, 4, .., NC - 2 in that order,   s1 likewise for kk = 1, 3, .., NC - 1,
// each the same fused multiply-add on the same values as with v[kk] read by read-lanes (the first term is an FMA as every other: a
// product of -0 still rounds to +0).  Columns 0..15 broadcast from x, columns 16..NC - 1 from y (NC <= 16: y is not read, pass x).
// ONE statement, and its order keeps the DPP wait states: x and y are VALU results (the swap writes both its registers) and may be
// the instruction before -- the two moves that zero the sums stand between them and the first broadcast.
#define DSGE_MV(ACC, SRC, T, J) "v_fmac_f64_dpp %" #ACC ", %" #SRC ", %" #T " row_newbcast:" #J " row_mask:0xf bank_mask:0xf\n\t"
#define DSGE_MV10                                                                                                               \
  "v_mov_b64 %0, 0\n\tv_mov_b64 %1, 0\n\t" DSGE_MV(0, 2, 4, 0) DSGE_MV(1, 2, 5, 1) DSGE_MV(0, 2, 6, 2) DSGE_MV(1, 2, 7, 3) DSGE_MV(0, 2, 8, 4) DSGE_MV(1, 2, 9, 5) \
      DSGE_MV(0, 2, 10, 6) DSGE_MV(1, 2, 11, 7) DSGE_MV(0, 2, 12, 8) DSGE_MV(1, 2, 13, 9)
#define DSGE_MV12 DSGE_MV10 DSGE_MV(0, 2, 14, 10) DSGE_MV(1, 2, 15, 11)
#define DSGE_MV14 DSGE_MV12 DSGE_MV(0, 2, 16, 12) DSGE_MV(1, 2, 17, 13)
#define DSGE_MV16 DSGE_MV14 DSGE_MV(0, 2, 18, 14) DSGE_MV(1, 2, 19, 15)
#define DSGE_MV18 DSGE_MV16 DSGE_MV(0, 3, 20, 0) DSGE_MV(1, 3, 21, 1)
#define DSGE_MV20 DSGE_MV18 DSGE_MV(0, 3, 22, 2) DSGE_MV(1, 3, 23, 3)
#define DSGE_MV_T10 "v"(t[0]), "v"(t[1]), "v"(t[2]), "v"(t[3]), "v"(t[4]), "v"(t[5]), "v"(t[6]), "v"(t[7]), "v"(t[8]), "v"(t[9])
#define DSGE_MV_T12 DSGE_MV_T10, "v"(t[10]), "v"(t[11])
#define DSGE_MV_T14 DSGE_MV_T12, "v"(t[12]), "v"(t[13])
#define DSGE_MV_T16 DSGE_MV_T14, "v"(t[14]), "v"(t[15])
#define DSGE_MV_T18 DSGE_MV_T16, "v"(t[16]), "v"(t[17])
#define DSGE_MV_T20 DSGE_MV_T18, "v"(t[18]), "v"(t[19])
template <int NC, int NT>
__device__ __forceinline__ void matvec_sums_row_bcast(double& s0, double& s1, double x, double y, const double (&t)[NT]) {
  static_assert(NC >= 10 && NC <= 20 && NC % 2 == 0 && NC <= NT, "columns");
  if constexpr (NC == 10) asm(DSGE_MV10 : "=&v"(s0), "=&v"(s1) : "v"(x), "v"(y), DSGE_MV_T10);
  if constexpr (NC == 12) asm(DSGE_MV12 : "=&v"(s0), "=&v"(s1) : "v"(x), "v"(y), DSGE_MV_T12);
  if constexpr (NC == 14) asm(DSGE_MV14 : "=&v"(s0), "=&v"(s1) : "v"(x), "v"(y), DSGE_MV_T14);
  if constexpr (NC == 16) asm(DSGE_MV16 : "=&v"(s0), "=&v"(s1) : "v"(x), "v"(y), DSGE_MV_T16);
  if constexpr (NC == 18) asm(DSGE_MV18 : "=&v"(s0), "=&v"(s1) : "v"(x), "v"(y), DSGE_MV_T18);
  if constexpr (NC == 20) asm(DSGE_MV20 : "=&v"(s0), "=&v"(s1) : "v"(x), "v"(y), DSGE_MV_T20);
}
#undef DSGE_MV_T20
#undef DSGE_MV_T18
#undef DSGE_MV_T16
#undef DSGE_MV_T14
#undef DSGE_MV_T12
#undef DSGE_MV_T10
#undef DSGE_MV20
#undef DSGE_MV18
#undef DSGE_MV16
#undef DSGE_MV14
#undef DSGE_MV12
#undef DSGE_MV10
#undef DSGE_MV

// sum over the 64 lanes (wave-uniform result): DPP row shifts + row broadcasts, no LDS traffic.
// Lanes that receive nothing get +0.0 (identity).  Summation order differs from wave_sum().
__device__ __forceinline__ double wave_sum_dpp(double v) {
  v += dpp_move_f64<0x111, 0xf>(v);  // row_shr:1
  v += dpp_move_f64<0x112, 0xf>(v);  // row_shr:2
  v += dpp_move_f64<0x114, 0xf>(v);  // row_shr:4
  v += dpp_move_f64<0x118, 0xf>(v);  // row_shr:8
  v += dpp_move_f64<0x142, 0xa>(v);  // row_bcast:15 -> rows 1,3
  v += dpp_move_f64<0x143, 0xc>(v);  // row_bcast:31 -> rows 2,3
  int lo = __builtin_amdgcn_readlane(__double2loint(v), 63);
  int hi = __builtin_amdgcn_readlane(__double2hiint(v), 63);
  return __hiloint2double(hi, lo);
}

// 1/sqrt(x) for x in a safe range: hardware estimate + two Newton steps (~1 ulp)
__device__ __forceinline__ double fast_rsqrt(double x) {
  double y = __builtin_amdgcn_rsq(x);
  const double hx = 0.5 * x;
  y = y * fma(-hx * y, y, 1.5);
  y = y * fma(-hx * y, y, 1.5);
  return y;
}

// 1/x for x in a safe range: hardware estimate + two Newton steps
__device__ __forceinline__ double fast_rcp(double x) {
  double y = __builtin_amdgcn_rcp(x);
  y = y * fma(-x, y, 2.0);
  y = y * fma(-x, y, 2.0);
  return y;
}

// reference implementation with plain shuffles (self-test of the DPP encodings)
__device__ __forceinline__ unsigned long long wave_max_u64_shfl(unsigned long long v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned long long t = __shfl_xor(v, m, 64);
    v = t > v ? t : v;
  }
  return v;
}

__device__ __forceinline__ double readlane_dyn_f64(double v, int src_lane_uniform) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_readlane(lo, src_lane_uniform);
  hi = __builtin_amdgcn_readlane(hi, src_lane_uniform);
  return __hiloint2double(hi, lo);
}

// W: n rows x (ngroups*NP) columns, row stride ldw, matrix in columns [0,n).  Scratch in LDS:
// Lbuf (NP*BS doubles), Ybuf (BS * ngroups*NP doubles), prow (NP ints).
// Largest / smallest |pivot| of a solve beyond which it is refined once.  The ratio is a free but loose proxy of cond(A1)
// (1e2 .. 3e4 below it), and the blocked elimination loses more digits the wider its panels: on the tiles of up to 40
// variables (panels of <= 5 columns) 1e4 in ANY iteration keeps the fuzz campaigns at the fixed 1e-9 bar (about two
// SW-shaped draws in a thousand refine an iteration); on the wider tiles (panels of 6..8 columns, and the four-wavefront
// kernel) a draw with a ratio of 3.3e3 at cond 9e7 came out 7e-9 off (fuzz seed 2): 1e3 there (one or two draws in a
// hundred).  Every refinement lengthens its draw by an elimination, and the launch by that draw's tail: the 1e3 rule on the
// 32-wide tile of the bench costs 0.1 ms of the 0.65 ms solver launch, the 1e4 rule 0.04 ms.
// Round 5: 3e3 on the tiles of up to 40 variables.  The round-4 campaign (ten times the suite's trial counts) left ONE system in
// 3000 at 2.7e-9 from the 40-digit T (an ill-conditioned intermediate A1 with a pivot ratio between 3e3 and 1e4) against the
// suite's own 1e-9 bar; 3e3 takes it.  Cost on the bench: see profiles/r5/ (about three draws in a thousand more refine an iteration).
constexpr double CR_REFINE_PIVOT_RATIO = 1e3;
template <int BS>
__device__ __forceinline__ constexpr double cr_refine_ratio() {
  // (round 6: 1e3 on the tiles of up to 24 variables as well -- the final campaign's one system above the bar, n = 18, 2.0e-9 from
  //  the 40-digit T at cond(B + C T) = 17: an intermediate A1 again; the bench's 32- and 40-wide instances keep 3e3)
  return (BS <= 3 || BS > 5) ? 1e3 : 3e3;
}

// RHS_REG (round 9, gauss_jordan_blocked_rhs below): the right-hand sides -- column group 1 of two -- live in the caller's
// register block Rg instead of W; false is the LDS form every other caller uses, which never touches Rg.
// REC_W (round 17, register form only): the multipliers of panel kb are kept in the panel's own block column of W -- columns
// kb BS .. kb BS + BS - 1 of rows < n, dead once the panel is done: the trailing updates skip them, the pivot-row copies to Ybuf
// read them for nothing -- as -Lhat, the very values Lbuf holds for one panel.  gj_replay<BS, true> applies the elimination to
// one more right-hand-side group from there.  Two LDS stores of a row per lane and panel; nothing else changes.
template <int BS, bool RHS_REG, bool REC_W = false>
__device__ __forceinline__ void gauss_jordan_blocked_impl(double* W, int ldw, int n, int ngroups, double* Lbuf, double* Ybuf,
                                                          int* prow, int lane, long long* ph, double& inv_min, double& inv_max,
                                                          double* rec_L, double (&Rg)[BS][BS]) {
  // rec_L (optional, nsteps x NP x BS doubles): the elimination's multipliers Lhat of every block step are kept, so that
  // gj_replay can apply the SAME elimination to further right-hand sides (with prow, which holds the pivot rows)
  // inv_min / inv_max: smallest and largest |1 / pivot| met (wave-uniform): their ratio is a free lower estimate of the
  // condition number, which crc_iterate uses to decide on a step of iterative refinement
  //
  // (round 7) The panel is bound by instruction issue, not by its arithmetic: what follows keeps every floating-point
  // operation of round 6 with its operands and its order (bit-identical results, tests/test_gpu_cr_bitwise.py) and trims the
  // integer, select and cross-lane instructions around them -- docs/design/cycle_reduction.md lists each cut with its count.
  constexpr int NP = 8 * BS;
  const int lr = lane >> 3, lc = lane & 7;
  const int wcols = ngroups * NP;
  // rows still to be chosen as pivots: bit i = row i exists and has not been a pivot row.  Wave-uniform (a scalar register
  // pair), handed to the pivot search as the condition of ONE select per pivot (inverse ballot) where every lane used to shift
  // a 64-bit `used` mask by its own index.
  const int nrow = (n < NP) ? n : NP;  // (n <= NP for every caller: the tile is chosen from n)
  unsigned long long avail = (nrow >= 64) ? ~0ull : ((1ull << nrow) - 1ull);
  const int nsteps = (n + BS - 1) / BS;
  // Lanes >= n take no part in the result of a panel: no pivot is searched there, no other lane reads their registers, and
  // their Lhat rows are zeros.  So they run the panel on whatever their (clamped) row holds, without a select per loaded
  // value, and the zero rows n .. NP-1 of Lbuf are written once per elimination instead of once per panel.
  // Lbuf holds -Lhat, the factor the trailing update multiplies by: loaded as Lhat and negated inside the FMAs, the negation
  // did not stay an operand modifier -- the register blocks are used by two column groups, the compiler negated them ahead of
  // both (and back for the skipped group): 65 moves and sign flips per panel.  (-Lhat of a zero row is -0.0.)
  const int prl = (lane < NP) ? lane : NP - 1;
  wave_sync();
  if (lane >= nrow && lane < NP) {
#pragma unroll
    for (int b = 0; b < BS; ++b) Lbuf[lane * BS + b] = -0.0;
  }
  for (int kb = 0; kb < nsteps; ++kb) {
    const int j0 = kb * BS;
    const int bw = (n - j0 < BS) ? (n - j0) : BS;
    wave_sync();
    const long long tk_p = ph ? clock64() : 0;
    // ---- panel: one matrix row per lane, augmented with the identity slots ------------
    double pw[BS], id[BS];
#pragma unroll
    for (int c = 0; c < BS; ++c) pw[c] = W[prl * ldw + j0 + c];  // (columns >= bw of a partial panel: inside the tile, never a pivot column)
    int rsel[BS];
    double inv_own = 1.0;  // pivot lanes: 1 / pivot of their row (the row is scaled once, after the panel)
#pragma unroll
    for (int c = 0; c < BS; ++c) {
      rsel[c] = 0;
      id[c] = 0.0;  // (columns a partial panel does not reach)
    }
    // one pivot of the panel (column c: a compile-time constant after unrolling)
    auto panel_pivot = [&](int c) {
      // pivot = largest |entry| among the unused rows, compared on the high 32 bits of the double (sign
      // cleared; exponent + 20 mantissa bits; low 6 bits carry 63 - lane so that ties go to the first row):
      // within 2^-14 of the true maximum, which is all partial pivoting needs, at one v_max_u32 per DPP step
      const unsigned own = ((unsigned)__double2hiint(pw[c]) & 0x7fffffc0u) | (unsigned)(63 - lane);
      const unsigned key = wave_max_u32(__builtin_amdgcn_inverse_ballot_w64(avail) ? own : 0u);
      const int r = 63 - (int)(key & 63u);
      rsel[c] = r;
      avail &= ~(1ull << r);
      const bool is_r = (lane == r);
      // broadcast the pivot lane's row scaled by 1 / pivot and eliminate everywhere else.  The pivot lane itself is
      // left alone (multiplier 0: no divergent branch) and scaled after the panel -- later columns only ever read
      // a row through its own elimination multiplier, which is consistent with the unscaled row.
      const double inv = fast_rcp(readlane_dyn_f64(pw[c], r));
      inv_min = fmin(inv_min, fabs(inv));
      inv_max = fmax(inv_max, fabs(inv));
      const double f = is_r ? 0.0 : pw[c];
      inv_own = is_r ? inv : inv_own;
      // identity slot of this column: 1 on the pivot lane (a select on the high word alone: 0.0 and 1.0 share the low one),
      // 0 elsewhere, eliminated at once.  The pivot lane's slot IS 1.0, so the broadcast of round 6 (two v_readlane and
      // 1.0 * inv, which is inv) is not issued.
      id[c] = fma(-f, inv, __hiloint2double(is_r ? 0x3ff00000 : 0, 0));
#pragma unroll
      for (int c2 = 0; c2 < BS; ++c2) {
        if (c2 > c) pw[c2] = fma(-f, readlane_dyn_f64(pw[c2], r) * inv, pw[c2]);
        if (c2 < c) id[c2] = fma(-f, readlane_dyn_f64(id[c2], r) * inv, id[c2]);
      }
    };
    // what a panel leaves behind: Lhat -> Lbuf, the pivot rows of W -> Ybuf, the pivot rows' indices -> prow.  FULL: a
    // compile-time flag, the per-column tests `< bw` of a partial panel are not issued for a full one.
    auto panel_store = [&](auto full_tag) {
      constexpr bool FULL = decltype(full_tag)::value;
#pragma unroll
      for (int c = 0; c < BS; ++c) id[c] *= inv_own;  // (pw is dead from here on)
      // Lhat row of this lane: -id for ordinary rows; pivot lane r_a holds id = Minv[a,:] and needs e_a - Minv[a,:].  Its
      // negative, nl = id - e_a, is one subtraction of a selected constant: 1.0 on the pivot lane, +0.0 elsewhere (x - (+0.0) is
      // x, signed zeros included) -- again a select on the high word alone, of the constant the identity slots are made of
      // (a second one would sit in a register through the whole kernel).  -(1 - x) and x - 1 round alike.
      if (lane < nrow) {
        double nl[BS];
#pragma unroll
        for (int b = 0; b < BS; ++b) {
          const bool piv = (FULL || b < bw) && lane == rsel[b];
          nl[b] = id[b] - __hiloint2double(piv ? 0x3ff00000 : 0, 0);
        }
#pragma unroll
        for (int b = 0; b < BS; ++b) Lbuf[lane * BS + b] = nl[b];
        if constexpr (REC_W) {  // (every slot of the row, as Lbuf: a partial panel's are signed zeros the FMAs see)
#pragma unroll
          for (int b = 0; b < BS; ++b) W[lane * ldw + j0 + b] = nl[b];
        }
        if (rec_L) {  // (Lhat itself: gj_replay negates)
#pragma unroll
          for (int b = 0; b < BS; ++b) rec_L[((size_t)kb * NP + lane) * BS + b] = -nl[b];
        }
      }
      if (rec_L && lane >= nrow && lane < NP) {
#pragma unroll
        for (int b = 0; b < BS; ++b) rec_L[((size_t)kb * NP + lane) * BS + b] = 0.0;
      }
      // pivot rows of W (original values) -> Ybuf, one column per lane
      for (int c = lane; c < (RHS_REG ? NP : wcols); c += 64) {
#pragma unroll
        for (int b = 0; b < BS; ++b) Ybuf[b * wcols + c] = (FULL || b < bw) ? W[rsel[b] * ldw + c] : 0.0;
      }
      if constexpr (RHS_REG) {
        // ... and of the register-resident group (the values before this panel's update, as the copy from W takes them).  Every
        // index into the register block is a compile-time constant: row i of a lane's block is matrix row lr * BS + i, and the
        // lane asks which pivot of the panel, if any, that row is -- compares against the wave-uniform rsel[b] and selects of
        // the target row of Ybuf, then ONE exec-masked row store per position i.  (A uniform branch per pivot on its position
        // rsel[b] % BS was built first: four cascades of scalar branches per panel cost what the saved LDS traffic gained.)
        double* ycol = Ybuf + NP + lc * BS;
#pragma unroll
        for (int i = 0; i < BS; ++i) {
          const int row = lr * BS + i;
          int yoff = -1;
#pragma unroll
          for (int b = 0; b < BS; ++b)
            if (FULL || b < bw) yoff = (row == rsel[b]) ? b * wcols : yoff;
          if (yoff >= 0) {
#pragma unroll
            for (int j = 0; j < BS; ++j) ycol[yoff + j] = Rg[i][j];
          }
        }
        if (!FULL && lr == 0) {  // (rows a partial panel does not reach: zero rows, their FMAs are issued)
#pragma unroll
          for (int b = 0; b < BS; ++b)
            if (b >= bw) {
#pragma unroll
              for (int j = 0; j < BS; ++j) ycol[b * wcols + j] = 0.0;
            }
        }
      }
#pragma unroll
      for (int a = 0; a < BS; ++a)
        if ((FULL || a < bw) && lane == 0) prow[j0 + a] = rsel[a];
    };
    // (round 6) a FULL panel -- every panel but possibly the last -- runs its BS pivots without the per-column test `c < bw`: the
    // (uniform) branches cut the chain of a panel into one basic block per pivot, which the scheduler cannot overlap; same
    // operations in the same order, bit-identical results
    if (bw == BS) {
#pragma unroll
      for (int c = 0; c < BS; ++c) panel_pivot(c);
      panel_store(std::true_type{});
    } else {
#pragma unroll
      for (int c = 0; c < BS; ++c)
        if (c < bw) panel_pivot(c);
      panel_store(std::false_type{});
    }
    wave_sync();
    const long long tk_t = ph ? clock64() : 0;
    if (ph) ph[0] += tk_t - tk_p;
    // ---- trailing update on register blocks: W[i,:] -= Lhat[i,:] Wpiv ---------------------
    double nl[BS][BS];  // -Lhat
#pragma unroll
    for (int i = 0; i < BS; ++i)
#pragma unroll
      for (int b = 0; b < BS; ++b) nl[i][b] = Lbuf[(lr * BS + i) * BS + b];
    for (int g = 0; g < (RHS_REG ? 1 : ngroups); ++g) {
      // block columns at or left of the panel inside the matrix part are dead (never read again)
      // (round 17) REC_W RESTS ON THIS: the record of panel kb sits in block column kb of group 0, and the pivot-row copies above
      // carry it into Ybuf -- columns < (kb + 1) BS of Ybuf and of W's group 0 must stay unread by every update from here to the
      // end of the elimination, and whatever follows the elimination overwrites group 0 entirely before reading it (crc_iterate).
      // A change that reads those columns breaks the bit-identity of gj_replay<BS, true> without any test of the plain path failing.
      if (g == 0 && lc <= kb) continue;
      const int c0 = g * NP + lc * BS;
      double wb[BS][BS], yb[BS][BS];
#pragma unroll
      for (int i = 0; i < BS; ++i)
#pragma unroll
        for (int j = 0; j < BS; ++j) wb[i][j] = W[(lr * BS + i) * ldw + c0 + j];
#pragma unroll
      for (int b = 0; b < BS; ++b)
#pragma unroll
        for (int j = 0; j < BS; ++j) yb[b][j] = Ybuf[b * wcols + c0 + j];
#pragma unroll
      for (int b = 0; b < BS; ++b)
#pragma unroll
        for (int i = 0; i < BS; ++i)
#pragma unroll
          for (int j = 0; j < BS; ++j) wb[i][j] = fma(nl[i][b], yb[b][j], wb[i][j]);
#pragma unroll
      for (int i = 0; i < BS; ++i)
#pragma unroll
        for (int j = 0; j < BS; ++j) W[(lr * BS + i) * ldw + c0 + j] = wb[i][j];
    }
    if constexpr (RHS_REG) {  // the same FMAs on the register block: no load of the block, no store
      double yb[BS][BS];
#pragma unroll
      for (int b = 0; b < BS; ++b)
#pragma unroll
        for (int j = 0; j < BS; ++j) yb[b][j] = Ybuf[b * wcols + NP + lc * BS + j];
#pragma unroll
      for (int b = 0; b < BS; ++b)
#pragma unroll
        for (int i = 0; i < BS; ++i)
#pragma unroll
          for (int j = 0; j < BS; ++j) Rg[i][j] = fma(nl[i][b], yb[b][j], Rg[i][j]);
    }
    if (ph) ph[1] += clock64() - tk_t;
  }
  wave_sync();
}

template <int BS>
__device__ __forceinline__ void gauss_jordan_blocked(double* W, int ldw, int n, int ngroups, double* Lbuf, double* Ybuf,
                                                     int* prow, int lane, long long* ph, double& inv_min, double& inv_max,
                                                     double* rec_L = nullptr) {
  double none[BS][BS];  // (never read or written by the LDS form)
  gauss_jordan_blocked_impl<BS, false>(W, ldw, n, ngroups, Lbuf, Ybuf, prow, lane, ph, inv_min, inv_max, rec_L, none);
}

template <int BS>
__device__ __forceinline__ void gauss_jordan_blocked(double* W, int ldw, int n, int ngroups, double* Lbuf, double* Ybuf,
                                                     int* prow, int lane, long long* ph = nullptr, double* rec_L = nullptr) {
  double lo = 1e300, hi = 0.0;
  gauss_jordan_blocked<BS>(W, ldw, n, ngroups, Lbuf, Ybuf, prow, lane, ph, lo, hi, rec_L);
}

// (round 9) [A | R] -> [. | A^-1 R] with the right-hand sides in the caller's register block: W holds the matrix in column group
// 0 (row stride ldw, as for two groups; its group 1 is neither read nor written), Rg the block (lr, lc) of R on entry and of
// A^-1 R on return, rows in pivot order exactly as the LDS form leaves them in W (row j of the solution sits in row prow[j];
// there is no row swap).  Ybuf as for two groups.  Every FMA of the LDS form with its operands and its order: bit-identical.
// What it saves is LDS traffic: per panel the block of group 1 is neither loaded nor stored (BS rows each way), and only the
// BS pivot rows go through Ybuf, one exec-masked row store each.
// (round 17) REC_W: the elimination's multipliers stay behind in column group 0 of W (gauss_jordan_blocked_impl).
template <int BS, bool REC_W = false>
__device__ __forceinline__ void gauss_jordan_blocked_rhs(double* W, int ldw, int n, double (&Rg)[BS][BS], double* Lbuf,
                                                         double* Ybuf, int* prow, int lane, long long* ph, double& inv_min,
                                                         double& inv_max) {
  gauss_jordan_blocked_impl<BS, true, REC_W>(W, ldw, n, 2, Lbuf, Ybuf, prow, lane, ph, inv_min, inv_max, nullptr, Rg);
}

// The elimination recorded by gauss_jordan_blocked (rec_L, prow) applied to ONE more right-hand-side column group Wg (NP columns,
// row stride ldw): Wg <- A^-1 Wg, rows in pivot order as there.  The arithmetic is that of the trailing update above, operation
// by operation (same multipliers, same pivot rows, same order of the FMAs): the result is bit-identical to eliminating
// [A | Wg] again, at the cost of the rank-BS updates alone -- no pivot search, no panel, nothing on the matrix part.
// Ybuf2: BS x NP doubles of scratch.  Syncs on entry and exit.
// IN_W (round 17): the record is the one gauss_jordan_blocked_rhs<BS, true> leaves in W -- rec_L = W, row stride ldw, panel kb in
// columns kb BS ..., holding -Lhat: the factor the trailing update multiplies by, so nothing is negated here (the same FMA,
// operand for operand).  Rows >= n of it were not written: they are the -0.0 rows of Lbuf.
template <int BS, bool IN_W = false>
__device__ __forceinline__ void gj_replay(double* Wg, int ldw, int n, const double* rec_L, const int* prow, double* Ybuf2,
                                          int lane) {
  constexpr int NP = 8 * BS;
  const int lr = lane >> 3, lc = lane & 7;
  const int nsteps = (n + BS - 1) / BS;
  for (int kb = 0; kb < nsteps; ++kb) {
    const int j0 = kb * BS;
    const int bw = (n - j0 < BS) ? (n - j0) : BS;
    wave_sync();
    for (int c = lane; c < NP; c += 64) {
#pragma unroll
      for (int b = 0; b < BS; ++b) Ybuf2[b * NP + c] = (b < bw) ? Wg[prow[j0 + (b < bw ? b : 0)] * ldw + c] : 0.0;
    }
    wave_sync();
    double lh[BS][BS], wb[BS][BS], yb[BS][BS];
#pragma unroll
    for (int i = 0; i < BS; ++i)
#pragma unroll
      for (int b = 0; b < BS; ++b) {
        if constexpr (IN_W)
          lh[i][b] = (lr * BS + i < n) ? rec_L[(lr * BS + i) * ldw + j0 + b] : -0.0;
        else
          lh[i][b] = rec_L[((size_t)kb * NP + lr * BS + i) * BS + b];
      }
    const int c0 = lc * BS;
#pragma unroll
    for (int i = 0; i < BS; ++i)
#pragma unroll
      for (int j = 0; j < BS; ++j) wb[i][j] = Wg[(lr * BS + i) * ldw + c0 + j];
#pragma unroll
    for (int b = 0; b < BS; ++b)
#pragma unroll
      for (int j = 0; j < BS; ++j) yb[b][j] = Ybuf2[b * NP + c0 + j];
#pragma unroll
    for (int b = 0; b < BS; ++b)
#pragma unroll
      for (int i = 0; i < BS; ++i)
#pragma unroll
        for (int j = 0; j < BS; ++j) wb[i][j] = fma(IN_W ? lh[i][b] : -lh[i][b], yb[b][j], wb[i][j]);
#pragma unroll
    for (int i = 0; i < BS; ++i)
#pragma unroll
      for (int j = 0; j < BS; ++j) Wg[(lr * BS + i) * ldw + c0 + j] = wb[i][j];
  }
  wave_sync();
}

// Restore natural row order of the right-hand-side column groups [g_first, ngroups): row j of the
// solution sits in row prow[j] of W.  Rows >= n are left untouched.
template <int BS>
__device__ __forceinline__ void gj_unpermute(double* W, int ldw, int n, int g_first, int ngroups, const int* prow,
                                             int lane) {
  constexpr int NP = 8 * BS;
  const int lr = lane >> 3, lc = lane & 7;
  for (int g = g_first; g < ngroups; ++g) {
    const int c0 = g * NP + lc * BS;
    double t[BS][BS];
#pragma unroll
    for (int i = 0; i < BS; ++i) {
      const int r = lr * BS + i;
      const int src = (r < n) ? prow[r] : r;
#pragma unroll
      for (int j = 0; j < BS; ++j) t[i][j] = W[src * ldw + c0 + j];
    }
    wave_sync();
#pragma unroll
    for (int i = 0; i < BS; ++i)
#pragma unroll
      for (int j = 0; j < BS; ++j) W[(lr * BS + i) * ldw + c0 + j] = t[i][j];
    wave_sync();
  }
}

// Dispatch order for the Kalman launch: draws sorted by DESCENDING key (counting sort, keys clamped to 0..63; the order inside
// a bin is arbitrary).  The key is the number of cycle-reduction iterations of the draw: both grow with the persistence of
// the model (roots close to the unit circle), and a persistent model is the one whose covariance recursion reaches its
// fixed point late.  One workgroup.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void kalman_order_kernel(const int32_t* __restrict__ key, int batch,
                                                            int32_t* __restrict__ order, int never_value = -1) {
  // never_value >= 0: the key is a filter's first steady step (-1: never steady = never_value steps), binned by four steps
  // one histogram per wavefront (the 64 bins are hot: a single shared histogram serialises the LDS atomics of the whole
  // block), bases by a wave scan over the bins: 10 -> 4 us per 4096 draws with 1024 threads
  constexpr int NW = BLOCK / 64;
  __shared__ int hist[NW][64], base[NW][64];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  hist[w][lane] = 0;
  __syncthreads();
  for (int i = tid; i < batch; i += BLOCK) {
    int kq = key[i];
    if (never_value >= 0) kq = (kq < 0 ? never_value : kq) >> 2;
    kq = kq < 0 ? 0 : (kq > 63 ? 63 : kq);
    atomicAdd(&hist[w][kq], 1);
  }
  __syncthreads();
  if (w == 0) {  // lane b owns bin 63 - b (descending keys first)
    const int bin = 63 - lane;
    int tot = 0;
#pragma unroll
    for (int q = 0; q < NW; ++q) tot += hist[q][bin];
    int incl = tot;  // inclusive scan over the lanes
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(incl, d, 64);
      if (lane >= d) incl += t;
    }
    int acc = incl - tot;
#pragma unroll
    for (int q = 0; q < NW; ++q) {
      base[q][bin] = acc;
      acc += hist[q][bin];
    }
  }
  __syncthreads();
  for (int i = tid; i < batch; i += BLOCK) {
    int kq = key[i];
    if (never_value >= 0) kq = (kq < 0 ? never_value : kq) >> 2;
    kq = kq < 0 ? 0 : (kq > 63 ? 63 : kq);
    order[atomicAdd(&base[w][kq], 1)] = i;
  }
}



// Persistence key of a draw for the dispatch order of the Kalman launches: a rough spectral-radius estimate of the
// transition matrix, rho ~ (||T^k v|| / ||v||)^(1/k) after k = 24 power-iteration steps from v = 1 (one row of T per lane
// in registers, the vector exchanged by v_readlane), mapped to key = 8 * -log2(1 - rho) clamped to 0..63 -- finer towards
// the unit circle, where the covariance recursion of the filter converges slowly.  Failed draws (status != 0) get key 0.
// One wavefront per draw, n <= 64; a few thousand cycles per draw.
template <int NMAX>
__global__ __launch_bounds__(64) void persistence_key_kernel(const double* __restrict__ T, const int32_t* __restrict__ status,
                                                             int batch, int n, int32_t* __restrict__ key) {
  const int lane = threadIdx.x;
  for (int draw = blockIdx.x; draw < batch; draw += gridDim.x) {
    if (status && status[draw] != 0) {
      if (lane == 0) key[draw] = 0;
      continue;
    }
    const double* Tg = T + (size_t)draw * n * n;
    double row[NMAX];
#pragma unroll
    for (int c = 0; c < NMAX; ++c) row[c] = (lane < n && c < n) ? Tg[(size_t)lane * n + c] : 0.0;
    double v = (lane < n) ? 1.0 : 0.0, lg = 0.0;
    for (int it = 0; it < 24; ++it) {
      double a0 = 0.0, a1 = 0.0;
#pragma unroll
      for (int c = 0; c < NMAX; c += 2) {
        if (c < n) {
          a0 = fma(row[c], readlane_dyn_f64(v, c), a0);
          a1 = fma(row[c + 1], readlane_dyn_f64(v, c + 1), a1);
        }
      }
      v = a0 + a1;
      if ((it & 3) == 3) {  // renormalise every fourth step
        const double nrm = sqrt(wave_sum_dpp(v * v));
        if (!(nrm > 0.0) || !(nrm < 1e300)) break;
        lg += log2(nrm);
        v *= 1.0 / nrm;
      }
    }
    // ||v_0|| = sqrt(n): rho^24 ~ 2^lg / sqrt(n)
    const double rho = exp2((lg - 0.5 * log2((double)n)) / 24.0);
    double kq = (rho < 1.0) ? -8.0 * log2(1.0 - rho) : 63.0;
    if (!(kq == kq)) kq = 0.0;
    kq = kq < 0.0 ? 0.0 : (kq > 63.0 ? 63.0 : kq);
    if (lane == 0) key[draw] = (int32_t)kq;
  }
}

}  // namespace dsge
