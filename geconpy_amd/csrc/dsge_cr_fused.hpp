// Static-variable deflation, cycle reduction on the reduced system and the back-substitution of the static rows in ONE
// launch ("cr_fused_kernel"): the three phases of dsge_cr_deflate.hpp / dsge_cr_compact.hpp with the reduced system handed
// from phase to phase through LDS instead of HBM.
//
//   phase 1  Householder QR of the static columns of B applied to [B_st | B_dy | A_dy | C_dy | D], one column per lane in
//            registers (crd_qr_chunk).  The h top rows go to a per-draw scratch record in global memory (8.5 KB at
//            n = 40, h = 10; read back in phase 3 by the same workgroup, i.e. from L2); the columns of the REDUCED system are
//            written straight into the compact kernel's LDS layout W = [B_dy | A_dy[:,S] C_dy[:,L]] -- the zero columns
//            of A_dy and C_dy are found by a ballot over the column registers, not by a pass over global memory.
//   phase 2  crc_iterate (the loop of cr_compact_kernel, unchanged) and the final solve  [T_dy[:,S] | R_dy] =
//            -A1_hat^-1 [A_dy[:,S] | D_red]; the right-hand side of that solve is the one thing that has to survive the
//            iteration outside the register blocks: it is parked in global scratch (NPD x (s + k) doubles, 6 KB).
//   phase 3  back-substitution of the static rows (crd_inflate_prepare / crd_inflate_chunk) with the columns of
//            [T_dy | R_dy] read from LDS, scatter to the caller's variable order.  (round 16) The top block and with it
//            the static rows are CONDITIONAL: given the caller's observation matrix Z (the fused likelihood call with T
//            and R in the library's arena), a draw none of whose h deflated variables is observed writes no top block in
//            phase 1 and +0.0 into the static rows here (crd_scatter_dynamic) -- the filter gathers T and R over states
//            and observed variables only, and a static variable, with zero columns in A and C, is never a state.  The
//            hand-over for a singular R_st is then decided from the reflectors' betas.  Z = nullptr: always computed.
//
// Against the three launches (SW-shaped 40-variable system, 10 static, 4096 draws): no reduced A, B, C, D, T_dy, R_dy in HBM
// (131 MB written and read back twice), two launches and their tails less.  Draws the fused kernel cannot take -- fewer
// static variables than the bound h, s + l or s + k beyond the reduced tile, a numerically singular R_st -- are flagged
// DSGE_ST_INTERNAL_RERUN and solved by the full-size dense kernel afterwards, exactly as on the three-launch path.
// Limits checked by the launcher: h + 3 nd + k <= 128 with two columns per lane, <= 192 with three (n = 46 .. 64), and
// nd + k <= 64.
#pragma once
#include "dsge_cr_compact.hpp"
#include "dsge_cr_deflate.hpp"

namespace dsge {

template <int BSF, int BSD>
struct CrfSmem {
  static constexpr int NMF = 8 * BSF, NPD = 8 * BSD, LDW = CrcSmem<BSD>::LDW, HM = CRD_HMAX;
  // doubles of the compact kernel's layout (W, Lbuf, Ybuf); phase 1 aliases V (HM x NMF) and phase 3 the inflate arrays
  static constexpr size_t dbl_compact = (size_t)(NPD * LDW + NPD * BSD + BSD * 2 * NPD);
  static constexpr size_t dbl_qr = (size_t)(HM * NMF + HM);
  static constexpr size_t dbl_inflate = CrdInflateLds<NPD>::doubles;
  static constexpr size_t dbl =
      dbl_compact > dbl_qr ? (dbl_compact > dbl_inflate ? dbl_compact : dbl_inflate) : (dbl_qr > dbl_inflate ? dbl_qr : dbl_inflate);
  // index tables: prow (NPD ints, shared with gauss_jordan_blocked); cmap, posS, posL, rsrc (NPD), dyi (64), sti (HM) as
  // bytes (all values < 64): with 32-bit tables the (5, 4) instance needs 20.9 KB -- 7 draws per CU instead of 8
  typedef signed char idx_t;
  static constexpr size_t bytes = sizeof(double) * dbl + sizeof(int) * NPD + ((4 * NPD + 64 + HM + 15) & ~(size_t)15);
};

// per-draw global scratch: top block (crd_top_doubles) and the right-hand side of the final solve, NPD columns of NPD
// doubles (column-major; columns [A_dy[:,S] | D_red], s + k <= NPD of them are written).  (round 13) The leading dimension is
// NPD, not nd: the writer stores whole register columns (rows >= nd are zeros) under a compile-time bound
__host__ __device__ inline size_t crf_rhs_doubles(int nd, int npd) { return (size_t)npd * npd; }

// bit (lane + shift) of the result = bit lane of b, for any shift in (-64, 64)
__device__ __forceinline__ unsigned long long crf_place(unsigned long long b, int shift) {
  return shift >= 0 ? (shift < 64 ? b << shift : 0ull) : (-shift < 64 ? b >> (-shift) : 0ull);
}

// NC = columns of [B_st | B_dy | A_dy | C_dy | D] per lane: 2 for h + 3 nd + k <= 128, 3 up to 192 (n = 46 .. 64)
// DBG (round 12): the stamped instance.  Shader cycles of draw 0 go to dbg (int64[16]): [0..4] the five stamps of crc_iterate,
// [5] final solve, [6] total, [7] iterations, [8] phase-1 loads + scans (static mask, index tables, the columns' loads),
// [9] the h reflectors, [10] deposit (column masks, tables, W, the parked right-hand sides, the register blocks), [11] phase 3;
// (round 13) [12] the static mask alone (part of [8]), and of phase 3: [13] the gather of y through prow, [14]
// crd_inflate_prepare, [15] crd_inflate_chunk up to its scatter -- the rest of [11] is the zero and scatter stores.
// (round 16) A draw that skips the static rows stamps the same places: [14] and [15] then read next to nothing.
// (round 17) The refinement branch of the iterations is counted over the WHOLE batch, not draw 0 (a few draws in a thousand take
// it): atomic adds of every draw that refined into [16] draws, [17] refinements, [18] cycles of the residuals, [19] of the
// second eliminations, [20] of the whole branch, [21] / [22] / [23] draws that refined in one / two / three or more iterations.
// With DBG = false nothing of it is compiled: the listing of the default instance is the one without the flag.
// NOREFINE (round 17): the iteration without its refinement branch (dsge_debug_cr_refine(1), a measuring tool: results change).
// REPLAY (round 17): crc_iterate's, on for the instances of two waves per SIMD.
template <int BSF, int BSD, int NC, bool DBG = false, bool NOREFINE = false, bool REPLAY = false>
__device__ __forceinline__ void cr_fused_body(const double* __restrict__ A, const double* __restrict__ B,
                                              const double* __restrict__ C, const double* __restrict__ D, int batch, int n,
                                              int k, int h, int max_iter, double tol, double* __restrict__ top,
                                              double* __restrict__ rhs, double* __restrict__ T_out,
                                              double* __restrict__ R_out, int32_t* __restrict__ status,
                                              int32_t* __restrict__ n_iter_out,
                                              unsigned long long* __restrict__ colmask_out,
                                              const double* __restrict__ Z, int z_batched, int p,
                                              long long* __restrict__ dbg = nullptr) {
  using SM = CrfSmem<BSF, BSD>;
  constexpr int NMF = SM::NMF, NPD = SM::NPD, LDW = SM::LDW, HM = CRD_HMAX;
  static_assert(NPD <= NMF, "the reduced tile is no larger than the full one");
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* W = smem;
  double* G1 = W + NPD;
  double* Lbuf = W + NPD * LDW;
  double* Ybuf = Lbuf + NPD * BSD;
  typedef typename SM::idx_t idx_t;
  int* prow = (int*)(smem + SM::dbl);
  idx_t* cmap = (idx_t*)(prow + NPD);
  idx_t* posS = cmap + NPD;
  idx_t* posL = posS + NPD;
  idx_t* rsrc = posL + NPD;
  idx_t* dyi = rsrc + NPD;
  idx_t* sti = dyi + 64;
  const int lane = threadIdx.x, lr = lane >> 3, lc = lane & 7;
  const int nd = n - h;
  const int draw = blockIdx.x;  // one draw per workgroup (see cr_deflate_kernel)
  if (draw >= batch) return;
  const size_t off = (size_t)draw * n * n, offk = (size_t)draw * n * k;
  auto hand_over = [&]() {  // the full-size kernel solves this draw
    if (lane == 0) {
      status[draw] = DSGE_ST_INTERNAL_RERUN;
      if (colmask_out) colmask_out[draw] = ~0ull;
    }
  };
  if (colmask_out && lane == 0) colmask_out[draw] = ~0ull;  // "not known" until the solve has succeeded

  // ---- phase 1: deflation ----------------------------------------------------------------------------------------------
  long long tk_start = 0, tk_ld = 0, tk_qr = 0, tk_mask = 0;
  if constexpr (DBG) tk_start = clock64();
  // (round 16) which variables the caller's filter observes: the loads of Z ride with the ones of A and C (a null Z reads row 0
  // of A in their place and the verdict below is "not skipped")
  unsigned long long obs = 0ull;
  unsigned long long smask = crd_static_mask<NMF>(A, C, off, n, lane, Z ? Z + (z_batched ? (size_t)draw * p * n : 0) : A + off,
                                                  Z ? p : 0, &obs);
  if constexpr (DBG) tk_mask = clock64();
  if (__popcll(smask) < h) return hand_over();
  smask = crd_first_bits(smask, h);
  // no deflated variable is observed: nobody reads the static rows of T and R (header comment, phase 3)
  const bool skip = Z != nullptr && (smask & obs) == 0ull;
  // (round 16) the lane index of the tables and the column sources, from two mbcnt and opaque (as in the reflector pass): at 256
  // registers `lane` is in scratch across the static mask, and with the Z registers live there the compiler reloaded it in front
  // of every use below, nine waits of a scratch round trip in a row
  int lane_t;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane_t));
  crd_index_tables(smask, n, lane_t, dyi, sti);
  double* tp = top + (size_t)draw * crd_top_doubles(n, k, h);
  double* rh = rhs + (size_t)draw * crf_rhs_doubles(nd, NPD);
  int s, l;
  unsigned long long state_cols = 0ull, maskS_red = 0ull, maskL_red = 0ull;  // (red: over the reduced variables)
  {
    double col[NC][NMF];
    bool act[NC];
    bool rst_bad = false;
    int lane_c;  // (a copy of its own for the column sources: two short live ranges, not one across both)
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane_c));
    crd_qr_chunk<NMF, NC>(A, B, C, D, off, offk, n, k, h, 0, dyi, sti, /*V=*/smem, tp, lane_c, col, act,
                          /*skip_zero_ac=*/true, DBG ? &tk_ld : nullptr, /*write_top=*/!skip, &rst_bad);
    // (round 16) the verdict for phase 3, parked in the one spare slot of the tables (h >= 1: dyi holds nd <= 63 entries) -- a
    // value carried across crc_iterate in a register is a register the iteration does not have.  Bit 0: skip the static rows,
    // bit 1: R_st is numerically singular, what crd_inflate_prepare would have found in the top block that was not written
    const bool rst_singular = __ballot(rst_bad) != 0ull;  // (every lane holds the same verdict: wave-uniform for the compiler)
    if (lane == 0) dyi[63] = (idx_t)(skip ? (rst_singular ? 3 : 1) : 0);
    if constexpr (DBG) tk_qr = clock64();
    // block (0 B, 1 A, 2 C, 3 D, -1 none) and column inside the block of this lane's columns 64 q + lane
    int blk[NC], dcol[NC];
    unsigned long long bS = 0ull, bL = 0ull;  // non-zero columns of A_dy (states) / C_dy (leads), over the reduced variables
#pragma unroll
    for (int q = 0; q < NC; ++q) {
      const int c = 64 * q + lane - h;
      blk[q] = -1;
      dcol[q] = 0;
      if (act[q] && c >= 0) {
        blk[q] = (c >= nd) + (c >= 2 * nd) + (c >= 3 * nd);
        dcol[q] = c - blk[q] * nd;
      }
      bool nz = false;  // (rows >= nd of a column are zeros by now)
#pragma unroll
      for (int r = 0; r < NMF; ++r) nz = nz || (col[q][r] != 0.0);
      bS |= crf_place(__ballot(blk[q] == 1 && nz), 64 * q - (h + nd));
      bL |= crf_place(__ballot(blk[q] == 2 && nz), 64 * q - (h + 2 * nd));
    }
    const unsigned long long ndmask = (nd >= 64) ? ~0ull : ((1ull << nd) - 1ull);
    const unsigned long long maskS = bS & ndmask, maskL = bL & ndmask;
    s = __popcll(maskS);
    l = __popcll(maskL);
    maskS_red = maskS;
    maskL_red = maskL;
    if (s + l > NPD || s + k > NPD) return hand_over();
    {  // the non-zero columns of T, in the caller's variable numbering: bit v <=> v is dynamic and a state
      const unsigned long long below = (1ull << lane) - 1ull;
      const bool dyn = (lane < n) && !((smask >> lane) & 1ull);
      const int dred = lane - __popcll(smask & below);
      state_cols = __ballot(dyn && ((maskS >> (dred & 63)) & 1ull));
    }
    wave_sync();  // every lane is done with V
    for (int idx = lane; idx < NPD * LDW; idx += 64) W[idx] = 0.0;
    if (lane < NPD) {
      const unsigned long long below = (1ull << lane) - 1ull;
      const bool isS = (maskS >> lane) & 1ull, isL = (maskL >> lane) & 1ull;
      const int ps = __popcll(maskS & below), pl = s + __popcll(maskL & below);
      posS[lane] = (idx_t)(isS ? ps : CrcPos<BSD, idx_t>::noS);
      posL[lane] = (idx_t)(isL ? pl : CrcPos<BSD, idx_t>::noL);
      if (isS) cmap[ps] = (idx_t)lane;
      if (isL) cmap[pl] = (idx_t)lane;
    }
    wave_sync();
    // the columns of the reduced system -> W = [B_dy | A_dy[:,S] C_dy[:,L]] (LDS); [A_dy[:,S] | D_red] -> global scratch
#pragma unroll
    for (int q = 0; q < NC; ++q) {
      const int d = dcol[q];
      const unsigned long long below = (1ull << d) - 1ull;
      int lcol = -1, gcol = -1;  // column of W / of the scratch record
      if (blk[q] == 0) {
        lcol = d;
      } else if (blk[q] == 1) {
        if ((maskS >> d) & 1ull) {
          gcol = __popcll(maskS & below);
          lcol = NPD + gcol;
        }
      } else if (blk[q] == 2) {
        if ((maskL >> d) & 1ull) lcol = NPD + s + __popcll(maskL & below);
      } else if (blk[q] == 3) {
        gcol = s + d;
      }
      // (round 13) all NPD rows, a compile-time bound: rows nd .. NPD - 1 of the column registers are +0.0 by now (shifted in
      // by the reflector passes, or cleared after the loads), W was zeroed just above, and the park's columns are NPD long --
      // the same bytes as under the wave-uniform test `r < nd`, without a scalar compare and a branch per store
      if (lcol >= 0) {
        double* dst = W + lcol;
#pragma unroll
        for (int r = 0; r < NPD; ++r) dst[r * LDW] = col[q][r];
      }
      if (gcol >= 0) {  // (column-major: a lane writes its column contiguously, unused columns are never touched)
        double* dst = rh + (size_t)gcol * NPD;
#pragma unroll
        for (int r = 0; r < NPD; ++r) dst[r] = col[q][r];
      }
    }
  }
  wave_sync();

  // ---- phase 2: cycle reduction on the reduced system ---------------------------------------------------------------------
  double A1[BSD][BSD], Ah[BSD][BSD], Rb[BSD][BSD];
  blk_load_lds<BSD>(A1, W, LDW, lr, lc);
  blk_load_lds<BSD>(Rb, G1, LDW, lr, lc);
  int vS[BSD], vL[BSD];
#pragma unroll
  for (int j = 0; j < BSD; ++j) {
    vS[j] = posS[lc * BSD + j];
    vL[j] = posL[lc * BSD + j];
  }
#pragma unroll
  for (int i = 0; i < BSD; ++i)
#pragma unroll
    for (int j = 0; j < BSD; ++j) Ah[i][j] = A1[i][j];
  wave_sync();
  bool converged, saw_nan;
  int it;
  long long ph[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  long long tk_dep = 0, tk_it = 0, tk_fin = 0;
  if constexpr (DBG) tk_dep = clock64();
  crc_iterate<BSD, DBG ? CRC_REFINE_STAMPED : (NOREFINE ? CRC_REFINE_NEVER : CRC_REFINE_RULE), REPLAY>(A1, Ah, Rb, W, Lbuf, Ybuf, prow, cmap, rsrc, posS, posL, nd, s, l, max_iter, tol, 0, lane,
                   DBG ? ph : nullptr, it, converged, saw_nan);
  if constexpr (DBG) {
    tk_it = clock64();
    if (dbg && lane == 0 && ph[8] > 0) {  // (before the early return of a draw that did not converge)
      unsigned long long* cnt = reinterpret_cast<unsigned long long*>(dbg);
      atomicAdd(cnt + 16, 1ull);
      for (int q = 0; q < 4; ++q) atomicAdd(cnt + 17 + q, (unsigned long long)ph[8 + q]);
      atomicAdd(cnt + (ph[8] >= 3 ? 23 : 20 + (int)ph[8]), 1ull);
    }
  }
  if (lane == 0) {
    status[draw] = converged ? DSGE_ST_OK : (DSGE_ST_NOT_CONVERGED | (saw_nan ? DSGE_ST_NAN : 0));
    if (n_iter_out) n_iter_out[draw] = it;
  }
  if (!converged) {  // zero policy matrices, as the full-size kernels write
    for (int idx = lane; idx < n * n; idx += 64) T_out[off + idx] = 0.0;
    for (int idx = lane; idx < n * k; idx += 64) R_out[offk + idx] = 0.0;
    return;
  }
  // [T_dy[:,S] | R_dy] = -A1_hat^-1 [A_dy[:,S] | D_red]  (cycle_reduction.py:181, shared.py:74-75; see cr_compact_body)
  wave_sync();
  int lane_f = lane;
  asm volatile("" : "+v"(lane_f));
  {
    // block coordinates re-derived from an opaque copy of the lane index, as in crc_iterate: what phase 1 computed from it
    // would otherwise be kept across the whole iteration -- in scratch, at 256 registers
    int lane_s = lane;
    asm volatile("" : "+v"(lane_s));
    const int lr_s = lane_s >> 3, lc_s = lane_s & 7;
    blk_store_lds<BSD>(Ah, W, LDW, lr_s, lc_s);
    // (round 12) the right-hand sides go from the park straight into the register block the elimination works on, as in the
    // iterations (gauss_jordan_blocked_rhs: the FMAs of the LDS form, operand for operand): column group 1 is neither
    // loaded nor stored per panel
    double t[BSD][BSD];
#pragma unroll
    for (int i = 0; i < BSD; ++i)
#pragma unroll
      for (int j = 0; j < BSD; ++j) {
        const int r = lr_s * BSD + i, c = lc_s * BSD + j;
        t[i][j] = (r < nd && c < s + k) ? rh[(size_t)c * NPD + r] : 0.0;
      }
    double inv_lo = 1e300, inv_hi = 0.0;  // (not looked at: the final solve is never refined)
    gauss_jordan_blocked_rhs<BSD>(W, LDW, nd, t, Lbuf, Ybuf, prow, lane_f, nullptr, inv_lo, inv_hi);
    blk_store_lds<BSD>(t, G1, LDW, lr_s, lc_s);  // rows in pivot order: row q of the solution sits in row prow[q]
  }
  wave_sync();

  // ---- phase 3: the static rows, scatter to the caller's variable order -------------------------------------------------
  if constexpr (DBG) tk_fin = clock64();
  // (round 16) The verdict of phase 1 first (bit 0: skip the static rows, bit 1: R_st singular), then ONE branch around the whole
  // phase: the full path below is the code it was -- the gather, the loads of the top block and the LDS arrays scheduled as one
  // piece -- and the skipping path is the gather and the stores.
  const int verdict = __builtin_amdgcn_readfirstlane((int)dyi[63]);
  double y[NPD];  // column `lane` of [T_dy | R_dy]: T_dy[:, v] = -X[:, posS(v)] for a state v, zero otherwise
  auto gather_y = [&]() {
    const int ntot = nd + k;
    int src = -1;
    if (lane < nd)
      src = (posS[lane] != CrcPos<BSD, idx_t>::noS) ? posS[lane] : -1;
    else if (lane < ntot)
      src = s + (lane - nd);
    // (read through prow where the elimination left the rows: no pass that restores the natural order)
    // (round 13) prow is the same for every lane: four entries per LDS read, up front, not one read in front of every row
    static_assert(SM::dbl % 2 == 0 && NPD % 4 == 0, "prow is read as int4");
    int pr[NPD];
#pragma unroll
    for (int q4 = 0; q4 < NPD / 4; ++q4) {
      const int4 v = reinterpret_cast<const int4*>(prow)[q4];
      pr[4 * q4] = v.x;
      pr[4 * q4 + 1] = v.y;
      pr[4 * q4 + 2] = v.z;
      pr[4 * q4 + 3] = v.w;
    }
#pragma unroll
    for (int q = 0; q < NPD; ++q) y[q] = (q < nd && src >= 0) ? -G1[(q < nd ? pr[q] : pr[0]) * LDW + src] : 0.0;
  };
  auto zero_static_columns = [&]() {  // static columns of T are exact zeros
    if (lane < n) {
#pragma unroll
      for (int s2 = 0; s2 < HM; ++s2)
        if (s2 < h) T_out[off + (size_t)lane * n + sti[s2]] = 0.0;
    }
  };
  long long tk_y = 0, tk_prep = 0, tk_z = 0, tk_x = 0;
  if (verdict != 0) {
    if (verdict & 2) return hand_over();  // (as the full path: before anything is written to T_out or R_out)
    gather_y();
    if constexpr (DBG) tk_y = tk_prep = clock64();
    zero_static_columns();
    if constexpr (DBG) tk_z = tk_x = clock64();
    crd_scatter_dynamic<NPD>(0, y, n, k, h, lane, dyi, sti, T_out + off, R_out + offk);
  } else {
    gather_y();
    wave_sync();  // the solution is in registers: W becomes the work space of the back-substitution
    if constexpr (DBG) tk_y = clock64();
    const CrdInflateLds<NPD> L(smem);
    if (!crd_inflate_prepare<NPD>(y, lane < nd + k, tp, n, k, h, lane, L, maskL_red)) return hand_over();
    if constexpr (DBG) tk_prep = clock64();
    zero_static_columns();
    if constexpr (DBG) tk_z = clock64();
    crd_inflate_chunk<NPD>(0, y, tp, n, k, h, lane, L, dyi, sti, T_out + off, R_out + offk, maskS_red, DBG ? &tk_x : nullptr);
  }
  // every other column of T is exactly zero (written so): the filter kernel need not look for them
  if (colmask_out && lane == 0) colmask_out[draw] = state_cols;
  if constexpr (DBG) {
    if (dbg && draw == 0 && lane == 0) {
      const long long tk_end = clock64();
      for (int q = 0; q < 5; ++q) dbg[q] = ph[q];
      dbg[5] = tk_fin - tk_it;
      dbg[6] = tk_end - tk_start;
      dbg[7] = it;
      dbg[8] = tk_ld - tk_start;
      dbg[9] = tk_qr - tk_ld;
      dbg[10] = tk_dep - tk_qr;
      dbg[11] = tk_end - tk_fin;
      dbg[12] = tk_mask - tk_start;
      dbg[13] = tk_y - tk_fin;
      dbg[14] = tk_prep - tk_y;
      dbg[15] = tk_x - tk_z;
    }
  }
}

template <int BSF, int BSD, int NC = 2>
__global__ __launch_bounds__(64) void cr_fused_kernel(const double* __restrict__ A, const double* __restrict__ B,
                                                       const double* __restrict__ C, const double* __restrict__ D, int batch,
                                                       int n, int k, int h, int max_iter, double tol,
                                                       double* __restrict__ top, double* __restrict__ rhs,
                                                       double* __restrict__ T_out, double* __restrict__ R_out,
                                                       int32_t* __restrict__ status, int32_t* __restrict__ n_iter_out,
                                                       unsigned long long* __restrict__ colmask_out,
                                                       const double* __restrict__ Z, int z_batched, int p) {
  cr_fused_body<BSF, BSD, NC>(A, B, C, D, batch, n, k, h, max_iter, tol, top, rhs, T_out, R_out, status, n_iter_out, colmask_out,
                              Z, z_batched, p);
}

// the register budget of two waves per SIMD for the 4 x 4 reduced tile (see cr_compact_kernel_occ2)
template <int BSF, int BSD>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void cr_fused_kernel_occ2(
    const double* __restrict__ A, const double* __restrict__ B, const double* __restrict__ C, const double* __restrict__ D,
    int batch, int n, int k, int h, int max_iter, double tol, double* __restrict__ top, double* __restrict__ rhs,
    double* __restrict__ T_out, double* __restrict__ R_out, int32_t* __restrict__ status, int32_t* __restrict__ n_iter_out,
    unsigned long long* __restrict__ colmask_out, const double* __restrict__ Z, int z_batched, int p) {
  cr_fused_body<BSF, BSD, 2, false, false, true>(A, B, C, D, batch, n, k, h, max_iter, tol, top, rhs, T_out, R_out, status,
                                                 n_iter_out, colmask_out, Z, z_batched, p);
}

// (round 17) ... and without the refinement branch of the iterations: what dsge_debug_cr_refine(1) launches to measure the
// branch's share of the launch.  Results differ from the default instance's on every draw that would have refined.
template <int BSF, int BSD>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void cr_fused_kernel_occ2_norefine(
    const double* __restrict__ A, const double* __restrict__ B, const double* __restrict__ C, const double* __restrict__ D,
    int batch, int n, int k, int h, int max_iter, double tol, double* __restrict__ top, double* __restrict__ rhs,
    double* __restrict__ T_out, double* __restrict__ R_out, int32_t* __restrict__ status, int32_t* __restrict__ n_iter_out,
    unsigned long long* __restrict__ colmask_out, const double* __restrict__ Z, int z_batched, int p) {
  cr_fused_body<BSF, BSD, 2, false, true, true>(A, B, C, D, batch, n, k, h, max_iter, tol, top, rhs, T_out, R_out, status,
                                                n_iter_out, colmask_out, Z, z_batched, p);
}

// The stamped instance of the kernel above (body flag DBG; dsge_debug_cr_fused_phases).  A kernel of its own because of the
// one argument more: the default kernel keeps its argument list and its code.
template <int BSF, int BSD>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void cr_fused_kernel_occ2_dbg(
    const double* __restrict__ A, const double* __restrict__ B, const double* __restrict__ C, const double* __restrict__ D,
    int batch, int n, int k, int h, int max_iter, double tol, double* __restrict__ top, double* __restrict__ rhs,
    double* __restrict__ T_out, double* __restrict__ R_out, int32_t* __restrict__ status, int32_t* __restrict__ n_iter_out,
    unsigned long long* __restrict__ colmask_out, const double* __restrict__ Z, int z_batched, int p,
    long long* __restrict__ dbg) {
  cr_fused_body<BSF, BSD, 2, true, false, true>(A, B, C, D, batch, n, k, h, max_iter, tol, top, rhs, T_out, R_out, status,
                                                n_iter_out, colmask_out, Z, z_batched, p, dbg);
}

}  // namespace dsge
