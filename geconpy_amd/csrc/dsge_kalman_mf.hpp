// Kalman filter log-likelihood, selector design matrix, covariance in the TILE LAYOUT of the FP64 matrix core: "kalman_mf_kernel"
// (round 6).
//
// Same algorithm, conventions and missing-data rules as kalman_nt_kernel (dsge_kalman_nt.hpp: exact reduction to the retained
// variables U = states u observed non-states, states first; stationary initial covariance by doubling; p x p inverse by row-per-lane
// Gauss-Jordan; P+ = P - K (P Zm' + jit_V K)' + jit_P I; steady-state switch with a register-resident mean recursion; the recursion
// of SURVEY.md Appendix B.4 for gEconpy/model/statespace.py:1151-1157) -- phases (a)-(d) and the steady loop are that kernel's code.
// What changed is where the covariance lives.  There: 3 x 3 register blocks on an 8 x 8 lane grid (24-wide tile for 18 variables:
// 2.4 x the flops), 432 FMAs + 144 LDS loads per lane for the two prediction products, 72 FMAs for the downdate, a shuffle
// transposition to symmetrise.  Here: the symmetric matrices P, Q are held as their UPPER 4 x 4 tiles in the result layout of
// v_mfma_f64_4x4x4f64 (dsge_mfma4.hpp; lane l of group g holds element (4 ta + (l >> 4), 4 tb + (l & 3)) of tile (ta, tb) =
// Mfma4Upper<TM>::tile(g, (l >> 2) & 3)): FOUR registers for 18 x 18 (5 x 5 tiles, 15 upper).  Per full step
//   (e) P+ = P + K (-V)'           8 issues with C = P (the rank-p downdate as a product),
//   (f) W  = P+[S,S] Tc'          35 issues, stored transposed,
//       P' = Tc W + Q             20 issues with C = Q, upper tiles only: symmetric by construction, no transposition,
// and the mean prediction rides along as column m of the last tile.  63 issues of 256 FMAs instead of ~500 FMAs of 64 plus their
// operand loads: tools/mfma_probe/product_probe.hip measured the two products alone at 0.61 x the VALU form's launch time.
// The register blocks are gone, so are their 96 operand registers.
//
// Capacity: s <= 4 KT state variables, m <= 4 TM retained variables, p <= 8, selector Z; a draw beyond it is flagged
// (DSGE_ST_INTERNAL_RERUN) for the next instance of the launcher's cascade, as in the other fast kernels.
#pragma once
#include <type_traits>

#include "dsge_kalman_nt.hpp"
#include "dsge_kalman_rec.hpp"
#include "dsge_mfma4.hpp"

namespace dsge {

template <int KT, int TM>
struct KmfSmem {
  static_assert(KT >= 1 && KT <= TM && TM <= 8, "tiles");
  static constexpr int NS = 4 * KT, NM = 4 * TM;  // padded state block, padded retained variables
  static constexpr int LDK = NS + 2;              // rows of Tc / W' / Pc (even: 16-byte aligned rows; + 2: conflict-free b128 reads)
  static constexpr int NR = 8 * ((NM + 7) / 8);   // rows of the update's panels (the update walks rows g8 + 8 ps)
  static constexpr int RP = NR / 8, PS = 10;
  static constexpr int WT = NM * LDK > NR * PS ? NM * LDK : NR * PS;  // W' buffer; the -V panel and the staged R alias it
  // doubles: Tc NM*LDK, Wt WT, Pc NS*LDK, PZt, Ks NR*PS each, av, af NR each, vv/dd/hh/zv 8 each; ints perm NR, zpos 8
  static constexpr size_t doubles = (size_t)NM * LDK + WT + (size_t)NS * LDK + 2 * (size_t)NR * PS + 2 * NR + 4 + 44 + NR / 2 + 4;
  static constexpr size_t bytes = sizeof(double) * doubles;
};

#ifndef KMF_WAVES
#define KMF_WAVES 2
#endif
// REC = true (round 6): the forward sweep of the gradient -- every step also writes its record for the reverse sweep
// (dsge_kalman_rec.hpp, KgRec<RBS>: the record of the 8 RBS-wide tile the reverse sweep runs on; 4 TM <= 8 RBS).  K, F, F^-1, a_t
// and the segment links as kalman_nt_kernel<.., REC> writes them; P+ in the TILE layout -- element g of lane l at [g 64 + l], the
// upper tiles straight from the registers, four coalesced stores for 18 variables instead of nine -- which the record announces in
// its layout word (KgRec::TS_LAYOUT) and the reverse sweep scatters into its LDS square.
template <int KT, int TM, bool DBG, bool REC = false, int RBS = (4 * TM + 7) / 8>
__global__ __launch_bounds__(64, KMF_WAVES) void kalman_mf_kernel(
    const double* __restrict__ T, const double* __restrict__ RQR, const double* __restrict__ P0, const double* __restrict__ Z,
    int z_batched, const double* __restrict__ dvec, int d_batched, const double* __restrict__ Hdiag, int h_batched,
    const double* __restrict__ y, int batch, int m_full, int p, int T_len, FilterConv cv, double missing_fill, double steady_tol,
    double* __restrict__ logp_out, int32_t* __restrict__ status, long long* __restrict__ dbg, int rerun_only,
    int32_t* __restrict__ steady_at, const int32_t* __restrict__ order, const double* __restrict__ Rsel,
    const double* __restrict__ qdiag, int q_batched, int k_shocks, const unsigned long long* __restrict__ colmask_in,
    double* __restrict__ rec_store = nullptr) {
  using SM = KmfSmem<KT, TM>;
  using RC = KgRec<RBS>;
  static_assert(!REC || (4 * TM <= 8 * RBS && Mfma4Upper<TM>::NG * 64 <= 8 * RBS * 8 * RBS), "the record's tile holds the filter's");
  using UX = Mfma4Upper<TM>;
  using MW = Mfma4Map<KT, TM>;
  constexpr int NS = SM::NS, NM = SM::NM, LDK = SM::LDK, NR = SM::NR, RP = SM::RP, PS = SM::PS, NG = UX::NG;
  // more than five groups of tiles (TM = 7: 28 upper tiles): the per-element tables of where a value is stored would push the kernel
  // past 256 registers -- the Pc offsets are recomputed where they are used and the selector values come from an LDS table
  constexpr bool LEAN = NG > 5;
  // the steady test's old values of the state block are requested at the top of the step where there are registers for them: not in
  // the seven-group instances, nor in the record instance (at its 256 registers four more doubles across the elimination are scratch)
  constexpr bool OLD_EARLY = !LEAN && !REC;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* Tc = smem;                // NM x LDK   transition, states-first ordering (columns >= s exactly zero)
  double* Wt = Tc + NM * LDK;       // WT         W' : Wt[j][k] = (P+[S,S] Tc')[k][j]
  double* Vs = Wt;                  //   alias: NR x PS  -V = -(P Zm' + jit_V K)     (phases d, e)
  double* Pc = Wt + SM::WT;         // NS x LDK   P+ restricted to the state block, full square
  double* PZt = Pc + NS * LDK;      // NR x PS    (predicted P) Z', unmasked
  double* Ks = PZt + NR * PS;       // NR x PS    K = P Zm' Finv
  double* av = Ks + NR * PS;        // NR + 2     predicted state (+ the dump slot of the mean's store)
  double* avd = av;
  double* af = av + NR + 2;         // NR + 2     filtered state (+ a dump slot)
  double* vv = af + NR + 2;         // 8 innovation (+ 2: dump slot)
  double* dd = vv + 10;             // 8 obs intercept
  double* hh = dd + 8;              // 8 diag(H)
  double* zv = hh + 8;              // 8 selector values
  double* zvt = zv + 8;             // 10: selector value by observation index, [8] = 0 (LEAN: the P Z' stores look their factor up)
  int* perm = (int*)(zvt + 10);     // NR: position -> original variable (states first)
  int* zpos = perm + NR;            // 8: position of the state each observation selects
  constexpr int W_DUMP = (NM - 1) * LDK + LDK - 1;   // padding slots that nothing reads: targets of the stores of dead blocks
  constexpr int TC_DUMP = (NM - 1) * LDK + LDK - 1;
  constexpr int PC_DUMP = (NS - 1) * LDK + LDK - 1;
  constexpr int PZ_DUMP = (NR - 1) * PS + PS - 1;
  const int lane = threadIdx.x;
  const int blk = (lane >> 2) & 3, i4 = lane & 3, kq = lane >> 4;
  const double LN2PI = 1.8378770664093453, LN2 = 0.6931471805599453;

  if (rerun_only && rerun_pass_is_empty(status, batch, order)) return;
  for (int bi = blockIdx.x; bi < batch; bi = batch) {  // (one draw per workgroup: see kalman_nt_kernel)
    const int draw = __builtin_amdgcn_readfirstlane(order ? order[bi] : bi);
    const int32_t st_in = __builtin_amdgcn_readfirstlane(status[draw]);
    if (rerun_only) {
      if (st_in != DSGE_ST_INTERNAL_RERUN) continue;
    } else if (st_in != 0) {
      if (lane == 0) logp_out[draw] = -INFINITY;
      continue;
    }
    const size_t off = (size_t)draw * m_full * m_full;
    wave_sync();
    for (int idx = lane; idx < (int)SM::doubles; idx += 64) smem[idx] = 0.0;

    // ---- exact state-space reduction to U = S u O, states first (kalman_nt_kernel's code) ---------------------------------
    const double* Zg = Z + (z_batched ? (size_t)draw * p * m_full : 0);
    bool is_state = false;
    const unsigned long long cm_in = colmask_in ? colmask_in[draw] : ~0ull;
    if (cm_in != ~0ull) {
      is_state = (lane < m_full) && ((cm_in >> lane) & 1ull);
    } else {
      const double* tcol = T + off + (lane < m_full ? lane : 0);
      for (int r0 = 0; r0 < m_full; r0 += 8) {
        double tv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) tv[u] = tcol[(size_t)(r0 + u < m_full ? r0 + u : m_full - 1) * m_full];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 8; ++u) is_state |= (tv[u] != 0.0);
      }
      is_state = is_state && (lane < m_full);
    }
    const unsigned long long colmask = __ballot(is_state);
    unsigned long long obsmask = 0ull, used = 0ull;
    bool ok = true;
    double zrow[8];
    {
      const int zl_lane = lane < m_full ? lane : m_full - 1;
#pragma unroll
      for (int o = 0; o < 8; ++o) zrow[o] = Zg[(size_t)(o < p ? o : (p > 0 ? p - 1 : 0)) * m_full + zl_lane];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int o = 0; o < 8; ++o) zrow[o] = (lane < m_full && o < p) ? zrow[o] : 0.0;
    }
#pragma unroll
    for (int o = 0; o < 8; ++o) {
      if (o < p) {
        const unsigned long long b = __ballot(zrow[o] != 0.0);
        if (__popcll(b) != 1 || ((used & b) != 0ull)) ok = false;
        used |= b;
        obsmask |= b;
      }
    }
    const unsigned long long extra = obsmask & ~colmask;  // observed non-states
    const int s = __popcll(colmask);
    const int m = s + __popcll(extra);
    ok = ok && (s <= NS) && (m <= NM) && (s >= 1);
    int my_pos = -1;
    if (lane < m_full) {
      const unsigned long long below = (1ull << lane) - 1ull;
      if ((colmask >> lane) & 1ull)
        my_pos = __popcll(colmask & below);
      else if ((extra >> lane) & 1ull)
        my_pos = s + __popcll(extra & below);
      if (my_pos >= 0 && my_pos < NR) perm[my_pos] = lane;
    }
#pragma unroll
    for (int o = 0; o < 8; ++o) {
      if (o < p && zrow[o] != 0.0) {
        zpos[o] = (my_pos >= 0 && my_pos < NR) ? my_pos : 0;
        zv[o] = zrow[o];
      }
    }
    if (!ok) {
      if (lane == 0) status[draw] = DSGE_ST_INTERNAL_RERUN;
      continue;
    }
    if (rerun_only && lane == 0) status[draw] = 0;
    wave_sync();

    // ---- this lane's elements of the symmetric matrices: (rr[g], cc[g]) of the upper tiles, and what they feed ---------------
    int rr[NG], cc[NG];
    bool inm[NG], up[NG];    // inside the m x m matrix; on or above the diagonal (the copy that is stored / mirrored)
    constexpr int NT_ = LEAN ? 1 : NG;
    int pcw0_[NT_], pcw1_[NT_];  // where the element goes in Pc (and its mirror image), or the dump slot
    int pzw0[NG], pzw1[NG];      // where it goes in the P Z' panel: row r at the observation selecting c, row c at the one selecting r
                                 // (LEAN: shifted left by four, the observation's index into zvt -- 8 = none -- in the low bits)
    double pzv0_[NT_], pzv1_[NT_];
    if (lane < 9) zvt[lane] = (lane < p) ? zv[lane] : 0.0;  // selector values by observation, zvt[8] = 0
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      int ta, tb;
      bool live;
      UX::tile(g, blk, ta, tb, live);
      const int r = 4 * ta + kq, c = 4 * tb + i4;
      rr[g] = r;
      cc[g] = c;
      inm[g] = live && r < m && c < m;
      up[g] = live && r <= c;
      int oc = -1, orr = -1;
      double zc = 0.0, zr = 0.0;
      for (int o = 0; o < p; ++o) {
        if (zpos[o] == c) {
          oc = o;
          zc = zv[o];
        }
        if (zpos[o] == r) {
          orr = o;
          zr = zv[o];
        }
      }
      const bool w0 = up[g] && inm[g] && oc >= 0, w1 = up[g] && inm[g] && r < c && orr >= 0;
      if constexpr (LEAN) {
        pzw0[g] = ((w0 ? r * PS + oc : PZ_DUMP) << 4) | (w0 ? oc : 8);
        pzw1[g] = ((w1 ? c * PS + orr : PZ_DUMP) << 4) | (w1 ? orr : 8);
      } else {
        const bool in_pc = up[g] && c < NS;  // (r <= c < NS)
        pcw0_[g] = in_pc ? r * LDK + c : PC_DUMP;
        pcw1_[g] = (in_pc && r < c) ? c * LDK + r : PC_DUMP;
        pzw0[g] = w0 ? r * PS + oc : PZ_DUMP;
        pzw1[g] = w1 ? c * PS + orr : PZ_DUMP;
        pzv0_[g] = zc;
        pzv1_[g] = zr;
      }
    }
    int rowa[NG], rowb[NG];  // operand rows of this lane's block in the three upper-tile products (computed once: mfma4_nt_upper_acc)
    mfma4_upper_rows<TM>(lane, rowa, rowb);
    auto pcw0 = [&](int g) {
      if constexpr (LEAN) return (up[g] && cc[g] < NS) ? rr[g] * LDK + cc[g] : PC_DUMP;
      else return pcw0_[g];
    };
    auto pcw1 = [&](int g) {
      if constexpr (LEAN) return (up[g] && cc[g] < NS && rr[g] < cc[g]) ? cc[g] * LDK + rr[g] : PC_DUMP;
      else return pcw1_[g];
    };
    wave_sync();

    // ---- T -> Tc (gathered: position -> original variable), Q and P in tile layout -----------------------------------------
    auto load_T = [&]() {
      lane_loop_batched<8>(m * s, lane,
                           [&](int idx) {
                             const int r = idx / s, c = idx - r * s;
                             return T[off + (size_t)perm[r] * m_full + perm[c]];
                           },
                           [&](int idx, double v) {
                             const int r = idx / s, c = idx - r * s;
                             Tc[r * LDK + c] = v;
                           });
    };
    double Qt[NG], Pt[NG];
    if (Rsel) {
      // sym(R diag(q) R')[U,U] from the selection matrix itself (m_full x k_shocks staged in the W' buffer; the launcher checked
      // that it fits), rqr_kernel's expression and summation order
      const int kp = (k_shocks + 1) & ~1;
      const double* Rg = Rsel + (size_t)draw * m_full * k_shocks;
      for (int idx = lane; idx < m_full * k_shocks; idx += 64) {
        const int i = idx / k_shocks, c = idx - i * k_shocks;
        Wt[i * kp + c] = Rg[idx];
      }
      const double* qd = qdiag + (q_batched ? (size_t)draw * k_shocks : 0);
      wave_sync();
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const double2* ri = reinterpret_cast<const double2*>(Wt + (inm[g] ? perm[rr[g]] : 0) * kp);
        const double2* rj = reinterpret_cast<const double2*>(Wt + (inm[g] ? perm[cc[g]] : 0) * kp);
        double a0 = 0.0, a1 = 0.0;
        for (int c2 = 0; 2 * c2 < kp; ++c2) {
          const double2 ti = ri[c2], tj = rj[c2];
          a0 = fma(ti.x * tj.x, qd[2 * c2], a0);
          a1 = fma(ti.y * tj.y, (2 * c2 + 1 < k_shocks) ? qd[2 * c2 + 1] : 0.0, a1);
        }
        Qt[g] = inm[g] ? a0 + a1 : 0.0;
      }
      wave_sync();
      for (int idx = lane; idx < m_full * kp; idx += 64) Wt[idx] = 0.0;  // (the filter relies on zero padding)
    } else {
#pragma unroll
      for (int g = 0; g < NG; ++g) Qt[g] = inm[g] ? RQR[off + (size_t)perm[rr[g]] * m_full + perm[cc[g]]] : 0.0;
    }
#pragma unroll
    for (int g = 0; g < NG; ++g) Pt[g] = (inm[g] && P0) ? P0[off + (size_t)perm[rr[g]] * m_full + perm[cc[g]]] : 0.0;
    load_T();
    wave_sync();
    // full square of the state block from the upper elements: Pc[r][c] and Pc[c][r]
#define KMF_STORE_PC()                        \
  do {                                        \
    _Pragma("unroll") for (int g = 0; g < NG; ++g) { \
      Pc[pcw0(g)] = Pt[g];                    \
      Pc[pcw1(g)] = Pt[g];                    \
    }                                         \
  } while (0)
    if (!P0) {
      // ---- P0 = dlyap(T, RQR)[U,U] by doubling on the reduced model (statespace.py:814-815): P += A_k P A_k', A_{k+1} = A_k^2 ----
#pragma unroll
      for (int g = 0; g < NG; ++g) Pt[g] = Qt[g];
      bool lyap_ok = false;
      for (int itl = 0; itl < 64; ++itl) {
        wave_sync();
        KMF_STORE_PC();
        wave_sync();
        mfma4_nt<KT, KT, TM, LDK>(Pc, Tc, lane, [&](int g, double d) {  // W = P[S,S] A_k', transposed
          const int at = (4 * MW::tb(g, blk) + i4) * LDK + 4 * MW::ta(g, blk) + kq;
          Wt[MW::live(g, blk) ? at : W_DUMP] = d;
        });
        using MA = Mfma4Map<TM, KT>;
        double a2r[MA::NG];
        mfma4_nn<KT, TM, KT, LDK>(Tc, Tc, lane, [&](int g, double d) { a2r[g] = d; });  // A_k[:,S] A_k[S,:]
        wave_sync();
        double dmax = 0.0, pmax = 0.0;
        mfma4_nt_upper_acc<KT, TM, LDK>(Tc, Wt, lane, rowa, rowb, [](int) { return 0.0; }, [&](int g, double d) {
          const double dlt = inm[g] ? d : 0.0;
          Pt[g] += dlt;
          dmax = nanmax(dmax, fabs(dlt));
          pmax = nanmax(pmax, fabs(Pt[g]));
        });
        wave_sync();
#pragma unroll
        for (int g = 0; g < MA::NG; ++g) {
          const int at = (4 * MA::ta(g, blk) + kq) * LDK + 4 * MA::tb(g, blk) + i4;
          Tc[MA::live(g, blk) ? at : TC_DUMP] = a2r[g];
        }
        dmax = wave_nanmax(dmax);
        pmax = wave_nanmax(pmax);
        if (!(dmax == dmax) || !(pmax < 1e300)) break;
        if (dmax <= 1e-17 * pmax) {
          lyap_ok = true;
          break;
        }
      }
      wave_sync();
      for (int idx = lane; idx < NM * LDK; idx += 64) Tc[idx] = 0.0;
      for (int idx = lane; idx < SM::WT; idx += 64) Wt[idx] = 0.0;  // (the filter relies on zero padding)
      wave_sync();
      load_T();
      if (!lyap_ok) {
        if (lane == 0) {
          status[draw] |= DSGE_ST_LYAP_FAIL;
          logp_out[draw] = -INFINITY;
        }
        continue;
      }
    }
    double* const rec_d = REC ? rec_store + (size_t)draw * RC::per_draw(T_len) : nullptr;  // this draw's record
    int seg_src = -1;                                                                       // source step of the running segment
    if constexpr (REC) {  // P_0, row-major NP x NP behind the last step (zero outside m x m), and the layout word
      constexpr int RNP = 8 * RBS;
      double* p0s = rec_d + (size_t)T_len * RC::STEP;
      for (int idx = lane; idx < RNP * RNP; idx += 64) {
        const int r = idx / RNP, c = idx - r * RNP;
        if (!(r < m && c < m)) p0s[idx] = 0.0;
      }
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        if (up[g] && inm[g]) {
          p0s[rr[g] * RNP + cc[g]] = Pt[g];
          p0s[cc[g] * RNP + rr[g]] = Pt[g];
        }
      }
      if (lane == 0) rec_d[RC::tail_state_off(T_len) + RC::TS_LAYOUT] = (double)(RC::LAYOUT_TILES + TM);
    }
    if (lane < 8) {
      dd[lane] = (dvec && lane < p) ? dvec[(d_batched ? (size_t)draw * p : 0) + lane] : 0.0;
      hh[lane] = (Hdiag && lane < p) ? Hdiag[(h_batched ? (size_t)draw * p : 0) + lane] : 0.0;
    }
    // P Z' panel of the predicted covariance (unmasked), from the upper elements and their mirror images
#define KMF_STORE_PZT()                                 \
  do {                                                  \
    _Pragma("unroll") for (int g = 0; g < NG; ++g) {    \
      if constexpr (LEAN) {                             \
        PZt[pzw0[g] >> 4] = zvt[pzw0[g] & 15] * Pt[g];  \
        PZt[pzw1[g] >> 4] = zvt[pzw1[g] & 15] * Pt[g];  \
      } else {                                          \
        PZt[pzw0[g]] = pzv0_[g] * Pt[g];                \
        PZt[pzw1[g]] = pzv1_[g] * Pt[g];                \
      }                                                 \
    }                                                   \
  } while (0)
    KMF_STORE_PZT();
    wave_sync();

    const int r8 = lane & 7, g8 = lane >> 3;  // the update runs on 8 replicas of an 8-lane group: lane -> row r8 of F
    const int r_zpos = (r8 < p) ? zpos[r8] : 0;
    const double r_zv = (r8 < p) ? zv[r8] : 0.0, r_dd = dd[r8], r_hh = hh[r8];
    const bool fold_a = m < NM;  // a spare padding column: the mean prediction rides along in the X product as column m

    double quad_sum = 0.0, quad_comp = 0.0;  // Kahan sum of v' Finv v over observed steps
    double ld_mant = 1.0;                    // prod of pivots = mant * 2^exp
    int ld_exp = 0;
    int n_ll_steps = 0, n_obs_entries = 0;
    long long ph[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const long long tk_start = DBG ? clock64() : 0;
    int steady_step = -1;
    const int r8c = (r8 < p) ? r8 : (p > 0 ? p - 1 : 0);
    double yt_next = (T_len > 0) ? y[r8c] : 0.0;
    for (int t = 0; t < T_len; ++t) {
      long long tk0 = DBG ? clock64() : 0;
      // ---- (a) missing-data mask; every LDS operand of the update is requested up front ------------------------------
      const double yt = yt_next;
      yt_next = y[(size_t)((t + 1 < T_len) ? t + 1 : t) * p + r8c];
      const bool obs = (r8 < p) && (yt == yt) && (yt != missing_fill);
      const unsigned long long omask = __ballot(obs) & 0xffull;
      const int n_obs = __popcll(omask);
      double* const sg = REC ? rec_d + (size_t)t * RC::STEP : nullptr;  // the record of this (full) step
      if constexpr (REC) {
        if (lane < 8 * RBS) sg[RC::OFF_A + lane] = (lane < NR) ? av[lane] : 0.0;
        if (lane == 0) {
          sg[RC::OFF_SRC] = (double)t;
          sg[RC::OFF_PREV] = (double)seg_src;
        }
        seg_src = t;
      }
      double2 fr2[4], pz2[RP][4];
      double pzo[RP], avi[RP];
#pragma unroll
      for (int q2 = 0; q2 < 4; ++q2) fr2[q2] = *reinterpret_cast<const double2*>(&PZt[r_zpos * PS + 2 * q2]);
      const double a_sel = av[r_zpos];
      auto load_panel = [&]() {
#pragma unroll
        for (int ps = 0; ps < RP; ++ps) {
          const int i = g8 + 8 * ps;
#pragma unroll
          for (int q2 = 0; q2 < 4; ++q2) pz2[ps][q2] = *reinterpret_cast<const double2*>(&PZt[i * PS + 2 * q2]);
          pzo[ps] = PZt[i * PS + r8];
          avi[ps] = av[i];
        }
      };
      if constexpr (!LEAN) load_panel();  // (LEAN: requested in phase (d) -- 72 registers less across the elimination)
      // the steady test's old values of the state block, requested here with the rest: Pc is not written between the previous step's
      // KMF_STORE_PC and this one's, and the latency sits under the elimination (otherwise: read in phase (e))
      double oldv[OLD_EARLY ? NG : 1];
      if constexpr (OLD_EARLY) {
#pragma unroll
        for (int g = 0; g < NG; ++g) oldv[g] = Pc[pcw0(g)];
      }
      __builtin_amdgcn_sched_barrier(0);
      bool steady = false;
      double pm = 0.0;  // max |P_{t|t-1}| = the largest diagonal entry (P is positive semi-definite)
      if (steady_tol > 0.0) {
        double pscale = 0.0;
#pragma unroll
        for (int g = 0; g < NG; ++g) pscale = fmax(pscale, (rr[g] == cc[g]) ? fabs(Pt[g]) : 0.0);
        if constexpr (!LEAN) {
          // (rr == cc only where lane & 3 == lane >> 4, every other lane holds +0; fmax has dropped a NaN diagonal)
          pm = tile_diag_wave_max(pscale);
        } else {  // (seven groups: the scale in a scalar register pair, the vector pair would be eight bytes of scratch more)
          const unsigned hi = (unsigned)__double2hiint(pscale), lo = (unsigned)__double2loint(pscale);
          const unsigned mhi = wave_max_u32(hi);
          const unsigned mlo = wave_max_u32(hi == mhi ? lo : 0u);
          pm = __hiloint2double((int)mhi, (int)mlo);
        }
      }
      // ---- (b) innovation v[r8] and row r8 of F = Zm P Zm' + Hm + jitter I, replicated over the eight 8-lane groups ----------
      const double c_r = obs ? r_zv : 0.0;
      const double v_r = (obs ? yt : 0.0) - (((obs || !cv.mask_d) ? r_dd : 0.0) + c_r * a_sel);
      const double dg = (r8 < p) ? ((obs ? r_hh : 0.0) + cv.jit_F) : 1.0;
      vv[lane < 8 ? lane : 8] = v_r;  // (entry 8: a slot for the other lanes -- no branch)
      asm volatile("" ::: "memory");
      double fr[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const double tq = (q & 1) ? fr2[q >> 1].y : fr2[q >> 1].x;
        const double wq = ((omask >> q) & 1ull) ? 1.0 : 0.0;  // wave-uniform
        // F[r8][q] = (c_r tq) wq, + dg on the diagonal, as ONE fused multiply-add with the addend selected: on the diagonal the
        // contraction the compiler made of `f + dg` anyway (now spelled out), elsewhere x wq + (-0.0) == x wq bit for bit for every x
        // (a zero product keeps its sign against -0.0, everything else is the rounded product) -- a multiply per column less
        fr[q] = fma(c_r * tq, wq, (q == r8) ? dg : -0.0);
      }
      if constexpr (REC) {
        if (lane < 8) {
#pragma unroll
          for (int q = 0; q < 8; ++q) sg[RC::OFF_F + lane * 8 + q] = fr[q];
        }
      }
      // ---- (c) Finv by Gauss-Jordan, one row per lane (SPD: no pivoting); the pivot row arrives by row broadcasts ------------
      double step_mant = 1.0, inv_own = 1.0;
      int step_exp = 0;
      // (p >= 7: pivots 0..6 unconditionally, pivot 7 only when there is an eighth observation: a row beyond p -- like the row of a missing
      //  observation -- is a row of the identity, pivot 1, multipliers 0, mantissa 0.5 x 2^1: a no-op.  Seven branches `j < p` cut the
      //  chain into basic blocks the scheduler could not overlap; one uniform branch at the end does not)
      auto pivot = [&](auto jt) {
        constexpr int j = decltype(jt)::value;
        // The rows are replicated over the 8-lane groups, so lane j of every 16-lane row holds pivot row j: its entries are taken
        // inside the consuming instruction (row_newbcast, dsge_device.hpp), the pivot by one broadcast move, the other seven by the
        // FMAs that use them -- fma(-ci, fr[q] of lane j, fr[q]), the operation it was with the row read into SGPR pairs first.
        // Every lane is active here (the time loop's branches are wave-uniform).  DPP wait states, by construction: pivot 0 reads
        // what the F build has just written and carries the nops (j == 0); a later pivot's move reads fr[j], the FIRST column the
        // previous statement wrote (six FMAs behind it); its FMAs sit behind that move and the reciprocal chain, which depend on
        // the previous statement, and fr[j - 1] -- the select below, which may be scheduled late -- is the LAST column they read.
        const double pj = row_bcast_f64<j, j == 0>(fr[j]);
        // (ONE Newton step on v_rcp_f64: 2.2e-15 relative, tools/latency_probe/rcp_probe.hip -- the multipliers and the final
        //  row scaling of a 7 x 7 inverse whose conditioning costs more digits than that; the determinant takes the pivots
        //  themselves.  Two dependent FMAs less on the chain of every pivot)
        double inv = __builtin_amdgcn_rcp(pj);
        inv = inv * fma(-pj, inv, 2.0);
        const bool is_j = (r8 == j);
        const double ci = is_j ? 0.0 : fr[j] * inv;
        pivot_row_bcast_update<j, j == 0>(fr, ci);
        // fr[j] = is_j ? 1.0 : -ci.  The low word is ci's own (ci is +0.0 in the pivot lane, and 1.0 ends in 32 zero bits): one
        // select, on the high word, instead of two
        fr[j] = __hiloint2double(is_j ? 0x3ff00000 : (__double2hiint(ci) ^ (int)0x80000000), __double2loint(ci));
        inv_own = is_j ? inv : inv_own;
        int e;
        step_mant *= frexp(pj, &e);
        step_exp += e;
      };
      if (p >= 7) {
        pivot(std::integral_constant<int, 0>{});
        pivot(std::integral_constant<int, 1>{});
        pivot(std::integral_constant<int, 2>{});
        pivot(std::integral_constant<int, 3>{});
        pivot(std::integral_constant<int, 4>{});
        pivot(std::integral_constant<int, 5>{});
        pivot(std::integral_constant<int, 6>{});
        if (p > 7) pivot(std::integral_constant<int, 7>{});
      } else {  // (few observables: the no-op pivots would cost more than the branches)
        pivot(std::integral_constant<int, 0>{});
        if (p > 1) pivot(std::integral_constant<int, 1>{});
        if (p > 2) pivot(std::integral_constant<int, 2>{});
        if (p > 3) pivot(std::integral_constant<int, 3>{});
        if (p > 4) pivot(std::integral_constant<int, 4>{});
        if (p > 5) pivot(std::integral_constant<int, 5>{});
      }
      if constexpr (REC) {
        if (lane < 8) {
#pragma unroll
          for (int q = 0; q < 8; ++q) sg[RC::OFF_FI + lane * 8 + q] = fr[q] * inv_own;
        }
      }
      {
        const double2* vv2 = reinterpret_cast<const double2*>(vv);
        double w0 = 0.0, w1 = 0.0;
#pragma unroll
        for (int q2 = 0; q2 < 4; ++q2) {
          const double2 vq = vv2[q2];
          w0 = fma(fr[2 * q2], vq.x, w0);
          w1 = fma(fr[2 * q2 + 1], vq.y, w1);
        }
        {  // (a step without any observed entry contributes nothing: selects on the wave-uniform condition instead of a branch,
           //  which would end the basic block between the elimination and the gain)
          const bool any = n_obs > 0;
          const double yk = ((lane < 8) ? (v_r * inv_own) * (w0 + w1) : 0.0) - quad_comp;
          const double tk = quad_sum + yk;
          quad_comp = any ? (tk - quad_sum) - yk : quad_comp;
          quad_sum = any ? tk : quad_sum;
          int e;
          const double lm = frexp(ld_mant * step_mant, &e);
          ld_mant = any ? lm : ld_mant;
          ld_exp += any ? e + step_exp : 0;
          n_ll_steps += any ? 1 : 0;
          n_obs_entries += n_obs;
        }
      }
      if constexpr (DBG) {
        const long long tk1 = clock64();
        ph[0] += tk1 - tk0;
        tk0 = tk1;
      }
      // ---- (d) K = (P Zm') Finv, V = P Zm' + jit_V K (stored negated), a+ = a + K v -----------------------------------------
      if constexpr (LEAN) load_panel();
#pragma unroll
      for (int ps = 0; ps < RP; ++ps) {
        const int i = g8 + 8 * ps;
        double k0 = 0.0, k1 = 0.0;
#pragma unroll
        for (int q2 = 0; q2 < 4; ++q2) {
          k0 = fma(pz2[ps][q2].x, fr[2 * q2], k0);
          k1 = fma(pz2[ps][q2].y, fr[2 * q2 + 1], k1);
        }
        const double kk = obs ? (k0 + k1) * inv_own : 0.0;
        Ks[i * PS + r8] = kk;
        Vs[i * PS + r8] = -fma(cv.jit_V, kk, obs ? pzo[ps] : 0.0);
        double part = kk * v_r;
        part += dpp_perm_f64<0xB1>(part);   // quad_perm [1,0,3,2]
        part += dpp_perm_f64<0x4E>(part);   // quad_perm [2,3,0,1]
        part += dpp_perm_f64<0x141>(part);  // row_half_mirror: the other quad of the 8-lane group
        af[(r8 == 0) ? i : NR] = avi[ps] + part;  // (entry NR: a slot for the lanes that own nothing -- no branch)
      }
      wave_sync();  // #2
      if constexpr (REC) {
        for (int idx = lane; idx < 8 * RBS * 8; idx += 64) sg[RC::OFF_K + idx] = ((idx >> 3) < NR) ? Ks[(idx >> 3) * PS + (idx & 7)] : 0.0;
      }
      if constexpr (DBG) {
        const long long tk1 = clock64();
        ph[1] += tk1 - tk0;
        tk0 = tk1;
      }
      // ---- (e) P+ = P + K (-V)' + jit_P I on the matrix core (C = P), then the state block -> Pc (full square) ---------------
      {
        double dmax = 0.0;
        mfma4_nt_upper_acc<2, TM, PS>(Ks, Vs, lane, rowa, rowb, [&](int g) { return Pt[g]; },
                                      [&](int g, double d) {
                                        const double pn = inm[g] ? d + ((rr[g] == cc[g]) ? cv.jit_P : 0.0) : 0.0;
                                        Pt[g] = pn;
                                      });
        if constexpr (REC) {  // P+ in tile layout, straight from the registers
#pragma unroll
          for (int g = 0; g < NG; ++g) sg[(size_t)g * 64 + lane] = Pt[g];
        }
        if (steady_tol > 0.0) {
          if constexpr (OLD_EARLY) {  // (old values: read at the top of the step)
#pragma unroll
            for (int g = 0; g < NG; ++g) dmax = fmax(dmax, (pcw0(g) != PC_DUMP) ? fabs(Pt[g] - oldv[g]) : 0.0);
          } else {
            // (one at a time, the registers are needed elsewhere.  Read UNCONDITIONALLY -- volatile: under the predicate
            //  the compiler turned each read into a branch with its own wait -- and through an LDS pointer: a volatile access through
            //  a generic pointer is a flat load, a round trip through the vector memory path with a full wait behind it)
            using LdsCVD = const volatile __attribute__((address_space(3))) double*;
#pragma unroll
            for (int g = 0; g < NG; ++g) {
              const int at = pcw0(g);
              const double old = *(LdsCVD)(&Pc[at]);
              dmax = fmax(dmax, (at != PC_DUMP) ? fabs(Pt[g] - old) : 0.0);
            }
          }
          steady = (t > 0) && (__ballot(!(dmax <= steady_tol * pm)) == 0ull);
        }
        // (no fence between the reads of the old state block and its stores: same element type, and LDS executes a wavefront's
        //  accesses in program order)
        KMF_STORE_PC();
      }
      // the filtered mean as row m of W': column m of X is then Tc a+ (rows >= m of Tc are zero: row m of W' feeds nothing else)
      double af_l = 0.0;
      if (fold_a) {
        af_l = af[lane < NR ? lane : 0];
      } else if (lane < m) {
        const double2* trow2 = reinterpret_cast<const double2*>(Tc + lane * LDK);
        const double2* af2 = reinterpret_cast<const double2*>(af);
        double s0 = 0.0, s1 = 0.0;
        for (int kk = 0; 2 * kk < s; ++kk) {
          const double2 tv2 = trow2[kk], fv = af2[kk];
          s0 = fma(tv2.x, fv.x, s0);
          s1 = fma(tv2.y, fv.y, s1);
        }
        av[lane] = s0 + s1;
      }
      wave_sync();  // #3
      if constexpr (DBG) {
        const long long tk1 = clock64();
        ph[2] += tk1 - tk0;
        tk0 = tk1;
      }
      // ---- (f) predict: W = P+[S,S] Tc' (stored transposed);  P' = Tc W + Q (upper tiles, C = Q) ---------------------------------
      mfma4_nt<KT, KT, TM, LDK>(Pc, Tc, lane, [&](int g, double d) {
        const int at = (4 * MW::tb(g, blk) + i4) * LDK + 4 * MW::ta(g, blk) + kq;
        Wt[MW::live(g, blk) ? at : W_DUMP] = d;
      });
      Wt[(fold_a && lane < NS) ? m * LDK + lane : W_DUMP] = af_l;  // (after the W stores: LDS keeps a wavefront's program order)
      wave_sync();  // #4
      if constexpr (DBG) {
        const long long tk1 = clock64();
        ph[3] += tk1 - tk0;
        tk0 = tk1;
      }
      mfma4_nt_upper_acc<KT, TM, LDK>(Tc, Wt, lane, rowa, rowb, [&](int g) { return Qt[g]; },
                                      [&](int g, double d) {
                                        // column m: the predicted mean (Q is zero there); everything else outside m x m: padding
                                        const bool is_mean = fold_a && cc[g] == m && rr[g] < m && up[g];
                                        // (entry NR: a slot of its own for the rest, which nothing reads -- whatever they hold;
                                        //  seven groups: the zero, that form is four bytes of scratch less there)
                                        avd[is_mean ? rr[g] : NR] = (LEAN && !is_mean) ? 0.0 : d;
                                        Pt[g] = inm[g] ? d : 0.0;
                                      });
      KMF_STORE_PZT();
      wave_sync();  // #5
      if constexpr (DBG) {
        const long long tk1 = clock64();
        ph[4] += tk1 - tk0;
        tk0 = tk1;
      }
      if (!steady) continue;
      // ==== steady-state steps: mean recursion only, while the missing-data mask stays the same (kalman_nt_kernel's loop) ====
      if (steady_step < 0) steady_step = t + 1;
      {
        double trow[NS], finv_row[8], kr_ss[8];
        double av_reg = (lane < m) ? av[lane] : 0.0;
#pragma unroll
        for (int kk = 0; kk < NS; ++kk) trow[kk] = (lane < NM) ? Tc[lane * LDK + kk] : 0.0;  // columns >= s are zero
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          finv_row[q] = (lane < 8) ? fr[q] * inv_own : 0.0;
          kr_ss[q] = (lane < m) ? Ks[lane * PS + q] : 0.0;
        }
        // What does not change while the loop runs (it runs while the mask is omask): which of this lane's entries is observed, the
        // intercept that goes with it, the 0 / 1 factor of the selector.
        // The innovation is computed on lanes 0..p-1 of EVERY 16-lane row (there lane & 15 == r8, and y, the selector and the
        // intercept are at hand per r8), so that the sums below take entry o from lane o of the lane's own row.
        const bool in_p = (lane & 15) < p;
        const bool obs_l = in_p && ((omask >> r8) & 1ull);
        const double d_l = (obs_l || !cv.mask_d) ? r_dd : 0.0, one_l = obs_l ? 1.0 : 0.0;
        const unsigned long long pbits = (1ull << p) - 1ull;  // (p <= 8)
        // NC: columns of Tc the mean prediction runs over -- the padded state block, or two less when the last pair of columns is
        // padding (18 state variables in 20 columns: trow is +0 there and s0, s1 are never -0, so fma(+0, afi, acc) == acc).  That, and
        // the missing select on the predicted mean below, assume a FINITE filtered mean: with an Inf or NaN in afi the parent's
        // 0 * afi poisoned every lane's sum where this one skips the column, and lanes >= m (which the record's OFF_A store may cover)
        // hold NaN instead of 0.  Such a draw's likelihood is already non-finite and flagged DSGE_ST_FILTER_NONFINITE either way.
        // (The row broadcasts of afi change nothing in that for lanes 0..31, which is all that is ever stored: column kk is the
        // value of lane kk there, finite or not.  Lanes 32..63 multiply their zero row by the entries of lanes 32..63.)
        auto steady_loop = [&](auto nc_tag) {
          constexpr int NC = decltype(nc_tag)::value;
          while (t + 1 < T_len) {
            const double yt_s = yt_next;
            // the mask test as a scalar compare: the ballot of the comparison itself, cut to the p observations
            // (one ballot per comparison: each is the comparison's own scalar result, their conjunction a scalar AND)
            if ((__builtin_amdgcn_ballot_w64(yt_s == yt_s) & __builtin_amdgcn_ballot_w64(yt_s != missing_fill) & pbits) != omask) break;
            ++t;
            yt_next = y[(size_t)((t + 1 < T_len) ? t + 1 : t) * p + r8c];
            if constexpr (REC) {
              double* sgs = rec_d + (size_t)t * RC::STEP;
              if (lane < 8 * RBS) sgs[RC::OFF_A + lane] = av_reg;
              if (lane == 0) sgs[RC::OFF_SRC] = (double)seg_src;
            }
            const double av_sel = __shfl(av_reg, r_zpos, 64);
            const double v_s = in_p ? (obs_l ? yt_s : 0.0) - (d_l + one_l * (r_zv * av_sel)) : 0.0;
            // w0 = fma(finv_row[o], v[o], w0), a0 = fma(kr_ss[o], v[o], a0) over o = 0, 2, 4, 6, w1 and a1 over o = 1, 3, 5, 7, with
            // v[o] broadcast from lane o of the row inside the FMA.  (Rows 1..3 now hold v_s too: finv_row is zero there, their
            // term of the quadratic form below is an exact zero for a finite v_s.)
            double w0 = 0.0, w1 = 0.0, a0 = av_reg, a1 = 0.0;
            steady_sums_row_bcast(w0, w1, a0, a1, v_s, finv_row, kr_ss);
            if (n_obs > 0) {
              const double yk = v_s * (w0 + w1) - quad_comp;  // lanes >= 8 hold finv_row = 0
              const double tk = quad_sum + yk;
              quad_comp = (tk - quad_sum) - yk;
              quad_sum = tk;
              int e;
              ld_mant = frexp(ld_mant * step_mant, &e);
              ld_exp += e + step_exp;
              ++n_ll_steps;
              n_obs_entries += n_obs;
            }
            const double afi = a0 + a1;
            // a_pred = Tc afi with afi[kk] broadcast inside the FMA.  Entry kk of afi sits in lane kk, row kk / 16, and every lane
            // below NM <= 28 (rows 0 and 1) consumes it: two lane swaps (one per half of the double) first give both rows both
            // halves of afi -- ax: entries 0..15, ay: entries 16..31, needed beyond 16 columns only -- then s0 takes the even columns
            // and s1 the odd ones, ascending, from +0.  Wait states: the sums are ONE statement that opens with the two moves zeroing
            // s0 and s1 -- they stand between the swaps (VALU writes of ax and ay) and the first broadcast, whatever the compiler
            // schedules around the statement.  All 64 lanes are active: the loop's branches are wave-uniform.
            double s0 = 0.0, s1 = 0.0;
            if constexpr (TM < 7) {
              double ax, ay;
              rows01_pair_f64<(NC > 16)>(afi, ax, ay);
              if constexpr (NC > 16) matvec_sums_row_bcast<NC>(s0, s1, ax, ay, trow);
              else matvec_sums_row_bcast<NC>(s0, s1, ax, ax, trow);
            } else {
              // TM = 7 (256 registers, 84 bytes of scratch) keeps the read-lanes: with the swaps it spilled four bytes more.
              // Batches of six to eight columns into SGPR pairs of their own, then the batch's FMAs in their order: a read-lane
              // into the pair the previous FMA still reads needs a hazard nop in front of every FMA; all the columns at once
              // would spill scalar registers elsewhere in the kernel.
#pragma unroll
              for (int b0 = 0; b0 < NC; b0 += 6) {
                const int b1 = (NC - b0 <= 8) ? NC : b0 + 6;
                double afs[8];
#pragma unroll
                for (int kk = b0; kk < b1; ++kk) afs[kk - b0] = readlane_f64(afi, kk);
#pragma unroll
                for (int kk = b0; kk < b1; kk += 2) {
                  s0 = fma(trow[kk], afs[kk - b0], s0);
                  s1 = fma(trow[kk + 1], afs[kk + 1 - b0], s1);
                }
                if (b1 == NC) break;
                __builtin_amdgcn_sched_barrier(0);
              }
            }
            av_reg = s0 + s1;  // (rows >= m of Tc are zero: +0 there for a finite afi, no select)
            if constexpr (DBG) ++ph[6];
          }
        };
        if (s <= NS - 2)
          steady_loop(std::integral_constant<int, NS - 2>{});
        else
          steady_loop(std::integral_constant<int, NS>{});
        if (lane < m) av[lane] = av_reg;
      }
      wave_sync();
      if constexpr (DBG) ph[5] += clock64() - tk0;
    }
#undef KMF_STORE_PZT
#undef KMF_STORE_PC
    if (DBG && dbg && draw == 0 && lane == 0) {
      ph[7] = clock64() - tk_start;
      for (int k = 0; k < 8; ++k) dbg[k] = ph[k];
    }
    const double quad_total = wave_sum_dpp(quad_sum - quad_comp);
    if (lane == 0) {
      const double logdet = log(ld_mant) + (double)ld_exp * LN2;
      const double ll = -0.5 * (cv.ll_terms(n_ll_steps, n_obs_entries, p) * LN2PI + logdet + quad_total);
      logp_out[draw] = ll;
      if (steady_at) steady_at[draw] = steady_step;
      if (!((ll == ll) && (fabs(ll) < 1.797e308))) status[draw] |= DSGE_ST_FILTER_NONFINITE;
    }
  }
}

}  // namespace dsge
