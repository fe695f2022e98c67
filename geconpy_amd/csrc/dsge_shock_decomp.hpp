// HISTORICAL SHOCK DECOMPOSITION per draw: the smoothed path x_t of the smoother (dsge_kalman_smooth.hpp) or of a draw of the
// simulation smoother (dsge_simsmooth.hpp), split into what each group of structural shocks, the initial condition and the
// filter conventions (the remainder) contribute:
//     X_0 = [0 .. 0 | x_0],   X_t = T X_{t-1} + R E_t,   E_t[j, c] = e_t[j] if group[j] == c else 0,   rem_t = x_t - sum_c X_t[:, c]
// A sibling of dynamics_propagate_kernel (dsge_dynamics.hpp): one workgroup of 256 threads per (draw, pack of paths).  The
// G = n_groups + 1 component columns of a path are columns of ONE 16-column matrix-core tile, and floor(16 / G) paths share
// it (column q G + c is component c of the pack's path q).  [T | R] of the draw sits in one zero-padded LDS image (R from column
// m4 on), the running [X ; E] in a second one, path-major (Xt[column][row]) and double-buffered, both with the row stride == 2
// (mod 32) of the fragment loads, so that a step is ONE product [T | R] [X_{t-1} ; E_t] of ks_gemm with K = m4 + k4.  E is
// never expanded in memory: its k possibly non-zero entries per path sit at the fixed places (q G + group[j], m4 + j) of an
// image zeroed once, and a step stores exactly the k doubles of e_t there.  e_0 (NaN by the smoother's definition) is not read.
// e_{t+1} and x_{t+1} are in flight while step t multiplies.  After the step's only barrier every thread reads finished columns:
// the n_out x C block of a path and step is written contiguously, the place of each of its elements looked up in a table built
// once (no division in the step loop), the remainder formed by the thread that writes it, in ascending component order.
// Shared pieces (dsge_postsolve.hpp) this file calls, and the lines it keeps: docs/design/dynamics.md, "the shared pieces".
#pragma once
#include "dsge_postsolve.hpp"

namespace dsge {

constexpr int SD_THREADS = 256, SD_COLS = 16, SD_MAX_PACK = 8;  // (G >= 2: at most 8 paths in a tile)
constexpr int SD_PF = 3;  // SD_PF * SD_THREADS >= SD_MAX_PACK * DSGE_MAX_N_BIG: x (and e, k <= m) of one step in flight

__host__ __device__ inline size_t sd_lds_doubles(int m, int k, int p, int pack) {
  // [T | R], two [X ; E] images, two copies of x_t of the pack, Z, the table of the largest output block (int32, two per double)
  return (size_t)(ks_mp(m) + 2 * SD_COLS) * ps_ld(m, k) + 2 * (size_t)pack * m + (size_t)p * m + ((size_t)m * (SD_COLS / pack + 1) + 1) / 2;
}

struct ShockDecompArgs {
  const double* T;        // [batch][m][m]
  const double* R;        // [batch][m][k]
  const double* eps;      // [batch][n_paths][T_len][k]
  const double* x;        // [batch][n_paths][T_len][m]
  const double* Z;        // [batch | 1][p][m] or nullptr
  const int32_t* status;  // [batch] or nullptr
  double* contrib;        // [batch][n_paths][T_len][n_out][C] or nullptr
  double* obs;            // [batch][n_paths][T_len][p][C] or nullptr
  long long* dbg;         // debug (dsge_debug_shock_decomp_phases): int64[8], shader-clock cycles of wavefront 0 of workgroup 0
  int batch, m, k, p, n_paths, T_len, n_out, g, remainder, z_batched, pack, units;
  unsigned char grp[DSGE_MAX_N_BIG];  // group of shock j
  unsigned char var[DSGE_MAX_N_BIG];  // variable of output row i
};

__global__ __launch_bounds__(SD_THREADS) void shock_decomp_kernel(ShockDecompArgs a) {
  constexpr int NT = SD_THREADS, NC = SD_COLS;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int tid = threadIdx.x, m = a.m, k = a.k, p = a.obs ? a.p : 0, T_len = a.T_len;
  const int draw = blockIdx.x / a.units, u = blockIdx.x - draw * a.units;
  if (draw >= a.batch) return;
  const int G = a.g + 1, C = G + (a.remainder ? 1 : 0), n_out = a.contrib ? a.n_out : 0;
  const int s0 = u * a.pack, np = a.n_paths - s0 < a.pack ? a.n_paths - s0 : a.pack;  // paths s0 .. s0 + np - 1
  const size_t path0 = (size_t)draw * a.n_paths + s0;
  const int cblk = n_out * C, oblk = p * C;  // doubles of one path and step
  double* co = a.contrib ? a.contrib + path0 * T_len * cblk : nullptr;
  double* oo = a.obs ? a.obs + path0 * T_len * oblk : nullptr;
  if (a.status && a.status[draw] != 0) {  // failed solve: EVERY output of the draw is NaN
    if (co) for (size_t i = tid; i < (size_t)np * T_len * cblk; i += NT) co[i] = NAN;
    if (oo) for (size_t i = tid; i < (size_t)np * T_len * oblk; i += NT) oo[i] = NAN;
    return;
  }
  const bool prof = a.dbg != nullptr && blockIdx.x == 0 && tid < 64;
  long long pc[4] = {0, 0, 0, 0}, p_begin = prof ? clock64() : 0;
  const int m4 = ps_r4(m), k4 = ps_r4(k), mp = ks_mp(m), mt = mp / 16, ld = ps_ld(m, k);
  ks_lds* TR = (ks_lds*)smem;            // [mp][ld]: T in columns 0 .. m-1, R in columns m4 .. m4+k-1
  ks_lds* cur = TR + mp * ld;            // [NC][ld]: column q G + c of X_{t-1} in cur[(q G + c) ld + 0 .. m-1], of E_t behind m4
  ks_lds* nxt = cur + NC * ld;
  ks_lds* xs = nxt + NC * ld;            // [2][pack m]: x_t of the pack, by the parity of t
  ks_lds* Zm = xs + 2 * a.pack * m;      // [p][m]
  __attribute__((address_space(3))) int* tab = (__attribute__((address_space(3))) int*)(Zm + p * m);
  // tab[io C + c]: where element (row io, component c) of the output block lives in a path's columns, c ld + var[io]; the
  // remainder of variable i: -1 - i
  for (size_t idx = tid; idx < (size_t)(mp + 2 * NC) * ld; idx += NT) TR[idx] = 0.0;
  __syncthreads();
  const double* Tg = a.T + (size_t)draw * m * m;
  const double* Rg = a.R + (size_t)draw * m * k;
  for (int idx = tid; idx < m * m; idx += NT) {
    const int i = idx / m, j = idx - i * m;
    TR[i * ld + j] = Tg[idx];
  }
  for (int idx = tid; idx < m * k; idx += NT) {
    const int i = idx / k, c = idx - i * k;
    TR[i * ld + m4 + c] = Rg[idx];
  }
  if (p > 0) {
    const double* Zg = a.Z + (a.z_batched ? (size_t)draw * p * m : 0);
    for (int idx = tid; idx < p * m; idx += NT) Zm[idx] = Zg[idx];
  }
  for (int idx = tid; idx < cblk; idx += NT) {
    const int io = idx / C, c = idx - io * C;
    tab[idx] = c < G ? c * ld + a.var[io] : -1 - a.var[io];
  }
  // what this thread moves at every step: entries idx = tid + q NT of the pack's e_t (idx = path k + j) and x_t (idx = path m + i;
  // read for the remainder alone)
  const double* eg = a.eps + path0 * T_len * k;
  const double* xg = a.x + path0 * T_len * m;
  int esrc[SD_PF], edst[SD_PF], xsrc[SD_PF];
#pragma unroll
  for (int q = 0; q < SD_PF; ++q) {
    const int idx = tid + q * NT;
    esrc[q] = edst[q] = xsrc[q] = -1;
    if (idx < np * k) {
      const int pq = idx / k, j = idx - pq * k;
      esrc[q] = pq * T_len * k + j;
      edst[q] = (pq * G + a.grp[j]) * ld + m4 + j;
    }
    if (idx < np * m) {
      const int pq = idx / m, i = idx - pq * m;
      cur[(pq * G + a.g) * ld + i] = xs[idx] = xg[pq * T_len * m + i];  // X_0: the initial condition alone
      if (a.remainder) xsrc[q] = pq * T_len * m + i;
    }
  }
  double xc[SD_PF] = {};  // x_t of the step being multiplied
  if (T_len > 1) {
#pragma unroll
    for (int q = 0; q < SD_PF; ++q) {
      if (esrc[q] >= 0) cur[edst[q]] = eg[esrc[q] + k];
      if (xsrc[q] >= 0) xc[q] = xg[xsrc[q] + m];
    }
  }
  __syncthreads();
  // the outputs of step t from the finished columns X and x_t (xt)
  auto emit = [&](const ks_lds* X, const ks_lds* xt, int t) {
    auto rem = [&](int pq, int i) -> double {  // ascending component order
      double s = 0.0;
      for (int c = 0; c < G; ++c) s += X[(pq * G + c) * ld + i];
      return xt[pq * m + i] - s;
    };
    for (int pq = 0; pq < np; ++pq) {
      const ks_lds* Xp = X + pq * G * ld;
      if (co) {
        double* dst = co + ((size_t)pq * T_len + t) * cblk;
        for (int idx = tid; idx < cblk; idx += NT) {
          const int o = tab[idx];
          dst[idx] = o >= 0 ? Xp[o] : rem(pq, -1 - o);
        }
      }
      if (oo) {
        double* dst = oo + ((size_t)pq * T_len + t) * oblk;
        for (int idx = tid; idx < oblk; idx += NT) {
          const int o = idx / C, c = idx - o * C;
          double s = 0.0;
          if (c < G) {
            for (int i = 0; i < m; ++i) s = fma(Zm[o * m + i], Xp[c * ld + i], s);
          } else {
            for (int i = 0; i < m; ++i) s = fma(Zm[o * m + i], rem(pq, i), s);
          }
          dst[idx] = s;
        }
      }
    }
  };
  emit((const ks_lds*)cur, (const ks_lds*)xs, 0);
  const long long p_setup = prof ? clock64() - p_begin : 0;
  for (int t = 1; t < T_len; ++t) {
    const long long p0 = prof ? clock64() : 0;
    const bool more = t + 1 < T_len;
    double ev[SD_PF] = {}, xv[SD_PF] = {};  // e_{t+1}, x_{t+1}, in flight while this step multiplies
    if (more) {
#pragma unroll
      for (int q = 0; q < SD_PF; ++q) {
        if (esrc[q] >= 0) ev[q] = eg[esrc[q] + (t + 1) * k];
        if (xsrc[q] >= 0) xv[q] = xg[xsrc[q] + (t + 1) * m];
      }
    }
    ks_gemm<false, true>((const ks_lds*)TR, ld, (const ks_lds*)cur, ld, mt, 1, m4 + k4, 0, 4, [&](int i, int j, double v) {
      if (i < m4) nxt[j * ld + i] = v;
    });
    const long long p1 = prof ? clock64() : 0;
    ks_lds* xt = xs + (t & 1) * a.pack * m;
#pragma unroll
    for (int q = 0; q < SD_PF; ++q) {
      if (more && esrc[q] >= 0) nxt[edst[q]] = ev[q];
      if (xsrc[q] >= 0) xt[tid + q * NT] = xc[q];
      xc[q] = xv[q];
    }
    const long long p2 = prof ? clock64() : 0;
    __syncthreads();
    const long long p3 = prof ? clock64() : 0;
    emit((const ks_lds*)nxt, (const ks_lds*)xt, t);
    if (prof) {
      pc[0] += p1 - p0; pc[1] += p2 - p1; pc[2] += p3 - p2; pc[3] += clock64() - p3;
    }
    ks_lds* sw = cur;
    cur = nxt;
    nxt = sw;
  }
  if (prof && tid == 0) {
    for (int i = 0; i < 4; ++i) a.dbg[i] = pc[i];
    a.dbg[4] = clock64() - p_begin;
    a.dbg[5] = T_len - 1;
    a.dbg[6] = p_setup;
  }
}

}  // namespace dsge
