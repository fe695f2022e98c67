// ANTICIPATED SHOCKS per draw: paths of the linearised model  A x_{t-1} + B x_t + C E_t x_{t+1} + D e_t = 0  when agents know shocks
// before they arrive.  With M = B + C T and G = -M^-1 C (A = -M T, R = -M^-1 D):
//     x_t = T x_{t-1} + w_t,   w_t = sum_{j >= 0} G^j R E_t e_{t+j},   x_{-1} = x0,   t = 0 .. n_steps-1
// perfect foresight (the whole path known at t = 0):  w_{n_shock_steps} = 0,  w_t = G w_{t+1} + R e_t, backward in time;
// news (e[t][j] = E_t e_{t+j}, j <= n_lead):          w_t = R e[t][0] + G (R e[t][1] + G (... R e[t][n_lead])), a Horner sum.
//
// ant_setup_kernel, one workgroup of 256 threads per draw: T and C staged in ONE LDS image [n][2n + 1], M = B + C T formed in
// registers (thread (lane c, wave y) owns column c of the rows y, y + 4, ..) and written over T, so the image is [M | C];
// Gauss-Jordan elimination with row pivoting and NO row exchange (the pivot row of column j is remembered, rows are never moved):
// every wavefront finds the pivot of column j itself (one row per lane, six cross-lane steps, the lowest row among equal maxima),
// so a pivot costs ONE barrier.  A pivot with |pivot| <= rank_tol max|M_ij| (or a NaN) -> DSGE_ST_ANTICIPATION_SINGULAR.
// G = -(the right half / the pivots) goes to G_out or to library scratch.
//
// ant_paths_kernel, one workgroup of 256 threads per (draw, 16 paths), the images and row stride of dynamics_propagate_kernel
// (dsge_dynamics.hpp).  Pass 1 holds [G | R] in the matrix image and runs the backward recursion (or, for news, n_lead + 1 Horner
// products per period) with the product step of ps_step on [w ; e] (an_step: the same product on PB tiles of 16 columns); w_t of
// a period inside the horizon is PARKED in the slab of that period (w_out if given, else x_out, else library scratch), periods
// beyond the horizon live in LDS only.  The Horner sums of different periods do not depend on each other: the instantiation
// PB = AN_PB runs four periods side by side in one step, which the launcher picks for grids too small to hide a step's latency
// (launch_anticipated.hip); a column's bits do not depend on PB.  Then T is staged over G and pass 2 runs x_t = T x_{t-1} + w_t
// forward with ps_step: the thread that parked an element reads it back (in flight while the step multiplies), adds it after the
// step's barrier and writes x_t over it.  No atomics: two calls give the same bits.
// Shared pieces (dsge_postsolve.hpp) this file calls: ps_r4, ps_ld, ps_stage_T, ps_stage_TR, ps_step, ps_swap, ps_obs_slice,
// ps_fill_nan.
#pragma once
#include "dsge_postsolve.hpp"

namespace dsge {

constexpr int AN_THREADS = 256, AN_COLS = 16;
constexpr int AN_ST_SINGULAR = 2048;  // DSGE_ST_ANTICIPATION_SINGULAR
constexpr int AN_EPF = 4;             // AN_EPF * AN_THREADS >= AN_COLS * DSGE_MAX_N: one slab (or one step's shocks) in flight
constexpr int AN_RPT = 16;            // rows of M per thread of the setup kernel: 4 waves x AN_RPT >= DSGE_MAX_N
constexpr int AN_PB = 4;              // news on a grid that does not fill the device: this many periods share a Horner step

__host__ __device__ inline int an_setup_ld(int n) { return 2 * n + 1; }
// the setup kernel: [M | C], the four wave maxima, the pivot row of every column
__host__ __device__ inline size_t an_setup_lds_doubles(int n) { return (size_t)n * an_setup_ld(n) + 4 + (n + 1) / 2; }
// the paths kernel: [G | R] (then T), two [w ; e] / x images of pblk x 16 columns, Z, d
__host__ __device__ inline size_t an_paths_lds_doubles(int m, int k, int p, int pblk) {
  return (size_t)(ks_mp(m) + 2 * AN_COLS * pblk) * ps_ld(m, k) + (size_t)p * m + AN_COLS;
}
// ps_step (dsge_postsolve.hpp) on nt tiles of 16 columns: nxt[j][0 .. m4-1] = [T | R] cur[j][0 .. K-1], j < 16 nt.  Every column
// is summed in the order of ps_step, whatever nt: its bits do not depend on the tiles next to it
__device__ __forceinline__ void an_step(const ks_lds* TR, const ks_lds* cur, ks_lds* nxt, int ld, int mt, int nt, int K, int m4) {
  ks_gemm<false, true>(TR, ld, cur, ld, mt, nt, K, 0, 4, [&](int i, int j, double v) {
    if (i < m4) nxt[j * ld + i] = v;
  });
}

struct AntArgs {
  const double* B;      // [batch][m][m]
  const double* C;      // [batch][m][m]
  const double* T;      // [batch][m][m]
  const double* R;      // [batch][m][k]
  const double* eps;    // element (draw, path, row, c) at draw eps_draw + (path rows + row) k + c; row = t (perfect foresight) or
                        // t (n_lead + 1) + j (news); nullptr with n_shock_steps == 0
  const double* x0;     // element (draw, path, i) at draw x0_draw + path x0_path + i, or nullptr (zero)
  const double* Z;      // [batch | 1][p][m] or nullptr (p == 0)
  const double* d;      // [batch | 1][p] or nullptr
  int32_t* status;      // [batch] in/out or nullptr
  double* G;            // [batch][m][m]: G_out or scratch
  int32_t* flag;        // scratch [batch]: non-zero = the draw gets NaN
  double* park;         // [batch][n_paths][n_steps][m]: where w_t waits for pass 2 (w_out, x_out or scratch)
  double* x_out;        // [batch][n_paths][n_steps][m] or nullptr
  double* w_out;        // likewise; park == w_out when it is given
  double* obs_out;      // [batch][n_paths][n_steps][p] or nullptr
  long long eps_draw, x0_draw, x0_path;
  double rank_tol;
  int batch, m, k, p, n_paths, n_steps, n_shock_steps, n_lead, news, z_batched, d_batched, groups, g_is_out;
};

__global__ __launch_bounds__(AN_THREADS) void ant_setup_kernel(AntArgs a) {
  constexpr int NT = AN_THREADS;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int tid = threadIdx.x, draw = blockIdx.x, n = a.m, tx = tid & 63, ty = tid >> 6;
  if (draw >= a.batch) return;
  double* Gg = a.G + (size_t)draw * n * n;
  if (a.status && a.status[draw] != 0) {  // failed solve: the paths kernel writes NaN
    if (tid == 0) a.flag[draw] = 1;
    if (a.g_is_out) ps_fill_nan(Gg, (size_t)n * n, tid, NT);
    return;
  }
  const int ld = an_setup_ld(n);
  ks_lds* A = (ks_lds*)smem;                    // [n][ld]: T, then M, in columns 0 .. n-1, C in columns n .. 2n-1
  ks_lds* red = A + n * ld;                     // [4]
  __attribute__((address_space(3))) int* prow = (__attribute__((address_space(3))) int*)(red + 4);  // [n]
  const double* Bg = a.B + (size_t)draw * n * n;
  const double* Cg = a.C + (size_t)draw * n * n;
  const double* Tg = a.T + (size_t)draw * n * n;
  for (int idx = tid; idx < n * n; idx += NT) {
    const int i = idx / n, c = idx - i * n;
    A[i * ld + c] = Tg[idx];
    A[i * ld + n + c] = Cg[idx];
  }
  __syncthreads();
  // M[i][c] = B[i][c] + sum_k C[i][k] T[k][c], ascending k
  double acc[AN_RPT];
#pragma unroll
  for (int r = 0; r < AN_RPT; ++r) {
    const int i = ty + 4 * r;
    acc[r] = tx < n && i < n ? Bg[i * n + tx] : 0.0;
  }
  if (tx < n)
    for (int kk = 0; kk < n; ++kk) {
      const double t = A[kk * ld + tx];
#pragma unroll
      for (int r = 0; r < AN_RPT; ++r) {
        const int i = ty + 4 * r;
        if (i < n) acc[r] = fma(A[i * ld + n + kk], t, acc[r]);
      }
    }
  __syncthreads();  // (T has been read by everyone)
  double mmax = 0.0;
#pragma unroll
  for (int r = 0; r < AN_RPT; ++r) {
    const int i = ty + 4 * r;
    if (tx < n && i < n) {
      A[i * ld + tx] = acc[r];
      mmax = fmax(mmax, fabs(acc[r]));
    }
  }
  for (int off = 32; off >= 1; off >>= 1) mmax = fmax(mmax, __shfl_xor(mmax, off));
  if (tx == 0) red[ty] = mmax;
  __syncthreads();
  mmax = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  const double thr = (a.rank_tol > 0.0 ? a.rank_tol : 1e-14) * mmax;
  unsigned long long used = 0;  // rows that have been a pivot row (the same in every thread)
  bool singular = false;
  for (int j = 0; j < n; ++j) {
    // the pivot of column j among the rows not used yet: lane l looks at row l
    double v = -1.0;
    if (tx < n && !((used >> tx) & 1ull)) {
      v = fabs(A[tx * ld + j]);
      if (!(v == v)) v = INFINITY;  // a NaN wins, and fails the test below
    }
    int r = tx;
    for (int off = 32; off >= 1; off >>= 1) {
      const double ov = __shfl_xor(v, off);
      const int orr = __shfl_xor(r, off);
      if (ov > v || (ov == v && orr < r)) {
        v = ov;
        r = orr;
      }
    }
    r = __builtin_amdgcn_readfirstlane(r);
    const double piv = r < n ? A[r * ld + j] : 0.0;  // (r < n whenever a row is left, which j < n says)
    if (!(fabs(piv) > thr)) {  // (every wavefront sees the same image: the whole workgroup leaves here)
      singular = true;
      break;
    }
    used |= 1ull << r;
    if (tid == 0) prow[j] = r;
    const double rinv = 1.0 / piv;
    for (int c = j + 1 + tx; c < 2 * n; c += 64) {  // columns <= j are not read again
      const double pjc = A[r * ld + c] * rinv;
      for (int i = ty; i < n; i += 4)
        if (i != r) A[i * ld + c] = fma(-A[i * ld + j], pjc, A[i * ld + c]);
    }
    __syncthreads();
  }
  if (singular) {
    if (tid == 0) {
      a.flag[draw] = 1;
      if (a.status) a.status[draw] |= AN_ST_SINGULAR;
    }
    if (a.g_is_out) ps_fill_nan(Gg, (size_t)n * n, tid, NT);
    return;
  }
  if (tid == 0) a.flag[draw] = 0;
  for (int idx = tid; idx < n * n; idx += NT) {  // row j of the solution sits in the pivot row of column j
    const int j = idx / n, c = idx - j * n, r = prow[j];
    Gg[idx] = -(A[r * ld + n + c] / A[r * ld + j]);
  }
}

// PB: periods per Horner step of the news mode (1 or AN_PB; perfect foresight: 1)
template <int PB>
__global__ __launch_bounds__(AN_THREADS) void ant_paths_kernel(AntArgs a) {
  constexpr int NT = AN_THREADS, NC = AN_COLS;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int tid = threadIdx.x, m = a.m, k = a.k, p = a.p, n_steps = a.n_steps;
  const int draw = blockIdx.x / a.groups, g = blockIdx.x - draw * a.groups;
  if (draw >= a.batch) return;
  const int s0 = g * NC, nc = a.n_paths - s0 < NC ? a.n_paths - s0 : NC;
  const size_t path0 = (size_t)draw * a.n_paths + s0;
  double* xo = a.x_out ? a.x_out + path0 * n_steps * m : nullptr;
  double* wo = a.w_out ? a.w_out + path0 * n_steps * m : nullptr;
  double* oo = a.obs_out ? a.obs_out + path0 * n_steps * p : nullptr;
  double* pk = a.park + path0 * n_steps * m;
  if ((a.status && a.status[draw] != 0) || a.flag[draw] != 0) {  // failed or singular: EVERY output of the draw is NaN
    if (xo) ps_fill_nan(xo, (size_t)nc * n_steps * m, tid, NT);
    if (wo) ps_fill_nan(wo, (size_t)nc * n_steps * m, tid, NT);
    if (oo) ps_fill_nan(oo, (size_t)nc * n_steps * p, tid, NT);
    return;
  }
  const int m4 = ps_r4(m), k4 = ps_r4(k), mp = ks_mp(m), mt = mp / 16, ld = ps_ld(m, k);
  constexpr int NV = NC * PB;  // columns of a vector image
  ks_lds* GR = (ks_lds*)smem;       // [mp][ld]: G (pass 2: T) in columns 0 .. m-1, R in columns m4 .. m4+k-1
  ks_lds* cur = GR + mp * ld;       // [NV][ld]: w (pass 2: x) of path j (period q of a block) in cur[(q NC + j) ld + 0 .. m-1],
  ks_lds* nxt = cur + NV * ld;      //           e in cur[(q NC + j) ld + m4 .. m4+k-1]
  ks_lds* Zm = nxt + NV * ld;       // [p][m]
  ks_lds* dv = Zm + p * m;          // [NC]
  for (size_t idx = tid; idx < an_paths_lds_doubles(m, k, p, PB); idx += NT) GR[idx] = 0.0;
  __syncthreads();
  const double* Tg = a.T + (size_t)draw * m * m;
  ps_stage_TR(GR, ld, m4, a.G + (size_t)draw * m * m, a.R + (size_t)draw * m * k, m, k, tid, NT);
  if (p > 0) {
    const double* Zg = ps_obs_slice(a.Z, a.z_batched, draw, p * m);
    for (int idx = tid; idx < p * m; idx += NT) Zm[idx] = Zg[idx];
    if (tid < p) dv[tid] = a.d ? ps_obs_slice(a.d, a.d_batched, draw, p)[tid] : 0.0;
  }
  // ---- pass 1: the anticipation term.  Perfect foresight: step s multiplies the shocks of period nsh-1-s.  News: the periods come
  // in blocks of PB, whose Horner sums do not depend on each other and run side by side as PB tiles of one product; step s
  // multiplies lead n_lead - s % L1 of the block s / L1.  A fresh step starts a sum (w = R e) ----
  const int L1 = a.n_lead + 1, nsh = a.n_shock_steps;
  const int S = a.news ? (nsh + PB - 1) / PB * L1 : nsh;
  const size_t per_path = (size_t)nsh * L1 * k;
  const double* eg = nsh > 0 ? a.eps + (size_t)draw * a.eps_draw + (size_t)s0 * per_path : nullptr;
  auto period0 = [&](int s) -> int { return a.news ? s / L1 * PB : nsh - 1 - s; };  // the first period of step s
  auto lead_of = [&](int s) -> int { return a.news ? a.n_lead - s % L1 : 0; };
  // entry idx = j k + c of the shocks of period t0 + q at lead l (zero beyond the last shock period)
  auto shock = [&](int idx, int t0, int q, int l) -> double {
    return t0 + q < nsh ? eg[(size_t)(idx / k) * per_path + ((size_t)(t0 + q) * L1 + l) * k + idx % k] : 0.0;
  };
  if (S > 0)
    for (int q = 0; q < PB; ++q)
      for (int idx = tid; idx < nc * k; idx += NT) cur[(q * NC + idx / k) * ld + m4 + idx % k] = shock(idx, period0(0), q, lead_of(0));
  __syncthreads();
  for (int s = 0; s < S; ++s) {
    const int t0 = period0(s), l = lead_of(s);
    const bool fresh = a.news ? l == a.n_lead : s == 0;
    const bool done = l == 0;  // w of the step's periods is complete after this step
    const bool more = s + 1 < S;
    double ev[PB][AN_EPF] = {};  // the next shocks, in flight while this step multiplies
    if (more) {
      const int nt0 = period0(s + 1), nl = lead_of(s + 1);
#pragma unroll
      for (int q = 0; q < PB; ++q)
#pragma unroll
        for (int e = 0; e < AN_EPF; ++e) {
          const int idx = tid + e * NT;
          if (idx < nc * k) ev[q][e] = shock(idx, nt0, q, nl);
        }
    }
    if (fresh)
      an_step((const ks_lds*)GR + m4, (const ks_lds*)cur + m4, nxt, ld, mt, PB, k4, m4);
    else
      an_step((const ks_lds*)GR, (const ks_lds*)cur, nxt, ld, mt, PB, m4 + k4, m4);
    if (more) {
#pragma unroll
      for (int q = 0; q < PB; ++q)
#pragma unroll
        for (int e = 0; e < AN_EPF; ++e) {
          const int idx = tid + e * NT;
          if (idx < nc * k) nxt[(q * NC + idx / k) * ld + m4 + idx % k] = ev[q][e];
        }
    }
    __syncthreads();
    if (done) {  // park w_t in the slab of its period
      for (int q = 0; q < PB; ++q) {
        const int t = t0 + q;
        if (t >= nsh || t >= n_steps) break;
#pragma unroll
        for (int e = 0; e < AN_EPF; ++e) {
          const int idx = tid + e * NT;
          if (idx < nc * m) {
            const int j = idx / m, i = idx - j * m;
            pk[((size_t)j * n_steps + t) * m + i] = nxt[(q * NC + j) * ld + i];
          }
        }
      }
    }
    ps_swap(cur, nxt);
  }
  __syncthreads();  // (G has been read by everyone)
  // ---- pass 2: x_t = T x_{t-1} + w_t, every slab of x written once over the parked w_t ----
  ps_stage_T(GR, ld, Tg, m, tid, NT);
  for (int idx = tid; idx < NC * ld; idx += NT) cur[idx] = 0.0;
  __syncthreads();
  if (a.x0) {
    const double* xg = a.x0 + (size_t)draw * a.x0_draw + (size_t)s0 * a.x0_path;
    for (int idx = tid; idx < nc * m; idx += NT) {
      const int j = idx / m, i = idx - j * m;
      cur[j * ld + i] = xg[(size_t)j * a.x0_path + i];
    }
  }
  __syncthreads();
  const int n_w = nsh < n_steps ? nsh : n_steps;  // periods with a parked w_t; later ones have w = 0
  for (int t = 0; t < n_steps; ++t) {
    const bool has_w = t < n_w;
    double wv[AN_EPF] = {};
    if (has_w) {
#pragma unroll
      for (int q = 0; q < AN_EPF; ++q) {
        const int idx = tid + q * NT;
        if (idx < nc * m) {
          const int j = idx / m, i = idx - j * m;
          wv[q] = pk[((size_t)j * n_steps + t) * m + i];  // (written by this thread in pass 1)
        }
      }
    }
    ps_step((const ks_lds*)GR, (const ks_lds*)cur, nxt, ld, mt, m4, m4);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < AN_EPF; ++q) {
      const int idx = tid + q * NT;
      if (idx < nc * m) {
        const int j = idx / m, i = idx - j * m;
        const size_t at = ((size_t)j * n_steps + t) * m + i;
        const double v = nxt[j * ld + i] + wv[q];
        nxt[j * ld + i] = v;
        if (xo) xo[at] = v;
        if (wo && !has_w) wo[at] = 0.0;
      }
    }
    __syncthreads();
    if (oo)
      for (int idx = tid; idx < nc * p; idx += NT) {
        const int j = idx / p, o = idx - j * p;
        double sum = 0.0;
        for (int i = 0; i < m; ++i) sum = fma(Zm[o * m + i], nxt[j * ld + i], sum);
        oo[((size_t)j * n_steps + t) * p + o] = dv[o] + sum;
      }
    ps_swap(cur, nxt);
  }
}

}  // namespace dsge
