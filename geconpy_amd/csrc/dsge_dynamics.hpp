// Post-solve DYNAMICS per draw: what a user of the reference runs on every retained draw after the solve --
//   impulse responses   gEconpy/model/simulate.py::impulse_response_function
//   simulated paths     gEconpy/model/simulate.py::simulate              (both through _simulate_linear_system)
//   forecasts           the `forecast` of the pymc_extras state-space model that DSGEStateSpace extends
// -- all the recursion x_t = T x_{t-1} + R e_t, which the reference evaluates in a Python loop, one draw and one shock at a time.
//
// dynamics_propagate_kernel (simulate, impulse responses, FEVD): one workgroup of 256 threads per (draw, group of 16 paths), so a
// single draw with many paths still fills the device.  [T | R] of the draw sits in ONE zero-padded LDS image (R from column
// m4 = 4 ceil(m / 4) on), the running [x ; e_t] of the 16 paths in a second one, stored path-major ("transposed": Xt[path][row])
// and double-buffered, so that a step is ONE product  [T | R] [x_{t-1} ; e_t]  of ks_gemm (dsge_mfma_f64.hpp) with K = m4 + k4
// while shocks remain and K = m4 after the last one.  Both images have the row stride == 2 (mod 32) of the fragment loads.  The
// result goes back into the other X image; after the step's only barrier the m x 16 slab is written once from LDS, contiguous
// along the variable index.  The job is bound by those writes (2 m^2 flops against 8 m bytes per path and step).
// FEVD of the impulses (c <= 16: one group holds them all): the running sums w_j sum_s irf^2 stay in LDS, the shares of a step are
// written behind its slab; c > 16: dynamics_fevd_kernel makes a second pass over the stored responses.
//
// dynamics_forecast_kernel: one workgroup per draw, T, P and one working image in LDS for all steps (three ks_mat images: 101 KB
// at m = 49..64), sym(R Q R') formed once per draw and kept in registers by the threads that own its elements; per step
//     a = T a;   W = P T';   P = T W;   P = sym(P) + sym(R Q R')      (the prediction step of dsge_kalman_out.hpp)
// with the two square products on the FP64 matrix core, then y = Z a + d, F = sym(Z P Z') + diag(H) on the VALU (p <= 16).
// Shared pieces (dsge_postsolve.hpp) this file calls, and the lines it keeps: docs/design/dynamics.md, "the shared pieces".
#pragma once
#include "dsge_postsolve.hpp"

namespace dsge {

constexpr int DY_THREADS = 256, DY_COLS = 16;
constexpr int DY_EPF = 6;  // DY_EPF * DY_THREADS >= DY_COLS * DSGE_MAX_N_BIG: the shocks of one step in flight

__host__ __device__ inline int dy_ldc(int m) { return m | 1; }  // row stride of the FEVD sums (odd: read along either index)
__host__ __device__ inline size_t dy_lds_doubles(int m, int k) {
  return (size_t)(ks_mp(m) + 2 * DY_COLS) * ps_ld(m, k) + (size_t)DY_COLS * dy_ldc(m) + m + DY_COLS;
}
__host__ __device__ inline size_t dy_fevd_lds_doubles(int m, int c) { return (size_t)c * dy_ldc(m) + m + c; }

struct DynArgs {
  const double* T;        // [batch][m][m]
  const double* R;        // [batch][m][k]
  const double* shocks;   // element (draw, path, step, component) at draw sh_draw + path sh_path + step sh_step + comp sh_comp
  long long sh_draw, sh_path, sh_step, sh_comp;
  int identity;           // shocks == nullptr: e_0 of path j is the unit vector j (n_paths == k), no identity is read
  const double* x0;       // [batch | 1][n_paths][m] or nullptr (zero)
  long long x0_draw;      // n_paths * m or 0
  const double* weights;  // [batch | 1][n_paths] or nullptr (ones): FEVD only
  long long w_draw;
  const int32_t* status;  // [batch] or nullptr
  double* x_out;          // [batch][n_paths][n_steps][m] or nullptr
  double* fevd;           // [batch][n_steps][m][n_paths] or nullptr; n_paths <= DY_COLS
  int batch, m, k, n_paths, n_steps, n_shock_steps, groups;
};

// The shares of one step from the weighted running sums cum[j ldc + i] (j < nc impulses, i < m variables): out[i nc + j] =
// cum_ji / sum_j' cum_j'i, NaN in the whole row of a variable nothing has moved yet (0 / 0).  Called by every thread of the
// workgroup, with the sums of the step complete in every thread's view only after the first barrier here.
__device__ __forceinline__ void dy_fevd_emit(const ks_lds* cum, ks_lds* den, int ldc, int m, int nc, double* out) {
  __syncthreads();
  for (int i = threadIdx.x; i < m; i += DY_THREADS) {
    double s = 0.0;
    for (int j = 0; j < nc; ++j) s += cum[j * ldc + i];
    den[i] = s;
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < m * nc; idx += DY_THREADS) {
    const int i = idx / nc, j = idx - i * nc;
    out[idx] = cum[j * ldc + i] / den[i];
  }
}

__global__ __launch_bounds__(DY_THREADS) void dynamics_propagate_kernel(DynArgs a) {
  constexpr int NT = DY_THREADS, NC = DY_COLS;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int tid = threadIdx.x, m = a.m, k = a.k;
  const int draw = blockIdx.x / a.groups, g = blockIdx.x - draw * a.groups;
  if (draw >= a.batch) return;
  const int s0 = g * NC, nc = a.n_paths - s0 < NC ? a.n_paths - s0 : NC;
  const size_t path_sz = (size_t)a.n_steps * m;
  double* xo = a.x_out ? a.x_out + ((size_t)draw * a.n_paths + s0) * path_sz : nullptr;
  double* fo = a.fevd ? a.fevd + (size_t)draw * path_sz * a.n_paths : nullptr;
  if (a.status && a.status[draw] != 0) {  // failed solve: EVERY output of the draw is NaN
    if (xo) for (size_t i = tid; i < (size_t)nc * path_sz; i += NT) xo[i] = NAN;
    if (fo) for (size_t i = tid; i < path_sz * a.n_paths; i += NT) fo[i] = NAN;
    return;
  }
  const int m4 = ps_r4(m), k4 = ps_r4(k), mp = ks_mp(m), mt = mp / 16, ld = ps_ld(m, k), ldc = dy_ldc(m);
  ks_lds* TR = (ks_lds*)smem;      // [mp][ld]: T in columns 0 .. m-1, R in columns m4 .. m4+k-1
  ks_lds* cur = TR + mp * ld;      // [NC][ld]: x_{t-1} of path j in cur[j ld + 0 .. m-1], e_t in cur[j ld + m4 .. m4+k-1]
  ks_lds* nxt = cur + NC * ld;
  ks_lds* cum = nxt + NC * ld;     // [NC][ldc]
  ks_lds* den = cum + NC * ldc;    // [m]
  ks_lds* wv = den + m;            // [NC]
  for (size_t idx = tid; idx < dy_lds_doubles(m, k); idx += NT) TR[idx] = 0.0;
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
  if (a.x0) {
    const double* xg = a.x0 + (size_t)draw * a.x0_draw + (size_t)s0 * m;
    for (int idx = tid; idx < nc * m; idx += NT) {
      const int j = idx / m, i = idx - j * m;
      cur[j * ld + i] = xg[idx];
    }
  }
  if (tid < nc) wv[tid] = a.weights ? a.weights[(size_t)draw * a.w_draw + s0 + tid] : 1.0;
  const double* sg = a.shocks ? a.shocks + (size_t)draw * a.sh_draw + (size_t)s0 * a.sh_path : nullptr;
  auto shock = [&](int idx, int t) -> double {  // entry idx = j k + c of e_t
    const int j = idx / k, c = idx - j * k;
    if (a.identity) return c == s0 + j ? 1.0 : 0.0;
    return sg[(size_t)j * a.sh_path + (size_t)t * a.sh_step + (size_t)c * a.sh_comp];
  };
  if (a.n_shock_steps > 0)
    for (int idx = tid; idx < nc * k; idx += NT) cur[(idx / k) * ld + m4 + idx % k] = shock(idx, 0);
  __syncthreads();
  for (int t = 0; t < a.n_steps; ++t) {
    const bool more = t + 1 < a.n_shock_steps;
    double ev[DY_EPF] = {};  // e_{t+1}, in flight while this step multiplies
    if (more) {
#pragma unroll
      for (int q = 0; q < DY_EPF; ++q) {
        const int idx = tid + q * NT;
        if (idx < nc * k) ev[q] = shock(idx, t + 1);
      }
    }
    ks_gemm<false, true>((const ks_lds*)TR, ld, (const ks_lds*)cur, ld, mt, 1, t < a.n_shock_steps ? m4 + k4 : m4, 0, 4,
                         [&](int i, int j, double v) {
                           if (i < m4) nxt[j * ld + i] = v;
                         });
    if (more) {
#pragma unroll
      for (int q = 0; q < DY_EPF; ++q) {
        const int idx = tid + q * NT;
        if (idx < nc * k) nxt[(idx / k) * ld + m4 + idx % k] = ev[q];
      }
    }
    __syncthreads();
    for (int idx = tid; idx < nc * m; idx += NT) {  // the slab of this step: m contiguous doubles per path
      const int j = idx / m, i = idx - j * m;
      const double v = nxt[j * ld + i];
      if (xo) xo[(size_t)j * path_sz + (size_t)t * m + i] = v;
      if (fo) cum[j * ldc + i] = fma(wv[j] * v, v, cum[j * ldc + i]);  // (the same thread owns (j, i) at every step)
    }
    if (fo) dy_fevd_emit(cum, den, ldc, m, nc, fo + (size_t)t * m * nc);
    ks_lds* sw = cur;
    cur = nxt;
    nxt = sw;
  }
}

// FEVD of more than 16 impulses: a second pass over the stored responses, one workgroup per draw.
struct FevdArgs {
  const double* irf;      // [batch][c][n_steps][m]
  const double* weights;  // [batch | 1][c] or nullptr
  long long w_draw;
  const int32_t* status;
  double* fevd;           // [batch][n_steps][m][c]
  int batch, m, c, n_steps;
};

__global__ __launch_bounds__(DY_THREADS) void dynamics_fevd_kernel(FevdArgs a) {
  constexpr int NT = DY_THREADS;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int tid = threadIdx.x, draw = blockIdx.x, m = a.m, c = a.c, ldc = dy_ldc(m);
  if (draw >= a.batch) return;
  const size_t path_sz = (size_t)a.n_steps * m;
  double* fo = a.fevd + (size_t)draw * path_sz * c;
  if (a.status && a.status[draw] != 0) {
    ps_fill_nan(fo, path_sz * c, tid, NT);
    return;
  }
  ks_lds* cum = (ks_lds*)smem;  // [c][ldc]
  ks_lds* den = cum + (size_t)c * ldc;
  ks_lds* wv = den + m;
  for (int idx = tid; idx < c * ldc; idx += NT) cum[idx] = 0.0;
  for (int j = tid; j < c; j += NT) wv[j] = a.weights ? a.weights[(size_t)draw * a.w_draw + j] : 1.0;
  __syncthreads();
  const double* xg = a.irf + (size_t)draw * c * path_sz;
  for (int t = 0; t < a.n_steps; ++t) {
    for (int idx = tid; idx < c * m; idx += NT) {
      const int j = idx / m, i = idx - j * m;
      const double v = xg[(size_t)j * path_sz + (size_t)t * m + i];
      cum[j * ldc + i] = fma(wv[j] * v, v, cum[j * ldc + i]);
    }
    dy_fevd_emit(cum, den, ldc, m, c, fo + (size_t)t * m * c);
    __syncthreads();  // (the next step's sums wait for this step's readers)
  }
}

// ---- forecast moments ----------------------------------------------------------------------------------------------------------
constexpr int FC_THREADS = 256, FC_PF = 16, FC_PMAX = 16;  // FC_PF * FC_THREADS >= 64 * 64

struct FcArgs {
  const double* T;       // [batch][m][m]
  const double* R;       // [batch][m][k]
  const double* Q;       // layout q_mode
  const double* Z;       // [p][m] or [batch][p][m]; nullptr with p == 0
  const double* d;       // nullptr, [p] or [batch][p]
  const double* Hdiag;   // nullptr, [p] or [batch][p]
  const double* a0;      // [batch][m]
  const double* P0;      // [batch][m][m] or nullptr (zero)
  const int32_t* status; // [batch] or nullptr
  double* a_out;         // [batch][n_steps][m] or nullptr
  double* p_out;         // [batch][n_steps][m] (diagonals) or [batch][n_steps][m][m] (full_cov) or nullptr
  double* y_out;         // [batch][n_steps][p] or nullptr
  double* f_out;         // [batch][n_steps][p][p] or nullptr
  int batch, m, k, p, n_steps, q_mode, z_batched, d_batched, h_batched, full_cov;
};

__host__ __device__ inline size_t fc_lds_doubles(int m, int p) {
  return 3 * ks_mat(m) + (size_t)p * m + (size_t)m * FC_PMAX + FC_PMAX * FC_PMAX + 2 * 64 + 2 * FC_PMAX;
}

__global__ __launch_bounds__(FC_THREADS) void dynamics_forecast_kernel(FcArgs a) {
  constexpr int NT = FC_THREADS, PM = FC_PMAX;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int tid = threadIdx.x, draw = blockIdx.x, m = a.m, k = a.k, p = a.p, mm = m * m, n = a.n_steps;
  if (draw >= a.batch) return;
  const size_t nv = (size_t)n * m, ncv = a.full_cov ? nv * m : nv;
  double* a_o = a.a_out ? a.a_out + (size_t)draw * nv : nullptr;
  double* p_o = a.p_out ? a.p_out + (size_t)draw * ncv : nullptr;
  double* y_o = a.y_out ? a.y_out + (size_t)draw * n * p : nullptr;
  double* f_o = a.f_out ? a.f_out + (size_t)draw * n * p * p : nullptr;
  if (a.status && a.status[draw] != 0) {  // failed solve: EVERY requested output of the draw is NaN
    if (a_o) ps_fill_nan(a_o, nv, tid, NT);
    if (p_o) ps_fill_nan(p_o, ncv, tid, NT);
    if (y_o) ps_fill_nan(y_o, (size_t)n * p, tid, NT);
    if (f_o) ps_fill_nan(f_o, (size_t)n * p * p, tid, NT);
    return;
  }
  const bool cov = p_o || f_o;
  const int ld = ks_ld(m), mt = ks_mp(m) / 16, m4 = ps_r4(m);
  const size_t MAT = ks_mat(m);
  ks_lds* Tm = (ks_lds*)smem;
  ks_lds* P = Tm + MAT;
  ks_lds* W = P + MAT;
  ks_lds* Zm = W + MAT;            // [p][m]
  ks_lds* PZ = Zm + (size_t)p * m; // [m][PM]
  ks_lds* Fm = PZ + (size_t)m * PM;
  ks_lds* ac = Fm + PM * PM;       // a_{h-1}
  ks_lds* an = ac + 64;            // a_h
  ks_lds* dv = an + 64;
  ks_lds* hv = dv + PM;
  const double* Rg = a.R + (size_t)draw * m * k;
  for (size_t idx = tid; idx < 3 * MAT; idx += NT) Tm[idx] = 0.0;  // (the padding of the three images stays zero)
  __syncthreads();
  ps_stage_T(Tm, ld, a.T + (size_t)draw * mm, m, tid, NT);
  if (p > 0) {
    const double* Zg = ps_obs_slice(a.Z, a.z_batched, draw, p * m);
    for (int idx = tid; idx < p * m; idx += NT) Zm[idx] = Zg[idx];
    if (tid < p) {
      dv[tid] = a.d ? ps_obs_slice(a.d, a.d_batched, draw, p)[tid] : 0.0;
      hv[tid] = a.Hdiag ? ps_obs_slice(a.Hdiag, a.h_batched, draw, p)[tid] : 0.0;
    }
  }
  if (tid < m) ac[tid] = a.a0[(size_t)draw * m + tid];
  // G = sym(R Q R'), once per draw: R -> P, R Q -> W, then element idx = tid + q NT of G (upper triangle) in g[q]
  double g[FC_PF] = {};
  if (cov) {
    bool qf;
    const double* Qg = ps_q_slice(a.Q, a.q_mode, draw, k, &qf);
    for (int idx = tid; idx < m * k; idx += NT) {
      const int i = idx / k, c = idx - i * k;
      P[i * ld + c] = Rg[idx];
    }
    __syncthreads();
    for (int idx = tid; idx < m * k; idx += NT) {
      const int i = idx / k, c = idx - i * k;
      double s;
      if (qf) {
        s = 0.0;
        for (int e = 0; e < k; ++e) s = fma(P[i * ld + e], Qg[e * k + c], s);
      } else {
        s = P[i * ld + c] * Qg[c];
      }
      W[i * ld + c] = s;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < FC_PF; ++q) {
      const int idx = tid + q * NT;
      if (idx < mm) {
        const int i = idx / m, j = idx - i * m;
        if (i <= j) {
          double s = 0.0;
          for (int c = 0; c < k; ++c) s = fma(W[i * ld + c], P[j * ld + c], fma(W[j * ld + c], P[i * ld + c], s));
          g[q] = 0.5 * s;
        }
      }
    }
    __syncthreads();
    for (size_t idx = tid; idx < 2 * MAT; idx += NT) P[idx] = 0.0;
    __syncthreads();
    if (a.P0)
      for (int idx = tid; idx < mm; idx += NT) {
        const int i = idx / m, j = idx - i * m;
        P[i * ld + j] = a.P0[(size_t)draw * mm + idx];
      }
  }
  __syncthreads();
  for (int h = 0; h < n; ++h) {
    const size_t oh = (size_t)h * m;
    // (1) a_h = T a_{h-1};  W = P T'
    if (tid < m) {
      double s = 0.0;
#pragma unroll 4
      for (int j = 0; j < m; ++j) s = fma(Tm[tid * ld + j], ac[j], s);
      an[tid] = s;
      if (a_o) a_o[oh + tid] = s;
    }
    if (cov)
      ks_gemm<false, true>((const ks_lds*)P, ld, (const ks_lds*)Tm, ld, mt, mt, m4, 0, 4,
                           [&](int i, int j, double v) { W[i * ld + j] = v; });
    __syncthreads();
    // (2) P = T W;  y_h = Z a_h + d
    if (cov)
      ks_gemm<false, false>((const ks_lds*)Tm, ld, (const ks_lds*)W, ld, mt, mt, m4, 0, 4,
                            [&](int i, int j, double v) { P[i * ld + j] = v; });
    if (y_o && tid < p) {
      double s = dv[tid];
      for (int j = 0; j < m; ++j) s = fma(Zm[tid * m + j], an[j], s);
      y_o[(size_t)h * p + tid] = s;
    }
    __syncthreads();
    // (3) P_h = sym(P) + sym(R Q R'): the owner of (i, j), i <= j, writes both halves
    if (cov) {
#pragma unroll
      for (int q = 0; q < FC_PF; ++q) {
        const int idx = tid + q * NT;
        if (idx < mm) {
          const int i = idx / m, j = idx - i * m;
          if (i <= j) {
            const double v = 0.5 * (P[i * ld + j] + P[j * ld + i]) + g[q];
            P[i * ld + j] = v;
            P[j * ld + i] = v;
          }
        }
      }
      __syncthreads();
      // (4) the requested outputs of the step, rows of P contiguous
      if (p_o) {
        if (a.full_cov) {
          for (int idx = tid; idx < mm; idx += NT) {
            const int i = idx / m, j = idx - i * m;
            p_o[oh * m + idx] = P[i * ld + j];
          }
        } else if (tid < m) {
          p_o[oh + tid] = P[tid * ld + tid];
        }
      }
      if (f_o) {  // F_h = sym(Z P_h Z') + diag(H)
        for (int idx = tid; idx < m * p; idx += NT) {
          const int i = idx / p, o = idx - i * p;
          double s = 0.0;
          for (int j = 0; j < m; ++j) s = fma(P[i * ld + j], Zm[o * m + j], s);
          PZ[i * PM + o] = s;
        }
        __syncthreads();
        if (tid < p * p) {
          const int o = tid / p, o2 = tid - o * p;
          double s = 0.0;
          for (int j = 0; j < m; ++j) s = fma(Zm[o * m + j], PZ[j * PM + o2], s);
          Fm[o * PM + o2] = s;
        }
        __syncthreads();
        if (tid < p * p) {
          const int o = tid / p, o2 = tid - o * p;
          f_o[(size_t)h * p * p + tid] = 0.5 * (Fm[o * PM + o2] + Fm[o2 * PM + o]) + (o == o2 ? hv[o] : 0.0);
        }
      }
    }
    ks_lds* sw = ac;
    ac = an;
    an = sw;
  }
}

}  // namespace dsge
