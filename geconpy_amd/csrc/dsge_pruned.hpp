// SECOND-ORDER post-solve dynamics per draw: simulation of the pruned system (Kim, Kim, Schaumburg & Sims) and generalised impulse
// responses, from the policy function dsge_second_order_logp_batched returns (T, R and g_yy, g_yu, g_uu, g_ss on the state columns S)
//     x_f' = T x_f + R u
//     x_s' = T x_s + 1/2 g_yy (f (x) f) + g_yu (f (x) u) + 1/2 g_uu (u (x) u) + 1/2 g_ss,      f = x_f[S],      x = x_f + x_s
// -- the recursion of oracle/second_order.py::simulate_pruned, in the time indexing of dsge_simulate_batched.
//
// pruned_pack_kernel, once per draw: the second-order blocks as ONE zero-padded panel
//     P = [ 1/2 sym-folded g_yy | g_yu | 1/2 sym-folded g_uu | 1/2 g_ss ]        16 ceil(n / 16) rows x Kp16 columns
// on the monomials  mon = [ f_a f_b (a <= b, row-major upper) ; f_a u_j (a-major) ; u_i u_j (i <= j) ; 1 ],  folded columns
// 1/2 (g[:, a, b] + g[:, b, a]) off the diagonal and 1/2 g[:, a, a] on it (exact whether or not the input is symmetric).  The panel
// does not fit the LDS (n = 40, s = 18, k = 7: 48 x 336 doubles; n = 64, s = 24, k = 12: 64 x 672), so it lives in library scratch and
// is stored in FRAGMENT ORDER: the 64 A values of v_mfma_f64_16x16x4_f64 for (row tile, four columns) are contiguous, one coalesced
// 512-byte load per wavefront and product.
//
// pruned_propagate_kernel: one workgroup of 256 threads per (draw, group of 16 paths), on the scheme of the first-order propagation:
// [T | R] in one padded LDS image, [x_f ; u_t] of the 16 paths path-major and double-buffered, x_s likewise.  A step is
//     x_f' = [T | R] [x_f ; u]                                     ks_gemm, K = n4 + k4
//     x_s' = T x_s + P mon                                         one accumulator per row tile: T out of LDS, P out of L2
// with NO monomial image: every monomial is a product v_p v_q of two entries of the path's row [x_f ; u ; 1 ; 0] of the x_f image
// (the constant 1 and a zero for the padding columns sit behind the shocks), so the B fragment of a panel product is two LDS reads
// through a table of (p, q) pairs built once per workgroup, and one multiplication.  All products read the current images and write
// the other ones: one barrier per step, after which the slab of the step is written once.
// Generalised impulse responses: one workgroup per (draw, impulse), baseline path p in column p and the same path with the impulse
// added to e_0 in column 8 + p, 8 pairs per pass; after each step thread i adds the differences of the pass in ascending path
// order to girf[t][i] (the same thread at every pass: no atomics, the mean is reproducible bit for bit).
// Padding, stride, [T | R] staging, the x_f product step and the NaN fill: dsge_postsolve.hpp (docs/design/dynamics.md).
#pragma once
#include "dsge_postsolve.hpp"

namespace dsge {

constexpr int PR_THREADS = 256, PR_COLS = 16, PR_PAIRS = 8;
constexpr int PR_MAX_N = 64, PR_MAX_S = 24, PR_MAX_K = 12;

// columns of the panel: the monomials, padded to four products (16 columns) per pass of the product loop
__host__ __device__ inline int pr_kp(int s, int k) { return s * (s + 1) / 2 + s * k + k * (k + 1) / 2 + 1; }
__host__ __device__ inline int pr_kp16(int s, int k) { return (pr_kp(s, k) + 15) & ~15; }
// row stride of the [T | R] and [x_f ; u ; 1 ; 0] images (two columns behind the shocks) / of the x_s images (no shocks)
__host__ __device__ inline int pr_ld(int n, int k) { return ps_ld(n, k, 2); }
__host__ __device__ inline int pr_lds(int n) { return ps_ld(n, 0); }
__host__ __device__ inline size_t pr_panel_doubles(int n, int s, int k) { return (size_t)ks_mp(n) * pr_kp16(s, k); }
__host__ __device__ inline size_t pr_lds_doubles(int n, int s, int k) {
  return (size_t)(ks_mp(n) + 2 * PR_COLS) * pr_ld(n, k) + (size_t)2 * PR_COLS * pr_lds(n) + pr_kp16(s, k) / 2;
}

struct PrunedPackArgs {
  const double* gyy;      // [batch][n][s][s]
  const double* gyu;      // [batch][n][s][k]
  const double* guu;      // [batch][n][k][k]
  const double* gss;      // [batch][n]
  const int32_t* status;  // [batch] or nullptr: a failed draw is not packed (and not read)
  double* panel;          // [batch][pr_panel_doubles]
  int batch, n, s, k;
};

// column c of the monomial list -> its kind and index pair: 0 = f_a f_b, 1 = f_a u_b, 2 = u_a u_b, 3 = the constant, 4 = padding
__device__ __forceinline__ int pr_column(int c, int s, int k, int* a_out, int* b_out) {
  const int nff = s * (s + 1) / 2, nfu = s * k, nuu = k * (k + 1) / 2;
  int kind, w, r;
  if (c < nff) { kind = 0; w = s; r = c; }
  else if (c < nff + nfu) { *a_out = (c - nff) / k; *b_out = (c - nff) % k; return 1; }
  else if (c < nff + nfu + nuu) { kind = 2; w = k; r = c - nff - nfu; }
  else { *a_out = *b_out = 0; return c == nff + nfu + nuu ? 3 : 4; }
  int a = 0;
  while (r >= w - a) {  // row a of the upper triangle holds w - a pairs
    r -= w - a;
    ++a;
  }
  *a_out = a;
  *b_out = a + r;
  return kind;
}

__global__ __launch_bounds__(PR_THREADS) void pruned_pack_kernel(PrunedPackArgs a) {
  const int draw = blockIdx.x, n = a.n, s = a.s, k = a.k;
  if (draw >= a.batch || (a.status && a.status[draw] != 0)) return;
  const int kp16 = pr_kp16(s, k), nk4 = kp16 / 4, total = (ks_mp(n) / 16) * nk4 * 64;
  const double* gyy = a.gyy + (size_t)draw * n * s * s;
  const double* gyu = a.gyu + (size_t)draw * n * s * k;
  const double* guu = a.guu + (size_t)draw * n * k * k;
  const double* gss = a.gss + (size_t)draw * n;
  double* out = a.panel + (size_t)draw * pr_panel_doubles(n, s, k);
  for (int idx = threadIdx.x; idx < total; idx += PR_THREADS) {  // element (tile ti, product kk, lane)
    const int lane = idx & 63, kk = (idx >> 6) % nk4, ti = (idx >> 6) / nk4;
    const int i = 16 * ti + (lane & 15), c = 4 * kk + (lane >> 4);
    double v = 0.0;
    if (i < n) {
      int p, q;
      switch (pr_column(c, s, k, &p, &q)) {
        case 0: v = p == q ? 0.5 * gyy[(i * s + p) * s + p] : 0.5 * (gyy[(i * s + p) * s + q] + gyy[(i * s + q) * s + p]); break;
        case 1: v = gyu[(i * s + p) * k + q]; break;
        case 2: v = p == q ? 0.5 * guu[(i * k + p) * k + p] : 0.5 * (guu[(i * k + p) * k + q] + guu[(i * k + q) * k + p]); break;
        case 3: v = 0.5 * gss[i]; break;
        default: break;
      }
    }
    out[idx] = v;
  }
}

struct PrunedArgs {
  const double* T;        // [batch][n][n]
  const double* R;        // [batch][n][k]
  const double* panel;    // [batch][pr_panel_doubles], from pruned_pack_kernel
  const double* eps;      // [batch | 1][n_paths][n_shock_steps][k] or nullptr (no shocks)
  long long eps_draw;     // n_paths * n_shock_steps * k or 0
  const double* xf0;      // [batch | 1][n_paths][n] or nullptr (zero)
  const double* xs0;
  long long x0_draw;      // n_paths * n or 0
  const double* imp;      // girf: [batch | 1][k][c] or nullptr (unit impulses, nothing read)
  long long imp_draw;     // k * c or 0
  const int32_t* status;  // [batch] or nullptr
  double* x_out;          // simulate: [batch][n_paths][n_steps][n], each may be nullptr
  double* xf_out;
  double* xs_out;
  double* girf_out;       // girf: [batch][c][n_steps][n]
  int batch, n, s, k, n_paths, n_steps, n_shock_steps;
  int units;              // workgroups per draw: groups of 16 paths (simulate) or impulses (girf)
  int girf;
  unsigned char S[PR_MAX_S];  // the state columns, strictly ascending
  long long* dbg;         // debug (dsge_debug_pruned_phases): int64[8], shader-clock cycles of wavefront 0 of workgroup 0, summed over
                          // the steps: x_f product, T x_s, P mon, wait at the barrier, slab; then total, steps, set-up
};

__global__ __launch_bounds__(PR_THREADS) void pruned_propagate_kernel(PrunedArgs a) {
  constexpr int NT = PR_THREADS, NC = PR_COLS;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int tid = threadIdx.x, n = a.n, k = a.k, s = a.s;
  const int draw = blockIdx.x / a.units, unit = blockIdx.x - draw * a.units;
  if (draw >= a.batch) return;
  const size_t path_sz = (size_t)a.n_steps * n;
  // simulate: the unit is a group of 16 paths; girf: the unit is an impulse, the passes run over groups of 8 baseline paths
  const int passes = a.girf ? (a.n_paths + PR_PAIRS - 1) / PR_PAIRS : 1;
  double* go = a.girf ? a.girf_out + ((size_t)draw * a.units + unit) * path_sz : nullptr;
  if (a.status && a.status[draw] != 0) {  // failed solve: EVERY output of the draw is NaN
    if (a.girf) {
      ps_fill_nan(go, path_sz, tid, NT);
    } else {
      const int s0 = unit * NC, nc = a.n_paths - s0 < NC ? a.n_paths - s0 : NC;
      const size_t o = ((size_t)draw * a.n_paths + s0) * path_sz;
      if (a.x_out) ps_fill_nan(a.x_out + o, (size_t)nc * path_sz, tid, NT);
      if (a.xf_out) ps_fill_nan(a.xf_out + o, (size_t)nc * path_sz, tid, NT);
      if (a.xs_out) ps_fill_nan(a.xs_out + o, (size_t)nc * path_sz, tid, NT);
    }
    return;
  }
  const int n4 = ps_r4(n), k4 = ps_r4(k), mp = ks_mp(n), mt = mp / 16, ld = pr_ld(n, k), lds = pr_lds(n);
  const int kp16 = pr_kp16(s, k), nk4 = kp16 / 4, one = n4 + k4, zero = one + 1;
  ks_lds* TR = (ks_lds*)smem;     // [mp][ld]: T in columns 0 .. n-1, R in columns n4 .. n4+k-1
  ks_lds* fcur = TR + mp * ld;    // [NC][ld]: x_f of column j in 0 .. n-1, u_t in n4 .. n4+k-1, 1 at `one`, 0 at `zero`
  ks_lds* fnxt = fcur + NC * ld;
  ks_lds* scur = fnxt + NC * ld;  // [NC][lds]: x_s
  ks_lds* snxt = scur + NC * lds;
  __attribute__((address_space(3))) int* tab = (__attribute__((address_space(3))) int*)(snxt + NC * lds);  // [kp16]: p | q << 16
  for (size_t idx = tid; idx < pr_lds_doubles(n, s, k); idx += NT) TR[idx] = 0.0;
  __syncthreads();
  ps_stage_TR(TR, ld, n4, a.T + (size_t)draw * n * n, a.R + (size_t)draw * n * k, n, k, tid, NT);
  if (tid < 2 * NC) (tid < NC ? fcur : fnxt)[(tid & (NC - 1)) * ld + one] = 1.0;
  for (int c = tid; c < kp16; c += NT) {
    int p, q, e;
    switch (pr_column(c, s, k, &p, &q)) {
      case 0: e = a.S[p] | a.S[q] << 16; break;
      case 1: e = a.S[p] | (n4 + q) << 16; break;
      case 2: e = (n4 + p) | (n4 + q) << 16; break;
      case 3: e = one | one << 16; break;
      default: e = zero | zero << 16; break;
    }
    tab[c] = e;
  }
  const ks_glb* panel = (const ks_glb*)(a.panel + (size_t)draw * pr_panel_doubles(n, s, k));
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 15, lk = lane >> 4;
  // what this thread loads of the shocks of a step: entry (column j, component c)
  const int ej = tid / k, ec = tid - ej * k;
  const double inv_paths = 1.0 / (double)a.n_paths;
  const bool prof = a.dbg != nullptr && blockIdx.x == 0 && wave == 0;
  long long pc[5] = {0, 0, 0, 0, 0}, p_begin = prof ? clock64() : 0, p_setup = 0, p_steps = 0;

  for (int pass = 0; pass < passes; ++pass) {
    // column j of this pass is path `first + (girf ? j & 7 : j)`, for j < nc (girf: pairs (j, 8 + j), j < nc)
    const int first = a.girf ? pass * PR_PAIRS : unit * NC;
    const int left = a.n_paths - first, nc = a.girf ? (left < PR_PAIRS ? left : PR_PAIRS) : (left < NC ? left : NC);
    auto path_of = [&](int j) -> int {  // -1: the column carries nothing
      const int jj = a.girf ? (j & (PR_PAIRS - 1)) : j;
      return jj < nc ? first + jj : -1;
    };
    auto shock = [&](int t) -> double {  // entry (ej, ec) of u_t
      double v = 0.0;
      if (ej >= NC) return v;
      const int p = path_of(ej);
      if (p < 0) return v;
      if (a.eps && t < a.n_shock_steps)
        v = a.eps[(size_t)draw * a.eps_draw + ((size_t)p * a.n_shock_steps + t) * k + ec];
      if (a.girf && ej >= PR_PAIRS && t == 0)
        v += a.imp ? a.imp[(size_t)draw * a.imp_draw + (size_t)ec * a.units + unit] : (ec == unit ? 1.0 : 0.0);
      return v;
    };
    __syncthreads();  // (the last readers of the images of the pass before)
    for (int idx = tid; idx < NC * n; idx += NT) {
      const int j = idx / n, i = idx - j * n, p = path_of(j);
      const size_t o = (size_t)draw * a.x0_draw + (size_t)(p < 0 ? 0 : p) * n + i;
      fcur[j * ld + i] = (p >= 0 && a.xf0) ? a.xf0[o] : 0.0;
      scur[j * lds + i] = (p >= 0 && a.xs0) ? a.xs0[o] : 0.0;
    }
    if (ej < NC) fcur[ej * ld + n4 + ec] = shock(0);
    __syncthreads();
    if (prof && pass == 0) p_setup = clock64() - p_begin;
    for (int t = 0; t < a.n_steps; ++t) {
      long long p0 = prof ? clock64() : 0, p1 = 0, p2 = 0;
      const double ev = shock(t + 1);  // u_{t+1}, in flight while this step multiplies (zero behind the last shock)
      ps_step(TR, fcur, fnxt, ld, mt, n4 + k4, n4);
      if (prof) p1 = clock64();
      for (int ti = wave; ti < mt; ti += 4) {  // x_s' = T x_s + P mon: one accumulator per row tile
        ks_v4f64 acc = {0.0, 0.0, 0.0, 0.0};
        const ks_lds* pa = (const ks_lds*)TR + (16 * ti + li) * ld + lk;
        const ks_lds* pb = (const ks_lds*)scur + li * lds + lk;
        for (int k0 = 0; k0 < n4; k0 += 4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[k0], pb[k0], acc, 0, 0, 0);
        if (prof) p2 = clock64();
        const ks_glb* pg = panel + (size_t)ti * nk4 * 64 + lane;
        const ks_lds* row = (const ks_lds*)fcur + li * ld;
        double av[4], an[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) av[q] = pg[q * 64];
        for (int kk = 0; kk < nk4; kk += 4) {  // four products per pass; the panel fragments of the next pass are loaded first
          const bool more = kk + 4 < nk4;
#pragma unroll
          for (int q = 0; q < 4; ++q) an[q] = more ? pg[(kk + 4 + q) * 64] : 0.0;
          double bv[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int e = tab[4 * (kk + q) + lk];
            bv[q] = row[e & 0xffff] * row[e >> 16];
          }
#pragma unroll
          for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[q], bv[q], acc, 0, 0, 0);
#pragma unroll
          for (int q = 0; q < 4; ++q) av[q] = an[q];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int i = 16 * ti + lk + 4 * e;
          if (i < n4) snxt[li * lds + i] = acc[e];
        }
      }
      if (ej < NC) fnxt[ej * ld + n4 + ec] = ev;
      const long long p3 = prof ? clock64() : 0;
      __syncthreads();
      const long long p4 = prof ? clock64() : 0;
      if (a.girf) {
        if (tid < n) {  // the differences of this pass, paths in ascending order, behind those of the passes before
          double sum = pass == 0 ? 0.0 : go[(size_t)t * n + tid];
          for (int p = 0; p < nc; ++p)
            sum += (fnxt[(PR_PAIRS + p) * ld + tid] - fnxt[p * ld + tid]) + (snxt[(PR_PAIRS + p) * lds + tid] - snxt[p * lds + tid]);
          go[(size_t)t * n + tid] = pass == passes - 1 ? sum * inv_paths : sum;
        }
      } else {
        const size_t o = ((size_t)draw * a.n_paths + first) * path_sz + (size_t)t * n;
        for (int idx = tid; idx < nc * n; idx += NT) {  // the slab of this step: n contiguous doubles per path
          const int j = idx / n, i = idx - j * n;
          const double f = fnxt[j * ld + i], sv = snxt[j * lds + i];
          const size_t oo = o + (size_t)j * path_sz + i;
          if (a.x_out) a.x_out[oo] = f + sv;
          if (a.xf_out) a.xf_out[oo] = f;
          if (a.xs_out) a.xs_out[oo] = sv;
        }
      }
      if (prof) {
        pc[0] += p1 - p0; pc[1] += p2 - p1; pc[2] += p3 - p2; pc[3] += p4 - p3; pc[4] += clock64() - p4;
        ++p_steps;
      }
      ps_swap(fcur, fnxt);
      ps_swap(scur, snxt);
    }
  }
  if (prof && lane == 0) {
    for (int i = 0; i < 5; ++i) a.dbg[i] = pc[i];
    a.dbg[5] = clock64() - p_begin;
    a.dbg[6] = p_steps;
    a.dbg[7] = p_setup;
  }
}

}  // namespace dsge
