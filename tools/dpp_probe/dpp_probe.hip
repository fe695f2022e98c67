// GPU box: the FP64 row broadcasts of gfx950 (row_newbcast on v_fmac_f64_dpp / v_mov_b64_dpp, csrc/dsge_device.hpp: row_bcast_f64,
// fmac_row_bcast, pivot_row_bcast_update) -- what they compute and what they cost to issue, one wavefront.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I geconpy_amd/csrc -o tools/dpp_probe/dpp_probe tools/dpp_probe/dpp_probe.hip
//   tools/dpp_probe/dpp_probe > profiles/r14/dpp_probe.txt
// Semantics: lane-dependent operands x, s, d; for J = 0..15 the results of the move, the FMA, the FMA with a negated multiplier, with
// a negated broadcast source, and the in-place form (destination = broadcast source) must EQUAL, in all 64 lanes, the host's
// fma(x[16 (lane / 16) + J], s, d).  Issue cost: clock64 ticks per instruction of a lone wavefront for the DPP forms, v_fma_f64 and
// the read-lane form they replace (two v_readlane_b32 into an SGPR pair + v_fma_f64), each as a dependent chain and as eight
// independent accumulators; then one whole pivot of the filter's 8 x 8 elimination (broadcast of the pivot, v_rcp_f64, Newton step,
// multiplier, seven updates) in three forms: fused, one v_mov_b64_dpp per value + plain FMA, read-lanes + plain FMA.
// Round 15 (profiles/r15/permlane_probe.txt): v_permlane16_swap_b32 on both halves of a double (rows01_pair_f64) -- the row pattern
// it leaves in all 64 lanes against a host table, the builtin and the instruction in place -- the broadcast FMAs that read its
// results two instructions behind them (matvec_sums_row_bcast, every column count), and the mean recursion of the filter's steady step in its
// read-lane form and in the swap + broadcast form: ticks per step and the two forms' bits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "dsge_device.hpp"
using namespace dsge;

__device__ __forceinline__ double readlane_f64(double v, int src_lane) {  // (as the filter kernels have it)
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), src_lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), src_lane);
  return __hiloint2double(hi, lo);
}

constexpr int NJ = 16, NV = 5;  // variants: mov, fmac, fmac -s, fmac -x, fmac in place

template <int J>
__device__ void sem_one(double* out, int lane, double x, double s, double d) {
  double r1 = d, r2 = d, r3 = d, r4 = x;
  const double r0 = row_bcast_f64<J, true>(x);
  fmac_row_bcast<J, true>(r1, x, s);
  asm("s_nop 1\n\tv_fmac_f64_dpp %0, %1, -%2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(r2) : "v"(x), "v"(s), "n"(J));
  asm("s_nop 1\n\tv_fmac_f64_dpp %0, -%1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(r3) : "v"(x), "v"(s), "n"(J));
  asm("s_nop 1\n\tv_fmac_f64_dpp %0, %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "+v"(r4) : "v"(s), "n"(J));
  double* o = out + (size_t)J * NV * 64 + lane;
  o[0] = r0, o[64] = r1, o[128] = r2, o[192] = r3, o[256] = r4;
}
template <int... J>
__device__ void sem_all(std::integer_sequence<int, J...>, double* out, int lane, double x, double s, double d) {
  (sem_one<J>(out, lane, x, s, d), ...);
}
__global__ void semantics(double* out, const double* xs, const double* ss, const double* ds) {
  const int lane = threadIdx.x;
  sem_all(std::make_integer_sequence<int, NJ>{}, out, lane, xs[lane], ss[lane], ds[lane]);
}

// MODE 0 v_fma_f64; 1 v_fmac_f64_dpp, loop-invariant broadcast source; 2 v_fmac_f64_dpp in place (the chain of one accumulator
// carries the wait states: s_nop 1; eight accumulators are seven instructions apart); 3 v_mov_b64_dpp; 4 two v_readlane_b32 + v_fma_f64
// on the SGPR pair, source = the accumulator itself (VALU -> SGPR -> VALU, as the pivot chain has it)
constexpr int N = 8192;
template <int MODE, int IND>
__global__ void rate(double* out, long long* cyc) {
  const int lane = threadIdx.x;
  const double x = 1.0 + lane * 0.03125, s = 1e-5 * (1 + (lane & 3));
  double acc[IND];
#pragma unroll
  for (int i = 0; i < IND; ++i) acc[i] = 1.0 + i + lane;
  __syncthreads();
  const long long t0 = clock64();
  for (int it = 0; it < N / IND; ++it) {
#pragma unroll
    for (int i = 0; i < IND; ++i) {
      if constexpr (MODE == 0) acc[i] = __builtin_fma(x, s, acc[i]);
      if constexpr (MODE == 1) fmac_row_bcast<3, false>(acc[i], x, s);
      if constexpr (MODE == 2) {
        if constexpr (IND == 1)
          asm volatile("s_nop 1\n\tv_fmac_f64_dpp %0, %0, %1 row_newbcast:3 row_mask:0xf bank_mask:0xf" : "+v"(acc[i]) : "v"(s));
        else
          asm volatile("v_fmac_f64_dpp %0, %0, %1 row_newbcast:3 row_mask:0xf bank_mask:0xf" : "+v"(acc[i]) : "v"(s));
      }
      if constexpr (MODE == 3) {
        if constexpr (IND == 1)
          asm volatile("s_nop 1\n\tv_mov_b64_dpp %0, %0 row_newbcast:3 row_mask:0xf bank_mask:0xf" : "+v"(acc[i]));
        else
          asm volatile("v_mov_b64_dpp %0, %0 row_newbcast:3 row_mask:0xf bank_mask:0xf" : "+v"(acc[i]));
      }
      if constexpr (MODE == 4) acc[i] = __builtin_fma(readlane_f64(acc[i], 3), s, acc[i]);
    }
  }
  const long long t1 = clock64();
  double r = 0;
#pragma unroll
  for (int i = 0; i < IND; ++i) r += acc[i];
  out[lane] = r;
  if (lane == 0) cyc[0] = t1 - t0;
}

// seven pivots of the row-per-lane elimination on a diagonally dominant 8 x 8 matrix replicated over the 8-lane groups, NP times.
// FORM 0 fused (the kernel's), 1 v_mov_b64_dpp per value + plain FMA, 2 read-lanes + plain FMA (the parent's).
constexpr int NP = 512;
template <int FORM, int j>
__device__ __forceinline__ void pivot(double (&fr)[8], int r8, double& inv_own) {
  const bool is_j = (r8 == j);
  if constexpr (FORM == 0) {
    const double pj = row_bcast_f64<j, j == 0>(fr[j]);
    double inv = __builtin_amdgcn_rcp(pj);
    inv = inv * fma(-pj, inv, 2.0);
    const double ci = is_j ? 0.0 : fr[j] * inv;
    pivot_row_bcast_update<j, j == 0>(fr, ci);
    fr[j] = is_j ? 1.0 : -ci;
    inv_own = is_j ? inv : inv_own;
  } else {
    double rowj[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      if constexpr (FORM == 1) rowj[q] = row_bcast_f64<j, true>(fr[q]);
      else rowj[q] = readlane_f64(fr[q], j);
    }
    double inv = __builtin_amdgcn_rcp(rowj[j]);
    inv = inv * fma(-rowj[j], inv, 2.0);
    const double ci = is_j ? 0.0 : fr[j] * inv;
#pragma unroll
    for (int q = 0; q < 8; ++q)
      if (q != j) fr[q] = fma(-ci, rowj[q], fr[q]);
    fr[j] = is_j ? 1.0 : -ci;
    inv_own = is_j ? inv : inv_own;
  }
}
template <int FORM>
__global__ void pivots(double* out, long long* cyc, const double* mat) {
  const int lane = threadIdx.x, r8 = lane & 7;
  double base[8], fr[8], sum = 0.0, inv_own = 1.0;
#pragma unroll
  for (int q = 0; q < 8; ++q) base[q] = mat[r8 * 8 + q];
  __syncthreads();
  const long long t0 = clock64();
  for (int it = 0; it < NP; ++it) {
#pragma unroll
    for (int q = 0; q < 8; ++q) fr[q] = base[q] + sum * 1e-9;  // (depends on the previous pass: nothing hoisted, nothing overlapped)
    pivot<FORM, 0>(fr, r8, inv_own);
    pivot<FORM, 1>(fr, r8, inv_own);
    pivot<FORM, 2>(fr, r8, inv_own);
    pivot<FORM, 3>(fr, r8, inv_own);
    pivot<FORM, 4>(fr, r8, inv_own);
    pivot<FORM, 5>(fr, r8, inv_own);
    pivot<FORM, 6>(fr, r8, inv_own);
    sum = fr[0] * inv_own;
  }
  const long long t1 = clock64();
#pragma unroll
  for (int q = 0; q < 8; ++q) out[lane * 8 + q] = fr[q] * inv_own;
  if (lane == 0) cyc[0] = t1 - t0;
}

// ---- v_permlane16_swap_b32 in front of the row broadcasts (rows01_pair_f64, matvec_sums_row_bcast: the steady loop's mean) -------
// Blocks of 64 doubles: 0 x, 1 y of rows01_pair_f64<true>(v); 2 x of rows01_pair_f64<false>(v); 3, 4 the instruction itself on the
// halves of two DIFFERENT registers a = v, b = w, in place, behind its wait states (a: even rows own, odd rows b's even rows; b: even
// rows a's odd rows, odd rows own); then for NC = 10, 12, .., 20 the sums s0, s1 of matvec_sums_row_bcast right behind the swaps.
constexpr int SW_BLOCKS = 5 + 2 * 6;
template <int NC>
__device__ void swap_sums(double* out, int lane, double v, const double (&t)[20]) {
  double s0 = 0.0, s1 = 0.0, x, y;
  rows01_pair_f64<(NC > 16)>(v, x, y);
  if constexpr (NC > 16) matvec_sums_row_bcast<NC>(s0, s1, x, y, t);
  else matvec_sums_row_bcast<NC>(s0, s1, x, x, t);
  out[lane] = s0;
  out[64 + lane] = s1;
}
__global__ void swap_semantics(double* out, const double* vs, const double* ws, const double* ts) {
  const int lane = threadIdx.x;
  const double v = vs[lane], w = ws[lane];
  double t[20];
#pragma unroll
  for (int kk = 0; kk < 20; ++kk) t[kk] = ts[lane * 20 + kk];
  double x, y, x1, y1;
  rows01_pair_f64<true>(v, x, y);
  rows01_pair_f64<false>(v, x1, y1);
  out[lane] = x, out[64 + lane] = y, out[128 + lane] = x1;
  int alo = __double2loint(v), ahi = __double2hiint(v), blo = __double2loint(w), bhi = __double2hiint(w);
  asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %2\n\tv_permlane16_swap_b32 %1, %3" : "+v"(alo), "+v"(ahi), "+v"(blo), "+v"(bhi));
  out[192 + lane] = __hiloint2double(ahi, alo);
  out[256 + lane] = __hiloint2double(bhi, blo);
  swap_sums<10>(out + 5 * 64, lane, v, t);
  swap_sums<12>(out + 7 * 64, lane, v, t);
  swap_sums<14>(out + 9 * 64, lane, v, t);
  swap_sums<16>(out + 11 * 64, lane, v, t);
  swap_sums<18>(out + 13 * 64, lane, v, t);
  swap_sums<20>(out + 15 * 64, lane, v, t);
}

// The mean recursion of the filter's steady step alone, NSTEP dependent steps: afi = av + c, av = sum over NC columns of t[kk] afi[kk]
// in two running sums.  FORM 0: 2 NC read-lanes into SGPR pairs in batches of six to eight columns + NC v_fma_f64 (the present form,
// its scheduling barriers included); FORM 1: two moves, two swaps, NC v_fmac_f64_dpp.
constexpr int NSTEP = 4096;
template <int FORM, int NC>
__global__ void mean_step(double* out, long long* cyc, const double* ts) {
  const int lane = threadIdx.x;
  double t[20];
#pragma unroll
  for (int kk = 0; kk < 20; ++kk) t[kk] = (lane < 28) ? ts[lane * 20 + kk] : 0.0;
  const double c = (lane < 28) ? 1.0 + 0.01 * lane : 0.0;
  double av = 0.0;
  __syncthreads();
  const long long t0 = clock64();
  for (int it = 0; it < NSTEP; ++it) {
    const double afi = av + c;
    double s0 = 0.0, s1 = 0.0;
    if constexpr (FORM == 0) {
#pragma unroll
      for (int b0 = 0; b0 < NC; b0 += 6) {
        const int b1 = (NC - b0 <= 8) ? NC : b0 + 6;
        double afs[8];
#pragma unroll
        for (int kk = b0; kk < b1; ++kk) afs[kk - b0] = readlane_f64(afi, kk);
#pragma unroll
        for (int kk = b0; kk < b1; kk += 2) {
          s0 = fma(t[kk], afs[kk - b0], s0);
          s1 = fma(t[kk + 1], afs[kk + 1 - b0], s1);
        }
        if (b1 == NC) break;
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
      double x, y;
      rows01_pair_f64<(NC > 16)>(afi, x, y);
      if constexpr (NC > 16) matvec_sums_row_bcast<NC>(s0, s1, x, y, t);
      else matvec_sums_row_bcast<NC>(s0, s1, x, x, t);
    }
    av = s0 + s1;
  }
  const long long t1 = clock64();
  out[lane] = av;
  if (lane == 0) cyc[0] = t1 - t0;
}

#define CHECK(e)                                                                    \
  do {                                                                              \
    hipError_t err_ = (e);                                                          \
    if (err_ != hipSuccess) {                                                       \
      printf("%s: %s\n", #e, hipGetErrorString(err_));                              \
      return 1;                                                                     \
    }                                                                               \
  } while (0)

static double* d_out;
static long long* d_cyc;
template <class K, class... A>
static long long timed(K kern, A... args) {
  long long c = -1;
  for (int rep = 0; rep < 3; ++rep) hipLaunchKernelGGL(kern, dim3(1), dim3(64), 0, 0, d_out, d_cyc, args...);
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpy(&c, d_cyc, 8, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return c;
}

int main() {
  CHECK(hipMalloc(&d_out, sizeof(double) * NJ * NV * 64));
  CHECK(hipMalloc(&d_cyc, 64));
  // ---- semantics ------------------------------------------------------------------------------------------------------------
  std::vector<double> x(64), s(64), d(64), got(NJ * NV * 64);
  for (int l = 0; l < 64; ++l) x[l] = 0.1 * l + 1.0 / 3.0, s[l] = 3.0 - l / 7.0, d[l] = -7.0 + 0.001 * l;
  double *dx, *dsv, *dd;
  CHECK(hipMalloc(&dx, 512));
  CHECK(hipMalloc(&dsv, 512));
  CHECK(hipMalloc(&dd, 512));
  CHECK(hipMemcpy(dx, x.data(), 512, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(dsv, s.data(), 512, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(dd, d.data(), 512, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(semantics, dim3(1), dim3(64), 0, 0, d_out, dx, dsv, dd);
  CHECK(hipDeviceSynchronize());
  CHECK(hipMemcpy(got.data(), d_out, sizeof(double) * got.size(), hipMemcpyDeviceToHost));
  const char* vname[NV] = {"v_mov_b64_dpp", "v_fmac_f64_dpp", "v_fmac_f64_dpp, -s", "v_fmac_f64_dpp, -x", "v_fmac_f64_dpp, d = x"};
  int bad_total = 0;
  printf("semantics: row_newbcast:J against the host's fma(x[16 (lane / 16) + J], s, d), compared with == in 64 lanes, J = 0..15\n");
  for (int v = 0; v < NV; ++v) {
    int bad = 0;
    for (int J = 0; J < NJ; ++J)
      for (int l = 0; l < 64; ++l) {
        const double xb = x[16 * (l / 16) + J];
        const double want = v == 0 ? xb : v == 1 ? std::fma(xb, s[l], d[l]) : v == 2 ? std::fma(xb, -s[l], d[l])
                          : v == 3 ? std::fma(-xb, s[l], d[l]) : std::fma(xb, s[l], x[l]);
        const double g = got[((size_t)J * NV + v) * 64 + l];
        if (std::memcmp(&g, &want, 8) != 0) {
          if (bad++ < 3) printf("    J %d lane %d: got %.17g, want %.17g\n", J, l, g, want);
        }
      }
    printf("  %-24s %4d of %d mismatches\n", vname[v], bad, NJ * 64);
    bad_total += bad;
  }
  printf("semantics %s\n\n", bad_total ? "FAILED" : "ok: all 16 J x 64 lanes x 5 forms equal");
  // ---- issue cost -----------------------------------------------------------------------------------------------------------
  printf("issue cost, one wavefront, clock64 ticks per instruction (%d instructions; the read-lane form counts as ONE slot of three instructions)\n", N);
  const long long c[5][2] = {{timed(rate<0, 1>), timed(rate<0, 8>)}, {timed(rate<1, 1>), timed(rate<1, 8>)},
                             {timed(rate<2, 1>), timed(rate<2, 8>)}, {timed(rate<3, 1>), timed(rate<3, 8>)},
                             {timed(rate<4, 1>), timed(rate<4, 8>)}};
  const char* rname[5] = {"v_fma_f64", "v_fmac_f64_dpp (source loop-invariant)", "v_fmac_f64_dpp in place (chain: + s_nop 1)",
                          "v_mov_b64_dpp in place (chain: + s_nop 1)", "2 x v_readlane_b32 + v_fma_f64 (SGPR pair)"};
  printf("  %-46s %12s %12s\n", "", "dependent", "8 independent");
  for (int m = 0; m < 5; ++m) printf("  %-46s %12.2f %12.2f\n", rname[m], (double)c[m][0] / N, (double)c[m][1] / N);
  // ---- one pivot ------------------------------------------------------------------------------------------------------------
  std::vector<double> mat(64), r0(512), r1(512), r2(512);
  for (int i = 0; i < 8; ++i)
    for (int j = 0; j < 8; ++j) mat[i * 8 + j] = (i == j ? 4.0 : 0.0) + 1.0 / (1.0 + i + j) + 0.01 * ((i * 5 + j * 3) % 7);
  double* dm;
  CHECK(hipMalloc(&dm, 512));
  CHECK(hipMemcpy(dm, mat.data(), 512, hipMemcpyHostToDevice));
  const long long p0 = timed(pivots<0>, dm);
  CHECK(hipMemcpy(r0.data(), d_out, 4096, hipMemcpyDeviceToHost));
  const long long p1 = timed(pivots<1>, dm);
  CHECK(hipMemcpy(r1.data(), d_out, 4096, hipMemcpyDeviceToHost));
  const long long p2 = timed(pivots<2>, dm);
  CHECK(hipMemcpy(r2.data(), d_out, 4096, hipMemcpyDeviceToHost));
  printf("\none pivot of the 8 x 8 elimination (7 pivots x %d passes, a pass depends on the one before), clock64 ticks per pivot\n", NP);
  printf("  fused (v_mov_b64_dpp of the pivot + 7 v_fmac_f64_dpp)    %8.1f\n", (double)p0 / (7.0 * NP));
  printf("  8 x v_mov_b64_dpp (s_nop 1 each) + 7 v_fma_f64           %8.1f\n", (double)p1 / (7.0 * NP));
  printf("  16 x v_readlane_b32 + 7 v_fma_f64 (present form)         %8.1f\n", (double)p2 / (7.0 * NP));
  const bool same = std::memcmp(r0.data(), r2.data(), 4096) == 0 && std::memcmp(r1.data(), r2.data(), 4096) == 0;
  printf("  the three forms' results (64 lanes x 8 entries of the scaled inverse): %s\n", same ? "bit-identical" : "DIFFER");
  // ---- lane swap + row broadcasts: the steady loop's mean --------------------------------------------------------------------
  std::vector<double> v(64), w(64), ts(64 * 20), sw(SW_BLOCKS * 64);
  for (int l = 0; l < 64; ++l) {
    v[l] = (l % 5 == 2 ? -1.0 : 1.0) * (0.37 * l + 1.0 / 7.0), w[l] = 1000.0 + l / 3.0;
    for (int kk = 0; kk < 20; ++kk) ts[l * 20 + kk] = 0.04 * std::sin(1.0 + 0.7 * l + 1.3 * kk);
  }
  v[0] = -0.0, v[1] = -0.0;  // (first terms t v = -0 where t > 0: the sums must still start as +0, as the host's fma(t, v, +0) does)
  double *dv, *dw, *dts;
  CHECK(hipMalloc(&dv, 512));
  CHECK(hipMalloc(&dw, 512));
  CHECK(hipMalloc(&dts, sizeof(double) * ts.size()));
  CHECK(hipMemcpy(dv, v.data(), 512, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(dw, w.data(), 512, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(dts, ts.data(), sizeof(double) * ts.size(), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(swap_semantics, dim3(1), dim3(64), 0, 0, d_out, dv, dw, dts);
  CHECK(hipDeviceSynchronize());
  CHECK(hipMemcpy(sw.data(), d_out, sizeof(double) * sw.size(), hipMemcpyDeviceToHost));
  printf("\nv_permlane16_swap_b32 on both halves of a double, against a host table, compared bit for bit in 64 lanes\n");
  int sw_bad_total = 0;
  auto sw_check = [&](const char* what, int block, auto want_of_lane) {
    int bad = 0;
    for (int l = 0; l < 64; ++l) {
      const double g = sw[block * 64 + l], want = want_of_lane(l);
      if (std::memcmp(&g, &want, 8) != 0 && bad++ < 3) printf("    lane %d: got %.17g, want %.17g\n", l, g, want);
    }
    printf("  %-76s %2d of 64 mismatches\n", what, bad);
    sw_bad_total += bad;
  };
  sw_check("rows01_pair_f64<true>  x: v[32 (lane / 32) + (lane & 15)]", 0, [&](int l) { return v[32 * (l / 32) + (l & 15)]; });
  sw_check("rows01_pair_f64<true>  y: v[32 (lane / 32) + 16 + (lane & 15)]", 1, [&](int l) { return v[32 * (l / 32) + 16 + (l & 15)]; });
  sw_check("rows01_pair_f64<false> x", 2, [&](int l) { return v[32 * (l / 32) + (l & 15)]; });
  sw_check("in place, a = v, b = w: a keeps its even rows, odd rows = b's even rows", 3,
           [&](int l) { return ((l >> 4) & 1) ? w[l - 16] : v[l]; });
  sw_check("in place, a = v, b = w: b keeps its odd rows, even rows = a's odd rows", 4,
           [&](int l) { return ((l >> 4) & 1) ? w[l] : v[l + 16]; });
  for (int nc = 10; nc <= 20; nc += 2) {
    for (int par = 0; par < 2; ++par) {
      char what[96];
      snprintf(what, sizeof what, "matvec_sums_row_bcast<%d> right behind the swaps, s%d", nc, par);
      sw_check(what, 5 + (nc - 10) + par, [&](int l) {
        double s = 0.0;
        for (int kk = par; kk < nc; kk += 2) s = std::fma(ts[l * 20 + kk], v[32 * (l / 32) + kk], s);
        return s;
      });
    }
  }
  printf("swap semantics %s\n", sw_bad_total ? "FAILED" : "ok");
  printf("\nthe mean recursion of one steady step (afi = av + c; av = two running sums over NC columns), %d dependent steps, clock64 ticks per step\n",
         NSTEP);
  std::vector<double> m0(64), m1(64);
  bool mean_same = true;
  auto mean_pair = [&](int nc, auto k0, auto k1) {
    const long long c0 = timed(k0, (const double*)dts);
    if (hipMemcpy(m0.data(), d_out, 512, hipMemcpyDeviceToHost) != hipSuccess) return false;
    const long long c1 = timed(k1, (const double*)dts);
    if (hipMemcpy(m1.data(), d_out, 512, hipMemcpyDeviceToHost) != hipSuccess) return false;
    const bool eq = std::memcmp(m0.data(), m1.data(), 512) == 0;
    printf("  NC = %2d   %2d x v_readlane_b32 + %2d v_fma_f64 (present form) %8.1f     2 moves + 2 swaps + %2d v_fmac_f64_dpp %8.1f     results %s\n",
           nc, 2 * nc, nc, (double)c0 / NSTEP, nc, (double)c1 / NSTEP, eq ? "bit-identical" : "DIFFER");
    mean_same = mean_same && eq && c0 > 0 && c1 > 0;
    return true;
  };
  mean_pair(10, mean_step<0, 10>, mean_step<1, 10>);
  mean_pair(16, mean_step<0, 16>, mean_step<1, 16>);
  mean_pair(18, mean_step<0, 18>, mean_step<1, 18>);
  mean_pair(20, mean_step<0, 20>, mean_step<1, 20>);
  return (bad_total || !same || sw_bad_total || !mean_same) ? 1 : 0;
}
