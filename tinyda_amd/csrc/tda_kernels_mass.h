// Warm-up adaptation of the diagonal inverse mass of HMC / NUTS (include/tinyda_amd_mass.h writes the algorithm out):
//   k_mass_accumulate  folds a block's recorded states into per-chain running moments (Welford, in step order)
//   k_mass_update      pools the chains' moments at a window's end, writes the regularised variances into the inverse mass that
//                      the step kernels read at their next launch, and zeroes the moments
// Both belong to the engine's own code object (no source-defined function is called).  Neither holds an array per lane.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tda {

constexpr int MASS_THREADS = 256;

struct MassAccumulateArgs {
  const double* rec;  // the block's recorded states, [S][N][d]
  double* mean;       // [N][DP]
  double* M2;         // [N][DP]
  int64_t N;
  int d, DP, S;
  int64_t n0;  // states of the running window folded before this block
};

// One thread per (chain c, parameter j), consecutive threads on consecutive (c, j): every step's row of N * d doubles is read
// front to back by consecutive lanes.  The S states of the pair are folded one after the other,
//   n += 1; delta = x - mean; mean += delta / n; M2 += delta * (x - mean),
// so the moments after a window do not depend on how the window was cut into blocks.
__global__ void __launch_bounds__(MASS_THREADS) k_mass_accumulate(MassAccumulateArgs a) {
  const int64_t nd = a.N * a.d;
  const int64_t idx = (int64_t)blockIdx.x * MASS_THREADS + threadIdx.x;
  if (idx >= nd) return;
  const int64_t c = idx / a.d;
  const int j = (int)(idx - c * a.d);
  const size_t at = (size_t)c * a.DP + j;
  double mean = a.mean[at], M2 = a.M2[at];
  const double* __restrict__ x = a.rec + idx;
  for (int s = 0; s < a.S; ++s) {
    const double xv = x[(size_t)s * nd];
    const double n = (double)(a.n0 + s + 1);
    const double delta = xv - mean;
    mean += delta / n;
    M2 += delta * (xv - mean);
  }
  a.mean[at] = mean;
  a.M2[at] = M2;
}

struct MassUpdateArgs {
  double* mean;           // [N][DP]: zeroed for the next window
  double* M2;             // [N][DP]
  double* inv_mass;       // [DP]
  unsigned int* refused;  // [1]: entries that a window's end left unchanged
  int64_t N;              // the real chains: padding rows are not pooled
  int DP;
  int64_t n;  // states per chain in the window
};

// a[t] += a[t + s] for s = 128, 64, .., 1, a barrier per level; the sum is a[0] (behind the last barrier)
__device__ inline void mass_tree(double* a, int t) {
  __syncthreads();
  for (int s = MASS_THREADS / 2; s >= 1; s >>= 1) {
    if (t < s) a[t] += a[t + s];
    __syncthreads();
  }
}

// One workgroup of 256 threads per parameter j (blockIdx.x).  Thread t takes the chains t, t + 256, .. in that order, in both
// passes and when it zeroes the moments, so no thread reads what another has zeroed.
__global__ void __launch_bounds__(MASS_THREADS) k_mass_update(MassUpdateArgs a) {
  __shared__ double s_a[MASS_THREADS], s_b[MASS_THREADS];
  const int j = blockIdx.x, t = threadIdx.x;
  double sum = 0.0;
  for (int64_t c = t; c < a.N; c += MASS_THREADS) sum += a.mean[(size_t)c * a.DP + j];
  s_a[t] = sum;
  mass_tree(s_a, t);
  const double mbar = s_a[0] / (double)a.N;
  __syncthreads();  // (every thread has read s_a[0] before the second pass overwrites it)
  double B = 0.0, Wn = 0.0;
  for (int64_t c = t; c < a.N; c += MASS_THREADS) {
    const size_t at = (size_t)c * a.DP + j;
    const double dm = a.mean[at] - mbar;
    B += dm * dm;
    Wn += a.M2[at];
    a.mean[at] = 0.0;
    a.M2[at] = 0.0;
  }
  s_a[t] = B;
  s_b[t] = Wn;
  mass_tree(s_a, t);
  mass_tree(s_b, t);
  if (t == 0) {
    const double n = (double)a.n, T = n * (double)a.N;
    const double var = (s_b[0] + n * s_a[0]) / (T - 1.0);
    const double w = var * T / (T + 5.0) + 1e-3 * 5.0 / (T + 5.0);
    if (isfinite(w) && w > 0.0)
      a.inv_mass[j] = w;
    else
      atomicAdd(a.refused, 1u);
  }
}

}  // namespace tda
