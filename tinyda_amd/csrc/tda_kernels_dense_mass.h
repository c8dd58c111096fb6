// Warm-up adaptation of the dense inverse mass of HMC / NUTS (include/tinyda_amd_dense_mass_adaptation.h writes the algorithm out):
//   k_dense_mass_shift       the pooled mean of the chains' current states: the shift a of the window that starts
//   k_dense_mass_accumulate  folds a block's recorded states into S1 = sum y and S2 = sum y y^T per chunk of 16 chains, y = x - a,
//                            the matrix on v_mfma_f64_16x16x4 (the hot path: it runs behind every block inside a window)
//   k_dense_mass_update      pools the chunks at a window's end, forms the regularised covariance and its Cholesky factor, writes
//                            L and L^T where the step kernels read them at their next launch, and zeroes the sums
// All three belong to the engine's own code object (no source-defined function is called).  Nothing here includes another kernel
// header: the file compiles on its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tda {

constexpr int DMASS_THREADS = 256;  // every kernel below: four waves
constexpr int DMASS_CH = 16;        // chains per chunk

typedef double dmass_f64x4 __attribute__((ext_vector_type(4)));

// tiles of 16 parameters of a padded width DP (8 .. 128), and the tile pairs tj <= ti of the lower triangle
__host__ __device__ constexpr int dmass_tiles(int DP) { return (DP + 15) / 16; }
__host__ __device__ constexpr int dmass_pairs(int T) { return T * (T + 1) / 2; }
// doubles of one chunk's S2: per pair the accumulator of the matrix instruction as the wave holds it, [pair][4][64 lanes]; lane
// (lc = lane & 15, hi = lane >> 4) keeps in register r the entry (row 16 ti + 4 r + hi, column 16 tj + lc)
__host__ __device__ constexpr size_t dmass_s2_doubles(int DP) { return (size_t)dmass_pairs(dmass_tiles(DP)) * 256; }

// a[t] += a[t + s] for s = 128, 64, .., 1, a barrier per level; the sum is a[0] (behind the last barrier)
__device__ inline void dmass_tree(double* a, int t) {
  __syncthreads();
  for (int s = DMASS_THREADS / 2; s >= 1; s >>= 1) {
    if (t < s) a[t] += a[t + s];
    __syncthreads();
  }
}

struct DenseMassShiftArgs {
  const double* x;  // the chains' states: x[c * stride + j]
  int64_t stride;
  double* a;  // [DP]
  int64_t N;  // the real chains
  int d;
};

// One workgroup per padded parameter j (blockIdx.x < DP): thread t adds the chains t, t + 256, .. in that order, the tree adds the
// 256 partial sums (steps 1 - 2 of k_mass_update).  The padding gets an exact zero.
__global__ void __launch_bounds__(DMASS_THREADS) k_dense_mass_shift(DenseMassShiftArgs a) {
  __shared__ double s_a[DMASS_THREADS];
  const int j = blockIdx.x, t = threadIdx.x;
  double sum = 0.0;
  if (j < a.d)
    for (int64_t c = t; c < a.N; c += DMASS_THREADS) sum += a.x[(size_t)c * a.stride + j];
  s_a[t] = sum;
  dmass_tree(s_a, t);
  if (t == 0) a.a[j] = j < a.d ? s_a[0] / (double)a.N : 0.0;
}

struct DenseMassAccumulateArgs {
  const double* rec;  // the block's recorded states, [S][N][d]
  const double* a;    // [DP]: the window's shift, zero in the padding
  double* S1;         // [NC][DP]
  double* S2;         // [NC][pairs][4][64]
  int64_t N;
  int d, DP, S;
};

// the p-th tile pair in row-major order of the lower triangle: p = ti (ti + 1) / 2 + tj
__host__ __device__ constexpr int dmass_pair_row(int p) {
  int ti = 0;
  while ((ti + 1) * (ti + 2) / 2 <= p) ++ti;
  return ti;
}

// acc[I] += y[ti] y[tj]^T for the pairs W + 4 I, I = 0 .. MINE - 1, every index a constant (the arrays stay in registers)
template <int T, int W, int I, int MINE>
__device__ __forceinline__ void dmass_products(const double (&y)[T], dmass_f64x4 (&acc)[MINE]) {
  if constexpr (I < MINE) {
    constexpr int p = W + 4 * I, ti = dmass_pair_row(p), tj = p - ti * (ti + 1) / 2;
    acc[I] = __builtin_amdgcn_mfma_f64_16x16x4f64(y[ti], y[tj], acc[I], 0, 0, 0);
    dmass_products<T, W, I + 1, MINE>(y, acc);
  }
}

// Wave W of the four takes the tile pairs p = W, W + 4, W + 8, ..: at 8 tiles nine accumulators each, 72 registers.  Per step
// and per group g of four chains one matrix instruction per pair, in that order, whatever the block's bounds are.
template <int T, int W>
__device__ __forceinline__ void dmass_accumulate_wave(const DenseMassAccumulateArgs& a, int64_t chunk, int lane) {
  constexpr int NP = dmass_pairs(T), MINE = (NP - W + 3) / 4;
  if constexpr (MINE > 0) {
    const int lc = lane & 15, hi = lane >> 4;
    double* __restrict__ s2 = a.S2 + (size_t)chunk * NP * 256;
    dmass_f64x4 acc[MINE];
#pragma unroll
    for (int i = 0; i < MINE; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[i][r] = s2[((size_t)(W + 4 * i) * 4 + r) * 64 + lane];
    double sh[T];
    bool col[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      col[t] = 16 * t + lc < a.d;
      sh[t] = col[t] ? a.a[16 * t + lc] : 0.0;
    }
    for (int s = 0; s < a.S; ++s) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int64_t ch = chunk * DMASS_CH + 4 * g + hi;
        const double* __restrict__ row = a.rec + ((size_t)s * a.N + (size_t)ch) * a.d + lc;
        double y[T];
#pragma unroll
        for (int t = 0; t < T; ++t) y[t] = (ch < a.N && col[t]) ? row[16 * t] - sh[t] : 0.0;
        dmass_products<T, W, 0, MINE>(y, acc);
      }
    }
#pragma unroll
    for (int i = 0; i < MINE; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) s2[((size_t)(W + 4 * i) * 4 + r) * 64 + lane] = acc[i][r];
  }
}

template <int T>
__device__ __forceinline__ void dmass_accumulate_tiles(const DenseMassAccumulateArgs& a, int64_t chunk, int wave, int lane) {
  switch (wave) {
    case 0: dmass_accumulate_wave<T, 0>(a, chunk, lane); break;
    case 1: dmass_accumulate_wave<T, 1>(a, chunk, lane); break;
    case 2: dmass_accumulate_wave<T, 2>(a, chunk, lane); break;
    default: dmass_accumulate_wave<T, 3>(a, chunk, lane); break;
  }
}

// One workgroup of four waves per chunk of 16 chains (blockIdx.x).  The accumulators live in S2 between blocks: loaded first,
// stored last, so the sums after a window do not depend on how the window was cut.  States come straight from global memory, 16
// consecutive parameters of one chain per 16 lanes; chains >= N and parameters >= d give y = 0 exactly.  Then thread j < DP adds
// the same y to S1[j], step by step and chain by chain in ascending order (the rows are in cache by then).
__global__ void __launch_bounds__(DMASS_THREADS) k_dense_mass_accumulate(DenseMassAccumulateArgs a) {
  const int64_t chunk = blockIdx.x;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  switch (dmass_tiles(a.DP)) {
    case 1: dmass_accumulate_tiles<1>(a, chunk, wave, lane); break;
    case 2: dmass_accumulate_tiles<2>(a, chunk, wave, lane); break;
    case 4: dmass_accumulate_tiles<4>(a, chunk, wave, lane); break;
    default: dmass_accumulate_tiles<8>(a, chunk, wave, lane); break;
  }
  if (tid < a.DP) {
    double s1 = a.S1[(size_t)chunk * a.DP + tid];
    if (tid < a.d) {
      const double sh = a.a[tid];
      const int64_t c0 = chunk * DMASS_CH;
      const int nc = a.N - c0 < DMASS_CH ? (int)(a.N - c0) : DMASS_CH;
      for (int s = 0; s < a.S; ++s) {
        const double* __restrict__ x = a.rec + ((size_t)s * a.N + (size_t)c0) * a.d + tid;
        for (int c = 0; c < nc; ++c) s1 += x[(size_t)c * a.d] - sh;
      }
    }
    a.S1[(size_t)chunk * a.DP + tid] = s1;
  }
}

struct DenseMassUpdateArgs {
  double* S1;             // [NC][DP]: zeroed for the next window
  double* S2;             // [NC][pairs][4][64]
  double* work;           // [DP][DP]: the factor while it is formed, column-major (work[j * DP + i] = L[i][j])
  double* chol;           // [2][DP][DP]: L and L^T
  unsigned int* refused;  // [1]: window ends that left the factor unchanged
  int64_t N;              // the real chains
  int64_t NC;             // chunks
  int d, DP;
  int64_t n;  // states per chain in the window
};

// One workgroup.  Thread t pools the entries t, t + 256, .. of S1 and of S2 over the chunks in ascending order and zeroes them,
// so no thread reads what another has zeroed.  The factorisation is left-looking by columns, thread i on row i, the matrix in
// global memory with a column's entries on consecutive addresses (128 KiB at DP = 128: it runs once per window).
__global__ void __launch_bounds__(DMASS_THREADS) k_dense_mass_update(DenseMassUpdateArgs a) {
  __shared__ double s_m[128];
  __shared__ double s_piv;
  __shared__ int s_bad;
  const int t = threadIdx.x, d = a.d, DP = a.DP;
  const int NP = dmass_pairs(dmass_tiles(DP));
  const double T = (double)a.n * (double)a.N;
  if (t == 0) s_bad = 0;
  // 1 - 2: s1 and the mean
  if (t < DP) {
    double s1 = 0.0;
    for (int64_t c = 0; c < a.NC; ++c) {
      s1 += a.S1[(size_t)c * DP + t];
      a.S1[(size_t)c * DP + t] = 0.0;
    }
    s_m[t] = s1 / T;
  }
  __syncthreads();
  // 1, 3, 4: s2, the covariance and the regulariser, entry by entry of the lower triangle
  for (int e = t; e < NP * 256; e += DMASS_THREADS) {
    double s2 = 0.0;
    for (int64_t c = 0; c < a.NC; ++c) {
      const size_t at = (size_t)c * NP * 256 + e;
      s2 += a.S2[at];
      a.S2[at] = 0.0;
    }
    const int p = e >> 8, r = (e >> 6) & 3, lane = e & 63;
    int ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= p) ++ti;
    const int tj = p - ti * (ti + 1) / 2;
    const int i = 16 * ti + 4 * r + (lane >> 4), j = 16 * tj + (lane & 15);
    if (i < d && j <= i) {
      const double C = (s2 - (T * s_m[i]) * s_m[j]) / (T - 1.0);
      double w = C * T / (T + 5.0);
      if (i == j) w += 1e-3 * 5.0 / (T + 5.0);
      a.work[(size_t)j * DP + i] = w;
    }
  }
  __syncthreads();
  // 5: left-looking Cholesky
  for (int j = 0; j < d; ++j) {
    double acc = 0.0;
    if (t >= j && t < d) {
      acc = a.work[(size_t)j * DP + t];
      for (int k = 0; k < j; ++k) acc = fma(-a.work[(size_t)k * DP + t], a.work[(size_t)k * DP + j], acc);
      if (t == j) {
        const double piv = sqrt(acc);
        if (!(isfinite(acc) && acc > 0.0 && isfinite(piv) && piv > 0.0)) s_bad = 1;
        s_piv = piv;
        a.work[(size_t)j * DP + j] = piv;
      }
    }
    __syncthreads();
    if (t > j && t < d) {
      const double l = acc / s_piv;
      if (!isfinite(l)) s_bad = 1;
      a.work[(size_t)j * DP + t] = l;
    }
    __syncthreads();
  }
  // 6 - 7: the whole factor or nothing
  if (s_bad) {
    if (t == 0) atomicAdd(a.refused, 1u);
    return;
  }
  for (int e = t; e < DP * DP; e += DMASS_THREADS) {
    const int i = e / DP, j = e - i * DP;  // chol[i][j] = L[i][j];  chol[DP DP + i][j] = L[j][i]
    a.chol[e] = (i < d && j <= i) ? a.work[(size_t)j * DP + i] : 0.0;
    a.chol[(size_t)DP * DP + e] = (j < d && i <= j) ? a.work[(size_t)i * DP + j] : 0.0;
  }
}

}  // namespace tda
