// On-device convergence diagnostics (included by tda_engine.hip): rank-normalised split bulk ESS and R-hat of
// Vehtari et al. (2021) -- the estimators behind the `az.summary` tables of the reference's notebooks
// (tinyDA/diagnostics.py:6-111 hands the chains to ArviZ) -- computed from a history that is already in HBM.
// Mirrors tinyda_amd/summaries.py::ess_bulk / rhat operation for operation (that NumPy version is the checker).
//
// Per parameter: split every chain in halves -> pooled average ranks (hipCUB radix sort of (value, position) pairs,
// tie runs resolved by binary search in the sorted keys) -> normal scores -> one batched real FFT of all half-chains;
// only the chain-AVERAGED autocovariance enters Geyer's sequence, so the power spectra are averaged before a single
// inverse transform.  The folded R-hat needs a second sort of |x - median|.
// A NaN among the kept draws of a parameter makes that parameter's ESS and R-hat NaN, as in the NumPy version: k_diag_rank hands
// it a NaN score, which reaches the series' mean and variance and from there both estimates.  Other parameters are untouched.
#include <hipcub/hipcub.hpp>
#include <hipfft/hipfft.h>

namespace {

// half-chain series: s < N: first n kept draws of chain s; s >= N: last n draws of chain s - N
__global__ void k_diag_gather(const double* __restrict__ params, int64_t T, int64_t N, int d, int j, int64_t burnin, int64_t n,
                              double* __restrict__ keys, uint32_t* __restrict__ idx) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= 2 * N * n) return;
  const int64_t s = p / n, i = p % n;
  const int64_t c = s < N ? s : s - N;
  const int64_t t = s < N ? burnin + i : T - n + i;
  keys[p] = params[(t * N + c) * d + j];
  idx[p] = (uint32_t)p;
}

// |x - med| of the same series (folded rank normalisation)
__global__ void k_diag_fold(const double* __restrict__ x, int64_t total, const double* __restrict__ sorted, double* __restrict__ keys,
                            uint32_t* __restrict__ idx) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= total) return;
  const double med = (total & 1) ? sorted[total / 2] : 0.5 * (sorted[total / 2 - 1] + sorted[total / 2]);
  keys[p] = fabs(x[p] - med);
  idx[p] = (uint32_t)p;
}

// average rank of every sorted element (ties share the mean of their positions, scipy.stats.rankdata 'average'),
// normal score, scattered back to the element's original position
__global__ void k_diag_rank(const double* __restrict__ sorted, const uint32_t* __restrict__ idx, int64_t total, double* __restrict__ z) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= total) return;
  const double v = sorted[p];
  if (v != v) {  // a NaN has no rank (the sort leaves it at either end): its score is NaN, and so is everything of this parameter
    z[idx[p]] = v;
    return;
  }
  int64_t lo = 0, hi = p;  // first position holding v
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (sorted[mid] < v) lo = mid + 1; else hi = mid;
  }
  const int64_t first = lo;
  lo = p;
  hi = total;  // one past the last position holding v
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (sorted[mid] <= v) lo = mid + 1; else hi = mid;
  }
  const double r = 0.5 * (double)(first + 1 + lo);  // mean of the 1-based ranks first+1 .. lo
  z[idx[p]] = normcdfinv((r - 0.375) / ((double)total + 0.25));
}

// one workgroup per series: mean, (n-1)-normalised variance, centred copy zero-padded to the FFT length
__global__ void __launch_bounds__(256) k_diag_center(const double* __restrict__ z, int64_t n, int64_t m, double* __restrict__ padded,
                                                     double* __restrict__ mean, double* __restrict__ var) {
  __shared__ double s_part[256];
  const int64_t s = blockIdx.x;
  const double* __restrict__ row = z + s * n;
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) acc += row[i];
  s_part[threadIdx.x] = acc;
  __syncthreads();
  for (unsigned o = 128; o >= 1; o >>= 1) {
    if (threadIdx.x < o) s_part[threadIdx.x] += s_part[threadIdx.x + o];
    __syncthreads();
  }
  const double mu = s_part[0] / (double)n;
  __syncthreads();
  acc = 0.0;
  for (int64_t i = threadIdx.x; i < m; i += 256) {
    const double v = i < n ? row[i] - mu : 0.0;
    if (padded) padded[s * m + i] = v;
    acc += v * v;
  }
  s_part[threadIdx.x] = acc;
  __syncthreads();
  for (unsigned o = 128; o >= 1; o >>= 1) {
    if (threadIdx.x < o) s_part[threadIdx.x] += s_part[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    mean[s] = mu;
    var[s] = s_part[0] / (double)(n - 1);
  }
}

// mean over the series of |X_s[f]|^2, two deterministic stages
__global__ void k_diag_power_partial(const hipfftDoubleComplex* __restrict__ spec, int64_t M, int64_t nf, int64_t rows_per_block,
                                     double* __restrict__ partial) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= nf) return;
  const int64_t s0 = (int64_t)blockIdx.y * rows_per_block, s1 = s0 + rows_per_block < M ? s0 + rows_per_block : M;
  double acc = 0.0;
  for (int64_t s = s0; s < s1; ++s) {
    const hipfftDoubleComplex v = spec[s * nf + f];
    acc += v.x * v.x + v.y * v.y;
  }
  partial[(int64_t)blockIdx.y * nf + f] = acc;
}
__global__ void k_diag_power_final(const double* __restrict__ partial, int64_t nb, int64_t nf, int64_t M, hipfftDoubleComplex* __restrict__ out) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= nf) return;
  double acc = 0.0;
  for (int64_t b = 0; b < nb; ++b) acc += partial[b * nf + f];
  out[f].x = acc / (double)M;
  out[f].y = 0.0;
}

#define FFT_TRY(expr)                                                                     \
  do {                                                                                    \
    hipfftResult _r = (expr);                                                             \
    if (_r != HIPFFT_SUCCESS) return fail(TDA_ERR_HIP, "%s failed: hipfft error %d", #expr, (int)_r); \
  } while (0)

double var_ddof1(const std::vector<double>& v) {
  double mu = 0.0;
  for (double x : v) mu += x;
  mu /= (double)v.size();
  double s = 0.0;
  for (double x : v) s += (x - mu) * (x - mu);
  return s / (double)(v.size() - 1);
}

}  // namespace

extern "C" int tda_diag_ess_rhat(int device, void* stream_, const double* params, int64_t n_steps, int64_t n_chains, int32_t dim,
                                 int64_t burnin, double* ess, double* rhat) {
  if (!params || !ess || !rhat) return fail(TDA_ERR_INVALID, "null argument");
  if (!is_device_ptr(params)) return fail(TDA_ERR_INVALID, "params must be a device pointer ([n_steps][n_chains][dim])");
  if (dim < 1 || n_chains < 1 || burnin < 0 || n_steps - burnin < 8) return fail(TDA_ERR_INVALID, "need at least 8 kept draws");
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream_;
  const int64_t T = n_steps, N = n_chains, n = (T - burnin) / 2, M = 2 * N, total = M * n;
  if (total >= (int64_t)1 << 31) return fail(TDA_ERR_UNSUPPORTED, "history too long for the diagnostics kernels (2 * chains * draws / 2 < 2^31)");
  int64_t m = 1;
  while (m < 2 * n) m <<= 1;
  const int64_t nf = m / 2 + 1;
  DevBuf<double> keys, sorted, x, z, padded, mean_d, var_d, partial, acov;
  DevBuf<uint32_t> idx, idx_sorted;
  DevBuf<hipfftDoubleComplex> spec, pmean;
  DevBuf<char> tmp;
  int rc;
  if ((rc = keys.alloc(total)) || (rc = sorted.alloc(total)) || (rc = x.alloc(total)) || (rc = z.alloc(total)) ||
      (rc = padded.alloc(M * m)) || (rc = mean_d.alloc(M)) || (rc = var_d.alloc(M)) || (rc = acov.alloc(m)) ||
      (rc = idx.alloc(total)) || (rc = idx_sorted.alloc(total)) || (rc = spec.alloc(M * nf)) || (rc = pmean.alloc(nf)))
    return rc;
  const int64_t rows_per_block = 256, nb = (M + rows_per_block - 1) / rows_per_block;
  if ((rc = partial.alloc(nb * nf))) return rc;
  size_t tmp_bytes = 0;
  HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, keys.p, sorted.p, idx.p, idx_sorted.p, (int)total, 0, 64, st));
  if ((rc = tmp.alloc(tmp_bytes))) return rc;
  hipfftHandle fwd, inv;
  int len = (int)m;
  FFT_TRY(hipfftPlanMany(&fwd, 1, &len, nullptr, 1, len, nullptr, 1, (int)nf, HIPFFT_D2Z, (int)M));
  FFT_TRY(hipfftPlanMany(&inv, 1, &len, nullptr, 1, (int)nf, nullptr, 1, len, HIPFFT_Z2D, 1));
  FFT_TRY(hipfftSetStream(fwd, st));
  FFT_TRY(hipfftSetStream(inv, st));
  const unsigned gt = (unsigned)((total + 255) / 256);
  std::vector<double> h_mean(M), h_var(M), h_acov(n);
  int result = TDA_OK;
  for (int j = 0; j < dim && result == TDA_OK; ++j) {
    hipLaunchKernelGGL(k_diag_gather, dim3(gt), dim3(256), 0, st, params, T, N, (int)dim, j, burnin, n, keys.p, idx.p);
    HIP_TRY(hipMemcpyAsync(x.p, keys.p, total * sizeof(double), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp.p, tmp_bytes, keys.p, sorted.p, idx.p, idx_sorted.p, (int)total, 0, 64, st));
    hipLaunchKernelGGL(k_diag_rank, dim3(gt), dim3(256), 0, st, sorted.p, idx_sorted.p, total, z.p);
    hipLaunchKernelGGL(k_diag_center, dim3((unsigned)M), dim3(256), 0, st, z.p, n, m, padded.p, mean_d.p, var_d.p);
    FFT_TRY(hipfftExecD2Z(fwd, padded.p, spec.p));
    hipLaunchKernelGGL(k_diag_power_partial, dim3((unsigned)((nf + 255) / 256), (unsigned)nb), dim3(256), 0, st, spec.p, M, nf,
                       rows_per_block, partial.p);
    hipLaunchKernelGGL(k_diag_power_final, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, st, partial.p, nb, nf, M, pmean.p);
    FFT_TRY(hipfftExecZ2D(inv, pmean.p, acov.p));
    HIP_TRY(hipMemcpyAsync(h_mean.data(), mean_d.p, M * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_var.data(), var_d.p, M * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_acov.data(), acov.p, n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // ---- summaries.py::_ess_raw on the chain-averaged biased autocovariance ----
    for (int64_t t = 0; t < n; ++t) h_acov[t] /= (double)m * (double)n;  // unnormalised inverse transform, biased estimator
    const double mean_var = h_acov[0] * (double)n / ((double)n - 1.0);
    double var_plus = mean_var * ((double)n - 1.0) / (double)n;
    const double b_over_n = M > 1 ? var_ddof1(h_mean) : 0.0;  // variance of the chain means
    var_plus += b_over_n;
    double e = NAN;
    if (var_plus > 0.0) {
      std::vector<double> rho(n);
      for (int64_t t = 0; t < n; ++t) rho[t] = 1.0 - (mean_var - h_acov[t]) / var_plus;
      rho[0] = 1.0;
      const int64_t npair = n / 2;
      double tau = -1.0, run = INFINITY;
      int64_t k = 0;
      for (; k < npair; ++k) {
        const double pk = rho[2 * k] + rho[2 * k + 1];
        if (pk < 0.0) break;
        run = pk < run ? pk : run;  // initial monotone sequence
        tau += 2.0 * run;
      }
      if (k < npair && rho[2 * k] > 0.0) tau += rho[2 * k];
      const double floor_tau = 1.0 / std::log10((double)M * (double)n);
      tau = tau > floor_tau ? tau : floor_tau;
      e = (double)M * (double)n / tau;
    }
    ess[j] = e;
    // ---- summaries.py::rhat: bulk part from the same normal scores ----
    auto rhat_of = [&](const std::vector<double>& vars, const std::vector<double>& means) {
      double w = 0.0;
      for (double v : vars) w += v;
      w /= (double)vars.size();
      const double b = (double)n * var_ddof1(means);
      return std::sqrt((((double)n - 1.0) / (double)n * w + b / (double)n) / w);
    };
    const double r_bulk = M > 1 ? rhat_of(h_var, h_mean) : NAN;
    // ---- folded part: ranks of |x - median| ----
    hipLaunchKernelGGL(k_diag_fold, dim3(gt), dim3(256), 0, st, x.p, total, sorted.p, keys.p, idx.p);
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp.p, tmp_bytes, keys.p, sorted.p, idx.p, idx_sorted.p, (int)total, 0, 64, st));
    hipLaunchKernelGGL(k_diag_rank, dim3(gt), dim3(256), 0, st, sorted.p, idx_sorted.p, total, z.p);
    hipLaunchKernelGGL(k_diag_center, dim3((unsigned)M), dim3(256), 0, st, z.p, n, n, (double*)nullptr, mean_d.p, var_d.p);
    HIP_TRY(hipMemcpyAsync(h_mean.data(), mean_d.p, M * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_var.data(), var_d.p, M * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const double r_fold = M > 1 ? rhat_of(h_var, h_mean) : NAN;
    rhat[j] = r_bulk > r_fold ? r_bulk : r_fold;
  }
  (void)hipfftDestroy(fwd);
  (void)hipfftDestroy(inv);
  HIP_TRY(hipGetLastError());
  return result;
}
