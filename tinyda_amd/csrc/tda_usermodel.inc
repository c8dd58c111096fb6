// User-defined forward models (included by tda_engine.hip): the model is HIP source handed over at run time,
//     __device__ double tda_forward(const double* theta, int dim, int o);     // output o of F(theta)
// compiled with hiprtc together with the step kernel below, so that non-linear models run fused on the device instead of
// through the host protocol (the reference evaluates a Python callable per chain and step, posterior.py:95-96).
// One wave per chain: lane j owns parameter j, the lanes stride over the outputs.  Same step semantics, records and
// RNG inputs as k_mh_steps; proposals, adaptation and Cholesky stay the engine's own kernels.
// MALA (0.5) additionally needs the model's vector-Jacobian product,
//     __device__ double tda_gradient(const double* theta, int dim, const double* sensitivity, int n_outputs, int j);
// = (J(theta)^T sensitivity)_j (the reference's model.gradient(parameters, sensitivity), proposal.py:996-998); its kernels are a
// second program, compiled at init only when the proposal is MALA.
#include <hip/hiprtc.h>

namespace {

struct UserStepArgs {
  long long N, NP;
  int d, DP, m, S, mode, prop_kind;
  double* theta;
  double* lp;
  double* ll;
  const double* scaling;
  int* acc_count;
  const double* inc;
  const double* u;
  const double* data;
  const double* w;  // 1 / diag(noise) or null (isotropic); source-defined likelihood: its per-output parameters
  double var;
  const double* pr_mean;
  const double* pr_pinv;
  const double* pr_lo;
  const double* pr_hi;
  double logconst;
  double* rec_params;
  double* rec_stats;
  unsigned char* rec_acc;
  int* anyacc;          // hierarchy base level: set when a step accepted (may be null)
  unsigned char* ring;  // hierarchy base level: accept-flag ring [ring_P][NP] of the scaling adaptation (may be null)
  int ring_P;
  long long ring_pos;   // absolute position of step 0's entry
};

// level q >= 1 of a hierarchy in ONE launch for a source-defined model: evaluate level q at the states of level q - 1,
// two-stage acceptance, alignment, records (what k_ext_propose + tda_user_eval + k_ext_level_action do in three); the
// uniforms of the step come in through `u` (drawn by the caller: the model source knows nothing of the engine's Philox)
struct UserLevelArgs {
  long long N, NP;
  int d, DP, m, nlev, q;
  const double* data;
  const double* w;
  double var;
  double* theta;
  double* lp;
  double* ll;
  double* Sst;
  int* anyacc;
  const double* u;  // [N]
  double* rec_params;
  double* rec_stats;
  unsigned char* rec_acc;
  unsigned char* ring;
  int ring_P;
  long long ring_pos;
  const double* ysnap;
};

const char* const kUserPrelude = R"SRC(
#include <hip/hip_runtime.h>
__device__ double tda_forward(const double* theta, int dim, int o);
)SRC";

// Source-defined likelihood (TDA_NOISE_SOURCE): log L(F) = sum_o tda_loglike_term(F_o, y_o, p_o, o), the function defined by the
// source after tda_forward.  This prelude goes ahead of the user source and switches the kernels' likelihood over; the
// Gaussian kinds compile without it, so their programs are what they were.  As with tda_gradient, a missing function
// resolves to a tagged template that a static_assert names.  The args' `w` then carries p (not inverted).
const char* const kLogLikePrelude = R"SRC(
#define TDA_LOGLIKE_SOURCE 1
struct tda_loglike_term_missing {};
template <class O>
__device__ tda_loglike_term_missing tda_loglike_term(double, double, double, O) { return {}; }
struct tda_loglike_term_grad_missing {};
template <class O>
__device__ tda_loglike_term_grad_missing tda_loglike_term_grad(double, double, double, O) { return {}; }
)SRC";

const char* const kUserKernel = R"SRC(
#ifdef TDA_LOGLIKE_SOURCE
static_assert(!__is_same(decltype(tda_loglike_term(0.0, 0.0, 0.0, 0)), tda_loglike_term_missing),
              "tda_loglike_term_missing: a source-defined likelihood needs __device__ double tda_loglike_term(double f, double y, double p, int o)");
#endif
struct UserStepArgs {
  long long N, NP;
  int d, DP, m, S, mode, prop_kind;
  double* theta;
  double* lp;
  double* ll;
  const double* scaling;
  int* acc_count;
  const double* inc;
  const double* u;
  const double* data;
  const double* w;
  double var;
  const double* pr_mean;
  const double* pr_pinv;
  const double* pr_lo;
  const double* pr_hi;
  double logconst;
  double* rec_params;
  double* rec_stats;
  unsigned char* rec_acc;
  int* anyacc;          // hierarchy base level: set when a step accepted (may be null)
  unsigned char* ring;  // hierarchy base level: accept-flag ring [ring_P][NP] of the scaling adaptation (may be null)
  int ring_P;
  long long ring_pos;   // absolute position of step 0's entry
};
__device__ __forceinline__ double tda_wave_sum(double v) {
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
extern "C" __global__ void __launch_bounds__(64) tda_user_steps(const UserStepArgs a) {
  __shared__ double s_th[128];  // (65 .. 128 parameters: a lane holds parameters `lane` and `lane + 64`)
  const int lane = threadIdx.x, lane2 = lane + 64;
  const long long c = blockIdx.x;
  if (c >= a.N) return;
  const bool lj = lane < a.d, lj2 = lane2 < a.d;
  double cur = lane < a.DP ? a.theta[c * a.DP + lane] : 0.0, cur2 = lane2 < a.DP ? a.theta[c * a.DP + lane2] : 0.0;
  double lp = a.lp[c], ll = a.ll[c];
  const double scal = a.scaling[c];
  const bool pcn = a.prop_kind == 1, eval = a.mode == 1;
  const double keep = pcn ? sqrt(1.0 - scal * scal) : 1.0;  // proposal.py:351-352
  const double pm = lj ? a.pr_mean[lane] : 0.0, pinv = lj ? a.pr_pinv[lane] : 0.0;
  const double pm2 = lj2 ? a.pr_mean[lane2] : 0.0, pinv2 = lj2 ? a.pr_pinv[lane2] : 0.0;
  int nacc = 0;
  for (int s = 0; s < a.S; ++s) {
    double prp = cur, prp2 = cur2;
    if (!eval) {  // proposal.py:249-251 / :351-355
      const double x = lane < a.DP ? a.inc[((size_t)s * a.NP + c) * a.DP + lane] : 0.0;
      const double x2 = lane2 < a.DP ? a.inc[((size_t)s * a.NP + c) * a.DP + lane2] : 0.0;
      const double sx = scal * x, sx2 = scal * x2;
      prp = pcn ? keep * cur + sx : cur + sx;
      prp2 = pcn ? keep * cur2 + sx2 : cur2 + sx2;
    }
    __syncthreads();
    s_th[lane] = prp;
    s_th[lane2] = prp2;
    __syncthreads();
#ifdef TDA_LOGLIKE_SOURCE
    double sse = 0.0;  // source-defined likelihood: the sum of its terms, a.w = the per-output parameters (link.py:48 takes any loglike)
    for (int o = lane; o < a.m; o += 64) sse += tda_loglike_term(tda_forward(s_th, a.d, o), a.data[o], a.w[o], o);
    sse = tda_wave_sum(sse);
#else
    double sse = 0.0;  // posterior.py:95-108, distributions.py:295-326
    for (int o = lane; o < a.m; o += 64) {
      const double r = tda_forward(s_th, a.d, o) - a.data[o];
      double sq = r * r;
      if (a.w) sq *= a.w[o];
      sse += sq;
    }
    sse = tda_wave_sum(sse);
#endif
    const double dv = prp - pm;
    double pj = lj ? dv * dv * pinv : 0.0;
    if (a.pr_lo && lj && (prp < a.pr_lo[lane] || prp > a.pr_hi[lane])) pj = __builtin_inf();  // uniform prior components
    if (lj2) {
      const double dv2 = prp2 - pm2;
      pj += dv2 * dv2 * pinv2;
      if (a.pr_lo && (prp2 < a.pr_lo[lane2] || prp2 > a.pr_hi[lane2])) pj = __builtin_inf();
    }
    const double maha = tda_wave_sum(pj);
#ifdef TDA_LOGLIKE_SOURCE
    const double ll_n = sse;
#else
    const double ll_n = a.w ? -0.5 * sse : -0.5 * sse / a.var;
#endif
    const double lp_n = -0.5 * (a.logconst + maha);  // scipy MVN logpdf, posterior.py:92
    const double post_n = lp_n + ll_n;               // link.py:48
    bool acc = true;
    if (!eval) {  // chain.py:112
      const double delta = pcn ? ll_n - ll : post_n - (lp + ll);
      double alpha = exp(delta);
      if (post_n != post_n) alpha = 0.0;
      acc = a.u[(size_t)s * a.NP + c] < alpha;
    }
    if (acc) {
      lp = lp_n;
      ll = ll_n;
      cur = prp;
      cur2 = prp2;
    }
    nacc += acc ? 1 : 0;
    if (!eval) {
      const size_t r = (size_t)s * a.N + c;
      if (lane == 0) {
        if (a.rec_stats) {
          a.rec_stats[r * 3 + 0] = lp;
          a.rec_stats[r * 3 + 1] = ll;
          a.rec_stats[r * 3 + 2] = lp + ll;
        }
        if (a.rec_acc) a.rec_acc[r] = acc ? 1 : 0;
        if (a.ring) a.ring[(size_t)((a.ring_pos + s) % a.ring_P) * a.NP + c] = acc ? 1 : 0;
      }
      if (a.rec_params && lj) a.rec_params[r * a.d + lane] = cur;
      if (a.rec_params && lj2) a.rec_params[r * a.d + lane2] = cur2;
    }
  }
  if (lane < a.DP) a.theta[c * a.DP + lane] = cur;
  if (lane2 < a.DP) a.theta[c * a.DP + lane2] = cur2;
  if (lane == 0) {
    a.lp[c] = lp;
    a.ll[c] = ll;
    if (!eval && a.acc_count) a.acc_count[c] += nacc;
    if (!eval && a.anyacc && nacc) a.anyacc[c] = 1;
  }
}
struct UserLevelArgs {
  long long N, NP;
  int d, DP, m, nlev, q;
  const double* data;
  const double* w;
  double var;
  double* theta;
  double* lp;
  double* ll;
  double* Sst;
  int* anyacc;
  const double* u;
  double* rec_params;
  double* rec_stats;
  unsigned char* rec_acc;
  unsigned char* ring;
  int ring_P;
  long long ring_pos;
  const double* ysnap;
};
// one step of level q >= 1 of a hierarchy (chain.py:353-402, :711-737; proposal.py:1515-1545), one wave per chain: the
// same decision, alignment and records as the engine's k_ext_level_action, with the model evaluated in place
extern "C" __global__ void __launch_bounds__(64) tda_user_level_action(const UserLevelArgs a) {
  __shared__ double s_th[128];  // (65 .. 128 parameters: a second parameter per lane)
  const int lane = threadIdx.x, lane2 = lane + 64;
  const long long c = blockIdx.x;
  if (c >= a.N) return;
  const int q = a.q, k = a.q - 1;
  const bool lj = lane < a.d, lj2 = lane2 < a.d;
  const double* ys = a.ysnap ? a.ysnap + (size_t)c * (a.DP + 2) : nullptr;
  double* thk = a.theta + ((size_t)k * a.NP + c) * a.DP;
  double* thq = a.theta + ((size_t)q * a.NP + c) * a.DP;
  const double yj = lj ? (ys ? ys[lane] : thk[lane]) : 0.0, xj = lj ? thq[lane] : 0.0;
  const double yj2 = lj2 ? (ys ? ys[lane2] : thk[lane2]) : 0.0, xj2 = lj2 ? thq[lane2] : 0.0;
  s_th[lane] = yj;
  s_th[lane2] = yj2;
  __syncthreads();
#ifdef TDA_LOGLIKE_SOURCE
  double lls = 0.0;  // source-defined likelihood: a.w = the per-output parameters
  for (int o = lane; o < a.m; o += 64) lls += tda_loglike_term(tda_forward(s_th, a.d, o), a.data[o], a.w[o], o);
  const double lln = tda_wave_sum(lls);
#else
  double sse = 0.0;
  for (int o = lane; o < a.m; o += 64) {
    const double r = tda_forward(s_th, a.d, o) - a.data[o];
    double sq = r * r;
    if (a.w) sq *= a.w[o];
    sse += sq;
  }
  sse = tda_wave_sum(sse);
  const double lln = a.w ? -0.5 * sse : -0.5 * sse / a.var;
#endif
  const double y_lp = ys ? ys[a.DP] : a.lp[(size_t)k * a.NP + c], y_ll = ys ? ys[a.DP + 1] : a.ll[(size_t)k * a.NP + c];
  const double x_lp = a.lp[(size_t)q * a.NP + c], x_ll = a.ll[(size_t)q * a.NP + c];
  const int pkq = q * (q - 1) / 2 + k;
  const double st_lp = a.Sst[((size_t)pkq * 2 + 0) * a.NP + c], st_ll = a.Sst[((size_t)pkq * 2 + 1) * a.NP + c];
  const bool any = a.anyacc[(size_t)k * a.NP + c] != 0;
  const double lpn = y_lp;
  const double alpha = exp(((lpn + lln) - (x_lp + x_ll)) + (st_lp + st_ll) - (y_lp + y_ll));
  const bool acc = any && (a.u[c] < alpha);
  if (acc) {
    if (lane < a.DP) thq[lane] = lj ? yj : 0.0;
    if (lane2 < a.DP) thq[lane2] = lj2 ? yj2 : 0.0;
    if (ys && lane < a.DP) thk[lane] = lj ? yj : 0.0;
    if (ys && lane2 < a.DP) thk[lane2] = lj2 ? yj2 : 0.0;
  } else {
    for (int j = 0; j < q; ++j) {
      if (lane < a.DP) a.theta[((size_t)j * a.NP + c) * a.DP + lane] = lj ? xj : 0.0;
      if (lane2 < a.DP) a.theta[((size_t)j * a.NP + c) * a.DP + lane2] = lj2 ? xj2 : 0.0;
    }
  }
  if (lane == 0) {
    if (acc) {
      a.lp[(size_t)q * a.NP + c] = lpn;
      a.ll[(size_t)q * a.NP + c] = lln;
      a.lp[(size_t)k * a.NP + c] = y_lp;
      a.ll[(size_t)k * a.NP + c] = y_ll;
    } else {
      for (int j = 0; j < q; ++j) {
        const int p = q * (q - 1) / 2 + j;
        a.lp[(size_t)j * a.NP + c] = a.Sst[((size_t)p * 2 + 0) * a.NP + c];
        a.ll[(size_t)j * a.NP + c] = a.Sst[((size_t)p * 2 + 1) * a.NP + c];
      }
    }
    for (int j = 0; j < q; ++j)
      for (int q2 = j + 1; q2 <= q; ++q2) {
        const int p = q2 * (q2 - 1) / 2 + j;
        a.Sst[((size_t)p * 2 + 0) * a.NP + c] = a.lp[(size_t)j * a.NP + c];
        a.Sst[((size_t)p * 2 + 1) * a.NP + c] = a.ll[(size_t)j * a.NP + c];
      }
    a.anyacc[(size_t)k * a.NP + c] = 0;
    if (q < a.nlev - 1 && acc) a.anyacc[(size_t)q * a.NP + c] = 1;
    if (a.rec_stats) {
      const double l1 = a.lp[(size_t)q * a.NP + c], l2 = a.ll[(size_t)q * a.NP + c];
      a.rec_stats[c * 3 + 0] = l1;
      a.rec_stats[c * 3 + 1] = l2;
      a.rec_stats[c * 3 + 2] = l1 + l2;
    }
    if (a.rec_acc) a.rec_acc[c] = acc ? 1 : 0;
    if (a.ring) a.ring[(size_t)(a.ring_pos % a.ring_P) * a.NP + c] = acc ? 1 : 0;
  }
  if (a.rec_params && lj) a.rec_params[c * a.d + lane] = acc ? yj : xj;
  if (a.rec_params && lj2) a.rec_params[c * a.d + lane2] = acc ? yj2 : xj2;
}
// model outputs only, F[c][:] = F(prop[c][:]): the evaluation step of a hierarchy (Delayed Acceptance / MLDA), where the
// engine's level kernels take the outputs from device memory exactly as they take a host callback's
extern "C" __global__ void __launch_bounds__(64) tda_user_eval(long long N, int d, int m, const double* prop, double* F) {
  __shared__ double s_th[128];
  const int lane = threadIdx.x;
  const long long c = blockIdx.x;
  if (c >= N) return;
  s_th[lane] = lane < d ? prop[c * d + lane] : 0.0;
  s_th[lane + 64] = lane + 64 < d ? prop[c * d + lane + 64] : 0.0;
  __syncthreads();
  for (int o = lane; o < m; o += 64) F[c * m + o] = tda_forward(s_th, d, o);
}
)SRC";

// MALA over a source-defined model (proposal.py:945-984): single level, iso / diag noise, diagonal Gaussian prior.  The
// gradient of the log-posterior at the current state is chain state ([NP][DP], like theta; checkpoint blobs carry it).
struct UserMalaArgs {
  long long N, NP;
  int d, DP, m, S;
  double* theta;
  double* lp;
  double* ll;
  double* grad;
  const double* scaling;
  int* acc_count;
  const double* inc;  // unit normals [S][NP][DP] (the proposal factor is the identity)
  const double* u;
  const double* data;
  const double* w;  // 1 / diag(noise) or null (isotropic)
  double var;
  const double* pr_mean;
  const double* pr_pinv;
  double logconst;
  double* rec_params;
  double* rec_stats;
  unsigned char* rec_acc;
};

// (before the user source: the fallback a call resolves to when the source defines no tda_gradient of the contract's signature --
// a non-template function of that signature wins overload resolution against it)
const char* const kMalaPrelude = R"SRC(
struct tda_gradient_missing {};
template <class J>
__device__ tda_gradient_missing tda_gradient(const double*, int, const double*, int, J) { return {}; }
)SRC";

const char* const kMalaKernel = R"SRC(
static_assert(!__is_same(decltype(tda_gradient((const double*)nullptr, 0, (const double*)nullptr, 0, 0)), tda_gradient_missing),
              "tda_gradient_missing: MALA needs __device__ double tda_gradient(const double* theta, int dim, const double* sensitivity, int n_outputs, int j)");
#ifdef TDA_LOGLIKE_SOURCE
static_assert(!__is_same(decltype(tda_loglike_term(0.0, 0.0, 0.0, 0)), tda_loglike_term_missing),
              "tda_loglike_term_missing: a source-defined likelihood needs __device__ double tda_loglike_term(double f, double y, double p, int o)");
static_assert(!__is_same(decltype(tda_loglike_term_grad(0.0, 0.0, 0.0, 0)), tda_loglike_term_grad_missing),
              "tda_loglike_term_grad_missing: MALA needs __device__ double tda_loglike_term_grad(double f, double y, double p, int o)");
#endif
struct UserMalaArgs {
  long long N, NP;
  int d, DP, m, S;
  double* theta;
  double* lp;
  double* ll;
  double* grad;
  const double* scaling;
  int* acc_count;
  const double* inc;
  const double* u;
  const double* data;
  const double* w;
  double var;
  const double* pr_mean;
  const double* pr_pinv;
  double logconst;
  double* rec_params;
  double* rec_stats;
  unsigned char* rec_acc;
};
__device__ __forceinline__ double tda_wave_sum(double v) {
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
// outputs of the model at the parameters in s_th: returns this lane's share of the weighted sum of squares and leaves the
// sensitivity grad_loglike = Sigma^-1 (y - F) in s_sens (distributions.py:300-301 iso: 1 / var * r, :314-315 diag: w * r)
__device__ __forceinline__ double tda_mala_outputs(const UserMalaArgs& a, const double* s_th, double* s_sens, int lane) {
#ifdef TDA_LOGLIKE_SOURCE
  // source-defined likelihood: this lane's share of the log-likelihood itself, and d term / d f as the sensitivity
  double lls = 0.0;
  for (int o = lane; o < a.m; o += 64) {
    const double f = tda_forward(s_th, a.d, o);
    lls += tda_loglike_term(f, a.data[o], a.w[o], o);
    s_sens[o] = tda_loglike_term_grad(f, a.data[o], a.w[o], o);
  }
  return lls;
#else
  const double iv = 1.0 / a.var;
  double sse = 0.0;
  for (int o = lane; o < a.m; o += 64) {
    const double f = tda_forward(s_th, a.d, o);
    const double r = f - a.data[o];
    double sq = r * r;
    if (a.w) sq *= a.w[o];
    sse += sq;
    s_sens[o] = (a.w ? a.w[o] : iv) * (a.data[o] - f);
  }
  return sse;
#endif
}
// one wave per chain: lane j owns parameter j (and j + 64 at 65 .. 128 parameters), the lanes stride over the outputs
extern "C" __global__ void __launch_bounds__(64) tda_user_mala_steps(const UserMalaArgs a) {
  extern __shared__ double s_sens[];  // [m]
  __shared__ double s_th[128];
  const int lane = threadIdx.x, lane2 = lane + 64;
  const long long c = blockIdx.x;
  if (c >= a.N) return;
  const bool lj = lane < a.d, lj2 = lane2 < a.d;
  const size_t row = (size_t)c * a.DP;
  double cur = lj ? a.theta[row + lane] : 0.0, cur2 = lj2 ? a.theta[row + lane2] : 0.0;
  double gc = lj ? a.grad[row + lane] : 0.0, gc2 = lj2 ? a.grad[row + lane2] : 0.0;  // gradient at the current state
  double lp = a.lp[c], ll = a.ll[c];
  const double sg = a.scaling[c], h = 0.5 * sg * sg, kq = -0.5 / (sg * sg);  // proposal.py:953, :1002
  const double pm = lj ? a.pr_mean[lane] : 0.0, pinv = lj ? a.pr_pinv[lane] : 0.0;
  const double pm2 = lj2 ? a.pr_mean[lane2] : 0.0, pinv2 = lj2 ? a.pr_pinv[lane2] : 0.0;
  int nacc = 0;
  for (int s = 0; s < a.S; ++s) {
    const double* z = a.inc + ((size_t)s * a.NP + c) * a.DP;
    const double prp = lj ? (cur + h * gc) + sg * z[lane] : 0.0;  // proposal.py:951-956
    const double prp2 = lj2 ? (cur2 + h * gc2) + sg * z[lane2] : 0.0;
    __syncthreads();  // (the previous step's readers of s_th / s_sens are done)
    s_th[lane] = prp;
    s_th[lane2] = prp2;
    __syncthreads();
    const double sse = tda_wave_sum(tda_mala_outputs(a, s_th, s_sens, lane));
    double pj = 0.0;
    if (lj) {
      const double dv = prp - pm;
      pj = dv * dv * pinv;
    }
    if (lj2) {
      const double dv2 = prp2 - pm2;
      pj += dv2 * dv2 * pinv2;
    }
    const double maha = tda_wave_sum(pj);
#ifdef TDA_LOGLIKE_SOURCE
    const double ll_n = sse;
#else
    const double ll_n = a.w ? -0.5 * sse : -0.5 * sse / a.var;
#endif
    const double lp_n = -0.5 * (a.logconst + maha);  // scipy MVN logpdf, posterior.py:92
    const double post_n = lp_n + ll_n;               // link.py:48
    __syncthreads();  // s_sens complete
    // gradient at the proposal: grad log prior + J^T grad loglike (proposal.py:996-998; utils.py:273-287)
    const double gp = lj ? pinv * (pm - prp) + tda_gradient(s_th, a.d, s_sens, a.m, lane) : 0.0;
    const double gp2 = lj2 ? pinv2 * (pm2 - prp2) + tda_gradient(s_th, a.d, s_sens, a.m, lane2) : 0.0;
    // transition densities (proposal.py:1000-1005): q(x|y) = -|x - y - s^2/2 grad(y)|^2 / (2 s^2)
    const double da = (cur - prp) - h * gp, da2 = (cur2 - prp2) - h * gp2;
    const double db = (prp - cur) - h * gc, db2 = (prp2 - cur2) - h * gc2;
    const double qa = tda_wave_sum(da * da + da2 * da2), qb = tda_wave_sum(db * db + db2 * db2);
    double alpha = exp(((post_n - (lp + ll)) + kq * qa) - kq * qb);  // proposal.py:976-984
    if (post_n != post_n) alpha = 0.0;
    const bool acc = a.u[(size_t)s * a.NP + c] < alpha;  // chain.py:112
    if (acc) {
      lp = lp_n;
      ll = ll_n;
      cur = prp;
      cur2 = prp2;
      gc = gp;
      gc2 = gp2;
    }
    nacc += acc ? 1 : 0;
    const size_t r = (size_t)s * a.N + c;
    if (lane == 0) {
      if (a.rec_stats) {
        a.rec_stats[r * 3 + 0] = lp;
        a.rec_stats[r * 3 + 1] = ll;
        a.rec_stats[r * 3 + 2] = lp + ll;
      }
      if (a.rec_acc) a.rec_acc[r] = acc ? 1 : 0;
    }
    if (a.rec_params && lj) a.rec_params[r * a.d + lane] = cur;
    if (a.rec_params && lj2) a.rec_params[r * a.d + lane2] = cur2;
  }
  if (lane < a.DP) {
    a.theta[row + lane] = cur;
    a.grad[row + lane] = gc;
  }
  if (lane2 < a.DP) {
    a.theta[row + lane2] = cur2;
    a.grad[row + lane2] = gc2;
  }
  if (lane == 0) {
    a.lp[c] = lp;
    a.ll[c] = ll;
    if (a.acc_count) a.acc_count[c] += nacc;
  }
}
// gradient of the log-posterior at the current states (init; the padding of a row is written as zero)
extern "C" __global__ void __launch_bounds__(64) tda_user_mala_grad0(const UserMalaArgs a) {
  extern __shared__ double s_sens[];
  __shared__ double s_th[128];
  const int lane = threadIdx.x, lane2 = lane + 64;
  const long long c = blockIdx.x;
  if (c >= a.N) return;
  const bool lj = lane < a.d, lj2 = lane2 < a.d;
  const size_t row = (size_t)c * a.DP;
  const double th = lj ? a.theta[row + lane] : 0.0, th2 = lj2 ? a.theta[row + lane2] : 0.0;
  s_th[lane] = th;
  s_th[lane2] = th2;
  __syncthreads();
  (void)tda_mala_outputs(a, s_th, s_sens, lane);
  __syncthreads();
  if (lane < a.DP) a.grad[row + lane] = lj ? a.pr_pinv[lane] * (a.pr_mean[lane] - th) + tda_gradient(s_th, a.d, s_sens, a.m, lane) : 0.0;
  if (lane2 < a.DP) a.grad[row + lane2] = lj2 ? a.pr_pinv[lane2] * (a.pr_mean[lane2] - th2) + tda_gradient(s_th, a.d, s_sens, a.m, lane2) : 0.0;
}
)SRC";

// hiprtc for gfx950; on failure `log` holds the (truncated) compiler log and `code` stays empty
int hiprtc_gfx950(const std::string& src, const char* name, std::vector<char>& code, std::string& log) {
  hiprtcProgram prog;
  if (hiprtcCreateProgram(&prog, src.c_str(), name, 0, nullptr, nullptr) != HIPRTC_SUCCESS)
    return fail(TDA_ERR_HIP, "hiprtcCreateProgram failed");
  const char* opts[] = {"--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17"};
  const hiprtcResult cr = hiprtcCompileProgram(prog, 4, opts);
  if (cr != HIPRTC_SUCCESS) {
    size_t n = 0;
    (void)hiprtcGetProgramLogSize(prog, &n);
    log.assign(n, '\0');
    if (n) (void)hiprtcGetProgramLog(prog, &log[0]);
    (void)hiprtcDestroyProgram(&prog);
    return TDA_OK;
  }
  size_t nb = 0;
  (void)hiprtcGetCodeSize(prog, &nb);
  code.resize(nb);
  (void)hiprtcGetCode(prog, code.data());
  (void)hiprtcDestroyProgram(&prog);
  return TDA_OK;
}

// compile prelude + user source + kernel for gfx950; on failure the hiprtc log goes into the error message
int compile_user_model(const char* source, bool loglike, hipModule_t* mod, hipFunction_t* fn, hipFunction_t* fn_eval, hipFunction_t* fn_level) {
  std::string src = std::string(kUserPrelude) + (loglike ? kLogLikePrelude : "") + "\n// ---- user source ----\n" + source + "\n// ---- engine ----\n" + kUserKernel;
  std::vector<char> code;
  std::string log;
  if (int rc = hiprtc_gfx950(src, "tda_user_model.hip", code, log)) return rc;
  if (code.empty()) {
    if (log.find("tda_loglike_term_missing") != std::string::npos)
      return fail(TDA_ERR_INVALID, "a source-defined likelihood: the source defines no __device__ double tda_loglike_term(double f, double y, double p, int o)");
    if (log.size() > 400) log.resize(400);
    return fail(TDA_ERR_INVALID, "the forward-model source does not compile: %s", log.c_str());
  }
  HIP_TRY(hipModuleLoadData(mod, code.data()));
  HIP_TRY(hipModuleGetFunction(fn, *mod, "tda_user_steps"));
  HIP_TRY(hipModuleGetFunction(fn_eval, *mod, "tda_user_eval"));
  HIP_TRY(hipModuleGetFunction(fn_level, *mod, "tda_user_level_action"));
  return TDA_OK;
}

// the MALA program: prelude + user source + MALA kernels.  A source without tda_gradient resolves the kernels' call to the
// tagged fallback template of the prelude, which a static_assert turns into the message below (not an unresolved symbol at load).
int compile_user_mala(const std::string& source, bool loglike, hipModule_t* mod, hipFunction_t* fn, hipFunction_t* fn_grad0) {
  std::string src = std::string(kUserPrelude) + kMalaPrelude + (loglike ? kLogLikePrelude : "") + "\n// ---- user source ----\n" + source + "\n// ---- engine ----\n" + kMalaKernel;
  std::vector<char> code;
  std::string log;
  if (int rc = hiprtc_gfx950(src, "tda_user_mala.hip", code, log)) return rc;
  if (code.empty()) {
    if (log.find("tda_gradient_missing") != std::string::npos)
      return fail(TDA_ERR_INVALID, "MALA on a source-defined model: the source defines no __device__ double tda_gradient(const double* theta, "
                                   "int dim, const double* sensitivity, int n_outputs, int j)");
    if (log.find("tda_loglike_term_grad_missing") != std::string::npos)
      return fail(TDA_ERR_INVALID, "MALA with a source-defined likelihood: the source defines no __device__ double tda_loglike_term_grad(double f, "
                                   "double y, double p, int o)");
    if (log.size() > 400) log.resize(400);
    return fail(TDA_ERR_INVALID, "the forward-model source does not compile with the MALA kernels: %s", log.c_str());
  }
  HIP_TRY(hipModuleLoadData(mod, code.data()));
  HIP_TRY(hipModuleGetFunction(fn, *mod, "tda_user_mala_steps"));
  HIP_TRY(hipModuleGetFunction(fn_grad0, *mod, "tda_user_mala_grad0"));
  return TDA_OK;
}

int launch_user_steps(hipFunction_t fn, UserStepArgs& a, hipStream_t st) {
  size_t sz = sizeof(UserStepArgs);
  void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &sz, HIP_LAUNCH_PARAM_END};
  HIP_TRY(hipModuleLaunchKernel(fn, (unsigned)a.N, 1, 1, 64, 1, 1, 0, st, nullptr, cfg));
  return TDA_OK;
}

int launch_user_level(hipFunction_t fn, UserLevelArgs& a, hipStream_t st) {
  size_t sz = sizeof(UserLevelArgs);
  void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &sz, HIP_LAUNCH_PARAM_END};
  HIP_TRY(hipModuleLaunchKernel(fn, (unsigned)a.N, 1, 1, 64, 1, 1, 0, st, nullptr, cfg));
  return TDA_OK;
}

// one wave per chain, the sensitivity Sigma^-1 (y - F) of its m outputs in dynamic LDS
int launch_user_mala(hipFunction_t fn, UserMalaArgs& a, hipStream_t st) {
  size_t sz = sizeof(UserMalaArgs);
  void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &sz, HIP_LAUNCH_PARAM_END};
  HIP_TRY(hipModuleLaunchKernel(fn, (unsigned)a.N, 1, 1, 64, 1, 1, (unsigned)(a.m * sizeof(double)), st, nullptr, cfg));
  return TDA_OK;
}

int launch_user_eval(hipFunction_t fn, long long N, int d, int m, const double* prop, double* F, hipStream_t st) {
  struct { long long N; int d, m; const double* prop; double* F; } a{N, d, m, prop, F};
  size_t sz = sizeof(a);
  void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &sz, HIP_LAUNCH_PARAM_END};
  HIP_TRY(hipModuleLaunchKernel(fn, (unsigned)N, 1, 1, 64, 1, 1, 0, st, nullptr, cfg));
  return TDA_OK;
}

}  // namespace
