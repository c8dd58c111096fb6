// The programs that hiprtc compiles at run time together with a user's HIP source (tda_usermodel.inc; embedded in the library as
// text, and compiled offline as it stands by tests/extprogram.py).  The user's source is the header "tda_user_source.h":
//     __device__ double tda_forward(const double* theta, int dim, int o);     // output o of F(theta)
// so that non-linear models run fused on the device instead of through the host protocol (the reference evaluates a Python
// callable per chain and step, posterior.py:95-96).  One wave per chain: lane j owns parameter j (and j + 64 at 65 .. 128
// parameters), the lanes stride over the outputs.  Same step semantics, records and RNG inputs as k_mh_steps; proposals,
// adaptation and Cholesky stay the engine's own kernels.
// A model whose outputs all come from one solve (an integrator, a time-stepping scheme, a tridiagonal solve) defines the
// wave-cooperative form instead, tda_forward_wave: the 64 lanes of the chain's wave call it together, once per evaluation;
// theta and out are LDS (out: n_outputs doubles, NaN before the call: an entry left unwritten rejects the proposal), `work` is
// TDA_WORKSPACE doubles of LDS of the chain's own (a #define of the source; 0 / undefined: null), __syncthreads() inside is legal
// and a wave barrier (one wave per workgroup).
// Compile options select what is built (the file itself never defines them; the signature of every function named here is
// written once, TDA_SIG_* in tda_user_args.h).  Seven for the programs that sample:
//   -DTDA_USER_MALA       the MALA kernels (tda_user_mala_steps, tda_user_mala_grad0) instead of tda_user_steps,
//                         tda_user_level_action and tda_user_eval.  MALA (0.5) needs the model's vector-Jacobian product,
//                         tda_gradient = (J(theta)^T sensitivity)_j (the reference's model.gradient(parameters, sensitivity), proposal.py:996-998)
//   -DTDA_LOGLIKE_SOURCE  source-defined likelihood (TDA_NOISE_SOURCE): log L(F) = sum_o tda_loglike_term(F_o, y_o, p_o, o), defined
//                         by the source after tda_forward; the args' `w` then carries p (not inverted).  MALA also needs
//                         tda_loglike_term_grad, d term / d f.  The Gaussian kinds compile without it.
//   -DTDA_LOGLIKE_WAVE    (in addition to -DTDA_LOGLIKE_SOURCE) the likelihood couples outputs: the source defines the wave form instead of
//                         the term, tda_loglike_wave.  The outputs go through LDS (s_out[m]; a per-output model fills it first), the
//                         chain's 64 lanes call the function together, once per evaluation, and the engine sums the 64 returns.  f is
//                         the complete outputs in LDS, y / p the data and the parameters as given (device memory).  Every lane is called,
//                         lanes >= n_outputs too; how the work spreads over the lanes is the function's own business
//                         (for (o = lane; o < n_outputs; o += 64)).  No barriers, no workspace, no writes; wave shuffles are legal (the
//                         call site is converged).  A NaN or -inf share rejects.  MALA also needs tda_loglike_grad_wave, one call by the
//                         whole wave that writes d log L / d f_o for every output into sens (LDS, n_outputs doubles, NaN before the call:
//                         an entry left unwritten makes the gradient NaN and rejects); the MALA program then holds 2 m doubles of
//                         dynamic LDS, the sensitivities and behind them the outputs (a coupled gradient reads its neighbours)
//   -DTDA_PRIOR_SOURCE    source-defined prior (tda_engine_set_prior_joint, kind TDA_PRIOR_SOURCE): log p(theta) = sum_j
//                         tda_logprior_term(theta_j, p_j, q_j, j), defined by the source; the args' `pr_mean` / `pr_pinv` then carry
//                         p / q as given.  tda_user_steps and the MALA kernels evaluate it (the level action carries the log-prior
//                         of the state it promotes).  MALA also needs tda_logprior_term_grad, d term / d x.
//                         Outside the support its value is free (NaN, +-inf, anything): the term is -inf there and rejects.
//   -DTDA_PRIOR_WAVE      (in addition to -DTDA_PRIOR_SOURCE) the prior couples parameters: the source defines the wave form instead of
//                         the term, tda_logprior_wave.  The chain's 64 lanes call it together, once per evaluation, and the engine sums
//                         the 64 returns.  theta is the proposal in LDS (entries at index >= dim are unspecified), p / q the arrays as given (device
//                         memory).  Every lane is called, lanes >= dim too; how the terms spread over the lanes is the function's own
//                         business (for (j = lane; j < dim; j += 64)).  Pure: no barriers, no workspace, no writes.  A NaN or -inf
//                         share rejects.  MALA also needs tda_logprior_grad, d log p / d theta_j, called by the lane that owns parameter j.
//   -DTDA_FORWARD_WAVE    the source defines tda_forward_wave: the outputs are taken from LDS (s_out[m], dynamic; the MALA program
//                         lets the model write into its s_sens[m]) after one call, not from tda_forward(theta, dim, o) per output
//   -DTDA_GRADIENT_WAVE   (MALA program) the source defines the vector-Jacobian product in the same form, tda_gradient_wave, one call for all
//                         parameters.  grad: LDS, 128 doubles, zero before the call; `work` is what tda_forward_wave left at the same theta
// and three more select a third program, which runs after the sampling, over its records:
//   -DTDA_USER_REPLAY     the replay kernel (tda_user_replay) instead of the step kernels: outputs and quantities of interest of
//                         recorded parameters.  -DTDA_FORWARD_WAVE applies as above
//   -DTDA_QOI             (replay program) the source defines a quantity of interest per call, tda_qoi: quantity k of n_qoi from
//                         theta and the complete outputs f (both LDS); the lanes stride over k
//   -DTDA_QOI_WAVE        (replay program) the source defines all quantities in one call by the chain's 64 lanes, tda_qoi_wave
//                         (converged call site, __syncthreads() legal).  qoi: LDS, n_qoi doubles, NaN before the call (an entry
//                         left unwritten stays NaN: a NaN quantity is data, nothing is rejected here); `work` is what
//                         tda_forward_wave left at the same theta (null without TDA_WORKSPACE)
// and one selects the optimiser, a program of its own as well:
//   -DTDA_USER_MAP        the optimiser kernel (tda_user_maximize) instead of the kernels that sample: multi-start L-BFGS towards a
//                         maximum of log-prior + log-likelihood, or of the log-likelihood alone.  Together with -DTDA_USER_MALA the
//                         gradient is the MALA kernels' (the source's vector-Jacobian product and the gradients of its likelihood
//                         and prior, required as MALA requires them); alone it is a forward difference of the objective, d
//                         evaluations per gradient.  The form switches apply as above
// and one turns the MALA program into the HMC program:
//   -DTDA_USER_HMC        (in addition to -DTDA_USER_MALA) the HMC kernel (tda_user_hmc_steps) in place of tda_user_mala_steps:
//                         leapfrog trajectories on the log-posterior and gradient of the MALA program, whose requirements are its own;
//                         tda_user_mala_grad0 stays and initialises the gradient
// and one turns it into the NUTS program:
//   -DTDA_USER_NUTS       (in addition to -DTDA_USER_MALA) the NUTS kernel (tda_user_nuts_steps) in that place: trees of leapfrog steps
//                         that end at a U-turn, on the same log-posterior and gradient; tda_user_mala_grad0 stays as under HMC
// and one gives either of the two a dense inverse mass:
//   -DTDA_DENSE_MASS      (in addition to -DTDA_USER_HMC / -DTDA_USER_NUTS) the arithmetic of include/tinyda_amd_dense_mass.h: the kernel
//                         holds the whitened momentum q = L^T p of the inverse mass W = L L^T, `inv_mass` points at [2][DP][DP], L and
//                         behind it L^T, and the two products v = L q, r = L^T g go through tda_dense_product and s_vec
#include <hip/hip_runtime.h>
#include "tda_user_args.h"
__device__ double tda_forward(const double* theta, int dim, int o);

// TDA_FALLBACK: what a call resolves to when the source does not define a function of the contract's signature (a non-template
// function of that signature wins overload resolution against it).  TDA_REQUIRE, after the source: a call that still resolves to
// the fallback becomes a message that holds the tag <name>_missing and the signature, not an unresolved symbol at load.
#define TDA_FALLBACK(name, ...) \
  struct name##_missing {};     \
  template <class T>            \
  __device__ name##_missing name(__VA_ARGS__) { return {}; }
#define TDA_REQUIRE(name, message, ...) static_assert(!__is_same(decltype(name(__VA_ARGS__)), name##_missing), #name "_missing: " message)
#ifdef TDA_FORWARD_WAVE
TDA_FALLBACK(tda_forward_wave, const double*, int, double*, int, double*, T)
#endif
#if defined(TDA_USER_MALA) && defined(TDA_GRADIENT_WAVE)
TDA_FALLBACK(tda_gradient_wave, const double*, int, const double*, int, double*, double*, T)
#elif defined(TDA_USER_MALA)
TDA_FALLBACK(tda_gradient, const double*, int, const double*, int, T)
#endif
#ifdef TDA_LOGLIKE_SOURCE
TDA_FALLBACK(tda_loglike_term, double, double, double, T)
TDA_FALLBACK(tda_loglike_term_grad, double, double, double, T)
#endif
#if defined(TDA_LOGLIKE_SOURCE) && defined(TDA_LOGLIKE_WAVE)
TDA_FALLBACK(tda_loglike_wave, const double*, int, const double*, const double*, T)
TDA_FALLBACK(tda_loglike_grad_wave, const double*, int, const double*, const double*, double*, T)
#endif
#ifdef TDA_PRIOR_SOURCE
TDA_FALLBACK(tda_logprior_term, double, double, double, T)
TDA_FALLBACK(tda_logprior_term_grad, double, double, double, T)
#endif
#if defined(TDA_PRIOR_SOURCE) && defined(TDA_PRIOR_WAVE)
TDA_FALLBACK(tda_logprior_wave, const double*, int, const double*, const double*, T)
TDA_FALLBACK(tda_logprior_grad, const double*, int, const double*, const double*, T)
#endif
#if defined(TDA_USER_REPLAY) && defined(TDA_QOI_WAVE)
TDA_FALLBACK(tda_qoi_wave, const double*, int, const double*, int, double*, int, double*, T)
#elif defined(TDA_USER_REPLAY) && defined(TDA_QOI)
TDA_FALLBACK(tda_qoi, const double*, int, const double*, int, T)
#endif

#include "tda_user_source.h"

#define TDA_CD (const double*)nullptr
#define TDA_D (double*)nullptr
#ifdef TDA_FORWARD_WAVE
TDA_REQUIRE(tda_forward_wave, "the wave form of the model is " TDA_SIG_FORWARD_WAVE, TDA_CD, 0, TDA_D, 0, TDA_D, 0);
#endif
#if defined(TDA_USER_MALA) && defined(TDA_GRADIENT_WAVE)
TDA_REQUIRE(tda_gradient_wave, "the wave form of the gradient is " TDA_SIG_GRADIENT_WAVE, TDA_CD, 0, TDA_CD, 0, TDA_D, TDA_D, 0);
#elif defined(TDA_USER_MALA)
TDA_REQUIRE(tda_gradient, "MALA needs " TDA_SIG_GRADIENT, TDA_CD, 0, TDA_CD, 0, 0);
#endif
#if defined(TDA_LOGLIKE_SOURCE) && defined(TDA_LOGLIKE_WAVE)  // (the wave form stands in for the term and its derivative)
TDA_REQUIRE(tda_loglike_wave, "the wave form of the likelihood is " TDA_SIG_LOGLIKE_WAVE, TDA_CD, 0, TDA_CD, TDA_CD, 0);
#ifdef TDA_USER_MALA
TDA_REQUIRE(tda_loglike_grad_wave, "MALA under TDA_LOGLIKE_WAVE needs " TDA_SIG_LOGLIKE_GRAD_WAVE, TDA_CD, 0, TDA_CD, TDA_CD, TDA_D, 0);
#endif
#elif defined(TDA_LOGLIKE_SOURCE)
TDA_REQUIRE(tda_loglike_term, "a source-defined likelihood needs " TDA_SIG_LOGLIKE_TERM, 0.0, 0.0, 0.0, 0);
#ifdef TDA_USER_MALA
TDA_REQUIRE(tda_loglike_term_grad, "MALA needs " TDA_SIG_LOGLIKE_TERM_GRAD, 0.0, 0.0, 0.0, 0);
#endif
#endif
#if defined(TDA_PRIOR_SOURCE) && defined(TDA_PRIOR_WAVE)
TDA_REQUIRE(tda_logprior_wave, "the wave form of the prior is " TDA_SIG_LOGPRIOR_WAVE, TDA_CD, 0, TDA_CD, TDA_CD, 0);
#ifdef TDA_USER_MALA
TDA_REQUIRE(tda_logprior_grad, "MALA under TDA_PRIOR_WAVE needs " TDA_SIG_LOGPRIOR_GRAD, TDA_CD, 0, TDA_CD, TDA_CD, 0);
#endif
#endif
#ifdef TDA_PRIOR_SOURCE
#if !defined(TDA_PRIOR_WAVE)  // (the wave form stands in for the term and its derivative)
TDA_REQUIRE(tda_logprior_term, "a source-defined prior needs " TDA_SIG_LOGPRIOR_TERM, 0.0, 0.0, 0.0, 0);
#ifdef TDA_USER_MALA
TDA_REQUIRE(tda_logprior_term_grad, "MALA under TDA_PRIOR_SOURCE needs " TDA_SIG_LOGPRIOR_TERM_GRAD, 0.0, 0.0, 0.0, 0);
#endif
#endif
#endif
#if defined(TDA_USER_REPLAY) && defined(TDA_QOI_WAVE)
TDA_REQUIRE(tda_qoi_wave, "the wave form of the quantity of interest is " TDA_SIG_QOI_WAVE, TDA_CD, 0, TDA_CD, 0, TDA_D, 0, TDA_D, 0);
#elif defined(TDA_USER_REPLAY) && defined(TDA_QOI)
TDA_REQUIRE(tda_qoi, "a quantity of interest is " TDA_SIG_QOI, TDA_CD, 0, TDA_CD, 0, 0);
#endif

// The wave forms' LDS: the outputs s_out[m] (dynamic, sized by the host; a wave-form model writes them, and a likelihood that
// couples outputs reads them) and the model's workspace.  A program without the switches has neither: the names are null
// pointers that no code reads.
#if (defined(TDA_FORWARD_WAVE) || defined(TDA_GRADIENT_WAVE)) && defined(TDA_WORKSPACE) && TDA_WORKSPACE > 0
#define TDA_DECLARE_WORK __shared__ double s_work[TDA_WORKSPACE]
#else
#define TDA_DECLARE_WORK double* const s_work = nullptr
#endif
#if defined(TDA_FORWARD_WAVE) || (defined(TDA_LOGLIKE_SOURCE) && defined(TDA_LOGLIKE_WAVE))
#define TDA_DECLARE_OUT extern __shared__ double s_out[]
#else
#define TDA_DECLARE_OUT double* const s_out = nullptr
#endif
#ifdef TDA_FORWARD_WAVE
// every output of the model at the parameters in s_th, by one converged call of the wave; the barriers order the NaN fill, the
// model's writes (any lane may write any entry) and the readers.  The callers' own barriers keep earlier readers of `out` away.
__device__ __forceinline__ void tda_outputs_wave(const double* s_th, int lane, int d, int m, double* out, double* s_work) {
  for (int o = lane; o < m; o += 64) out[o] = __builtin_nan("");
  __syncthreads();
  tda_forward_wave(s_th, d, out, m, s_work, lane);
  __syncthreads();
}
#endif
#if defined(TDA_LOGLIKE_SOURCE) && defined(TDA_LOGLIKE_WAVE) && !defined(TDA_FORWARD_WAVE)
// the same for a per-output model under a likelihood that couples outputs: the lanes stride over the outputs and leave them in
// `out`, complete behind the barrier.  The callers' own barriers keep earlier readers of `out` away.
__device__ __forceinline__ void tda_outputs_fill(const double* s_th, int lane, int d, int m, double* out) {
  for (int o = lane; o < m; o += 64) out[o] = tda_forward(s_th, d, o);
  __syncthreads();
}
#endif

__device__ __forceinline__ double tda_wave_sum(double v) {
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
// the log-likelihood from the wave's sum over the outputs: of the terms themselves (source-defined), or of the weighted squares
// (posterior.py:95-108, distributions.py:295-326)
__device__ __forceinline__ double tda_loglike_of_sum(double sum, const double* w, double var) {
#ifdef TDA_LOGLIKE_SOURCE
  (void)w, (void)var;
  return sum;
#else
  return w ? -0.5 * sum : -0.5 * sum / var;
#endif
}

#ifdef TDA_USER_MAP
// log-prior of the point (x, x2) that stands in s_th, as tda_user_steps and tda_user_mala_steps evaluate lp_n (the same
// functions, the same summation: the same bits for the same state); the support bounds of uniform components as in tda_user_steps
__device__ __forceinline__ double tda_map_logprior(const UserMapArgs& a, const double* s_th, int lane, double x, double x2) {
  const int lane2 = lane + 64;
  const bool lj = lane < a.d, lj2 = lane2 < a.d;
#if defined(TDA_PRIOR_SOURCE) && defined(TDA_PRIOR_WAVE)
  (void)x, (void)x2, (void)lj, (void)lj2;
  return tda_wave_sum(tda_logprior_wave(s_th, a.d, a.pr_mean, a.pr_pinv, lane));
#else
  (void)s_th;
  const double pm = lj ? a.pr_mean[lane] : 0.0, pinv = lj ? a.pr_pinv[lane] : 0.0;
  const double pm2 = lj2 ? a.pr_mean[lane2] : 0.0, pinv2 = lj2 ? a.pr_pinv[lane2] : 0.0;
#ifdef TDA_PRIOR_SOURCE
  double pj = lj ? tda_logprior_term(x, pm, pinv, lane) : 0.0;
  if (lj2) pj += tda_logprior_term(x2, pm2, pinv2, lane2);
  return tda_wave_sum(pj);
#else
  const double dv = x - pm;
  double pj = lj ? dv * dv * pinv : 0.0;
  if (a.pr_lo && lj && (x < a.pr_lo[lane] || x > a.pr_hi[lane])) pj = __builtin_inf();
  if (lj2) {
    const double dv2 = x2 - pm2;
    pj += dv2 * dv2 * pinv2;
    if (a.pr_lo && (x2 < a.pr_lo[lane2] || x2 > a.pr_hi[lane2])) pj = __builtin_inf();
  }
  return -0.5 * (a.logconst + tda_wave_sum(pj));
#endif
#endif
}
#endif

#ifdef TDA_USER_REPLAY
// Outputs and quantities of interest of recorded parameters, after the run: the forward model is deterministic, so the records
// [R][N][d] hold everything that the reference's Link carries beside them (link.py:23-48: model_output, qoi).  One wave per
// chain c and segment of rows [r0, r1): the wave walks its rows in order and keeps the previous row in registers; a rejected
// step repeats its predecessor's parameters bit for bit, so a row whose integer image equals the previous row's (one wave vote;
// -0.0 differs from 0.0, a NaN equals itself) takes the outputs and quantities that already stand in LDS, and the model runs
// once per accepted state, not once per row.  The test is on the parameters, not on the accept flags: it holds under thinning and
// on every level of a hierarchy.  Dynamic LDS: the outputs s_out[m] and behind them the quantities s_qoi[nq].
#if (defined(TDA_FORWARD_WAVE) || defined(TDA_QOI_WAVE)) && defined(TDA_WORKSPACE) && TDA_WORKSPACE > 0
#define TDA_DECLARE_REPLAY_WORK __shared__ double s_work[TDA_WORKSPACE]
#else
#define TDA_DECLARE_REPLAY_WORK double* const s_work = nullptr
#endif
extern "C" __global__ void __launch_bounds__(64) tda_user_replay(const UserReplayArgs a) {
  extern __shared__ double s_out[];
  __shared__ double s_th[128];  // (65 .. 128 parameters: a lane holds parameters `lane` and `lane + 64`)
  TDA_DECLARE_REPLAY_WORK;
  const int lane = threadIdx.x, lane2 = lane + 64;
  const long long c = blockIdx.x % a.N, r0 = blockIdx.x / a.N * a.seg;
  const long long r1 = r0 + a.seg < a.R ? r0 + a.seg : a.R;
  const bool lj = lane < a.d, lj2 = lane2 < a.d;
  double* const s_qoi = s_out + a.m;
  long long prev = 0, prev2 = 0;
  long long neval = 0;
  for (long long r = r0; r < r1; ++r) {
    const size_t row = (size_t)r * a.N + c;
    const double th = lj ? a.params[row * a.d + lane] : 0.0, th2 = lj2 ? a.params[row * a.d + lane2] : 0.0;
    const long long bits = __double_as_longlong(th), bits2 = __double_as_longlong(th2);
    if (r == r0 || __any(bits != prev || bits2 != prev2)) {
      __syncthreads();  // (the previous row's stores have read s_out / s_qoi)
      s_th[lane] = th;
      s_th[lane2] = th2;
      __syncthreads();
#ifdef TDA_FORWARD_WAVE
      tda_outputs_wave(s_th, lane, a.d, a.m, s_out, s_work);
#else
      for (int o = lane; o < a.m; o += 64) s_out[o] = tda_forward(s_th, a.d, o);  // (the order in which tda_user_eval strides)
      __syncthreads();
#endif
#ifdef TDA_QOI_WAVE
      // all quantities by one converged call of the wave; a NaN is data here, an entry left unwritten stays NaN
      for (int k = lane; k < a.nq; k += 64) s_qoi[k] = __builtin_nan("");
      __syncthreads();
      tda_qoi_wave(s_th, a.d, s_out, a.m, s_qoi, a.nq, s_work, lane);
      __syncthreads();
#elif defined(TDA_QOI)
      for (int k = lane; k < a.nq; k += 64) s_qoi[k] = tda_qoi(s_th, a.d, s_out, a.m, k);
      __syncthreads();
#endif
      ++neval;
    }
    prev = bits;
    prev2 = bits2;
    if (a.outputs)
      for (int o = lane; o < a.m; o += 64) a.outputs[row * a.m + o] = s_out[o];
#if defined(TDA_QOI_WAVE) || defined(TDA_QOI)
    if (a.qoi)
      for (int k = lane; k < a.nq; k += 64) a.qoi[row * a.nq + k] = s_qoi[k];
#endif
  }
  if (lane == 0 && a.n_eval) atomicAdd((unsigned long long*)a.n_eval, (unsigned long long)neval);
}

#elif !defined(TDA_USER_MALA)
// log-likelihood of the model outputs at the parameters in s_th, for the whole wave (link.py:48 takes any loglike).  The level's
// fields come in one by one: with the argument struct passed whole the kernels no longer compile to the instructions they had.
#ifdef TDA_FORWARD_WAVE
#define TDA_OUTPUT(o) s_out[o]
#else
#define TDA_OUTPUT(o) tda_forward(s_th, d, o)
#endif
__device__ __forceinline__ double tda_loglike(const double* s_th, int lane, int d, int m, const double* data, const double* w, double var, double* s_out,
                                              double* s_work) {
  double sum = 0.0;
#ifdef TDA_FORWARD_WAVE
  tda_outputs_wave(s_th, lane, d, m, s_out, s_work);
#elif defined(TDA_LOGLIKE_SOURCE) && defined(TDA_LOGLIKE_WAVE)
  (void)s_work;
  tda_outputs_fill(s_th, lane, d, m, s_out);
#else
  (void)s_out, (void)s_work;
#endif
#if defined(TDA_LOGLIKE_SOURCE) && defined(TDA_LOGLIKE_WAVE)
  // a likelihood that couples outputs: one converged call by the whole wave over the complete outputs, the lanes' shares summed
  // below; a NaN or -inf share makes the sum NaN or -inf and rejects
  sum = tda_loglike_wave(s_out, m, data, w, lane);
#elif defined(TDA_LOGLIKE_SOURCE)
  for (int o = lane; o < m; o += 64) sum += tda_loglike_term(TDA_OUTPUT(o), data[o], w[o], o);
#else
  for (int o = lane; o < m; o += 64) {
    const double r = TDA_OUTPUT(o) - data[o];
    double sq = r * r;
    if (w) sq *= w[o];
    sum += sq;
  }
#endif
  return tda_loglike_of_sum(tda_wave_sum(sum), w, var);
}
#ifdef TDA_USER_MAP
// the optimiser without a gradient in the source (tda_user_maximize below, in place of the three step kernels): the
// log-likelihood is tda_loglike, the gradient a difference of objective values
__device__ __forceinline__ double tda_map_loglike(const UserMapArgs& a, const double* s_th, double* s_out, double* s_work, int lane) {
  return tda_loglike(s_th, lane, a.d, a.m, a.data, a.w, a.var, s_out, s_work);
}
#else
extern "C" __global__ void __launch_bounds__(64) tda_user_steps(const UserStepArgs a) {
  __shared__ double s_th[128];  // (65 .. 128 parameters: a lane holds parameters `lane` and `lane + 64`)
  TDA_DECLARE_OUT;
  TDA_DECLARE_WORK;
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
    const double ll_n = tda_loglike(s_th, lane, a.d, a.m, a.data, a.w, a.var, s_out, s_work);
#if defined(TDA_PRIOR_SOURCE) && defined(TDA_PRIOR_WAVE)
    // a prior that couples parameters: one call by the whole wave over the proposal in s_th (nothing writes s_th before the next
    // step's barrier), the lanes' shares summed; a NaN or -inf share makes the sum NaN or -inf and rejects
    const double lp_n = tda_wave_sum(tda_logprior_wave(s_th, a.d, a.pr_mean, a.pr_pinv, lane));
#else
#ifdef TDA_PRIOR_SOURCE
    // source-defined prior: the sum of the components' terms (pm / pinv hold p / q); a component outside its support is -inf
    double pj = lj ? tda_logprior_term(prp, pm, pinv, lane) : 0.0;
    if (lj2) pj += tda_logprior_term(prp2, pm2, pinv2, lane2);
    const double lp_n = tda_wave_sum(pj);  // distributions.py:44-56 (JointPrior.logpdf)
#else
    const double dv = prp - pm;
    double pj = lj ? dv * dv * pinv : 0.0;
    if (a.pr_lo && lj && (prp < a.pr_lo[lane] || prp > a.pr_hi[lane])) pj = __builtin_inf();  // uniform prior components
    if (lj2) {
      const double dv2 = prp2 - pm2;
      pj += dv2 * dv2 * pinv2;
      if (a.pr_lo && (prp2 < a.pr_lo[lane2] || prp2 > a.pr_hi[lane2])) pj = __builtin_inf();
    }
    const double maha = tda_wave_sum(pj);
    const double lp_n = -0.5 * (a.logconst + maha);  // scipy MVN logpdf, posterior.py:92
#endif
#endif
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
// one step of level q >= 1 of a hierarchy (chain.py:353-402, :711-737; proposal.py:1515-1545), one wave per chain: the
// same decision, alignment and records as the engine's k_ext_level_action, with the model evaluated in place
extern "C" __global__ void __launch_bounds__(64) tda_user_level_action(const UserLevelArgs a) {
  __shared__ double s_th[128];  // (65 .. 128 parameters: a second parameter per lane)
  TDA_DECLARE_OUT;
  TDA_DECLARE_WORK;
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
  const double lln = tda_loglike(s_th, lane, a.d, a.m, a.data, a.w, a.var, s_out, s_work);
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
#ifdef TDA_FORWARD_WAVE
  TDA_DECLARE_OUT;
  TDA_DECLARE_WORK;
  tda_outputs_wave(s_th, lane, d, m, s_out, s_work);
#endif
  for (int o = lane; o < m; o += 64) F[c * m + o] = TDA_OUTPUT(o);
}
#endif  // TDA_USER_MAP

#else  // TDA_USER_MALA
// outputs of the model at the parameters in s_th: returns this lane's share of the sum that tda_loglike_of_sum finishes (the
// weighted squares, or the terms of a source-defined likelihood) and leaves the sensitivity in s_sens: grad_loglike =
// Sigma^-1 (y - F) (distributions.py:300-301 iso: 1 / var * r, :314-315 diag: w * r), or d term / d f
// (wave form: the model writes its outputs into s_sens, each lane then turns its own entries into sensitivities in place)
// gradient of the log-prior in parameter j: the source's own under TDA_PRIOR_SOURCE (pm / pinv hold p / q), else the diagonal
// Gaussian's (utils.py:273-280)
#if defined(TDA_PRIOR_SOURCE) && defined(TDA_PRIOR_WAVE)
// (the coupled form reads the whole state: s_th holds the proposal in tda_user_mala_steps, the current state in tda_user_mala_grad0)
#define TDA_PRIOR_GRAD(x, pm, pinv, j) tda_logprior_grad(s_th, a.d, a.pr_mean, a.pr_pinv, j)
#elif defined(TDA_PRIOR_SOURCE)
#define TDA_PRIOR_GRAD(x, pm, pinv, j) tda_logprior_term_grad(x, pm, pinv, j)
#else
#define TDA_PRIOR_GRAD(x, pm, pinv, j) ((pinv) * ((pm) - (x)))
#endif
#ifdef TDA_FORWARD_WAVE
#define TDA_MALA_OUTPUT(o) s_sens[o]
#else
#define TDA_MALA_OUTPUT(o) tda_forward(s_th, a.d, o)
#endif
#if defined(TDA_LOGLIKE_SOURCE) && defined(TDA_LOGLIKE_WAVE)
// a likelihood that couples outputs: its gradient reads its neighbours, so the outputs are not turned into sensitivities in place.
// The dynamic LDS is 2 m doubles, s_sens[m] and behind it the outputs s_f[m]; the model writes s_f, tda_loglike_wave gives this
// lane's share of the sum, and tda_loglike_grad_wave writes s_sens (NaN before the call: the callers' barrier completes it).
// `work` still holds what tda_forward_wave left, for tda_gradient_wave.
__device__ __forceinline__ double tda_mala_outputs(const UserMalaArgs& a, const double* s_th, double* s_sens, double* s_work, int lane) {
  double* const s_f = s_sens + a.m;
#ifdef TDA_FORWARD_WAVE
  tda_outputs_wave(s_th, lane, a.d, a.m, s_f, s_work);
#else
  (void)s_work;
  tda_outputs_fill(s_th, lane, a.d, a.m, s_f);
#endif
  const double sum = tda_loglike_wave(s_f, a.m, a.data, a.w, lane);
  for (int o = lane; o < a.m; o += 64) s_sens[o] = __builtin_nan("");
  __syncthreads();
  tda_loglike_grad_wave(s_f, a.m, a.data, a.w, s_sens, lane);
  return sum;
}
#else
__device__ __forceinline__ double tda_mala_outputs(const UserMalaArgs& a, const double* s_th, double* s_sens, double* s_work, int lane) {
  double sum = 0.0;
#ifdef TDA_FORWARD_WAVE
  tda_outputs_wave(s_th, lane, a.d, a.m, s_sens, s_work);
#else
  (void)s_work;
#endif
#ifdef TDA_LOGLIKE_SOURCE
  for (int o = lane; o < a.m; o += 64) {
    const double f = TDA_MALA_OUTPUT(o);
    sum += tda_loglike_term(f, a.data[o], a.w[o], o);
    s_sens[o] = tda_loglike_term_grad(f, a.data[o], a.w[o], o);
  }
#else
  const double iv = 1.0 / a.var;
  for (int o = lane; o < a.m; o += 64) {
    const double f = TDA_MALA_OUTPUT(o);
    const double r = f - a.data[o];
    double sq = r * r;
    if (a.w) sq *= a.w[o];
    sum += sq;
    s_sens[o] = (a.w ? a.w[o] : iv) * (a.data[o] - f);
  }
#endif
  return sum;
}
#endif
#ifdef TDA_USER_MAP
// the optimiser over the source's own gradient (tda_user_maximize below, in place of the two MALA kernels): the log-likelihood
// as tda_user_mala_steps has its ll_n, which leaves the sensitivities in s_sens, and the gradient as it has its gp
__device__ __forceinline__ double tda_map_loglike(const UserMapArgs& a, const double* s_th, double* s_sens, double* s_work, int lane) {
  UserMalaArgs ma{};
  ma.d = a.d, ma.m = a.m, ma.data = a.data, ma.w = a.w, ma.var = a.var;
  return tda_loglike_of_sum(tda_wave_sum(tda_mala_outputs(ma, s_th, s_sens, s_work, lane)), a.w, a.var);
}
// gradient of the objective at the point (x, x2) whose evaluation was the last one: s_th, s_sens and the workspace still hold it
__device__ __forceinline__ void tda_map_gradient(const UserMapArgs& a, const double* s_th, double* s_sens, double* s_grad, double* s_work, int lane, double x,
                                                 double x2, double& g, double& g2) {
  const int lane2 = lane + 64;
  const bool lj = lane < a.d, lj2 = lane2 < a.d, prior = a.objective == 0;
  const double pm = lj ? a.pr_mean[lane] : 0.0, pinv = lj ? a.pr_pinv[lane] : 0.0;
  const double pm2 = lj2 ? a.pr_mean[lane2] : 0.0, pinv2 = lj2 ? a.pr_pinv[lane2] : 0.0;
  (void)pm, (void)pinv, (void)pm2, (void)pinv2, (void)x, (void)x2;
#ifdef TDA_GRADIENT_WAVE
  s_grad[lane] = 0.0;
  s_grad[lane2] = 0.0;
  __syncthreads();  // s_sens complete
  tda_gradient_wave(s_th, a.d, s_sens, a.m, s_grad, s_work, lane);
  __syncthreads();
  g = lj ? (prior ? TDA_PRIOR_GRAD(x, pm, pinv, lane) : 0.0) + s_grad[lane] : 0.0;
  g2 = lj2 ? (prior ? TDA_PRIOR_GRAD(x2, pm2, pinv2, lane2) : 0.0) + s_grad[lane2] : 0.0;
#else
  (void)s_grad, (void)s_work;
  __syncthreads();  // s_sens complete
  g = lj ? (prior ? TDA_PRIOR_GRAD(x, pm, pinv, lane) : 0.0) + tda_gradient(s_th, a.d, s_sens, a.m, lane) : 0.0;
  g2 = lj2 ? (prior ? TDA_PRIOR_GRAD(x2, pm2, pinv2, lane2) : 0.0) + tda_gradient(s_th, a.d, s_sens, a.m, lane2) : 0.0;
#endif
}
#else
#ifdef TDA_DENSE_MASS
// y_i = sum_j M[j][i] x_j for the parameters i = lane, lane + 64 (include/tinyda_amd_dense_mass.h, "The two products"): M is
// [DP][DP] row-major, zero outside the triangle and in the padding, so M = L gives r = L^T g and M = L^T gives v = L q.  The sum
// runs over j = 0, 1, .., d - 1 in that order from 0.0, one fused multiply-add per term: the terms outside the triangle add exact
// zeros.  Lane i reads M[j][i]: consecutive lanes on consecutive addresses, one row of 8 DP bytes per j, the same row for every
// chain on the device; the operand x_j is broadcast from s_vec.  A lane without a parameter gets 0 (whatever x holds: 0 * NaN
// is not 0).  Barriers: the first puts the readers of s_vec of the product before behind it, the second the stores before the
// reads; called from the converged wave only.
__device__ __forceinline__ void tda_dense_product(const double* __restrict__ M, int d, int DP, double* s_vec, int lane, double x, double x2, double& y, double& y2) {
  __syncthreads();
  s_vec[lane] = x;
  s_vec[lane + 64] = x2;
  __syncthreads();
  double acc = 0.0, acc2 = 0.0;
  if (DP > 64) {  // (DP = 128: both slots of a lane lie inside a row)
#pragma unroll 4
    for (int j = 0; j < d; ++j) {
      const double xj = s_vec[j];
      acc = fma(M[(size_t)j * DP + lane], xj, acc);
      acc2 = fma(M[(size_t)j * DP + lane + 64], xj, acc2);
    }
  } else if (lane < DP) {
#pragma unroll 4
    for (int j = 0; j < d; ++j) acc = fma(M[(size_t)j * DP + lane], s_vec[j], acc);
  }
  y = lane < d ? acc : 0.0;
  y2 = lane + 64 < d ? acc2 : 0.0;
}
#endif
#if defined(TDA_USER_NUTS)
// The no-U-turn sampler in place of tda_user_mala_steps (the algorithm, step by step: include/tinyda_amd_nuts.h): multinomial NUTS
// in iterative form, one wave per chain.  Both edges of the tree, its candidate, the new subtree's candidate, the moving leaf and
// the two momentum sums stay in registers, two doubles per lane each; the log-posterior and its gradient are MALA's (the same
// calls in the same order: tda_mala_outputs, the prior's three forms, tda_gradient / tda_gradient_wave), a leaf is one of HMC's
// leapfrog steps.  The U-turn checkpoints of a subtree (momentum and running momentum sum at its even leaves) live in LDS behind
// s_sens, because their index is a run-time value; every lane reads back only what it stored itself, so they need no barrier.
// The kernel reads no variates but z: direction, merge and selection draws are Philox stream 8, computed here.
// Every tree decision (finite log-posterior, divergence, selection, U-turn, merge) compares wave sums or Philox words, the same
// bits in all 64 lanes, and goes through a scalar register: the wave leaves a loop as one, so every source function that may hold
// a barrier or a shuffle is called from a converged wave.
// Barriers: the one at the top of a leaf puts the readers of s_th / s_sens / s_grad of the leaf before it (of this subtree, of an
// earlier one or of the previous step, whichever way they were left) behind it before the next position is stored.
__device__ __forceinline__ void tda_nuts_philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned& x, unsigned& y, unsigned& z) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    c1 = (unsigned)p1;
    c3 = (unsigned)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  x = c0, y = c1, z = c2;
}
__device__ __forceinline__ double tda_nuts_u53(unsigned a, unsigned b) { return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) * (1.0 / 9007199254740992.0); }
__device__ __forceinline__ double tda_nuts_logaddexp(double a, double b) {
  const double hi = a > b ? a : b, lo = a > b ? b : a;
  return hi + log1p(exp(lo - hi));
}
extern "C" __global__ void __launch_bounds__(64) tda_user_nuts_steps(const UserNutsArgs a) {
  extern __shared__ double s_sens[];  // [m] ([2 m] under TDA_LOGLIKE_WAVE), and at ck_off the checkpoints [max_depth][2][DP]
  __shared__ double s_th[128];
  TDA_DECLARE_WORK;
#ifdef TDA_GRADIENT_WAVE
  __shared__ double s_grad[128];
#endif
#ifdef TDA_DENSE_MASS
  __shared__ double s_vec[128];  // the broadcast operand of tda_dense_product
#endif
  const int lane = threadIdx.x, lane2 = lane + 64;
  const long long c = blockIdx.x;
  if (c >= a.N) return;
  const bool lj = lane < a.d, lj2 = lane2 < a.d;
  const size_t row = (size_t)c * a.DP;
  double* const s_ck = s_sens + a.ck_off;
  double cur = lj ? a.theta[row + lane] : 0.0, cur2 = lj2 ? a.theta[row + lane2] : 0.0;
  double gc = lj ? a.grad[row + lane] : 0.0, gc2 = lj2 ? a.grad[row + lane2] : 0.0;
  double lp = a.lp[c], ll = a.ll[c];
  const double eps = a.scaling[c];
#ifdef TDA_DENSE_MASS
  // p, pl, pr, rho, rs and the checkpoints below hold the whitened momentum q = L^T p and its sums
  const double* const chol = a.inv_mass;
  const double* const cholT = a.inv_mass + (size_t)a.DP * a.DP;
#else
  const double w = lj ? a.inv_mass[lane] : 1.0, w2 = lj2 ? a.inv_mass[lane2] : 1.0;
  const double sw = sqrt(w), sw2 = sqrt(w2);
#endif
  const double pm = lj ? a.pr_mean[lane] : 0.0, pinv = lj ? a.pr_pinv[lane] : 0.0;
  const double pm2 = lj2 ? a.pr_mean[lane2] : 0.0, pinv2 = lj2 ? a.pr_pinv[lane2] : 0.0;
  (void)pm, (void)pinv, (void)pm2, (void)pinv2;
  const unsigned k0 = (unsigned)a.seed, k1 = (unsigned)(a.seed >> 32), gchain = (unsigned)(a.chain_offset + c);
  double accsum = a.accsum[c];
  long long n_leap = 0, n_div = 0, n_cap = 0, n_depth = 0;
  int nacc = 0;
  for (int s = 0; s < a.S; ++s) {
    const double* z = a.inc + ((size_t)s * a.NP + c) * a.DP;
    const unsigned gstep = (unsigned)(a.step0 + s);
#ifdef TDA_DENSE_MASS
    const double p0 = lj ? z[lane] : 0.0, p02 = lj2 ? z[lane2] : 0.0;  // q = z: the momentum L^-T z ~ N(0, W^-1)
    const double h0 = -(lp + ll) + 0.5 * tda_wave_sum(p0 * p0 + p02 * p02);
#else
    const double p0 = lj ? z[lane] / sw : 0.0, p02 = lj2 ? z[lane2] / sw2 : 0.0;  // momentum ~ N(0, 1 / w)
    const double h0 = -(lp + ll) + 0.5 * tda_wave_sum(w * (p0 * p0) + w2 * (p02 * p02));
#endif
    // the tree: its edges (l: backward, r: forward), the sum of its momenta, its log-weight, its candidate
    double lth = cur, lth2 = cur2, pl = p0, pl2 = p02, lg = gc, lg2 = gc2;
    double rth = cur, rth2 = cur2, pr = p0, pr2 = p02, rg = gc, rg2 = gc2;
    double rho = p0, rho2 = p02, LW = 0.0;
    double cth = cur, cth2 = cur2, cg = gc, cg2 = gc2, clp = lp, cll = ll;
    double asum = 0.0;
    int moved = 0, nleaf = 0, depth = 0, stop = 0;  // stop: 1 a divergent leaf, 2 a U-turn inside the new subtree, 3 a U-turn of the whole tree
    for (int j = 0; j < a.max_depth; ++j) {
      unsigned x0, x1, x2;
      tda_nuts_philox((unsigned)j, gstep, gchain, 8u, k0, k1, x0, x1, x2);
      const int fwd = __builtin_amdgcn_readfirstlane((int)(x2 & 1u));
      const double uj = tda_nuts_u53(x0, x1);
      const double e = fwd ? eps : -eps, he = 0.5 * e;
      double th = fwd ? rth : lth, th2 = fwd ? rth2 : lth2, p = fwd ? pr : pl, p2 = fwd ? pr2 : pl2, g = fwd ? rg : lg, g2 = fwd ? rg2 : lg2;
      // the new subtree: its candidate, its log-weight, the sum of its momenta
      double sth = 0.0, sth2 = 0.0, sg = 0.0, sg2 = 0.0, slp = 0.0, sll = 0.0, LWs = 0.0, rs = 0.0, rs2 = 0.0;
      const int nl = 1 << j;
#ifdef TDA_DENSE_MASS
      double r, r2;  // r = L^T g at the moving leaf: of the edge here, of each new leaf below
      tda_dense_product(chol, a.d, a.DP, s_vec, lane, g, g2, r, r2);
#endif
      for (int n = 0; n < nl; ++n) {
#ifdef TDA_DENSE_MASS
        p += he * r;
        p2 += he * r2;
        double v, v2;
        tda_dense_product(cholT, a.d, a.DP, s_vec, lane, p, p2, v, v2);  // v = L q
        th += e * v;  // (a lane without a parameter keeps q = v = r = 0 and th = 0)
        th2 += e * v2;
#else
        p += he * g;
        p2 += he * g2;
        th += e * (w * p);  // (a lane without a parameter keeps p = 0 and th = 0)
        th2 += e * (w2 * p2);
#endif
        __syncthreads();
        s_th[lane] = th;
        s_th[lane2] = th2;
        __syncthreads();
        const double sum = tda_wave_sum(tda_mala_outputs(a, s_th, s_sens, s_work, lane));
        const double ll_n = tda_loglike_of_sum(sum, a.w, a.var);
        double lp_n;
#if defined(TDA_PRIOR_SOURCE) && defined(TDA_PRIOR_WAVE)
        lp_n = tda_wave_sum(tda_logprior_wave(s_th, a.d, a.pr_mean, a.pr_pinv, lane));
#elif defined(TDA_PRIOR_SOURCE)
        double pj = lj ? tda_logprior_term(th, pm, pinv, lane) : 0.0;
        if (lj2) pj += tda_logprior_term(th2, pm2, pinv2, lane2);
        lp_n = tda_wave_sum(pj);
#else
        double pj = 0.0;
        if (lj) {
          const double dv = th - pm;
          pj = dv * dv * pinv;
        }
        if (lj2) {
          const double dv2 = th2 - pm2;
          pj += dv2 * dv2 * pinv2;
        }
        lp_n = -0.5 * (a.logconst + tda_wave_sum(pj));
#endif
        const double post_n = lp_n + ll_n;
        nleaf += 1;
        if (!__builtin_amdgcn_readfirstlane(__builtin_isfinite(post_n) ? 1 : 0)) {
          stop = 1;
          break;
        }
#ifdef TDA_GRADIENT_WAVE
        s_grad[lane] = 0.0;  // (its readers of the previous leaf are behind the barriers above)
        s_grad[lane2] = 0.0;
#endif
        __syncthreads();  // s_sens complete
#ifdef TDA_GRADIENT_WAVE
        tda_gradient_wave(s_th, a.d, s_sens, a.m, s_grad, s_work, lane);
        __syncthreads();
        g = lj ? TDA_PRIOR_GRAD(th, pm, pinv, lane) + s_grad[lane] : 0.0;
        g2 = lj2 ? TDA_PRIOR_GRAD(th2, pm2, pinv2, lane2) + s_grad[lane2] : 0.0;
#else
        g = lj ? TDA_PRIOR_GRAD(th, pm, pinv, lane) + tda_gradient(s_th, a.d, s_sens, a.m, lane) : 0.0;
        g2 = lj2 ? TDA_PRIOR_GRAD(th2, pm2, pinv2, lane2) + tda_gradient(s_th, a.d, s_sens, a.m, lane2) : 0.0;
#endif
#ifdef TDA_DENSE_MASS
        tda_dense_product(chol, a.d, a.DP, s_vec, lane, g, g2, r, r2);
        p += he * r;
        p2 += he * r2;
        const double h = -post_n + 0.5 * tda_wave_sum(p * p + p2 * p2);
#else
        p += he * g;
        p2 += he * g2;
        // (a gradient that is not finite leaves a NaN momentum: the energy is NaN and the leaf divergent)
        const double h = -post_n + 0.5 * tda_wave_sum(w * (p * p) + w2 * (p2 * p2));
#endif
        if (__builtin_amdgcn_readfirstlane((h != h || h - h0 > 1000.0) ? 1 : 0)) {
          stop = 1;
          break;
        }
        const double lw = h0 - h, ew = exp(lw);
        asum += ew < 1.0 ? ew : 1.0;
        int take = 1;
        if (n == 0) {
          LWs = lw;
          rs = p;
          rs2 = p2;
        } else {
          LWs = tda_nuts_logaddexp(LWs, lw);
          rs += p;
          rs2 += p2;
          tda_nuts_philox(32u + (unsigned)nleaf, gstep, gchain, 8u, k0, k1, x0, x1, x2);
          take = __builtin_amdgcn_readfirstlane(tda_nuts_u53(x0, x1) < exp(lw - LWs) ? 1 : 0);
        }
        if (take) {
          sth = th, sth2 = th2, sg = g, sg2 = g2, slp = lp_n, sll = ll_n;
        }
        // U-turns inside the subtree: leaf n closes the aligned sub-subtrees of 2^k leaves for k = 1 .. (trailing ones of n);
        // the one of 2^k leaves began at the even leaf whose checkpoint is row popcount(n >> 1) - k + 1
        const int top = __builtin_popcount((unsigned)n >> 1);
        if (!(n & 1)) {
          double* const ck = s_ck + (size_t)top * 2 * a.DP;
          if (lj) ck[lane] = p, ck[a.DP + lane] = rs;
          if (lj2) ck[lane2] = p2, ck[a.DP + lane2] = rs2;
        } else {
          const int low = top - __builtin_ctz(~(unsigned)n) + 1;
          int turn = 0;
          for (int k = top; k >= low; --k) {
            const double* const ck = s_ck + (size_t)k * 2 * a.DP;
            const double pa = lj ? ck[lane] : 0.0, pa2 = lj2 ? ck[lane2] : 0.0;
            const double rr = lj ? (rs - ck[a.DP + lane]) + pa : 0.0, rr2 = lj2 ? (rs2 - ck[a.DP + lane2]) + pa2 : 0.0;
#ifdef TDA_DENSE_MASS
            const double da = tda_wave_sum(pa * rr + pa2 * rr2), db = tda_wave_sum(p * rr + p2 * rr2);  // p_a^T W rho_p = q_a . rho_q
#else
            const double da = tda_wave_sum((w * pa) * rr + (w2 * pa2) * rr2), db = tda_wave_sum((w * p) * rr + (w2 * p2) * rr2);
#endif
            turn |= (da > 0.0 && db > 0.0) ? 0 : 1;
          }
          if (__builtin_amdgcn_readfirstlane(turn)) {
            stop = 2;
            break;
          }
        }
      }
      if (stop) break;
      // merge: the biased progressive rule on the candidates, the weights and the momentum sums, the extended edge
      if (__builtin_amdgcn_readfirstlane(uj < exp(LWs - LW) ? 1 : 0)) {
        cth = sth, cth2 = sth2, cg = sg, cg2 = sg2, clp = slp, cll = sll;
        moved = 1;
      }
      LW = tda_nuts_logaddexp(LW, LWs);
      rho += rs;
      rho2 += rs2;
      if (fwd) {
        rth = th, rth2 = th2, pr = p, pr2 = p2, rg = g, rg2 = g2;
      } else {
        lth = th, lth2 = th2, pl = p, pl2 = p2, lg = g, lg2 = g2;
      }
      depth = j + 1;
#ifdef TDA_DENSE_MASS
      const double da = tda_wave_sum(pl * rho + pl2 * rho2), db = tda_wave_sum(pr * rho + pr2 * rho2);
#else
      const double da = tda_wave_sum((w * pl) * rho + (w2 * pl2) * rho2), db = tda_wave_sum((w * pr) * rho + (w2 * pr2) * rho2);
#endif
      if (__builtin_amdgcn_readfirstlane((da > 0.0 && db > 0.0) ? 0 : 1)) {
        stop = 3;
        break;
      }
    }
    cur = cth, cur2 = cth2, gc = cg, gc2 = cg2, lp = clp, ll = cll;
    nacc += moved;
    accsum += asum / (double)nleaf;
    n_leap += nleaf;
    n_div += stop == 1 ? 1 : 0;
    n_cap += stop == 0 ? 1 : 0;
    n_depth += depth;
    const size_t r = (size_t)s * a.N + c;
    if (lane == 0) {
      if (a.rec_stats) {
        a.rec_stats[r * 3 + 0] = lp;
        a.rec_stats[r * 3 + 1] = ll;
        a.rec_stats[r * 3 + 2] = lp + ll;
      }
      if (a.rec_acc) a.rec_acc[r] = (unsigned char)moved;
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
    if (a.scaling_out) {  // the engine's rule of the period boundary on the mean acceptance statistic
      a.scaling_out[c] = exp(log(eps) + a.gamma_pow * (accsum / (double)a.period - a.alpha_star));
      accsum = 0.0;
    }
    a.accsum[c] = accsum;
    long long* const tot = a.totals + (size_t)c * TDA_NUTS_TOTALS;
    tot[0] += n_leap;
    tot[1] += n_div;
    tot[2] += n_cap;
    tot[3] += n_depth;
  }
}
#elif defined(TDA_USER_HMC)
// Hamiltonian Monte Carlo in place of tda_user_mala_steps: per step one momentum from the step's unit normals, n_leapfrog
// leapfrog steps of size scaling[c] under the diagonal inverse mass w on the log-posterior and gradient that MALA evaluates
// (the same calls in the same order: tda_mala_outputs, the prior's three forms, tda_gradient / tda_gradient_wave), one accept
// test on the energy difference at the end.  The state, the momentum and the gradient stay in registers; s_th holds the moving
// position.  The interior leapfrog steps read no variates and write no records.
// A position whose log-posterior is not finite (outside a support, a NaN output) ends the trajectory and rejects.  That test
// is on wave sums, the same bits in all 64 lanes, and goes through a scalar register: the wave leaves the loop as one, so every
// source function that may hold a barrier or a shuffle is called from a converged wave.
// Barriers: the one at the top of a leapfrog step puts the readers of s_th / s_sens / s_grad of the step before it (and of the
// previous trajectory, whichever way it left the loop) behind it before the next position is stored.
extern "C" __global__ void __launch_bounds__(64) tda_user_hmc_steps(const UserHmcArgs a) {
  extern __shared__ double s_sens[];  // [m] ([2 m] under TDA_LOGLIKE_WAVE: the outputs behind the sensitivities)
  __shared__ double s_th[128];
  TDA_DECLARE_WORK;
#ifdef TDA_GRADIENT_WAVE
  __shared__ double s_grad[128];  // J^T sens at the moving position, all parameters from one tda_gradient_wave call
#endif
#ifdef TDA_DENSE_MASS
  __shared__ double s_vec[128];  // the broadcast operand of tda_dense_product
#endif
  const int lane = threadIdx.x, lane2 = lane + 64;
  const long long c = blockIdx.x;
  if (c >= a.N) return;
  const bool lj = lane < a.d, lj2 = lane2 < a.d;
  const size_t row = (size_t)c * a.DP;
  double cur = lj ? a.theta[row + lane] : 0.0, cur2 = lj2 ? a.theta[row + lane2] : 0.0;
  double gc = lj ? a.grad[row + lane] : 0.0, gc2 = lj2 ? a.grad[row + lane2] : 0.0;  // gradient at the current state
  double lp = a.lp[c], ll = a.ll[c];
  const double eps = a.scaling[c], he = 0.5 * eps;
#ifdef TDA_DENSE_MASS
  // p below holds the whitened momentum q = L^T p of include/tinyda_amd_dense_mass.h
  const double* const chol = a.inv_mass;
  const double* const cholT = a.inv_mass + (size_t)a.DP * a.DP;
#else
  const double w = lj ? a.inv_mass[lane] : 1.0, w2 = lj2 ? a.inv_mass[lane2] : 1.0;
  const double sw = sqrt(w), sw2 = sqrt(w2);
#endif
  const double pm = lj ? a.pr_mean[lane] : 0.0, pinv = lj ? a.pr_pinv[lane] : 0.0;
  const double pm2 = lj2 ? a.pr_mean[lane2] : 0.0, pinv2 = lj2 ? a.pr_pinv[lane2] : 0.0;
  (void)pm, (void)pinv, (void)pm2, (void)pinv2;
  int nacc = 0;
  for (int s = 0; s < a.S; ++s) {
    const double* z = a.inc + ((size_t)s * a.NP + c) * a.DP;
#ifdef TDA_DENSE_MASS
    double p = lj ? z[lane] : 0.0, p2 = lj2 ? z[lane2] : 0.0;  // q = z: the momentum L^-T z ~ N(0, W^-1)
    const double k0 = 0.5 * tda_wave_sum(p * p + p2 * p2);
    double fr, fr2, v, v2;  // fr: the r = L^T g of include/tinyda_amd_dense_mass.h
    tda_dense_product(chol, a.d, a.DP, s_vec, lane, gc, gc2, fr, fr2);
    p += he * fr;
    p2 += he * fr2;
#else
    double p = lj ? z[lane] / sw : 0.0, p2 = lj2 ? z[lane2] / sw2 : 0.0;  // momentum ~ N(0, 1 / w)
    const double k0 = 0.5 * tda_wave_sum(w * (p * p) + w2 * (p2 * p2));
    p += he * gc;
    p2 += he * gc2;
#endif
    double th = cur, th2 = cur2, g = gc, g2 = gc2, lp_n = lp, ll_n = ll, post_n = lp + ll;
    int alive = 1;
    for (int i = 1; i <= a.n_leapfrog; ++i) {
#ifdef TDA_DENSE_MASS
      tda_dense_product(cholT, a.d, a.DP, s_vec, lane, p, p2, v, v2);  // v = L q
      th += eps * v;  // (a lane without a parameter keeps q = v = r = 0 and th = 0)
      th2 += eps * v2;
#else
      th += eps * (w * p);  // (a lane without a parameter keeps p = 0 and th = 0)
      th2 += eps * (w2 * p2);
#endif
      __syncthreads();
      s_th[lane] = th;
      s_th[lane2] = th2;
      __syncthreads();
      const double sum = tda_wave_sum(tda_mala_outputs(a, s_th, s_sens, s_work, lane));
      ll_n = tda_loglike_of_sum(sum, a.w, a.var);
#if defined(TDA_PRIOR_SOURCE) && defined(TDA_PRIOR_WAVE)
      lp_n = tda_wave_sum(tda_logprior_wave(s_th, a.d, a.pr_mean, a.pr_pinv, lane));
#elif defined(TDA_PRIOR_SOURCE)
      double pj = lj ? tda_logprior_term(th, pm, pinv, lane) : 0.0;
      if (lj2) pj += tda_logprior_term(th2, pm2, pinv2, lane2);
      lp_n = tda_wave_sum(pj);
#else
      double pj = 0.0;
      if (lj) {
        const double dv = th - pm;
        pj = dv * dv * pinv;
      }
      if (lj2) {
        const double dv2 = th2 - pm2;
        pj += dv2 * dv2 * pinv2;
      }
      lp_n = -0.5 * (a.logconst + tda_wave_sum(pj));
#endif
      post_n = lp_n + ll_n;
      alive = __builtin_amdgcn_readfirstlane(__builtin_isfinite(post_n) ? 1 : 0);
      if (!alive) break;
#ifdef TDA_GRADIENT_WAVE
      s_grad[lane] = 0.0;  // (its readers of the previous leapfrog step are behind the barriers above)
      s_grad[lane2] = 0.0;
#endif
      __syncthreads();  // s_sens complete
#ifdef TDA_GRADIENT_WAVE
      tda_gradient_wave(s_th, a.d, s_sens, a.m, s_grad, s_work, lane);
      __syncthreads();
      g = lj ? TDA_PRIOR_GRAD(th, pm, pinv, lane) + s_grad[lane] : 0.0;
      g2 = lj2 ? TDA_PRIOR_GRAD(th2, pm2, pinv2, lane2) + s_grad[lane2] : 0.0;
#else
      g = lj ? TDA_PRIOR_GRAD(th, pm, pinv, lane) + tda_gradient(s_th, a.d, s_sens, a.m, lane) : 0.0;
      g2 = lj2 ? TDA_PRIOR_GRAD(th2, pm2, pinv2, lane2) + tda_gradient(s_th, a.d, s_sens, a.m, lane2) : 0.0;
#endif
      const double cc = i < a.n_leapfrog ? eps : he;
#ifdef TDA_DENSE_MASS
      tda_dense_product(chol, a.d, a.DP, s_vec, lane, g, g2, fr, fr2);
      p += cc * fr;
      p2 += cc * fr2;
#else
      p += cc * g;
      p2 += cc * g2;
#endif
    }
    // a gradient that is not finite leaves a NaN momentum: the next position's log-posterior is NaN and ends the trajectory, or
    // (at the last step) k1 is NaN, alpha is NaN and `u < NaN` is false
#ifdef TDA_DENSE_MASS
    const double k1 = 0.5 * tda_wave_sum(p * p + p2 * p2);
#else
    const double k1 = 0.5 * tda_wave_sum(w * (p * p) + w2 * (p2 * p2));
#endif
    double alpha = exp((post_n - (lp + ll)) + (k0 - k1));
    if (!alive || post_n != post_n) alpha = 0.0;
    const bool acc = a.u[(size_t)s * a.NP + c] < alpha;
    if (acc) {
      lp = lp_n;
      ll = ll_n;
      cur = th;
      cur2 = th2;
      gc = g;
      gc2 = g2;
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
#else
extern "C" __global__ void __launch_bounds__(64) tda_user_mala_steps(const UserMalaArgs a) {
  extern __shared__ double s_sens[];  // [m] ([2 m] under TDA_LOGLIKE_WAVE: the outputs behind the sensitivities)
  __shared__ double s_th[128];
  TDA_DECLARE_WORK;
#ifdef TDA_GRADIENT_WAVE
  __shared__ double s_grad[128];  // J^T sens of the proposal, all parameters from one tda_gradient_wave call
#endif
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
    const double sum = tda_wave_sum(tda_mala_outputs(a, s_th, s_sens, s_work, lane));
#if defined(TDA_PRIOR_SOURCE) && defined(TDA_PRIOR_WAVE)
    // a prior that couples parameters: as tda_user_steps calls and sums it (the same bits for the same state)
    const double ll_n = tda_loglike_of_sum(sum, a.w, a.var);
    const double lp_n = tda_wave_sum(tda_logprior_wave(s_th, a.d, a.pr_mean, a.pr_pinv, lane));
#elif defined(TDA_PRIOR_SOURCE)
    // source-defined prior: the terms summed as tda_user_steps sums them (the same bits for the same state); -inf outside a support
    double pj = lj ? tda_logprior_term(prp, pm, pinv, lane) : 0.0;
    if (lj2) pj += tda_logprior_term(prp2, pm2, pinv2, lane2);
    const double ll_n = tda_loglike_of_sum(sum, a.w, a.var);
    const double lp_n = tda_wave_sum(pj);  // distributions.py:44-56 (JointPrior.logpdf)
#else
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
    const double ll_n = tda_loglike_of_sum(sum, a.w, a.var);  // (in both branches: below the #endif the Gaussian programs lose the instruction order they had)
    const double lp_n = -0.5 * (a.logconst + maha);  // scipy MVN logpdf, posterior.py:92
#endif
    const double post_n = lp_n + ll_n;               // link.py:48
#ifdef TDA_GRADIENT_WAVE
    s_grad[lane] = 0.0;  // (its readers of the previous step are behind the barriers above)
    s_grad[lane2] = 0.0;
#endif
    __syncthreads();  // s_sens complete
    // gradient at the proposal: grad log prior + J^T grad loglike (proposal.py:996-998; utils.py:273-287)
#ifdef TDA_GRADIENT_WAVE
    tda_gradient_wave(s_th, a.d, s_sens, a.m, s_grad, s_work, lane);
    __syncthreads();
    const double gp = lj ? TDA_PRIOR_GRAD(prp, pm, pinv, lane) + s_grad[lane] : 0.0;
    const double gp2 = lj2 ? TDA_PRIOR_GRAD(prp2, pm2, pinv2, lane2) + s_grad[lane2] : 0.0;
#else
    const double gp = lj ? TDA_PRIOR_GRAD(prp, pm, pinv, lane) + tda_gradient(s_th, a.d, s_sens, a.m, lane) : 0.0;
    const double gp2 = lj2 ? TDA_PRIOR_GRAD(prp2, pm2, pinv2, lane2) + tda_gradient(s_th, a.d, s_sens, a.m, lane2) : 0.0;
#endif
    // transition densities (proposal.py:1000-1005): q(x|y) = -|x - y - s^2/2 grad(y)|^2 / (2 s^2)
    // A proposal outside a source-defined prior's support is rejected whatever tda_logprior_term_grad (tda_logprior_grad) returns there (NaN, +-inf):
    // lp_n is -inf, so post_n - (lp + ll) is -inf or NaN, and a sum that holds a -inf is -inf or NaN whatever is added to it
    // (kq < 0 and qa >= 0 or NaN: kq * qa is never +inf; kq * qb is finite, gc being the gradient at a state inside the support,
    // and were it not, -inf + inf is NaN).  alpha is 0 or NaN, `u < NaN` is false, and gc only ever takes an accepted gp.
    // The first gc is tda_user_mala_grad0's at theta0, which nothing guards: a chain started outside a support has log-prior -inf
    // and whatever gradient the source returns there, as the host protocol and the oracle have it.
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
#endif  // TDA_USER_HMC
// gradient of the log-posterior at the current states (init; the padding of a row is written as zero)
extern "C" __global__ void __launch_bounds__(64) tda_user_mala_grad0(const UserMalaArgs a) {
  extern __shared__ double s_sens[];
  __shared__ double s_th[128];
  TDA_DECLARE_WORK;
  const int lane = threadIdx.x, lane2 = lane + 64;
  const long long c = blockIdx.x;
  if (c >= a.N) return;
  const bool lj = lane < a.d, lj2 = lane2 < a.d;
  const size_t row = (size_t)c * a.DP;
  const double th = lj ? a.theta[row + lane] : 0.0, th2 = lj2 ? a.theta[row + lane2] : 0.0;
  s_th[lane] = th;
  s_th[lane2] = th2;
  __syncthreads();
  (void)tda_mala_outputs(a, s_th, s_sens, s_work, lane);
#ifdef TDA_GRADIENT_WAVE
  __shared__ double s_grad[128];
  s_grad[lane] = 0.0;
  s_grad[lane2] = 0.0;
  __syncthreads();
  tda_gradient_wave(s_th, a.d, s_sens, a.m, s_grad, s_work, lane);
  __syncthreads();
  if (lane < a.DP) a.grad[row + lane] = lj ? TDA_PRIOR_GRAD(th, a.pr_mean[lane], a.pr_pinv[lane], lane) + s_grad[lane] : 0.0;
  if (lane2 < a.DP) a.grad[row + lane2] = lj2 ? TDA_PRIOR_GRAD(th2, a.pr_mean[lane2], a.pr_pinv[lane2], lane2) + s_grad[lane2] : 0.0;
#else
  __syncthreads();
  if (lane < a.DP) a.grad[row + lane] = lj ? TDA_PRIOR_GRAD(th, a.pr_mean[lane], a.pr_pinv[lane], lane) + tda_gradient(s_th, a.d, s_sens, a.m, lane) : 0.0;
  if (lane2 < a.DP) a.grad[row + lane2] = lj2 ? TDA_PRIOR_GRAD(th2, a.pr_mean[lane2], a.pr_pinv[lane2], lane2) + tda_gradient(s_th, a.d, s_sens, a.m, lane2) : 0.0;
#endif
}
#endif  // TDA_USER_MAP
#endif  // TDA_USER_MALA

#if defined(TDA_USER_MAP) && !defined(TDA_USER_REPLAY)
// A mode of the posterior (the reference's get_MAP / get_ML, utils.py:204-269: scipy.optimize.minimize over a Python callable
// from one start), from many starts at once: one wave per start, lane j owns parameters j and j + 64, one launch takes every
// start from its initial point to its end.  The objective f is lp_n + ll_n of tda_user_mala_steps (objective 1: ll_n alone,
// the prior and its support ignored), the gradient its gp -- or, without a gradient in the source, forward differences of f.
// L-BFGS ascent: the last TDA_MAP_HISTORY pairs s = x' - x, y = g - g' in LDS (a lane reads and writes its own two entries of a
// pair only, so the ring needs no barrier), two-loop recursion with every inner product a tda_wave_sum, initial scaling
// s^T y / y^T y.  Without history the direction is g, scaled to unit 2-norm when |g|_2 > 1.  Backtracking Armijo from t = 1; a
// trial whose value is NaN or -inf (outside a support) fails like any other, so iterates never leave the support.
// Every value that a branch around a source function is taken on is the result of tda_wave_sum / tda_map_max (an xor butterfly:
// the same bits in all 64 lanes) or a kernel argument: the wave never diverges around a call that may hold a barrier, every
// loop has a static bound, and the wave leaves the iteration loop at its top only.
__device__ __forceinline__ double tda_map_max(double v) {
  for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off));
  return v;
}
__device__ __forceinline__ bool tda_map_finite(double v) { return v - v == 0.0; }
// f at (x, x2): the point goes into s_th behind the barrier that ends the previous evaluation's reads
__device__ __forceinline__ double tda_map_value(const UserMapArgs& a, double* s_th, double* s_buf, double* s_work, int lane, double x, double x2, double& lp,
                                                double& ll) {
  __syncthreads();
  s_th[lane] = x;
  s_th[lane + 64] = x2;
  __syncthreads();
  ll = tda_map_loglike(a, s_th, s_buf, s_work, lane);
  lp = tda_map_logprior(a, s_th, lane, x, x2);
  return a.objective == 0 ? lp + ll : ll;
}
#ifndef TDA_USER_MALA
// forward differences of f at (x, x2), where f = f0: h_j = 2^-26 max(1, |x_j|) (scipy's step for the reference's call), the
// backward difference where the forward point is not finite; false when neither is.  d evaluations by the wave, one after the other.
__device__ __forceinline__ bool tda_map_difference(const UserMapArgs& a, double* s_th, double* s_buf, double* s_work, int lane, double x, double x2, double f0,
                                                   double& g, double& g2, int& neval) {
  bool ok = true;
  g = 0.0, g2 = 0.0;
  for (int j = 0; j < a.d; ++j) {
    const double xj = __shfl(j < 64 ? x : x2, j & 63);
    const double hj = (xj + 0x1p-26 * fmax(1.0, fabs(xj))) - xj;  // (the step that the addition really takes)
    const bool mine = lane == (j & 63);
    double lp, ll;
    double fj = tda_map_value(a, s_th, s_buf, s_work, lane, mine && j < 64 ? x + hj : x, mine && j >= 64 ? x2 + hj : x2, lp, ll);
    double gj = (fj - f0) / hj;
    ++neval;
    if (!tda_map_finite(fj)) {
      fj = tda_map_value(a, s_th, s_buf, s_work, lane, mine && j < 64 ? x - hj : x, mine && j >= 64 ? x2 - hj : x2, lp, ll);
      gj = (f0 - fj) / hj;
      ++neval;
      ok = ok && tda_map_finite(fj);
    }
    if (mine && j < 64) g = gj;
    if (mine && j >= 64) g2 = gj;
  }
  return ok;
}
#endif
extern "C" __global__ void __launch_bounds__(64) tda_user_maximize(const UserMapArgs a) {
#ifdef TDA_USER_MALA
  extern __shared__ double s_buf[];  // s_sens[m] ([2 m] under TDA_LOGLIKE_WAVE), as in tda_user_mala_steps
#else
  TDA_DECLARE_OUT;
  double* const s_buf = s_out;
#endif
  __shared__ double s_th[128];
  TDA_DECLARE_WORK;
#if defined(TDA_USER_MALA) && defined(TDA_GRADIENT_WAVE)
  __shared__ double s_grad[128];
#else
  double* const s_grad = nullptr;
#endif
  __shared__ double s_S[TDA_MAP_HISTORY][128], s_Y[TDA_MAP_HISTORY][128];  // the ring of pairs
  __shared__ double s_rho[TDA_MAP_HISTORY];                                 // 1 / s^T y of a pair (every lane writes the same bits)
  __shared__ double s_x[128], s_g[128];  // the point and its gradient, a lane's own two entries: not in registers across the source's functions
  const int lane = threadIdx.x, lane2 = lane + 64;
  const long long c = blockIdx.x;
  if (c >= a.N) return;
  const bool lj = lane < a.d, lj2 = lane2 < a.d;
  // log-prior and log-likelihood of the point, the scaling s^T y / y^T y and the last gain: carried from iteration to iteration
  // and read a few times in each, so they live in LDS too (every lane writes the same bits and reads its own write back)
  __shared__ double s_stat[4];
  double f = 0.0, gmax = __builtin_nan("");
  s_stat[0] = 0.0, s_stat[1] = 0.0, s_stat[2] = 1.0, s_stat[3] = 0.0;
  int neval = 0, iters = 0, status = -1, count = 0, head = 0;
  s_x[lane] = lj ? a.x0[c * a.d + lane] : 0.0, s_x[lane2] = lj2 ? a.x0[c * a.d + lane2] : 0.0;
  s_g[lane] = 0.0, s_g[lane2] = 0.0;
  // Pass -1 evaluates the start, as the one "trial" of a search with the zero direction that a finite value accepts: the
  // source's functions are inlined at one place for the objective and one for the gradient, whatever point they are called at.
  for (int it = -1; it <= a.max_iter; ++it) {
    const bool first = it < 0;
    if (status >= 0) break;
    if (!first && gmax <= a.gtol) {
      status = TDA_MAP_CONVERGED_GRADIENT;
      break;
    }
    if (it > 0 && a.ftol > 0.0 && s_stat[3] <= a.ftol * fmax(1.0, fabs(f))) {
      status = TDA_MAP_CONVERGED_VALUE;
      break;
    }
    if (it == a.max_iter) {
      status = TDA_MAP_MAX_ITER;
      break;
    }
    // the direction: two-loop recursion over the pairs, newest first
    double p = s_g[lane], p2 = s_g[lane2], al[TDA_MAP_HISTORY];
#pragma unroll
    for (int k = 0; k < TDA_MAP_HISTORY; ++k) {
      al[k] = 0.0;
      if (k < count) {
        const int slot = (head - 1 - k) & (TDA_MAP_HISTORY - 1);
        al[k] = s_rho[slot] * tda_wave_sum(s_S[slot][lane] * p + s_S[slot][lane2] * p2);
        p -= al[k] * s_Y[slot][lane];
        p2 -= al[k] * s_Y[slot][lane2];
      }
    }
    if (count > 0) {
      p *= s_stat[2];
      p2 *= s_stat[2];
    }
#pragma unroll
    for (int k = TDA_MAP_HISTORY - 1; k >= 0; --k) {
      if (k < count) {
        const int slot = (head - 1 - k) & (TDA_MAP_HISTORY - 1);
        const double beta = s_rho[slot] * tda_wave_sum(s_Y[slot][lane] * p + s_Y[slot][lane2] * p2);
        p += s_S[slot][lane] * (al[k] - beta);
        p2 += s_S[slot][lane2] * (al[k] - beta);
      }
    }
    double gtp = tda_wave_sum(s_g[lane] * p + s_g[lane2] * p2);
    if (count > 0 && !(gtp > 0.0 && tda_map_finite(gtp))) count = 0;  // not an ascent direction: the history is dropped
    // backtracking Armijo, along the L-BFGS direction and, when every trial there failed, once more along the gradient
    // Where the values no longer tell the points apart (|f' - f| <= TDA_MAP_FLOOR eps max(1, |f|): the gain of a good step near a
    // maximum, g^T H^-1 g / 2, drops below the rounding of f long before the gradient is small) the trial is judged by its
    // slope p^T g' instead, the approximate Wolfe conditions of Hager and Zhang (2005): -(1 - 2 c1) g^T p <= p^T g' <= 0.9 g^T p.
    bool accepted = false, okn = true;
    double xn = 0.0, xn2 = 0.0, fn = f, lpn = 0.0, lln = 0.0, gn = 0.0, gn2 = 0.0;
    for (int attempt = 0; attempt < 2 && !accepted; ++attempt) {
      if (attempt == 1) {
        if (count == 0) break;  // (the first attempt already went along the gradient)
        count = 0;
      }
      if (count == 0) {  // (the start's pass: g = 0, the zero direction)
        const double g = s_g[lane], g2 = s_g[lane2];
        const double gg = tda_wave_sum(g * g + g2 * g2), scale = gg > 1.0 ? 1.0 / sqrt(gg) : 1.0;
        p = g * scale, p2 = g2 * scale;
        gtp = gg * scale;
      }
      double t = 1.0;
      for (int k = 0; k <= TDA_MAP_HALVINGS; ++k) {
        xn = s_x[lane] + t * p, xn2 = s_x[lane2] + t * p2;
        fn = tda_map_value(a, s_th, s_buf, s_work, lane, xn, xn2, lpn, lln);
        ++neval;
        const bool armijo = tda_map_finite(fn) && (first || fn >= f + 1e-4 * t * gtp);
        if (armijo || (tda_map_finite(fn) && fabs(fn - f) <= TDA_MAP_FLOOR * 0x1p-52 * fmax(1.0, fabs(f)))) {
          // the gradient at the trial, the last point evaluated: of an accepted trial it is the next iteration's
#ifdef TDA_USER_MALA
          tda_map_gradient(a, s_th, s_buf, s_grad, s_work, lane, xn, xn2, gn, gn2);
#else
          okn = tda_map_difference(a, s_th, s_buf, s_work, lane, xn, xn2, fn, gn, gn2, neval);
#endif
          const double slope = tda_wave_sum(gn * p + gn2 * p2);
          if (armijo || (okn && slope >= -(1.0 - 2e-4) * gtp && slope <= 0.9 * gtp)) {
            accepted = true;
            break;
          }
        }
        if (first) break;
        t *= 0.5;
      }
    }
    if (first) {  // the start: its value, and where that is finite its gradient
      f = fn, s_stat[0] = lpn, s_stat[1] = lln;
      if (!accepted) {
        status = TDA_MAP_INFEASIBLE_START;
        continue;
      }
      s_g[lane] = gn, s_g[lane2] = gn2;
      gmax = tda_map_max(fmax(fabs(gn), fabs(gn2)));
      if (!okn || tda_wave_sum(tda_map_finite(gn) && tda_map_finite(gn2) ? 0.0 : 1.0) != 0.0) status = TDA_MAP_NONFINITE_GRADIENT;
      continue;
    }
    if (!accepted) {
      status = TDA_MAP_LINESEARCH_FAILED;
      continue;
    }
    const bool ok = okn;
    const double sx = xn - s_x[lane], sx2 = xn2 - s_x[lane2], yg = s_g[lane] - gn, yg2 = s_g[lane2] - gn2;
    const double sy = tda_wave_sum(sx * yg + sx2 * yg2), yy = tda_wave_sum(yg * yg + yg2 * yg2);
    s_stat[3] = fn - f;
    s_x[lane] = xn, s_x[lane2] = xn2, f = fn, s_stat[0] = lpn, s_stat[1] = lln, s_g[lane] = gn, s_g[lane2] = gn2;
    ++iters;
    gmax = tda_map_max(fmax(fabs(gn), fabs(gn2)));
    if (!ok || tda_wave_sum(tda_map_finite(gn) && tda_map_finite(gn2) ? 0.0 : 1.0) != 0.0) {
      status = TDA_MAP_NONFINITE_GRADIENT;
      continue;
    }
    if (sy > 0x1p-52 * yy) {  // curvature along the step: the pair enters the ring
      s_S[head][lane] = sx, s_S[head][lane2] = sx2;
      s_Y[head][lane] = yg, s_Y[head][lane2] = yg2;
      s_rho[head] = 1.0 / sy;
      s_stat[2] = sy / yy;
      head = (head + 1) & (TDA_MAP_HISTORY - 1);
      count = count < TDA_MAP_HISTORY ? count + 1 : TDA_MAP_HISTORY;
    }
  }
  if (lj) a.x[c * a.d + lane] = s_x[lane];
  if (lj2) a.x[c * a.d + lane2] = s_x[lane2];
  if (lane == 0) {
    double* st = a.stats + c * 6;
    st[0] = s_stat[0], st[1] = s_stat[1], st[2] = f, st[3] = gmax, st[4] = (double)iters, st[5] = (double)neval;
    a.status[c] = status;
  }
}
#endif  // TDA_USER_MAP
