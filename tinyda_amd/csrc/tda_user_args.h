// Kernel arguments of the source-defined ("user") programs, written once: the host includes this header (tda_usermodel.inc) and
// hands the same bytes to hiprtc as the named header "tda_user_args.h" of tda_user_program.hip.  Plain C++ without includes;
// the member order is the kernel-argument layout.
#pragma once

// The contract's signatures, each written once: the program's static_asserts and the host's refusals are built from these strings.
#define TDA_SIG_FORWARD_WAVE "__device__ void tda_forward_wave(const double* theta, int dim, double* out, int n_outputs, double* work, int lane)"
#define TDA_SIG_GRADIENT_WAVE \
  "__device__ void tda_gradient_wave(const double* theta, int dim, const double* sensitivity, int n_outputs, double* grad, double* work, int lane)"
#define TDA_SIG_GRADIENT "__device__ double tda_gradient(const double* theta, int dim, const double* sensitivity, int n_outputs, int j)"
#define TDA_SIG_LOGLIKE_TERM "__device__ double tda_loglike_term(double f, double y, double p, int o)"
#define TDA_SIG_LOGLIKE_TERM_GRAD "__device__ double tda_loglike_term_grad(double f, double y, double p, int o)"
#define TDA_SIG_LOGLIKE_WAVE "__device__ double tda_loglike_wave(const double* f, int n_outputs, const double* y, const double* p, int lane)"
#define TDA_SIG_LOGLIKE_GRAD_WAVE \
  "__device__ void tda_loglike_grad_wave(const double* f, int n_outputs, const double* y, const double* p, double* sens, int lane)"
#define TDA_SIG_LOGPRIOR_TERM "__device__ double tda_logprior_term(double x, double p, double q, int j)"
#define TDA_SIG_LOGPRIOR_TERM_GRAD "__device__ double tda_logprior_term_grad(double x, double p, double q, int j)"
#define TDA_CALL_LOGPRIOR_WAVE "tda_logprior_wave(const double* theta, int dim, const double* p, const double* q, int lane)"
#define TDA_SIG_LOGPRIOR_WAVE "__device__ double " TDA_CALL_LOGPRIOR_WAVE
#define TDA_SIG_LOGPRIOR_GRAD "__device__ double tda_logprior_grad(const double* theta, int dim, const double* p, const double* q, int j)"
#define TDA_SIG_QOI "__device__ double tda_qoi(const double* theta, int dim, const double* f, int n_outputs, int k)"
#define TDA_SIG_QOI_WAVE \
  "__device__ void tda_qoi_wave(const double* theta, int dim, const double* f, int n_outputs, double* qoi, int n_qoi, double* work, int lane)"

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
  const double* w;  // 1 / diag(noise) or null (isotropic); source-defined likelihood: its per-output parameters (not inverted)
  double var;
  const double* pr_mean;  // diagonal Gaussian prior: mean and 1 / variance; source-defined prior: its p and q per parameter, as given
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
  const double* w;  // as in UserStepArgs
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
  const double* w;  // as in UserStepArgs
  double var;
  const double* pr_mean;
  const double* pr_pinv;
  double logconst;
  double* rec_params;
  double* rec_stats;
  unsigned char* rec_acc;
};

// HMC over a source-defined model (tda_user_hmc_steps): MALA's chain state, variates and records, and the trajectory's
// configuration behind them.  `scaling` is the leapfrog step size.
struct UserHmcArgs : UserMalaArgs {
  int n_leapfrog;          // leapfrog steps per proposal, >= 1
  const double* inv_mass;  // [DP]: the diagonal inverse mass, positive; ones in the padding.  A program built with -DTDA_DENSE_MASS:
                           // [2][DP][DP], the factor L of the dense inverse mass and behind it L^T, zero outside the triangle and in the padding
};

// NUTS over a source-defined model (tda_user_nuts_steps; the algorithm: include/tinyda_amd_nuts.h): MALA's chain state, unit
// normals and records (`u` is not read), the tree's configuration, the Philox position of the launch's first step for the tree
// draws (stream 8), and the per-chain sums that outlive a launch.  `scaling` is the leapfrog step size.
#define TDA_NUTS_MAX_DEPTH 10
#define TDA_NUTS_TOTALS 4  // per chain: leapfrog steps, divergent trees, trees that completed max_depth doublings, sum of tree depths
struct UserNutsArgs : UserMalaArgs {
  int max_depth;           // doublings per tree at the most, 1 .. TDA_NUTS_MAX_DEPTH
  int ck_off;              // where the checkpoints start in the dynamic LDS, in doubles (behind the MALA program's s_sens)
  const double* inv_mass;  // [DP]: the diagonal inverse mass, positive; ones in the padding ([2][DP][DP] under -DTDA_DENSE_MASS, as above)
  unsigned long long seed;
  long long step0, chain_offset;  // global step of this launch's step 0; global id of chain 0
  double* accsum;          // [NP]: the running period's sum of per-step acceptance statistics
  long long* totals;       // [NP][TDA_NUTS_TOTALS]
  double* scaling_out;     // the launch ends a period of an adaptive proposal: scaling <- exp(log scaling + gamma_pow (accsum / period -
                           // alpha_star)) and accsum <- 0 (null: neither)
  int period;
  double gamma_pow, alpha_star;
};

// The replay of recorded parameters through the model (tda_user_replay): outputs and quantities of interest of the rows
// [0, R) of N chains, one wave per chain and segment of `seg` rows.  Either destination may be null.
struct UserReplayArgs {
  long long N, R, seg;
  int d, m, nq;
  const double* params;  // [R][N][d]
  double* outputs;       // [R][N][m] or null
  double* qoi;           // [R][N][nq] or null
  long long* n_eval;     // model evaluations, added to (may be null)
};

// The optimiser (tda_user_maximize): multi-start L-BFGS towards a maximum of the log-posterior (objective 0) or of the
// log-likelihood alone (objective 1), one wave per start, every start from its initial point to its end in one launch.
// TDA_MAP_HISTORY pairs (s, y) per start live in LDS, a ring of 2 * TDA_MAP_HISTORY * 128 doubles, beside the point and its
// gradient (128 doubles each); a start ends with one of the status words below.
#define TDA_MAP_HISTORY 8
#define TDA_MAP_HALVINGS 40
#define TDA_MAP_FLOOR 64.0  // in units of eps max(1, |f|): closer values do not tell two points apart, the line search then looks at slopes
enum {
  TDA_MAP_CONVERGED_GRADIENT = 0,  // max_j |g_j| <= gtol
  TDA_MAP_CONVERGED_VALUE = 1,     // ftol > 0 and an accepted step gained <= ftol * max(1, |f|)
  TDA_MAP_MAX_ITER = 2,
  TDA_MAP_LINESEARCH_FAILED = 3,   // no trial of the backtracking passed, along the L-BFGS direction and along the gradient
  TDA_MAP_INFEASIBLE_START = 4,    // f(x0) is not finite: x0 is returned
  TDA_MAP_NONFINITE_GRADIENT = 5,
};
struct UserMapArgs {
  long long N;
  int d, m, objective, max_iter;
  double gtol, ftol;
  const double* x0;  // [N][d]
  const double* data;
  const double* w;  // as in UserStepArgs
  double var;
  const double* pr_mean;  // as in UserStepArgs
  const double* pr_pinv;
  const double* pr_lo;
  const double* pr_hi;
  double logconst;
  double* x;      // [N][d]
  double* stats;  // [N][6]: log-prior, log-likelihood, objective, max_j |g_j|, iterations, objective evaluations
  int* status;    // [N]
};
