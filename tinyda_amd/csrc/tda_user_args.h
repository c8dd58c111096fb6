// Kernel arguments of the source-defined ("user") programs, written once: the host includes this header (tda_usermodel.inc) and
// hands the same bytes to hiprtc as the named header "tda_user_args.h" of tda_user_program.hip.  Plain C++ without includes;
// the member order is the kernel-argument layout.
#pragma once

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
