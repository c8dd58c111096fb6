/*
 * tinyda_amd_optimize.h  --  modes of a source-defined posterior: multi-start L-BFGS on the device (libtinyda_hip.so).
 *
 * The reference's get_MAP / get_ML (tinyDA/utils.py:204-269) run scipy.optimize.minimize over posterior.create_link(x), one
 * Python model call per function evaluation, from one start.  Here the posterior is HIP source (the source of
 * tda_engine_set_level_source: the model, and beside it a likelihood and a prior where they are source-defined), and one kernel,
 * tda_user_maximize, takes any number of starts from their initial points to their ends in one launch: one wave per start.
 * The optimiser needs no tda_engine and no proposal: it is an object of its own, compiled once and run over any number of sets
 * of starts.
 *
 * Objective: log-prior + log-likelihood (TDA_OBJECTIVE_POSTERIOR), evaluated exactly as the MALA kernel evaluates it, or the
 * log-likelihood alone (TDA_OBJECTIVE_LIKELIHOOD; the prior and its support are then ignored).  Gradient: the source's own
 * (use_source_gradient: tda_gradient / tda_gradient_wave and the gradients of a source-defined likelihood and prior, as MALA
 * requires them), or forward differences of the objective with h_j = 2^-26 max(1, |x_j|), d evaluations per gradient.
 * Algorithm: L-BFGS with 8 pairs, initial scaling s^T y / y^T y, first direction the gradient (scaled to unit 2-norm when its
 * norm exceeds 1); backtracking Armijo line search (t = 1, halved at most 40 times, c1 = 1e-4) in which a trial whose value is
 * NaN or -inf fails like any other, so iterates never leave a prior's support; a failed search drops the pairs and tries the
 * gradient once.  Where two values no longer tell the points apart (|f' - f| <= 64 eps max(1, |f|), which near a maximum happens
 * long before the gradient is small) a trial is accepted on its slope instead, -(1 - 2 c1) g^T p <= p^T g' <= 0.9 g^T p (the
 * approximate Wolfe conditions of Hager and Zhang, 2005).  LDS per start: that of the MALA (or step) program of the same source + 18528 bytes, at most 64 KiB.
 *
 * Conventions as in tinyda_amd.h: TDA_OK (0) or a negative tda_status, tda_last_error() gives the message.
 */
#ifndef TINYDA_AMD_OPTIMIZE_H
#define TINYDA_AMD_OPTIMIZE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tda_optimizer tda_optimizer;

enum { TDA_OBJECTIVE_POSTERIOR = 0, TDA_OBJECTIVE_LIKELIHOOD = 1 };

/* how a start ended (status[i] of tda_optimizer_run) */
enum {
  TDA_OPT_CONVERGED_GRADIENT = 0, /* max_j |g_j| <= gtol */
  TDA_OPT_CONVERGED_VALUE = 1,    /* ftol > 0 and an accepted step gained <= ftol * max(1, |f|) */
  TDA_OPT_MAX_ITER = 2,
  TDA_OPT_LINESEARCH_FAILED = 3,
  TDA_OPT_INFEASIBLE_START = 4, /* the objective is not finite at the start: the start is returned */
  TDA_OPT_NONFINITE_GRADIENT = 5
};

/* The posterior.  Every pointer is HOST memory and is copied by tda_optimizer_create.
 * noise_kind / noise as in tda_engine_set_level_source: TDA_NOISE_ISO (noise[0] the variance), TDA_NOISE_DIAG (n_outputs
 * variances) or TDA_NOISE_SOURCE (n_outputs parameters of the source's likelihood).
 * prior_kind / prior_loc / prior_scale as in tda_engine_set_prior_joint, one entry per parameter: TDA_PRIOR_NORMAL,
 * TDA_PRIOR_UNIFORM (mixed freely), or TDA_PRIOR_SOURCE for every parameter (loc / scale are then the source's p / q). */
typedef struct tda_optimize_problem {
  uint32_t struct_size;
  int32_t dim;       /* 1..128 */
  int32_t n_outputs; /* >= 1 */
  int32_t noise_kind;
  int32_t use_source_gradient; /* 0: forward differences */
  int32_t reserved;
  const double* data; /* [n_outputs] */
  const double* noise;
  const int32_t* prior_kind; /* [dim] */
  const double* prior_loc;   /* [dim] */
  const double* prior_scale; /* [dim] */
} tda_optimize_problem;

typedef struct tda_optimize_options {
  uint32_t struct_size;
  int32_t max_iter; /* >= 0 */
  double gtol;      /* >= 0 */
  double ftol;      /* >= 0; 0 switches the value test off */
} tda_optimize_options;

/* compile the optimiser of `source` for `problem` on `device` */
int tda_optimizer_create(int device, const char* source, const tda_optimize_problem* problem, tda_optimizer** out);

/* n starts [n][dim] -> x [n][dim], stats [n][6] (log-prior, log-likelihood, objective, max_j |gradient_j|, iterations,
 * objective evaluations) and status [n] (int32).  All four are DEVICE memory, row-major; the launch is queued on `stream`
 * and not waited for. */
int tda_optimizer_run(tda_optimizer* opt, const double* starts, int64_t n, int32_t objective, const tda_optimize_options* options,
                      double* x, double* stats, int32_t* status, void* stream);

void tda_optimizer_destroy(tda_optimizer* opt);

#ifdef __cplusplus
}
#endif
#endif
