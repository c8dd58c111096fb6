/*
 * tinyda_amd_hmc.h  --  Hamiltonian Monte Carlo over a source-defined posterior (libtinyda_hip.so).
 *
 * An extension: the reference has no HMC.  The proposal is set like any other, tda_engine_set_proposal with kind TDA_PROP_HMC
 * (scaling = the leapfrog step size eps; adaptive / gamma / period adapt it at the period boundary towards 0.65 acceptance), over
 * what MALA over a source-defined model takes: a single level set by tda_engine_set_level_source whose source defines the
 * model's vector-Jacobian product (tda_gradient or tda_gradient_wave), isotropic / diagonal noise or a source-defined likelihood
 * with its gradient, a diagonal Gaussian prior or a source-defined prior with its gradient, dim <= 128, n_outputs <= 2048.
 * tda_engine_init refuses anything else, the engine's own linear model included.
 *
 * One step of a chain (kernel tda_user_hmc_steps, one wave per chain), with z the step's unit normals, u its uniform, w the
 * diagonal inverse mass and g the gradient of the log-posterior pi:
 *     p = z / sqrt(w),  K0 = 1/2 sum_j w_j p_j^2,  p += eps/2 g(theta)
 *     n_leapfrog times:  theta' += eps w p;  p += c g(theta')      (c = eps, eps/2 at the last step)
 *     accept iff u < exp(pi(theta') - pi(theta) + K0 - K1)
 * A position at which pi is NaN or infinite (outside a prior's support, a NaN model output) ends the trajectory and rejects.
 * Chain state, checkpoint blobs, variates (set_export / set_replay: z [S][N][dim], u [S][N]) and records are MALA's.
 *
 * Conventions as in tinyda_amd.h: TDA_OK (0) or a negative tda_status, tda_last_error() gives the message.
 */
#ifndef TINYDA_AMD_HMC_H
#define TINYDA_AMD_HMC_H

#include <stdint.h>

#include "tinyda_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Trajectory length and mass of the HMC proposal: after tda_engine_set_proposal(kind = TDA_PROP_HMC), before tda_engine_init
 * (defaults without this call: 8 leapfrog steps, unit mass).  1 <= n_leapfrog <= 1024; inv_mass: HOST [dim], finite and > 0,
 * or NULL for unit mass. */
int tda_engine_set_hmc(tda_engine* e, int32_t n_leapfrog, const double* inv_mass /* HOST [dim] or NULL */);

#ifdef __cplusplus
}
#endif
#endif
