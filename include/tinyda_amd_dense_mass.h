/*
 * tinyda_amd_dense_mass.h  --  a fixed dense inverse mass for HMC and NUTS over a source-defined posterior (libtinyda_hip.so).
 *
 * An extension: the reference has neither sampler.  HMC (tinyda_amd_hmc.h) and NUTS (tinyda_amd_nuts.h) take a diagonal inverse
 * mass w; with tda_engine_set_dense_mass they run under a symmetric positive definite inverse mass W instead, given by its
 * Cholesky factor: W = L L^T, L lower triangular with a positive diagonal.  W is configuration, fixed for the engine's life; the
 * warm-up adaptation of tinyda_amd_mass.h learns a diagonal and is refused beside it.  The kernels (tda_user_hmc_steps /
 * tda_user_nuts_steps built with -DTDA_DENSE_MASS), the host classes tinyda_amd.HMC / NUTS with a [d, d] inv_mass and the tests'
 * NumPy twin follow this text.
 *
 * The whitened momentum.  The momentum p ~ N(0, W^-1) is never held; the kernels hold q = L^T p, so that no triangular solve
 * occurs anywhere.  With z the step's d unit normals, pi the log-posterior and g its gradient:
 *
 *   Draw.            q = z.  (Then p = L^-T z ~ N(0, W^-1).)
 *   Kinetic energy.  K = 1/2 sum_j q_j q_j  (= 1/2 p^T W p).
 *   A leapfrog step of size e (HMC's, and the NUTS leaf, in their order of operations with `w p` replaced by v and g by r):
 *       r = L^T g;  q += (e/2) r;  v = L q;  theta += e v;  pi, g at theta;  r = L^T g;  q += (e/2) r
 *     HMC fuses the interior half steps as it does under a diagonal mass: q += c r with c = eps, and eps / 2 at the last step.
 *     (r depends on g alone, so a kernel may keep the r of a leaf for the first half step of the next.)
 *   NUTS.            The two edges carry q; rho, rho' and the checkpoints (the same rows, the same LDS) are sums of q; a
 *                    (sub)tree turns iff not (q_a . rho'' > 0 and q_b . rho'' > 0), plain dot products, because
 *                    p_a^T W rho_p = q_a . rho_q.  Energies H = -pi + K, divergence, selection, merge, the Philox stream 8 draws
 *                    and the acceptance statistic are those of tinyda_amd_nuts.h.
 *   HMC.             alpha = exp((pi' - pi) + (K0 - K1)), as in tinyda_amd_hmc.h.
 *
 * The two products.  v_i = sum_j L[i][j] q_j and r_i = sum_j L[j][i] g_j, for every parameter i, each accumulated over
 * j = 0, 1, ..., d - 1 IN THAT ORDER, starting from 0.0, with one fused multiply-add per term:  acc <- fma(L.., x_j, acc).
 * The terms outside the triangle multiply an exact zero and leave acc as it is, so W = I gives the unit-mass programs' numbers
 * bit for bit, and so does W = diag(w) whose entries are powers of 4.  (A twin without a fused multiply-add differs by at most
 * d roundings of 2^-53 per product.)  A gradient that is not finite makes every r_i NaN: the energy is NaN and the leaf divergent
 * (HMC: alpha is NaN and the proposal rejected), as under a diagonal mass.
 *
 * On the device the engine keeps two matrices [DP][DP] (DP: dim padded to 8, 16, 32, 64 or 128), L and L^T, row-major, zero
 * outside the triangle and in the padding, so that lane i reads M[j][i] for both products: consecutive lanes on consecutive
 * addresses, the same row for every chain.  The operand x_j is broadcast from 1 KiB of LDS per chain (128 doubles), which only a
 * dense program declares; tda_engine_init refuses a source that then needs more than 64 KiB, with the byte counts.  Lanes without
 * a parameter keep q = v = r = 0.
 *
 * Chain state, records, variates and checkpoint blobs are those of the diagonal engine of the same shape: the mass is not in the blob.
 * Conventions as in tinyda_amd.h: TDA_OK (0) or a negative tda_status, tda_last_error() gives the message.
 */
#ifndef TINYDA_AMD_DENSE_MASS_H
#define TINYDA_AMD_DENSE_MASS_H

#include <stdint.h>

#include "tinyda_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* after tda_engine_set_hmc / tda_engine_set_nuts, before tda_engine_init; NULL switches it off.  chol: HOST [dim][dim] row-major,
 * the lower-triangular factor L of the inverse mass W = L L^T: finite, diagonal > 0, strict upper triangle exactly 0.
 * TDA_ERR_STATE without a preceding HMC / NUTS proposal, or on an engine set to adapt its mass (tda_engine_set_mass_adaptation:
 * the warm-up learns a diagonal); TDA_ERR_INVALID names the offending entry.  A later tda_engine_set_proposal clears it, and it
 * replaces the diagonal inv_mass of set_hmc / set_nuts. */
int tda_engine_set_dense_mass(tda_engine* e, const double* chol);
/* the factor in force of an initialised engine with a dense mass: HOST or DEVICE [dim][dim] */
int tda_engine_get_dense_mass(tda_engine* e, double* chol);

#ifdef __cplusplus
}
#endif
#endif
