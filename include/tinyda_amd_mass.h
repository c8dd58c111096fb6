/*
 * tinyda_amd_mass.h  --  warm-up adaptation of the diagonal inverse mass of HMC and NUTS (libtinyda_hip.so).
 *
 * An extension: the reference has neither sampler.  HMC (tinyda_amd_hmc.h) and NUTS (tinyda_amd_nuts.h) take a diagonal inverse
 * mass w; with tda_engine_set_mass_adaptation the engine learns it during the first W steps from the states of all its chains,
 * which share one mass vector.  Nothing leaves the device: the step kernels read w from memory at every launch, and the two
 * kernels below (csrc/tda_kernels_mass.h) run on the engine's stream between their launches.  The host class (tinyda_amd.HMC /
 * NUTS with adapt_mass = W) and the tests' NumPy twin follow this text; a host chain pools over itself alone (N = 1 below).
 *
 * Schedule.  W is a multiple of the proposal's period and at least two periods; P = W / period.  In units of periods: period 0
 * is a buffer in which nothing is accumulated (the chains are still leaving their starts).  Windows follow with lengths
 * L = 1, 2, 4, ... periods; a window of length L that would start at period s with s + 3 L > P takes all the rest instead,
 * L = P - s, and is the last (the window after it would not fit whole before W).  P = 2: [1, 2).  P = 8: [1, 2), [2, 4), [4, 8).
 * P = 10: [1, 2), [2, 4), [4, 10).  After step W the mass is frozen.  During the W steps a block of steps never crosses a period
 * boundary, whether the step size adapts or not, so a window's end is always a block's end.
 *
 * Accumulation (k_mass_accumulate, after the step kernel of every block inside a window).  Per chain c < N and parameter j < d,
 * over the block's recorded states x in step order (every step is recorded for this purpose, whatever the caller records):
 *     n += 1;  delta = x - mean;  mean += delta / n;  M2 += delta * (x - mean)
 * with mean = M2 = 0 and n = 0 at the start of a window (n is the same for all chains and parameters: the engine keeps one).
 * The moments after a window therefore do not depend on how a run was cut into blocks or into run() calls.
 *
 * Update (k_mass_update, once at a window's end; one workgroup of 256 threads per parameter j).  Over the N real chains:
 *   1. thread t adds mean_c for c = t, t + 256, ... in that order, starting from 0;
 *   2. a tree over the 256 partial sums: a[t] += a[t + s] for t < s, s = 128, 64, ..., 1;  mbar = a[0] / N;
 *   3. a second pass in the same order gives B = sum_c (mean_c - mbar)^2 and Wn = sum_c M2_c, each by the same tree;
 *   4. var = (Wn + n B) / (n N - 1);
 *   5. with T = n N:  w = var * T / (T + 5) + 1e-3 * 5 / (T + 5)   (evaluated left to right; the regulariser Stan uses).
 * If w is finite and positive, inv_mass[j] = w.  Otherwise the entry keeps its value and the refused count goes up by one.  The
 * moments of the parameter are zeroed and n = 0.  With an adaptive step size the diminishing-adaptation counter k restarts at 0
 * (after the step-size update of the period that ends with the window), so that the gain gamma^-k is full again under the new
 * metric; the step size itself is kept.  The next block's step kernel follows on the same stream and sees the new mass.
 *
 * A mass-adapting engine's checkpoint blob also carries W and the period (checked by set_state, not adopted), inv_mass, the
 * moments, n and the two counts; every other blob is what it was.
 * Conventions as in tinyda_amd.h: TDA_OK (0) or a negative tda_status, tda_last_error() gives the message.
 */
#ifndef TINYDA_AMD_MASS_H
#define TINYDA_AMD_MASS_H

#include <stdint.h>

#include "tinyda_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Adapt the inverse mass during the first warmup_steps steps: after tda_engine_set_hmc / tda_engine_set_nuts (or
 * tda_engine_set_proposal with one of their kinds), before tda_engine_init; 0 switches it off, and so does a later
 * tda_engine_set_proposal.  TDA_ERR_STATE for any other proposal kind; TDA_ERR_INVALID for a warmup_steps that is negative, not
 * a multiple of the period or shorter than two periods.  The mass of set_hmc / set_nuts is the starting mass. */
int tda_engine_set_mass_adaptation(tda_engine* e, int64_t warmup_steps);

/* The mass in force and the adaptation's counters, of any initialised HMC / NUTS engine (adapting or not).
 * info: updates applied, steps accumulated in the running window, the global step at which the next update happens (-1: none),
 * entries refused so far.  Either pointer may be NULL. */
int tda_engine_get_mass(tda_engine* e, double* inv_mass /* HOST or DEVICE [dim] */, int64_t* info /* HOST [4] */);

#ifdef __cplusplus
}
#endif
#endif
