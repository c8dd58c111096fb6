/*
 * tinyda_amd_nuts.h  --  the no-U-turn sampler over a source-defined posterior (libtinyda_hip.so).
 *
 * An extension: the reference has no NUTS.  The proposal is set like any other, tda_engine_set_proposal with kind TDA_PROP_NUTS
 * (scaling = the leapfrog step size eps; adaptive / gamma / period adapt it at the period boundary, see below), over what HMC
 * takes (tinyda_amd_hmc.h): a single level set by tda_engine_set_level_source whose source defines tda_gradient or
 * tda_gradient_wave, isotropic / diagonal noise or a source-defined likelihood with its gradient, a diagonal Gaussian prior or a
 * source-defined prior with its gradient, dim <= 128, n_outputs <= 2048.  tda_engine_init refuses anything else, the engine's own
 * linear model included.
 *
 * The algorithm: multinomial NUTS with a diagonal inverse mass w, in iterative (non-recursive) form.  The kernel
 * (tda_user_nuts_steps, one wave per chain), the host class tinyda_amd.NUTS and the tests' NumPy twin follow this text.
 * One step of a chain, with z the step's d unit normals, pi the log-posterior and g its gradient:
 *
 * 1. Start.  p0 = z / sqrt(w), H0 = -pi(theta) + 1/2 sum_j w_j p0_j^2.  The tree is the single leaf (theta, p0, g); both edges
 *    are that leaf; rho = p0 is the sum of momenta over the tree; the tree's log-weight is LW = 0; the candidate is the initial state.
 * 2. Doublings j = 0 .. max_depth - 1.  One Philox block (below) gives the direction bit and the uniform u_j.  The bit chooses
 *    the edge to extend: forward with step size e = +eps, backward with e = -eps.  The new subtree of 2^j leaves is built one
 *    leapfrog step after the other from that edge, each one HMC's step in its order of operations,
 *        p += (e/2) g;  theta += e (w p);  pi, g at theta;  p += (e/2) g
 *    (a backward step uses the actual momentum and -eps; nothing is negated and restored).  Per new leaf i with energy
 *    H_i = -pi + 1/2 sum_j w_j p_j^2:
 *      - Divergence.  The leaf is divergent if pi is NaN or infinite there (the gradient is then not evaluated), or H_i is NaN, or
 *        H_i - H0 > 1000.  It adds 0 to the acceptance sum and 1 to the leaf count; the subtree is discarded and the tree stops.
 *      - Acceptance statistic.  Otherwise lw_i = H0 - H_i is the leaf's log-weight, and min(1, exp(lw_i)) is added to the sum.
 *      - Selection.  The subtree's log-weight is LW' = lw_1 at its first leaf and LW' <- logaddexp(LW', lw_i) after, with
 *        logaddexp(a, b) = max + log1p(exp(min - max)).  The first leaf is the subtree's candidate; a later leaf replaces it
 *        iff its uniform < exp(lw_i - LW') (LW' updated first).
 *      - U-turn inside the subtree.  rho' is the sum of the subtree's momenta (rho' = p at the first leaf, rho' += p after).
 *        With the leaves numbered n = 0 .. 2^j - 1: an even leaf stores the checkpoint (p, rho') in row popcount(n >> 1); an odd
 *        leaf closes the aligned sub-subtrees of 2^k leaves for k = 1 .. t, t the number of trailing one bits of n (the subtree
 *        itself at its last leaf), whose first leaves are the checkpoints of the rows popcount(n >> 1) down to popcount(n >> 1) - t + 1.
 *        With (p_a, r_a) such a checkpoint, p_b = p and rho'' = (rho' - r_a) + p_a, elementwise per parameter, the sub-subtree
 *        turns iff not ((w o p_a) . rho'' > 0 and (w o p_b) . rho'' > 0); a NaN therefore turns.  A turning sub-subtree discards
 *        the new subtree and stops the tree.  At most max_depth - 1 rows are in use.
 *    Merge, for a subtree that completed: its candidate replaces the tree's iff u_j < exp(LW' - LW) (the biased progressive
 *    rule); LW <- logaddexp(LW, LW'), rho <- rho + rho'; the extended edge becomes the subtree's last leaf; the same U-turn test on
 *    the whole tree (p-, p+, rho) stops it after the merge, and it keeps its candidate.
 * 3. End.  The new state is the candidate (theta, log-prior, log-likelihood, gradient).  The step's `accepted` record is 1 iff the
 *    candidate is not the initial leaf; its acceptance statistic is the acceptance sum over the leaf count.  The tree's depth is
 *    the number of merged doublings.  A tree that merged max_depth doublings and was stopped by none of the tests counts as a
 *    tree at max_depth.
 *
 * RNG stream (beside the streams 0 - 7 of tinyda_amd.h, "RNG stream"): all tree draws are Philox4x32-10 words x with the engine's
 * key and counter = (block, global step, global chain id, stream 8).  Doubling j uses block j: direction = x.z & 1 (1 = forward),
 * u_j = u53(x.x, x.y).  The l-th leaf made in a step (l = 1, 2, ...; discarded and divergent leaves count) uses block 32 + l and
 * the uniform u53(x.x, x.y), drawn only where the selection uses it (never at a subtree's first leaf).  The momentum's normals are
 * stream 0, as for HMC: exported by set_export and replaced by set_replay; the accept uniform u is not read, and under
 * set_replay the tree draws still come from Philox.
 *
 * Step-size adaptation: with adaptive != 0 the engine's rule applies at the period boundary, scaling <- exp(log scaling +
 * gamma^-k (rate - target_accept)), rate = (the sum of the period's per-step acceptance statistics, added in step order) / period.
 *
 * Chain state and records are MALA's; a NUTS engine's checkpoint blob also carries the period's acceptance sum and the totals.
 * Conventions as in tinyda_amd.h: TDA_OK (0) or a negative tda_status, tda_last_error() gives the message.
 */
#ifndef TINYDA_AMD_NUTS_H
#define TINYDA_AMD_NUTS_H

#include <stdint.h>

#include "tinyda_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Depth, adaptation target and mass of the NUTS proposal: after tda_engine_set_proposal(kind = TDA_PROP_NUTS), before
 * tda_engine_init (defaults without this call: max_depth 8, target 0.8, unit mass).  1 <= max_depth <= 10; 0 < target_accept < 1;
 * inv_mass: HOST [dim], finite and > 0, or NULL for unit mass.  The U-turn checkpoints take 2 * max_depth * DP doubles of LDS per
 * chain (DP: dim padded to 8, 16, 32, 64 or 128) beside what MALA holds for the source; tda_engine_init refuses a source that then
 * needs more than 64 KiB, with the byte counts. */
int tda_engine_set_nuts(tda_engine* e, int32_t max_depth /* 1..10 */, double target_accept /* (0,1) */, const double* inv_mass /* HOST [dim] or NULL */);

/* Per-chain totals since tda_engine_init (an initialised NUTS engine): totals [n_chains][4], HOST or DEVICE memory -- leapfrog
 * steps (leaves made), divergent trees, trees at max_depth, and the sum of tree depths (mean depth = that sum / steps run). */
int tda_engine_get_nuts_totals(tda_engine* e, int64_t* totals /* HOST or DEVICE [n_chains][4] */);

#ifdef __cplusplus
}
#endif
#endif
