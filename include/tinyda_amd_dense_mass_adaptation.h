/*
 * tinyda_amd_dense_mass_adaptation.h  --  warm-up adaptation of a dense inverse mass of HMC and NUTS (libtinyda_hip.so).
 *
 * An extension: the reference has neither sampler.  tinyda_amd_mass.h learns a diagonal inverse mass during warm-up and
 * tinyda_amd_dense_mass.h runs HMC / NUTS under a fixed dense one, W = L L^T.  With tda_engine_set_dense_mass_adaptation the engine
 * learns the dense W during the first `warmup_steps` steps from the states of all its chains, which share one matrix.  Nothing
 * leaves the device: the dense programs read L and L^T, [2][DP][DP], from memory at every launch, and the three kernels below
 * (csrc/tda_kernels_dense_mass.h) run on the engine's stream between their launches.  The host classes (tinyda_amd.HMC / NUTS with
 * adapt_mass = W, adapt_dense = True) and the tests' NumPy twin follow this text; a host chain pools over itself alone (N = 1).
 *
 * Schedule.  That of tinyda_amd_mass.h, word for word: W is a multiple of the proposal's period and at least two periods; period 0
 * is a buffer; windows of 1, 2, 4, ... periods follow and the last takes the rest; after step W the mass is frozen; during the W
 * steps a block of steps never crosses a period boundary; every state of a block is recorded internally, whatever the caller
 * records; the step-size counter k restarts at every update.
 *
 * State.  A shift a[DP]; per chunk c of CH = 16 consecutive chains (NC = ceil(N / 16) chunks) a vector S1[c][DP] and the lower
 * triangle of a matrix S2[c] in tiles of 16 x 16; the count n of steps folded into the running window; `updates`, `refused`.
 * DP is dim padded to 8, 16, 32, 64 or 128; T = ceil(DP / 16) tiles; the tile pairs (ti, tj), tj <= ti, are numbered
 * p = ti (ti + 1) / 2 + tj.
 *
 * Shift (k_dense_mass_shift, before the step kernel of the block that starts a window; S1 = S2 = 0 and n = 0 then).  a_j is the
 * pooled mean of the current state over the N real chains, summed by the rule of k_mass_update (tinyda_amd_mass.h, steps 1 - 2):
 * thread t of 256 adds the chains t, t + 256, ... in that order starting from 0, a tree adds the 256 partial sums,
 * a[t] += a[t + s] for t < s, s = 128, 64, ..., 1, and a_j = a[0] / N.  a_j = 0 exactly for j >= d.  The shift keeps the raw
 * second moments well conditioned when the posterior sits far from the origin; it is a function of the state alone, so a run
 * resumed at a window's start forms the same a.
 *
 * Accumulation (k_dense_mass_accumulate, after the step kernel of every block inside a window: the hot path).  With y = x - a,
 * and y = 0 exactly for chains >= N and parameters >= d:  for each step of the block in step order, and for g = 0, 1, 2, 3 in
 * that order, the four chains 16 c + 4 g .. 16 c + 4 g + 3 of chunk c are the k dimension of one v_mfma_f64_16x16x4 per tile pair:
 *     S2(ti, tj) <- mfma(y[ti], y[tj], S2(ti, tj))          (y[t]: the 16 parameters of tile t by the 4 chains)
 * (how the instruction orders its four products is not documented: the tests hold the result to a bound, not to bits).  Then
 *     S1_j <- S1_j + y_j   for the block's steps in order and, within a step, the chunk's real chains in ascending order.
 * The grouping of (step, chain) into instructions does not depend on where a block starts or ends, and the sums are carried in
 * memory between blocks, so S1 and S2 after a window are bitwise independent of how the window was cut into blocks and run() calls.
 *   What the implementation chose: one workgroup of four waves per chunk; wave w takes the pairs p = w, w + 4, w + 8, ... (nine
 * accumulators of 8 registers at DP = 128); states come straight from global memory, lane (lc, hi) reading parameter 16 t + lc of
 * chain 16 c + 4 g + hi; between blocks S2 lies in global memory in the instruction's own accumulator layout,
 * S2[c][p][r][lane] = entry (16 ti + 4 r + hi, 16 tj + lc), which the update kernel decodes; the entries above the diagonal
 * of a diagonal tile are formed and never read.
 *
 * Update (k_dense_mass_update, one workgroup, once at a window's end).
 *   1. s1 = sum_c S1[c] and s2 = sum_c S2[c], each entry over the chunks in ascending order, starting from 0.
 *   2. T = n N;  m = s1 / T.
 *   3. For i >= j:  C_ij = (s2_ij - (T m_i) m_j) / (T - 1).
 *   4. Stan's dense regulariser, evaluated left to right:  W_ij = C_ij * T / (T + 5), and on the diagonal + 1e-3 * 5 / (T + 5).
 *   5. Left-looking Cholesky by columns j ascending: acc = W_ij; acc <- fma(-L_ik, L_jk, acc) for k = 0 .. j - 1 ascending;
 *      L_jj = sqrt(acc); L_ij = acc / L_jj for i > j.
 *   6. If every pivot (acc and its root) is finite and positive and every entry of L is finite, L and L^T replace [2][DP][DP], the
 *      layout of tinyda_amd_dense_mass.h, zeros outside the triangle and in the padding.  Only the lower triangle is ever formed,
 *      so the new W is symmetric by construction.
 *   7. Otherwise the WHOLE factor keeps its value and `refused` goes up by one.
 *   8. Either way S1, S2 and n are zeroed and `updates` goes up by one; with an adaptive step size k restarts at 0, as under the
 *      diagonal adaptation.  The next block's step kernel follows on the same stream and sees the new factor.
 *   (The factor is formed in a global workspace of [DP][DP] doubles, a column on consecutive addresses; thread i holds row i.)
 *
 * A dense-adapting engine's checkpoint blob also carries W and the period (checked by set_state, not adopted), n, `updates`,
 * `refused`, a, the factor [2][DP][DP], S1 and S2; every other blob is what it was.
 * Conventions as in tinyda_amd.h: TDA_OK (0) or a negative tda_status, tda_last_error() gives the message.
 */
#ifndef TINYDA_AMD_DENSE_MASS_ADAPTATION_H
#define TINYDA_AMD_DENSE_MASS_ADAPTATION_H

#include <stdint.h>

#include "tinyda_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Adapt a dense inverse mass during the first warmup_steps steps: after tda_engine_set_hmc / tda_engine_set_nuts, and after
 * tda_engine_set_dense_mass if a dense start is wanted; before tda_engine_init.  0 switches it off, and so does a later
 * tda_engine_set_proposal.  The starting mass is the dense factor if one was set, else diag(sqrt(inv_mass)) of set_hmc / set_nuts.
 * The engine builds the dense program (tinyda_amd_dense_mass.h) from the start, and its LDS refusals apply at init.
 * TDA_ERR_STATE for any other proposal kind, and on an engine that adapts a diagonal mass (tda_engine_set_mass_adaptation); after
 * it tda_engine_set_mass_adaptation and tda_engine_set_dense_mass are refused with TDA_ERR_STATE.  TDA_ERR_INVALID for a
 * warmup_steps that is negative, not a multiple of the period or shorter than two periods. */
int tda_engine_set_dense_mass_adaptation(tda_engine* e, int64_t warmup_steps);

/* The adaptation's counters of an initialised HMC / NUTS engine with a dense mass (tda_engine_get_dense_mass reads the factor
 * in force): updates applied, steps accumulated in the running window, the global step at which the next update happens
 * (-1: none), window ends refused so far. */
int tda_engine_get_dense_mass_adaptation(tda_engine* e, int64_t* info /* HOST [4] */);

/* The three kernels over given states, without an engine: one window of n steps of N chains with d parameters, folded in blocks
 * that end at cuts[0] < cuts[1] < ... (steps, each in 1 .. n - 1; none: one block), then the update.  shift: [d], or NULL: formed
 * by the shift kernel from states[0].  chol_in, chol_out: HOST [d][d], the factor before and after; *refused: 0 or 1.
 * TDA_ERR_INVALID for d outside 1 .. 128, N or n below 1, or cuts that do not ascend inside the window. */
int tda_dense_mass_window(int device, int d, int64_t N, int64_t n, const double* states /* HOST [n][N][d] */, const int64_t* cuts, int n_cuts,
                          const double* shift, const double* chol_in, double* chol_out, int64_t* refused);

#ifdef __cplusplus
}
#endif
#endif
