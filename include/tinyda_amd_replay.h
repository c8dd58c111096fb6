/*
 * tinyda_amd_replay.h  --  model outputs and quantities of interest of recorded parameters (libtinyda_hip.so).
 *
 * The reference's Link carries `model_output` and `qoi` beside the parameters (tinyDA/link.py:23-48), evaluated at every
 * proposal (posterior.py:95-101).  The engine records parameters and log-densities only; a forward model is deterministic, so
 * the outputs and the quantities of every recorded row are produced AFTER the run, and only when somebody asks, by replaying the
 * model over the records.  The replay needs no tda_engine (a result outlives its engine): it is an object of its own, compiled
 * once from the model's HIP source (the source of tda_engine_set_level_source) and run over any number of chunks of records.
 *
 * The source may define a quantity of interest in one of two forms (the wave form is used when both are there):
 *   __device__ double tda_qoi(const double* theta, int dim, const double* f, int n_outputs, int k);
 *       quantity k of n_qoi; f: the model's complete outputs at theta (LDS); the lanes stride over k
 *   __device__ void tda_qoi_wave(const double* theta, int dim, const double* f, int n_outputs, double* qoi, int n_qoi, double* work, int lane);
 *       all quantities in one call by the chain's 64 lanes (converged call site; __syncthreads() legal: one wave per workgroup);
 *       qoi: LDS, n_qoi doubles, NaN before the call (an entry left unwritten stays NaN); work: what tda_forward_wave left at the
 *       same theta (null without TDA_WORKSPACE)
 * A NaN quantity is data, not a rejection.  LDS per workgroup: 8 (n_outputs + n_qoi + 128 + TDA_WORKSPACE) bytes, at most 64 KiB.
 *
 * Conventions as in tinyda_amd.h: TDA_OK (0) or a negative tda_status, tda_last_error() gives the message.
 */
#ifndef TINYDA_AMD_REPLAY_H
#define TINYDA_AMD_REPLAY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tda_replay tda_replay;

/* compile the replay program of `source` for models of `dim` parameters (1..128), n_outputs >= 1 outputs and n_qoi >= 0 quantities
 * of interest.  n_qoi > 0 needs one of the two functions in the source, n_qoi == 0 a source without them. */
int tda_replay_create(int device, const char* source, int32_t dim, int32_t n_outputs, int32_t n_qoi, tda_replay** out);

/* outputs[r][c][:] = F(params[r][c][:]) and qoi[r][c][:] for rows r < rows of n_chains chains (device memory, row-major fp64).
 * One wave per chain and segment of segment_rows rows (0: chosen by the library) walks its rows in order and evaluates the model
 * only where a row's parameters differ bit for bit from the previous row's, or at the start of a segment; the results do not
 * depend on segment_rows.  Either destination may be null, but not both; `qoi` must be null when n_qoi == 0.  n_evaluated (host,
 * optional) receives the number of model evaluations; asking for it synchronises `stream`. */
int tda_replay_run(tda_replay* r, const double* params, int64_t rows, int64_t n_chains, int64_t segment_rows, double* outputs,
                   double* qoi, int64_t* n_evaluated, void* stream);

void tda_replay_destroy(tda_replay* r);

#ifdef __cplusplus
}
#endif
#endif
