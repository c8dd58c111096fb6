// Part of libtinyda_hip.so: included by tda_engine.hip.  The entry points of include/tinyda_amd_nuts.h: depth, adaptation
// target and mass of the NUTS proposal (tda_user_nuts_steps of tda_user_program.hip) and the read-out of its per-chain totals.
// Everything else of NUTS is a branch beside HMC's in tda_host_setup.inc (set_proposal), tda_host_init.inc (refusals, the
// program and its LDS, the gradient at the initial states, the per-chain sums) and tda_host_single.inc (the launch of a block,
// which adapts the step size itself at a period boundary); tda_host_state.inc puts the sums into the checkpoint blob.
#include "tinyda_amd_nuts.h"

extern "C" {

int tda_engine_set_nuts(tda_engine* e, int32_t max_depth, double target_accept, const double* inv_mass) {
  if (!e) return fail(TDA_ERR_INVALID, "null engine");
  if (!e->prop_set || e->is_dreamz || e->pp.kind != TDA_PROP_NUTS) return fail(TDA_ERR_STATE, "set_proposal with kind TDA_PROP_NUTS must precede set_nuts");
  if (max_depth < 1 || max_depth > TDA_NUTS_MAX_DEPTH) return fail(TDA_ERR_INVALID, "NUTS: max_depth = %d outside 1 .. %d", (int)max_depth, (int)TDA_NUTS_MAX_DEPTH);
  if (!(target_accept > 0.0 && target_accept < 1.0)) return fail(TDA_ERR_INVALID, "NUTS: target_accept = %g outside (0, 1)", target_accept);
  if (inv_mass)
    for (int j = 0; j < e->d; ++j)
      if (!std::isfinite(inv_mass[j]) || !(inv_mass[j] > 0.0)) return fail(TDA_ERR_INVALID, "NUTS: inv_mass[%d] = %g must be finite and positive", j, inv_mass[j]);
  e->nuts_max_depth = max_depth;
  e->nuts_target = target_accept;
  if (inv_mass)
    e->hmc_inv_mass_h.assign(inv_mass, inv_mass + e->d);
  else
    e->hmc_inv_mass_h.clear();
  e->inited = false;
  return TDA_OK;
}

int tda_engine_get_nuts_totals(tda_engine* e, int64_t* totals) {
  if (!e || !totals) return fail(TDA_ERR_INVALID, "null argument");
  if (!e->inited || e->is_dreamz || e->pp.kind != TDA_PROP_NUTS) return fail(TDA_ERR_STATE, "get_nuts_totals applies to an initialised NUTS engine");
  HIP_TRY(hipSetDevice(e->cfg.device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  // (the rows of the N chains are the first N of the NP padded ones; a device destination keeps the numbers in HBM until somebody reads them)
  HIP_TRY(hipMemcpy(totals, e->nuts_totals.p, (size_t)e->N * TDA_NUTS_TOTALS * sizeof(long long), is_device_ptr(totals) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
  return TDA_OK;
}

}  // extern "C"
