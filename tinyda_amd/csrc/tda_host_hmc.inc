// Part of libtinyda_hip.so: included by tda_engine.hip.  The one entry point of include/tinyda_amd_hmc.h: trajectory length and
// mass of the HMC proposal (tda_user_hmc_steps of tda_user_program.hip).  Everything else of HMC is a branch beside MALA's in
// tda_host_setup.inc (set_proposal), tda_host_init.inc (refusals, the program, the gradient at the initial states) and
// tda_host_single.inc (the launch of a block, the adaptation's target).
#include "tinyda_amd_hmc.h"

extern "C" {

int tda_engine_set_hmc(tda_engine* e, int32_t n_leapfrog, const double* inv_mass) {
  if (!e) return fail(TDA_ERR_INVALID, "null engine");
  if (!e->prop_set || e->is_dreamz || e->pp.kind != TDA_PROP_HMC) return fail(TDA_ERR_STATE, "set_proposal with kind TDA_PROP_HMC must precede set_hmc");
  if (n_leapfrog < 1 || n_leapfrog > 1024) return fail(TDA_ERR_INVALID, "HMC: n_leapfrog = %d outside 1 .. 1024", (int)n_leapfrog);
  if (inv_mass)
    for (int j = 0; j < e->d; ++j)
      if (!std::isfinite(inv_mass[j]) || !(inv_mass[j] > 0.0)) return fail(TDA_ERR_INVALID, "HMC: inv_mass[%d] = %g must be finite and positive", j, inv_mass[j]);
  e->hmc_n_leapfrog = n_leapfrog;
  if (inv_mass)
    e->hmc_inv_mass_h.assign(inv_mass, inv_mass + e->d);
  else
    e->hmc_inv_mass_h.clear();
  e->inited = false;
  return TDA_OK;
}

}  // extern "C"
