// Part of libtinyda_hip.so: included by tda_engine.hip.  The two entry points of include/tinyda_amd_dense_mass.h: the Cholesky
// factor of a fixed dense inverse mass of HMC / NUTS.  The kernels' side is -DTDA_DENSE_MASS in tda_user_program.hip (the
// `dense_mass` flag of tda_user_build.h, part of the build key); tda_host_init.inc uploads L and L^T and has the LDS refusals,
// tda_host_setup.inc clears the factor at set_proposal, tda_host_mass.inc refuses the warm-up adaptation beside it.
#include "tinyda_amd_dense_mass.h"

extern "C" {

int tda_engine_set_dense_mass(tda_engine* e, const double* chol) {
  if (!e) return fail(TDA_ERR_INVALID, "null engine");
  if (!e->prop_set || e->is_dreamz || !leapfrog_proposal(e->pp.kind))
    return fail(TDA_ERR_STATE, "set_proposal with kind TDA_PROP_HMC or TDA_PROP_NUTS must precede set_dense_mass");
  if (e->dmass_W > 0)
    return fail(TDA_ERR_STATE, "set_dense_mass on an engine that adapts a dense mass: tda_engine_set_dense_mass_adaptation took its starting factor when it "
                               "was called (switch it off with warmup_steps = 0 first, set the factor, and switch it on again)");
  if (chol && e->mass_W > 0)
    return fail(TDA_ERR_STATE, "set_dense_mass on an engine that adapts its mass: tda_engine_set_mass_adaptation learns a diagonal mass during warm-up "
                               "(switch it off with warmup_steps = 0 first)");
  const int d = e->d;
  for (int i = 0; chol && i < d; ++i)
    for (int j = 0; j < d; ++j) {
      const double v = chol[(size_t)i * d + j];
      if (j > i && v != 0.0) return fail(TDA_ERR_INVALID, "dense mass: chol[%d][%d] = %g lies above the diagonal and must be exactly 0 (the factor is lower triangular)", i, j, v);
      if (!std::isfinite(v)) return fail(TDA_ERR_INVALID, "dense mass: chol[%d][%d] = %g must be finite", i, j, v);
      if (j == i && !(v > 0.0)) return fail(TDA_ERR_INVALID, "dense mass: chol[%d][%d] = %g on the diagonal must be positive", i, j, v);
    }
  if (chol)
    e->dense_chol_h.assign(chol, chol + (size_t)d * d);
  else
    e->dense_chol_h.clear();
  e->inited = false;
  return TDA_OK;
}

int tda_engine_get_dense_mass(tda_engine* e, double* chol) {
  if (!e || !chol) return fail(TDA_ERR_INVALID, "null engine or destination");
  if (!e->inited || e->is_dreamz || !leapfrog_proposal(e->pp.kind) || e->dense_chol_h.empty() || !e->dense_chol.p)
    return fail(TDA_ERR_STATE, "get_dense_mass applies to an initialised HMC or NUTS engine with a dense mass (tda_engine_set_dense_mass)");
  HIP_TRY(hipSetDevice(e->cfg.device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  // the device's L, [DP][DP], without its padding
  HIP_TRY(hipMemcpy2D(chol, (size_t)e->d * sizeof(double), e->dense_chol.p, (size_t)e->DP * sizeof(double), (size_t)e->d * sizeof(double), (size_t)e->d,
                      is_device_ptr(chol) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
  return TDA_OK;
}

}  // extern "C"
