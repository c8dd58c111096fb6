// Part of libtinyda_hip.so: included by tda_engine.hip.  Warm-up adaptation of the diagonal inverse mass of HMC / NUTS
// (include/tinyda_amd_mass.h): the schedule of the windows, the two launches of csrc/tda_kernels_mass.h that tda_engine_run
// (tda_host_single.inc) queues behind a block's step kernel, and the two entry points.  tda_host_init.inc allocates the moments,
// tda_host_state.inc puts them into the checkpoint blob of a mass-adapting engine.
#include "tinyda_amd_mass.h"

namespace {

// the window [*first, *end) (in periods) that holds period `p`, or, if none does, the first window behind it; false: there is none
// (P = W / period: period 0 is a buffer, windows of 1, 2, 4, .. periods follow, and a window after which the next would not fit
// whole takes the rest)
bool mass_window(int64_t P, int64_t p, int64_t* first, int64_t* end) {
  for (int64_t s = 1, L = 1; s < P; s += L, L *= 2) {
    if (s + 3 * L > P) L = P - s;
    if (p < s + L) {
      *first = s;
      *end = s + L;
      return true;
    }
  }
  return false;
}

// (either kind of adaptation: the dense one, tda_host_dense_mass_adapt.inc, cuts the blocks and records the states in the same way)
inline bool mass_warming(const tda_engine* e, int64_t t) { return (e->mass_W > 0 && t < e->mass_W) || (e->dmass_W > 0 && t < e->dmass_W); }
int dense_mass_after_block(tda_engine* e, int64_t t, int64_t S, const double* rec);

// behind the step kernel of the block [t, t + S) (inside one period while the mass adapts): fold its states if it lies in a
// window, and pool the chains if the window ends with it.  rec: the block's states, [S][N][d]
int mass_after_block(tda_engine* e, int64_t t, int64_t S, const double* rec) {
  if (e->dmass_W > 0) return dense_mass_after_block(e, t, S, rec);
  const int64_t period = e->pp.period;
  int64_t first = 0, end = 0;
  if (!mass_warming(e, t) || !mass_window(e->mass_W / period, t / period, &first, &end) || t / period < first) return TDA_OK;
  if (!rec) return fail(TDA_ERR_STATE, "mass adaptation: the block's states were not recorded");
  MassAccumulateArgs aa{};
  aa.rec = rec;
  aa.mean = e->mass_mean.p;
  aa.M2 = e->mass_M2.p;
  aa.N = e->N;
  aa.d = e->d;
  aa.DP = e->DP;
  aa.S = (int)S;
  aa.n0 = e->mass_n;
  const int64_t nd = e->N * e->d;
  {
    ScopedTimer tm(e, 2);  // (tda_profile counts it under `adapt`: a NUTS engine has no other launch there)
    hipLaunchKernelGGL(k_mass_accumulate, dim3((unsigned)((nd + MASS_THREADS - 1) / MASS_THREADS)), dim3(MASS_THREADS), 0, e->stream, aa);
  }
  HIP_TRY(hipGetLastError());
  e->mass_n += S;
  if (t + S == end * period) {
    MassUpdateArgs ua{};
    ua.mean = e->mass_mean.p;
    ua.M2 = e->mass_M2.p;
    ua.inv_mass = e->hmc_inv_mass.p;
    ua.refused = e->mass_refused.p;
    ua.N = e->N;
    ua.DP = e->DP;
    ua.n = e->mass_n;
    ScopedTimer tm(e, 2);
    hipLaunchKernelGGL(k_mass_update, dim3((unsigned)e->d), dim3(MASS_THREADS), 0, e->stream, ua);
    HIP_TRY(hipGetLastError());
    e->mass_n = 0;
    e->mass_updates += 1;
    if (e->pp.adaptive) e->k_adapt = 0;  // the step-size rule's gain is full again under the new metric
  }
  return TDA_OK;
}

}  // namespace

extern "C" {

int tda_engine_set_mass_adaptation(tda_engine* e, int64_t warmup_steps) {
  if (!e) return fail(TDA_ERR_INVALID, "null engine");
  if (!e->prop_set || e->is_dreamz || !leapfrog_proposal(e->pp.kind))
    return fail(TDA_ERR_STATE, "set_proposal with kind TDA_PROP_HMC or TDA_PROP_NUTS must precede set_mass_adaptation");
  if (warmup_steps != 0 && e->dmass_W > 0)
    return fail(TDA_ERR_STATE, "set_mass_adaptation on an engine that adapts a dense mass: tda_engine_set_dense_mass_adaptation learns the whole matrix "
                               "during warm-up (switch it off with warmup_steps = 0 first)");
  if (warmup_steps != 0 && !e->dense_chol_h.empty())
    return fail(TDA_ERR_STATE, "set_mass_adaptation on an engine with a dense mass: the warm-up learns a diagonal mass, tda_engine_set_dense_mass "
                               "fixed a dense one (switch it off with chol = NULL first)");
  const int64_t period = e->pp.period;
  if (warmup_steps < 0 || warmup_steps % period != 0 || (warmup_steps != 0 && warmup_steps < 2 * period))
    return fail(TDA_ERR_INVALID, "mass adaptation: warmup_steps = %lld must be a multiple of the period (%lld) and at least two periods (or 0: off)",
                (long long)warmup_steps, (long long)period);
  e->mass_W = warmup_steps;
  e->inited = false;
  return TDA_OK;
}

int tda_engine_get_mass(tda_engine* e, double* inv_mass, int64_t* info) {
  if (!e) return fail(TDA_ERR_INVALID, "null engine");
  if (!e->inited || e->is_dreamz || !leapfrog_proposal(e->pp.kind) || !e->hmc_inv_mass.p)
    return fail(TDA_ERR_STATE, "get_mass applies to an initialised HMC or NUTS engine");
  if (!e->dense_chol_h.empty())
    return fail(TDA_ERR_STATE, "get_mass reads a diagonal mass: this engine has a dense one, which tda_engine_get_dense_mass reads");
  HIP_TRY(hipSetDevice(e->cfg.device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (inv_mass)
    HIP_TRY(hipMemcpy(inv_mass, e->hmc_inv_mass.p, (size_t)e->d * sizeof(double), is_device_ptr(inv_mass) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
  if (info) {
    unsigned int refused = 0;
    if (e->mass_refused.p) HIP_TRY(hipMemcpy(&refused, e->mass_refused.p, sizeof refused, hipMemcpyDeviceToHost));
    int64_t first = 0, end = 0;
    const bool more = mass_warming(e, e->t) && mass_window(e->mass_W / e->pp.period, e->t / e->pp.period, &first, &end);
    info[0] = e->mass_updates;
    info[1] = e->mass_n;
    info[2] = more ? end * e->pp.period : -1;
    info[3] = (int64_t)refused;
  }
  return TDA_OK;
}

}  // extern "C"
