// Part of libtinyda_hip.so: included by tda_engine.hip behind tda_host_mass.inc, whose schedule (mass_window) it shares.  Warm-up
// adaptation of the dense inverse mass of HMC / NUTS (include/tinyda_amd_dense_mass_adaptation.h): the launches of
// csrc/tda_kernels_dense_mass.h that tda_engine_run (tda_host_single.inc) queues before and behind a block's step kernel, the two
// entry points of an engine, and the stand-alone tda_dense_mass_window.  tda_host_init.inc allocates the sums, tda_host_state.inc
// puts them into the checkpoint blob of a dense-adapting engine.  The count n and `updates` are the engine's mass_n / mass_updates,
// `refused` its mass_refused: an engine adapts one kind of mass or the other.
#include "tinyda_amd_dense_mass_adaptation.h"

namespace {

int64_t dense_mass_chunks(int64_t N) { return (N + DMASS_CH - 1) / DMASS_CH; }

int launch_dense_mass_shift(const double* x, int64_t stride, double* a, int64_t N, int d, int DP, hipStream_t stream) {
  DenseMassShiftArgs sa{};
  sa.x = x;
  sa.stride = stride;
  sa.a = a;
  sa.N = N;
  sa.d = d;
  hipLaunchKernelGGL(k_dense_mass_shift, dim3((unsigned)DP), dim3(DMASS_THREADS), 0, stream, sa);
  HIP_TRY(hipGetLastError());
  return TDA_OK;
}

int launch_dense_mass_accumulate(const double* rec, const double* a, double* S1, double* S2, int64_t N, int d, int DP, int64_t S, hipStream_t stream) {
  DenseMassAccumulateArgs aa{};
  aa.rec = rec;
  aa.a = a;
  aa.S1 = S1;
  aa.S2 = S2;
  aa.N = N;
  aa.d = d;
  aa.DP = DP;
  aa.S = (int)S;
  hipLaunchKernelGGL(k_dense_mass_accumulate, dim3((unsigned)dense_mass_chunks(N)), dim3(DMASS_THREADS), 0, stream, aa);
  HIP_TRY(hipGetLastError());
  return TDA_OK;
}

int launch_dense_mass_update(double* S1, double* S2, double* work, double* chol, unsigned int* refused, int64_t N, int d, int DP, int64_t n, hipStream_t stream) {
  DenseMassUpdateArgs ua{};
  ua.S1 = S1;
  ua.S2 = S2;
  ua.work = work;
  ua.chol = chol;
  ua.refused = refused;
  ua.N = N;
  ua.NC = dense_mass_chunks(N);
  ua.d = d;
  ua.DP = DP;
  ua.n = n;
  hipLaunchKernelGGL(k_dense_mass_update, dim3(1), dim3(DMASS_THREADS), 0, stream, ua);
  HIP_TRY(hipGetLastError());
  return TDA_OK;
}

inline bool dense_mass_warming(const tda_engine* e, int64_t t) { return e->dmass_W > 0 && t < e->dmass_W; }

// before the step kernel of the block that starts at t: the shift of the window that starts there, from the chains' current states
int dense_mass_before_block(tda_engine* e, int64_t t) {
  const int64_t period = e->pp.period;
  int64_t first = 0, end = 0;
  if (!dense_mass_warming(e, t) || t % period != 0 || !mass_window(e->dmass_W / period, t / period, &first, &end) || t / period != first) return TDA_OK;
  ScopedTimer tm(e, 2);
  return launch_dense_mass_shift(e->theta.p, e->DP, e->dmass_a.p, e->N, e->d, e->DP, e->stream);
}

// behind the step kernel of the block [t, t + S) (inside one period while the mass adapts): fold its states if it lies in a
// window, and form the new factor if the window ends with it.  rec: the block's states, [S][N][d]
int dense_mass_after_block(tda_engine* e, int64_t t, int64_t S, const double* rec) {
  const int64_t period = e->pp.period;
  int64_t first = 0, end = 0;
  if (!dense_mass_warming(e, t) || !mass_window(e->dmass_W / period, t / period, &first, &end) || t / period < first) return TDA_OK;
  if (!rec) return fail(TDA_ERR_STATE, "dense mass adaptation: the block's states were not recorded");
  int rc;
  {
    ScopedTimer tm(e, 2);  // (tda_profile counts it under `adapt`, like the diagonal adaptation's launches)
    if ((rc = launch_dense_mass_accumulate(rec, e->dmass_a.p, e->dmass_S1.p, e->dmass_S2.p, e->N, e->d, e->DP, S, e->stream))) return rc;
  }
  e->mass_n += S;
  if (t + S == end * period) {
    ScopedTimer tm(e, 2);
    if ((rc = launch_dense_mass_update(e->dmass_S1.p, e->dmass_S2.p, e->dmass_work.p, e->dense_chol.p, e->mass_refused.p, e->N, e->d, e->DP, e->mass_n, e->stream)))
      return rc;
    e->mass_n = 0;
    e->mass_updates += 1;
    if (e->pp.adaptive) e->k_adapt = 0;  // the step-size rule's gain is full again under the new metric
  }
  return TDA_OK;
}

}  // namespace

extern "C" {

int tda_engine_set_dense_mass_adaptation(tda_engine* e, int64_t warmup_steps) {
  if (!e) return fail(TDA_ERR_INVALID, "null engine");
  if (!e->prop_set || e->is_dreamz || !leapfrog_proposal(e->pp.kind))
    return fail(TDA_ERR_STATE, "set_proposal with kind TDA_PROP_HMC or TDA_PROP_NUTS must precede set_dense_mass_adaptation");
  if (warmup_steps != 0 && e->mass_W > 0)
    return fail(TDA_ERR_STATE, "set_dense_mass_adaptation on an engine that adapts a diagonal mass: tda_engine_set_mass_adaptation learns the variances "
                               "during warm-up (switch it off with warmup_steps = 0 first)");
  const int64_t period = e->pp.period;
  if (warmup_steps < 0 || warmup_steps % period != 0 || (warmup_steps != 0 && warmup_steps < 2 * period))
    return fail(TDA_ERR_INVALID, "dense mass adaptation: warmup_steps = %lld must be a multiple of the period (%lld) and at least two periods (or 0: off)",
                (long long)warmup_steps, (long long)period);
  const int d = e->d;
  if (warmup_steps != 0 && e->dense_chol_h.empty()) {  // no dense start: diag(sqrt(inv_mass)) of set_hmc / set_nuts
    e->dense_chol_h.assign((size_t)d * d, 0.0);
    for (int j = 0; j < d; ++j) e->dense_chol_h[(size_t)j * d + j] = e->hmc_inv_mass_h.empty() ? 1.0 : std::sqrt(e->hmc_inv_mass_h[j]);
    e->dmass_own_start = true;
  } else if (warmup_steps == 0 && e->dmass_own_start) {
    e->dense_chol_h.clear();
    e->dmass_own_start = false;
  }
  e->dmass_W = warmup_steps;
  e->inited = false;
  return TDA_OK;
}

int tda_engine_get_dense_mass_adaptation(tda_engine* e, int64_t* info) {
  if (!e || !info) return fail(TDA_ERR_INVALID, "null engine or destination");
  if (!e->inited || e->is_dreamz || !leapfrog_proposal(e->pp.kind) || e->dense_chol_h.empty() || !e->dense_chol.p)
    return fail(TDA_ERR_STATE, "get_dense_mass_adaptation applies to an initialised HMC or NUTS engine with a dense mass");
  HIP_TRY(hipSetDevice(e->cfg.device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  unsigned int refused = 0;
  if (e->dmass_W > 0 && e->mass_refused.p) HIP_TRY(hipMemcpy(&refused, e->mass_refused.p, sizeof refused, hipMemcpyDeviceToHost));
  int64_t first = 0, end = 0;
  const bool more = dense_mass_warming(e, e->t) && mass_window(e->dmass_W / e->pp.period, e->t / e->pp.period, &first, &end);
  info[0] = e->dmass_W > 0 ? e->mass_updates : 0;
  info[1] = e->dmass_W > 0 ? e->mass_n : 0;
  info[2] = more ? end * e->pp.period : -1;
  info[3] = (int64_t)refused;
  return TDA_OK;
}

int tda_dense_mass_window(int device, int d, int64_t N, int64_t n, const double* states, const int64_t* cuts, int n_cuts, const double* shift,
                          const double* chol_in, double* chol_out, int64_t* refused) {
  if (!states || !chol_in || !chol_out || !refused || (n_cuts > 0 && !cuts)) return fail(TDA_ERR_INVALID, "null argument");
  if (d < 1 || d > 128 || N < 1 || n < 1 || n_cuts < 0) return fail(TDA_ERR_INVALID, "dense mass window: d = %d must lie in 1 .. 128, N = %lld and n = %lld be at least 1", d, (long long)N, (long long)n);
  if (n > INT32_MAX || (uint64_t)dense_mass_chunks(N) > (uint64_t)INT32_MAX) return fail(TDA_ERR_INVALID, "dense mass window: too many steps or chains for one launch");
  for (int i = 0; i < n_cuts; ++i)
    if (cuts[i] < 1 || cuts[i] >= n || (i > 0 && cuts[i] <= cuts[i - 1]))
      return fail(TDA_ERR_INVALID, "dense mass window: cuts[%d] = %lld must ascend inside 1 .. n - 1 = %lld", i, (long long)cuts[i], (long long)(n - 1));
  HIP_TRY(hipSetDevice(device));
  const int DP = dpad_for(d);
  const int64_t NC = dense_mass_chunks(N);
  const size_t nd = (size_t)N * d;
  DevBuf<double> x, a, S1, S2, work, chol;
  DevBuf<unsigned int> ref;
  int rc;
  if ((rc = x.upload(std::vector<double>(states, states + (size_t)n * nd)))) return rc;
  std::vector<double> ah(DP, 0.0), LL(2 * (size_t)DP * DP, 0.0);
  for (int j = 0; j < d && shift; ++j) ah[j] = shift[j];
  for (int i = 0; i < d; ++i)
    for (int j = 0; j <= i; ++j) {
      LL[(size_t)i * DP + j] = chol_in[(size_t)i * d + j];
      LL[(size_t)DP * DP + (size_t)j * DP + i] = chol_in[(size_t)i * d + j];
    }
  if ((rc = a.upload(ah)) || (rc = chol.upload(LL)) || (rc = S1.alloc((size_t)NC * DP)) || (rc = S2.alloc((size_t)NC * dmass_s2_doubles(DP))) ||
      (rc = work.alloc((size_t)DP * DP)) || (rc = ref.alloc(1)))
    return rc;
  HIP_TRY(hipMemset(S1.p, 0, S1.n * sizeof(double)));
  HIP_TRY(hipMemset(S2.p, 0, S2.n * sizeof(double)));
  HIP_TRY(hipMemset(work.p, 0, work.n * sizeof(double)));
  HIP_TRY(hipMemset(ref.p, 0, sizeof(unsigned int)));
  if (!shift && (rc = launch_dense_mass_shift(x.p, d, a.p, N, d, DP, nullptr))) return rc;
  for (int64_t lo = 0, i = 0; lo < n; ++i) {
    const int64_t hi = i < n_cuts ? cuts[i] : n;
    if ((rc = launch_dense_mass_accumulate(x.p + (size_t)lo * nd, a.p, S1.p, S2.p, N, d, DP, hi - lo, nullptr))) return rc;
    lo = hi;
  }
  if ((rc = launch_dense_mass_update(S1.p, S2.p, work.p, chol.p, ref.p, N, d, DP, n, nullptr))) return rc;
  HIP_TRY(hipDeviceSynchronize());
  unsigned int r = 0;
  HIP_TRY(hipMemcpy(&r, ref.p, sizeof r, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy2D(chol_out, (size_t)d * sizeof(double), chol.p, (size_t)DP * sizeof(double), (size_t)d * sizeof(double), (size_t)d, hipMemcpyDeviceToHost));
  *refused = (int64_t)r;
  return TDA_OK;
}

}  // extern "C"
