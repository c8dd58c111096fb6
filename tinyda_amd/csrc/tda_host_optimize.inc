// Modes of a source-defined posterior (include/tinyda_amd_optimize.h; included by tda_engine.hip): the host side of
// tda_user_maximize.  No tda_engine and no proposal: like the replay, the optimiser is a small object of its own -- one compiled
// program (compile_user_program, the one hiprtc call site) and the device copies of what the posterior is made of.
#include "tinyda_amd_optimize.h"

struct tda_optimizer {
  int device = 0, d = 0, m = 0;
  UserProgram prog;
  double var = 1.0, logconst = 0.0;
  double* dev = nullptr;  // one allocation: data [m], w [m], pr_mean [d], pr_pinv [d], pr_lo [d], pr_hi [d]
  bool has_w = false, bounded = false;
};

extern "C" {

int tda_optimizer_create(int device, const char* source, const tda_optimize_problem* p, tda_optimizer** out) {
  if (!source || !p || !out) return fail(TDA_ERR_INVALID, "null argument");
  if (p->struct_size != sizeof(tda_optimize_problem)) return fail(TDA_ERR_INVALID, "tda_optimize_problem: struct_size %u, expected %zu", p->struct_size, sizeof(tda_optimize_problem));
  if (!p->data || !p->noise || !p->prior_kind || !p->prior_loc || !p->prior_scale) return fail(TDA_ERR_INVALID, "null argument in tda_optimize_problem");
  const int d = p->dim, m = p->n_outputs;
  if (d < 1 || d > 128) return fail(TDA_ERR_UNSUPPORTED, "dim=%d outside the device engine's range 1..128", d);
  if (m < 1) return fail(TDA_ERR_INVALID, "n_outputs must be >= 1");
  if (p->noise_kind != TDA_NOISE_ISO && p->noise_kind != TDA_NOISE_DIAG && p->noise_kind != TDA_NOISE_SOURCE)
    return fail(TDA_ERR_UNSUPPORTED, "the optimiser takes isotropic / diagonal noise or a source-defined likelihood (noise kind %d)", (int)p->noise_kind);
  const UserForms forms = user_forms(source);
  if (!forms.forward_wave && !source_defines(source, "tda_forward"))
    return fail(TDA_ERR_INVALID, "the source defines neither tda_forward nor %s", TDA_SIG_FORWARD_WAVE);
  if (forms.both_prior_forms())
    return fail(TDA_ERR_INVALID, "a source-defined prior: the source defines both tda_logprior_term and tda_logprior_wave (a prior has one form)");
  if (forms.both_loglike_forms())
    return fail(TDA_ERR_INVALID, "a source-defined likelihood: the source defines both tda_loglike_term and tda_loglike_wave (a likelihood has one form)");
  // the posterior's arrays as the kernels of tda_user_program.hip take them (tda_engine_set_level_source, tda_engine_set_prior_joint)
  std::vector<double> h((size_t)2 * m + (size_t)4 * d, 0.0);
  double *y = h.data(), *w = y + m, *pm = w + m, *pinv = pm + d, *lo = pinv + d, *hi = lo + d;
  double var = 1.0, logconst = 0.0;
  bool bounded = false;
  for (int i = 0; i < m; ++i) y[i] = p->data[i];
  if (p->noise_kind == TDA_NOISE_ISO) {
    if (!(p->noise[0] > 0.0)) return fail(TDA_ERR_NUMERIC, "noise variance must be positive");
    var = p->noise[0];
  } else {
    for (int i = 0; i < m; ++i) {
      if (p->noise_kind == TDA_NOISE_DIAG && !(p->noise[i] > 0.0)) return fail(TDA_ERR_NUMERIC, "noise variance must be positive");
      w[i] = p->noise_kind == TDA_NOISE_DIAG ? 1.0 / p->noise[i] : p->noise[i];
    }
  }
  int n_source = 0;
  for (int j = 0; j < d; ++j) n_source += p->prior_kind[j] == TDA_PRIOR_SOURCE ? 1 : 0;
  if (n_source && n_source != d)
    return fail(TDA_ERR_UNSUPPORTED, "prior components are either all source-defined (kind %d) or all normal / uniform", (int)TDA_PRIOR_SOURCE);
  for (int j = 0; j < d; ++j) {
    const double loc = p->prior_loc[j], scale = p->prior_scale[j];
    lo[j] = -INFINITY, hi[j] = INFINITY;
    if (n_source) {
      if (!std::isfinite(loc) || !std::isfinite(scale)) return fail(TDA_ERR_NUMERIC, "prior component %d: p and q must be finite", j);
      pm[j] = loc, pinv[j] = scale;
    } else if (!(scale > 0.0)) {
      return fail(TDA_ERR_NUMERIC, "prior component %d: scale must be positive", j);
    } else if (p->prior_kind[j] == TDA_PRIOR_NORMAL) {
      pm[j] = loc, pinv[j] = 1.0 / (scale * scale);
      logconst += std::log(2.0 * M_PI) + 2.0 * std::log(scale);
    } else if (p->prior_kind[j] == TDA_PRIOR_UNIFORM) {
      lo[j] = loc, hi[j] = loc + scale;
      logconst += 2.0 * std::log(scale);
      bounded = true;
    } else {
      return fail(TDA_ERR_UNSUPPORTED, "prior component %d: kind %d (0 = normal, 1 = uniform, 2 = source-defined)", j, (int)p->prior_kind[j]);
    }
  }
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (ndev < 1) return fail(TDA_ERR_HIP, "no HIP device visible: the optimiser has no CPU fallback");
  if (device < 0 || device >= ndev) return fail(TDA_ERR_INVALID, "device %d of %d", device, ndev);
  HIP_TRY(hipSetDevice(device));
  UserProgramSpec spec;
  spec.map = true;
  spec.mala = p->use_source_gradient != 0;
  spec.loglike_source = p->noise_kind == TDA_NOISE_SOURCE;
  spec.loglike_wave = spec.loglike_source && forms.loglike_wave;
  spec.prior_form = !n_source ? 0 : forms.prior_wave ? 2 : 1;
  spec.forward_wave = forms.forward_wave;
  spec.gradient_wave = spec.mala && forms.gradient_wave;
  tda_optimizer* o = new tda_optimizer();
  o->device = device, o->d = d, o->m = m, o->var = var, o->logconst = logconst;
  o->has_w = p->noise_kind != TDA_NOISE_ISO, o->bounded = bounded;
  int rc = compile_user_program(source, spec, m, &o->prog);
  if (rc == TDA_OK) {
    hipError_t er = hipMalloc((void**)&o->dev, h.size() * sizeof(double));
    if (er == hipSuccess) er = hipMemcpy(o->dev, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice);
    if (er != hipSuccess) rc = fail(TDA_ERR_HIP, "tda_optimizer_create: %s", hipGetErrorString(er));
  }
  if (rc != TDA_OK) {
    o->prog.unload();
    if (o->dev) (void)hipFree(o->dev);
    delete o;
    return rc;
  }
  *out = o;
  return TDA_OK;
}

int tda_optimizer_run(tda_optimizer* o, const double* starts, int64_t n, int32_t objective, const tda_optimize_options* opt, double* x, double* stats,
                      int32_t* status, void* stream) {
  if (!o || !starts || !opt || !x || !stats || !status) return fail(TDA_ERR_INVALID, "null argument");
  if (opt->struct_size != sizeof(tda_optimize_options)) return fail(TDA_ERR_INVALID, "tda_optimize_options: struct_size %u, expected %zu", opt->struct_size, sizeof(tda_optimize_options));
  if (n < 1 || n > (1ll << 30)) return fail(TDA_ERR_INVALID, "the number of starts must be in 1 .. 2^30");
  if (objective != TDA_OBJECTIVE_POSTERIOR && objective != TDA_OBJECTIVE_LIKELIHOOD) return fail(TDA_ERR_INVALID, "objective %d (0 = posterior, 1 = likelihood)", (int)objective);
  if (opt->max_iter < 0 || !(opt->gtol >= 0.0) || !(opt->ftol >= 0.0)) return fail(TDA_ERR_INVALID, "max_iter, gtol and ftol must be >= 0");
  if (!is_device_ptr(starts) || !is_device_ptr(x) || !is_device_ptr(stats) || !is_device_ptr(status))
    return fail(TDA_ERR_INVALID, "starts, x, stats and status must be device pointers");
  HIP_TRY(hipSetDevice(o->device));
  UserMapArgs a{};
  a.N = n, a.d = o->d, a.m = o->m, a.objective = objective, a.max_iter = opt->max_iter;
  a.gtol = opt->gtol, a.ftol = opt->ftol;
  a.x0 = starts;
  a.data = o->dev;
  a.w = o->has_w ? o->dev + o->m : nullptr;
  a.var = o->var;
  a.pr_mean = o->dev + 2 * (size_t)o->m;
  a.pr_pinv = a.pr_mean + o->d;
  a.pr_lo = o->bounded ? a.pr_pinv + o->d : nullptr;
  a.pr_hi = o->bounded ? a.pr_pinv + 2 * o->d : nullptr;
  a.logconst = o->logconst;
  a.x = x, a.stats = stats, a.status = status;
  return launch_user(o->prog.maximize, a, o->prog.out_lds, (hipStream_t)stream);
}

void tda_optimizer_destroy(tda_optimizer* o) {
  if (!o) return;
  (void)hipSetDevice(o->device);
  (void)hipDeviceSynchronize();
  o->prog.unload();
  if (o->dev) (void)hipFree(o->dev);
  delete o;
}

}  // extern "C"
