// Part of libtinyda_hip.so: included by tda_engine.hip (ONE translation unit -- the helpers, the engine struct and the kernel
// launchers above it are visible here).  The problem: prior, levels (linear / Rosenbrock / HIP source / host callback), Gaussian proposals.
extern "C" {

int tda_engine_set_prior(tda_engine* e, const double* mean, const double* cov) {
  if (!e || !mean || !cov) return fail(TDA_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(e->cfg.device));
  const int d = e->d, DP = e->DP;
  e->prior_mean_h.assign(mean, mean + d);
  e->prior_cov_h.assign(cov, cov + (size_t)d * d);
  if (!cholesky_host(cov, d, e->prior_L_h))
    return fail(TDA_ERR_NUMERIC, "prior covariance is not positive definite");
  double logdet = 0.0;
  for (int j = 0; j < d; ++j) logdet += 2.0 * std::log(e->prior_L_h[(size_t)j * d + j]);
  bool diag = true;
  for (int i = 0; i < d && diag; ++i)
    for (int j = 0; j < d; ++j)
      if (i != j && cov[(size_t)i * d + j] != 0.0) {
        diag = false;
        break;
      }
  std::vector<double> mh(DP, 0.0), ph(DP, 0.0);
  for (int j = 0; j < d; ++j) mh[j] = mean[j];
  int rc;
  if ((rc = e->prior_mean.upload(mh))) return rc;
  if (diag) {
    e->prior_kind = PRIOR_DIAG;
    logdet = 0.0;
    bool standard = true;
    for (int j = 0; j < d; ++j) {
      ph[j] = 1.0 / cov[(size_t)j * d + j];
      logdet += std::log(cov[(size_t)j * d + j]);
      standard = standard && cov[(size_t)j * d + j] == 1.0 && mean[j] == 0.0;
    }
    e->prior_is_standard = standard;
    e->prior_ncb = 0;
  } else {
    e->prior_kind = PRIOR_DENSE;
    std::vector<double> W, Wpk;
    tri_inverse_host(e->prior_L_h, d, W);
    pack_fragments(W.data(), d, d, DP, Wpk, e->prior_ncb);
    std::vector<double> wmu((size_t)e->prior_ncb * 16, 0.0);
    for (int i = 0; i < d; ++i) {
      double s = 0.0;
      for (int j = 0; j < d; ++j) s += W[(size_t)i * d + j] * mean[j];
      wmu[i] = s;
    }
    if ((rc = e->prior_Wpk.upload(Wpk))) return rc;
    if ((rc = e->prior_wmu.upload(wmu))) return rc;
  }
  if ((rc = e->prior_pinv.upload(ph))) return rc;
  e->prior_logconst = d * std::log(2.0 * M_PI) + logdet;
  e->prior_bounded = false;
  e->prior_joint = false;
  e->prior_source = false;
  e->prior_set = true;
  return TDA_OK;
}

int tda_engine_set_prior_joint(tda_engine* e, const int32_t* kind, const double* loc, const double* scale) {
  if (!e || !kind || !loc || !scale) return fail(TDA_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(e->cfg.device));
  const int d = e->d, DP = e->DP;
  std::vector<double> mh(DP, 0.0), ph(DP, 0.0), lo(DP, -INFINITY), hi(DP, INFINITY);
  e->prior_mean_h.assign(d, 0.0);
  e->prior_cov_h.assign((size_t)d * d, 0.0);
  e->prior_L_h.assign((size_t)d * d, 0.0);
  double logconst = 0.0;
  bool bounded = false;
  int n_source = 0;
  for (int j = 0; j < d; ++j) n_source += kind[j] == TDA_PRIOR_SOURCE ? 1 : 0;
  if (n_source && n_source != d)
    return fail(TDA_ERR_UNSUPPORTED, "prior components are either all source-defined (kind %d) or all normal / uniform", (int)TDA_PRIOR_SOURCE);
  for (int j = 0; j < d; ++j) {
    if (n_source) {
      // tda_logprior_term(theta_j, p_j, q_j, j) of the levels' sources: p = loc, q = scale, passed on as given.  The host-side
      // moments are placeholders (standard normal): every route that reads them is refused at tda_engine_init.
      if (!std::isfinite(loc[j]) || !std::isfinite(scale[j])) return fail(TDA_ERR_NUMERIC, "prior component %d: p and q must be finite", j);
      mh[j] = loc[j];
      ph[j] = scale[j];
      e->prior_cov_h[(size_t)j * d + j] = 1.0;
      e->prior_L_h[(size_t)j * d + j] = 1.0;
      continue;
    }
    if (!(scale[j] > 0.0)) return fail(TDA_ERR_NUMERIC, "prior component %d: scale must be positive", j);
    if (kind[j] == 0) {  // scipy.stats.norm(loc, scale)
      mh[j] = loc[j];
      ph[j] = 1.0 / (scale[j] * scale[j]);
      logconst += std::log(2.0 * M_PI) + 2.0 * std::log(scale[j]);
      e->prior_mean_h[j] = loc[j];
      e->prior_cov_h[(size_t)j * d + j] = scale[j] * scale[j];
      e->prior_L_h[(size_t)j * d + j] = scale[j];
    } else if (kind[j] == 1) {  // scipy.stats.uniform(loc, scale): density 1/scale on [loc, loc + scale]
      lo[j] = loc[j];
      hi[j] = loc[j] + scale[j];
      logconst += 2.0 * std::log(scale[j]);
      bounded = true;
      e->prior_mean_h[j] = loc[j] + 0.5 * scale[j];
      e->prior_cov_h[(size_t)j * d + j] = scale[j] * scale[j] / 12.0;
      e->prior_L_h[(size_t)j * d + j] = scale[j] / std::sqrt(12.0);
    } else {
      return fail(TDA_ERR_UNSUPPORTED, "prior component %d: kind %d (0 = normal, 1 = uniform, 2 = source-defined)", j, (int)kind[j]);
    }
  }
  int rc;
  if ((rc = e->prior_mean.upload(mh)) || (rc = e->prior_pinv.upload(ph)) || (rc = e->prior_lo.upload(lo)) || (rc = e->prior_hi.upload(hi)))
    return rc;
  e->prior_kind = PRIOR_DIAG;
  e->prior_is_standard = false;
  e->prior_ncb = 0;
  e->prior_logconst = logconst;
  e->prior_bounded = bounded;
  e->prior_joint = true;
  e->prior_source = n_source != 0;
  e->prior_set = true;
  return TDA_OK;
}

int tda_engine_set_level(tda_engine* e, int level, int m, const double* A, const double* b, const double* data,
                         int noise_kind, const double* noise) {
  if (!e || !A || !data || !noise) return fail(TDA_ERR_INVALID, "null argument");
  if (level < 0 || level >= (int)e->levels.size()) return fail(TDA_ERR_INVALID, "level %d out of range", level);
  if (m < 1) return fail(TDA_ERR_INVALID, "m must be >= 1");
  HIP_TRY(hipSetDevice(e->cfg.device));
  Level& lv = e->levels[level];
  if (noise_kind == TDA_NOISE_SOURCE)
    return fail(TDA_ERR_UNSUPPORTED, "a source-defined likelihood (TDA_NOISE_SOURCE) needs a source-defined forward model (tda_engine_set_level_source)");
  if (noise_kind < TDA_NOISE_ISO || noise_kind > TDA_NOISE_ADAPTIVE) return fail(TDA_ERR_INVALID, "noise_kind %d", noise_kind);
  if (noise_kind == TDA_NOISE_ADAPTIVE && m > AEM_MP_MAX)
    return fail(TDA_ERR_UNSUPPORTED, "AdaptiveGaussianLogLike on the device is limited to m <= %d observations (per-chain m x m state)", (int)AEM_MP_MAX);
  // row stride of this level's error-model copies (65 .. 128 parameters: at least 128 -- k_aem_action maps a parameter to a thread, too)
  const int AEM_MP = (m <= 64 && e->DP <= 64) ? 64 : (m <= 128 ? 128 : 256);
  // (dense noise covariance: single-level chains, and since round 4 any level of a hierarchy of linear levels -- k_ml_steps)
  std::vector<double> Apk;
  pack_fragments(A, m, e->d, e->DP, Apk, lv.ncb);
  lv.m = m;
  lv.m_pad = lv.ncb * 16;
  lv.noise_kind = noise_kind;
  std::vector<double> yt(lv.m_pad, 0.0), w;
  for (int i = 0; i < m; ++i) yt[i] = data[i] - (b ? b[i] : 0.0);
  // row-major copies (error-model kernel)
  lv.A_h.assign(A, A + (size_t)m * e->d);
  lv.ytil_h.assign(AEM_MP > m ? AEM_MP : m, 0.0);
  lv.data_h.assign(AEM_MP > m ? AEM_MP : m, 0.0);
  for (int i = 0; i < m; ++i) {
    lv.ytil_h[i] = data[i] - (b ? b[i] : 0.0);
    lv.data_h[i] = data[i];
  }
  lv.cov_h.clear();
  std::vector<double> Ppk;
  if (noise_kind == TDA_NOISE_ADAPTIVE) {
    std::vector<double> Lc;
    if (!cholesky_host(noise, m, Lc)) return fail(TDA_ERR_NUMERIC, "noise covariance is not positive definite");
    lv.cov_h.assign(noise, noise + (size_t)m * m);
    lv.var = 1.0;
  } else if (noise_kind == TDA_NOISE_DENSE) {
    // Sigma^-1 (distributions.py:280) through the Cholesky factor: P = L^-T L^-1, symmetric by construction
    std::vector<double> Lc, W;
    if (!cholesky_host(noise, m, Lc)) return fail(TDA_ERR_NUMERIC, "noise covariance is not positive definite");
    tri_inverse_host(Lc, m, W);
    std::vector<double> P((size_t)m * m, 0.0);
    for (int i = 0; i < m; ++i)
      for (int j = 0; j <= i; ++j) {
        double s = 0.0;
        for (int k = i; k < m; ++k) s += W[(size_t)k * m + i] * W[(size_t)k * m + j];
        P[(size_t)i * m + j] = P[(size_t)j * m + i] = s;
      }
    int ncb2 = 0;
    pack_fragments(P.data(), m, m, lv.m_pad, Ppk, ncb2);
    lv.Pinv_h = P;
    lv.var = 1.0;
  } else if (noise_kind == TDA_NOISE_ISO) {
    if (!(noise[0] > 0.0)) return fail(TDA_ERR_NUMERIC, "noise variance must be positive");
    lv.var = noise[0];
  } else {
    w.assign(lv.m_pad, 0.0);
    for (int i = 0; i < m; ++i) {
      if (!(noise[i] > 0.0)) return fail(TDA_ERR_NUMERIC, "noise variance must be positive");
      w[i] = 1.0 / noise[i];
    }
    lv.w_h.assign(w.begin(), w.begin() + m);
    lv.var = 1.0;
  }
  const size_t lds = ((size_t)16 * (e->DP + 2) + 256 + 2 * e->DP + (size_t)lv.m_pad * 2 + 64 +
                      (noise_kind == TDA_NOISE_DENSE ? (size_t)16 * (lv.m_pad + 2) : 0)) * sizeof(double);
  if (lds > 158 * 1024) return fail(TDA_ERR_UNSUPPORTED, "m=%d observations exceed the LDS staging budget", m);
  int rc;
  lv.em_ld = m <= AEM_MP_MAX ? AEM_MP : 0;
  if (m <= AEM_MP_MAX) {
    std::vector<double> y64(lv.ytil_h.begin(), lv.ytil_h.begin() + AEM_MP), c64;
    {  // column-major [d][AEM_MP] for k_aem_action: lane = observation reads consecutive addresses
      std::vector<double> acm((size_t)e->d * AEM_MP, 0.0);
      for (int i = 0; i < m; ++i)
        for (int j = 0; j < e->d; ++j) acm[(size_t)j * AEM_MP + i] = lv.A_h[(size_t)i * e->d + j];
      if ((rc = lv.A_rm.upload(acm))) return rc;
    }
    if ((rc = lv.ytil64.upload(y64))) return rc;
    std::vector<double> d64(lv.data_h.begin(), lv.data_h.begin() + AEM_MP);
    if ((rc = lv.data64.upload(d64))) return rc;
    if (!lv.cov_h.empty()) {
      // Sigma_e as the UPPER 16 x 16 tiles k_aem_refresh factors (tda_kernels_aemr.h), identity in the padding rows / columns
      c64.assign(aemr_v_doubles(AEM_MP), 0.0);
      for (int i = 0; i < AEM_MP; ++i)
        for (int j = i; j < AEM_MP; ++j)
          c64[aemr_u_offset(AEM_MP, i, j)] = (i < m && j < m) ? lv.cov_h[(size_t)i * m + j] : (i == j ? 1.0 : 0.0);
      if ((rc = lv.cov64.upload(c64))) return rc;
    }
  }
  if (e->nlev > 1 && noise_kind != TDA_NOISE_DENSE) {
    // a linear level may sit in a hierarchy with callback / source-defined levels, which is sequenced by the host: the
    // level kernels of that mode take model outputs, residual data and weights from these buffers
    std::vector<double> yd(lv.data_h.begin(), lv.data_h.begin() + m), bd(m, 0.0);
    for (int i = 0; i < m; ++i) bd[i] = b ? b[i] : 0.0;
    if ((rc = lv.A_dev.upload(lv.A_h))) return rc;
    if ((rc = lv.b_dev.upload(bd))) return rc;
    if ((rc = lv.udata.upload(yd))) return rc;
    if (noise_kind == TDA_NOISE_DIAG) {
      std::vector<double> wd(w.begin(), w.begin() + m);
      if ((rc = lv.uw.upload(wd))) return rc;
    }
    if ((rc = lv.cb_prop.alloc((size_t)e->N * e->d))) return rc;
    if ((rc = lv.cb_F.alloc((size_t)e->N * m))) return rc;
  }
  if ((rc = lv.Ppk.upload(Ppk))) return rc;
  if ((rc = lv.Apk.upload(Apk))) return rc;
  if ((rc = lv.ytil.upload(yt))) return rc;
  if ((rc = lv.w.upload(w))) return rc;
  lv.set = true;
  return TDA_OK;
}

int tda_engine_set_proposal(tda_engine* e, const tda_proposal_params* p) {
  if (!e || !p) return fail(TDA_ERR_INVALID, "null argument");
  if (p->struct_size != sizeof(tda_proposal_params)) return fail(TDA_ERR_INVALID, "tda_proposal_params.struct_size mismatch");
  const bool indep = p->kind == TDA_PROP_INDEPENDENCE, owcn = p->kind == TDA_PROP_OWCN, mala = gradient_proposal(p->kind);
  const char* const gname = gradient_proposal_name(p->kind);
  if ((p->kind < TDA_PROP_GRW || p->kind > TDA_PROP_AM) && !indep && !owcn && !mala) return fail(TDA_ERR_UNSUPPORTED, "proposal kind %d", p->kind);
  if (mala && e->nlev != 1) return fail(TDA_ERR_UNSUPPORTED, "%s is lowered for single-level chains only", gname);
  if (mala && !(p->scaling > 0.0)) return fail(TDA_ERR_INVALID, "%s: scaling must be positive", gname);
  if (owcn && e->nlev != 1) return fail(TDA_ERR_UNSUPPORTED, "the operator-weighted pCN proposal is lowered for single-level chains only");
  if ((p->kind == TDA_PROP_GRW || p->kind == TDA_PROP_AM || indep) && !p->C) return fail(TDA_ERR_INVALID, "proposal covariance missing");
  if (indep && !p->q_mean) return fail(TDA_ERR_INVALID, "independence sampler: q_mean missing");
  if (indep && e->nlev != 1) return fail(TDA_ERR_UNSUPPORTED, "the independence sampler is lowered for single-level chains only");
  if (p->period < 1) return fail(TDA_ERR_INVALID, "period must be >= 1");
  e->pp = *p;
  e->pp.q_mean = nullptr;
  if (owcn) {  // the scaling is inside the operators (proposal.py:579-580); per-chain with tda_engine_set_proposal_spectrum
    e->ow_scaling0 = p->scaling;
    e->pp.scaling = 1.0;
    e->ow_state_h.clear();
    e->ow_noise_h.clear();
    e->ow_spectral = false;
    e->ow_V_h.clear();
    e->ow_lam_h.clear();
  }
  if (indep) {  // never adapts (proposal.py:107-111); scaling plays no role
    e->pp.adaptive = 0;
    e->pp.scaling = 1.0;
    e->q_mean_h.assign(p->q_mean, p->q_mean + e->d);
  }
  if (p->kind == TDA_PROP_HMC) {  // the defaults of tda_engine_set_hmc, which follows
    e->hmc_n_leapfrog = 8;
    e->hmc_inv_mass_h.clear();
  }
  if (p->kind == TDA_PROP_NUTS) {  // the defaults of tda_engine_set_nuts, which follows
    e->nuts_max_depth = 8;
    e->nuts_target = 0.8;
    e->hmc_inv_mass_h.clear();
  }
  e->mass_W = 0;  // (tda_engine_set_mass_adaptation follows a proposal that takes it)
  e->dense_chol_h.clear();  // (and so does tda_engine_set_dense_mass)
  e->dmass_W = 0;  // (and tda_engine_set_dense_mass_adaptation)
  e->dmass_own_start = false;
  if (p->C) e->prop_C_h.assign(p->C, p->C + (size_t)e->d * e->d);
  e->pp.C = nullptr;
  e->am_sd = p->sd > 0.0 ? p->sd : std::min(1.0, 2.4 * 2.4 / e->d);
  e->prop_set = true;
  e->inited = false;
  return TDA_OK;
}

int tda_engine_set_proposal_operators(tda_engine* e, const double* state_operator, const double* noise_operator) {
  if (!e || !state_operator || !noise_operator) return fail(TDA_ERR_INVALID, "null argument");
  if (!e->prop_set || e->pp.kind != TDA_PROP_OWCN) return fail(TDA_ERR_STATE, "set_proposal with kind TDA_PROP_OWCN must precede set_proposal_operators");
  const size_t dd = (size_t)e->d * e->d;
  for (size_t i = 0; i < dd; ++i)
    if (!std::isfinite(state_operator[i]) || !std::isfinite(noise_operator[i])) return fail(TDA_ERR_NUMERIC, "proposal operators must be finite");
  e->ow_state_h.assign(state_operator, state_operator + dd);
  e->ow_noise_h.assign(noise_operator, noise_operator + dd);
  e->inited = false;
  return TDA_OK;
}

int tda_engine_set_proposal_spectrum(tda_engine* e, const double* V, const double* lambda) {
  if (!e || !V || !lambda) return fail(TDA_ERR_INVALID, "null argument");
  if (!e->prop_set || e->pp.kind != TDA_PROP_OWCN) return fail(TDA_ERR_STATE, "set_proposal with kind TDA_PROP_OWCN must precede set_proposal_spectrum");
  if (!(e->ow_scaling0 > 0.0)) return fail(TDA_ERR_INVALID, "operator-weighted pCN: scaling must be positive");
  const size_t dd = (size_t)e->d * e->d;
  for (size_t i = 0; i < dd; ++i)
    if (!std::isfinite(V[i])) return fail(TDA_ERR_NUMERIC, "eigenvectors must be finite");
  for (int i = 0; i < e->d; ++i)
    if (!std::isfinite(lambda[i])) return fail(TDA_ERR_NUMERIC, "eigenvalues must be finite");
  e->ow_V_h.assign(V, V + dd);
  e->ow_lam_h.assign(lambda, lambda + e->d);
  e->ow_spectral = true;
  e->inited = false;
  return TDA_OK;
}

int tda_engine_set_level_rosenbrock(tda_engine* e, int level, double a, double b, double data, double noise_var) {
  if (!e) return fail(TDA_ERR_INVALID, "null engine");
  if (level < 0 || level >= (int)e->levels.size()) return fail(TDA_ERR_INVALID, "level %d out of range", level);
  if (e->d < 2) return fail(TDA_ERR_INVALID, "the Rosenbrock chain needs dim >= 2");
  if (!(noise_var > 0.0)) return fail(TDA_ERR_NUMERIC, "noise variance must be positive");
  Level& lv = e->levels[level];
  lv.model = MODEL_ROSENBROCK;
  lv.ros_a = a;
  lv.ros_b = b;
  lv.ros_data = data;
  lv.m = 1;
  lv.m_pad = 0;
  lv.ncb = 0;
  lv.noise_kind = TDA_NOISE_ISO;
  lv.var = noise_var;
  lv.set = true;
  return TDA_OK;
}

int tda_engine_set_level_source(tda_engine* e, int level, const char* source, int32_t m, const double* data, int32_t noise_kind,
                                const double* noise) {
  if (!e || !source || !data || !noise) return fail(TDA_ERR_INVALID, "null argument");
  if (level < 0 || level >= (int)e->levels.size()) return fail(TDA_ERR_INVALID, "level %d out of range", level);
  if (m < 1) return fail(TDA_ERR_INVALID, "m must be >= 1");
  const bool loglike = noise_kind == TDA_NOISE_SOURCE;  // the likelihood is part of the source (tda_loglike_term, or tda_loglike_wave for one that couples outputs), `noise` its parameters
  if (!loglike && noise_kind != TDA_NOISE_ISO && noise_kind != TDA_NOISE_DIAG && noise_kind != TDA_NOISE_DENSE && !(noise_kind == TDA_NOISE_ADAPTIVE && e->nlev > 1))
    return fail(TDA_ERR_UNSUPPORTED, "noise kind %d (AdaptiveGaussianLogLike only below the finest level of a hierarchy)", noise_kind);
  HIP_TRY(hipSetDevice(e->cfg.device));
  Level& lv = e->levels[level];
  // (a source refused here leaves the level as it was: its text, its forms and its programs belong together)
  const UserForms forms = user_forms(source);
  if (forms.both_prior_forms())
    return fail(TDA_ERR_INVALID, "a source-defined prior: the source defines both tda_logprior_term and tda_logprior_wave (a prior has one form)");
  if (forms.both_loglike_forms())
    return fail(TDA_ERR_INVALID, "a source-defined likelihood: the source defines both tda_loglike_term and tda_loglike_wave (a likelihood has one form)");
  lv.uprog.unload();
  lv.uprog_mala.unload();
  lv.forms = forms;
  // compiled here, so that a bad source is refused now (a prior set later: tda_engine_init compiles again, ensure_user_programs)
  const int m_was = lv.m, noise_kind_was = lv.noise_kind;
  lv.usrc = source;
  lv.m = m;
  lv.noise_kind = noise_kind;
  int rc = ensure_user_program(e, lv, false);
  if (rc) {  // (whatever the level was set to before keeps its shape)
    lv.m = m_was;
    lv.noise_kind = noise_kind_was;
    return rc;
  }
  std::vector<double> y(data, data + m), w;
  lv.upar.release();
  if (loglike) {
    lv.var = 1.0;
    if ((rc = lv.upar.upload(std::vector<double>(noise, noise + m)))) return rc;
  } else if (noise_kind == TDA_NOISE_ADAPTIVE) {
    if ((rc = ext_level_adaptive(e, lv, m, data, noise))) return rc;
  } else if (noise_kind == TDA_NOISE_DENSE) {
    if ((rc = ext_level_dense(e, lv, m, noise))) return rc;
  } else if (noise_kind == TDA_NOISE_ISO) {
    if (!(noise[0] > 0.0)) return fail(TDA_ERR_NUMERIC, "noise variance must be positive");
    lv.var = noise[0];
  } else {
    w.resize(m);
    for (int i = 0; i < m; ++i) {
      if (!(noise[i] > 0.0)) return fail(TDA_ERR_NUMERIC, "noise variance must be positive");
      w[i] = 1.0 / noise[i];
    }
    lv.var = 1.0;
    if ((rc = lv.uw.upload(w))) return rc;
  }
  if ((rc = lv.udata.upload(y))) return rc;
  if (noise_kind != TDA_NOISE_ADAPTIVE) {  // host / padded device copies of the data (error-model initialisation and kernels)
    const int mp = m > 128 ? m : 128;
    lv.ytil_h.assign(mp, 0.0);
    lv.data_h.assign(mp, 0.0);
    for (int i = 0; i < m; ++i) lv.ytil_h[i] = lv.data_h[i] = data[i];
    if ((rc = lv.data64.upload(lv.data_h))) return rc;
  }
  // hierarchies and DREAM(Z): proposals / outputs of a step pass through device buffers (tda_user_eval)
  if ((rc = lv.cb_prop.alloc((size_t)e->N * e->d))) return rc;
  if ((rc = lv.cb_F.alloc((size_t)e->N * m))) return rc;
  lv.model = MODEL_USER;
  lv.m = m;
  lv.m_pad = 16;  // (no MFMA staging; keeps the shared LDS-size arithmetic of the run loop valid)
  lv.ncb = 1;
  lv.noise_kind = noise_kind;
  lv.set = true;
  e->inited = false;
  return TDA_OK;
}

int tda_engine_set_level_callback(tda_engine* e, int level, tda_forward_batch_fn fn, void* user, int32_t m, const double* data,
                                  int32_t noise_kind, const double* noise) {
  if (!e || !fn || !data || !noise) return fail(TDA_ERR_INVALID, "null argument");
  if (level < 0 || level >= (int)e->levels.size()) return fail(TDA_ERR_INVALID, "level %d out of range", level);
  if (m < 1) return fail(TDA_ERR_INVALID, "m must be >= 1");
  if (noise_kind == TDA_NOISE_SOURCE)
    return fail(TDA_ERR_UNSUPPORTED, "a source-defined likelihood (TDA_NOISE_SOURCE) needs a source-defined forward model (tda_engine_set_level_source)");
  if (noise_kind != TDA_NOISE_ISO && noise_kind != TDA_NOISE_DIAG && noise_kind != TDA_NOISE_DENSE && !(noise_kind == TDA_NOISE_ADAPTIVE && e->nlev > 1))
    return fail(TDA_ERR_UNSUPPORTED, "noise kind %d (AdaptiveGaussianLogLike only below the finest level of a hierarchy)", noise_kind);
  HIP_TRY(hipSetDevice(e->cfg.device));
  Level& lv = e->levels[level];
  std::vector<double> y(data, data + m), w;
  int rc;
  if (noise_kind == TDA_NOISE_ADAPTIVE) {
    if ((rc = ext_level_adaptive(e, lv, m, data, noise))) return rc;
  } else if (noise_kind == TDA_NOISE_DENSE) {
    if ((rc = ext_level_dense(e, lv, m, noise))) return rc;
  } else if (noise_kind == TDA_NOISE_ISO) {
    if (!(noise[0] > 0.0)) return fail(TDA_ERR_NUMERIC, "noise variance must be positive");
    lv.var = noise[0];
  } else {
    w.resize(m);
    for (int i = 0; i < m; ++i) {
      if (!(noise[i] > 0.0)) return fail(TDA_ERR_NUMERIC, "noise variance must be positive");
      w[i] = 1.0 / noise[i];
    }
    lv.var = 1.0;
    if ((rc = lv.uw.upload(w))) return rc;
  }
  if ((rc = lv.udata.upload(y))) return rc;
  if (noise_kind != TDA_NOISE_ADAPTIVE) {  // host / padded device copies of the data (error-model initialisation and kernels)
    const int mp = m > 128 ? m : 128;
    lv.ytil_h.assign(mp, 0.0);
    lv.data_h.assign(mp, 0.0);
    for (int i = 0; i < m; ++i) lv.ytil_h[i] = lv.data_h[i] = data[i];
    if ((rc = lv.data64.upload(lv.data_h))) return rc;
  }
  lv.release_callback_buffers();
  HIP_TRY(hipHostMalloc((void**)&lv.cb_theta_h, (size_t)e->N * e->d * sizeof(double), hipHostMallocDefault));
  HIP_TRY(hipHostMalloc((void**)&lv.cb_F_h, (size_t)e->N * m * sizeof(double), hipHostMallocDefault));
  if ((rc = lv.cb_prop.alloc((size_t)e->N * e->d))) return rc;
  if ((rc = lv.cb_F.alloc((size_t)e->N * m))) return rc;
  lv.cb_fn = fn;
  lv.cb_user = user;
  lv.model = MODEL_CALLBACK;
  lv.m = m;
  lv.m_pad = 16;  // (no MFMA staging; keeps the shared LDS-size arithmetic of the run loop valid)
  lv.ncb = 1;
  lv.noise_kind = noise_kind;
  lv.set = true;
  e->inited = false;
  return TDA_OK;
}

}  // extern "C"
