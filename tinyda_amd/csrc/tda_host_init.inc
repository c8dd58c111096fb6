// Part of libtinyda_hip.so: included by tda_engine.hip (ONE translation unit -- the helpers, the engine struct and the kernel
// launchers above it are visible here).  Tda_engine_init: allocation, initial links, proposal factors, level and error-model state.
extern "C" {

int tda_engine_init(tda_engine* e, const double* theta0) {
  if (!e) return fail(TDA_ERR_INVALID, "null engine");
  if (!e->prior_set || !e->prop_set) return fail(TDA_ERR_STATE, "set_prior and set_proposal must precede init");
  for (auto& lv : e->levels)
    if (!lv.set) return fail(TDA_ERR_STATE, "set_level missing");
  if (e->prior_source) {
    // a source-defined prior (TDA_PRIOR_SOURCE) exists inside tda_user_steps of the levels' programs only: every route on which
    // one of the engine's own kernels (k_ext_accept, k_mh_steps, k_ml_steps, k_da_steps, the DREAM(Z) kernels) would evaluate
    // the prior, or that needs the prior to be Gaussian, would read p / q as a mean and an inverse variance
    for (const Level& ls : e->levels)
      if (ls.model != MODEL_USER || ls.noise_kind == TDA_NOISE_DENSE)
        return fail(TDA_ERR_UNSUPPORTED, "a source-defined prior needs source-defined forward models with isotropic / diagonal noise or a source-defined likelihood at every level");
    if (e->is_dreamz) return fail(TDA_ERR_UNSUPPORTED, "a source-defined prior under DREAM(Z) is not lowered");
    if (e->pp.kind == TDA_PROP_PCN || e->pp.kind == TDA_PROP_OWCN)
      return fail(TDA_ERR_UNSUPPORTED, "a source-defined prior under pCN and operator-weighted pCN is not lowered (they need a Gaussian prior)");
    if (gradient_proposal(e->pp.kind)) {  // tda_user_mala_steps / tda_user_hmc_steps take the prior's own gradient from the level's source (single level: set_proposal)
      const UserForms& f0 = e->levels[0].forms;
      if (f0.prior_wave ? !f0.prior_grad : !f0.prior_term_grad)
        return fail(TDA_ERR_UNSUPPORTED, "a source-defined prior under %s needs %s in the level's source", gradient_proposal_name(e->pp.kind),
                    f0.prior_wave ? TDA_SIG_LOGPRIOR_GRAD : TDA_SIG_LOGPRIOR_TERM_GRAD);
    }
    if (e->pp.kind == TDA_PROP_INDEPENDENCE) return fail(TDA_ERR_UNSUPPORTED, "a source-defined prior under the Independence proposal is not lowered");
    if (e->aem) return fail(TDA_ERR_UNSUPPORTED, "a source-defined prior together with an error model is not lowered");
    if (e->nlev > 1 && e->randomize) return fail(TDA_ERR_UNSUPPORTED, "a source-defined prior with randomised subchain lengths is not lowered");
    if (e->nlev > AEM_MAXLEV) return fail(TDA_ERR_UNSUPPORTED, "a source-defined prior: hierarchies of at most %d levels", (int)AEM_MAXLEV);
    if (!theta0) return fail(TDA_ERR_INVALID, "a source-defined prior needs explicit initial parameters");
  }
  if (e->nlev > AEM_MAXLEV) {  // five and six levels (0.5): the generic level kernel over the engine's own models, no error model
    if (e->aem) return fail(TDA_ERR_UNSUPPORTED, "error models are lowered for hierarchies of at most %d levels", (int)AEM_MAXLEV);
    if (e->wide) return fail(TDA_ERR_UNSUPPORTED, "more than 64 parameters: hierarchies of at most %d levels", (int)AEM_MAXLEV);
    for (const Level& l0 : e->levels)
      if (l0.noise_kind == TDA_NOISE_DENSE) return fail(TDA_ERR_UNSUPPORTED, "a dense observation covariance in a hierarchy: at most %d levels", (int)AEM_MAXLEV);
  }
  if (e->wide) {  // 65 .. 128 parameters (tda_kernels_wide.h): what that path is built for
    const bool user_mala = !e->is_dreamz && gradient_proposal(e->pp.kind) && e->nlev == 1 && e->levels[0].model == MODEL_USER;
    if (e->is_dreamz || (e->pp.kind != TDA_PROP_GRW && e->pp.kind != TDA_PROP_PCN && e->pp.kind != TDA_PROP_AM && !user_mala))
      return fail(TDA_ERR_UNSUPPORTED, "more than 64 parameters: GaussianRandomWalk, CrankNicolson and AdaptiveMetropolis are lowered (MALA and HMC: single-level source-defined models)");
    if (e->pp.kind == TDA_PROP_AM && e->pp.block_moments) return fail(TDA_ERR_UNSUPPORTED, "more than 64 parameters: block_moments is not lowered");
    for (const Level& l0 : e->levels) {
      // (a batched host callback, single level or in a host-sequenced hierarchy: k_ext_propose / k_ext_accept / k_ext_level_action take a
      // second parameter per lane)
      const bool model_ok = l0.model == MODEL_LINEAR || l0.model == MODEL_CALLBACK || l0.model == MODEL_USER;
      const bool noise_ok = l0.noise_kind == TDA_NOISE_ISO || l0.noise_kind == TDA_NOISE_DIAG || l0.noise_kind == TDA_NOISE_ADAPTIVE ||
                            l0.noise_kind == TDA_NOISE_SOURCE ||  // (tda_user_steps / tda_user_level_action, refusals below)
                            (l0.noise_kind == TDA_NOISE_DENSE && e->nlev == 1 && l0.model == MODEL_LINEAR);  // (dense: the step kernel's own path, single level)
      if (!model_ok || !noise_ok)
        return fail(TDA_ERR_UNSUPPORTED, "more than 64 parameters: linear, source-defined and host-callback forward models with isotropic or diagonal noise (single-level linear models: dense too) are lowered");
    }
    if (e->nlev > 1 && e->aem == TDA_AEM_STATE_INDEPENDENT_DIAGONAL) return fail(TDA_ERR_UNSUPPORTED, "more than 64 parameters: the dense error model is lowered, the diagonal one is not");
  }
  if (e->prop_set && !e->is_dreamz && e->pp.kind == TDA_PROP_OWCN) {
    if (e->ow_state_h.empty() && !e->ow_spectral) return fail(TDA_ERR_STATE, "operator-weighted pCN: set_proposal_operators / set_proposal_spectrum missing");
    if (e->pp.adaptive && !e->ow_spectral)
      return fail(TDA_ERR_UNSUPPORTED, "operator-weighted pCN: adaptive scaling needs per-chain operators (tda_engine_set_proposal_spectrum)");
    if (e->ow_spectral && e->levels[0].model != MODEL_LINEAR)
      return fail(TDA_ERR_UNSUPPORTED, "operator-weighted pCN with per-chain operators is lowered for linear forward models");
    if (e->levels[0].model != MODEL_LINEAR && e->levels[0].model != MODEL_CALLBACK && e->levels[0].model != MODEL_USER)
      return fail(TDA_ERR_UNSUPPORTED, "operator-weighted pCN is lowered for linear, callback and source-defined forward models");
    if (e->prior_bounded) return fail(TDA_ERR_UNSUPPORTED, "operator-weighted pCN needs a Gaussian prior");
  }
  if (e->prop_set && !e->is_dreamz && gradient_proposal(e->pp.kind)) {
    const Level& l0 = e->levels[0];
    const char* const gname = gradient_proposal_name(e->pp.kind);
    if (leapfrog_proposal(e->pp.kind) && l0.model != MODEL_USER)  // (k_mh_steps has MALA's closed-form gradient of the linear model and no leapfrog loop)
      return fail(TDA_ERR_UNSUPPORTED, "%s is lowered for source-defined forward models with tda_gradient only (the built-in linear model has MALA)", gname);
    if (l0.model != MODEL_LINEAR && l0.model != MODEL_USER)
      return fail(TDA_ERR_UNSUPPORTED, "MALA is lowered for linear and source-defined forward models only (exact gradient)");
    if (e->prior_bounded) return fail(TDA_ERR_UNSUPPORTED, "%s needs a Gaussian prior", gname);
    if (l0.noise_kind == TDA_NOISE_ADAPTIVE) return fail(TDA_ERR_UNSUPPORTED, "%s: adaptive likelihoods are not lowered", gname);
    if (l0.model == MODEL_USER) {  // tda_user_mala_steps / tda_user_hmc_steps: iso / diag noise, diagonal Gaussian or source-defined prior, sensitivity of m <= 2048 outputs in LDS
      if ((e->prior_joint && !e->prior_source) || e->prior_kind == PRIOR_DENSE)
        return fail(TDA_ERR_UNSUPPORTED, "%s over a source-defined model needs a multivariate normal prior with diagonal covariance or a source-defined prior", gname);
      if (l0.noise_kind == TDA_NOISE_DENSE) return fail(TDA_ERR_UNSUPPORTED, "%s over a source-defined model: isotropic or diagonal noise", gname);
      if (l0.m > 2048) return fail(TDA_ERR_UNSUPPORTED, "%s over a source-defined model: at most 2048 outputs", gname);
    }
  }
  for (const Level& ls : e->levels) {
    // a source-defined likelihood exists inside the level's hiprtc programs only (tda_user_steps, tda_user_level_action, the MALA
    // kernels): every route that evaluates a source level's likelihood in the engine's own kernels would treat it as Gaussian
    if (ls.noise_kind != TDA_NOISE_SOURCE) continue;
    if (e->is_dreamz) return fail(TDA_ERR_UNSUPPORTED, "a source-defined likelihood under DREAM(Z) is not lowered");
    if (e->aem) return fail(TDA_ERR_UNSUPPORTED, "a source-defined likelihood together with an error model is not lowered");
    if (e->nlev > 1 && e->randomize) return fail(TDA_ERR_UNSUPPORTED, "a source-defined likelihood with randomised subchain lengths is not lowered");
    if (e->pp.kind == TDA_PROP_INDEPENDENCE || e->pp.kind == TDA_PROP_OWCN)
      return fail(TDA_ERR_UNSUPPORTED, "a source-defined likelihood under the Independence and operator-weighted pCN proposals is not lowered");
    if (e->nlev > AEM_MAXLEV) return fail(TDA_ERR_UNSUPPORTED, "a source-defined likelihood: hierarchies of at most %d levels", (int)AEM_MAXLEV);
  }
  {
    int n_cb = 0;
    for (auto& lv : e->levels) n_cb += (lv.model == MODEL_CALLBACK || lv.model == MODEL_USER) ? 1 : 0;
    // DREAMZ below a hierarchy (the reference's MLDA notebook): its jump needs the chain's growing archive at every base step,
    // so such a hierarchy is sequenced by the host like one with callback / source-defined levels, linear levels included
    const bool dz_hier = e->is_dreamz && e->nlev > 1;
    const bool aemd = e->aem == TDA_AEM_STATE_INDEPENDENT_DIAGONAL;  // the diagonal error model works on model-output arrays
    e->ext_hier = (n_cb || dz_hier || aemd) && e->nlev > 1;
    if (e->ext_hier && e->nlev > AEM_MAXLEV) return fail(TDA_ERR_UNSUPPORTED, "hierarchies sequenced by the host (callback / source-defined levels, DREAM(Z) below): at most %d levels", (int)AEM_MAXLEV);
    if (e->ext_hier) {  // Delayed Acceptance / MLDA with callback / source-defined models (host-sequenced level actions)
      for (auto& lv : e->levels)  // linear levels may be mixed in (k_ext_linear_eval); anything else may not
        if (lv.model != MODEL_CALLBACK && lv.model != MODEL_USER && (lv.model != MODEL_LINEAR || !lv.A_dev.p))
          return fail(TDA_ERR_UNSUPPORTED, "hierarchies with callback / source-defined levels take linear levels with isotropic or diagonal noise beside them");
      if (e->pp.kind != TDA_PROP_GRW && e->pp.kind != TDA_PROP_PCN && e->pp.kind != TDA_PROP_AM && !dz_hier)
        return fail(TDA_ERR_UNSUPPORTED, "callback hierarchies take GaussianRandomWalk / CrankNicolson / AdaptiveMetropolis / DREAMZ proposals");
      if (dz_hier && e->aem == TDA_AEM_STATE_INDEPENDENT_DIAGONAL)
        return fail(TDA_ERR_UNSUPPORTED, "DREAMZ below a hierarchy with the diagonal error model is not lowered (the reference's dense model is)");
      if (e->prior_kind == PRIOR_DENSE) return fail(TDA_ERR_UNSUPPORTED, "callback forward models need a diagonal prior covariance");
    }
  }
  if (e->prior_bounded) {  // JointPrior with uniform components
    // single-level GRW / AM (fused), or a host-sequenced hierarchy (callback / source-defined levels): there the base-level
    // kernels test the support bounds and the upper levels carry the log-prior of the states they promote
    if (e->is_dreamz && e->levels[0].model == MODEL_ROSENBROCK)
      return fail(TDA_ERR_UNSUPPORTED, "priors with uniform components are not lowered for the Rosenbrock example model");
    if (e->is_dreamz && !(e->arch_set && e->arch_given)) return fail(TDA_ERR_INVALID, "priors with uniform components: DREAM(Z) needs an explicit initial archive");
    if (e->pp.kind == TDA_PROP_PCN) return fail(TDA_ERR_UNSUPPORTED, "pCN needs a Gaussian prior");
    for (auto& lv : e->levels)
      if (lv.noise_kind == TDA_NOISE_DENSE) return fail(TDA_ERR_UNSUPPORTED, "priors with uniform components: iso / diag noise only");
    if (!theta0) return fail(TDA_ERR_INVALID, "priors with uniform components need explicit initial parameters");
  }
  HIP_TRY(hipSetDevice(e->cfg.device));
  const int d = e->d, DP = e->DP;
  const int64_t N = e->N, NP = e->NP;
  int rc;
  if ((rc = ensure_user_programs(e))) return rc;
  if ((rc = e->theta.alloc((size_t)NP * DP))) return rc;
  if ((rc = e->lp.alloc(NP))) return rc;
  if ((rc = e->ll.alloc(NP))) return rc;
  if ((rc = e->acc_count.alloc(NP))) return rc;
  if ((rc = e->flags.alloc(NP))) return rc;
  HIP_TRY(hipMemsetAsync(e->acc_count.p, 0, NP * sizeof(int32_t), e->stream));
  HIP_TRY(hipMemsetAsync(e->flags.p, 0, NP * sizeof(int32_t), e->stream));
  HIP_TRY(hipMemsetAsync(e->lp.p, 0, NP * sizeof(double), e->stream));
  HIP_TRY(hipMemsetAsync(e->ll.p, 0, NP * sizeof(double), e->stream));

  // initial parameters
  std::vector<double> th0;
  if (!theta0) {  // theta0 ~ prior (sampler.py:209) from RNG stream 2
    th0.resize((size_t)N * d);
    // (a few host threads: 4096 chains x 32 Philox / Box-Muller pairs were 17 of the 20 ms an init took)
    host_chain_ranges(N, [&](int64_t c0, int64_t c1) {
      std::vector<double> z(d + 1);
      for (int64_t c = c0; c < c1; ++c) {
        for (int b = 0; b < (d + 1) / 2; ++b)
          normal_pair(e->cfg.seed, (uint32_t)(e->cfg.chain_offset + c), 0u, STREAM_INIT, (uint32_t)b, z[2 * b], z[2 * b + 1]);
        for (int i = 0; i < d; ++i) {
          double s = 0.0;
          for (int k = 0; k <= i; ++k) s = std::fma(e->prior_L_h[(size_t)i * d + k], z[k], s);
          th0[(size_t)c * d + i] = e->prior_mean_h[i] + s;
        }
      }
    });
    theta0 = th0.data();
  }
  if ((rc = upload_states(e, theta0, N, e->theta.p))) return rc;
  if (e->pp.kind == TDA_PROP_INDEPENDENCE) {
    // log q(theta0) up to q's constant: -|L^-1 (theta0 - q_mean)|^2 / 2 (the kernels carry -|z|^2 / 2 for proposals)
    std::vector<double> Lq, th_h;
    if (!cholesky_host(e->prop_C_h.data(), d, Lq)) return fail(TDA_ERR_NUMERIC, "proposal covariance is not positive definite");
    const double* hs = theta0;
    if (is_device_ptr(theta0)) {
      th_h.resize((size_t)N * d);
      HIP_TRY(hipMemcpy(th_h.data(), theta0, th_h.size() * sizeof(double), hipMemcpyDeviceToHost));
      hs = th_h.data();
    }
    std::vector<double> lq0(NP, 0.0), w(d), qm(DP, 0.0);
    for (int64_t c = 0; c < N; ++c) {
      double s2 = 0.0;
      for (int i = 0; i < d; ++i) {
        double s = hs[(size_t)c * d + i] - e->q_mean_h[i];
        for (int k = 0; k < i; ++k) s -= Lq[(size_t)i * d + k] * w[k];
        w[i] = s / Lq[(size_t)i * d + i];
        s2 += w[i] * w[i];
      }
      lq0[c] = -0.5 * s2;
    }
    for (int j = 0; j < d; ++j) qm[j] = e->q_mean_h[j];
    if ((rc = e->lq.upload(lq0)) || (rc = e->q_mean_d.upload(qm))) return rc;
    if ((rc = e->qzblk.alloc((size_t)e->SMAX * NP)) || (rc = e->qzblk2[0].alloc((size_t)e->SMAX * NP)) ||
        (rc = e->qzblk2[1].alloc((size_t)e->SMAX * NP)))
      return rc;
  }

  // proposal state (chain.py:74-76)
  std::vector<double> sc(NP, (e->pp.kind == TDA_PROP_AM || e->pp.kind == TDA_PROP_INDEPENDENCE) ? 1.0
                             : (e->pp.kind == TDA_PROP_OWCN && e->ow_spectral) ? e->ow_scaling0 : e->pp.scaling);
  if ((rc = e->scaling.upload(sc))) return rc;
  if (e->is_dreamz) {
    if (!e->arch_set && (rc = tda_engine_set_archive(e, nullptr))) return rc;
    const bool sh = e->dz.shared != 0;
    const int64_t M0 = e->dz.M0;
    e->arch_cap = e->dz.capacity;
    const size_t narch = (size_t)(sh ? 1 : NP) * e->arch_cap * DP;
    if ((rc = e->arch.alloc(narch))) return rc;
    HIP_TRY(hipMemsetAsync(e->arch.p, 0, narch * sizeof(double), e->stream));
    {  // Z0 -> padded device layout
      const int64_t nA = sh ? 1 : N;
      std::vector<double> pad((size_t)M0 * DP, 0.0);
      for (int64_t c = 0; c < nA; ++c) {
        for (int64_t r = 0; r < M0; ++r)
          for (int j = 0; j < d; ++j) pad[(size_t)r * DP + j] = e->Z0_h[((size_t)c * M0 + r) * d + j];
        HIP_TRY(hipMemcpy(e->arch.p + (size_t)c * e->arch_cap * DP, pad.data(), pad.size() * sizeof(double), hipMemcpyHostToDevice));
      }
    }
    e->arch_rows = M0;
    e->sums_rows = 0;
    const size_t nsum = (size_t)(sh ? 1 : NP) * DP;
    std::vector<double> zero(nsum, 0.0), pcr((size_t)NP * MAX_NCR, 0.0), ones((size_t)NP * MAX_NCR, 1.0), zer2((size_t)NP * MAX_NCR, 0.0);
    for (int64_t c = 0; c < NP; ++c)
      for (int k = 0; k < e->dz.nCR; ++k) pcr[(size_t)c * MAX_NCR + k] = 1.0 / e->dz.nCR;  // proposal.py:731
    if ((rc = e->zsum.upload(zero))) return rc;
    if ((rc = e->zsq.upload(zero))) return rc;
    if ((rc = e->dz_pCR.upload(pcr))) return rc;
    if ((rc = e->dz_Delta.upload(ones))) return rc;  // proposal.py:755
    if ((rc = e->dz_LCR.upload(zer2))) return rc;    // proposal.py:754
    if ((rc = e->dz_mcr_last.alloc(NP))) return rc;
    HIP_TRY(hipMemsetAsync(e->dz_mcr_last.p, 0, NP * sizeof(int32_t), e->stream));
    if ((rc = e->dz_coef.alloc((size_t)e->SMAX * NP * DP))) return rc;
    if ((rc = e->dz_epsm.alloc((size_t)e->SMAX * NP * DP))) return rc;
    if ((rc = e->dz_ridx.alloc((size_t)e->SMAX * NP * 2 * MAX_DELTA))) return rc;
    if ((rc = e->theta_prev.alloc((size_t)NP * DP))) return rc;
    HIP_TRY(hipMemcpyAsync(e->theta_prev.p, e->theta.p, (size_t)NP * DP * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
    if (sh) {
      if ((rc = e->blk_states.alloc((size_t)e->SMAX * NP * DP))) return rc;
      if ((rc = e->blk_hist.alloc((size_t)e->SMAX * NP * DP))) return rc;
    }
    if ((rc = e->ublk.alloc((size_t)e->SMAX * NP))) return rc;
    if ((rc = e->rec_params.alloc((size_t)e->SMAX * N * d))) return rc;
    if ((rc = e->rec_stats.alloc((size_t)e->SMAX * N * 3))) return rc;
    if ((rc = e->rec_acc.alloc((size_t)e->SMAX * N))) return rc;
    e->t = 0;
    e->k_adapt = 0;
    e->rp_pos = 0;
    e->exp_pos = 0;
    e->pending_steps = 0;
    e->inited = true;  // dreamz_sums_catchup checks nothing else
    if ((rc = dreamz_sums_catchup(e, 0, M0, false, false, 1.0))) return rc;
    if ((rc = e->theta_last.alloc((size_t)NP * DP))) return rc;
    // initial link (chain.py:70); below a hierarchy the level set-up further down evaluates every level at theta0
    if (e->nlev > 1) {
      if (e->levels[0].model == MODEL_ROSENBROCK) return fail(TDA_ERR_UNSUPPORTED, "the Rosenbrock example model is single-level");
    } else if (e->levels[0].model == MODEL_LINEAR || e->levels[0].model == MODEL_CALLBACK || e->levels[0].model == MODEL_USER) {
      if ((rc = launch_eval(e, 0, e->theta.p, e->lp.p, e->ll.p))) return rc;
    } else {
      // Rosenbrock level: evaluate theta0 with a zero-jump DREAMZ step (coef = eps = 0, u = 0 -> accepted)
      HIP_TRY(hipMemsetAsync(e->dz_coef.p, 0, (size_t)NP * DP * sizeof(double), e->stream));
      HIP_TRY(hipMemsetAsync(e->dz_epsm.p, 0, (size_t)NP * DP * sizeof(double), e->stream));
      HIP_TRY(hipMemsetAsync(e->dz_ridx.p, 0, (size_t)NP * 2 * MAX_DELTA * sizeof(int32_t), e->stream));
      std::vector<double> uz(NP, -1.0), big(NP, -1e300);
      HIP_TRY(hipMemcpy(e->ublk.p, uz.data(), NP * sizeof(double), hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(e->lp.p, big.data(), NP * sizeof(double), hipMemcpyHostToDevice));
      HIP_TRY(hipMemsetAsync(e->ll.p, 0, NP * sizeof(double), e->stream));
      DreamStepArgs sa{};
      extern void fill_dreamz_step_args(tda_engine*, DreamStepArgs&);
      fill_dreamz_step_args(e, sa);
      sa.S = 1;
      sa.shared = 1;  // no archive append for this evaluation
      sa.blk_states = nullptr;
      sa.rec_params = nullptr;
      sa.rec_stats = nullptr;
      sa.rec_acc = nullptr;
      const size_t lds = ((size_t)16 * (DP + 2) + 128 + 64) * sizeof(double);
      DISPATCH_DPAD(DP, launch_dz_steps<DPAD>(sa, lds, e->stream));
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemsetAsync(e->acc_count.p, 0, NP * sizeof(int32_t), e->stream));
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->nlev == 1) return TDA_OK;
  }
  const bool owcn = !e->is_dreamz && e->pp.kind == TDA_PROP_OWCN, mala = !e->is_dreamz && gradient_proposal(e->pp.kind);
  const bool user_mala = mala && e->levels[0].model == MODEL_USER;  // (HMC: always, the refusals above)
  // the second program (the MALA program, or under HMC the HMC program): GRW / pCN / AM engines never build it
  if (user_mala && (rc = ensure_user_program(e, e->levels[0], true))) return rc;
  if (user_mala && e->pp.kind == TDA_PROP_NUTS) {  // the U-turn checkpoints are dynamic LDS behind the MALA program's: 64 KiB per chain with them
    const Level& l0 = e->levels[0];
    const size_t dyn = user_mala_lds(l0.uprog_mala.spec, l0.m), ck = user_nuts_checkpoint_lds(e->nuts_max_depth, DP);
    int stat = 0;
    HIP_TRY(hipFuncGetAttribute(&stat, HIP_FUNC_ATTRIBUTE_SHARED_SIZE_BYTES, l0.uprog_mala.steps));
    if ((size_t)stat + dyn + ck > USER_LDS_MAX && l0.uprog_mala.spec.dense_mass)
      return fail(TDA_ERR_UNSUPPORTED, "NUTS over a source-defined model needs more than 64 KiB of LDS per chain: this source needs %d bytes (parameters, gradient, "
                                       "TDA_WORKSPACE and %zu bytes for the operand of the dense mass's products) + %zu bytes for its %d outputs + %zu bytes for the "
                                       "checkpoints of max_depth = %d over %d padded parameters = %zu bytes",
                  stat, user_dense_mass_lds(), dyn, l0.m, ck, e->nuts_max_depth, DP, (size_t)stat + dyn + ck);
    if ((size_t)stat + dyn + ck > USER_LDS_MAX)
      return fail(TDA_ERR_UNSUPPORTED, "NUTS over a source-defined model holds at most 64 KiB of LDS per chain: this source needs %d bytes (parameters, gradient and "
                                       "TDA_WORKSPACE) + %zu bytes for its %d outputs + %zu bytes for the checkpoints of max_depth = %d over %d padded parameters",
                  stat, dyn, l0.m, ck, e->nuts_max_depth, DP);
  }
  if (user_mala && e->pp.kind == TDA_PROP_HMC && e->levels[0].uprog_mala.spec.dense_mass) {  // (HMC: the dense mass's 1 KiB may be what no longer fits)
    const Level& l0 = e->levels[0];
    const size_t dyn = user_mala_lds(l0.uprog_mala.spec, l0.m);
    int stat = 0;
    HIP_TRY(hipFuncGetAttribute(&stat, HIP_FUNC_ATTRIBUTE_SHARED_SIZE_BYTES, l0.uprog_mala.steps));
    if ((size_t)stat + dyn > USER_LDS_MAX)
      return fail(TDA_ERR_UNSUPPORTED, "HMC over a source-defined model needs more than 64 KiB of LDS per chain: this source needs %d bytes (parameters, gradient, "
                                       "TDA_WORKSPACE and %zu bytes for the operand of the dense mass's products) + %zu bytes for its %d outputs = %zu bytes",
                  stat, user_dense_mass_lds(), dyn, l0.m, (size_t)stat + dyn);
  }
  if (!e->is_dreamz) {  // ---- Gaussian proposals: factor of the proposal covariance (DREAMZ has its archive instead) ----
  std::vector<double> L;
  const double* Cuse = (e->pp.kind == TDA_PROP_PCN || owcn) ? e->prior_cov_h.data() : e->prop_C_h.data();  // proposal.py:336-341
  if (!mala && !cholesky_host(Cuse, d, L)) return fail(TDA_ERR_NUMERIC, "proposal covariance is not positive definite");
  std::vector<double> Lk((size_t)DP * DP, 0.0);
  if (mala) {  // np.random.normal(size = d) (proposal.py:955): unit factor
    for (int j = 0; j < d; ++j) Lk[(size_t)j * DP + j] = 1.0;
    L.assign((size_t)d * d, 0.0);  // (65 .. 128 parameters: packed into tiles below)
    for (int j = 0; j < d; ++j) L[(size_t)j * d + j] = 1.0;
  }
  if (user_mala) {
    // source-defined model: the gradient comes from the model's own tda_gradient at every step (tda_user_mala_steps)
    if ((rc = e->mala_grad.alloc((size_t)NP * DP))) return rc;
    HIP_TRY(hipMemsetAsync(e->mala_grad.p, 0, (size_t)NP * DP * sizeof(double), e->stream));
    if (e->pp.kind == TDA_PROP_NUTS) {  // the per-chain sums: chain state of a NUTS engine alone
      if ((rc = e->nuts_accsum.alloc((size_t)NP)) || (rc = e->nuts_totals.alloc((size_t)NP * TDA_NUTS_TOTALS))) return rc;
      HIP_TRY(hipMemsetAsync(e->nuts_accsum.p, 0, (size_t)NP * sizeof(double), e->stream));
      HIP_TRY(hipMemsetAsync(e->nuts_totals.p, 0, (size_t)NP * TDA_NUTS_TOTALS * sizeof(long long), e->stream));
    } else {
      e->nuts_accsum.release();
      e->nuts_totals.release();
    }
    if (leapfrog_proposal(e->pp.kind)) {  // the diagonal inverse mass, ones in the padding (and everywhere without tda_engine_set_hmc's / set_nuts's array)
      std::vector<double> wm(DP, 1.0);
      for (int j = 0; j < d && !e->hmc_inv_mass_h.empty(); ++j) wm[j] = e->hmc_inv_mass_h[j];
      if ((rc = e->hmc_inv_mass.upload(wm))) return rc;
    }
    if (leapfrog_proposal(e->pp.kind) && !e->dense_chol_h.empty()) {  // the dense factor and its transpose, zero outside the triangle and in the padding
      std::vector<double> LL(2 * (size_t)DP * DP, 0.0);
      for (int i = 0; i < d; ++i)
        for (int j = 0; j <= i; ++j) {
          LL[(size_t)i * DP + j] = e->dense_chol_h[(size_t)i * d + j];
          LL[(size_t)DP * DP + (size_t)j * DP + i] = e->dense_chol_h[(size_t)i * d + j];
        }
      if ((rc = e->dense_chol.upload(LL))) return rc;
    } else {
      e->dense_chol.release();
    }
    e->mass_n = 0;
    e->mass_updates = 0;
    if (leapfrog_proposal(e->pp.kind) && e->dmass_W > 0) {  // the window's sums: state of a dense-adapting engine alone
      const size_t NC = (size_t)((e->N + DMASS_CH - 1) / DMASS_CH);
      if ((rc = e->dmass_a.alloc((size_t)DP)) || (rc = e->dmass_S1.alloc(NC * DP)) || (rc = e->dmass_S2.alloc(NC * dmass_s2_doubles(DP))) ||
          (rc = e->dmass_work.alloc((size_t)DP * DP)))
        return rc;
      HIP_TRY(hipMemsetAsync(e->dmass_a.p, 0, e->dmass_a.n * sizeof(double), e->stream));
      HIP_TRY(hipMemsetAsync(e->dmass_S1.p, 0, e->dmass_S1.n * sizeof(double), e->stream));
      HIP_TRY(hipMemsetAsync(e->dmass_S2.p, 0, e->dmass_S2.n * sizeof(double), e->stream));
      HIP_TRY(hipMemsetAsync(e->dmass_work.p, 0, e->dmass_work.n * sizeof(double), e->stream));
    } else {
      e->dmass_a.release();
      e->dmass_S1.release();
      e->dmass_S2.release();
      e->dmass_work.release();
    }
    if (leapfrog_proposal(e->pp.kind) && e->dmass_W > 0) {  // (its count of refusals)
      if ((rc = e->mass_refused.alloc(1))) return rc;
      HIP_TRY(hipMemsetAsync(e->mass_refused.p, 0, sizeof(unsigned int), e->stream));
      e->mass_mean.release();
      e->mass_M2.release();
    } else if (leapfrog_proposal(e->pp.kind) && e->mass_W > 0) {  // the window's moments: state of a mass-adapting engine alone
      if ((rc = e->mass_mean.alloc((size_t)NP * DP)) || (rc = e->mass_M2.alloc((size_t)NP * DP)) || (rc = e->mass_refused.alloc(1))) return rc;
      HIP_TRY(hipMemsetAsync(e->mass_mean.p, 0, (size_t)NP * DP * sizeof(double), e->stream));
      HIP_TRY(hipMemsetAsync(e->mass_M2.p, 0, (size_t)NP * DP * sizeof(double), e->stream));
      HIP_TRY(hipMemsetAsync(e->mass_refused.p, 0, sizeof(unsigned int), e->stream));
    } else {
      e->mass_mean.release();
      e->mass_M2.release();
      e->mass_refused.release();
    }
  } else if (mala) {
    // linear model: gradient of the log-posterior of the linear-Gaussian target (proposal.py:986-998; utils.py:273-287) in
    // closed form, grad = c - H theta with
    //   H = Sigma_prior^-1 + A^T Sigma_e^-1 A,   c = Sigma_prior^-1 mu + A^T Sigma_e^-1 (data - b)
    const Level& lv0 = e->levels[0];
    const int m = lv0.m;
    std::vector<double> Wp, H((size_t)DP * DP, 0.0), cv(DP, 0.0);
    tri_inverse_host(e->prior_L_h, d, Wp);
    for (int i = 0; i < d; ++i)
      for (int j = 0; j <= i; ++j) {
        double sacc = 0.0;
        for (int k = i; k < d; ++k) sacc += Wp[(size_t)k * d + i] * Wp[(size_t)k * d + j];
        H[(size_t)i * DP + j] = H[(size_t)j * DP + i] = sacc;
      }
    for (int i = 0; i < d; ++i) {
      double sacc = 0.0;
      for (int j = 0; j < d; ++j) sacc += H[(size_t)i * DP + j] * e->prior_mean_h[j];
      cv[i] = sacc;
    }
    // WA = Sigma_e^-1 A  [m][d]
    std::vector<double> WA((size_t)m * d, 0.0);
    if (lv0.noise_kind == TDA_NOISE_DENSE) {
      for (int o = 0; o < m; ++o)
        for (int q = 0; q < m; ++q) {
          const double pv = lv0.Pinv_h[(size_t)o * m + q];
          for (int j = 0; j < d; ++j) WA[(size_t)o * d + j] += pv * lv0.A_h[(size_t)q * d + j];
        }
    } else {
      for (int o = 0; o < m; ++o) {
        const double wv = lv0.noise_kind == TDA_NOISE_DIAG ? lv0.w_h[o] : 1.0 / lv0.var;
        for (int j = 0; j < d; ++j) WA[(size_t)o * d + j] = wv * lv0.A_h[(size_t)o * d + j];
      }
    }
    for (int o = 0; o < m; ++o)
      for (int i = 0; i < d; ++i) {
        const double ai = lv0.A_h[(size_t)o * d + i];
        for (int j = 0; j < d; ++j) H[(size_t)i * DP + j] += ai * WA[(size_t)o * d + j];
      }
    for (int o = 0; o < m; ++o)
      for (int j = 0; j < d; ++j) cv[j] += WA[(size_t)o * d + j] * lv0.ytil_h[o];
    if ((rc = e->mala_H.upload(H))) return rc;
    if ((rc = e->mala_c.upload(cv))) return rc;
    if ((rc = e->mala_grad.alloc((size_t)NP * DP))) return rc;
  } else if (owcn && e->ow_spectral) {
    // per-chain operators: the increments are w = V^T chol(C_prior) z, eigen-coordinates of the prior draw (k_mh_steps, PX = 3)
    for (int j = 0; j < d; ++j)
      for (int k = 0; k < d; ++k) {
        double g = 0.0;
        for (int i = k; i < d; ++i) g = std::fma(e->ow_V_h[(size_t)i * d + j], L[(size_t)i * d + k], g);
        Lk[(size_t)k * DP + j] = g;
      }
    std::vector<double> VV((size_t)2 * DP * DP, 0.0), lam(DP, 0.0);
    for (int i = 0; i < d; ++i) {
      lam[i] = e->ow_lam_h[i];
      for (int j = 0; j < d; ++j) {
        VV[(size_t)i * DP + j] = e->ow_V_h[(size_t)i * d + j];                    // V[i][j]
        VV[(size_t)DP * DP + (size_t)j * DP + i] = e->ow_V_h[(size_t)i * d + j];  // V^T[j][i]
      }
    }
    if ((rc = e->ow_VVt.upload(VV)) || (rc = e->ow_lam.upload(lam))) return rc;
  } else if (owcn) {
    // increments = noise_operator N(0, C_prior) = (noise_operator chol(C_prior)) z (proposal.py:596-598): a full factor
    for (int j = 0; j < d; ++j)
      for (int k = 0; k < d; ++k) {
        double g = 0.0;
        for (int i = k; i < d; ++i) g = std::fma(e->ow_noise_h[(size_t)j * d + i], L[(size_t)i * d + k], g);
        Lk[(size_t)k * DP + j] = g;
      }
    std::vector<double> St((size_t)DP * DP, 0.0);
    for (int i = 0; i < d; ++i)
      for (int j = 0; j < d; ++j) St[(size_t)j * DP + i] = e->ow_state_h[(size_t)i * d + j];
    if ((rc = e->ow_SopT.upload(St))) return rc;
  } else {
    for (int j = 0; j < d; ++j)
      for (int k = 0; k <= j; ++k) Lk[(size_t)k * DP + j] = L[(size_t)j * d + k];
  }
  if (e->wide) {
    // 65 .. 128 parameters (tda_kernels_wide.h): the factor as tiles -- U = L^T off the diagonal in the factor form's order, the
    // diagonal tiles U_pp beside them -- in TWO buffers per chain (AdaptiveMetropolis: the swap writes the one that is not current)
    // or one shared set; the padding "Sigma_e" of the swap's factorisation
    std::vector<double> fac, ud;
    wide_factor_pack_host(L, d, fac, ud);
    const bool am = e->pp.kind == TDA_PROP_AM;
    e->L_shared = !am;
    const int64_t NPf = am ? NP : 1;
    if ((rc = e->Lk.alloc((size_t)2 * NPf * WIDE_FACTOR_DOUBLES)) || (rc = e->wide_ud.alloc((size_t)2 * NPf * WIDE_UD_DOUBLES))) return rc;
    if ((rc = e->wide_sel.alloc(NP))) return rc;
    HIP_TRY(hipMemsetAsync(e->wide_sel.p, 0, NP * sizeof(int32_t), e->stream));
    auto replicate = [&](double* dst, const std::vector<double>& one) -> int {  // buffer 0 of every chain (buffer 1: written by the first swap)
      const size_t n1 = one.size();
      HIP_TRY(hipMemcpyAsync(dst, one.data(), n1 * sizeof(double), hipMemcpyHostToDevice, e->stream));
      for (int64_t have = 1; have < NPf; have *= 2)
        HIP_TRY(hipMemcpyAsync(dst + (size_t)have * n1, dst, (size_t)std::min<int64_t>(have, NPf - have) * n1 * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
      return TDA_OK;
    };
    if ((rc = replicate(e->Lk.p, fac)) || (rc = replicate(e->wide_ud.p, ud))) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));  // (fac / ud are locals)
    if (am) {
      std::vector<double> pc(WIDE_FACTOR_DOUBLES, 0.0);  // upper tiles: zero inside the d parameters, identity in the padding
      for (int i = d; i < 128; ++i) pc[aemr_u_offset(128, i, i)] = 1.0;
      if ((rc = e->wide_cov.upload(pc))) return rc;
      // RecursiveSampleMoments(mu0 = theta0, sigma0 = 0) (proposal.py:495-500): Sigma as its 36 UPPER tiles (k_wide_adapt)
      if ((rc = e->am_mu.alloc((size_t)NP * DP)) || (rc = e->am_sigma.alloc((size_t)NP * WIDE_FACTOR_DOUBLES))) return rc;
      HIP_TRY(hipMemcpyAsync(e->am_mu.p, e->theta.p, (size_t)NP * DP * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
      HIP_TRY(hipMemsetAsync(e->am_sigma.p, 0, (size_t)NP * WIDE_FACTOR_DOUBLES * sizeof(double), e->stream));
    }
  } else if (e->pp.kind == TDA_PROP_AM) {
    e->L_shared = false;
    if ((rc = e->Lk.alloc((size_t)NP * DP * DP))) return rc;
    // one factor over PCIe, replicated to every chain by doubling device copies (the 128 MiB of 4096 copies took 10 ms from
    // pageable host memory)
    HIP_TRY(hipMemcpyAsync(e->Lk.p, Lk.data(), (size_t)DP * DP * sizeof(double), hipMemcpyHostToDevice, e->stream));
    for (int64_t have = 1; have < NP; have *= 2)
      HIP_TRY(hipMemcpyAsync(e->Lk.p + (size_t)have * DP * DP, e->Lk.p, (size_t)std::min<int64_t>(have, NP - have) * DP * DP * sizeof(double),
                             hipMemcpyDeviceToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));  // (Lk is a local: the first copy must have left the host before it goes)
    // RecursiveSampleMoments(mu0 = theta0, sigma0 = 0) (proposal.py:495-500)
    if ((rc = e->am_mu.alloc((size_t)NP * DP))) return rc;
    const size_t nsig = (size_t)NP * am_tiles_rt(DP) * 256;  // lower 16x16 tiles in MFMA C/D layout (k_adapt)
    if ((rc = e->am_sigma.alloc(nsig))) return rc;
    HIP_TRY(hipMemcpyAsync(e->am_mu.p, e->theta.p, (size_t)NP * DP * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
    HIP_TRY(hipMemsetAsync(e->am_sigma.p, 0, nsig * sizeof(double), e->stream));
  } else {
    e->L_shared = true;
    if ((rc = e->Lk.upload(Lk))) return rc;
  }
  e->L_identity = false;
  if (e->L_shared && (e->pp.kind == TDA_PROP_GRW || e->pp.kind == TDA_PROP_PCN)) {
    bool ident = true;
    for (int k = 0; k < d && ident; ++k)
      for (int j = 0; j < d; ++j)
        if (Lk[(size_t)k * DP + j] != (j == k ? 1.0 : 0.0)) {
          ident = false;
          break;
        }
    e->L_identity = ident;
  }
  }

  // block buffers
  if (!e->is_dreamz && (rc = e->inc.alloc((size_t)e->SMAX * NP * DP))) return rc;
  if ((rc = e->ublk.alloc((size_t)e->SMAX * NP))) return rc;
  if ((rc = e->lublk.alloc((size_t)e->SMAX * NP))) return rc;
  if ((rc = e->rec_params.alloc((size_t)e->SMAX * N * d))) return rc;
  if ((rc = e->rec_stats.alloc((size_t)e->SMAX * N * 3))) return rc;
  if ((rc = e->rec_acc.alloc((size_t)e->SMAX * N))) return rc;

  e->t = 0;
  e->k_adapt = 0;
  e->rep_pos = 0;
  e->exp_pos = 0;
  // initial links (chain.py:70)
  if ((rc = launch_eval(e, 0, e->theta.p, e->lp.p, e->ll.p))) return rc;
  if (user_mala) {
    UserMalaArgs ga{};
    if ((rc = fill_user_mala_args(e, e->levels[0], ga))) return rc;
    if ((rc = launch_user(e->levels[0].uprog_mala.grad0, ga, user_mala_lds(e->levels[0].uprog_mala.spec, ga.m), e->stream))) return rc;
  } else if (mala) {
    const int64_t nt = NP * DP;
    hipLaunchKernelGGL(k_mala_grad0, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, e->stream, NP, DP, e->mala_H.p, e->mala_c.p,
                       e->theta.p, e->mala_grad.p);
    HIP_TRY(hipGetLastError());
  }
  if (e->nlev > 1) {
    // every level starts from theta0 (chain.py:253-261; proposal.py:1379); S[j][q] = level j's densities there
    if (!e->sub_set) return fail(TDA_ERR_STATE, "set_subchains must precede init for n_levels > 1");
    const int nl = e->nlev, npair = nl * (nl - 1) / 2;
    if ((rc = e->ml_theta.alloc((size_t)nl * NP * DP))) return rc;
    if ((rc = e->ml_lp.alloc((size_t)nl * NP))) return rc;
    if ((rc = e->ml_ll.alloc((size_t)nl * NP))) return rc;
    if ((rc = e->ml_S.alloc((size_t)npair * 2 * NP))) return rc;
    if ((rc = e->ml_anyacc.alloc((size_t)nl * NP))) return rc;
    if ((rc = e->ml_ysnap.alloc((size_t)NP * (DP + 2)))) return rc;
    if ((rc = e->ml_pick.alloc(NP))) return rc;
    e->ring_P = e->pp.adaptive ? e->pp.period + MAXLEV : 1;
    if ((rc = e->ml_ring.alloc((size_t)e->ring_P * NP))) return rc;
    HIP_TRY(hipMemsetAsync(e->ml_anyacc.p, 0, (size_t)nl * NP * sizeof(int32_t), e->stream));
    HIP_TRY(hipMemsetAsync(e->ml_ysnap.p, 0, (size_t)NP * (DP + 2) * sizeof(double), e->stream));
    HIP_TRY(hipMemsetAsync(e->ml_pick.p, 0, NP * sizeof(int32_t), e->stream));
    HIP_TRY(hipMemsetAsync(e->ml_ring.p, 0, (size_t)e->ring_P * NP, e->stream));
    for (int k = 0; k < nl; ++k) {
      double* thk = e->ml_theta.p + (size_t)k * NP * DP;
      HIP_TRY(hipMemcpyAsync(thk, e->theta.p, (size_t)NP * DP * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
      if ((rc = launch_eval(e, k, thk, e->ml_lp.p + (size_t)k * NP, e->ml_ll.p + (size_t)k * NP))) return rc;
    }
    for (int q = 1; q < nl; ++q)
      for (int j = 0; j < q; ++j) {
        const int p = q * (q - 1) / 2 + j;
        HIP_TRY(hipMemcpyAsync(e->ml_S.p + ((size_t)p * 2 + 0) * NP, e->ml_lp.p + (size_t)j * NP, NP * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(e->ml_S.p + ((size_t)p * 2 + 1) * NP, e->ml_ll.p + (size_t)j * NP, NP * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
      }
    for (int k = 0; k < MAXLEV; ++k) {
      e->cnt[k] = 0;
      e->done[k] = 0;
      e->u_rep_lv_pos[k] = 0;
    }
    e->ridx_rep_pos = 0;
    e->ring_pos = 0;
    for (int k = 0; k < nl; ++k) {
      if ((rc = e->ml_rec_params[k].alloc((size_t)e->SMAX * N * d))) return rc;
      if ((rc = e->ml_rec_stats[k].alloc((size_t)e->SMAX * N * 3))) return rc;
      if ((rc = e->ml_rec_acc[k].alloc((size_t)e->SMAX * N))) return rc;
    }
    if ((rc = e->ml_sid.alloc((size_t)nl * NP))) return rc;
    HIP_TRY(hipMemsetAsync(e->ml_sid.p, 0, (size_t)nl * NP * sizeof(int64_t), e->stream));
    if (e->aem == TDA_AEM_STATE_INDEPENDENT_DIAGONAL) {
      if ((rc = init_error_model_diagonal(e))) return rc;
    } else if (e->aem) {
      // ---- adaptive error model set-up (chain.py:268-305; :643-678; proposal.py:1407-1467) ----
      if (e->randomize) return fail(TDA_ERR_UNSUPPORTED, "randomize_subchain_length together with an error model is not lowered");
      if (e->prior_kind == PRIOR_DENSE && e->aem == TDA_AEM_STATE_DEPENDENT && e->pp.kind != TDA_PROP_PCN) {}
      const int m = e->levels[0].m;
      for (int k = 0; k < nl; ++k) {
        if (e->levels[k].m != m) return fail(TDA_ERR_INVALID, "error model: all levels must share the output dimension");
        const bool want_adaptive = k < nl - 1;
        if (want_adaptive && e->levels[k].noise_kind != TDA_NOISE_ADAPTIVE)
          return fail(TDA_ERR_INVALID, "error model: level %d needs an AdaptiveGaussianLogLike (TDA_NOISE_ADAPTIVE)", k);
        if (!want_adaptive && e->levels[k].noise_kind != TDA_NOISE_ISO)
          return fail(TDA_ERR_UNSUPPORTED, "error model: the finest level must have an isotropic likelihood on the device");
      }
      e->aem_m = m;
      const int AEM_MP = e->aem_ld = e->levels[0].em_ld;
      if (e->ext_hier && AEM_MP > AEM_MP_MAX_EXT)
        return fail(TDA_ERR_UNSUPPORTED, "dense error model with more than %d outputs: hierarchies of the engine's linear levels only (no callback / source-defined level, no DREAM(Z) below)", (int)AEM_MP_MAX_EXT);
      HIP_TRY(hipStreamSynchronize(e->stream));
      // host copies of theta0 / log-priors, model outputs of every level
      std::vector<double> th((size_t)NP * DP), lph(NP);
      HIP_TRY(hipMemcpy(th.data(), e->theta.p, th.size() * sizeof(double), hipMemcpyDeviceToHost));
      std::vector<std::vector<double>> F(nl, std::vector<double>((size_t)N * m));
      if (e->ext_hier) {
        // callback / source-defined (and linear) levels of a host-sequenced hierarchy: the model outputs at theta0 come
        // from the same evaluation path the steps use
        for (int k = 0; k < nl; ++k) {
          const Level& lvk = e->levels[k];
          ExtArgs ya{};
          fill_ext_args(e, lvk, ya);
          ya.mode = 1;
          ya.theta = e->theta.p;
          ya.scaling = e->scaling.p;
          hipLaunchKernelGGL(k_ext_propose, dim3((unsigned)((N + EXT_WAVES - 1) / EXT_WAVES)), dim3(64 * EXT_WAVES), 0, e->stream, ya);
          if ((rc = ext_model_outputs(e, lvk))) return rc;
          HIP_TRY(hipStreamSynchronize(e->stream));
          HIP_TRY(hipMemcpy(F[k].data(), lvk.cb_F.p, F[k].size() * sizeof(double), hipMemcpyDeviceToHost));
          for (int64_t c = 0; c < N; ++c)
            for (int o = 0; o < m; ++o) F[k][(size_t)c * m + o] -= lvk.data_h[o];  // residual form; Fout() adds the data back
        }
      } else
      for (int k = 0; k < nl; ++k)
        for (int64_t c = 0; c < N; ++c)
          for (int o = 0; o < m; ++o) {
            double f = 0.0;
            for (int j = 0; j < d; ++j) f = std::fma(e->levels[k].A_h[(size_t)o * d + j], th[(size_t)c * DP + j], f);
            F[k][(size_t)c * m + o] = f - e->levels[k].ytil_h[o];  // F - y + (y - ytil) handled below: residual form
          }
      // residual r_k = F_k - ytil_k ; model output F_k = r_k + ytil_k + b_k - b_k ... differences of outputs:
      // F_q - F_{q-1} = (r_q + y_q) - (r_{q-1} + y_{q-1}) with y = data (ytil = data - b, F = A theta + b)
      auto Fout = [&](int k, int64_t c, int o) { return F[k][(size_t)c * m + o] + e->levels[k].data_h[o]; };
      std::vector<std::vector<double>> mdiff(nl, std::vector<double>((size_t)NP * AEM_MP, 0.0));
      for (int q = 1; q < nl; ++q)
        for (int64_t c = 0; c < N; ++c)
          for (int o = 0; o < m; ++o) mdiff[q][(size_t)c * AEM_MP + o] = Fout(q, c, o) - Fout(q - 1, c, o);
      for (int q = 1; q < nl; ++q) {
        if ((rc = e->aem_mdiff[q].upload(mdiff[q]))) return rc;
        if ((rc = e->aem_bmu[q].upload(mdiff[q]))) return rc;  // RecursiveSampleMoments(mu0 = model_diff, sigma0 = 0)
        // tracker covariance: upper 16 x 16 tiles in the MFMA C/D layout (tda_kernels_aemr.h), Sigma_0 = 0
        if ((rc = e->aem_bsig[q].alloc((size_t)NP * aemr_v_doubles(AEM_MP)))) return rc;
        HIP_TRY(hipMemset(e->aem_bsig[q].p, 0, (size_t)NP * aemr_v_doubles(AEM_MP) * sizeof(double)));
        e->aem_bt[q] = 1;
      }
      std::vector<double> llh(NP, 0.0);
      if ((rc = e->aem_rvec.alloc((size_t)NP * AEM_MP))) return rc;
      HIP_TRY(hipMemset(e->aem_rvec.p, 0, (size_t)NP * AEM_MP * sizeof(double)));
      if ((rc = e->aem_upd.alloc((size_t)NP * 3 * AEM_MP))) return rc;
      HIP_TRY(hipMemset(e->aem_upd.p, 0, (size_t)NP * 3 * AEM_MP * sizeof(double)));
      if ((rc = e->aem_F.alloc((size_t)4 * NP * AEM_MP))) return rc;
      HIP_TRY(hipMemset(e->aem_F.p, 0, (size_t)4 * NP * AEM_MP * sizeof(double)));
      for (int k = 0; k < nl - 1; ++k) {
        // Sigma_e^-1 (distributions.py:280) as the Cholesky factor of Sigma_e = L L^T (r^T Sigma_e^-1 r = |L^-1 r|^2) in the factor form
        // of tda_kernels_aemr.h; identical for all chains until a bias covariance exceeds 1e-9.  Padding: identity.
        std::vector<double> Lc, W;
        cholesky_host(e->levels[k].cov_h.data(), m, Lc);
        tri_inverse_host(Lc, m, W);
        const size_t VD = aemr_v_doubles(AEM_MP);
        std::vector<double> V0;
        factor_form_pack_host(Lc, m, AEM_MP, V0);
        if ((rc = e->aem_covinv[k].alloc((size_t)NP * VD))) return rc;
        HIP_TRY(hipMemcpy(e->aem_covinv[k].p, V0.data(), VD * sizeof(double), hipMemcpyHostToDevice));
        for (int64_t have = 1; have < NP; have *= 2)  // replicate to every chain by doubling device copies
          HIP_TRY(hipMemcpy(e->aem_covinv[k].p + (size_t)have * VD, e->aem_covinv[k].p,
                            (size_t)std::min<int64_t>(have, NP - have) * VD * sizeof(double), hipMemcpyDeviceToDevice));
        // total bias: state-dependent = the difference itself, otherwise the sum of the means of all trackers above
        std::vector<double> bt((size_t)NP * AEM_MP, 0.0);
        for (int64_t c = 0; c < N; ++c)
          for (int o = 0; o < m; ++o) {
            double s = 0.0;
            if (e->aem == TDA_AEM_STATE_DEPENDENT) s = mdiff[k + 1][(size_t)c * AEM_MP + o];
            else
              for (int p = k + 1; p < nl; ++p) s += mdiff[p][(size_t)c * AEM_MP + o];
            bt[(size_t)c * AEM_MP + o] = s;
          }
        if ((rc = e->aem_bias[k].upload(bt))) return rc;
        // update_link of the initial link of level k
        for (int64_t c = 0; c < N; ++c) {
          double acc = 0.0;
          for (int i = 0; i < m; ++i) {  // |L^-1 r|^2
            double z = 0.0;
            for (int j = 0; j <= i; ++j) z += W[(size_t)i * m + j] * (F[k][(size_t)c * m + j] + bt[(size_t)c * AEM_MP + j]);
            acc += z * z;
          }
          llh[c] = -0.5 * acc;
        }
        HIP_TRY(hipMemcpy(e->ml_ll.p + (size_t)k * NP, llh.data(), NP * sizeof(double), hipMemcpyHostToDevice));
      }
      // S[j][q] = densities of level j at theta0 under the initial error model
      for (int qq = 1; qq < nl; ++qq)
        for (int j = 0; j < qq; ++j) {
          const int p = qq * (qq - 1) / 2 + j;
          HIP_TRY(hipMemcpy(e->ml_S.p + ((size_t)p * 2 + 0) * NP, e->ml_lp.p + (size_t)j * NP, NP * sizeof(double), hipMemcpyDeviceToDevice));
          HIP_TRY(hipMemcpy(e->ml_S.p + ((size_t)p * 2 + 1) * NP, e->ml_ll.p + (size_t)j * NP, NP * sizeof(double), hipMemcpyDeviceToDevice));
        }
      if (e->ext_hier) {  // model outputs of the current links and of level j at theta_q: all at theta0
        const int npair = nl * (nl - 1) / 2;
        std::vector<std::vector<double>> Fo(nl, std::vector<double>((size_t)NP * AEM_MP, 0.0));
        for (int k = 0; k < nl; ++k) {
          for (int64_t c = 0; c < N; ++c)
            for (int o = 0; o < m; ++o) Fo[k][(size_t)c * AEM_MP + o] = Fout(k, c, o);
          if ((rc = e->ext_Fcur[k].upload(Fo[k]))) return rc;
        }
        if ((rc = e->ext_Fst.alloc((size_t)npair * NP * AEM_MP))) return rc;
        for (int qq = 1; qq < nl; ++qq)
          for (int j = 0; j < qq; ++j)
            HIP_TRY(hipMemcpy(e->ext_Fst.p + (size_t)(qq * (qq - 1) / 2 + j) * NP * AEM_MP, Fo[j].data(), Fo[j].size() * sizeof(double), hipMemcpyHostToDevice));
      }
      // whitening matrix of the prior, row-major (pCN transition densities of the state-dependent acceptance)
      std::vector<double> Wp;
      tri_inverse_host(e->prior_L_h, d, Wp);
      if ((rc = e->prior_W_rm.upload(Wp))) return rc;
    }
  }
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->inited = true;
  return TDA_OK;
}

}  // extern "C"
