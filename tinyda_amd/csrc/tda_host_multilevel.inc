// Part of libtinyda_hip.so: included by tda_engine.hip (ONE translation unit -- the helpers, the engine struct and the kernel
// launchers above it are visible here).  Multilevel drivers: host-sequenced hierarchies (run_ext_hierarchy_block) and the fused level kernels (run_multilevel).
extern "C" {

// One block of S base steps of a hierarchy whose levels live outside the fused level kernel (run_multilevel): batched host
// callbacks, source-defined models, linear levels beside them.  `ma` carries the block's buffers (increments, uniforms,
// record rows per level, replay pointers) exactly as the fused kernel would get them.
static int run_ext_hierarchy_block(tda_engine* e, const MLArgs& ma, int64_t S, bool adaptive) {
  const int nl = e->nlev, d = e->d, DP = e->DP;
  const int64_t N = e->N, NP = e->NP;
  // every base step is propose -> model(level 0) -> accept; when the subchain of level k completes, level k + 1's model is
  // evaluated at the states of level k (one evaluation for all chains) and k_ext_level_action decides, aligns and records
  // (the cascade of k_ml_steps, one level at a time)
  const unsigned grid = (unsigned)((N + EXT_WAVES - 1) / EXT_WAVES);
  int cc[MAXLEV];
  int64_t row[MAXLEV] = {0, 0, 0, 0};
  int64_t rp = e->ring_pos;  // position in the base proposal's accepted list: one entry per base step and per level action
  for (int k = 0; k < MAXLEV; ++k) cc[k] = e->cnt[k];
  // diagonal error model over a hierarchy of linear levels: base subchains in the fused level kernel (TINYDA_AEMD_FUSED=0: one
  // propose / outputs / accept triple per base step, for A/B measurements); the residual tile of level 0 must fit into LDS
  static const bool aemd_fused_ok = env_int("TINYDA_AEMD_FUSED", 1) != 0;
  bool all_linear = true;
  for (int k = 0; k < nl; ++k) all_linear = all_linear && e->levels[k].model == MODEL_LINEAR && e->levels[k].Apk.p != nullptr;
  // (LDS of k_ml_steps with only the base level staged: proposal tile, reduction slabs, level 0's data [and weights], prior rows,
  // the residual tile; lds_y[0] = 0, so the base level's slab is the first of the staging region)
  const int stage0 = e->levels[0].m_pad * (e->levels[0].noise_kind == TDA_NOISE_DIAG ? 2 : 1);
  const size_t aemd_lds = ((size_t)16 * (DP + 2) + 128 + stage0 + (e->prior_kind == PRIOR_DENSE ? e->prior_ncb * 16 : 0) +
                           16 * (e->levels[0].m_pad + 2) + 16) * sizeof(double);
  const bool aemd_fused = aemd_fused_ok && e->aem == TDA_AEM_STATE_INDEPENDENT_DIAGONAL && all_linear && !e->randomize && !e->is_dreamz &&
                          aemd_lds <= 160 * 1024;
  bool fused_base_ran = false;
  // DREAMZ base step (proposal.py:811-852 / :790-809): the block's draws are in dz_coef / dz_epsm / dz_ridx (k_dreamz_draw); the
  // jump comes from the chain's own archive, the state the chain is left in is appended to it
  auto dz_args = [&](int64_t s) {
    DzExtArgs za{};
    za.N = N;
    za.NP = NP;
    za.d = d;
    za.DP = DP;
    za.delta = e->dz.delta;
    za.s = (int)s;
    za.shared = 0;
    za.jump_ready = 0;
    za.M_base = e->arch_rows;
    za.cap = e->arch_cap;
    za.arch = e->arch.p;
    za.theta = e->ml_theta.p;
    za.coef = e->dz_coef.p;
    za.epsm = e->dz_epsm.p;
    za.ridx = e->dz_ridx.p;
    za.prop = e->levels[0].cb_prop.p;
    za.blk_states = nullptr;
    return za;
  };
  for (int64_t s = 0; s < S;) {
    if (e->randomize && cc[0] == 0) {  // Delayed Acceptance: draw the promoted index of the subchain that starts now
      hipLaunchKernelGGL(k_ext_pick, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, e->stream, (long long)N, e->sl[0],
                         (unsigned long long)e->cfg.seed, (long long)e->cfg.chain_offset, (long long)(e->done[1] + row[1]),
                         ma.ridx_rep ? ma.ridx_rep + (size_t)row[1] * N : nullptr, e->ml_pick.p);
    }
    if (e->levels[0].model == MODEL_USER && !e->aem && !e->randomize && !e->is_dreamz && e->levels[0].noise_kind != TDA_NOISE_DENSE) {
      // source-defined base level: the rest of the running subchain (inside this block) is ONE launch of the fused
      // step kernel compiled with the model
      const int64_t n = std::min<int64_t>(S - s, (int64_t)e->sl[0] - cc[0]);
      UserStepArgs ua{};
      int urc = fill_user_args(e, e->levels[0], ua);
      if (urc) return urc;
      ua.S = (int)n;
      ua.mode = 0;
      ua.prop_kind = e->pp.kind;
      ua.theta = e->ml_theta.p;
      ua.lp = e->ml_lp.p;
      ua.ll = e->ml_ll.p;
      ua.scaling = e->scaling.p;
      ua.acc_count = nullptr;
      ua.inc = e->inc.p + (size_t)s * NP * DP;
      ua.u = e->ublk.p + (size_t)s * NP;
      ua.rec_params = ma.rec_params[0] ? ma.rec_params[0] + (size_t)s * N * d : nullptr;
      ua.rec_stats = ma.rec_stats[0] ? ma.rec_stats[0] + (size_t)s * N * 3 : nullptr;
      ua.rec_acc = ma.rec_acc[0] ? ma.rec_acc[0] + (size_t)s * N : nullptr;
      ua.anyacc = e->ml_anyacc.p;
      ua.ring = adaptive ? e->ml_ring.p : nullptr;
      ua.ring_P = e->ring_P;
      ua.ring_pos = rp;
      if ((urc = launch_user(e->levels[0].uprog.steps, ua, e->levels[0].uprog.out_lds, e->stream))) return urc;
      rp += n;
      s += n;
      cc[0] += (int)n;
    } else if (aemd_fused) {
      // diagonal error model over linear levels: the rest of the running base subchain (inside this block) is ONE launch of the
      // fused level kernel with the corrected likelihood (k_ml_steps, aem_on = 2: bias and inverse variances of chain c from
      // the arrays the level actions maintain) instead of propose / outputs / accept launches per base step
      const int64_t n = std::min<int64_t>(S - s, (int64_t)e->sl[0] - cc[0]);
      MLArgs mb = ma;
      mb.S = (int)n;
      mb.cascade = 0;
      mb.randomize = 0;
      mb.aem_on = 2;
      mb.aem_mp = e->levels[0].m_pad;
      mb.aem_ld = e->levels[0].m;
      mb.aem_bias = e->aemd_bias[0].p;
      mb.aem_P = e->aemd_w[0].p;
      mb.lds_total = stage0;
      mb.inc = e->inc.p + (size_t)s * NP * DP;
      mb.u0 = e->ublk.p + (size_t)s * NP;
      mb.logu0 = nullptr;
      mb.cnt[0] = cc[0];
      mb.done[0] = e->done[0] + s;
      mb.ring_pos = rp;
      mb.rec_params[0] = ma.rec_params[0] ? ma.rec_params[0] + (size_t)s * N * d : nullptr;
      mb.rec_stats[0] = ma.rec_stats[0] ? ma.rec_stats[0] + (size_t)s * N * 3 : nullptr;
      mb.rec_acc[0] = ma.rec_acc[0] ? ma.rec_acc[0] + (size_t)s * N : nullptr;
      int lrc = TDA_OK;
      DISPATCH_DPAD(DP, lrc = launch_ml<DPAD>(mb, NP / 16, aemd_lds, e->stream));
      if (lrc) return lrc;
      HIP_TRY(hipGetLastError());
      fused_base_ran = true;
      rp += n;
      s += n;
      cc[0] += (int)n;
    } else if (e->aem == TDA_AEM_STATE_INDEPENDENT_DIAGONAL) {
      // base step under the corrected diagonal likelihood (per-chain bias and inverse variances, tda_kernels_aemd.h)
      const Level& l0 = e->levels[0];
      ExtArgs pa2{};
      fill_ext_args(e, l0, pa2);
      pa2.mode = 0;
      pa2.prop_kind = e->pp.kind;
      pa2.theta = e->ml_theta.p;
      pa2.scaling = e->scaling.p;
      pa2.inc = e->inc.p;
      pa2.s = (int)s;
      hipLaunchKernelGGL(k_ext_propose, dim3(grid), dim3(64 * EXT_WAVES), 0, e->stream, pa2);
      int mrc0 = ext_model_outputs(e, l0);
      if (mrc0) return mrc0;
      AemdArgs da{};
      fill_aemd_args(e, da);
      da.s = (int)s;
      da.F = l0.cb_F.p;
      da.prop = l0.cb_prop.p;
      da.u0 = e->ublk.p;
      da.sid_value = e->done[0] + s + 1;
      da.ring = adaptive ? e->ml_ring.p : nullptr;
      da.ring_P = e->ring_P;
      da.ring_pos = rp++;
      da.rec_params = ma.rec_params[0];
      da.rec_stats = ma.rec_stats[0];
      da.rec_acc = ma.rec_acc[0];
      hipLaunchKernelGGL(k_aemd_accept, dim3(grid), dim3(64 * EXT_WAVES), 0, e->stream, da);
      HIP_TRY(hipGetLastError());
      cc[0] += 1;
      s += 1;
    } else if (e->aem) {
      // base step under the bias-corrected likelihood of the error model (per-chain bias and inverse)
      const Level& l0 = e->levels[0];
      if (e->is_dreamz) {  // DREAMZ at the base (round 3): its jump instead of the Gaussian increment, the same corrected acceptance
        if (s == S - 1)  // jumping distance of the crossover adaptation: the state before the block's last base step
          HIP_TRY(hipMemcpyAsync(e->theta_prev.p, e->ml_theta.p, (size_t)NP * DP * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
        hipLaunchKernelGGL(k_dz_ext_propose, dim3(grid), dim3(64 * EXT_WAVES), 0, e->stream, dz_args(s));
      } else {
      ExtArgs pa2{};
      fill_ext_args(e, l0, pa2);
      pa2.mode = 0;
      pa2.prop_kind = e->pp.kind;
      pa2.theta = e->ml_theta.p;
      pa2.scaling = e->scaling.p;
      pa2.inc = e->inc.p;
      pa2.s = (int)s;
      hipLaunchKernelGGL(k_ext_propose, dim3(grid), dim3(64 * EXT_WAVES), 0, e->stream, pa2);
      }
      int mrc0 = ext_model_outputs(e, l0);
      if (mrc0) return mrc0;
      ExtAemAcceptArgs ea{};
      ea.N = N;
      ea.NP = NP;
      ea.d = d;
      ea.DP = DP;
      ea.m = e->aem_m;
      ea.MP = e->aem_ld;
      ea.s = (int)s;
      ea.prop_kind = e->is_dreamz ? TDA_PROP_GRW : e->pp.kind;  // DREAMZ: acceptance on the posterior ratio (proposal.py:253-258)
      ea.theta = e->ml_theta.p;
      ea.lp = e->ml_lp.p;
      ea.ll = e->ml_ll.p;
      ea.u = e->ublk.p;
      ea.prop = l0.cb_prop.p;
      ea.F = l0.cb_F.p;
      ea.data = l0.data64.p;
      ea.bias = e->aem_bias[0].p;
      ea.P = e->aem_covinv[0].p;
      ea.Fcur = e->ext_Fcur[0].p;
      ea.pr_mean = e->prior_mean.p;
      ea.pr_pinv = e->prior_pinv.p;
      ea.pr_lo = e->prior_bounded ? e->prior_lo.p : nullptr;
      ea.pr_hi = e->prior_bounded ? e->prior_hi.p : nullptr;
      ea.logconst = e->prior_logconst;
      ea.anyacc = e->ml_anyacc.p;
      ea.sid = e->ml_sid.p;
      ea.sid_value = e->done[0] + s + 1;
      ea.ring = adaptive ? e->ml_ring.p : nullptr;
      ea.ring_P = e->ring_P;
      ea.ring_pos = rp++;
      ea.rec_params = ma.rec_params[0];
      ea.rec_stats = ma.rec_stats[0];
      ea.rec_acc = ma.rec_acc[0];
      if (e->aem_ld == 64) hipLaunchKernelGGL(k_ext_aem_accept<64>, dim3((unsigned)N), dim3(64), 0, e->stream, ea);
      else if (e->aem_ld == 128) hipLaunchKernelGGL(k_ext_aem_accept<128>, dim3((unsigned)N), dim3(128), 0, e->stream, ea);
      else hipLaunchKernelGGL(k_ext_aem_accept<256>, dim3((unsigned)N), dim3(256), 0, e->stream, ea);
      if (e->is_dreamz) {
        hipLaunchKernelGGL(k_dz_ext_append, dim3((unsigned)((NP + EXT_WAVES - 1) / EXT_WAVES)), dim3(64 * EXT_WAVES), 0, e->stream, dz_args(s));
        if (s == S - 1)  // ... and the state right after it, before an upper level realigns the chain
          HIP_TRY(hipMemcpyAsync(e->theta_last.p, e->ml_theta.p, (size_t)NP * DP * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
      }
      HIP_TRY(hipGetLastError());
      cc[0] += 1;
      s += 1;
    } else {
    ExtArgs xa{};
    fill_ext_args(e, e->levels[0], xa);
    xa.mode = 0;
    xa.prop_kind = e->pp.kind;
    xa.theta = e->ml_theta.p;
    xa.lp = e->ml_lp.p;
    xa.ll = e->ml_ll.p;
    xa.scaling = e->scaling.p;
    xa.acc_count = nullptr;
    xa.anyacc = e->ml_anyacc.p;
    xa.inc = e->inc.p;
    xa.u = e->ublk.p;
    xa.s = (int)s;
    xa.rec_params = ma.rec_params[0];
    xa.rec_stats = ma.rec_stats[0];
    xa.rec_acc = ma.rec_acc[0];
    xa.ring = adaptive ? e->ml_ring.p : nullptr;
    xa.ring_P = e->ring_P;
    xa.ring_pos = rp++;
    if (e->randomize) {
      xa.pick = e->ml_pick.p;
      xa.cnt = cc[0];
      xa.ysnap = e->ml_ysnap.p;
    }
    if (e->is_dreamz) {
      // DREAMZ base step (proposal.py:811-852 / :790-809): the block's draws are in dz_coef / dz_epsm / dz_ridx (k_dreamz_draw);
      // apply the jump from the chain's archive, evaluate, decide, append the state the chain is left in to its archive
      if (s == S - 1)  // jumping distance of the crossover adaptation: the state before the block's last base step
        HIP_TRY(hipMemcpyAsync(e->theta_prev.p, e->ml_theta.p, (size_t)NP * DP * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
      const DzExtArgs za = dz_args(s);
      hipLaunchKernelGGL(k_dz_ext_propose, dim3(grid), dim3(64 * EXT_WAVES), 0, e->stream, za);
      int mrc = ext_model_outputs(e, e->levels[0]);
      if (mrc) return mrc;
      xa.prop_kind = TDA_PROP_GRW;  // acceptance on the posterior ratio (proposal.py:253-258)
      hipLaunchKernelGGL(k_ext_accept, dim3(grid), dim3(64 * EXT_WAVES), xa.Pd ? (size_t)EXT_WAVES * e->levels[0].m * sizeof(double) : 0,
                         e->stream, xa);
      hipLaunchKernelGGL(k_dz_ext_append, dim3((unsigned)((NP + EXT_WAVES - 1) / EXT_WAVES)), dim3(64 * EXT_WAVES), 0, e->stream, za);
      if (s == S - 1)  // ... and the state right after it, before an upper level realigns the chain
        HIP_TRY(hipMemcpyAsync(e->theta_last.p, e->ml_theta.p, (size_t)NP * DP * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
      HIP_TRY(hipGetLastError());
    } else {
    int xrc = ext_step(e, e->levels[0], xa);
    if (xrc) return xrc;
    }
    cc[0] += 1;
    s += 1;
    }
    if (fused_base_ran && cc[0] == e->sl[0]) {
      // the level actions keep the model output of every level's current link; the fused base kernel does not: F_0(theta_0)
      // for all chains by the same product that evaluates linear levels anywhere else on this path
      linear_outputs_at(e, e->levels[0], e->ml_theta.p, DP, e->aemd_F[0].p);
      fused_base_ran = false;
    }
    for (int k = 0; k < nl - 1 && cc[k] == e->sl[k]; ++k) {
      const int q = k + 1;
      const Level& lq = e->levels[q];
      if (lq.model == MODEL_USER && !e->aem && lq.noise_kind != TDA_NOISE_DENSE) {
        // source-defined level without error model: evaluation, decision, alignment and records in one launch of the
        // kernel compiled with the model (+ the step's uniforms)
        double* ul = e->lublk.p;  // scratch of the single-level path, at least SMAX * NP doubles
        hipLaunchKernelGGL(k_ext_level_uniforms, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, e->stream, (long long)N,
                           (unsigned long long)e->cfg.seed, (long long)e->cfg.chain_offset, (long long)(e->done[q] + row[q]), q,
                           ma.u_rep[q] ? ma.u_rep[q] + (size_t)row[q] * N : nullptr, ul);
        UserLevelArgs ua{};
        fill_user_level(e, lq, ua);
        ua.nlev = nl;
        ua.q = q;
        ua.theta = e->ml_theta.p;
        ua.lp = e->ml_lp.p;
        ua.ll = e->ml_ll.p;
        ua.Sst = e->ml_S.p;
        ua.anyacc = e->ml_anyacc.p;
        ua.u = ul;
        ua.rec_params = ma.rec_params[q] ? ma.rec_params[q] + (size_t)row[q] * N * d : nullptr;
        ua.rec_stats = ma.rec_stats[q] ? ma.rec_stats[q] + (size_t)row[q] * N * 3 : nullptr;
        ua.rec_acc = ma.rec_acc[q] ? ma.rec_acc[q] + (size_t)row[q] * N : nullptr;
        ua.ring = adaptive ? e->ml_ring.p : nullptr;
        ua.ring_P = e->ring_P;
        ua.ring_pos = rp++;
        ua.ysnap = (e->randomize && k == 0) ? e->ml_ysnap.p : nullptr;
        int lrc = launch_user(lq.uprog.level, ua, lq.uprog.out_lds, e->stream);
        if (lrc) return lrc;
        cc[k] = 0;
        cc[q] += 1;
        row[q] += 1;
        continue;
      }
      const bool snap = e->randomize && k == 0;
      if (lq.model == MODEL_LINEAR && lq.Apk.p) {
        // linear level: its outputs at the states of level k straight from the state array (no copy of the states first)
        linear_outputs_at(e, lq, snap ? e->ml_ysnap.p : e->ml_theta.p + (size_t)k * NP * DP, snap ? DP + 2 : DP, lq.cb_F.p);
      } else {
        ExtArgs ya{};
        fill_ext_args(e, lq, ya);
        ya.mode = 1;  // "proposals" = the current states of level k (the promoted states of a randomised subchain)
        ya.theta = snap ? e->ml_ysnap.p : e->ml_theta.p + (size_t)k * NP * DP;
        ya.theta_ld = snap ? DP + 2 : 0;
        hipLaunchKernelGGL(k_ext_propose, dim3(grid), dim3(64 * EXT_WAVES), 0, e->stream, ya);
        const int mrc = ext_model_outputs(e, lq);
        if (mrc) return mrc;
      }
      if (e->aem == TDA_AEM_STATE_INDEPENDENT_DIAGONAL) {  // decision, alignment, tracker, bias, update_link: one launch
        AemdArgs da{};
        fill_aemd_args(e, da);
        da.q = q;
        da.step = e->done[q] + row[q];
        da.F = lq.cb_F.p;
        da.b_t = e->aem_bt[q];
        da.u_rep = ma.u_rep[q] ? ma.u_rep[q] + (size_t)row[q] * N : nullptr;
        da.ring = adaptive ? e->ml_ring.p : nullptr;
        da.ring_P = e->ring_P;
        da.ring_pos = rp++;
        da.rec_params = ma.rec_params[q] ? ma.rec_params[q] + (size_t)row[q] * N * d : nullptr;
        da.rec_stats = ma.rec_stats[q] ? ma.rec_stats[q] + (size_t)row[q] * N * 3 : nullptr;
        da.rec_acc = ma.rec_acc[q] ? ma.rec_acc[q] + (size_t)row[q] * N : nullptr;
        hipLaunchKernelGGL(k_aemd_action, dim3(grid), dim3(64 * EXT_WAVES), 0, e->stream, da);
        HIP_TRY(hipGetLastError());
        e->aem_bt[q] += 1;
        cc[k] = 0;
        cc[q] += 1;
        row[q] += 1;
        continue;
      }
      if (e->aem) {
        ExtAemArgs ga{};
        ga.N = N;
        ga.NP = NP;
        ga.chain_offset = e->cfg.chain_offset;
        ga.d = d;
        ga.DP = DP;
        ga.m = e->aem_m;
        ga.MP = e->aem_ld;
        ga.nlev = nl;
        ga.q = q;
        ga.is_da = nl == 2;
        ga.dependent = e->aem == TDA_AEM_STATE_DEPENDENT;
        ga.prop_kind = e->pp.kind;
        ga.pr_W = e->prior_W_rm.p;
        ga.pr_logdet = e->prior_logconst - d * std::log(2.0 * M_PI);
        ga.scaling = e->scaling.p;
        ga.seed = e->cfg.seed;
        ga.step = e->done[q] + row[q];
        ga.Fnew = lq.cb_F.p;
        for (int k2 = 0; k2 < nl; ++k2) {
          ga.data[k2] = e->levels[k2].data64.p;
          ga.Fcur[k2] = e->ext_Fcur[k2].p;
          ga.bias_tot[k2] = e->aem_bias[k2].p;
          ga.cov_inv[k2] = e->aem_covinv[k2].p;
          ga.b_mu[k2] = e->aem_bmu[k2].p;
          ga.mdiff[k2] = e->aem_mdiff[k2].p;
        }
        ga.var_finest = e->levels[nl - 1].var;
        ga.Fst = e->ext_Fst.p;
        ga.theta = e->ml_theta.p;
        ga.lp = e->ml_lp.p;
        ga.ll = e->ml_ll.p;
        ga.Sst = e->ml_S.p;
        ga.anyacc = e->ml_anyacc.p;
        ga.sid = e->ml_sid.p;
        ga.b_t = e->aem_bt[q];
        ga.u_rep = ma.u_rep[q] ? ma.u_rep[q] + (size_t)row[q] * N : nullptr;
        ga.ring = adaptive ? e->ml_ring.p : nullptr;
        ga.ring_P = e->ring_P;
        ga.ring_pos = rp++;
        ga.rec_params = ma.rec_params[q] ? ma.rec_params[q] + (size_t)row[q] * N * d : nullptr;
        ga.rec_stats = ma.rec_stats[q] ? ma.rec_stats[q] + (size_t)row[q] * N * 3 : nullptr;
        ga.rec_acc = ma.rec_acc[q] ? ma.rec_acc[q] + (size_t)row[q] * N : nullptr;
        ga.rvec = e->aem_rvec.p;
        ga.upd = e->aem_upd.p;
        AemRefreshArgs ra{};
        ra.N = N;
        ra.NP = NP;
        ra.m = e->aem_m;
        ra.MP = e->aem_ld;
        ra.cov = e->levels[k].cov64.p;
        if (ga.dependent) {
          ra.nsum = 1;
          ra.sig[0] = e->aem_bsig[q].p;
        } else {
          ra.nsum = nl - q;
          for (int p2 = q; p2 < nl; ++p2) ra.sig[p2 - q] = e->aem_bsig[p2].p;
        }
        ra.V = e->aem_covinv[k].p;
        ra.rvec = e->aem_rvec.p;
        ra.upd = e->aem_upd.p;
        ra.ll = e->ml_ll.p;
        ra.Sst = e->ml_S.p;
        ra.sid = e->ml_sid.p;
        ra.nlev = nl;
        ra.k = k;
        ra.b_t = e->aem_bt[q];
        {
          ScopedTimer tm(e, 3);
          if (e->aem_ld == 64) hipLaunchKernelGGL(k_ext_aem_action<64>, dim3((unsigned)N), dim3(64), 0, e->stream, ga);
          else if (e->aem_ld == 128) hipLaunchKernelGGL(k_ext_aem_action<128>, dim3((unsigned)N), dim3(128), 0, e->stream, ga);
          else hipLaunchKernelGGL(k_ext_aem_action<256>, dim3((unsigned)N), dim3(256), 0, e->stream, ga);
          launch_aem_refresh(ra, e->stream);  // the new factor V = L^-1 of level k and update_link of its latest link
        }
        HIP_TRY(hipGetLastError());
        e->aem_bt[q] += 1;
        cc[k] = 0;
        cc[q] += 1;
        row[q] += 1;
        continue;
      }
      ExtLevelArgs la{};
      la.N = N;
      la.NP = NP;
      la.chain_offset = e->cfg.chain_offset;
      la.d = d;
      la.DP = DP;
      la.m = lq.m;
      la.nlev = nl;
      la.q = q;
      la.seed = e->cfg.seed;
      la.step = e->done[q] + row[q];
      la.F = lq.cb_F.p;
      la.data = lq.udata.p;
      la.w = lq.noise_kind == TDA_NOISE_DIAG ? lq.uw.p : nullptr;
      la.Pd = lq.noise_kind == TDA_NOISE_DENSE ? lq.Pd.p : nullptr;
      la.var = lq.var;
      la.theta = e->ml_theta.p;
      la.lp = e->ml_lp.p;
      la.ll = e->ml_ll.p;
      la.Sst = e->ml_S.p;
      la.anyacc = e->ml_anyacc.p;
      la.u_rep = ma.u_rep[q] ? ma.u_rep[q] + (size_t)row[q] * N : nullptr;
      la.rec_params = ma.rec_params[q] ? ma.rec_params[q] + (size_t)row[q] * N * d : nullptr;
      la.rec_stats = ma.rec_stats[q] ? ma.rec_stats[q] + (size_t)row[q] * N * 3 : nullptr;
      la.rec_acc = ma.rec_acc[q] ? ma.rec_acc[q] + (size_t)row[q] * N : nullptr;
      la.ring = adaptive ? e->ml_ring.p : nullptr;
      la.ring_P = e->ring_P;
      la.ring_pos = rp++;
      la.ysnap = (e->randomize && k == 0) ? e->ml_ysnap.p : nullptr;
      hipLaunchKernelGGL(k_ext_level_action, dim3(grid), dim3(64 * EXT_WAVES), la.Pd ? (size_t)EXT_WAVES * lq.m * sizeof(double) : 0, e->stream, la);
      HIP_TRY(hipGetLastError());
      cc[k] = 0;
      cc[q] += 1;
      row[q] += 1;
    }
  }
  return TDA_OK;
}

static int run_multilevel(tda_engine* e, int64_t n_fine, const tda_outputs* outs) {
  HIP_TRY(hipSetDevice(e->cfg.device));
  const int nl = e->nlev, d = e->d, DP = e->DP;
  const int64_t N = e->N, NP = e->NP;
  if (outs)
    for (int k = 0; k < nl; ++k)
      if (outs[k].struct_size != sizeof(tda_outputs)) return fail(TDA_ERR_INVALID, "tda_outputs[%d].struct_size mismatch", k);
  int64_t mult[MAXLEV];  // local steps of level k per finest step
  mult[nl - 1] = 1;
  for (int k = nl - 2; k >= 0; --k) mult[k] = mult[k + 1] * e->sl[k];
  const int64_t total_base = n_fine * mult[0];
  if (outs)
    for (int k = 0; k < nl; ++k)
      if (int crc = check_out_capacity(outs + k, k, n_fine * mult[k], N, d)) return crc;
  if (e->rep_steps && e->rep_pos + total_base > e->rep_steps) return fail(TDA_ERR_INVALID, "replay buffer too short");
  if (e->exp_steps && e->exp_pos + total_base > e->exp_steps) return fail(TDA_ERR_INVALID, "export buffer too small");
  if (e->is_dreamz) {
    if (e->rp_steps && e->rp_pos + total_base > e->rp_steps) return fail(TDA_ERR_INVALID, "DREAMZ replay buffer too short");
    if (e->arch_rows + total_base > e->arch_cap) return fail(TDA_ERR_INVALID, "archive capacity (%lld rows) exceeded", (long long)e->arch_cap);
  }
  for (int k = 1; k < nl; ++k)
    if (e->u_rep_lv_n[k] && e->u_rep_lv_pos[k] + n_fine * mult[k] > e->u_rep_lv_n[k])
      return fail(TDA_ERR_INVALID, "replay buffer of level %d too short", k);
  if (e->rep_steps || (e->is_dreamz && e->rp_steps))
    for (int k = 1; k < nl; ++k)
      if (!e->u_rep_lv_n[k]) return fail(TDA_ERR_STATE, "replay mode needs uniforms for every level (set_replay_level)");

  const bool is_am = e->pp.kind == TDA_PROP_AM, adaptive = e->pp.adaptive != 0, periodic = is_am || adaptive;
  const int period = e->pp.period;
  // dense error model over linear levels, diagonal prior, fixed subchains: the base subchain on k_aem_base_steps (TINYDA_AEM_BASE=0:
  // on k_ml_steps, one pass over every chain's factor per step -- the A/B switch and the path of everything else)
  static const bool aem_base_ok = env_int("TINYDA_AEM_BASE", 1) != 0;
  // (65 .. 128 parameters: k_ml_steps<128, 1> -- k_aem_base_steps maps a parameter to a lane of its one wave)
  const bool aem_base_kernel = aem_base_ok && (e->aem == TDA_AEM_STATE_INDEPENDENT || e->aem == TDA_AEM_STATE_DEPENDENT) && !e->ext_hier && !e->wide &&
                               !e->randomize && !e->is_dreamz && e->prior_kind != PRIOR_DENSE && e->levels[0].Apk.p != nullptr;
  // LDS staging layout of the per-level data vectors
  int lds_y[MAXLEV] = {0, 0, 0, 0}, lds_w[MAXLEV] = {0, 0, 0, 0}, off = 0;
  for (int k = 0; k < nl; ++k) {
    lds_y[k] = off;
    off += e->levels[k].m_pad;
    if (e->levels[k].noise_kind == TDA_NOISE_DIAG) {
      lds_w[k] = off;
      off += e->levels[k].m_pad;
    }
  }
  const int prow = e->prior_kind == PRIOR_DENSE ? e->prior_ncb * 16 : 0;
  int dense_mp = 0;  // residual tile of the widest level with a dense observation covariance (k_ml_steps evaluates r^T Sigma^-1 r from LDS)
  for (int k = 0; k < nl; ++k)
    if (e->levels[k].noise_kind == TDA_NOISE_DENSE) dense_mp = std::max(dense_mp, e->levels[k].m_pad);
  // (k_ml_steps keeps what the levels above the base hold in LDS between level actions: states per thread, densities and flags per
  // lane-mapped chain and wave -- four waves, 16 threads per chain)
  const int up_ept = DP >= 16 ? DP / 16 : 1, up_pairs = nl * (nl - 1) / 2;
  const size_t up_doubles = (size_t)(nl - 1) * up_ept * 256 + (size_t)4 * (3 * (nl - 1) + 2 * up_pairs) * 16;
  const size_t lds = ((size_t)16 * (DP + 2) + 128 + off + prow + (e->aem ? 16 * (e->levels[0].m_pad + 2) + 16 : 0) +
                      (dense_mp ? 16 * (dense_mp + 2) + 16 : 0) + up_doubles) * sizeof(double);
  if (!e->ext_hier && lds > 160 * 1024)  // (host-sequenced hierarchies stage nothing: their level kernels stream the model outputs)
    return fail(TDA_ERR_UNSUPPORTED, "levels need %zu bytes of LDS staging", lds);

  if (e->profiling) {
    for (auto& t : e->timed) {
      (void)hipEventDestroy(t.a);
      (void)hipEventDestroy(t.b);
    }
    e->timed.clear();
  }
  int64_t rows_out[MAXLEV] = {0, 0, 0, 0};  // rows already written to the caller's buffers, per level
  // host outputs in pinned memory: copies on a second stream under the next block (see tda_engine_run)
  bool any_host = false, all_pinned = true;
  if (outs)
    for (int k = 0; k < nl; ++k) {
      const void* hp[3] = {outs[k].params, outs[k].stats, outs[k].accepted};
      for (const void* q : hp)
        if (q && !is_device_ptr(q)) {
          any_host = true;
          all_pinned = all_pinned && is_pinned_host_ptr(q);
        }
    }
  const bool async_host = any_host && all_pinned;
  if (async_host) {
    if (!e->copy_stream) {
      HIP_TRY(hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking));
      for (int i = 0; i < 2; ++i) {
        HIP_TRY(hipEventCreateWithFlags(&e->ev_rec[i], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&e->ev_cp[i], hipEventDisableTiming));
      }
    }
    for (int k = 0; k < nl; ++k)
      if (!e->ml_rec_params2[k].p) {
        int rc;
        if ((rc = e->ml_rec_params2[k].alloc((size_t)e->SMAX * N * d)) || (rc = e->ml_rec_stats2[k].alloc((size_t)e->SMAX * N * 3)) ||
            (rc = e->ml_rec_acc2[k].alloc((size_t)e->SMAX * N)))
          return rc;
      }
  }
  // Draws of block b + 1 on a second stream under block b's level kernel, as tda_engine_run does (tda_host_single.inc), when the
  // generator's waves (64 registers) fit beside a resident tile of the level kernel (hipFuncGetAttributes on the kernel launch_ml
  // would pick): the lean two- and three-level kernels through their 224-register entry points (C3, C5-literal) or as compiled,
  // every instance for <= 32 parameters; not the instances with diagonal noise on two operator blocks, the diagonal error model
  // in three levels, or the generic kernel -- there the generator would only take CUs from the tiles (measured on C3 before its
  // kernel fitted: step kernel 0.66 -> 0.98 ms per block for 0.10 ms of draws) and the block's draws stay in front of it on the
  // one stream (k_propose).  Identity proposal factor: the normals ARE the increments (k_rng_direct).  Any other factor: normals as
  // fragments (k_rng), increments by k_apply at the head of the block -- or, at an AdaptiveMetropolis swap, by the launch that
  // folds the block's states into the moments and factors the new covariance (k_adapt_chol_apply), as in the single-level pipeline.
  // TINYDA_ML_SPLIT=0 / 1: never / always (A/B measurements).
  static const int ml_split_env = env_int("TINYDA_ML_SPLIT", -1);  // 0: never, 1: always, unset: by registers
  const bool ml_direct = e->L_identity;
  bool ml_split = ml_split_env != 0 && !e->rep_steps && !e->ext_hier && !e->is_dreamz && !e->aem &&
                  (e->pp.kind == TDA_PROP_GRW || e->pp.kind == TDA_PROP_PCN || e->pp.kind == TDA_PROP_AM);
  if (ml_split && ml_split_env != 1) {
    MLArgs qa{};  // (the fields the kernel choice depends on: da_lean_eligible, launch_ml)
    qa.nlev = nl;
    qa.d = d;
    qa.prop_kind = e->pp.kind;
    qa.randomize = e->randomize;
    qa.cascade = 1;
    qa.pr.kind = e->prior_kind;
    qa.lds_total = off;
    for (int k = 0; k < nl; ++k) {
      qa.lv[k].ncb = e->levels[k].ncb;
      qa.lv[k].noise_kind = e->levels[k].noise_kind;
    }
    int free_regs = 0, qrc = TDA_OK;
    DISPATCH_DPAD_W(DP, qrc = launch_ml<DPAD>(qa, NP / 16, lds, e->stream, &free_regs, true));
    if (qrc) return qrc;
    ml_split = free_regs >= 64;
  }
  // (guarded on the LAST buffer of the set, not on the stream: a set-up that failed half way -- an allocation refused -- is
  // retried by the next run() instead of leaving a stream behind that says "ready" over null buffers; ADVICE r4)
  if (ml_split && !e->lublk2[1].p) {
    if (!e->rng_stream) HIP_TRY(hipStreamCreateWithFlags(&e->rng_stream, hipStreamNonBlocking));
    for (int i = 0; i < 2; ++i) {
      if (!e->ev_rng[i]) HIP_TRY(hipEventCreateWithFlags(&e->ev_rng[i], hipEventDisableTiming));
      if (!e->ev_apply[i]) HIP_TRY(hipEventCreateWithFlags(&e->ev_apply[i], hipEventDisableTiming));
      if (!e->ev_steps[i]) HIP_TRY(hipEventCreateWithFlags(&e->ev_steps[i], hipEventDisableTiming));
      int rc;
      if ((rc = e->zfrag[i].alloc((size_t)((e->SMAX + 15) / 16 * 16) * NP * DP))) return rc;
      if ((rc = e->ublk2[i].alloc((size_t)e->SMAX * NP))) return rc;
      if ((rc = e->lublk2[i].alloc((size_t)e->SMAX * NP))) return rc;
    }
  }
  auto ml_block_len = [&](int64_t t_now, int64_t left) {
    int64_t S = std::min<int64_t>(left, e->SMAX);
    if (periodic) S = std::min<int64_t>(S, period - (t_now % period));
    return S;
  };
  auto enqueue_ml_rng = [&](int64_t blk, int64_t t0, int64_t S, int64_t exp_off) -> int {
    const int b = (int)(blk & 1);
    RngArgs ra{};
    ra.N = N;
    ra.NP = NP;
    ra.chain_offset = e->cfg.chain_offset;
    ra.d = d;
    ra.S = (int)S;
    ra.step0 = t0;
    ra.seed = e->cfg.seed;
    ra.u = e->ublk2[b].p;
    ra.logu = e->lublk2[b].p;
    if (e->exp_steps) {
      ra.z_export = (e->exp_dev ? e->z_exp : e->z_exp_d.p) + (size_t)exp_off * N * d;
      ra.u_export = (e->exp_dev ? e->u_exp : e->u_exp_d.p) + (size_t)exp_off * N;
    }
    if (ml_direct) {
      DISPATCH_DPAD_W(DP, launch_rng_direct<DPAD>(ra, e->zfrag[b].p, e->rng_stream));
    } else {
      ra.zf = e->zfrag[b].p;
      DISPATCH_DPAD_W(DP, launch_rng<DPAD>(ra, e->rng_stream));
    }
    HIP_TRY(hipEventRecord(e->ev_rng[b], e->rng_stream));
    return TDA_OK;
  };
  if (ml_split && total_base > 0) {
    HIP_TRY(hipEventRecord(e->ev_steps[0], e->stream));  // init and earlier run() calls precede the first draw
    HIP_TRY(hipStreamWaitEvent(e->rng_stream, e->ev_steps[0], 0));
    if (int rc = enqueue_ml_rng(0, e->t, ml_block_len(e->t, total_base), e->exp_pos)) return rc;
  }
  int64_t blk_ix = 0;
  int64_t done_base = 0;
  e->am_pending = 0;  // (a run that failed half way may have left rows pending)
  // The error model cuts the blocks at every base subchain (5 steps at C5): the proposal increments and uniforms do not depend on
  // the chains and the proposal factor only changes at a period boundary, so they are drawn for a whole WINDOW of steps (up to the
  // boundary / SMAX) in one launch and the blocks walk through it -- 60 launches of 48 us became 3 of 160 at C5 + error model.
  // Same counters, so the same draws.  TINYDA_ML_PREDRAW=0: one launch per block.
  static const bool predraw_ok = env_int("TINYDA_ML_PREDRAW", 1) != 0;
  const bool predraw = predraw_ok && e->aem && !e->ext_hier && !e->is_dreamz && !e->rep_steps && !ml_split;
  int64_t win_t0 = 0, win_n = 0;  // steps [win_t0, win_t0 + win_n) are in the increment / uniform buffers
  bool inc_ready = false;  // the block about to start already has its increments (the swap launch of the block before it)
  while (done_base < total_base) {
    int64_t S = std::min<int64_t>(total_base - done_base, e->SMAX);
    if (periodic) S = std::min<int64_t>(S, period - (e->t % period));
    if (e->aem && !e->ext_hier) S = std::min<int64_t>(S, e->sl[0] - e->cnt[0]);  // level actions sequenced after the block: stop when the base subchain completes (host-sequenced hierarchies run their actions inside the block)
    // how many local steps each level completes inside this block (uniform schedule)
    int c2[MAXLEV];
    int64_t nblk[MAXLEV] = {S, 0, 0, 0};
    for (int k = 0; k < MAXLEV; ++k) c2[k] = e->cnt[k];
    int64_t tail_appends = 0;  // alignment entries appended by the block's last base step
    for (int64_t s = 0; s < S; ++s) {
      c2[0] += 1;
      for (int k = 0; k < nl - 1 && c2[k] == e->sl[k]; ++k) {
        c2[k] = 0;
        nblk[k + 1] += 1;
        c2[k + 1] += 1;
        if (s == S - 1) tail_appends += 1;
      }
    }

    ProposeArgs pa{};
    pa.N = N;
    pa.NP = NP;
    pa.chain_offset = e->cfg.chain_offset;
    pa.d = d;
    pa.S = (int)S;
    bool draw_now = true;
    if (predraw) {
      if (e->t >= win_t0 && e->t + S <= win_t0 + win_n) {
        draw_now = false;
      } else {
        int64_t W = std::min<int64_t>(total_base - done_base, e->SMAX);
        if (periodic) W = std::min<int64_t>(W, period - (e->t % period));
        win_t0 = e->t;
        win_n = W;
        pa.S = (int)W;
      }
    }
    pa.step0 = e->t;
    pa.seed = e->cfg.seed;
    pa.Lk = e->Lk.p;
    pa.L_stride = e->L_shared ? 0 : (int64_t)DP * DP;
    pa.inc = e->inc.p;
    pa.u = e->ublk.p;
    pa.logu = e->ext_hier ? nullptr : e->lublk.p;  // (the host-sequenced path uses that buffer as scratch)
    if (e->rep_steps) {
      pa.z_replay = e->z_rep.p + (size_t)e->rep_pos * N * d;
      pa.u_replay = e->u_rep.p + (size_t)e->rep_pos * N;
    }
    if (e->exp_steps) {
      pa.z_export = (e->exp_dev ? e->z_exp : e->z_exp_d.p) + (size_t)e->exp_pos * N * d;
      pa.u_export = (e->exp_dev ? e->u_exp : e->u_exp_d.p) + (size_t)e->exp_pos * N;
    }
    if (ml_split) {
      // this block's draws were queued a block ago; the event on the main stream marks the end of block blk_ix - 1, the last reader of
      // the buffer set the next block's draws overwrite
      const int b = (int)(blk_ix & 1);
      if (!inc_ready) HIP_TRY(hipStreamWaitEvent(e->stream, e->ev_rng[b], 0));
      if (!ml_direct && !inc_ready) {
        ApplyArgs ap{};
        ap.NP = NP;
        ap.S = (int)S;
        ap.Lk = e->Lk.p;
        ap.L_stride = pa.L_stride;
        ap.zf = e->zfrag[b].p;
        ap.inc = e->inc.p;
        wide_fill(e, ap);
        ScopedTimer tm(e, 0);
        int arc = TDA_OK;
        DISPATCH_DPAD_W(DP, arc = launch_apply<DPAD>(ap, e->stream));
        if (arc) return arc;
      }
      inc_ready = false;
      HIP_TRY(hipEventRecord(e->ev_apply[b], e->stream));
      pa.inc = ml_direct ? e->zfrag[b].p : e->inc.p;
      pa.u = e->ublk2[b].p;
      pa.logu = e->lublk2[b].p;
      if (done_base + S < total_base) {
        HIP_TRY(hipStreamWaitEvent(e->rng_stream, e->ev_apply[b], 0));
        if (int rc = enqueue_ml_rng(blk_ix + 1, e->t + S, ml_block_len(e->t + S, total_base - done_base - S), e->exp_pos + S)) return rc;
      }
    } else if (e->is_dreamz) {  // everything DREAMZ.make_proposal draws for the block's base steps (the archive grows by a row per step)
      DreamDrawArgs da{};
      da.N = N;
      da.NP = NP;
      da.chain_offset = e->cfg.chain_offset;
      da.d = d;
      da.S = (int)S;
      da.delta = e->dz.delta;
      da.nCR = e->dz.nCR;
      da.step0 = e->t;
      da.M_base = e->arch_rows;
      da.grow = 1;
      da.seed = e->cfg.seed;
      da.b = e->dz.b;
      da.b_star = e->dz.b_star;
      da.scaling = e->scaling.p;
      da.pCR = e->dz_pCR.p;
      da.coef = e->dz_coef.p;
      da.epsm = e->dz_epsm.p;
      da.ridx = e->dz_ridx.p;
      da.u = e->ublk.p;
      da.mcr_last = e->dz_mcr_last.p;
      if (e->rp_steps) {
        const size_t o = (size_t)e->rp_pos * N;
        da.r_rep = e->rp_r.p + o * e->dz.delta * 2;
        da.mcr_rep = e->rp_mcr.p + o;
        da.forced_rep = e->rp_forced.p + o;
        da.sub_rep = e->rp_sub.p + o * d;
        da.e_rep = e->rp_e.p + o * d;
        da.eps_rep = e->rp_eps.p + o * d;
        da.u_rep = e->rp_u.p + o;
      }
      if (e->exp_steps) {
        da.eps_export = (e->exp_dev ? e->z_exp : e->z_exp_d.p) + (size_t)e->exp_pos * N * d;
        da.u_export = (e->exp_dev ? e->u_exp : e->u_exp_d.p) + (size_t)e->exp_pos * N;
      }
      da.arch_shared = nullptr;
      ScopedTimer tm(e, 0);
      DISPATCH_DPAD(DP, launch_dz_draw<DPAD>(da, e->stream));
    } else if (!draw_now) {
      // (inside the window drawn earlier)
    } else if (e->L_identity && !e->rep_steps && pa.logu) {
      // identity proposal factor (CrankNicolson under a standard-normal prior): the increments are the normals, drawn at
      // eight waves per SIMD straight into the increment block (C3: k_propose 3.6 ms -> this, per 2000 base steps)
      RngArgs ra{};
      ra.N = N;
      ra.NP = NP;
      ra.chain_offset = e->cfg.chain_offset;
      ra.d = d;
      ra.S = pa.S;
      ra.step0 = e->t;
      ra.seed = e->cfg.seed;
      ra.u = pa.u;
      ra.logu = pa.logu;
      ra.z_export = pa.z_export;
      ra.u_export = pa.u_export;
      ScopedTimer tm(e, 0);
      DISPATCH_DPAD_W(DP, launch_rng_direct<DPAD>(ra, e->inc.p, e->stream));
    } else {
      if (e->wide) {  // (65 .. 128 parameters: the normals go through a fragment buffer, tda_kernels_wide.h)
        if (!e->zfrag[0].p) {
          int zrc = e->zfrag[0].alloc((size_t)((e->SMAX + 15) / 16 * 16) * NP * DP);
          if (zrc) return zrc;
        }
        pa.zf_tmp = e->zfrag[0].p;
        pa.ud = e->wide_ud.p;
        pa.sel = e->L_shared ? nullptr : e->wide_sel.p;
        pa.NPf = e->L_shared ? 1 : NP;
      }
      ScopedTimer tm(e, 0);
      int prc = TDA_OK;
      DISPATCH_DPAD_W(DP, prc = launch_propose<DPAD>(pa, e->stream));
      if (prc) return prc;
    }

    if (predraw) {  // this block's place in the window
      const size_t o = (size_t)(e->t - win_t0);
      pa.inc += o * NP * DP;
      pa.u += o * NP;
      if (pa.logu) pa.logu += o * NP;
    }
    MLArgs ma{};
    ma.logu0 = pa.logu;
    for (int k = 0; k < nl; ++k) {
      const Level& lv = e->levels[k];
      ma.lv[k].Apk = lv.Apk.p;
      ma.lv[k].ytil = lv.ytil.p;
      ma.lv[k].w = lv.w.p;
      ma.lv[k].Ppk = lv.Ppk.p;
      ma.lv[k].ncb = lv.ncb;
      ma.lv[k].m_pad = lv.m_pad;
      ma.lv[k].noise_kind = lv.noise_kind;
      ma.lv[k].var = lv.var;
      ma.lds_y[k] = lds_y[k];
      ma.lds_w[k] = lds_w[k];
      ma.sl[k] = e->sl[k];
      ma.cnt[k] = e->cnt[k];
      ma.done[k] = e->done[k];
    }
    ma.lds_total = off;
    ma.pr.mean = e->prior_mean.p;
    ma.pr.pinv = e->prior_pinv.p;
    ma.pr.Wpk = e->prior_Wpk.p;
    ma.pr.wmu = e->prior_wmu.p;
    ma.pr.ncb = e->prior_ncb;
    ma.pr.kind = e->prior_kind;
    ma.pr.lo = e->prior_bounded ? e->prior_lo.p : nullptr;
    ma.pr.hi = e->prior_bounded ? e->prior_hi.p : nullptr;
    ma.pr.logconst = e->prior_logconst;
    ma.N = N;
    ma.NP = NP;
    ma.d = d;
    ma.S = (int)S;
    ma.prop_kind = e->pp.kind;
    ma.nlev = nl;
    ma.randomize = e->randomize;
    ma.seed = e->cfg.seed;
    ma.chain_offset = e->cfg.chain_offset;
    ma.theta = e->ml_theta.p;
    ma.lp = e->ml_lp.p;
    ma.ll = e->ml_ll.p;
    ma.Sst = e->ml_S.p;
    ma.anyacc = e->ml_anyacc.p;
    ma.ysnap = e->ml_ysnap.p;
    ma.pick = e->ml_pick.p;
    ma.scaling = e->scaling.p;
    ma.ring = e->ml_ring.p;
    ma.ring_P = e->ring_P;
    ma.ring_pos = e->ring_pos;
    ma.inc = pa.inc;
    ma.u0 = pa.u;
    for (int k = 1; k < nl; ++k)
      ma.u_rep[k] = e->u_rep_lv_n[k] ? e->u_rep_lv[k].p + (size_t)e->u_rep_lv_pos[k] * N : nullptr;
    ma.ridx_rep = e->ridx_rep_n ? e->ridx_rep.p + (size_t)e->ridx_rep_pos * N : nullptr;
    ma.cascade = e->aem ? 0 : 1;
    ma.aem_on = e->aem ? 1 : 0;
    ma.aem_mp = e->aem ? e->levels[0].m_pad : 0;
    ma.aem_ld = e->aem_ld;
    ma.aem_bias = e->aem ? e->aem_bias[0].p : nullptr;
    ma.aem_P = e->aem ? e->aem_covinv[0].p : nullptr;
    ma.sid = e->ml_sid.p;
    bool dev_p[MAXLEV], dev_s[MAXLEV], dev_a[MAXLEV];
    for (int k = 0; k < nl; ++k) {
      double* op = outs ? outs[k].params : nullptr;
      double* os = outs ? outs[k].stats : nullptr;
      uint8_t* oa = outs ? outs[k].accepted : nullptr;
      dev_p[k] = is_device_ptr(op);
      dev_s[k] = is_device_ptr(os);
      dev_a[k] = is_device_ptr(oa);
      const bool need_p = op || (k == 0 && is_am);
      const bool second = async_host && (blk_ix & 1);
      ma.rec_params[k] = dev_p[k] ? op + (size_t)rows_out[k] * N * d : (need_p ? (second ? e->ml_rec_params2[k].p : e->ml_rec_params[k].p) : nullptr);
      ma.rec_stats[k] = dev_s[k] ? os + (size_t)rows_out[k] * N * 3 : (os ? (second ? e->ml_rec_stats2[k].p : e->ml_rec_stats[k].p) : nullptr);
      ma.rec_acc[k] = dev_a[k] ? oa + (size_t)rows_out[k] * N : (oa ? (second ? e->ml_rec_acc2[k].p : e->ml_rec_acc[k].p) : nullptr);
    }
    if (async_host && blk_ix >= 2) HIP_TRY(hipStreamWaitEvent(e->stream, e->ev_cp[blk_ix & 1], 0));  // buffer set free again
    if (e->ext_hier) {
      const int xrc = run_ext_hierarchy_block(e, ma, S, adaptive);
      if (xrc) return xrc;
    } else if (aem_base_kernel && aem_base_lds_bytes((int)S, e->aem_ld) <= 64 * 1024) {
      // dense error model over the engine's linear levels: the base subchain with ONE pass over every chain's factor
      // (k_aem_base_steps, tda_kernels_aemr.h) instead of one per step.  Its S + 2 product vectors live in LDS: a block whose
      // set would not fit 64 KB (a base subchain beyond ~50 steps at 128 outputs; two workgroups per CU beyond that, and past
      // 160 KB the launch would be refused) takes the step-by-step level kernel below, as TINYDA_AEM_BASE=0 does (ADVICE r4).
      AemBaseArgs ba{};
      ba.N = N;
      ba.NP = NP;
      ba.d = d;
      ba.DP = DP;
      ba.m = e->aem_m;
      ba.MP = e->aem_ld;
      ba.S = (int)S;
      ba.pcn = e->pp.kind == TDA_PROP_PCN;
      ba.Apk = e->levels[0].Apk.p;
      ba.ncb = e->levels[0].ncb;
      ba.ytil = e->levels[0].ytil64.p;
      ba.bias = e->aem_bias[0].p;
      ba.V = e->aem_covinv[0].p;
      ba.pr_mean = e->prior_mean.p;
      ba.pr_pinv = e->prior_pinv.p;
      ba.pr_lo = e->prior_bounded ? e->prior_lo.p : nullptr;
      ba.pr_hi = e->prior_bounded ? e->prior_hi.p : nullptr;
      ba.logconst = e->prior_logconst;
      ba.theta = e->ml_theta.p;
      ba.lp = e->ml_lp.p;
      ba.ll = e->ml_ll.p;
      ba.anyacc = e->ml_anyacc.p;
      ba.sid = e->ml_sid.p;
      ba.step0 = e->done[0];
      ba.scaling = e->scaling.p;
      ba.inc = pa.inc;
      ba.u0 = pa.u;
      ba.ring = e->ml_ring.p;
      ba.ring_P = e->ring_P;
      ba.ring_pos = e->ring_pos;
      ba.rec_params = ma.rec_params[0];
      ba.rec_stats = ma.rec_stats[0];
      ba.rec_acc = ma.rec_acc[0];
      const size_t blds = aem_base_lds_bytes((int)S, e->aem_ld);
      ScopedTimer tm(e, 1);
      if (e->aem_ld == 64) {
        hipLaunchKernelGGL(k_aem_base_steps<4>, dim3((unsigned)N), dim3(64), blds, e->stream, ba);
      } else if (e->aem_ld == 128) {
        hipLaunchKernelGGL(k_aem_base_steps<8>, dim3((unsigned)N), dim3(64), blds, e->stream, ba);
      } else {
        hipLaunchKernelGGL(k_aem_base_steps<16>, dim3((unsigned)N), dim3(64), blds, e->stream, ba);
      }
#ifdef AEMB_TRACE
      {
        static int n_tr = 0;
        if (++n_tr == 40) {
          std::vector<unsigned long long> tr(8192 * 16);
          (void)hipStreamSynchronize(e->stream);
          (void)hipMemcpyFromSymbol(tr.data(), HIP_SYMBOL(aemb_trace_buf), tr.size() * 8);
          if (FILE* fp = fopen(getenv("AEMB_TRACE_FILE") ? getenv("AEMB_TRACE_FILE") : "/tmp/aemb_trace.bin", "wb")) {
            fwrite(tr.data(), 8, tr.size(), fp);
            fclose(fp);
          }
        }
      }
#endif
    } else {
      ScopedTimer tm(e, 1);
      int lrc = TDA_OK;
      DISPATCH_DPAD_W(DP, lrc = launch_ml<DPAD>(ma, NP / 16, lds, e->stream, nullptr, ml_split));
      if (lrc) return lrc;
    }

    const bool boundary = periodic && ((e->t + S) % period == 0);
    if (e->is_dreamz) {
      // archive column sums of the S rows the block appended; at a period boundary the global scaling (accept-flag window
      // incl. alignment entries) and the crossover probabilities (proposal.py:797-809)
      int64_t app = 0;
      for (int k = 0; k < nl; ++k) app += nblk[k];
      ScopedTimer tm(e, 2);
      const int drc = dreamz_sums_catchup(e, e->arch_rows, S, boundary, adaptive, std::pow(e->dz.gamma, -(double)e->k_adapt), e->theta_last.p,
                                          adaptive ? e->ml_ring.p : nullptr, e->ring_P, e->ring_pos + app - tail_appends);
      if (drc) return drc;
      e->arch_rows += S;
      if (e->rp_steps) e->rp_pos += S;
    } else if (is_am || (boundary && adaptive)) {
      // The moment recursion reads and writes every chain's mean and covariance (168 MB at 4096 chains x 64 parameters) however few
      // states it folds in, and nothing looks at the moments before the period's swap: blocks that end inside a period (the error
      // model cuts them at every base subchain: 5 states) leave their states where the level kernel recorded them and the
      // boundary -- or the end of the run -- folds the period in one launch, state by state in the same order (the same bits).
      // Device outputs: the rows are contiguous in the caller's buffer; host outputs: staged.  TINYDA_AM_DEFER=0: every block.
      static const bool defer_ok = env_int("TINYDA_AM_DEFER", 1) != 0;
      const bool last_block = done_base + S >= total_base;
      const double* fold_rows = ma.rec_params[0];
      int64_t fold_n = S, fold_t0 = e->t;
      bool fold_now = true;
      if (is_am && defer_ok && !e->pp.block_moments && (e->am_pending > 0 || !(boundary || last_block))) {
        if (!dev_p[0]) {
          if (e->am_stage.n < (size_t)period * N * d) {  // (first use, or a longer period than the last run's; nothing is pending then)
            if (e->am_pending > 0) return fail(TDA_ERR_STATE, "adaptation period changed inside a period");
            if (int src = e->am_stage.alloc((size_t)period * N * d)) return src;
          }
          HIP_TRY(hipMemcpyAsync(e->am_stage.p + (size_t)e->am_pending * N * d, ma.rec_params[0], (size_t)S * N * d * sizeof(double),
                                 hipMemcpyDeviceToDevice, e->stream));
        }
        if (e->am_pending == 0) {
          e->am_pending_t0 = e->t;
          e->am_pending_rows = dev_p[0] ? ma.rec_params[0] : e->am_stage.p;
        }
        e->am_pending += S;
        fold_now = boundary || last_block;
        fold_rows = e->am_pending_rows;
        fold_n = e->am_pending;
        fold_t0 = e->am_pending_t0;
      }
      if (fold_now) {
      e->am_pending = 0;
      AdaptArgs aa{};
      aa.N = N;
      aa.NP = NP;
      aa.d = d;
      aa.S = (int)fold_n;
      aa.t_base = fold_t0;
      aa.do_am = is_am;
      aa.boundary = boundary;
      aa.do_scale = adaptive;
      const bool do_swap = is_am && boundary && (e->t + S >= e->pp.t0);
      aa.do_swap = do_swap;
      aa.block_moments = e->pp.block_moments != 0;
      aa.period = period;
      aa.gamma_pow = std::pow(e->pp.gamma, -(double)e->k_adapt);
      aa.sd = e->am_sd;
      aa.alpha_star = e->pp.kind == TDA_PROP_MALA ? 0.57 : 0.24;  // proposal.py:899 / :169
      aa.eps = e->pp.epsilon;
      aa.rec_params = const_cast<double*>(fold_rows);
      aa.am_mu = e->am_mu.p;
      aa.am_sigma = e->am_sigma.p;
      aa.scaling = e->scaling.p;
      aa.acc_count = e->acc_count.p;
      aa.flags = e->flags.p;
      aa.ring = adaptive ? e->ml_ring.p : nullptr;
      aa.ring_P = e->ring_P;
      {
        int64_t app = 0;
        for (int k = 0; k < nl; ++k) app += nblk[k];
        aa.ring_hi = e->ring_pos + app - tail_appends;
      }
      ScopedTimer tm(e, 2);
      CholArgs ca{};
      ca.N = N;
      ca.d = d;
      ca.am_sigma = e->am_sigma.p;
      ca.Lk = e->Lk.p;
      ca.flags = e->flags.p;
      if (e->wide) {
        ca.ud = e->wide_ud.p;
        ca.sel = e->wide_sel.p;
        ca.pad_cov = e->wide_cov.p;
        ca.NP = NP;
      }
      ApplyArgs ap{};
      const bool swap_apply = do_swap && ml_split && !ml_direct && done_base + S < total_base;
      if (swap_apply) {  // C <- Sigma and the next block's increments from the new factor in the same launch (its normals were drawn under this block)
        const int nb = (int)((blk_ix + 1) & 1);
        HIP_TRY(hipStreamWaitEvent(e->stream, e->ev_rng[nb], 0));
        ap.NP = NP;
        ap.S = (int)ml_block_len(e->t + S, total_base - done_base - S);
        ap.Lk = e->Lk.p;
        ap.L_stride = (int64_t)DP * DP;
        ap.zf = e->zfrag[nb].p;
        ap.inc = e->inc.p;
        wide_fill(e, ap);
      }
      bool one_launch = false;
      if (swap_apply) DISPATCH_DPAD_W(DP, one_launch = launch_adapt_chol_apply<DPAD>(aa, ca, ap, e->stream));
      if (one_launch) {
        inc_ready = true;
      } else {
        DISPATCH_DPAD_W(DP, launch_adapt<DPAD>(aa, e->stream));
        if (swap_apply) {
          int arc = TDA_OK;
          DISPATCH_DPAD_W(DP, arc = launch_chol_apply<DPAD>(ca, ap, e->stream));
          if (arc) return arc;
          inc_ready = true;
        } else if (do_swap) {
          DISPATCH_DPAD_W(DP, launch_chol<DPAD>(ca, e->stream));
        }
      }
      }  // fold_now
    }
    HIP_TRY(hipGetLastError());
    if (boundary && adaptive) e->k_adapt += 1;

    if (e->aem && !e->ext_hier) {
      // host-sequenced upper levels: decision of level q, then the error-model update of level q-1, in ascending q
      int64_t extra = 0;
      for (int qq = 1; qq < nl; ++qq) {
        if (nblk[qq] == 0) continue;
        AemArgs ag{};
        ag.N = N;
        ag.NP = NP;
        ag.chain_offset = e->cfg.chain_offset;
        ag.d = d;
        ag.DP = DP;
        ag.m = e->aem_m;
        ag.MP = e->aem_ld;
        ag.nlev = nl;
        ag.q = qq;
        ag.is_da = nl == 2;
        ag.dependent = e->aem == TDA_AEM_STATE_DEPENDENT;
        ag.prop_kind = e->pp.kind;
        ag.seed = e->cfg.seed;
        ag.step = e->done[qq];
        for (int k = 0; k < nl; ++k) {
          ag.A[k] = e->levels[k].A_rm.p;
          ag.ytil[k] = e->levels[k].ytil64.p;
          ag.data[k] = e->levels[k].data64.p;
          ag.bias_tot[k] = e->aem_bias[k].p;
          ag.cov_inv[k] = e->aem_covinv[k].p;
          ag.b_mu[k] = e->aem_bmu[k].p;
          ag.mdiff[k] = e->aem_mdiff[k].p;
        }
        ag.var_finest = e->levels[nl - 1].var;
        ag.pr_mean = e->prior_mean.p;
        ag.pr_W = e->prior_W_rm.p;
        ag.pr_logdet = e->prior_logconst - d * std::log(2.0 * M_PI);
        ag.theta = e->ml_theta.p;
        ag.lp = e->ml_lp.p;
        ag.ll = e->ml_ll.p;
        ag.Sst = e->ml_S.p;
        ag.anyacc = e->ml_anyacc.p;
        ag.sid = e->ml_sid.p;
        ag.b_t = e->aem_bt[qq];
        ag.scaling = e->scaling.p;
        ag.u_rep = e->u_rep_lv_n[qq] ? e->u_rep_lv[qq].p + (size_t)e->u_rep_lv_pos[qq] * N : nullptr;
        ag.ring = e->ml_ring.p;
        ag.ring_P = e->ring_P;
        ag.ring_pos = e->ring_pos + S + extra;
        ag.rec_params = ma.rec_params[qq];
        ag.rec_stats = ma.rec_stats[qq];
        ag.rec_acc = ma.rec_acc[qq];
        ag.rvec = e->aem_rvec.p;
        ag.upd = e->aem_upd.p;
        AemRefreshArgs ra{};
        ra.N = N;
        ra.NP = NP;
        ra.m = e->aem_m;
        ra.MP = e->aem_ld;
        ra.cov = e->levels[qq - 1].cov64.p;
        if (ag.dependent) {
          ra.nsum = 1;
          ra.sig[0] = e->aem_bsig[qq].p;
        } else {
          ra.nsum = nl - qq;
          for (int p = qq; p < nl; ++p) ra.sig[p - qq] = e->aem_bsig[p].p;
        }
        ra.V = e->aem_covinv[qq - 1].p;
        ra.rvec = e->aem_rvec.p;
        ra.upd = e->aem_upd.p;
        ra.ll = e->ml_ll.p;
        ra.Sst = e->ml_S.p;
        ra.sid = e->ml_sid.p;
        ra.nlev = nl;
        ra.k = qq - 1;
        ra.b_t = e->aem_bt[qq];
        {
          // decision of level qq + tracker update, then the refreshed factor of level qq - 1 and update_link of its latest link
          ScopedTimer tm(e, 3);
          // the model outputs the decision and the update need, for all chains on the matrix cores (TINYDA_AEM_PRE=0: matrix-vector
          // products per chain inside k_aem_action)
          static const bool pre_ok = env_int("TINYDA_AEM_PRE", 1) != 0;
          if (pre_ok && e->aem_F.p && e->levels[qq].Apk.p && e->levels[qq - 1].Apk.p) {
            LinMultiArgs la{};
            la.N = N;
            la.d = d;
            la.m = e->aem_m;
            la.ldp = DP;
            la.ldf = e->aem_ld;
            la.n = 4;
            for (int w = 0; w < 4; ++w) {
              const int lev = w < 2 ? qq : qq - 1, at = (w & 1) ? qq : qq - 1;  // operator of level `lev` at the state of level `at`
              la.Apk[w] = e->levels[lev].Apk.p;
              la.ncb[w] = e->levels[lev].ncb;
              la.prop[w] = e->ml_theta.p + (size_t)at * NP * DP;
              la.F[w] = e->aem_F.p + (size_t)w * NP * e->aem_ld;
              ag.Fpre[w] = la.F[w];
            }
            DISPATCH_DPAD_W(DP, hipLaunchKernelGGL((k_linear_outputs_multi<DPAD>), dim3((unsigned)(NP / 16), 4), dim3(256), 0, e->stream, la));
          }
          if (e->aem_ld == 64) hipLaunchKernelGGL(k_aem_action<64>, dim3((unsigned)N), dim3(64), 0, e->stream, ag);
          else if (e->aem_ld == 128) hipLaunchKernelGGL(k_aem_action<128>, dim3((unsigned)N), dim3(128), 0, e->stream, ag);
          else hipLaunchKernelGGL(k_aem_action<256>, dim3((unsigned)N), dim3(256), 0, e->stream, ag);
          launch_aem_refresh(ra, e->stream);
        }
        e->aem_bt[qq] += 1;
        extra += 1;
      }
      HIP_TRY(hipGetLastError());
    }

    bool host_copies = false;
    int rc;
    if (async_host) {
      const int i = (int)(blk_ix & 1);
      HIP_TRY(hipEventRecord(e->ev_rec[i], e->stream));
      HIP_TRY(hipStreamWaitEvent(e->copy_stream, e->ev_rec[i], 0));
      for (int k = 0; k < nl; ++k) {
        if (outs[k].params && !dev_p[k])
          HIP_TRY(hipMemcpyAsync(outs[k].params + (size_t)rows_out[k] * N * d, ma.rec_params[k], (size_t)nblk[k] * N * d * sizeof(double), hipMemcpyDeviceToHost, e->copy_stream));
        if (outs[k].stats && !dev_s[k])
          HIP_TRY(hipMemcpyAsync(outs[k].stats + (size_t)rows_out[k] * N * 3, ma.rec_stats[k], (size_t)nblk[k] * N * 3 * sizeof(double), hipMemcpyDeviceToHost, e->copy_stream));
        if (outs[k].accepted && !dev_a[k])
          HIP_TRY(hipMemcpyAsync(outs[k].accepted + (size_t)rows_out[k] * N, ma.rec_acc[k], (size_t)nblk[k] * N, hipMemcpyDeviceToHost, e->copy_stream));
      }
      HIP_TRY(hipEventRecord(e->ev_cp[i], e->copy_stream));
    } else {
      for (int k = 0; k < nl; ++k) {
        if (!outs) break;
        if (outs[k].params && !dev_p[k]) {
          if ((rc = copy_out(e, outs[k].params + (size_t)rows_out[k] * N * d, e->ml_rec_params[k].p, (size_t)nblk[k] * N * d * sizeof(double)))) return rc;
          host_copies = true;
        }
        if (outs[k].stats && !dev_s[k]) {
          if ((rc = copy_out(e, outs[k].stats + (size_t)rows_out[k] * N * 3, e->ml_rec_stats[k].p, (size_t)nblk[k] * N * 3 * sizeof(double)))) return rc;
          host_copies = true;
        }
        if (outs[k].accepted && !dev_a[k]) {
          if ((rc = copy_out(e, outs[k].accepted + (size_t)rows_out[k] * N, e->ml_rec_acc[k].p, (size_t)nblk[k] * N))) return rc;
          host_copies = true;
        }
      }
      if (host_copies) HIP_TRY(hipStreamSynchronize(e->stream));
    }
    blk_ix += 1;
    if (int prc = progress_mark(e, nblk[nl - 1], nullptr, 0)) return prc;  // progress counts finest-level iterations (chain.py:343-351)

    int64_t appended = 0;
    for (int k = 0; k < nl; ++k) {
      e->cnt[k] = c2[k];
      e->done[k] += nblk[k];
      rows_out[k] += nblk[k];
      appended += nblk[k];
      if (k >= 1 && e->u_rep_lv_n[k]) e->u_rep_lv_pos[k] += nblk[k];
    }
    if (e->ridx_rep_n) e->ridx_rep_pos += nblk[1];
    e->ring_pos += appended;
    e->t += S;
    done_base += S;
    if (e->rep_steps) e->rep_pos += S;
    if (e->exp_steps) e->exp_pos += S;
  }
  if (async_host) {  // host outputs: run() returns with the records in place
    HIP_TRY(hipStreamSynchronize(e->copy_stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
  }
  if (e->exp_steps && !e->exp_dev) {
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(e->z_exp, e->z_exp_d.p, (size_t)e->exp_pos * N * d * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(e->u_exp, e->u_exp_d.p, (size_t)e->exp_pos * N * sizeof(double), hipMemcpyDeviceToHost));
  }
  return TDA_OK;
}

}  // extern "C"
