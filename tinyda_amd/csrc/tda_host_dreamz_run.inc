// Part of libtinyda_hip.so: included by tda_engine.hip (ONE translation unit -- the helpers, the engine struct and the kernel
// launchers above it are visible here).  DREAM(Z) driver: step arguments, column sums / adaptation, run_dreamz.
extern "C" {

void fill_dreamz_step_args(tda_engine* e, DreamStepArgs& sa) {
  const Level& lv = e->levels[0];
  sa.lv.Apk = lv.Apk.p;
  sa.lv.ytil = lv.ytil.p;
  sa.lv.w = lv.w.p;
  sa.lv.Ppk = lv.Ppk.p;
  sa.lv.ncb = lv.ncb;
  sa.lv.m_pad = lv.m_pad;
  sa.lv.noise_kind = lv.noise_kind;
  sa.lv.var = lv.var;
  sa.pr.mean = e->prior_mean.p;
  sa.pr.pinv = e->prior_pinv.p;
  sa.pr.Wpk = e->prior_Wpk.p;
  sa.pr.wmu = e->prior_wmu.p;
  sa.pr.ncb = e->prior_ncb;
  sa.pr.kind = e->prior_kind;
  sa.pr.lo = e->prior_bounded ? e->prior_lo.p : nullptr;
  sa.pr.hi = e->prior_bounded ? e->prior_hi.p : nullptr;
  sa.pr.logconst = e->prior_logconst;
  sa.model = lv.model;
  sa.ros_a = lv.ros_a;
  sa.ros_b = lv.ros_b;
  sa.ros_data = lv.ros_data;
  sa.N = e->N;
  sa.NP = e->NP;
  sa.d = e->d;
  sa.delta = e->dz.delta;
  sa.M_base = e->arch_rows;
  sa.shared = e->dz.shared;
  sa.cap = e->arch_cap;
  sa.arch = e->arch.p;
  sa.theta = e->theta.p;
  sa.theta_prev = e->theta_prev.p;
  sa.lp = e->lp.p;
  sa.ll = e->ll.p;
  sa.acc_count = e->acc_count.p;
  sa.coef = e->dz_coef.p;
  sa.epsm = e->dz_epsm.p;
  sa.ridx = e->dz_ridx.p;
  sa.u = e->ublk.p;
}

static int dreamz_sums_catchup(tda_engine* e, int64_t row0, int64_t nrows, bool boundary, bool scale, double gamma_pow,
                               const double* theta_now, const uint8_t* ring, int ring_P, int64_t ring_hi) {
  DreamAdaptArgs aa{};
  aa.N = e->N;
  aa.NP = e->NP;
  aa.d = e->d;
  aa.nCR = e->dz.nCR;
  aa.period = e->dz.period;
  aa.gamma_pow = gamma_pow;
  aa.shared = e->dz.shared;
  aa.cap = e->arch_cap;
  aa.arch = e->arch.p;
  aa.zsum = e->zsum.p;
  aa.zsq = e->zsq.p;
  aa.theta = theta_now ? theta_now : e->theta.p;
  aa.theta_prev = e->theta_prev.p;
  aa.ring = ring;
  aa.ring_P = ring_P;
  aa.ring_hi = ring_hi;
  aa.mcr_last = e->dz_mcr_last.p;
  aa.pCR = e->dz_pCR.p;
  aa.LCR = e->dz_LCR.p;
  aa.DeltaCR = e->dz_Delta.p;
  aa.scaling = e->scaling.p;
  aa.acc_count = e->acc_count.p;
  aa.row0 = row0;
  aa.nrows = nrows;
  aa.M_total = row0 + nrows;
  if (e->dz.shared) {
    // The column sums only feed the crossover adaptation (np.var(Z, axis=0), proposal.py:800), so appended rows are summed
    // when a boundary asks for them -- [sums_rows, row0 + nrows) in one pass -- and not after every exchange interval (two
    // launches per block, 18 % of the kernel time of C4 at an interval of 16 steps).  Chunked column sums in parallel, then
    // one workgroup accumulates the chunks in a fixed order: deterministic for a given sequence of appends and boundaries.
    if (!boundary) return TDA_OK;
    const int64_t upto = row0 + nrows, from = e->sums_rows;
    if (upto > from) {
      const int64_t nb = (upto - from + COLSUM_CHUNK - 1) / COLSUM_CHUNK;
      if (e->dz_partial.n < colsum_partial_doubles(nb, e->DP)) {
        HIP_TRY(hipStreamSynchronize(e->stream));
        int rc = e->dz_partial.alloc(colsum_partial_doubles(nb, e->DP));
        if (rc) return rc;
      }
      DISPATCH_DPAD(e->DP, launch_colsum<DPAD>(e->arch.p, from, upto - from, e->dz_partial.p, nb, e->stream));
      DISPATCH_DPAD(e->DP, launch_colsum_final<DPAD>(e->dz_partial.p, nb, e->zsum.p, e->zsq.p, e->stream));
      e->sums_rows = upto;
    }
    aa.nrows = 0;  // ... then every chain adapts against the finished sums
    aa.M_total = upto;
  }
  aa.boundary = boundary;
  aa.do_scale = scale;
  DISPATCH_DPAD(e->DP, launch_dz_adapt<DPAD>(aa, e->stream));
  HIP_TRY(hipGetLastError());
  return TDA_OK;
}

static int run_dreamz(tda_engine* e, int64_t n_iter, const tda_outputs* out) {
  HIP_TRY(hipSetDevice(e->cfg.device));
  if (out && out->struct_size != sizeof(tda_outputs)) return fail(TDA_ERR_INVALID, "tda_outputs.struct_size mismatch");
  const int d = e->d, DP = e->DP;
  const int64_t N = e->N, NP = e->NP;
  const bool sh = e->dz.shared != 0, adaptive = e->dz.adaptive != 0;
  const int period = e->dz.period;
  if (e->rp_steps && e->rp_pos + n_iter > e->rp_steps) return fail(TDA_ERR_INVALID, "DREAMZ replay buffer too short");
  if (int crc = check_out_capacity(out, 0, n_iter, N, d)) return crc;
  if (e->exp_steps && e->exp_pos + n_iter > e->exp_steps) return fail(TDA_ERR_INVALID, "export buffer too small");
  if (!sh && e->arch_rows + n_iter > e->arch_cap) return fail(TDA_ERR_INVALID, "archive capacity (%lld rows) exceeded", (long long)e->arch_cap);
  if (sh && e->auto_append && e->arch_rows + n_iter * N > e->arch_cap)
    return fail(TDA_ERR_INVALID, "shared archive capacity (%lld rows) exceeded", (long long)e->arch_cap);
  double* o_params = out ? out->params : nullptr;
  double* o_stats = out ? out->stats : nullptr;
  uint8_t* o_acc = out ? out->accepted : nullptr;
  const bool p_dev = is_device_ptr(o_params), s_dev = is_device_ptr(o_stats), a_dev = is_device_ptr(o_acc);
  const Level& lv = e->levels[0];
  const bool linear = lv.model == MODEL_LINEAR;
  const bool diag = lv.noise_kind == TDA_NOISE_DIAG;
  const int prow = e->prior_kind == PRIOR_DENSE ? e->prior_ncb * 16 : 0;
  const size_t lds = ((size_t)16 * (DP + 2) + 128 + (linear ? lv.m_pad * (diag ? 2 : 1) : 0) + prow +
                      ((linear && lv.noise_kind == TDA_NOISE_DENSE) ? (size_t)16 * (lv.m_pad + 2) : 0)) * sizeof(double);
  if (e->profiling) {
    for (auto& t : e->timed) {
      (void)hipEventDestroy(t.a);
      (void)hipEventDestroy(t.b);
    }
    e->timed.clear();
  }
  const bool ext_model0 = lv.model == MODEL_CALLBACK || lv.model == MODEL_USER;
  // Shared archive, one process appending its own rows: the exchange points are the CALL-RELATIVE multiples of sync_every -- where
  // the multi-rank driver (distributed.run_shared_dream: one run() per interval, then the all-gather) has them.  A block that an
  // adaptation boundary cuts in two is not an exchange point: the rows of its first half become visible together with the second
  // half's (`since` = steps since the last exchange point), so one process and N ranks see the same archive at every step whatever
  // the period (ADVICE r2: the engine used to restart full intervals after a boundary).
  int64_t since = 0;
  const bool pending_at_entry = e->pending_steps != 0;  // (rows taken over from an earlier call sit in blk_hist, not in place)
  auto block_len = [&](int64_t t_now, int64_t left, int64_t since_now) {
    int64_t S = std::min<int64_t>(left, e->SMAX);
    if (adaptive) S = std::min<int64_t>(S, period - (t_now % period));
    if (sh) {
      const int64_t K = e->dz.sync_every > 0 ? e->dz.sync_every : e->SMAX;
      S = std::min<int64_t>(S, K - (e->auto_append && !e->dist_ranks ? since_now % K : 0));
      if (!e->dist_ranks && !e->auto_append && e->pending_steps + S > e->SMAX) S = e->SMAX - e->pending_steps;
    }
    return S;
  };
  if (e->dist_ranks) {  // distributed archive: one exchange interval per call, then tda_engine_archive_publish (after the ranks met)
    if (e->dist_n_unpub >= 2) return fail(TDA_ERR_STATE, "distributed archive: two blocks wait for tda_engine_archive_publish");
    if (e->dist_adapt_pending) return fail(TDA_ERR_STATE, "distributed archive: an adaptation waits for tda_engine_archive_publish");
    const int64_t K = e->dz.sync_every > 0 ? e->dz.sync_every : e->SMAX;
    if (n_iter > K || (adaptive && n_iter > period - (e->t % period)))
      return fail(TDA_ERR_INVALID, "distributed archive: a run() call covers at most one exchange interval (%lld steps) and does not cross an adaptation boundary", (long long)K);
    if (e->dz.M0 + (e->dist_steps + e->dist_pending + n_iter) * N > e->arch_cap) return fail(TDA_ERR_INVALID, "archive segment capacity (%lld rows) exceeded", (long long)e->arch_cap);
  }
  // everything DREAMZ.make_proposal draws for the S steps of the next block
  auto enqueue_draw = [&](int64_t S, bool gather, const DreamFuseArgs* fuse = nullptr) -> int {
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
    da.grow = sh ? 0 : 1;
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
    da.arch_shared = gather ? e->arch.p : nullptr;
    if (e->dist_ranks) {
      da.dist_ranks = e->dist_ranks;
      da.dist_me = e->dist_me;
      da.dist_M0 = e->dz.M0;
      da.dist_nloc = N;
      da.dist_ntot = N * e->dist_ranks;
      da.seg = e->dist_seg_dev.p;
    }
    DISPATCH_DPAD(DP, launch_dz_draw<DPAD>(da, e->stream, fuse));
    return TDA_OK;
  };
  int64_t done = 0;
  while (done < n_iter) {
    const int64_t S = block_len(e->t, n_iter - done, since);
    if (S <= 0) return fail(TDA_ERR_STATE, "shared archive: call archive_take / archive_append before running further");
    DreamStepArgs sa{};
    fill_dreamz_step_args(e, sa);
    // BASELINE configs[3] in one launch per block (k_dreamz_draw<32, false, true>): one process appending in place, the built-in
    // Rosenbrock model under a diagonal prior, engine-generated variates; TINYDA_DZ_FUSED=0: the two kernels (same bits)
    static const bool fused_ok = env_int("TINYDA_DZ_FUSED", 1) != 0;
    const bool fused = fused_ok && sh && !e->dist_ranks && e->auto_append && N == NP && !pending_at_entry && DP == 32 && !ext_model0 &&
                       lv.model == MODEL_ROSENBROCK && e->prior_kind != PRIOR_DENSE && !e->rp_steps;
    if (!fused) {
      ScopedTimer tm(e, 0);
      if (int rc = enqueue_draw(S, sh)) return rc;
    }
    sa.S = (int)S;
    sa.jump_ready = sh ? 1 : 0;
    const bool ext_model = ext_model0;
    sa.rec_params = p_dev ? o_params + (size_t)done * N * d : (o_params ? e->rec_params.p : nullptr);
    sa.rec_stats = s_dev ? o_stats + (size_t)done * N * 3 : (o_stats ? e->rec_stats.p : nullptr);
    sa.rec_acc = a_dev ? o_acc + (size_t)done * N : (o_acc ? e->rec_acc.p : nullptr);
    // single process, no padding chains: the block's states ARE the next archive rows in canonical order (step-major,
    // chain minor), the kernel appends them in place (the jumps of this block were gathered before it started)
    const bool dist = e->dist_ranks != 0;
    const bool direct = !dist && sh && e->auto_append && N == NP && !pending_at_entry;
    // distributed archive: the block's states are this rank's next rows of its own segment, written in place
    // (in place = behind the visible rows and behind the rows of an interval's earlier blocks that are not visible yet)
    sa.blk_states = sh ? (dist ? e->arch.p + (size_t)(e->dz.M0 + (e->dist_steps + e->dist_pending) * N) * DP
                               : (direct ? e->arch.p + (size_t)(e->arch_rows + e->pending_steps * N) * DP : e->blk_states.p))
                       : nullptr;
    if (ext_model) {
      // model outside the engine's kernels: per step apply the jump, evaluate (callback: one host call for all chains;
      // source-defined: tda_user_eval on the stream), accept, append
      if (e->prior_kind == PRIOR_DENSE) return fail(TDA_ERR_UNSUPPORTED, "callback / source-defined forward models need a diagonal prior covariance");
      const unsigned grid = (unsigned)((N + EXT_WAVES - 1) / EXT_WAVES), gridp = (unsigned)((NP + EXT_WAVES - 1) / EXT_WAVES);
      for (int64_t s = 0; s < S; ++s) {
        if (s == S - 1)  // jumping distance of the adaptation: the state before the block's last step (proposal.py:800)
          HIP_TRY(hipMemcpyAsync(e->theta_prev.p, e->theta.p, (size_t)NP * DP * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
        DzExtArgs za{};
        za.N = N;
        za.NP = NP;
        za.d = d;
        za.DP = DP;
        za.delta = e->dz.delta;
        za.s = (int)s;
        za.shared = sh ? 1 : 0;
        za.jump_ready = sa.jump_ready;
        za.M_base = e->arch_rows;
        za.cap = e->arch_cap;
        za.arch = e->arch.p;
        za.theta = e->theta.p;
        za.coef = e->dz_coef.p;
        za.epsm = e->dz_epsm.p;
        za.ridx = e->dz_ridx.p;
        za.prop = lv.cb_prop.p;
        za.blk_states = sa.blk_states;
        hipLaunchKernelGGL(k_dz_ext_propose, dim3(grid), dim3(64 * EXT_WAVES), 0, e->stream, za);
        int mrc = ext_model_outputs(e, lv);
        if (mrc) return mrc;
        ExtArgs xa{};
        fill_ext_args(e, lv, xa);
        xa.mode = 0;
        xa.prop_kind = TDA_PROP_GRW;  // posterior ratio (proposal.py:253-258)
        xa.theta = e->theta.p;
        xa.lp = e->lp.p;
        xa.ll = e->ll.p;
        xa.scaling = e->scaling.p;
        xa.acc_count = e->acc_count.p;
        xa.u = e->ublk.p;
        xa.s = (int)s;
        xa.rec_params = sa.rec_params;
        xa.rec_stats = sa.rec_stats;
        xa.rec_acc = sa.rec_acc;
        hipLaunchKernelGGL(k_ext_accept, dim3(grid), dim3(64 * EXT_WAVES), xa.Pd ? (size_t)EXT_WAVES * lv.m * sizeof(double) : 0, e->stream, xa);
        hipLaunchKernelGGL(k_dz_ext_append, dim3(gridp), dim3(64 * EXT_WAVES), 0, e->stream, za);
      }
    } else if (fused) {
      DreamFuseArgs fa{};
      fa.pr_mean = sa.pr.mean;
      fa.pr_pinv = sa.pr.pinv;
      fa.pr_lo = sa.pr.lo;
      fa.pr_hi = sa.pr.hi;
      fa.logconst = sa.pr.logconst;
      fa.ros_a = sa.ros_a;
      fa.ros_b = sa.ros_b;
      fa.ros_data = sa.ros_data;
      fa.var = sa.lv.var;
      fa.theta = sa.theta;
      fa.theta_prev = sa.theta_prev;
      fa.lp = sa.lp;
      fa.ll = sa.ll;
      fa.acc_count = sa.acc_count;
      fa.rec_params = sa.rec_params;
      fa.rec_stats = sa.rec_stats;
      fa.rec_acc = sa.rec_acc;
      fa.blk_states = sa.blk_states;
      ScopedTimer tm(e, 1);
      if (int rc = enqueue_draw(S, true, &fa)) return rc;
    } else {
      ScopedTimer tm(e, 1);
      DISPATCH_DPAD(DP, launch_dz_steps<DPAD>(sa, lds, e->stream));
    }
    HIP_TRY(hipGetLastError());
    const bool boundary = adaptive && ((e->t + S) % period == 0);
    int rc;
    if (!sh) {  // per-chain archives grew inside the kernel
      ScopedTimer tm(e, 2);
      if ((rc = dreamz_sums_catchup(e, e->arch_rows, S, boundary, adaptive, std::pow(e->dz.gamma, -(double)e->k_adapt)))) return rc;
      e->arch_rows += S;
    } else if (dist) {
      // rows are in place in this rank's segment; they become visible (and an adaptation at this boundary runs) in
      // tda_engine_archive_publish, once every rank has finished the block
      e->dist_unpub[e->dist_n_unpub++] = S;
      e->dist_pending += S;
      e->dist_adapt_pending = boundary;
      e->dist_adapt_gamma = std::pow(e->dz.gamma, -(double)e->k_adapt);
      e->dist_adapt_rows = e->arch_rows;  // what this block's proposals could see
    } else {
      // keep this block's states for the exchange, [pending + s][NP][DP]
      if (!direct)
        HIP_TRY(hipMemcpyAsync(e->blk_hist.p + (size_t)e->pending_steps * NP * DP, e->blk_states.p, (size_t)S * NP * DP * sizeof(double),
                               hipMemcpyDeviceToDevice, e->stream));
      e->pending_steps += S;
      // crossover / scaling adaptation sees the archive the finished block proposed from (rows of this block are
      // appended afterwards), so the result does not depend on who appends when
      {
        ScopedTimer tm(e, 2);
        if (boundary && (rc = dreamz_sums_catchup(e, e->arch_rows, 0, true, adaptive, std::pow(e->dz.gamma, -(double)e->k_adapt)))) return rc;
      }
      since += S;
      const int64_t Ksync = e->dz.sync_every > 0 ? e->dz.sync_every : e->SMAX;
      if (e->auto_append && (since % Ksync == 0 || done + S >= n_iter)) {  // single process: the local rows are all rows; canonical order = step-major, chain minor
        if (direct) {
          // already in place
        } else if (N == NP) {
          HIP_TRY(hipMemcpyAsync(e->arch.p + (size_t)e->arch_rows * DP, e->blk_hist.p, (size_t)e->pending_steps * N * DP * sizeof(double),
                                 hipMemcpyDeviceToDevice, e->stream));
        } else {
          for (int64_t s = 0; s < e->pending_steps; ++s)
            HIP_TRY(hipMemcpy2DAsync(e->arch.p + (size_t)(e->arch_rows + s * N) * DP, DP * sizeof(double),
                                     e->blk_hist.p + (size_t)s * NP * DP, DP * sizeof(double), DP * sizeof(double), N,
                                     hipMemcpyDeviceToDevice, e->stream));
        }
        const int64_t new_rows = e->pending_steps * N;
        e->pending_steps = 0;
        if ((rc = dreamz_sums_catchup(e, e->arch_rows, new_rows, false, false, 1.0))) return rc;
        e->arch_rows += new_rows;
      }
    }
    if (boundary && !dist) e->k_adapt += 1;
    bool host_copies = false;
    if (o_params && !p_dev) {
      if ((rc = copy_out(e, o_params + (size_t)done * N * d, e->rec_params.p, (size_t)S * N * d * sizeof(double)))) return rc;
      host_copies = true;
    }
    if (o_stats && !s_dev) {
      if ((rc = copy_out(e, o_stats + (size_t)done * N * 3, e->rec_stats.p, (size_t)S * N * 3 * sizeof(double)))) return rc;
      host_copies = true;
    }
    if (o_acc && !a_dev) {
      if ((rc = copy_out(e, o_acc + (size_t)done * N, e->rec_acc.p, (size_t)S * N))) return rc;
      host_copies = true;
    }
    if (host_copies) HIP_TRY(hipStreamSynchronize(e->stream));
    if ((rc = progress_mark(e, S, nullptr, 0))) return rc;
    e->t += S;
    done += S;
    if (e->rp_steps) e->rp_pos += S;
    if (e->exp_steps) e->exp_pos += S;
  }
  if (e->exp_steps && !e->exp_dev) {
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(e->z_exp, e->z_exp_d.p, (size_t)e->exp_pos * N * d * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(e->u_exp, e->u_exp_d.p, (size_t)e->exp_pos * N * sizeof(double), hipMemcpyDeviceToHost));
  }
  return TDA_OK;
}

}  // extern "C"
