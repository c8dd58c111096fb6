// Part of libtinyda_hip.so: included by tda_engine.hip (ONE translation unit -- the helpers, the engine struct and the kernel
// launchers above it are visible here).  Single-level driver: current state, replay / export, tda_engine_run (k_rng || k_apply -> k_mh_steps -> k_adapt -> k_chol_apply).
extern "C" {

int tda_engine_get_current(tda_engine* e, double* theta, double* stats) {
  if (!e || !e->inited) return fail(TDA_ERR_STATE, "engine not initialised");
  if (e->nlev > 1) return tda_engine_get_level_state(e, e->nlev - 1, theta, stats);
  HIP_TRY(hipSetDevice(e->cfg.device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  const int64_t N = e->N, NP = e->NP;
  if (theta) {
    std::vector<double> h((size_t)NP * e->DP), o((size_t)N * e->d);
    HIP_TRY(hipMemcpy(h.data(), e->theta.p, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int64_t c = 0; c < N; ++c)
      for (int j = 0; j < e->d; ++j) o[(size_t)c * e->d + j] = h[(size_t)c * e->DP + j];
    HIP_TRY(hipMemcpy(theta, o.data(), o.size() * sizeof(double), is_device_ptr(theta) ? hipMemcpyHostToDevice : hipMemcpyHostToHost));
  }
  if (stats) {
    std::vector<double> a(NP), b(NP), o((size_t)N * 3);
    HIP_TRY(hipMemcpy(a.data(), e->lp.p, NP * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(b.data(), e->ll.p, NP * sizeof(double), hipMemcpyDeviceToHost));
    for (int64_t c = 0; c < N; ++c) {
      o[c * 3] = a[c];
      o[c * 3 + 1] = b[c];
      o[c * 3 + 2] = a[c] + b[c];
    }
    HIP_TRY(hipMemcpy(stats, o.data(), o.size() * sizeof(double), is_device_ptr(stats) ? hipMemcpyHostToDevice : hipMemcpyHostToHost));
  }
  return TDA_OK;
}

int tda_engine_set_replay(tda_engine* e, const double* z, const double* u, int64_t n_steps) {
  if (!e) return fail(TDA_ERR_INVALID, "null engine");
  HIP_TRY(hipSetDevice(e->cfg.device));
  e->rep_steps = 0;
  e->rep_pos = 0;
  e->z_rep.release();
  e->u_rep.release();
  if (!z || !u || n_steps <= 0) return TDA_OK;
  int rc;
  const size_t nz = (size_t)n_steps * e->N * e->d, nu = (size_t)n_steps * e->N;
  if ((rc = e->z_rep.alloc(nz))) return rc;
  if ((rc = e->u_rep.alloc(nu))) return rc;
  HIP_TRY(hipMemcpy(e->z_rep.p, z, nz * sizeof(double), is_device_ptr(z) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->u_rep.p, u, nu * sizeof(double), is_device_ptr(u) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
  e->rep_steps = n_steps;
  return TDA_OK;
}

int tda_engine_set_export(tda_engine* e, double* z, double* u, int64_t n_steps) {
  if (!e) return fail(TDA_ERR_INVALID, "null engine");
  HIP_TRY(hipSetDevice(e->cfg.device));
  e->z_exp = e->u_exp = nullptr;
  e->exp_steps = 0;
  e->exp_pos = 0;
  e->z_exp_d.release();
  e->u_exp_d.release();
  if (!z || !u || n_steps <= 0) return TDA_OK;
  if (is_device_ptr(z) != is_device_ptr(u)) return fail(TDA_ERR_INVALID, "export buffers must both be host or both be device");
  e->exp_dev = is_device_ptr(z);
  if (!e->exp_dev) {
    int rc;
    if ((rc = e->z_exp_d.alloc((size_t)n_steps * e->N * e->d))) return rc;
    if ((rc = e->u_exp_d.alloc((size_t)n_steps * e->N))) return rc;
  }
  e->z_exp = z;
  e->u_exp = u;
  e->exp_steps = n_steps;
  return TDA_OK;
}


// A caller's record buffers must hold `need` records of this level (tda_outputs.rows states the capacity); for device
// pointers the extent of the underlying allocation is checked as well, so a short buffer is an error code, never a fault.
static int check_out_capacity(const tda_outputs* o, int level, int64_t need, int64_t N, int d) {
  if (!o || (!o->params && !o->stats && !o->accepted)) return TDA_OK;
  if ((int64_t)o->rows < need)
    return fail(TDA_ERR_INVALID, "tda_outputs[%d].rows = %u but this run() produces %lld records for that level", level, o->rows,
                (long long)need);
  const void* ptr[3] = {o->params, o->stats, o->accepted};
  const size_t bytes[3] = {(size_t)need * N * d * sizeof(double), (size_t)need * N * 3 * sizeof(double), (size_t)need * N};
  static const char* const nm[3] = {"params", "stats", "accepted"};
  for (int i = 0; i < 3; ++i) {
    if (!ptr[i] || !is_device_ptr(ptr[i])) continue;
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)ptr[i]) != hipSuccess) {
      (void)hipGetLastError();
      continue;
    }
    const size_t room = size - (size_t)((const char*)ptr[i] - (const char*)base);
    if (room < bytes[i])
      return fail(TDA_ERR_INVALID, "tda_outputs[%d].%s: device allocation has %zu bytes after the pointer, %zu needed", level, nm[i],
                  room, bytes[i]);
  }
  return TDA_OK;
}

static int run_multilevel(tda_engine* e, int64_t n_fine, const tda_outputs* outs);
static int run_dreamz(tda_engine* e, int64_t n_iter, const tda_outputs* out);

// 65 .. 128 parameters: what k_wide_apply needs beyond the factor's address (per-chain factors after an AdaptiveMetropolis set-up,
// one shared factor otherwise)
static void wide_fill(tda_engine* e, tda::ApplyArgs& ap) {
  if (!e->wide) return;
  ap.ud = e->wide_ud.p;
  ap.sel = e->L_shared ? nullptr : e->wide_sel.p;
  ap.NPf = e->L_shared ? 1 : e->NP;
  ap.L_stride = e->L_shared ? 0 : 1;
}

int tda_engine_run(tda_engine* e, int64_t n_iter, const tda_outputs* out) {
  if (!e || !e->inited) return fail(TDA_ERR_STATE, "engine not initialised");
  if (n_iter < 0) return fail(TDA_ERR_INVALID, "n_iterations < 0");
  if (e->nlev > 1) return run_multilevel(e, n_iter, out);
  if (e->is_dreamz) return run_dreamz(e, n_iter, out);
  if (out && out->struct_size != sizeof(tda_outputs)) return fail(TDA_ERR_INVALID, "tda_outputs.struct_size mismatch");
  HIP_TRY(hipSetDevice(e->cfg.device));
  if (e->rep_steps && e->rep_pos + n_iter > e->rep_steps)
    return fail(TDA_ERR_INVALID, "replay buffer holds %lld steps, %lld requested", (long long)(e->rep_steps - e->rep_pos), (long long)n_iter);
  if (e->exp_steps && e->exp_pos + n_iter > e->exp_steps)
    return fail(TDA_ERR_INVALID, "export buffer too small");
  const int thin = e->thin;
  if (int crc = check_out_capacity(out, 0, kept_records(e->t, n_iter, thin), e->N, e->d)) return crc;

  const int d = e->d;
  const int64_t N = e->N, NP = e->NP;
  int64_t out_row = 0;  // thinning: next row of the caller's buffers
  double* o_params = out ? out->params : nullptr;
  double* o_stats = out ? out->stats : nullptr;
  uint8_t* o_acc = out ? out->accepted : nullptr;
  const bool p_dev = is_device_ptr(o_params), s_dev = is_device_ptr(o_stats), a_dev = is_device_ptr(o_acc);
  const bool is_am = e->pp.kind == TDA_PROP_AM;
  const bool adaptive = e->pp.adaptive != 0;
  const bool periodic = is_am || adaptive;
  const int period = e->pp.period;
  const Level& lv = e->levels[0];
  const size_t lds = steps_lds_bytes(e, lv);
  bool host_copies = false;
  // Host outputs in pinned memory (hipHostMalloc / torch pin_memory): the block's records are copied by a second
  // stream while the next block computes (two sets of device block buffers).  Pageable memory: one synchronous copy
  // per block, as before.
  const bool any_host = (o_params && !p_dev) || (o_stats && !s_dev) || (o_acc && !a_dev);
  const bool async_host = any_host && (!o_params || p_dev || is_pinned_host_ptr(o_params)) &&
                          (!o_stats || s_dev || is_pinned_host_ptr(o_stats)) && (!o_acc || a_dev || is_pinned_host_ptr(o_acc));
  if (async_host && !e->copy_stream) {
    HIP_TRY(hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking));
    for (int i = 0; i < 2; ++i) {
      HIP_TRY(hipEventCreateWithFlags(&e->ev_rec[i], hipEventDisableTiming));
      HIP_TRY(hipEventCreateWithFlags(&e->ev_cp[i], hipEventDisableTiming));
    }
    int rc;
    if ((rc = e->rec_params2.alloc((size_t)e->SMAX * N * d)) || (rc = e->rec_stats2.alloc((size_t)e->SMAX * N * 3)) ||
        (rc = e->rec_acc2.alloc((size_t)e->SMAX * N)))
      return rc;
  }

  if (e->profiling) {
    for (auto& t : e->timed) {
      (void)hipEventDestroy(t.a);
      (void)hipEventDestroy(t.b);
    }
    e->timed.clear();
  }

  // Philox mode: the normals and uniforms of a block do not depend on the chains, so block b+1's are drawn on a second
  // stream while block b's k_mh_steps runs (k_rng fits into the registers the step kernel leaves free); only
  // INC = Z L^T (k_apply) stays on the critical path behind the Cholesky swap.  Replay mode keeps the fused k_propose.
  const bool split = !e->rep_steps;
  if (split && !e->rng_stream) {
    HIP_TRY(hipStreamCreateWithFlags(&e->rng_stream, hipStreamNonBlocking));
    for (int i = 0; i < 2; ++i) {
      HIP_TRY(hipEventCreateWithFlags(&e->ev_rng[i], hipEventDisableTiming));
      HIP_TRY(hipEventCreateWithFlags(&e->ev_apply[i], hipEventDisableTiming));
      HIP_TRY(hipEventCreateWithFlags(&e->ev_steps[i], hipEventDisableTiming));
      int rc;
      if ((rc = e->zfrag[i].alloc((size_t)((e->SMAX + 15) / 16 * 16) * NP * e->DP))) return rc;
      if ((rc = e->ublk2[i].alloc((size_t)e->SMAX * NP))) return rc;
      if ((rc = e->lublk2[i].alloc((size_t)e->SMAX * NP))) return rc;
    }
  }
  auto block_len = [&](int64_t t_now, int64_t left) {
    int64_t S = std::min<int64_t>(left, e->SMAX);
    if (periodic || mass_warming(e, t_now)) S = std::min<int64_t>(S, period - (t_now % period));  // (a window of the mass adaptation ends with a block)
    return S;
  };
  // draw block `blk` (steps t0 .. t0 + S - 1, the exp_off-th exported step) into buffer blk & 1 on the rng stream
  auto enqueue_rng = [&](int64_t blk, int64_t t0, int64_t S, int64_t exp_off) -> int {
    const int b = (int)(blk & 1);
    RngArgs ra{};
    ra.N = N;
    ra.NP = NP;
    ra.chain_offset = e->cfg.chain_offset;
    ra.d = d;
    ra.S = (int)S;
    ra.step0 = t0;
    ra.seed = e->cfg.seed;
    ra.zf = e->zfrag[b].p;
    ra.u = e->ublk2[b].p;
    ra.logu = e->lublk2[b].p;
    ra.qz = e->pp.kind == TDA_PROP_INDEPENDENCE ? e->qzblk2[b].p : nullptr;
    if (e->exp_steps) {
      ra.z_export = (e->exp_dev ? e->z_exp : e->z_exp_d.p) + (size_t)exp_off * N * d;
      ra.u_export = (e->exp_dev ? e->u_exp : e->u_exp_d.p) + (size_t)exp_off * N;
    }
    // (the buffers were last read by block blk - 2, its k_apply (fragments) and k_mh_steps (uniforms): both precede the release
    // event of block blk - 1 on the main stream, which the caller has made this stream wait for)
    DISPATCH_DPAD_W(e->DP, launch_rng<DPAD>(ra, e->rng_stream));
    HIP_TRY(hipEventRecord(e->ev_rng[b], e->rng_stream));
    return TDA_OK;
  };

  int64_t done = 0, blk = 0;
  bool inc_ready = false;  // the block about to start already has its increments (k_chol_apply of the block before it)
  if (split && n_iter > 0) {
    // everything queued on the main stream so far (init, earlier run() calls) precedes the first draw
    HIP_TRY(hipEventRecord(e->ev_steps[0], e->stream));
    HIP_TRY(hipStreamWaitEvent(e->rng_stream, e->ev_steps[0], 0));
    int rc = enqueue_rng(0, e->t, block_len(e->t, n_iter), e->exp_pos);
    if (rc) return rc;
  }
  while (done < n_iter) {
    const int64_t S = block_len(e->t, n_iter - done);
    const double* u_blk = e->ublk.p;
    const double* lu_blk = e->lublk.p;
    const double* qz_blk = e->qzblk.p;

    // ---- proposal increments + uniforms ----
    if (split) {
      const int b = (int)(blk & 1);
      if (!inc_ready) {  // (after a covariance swap the previous block's k_chol_apply has produced this block's increments already)
        HIP_TRY(hipStreamWaitEvent(e->stream, e->ev_rng[b], 0));
        ApplyArgs ap{};
        ap.NP = NP;
        ap.S = (int)S;
        ap.Lk = e->Lk.p;
        ap.L_stride = e->L_shared ? 0 : (int64_t)e->DP * e->DP;
        ap.zf = e->zfrag[b].p;
        ap.inc = e->inc.p;
        wide_fill(e, ap);
        ScopedTimer tm(e, 0);
        int arc = TDA_OK;
        DISPATCH_DPAD_W(e->DP, arc = launch_apply<DPAD>(ap, e->stream));
        if (arc) return arc;
      }
      inc_ready = false;
      HIP_TRY(hipEventRecord(e->ev_apply[b], e->stream));
      u_blk = e->ublk2[b].p;
      lu_blk = e->lublk2[b].p;
      qz_blk = e->qzblk2[b].p;
      if (done + S < n_iter) {
        // next block's draws go under THIS block's steps: released by this block's k_apply / the fused
        // k_chol_apply before it (the host runs ahead of the GPU; without the wait the draws would start as soon as block blk - 1's steps
        // end, i.e. next to its k_adapt, which is itself bound by the VALU).  The event also orders the draws behind block
        // blk - 1's k_apply and k_mh_steps, the last readers of the buffers they overwrite.
        HIP_TRY(hipStreamWaitEvent(e->rng_stream, e->ev_apply[b], 0));
        int rc = enqueue_rng(blk + 1, e->t + S, block_len(e->t + S, n_iter - done - S), e->exp_pos + S);
        if (rc) return rc;
      }
    } else {
    ProposeArgs pa{};
    pa.N = N;
    pa.NP = NP;
    pa.chain_offset = e->cfg.chain_offset;
    pa.d = d;
    pa.S = (int)S;
    pa.step0 = e->t;
    pa.seed = e->cfg.seed;
    pa.Lk = e->Lk.p;
    pa.L_stride = e->L_shared ? 0 : (int64_t)e->DP * e->DP;
    pa.inc = e->inc.p;
    pa.u = e->ublk.p;
    pa.logu = e->lublk.p;
    pa.qz = e->pp.kind == TDA_PROP_INDEPENDENCE ? e->qzblk.p : nullptr;
    if (e->rep_steps) {
      pa.z_replay = e->z_rep.p + (size_t)e->rep_pos * N * d;
      pa.u_replay = e->u_rep.p + (size_t)e->rep_pos * N;
    }
    if (e->exp_steps) {
      pa.z_export = (e->exp_dev ? e->z_exp : e->z_exp_d.p) + (size_t)e->exp_pos * N * d;
      pa.u_export = (e->exp_dev ? e->u_exp : e->u_exp_d.p) + (size_t)e->exp_pos * N;
    }
    if (e->wide) {  // (65 .. 128 parameters: the normals go through a fragment buffer, tda_kernels_wide.h)
      if (!e->zfrag[0].p) {
        int zrc = e->zfrag[0].alloc((size_t)((e->SMAX + 15) / 16 * 16) * NP * e->DP);
        if (zrc) return zrc;
      }
      pa.zf_tmp = e->zfrag[0].p;
      pa.ud = e->wide_ud.p;
      pa.sel = e->L_shared ? nullptr : e->wide_sel.p;
      pa.NPf = e->L_shared ? 1 : NP;
    }
    {
      ScopedTimer tm(e, 0);
      int prc = TDA_OK;
      DISPATCH_DPAD_W(e->DP, prc = launch_propose<DPAD>(pa, e->stream));
      if (prc) return prc;
    }
    }

    if (int mrc = dense_mass_before_block(e, e->t)) return mrc;  // (the shift of a window of the dense adaptation: tda_host_dense_mass_adapt.inc)

    // ---- fused MH steps ----
    StepArgs sa{};
    fill_level(e, lv, sa);
    sa.S = (int)S;
    sa.mode = MODE_STEP;
    sa.prop_kind = e->pp.kind;
    sa.theta = e->theta.p;
    sa.lp = e->lp.p;
    sa.ll = e->ll.p;
    sa.scaling = e->scaling.p;
    sa.acc_count = e->acc_count.p;
    sa.inc = e->inc.p;
    sa.u = u_blk;
    sa.logu = lu_blk;
    const bool ow_spec = e->pp.kind == TDA_PROP_OWCN && e->ow_spectral;
    sa.SopT = e->pp.kind == TDA_PROP_OWCN ? (ow_spec ? e->ow_VVt.p : e->ow_SopT.p) : (e->pp.kind == TDA_PROP_MALA ? e->mala_H.p : nullptr);
    sa.cvec = e->pp.kind == TDA_PROP_MALA ? e->mala_c.p : (ow_spec ? e->ow_lam.p : nullptr);
    sa.grad = e->pp.kind == TDA_PROP_MALA ? e->mala_grad.p : nullptr;
    if (e->pp.kind == TDA_PROP_INDEPENDENCE) {
      sa.q_mean = e->q_mean_d.p;
      sa.qz = qz_blk;
      sa.lq = e->lq.p;
    }
    // records go straight into caller memory when it is device memory; AM needs the states either way
    double* const blk_params = (async_host && (blk & 1)) ? e->rec_params2.p : e->rec_params.p;
    double* const blk_stats = (async_host && (blk & 1)) ? e->rec_stats2.p : e->rec_stats.p;
    uint8_t* const blk_acc = (async_host && (blk & 1)) ? e->rec_acc2.p : e->rec_acc.p;
    if (async_host && blk >= 2) HIP_TRY(hipStreamWaitEvent(e->stream, e->ev_cp[blk & 1], 0));  // buffer set free again
    // (the same while the mass of HMC / NUTS adapts: k_mass_accumulate reads every state of the block)
    sa.rec_params = (p_dev && thin == 1) ? o_params + (size_t)done * N * d : ((o_params || is_am || mass_warming(e, e->t)) ? blk_params : nullptr);
    sa.rec_stats = (s_dev && thin == 1) ? o_stats + (size_t)done * N * 3 : (o_stats ? blk_stats : nullptr);
    sa.rec_acc = (a_dev && thin == 1) ? o_acc + (size_t)done * N : ((o_acc || (e->prog_h && thin > 1)) ? blk_acc : nullptr);
    const bool user_stepwise = lv.model == MODEL_USER && (lv.noise_kind == TDA_NOISE_DENSE || e->pp.kind == TDA_PROP_INDEPENDENCE || e->pp.kind == TDA_PROP_OWCN);
    if (lv.model == MODEL_CALLBACK || user_stepwise) {  // (the fused source-model kernel knows GRW / pCN steps and iso / diag noise)
      ExtArgs xa{};
      fill_ext_args(e, lv, xa);
      xa.mode = 0;
      xa.prop_kind = e->pp.kind;
      xa.theta = sa.theta;
      xa.lp = sa.lp;
      xa.ll = sa.ll;
      xa.scaling = sa.scaling;
      xa.acc_count = sa.acc_count;
      xa.inc = sa.inc;
      xa.u = sa.u;
      xa.rec_params = sa.rec_params;
      xa.rec_stats = sa.rec_stats;
      xa.rec_acc = sa.rec_acc;
      xa.q_mean = sa.q_mean;
      xa.qz = sa.qz;
      xa.lq = sa.lq;
      xa.SopT = sa.SopT;
      for (int s = 0; s < (int)S; ++s) {
        xa.s = s;
        int xrc = ext_step(e, lv, xa);
        if (xrc) return xrc;
      }
    } else if (lv.model == MODEL_USER && e->pp.kind == TDA_PROP_NUTS) {  // (the NUTS program stands in the MALA program's place as well)
      UserNutsArgs na{};
      int urc = fill_user_nuts_args(e, lv, na);
      if (urc) return urc;
      na.S = (int)S;
      na.inc = sa.inc;
      na.step0 = e->t;
      na.rec_params = sa.rec_params;
      na.rec_stats = sa.rec_stats;
      na.rec_acc = sa.rec_acc;
      if (adaptive && (e->t + S) % period == 0) {  // the period ends with this launch: the kernel applies the engine's rule itself, on its acceptance statistic
        na.scaling_out = e->scaling.p;
        na.period = period;
        na.gamma_pow = std::pow(e->pp.gamma, -(double)e->k_adapt);
        na.alpha_star = e->nuts_target;
      }
      ScopedTimer tm(e, 1);
      if ((urc = launch_user(lv.uprog_mala.steps, na, user_mala_lds(lv.uprog_mala.spec, na.m) + user_nuts_checkpoint_lds(na.max_depth, na.DP), e->stream))) return urc;
    } else if (lv.model == MODEL_USER && e->pp.kind == TDA_PROP_HMC) {  // (the HMC program stands in the MALA program's place: ensure_user_program)
      UserHmcArgs ha{};
      int urc = fill_user_hmc_args(e, lv, ha);
      if (urc) return urc;
      ha.S = (int)S;
      ha.inc = sa.inc;
      ha.u = sa.u;
      ha.rec_params = sa.rec_params;
      ha.rec_stats = sa.rec_stats;
      ha.rec_acc = sa.rec_acc;
      ScopedTimer tm(e, 1);
      if ((urc = launch_user(lv.uprog_mala.steps, ha, user_mala_lds(lv.uprog_mala.spec, ha.m), e->stream))) return urc;
    } else if (lv.model == MODEL_USER && e->pp.kind == TDA_PROP_MALA) {
      UserMalaArgs ga{};
      int urc = fill_user_mala_args(e, lv, ga);
      if (urc) return urc;
      ga.S = (int)S;
      ga.inc = sa.inc;
      ga.u = sa.u;
      ga.rec_params = sa.rec_params;
      ga.rec_stats = sa.rec_stats;
      ga.rec_acc = sa.rec_acc;
      ScopedTimer tm(e, 1);
      if ((urc = launch_user(lv.uprog_mala.steps, ga, user_mala_lds(lv.uprog_mala.spec, ga.m), e->stream))) return urc;
    } else if (lv.model == MODEL_USER) {
      UserStepArgs ua{};
      int urc = fill_user_args(e, lv, ua);
      if (urc) return urc;
      ua.S = (int)S;
      ua.mode = 0;
      ua.prop_kind = e->pp.kind;
      ua.theta = sa.theta;
      ua.lp = sa.lp;
      ua.ll = sa.ll;
      ua.scaling = sa.scaling;
      ua.acc_count = sa.acc_count;
      ua.inc = sa.inc;
      ua.u = sa.u;
      ua.rec_params = sa.rec_params;
      ua.rec_stats = sa.rec_stats;
      ua.rec_acc = sa.rec_acc;
      ScopedTimer tm(e, 1);
      if ((urc = launch_user(lv.uprog.steps, ua, lv.uprog.out_lds, e->stream))) return urc;
    } else {
      ScopedTimer tm(e, 1);
      DISPATCH_DPAD_W(e->DP, launch_steps<DPAD>(sa, NP / 16, lds, e->stream));
    }
    // ---- adaptation (proposal.py:228-245, :502-512) ----
    const bool boundary = periodic && ((e->t + S) % period == 0);
    if (is_am || (boundary && adaptive && e->pp.kind != TDA_PROP_NUTS)) {  // (NUTS: tda_user_nuts_steps has adapted already; the count of moves is reset below)
      AdaptArgs aa{};
      aa.N = N;
      aa.NP = NP;
      aa.d = d;
      aa.S = (int)S;
      aa.t_base = e->t;
      aa.do_am = is_am;
      aa.boundary = boundary;
      aa.do_scale = adaptive;
      const bool do_swap = is_am && boundary && (e->t + S >= e->pp.t0);
      aa.do_swap = do_swap;
      aa.block_moments = e->pp.block_moments != 0;
      aa.period = period;
      aa.gamma_pow = std::pow(e->pp.gamma, -(double)e->k_adapt);
      aa.sd = e->am_sd;
      aa.alpha_star = e->pp.kind == TDA_PROP_HMC ? 0.65 : e->pp.kind == TDA_PROP_MALA ? 0.57 : 0.24;  // HMC (an extension) / proposal.py:899 / :169
      aa.eps = e->pp.epsilon;
      aa.rec_params = sa.rec_params;
      aa.am_mu = e->am_mu.p;
      aa.am_sigma = e->am_sigma.p;
      aa.scaling = e->scaling.p;
      aa.acc_count = e->acc_count.p;
      aa.flags = e->flags.p;
      ScopedTimer tm(e, 2);
      static const bool fuse_ok = env_int("TINYDA_FUSE_CHOL_APPLY", 1) != 0;  // A/B switch
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
      const bool swap_apply = do_swap && split && fuse_ok && done + S < n_iter;
      if (swap_apply) {
        // C <- Sigma (proposal.py:509-510) and the next block's increments from the new factor in the same launch; that block's
        // normals were drawn under this block's steps
        // (releasing block blk + 2's draws here, ahead of the swap, was measured: k_rng next to k_chol_apply costs the swap
        // 0.07 ms and gains the steps 0.03 -- the release stays behind the swap)
        const int nb = (int)((blk + 1) & 1);
        HIP_TRY(hipStreamWaitEvent(e->stream, e->ev_rng[nb], 0));
        ap.NP = NP;
        ap.S = (int)block_len(e->t + S, n_iter - done - S);
        ap.Lk = e->Lk.p;
        ap.L_stride = (int64_t)e->DP * e->DP;
        ap.zf = e->zfrag[nb].p;
        ap.inc = e->inc.p;
        wide_fill(e, ap);
      }
      bool one_launch = false;
      if (swap_apply)  // the moment recursion, the swap and the increments in ONE launch (64 parameters: k_adapt_chol_apply)
        DISPATCH_DPAD_W(e->DP, one_launch = launch_adapt_chol_apply<DPAD>(aa, ca, ap, e->stream));
      if (one_launch) {
        inc_ready = true;
      } else {
        DISPATCH_DPAD_W(e->DP, launch_adapt<DPAD>(aa, e->stream));
        if (swap_apply) {
          int arc = TDA_OK;
          DISPATCH_DPAD_W(e->DP, arc = launch_chol_apply<DPAD>(ca, ap, e->stream));
          if (arc) return arc;
          inc_ready = true;
        } else if (do_swap) {
          DISPATCH_DPAD_W(e->DP, launch_chol<DPAD>(ca, e->stream));
        }
      }
    } else if (boundary) {
      HIP_TRY(hipMemsetAsync(e->acc_count.p, 0, NP * sizeof(int32_t), e->stream));
    }
    HIP_TRY(hipGetLastError());
    if (boundary && adaptive) e->k_adapt += 1;
    if (int mrc = mass_after_block(e, e->t, S, sa.rec_params)) return mrc;  // (warm-up adaptation of the mass: tda_host_mass.inc)

    // ---- progress mark; thinned / host-side records ----
    int rc;
    if ((rc = progress_mark(e, S, sa.rec_acc, S * N))) return rc;
    if (thin > 1) {
      // kept iterations of this block: s with (t + s + 1) % thin == 0
      const int64_t s0 = (thin - 1 - (e->t % thin)) % thin, nkeep = s0 < S ? (S - s0 + thin - 1) / thin : 0;
      hipStream_t cs = e->stream;
      if (async_host) {
        HIP_TRY(hipEventRecord(e->ev_rec[blk & 1], e->stream));
        HIP_TRY(hipStreamWaitEvent(e->copy_stream, e->ev_rec[blk & 1], 0));
        cs = e->copy_stream;
      }
      // (device destinations are gathered on the main stream, host ones copied row by row on the copy stream when page-locked)
      if ((rc = thin_out(e, o_params ? o_params + (size_t)out_row * N * d : nullptr, p_dev, blk_params, (size_t)N * d * sizeof(double), s0, nkeep, p_dev ? e->stream : cs)) ||
          (rc = thin_out(e, o_stats ? o_stats + (size_t)out_row * N * 3 : nullptr, s_dev, blk_stats, (size_t)N * 3 * sizeof(double), s0, nkeep, s_dev ? e->stream : cs)) ||
          (rc = thin_out(e, o_acc ? o_acc + (size_t)out_row * N : nullptr, a_dev, blk_acc, (size_t)N, s0, nkeep, a_dev ? e->stream : cs)))
        return rc;
      if (async_host) HIP_TRY(hipEventRecord(e->ev_cp[blk & 1], e->copy_stream));
      else if (any_host) HIP_TRY(hipStreamSynchronize(e->stream));  // block buffers are reused next iteration
      out_row += nkeep;
    } else if (async_host) {
      const int i = (int)(blk & 1);
      HIP_TRY(hipEventRecord(e->ev_rec[i], e->stream));
      HIP_TRY(hipStreamWaitEvent(e->copy_stream, e->ev_rec[i], 0));
      if (o_params && !p_dev)
        HIP_TRY(hipMemcpyAsync(o_params + (size_t)done * N * d, blk_params, (size_t)S * N * d * sizeof(double), hipMemcpyDeviceToHost, e->copy_stream));
      if (o_stats && !s_dev)
        HIP_TRY(hipMemcpyAsync(o_stats + (size_t)done * N * 3, blk_stats, (size_t)S * N * 3 * sizeof(double), hipMemcpyDeviceToHost, e->copy_stream));
      if (o_acc && !a_dev)
        HIP_TRY(hipMemcpyAsync(o_acc + (size_t)done * N, blk_acc, (size_t)S * N, hipMemcpyDeviceToHost, e->copy_stream));
      HIP_TRY(hipEventRecord(e->ev_cp[i], e->copy_stream));
    } else {
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
      if (host_copies) HIP_TRY(hipStreamSynchronize(e->stream));  // block buffers are reused next iteration
    }

    e->t += S;
    done += S;
    blk += 1;
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
