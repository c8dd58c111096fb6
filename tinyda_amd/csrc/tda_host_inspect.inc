// Part of libtinyda_hip.so: included by tda_engine.hip (ONE translation unit -- the helpers, the engine struct and the kernel
// launchers above it are visible here).  Proposal state (live and detached snapshots), flags, tda_engine_evaluate, RNG probes, profiling.
namespace {
// what tda_engine_get_proposal_state reads: the engine's own buffers, or the ones a snapshot took over from it
struct PropView {
  int device = 0, d = 0, DP = 0, kind = 0;
  int64_t N = 0, NP = 0, t = 0, k = 0;
  bool L_shared = true;
  const double *Lk = nullptr, *am_mu = nullptr, *am_sigma = nullptr, *scaling = nullptr;
  // 65 .. 128 parameters (tda_kernels_wide.h): the factor as tiles in two buffers, its diagonal tiles, the current-buffer selector
  bool wide = false;
  const double* ud = nullptr;
  const int32_t* sel = nullptr;
};

int read_proposal_view(const PropView& v, double* scaling, double* C, double* am_mu, double* am_sigma, int64_t* counters) {
  const int d = v.d, DP = v.DP;
  const int64_t N = v.N, NP = v.NP;
  if (scaling) {
    std::vector<double> h(NP);
    HIP_TRY(hipMemcpy(h.data(), v.scaling, NP * sizeof(double), hipMemcpyDeviceToHost));
    std::copy(h.begin(), h.begin() + N, scaling);
  }
  if (C && v.wide) {  // C = L L^T from the tiles of the current buffer of every chain
    const int64_t nL = v.L_shared ? 1 : NP;
    std::vector<double> hf((size_t)2 * nL * tda::WIDE_FACTOR_DOUBLES), hu((size_t)2 * nL * tda::WIDE_UD_DOUBLES);
    std::vector<int32_t> hs(NP, 0);
    HIP_TRY(hipMemcpy(hf.data(), v.Lk, hf.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(hu.data(), v.ud, hu.size() * sizeof(double), hipMemcpyDeviceToHost));
    if (!v.L_shared) HIP_TRY(hipMemcpy(hs.data(), v.sel, NP * sizeof(int32_t), hipMemcpyDeviceToHost));
    auto unpack = [&](int64_t c0, int64_t c1) {
      std::vector<double> L;
      for (int64_t c = c0; c < c1; ++c) {
        const int64_t cf = v.L_shared ? 0 : c;
        const double* f = hf.data() + ((size_t)hs[cf] * nL + cf) * tda::WIDE_FACTOR_DOUBLES;
        const double* u = hu.data() + ((size_t)hs[cf] * nL + cf) * tda::WIDE_UD_DOUBLES;
        wide_factor_unpack_host(f, u, d, L);
        double* Cc = C + (size_t)c * d * d;
        for (int i = 0; i < d; ++i)
          for (int j = 0; j <= i; ++j) {
            double acc = 0.0;
            for (int k = 0; k <= j; ++k) acc += L[(size_t)i * d + k] * L[(size_t)j * d + k];
            Cc[(size_t)i * d + j] = Cc[(size_t)j * d + i] = acc;
          }
      }
    };
    if (v.L_shared) {
      unpack(0, 1);
      for (int64_t c = 1; c < N; ++c) std::copy(C, C + (size_t)d * d, C + (size_t)c * d * d);
    } else {
      host_chain_ranges(N, unpack);
    }
  } else if (C) {  // C = L L^T from the factor in use
    const int64_t nL = v.L_shared ? 1 : NP;
    std::vector<double> h((size_t)nL * DP * DP);
    HIP_TRY(hipMemcpy(h.data(), v.Lk, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    // C = L L^T as d rank-1 updates per chain (the innermost loop runs over contiguous memory and vectorises; every
    // element still accumulates its products in ascending k); a factor shared by all chains is multiplied out once
    auto unpack = [&](int64_t c0, int64_t c1) {
      std::vector<double> acc((size_t)d * d);
      for (int64_t c = c0; c < c1; ++c) {
        const double* Lc = h.data() + (size_t)c * DP * DP;
        std::fill(acc.begin(), acc.end(), 0.0);
        for (int k = 0; k < d; ++k) {
          const double* Lk = Lc + (size_t)k * DP;  // column k of L: Lk[i] = L[i][k], zero for i < k
          for (int i = k; i < d; ++i) {
            const double lik = Lk[i];
            double* row = acc.data() + (size_t)i * d;
            for (int j = k; j <= i; ++j) row[j] += lik * Lk[j];
          }
        }
        double* Cc = C + (size_t)c * d * d;
        for (int i = 0; i < d; ++i)
          for (int j = 0; j <= i; ++j) Cc[(size_t)i * d + j] = Cc[(size_t)j * d + i] = acc[(size_t)i * d + j];
      }
    };
    if (v.L_shared) {
      unpack(0, 1);
      for (int64_t c = 1; c < N; ++c) std::copy(C, C + (size_t)d * d, C + (size_t)c * d * d);
    } else {
      host_chain_ranges(N, unpack);
    }
  }
  if (am_mu || am_sigma) {
    if (v.kind != TDA_PROP_AM) return fail(TDA_ERR_STATE, "proposal has no running moments");
    if (am_mu) {
      std::vector<double> h((size_t)NP * DP);
      HIP_TRY(hipMemcpy(h.data(), v.am_mu, h.size() * sizeof(double), hipMemcpyDeviceToHost));
      for (int64_t c = 0; c < N; ++c)
        for (int j = 0; j < d; ++j) am_mu[(size_t)c * d + j] = h[(size_t)c * DP + j];
    }
    if (am_sigma && v.wide) {  // dense symmetric matrices from the upper tiles (k_wide_adapt)
      const size_t per = tda::WIDE_FACTOR_DOUBLES;
      std::vector<double> h((size_t)N * per);
      HIP_TRY(hipMemcpy(h.data(), v.am_sigma, h.size() * sizeof(double), hipMemcpyDeviceToHost));
      host_chain_ranges(N, [&](int64_t c0, int64_t c1) {
        for (int64_t c = c0; c < c1; ++c) {
          const double* f = h.data() + (size_t)c * per;
          for (int i = 0; i < d; ++i)
            for (int j = 0; j < d; ++j) am_sigma[((size_t)c * d + i) * d + j] = f[tda::aemr_u_offset(128, std::min(i, j), std::max(i, j))];
        }
      });
    } else if (am_sigma) {  // dense symmetric matrices from the lower-tile storage
      const size_t per = (size_t)am_tiles_rt(DP) * 256;
      std::vector<double> h((size_t)N * per);
      HIP_TRY(hipMemcpy(h.data(), v.am_sigma, h.size() * sizeof(double), hipMemcpyDeviceToHost));
      host_chain_ranges(N, [&](int64_t c0, int64_t c1) {
        for (int64_t c = c0; c < c1; ++c) {
          const double* f = h.data() + (size_t)c * per;
          for (int i = 0; i < d; ++i)
            for (int j = 0; j < d; ++j)
              am_sigma[((size_t)c * d + i) * d + j] = f[am_sigma_offset(std::max(i, j), std::min(i, j))];
        }
      });
    }
  }
  if (counters) {
    counters[0] = v.t;
    counters[1] = v.k;
  }
  return TDA_OK;
}

PropView view_of(const tda_engine* e) {
  PropView v;
  v.device = e->cfg.device;
  v.d = e->d;
  v.DP = e->DP;
  v.kind = e->is_dreamz ? TDA_PROP_DREAMZ : e->pp.kind;
  v.N = e->N;
  v.NP = e->NP;
  v.t = e->t;
  v.k = e->k_adapt;
  v.L_shared = e->L_shared;
  v.Lk = e->Lk.p;
  v.am_mu = e->am_mu.p;
  v.am_sigma = e->am_sigma.p;
  v.scaling = e->scaling.p;
  v.wide = e->wide;
  v.ud = e->wide_ud.p;
  v.sel = e->wide_sel.p;
  return v;
}
}  // namespace

// the proposal state of an engine that is about to be destroyed: the buffers themselves, taken over without a copy
struct tda_proposal_snapshot {
  PropView v;
  DevBuf<double> Lk, am_mu, am_sigma, scaling, wide_ud;
  DevBuf<int32_t> wide_sel;
};

extern "C" {

int tda_engine_get_proposal_state(tda_engine* e, double* scaling, double* C, double* am_mu, double* am_sigma,
                                  int64_t* counters) {
  if (!e || !e->inited) return fail(TDA_ERR_STATE, "engine not initialised");
  HIP_TRY(hipSetDevice(e->cfg.device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (C && !e->Lk.p) return fail(TDA_ERR_STATE, "this proposal has no covariance factor");
  return read_proposal_view(view_of(e), scaling, C, am_mu, am_sigma, counters);
}

int tda_engine_detach_proposal_state(tda_engine* e, tda_proposal_snapshot** out) {
  if (!e || !e->inited || !out) return fail(TDA_ERR_STATE, "engine not initialised");
  HIP_TRY(hipSetDevice(e->cfg.device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (e->rng_stream) HIP_TRY(hipStreamSynchronize(e->rng_stream));
  tda_proposal_snapshot* s = new tda_proposal_snapshot();
  s->v = view_of(e);
  auto take = [](DevBuf<double>& dst, DevBuf<double>& src) {
    dst.p = src.p;
    dst.n = src.n;
    dst.dev = src.dev;
    src.p = nullptr;
    src.n = 0;
  };
  take(s->Lk, e->Lk);
  take(s->am_mu, e->am_mu);
  take(s->am_sigma, e->am_sigma);
  take(s->scaling, e->scaling);
  take(s->wide_ud, e->wide_ud);
  s->wide_sel.p = e->wide_sel.p;
  s->wide_sel.n = e->wide_sel.n;
  s->wide_sel.dev = e->wide_sel.dev;
  e->wide_sel.p = nullptr;
  e->wide_sel.n = 0;
  e->inited = false;  // the engine has given its proposal away: only tda_engine_destroy is left for it
  *out = s;
  return TDA_OK;
}

int tda_proposal_snapshot_read(tda_proposal_snapshot* s, double* scaling, double* C, double* am_mu, double* am_sigma, int64_t* counters) {
  if (!s) return fail(TDA_ERR_INVALID, "null snapshot");
  HIP_TRY(hipSetDevice(s->v.device));
  if (C && !s->v.Lk) return fail(TDA_ERR_STATE, "this proposal has no covariance factor");
  return read_proposal_view(s->v, scaling, C, am_mu, am_sigma, counters);
}

void tda_proposal_snapshot_destroy(tda_proposal_snapshot* s) {
  if (!s) return;
  (void)hipSetDevice(s->v.device);
  g_pool_accepting = true;  // nothing is queued on these buffers (detach synchronised the engine's streams)
  delete s;
  g_pool_accepting = false;
}

int tda_engine_get_flags(tda_engine* e, int32_t* flags) {
  if (!e || !e->inited || !flags) return fail(TDA_ERR_STATE, "engine not initialised");
  HIP_TRY(hipSetDevice(e->cfg.device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  std::vector<int32_t> h(e->NP);
  HIP_TRY(hipMemcpy(h.data(), e->flags.p, e->NP * sizeof(int32_t), hipMemcpyDeviceToHost));
  std::copy(h.begin(), h.begin() + e->N, flags);
  return TDA_OK;
}

int tda_engine_evaluate(tda_engine* e, int level, const double* theta, int64_t n, double* stats) {
  if (!e || !theta || !stats) return fail(TDA_ERR_INVALID, "null argument");
  if (!e->prior_set) return fail(TDA_ERR_STATE, "set_prior missing");
  if (level < 0 || level >= (int)e->levels.size() || !e->levels[level].set) return fail(TDA_ERR_STATE, "level %d not set", level);
  if (n < 1 || n > e->N) return fail(TDA_ERR_INVALID, "n must be in 1..n_chains");
  HIP_TRY(hipSetDevice(e->cfg.device));
  int rc;
  if ((rc = ensure_user_programs(e))) return rc;
  const int64_t NP = e->NP;
  if (!e->theta_s.p) {
    if ((rc = e->theta_s.alloc((size_t)NP * e->DP))) return rc;
    if ((rc = e->lp_s.alloc(NP))) return rc;
    if ((rc = e->ll_s.alloc(NP))) return rc;
  }
  if (!e->scaling.p) {
    std::vector<double> sc(NP, 1.0);
    if ((rc = e->scaling.upload(sc))) return rc;
  }
  if ((rc = upload_states(e, theta, n, e->theta_s.p))) return rc;
  if ((rc = launch_eval(e, level, e->theta_s.p, e->lp_s.p, e->ll_s.p))) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));
  std::vector<double> a(NP), b(NP), o((size_t)n * 3);
  HIP_TRY(hipMemcpy(a.data(), e->lp_s.p, NP * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(b.data(), e->ll_s.p, NP * sizeof(double), hipMemcpyDeviceToHost));
  for (int64_t c = 0; c < n; ++c) {
    o[c * 3] = a[c];
    o[c * 3 + 1] = b[c];
    o[c * 3 + 2] = a[c] + b[c];
  }
  HIP_TRY(hipMemcpy(stats, o.data(), o.size() * sizeof(double), is_device_ptr(stats) ? hipMemcpyHostToDevice : hipMemcpyHostToHost));
  return TDA_OK;
}

int tda_engine_rng_probe(tda_engine* e, int64_t step, double* z, double* u) {
  if (!e || !z || !u) return fail(TDA_ERR_INVALID, "null argument");
  if (e->wide) return fail(TDA_ERR_UNSUPPORTED, "rng_probe is not lowered for more than 64 parameters (set_export hands out the same variates)");
  HIP_TRY(hipSetDevice(e->cfg.device));
  const int d = e->d, DP = e->DP;
  const int64_t N = e->N, NP = e->NP;
  DevBuf<double> Lid, inc, ub, zd, ud;
  std::vector<double> I((size_t)DP * DP, 0.0);
  for (int j = 0; j < DP; ++j) I[(size_t)j * DP + j] = 1.0;
  int rc;
  if ((rc = Lid.upload(I))) return rc;
  if ((rc = inc.alloc((size_t)NP * DP))) return rc;
  if ((rc = ub.alloc(NP))) return rc;
  if ((rc = zd.alloc((size_t)N * d))) return rc;
  if ((rc = ud.alloc(N))) return rc;
  ProposeArgs pa{};
  pa.N = N;
  pa.NP = NP;
  pa.chain_offset = e->cfg.chain_offset;
  pa.d = d;
  pa.S = 1;
  pa.step0 = step;
  pa.seed = e->cfg.seed;
  pa.Lk = Lid.p;
  pa.L_stride = 0;
  pa.inc = inc.p;
  pa.u = ub.p;
  pa.z_export = zd.p;
  pa.u_export = ud.p;
  int prc = TDA_OK;
  DISPATCH_DPAD(DP, prc = launch_propose<DPAD>(pa, e->stream));
  if (prc) return prc;
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemcpy(z, zd.p, (size_t)N * d * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(u, ud.p, (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
  return TDA_OK;
}

namespace {
__global__ void k_philox_probe(const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  if (threadIdx.x == 0) {
    const tda::u32x4 r = tda::philox4x32_10(tda::u32x4{in[0], in[1], in[2], in[3]}, in[4], in[5]);
    out[0] = r.x;
    out[1] = r.y;
    out[2] = r.z;
    out[3] = r.w;
  }
}
}  // namespace

int tda_rng_philox(int device, const uint32_t* counter, const uint32_t* key, uint32_t* out) {
  if (!counter || !key || !out) return fail(TDA_ERR_INVALID, "null argument");
  if (device < 0) {  // the same header compiled for the host
    const tda::u32x4 r = tda::philox4x32_10(tda::u32x4{counter[0], counter[1], counter[2], counter[3]}, key[0], key[1]);
    out[0] = r.x;
    out[1] = r.y;
    out[2] = r.z;
    out[3] = r.w;
    return TDA_OK;
  }
  HIP_TRY(hipSetDevice(device));
  DevBuf<uint32_t> in, res;
  int rc;
  std::vector<uint32_t> h = {counter[0], counter[1], counter[2], counter[3], key[0], key[1]};
  if ((rc = in.upload(h))) return rc;
  if ((rc = res.alloc(4))) return rc;
  hipLaunchKernelGGL(k_philox_probe, dim3(1), dim3(64), 0, nullptr, in.p, res.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, res.p, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return TDA_OK;
}

#ifdef TDA_DA_TRACE
extern "C" int tda_debug_da_trace(long long* out) {  // debug builds only (tools/da_trace.py)
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(tda::g_da_trace), sizeof(long long) * 128 * 8 * 8));
  return TDA_OK;
}
#endif

int tda_engine_set_profiling(tda_engine* e, int enable) {
  if (!e) return fail(TDA_ERR_INVALID, "null engine");
  e->profiling = enable != 0;
  return TDA_OK;
}

int tda_engine_get_profile(tda_engine* e, tda_profile* p) {
  if (!e || !p) return fail(TDA_ERR_INVALID, "null argument");
  if (p->struct_size != sizeof(tda_profile) && p->struct_size != 48) return fail(TDA_ERR_INVALID, "tda_profile.struct_size mismatch");
  HIP_TRY(hipSetDevice(e->cfg.device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  const uint32_t ss = p->struct_size;
  const bool v4 = ss == sizeof(tda_profile);  // a 0.3 caller's struct ends after ms_total: the error-model time stays under `adapt`
  memset(p, 0, ss);
  p->struct_size = ss;
  for (auto& t : e->timed) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, t.a, t.b));
    if (t.kind == 0) {
      p->ms_propose += ms;
      p->n_launch_propose++;
    } else if (t.kind == 1) {
      p->ms_steps += ms;
      p->n_launch_steps++;
    } else if (t.kind == 3 && v4) {
      p->ms_aem += ms;
      p->n_launch_aem++;
    } else {
      p->ms_adapt += ms;
      p->n_launch_adapt++;
    }
  }
  if (!e->timed.empty()) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e->timed.front().a, e->timed.back().b));
    p->ms_total = ms;
  }
  return TDA_OK;
}

}  // extern "C"
