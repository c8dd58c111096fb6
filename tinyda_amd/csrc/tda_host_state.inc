// Part of libtinyda_hip.so: included by tda_engine.hip (ONE translation unit -- the helpers, the engine struct and the kernel
// launchers above it are visible here).  Pooled-moment extension entry points and the checkpoint blob (get_state / set_state).
extern "C" {

int tda_engine_reduce_moments(tda_engine* e, const double* rows, int64_t n_rows, double* out) {
  if (!e || !rows || !out) return fail(TDA_ERR_INVALID, "null argument");
  if (!is_device_ptr(rows)) return fail(TDA_ERR_INVALID, "reduce_moments needs a device record buffer");
  if (n_rows < 1) return fail(TDA_ERR_INVALID, "n_rows must be >= 1");
  HIP_TRY(hipSetDevice(e->cfg.device));
  const int d = e->d, DP = e->DP;
  const int64_t nb = (n_rows + MOM_CHUNK - 1) / MOM_CHUNK;
  DevBuf<double> partial, outd;
  int rc;
  if ((rc = partial.alloc((size_t)nb * (DP + (size_t)DP * DP)))) return rc;
  const bool odev = is_device_ptr(out);
  const size_t nout = 1 + d + (size_t)d * d;
  if (!odev && (rc = outd.alloc(nout))) return rc;
  double* o = odev ? out : outd.p;
  if (DP == 128) {  // (S[128] per lane would spill: each block accumulates 64 rows of sum x x^T, blockIdx.y picks which)
    hipLaunchKernelGGL(k_moments_partial_w, dim3((unsigned)nb, 2), dim3(128), 0, e->stream, rows, n_rows, d, partial.p);
    hipLaunchKernelGGL(k_moments_final_w, dim3((unsigned)(d + 1)), dim3(128), 0, e->stream, partial.p, nb, n_rows, d, o);
  } else {
    DISPATCH_DPAD(DP, hipLaunchKernelGGL(k_moments_partial<DPAD>, dim3((unsigned)nb), dim3(64), 0, e->stream, rows, n_rows, d, partial.p));
    DISPATCH_DPAD(DP, hipLaunchKernelGGL(k_moments_final<DPAD>, dim3((unsigned)(d + 1)), dim3(64), 0, e->stream, partial.p, nb, n_rows, d, o));
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (!odev) HIP_TRY(hipMemcpy(out, outd.p, nout * sizeof(double), hipMemcpyDeviceToHost));
  return TDA_OK;
}

int tda_engine_set_proposal_covariance(tda_engine* e, const double* C) {
  if (!e || !C) return fail(TDA_ERR_INVALID, "null argument");
  if (!e->inited || e->pp.kind != TDA_PROP_GRW || !e->L_shared)
    return fail(TDA_ERR_STATE, "set_proposal_covariance applies to an initialised GaussianRandomWalk engine");
  HIP_TRY(hipSetDevice(e->cfg.device));
  const int d = e->d, DP = e->DP;
  std::vector<double> Ch(C, C + (size_t)d * d), L;
  if (!cholesky_host(Ch.data(), d, L)) return fail(TDA_ERR_NUMERIC, "proposal covariance is not positive definite");
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (e->wide) {  // the shared factor's tiles: buffer 0 of the factor and of its diagonal tiles (a shared factor is never swapped)
    std::vector<double> fac, ud;
    wide_factor_pack_host(L, d, fac, ud);
    HIP_TRY(hipMemcpy(e->Lk.p, fac.data(), fac.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->wide_ud.p, ud.data(), ud.size() * sizeof(double), hipMemcpyHostToDevice));
  } else {
    std::vector<double> Lk((size_t)DP * DP, 0.0);
    for (int j = 0; j < d; ++j)
      for (int k = 0; k <= j; ++k) Lk[(size_t)k * DP + j] = L[(size_t)j * d + k];
    HIP_TRY(hipMemcpy(e->Lk.p, Lk.data(), Lk.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  e->prop_C_h = Ch;
  e->L_identity = false;
  return TDA_OK;
}

namespace {
// "SDATTDA" + format digit.  Format 4 (ABI 0.5, second half of the round): per-level counters for six levels.  Format 3: the error model kept
// as the Cholesky factor in factor form (tda_kernels_aemr.h), four levels.
// Format 2 (ABI 0.4): the error model as the triangular inverse V = L^-1; DREAM(Z) RNG contract of 0.4, the record-thinning setting
// inside the blob.  Format-1 blobs (<= 0.3) have the same item count for the same configuration and would be continued on a different
// variate stream.  Older formats are refused by magic.
constexpr uint64_t TDA_STATE_MAGIC = 0x3441445454414453ull;
struct StateItem {
  void* p;
  size_t bytes;
  bool device;
  bool check = false;  // a host item that set_state compares with the engine's own value and refuses on a difference
};

// every piece of mutable state of an initialised engine, in a fixed order for its configuration
void enumerate_state(tda_engine* e, std::vector<StateItem>& v) {
  auto dev = [&](auto& buf) {
    if (buf.p && buf.n) v.push_back({(void*)buf.p, buf.n * sizeof(*buf.p), true});
  };
  auto host = [&](void* p, size_t b) { v.push_back({p, b, false}); };
  host(&e->t, sizeof e->t);
  host(&e->k_adapt, sizeof e->k_adapt);
  host(&e->thin, sizeof e->thin);  // (checked, not adopted: set_state refuses a blob saved under another record thinning)
  dev(e->theta);
  dev(e->lp);
  dev(e->ll);
  dev(e->scaling);
  dev(e->acc_count);
  dev(e->flags);
  dev(e->Lk);
  dev(e->wide_ud);   // (65 .. 128 parameters: the factor's diagonal tiles and the current-buffer selector)
  dev(e->wide_sel);
  dev(e->am_mu);
  dev(e->am_sigma);
  dev(e->lq);
  dev(e->mala_grad);
  dev(e->nuts_accsum);  // (a NUTS engine alone holds these two: the running period's acceptance sum and the per-chain totals)
  dev(e->nuts_totals);
  if (e->mass_W > 0 && e->mass_mean.p) {  // a mass-adapting HMC / NUTS engine alone (tinyda_amd_mass.h)
    v.push_back({&e->mass_W, sizeof e->mass_W, false, true});  // (checked, not adopted: the schedule is the engine's configuration)
    v.push_back({&e->pp.period, sizeof e->pp.period, false, true});
    host(&e->mass_n, sizeof e->mass_n);
    host(&e->mass_updates, sizeof e->mass_updates);
    dev(e->hmc_inv_mass);
    dev(e->mass_mean);
    dev(e->mass_M2);
    dev(e->mass_refused);
  }
  if (e->dmass_W > 0 && e->dmass_S1.p) {  // a dense-adapting HMC / NUTS engine alone (tinyda_amd_dense_mass_adaptation.h)
    v.push_back({&e->dmass_W, sizeof e->dmass_W, false, true});  // (checked, not adopted, like the diagonal adaptation's)
    v.push_back({&e->pp.period, sizeof e->pp.period, false, true});
    host(&e->mass_n, sizeof e->mass_n);
    host(&e->mass_updates, sizeof e->mass_updates);
    dev(e->mass_refused);
    dev(e->dmass_a);
    dev(e->dense_chol);
    dev(e->dmass_S1);
    dev(e->dmass_S2);
  }
  if (e->nlev > 1) {
    host(e->cnt, sizeof e->cnt);
    host(e->done, sizeof e->done);
    host(&e->ring_pos, sizeof e->ring_pos);
    host(e->aem_bt, sizeof e->aem_bt);
    dev(e->ml_theta);
    dev(e->ml_lp);
    dev(e->ml_ll);
    dev(e->ml_S);
    dev(e->ml_anyacc);
    dev(e->ml_ysnap);
    dev(e->ml_pick);
    dev(e->ml_ring);
    dev(e->ml_sid);
    for (int k = 0; k < MAXLEV; ++k) {
      dev(e->aem_bias[k]);
      dev(e->aem_covinv[k]);
      dev(e->aem_bmu[k]);
      dev(e->aem_bsig[k]);
      dev(e->aem_mdiff[k]);
      dev(e->ext_Fcur[k]);
      dev(e->aemd_F[k]);
      dev(e->aemd_bias[k]);
      dev(e->aemd_w[k]);
      dev(e->aemd_mu[k]);
      dev(e->aemd_var[k]);
      dev(e->aemd_md[k]);
    }
    dev(e->ext_Fst);
    dev(e->aemd_Fst);
  }
  if (e->is_dreamz) {
    host(&e->arch_rows, sizeof e->arch_rows);
    host(&e->sums_rows, sizeof e->sums_rows);
    host(&e->pending_steps, sizeof e->pending_steps);
    if (e->dist_ranks) {  // distributed archive: the publish protocol's position (the peer mappings belong to the process, not the state)
      host(&e->dist_steps, sizeof e->dist_steps);
      host(&e->dist_pending, sizeof e->dist_pending);
      host(e->dist_unpub, sizeof e->dist_unpub);
      host(&e->dist_n_unpub, sizeof e->dist_n_unpub);
      host(&e->dist_adapt_rows, sizeof e->dist_adapt_rows);
      host(&e->dist_sum_steps, sizeof e->dist_sum_steps);
      host(&e->dist_m0_summed, sizeof e->dist_m0_summed);
      host(&e->dist_adapt_pending, sizeof e->dist_adapt_pending);
      host(&e->dist_adapt_gamma, sizeof e->dist_adapt_gamma);
    }
    dev(e->arch);
    dev(e->zsum);
    dev(e->zsq);
    dev(e->dz_pCR);
    dev(e->dz_LCR);
    dev(e->dz_Delta);
    dev(e->dz_mcr_last);
    dev(e->theta_prev);
    dev(e->blk_hist);
  }
}
}  // namespace

int64_t tda_engine_state_size(tda_engine* e) {
  if (!e || !e->inited) return fail(TDA_ERR_STATE, "engine not initialised");
  std::vector<StateItem> v;
  enumerate_state(e, v);
  int64_t n = 16;  // header: magic + item count
  for (auto& it : v) n += 8 + (int64_t)it.bytes;
  return n;
}

int tda_engine_get_state(tda_engine* e, void* blob, int64_t bytes) {
  if (!e || !e->inited || !blob) return fail(TDA_ERR_STATE, "engine not initialised");
  if (bytes != tda_engine_state_size(e)) return fail(TDA_ERR_INVALID, "state blob must be exactly tda_engine_state_size() bytes");
  HIP_TRY(hipSetDevice(e->cfg.device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  std::vector<StateItem> v;
  enumerate_state(e, v);
  char* o = (char*)blob;
  const uint64_t magic = TDA_STATE_MAGIC, cnt = v.size();
  memcpy(o, &magic, 8);
  memcpy(o + 8, &cnt, 8);
  o += 16;
  for (auto& it : v) {
    const uint64_t b = it.bytes;
    memcpy(o, &b, 8);
    o += 8;
    if (it.device) HIP_TRY(hipMemcpy(o, it.p, it.bytes, hipMemcpyDeviceToHost));
    else memcpy(o, it.p, it.bytes);
    o += it.bytes;
  }
  return TDA_OK;
}

int tda_engine_set_state(tda_engine* e, const void* blob, int64_t bytes) {
  if (!e || !e->inited || !blob) return fail(TDA_ERR_STATE, "engine not initialised (configure and init() it like the saved one first)");
  if (bytes != tda_engine_state_size(e)) return fail(TDA_ERR_INVALID, "state blob does not match this engine's configuration");
  HIP_TRY(hipSetDevice(e->cfg.device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  std::vector<StateItem> v;
  enumerate_state(e, v);
  const char* o = (const char*)blob;
  uint64_t magic, cnt;
  memcpy(&magic, o, 8);
  memcpy(&cnt, o + 8, 8);
  if (magic == 0x3141445454414453ull)
    return fail(TDA_ERR_INVALID, "state blob written by tinyda_amd <= 0.3: its DREAM(Z) variate stream and error-model layout differ (format 1), refusing to continue on it");
  if (magic == 0x3241445454414453ull)
    return fail(TDA_ERR_INVALID, "state blob written by tinyda_amd 0.4 (format 2): its error-model layout (V = L^-1) differs from this release's factor form, refusing to continue on it");
  if (magic != TDA_STATE_MAGIC || cnt != v.size()) return fail(TDA_ERR_INVALID, "not a state blob of this engine configuration");
  o += 16;
  const int thin_now = e->thin;
  {  // third item: the record thinning the blob was saved under (which iterations reach the caller depends on it and on t)
    const char* q = o;
    for (int i = 0; i < 2; ++i) {
      uint64_t b;
      memcpy(&b, q, 8);
      q += 8 + b;
    }
    int thin_saved;
    memcpy(&thin_saved, q + 8, sizeof thin_saved);
    if (thin_saved != thin_now)
      return fail(TDA_ERR_INVALID, "state blob was saved with record thinning %d, this engine is set to %d", thin_saved, thin_now);
  }
  {  // the checked items first, so that a refused blob leaves the engine as it was
    const char* q = o;
    for (auto& it : v) {
      uint64_t b;
      memcpy(&b, q, 8);
      if (b != it.bytes) return fail(TDA_ERR_INVALID, "state blob layout mismatch");
      if (it.check && memcmp(it.p, q + 8, it.bytes) != 0)
        return fail(TDA_ERR_INVALID, "state blob was saved under another mass adaptation (warm-up steps or period differ from this engine's)");
      q += 8 + b;
    }
  }
  for (auto& it : v) {
    uint64_t b;
    memcpy(&b, o, 8);
    if (b != it.bytes) return fail(TDA_ERR_INVALID, "state blob layout mismatch");
    o += 8;
    if (it.check) {
      o += it.bytes;
      continue;
    }
    if (it.device) HIP_TRY(hipMemcpy(it.p, o, it.bytes, hipMemcpyHostToDevice));
    else memcpy(it.p, o, it.bytes);
    o += it.bytes;
  }
  if (e->L_identity) {  // derived from the factor at init(): the restored one may come from tda_engine_set_proposal_covariance
    const int d = e->d, DP = e->DP;
    std::vector<double> Lh((size_t)DP * DP, 0.0);
    if (e->wide) {  // (65 .. 128 parameters: the shared factor's tiles, buffer 0; dense again, k-major like the narrow factor)
      std::vector<double> f(WIDE_FACTOR_DOUBLES), u(WIDE_UD_DOUBLES), L;
      HIP_TRY(hipMemcpy(f.data(), e->Lk.p, f.size() * sizeof(double), hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy(u.data(), e->wide_ud.p, u.size() * sizeof(double), hipMemcpyDeviceToHost));
      wide_factor_unpack_host(f.data(), u.data(), d, L);
      for (int j = 0; j < d; ++j)
        for (int k = 0; k <= j; ++k) Lh[(size_t)k * DP + j] = L[(size_t)j * d + k];
    } else {
      HIP_TRY(hipMemcpy(Lh.data(), e->Lk.p, Lh.size() * sizeof(double), hipMemcpyDeviceToHost));
    }
    for (int k = 0; k < d && e->L_identity; ++k)
      for (int j = 0; j < d; ++j)
        if (Lh[(size_t)k * DP + j] != (j == k ? 1.0 : 0.0)) {
          e->L_identity = false;
          break;
        }
  }
  return TDA_OK;
}

}  // extern "C"
