// Model outputs and quantities of interest of recorded parameters (include/tinyda_amd_replay.h; included by tda_engine.hip):
// the host side of tda_user_replay.  No tda_engine: sample() has closed its engine by the time a result is read, so the replay
// is a small object of its own -- one compiled program (compile_user_program, the one hiprtc call site) and a device counter.
#include "tinyda_amd_replay.h"

struct tda_replay {
  int device = 0, d = 0, m = 0, nq = 0;
  UserProgram prog;
  size_t lds = 0;               // of one workgroup, static and dynamic: what decides how many are resident (replay_segment_rows)
  long long* d_count = nullptr;  // model evaluations of one run
};

extern "C" {

int tda_replay_create(int device, const char* source, int32_t dim, int32_t n_outputs, int32_t n_qoi, tda_replay** out) {
  if (!source || !out) return fail(TDA_ERR_INVALID, "null argument");
  if (dim < 1 || dim > 128) return fail(TDA_ERR_UNSUPPORTED, "dim=%d outside the device engine's range 1..128", dim);
  if (n_outputs < 1 || n_qoi < 0) return fail(TDA_ERR_INVALID, "n_outputs must be >= 1 and n_qoi >= 0");
  const UserForms forms = user_forms(source);
  if (!forms.forward_wave && !source_defines(source, "tda_forward"))
    return fail(TDA_ERR_INVALID, "the source defines neither tda_forward nor %s", TDA_SIG_FORWARD_WAVE);
  if (n_qoi > 0 && !forms.qoi && !forms.qoi_wave)
    return fail(TDA_ERR_INVALID, "n_qoi = %d, but the source defines neither %s nor %s", n_qoi, TDA_SIG_QOI, TDA_SIG_QOI_WAVE);
  if (n_qoi == 0 && (forms.qoi || forms.qoi_wave))
    return fail(TDA_ERR_INVALID, "the source defines %s, but n_qoi = 0", forms.qoi_wave ? TDA_SIG_QOI_WAVE : TDA_SIG_QOI);
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (ndev < 1) return fail(TDA_ERR_HIP, "no HIP device visible: the replay has no CPU fallback");
  if (device < 0 || device >= ndev) return fail(TDA_ERR_INVALID, "device %d of %d", device, ndev);
  HIP_TRY(hipSetDevice(device));
  UserProgramSpec spec;
  spec.replay = true;
  spec.forward_wave = forms.forward_wave;
  spec.qoi_form = n_qoi == 0 ? 0 : forms.qoi_wave ? 2 : 1;  // (both forms: the wave form, as for tda_forward_wave)
  tda_replay* r = new tda_replay();
  r->device = device, r->d = dim, r->m = n_outputs, r->nq = n_qoi;
  int rc = compile_user_program(source, spec, n_outputs, &r->prog, n_qoi);
  if (rc == TDA_OK) {
    int stat = 0;
    hipError_t er = hipFuncGetAttribute(&stat, HIP_FUNC_ATTRIBUTE_SHARED_SIZE_BYTES, r->prog.replay);
    if (er == hipSuccess) er = hipMalloc((void**)&r->d_count, sizeof(long long));
    if (er != hipSuccess) rc = fail(TDA_ERR_HIP, "tda_replay_create: %s", hipGetErrorString(er));
    r->lds = (size_t)stat + r->prog.out_lds;
  }
  if (rc != TDA_OK) {
    r->prog.unload();
    delete r;
    return rc;
  }
  *out = r;
  return TDA_OK;
}

int tda_replay_run(tda_replay* r, const double* params, int64_t rows, int64_t n_chains, int64_t segment_rows, double* outputs,
                   double* qoi, int64_t* n_evaluated, void* stream) {
  if (!r || !params) return fail(TDA_ERR_INVALID, "null argument");
  if (rows < 1 || n_chains < 1 || segment_rows < 0) return fail(TDA_ERR_INVALID, "rows and n_chains must be >= 1, segment_rows >= 0");
  if (qoi && r->nq == 0) return fail(TDA_ERR_INVALID, "this model has no quantity of interest (n_qoi = 0): qoi must be null");
  if (!outputs && !qoi)
    return fail(TDA_ERR_INVALID, "nothing to do: %s", r->nq ? "outputs and qoi are both null" : "outputs is null and the model has no quantity of interest");
  if (!is_device_ptr(params) || (outputs && !is_device_ptr(outputs)) || (qoi && !is_device_ptr(qoi)))
    return fail(TDA_ERR_INVALID, "params, outputs and qoi must be device pointers");
  HIP_TRY(hipSetDevice(r->device));
  hipStream_t st = (hipStream_t)stream;
  long long seg = segment_rows ? (long long)segment_rows : replay_segment_rows(rows, n_chains, r->lds);
  if (seg > rows) seg = rows;
  if (n_evaluated) HIP_TRY(hipMemsetAsync(r->d_count, 0, sizeof(long long), st));
  // one launch holds at most 2^30 workgroups (chains x segments): more go out in several launches of whole segments
  const long long max_groups = 1ll << 30;
  if (n_chains > max_groups) return fail(TDA_ERR_UNSUPPORTED, "more than 2^30 chains in one replay");
  const long long segs_per_launch = max_groups / n_chains, rows_per_launch = segs_per_launch * seg;
  for (long long ra = 0; ra < rows; ra += rows_per_launch) {
    const long long nr = rows - ra < rows_per_launch ? rows - ra : rows_per_launch;
    const size_t off = (size_t)ra * (size_t)n_chains;
    UserReplayArgs a{n_chains, nr, seg, r->d, r->m, r->nq, params + off * r->d, outputs ? outputs + off * r->m : nullptr,
                     qoi ? qoi + off * r->nq : nullptr, n_evaluated ? r->d_count : nullptr};
    const long long groups = n_chains * ((nr + seg - 1) / seg);
    size_t sz = sizeof a;
    void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &sz, HIP_LAUNCH_PARAM_END};
    HIP_TRY(hipModuleLaunchKernel(r->prog.replay, (unsigned)groups, 1, 1, 64, 1, 1, (unsigned)r->prog.out_lds, st, nullptr, cfg));
  }
  if (n_evaluated) {
    long long n = 0;
    HIP_TRY(hipMemcpyAsync(&n, r->d_count, sizeof n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *n_evaluated = (int64_t)n;
  }
  return TDA_OK;
}

void tda_replay_destroy(tda_replay* r) {
  if (!r) return;
  (void)hipSetDevice(r->device);
  (void)hipDeviceSynchronize();
  r->prog.unload();
  if (r->d_count) (void)hipFree(r->d_count);
  delete r;
}

}  // extern "C"
