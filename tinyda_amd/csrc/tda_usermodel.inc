// User-defined forward models (included by tda_engine.hip): the model is HIP source handed over at run time,
//     __device__ double tda_forward(const double* theta, int dim, int o);     // output o of F(theta)
// or, for a model whose outputs all come from one solve, the wave-cooperative form tda_forward_wave (one call per evaluation by the 64 lanes),
// compiled with hiprtc together with the kernels of tda_user_program.hip, so that non-linear models run fused on the device
// instead of through the host protocol (the reference evaluates a Python callable per chain and step, posterior.py:95-96).
// This file is the host side only: compile, load, launch.  The program text (tda_user_program.hip) and the kernel-argument
// structs (tda_user_args.h) are files of their own, embedded below as text; the user's source is the program's header
// "tda_user_source.h".  The MALA kernels are a second program, compiled at init only when the proposal is MALA; under HMC the
// HMC program (tda_user_hmc_steps beside tda_user_mala_grad0, the `hmc` flag of the build description) stands in its place, and under NUTS the
// NUTS program (tda_user_nuts_steps, the `nuts` flag).  What a build
// is made from without any HIP (the forms a source defines, the build key, the options, the reading of a failed compile) is
// tda_user_build.h.
#include <hip/hiprtc.h>

#include "tda_user_build.h"

// (.incbin looks the two files up on the include path: a host build of this file needs -I<this directory>)
#if !defined(__HIP_DEVICE_COMPILE__)
__asm__(
    ".pushsection .rodata\n"
    "tda_user_program_text:\n.incbin \"tda_user_program.hip\"\n.byte 0\n"
    "tda_user_args_text:\n.incbin \"tda_user_args.h\"\n.byte 0\n"
    ".popsection\n");
#endif
extern "C" const char tda_user_program_text[] __attribute__((visibility("hidden")));
extern "C" const char tda_user_args_text[] __attribute__((visibility("hidden")));

namespace {

// one compiled program of a level: the step program (steps, eval, level) or the MALA program (steps, grad0); or, of no level
// and no engine, the replay program (replay: tda_host_replay.inc) or the optimiser (maximize: tda_host_optimize.inc)
struct UserProgram {
  hipModule_t mod = nullptr;
  hipFunction_t steps = nullptr, eval = nullptr, level = nullptr, grad0 = nullptr, replay = nullptr, maximize = nullptr;
  size_t out_lds = 0;    // dynamic LDS of steps / eval / level: the outputs s_out[m] of a wave-form model or likelihood (0 without one;
                         // tda_user_eval reads it under a wave-form model only and is launched with it all the same: one size per program)
  UserProgramSpec spec;  // what it was compiled with (ensure_user_program of tda_engine.hip builds it again when that changed since)
  void unload() {
    if (mod) (void)hipModuleUnload(mod);
    *this = UserProgram{};
  }
};

constexpr size_t USER_LDS_MAX = 64 * 1024;  // (the hardware has 160 KiB: this much needs no opt-in and keeps two chains per CU)

// hiprtc for gfx950: tda_user_program.hip with the user's source and the argument structs as its named headers, under the
// options of `spec`; a failed compile is read by diagnose_user_build.  A program with a wave form of the model or of the
// likelihood holds at most 64 KiB of LDS per workgroup (= per chain), static and dynamic together, for `m` outputs (the MALA
// program of a likelihood that couples outputs: 2 m doubles, user_mala_lds).  The replay program holds its m outputs and its
// n_qoi quantities in every form, under the same rule.
int compile_user_program(const char* source, const UserProgramSpec& spec, int m, UserProgram* out, int n_qoi = 0) {
  const bool mala = spec.mala;
  const char* const headers[] = {source, tda_user_args_text};
  const char* const names[] = {"tda_user_source.h", "tda_user_args.h"};
  hiprtcProgram prog;
  if (hiprtcCreateProgram(&prog, tda_user_program_text, spec.replay ? "tda_user_replay.hip" : spec.map ? "tda_user_map.hip" : mala ? "tda_user_mala.hip" : "tda_user_model.hip", 2, headers, names) != HIPRTC_SUCCESS)
    return fail(TDA_ERR_HIP, "hiprtcCreateProgram failed");
  std::vector<const char*> opts = user_program_options(spec);
  if (hiprtcCompileProgram(prog, (int)opts.size(), opts.data()) != HIPRTC_SUCCESS) {
    size_t n = 0;
    (void)hiprtcGetProgramLogSize(prog, &n);
    std::string log(n, '\0');
    if (n) (void)hiprtcGetProgramLog(prog, &log[0]);
    (void)hiprtcDestroyProgram(&prog);
    const UserBuildError err = diagnose_user_build(log, spec, m);
    return fail(err.code, "%s", err.message.c_str());
  }
  size_t nb = 0;
  (void)hiprtcGetCodeSize(prog, &nb);
  std::vector<char> code(nb);
  (void)hiprtcGetCode(prog, code.data());
  (void)hiprtcDestroyProgram(&prog);
  HIP_TRY(hipModuleLoadData(&out->mod, code.data()));
  if (spec.replay) {
    HIP_TRY(hipModuleGetFunction(&out->replay, out->mod, "tda_user_replay"));
    out->spec = spec;
    out->out_lds = user_replay_lds(m, n_qoi);
    int stat = 0;
    HIP_TRY(hipFuncGetAttribute(&stat, HIP_FUNC_ATTRIBUTE_SHARED_SIZE_BYTES, out->replay));
    if ((size_t)stat + out->out_lds > USER_LDS_MAX) {
      const size_t dyn = out->out_lds;
      out->unload();
      return fail(TDA_ERR_UNSUPPORTED, "the replay of a source-defined model holds at most 64 KiB of LDS per chain: this source needs %d bytes (parameters and "
                                       "TDA_WORKSPACE) + %zu bytes for its %d outputs and its %d quantities of interest (%zu of them for the quantities)",
                  stat, dyn, m, n_qoi, (size_t)n_qoi * sizeof(double));
    }
    return TDA_OK;
  }
  if (spec.map) {  // the optimiser: the LDS of the program it stands in for, and the ring of pairs in its static part
    HIP_TRY(hipModuleGetFunction(&out->maximize, out->mod, "tda_user_maximize"));
    out->spec = spec;
    out->out_lds = user_map_dynamic_lds(spec, m);
    int stat = 0;
    HIP_TRY(hipFuncGetAttribute(&stat, HIP_FUNC_ATTRIBUTE_SHARED_SIZE_BYTES, out->maximize));
    if ((size_t)stat + out->out_lds > USER_LDS_MAX) {
      const size_t dyn = out->out_lds;
      out->unload();
      return fail(TDA_ERR_UNSUPPORTED, "the optimiser of a source-defined model holds at most 64 KiB of LDS per start: this source needs %d bytes (parameters, "
                                       "gradient, TDA_WORKSPACE and %zu bytes for the ring of %d L-BFGS pairs, the point, its gradient and four scalars) + %zu bytes for its %d outputs",
                  stat, user_map_ring_lds(), (int)TDA_MAP_HISTORY, dyn, m);
    }
    return TDA_OK;
  }
  HIP_TRY(hipModuleGetFunction(&out->steps, out->mod, mala ? (spec.nuts ? "tda_user_nuts_steps" : spec.hmc ? "tda_user_hmc_steps" : "tda_user_mala_steps") : "tda_user_steps"));
  if (mala) {
    HIP_TRY(hipModuleGetFunction(&out->grad0, out->mod, "tda_user_mala_grad0"));
  } else {
    HIP_TRY(hipModuleGetFunction(&out->eval, out->mod, "tda_user_eval"));
    HIP_TRY(hipModuleGetFunction(&out->level, out->mod, "tda_user_level_action"));
  }
  out->spec = spec;
  const bool loglike_wave = spec.loglike_source && spec.loglike_wave;
  out->out_lds = mala ? 0 : user_dynamic_lds(spec, m);
  if (spec.forward_wave || spec.gradient_wave || loglike_wave) {  // the LDS of a chain: what the kernels declare (s_th, s_grad, the workspace) + outputs / sensitivities
    const size_t dyn = user_dynamic_lds(spec, m);
    for (hipFunction_t fn : {out->steps, out->eval, out->level, out->grad0}) {
      int stat = 0;
      if (!fn) continue;
      HIP_TRY(hipFuncGetAttribute(&stat, HIP_FUNC_ATTRIBUTE_SHARED_SIZE_BYTES, fn));
      if ((size_t)stat + dyn > USER_LDS_MAX) {
        out->unload();
        if (loglike_wave)
          return fail(TDA_ERR_UNSUPPORTED, "a likelihood that couples outputs holds at most 64 KiB of LDS per chain: this source needs %d bytes (parameters, "
                                           "gradient and TDA_WORKSPACE) + %zu bytes for its %d outputs%s",
                      stat, dyn, m, mala ? " and their sensitivities" : "");
        if (spec.dense_mass)  // (s_vec is part of `stat`, and may be what no longer fits)
          return fail(TDA_ERR_UNSUPPORTED, "a wave-form model under a dense mass needs more than 64 KiB of LDS per chain: this source needs %d bytes (parameters, gradient, "
                                           "TDA_WORKSPACE and %zu bytes for the operand of the dense mass's products) + %zu bytes for its %d outputs",
                      stat, user_dense_mass_lds(), dyn, m);
        return fail(TDA_ERR_UNSUPPORTED, "a wave-form model holds at most 64 KiB of LDS per chain: this source needs %d bytes (parameters, gradient and "
                                         "TDA_WORKSPACE) + %zu bytes for its %d outputs",
                    stat, dyn, m);
      }
    }
  }
  return TDA_OK;
}

// one wave per chain; `lds` bytes of dynamic LDS
template <class Args>
int launch_user(hipFunction_t fn, Args& a, size_t lds, hipStream_t st) {
  size_t sz = sizeof(Args);
  void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &sz, HIP_LAUNCH_PARAM_END};
  HIP_TRY(hipModuleLaunchKernel(fn, (unsigned)a.N, 1, 1, 64, 1, 1, (unsigned)lds, st, nullptr, cfg));
  return TDA_OK;
}

int launch_user_eval(hipFunction_t fn, long long N, int d, int m, const double* prop, double* F, size_t lds, hipStream_t st) {
  struct { long long N; int d, m; const double* prop; double* F; } a{N, d, m, prop, F};
  size_t sz = sizeof(a);
  void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &sz, HIP_LAUNCH_PARAM_END};
  HIP_TRY(hipModuleLaunchKernel(fn, (unsigned)N, 1, 1, 64, 1, 1, (unsigned)lds, st, nullptr, cfg));
  return TDA_OK;
}

}  // namespace
