// User-defined forward models (included by tda_engine.hip): the model is HIP source handed over at run time,
//     __device__ double tda_forward(const double* theta, int dim, int o);     // output o of F(theta)
// or, for a model whose outputs all come from one solve, the wave-cooperative form (one call per evaluation by the 64 lanes)
//     __device__ void tda_forward_wave(const double* theta, int dim, double* out, int n_outputs, double* work, int lane);
// compiled with hiprtc together with the kernels of tda_user_program.hip, so that non-linear models run fused on the device
// instead of through the host protocol (the reference evaluates a Python callable per chain and step, posterior.py:95-96).
// This file is the host side only: compile, load, launch.  The program text (tda_user_program.hip) and the kernel-argument
// structs (tda_user_args.h) are files of their own, embedded below as text; the user's source is the program's header
// "tda_user_source.h".  The MALA kernels are a second program, compiled at init only when the proposal is MALA.
#include <hip/hiprtc.h>

#include <cctype>
#include <cstring>

#include "tda_user_args.h"

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

// one compiled program of a level: the step program (steps, eval, level) or the MALA program (steps, grad0)
struct UserProgram {
  hipModule_t mod = nullptr;
  hipFunction_t steps = nullptr, eval = nullptr, level = nullptr, grad0 = nullptr;
  size_t out_lds = 0;  // dynamic LDS of steps / eval / level: the outputs s_out[m] of a wave-form model (0 without one)
  void unload() {
    if (mod) (void)hipModuleUnload(mod);
    *this = UserProgram{};
  }
};

constexpr size_t USER_LDS_MAX = 64 * 1024;  // (the hardware has 160 KiB: this much needs no opt-in and keeps two chains per CU)

// does `source` use the identifier `name` outside // and /* */ comments, string literals and character literals?
// (DeviceModel in models.py skips the same things for its has_*_wave attributes; what this function says is what is compiled)
bool source_defines(const char* source, const char* name) {
  const size_t n = strlen(name);
  auto ident = [](char ch) { return isalnum((unsigned char)ch) || ch == '_'; };
  for (const char* p = source; *p;) {
    if (p[0] == '/' && p[1] == '/') {
      while (*p && *p != '\n') ++p;
    } else if (p[0] == '/' && p[1] == '*') {
      for (p += 2; *p && !(p[0] == '*' && p[1] == '/'); ++p) {}
      if (*p) p += 2;
    } else if (*p == '"' || *p == '\'') {
      const char quote = *p;
      for (++p; *p && *p != quote; ++p)
        if (*p == '\\' && p[1]) ++p;
      if (*p) ++p;
    } else if (ident(*p)) {
      const char* q = p;
      while (ident(*q)) ++q;
      if ((size_t)(q - p) == n && strncmp(p, name, n) == 0) return true;
      p = q;
    } else {
      ++p;
    }
  }
  return false;
}

// hiprtc for gfx950: tda_user_program.hip with the user's source and the argument structs as its named headers.  A source
// without a function that the selected kernels call resolves to the program's tagged fallback template, which a static_assert
// turns into the messages below (not an unresolved symbol at load); any other failure quotes the (truncated) compiler log.
// forward_wave / gradient_wave: the source defines tda_forward_wave / tda_gradient_wave (source_defines above); a program with
// either holds at most 64 KiB of LDS per workgroup (= per chain), static and dynamic together, for `m` outputs.  Static LDS
// beyond the hardware's 160 KiB does not get as far as a module: the compiler refuses it, and its message becomes the same refusal.
// prior_wave (with prior_source): the source defines the coupled form of the prior, tda_logprior_wave, instead of the term.
int compile_user_program(const char* source, int noise_kind, bool mala, bool prior_source, bool prior_wave, bool forward_wave, bool gradient_wave, int m,
                         UserProgram* out) {
  const char* const headers[] = {source, tda_user_args_text};
  const char* const names[] = {"tda_user_source.h", "tda_user_args.h"};
  hiprtcProgram prog;
  if (hiprtcCreateProgram(&prog, tda_user_program_text, mala ? "tda_user_mala.hip" : "tda_user_model.hip", 2, headers, names) != HIPRTC_SUCCESS)
    return fail(TDA_ERR_HIP, "hiprtcCreateProgram failed");
  std::vector<const char*> opts = {"--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17"};
  if (noise_kind == TDA_NOISE_SOURCE) opts.push_back("-DTDA_LOGLIKE_SOURCE");
  if (mala) opts.push_back("-DTDA_USER_MALA");
  if (prior_source) opts.push_back("-DTDA_PRIOR_SOURCE");  // (with MALA: the source defines tda_logprior_term_grad too)
  if (prior_wave) opts.push_back("-DTDA_PRIOR_WAVE");  // (beside the switch above: tda_logprior_wave, under MALA tda_logprior_grad too)
  if (forward_wave) opts.push_back("-DTDA_FORWARD_WAVE");
  if (gradient_wave) opts.push_back("-DTDA_GRADIENT_WAVE");  // (the MALA program only: the step program calls no gradient)
  if (hiprtcCompileProgram(prog, (int)opts.size(), opts.data()) != HIPRTC_SUCCESS) {
    size_t n = 0;
    (void)hiprtcGetProgramLogSize(prog, &n);
    std::string log(n, '\0');
    if (n) (void)hiprtcGetProgramLog(prog, &log[0]);
    (void)hiprtcDestroyProgram(&prog);
    unsigned long lds_need = 0, lds_limit = 0;
    const size_t at = log.find("local memory (");
    if (at != std::string::npos && sscanf(log.c_str() + at, "local memory (%lu) exceeds limit (%lu)", &lds_need, &lds_limit) == 2)
      return fail(TDA_ERR_UNSUPPORTED, "a source-defined model holds at most 64 KiB of LDS per chain: this source declares %lu bytes (parameters, gradient, "
                                       "TDA_WORKSPACE and its own __shared__ arrays), more than the %lu bytes of the hardware, before the %zu bytes "
                                       "for its %d outputs",
                  lds_need, lds_limit, (size_t)m * sizeof(double), m);
    if (log.find("tda_forward_wave_missing") != std::string::npos)
      return fail(TDA_ERR_INVALID, "the source's tda_forward_wave is not __device__ void tda_forward_wave(const double* theta, int dim, double* out, "
                                   "int n_outputs, double* work, int lane)");
    if (log.find("tda_gradient_wave_missing") != std::string::npos)
      return fail(TDA_ERR_INVALID, "the source's tda_gradient_wave is not __device__ void tda_gradient_wave(const double* theta, int dim, "
                                   "const double* sensitivity, int n_outputs, double* grad, double* work, int lane)");
    if (mala && log.find("tda_gradient_missing") != std::string::npos)
      return fail(TDA_ERR_INVALID, "MALA on a source-defined model: the source defines no __device__ double tda_gradient(const double* theta, "
                                   "int dim, const double* sensitivity, int n_outputs, int j)");
    if (mala && log.find("tda_loglike_term_grad_missing") != std::string::npos)
      return fail(TDA_ERR_INVALID, "MALA with a source-defined likelihood: the source defines no __device__ double tda_loglike_term_grad(double f, "
                                   "double y, double p, int o)");
    if (!mala && log.find("tda_loglike_term_missing") != std::string::npos)
      return fail(TDA_ERR_INVALID, "a source-defined likelihood: the source defines no __device__ double tda_loglike_term(double f, double y, double p, int o)");
    if (log.find("tda_logprior_wave_missing") != std::string::npos)
      return fail(TDA_ERR_INVALID, "a source-defined prior: the source's tda_logprior_wave is not __device__ double tda_logprior_wave(const double* theta, "
                                   "int dim, const double* p, const double* q, int lane)");
    if (mala && log.find("tda_logprior_grad_missing") != std::string::npos)
      return fail(TDA_ERR_INVALID, "a source-defined prior under MALA: the source defines no __device__ double tda_logprior_grad(const double* theta, "
                                   "int dim, const double* p, const double* q, int j)");
    if (mala && log.find("tda_logprior_term_grad_missing") != std::string::npos)
      return fail(TDA_ERR_INVALID, "a source-defined prior under MALA: the source defines no __device__ double tda_logprior_term_grad(double x, double p, "
                                   "double q, int j)");
    if (log.find("tda_logprior_term_missing") != std::string::npos)
      return fail(TDA_ERR_INVALID, "a source-defined prior: the source defines no __device__ double tda_logprior_term(double x, double p, double q, int j)"
                                   " (or, for a prior that couples parameters, tda_logprior_wave(const double* theta, int dim, const double* p, const double* q, int lane))");
    if (log.size() > 400) log.resize(400);
    return fail(TDA_ERR_INVALID, "the forward-model source does not compile%s: %s", mala ? " with the MALA kernels" : "", log.c_str());
  }
  size_t nb = 0;
  (void)hiprtcGetCodeSize(prog, &nb);
  std::vector<char> code(nb);
  (void)hiprtcGetCode(prog, code.data());
  (void)hiprtcDestroyProgram(&prog);
  HIP_TRY(hipModuleLoadData(&out->mod, code.data()));
  HIP_TRY(hipModuleGetFunction(&out->steps, out->mod, mala ? "tda_user_mala_steps" : "tda_user_steps"));
  if (mala) {
    HIP_TRY(hipModuleGetFunction(&out->grad0, out->mod, "tda_user_mala_grad0"));
  } else {
    HIP_TRY(hipModuleGetFunction(&out->eval, out->mod, "tda_user_eval"));
    HIP_TRY(hipModuleGetFunction(&out->level, out->mod, "tda_user_level_action"));
  }
  out->out_lds = forward_wave && !mala ? (size_t)m * sizeof(double) : 0;
  if (forward_wave || gradient_wave) {  // the LDS of a chain: what the kernels declare (s_th, s_grad, the workspace) + outputs / sensitivities
    const size_t dyn = (size_t)m * sizeof(double);
    for (hipFunction_t fn : {out->steps, out->eval, out->level, out->grad0}) {
      int stat = 0;
      if (!fn) continue;
      HIP_TRY(hipFuncGetAttribute(&stat, HIP_FUNC_ATTRIBUTE_SHARED_SIZE_BYTES, fn));
      if ((size_t)stat + dyn > USER_LDS_MAX) {
        out->unload();
        return fail(TDA_ERR_UNSUPPORTED, "a wave-form model holds at most 64 KiB of LDS per chain: this source needs %d bytes (parameters, gradient and "
                                         "TDA_WORKSPACE) + %zu bytes for its %d outputs",
                    stat, dyn, m);
      }
    }
  }
  return TDA_OK;
}

// dynamic LDS of the MALA kernels: the sensitivity of the m outputs (s_sens[m] of tda_user_program.hip)
inline size_t user_mala_lds(const UserMalaArgs& a) { return a.m * sizeof(double); }

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
