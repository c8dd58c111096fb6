// What a source-defined ("user") program is built from, without any HIP: which forms of the contract a source defines, the
// key of one build (UserProgramSpec), its hiprtc option list and the reading of a failed compile's log.  tda_usermodel.inc is
// the only user in the library; tests/user_build_main.cpp compiles this header alone with the host compiler.
#pragma once

#include <cctype>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "tda_user_args.h"
#include "tinyda_amd.h"

namespace {

// does `source` use the identifier `name` outside // and /* */ comments, string literals and character literals?
// (_defines in models.py is the same scan: what this function says is what is compiled)
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

// the optional functions of the contract that a level's source defines, found once when the source is set
struct UserForms {
  bool forward_wave = false, gradient_wave = false;    // the wave forms of the model: one call per evaluation by the chain's whole wave
  bool prior_term = false, prior_term_grad = false;    // a separable prior and its derivative (MALA)
  bool prior_wave = false, prior_grad = false;         // a prior that couples parameters and its gradient (MALA)
  bool loglike_term = false, loglike_wave = false, loglike_grad_wave = false;  // a separable likelihood, one that couples outputs, and its gradient (MALA)
  bool qoi = false, qoi_wave = false;                  // a quantity of interest per call, or all of them in one call by the whole wave (the replay program)
  bool both_prior_forms() const { return prior_term && prior_wave; }  // (a prior has one form: tda_engine_set_level_source refuses)
  bool both_loglike_forms() const { return loglike_term && loglike_wave; }  // (and so has a likelihood)
};
UserForms user_forms(const char* source) {
  auto has = [source](const char* name) { return source_defines(source, name); };
  return {has("tda_forward_wave"), has("tda_gradient_wave"), has("tda_logprior_term"), has("tda_logprior_term_grad"), has("tda_logprior_wave"), has("tda_logprior_grad"),
          has("tda_loglike_term"), has("tda_loglike_wave"), has("tda_loglike_grad_wave"), has("tda_qoi"), has("tda_qoi_wave")};
}

// what one program is compiled with: a program built with another spec than the one wanted now is built again
struct UserProgramSpec {
  bool mala = false;            // the MALA program (tda_user_mala_steps, tda_user_mala_grad0), not the step program
  bool loglike_source = false;  // TDA_NOISE_SOURCE: the source's tda_loglike_term (or its tda_loglike_wave: loglike_wave below)
  int prior_form = 0;           // 0 the engine's own Gaussian / uniform code, 1 the source's tda_logprior_term, 2 its tda_logprior_wave
  bool forward_wave = false, gradient_wave = false;  // (gradient_wave: the MALA program only, the step program calls no gradient)
  bool loglike_wave = false;    // (with loglike_source) the source's tda_loglike_wave, not its tda_loglike_term
  bool replay = false;          // the replay program (tda_user_replay), not the step program: of the fields above, forward_wave alone applies
  int qoi_form = 0;             // (with replay) 0 no quantity of interest, 1 the source's tda_qoi, 2 its tda_qoi_wave
  bool map = false;             // the optimiser (tda_user_maximize) in place of the kernels that sample: with `mala` over the source's
                                // gradient (the MALA program's requirements), without it over differences of the step program's objective
  bool hmc = false;             // (with mala) the HMC program: tda_user_hmc_steps in place of tda_user_mala_steps, everything else the MALA program's
  bool nuts = false;            // (with mala) the NUTS program: tda_user_nuts_steps in that place; the checkpoints of its trees are LDS behind the MALA program's
  bool dense_mass = false;      // (with hmc or nuts) the dense inverse mass of include/tinyda_amd_dense_mass.h: the whitened momentum, two
                                // matrix-vector products per leapfrog step, 1 KiB of static LDS more (s_vec)
  bool operator==(const UserProgramSpec& o) const {
    return mala == o.mala && loglike_source == o.loglike_source && prior_form == o.prior_form && forward_wave == o.forward_wave &&
           gradient_wave == o.gradient_wave && loglike_wave == o.loglike_wave && replay == o.replay && qoi_form == o.qoi_form && map == o.map && hmc == o.hmc && nuts == o.nuts &&
           dense_mass == o.dense_mass;
  }
};

// dynamic LDS of the MALA kernels: the sensitivity of the m outputs (s_sens[m] of tda_user_program.hip), and behind it the
// outputs themselves under a likelihood that couples them
inline size_t user_mala_lds(const UserProgramSpec& spec, int m) { return (spec.loglike_source && spec.loglike_wave ? 2 : 1) * (size_t)m * sizeof(double); }
// dynamic LDS of tda_user_nuts_steps behind that: the U-turn checkpoints of a subtree, (momentum, running momentum sum) per row of
// DP doubles, max_depth rows at the most
inline size_t user_nuts_checkpoint_lds(int max_depth, int DP) { return 2 * (size_t)max_depth * (size_t)DP * sizeof(double); }
// static LDS that a dense mass adds to tda_user_hmc_steps / tda_user_nuts_steps: s_vec[128], the operand of its two products
constexpr size_t user_dense_mass_lds() { return 128 * sizeof(double); }
// dynamic LDS of a program's kernels for m outputs: the MALA program's buffer, or the step program's s_out[m] under a wave form of
// the model or of the likelihood (0 without one)
inline size_t user_dynamic_lds(const UserProgramSpec& spec, int m) {
  if (spec.mala) return user_mala_lds(spec, m);
  return spec.forward_wave || (spec.loglike_source && spec.loglike_wave) ? (size_t)m * sizeof(double) : 0;
}

// dynamic LDS of the replay kernel: the outputs s_out[m] (always there: the quantities read them) and behind them s_qoi[n_qoi]
inline size_t user_replay_lds(int m, int n_qoi) { return ((size_t)m + (size_t)n_qoi) * sizeof(double); }

// LDS of the optimiser, per start.  Dynamic: what the program it stands in for holds for the same source (user_dynamic_lds: the
// MALA program's sensitivities over the source's gradient, the step program's outputs otherwise).  Static, beside what the
// source's forms declare (parameters, s_grad, TDA_WORKSPACE): the ring of TDA_MAP_HISTORY pairs of 128 doubles, their 1 / s^T y, and
// the point and its gradient (128 doubles each) and four scalars carried between iterations
inline size_t user_map_dynamic_lds(const UserProgramSpec& spec, int m) { return user_dynamic_lds(spec, m); }
constexpr size_t user_map_ring_lds() { return (2 * (size_t)TDA_MAP_HISTORY * 128 + TDA_MAP_HISTORY + 2 * 128 + 4) * sizeof(double); }

// How many rows of a chain one wave of the replay walks.  A long segment evaluates the model once per accepted state (a row that
// repeats its predecessor is copied forward, but a segment's first row is always evaluated); a short one gives the device more
// workgroups.  The longest segment that still leaves REPLAY_ROUNDS rounds of resident workgroups: residency is what the LDS of a
// workgroup (`lds_bytes`, static and dynamic) leaves of a CU's 160 KiB, capped by its 32 wave slots (one wave per workgroup), on
// the 256 CUs of gfx950.  Always in [1, rows]; ceil(rows / result) segments cover every row once and none is empty.
// REPLAY_ROUNDS = 12 is read from the sweep of tools/replay_rate.py on an MI355X (profiles/replay_rate.json, 4096 chains x 2001
// rows of an AdaptiveMetropolis run).  Measured time of one replay against the best segment length of the sweep: the ring
// (d = 4, m = 16, 6 workgroups per CU) +12 % at 2.7 rounds (one segment per chain), +1 % at 11, best at 21, +0.5 % at 85, +17 %
// at 680; the d = 64, m = 1024 model (17 per CU) +24 % at one round, +7 % at 7.5, best at 30 .. 59, +3 % at 240.  Workgroups of
// one launch differ in length (a chain that accepts often evaluates more) and the short ones fill in behind the long ones, so
// a few rounds are not enough; every further segment costs one evaluation (0.7058 evaluations per row at one segment per
// chain, 0.7148 at 63), which weighs more the dearer the model.  12 rounds is the long-segment end of the flat part: +1 % and
// +4 % on the two cases.  One row per segment (every row evaluated) takes 5.1 and 1.4 times the best.
constexpr long long REPLAY_CUS = 256, REPLAY_LDS_PER_CU = 160 * 1024, REPLAY_WAVES_PER_CU = 32, REPLAY_ROUNDS = 12;
inline long long replay_segment_rows(long long rows, long long n_chains, size_t lds_bytes) {
  if (rows < 1 || n_chains < 1) return 1;
  long long per_cu = lds_bytes ? REPLAY_LDS_PER_CU / (long long)lds_bytes : REPLAY_WAVES_PER_CU;
  per_cu = per_cu < 1 ? 1 : per_cu > REPLAY_WAVES_PER_CU ? REPLAY_WAVES_PER_CU : per_cu;
  const long long want = REPLAY_ROUNDS * REPLAY_CUS * per_cu;      // workgroups wanted
  const long long segments = (want + n_chains - 1) / n_chains;     // ... per chain
  const long long seg = rows / (segments < 1 ? 1 : segments);
  return seg < 1 ? 1 : seg > rows ? rows : seg;
}

std::vector<const char*> user_program_options(const UserProgramSpec& s) {
  std::vector<const char*> opts = {"--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17"};
  if (s.replay) {  // a program of its own: no likelihood, no prior, no gradient
    opts.push_back("-DTDA_USER_REPLAY");
    if (s.forward_wave) opts.push_back("-DTDA_FORWARD_WAVE");
    if (s.qoi_form) opts.push_back(s.qoi_form == 2 ? "-DTDA_QOI_WAVE" : "-DTDA_QOI");
    return opts;
  }
  if (s.loglike_source) opts.push_back("-DTDA_LOGLIKE_SOURCE");
  if (s.loglike_source && s.loglike_wave) opts.push_back("-DTDA_LOGLIKE_WAVE");  // (under MALA: tda_loglike_grad_wave too)
  if (s.mala) opts.push_back("-DTDA_USER_MALA");
  if (s.mala && s.hmc) opts.push_back("-DTDA_USER_HMC");
  if (s.mala && s.nuts) opts.push_back("-DTDA_USER_NUTS");
  if (s.mala && (s.hmc || s.nuts) && s.dense_mass) opts.push_back("-DTDA_DENSE_MASS");
  if (s.map) opts.push_back("-DTDA_USER_MAP");
  if (s.prior_form) opts.push_back("-DTDA_PRIOR_SOURCE");  // (with MALA: the source defines the prior's gradient too)
  if (s.prior_form == 2) opts.push_back("-DTDA_PRIOR_WAVE");
  if (s.forward_wave) opts.push_back("-DTDA_FORWARD_WAVE");
  if (s.gradient_wave) opts.push_back("-DTDA_GRADIENT_WAVE");
  return opts;
}

// A failed compile.  A source without a function that the selected kernels call resolves to the program's tagged fallback
// template, which a static_assert turns into a log that holds the tag: the first row below whose tag the log holds (and that
// applies to the program) is the refusal.  Static LDS beyond the hardware's 160 KiB does not get as far as a module either: the
// compiler's message becomes the LDS refusal.  Any other failure quotes the (truncated) compiler log.
struct UserBuildError {
  int code;
  std::string message;
};
enum { USER_MALA = 1, USER_STEPS = 2, USER_BOTH = 3, USER_REPLAY = 4 };
const struct UserMissingRow {
  const char* tag;
  int applies, code;
  const char* message;
} USER_MISSING[] = {
    {"tda_forward_wave_missing", USER_BOTH | USER_REPLAY, TDA_ERR_INVALID, "the source's tda_forward_wave is not " TDA_SIG_FORWARD_WAVE},
    {"tda_gradient_wave_missing", USER_BOTH, TDA_ERR_INVALID, "the source's tda_gradient_wave is not " TDA_SIG_GRADIENT_WAVE},
    {"tda_gradient_missing", USER_MALA, TDA_ERR_INVALID, "MALA on a source-defined model: the source defines no " TDA_SIG_GRADIENT},
    {"tda_loglike_wave_missing", USER_BOTH, TDA_ERR_INVALID, "a source-defined likelihood: the source's tda_loglike_wave is not " TDA_SIG_LOGLIKE_WAVE},
    {"tda_loglike_grad_wave_missing", USER_MALA, TDA_ERR_INVALID,
     "MALA with a source-defined likelihood that couples outputs: the source defines no " TDA_SIG_LOGLIKE_GRAD_WAVE},
    {"tda_loglike_term_grad_missing", USER_MALA, TDA_ERR_INVALID, "MALA with a source-defined likelihood: the source defines no " TDA_SIG_LOGLIKE_TERM_GRAD},
    {"tda_loglike_term_missing", USER_STEPS, TDA_ERR_INVALID, "a source-defined likelihood: the source defines no " TDA_SIG_LOGLIKE_TERM},
    {"tda_logprior_wave_missing", USER_BOTH, TDA_ERR_INVALID, "a source-defined prior: the source's tda_logprior_wave is not " TDA_SIG_LOGPRIOR_WAVE},
    {"tda_logprior_grad_missing", USER_MALA, TDA_ERR_INVALID, "a source-defined prior under MALA: the source defines no " TDA_SIG_LOGPRIOR_GRAD},
    {"tda_logprior_term_grad_missing", USER_MALA, TDA_ERR_INVALID, "a source-defined prior under MALA: the source defines no " TDA_SIG_LOGPRIOR_TERM_GRAD},
    {"tda_logprior_term_missing", USER_BOTH, TDA_ERR_INVALID,
     "a source-defined prior: the source defines no " TDA_SIG_LOGPRIOR_TERM " (or, for a prior that couples parameters, " TDA_CALL_LOGPRIOR_WAVE ")"},
    {"tda_qoi_wave_missing", USER_REPLAY, TDA_ERR_INVALID, "a quantity of interest: the source's tda_qoi_wave is not " TDA_SIG_QOI_WAVE},
    {"tda_qoi_missing", USER_REPLAY, TDA_ERR_INVALID, "a quantity of interest: the source's tda_qoi is not " TDA_SIG_QOI},
};
UserBuildError diagnose_user_build(std::string log, const UserProgramSpec& spec, int m) {
  char buf[512];  // (the length of the engine's error text)
  unsigned long lds_need = 0, lds_limit = 0;
  const size_t at = log.find("local memory (");
  if (at != std::string::npos && sscanf(log.c_str() + at, "local memory (%lu) exceeds limit (%lu)", &lds_need, &lds_limit) == 2) {
    snprintf(buf, sizeof buf,
             "a source-defined model holds at most 64 KiB of LDS per chain: this source declares %lu bytes (parameters, gradient, "
             "TDA_WORKSPACE and its own __shared__ arrays), more than the %lu bytes of the hardware, before the %zu bytes "
             "for its %d outputs%s",
             lds_need, lds_limit, spec.mala ? user_mala_lds(spec, m) : (size_t)m * sizeof(double), m,
             spec.mala && spec.loglike_source && spec.loglike_wave ? " and their sensitivities" : "");
    return {TDA_ERR_UNSUPPORTED, buf};
  }
  for (const UserMissingRow& row : USER_MISSING)
    if ((row.applies & (spec.replay ? USER_REPLAY : spec.mala ? USER_MALA : USER_STEPS)) && log.find(row.tag) != std::string::npos)
      return {row.code, std::string(spec.map && spec.mala ? "the optimiser over the source's gradient needs what MALA needs -- " : spec.mala && spec.nuts ? "NUTS needs what MALA needs -- " : spec.mala && spec.hmc ? "HMC needs what MALA needs -- " : "") + row.message};
  if (log.size() > 400) log.resize(400);
  snprintf(buf, sizeof buf, "the forward-model source does not compile%s: %s",
           spec.replay ? " with the replay kernel" : spec.map ? (spec.mala ? " with the optimiser over its gradient" : " with the optimiser") : spec.mala && spec.nuts ? " with the NUTS kernels" : spec.mala && spec.hmc ? " with the HMC kernels" : spec.mala ? " with the MALA kernels" : "",
           log.c_str());
  return {TDA_ERR_INVALID, buf};
}

}  // namespace
