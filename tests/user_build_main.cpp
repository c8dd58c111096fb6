// The HIP-free part of the source-defined programs' build (csrc/tda_user_build.h) as a command-line program, built and driven by
// tests/test_user_build.py:
//   scan NAME FILE                         1 / 0: does the source in FILE define NAME (source_defines)
//   forms FILE                             the six UserForms flags and the "both forms" decision
//   options                                every spec, one line each: its five fields, a colon, its option list
//   diagnose MALA LOGLIKE PRIOR FW GW M FILE   the error code, a newline, the message for the compiler log in FILE
//   signatures                             the contract's signatures (TDA_SIG_* in csrc/tda_user_args.h), one line each: the function's name, a tab, the text
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>

#include "tda_user_build.h"

static std::string slurp(const char* path) {
  std::ifstream in(path, std::ios::binary);
  std::stringstream ss;
  ss << in.rdbuf();
  return ss.str();
}

int main(int argc, char** argv) {
  const std::string cmd = argc > 1 ? argv[1] : "";
  if (cmd == "scan" && argc == 4) {
    std::cout << (source_defines(slurp(argv[3]).c_str(), argv[2]) ? 1 : 0) << "\n";
  } else if (cmd == "forms" && argc == 3) {
    const UserForms f = user_forms(slurp(argv[2]).c_str());
    std::cout << f.forward_wave << f.gradient_wave << f.prior_term << f.prior_term_grad << f.prior_wave << f.prior_grad << " " << f.both_prior_forms() << "\n";
  } else if (cmd == "options" && argc == 2) {
    for (int i = 0; i < 48; ++i) {
      UserProgramSpec s;
      s.mala = i & 1, s.loglike_source = i & 2, s.forward_wave = i & 4, s.gradient_wave = i & 8, s.prior_form = i / 16;
      std::cout << s.mala << s.loglike_source << s.prior_form << s.forward_wave << s.gradient_wave << ":";
      for (const char* o : user_program_options(s)) std::cout << " " << o;
      std::cout << "\n";
    }
  } else if (cmd == "diagnose" && argc == 9) {
    UserProgramSpec s;
    s.mala = atoi(argv[2]), s.loglike_source = atoi(argv[3]), s.prior_form = atoi(argv[4]), s.forward_wave = atoi(argv[5]), s.gradient_wave = atoi(argv[6]);
    const UserBuildError err = diagnose_user_build(slurp(argv[8]), s, atoi(argv[7]));
    std::cout << err.code << "\n" << err.message;
  } else if (cmd == "signatures" && argc == 2) {
    const char* const sigs[][2] = {
        {"tda_forward_wave", TDA_SIG_FORWARD_WAVE},   {"tda_gradient_wave", TDA_SIG_GRADIENT_WAVE},
        {"tda_gradient", TDA_SIG_GRADIENT},           {"tda_loglike_term", TDA_SIG_LOGLIKE_TERM},
        {"tda_loglike_term_grad", TDA_SIG_LOGLIKE_TERM_GRAD}, {"tda_loglike_wave", TDA_SIG_LOGLIKE_WAVE},
        {"tda_loglike_grad_wave", TDA_SIG_LOGLIKE_GRAD_WAVE}, {"tda_logprior_term", TDA_SIG_LOGPRIOR_TERM},
        {"tda_logprior_term_grad", TDA_SIG_LOGPRIOR_TERM_GRAD}, {"tda_logprior_wave", TDA_SIG_LOGPRIOR_WAVE},
        {"tda_logprior_grad", TDA_SIG_LOGPRIOR_GRAD}};
    for (const auto& sig : sigs) std::cout << sig[0] << "\t" << sig[1] << "\n";
  } else {
    std::cerr << "usage: scan NAME FILE | forms FILE | options | signatures | diagnose MALA LOGLIKE PRIOR FW GW M FILE\n";
    return 2;
  }
  return 0;
}
