// The HIP-free part of the source-defined programs' build (csrc/tda_user_build.h) as a command-line program, built and driven by
// tests/test_user_build.py:
//   scan NAME FILE                         1 / 0: does the source in FILE define NAME (source_defines)
//   forms FILE                             the six UserForms flags and the "both forms" decision
//   options                                every spec, one line each: its five fields, a colon, its option list
//   diagnose MALA LOGLIKE PRIOR FW GW M FILE   the error code, a newline, the message for the compiler log in FILE
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
  } else {
    std::cerr << "usage: scan NAME FILE | forms FILE | options | diagnose MALA LOGLIKE PRIOR FW GW M FILE\n";
    return 2;
  }
  return 0;
}
