// The HIP-free part of the HMC program's build (csrc/tda_user_build.h) as a command-line program, built and driven by
// tests/test_hmc.py (once as it is and once with -fsanitize=address,undefined):
//   options FW GW LOGLIKE PRIOR_FORM   for the MALA program of these forms and the HMC program of the same forms: "same key" bits
//                                      (mala == mala, mala == hmc, hmc == hmc), then one line each with the option list
//   diagnose HMC FILE                  the error code, a newline, the message for the compiler log in FILE (MALA / HMC program of a plain source)
//   lds LOGLIKE_WAVE M                 user_mala_lds of the MALA and of the HMC program
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
  if (cmd == "options" && argc == 6) {
    UserProgramSpec mala;
    mala.mala = true, mala.forward_wave = atoi(argv[2]), mala.gradient_wave = atoi(argv[3]);
    mala.loglike_source = atoi(argv[4]) > 0, mala.loglike_wave = atoi(argv[4]) == 2, mala.prior_form = atoi(argv[5]);
    UserProgramSpec hmc = mala;
    hmc.hmc = true;
    std::cout << (mala == mala) << (mala == hmc) << (hmc == hmc) << "\n";
    for (const UserProgramSpec* s : {&mala, &hmc}) {
      for (const char* o : user_program_options(*s)) std::cout << o << " ";
      std::cout << "\n";
    }
  } else if (cmd == "diagnose" && argc == 4) {
    UserProgramSpec s;
    s.mala = true, s.hmc = atoi(argv[2]);
    const UserBuildError err = diagnose_user_build(slurp(argv[3]), s, 1);
    std::cout << err.code << "\n" << err.message;
  } else if (cmd == "lds" && argc == 4) {
    UserProgramSpec s;
    s.mala = true, s.loglike_source = s.loglike_wave = atoi(argv[2]);
    UserProgramSpec h = s;
    h.hmc = true;
    std::cout << user_mala_lds(s, atoi(argv[3])) << " " << user_mala_lds(h, atoi(argv[3])) << " " << user_dynamic_lds(h, atoi(argv[3])) << "\n";
  } else {
    std::cerr << "usage: options FW GW LOGLIKE PRIOR_FORM | diagnose HMC FILE | lds LOGLIKE_WAVE M\n";
    return 2;
  }
  return 0;
}
