// The HIP-free part of the optimiser's build (csrc/tda_user_build.h) as a command-line program, built and driven by
// tests/test_optimize.py (plain, and with -fsanitize=address,undefined):
//   options MALA FW GW LS LW PF       "same spec" / "spec without map" / "spec with the other gradient" equalities, then the option list
//   diagnose MALA LS PF M FILE        the error code, a newline, the message for the compiler log in FILE (an optimiser spec)
//   lds MALA FW LS LW M               user_map_dynamic_lds, user_map_ring_lds
//   constants                         TDA_MAP_HISTORY TDA_MAP_HALVINGS TDA_MAP_FLOOR and the six status words
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
  if (cmd == "options" && argc == 8) {
    UserProgramSpec s, t, u;
    s.map = true, s.mala = atoi(argv[2]), s.forward_wave = atoi(argv[3]), s.gradient_wave = atoi(argv[4]);
    s.loglike_source = atoi(argv[5]), s.loglike_wave = atoi(argv[6]), s.prior_form = atoi(argv[7]);
    t = s, u = s;
    t.map = false;
    u.mala = !s.mala;
    std::cout << (s == s) << (s == t) << (s == u);
    for (const char* o : user_program_options(s)) std::cout << " " << o;
    std::cout << "\n";
  } else if (cmd == "diagnose" && argc == 7) {
    UserProgramSpec s;
    s.map = true, s.mala = atoi(argv[2]), s.loglike_source = atoi(argv[3]), s.prior_form = atoi(argv[4]);
    const UserBuildError err = diagnose_user_build(slurp(argv[6]), s, atoi(argv[5]));
    std::cout << err.code << "\n" << err.message;
  } else if (cmd == "lds" && argc == 7) {
    UserProgramSpec s;
    s.map = true, s.mala = atoi(argv[2]), s.forward_wave = atoi(argv[3]), s.loglike_source = atoi(argv[4]), s.loglike_wave = atoi(argv[5]);
    std::cout << user_map_dynamic_lds(s, atoi(argv[6])) << " " << user_map_ring_lds() << "\n";
  } else if (cmd == "constants" && argc == 2) {
    std::cout << TDA_MAP_HISTORY << " " << TDA_MAP_HALVINGS << " " << TDA_MAP_FLOOR << " " << TDA_MAP_CONVERGED_GRADIENT << TDA_MAP_CONVERGED_VALUE << TDA_MAP_MAX_ITER
              << TDA_MAP_LINESEARCH_FAILED << TDA_MAP_INFEASIBLE_START << TDA_MAP_NONFINITE_GRADIENT << "\n";
  } else {
    std::cerr << "usage: options MALA FW GW LS LW PF | diagnose MALA LS PF M FILE | lds MALA FW LS LW M | constants\n";
    return 2;
  }
  return 0;
}
