// The HIP-free part of a dense-mass program's build (csrc/tda_user_build.h) as a command-line program, built and driven by
// tests/test_dense_mass.py (once as it is and once with -fsanitize=address,undefined):
//   options KIND   KIND = hmc | nuts | mala: the program of that kind without and with the dense_mass flag: "same key" bits
//                  (plain == plain, plain == dense, dense == dense), then one line each with the option list
//   lds            user_dense_mass_lds()
#include <iostream>
#include <string>

#include "tda_user_build.h"

int main(int argc, char** argv) {
  const std::string cmd = argc > 1 ? argv[1] : "";
  if (cmd == "options" && argc == 3) {
    const std::string kind = argv[2];
    UserProgramSpec plain;
    plain.mala = true, plain.hmc = kind == "hmc", plain.nuts = kind == "nuts";
    UserProgramSpec dense = plain;
    dense.dense_mass = true;
    std::cout << (plain == plain) << (plain == dense) << (dense == dense) << "\n";
    for (const UserProgramSpec* s : {&plain, &dense}) {
      for (const char* o : user_program_options(*s)) std::cout << o << " ";
      std::cout << "\n";
    }
  } else if (cmd == "lds" && argc == 2) {
    std::cout << user_dense_mass_lds() << "\n";
  } else {
    std::cerr << "usage: options hmc|nuts|mala | lds\n";
    return 2;
  }
  return 0;
}
