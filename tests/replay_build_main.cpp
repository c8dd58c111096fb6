// The HIP-free part of the replay program's build (csrc/tda_user_build.h) as a command-line program, built and driven by
// tests/test_replay.py (and once, by hand or there, with -fsanitize=address,undefined):
//   forms FILE                    the two quantity-of-interest flags of UserForms
//   options FW QOI_FORM           "same spec" / "spec with another qoi_form" / "spec without replay" equalities, then the option list
//   diagnose FW QOI_FORM M FILE   the error code, a newline, the message for the compiler log in FILE (the replay program's spec)
//   signatures                    TDA_SIG_QOI / TDA_SIG_QOI_WAVE, one line each: the function's name, a tab, the text
//   segment ROWS CHAINS LDS       replay_segment_rows, then the number of segments, the rows that the segments cover in all and
//                                 the length of the shortest one
//   lds M NQ                      user_replay_lds
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
  if (cmd == "forms" && argc == 3) {
    const UserForms f = user_forms(slurp(argv[2]).c_str());
    std::cout << f.qoi << f.qoi_wave << " " << f.forward_wave << "\n";
  } else if (cmd == "options" && argc == 4) {
    UserProgramSpec s, t, u;
    s.replay = true, s.forward_wave = atoi(argv[2]), s.qoi_form = atoi(argv[3]);
    t = s, u = s;
    t.qoi_form = (s.qoi_form + 1) % 3;
    u.replay = false;
    std::cout << (s == s) << (s == t) << (s == u);
    for (const char* o : user_program_options(s)) std::cout << " " << o;
    std::cout << "\n";
  } else if (cmd == "diagnose" && argc == 6) {
    UserProgramSpec s;
    s.replay = true, s.forward_wave = atoi(argv[2]), s.qoi_form = atoi(argv[3]);
    const UserBuildError err = diagnose_user_build(slurp(argv[5]), s, atoi(argv[4]));
    std::cout << err.code << "\n" << err.message;
  } else if (cmd == "signatures" && argc == 2) {
    std::cout << "tda_qoi\t" << TDA_SIG_QOI << "\n" << "tda_qoi_wave\t" << TDA_SIG_QOI_WAVE << "\n";
  } else if (cmd == "segment" && argc == 5) {
    const long long rows = atoll(argv[2]), chains = atoll(argv[3]);
    const long long seg = replay_segment_rows(rows, chains, (size_t)atoll(argv[4]));
    long long n = 0, covered = 0, shortest = rows;
    for (long long r0 = 0; seg >= 1 && r0 < rows; r0 += seg) {  // the kernel's own segments: [r0, min(r0 + seg, rows))
      const long long len = (r0 + seg < rows ? r0 + seg : rows) - r0;
      ++n, covered += len, shortest = len < shortest ? len : shortest;
    }
    std::cout << seg << " " << n << " " << covered << " " << shortest << "\n";
  } else if (cmd == "lds" && argc == 4) {
    std::cout << user_replay_lds(atoi(argv[2]), atoi(argv[3])) << "\n";
  } else {
    std::cerr << "usage: forms FILE | options FW QOI_FORM | diagnose FW QOI_FORM M FILE | signatures | segment ROWS CHAINS LDS | lds M NQ\n";
    return 2;
  }
  return 0;
}
