// The device branch of the engine's variate map (tinyda_amd/csrc/tda_philox.h: tda_log_unit, tda_sincos_turn and the lines of
// normal_pair under __HIP_DEVICE_COMPILE__), compiled for the host so that tests/test_variate_map.py can hold it to an exact
// reference without a GPU.  Nothing of the map is restated here: the header is included as it is, and the few device intrinsics it
// uses are given host definitions first.  Build with -ffp-contract=off (the engine's flag: the map's error bounds count roundings).
//
//   variate_math_main map     < (u1, u2) doubles      > (ln(1 - u1), sin, cos, z0, z1) doubles per pair
//   variate_math_main stream  < (seed, chain, step, stream, block) uint64   > (z0, z1) doubles per counter, through normal_pair itself
//
// The result is the device's up to rare last-bit differences, not bit for bit: __builtin_amdgcn_rcp is a 24-bit seed here (the
// two Newton steps on it converge from any seed of that quality), frexp_mant / frexp_exp are std::frexp.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#define __HIP_DEVICE_COMPILE__ 1
#define __forceinline__ inline
static inline uint32_t __umulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32); }
static inline double shim_frexp_mant(double x) {
  int k;
  return std::frexp(x, &k);
}
static inline int shim_frexp_exp(double x) {
  int k;
  (void)std::frexp(x, &k);
  return k;
}
#define __builtin_amdgcn_frexp_mant(x) shim_frexp_mant(x)
#define __builtin_amdgcn_frexp_exp(x) shim_frexp_exp(x)
#define __builtin_amdgcn_rcp(x) ((double)(float)(1.0 / (x)))
using std::fma;
using std::sqrt;

#include "tda_philox.h"

// the two lines of normal_pair's device branch, at given uniforms (normal_pair itself draws them from the counter: mode `stream`)
static void normal_pair_at(double u1, double u2, double& z0, double& z1) {
  const double rad = sqrt(-2.0 * tda::tda_log_unit(1.0 - u1));
  double s, c;
  tda::tda_sincos_turn(u2, s, c);
  z0 = rad * c;
  z1 = rad * s;
}

template <typename T>
static std::vector<T> read_all() {
  std::vector<T> v;
  T buf[4096];
  size_t n;
  while ((n = std::fread(buf, sizeof(T), 4096, stdin)) > 0) v.insert(v.end(), buf, buf + n);
  return v;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: variate_math_main map|stream\n");
    return 2;
  }
  std::vector<double> out;
  if (!std::strcmp(argv[1], "map")) {
    const std::vector<double> in = read_all<double>();
    if (in.size() % 2) return 3;
    out.resize(in.size() / 2 * 5);
    for (size_t i = 0; i < in.size() / 2; ++i) {
      const double u1 = in[2 * i], u2 = in[2 * i + 1];
      double* o = &out[5 * i];
      o[0] = tda::tda_log_unit(1.0 - u1);
      tda::tda_sincos_turn(u2, o[1], o[2]);
      normal_pair_at(u1, u2, o[3], o[4]);
    }
  } else if (!std::strcmp(argv[1], "stream")) {
    const std::vector<uint64_t> in = read_all<uint64_t>();
    if (in.size() % 5) return 3;
    out.resize(in.size() / 5 * 2);
    for (size_t i = 0; i < in.size() / 5; ++i) {
      const uint64_t* c = &in[5 * i];
      tda::normal_pair(c[0], (uint32_t)c[1], (uint32_t)c[2], (uint32_t)c[3], (uint32_t)c[4], out[2 * i], out[2 * i + 1]);
    }
  } else {
    return 2;
  }
  return std::fwrite(out.data(), sizeof(double), out.size(), stdout) == out.size() ? 0 : 4;
}
