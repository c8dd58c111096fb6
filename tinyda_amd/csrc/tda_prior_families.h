// Term library of the scipy.stats families that tinyda_amd.JointPrior lowers as a source-defined prior (TDA_PRIOR_SOURCE):
// appended to the HIP source of every level behind a generated prologue (likelihoods.py, _family_prologue) that holds one table
// row per parameter,
//     #define TDA_PRIOR_DIM <dim>
//     static __device__ const int tda_prior_family[TDA_PRIOR_DIM];     // the ids below
//     static __device__ const double tda_prior_a[TDA_PRIOR_DIM];       // first shape parameter (0 when the family has none)
//     static __device__ const double tda_prior_b[TDA_PRIOR_DIM];       // second shape parameter
//     static __device__ const double tda_prior_c[TDA_PRIOR_DIM];       // normalising constant - log(scale), computed on the host
// With z = (x - loc) / scale (p = loc, q = scale) every log-density is g(z) + c; outside the family's support it is -inf, which
// rejects the proposal.  The lanes of a wave own different parameters, so they diverge over the FAMILIES present, not over the
// parameters: the logarithms that several families share are taken once, ahead of the switch.
//   id family        g(z)                                  support
//    0 norm          -z^2 / 2
//    1 uniform       0                                     0 <= z <= 1
//    2 lognorm(s)    -log z - (log z / s)^2 / 2            z > 0
//    3 gamma(a)      (a - 1) log z - z                     z > 0
//    4 invgamma(a)   -(a + 1) log z - 1 / z                z > 0
//    5 beta(a, b)    (a - 1) log z + (b - 1) log1p(-z)     0 < z < 1
//    6 expon         -z                                    z >= 0
//    7 halfnorm      -z^2 / 2                              z >= 0
//    8 laplace       -|z|
//    9 cauchy        -log1p(z^2)
//   10 t(nu)         -(nu + 1) / 2 log1p(z^2 / nu)
//   11 truncnorm(a, b)  -z^2 / 2                           a <= z <= b
//   12 weibull_min(c)   (c - 1) log z - exp(c log z)       z > 0
// The supports are the table's, open at z = 0 (and z = 1) for gamma, invgamma, beta and weibull_min whatever the shape.  scipy
// gives a finite value at such an edge when the shape parameter there is exactly 1 (gamma(1).logpdf(0) = 0, beta(1, b).logpdf(0)
// = log b, weibull_min(1).logpdf(0) = 0), where this library gives -inf: the sets of -inf points agree with scipy's for every
// other shape, and for shape 1 everywhere but at that one point, which no proposal hits with positive probability.
__device__ double tda_logprior_term(double x, double p, double q, int j) {
  const int f = tda_prior_family[j];
  const double a = tda_prior_a[j], b = tda_prior_b[j];
  const double z = (x - p) / q;
  const double none = -__builtin_inf();
  // families 2, 3, 4, 5, 12 take log z (tested z > 0 below, so a NaN of log never reaches the sum); 5, 9, 10 take one log1p
  const double lz = ((0x103c >> f) & 1) ? log(z) : 0.0;
  const double l1 = ((0x0620 >> f) & 1) ? log1p(f == 5 ? -z : (f == 10 ? z * z / a : z * z)) : 0.0;
  double g;
  switch (f) {
    case 0: g = -0.5 * z * z; break;
    case 1: g = (z >= 0.0 && z <= 1.0) ? 0.0 : none; break;
    case 2: g = z > 0.0 ? -lz - 0.5 * (lz / a) * (lz / a) : none; break;
    case 3: g = z > 0.0 ? (a - 1.0) * lz - z : none; break;
    case 4: g = z > 0.0 ? -(a + 1.0) * lz - 1.0 / z : none; break;
    case 5: g = (z > 0.0 && z < 1.0) ? (a - 1.0) * lz + (b - 1.0) * l1 : none; break;
    case 6: g = z >= 0.0 ? -z : none; break;
    case 7: g = z >= 0.0 ? -0.5 * z * z : none; break;
    case 8: g = -fabs(z); break;
    case 9: g = -l1; break;
    case 10: g = -0.5 * (a + 1.0) * l1; break;
    case 11: g = (z >= a && z <= b) ? -0.5 * z * z : none; break;
    case 12: g = z > 0.0 ? (a - 1.0) * lz - exp(a * lz) : none; break;  // (z^c from the logarithm already taken: pow would take it again)
    default: g = __builtin_nan(""); break;  // (an id the prologue never writes)
  }
  return g + tda_prior_c[j];
}
// d term / d x = g'(z) / q, which the MALA program needs (tda_user_program.hip, TDA_USER_MALA with TDA_PRIOR_SOURCE); the step
// programs never call it.  Inside the support only: outside, the term above is -inf and rejects the proposal, and what this
// function returns there (a NaN of log, a division by zero, a finite number) is never used.
//   id family        g'(z)
//    0 norm, 7 halfnorm, 11 truncnorm    -z
//    1 uniform       0
//    2 lognorm(s)    (-1 - log z / s^2) / z
//    3 gamma(a)      (a - 1) / z - 1
//    4 invgamma(a)   -(a + 1) / z + 1 / z^2               (as (1 / z - (a + 1)) / z: z^2 underflows before 1 / z overflows)
//    5 beta(a, b)    (a - 1) / z - (b - 1) / (1 - z)
//    6 expon         -1
//    8 laplace       -sign z (0 at z = 0)
//    9 cauchy        -2 z / (1 + z^2)
//   10 t(nu)         -(nu + 1) z / (nu + z^2)
//   12 weibull_min(c)   ((c - 1) - c exp(c log z)) / z
// As above the lanes diverge over the families present, and the one logarithm (families 2 and 12) is taken ahead of the switch.
__device__ double tda_logprior_term_grad(double x, double p, double q, int j) {
  const int f = tda_prior_family[j];
  const double a = tda_prior_a[j], b = tda_prior_b[j];
  const double z = (x - p) / q;
  const double lz = ((0x1004 >> f) & 1) ? log(z) : 0.0;
  double g;
  switch (f) {
    case 0: case 7: case 11: g = -z; break;
    case 1: g = 0.0; break;
    case 2: g = (-1.0 - lz / (a * a)) / z; break;
    case 3: g = (a - 1.0) / z - 1.0; break;
    case 4: g = (1.0 / z - (a + 1.0)) / z; break;
    case 5: g = (a - 1.0) / z - (b - 1.0) / (1.0 - z); break;
    case 6: g = -1.0; break;
    case 8: g = z > 0.0 ? -1.0 : (z < 0.0 ? 1.0 : 0.0); break;
    case 9: g = -2.0 * z / (1.0 + z * z); break;
    case 10: g = -(a + 1.0) * z / (a + z * z); break;
    case 12: g = ((a - 1.0) - a * exp(a * lz)) / z; break;
    default: g = __builtin_nan(""); break;  // (an id the prologue never writes)
  }
  return g / q;
}
