"""The functions a HIP source may define for the engine, each signature written once for the Python side (the C++ side's are
TDA_SIG_* in csrc/tda_user_args.h; tests/test_user_build.py compares the two): every message that quotes one takes it from here."""

SIG = {
    "tda_forward": "__device__ double tda_forward(const double* theta, int dim, int o)",
    "tda_forward_wave": "__device__ void tda_forward_wave(const double* theta, int dim, double* out, int n_outputs, double* work, int lane)",
    "tda_gradient": "__device__ double tda_gradient(const double* theta, int dim, const double* sensitivity, int n_outputs, int j)",
    "tda_gradient_wave": "__device__ void tda_gradient_wave(const double* theta, int dim, const double* sensitivity, int n_outputs, double* grad, double* work, int lane)",
    "tda_loglike_term": "__device__ double tda_loglike_term(double f, double y, double p, int o)",
    "tda_loglike_term_grad": "__device__ double tda_loglike_term_grad(double f, double y, double p, int o)",
    "tda_loglike_wave": "__device__ double tda_loglike_wave(const double* f, int n_outputs, const double* y, const double* p, int lane)",
    "tda_loglike_grad_wave": "__device__ void tda_loglike_grad_wave(const double* f, int n_outputs, const double* y, const double* p, double* sens, int lane)",
    "tda_logprior_term": "__device__ double tda_logprior_term(double x, double p, double q, int j)",
    "tda_logprior_term_grad": "__device__ double tda_logprior_term_grad(double x, double p, double q, int j)",
    "tda_logprior_wave": "__device__ double tda_logprior_wave(const double* theta, int dim, const double* p, const double* q, int lane)",
    "tda_logprior_grad": "__device__ double tda_logprior_grad(const double* theta, int dim, const double* p, const double* q, int j)",
}

# the quantity of interest of a DeviceModel (TDA_SIG_QOI / TDA_SIG_QOI_WAVE; tests/test_replay.py compares the two sides)
QOI_SIG = {
    "tda_qoi": "__device__ double tda_qoi(const double* theta, int dim, const double* f, int n_outputs, int k)",
    "tda_qoi_wave": "__device__ void tda_qoi_wave(const double* theta, int dim, const double* f, int n_outputs, double* qoi, int n_qoi, double* work, int lane)",
}
