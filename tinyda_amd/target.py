"""Posterior = prior x likelihood x forward model (tinyDA/posterior.py:41-151)."""
import numpy as np

from . import _lib
from .likelihoods import DevicePrior
from .records import Link
from .models import BatchedModel, DeviceModel, LinearModel, Rosenbrock


class Posterior:
    def __init__(self, prior, likelihood, model=None):
        self.prior = prior
        self.likelihood = likelihood
        # subclasses may provide evaluate_model instead of passing a callable (posterior.py:57-61)
        self.model = self.evaluate_model if model is None else model

    def evaluate_model(self, parameters):  # pragma: no cover - to be overridden
        raise NotImplementedError("pass model= or override evaluate_model")

    def create_link(self, parameters):
        """prior.logpdf -> model -> loglike -> Link (posterior.py:78-110)."""
        log_prior = self.prior.logpdf(parameters)
        result = self.model(parameters)
        output, qoi = result if isinstance(result, tuple) else (result, None)
        if not isinstance(output, np.ndarray):
            raise TypeError("Model output must be a numpy array!")
        return Link(parameters, log_prior, output, self.likelihood.loglike(output), qoi)

    def update_link(self, link, bias=None):
        """Re-evaluate only the likelihood of an existing link (posterior.py:112-134)."""
        if bias is None:
            log_like = self.likelihood.loglike(link.model_output)
        else:
            log_like = self.likelihood.loglike_custom_bias(link.model_output, bias)
        return Link(link.parameters, link.prior, link.model_output, log_like, link.qoi)

    def logpdf(self, parameters):
        return self.create_link(parameters).posterior

    __call__ = logpdf

    # ---- device lowering ---------------------------------------------------------------
    def _lowering(self):
        """What the HIP engine needs, or None when this posterior only runs through the host protocol
        (opaque Python model, non-Gaussian prior, ...)."""
        prior = self.prior
        joint = None
        if isinstance(prior, DevicePrior) or (hasattr(prior, "distributions") and hasattr(prior, "_lowering")):
            # JointPrior of scalar components, DevicePrior
            joint = None if isinstance(prior, DevicePrior) else prior._lowering()
            if joint is None:
                # source-defined prior (DevicePrior, or a JointPrior of scipy families through the term library): its function is
                # compiled with the model (+ likelihood), one program per level; the moments are placeholders nothing reads
                joint = getattr(prior, "_source_lowering", lambda: None)()
                if joint is None:
                    return None
                kinds, p, q, src = joint
                low = self._lowering_with(np.zeros(kinds.shape[0]), np.eye(kinds.shape[0]))
                if low is not None:
                    low["prior_joint"] = (kinds, p, q)
                    # has_gradient: the source defines tda_logprior_term_grad too (MALA).  A JointPrior's lowering stays closed
                    # under MALA: DevicePrior.from_distributions is the route for scipy families there
                    low["prior_source"] = dict(source=src, p=p, q=q, label="DevicePrior" if isinstance(prior, DevicePrior)
                                               else "JointPrior of scipy families (source-defined prior)",
                                               has_gradient=isinstance(prior, DevicePrior) and prior.has_gradient,
                                               coupled=bool(getattr(prior, "coupled", False)))
                    if "source" in low:
                        low["source"] = low["source"] + "\n" + src
                return low
            kinds, loc, scale = joint
            low = self._lowering_with(np.where(kinds == 0, loc, loc + 0.5 * scale),
                                      np.diag(np.where(kinds == 0, scale ** 2, scale ** 2 / 12.0)))
            if low is not None:
                low["prior_joint"] = joint
            return low
        mean = getattr(prior, "mean", None)
        cov = getattr(prior, "cov", None)
        if cov is None and hasattr(prior, "cov_object"):
            cov = prior.cov_object.covariance
        if mean is None or cov is None or not hasattr(prior, "logpdf"):
            return None
        return self._lowering_with(mean, cov)

    def _lowering_with(self, mean, cov):
        if not isinstance(self.model, (LinearModel, Rosenbrock, DeviceModel, BatchedModel)) or not hasattr(self.likelihood, "_lowering"):
            return None
        mean = np.atleast_1d(np.asarray(mean, dtype=np.float64))
        cov = np.atleast_2d(np.asarray(cov, dtype=np.float64))
        kind, noise = self.likelihood._lowering()
        noise = np.asarray(noise, dtype=np.float64)
        data = np.asarray(self.likelihood.data, dtype=np.float64)
        if isinstance(self.model, LinearModel):
            if self.model.A.shape[1] != mean.shape[0]:
                return None
            return dict(prior_mean=mean, prior_cov=cov, A=self.model.A, b=self.model.b, data=data, noise_kind=kind, noise=noise)
        data = np.atleast_1d(data)
        low = dict(prior_mean=mean, prior_cov=cov, A=None, b=None, data=data, noise_kind=kind, noise=noise)
        if isinstance(self.model, Rosenbrock):
            if data.shape != (1,) or np.size(noise) != 1 or mean.shape[0] < 2:
                return None
            return dict(low, rosenbrock=(self.model.a, self.model.b), noise=noise.reshape(1))
        if data.shape != (self.model.n_outputs,):
            return None
        if isinstance(self.model, BatchedModel):
            return dict(low, batched=self.model.batch)
        low.update(source=self.model.source, has_gradient=self.model.has_gradient, has_forward_wave=self.model.has_forward_wave,
                   has_gradient_wave=self.model.has_gradient_wave)
        if kind == _lib.NOISE_SOURCE:  # DeviceLogLike: its functions are compiled with the model, one program
            low.update(source=self.model.source + "\n" + self.likelihood.source, loglike_source=True,
                       loglike_has_gradient=self.likelihood.has_gradient, loglike_coupled=bool(getattr(self.likelihood, "coupled", False)))
        return low
