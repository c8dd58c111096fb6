#!/usr/bin/env python
"""The device code of every source-defined program, as one table: per valid combination of forms, the sha256 of the program's
normalised assembly (tests/extprogram.assembly).  Two program texts with equal tables compile to the same instructions.

    python tools/user_program_matrix.py [program.hip]          (default: the shipped csrc/tda_user_program.hip)

Step program: likelihood {gauss, source, wave} x prior {engine, term, wave} x model {per_output, wave}; MALA program: the same x
gradient {per_parameter, wave}.  The user sources are the ones tests/ext*.py hold; a combination they hold none for is listed
as such."""
import hashlib
import itertools
import os
import pathlib
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import extloglike as xl  # noqa: E402
from tests import extloglikewave as xlw  # noqa: E402
from tests import extmodel as xm  # noqa: E402
from tests import extprior as xp  # noqa: E402
from tests import extprogram  # noqa: E402
from tests import extpriorwave as xpw  # noqa: E402
from tests import extwave as xw  # noqa: E402
from tests.extpriorgrad import LOGNORMAL_GRAD_SRC  # noqa: E402

M = 23  # (the per-output form of tests/extwave.py has the number of outputs written in)
LIKELIHOODS = {"gauss": ("", []), "source": (xl.KINDS["t"][0], ["TDA_LOGLIKE_SOURCE"]),
               "wave": (xlw.MARGINAL_SRC, ["TDA_LOGLIKE_SOURCE", "TDA_LOGLIKE_WAVE"])}
PRIORS = {"engine": ("", []), "term": (xp.LOGNORMAL_SRC + LOGNORMAL_GRAD_SRC, ["TDA_PRIOR_SOURCE"]),
          "wave": (xpw.CAUCHY_DIFF_SRC, ["TDA_PRIOR_SOURCE", "TDA_PRIOR_WAVE"])}
MODELS = {"per_output": [], "wave": ["TDA_FORWARD_WAVE"]}
GRADIENTS = {"per_parameter": [], "wave": ["TDA_GRADIENT_WAVE"]}


def model_source(model, gradient):
    """the model of tests/extmodel.py where it serves (per output, tda_gradient per parameter), else that of tests/extwave.py"""
    if model == "per_output" and gradient in (None, "per_parameter"):
        return xm.source()
    return xw.source(model, gradient, m=M)


def rows():
    for like, prior, model in itertools.product(LIKELIHOODS, PRIORS, MODELS):
        yield "steps like=%s prior=%s model=%s" % (like, prior, model), model_source(model, None), like, prior, MODELS[model]
    for like, prior, model, grad in itertools.product(LIKELIHOODS, PRIORS, MODELS, GRADIENTS):
        yield ("mala  like=%s prior=%s model=%s gradient=%s" % (like, prior, model, grad), model_source(model, grad), like, prior,
               ["TDA_USER_MALA"] + MODELS[model] + GRADIENTS[grad])


def main():
    text = open(sys.argv[1]).read() if len(sys.argv) > 1 else None
    with tempfile.TemporaryDirectory() as tmp:
        for i, (label, model_src, like, prior, switches) in enumerate(rows()):
            try:
                user = model_src + LIKELIHOODS[like][0] + "\n" + PRIORS[prior][0]
                asm = extprogram.assembly(pathlib.Path(tmp), "row%d" % i, user, LIKELIHOODS[like][1] + PRIORS[prior][1] + switches, text)
                print("%-66s %s" % (label, hashlib.sha256(asm.encode()).hexdigest()), flush=True)
            except (AssertionError, KeyError) as exc:
                print("%-66s no source in tests/ext*.py compiles for it (%s)" % (label, str(exc).strip().splitlines()[-1][:80] if str(exc).strip() else type(exc).__name__), flush=True)


if __name__ == "__main__":
    main()
