"""logreg_amd -- many-chain MCMC for Bayesian logistic regression on AMD MI355X (gfx950).

Drop-in for the hot path of darrenjw/logreg's NumPy scripts (Python/fit-numpy.py,
fit-np-mala.py, fit-np-hmc.py, fit-np-ul.py): the same `ll / lprior / lpost / glp` closures and
`mhKernel / malaKernel / hmcKernel / ulKernel / mcmc` constructors (and `nutsKernel`, the sampler of fit-blackjax-nuts.py), executed by hand-written HIP
kernels through the C ABI in include/logreg_hip.h.  There is no CPU fallback.

    from logreg_amd import LogReg, hmcKernel, mcmc, load_pima
    X, y = load_pima()
    model = LogReg(X, y, pscale=[10, 1, 1, 1, 1, 1, 1, 1])
    kern = hmcKernel(model.lpost, model.glp, eps=1e-3, l=50, dmm=1 / pre)
    out = mcmc(init, kern, thin=20)                 # [10000, 8], like the reference
    out = mcmc(np.tile(init, (4096, 1)), kern, thin=20, iters=1000)   # [1000, 4096, 8]
"""
from ._lib import LogregHipError, device_count  # noqa: F401
from .autocorr import Autocorr, merge_autocorr  # noqa: F401
from .marginals import Marginals, marginal_grid, merge_marginals  # noqa: F401
from .covariance import Covariance, covariance_scaling, merge_covariance  # noqa: F401
from .data import load_pima, load_pima_parquet, synthetic_logreg  # noqa: F401
from .diagnostics import describe, ess_geyer, ess_per_param, ess_pooled, split_rhat, summarise  # noqa: F401
from .kernels import (ChainSet, FusedKernel, hmcKernel, malaKernel, mcmc, mhKernel, nutsKernel, pgKernel, hsKernel, rwProposal,  # noqa: F401
                      ulKernel)
from .adapt import nuts_warmup, nuts_warmup_dense, nuts_warmup_stepwise  # noqa: F401
from .model import DeviceArray, LogReg  # noqa: F401
from .optimize import find_map, laplace_metric, overdispersed_init  # noqa: F401
from .predict import PosteriorPredictive, merge_predictive, predict_proba, waic, waic_from_table  # noqa: F401
from .loo import PsisLoo, loo_compare, loo_from_table, psis_from_loglik, psis_loo  # noqa: F401
from .rankdiag import RankDiagnostics, rank_result_from_table  # noqa: F401
from .ppc import PredictiveCheck, ppc_from_table  # noqa: F401
from .bridge import Bridge, bridge_compare, bridge_from_table, bridge_from_terms, bridge_proposal, bridge_sampling  # noqa: F401
from .output import print_summary, read_parquet, to_frame, write_parquet  # noqa: F401

__all__ = ["LogReg", "DeviceArray", "ChainSet", "FusedKernel", "mhKernel", "malaKernel", "hmcKernel", "ulKernel", "nutsKernel", "pgKernel", "hsKernel",
           "rwProposal", "mcmc", "load_pima", "load_pima_parquet", "synthetic_logreg", "summarise", "describe",
           "ess_geyer", "ess_per_param", "ess_pooled", "split_rhat", "device_count", "LogregHipError", "find_map", "laplace_metric", "overdispersed_init", "write_parquet",
           "read_parquet", "to_frame", "print_summary", "PosteriorPredictive", "merge_predictive", "predict_proba", "waic", "waic_from_table", "Autocorr", "merge_autocorr", "Marginals", "marginal_grid", "merge_marginals", "Covariance", "covariance_scaling", "merge_covariance",
           "nuts_warmup", "nuts_warmup_dense", "nuts_warmup_stepwise", "PsisLoo", "psis_loo", "psis_from_loglik", "loo_from_table", "loo_compare",
           "RankDiagnostics", "rank_result_from_table", "PredictiveCheck", "ppc_from_table", "Bridge", "bridge_sampling", "bridge_from_terms", "bridge_from_table", "bridge_compare", "bridge_proposal"]
