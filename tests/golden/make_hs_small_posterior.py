"""Writes tests/golden/hs_small_posterior.json: posterior means of the small horseshoe model of tests/hs_reference.py (`small_model`) by
importance sampling from the prior -- no Gibbs step, no Polya-Gamma draw, nothing the samplers under test share.

    python tests/golden/make_hs_small_posterior.py

The target (include/logreg_hip_hs.h "The model"):  L(beta) prod_j N(beta_j; 0, ps_j^2) prod_{j in S} N(beta_j; 0, tau^2 lambda_j^2) C+(lambda_j; 0, 1) C+(tau; 0, tau0).
The proposal: lambda_j, tau half-Cauchy, then beta_j ~ N(0, v_j) with 1 / v_j = 1 / ps_j^2 + s_j / (tau^2 lambda_j^2) -- the product of the
two normals, normalised.  The product's constant is N(0; 0, ps_j^2 + tau^2 lambda_j^2) up to a factor free of the scales, so the weight is
    w = L(beta) prod_{j in S} (ps_j^2 + tau^2 lambda_j^2)^(-1/2),
bounded by prod_{j in S} 1 / ps_j: every self-normalised estimate has a finite variance.  The MCSE of a mean is sqrt(sum w^2 (f - mean)^2) / sum w;
that of a standard deviation follows by the delta method from g = ((f - mean)^2 - var) / (2 sd).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import hs_reference as hr  # noqa: E402

DRAWS, CHUNK, SEED = 1 << 24, 1 << 20, 777


def main():
    X, y = hr.small_model()
    ps, mask, tau0 = hr.SMALL_PSCALE, hr.SMALL_MASK, hr.SMALL_TAU0
    Xs = (2.0 * y - 1.0)[:, None] * X
    p = X.shape[1]
    rng = np.random.default_rng(SEED)
    ws, qs = [], []
    for _ in range(DRAWS // CHUNK):
        lam = np.abs(rng.standard_cauchy((CHUNK, p)))
        tau = tau0 * np.abs(rng.standard_cauchy(CHUNK))
        t2l2 = (tau * tau)[:, None] * (lam * lam)
        with np.errstate(divide="ignore"):
            v = 1.0 / (1.0 / ps ** 2 + np.where(mask, 1.0 / t2l2, 0.0))
        beta = np.sqrt(v) * rng.standard_normal((CHUNK, p))
        loglik = -np.logaddexp(0.0, -(beta @ Xs.T)).sum(axis=1)
        logw = loglik - 0.5 * np.log(ps[mask] ** 2 + t2l2[:, mask]).sum(axis=1)
        ws.append(np.exp(logw))
        qs.append(hr.posterior_quantities(beta, lam * lam, tau * tau, mask))
    w, q = np.concatenate(ws), np.concatenate(qs)
    W = w.sum()
    mean = (w[:, None] * q).sum(axis=0) / W
    dev = q - mean
    mean_mcse = np.sqrt((w[:, None] ** 2 * dev ** 2).sum(axis=0)) / W
    var = (w[:, None] * dev ** 2).sum(axis=0) / W
    sd = np.sqrt(var)
    g = (dev ** 2 - var) / (2.0 * sd)
    sd_mcse = np.sqrt((w[:, None] ** 2 * g ** 2).sum(axis=0)) / W
    names = [f"beta_{j}" for j in range(p)] + [f"kappa_{j}" for j in np.nonzero(mask)[0]] + ["log_tau2"]
    out = {"about": "importance sampling from the prior: tests/golden/make_hs_small_posterior.py", "draws": DRAWS, "seed": SEED, "ess": float(W * W / (w * w).sum()),
           "names": names, "mean": mean.tolist(), "mean_mcse": mean_mcse.tolist(), "sd": sd[:p].tolist(), "sd_mcse": sd_mcse[:p].tolist(),
           "X": X.tolist(), "y": y.tolist(), "pscale": ps.tolist(), "shrink": mask.tolist(), "global_scale": tau0}
    with open(os.path.join(HERE, "hs_small_posterior.json"), "w") as f:
        json.dump(out, f, indent=1)
    for k, nme in enumerate(names):
        print(f"{nme:10s} mean {mean[k]:+.5f} +- {mean_mcse[k]:.5f}" + (f"   sd {sd[k]:.5f} +- {sd_mcse[k]:.5f}" if k < p else ""))
    print("importance-sampling ESS", out["ess"])


if __name__ == "__main__":
    main()
