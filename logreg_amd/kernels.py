"""The reference's kernel constructors and chain driver, with the same names and signatures:

    mhKernel(lpost, rprop, dprop=...)            fit-numpy.py:53-62 / fit-np-mala.py:61-70 / fit-np-hmc.py:56-63
    malaKernel(lpi, glpi, dt=1e-4, pre=1)        fit-np-mala.py:72-78
    hmcKernel(lpi, glpi, eps=1e-4, l=10, dmm=1)  fit-np-hmc.py:65-87
    ulKernel(glpi, dt=1e-4, pre=1)               fit-np-ul.py:61-68
    nutsKernel(lpi, glpi, eps=1e-4, dmm=1, max_depth=10)   blackjax.nuts in fit-blackjax-nuts.py:101 (dmm = 1 / pre)
    pgKernel(lpost)                              the tuning-free Gibbs sampler (fit-rjags.R's role): Polya-Gamma augmentation
    hsKernel(lpost, shrink, global_scale)        the same sampler under the horseshoe prior, for sparse models (no counterpart in the reference)
    mcmc(init, kernel, thin=10, iters=10000, verb=True)   fit-np-hmc.py:89-103

When the callables passed in are the closures of a `LogReg` model (and, for RWMH, a
`rwProposal`), the constructors return a `FusedKernel`: still callable one step at a time with
the reference's per-step signature, but `mcmc()` recognises it and runs the whole
`iters x thin` loop for all chains inside one HIP kernel launch per chunk.

Any other callables get the reference's generic composition semantics (the kernel simply calls
what it was given, drawing from NumPy's global RNG exactly where the reference does); that path
contains no model arithmetic of its own.

Extensions (additive): `init` may be `[C, p]` (then `mcmc` returns `[iters, C, p]`);
`mcmc(..., seed=, chunk=, group=, mode=, chain_offset=, return_info=)`.
"""
from __future__ import annotations

import ctypes as C
import sys

import numpy as np

from . import _lib
from ._lib import RunOpts, check
from .model import DeviceArray, LogReg, ModelFn

# lr_nuts_counters (include/logreg_hip_nuts.h) as a NumPy record
NUTS_COUNTERS = np.dtype([("n_leapfrog", "<u8"), ("depth_sum", "<u8"), ("accept_stat_sum", "<f8"), ("divergent", "<u4"),
                          ("max_depth_hits", "<u4")])
# lr_pg_counters (include/logreg_hip_pg.h) as a NumPy record
PG_COUNTERS = np.dtype([("proposals", "<u8"), ("series_terms", "<u8"), ("skipped", "<u4"), ("reserved", "<u4")])
# lr_hs_counters (include/logreg_hip_hs.h)
HS_COUNTERS = np.dtype([("proposals", "<u8"), ("series_terms", "<u8"), ("skipped", "<u4"), ("clamped", "<u4")])
_COUNTERS_BY_KIND = {"nuts": ("nuts_", NUTS_COUNTERS), "pg": ("pg_", PG_COUNTERS), "hs": ("hs_", HS_COUNTERS)}  # checkpoint prefix, record


# ------------------------------------------------------------------------------------------------
def _default_dprop(new, old):  # fit-numpy.py:53 `dprop = lambda new, old: 1.`
    return 1.0


class RandomWalkProposal:
    """rprop(beta) = beta + sd * N(0, I)   (fit-numpy.py:81-84 with sd = 0.02*pre)."""

    def __init__(self, sd):
        self.sd = np.asarray(sd, dtype=np.float64)

    def __call__(self, beta):
        beta = np.asarray(beta, dtype=np.float64)
        return beta + self.sd * np.random.randn(*beta.shape)


def rwProposal(sd) -> RandomWalkProposal:
    return RandomWalkProposal(sd)


_PROBE_LOCK = __import__("threading").Lock()


def _model_of(fn, kind):
    return fn.model if isinstance(fn, ModelFn) and fn.kind == kind else None


def _recognise_random_walk(rprop, p):
    """The proposal scale `sd` if the Python callable `rprop` is the reference's random-walk proposal
    `beta + sd * np.random.randn(p)` (fit-numpy.py:81-84, `sd = 0.02*pre`), else None.

    The script's own `rprop` is an opaque function, so it is PROBED, with `np.random.randn` replaced by recorded stand-ins
    (NumPy's global generator is not touched): zeros must give the identity, unit vectors the diagonal scale, and two
    random draws at two random points must reproduce `x + sd * z` to the last bit or two; exactly one `randn` call of p
    values per proposal.  Anything else -- another generator, a dense or state-dependent scale, side effects that raise --
    is not recognised and the kernel stays on the generic path."""
    if isinstance(rprop, RandomWalkProposal):
        return rprop.sd
    if not callable(rprop):
        return None
    with _PROBE_LOCK:  # np.random.randn is process-wide state while patched: one probe at a time
        state = np.random.get_state()  # a proposal that draws through another np.random function must not move the caller's seeded stream
        try:
            return _probe_random_walk(rprop, p)
        finally:
            np.random.set_state(state)


def _probe_random_walk(rprop, p):
    saved = np.random.randn
    calls = []

    def probe(x, z):
        def fake(*shape):
            calls.append(shape)
            return np.array(z, dtype=np.float64).reshape(shape if shape else ())
        np.random.randn = fake
        try:
            out = rprop(np.array(x, dtype=np.float64))
        finally:
            np.random.randn = saved
        out = np.asarray(out, dtype=np.float64)
        if out.shape != (p,) or not np.all(np.isfinite(out)):
            raise ValueError("not a [p] -> [p] map")
        return out
    try:
        x0 = np.linspace(-1.0, 1.0, p) * 0.37 + 0.11
        if not np.array_equal(probe(x0, np.zeros(p)), x0):
            return None
        sd = np.empty(p)
        for j in range(p):
            d = probe(np.zeros(p), np.eye(p)[j])  # at the origin: 0 + sd_j * 1 is sd_j to the last bit
            if np.any(d[np.arange(p) != j] != 0.0):
                return None  # a dense proposal covariance
            sd[j] = d[j]
        if np.any(sd < 0) or len(calls) != p + 1 or any(int(np.prod(c)) != p for c in calls):
            return None
        rng = np.random.RandomState(12345)  # a private generator: the caller's seeding of the global one stays as it is
        for _ in range(2):
            x, z = 3.0 * rng.standard_normal(p), rng.standard_normal(p)
            if not np.allclose(probe(x, z), x + sd * z, rtol=1e-14, atol=1e-300):
                return None
    except Exception:
        return None
    return sd


# ------------------------------------------------------------------------------------------------
class FusedKernel:
    """A transition kernel whose whole step runs inside the HIP chain kernel.

    kind in {"rwmh", "mala", "hmc", "ul", "nuts", "pg", "hs"}.  Calling it performs ONE iteration on the device with
    the reference's per-step signature: `kernel(x, ll) -> (x, ll)` for rwmh/mala (the threaded
    log-density, fit-np-mala.py:61-70), `kernel(x) -> x` for hmc/ul/nuts/pg/hs.  Successive calls use
    successive iteration indices of the kernel's own Philox stream.
    """

    def __init__(self, kind: str, model: LogReg, **params):
        self.kind = kind
        self.model = model
        self.params = params
        self.threaded = kind in ("rwmh", "mala")
        self._seed = None
        self._calls = 0

    def __repr__(self):
        return f"FusedKernel({self.kind}, {self.params}, {self.model!r})"

    def _vec(self, name):
        return np.ascontiguousarray(np.broadcast_to(np.asarray(self.params[name], dtype=np.float64), (self.model.p,)))

    def launch(self, opts: RunOpts, state_ptr, lp_ptr, out_ptr, acc_ptr, counters_ptr=None, depth_ptr=None, hyper_ptr=None, scale_ptr=None):
        """One lr_run_<kind> call.  NUTS has no accept counts and no threaded log-density: it takes the per-chain counters
        (lr_nuts_counters) and the optional tree depths of the kept rows instead; the Polya-Gamma sampler its own counters
        (lr_pg_counters); the horseshoe sampler lr_hs_counters, the hyper-state `[C, 2p+2]` (required) and the optional scales of the
        kept rows `[iters, C, p+1]`."""
        L = self.model._L
        h = self.model.handle
        if self.kind == "hs":
            mask = np.ascontiguousarray(self.params["shrink"], dtype=np.uint8)
            prior = _lib.HsPrior(mask.ctypes.data, float(self.params["global_scale"]))
            check(_lib.bind_hs(L).lr_run_hs(h, C.byref(prior), state_ptr, hyper_ptr, C.byref(opts), out_ptr, scale_ptr, counters_ptr))
        elif self.kind == "pg":
            check(_lib.bind_pg(L).lr_run_pg(h, state_ptr, C.byref(opts), out_ptr, counters_ptr))
        elif self.kind == "nuts" and self.params.get("inv_metric") is not None:  # dense metric (include/logreg_hip_dense.h)
            v = self.params["inv_metric"]
            check(_lib.bind_dense(L).lr_run_nuts_dense(h, state_ptr, float(self.params["eps"]), int(self.params["max_depth"]), v.ctypes.data,
                                                       C.byref(opts), out_ptr, counters_ptr, depth_ptr))
        elif self.kind == "nuts":
            v = self._vec("dmm")
            check(_lib.bind_nuts(L).lr_run_nuts(h, state_ptr, float(self.params["eps"]), int(self.params["max_depth"]), v.ctypes.data,
                                                C.byref(opts), out_ptr, counters_ptr, depth_ptr))
        elif self.kind == "rwmh":
            v = self._vec("prop_sd")
            check(L.lr_run_rwmh(h, state_ptr, lp_ptr, v.ctypes.data, C.byref(opts), out_ptr, acc_ptr))
        elif self.kind == "mala":
            v = self._vec("pre")
            check(L.lr_run_mala(h, state_ptr, lp_ptr, float(self.params["dt"]), v.ctypes.data, C.byref(opts), out_ptr,
                                acc_ptr))
        elif self.kind == "ul":
            v = self._vec("pre")
            check(L.lr_run_ul(h, state_ptr, float(self.params["dt"]), v.ctypes.data, C.byref(opts), out_ptr, acc_ptr))
        elif self.kind == "hmc":
            v = self._vec("dmm")
            check(L.lr_run_hmc(h, state_ptr, float(self.params["eps"]), int(self.params["l"]), v.ctypes.data,
                               C.byref(opts), out_ptr, acc_ptr))
        else:
            raise ValueError(self.kind)

    # one step, reference signature
    def __call__(self, x, ll=None):
        if self._seed is None:
            self._seed = int(np.random.randint(0, 2**31 - 1))
        x = np.asarray(x, dtype=np.float64)
        single = x.ndim == 1
        st = np.array(np.atleast_2d(x), dtype=self.model.np_dtype, order="C")  # a copy: the launch updates it in place, the caller's x stays
        Cn = st.shape[0]
        lp = np.ascontiguousarray(np.broadcast_to(np.asarray(-np.inf if ll is None else ll, dtype=np.float64), (Cn,))).copy()
        opts = RunOpts(n_chains=Cn, chain_offset=0, thin=1, iters=1, iter_offset=self._calls, seed=self._seed,
                       group=0, mode=_lib.MODE_AUTO, on_device=0)
        hyper_ptr = None
        if self.kind == "hs":  # the scales travel with the kernel object between calls (a new chain count starts them afresh)
            if getattr(self, "_hyper", None) is None or self._hyper.shape[0] != Cn:
                self._hyper = default_hyper(Cn, self.model.p, self.params["global_scale"])
            hyper_ptr = self._hyper.ctypes.data
        self.launch(opts, st.ctypes.data, lp.ctypes.data, None, None, hyper_ptr=hyper_ptr)
        self._calls += 1
        xo = st.astype(np.float64)
        if single:
            xo = xo[0]
        if self.threaded:
            return xo, (float(lp[0]) if single else lp)
        return xo


# ------------------------------------------------------------------------------------------------
def mhKernel(lpost, rprop, dprop=_default_dprop, *, fuse=True):
    """Metropolis-Hastings kernel constructor.

    `fuse=False` (an addition to the reference's signature) keeps the reference's generic composition whatever `rprop` is: the caller's
    own Python proposal is then called every step and draws from NumPy's generator, instead of being recognised and replaced by the
    device kernel's Philox draws.  A fused kernel says how its proposal was recognised in `kernel.proposal` ("rwProposal" | "probed"),
    which `mcmc(..., return_info=True)` reports as `info["proposal"]`.

    Fused when `lpost` is a LogReg's lpost and `rprop` is a random-walk proposal `beta + sd * N(0, I)` -- a
    `rwProposal(sd)`, or the script's own Python function `rprop` (fit-numpy.py:81-84), recognised by probing it
    (`_recognise_random_walk`) -- so that the reference's call `mhKernel(lpost, rprop)` runs fused unchanged
    (fit-numpy.py:53-62,86).  Otherwise the reference's generic composition: the returned
    `kernel(x, ll)` threads the current log-density (fit-numpy.py:54-61); called as `kernel(x)`
    it re-evaluates both ends like the HMC script's variant (fit-np-hmc.py:56-63)."""
    model = _model_of(lpost, "lpost")
    if fuse and model is not None and dprop is _default_dprop:
        sd = _recognise_random_walk(rprop, model.p)  # a rwProposal, or the script's own `rprop` recognised by probing it
        if sd is not None:
            k = FusedKernel("rwmh", model, prop_sd=sd)
            k.proposal = "rwProposal" if isinstance(rprop, RandomWalkProposal) else "probed"
            return k

    def kernel(x, ll=None):
        prop = rprop(x)
        lp = lpost(prop)
        if ll is None:  # fit-np-hmc.py:59
            a = lp - lpost(x)
        else:  # fit-numpy.py:57
            a = lp - ll + dprop(x, prop) - dprop(prop, x)
        if np.log(np.random.rand()) < a:
            x = prop
            ll = lp if ll is not None else None
        return x if ll is None else (x, ll)
    return kernel


def malaKernel(lpi, glpi, dt=1e-4, pre=1):
    """MALA with diagonal pre-conditioner (fit-np-mala.py:72-78)."""
    model = _model_of(lpi, "lpost")
    if model is not None and _model_of(glpi, "glp") is model:
        return FusedKernel("mala", model, dt=float(dt), pre=pre)
    sdt = np.sqrt(dt)
    spre = np.sqrt(pre)

    def advance(x):
        return x + 0.5 * pre * glpi(x) * dt

    def lognorm(x, loc, scale):
        z = (x - loc) / scale
        return np.sum(-0.5 * z * z - 0.5 * np.log(2 * np.pi) - np.log(scale))
    return mhKernel(lpi, lambda x: advance(x) + np.random.randn(*np.shape(x)) * spre * sdt,
                    lambda new, old: lognorm(new, advance(old), spre * sdt * np.ones(np.shape(new))))


def ulKernel(glpi, dt=1e-4, pre=1):
    """Unadjusted Langevin (fit-np-ul.py:61-68)."""
    model = _model_of(glpi, "glp")
    if model is not None:
        return FusedKernel("ul", model, dt=float(dt), pre=pre)
    sdt = np.sqrt(dt)
    spre = np.sqrt(pre)

    def kernel(x):
        return x + 0.5 * pre * glpi(x) * dt + np.random.randn(*np.shape(x)) * spre * sdt
    return kernel


def hmcKernel(lpi, glpi, eps=1e-4, l=10, dmm=1):
    """HMC with diagonal mass matrix (fit-np-hmc.py:65-87)."""
    model = _model_of(lpi, "lpost")
    if model is not None and _model_of(glpi, "glp") is model:
        return FusedKernel("hmc", model, eps=float(eps), l=int(l), dmm=dmm)
    sdmm = np.sqrt(dmm)

    def leapf(q, p):
        p = p + 0.5 * eps * glpi(q)
        for i in range(l):
            q = q + eps * p / dmm
            p = p + (eps if i < l - 1 else 0.5 * eps) * glpi(q)
        return (q, -p)

    def alpi(x):
        q, p = x
        return lpi(q) - 0.5 * np.sum((p ** 2) / dmm)
    mhk = mhKernel(alpi, lambda x: leapf(*x))

    def kern(q):
        p = np.random.randn(len(q)) * sdmm
        return mhk((q, p))[0]
    return kern


def dense_factor(inv_metric):
    """-> (s [p], R [p, p], A [p, p]) of a dense inverse metric Sigma (include/logreg_hip_dense.h "Factorisation", `lr_dense_factor`: host
    code, no device): s = sqrt(diag Sigma), R = Sigma / (s s^T), A = L^-T with R = L L^T.  p = (A z) / s has covariance Sigma^-1.
    Only the lower triangle is read; a Sigma that is not finite or not positive definite raises."""
    sig = _inv_metric_array(inv_metric, None)
    p = sig.shape[0]
    s, R, A = np.empty(p), np.empty((p, p)), np.empty((p, p))
    L = _lib.load_factor()  # the library itself, whichever handle load() returns: the error text below is then its own too
    rc = L.lr_dense_factor(p, sig.ctypes.data, s.ctypes.data, R.ctypes.data, A.ctypes.data)
    if rc != 0:
        raise _lib.LogregHipError(f"liblogreg_hip error {rc}: {L.lr_last_error().decode()}")
    return s, R, A


def _inv_metric_array(inv_metric, p):
    sig = np.array(inv_metric, dtype=np.float64, order="C")
    if sig.ndim != 2 or sig.shape[0] != sig.shape[1] or (p is not None and sig.shape[0] != p):
        raise ValueError(f"inv_metric must be a square matrix [p, p]" + (f" with p={p}" if p is not None else "") + f"; got {np.shape(inv_metric)}")
    return sig


def nutsKernel(lpi, glpi, eps=1e-4, dmm=1, max_depth=10, *, inv_metric=None):
    """The No-U-Turn sampler with diagonal metric, in the reference HMC's convention (fit-np-hmc.py:65-87): p ~ N(0, dmm),
    H = -lpi(q) + sum(p^2 / dmm) / 2, q += eps * p / dmm.  Multinomial NUTS, iterative with U-turn checkpoints, at most `max_depth`
    doublings (DESIGN.md "NUTS").  `blackjax.nuts(lpost, eps, pre)` (fit-blackjax-nuts.py:101) is `nutsKernel(lpost, glp, eps, 1 / pre)`.

    `inv_metric=` a `[p, p]` symmetric positive definite matrix selects the DENSE metric instead (`dmm` is then not read): BlackJAX's
    matrix `inverse_mass_matrix`, about the posterior covariance -- p ~ N(0, inv_metric^-1), H = -lpi(q) + p^T inv_metric p / 2,
    q += eps * inv_metric p (include/logreg_hip_dense.h).  `dmm` is the diagonal case inv_metric = diag(1 / dmm).

    A LogReg's closures give a FusedKernel (include/logreg_hip_nuts.h); any other callables a plain NumPy NUTS that draws from
    NumPy's global generator, like the other generic kernels.

    The fused kernel keeps the rows in LDS: p <= 32 and a few thousand rows; beyond that the default mode raises with the reason.  Tall
    and wide models (p <= 128) -- those shapes and no others -- run the same chain with `mcmc(..., mode="stepwise")` /
    `ChainSet(..., mode="stepwise")`, diagonal metric only: one evaluation and one update launch per leapfrog step, all chains of a call in lockstep, `group=` the number of row slices
    (`examples/fit_nuts_tall.py`).  Such a call waits on its stream up to `max_depth - 1` times per iteration."""
    max_depth = int(max_depth)
    if not 1 <= max_depth <= _lib.NUTS_MAX_DEPTH:
        raise ValueError(f"max_depth must be in 1..{_lib.NUTS_MAX_DEPTH}, got {max_depth}")
    model = _model_of(lpi, "lpost")
    fused = model is not None and _model_of(glpi, "glp") is model
    if inv_metric is not None:
        sig = _inv_metric_array(inv_metric, model.p if fused else None)
        factor = dense_factor(sig)  # refuses what is not finite or not positive definite, here rather than at the first launch
        if fused:
            return FusedKernel("nuts", model, eps=float(eps), inv_metric=sig, max_depth=max_depth)
        return _numpy_nuts(lpi, glpi, float(eps), None, max_depth, dense=(sig, factor))
    if fused:
        return FusedKernel("nuts", model, eps=float(eps), dmm=dmm, max_depth=max_depth)
    return _numpy_nuts(lpi, glpi, float(eps), dmm, max_depth)


def pgKernel(lpost):
    """The Polya-Gamma Gibbs sampler of Polson, Scott & Windle (2013) for the logistic-regression posterior of a `LogReg`: an exact
    Gibbs sweep per iteration (omega_i ~ PG(1, |x_i . beta|), then beta ~ N(A^-1 b, A^-1)), with no tuning constant, no accept step
    and no warm-up (include/logreg_hip_pg.h).  Takes the model's `lpost` closure and returns `FusedKernel("pg", model)`.

    The sampler is built from the design X and the labels y, not from a log-density, so anything but a LogReg's closure is refused."""
    model = _model_of(lpost, "lpost")
    if model is None:
        raise TypeError("pgKernel needs the `lpost` closure of a LogReg: the Polya-Gamma sampler is built from the model's X, y and prior "
                        f"scale, not from a log-density it could call (got {type(lpost).__name__})")
    return FusedKernel("pg", model)


def default_hyper(C, p, global_scale):
    """The default start of the horseshoe's hyper-state `[C, 2p+2]`: lambda^2 = nu = xi = 1, tau^2 = global_scale^2."""
    h = np.ones((int(C), 2 * int(p) + 2), dtype=np.float64)
    h[:, 2 * int(p)] = float(global_scale) ** 2
    return h


def hsKernel(lpost, shrink=None, global_scale=1.0):
    """The Polya-Gamma Gibbs sampler under the horseshoe prior (Carvalho, Polson & Scott 2010), for sparse models: `pgKernel`'s sweep
    with the local scales lambda_j and the global scale tau as further Gibbs blocks (include/logreg_hip_hs.h).  Tuning-free like
    `pgKernel`: no step size, no accept step, no warm-up.

    `shrink`: a boolean mask `[p]` of the coordinates under the horseshoe; the default is every coordinate but 0 (the intercept
    column).  The model's own Gaussian N(0, pscale_j^2) stays on every coordinate: on a shrunk one it is the slab of the regularised
    horseshoe, an unshrunk one keeps exactly `pgKernel`'s prior.  `global_scale`: tau0 of tau ~ C+(0, tau0); for p0 expected nonzero
    effects among m shrunk ones and n rows, Piironen & Vehtari (2017) suggest `p0 / (m - p0) / sqrt(n)` (examples/fit_hs.py).
    Returns `FusedKernel("hs", model, shrink=mask, global_scale=tau0)`; a `ChainSet` of it carries the hyper-state
    (`get_hyper` / `set_hyper`), and `mcmc(..., return_info=True)` reports the scales of the kept draws."""
    model = _model_of(lpost, "lpost")
    if model is None:
        raise TypeError("hsKernel needs the `lpost` closure of a LogReg: the Polya-Gamma sampler is built from the model's X, y and prior "
                        f"scale, not from a log-density it could call (got {type(lpost).__name__})")
    if shrink is None:
        mask = np.arange(model.p) > 0
    else:
        mask = np.asarray(shrink)
        if mask.shape != (model.p,) or mask.dtype != np.bool_:
            raise ValueError(f"shrink must be a boolean mask of shape [{model.p}]; got {mask.dtype} {mask.shape}")
    if not mask.any():
        raise ValueError("shrink selects no coordinate: that model is pgKernel's (a LogReg with p = 1 has nothing but its first column)")
    try:
        tau0 = float(global_scale)
    except (TypeError, ValueError):
        raise ValueError(f"global_scale must be a number; got {global_scale!r}") from None
    if not (np.isfinite(tau0) and tau0 > 0):
        raise ValueError(f"global_scale must be finite and > 0; got {global_scale!r}")
    return FusedKernel("hs", model, shrink=mask.copy(), global_scale=tau0)


def _numpy_nuts(lpi, glpi, eps, dmm, max_depth, dense=None):
    """The same algorithm on NumPy arrays for arbitrary callables (the generic path: NumPy's global generator, no model arithmetic of
    its own).  `dense` = (Sigma, (s, R, A)): the dense metric -- `c` below is then the matrix Sigma, applied as a product."""
    if dense is not None:
        sigma, (s_, _, A_) = dense
        sigma = np.tril(sigma) + np.tril(sigma, -1).T  # the lower triangle, as the library reads it

    def velocity(c, v):  # (inverse metric) v
        return c @ v if dense is not None else c * v

    def kinetic2(c, v):
        return np.dot(v, c @ v) if dense is not None else np.sum(c * v * v)

    def turning(c, a, b, rho):
        r = rho - 0.5 * (a + b)
        if dense is not None:
            r = c @ r
            return np.dot(a, r) <= 0 or np.dot(b, r) <= 0
        return np.dot(c * a, r) <= 0 or np.dot(c * b, r) <= 0

    def lae(a, b):
        return np.logaddexp(a, b)

    def kern(q):
        q = np.asarray(q, dtype=np.float64)
        x, g, lp = q, np.asarray(glpi(q), dtype=np.float64), float(lpi(q))
        if dense is not None:
            c = sigma
            p0 = (A_ @ np.random.randn(len(q))) / s_
        else:
            dm = np.broadcast_to(np.asarray(dmm, dtype=np.float64), q.shape)
            c = 1.0 / dm
            p0 = np.random.randn(len(q)) * np.sqrt(dm)
        H0 = 0.5 * kinetic2(c, p0) - lp
        ends = {-1: (x, p0, g), 1: (x, p0, g)}
        rho, W, prop = p0.copy(), 0.0, x
        for d in range(max_depth):
            sgn = 1 if np.random.rand() < 0.5 else -1
            cq, cp, cg = ends[sgn]
            pinner, rhos, Ws, ck, stop = cp, np.zeros_like(q), 0.0, {}, False
            sub = pfirst = None
            for i in range(2 ** d):
                cp = cp + sgn * 0.5 * eps * cg
                cq = cq + sgn * eps * velocity(c, cp)
                lpl, cg = float(lpi(cq)), np.asarray(glpi(cq), dtype=np.float64)
                cp = cp + sgn * 0.5 * eps * cg
                delta = 0.5 * kinetic2(c, cp) - lpl - H0
                if not np.isfinite(delta) or delta > 1000:
                    return prop  # divergence: the subtree is discarded, the iteration ends
                rhos = rhos + cp
                if i == 0:
                    Ws, sub, pfirst = -delta, cq, cp
                else:
                    Wn = lae(Ws, -delta)
                    if np.random.rand() < np.exp(-delta - Wn):
                        sub = cq
                    Ws = Wn
                imax = bin(i >> 1).count("1")
                if i % 2 == 0:
                    ck[imax] = (cp, rhos)
                else:
                    imin = imax - (len(bin(i)) - len(bin(i).rstrip("1"))) + 1
                    if any(turning(c, ck[j][0], cp, rhos - ck[j][1] + ck[j][0]) for j in range(imin, imax + 1)):
                        stop = True
                        break
            if stop:
                return prop
            if np.random.rand() < np.exp(Ws - W):
                prop = sub
            W = lae(W, Ws)
            pouter = ends[-sgn][1]
            ends[sgn] = (cq, cp, cg)
            rho_old, rho = rho, rho + rhos
            if (turning(c, ends[-1][1], ends[1][1], rho) or turning(c, pouter, pfirst, rho_old + pfirst)
                    or turning(c, cp, pinner, rhos + pinner)):
                return prop
        return prop
    return kern


# ------------------------------------------------------------------------------------------------
class ChainSet:
    """C chains of one FusedKernel, resident on the device between launches.

    `advance(iters, thin)` enqueues one fused launch (iters*thin iterations per chain) and
    returns the thinned samples as a DeviceArray [iters, C, p] (or None with keep=False).
    Iteration counters advance automatically, so any chunking of a run gives identical output.
    """

    def __init__(self, kernel: FusedKernel, init, seed: int, chain_offset: int = 0, ll=None, group: int = 0,
                 mode: str = "auto", stream=None, precision: str = "auto", plan_chains: int = 0, plan_first: int = 0):
        self.kernel = kernel
        self.model = kernel.model
        m = self.model
        st = np.ascontiguousarray(np.atleast_2d(np.asarray(init, dtype=np.float64)), dtype=m.np_dtype)
        if st.ndim != 2 or st.shape[1] != m.p:
            raise ValueError(f"init must be [p] or [C,p] with p={m.p}; got {np.shape(init)}")
        self.C = st.shape[0]
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.chain_offset = int(chain_offset)
        self.iter_offset = 0
        self.group = int(group)
        self.mode = _lib.MODE_BY_NAME[mode]
        # arithmetic of HMC's interior leapfrog gradients (include/logreg_hip.h LR_PREC_*): "auto" | "full" | "bf16"
        self.precision = _lib.PREC_BY_NAME[precision]
        # chain count every chain-count-dependent choice is made for (0 = this set's own): a shard of a larger run passes the
        # whole run's count and reproduces the one-GPU run bit for bit (lr_run_opts.plan_chains)
        self.plan_chains = int(plan_chains)
        # ... and the global id of that run's first chain (a two-part plan assigns a chain to its part by its position in the run)
        self.plan_first = int(plan_first)
        self.stream = stream
        self.state = DeviceArray.from_host(m.device, st)
        lp0 = np.full(self.C, -np.inf) if ll is None else np.broadcast_to(np.asarray(ll, dtype=np.float64), (self.C,))
        self.lp = DeviceArray.from_host(m.device, lp0, dtype=np.float64)
        self.acc = DeviceArray(m.device, (self.C,), np.uint32)
        self.acc.zero_()
        self.counters = None  # NUTS / PG: per-chain lr_nuts_counters / lr_pg_counters, added to by every launch
        if kernel.kind in _COUNTERS_BY_KIND:
            self.counters = DeviceArray(m.device, (self.C,), _COUNTERS_BY_KIND[kernel.kind][1])
            self.counters.zero_()
        self.hyper = None  # horseshoe: the hyper-state [C, 2p+2] (lambda^2, nu, tau^2, xi), float64, moved by every launch
        if kernel.kind == "hs":
            self.hyper = DeviceArray.from_host(m.device, default_hyper(self.C, m.p, kernel.params["global_scale"]), dtype=np.float64)
        check(m._L.lr_stream_sync(m.device, None))
        # streaming statistics (enable_stats): device buffer [slots, C, 2, p], batch length, kept samples folded in
        self.stats = None
        self.stats_batch = 0
        self.stats_kept = 0
        self.pivot = st[0].astype(np.float64)  # any point near the posterior; shards of one run must share it

    def plan(self):
        """The kernel variant `advance` launches for this chain set (family- and precision-aware: `lr_plan_run`)."""
        opts = RunOpts(n_chains=self.C, group=self.group, mode=self.mode, precision=self.precision, plan_chains=self.plan_chains,
                       chain_offset=self.chain_offset, plan_first=self.plan_first)
        info = _lib.PlanInfo()
        kind = "pg" if self.kernel.kind == "hs" else self.kernel.kind  # (the horseshoe sampler is planned as lr_run_pg is)
        check(self.model._L.lr_plan_run_info(self.model.handle, _lib.KIND_BY_NAME[kind], C.byref(opts), C.byref(info)))
        plan = {"mode": _lib.MODE_NAMES[info.mode], "group": info.group, "rows_per_lane": info.rows}
        if info.split > 0:  # a run planned in two parts: chains [split, n) of the planned run on wider lane groups
            plan["tail"] = {"from": int(info.split), "mode": _lib.MODE_NAMES[info.tail_mode], "group": info.tail_group,
                            "rows_per_lane": info.tail_rows}
        return plan

    def enable_stats(self, batch: int, slots: int, pivot=None):
        """Start a statistics window: from now on every kept sample is folded, on the device, into the running
        (mean, M2) of its batch of `batch` kept samples (include/logreg_hip.h "Streaming statistics"); `slots`
        batches are provided for.  The window restarts at the current state."""
        m = self.model
        if self.stats is not None:
            self.stats.free()
        self.stats = DeviceArray(m.device, (int(slots), self.C, 2, m.p), np.float64)
        self.stats_batch = int(batch)
        self.stats_kept = 0
        if pivot is not None:
            self.pivot = np.asarray(pivot, dtype=np.float64).copy()

    def advance(self, iters: int, thin: int, keep: bool = True, out: DeviceArray | None = None, stats: bool | None = None,
                depth: DeviceArray | None = None, scales: DeviceArray | None = None):
        """One fused launch: iters*thin iterations per chain.  keep: return the thinned samples `[iters, C, p]`
        (a DeviceArray); stats (default: on when enable_stats was called): fold the kept samples into the
        streaming statistics -- with keep=False nothing of size iters*C*p is ever allocated.
        depth (NUTS): an int8 DeviceArray `[iters, C]` that receives the tree depth of the iteration behind each kept row (negated
        when it diverged).
        scales (horseshoe): a float64 DeviceArray `[iters, C, p+1]` that receives, with each kept row, lambda_j^2 (1 where unshrunk) and
        tau^2 at index p."""
        m = self.model
        if scales is not None and (self.kernel.kind != "hs" or scales.shape != (int(iters), self.C, m.p + 1) or scales.dtype != np.float64):
            raise ValueError(f"scales= takes a float64 [iters, C, p+1] = [{int(iters)}, {self.C}, {m.p + 1}] array of a horseshoe chain set")
        if keep and out is None:
            out = DeviceArray(m.device, (iters, self.C, m.p), m.np_dtype)
        opts = RunOpts(n_chains=self.C, chain_offset=self.chain_offset, thin=int(thin), iters=int(iters),
                       iter_offset=self.iter_offset, seed=self.seed, group=self.group, mode=self.mode, on_device=1,
                       stream=self.stream, precision=self.precision, plan_chains=self.plan_chains, plan_first=self.plan_first)
        use_stats = self.stats is not None if stats is None else bool(stats)
        if use_stats:
            if self.stats is None:
                raise ValueError("advance(stats=True) needs enable_stats(batch, slots) first")
            opts.stats, opts.stats_batch = self.stats.ptr, self.stats_batch
            opts.stats_first, opts.stats_slots = self.stats_kept, self.stats.shape[0]
        if depth is not None and (self.kernel.kind != "nuts" or depth.shape != (int(iters), self.C) or depth.dtype != np.int8):
            raise ValueError(f"depth= takes an int8 [iters, C] = [{int(iters)}, {self.C}] array of a NUTS chain set")
        self.kernel.launch(opts, self.state.ptr, self.lp.ptr, out.ptr if keep else None, self.acc.ptr,
                           self.counters.ptr if self.counters is not None else None, depth.ptr if depth is not None else None,
                           **({"hyper_ptr": self.hyper.ptr, "scale_ptr": scales.ptr if scales is not None else None} if self.hyper is not None else {}))
        self.iter_offset += int(iters) * int(thin)
        if use_stats:
            self.stats_kept += int(iters)
        return out if keep else None

    def stats_sums(self) -> np.ndarray:
        """Chain-pooled sums `[7, p]` of the statistics window (`lr_stats_reduce`: a device reduction over the
        chains; only 7p doubles cross PCIe).  Sums of chain shards add: see distributed.reduce_stats."""
        if self.stats is None:
            raise ValueError("no statistics window: call enable_stats first")
        m = self.model
        piv = np.ascontiguousarray(self.pivot, dtype=np.float64)
        sums = np.empty((_lib.STATS_ROWS, m.p), dtype=np.float64)
        check(m._L.lr_stats_reduce(m.device, self.stats.ptr, self.C, m.p, self.stats_batch, self.stats_kept,
                                          piv.ctypes.data, sums.ctypes.data, self.stream))
        return sums

    def stats_summary(self) -> dict:
        """mean / sd / split-R-hat / batch-means ESS / MCSE of the window, from the device accumulators."""
        from .diagnostics import summary_from_sums
        return summary_from_sums(self.stats_sums(), self.C, self.stats_kept, self.stats_batch, self.pivot)

    def sync(self):
        check(self.model._L.lr_stream_sync(self.model.device, self.stream))

    def get_state(self):
        self.sync()
        return self.state.to_host().astype(np.float64)

    def get_ll(self):
        self.sync()
        return self.lp.to_host()

    def get_accepts(self):
        self.sync()
        return self.acc.to_host()

    def get_counters(self) -> np.ndarray:
        """NUTS: the per-chain counters `[C]` (fields of lr_nuts_counters: n_leapfrog, depth_sum, accept_stat_sum, divergent,
        max_depth_hits), summed over every launch of this chain set."""
        if self.counters is None:
            raise ValueError("counters exist for NUTS and Polya-Gamma chain sets only")
        self.sync()
        return self.counters.to_host()

    def nuts_info(self) -> dict:
        """NUTS: per-chain n_leapfrog, divergent, max_depth_hits, mean_depth and mean_accept_stat over the iterations run so far."""
        c = self.get_counters()
        n = max(self.iter_offset, 1)
        return {"n_leapfrog": c["n_leapfrog"].astype(np.int64), "divergent": c["divergent"].astype(np.int64),
                "max_depth_hits": c["max_depth_hits"].astype(np.int64), "mean_depth": c["depth_sum"] / n,
                "mean_accept_stat": c["accept_stat_sum"] / n}

    def pg_info(self) -> dict:
        """Polya-Gamma: per-chain proposals, series_terms and skipped (lr_pg_counters) over the iterations run so far, and the two
        ratios to rows x iterations (`proposals_per_draw`: theory <= 1.0009; skipped iterations draw nothing).  A horseshoe chain set
        adds `clamped` (lr_hs_counters)."""
        if self.kernel.kind not in ("pg", "hs"):
            raise ValueError("pg_info is for Polya-Gamma chain sets")
        c = self.get_counters()
        draws = np.maximum((self.iter_offset - c["skipped"].astype(np.int64)) * self.model.n, 1)
        info = {"proposals": c["proposals"].astype(np.int64), "series_terms": c["series_terms"].astype(np.int64),
                "skipped": c["skipped"].astype(np.int64), "proposals_per_draw": c["proposals"] / draws,
                "series_terms_per_draw": c["series_terms"] / draws}
        if self.kernel.kind == "hs":
            info["clamped"] = c["clamped"].astype(np.int64)
        return info

    def get_hyper(self) -> np.ndarray:
        """Horseshoe: the hyper-state `[C, 2p+2]` (lambda^2 `[p]`, nu `[p]`, tau^2, xi per chain), float64."""
        if self.hyper is None:
            raise ValueError("the hyper-state exists for horseshoe chain sets only")
        self.sync()
        return self.hyper.to_host()

    def set_hyper(self, hyper):
        """Horseshoe: replace the hyper-state; `[2p+2]` or `[C, 2p+2]`, every entry finite and in [1e-100, 1e100]."""
        if self.hyper is None:
            raise ValueError("the hyper-state exists for horseshoe chain sets only")
        h = np.ascontiguousarray(np.broadcast_to(np.asarray(hyper, dtype=np.float64), (self.C, 2 * self.model.p + 2)))
        if not np.all((h >= _lib.HS_MIN) & (h <= _lib.HS_MAX)):
            raise ValueError(f"every entry of the hyper-state must be finite and in [{_lib.HS_MIN:g}, {_lib.HS_MAX:g}]")
        self.sync()
        self.hyper.copy_from(h)

    # -- checkpoint / resume (the reference has none: a run is all-or-nothing).  Because the random
    # stream is counter-based, (state, threaded ll, iteration counter, seed, chain offset) IS the
    # complete sampler state: a resumed run continues bit-for-bit.
    def _fingerprint(self) -> dict:
        """What a resumed run must share with the saved one for the continuation to be bit-exact: model shape and
        arithmetic type, a hash of the data block, and the kernel's parameters."""
        m, k = self.model, self.kernel
        par = {name: np.broadcast_to(np.asarray(v, dtype=np.float64), ((m.p, m.p) if np.ndim(v) == 2 else (m.p,)) if np.ndim(v) else ()).copy()
               for name, v in sorted(k.params.items())}  # (a dense NUTS kernel's inv_metric [p, p] among them)
        return {"kind": k.kind, "n": np.int64(m.n), "p": np.int64(m.p), "dtype": np.dtype(m.np_dtype).name,
                "data_hash": m.data_hash, **{"param_" + name: v for name, v in par.items()}}

    def checkpoint(self) -> dict:
        self.sync()
        ck = {"state": self.state.to_host(), "ll": self.lp.to_host(), "accepts": self.acc.to_host(),
              "iter_offset": np.int64(self.iter_offset), "seed": np.uint64(self.seed),
              "chain_offset": np.int64(self.chain_offset), "plan_chains": np.int64(self.plan_chains),
              "plan_first": np.int64(self.plan_first), **self._fingerprint()}
        if self.counters is not None:  # NUTS / PG counters, field by field
            cn = self.counters.to_host()
            prefix, rec = _COUNTERS_BY_KIND[self.kernel.kind]
            ck.update({prefix + f: cn[f].copy() for f in rec.names})
        if self.hyper is not None:  # horseshoe: the scales are part of the sampler's state
            ck.update(hyper=self.hyper.to_host())
        if self.stats is not None:  # the statistics window travels with the run
            ck.update(stats=self.stats.to_host(), stats_batch=np.int64(self.stats_batch), stats_kept=np.int64(self.stats_kept),
                      stats_pivot=np.asarray(self.pivot, dtype=np.float64))
        return ck

    def save(self, path: str) -> str:
        """Write the checkpoint as an .npz archive; returns the path actually written (np.savez appends
        ".npz" to a name without it), so `ChainSet.resume(kernel, cs.save("ckpt"))` works."""
        path = str(path)
        if not path.endswith(".npz"):
            path += ".npz"
        np.savez(path, **self.checkpoint())
        return path

    @classmethod
    def resume(cls, kernel: "FusedKernel", ckpt, group: int = 0, mode: str = "auto", stream=None,
               precision: str = "auto") -> "ChainSet":
        if isinstance(ckpt, (str, bytes)) or hasattr(ckpt, "__fspath__"):
            path = str(ckpt)
            if not path.endswith(".npz"):
                path += ".npz"
            ckpt = dict(np.load(path, allow_pickle=False))
        if str(ckpt["kind"]) != kernel.kind:
            raise ValueError(f"checkpoint is for a {ckpt['kind']} kernel, got {kernel.kind}")
        # (a shard resumes as the shard of the same planned run: its chains keep the kernel variants they had)
        cs = cls(kernel, ckpt["state"], int(ckpt["seed"]), chain_offset=int(ckpt["chain_offset"]), ll=ckpt["ll"],
                 group=group, mode=mode, stream=stream, precision=precision,
                 plan_chains=int(ckpt["plan_chains"]) if "plan_chains" in ckpt else 0,
                 plan_first=int(ckpt["plan_first"]) if "plan_first" in ckpt else 0)
        want = cs._fingerprint()
        for key, val in want.items():
            if key not in ckpt:
                continue  # checkpoints written before the fingerprint existed carry only `kind`
            have = ckpt[key]
            same = np.array_equal(np.asarray(have), np.asarray(val)) if key.startswith("param_") else str(have) == str(val)
            if not same:
                raise ValueError(f"checkpoint does not match this kernel/model: {key} = {have!r} in the checkpoint, "
                                 f"{val!r} here (a resumed run would silently stop being the continuation)")
        cs.iter_offset = int(ckpt["iter_offset"])
        cs.acc.copy_from(np.asarray(ckpt["accepts"], dtype=np.uint32))
        if cs.counters is not None:
            prefix, rec = _COUNTERS_BY_KIND[kernel.kind]
            if prefix + rec.names[0] in ckpt:
                cn = np.zeros(cs.C, dtype=rec)
                for f in rec.names:
                    cn[f] = ckpt[prefix + f]
                cs.counters.copy_from(cn)
        if cs.hyper is not None:
            if "hyper" not in ckpt:
                raise ValueError("checkpoint of a horseshoe chain set without its hyper-state")
            cs.set_hyper(ckpt["hyper"])
        if "stats" in ckpt:
            st = np.asarray(ckpt["stats"], dtype=np.float64)
            cs.enable_stats(int(ckpt["stats_batch"]), st.shape[0], pivot=ckpt["stats_pivot"])
            cs.stats.copy_from(st)
            cs.stats_kept = int(ckpt["stats_kept"])
        return cs


def _auto_chunk(kernel: FusedKernel, C: int, thin: int, iters: int, evals_per_iter: float | None = None) -> int:
    """Kept samples per launch.  A launch is bounded to ~2e9 data-element visits per chain (a few
    hundred ms at Pima scale): short enough to report progress and to stay far from any watchdog,
    long enough that launch overhead is invisible.  Chunking never changes the samples.
    NUTS: `evals_per_iter` (leapfrog steps per iteration seen so far, the widest chain's) or, before any, the full tree's
    2^max_depth - 1."""
    if kernel.kind == "nuts":
        evals = evals_per_iter if evals_per_iter else 2 ** int(kernel.params["max_depth"]) - 1
    else:
        # (a Polya-Gamma sweep: n draws and n p (p + 1) / 2 multiply-adds -- priced as p / 2 + 8 passes over the data)
        evals = {"hmc": kernel.params.get("l", 1), "mala": 1, "ul": 1, "rwmh": 1, "pg": kernel.model.p / 2 + 8, "hs": kernel.model.p / 2 + 8}[kernel.kind]
    work_per_kept = max(1, int(thin * evals * kernel.model.n * kernel.model.p))
    return int(max(1, min(iters, 2_000_000_000 // work_per_kept)))


def _accumulator_class(keyword):
    """(class, its name with an article) of the accumulator `mcmc` takes as `keyword=`"""
    if keyword == "autocorr":
        from .autocorr import Autocorr
        return Autocorr, "an Autocorr"
    if keyword == "rank":
        from .rankdiag import RankDiagnostics
        return RankDiagnostics, "a RankDiagnostics"
    if keyword == "marginals":
        from .marginals import Marginals
        return Marginals, "a Marginals"
    if keyword == "covariance":
        from .covariance import Covariance
        return Covariance, "a Covariance"
    if keyword == "bridge":
        from .bridge import Bridge
        return Bridge, "a Bridge"
    if keyword == "check":
        from .ppc import PredictiveCheck
        return PredictiveCheck, "a PredictiveCheck"
    from .loo import PsisLoo
    return PsisLoo, "a PsisLoo"


def mcmc(init, kernel, thin=10, iters=10000, verb=True, *, seed=None, chunk=None, chain_offset=0, ll=None,
         group=0, mode="auto", return_info=False, summary_only=False, max_batches=16, precision="auto", plan_chains=0, plan_first=0,
         autocorr=None, rank=None, check=None, loo=None, bridge=None, covariance=None, marginals=None, predictive=None):
    """Run a chain (or C chains): `mat[i]` = state after (i+1)*thin iterations (fit-np-hmc.py:89-103).

    Fused kernels run on the device; `init` of shape [p] returns a float64 `[iters, p]` matrix
    like the reference, `[C, p]` returns `[iters, C, p]` in the model's dtype.  RWMH/MALA start
    with the threaded log-density at -inf as the reference does (fit-np-mala.py:82) unless
    `ll=` is given.  `seed=None` draws the Philox key from NumPy's global RNG, so
    `np.random.seed(s)` before the call makes a run reproducible, like the reference.

    `precision="auto"` (the DEFAULT) lets HMC's l - 1 gradient evaluations strictly inside a trajectory run in reduced precision where such
    a kernel exists -- on a float64 model too (float64 state, end points and Metropolis test; float32 / 16-bit force inside the
    trajectory, at any chain count): such a run is NOT step-for-step comparable with the reference; `precision="full"` is (every
    evaluation in the model's dtype).  INTEGRATION.md section 3b has the numbers.

    `summary_only=True` (fused kernels): no sample matrix at all -- the kept samples are folded into on-device
    running statistics and the call returns a dict (mean, sd, rhat, ess, mcse, accept_rate, ...): what the
    reference computes from the full matrix afterwards (fit-np-hmc.py:113-117, analyse.R:17-19).

    `precision` (HMC): "auto" (DEFAULT) lets the L - 1 interior leapfrog gradients of a trajectory run on the matrix
    pipe from 16-bit operands (bf16 pieces; IEEE half precision for wide models whose design fits it) where such a kernel exists (the end-point value + gradient and the Metropolis test stay in the model's dtype, so
    the sampler stays exact; the acceptance rate is the only thing that can move); "full" keeps every evaluation in the
    model's dtype (step-for-step comparable with the float64 reference); see include/logreg_hip.h LR_PREC_*.  float64 models
    follow the same policy with more kept exact: position, momentum, end points, kinetic energies and the Metropolis test are
    float64, only the force inside the trajectory comes from float32 / 16-bit operands (4 - 6 x the all-float64 rate).
    `predictive` (fused kernels): a `PosteriorPredictive` of the same model.  Every chunk's block of kept samples is folded into it ON
    THE DEVICE before the block is copied or freed -- with `summary_only=True` the block lives only that long and no sample matrix reaches
    the host; the returned dict gains `"predictive"`.  Chains, states, statistics and accept counts are those of the same call without it.
    `autocorr` (fused kernels): an `Autocorr` of the run's chain count, p and dtype.  Every chunk's block of kept samples is folded into
    it on the device, in time order, before the block is copied or freed (under `summary_only=True` the block lives only that long);
    the summary dict -- or, with `return_info=True`, the info dict -- gains `"autocorr": autocorr.result()` (Geyer ESS per chain and
    pooled, the pooled autocorrelation).  Chains, states, statistics and accept counts are those of the same call without it.
    `rank` (fused kernels): a `RankDiagnostics` of the run's chain count, p, dtype and device with room for `iters` more steps.  Every
    chunk's block of kept samples is stored in it on the device exactly where `autocorr` is fed; the summary dict -- or, with
    `return_info=True`, the info dict -- gains `"rank": rank.result()` (rank-normalised split-R-hat, bulk and tail ESS, exact median and
    5 % / 95 % order statistics).  Chains, states, statistics and accept counts are those of the same call without it.
    `marginals` (fused kernels): a `Marginals` of the run's chain count, p, dtype and device.  Every chunk's block of kept samples is
    folded into it on the device exactly where `autocorr` is; the summary dict -- or, with `return_info=True`, the info dict -- gains
    `"marginals": marginals.result()` (min/max, mean, variance, skewness, kurtosis, the histograms; `quantile`, `interval` and `hpd` of
    logreg_amd.marginals read quantiles and credible intervals off it).  Chains, states, statistics and accept counts are those of the
    same call without it.
    `covariance` (fused kernels): a `Covariance` of the run's chain count, p, dtype and device.  Every chunk's block of kept samples is
    folded into it on the device exactly where `marginals` is; the summary dict -- or, with `return_info=True`, the info dict -- gains
    `"covariance": covariance.result()` (cov, cor, the within- and between-chain matrices, the multivariate R-hat; `metric` of
    logreg_amd.covariance turns it into a diagonal `dmm` / `pre`).  Chains, states, statistics and accept counts are those of the same
    call without it.
    `loo` (fused kernels): a `PsisLoo` of the kernel's own model with `max_draws` >= the draws it already holds + iters x chains.  Every
    chunk's block of kept samples is appended to its log-likelihood matrix on the device where `predictive` is fed; the summary dict --
    or, with `return_info=True`, the info dict -- gains `"loo": loo.result()` (elpd_loo, p_loo, se, looic, the Pareto k-hat per
    observation).  Chains, states, statistics and accept counts are those of the same call without it.
    `bridge` (fused kernels): a `Bridge` of the kernel's own model with `max_draws` >= the draws it already holds + iters x chains.  Every
    chunk's block of kept samples becomes bridge-sampling terms on the device where `loo` is fed; the summary dict -- or, with
    `return_info=True`, the info dict -- gains `"bridge": bridge.result()` (logml, its standard error with n_eff = the number of draws;
    `bridge.result(n_eff=...)` afterwards takes the effective size from `autocorr`).  Chains, states, statistics and accept counts are
    those of the same call without it.
    `check` (fused kernels): a `PredictiveCheck` of the kernel's own model.  Every chunk's block of kept samples is replicated on the
    device where `predictive` is fed (draw index = the draws it already holds, time-major); the summary dict -- or, with
    `return_info=True`, the info dict -- gains `"check": check.result()` (per group the observed and replicated counts with their tail
    probabilities, the deviance check, the per-row frequency of ones).  Chains, states, statistics and accept counts are those of the same
    call without it.
    An `hsKernel` (the horseshoe Polya-Gamma sampler) reports what a `pgKernel` does, plus `clamped` and the final hyper-state `hyper`
    `[C, 2p+2]`; a sample-returning run with `return_info=True` adds the scales of the kept draws, `local_scale2` `[iters, C, p]`
    (lambda_j^2; 1 where unshrunk) and `global_scale2` `[iters, C]` (tau^2).  `bridge=` is refused: the evidence a `Bridge` computes is
    under the model's Gaussian prior, not the horseshoe.
    A `pgKernel` (the Polya-Gamma Gibbs sampler) has no accept count: `return_info=True` and `summary_only=True` report its per-chain
    counters instead (`proposals`, `series_terms`, `skipped` and the two ratios of `ChainSet.pg_info`); `accept_rate` is the share of
    sweeps that were not skipped.
    `plan_chains`, `plan_first`: chain count to plan the kernel variant for and the global id of that run's first chain (a shard of
    a larger run passes the whole run's: its chains then run on the variants they have in the whole run, bit for bit).
    """
    # the accumulators given: refused in the order of the keywords here, fed and reported in the order of `accs`
    given = {name: acc for name, acc in (("predictive", predictive), ("autocorr", autocorr), ("rank", rank), ("marginals", marginals), ("covariance", covariance), ("loo", loo),
                                              ("bridge", bridge), ("check", check))
             if acc is not None}
    accs = [(name, given[name]) for name in ("autocorr", "rank", "marginals", "covariance", "loo", "bridge", "check", "predictive") if name in given]
    if not isinstance(kernel, FusedKernel):
        for name in given:
            raise ValueError(f"{name}= needs a fused kernel (the closures of a LogReg)")
        return _mcmc_generic(init, kernel, thin, iters, verb)
    if kernel.kind == "hs" and bridge is not None:
        raise ValueError("bridge= is refused with an hsKernel: the evidence a Bridge computes is under the model's Gaussian prior, not "
                         "the horseshoe the chains sample from")
    if predictive is not None and getattr(predictive, "model", None) is not kernel.model:
        raise ValueError("predictive= must be a PosteriorPredictive of the kernel's own model")
    init = np.asarray(init, dtype=np.float64)
    single = init.ndim == 1
    for name, acc in given.items():  # refused before anything runs
        if name != "predictive":
            cls, a_cls = _accumulator_class(name)
            if not isinstance(acc, cls):
                raise ValueError(f"{name}= must be {a_cls}; got {type(acc).__name__}")
            acc.check_run(np.atleast_2d(init).shape[0], kernel.model, iters)

    def fold(out):  # a chunk's block of kept samples, still on the device
        for _, acc in accs:
            acc.update(out, stream=cs.stream)

    def attach(d, info=False):  # the results; predictive goes into a summary as the object itself and into no info dict
        for name, acc in accs:
            if name != "predictive":
                d[name] = acc.result()
            elif not info:
                d[name] = acc
    if seed is None:
        seed = int(np.random.randint(0, 2**31 - 1))
    cs = ChainSet(kernel, init, seed, chain_offset=chain_offset, ll=ll, group=group, mode=mode, precision=precision,
                  plan_chains=plan_chains, plan_first=plan_first)
    m = kernel.model
    nuts = kernel.kind == "nuts"
    auto = chunk is None
    if chunk is None:
        chunk = _auto_chunk(kernel, cs.C, thin, iters)

    def rechunk():  # NUTS: from the counters of the chunks so far (the widest chain bounds a lockstep launch)
        if nuts and auto and cs.iter_offset > 0:
            return _auto_chunk(kernel, cs.C, thin, iters, float(cs.get_counters()["n_leapfrog"].max()) / cs.iter_offset)
        return chunk
    if summary_only:
        from .diagnostics import choose_batches
        batch, slots = choose_batches(iters, max_batches)
        cs.enable_stats(batch, slots)
        if verb:
            print(str(iters) + " iterations")
        done = 0
        while done < iters:
            k = min(chunk, iters - done)
            if not accs:
                cs.advance(k, thin, keep=False)
                cs.sync()
            else:  # the chunk's samples exist on the device just long enough to be folded into the accumulator(s)
                out = cs.advance(k, thin, keep=True)
                fold(out)
                cs.sync()
                out.free()
            done += k
            chunk = rechunk()
            if verb:
                print(str(done), end=" ", flush=True)
        if verb:
            print("\nDone.", flush=True)
        res = cs.stats_summary()
        if nuts:  # the mean acceptance statistic in place of an acceptance rate
            ni = cs.nuts_info()
            res.update(ni, accept_rate=float(np.mean(ni["mean_accept_stat"])))
        elif kernel.kind in ("pg", "hs"):  # a Gibbs sweep always moves, unless it was skipped
            gi = cs.pg_info()
            res.update(gi, accept_rate=float(1.0 - gi["skipped"].sum() / (cs.C * iters * thin)))
            if kernel.kind == "hs":
                res.update(hyper=cs.get_hyper())
        else:
            res.update(accept_rate=float(cs.get_accepts().sum() / (cs.C * iters * thin)))
        res.update(batch=batch, seed=seed, plan=cs.plan(), state=cs.get_state())
        attach(res)
        return res
    mat = np.empty((iters, cs.C, m.p), dtype=m.np_dtype)
    want_scales = kernel.kind == "hs" and return_info
    scale_mat = np.empty((iters, cs.C, m.p + 1), dtype=np.float64) if want_scales else None
    if verb:
        print(str(iters) + " iterations")
    done = 0
    while done < iters:
        k = min(chunk, iters - done)
        sc = DeviceArray(m.device, (k, cs.C, m.p + 1), np.float64) if want_scales else None
        out = cs.advance(k, thin, keep=True, scales=sc)
        fold(out)
        cs.sync()
        mat[done:done + k] = out.to_host()
        out.free()
        if sc is not None:
            scale_mat[done:done + k] = sc.to_host()
            sc.free()
        done += k
        chunk = rechunk()
        if verb:
            print(str(done), end=" ", flush=True)
    if verb:
        print("\nDone.", flush=True)
    res = mat[:, 0, :].astype(np.float64) if single else mat
    if return_info:
        if nuts:  # per chain: n_leapfrog, divergent, max_depth_hits, mean_depth, mean_accept_stat
            info = {"state": cs.get_state(), "seed": seed, "plan": cs.plan(), "iterations": iters * thin, **cs.nuts_info()}
        elif kernel.kind in ("pg", "hs"):  # per chain: proposals, series_terms, skipped and the two ratios
            info = {"state": cs.get_state(), "seed": seed, "plan": cs.plan(), "iterations": iters * thin, **cs.pg_info()}
            if kernel.kind == "hs":
                local = scale_mat[:, :, :m.p]
                info.update(hyper=cs.get_hyper(), local_scale2=local[:, 0] if single else local, global_scale2=scale_mat[:, 0, m.p] if single else scale_mat[:, :, m.p])
        else:
            info = {"accepts": cs.get_accepts(), "state": cs.get_state(), "ll": cs.get_ll(), "seed": seed,
                    "plan": cs.plan(), "iterations": iters * thin}
        if getattr(kernel, "proposal", None):  # RWMH: how the proposal was recognised ("rwProposal" | "probed": mhKernel)
            info["proposal"] = kernel.proposal
        attach(info, info=True)
        return res, info
    return res


def _mcmc_generic(init, kernel, thin, iters, verb):
    """The reference's driver for arbitrary Python kernels.  Kernels built by the generic
    `mhKernel` / `malaKernel` thread `ll` (fit-np-mala.py:80-95); `hmcKernel` / `ulKernel`
    kernels take and return the state only (fit-np-hmc.py:89-103)."""
    import inspect
    p = len(init)
    mat = np.zeros((iters, p))
    x = init
    try:
        nparams = len(inspect.signature(kernel).parameters)
    except (TypeError, ValueError):
        nparams = 1
    threaded = nparams >= 2
    ll = -np.inf
    if verb:
        print(str(iters) + " iterations")
    for i in range(iters):
        if verb:
            print(str(i), end=" ", flush=True)
        for j in range(thin):
            if threaded:
                x, ll = kernel(x, ll)
            else:
                x = kernel(x)
        mat[i, :] = x
    if verb:
        print("\nDone.", flush=True)
    return mat
