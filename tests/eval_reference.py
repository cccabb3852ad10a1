"""An independent reference of the model closures -- ll, lprior, lpost, glp -- and of the negative Hessian, written from
include/logreg_hip.h alone, that stays exact where |t_i| = |xs_i . beta| is large (the oracle keeps the reference's naive
log(1 + exp(.)) and returns -inf once t < -709: it cannot judge that regime).

    xs_i = (2 y_i - 1) x_i          t_i = xs_i . beta          s_i = sum_j |xs_ij beta_j|
    l_i  = min(t_i, 0) - log1p(exp(-|t_i|))                    ll     = sum_i l_i
    w_i  = sigma(-t_i)  (sign-symmetric: e / (1 + e) for t > 0, 1 / (1 + e) otherwise, e = exp(-|t_i|))
    q_i  = w_i (1 - w_i)
    lprior = sum_j -(beta_j / sd_j)^2 / 2 - log sqrt(2 pi) - log sd_j
    glp_j  = sum_i w_i xs_ij - beta_j / sd_j^2                 H = X^T diag(q) X + diag(1 / sd^2)

Arithmetic: every product x_ij beta_j is split exactly in two doubles (Dekker) and t_i is their sum by math.fsum, taken twice:
a head and a residual, which together make the numpy.longdouble t_i and more.  Every sum over rows is math.fsum over terms held as
two doubles each.  The row terms l_i, w_i, q_i themselves are carried as two doubles as well, from 40-digit `decimal` arithmetic on
head + residual: glp and H are sums that cancel (by 1e5 on some coordinates of the cases), and longdouble row terms -- 1e-19 each --
leave such a sum short of the 1e-15 relative that tests/test_eval_regimes_cpu.py asks of it against mpmath at 50 digits.
The reference is computed on the data the MODEL holds: a float32 model's X and beta are rounded to float32 first.

The error bounds of the device paths are stated here, once (`bounds`); `emulate_f32` is the same model in plain sequential float32
NumPy, in the two value forms the float32 kernels use, and exists only to validate those bounds without a GPU.
"""
import decimal
import math

import numpy as np

LD = np.longdouble
D = decimal.Decimal
CTX = decimal.Context(prec=40, Emax=decimal.MAX_EMAX, Emin=decimal.MIN_EMIN)
U = {"float32": 2.0 ** -24, "float64": 2.0 ** -53}
# the project's own relative constants (tests/test_gpu_fullsize.py: test_model_closures_match_the_reference_at_other_shapes)
R = {"float32": 2e-6, "float64": 1e-11}
HALF_LOG_2PI = D("0.918938533204672741780329736405617639861398")
WANT = ("ll", "lprior", "lpost", "glp")


def held(a, dtype):
    """`a` as a model of `dtype` holds it, as float64."""
    a = np.asarray(a, dtype=np.float64)
    return a.astype(np.float32).astype(np.float64) if dtype == "float32" else a.copy()


def _two_prod(a, b):
    """a * b = hi + lo exactly (Veltkamp / Dekker; no overflow or underflow at the sizes used here)."""
    hi = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return hi, ((ah * bh - hi) + ah * bl + al * bh) + al * bl


def _pair(v):
    """A Decimal as two doubles (values below the double range give zeros: the comparisons have an absolute floor)."""
    hi = float(v)
    return hi, float(CTX.subtract(v, D(hi)))


def logits(xs, beta):
    """Head and residual of t [C, n] (two float64 arrays) and s [C, n] of signed rows xs [n, p] and beta [C, p]."""
    hi, lo = _two_prod(xs[None, :, :], beta[:, None, :])
    both = np.concatenate([hi, lo], axis=2)
    C, n, _ = both.shape
    th, tl = np.empty((C, n)), np.empty((C, n))
    for c in range(C):
        for i in range(n):
            row = both[c, i].tolist()
            th[c, i] = head = math.fsum(row)
            tl[c, i] = math.fsum(row + [-head])
    return th, tl, np.abs(hi).sum(axis=2)


def row_terms(th, tl):
    """l_i, w_i = sigma(-t_i), q_i = w_i (1 - w_i), each as (head, residual) float64 arrays shaped like th."""
    out = np.empty((6,) + th.shape)
    flat = out.reshape(6, -1)
    one, tiny = D(1), D("1e-25")
    for k, (a, b) in enumerate(zip(th.ravel().tolist(), tl.ravel().tolist())):
        t = CTX.add(D(a), D(b))
        e = CTX.exp(t.copy_abs().copy_negate())  # (copy_*: the unary operators would round to the default context)
        s = CTX.add(one, e)
        # log1p(e): below 1e-25 the series e - e^2 / 2 is exact to 40 digits where ln(1 + e) would have rounded e away
        l1p = CTX.ln(s) if e > tiny else CTX.subtract(e, CTX.multiply(CTX.multiply(e, e), D("0.5")))
        r = CTX.divide(one, s)
        w = CTX.multiply(e, r) if t > 0 else r
        flat[0, k], flat[1, k] = _pair(CTX.subtract(min(t, D(0)), l1p))
        flat[2, k], flat[3, k] = _pair(w)
        flat[4, k], flat[5, k] = _pair(CTX.multiply(CTX.multiply(e, r), r))
    return out


def _fsum(*arrays):
    return math.fsum(v for a in arrays for v in np.asarray(a, dtype=np.float64).ravel().tolist())


def reference(X, y, prior_sd, beta, dtype="float64", hessian=False, round_beta=True):
    """The closures at beta [C, p] for a model of `dtype`: dict of float64 arrays ll, lprior, lpost [C], glp [C, p], t, s, q [C, n]
    (and H [C, p, p] with hessian=True), plus what the bounds need: xs, beta, prior_sd as used, const = lprior(0).
    round_beta=False: beta stays float64 over rounded rows (lr_hessian takes a host double beta whatever the model's dtype)."""
    X = held(X, dtype)
    y = np.asarray(y, dtype=np.float64)
    sd = np.asarray(prior_sd, dtype=np.float64)
    beta_all = np.atleast_2d(held(beta, dtype) if round_beta else np.asarray(beta, dtype=np.float64))
    beta, inverse = np.unique(beta_all, axis=0, return_inverse=True)  # (chains of one case repeat parameter vectors)
    inverse = np.asarray(inverse).ravel()
    xs = (2.0 * y - 1.0)[:, None] * X
    C, p = beta.shape
    n = xs.shape[0]
    th, tl, s = logits(xs, beta)
    lh, ll_, wh, wl, qh, ql = row_terms(th, tl)
    sdd = [D(v) for v in sd.tolist()]
    cterms = np.array([_pair(CTX.subtract(HALF_LOG_2PI.copy_negate(), CTX.ln(v))) for v in sdd])  # [p, 2]
    out = {k: np.empty(C) for k in ("ll", "lprior", "lpost")}
    out["glp"] = np.empty((C, p))
    if hessian:
        out["H"] = np.empty((C, p, p))
        ivar = [_pair(CTX.divide(D(1), CTX.multiply(v, v))) for v in sdd]
    for c in range(C):
        bd = [D(v) for v in beta[c].tolist()]
        quad = np.array([_pair(CTX.multiply(CTX.power(CTX.divide(b, v), 2), D("-0.5"))) for b, v in zip(bd, sdd)])
        pull = np.array([_pair(CTX.divide(b, CTX.multiply(v, v)).copy_negate()) for b, v in zip(bd, sdd)])  # -beta_j / sd_j^2
        out["ll"][c] = _fsum(lh[c], ll_[c])
        out["lprior"][c] = _fsum(quad, cterms)
        out["lpost"][c] = _fsum(lh[c], ll_[c], quad, cterms)
        g_hi, g_lo = _two_prod(wh[c][:, None], xs)
        g_rest = wl[c][:, None] * xs
        for j in range(p):
            out["glp"][c, j] = _fsum(g_hi[:, j], g_lo[:, j], g_rest[:, j], pull[j])
        if hessian:
            for a in range(p):
                xx_hi, xx_lo = _two_prod(xs[:, a:a + 1], xs[:, a:])  # row a of the upper triangle, [n, p - a]
                h_hi, h_lo = _two_prod(qh[c][:, None], xx_hi)
                rest = qh[c][:, None] * xx_lo + ql[c][:, None] * xx_hi
                cols = np.concatenate([h_hi, h_lo, rest]).T.tolist()
                cols[0] += list(ivar[a])
                for k, col in enumerate(cols):
                    out["H"][c, a, a + k] = out["H"][c, a + k, a] = math.fsum(col)
    t = (th.astype(LD) + tl.astype(LD)).astype(np.float64)
    out.update(t=t, s=s, q=qh)
    out = {k: v[inverse] for k, v in out.items()}
    out.update(xs=xs, beta=beta_all, prior_sd=sd, const=_fsum(cterms))
    return out


# ------------------------------------------------------------------------------------------------
# error bounds of a device path computing in `dtype`, from the inputs alone
def bounds(ref, dtype, pad_rows=0):
    """dict of tolerances: ll, lprior, lpost [C], glp [C, p]; u the unit roundoff and r the relative constant of `dtype`.
        delta_i = (p + 1) u s_i                                      worst-case error of the dot product
        w+_i    = sigma(-(|t_i| - delta_i)+ sign t_i),  q+_i = w (1 - w) at (|t_i| - delta_i)+
        ll      r |ll| + sum_i [ w+_i delta_i + 2 u max(t_i, 0) ]    (the last term: the documented cancellation of
                                                                      ts - log2(1 + 2^ts), an absolute ulp(ts) per row)
        lprior  r (|const| + sum_j beta_j^2 / sd_j^2 / 2)
        lpost   the sum of the two
        glp_j   r sum_i |x_ij| + sum_i |x_ij| q+_i delta_i + r |beta_j| / sd_j^2
    pad_rows (register-resident rows: lanes x rows per lane - n): the zero rows that fill the layout each add log sigma(0) = -log 2 to their
    lane's sum, which value_fixup() takes back at the end.  Subtracting 1 (log2 units) is exact except where the sum crosses a binade (2 u
    pad per lane in all); the scaling to nats, the fix-up's own product and its addition round once each at that magnitude: the term
    6 u log 2 pad_rows on ll, absent from the bound above, which knows of no padding (n = 1 on 16 lanes x 13 rows: 207 such rows)."""
    u, r = U[dtype], R[dtype]
    t, s, xs, beta, sd = ref["t"], ref["s"], ref["xs"], ref["beta"], ref["prior_sd"]
    p = xs.shape[1]
    delta = (p + 1) * u * s
    e = np.exp(-np.maximum(np.abs(t) - delta, 0.0))
    wplus = np.where(t > 0, e / (1 + e), 1 / (1 + e))
    qplus = e / ((1 + e) * (1 + e))
    ax = np.abs(xs)
    tol = {"ll": r * np.abs(ref["ll"]) + np.sum(wplus * delta + 2 * u * np.maximum(t, 0.0), axis=1) + 6 * u * math.log(2) * pad_rows,
           "lprior": r * (abs(ref["const"]) + 0.5 * np.sum(beta ** 2 / sd ** 2, axis=1)),
           "glp": r * ax.sum(axis=0)[None, :] + (qplus * delta) @ ax + r * np.abs(beta) / sd ** 2}
    tol["lpost"] = tol["ll"] + tol["lprior"]
    return tol


def bound_hessian(ref):
    """tol_H[a, c] = sum_i |x_ia x_ic| (1e-12 q_i + 0.1 delta_i), delta_i with u = 2^-53 (lr_hessian computes in float64 whatever the
    model's dtype); 0.1 bounds |dq / dt|.  [C, p, p].
    On the diagonal the prior's 1 / sd_a^2 is added, which the sum over rows above knows nothing of: sd_a^2, its reciprocal and the addition
    round once each, the term 4 2^-53 H_aa (sd = 1e-2 over a column of zeros: H_aa = 1e4 exactly in the reference, and no row term at all)."""
    xs, p = ref["xs"], ref["xs"].shape[1]
    ax = np.abs(xs)
    wgt = 1e-12 * ref["q"] + 0.1 * (p + 1) * U["float64"] * ref["s"]
    tol = np.einsum("ci,ia,ib->cab", wgt, ax, ax)
    idx = np.arange(p)
    tol[:, idx, idx] += 4 * U["float64"] * np.abs(ref["H"][:, idx, idx])
    return tol


def ratios(got, ref, tol, want=WANT):
    """Largest |got - ref| / tol per output (0 / 0 counts as 0: an exactly reproduced value under a zero bound)."""
    out = {}
    for k in want:
        err = np.abs(np.asarray(got[k], dtype=np.float64) - ref[k])
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(err == 0, 0.0, err / tol[k])
        out[k] = float(np.max(q)) if np.all(np.isfinite(np.asarray(got[k], dtype=np.float64))) else float("inf")
    return out


# ------------------------------------------------------------------------------------------------
# float32 mode: the same model in plain sequential float32 NumPy (CPU validation of the bounds only)
def emulate_f32(X, y, prior_sd, beta, form):
    """form = "log1p": l = min(t, 0) - log1p(exp(-|t|)) (the scalar / packed row form); form = "log2": ts = t log2(e) with log2(e) folded
    into beta, clamped at 100, l = ln2 (ts - log2(1 + 2^ts)) (the row-pair and matrix-core form).  The weight is 1 / (1 + exp(t)) in
    both, an overflowing exponential giving 0.  Every sum runs in index order in float32."""
    f = np.float32
    xs = ((2.0 * np.asarray(y, dtype=np.float64) - 1.0)[:, None] * np.asarray(X, dtype=np.float64)).astype(f)
    b = np.atleast_2d(np.asarray(beta, dtype=np.float64)).astype(f)
    sd = np.asarray(prior_sd, dtype=np.float64)
    iv = (1.0 / sd ** 2).astype(f)
    const = f(np.sum(-float(HALF_LOG_2PI) - np.log(sd)))
    C, p = b.shape
    n = xs.shape[0]
    bs = b * f(1.44269504088896341) if form == "log2" else b
    ts = np.zeros((C, n), dtype=f)
    for j in range(p):
        ts = ts + bs[:, j:j + 1] * xs[None, :, j]
    with np.errstate(over="ignore"):
        if form == "log2":
            tc = np.minimum(ts, f(100.0))
            val = tc - np.log2(f(1.0) + np.exp2(tc))
            w = f(1.0) / (f(1.0) + np.exp2(ts))
        else:
            val = np.minimum(ts, f(0.0)) - np.log1p(np.exp(-np.abs(ts)))
            w = f(1.0) / (f(1.0) + np.exp(ts))
    ll = np.zeros(C, dtype=f)
    g = np.zeros((C, p), dtype=f)
    for i in range(n):
        ll = ll + val[:, i]
        g = g + w[:, i:i + 1] * xs[i][None, :]
    if form == "log2":
        ll = ll * f(0.693147180559945309)
    quad = np.zeros(C, dtype=f)
    for j in range(p):
        quad = quad + b[:, j] * b[:, j] * iv[j]
    lprior = const - f(0.5) * quad
    assert ll.dtype == f and lprior.dtype == f and g.dtype == f and ts.dtype == f and val.dtype == f and w.dtype == f
    return {"ll": ll, "lprior": lprior, "lpost": ll + lprior, "glp": g - b * iv[None, :]}
