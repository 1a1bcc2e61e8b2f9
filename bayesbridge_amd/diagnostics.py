"""MCMC output diagnostics used by the reference's benchmark protocol.

The reference publishes effective sample size (ESS) and ESS per second (ESR) per
coefficient, computed by ``coda::effectiveSize`` (Code/R/PublicBenchmark.R:112-134,
``sum.stat``).  ``effective_size`` restates coda's estimator: the spectral density of each
trace at frequency 0 from an autoregressive fit (``spectrum0.ar``: ``ar()`` by Yule-Walker
with the order chosen by AIC up to ``10 log10(n)``), and ESS = n var(x) / spec0.
Pure numpy, host-side post-processing of the traces the sampler returns.
"""
from __future__ import annotations

import numpy as np

__all__ = ["effective_size", "sum_stat", "rhat", "sum_stat_chains", "effective_size_from_acov",
           "rhat_from_moments", "sum_stat_from_summary", "default_maxlag",
           "quantiles_from_bins"]


def default_maxlag(n: int) -> int:
    """coda's largest autoregressive order for n samples: floor(min(n - 1, 10 log10 n))."""
    return max(0, int(np.floor(min(n - 1, 10 * np.log10(n)))))


def _acov(x: np.ndarray, maxlag: int) -> np.ndarray:
    """Biased autocovariances (divisor n) at lags 0..maxlag, as R's acf(type="covariance")."""
    n = x.shape[0]
    xc = x - x.mean()
    m = 1 << int(np.ceil(np.log2(2 * n)))
    f = np.fft.rfft(xc, m)
    ac = np.fft.irfft(f * np.conj(f), m)[: maxlag + 1] / n
    return ac


def _ar_yw_aic(x: np.ndarray, order_max: int | None = None):
    """R's ar.yw(x, aic = TRUE): Levinson-Durbin on the sample autocovariances, the order
    with the smallest AIC = n log(var_k) + 2 k, var.pred = var_k n / (n - (k + 1)).
    Returns (coefficients, var.pred)."""
    n = x.shape[0]
    if order_max is None:
        order_max = default_maxlag(n)
    order_max = max(0, min(order_max, n - 1))
    return _ar_from_acov(n, _acov(x, order_max))


def _ar_from_acov(n: int, r: np.ndarray):
    """_ar_yw_aic from the biased autocovariances r[0..order_max] of n samples."""
    order_max = max(0, min(len(r) - 1, n - 1))
    if r[0] <= 0:
        return np.zeros(0), 0.0
    # Levinson-Durbin recursion
    best_k, best_aic = 0, n * np.log(r[0])
    phi = np.zeros(0)
    v = r[0]
    coefs = {0: (np.zeros(0), r[0])}
    for k in range(1, order_max + 1):
        acc = r[k] - (phi @ r[k - 1:0:-1] if k > 1 else 0.0)
        kappa = acc / v
        phi = np.concatenate([phi - kappa * phi[::-1], [kappa]])
        v = v * (1.0 - kappa * kappa)
        if v <= 0:
            break
        coefs[k] = (phi.copy(), v)
        aic = n * np.log(v) + 2 * k
        if aic < best_aic:
            best_aic, best_k = aic, k
    ar, v = coefs[best_k]
    var_pred = v * n / (n - (best_k + 1))
    return ar, var_pred


def _ess(n: int, var: float, ar: np.ndarray, var_pred: float) -> float:
    """n var / spectrum0 of the fitted autoregression, 0 where the spectral estimate is 0."""
    spec = var_pred / (1.0 - ar.sum()) ** 2
    return 0.0 if spec == 0 else n * var / spec


def effective_size(x) -> np.ndarray:
    """coda::effectiveSize of each column of x (samples x parameters; a 1-D trace is one
    parameter): n var(x) / spectrum0.ar(x), 0 where the spectral estimate is 0."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    n = x.shape[0]
    out = np.zeros(x.shape[1])
    for j in range(x.shape[1]):
        col = x[:, j]
        if np.all(col == col[0]):
            out[j] = 0.0
            continue
        out[j] = _ess(n, col.var(ddof=1), *_ar_yw_aic(col))
    return out


def effective_size_from_acov(n: int, acov) -> np.ndarray:
    """effective_size with the autocovariances given: acov[..., k] is the biased
    autocovariance (divisor n, centred at the trace's mean) at lag k = 0..L of a trace of n
    samples, L the largest autoregressive order tried (coda tries default_maxlag(n)).  The
    unbiased variance is acov[..., 0] n / (n - 1); a zero-variance trace returns 0."""
    acov = np.asarray(acov, dtype=np.float64)
    flat = acov.reshape(-1, acov.shape[-1])
    out = np.zeros(flat.shape[0])
    for j, r in enumerate(flat):
        if r[0] == 0:
            continue
        if not np.isfinite(r[0]):
            out[j] = np.nan
            continue
        out[j] = _ess(n, r[0] * n / (n - 1), *_ar_from_acov(n, r))
    return out.reshape(acov.shape[:-1])


def sum_stat(beta, runtime: float):
    """PublicBenchmark.R:112-134 (sum.stat) without the posterior summaries' formatting:
    per-coefficient ESS and ESR (= ESS / runtime), with their min / median / max."""
    ess = effective_size(beta)
    esr = ess / runtime if runtime > 0 else np.full_like(ess, np.inf)
    return {"ess": ess, "esr": esr,
            "ess_summary": (float(ess.min()), float(np.median(ess)), float(ess.max())),
            "esr_summary": (float(esr.min()), float(np.median(esr)), float(esr.max())),
            "runtime": runtime}


def rhat(x) -> np.ndarray:
    """Split potential scale reduction factor of K chains: x is (K, M) or (K, M, P) and the
    result a scalar array or (P,).  Each chain is split in halves (the middle draw dropped
    when M is odd), giving 2K sequences of length n; with W the mean within-sequence variance
    and B / n the variance of the sequence means, R-hat = sqrt(((n - 1) / n W + B / n) / W)
    (Gelman et al., Bayesian Data Analysis 3rd ed., s11.4)."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim not in (2, 3):
        raise ValueError("rhat: x must be (chains, draws) or (chains, draws, parameters)")
    n = x.shape[1] // 2
    if n < 2:
        raise ValueError("rhat: at least four draws per chain are needed")
    seq = np.concatenate([x[:, :n], x[:, x.shape[1] - n:]], axis=0)  # (2K, n[, P])
    return _rhat_of_sequences(n, seq.mean(axis=1), seq.var(axis=1, ddof=1))


def _rhat_of_sequences(n: int, means, variances) -> np.ndarray:
    """R-hat from the means and unbiased variances (sequences first) of sequences of length n."""
    W = variances.mean(axis=0)
    B_over_n = means.var(axis=0, ddof=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.sqrt((n - 1) / n + B_over_n / W)


def rhat_from_moments(n: int, hmean, hvar) -> np.ndarray:
    """rhat from the moments of the halves: n is the number of draws per chain, hmean and hvar
    are (K, 2) or (K, P, 2), the mean and unbiased variance of the first and of the last
    n // 2 draws of each chain."""
    hmean = np.asarray(hmean, dtype=np.float64)
    hvar = np.asarray(hvar, dtype=np.float64)
    if hmean.ndim not in (2, 3) or hmean.shape[-1] != 2 or hvar.shape != hmean.shape:
        raise ValueError("rhat_from_moments: hmean and hvar must be (chains[, parameters], 2)")
    if n // 2 < 2:
        raise ValueError("rhat: at least four draws per chain are needed")
    # the 2K sequences in rhat's order: every chain's first half, then every chain's second
    seq = lambda a: np.concatenate([a[..., 0], a[..., 1]], axis=0)  # noqa: E731
    return _rhat_of_sequences(n // 2, seq(hmean), seq(hvar))


def sum_stat_chains(beta, runtime: float):
    """sum_stat for K chains: beta is (K, M, P) (a (K, M) trace is one coefficient).  Per
    coefficient: the pooled posterior mean and sd, the ESS summed over the chains (each
    chain's coda effective size), ESS per second of the batch's runtime, and split R-hat."""
    beta = np.asarray(beta, dtype=np.float64)
    if beta.ndim == 2:
        beta = beta[:, :, None]
    K, M, P = beta.shape
    ess = np.zeros(P)
    for c in range(K):
        ess += effective_size(beta[c])
    esr = ess / runtime if runtime > 0 else np.full_like(ess, np.inf)
    pooled = beta.reshape(K * M, P)
    return {"mean": pooled.mean(axis=0), "sd": pooled.std(axis=0, ddof=1), "ess": ess,
            "esr": esr, "rhat": rhat(beta),
            "ess_summary": (float(ess.min()), float(np.median(ess)), float(ess.max())),
            "esr_summary": (float(esr.min()), float(np.median(esr)), float(esr.max())),
            "runtime": runtime, "chains": K}


def sum_stat_from_summary(summary, runtime: float):
    """sum_stat_chains from the per-chain moments a summary call returns, without the traces:
    summary has nsamp, mean and var (K, Q), acov (K, Q, L + 1), hmean and hvar (K, Q, 2)
    (optionally p: only the first p parameters, the coefficients, are summarised).  The pooled
    mean and sd merge the chains' moments (Chan et al.), the ESS is each chain's
    effective_size_from_acov summed, R-hat is rhat_from_moments."""
    M = int(summary["nsamp"])
    P = int(summary.get("p", np.asarray(summary["mean"]).shape[1]))
    mean = np.asarray(summary["mean"], dtype=np.float64)[:, :P]
    var = np.asarray(summary["var"], dtype=np.float64)[:, :P]
    acov = np.asarray(summary["acov"], dtype=np.float64)[:, :P]
    K = mean.shape[0]
    ess = effective_size_from_acov(M, acov).sum(axis=0)
    esr = ess / runtime if runtime > 0 else np.full_like(ess, np.inf)
    pooled = mean.mean(axis=0)  # equal chain lengths
    m2 = ((M - 1) * var).sum(axis=0) + M * ((mean - pooled) ** 2).sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        sd = np.sqrt(m2 / (K * M - 1))
    if M // 2 >= 2:
        r = rhat_from_moments(M, np.asarray(summary["hmean"])[:, :P],
                              np.asarray(summary["hvar"])[:, :P])
    else:
        r = np.full(P, np.nan)
    return {"mean": pooled, "sd": sd, "ess": ess, "esr": esr, "rhat": r,
            "ess_summary": (float(ess.min()), float(np.median(ess)), float(ess.max())),
            "esr_summary": (float(esr.min()), float(np.median(esr)), float(esr.max())),
            "runtime": runtime, "chains": K}


def quantiles_from_bins(probs, centre, zlo, zhi, below, inbin, counts):
    """Point estimates of pooled quantiles from the device's bin selection (the quantile keys
    of ``bridge_reg_stb_chains_summary``): for parameter q and probability pi, with N =
    counts[q, 0] and the rank k = min(N, max(1, ceil(pi N))) (R's type-1 quantile), the k-th
    smallest draw lies in [centre + zlo, centre + zhi], a bin that holds ``inbin`` draws above
    ``below`` lower ones; the estimate interpolates by rank inside it,
    centre + zlo + (k - below - 1/2) / inbin (zhi - zlo), and is the finite edge in an overflow
    bin.  Returns quantile, quantile_lo, quantile_hi (Q x nprobs; NaN where N = 0) and
    prob_pos, prob_neg (Q: the shares of draws > 0 and < 0 among the N that are not NaN)."""
    probs = np.atleast_1d(np.asarray(probs, dtype=np.float64))
    centre = np.asarray(centre, dtype=np.float64)[:, None]
    zlo, zhi = np.asarray(zlo, dtype=np.float64), np.asarray(zhi, dtype=np.float64)
    below, inbin = np.asarray(below, dtype=np.float64), np.asarray(inbin, dtype=np.float64)
    counts = np.asarray(counts, dtype=np.float64)
    N = counts[:, :1]
    k = np.minimum(N, np.maximum(1.0, np.ceil(probs[None, :] * N)))
    with np.errstate(invalid="ignore", divide="ignore"):
        frac = (k - below - 0.5) / inbin
        est = zlo + frac * (zhi - zlo)
        est = np.where(np.isinf(zlo), zhi, np.where(np.isinf(zhi), zlo, est))
        est = np.where(N > 0, est, np.nan)
        n1 = np.where(counts[:, 0] > 0, counts[:, 0], np.nan)
        out = {"quantile": centre + est, "quantile_lo": centre + zlo, "quantile_hi": centre + zhi,
               "prob_neg": counts[:, 2] / n1, "prob_pos": counts[:, 3] / n1}
    return out
