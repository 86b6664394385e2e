"""Float64 restatement of the GGD error model (mlggd_error_stats' sums and mlggd_ggd_fit), in plain Python floats with
math.lgamma: what the tests compare the library against.

Density of one bin (the reference's, BP_GPU.cu:271-301):  beta / (2 alpha Gamma(1/beta)) * exp(-(|e| / alpha)^beta).
For a fixed beta the ML scale is alpha^beta = beta * sum|e|^beta / n, at which sum (|e|/alpha)^beta = n / beta, so the
profile log-likelihood is  n [ln beta - ln 2 - lgamma(1/beta) - ln alpha - 1/beta]."""
import collections
import math

import numpy as np

Fit = collections.namedtuple("Fit", "mean var kurt alpha loglik best loglik_shared best_shared")
NAN = float("nan")


def grid(lo=0.5, step=0.1, hi=2.5):
    """beta_i = float32(lo + i * step), the sum evaluated in double, while <= hi + step / 2"""
    out, i = [], 0
    while lo + i * step <= hi + step / 2:
        out.append(np.float32(lo + i * step))
        i += 1
    return np.array(out, np.float32)


def sums(e, betas):
    """[4 + K][D] float64 sums of e, e^2, e^3, e^4 and |e|^beta_k over the rows of e [n][D], each sum by math.fsum"""
    e = np.asarray(e, np.float64)
    e2 = e * e
    terms = [e, e2, e2 * e, e2 * e2] + [np.abs(e) ** float(np.float32(b)) for b in betas]
    return np.array([[math.fsum(t[:, d]) for d in range(e.shape[1])] for t in terms], np.float64)


def fit(n, s, betas):
    s = np.asarray(s, np.float64)
    K, D = len(betas), s.shape[1]
    assert s.shape[0] == 4 + K and n > 0
    nn = float(n)
    mean, var, kurt, best = [0.0] * D, [0.0] * D, [NAN] * D, [-1] * D
    alpha = [[0.0] * D for _ in range(K)]
    loglik = [[NAN] * D for _ in range(K)]
    shared = [0.0] * K
    for d in range(D):
        s1, s2, s3, s4 = (float(s[j, d]) for j in range(4))
        mu, r2, r3, r4 = s1 / nn, s2 / nn, s3 / nn, s4 / nn
        m2 = r2 - mu * mu
        m4 = ((r4 - 4.0 * mu * r3) + 6.0 * (mu * mu) * r2) - 3.0 * ((mu * mu) * (mu * mu))
        mean[d], var[d] = mu, m2
        if s2 == 0.0:
            continue                                      # no fit: alpha 0, loglik and kurt NaN, best -1
        kurt[d] = m4 / (m2 * m2) - 3.0
        top = None
        for k in range(K):
            b = float(np.float32(betas[k]))
            lna = math.log(b * float(s[4 + k, d]) / nn) / b
            alpha[k][d] = math.exp(lna)
            l = nn * ((((math.log(b) - math.log(2.0)) - math.lgamma(1.0 / b)) - lna) - 1.0 / b)
            loglik[k][d] = l
            shared[k] += l
            if top is None or l > top:
                top, best[d] = l, k
    best_shared = -1
    if any(b >= 0 for b in best):
        best_shared = max(range(K), key=lambda k: (shared[k], -k))
    return Fit(np.array(mean), np.array(var), np.array(kurt), np.array(alpha), np.array(loglik),
               np.array(best, np.int32), np.array(shared), best_shared)


def draw(rng, n, alphas, beta):
    """[n][len(alphas)] float64 GGD samples: |e| = alpha * G^(1/beta), G ~ Gamma(1/beta, 1), with a random sign"""
    alphas = np.asarray(alphas, np.float64)
    g = rng.gamma(1.0 / beta, 1.0, size=(n, alphas.size))
    sign = np.where(rng.random((n, alphas.size)) < 0.5, -1.0, 1.0)
    return sign * alphas * g ** (1.0 / beta)
