"""The model of the ratio-mask targets and the mask post-filter (csrc/mask_rule.h), restated for the tests: the rule one
NumPy float32 operation at a time (the exponential is handed in: pyoracle.exp_det, the kernels' own), the float64 value
of the target and the bound between the two, and the tables the stand-alone program and the tests run on."""
import numpy as np

U24 = 2.0 ** -24          # half an fp32 ulp, relative: the rounding of one fp32 operation on a normal number
TINY = 2.0 ** -149        # the smallest fp32 step: what an operation whose result is subnormal may lose
EXP_LO = -85.5            # below it exp_det returns its value at -85.5 (kernels.hip.h)
EXP_SAT = 7.5e-38         # ... which is below this


def f32(x):
    return np.asarray(x, np.float32)


def half_diff32(c, y):
    """a = c - y, h = 0.5 a (exact)"""
    with np.errstate(invalid="ignore"):
        a = (f32(c) - f32(y)).astype(np.float32)
    return (np.float32(0.5) * a).astype(np.float32)


def target_from_exp32(ex, s):
    """m = ex > 1 ? 1 : ex (a NaN stays), t = s m"""
    ex = f32(ex)
    with np.errstate(invalid="ignore"):
        m = np.where(ex > np.float32(1), np.float32(1), ex).astype(np.float32)
    return (np.float32(s) * m).astype(np.float32)


def target32(c, y, s, exp_det):
    """t = s min(1, exp_det(0.5 (c - y))) in float32, exp_det the kernels' exponential (pyoracle.exp_det)"""
    h = half_diff32(c, y)
    return target_from_exp32(exp_det(h.ravel()).reshape(h.shape), s)


def select32(n, x, o, s, lo, hi):
    """m = o / s;  v = m > hi ? n : (m >= lo ? 0.5 (n + x) : x);  a NaN mask takes x"""
    n, x = f32(n), f32(x)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = (f32(o) / np.float32(s)).astype(np.float32)
        mid = (np.float32(0.5) * (n + x).astype(np.float32)).astype(np.float32)
        v = np.where(m > np.float32(hi), n, np.where(m >= np.float32(lo), mid, x))
    return v.astype(np.float32)


def branches(o, s, lo, hi):
    """which branch each element takes: 2 noisy, 1 mean, 0 estimate"""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = (f32(o) / np.float32(s)).astype(np.float32)
        return np.where(m > np.float32(hi), 2, np.where(m >= np.float32(lo), 1, 0)), m


def target64(c, y, s):
    """s min(1, sqrt(Pc / Py)) in float64 with Pc = exp(c), Py = exp(y): s min(1, exp((c - y) / 2))"""
    with np.errstate(over="ignore", invalid="ignore"):
        d = f32(c).astype(np.float64) - f32(y).astype(np.float64)  # two fp32 values in double: one rounding of 2^-53
        return float(s) * np.minimum(1.0, np.exp(0.5 * d))


def target_bound(c, y, s):
    """|target32 - target64| per element for finite rows, derived and not fitted.  With d = c - y exact, u = 2^-24:
      a = fl(d)                  |a - d| <= u |d|; h = a / 2 is exact
      e = exp_det(h)             |e - exp(h)| < one ulp of exp(h) <= 2^-23 exp(h) for -85.5 <= h <= 88.7, the distance
                                 tests/test_oracle.py pins; below -85.5 both e and exp(h) lie in [0, 7.5e-38)
      exp(h) against exp(d / 2)  exp(d / 2) |exp((a - d) / 2) - 1| <= exp(d / 2) expm1(u |d| / 2)
      m = min(1, .)              min(1, .) moves by no more than its argument does; from d / 2 >= 1 on both sides are
                                 capped (exp(h) > 2.7, so is an e within one ulp of it) and m does not move at all
      t = fl(s m)                |t - s m| <= u s m, or 2^-149 where the product is subnormal
    and float64's own error in target64, a few 2^-53 relative, is covered by doubling the last term."""
    s = float(s)
    with np.errstate(over="ignore", invalid="ignore"):
        d = f32(c).astype(np.float64) - f32(y).astype(np.float64)
        # d / 2 >= 1: h >= 1 (1 - 2^-24), exp(h) > 2.7 and an e within one ulp of it is above 1: both sides are capped
        capped = 0.5 * d >= 1.0
        e_half = np.exp(np.minimum(0.5 * d, 1.0))
        arg = e_half * np.expm1(U24 * np.abs(d) / 2.0)
        ulp = 2.0 ** -23 * e_half
        sat = np.where(0.5 * d < EXP_LO + 1e-3, EXP_SAT, 0.0)
        dm = np.where(capped, 0.0, arg + ulp + sat)
        m = np.minimum(1.0, e_half)
        return s * dm + 2.0 * U24 * s * (m + dm) + TINY


# ---- tables -----------------------------------------------------------------------------------------------------

def target_table():
    """(c, y, s) float32, flat: random LPS values, c > y (the cap), c == y, floor-valued entries (digital silence, -50),
    differences beyond both ends of the exponential's range, +-inf and NaN"""
    rng = np.random.default_rng(21)
    c = rng.normal(8, 5, 600).astype(np.float32)
    y = (c + rng.normal(-1.5, 3, 600)).astype(np.float32)
    y[:40] = c[:40]                                                     # c == y
    c[40:60] = -50.0                                                    # silence in the clean wave
    y[60:80] = -50.0                                                    # ... in the noisy wave: the cap
    c[80:90] = y[80:90] = -50.0                                         # ... in both
    sp_c = np.array([0, 0, 1, -1, 200, -200, np.inf, -np.inf, np.inf, -np.inf, np.nan, 3, np.nan, 1e-30, 177.5, -171.0], np.float32)
    sp_y = np.array([0, -0.0, 1, -1, -200, 200, 0, 0, np.inf, -np.inf, 3, np.nan, np.nan, -1e-30, 0.0, 0.0], np.float32)
    c, y = np.concatenate([c, sp_c]), np.concatenate([y, sp_y])
    s = np.tile(np.array([1.0, 0.5, 3.0, 0.1], np.float32), (c.size + 3) // 4)[:c.size]
    return c, y, s


def select_table():
    """(n, x, o, s, lo, hi) float32, flat: masks around and exactly on both thresholds, lo == hi, NaN and +-inf in the
    mask, in the noisy row and in the estimate"""
    rng = np.random.default_rng(22)
    rows = []
    for lo, hi, s in ((0.25, 0.75, 1.0), (0.25, 0.75, 0.5), (0.5, 0.5, 2.0), (0.1, 0.9, 3.0), (0.0, 1.0, 0.25), (-1.0, -1.0, 1.0)):
        lo, hi, s = np.float32(lo), np.float32(hi), np.float32(s)
        m = np.concatenate([rng.uniform(-0.3, 1.3, 80).astype(np.float32),
                            np.array([lo, hi, np.nextafter(lo, np.float32(-9)), np.nextafter(lo, np.float32(9)),
                                      np.nextafter(hi, np.float32(-9)), np.nextafter(hi, np.float32(9)), np.nan, np.inf,
                                      -np.inf, 0.0, -0.0, 1.0], np.float32)])
        o = (m * s).astype(np.float32)                                   # exact for the powers of two, near for s = 3
        n = rng.normal(8, 5, m.size).astype(np.float32)
        x = rng.normal(6, 5, m.size).astype(np.float32)
        n[3], x[5], n[7], x[7] = np.nan, np.nan, np.inf, -np.inf
        n[9], x[9] = 3.0e38, 3.0e38                                      # n + x overflows: the mean is +inf
        for i in range(m.size):
            rows.append((n[i], x[i], o[i], s, lo, hi))
    t = np.array(rows, np.float32)
    return tuple(np.ascontiguousarray(t[:, k]) for k in range(6))
