"""The parameter gradient of the GGX conductor's eval (include/merl_hip_fit.h, mrl_ggx_grad_batch) from tests/ggx_reference.py alone:
J = d eval_c / d p for p = (alpha, eta_r, eta_g, eta_b, k_r, k_g, k_b) by central differences of ggx_reference.eval in f64, with
the step 1e-5 |p| (an absolute 1e-6 where p = 0).  Nothing here knows the analytic derivative the kernel computes.

Channel c depends on alpha, eta_c and k_c only; the other entries of J are structurally zero.  For a channel with k = 0 the
k-derivative is exactly 0 (F depends on k through k^2), and is set so instead of differenced.  A unit eval masks — cos(theta_i) <= 0,
cos(theta_o) <= 0, a NaN / inf / zero-length direction — has J = 0 and its g and h are not looked at."""
import numpy as np

from tests import ggx_reference as ggx

N_PARAMS = 7
PARAM_NAMES = ("alpha", "eta_r", "eta_g", "eta_b", "k_r", "k_g", "k_b")
REL_STEP = 1e-5
ABS_STEP_AT_ZERO = 1e-6          # at REL_STEP; scaled with the step


def params_vector(alpha, eta, k):
    return np.array([alpha, *eta, *k], np.float64)


def split(p):
    return float(p[0]), [float(x) for x in p[1:4]], [float(x) for x in p[4:7]]


def live_units(wi, wo):
    """The units eval does not mask."""
    wi, wo = np.asarray(wi, np.float64), np.asarray(wo, np.float64)
    with np.errstate(all="ignore"):
        return np.isfinite(wi).all(-1) & np.isfinite(wo).all(-1) & (wi[:, 2] > 0) & (wo[:, 2] > 0)


def same_channel(a, b):
    """Does entry (a, b) of the normal matrix couple parameters of one channel (alpha belongs to all three)?"""
    ca, cb = (None if a == 0 else (a - 1) % 3), (None if b == 0 else (b - 1) % 3)
    return ca is None or cb is None or ca == cb


def jacobian(alpha, eta, k, wi, wo, rel_step=REL_STEP):
    """J [n, 3, 7] f64 at the parameters given (pass what the material stores: ggx_reference.f32_params)."""
    p = params_vector(alpha, eta, k)
    live = live_units(wi, wo)
    lwi, lwo = np.asarray(wi, np.float64)[live], np.asarray(wo, np.float64)[live]
    J = np.zeros((len(live), 3, N_PARAMS))
    for j in range(N_PARAMS):
        if j >= 4 and p[j] == 0.0:
            continue                                         # F is even in k
        step = rel_step * abs(p[j]) if p[j] != 0.0 else ABS_STEP_AT_ZERO * (rel_step / REL_STEP)
        hi, lo = p.copy(), p.copy()
        hi[j] += step; lo[j] -= step
        d = (ggx.eval(*split(hi), lwi, lwo) - ggx.eval(*split(lo), lwi, lwo)) / (hi[j] - lo[j])
        if j == 0:
            J[live, :, 0] = d
        else:
            c = (j - 1) % 3
            J[live, c, j] = d[:, c]
    return J


def sums(J, g, h=None):
    """R [7] = sum g J and S [7] = sum |g J|; with h also R2 [7, 7] = sum h J_a J_b and S2 = sum |h J_a J_b|.  g, h: [n, 3]; the values
    of units with J = 0 everywhere (dead units) are not used, whatever they hold."""
    dead = ~(J != 0).any((1, 2))
    g = np.where(dead[:, None], 0.0, np.asarray(g, np.float64))
    with np.errstate(all="ignore"):
        t = g[:, :, None] * J
    out = [t.sum((0, 1)), np.abs(t).sum((0, 1))]
    if h is not None:
        h = np.where(dead[:, None], 0.0, np.asarray(h, np.float64))
        with np.errstate(all="ignore"):
            t2 = np.einsum("uc,uca,ucb->ucab", h, J, J)
        out += [t2.sum((0, 1)), np.abs(t2).sum((0, 1))]
    return tuple(out)


def reference(alpha, eta, k, wi, wo, g, h=None, rel_step=REL_STEP):
    return sums(jacobian(alpha, eta, k, wi, wo, rel_step), g, h)
