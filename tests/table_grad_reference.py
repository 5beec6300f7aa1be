"""numpy f64 restatement of A^T, the adjoint of eval on an RGB table (include/merl_hip.h, mrl_table_grad_batch).

Row u of A holds guard x (cos(theta_o) or 1) x scale[c] x the eight corner weights of the trilinear lookup (a single 1 for the
nearest lookup).  The coordinates come from tests/np_restatement.py (half_diff / coords) and its split rules; the weights are
formed in f64 the way corner_weights() does and rounded once to f32, the cosine is the Float wo.z.  Pinned to the CPU oracle by
tests/test_table_grad_cpu.py, never to the code under test."""
import numpy as np

from tests import np_restatement as npr

HALF_DIFF, STANDARD, STANDARD_FULL = 0, 1, 2


def guard(wi, wo):
    """The units eval does not mask: both cosines positive, every component finite."""
    wi = np.asarray(wi, np.float32); wo = np.asarray(wo, np.float32)
    with np.errstate(invalid="ignore"):
        return (wi[:, 2] > 0) & (wo[:, 2] > 0) & np.isfinite(wi).all(1) & np.isfinite(wo).all(1)


def table_coords(wi, wo, dims, param=HALF_DIFF):
    """Continuous table coordinates (x0, x1, x2) of the guarded units (the others get a harmless direction)."""
    ok = guard(wi, wo)
    up = np.array([0.0, 0.0, 1.0])
    a = np.where(ok[:, None], np.asarray(wi, np.float32).astype(np.float64), up)
    b = np.where(ok[:, None], np.asarray(wo, np.float32).astype(np.float64), up)
    if param == HALF_DIFF:
        return npr.coords(*npr.half_diff(a, b), dims) + (ok,)
    a, b = npr.unit(a), npr.unit(b)
    n0, n1, n2 = dims
    ti = np.arctan2(np.hypot(a[:, 0], a[:, 1]), a[:, 2])
    to = np.arctan2(np.hypot(b[:, 0], b[:, 1]), b[:, 2])
    cr = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    dt = a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]
    dp = np.where((cr == 0) & (dt == 0), 0.0, np.arctan2(cr, dt))
    x0, x1 = ti / (np.pi / 2) * n0, to / (np.pi / 2) * n1
    if param == STANDARD:
        x2 = np.abs(dp) / np.pi * n2
    else:
        x2 = np.where(dp < 0, dp + 2 * np.pi, dp) / (2 * np.pi) * n2
    return x0, x1, x2, ok


def near_cell_boundary(wi, wo, dims, param=HALF_DIFF, eps=1e-9):
    """Units whose coordinate on some axis is within eps of an integer: a nearest lookup may bin them either way."""
    x0, x1, x2, ok = table_coords(wi, wo, dims, param)
    near = np.zeros(len(ok), bool)
    for x in (x0, x1, x2):
        near |= np.abs(x - np.round(x)) <= eps
    return near & ok


def _split_clamped(x, n):
    i = np.clip(np.floor(x).astype(np.int64), 0, n - 1)
    return i, np.minimum(i + 1, n - 1), np.clip(x - i, 0.0, 1.0)


def _split_periodic(x, n):
    fl = np.floor(x)
    i = np.mod(fl.astype(np.int64), n)
    return i, np.mod(i + 1, n), x - fl


def adjoint(wi, wo, g, dims, param=HALF_DIFF, trilinear=True, center=False, cosine=True, scale=(1.0, 1.0, 1.0)):
    """Returns (R, S): R = A^T g as f64 [3, n0, n1, n2] and S = sum_u |a_u g_u| per cell and channel (the error scale)."""
    n0, n1, n2 = dims
    wo32 = np.asarray(wo, np.float32)
    g64 = np.asarray(g, np.float32).astype(np.float64)
    x0, x1, x2, ok = table_coords(wi, wo, dims, param)
    factor = wo32[:, 2].astype(np.float64) if cosine else np.ones(len(ok))
    with np.errstate(invalid="ignore"):
        s = np.asarray(scale, np.float64)[None, :] * factor[:, None] * g64                   # [n, 3]
    keep = np.nonzero(ok)[0]
    s = s[keep]
    if trilinear:
        sh = 0.5 if center else 0.0
        h0, h1, fh = _split_clamped(x0[keep] - sh, n0)
        d0, d1, fd = _split_clamped(x1[keep] - sh, n1)
        p0, p1, fp = _split_clamped(x2[keep] - sh, n2) if param == STANDARD else _split_periodic(x2[keep] - sh, n2)
        gh, gd, gp = 1.0 - fh, 1.0 - fd, 1.0 - fp
        corners = [(h0, d0, p0, (gh * gd) * gp), (h0, d0, p1, (gh * gd) * fp), (h0, d1, p0, (gh * fd) * gp), (h0, d1, p1, (gh * fd) * fp),
                   (h1, d0, p0, (fh * gd) * gp), (h1, d0, p1, (fh * gd) * fp), (h1, d1, p0, (fh * fd) * gp), (h1, d1, p1, (fh * fd) * fp)]
    else:
        ih = np.clip(np.trunc(x0[keep]).astype(np.int64), 0, n0 - 1)
        id_ = np.clip(np.trunc(x1[keep]).astype(np.int64), 0, n1 - 1)
        ip = np.clip(np.trunc(x2[keep]).astype(np.int64), 0, n2 - 1)
        corners = [(ih, id_, ip, np.ones(len(keep)))]
    plane = n0 * n1 * n2
    R = np.zeros(3 * plane); S = np.zeros(3 * plane)
    for hi, di, pi, w in corners:
        w = w.astype(np.float32).astype(np.float64)                  # rounded once to Float, like corner_weights()
        cell = (hi * n1 + di) * n2 + pi
        for c in range(3):
            v = w * s[:, c]
            np.add.at(R, c * plane + cell, v)
            np.add.at(S, c * plane + cell, np.abs(v))
    return R.reshape(3, n0, n1, n2), S.reshape(3, n0, n1, n2)



# ---- inputs for the wave-level tests (tests/test_gpu_table_grad_waves.py, tests/test_table_grad_waves_cpu.py) ----

def _angles(wi, wo):
    """theta_h, theta_d of the f32 pairs in their cancellation-free atan2 forms.  The twin of tests/test_gpu_table_shapes.py::_angles,
    restated so that this module imports no test module: keep the two alike."""
    a = np.asarray(wi, np.float32).astype(np.float64); b = np.asarray(wo, np.float32).astype(np.float64)
    a = a / np.linalg.norm(a, axis=1, keepdims=True); b = b / np.linalg.norm(b, axis=1, keepdims=True)
    s, e = a + b, a - b
    return np.arctan2(np.hypot(s[:, 0], s[:, 1]), s[:, 2]), np.arctan2(np.linalg.norm(e, axis=1), np.linalg.norm(s, axis=1))


def interior(wi, wo, dims, param=HALF_DIFF, center=False, lo=0.05, hi=0.95):
    """Mask of the guarded units well inside a cell and away from the transform's singular directions: the fractional part of the
    coordinate the lookup splits (x - 0.5 with center; the unshifted x otherwise, which is also what the nearest lookup truncates)
    lies in [lo, hi] on all three axes, and theta_h, theta_d both exceed 0.02 rad.  For these no two correct implementations can
    disagree on the cell, and a corner weight is 0 (a clamped end) or at least lo^3 = 1.25e-4."""
    x0, x1, x2, ok = table_coords(wi, wo, dims, param)
    sh = 0.5 if center else 0.0
    inside = ok.copy()
    for x in (x0, x1, x2):
        y = x - sh
        f = y - np.floor(y)
        inside &= (f >= lo) & (f <= hi)
    with np.errstate(invalid="ignore"):
        th, td = _angles(np.where(ok[:, None], wi, (0.0, 0.0, 1.0)), np.where(ok[:, None], wo, (0.0, 0.0, 1.0)))
    return inside & (th > 0.02) & (td > 0.02)


def cell_index(wi, wo, dims, param=HALF_DIFF, center=False):
    """The flattened cell (h0, d0, p0) adjoint() gives each unit's trilinear lookup (for an interior unit and center=False it is the
    nearest lookup's texel too); -1 for a unit the guard removes."""
    n0, n1, n2 = dims
    x0, x1, x2, ok = table_coords(wi, wo, dims, param)
    sh = 0.5 if center else 0.0
    h0 = _split_clamped(x0 - sh, n0)[0]
    d0 = _split_clamped(x1 - sh, n1)[0]
    p0 = (_split_clamped(x2 - sh, n2) if param == STANDARD else _split_periodic(x2 - sh, n2))[0]
    return np.where(ok, (h0 * n1 + d0) * n2 + p0, -1)


DEAD_KINDS = 5


def kill(wi, wo, at):
    """Makes the units at the indices `at` dead in place, cycling through: wi below the horizon, wo below the horizon, a NaN
    component, an infinite component, a zero-length wi."""
    for k, i in enumerate(np.asarray(at, np.int64)):
        kind = k % DEAD_KINDS
        if kind == 0: wi[i, 2] = -wi[i, 2]
        elif kind == 1: wo[i, 2] = -wo[i, 2]
        elif kind == 2: wi[i, k % 3] = np.nan
        elif kind == 3: wo[i, k % 3] = np.inf
        else: wi[i] = 0.0


def poisoned(g, wi, wo):
    """A copy of g with NaN and inf, alternating, in the rows of the units the guard removes."""
    g = np.array(g, np.float32)
    dead = np.nonzero(~guard(wi, wo))[0]
    g[dead[0::2]] = np.nan
    g[dead[1::2]] = np.inf
    return g


def sequence(pool_wi, pool_wo, dims, param=HALF_DIFF, center=False, length=1021, every=9):
    """The first `length` interior units of the pool, every 9th replaced by a dead one (kill's kinds in turn).  f32 copies."""
    keep = np.nonzero(interior(pool_wi, pool_wo, dims, param, center))[0][:length]
    assert len(keep) == length, (len(keep), length)
    wi = np.array(pool_wi[keep], np.float32); wo = np.array(pool_wo[keep], np.float32)
    kill(wi, wo, np.arange(every - 1, length, every))
    return wi, wo


WAVE = 64
LAYOUT_UNITS = 5 * WAVE                  # four waves of one block and a ragged second block
LAYOUT_NAMES = tuple("abcdefghij")
_DEAD, _DISTINCT = -1, -2                # lane codes; a code >= 0 names a group (0: cell X, 1: cell Y)


def layout_lanes(name):
    """The make-up of the chosen wave of layout `name`, lane by lane: a group number (0, 1: all lanes of a group share one cell),
    _DISTINCT (a cell no other lane of the wave has) or _DEAD."""
    lanes = np.full(WAVE, _DISTINCT)
    if name == "a":                      # one cell
        lanes[:] = 0
    elif name == "b":                    # the auto rule merges on lanes 0-3; a group with no member in the low half
        lanes[0:4] = 0; lanes[32:64] = 1
    elif name == "c":                    # the first live lane is 30; its group straddles the halves
        lanes[0:30] = _DEAD; lanes[30:34] = 0
    elif name in "de":                   # 3 / 4 sharers of the first live lane's cell, a group of 40 later in the wave
        lanes[[0, 5, 11] if name == "d" else [0, 5, 11, 17]] = 0
        lanes[24:64] = 1
    elif name == "f":                    # a merged group of 48, every third member dead
        lanes[0:48] = 0; lanes[2:48:3] = _DEAD
    elif name == "g":                    # a dead wave between live ones
        lanes[:] = _DEAD
    elif name == "h":                    # live on even lanes only
        lanes[1::2] = _DEAD
    elif name == "i":                    # live on odd lanes only
        lanes[0::2] = _DEAD
    elif name == "j":                    # two groups of 32, lane by lane
        lanes[0::2] = 0; lanes[1::2] = 1
    else:
        raise ValueError(name)
    return lanes


def wave_layouts(pool_wi, pool_wo, dims, param=HALF_DIFF, center=False, wave=1):
    """{name: (wi, wo)}: arrays of LAYOUT_UNITS units whose wave `wave` (units 64 wave .. 64 wave + 63; a unit's lane in the kernel
    is its index mod 64) has the make-up layout_lanes(name) and whose other waves are live pool units.  All live units are interior
    units of the pool, each used once per layout; the groups take the fullest cells, in a different rotation per layout."""
    inside = np.nonzero(interior(pool_wi, pool_wo, dims, param, center))[0]
    cells = cell_index(pool_wi[inside], pool_wo[inside], dims, param, center)
    ids, counts = np.unique(cells, return_counts=True)
    order = np.argsort(-counts, kind="stable")
    big = [int(c) for c in ids[order] if counts[ids == c][0] >= WAVE]
    assert len(big) >= 2, "the pool needs two cells with a wave of interior units each: cell X and cell Y of a layout"
    members = {int(c): list(inside[cells == c]) for c in ids}
    out = {}
    for k, name in enumerate(LAYOUT_NAMES):
        x, y = big[k % len(big)], big[(k + 1) % len(big)]
        take = {c: iter(m) for c, m in members.items()}
        singles = iter([int(c) for c in ids if c not in (x, y)])
        lanes = layout_lanes(name)
        chosen = np.empty(WAVE, np.int64)
        for lane, code in enumerate(lanes):
            if code >= 0:
                chosen[lane] = next(take[(x, y)[code]])
            else:                        # a dead lane starts from a live unit of a cell of its own too
                chosen[lane] = next(take[next(singles)])
        used = set(chosen.tolist())
        filler = [i for i in inside[: LAYOUT_UNITS + WAVE] if i not in used][: LAYOUT_UNITS - WAVE]
        idx = np.concatenate([filler[: wave * WAVE], chosen, filler[wave * WAVE:]]).astype(np.int64)
        wi = np.array(pool_wi[idx], np.float32); wo = np.array(pool_wo[idx], np.float32)
        kill(wi, wo, wave * WAVE + np.nonzero(lanes == _DEAD)[0])
        out[name] = (wi, wo)
    return out
