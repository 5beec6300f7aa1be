"""The gradient of eval in the measured values of an RGB RGL material (include/merl_hip_fit_rgl.h) from a restatement of the model
alone: autograd, on the CPU, of tests/rgl_dir_grad_reference.forward — torch f64 on the oracle's own Float arrays — with
A.rgb["data"] requiring grad.  Nothing here knows an analytic derivative.

    G = d / dR  sum_u sum_c g_uc E_c(u; R)          S = d / dR  sum_u sum_c |g_uc| E_c(u; R)

S_t = sum_u sum_c |g_c| |dE_c / dR_t| is the scale of the bar |G_t - R_t| <= REL S_t: every partial derivative J ws_k wc_j is >= 0
(J = ndf / (4 sigma) of positive tables, the slice weights are clamped to [0, 1], the cell fractions lie in [0, 1] up to an f64
rounding of sx at the right edge), so the derivative of the |g|-weighted sum IS that sum of absolute values, to 1e-15 of itself.

Units rgl_dir_grad_reference.excused marks (a last-bit change selects another cell, or flips a clamp) are replaced by HARMLESS
BEFORE either side runs — a sum cannot leave units out afterwards; case_data asserts the cap on them on the reference alone.  Dead
units keep their dirty g: the code under test must not look at it, the reference leaves them out."""
import copy
import os
import subprocess

import numpy as np
import torch

from tests import rgl_dir_grad_reference as rref

REL = 1e-6
FILE_NAMES = rref.FILE_NAMES
ROOT = rref.ROOT
KERNEL_SOURCE = os.path.join(ROOT, "mitsuba_customization_amd", "csrc", "merl_rgl_values_grad.hip")
_CASE = {}


def values_shape(A):
    return (A.n_phi, A.n_theta, 3, A.rgb["ny"], A.rgb["nx"])


def values_grad(A, wi, wo, g, rgb=None):
    """(G, S, E): f64 [n_phi, n_theta, 3, ny, nx] twice and eval [n, 3] of LIVE pairs (f64 numpy wi, wo [n, 3]; g [n, 3]);
    rgb: other values than the file's own (same layout)"""
    R = (A.rgb["data"] if rgb is None else torch.as_tensor(np.asarray(rgb, np.float64)).reshape(A.rgb["data"].shape)).clone().requires_grad_(True)
    B = copy.copy(A)
    B.rgb = dict(A.rgb, data=R)
    with torch.enable_grad():
        val, _ = rref.forward(B, torch.as_tensor(np.asarray(wi, np.float64)), torch.as_tensor(np.asarray(wo, np.float64)))
        gt = torch.as_tensor(np.asarray(g, np.float64))
        G, = torch.autograd.grad((val * gt).sum(), R, retain_graph=True)
        S, = torch.autograd.grad((val * gt.abs()).sum(), R)
    sh = values_shape(A)
    return G.numpy().reshape(sh), S.numpy().reshape(sh), val.detach().numpy()


def case(name):
    """case_data(name) with the excused units replaced by HARMLESS, and the reference's G, S on it — once per file, read-only.
    wi, wo, g are what the code under test receives (dead units with their dirty g included)."""
    if name not in _CASE:
        d = rref.case_data(name)
        wi, wo = d["wi"].copy(), d["wo"].copy()
        wi[d["excused"]], wo[d["excused"]] = rref.HARMLESS[0], rref.HARMLESS[1]
        alive = d["alive"]
        G, S, E = values_grad(d["arrays"], wi[alive], wo[alive], d["g"][alive])
        assert np.isfinite(G).all() and np.isfinite(S).all() and (S >= 0).all()
        c = dict(name=name, fields=d["fields"], arrays=d["arrays"], wi=wi, wo=wo, g=d["g"], alive=alive, G=G, S=S, E=E)
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CASE[name] = c
    return _CASE[name]


def check(G, c, start=0.0, what="", adds=1):
    """the bar: |G_t - R_t| <= REL S_t, exactly the initial bits where S_t == 0, everything finite.  G: what the code under test
    added, in `adds` calls, into an array that held `start` everywhere: each add into a non-zero start rounds the sum once at the
    start's magnitude (2^-53 |start + x| <= 2^-52 |start| while |x| <= |start|), which no code can avoid and the bar allows for; into
    +-0 the add is exact.  Returns the worst measured ratio of |G - R| to S (printed)."""
    G = np.asarray(G, np.float64).reshape(c["S"].shape)
    assert np.isfinite(G).all(), what
    zero = c["S"] == 0.0
    want0 = np.full(1, start, np.float64)
    assert np.array_equal(G[zero].view(np.uint64), np.broadcast_to(want0.view(np.uint64), G[zero].shape)), (what, "a texel nothing reaches must keep its bits")
    assert start == 0.0 or float(np.abs(c["G"]).max()) <= abs(start)
    err = np.abs((G - start) - c["G"])[~zero]
    slack = adds * 2.0 ** -52 * abs(start)
    worst = float((np.maximum(err - slack, 0.0) / c["S"][~zero]).max()) if err.size else 0.0
    print(f"rgl values grad {what or c['name']}: worst |G - R| / S = {worst:.3e} over {int((~zero).sum())} texels ({int(zero.sum())} unreached)")
    assert worst <= REL, (what, worst)
    return worst


# ------------------------------------------------------------------ the per-lane function and the fold, compiled for the host
HARNESS_SOURCE = os.path.join(ROOT, "tests", "rgl_values_grad_host_harness.hip")


def build_harness(tmp_path_factory, sanitize=False):
    """tests/rgl_values_grad_host_harness.hip, built once per session (sanitize: with AddressSanitizer + UBSan on the host code)"""
    build = tmp_path_factory.getbasetemp() / ("rgl_values_grad_host_harness" + ("_san" if sanitize else ""))
    if not build.exists():
        extra = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-g"] if sanitize else []
        subprocess.check_call(["hipcc", "-O1" if sanitize else "-O2", "-std=c++17", "--offload-arch=gfx950", "-mavx2", "-mfma", "-w"] + extra +
                              ["-o", str(build), HARNESS_SOURCE])
    return build


def run_harness(build, tmp, fields, wi, wo, g, start=-0.0, own_mask=False):
    """(G_bricks, G_plain) f64 in the file's rgb layout: the units through values_grad_unit, the gradient bricks and fold_sources /
    through values_texel, both added into arrays that held `start`.  own_mask: values_grad_unit instantiated for the file's bracket
    shape (MASK = rref.file_mask(fields), the single-material brick kernels' form) instead of MASK 0"""
    n = len(wi)
    rref.write_fields(tmp / "f.bin", fields)
    with open(tmp / "u.bin", "wb") as o:
        np.array([n], np.uint64).tofile(o)
        for x in (wi, wo, g):
            np.ascontiguousarray(x, np.float32).tofile(o)
        np.array([start], np.float64).tofile(o)
    r = subprocess.run([str(build), "grad", str(tmp / "f.bin"), str(tmp / "u.bin"), str(tmp / "o.bin")] + (["mask"] if own_mask else []),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    assert f"MASK {rref.file_mask(fields) if own_mask else 0}\n" in r.stdout, r.stdout
    shape = np.asarray(fields["rgb"]).shape
    out = np.fromfile(tmp / "o.bin", np.float64).reshape((2,) + shape)
    return out[0], out[1]


def fold_expected(n_phi, n_theta, nx, ny, slot_value):
    """texel sums [n_phi, n_theta, 3, ny, nx] that append_warp's copy rule implies: slice (ip, it) goes to every bracket (ip - dp,
    it - dt) it bounds as the bracket's slice dp + 2 dt (dt with one phi node), node (y, x) to corner 2 dy + dx of cell (y - dy, x - dx);
    slot_value(index of the double in the workspace) is what that slot holds"""
    tb, pb = max(n_theta - 1, 1), max(n_phi - 1, 1)
    S = (2 if n_phi > 1 else 1) * (2 if n_theta > 1 else 1)
    cells = (nx - 1) * (ny - 1)
    out = np.zeros((n_phi, n_theta, 3, ny, nx))
    for ipb in range(pb):
        for itb in range(tb):
            for cy in range(ny - 1):
                for cx in range(nx - 1):
                    rec = (ipb * tb + itb) * cells + cy * (nx - 1) + cx
                    for c in range(3):
                        for dp in range(2 if n_phi > 1 else 1):
                            for dt in range(2 if n_theta > 1 else 1):
                                k = dp + 2 * dt if n_phi > 1 else dt
                                for dy in range(2):
                                    for dx in range(2):
                                        out[ipb + dp, itb + dt, c, cy + dy, cx + dx] += slot_value(rec * 16 * S + (c * S + k) * 4 + 2 * dy + dx)
    return out


# ------------------------------------------------------------------ the reference's own weights, unit by unit
def weights(A, wi, wo):
    """(J [n], cols [n, 16], w [n, 16]) of LIVE pairs on a file without negative values: E_uc = J_u sum_q w_uq R[cols_uq + c ny nx] —
    read off the reference's forward pass alone.  eval is linear in R there, and the slice and corner weights of a unit each sum to 1,
    so forward on R = 1 gives J, and on R = a node's x (y, theta, phi) index gives J (ox + fx) (oy + fy, it + tt, ip + tp): the cell
    and bracket with their fractions.  (An index that rounds across an integer names the neighbouring cell with the fraction at its
    other end: the same weights on the same texels.)"""
    n_phi, n_theta, _, ny, nx = sh = values_shape(A)
    assert float(A.rgb["data"].min()) >= 0.0
    B = copy.copy(A)

    def probe(P):
        B.rgb = dict(A.rgb, data=torch.as_tensor(np.array(np.broadcast_to(P, sh), np.float64)).reshape(A.rgb["data"].shape))
        with torch.no_grad():
            return rref.forward(B, torch.as_tensor(np.asarray(wi, np.float64)), torch.as_tensor(np.asarray(wo, np.float64)))[0][:, 0].numpy()
    J = probe(np.ones(sh))
    safe = np.where(J != 0.0, J, 1.0)
    axis = lambda k, m: np.arange(m, dtype=np.float64).reshape([m if a == k else 1 for a in range(5)])
    split = lambda v, m: (np.clip(np.floor(v), 0, max(m - 2, 0)).astype(np.int64), v - np.clip(np.floor(v), 0, max(m - 2, 0)))
    ox, fx = split(probe(axis(4, nx)) / safe, nx)
    oy, fy = split(probe(axis(3, ny)) / safe, ny)
    it, tt = split(probe(axis(1, n_theta)) / safe, n_theta)
    ip, tp = split(probe(axis(0, n_phi)) / safe, n_phi)
    cols, w = [], []
    for dp, wp in ((0, 1 - tp), (1, tp)):
        for dt, wt in ((0, 1 - tt), (1, tt)):
            sl = np.minimum(ip + dp, n_phi - 1) * n_theta + np.minimum(it + dt, n_theta - 1)
            for dy, wy in ((0, 1 - fy), (1, fy)):
                for dx, wx in ((0, 1 - fx), (1, fx)):
                    cols.append((sl * 3 * ny + (oy + dy)) * nx + ox + dx)
                    w.append(wp * wt * wy * wx)
    return J, np.stack(cols, -1), np.stack(w, -1)


def dense(A, wi, wo):
    """eval's matrix [3 n, texels] on LIVE pairs (rows u-major, channel fastest: E.reshape(-1) = dense @ R.reshape(-1))"""
    n_phi, n_theta, _, ny, nx = values_shape(A)
    J, cols, w = weights(A, wi, wo)
    n = len(J)
    M = np.zeros((3 * n, n_phi * n_theta * 3 * ny * nx))
    rows = np.broadcast_to(np.arange(n)[:, None], cols.shape)
    for c in range(3):
        np.add.at(M, (3 * rows + c, cols + c * ny * nx), J[:, None] * w)
    return M


def term_counts(A, wi, wo, g):
    """m_t [n_phi, n_theta, 3, ny, nx]: how many units add a non-zero term to texel t (LIVE pairs, a file without negative values)"""
    sh = values_shape(A)
    J, cols, w = weights(A, wi, wo)
    m = np.zeros(int(np.prod(sh)), np.int64)
    for c in range(3):
        on = (J[:, None] * w * np.asarray(g, np.float64)[:, c:c + 1]) != 0.0
        np.add.at(m, (cols + c * sh[3] * sh[4])[on], 1)
    return m.reshape(sh)
