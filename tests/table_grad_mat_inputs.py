"""Inputs and the reference of the multi-material table adjoint (include/merl_hip_fit_table.h, mrl_table_grad_batch_mat /
mrl_table_grad_queue), shared by tests/test_table_grad_mat_cpu.py (which checks them on the reference alone) and
tests/test_gpu_table_grad_mat.py.  Everything is built from tests/table_grad_reference.py: a unit whose cell must not be in doubt
is a ref.interior unit of the pool generate_pairs(0x5EED, 0, 1 << 16) for that unit's OWN material, and the reference of the
multi-material operator is ref.adjoint per target on the units that carry that target's id."""
import functools

import numpy as np

from tests import table_grad_reference as ref

SCALES = ((0.7, 1.3, 2.1), (1.9, 0.6, 1.1), (1.0, 2.5, 0.4), (0.8, 0.9, 1.7))
# (dims, param) of the targets of the mixed test; of the thin test (a quiet target between them: no unit carries its id)
MIXED = (((7, 5, 12), ref.HALF_DIFF), ((9, 4, 6), ref.STANDARD), ((33, 17, 64), ref.STANDARD_FULL))
THIN = (((1, 1, 1), ref.HALF_DIFF), ((7, 5, 12), ref.HALF_DIFF), ((5, 1, 2), ref.STANDARD), ((2, 3, 1), ref.HALF_DIFF))
THIN_QUIET = 1
SAME = ((7, 5, 12), ref.HALF_DIFF)
# roles of a unit beyond "target k": its id names another table, a GGX, a released material, is -1, is out of range
OTHERS = ("table", "ggx", "released", "negative", "out of range")
BASE = 1021


@functools.lru_cache(maxsize=None)
def pool():
    from oracle import binding
    wi, wo, _ = binding.generate_pairs(0x5EED, 0, 1 << 16)
    wi = np.ascontiguousarray(wi, np.float32); wo = np.ascontiguousarray(wo, np.float32)
    wi.setflags(write=False); wo.setflags(write=False)
    return wi, wo


def cells(specs):
    return [int(np.prod(dims)) for dims, _ in specs]


@functools.lru_cache(maxsize=None)
def interleaved(specs, center, n, quiet=(), others=True):
    """(wi, wo, g, role) of n units, roles lane by lane in turn: target 0, 1, .. (those in `quiet` left out), then OTHERS.  A unit
    of target k is the next unit of ref.sequence for k's dims and parameterisation (interior pool units, every 9th dead); a unit of
    another role takes target 0's.  g: random, NaN / inf in the rows of dead units and of every unit that is no target's.
    role: the target's index, or len(specs) + index into OTHERS.  Shared, read-only."""
    roles = [k for k in range(len(specs)) if k not in quiet] + ([len(specs) + j for j in range(len(OTHERS))] if others else [])
    per = -(-n // len(roles))
    seqs = [ref.sequence(*pool(), dims, param, center, per) for dims, param in specs]
    role = np.array([roles[i % len(roles)] for i in range(n)])
    wi = np.empty((n, 3), np.float32); wo = np.empty((n, 3), np.float32)
    for i in range(n):
        s = seqs[role[i]] if role[i] < len(specs) else seqs[roles[0]]
        wi[i], wo[i] = s[0][i // len(roles)], s[1][i // len(roles)]
    g = ref.poisoned(np.random.default_rng(n).standard_normal((n, 3)), wi, wo)
    stray = np.nonzero(role >= len(specs))[0]
    g[stray[0::2]] = np.nan; g[stray[1::2]] = np.inf
    for a in (wi, wo, g, role):
        a.setflags(write=False)
    return wi, wo, g, role


def reference(wi, wo, g, role, specs, lookup, node, cosine=True):
    """[(R_k, S_k)]: ref.adjoint per target on the units that carry its id, with its dims, parameterisation and scale."""
    out = []
    for k, (dims, param) in enumerate(specs):
        at = np.asarray(role) == k
        out.append(ref.adjoint(wi[at], wo[at], g[at], dims, param=param, trilinear=bool(lookup), center=bool(node), cosine=cosine,
                               scale=SCALES[k % len(SCALES)]))
    return out


def ids_of(role, target_ids, other_ids):
    """The material id of every unit: target_ids[k] for role k, other_ids[name] for the OTHERS."""
    table = np.array(list(target_ids) + [other_ids[name] for name in OTHERS], np.int32)
    return np.ascontiguousarray(table[np.asarray(role)])


# ---- one wave on one cell, shared between two tables of the same dims ----
SAME_PATTERNS = ("alternating", "halves", "four")


@functools.lru_cache(maxsize=None)
def one_cell_wave(center):
    """(wi, wo): 64 interior pool units of SAME that all fall into one cell, the fullest of the pool."""
    wi, wo = pool()
    dims, param = SAME
    inside = np.nonzero(ref.interior(wi, wo, dims, param, center))[0]
    cell = ref.cell_index(wi[inside], wo[inside], dims, param, center)
    best = int(np.argmax(np.bincount(cell)))
    pick = inside[cell == best][:ref.WAVE]
    assert len(pick) == ref.WAVE
    return np.array(wi[pick], np.float32), np.array(wo[pick], np.float32)


def same_pattern(name):
    """role per lane: 0 = table A, 1 = table B."""
    lanes = np.arange(ref.WAVE)
    if name == "alternating":
        return lanes % 2
    if name == "halves":
        return (lanes >= 32).astype(int)
    if name == "four":
        return (lanes >= 4).astype(int)
    raise ValueError(name)


# ---- a queue over BASE slots: permuted, one slot listed twice, one skipped ----
@functools.lru_cache(maxsize=None)
def queue_slots():
    q = np.random.default_rng(77).permutation(BASE).astype(np.int32)
    at = int(np.nonzero(q == 8)[0][0])             # slot 8 of interleaved(): a live unit of target 0 — it becomes the doubled one
    q[at], q[3] = q[3], q[at]
    q[10] = q[3]                                   # slot q[3] twice among the first 600; the slot q[10] named is skipped by every count
    q.setflags(write=False)
    return q
