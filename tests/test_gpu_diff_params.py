"""diff.table_eval / table_eval_nch / ggx_eval / eval with tables= and params=: eval differentiable in the material.  Forward writes the
tensor into its resident material in place when the tensor has changed; backward is the adjoint call the host already has.  The bars:
a table gradient against a direct table_grad call within 1e-12 S (S = sum_u |a_u g_u| from the numpy reference, the bar two runs of
the adjoint are compared at in test_gpu_table_grad.py); a GGX parameter gradient against ggx_grad bit for bit (that sum is
deterministic)."""
import numpy as np
import pytest

from tests import table_grad_nch_reference as nref
from tests import table_grad_reference as ref

pytestmark = pytest.mark.gpu

SCALE = (0.7, 1.3, 2.1)
SMALL, LARGE = (7, 5, 12), (33, 17, 64)
N = 1 << 14


def _ctx(negative=1, lookup=1, node=0):
    from mitsuba_customization_amd import host
    g = host.MerlHip(0)
    g.set_option(host.OPT_NEGATIVE, negative); g.set_option(host.OPT_LOOKUP, lookup); g.set_option(host.OPT_NODE, node)
    return g


def _inputs(gpu, seed, n=N, width=3):
    import torch
    wi, wo, _ = gpu.generate_pairs(seed, 0, n)
    g = torch.from_numpy(np.random.default_rng(seed).standard_normal((n, width)).astype(np.float32)).cuda()
    return wi, wo, g


def _table(seed, dims, n_ch=3):
    """values of both signs (the iterates of a fit have them)"""
    return np.random.default_rng(seed).standard_normal((n_ch,) + tuple(dims)) * 50.0 + 20.0


def _param(a):
    import torch
    return torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda())


def _bits_equal(a, b):
    import torch
    return bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def _within(got, direct, S, what, factor=1e-12):
    got, direct = got.detach().cpu().numpy(), direct.detach().cpu().numpy()
    err = np.abs(got - direct)
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = float(np.nanmax(np.where(S > 0, err / S, 0.0)))
    print(f"{what}: worst |autograd - direct| / S = {worst:.3e}; cells reached {int((S > 0).sum())}")
    assert (err <= factor * S).all(), (what, worst)
    assert np.abs(direct).max() > 0


def _counting(gpu, name):
    calls = []
    inner = getattr(gpu, name)

    def wrapper(*a, **k):
        calls.append(a)
        return inner(*a, **k)
    setattr(gpu, name, wrapper)
    return calls


@pytest.mark.parametrize("negative", (0, 1))
@pytest.mark.parametrize("dims", (SMALL, LARGE))
def test_table_gradient_is_the_adjoint_call(dims, negative):
    from mitsuba_customization_amd import diff
    with _ctx(negative) as gpu:
        mid = gpu.upload_table(np.ones((3,) + dims), SCALE)
        wi, wo, g = _inputs(gpu, 101)
        T = _param(_table(1, dims))
        rgb = diff.table_eval(gpu, wi, wo, material=mid, tables=T)
        (rgb * g).sum().backward()
        direct = gpu.table_grad(wi, wo, g, material=mid)
        _, S = ref.adjoint(wi.cpu().numpy(), wo.cpu().numpy(), g.cpu().numpy(), dims, scale=SCALE)
        _within(T.grad, direct, S, f"dims {dims} negative {negative}")
        if negative == 1:
            # A is linear in T under keep: the dot test <A T, g> = <T, A^T g>, to 1e-6 of the sum of the |terms| (eval is f32)
            lhs_terms = rgb.detach().double() * g.double()
            lhs, rhs = float(lhs_terms.sum()), float((T.detach() * T.grad).sum())
            scale = float(lhs_terms.abs().sum())
            print(f"dot test: <A T, g> = {lhs:.9e}, <T, A^T g> = {rhs:.9e}, sum |terms| = {scale:.3e}")
            assert abs(lhs - rhs) <= 1e-6 * scale


def test_direction_and_table_gradients_from_one_backward():
    from mitsuba_customization_amd import diff
    dims = LARGE
    with _ctx() as gpu:
        mid = gpu.upload_table(np.ones((3,) + dims), SCALE)
        wi, wo, g = _inputs(gpu, 102)
        wi.requires_grad_(True); wo.requires_grad_(True)
        T = _param(_table(2, dims))
        grad_calls, dir_calls = _counting(gpu, "table_grad"), _counting(gpu, "table_grad_dir")
        (diff.table_eval(gpu, wi, wo, material=mid, tables=T) * g).sum().backward()
        assert len(grad_calls) == 1 and len(dir_calls) == 1
        want_wi, want_wo = gpu.table_grad_dir(wi.detach(), wo.detach(), g, material=mid)
        assert _bits_equal(wi.grad, want_wi) and _bits_equal(wo.grad, want_wo)
        _, S = ref.adjoint(wi.detach().cpu().numpy(), wo.detach().cpu().numpy(), g.cpu().numpy(), dims, scale=SCALE)
        _within(T.grad, gpu.table_grad(wi.detach(), wo.detach(), g, material=mid), S, "with directions")
        # only what the graph needs: a table that needs no gradient costs no adjoint call, and the old calls behave as before
        del grad_calls[:], dir_calls[:]
        wi.grad = wo.grad = None
        (diff.table_eval(gpu, wi, wo, material=mid, tables=T.detach()) * g).sum().backward()
        assert len(grad_calls) == 0 and len(dir_calls) == 1 and _bits_equal(wi.grad, want_wi)
        wi.grad = None
        (diff.table_eval(gpu, wi, wo, material=mid) * g).sum().backward()
        assert _bits_equal(wi.grad, want_wi)


def test_forward_updates_only_when_the_tensor_has_changed():
    import torch
    from mitsuba_customization_amd import diff
    dims = SMALL
    with _ctx() as gpu, _ctx() as fresh:
        mid = gpu.upload_table(np.ones((3,) + dims), SCALE)
        wi, wo, _ = _inputs(gpu, 103)
        T = _param(_table(3, dims))
        updates = _counting(gpu, "update_table")

        def fresh_eval(values):
            m = fresh.upload_table(values.detach().cpu().numpy(), SCALE)
            try:
                return fresh.eval(wi, wo, material=m).clone()
            finally:
                fresh.release_material(m)
        first = diff.table_eval(gpu, wi, wo, material=mid, tables=T)
        assert len(updates) == 1 and _bits_equal(first, fresh_eval(T))
        again = diff.table_eval(gpu, wi, wo, material=mid, tables=T)
        assert len(updates) == 1 and _bits_equal(again, first)                  # unchanged: no update
        with torch.no_grad():
            T.add_(0.5)
        moved = diff.table_eval(gpu, wi, wo, material=mid, tables=T)
        assert len(updates) == 2 and _bits_equal(moved, fresh_eval(T)) and not _bits_equal(moved, first)
        # another tensor, and someone else's update of the material, are noticed too
        other = _param(_table(4, dims))
        assert _bits_equal(diff.table_eval(gpu, wi, wo, material=mid, tables=other), fresh_eval(other)) and len(updates) == 3
        assert _bits_equal(diff.table_eval(gpu, wi, wo, material=mid, tables=T), moved) and len(updates) == 4
        gpu.update_table(mid, other.detach())
        assert _bits_equal(diff.table_eval(gpu, wi, wo, material=mid, tables=T), moved) and len(updates) == 6
        with pytest.raises(ValueError):
            diff.table_eval(gpu, wi, wo, material=mid, tables=T.detach().float())
        with pytest.raises(ValueError):
            diff.table_eval(gpu, wi, wo, material=mid, tables=_param(_table(3, LARGE)))


def test_dict_form_serves_two_tables_of_different_dims_in_one_batch():
    import torch
    from mitsuba_customization_amd import diff
    with _ctx() as gpu:
        m0, m1 = gpu.upload_table(np.ones((3,) + SMALL), SCALE), gpu.upload_table(np.ones((3,) + LARGE), SCALE)
        ggx = gpu.ggx(0.2, (0.2, 0.9, 1.1), (3.9, 2.4, 2.2))
        wi, wo, g = _inputs(gpu, 104)
        mat = torch.tensor([m0, m1, ggx], dtype=torch.int32, device="cuda")[torch.arange(N, device="cuda") % 3].contiguous()
        T0, T1 = _param(_table(5, SMALL)), _param(_table(6, LARGE))
        launches = _counting(gpu, "table_grad_mat")
        rgb = diff.table_eval(gpu, wi, wo, mat=mat, tables={m0: T0, m1: T1})
        (rgb * g).sum().backward()
        assert len(launches) == 1
        d0, d1 = gpu.table_grad_mat(wi, wo, g, [m0, m1], mat=mat)
        hwi, hwo, hg, hmat = wi.cpu().numpy(), wo.cpu().numpy(), g.cpu().numpy(), mat.cpu().numpy()
        for T, direct, mid, dims in ((T0, d0, m0, SMALL), (T1, d1, m1, LARGE)):
            at = hmat == mid
            _, S = ref.adjoint(hwi[at], hwo[at], hg[at], dims, scale=SCALE)
            _within(T.grad, direct, S, f"table {mid}")
        # the forward is the batch's: each table's units see their own tensor
        gpu.update_table(m0, T0.detach()); gpu.update_table(m1, T1.detach())
        assert _bits_equal(rgb, gpu.eval(wi, wo, mat=mat))
        # one table of the two needs a gradient: the launch has one target
        T0.grad = None
        (diff.eval(gpu, wi, wo, mat=mat, tables={m0: T0, m1: T1.detach()}) * g).sum().backward()
        assert len(launches[-1][3]) == 1 and T0.grad is not None


@pytest.mark.parametrize("n_ch", (4, 16))
def test_n_channel_tables(n_ch):
    from mitsuba_customization_amd import diff
    dims = SMALL
    scale = nref.scales(n_ch)
    with _ctx() as gpu, _ctx() as fresh:
        mid = gpu.upload_table_nch(np.ones((n_ch,) + dims), list(scale))
        wi, wo, g = _inputs(gpu, 105, width=n_ch)
        T = _param(_table(7, dims, n_ch))
        values = diff.table_eval_nch(gpu, wi, wo, n_ch, material=mid, tables=T)
        (values * g).sum().backward()
        ref_mid = fresh.upload_table_nch(T.detach().cpu().numpy(), list(scale))
        assert _bits_equal(values, fresh.eval_nch(wi, wo, n_ch, material=ref_mid))
        (direct,) = gpu.table_grad_nch(wi, wo, g, n_ch, [mid], material=mid)
        _, S = nref.adjoint_nch(wi.cpu().numpy(), wo.cpu().numpy(), g.cpu().numpy(), dims, scale=scale)
        _within(T.grad, direct, S, f"{n_ch} channels")


def test_ggx_parameters():
    import torch
    from mitsuba_customization_amd import diff
    true = np.array([0.2, 0.2, 0.9, 1.1, 3.9, 2.4, 2.2])
    with _ctx() as gpu, _ctx() as fresh:
        mid = gpu.ggx(0.5, (1, 1, 1), (1, 1, 1))
        other = gpu.ggx(0.3, (1.2, 0.8, 0.5), (2.0, 2.5, 3.0))
        wi, wo, g = _inputs(gpu, 106)
        P = _param(true * 1.1)
        updates = _counting(gpu, "update_ggx")
        rgb = diff.ggx_eval(gpu, wi, wo, material=mid, params=P)
        (rgb * g).sum().backward()
        p = P.detach().cpu().numpy()
        ref_mid = fresh.ggx(float(p[0]), p[1:4], p[4:7])
        assert _bits_equal(rgb, fresh.eval(wi, wo, material=ref_mid))
        direct = gpu.ggx_grad(wi, wo, g, mid)
        assert _bits_equal(P.grad, direct) and float(direct.abs().max()) > 0
        diff.ggx_eval(gpu, wi, wo, material=mid, params=P)
        assert len(updates) == 1                                                # unchanged: no update
        # with material ids: two conductors, one launch, each row its own material's sums
        mat = torch.tensor([mid, other], dtype=torch.int32, device="cuda")[torch.arange(N, device="cuda") % 2].contiguous()
        Q = _param(np.array([0.3, 1.2, 0.8, 0.5, 2.0, 2.5, 3.0]))
        P.grad = None
        (diff.eval(gpu, wi, wo, mat=mat, params={mid: P, other: Q}) * g).sum().backward()
        rows = gpu.ggx_grad_mat(wi, wo, g, [mid, other], mat=mat)
        assert _bits_equal(P.grad, rows[0]) and _bits_equal(Q.grad, rows[1])
        # five Adam steps from the perturbed start lower the loss
        y = fresh.eval(wi, wo, material=fresh.ggx(float(true[0]), true[1:4], true[4:7])).clone()
        opt = torch.optim.Adam([P], lr=2e-3)
        losses = []
        for _ in range(6):
            opt.zero_grad()
            loss = ((diff.ggx_eval(gpu, wi, wo, material=mid, params=P) - y) ** 2).sum()
            losses.append(float(loss.detach()))
            if len(losses) <= 5:
                loss.backward()
                opt.step()
        print("Adam on the GGX parameters:", " ".join(f"{v:.6e}" for v in losses))
        assert losses[5] < losses[0]


def test_example_fit_table_adam_fills_the_cells_no_measurement_reaches():
    """examples/fit_table_adam.py: the data term falls, and on the cells no unit reaches — where the splat leaves zeros, so that its
    error there is the truth's own rms — the regularised table is closer to the truth than zeros are."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import fit_table_adam as example
    with _ctx() as gpu:
        truth, wi, wo, y = example.measurements(gpu, 1 << 8)                 # 8 corners each: at most 2048 of the 6912 cells
        T, history = example.fit(gpu, wi, wo, y, steps=60)
        r = example.report(gpu, truth, T, wi, wo, y)
    print(f"data term {history[0]:.4e} -> {history[-1]:.4e}; reached {r['reached_cells']} of {r['cells']}; unreached rms: Adam "
          f"{r['adam_unreached']:.4e}, zeros {r['splat_unreached']:.4e}")
    assert r["reached_cells"] < r["cells"] // 2                              # sparse
    assert history[-1] < history[0]
    assert r["splat_unreached"] == r["truth_rms_unreached"] and r["adam_unreached"] < r["truth_rms_unreached"]
