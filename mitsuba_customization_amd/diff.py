"""eval as a differentiable torch operation: forward is MerlHip.eval, backward one MerlHip.ggx_grad_dir call for GGX conductors
(include/merl_hip_diff.h, mrl_ggx_grad_dir_batch), one MerlHip.table_grad_dir call for MERL / customized_measurement
tables (include/merl_hip_diff_table.h, mrl_table_grad_dir_batch), both for a batch with material ids.  After

    rgb = diff.ggx_eval(gpu, wi, wo, material=mid)        # wi, wo: [n, 3] float32 device tensors, possibly results of torch code
    loss(rgb).backward()

the gradient has flowed through eval into whatever produced wi and wo — a shading-frame rotation, a normal map, a camera pose.  The
gradient in the material's own parameters is MerlHip.ggx_grad, in a table's texels MerlHip.table_grad (fit.py).  table_eval is the
same on a table material, and eval serves either kind and batches that mix them.  table_eval_nch is MerlHip.eval_nch on n-channel
tables (include/merl_hip_diff_nch.h, mrl_table_grad_dir_batch_nch): its values are [n, n_channels]."""
from functools import partial

import torch

from . import host


def _any_backward(gpu, wi, wo, grad_rgb, mat=None, material=0, want=("wi", "wo")):
    """Single material: the gradient call of its kind (a kind without one: mrl_table_grad_dir_batch's MRL_ERR_MATERIAL).  With ids: the
    sum of the two calls — each writes exact zeros on the other's units and on units of kinds without a gradient, so the sum is exact."""
    if mat is None:
        try:
            kind = gpu.material_info(material)[0]
        except host.MerlHipError:
            kind = None
        call = gpu.ggx_grad_dir if kind == host.KIND_GGX else gpu.table_grad_dir
        return call(wi, wo, grad_rgb, material=material, want=want)
    table = gpu.table_grad_dir(wi, wo, grad_rgb, mat=mat, want=want)
    ggx = gpu.ggx_grad_dir(wi, wo, grad_rgb, mat=mat, want=want)
    return table + ggx if len(want) == 1 else tuple(t + g for t, g in zip(table, ggx))


class _Eval(torch.autograd.Function):
    """forward_call(wi, wo): an eval of the host; backward_call(wi, wo, grad, want=): the direction gradient of that eval"""
    @staticmethod
    def forward(ctx, wi, wo, forward_call, backward_call):
        wi, wo = wi.contiguous(), wo.contiguous()
        ctx.save_for_backward(wi, wo)
        ctx.backward_call = backward_call
        return forward_call(wi, wo)

    @staticmethod
    def backward(ctx, grad_values):
        wi, wo = ctx.saved_tensors
        # only what the graph asks for: the other output pointer is NULL and that gradient is neither computed nor written
        want = tuple(name for name, needed in zip(("wi", "wo"), ctx.needs_input_grad[:2]) if needed)
        grads = {}
        if want:
            out = ctx.backward_call(wi, wo, grad_values.contiguous(), want=want)
            grads = dict(zip(want, out if len(want) == 2 else (out,)))
        return grads.get("wi"), grads.get("wo"), None, None


def ggx_eval(ctx, wi, wo, mat=None, material: int = 0):
    """MerlHip.eval(wi, wo, mat, material) of the context `ctx`, differentiable in wi and wo.  The materials must be GGX conductors:
    the backward pass of a single material of another kind raises MRL_ERR_MATERIAL, and with mat= a unit whose id names no live GGX
    material receives a zero gradient."""
    return _Eval.apply(wi, wo, partial(ctx.eval, mat=mat, material=material), partial(ctx.ggx_grad_dir, mat=mat, material=material))


def table_eval(ctx, wi, wo, mat=None, material: int = 0):
    """MerlHip.eval(wi, wo, mat, material) of the context `ctx`, differentiable in wi and wo.  The materials must be RGB tables (MERL /
    customized_measurement): the backward pass of a single material of another kind raises MRL_ERR_MATERIAL, and with mat= a unit whose
    id names no live RGB table receives a zero gradient.  The gradient is the one of the trilinear interpolant in the cell eval
    selects (include/merl_hip_diff_table.h): piecewise smooth, like the function."""
    return _Eval.apply(wi, wo, partial(ctx.eval, mat=mat, material=material), partial(ctx.table_grad_dir, mat=mat, material=material))


def eval(ctx, wi, wo, mat=None, material: int = 0):
    """MerlHip.eval(wi, wo, mat, material), differentiable in wi and wo, for GGX conductors, RGB tables and batches that mix them.
    Single material: the backward pass is the gradient call of that material's kind.  With mat=: the sum of table_grad_dir and
    ggx_grad_dir, each exactly zero on the other's units; units of kinds with no gradient (n-channel, RGL, spectral, released or
    unknown ids) receive zeros."""
    return _Eval.apply(wi, wo, partial(ctx.eval, mat=mat, material=material), partial(_any_backward, ctx, mat=mat, material=material))


def table_eval_nch(ctx, wi, wo, n_channels: int, mat=None, material: int = 0):
    """MerlHip.eval_nch(wi, wo, n_channels, mat, material) of the context `ctx` — [n, n_channels] values —, differentiable in wi and wo.
    The materials must be n-channel tables of exactly n_channels channels: the backward pass of a single material of another kind or
    width raises MRL_ERR_MATERIAL, and with mat= a unit whose id names no such table receives a zero gradient.  One
    MerlHip.table_grad_dir_nch call for what the graph needs (include/merl_hip_diff_nch.h)."""
    return _Eval.apply(wi, wo, partial(ctx.eval_nch, n_channels=n_channels, mat=mat, material=material),
                       partial(ctx.table_grad_dir_nch, n_channels=n_channels, mat=mat, material=material))
