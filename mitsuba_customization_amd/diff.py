"""eval of GGX conductors as a differentiable torch operation: forward is MerlHip.eval, backward one MerlHip.ggx_grad_dir call
(include/merl_hip_diff.h, mrl_ggx_grad_dir_batch).  After

    rgb = diff.ggx_eval(gpu, wi, wo, material=mid)        # wi, wo: [n, 3] float32 device tensors, possibly results of torch code
    loss(rgb).backward()

the gradient has flowed through eval into whatever produced wi and wo — a shading-frame rotation, a normal map, a camera pose.  The
gradient in the material's own parameters is MerlHip.ggx_grad (fit.py)."""
import torch


class _GgxEval(torch.autograd.Function):
    @staticmethod
    def forward(ctx, wi, wo, gpu, mat, material):
        wi, wo = wi.contiguous(), wo.contiguous()
        ctx.save_for_backward(wi, wo)
        ctx.gpu, ctx.mat, ctx.material = gpu, mat, material
        return gpu.eval(wi, wo, mat=mat, material=material)

    @staticmethod
    def backward(ctx, grad_rgb):
        wi, wo = ctx.saved_tensors
        # only what the graph asks for: the other output pointer is NULL and that gradient is neither computed nor written
        want = tuple(name for name, needed in zip(("wi", "wo"), ctx.needs_input_grad[:2]) if needed)
        grads = {}
        if want:
            out = ctx.gpu.ggx_grad_dir(wi, wo, grad_rgb.contiguous(), mat=ctx.mat, material=ctx.material, want=want)
            grads = dict(zip(want, out if len(want) == 2 else (out,)))
        return grads.get("wi"), grads.get("wo"), None, None, None


def ggx_eval(ctx, wi, wo, mat=None, material: int = 0):
    """MerlHip.eval(wi, wo, mat, material) of the context `ctx`, differentiable in wi and wo.  The materials must be GGX conductors:
    the backward pass of a single material of another kind raises MRL_ERR_MATERIAL, and with mat= a unit whose id names no live GGX
    material receives a zero gradient."""
    return _GgxEval.apply(wi, wo, ctx, mat, material)
