"""eval as a differentiable torch operation: forward is MerlHip.eval, backward one MerlHip.ggx_grad_dir call for GGX conductors
(include/merl_hip_diff.h, mrl_ggx_grad_dir_batch), one MerlHip.table_grad_dir call for MERL / customized_measurement
tables (include/merl_hip_diff_table.h, mrl_table_grad_dir_batch), one MerlHip.rgl_grad_dir call for RGB RGL materials
(include/merl_hip_diff_rgl.h, mrl_rgl_grad_dir_batch), their sum for a batch with material ids.  After

    rgb = diff.ggx_eval(gpu, wi, wo, material=mid)        # wi, wo: [n, 3] float32 device tensors, possibly results of torch code
    loss(rgb).backward()

the gradient has flowed through eval into whatever produced wi and wo — a shading-frame rotation, a normal map, a camera pose.  The
gradient in the material's own parameters is MerlHip.ggx_grad, in a table's texels MerlHip.table_grad (fit.py).  table_eval is the
same on a table material, rgl_eval on an RGL material, and eval serves every one of these kinds and batches that mix them.  table_eval_nch is MerlHip.eval_nch on n-channel
tables (include/merl_hip_diff_nch.h, mrl_table_grad_dir_batch_nch): its values are [n, n_channels].
rgl_spectral_eval is MerlHip.eval_spectral on spectral RGL materials (include/merl_hip_diff_rgl_spectral.h,
mrl_rgl_grad_dir_spectral_batch): [n, W] values at per-unit wavelengths, differentiable in the wavelengths as well,
and with values= in the files' spectra (include/merl_hip_fit_rgl_spectral.h).

tables= and params= make the same calls differentiable in the MATERIAL as well: the table tensor(s) behind table
materials, the 7 parameters behind GGX conductors.  Forward writes a tensor's current values into its resident material in place
(MerlHip.update_table / update_ggx, include/merl_hip_update.h) — only when the tensor has changed since that material last received
it — and evaluates as before; backward adds the adjoint calls (table_grad*, ggx_grad*) for the tensors that need a gradient:

    T = torch.nn.Parameter(start)                          # f64 [3, n_th, n_td, n_pd] on the device; `mid` was uploaded with these dims
    loss = ((diff.table_eval(gpu, wi, wo, material=mid, tables=T) - y) ** 2).sum() + smoothness(T)
    loss.backward()                                        # T.grad = A^T dL/d eval + the regulariser's own gradient"""
import weakref
from functools import partial

import torch

from . import host


def _any_backward(gpu, wi, wo, grad_rgb, mat=None, material=0, want=("wi", "wo")):
    """Single material: the gradient call of its kind (a kind without one: mrl_table_grad_dir_batch's MRL_ERR_MATERIAL).  With ids: the
    sum of the table and the GGX call — each writes exact zeros on the other's units and on units of kinds without a gradient, so the
    sum is exact — and, only when the context holds a live RGB RGL material, of the RGL call as a third: a context without one makes
    exactly the two calls it made before RGL materials had a gradient."""
    if mat is None:
        try:
            kind = gpu.material_info(material)[0]
        except host.MerlHipError:
            kind = None
        call = gpu.ggx_grad_dir if kind == host.KIND_GGX else gpu.rgl_grad_dir if kind == host.KIND_RGL else gpu.table_grad_dir
        return call(wi, wo, grad_rgb, material=material, want=want)
    table = gpu.table_grad_dir(wi, wo, grad_rgb, mat=mat, want=want)
    ggx = gpu.ggx_grad_dir(wi, wo, grad_rgb, mat=mat, want=want)
    parts = [table, ggx] + ([gpu.rgl_grad_dir(wi, wo, grad_rgb, mat=mat, want=want)] if _holds_rgl(gpu) else [])
    if len(want) == 1:
        return sum(parts[1:], parts[0])
    return tuple(sum(side[1:], side[0]) for side in zip(*parts))


def _rgl_ids(gpu):
    """the ids of the context's live RGB RGL materials, ascending  (a released slot has no info: MerlHipError)"""
    ids = []
    for mid in range(gpu.material_count()):
        try:
            if gpu.material_info(mid)[0] == host.KIND_RGL:
                ids.append(mid)
        except host.MerlHipError:
            pass
    return ids


def _holds_rgl(gpu):
    """does the context hold a live RGB RGL material?"""
    return bool(_rgl_ids(gpu))


class _Eval(torch.autograd.Function):
    """forward_call(wi, wo): an eval of the host; backward_call(wi, wo, grad, want=): the direction gradient of that eval;
    material_call(wi, wo, grad, needed): the gradients in `values` — the tensors behind the materials (_Materials) — for the
    positions listed in `needed`, as a list aligned with values (None elsewhere)"""
    @staticmethod
    def forward(ctx, wi, wo, forward_call, backward_call, material_call=None, *values):
        wi, wo = wi.contiguous(), wo.contiguous()
        ctx.save_for_backward(wi, wo)
        ctx.backward_call = backward_call
        ctx.material_call = material_call
        ctx.n_values = len(values)
        return forward_call(wi, wo)

    @staticmethod
    def backward(ctx, grad_values):
        wi, wo = ctx.saved_tensors
        # only what the graph asks for: the other output pointer is NULL and that gradient is neither computed nor written
        want = tuple(name for name, needed in zip(("wi", "wo"), ctx.needs_input_grad[:2]) if needed)
        g = grad_values.contiguous()
        grads = {}
        if want:
            out = ctx.backward_call(wi, wo, g, want=want)
            grads = dict(zip(want, out if len(want) == 2 else (out,)))
        needed = [i for i, need in enumerate(ctx.needs_input_grad[5:]) if need]
        in_values = ctx.material_call(wi, wo, g, needed) if needed else [None] * ctx.n_values
        return (grads.get("wi"), grads.get("wo"), None, None, None, *in_values)


class _SpectralEval(torch.autograd.Function):
    """_Eval's sibling with a third differentiable input, the per-unit wavelengths [n, W]: forward_call(wi, wo, wavelengths) is a
    spectral eval of the host, backward_call(wi, wo, wavelengths, grad, want=) its gradient for a subset of ("wi", "wo",
    "wavelengths")"""
    @staticmethod
    def forward(ctx, wi, wo, wavelengths, forward_call, backward_call, material_call=None, *values):
        wi, wo, wavelengths = wi.contiguous(), wo.contiguous(), wavelengths.contiguous()
        ctx.save_for_backward(wi, wo, wavelengths)
        ctx.backward_call = backward_call
        ctx.material_call = material_call                       # (wi, wo, wavelengths, grad, needed) -> the gradients in `values`
        ctx.n_values = len(values)
        return forward_call(wi, wo, wavelengths)

    @staticmethod
    def backward(ctx, grad_values):
        wi, wo, wavelengths = ctx.saved_tensors
        # only what the graph asks for: the other output pointers are NULL and those gradients are neither computed nor written
        want = tuple(name for name, needed in zip(("wi", "wo", "wavelengths"), ctx.needs_input_grad[:3]) if needed)
        g = grad_values.contiguous()
        grads = {}
        if want:
            out = ctx.backward_call(wi, wo, wavelengths, g, want=want)
            grads = dict(zip(want, (out,) if len(want) == 1 else out))
        needed = [i for i, need in enumerate(ctx.needs_input_grad[6:]) if need]
        in_values = ctx.material_call(wi, wo, wavelengths, g, needed) if needed else [None] * ctx.n_values
        return (grads.get("wi"), grads.get("wo"), grads.get("wavelengths"), None, None, None, *in_values)


class _SpectralValues:
    """The spectra tensors behind the spectral RGL materials of one rgl_spectral_eval call: {material id: tensor}.  refresh() makes
    every material hold its tensor's current values (the record of _Materials.refresh, shared with it); gradients() is
    _SpectralEval's material_call: one MerlHip.rgl_spectral_values_grad launch for all tensors that need a gradient."""

    def __init__(self, gpu, mat, material, values):
        self.gpu, self.mat, self.material = gpu, mat, material
        self.entries = [(int(k), t) for k, t in (values.items() if isinstance(values, dict) else [(material, values)])]
        for _, t in self.entries:
            if not torch.is_tensor(t) or t.dtype not in (torch.float32, torch.float64):
                raise ValueError("values=: torch.float32 or torch.float64 tensors [n_phi, n_theta, n_wl, ny, nx]")

    @property
    def values(self):
        return tuple(t for _, t in self.entries)

    def refresh(self):
        record = self.gpu.__dict__.setdefault("_resident", {})
        self.gpu.use_torch_stream()                             # the updates run on the stream the eval behind them will run on
        for mid, t in self.entries:
            seen = record.get(mid)
            if seen is not None and seen[0]() is t and seen[1:] == (t.data_ptr(), t._version):
                continue
            self.gpu.update_rgl_spectral_values(mid, t.detach().to(torch.float32).contiguous())   # rounded once, on the device
            record[mid] = (weakref.ref(t), t.data_ptr(), t._version)

    def gradients(self, wi, wo, wavelengths, g, needed):
        out = [None] * len(self.entries)
        grads = self.gpu.rgl_spectral_values_grad(wi, wo, wavelengths, g, [self.entries[i][0] for i in needed], mat=self.mat, material=self.material)
        for i, grad in zip(needed, grads):
            out[i] = grad.to(self.entries[i][1].dtype)
        return out


class _Materials:
    """The tensors behind the materials of one differentiable call: entries (kind "table" / "ggx" / "rgl", material id, tensor).
    refresh() makes every material hold its tensor's current values; gradients() is _Eval's material_call."""

    def __init__(self, gpu, mat, material, tables, params, n_channels=None, values=None):
        self.gpu, self.mat, self.material, self.n_channels = gpu, mat, material, n_channels
        as_dict = lambda v: {} if v is None else ({int(k): t for k, t in v.items()} if isinstance(v, dict) else {int(material): v})
        if isinstance(values, (list, tuple)):                   # one tensor per live RGB RGL material of the context, in the order of their ids
            ids = _rgl_ids(gpu)
            if len(ids) != len(values):
                raise ValueError(f"values=: {len(values)} tensors for the context's {len(ids)} RGB RGL materials (or pass {{id: tensor}})")
            values = dict(zip(ids, values))
        self.entries = [("table", k, t) for k, t in as_dict(tables).items()] + [("ggx", k, t) for k, t in as_dict(params).items()] + \
                       [("rgl", k, t) for k, t in as_dict(values).items()]
        for kind, _, t in self.entries:
            if kind == "rgl":
                if not torch.is_tensor(t) or t.dtype not in (torch.float32, torch.float64):
                    raise ValueError("values=: torch.float32 or torch.float64 tensors [n_phi, n_theta, 3, ny, nx]")
                continue
            if not torch.is_tensor(t) or t.dtype != torch.float64:
                raise ValueError("tables= / params=: torch.float64 tensors")
            if kind == "ggx" and tuple(t.shape) != (7,):
                raise ValueError("params=: [7] tensors (alpha, eta rgb, k rgb)")

    @property
    def values(self):
        return tuple(t for _, _, t in self.entries)

    def refresh(self):
        # the record lives on the context object: per material the tensor (weakly: an address is reused after a tensor dies), its
        # address and its version when the material last received it.  MerlHip.update_* and release_material forget a material
        record = self.gpu.__dict__.setdefault("_resident", {})
        self.gpu.use_torch_stream()                             # the updates run on the stream the eval behind them will run on
        for kind, mid, t in self.entries:
            seen = record.get(mid)
            if seen is not None and seen[0]() is t and seen[1:] == (t.data_ptr(), t._version):
                continue
            if kind == "table":
                self.gpu.update_table(mid, t.detach(), keep_sampling=True)
            elif kind == "rgl":                                 # the image holds Floats: an f64 tensor is rounded once, on the device
                self.gpu.update_rgl_values(mid, t.detach().to(torch.float32).contiguous())
            else:
                p = t.detach().cpu().tolist()                   # 7 values to the host: waits for whatever computes them
                self.gpu.update_ggx(mid, p[0], p[1:4], p[4:7])
            record[mid] = (weakref.ref(t), t.data_ptr(), t._version)

    def gradients(self, wi, wo, g, needed):
        gpu, out = self.gpu, [None] * len(self.entries)
        tables = [i for i in needed if self.entries[i][0] == "table"]
        ggx = [i for i in needed if self.entries[i][0] == "ggx"]
        if tables:
            ids = [self.entries[i][1] for i in tables]
            if self.n_channels is not None:
                grads = gpu.table_grad_nch(wi, wo, g, self.n_channels, ids, mat=self.mat, material=self.material)
            elif self.mat is None and ids == [self.material]:
                grads = (gpu.table_grad(wi, wo, g, material=self.material),)
            else:                                               # one launch for all targets, split by table_grad_layout
                grads = gpu.table_grad_mat(wi, wo, g, ids, mat=self.mat, material=self.material)
            for i, grad in zip(tables, grads):
                out[i] = grad
        rgl = [i for i in needed if self.entries[i][0] == "rgl"]
        if rgl:                                                 # one launch for all targets, split by rgl_values_grad_layout
            grads = gpu.rgl_values_grad(wi, wo, g, [self.entries[i][1] for i in rgl], mat=self.mat, material=self.material)
            for i, grad in zip(rgl, grads):
                out[i] = grad.to(self.entries[i][2].dtype)
        if ggx:
            ids = [self.entries[i][1] for i in ggx]
            if self.mat is None and ids == [self.material]:
                grads = (gpu.ggx_grad(wi, wo, g, self.material),)
            else:
                grads = gpu.ggx_grad_mat(wi, wo, g, ids, mat=self.mat, material=self.material)
            for i, grad in zip(ggx, grads):
                out[i] = grad.to(self.entries[i][2].device)
        return out


def _apply(gpu, wi, wo, forward_call, backward_call, mat, material, tables=None, params=None, n_channels=None, values=None):
    if tables is None and params is None and values is None:
        return _Eval.apply(wi, wo, forward_call, backward_call, None)
    m = _Materials(gpu, mat, material, tables, params, n_channels, values)
    m.refresh()
    return _Eval.apply(wi, wo, forward_call, backward_call, m.gradients, *m.values)


def _per_material_sums(gpu, per_unit, mat, ids, values):
    """The per-unit parameter gradients of a pdf / sample gradient call — [n, 7] f32, or [n] for grad_alpha — summed in f64 on the device
    into one [7] (or scalar) per tensor of `values` (the materials `ids`): the whole array for a call on one material, index_add_ by id
    for a call with ids (a unit whose id names nothing in range adds nothing: its row is zero anyway)."""
    rows = per_unit.double()
    if mat is None:
        total = rows.sum(0)
        return [total.to(t.device) for t in values]
    count = gpu.material_count()
    ok = (mat >= 0) & (mat < count)
    sums = torch.zeros((count,) + tuple(rows.shape[1:]), dtype=torch.float64, device=rows.device)
    sums.index_add_(0, torch.where(ok, mat, torch.zeros_like(mat)).long(), torch.where(ok.reshape((-1,) + (1,) * (rows.dim() - 1)), rows, torch.zeros_like(rows)))
    return [sums[mid].to(t.device) for mid, t in zip(ids, values)]


class _GgxPdf(torch.autograd.Function):
    """forward MerlHip.pdf, backward one MerlHip.ggx_pdf_grad call for the outputs the graph needs (include/merl_hip_diff_sample.h)"""
    @staticmethod
    def forward(ctx, wi, wo, gpu, mat, material, ids, *values):
        wi, wo = wi.contiguous(), wo.contiguous()
        ctx.save_for_backward(wi, wo)
        ctx.call = (gpu, mat, material, ids)
        ctx.values = values
        return gpu.pdf(wi, wo, mat=mat, material=material)

    @staticmethod
    def backward(ctx, grad_pdf):
        wi, wo = ctx.saved_tensors
        gpu, mat, material, ids = ctx.call
        in_values = [None] * len(ctx.values)
        needed = [i for i, need in enumerate(ctx.needs_input_grad[6:]) if need]
        # only what the graph asks for: the other output pointers are NULL and those gradients are neither computed nor written
        want = tuple(name for name, need in zip(("wi", "wo", "alpha"), (*ctx.needs_input_grad[:2], bool(needed))) if need)
        grads = {}
        if want:
            out = gpu.ggx_pdf_grad(wi, wo, grad_pdf.contiguous(), mat=mat, material=material, want=want)
            grads = dict(zip(want, (out,) if len(want) == 1 else out))
        if needed:                                              # the pdf depends on alpha alone: entry 0 of a tensor's gradient
            sums = _per_material_sums(gpu, grads["alpha"], mat, ids, ctx.values)
            for i in needed:
                in_values[i] = torch.zeros(7, dtype=torch.float64, device=sums[i].device)
                in_values[i][0] = sums[i]
        return (grads.get("wi"), grads.get("wo"), None, None, None, None, *in_values)


class _GgxSample(torch.autograd.Function):
    """forward MerlHip.sample -> (wo, pdf, weight), backward one MerlHip.ggx_sample_grad call on the packed cotangent [n, 7] for the
    outputs the graph needs; u is held fixed"""
    @staticmethod
    def forward(ctx, wi, u, gpu, mat, material, ids, *values):
        wi, u = wi.contiguous(), u.contiguous()
        ctx.save_for_backward(wi, u)
        ctx.call = (gpu, mat, material, ids)
        ctx.values = values
        return tuple(gpu.sample(wi, u, mat=mat, material=material))

    @staticmethod
    def backward(ctx, g_wo, g_pdf, g_weight):
        wi, u = ctx.saved_tensors
        gpu, mat, material, ids = ctx.call
        n = wi.shape[0]
        in_values = [None] * len(ctx.values)
        needed = [i for i, need in enumerate(ctx.needs_input_grad[6:]) if need]
        want = tuple(name for name, need in zip(("wi", "params"), (ctx.needs_input_grad[0], bool(needed))) if need)
        grads = {}
        if want:
            g = torch.zeros((n, 7), dtype=torch.float32, device=wi.device)         # a None incoming gradient stays zero
            if g_wo is not None:
                g[:, 0:3] = g_wo
            if g_pdf is not None:
                g[:, 3] = g_pdf
            if g_weight is not None:
                g[:, 4:7] = g_weight
            out = gpu.ggx_sample_grad(wi, u, g, mat=mat, material=material, want=want)
            grads = dict(zip(want, (out,) if len(want) == 1 else out))
        if needed:
            sums = _per_material_sums(gpu, grads["params"], mat, ids, ctx.values)
            for i in needed:
                in_values[i] = sums[i]
        return (grads.get("wi"), None, None, None, None, None, *in_values)


def _ggx_values(ctx, mat, material, params):
    """(ids, tensors) of params= after the materials have received the tensors' current values (_Materials.refresh)"""
    if params is None:
        return (), ()
    m = _Materials(ctx, mat, material, None, params)
    m.refresh()
    return tuple(mid for _, mid, _ in m.entries), m.values


def ggx_pdf(ctx, wi, wo, mat=None, material: int = 0, params=None):
    """MerlHip.pdf(wi, wo, mat, material) of the context `ctx` — the same bits —, differentiable in wi and wo: what an MIS weight needs.
    The materials must be GGX conductors: the backward pass of a single material of another kind raises MRL_ERR_MATERIAL, and with mat=
    a unit whose id names no live GGX material receives a zero gradient.  Backward is one MerlHip.ggx_pdf_grad call
    (include/merl_hip_diff_sample.h) for the outputs the graph needs.
    params=: as in ggx_eval(): an f64 [7] tensor (alpha, eta rgb, k rgb) or {id: tensor}; forward does update_ggx on change.  Their
    gradient is the per-unit grad_alpha summed in f64 on the device (.double().sum(0), with ids index_add_ by id); the pdf depends on
    alpha alone, so only entry 0 is non-zero."""
    ids, values = _ggx_values(ctx, mat, material, params)
    return _GgxPdf.apply(wi, wo, ctx, mat, material, ids, *values)


def ggx_sample(ctx, wi, u, mat=None, material: int = 0, params=None):
    """MerlHip.sample(wi, u, mat, material) of the context `ctx` — (wo, pdf, weight), the same bits —, differentiable in wi: the sampled
    direction, its pdf and its weight move with the shading frame, so the next bounce's gradient flows through this one's sampler.  u
    is held fixed and the function is differentiated on the branch the forward call takes (include/merl_hip_diff_sample.h, DESIGN.md
    §5t); a rejected sample receives a zero gradient.  Backward is one MerlHip.ggx_sample_grad call on the packed cotangent for the
    outputs the graph needs.
    params=: as in ggx_pdf(); their gradient is the per-unit grad_params summed in f64 on the device."""
    ids, values = _ggx_values(ctx, mat, material, params)
    return _GgxSample.apply(wi, u, ctx, mat, material, ids, *values)


def ggx_eval(ctx, wi, wo, mat=None, material: int = 0, params=None):
    """MerlHip.eval(wi, wo, mat, material) of the context `ctx`, differentiable in wi and wo.  The materials must be GGX conductors:
    the backward pass of a single material of another kind raises MRL_ERR_MATERIAL, and with mat= a unit whose id names no live GGX
    material receives a zero gradient.
    params=: an f64 tensor [7] (alpha, eta rgb, k rgb) for the single material, or {id: tensor}: the call is differentiable in them
    too.  Forward writes a tensor's values into its material with MerlHip.update_ggx when the tensor has changed since — a 7-value
    read on the host, which waits for whatever computes the tensor; the material holds the values rounded to float, and the
    gradient is taken there.  Backward is MerlHip.ggx_grad / ggx_grad_mat (sum g . J) for the tensors that need it, at the parameters
    the material holds THEN: run it before the same material receives other values."""
    return _apply(ctx, wi, wo, partial(ctx.eval, mat=mat, material=material), partial(ctx.ggx_grad_dir, mat=mat, material=material),
                  mat, material, params=params)


def table_eval(ctx, wi, wo, mat=None, material: int = 0, tables=None):
    """MerlHip.eval(wi, wo, mat, material) of the context `ctx`, differentiable in wi and wo.  The materials must be RGB tables (MERL /
    customized_measurement): the backward pass of a single material of another kind raises MRL_ERR_MATERIAL, and with mat= a unit whose
    id names no live RGB table receives a zero gradient.  The gradient is the one of the trilinear interpolant in the cell eval
    selects (include/merl_hip_diff_table.h): piecewise smooth, like the function.
    tables=: an f64 device tensor [3, n_th, n_td, n_pd] (contiguous) for the single material, or {id: tensor} with mat=: the call is
    differentiable in the tables too.  Forward writes a tensor into its resident material with MerlHip.update_table(id, T.detach(),
    keep_sampling=True) — in place, from device memory — only when (T.data_ptr(), T._version) differs from what that material last
    received, then evaluates.  Backward returns MerlHip.table_grad of the incoming gradient (a dict: one table_grad_mat launch for all
    tables that need a gradient), beside the direction gradients; each call is issued only if the graph needs it.
    Under OPT_NEGATIVE = 0 the image is the clamped table, and the gradient returned is the adjoint's: the derivative of the clamped
    table where a texel is positive — where it is not, the true derivative is 0 (fit.py: A is linear only under OPT_NEGATIVE = 1)."""
    return _apply(ctx, wi, wo, partial(ctx.eval, mat=mat, material=material), partial(ctx.table_grad_dir, mat=mat, material=material),
                  mat, material, tables=tables)


def rgl_eval(ctx, wi, wo, mat=None, material: int = 0, values=None):
    """MerlHip.eval(wi, wo, mat, material) of the context `ctx`, differentiable in wi and wo.  The materials must be RGB RGL materials
    (upload_rgl / load_rgl): the backward pass of a single material of another kind raises MRL_ERR_MATERIAL, and with mat= a unit whose
    id names no live RGB RGL material receives a zero gradient.  The gradient is the exact one of the piecewise function in the cells
    eval selects (include/merl_hip_diff_rgl.h): piecewise smooth, like the function.
    values=: a device tensor [n_phi, n_theta, 3, ny, nx] (f32 or f64) for the single material, {id: tensor} with mat=, or a list with
    one tensor per live RGB RGL material of the context in the order of their ids: the call is differentiable in the files' measured
    values too (include/merl_hip_fit_rgl.h).  Forward writes a tensor into its resident material with
    MerlHip.update_rgl_values — in place, from device memory, rounded to float — only when (data_ptr, _version) differs from what that
    material last received; backward is one MerlHip.rgl_values_grad launch for all tensors that need a gradient, cast to each tensor's
    dtype.  vndf, ndf, sigma, luminance and the grids are not differentiable."""
    return _apply(ctx, wi, wo, partial(ctx.eval, mat=mat, material=material), partial(ctx.rgl_grad_dir, mat=mat, material=material),
                  mat, material, values=values)


def rgl_spectral_eval(ctx, wi, wo, wavelengths, mat=None, material: int = 0, values=None):
    """MerlHip.eval_spectral(wi, wo, wavelengths, material) — with mat=, eval_spectral_mat — of the context `ctx`: [n, W] values at the
    per-unit wavelengths [n, W] (float32 device tensor), differentiable in wi, wo AND the wavelengths.  The materials must be
    spectral RGL materials (upload_rgl of a file with "spectra"): the backward pass of a single material of another kind raises
    MRL_ERR_MATERIAL, and with mat= a unit whose id names no live spectral RGL material receives zero gradients.  Backward is one
    MerlHip.rgl_grad_dir_spectral call for what the graph needs (include/merl_hip_diff_rgl_spectral.h): the exact gradient of the
    piecewise function in the cells and the wavelength bracket eval selects; d value / d wavelength is piecewise constant, 0 outside
    the file's nodes and where the value is clamped.
    values=: a device tensor [n_phi, n_theta, n_wl, ny, nx] (f32 or f64) for the single material, or {id: tensor} with mat=: the call
    is differentiable in the files' spectra too (include/merl_hip_fit_rgl_spectral.h).  Forward writes a tensor into
    its resident material with MerlHip.update_rgl_spectral_values — in place, from device memory, rounded to float — only when
    (data_ptr, _version) differs from what that material last received; backward is one MerlHip.rgl_spectral_values_grad launch for
    all tensors that need a gradient, beside the direction and wavelength call, cast to each tensor's dtype.  vndf, ndf, sigma,
    luminance, the grids and the wavelength nodes are not differentiable."""
    if wavelengths is None:
        raise ValueError("rgl_spectral_eval: per-unit wavelengths [n, W] (the file's own nodes are no differentiable input)")
    if mat is None:
        forward = lambda a, b, wl: ctx.eval_spectral(a, b, wl, material)
    else:
        forward = lambda a, b, wl: ctx.eval_spectral_mat(a, b, wl, mat)
    backward = partial(ctx.rgl_grad_dir_spectral, mat=mat, material=material)
    if values is None:
        return _SpectralEval.apply(wi, wo, wavelengths, forward, backward)
    m = _SpectralValues(ctx, mat, material, values)
    m.refresh()
    return _SpectralEval.apply(wi, wo, wavelengths, forward, backward, m.gradients, *m.values)


def eval(ctx, wi, wo, mat=None, material: int = 0, tables=None, params=None, values=None):
    """MerlHip.eval(wi, wo, mat, material), differentiable in wi and wo, for GGX conductors, RGB tables, RGB RGL materials and batches
    that mix them.  Single material: the backward pass is the gradient call of that material's kind.  With mat=: the sum of
    table_grad_dir and ggx_grad_dir — and of rgl_grad_dir when the context holds a live RGB RGL material —, each exactly zero on the
    others' units; units of kinds this RGB-wide call does not serve (n-channel tables, spectral RGL materials — their values are
    [n, W]: rgl_spectral_eval() is their differentiable eval —, released or unknown ids) receive zeros.
    tables= / params= / values=: as in table_eval(), ggx_eval() and rgl_eval(), for the tables, the conductors and the RGL files of a
    mixed batch."""
    return _apply(ctx, wi, wo, partial(ctx.eval, mat=mat, material=material), partial(_any_backward, ctx, mat=mat, material=material),
                  mat, material, tables=tables, params=params, values=values)


def table_eval_nch(ctx, wi, wo, n_channels: int, mat=None, material: int = 0, tables=None):
    """MerlHip.eval_nch(wi, wo, n_channels, mat, material) of the context `ctx` — [n, n_channels] values —, differentiable in wi and wo.
    The materials must be n-channel tables of exactly n_channels channels: the backward pass of a single material of another kind or
    width raises MRL_ERR_MATERIAL, and with mat= a unit whose id names no such table receives a zero gradient.  One
    MerlHip.table_grad_dir_nch call for what the graph needs (include/merl_hip_diff_nch.h).
    tables=: as in table_eval(), with tensors [n_channels, n_th, n_td, n_pd]; backward is one MerlHip.table_grad_nch launch."""
    return _apply(ctx, wi, wo, partial(ctx.eval_nch, n_channels=n_channels, mat=mat, material=material),
                  partial(ctx.table_grad_dir_nch, n_channels=n_channels, mat=mat, material=material), mat, material, tables=tables,
                  n_channels=n_channels)
