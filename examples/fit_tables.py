"""Several tables from one capture session: draws (wi, wo, material, rgb) samples of three synthetic tables of different dims
and parameterisations — interleaved, a table index per sample, as a wavefront renderer's hit queue holds them — and fits all three
at once with fit.fit_tables: per CGLS iteration one eval with material ids and one MerlHip.table_grad_mat launch, whatever the
number of tables.  Prints every table's residuals and its distance from the truth on the cells the samples reach.

    python examples/fit_tables.py [--log2n 20] [--iters 20]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mitsuba_customization_amd import fit, host, synth  # noqa: E402

TABLES = (((24, 24, 48), 0), ((16, 16, 24), 1), ((12, 20, 32), 2))        # (dims, parameterisation: half/diff, standard, standard-full)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    n = 1 << args.log2n
    dims_list, params = [d for d, _ in TABLES], [p for _, p in TABLES]
    truths = [synth.make_table("ggx_tab", k, dims) for k, dims in enumerate(dims_list)]
    with host.MerlHip(0) as gpu:
        gpu.set_option(host.OPT_NEGATIVE, 1)                  # keep: eval stays linear in the iterates (fit.py)
        wi, wo, _ = gpu.generate_pairs(0x5EED, 0, n)
        mat = torch.randint(0, len(TABLES), (n,), device=wi.device, dtype=torch.int32)
        ids = [gpu.upload_table_param(t, p) for t, p in zip(truths, params)]
        rgb = gpu.eval(wi, wo, mat=fit._unit_ids(mat, ids))   # the "measurement": every sample through its own table
        for mid in ids:
            gpu.release_material(mid)
        tables, residuals = fit.fit_tables(gpu, dims_list, wi, wo, mat, rgb, args.iters, params=params)
        _, masks = fit.splat_mat(gpu, dims_list, wi, wo, mat, rgb, params=params)
    for k, (dims, res) in enumerate(zip(dims_list, residuals)):
        truth, reached = torch.from_numpy(truths[k]).to(tables[k].device), masks[k]
        err = float(((tables[k] - truth)[reached] ** 2).sum() / (truth[reached] ** 2).sum()) ** 0.5
        print(f"table {k} dims {dims} param {params[k]}: |A T - y| {res[0]:.4e} -> {res[-1]:.4e} in {args.iters} iterations, "
              f"relative distance from the truth on {int(reached.sum())} reached texels {err:.3e}")


if __name__ == "__main__":
    main()
