#!/usr/bin/env python3
"""What a spectral RGL material costs over a wavefront queue and with material ids (mrl_eval_sample_spectral_queue / _batch_mat)
next to the whole-array call: 16M slots, a file of the database's isotropic shape (8 theta_i nodes, 32 x 32 warps) with 32 wavelength
nodes, four wavelengths per slot — the spectral_isotropic_8x32x32_32wl row of profiles/r04_rgl_rates.json.  Device events around 5
calls after 2 warm-up calls.   python tools/rgl_spectral_queue_rates.py > profiles/r05_rgl_spectral_queue_rates.json"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from mitsuba_customization_amd import host, synth

n, W = 16 << 20, 4
shape = dict(n_phi=1, n_theta=8, res=32, res_ndf=128, res_sigma=64, n_wavelengths=32)
res = {"units": n, "wavelengths_per_unit": W, "file": "isotropic 8x32x32, 32 wavelength nodes", "library": host.build_info()}


def rate(g, call):
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    g.timer_start()
    for _ in range(5):
        call()
    ms = g.timer_stop() / 5
    return {"ms": round(ms, 3), "G_units_per_s": round(n / ms / 1e6, 3)}


with host.MerlHip(0) as g:
    g.use_torch_stream()
    wi, wo, u = g.generate_pairs(0x5EED, 0, n)
    wl = torch.rand(n, W, device="cuda") * 640.0 + 360.0
    m1 = g.upload_rgl(synth.make_rgl_fields(seed=9, **shape))
    m2 = g.upload_rgl(synth.make_rgl_fields(seed=10, **shape))
    out = (torch.zeros(n, W, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, 3, device="cuda"), torch.zeros(n, device="cuda"),
           torch.zeros(n, W, device="cuda"))
    full = torch.tensor([n], dtype=torch.int32, device="cuda")
    dense = torch.arange(n, dtype=torch.int32, device="cuda")
    half = torch.sort(torch.randperm(n, device="cuda")[: n // 2])[0].to(torch.int32)
    half_count = torch.tensor([n // 2], dtype=torch.int32, device="cuda")
    shuffled = torch.randperm(n, device="cuda").to(torch.int32)
    res["whole_array"] = rate(g, lambda: g.eval_sample_spectral(wi, wo, u, wl, m1))
    res["queue_density_1_ascending"] = rate(g, lambda: g.eval_sample_spectral_queue(wi, wo, u, wl, dense, full, material=m1, out=out))
    res["queue_density_0.5_ascending"] = rate(g, lambda: g.eval_sample_spectral_queue(wi, wo, u, wl, half, half_count, material=m1, out=out))
    res["queue_density_1_shuffled"] = rate(g, lambda: g.eval_sample_spectral_queue(wi, wo, u, wl, shuffled, full, material=m1, out=out))
    ids = torch.tensor([m1, m2], dtype=torch.int32, device="cuda")
    mat = ids[torch.arange(n, device="cuda") % 2].contiguous()
    res["multi_id_two_materials_alternating_queue"] = rate(g, lambda: g.eval_sample_spectral_queue(wi, wo, u, wl, dense, full, mat=mat, out=out))
    res["multi_id_two_materials_alternating_batch_mat"] = rate(g, lambda: g.eval_sample_spectral_mat(wi, wo, u, wl, mat))
    at = g.partition_by_material(mat)[1].cpu().tolist()

    def partitioned():
        pq, _, counts = g.partition_by_material(mat)
        for m in (m1, m2):
            g.eval_sample_spectral_queue(wi, wo, u, wl, pq[at[m]:], counts[m:m + 1], material=m, capacity=n - at[m], out=out)
    res["partition_then_single_id_queues"] = rate(g, partitioned)
    res["queue_dense_over_whole_array"] = round(res["queue_density_1_ascending"]["ms"] / res["whole_array"]["ms"], 3)
    res["multi_id_over_partitioned"] = round(res["multi_id_two_materials_alternating_queue"]["ms"] / res["partition_then_single_id_queues"]["ms"], 3)
print(json.dumps(res, indent=1))
