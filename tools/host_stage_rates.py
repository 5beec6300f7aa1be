#!/usr/bin/env python3
"""The host-array figures behind profiles/host_stage_rates.json, one JSON line per run.  MRL_LIB_PATH selects the build, so that two
builds can be run alternately on one machine:  MRL_LIB_PATH=<libmerl_hip.so> python tools/host_stage_rates.py

  threads_0 / threads_4   eval_sample on pageable numpy arrays, 16 Mi units, as tools/extra_rates.py measures it (one warm-up call,
                          best of 3), through the staged and the pipelined mover
  spectral                one eval_sample_spectral host call of 2^20 units at 4 wavelengths per unit: the first call of the context
                          (it allocates) and the best of 3 after it"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from mitsuba_customization_amd import host, synth


def best_of(fn, reps=3):
    best = 1e9
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best


res = {"build": host.build_info()}
with host.MerlHip(0) as gpu:
    mid = gpu.upload_merl(synth.make_table("ggx_tab", 0))
    m = 16 << 20
    wi, wo, u = (t.cpu().numpy() for t in gpu.generate_pairs(0x5EED, 0, m))
    out = tuple(np.empty(s, np.float32) for s in ((m, 3), (m,), (m, 3), (m,), (m, 3)))
    for threads in (0, 4):
        gpu.set_option(host.OPT_HOST_THREADS, threads)
        gpu.eval_sample(wi, wo, u, material=mid, out=out)
        s = best_of(lambda: gpu.eval_sample(wi, wo, u, material=mid, out=out))
        res[f"threads_{threads}"] = {"units": m, "s": s, "Munits_per_s": m / s / 1e6}
    fields = synth.make_rgl_fields(seed=3, n_phi=1, n_theta=8, res=32, n_wavelengths=32)
    spec = gpu.upload_rgl(fields)
    n, W = 1 << 20, 4
    nodes = np.asarray(fields["wavelengths"], np.float32)
    wl = np.random.default_rng(1).uniform(nodes[0], nodes[-1], (n, W)).astype(np.float32)
    call = lambda: gpu.eval_sample_spectral(wi[:n], wo[:n], u[:n], wl, spec)
    t0 = time.perf_counter()
    call()
    first = time.perf_counter() - t0
    s = best_of(call)
    res["spectral"] = {"units": n, "wavelengths_per_unit": W, "first_call_s": first, "s": s, "Munits_per_s": n / s / 1e6}
print(json.dumps(res))
