"""The spectral queue / material-id kernels (k_rgl_spectral_q, merl_rgl.hip) on the compiled code (hipcc cross-compiles without a GPU):
every instance launch_rgl_spectral_q can launch exists, the isotropic-shape kernels keep every value in registers, and no other new
kernel has more scratch than the whole-array kernel of its mode and run-time shape (k_rgl_spectral<MODE, false, 0>).  The memory
round trips of the new kernels are printed as a report, not checked: nobody has measured what the W loop does to them."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

MODES = (0, 2, 3, 4)                 # eval, sample, eval + sample, eval + pdf (the pdf alone is the RGB pdf call's)


def _resources(asm):
    """{demangled kernel name: scratch bytes per lane}"""
    blocks = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm, re.S)
    names = subprocess.run(["c++filt"] + [b[0] for b in blocks], capture_output=True, text=True).stdout.splitlines()
    out = {}
    for (_, body), d in zip(blocks, names):
        d = d.replace("mrl::(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        out[d] = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
    return out


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc missing")
def test_spectral_queue_kernels_exist_and_keep_scratch_bounded():
    import isa_round_trips as irt
    asm = irt.compile_to_asm(os.path.join(ROOT, "mitsuba_customization_amd", "csrc", "merl_rgl.hip"))
    scratch = _resources(asm)
    trips = irt.round_trips(asm)
    single = [f"k_rgl_spectral_q<{m}, true, false, {lds}, {mask}>" for m in MODES for lds in ("true", "false") for mask in (5, 0)]
    multi = [f"k_rgl_spectral_q<{m}, {ix}, true, false, 0>" for m in MODES for ix in ("true", "false")]
    assert len(single) == 16 and len(multi) == 8
    for name in single + multi:
        assert name in scratch, (name, sorted(k for k in scratch if "spectral" in k))
    for name in single + multi:
        mode = int(name.split("<")[1].split(",")[0])
        if name.endswith(", 5>"):
            assert scratch[name] == 0, (name, scratch[name])
        else:
            bound = scratch[f"k_rgl_spectral<{mode}, false, 0>"]
            assert scratch[name] <= bound, (name, scratch[name], bound)
    new = sorted(k for k in scratch if k.startswith("k_rgl_spectral_q<"))
    assert len(new) == 24, new                      # nothing else is instantiated (no pdf-alone kernel)
    for name in new:
        print(f"{name:45s} scratch {scratch[name]:3d} B  loads {trips[name]['loads']:4d}  round_trips {trips[name]['round_trips']:4d}")
