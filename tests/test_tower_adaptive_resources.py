"""The adaptive tower shape gates the EXISTING kernels on the device-side count -- no new kernel, no new
instantiation -- so the budget to hold is theirs: the gate and the tally sit before the first barrier of every bf16 tower
kernel and must cost the hot path nothing.  Read from the compiler's metadata, as tests/test_kernel_resources.py does:
no kernel of the family spills or uses scratch, and the benchmark net's throughput shape keeps the register counts it had
before the gate existed (354 VGPRs of which 190 AGPRs; symmetric form 380 / 216)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_gated_tower_kernels_keep_their_registers(tmp_path):
    out = tmp_path / "bz_net.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S",
                           "-o", str(out), os.path.join(ROOT, "betazero_amd", "csrc", "bz_net.hip")], stderr=subprocess.DEVNULL)
    res = {}
    for blk in re.split(r"\n  - \.agpr_count:", out.read_text())[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        g = lambda k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1))  # noqa: E731
        res[name] = {"agpr": int(re.match(r"\s*(\d+)", blk).group(1)), "vgpr": g("vgpr_count"), "vspill": g("vgpr_spill_count"),
                     "sspill": g("sgpr_spill_count"), "scratch": g("private_segment_fixed_size")}
    family = {k: v for k, v in res.items() if "k_tower_bf16" in k or "k_sym_bf16" in k}
    assert len(family) == 12, sorted(family)   # six geometries x (plain, symmetric): the gate added none
    for k, v in family.items():
        assert v["vspill"] == 0 and v["sspill"] == 0 and v["scratch"] == 0 and v["vgpr"] <= 512, (k, v)

    def one(*parts):
        hits = [k for k in family if all(p in k for p in parts)]
        assert len(hits) == 1, (parts, hits)
        return family[hits[0]]
    for kernel, geom, vgpr, agpr in (("k_tower_bf16", "Li128ELi4ELb1E", 354, 190), ("k_sym_bf16", "Li128ELi4ELb1E", 380, 216),
                                     ("k_tower_bf16", "Li128ELi1ELb0E", 176, 32), ("k_sym_bf16", "Li128ELi1ELb0E", 176, 32)):
        k = one(kernel, geom)
        print(kernel, geom, k)
        assert k["vgpr"] <= vgpr and k["agpr"] <= agpr, (kernel, geom, k)
