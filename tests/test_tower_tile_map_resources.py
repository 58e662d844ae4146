"""k_edge_bf16<Tw<128, 4, true, 1>> -- the 128-channel throughput tower on the edge-aware cell tiling (DESIGN.md 5,
csrc/bz_tile_map.h) -- read from the compiler's metadata and assembly, as tests/test_kernel_resources.py does: it is one
kernel under a name of its own, it neither spills nor uses scratch, it fits the 512 registers of one workgroup per CU,
and it really skips the column tiles: per layer body 126 tile-taps x 4 k-steps x 2 channel halves = 1008
v_mfma_f32_16x16x32_bf16 (board-row tiles: 1056), plus 32 for the stem; the heads stay on 16 v_mfma_f32_32x32x16_bf16."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_edge_kernel_resources_and_mfma_count(tmp_path):
    out = tmp_path / "bz_net.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S",
                           "-o", str(out), os.path.join(ROOT, "betazero_amd", "csrc", "bz_net.hip")], stderr=subprocess.DEVNULL)
    asm = out.read_text()
    res = {}
    for blk in re.split(r"\n  - \.agpr_count:", asm)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        g = lambda k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1))  # noqa: E731
        res[name] = {"vgpr": g("vgpr_count"), "vspill": g("vgpr_spill_count"), "sspill": g("sgpr_spill_count"),
                     "scratch": g("private_segment_fixed_size"), "lds_static": g("group_segment_fixed_size"),
                     "max_wg": g("max_flat_workgroup_size")}
    hits = [k for k in res if "k_edge_bf16" in k]
    assert len(hits) == 1 and "Li128ELi4ELb1ELi1E" in hits[0], hits   # one instantiation: Tw<128, 4, true, 1>
    assert "k_tower_bf16" not in hits[0] and "k_sym_bf16" not in hits[0]
    k = res[hits[0]]
    print(hits[0], k)
    assert k["vspill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0, k
    assert k["vgpr"] <= 512 and k["max_wg"] == 256, k                  # 4 waves, one per SIMD: one workgroup per CU

    m = next(m for m in re.finditer(r"^(\S+):\s*; @\1$", asm, re.M) if m.group(1) == hits[0])
    body = asm[m.end():asm.index("s_endpgm", m.end())]
    count = lambda mn: len(re.findall(rf"^\s+{mn}\b", body, re.M))    # noqa: E731
    assert count("v_mfma_f32_16x16x32_bf16") == 2 * 1008 + 32
    assert count("v_mfma_f32_32x32x16_bf16") == 16
    assert "scratch_" not in body
