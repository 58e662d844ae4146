"""Register / spill budget of the symmetric net kernels, read from the compiler's own metadata (hipcc -S
cross-compiles for gfx950 without a GPU), and the proof that the plain kernels did not move: the symmetric forms are
compiled from the same text, and each plain tower keeps the register count it had before they existed."""
import os

import pytest

from test_kernel_resources import HIPCC, _count, _find, _resources

GEOMETRIES = ("Li128ELi4ELb1E", "Li64ELi8E", "Li256ELi2E", "Li128ELi1E", "Li64ELi2E", "Li256ELi1E")
# VGPRs of the plain towers at the parent commit (the one before the symmetric kernels were added), read from its build
PARENT_VGPR = {"Li128ELi4ELb1E": 354, "Li64ELi8E": 320, "Li256ELi2E": 388, "Li128ELi1E": 176, "Li64ELi2E": 148, "Li256ELi1E": 324}
PARENT_VGPR_FP8 = 256

_RES = {}


def _net_resources(tmp_path):
    if not _RES:  # one compile for the whole module
        _RES["res"] = _resources("bz_net.hip", tmp_path)
        _RES["asm"] = _resources.asm
    return _RES["res"], _RES["asm"]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_symmetric_kernels_keep_the_plain_kernels_occupancy(tmp_path):
    """no scratch, no spills; one workgroup per CU for bf16 (<= 512 VGPRs), two for fp8 (<= 256)"""
    res, _ = _net_resources(tmp_path)
    for geo in GEOMETRIES:
        k = _find(res, "k_sym_bf16", geo)
        assert k["vgpr"] <= 512 and k["vspill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0, (geo, k)
    k = _find(res, "k_sym_fp8")
    assert k["vgpr"] <= 256 and k["vspill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0, k
    for name in ("k_sym_mean", "k_sym_stem", "k_sym_heads"):
        k = _find(res, name)
        assert k["vspill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0, (name, k)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_plain_kernels_did_not_move(tmp_path):
    res, asm = _net_resources(tmp_path)
    for geo in GEOMETRIES:  # the lookups of test_kernel_resources.py still find exactly one kernel each
        assert _find(res, "k_tower_bf16", geo)["vgpr"] == PARENT_VGPR[geo], geo
    assert _find(res, "k_tower_fp8")["vgpr"] == PARENT_VGPR_FP8
    # the symmetric towers do the same matrix work as their plain counterparts
    for mn in ("v_mfma_f32_16x16x32_bf16", "v_mfma_f32_32x32x16_bf16"):
        assert _count(asm, ("k_sym_bf16", "Li128ELi4ELb1E"), mn) == _count(asm, ("k_tower_bf16", "Li128ELi4ELb1E"), mn)
    assert _count(asm, ("k_sym_bf16", "Li64ELi8ELb0E"), "v_mfma_f32_32x32x16_bf16") == \
        _count(asm, ("k_tower_bf16", "Li64ELi8ELb0E"), "v_mfma_f32_32x32x16_bf16")
    mn = "v_mfma_scale_f32_32x32x64_f8f6f4"
    assert _count(asm, ("k_sym_fp8",), mn) == _count(asm, ("k_tower_fp8",), mn)
