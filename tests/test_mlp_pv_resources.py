"""The tic-tac-toe MLP kernels (csrc/bz_mlp.hip) in the compiler's own metadata, on one compile of the source
(tests/kernel_meta.py: each source once per process).  The bf16 forward holds a whole layer's activations in registers: the
value lane of its last tile must cost it no VGPR spill and no scratch at any of the 16 hidden sizes -- H = 512 sits
just above 430 VGPRs.  The f32 forward and the training kernels, supervised and PV, keep their rows' private arrays in registers
too: no scratch."""
import os

import pytest

import kernel_meta
from kernel_meta import compile_asm

needs_hipcc = pytest.mark.skipif(not os.path.exists(kernel_meta.HIPCC), reason="needs hipcc")
HS = list(range(32, 513, 32))


@needs_hipcc
@pytest.mark.parametrize("H", HS)
def test_bf16_forward_has_no_vgpr_spill_and_no_scratch(H):
    asm = compile_asm("bz_mlp.hip")
    assert len(kernel_meta.matches(asm.kernels, "k_mlp_bf16")) == len(HS), kernel_meta.matches(asm.kernels, "k_mlp_bf16")
    k = asm.kernels[asm.find("k_mlp_bf16", f"Li{H}E")]
    assert (k["vspill"], k["scratch"]) == (0, 0), (H, k)
    assert k["vgpr"] <= 512 and k["lds_static"] == 0 and k["max_wg"] == 64, (H, k)


@needs_hipcc
@pytest.mark.parametrize("kernel", ["k_mlp_f32", "k_mlp_train_fb", "k_mlp_train_fb_pv", "k_mlp_train_adam", "k_mlp_pack_bf16"])
def test_f32_and_training_kernels_have_no_scratch(kernel):
    asm = compile_asm("bz_mlp.hip")
    k = asm.kernels[asm.find(kernel)]
    assert (k["vspill"], k["sspill"], k["scratch"]) == (0, 0, 0), (kernel, k)
