"""The two reanalysis kernels in the compiler's own metadata, on the compile of bz_mcts.hip that
tests/test_kernel_resources.py reads (tests/kernel_meta.py: each source once per process): kernels of their own, one per game, with
no VGPR spills, no SGPR spills and no scratch -- the store kernel builds a slot's pi in shared memory, not in a private array --
and that shared memory is what 64 slots of NA floats take."""
import os

import pytest

import kernel_meta
from kernel_meta import compile_asm

needs_hipcc = pytest.mark.skipif(not os.path.exists(kernel_meta.HIPCC), reason="needs hipcc")
GAMES = {"ReversiTILi8": 65, "ReversiTILi6": 65, "ReversiTILi4": 65, "TicTacToe": 9}   # template argument -> NA


@needs_hipcc
@pytest.mark.parametrize("kernel", ["k_reanalyse_load", "k_reanalyse_store"])
@pytest.mark.parametrize("game", sorted(GAMES))
def test_no_spills_and_no_scratch_in_any_instantiation(kernel, game):
    asm = compile_asm("bz_mcts.hip")
    assert len(kernel_meta.matches(asm.kernels, kernel)) == len(GAMES), kernel_meta.matches(asm.kernels, kernel)
    k = asm.kernels[asm.find(kernel, game)]
    assert (k["vspill"], k["sspill"], k["scratch"]) == (0, 0, 0), (kernel, game, k)
    if kernel == "k_reanalyse_store":
        assert k["max_wg"] == 64 and k["lds_static"] == 64 * GAMES[game] * 4 + 64 * 8, (game, k)
    else:
        assert k["lds_static"] == 0, (game, k)
