"""Layer-1 lattice forward, last row tile: wavefronts without a live replay row skip the matrix work -- on the hipemu (CPU) build of
the kernel sources, both wavefront forms and both operand forms.  Same checks on the GPU: test_forward_edge_gpu.py."""
import pytest

import forward_edge_checks as FC
from test_kernels_emu import EmuBackend


@pytest.fixture(scope="module")
def bk():
    return EmuBackend()


@pytest.mark.parametrize("w8", ["0", "1"])
@pytest.mark.parametrize("mode", [3, 0])
@pytest.mark.parametrize("B", FC.EDGES)
def test_rows_below_B_equal_the_full_tile_and_rows_beyond_keep_their_sentinel(bk, B, mode, w8, monkeypatch, lattice_form):
    lattice_form(bk, mode)
    monkeypatch.setenv("RCMARL_LAT_W8", w8)
    FC.check_forward_edge(bk, B)
