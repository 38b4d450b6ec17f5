"""CPU suite: the built library exports the LQR score's adjoint (no compute call: no GPU here)."""
import ctypes

from conftest import PKG


def test_library_exports_the_lqr_score_vjp():
    assert hasattr(ctypes.CDLL(str(PKG / "ttmpc" / "libttmpc.so")), "tt_lqr_score_vjp_device")
