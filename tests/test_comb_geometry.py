"""dkg_comb_geometry (a host function: no GPU, no ctx): the geometry of the two comb kinds -- 0 the
shared bases' radix-2^DKG_COMBW_BITS comb, 1 the member keys' radix-2^DKG_KEY_COMB_BITS comb -- and the
chunk the chained builder walks per thread."""
import ctypes

import pytest

import dkg_amd
from dkg_amd import _lib
from tests import edge_vectors as EV


@pytest.mark.parametrize("kind", [0, 1])
def test_geometry_agrees_with_the_window_counts(kind):
    L = dkg_amd.lib()
    g = dkg_amd.comb_geometry(kind)
    windows = L.dkg_fixed_base_windows() if kind == 0 else L.dkg_key_comb_windows()
    assert g["windows"] == windows == 256 // g["bits"] + 1
    assert g["bits"] == EV.comb_radix(windows)
    assert g["entries"] == 1 << (g["bits"] - 1)
    # the top window absorbs the signed recoding's carry
    assert g["windows"] * g["bits"] > 256


@pytest.mark.parametrize("kind", [0, 1])
def test_chunk_divides_the_window(kind):
    g = dkg_amd.comb_geometry(kind)
    assert g["chunk"] >= 2
    assert g["entries"] % g["chunk"] == 0


@pytest.mark.parametrize("kind", [-1, 2, 3, 1 << 20])
def test_bad_kinds_are_rejected(kind):
    with pytest.raises(dkg_amd.DkgError) as e:
        dkg_amd.comb_geometry(kind)
    assert e.value.code == _lib.DKG_E_ARG


def test_outputs_may_be_null_and_the_function_is_pure():
    L = dkg_amd.lib()
    for kind in (0, 1):
        assert L.dkg_comb_geometry(kind, None, None, None, None) == _lib.DKG_OK
        want = dkg_amd.comb_geometry(kind)
        bits, chunk = ctypes.c_int(), ctypes.c_uint32()
        assert L.dkg_comb_geometry(kind, ctypes.byref(bits), None, None, None) == _lib.DKG_OK
        assert L.dkg_comb_geometry(kind, None, None, None, ctypes.byref(chunk)) == _lib.DKG_OK
        assert (bits.value, chunk.value) == (want["bits"], want["chunk"])
        assert dkg_amd.comb_geometry(kind) == want
    # a rejected kind leaves the outputs alone
    bits = ctypes.c_int(-7)
    assert L.dkg_comb_geometry(9, ctypes.byref(bits), None, None, None) == _lib.DKG_E_ARG
    assert bits.value == -7
