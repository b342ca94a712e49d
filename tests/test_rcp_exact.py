"""The triangle test's reciprocal (traversal.hip.h rcpExact): v_rcp_f32 and one Newton step where that is bit for bit the
correctly rounded 1.0f / d, the IEEE division for a wavefront with any other input.  crt_debug_check_rcp compares it with the
device's division for every one of the 2^32 single-precision inputs and counts, by class, where the unguarded Newton form
differs -- the evidence for the guard."""
import ctypes as C

import numpy as np
import pytest


def test_check_entry_point_is_exported(pkg):
    L = pkg.lib()
    assert "crt_debug_check_rcp" in pkg.ABI_SYMBOLS and hasattr(L, "crt_debug_check_rcp")
    assert L.crt_debug_check_rcp(0, None) == 1  # CRT_EINVAL


@pytest.mark.gpu
def test_rcp_exact_equals_division_for_every_input(pkg):
    out = np.zeros(8, dtype=np.uint64)
    assert pkg.lib().crt_debug_check_rcp(0, out.ctypes.data_as(C.c_void_p)) == 0
    bad, checked, exp0, exp_high, all_ones, rest, first = (int(v) for v in out[:7])
    print("rcpExact mismatches %d of %d inputs; unguarded Newton form: exponent 0 %d, exponent 253..255 %d, all-ones "
          "significand %d, accepted by the guard %d" % (bad, checked, exp0, exp_high, all_ones, rest))
    assert checked == 1 << 32
    assert bad == 0, "first mismatch at input 0x%08x" % first
    # the guard is needed (the Newton form alone is not the division on the excluded classes) ...
    assert exp0 > 0 and exp_high > 0
    # ... and sufficient: on every input it accepts (biased exponent 1..252, all-ones significands included), the Newton
    # form is the division
    assert all_ones == 0 and rest == 0
