"""tests/helpers.assert_bits_equal_nan, the comparison of the non-finite pins (tests/test_ref_shaders_nonfinite.py, tests/test_gpu_nonfinite.py):
NaN == NaN whatever the sign and payload, every other value bit for bit.  No GPU."""
import numpy as np
import pytest

import helpers


def _h(*v):
    return np.array(v, np.float32).astype(np.float16).view(np.uint16)


def _f(*v):
    return np.array(v, np.float32).view(np.uint32)


@pytest.mark.parametrize("pack", [_h, _f])
def test_equal_nan_any_payload(pack):
    a = pack(1.0, np.nan, -0.0, np.inf, 65504.0)
    b = a.copy()
    b[1] = b[1] | (0x8001 if a.dtype == np.uint16 else 0x80000001)     # a NaN of the other sign and another payload
    helpers.assert_bits_equal_nan(a, b, "NaN payloads")


@pytest.mark.parametrize("pack", [_h, _f])
@pytest.mark.parametrize("got,ref", [(np.nan, np.inf), (0.0, -0.0), (65504.0, np.inf), (-np.inf, np.inf), (np.nan, 1.0)])
def test_rejects(pack, got, ref):
    with pytest.raises(AssertionError, match="1 of 3 values differ"):
        helpers.assert_bits_equal_nan(pack(2.0, got, 3.0), pack(2.0, ref, 3.0), "edge")


@pytest.mark.parametrize("pack", [_h, _f])
def test_rejects_one_ulp(pack):
    a = pack(0.75, 1.0, 1.0e4)
    b = a.copy()
    b[2] += 1
    with pytest.raises(AssertionError, match="1 of 3 values differ"):
        helpers.assert_bits_equal_nan(b, a, "1 ulp")


def test_rejects_dtype_and_shape_mismatch():
    with pytest.raises(AssertionError):
        helpers.assert_bits_equal_nan(_h(1.0), _f(1.0), "dtype")
    with pytest.raises(AssertionError):
        helpers.assert_bits_equal_nan(_h(1.0, 2.0), _h(1.0), "shape")
