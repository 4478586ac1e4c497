"""CPU-side checks of the lane_framed pair (ptls_mi355x_keyset_set_lane_framed / _get_lane_framed): declared by the
header, exported by the built library, listed in the Python layer with their ctypes signatures, and wrapped by Keyset.

No device call (test_abi.py's way of loading the library without a GPU)."""
import ctypes
import inspect

import picotls_amd as pa
from test_abi import declared, exported

PAIR = {"ptls_mi355x_keyset_set_lane_framed", "ptls_mi355x_keyset_get_lane_framed"}


def test_the_header_declares_and_the_library_exports_the_pair():
    assert PAIR <= declared("mi355x.h")
    pa.load_library()
    assert PAIR <= exported(pa.LIB_PATH)


def test_the_python_layer_lists_and_types_the_pair():
    assert PAIR <= set(pa.ABI_FUNCTIONS)
    lib = pa.load_library()
    assert lib.ptls_mi355x_keyset_set_lane_framed.argtypes == [ctypes.c_void_p, ctypes.c_int]
    assert lib.ptls_mi355x_keyset_get_lane_framed.argtypes == [ctypes.c_void_p]
    assert lib.ptls_mi355x_keyset_get_lane_framed.restype is ctypes.c_int


def test_keyset_wraps_the_pair():
    assert hasattr(pa.Keyset, "set_lane_framed") and hasattr(pa.Keyset, "lane_framed")
    params = list(inspect.signature(pa.Keyset.set_lane_framed).parameters)
    assert params == ["self", "on"]
    prop = inspect.getattr_static(pa.Keyset, "lane_framed")
    assert isinstance(prop, property) and prop.fset is None, "lane_framed is a read-only property"
    # what this pull request must not change
    assert pa.Keyset.SCHEDULES == {"auto": 0, "lockstep": 1, "chunked": 2, "record_per_lane": 3}
    assert list(inspect.signature(pa.Keyset.set_schedule).parameters) == ["self", "schedule", "allow_variable_time"]
