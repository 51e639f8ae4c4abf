"""Device-resident array I/O (mg_*_device, include/mg_hip.h) -- what can be checked without a GPU: capi.device_view's
reading of __cuda_array_interface__ and the NULL-handle refusal of the six entry points."""
import ctypes as C

import pytest

from multigrid_prj_amd import capi


class FakeDeviceArray:
    """anything that follows the protocol: device_view must not ask for more than the interface"""

    def __init__(self, shape=(3, 5, 5), typestr="<f8", ptr=0x7F0000001008, readonly=False, strides=None):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, readonly), "strides": strides, "version": 2}


def test_device_view_reads_pointer_and_dtype():
    assert capi.device_view(FakeDeviceArray(), (3, 5, 5)) == (0x7F0000001008, capi.MG_F64)
    assert capi.device_view(FakeDeviceArray(typestr="<f4", ptr=0x1004), (3, 5, 5), writable=True) == (0x1004, capi.MG_F32)
    # explicit C-contiguous strides (bytes) are what a non-None `strides` has to say
    assert capi.device_view(FakeDeviceArray(strides=(200, 40, 8)), (3, 5, 5)) == (0x7F0000001008, capi.MG_F64)
    assert capi.device_view(FakeDeviceArray(shape=(9, 9), typestr="<f4", strides=(36, 4)), (9, 9))[1] == capi.MG_F32
    # a read-only array is good enough as a source
    assert capi.device_view(FakeDeviceArray(readonly=True), (3, 5, 5))[0] == 0x7F0000001008
    assert capi.device_view(FakeDeviceArray(shape=[3, 5, 5]), (3, 5, 5))[1] == capi.MG_F64


@pytest.mark.parametrize("obj,writable,what", [
    (object(), False, "no __cuda_array_interface__"),
    ([1.0, 2.0], False, "no __cuda_array_interface__"),
    (FakeDeviceArray(typestr="<f2"), False, "typestr"),
    (FakeDeviceArray(typestr="<i8"), False, "typestr"),
    (FakeDeviceArray(typestr=">f8"), False, "typestr"),
    (FakeDeviceArray(shape=(3, 5, 4)), False, "shape"),
    (FakeDeviceArray(shape=(75,)), False, "shape"),
    (FakeDeviceArray(strides=(40, 200, 8)), False, "strides"),
    (FakeDeviceArray(strides=(400, 80, 16)), False, "strides"),
    (FakeDeviceArray(typestr="<f4", strides=(200, 40, 8)), False, "strides"),
    (FakeDeviceArray(ptr=0), False, "null"),
    (FakeDeviceArray(ptr=None), False, "null"),
    (FakeDeviceArray(readonly=True), True, "read-only"),
], ids=["no-interface", "list", "f16", "int64", "big-endian", "shape", "flat", "transposed", "strided", "f8-strides-on-f4", "null", "none",
        "read-only"])
def test_device_view_refuses_malformed(obj, writable, what):
    with pytest.raises(ValueError, match=what):
        capi.device_view(obj, (3, 5, 5), writable=writable)


def test_null_handle_is_bad_arg():
    lib = capi.load()
    buf = C.c_void_p(0x1000)   # never looked at: the handle is refused first
    calls = [
        lambda: lib.mg_set_array_device(None, capi.ARR_U, 0, buf, capi.MG_F64, None),
        lambda: lib.mg_get_array_device(None, capi.ARR_U, 0, buf, capi.MG_F64, None),
        lambda: lib.mg_heat_set_source_device(None, buf, capi.MG_F64, None),
        lambda: lib.mg_mixed_set_rhs_device(None, buf, capi.MG_F64, None),
        lambda: lib.mg_mixed_set_solution_device(None, buf, capi.MG_F64, None),
        lambda: lib.mg_mixed_get_solution_device(None, buf, capi.MG_F64, None),
    ]
    for call in calls:
        assert call() == -4
        assert b"null handle" in lib.mg_last_error()
