"""The minimum-jerk start point on the CPU: the C-ABI's new symbols, the ABI version and the Python bindings (what
runs on the device is tests/test_gpu_minjerk.py's; the arithmetic is tests/test_minjerk_twin.py's)."""
import ctypes


def test_symbols_bindings_and_abi_version(gtop):
    lib = ctypes.CDLL(gtop.library_path())
    for name in ("gtop_min_jerk_start_device", "gtop_min_jerk_start"):
        assert hasattr(lib, name), name
    assert lib.gtop_abi_version() >= 8
    for name in ("min_jerk_start", "min_jerk_start_device"):
        assert hasattr(gtop.GtopContext, name), name
    L = gtop.load_library()
    assert L.gtop_min_jerk_start_device.argtypes is not None and len(L.gtop_min_jerk_start_device.argtypes) == 8
    assert L.gtop_min_jerk_start.argtypes is not None and len(L.gtop_min_jerk_start.argtypes) == 3


def test_null_context_is_refused_without_a_device(gtop):
    L = gtop.load_library()
    assert L.gtop_min_jerk_start_device(None, 1, 6, None, None, None, 6, None) == 1      # GTOP_ERR_INVALID
    assert L.gtop_min_jerk_start(None, 1, None) == 1
