"""CPU-side checks of the signed field's boundary (include/gtop.h, gtop_set_field_sign): the three entry points are
declared, exported and bound, the ABI version says so, and they refuse a missing object without a device."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gtop_set_field_sign", "gtop_get_field_sign", "gtop_group_set_field_sign")


def test_header_declares_the_field_sign_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gtop.h")).read(), flags=re.S)
    assert re.search(r"int gtop_set_field_sign\(gtop_ctx \*ctx, int signed_mode, double max_depth\);", src)
    assert re.search(r"int gtop_get_field_sign\(const gtop_ctx \*ctx, int \*signed_mode, double \*max_depth\);", src)
    assert re.search(r"int gtop_group_set_field_sign\(gtop_group \*g, int signed_mode, double max_depth\);", src)


def test_library_exports_and_binds_the_field_sign_entry_points(gtop):
    raw = ctypes.CDLL(gtop.library_path())
    for name in NAMES:
        assert hasattr(raw, name), name
    lib = gtop.load_library()
    for name in NAMES:
        assert getattr(lib, name).argtypes is not None, name
    assert lib.gtop_abi_version() >= 3
    assert hasattr(gtop.GtopContext, "set_field_sign") and hasattr(gtop.GtopContext, "field_sign")
    assert hasattr(gtop.GtopGroup, "set_field_sign")


def test_field_sign_entry_points_refuse_a_null_object(gtop):
    """No context can exist without a device; what can be reached is the NULL check (GTOP_ERR_INVALID = 1)."""
    lib = gtop.load_library()
    mode, depth = ctypes.c_int(7), ctypes.c_double(7.0)
    assert lib.gtop_set_field_sign(None, 1, 0.0) == 1
    assert lib.gtop_get_field_sign(None, ctypes.byref(mode), ctypes.byref(depth)) == 1
    assert mode.value == 7 and depth.value == 7.0
    assert lib.gtop_group_set_field_sign(None, 1, 0.0) == 1
