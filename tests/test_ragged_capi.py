"""rcmarl_ragged_class is declared three times (include/rcmarl.h, csrc/rcmarl_common.h, capi.RaggedClass): the library reports
its own layout, the ctypes structure must match it field by field, and the public header must declare the same fields in the
same order.  Argument validation of the two ragged entry points in the gfx950 build needs no GPU."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ragged_class_structure_is_the_same_in_the_header_the_library_and_the_binding():
    from rcmarl_amd import build, capi
    lib = capi.CLib(build.build_hip())
    assert lib.rcmarl_ragged_class_layout(0) == ctypes.sizeof(capi.RaggedClass) == 16
    for k, name in enumerate(("H", "first", "count"), 1):
        assert lib.rcmarl_ragged_class_layout(k) == getattr(capi.RaggedClass, name).offset, name
    assert capi.RaggedClass.d.offset == 0 and lib.rcmarl_ragged_class_layout(4) == -1
    txt = open(os.path.join(ROOT, "include", "rcmarl.h")).read()
    body = re.search(r"typedef struct rcmarl_ragged_class \{(.*?)\} rcmarl_ragged_class;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*[;,]", body) == [f[0] for f in capi.RaggedClass._fields_]
    assert lib.rcmarl_abi_version() == 4          # additions only


def test_argument_validation_of_the_ragged_entry_points_in_the_product_library():
    import ragged_checks as RC
    from rcmarl_amd import build, capi
    RC.check_argument_validation(capi.CLib(build.build_hip()))
