"""The ctypes binding (ultrazoom_amd/_ffi.py) against the header it binds: _ffi.PROTOTYPES restates every prototype of
include/mewzoom_hip.h in the header's spelling, and the bound argtypes / restype follow from that text alone.  The header is read here, at
test time; the package never reads it."""

import re
from ctypes import (POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_longlong, c_size_t, c_uint, c_uint8, c_uint32, c_uint64,
                    c_ulonglong, c_void_p)
from pathlib import Path

import pytest

from ultrazoom_amd import _ffi

REPO = Path(__file__).resolve().parent.parent


def prototypes(text: str) -> dict:
    """{name: the prototype on one line, single spaces} of C text without comments and preprocessor lines"""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("#"))
    found = [" ".join(p.split()) for p in re.findall(r"[\w \*]+?\bmz_\w+\([^;{)]*\);", text)]
    table = {re.search(r"\b(mz_\w+)\(", p).group(1): p for p in found}
    assert len(table) == len(found)  # no name twice
    return table


def test_the_table_is_the_header():
    header = prototypes((REPO / "include" / "mewzoom_hip.h").read_text())
    table = prototypes(_ffi.PROTOTYPES)
    assert sorted(table) == sorted(header) and len(header) >= 50  # a function in one and not in the other fails here
    for name, proto in header.items():
        assert table[name] == proto, name
    assert list(_ffi.SIGNATURES) == list(table)  # the parser saw every prototype of the text


def test_every_name_is_bound_in_the_built_library():
    lib = _ffi.lib()
    for name, (restype, argtypes) in _ffi.SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


VIEW, I = POINTER(_ffi.MzImageView), c_int


@pytest.mark.parametrize("name, restype, argtypes", [
    # one function for each scalar type and each pointer rule of _ffi._ctype
    ("mz_blur", I, [VIEW, VIEW, I, I, I, I, c_double, c_void_p]),                                       # int, double, void*, a view
    ("mz_noise", I, [VIEW, VIEW, I, I, I, I, c_double, c_uint64, c_uint64, c_void_p]),                  # uint64_t
    ("mz_op_stem", I, [I, c_void_p, c_void_p, c_void_p, c_void_p, I, I, I, I, c_void_p]),               # const void*, const float*
    ("mz_op_conv_mix", I, [I] + [c_void_p] * 4 + [c_float, c_void_p] + [I] * 5 + [c_void_p]),           # float
    ("mz_jpeg", I, [VIEW, VIEW, I, I, I, I, I, c_void_p, c_size_t, c_void_p]),                          # size_t
    ("mz_jpeg_workspace_bytes", I, [I, I, I, POINTER(c_size_t)]),                                       # size_t*
    ("mz_debug_pack", c_longlong, [I, I, I, I, I, c_void_p, c_longlong]),                               # long long, as a result too
    ("mz_debug_read", I, [c_void_p]),                                                                   # unsigned long long*
    ("mz_debug_tile_list", I, [I] * 9 + [c_void_p, I]),                                                 # unsigned int*
    ("mz_debug_philox", I, [c_void_p, c_void_p, c_void_p]),                                             # T name[N]
    ("mz_flops_per_image", c_double, [c_void_p, I, I]),                                                 # double result, const mz_handle*
    ("mz_last_error", c_char_p, []),                                                                    # const char* result, (void)
    ("mz_debug_select", c_char_p, [I] * 8),
    ("mz_profile_dump", I, [c_void_p, c_char_p]),                                                       # const char* parameter
    ("mz_weight_info", I, [c_void_p, I, POINTER(c_char_p), c_void_p]),                                  # const char**, int64_t[4]
    ("mz_create", I, [POINTER(_ffi.MzConfig), I, POINTER(c_void_p)]),                                   # mz_config*, mz_handle**
    ("mz_debug_schedule", I, [c_void_p, I, I, I, I, I, POINTER(_ffi.MzDebugStep), I]),                  # mz_debug_step*
    ("mz_ensemble_finish", I, [VIEW, I, I, I, I, I, I, c_void_p, c_void_p, c_size_t, c_void_p]),        # const int32_t window[4]
])
def test_bound_types(name, restype, argtypes):
    assert _ffi.SIGNATURES[name] == (restype, argtypes)


def test_scalars_map_exactly_and_unknown_types_are_errors():
    want = {"int": c_int, "unsigned int": c_uint, "long long": c_longlong, "unsigned long long": c_ulonglong, "int32_t": c_int32,
            "int64_t": c_int64, "uint8_t": c_uint8, "uint32_t": c_uint32, "uint64_t": c_uint64, "size_t": c_size_t, "float": c_float,
            "double": c_double}
    for spelling, ctype in want.items():
        pointer = POINTER(c_size_t) if spelling == "size_t" else c_void_p
        assert _ffi._ctype(spelling) is ctype and _ffi._ctype("const " + spelling + "*") is pointer, spelling
    for spelling in ("short", "char", "long", "mz_image_view", "mz_other*", "double**", "void", "void**"):
        with pytest.raises(TypeError, match="no ctypes type"):
            _ffi._ctype(spelling)
    with pytest.raises(TypeError, match="no ctypes type"):
        _ffi._parse("int mz_f(int a, short b);")
    assert _ffi._parse("long long mz_f(const long long* p, unsigned int n);\nconst char* mz_g(void);") == {
        "mz_f": (c_longlong, [c_void_p, c_uint]), "mz_g": (c_char_p, [])}
