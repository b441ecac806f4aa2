"""CPU-only tests of the generated ctypes binding (realtime_video_amd/_lib.py): the structs and prototypes parsed from
include/rtv_hip.h and include/rtv_hip_lab.h cover every declaration, refuse what they do not understand, lay the structs out as
the C compiler does, and are what load() puts on the library's functions."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from realtime_video_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
SCALARS = (ctypes.c_int, ctypes.c_int64, ctypes.c_float)
STRUCT_PTRS = tuple(ctypes.POINTER(s) for s in _lib.STRUCTS.values())


def test_parser_covers_every_declaration_with_expected_kinds():
    assert set(_lib.PROTOTYPES) == set(_lib.declared_symbols()) and len(_lib.PROTOTYPES) == 90
    assert len(_lib.STRUCTS) == 14
    for name, (restype, argtypes) in _lib.PROTOTYPES.items():
        assert restype in (ctypes.c_int, ctypes.c_size_t, ctypes.c_char_p), name
        for t in argtypes:
            assert t in SCALARS + (ctypes.c_size_t, ctypes.c_void_p) + STRUCT_PTRS, (name, t)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, "rtv_hip.h")).read(), flags=re.S)
    bodies = {m.group(2): m.group(1) for m in re.finditer(r"typedef\s+struct\s*\w*\s*\{([^}]*)\}\s*(\w+)\s*;", header)}
    assert list(bodies) == list(_lib.STRUCTS)                   # header order
    for name, cls in _lib.STRUCTS.items():
        # every declarator of the body, found without the parser: an identifier in front of `,` `;` or its array bounds
        assert [n for n, _ in cls._fields_] == re.findall(r"(\w+)\s*(?:\[\d+\]\s*)*[,;]", bodies[name]), name
        for field, t in cls._fields_:
            while issubclass(t, ctypes.Array):
                t = t._type_
            assert t in SCALARS + (ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_float)) \
                + STRUCT_PTRS + tuple(_lib.STRUCTS.values()), (name, field, t)
    # spot checks of each rule against the header text
    S, P = _lib.STRUCTS, _lib.PROTOTYPES
    conv = S["rtv_vae_conv"]
    assert dict(S["rtv_taehv_weights"]._fields_)["mem"] is (conv * 3) * 9                       # rtv_vae_conv mem[9][3]
    assert dict(S["rtv_taehv_weights"]._fields_)["up"] is ctypes.c_void_p * 3                   # const void* up[3]
    assert dict(S["rtv_vae_weights"]._fields_)["up"] is S["rtv_vae_res"] * 12                   # rtv_vae_res mid0, mid2, up[12]
    assert dict(S["rtv_dit_step"]._fields_)["kv_k"] is ctypes.POINTER(ctypes.c_void_p)          # void* const* kv_k
    assert dict(S["rtv_dit_step"]._fields_)["kv_row_stride"] is ctypes.c_int64
    assert dict(S["rtv_dit_weights"]._fields_)["layers"] is ctypes.POINTER(S["rtv_dit_layer_weights"])
    assert dict(S["rtv_dit_weights"]._fields_)["fp8_scales"] is ctypes.POINTER(ctypes.c_float)
    assert dict(S["rtv_vae_attn"]._fields_)["bproj"] is ctypes.c_void_p                         # const void *wq, *bq, ...
    assert P["rtv_version"] == (ctypes.c_int, []) and P["rtv_last_error"] == (ctypes.c_char_p, [])
    assert P["rtv_vae_arena_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 2)
    assert P["rtv_dit_workspace_bytes"] == (ctypes.c_size_t, [ctypes.POINTER(S["rtv_dit_config"])] + [ctypes.c_int] * 3)
    assert P["rtv_gemm_fp8"][1][4:6] == [ctypes.c_void_p, ctypes.c_float]                      # const float* a_scale, float w_scale
    assert P["rtv_silu"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p])
    assert P["rtv_vae_cache_slot"][1] == [ctypes.c_int] * 3 + [ctypes.c_void_p] * 4            # size_t* offset, int* C, ...
    assert P["rtv_rope_set_wave"] == (ctypes.c_int, [ctypes.c_int])                             # lab header
    assert _lib.ABI_VERSION == int(re.search(r"#define RTV_ABI_VERSION (\d+)", header).group(1))


@pytest.mark.parametrize("text,named", [
    ("int rtv_x(unsigned long n);", "rtv_x"),
    ("int rtv_x(const void* a, char** names, void* stream);", "rtv_x"),
    ("long rtv_x(void);", "rtv_x"),
    ("typedef struct { int a; } rtv_s;\nint rtv_x(rtv_s by_value);", "rtv_x"),
    ("typedef struct rtv_s { int a; unsigned long n; } rtv_s;", "rtv_s"),
    ("typedef struct { const rtv_unknown* p; } rtv_s;", "rtv_s"),
    ("typedef struct { void v; } rtv_s;", "rtv_s"),
])
def test_parser_refuses_an_unknown_type(text, named):
    with pytest.raises(ValueError, match=named):
        _lib.parse_header(text, {})
    assert _lib.parse_header("/* c */\n#define X 1\nsize_t rtv_ok(const int* p, rtv_stream_t s);", {}) == \
        {"rtv_ok": (ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_void_p])}


def test_struct_layout_matches_the_c_compiler(tmp_path):
    """sizeof / offsetof as a host-only C++ program that includes rtv_hip.h prints them, against the generated classes."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler found (the build needs one)"
    lines = ["#include <cstddef>", "#include <cstdio>", '#include "rtv_hip.h"', "int main() {"]
    for name, cls in _lib.STRUCTS.items():
        lines.append(f'  std::printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'  std::printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f, _ in cls._fields_]
    src = tmp_path / "layout.cpp"
    src.write_text("\n".join(lines + ["  return 0;", "}", ""]))
    subprocess.run([cxx, "-std=c++17", "-I", INCLUDE, str(src), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout
    got = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    want = {}
    for name, cls in _lib.STRUCTS.items():
        want[name] = ctypes.sizeof(cls)
        want.update({f"{name}.{f}": getattr(cls, f).offset for f, _ in cls._fields_})
    assert got == want
    assert got["rtv_dit_step"] == 152 and got["rtv_dit_step.kv_row_stride"] == 64 and got["rtv_vae_weights"] == 1120


def test_loaded_library_carries_the_generated_prototypes():
    lib = _lib.load()
    assert lib.rtv_version() == _lib.ABI_VERSION
    for name, (restype, argtypes) in _lib.PROTOTYPES.items():
        if os.environ.get("RTV_LIB_PATH") and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    # size_t results beyond what an `int` restype would hand back: the Wan decoder arena at 480 x 832 is past 2^32 bytes, the
    # encoder arena past 2^31 (negative as an int); nothing the library sizes exceeds the 288 GB of one MI355X
    hbm = 288e9
    assert 2 ** 32 < lib.rtv_vae_arena_bytes(60, 104) < hbm
    assert lib.rtv_vae_arena_bytes_rows(60, 104, 0, 480) == lib.rtv_vae_arena_bytes(60, 104)
    assert 2 ** 31 < lib.rtv_vae_enc_arena_bytes(480, 832) < hbm
    assert 0 < lib.rtv_gemm_workspace_bytes() < hbm
    assert 0 < lib.rtv_attn_split_workspace_bytes(1, 4680, 40, 4) < hbm
    assert 0 < lib.rtv_taehv_arena_bytes(60, 104, 3) < lib.rtv_vae_arena_bytes(60, 104)
