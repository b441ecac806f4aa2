"""ctypes binding of librtv_hip.so (the C-ABI HIP kernel library), generated from include/rtv_hip.h and include/rtv_hip_lab.h:
STRUCTS (the ABI structs as ctypes.Structure classes), PROTOTYPES (restype / argtypes of every declared function, which load()
puts on the library) and ABI_VERSION are parsed from the headers at import; nothing restates them by hand.  The pixel input side,
include/rtv_hip_io.h, is parsed the same way into tables of its own (IO_STRUCTS / IO_PROTOTYPES) until it is folded into rtv_hip.h,
and so are the frame delivery side, include/rtv_hip_jpeg.h (JPEG_STRUCTS / JPEG_PROTOTYPES), and the JPEG frame decoder,
include/rtv_hip_jpeg_decode.h (JPEGDEC_STRUCTS / JPEGDEC_PROTOTYPES), and the LoRA merge, include/rtv_hip_lora.h (LORA_STRUCTS /
LORA_PROTOTYPES), with its dense-delta and DoRA forms, include/rtv_hip_lora_ext.h (LORA_EXT_STRUCTS / LORA_EXT_PROTOTYPES), and the folded text cross-attention, include/rtv_hip_cross_fold.h (CROSS_FOLD_PROTOTYPES), and the fp8 Linears
with per-row scales, include/rtv_hip_fp8_rows.h (FP8_ROWS_PROTOTYPES), and the fp8 self-attention on an e4m3 shadow of the KV cache,
include/rtv_hip_attn_fp8.h (ATTN_FP8_STRUCTS / ATTN_FP8_PROTOTYPES), with the K smoothing of that shadow,
include/rtv_hip_attn_fp8_center.h (ATTN_FP8_CENTER_PROTOTYPES), its KV split and sharded phases,
include/rtv_hip_attn_fp8_cp.h (ATTN_FP8_CP_PROTOTYPES), and the e4m3-only KV cache of that mode,
include/rtv_hip_attn_fp8_only.h (ATTN_FP8_ONLY_PROTOTYPES), with K smoothing on that cache,
include/rtv_hip_attn_fp8_only_center.h (ATTN_FP8_ONLY_CENTER_PROTOTYPES), and that cache under the row exchange of context
parallelism with the exchange carrying codes, include/rtv_hip_attn_fp8_only_cp.h (ATTN_FP8_ONLY_CP_PROTOTYPES), and the MXFP4 Linears, include/rtv_hip_mxfp4.h (MXFP4_PROTOTYPES), and the MXFP6
Linears, include/rtv_hip_mxfp6.h (MXFP6_PROTOTYPES), and the block Hadamard rotation in front of both quantisers,
include/rtv_hip_mx_rotate.h (MX_ROTATE_PROTOTYPES), and the unit entry points of the text encoder's kernels,
include/rtv_hip_t5_units.h (T5_UNITS_PROTOTYPES), and the text encoder on e4m3 weights with its skinny-M weight-only GEMM,
include/rtv_hip_t5_w8.h (T5_W8_STRUCTS / T5_W8_PROTOTYPES).

The product path has no CPU / eager fallback: if the library is missing or a kernel reports an
error, a RuntimeError is raised (the reference's attention()/pipeline API reports errors as Python
exceptions, wan/modules/attention.py:72-73,129).
"""
import ctypes
import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
# RTV_LIB_PATH: A/B measurements against another build of the same C ABI (scripts/ab_build.sh); never set in production
LIB_PATH = os.environ.get("RTV_LIB_PATH") or os.path.join(_HERE, "librtv_hip.so")
CSRC = os.path.join(_HERE, "csrc")

_INCLUDE = os.path.join(os.path.dirname(_HERE), "include")
HEADERS = ("rtv_hip.h", "rtv_hip_lab.h")

_lib = None

_SCALARS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double,
            "size_t": ctypes.c_size_t}
_RETURNS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "const char*": ctypes.c_char_p}
_STARS = r"(\*(?:\s*const\s*\*)?)?"     # nothing, `*` or `* const*`


def _field_type(base, stars, structs):
    value = _SCALARS.get(base) or structs.get(base)
    if not stars:
        return value                                  # None for `void` and unknown names: the caller raises
    if base == "void":
        return ctypes.c_void_p if stars == "*" else ctypes.POINTER(ctypes.c_void_p)
    return ctypes.POINTER(value) if value and stars == "*" else None


def _param_type(base, stars, structs):
    if not stars:
        return ctypes.c_void_p if base == "rtv_stream_t" else _SCALARS.get(base)
    if base in structs:
        return ctypes.POINTER(structs[base]) if stars == "*" else None
    # device addresses arrive as Python ints, out-parameters as byref() / ctypes arrays: c_void_p takes all of them
    return ctypes.c_void_p if base == "void" or base in _SCALARS else None


def parse_header(text, structs):
    """One C header of the ABI -> {function: (restype, argtypes)}; its struct typedefs are added to `structs` as generated
    ctypes.Structure classes (header order, so nested structs resolve).  The headers are the only statement of the ABI: a
    declaration this parser does not understand raises, it never gets a default type."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"#ifdef __cplusplus.*?#endif", "", text, flags=re.S)          # the extern "C" braces
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    text = re.sub(r"\benum\s*\{[^}]*\}\s*;|\btypedef\s+void\s*\*\s*rtv_stream_t\s*;", "", text)

    def struct(m):
        name, fields = m.group(2), []
        for decl in filter(None, (d.strip() for d in m.group(1).split(";"))):
            head = re.match(r"(?:const\s+)?(\w+)\s*", decl)
            for item in decl[head.end():].split(","):
                d = re.fullmatch(_STARS + r"\s*(\w+)((?:\s*\[\d+\])*)", item.strip())
                t = d and _field_type(head.group(1), re.sub(r"\s", "", d.group(1) or ""), structs)
                if not t:
                    raise ValueError(f"{name}: cannot bind field declaration `{decl}`")
                for n in reversed(re.findall(r"\d+", d.group(3))):
                    t = t * int(n)
                fields.append((d.group(2), t))
        structs[name] = type(name, (ctypes.Structure,), {"_fields_": fields})
        return ""

    text = re.sub(r"\btypedef\s+struct\s*\w*\s*\{([^}]*)\}\s*(\w+)\s*;", struct, text)
    protos = {}
    for stmt in filter(None, (" ".join(s.split()) for s in text.split(";"))):
        m = re.fullmatch(r"(.*?)\s*\b(\w+)\s*\((.*)\)", stmt)
        if not m:
            raise ValueError(f"cannot bind declaration `{stmt}`")
        ret, name, params = m.group(1).replace(" *", "*"), m.group(2), m.group(3).strip()
        if ret not in _RETURNS:
            raise ValueError(f"{name}: cannot bind return type `{ret}`")
        argtypes = []
        for param in ([] if params == "void" else params.split(",")):
            d = re.fullmatch(r"(?:const\s+)?(\w+)\s*" + _STARS + r"\s*(\w+)?", param.strip())
            t = d and _param_type(d.group(1), re.sub(r"\s", "", d.group(2) or ""), structs)
            if not t:
                raise ValueError(f"{name}: cannot bind parameter `{param.strip()}`")
            argtypes.append(t)
        protos[name] = (_RETURNS[ret], argtypes)
    return protos


def _read(name):
    with open(os.path.join(_INCLUDE, name)) as f:
        return f.read()


STRUCTS, PROTOTYPES = {}, {}      # struct name -> ctypes.Structure class; function name -> (restype, argtypes)
for _name in HEADERS:
    PROTOTYPES.update(parse_header(_read(_name), STRUCTS))
IO_HEADER = "rtv_hip_io.h"
IO_STRUCTS = dict(STRUCTS)        # the io header may use the ABI's structs; what it adds stays out of STRUCTS
IO_PROTOTYPES = parse_header(_read(IO_HEADER), IO_STRUCTS)
IO_STRUCTS = {k: v for k, v in IO_STRUCTS.items() if k not in STRUCTS}
JPEG_HEADER = "rtv_hip_jpeg.h"   # frame delivery side (JPEG encoder), kept apart like the io header
JPEG_STRUCTS = dict(STRUCTS)
JPEG_PROTOTYPES = parse_header(_read(JPEG_HEADER), JPEG_STRUCTS)
JPEG_STRUCTS = {k: v for k, v in JPEG_STRUCTS.items() if k not in STRUCTS}
JPEGDEC_HEADER = "rtv_hip_jpeg_decode.h"   # frame input side, second half (JPEG decoder): its descriptor struct stays out of STRUCTS
JPEGDEC_STRUCTS = dict(STRUCTS)
JPEGDEC_PROTOTYPES = parse_header(_read(JPEGDEC_HEADER), JPEGDEC_STRUCTS)
JPEGDEC_STRUCTS = {k: v for k, v in JPEGDEC_STRUCTS.items() if k not in STRUCTS}
LORA_HEADER = "rtv_hip_lora.h"   # LoRA adapters merged into the DiT's weights in place: its adapter struct stays out of STRUCTS
LORA_STRUCTS = dict(STRUCTS)
LORA_PROTOTYPES = parse_header(_read(LORA_HEADER), LORA_STRUCTS)
LORA_STRUCTS = {k: v for k, v in LORA_STRUCTS.items() if k not in STRUCTS}
LORA_EXT_HEADER = "rtv_hip_lora_ext.h"   # dense-delta and DoRA merges: the term struct stays out of STRUCTS and of LORA_STRUCTS
LORA_EXT_STRUCTS = dict(STRUCTS)
LORA_EXT_PROTOTYPES = parse_header(_read(LORA_EXT_HEADER), LORA_EXT_STRUCTS)
LORA_EXT_STRUCTS = {k: v for k, v in LORA_EXT_STRUCTS.items() if k not in STRUCTS}
CROSS_FOLD_HEADER = "rtv_hip_cross_fold.h"   # the folded text cross-attention: three entry points, no struct of its own
CROSS_FOLD_STRUCTS = dict(STRUCTS)
CROSS_FOLD_PROTOTYPES = parse_header(_read(CROSS_FOLD_HEADER), CROSS_FOLD_STRUCTS)
FP8_ROWS_HEADER = "rtv_hip_fp8_rows.h"   # fp8 Linears with per-row scales: three entry points, no struct of its own
FP8_ROWS_PROTOTYPES = parse_header(_read(FP8_ROWS_HEADER), dict(STRUCTS))
ATTN_FP8_HEADER = "rtv_hip_attn_fp8.h"   # fp8 self-attention: the shadow struct rtv_dit_step.attn_fp8 points at stays out of STRUCTS
ATTN_FP8_STRUCTS = dict(STRUCTS)
ATTN_FP8_PROTOTYPES = parse_header(_read(ATTN_FP8_HEADER), ATTN_FP8_STRUCTS)
ATTN_FP8_STRUCTS = {k: v for k, v in ATTN_FP8_STRUCTS.items() if k not in STRUCTS}
ATTN_FP8_CENTER_HEADER = "rtv_hip_attn_fp8_center.h"   # K smoothing of the shadow: four entry points, no struct of its own (it takes the shadow struct)
ATTN_FP8_CENTER_PROTOTYPES = parse_header(_read(ATTN_FP8_CENTER_HEADER), {**STRUCTS, **ATTN_FP8_STRUCTS})
ATTN_FP8_CP_HEADER = "rtv_hip_attn_fp8_cp.h"   # the KV split of the fp8 attention kernel and the fp8 forms of the sharded phases: four entry points, no struct of its own
ATTN_FP8_CP_PROTOTYPES = parse_header(_read(ATTN_FP8_CP_HEADER), {**STRUCTS, **ATTN_FP8_STRUCTS})
ATTN_FP8_ONLY_HEADER = "rtv_hip_attn_fp8_only.h"   # the e4m3-only KV cache (no bf16 arena beside the shadow): three entry points, no struct of its own
ATTN_FP8_ONLY_PROTOTYPES = parse_header(_read(ATTN_FP8_ONLY_HEADER), {**STRUCTS, **ATTN_FP8_STRUCTS})
ATTN_FP8_ONLY_CENTER_HEADER = "rtv_hip_attn_fp8_only_center.h"   # K smoothing on the e4m3-only cache: four entry points, no struct of its own
ATTN_FP8_ONLY_CENTER_PROTOTYPES = parse_header(_read(ATTN_FP8_ONLY_CENTER_HEADER), {**STRUCTS, **ATTN_FP8_STRUCTS})
ATTN_FP8_ONLY_CP_HEADER = "rtv_hip_attn_fp8_only_cp.h"   # the e4m3-only cache under the row exchange, codes on the wire: five entry points, no struct of its own
ATTN_FP8_ONLY_CP_PROTOTYPES = parse_header(_read(ATTN_FP8_ONLY_CP_HEADER), {**STRUCTS, **ATTN_FP8_STRUCTS})
MXFP4_HEADER = "rtv_hip_mxfp4.h"   # MXFP4 Linears (e2m1 codes, e8m0 block scales): three entry points, no struct of its own
MXFP4_PROTOTYPES = parse_header(_read(MXFP4_HEADER), dict(STRUCTS))
MXFP6_HEADER = "rtv_hip_mxfp6.h"   # MXFP6 Linears (e2m3 codes, e8m0 block scales): three entry points, no struct of its own
MXFP6_PROTOTYPES = parse_header(_read(MXFP6_HEADER), dict(STRUCTS))
MX_ROTATE_HEADER = "rtv_hip_mx_rotate.h"   # the rotated MXFP4 / MXFP6 quantisers: four entry points, no struct of its own
MX_ROTATE_PROTOTYPES = parse_header(_read(MX_ROTATE_HEADER), dict(STRUCTS))
T5_UNITS_HEADER = "rtv_hip_t5_units.h"   # one launcher per kernel of the text encoder, for its unit tests: no struct of its own
T5_UNITS_PROTOTYPES = parse_header(_read(T5_UNITS_HEADER), dict(STRUCTS))
T5_W8_HEADER = "rtv_hip_t5_w8.h"   # the text encoder on e4m3 weights: its two weight structs stay out of STRUCTS
T5_W8_STRUCTS = dict(STRUCTS)
T5_W8_PROTOTYPES = parse_header(_read(T5_W8_HEADER), T5_W8_STRUCTS)
T5_W8_STRUCTS = {k: v for k, v in T5_W8_STRUCTS.items() if k not in STRUCTS}
MX_ROT_ACT_SHIFT, MX_ROT_WEIGHT_SHIFT, MX_ROT_MAX_SHIFT = (
    int(re.search(rf"^#define\s+RTV_MX_ROT_{n}_SHIFT\s+(\d+)", _read(MX_ROTATE_HEADER), flags=re.M).group(1)) for n in ("ACT", "WEIGHT", "MAX"))
LORA_MAX_ADAPTERS, LORA_MAX_RANK = (int(re.search(rf"^#define\s+RTV_LORA_MAX_{n}\s+(\d+)", _read(LORA_HEADER), flags=re.M).group(1))
                                    for n in ("ADAPTERS", "RANK"))
FRAMES_MAX = int(re.search(r"^#define\s+RTV_FRAMES_MAX\s+(\d+)", _read(IO_HEADER), flags=re.M).group(1))
ABI_VERSION = int(re.search(r"^#define\s+RTV_ABI_VERSION\s+(\d+)", _read(HEADERS[0]), flags=re.M).group(1))


def build(verbose=False):
    """Compile librtv_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    # MAX_JOBS if the environment sets it, else the CPUs this process may use, at most 16 (os.cpu_count() counts the whole host)
    jobs = os.environ.get("MAX_JOBS") or str(min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count() or 4))
    cmd = ["make", "-C", CSRC, "-j", jobs]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout[-4000:])
        print(res.stderr[-4000:])
    if res.returncode != 0:
        raise RuntimeError("building librtv_hip.so failed")
    return LIB_PATH


def declared_symbols(lab=True):
    """Every extern "C" function declared in include/rtv_hip.h - the drop-in boundary - and, with `lab`, in
    include/rtv_hip_lab.h (test / measurement hooks, not part of the boundary), parsed from the headers."""
    out = set()
    for name in HEADERS if lab else HEADERS[:1]:
        text = re.sub(r"/\*.*?\*/", "", _read(name), flags=re.S)
        out.update(re.findall(r"\b(rtv_[a-z0-9_]+)\s*\(", text))
    return sorted(out)


def load():
    """Load the library (no compute happens here; safe on a CPU-only box)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C realtime_video_amd/csrc`). There is no CPU fallback for the HIP path.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in list(PROTOTYPES.items()) + list(IO_PROTOTYPES.items()) + list(JPEG_PROTOTYPES.items()) + list(JPEGDEC_PROTOTYPES.items()) + list(LORA_PROTOTYPES.items()) + list(LORA_EXT_PROTOTYPES.items()) + list(CROSS_FOLD_PROTOTYPES.items()) + list(FP8_ROWS_PROTOTYPES.items()) + list(ATTN_FP8_PROTOTYPES.items()) + list(ATTN_FP8_CENTER_PROTOTYPES.items()) + list(ATTN_FP8_CP_PROTOTYPES.items()) + list(ATTN_FP8_ONLY_PROTOTYPES.items()) + list(ATTN_FP8_ONLY_CENTER_PROTOTYPES.items()) + list(ATTN_FP8_ONLY_CP_PROTOTYPES.items()) + list(MXFP4_PROTOTYPES.items()) + list(MXFP6_PROTOTYPES.items()) + list(MX_ROTATE_PROTOTYPES.items()) + list(T5_UNITS_PROTOTYPES.items()) + list(T5_W8_PROTOTYPES.items()):
        fn = getattr(lib, name, None)
        if fn is None:
            # RTV_LIB_PATH = an older build of the same C ABI (A/B measurements): entry points added since are simply absent
            if os.environ.get("RTV_LIB_PATH"):
                continue
            raise RuntimeError(f"librtv_hip.so does not export {name}")
        fn.restype, fn.argtypes = restype, argtypes
    have = lib.rtv_version()
    if have != ABI_VERSION:
        # struct layouts (rtv_dit_config, rtv_dit_step, ...) are part of the ABI: a library of another revision would read
        # garbage for fields it does not know.  RTV_LIB_PATH (A/B against an older build) is no exception.
        raise RuntimeError(f"{LIB_PATH} reports ABI revision {have}, include/rtv_hip.h declares RTV_ABI_VERSION {ABI_VERSION}: "
                           "rebuild the library (`make -C realtime_video_amd/csrc`)")
    _lib = lib
    return lib


def check(status, what):
    if status != 0:
        msg = load().rtv_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{what} failed (status {status}): {msg}")


def call(name, *args):
    check(getattr(load(), name)(*args), name)
