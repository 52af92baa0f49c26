"""ctypes binding of libnsid_hip.so (C ABI: include/nsid.h).

The product path has no CPU fallback: if the library is missing this module raises, and every op raises
RuntimeError on a non-zero return code."""
import ctypes
import os
import re

import torch  # noqa: F401  -- must come first: torch bundles its own libamdhip64; loading the kernel library before it
#                              would bind the system HIP runtime and leave two runtimes in one process

_PKG = os.path.dirname(os.path.abspath(__file__))
# NSID_LIB: path of an alternative BUILD of the same library (one-box kernel A/B, tools/build_variant.sh). It selects which .so is
# loaded, nothing inside the library reads the environment; bench.py records an override in its JSON line (config.lib).
LIB_PATH = os.environ.get("NSID_LIB") or os.path.join(_PKG, "libnsid_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_PKG), "include", "nsid.h")      # the C ABI; build.py compiles against the same file

# type letters: p = pointer, s = the `void* stream` parameter, i = int / int32_t, l = long / int64_t, z = size_t, f = float, d = double,
# c = const char*. include/nsid.h is the only description of the entry points: nothing below names one.
_CT = {"p": ctypes.c_void_p, "s": ctypes.c_void_p, "i": ctypes.c_int, "l": ctypes.c_long, "z": ctypes.c_size_t, "f": ctypes.c_float,
       "d": ctypes.c_double, "c": ctypes.c_char_p}
_SCALARS = {"int": "i", "int32_t": "i", "long": "l", "int64_t": "l", "size_t": "z", "float": "f", "double": "d"}
_POINTEES = {"void", "char", "float", "double", "int", "long", "int32_t", "int64_t", "uint8_t", "size_t"}


def _letter(ctype: str, pointees) -> str:
    """type letter of a C type without its parameter name; KeyError (parse_header's ImportError) for a type outside the alphabet"""
    words = ctype.replace("*", " * ").split()
    base = [w for w in words if w not in ("const", "*")]
    if len(base) != 1:
        raise KeyError(ctype)
    if "*" not in words:
        return _SCALARS[base[0]]
    if base[0] not in pointees:
        raise KeyError(ctype)
    return "c" if words == ["const", "char", "*"] else "p"


def parse_header(text: str):
    """(prototypes, defines) of a C header in the style of include/nsid.h: prototypes = {name: (return letter, parameter letters)} in
    header order, defines = {NSID_*: int}. Fails closed: a declaration, a type or an NSID_* define it does not understand raises
    ImportError naming it; nothing defaults to int."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    scanned = set(re.findall(r"\b(nsid_\w+)\s*\(", text))
    guards = set(re.findall(r"^[ \t]*#[ \t]*ifndef[ \t]+(\w+)", text, flags=re.M))
    defines = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(NSID_\w+)(.*)$", text, flags=re.M):
        if name in guards and not value.strip():
            continue
        m = re.fullmatch(r"\s+(?:\(\s*([+-]?\d+)\s*\)|([+-]?\d+))\s*", value)
        if not m:
            raise ImportError(f"#define {name}{value.rstrip()}: not an integer constant")
        defines[name] = int(m.group(1) or m.group(2))
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', " ", text)
    structs = set()

    def skip_struct(m):
        structs.add(m.group(1))
        return " "
    text = re.sub(r"typedef\s+struct\b[^{;]*\{[^{}]*\}\s*(\w+)\s*;", skip_struct, text)
    *statements, rest = text.split(";")
    if rest.strip() not in ("", "}"):
        raise ImportError(f"cannot parse the end of the header: {' '.join(rest.split())[:80]!r}")
    prototypes = {}
    for statement in statements:
        statement = " ".join(statement.split())
        m = re.fullmatch(r"(.*?)\b(nsid_\w+) ?\((.*)\)", statement)
        if not m or m.group(2) in prototypes:
            raise ImportError(f"cannot parse the declaration {statement[:120]!r}")
        ret, name, params = m.groups()
        try:
            letters = _letter(ret, {"char"})
            if letters not in "ilzc":
                raise KeyError(ret)
            for param in ([] if params.strip() == "void" else params.split(",")):
                pm = re.fullmatch(r"(.*[\s*])(\w+)", param.strip())
                if not pm:
                    raise KeyError(param)
                letter = _letter(pm.group(1), _POINTEES | structs)
                letters += "s" if pm.group(2) == "stream" and pm.group(1).replace(" ", "") == "void*" else letter
        except KeyError as e:
            raise ImportError(f"{name}: unknown type or unsplittable parameter {e.args[0].strip()!r}") from None
        prototypes[name] = (letters[0], letters[1:])
    if set(prototypes) != scanned:
        raise ImportError(f"prototypes parsed and names scanned disagree: {sorted(set(prototypes) ^ scanned)}")
    return prototypes, defines


def load_header():
    if not os.path.exists(HEADER_PATH):
        raise ImportError(f"{HEADER_PATH} is missing: the ctypes binding is derived from it")
    with open(HEADER_PATH) as f:
        return parse_header(f.read())


PROTOTYPES, DEFINES = load_header()
SIGNATURES = {name: args for name, (_, args) in PROTOTYPES.items()}
EXPORTS = list(SIGNATURES)


class WgradProblem(ctypes.Structure):
    """include/nsid.h nsid_wgrad_problem: one layer's weight gradient over up to two row segments (the two views)"""
    _fields_ = [("dout", ctypes.c_void_p * 2), ("x", ctypes.c_void_p * 2), ("in_scale", ctypes.c_void_p * 2),
                ("in_shift", ctypes.c_void_p * 2), ("dw", ctypes.c_void_p), ("ldd", ctypes.c_int), ("ldx", ctypes.c_int),
                ("M", ctypes.c_int), ("Nout", ctypes.c_int), ("K", ctypes.c_int), ("groups", ctypes.c_int), ("act_in", ctypes.c_int),
                ("ds_out_nodes", ctypes.c_int)]


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -m neuralsampleid_amd.build` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback for the product path.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (ret, args) in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.argtypes = [_CT[c] for c in args]
        fn.restype = _CT[ret]
    if lib.nsid_version() < 0:      # (builds of rounds 3-4 with result-changing timing switches reported a negative version)
        raise ImportError(f"{LIB_PATH} reports a negative version: not a product build of this tree; rebuild with "
                          "`python -m neuralsampleid_amd.build --force`")
    return lib


lib = _load()

_ERR = {DEFINES["NSID_EINVAL"]: "NSID_EINVAL (unsupported shape, misaligned pointer or bad argument)",
        DEFINES["NSID_ELAUNCH"]: "NSID_ELAUNCH (HIP runtime refused the launch)",
        DEFINES["NSID_DECLINED"]: "NSID_DECLINED (the fused form does not serve this call; nothing was launched)"}


def call(name, *args):
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise RuntimeError(f"{name} failed: {_ERR.get(rc, rc)}")


def set_tuning(key: str, value: int) -> None:
    """one launch-heuristic constant of the kernel library (include/nsid.h nsid_set_tuning; keys: tuning_keys())"""
    if lib.nsid_set_tuning(key.encode(), int(value)) != 0:
        raise KeyError(f"unknown tuning key {key!r}; known: {', '.join(tuning_keys())}")


def get_tuning(key: str) -> int:
    v = ctypes.c_long()
    if lib.nsid_get_tuning(key.encode(), ctypes.byref(v)) != 0:
        raise KeyError(f"unknown tuning key {key!r}")
    return int(v.value)


def reset_tuning() -> None:
    lib.nsid_reset_tuning()


def launch_counters(reset: bool = False) -> dict:
    """launches per kernel variant since the last reset (include/nsid.h nsid_debug_counter)"""
    out = {}
    for i in range(lib.nsid_debug_counter_count()):
        k = lib.nsid_debug_counter_key(i)
        out[k.decode()] = int(lib.nsid_debug_counter(k))
    if reset:
        lib.nsid_debug_counters_reset()
    return out


def tuning_keys():
    return [lib.nsid_tuning_key(i).decode() for i in range(lib.nsid_tuning_count())]
