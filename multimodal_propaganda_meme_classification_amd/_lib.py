"""ctypes binding of libmemehip.so, read from the C ABI's one declaration: include/memehip.h.

At import a small reader turns the header into this module's attributes -- every ``MH_*`` constant, a ctypes class per
struct and the argument and return types of every ``mh_*`` entry point -- so a prototype is written once, in C.  The reader
never skips: a declaration it cannot read stops the import, it does not become a function with ctypes' default int arguments.

The library is built in-tree by ``__graft_entry__.build()`` /
``make -C multimodal_propaganda_meme_classification_amd/csrc``.  There is no
fallback: if it is missing, importing the compute path raises.
"""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmemehip.so")            # bf16 storage
LIB_PATH_F16 = os.path.join(_HERE, "libmemehip_f16.so")    # fp16 storage (same kernels, -DMH_FP16)
LIB_PATHS = {"bf16": LIB_PATH, "fp16": LIB_PATH_F16}
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "memehip.h")


class MemehipError(RuntimeError):
    pass


# The whole type rule.  A pointer to a header struct is POINTER(thatStruct), a returned char pointer is a c_char_p, every other
# pointer (and a `typedef void* name`) is a c_void_p; _POINTEES are the further names that may only be pointed to.
_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint8_t": C.c_uint8,
            "float": C.c_float, "double": C.c_double}
_POINTEES = ("void", "char", "unsigned long long")
_INT = r"-?(?:0[xX][0-9a-fA-F]+|\d+)"
_DECLARATOR = r"(\**)\s*\b(\w+)\s*(?:\[\s*(\w+)\s*\])?"               # stars, name, array bound
_TYPED = re.compile(r"((?:\w+\s+)*\w+)\b\s*" + _DECLARATOR)              # type words, then a declarator
_STATEMENTS = [(kind, re.compile(rx)) for kind, rx in (
    ("enum", r"typedef\s+enum\s+\w*\s*\{([^{}]*)\}\s*(\w+)\s*;"),
    ("struct", r"typedef\s+struct\s+\w*\s*\{([^{}]*)\}\s*(\w+)\s*;"),
    ("handle", r"typedef\s+void\s*\*\s*()(\w+)\s*;"),
    ("proto", r"([\w\s*]+?)\b(mh_\w+)\s*\(([^(){};]*)\)\s*;"))]


def read_header(text: str):
    """C header text -> (constants {name: int}, structs {name: ctypes class}, prototypes {name: (restype, argtypes)}),
    each in header order.  Raises MemehipError, naming the text, for anything outside the forms and the type rule above."""
    def fail(why, what):
        raise MemehipError(f"memehip.h reader: {why}: {' '.join(what.split())!r}")

    consts, structs, handles, protos = {}, {}, {}, {}
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(MH_\w+)\b[ \t]*(.*)$", text, flags=re.M):
        if not re.fullmatch(_INT, value.strip()) or consts.setdefault(name, int(value, 0)) != int(value, 0):
            fail("a constant that is not one integer", f"#define {name} {value}")
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    n_calls = len(re.findall(r"mh_\w+\s*\(", text))
    text, wrapped = re.subn(r'extern\s+"C"\s*\{', " ", text)
    text = text.strip()
    if wrapped:
        text = text[:-1].rstrip() if text.endswith("}") else fail('extern "C" { is not closed at the end', text[-80:])

    def ctype(words, stars, returned=False):
        base = " ".join(w for w in words.split() if w != "const")
        if base in structs:
            return C.POINTER(structs[base]) if stars else structs[base]
        if stars:
            if base not in _SCALARS and base not in _POINTEES and base not in handles:
                fail("a type name outside the rule", words + stars)
            return C.c_char_p if returned and base == "char" else C.c_void_p
        if base not in _SCALARS and base not in handles:
            fail("a type name outside the rule", words)
        return _SCALARS.get(base, C.c_void_p)

    def fields(body):
        out = []
        for stmt in filter(None, (s.strip() for s in body.split(";"))):
            first, *more = stmt.split(",")
            m = _TYPED.fullmatch(first.strip()) or fail("a declarator it cannot split", stmt)
            rest = [re.fullmatch(_DECLARATOR, d.strip()) or fail("a declarator it cannot split", stmt) for d in more]
            for stars, name, bound in [m.groups()[1:]] + [d.groups() for d in rest]:
                t = ctype(m.group(1), stars)
                if bound is not None:
                    if bound not in consts and not re.fullmatch(_INT, bound):
                        fail("an array bound that is neither a known constant nor an integer", stmt)
                    t = t * (consts[bound] if bound in consts else int(bound, 0))
                out.append((name, t))
        return out

    pos = 0
    while pos < len(text):
        for kind, rx in _STATEMENTS:
            m = rx.match(text, pos)
            if m:
                break
        else:
            fail("a declaration it cannot read", text[pos:].split(";")[0][:200])
        pos, (body, name) = re.compile(r"\s*").match(text, m.end()).end(), m.groups()[:2]
        if kind == "enum":
            for item in body.split(","):
                e = re.fullmatch(rf"\s*(\w+)\s*=\s*({_INT})\s*", item) or fail("an enumerator without an integer value", item)
                consts[e.group(1)] = int(e.group(2), 0)
        elif kind == "struct":
            structs[name] = type(name, (C.Structure,), {"_fields_": fields(body)})
        elif kind == "handle":
            handles[name] = C.c_void_p
        else:
            r = re.fullmatch(r"((?:\w+\s+)*\w+)\s*(\**)\s*", body) or fail("a prototype it cannot split", m.group(0))
            args = [] if m.group(3).strip() == "void" else [_TYPED.fullmatch(a.strip()) for a in m.group(3).split(",")]
            if not all(args) or any(a.group(4) for a in args):
                fail("a prototype it cannot split", m.group(0))
            protos[name] = (ctype(r.group(1), r.group(2), returned=True), [ctype(a.group(1), a.group(2)) for a in args])
    if len(protos) != n_calls:
        fail(f"{n_calls} times 'mh_name (' but {len(protos)} prototypes", ", ".join(protos))
    return consts, structs, protos


with open(HEADER_PATH) as _f:
    _CONSTS, _STRUCTS, _SIGNATURES = read_header(_f.read())
globals().update(_CONSTS)       # MH_GEMM_MAX_GROUP, ..., MH_OK, ...
globals().update(_STRUCTS)      # MhGemmProblem, ...
EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_libs = {}


def load(kind: str = "bf16") -> C.CDLL:
    """Load libmemehip.so (kind="bf16") or libmemehip_f16.so (kind="fp16"), once each.
    Raises MemehipError when it has not been built."""
    if kind in _libs:
        return _libs[kind]
    if kind not in LIB_PATHS:
        raise ValueError(f"compute dtype must be 'bf16' or 'fp16', got {kind!r}")
    path = LIB_PATHS[kind]
    if kind == "bf16" and os.environ.get("MEMEHIP_LIB"):      # A/B of two builds of the library in one session
        path = os.environ["MEMEHIP_LIB"]
    if kind == "fp16" and os.environ.get("MEMEHIP_LIB_F16"):
        path = os.environ["MEMEHIP_LIB_F16"]
    if not os.path.exists(path):
        raise MemehipError(
            f"{path} is missing: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()' or make -C "
            "multimodal_propaganda_meme_classification_amd/csrc). There is no CPU/PyTorch fallback.")
    lib = C.CDLL(path)
    for name, (restype, argtypes) in _SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here = header/library drift
        fn.restype, fn.argtypes = restype, argtypes
    _libs[kind] = lib
    return lib


def check(status: int, what: str):
    if status != 0:
        msg = load().mh_status_str(status).decode()
        raise MemehipError(f"{what} failed: status {status} ({msg})")
