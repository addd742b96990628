"""ctypes binding of librs_hip.so (the C ABI in include/radsearch.h).

torch is imported first on purpose: PyTorch-ROCm ships its own libamdhip64.so.7; loading it before
our library makes the dynamic loader resolve our DT_NEEDED entry to the SAME runtime instance, so
device pointers and streams created by torch are valid in our launches."""
import ctypes as C
import os
import re

import torch  # noqa: F401  (must precede CDLL, see module docstring)

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RS_LIB_PATH") or os.path.join(_PKG, "lib", "librs_hip.so")   # override: A/B builds

HEADER_PATH = os.path.join(os.path.dirname(_PKG), "include", "radsearch.h")

# The one mapping from the header's C types to ctypes.  A scalar argument, return value or field is one of _SCALARS; the _POINTEES stand
# behind a pointer only.  Pointers: `const char*` is c_char_p, a pointer to a struct the header defines POINTER(its class), a pointer to
# a pointer POINTER(c_void_p), every other pointer c_void_p (callers pass tensor.data_ptr(), or byref() of an out-parameter).
_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "size_t": C.c_size_t,
            "float": C.c_float, "double": C.c_double, "rs_stream_t": C.c_void_p}
_POINTEES = ("void", "char", "int8_t", "uint8_t", "uint16_t")
# ... but rs_update_state lives in device memory (FusedPPOGrad.state is a tensor): a pointer to it is an address like any tensor's, c_void_p
_DEVICE_STRUCTS = ("rs_update_state",)


def _ctype(t, classes):
    """'int32_t', 'const float*', 'const rs_config*', 'void**' -> the ctypes type; classes {struct name: its Structure, None if opaque}"""
    name, stars = t.rstrip("*").replace("const ", ""), t.count("*")
    if stars == 0:
        if name not in _SCALARS:
            raise ValueError(f"radsearch.h: {t!r} is passed by value, and the binding has no ctypes type for it")
        return _SCALARS[name]
    if stars > 1:
        return C.POINTER(C.c_void_p)
    if t == "const char*":
        return C.c_char_p
    return C.POINTER(classes[name]) if classes.get(name) and name not in _DEVICE_STRUCTS else C.c_void_p


_STARS = r"((?:\*\s*(?:const\b\s*)?)*)"
_FIRST = re.compile(r"(const\s+)?(\w+)\s*" + _STARS + r"(\w+)\s*(?:\[(\d+)\])?")
_NEXT = re.compile(_STARS + r"(\w+)\s*(?:\[(\d+)\])?")


def parse_header(text):
    """The C ABI out of the header's text: (functions, structs, enums, defines).
    functions {name: (return type, [(type, argument name), ...])}; structs {name: [(type, field name, array length or None), ...]}, or
    None for an opaque `typedef struct X X;`; enums and defines {NAME: int}.  A type is spelt 'int32_t', 'const float*', 'void**'.
    Whatever is not one of the forms include/radsearch.h uses raises ValueError with the offending text; nothing is skipped."""
    functions, structs, enums, defines = {}, {}, {}, {}

    def integer(term, where):
        try:
            return defines[term] if term in defines else int(term, 0)
        except ValueError:
            raise ValueError(f"radsearch.h: {term!r} is no integer in {where!r}") from None

    def declarators(decl):
        """'const float *w1, *b1' -> [('const float*', 'w1', None), ('const float*', 'b1', None)]; 'int32_t bbox[4]' -> [('int32_t', 'bbox', 4)]"""
        first, *rest = [p.strip() for p in decl.split(",")]
        m = _FIRST.fullmatch(first)
        more = [_NEXT.fullmatch(p) for p in rest]
        if not m or not all(more):
            raise ValueError(f"radsearch.h: cannot split the declaration {decl!r}")
        if m.group(2) not in _SCALARS and m.group(2) not in _POINTEES and m.group(2) not in structs:
            raise ValueError(f"radsearch.h: unknown type {m.group(2)!r} in {decl!r}")
        base = ("const " if m.group(1) else "") + m.group(2)
        return [(base + "*" * stars.count("*"), name, n and int(n)) for stars, name, n in [m.groups()[2:]] + [x.groups() for x in more]]

    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    for line in re.findall(r"^[ \t]*#.*$", text, re.M):               # #define NAME int | #define NAME (int + NAME); the guards
        line = " ".join(line.split())
        if re.fullmatch(r"#(include <\w+\.h>|ifn?def \w+|endif|define \w+)", line):
            continue
        m = re.fullmatch(r"#define (\w+) \(?([^()]+)\)?", line)
        if not m:
            raise ValueError(f"radsearch.h: not an integer #define: {line!r}")
        defines[m.group(1)] = sum(integer(t.strip(), line) for t in m.group(2).split("+"))
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    if m := re.search(r'extern\s*"C"\s*\{', text):                    # ... and its closing brace, the last one of the file
        text = text[:m.start()] + text[m.end():text.rindex("}")] + text[text.rindex("}") + 1:]
    stmt, depth = "", 0
    for ch in text:
        depth += (ch == "{") - (ch == "}")
        if ch != ";" or depth:
            stmt += ch
            continue
        s, stmt = " ".join(stmt.split()), ""
        if m := re.fullmatch(r"typedef struct (\w+) (\w+)", s):
            structs[m.group(2)] = None
        elif m := re.fullmatch(r"typedef struct (?:\w+ )?\{(.*)\} (\w+)", s):
            structs[m.group(2)] = [f for decl in m.group(1).split(";") if decl.strip() for f in declarators(decl.strip())]
        elif m := re.fullmatch(r"enum \{(.*)\}", s):
            for member in m.group(1).split(","):
                if not (e := re.fullmatch(r"(\w+) = (-?\w+)", member.strip())):
                    raise ValueError(f"radsearch.h: not an enum member NAME = int: {member.strip()!r}")
                enums[e.group(1)] = integer(e.group(2), member.strip())
        elif m := re.fullmatch(r"typedef void ?\* ?(\w+)", s):
            if _SCALARS.get(m.group(1)) is not C.c_void_p:
                raise ValueError(f"radsearch.h: unknown type {m.group(1)!r} in {s!r}")
        elif m := re.fullmatch(r"([^()]+?) ?\((.*)\)", s):            # `return type name` splits as a declarator does
            (ret, name, _), = declarators(m.group(1))
            functions[name] = (ret, [] if m.group(2).strip() == "void" else [declarators(a)[0][:2] for a in m.group(2).split(",")])
        else:
            raise ValueError(f"radsearch.h: not a declaration this reader knows: {s!r}")
    if stmt.strip():
        raise ValueError(f"radsearch.h: unterminated declaration: {' '.join(stmt.split())!r}")
    return functions, structs, enums, defines


if not os.path.exists(HEADER_PATH):
    raise RuntimeError(f"{HEADER_PATH} is missing: the ctypes binding of librs_hip.so is read from the C header at import, "
                       "so the package needs the source tree's include/ directory next to it.")
_functions, _structs, _enums, _defines = parse_header(open(HEADER_PATH).read())

# the header's structs by their C names; each also under its class name, rs_collect_state -> RsCollectState
STRUCTS = {}
for _name, _fields in _structs.items():
    if _fields:                                                       # an opaque one stays a pointee
        STRUCTS[_name] = type("".join(w.capitalize() for w in _name.split("_")), (C.Structure,), {
            "__doc__": f"{_name} (include/radsearch.h)",
            "_fields_": [(f, _ctype(t, STRUCTS) * n if n else _ctype(t, STRUCTS)) for t, f, n in _fields]})
globals().update({c.__name__: c for c in STRUCTS.values()})

# the header's enum members and integer #defines under their own names: RS_ABI_VERSION, RS_ERR_INVALID_ARG, RS_ENVERR_NO_PATH, ...
CONSTANTS = {**_enums, **_defines}
globals().update(CONSTANTS)

# every function the header declares, in its order: (name, restype, argtypes)
SYMBOLS = [(_name, None if _ret == "void" else _ctype(_ret, STRUCTS), [_ctype(t, STRUCTS) for t, _ in _args])
           for _name, (_ret, _args) in _functions.items()]

_lib = None

# Optional kernel timing for bench.py: when EVENTS is a dict, every library call wrapped in `timed(name)` is bracketed by
# HIP events on the stream it is launched on (torch's current stream) and the pair is appended to EVENTS[name].
EVENTS = None


class timed:
    def __init__(self, name: str):
        self.name = name

    def __enter__(self):
        self.ev = None
        if EVENTS is not None and not torch.cuda.is_current_stream_capturing():     # no timing events inside a graph capture
            self.ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            self.ev[0].record()
        return self

    def __exit__(self, *exc):
        if self.ev is not None:
            self.ev[1].record()
            EVENTS.setdefault(self.name, []).append(self.ev)
        return False


def load():
    """Load librs_hip.so (once).  Fails loudly: there is no fallback implementation."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the MI355X HIP extension has not been built "
            "(run `python -c 'import __graft_entry__ as g; g.build()'` or `python radiation_ppo_amd/build.py`). "
            "There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, restype, argtypes in SYMBOLS:
        fn = getattr(lib, name)          # AttributeError if the library does not export it
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.rs_abi_version() != RS_ABI_VERSION:
        raise RuntimeError("librs_hip.so ABI version mismatch")
    _lib = lib
    return lib


def check(code: int, what: str = "") -> None:
    if code != 0:
        msg = load().rs_strerror(code).decode()
        raise RuntimeError(f"librs_hip {what}: {msg} (code {code})")
