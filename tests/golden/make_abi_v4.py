"""Recorder of tests/golden/abi_v4.json: the ctypes binding of ABI version 4 as the last hand-written table held it.

    python tests/golden/make_abi_v4.py FILE       FILE: that table, `git show 79d88c8:radiation_ppo_amd/_lib.py > FILE`

The table is executed with a stand-in for ctypes whose types are the words of the record's vocabulary (i32 i64 u32 int size f32 f64 cstr
ptr ptr:<struct> pptr void), so that `int` and `int32_t`, one ctypes type on most platforms, stay apart as the table spelt them.  The
table's five POINTER(c_int32) / POINTER(c_uint32) out-parameters (rs_state_field, rs_maps_field, rs_error_flags) are recorded as `ptr`:
the vocabulary has no word for them, and the binding derived from the header passes them as plain addresses.  The constants are what
the C compiler reads out of include/radsearch.h, which the table's own literals (RS_OBS_DIM, ENVERR_*, MAPERR_*, the 4 of load()) are
asserted against.  tests/test_abi_cpu.py holds every later binding to this record; entries may be appended, none may change."""
import json
import os
import re
import subprocess
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HEADER = os.path.join(ROOT, "include", "radsearch.h")


class Kind(str):
    def __mul__(self, n):                      # a fixed array in a _fields_ list
        return (self, n)


class Structure:
    pass


def c_name(cls):
    return re.sub(r"(?<!^)(?=[A-Z])", "_", cls.__name__).lower()           # RsCnnHeadParams -> rs_cnn_head_params


def pointer(t):
    if isinstance(t, type) and issubclass(t, Structure):
        return Kind("ptr:" + c_name(t))
    return Kind("pptr" if t == "ptr" else "ptr")


C = types.SimpleNamespace(Structure=Structure, POINTER=pointer, c_int32=Kind("i32"), c_int64=Kind("i64"), c_uint32=Kind("u32"),
                          c_int=Kind("int"), c_size_t=Kind("size"), c_float=Kind("f32"), c_double=Kind("f64"), c_char_p=Kind("cstr"),
                          c_void_p=Kind("ptr"))


def constants():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = re.findall(r"^#define (RS_\w+) \S", src, re.M) + re.findall(r"\b(RS_\w+) = ", src)
    prog = '#include <stdio.h>\n#include "radsearch.h"\nint main(void) {\n' + "".join(
        f'    printf("{n} %lld\\n", (long long)({n}));\n' for n in names) + "    return 0;\n}\n"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "c.c"), "w").write(prog)
        subprocess.run(["cc", "-I", os.path.dirname(HEADER), os.path.join(d, "c.c"), "-o", os.path.join(d, "c")], check=True)
        out = subprocess.run([os.path.join(d, "c")], check=True, capture_output=True, text=True).stdout
    return {line.split()[0]: int(line.split()[1]) for line in out.splitlines()}


def main(table):
    src = open(table).read()
    assert "import ctypes as C\n" in src and "rs_abi_version() != 4" in src
    ns = {"C": C, "__file__": os.path.join(ROOT, "radiation_ppo_amd", "_lib.py")}
    exec(compile(src.replace("import ctypes as C\n", ""), table, "exec"), ns)
    functions = {name: {"ret": "void" if ret is None else ret, "args": list(args)} for name, ret, args in ns["SYMBOLS"]}
    assert len(functions) == len(ns["SYMBOLS"])
    structs = {c_name(v): [[f, *(t if isinstance(t, tuple) else (t, None))] for f, t in v._fields_]
               for v in ns.values() if isinstance(v, type) and issubclass(v, Structure) and v is not Structure}
    const = constants()
    assert const["RS_ABI_VERSION"] == 4
    for k, v in ns.items():                                                # the table's own copies
        if re.match(r"(RS_|ENVERR_|MAPERR_)[A-Z_]+$", k):
            assert const[k if k.startswith("RS_") else "RS_" + k] == v, k
    rows = lambda d: ",\n".join(f"    {json.dumps(k)}: {json.dumps(v)}" for k, v in d.items())
    with open(os.path.join(ROOT, "tests", "golden", "abi_v4.json"), "w") as f:
        f.write('{\n  "functions": {\n' + rows(functions) + '\n  },\n  "structs": {\n' + rows(structs) + '\n  },\n  "constants": {\n'
                + rows(const) + "\n  }\n}\n")
    print(len(functions), "functions,", len(structs), "structs,", len(const), "constants")


if __name__ == "__main__":
    main(sys.argv[1])
