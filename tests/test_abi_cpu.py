"""The one place that holds the ctypes binding to include/radsearch.h, without a GPU.  radiation_ppo_amd/_lib.py reads the header at
import and derives every signature, struct and constant from it; here
  - the derived binding is held to tests/golden/abi_v4.json, the record of ABI version 4 taken from the last hand-written table
    (tests/golden/make_abi_v4.py): every recorded function, struct and constant must be there unchanged, new ones may be appended;
  - every struct's size and every field's offset and size are held to what the C compiler makes of the same header;
  - the header reader is fed one declaration of each form the header uses, and three it must refuse;
  - the built library loads without a GPU and exports every declared function."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = json.load(open(os.path.join(ROOT, "tests", "golden", "abi_v4.json")))
# the record's vocabulary; `int` and `i32` (`size` and an unsigned 64-bit) may be one ctypes type, so the words are compared through it
KINDS = {"i32": C.c_int32, "i64": C.c_int64, "u32": C.c_uint32, "int": C.c_int, "size": C.c_size_t, "f32": C.c_float, "f64": C.c_double,
         "cstr": C.c_char_p, "ptr": C.c_void_p, "pptr": C.POINTER(C.c_void_p), "void": None}


@pytest.fixture(scope="module")
def lib():
    from radiation_ppo_amd import build
    build.build(verbose=False)
    from radiation_ppo_amd import _lib
    return _lib.load()


def _kind(t):
    """a ctypes type of the binding -> its word of the record's vocabulary"""
    from radiation_ppo_amd import _lib
    for c_name, cls in _lib.STRUCTS.items():
        if t is C.POINTER(cls):
            return "ptr:" + c_name
    return next(k for k, v in KINDS.items() if v is t)


def _same(word):
    return word if word.startswith("ptr:") else _kind(KINDS[word])


def test_the_binding_reduces_to_the_record_of_abi_version_4():
    from radiation_ppo_amd import _lib
    bound = {name: (ret, args) for name, ret, args in _lib.SYMBOLS}
    assert len(bound) == len(_lib.SYMBOLS) and len(RECORD["functions"]) == 107 and len(RECORD["structs"]) == 11
    for name, rec in RECORD["functions"].items():
        assert name in bound, name
        assert _kind(bound[name][0]) == _same(rec["ret"]), name
        assert [_kind(t) for t in bound[name][1]] == [_same(k) for k in rec["args"]], name
    for c_name, rec in RECORD["structs"].items():
        cls = _lib.STRUCTS[c_name]
        assert cls is getattr(_lib, "".join(w.capitalize() for w in c_name.split("_")))            # rs_mlp_params -> _lib.RsMlpParams
        got = [[f, _kind(getattr(t, "_type_", t) if issubclass(t, C.Array) else t), t._length_ if issubclass(t, C.Array) else None]
               for f, t in cls._fields_]
        assert got == [[f, _same(k), n] for f, k, n in rec], c_name
    for name, value in RECORD["constants"].items():
        assert getattr(_lib, name) == value, name
    assert "rs_update_state" in _lib.STRUCTS                                                       # the mirror the table lacked


def _host_cc():
    from radiation_ppo_amd import build
    for cc in ("cc", "gcc", "clang"):
        if shutil.which(cc):
            return [shutil.which(cc)]
    try:
        return [build.hipcc(), "-x", "c"]
    except RuntimeError:
        return None


def test_struct_layouts_are_the_c_compiler_s(tmp_path):
    """sizeof of every struct, offsetof and size of every field: a host-only C program over the header against ctypes"""
    from radiation_ppo_amd import _lib
    cc = _host_cc()
    if cc is None:
        pytest.skip("no host C compiler found (cc, gcc, clang, hipcc)")
    lines = []
    for c_name, cls in _lib.STRUCTS.items():
        lines.append(f'    printf("{c_name} - %zu 0\\n", sizeof({c_name}));')
        lines += [f'    printf("{c_name} {f} %zu %zu\\n", offsetof({c_name}, {f}), sizeof((({c_name}*)0)->{f}));' for f, _ in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "radsearch.h"\nint main(void) {\n' + "\n".join(lines) + "\n    return 0;\n}\n")
    subprocess.run(cc + ["-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout
    seen = [tuple(line.split()) for line in out.splitlines()]
    want = []
    for c_name, cls in _lib.STRUCTS.items():
        want.append((c_name, "-", str(C.sizeof(cls)), "0"))
        want += [(c_name, f, str(getattr(cls, f).offset), str(getattr(cls, f).size)) for f, _ in cls._fields_]
    assert len(_lib.STRUCTS) == 12 and seen == want


FORMS = """
/* a comment with int rs_not_a_function(void); inside */
#ifndef GUARD_H
#define GUARD_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define RS_A 4      /* trailing comment */
#define RS_B (10 + RS_A)
typedef void* rs_stream_t;
typedef struct rs_handle rs_handle;
enum { RS_X = 0, RS_Y = 16 };
typedef struct rs_named {
    int32_t n;          // a line comment
    int32_t bbox[4];
    double last_stats[5];
} rs_named;
typedef struct { const float *w1, *b1; int32_t N, A, use_team_reward; double* w_count; double* w_mean; } rs_anonymous;
const char* rs_strerror(int code);
int rs_abi_version(void);
void rs_destroy(rs_handle* h);
size_t rs_bytes(const rs_named* cfg, void* workspace, size_t n, rs_stream_t stream,
                rs_handle** out);
int64_t rs_team(const float* const* weights, const rs_anonymous* p, float lr, double alpha, uint32_t seed, const uint8_t* mask, void** dev_ptr);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_the_reader_on_one_declaration_of_each_form():
    from radiation_ppo_amd import _lib
    functions, structs, enums, defines = _lib.parse_header(FORMS)
    assert defines == {"RS_A": 4, "RS_B": 14} and enums == {"RS_X": 0, "RS_Y": 16}
    assert structs == {"rs_handle": None,
                       "rs_named": [("int32_t", "n", None), ("int32_t", "bbox", 4), ("double", "last_stats", 5)],
                       "rs_anonymous": [("const float*", "w1", None), ("const float*", "b1", None), ("int32_t", "N", None), ("int32_t", "A", None),
                                        ("int32_t", "use_team_reward", None), ("double*", "w_count", None), ("double*", "w_mean", None)]}
    assert functions == {
        "rs_strerror": ("const char*", [("int", "code")]), "rs_abi_version": ("int", []), "rs_destroy": ("void", [("rs_handle*", "h")]),
        "rs_bytes": ("size_t", [("const rs_named*", "cfg"), ("void*", "workspace"), ("size_t", "n"), ("rs_stream_t", "stream"),
                                ("rs_handle**", "out")]),
        "rs_team": ("int64_t", [("const float**", "weights"), ("const rs_anonymous*", "p"), ("float", "lr"), ("double", "alpha"),
                                ("uint32_t", "seed"), ("const uint8_t*", "mask"), ("void**", "dev_ptr")])}
    assert list(functions) == ["rs_strerror", "rs_abi_version", "rs_destroy", "rs_bytes", "rs_team"]           # the header's order


def test_the_type_mapping():
    from radiation_ppo_amd import _lib
    classes = {"rs_handle": None, "rs_config": _lib.RsConfig}
    for t, want in (("int", C.c_int), ("int32_t", C.c_int32), ("int64_t", C.c_int64), ("uint32_t", C.c_uint32), ("size_t", C.c_size_t),
                    ("float", C.c_float), ("double", C.c_double), ("rs_stream_t", C.c_void_p), ("const char*", C.c_char_p),
                    ("const rs_config*", C.POINTER(_lib.RsConfig)), ("rs_handle**", C.POINTER(C.c_void_p)), ("void**", C.POINTER(C.c_void_p)),
                    ("const float**", C.POINTER(C.c_void_p)), ("rs_handle*", C.c_void_p), ("const float*", C.c_void_p), ("int32_t*", C.c_void_p),
                    ("uint32_t*", C.c_void_p), ("void*", C.c_void_p), ("const uint8_t*", C.c_void_p)):
        assert _lib._ctype(t, classes) is want, t
    with pytest.raises(ValueError, match="uint8_t"):
        _lib._ctype("uint8_t", classes)                                # a pointee only: no by-value type of the binding
    assert C.c_void_p.from_param(C.byref(C.c_int32())) is not None      # what the five out-parameters' call sites pass


@pytest.mark.parametrize("text,named", [
    ("int rs_f(const half* x);", "half"),                                              # an unknown type
    ("typedef struct { int32_t n; rs_later* p; } rs_s;", "rs_later"),
    ("int rs_f(int32_t n);\nint rs_g(int32_t n, float* x", "int rs_g(int32_t n, float* x"),   # an unterminated prototype
    ("#define RS_SQ(x) ((x) * (x))\nint rs_f(void);", "#define RS_SQ(x)"),               # a function-like macro
    ("#define RS_HALF 0.5", "0.5"), ("#define RS_N (4 + RS_M)", "RS_M"), ("#pragma once", "#pragma once"),
    ("enum { RS_P = 1, RS_Q };", "RS_Q"), ("int rs_f(int32_t);", "int32_t"), ("int rs_table[4];", "rs_table"),
    ("typedef int32_t rs_count;", "rs_count"), ("typedef void* rs_queue_t;", "rs_queue_t"),
    ("int rs_f(int32_t n, int (*cb)(int));", "cb")])
def test_the_reader_refuses_what_it_does_not_know_and_names_it(text, named):
    from radiation_ppo_amd import _lib
    with pytest.raises(ValueError, match=re.escape(named)):
        _lib.parse_header(text)


def test_header_symbols_exported(lib):
    from radiation_ppo_amd import _lib
    names = [s[0] for s in _lib.SYMBOLS]
    src = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    assert sorted(names) == sorted(set(re.findall(r"\b(rs_[a-z0-9_]+)\s*\(", src)))          # the reader dropped nothing
    assert "rs_step" in names and "rs_reset" in names and "rs_gae" in names and "rs_create" in names
    assert "rs_cnn_trunk_forward_grid" in names and "rs_cnn_trunk_slab_rows" in names        # the host-only grid queries of the CNN trunk
    for n in names:
        assert hasattr(lib, n), f"librs_hip.so does not export {n}"
        assert getattr(lib, n).argtypes is not None                                          # bound by _lib.load()
    assert lib.rs_abi_version() == _lib.RS_ABI_VERSION == 4


def test_a_missing_header_fails_like_a_missing_library(tmp_path):
    """a copy of the module without include/ beside its package: the import names the path it looked for"""
    import importlib.util
    os.mkdir(tmp_path / "pkg")
    shutil.copy(os.path.join(ROOT, "radiation_ppo_amd", "_lib.py"), tmp_path / "pkg" / "_lib.py")
    spec = importlib.util.spec_from_file_location("_lib_without_header", tmp_path / "pkg" / "_lib.py")
    with pytest.raises(RuntimeError, match=re.escape(str(tmp_path / "include" / "radsearch.h")) + " is missing"):
        spec.loader.exec_module(importlib.util.module_from_spec(spec))


def test_config_validation_and_errors(lib):
    from radiation_ppo_amd import _lib
    good = _lib.RsConfig(num_envs=4, num_agents=1, obstruction_count=0, enforce_grid_boundaries=1,
                         bbox=(0, 0, 2700, 2700), observation_area=(200, 500), falloff=0, geom_group_size=1,
                         seed=2, env_id_base=0)
    assert lib.rs_state_bytes(C.byref(good)) > 0
    for field, bad in (("num_envs", 0), ("num_agents", 9), ("obstruction_count", 8), ("obstruction_count", -2),
                       ("geom_group_size", 0)):
        cfg = _lib.RsConfig.from_buffer_copy(good)
        setattr(cfg, field, bad)
        assert lib.rs_state_bytes(C.byref(cfg)) == 0
    h = C.c_void_p()
    assert lib.rs_create(C.byref(good), None, 0, None, C.byref(h)) == _lib.RS_ERR_INVALID_ARG
    assert lib.rs_strerror(0) == b"ok" and b"workspace" in lib.rs_strerror(_lib.RS_ERR_WORKSPACE)
    assert lib.rs_step(None, None, None, None, None, None, None, None) == _lib.RS_ERR_INVALID_ARG


def test_product_does_not_import_oracle():
    """The oracle is test infrastructure: nothing under radiation_ppo_amd/ may import or execute it."""
    pkg = os.path.join(ROOT, "radiation_ppo_amd")
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h", ".cpp")):
                txt = open(os.path.join(d, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", txt, flags=re.M), (d, f)
                assert "oracle/" not in txt and "radsearch_oracle" not in txt, (d, f)


def test_env_requires_gpu_and_fails_loudly():
    import torch
    from radiation_ppo_amd.envs import RadSearchVec
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError):
        RadSearchVec(4, device="cpu")
