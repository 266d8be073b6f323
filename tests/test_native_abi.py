"""The kernel library's C ABI is written once, in csrc/kernels/sl_api.h: the parser that turns it
into ctypes signatures (ops/_native.py), the build's export check (build.py) and the compiler's
own check of a definition against its declaration.  None of this needs a GPU."""
import ctypes
import glob
import os
import re
import shutil
import subprocess

import pytest

from serverless_learn_amd import build
from serverless_learn_amd.ops import _native

P, I, U, L, F, D = (ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_long, ctypes.c_float, ctypes.c_double)
LL, ULL = ctypes.c_longlong, ctypes.c_ulonglong


def _header(*decls: str) -> str:
    return '#pragma once\nnamespace sl { struct S; }\nextern "C" {\n' + "\n".join(decls) + '\n}  // extern "C"\n'


# ---- 1. parser vocabulary ----
def test_every_type_of_the_vocabulary_maps_to_its_ctype():
    api = _native.parse_api(_header(
        "int f_scalars(int a, unsigned b, long c, long long d, unsigned long long e, float f, double g);",
        "long f_pointers(const float* a, uint16_t* b, char* const* c, void** d, const sl::S* e, hipStream_t s);",
        "void f_void(int a);",
        "hipStream_t f_stream(hipStream_t main);",
        "void* f_ptr(const void *p);",
    ))
    assert api == {
        "f_scalars": (I, [I, U, L, LL, ULL, F, D]),
        "f_pointers": (L, [P, P, P, P, P, P]),
        "f_void": (None, [I]),
        "f_stream": (P, [P]),
        "f_ptr": (P, [P]),
    }


def test_const_names_comments_and_line_breaks_are_ignored():
    api = _native.parse_api(_header(
        "// int commented_out(int a);",
        "/* int also_commented_out(int a);",
        "   over two lines */",
        "int f(const int n,  // the count",
        "      const unsigned long long",
        "          seed, /* inline */ float,",
        "      long long);",
    ))
    assert api == {"f": (I, [I, ULL, F, LL])}


def test_void_and_empty_parameter_lists_take_no_arguments():
    api = _native.parse_api(_header("int f();", "long g(void);", "int h( );"))
    assert api == {"f": (I, []), "g": (L, []), "h": (I, [])}


@pytest.mark.parametrize("decl, quoted", [
    ("int f(size_t n);", "size_t n"),                       # a type outside the vocabulary
    ("int f(int a, struct WtDesc d);", "struct WtDesc d"),  # a struct by value
    ("size_t f(int a);", "size_t"),                         # ... as the return type
    ("int f(unsigned int a);", "unsigned int a"),           # the vocabulary is closed: it is spelled `unsigned`
    ("int f(int a, ...);", "..."),                          # variadic
    ("int f(int a = 0);", "int a = 0"),                     # a default argument
    ("int f(int (*cb)(int));", "int f(int (*cb)(int))"),    # a function pointer
    ("int f(int a)", "int f(int a)"),                       # no ';'
    ("int f(int a)\nint g(int b);", "int f(int a) int g(int b)"),  # no ';' between two declarations
    ("int f(SOME_PARAMS);", "SOME_PARAMS"),                 # a macro for the parameter list
    ("#define X 1;", "#define X 1"),                        # anything else in the block
    ("int f(int a); int f(long a);", "declared twice: f"),
])
def test_what_the_parser_does_not_understand_raises_and_is_quoted(decl, quoted):
    with pytest.raises(ValueError) as e:
        _native.parse_api(_header("int ok(int a);", decl))
    assert quoted in str(e.value)


def test_a_header_without_the_block_raises():
    with pytest.raises(ValueError):
        _native.parse_api("int f(int a);\n")


# ---- 2. pinned signatures: guards the parser against the real header, not the ABI ----
_ROWS = [P, P, P, I, I, P, P, P, P, P, P, F, F, F, F, P, P, P, P, P, P, P, I, P, P, P]
PINNED = {
    "sl_mlp_rows": _ROWS,
    "sl_mlp_rows_xt": _ROWS,
    "sl_mlp_opt": [I, P, P, P, P, I, L, P, F, F, F, F, F, P, P, P, P, P, P, P, P, P, P, I, F, F, F, F, F, F, F, P],
    "sl_conv_fwd": [P, I, I, I, I, P, I, I, I, I, I, I, I, P, I, P, P, P, P],
    "sl_softmax_ce_wide": [P, P, P, P, P, I, P, I, I, F, P, F, I, P, L, P],
    "sl_gossip_scatter": [P, P, P, P, L, L, D, I, P],
    "sl_input_aug": [P, P, P, I, I, I, I, I, I, ULL, P, P, P, F, F, F, F, F, F, P],
    "sl_xgmi_alloc": [L, P],
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_pinned_signature(name):
    assert _native._SIGS[name] == PINNED[name]
    assert _native._RESTYPE[name] is I


def test_return_types_come_from_the_header():
    for name in ("sl_mlp_param_count", "sl_mlp_slab_stride", "sl_mlp_x_tile_bytes", "sl_conv_wgrad_ws_need",
                 "sl_rsum_floats", "sl_gossip_topk_workspace", "sl_xgmi_buffer_bytes"):
        assert _native._RESTYPE[name] is L, name
    assert _native._RESTYPE["sl_conv_note_kernel"] is None
    assert _native._RESTYPE["sl_wgrad_reduce_stream"] is P
    assert set(_native._RESTYPE) == set(_native._SIGS) == build.api_names()


# ---- 4. export parity ----
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists(os.path.join(build.ROCM, "bin", "hipcc")),
                    reason="needs hipcc")
@pytest.mark.parametrize("deterministic", [False, True])
def test_the_library_exports_exactly_what_the_header_declares(deterministic):
    so = build.build_kernels(deterministic=deterministic)
    assert build.exported_names(so) == set(_native._SIGS)
    build._check_exports(so)


def test_the_build_refuses_exports_that_differ_from_the_header():
    names = build.api_names()
    assert "sl_accum_flat" in names
    build._check_exports("fake.so", set(names))
    with pytest.raises(RuntimeError) as e:
        build._check_exports("fake.so", names - {"sl_accum_flat"} | {"sl_added_without_a_declaration"})
    msg = str(e.value)
    assert "exported but not declared: sl_added_without_a_declaration" in msg
    assert "declared but not exported: sl_accum_flat" in msg


# ---- 5. the compiler is the enforcer ----
_CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")


@pytest.mark.skipif(_CXX is None, reason="needs a host C++ compiler")
def test_a_definition_that_disagrees_with_the_header_does_not_compile(tmp_path):
    def compiles(n_type):
        tu = tmp_path / ("accum_%s.cpp" % n_type)
        tu.write_text('#include "sl_api.h"\nextern "C" int sl_accum_flat(float* dst, const float* src, %s n, int add, '
                      "hipStream_t stream) { return 0; }\n" % n_type)
        return subprocess.run([_CXX, "-fsyntax-only", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + build.KERNEL_DIR,
                               "-I" + os.path.join(build.ROCM, "include"), str(tu)],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)

    good = compiles("long")
    assert good.returncode == 0, good.stdout
    bad = compiles("int")
    assert bad.returncode != 0
    assert "sl_accum_flat" in bad.stdout


# ---- 6. no stragglers ----
def test_no_signature_is_written_anywhere_else():
    pkg = os.path.join(build.ROOT, "serverless_learn_amd")
    for path in glob.glob(os.path.join(pkg, "**", "*.py"), recursive=True):
        with open(path) as f:
            assert not re.search(r"\b(N|_native)\.register\(", f.read()), path
    assert not hasattr(_native, "register")
    # a declaration without a body: `TYPE sl_name(...);` at the start of a statement
    decl = re.compile(r'^\s*(?:extern\s+"C"\s+)?(?:int|long|void|hipStream_t)\s+(sl_\w+)\s*\([^(){};]*\)\s*;', re.M)
    for path in glob.glob(os.path.join(build.KERNEL_DIR, "*.h*")):
        if os.path.basename(path) == "sl_api.h":
            continue
        with open(path) as f:
            assert decl.findall(f.read()) == [], path
