"""The C-ABI library loads without a GPU and exports exactly what include/probnmn_hip.h declares; the binding that
probnmn._hip derives from that header -- argument lists, return types, record layouts, constants -- is what the C / C++
compiler makes of the same header, and a declaration the reader cannot take fails loudly."""
import ctypes
import os
import re
import subprocess
import tempfile

import pytest

from probnmn import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "probnmn_hip.h")


def declared_functions():
    text = open(HEADER).read()
    return sorted(set(re.findall(r"^(?:int|int64_t)\s+(pnmn_\w+)\s*\(", text, flags=re.M)))


def test_library_exports_every_declared_symbol():
    names = declared_functions()
    assert len(names) >= 18
    assert sorted(_hip.SIGNATURES) == names  # binding table and header agree
    handle = _hip.lib()
    for n in names:
        assert hasattr(handle, n), n
    assert handle.pnmn_abi_version() == _hip.ABI_VERSION == 14


def test_launch_trace_without_launches_is_empty():
    """pnmn_launch_trace_begin / _end around nothing: zero entries, no device needed; a second _end is harmless."""
    handle = _hip.lib()
    import numpy as np
    out, n = np.zeros(4, _hip.LAUNCH_TIMING), np.full(1, -1, np.int32)
    assert handle.pnmn_launch_trace_begin() == 0
    assert handle.pnmn_launch_trace_end(out.ctypes.data, 4, n.ctypes.data) == 0 and n[0] == 0
    assert handle.pnmn_launch_trace_end(out.ctypes.data, 4, n.ctypes.data) == 0 and n[0] == 0
    assert handle.pnmn_launch_trace_end(0, 0, 0) == _hip.EINVAL


# sizeof of every record, pinned: a layout change is an ABI change and is made here too, on purpose
RECORD_BYTES = {
    "pnmn_launch": 64,
    "pnmn_launch_timing": 64,
    "pnmn_conv2d_desc": 96,
    "pnmn_conv_item": 96,
    "pnmn_wgrad_item": 48,
    "pnmn_wgrad_job": 24,
    "pnmn_wtrans_item": 32,
    "pnmn_dot1_item": 64,
    "pnmn_same_item": 80,
    "pnmn_minmax_item": 64,
    "pnmn_maskbwd_item": 40,
    "pnmn_axpy_item": 24,
    "pnmn_adam_item": 48,
    "pnmn_derive_job": 40,
    "pnmn_plan_in": 216,
    "pnmn_decoder_fwd_job": 184,
    "pnmn_decoder_bwd_job": 136,
    "pnmn_trunk_config": 88,
    "pnmn_trunk_io": 256,
    "pnmn_gemm_desc": 120,
    "pnmn_token_seg": 32,
    "pnmn_lstm_stack_job": 104,
    "pnmn_lstm_dropout_desc": 32,
}


def test_record_layouts_match_c_structs():
    """Compile a tiny C program against the header and compare sizeof/offsetof with numpy."""
    assert sorted(_hip.ITEM_SIZES) == sorted(RECORD_BYTES)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "probnmn_hip.h"', "int main(){"]
    for cname, (dtype, size) in _hip.ITEM_SIZES.items():
        lines.append('printf("%s %%zu", sizeof(%s));' % (cname, cname))
        for field in dtype.names:
            cfield = {"in": "in"}.get(field, field)
            lines.append('printf(" %s=%%zu", offsetof(%s, %s));' % (field, cname, cfield))
        lines.append('printf("\\n");')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write("\n".join(lines))
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.check_output([exe]).decode().strip().splitlines()
    seen = {}
    for line in out:
        parts = line.split()
        seen[parts[0]] = (int(parts[1]), {p.split("=")[0]: int(p.split("=")[1]) for p in parts[2:]})
    for cname, (dtype, size) in _hip.ITEM_SIZES.items():
        csize, offsets = seen[cname]
        assert csize == size == dtype.itemsize, cname
        assert csize == RECORD_BYTES[cname], cname
        for field in dtype.names:
            assert dtype.fields[field][1] == offsets[field], (cname, field)


SIGNATURE_PROGRAM = r"""
#include <cstdio>
#include <type_traits>
#include "probnmn_hip.h"
template <class T> void kind() {
    std::printf(" %s%zu", std::is_pointer<T>::value ? "pointer" : std::is_floating_point<T>::value ? "float"
                          : std::is_signed<T>::value ? "signed" : "unsigned", sizeof(T));
}
template <class F> struct Sig;
template <class R, class... A> struct Sig<R(A...)> {
    static void print(const char* name) {
        std::printf("%s", name);
        kind<R>();
        int each[] = {0, (kind<A>(), 0)...};
        (void)each;
        std::printf("\n");
    }
};
int main() {
@CALLS@
    return 0;
}
"""
C_KINDS = {ctypes.c_void_p: "pointer8", ctypes.c_int: "signed4", ctypes.c_int64: "signed8", ctypes.c_uint64: "unsigned8",
           ctypes.c_uint32: "unsigned4", ctypes.c_float: "float4", ctypes.c_double: "float8"}


def test_argument_lists_match_the_compiler():
    """What the C++ compiler makes of every prototype -- kind (pointer / signed / unsigned / float) and size of the return
    type and of each parameter, through decltype, nothing linked -- against the ctypes the binding sets on the library."""
    names = declared_functions()
    calls = "\n".join('    Sig<decltype(%s)>::print("%s");' % (n, n) for n in names)
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "sig.cpp"), os.path.join(d, "sig")
        open(src, "w").write(SIGNATURE_PROGRAM.replace("@CALLS@", calls))
        subprocess.check_call(["g++", "-std=c++11", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        seen = {line.split()[0]: line.split()[1:] for line in subprocess.check_output([exe]).decode().splitlines()}
    assert sorted(seen) == names == sorted(_hip.SIGNATURES)
    handle = _hip.lib()
    for name, argtypes in _hip.SIGNATURES.items():
        fn = getattr(handle, name)
        assert tuple(fn.argtypes) == tuple(argtypes), name  # what a call goes through is what the table says
        assert [C_KINDS[fn.restype]] + [C_KINDS[t] for t in argtypes] == seen[name], name


@pytest.mark.parametrize("text, naming", [
    ("int pnmn_f(const float* x, size_t n, void* stream);", "size_t n"),                       # parameter type not in the map
    ("typedef struct pnmn_r { float* x; int16_t n; } pnmn_r;", "int16_t n"),                   # field type not in the map
    ("typedef struct pnmn_r { int32_t p[PNMN_UNDEFINED]; } pnmn_r;", "PNMN_UNDEFINED"),        # array length: no such macro
    ("extern int\npnmn_f(int n);", "pnmn_f"),                                                 # split: no return type at a line's start
    ("int pnmn_g(unsigned int n);", "unsigned int n"),                                         # a type of two words
    ("int pnmn_f(int n,\n#ifdef X\n    int m,\n#endif\n    void* stream);", "#ifdef X"),        # conditional parameter
    ("int pnmn_ok(void);\nint pnmn_f(int (*callback)(int), void* stream);", "pnmn_f"),       # nested parentheses
    ("#define PNMN_WIDTH (4 * 32)", "PNMN_WIDTH"),                                             # not a plain integer
    ("typedef union { float f; int32_t i; } pnmn_u;", "typedef union"),                        # not a struct
])
def test_header_reader_fails_loudly(text, naming):
    with pytest.raises(_hip.HipLibraryError) as e:
        _hip.read_header(text=text)
    assert naming in str(e.value)


def test_header_reader_takes_the_conventions_and_names_a_missing_header(tmp_path):
    sigs, restypes, records, constants = _hip.read_header(text="""
        #define PNMN_N 3   /* a comment */
        #define PNMN_E (-7)
        typedef struct { const float *a, *b; int32_t n, p[PNMN_N]; double d; } pnmn_r;   // anonymous
int64_t pnmn_f(const pnmn_r* r /* HOST */, int n, uint32_t u, float x,
               void* stream);
int pnmn_g(void);
    """)
    assert sigs == {"pnmn_f": (ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_float, ctypes.c_void_p), "pnmn_g": ()}
    assert restypes == {"pnmn_f": ctypes.c_int64, "pnmn_g": ctypes.c_int}
    assert constants == {"PNMN_N": 3, "PNMN_E": -7}
    r = records["pnmn_r"]
    assert r.names == ("a", "b", "n", "p", "d") and r.itemsize == 40 and r.fields["p"][0].shape == (3,)
    assert [r.fields[f][1] for f in r.names] == [0, 8, 16, 20, 32]
    missing = str(tmp_path / "absent" / "probnmn_hip.h")
    with pytest.raises(_hip.HipLibraryError) as e:
        _hip.read_header(missing)
    assert missing in str(e.value)


def test_constants_are_the_headers_defines():
    text = open(HEADER).read()
    defines = {k: int(v) for k, v in re.findall(r"^#define\s+PNMN_(\w+)\s+\(?(-?\d+)\)?", text, flags=re.M)}
    ops = {k: v for k, v in defines.items() if k.startswith("OP_")}
    assert len(ops) == 17 and sorted(ops.values()) == list(range(0, 16 + 1))  # seventeen distinct launch ops, 0 .. 16
    names = list(ops) + ["CONV_ACCUMULATE", "CONV_ATOMIC", "CONV_MASKBWD", "CONV_DATTN", "GEMM_MAX", "EINVAL", "ESHAPE", "EAGAIN",
                         "CHANNELS", "LSTM_STACK_JOBS", "ABI_VERSION", "BEAM_MAX_STATES", "BEAM_MAX_CLASSES"]
    for name in names:
        assert getattr(_hip, name) == defines[name], name
    assert (_hip.GEMM_A_T, _hip.GEMM_B_T, _hip.GEMM_ACC) == (defines["GEMM_A_TRANSPOSED"], defines["GEMM_B_TRANSPOSED"],
                                                             defines["GEMM_ACCUMULATE"])
    assert (_hip.EINVAL, _hip.ESHAPE, _hip.EAGAIN) == (-1, -2, -3) and _hip.CHANNELS == 128
    from probnmn.runtime import program_compiler as pc
    assert (pc.MAX_AUTOMATON_STATES, pc.MAX_AUTOMATON_CLASSES) == (defines["BEAM_MAX_STATES"], defines["BEAM_MAX_CLASSES"])


def test_missing_library_fails_loudly(monkeypatch):
    monkeypatch.setattr(_hip, "_lib", None)
    monkeypatch.setattr(_hip, "LIB_PATH", "/nonexistent/libprobnmn_hip.so")
    try:
        _hip.lib()
    except _hip.HipLibraryError as e:
        assert "no" in str(e) and "fallback" in str(e)
    else:
        raise AssertionError("expected HipLibraryError")
