"""The C-ABI shared library loads on a CPU-only box and exports every symbol include/phendiff_hip.h declares
(no compute calls here: there is no GPU).  Also holds the binding that phendiff_amd/_lib.py derives from the header against what a C
compiler makes of the same header: every struct, every field, offsets, sizes and type classes."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from abi_header import HEADER, declared_functions, define, header_fields, source, struct_names


def test_library_exports_every_declared_symbol():
    import phendiff_amd._lib as L
    assert os.path.exists(L.LIB_PATH), "build the library first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = L.lib()
    names = declared_functions()
    assert len(names) >= 18
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/phendiff_hip.h but not exported"
        assert n in L.SYMBOLS, f"{n} has no ctypes prototype in phendiff_amd/_lib.py"
    assert sorted(L.SYMBOLS) == names
    # one version number in three places: the header's macro, the binding's constant, the library's answer (bumped whenever an
    # args struct grows or an entry point is added: r2 added trailing pointer fields, r3 = 3)
    assert lib.pd_abi_version() == L.ABI_VERSION == define("PD_ABI_VERSION")
    assert lib.pd_last_error() is not None


def class_of(cname):
    """The binding's class of a C struct, by the naming rule: pd_foo_bar_args -> FooBarArgs."""
    import phendiff_amd._lib as L
    return getattr(L, "".join(w.capitalize() for w in cname[3:].split("_")))


def host_c_compiler():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for cc in (shutil.which("cc"), os.path.join(rocm, "llvm", "bin", "clang"), os.path.join(rocm, "lib", "llvm", "bin", "clang")):
        if cc and os.path.exists(cc):
            return cc
    pytest.fail("no host C compiler (cc, or ROCm's clang): the library's build needs one too")


PROBE = """#include <stdio.h>
#include "phendiff_hip.h"
#define KIND(x) _Generic((x), int: "int", float: "float", double: "double", long: "long", long long: "longlong", \\
                         unsigned long: "ulong", default: "other")
#define FIELD(T, f) printf("F %s %zu %zu %s\\n", #f, offsetof(T, f), sizeof(((T*)0)->f), KIND(((T*)0)->f))
int main(void) {
@BODY@  return 0;
}
"""


def compiled_layout(tmp_path):
    """{struct: (sizeof, [(field, offset, size, kind)])} as the host C compiler lays the header's structs out."""
    lines = "".join(f'  printf("S {s} %zu\\n", sizeof({s}));\n' + "".join(f"  FIELD({s}, {f});\n" for f in header_fields(s))
                    for s in struct_names())
    (tmp_path / "layout.c").write_text(PROBE.replace("@BODY@", lines))
    exe = str(tmp_path / "layout")
    subprocess.run([host_c_compiler(), "-std=c11", "-I", os.path.dirname(HEADER), "-o", exe, str(tmp_path / "layout.c")], check=True)
    layout = {}
    for tag, name, *rest in (line.split() for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()):
        if tag == "S":
            fields = []
            layout[name] = (int(rest[0]), fields)
        else:
            fields.append((name, int(rest[0]), int(rest[1]), rest[2]))
    return layout


def same_type(ctype, kind, size):
    """Is a ctypes field type what C calls `kind` (a _Generic class) of `size` bytes?"""
    if kind in ("float", "double"):
        return ctype is {"float": C.c_float, "double": C.c_double}[kind]
    if kind == "other":     # a pointer or char[N]
        return ctype is C.c_void_p and size == C.sizeof(C.c_void_p) or issubclass(ctype, C.Array) and ctype._type_ is C.c_char and ctype._length_ == size
    codes = "BHILQ" if kind == "ulong" else "bhilq"      # integers: signedness and width
    return issubclass(ctype, C._SimpleCData) and ctype._type_ in codes and C.sizeof(ctype) == size


def test_struct_field_order_matches_header(tmp_path):
    """Every struct of the header, as the compiler lays it out, against the derived ctypes class: field names and order, every offset
    and size, float / double exactly where C has them, integers by signedness and width, c_void_p for pointers, sizeof."""
    import phendiff_amd._lib as L
    layout = compiled_layout(tmp_path)
    assert list(layout) == struct_names() and len(layout) >= 62
    nfields = 0
    for cname, (size, fields) in layout.items():
        cls = class_of(cname)
        assert L.STRUCTS[cname] is cls and issubclass(cls, C.Structure)
        assert [f[0] for f in fields] == [f[0] for f in cls._fields_] == header_fields(cname), cname
        for (name, offset, fsize, kind), (_, ctype) in zip(fields, cls._fields_):
            where = f"{cname}.{name}"
            assert (getattr(cls, name).offset, getattr(cls, name).size) == (offset, fsize), where
            assert same_type(ctype, kind, fsize), (where, kind, ctype)
            nfields += 1
        assert C.sizeof(cls) == size, cname
    assert nfields >= 840
    # the three classes whose long-standing names the rule does not give
    assert (L.AdamWEmaArgs, L.LayerNormArgs, L.LayerNormBwdArgs) == (class_of("pd_adamw_ema_args"), class_of("pd_layernorm_args"),
                                                                    class_of("pd_layernorm_bwd_args"))
    assert not same_type(C.c_int, "float", 4) and not same_type(C.c_int, "long", 8) and not same_type(C.c_int64, "ulong", 8)


def test_prototypes_match_header():
    import re
    import phendiff_amd._lib as L
    src = re.sub(r"/\*.*?\*/", "", source(), flags=re.S)
    nstruct = 0
    for fn, params in re.findall(r"\b(pd_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src):
        restype, argtypes = L.SYMBOLS[fn]
        params = [] if params.strip() == "void" else params.split(",")
        assert len(argtypes) == len(params), fn
        for p, t in zip(params, argtypes):
            m = re.fullmatch(r"\s*(?:const\s+)?(pd_\w+)\s*\*\s*\w+\s*", p)
            if m:
                assert t is C.POINTER(class_of(m.group(1))), (fn, p)
                nstruct += 1
    assert nstruct >= 69      # struct-pointer parameters of the 89 prototypes of ABI 8
    # scalars the host receives through byref(); device pointers passed as integers stay c_void_p
    assert L.SYMBOLS["pd_event_elapsed_ms"] == (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_float)])
    assert L.SYMBOLS["pd_comm_query"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)])
    assert L.SYMBOLS["pd_grad_norm"][1] == [C.c_void_p, C.c_int64, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    assert L.SYMBOLS["pd_allreduce_bucket"][1] == [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
    assert L.SYMBOLS["pd_lp_guidance_scaled"][1][1:] == L.SYMBOLS["pd_ddim_raw_x0"][1][1:] == [C.c_void_p, C.c_void_p]
    assert L.SYMBOLS["pd_last_error"] == (C.c_char_p, []) and L.SYMBOLS["pd_graph_end"][1] == [C.c_void_p, C.POINTER(C.c_void_p)]
    assert L.SYMBOLS["pd_conv_wgrad_workspace"] == (C.c_size_t, [C.POINTER(L.WgradArgs)])


def test_the_reader_refuses_what_it_does_not_know(tmp_path):
    """Nothing is guessed: an unmapped type names its struct and field, a stale out-parameter is an error, a missing header names its path."""
    import phendiff_amd._lib as L
    from phendiff_amd import _abi
    ok = "typedef struct { int n; const float *a, *b; char tag[16]; } pd_toy_args;\nint pd_toy(const pd_toy_args* a, void* stream);\n"
    structs, symbols, _ = _abi.read(ok, {})
    assert structs["pd_toy_args"]._fields_ == [("n", C.c_int), ("a", C.c_void_p), ("b", C.c_void_p), ("tag", C.c_char * 16)]
    assert symbols == {"pd_toy": (C.c_int, [C.POINTER(structs["pd_toy_args"]), C.c_void_p])}
    with pytest.raises(TypeError, match=r"pd_toy_args\.flag.*'short'"):
        _abi.read(ok.replace("int n;", "int n; short flag;"), {})
    with pytest.raises(TypeError, match="pd_toy.*'unsigned'"):
        _abi.read(ok.replace("void* stream", "unsigned flags"), {})
    with pytest.raises(TypeError, match="pd_toy.*'float'"):
        _abi.read(ok.replace("int pd_toy", "float pd_toy"), {})
    with pytest.raises(TypeError, match="pd_gone"):
        _abi.read(ok, {("pd_gone", "out"): C.POINTER(C.c_int)})
    with pytest.raises(TypeError, match="explicit integer value"):
        _abi.read(ok + "enum { PD_A = 0, PD_B };\n", {})
    missing = str(tmp_path / "phendiff_hip.h")
    with pytest.raises(L.PhenDiffHipError, match=missing):
        L.read_header(missing)


def test_argument_validation_without_gpu():
    """Entry points validate before launching: bad arguments return an error code and a message, no device needed."""
    import phendiff_amd._lib as L
    lib = L.lib()
    a = L.ConvArgs(dtype=7)
    assert lib.pd_conv(C.byref(a), None) == -1 and b"dtype" in lib.pd_last_error()
    a = L.ConvArgs(dtype=1, B=1, Hin=8, Win=8, Hout=8, Wout=8, C0=48, Cout=64, Cout_pad=64, ksize=3, stride=1, pad=1)
    assert lib.pd_conv(C.byref(a), None) == -2 and b"multiples of 32" in lib.pd_last_error()
    assert lib.pd_attn_d8(C.byref(L.AttnArgs(dtype=1, B=0)), None) == -2
    assert lib.pd_ddim_step(C.byref(L.DdimStepArgs(numel=0)), None) == -1
    # per_sample < 1 or no divisor of numel (the kernel divides by it): refused like its siblings, before the pointers are looked at
    for per_sample in (0, -8, 3):
        assert lib.pd_ddim_step(C.byref(L.DdimStepArgs(numel=8, per_sample=per_sample, pred_type=2)), None) == L.CONSTANTS["PD_ERR_ARG"]
        assert b"per_sample" in lib.pd_last_error() and lib.pd_last_error().startswith(b"pd_ddim_step:")
    # every tensor of pd_ddim_step goes through 16-byte loads / stores: each of the five pointers in turn at 16k + 4, the others
    # aligned, is refused before any launch (the addresses are never dereferenced)
    base = dict(sample=0x10000, model_out=0x20000, uncond_out=0x30000, prev_sample=0x40000, pred_x0=0x50000)
    for name in base:
        p = dict(base, **{name: base[name] + 4})
        assert lib.pd_ddim_step(C.byref(L.DdimStepArgs(numel=8, per_sample=8, pred_type=2, w=0x60000, **p)), None) == -1, name
        assert b"16-byte aligned" in lib.pd_last_error(), name
    assert lib.pd_conv_stat_tiles(256, 256, 3, 1) == 256 and lib.pd_conv_stat_tiles(64, 64, 3, 2) == 32
    assert lib.pd_attn_wide(C.byref(L.AttnWideArgs(dtype=1, B=1, heads=1, D=512, Nq=0, Nkv=4)), None) == -2
    assert lib.pd_attn_d64_bwd(C.byref(L.AttnD64BwdArgs(dtype=1, B=1, heads=1, Nq=4, Nkv=4)), None) == -1
    assert lib.pd_attn_wide_bwd(C.byref(L.AttnWideBwdArgs(dtype=1, B=1, heads=1, D=512, Nq=4, Nkv=4)), None) == -1
    assert lib.pd_allreduce_bucket(None, None, 16, 1, 1, None) == -1 and b"communicator" in lib.pd_last_error()
    assert lib.pd_comm_init(None, 0, 1, None) == -1 and lib.pd_comm_destroy(None) == 0
    assert lib.pd_layernorm_bwd(C.byref(L.LayerNormBwdArgs(dtype=1, rows=4, C=12)), None) == -1
    assert lib.pd_layernorm_bwd_blocks(10) == 3 and lib.pd_layernorm_bwd_blocks(1 << 20) == 2048
    with pytest.raises(L.PhenDiffHipError):
        L.check(-1, "x")
