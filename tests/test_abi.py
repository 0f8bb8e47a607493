"""CPU checks of the drop-in boundary: the C-ABI library builds, loads, and exports exactly the
symbols include/memehip.h declares; the Python binding covers all of them; and the product refuses
to run without a HIP device (no CPU fallback).  No compute calls here."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "memehip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mh_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from multimodal_propaganda_meme_classification_amd import _lib
    return _lib


def test_header_symbols_exported(lib):
    names = _declared()
    assert len(names) >= 20
    for path in (lib.LIB_PATH, lib.LIB_PATH_F16):           # the bf16 and the fp16 build export the same ABI
        cdll = ctypes.CDLL(path)
        for n in names:
            assert hasattr(cdll, n), f"{n} declared in include/memehip.h but not exported by {path}"


def test_binding_covers_header(lib):
    assert sorted(lib.EXPORTED_SYMBOLS) == _declared()
    handle = lib.load()
    assert handle.mh_version().startswith(b"memehip") and b"bf16" in handle.mh_version()
    assert b"fp16" in lib.load("fp16").mh_version()
    assert b"shape" in handle.mh_status_str(2)


def test_struct_layout_matches_header(lib):
    # 8 pointers + 7 int32 + float + pointer + float + uint32 + 2 pointers + 2 int32 = 136 bytes; a drift here would corrupt every
    # grouped launch
    assert ctypes.sizeof(lib.MhGemmProblem) == 136
    assert ctypes.sizeof(lib.MhColsumJob) == 24
    assert ctypes.sizeof(lib.MhAttnProblem) == 104
    assert ctypes.sizeof(lib.MhLnFwdJob) == 72 and ctypes.sizeof(lib.MhLnBwdJob) == 112
    assert ctypes.sizeof(lib.MhHeadParams) == 64 == ctypes.sizeof(lib.MhHeadGrads)


def test_no_cpu_fallback(lib):
    from multimodal_propaganda_meme_classification_amd import ops
    x = torch.zeros((128, 64), dtype=torch.bfloat16)
    w = torch.zeros((128, 64), dtype=torch.bfloat16)
    with pytest.raises(lib.MemehipError):
        ops.linear_fwd(x, w)
    with pytest.raises(lib.MemehipError):
        ops.layernorm_fwd(x, torch.ones(64), torch.zeros(64), 1e-6)


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, "multimodal_propaganda_meme_classification_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f
                assert "from .. import oracle" not in src and "import oracle" not in src, f


def test_ctypes_structs_match_the_c_compiler(tmp_path):
    """Every struct the binding read from include/memehip.h against gcc: its size and the offset of every field.  A field read with
    the wrong type, or lost, shifts the second element of a job array and fails far from its cause."""
    import subprocess
    from multimodal_propaganda_meme_classification_amd import _lib as lib
    structs = {n: v for n, v in vars(lib).items() if isinstance(v, type) and issubclass(v, ctypes.Structure)}
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "memehip.h")).read(), flags=re.S)
    assert len(structs) == len(re.findall(r"\btypedef\s+struct\b", header)) >= 17      # counted without the reader: none was lost
    src = tmp_path / "sz.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "memehip.h"\nint main(void){' +
                   "".join(f'printf("{n} %zu\\n", sizeof({n}));' +
                           "".join(f'printf("{n}.{f} %zu\\n", offsetof({n}, {f}));' for f, _ in t._fields_) for n, t in structs.items()) +
                   "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    want = {k: int(v) for k, v in (line.split() for line in out.strip().splitlines())}
    got = {n: ctypes.sizeof(t) for n, t in structs.items()}
    got.update({f"{n}.{f}": getattr(t, f).offset for n, t in structs.items() for f, _ in t._fields_})
    assert len(got) > 150 and got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}


def test_reader_types_against_hand_spelled_lists(lib):
    """What the binding read from the header for the declarations that are easiest to get wrong, spelled out by hand here."""
    P, I, I64, F, U32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_uint32
    handle = lib.load()
    want = {
        "mh_adam_step": (I, [P] * 5 + [I64, I64, P, I, P, F, F, P, I, P]),                      # int64_t among ints
        "mh_attn_decode_beams": (I, [P, I, P, P, I64, I, P, I, P, I, P, I, P, I, I, I, I, P, I, P]),   # int64_t ld_b; ..., src, ld_src, stream
        "mh_beam_step": (I, [P, I, I, I, I, ctypes.POINTER(lib.MhBeamState), I, I, F, I, I64, P]),
        "mh_image_resample_u8": (I, [P] * 5 + [I] + [P] * 2 + [I] + [P] * 4 + [I] * 5 + [P]),
        "mh_image_normalize_u8": (I, [P, P, I, I, I, P, P, P]),
        "mh_bert_embed_bwd": (I, [P] * 5 + [I, I, I, I, I64, F, P, P, P, P]),
        "mh_dropout_apply": (I, [P, I64, P, F, U32, P]),
        "mh_mca3_bwd": (I, [P] * 15 + [I, I, P]),
        "mh_rows_gather": (I, [ctypes.POINTER(lib.MhRowsJob), I, P]),
        "mh_version": (ctypes.c_char_p, []),
        "mh_status_str": (ctypes.c_char_p, [I]),
        "mh_bn2d_workspace_elems": (I64, [I, I]),
        "mh_dwconv_wgrad_workspace_elems": (I64, [I] * 5),
    }
    for name, (restype, argtypes) in want.items():
        fn = getattr(handle, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert {n for n in lib.EXPORTED_SYMBOLS if getattr(handle, n).restype is not I} == {n for n, (r, _) in want.items() if r is not I}
    # arrays sized by a constant
    assert lib.MH_ADAM_MAX_GROUPS == 8
    assert lib.MhAdamSkipGroups._fields_ == [("hyper", P * 8), ("beta1", ctypes.c_double * 8), ("beta2", ctypes.c_double * 8),
                                             ("n", ctypes.c_int32), ("reserved_", ctypes.c_int32)]
    # a struct by value inside another
    assert lib.MhConvWgradProblem._fields_ == [("dy", P), ("x", P), ("slabs", P), ("ksplit", ctypes.c_int32), ("alpha", F),
                                               ("geom", lib.MhConvGeom)]
    assert lib.MhConvGeom._fields_ == [(n, ctypes.c_int32) for n in ("B", "H", "W", "C", "KH", "KW", "stride", "pad", "Cout", "ldk")]
    # the anonymous typedef, several declarators per statement and several statements per line
    assert lib.MhRowsJob._fields_ == [(n, P) for n in ("src", "dst", "idx", "rows_dev")] + \
        [(n, ctypes.c_int32) for n in ("n", "rows", "D", "stride", "offset", "reserved_")]
    # `const float *Wt, *bt;`: the star belongs to the declarator
    assert lib.MhHeadParams._fields_ == [(n, P) for n in ("Wt", "bt", "Wi", "bi", "Wf", "bf_", "Wo", "bo")]
    assert (lib.MH_OK, lib.MH_EINVAL, lib.MH_ESHAPE, lib.MH_ELAUNCH) == (0, 1, 2, 3)
    assert (lib.MH_GEMM_MAX_GROUP, lib.MH_GEMM_DERIV_AUX, lib.MH_BN_ACCUM_PARAM_GRADS, lib.MH_F32_BN, lib.MH_CONV_MAX_GROUP) == (8, 16, 2, 8, 6)
    # ops.py hands (c_float * 3) host arrays to mh_image_normalize_u8's two c_void_p arguments
    assert ctypes.c_void_p.from_param((ctypes.c_float * 3)()) is not None


_SMALL_HEADER = """
#define MH_N 2 /* a bound */
typedef void* mh_stream_t;
typedef struct A { const float *v[MH_N], *w; int32_t n, m; } A;
int mh_x(const A* a /*host*/, int64_t n,
         mh_stream_t stream);
"""


@pytest.mark.parametrize("bad, named", [
    ("int mh_y(size_t n);", "size_t"),                                           # a type name outside the rule
    ("int mh_y(const struct foo* p);", "struct foo"),                            # ... also behind a pointer
    ("void mh_y(int n);", "void"),                                               # ... and as a return type
    ("typedef struct B { long n; } B;", "long"),
    ("typedef struct B { float v[MH_NOPE]; } B;", "MH_NOPE"),                     # an array bound that is no known constant
    ("typedef struct B { float v[2 * MH_N]; } B;", "v[2 * MH_N]"),               # a declarator it cannot split
    ("int mh_y(int, float y);", "mh_y"),                                         # a prototype it cannot split
    ("int mh_y(int (*f)(int));", "mh_y"),
    ("int mh_x(int n);", "mh_x"),                                                # declared twice: 3 calls, 2 prototypes
    ("#define MH_M (1 << 3)", "MH_M"),                                           # a constant that is no integer
    ("static inline int twice(int a) { return a + a; }", "twice"),               # anything that is no declaration it knows
])
def test_reader_is_strict(lib, bad, named):
    """The reader never skips: text it cannot read raises MemehipError naming that text, so the import stops."""
    consts, structs, protos = lib.read_header(_SMALL_HEADER)
    assert consts == {"MH_N": 2} and list(protos) == ["mh_x"]
    assert protos["mh_x"] == (ctypes.c_int, [ctypes.POINTER(structs["A"]), ctypes.c_int64, ctypes.c_void_p])
    assert structs["A"]._fields_ == [("v", ctypes.c_void_p * 2), ("w", ctypes.c_void_p), ("n", ctypes.c_int32), ("m", ctypes.c_int32)]
    with pytest.raises(lib.MemehipError, match=re.escape(named)):
        lib.read_header(_SMALL_HEADER + bad + "\n")


def test_isa_guard_bands_hold(lib):
    """tools/isa_guard.py (run by __graft_entry__.build()): register counts, spills, scratch and the K-loop ISA of the hot kernels
    are inside the committed bands -- and the guard does fire: a band moved away from the build must fail."""
    import json
    import subprocess
    import sys
    guard = os.path.join(ROOT, "tools", "isa_guard.py")
    r = subprocess.run([sys.executable, guard], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    bands = json.load(open(os.path.join(ROOT, "tools", "isa_bands.json")))["kernels"]
    assert any("gemm_kernel<0, 0, false>" in k for k in bands) and any("conv_gemm_kernel" in k for k in bands) and any("attn_" in k for k in bands)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_guard
    got = isa_guard.collect()
    k = "gemm.f16.o:gemm_kernel<0, 0, false>"
    assert bands[k]["vgpr_count"][0] <= got[k]["vgpr_count"] <= bands[k]["vgpr_count"][1]
    assert got[k]["loop_mfma"] == 16 and got[k]["vgpr_spill_count"] == 0 and got[k]["waterfall_loops"] == 0
    # the accident of round 3 (112 -> 90 VGPRs) would have left the band
    assert not (bands[k]["vgpr_count"][0] <= 90 <= bands[k]["vgpr_count"][1])


def test_load_chain_guard_and_skeleton_tool(lib):
    """round 4, second session: the guard's `load_chain` (longest run of load - s_waitcnt vmcnt(0) - load: dependent memory round trips)
    is zero for the kernels that were rewritten for it, and tools/isa_loadchain.py prints a kernel's memory skeleton from the source."""
    import json
    import subprocess
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_guard
    bands = json.load(open(os.path.join(ROOT, "tools", "isa_bands.json")))["kernels"]
    got = isa_guard.collect()
    for k in ("layernorm.f16.o:ln_fwd_kernel<2, 2>", "head.f16.o:linear_fwd_kernel", "layernorm.f16.o:colsum_partials_kernel"):
        assert bands[k]["load_chain"] == [0, 0] and got[k]["load_chain"] == 0, k
    # a synthetic chain is counted: load, wait, load, wait
    insns = [(0, "global_load_dwordx4 v[0:3], v[4:5], off"), (4, "s_waitcnt vmcnt(0)"), (8, "s_cbranch_execz 12"),
             (12, "global_load_dwordx4 v[0:3], v[4:5], off"), (16, "s_waitcnt vmcnt(0) lgkmcnt(1)"), (20, "global_store_dword v0, v1, off")]
    assert isa_guard.load_chain(insns) == 2
    assert isa_guard.load_chain([(0, "global_load_dword v0, v1, off"), (4, "global_load_dword v2, v1, off"), (8, "s_waitcnt vmcnt(1)")]) == 0
    tool = os.path.join(ROOT, "tools", "isa_loadchain.py")
    src = os.path.join(ROOT, "multimodal_propaganda_meme_classification_amd", "csrc", "dwconv.hip")
    r = subprocess.run([sys.executable, tool, src, "dwconv_weight_pack"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 2 and "dwconv_weight_pack_kernel" in lines[0] and set(lines[1].split()) >= {"L", "S", "$"}
