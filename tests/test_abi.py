"""CPU: the C-ABI library loads without a GPU, exports every symbol include/cnr_hip.h declares, the ctypes tables the binding
reads from the header are what this file's own reading of it (and the C compiler's) says, and argument errors come back as codes
(never exit(), never a crash)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "cnr_hip.h")
LIB = os.path.join(ROOT, "category-nerf-reconstruction-official_amd", "libcnr_hip.so")


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(int64_t|int)\s+(cnr_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
        args = [a.strip() for a in m.group(3).split(",")]
        out[m.group(2)] = [a for a in args if a and a != "void"]
    return out


def declared_int64_returns():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"\bint64_t\s+(cnr_\w+)\s*\(", src))


DECLARED_CTYPES = {"float": ctypes.c_float, "double": ctypes.c_double, "int": ctypes.c_int, "int32_t": ctypes.c_int32,
                   "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64}


def assert_row_matches(name, row, decls):
    """one row of _C.SIGNATURES against the parameter declarations declared_functions() read for that name: a pointer is
    c_void_p, every other C type has exactly one ctypes type, and a type this test does not know fails it"""
    assert len(row) == len(decls), (name, len(row), len(decls))
    for ct, decl in zip(row, decls):
        ctype = decl.replace("const ", "").split()[0]
        assert "*" in decl or ctype in DECLARED_CTYPES, (name, decl)
        assert ct is (ctypes.c_void_p if "*" in decl else DECLARED_CTYPES[ctype]), (name, decl, ct)


def load_library():
    """libcnr_hip.so as the binding loads it (argtypes / restype set from its tables), built first when it is not there"""
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    import cnr_amd
    return cnr_amd._C.load()


@pytest.fixture(scope="module")
def lib():
    return load_library()


def test_header_declares_the_hot_path():
    fns = declared_functions()
    for name in ("cnr_sample_rays", "cnr_pe_fwd", "cnr_pe_bwd", "cnr_mlp_fwd_f32", "cnr_mlp_bwd_f32",
                 "cnr_composite_fwd", "cnr_composite_bwd", "cnr_loss_fwd_bwd", "cnr_adamw_step", "cnr_pack_weights",
                 "cnr_field_fwd", "cnr_field_bwd_pipe", "cnr_render_loss", "cnr_render_loss_finish", "cnr_step_epilogue", "cnr_param_prep", "cnr_step_prologue", "cnr_adamw_epilogue", "cnr_step_tail", "cnr_slice_maxdepth", "cnr_step_grad", "cnr_field_fwd_render", "cnr_gather_pool", "cnr_dense_fwd", "cnr_dense_bwd", "cnr_latent_fwd", "cnr_latent_bwd", "cnr_step_advance", "cnr_field_train", "cnr_slice_maskcounts", "cnr_field_fwd_fp8",
                 "cnr_pack_weights_fp8"):
        assert name in fns, name


def test_every_declared_symbol_is_exported(lib):
    for name in declared_functions():
        assert hasattr(lib, name), f"{name} declared in cnr_hip.h but not exported by libcnr_hip.so"


def test_ctypes_table_matches_header():
    import cnr_amd
    fns = declared_functions()
    sig = cnr_amd._C.SIGNATURES
    assert set(sig) == set(fns) and len(fns) >= 129, (set(sig) ^ set(fns))
    for name, args in fns.items():
        assert_row_matches(name, sig[name], args)
    seen = {decl.replace("const ", "").split()[0] for args in fns.values() for decl in args if "*" not in decl}
    assert seen >= {"float", "double", "int", "int64_t", "uint64_t"}, seen          # what the loop above really compared


def test_int64_returns_match_header():
    import cnr_amd
    want = declared_int64_returns()
    assert cnr_amd._C._RESTYPE64 == want and len(want) >= 27 and want <= set(declared_functions())
    assert {"cnr_pack_bytes", "cnr_clique_workspace_bytes", "cnr_tsdf_touch_slots"} <= want


def declared_structs():
    """typedef struct NAME_args { type field; ... } NAME_args;  ->  {NAME: [(field, c type text), ...]}"""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"typedef\s+struct\s+(cnr_\w+)_args\s*\{(.*?)\}\s*\1_args\s*;", src, flags=re.S):
        fields = []
        for decl in m.group(2).split(";"):
            decl = " ".join(decl.split())
            if decl:
                typ, name = decl.rsplit(" ", 1)
                if name.startswith("*"):
                    typ, name = typ + "*", name.lstrip("*")
                fields.append((name, typ))
        out[m.group(1)] = fields
    return out


def test_argument_blocks_match_the_header():
    """The versioned argument structs: same fields, order and C types in include/cnr_hip.h and in the ctypes table, and the
    same size as the C compiler gives the header's typedef."""
    import subprocess
    import tempfile
    import cnr_amd
    _C = cnr_amd._C
    structs = declared_structs()
    assert set(structs) == set(_C.STRUCTS) and len(structs) == 5
    for name, fields in structs.items():
        assert fields[0] == ("struct_size", "uint32_t") and fields[1] == ("abi_version", "uint32_t"), name
        assert [f for f, _ in fields[2:]] == [f for f, _ in _C.STRUCTS[name]], name
        for (f, typ), (_, ct) in zip(fields[2:], _C.STRUCTS[name]):
            assert "*" in typ or typ in DECLARED_CTYPES, (name, f, typ)
            assert ct is (ctypes.c_void_p if "*" in typ else DECLARED_CTYPES[typ]), (name, f, typ)
    scalars = {typ for fields in structs.values() for _, typ in fields if "*" not in typ}
    assert scalars >= {"float", "int32_t", "uint32_t", "int64_t", "uint64_t"}, scalars
    src = '#include <stdio.h>\n#include "cnr_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu %d", sizeof(cnr_step_prologue_args), ' \
          'sizeof(cnr_step_tail_args), sizeof(cnr_field_train_args), sizeof(cnr_bg_backward_render_args), ' \
          'sizeof(cnr_bg_tail_sample_args), CNR_ABI_VERSION);return 0;}'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.dirname(HEADER), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")], check=True)
        a, b, c, e, f5, ver = (int(v) for v in subprocess.run([os.path.join(d, "s")], capture_output=True, text=True).stdout.split())
    assert (a, b, c, e, f5) == tuple(ctypes.sizeof(_C.struct_type(n)) for n in ("cnr_step_prologue", "cnr_step_tail", "cnr_field_train",
                                                                                  "cnr_bg_backward_render", "cnr_bg_tail_sample"))
    assert ver == _C.ABI_VERSION


def test_argument_blocks_of_another_revision_are_refused(lib):
    """struct_size / abi_version that do not match this library: CNR_E_ARG before anything else is read."""
    import cnr_amd
    _C = cnr_amd._C
    for name in _C.STRUCTS:
        fn = getattr(lib, name)
        assert fn.argtypes == [ctypes.c_void_p, ctypes.c_void_p] and fn.restype is ctypes.c_int, name
        st = _C.struct_type(name)()
        st.struct_size, st.abi_version = ctypes.sizeof(st) - 8, _C.ABI_VERSION
        assert fn(ctypes.byref(st), None) == -1, name
        st.struct_size, st.abi_version = ctypes.sizeof(st), _C.ABI_VERSION + 1
        assert fn(ctypes.byref(st), None) == -1, name
        assert fn(None, None) == -1, name
        st.struct_size, st.abi_version = ctypes.sizeof(st), _C.ABI_VERSION      # right revision, all-NULL fields: still an error code
        assert fn(ctypes.byref(st), None) == -1, name


def test_binding_refuses_short_misspelt_and_surplus_arguments():
    """_C.call wants exactly the header's parameter list (round 2 padded missing trailing arguments with NULL / 0);
    _C.call_struct wants every field of the argument block by name."""
    import torch
    import cnr_amd
    _C = cnr_amd._C
    with pytest.raises(_C.CnrError, match="arguments for"):
        _C.call("cnr_pe_fwd", None, None, None, 1, 10)                     # scale and the output left out
    with pytest.raises(_C.CnrError, match="arguments for"):
        _C.call("cnr_step_advance", None, 1, 2, 3)
    with pytest.raises(_C.CnrError, match="versioned argument block"):
        _C.call("cnr_step_tail", *([None] * 42))
    good = {n: (None if t is ctypes.c_void_p else 0) for n, t in _C.STRUCTS["cnr_step_tail"]}
    with pytest.raises(_C.CnrError, match="missing fields \\['code_lr'\\]"):
        _C.call_struct("cnr_step_tail", **{k: v for k, v in good.items() if k != "code_lr"})
    with pytest.raises(_C.CnrError, match="unknown fields \\['learning_rate'\\]"):
        _C.call_struct("cnr_step_tail", learning_rate=1e-3, **good)
    with pytest.raises(_C.CnrError, match="expected a number"):
        _C.call_struct("cnr_step_tail", **dict(good, lr=None))
    with pytest.raises(_C.CnrError):                                          # a host tensor where a device pointer belongs
        _C.call_struct("cnr_step_tail", **dict(good, grad=torch.zeros(4)))


def test_argument_errors_are_return_codes(lib):
    """NULL pointers / bad sizes -> CNR_E_ARG (-1) before anything touches the device."""
    assert lib.cnr_version() >= 100
    assert lib.cnr_pack_bytes() == 62464
    assert lib.cnr_pe_fwd(None, None, None, 1, 10, 2.0, None) == -1
    assert lib.cnr_composite_fwd(None, None, None, None, None, None, None, None, 4, 8, 0, None) == -1
    assert lib.cnr_adamw_step(None, None, None, None, 10, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, None, None) == -1
    assert lib.cnr_step_advance(None, 1, None) == -1
    rec_entries = (13892 + 126 + 15 * 128 + 255) // 256 * 256     # trunk | two dB halves | up to 15 object rows x 128
    assert lib.cnr_field_bwd_workspace_bytes(2, 0) == 2 * 256 * rec_entries * 2       # bf16 entries


# ---- the binding's header reader on strings ------------------------------------------------------------------------------------
HEADER_TAIL = "\n#define CNR_ABI_VERSION 3\n"


def test_parse_header_pins_five_signatures():
    """five rows written out by hand: every row of the type map, both return types and an empty parameter list"""
    from cnr_amd import _C
    vp, i, i64, u64, f, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float, ctypes.c_double
    want = {"cnr_version": [],
            "cnr_camera_rays": [vp, i, i, f, f, f, f, vp],
            "cnr_sample_rays": [vp, vp, vp, vp, vp, vp, u64, u64, vp, i64, vp, i, i, i, i, i, f, f, f,
                                vp, vp, vp, vp, vp, vp, vp, vp, vp, i, vp, vp, i, vp],
            "cnr_unproject_emit": [vp, vp, vp, i, i, i, d, d, d, d, vp, vp, vp, vp, vp],
            "cnr_nn_workspace_bytes": [i64, i64]}
    sig, ret64, structs, version = _C.parse_header(open(HEADER).read())
    for name, row in want.items():
        assert len(sig[name]) == len(row) and all(a is b for a, b in zip(sig[name], row)), (name, sig[name])
        assert (name in ret64) == (name == "cnr_nn_workspace_bytes"), name
    assert version == 3 and len(structs) == 5
    # ... and a text of its own: comments of both kinds, a block, the 32-bit types
    text = """/* int cnr_in_a_comment(int a); */
    int64_t cnr_a(void);   // int cnr_in_a_line_comment(size_t n);
    int cnr_b(const uint8_t* p, int32_t a, uint32_t b, int64_t c, uint64_t d, float e, double f, int g,
              void* stream);
    typedef struct cnr_c_args {
      uint32_t struct_size;
      uint32_t abi_version;   /* first */
      const float* x;
      int32_t n;
      uint64_t seed;
    } cnr_c_args;
    int cnr_c(const cnr_c_args* args, void* stream);
    #define CNR_ABI_VERSION 7
    """
    sig, ret64, structs, version = _C.parse_header(text)
    assert sig == {"cnr_a": [], "cnr_b": [vp, ctypes.c_int32, ctypes.c_uint32, i64, u64, f, d, i, vp], "cnr_c": [vp, vp]}
    assert ret64 == {"cnr_a"} and version == 7
    assert structs == {"cnr_c": [("x", vp), ("n", ctypes.c_int32), ("seed", u64)]}


@pytest.mark.parametrize("text,match", [
    ("int cnr_x(const float* p, size_t n, void* stream);", "size_t"),                               # a type outside the map
    ("void cnr_x(const float* p, void* stream);", "returns 'void'"),                                # a third return type
    ("int cnr_ok(int n);\nint cnr_x(void (*done)(int), void* stream);", r"prototype for \['cnr_x'\]"),     # not consumed
    ("typedef struct cnr_x_args { const float* p; int32_t n; } cnr_x_args;\nint cnr_x(const cnr_x_args* a, void* stream);",
     "must begin with uint32_t struct_size, abi_version"),
], ids=["size_t_parameter", "void_return", "function_pointer_parameter", "block_without_its_head"])
def test_parse_header_is_strict(text, match):
    """what the reader cannot read exactly is an error that names it, never a guessed or a skipped row"""
    from cnr_amd import _C
    assert _C.parse_header("int cnr_ok(int n);" + HEADER_TAIL)[0] == {"cnr_ok": [ctypes.c_int]}       # the frame alone reads
    with pytest.raises(_C.CnrError, match=match):
        _C.parse_header(text + HEADER_TAIL)


def test_missing_header_fails_loudly(monkeypatch):
    from cnr_amd import _C
    monkeypatch.setattr(_C, "HEADER_PATH", "/nonexistent/include/cnr_hip.h")
    with pytest.raises(_C.CnrError, match="/nonexistent/include/cnr_hip.h"):
        _C._read_header()


def test_missing_library_fails_loudly(monkeypatch):
    import cnr_amd
    monkeypatch.setattr(cnr_amd._C, "_lib", None)
    monkeypatch.setattr(cnr_amd._C, "LIB_PATH", "/nonexistent/libcnr_hip.so")
    with pytest.raises(cnr_amd._C.CnrError):
        cnr_amd._C.load()


def test_cpu_tensors_are_rejected():
    """No CPU fallback: handing a host tensor to a kernel wrapper raises."""
    import torch
    import cnr_amd
    with pytest.raises(cnr_amd._C.CnrError):
        cnr_amd.ops.UniDirsEmbedFn.apply(torch.zeros(4, 3), torch.zeros(21, 3), 2.0)


def test_kernels_contain_no_instruction_emitting_inline_asm():
    """hipcc pads no hazards around an inline-asm instruction and may hand its output a register an MFMA issued just before
    is still reading ("a hazard worth recording": run-to-run different gradients that the small fixtures
    never showed).  The kernels therefore use asm statements only as optimisation barriers: every asm template in csrc/ must
    be the empty string -- or an assembler COMMENT ("; ..."), which emits nothing either (the phase marks of tools/isa_mix.py,
    compiled in only with -DCNR_ISA_MARKS)."""
    csrc = os.path.join(ROOT, "category-nerf-reconstruction-official_amd", "csrc")
    bad = []
    for name in sorted(os.listdir(csrc)):
        if not name.endswith((".hip", ".h")):
            continue
        src = open(os.path.join(csrc, name)).read()
        for m in re.finditer(r"\basm\s*(?:volatile)?\s*\(\s*\"([^\"]*)\"", src):
            if m.group(1).strip() and not m.group(1).strip().startswith(";"):
                bad.append((name, m.group(1)))
    assert not bad, bad
