"""ctypes binding of libcnr_hip.so (the C-ABI declared in include/cnr_hip.h).

The header is the one statement of the ABI: parse_header() reads every prototype, every versioned argument block and
CNR_ABI_VERSION from it when the package is imported, so a new entry point takes its prototype and its kernel and nothing here.

There is NO CPU fallback: if the library is missing, or a tensor is not a contiguous device tensor of
the documented dtype, the call raises.  (tests/ may install a test double for host-logic tests on a
GPU-less box through :func:`install_test_double`; nothing in the product ever does.)
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# (CNR_HIP_LIB: another build of the same library, e.g. tools/exp's cycle-stamp build; never a different implementation)
LIB_PATH = os.environ.get("CNR_HIP_LIB") or os.path.join(_HERE, "libcnr_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "cnr_hip.h")      # in-tree, as csrc/Makefile reads it

_vp, _f = ctypes.c_void_p, ctypes.c_float
_CTYPES = {"float": _f, "double": ctypes.c_double, "int": ctypes.c_int, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32,
           "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64}
_BLOCK_HEAD = [("struct_size", ctypes.c_uint32), ("abi_version", ctypes.c_uint32)]


class CnrError(RuntimeError):
    pass


def _declaration(decl, where):
    """`const float* x` -> ("x", c_void_p), `int64_t n` -> ("n", c_int64): anything with a `*` is a pointer, every other type
    must be one of _CTYPES.  There is no default: a wrong guess would shift or truncate an argument silently."""
    words = decl.replace("*", " * ").split()
    name, typ = words[-1], [w for w in words[:-1] if w != "const"]
    if not name.isidentifier() or not typ:
        raise CnrError(f"cnr_hip.h, {where}: cannot read the declaration {decl.strip()!r}")
    if "*" in typ:
        return name, _vp
    if len(typ) != 1 or typ[0] not in _CTYPES:
        raise CnrError(f"cnr_hip.h, {where}: {name} has type {' '.join(typ)!r}, which the binding's type map does not hold")
    return name, _CTYPES[typ[0]]


def parse_header(text):
    """The text of include/cnr_hip.h -> (signatures, restype64, structs, abi_version):
    signatures {entry point: [ctypes type of every parameter, the trailing stream included]}, restype64 the names that return
    int64_t (all others return int), structs {entry point: [(field, ctypes type), ...]} of every `cnr_X_args` typedef without
    its two leading fields struct_size and abi_version, abi_version the value of CNR_ABI_VERSION.  Strict: whatever it cannot
    read exactly raises CnrError."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    signatures, restype64, structs = {}, set(), {}
    protos = re.findall(r"(\w+)\s+(cnr_\w+)\s*\(([^;()]*)\)\s*;", text)
    for ret, name, params in protos:
        if ret not in ("int", "int64_t"):
            raise CnrError(f"cnr_hip.h: {name} returns {ret!r}; entry points return int or int64_t")
        params = [] if params.strip() in ("", "void") else params.split(",")
        signatures[name] = [_declaration(p, name)[1] for p in params]
        if ret == "int64_t":
            restype64.add(name)
    met = re.findall(r"\b(cnr_\w+)\s*\(", text)
    if met != [name for _, name, _ in protos] or len(signatures) != len(protos):
        odd = sorted(n for n in set(met) if met.count(n) != 1 or n not in signatures)
        raise CnrError(f"cnr_hip.h: cannot read exactly one prototype for {odd}")
    blocks = re.findall(r"typedef\s+struct\s+(cnr_\w+)_args\s*\{(.*?)\}\s*\1_args\s*;", text, flags=re.S)
    if len(blocks) != len(re.findall(r"\btypedef\b", text)):
        raise CnrError("cnr_hip.h: a typedef that is not `typedef struct cnr_X_args { ... } cnr_X_args;`")
    for name, body in blocks:
        fields = [_declaration(d, name + "_args") for d in body.split(";") if d.strip()]
        if fields[:2] != _BLOCK_HEAD:
            raise CnrError(f"cnr_hip.h: {name}_args must begin with uint32_t struct_size, abi_version; it begins {fields[:2]}")
        structs[name] = fields[2:]
    version = re.search(r"#\s*define\s+CNR_ABI_VERSION\s+(\d+)\s*$", text, flags=re.M)
    if version is None:
        raise CnrError("cnr_hip.h: no #define CNR_ABI_VERSION <number>")
    return signatures, restype64, structs, int(version.group(1))


def _read_header():
    if not os.path.exists(HEADER_PATH):
        raise CnrError(f"{HEADER_PATH} not found: the binding reads its signatures from the header, in its place in the tree")
    with open(HEADER_PATH) as f:
        return parse_header(f.read())


# name -> argtypes | the names that return int64_t (all others: int) | name -> fields of its versioned argument block, which
# call_struct() wants by NAME: a missing, misspelt or surplus one raises instead of shifting 40 values | CNR_ABI_VERSION
SIGNATURES, _RESTYPE64, STRUCTS, ABI_VERSION = _read_header()
_struct_types = {}


def struct_type(name):
    """ctypes.Structure of entry point `name`'s argument block (natural C alignment, like the header's typedef)."""
    if name not in _struct_types:
        _struct_types[name] = type(name + "_args", (ctypes.Structure,), {"_fields_": _BLOCK_HEAD + STRUCTS[name]})
    return _struct_types[name]


_lib = None
_double = None


def load():
    """Load libcnr_hip.so; raise loudly when it is absent (build with __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CnrError(f"{LIB_PATH} not found: the HIP extension is not built "
                           "(run `python -c 'import __graft_entry__ as g; g.build()'`); there is no CPU path")
        lib = ctypes.CDLL(LIB_PATH)
        for name, argtypes in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.argtypes = argtypes
            fn.restype = ctypes.c_int64 if name in _RESTYPE64 else ctypes.c_int
        _lib = lib
    return _lib


def install_test_double(obj):
    """tests/ only: route calls to `obj.<name>(*tensors_and_scalars)` instead of the HIP library."""
    global _double
    _double = obj


def _ptr(t, dtype=None, allow_none=False):
    if t is None:
        if allow_none:
            return None
        raise CnrError("required tensor is None")
    if not t.is_cuda:
        raise CnrError("cnr kernels take device tensors only (got a CPU tensor); there is no CPU path")
    if not t.is_contiguous():
        raise CnrError("cnr kernels take contiguous tensors")
    if dtype is not None and t.dtype != dtype:
        raise CnrError(f"expected dtype {dtype}, got {t.dtype}")
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- optional per-kernel HIP-event timing (bench.py's roofline leg) -------------------------------------
_timing = None  # {name: [(start_event, end_event), ...]} when enabled


def enable_kernel_timing(names):
    """Record a HIP event pair (on the launch stream) around every call of the named entry points."""
    global _timing
    _timing = {n: [] for n in names}


def kernel_timings_ms():
    """-> {name: [ms, ...]} ; synchronises.  Disables timing."""
    global _timing
    torch.cuda.synchronize()
    out = {n: [a.elapsed_time(b) for a, b in evs] for n, evs in (_timing or {}).items()}
    _timing = None
    return out


def _event(name):
    """a HIP event recorded on the launch stream when enable_kernel_timing() named this entry point, else None"""
    if _timing is not None and name in _timing:
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e


def _check(name, rc):
    if rc and _double is not None:
        raise CnrError(f"{name} (test double) returned {rc}")
    if rc:
        raise CnrError(f"{name} failed with code {rc}" + (" (argument error)" if rc < 0 else " (hipError_t)"))


def call(name, *args):
    """args: torch tensors (passed as device pointers), None (NULL) or python scalars."""
    start = _event(name)
    if _double is not None:
        _check(name, getattr(_double, name)(*args))
    else:
        lib = load()
        conv = [_ptr(a) if torch.is_tensor(a) else a for a in args]
        # every parameter of the header's prototype, in order (optional pointers as an explicit None): a short or long
        # argument list is a caller bug, never padded
        if name in STRUCTS:
            raise CnrError(f"{name} takes a versioned argument block: use call_struct({name!r}, field=value, ...)")
        types = SIGNATURES[name][:-1]
        if len(conv) != len(types):
            raise CnrError(f"{name}: {len(conv)} arguments for {len(types)} parameters (include/cnr_hip.h)")
        _check(name, getattr(lib, name)(*conv, _stream()))
    if start is not None:
        _timing[name].append((start, _event(name)))


def call_struct(name, **fields):
    """Entry points with a versioned argument block: every field of STRUCTS[name] by keyword (tensors as device pointers,
    None = NULL).  Unknown or missing names raise."""
    st = _prepare_struct(name, fields)       # (the argument block is filled BEFORE the first event: ~40 us of host work that an
    start = _event(name)                     # idle GPU would otherwise show as kernel time)
    _invoke_struct(name, st)
    if start is not None:
        _timing[name].append((start, _event(name)))


def _prepare_struct(name, fields):
    spec = STRUCTS[name]
    names = [n for n, _ in spec]
    missing, unknown = [n for n in names if n not in fields], [n for n in fields if n not in names]
    if missing or unknown:
        raise CnrError(f"{name}: missing fields {missing}, unknown fields {unknown}")
    if _double is not None:
        return dict(fields)
    load()
    st = struct_type(name)()
    st.struct_size, st.abi_version = ctypes.sizeof(st), ABI_VERSION
    for n, t in spec:
        v = fields[n]
        if t is _vp:
            v = _ptr(v) if torch.is_tensor(v) else v
            if v is not None and not isinstance(v, int):
                raise CnrError(f"{name}.{n}: expected a device tensor or None, got {type(fields[n]).__name__}")
        elif torch.is_tensor(v) or v is None:
            raise CnrError(f"{name}.{n}: expected a number, got {type(v).__name__}")
        elif t is not _f:
            v = int(v)
        setattr(st, n, v)
    return st


def _invoke_struct(name, st):
    """one launch with a filled argument block (also on its own: FusedCategoryTrainer.time_field_train fills the block once)"""
    if _double is not None:
        return _check(name, getattr(_double, name)(**st))
    _check(name, getattr(load(), name)(ctypes.byref(st), _stream()))


def version():
    return load().cnr_version()


def pack_bytes():
    return int(load().cnr_pack_bytes())


def field_bwd_workspace_bytes(C, max_blocks):
    """bytes of the per-workgroup gradient records of cnr_field_bwd_pipe / cnr_field_train"""
    return int(load().cnr_field_bwd_workspace_bytes(int(C), int(max_blocks)))


def render_loss_workspace_bytes(C, R):
    return int(load().cnr_render_loss_workspace_bytes(int(C), int(R)))


def workspace(nbytes, dev, what):
    """the uint8 device tensor for a `*_workspace_bytes` answer (at least one byte); a negative answer is the query's error"""
    nbytes = int(nbytes)
    if nbytes < 0:
        raise CnrError(f"{what}: workspace query failed with {nbytes}")
    return torch.empty(max(nbytes, 1), device=dev, dtype=torch.uint8)


def device_info():
    n_cu, lds, is950 = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    rc = load().cnr_device_info(ctypes.byref(n_cu), ctypes.byref(lds), ctypes.byref(is950))
    if rc != 0:
        raise CnrError(f"cnr_device_info failed with {rc}")
    return {"n_cu": n_cu.value, "lds_bytes": lds.value, "gfx950": bool(is950.value)}
