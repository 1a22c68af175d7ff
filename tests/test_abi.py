"""CPU checks of the drop-in boundary: the C-ABI library builds, loads, and exports exactly what
include/vjepa_hip.h declares (no compute is launched here -- there is no GPU on this host)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "vjepa_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(vj_[a-z0-9_]+)\s*\(", text)) - {"vj_stream_t"})


def test_library_builds_and_exports_every_declared_symbol():
    from jepa_amd import build
    from jepa_amd.hip import lib as L
    build.build(verbose=False)
    lib = L.load_library()
    names = _declared()
    assert len(names) >= 25
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/vjepa_hip.h but not exported"
        assert n in L.SIGNATURES, f"{n} has no ctypes signature"
    for n in L.SIGNATURES:
        assert n in names, f"{n} bound in python but not declared in the header"
    assert lib.vj_abi_version() == 1


def _prototypes():
    """name -> (return type, [parameter types]) as C type strings, parsed out of include/vjepa_hip.h: comments, preprocessor lines,
    struct typedefs, enums and the remaining typedefs are stripped first; every statement that is left must be a prototype."""
    text = open(os.path.join(ROOT, "include", "vjepa_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', " ", text)
    text = re.sub(r"\b(?:typedef\s+struct\s+\w+|enum)\s*\{.*?\}\s*\w*\s*;", " ", text, flags=re.S)
    text = re.sub(r"\btypedef\b[^;{}]*;", " ", text)
    protos = {}
    for stmt in (s.strip() for s in text.split(";")):
        if stmt in ("", "}"):       # "}" closes extern "C"
            continue
        m = re.fullmatch(r"([\w\s\*]+?)\s*\b(vj_\w+)\s*\(([^()]*)\)", stmt, flags=re.S)
        assert m, f"not a prototype: {stmt!r}"
        ret, name, params = m.groups()
        assert name not in protos, f"{name} declared twice"
        params = [] if params.strip() in ("", "void") else [p.strip() for p in params.split(",")]
        types = []
        for p in params:
            pm = re.fullmatch(r"(.*?[\s\*])(\w+)\s*(\[\s*\])?", p, flags=re.S)    # type, name, optional []
            assert pm, f"{name}: parameter {p!r}"
            types.append(pm.group(1).strip() + ("*" if pm.group(3) else ""))
        protos[name] = (" ".join(ret.split()), types)
    return protos


_POINTER_TYPEDEFS = {"vj_stream_t", "vj_comm_t", "vj_layer_cb_t"}
_C_SCALARS = {"int64_t": "int64", "int": "int", "float": "float", "double": "double", "void": "void"}


def _c_class(ctype):
    t = " ".join(re.sub(r"\bconst\b", " ", ctype).split())
    if "*" in t or t in _POINTER_TYPEDEFS:
        return "pointer"
    assert t in _C_SCALARS, f"C type {ctype!r} has no class"
    return _C_SCALARS[t]


def _ctypes_class(t):
    import ctypes
    if t is None:
        return "void"
    scalars = {ctypes.c_int64: "int64", ctypes.c_int: "int", ctypes.c_float: "float", ctypes.c_double: "double"}
    if t in scalars:
        return scalars[t]
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, (ctypes._Pointer, ctypes._CFuncPtr)):
        return "pointer"
    raise AssertionError(f"ctypes type {t!r} has no class")


def test_signatures_match_the_header_type_by_type():
    """SIGNATURES against the prototypes of include/vjepa_hip.h: the same names, and per name the same return class and the same
    class for every parameter (pointer / int64 / int / float / double) -- an int bound as c_int64 or a float bound as c_double
    would pass the by-name test above and corrupt arguments at run time."""
    from jepa_amd.hip import lib as L
    protos = _prototypes()
    assert set(protos) == set(L.SIGNATURES), sorted(set(protos) ^ set(L.SIGNATURES))
    assert sorted(protos) == _declared()
    wrong = []
    for name, (ret, params) in sorted(protos.items()):
        res, args = L.SIGNATURES[name]
        want = [_c_class(ret)] + [_c_class(p) for p in params]
        have = [_ctypes_class(res)] + [_ctypes_class(a) for a in args]
        if want != have:
            wrong.append(f"{name}: header {want}, SIGNATURES {have}")
    assert not wrong, "\n".join(wrong)


def test_type_classes_tell_the_widths_apart():
    """The classifier itself: the mistakes it exists for land in different classes."""
    import ctypes
    assert _ctypes_class(ctypes.c_int) != _ctypes_class(ctypes.c_int64)
    assert _ctypes_class(ctypes.c_float) != _ctypes_class(ctypes.c_double)
    assert _c_class("const int64_t*") == _c_class("vj_stream_t") == _c_class("vj_comm_t*") == "pointer"
    assert [_c_class(t) for t in ("int64_t", "int", "float", "double", "const char*")] == ["int64", "int", "float", "double", "pointer"]


def test_no_cpu_fallback_in_ops():
    """The product path must fail loudly on CPU tensors instead of silently computing somewhere else."""
    import pytest
    import torch
    from jepa_amd.hip import ops
    x = torch.zeros(4, 8, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        ops.layernorm_fwd(x, torch.ones(8), torch.zeros(8), 1e-6)
    with pytest.raises(ValueError):
        ops.gemm_nt(x, x)


def test_chain_workspace_queries_and_host_side_validation():
    """Pure host functions of the launch chains, callable without a GPU: workspace sizes follow the documented layout
    (16*D bf16 per token and block + row statistics + lse; one set + one x buffer without saving), and argument errors are
    rejected before any HIP call (negative return code + message)."""
    import ctypes
    from jepa_amd.hip import lib as L
    lib = L.load_library()
    M, D, H, n = 10560, 1024, 16, 24
    save = lib.vj_blocks_fwd_ws_bytes(M, D, 4 * D, H, n, 1)
    nosave = lib.vj_blocks_fwd_ws_bytes(M, D, 4 * D, H, n, 0)
    per_block = 16 * D * 2 * M + 4 * 4 * M + 4 * H * M + 8 * M   # activations + mean/rstd x2 + lse + the folded LayerNorm's row statistics
    assert save % 256 == 0 and per_block * n <= save <= per_block * n + n * 14 * 256
    assert per_block + 2 * D * M <= nosave <= per_block + 2 * D * M + 14 * 256
    assert lib.vj_blocks_fwd_ws_bytes(2 * M, D, 4 * D, H, n, 1) >= 2 * save - n * 13 * 256
    bwd = lib.vj_blocks_bwd_ws_bytes(M, D, 4 * D, H)
    assert bwd > 2 * (4 * D + D + 3 * D) * 2 * M                 # two parities of du / dx1 / dqkv at least
    assert lib.vj_grad_stats_chunks() == 8 and lib.vj_comm_unique_id_bytes() == 128
    # validation happens on the host, before anything touches a device
    seg = (L.VjSeg * 1)(L.VjSeg(0, 1, 8))
    rc = lib.vj_blocks_fwd(None, 0, None, None, 8, 64, 2, seg, 1, 1e-6, 0, 0, None, 0, None)
    assert rc < 0 and b"no blocks" in lib.vj_last_error()
    blk = (L.VjBlock * 1)()
    blk[0].qkv.n_out, blk[0].qkv.k_in = 3 * 64, 64
    blk[0].proj.n_out, blk[0].proj.k_in = 64, 64
    blk[0].fc1.n_out, blk[0].fc1.k_in = 256, 64
    blk[0].fc2.n_out, blk[0].fc2.k_in = 64, 256
    rc = lib.vj_blocks_fwd(blk, 1, None, None, 8, 64, 2, (L.VjSeg * 1)(L.VjSeg(0, 1, 7)), 1, 1e-6, 0, 0, None, 0, None)
    assert rc < 0 and b"segments" in lib.vj_last_error()
    blk[0].fc2.k_in = 128
    rc = lib.vj_blocks_fwd(blk, 1, None, None, 8, 64, 2, seg, 1, 1e-6, 0, 0, None, 0, None)
    assert rc < 0 and b"inconsistent Linear shapes" in lib.vj_last_error()
    comm = ctypes.c_void_p()
    assert lib.vj_comm_allreduce_bucket(None, None, 4, None) != 0   # null communicator (or no RCCL on this host): refused
