"""The C-ABI library: loads without a GPU, exports every symbol include/lightgaussian.h declares,
and the product path fails loudly (no fallback) when it cannot run.  No compute calls here."""
import ctypes as C
import os
import re

import pytest
import torch

import common
from lightgaussian_amd import _lib

HDR = os.path.join(common.ROOT, "include", "lightgaussian.h")
HDR_DEBUG = os.path.join(common.ROOT, "include", "lightgaussian_debug.h")     # diagnostics for tests/ and tools/: not the drop-in ABI


def _declared_functions(hdr=None):
    if hdr is None:
        return sorted(set(_declared_functions(HDR)) | set(_declared_functions(HDR_DEBUG)))
    src = open(hdr).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = re.findall(r"^\s*(?:int|size_t|void|const char\*)\s+\*?(lg_[a-z0-9_]+)\s*\(", src, flags=re.M)
    return sorted(set(names))


def test_header_declares_expected_entry_points():
    names = _declared_functions()
    for must in ("lg_forward", "lg_forward_count", "lg_backward", "lg_geom_bytes", "lg_img_bytes", "lg_binning_bytes",
                 "lg_backward_scratch_bytes", "lg_score_from_count", "lg_last_error", "lg_abi_version"):
        assert must in names
    assert set(names) == set(_lib.EXPORTS), (sorted(set(names) ^ set(_lib.EXPORTS)))
    # the drop-in header holds no diagnostics, the debug header nothing else (r3 verdict: eight lg_debug_* in the public ABI)
    assert not [n for n in _declared_functions(HDR) if n.startswith("lg_debug_")]
    assert all(n.startswith("lg_debug_") for n in _declared_functions(HDR_DEBUG)) and len(_declared_functions(HDR_DEBUG)) == 8


def test_library_built_loads_and_exports_every_declared_symbol():
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first (hipcc --offload-arch=gfx950)"
    lib = C.CDLL(_lib.LIB_PATH)
    for name in _declared_functions():
        assert hasattr(lib, name), f"{name} declared in include/lightgaussian.h but not exported"
    lib.lg_abi_version.restype = C.c_int
    assert lib.lg_abi_version() == 7
    lib.lg_img_bytes.restype = C.c_size_t
    lib.lg_img_bytes.argtypes = [C.c_int32, C.c_int32]
    assert lib.lg_img_bytes(1920, 1080) >= 1920 * 1080 * 8
    lib.lg_backward_scratch_bytes.restype = C.c_size_t
    lib.lg_backward_scratch_bytes.argtypes = [C.c_int32, C.c_int64]
    assert lib.lg_backward_scratch_bytes(1000, 5000) >= 5000 * 9 * 4


def test_struct_layout_matches_header():
    # field order of lg_view / lg_gaussians as declared in the header (ctypes mirrors must follow it)
    src = open(HDR).read()
    view = re.search(r"typedef struct lg_view \{(.*?)\} lg_view;", src, flags=re.S).group(1)
    fields = re.findall(r"\b([a-z_0-9]+);", re.sub(r"/\*.*?\*/", "", view, flags=re.S))
    assert fields == [f[0] for f in _lib.lg_view._fields_]
    gs = re.search(r"typedef struct lg_gaussians \{(.*?)\} lg_gaussians;", src, flags=re.S).group(1)
    fields = re.findall(r"\b([A-Za-z_0-9]+);", re.sub(r"/\*.*?\*/", "", gs, flags=re.S))
    assert fields == [f[0] for f in _lib.lg_gaussians._fields_]


def test_invalid_arguments_rejected_before_any_launch():
    lib = _lib.load()
    assert lib.lg_forward(None, None, None, None, _lib.ALLOC_FN(lambda u, n: 0), None, None, None, None, None, None) == _lib.LG_ERR_INVALID_ARGUMENT
    assert b"null" in lib.lg_last_error()


def test_no_cpu_fallback():
    """CPU tensors must raise, never silently run somewhere else."""
    from lightgaussian_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    rs = GaussianRasterizationSettings(8, 8, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3), False, False, False)
    r = GaussianRasterizer(rs)
    with pytest.raises(RuntimeError, match="no CPU path"):
        r(means3D=torch.zeros(4, 3), means2D=torch.zeros(4, 3), opacities=torch.ones(4, 1), colors_precomp=torch.ones(4, 3),
          scales=torch.ones(4, 3), rotations=torch.ones(4, 4))
    with pytest.raises(Exception, match="excatly one"):
        r(means3D=torch.zeros(4, 3), means2D=torch.zeros(4, 3), opacities=torch.ones(4, 1), scales=torch.ones(4, 3), rotations=torch.ones(4, 4))


def test_product_never_imports_the_oracle():
    import glob
    for path in glob.glob(os.path.join(common.ROOT, "lightgaussian_amd", "**", "*.py"), recursive=True) + \
            glob.glob(os.path.join(common.ROOT, "diff_gaussian_rasterization", "*.py")):
        txt = open(path).read()
        assert "oracle" not in txt.replace("(the reference has no CPU", ""), path
    for path in glob.glob(os.path.join(common.ROOT, "lightgaussian_amd", "csrc", "*")):
        assert "lg_oracle" not in open(path).read(), path


def test_the_library_has_no_process_wide_setters_and_the_segment_length_travels_with_the_view():
    """ABI v5 (r2 verdict): lg_set_segment_length / lg_set_long_tile_mode are gone -- the segment length is a field of lg_view,
    the long-tile mode two flag bits -- and the buffer size is a pure function of its arguments (no device needed here)."""
    lib = _lib.load()
    assert not hasattr(lib, "lg_set_segment_length") and not hasattr(lib, "lg_set_long_tile_mode")
    for name in ("lg_set_segment_length", "lg_set_long_tile_mode"):
        with pytest.raises(AttributeError):
            getattr(C.CDLL(_lib.LIB_PATH), name)
    assert [f[0] for f in _lib.lg_view._fields_][-2:] == ["segment_length", "count_sum"]
    for n in (0, 1, 63, 64, 100000):                                     # visibility bytes live inside the geom buffer (host-only query)
        off = lib.lg_geom_visible_offset(n)
        assert off % 16 == 0 and off + n <= lib.lg_geom_bytes(n)
    a, b = lib.lg_binning_bytes(100000, 640, 480, 0), lib.lg_binning_bytes(100000, 640, 480, 512)
    assert a == b > 0                                                   # 0 = the default of 512
    assert lib.lg_binning_bytes(100000, 640, 480, 64) > a               # more checkpoint records for shorter segments
    assert lib.lg_binning_bytes(100000, 640, 480, 100) == 0             # not a multiple of 64
    assert lib.lg_binning_bytes(100000, 640, 480, 32) == 0              # below 64
    assert lib.lg_binning_bytes(100000, 640, 480, 0) == a               # ... and asking twice changes nothing
    # a view with a bad segment length or contradictory long-tile flags is refused before any launch
    v = _lib.lg_view(8, 8, 1.0, 1.0, None, 1.0, None, None, 0, None, 0, 0, 100)
    g = _lib.lg_gaussians(0, 0, None, None, None, None, None, None, None, None)
    cb = _lib.ALLOC_FN(lambda u, n: 0)
    assert lib.lg_forward(C.byref(v), C.byref(g), None, None, cb, None, None, None, None, None, None) == _lib.LG_ERR_INVALID_ARGUMENT
    assert b"segment_length" in lib.lg_last_error()
    v = _lib.lg_view(8, 8, 1.0, 1.0, None, 1.0, None, None, 0, None, 0, _lib.FLAG_LONG_SERIAL | _lib.FLAG_LONG_PARALLEL, 0)
    assert lib.lg_forward(C.byref(v), C.byref(g), None, None, cb, None, None, None, None, None, None) == _lib.LG_ERR_INVALID_ARGUMENT
    assert b"exclude each other" in lib.lg_last_error()


def test_options_are_resolved_per_call_and_per_thread_never_by_mutating_the_defaults():
    """rasterizer.options(...) is thread-local and nests; an `options=` argument wins; the process defaults stay untouched
    (r2 verdict: prune_list_sharded / _ViewRunner used to flip module-level switches under other threads' feet)."""
    import threading
    from lightgaussian_amd import rasterizer as R
    base = dict(R._OPTIONS)
    seen = {}

    def other():
        seen["other"] = R.resolve_options()

    with R.options(sync_free=True, skip_color_in_count=True):
        with R.options(tag=7, long_tiles="serial"):
            inner = R.resolve_options({"segment_length": 128})
            t = threading.Thread(target=other); t.start(); t.join()
        mid = R.resolve_options()
    assert inner["sync_free"] is True and inner["skip_color_in_count"] is True and inner["tag"] == 7
    assert inner["long_tiles"] == "serial" and inner["segment_length"] == 128
    assert mid["long_tiles"] == base["long_tiles"] and "tag" not in mid and mid["sync_free"] is True
    assert seen["other"] == base                                          # the other thread saw the defaults
    assert R.resolve_options() == base and R._OPTIONS == base
    with pytest.raises(KeyError):
        R.options(no_such_knob=1)
    with pytest.raises(ValueError):
        R.resolve_options({"segment_length": 100})
    with pytest.raises(ValueError):
        R.set_option("long_tiles", "sometimes")
    assert R.set_option("long_tiles", "parallel") == base["long_tiles"]   # returns the previous default
    assert R.set_option("long_tiles", base["long_tiles"]) == "parallel"
    # a PendingBatch keeps the status words of ITS forwards only, tagged
    b = R.PendingBatch()
    b.add(None, ("k",), 3); b.add(None, ("k",), 5)
    assert b.resolve() == [(3, False), (5, False)] and b.resolve() == []


def test_prune_pass_and_view_runner_do_not_touch_the_process_defaults():
    import inspect
    from lightgaussian_amd import prune, parallel, dp
    for mod in (prune, parallel, dp):
        src = inspect.getsource(mod)
        assert "set_option(" not in src and "_OPTIONS[" not in src, mod.__name__


# ---- the binding against the headers: every prototype, constant and struct ---------------------------------------------------

_SCALAR_KINDS = {"int": "int32", "int32_t": "int32", "int64_t": "int64", "uint32_t": "uint32", "float": "float", "double": "double",
                 "size_t": "size_t", "void": "void"}
_POINTER_TYPES = ("hipStream_t", "lg_alloc_fn", "lg_chunk_fn")


def _header_text(headers=None):
    """The headers (None: the drop-in header and the debug header), comments removed."""
    src = "\n".join(open(h).read() for h in headers or (HDR, HDR_DEBUG))
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


def _c_kind(text, named):
    """Kind of a C return type (named=False) or of one parameter declaration `type name` (named=True)."""
    words = [w for w in re.findall(r"\w+", text) if w != "const"]
    if "*" in text or any(w in _POINTER_TYPES for w in words):
        return "pointer"
    assert len(words) == (2 if named else 1), f"cannot read the C type in {text!r}"
    return _SCALAR_KINDS[words[0]]


def _header_prototypes(headers=None):
    """name -> (return kind, [parameter kinds]) of every lg_* function the headers declare, in the order of the declarations."""
    src = re.sub(r"typedef\s+struct\s+\w+\s*\{.*?\}\s*\w+\s*;", "", _header_text(headers), flags=re.S)
    src = re.sub(r"typedef[^;{]*;|enum\s*\{.*?\}\s*;|^\s*#[^\n]*|extern\s+\"C\"\s*\{", "", src, flags=re.S | re.M)
    out = {}
    for ret, name, params in re.findall(r"([\w\s\*]+?)\b(lg_\w+)\s*\(([^()]*)\)\s*;", src):
        assert name not in out, f"{name} declared twice"
        params = [] if params.strip() in ("", "void") else params.split(",")
        out[name] = (_c_kind(ret, False), [_c_kind(p, True) for p in params])
    return out


def _ctypes_kind(t):
    if t is None:
        return "void"
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, (C._Pointer, C._CFuncPtr)):
        return "pointer"
    if t is C.c_size_t:           # (before the sized integers: on LP64 it is one class with c_uint64)
        return "size_t"
    return {C.c_int32: "int32", C.c_int64: "int64", C.c_uint32: "uint32", C.c_float: "float", C.c_double: "double"}[t]


def _prototype_mismatches(declared, table):
    """One line per function on which the header (`declared`: _header_prototypes()) and a binding table (name -> (restype, argtypes))
    disagree; every line begins with the function's name."""
    bad = [f"{n}: declared in the headers, not in the table" for n in sorted(set(declared) - set(table))]
    bad += [f"{n}: in the table, not declared in the headers" for n in sorted(set(table) - set(declared))]
    for name in sorted(set(declared) & set(table)):
        ret, params = declared[name]
        got_ret, got = _ctypes_kind(table[name][0]), [_ctypes_kind(t) for t in table[name][1]]
        if got_ret != ret:
            bad.append(f"{name}: returns {ret}, the table says {got_ret}")
        if len(got) != len(params):
            bad.append(f"{name}: {len(params)} parameters, the table has {len(got)}")
        bad += [f"{name}: parameter {k} is {a}, the table says {b}" for k, (a, b) in enumerate(zip(params, got)) if a != b]
    return bad


def check_extension_header(header, table):
    """What the test of every extension header (include/lightgaussian_<name>.h) holds its module's prototype table against: the
    table's names are the header's declarations in header order, every return and argument type matches, none of the names is
    declared in include/lightgaussian.h, and the built library exports every one.  Returns the parsed declarations."""
    declared = _header_prototypes((os.path.join(common.ROOT, "include", header),))
    assert list(declared) == list(table)
    assert _prototype_mismatches(declared, table) == []
    main = open(HDR).read()
    assert not any(name in main for name in table), "the extension's functions are declared in the extension header only"
    lib = C.CDLL(_lib.LIB_PATH)
    assert all(hasattr(lib, name) for name in table)
    return declared


def test_every_prototype_of_the_binding_matches_the_headers():
    declared = _header_prototypes()
    assert set(declared) == set(_declared_functions()) and len(declared) == 67       # the two parses agree on what is declared
    assert list(_lib.PROTOTYPES) == _lib.EXPORTS
    assert _prototype_mismatches(declared, _lib.PROTOTYPES) == []
    # spot checks of the parse itself, so that an all-"pointer" reading of both sides could not pass
    assert declared["lg_binning_bytes"] == ("size_t", ["int64", "int32", "int32", "int32"])
    assert declared["lg_profile_reset"] == ("void", []) and declared["lg_last_error"] == ("pointer", [])
    assert declared["lg_prune_epilogue"] == ("int32", ["int32", "pointer", "pointer", "float", "double"] + ["pointer"] * 4 + ["uint32", "pointer"])
    assert declared["lg_compact_rows"][1] == ["int32", "pointer", "int32", "pointer", "pointer", "pointer", "pointer"]


def test_the_prototype_check_reports_a_wrong_table():
    declared, good = _header_prototypes(), dict(_lib.PROTOTYPES)
    ret, args = good["lg_backward_scratch_bytes"]
    assert args == (C.c_int32, C.c_int64)
    widened = dict(good, lg_backward_scratch_bytes=(ret, (C.c_int64, C.c_int64)))                      # int32 -> int64
    bad = _prototype_mismatches(declared, widened)
    assert len(bad) == 1 and bad[0].startswith("lg_backward_scratch_bytes: parameter 0 is int32")
    ret, args = good["lg_densify_rows"]
    bad = _prototype_mismatches(declared, dict(good, lg_densify_rows=(ret, args[:4] + args[5:])))      # a parameter dropped
    assert bad and all(line.startswith("lg_densify_rows:") for line in bad) and "12 parameters, the table has 11" in bad[0]
    swapped = dict(good, lg_vq_nearest=good["lg_vq_ema_step"], lg_vq_ema_step=good["lg_vq_nearest"])   # two entries exchanged
    bad = _prototype_mismatches(declared, swapped)
    assert {line.split(":")[0] for line in bad} == {"lg_vq_nearest", "lg_vq_ema_step"}
    missing = {n: v for n, v in good.items() if n != "lg_forward"}
    assert _prototype_mismatches(declared, missing) == ["lg_forward: declared in the headers, not in the table"]


def _header_constants():
    src = _header_text()
    values = {}
    for body in re.findall(r"enum\s*\{(.*?)\}\s*;", src, flags=re.S):
        members = [m.strip() for m in body.split(",") if m.strip()]
        assert all(re.fullmatch(r"LG_\w+\s*=\s*-?\d+", m) for m in members), members        # every member states its value
        values.update((m.split("=")[0].strip(), int(m.split("=")[1])) for m in members)
    for name, value in re.findall(r"^\s*#\s*define\s+(LG_\w+)\s+(-?\d+)u?\s*$", src, flags=re.M):
        assert name not in values, name
        values[name] = int(value)
    return values


def test_every_constant_of_the_binding_matches_the_headers():
    values = _header_constants()
    assert len(values) == 36 and values["LG_ABI_VERSION"] == 7 and values["LG_ERR_PREFILTERED"] == -4 and values["LG_ADAM_DECOUPLED_WD"] == 1
    for name, value in values.items():
        mine = name if name == "LG_OK" or name.startswith("LG_ERR_") else name[len("LG_"):]
        assert hasattr(_lib, mine), f"{name} has no counterpart _lib.{mine}"
        assert getattr(_lib, mine) == value, f"_lib.{mine} = {getattr(_lib, mine)}, the header says {name} = {value}"
    flags = {n: v for n, v in values.items() if n.startswith("LG_FLAG_")}
    assert len(flags) == 15 and all(v > 0 and v & (v - 1) == 0 for v in flags.values()), flags
    assert len(set(flags.values())) == len(flags), flags
    # every FLAG_* / WEIGHT_* / ... the binding states exists in the header too
    prefixes = ("FLAG_", "WEIGHT_", "LG_ERR_", "ADAM_", "DENSIFY_", "FEATURES_", "FILTER3D_")
    for mine in (n for n in vars(_lib) if n.startswith(prefixes)):
        assert (mine if mine.startswith("LG_") else "LG_" + mine) in values, f"_lib.{mine} is not in the headers"


def _header_structs():
    """name -> [field names in order] of every `typedef struct lg_* { ... } lg_*;`."""
    out = {}
    for name, body in re.findall(r"typedef\s+struct\s+(lg_\w+)\s*\{(.*?)\}\s*\1\s*;", _header_text(), flags=re.S):
        fields = []
        for decl in (d.strip() for d in body.split(";") if d.strip()):
            for part in decl.split(","):
                fields.append(re.fullmatch(r".*?(\w+)\s*(?:\[\s*\d+\s*\])?", part.strip(), flags=re.S).group(1))
        out[name] = fields
    return out


def test_every_struct_of_the_binding_has_the_layout_the_compiler_gives_the_header(tmp_path):
    import subprocess
    structs = _header_structs()
    mirrors = {n: t for n, t in vars(_lib).items() if isinstance(t, type) and issubclass(t, C.Structure) and t is not C.Structure}
    assert set(structs) == set(mirrors) and len(structs) == 8
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "lightgaussian_debug.h"', "int main(void) {"]
    for name, fields in structs.items():
        assert fields == [f[0] for f in mirrors[name]._fields_], name
        lines.append(f'    printf("{name} sizeof %zu\\n", sizeof({name}));')
        lines += [f'    printf("{name} {f} %zu\\n", offsetof({name}, {f}));' for f in fields]
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "abi_layout.cpp", tmp_path / "abi_layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(common.ROOT, "include"), str(src), "-o", str(exe)])
    measured = [line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()]
    assert len(measured) == sum(len(f) + 1 for f in structs.values())
    for name, what, value in measured:
        mine = C.sizeof(mirrors[name]) if what == "sizeof" else getattr(mirrors[name], what).offset
        assert mine == int(value), f"{name} {what}: ctypes {mine}, the compiler {value}"
    assert C.sizeof(_lib.lg_filter_camera) == 80 and C.sizeof(_lib.lg_adam_rows_tensor) == C.sizeof(_lib.lg_adam_tensor) + 16
