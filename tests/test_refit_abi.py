"""The refit header (include/rrte_hip_refit.h) across its bindings, checked without a GPU: the record's
size and field offsets from a C program compiled against the header equal the ctypes struct and the
Rust repr(C) struct (rust/rrte-hip-sys/src/refit.rs); the header's functions are abi.REFIT_EXPORTS and
refit.rs's extern block with the same signatures, and the library exports them; the other headers'
function sets and RRTE_ABI_VERSION are unchanged."""
import ctypes as C
import re
import subprocess
from pathlib import Path

from test_rust_binding import _c_param, _rust_type, _split_top, rust_layout, rust_structs

from rrte_amd import abi

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "rrte_hip_refit.h"
REFIT_RS = ROOT / "rust" / "rrte-hip-sys" / "src" / "refit.rs"
FIELDS = ["refits", "device_refits", "levels", "deformed"]
OFFSETS = {"refits": 0, "device_refits": 8, "levels": 16, "deformed": 20}
# what the issue names; a read-back of the slot table sits beside them for the box checker
REQUIRED = {"rrte_hip_mesh_refit", "rrte_hip_refit_info", "rrte_hip_mesh_nodes"}


def _header_text():
    return re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)


def _rust_text():
    return re.sub(r"//[^\n]*", "", REFIT_RS.read_text())


def _header_functions():
    return {name: ("i32", [_c_param(a) for a in _split_top(args)])
            for name, args in re.findall(r"^rrte_status\s+(rrte_hip_\w+)\((.*?)\);", _header_text(), re.S | re.M)}


def test_record_layout_agrees_across_the_bindings(tmp_path):
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {",
             'printf("rrte_refit_info %zu\\n", sizeof(rrte_refit_info));']
    lines += [f'printf("{f} %zu\\n", offsetof(rrte_refit_info, {f}));' for f in FIELDS]
    lines += ["return 0; }"]
    src, exe = tmp_path / "refit_layout.c", tmp_path / "refit_layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    c = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    rs = rust_structs(_rust_text())
    assert set(rs) == {"rrte_refit_info"}
    size, _, offs = rust_layout(rs)["rrte_refit_info"]
    assert c["rrte_refit_info"] == 24 == C.sizeof(abi.RefitInfo) == size
    assert [f for f, _ in abi.RefitInfo._fields_] == FIELDS == [f for f, _ in rs["rrte_refit_info"]]
    for f, off in offs:
        assert c[f] == getattr(abi.RefitInfo, f).offset == off == OFFSETS[f], f
    assert [t for _, t in rs["rrte_refit_info"]] == ["u64", "u64", "u32", "u32"]
    assert re.search(r"\}\s*rrte_refit_info;\s*/\*\s*24 bytes", HEADER.read_text())


def test_the_functions_are_bound_with_the_same_signatures():
    hf = _header_functions()
    assert REQUIRED <= set(hf) and set(hf) == set(abi.REFIT_EXPORTS)
    block = re.search(r'extern "C" \{(.*?)\n\}', _rust_text(), re.S).group(1)
    rf = {name: (_rust_type(ret) if ret else "void", [_rust_type(a.split(":", 1)[1]) for a in _split_top(args)])
          for name, args, ret in re.findall(r"pub fn (\w+)\((.*?)\)\s*(?:->\s*([^;]+))?;", block, re.S)}
    assert rf == hf
    assert hf["rrte_hip_mesh_refit"][1] == ["*rrte_ctx", "const*rrte_scene_ir"]
    assert hf["rrte_hip_refit_info"][1] == ["*rrte_ctx", "*rrte_refit_info"]
    assert hf["rrte_hip_mesh_nodes"][1] == ["*rrte_ctx", "*void", "usize", "*u32"]
    res, args = abi.REFIT_EXPORTS["rrte_hip_mesh_refit"]
    assert res is C.c_int and args[0] is C.c_void_p and args[1]._type_ is abi.SceneIR
    res, args = abi.REFIT_EXPORTS["rrte_hip_refit_info"]
    assert res is C.c_int and args[1]._type_ is abi.RefitInfo
    res, args = abi.REFIT_EXPORTS["rrte_hip_mesh_nodes"]
    assert res is C.c_int and args[1:] == [C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)]
    lib_rs = (ROOT / "rust" / "rrte-hip-sys" / "src" / "lib.rs").read_text()
    assert "pub mod refit;" in lib_rs and "rrte_hip_mesh_refit" not in lib_rs
    # the safe wrappers call the FFI with the declared arity
    text = re.sub(r"pub fn rrte_hip_\w+\(", "pub fn X(", _rust_text())
    for name, (_, params) in hf.items():
        calls = re.findall(r"\b%s\(((?:[^()]|\([^()]*\))*)\)" % name, text)
        assert calls and all(len(_split_top(a)) == len(params) for a in calls), name


def test_library_exports_the_symbols():
    lib = abi.load()
    for name in abi.REFIT_EXPORTS:
        assert hasattr(lib, name), name
    info, n = abi.RefitInfo(), C.c_uint32()
    assert lib.rrte_hip_mesh_refit(None, None) == abi.RRTE_INVALID_ARG
    assert lib.rrte_hip_refit_info(None, C.byref(info)) == abi.RRTE_INVALID_ARG
    assert lib.rrte_hip_mesh_nodes(None, None, 0, C.byref(n)) == abi.RRTE_INVALID_ARG
    assert lib.rrte_hip_mesh_slots(None, None, 0, C.byref(n)) == abi.RRTE_INVALID_ARG


def test_the_other_headers_are_unchanged():
    import test_mesh_abi
    lib = abi.load()
    assert lib.rrte_hip_abi_version() == 2 == abi.ABI_VERSION
    render_text = re.sub(r"/\*.*?\*/", "", test_mesh_abi.RENDER_HEADER.read_text(), flags=re.S)
    assert set(re.findall(r"\b(rrte_hip_\w+)\s*\(", render_text)) == test_mesh_abi.RENDER_FUNCTIONS == set(abi.EXPORTS)
    others = set(abi.EXPORTS) | set(abi.QUERY_EXPORTS) | set(abi.MESH_EXPORTS)
    assert not set(abi.REFIT_EXPORTS) & others
    assert set(abi.MESH_EXPORTS) == {"rrte_hip_mesh_info"}
    for h in ("rrte_hip.h", "rrte_hip_query.h", "rrte_hip_mesh.h"):
        assert "refit" not in (ROOT / "include" / h).read_text()
    assert '#include "rrte_hip.h"' in HEADER.read_text()
