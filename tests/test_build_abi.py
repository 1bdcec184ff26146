"""The build header (include/rrte_hip_build.h) across its bindings, checked without a GPU: the record's
size and field offsets from a C program compiled against the header equal the ctypes struct and the
Rust repr(C) struct (rust/rrte-hip-sys/src/build.rs); the header's functions are abi.BUILD_EXPORTS and
build.rs's extern block with the same signatures, and the library exports them; no name is shared
with another export set, the other headers know nothing of it, and the device code's identity
(abi.build_id) is the one it had before the build policy existed."""
import ctypes as C
import re
import subprocess
from pathlib import Path

from test_rust_binding import _c_param, _rust_type, _split_top, rust_layout, rust_structs

from rrte_amd import abi

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "rrte_hip_build.h"
BUILD_RS = ROOT / "rust" / "rrte-hip-sys" / "src" / "build.rs"
FIELDS = ["device_builds", "host_fallbacks", "policy", "depth"]
OFFSETS = {"device_builds": 0, "host_fallbacks": 8, "policy": 16, "depth": 20}
FUNCTIONS = {"rrte_hip_set_mesh_build", "rrte_hip_build_info"}
# rrte_hip_build_id of the device code as committed: whoever edits an embedded device header (the
# Makefile's DEVICE_HDR: ray_kernels.hpp and the headers under it, device_scene.hpp, search_groups.hpp,
# rrte_hip.h) moves it knowingly (the JIT caches and the committed counter profiles go stale with it).
# The header of this file left it at 027c2cd794e4ea10a4daf2982fd7a101; the edge-case ray bank moved it:
# leaves_sphere bounded by hb < 2^63, the culls and the mesh walk standing down (a37e396d93f8eadcea26e8ff40191b25).
# The split of ray_kernels.hpp into layered headers moved it: the same kernels from another hashed text.
PINNED_BUILD_ID = "827928e4f1af32f488444308c4ead015"


def _header_text():
    return re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)


def _rust_text():
    return re.sub(r"//[^\n]*", "", BUILD_RS.read_text())


def _header_functions():
    return {name: ("i32", [_c_param(a) for a in _split_top(args)])
            for name, args in re.findall(r"^rrte_status\s+(rrte_hip_\w+)\((.*?)\);", _header_text(), re.S | re.M)}


def test_record_layout_agrees_across_the_bindings(tmp_path):
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {",
             'printf("rrte_build_info %zu\\n", sizeof(rrte_build_info));',
             'printf("HOST %u\\nDEVICE %u\\n", RRTE_MESH_BUILD_HOST, RRTE_MESH_BUILD_DEVICE);']
    lines += [f'printf("{f} %zu\\n", offsetof(rrte_build_info, {f}));' for f in FIELDS]
    lines += ["return 0; }"]
    src, exe = tmp_path / "build_layout.c", tmp_path / "build_layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    c = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    rs = rust_structs(_rust_text())
    assert set(rs) == {"rrte_build_info"}
    size, _, offs = rust_layout(rs)["rrte_build_info"]
    assert c["rrte_build_info"] == 24 == C.sizeof(abi.BuildInfo) == size
    assert [f for f, _ in abi.BuildInfo._fields_] == FIELDS == [f for f, _ in rs["rrte_build_info"]]
    for f, off in offs:
        assert c[f] == getattr(abi.BuildInfo, f).offset == off == OFFSETS[f], f
    assert [t for _, t in rs["rrte_build_info"]] == ["u64", "u64", "u32", "u32"]
    assert re.search(r"\}\s*rrte_build_info;\s*/\*\s*24 bytes", HEADER.read_text())
    assert (c["HOST"], c["DEVICE"]) == (0, 1) == (abi.MESH_BUILD_HOST, abi.MESH_BUILD_DEVICE)
    consts = dict(re.findall(r"pub const (RRTE_MESH_BUILD_\w+): u32 = (\d+);", _rust_text()))
    assert consts == {"RRTE_MESH_BUILD_HOST": "0", "RRTE_MESH_BUILD_DEVICE": "1"}


def test_the_functions_are_bound_with_the_same_signatures():
    hf = _header_functions()
    assert set(hf) == FUNCTIONS == set(abi.BUILD_EXPORTS)
    block = re.search(r'extern "C" \{(.*?)\n\}', _rust_text(), re.S).group(1)
    rf = {name: (_rust_type(ret) if ret else "void", [_rust_type(a.split(":", 1)[1]) for a in _split_top(args)])
          for name, args, ret in re.findall(r"pub fn (\w+)\((.*?)\)\s*(?:->\s*([^;]+))?;", block, re.S)}
    assert rf == hf
    assert hf["rrte_hip_set_mesh_build"][1] == ["*rrte_ctx", "u32"]
    assert hf["rrte_hip_build_info"][1] == ["*rrte_ctx", "*rrte_build_info"]
    res, args = abi.BUILD_EXPORTS["rrte_hip_set_mesh_build"]
    assert res is C.c_int and args == [C.c_void_p, C.c_uint32]
    res, args = abi.BUILD_EXPORTS["rrte_hip_build_info"]
    assert res is C.c_int and args[0] is C.c_void_p and args[1]._type_ is abi.BuildInfo
    lib_rs = (ROOT / "rust" / "rrte-hip-sys" / "src" / "lib.rs").read_text()
    assert "pub mod build;" in lib_rs and "rrte_hip_set_mesh_build" not in lib_rs
    # the safe wrappers call the FFI with the declared arity
    text = re.sub(r"pub fn rrte_hip_\w+\(", "pub fn X(", _rust_text())
    for name, (_, params) in hf.items():
        calls = re.findall(r"\b%s\(((?:[^()]|\([^()]*\))*)\)" % name, text)
        assert calls and all(len(_split_top(a)) == len(params) for a in calls), name


def test_library_exports_the_symbols():
    lib = abi.load()
    for name in abi.BUILD_EXPORTS:
        assert hasattr(lib, name), name
    info = abi.BuildInfo()
    assert lib.rrte_hip_set_mesh_build(None, abi.MESH_BUILD_DEVICE) == abi.RRTE_INVALID_ARG
    assert lib.rrte_hip_build_info(None, C.byref(info)) == abi.RRTE_INVALID_ARG


def test_no_name_is_shared_and_the_other_headers_are_unchanged():
    import test_mesh_abi
    lib = abi.load()
    assert lib.rrte_hip_abi_version() == 2 == abi.ABI_VERSION
    render_text = re.sub(r"/\*.*?\*/", "", test_mesh_abi.RENDER_HEADER.read_text(), flags=re.S)
    assert set(re.findall(r"\b(rrte_hip_\w+)\s*\(", render_text)) == test_mesh_abi.RENDER_FUNCTIONS == set(abi.EXPORTS)
    others = [abi.EXPORTS, abi.QUERY_EXPORTS, abi.MESH_EXPORTS, abi.REFIT_EXPORTS, abi.JIT_EXPORTS]
    for other in others:
        assert not set(abi.BUILD_EXPORTS) & set(other)
    assert set(abi.MESH_EXPORTS) == {"rrte_hip_mesh_info"}
    assert set(abi.REFIT_EXPORTS) == {"rrte_hip_mesh_refit", "rrte_hip_refit_info", "rrte_hip_mesh_nodes", "rrte_hip_mesh_slots"}
    for h in ("rrte_hip.h", "rrte_hip_query.h", "rrte_hip_mesh.h", "rrte_hip_refit.h", "rrte_hip_jit.h"):
        text = (ROOT / "include" / h).read_text()
        assert "mesh_build" not in text and "build_info" not in text and "MESH_BUILD" not in text, h
    assert '#include "rrte_hip.h"' in HEADER.read_text()


def test_the_device_code_identity_is_the_pinned_one():
    assert abi.build_id() == PINNED_BUILD_ID
