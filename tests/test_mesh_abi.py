"""The mesh header (include/rrte_hip_mesh.h) and the RRTE_PRIM_MESH_INSTANCE constant across their
bindings, checked without a GPU: the record's size and field offsets from a C program compiled
against the header equal the ctypes struct and the Rust repr(C) struct (rust/rrte-hip-sys/src/mesh.rs);
the function is in abi.MESH_EXPORTS and in mesh.rs's extern block with the same signature, and the
library exports it; the render ABI (rrte_hip.h's function set, RRTE_ABI_VERSION) is unchanged."""
import ctypes as C
import re
import subprocess
from pathlib import Path

from test_rust_binding import _c_consts, _c_param, _rust_type, _split_top, rust_layout, rust_structs

from rrte_amd import abi

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "rrte_hip_mesh.h"
RENDER_HEADER = ROOT / "include" / "rrte_hip.h"
MESH_RS = ROOT / "rust" / "rrte-hip-sys" / "src" / "mesh.rs"
FIELDS = ["bvh_builds", "ranges", "tri_slots", "bvh_nodes", "_pad"]

# rrte_hip.h's entry points as they were before mesh instances: the render ABI keeps exactly these
RENDER_FUNCTIONS = {
    "rrte_hip_abi_version", "rrte_hip_create", "rrte_hip_destroy", "rrte_hip_last_error", "rrte_hip_render",
    "rrte_hip_render_f32", "rrte_hip_render_async", "rrte_hip_synchronize", "rrte_hip_query", "rrte_hip_stats",
    "rrte_hip_set_jit", "rrte_hip_jit_check", "rrte_hip_fpcheck", "rrte_hip_sdf_guards", "rrte_hip_tile_order_plan",
    "rrte_hip_build_id", "rrte_hip_jit_cache_key", "rrte_hip_check_word", "rrte_hip_scene_dump", "rrte_hip_scene_load",
    "rrte_hip_scene_free", "rrte_hip_comm_unique_id", "rrte_hip_comm_init", "rrte_hip_render_gather",
    "rrte_hip_render_gather_async", "rrte_hip_set_comm_timeout", "rrte_hip_set_gather_batch", "rrte_hip_flush",
    "rrte_hip_gather_info", "rrte_hip_host_register", "rrte_hip_host_unregister", "rrte_hip_band_rows_for_rank",
    "rrte_hip_band_layout", "rrte_hip_band_rows_for_rank_ex"}


def _header_text():
    return re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)


def _rust_text():
    return re.sub(r"//[^\n]*", "", MESH_RS.read_text())


def test_record_layout_agrees_across_the_bindings(tmp_path):
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {",
             'printf("rrte_mesh_info %zu\\n", sizeof(rrte_mesh_info));']
    lines += [f'printf("{f} %zu\\n", offsetof(rrte_mesh_info, {f}));' for f in FIELDS]
    lines += ['printf("kind %d\\n", (int)RRTE_PRIM_MESH_INSTANCE);', "return 0; }"]
    src, exe = tmp_path / "mesh_layout.c", tmp_path / "mesh_layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    c = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    rs = rust_structs(_rust_text())
    assert set(rs) == {"rrte_mesh_info"}
    size, _, offs = rust_layout(rs)["rrte_mesh_info"]
    assert c["rrte_mesh_info"] == 24 == C.sizeof(abi.MeshInfo) == size
    assert [f for f, _ in abi.MeshInfo._fields_] == FIELDS == [f for f, _ in rs["rrte_mesh_info"]]
    for f, off in offs:
        assert c[f] == getattr(abi.MeshInfo, f).offset == off, f
    assert dict(rs["rrte_mesh_info"])["bvh_builds"] == "u64" and abi.MeshInfo.bvh_builds.size == 8
    assert re.search(r"\}\s*rrte_mesh_info;\s*/\*\s*24 bytes", HEADER.read_text())
    # the constant: C enum, Python, Rust
    assert c["kind"] == 9 == abi.PRIM_MESH_INSTANCE == _c_consts()["RRTE_PRIM_MESH_INSTANCE"]
    assert re.findall(r"pub const (RRTE_\w+): u32 = (\d+);", _rust_text()) == [("RRTE_PRIM_MESH_INSTANCE", "9")]
    assert abi.PRIM_MESH == 8 and _c_consts()["RRTE_PRIM_MESH"] == 8


def test_the_function_is_bound_with_the_same_signature():
    hf = {name: ("i32", [_c_param(a) for a in _split_top(args)])
          for name, args in re.findall(r"^rrte_status\s+(rrte_hip_\w+)\((.*?)\);", _header_text(), re.S | re.M)}
    assert set(hf) == {"rrte_hip_mesh_info"} == set(abi.MESH_EXPORTS)
    block = re.search(r'extern "C" \{(.*?)\n\}', _rust_text(), re.S).group(1)
    rf = {name: (_rust_type(ret) if ret else "void", [_rust_type(a.split(":", 1)[1]) for a in _split_top(args)])
          for name, args, ret in re.findall(r"pub fn (\w+)\((.*?)\)\s*(?:->\s*([^;]+))?;", block, re.S)}
    assert rf == hf
    res, args = abi.MESH_EXPORTS["rrte_hip_mesh_info"]
    assert res is C.c_int and args[0] is C.c_void_p and args[1]._type_ is abi.MeshInfo
    assert hf["rrte_hip_mesh_info"][1] == ["*rrte_ctx", "*rrte_mesh_info"]
    lib_rs = (ROOT / "rust" / "rrte-hip-sys" / "src" / "lib.rs").read_text()
    assert "pub mod mesh;" in lib_rs and "RRTE_PRIM_MESH_INSTANCE" not in lib_rs and "rrte_hip_mesh_info" not in lib_rs
    # the safe wrapper calls the FFI with the declared arity
    text = re.sub(r"pub fn rrte_hip_\w+\(", "pub fn X(", _rust_text())
    calls = re.findall(r"\brrte_hip_mesh_info\(([^()]*)\)", text)
    assert calls and all(len(_split_top(a)) == 2 for a in calls)


def test_library_exports_the_symbol():
    lib = abi.load()
    assert hasattr(lib, "rrte_hip_mesh_info")
    assert lib.rrte_hip_mesh_info(None, None) == abi.RRTE_INVALID_ARG
    info = abi.MeshInfo()
    assert lib.rrte_hip_mesh_info(None, C.byref(info)) == abi.RRTE_INVALID_ARG


def test_render_abi_is_unchanged():
    lib = abi.load()
    assert lib.rrte_hip_abi_version() == 2 == abi.ABI_VERSION
    assert re.search(r"#define RRTE_ABI_VERSION 2u", RENDER_HEADER.read_text())
    render_text = re.sub(r"/\*.*?\*/", "", RENDER_HEADER.read_text(), flags=re.S)
    assert set(re.findall(r"\b(rrte_hip_\w+)\s*\(", render_text)) == RENDER_FUNCTIONS == set(abi.EXPORTS)
    assert not set(abi.MESH_EXPORTS) & (set(abi.EXPORTS) | set(abi.QUERY_EXPORTS))
    assert "rrte_mesh_info" not in render_text
    assert '#include "rrte_hip.h"' in HEADER.read_text()
