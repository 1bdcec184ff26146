"""The frame-AOV boundary (include/rrte_hip_aov.h) across its bindings, checked without a GPU: record
sizes and field offsets from a C program compiled against the header equal the ctypes structs and the
Rust repr(C) structs (rust/rrte-hip-sys/src/aov.rs); every function of the header is in
abi.AOV_EXPORTS and in aov.rs's extern block with the same signature, and the library exports it; the
render ABI is unchanged; and the structural promises of the kernel sources that can be read without
running anything."""
import ctypes as C
import re
import subprocess
from pathlib import Path

from test_rust_binding import _c_param, _rust_type, _split_top, rust_layout, rust_structs

from rrte_amd import abi

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "rrte_hip_aov.h"
RENDER_HEADER = ROOT / "include" / "rrte_hip.h"
AOV_RS = ROOT / "rust" / "rrte-hip-sys" / "src" / "aov.rs"
CSRC = ROOT / "rrte_amd" / "csrc"

DESC_FIELDS = ["planes", "x0", "y0", "width", "height", "_pad"]
BUF_FIELDS = ["depth", "prim", "material", "tri", "normal", "position", "albedo", "_reserved"]
RECORDS = {"rrte_aov_desc": (DESC_FIELDS, 32, abi.AovDesc), "rrte_aov_buffers": (BUF_FIELDS, 64, abi.AovBuffers)}
FUNCTIONS = {"rrte_hip_render_aov", "rrte_hip_render_aov_async"}
CONSTANTS = {"RRTE_AOV_DEPTH": 1, "RRTE_AOV_PRIM": 2, "RRTE_AOV_MATERIAL": 4, "RRTE_AOV_TRI": 8, "RRTE_AOV_NORMAL": 16,
             "RRTE_AOV_POSITION": 32, "RRTE_AOV_ALBEDO": 64, "RRTE_AOV_ALL": 127}


def _header_text():
    return re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)


def _rust_text():
    return re.sub(r"//[^\n]*", "", AOV_RS.read_text())


def c_layout(tmp_path):
    """{record: size, record.field: offset} from a C program compiled with the header."""
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {"]
    for name, (fields, _, _) in RECORDS.items():
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f in fields]
    lines.append("return 0; }")
    src = tmp_path / "aov_layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "aov_layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def header_functions():
    out = {}
    for name, args in re.findall(r"^rrte_status\s+(rrte_hip_\w+)\((.*?)\);", _header_text(), re.S | re.M):
        out[name] = ("i32", [_c_param(a) for a in _split_top(args)])
    return out


def test_struct_sizes():
    assert C.sizeof(abi.AovDesc) == 32 and C.sizeof(abi.AovBuffers) == 64
    text = HEADER.read_text()
    for name, (_, size, _) in RECORDS.items():
        assert re.search(r"\}\s*" + name + r";\s*/\*\s*" + str(size) + " bytes", text), name


def test_field_offsets_agree_across_the_bindings(tmp_path):
    c = c_layout(tmp_path)
    rs = {k: v for k, v in rust_structs(_rust_text()).items() if k.startswith("rrte_")}
    assert set(rs) == set(RECORDS)
    lay = rust_layout(rs)
    for name, (fields, size, ct) in RECORDS.items():
        assert c[name] == size == C.sizeof(ct) == lay[name][0]
        assert [f for f, _ in ct._fields_] == fields == [f for f, _ in rs[name]]
        for f, off in lay[name][2]:
            assert c[f"{name}.{f}"] == getattr(ct, f).offset == off, (name, f)
    # the same element kinds: signed ids, an unsigned triangle index, floats elsewhere
    want = {"depth": ("*mut f32", C.c_float), "prim": ("*mut i32", C.c_int32), "material": ("*mut i32", C.c_int32),
            "tri": ("*mut u32", C.c_uint32), "normal": ("*mut f32", C.c_float), "position": ("*mut f32", C.c_float),
            "albedo": ("*mut f32", C.c_float)}
    ctf = dict(abi.AovBuffers._fields_)
    for f, (rust_t, ctype) in want.items():
        assert dict(rs["rrte_aov_buffers"])[f] == rust_t and ctf[f]._type_ is ctype, f
    assert dict(rs["rrte_aov_desc"])["_pad"] == "[u32; 3]"


def test_constants_agree():
    cv = {k: int(v, 16) for k, v in re.findall(r"#define (RRTE_AOV_\w+)\s+0x([0-9A-Fa-f]+)u\b", HEADER.read_text())}
    assert cv == CONSTANTS
    rv = {k: int(v) for k, v in re.findall(r"pub const (RRTE_AOV_\w+): u32 = (\d+);", _rust_text())}
    assert rv == cv
    assert (abi.AOV_DEPTH, abi.AOV_PRIM, abi.AOV_MATERIAL, abi.AOV_TRI, abi.AOV_NORMAL, abi.AOV_POSITION, abi.AOV_ALBEDO,
            abi.AOV_ALL) == (1, 2, 4, 8, 16, 32, 64, 127)
    # the plane table: a name per field of rrte_aov_buffers, in bit order
    assert list(abi.AOV_PLANES) == BUF_FIELDS[:-1]
    assert [b for b, _, _ in abi.AOV_PLANES.values()] == [1 << k for k in range(7)]


_CTYPES = {C.c_int: "i32", C.c_uint32: "u32", C.c_void_p: "void*"}


def _ctypes_param(t):
    """A ctypes argument type in the canonical form of _c_param, up to constness (ctypes has none)."""
    if t in _CTYPES:
        return _CTYPES[t]
    names = {abi.SceneIR: "rrte_scene_ir", abi.RenderParams: "rrte_render_params", abi.AovDesc: "rrte_aov_desc",
             abi.AovBuffers: "rrte_aov_buffers"}
    return "*" + names[t._type_]


def test_every_function_is_bound_with_the_same_signature():
    hf = header_functions()
    assert set(hf) == FUNCTIONS
    block = re.search(r'extern "C" \{(.*?)\n\}', _rust_text(), re.S).group(1)
    rf = {}
    for name, args, ret in re.findall(r"pub fn (\w+)\((.*?)\)\s*(?:->\s*([^;]+))?;", block, re.S):
        rf[name] = (_rust_type(ret) if ret else "void", [_rust_type(a.split(":", 1)[1]) for a in _split_top(args)])
    assert set(rf) == set(hf)
    for name in hf:
        assert rf[name] == hf[name], f"{name}: Rust {rf[name]} != C {hf[name]}"
    assert set(abi.AOV_EXPORTS) == set(hf)
    for name, (ret, params) in hf.items():
        res, args = abi.AOV_EXPORTS[name]
        assert res is C.c_int and len(args) == len(params), name
        for a, p in zip(args, params):
            want = p.replace("const*", "*")
            want = "void*" if want in ("*rrte_ctx", "*void") else want
            assert _ctypes_param(a) == want, (name, p)
    # the safe wrapper calls the FFI with the declared arity
    text = re.sub(r"pub fn rrte_hip_\w+\(", "pub fn X(", _rust_text())
    calls = []
    for m in re.finditer(r"\b(rrte_hip_\w+)\(", text):
        depth, i = 1, m.end()
        while depth and i < len(text):
            depth += {"(": 1, ")": -1}.get(text[i], 0)
            i += 1
        calls.append((m.group(1), len(_split_top(text[m.end():i - 1]))))
    assert {n for n, _ in calls} == {"rrte_hip_render_aov"}
    for name, n in calls:
        assert n == len(hf[name][1]), name
    # the safe wrapper sizes its vectors as the library reads the desc: all zero is the whole frame
    assert "(x0 | y0 | width | height) == 0" in _rust_text() and "rect.is_some()" not in _rust_text()
    assert "pub mod aov;" in (ROOT / "rust" / "rrte-hip-sys" / "src" / "lib.rs").read_text()


def test_library_exports_the_aov_symbols():
    lib = abi.load()
    for name in FUNCTIONS:
        assert hasattr(lib, name), name
    # a null context is refused on the host, without a device
    assert lib.rrte_hip_render_aov(None, None, None, None, None) == abi.RRTE_INVALID_ARG
    assert lib.rrte_hip_render_aov_async(None, None, None, None, None, None) == abi.RRTE_INVALID_ARG
    desc, bufs = abi.AovDesc(planes=abi.AOV_DEPTH), abi.AovBuffers()
    assert lib.rrte_hip_render_aov(None, None, None, C.byref(desc), C.byref(bufs)) == abi.RRTE_INVALID_ARG


def test_render_abi_is_unchanged():
    lib = abi.load()
    assert lib.rrte_hip_abi_version() == 2 == abi.ABI_VERSION
    assert re.search(r"#define RRTE_ABI_VERSION 2u?\b", RENDER_HEADER.read_text())
    others = {k: v for k, v in vars(abi).items() if k.endswith("EXPORTS") and k != "AOV_EXPORTS"}
    assert len(others) >= 8 and "EXPORTS" in others and "QUERY_EXPORTS" in others
    for k, other in others.items():
        assert not set(abi.AOV_EXPORTS) & set(other), k
    # rrte_hip.h's function set is still abi.EXPORTS
    render_text = re.sub(r"/\*.*?\*/", "", RENDER_HEADER.read_text(), flags=re.S)
    declared = set(re.findall(r"^(?:rrte_status|uint32_t|void|const char\*)\s+(rrte_hip_\w+)\(", render_text, re.M))
    assert declared == set(abi.EXPORTS)
    for name in abi.AOV_EXPORTS:
        assert name not in render_text
    assert '#include "rrte_hip.h"' in HEADER.read_text()


def _make_list(name):
    out = subprocess.run(["make", "-s", "--no-print-directory", "-C", str(CSRC), name], check=True, capture_output=True,
                         text=True).stdout
    return out.split()


def _code(path):
    """A source file without its comments."""
    return re.sub(r"//[^\n]*|/\*.*?\*/", "", path.read_text(), flags=re.S)


def test_structural_promises_of_the_sources():
    """What can be read from aov.hip and aov_kernels.hpp without running anything."""
    assert "aov.hip" in _make_list("print-src")
    device_hdr = [Path(h).name for h in _make_list("print-device-hdr")]
    assert "aov_kernels.hpp" not in device_hdr and "ray_query.hpp" not in device_hdr
    # host-TU only: no embedded header includes it, and only aov.hip does at all
    users = [p.name for p in sorted(CSRC.glob("*.h*")) if '"aov_kernels.hpp"' in _code(p)]
    assert users == ["aov.hip"]
    kern, host = _code(CSRC / "aov_kernels.hpp"), _code(CSRC / "aov.hip")
    # the search is the one shared body, over both object loops
    assert kern.count("closest_hit_search(") == 1 and "visit_all(" in kern and "visit_candidates(" in kern
    query = _code(CSRC / "ray_query.hpp")
    assert query.count("closest_hit_search(") == 2  # its definition and ray_query_kernel's call
    assert _code(CSRC / "accel_kernels.hpp").count("closest_hit_search(") == 1
    # one wave per workgroup; idle lanes stay in the wave: no return in the body, the stores behind `live`
    assert "kBlockThreads == 64u" in kern and "__launch_bounds__(kBlockThreads)" in kern
    tile = kern[kern.index("void aov_tile("):kern.index("__global__")]
    assert not re.search(r"\breturn\b", tile) and "if (live)" in tile
    # no LDS staging, no atomics, no inline assembly
    assert not re.search(r"__shared__|\batomic\w*\s*\(|\basm\b|__syncthreads", kern)
    # the five feature variants of launch_query plus the accelerated one
    assert re.findall(r"aov_kernel<(\w+)>", kern) == ["0u", "kFeatAnalytic", "kFeatSdf", "kFeatAll", "kFeatEvery"]
    assert "aov_accel_kernel" in kern and "c->accel_on" in host
    # both forms take the scene through query_scene, and the staging buffer is a context-owned DeviceBuf
    assert len(re.findall(r"\bquery_scene\(c, s,", host)) == 2
    assert "ensure(c, c->d_aov" in host and "kQueryChunk" in host
    assert not re.search(r"\bhip(Malloc|Free)\w*\(", host)
    assert "DeviceBuf<uint8_t> d_aov" in _code(CSRC / "context.hpp")
