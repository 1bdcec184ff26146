"""The ray-query boundary (include/rrte_hip_query.h) across its bindings, checked without a GPU:
record sizes and field offsets from a C program compiled against the header equal the ctypes
structs, the numpy dtypes and the Rust repr(C) structs (rust/rrte-hip-sys/src/query.rs); every
function of the header is in abi.QUERY_EXPORTS and in query.rs's extern block with the same
signature, and the library exports it; the render ABI is unchanged."""
import ctypes as C
import re
import subprocess
from pathlib import Path

from test_rust_binding import _c_param, _rust_type, _split_top, rust_layout, rust_structs

from rrte_amd import abi

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "rrte_hip_query.h"
RENDER_HEADER = ROOT / "include" / "rrte_hip.h"
QUERY_RS = ROOT / "rust" / "rrte-hip-sys" / "src" / "query.rs"

RAY_FIELDS = ["origin", "t_min", "direction", "t_max"]
HIT_FIELDS = ["t", "prim", "point", "normal", "front_face", "tri", "material", "_pad"]
RECORDS = {"rrte_ray": (RAY_FIELDS, 32), "rrte_ray_hit": (HIT_FIELDS, 48)}


def _header_text():
    return re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)


def _rust_text():
    return re.sub(r"//[^\n]*", "", QUERY_RS.read_text())


def c_layout(tmp_path):
    """{record: size, record.field: offset} from a C program compiled with the header."""
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {"]
    for name, (fields, _) in RECORDS.items():
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f in fields]
    lines.append("return 0; }")
    src = tmp_path / "query_layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "query_layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def header_functions():
    out = {}
    for name, args in re.findall(r"^rrte_status\s+(rrte_hip_\w+)\((.*?)\);", _header_text(), re.S | re.M):
        out[name] = ("i32", [_c_param(a) for a in _split_top(args)])
    return out


def test_struct_sizes():
    assert C.sizeof(abi.Ray) == 32 and C.sizeof(abi.RayHit) == 48
    assert abi.RAY_DTYPE.itemsize == 32 and abi.RAY_HIT_DTYPE.itemsize == 48
    text = HEADER.read_text()
    for name, (_, size) in RECORDS.items():
        assert re.search(r"\}\s*" + name + r";\s*/\*\s*" + str(size) + " bytes", text), name


def test_field_offsets_agree_across_the_bindings(tmp_path):
    c = c_layout(tmp_path)
    rs = rust_structs(_rust_text())
    assert set(rs) == set(RECORDS)
    lay = rust_layout(rs)
    for name, ct, dt in (("rrte_ray", abi.Ray, abi.RAY_DTYPE), ("rrte_ray_hit", abi.RayHit, abi.RAY_HIT_DTYPE)):
        fields, size = RECORDS[name]
        assert c[name] == size == C.sizeof(ct) == dt.itemsize == lay[name][0]
        assert [f for f, _ in ct._fields_] == fields == list(dt.names) == [f for f, _ in rs[name]]
        for f, off in lay[name][2]:
            assert c[f"{name}.{f}"] == getattr(ct, f).offset == dt.fields[f][1] == off, (name, f)
    # the same scalar kinds: a signed object index and material, unsigned flags, floats elsewhere
    assert abi.RAY_HIT_DTYPE["prim"] == "<i4" and abi.RAY_HIT_DTYPE["material"] == "<i4"
    assert dict(rs["rrte_ray_hit"])["prim"] == "i32" and dict(rs["rrte_ray_hit"])["material"] == "i32"
    assert abi.RayHit.prim.size == 4 and abi.RayHit(prim=-1).prim == -1


def test_constants_agree():
    cv = {k: int(v) for k, v in re.findall(r"#define (RRTE_QUERY_\w+)\s+(\d+)u\b", HEADER.read_text())}
    assert cv == {"RRTE_QUERY_CLOSEST": 0, "RRTE_QUERY_ANY": 1}
    rv = {k: int(v) for k, v in re.findall(r"pub const (RRTE_QUERY_\w+): u32 = (\d+);", _rust_text())}
    assert rv == cv
    assert (abi.QUERY_CLOSEST, abi.QUERY_ANY) == (0, 1)


_CTYPES = {C.c_int: "i32", C.c_uint32: "u32", C.c_void_p: "void*"}


def _ctypes_param(t):
    """A ctypes argument type in the canonical form of _c_param, up to constness (ctypes has none)."""
    if t in _CTYPES:
        return _CTYPES[t]
    names = {abi.SceneIR: "rrte_scene_ir", abi.RenderParams: "rrte_render_params", abi.Ray: "rrte_ray",
             abi.RayHit: "rrte_ray_hit", C.c_uint32: "u32"}
    return "*" + names[t._type_]


def test_every_function_is_bound_with_the_same_signature():
    hf = header_functions()
    assert set(hf) == {"rrte_hip_raycast", "rrte_hip_raycast_async", "rrte_hip_pick"}
    # Rust: query.rs's own extern block
    block = re.search(r'extern "C" \{(.*?)\n\}', _rust_text(), re.S).group(1)
    rf = {}
    for name, args, ret in re.findall(r"pub fn (\w+)\((.*?)\)\s*(?:->\s*([^;]+))?;", block, re.S):
        rf[name] = (_rust_type(ret) if ret else "void", [_rust_type(a.split(":", 1)[1]) for a in _split_top(args)])
    assert set(rf) == set(hf)
    for name in hf:
        assert rf[name] == hf[name], f"{name}: Rust {rf[name]} != C {hf[name]}"
    # Python: abi.QUERY_EXPORTS (ctypes carries no const; the opaque context and void* are c_void_p)
    assert set(abi.QUERY_EXPORTS) == set(hf)
    for name, (ret, params) in hf.items():
        res, args = abi.QUERY_EXPORTS[name]
        assert res is C.c_int and len(args) == len(params), name
        for a, p in zip(args, params):
            want = p.replace("const*", "*")
            want = "void*" if want in ("*rrte_ctx", "*void") else want
            assert _ctypes_param(a) == want, (name, p)
    # the safe wrappers call the FFI with the declared arity
    text = re.sub(r"pub fn rrte_hip_\w+\(", "pub fn X(", _rust_text())
    calls = []
    for m in re.finditer(r"\b(rrte_hip_\w+)\(", text):
        depth, i = 1, m.end()
        while depth and i < len(text):
            depth += {"(": 1, ")": -1}.get(text[i], 0)
            i += 1
        calls.append((m.group(1), len(_split_top(text[m.end():i - 1]))))
    assert {n for n, _ in calls} == {"rrte_hip_raycast", "rrte_hip_pick"}
    for name, n in calls:
        assert n == len(hf[name][1]), name
    assert "pub mod query;" in (ROOT / "rust" / "rrte-hip-sys" / "src" / "lib.rs").read_text()


def test_library_exports_the_query_symbols():
    lib = abi.load()
    for name in header_functions():
        assert hasattr(lib, name), name
    # host-side argument checks work without a device
    assert lib.rrte_hip_raycast(None, None, None, 0, 0, None) == abi.RRTE_INVALID_ARG
    assert lib.rrte_hip_raycast_async(None, None, None, 0, 0, None, None) == abi.RRTE_INVALID_ARG
    assert lib.rrte_hip_pick(None, None, None, None, 0, None) == abi.RRTE_INVALID_ARG


def test_render_abi_is_unchanged():
    lib = abi.load()
    assert lib.rrte_hip_abi_version() == 2
    assert not set(abi.QUERY_EXPORTS) & set(abi.EXPORTS)
    render_text = re.sub(r"/\*.*?\*/", "", RENDER_HEADER.read_text(), flags=re.S)
    for name in abi.QUERY_EXPORTS:
        assert name not in render_text
    assert '#include "rrte_hip.h"' in HEADER.read_text()
