"""The embedded device headers: one list in the Makefile (DEVICE_HDR) names what is
embedded for hiprtc, hashed into rrte_hip_build_id and copied for offline compiles.  The list must be
closed under #include and hold nothing unreachable; search_groups.hpp is an ordinary header of the
generated source; the retired part-wise exit and the gather's de-interleave kernel stay out."""
import ctypes as C
import re

import pytest

import offline_jit
from rrte_amd import LoweredScene, abi, scenes

CSRC = offline_jit.CSRC
INCLUDE = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)


def _includes(path):
    """The quoted includes of a file, resolved against its directory."""
    return [(path.parent / inc).resolve() for inc in INCLUDE.findall(path.read_text())]


def test_header_list_is_closed_and_minimal():
    hdrs = offline_jit.device_headers()
    names = [h.name for h in hdrs]
    assert len(set(names)) == len(names) and all(h.is_file() for h in hdrs), hdrs
    assert "ray_kernels.hpp" in names and "search_groups.hpp" in names and "device_scene.hpp" in names
    # closed: a listed header includes listed headers only (so no csrc/*.hpp one of them needs is missing),
    # and only ones listed before it -- the list is in include order, which also rules out a cycle
    for k, h in enumerate(hdrs):
        for inc in _includes(h):
            assert inc in hdrs[:k], f"{h.name} includes {inc}, which is not listed before it"
    # minimal: everything listed is reachable from ray_kernels.hpp, or is search_groups.hpp (which the
    # generated source includes itself)
    top = next(h for h in hdrs if h.name == "ray_kernels.hpp")
    seen, todo = {top}, [top]
    while todo:
        for inc in _includes(todo.pop()):
            if inc not in seen:
                seen.add(inc)
                todo.append(inc)
    assert {h.name for h in hdrs} - {h.name for h in seen} == {"search_groups.hpp"}


@pytest.mark.parametrize("topo", ["0", "1"])
def test_generated_source_includes_search_groups_once(topo, tmp_path, monkeypatch):
    src = tmp_path / f"basic_demo_topo{topo}.hip"
    monkeypatch.setenv("RRTE_JIT_DUMP", str(src))
    monkeypatch.setenv("RRTE_JIT_TOPO", topo)
    objs, lights, cam, cfg = scenes.SCENES["basic-demo"](64, 36)
    sc = LoweredScene(objs, lights, cam)
    log = C.create_string_buffer(1 << 16)
    assert abi.load().rrte_hip_jit_check(sc.ref(), 1, log, len(log)) == abi.RRTE_OK, log.value.decode()[:4000]
    text = src.read_text()
    assert ("kTopo = true" in text) == (topo == "1")
    inc = '#include "search_groups.hpp"'
    assert text.count(inc) == 1 and text.count("search_groups") == 1
    scene_end = text.index("}  // namespace rrte_jit")
    assert text.index("struct Scene {") < scene_end < text.index(inc) < text.index('extern "C" __global__')
    # no line of the header's body is pasted any more (lines that say something: code or comment)
    body = {l.strip() for l in (CSRC / "search_groups.hpp").read_text().splitlines()}
    body = {l for l in body if len(l) > 3}
    assert len(body) > 60
    pasted = [l for l in text.splitlines() if l.strip() in body]
    assert not pasted, pasted[:5]


def test_retired_code_stays_out():
    for f in sorted(CSRC.iterdir()):
        if f.is_file():
            text = f.read_text(errors="replace")
            assert "RRTE_PARTS_EXIT" not in text and "kPlan" not in text, f.name
    for h in offline_jit.device_headers():
        assert "deinterleave_batch_kernel" not in h.read_text(), h.name
    assert "deinterleave_batch_kernel" in (CSRC / "gather.hip").read_text()
