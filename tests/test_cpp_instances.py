"""The C++ mirror's MeshInstance (include/rrte/rrte_renderer.hpp, rrte_amd/cpp/): instance_demo lowers
to exactly the bytes the Python mirror produces -- one vertex range per base mesh, kind 9 prims with the
instances' transforms -- for the same two base meshes."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from rrte_amd import LoweredScene, Mesh, scenes
from test_cpp_mirror import ir_bytes

ROOT = Path(__file__).resolve().parents[1]
TOOL = ROOT / "rrte_amd" / "lib" / "cpp_instance_tool"


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.run(["make", "-s", "-C", str(ROOT / "rrte_amd" / "cpp")], check=True)


@pytest.mark.parametrize("mode", ["refcompat", "lambert_shadow"])
def test_cpp_and_python_mirrors_lower_instance_demo_identically(mode, tmp_path):
    ball, ring = scenes.instance_demo_meshes(0.1)
    blob = tmp_path / "meshes.bin"
    with open(blob, "wb") as f:
        for m in (ball, ring):
            f.write(np.array([len(m.positions), len(m.indices)], np.uint32).tobytes())
            f.write(m.positions.tobytes() + m.normals.tobytes() + m.indices.tobytes())
    out = tmp_path / "ir.bin"
    subprocess.run([str(TOOL), "ir", str(blob), "160", "90", mode, str(out)], check=True)
    # both mirrors construct their meshes from the same arrays (the constructor normalises the normals)
    twins = tuple(Mesh(m.positions, m.indices, m.normals, m.material) for m in (ball, ring))
    objs, lights, cam, cfg = scenes.instance_demo(160, 90, mode, meshes=twins)
    sc = LoweredScene(objs, lights, cam)
    assert [sc.prims[i].kind for i in range(sc.ir.num_prims)] == [0, 8] + [9] * 8
    want = ir_bytes(sc, cfg.lower())
    got = out.read_bytes()
    assert len(got) == len(want)
    if got != want:
        d = np.nonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))[0]
        pytest.fail(f"{len(d)} bytes differ, first at {d[0]}")
