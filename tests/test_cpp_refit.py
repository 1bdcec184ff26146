"""The C++ mirror's deforming meshes (Mesh::set_vertices, Raytracer::render_deformed; include/rrte/
rrte_renderer.hpp): a deformed mesh lowers to exactly the bytes the Python mirror produces (normals
recomputed the same way), and on the GPU render_deformed refits and gives the oracle's frame."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from rrte_amd import Color, LambertianMaterial, LoweredScene, Mesh, PointLight, RaytracerConfig, Sphere, abi, scenes
from rrte_amd.mesh import heightfield
from test_cpp_mirror import ir_bytes

ROOT = Path(__file__).resolve().parents[1]
TOOL = ROOT / "rrte_amd" / "lib" / "cpp_refit_tool"
W, H = 64, 36


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.run(["make", "-s", "-C", str(ROOT / "rrte_amd" / "cpp")], check=True)


def _case(tmp_path):
    field = heightfield((-3.0, 0.5, -2.0), 6.0, 7, lambda x, z: 0.6 * np.sin(x) * np.cos(z),
                        LambertianMaterial(Color(0.8, 0.3, 0.3, 1.0)))
    p = field.positions.astype(np.float64)
    pose = np.stack([p[:, 0] + 7.0, p[:, 1] + 1.5 * np.sin(p[:, 0] + p[:, 2]) + 1.0, p[:, 2] + 5.0], 1).astype(np.float32)
    blob, posef = tmp_path / "mesh.bin", tmp_path / "pose.bin"
    with open(blob, "wb") as f:
        f.write(np.array([len(field.positions), len(field.indices)], np.uint32).tobytes())
        f.write(field.positions.tobytes() + field.normals.tobytes() + field.indices.tobytes())
    posef.write_bytes(pose.tobytes())
    twin = Mesh(field.positions, field.indices, field.normals, field.material)
    twin.set_vertices(pose)
    objs = [Sphere((0.0, -1000.0, 0.0), 1000.0, LambertianMaterial(Color(0.5, 0.5, 0.5, 1.0))), twin]
    lights = [PointLight((-10.0, 15.0, 10.0), Color(1.0, 1.0, 1.0, 1.0), 25.0)]
    cam = scenes._camera(W, H, (1.0, 7.0, 16.0), (1.0, 1.5, 0.0))
    cfg = RaytracerConfig(max_depth=1, samples_per_pixel=1, width=W, height=H, mode="lambert_shadow", jitter="center")
    return blob, posef, LoweredScene(objs, lights, cam), cfg, LoweredScene(objs[:1], lights, cam)


def test_cpp_and_python_mirrors_lower_a_deformed_mesh_identically(tmp_path):
    blob, posef, sc, cfg, _ = _case(tmp_path)
    out = tmp_path / "ir.bin"
    subprocess.run([str(TOOL), "ir", str(blob), str(posef), str(W), str(H), str(out)], check=True)
    want, got = ir_bytes(sc, cfg.lower()), out.read_bytes()
    assert len(got) == len(want)
    if got != want:
        d = np.nonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))[0]
        pytest.fail(f"{len(d)} bytes differ, first at {d[0]}")


@pytest.mark.gpu
def test_cpp_render_deformed_refits_and_matches_the_oracle(tmp_path):
    import oracle
    blob, posef, sc, cfg, ground_sc = _case(tmp_path)
    out = tmp_path / "frame.bin"
    subprocess.run([str(TOOL), "render", str(blob), str(posef), str(W), str(H), str(out)], check=True)
    raw = out.read_bytes()
    ri = abi.RefitInfo.from_buffer_copy(raw[:24])
    assert (ri.refits, ri.device_refits, ri.deformed) == (1, 1, 1) and ri.levels >= 3
    got = np.frombuffer(raw[24:], np.uint8)
    r8, _, _ = oracle.render(sc, cfg.lower(), nthreads=8)
    ground, _, _ = oracle.render(ground_sc, cfg.lower(), nthreads=8)
    assert len(got) == W * H * 4 and np.abs(got.astype(np.int16) - r8.astype(np.int16)).max() <= 1
    assert (r8.reshape(-1, 4) != ground.reshape(-1, 4)).any(1).sum() > W * H // 12

