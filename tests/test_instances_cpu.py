"""Mesh instances without a GPU: lowering (one Mesh object, one range), the scene-asset loader's
instance mode, the dump/load round trip of an instance scene, and the scene-specialised kernels of
instance_demo compiling for gfx950 (full and topology), with their register and scratch figures."""
import ctypes as C
import json
import shutil

import numpy as np
import pytest

import instance_ref as ir
import offline_jit
from rrte_amd import (Camera, Color, LambertianMaterial, LoweredScene, Mesh, MeshInstance, Sphere, Transform, abi,
                      load_scene_asset, scenes, sceneio)
from rrte_amd.mesh import icosphere


def _trs(p):
    return [np.float32(v) for v in p.trs]


def test_base_and_three_instances_share_one_range():
    red, blue = LambertianMaterial(Color.rgb(0.8, 0.2, 0.2)), LambertianMaterial(Color.rgb(0.2, 0.2, 0.8))
    ball = icosphere((0.0, 1.0, 0.0), 1.0, 1, red)
    trs = [Transform((1.0, 2.0, 3.0), scenes.Q_Y90, (1.0, 1.0, 1.0)),
           Transform((-1.0, 0.0, 0.5), scenes.Q_X45, (2.0, 0.5, 1.0)),
           Transform((0.0, 0.0, -4.0), scenes.Q_X45_Y45, (-1.0, 1.0, 1.0))]
    insts = [MeshInstance(ball, trs[0]), MeshInstance(ball, trs[1], blue), MeshInstance(ball)]
    insts[2].set_transform(trs[2])
    sc = LoweredScene([ball, *insts], [], Camera())
    assert sc.ir.num_mesh_vertices == len(ball.positions) and sc.ir.num_mesh_indices == 3 * ball.num_triangles
    assert [sc.prims[i].kind for i in range(4)] == [8, 9, 9, 9]
    assert {(sc.prims[i].sdf_first, sc.prims[i].sdf_count) for i in range(4)} == {(0, ball.num_triangles)}
    for i, t in enumerate(trs):
        assert _trs(sc.prims[1 + i]) == [np.float32(v) for v in t.trs()]
    # the material defaults to the mesh's; an own material is kept
    assert [sc.prims[i].material for i in range(4)] == [0, 0, 1, 0] and sc.ir.num_materials == 2
    # an instance listed before (or without) its base gets the same single range; another Mesh another
    other = icosphere((0.0, 0.0, 0.0), 0.5, 0, red)
    sc = LoweredScene([insts[0], MeshInstance(other), ball, other], [], Camera())
    assert [(sc.prims[i].kind, sc.prims[i].sdf_first, sc.prims[i].sdf_count) for i in range(4)] == [
        (9, 0, 80), (9, 80, 20), (8, 0, 80), (8, 80, 20)]
    assert sc.ir.num_mesh_indices == 3 * 100
    assert insts[0].num_triangles == 80 and isinstance(insts[0].baked(), Mesh)


def test_instance_demo_lowering():
    objs, lights, cam, cfg = scenes.instance_demo(64, 36, detail=0.1)
    sc = LoweredScene(objs, lights, cam)
    kinds = [sc.prims[i].kind for i in range(sc.ir.num_prims)]
    assert kinds == [0, 8] + [9] * 8
    ranges = {(sc.prims[i].sdf_first, sc.prims[i].sdf_count) for i in range(1, 10)}
    assert ranges == {(0, 320), (320, 256)}
    scales = [tuple(sc.prims[i].trs[7:10]) for i in range(2, 10)]
    assert any(s[0] == s[1] == s[2] == 1.0 for s in scales)                  # rigid
    assert any(s[0] == s[1] == s[2] != 1.0 for s in scales)                  # uniformly scaled
    assert any(len(set(s)) > 1 and min(s) > 0 for s in scales)               # non-uniformly scaled
    assert sum(1 for s in scales if s[0] * s[1] * s[2] < 0) == 2             # mirrored
    for name in ("Q_Y90", "Q_X45", "Q_Y45", "Q_X45_Y45"):  # unit quaternions to f32 rounding
        qv = np.array(getattr(scenes, name), dtype=np.float32).astype(np.float64)
        assert abs(float(qv @ qv) - 1.0) < 2e-7, name
    assert "instance-demo" not in scenes.SCENES  # (the BASELINE scene list is the oracle's)


def _asset_scene(tmp_path):
    ball = icosphere((0.0, 0.0, 0.0), 1.0, 1)
    (tmp_path / "ball.json").write_text(json.dumps(ball.to_asset("ball.json")))
    tr = [{"position": [1.0, 2.0, 3.0], "rotation": list(scenes.Q_Y45), "scale": [1.0, 2.0, 0.5]},
          {"position": [-2.0, 0.5, 0.0], "rotation": [0.0, 0.0, 0.0, 1.0], "scale": [-1.0, 1.0, 1.0]}]
    mat = {"albedo": {"r": 0.2, "g": 0.6, "b": 0.3, "a": 1.0}}
    scene = {"entities": [{"name": "a", "mesh": "ball.json", "material": mat, "transform": tr[0]},
                          {"name": "b", "mesh": "ball.json", "material": None, "transform": tr[1]}],
             "lights": [], "camera": {"fov": 0.8, "near": 0.1, "far": 100.0,
                                      "transform": {"position": [0, 1, 8], "rotation": [0, 0, 0, 1], "scale": [1, 1, 1]}}}
    path = tmp_path / "scene.json"
    path.write_text(json.dumps(scene))
    return path, ball, tr


def test_scene_asset_loader_shares_meshes_as_instances(tmp_path):
    path, ball, tr = _asset_scene(tmp_path)
    objs, lights, cam = load_scene_asset(path, 16 / 9, instances=True)
    assert [type(o) for o in objs] == [MeshInstance, MeshInstance]
    assert objs[0].mesh is objs[1].mesh and [o.name for o in objs] == ["a", "b"]
    assert objs[0].material is not objs[1].material
    sc = LoweredScene(objs, lights, cam)
    assert sc.ir.num_mesh_indices == 3 * ball.num_triangles and sc.ir.num_mesh_vertices == len(ball.positions)
    for i in range(2):
        assert sc.prims[i].kind == abi.PRIM_MESH_INSTANCE
        want = [*tr[i]["position"], *tr[i]["rotation"], *tr[i]["scale"]]
        assert _trs(sc.prims[i]) == [np.float32(v) for v in want]
    assert np.array_equal(objs[0].mesh.positions, ball.positions)


def test_scene_asset_loader_still_bakes_by_default(tmp_path):
    path, ball, tr = _asset_scene(tmp_path)
    objs, lights, cam = load_scene_asset(path, 16 / 9)
    assert [type(o) for o in objs] == [Mesh, Mesh]
    sc = LoweredScene(objs, lights, cam)
    assert [sc.prims[i].kind for i in range(2)] == [8, 8]
    assert sc.ir.num_mesh_indices == 2 * 3 * ball.num_triangles
    want = Mesh.from_asset(tmp_path / "ball.json").transformed(Transform(tuple(tr[0]["position"]), tuple(tr[0]["rotation"]), tuple(tr[0]["scale"])))
    assert np.array_equal(objs[0].positions, want.positions) and np.array_equal(objs[0].normals, want.normals)


def test_dump_load_round_trip_of_an_instance_scene(tmp_path, monkeypatch):
    from test_scene_io import _arrays
    objs, lights, cam, cfg = scenes.instance_demo(24, 14, detail=0.1)
    sc, prm = LoweredScene(objs, lights, cam), cfg.lower()
    path = tmp_path / "frame.rrtesir"
    sceneio.dump(sc.ref(), prm, str(path))
    ld = sceneio.load(str(path))
    assert _arrays(ld.ir) == _arrays(sc.ir)
    assert bytes(ld.params) == bytes(prm)
    assert [ld.ir.prims[i].kind for i in range(ld.ir.num_prims)] == [0, 8] + [9] * 8
    # and it replays on the checker: the same frame from the loaded copy
    a = ir.render(monkeypatch, sc, prm)
    b = ir.render(monkeypatch, ld, ld.params)
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and a[2] == b[2]
    ld.close()


@pytest.mark.skipif(shutil.which("/opt/rocm/bin/hipcc") is None, reason="needs hipcc")
@pytest.mark.parametrize("topo", ["0", "1"])
def test_instance_demo_kernels_compile_for_gfx950(topo, tmp_path, monkeypatch):
    """rrte_hip_jit_check: the full (RRTE_JIT_TOPO=0) and the topology (=1) LAMBERT_SHADOW kernels of
    instance_demo compile with hiprtc, no device needed.  Their resources are printed (pytest -s) and
    recorded in DESIGN.md §16 (measured: 75 VGPRs, 106 SGPRs, no scratch, 5 waves per SIMD for both; the
    same scene baked to plain meshes: 67 VGPRs, 104 SGPRs, no scratch, 5 waves).  Asserted: no scratch, and
    the occupancy every mesh kernel has -- the per-lane BVH stack takes 8 KiB of LDS per wave, so the
    160 KiB of a CU hold 20 waves, 5 per SIMD, which 512 / 5 -> 96 VGPRs still reach."""
    monkeypatch.setenv("RRTE_JIT_TOPO", topo)
    src = tmp_path / f"instance_demo_topo{topo}.hip"
    monkeypatch.setenv("RRTE_JIT_DUMP", str(src))
    objs, lights, cam, cfg = scenes.instance_demo(64, 36, detail=0.1)
    sc = LoweredScene(objs, lights, cam)
    log = C.create_string_buffer(1 << 16)
    assert abi.load().rrte_hip_jit_check(sc.ref(), 1, log, len(log)) == abi.RRTE_OK, log.value.decode()[:4000]
    text = src.read_text()
    assert ("kTopo = true" in text) == (topo == "1")
    res = offline_jit.resources(src, tmp_path)
    print(f"instance_demo {'topology' if topo == '1' else 'full'} kernel: {res}")
    assert res["ScratchSize [bytes/lane]"] == 0
    assert res["VGPRs"] <= 96 and res["Occupancy [waves/SIMD]"] == 5


def test_topology_source_names_the_instance_kind(tmp_path, monkeypatch):
    """The topology kernel compiles in each object's kind: 8 for a plain mesh, 9 for an instance of it."""
    src = tmp_path / "mesh_demo.hip"
    monkeypatch.setenv("RRTE_JIT_DUMP", str(src))
    monkeypatch.setenv("RRTE_JIT_TOPO", "1")
    ball = icosphere((0.0, 1.0, 0.0), 1.0, 1, LambertianMaterial(Color.rgb(0.8, 0.2, 0.2)))
    for objs, want in (([Sphere((0, -1000.0, 0), 1000.0), ball], "{0u,0u,0u,false},{8u,"),
                       ([Sphere((0, -1000.0, 0), 1000.0), MeshInstance(ball)], "{0u,0u,0u,false},{9u,")):
        sc = LoweredScene(objs, [], Camera())
        log = C.create_string_buffer(1 << 16)
        assert abi.load().rrte_hip_jit_check(sc.ref(), 0, log, len(log)) == abi.RRTE_OK, log.value.decode()[:4000]
        assert want in src.read_text()
