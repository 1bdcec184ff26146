"""Every entry point of a scene-specialised kernel within the register / scratch budget, and the
ground sphere's tile rectangle, checked without a GPU.

test_jit_resources.py reads the first kernel of the resource remarks; a module now has two (the
general entry and the plain one, rrte_amd/csrc/jit.hip), and a spilled kernel-argument block in
either is the ~10x regression that test exists for.  The rectangle of a sphere that reaches the eye
plane (launch_plan.hip tile_rects) is compared with a brute-force scan of the pixel-centre rays in
double precision: no tile that holds a hit may lie outside it."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from rrte_amd import LoweredScene, abi, scenes
from test_gpu_empty_tiles import POSES, _frame

ROOT = Path(__file__).resolve().parents[1]


@pytest.mark.skipif(shutil.which("/opt/rocm/bin/hipcc") is None, reason="needs hipcc")
@pytest.mark.parametrize("scene", ["sdf-showcase", "basic-demo", "advanced-demo"])
def test_every_entry_has_no_scratch(scene, tmp_path):
    r = subprocess.run(["bash", str(ROOT / "tools" / "jit_isa.sh"), scene, str(tmp_path / "k.s")],
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    out = r.stdout + r.stderr
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out)]
    vgprs = [int(v) for v in re.findall(r"VGPRs: (\d+)", out)]
    waves = [int(v) for v in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", out)]
    names = re.findall(r"^(rrte_jit_kernel\w*):", (tmp_path / "k.s").read_text(), re.M)
    assert sorted(names) == ["rrte_jit_kernel", "rrte_jit_kernel_plain"], out[-2000:]
    assert len(scratch) == len(vgprs) == len(waves) == len(names), out[-2000:]
    assert scratch == [0, 0], out[-2000:]
    assert all(v <= 64 for v in vgprs), out[-2000:]
    assert waves == [8, 8], out[-2000:]


def _rects(sc, prm):
    sh, n, rects = C.c_uint32(), C.c_uint32(), (C.c_uint32 * 32)()
    assert abi.load().rrte_hip_tile_rects(sc.ref(), C.byref(prm), C.byref(sh), C.byref(n), rects) == abi.RRTE_OK
    return sh.value, [rects[i] for i in range(n.value)]


def _quat_rotate(q, v):
    x, y, z, w = q
    u = np.array([x, y, z])
    return v + 2.0 * np.cross(u, np.cross(u, v) + w * v)


def _hit_tiles(cam, w, h, centre, radius, shift):
    """The tiles holding a pixel whose centre ray meets the sphere (double precision, ray_kernels.hpp generate_ray)."""
    q = np.array(list(cam.rotation), np.float64)
    q /= np.linalg.norm(q)
    o = np.array(list(cam.position), np.float64)
    hh = np.tan(0.5 * float(cam.fov))
    hw = float(cam.aspect_ratio) * hh
    xs, ys = np.meshgrid(np.arange(w), np.arange(h))
    d = np.stack([(2.0 * (xs + 0.5) / w - 1.0) * hw, (1.0 - 2.0 * (ys + 0.5) / h) * hh, -np.ones((h, w))], axis=-1)
    d = _quat_rotate(q, d.reshape(-1, 3))
    oc = o - np.asarray(centre, np.float64)
    b = d @ oc
    a = (d * d).sum(-1)
    disc = b * b - a * (oc @ oc - radius * radius)
    hit = (disc >= 0.0) & (-b + np.sqrt(np.maximum(disc, 0.0)) > 0.0)
    return {(int(x) >> shift, int(y) >> shift) for x, y in zip(xs.reshape(-1)[hit], ys.reshape(-1)[hit])}


@pytest.mark.parametrize("pose", POSES, ids=[p[0] for p in POSES])
def test_ground_rectangle_holds_every_hit_tile(pose):
    objs, lights, cam, cfg = _frame("sdf-showcase", *pose[1:])
    sc, prm = LoweredScene(objs, lights, cam), cfg.lower()
    shift, rects = _rects(sc, prm)
    assert shift == (4 if pose[1] > 2048 else 3) and len(rects) == min(len(objs), 32)
    (g,) = [i for i, o in enumerate(objs) if getattr(o, "radius", 0) == 1000.0]
    r = rects[g]
    bx0, bx1, by0, by1 = r & 255, (r >> 8) & 255, (r >> 16) & 255, r >> 24
    tiles = _hit_tiles(sc.ir.camera, pose[1], pose[2], objs[g].center, 1000.0, shift)
    outside = [t for t in tiles if not (bx0 <= t[0] <= bx1 and by0 <= t[1] <= by1)]
    assert not outside, (pose[0], sorted(outside)[:8])
    # and the bound is the horizon, not the frame.  From 2 or more above the ground the culling sphere's
    # inflated radius (~1001.01, bvh.hip sphere_bound) lifts the horizon by acos(1000 / 1002) -
    # acos(1001.01 / 1002) = 0.019 rad, 2.1 rows of the smallest field of view per row here (45 degrees
    # over 88 rows), plus the margin of 2: less than a tile row of 8 above the first hit row
    if tiles and bx0 <= bx1 and cam.transform.position[1] >= 2.0:
        assert by0 >= min(t[1] for t in tiles) - 1, pose[0]


def test_the_poses_are_what_they_say():
    """All sky has no rectangle at all; the horizon poses start the ground's rectangle near the horizon's
    tile row; looking down, from inside the ground and from inside its culling sphere it is the whole
    frame; just outside the culling sphere it is bounded again."""
    tops = {}
    for pose in POSES[:7]:
        objs, lights, cam, cfg = _frame("sdf-showcase", *pose[1:])
        _, rects = _rects(LoweredScene(objs, lights, cam), cfg.lower())
        (g,) = [i for i, o in enumerate(objs) if getattr(o, "radius", 0) == 1000.0]
        tops[pose[0]] = None if (rects[g] & 255) > ((rects[g] >> 8) & 255) else (rects[g] >> 16) & 255
        if pose[0] == "up":
            assert all((r & 255) > ((r >> 8) & 255) for r in rects)
    assert tops["up"] is None
    # (the horizon is the frame's centre row, 44 of 88 and 40 of 80: tile rows 5 and 4 at the latest)
    assert 0 < tops["horizon-mid-tile"] <= 5 and 0 < tops["horizon-on-boundary"] <= 4
    assert tops["down"] == 0 and tops["inside-ground"] == 0 and tops["just-above"] == 0
    assert tops["above-the-bound"] is not None and tops["above-the-bound"] > 0


def test_tile_rects_rejects_null_arguments():
    lib = abi.load()
    objs, lights, cam, cfg = scenes.SCENES["basic-demo"](64, 36)
    sc, prm = LoweredScene(objs, lights, cam), cfg.lower()
    sh, n, rects = C.c_uint32(), C.c_uint32(), (C.c_uint32 * 32)()
    assert lib.rrte_hip_tile_rects(None, C.byref(prm), C.byref(sh), C.byref(n), rects) == abi.RRTE_INVALID_ARG
    assert lib.rrte_hip_tile_rects(sc.ref(), None, C.byref(sh), C.byref(n), rects) == abi.RRTE_INVALID_ARG
    assert lib.rrte_hip_tile_rects(sc.ref(), C.byref(prm), C.byref(sh), C.byref(n), None) == abi.RRTE_INVALID_ARG
