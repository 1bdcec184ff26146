"""All-miss tiles (ray_kernels.hpp ray_kernel_body, launch_plan.hip tile_rects): a ground sphere that
reaches the eye plane gets a rectangle bounded above by its horizon, and a tile outside every object's
rectangle writes the background without casting a ray.  Neither may change a bit: frames with the
rectangles on equal frames with RRTE_TILE_CULL=0 -- linear f32 images, RGBA8 frames and shadow-ray
counts, on the generic and the scene-specialised kernel (its general and its plain entry) -- for
cameras looking up (all sky), with the horizon through the middle of a tile row and exactly on a
tile boundary, looking down (no sky), inside the ground sphere, just above it and just above its culling sphere, with random jitter,
an odd frame size and a frame wider than 2048 pixels (16x16 blocks)."""
import ctypes as C
import math

import numpy as np
import pytest

from rrte_amd import LoweredScene, Raytracer, abi, scenes
from rrte_amd.renderer import Context

pytestmark = pytest.mark.gpu

EYE = (0.0, 2.0, 12.0)  # 2 above the showcase's ground sphere (centre (0, -1000, 0), radius 1000)


def _at_horizon(eye):
    """A target on the ground sphere's horizon, straight ahead (-z): the frame's centre row is the horizon."""
    dip = math.acos(1000.0 / (1000.0 + eye[1]))
    return (eye[0], eye[1] - 10.0 * math.sin(dip), eye[2] - 10.0 * math.cos(dip))


# (name, w, h, position, target, fov, spp, jitter)
POSES = [
    ("up", 160, 88, EYE, (0.0, 14.0, 2.0), 45.0, 1, "center"),
    ("horizon-mid-tile", 160, 88, EYE, _at_horizon(EYE), 45.0, 1, "center"),     # centre row 44: inside tile row 5
    ("horizon-on-boundary", 160, 80, EYE, _at_horizon(EYE), 45.0, 1, "center"),  # centre row 40: between tile rows
    ("down", 160, 88, (0.0, 9.0, 0.5), (0.0, 0.0, 0.0), 45.0, 1, "center"),
    ("inside-ground", 160, 88, (0.0, -1.0, 6.0), (0.0, -1.5, 0.0), 60.0, 1, "center"),
    # the ground's culling sphere is its own, inflated to a radius of ~1001.01 (bvh.hip sphere_bound):
    # 0.3 above the ground is inside it (whole frame), 1.3 above just outside (a tilted horizon: the
    # camera's rotation arc towards an off-axis target rolls it)
    ("just-above", 160, 88, (3.0, 0.3, 9.0), (0.0, 1.0, 0.0), 70.0, 1, "center"),
    ("above-the-bound", 160, 88, (3.0, 1.3, 9.0), (0.0, 1.0, 0.0), 70.0, 1, "center"),
    ("jitter", 160, 88, EYE, (0.0, 2.0, 0.0), 45.0, 2, "random"),
    ("odd-size", 200, 77, (0.0, 8.0, 20.0), (0.0, 2.0, 0.0), 45.0, 1, "center"),
    ("wide", 2056, 24, (0.0, 8.0, 20.0), (0.0, 2.0, 0.0), 45.0, 1, "center"),
]


def _frame(name, w, h, pos, tgt, fov, spp, jitter):
    objs, lights, _, cfg = scenes.SCENES[name](w, h, mode="lambert_shadow")
    cfg.samples_per_pixel, cfg.jitter = spp, jitter
    return objs, lights, scenes._camera(w, h, pos, tgt, fov), cfg


@pytest.mark.parametrize("jit", [abi.JIT_OFF, abi.JIT_ON])
@pytest.mark.parametrize("name", ["sdf-showcase", "advanced-demo"])
def test_rectangles_never_change_a_bit(name, jit, monkeypatch):
    import torch
    rts = {}
    for tc in ("0", "1"):  # the switch is read when a context is created
        monkeypatch.setenv("RRTE_TILE_CULL", tc)
        rts[tc] = Raytracer(scenes.SCENES[name](64, 36, mode="lambert_shadow")[3], device=0, jit=jit)
    for pose in POSES:
        objs, lights, cam, cfg = _frame(name, *pose[1:])
        sc, prm = LoweredScene(objs, lights, cam), cfg.lower()
        out = {}
        for tc, rt in rts.items():
            rt.update_config(cfg)
            _, lin = rt.render_f32(objs, lights, [], cam, linear=True)
            shadow = int(rt.stats().shadow_rays)
            # the RGBA8 frame of a stream (the specialised kernel's plain entry for one sample per pixel)
            ctx = rt.ctx
            o8 = torch.full((prm.width * prm.height,), -1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            ctx.check(ctx.lib.rrte_hip_render_async(ctx.h, sc.ref(), C.byref(prm), o8.data_ptr(), None, None))
            ctx.check(ctx.lib.rrte_hip_synchronize(ctx.h))
            entry = C.c_uint32()
            ctx.check(ctx.lib.rrte_hip_jit_entry(ctx.h, C.byref(entry)))
            want_entry = abi.ENTRY_GENERIC if jit == abi.JIT_OFF else (abi.ENTRY_PLAIN if pose[6] == 1 else abi.ENTRY_GENERAL)
            assert entry.value == want_entry, pose[0]
            out[tc] = (lin.view(np.uint32).copy(), shadow, o8.cpu().numpy(), int(ctx.stats().shadow_rays))
        assert np.array_equal(out["0"][0], out["1"][0]), (name, pose[0])
        assert np.array_equal(out["0"][2], out["1"][2]), (name, pose[0])
        assert out["0"][1] == out["1"][1] == out["0"][3] == out["1"][3], (name, pose[0])
