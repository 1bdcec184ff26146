#!/usr/bin/env python3
"""Mesh-instance measurements through rrte_stats, one JSON line per leg:

  kernel     mesh-demo's meshes under fixed transforms, once baked into plain RRTE_PRIM_MESH objects and
             once as RRTE_PRIM_MESH_INSTANCE objects with the same transforms: kernel_ms of each
             (LAMBERT_SHADOW, generic and scene-specialised kernels).
  move       one mesh moves every frame: the baked way (re-bake the vertices, lower again: a new
             mesh_version, so the library rebuilds its BVHs) and the instance way (only the prim's trs
             changes): upload_ms, the render call's wall time, and the host's bake + lowering time.
  unrelated  a sphere moves every frame in a scene that holds meshes: upload_ms (the mesh cache).

--root DIR imports rrte_amd (and loads its library) from another checkout, e.g. the parent commit's;
legs that need mesh instances are skipped where the package has none.  Blocking renders, the generic
kernel for the move / unrelated legs (no compile in the timed frames); medians over --frames frames
after --warmup.  Needs a GPU: no fallback.
"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=str(Path(__file__).resolve().parents[1]))
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--frames", type=int, default=40)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--detail", type=float, default=1.0, help="mesh_demo's detail (1.0: ~56 K triangles)")
ap.add_argument("--legs", default="kernel,move,unrelated")
ap.add_argument("--tag", default="")
args = ap.parse_args()
sys.path.insert(0, args.root)

from rrte_amd import LoweredScene, Transform, abi, scenes  # noqa: E402
from rrte_amd.renderer import Context  # noqa: E402

try:
    from rrte_amd import MeshInstance  # noqa: E402
except ImportError:
    MeshInstance = None

W, H = args.width, args.height
Q_Y45 = (0.0, 0.38268343, 0.0, 0.9238795)
Q_X45 = (0.38268343, 0.0, 0.0, 0.9238795)
# the fixed transforms of mesh_demo's four meshes (terrain, ball, ring, small ball)
TRANSFORMS = [Transform((0.0, 0.0, 0.0), Q_Y45, (1.0, 1.0, 1.0)), Transform((0.5, 0.3, 0.0), Q_X45, (1.2, 0.8, 1.0)),
              Transform((0.0, 0.5, 0.5), Q_Y45, (0.9, 0.9, 0.9)), Transform((0.0, 0.0, 0.0), Q_X45, (-1.0, 1.0, 1.0))]


def base_scene():
    objs, lights, cam, cfg = scenes.mesh_demo(W, H, "lambert_shadow", detail=args.detail)
    return objs[0], objs[1:], lights, cam, cfg


def render_stats(ctx, sc, prm, out):
    t0 = time.perf_counter()
    ctx.check(ctx.lib.rrte_hip_render(ctx.h, sc.ref(), C.byref(prm), out.ctypes.data_as(C.POINTER(C.c_uint8))))
    wall = (time.perf_counter() - t0) * 1e3
    st = ctx.stats()
    return wall, st.kernel_ms, st.upload_ms, st.jit_active


def med(v):
    return round(statistics.median(v), 4)


def emit(leg, **kw):
    import torch
    rec = dict(leg=leg, tag=args.tag, root=args.root, size=f"{W}x{H}", frames=args.frames, build_id=abi.build_id(),
               device=torch.cuda.get_device_name(0), **kw)
    print(json.dumps(rec), flush=True)


def leg_kernel():
    ground, meshes, lights, cam, cfg = base_scene()
    prm = cfg.lower()
    out = np.empty(W * H * 4, np.uint8)
    forms = {"baked": [ground] + [m.transformed(t) for m, t in zip(meshes, TRANSFORMS)]}
    for o, m in zip(forms["baked"][1:], meshes):
        o.material = m.material
    if MeshInstance is not None:
        forms["instances"] = [ground] + [MeshInstance(m, t) for m, t in zip(meshes, TRANSFORMS)]
    res = {}
    for jit_name, jit in (("generic", abi.JIT_OFF), ("specialised", abi.JIT_ON)):
        for form, objs in forms.items():
            sc = LoweredScene(objs, lights, cam)
            ctx = Context(0, jit=jit)
            ks, active = [], 0
            for f in range(args.warmup + args.frames):
                _, k, _, active = render_stats(ctx, sc, prm, out)
                if f >= args.warmup:
                    ks.append(k)
            ctx.close()
            res[f"{form}_{jit_name}"] = dict(kernel_ms=med(ks), kernel_ms_min=round(min(ks), 4), jit_active=active)
    emit("kernel", triangles=int(sum(m.num_triangles for m in meshes)), **res)


def leg_move():
    ground, meshes, lights, cam, cfg = base_scene()
    prm = cfg.lower()
    out = np.empty(W * H * 4, np.uint8)
    n = args.warmup + args.frames

    def transform(f):  # the ball drifts and turns
        a = 0.01 * f
        return Transform((0.5 + 0.02 * f, 0.3, 0.0), (0.0, float(np.sin(a)), 0.0, float(np.cos(a))), (1.2, 0.8, 1.0))
    res = {}
    # the baked way: re-bake the moving mesh, lower the scene again
    ctx = Context(0, jit=abi.JIT_OFF)
    walls, ups, hosts = [], [], []
    fixed = [m.transformed(t) for m, t in zip(meshes, TRANSFORMS)]
    for o, m in zip(fixed, meshes):
        o.material = m.material
    for f in range(n):
        t0 = time.perf_counter()
        moving = meshes[1].transformed(transform(f))
        moving.material = meshes[1].material
        sc = LoweredScene([ground, fixed[0], moving, fixed[2], fixed[3]], lights, cam)
        host = (time.perf_counter() - t0) * 1e3
        wall, _, up, _ = render_stats(ctx, sc, prm, out)
        if f >= args.warmup:
            walls.append(wall), ups.append(up), hosts.append(host)
    ctx.close()
    res["baked"] = dict(upload_ms=med(ups), render_call_ms=med(walls), host_bake_lower_ms=med(hosts))
    if MeshInstance is not None:
        objs = [ground] + [MeshInstance(m, t) for m, t in zip(meshes, TRANSFORMS)]
        sc = LoweredScene(objs, lights, cam)
        ctx = Context(0, jit=abi.JIT_OFF)
        walls, ups, hosts = [], [], []
        for f in range(n):
            t0 = time.perf_counter()
            sc.prims[2].trs[:] = [float(v) for v in transform(f).trs()]
            host = (time.perf_counter() - t0) * 1e3
            wall, _, up, _ = render_stats(ctx, sc, prm, out)
            if f >= args.warmup:
                walls.append(wall), ups.append(up), hosts.append(host)
        info = ctx.mesh_info()
        ctx.close()
        res["instances"] = dict(upload_ms=med(ups), render_call_ms=med(walls), host_edit_ms=med(hosts),
                                bvh_builds=int(info.bvh_builds), ranges=int(info.ranges))
    emit("move", **res)


def leg_unrelated():
    ground, meshes, lights, cam, cfg = base_scene()
    from rrte_amd import Color, LambertianMaterial, Sphere
    prm = cfg.lower()
    out = np.empty(W * H * 4, np.uint8)
    objs = [ground, *meshes, Sphere((0.0, 3.0, 5.0), 0.5, LambertianMaterial(Color.rgb(0.9, 0.9, 0.2)))]
    sc = LoweredScene(objs, lights, cam)
    ctx = Context(0, jit=abi.JIT_OFF)
    walls, ups = [], []
    for f in range(args.warmup + args.frames):
        sc.prims[len(objs) - 1].p[0] = 0.02 * f
        wall, _, up, _ = render_stats(ctx, sc, prm, out)
        if f >= args.warmup:
            walls.append(wall), ups.append(up)
    ctx.close()
    emit("unrelated", sphere_moves=dict(upload_ms=med(ups), render_call_ms=med(walls)))


for leg in args.legs.split(","):
    {"kernel": leg_kernel, "move": leg_move, "unrelated": leg_unrelated}[leg]()
