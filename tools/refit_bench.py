#!/usr/bin/env python3
"""Deforming-mesh measurements through rrte_stats, one JSON line per leg:

  deform     mesh-demo's four meshes, the ball's vertices move every frame.  The rebuild way: lower the
             scene again (a new mesh_version, so the library rebuilds every BVH on the host and uploads
             all of it).  The refit way: the same lowering announced with rrte_hip_mesh_refit first, so
             the device refits.  upload_ms, the render call's wall time, kernel_ms, and the host's
             deform + lowering time.
  quality    traversal quality: kernel_ms of a frame on a tree refitted from pose 0 to a deformed pose
             against a tree built for that pose, at three deformation amplitudes (fractions of the
             ball's radius).

--root DIR imports rrte_amd (and loads its library) from another checkout, e.g. the parent commit's;
the refit legs are skipped where the library has no rrte_hip_mesh_refit.  Blocking renders, the
generic kernel (no compile in the timed frames); medians over --frames frames after --warmup.  Needs
a GPU: no fallback.
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
ap.add_argument("--legs", default="deform,quality")
ap.add_argument("--tag", default="")
args = ap.parse_args()
sys.path.insert(0, args.root)

from rrte_amd import LoweredScene, abi, scenes  # noqa: E402
from rrte_amd.renderer import Context  # noqa: E402

HAS_REFIT = hasattr(Context, "mesh_refit")
W, H = args.width, args.height


def base_scene():
    objs, lights, cam, cfg = scenes.mesh_demo(W, H, "lambert_shadow", detail=args.detail)
    return objs[0], objs[1:], lights, cam, cfg


def render_stats(ctx, sc, prm, out):
    t0 = time.perf_counter()
    ctx.check(ctx.lib.rrte_hip_render(ctx.h, sc.ref(), C.byref(prm), out.ctypes.data_as(C.POINTER(C.c_uint8))))
    wall = (time.perf_counter() - t0) * 1e3
    st = ctx.stats()
    return wall, st.kernel_ms, st.upload_ms


def med(v):
    return round(statistics.median(v), 4)


def emit(leg, **kw):
    import torch
    rec = dict(leg=leg, tag=args.tag, root=args.root, size=f"{W}x{H}", frames=args.frames, build_id=abi.build_id(),
               has_refit=HAS_REFIT, device=torch.cuda.get_device_name(0), **kw)
    print(json.dumps(rec), flush=True)


class Deforming:
    """The ball of mesh-demo, displaced along its normals by amp * radius * sin(...): the positions are
    written into the Mesh object (normals kept: shading is not what is measured)."""

    def __init__(self, mesh):
        self.mesh = mesh
        self.base = mesh.positions.copy()
        c = self.base.mean(0)
        self.radius = float(np.linalg.norm(self.base - c, axis=1).max())
        self.dir = mesh.normals.copy()

    def pose(self, amp, phase):
        b = self.base
        s = np.sin(3.0 * b[:, 0] + 2.0 * b[:, 1] + phase) * np.cos(2.5 * b[:, 2] - phase)
        self.mesh.positions = (b + self.dir * (amp * self.radius * s)[:, None]).astype(np.float32)


def leg_deform():
    ground, meshes, lights, cam, cfg = base_scene()
    prm = cfg.lower()
    out = np.empty(W * H * 4, np.uint8)
    n = args.warmup + args.frames
    res = {}
    for way in ("rebuild", "refit"):
        if way == "refit" and not HAS_REFIT:
            continue
        d = Deforming(meshes[1])
        ctx = Context(0, jit=abi.JIT_OFF)
        walls, ups, ks, hosts, refits = [], [], [], [], []
        for f in range(n):
            t0 = time.perf_counter()
            d.pose(0.2, 0.05 * f)
            sc = LoweredScene([ground, *meshes], lights, cam)
            host = (time.perf_counter() - t0) * 1e3
            t1 = time.perf_counter()
            if way == "refit" and f:  # (frame 0 builds)
                ctx.mesh_refit(sc)
            refit_ms = (time.perf_counter() - t1) * 1e3
            wall, k, up = render_stats(ctx, sc, prm, out)
            if f >= args.warmup:
                walls.append(wall), ups.append(up), ks.append(k), hosts.append(host), refits.append(refit_ms)
        extra = {}
        if HAS_REFIT:
            ri = ctx.refit_info()
            extra = dict(refits=int(ri.refits), device_refits=int(ri.device_refits), levels=int(ri.levels))
        extra["bvh_builds"] = int(ctx.mesh_info().bvh_builds)
        ctx.close()
        res[way] = dict(upload_ms=med(ups), render_call_ms=med(walls), kernel_ms=med(ks), host_deform_lower_ms=med(hosts),
                        refit_call_ms=med(refits), **extra)
        d.pose(0.0, 0.0)
    emit("deform", triangles=int(sum(m.num_triangles for m in meshes)), **res)


def leg_quality():
    if not HAS_REFIT:
        return
    ground, meshes, lights, cam, cfg = base_scene()
    prm = cfg.lower()
    out = np.empty(W * H * 4, np.uint8)
    res = {}
    for amp in (0.05, 0.3, 1.0):
        d = Deforming(meshes[1])
        d.pose(0.0, 0.0)
        sc0 = LoweredScene([ground, *meshes], lights, cam)
        d.pose(amp, 1.0)
        sc1 = LoweredScene([ground, *meshes], lights, cam)
        row = {}
        for way in ("rebuilt", "refitted"):
            ctx = Context(0, jit=abi.JIT_OFF)
            if way == "refitted":
                render_stats(ctx, sc0, prm, out)
                ctx.mesh_refit(sc1)
            ks = []
            for f in range(args.warmup + args.frames):
                _, k, _ = render_stats(ctx, sc1, prm, out)
                if f >= args.warmup:
                    ks.append(k)
            row[way] = dict(kernel_ms=med(ks), device_refits=int(ctx.refit_info().device_refits))
            ctx.close()
        res[f"amp_{amp}"] = row
        d.pose(0.0, 0.0)
    emit("quality", **res)


for leg in args.legs.split(","):
    {"deform": leg_deform, "quality": leg_quality}[leg]()
