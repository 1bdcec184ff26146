#!/usr/bin/env python3
"""Mesh build measurements through rrte_stats, one JSON line per leg:

  rebuild    mesh-demo's four meshes; one of them (the ball) gets a new index order every frame, so
             every frame is a mesh-cache miss that builds all four BVHs: a streamed-in asset, an LOD
             switch, a re-meshed surface.  upload_ms (the scene upload with the build in it), the render
             call's wall time and kernel_ms, under --policy host or device.
  quality    traversal quality: kernel_ms of frames of one fixed scene on the host's SAH trees and on
             the device's LBVH trees, same vertices, both in this process, in alternating blocks.

--root DIR imports rrte_amd (and loads its library) from another checkout, e.g. the parent commit's;
policy device and the quality leg are skipped where the library has no rrte_hip_set_mesh_build.
Blocking renders, the generic kernel (no compile in the timed frames); medians over --frames frames
after --warmup.  Compare two builds by alternating runs of this script in one session.  Needs a GPU:
no fallback.
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
ap.add_argument("--legs", default="rebuild,quality")
ap.add_argument("--policy", default="host", choices=["host", "device"])
ap.add_argument("--tag", default="")
args = ap.parse_args()
sys.path.insert(0, args.root)

from rrte_amd import LoweredScene, abi, scenes  # noqa: E402
from rrte_amd.mesh import Mesh  # noqa: E402
from rrte_amd.renderer import Context  # noqa: E402

HAS_POLICY = hasattr(Context, "set_mesh_build")
W, H = args.width, args.height


def base_scene():
    objs, lights, cam, cfg = scenes.mesh_demo(W, H, "lambert_shadow", detail=args.detail)
    return objs[0], list(objs[1:]), lights, cam, cfg


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
               has_policy=HAS_POLICY, device=torch.cuda.get_device_name(0), **kw)
    print(json.dumps(rec), flush=True)


def context(policy):
    ctx = Context(0, jit=abi.JIT_OFF)
    if HAS_POLICY:
        ctx.set_mesh_build(abi.MESH_BUILD_DEVICE if policy == "device" else abi.MESH_BUILD_HOST)
    return ctx


def leg_rebuild():
    if args.policy == "device" and not HAS_POLICY:
        return
    ground, meshes, lights, cam, cfg = base_scene()
    prm = cfg.lower()
    out = np.empty(W * H * 4, np.uint8)
    ball = meshes[1]
    ctx = context(args.policy)
    walls, ups, ks, hosts = [], [], [], []
    for f in range(args.warmup + args.frames):
        t0 = time.perf_counter()
        # the same surface with its triangles in another order: a new topology as far as the library can tell
        meshes[1] = Mesh(ball.positions, np.roll(ball.indices, f + 1, axis=0), ball.normals, ball.material)
        sc = LoweredScene([ground, *meshes], lights, cam)
        host = (time.perf_counter() - t0) * 1e3
        wall, k, up = render_stats(ctx, sc, prm, out)
        if f >= args.warmup:
            walls.append(wall), ups.append(up), ks.append(k), hosts.append(host)
    extra = dict(bvh_builds=int(ctx.mesh_info().bvh_builds))
    if HAS_POLICY:
        bi = ctx.build_info()
        extra.update(device_builds=int(bi.device_builds), host_fallbacks=int(bi.host_fallbacks), depth=int(bi.depth))
    ctx.close()
    emit("rebuild", policy=args.policy, triangles=int(sum(m.num_triangles for m in meshes)), upload_ms=med(ups),
         upload_ms_min=round(min(ups), 4), upload_ms_max=round(max(ups), 4), render_call_ms=med(walls), kernel_ms=med(ks),
         host_lower_ms=med(hosts), **extra)


def leg_quality():
    if not HAS_POLICY:
        return
    ground, meshes, lights, cam, cfg = base_scene()
    prm = cfg.lower()
    out = np.empty(W * H * 4, np.uint8)
    sc = LoweredScene([ground, *meshes], lights, cam)
    ctxs = {p: context(p) for p in ("host", "device")}
    ks = {p: [] for p in ctxs}
    frames = {}
    for p, ctx in ctxs.items():
        for _ in range(args.warmup):
            render_stats(ctx, sc, prm, out)
        frames[p] = out.copy()
    block = 10
    for _ in range(max(1, args.frames // block)):  # alternating blocks
        for p, ctx in ctxs.items():
            for _ in range(block):
                ks[p].append(render_stats(ctx, sc, prm, out)[1])
    depth = int(ctxs["device"].build_info().depth)
    nodes = {p: int(ctx.mesh_info().bvh_nodes) for p, ctx in ctxs.items()}
    for ctx in ctxs.values():
        ctx.close()
    emit("quality", same_frame=bool(np.array_equal(frames["host"], frames["device"])), device_depth=depth, bvh_nodes=nodes,
         kernel_ms={p: med(v) for p, v in ks.items()}, ratio=round(statistics.median(ks["device"]) / statistics.median(ks["host"]), 4))


for leg in args.legs.split(","):
    {"rebuild": leg_rebuild, "quality": leg_quality}[leg]()
