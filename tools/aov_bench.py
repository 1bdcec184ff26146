#!/usr/bin/env python3
"""Frame-AOV measurements, one JSON line: the sdf-showcase view at 1920x1080, every
leg in this one process on this one box, the legs alternating repeat by repeat.

  a  rrte_hip_render_aov, DEPTH|PRIM, blocking (8 bytes per pixel back)
  b  rrte_hip_render_aov, every plane, blocking (64 bytes per pixel back)
  c  rrte_hip_pick over every pixel of the frame, blocking (8 bytes per pixel up, 48 back): what a
     caller had to do before the AOV entry points existed

and kernel-only times from events around the asynchronous forms into device buffers:

  a_kernel  rrte_hip_render_aov_async, DEPTH|PRIM (8x8 pixel tiles)
  c_kernel  rrte_hip_raycast_async over the frame's pixel-centre rays in row-major order (64x1 pixel
            rows per wave).  rrte_hip_pick has no asynchronous form; this is its kernel with the rays
            read from memory instead of generated, storing the same 48-byte records.

Each leg reports the median, minimum and maximum of --repeats timed calls after --warmup, so the
run-to-run spread is in the line.  --legs picks a subset: `--legs c,c_kernel --root <other tree>`
measures the pick legs of another build of the library (the yardstick is the parent commit's pick),
which needs none of the AOV bindings.  Needs a GPU: no fallback.
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
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--legs", default="a,b,c,a_kernel,c_kernel")
ap.add_argument("--tag", default="")
args = ap.parse_args()
sys.path.insert(0, args.root)

import oracle  # noqa: E402
from rrte_amd import LoweredScene, Raytracer, abi, scenes  # noqa: E402

W, H = args.width, args.height
LEGS = args.legs.split(",")


def frame_rays(sc, t_min):
    """The frame's pixel-centre rays, row-major, as abi.RAY_DTYPE records.  A perspective camera's
    direction scaled to unit length along the view axis is affine in (u, v): fitted through three
    pixels of rrte_oracle_generate_ray, evaluated for all (rrte_hip_raycast normalises it again).
    Equal to the device's rays up to rounding -- for timing, not for comparing hits."""
    lib = oracle.load()

    def ray(u, v):
        o, d = (C.c_float * 3)(), (C.c_float * 3)()
        lib.rrte_oracle_generate_ray(C.byref(sc.ir.camera), float(u), float(v), o, d)
        return np.array(list(o), np.float64), np.array(list(d), np.float64)

    o, fwd = ray(0.5, 0.5)
    g = {uv: ray(*uv)[1] / (ray(*uv)[1] @ fwd) for uv in ((0.0, 0.0), (1.0, 0.0), (0.0, 1.0))}
    u = (np.arange(W) + 0.5) / W
    v = (np.arange(H) + 0.5) / H
    d = (g[0.0, 0.0][None, None, :] + u[None, :, None] * (g[1.0, 0.0] - g[0.0, 0.0])[None, None, :]
         + v[:, None, None] * (g[0.0, 1.0] - g[0.0, 0.0])[None, None, :])
    rays = np.zeros(W * H, dtype=abi.RAY_DTYPE)
    rays["origin"], rays["direction"] = o.astype(np.float32), d.reshape(-1, 3).astype(np.float32)
    rays["t_min"], rays["t_max"] = t_min, np.inf
    return rays


def summary(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4),
                n=len(ms))


def main():
    import torch
    objs, lights, cam, cfg = scenes.sdf_showcase(W, H)
    sc, prm = LoweredScene(objs, lights, cam), cfg.lower()
    rt = Raytracer(cfg, device=0, jit=abi.JIT_OFF)
    ctx, lib, h = rt.ctx, rt.ctx.lib, rt.ctx.h
    n = W * H
    ys, xs = np.divmod(np.arange(n, dtype=np.uint32), np.uint32(W))
    xy = np.ascontiguousarray(np.stack([xs, ys], axis=1), dtype=np.uint32)
    hits = np.zeros(n, dtype=abi.RAY_HIT_DTYPE)
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    calls = {}
    if "a" in LEGS or "b" in LEGS or "a_kernel" in LEGS:
        host = {name: np.zeros((H, W, comps) if comps else (H, W), dtype=dt) for name, (_, dt, comps) in abi.AOV_PLANES.items()}
        hb = abi.AovBuffers()
        for name, a in host.items():
            setattr(hb, name, a.ctypes.data_as(type(getattr(hb, name))))
        d_depth = torch.empty(n, dtype=torch.float32, device="cuda")
        d_prim = torch.empty(n, dtype=torch.int32, device="cuda")
        db = abi.AovBuffers()
        db.depth = C.cast(C.c_void_p(d_depth.data_ptr()), type(db.depth))
        db.prim = C.cast(C.c_void_p(d_prim.data_ptr()), type(db.prim))
        d2 = abi.AovDesc(planes=abi.AOV_DEPTH | abi.AOV_PRIM)
        d7 = abi.AovDesc(planes=abi.AOV_ALL)
        calls["a"] = lambda: ctx.check(lib.rrte_hip_render_aov(h, sc.ref(), C.byref(prm), C.byref(d2), C.byref(hb)))
        calls["b"] = lambda: ctx.check(lib.rrte_hip_render_aov(h, sc.ref(), C.byref(prm), C.byref(d7), C.byref(hb)))
        calls["a_kernel"] = lambda: ctx.check(lib.rrte_hip_render_aov_async(h, sc.ref(), C.byref(prm), C.byref(d2),
                                                                            C.byref(db), sp))
    calls["c"] = lambda: ctx.check(lib.rrte_hip_pick(h, sc.ref(), C.byref(prm), xy.ctypes.data_as(C.POINTER(C.c_uint32)), n,
                                                     hits.ctypes.data_as(C.POINTER(abi.RayHit))))
    if "c_kernel" in LEGS:
        d_rays = torch.from_numpy(frame_rays(sc, cfg.t_min).view(np.uint8).copy()).cuda()
        d_hits = torch.empty(n * 48, dtype=torch.uint8, device="cuda")
        calls["c_kernel"] = lambda: ctx.check(lib.rrte_hip_raycast_async(h, sc.ref(), d_rays.data_ptr(), n, abi.QUERY_CLOSEST,
                                                                         d_hits.data_ptr(), sp))
    ms = {k: [] for k in LEGS}
    for rep in range(args.warmup + args.repeats):  # the legs alternate repeat by repeat
        for k in LEGS:
            if k.endswith("_kernel"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                calls[k]()
                e1.record(stream)
                e1.synchronize()
                t = e0.elapsed_time(e1)
            else:
                t0 = time.perf_counter()
                calls[k]()
                t = (time.perf_counter() - t0) * 1e3
            if rep >= args.warmup:
                ms[k].append(t)
    rec = dict(tag=args.tag, scene="sdf-showcase", size=f"{W}x{H}", build_id=abi.build_id(),
               device=torch.cuda.get_device_name(0), repeats=args.repeats, warmup=args.warmup,
               **{k: summary(v) for k, v in ms.items()})
    # the legs agree where they overlap: AOV depth / prim are pick's t / prim, pixel for pixel
    if "a" in LEGS and "c" in LEGS:
        calls["a"]()
        rec["a_equals_c"] = bool(np.array_equal(host["depth"].ravel().view(np.uint32), hits["t"].view(np.uint32))
                                 and np.array_equal(host["prim"].ravel(), hits["prim"]))
    if "a_kernel" in LEGS and "c_kernel" in LEGS:
        got = d_hits.cpu().numpy().view(abi.RAY_HIT_DTYPE)
        rec["kernel_prims_differ"] = int((got["prim"] != d_prim.cpu().numpy()).sum())  # (rays equal up to rounding)
    ctx.check(lib.rrte_hip_synchronize(h))
    print(json.dumps(rec), flush=True)


main()
