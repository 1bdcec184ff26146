#!/usr/bin/env python3
"""Ray-query throughput on the GPU (include/rrte_hip_query.h).  Does not gate anything.

  raycast  2^20 incoherent rays (the generator of tests/query_ref.py, reseeded per size) through
           rrte_hip_raycast_async on device buffers, closest hit and any hit, on sdf-showcase and
           mesh-demo: HIP events around `--steps` launches after `--warmup` launches.
  pick     a full 1920x1080 rrte_hip_pick on sdf-showcase: host clock around the blocking call (it ends
           in a stream synchronise), so the figure includes the 16.6 MB of pixel pairs going in and the
           99.5 MB of hit records coming out.  The kernel's own time comes from a kernel trace of
           `--only pick` (rocprofv3 --kernel-trace --stats, in a run of its own).
  frame    the same scene's REFCOMPAT depth-1 1080p frame (generic kernel, JIT off) through
           rrte_hip_render_async into a device buffer, HIP events: the same primary-ray work as `pick`
           with 4 B per pixel written instead of 48 B per ray.

One JSON line per measurement.  RRTE_PACKAGE_ROOT=<checkout> measures that checkout's package and
library instead of this one's (the frame on the parent commit, on the same box)."""
import argparse
import ctypes as C
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(os.environ.get("RRTE_PACKAGE_ROOT", Path(__file__).resolve().parents[1])).resolve()
sys.path.insert(0, str(ROOT))

from rrte_amd import LoweredScene, Raytracer, abi, scenes  # noqa: E402


def gen_rays(n, t_max=np.inf):
    rng = np.random.default_rng(0x5EED2025)
    o = rng.uniform([-12.0, 0.2, -12.0], [12.0, 9.0, 12.0], (n, 3)).astype(np.float32)
    tg = rng.uniform([-8.0, 0.0, -8.0], [8.0, 4.0, 8.0], (n, 3)).astype(np.float32)
    d = (tg - o) * rng.uniform(0.1, 3.0, n).astype(np.float32)[:, None]
    rays = np.zeros(n, dtype=[("origin", "<f4", (3,)), ("t_min", "<f4"), ("direction", "<f4", (3,)), ("t_max", "<f4")])
    rays["origin"], rays["direction"], rays["t_min"] = o, d, 1e-3
    rays["t_max"] = np.sqrt(((tg - o).astype(np.float64) ** 2).sum(1)) if t_max is None else t_max
    return rays


def emit(**kw):
    print(json.dumps(kw), flush=True)


def bench_raycast(args, torch):
    n = args.rays
    for name in ("sdf-showcase", "mesh-demo"):
        objs, lights, cam, cfg = scenes.SCENES[name](1920, 1080)
        rt = Raytracer(cfg, device=0)
        stream = torch.cuda.Stream()
        st = C.c_void_p(stream.cuda_stream)
        for kind, any_hit, t_max in (("closest", False, np.inf), ("any_segment", True, None)):
            rays = gen_rays(n, t_max)
            d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
            d_hits = torch.empty(n * 48, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            sc = LoweredScene(objs, lights, cam)  # lowered once: every launch finds the scene cached

            def launch():
                rt.ctx.check(rt.ctx.lib.rrte_hip_raycast_async(rt.ctx.h, sc.ref(), d_rays.data_ptr(), n,
                                                               abi.QUERY_ANY if any_hit else abi.QUERY_CLOSEST,
                                                               d_hits.data_ptr(), st))
            for _ in range(args.warmup):
                launch()
            stream.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.steps):
                launch()
            e1.record(stream)
            stream.synchronize()
            ms = e0.elapsed_time(e1) / args.steps
            hits = d_hits.cpu().numpy().view(abi.RAY_HIT_DTYPE)
            emit(what="raycast_async", scene=name, kind=kind, rays=n, ms_per_call=round(ms, 4),
                 mray_per_s=round(n / ms / 1e3, 1), hit_fraction=round(float((hits["prim"] >= 0).mean()), 4),
                 steps=args.steps, warmup=args.warmup, timing="hip events")
        rt.ctx.check(rt.ctx.lib.rrte_hip_synchronize(rt.ctx.h))


def bench_pick(args, torch):
    w, h = 1920, 1080
    objs, lights, cam, cfg = scenes.sdf_showcase(w, h, mode="refcompat")
    rt = Raytracer(cfg, device=0)
    sc = LoweredScene(objs, lights, cam)
    prm = cfg.lower()
    ys, xs = np.divmod(np.arange(w * h, dtype=np.uint32), np.uint32(w))
    xy = np.ascontiguousarray(np.stack([xs, ys], axis=1), dtype=np.uint32)
    hits = np.zeros(w * h, dtype=abi.RAY_HIT_DTYPE)

    def call():
        rt.ctx.check(rt.ctx.lib.rrte_hip_pick(rt.ctx.h, sc.ref(), C.byref(prm), xy.ctypes.data_as(C.POINTER(C.c_uint32)),
                                              w * h, hits.ctypes.data_as(C.POINTER(abi.RayHit))))
    for _ in range(max(1, args.warmup // 4)):
        call()
    steps = max(1, args.steps // 4)
    t0 = time.perf_counter()
    for _ in range(steps):
        call()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    emit(what="pick", scene="sdf-showcase", rays=w * h, ms_per_call=round(ms, 3), mray_per_s=round(w * h / ms / 1e3, 1),
         hit_fraction=round(float((hits["prim"] >= 0).mean()), 4), steps=steps,
         timing="host clock around the blocking call (pageable host buffers, copies included)")


def bench_frame(args, torch):
    w, h = 1920, 1080
    objs, lights, cam, cfg = scenes.sdf_showcase(w, h, mode="refcompat")
    rt = Raytracer(cfg, device=0, jit=abi.JIT_OFF)
    sc = LoweredScene(objs, lights, cam)
    prm = cfg.lower()
    buf = torch.empty(w * h, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    st = C.c_void_p(stream.cuda_stream)

    def launch():
        rt.ctx.check(rt.ctx.lib.rrte_hip_render_async(rt.ctx.h, sc.ref(), C.byref(prm), buf.data_ptr(), None, st))
    for _ in range(args.warmup):
        launch()
    stream.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(args.steps):
        launch()
    e1.record(stream)
    stream.synchronize()
    ms = e0.elapsed_time(e1) / args.steps
    rt.ctx.check(rt.ctx.lib.rrte_hip_synchronize(rt.ctx.h))
    emit(what="frame_refcompat_depth1", scene="sdf-showcase", package=str(ROOT), build_id=abi.build_id(), rays=w * h,
         ms_per_frame=round(ms, 4), mray_per_s=round(w * h / ms / 1e3, 1), jit_active=int(rt.stats().jit_active),
         steps=args.steps, warmup=args.warmup, timing="hip events")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--only", choices=["raycast", "pick", "frame"], default=None)
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("query_bench: no GPU visible (there is no CPU path to measure)")
    emit(what="box", device=torch.cuda.get_device_name(0), build_id=abi.build_id())
    for name, fn in (("raycast", bench_raycast), ("pick", bench_pick), ("frame", bench_frame)):
        if args.only in (None, name):
            fn(args, torch)


if __name__ == "__main__":
    main()
