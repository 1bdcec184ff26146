"""One version of a device resource read from several streams at once (context.hpp struct Version,
DESIGN.md §25): a scene version read by frames on two caller streams and by a ray query on a third,
then retired while those may still run -- more scene changes than the context has scene versions,
frames queued alternately on the two streams, nothing synchronised until the end.  Every frame and the
query's hits must equal, byte for byte, the blocking calls of a context that never saw asynchronous
work.  The second case adds tile-list versions that are recycled on every launch, with the kernels' own
index checks on (rrte_hip_check_word)."""
import ctypes as C
import functools

import numpy as np
import pytest

from rrte_amd import LoweredScene, Raytracer, abi, scenes
from rrte_amd.renderer import Context

pytestmark = pytest.mark.gpu

W, H = 64, 36
CHANGES = 6  # more than rrte_ctx::kSceneVersions (4): the ring of scene versions wraps
N_RAYS = 256


def _scene(k):
    """basic-demo with its first light dimmed k times: a different cached scene for every k."""
    objs, lights, cam, cfg = scenes.basic_demo(W, H, mode="lambert_shadow")
    lights[0].intensity = np.float32(50.0 * (1.0 - 0.1 * k))
    return LoweredScene(objs, lights, cam), cfg.lower()


def _camera_rays():
    """256 rays from basic-demo's camera position through a 16 x 16 grid of points around its target."""
    xs, ys = np.meshgrid(np.linspace(-4.0, 4.0, 16), np.linspace(-0.5, 8.0, 16))
    targets = np.stack([xs.ravel(), ys.ravel(), np.zeros(N_RAYS)], axis=1).astype(np.float32)
    origin = np.array([6.0, 4.0, 6.0], np.float32)
    return Raytracer.make_rays(np.broadcast_to(origin, targets.shape), targets - origin)


@functools.lru_cache(maxsize=None)
def _reference():
    """(the frame of every scene, the hits of scene 0) from blocking calls on a fresh context: the
    generic kernel, default environment.  Computed once and shared by every case."""
    ctx = Context(0, jit=abi.JIT_OFF)
    frames = []
    for k in range(CHANGES + 1):
        sc, prm = _scene(k)
        out = np.empty(W * H * 4, np.uint8)
        ctx.check(ctx.lib.rrte_hip_render(ctx.h, sc.ref(), C.byref(prm), out.ctypes.data))
        frames.append(out.tobytes())
    rays = _camera_rays()
    hits = np.zeros(N_RAYS, dtype=abi.RAY_HIT_DTYPE)
    sc, _ = _scene(0)
    ctx.check(ctx.lib.rrte_hip_raycast(ctx.h, sc.ref(), rays.ctypes.data_as(C.POINTER(abi.Ray)), N_RAYS,
                                       abi.QUERY_CLOSEST, hits.ctypes.data_as(C.POINTER(abi.RayHit))))
    ctx.close()
    # not vacuous: every change of the light changes the frame, and the rays hit and miss
    assert len(set(frames)) == CHANGES + 1
    assert 0 < int((hits["prim"] >= 0).sum()) < N_RAYS
    return frames, hits.tobytes()


@pytest.mark.parametrize("recycle", [False, True], ids=["plain", "list_recycling"])
@pytest.mark.parametrize("jit", ["1", "0"], ids=["jit_on", "jit_off"])
def test_one_scene_on_three_caller_streams(jit, recycle, monkeypatch):
    import torch
    want_frames, want_hits = _reference()
    monkeypatch.setenv("RRTE_JIT", jit)
    if recycle:  # a new tile-list version with every launch, and every slot range-checked on the device
        monkeypatch.setenv("RRTE_TILE_ORDER", "2")
        monkeypatch.setenv("RRTE_TEST_RECYCLE", "1")
        monkeypatch.setenv("RRTE_DEBUG", "4")
    ctx = Context(0)
    streams = [torch.cuda.Stream() for _ in range(3)]
    handles = [C.c_void_p(s.cuda_stream) for s in streams]
    bufs = [torch.zeros(W * H, dtype=torch.int32, device="cuda") for _ in range(2 + CHANGES)]
    d_rays = torch.from_numpy(_camera_rays().view(np.uint8).copy()).cuda()
    d_hits = torch.zeros(N_RAYS * abi.RAY_HIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # the fills ran on torch's stream; the library's work runs on others

    def frame(k, buf, stream):
        sc, prm = _scene(k)
        ctx.check(ctx.lib.rrte_hip_render_async(ctx.h, sc.ref(), C.byref(prm), buf.data_ptr(), None, stream))

    # one scene version, three readers: two frames on two streams and a query on a third
    frame(0, bufs[0], handles[0])
    frame(0, bufs[1], handles[1])
    sc0, _ = _scene(0)
    ctx.check(ctx.lib.rrte_hip_raycast_async(ctx.h, sc0.ref(), d_rays.data_ptr(), N_RAYS, abi.QUERY_CLOSEST,
                                             d_hits.data_ptr(), handles[2]))
    # that version and its successors retired while their readers may still run
    for k in range(1, CHANGES + 1):
        frame(k, bufs[1 + k], handles[k % 2])
    if recycle:
        word = C.c_uint64(1)
        ctx.check(ctx.lib.rrte_hip_check_word(ctx.h, C.byref(word)))  # (synchronises the context)
        assert word.value == 0
    else:
        ctx.check(ctx.lib.rrte_hip_synchronize(ctx.h))
    got = [b.cpu().numpy().tobytes() for b in bufs]
    hits = d_hits.cpu().numpy().tobytes()
    ctx.close()
    for i, k in enumerate([0, 0] + list(range(1, CHANGES + 1))):
        assert got[i] == want_frames[k], f"frame {i} (scene {k})"
    assert hits == want_hits
