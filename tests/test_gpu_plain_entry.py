"""The two entry points of a scene-specialised kernel (rrte_amd/csrc/jit.hip, shade.hpp
LaunchPlain): the plain entry, with an engine frame's launch constants compiled in, renders the bytes
and counts the shadow rays of the general entry (RRTE_JIT_PLAIN=0), within the usual bar of the oracle
(u8 <= 1, counts exact); and every launch that breaks one of the plain entry's assumptions -- f32
output, a rank's band share, a gather batch, a registered host buffer, RRTE_DEBUG -- takes the
general entry (rrte_hip_jit_entry) and still renders the general frame."""
import ctypes as C

import numpy as np
import pytest

import oracle
from rrte_amd import LoweredScene, abi, scenes
from rrte_amd.renderer import Context

pytestmark = pytest.mark.gpu

CASES = [("sdf-showcase", 160, 90), ("sdf-showcase", 161, 91), ("advanced-demo", 160, 90), ("basic-demo", 160, 90)]


def _entry(ctx):
    e = C.c_uint32(99)
    ctx.check(ctx.lib.rrte_hip_jit_entry(ctx.h, C.byref(e)))
    return e.value


def _scene(name, w, h):
    objs, lights, cam, cfg = scenes.SCENES[name](w, h)
    return LoweredScene(objs, lights, cam), cfg.lower()


def _async(ctx, sc, prm, rows=None, f32=False):
    """One frame through rrte_hip_render_async: (RGBA8 bytes, f32 or None, shadow rays, entry)."""
    import torch
    n = prm.width * (prm.height if rows is None else rows)
    o8 = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    of = torch.zeros(n * 4, dtype=torch.float32, device="cuda") if f32 else None
    torch.cuda.synchronize()  # the fills ran on torch's stream; the render runs on the context's
    ctx.check(ctx.lib.rrte_hip_render_async(ctx.h, sc.ref(), C.byref(prm), o8.data_ptr(),
                                            of.data_ptr() if f32 else None, None))
    ctx.check(ctx.lib.rrte_hip_synchronize(ctx.h))
    return (o8.cpu().numpy().view(np.uint8), of.cpu().numpy() if f32 else None, int(ctx.stats().shadow_rays),
            _entry(ctx))


def _context(monkeypatch, **env):
    for k, v in env.items():  # the switches are read when a context is created
        monkeypatch.setenv(k, v)
    ctx = Context(0, jit=abi.JIT_ON)
    for k in env:
        monkeypatch.delenv(k)
    return ctx


_general = {}


def _general_frame(name, w, h, monkeypatch):
    """The frame and shadow-ray count of the general entry (rendered once per case)."""
    if (name, w, h) not in _general:
        ctx = _context(monkeypatch, RRTE_JIT_PLAIN="0")
        sc, prm = _scene(name, w, h)
        got, _, shadow, entry = _async(ctx, sc, prm)
        ctx.close()
        assert entry == abi.ENTRY_GENERAL
        got.setflags(write=False)
        _general[(name, w, h)] = (got, shadow)
    return _general[(name, w, h)]


def test_no_launch_yet_reports_no_entry():
    ctx = Context(0, jit=abi.JIT_ON)
    assert _entry(ctx) == abi.ENTRY_NONE
    assert ctx.lib.rrte_hip_jit_entry(ctx.h, None) == abi.RRTE_INVALID_ARG
    ctx.close()


@pytest.mark.parametrize("name,w,h", CASES)
def test_plain_entry_renders_the_general_entrys_frame(name, w, h, monkeypatch):
    want, want_shadow = _general_frame(name, w, h, monkeypatch)
    ctx = Context(0, jit=abi.JIT_ON)
    sc, prm = _scene(name, w, h)
    for frame in range(2):
        got, _, shadow, entry = _async(ctx, sc, prm)
        assert entry == abi.ENTRY_PLAIN and ctx.stats().jit_active == 1
        assert np.array_equal(got, want), f"frame {frame}: {int((got != want).sum())} bytes differ"
        assert shadow == want_shadow
    ctx.close()
    ref8, _, ref_shadow = oracle.render(sc, prm, nthreads=16, want_f32=False)
    assert int(np.abs(got.astype(np.int16) - ref8.astype(np.int16)).max()) <= 1
    assert shadow == ref_shadow


def test_jit_off_runs_the_generic_kernel():
    ctx = Context(0, jit=abi.JIT_OFF)
    sc, prm = _scene("sdf-showcase", 160, 90)
    assert _async(ctx, sc, prm)[3] == abi.ENTRY_GENERIC
    ctx.close()


def test_f32_frame_takes_the_general_entry(monkeypatch):
    want, want_shadow = _general_frame("sdf-showcase", 160, 90, monkeypatch)
    ctx = Context(0, jit=abi.JIT_ON)
    sc, prm = _scene("sdf-showcase", 160, 90)
    got, f32, shadow, entry = _async(ctx, sc, prm, f32=True)
    assert entry == abi.ENTRY_GENERAL
    assert np.array_equal(got, want) and shadow == want_shadow and np.isfinite(f32).all() and f32.any()
    assert _async(ctx, sc, prm)[3] == abi.ENTRY_PLAIN  # the same context's next RGBA8 frame
    ctx.close()


def test_other_gamma_and_more_samples_take_the_general_entry():
    ctx = Context(0, jit=abi.JIT_ON)
    sc, prm = _scene("sdf-showcase", 160, 90)
    prm.gamma = 2.0
    assert _async(ctx, sc, prm)[3] == abi.ENTRY_GENERAL
    prm.gamma = 2.2
    assert _async(ctx, sc, prm)[3] == abi.ENTRY_PLAIN
    prm.samples_per_pixel = 2
    assert _async(ctx, sc, prm)[3] == abi.ENTRY_GENERAL
    ctx.close()


def test_band_share_takes_the_general_entry(monkeypatch):
    from test_gpu_4k import band_owner
    w, h, nranks, rank, band = 160, 90, 2, 1, 16
    want, _ = _general_frame("sdf-showcase", w, h, monkeypatch)
    ctx = _context(monkeypatch, RRTE_EMULATE_RANK=f"{nranks}:{rank}")
    sc, prm = _scene("sdf-showcase", w, h)
    prm.band_rows = band
    part = abi.band_layout(sc.ref(), C.byref(prm), nranks)
    rows = ctx.lib.rrte_hip_band_rows_for_rank_ex(h, band, nranks, rank, *part)
    img_rows = [y for y in range(h) if band_owner(y // band, nranks, *part) == rank]
    assert 0 < rows == len(img_rows) < h
    got, _, _, entry = _async(ctx, sc, prm, rows=rows)
    ctx.close()
    assert entry == abi.ENTRY_GENERAL
    assert np.array_equal(got.reshape(rows, w * 4), want.reshape(h, w * 4)[img_rows])


def test_gather_batch_takes_the_general_entry(monkeypatch):
    import torch
    w, h, nranks = 160, 90, 2
    want, _ = _general_frame("sdf-showcase", w, h, monkeypatch)
    ctx = _context(monkeypatch, RRTE_FORCE_GATHER="1", RRTE_EMULATE_PEERS=str(nranks))
    lib = ctx.lib
    uid = (C.c_uint8 * abi.UNIQUE_ID_BYTES)()
    ctx.check(lib.rrte_hip_comm_unique_id(uid))
    ctx.check(lib.rrte_hip_comm_init(ctx.h, 1, 0, uid))
    ctx.check(lib.rrte_hip_set_gather_batch(ctx.h, 2))
    sc, prm = _scene("sdf-showcase", w, h)
    outs = [torch.full((w * h,), -1, dtype=torch.int32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    for o in outs:
        ctx.check(lib.rrte_hip_render_gather_async(ctx.h, sc.ref(), C.byref(prm), 0, o.data_ptr(), None))
        assert _entry(ctx) != abi.ENTRY_PLAIN
    ctx.check(lib.rrte_hip_flush(ctx.h))
    ctx.check(lib.rrte_hip_synchronize(ctx.h))
    assert _entry(ctx) == abi.ENTRY_GENERAL
    for o in outs:
        assert np.array_equal(o.cpu().numpy().view(np.uint8), want)
    ctx.close()


def test_registered_host_buffer_takes_the_general_entry(monkeypatch):
    w, h = 160, 90
    want, want_shadow = _general_frame("sdf-showcase", w, h, monkeypatch)
    ctx = Context(0, jit=abi.JIT_ON)
    sc, prm = _scene("sdf-showcase", w, h)
    reg = np.full(w * h * 4, 7, np.uint8)
    ctx.check(ctx.lib.rrte_hip_host_register(ctx.h, reg.ctypes.data, reg.nbytes))
    ctx.check(ctx.lib.rrte_hip_render(ctx.h, sc.ref(), C.byref(prm), reg.ctypes.data_as(C.POINTER(C.c_uint8))))
    assert _entry(ctx) == abi.ENTRY_GENERAL
    assert np.array_equal(reg, want) and int(ctx.stats().shadow_rays) == want_shadow
    ctx.check(ctx.lib.rrte_hip_host_unregister(ctx.h, reg.ctypes.data))
    ctx.close()


def test_debug_bits_take_the_general_entry(monkeypatch):
    want, want_shadow = _general_frame("sdf-showcase", 160, 90, monkeypatch)
    ctx = _context(monkeypatch, RRTE_DEBUG="4")
    sc, prm = _scene("sdf-showcase", 160, 90)
    got, _, shadow, entry = _async(ctx, sc, prm)
    assert entry == abi.ENTRY_GENERAL
    assert np.array_equal(got, want) and shadow == want_shadow
    word = C.c_uint64(1)
    ctx.check(ctx.lib.rrte_hip_check_word(ctx.h, C.byref(word)))
    assert word.value == 0
    ctx.close()
