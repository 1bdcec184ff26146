"""The grouped object searches of the scene-specialised kernels (rrte_amd/csrc/search_groups.hpp): every
object whose mask bit is set is still tested, in index order, so frames are the oracle's byte for byte and
shadow-ray counts are exact -- for object counts around the group size and the 32- and 64-bit mask widths,
with the only occluder of the probe region in the first slot of a group, the last slot of a group and the
last index overall (tests/search_group_scenes.py), through every kernel variant, and with the searches
switched off (-DRRTE_SEARCH_GROUPS=0)."""
import numpy as np
import pytest

import oracle
import search_group_scenes as sg
from rrte_amd import LoweredScene, abi
from rrte_amd.renderer import Context
from test_gpu_plain_entry import _async

pytestmark = pytest.mark.gpu

W, H = 72, 40

# (id, environment, samples per pixel, expected entry, expected stats.jit_active)
VARIANTS = [
    ("plain", {}, 1, abi.ENTRY_PLAIN, 1),
    ("general", {"RRTE_JIT_PLAIN": "0"}, 1, abi.ENTRY_GENERAL, 1),
    ("topology", {"RRTE_JIT_TOPO": "1"}, 1, abi.ENTRY_GENERAL, 2),
    ("two-samples", {}, 2, abi.ENTRY_GENERAL, 1),
    ("switch-off", {"RRTE_JIT_EXTRA_OPTS": "-DRRTE_SEARCH_GROUPS=0"}, 1, abi.ENTRY_PLAIN, 1),
]

_scenes, _refs = {}, {}


def _scene(cid, w, h):
    if (cid, w, h) not in _scenes:
        _, build, lk = sg.CASE_BY_ID[cid]
        _scenes[(cid, w, h)] = LoweredScene(build(), sg.lights_of(lk), sg.camera(w, h))
    return _scenes[(cid, w, h)]


def _params(w, h, spp, mode="lambert_shadow", max_depth=1):
    prm = sg.config(w, h, mode, max_depth).lower()
    prm.samples_per_pixel = spp
    return prm


def _reference(cid, w, h, spp):
    """The oracle's frame, its shadow-ray count and how many of those rays reached their light (once per case)."""
    if (cid, w, h, spp) not in _refs:
        sc, prm = _scene(cid, w, h), _params(w, h, spp)
        ref8, _, shadow = oracle.render(sc, prm, nthreads=16, want_f32=False)
        cnt, _ = oracle.count(sc, prm, nthreads=16)
        ref8.setflags(write=False)
        _refs[(cid, w, h, spp)] = (ref8, shadow, int(cnt.shadow_rays), int(cnt.lambert_terms))
    return _refs[(cid, w, h, spp)]


def _check(cid, w, h, variant, monkeypatch):
    _, env, spp, entry, jit_active = variant
    ref8, ref_shadow, cast, lit = _reference(cid, w, h, spp)
    # no case passes vacuously: some shadow rays are occluded and some are not
    assert cast == ref_shadow and 0 < lit < cast, (cast, lit)
    for k, v in env.items():  # (the extra options are read at every compile, the rest with the context)
        monkeypatch.setenv(k, v)
    ctx = Context(0, jit=abi.JIT_ON)
    got, _, shadow, got_entry = _async(ctx, _scene(cid, w, h), _params(w, h, spp))
    active = ctx.stats().jit_active
    ctx.close()
    assert (got_entry, active) == (entry, jit_active)
    diff = int((got != ref8).sum())
    print(f"{cid} {variant[0]} {w}x{h}: bytes differing {diff}, shadow rays {shadow}/{ref_shadow}, lit {lit}")
    assert diff == 0
    assert shadow == ref_shadow


@pytest.mark.parametrize("variant", VARIANTS, ids=[v[0] for v in VARIANTS])
@pytest.mark.parametrize("cid", [c[0] for c in sg.CASES])
def test_frames_are_the_oracles(cid, variant, monkeypatch):
    _check(cid, W, H, variant, monkeypatch)


@pytest.mark.parametrize("variant", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_ragged_frame_is_the_oracles(variant, monkeypatch):
    """70x37: partial tiles on the right and at the bottom."""
    _check(f"n17-L4-occ{sg.GROUP}", 70, 37, variant, monkeypatch)


@pytest.mark.parametrize("extra", [None, "-DRRTE_SEARCH_GROUPS=0"])
def test_refcompat_depth_2_keeps_the_tie_break(extra, monkeypatch):
    """REFCOMPAT at depth 2 (the deepest at which the forward path sum is the oracle's exactly) on 33
    objects, two of them the same sphere: equal t goes to the lower index, whose material differs.  The
    linear image is compared bit for bit (the byte image passes through powf, which may differ from the
    host's by an ulp)."""
    from rrte_amd import Color, LambertianMaterial, Sphere
    objs = sg.objects(33, 32, False)
    objs[31] = Sphere((0.0, 2.2, 0.0), 0.9, LambertianMaterial(Color.rgb(0.2, 0.8, 0.8)))  # index 32's twin
    sc = LoweredScene(objs, sg.lights_of("L1"), sg.camera(W, H))
    prm = _params(W, H, 1, "refcompat", 2)
    prm.flags |= abi.FLAG_F32_LINEAR
    _, want, want_shadow = oracle.render(sc, prm, nthreads=16, linear=True)
    if extra:
        monkeypatch.setenv("RRTE_JIT_EXTRA_OPTS", extra)
    ctx = Context(0, jit=abi.JIT_ON)
    _, lin, shadow, _ = _async(ctx, sc, prm, f32=True)
    active = ctx.stats().jit_active
    ctx.close()
    assert active == 1
    assert np.array_equal(lin.view(np.uint32), want.view(np.uint32))
    assert shadow == want_shadow
