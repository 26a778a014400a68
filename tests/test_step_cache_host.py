"""The step cache (denoise(cache_interval=n): DeepCache-style reuse of the deep UNet features) on the host: what the restatement
the GPU tests compare against claims, checked against the oracle itself, and the host-side surface of the feature."""
import os
import re

import pytest
import torch

import step_cache_restatement as SC
from oracle import pipeline as OP, unet as OU
from util import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dmx_unet_step_cache_bytes", "dmx_unet_workspace_bytes_cached", "dmx_unet_forward_cached", "dmx_unet_forward_cached_graph")


@pytest.fixture(scope="module")
def P():
    return OU.make_params(OU.unet_param_spec(OU.TINY_UNET))


@pytest.fixture(scope="module")
def inputs():
    from diffute_amd.synthetic import synth_inputs
    return synth_inputs(2, 16, 16, 77, 128)


@pytest.fixture(scope="module")
def honest_7_3(P, inputs):
    """the honest cached loop of the fault cases (7 steps, interval 3, B = 2, 16 x 16, bf16 emulation): computed once"""
    return SC.cached_denoise(P, OU.TINY_UNET, *inputs, 7, 3, emulate_bf16=True)


@pytest.mark.parametrize("em", [False, True], ids=["fp32", "bf16emu"])
def test_shallow_step_on_its_own_cache_is_the_full_step(P, inputs, em):
    """a shallow forward with the cache of a full forward on the same input and timestep IS that forward: same layers on the same values"""
    lat, mask, mlat, ctx = inputs
    x = torch.cat([lat, mask, mlat], 1)
    for t in (torch.tensor(981), torch.tensor([981, 3])):
        taps = {}
        full = OU.unet_forward(P, OU.TINY_UNET, x, t, ctx, emulate_bf16=em, taps=taps)
        assert taps["up2"].shape == (2, OU.TINY_UNET["block_out_channels"][1], 16, 16)
        assert torch.equal(SC.shallow_forward(P, OU.TINY_UNET, x, t, ctx, taps["up2"], emulate_bf16=em), full)


def test_interval_1_is_the_plain_loop(P, inputs):
    assert torch.equal(SC.cached_denoise(P, OU.TINY_UNET, *inputs, 3, 1, emulate_bf16=True),
                       OP.denoise(P, OU.TINY_UNET, *inputs, 3, "ddim", emulate_bf16=True))


@pytest.mark.parametrize("steps,interval", [(5, 2), (6, 3), (7, 3)])
def test_bf16_bounds_of_the_plain_loop_carry_over(P, inputs, steps, interval, honest_7_3):
    """the cached loops' bf16-emulated result sits 5.9e-3 .. 6.3e-3 from their fp32 result (measured), the plain 4-step loop's 5.7e-3:
    the GPU bounds of test_tiny_denoise_loops (2e-2 vs bf16 emulation, 5e-2 vs fp32) hold for cached loops with the same margin"""
    f32 = SC.cached_denoise(P, OU.TINY_UNET, *inputs, steps, interval)
    emu = honest_7_3 if (steps, interval) == (7, 3) else SC.cached_denoise(P, OU.TINY_UNET, *inputs, steps, interval, emulate_bf16=True)
    e = rel_l2(emu, f32)
    print(f"cached loop ({steps} steps, interval {interval}): bf16-emulated vs fp32 rel-L2 {e:.2e}")
    assert e <= 1e-2


@pytest.mark.parametrize("fault,refresh", [("cache never refreshed after step 0", lambda i: i == 0),
                                           ("refresh one step late", lambda i: i % 3 == 1),
                                           ("no caching at all", lambda i: True)],
                         ids=["never_refreshed", "one_step_late", "no_caching"])
def test_injected_faults_are_visible(P, inputs, honest_7_3, fault, refresh):
    """a loop that caches on another schedule is far (measured 4.6e-2 / 8.2e-2 / 9.1e-2) from the honest one: the GPU loop bound of
    2e-2 tells them apart"""
    bad = SC.cached_denoise(P, OU.TINY_UNET, *inputs, 7, 3, emulate_bf16=True, refresh=refresh)
    e = rel_l2(bad, honest_7_3)
    print(f"{fault}: rel-L2 {e:.2e} from the honest cached loop")
    assert e > 2e-2


def test_stale_cache_is_far_from_the_full_forward(P, inputs):
    """a shallow forward at (x', 961) on the cache of (x, 981) is ~0.27 from the full forward at (x', 961): the margin by which the GPU
    test tells 'the deep part was skipped' from 'it ran anyway'"""
    lat, mask, mlat, ctx = inputs
    x = torch.cat([lat, mask, mlat], 1)
    x2 = torch.cat([lat + 0.3 * torch.roll(lat, 1, 0), mask, mlat], 1)
    taps = {}
    OU.unet_forward(P, OU.TINY_UNET, x, torch.tensor(981), ctx, emulate_bf16=True, taps=taps)
    sh = SC.shallow_forward(P, OU.TINY_UNET, x2, torch.tensor(961), ctx, taps["up2"], emulate_bf16=True)
    full = OU.unet_forward(P, OU.TINY_UNET, x2, torch.tensor(961), ctx, emulate_bf16=True)
    e = rel_l2(sh, full)
    print(f"stale cache: rel-L2 {e:.2e} from the full forward")
    assert e > 0.1


def test_new_symbols_declared_and_exported():
    from diffute_amd import _cabi
    hdr = open(os.path.join(ROOT, "include", "diffute_hip.h")).read()
    declared = set(re.findall(r"\b(dmx_[a-z0-9_]+)\s*\(", hdr))
    for sym in NEW_SYMBOLS:
        assert sym in declared and sym in set(_cabi.exported_symbols())
        for elem in ("bf16", "fp16"):
            assert hasattr(_cabi.lib(elem), sym), f"{sym} not exported by the {elem} build"
    assert re.search(r"#define\s+DMX_STEP_CACHE_FILL\s+1\b", hdr) and re.search(r"#define\s+DMX_STEP_CACHE_USE\s+2\b", hdr)
    assert (_cabi.STEP_CACHE_FILL, _cabi.STEP_CACHE_USE) == (1, 2)


@pytest.mark.parametrize("bad", [0, -1, 1.5, "2"])
def test_bad_cache_interval_raises_before_the_device(bad):
    import diffute_amd as D
    x = torch.zeros(1, 4, 8, 8); m = torch.zeros(1, 1, 8, 8); ctx = torch.zeros(1, 77, 128)
    with pytest.raises(ValueError, match="cache_interval"):
        D.denoise(None, None, x, m, x, ctx, 2, cache_interval=bad)
    with pytest.raises(ValueError, match="cache_interval"):
        D.edit_latents(None, None, None, None, x, m, ctx, 2, cache_interval=bad)


def test_shallow_flops():
    """flops.unet_flops(shallow=True): the default is unchanged, the shallow step of the full-size UNet is about 40 % of a forward"""
    import diffute_amd as D
    from diffute_amd import flops
    cfg = D.models._Config(**D.SD2_INPAINT_UNET_CONFIG)
    full = flops.unet_flops(cfg, 4, 64, 64, 577, cached_ctx_kv=True, phase_upsample=True)
    assert full == flops.unet_flops(cfg, 4, 64, 64, 577, cached_ctx_kv=True, phase_upsample=True, shallow=False)
    sh = flops.unet_flops(cfg, 4, 64, 64, 577, cached_ctx_kv=True, phase_upsample=True, shallow=True)
    print(f"shallow step: {sh / full:.3f} of a full forward's FLOPs")
    assert 0.3 < sh / full < 0.5
