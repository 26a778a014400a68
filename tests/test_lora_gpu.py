"""LoRA on the GPU (diffute_amd/lora.py, csrc/lora.hip), against tests/lora_restatement.py:

 1. dmx_lora_merge per element into guarded, sentinel-filled staging: (33,7), (320,320), (320,1024), (1280,1280), each with r = 1, 3, 16, 64 and one
    target of three adapters, bound (R+3) 2^-24 (|W0| + sum |s| sum |B||A|); two runs and alone-vs-full-table are bit-equal;
 2. dmx_lora_grads per element from a test-owned dW, bounds (N+3) / (K+3) 2^-24 |s| sum |.||.|; an inf and a NaN in dW reach their column of dA and
    their row of dB and nothing else; bit-equal run to run and alone versus in the full table;
 3. the tiny UNet with an adapter equals, bit for bit, a fresh model loaded from merged_lora_weights() (also with proj_out / ff targets: the
    LayerNorm-folded and composed packs); B = 0, weight 0, disable_adapters and delete_adapter give the base forward; the base bytes never change;
 4. switching a -> b -> a with the SAME context tensor object (the K/V cache must notice the epoch), and a weighted sum of two adapters;
 5. training: base grads None and bytes unchanged, .grad of A / B within bound 2 of the restatement on the exported dW, the loss equal to the merged
    model's, 30 AdamW steps lower the loss, the fp16 build under a GradScaler with a forced overflow, EMAModel over the LoRA Parameters;
 6. save_lora_weights / load_lora_weights into a fresh model: same forward, the file's keys and shapes as specified."""
import ctypes

import numpy as np
import pytest
import torch

import ema_restatement as ER
import lora_restatement as LR
from util import SENTINEL_BITS, assert_guard_intact

pytestmark = pytest.mark.gpu
ELEMS = ["bf16", "fp16"]
TINY_UNET = dict(block_out_channels=(64, 128, 256, 256), attention_head_dim=(1, 2, 4, 4), cross_attention_dim=128)
TINY_VAE = dict(block_out_channels=(64, 128, 128, 128), layers_per_block=1)
GUARD = 64
MORE_TARGETS = ("to_q", "to_k", "to_v", "to_out.0", "proj_out", "ff.net.0.proj", "ff.net.2")


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def guarded(shape, dev):
    """-> (sentinel-filled fp32 buffer with guard bands, the contiguous view of `shape` inside it)"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL_BITS[torch.float32][1], dtype=torch.int32, device=dev).view(torch.float32)
    return buf, buf[GUARD:GUARD + n].view(shape)


def run_table(entry, recs_py, dev):
    """one launch of dmx_lora_merge / dmx_lora_grads of the active build over records given as dicts of tensors and scalars"""
    from diffute_amd import _cabi, ops
    lib = ops.lib()
    recs = (_cabi.LoraRec * len(recs_py))()
    for q, r in zip(recs, recs_py):
        q.A, q.B, q.W, q.dst = r["A"].data_ptr(), r["B"].data_ptr(), r["W"].data_ptr(), r["dst"].data_ptr()
        q.dst2 = r["dst2"].data_ptr() if r.get("dst2") is not None else None
        q.N, q.K, q.r, q.s, q.count = r["B"].shape[0], r["A"].shape[1], r["A"].shape[0], float(r["s"]), r.get("count", 0)
    table = torch.empty(len(recs_py) * ctypes.sizeof(_cabi.LoraRec), dtype=torch.uint8, device=dev)
    _cabi.check(getattr(lib, entry)(recs, len(recs_py), _cabi.ptr(table), table.numel(), _cabi.current_stream()), entry, lib)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 1. merge
def merge_targets(shape, dev):
    """the targets of one shape: r = 1, 3, 16, 64 alone and three adapters (3, 16, 1) summed -> [(W0, [(A, B, s)] numpy, device copies)]"""
    N, K = shape
    out = []
    for i, ranks in enumerate([[r] for r in LR.RANKS] + [[3, 16, 1]]):
        W0, ads = LR.make_case(N, K, ranks, seed=100 + i)
        out.append((W0, ads, torch.from_numpy(W0).to(dev), [(torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev), s) for A, B, s in ads]))
    return out


def merge_records(targets, dsts):
    recs = []
    for (_, _, W0d, adsd), dst in zip(targets, dsts):
        for j, (A, B, s) in enumerate(adsd):
            recs.append(dict(A=A, B=B, W=W0d, dst=dst, s=s, count=len(adsd) if j == 0 else 0))
    return recs


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("shape", LR.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_merge_per_element(cuda, shape, elem):
    from diffute_amd import ops
    targets = merge_targets(shape, cuda)
    with ops.element_type(elem):
        outs = [guarded(shape, cuda) for _ in targets]
        run_table("dmx_lora_merge", merge_records(targets, [v for _, v in outs]), cuda)
        again = [guarded(shape, cuda) for _ in targets]
        run_table("dmx_lora_merge", merge_records(targets, [v for _, v in again]), cuda)
        alone = []
        for t in targets:
            b, v = guarded(shape, cuda)
            run_table("dmx_lora_merge", merge_records([t], [v]), cuda)
            alone.append(v)
    for i, ((W0, ads, _, _), (buf, view)) in enumerate(zip(targets, outs)):
        name = f"merge {shape} target {i} ({elem})"
        assert_guard_intact(buf, view, name=name)                       # nothing outside, every element written
        got = view.cpu().numpy().astype(np.float64)
        err, bound = np.abs(got - LR.merge64(W0, ads)), LR.merge_bound(W0, ads)
        print(f"{name}: worst |err| / bound = {(err / bound).max():.3f}")
        assert (err <= bound).all(), f"{name}: {(err > bound).sum()} elements outside the bound, worst ratio {(err / bound).max():.3f}"
        assert same_bits(view, again[i][1]), f"{name}: two runs differ"
        assert same_bits(view, alone[i]), f"{name}: alone differs from the full table"


# ---------------------------------------------------------------------------------------------- 2. grads
def grad_cases(shape, dev):
    """r = 1, 3, 16, 64 on a clean dW, r = 3 on a dW holding an inf, r = 3 on one holding a NaN -> [(dW, A, B, s, device copies, bad index or None)]"""
    N, K = shape
    out = []
    for i, (r, bad) in enumerate([(r, None) for r in LR.RANKS] + [(3, np.inf), (3, np.nan)]):
        _, ads = LR.make_case(N, K, [r], seed=200 + i)
        A, B, s = ads[0]
        dW = LR.make_dw(N, K, 300 + i)
        at = None
        if bad is not None:
            at = (N // 2, K // 3)
            dW[at] = bad
        out.append((dW, A, B, s, tuple(torch.from_numpy(x).to(dev) for x in (dW, A, B)), at))
    return out


def grad_records(cases, outs):
    return [dict(A=d[1], B=d[2], W=d[0], s=s, dst=oa[1], dst2=ob[1]) for (_, _, _, s, d, _), (oa, ob) in zip(cases, outs)]


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("shape", LR.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_grads_per_element(cuda, shape, elem):
    from diffute_amd import ops
    N, K = shape
    cases = grad_cases(shape, cuda)

    def outputs():
        return [(guarded(c[1].shape, cuda), guarded(c[2].shape, cuda)) for c in cases]
    with ops.element_type(elem):
        outs = outputs()
        run_table("dmx_lora_grads", grad_records(cases, outs), cuda)
        again = outputs()
        run_table("dmx_lora_grads", grad_records(cases, again), cuda)
        alone = outputs()
        for c, o in zip(cases, alone):
            run_table("dmx_lora_grads", grad_records([c], [o]), cuda)
    for i, ((dW, A, B, s, _, at), ((bufa, va), (bufb, vb))) in enumerate(zip(cases, outs)):
        name = f"grads {shape} case {i} ({elem})"
        assert_guard_intact(bufa, va, name=name + " dA"); assert_guard_intact(bufb, vb, name=name + " dB")
        with np.errstate(invalid="ignore"):
            rA, rB = LR.grads64(dW, A, B, s)
            bA, bB = LR.grads_bound(dW, A, B, s)
        for what, got, ref, bound in (("dA", va, rA, bA), ("dB", vb, rB, bB)):
            g = got.cpu().numpy().astype(np.float64)
            fin = np.isfinite(ref)
            assert np.array_equal(np.isfinite(g), fin), f"{name} {what}: non-finite values are not where the restatement has them"
            with np.errstate(invalid="ignore"):
                err = np.abs(g - ref)
            print(f"{name} {what}: worst |err| / bound = {(err[fin] / bound[fin]).max():.3f}")
            assert (err[fin] <= bound[fin]).all(), f"{name} {what}: worst ratio {(err[fin] / bound[fin]).max():.3f}"
        if at is not None:                                               # the inf / NaN reached its column of dA and its row of dB, nothing else
            ga, gb = va.cpu().numpy(), vb.cpu().numpy()
            assert not np.isfinite(ga[:, at[1]]).any() and np.isfinite(np.delete(ga, at[1], 1)).all(), name
            assert not np.isfinite(gb[at[0]]).any() and np.isfinite(np.delete(gb, at[0], 0)).all(), name
        for what, k in (("dA", 0), ("dB", 1)):
            assert same_bits(outs[i][k][1], again[i][k][1]), f"{name} {what}: two runs differ"
            assert same_bits(outs[i][k][1], alone[i][k][1]), f"{name} {what}: alone differs from the full table"


def test_table_refusals(cuda):
    from diffute_amd import _cabi, ops
    lib = ops.lib()
    t = merge_targets((33, 7), cuda)[0]
    _, v = guarded((33, 7), cuda)
    rec = merge_records([t], [v])
    recs = (_cabi.LoraRec * 1)()
    q = recs[0]
    q.A, q.B, q.W, q.dst, q.N, q.K, q.r, q.s, q.count = rec[0]["A"].data_ptr(), rec[0]["B"].data_ptr(), rec[0]["W"].data_ptr(), v.data_ptr(), 33, 7, 1, 1.0, 2
    table = torch.empty(ctypes.sizeof(_cabi.LoraRec), dtype=torch.uint8, device=cuda)
    assert lib.dmx_lora_merge(recs, 1, _cabi.ptr(table), table.numel(), _cabi.current_stream()) != 0 and b"opens a target" in lib.dmx_last_error()
    q.count = 1
    assert lib.dmx_lora_merge(recs, 1, _cabi.ptr(table), table.numel() - 1, _cabi.current_stream()) != 0 and b"table" in lib.dmx_last_error()
    assert lib.dmx_lora_grads(recs, 1, _cabi.ptr(table), table.numel(), _cabi.current_stream()) != 0 and b"null pointer" in lib.dmx_last_error()
    q.r = 0
    assert lib.dmx_lora_merge(recs, 1, _cabi.ptr(table), table.numel(), _cabi.current_stream()) != 0
    torch.cuda.synchronize()
    assert (v.cpu().view(torch.int32) == SENTINEL_BITS[torch.float32][1]).all()          # a refused call launches nothing


# ---------------------------------------------------------------------------------------------- the tiny UNet
@pytest.fixture(scope="module")
def inputs(cuda):
    from diffute_amd.synthetic import synth_inputs
    lat, mask, mlat, ctx = synth_inputs(2, 16, 16, 77, 128, seed=3, device=cuda)
    return torch.cat([lat, mask, mlat], 1), torch.tensor([981, 17], device=cuda), ctx


def tiny():
    import diffute_amd as D
    return D.UNet2DConditionModel(**TINY_UNET).cuda()


def randomise(unet, name, seed, scale=0.05):
    """random non-zero A and B (written on the Parameters under no_grad: the version counters move)"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in unet.lora_parameters(name):
            p.copy_((torch.randn(p.shape, generator=g) * scale).to(p.device))


@torch.no_grad()
def fwd(unet, inputs):
    return unet(*inputs).sample.clone()


def merged_twin(unet):
    """a fresh model (same seed: same base) whose Parameters are loaded from merged_lora_weights()"""
    m = tiny()
    sd = m.state_dict()
    merged = unet.merged_lora_weights()
    assert merged and set(merged) <= set(sd)
    sd.update({k: v.clone() for k, v in merged.items()})
    m.load_state_dict(sd)
    return m


def base_bytes(unet):
    return {k: p.detach().clone() for k, p in unet.named_parameters() if not k.startswith("lora_adapters.")}


def assert_base_unchanged(unet, before):
    now = dict(unet.named_parameters())
    assert all(same_bits(now[k], v) for k, v in before.items()), "a base Parameter was written"


@pytest.fixture(scope="module")
def base_forward(cuda, inputs):
    return fwd(tiny(), inputs)


@pytest.mark.parametrize("targets", [None, MORE_TARGETS], ids=["default", "with_ff_proj_out"])
def test_model_equals_merged_twin(cuda, inputs, base_forward, targets):
    import diffute_amd as D
    unet = tiny()
    before = base_bytes(unet)
    cfg = D.LoraConfig(r=4, lora_alpha=8) if targets is None else D.LoraConfig(r=4, lora_alpha=8, target_modules=targets)
    unet.add_adapter(cfg, adapter_name="a")
    assert same_bits(fwd(unet, inputs), base_forward), "B = 0 must be the base model"
    randomise(unet, "a", 1)
    out = fwd(unet, inputs)
    assert not same_bits(out, base_forward)
    assert same_bits(out, fwd(merged_twin(unet), inputs)), "adapter forward differs from the model loaded with the merged weights"
    # the merged values themselves, per element against fp64
    merged = unet.merged_lora_weights()
    assert len(merged) == (128 if targets is None else 128 + 48)
    from diffute_amd.lora import merge_scale
    ad = unet._lora["a"]
    worst = 0.0
    for k, A, B, alpha in ad.items():
        ads = [(A.detach().cpu().numpy(), B.detach().cpu().numpy(), np.float32(merge_scale(1.0, alpha, A.shape[0])))]
        W0 = before[k].cpu().numpy()
        err, bound = np.abs(merged[k].cpu().numpy().astype(np.float64) - LR.merge64(W0, ads)), LR.merge_bound(W0, ads)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), f"{k}: merged weight outside the bound (ratio {(err / bound).max():.3f})"
    print(f"merged weights of the tiny UNet: worst |err| / bound = {worst:.3f}")
    # every way back to the base model
    unet.set_adapters(["a"], weights=[0.0])
    assert same_bits(fwd(unet, inputs), base_forward), "weight 0"
    unet.set_adapters("a")
    assert same_bits(fwd(unet, inputs), out)
    unet.disable_adapters()
    assert same_bits(fwd(unet, inputs), base_forward), "disable_adapters"
    unet.enable_adapters()
    assert same_bits(fwd(unet, inputs), out)
    unet.delete_adapter("a")
    assert same_bits(fwd(unet, inputs), base_forward), "delete_adapter"
    assert unet.merged_lora_weights() == {}
    assert_base_unchanged(unet, before)


def test_removed_adapters_give_back_the_arena(cuda, inputs):
    import diffute_amd as D
    unet = tiny()
    fwd(unet, inputs)
    arena0 = unet._arena.clone()
    unet.add_adapter(D.LoraConfig(r=3, lora_alpha=3, target_modules=MORE_TARGETS), adapter_name="a")
    randomise(unet, "a", 2)
    fwd(unet, inputs)
    assert not torch.equal(unet._arena, arena0)
    unet.delete_adapter("a")
    fwd(unet, inputs)
    assert torch.equal(unet._arena, arena0), "the arena is not the base model's after the adapter left"


def test_switching(cuda, inputs, base_forward):
    import diffute_amd as D
    unet = tiny()
    before = base_bytes(unet)
    unet.add_adapter(D.LoraConfig(r=4, lora_alpha=4), adapter_name="a")
    unet.add_adapter(D.LoraConfig(r=2, lora_alpha=6, target_modules=("to_k", "to_v", "ff.net.2")), adapter_name="b")
    randomise(unet, "a", 3); randomise(unet, "b", 4)
    x, t, ctx = inputs                                     # the SAME context tensor object every time
    unet.set_adapters("a"); a1 = fwd(unet, (x, t, ctx)); ref_a = fwd(merged_twin(unet), (x, t, ctx))
    epoch = unet._epoch
    unet.set_adapters("b"); b1 = fwd(unet, (x, t, ctx)); ref_b = fwd(merged_twin(unet), (x, t, ctx))
    assert unet._epoch == epoch + 1, "a switch is one arena change, not a re-pack"
    unet.set_adapters("a"); a2 = fwd(unet, (x, t, ctx))
    assert same_bits(a1, a2) and same_bits(a1, ref_a) and same_bits(b1, ref_b)
    assert not same_bits(a1, b1) and not same_bits(a1, base_forward) and not same_bits(b1, base_forward)
    packed = unet._packed_sig
    unet.set_adapters(["a", "b"], [0.5, 2.0])
    ab = fwd(unet, (x, t, ctx))
    assert same_bits(ab, fwd(merged_twin(unet), (x, t, ctx))) and not same_bits(ab, a1) and not same_bits(ab, b1)
    assert unet._packed_sig == packed
    assert unet.active_adapters == ["a", "b"]
    # a write to the base Parameters: the full re-pack, the adapters on top
    with torch.no_grad():
        dict(unet.named_parameters())["conv_in.bias"].add_(0.25)
    moved = fwd(unet, (x, t, ctx))
    twin = merged_twin(unet)
    with torch.no_grad():
        dict(twin.named_parameters())["conv_in.bias"].add_(0.25)
    assert same_bits(moved, fwd(twin, (x, t, ctx))) and not same_bits(moved, ab)
    with torch.no_grad():
        dict(unet.named_parameters())["conv_in.bias"].sub_(0.25)
    before["conv_in.bias"] = dict(unet.named_parameters())["conv_in.bias"].detach().clone()
    # fuse_lora writes the merged values and drops the adapters
    unet.set_adapters("a")
    unet.fuse_lora()
    assert unet.active_adapters == [] and unet.lora_parameters() == []
    assert same_bits(fwd(unet, (x, t, ctx)), fwd(merged_twin_from(unet), (x, t, ctx)))
    changed = [k for k, v in before.items() if not same_bits(dict(unet.named_parameters())[k], v)]
    assert len(changed) == 128 and all(".attentions." in k for k in changed)


def merged_twin_from(unet):
    m = tiny()
    m.load_state_dict({k: v for k, v in unet.state_dict().items() if not k.startswith("lora_adapters.")})
    return m


# ---------------------------------------------------------------------------------------------- 5. training
@pytest.fixture(scope="module")
def train_setup(cuda):
    import diffute_amd as D
    vae = D.AutoencoderKL(**TINY_VAE).cuda().requires_grad_(False)
    gen = torch.Generator(device=cuda).manual_seed(7)
    B = 2
    masks = torch.zeros(B, 1, 128, 128, device=cuda); masks[0, :, 32:64, 16:112] = 1; masks[1, :, 80:104, 8:72] = 1
    batch = dict(pixel_values=torch.rand(B, 3, 128, 128, device=cuda, generator=gen) * 2 - 1,
                 masked_images=torch.rand(B, 3, 128, 128, device=cuda, generator=gen) * 2 - 1, masks=masks,
                 ocr_embeddings=torch.randn(B, 77, 128, device=cuda, generator=gen))
    draws = dict(noise=torch.randn(B, 4, 16, 16, device=cuda, generator=gen), timesteps=torch.tensor([700, 150], device=cuda),
                 enc_noise=torch.randn(B, 4, 16, 16, device=cuda, generator=gen), enc_noise_masked=torch.randn(B, 4, 16, 16, device=cuda, generator=gen))
    return vae, D.DDPMScheduler(), batch, draws


class ProbeAdamW(torch.optim.AdamW):
    """keeps the gradients the step saw (train_step clears them afterwards) and the values they were taken at"""

    def step(self, *a, **k):
        self.at = [p.detach().clone() for g in self.param_groups for p in g["params"]]
        self.seen = [None if p.grad is None else p.grad.detach().clone() for g in self.param_groups for p in g["params"]]
        return super().step(*a, **k)


def check_lora_grads(unet, name, seen, at, weight=1.0):
    """`.grad` of every A / B (taken at the values `at`) against the restatement applied to the dW exported from the gradient arena (bound 2)"""
    from diffute_amd.lora import merge_scale
    worst = 0.0
    items = unet._lora[name].items()
    assert len(seen) == 2 * len(items) and all(g is not None for g in seen)
    dWs = unet._export_arena(unet._tb["grads"], [torch.empty(B.shape[0], A.shape[1], device=A.device) for _, A, B, _ in items], [k for k, _, _, _ in items])
    for i, (k, _, _, alpha) in enumerate(items):
        dW, A, B = dWs[i].cpu().numpy(), at[2 * i].cpu().numpy(), at[2 * i + 1].cpu().numpy()
        s = np.float32(merge_scale(weight, alpha, A.shape[0]))
        rA, rB = LR.grads64(dW, A, B, s)
        bA, bB = LR.grads_bound(dW, A, B, s)
        for got, ref, bound, what in ((seen[2 * i], rA, bA, "dA"), (seen[2 * i + 1], rB, bB, "dB")):
            err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
            assert (err <= bound).all(), f"{k} {what}: outside the bound"
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert np.abs(rA).max() > 0 and np.abs(rB).max() > 0, f"{k}: zero gradient"
    print(f"LoRA gradients of the tiny UNet: worst |err| / bound = {worst:.3f}")


@pytest.mark.parametrize("weighted", [False, True], ids=["mse", "min_snr_box"])
def test_train_step_gradients_and_loss(cuda, train_setup, weighted):
    import diffute_amd as D
    from diffute_amd.training import train_step
    vae, sch, batch, draws = train_setup
    kw = dict(snr_gamma=5.0, mask_weight=4.0) if weighted else {}
    unet = tiny()
    before = base_bytes(unet)
    unet.add_adapter(D.LoraConfig(r=4, lora_alpha=8, target_modules=MORE_TARGETS), adapter_name="a")
    randomise(unet, "a", 5)
    twin = merged_twin(unet)
    a_before = [p.detach().clone() for p in unet.lora_parameters("a")]
    opt = ProbeAdamW(unet.lora_parameters(), lr=1e-3)
    out = train_step(unet, vae, sch, opt, batch, **draws, max_grad_norm=None, **kw)
    base = {k: p for k, p in unet.named_parameters() if not k.startswith("lora_adapters.")}
    assert all(p.grad is None and not p.requires_grad for p in base.values())
    assert_base_unchanged(unet, before)
    check_lora_grads(unet, "a", opt.seen, opt.at)
    assert any(not same_bits(p, q) for p, q in zip(unet.lora_parameters("a"), a_before)), "the step moved nothing"
    assert set(id(p) for p in opt.state) == set(id(p) for p in unet.lora_parameters()), "optimizer state for the LoRA Parameters only"
    ref = train_step(twin, vae, sch, torch.optim.SGD(twin.parameters(), lr=0.0), batch, **draws, max_grad_norm=None, **kw)
    assert same_bits(out["loss"], ref["loss"]), "the loss differs from the merged model's training forward"
    with pytest.raises(RuntimeError, match="LoRA"):
        D.FusedAdamW(unet)


def test_full_finetune_after_the_adapters_left(cuda, train_setup):
    """a model whose adapters were all deleted trains its base weights again: the loss and every gradient of a model that never had one"""
    import diffute_amd as D
    from diffute_amd.training import train_step
    vae, sch, batch, draws = train_setup
    unet = tiny()
    unet.add_adapter(D.LoraConfig(r=2, lora_alpha=2), adapter_name="a")
    randomise(unet, "a", 9)
    train_step(unet, vae, sch, torch.optim.SGD(unet.lora_parameters(), lr=1e-2), batch, **draws)
    unet.delete_adapter("a")
    unet.requires_grad_(True)
    outs = []
    for m in (unet, tiny()):
        opt = ProbeAdamW(m.parameters(), lr=0.0, weight_decay=0.0)
        outs.append((train_step(m, vae, sch, opt, batch, **draws, max_grad_norm=None)["loss"], opt.seen))
    assert same_bits(outs[0][0], outs[1][0])
    assert len(outs[0][1]) == len(outs[1][1]) and all(g is not None and same_bits(g, h) for g, h in zip(*[o[1] for o in outs]))


def test_thirty_steps_lower_the_loss(cuda, train_setup):
    import diffute_amd as D
    from diffute_amd.training import train_step
    vae, sch, batch, draws = train_setup
    unet = tiny()
    unet.add_adapter(D.LoraConfig(r=8, lora_alpha=8), adapter_name="default")
    opt = torch.optim.AdamW(unet.lora_parameters(), lr=1e-3)
    losses = [float(train_step(unet, vae, sch, opt, batch, **draws)["loss"]) for _ in range(30)]
    print(f"loss {losses[0]:.6f} -> {losses[-1]:.6f}")
    assert losses[-1] < losses[0]
    assert len(opt.state) == len(unet.lora_parameters()) == 256


def test_fp16_scaler_and_overflow(cuda, train_setup):
    import diffute_amd as D
    from diffute_amd.training import train_step
    vae, sch, batch, draws = train_setup
    unet = tiny().to(dtype=torch.float16)
    unet.add_adapter(D.LoraConfig(r=4, lora_alpha=4), adapter_name="a")
    randomise(unet, "a", 6)
    scaler = D.GradScaler(init_scale=2.0 ** 16)
    opt = ProbeAdamW(unet.lora_parameters(), lr=1e-3)
    start = [p.detach().clone() for p in unet.lora_parameters()]
    out = train_step(unet, vae, sch, opt, batch, **draws, max_grad_norm=None, scaler=scaler)
    assert torch.isfinite(out["loss"]) and scaler.get_scale() == 2.0 ** 16
    check_lora_grads_scaled(unet, "a", opt.seen, opt.at, 2.0 ** 16)
    assert any(not same_bits(p, q) for p, q in zip(unet.lora_parameters(), start))
    mid = [p.detach().clone() for p in unet.lora_parameters()]
    bad = dict(draws, noise=draws["noise"].clone()); bad["noise"][0, 0, 0, 0] = float("inf")
    opt.seen = None
    train_step(unet, vae, sch, opt, batch, **bad, max_grad_norm=None, scaler=scaler)
    assert opt.seen is None, "the overflowed step was not skipped"
    assert scaler.get_scale() == 2.0 ** 15
    assert all(same_bits(p, q) for p, q in zip(unet.lora_parameters(), mid)), "A / B changed in a skipped step"


def check_lora_grads_scaled(unet, name, seen, at, scale):
    """the step saw g / S (torch's unscale: one multiplication by the exactly representable 1 / S, exact here): compare S * seen with the
    restatement on the arena's dW, which holds the scaled gradient"""
    check_lora_grads(unet, name, [g * scale for g in seen], at)


def test_ema_over_lora_parameters(cuda):
    import diffute_amd as D
    unet = tiny()
    unet.add_adapter(D.LoraConfig(r=4, lora_alpha=4), adapter_name="a")
    randomise(unet, "a", 7)
    params = unet.lora_parameters()
    ema = D.EMAModel(params, decay=0.75)
    shadows = [p.detach().clone() for p in params]
    for n in range(1, 4):
        randomise(unet, "a", 10 + n)
        ema.step(params)
        ER.step(shadows, params, ER.get_decay(n, decay=0.75))
    assert all(same_bits(s, r) for s, r in zip(ema.shadow_params, shadows))
    assert not same_bits(shadows[0], params[0])


# ---------------------------------------------------------------------------------------------- 6. save / load
def test_save_load(cuda, inputs, tmp_path):
    import diffute_amd as D
    from safetensors import safe_open
    unet = tiny()
    unet.add_adapter(D.LoraConfig(r=4, lora_alpha=12, target_modules=MORE_TARGETS), adapter_name="a")
    randomise(unet, "a", 8)
    out = fwd(unet, inputs)
    path = unet.save_lora_weights(str(tmp_path / "adapter"), "a")
    assert path.endswith("pytorch_lora_weights.safetensors")
    shapes = {k[:-len(".weight")]: tuple(p.shape) for k, p in unet.named_parameters() if k in unet._lora["a"].layers}
    with safe_open(path, framework="pt") as f:
        keys = set(f.keys())
        assert f.metadata()["lora_alpha"] == "12.0"
        for m, (N, K) in shapes.items():
            assert tuple(f.get_tensor(f"unet.{m}.lora_A.weight").shape) == (4, K) and tuple(f.get_tensor(f"unet.{m}.lora_B.weight").shape) == (N, 4)
            al = f.get_tensor(f"unet.{m}.alpha")
            assert al.ndim == 0 and float(al) == 12.0
    assert len(shapes) == 176 and keys == {f"unet.{m}.{x}" for m in shapes for x in ("lora_A.weight", "lora_B.weight", "alpha")}
    fresh = tiny()
    fresh.load_lora_weights(str(tmp_path / "adapter"), adapter_name="loaded")
    assert fresh.active_adapters == ["loaded"]
    assert same_bits(fwd(fresh, inputs), out)
    again = tiny()
    again.load_lora_weights(path, adapter_name="a")                    # the file itself, and through a state dict
    third = tiny()
    third.load_lora_weights(unet.lora_state_dict("a"), adapter_name="a")
    assert same_bits(fwd(again, inputs), out) and same_bits(fwd(third, inputs), out)
