"""LoRA on the host: the fp64 restatement (tests/lora_restatement.py) pinned to torch autograd, honest fp32 evaluations inside the bounds the
GPU test applies to the kernels, the injected faults outside them, and the key handling / refusals of diffute_amd/lora.py (no GPU needed)."""
import numpy as np
import pytest
import torch

import lora_restatement as LR

HOST_SHAPES = [(33, 7), (64, 64), (40, 96)]


# ---------------------------------------------------------------------------------------------- the restatement is what autograd computes
@pytest.mark.parametrize("shape", HOST_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_is_autograd(shape):
    N, K = shape
    W0, ads = LR.make_case(N, K, [3], seed=5, scales=[0.75])
    A, B, s = ads[0]
    g = torch.Generator().manual_seed(1)
    x = torch.randn(11, K, dtype=torch.float64, generator=g)
    up = torch.randn(11, N, dtype=torch.float64, generator=g)
    W0t = torch.tensor(W0, dtype=torch.float64)
    At = torch.tensor(A, dtype=torch.float64, requires_grad=True)
    Bt = torch.tensor(B, dtype=torch.float64, requires_grad=True)
    W = (W0t + float(s) * Bt @ At)
    W.retain_grad()
    assert np.abs(W.detach().numpy() - LR.merge64(W0, ads)).max() <= 1e-12
    ((x @ W.T) * up).sum().backward()
    dW = W.grad.numpy()
    d = dW.astype(np.float64)
    dA, dB = float(s) * (B.astype(np.float64).T @ d), float(s) * (d @ A.astype(np.float64).T)
    assert np.abs(At.grad.numpy() - dA).max() <= 1e-12 * max(1.0, np.abs(dA).max())
    assert np.abs(Bt.grad.numpy() - dB).max() <= 1e-12 * max(1.0, np.abs(dB).max())
    # (grads64 takes a float32 dW like the kernel: on a float32-representable dW it is the same expression)
    dW32 = dW.astype(np.float32)
    rA, rB = LR.grads64(dW32, A, B, s)
    d32 = dW32.astype(np.float64)
    assert np.array_equal(rA, float(s) * (B.astype(np.float64).T @ d32)) and np.array_equal(rB, float(s) * (d32 @ A.astype(np.float64).T))


# ---------------------------------------------------------------------------------------------- fp32 stays inside, faults do not
@pytest.mark.parametrize("order", LR.ORDERS)
@pytest.mark.parametrize("ranks", [[1], [3], [16], [2, 5, 3]], ids=lambda r: "r" + "+".join(map(str, r)))
@pytest.mark.parametrize("shape", HOST_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fp32_inside_bounds(shape, ranks, order):
    N, K = shape
    W0, ads = LR.make_case(N, K, ranks, seed=7)
    err = np.abs(LR.merge32(W0, ads, order).astype(np.float64) - LR.merge64(W0, ads))
    assert (err <= LR.merge_bound(W0, ads)).all(), f"merge {shape} {ranks} {order}: worst ratio {(err / LR.merge_bound(W0, ads)).max():.3f}"
    dW = LR.make_dw(N, K, 8)
    for A, B, s in ads:
        dA, dB = LR.grads32(dW, A, B, s, order)
        rA, rB = LR.grads64(dW, A, B, s)
        bA, bB = LR.grads_bound(dW, A, B, s)
        assert (np.abs(dA - rA) <= bA).all() and (np.abs(dB - rB) <= bB).all(), f"grads {shape} {ranks} {order}"


@pytest.mark.parametrize("fault", LR.MERGE_FAULTS)
@pytest.mark.parametrize("shape", HOST_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_merge_faults_break_the_bound(shape, fault):
    N, K = shape
    W0, ads = LR.make_case(N, K, [3, 2], seed=9, scales=[0.5, 2.0])
    err = np.abs(LR.fault_merge(W0, ads, fault) - LR.merge64(W0, ads))
    assert (err > LR.merge_bound(W0, ads)).any(), f"{fault} on {shape} stays inside the bound"
    if fault == "dropped_tail_row":                                  # ... and only where the fault is
        assert (err[:-1] == 0).all() and (err[-1] > LR.merge_bound(W0, ads)[-1]).all()


@pytest.mark.parametrize("fault", LR.GRAD_FAULTS)
@pytest.mark.parametrize("shape", HOST_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_grad_faults_break_the_bound(shape, fault):
    N, K = shape
    _, ads = LR.make_case(N, K, [3], seed=10, scales=[0.5])
    A, B, s = ads[0]
    dW = LR.make_dw(N, K, 11)
    fA, fB = LR.fault_grads(dW, A, B, s, fault)
    rA, rB = LR.grads64(dW, A, B, s)
    bA, bB = LR.grads_bound(dW, A, B, s)
    assert (np.abs(fA - rA) > bA).any(), f"{fault} on {shape}: dA stays inside the bound"
    if fault != "dA_from_A":
        assert (np.abs(fB - rB) > bB).any(), f"{fault} on {shape}: dB stays inside the bound"


def test_nonfinite_pattern_of_the_restatement():
    """an inf / NaN in dW[n0][k0] reaches column k0 of dA and row n0 of dB and nothing else (no coefficient is zero here)"""
    N, K = 33, 7
    _, ads = LR.make_case(N, K, [3], seed=12)
    A, B, s = ads[0]
    for bad in (np.inf, np.nan):
        dW = LR.make_dw(N, K, 13)
        dW[5, 2] = bad
        with np.errstate(invalid="ignore"):
            rA, rB = LR.grads64(dW, A, B, s)
        fa, fb = np.isfinite(rA), np.isfinite(rB)
        assert not fa[:, 2].any() and fa[:, [0, 1, 3, 4, 5, 6]].all()
        assert not fb[5].any() and np.delete(fb, 5, 0).all()


# ---------------------------------------------------------------------------------------------- keys and refusals
MODS = {"down_blocks.0.attentions.0.transformer_blocks.0.attn1.to_q": (64, 64),
        "down_blocks.0.attentions.0.transformer_blocks.0.attn2.to_k": (64, 128),
        "down_blocks.0.attentions.0.transformer_blocks.0.attn1.to_out.0": (64, 64)}


def _sd(prefix="unet.", r=4, alpha=None, old=False):
    sd = {}
    for i, (m, (N, K)) in enumerate(MODS.items()):
        A, B = torch.full((r, K), 1.0 + i), torch.full((N, r), 2.0 + i)
        if old:
            m2 = m[:-2] if m.endswith(".0") else m
            head, leaf = m2.rsplit(".", 1)
            sd[f"{prefix}{head}.processor.{leaf}_lora.down.weight"], sd[f"{prefix}{head}.processor.{leaf}_lora.up.weight"] = A, B
        else:
            sd[f"{prefix}{m}.lora_A.weight"], sd[f"{prefix}{m}.lora_B.weight"] = A, B
            if alpha is not None:
                sd[f"{prefix}{m}.alpha"] = torch.tensor(float(alpha))
    return sd


@pytest.mark.parametrize("prefix", ["unet.", "base_model.model.", ""])
def test_prefixes_and_alpha_sources(prefix):
    from diffute_amd.lora import parse_lora_state_dict
    got = parse_lora_state_dict(_sd(prefix, alpha=8), MODS)
    assert list(got) == list(MODS)
    for i, (m, (A, B, alpha)) in enumerate(got.items()):
        assert alpha == 8.0 and tuple(A.shape) == (4, MODS[m][1]) and tuple(B.shape) == (MODS[m][0], 4) and float(A[0, 0]) == 1.0 + i
    assert all(al == 2.0 for _, _, al in parse_lora_state_dict(_sd(prefix), MODS, {"lora_alpha": "2.0"}).values())      # from the metadata
    assert all(al == 4.0 for _, _, al in parse_lora_state_dict(_sd(prefix), MODS).values())                              # defaulted: alpha = r
    assert all(al == 8.0 for _, _, al in parse_lora_state_dict(_sd(prefix, alpha=8), MODS, {"lora_alpha": "2.0"}).values())   # the key wins


def test_old_down_up_names():
    from diffute_amd.lora import parse_lora_state_dict
    got = parse_lora_state_dict(_sd("unet.", old=True), MODS)
    assert set(got) == set(MODS)
    for i, m in enumerate(MODS):
        A, B, alpha = got[m]
        assert float(A[0, 0]) == 1.0 + i and float(B[0, 0]) == 2.0 + i and alpha == 4.0
    plain = {k.replace(".processor.", "."): v for k, v in _sd("", old=True).items()}
    assert set(parse_lora_state_dict(plain, MODS)) == set(MODS)


def test_written_names_round_trip():
    from diffute_amd.lora import lora_file_keys, parse_lora_state_dict
    sd = {}
    for m, (N, K) in MODS.items():
        ka, kb, kal = lora_file_keys(m)
        assert (ka, kb, kal) == (f"unet.{m}.lora_A.weight", f"unet.{m}.lora_B.weight", f"unet.{m}.alpha")
        sd[ka], sd[kb], sd[kal] = torch.randn(3, K), torch.randn(N, 3), torch.tensor(6.0)
    got = parse_lora_state_dict(sd, MODS)
    for m in MODS:
        ka, kb, _ = lora_file_keys(m)
        assert got[m][0] is sd[ka] and got[m][1] is sd[kb] and got[m][2] == 6.0


def test_state_dict_refusals_name_the_key():
    from diffute_amd.lora import parse_lora_state_dict
    m = next(iter(MODS))
    sd = _sd()
    sd["unet.mid_block.resnets.0.conv1.lora_A.weight"] = torch.zeros(4, 9)
    with pytest.raises(ValueError, match="mid_block.resnets.0.conv1"):                          # unknown module (a convolution)
        parse_lora_state_dict(sd, MODS)
    sd = _sd(); sd[f"unet.{m}.lora_B.weight"] = torch.zeros(64, 5)
    with pytest.raises(ValueError, match=f"unet.{m}.lora_B.weight.*rank 5"):                    # rank mismatch
        parse_lora_state_dict(sd, MODS)
    sd = _sd(); sd[f"unet.{m}.lora_A.weight"] = torch.zeros(4, 65)
    with pytest.raises(ValueError, match=f"unet.{m}.lora_A.weight.*shape"):                     # shape mismatch
        parse_lora_state_dict(sd, MODS)
    sd = _sd(); sd[f"unet.{m}.lora_B.weight"] = torch.zeros(63, 4)
    with pytest.raises(ValueError, match=f"unet.{m}.lora_B.weight.*shape"):
        parse_lora_state_dict(sd, MODS)
    sd = _sd(); del sd[f"unet.{m}.lora_B.weight"]
    with pytest.raises(ValueError, match="not both"):
        parse_lora_state_dict(sd, MODS)
    with pytest.raises(ValueError, match="not a LoRA tensor name"):
        parse_lora_state_dict({"unet.x.weight": torch.zeros(1)}, MODS)


TINY_UNET = dict(block_out_channels=(64, 128, 256, 256), attention_head_dim=(1, 2, 4, 4), cross_attention_dim=128)


@pytest.fixture(scope="module")
def tiny():
    import diffute_amd as D
    return D.UNet2DConditionModel(**TINY_UNET)


def test_targets_of_the_model(tiny):
    from diffute_amd.lora import DEFAULT_TARGETS, LORA_TARGETS, target_keys
    shapes = {k: tuple(p.shape) for k, p in tiny.named_parameters()}
    default = target_keys(shapes, DEFAULT_TARGETS)
    assert len(default) == 16 * 8                                     # q, k, v, out of attn1 and attn2 in 16 transformer blocks
    assert all(".attentions." in k and len(shapes[k]) == 2 for k in default)
    every = target_keys(shapes, LORA_TARGETS)
    assert len(every) == 16 * 12
    assert len(target_keys(shapes, "proj_out")) == 16 and len(target_keys(shapes, ("ff.net.0.proj", "ff.net.2"))) == 32
    for bad in ("conv1", "conv_in", "time_emb_proj", "norm1", "to_out", "linear_1", "conv_shortcut"):
        with pytest.raises(ValueError, match=bad):
            target_keys(shapes, ("to_q", bad))


def test_adapter_bookkeeping_on_the_cpu(tiny):
    """what needs no arena: registration, freezing, initialisation, active set, state dict, refusals"""
    import diffute_amd as D
    u = D.UNet2DConditionModel(**TINY_UNET)
    before = {k: v.clone() for k, v in u.state_dict().items()}
    with pytest.raises(ValueError, match="conv1"):
        u.add_adapter(D.LoraConfig(r=4, target_modules=("conv1",)))
    u.add_adapter(D.LoraConfig(r=4, lora_alpha=8), adapter_name="a")
    u.add_adapter(D.LoraConfig(r=2, lora_alpha=2, target_modules=("proj_out", "ff.net.2")), adapter_name="b")
    assert u.active_adapters == ["b"]
    with pytest.raises(ValueError):
        u.add_adapter(D.LoraConfig(), adapter_name="a")
    lp = u.lora_parameters("a")
    assert len(lp) == 2 * 128 and all(p.requires_grad and p.dtype == torch.float32 for p in lp)
    assert len(u.lora_parameters()) == 2 * 128 + 2 * 32
    base = [p for k, p in u.named_parameters() if not k.startswith("lora_adapters.")]
    assert len(base) == len(before) and not any(p.requires_grad for p in base)
    ids = {id(p) for p in u.parameters()}
    assert all(id(p) in ids for p in u.lora_parameters())            # registered: .to() / .cuda() move them
    sd = u.lora_state_dict("a")
    m = "down_blocks.0.attentions.0.transformer_blocks.0.attn2.to_k"
    A, B = sd[f"unet.{m}.lora_A.weight"], sd[f"unet.{m}.lora_B.weight"]
    assert tuple(A.shape) == (4, 128) and tuple(B.shape) == (64, 4) and float(sd[f"unet.{m}.alpha"]) == 8.0 and sd[f"unet.{m}.alpha"].ndim == 0
    assert float(B.abs().max()) == 0.0 and 0 < float(A.abs().max()) <= 1 / np.sqrt(128)       # kaiming-uniform(a = sqrt 5): U(-1/sqrt K, 1/sqrt K)
    u.set_adapters(["a", "b"], [0.5, 2.0])
    assert u.active_adapters == ["a", "b"]
    u.disable_adapters()
    assert u.active_adapters == []
    with pytest.raises(ValueError, match="nope"):
        u.set_adapters("nope")
    u.set_adapters("a")
    u.delete_adapter("b")
    assert list(u._lora) == ["a"] and len(u.lora_parameters()) == 2 * 128
    assert all(torch.equal(before[k], v) for k, v in u.state_dict().items() if not k.startswith("lora_adapters."))
    # loading: a fresh model takes the state dict; wrong rank for an existing adapter and unknown modules are refused
    v = D.UNet2DConditionModel(**TINY_UNET)
    v.load_lora_weights(dict(sd), adapter_name="a")
    assert v.active_adapters == ["a"] and all(torch.equal(x, y) for x, y in zip(v.lora_parameters("a"), u.lora_parameters("a")))
    bad = {k: (t[:2] if k.endswith("lora_A.weight") else t[:, :2] if k.endswith("lora_B.weight") else t) for k, t in sd.items()}
    with pytest.raises(ValueError, match="rank 2"):
        v.load_lora_weights(bad, adapter_name="a")
