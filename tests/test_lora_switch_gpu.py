"""LoRA switch at run time on the device (minsdtf_amd/lora.py, csrc/lora.hip): the merge kernel against a float64 restatement in
every destination form, the switched packed image against the load-time merge, captured graphs that stay valid across a switch,
the end-to-end result against the oracle, the text encoder, failures that leave no trace and repeat switches that read no file."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RANK = 4


def _lora_sd(seed, te=True, rank=RANK, std=0.05):
    """kohya-named factors for all 278 UNet layers (and the 72 text-encoder layers)."""
    from minsdtf_amd import weights as Wt

    rng = np.random.default_rng(seed)
    spec_of = {s.alt_key: s for s in Wt.table("civitai_model") if s.alt_key}
    items = [(n, spec_of[k].torch_shape) for n, k in Wt._lora_unet_name_map().items()]
    if te:
        for s in Wt.table("text_encoder"):
            if s.kind == "dense_w" and s.name.endswith(Wt._LORA_TE_SUFFIXES):
                items.append(("lora_te_" + s.name.replace(".", "_"), s.torch_shape))
    sd = {}
    for n, ts in items:
        up, down = ((ts[0], rank), (rank, ts[1])) if len(ts) == 2 else ((ts[0], rank, 1, 1), (rank, ts[1], ts[2], ts[3]))
        sd[n + ".lora_up.weight"] = torch.from_numpy((rng.standard_normal(up) * std).astype(np.float32))
        sd[n + ".lora_down.weight"] = torch.from_numpy((rng.standard_normal(down) * std).astype(np.float32))
        sd[n + ".alpha"] = torch.tensor(float(rank))
    return sd


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from safetensors.torch import save_file

    from minsdtf_amd import weights as Wt

    d = tmp_path_factory.mktemp("lora_switch")
    ck = str(d / "sd15.safetensors")
    Wt.write_synthetic_checkpoint(ck, kinds=("civitai_model", "decoder", "text_encoder", "text_clip_embedding"), seed=0,
                                  bias_scale=0.05)
    l1, l2 = str(d / "a.safetensors"), str(d / "b.safetensors")
    save_file(_lora_sd(1), l1)
    save_file(_lora_sd(2), l2)
    return ck, l1, l2


def _inputs():
    rng = np.random.default_rng(31)
    return (rng.standard_normal((77, 768)).astype(np.float32), rng.standard_normal((77, 768)).astype(np.float32),
            rng.standard_normal((8, 8, 4)).astype(np.float32))


def _run(sd, ctx, unc, noise, **kw):
    sd.unconditional_context = unc
    return sd.generate_image(ctx, batch_size=1, num_steps=2, unconditional_guidance_scale=7.5, diffusion_noise=noise,
                             guidance_rescale=0.7, return_latent=True, **kw)


def _bf16_ulps(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """|a - b| in bf16 units in the last place (ordered-integer distance)."""
    def key(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (key(a) - key(b)).abs()


def _rows(W, k):
    t = W[k]
    if k in W.chunk_major_keys:
        t = t.permute(1, 0, 2).reshape(t.shape[1], -1)
    return t


def _compare_packed(got, ref, label):
    """bf16: every element within 1 ulp (or 2^-20 of the matrix's largest value), >= 99.9 % equal; .lncs = fp64 row sum of got's own .lnw (<= 1 fp32 ulp); other fp32
    within 1e-5 max(1, |ref|); every fragment-major copy = packing.fragment_major of its stored matrix, bit for bit."""
    from minsdtf_amd import packing

    assert set(got) == set(ref)
    total = equal = 0
    for k in ref:
        a, b = got[k], ref[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        if a.dtype == torch.bfloat16:
            u = _bf16_ulps(a, b)
            # where W + delta (or the 4C-term ffproj product) nearly cancels, the two routes' fp32 roundings of their different
            # summation orders move the tiny result by more than one of ITS bf16 ulps: such elements are held to 2^-20 of the
            # matrix's largest value instead (LoRA switch: numerics)
            small = (a.float() - b.float()).abs() <= b.float().abs().max() * 2.0 ** -20
            u = torch.where(small, torch.zeros_like(u), u)
            assert int(u.max()) <= 1, (label, k, int(u.max()))
            total += u.numel()
            equal += int((u == 0).sum())
        elif k.endswith(".lncs"):
            own = _rows(got, k[: -len(".lncs")] + ".lnw").double().sum(dim=1).float()
            d = (a.view(torch.int32) - own.view(torch.int32)).abs()
            assert int(d.max()) <= 1, (label, k)
        else:
            tol = 1e-5 * torch.clamp(b.abs(), min=1.0)
            assert bool(((a - b).abs() <= tol).all()), (label, k, float((a - b).abs().max()))
    assert equal >= 0.999 * total, (label, equal / total)
    print(f"{label}: {equal / total * 100:.4f} % of {total} bf16 elements equal, the rest within 1 ulp")
    for k, f in got._fragment.items():
        assert torch.equal(f, packing.fragment_major(_rows(got, k))), (label, k)


# ---------------------------------------------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("rank", [1, 7, 32, 128])
def test_merge_kernel_matches_float64(gpu, rank):
    from minsdtf_amd import ops, packing

    dev = gpu
    g = torch.Generator().manual_seed(rank)
    rnd = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    N, K = 48, 128
    master, U, D = rnd(N, K), rnd(N, rank) * 0.1, rnd(rank, K) * 0.1
    rs, cs = rnd(N).abs() + 0.5, rnd(K).abs() + 0.5
    ref = ((master.double() + U.double() @ D.double()) * rs.double()[:, None]) * cs.double()[None, :]
    dm, dU, dD, drs, dcs = (t.contiguous().to(dev) for t in (master, U, D, rs, cs))
    perm = torch.randperm(N, generator=g).to(torch.int32)
    dperm = perm.to(dev)   # (the descriptors hold raw addresses: every operand stays alive until the launch has run)
    Nr, Kr, ld = 37, 100, 104       # the rows form: N, K and ld not multiples of 64 (down is [rank][k]: its own copy)
    dDr = D[:, :Kr].contiguous().to(dev)
    jobs, outs = [], {}
    outs["rows"] = torch.zeros(Nr + 3, ld, dtype=torch.bfloat16, device=dev)
    jobs.append(ops.lora_job(master=dm, master_ld=K, up=dU, down=dDr, rank=rank, rowscale=drs, colscale=dcs, out=outs["rows"],
                             n=Nr, k=Kr, out_rows=Nr + 3, out_cols=Kr + 2, ld=ld, row_off=3, col_off=2))
    outs["chunk"] = torch.zeros(K // 64, N, 64, dtype=torch.bfloat16, device=dev)
    outs["frag"] = torch.zeros(N * K, dtype=torch.bfloat16, device=dev)
    outs["colsum"] = torch.zeros(N, dtype=torch.float32, device=dev)
    jobs.append(ops.lora_job(master=dm, up=dU, down=dD, rank=rank, rowscale=drs, colscale=dcs, out=outs["chunk"], n=N, k=K,
                             out_rows=N, out_cols=K, layout=ops.LORA_LAYOUT_CHUNK, out_frag=outs["frag"], colsum=outs["colsum"]))
    outs["map"] = torch.zeros(N, K, dtype=torch.bfloat16, device=dev)
    jobs.append(ops.lora_job(master=dm, up=dU, down=dD, rank=rank, out=outs["map"], n=N, k=K, out_rows=N, out_cols=K,
                             rowmap=dperm))
    outs["f32"] = torch.zeros(N, K, dtype=torch.float32, device=dev)
    jobs.append(ops.lora_job(master=dm, up=dU, down=dD, rank=rank, colscale=dcs, out=outs["f32"], n=N, k=K, out_rows=N, out_cols=K,
                             out_dtype=ops.OUT_F32))
    outs["f32t"] = torch.zeros(K, N, dtype=torch.float32, device=dev)
    jobs.append(ops.lora_job(master=dm, up=dU, down=dD, rank=rank, out=outs["f32t"], n=N, k=K, out_rows=N, out_cols=K,
                             out_dtype=ops.OUT_F32, layout=ops.LORA_LAYOUT_T))
    call = ops.lora_merge(jobs, dev)
    call(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    o = {k: v.cpu() for k, v in outs.items()}

    def near(got_bf16, want64):
        u = _bf16_ulps(got_bf16, want64.float().to(torch.bfloat16))
        assert int(u.max()) <= 1

    near(o["rows"][3:3 + Nr, 2:2 + Kr], ref[:Nr, :Kr])
    assert not o["rows"][:3].any() and not o["rows"][:, :2].any() and not o["rows"][:, 2 + Kr:].any()
    rows = o["chunk"].permute(1, 0, 2).reshape(N, K)
    near(rows, ref)
    assert torch.equal(o["frag"].view(-1), packing.fragment_major(rows).reshape(-1))
    own = rows.double().sum(dim=1).float()
    assert int((o["colsum"].view(torch.int32) - own.view(torch.int32)).abs().max()) <= 1
    plain = master.double() + U.double() @ D.double()
    near(o["map"][perm.long()], plain)
    np.testing.assert_allclose(o["f32"].double().numpy(), (plain * cs.double()[None, :]).numpy(), rtol=2e-6, atol=2e-6)
    np.testing.assert_allclose(o["f32t"].t().double().numpy(), plain.numpy(), rtol=2e-6, atol=2e-6)
    # determinism: the same launch again gives the same bits
    call(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert all(torch.equal(outs[k].cpu(), o[k]) for k in o)


# ------------------------------------------------------------------------------------------ 2. parity with the load-time merge
def _unet_with_deltas(ck, dev, deltas):
    from minsdtf_amd.models import DiffusionModel

    return DiffusionModel(64, 64, ckpt_path=ck, lora_dict=deltas, device=dev)


def test_packed_parity_with_load_time_merge(gpu, files):
    from minsdtf_amd import weights as Wt
    from minsdtf_amd.stable_diffusion import StableDiffusion

    ck, l1, l2 = files
    sw = StableDiffusion(64, 64, unet_ckpt=ck, text_encoder_ckpt=ck, vae_ckpt=ck, lora_path=l1, lora_switch=True, device=gpu)
    W = sw.diffusion_model._W
    for k, t in list(W.items()):   # every eligible matrix gets its fragment-major copy, so the switch must keep them all
        if t.dtype == torch.bfloat16 and t.dim() in (2, 3) and k.endswith((".w", ".lnw")):
            r = _rows(W, k)
            if r.shape[0] % 16 == 0 and r.shape[1] % 64 == 0:
                W.fragment_major(k)
    sw.set_loras([(l1, 1.0)])
    assert sw.active_loras == ((l1, 1.0),)
    ld = StableDiffusion(64, 64, unet_ckpt=ck, text_encoder_ckpt=ck, vae_ckpt=ck, lora_path=l1, device=gpu)
    _compare_packed(W, ld.diffusion_model._W, "one LoRA, scale 1")
    _compare_packed(sw.text_encoder._W, ld.text_encoder._W, "text encoder, one LoRA")
    del ld

    sw.set_loras([(l1, 0.7), (l2, -0.4)])
    _t1, d1 = Wt.load_weights_from_lora(l1)
    _t2, d2 = Wt.load_weights_from_lora(l2)
    ref = _unet_with_deltas(ck, gpu, {k: 0.7 * d1[k] - 0.4 * d2[k] for k in d1})
    _compare_packed(W, ref._W, "two LoRAs (0.7, -0.4)")


# -------------------------------------------------------------------------------------------- 3. captured graphs stay valid
def test_switch_keeps_the_captured_loop(gpu, files):
    from minsdtf_amd.stable_diffusion import StableDiffusion

    ck, l1, _l2 = files
    ctx, unc, noise = _inputs()
    sd = StableDiffusion(64, 64, jit_compile=True, unet_ckpt=ck, vae_ckpt=ck, lora_switch=True, device=gpu)
    a = _run(sd, ctx, unc, noise)
    W = sd.diffusion_model._W
    snap = {k: t.clone() for k, t in W.items()}
    frags = {k: t.clone() for k, t in W._fragment.items()}
    (eng,) = sd._engines.values()
    graph = eng._loop_graph
    wver = sd.diffusion_model.weights_version
    sd.set_loras([(l1, 1.0)])
    b = _run(sd, ctx, unc, noise)
    (eng_b,) = sd._engines.values()
    assert eng_b is eng and eng._loop_graph is graph and sd.diffusion_model.weights_version == wver
    assert sd.diffusion_model.lora_version == 1
    assert not np.array_equal(a, b)
    eager = StableDiffusion(64, 64, jit_compile=False, unet_ckpt=ck, vae_ckpt=ck, lora_switch=True, device=gpu)
    eager.set_loras([(l1, 1.0)])
    np.testing.assert_array_equal(b, _run(eager, ctx, unc, noise))
    del eager
    sd.set_loras([])
    c = _run(sd, ctx, unc, noise)
    assert sd.active_loras == ()
    np.testing.assert_array_equal(c, a)
    for k, t in snap.items():
        assert torch.equal(W[k], t), k
    for k, t in frags.items():
        assert torch.equal(W._fragment[k], t), k


# ---------------------------------------------------------------------------------------------------- 4. end to end vs oracle
class _Collector:
    def __init__(self, specs):
        from minsdtf_amd.models import WeightVar

        self.name = "collector"
        self.weights = [WeightVar(s.name, s.shape) for s in specs]
        self.arrays = None

    def set_weights(self, arrays):
        self.arrays = list(arrays)


def test_switched_pipeline_vs_oracle(gpu, files, tmp_path):
    from safetensors.torch import save_file

    from minsdtf_amd import weights as Wt
    from minsdtf_amd.stable_diffusion import StableDiffusion
    from oracle import sd_oracle as O

    ck, _l1, _l2 = files
    lp = str(tmp_path / "unet_lora.safetensors")
    save_file(_lora_sd(7, te=False, std=0.03), lp)
    ctx, unc, noise = _inputs()
    sw = StableDiffusion(64, 64, jit_compile=True, unet_ckpt=ck, vae_ckpt=ck, lora_switch=True, device=gpu)
    plain = _run(sw, ctx, unc, noise)
    sw.set_loras([(lp, 1.0)])
    got = _run(sw, ctx, unc, noise)
    loaded = _run(StableDiffusion(64, 64, jit_compile=True, unet_ckpt=ck, vae_ckpt=ck, lora_path=lp, device=gpu), ctx, unc, noise)
    specs = Wt.table("civitai_model")
    col = _Collector(specs)
    _te, deltas = Wt.load_weights_from_lora(lp)
    Wt.load_weights_from_file(col, ck, "civitai_model", lora_dict=deltas, specs=specs)
    Wn = O.named_weights(specs, col.arrays)
    ref = O.denoise_loop(lambda l, t, c, ctl: O.unet_forward(Wn, l, t, c), ctx[None], unc[None], noise[None], num_steps=2,
                         guidance=7.5, guidance_rescale=0.7)
    p, p_plain, p_load = O.psnr(got, ref), O.psnr(plain, ref), O.psnr(got, loaded)
    print(f"LoRA switch: final-latent PSNR {p:.1f} dB vs the oracle on merged weights (without the LoRA: {p_plain:.1f} dB); "
          f"{p_load:.1f} dB vs the load-time merge")
    # (the switched and the load-time weights are two bf16 roundings of the same fp32 values that differ in ~0.1 % of the elements
    # by one ulp: after two guided steps the two pipelines are as far apart as either is from the fp32 oracle, ~46 dB)
    assert p >= 40.0 and p_plain < p - 6.0 and p_load >= 40.0


# ------------------------------------------------------------------------------------------------------------- 5. text encoder
def test_text_encoder_switch_and_unconditional_context(gpu, files):
    from minsdtf_amd.models import TextEncoder
    from minsdtf_amd import weights as Wt
    from minsdtf_amd.stable_diffusion import StableDiffusion

    ck, l1, _l2 = files
    sd = StableDiffusion(64, 64, unet_ckpt=ck, text_encoder_ckpt=ck, vae_ckpt=ck, lora_switch=True, device=gpu)
    u0 = sd._get_unconditional_context().copy()
    ids = np.asarray([[49406, 320, 1125, 539] + [49407] * 73], dtype=np.int32)
    e0 = sd.encode_tokens(ids)
    sd.set_loras([(l1, 1.0)])
    assert sd.unconditional_context is None           # computed by the pipeline: recomputed after a text-encoder switch
    u1 = sd._get_unconditional_context()
    assert not np.array_equal(u0, u1)
    e1 = sd.encode_tokens(ids)
    te_d, _u = Wt.load_weights_from_lora(l1)
    ref = TextEncoder(77, clip_skip=-1, ckpt_path=ck, lora_dict=te_d, device=gpu)
    _compare_packed(sd.text_encoder._W, ref._W, "text encoder after the switch")
    r1 = sd.text_clip_embedding.predict_on_batch([ids, sd._get_pos_ids()])
    want = ref.predict_on_batch(r1).reshape(-1, 768)
    assert not np.array_equal(e0, e1)
    np.testing.assert_allclose(e1, want, rtol=0, atol=0.05 * np.abs(want).max())
    sd.unconditional_context = unc = np.zeros((77, 768), np.float32)   # set by the caller: kept
    sd.set_loras([])
    assert sd.unconditional_context is unc


# ------------------------------------------------------------------------------------------------- 6. failure leaves no trace
def test_failed_switch_leaves_weights_untouched(gpu, files, tmp_path):
    from safetensors.torch import save_file

    from minsdtf_amd.stable_diffusion import StableDiffusion

    ck, l1, _l2 = files
    sd = StableDiffusion(64, 64, unet_ckpt=ck, vae_ckpt=ck, lora_switch=True, device=gpu)
    sd.set_loras([(l1, 0.5)])
    W = sd.diffusion_model._W
    snap = {k: t.clone() for k, t in W.items()}
    bad = _lora_sd(3, te=False)
    n = "lora_unet_mid_block_attentions_0_proj_in"
    bad[n + ".lora_down.weight"] = bad[n + ".lora_down.weight"][:, :640].contiguous()   # 640 inputs for a 1280-channel layer
    bp = str(tmp_path / "bad.safetensors")
    save_file(bad, bp)
    with pytest.raises(ValueError, match="proj_in"):
        sd.set_loras([(bp, 1.0)])
    with pytest.raises(FileNotFoundError):
        sd.set_loras([(str(tmp_path / "missing.safetensors"), 1.0)])
    for k, t in snap.items():
        assert torch.equal(W[k], t), k
    assert sd.active_loras == ((l1, 0.5),)
    plain = StableDiffusion(64, 64, unet_ckpt=ck, vae_ckpt=ck, device=gpu)
    with pytest.raises(RuntimeError, match="lora_switch"):
        plain.set_loras([(l1, 1.0)])


# ------------------------------------------------------------------------------------------- 7. a repeat switch reads no file
def test_repeat_switch_reads_no_file(gpu, files, monkeypatch):
    from minsdtf_amd import weights as Wt
    from minsdtf_amd.stable_diffusion import StableDiffusion

    ck, l1, l2 = files
    sd = StableDiffusion(64, 64, unet_ckpt=ck, vae_ckpt=ck, lora_switch=True, device=gpu)
    sd.set_loras([(l1, 1.0)])
    first = {k: t.clone() for k, t in sd.diffusion_model._W.items()}
    sd.set_loras([(l2, 1.0)])

    def no_io(*a, **k):
        raise AssertionError("a repeat switch read a file")

    monkeypatch.setattr(Wt, "read_state_dict", no_io)
    sd.set_loras([(l1, 1.0)])
    for k, t in first.items():
        assert torch.equal(sd.diffusion_model._W[k], t), k
