"""The T2I-Adapter library on the GPU: msda_feature_add against its statement bit for bit (fmaf emulated in float64 on operands for
which that is exact), msda_unshuffle / msda_relu / msda_avgpool2 against their numpy statements bit for bit, all between guard bands;
the adapter network against t2iadapter.forward_host; and the adapter job through the pipeline."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _extents_t2i as XT
import _guard as G
from conftest import run_calls

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16
NAN = float("nan")
STEPS = 3


def bits(t):
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------------------ msda_feature_add
def table_of(U):
    """fp32 [3][U][4]: every entry differs - (1 + index) / 64, at most 6 significant bits - so a wrong row, unit or site column
    changes the result."""
    idx = np.arange(STEPS * U * 4, dtype=np.float64).reshape(STEPS, U, 4)
    return ((1.0 + idx) / 64.0).astype(np.float32)


def statement(x, feats, scales):
    """The header's statement: acc = float(x); for u ascending with s_u != 0: acc = fmaf(s_u, float(f_u), acc); one rounding to bf16.
    fmaf is emulated in float64: the product (24 x 8 bits) is always exact there, and the sum is ASSERTED exact by the error term of
    Knuth's two-sum, so the one rounding to fp32 is fmaf's.  x (rows, n) / feats [(n,)] bf16 tensors, scales fp32 -> bf16 (rows, n)."""
    acc = x.float().numpy().astype(np.float32)
    for f, s in zip(feats, scales):
        if float(s) == 0.0:
            continue
        p = np.float64(s) * f.float().numpy().astype(np.float64)[None, :]
        a = acc.astype(np.float64)
        t = p + a
        bv = t - p
        err = (p - (t - bv)) + (a - bv)
        assert not err.any(), "the float64 sum is not exact for these operands: the emulation of fmaf would round twice"
        acc = t.astype(np.float32)
    return torch.from_numpy(acc).to(BF16)


def dyadic(rows, n, U, scales, seed):
    """Operands that land on bf16 ties in both directions: x = +-(128 + m) 2^(e - 7) (ulp 2^(e - 7)); with s_u = k_u / 64, k_u = o_u 2^t_u
    (o_u odd), unit 0's feature is 2^(e - 2 - t_0), so its term is o_0 HALF ulps - a tie - and the further units' features are
    2^(e - 1 - t_u): o_u whole ulps.  m stays where no sum leaves the binade; even and odd m give ties that round down and up."""
    rng = np.random.default_rng(seed)
    k = [int(round(float(s) * 64)) for s in scales]
    t = [(kk & -kk).bit_length() - 1 for kk in k]
    e = rng.integers(1, 4, n)
    sign = rng.choice([-1.0, 1.0], (rows, n))
    m = np.where(sign > 0, rng.integers(0, 37, (rows, n)), rng.integers(92, 128, (rows, n)))
    x = sign * (128 + m) * np.exp2(e - 7.0)[None, :]
    feats = [np.exp2(e - 2.0 - t[0])] + [np.exp2(e - 1.0 - t[u]) for u in range(1, U)]
    xt = torch.from_numpy(x.astype(np.float32)).to(BF16)
    ft = [torch.from_numpy(f.astype(np.float32)).to(BF16) for f in feats]
    assert torch.equal(xt.float(), torch.from_numpy(x.astype(np.float32))) and all(torch.equal(a.float(), torch.from_numpy(f.astype(np.float32))) for a, f in zip(ft, feats))
    return xt, ft


def real(rows, n, U, seed):
    """Seeded real operands with magnitudes in [2^-6, 2^6]: sign * 2^uniform(-6, 6), rounded to bf16."""
    gen = torch.Generator().manual_seed(seed)

    def draw(*shape):
        mag = torch.exp2(torch.rand(*shape, generator=gen) * 11.9 - 5.95)
        return (mag * (torch.randint(0, 2, shape, generator=gen) * 2 - 1)).to(BF16)

    return draw(rows, n), [draw(n) for _ in range(U)]


def launch(dev, x, feats, table, site, step=0, null_step=False):
    """One launch between guard bands sized by the header's extents; returns x afterwards (CPU) and the guard."""
    from minsdtf_amd import ops

    rows, n = x.shape
    U = len(feats)
    geo = dict(rows=rows, n=n, site=site, num_steps=table.shape[0])
    g = G.Guard(dev, XT.feature_add(feats=[1] * U, step_ptr=None if null_step else 1, **geo))
    xd = g.inp(x, "x")
    fd = [g.inp(f, f"feats.{u}") for u, f in enumerate(feats)]
    sc = g.inp(torch.from_numpy(np.ascontiguousarray(table, dtype=np.float32)), "scales")
    sp = None if null_step else g.inp(torch.tensor([step], dtype=torch.int32), "step_ptr")
    run_calls(ops.feature_add(x=xd, feats=fd, scales=sc, step_ptr=sp, **geo))
    g.check()
    for u, f in enumerate(feats):   # the inputs keep their bits
        assert torch.equal(bits(fd[u].cpu()), bits(f))
    return xd.clone().cpu()


@pytest.mark.parametrize("site", [0, 3])
@pytest.mark.parametrize("U", [1, 3])
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("n", [8, 2048, 2056, 5 * 320])
def test_feature_add_bits(gpu, n, rows, U, site):
    """No tolerance: the result is the statement's, bit for bit, on dyadic operands that land on ties in both directions and on seeded
    real operands; the table's entries all differ, and row 1 of 3 is the one read."""
    table = table_of(U)
    x, feats = dyadic(rows, n, U, table[1, :, site], seed=n + rows)
    want = statement(x, feats, table[1, :, site])
    if n >= 2048:   # every sum is a tie (an odd number of half ulps inside x's binade): none is kept, and both directions occur
        exact = x.double() + sum(float(s) * f.double()[None] for s, f in zip(table[1, :, site], feats))
        assert not bool((want.double() == exact).any())
        assert bool((want.double().abs() < exact.abs()).any()) and bool((want.double().abs() > exact.abs()).any())
    got = launch(gpu, x, feats, table, site, step=1)
    assert torch.equal(bits(got), bits(want)), f"dyadic: {int((bits(got) != bits(want)).sum())} of {got.numel()} elements differ"
    table = table * np.float32(7.0)   # (7 .. 252) / 64: all different, up to 3.94
    x, feats = real(rows, n, U, seed=3 * n + U)
    want = statement(x, feats, table[1, :, site])
    got = launch(gpu, x, feats, table, site, step=1)
    assert torch.equal(bits(got), bits(want)), f"real: {int((bits(got) != bits(want)).sum())} of {got.numel()} elements differ"
    for other_step, other_site in ((0, site), (2, site), (1, (site + 1) % 4)):   # another row or column is another result
        assert not torch.equal(bits(statement(x, feats, table[other_step, :, other_site])), bits(want))


def test_step_pointer_is_clamped_and_null_is_row_zero(gpu):
    n, rows, U, site = 2056, 2, 3, 2
    table = table_of(U) * np.float32(3.0)
    x, feats = real(rows, n, U, seed=17)
    want = [statement(x, feats, table[i, :, site]) for i in range(STEPS)]
    assert not torch.equal(bits(want[0]), bits(want[2])) and not torch.equal(bits(want[0]), bits(want[1]))
    for step, row in ((-5, 0), (0, 0), (1, 1), (2, 2), (7, 2), (1 << 30, 2)):
        assert torch.equal(bits(launch(gpu, x, feats, table, site, step=step)), bits(want[row])), (step, row)
    assert torch.equal(bits(launch(gpu, x, feats, table, site, null_step=True)), bits(want[0]))


def test_a_unit_at_scale_zero_is_not_read(gpu):
    n, rows, site = 5 * 320, 3, 1
    table = table_of(3)
    table[1, 1, site] = 0.0
    x, feats = real(rows, n, 3, seed=23)
    want = statement(x, feats, table[1, :, site])
    poisoned = [feats[0], torch.full((n,), NAN).to(BF16), feats[2]]
    got = launch(gpu, x, poisoned, table, site, step=1)
    assert bool(torch.isfinite(got.float()).all()) and torch.equal(bits(got), bits(want))
    assert torch.equal(bits(want), bits(statement(x, [feats[0], feats[2]], [table[1, 0, site], table[1, 2, site]])))
    # ... and the other rows and columns of the table may hold anything
    table2 = np.full_like(table, np.nan)
    table2[1, :, site] = table[1, :, site]
    assert torch.equal(bits(launch(gpu, x, poisoned, table2, site, step=1)), bits(want))


@pytest.mark.parametrize("U", [1, 3])
def test_an_all_zero_row_leaves_x_bit_for_bit(gpu, U):
    """x holds NaNs with payloads, infinities, denormals and garbage: with every scale of the row 0 it is neither read nor written."""
    n, rows, site = 2056, 3, 3
    table = table_of(U)
    table[2, :, site] = 0.0
    table[2, U - 1, site] = -0.0   # (a negative zero is a zero)
    gen = torch.Generator().manual_seed(5)
    x = torch.randint(-32768, 32767, (rows, n), generator=gen, dtype=torch.int16)
    x[0, :8] = torch.tensor([0x7FC1, 0x7F81, -1, -0x7F, 0x7F80, -0x80, 0x0001, -0x8000], dtype=torch.int16)   # quiet / signalling NaNs, inf, -inf, denormal, -0
    xb = x.view(BF16)
    feats = [torch.full((n,), NAN).to(BF16) for _ in range(U)]
    got = launch(gpu, xb, feats, table, site, step=2)
    assert torch.equal(bits(got), x)
    assert not torch.equal(bits(launch(gpu, xb, real(rows, n, U, 1)[1], table, site, step=1)), x)


def test_two_units_at_a_and_b_are_one_unit_at_a_plus_b(gpu):
    """Two units of the same feature at weights a and b add the terms of one unit at a + b - exactly where a f, b f and (a + b) f are
    exact in fp32 and the partial sum needs no rounding: dyadic operands."""
    n, rows = 2048, 2
    rng = np.random.default_rng(9)
    f = torch.from_numpy((rng.integers(-64, 65, n) / 8.0).astype(np.float32)).to(BF16)
    x = torch.from_numpy((rng.integers(-127, 128, (rows, n)) / 16.0).astype(np.float32)).to(BF16)
    a, b = 0.75, 0.5
    two, one = np.zeros((1, 2, 4), dtype=np.float32), np.zeros((1, 1, 4), dtype=np.float32)
    two[0, 0, 1], two[0, 1, 1], one[0, 0, 1] = a, b, a + b
    got2, got1 = launch(gpu, x, [f, f], two, 1), launch(gpu, x, [f], one, 1)
    assert torch.equal(bits(got2), bits(got1)) and torch.equal(bits(got1), bits(statement(x, [f], [a + b])))


def test_feature_add_argument_errors_launch_nothing(gpu):
    from minsdtf_amd import _lib_t2i, ops

    n = 64
    x = torch.full((2, n), 1.5, dtype=BF16, device=gpu)
    f = torch.ones(n, dtype=BF16, device=gpu)
    sc = torch.ones(1, 1, 4, dtype=torch.float32, device=gpu)
    good = dict(x=x, feats=[f], scales=sc, rows=2, n=n, site=0, num_steps=1)
    for bad in (dict(site=4), dict(n=60), dict(rows=0), dict(feats=[x]), dict(num_steps=0), dict(x=x.data_ptr() + 2), dict(scales=None)):
        call = ops.feature_add(**dict(good, **bad))
        assert call.fn(*call.args, torch.cuda.current_stream().cuda_stream) == -1, bad
        assert b"feature_add" in _lib_t2i.load().msda_last_error()
    torch.cuda.synchronize()
    assert bool((x == 1.5).all())
    run_calls(ops.feature_add(**good))
    assert bool((x == 2.5).all())


# ---------------------------------------------------------------------------------- msda_unshuffle, msda_relu, msda_avgpool2
@pytest.mark.parametrize("cin", [1, 3])
def test_unshuffle_bits(gpu, cin):
    from minsdtf_amd import ops, t2iadapter as T

    B, H, W = 2, 8, 16
    pic = torch.rand(B, H, W, cin, generator=torch.Generator().manual_seed(cin))
    y, x, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(cin), indexing="ij")
    pic[1] = torch.from_numpy((y * 64 + x * 4 + c).astype(np.float32))   # an index-valued sample (exact in bf16 up to 256; rounded beyond)
    want = torch.from_numpy(T.unshuffle_host(pic.numpy())).to(BF16)
    geo = dict(batch=B, h=H, w=W, cin=cin)
    g = G.Guard(gpu, XT.unshuffle(**geo))
    xd = g.inp(pic, "x")
    out = g.out((B, H // 8, W // 8, 64 * cin), BF16, NAN, "out")
    run_calls(ops.unshuffle(x=xd, out=out, **geo))
    g.check()
    assert torch.equal(bits(out.cpu()), bits(want)) and torch.equal(xd.cpu(), pic)
    assert float(out[1, 0, 1, (cin - 1) * 64 + 3 * 8 + 5]) == 3 * 64 + (8 + 5) * 4 + (cin - 1)   # (dy, dx) = (3, 5) of output pixel (0, 1)


@pytest.mark.parametrize("n", [8, 2056])
def test_relu_bits(gpu, n):
    from minsdtf_amd import ops

    gen = torch.Generator().manual_seed(n)
    x = torch.randint(-32768, 32767, (n,), generator=gen, dtype=torch.int16)
    x[:8] = torch.tensor([0, -0x8000, 0x3F80, -0x4080, 0x7FC1, -0x3F, 0x7F80, -0x80], dtype=torch.int16)   # +0, -0, 1, -1, NaN, -NaN (payload), inf, -inf
    xb = x.view(BF16)
    f = xb.float()
    want = torch.where(f <= 0, torch.zeros_like(x), x)      # +0 for every x <= 0, both zeros included; else x; NaN (no order) stays
    assert int(want[1]) == 0 and int(want[3]) == 0 and int(want[4]) == 0x7FC1 and int(want[5]) == -0x3F and int(want[7]) == 0
    g = G.Guard(gpu, XT.relu(n=n))
    xd = g.inp(xb, "x")
    run_calls(ops.relu(x=xd, n=n))
    g.check()
    got = bits(xd.cpu())
    assert torch.equal(got, want), f"{int((got != want).sum())} of {n} differ"
    assert bool(torch.isnan(xd.cpu().float()[torch.isnan(f)]).all())


@pytest.mark.parametrize("C", [8, 320])
@pytest.mark.parametrize("hw", [(2, 4), (6, 2)])
def test_avgpool2_bits(gpu, hw, C):
    from minsdtf_amd import ops

    B, (H, W) = 2, hw
    x = (torch.randn(B, H, W, C, generator=torch.Generator().manual_seed(H * C)) * 3).to(BF16)
    a = x.float().numpy()
    want = ((a[:, 0::2, 0::2] + a[:, 0::2, 1::2]) + (a[:, 1::2, 0::2] + a[:, 1::2, 1::2])) * np.float32(0.25)   # fp32, the pinned order
    assert want.dtype == np.float32
    want = torch.from_numpy(want).to(BF16)
    geo = dict(batch=B, h=H, w=W, c=C)
    g = G.Guard(gpu, XT.avgpool2(**geo))
    xd = g.inp(x, "x")
    out = g.out((B, H // 2, W // 2, C), BF16, NAN, "out")
    run_calls(ops.avgpool2(x=xd, out=out, **geo))
    g.check()
    assert torch.equal(bits(out.cpu()), bits(want)) and torch.equal(bits(xd.cpu()), bits(x))


def test_adapter_op_argument_errors_launch_nothing(gpu):
    from minsdtf_amd import ops

    st = torch.cuda.current_stream().cuda_stream
    pic = torch.rand(1, 16, 16, 3, device=gpu)
    out = torch.full((1, 2, 2, 192), 7.0, dtype=BF16, device=gpu)
    for bad in (dict(h=12), dict(w=4), dict(cin=5), dict(batch=0), dict(out=out.data_ptr() + 2)):
        call = ops.unshuffle(**dict(dict(x=pic, out=out, batch=1, h=16, w=16, cin=3), **bad))
        assert call.fn(*call.args, st) == -1, bad
    x = torch.full((2, 4, 4, 16), -2.0, dtype=BF16, device=gpu)
    for bad in (dict(n=12), dict(n=0), dict(x=x.data_ptr() + 2)):
        call = ops.relu(**dict(dict(x=x, n=x.numel()), **bad))
        assert call.fn(*call.args, st) == -1, bad
    pooled = torch.full((2, 2, 2, 16), 7.0, dtype=BF16, device=gpu)
    for bad in (dict(h=3), dict(w=5), dict(c=12), dict(out=x)):
        call = ops.avgpool2(**dict(dict(x=x, out=pooled, batch=2, h=4, w=4, c=16), **bad))
        assert call.fn(*call.args, st) == -1, bad
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((x == -2.0).all()) and bool((pooled == 7.0).all())


# ------------------------------------------------------------------------------------------------------- the adapter network
GOLD = os.path.join(ROOT, "tests", "golden")
PSNR_MIN = 40.0        # the project's bar for a network against float64, and for every job


@pytest.mark.parametrize("cin", [1, 3])
@pytest.mark.parametrize("hw", [(128, 128), (128, 192)])
def test_adapter_network_against_forward_host(gpu, cin, hw):
    from minsdtf_amd import t2iadapter as T
    from minsdtf_amd.models import T2IAdapter
    from oracle import sd_oracle as O

    m = T2IAdapter.synthetic(3, cin, device=gpu)
    pic = np.random.default_rng(cin + hw[1]).random((1,) + hw + (cin,)).astype(np.float32)
    got = m.predict_on_batch(pic)
    ref = T.forward_host(m.state, pic)
    assert len(m._plans[hw].plan.calls) == 31 and m.runs == 1
    ps = [float(O.psnr(g, r.astype(np.float32))) for g, r in zip(got, ref)]
    print(f"t2i adapter cin {cin} at {hw}: feature PSNR vs float64 " + ", ".join(f"{p:.1f}" for p in ps) + " dB")
    assert [g.shape for g in got] == [r.shape for r in ref] and all(np.isfinite(g).all() for g in got)
    assert min(ps) >= PSNR_MIN, ps
    again = m.predict_on_batch(pic.copy())
    assert m.runs == 1 and all(np.array_equal(a, b) for a, b in zip(again, got))


# -------------------------------------------------------------------------------------------------------------------- jobs
@pytest.fixture(scope="module")
def nets(gpu):
    """The synthetic UNet, decoder and encoder at 64 x 64 (the other sizes share the UNet's packed weights), two synthetic T2I-Adapters
    (3 and 1 input channels) and a synthetic IP-Adapter."""
    from minsdtf_amd.models import DiffusionModel, ImageDecoder, ImageEncoder, IPAdapter, T2IAdapter

    out = {}
    m = DiffusionModel(64, 64, device=gpu)
    m.load_synthetic(seed=0, bias_scale=0.05)
    out[("unet", 64)] = m
    for size in (128, 256):
        v = DiffusionModel(size, size, device=gpu)
        v.share_weights(m)
        out[("unet", size)] = v
    out["dec"] = ImageDecoder(device=gpu)
    out["dec"].load_synthetic(seed=0, bias_scale=0.05)
    out["enc"] = ImageEncoder(device=gpu)
    out["enc"].load_synthetic(seed=0, bias_scale=0.05)
    out["t2i"] = T2IAdapter.synthetic(7, 3, device=gpu)
    out["t2i1"] = T2IAdapter.synthetic(8, 1, device=gpu)
    out["ip"] = IPAdapter.synthetic(5, 4, device=gpu)
    return out


def _pipe(gpu, nets, size=64, jit=True, **kw):
    from minsdtf_amd.stable_diffusion import StableDiffusion

    sd = StableDiffusion(size, size, jit_compile=jit, device=gpu, **kw)
    sd._diffusion_model, sd._image_decoder, sd._image_encoder = nets[("unet", size)], nets["dec"], nets["enc"]
    return sd


_RNG = np.random.default_rng(79)
CTX = _RNG.standard_normal((77, 768)).astype(np.float32)
UNC = _RNG.standard_normal((77, 768)).astype(np.float32)
PIC_A = _RNG.integers(0, 256, (64, 64, 3)).astype(np.uint8)
PIC_B = _RNG.integers(0, 256, (48, 80, 3)).astype(np.uint8)   # (resized to the job's size)
PICTURE = _RNG.integers(0, 256, (64, 64, 3)).astype(np.uint8)
EMB = _RNG.standard_normal(1024)
KW = dict(batch_size=1, num_steps=3, unconditional_guidance_scale=7.5, guidance_rescale=0.7, seed=5, return_latent=True)


def _t2i(nets, pic=PIC_A, **kw):
    return dict(image=pic, model=nets["t2i"], **kw)


def _job(sd, **kw):
    sd.unconditional_context = UNC
    return sd.generate_image(CTX, **{**KW, **kw})


@pytest.mark.parametrize("size", [128, 256])
def test_vs_oracle_fixture(gpu, nets, size):
    """The fixture jobs against the fp32 oracle's composition (tools/make_t2i_adapter_fixtures.py: sd_oracle.attentions / res_block
    wrapped at the four sites): final latent PSNR >= 40 dB, where the plain job stays under 35 dB (`plain_psnr` in the file)."""
    from minsdtf_amd.models import T2IAdapter
    from oracle import sd_oracle as O

    g = np.load(os.path.join(GOLD, f"t2i_adapter_{size}.npz"))
    assert (int(g["weight_seed"]), float(g["bias_scale"])) == (0, 0.05) and float(g["plain_psnr"]) < 35.0
    sd = _pipe(gpu, nets, size)
    rng = np.random.default_rng(int(g["context_seed"]))
    ctx = rng.standard_normal((1, 77, 768)).astype(np.float32)[0]
    sd.unconditional_context = rng.standard_normal((1, 77, 768)).astype(np.float32)[0]
    units = []
    for n in range(int(g["units"])):
        seed, cin = int(g["adapter_seeds"][n]), int(g["in_channels"][n])
        model = {(7, 3): nets["t2i"], (8, 1): nets["t2i1"]}.get((seed, cin)) or T2IAdapter.synthetic(seed, cin, device=gpu)
        pic = np.random.default_rng([int(g["picture_seed"]), n]).integers(0, 256, (size, size, 3) if cin == 3 else (size, size)).astype(np.uint8)
        units.append(dict(image=pic, model=model, weight=[float(v) for v in g["site_weights"][n]], start=float(g["start"][n]), end=float(g["end"][n])))
    kw = dict(batch_size=1, num_steps=int(g["steps"]), unconditional_guidance_scale=float(g["guidance"]), seed=int(g["noise_seed"]),
              return_latent=True)
    got = sd.generate_image(ctx, t2i_adapter=units, **kw)
    p = O.psnr(got, g["latent"])
    plain = O.psnr(sd.generate_image(ctx, **kw), g["latent"])
    print(f"t2i_adapter fixture {size}x{size} ({len(units)} unit(s)): final latent PSNR {p:.1f} dB; the plain job {plain:.1f} dB on the "
          f"device, {float(g['plain_psnr']):.1f} dB in the oracle")
    assert p >= PSNR_MIN
    assert plain < PSNR_MIN   # (by construction)


@pytest.mark.parametrize("sampler, steps", [(None, 3), ("dpmpp_2m_karras", 8)])
def test_device_loop_vs_host_loop(gpu, nets, sampler, steps):
    """The device loop against host_loop=True (DiffusionModel.predict_t2i per half) at 40 dB."""
    from oracle import sd_oracle as O

    sd = _pipe(gpu, nets)
    kw = dict(t2i_adapter=_t2i(nets, weight=[1.0, 0.8, 0.6, 0.4], end=0.75), sampler=sampler, num_steps=steps)
    dev = _job(sd, **kw)
    host = _job(sd, host_loop=True, **kw)
    plain = _job(sd, sampler=sampler, num_steps=steps)
    p, q = O.psnr(dev, host), O.psnr(plain, host)
    print(f"t2i_adapter, sampler {sampler}, {steps} steps: device loop vs host loop {p:.1f} dB (bar {PSNR_MIN:.0f}); the plain job against it {q:.1f} dB")
    assert p >= PSNR_MIN and q < p


@pytest.mark.parametrize("form", ["euler_a", "tcd", "img2img", "inpaint", "ip_adapter", "dynamic_threshold", "two_units", "eager"])
def test_forms_run_and_repeat(gpu, nets, form):
    """A stochastic sampler, a TCD pipeline, image_to_image, inpainting, with an image prompt, with dynamic thresholding, two adapters:
    the job runs, repeats its bits, differs from the job without the adapter and records four adds per pass."""
    sd = _pipe(gpu, nets, jit=form != "eager", **(dict(active_tcd=True) if form == "tcd" else {}))
    kw = {"euler_a": dict(sampler="euler_a"), "img2img": dict(reference_image=PICTURE, reference_image_strength=0.7),
          "ip_adapter": dict(ip_adapter=dict(embeds=EMB, model=nets["ip"])), "dynamic_threshold": dict(dynamic_threshold=dict(mimic_scale=5.0)),
          "inpaint": dict(reference_image=PICTURE, reference_image_strength=0.7, inpaint_mask=np.pad(np.full((32, 32), 255.0), 16))}.get(form, {})
    spec = [_t2i(nets), dict(image=PIC_B[..., 0], model=nets["t2i1"], weight=0.5)] if form == "two_units" else _t2i(nets)

    def run(**more):
        np.random.seed(3)   # (the TCD sampler's draws come from numpy's global stream)
        return _job(sd, **kw, **more)

    a = run(t2i_adapter=spec)
    eng = next(iter(sd._engines.values()))
    assert eng.t2i_units == (2 if form == "two_units" else 1) and len(eng.passes) == 1
    assert [c.name for c in eng.calls if c.name.endswith(".t2i")] == [s + ".t2i" for s in ("down_blocks.0.attentions.1", "down_blocks.1.attentions.1",
                                                                                            "down_blocks.2.attentions.1", "down_blocks.3.resnets.1")]
    assert np.isfinite(a).all()
    np.testing.assert_array_equal(run(t2i_adapter=spec), a)
    assert not np.array_equal(run(), a)


def test_all_zero_table_and_weight_zero_are_the_plain_job(gpu, nets):
    sd = _pipe(gpu, nets)
    plain = _job(sd)
    for spec in (dict(weight=0.0), dict(start=1.0), dict(weight=[0.0] * 4)):
        np.testing.assert_array_equal(_job(sd, t2i_adapter=_t2i(nets, **spec)), plain)
        assert len(sd._engines) == 1 and next(iter(sd._engines.values())).t2i_units == 0
    # on the adapter's engine too: a table whose EXECUTED rows are all 0 leaves every activation its bits (the launch neither reads
    # nor writes x), so the latent is the plain job's bit for bit.  strength 0.5 over 4 steps executes rows 2 and 3; end = 0.5 keeps 0, 1
    i2i = dict(num_steps=4, reference_image=PICTURE, reference_image_strength=0.5)
    late = _job(sd, t2i_adapter=_t2i(nets, end=0.5), **i2i)
    assert any(e.t2i_units == 1 for e in sd._engines.values())
    np.testing.assert_array_equal(late, _job(sd, **i2i))
    on = _job(sd, t2i_adapter=_t2i(nets, start=0.5), **i2i)
    assert not np.array_equal(on, late)
    np.testing.assert_array_equal(_job(sd, t2i_adapter=_t2i(nets), **i2i), on)


def test_sample_bits_do_not_depend_on_the_batch(gpu, nets):
    sd = _pipe(gpu, nets)
    spec = _t2i(nets, weight=0.8)
    noise = np.random.default_rng(2).standard_normal((3, 8, 8, 4)).astype(np.float32)
    kw = dict(t2i_adapter=spec, seed=None)
    full = _job(sd, batch_size=3, diffusion_noise=noise, **kw)
    np.testing.assert_array_equal(_job(sd, batch_size=3, diffusion_noise=noise, **kw), full)
    for b in (0, 2):
        np.testing.assert_array_equal(_job(sd, batch_size=1, diffusion_noise=noise[b], **kw)[0], full[b])


def test_other_pictures_weights_and_schedules_build_no_engine(gpu, nets, monkeypatch):
    import minsdtf_amd.stable_diffusion as sdm

    built = []
    init = sdm.DenoiseEngine.__init__

    def counting(self, *a, **k):
        built.append(k.get("t2i_units"))
        return init(self, *a, **k)

    monkeypatch.setattr(sdm.DenoiseEngine, "__init__", counting)
    from minsdtf_amd.models import T2IAdapter

    sd = _pipe(gpu, nets)
    own = T2IAdapter.synthetic(7, 3, device=gpu)              # (its own: the module's adapter remembers another test's last picture)
    a = dict(image=PIC_A, model=own, weight=0.8, end=0.75)
    b = dict(image=PIC_B, model=own, weight=[1.3, 1.0, 0.5, 0.2], start=0.3)
    first = _job(sd, t2i_adapter=a)
    second = _job(sd, t2i_adapter=b)
    assert built == [1] and len(sd._engines) == 1 and own.runs == 2
    np.testing.assert_array_equal(_job(sd, t2i_adapter=dict(b)), second)
    assert own.runs == 2                                      # the last picture's features are kept: the adapter did not run
    np.testing.assert_array_equal(_job(sd, t2i_adapter=a), first)
    assert built == [1] and not np.array_equal(first, second)
    np.testing.assert_array_equal(_job(_pipe(gpu, nets), t2i_adapter=b), second)


def test_sharded_job_equals_unsharded(gpu):
    """A one-rank process group with forced collectives (as tests/test_ip_adapter_gpu.py): the sharded job == the unsharded one."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_t2i_adapter_world1_child.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=570)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert any(line.startswith("OK ") for line in p.stdout.splitlines()), p.stdout[-2000:]
    print(p.stdout.strip().splitlines()[-1])
