"""ControlNet units on the device: msdc_control_combine through the C ABI, between guard bands, against float64; what it reads and
what it leaves alone; then jobs on the seeded synthetic nets - the all-ones table against the plain ControlNet job bit for bit in
every form an engine takes, weight 0 against the job without a ControlNet, the row index of an img2img job, engine reuse, the
host loop, the sharded job and the oracle fixtures (tests/golden/control_units_*.npz, tools/make_control_units_fixtures.py).

The kernel bound is derived, not measured.  With A = |skip| + sum_n |s_n r_n| and the exact result e: the fp32 value in front of
the one bf16 rounding is off by at most N single-rounded fmaf errors, each at most 2^-24 of a partial sum that A bounds; the
rounding to bf16 (8 significant bits, round to nearest even) adds at most half an ulp, 2^-8 of the value, and carries the fp32 error
through, which the (N + 1)-th 2^-24 A covers:

    |out - e| <= 2^-8 |e| + (N + 1) 2^-24 A."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _extents_control as XC
import _guard as G

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
PSNR_MIN = 40.0   # the project's bar for every job, and what tests/test_configs_gpu.py holds the ControlNet job's two loops to

LEVEL_OF_TAP = (0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 3)
LATENTS = [(8, 8), (16, 24)]   # 8 x 8: the taps go down to 1 x 1 x 1280 (less than one chunk: the tail predicate); 16 x 24: up to 60 chunks a row


def counts_of(h, w):
    from minsdtf_amd import engine
    from minsdtf_amd import weights as wtab

    levels = engine.unet_levels(h, w)
    return [levels[lv][0] * levels[lv][1] * ch for lv, ch in zip(LEVEL_OF_TAP, tuple(wtab.UNET_SKIP_CH) + (1280,))]


def run_calls(calls):
    if not isinstance(calls, (list, tuple)):
        calls = [calls]
    st = torch.cuda.current_stream().cuda_stream
    for c in calls:
        c(st)
    torch.cuda.synchronize()


_DATA = {}


def data(latent, rows):
    """13 bf16 skips and 3 x 13 fp32 residuals of `rows` rows, and a 3-step table for 3 units, made once and never changed."""
    key = (latent, rows)
    if key not in _DATA:
        rng = np.random.default_rng(1009 * latent[0] + 17 * latent[1] + rows)
        counts = counts_of(*latent)
        skips = [torch.from_numpy(rng.standard_normal((rows, n)).astype(np.float32)).to(torch.bfloat16) for n in counts]
        resid = [[torch.from_numpy((rng.standard_normal((rows, n)) * 0.5).astype(np.float32)) for n in counts] for _ in range(3)]
        table = rng.uniform(0.05, 2.0, (3, 3, 13, 2)).astype(np.float32)
        table.setflags(write=False)
        _DATA[key] = (counts, skips, resid, table)
    return _DATA[key]


def launch(gpu, counts, skips, resid, table, rows_u, step=1, with_step_ptr=True, num_steps=None):
    """One guarded launch over copies of the operands.  Returns (the 13 skips after, as bf16 host tensors; the step counter after)."""
    from minsdtf_amd import ops

    rows, units = skips[0].shape[0], len(resid)
    num_steps = table.shape[0] if num_steps is None else num_steps
    assert table.shape == (num_steps, units, 13, 2)
    gd = G.Guard(gpu, XC.control_combine(rows=rows, counts=counts, units=units, num_steps=num_steps, step_ptr=True if with_step_ptr else None))
    sk = [gd.inp(s, f"skips.{k}") for k, s in enumerate(skips)]
    rs = [[gd.inp(r, f"resid.{n}.{k}") for k, r in enumerate(unit)] for n, unit in enumerate(resid)]
    tb = gd.inp(torch.from_numpy(np.array(table, dtype=np.float32)), "scales")
    sp = gd.inp(torch.tensor([step], dtype=torch.int32), "step_ptr") if with_step_ptr else None
    run_calls(ops.control_combine(skips=sk, resid=rs, counts=counts, scales=tb, step_ptr=sp, rows=rows, rows_u=rows_u, num_steps=num_steps))
    gd.check()   # a NaN band behind every skip (and every other operand) still carries its bits
    for n, unit in enumerate(resid):   # the residuals are only read
        for k, r in enumerate(unit):
            assert torch.equal(rs[n][k].cpu().view(torch.int32), r.view(torch.int32)), f"resid {n}.{k} was written"
    assert torch.equal(tb.cpu(), torch.from_numpy(np.array(table, dtype=np.float32)))
    return [s.cpu() for s in sk], None if sp is None else int(sp.cpu()[0])


def exact(skips, resid, row_scales, rows_u):
    """(e, A) per tap in float64: row_scales fp32 [N][13][2]."""
    out = []
    for k, s in enumerate(skips):
        rows = s.shape[0]
        e = s.to(torch.float64).numpy().copy()
        A = np.abs(e)
        for n, unit in enumerate(resid):
            col = np.where(np.arange(rows) < rows_u, row_scales[n, k, 0], row_scales[n, k, 1]).astype(np.float64)[:, None]
            term = col * unit[k].to(torch.float64).numpy()
            e = e + term
            A = A + np.abs(term)
        out.append((e, A))
    return out


@pytest.mark.parametrize("rows_u", ["none", "one", "all"])
@pytest.mark.parametrize("units", [1, 2, 3])
@pytest.mark.parametrize("rows", [2, 3])
@pytest.mark.parametrize("latent", LATENTS, ids=lambda s: "x".join(str(v) for v in s))
def test_kernel_against_float64(gpu, latent, rows, units, rows_u):
    counts, skips, resid, table = data(latent, rows)
    ru = {"none": 0, "one": 1, "all": rows}[rows_u]
    tab = np.full((3, units, 13, 2), 977.0, dtype=np.float32)   # (a row the launch must not read would show)
    tab[1] = table[1, :units]
    got, after = launch(gpu, counts, skips, resid[:units], tab, ru, step=1)
    assert after == 1
    worst = 0.0
    for k, ((e, A), g) in enumerate(zip(exact(skips, resid[:units], tab[1], ru), got)):
        g = g.to(torch.float64).numpy()
        assert np.all(np.isfinite(g))
        bound = 2.0 ** -8 * np.abs(e) + (units + 1) * 2.0 ** -24 * A
        share = np.abs(g - e) / bound
        worst = max(worst, float(share.max()))
        assert (share <= 1.0).all(), f"tap {k}: {float(share.max()):.3f} of the bound"
    print(f"control_combine {latent} rows {rows} units {units} rows_u {ru}: largest share of the bound used {worst:.3f}")


def test_step_counter_is_read_and_clamped(gpu):
    counts, skips, resid, table = data((8, 8), 2)
    at = lambda **kw: launch(gpu, counts, skips, resid[:2], table[:, :2], 1, **kw)
    rows = {}
    for i in range(3):
        one = np.repeat(table[i:i + 1, :2], 3, axis=0)
        rows[i], _ = launch(gpu, counts, skips, resid[:2], one, 1, step=0)
    same = lambda a, b: all(torch.equal(x.view(torch.int16), y.view(torch.int16)) for x, y in zip(a, b))
    assert not same(rows[0], rows[2]) and not same(rows[1], rows[2])
    for step, want in ((0, 0), (2, 2), (7, 2), (-3, 0)):
        got, after = at(step=step)
        assert after == step and same(got, rows[want]), step
    got, _ = at(with_step_ptr=False)
    assert same(got, rows[0])


def test_a_row_does_not_depend_on_its_batch(gpu):
    counts, skips3, resid3, table = data((16, 24), 3)
    got3, _ = launch(gpu, counts, skips3, resid3, table, 1)
    first = lambda ts: [t[:1].clone() for t in ts]
    got1, _ = launch(gpu, counts, first(skips3), [first(u) for u in resid3], table, 1)
    for k in range(13):
        assert torch.equal(got3[k][:1].view(torch.int16), got1[k].view(torch.int16)), k
    # the last row takes the conditional column: alone, as the one row of a launch with rows_u = 0
    last = lambda ts: [t[2:].clone() for t in ts]
    gotc, _ = launch(gpu, counts, last(skips3), [last(u) for u in resid3], table, 0)
    for k in range(13):
        assert torch.equal(got3[k][2:].view(torch.int16), gotc[k].view(torch.int16)), k


def test_zero_scales_read_nothing(gpu):
    """A (tap, row) whose scales are all zero keeps its bits even where its residuals are NaN; a unit whose scale is zero is not
    read, so its NaN does not appear, and the result is the launch's without that unit."""
    counts, skips, resid, table = data((8, 8), 3)
    nan = [[torch.full_like(r, float("nan")) for r in unit] for unit in resid]
    tab = np.repeat(table[1:2], 3, axis=0).copy()
    tab[:, :, 5, 0] = 0.0    # tap 5, the unconditional rows: every unit off
    tab[:, :, 12, :] = 0.0   # the mid block's tap (1 x 1 x 1280): off for every row
    mixed = [[(n_ if k in (5, 12) else r).clone() for k, (r, n_) in enumerate(zip(unit, bad))] for unit, bad in zip(resid, nan)]
    for k in (5,):   # only the u rows (rows_u = 2) of tap 5 are NaN: its last row is read
        for unit, src in zip(mixed, resid):
            unit[k][2:] = src[k][2:]
    got, _ = launch(gpu, counts, skips, mixed, tab, 2)
    assert torch.equal(got[5][:2].view(torch.int16), skips[5][:2].view(torch.int16)) and torch.equal(got[12].view(torch.int16), skips[12].view(torch.int16))
    assert all(bool(torch.isfinite(g.float()).all()) for g in got)
    assert not torch.equal(got[5][2:].view(torch.int16), skips[5][2:].view(torch.int16))
    # unit 1 at scale 0 everywhere, all of its residuals NaN == the launch of units 0 and 2 alone
    tab = np.repeat(table[1:2], 3, axis=0).copy()
    tab[:, 1] = 0.0
    got, _ = launch(gpu, counts, skips, [resid[0], nan[1], resid[2]], tab, 1)
    two, _ = launch(gpu, counts, skips, [resid[0], resid[2]], np.ascontiguousarray(tab[:, (0, 2)]), 1)
    for k in range(13):
        assert bool(torch.isfinite(got[k].float()).all()) and torch.equal(got[k].view(torch.int16), two[k].view(torch.int16)), k


def test_scale_one_is_the_fused_epilogue_bit_for_bit(gpu):
    """One unit at scale exactly 1: fmaf(1, r, skip) is skip + r rounded once, then one rounding to bf16 - the `v += residual` of
    the zero conv's fused epilogue."""
    for latent in LATENTS:
        counts, skips, resid, _ = data(latent, 2)
        got, _ = launch(gpu, counts, skips, resid[:1], np.ones((3, 1, 13, 2), dtype=np.float32), 1)
        for k in range(13):
            want = (skips[k].float() + resid[0][k]).to(torch.bfloat16)
            assert torch.equal(got[k].view(torch.int16), want.view(torch.int16)), (latent, k)


# ------------------------------------------------------------------------------------------------------------------- jobs
@pytest.fixture(scope="module")
def nets(gpu):
    """The synthetic UNet, decoder and encoder, and two ControlNet / HintNet pairs (seeds 0 and 1), at 64 x 64; the fixture sizes
    share their packed weights."""
    from minsdtf_amd.models import ControlNet, DiffusionModel, HintNet, ImageDecoder, ImageEncoder

    out = {}
    kinds = dict(unet=(DiffusionModel, 0), cn0=(ControlNet, 0), hn0=(HintNet, 0), cn1=(ControlNet, 1), hn1=(HintNet, 1))
    for name, (cls, seed) in kinds.items():
        m = cls(64, 64, device=gpu)
        m.load_synthetic(seed=seed, bias_scale=0.05)
        out[(name, 64)] = m
        for size in (128, 256):
            v = cls(size, size, device=gpu)
            v.share_weights(m)
            out[(name, size)] = v
    out["dec"] = ImageDecoder(device=gpu)
    out["dec"].load_synthetic(seed=0, bias_scale=0.05)
    out["enc"] = ImageEncoder(device=gpu)
    out["enc"].load_synthetic(seed=0, bias_scale=0.05)
    return out


def _pipe(gpu, nets, size=64, jit=True, control=True, **kw):
    from minsdtf_amd.stable_diffusion import StableDiffusion

    sd = StableDiffusion(size, size, jit_compile=jit, device=gpu, **(dict(controlnet_path="synthetic") if control else {}), **kw)
    sd._diffusion_model, sd._image_decoder, sd._image_encoder = nets[("unet", size)], nets["dec"], nets["enc"]
    if control:
        sd._control_net, sd._hint_net = nets[("cn0", size)], nets[("hn0", size)]
    return sd


_RNG = np.random.default_rng(77)
CTX = _RNG.standard_normal((77, 768)).astype(np.float32)
UNC = _RNG.standard_normal((77, 768)).astype(np.float32)
UNC_LONG = _RNG.standard_normal((154, 768)).astype(np.float32)
IMG = _RNG.integers(0, 256, (64, 64, 3)).astype(np.float32)
IMG2 = _RNG.integers(0, 256, (64, 64, 3)).astype(np.float32)
PICTURE = _RNG.integers(0, 256, (64, 64, 3)).astype(np.uint8)
KW = dict(batch_size=1, num_steps=3, unconditional_guidance_scale=7.5, guidance_rescale=0.7, seed=5, return_latent=True)


def _second(nets, size=64, **kw):
    return dict(image=IMG2, models=(nets[("cn1", size)], nets[("hn1", size)]), **kw)


def _job(sd, **kw):
    sd.unconditional_context = UNC
    return sd.generate_image(CTX, **{**KW, **kw})


@pytest.mark.parametrize("form", ["fused", "overlap_off", "two_streams", "long_negative", "tcd", "inpaint", "no_guidance", "euler_a"])
def test_all_ones_table_is_the_plain_controlnet_job(gpu, nets, form, monkeypatch):
    """control = one unit at its defaults: the fp32 zero convs and ONE rounding in msdc_control_combine against the fused epilogue's
    `v += residual`, final latent bit for bit - in every form an engine records a ControlNet job in, and with the states a
    ControlNet job goes with.  It holds because the zero conv keeps its tile and split-K configuration whatever its output type."""
    import minsdtf_amd.stable_diffusion as sdm

    if form == "overlap_off":
        monkeypatch.setattr(sdm, "CONTROLNET_OVERLAP", False)
    sd = _pipe(gpu, nets, **(dict(active_tcd=True) if form == "tcd" else {}))
    sd.denoise_streams = 2 if form == "two_streams" else None
    kw = dict(control_net_image=IMG)
    kw.update({"long_negative": dict(negative_prompt=UNC_LONG), "no_guidance": dict(unconditional_guidance_scale=0.0), "euler_a": dict(sampler="euler_a"),
               "inpaint": dict(reference_image=PICTURE, reference_image_strength=0.7, inpaint_mask=np.pad(np.full((32, 32), 255.0), 16))}.get(form, {}))

    def run(**more):
        np.random.seed(3)   # (the TCD sampler's draws come from numpy's global stream)
        return _job(sd, **kw, **more)

    plain = run()
    eng = next(iter(sd._engines.values()))
    assert eng.has_control and not eng.control_units and eng.dual == (form == "two_streams") and (eng.cn_plan is not None) == (form in ("fused", "tcd", "inpaint", "no_guidance", "euler_a"))
    assert len(eng.passes) == (2 if form in ("two_streams", "long_negative") else 1)
    ones = run(control={})
    eng = next(iter(sd._engines.values()))
    assert eng.control_units == 1 and sum(c.name == "control_combine" for c in eng.calls) == len(eng.passes)
    np.testing.assert_array_equal(ones, plain)
    assert not np.array_equal(run(control=dict(weight=0.5)), plain)


def test_weight_zero_is_the_job_without_a_controlnet(gpu, nets):
    sd = _pipe(gpu, nets)
    none = _job(sd)
    assert not next(iter(sd._engines.values())).has_control
    np.testing.assert_array_equal(_job(sd, control_net_image=IMG, control=dict(weight=0.0)), none)
    np.testing.assert_array_equal(_job(sd, control_net_image=IMG, control=[dict(weight=0.0, mode="control"), _second(nets, weight=[0.0] * 13)]), none)
    np.testing.assert_array_equal(_job(sd, control_net_image=IMG, control=dict(start=1.0)), none)   # (no step lies inside [1, 1])
    assert not np.array_equal(_job(sd, control_net_image=IMG), none)


@pytest.mark.parametrize("form", ["fused", "overlap_off", "two_streams"])
def test_a_second_unit_at_weight_zero_is_the_one_unit_job(gpu, nets, form, monkeypatch):
    import minsdtf_amd.stable_diffusion as sdm

    if form == "overlap_off":
        monkeypatch.setattr(sdm, "CONTROLNET_OVERLAP", False)
    sd = _pipe(gpu, nets)
    sd.denoise_streams = 2 if form == "two_streams" else None
    first = dict(weight=0.6, mode="prompt")
    one = _job(sd, control_net_image=IMG, control=first)
    two = _job(sd, control_net_image=IMG, control=[first, _second(nets, weight=0.0)])
    assert next(iter(sd._engines.values())).control_units == 2
    np.testing.assert_array_equal(two, one)
    three = _job(sd, control_net_image=IMG, control=[first, _second(nets, end=0.0), dict(image=IMG2, weight=0.0)])
    assert next(iter(sd._engines.values())).control_units == 3
    np.testing.assert_array_equal(three, one)
    on = _job(sd, control_net_image=IMG, control=[first, _second(nets, weight=0.7)])
    assert not np.array_equal(on, one)
    # the second unit alone == that ControlNet as the pipeline's own on its picture
    other = _pipe(gpu, nets)
    other._control_net, other._hint_net = nets[("cn1", 64)], nets[("hn1", 64)]
    other.denoise_streams = sd.denoise_streams
    alone = _job(sd, control_net_image=IMG, control=[dict(weight=0.0), _second(nets, weight=0.7)])
    np.testing.assert_array_equal(alone, _job(other, control_net_image=IMG2, control=dict(weight=0.7)))


def test_img2img_reads_the_rows_from_its_entry(gpu, nets):
    """strength 0.5 over 4 steps executes rows 2 and 3 of the table; end = 0.5 keeps rows 0 and 1 only: the job is weight 0."""
    sd = _pipe(gpu, nets)
    kw = dict(num_steps=4, reference_image=PICTURE, reference_image_strength=0.5, control_net_image=IMG)
    off = _job(sd, control=dict(weight=0.0), **kw)
    np.testing.assert_array_equal(_job(sd, control=dict(end=0.5), **kw), off)
    plain = _job(sd, **kw)
    np.testing.assert_array_equal(_job(sd, control=dict(start=0.5), **kw), plain)   # (rows 2 and 3 on: the whole executed part)
    assert not np.array_equal(plain, off)
    for sampler in ("dpmpp_2m",):
        off = _job(sd, control=dict(weight=0.0), sampler=sampler, **kw)
        np.testing.assert_array_equal(_job(sd, control=dict(end=0.5), sampler=sampler, **kw), off)
        assert not np.array_equal(_job(sd, control=dict(end=0.75), sampler=sampler, **kw), off)


def test_eager_per_step_graph_and_loop_graph_agree(gpu, nets):
    units = [dict(weight=0.8, mode="control"), _second(nets, weight=0.7, start=0.3)]
    loop = _job(_pipe(gpu, nets), control_net_image=IMG, control=units)
    calls = []
    stepped = _job(_pipe(gpu, nets), control_net_image=IMG, control=units, callback=calls.append)
    assert calls == [1, 2, 3]
    np.testing.assert_array_equal(stepped, loop)
    np.testing.assert_array_equal(_job(_pipe(gpu, nets, jit=False), control_net_image=IMG, control=units), loop)


def test_other_numbers_build_no_engine(gpu, nets, monkeypatch):
    import minsdtf_amd.stable_diffusion as sdm

    built = []
    init = sdm.DenoiseEngine.__init__

    def counting(self, *a, **k):
        built.append(k.get("control_units"))
        return init(self, *a, **k)

    monkeypatch.setattr(sdm.DenoiseEngine, "__init__", counting)
    sd = _pipe(gpu, nets)
    a = [dict(weight=0.8, mode="control"), _second(nets, weight=0.7, start=0.3)]
    b = [dict(weight=[0.1 * k for k in range(13)], end=0.7, mode="prompt"), _second(nets, weight=1.3, mode="control")]
    first = _job(sd, control_net_image=IMG, control=a)
    second = _job(sd, control_net_image=IMG, control=b)
    assert built == [2] and len(sd._engines) == 1
    np.testing.assert_array_equal(_job(sd, control_net_image=IMG, control=a), first)
    assert built == [2] and not np.array_equal(first, second)
    np.testing.assert_array_equal(_job(_pipe(gpu, nets), control_net_image=IMG, control=b), second)


@pytest.mark.parametrize("sampler, steps", [(None, 3), ("dpmpp_2m_karras", 8)])
def test_device_loop_vs_host_loop(gpu, nets, sampler, steps):
    """The device loop against host_loop=True (predict_on_batch of every unit's ControlNet, control.scale_host, predict_on_batch of the
    UNet with the 13 sums) at the bar tests/test_configs_gpu.py holds the ControlNet job's two loops to, 40 dB: the default step at
    3 steps, and the case tests/test_samplers_gpu.py holds a ControlNet job with a sampler to (dpmpp_2m_karras, 8 steps, the same bar).

    The host loop is the coarser of the two: ControlNet.predict_on_batch hands the residuals over rounded to bf16, the device loop
    scales and adds them in fp32.  Measured on one MI355X, device vs host, these inputs (plain ControlNet job / this job):
    default step 44.6 / 42.6 dB at 3 steps, 46.8 / 44.6 at 8; dpmpp_2m_karras 45.7 / 42.9 at 3, 45.8 / 44.1 at 8; euler_a 44.7 / 43.0
    at 3, 46.5 / 43.3 at 8; dpmpp_2m 46.9 / 44.3 at 8 - and 41.1 / 38.4 at 3 steps, where the plain job itself has 1 dB to spare:
    that schedule at 3 steps is not a case this bar can be asked of, and it is not asked here."""
    from oracle import sd_oracle as O

    sd = _pipe(gpu, nets)
    units = [dict(weight=0.8, mode="control"), _second(nets, weight=0.7, start=0.3)]
    kw = dict(control_net_image=IMG, control=units, sampler=sampler, num_steps=steps)
    dev = _job(sd, **kw)
    host = _job(sd, host_loop=True, **kw)
    plain = _job(sd, control_net_image=IMG, sampler=sampler, num_steps=steps)
    p, q = O.psnr(dev, host), O.psnr(plain, host)
    print(f"control units, sampler {sampler}, {steps} steps: device loop vs host loop {p:.1f} dB (the plain ControlNet job against it: {q:.1f} dB)")
    assert p >= PSNR_MIN and q < PSNR_MIN


def test_sharded_job_equals_unsharded(gpu):
    """A one-rank process group with forced collectives (as tests/test_dynthresh_gpu.py): the sharded job == the unsharded one."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, os.path.join(HERE, "_control_units_world1_child.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=570)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert any(line.startswith("OK ") for line in p.stdout.splitlines()), p.stdout[-2000:]
    print(p.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("size", [128, 256])
def test_vs_oracle_fixture(gpu, nets, size):
    """The fixture jobs against the fp32 oracle's composition (tools/make_control_units_fixtures.py: hintnet_forward,
    controlnet_forward per unit, the scaled sums through unet_forward(controls=...), OracleScheduler.step): final latent PSNR >= 40 dB,
    where the plain ControlNet job and the job without a ControlNet stay under 35 dB (`plain_psnr`, `none_psnr` in the file)."""
    from oracle import sd_oracle as O

    g = np.load(os.path.join(GOLD, f"control_units_{size}.npz"))
    assert (int(g["weight_seed"]), float(g["bias_scale"])) == (0, 0.05) and float(g["plain_psnr"]) < 35.0 and float(g["none_psnr"]) < 35.0
    sd = _pipe(gpu, nets, size)
    rng = np.random.default_rng(int(g["context_seed"]))
    ctx = rng.standard_normal((1, 77, 768)).astype(np.float32)[0]
    sd.unconditional_context = rng.standard_normal((1, 77, 768)).astype(np.float32)[0]
    pictures = [np.random.default_rng(int(g["hint_seed"]) + n).integers(0, 256, (size, size, 3)).astype(np.float32) for n in range(int(g["units"]))]
    units = []
    for n in range(int(g["units"])):
        u = dict(weight=float(g[f"unit{n}_weight"]), start=float(g[f"unit{n}_start"]), end=float(g[f"unit{n}_end"]), mode=str(g[f"unit{n}_mode"]))
        if n:
            u.update(image=pictures[n], models=(nets[(f"cn{n}", size)], nets[(f"hn{n}", size)]))
        units.append(u)
    got = sd.generate_image(ctx, batch_size=1, num_steps=int(g["steps"]), unconditional_guidance_scale=float(g["guidance"]),
                            seed=int(g["noise_seed"]), guidance_rescale=float(g["rescale"]), return_latent=True,
                            control_net_image=pictures[0], control=units)
    p = O.psnr(got, g["latent"])
    print(f"control units fixture {size}x{size} ({len(units)} unit(s)): final latent PSNR {p:.1f} dB; the plain ControlNet job "
          f"{float(g['plain_psnr']):.1f} dB, the job without a ControlNet {float(g['none_psnr']):.1f} dB")
    assert p >= PSNR_MIN
