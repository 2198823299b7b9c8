"""msd_cfg_step and msd_sampler_step on dyadic operands, and the small elementwise helpers bit for bit (tests/_exact_step.py).

test_cfg_step and test_sampler_step hold these kernels to rtol 2e-4 / atol 2e-4 max |ref| on randn data at four sizes, each a
form's full size or a multiple of 1024 quads.  Here:

  test_exact               one launch from a preset counter on the fractional rows: both kernels, every size of VEC4_SIZES (the first,
                           the last and the first ragged quad pass of each register form) and GENERIC_SIZES (n % 4 != 0, n < 4),
                           two option sets per size so that every size meets guidance 7.5 / 0, step_noise on / off and the inpaint
                           blend on / off, and every option meets each of the three forms; `latent` and `denoised_prev` carry the
                           float64 reference's bits
  test_exact_misaligned    n = 4096 with one operand 4 bytes off a 16-byte boundary (the generic form must take it): eps, latent,
                           and for msd_sampler_step denoised_prev and step_noise
  test_exact_chain         five chained launches on integer rows, one size per form, every option on; P starts as NaN
  test_counter_*           advance 0, step_ptr NULL, presets below and above the range (the row AND the step_noise row are clamped,
                           the stored counter is not), the ticket at batch 1 / 3 / 17, guidance < 0, rescale without guidance
  test_moments             the rescale factor read back through the probe row: within (R + 1) 2^-24 of the float64 factor and ONE
                           factor per sample (check_factor); constant c (factor = 1 - rescale exactly), u == c constant
  test_one_wrong_operand_  the same checks refuse a launch whose coefficient row or whose c differs in one number
  is_seen
  test_real                randn operands on Scheduler.coefficient_table() / the TCD table with draws / dpmpp_2m /
                           dpmpp_2m_sde_karras, five chained launches per form against the running-error bound; one case with c[b][0]
                           eight standard deviations out
  test_batch_independence  sample b of a batch-17 launch = the same sample launched alone, bit for bit (rescale on, real operands)
  test_add_exact / _cast_  msd_add_bf16 / msd_add_f32_bf16 at n = 8 and at the first n that needs the grid-stride pass, the two
                           casts at n = 1, 1001 and 4096 * 256 + 1: bit-equal to torch

Every operand sits between guard bands (tests/_guard.py, sized by tests/_extents.py); a misaligned operand is the 4-byte-offset view of
a guarded buffer one float larger, whose first float must stay NaN.

Measured on an MI355X (this module's first run: 164 tests in 4.3 s, none refused; test_one_wrong_operand_is_seen's two came after it
and passed with the whole suite; the RECORD lines print the same figures again):
  exact stage     every launch bit-equal; the largest magnitude of a five-step chain is 572
  factor          |x' / e - factor| / factor at its largest, in units of 2^-24 (the bound is R + 1 = 9):
                  NPT 16  2.50 (n 256, rescale 1.0)   NPT 36  1.40   the loop  2.62 (n 1023, rescale 1.0);  about 100: 1.73
  real operands   measured / bound at its largest: NPT 16  0.715   NPT 36  0.634   the loop  0.595  (bounds of 6e-6 .. 1.7e-4 of max |ref|)
  outlier shift   c[b][0] eight standard deviations out: measured / bound 0.194 (msd_cfg_step) and 0.200 (msd_sampler_step); the
                  bound itself grows to 2.7e-3 / 7.4e-3 of max |ref| (the variance about that shift is a difference 65 / 600 times
                  its size)
The numpy float32 restatement (tests/test_step_exact_cpu.py) gives the same ratios to three digits in most real-operand cases: the
kernel's error is the formula's own."""
import numpy as np
import pytest
import torch

import _exact_step as E
import _extents as X
import _guard as G
from conftest import run_calls

pytestmark = pytest.mark.gpu

NAN = float("nan")
KINDS = ("cfg", "multi")
VEC4_SIZES = [4, 8, 252, 256, 4096, 4100, 16380, 16384, 16388, 36864, 36868]
GENERIC_SIZES = [1, 2, 3, 6, 1023, 1025, 4098]
# (guidance, step_noise, inpaint): sizes at even / odd positions of the list take the first / second pair
OPTION_PAIRS = ([(7.5, True, False), (0.0, False, True)], [(7.5, False, True), (0.0, True, False)])
CHAIN_SIZES = [4100, 16388, 36868]          # NPT 16, NPT 36, the loop; each with a ragged last pass
MISALIGNED = {"cfg": ["eps", "latent"], "multi": ["eps", "latent", "denoised_prev", "step_noise"]}
MOMENT_SIZES = [256, 1023, 4100, 16384, 16388, 36864, 40000]
RESCALES = [0.25, 0.7, 1.0]
REAL_SIZES = [256, 16384, 36864, 40000]


def exact_cases():
    out = []
    for kind in KINDS:
        for i, n in enumerate(VEC4_SIZES + GENERIC_SIZES):
            for guidance, noise, inpaint in OPTION_PAIRS[i % 2]:
                out.append(dict(kind=kind, n=n, guidance=guidance, noise=noise, inpaint=inpaint, step0=i % 4))
    return out


def case_id(c):
    return "-".join(f"{k}{v}" if k not in ("kind",) else str(v) for k, v in c.items())


EXACT_CASES = exact_cases()
MOMENT_CASES = ([dict(kind="cfg", n=n, rescale=r) for n in MOMENT_SIZES for r in RESCALES]
                + [dict(kind="multi", n=n, rescale=0.7) for n in MOMENT_SIZES]
                + [dict(kind=k, n=n, rescale=0.7, mode=m) for k in KINDS for n in (1023, 16388) for m in ("const c", "const")]
                # the same integers about 100: the kernel's shifted moments are as exact, one-pass moments about 0 are not
                + [dict(kind="cfg", n=n, rescale=0.7, offset=100) for n in (4100, 40000)])
REAL_CASES = ([dict(kind="cfg", n=n, table="ddim") for n in REAL_SIZES] + [dict(kind="cfg", n=16384, table="tcd", noise=True)]
              + [dict(kind="multi", n=n, table="dpmpp_2m") for n in REAL_SIZES]
              + [dict(kind="multi", n=n, table="dpmpp_2m_sde_karras", noise=True) for n in REAL_SIZES]
              + [dict(kind=k, n=16384, table=t, outlier=8.0) for k, t in (("cfg", "ddim"), ("multi", "dpmpp_2m"))])


def real_table(name, steps=5):
    """The project's own fp32 tables."""
    from minsdtf_amd import samplers
    from minsdtf_amd.scheduler import Scheduler

    sch = Scheduler(active_tcd=name == "tcd")
    sch.set_timesteps(steps)
    if name == "tcd":
        return sch.coefficient_table(), sch.noise_coefficients()
    if name == "ddim":
        return sch.coefficient_table()
    return samplers.coefficient_table(samplers.schedule(samplers.parse(name), sch, steps))


def real_problem(c):
    kw = {k: v for k, v in c.items() if k not in ("kind", "n", "table")}
    return E.real_problem(c["kind"], c["n"], real_table(c["table"]), **kw)


# ---- one guarded launch sequence -------------------------------------------------------------------------------------------------------
class Run:
    """p's operands on the device, every one between guard bands; launch(i) launches once and returns (latent, P, counter)."""
    def __init__(self, gpu, p, misaligned=None):
        from minsdtf_amd import ops

        self.p, self.gpu, self.off, self.misaligned = p, gpu, [], misaligned
        self.multi = p.kind == "multi"
        self.fn = ops.sampler_step if self.multi else ops.cfg_step
        self.geo = dict(batch=p.B, n=p.n, num_steps=p.S, guidance=p.guidance, guidance_rescale=p.rescale, advance=p.advance)
        present = dict(eps=1, latent=1, coef=1, step_ptr=None if p.step0 is None else 1)
        if self.multi:
            present["denoised_prev"] = 1
        if p.z is not None:
            present["step_noise"] = 1
            if not self.multi:
                present["noise_coef"] = 1
        if p.ip is not None:
            present.update(inpaint_init=1, inpaint_noise=1, inpaint_mask=1)
        self.g = g = G.Guard(gpu, (X.sampler_step if self.multi else X.cfg_step)(**present, **self.geo))
        self.kw = dict(coef=g.inp(torch.from_numpy(np.ascontiguousarray(p.coef)), "coef"))
        self.lat = self.kw["latent"] = self._operand(p.lat, "latent")
        self.step = None
        if p.step0 is not None:
            self.step = g.inp(torch.tensor([p.step0, 0][:2 if p.advance == 2 else 1], dtype=torch.int32), "step_ptr")
        self.kw["step_ptr"] = self.step
        self.P = None
        if self.multi:
            self.P = self.kw["denoised_prev"] = self._operand(p.P0, "denoised_prev")
        if p.z is not None:
            self.kw["step_noise"] = self._operand(p.z, "step_noise")
            if not self.multi:
                self.kw["noise_coef"] = g.inp(torch.from_numpy(np.ascontiguousarray(p.noise_coef)), "noise_coef")
        if p.ip is not None:
            for name, v in zip(("inpaint_init", "inpaint_noise", "inpaint_mask"), p.ip):
                self.kw[name] = g.inp(torch.from_numpy(np.ascontiguousarray(v)), name)

    def _operand(self, array, name, label=None):
        t = torch.from_numpy(np.ascontiguousarray(array))
        if name != self.misaligned:
            return self.g.inp(t, name, label=label)
        buf = self.g.out((t.numel() + 1,), torch.float32, NAN, label=f"{label or name}, 4 bytes off")
        view = buf[1:].view(t.shape)
        assert view.data_ptr() % 16 == 4
        view.copy_(t)
        self.off.append(buf)
        return view

    def eps(self, i):
        p = self.p
        return np.concatenate([p.us[i], p.cs[i]]) if p.guidance > 0 else p.us[i]

    def launch(self, i):
        eps = self._operand(self.eps(i), "eps", label=f"eps of launch {i}")
        run_calls(self.fn(eps=eps, **self.kw, **self.geo))
        return (self.lat.cpu().numpy(), self.P.cpu().numpy() if self.multi else None, None if self.step is None else int(self.step[0]))

    def run(self):
        return [self.launch(i) for i in range(self.p.launches)]

    def check(self):
        self.g.check()
        for buf in self.off:
            assert bool(torch.isnan(buf[0])), "the float in front of a misaligned operand was written"
        if self.step is not None and self.step.numel() == 2:
            assert int(self.step[1]) == 0, f"the ticket is {int(self.step[1])} after the launch"


def run_exact(gpu, p, what, **kw):
    ref = E.reference(p)
    r = Run(gpu, p, **kw)
    E.check_run(r.run(), ref, what)
    r.check()
    return r


# ---- the exact stage --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", EXACT_CASES, ids=[case_id(c) for c in EXACT_CASES])
def test_exact(gpu, c):
    p = E.exact_problem(**c)
    run_exact(gpu, p, f"{p.id} [NPT {E.form_of(p.n)}]")


@pytest.mark.parametrize("kind,operand", [(k, o) for k in KINDS for o in MISALIGNED[k]])
def test_exact_misaligned(gpu, kind, operand):
    p = E.exact_problem(kind, 4096, guidance=7.5, noise=True, inpaint=operand in ("eps", "latent"), step0=1)
    run_exact(gpu, p, f"{p.id}, {operand} 4 bytes off a 16-byte boundary", misaligned=operand)


@pytest.mark.parametrize("n", CHAIN_SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_exact_chain(gpu, kind, n):
    p = E.exact_problem(kind, n, guidance=7.5, noise=True, inpaint=True, chained=True)
    assert kind == "cfg" or bool(np.isnan(p.P0).all())
    run_exact(gpu, p, f"{p.id} [NPT {E.form_of(n)}]")
    print(f"\nRECORD | chain | {p.id} | NPT {E.form_of(n)} | largest magnitude {p.top:g}")


# ---- the counter ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_counter_advance_0_and_null(gpu, kind):
    """advance 0 leaves *step_ptr alone (and needs no ticket word); step_ptr = NULL uses row 0."""
    p = E.exact_problem(kind, 256, noise=True, step0=2, advance=0)
    r = run_exact(gpu, p, f"{p.id}, advance 0")
    assert r.step.tolist() == [2]
    p = E.exact_problem(kind, 256, noise=True, step0=None, advance=0)
    run_exact(gpu, p, f"{p.id}, step_ptr NULL")
    assert E.clamp_row(None, 4) == (0, 0)


@pytest.mark.parametrize("advance", [1, 2])
@pytest.mark.parametrize("preset", [-3, 6])
@pytest.mark.parametrize("kind", KINDS)
def test_counter_out_of_range(gpu, kind, preset, advance):
    """A counter of -3 / num_steps + 2 takes row 0 / the last row of the table AND of step_noise (rows differ in every column, the
    draws in every row); what the kernel stores is the counter it read plus one: -2 / num_steps + 3."""
    p = E.exact_problem(kind, 4100, noise=True, inpaint=True, step0=preset, advance=advance)
    assert p.S == 4 and E.clamp_row(preset, 4)[0] == (0 if preset < 0 else 3)
    r = run_exact(gpu, p, f"{p.id}, counter preset to {preset}, advance {advance}")
    assert int(r.step[0]) == preset + 1


@pytest.mark.parametrize("B", [1, 3, 17])
@pytest.mark.parametrize("kind", KINDS)
def test_counter_ticket(gpu, kind, B):
    """advance 2: the workgroup that draws the last ticket moves the counter and returns the ticket to 0 - at batch 1 (its own last
    ticket), 3 and 17, over five chained launches."""
    p = E.exact_problem(kind, 252, B=B, noise=True, chained=True)
    r = run_exact(gpu, p, f"{p.id}, batch {B}")
    assert r.step.tolist() == [5, 0]


@pytest.mark.parametrize("kind", KINDS)
def test_counter_guidance_off(gpu, kind):
    """A negative guidance behaves as 0: eps is [batch][n] (the guard band follows row batch - 1) and guidance_rescale is ignored."""
    for guidance, rescale in ((-1.0, 0.0), (0.0, 0.7), (-2.5, 0.7)):
        p = E.exact_problem(kind, 4100, guidance=guidance, inpaint=True, step0=3, case_id=f"{kind}/guidance off")
        ref = E.reference(p)
        p.rescale = rescale
        r = Run(gpu, p)
        assert r.eps(0).shape == (p.B, p.n)
        E.check_run(r.run(), ref, f"{p.id}, guidance {guidance}, rescale {rescale}")
        r.check()


# ---- the moment stage -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", MOMENT_CASES, ids=[case_id(c) for c in MOMENT_CASES])
def test_moments(gpu, c):
    p = E.moment_problem(**c)
    r = Run(gpu, p)
    lat, _, counter = r.launch(0)
    worst = E.check_factor(lat, p, p.id)
    r.check()
    assert counter == 1
    print(f"\nRECORD | factor | {p.id} | NPT {E.form_of(p.n)} | {worst:.2f} x 2^-24 of {E.R_FACTOR + 1} | sums {p.sums}")


@pytest.mark.parametrize("kind", KINDS)
def test_one_wrong_operand_is_seen(gpu, kind):
    """The checks end to end, on the device.  The launch runs on valid operands that differ from the reference's in ONE number: a
    quarter added to one entry of the coefficient row; then 1 added to one element of c (the sum of squares of c moves by a few
    parts in 10^4, the factor by half of that).  Both are refused against the reference and accepted against their own."""
    p = E.exact_problem(kind, 4100, noise=True, inpaint=True, step0=2)
    ref = E.reference(p)
    q = E.exact_problem(kind, 4100, noise=True, inpaint=True, step0=2)
    q.coef = p.coef.copy()
    q.coef[2, 3] += 0.25
    got = Run(gpu, q).run()
    E.check_run(got, E.reference(q), q.id)
    with pytest.raises(AssertionError, match="latent after launch 0"):
        E.check_run(got, ref, p.id)
    p = E.moment_problem(kind, 16388, 0.7)
    q = E.moment_problem(kind, 16388, 0.7)
    q.cs[0][2, 16387] += 1
    lat = Run(gpu, q).launch(0)[0]
    E.check_factor(lat, q, q.id)
    with pytest.raises(AssertionError, match="sample 2"):
        E.check_factor(lat, p, p.id)


# ---- the real-operand stage -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", REAL_CASES, ids=[case_id(c) for c in REAL_CASES])
def test_real(gpu, c):
    p = real_problem(c)
    bound = E.real_bound(p, E.form_of(p.n))
    r = Run(gpu, p)
    worst, rel = E.check_real(r.run(), bound, p.id)
    r.check()
    print(f"\nRECORD | real | {p.id} {c['table']} | NPT {E.form_of(p.n)} | measured / bound {worst:.3f} | largest bound {rel:.3g} of max |ref|")


@pytest.mark.parametrize("n", [16384, 40000])
@pytest.mark.parametrize("kind", KINDS)
def test_batch_independence(gpu, kind, n):
    table = "ddim" if kind == "cfg" else "dpmpp_2m_sde_karras"
    p = E.real_problem(kind, n, real_table(table), B=17, steps=2, noise=kind == "multi")
    whole = Run(gpu, p).run()
    for b in (0, 8, 16):
        q = E.real_problem(kind, n, real_table(table), B=17, steps=2, noise=kind == "multi")
        q.B, q.lat = 1, p.lat[b:b + 1]
        q.us, q.cs = [u[b:b + 1] for u in p.us], [c_[b:b + 1] for c_ in p.cs]
        q.z = None if p.z is None else p.z[:, b:b + 1]
        q.P0 = None if p.P0 is None else p.P0[b:b + 1]
        r = Run(gpu, q)
        alone = r.run()
        r.check()
        for i in range(p.launches):
            assert np.array_equal(E.bits(alone[i][0][0]), E.bits(whole[i][0][b])), f"{p.id}: sample {b}, latent after launch {i}"
            if kind == "multi":
                assert np.array_equal(E.bits(alone[i][1][0]), E.bits(whole[i][1][b])), f"{p.id}: sample {b}, P after launch {i}"


# ---- the elementwise helpers ------------------------------------------------------------------------------------------------------------
def _rows(n):
    """A 2-D shape of n elements with short rows (the guard band is 256 rows)."""
    for cols in (8, 17, 13, 7, 1):
        if n % cols == 0 and n > cols:
            return n // cols, cols
    return (n,)


@pytest.mark.parametrize("n", [8, 8 * 4096 * 256 + 8])
def test_add_exact(gpu, n):
    from minsdtf_amd import ops

    bf = torch.bfloat16
    gen = torch.Generator().manual_seed(n)
    a, b, c = (torch.randn(_rows(n), generator=gen) for _ in range(3))
    g = G.Guard(gpu)
    g.bind("add.", X.add_bf16(n=n))
    g.bind("mix.", X.add_f32_bf16(n=n))
    out = g.out(_rows(n), bf, NAN, "add.out")
    run_calls(ops.add_bf16(a=g.inp(a.to(bf), "add.a"), b=g.inp(b.to(bf), "add.b"), out=out, n=n))
    assert torch.equal(out.cpu().view(torch.int16), (a.to(bf).float() + b.to(bf).float()).to(bf).view(torch.int16))
    out = g.out(_rows(n), bf, NAN, "mix.out")
    run_calls(ops.add_f32_bf16(a=g.inp(a.to(bf), "mix.a"), b=g.inp(c, "mix.b"), out=out, n=n))
    assert torch.equal(out.cpu().view(torch.int16), (a.to(bf).float() + c).to(bf).view(torch.int16))
    g.check()


@pytest.mark.parametrize("n", [1, 1001, 4096 * 256 + 1])
def test_cast_exact(gpu, n):
    from minsdtf_amd import ops

    bf = torch.bfloat16
    x = torch.randn(_rows(n), generator=torch.Generator().manual_seed(n))
    g = G.Guard(gpu)
    g.bind("f2b.", X.cast_f32_to_bf16(n=n))
    g.bind("b2f.", X.cast_bf16_to_f32(n=n))
    o = g.out(_rows(n), bf, NAN, "f2b.out")
    run_calls(ops.cast_f32_to_bf16(x=g.inp(x, "f2b.x"), out=o, n=n))
    assert torch.equal(o.cpu().view(torch.int16), x.to(bf).view(torch.int16))
    o2 = g.out(_rows(n), torch.float32, NAN, "b2f.out")
    run_calls(ops.cast_bf16_to_f32(x=g.same(o, "b2f.x"), out=o2, n=n))
    assert torch.equal(o2.cpu().view(torch.int32), x.to(bf).float().view(torch.int32))
    g.check()
