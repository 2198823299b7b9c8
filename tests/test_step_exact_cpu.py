"""CPU tests (no GPU) of tests/test_step_exact_gpu.py: every case of that module walked through a numpy float32 restatement of the
kernel's formula (_exact_step.emulate: the operations as written, the moments per thread, per wave and across the sixteen waves),
and both of its checkers run on the result.  That proves the case list exact (AExact asserts every product, sum and quotient of
every exact-stage case to be a float32) and the derived bounds reachable by the formula alone: R + 1 for the factor, the running-
error bound for real operands.

Then seven emulated faults (_exact_step.FAULTS), each on the case that exists to see it; each must be refused by the new checks.
OLD_BOUND_ACCEPTS records what test_cfg_step's / test_sampler_step's comparison (rtol 2e-4, atol 2e-4 max |ref|) says of the same
faulty result: the faults it accepts are the gap this module and its GPU twin close; those it refuses went unseen only because no
test ran the case (a ragged size, a preset counter, the inpaint operands of msd_cfg_step).  If an entry flips, say so here."""
import numpy as np
import pytest

import _exact_step as E
import test_step_exact_gpu as T


def _refused(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def test_option_coverage():
    """Each size sees every option value; each option value sees each of the three forms; every form has its smallest size."""
    seen = {}
    for c in T.EXACT_CASES:
        for opt in (("g", c["guidance"] > 0), ("z", c["noise"]), ("ip", c["inpaint"])):
            seen.setdefault((c["kind"], c["n"]), set()).add(opt)
            seen.setdefault((c["kind"], opt), set()).add(E.form_of(c["n"]))
    for k, v in seen.items():
        assert len(v) == (6 if isinstance(k[1], int) else 3), (k, v)
    assert [E.form_of(n) for n in (4, 16384, 16388, 36864, 36868, 4098, 3)] == [16, 16, 36, 36, 0, 0, 0]
    assert E.form_of(4096, aligned=False) == 0
    assert {E.form_of(n) for n in T.CHAIN_SIZES} == {E.form_of(n) for n in T.REAL_SIZES} == {0, 16, 36}
    assert [E.per_thread(n, E.form_of(n)) for n in (4, 4100, 16384, 16388, 36864, 36868, 40000, 1023)] == [4, 8, 16, 20, 36, 37, 40, 1]
    for tab in (E.FRAC4, E.FRAC8[:, :6], E.FRAC_NOISE[:, None]):
        assert all(len(set(col)) == len(col) for col in tab.T), "two fractional rows share a value in a column"
    assert E.FRAC8[0, 4] == 0 and (E.FRAC8[1:, 4] != 0).all()


@pytest.mark.parametrize("c", T.EXACT_CASES, ids=[T.case_id(c) for c in T.EXACT_CASES])
def test_exact_cases_are_exact(c):
    p = E.exact_problem(**c)
    ref = E.reference(p)
    assert p.top <= 128, p.top
    E.check_run(E.emulate(p, E.form_of(p.n)), ref, p.id)


def test_other_exact_cases_are_exact():
    """The misaligned, chained and counter cases, built as the GPU module builds them."""
    ps = [E.exact_problem(k, 4096, noise=True, inpaint=ip, step0=1) for k in T.KINDS for ip in (True, False)]
    ps += [E.exact_problem(k, n, noise=True, inpaint=True, chained=True) for k in T.KINDS for n in T.CHAIN_SIZES]
    ps += [E.exact_problem(k, 252, B=B, noise=True, chained=True) for k in T.KINDS for B in (1, 3, 17)]
    ps += [E.exact_problem(k, 256, noise=True, step0=s, advance=0) for k in T.KINDS for s in (2, None)]
    ps += [E.exact_problem(k, 4100, noise=True, inpaint=True, step0=s, advance=a) for k in T.KINDS for s in (-3, 6) for a in (1, 2)]
    ps += [E.exact_problem(k, 4100, guidance=-1.0, inpaint=True, step0=3, case_id=f"{k}/guidance off") for k in T.KINDS]
    top = 0.0
    for p in ps:
        ref = E.reference(p)
        E.check_run(E.emulate(p, E.form_of(p.n)), ref, p.id)
        top = max(top, p.top)
        if p.step0 in (-3, 6):
            assert ref[0][2] == p.step0 + 1            # the counter the kernel stores today: what it read, plus one
        if p.advance == 0:
            assert ref[0][2] == p.step0
    print(f"\nRECORD | the largest magnitude of a chained run: {top:g} (2^24 = {E.LIMIT})")
    assert top < E.LIMIT / 256


@pytest.mark.parametrize("c", T.MOMENT_CASES, ids=[T.case_id(c) for c in T.MOMENT_CASES])
def test_moment_cases(c):
    p = E.moment_problem(**c)
    form = E.form_of(p.n)
    res = E.emulate(p, form)
    worst = E.check_factor(res[0][0], p, p.id)
    # the four moments are integers: the emulation's fp32 sums are the float64 ones
    u, cc = p.us[0], p.cs[0]
    e = E.guided(u, cc, p.guidance)
    for t in (cc.astype(np.float64), e):
        d = t - t[:, :1]
        for b in range(p.B):
            assert E._block_sum(d[b], form) == d[b].sum() and E._block_sum(d[b] * d[b], form) == (d[b] * d[b]).sum()
    print(f"\nRECORD | factor, emulated | {p.id} | {worst:.2f} x 2^-24 of {E.R_FACTOR + 1}")


@pytest.mark.parametrize("c", T.REAL_CASES, ids=[T.case_id(c) for c in T.REAL_CASES])
def test_real_cases(c):
    p = T.real_problem(c)
    form = E.form_of(p.n)
    bound = E.real_bound(p, form)
    worst, rel = E.check_real(E.emulate(p, form), bound, p.id)
    ref = E.walk(p, E.A64())
    for (rl, rp, _), (bl, bp, _) in zip(ref, bound):     # the bound's value IS the float64 reference
        assert np.allclose(rl, bl[0], rtol=1e-12, atol=1e-12)
    print(f"\nRECORD | real, emulated | {p.id} {c['table']} | measured / bound {worst:.3f} | largest bound {rel:.3g} of max |ref|")
    if not c.get("outlier"):      # (about a shift 8 sigma out the variance is a difference of numbers 65 / 600 times its size: the bound says so)
        assert rel < E.OLD_RTOL, "the derived bound is no tighter than the old one"


# ---- the emulated faults ----------------------------------------------------------------------------------------------------------------
OLD_BOUND_ACCEPTS = {
    "last quad": False,
    "other sample's factor": False,
    "unshifted moments": True,
    "noise row": False,
    "inpaint A B": False,
    "reads P": False,
    "row": False,
}


def _fault_case(fault):
    """(problem, the new check on a run of it)."""
    def exact(p):
        ref = E.reference(p)
        return p, ref, lambda run: E.check_run(run, ref, p.id)

    def factor(p):
        return p, E.walk(p, E.A64()), lambda run: E.check_factor(run[0][0], p, p.id)
    if fault == "last quad":
        return exact(E.exact_problem("multi", 16388, noise=True, step0=1))
    if fault == "other sample's factor":
        return factor(E.moment_problem("cfg", 16384, 0.7))
    if fault == "unshifted moments":
        return factor(E.moment_problem("cfg", 40000, 0.7, offset=100))
    if fault == "noise row":
        return exact(E.exact_problem("cfg", 4100, noise=True, inpaint=True, step0=-3))
    if fault == "inpaint A B":
        return exact(E.exact_problem("cfg", 4100, inpaint=True, step0=2))
    if fault == "reads P":
        return exact(E.exact_problem("multi", 256, step0=0))
    if fault == "row":
        return exact(E.exact_problem("multi", 4100, noise=True, inpaint=True, step0=6))
    raise KeyError(fault)


@pytest.mark.parametrize("fault", E.FAULTS)
def test_fault_is_refused(fault):
    p, ref, check = _fault_case(fault)
    form = E.form_of(p.n)
    check(E.emulate(p, form))                                       # the right formula passes
    run = E.emulate(p, form, fault=fault)
    assert _refused(lambda: check(run)), f"{fault}: the new check accepts it"
    old = all(E.old_bound_accepts(g[0], r[0]) and (r[1] is None or E.old_bound_accepts(g[1], r[1])) for g, r in zip(run, ref))
    print(f"\nRECORD | fault | {fault} | {p.id} | refused by the new check | the 2e-4 bound {'ACCEPTS' if old else 'refuses'} it")
    assert old == OLD_BOUND_ACCEPTS[fault], f"{fault}: the old bound now {'accepts' if old else 'refuses'} it"


def test_factor_faults_on_real_operands():
    """Faults 2 and 3, and a factor that is off by 1e-4, on test_cfg_step's own kind of data (randn, batch 3, 64x64, five steps).
    Another sample's factor is off by the sampling error of a standard deviation, about 1 / sqrt(2 n) = 5e-3 here: both bounds refuse
    it (at 96x96 and beyond it comes within reach of 2e-4).  A relative error of 1e-4 in the factor - 1700 ulp - passes the old
    bound and misses the running-error bound by a factor of ten or more.  One-pass moments about 0 are as good as shifted ones on
    zero-mean data: no fault there, both accept - which is why the moment stage has cases about 100."""
    p = T.real_problem(dict(kind="cfg", n=16384, table="ddim"))
    bound = E.real_bound(p, 16)
    ref = E.walk(p, E.A64())

    def old(run):
        return all(E.old_bound_accepts(g[0], r[0]) for g, r in zip(run, ref))
    run = E.emulate(p, 16, fault="other sample's factor")
    assert _refused(lambda: E.check_real(run, bound, p.id)) and not old(run)
    off = E.walk(p, E.A32(), factors=lambda i, u, c: (E.factor32(u, c, p.guidance, p.rescale, 16) * np.float32(1 + 1e-4))[:, None])
    assert _refused(lambda: E.check_real(off, bound, p.id)) and old(off)
    worst = max(float((np.abs(g[0] - r[0]) / b[0][1]).max()) for g, r, b in zip(off, ref, bound))
    print(f"\nRECORD | fault | factor off by 1e-4 on randn operands | {worst:.1f} x the running-error bound | the 2e-4 bound ACCEPTS it")
    assert worst > 10
    E.check_real(E.emulate(p, 16, fault="unshifted moments"), bound, p.id)
    assert old(E.emulate(p, 16, fault="unshifted moments"))


def test_checkers_see_one_ulp():
    """check_bits refuses one ulp and a zero of the other sign; check_factor refuses one element that took its neighbour's factor."""
    p = E.exact_problem("cfg", 256)
    ref = E.reference(p)
    got = ref[0][0].astype(np.float32)
    E.check_bits(got, ref[0][0], "as is")
    bad = got.copy()
    bad[1, 7] = np.nextafter(bad[1, 7], np.float32(np.inf))
    assert _refused(lambda: E.check_bits(bad, ref[0][0], "one ulp"))
    q = E.moment_problem("cfg", 4100, 0.7)
    x = E.emulate(q, 16)[0][0]
    E.check_factor(x, q, "as is")
    e = E.guided(q.us[0], q.cs[0], q.guidance)
    i = int(np.argmax(np.abs(e[0])))
    x2 = x.copy()
    x2[0, i] = np.float32(e[0, i] * float(E.factor32(q.us[0], q.cs[0], q.guidance, q.rescale, 16)[1]))
    assert _refused(lambda: E.check_factor(x2, q, "one element on sample 1's factor"))
