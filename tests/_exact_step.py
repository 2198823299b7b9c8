"""Dyadic operands for the two step kernels (msd_cfg_step, msd_sampler_step; csrc/elementwise.hip): a float64 statement of both,
taken from the formulas of include/minsdtf_hip.h, and three checkers that leave the kernels no tolerance they have not earned.

The statement (`walk`) is written ONCE, over an arithmetic: the same lines run in float64 (A64: the reference), in float64 with
every product, sum and quotient asserted to be its own float32 round trip (AExact: the exact stage's condition), in numpy float32
in the kernel's operation order (A32: what a right kernel leaves, and - with `fault` - what a wrong one would), and on (value,
bound) pairs (AErr: the forward running-error bound of the real-operand stage).

  e  = u + guidance (c - u), times `factor` where guidance_rescale > 0      (guidance <= 0: e = eps as is, rescale ignored)
  factor = rescale std(c) / (std(e) + 1e-5f) + (1 - rescale)                (population std over the sample)
  msd_cfg_step      row {signal, noise, A, B}:   x0 = (x - noise e) / signal,  x' = A x0 + B e  (+ noise_coef[row] z[row])
  msd_sampler_step  row {alpha, sigma, c_x, c_D, c_P, c_z, 0, 0}:  D = (x - sigma e) / alpha,
                    x' = c_x x + c_D D + c_P P (read only where c_P != 0) + c_z z[row],  then P = D
  inpaint           x' = org (1 - m) + x' m,  org = signal inpaint_init + noise inpaint_noise   (the row's first two columns)
  counter           row = clamp(*step_ptr, 0, num_steps - 1) (NULL: 0) for the coefficients AND for step_noise; advance != 0
                    stores *step_ptr + 1 - the UNCLAMPED value plus one, so a counter outside the range stays outside it

1. Exact stage (`exact_problem`, `check_bits`).  Rows are dyadic (signal a power of two, the rest small multiples of 1/4; FRAC4 /
   FRAC8: no two rows share a value in any column, so a wrong row or a wrong column changes the result), the data small integers
   (latent in [-8, 8], u in [-3, 3], c - u in {-2, 0, 2}, guidance 7.5, z / P / inpaint_init / inpaint_noise in [-4, 4], mask in
   {0, 1/4, 1/2, 1}).  Every intermediate is then a float32, whether or not the compiler contracts a multiply-add, and the kernel
   must return the float64 reference's BITS in `latent` and `denoised_prev`.  AExact asserts the condition on every operation; a
   case that breaks it is an error of the case list.  Chained five-step runs use integer rows (INT4 / INT8: signal 1, the others in
   {+-1, +-2}) and a mask in {0, 1/2, 1}, so the fifth step is as exact as the first.

2. Moment stage (`moment_problem`, `check_factor`).  Integer u and c with u[b][0] = c[b][0], so that both of the kernel's shifts
   (c[0] and e[0]) are the data's centre; `moment_problem` asserts that sum |d| and sum d^2 stay below 2^24 for both tensors of
   every sample: fp32 then adds the four moments exactly in ANY order.  The factor is read back through the probe row {1, -1, 1, 0}
   on a zero latent (x' = fl(e factor)); for msd_sampler_step the probe is {1, -1, 0, 1, 0, 0, 0, 0}.  R, the fp32 roundings
   between the exact fp64 moments and `factor`, counted from the kernel's lines:
       std_text = (float)sqrt(vc)                                        1   (the cast; the fp64 square root is far below it)
       std_cfg  = (float)sqrt(vg) + 1e-5f                                2   (the cast, the sum)
       factor   = rescale * (std_text / std_cfg) + (1.0f - rescale)      4   (the quotient, the product, 1 - rescale, the sum)
   which is 7; one more unit is charged for the fp64 section (the sixteen wave sums are exact on these operands; m / n, the
   difference q / n - mean^2 - no cancellation about a central shift, asserted - and the square root are each 2^-53) and for the
   second-order terms of seven factors (1 + d): R = 8, the issue's count.  Division and square root are taken as correctly rounded,
   hipcc's default.  x' adds one rounding, so for every element with e != 0 the quotient x' / e lies within (R + 1) 2^-24 relative
   of the float64 factor, and - one factor per sample - the intervals [(x' -+ ulp / 2) / e] of a sample share a common point.

3. Real-operand stage (`real_problem`, `check_bound`).  randn operands on the project's own tables.  The bound is computed next to
   the float64 reference by AErr: every fp32 operation of the kernel's formula adds 2^-24 of its (bounded) result to what its
   operands carry; contraction only removes roundings; division and square root are charged as correctly rounded (hipcc's default:
   assumed, not tested).  The four moment sums are charged at depth (values per thread + 6 wave levels), never n.  A chained run
   carries the bound of step i's latent and P into step i + 1.  Underflow is not modelled (no operand here comes near it).

`form_of` restates the host rule: which of the three register forms (NPT 16, NPT 36, the re-reading loop NPT 0) a launch takes.

Plain numpy on the CPU.  Not a conftest: imported by name."""
import types
import zlib

import numpy as np

U = 2.0 ** -24
EPS32 = float(np.float32(1e-5))
R_FACTOR = 8
LIMIT = 1 << 24
OLD_RTOL = 2e-4          # test_cfg_step / test_sampler_step: rtol = 2e-4, atol = 2e-4 * max |ref|

# {signal, noise, A, B} / noise_coef: single steps from a preset counter
FRAC4 = np.array([[2, .5, 1.5, -.25], [.5, 1.5, .5, .5], [4, -.5, -1, .75], [1, 1, 2, -.5]], dtype=np.float32)
FRAC_NOISE = np.array([.5, -1, .25, 1.5], dtype=np.float32)
# {alpha, sigma, c_x, c_D, c_P, c_z, 0, 0}: row 0 has c_P = 0 (P starts as NaN there)
FRAC8 = np.array([[2, .5, 1.5, -.25, 0, .5, 0, 0], [.5, 1.5, .5, .5, -.5, -1, 0, 0], [4, -.5, -1, .75, 1.5, .25, 0, 0],
                  [1, 1, 2, -.5, .25, 1.5, 0, 0]], dtype=np.float32)
INT4 = np.array([[1, 1, 2, -1], [1, -1, 1, 2], [1, 2, -1, 1], [1, -2, -2, -1], [1, 1, 1, -2]], dtype=np.float32)
INT_NOISE = np.array([1, -1, 2, -2, 1], dtype=np.float32)
INT8 = np.array([[1, 1, 2, -1, 0, 1, 0, 0], [1, -1, 1, 2, -1, 2, 0, 0], [1, 2, -1, 1, 2, -1, 0, 0], [1, -2, -2, -1, 1, -2, 0, 0],
                 [1, 1, 1, -2, -2, 1, 0, 0]], dtype=np.float32)
PROBE = {"cfg": np.array([[1, -1, 1, 0]], dtype=np.float32), "multi": np.array([[1, -1, 0, 1, 0, 0, 0, 0]], dtype=np.float32)}

FAULTS = ("last quad", "other sample's factor", "unshifted moments", "noise row", "inpaint A B", "reads P", "row")


def rng(case_id):
    return np.random.default_rng(zlib.crc32(case_id.encode()))


def form_of(n, aligned=True):
    """NPT of the kernel form msd_cfg_step / msd_sampler_step launch: 16, 36 or 0 (the re-reading loop)."""
    vec4 = n % 4 == 0 and n >= 4 and aligned
    return 16 if vec4 and n <= 16 * 1024 else 36 if vec4 and n <= 36 * 1024 else 0


def per_thread(n, form):
    """The most values one thread adds into a moment."""
    return 4 * -(-(n // 4) // 1024) if form else -(-n // 1024)


# ---- the arithmetics -------------------------------------------------------------------------------------------------------------------
class A64:
    """float64: the reference."""
    def lift(self, x):
        return np.asarray(x, dtype=np.float64)

    def add(self, a, b):
        return a + b

    def sub(self, a, b):
        return a - b

    def mul(self, a, b):
        return a * b

    def div(self, a, b):
        return a / b

    def keep(self, new, old, sl):
        """new with the slice `sl` of the last axis taken from old (a fault's doing)."""
        new = np.array(new)
        new[..., sl] = old[..., sl]
        return new

    def value(self, x):
        return x


class AExact(A64):
    """float64 in which every operand and every result must be a float32.  `top`: the largest magnitude met."""
    def __init__(self, what):
        self.what, self.top, self.ops = what, 0.0, 0

    def _is_f32(self, r, op):
        r = np.asarray(r, dtype=np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            bad = ~np.isnan(r) & (r.astype(np.float32).astype(np.float64) != r)
        if bad.any():
            i = tuple(int(v) for v in np.argwhere(bad)[0])
            raise AssertionError(f"{self.what}: a {op} that is no float32 ({float(r[i])!r} at {i}; {int(bad.sum())} of {r.size}): the case is not exact")
        if r.size and not np.isnan(r).all():
            self.top = max(self.top, float(np.nanmax(np.abs(r))))
        self.ops += 1
        return r

    def lift(self, x):
        return self._is_f32(x, "operand")

    def add(self, a, b):
        return self._is_f32(a + b, "sum")

    def sub(self, a, b):
        return self._is_f32(a - b, "difference")

    def mul(self, a, b):
        return self._is_f32(a * b, "product")

    def div(self, a, b):
        return self._is_f32(a / b, "quotient")


class A32(A64):
    """numpy float32, one rounding per operation (no contraction): the kernel's formula as written."""
    def lift(self, x):
        return np.asarray(x, dtype=np.float32)

    def value(self, x):
        return x.astype(np.float64)


class AErr:
    """(float64 value, bound on |fp32 result - value|) pairs.  An operation's bound: what its operands carry, propagated, plus
    2^-24 of the largest result that admits."""
    def lift(self, x, err=0.0):
        v = np.asarray(x, dtype=np.float64)
        return v, np.zeros_like(v) + err

    @staticmethod
    def rnd(v, e):
        return v, e + U * (np.abs(v) + e)

    def add(self, a, b):
        return self.rnd(a[0] + b[0], a[1] + b[1])

    def sub(self, a, b):
        return self.rnd(a[0] - b[0], a[1] + b[1])

    def mul(self, a, b):
        return self.rnd(a[0] * b[0], np.abs(a[0]) * b[1] + np.abs(b[0]) * a[1] + a[1] * b[1])

    def div(self, a, b):
        den = np.abs(b[0]) - b[1]
        assert (den > 0).all(), "a divisor whose bound reaches zero"
        v = a[0] / b[0]
        return self.rnd(v, (a[1] + np.abs(v) * b[1]) / den)

    def keep(self, new, old, sl):
        raise NotImplementedError

    def value(self, x):
        return x[0]


# ---- the statement ----------------------------------------------------------------------------------------------------------------------
def clamp_row(counter, steps):
    """(row, what *step_ptr holds before the launch)."""
    raw = 0 if counter is None else int(counter)
    return min(max(raw, 0), steps - 1), raw


def walk(p, A, factors=None, fault=None):
    """p's launches under arithmetic A: [(latent, P or None, counter)] after each.  factors(i, u, c): the [B][1] rescale factors of
    launch i, lifted (None: the float64 ones, exact).  fault: one of FAULTS, for A32."""
    multi = p.kind == "multi"
    S = p.coef.shape[0]
    lat = A.lift(p.lat)
    P = A.lift(p.P0) if multi else None
    counter = p.step0
    cfg = p.guidance > 0
    res = []
    for i in range(p.launches):
        r, raw = clamp_row(counter, S)
        row = p.coef[raw % S if fault == "row" else r]
        rz = raw % S if fault == "noise row" else r
        sr, nr, ca, cb = (A.lift(v) for v in row[:4])
        u = A.lift(p.us[i])
        if cfg:
            c = A.lift(p.cs[i])
            e = A.add(u, A.mul(A.lift(np.float32(p.guidance)), A.sub(c, u)))
            if p.rescale > 0:
                f = factors(i, p.us[i], p.cs[i]) if factors else A.lift(factor64(p.us[i], p.cs[i], p.guidance, p.rescale)[:, None])
            else:
                f = A.lift(np.ones((p.B, 1)))
            e = A.mul(e, f)
        else:
            e = u
        d = A.div(A.sub(lat, A.mul(nr, e)), sr)
        if multi:
            x = A.add(A.mul(ca, lat), A.mul(cb, d))
            if row[4] != 0 or fault == "reads P":
                x = A.add(x, A.mul(A.lift(row[4]), P))
        else:
            x = A.add(A.mul(ca, d), A.mul(cb, e))
        if p.z is not None:
            cz = row[5] if multi else p.noise_coef[r]
            x = A.add(x, A.mul(A.lift(cz), A.lift(p.z[rz])))
        if p.ip is not None:
            init, noise, m = (A.lift(v) for v in p.ip)
            k0, k1 = (ca, cb) if fault == "inpaint A B" else (sr, nr)
            org = A.add(A.mul(k0, init), A.mul(k1, noise))
            x = A.add(A.mul(org, A.sub(A.lift(1.0), m)), A.mul(x, m))
        if fault == "last quad":
            x = A.keep(x, lat, slice(-4, None))
            if multi:
                d = A.keep(d, P, slice(-4, None))
        lat, P = x, (d if multi else None)
        if counter is not None and p.advance:
            counter = raw + 1
        res.append((lat, P, counter))
    return res


def reference(p):
    """The float64 reference of every launch; where p.exact, with AExact's assertions (p.top: the largest magnitude met)."""
    if getattr(p, "exact", False):
        A = AExact(p.id)
        res = walk(p, A)
        p.top = A.top
        return res
    return walk(p, A64())


# ---- the rescale factor -----------------------------------------------------------------------------------------------------------------
def guided(u, c, guidance):
    G = float(np.float32(guidance))
    u, c = np.asarray(u, dtype=np.float64), np.asarray(c, dtype=np.float64)
    return u + G * (c - u)


def factor64(u, c, guidance, rescale):
    """float64 [B]: the factor of every sample, from two-pass float64 deviations; guidance, rescale and 1e-5 at their fp32 values."""
    r = float(np.float32(rescale))
    g = guided(u, c, guidance)
    return r * (np.std(np.asarray(c, dtype=np.float64), axis=1) / (np.std(g, axis=1) + EPS32)) + (1.0 - r)


def _thread_rows(x, form):
    """x float32 [n] in the order the workgroup's 1024 threads add it: [values per thread][1024], zero-padded (adding 0 is exact)."""
    n = x.shape[0]
    if form:
        q = x.reshape(-1, 4)
        K = -(-q.shape[0] // 1024)
        q = np.concatenate([q, np.zeros((K * 1024 - q.shape[0], 4), dtype=x.dtype)])
        return q.reshape(K, 1024, 4).transpose(0, 2, 1).reshape(K * 4, 1024)
    K = -(-n // 1024)
    return np.concatenate([x, np.zeros(K * 1024 - n, dtype=x.dtype)]).reshape(K, 1024)


def _block_sum(x, form):
    """fp32 per thread, a 6-level fp32 tree per wave, the 16 wave sums in float64."""
    acc = np.zeros(1024, dtype=np.float32)
    for row in _thread_rows(x.astype(np.float32), form):
        acc = acc + row
    w = acc.reshape(16, 64)
    while w.shape[1] > 1:
        w = w[:, 0::2] + w[:, 1::2]
    return float(w[:, 0].astype(np.float64).sum())


def factor32(u, c, guidance, rescale, form, shifted=True):
    """float32 [B]: the kernel's lines in fp32 / fp64 as written.  shifted=False: one-pass moments about 0 (fault 3)."""
    G, r = np.float32(guidance), np.float32(rescale)
    out = np.zeros(len(u), dtype=np.float32)
    for b in range(len(u)):
        uu, cc = np.asarray(u[b], dtype=np.float32), np.asarray(c[b], dtype=np.float32)
        g = uu + G * (cc - uu)
        c0, g0 = (cc[0], g[0]) if shifted else (np.float32(0), np.float32(0))
        dc, dg = cc - c0, g - g0
        n = float(uu.shape[0])
        m = [_block_sum(v, form) for v in (dc, dc * dc, dg, dg * dg)]
        mc, mg = m[0] / n, m[2] / n
        vc, vg = max(m[1] / n - mc * mc, 0.0), max(m[3] / n - mg * mg, 0.0)
        std_text = np.float32(np.sqrt(vc))
        std_cfg = np.float32(np.sqrt(vg)) + np.float32(1e-5)
        out[b] = r * (std_text / std_cfg) + (np.float32(1) - r)
    return out


def factor_err(u, c, guidance, rescale, depth):
    """AErr pair [B][1]: the float64 factor and the bound on the kernel's, the moment sums charged at `depth` additions."""
    A = AErr()
    uu, cc = A.lift(u), A.lift(c)
    g = A.add(uu, A.mul(A.lift(np.float32(guidance)), A.sub(cc, uu)))
    dc = A.sub(cc, (cc[0][:, :1], cc[1][:, :1]))
    dg = A.sub(g, (g[0][:, :1], g[1][:, :1]))
    n = float(np.asarray(u).shape[1])
    gam = depth * U / (1 - depth * U)

    def total(x):
        return x[0].sum(1, keepdims=True), x[1].sum(1, keepdims=True) + gam * (np.abs(x[0]) + x[1]).sum(1, keepdims=True)

    def std(d):
        s, q = total(d), total(A.mul(d, d))
        var = q[0] / n - (s[0] / n) ** 2
        ev = q[1] / n + (2 * np.abs(s[0]) * s[1] + s[1] ** 2) / n ** 2 + 2.0 ** -48 * (q[0] / n)      # (the fp64 lines)
        v = np.sqrt(np.maximum(var, 0))
        return A.rnd(v, v - np.sqrt(np.maximum(var - ev, 0)))                                             # (the cast)

    ratio = A.div(std(dc), A.add(std(dg), A.lift(EPS32)))
    r = A.lift(np.float32(rescale))
    f = A.add(A.mul(r, ratio), A.sub(A.lift(1.0), r))
    ref = factor64(u, c, guidance, rescale)[:, None]
    return ref, f[1] + np.abs(f[0] - ref)


# ---- the draws --------------------------------------------------------------------------------------------------------------------------
def _ints(g, lo, hi, shape):
    return g.integers(lo, hi + 1, size=shape).astype(np.float32)


def exact_problem(kind, n, B=3, guidance=7.5, noise=False, inpaint=False, step0=0, chained=False, advance=2, case_id=None):
    """One exact-stage case.  chained: five launches from counter 0 on integer rows; else one launch from counter step0 on the
    fractional rows (step0 may lie outside 0..3, or be None for step_ptr = NULL)."""
    p = types.SimpleNamespace(kind=kind, n=n, B=B, guidance=guidance, rescale=0.0, step0=step0, advance=advance, exact=True)
    p.id = case_id or f"{kind}/n{n}/B{B}/g{guidance}/z{int(noise)}/ip{int(inpaint)}/s{step0}{'/chain' if chained else ''}"
    g = rng(p.id)
    multi = kind == "multi"
    p.coef = (INT8 if multi else INT4) if chained else (FRAC8 if multi else FRAC4)
    p.S = p.coef.shape[0]
    p.noise_coef = None if multi or not noise else (INT_NOISE if chained else FRAC_NOISE)
    p.launches = 5 if chained else 1
    p.lat = _ints(g, -8, 8, (B, n))
    p.us = [_ints(g, -3, 3, (B, n)) for _ in range(p.launches)]
    p.cs = [u + 2 * _ints(g, -1, 1, (B, n)) for u in p.us]
    p.z = _ints(g, -4, 4, (p.S, B, n)) if noise else None
    p.ip = None
    if inpaint:
        masks = np.array([0, .5, 1] if chained else [0, .25, .5, 1], dtype=np.float32)
        p.ip = (_ints(g, -4, 4, (n,)), _ints(g, -4, 4, (B, n)), masks[g.integers(0, len(masks), size=n)])
    p.P0 = None
    if multi:
        row = p.coef[clamp_row(step0, p.S)[0]]
        p.P0 = _ints(g, -4, 4, (B, n)) if row[4] != 0 else np.full((B, n), np.nan, dtype=np.float32)
    return p


def moment_problem(kind, n, rescale, B=3, guidance=None, mode="draw", offset=0, case_id=None):
    """Integer u, c whose four shifted moments are integers below 2^24 (asserted), on the probe row and a zero latent.
    mode "draw": different data per sample, element 0 of both tensors = offset (the shifts are central); "const c": c constant
    (std_text = 0: factor = 1 - rescale exactly); "const": u == c constant (std_cfg = 1e-5f)."""
    guidance = (7.5 if n <= 4100 else 4.0) if guidance is None else guidance
    p = types.SimpleNamespace(kind=kind, n=n, B=B, guidance=guidance, rescale=rescale, step0=0, advance=2, launches=1, z=None, ip=None,
                              noise_coef=None, coef=PROBE[kind], S=1, mode=mode)
    p.id = case_id or f"moments/{kind}/n{n}/r{rescale}/{mode}/o{offset}"
    g = rng(p.id)
    if mode == "const":
        u = np.full((B, n), 3.0, dtype=np.float32) + np.arange(B, dtype=np.float32)[:, None]
        c = u.copy()
    else:
        u = _ints(g, -2, 2, (B, n)) + np.float32(offset)
        step = 2 if guidance == 7.5 else 1
        c = u + step * _ints(g, -1, 1, (B, n)) if mode == "draw" else np.full((B, n), 2.0, dtype=np.float32) + np.float32(offset)
        if mode == "draw":
            u[:, 0] = c[:, 0] = offset
    p.us, p.cs = [u], [c]
    p.lat = np.zeros((B, n), dtype=np.float32)
    p.P0 = np.full((B, n), np.nan, dtype=np.float32) if kind == "multi" else None
    A = AExact(p.id)
    e = A.add(A.lift(u), A.mul(A.lift(np.float32(guidance)), A.sub(A.lift(c), A.lift(u))))
    p.sums = {}
    for name, t in (("c", np.asarray(c, dtype=np.float64)), ("e", e)):
        d = A.sub(t, t[:, :1])
        A.mul(d, d)
        s1, s2 = np.abs(d).sum(1).max(), (d * d).sum(1).max()
        assert s1 < LIMIT and s2 < LIMIT, f"{p.id}: sum |d| = {s1:.0f}, sum d^2 = {s2:.0f} of {name}: not below 2^24"
        if mode == "draw":    # (no cancellation in q / n - mean^2 about this shift)
            assert ((d.sum(1) / n) ** 2 <= (d * d).sum(1) / n / 2).all(), f"{p.id}: the shift of {name} is not central"
        p.sums[name] = (float(s1), float(s2))
    return p


def real_problem(kind, n, table, B=3, steps=5, guidance=7.5, rescale=0.7, noise=False, outlier=0.0, case_id=None):
    """randn operands on a real table (float [steps][4] / [steps][8]; cfg + noise: (table, noise_coef)), five chained launches.
    outlier: c[b][0] is moved that many standard deviations out."""
    p = types.SimpleNamespace(kind=kind, n=n, B=B, guidance=guidance, rescale=rescale, step0=0, advance=2, launches=steps, ip=None,
                              noise_coef=None, exact=False)
    p.id = case_id or f"real/{kind}/n{n}/B{B}/z{int(noise)}/o{outlier}"
    g = rng(p.id)
    if isinstance(table, tuple):
        table, p.noise_coef = table[0], np.asarray(table[1], dtype=np.float32)
    p.coef = np.asarray(table, dtype=np.float32)
    p.S = p.coef.shape[0]
    p.lat = g.standard_normal((B, n)).astype(np.float32)
    p.us = [g.standard_normal((B, n)).astype(np.float32) for _ in range(steps)]
    p.cs = [(u + 0.3 * g.standard_normal((B, n))).astype(np.float32) for u in p.us]
    if outlier:
        for c in p.cs:
            c[:, 0] = c.mean(1) + outlier * c.std(1)
    p.z = g.standard_normal((p.S, B, n)).astype(np.float32) if noise else None
    p.P0 = np.full((B, n), np.nan, dtype=np.float32) if kind == "multi" else None
    return p


def real_bound(p, form):
    """[(reference, bound)] for the latent and P of every launch: AErr over the whole chain."""
    depth = per_thread(p.n, form) + 6
    A = AErr()
    res = walk(p, A, factors=lambda i, u, c: factor_err(u, c, p.guidance, p.rescale, depth))
    return res


def emulate(p, form, fault=None):
    """What the kernel's formula leaves in numpy float32 (as written: no contraction), or what `fault` would."""
    def factors(i, u, c):
        f = factor32(u, c, p.guidance, p.rescale, form, shifted=fault != "unshifted moments")
        return (np.roll(f, 1) if fault == "other sample's factor" else f)[:, None]
    return walk(p, A32(), factors=factors, fault=fault)


# ---- the checkers -----------------------------------------------------------------------------------------------------------------------
def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)


def check_bits(got, ref, what):
    """got float32 against the float64 reference (every value a float32, asserted when it was made): the same bits."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    want = ref.astype(np.float32)
    if not np.array_equal(bits(got), bits(want)):
        bad = bits(got) != bits(want)
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} values differ in their bits from the float64 reference, first at {i}: "
                             f"got {float(got[i])!r}, reference {float(ref[i])!r}")


def check_run(got, ref, what, counter=True):
    """A whole run - [(latent, P, counter)] per launch - bit for bit."""
    assert len(got) == len(ref), what
    for i, ((gl, gp, gc), (rl, rp, rc)) in enumerate(zip(got, ref)):
        check_bits(gl, rl, f"{what}: latent after launch {i}")
        if rp is not None:
            check_bits(gp, rp, f"{what}: denoised_prev after launch {i}")
        if counter:
            assert gc == rc, f"{what}: the counter after launch {i} is {gc}, the statement gives {rc}"


def check_factor(x, p, what):
    """x float32 [B][n], the probe's latent: one factor per sample, within (R + 1) 2^-24 of the float64 one.  Returns the largest
    |x' / e - factor| / factor in units of 2^-24."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and np.isfinite(x).all(), f"{what}: a value that is not finite"
    u, c = p.us[0], p.cs[0]
    e = guided(u, c, p.guidance)
    f = factor64(u, c, p.guidance, p.rescale)[:, None]
    if p.mode != "draw":
        r = np.float32(p.rescale)
        check_bits(x, (e * float(np.float32(1) - r)).astype(np.float32).astype(np.float64), f"{what}: factor = 1 - rescale exactly")
        return 0.0
    nz = e != 0
    assert (x[~nz] == 0).all(), f"{what}: e = 0 gave a non-zero value"
    x64 = x.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(nz, np.abs(x64 / e / f - 1.0), 0.0)
    worst = rel.max() / U
    if worst > R_FACTOR + 1:
        b, i = (int(v) for v in np.argwhere(rel == rel.max())[0])
        raise AssertionError(f"{what}: sample {b}, element {i}: x' / e = {x64[b, i] / e[b, i]!r}, the float64 factor is {float(f[b, 0])!r}: "
                             f"{worst:.2f} x 2^-24 apart, the bound is {R_FACTOR + 1}")
    h = np.spacing(np.abs(x)).astype(np.float64) / 2
    with np.errstate(divide="ignore", invalid="ignore"):
        a, b_ = (x64 - h) / e, (x64 + h) / e
    lo = np.where(nz, np.minimum(a, b_), -np.inf).max(1)
    hi = np.where(nz, np.maximum(a, b_), np.inf).min(1)
    bad = lo > hi * (1 + 2.0 ** -50)
    assert not bad.any(), (f"{what}: sample {int(np.argwhere(bad)[0, 0])}: no single factor gives every element of the sample "
                           f"(the intervals end at {lo[bad][0]!r} > {hi[bad][0]!r})")
    return float(worst)


def check_bound(got, ref, bound, what):
    """|got - ref| <= bound, element for element.  Returns the largest measured / bound."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref.shape, what
    err = np.abs(got.astype(np.float64) - ref)
    bad = ~(err <= bound)
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} values miss the running-error bound, first at {i}: got {float(got[i])!r}, "
                             f"reference {float(ref[i])!r}, bound {float(bound[i]):.3g}")
    return float((err / bound).max())


def check_real(got, bound, what):
    """A chained run against real_bound's pairs.  Returns (measured / bound at its largest, the largest bound relative to max |ref|)."""
    worst = rel = 0.0
    for i, ((gl, gp, _), (rl, rp, _)) in enumerate(zip(got, bound)):
        worst = max(worst, check_bound(gl, rl[0], rl[1], f"{what}: latent after launch {i}"))
        rel = max(rel, float(rl[1].max() / np.abs(rl[0]).max()))
        if rp is not None:
            worst = max(worst, check_bound(gp, rp[0], rp[1], f"{what}: denoised_prev after launch {i}"))
    return worst, rel


def old_bound_accepts(got, ref):
    """test_cfg_step's / test_sampler_step's comparison."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return bool((np.abs(got - ref) <= OLD_RTOL * np.abs(ref).max() + OLD_RTOL * np.abs(ref)).all())
